"""GPU: generation stamps of a shard (HipIndexShard(..., generations=True); emdr2_mips_update_rows_stamped, _update_rows_scattered_stamped,
_generation_stats).  A newest-wins update leaves rows with a higher stamp alone, image and stamp, and the shard is still -- fp16 image,
emax_sq, int8 shadow image and its table -- byte for byte a fresh build of the rows it now holds; the numpy statements of the rule and of
the report are those of tests/test_index_generations_cpu.py.  Shapes: (1000, 64) has no shadow, a partial last block and padding to 1,024;
(9001, 256) is the smallest shape at which `_build` seals a shadow, its last block has 41 rows."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.test_index_generations_cpu import U64_NONE, apply_list, apply_range, stats_words
from tests.test_mips_i8_gpu import _assert_same
from tests.test_mips_update_gpu import _assert_identical_to_a_fresh_build, _build

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1000, 64, False, 0), (9001, 256, True, 70000)]


def _matrix(n, dim, seed):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, dim)).astype(np.float16)
    m[300] *= 8                                                          # `_build`'s recipe: row 300 holds emax_sq until it is overwritten
    return rng, m


def _stamped(m, row_base=0, generation=0):
    """`_build` with stamps"""
    from emdr2_amd.data.emdr2_index import HipIndexShard
    sh = HipIndexShard(m.shape[1], m.shape[0], row_base, shadow_min_rows=1, generations=True)
    sh.append_rows(m, generation=generation)
    return sh


def _dev_rows(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float16)).cuda()


def _dev_ids(ids):
    return torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).cuda()


def _plant(sh, stamps, rows, gens):
    """stamps of `rows` on the device and in the host copy"""
    stamps[rows] = gens
    sh.generation[torch.from_numpy(np.asarray(rows, dtype=np.int64)).cuda()] = torch.from_numpy(np.asarray(gens, dtype=np.int32)).cuda()


def _range(sh, m, stamps, lo, new, gen, newest_wins):
    """the update on the shard and, by the numpy rule, on the host copies; the counter must say what the rule says"""
    sh.update_rows(lo, _dev_rows(new), generation=gen, newest_wins=newest_wins)
    kept = apply_range(m, stamps, lo, new, gen, newest_wins)
    assert sh.kept_newer() == kept
    return kept


def _list(sh, m, stamps, ids, new, gen, newest_wins):
    ids = np.asarray(ids, dtype=np.int64)
    sh.update_rows_at(_dev_ids(ids), _dev_rows(new), generation=gen, newest_wins=newest_wins)
    kept = apply_list(m, stamps, ids, new, gen, newest_wins)
    assert sh.kept_newer() == kept
    return kept


def _check(sh, m, stamps, what, shadow):
    assert np.array_equal(sh.generation.cpu().numpy()[:m.shape[0]].astype(np.int64), stamps), "stamps differ %s" % what
    _assert_identical_to_a_fresh_build(sh, m, what, expect_shadow=shadow)
    audit = sh.audit()
    assert audit["sound"] and audit["canonical"], (what, audit)


@pytest.mark.parametrize("n,dim,shadow,row_base", SHAPES)
def test_range_update_leaves_newer_rows_alone(n, dim, shadow, row_base):
    rng, m = _matrix(n, dim, n + dim + 7)
    sh = _stamped(m, row_base)
    assert (sh._shadow is not None) == shadow
    stamps = np.zeros(n, dtype=np.int64)
    fresh = lambda k: rng.standard_normal((k, dim)).astype(np.float16)
    # generations 0, 5 and 9 in alternating rows of a range that crosses a block boundary
    rows = np.arange(128, 384)
    _plant(sh, stamps, rows, np.array([0, 5, 9])[(rows - 128) % 3])
    before = m.copy()
    kept = _range(sh, m, stamps, 128, fresh(256), 5, True)
    nines = int(((rows - 128) % 3 == 2).sum())
    assert kept == nines == 85
    assert (stamps[rows][(rows - 128) % 3 != 2] == 5).all() and (stamps[rows][(rows - 128) % 3 == 2] == 9).all()
    assert np.array_equal(m[rows[(rows - 128) % 3 == 2]], before[rows[(rows - 128) % 3 == 2]])
    assert not np.array_equal(m[rows[(rows - 128) % 3 != 2]], before[rows[(rows - 128) % 3 != 2]])
    _check(sh, m, stamps, "(range 128..383 at generation 5)", shadow)
    # newest_wins=False overwrites and re-stamps regardless, also downwards
    assert _range(sh, m, stamps, 120, fresh(270), 2, False) == 0
    assert (stamps[120:390] == 2).all()
    _check(sh, m, stamps, "(range 120..389 overwritten at generation 2)", shadow)
    # the partial last block and the last row, all newer / all older
    last_block = (n - 1) // 256 * 256
    _plant(sh, stamps, np.arange(last_block, n), 40)
    image = sh.tiled.clone()
    assert _range(sh, m, stamps, last_block, fresh(n - last_block), 39, True) == n - last_block
    torch.cuda.synchronize()
    assert torch.equal(sh.tiled, image)
    assert _range(sh, m, stamps, last_block, fresh(n - last_block), 40, True) == 0      # a tie writes
    _check(sh, m, stamps, "(the partial last block)", shadow)


@pytest.mark.parametrize("n,dim,shadow,row_base", SHAPES)
def test_list_update_leaves_newer_rows_alone(n, dim, shadow, row_base):
    rng, m = _matrix(n, dim, n + dim + 8)
    sh = _stamped(m, row_base)
    stamps = np.zeros(n, dtype=np.int64)
    fresh = lambda k: rng.standard_normal((k, dim)).astype(np.float16)
    rows = np.arange(128, 384)
    _plant(sh, stamps, rows, np.array([0, 5, 9])[(rows - 128) % 3])
    perm = rows[rng.permutation(256)]
    assert _list(sh, m, stamps, perm, fresh(256), 5, True) == 85
    _check(sh, m, stamps, "(permuted range 128..383 at generation 5)", shadow)
    # duplicates: the last occurrence decides and is then subject to the rule.  Row 7 (stamp 0) is named three times, row 130 (stamp 9:
    # 130 - 128 = 2) twice and stays; invalid ids -- -1, n, one in the zero padding, +-2^40 -- are skipped and not counted
    padded = (n + 511) // 512 * 512
    assert stamps[130] == 9 and padded - 1 >= n
    ids = np.array([7, 130, -1, 7, 600, n, 130, padded - 1, 7, -(1 << 40), 601, 1 << 40], dtype=np.int64)
    new = fresh(len(ids))
    assert _list(sh, m, stamps, ids, new, 6, True) == 1
    assert np.array_equal(m[7], new[8]) and stamps[7] == 6 and stamps[130] == 9 and stamps[600] == 6
    _check(sh, m, stamps, "(duplicates and invalid ids)", shadow)
    # a list whose rows are all newer: image and emax_sq are bit-equal to before
    newer = rows[(rows - 128) % 3 == 2][:40]
    image, emax = sh.tiled.clone(), sh.emax_sq.clone()
    assert _list(sh, m, stamps, newer[::-1], fresh(40), 8, True) == 40
    torch.cuda.synchronize()
    assert torch.equal(sh.tiled, image) and torch.equal(sh.emax_sq.view(torch.int32), emax.view(torch.int32))
    _check(sh, m, stamps, "(a list of newer rows only)", shadow)
    # an empty list, and a list of invalid ids only
    assert _list(sh, m, stamps, [], fresh(0), 8, True) == 0
    assert _list(sh, m, stamps, [-1, n, padded - 1], fresh(3), 8, True) == 0
    torch.cuda.synchronize()
    assert torch.equal(sh.tiled, image)
    # newest_wins=False through the list: overwritten and re-stamped, downwards too
    assert _list(sh, m, stamps, newer, fresh(40), 1, False) == 0
    assert (stamps[newer] == 1).all()
    _check(sh, m, stamps, "(newer rows overwritten at generation 1)", shadow)


@pytest.mark.parametrize("n,dim,shadow,row_base", SHAPES)
def test_emax_falls_only_when_the_row_that_held_it_is_really_overwritten(n, dim, shadow, row_base):
    rng, m = _matrix(n, dim, n + dim + 9)
    sh = _stamped(m, row_base)
    stamps = np.zeros(n, dtype=np.int64)
    fresh = lambda k: rng.standard_normal((k, dim)).astype(np.float16)
    high = float(sh.emax_sq)
    _plant(sh, stamps, [300], [9])                                       # the x8 row is newer than the writer
    assert _range(sh, m, stamps, 290, fresh(20), 5, True) == 1
    assert float(sh.emax_sq) == high
    _check(sh, m, stamps, "(x8 row newer than the range writer)", shadow)
    assert _list(sh, m, stamps, [299, 300, 301], fresh(3), 8, True) == 1
    assert float(sh.emax_sq) == high
    _check(sh, m, stamps, "(x8 row newer than the list writer)", shadow)
    assert _list(sh, m, stamps, [300], fresh(1), 9, True) == 0           # the same row no longer newer: emax_sq falls to the fresh build's value
    assert float(sh.emax_sq) < 0.25 * high
    _check(sh, m, stamps, "(x8 row replaced)", shadow)


def test_swap_refresh_stamps_the_whole_pass():
    n, dim = 9001, 256
    rng, m = _matrix(n, dim, 11)
    sh = _stamped(m, 0, generation=3)
    assert (sh.generation[:n] == 3).all()
    m2 = rng.standard_normal((n, dim)).astype(np.float16)
    sh.begin_refresh(generation=7)
    sh.refresh_rows(0, _dev_rows(m2[:4000]))
    assert (sh.generation[:n] == 3).all()                                # the image being searched keeps its stamps until the swap
    sh.refresh_rows(4000, _dev_rows(m2[4000:]))
    sh.commit_refresh()
    stamps = np.full(n, 7, dtype=np.int64)
    assert np.array_equal(sh.generation.cpu().numpy()[:n], stamps)
    image = sh.tiled.clone()
    fresh = rng.standard_normal((300, dim)).astype(np.float16)
    assert _range(sh, m2, stamps, 100, fresh, 6, True) == 300             # an older writer changes nothing
    assert _list(sh, m2, stamps, np.arange(5000, 5300), fresh, 6, True) == 300
    torch.cuda.synchronize()
    assert torch.equal(sh.tiled, image)
    _check(sh, m2, stamps, "(after a swap refresh at generation 7)", True)
    sh.begin_refresh(generation=8)                                       # the second pass reuses the spare stamp array
    sh.refresh_rows(0, _dev_rows(m))
    sh.commit_refresh()
    assert (sh.generation[:n] == 8).all()


def test_search_after_a_newest_wins_update_is_the_fresh_build_s():
    n, dim, nq, k = 9001, 256, 130, 20
    rng, m = _matrix(n, dim, 12)
    sh = _stamped(m, 70000)
    stamps = np.zeros(n, dtype=np.int64)
    rows = np.arange(0, n, 3)
    _plant(sh, stamps, rows, 9)
    _range(sh, m, stamps, 200, rng.standard_normal((5376, dim)).astype(np.float16), 5, True)
    ids = rng.choice(n, 640, replace=False)
    _list(sh, m, stamps, ids, rng.standard_normal((640, dim)).astype(np.float16), 5, True)
    assert sh._shadow is not None
    b = _build(m, row_base=70000, shadow=False)
    q = torch.from_numpy(rng.standard_normal((nq, dim)).astype(np.float16)).cuda()
    # the comparison of test_mips_i8_gpu._compare_all_entry_points (which also asserts whether the int8 scan ran: not this test's subject)
    for kw in ({"exact_fallback": False}, {}):
        _assert_same(sh.search(q, k, **kw), b.search(q, k, **kw), "(search %s)" % kw)
        _assert_same(sh.search_f32(q, k, **kw), b.search_f32(q, k, **kw), "(search_f32 %s)" % kw)
        for f32 in (False, True):
            ra, fa = sh.search_records(q, k, f32=f32, **kw)
            rb, fb = b.search_records(q, k, f32=f32, **kw)
            keep = (fa & 2) == 0
            assert torch.equal(fa & 2, fb & 2) and torch.equal(fa[keep], fb[keep]) and torch.equal(ra[keep], rb[keep]), "records differ (f32=%s %s)" % (f32, kw)


def _words(sh, now, global_rows=None):
    return [w & U64_NONE for w in sh.generation_report(now, global_rows).tolist()]


@pytest.mark.parametrize("n,row_base", [(1000, 0), (9001, 70000)])
def test_generation_stats_match_the_numpy_report_word_for_word(n, row_base):
    from emdr2_amd.data.emdr2_index import generation_result
    rng, m = _matrix(n, 64, n)
    sh = _stamped(m, row_base)
    stamps = np.zeros(n, dtype=np.int64)
    rows = np.arange(n)
    _plant(sh, stamps, rows, rng.integers(0, 5000, n))
    _plant(sh, stamps, [0, 1, 2, n - 1], [0, 4999, 5000, 4096])
    now = 5000
    assert _words(sh, now) == stats_words(stamps, now)                   # the whole shard; ages 0, 1, 904, 5000 are among them
    got = sh.generation_stats(now)
    want = generation_result(stats_words(stamps, now))
    assert got == want and got["count"] == n and got["min_age"] == 0 and got["max_age"] == 5000 and got["from_future"] == 0
    assert abs(got["mean_age"] - float((now - stamps).mean())) < 1e-9
    # a hit list [Q, k] with rows of other shards, negatives and a duplicate
    hits = row_base + rng.integers(0, n, (16, 8))
    hits[0, :4] = [-1, row_base - 1, row_base + n, row_base + 5]
    hits[1, :3] = [row_base + 5, -(1 << 40), 1 << 40]
    assert _words(sh, now, _dev_ids(hits)) == stats_words(stamps, now, row_base, hits)
    assert sh.generation_stats(now, _dev_ids(hits))["count"] == 16 * 8 - 5
    # n_sel == 0, and a list that names no row of this shard
    empty = stats_words(stamps, now, row_base, [])
    assert empty[:5] == [0, 0, U64_NONE, 0, 0] and sum(empty) == U64_NONE
    assert _words(sh, now, _dev_ids(np.zeros((0,), dtype=np.int64))) == empty
    assert _words(sh, now, _dev_ids([-1, row_base + n])) == empty
    # stamps above `now` count as age 0 and in word 4
    early = 2500
    w = _words(sh, early)
    assert w == stats_words(stamps, early) and w[4] == int((stamps > early).sum()) > 0


def test_an_unstamped_shard_behaves_as_before_and_refuses_the_keywords():
    n, dim = 9001, 256
    rng, m = _matrix(n, dim, 13)
    a, twin = _build(m.copy()), _stamped(m.copy())
    assert a.generation is None and a._kept_newer is None and a._spare_generation is None
    new, ids = rng.standard_normal((300, dim)).astype(np.float16), rng.choice(n, 300, replace=False)
    a.update_rows(250, _dev_rows(new)); twin.update_rows(250, _dev_rows(new), generation=4)
    a.update_rows_at(_dev_ids(ids), _dev_rows(new)); twin.update_rows_at(_dev_ids(ids), _dev_rows(new), generation=4, newest_wins=True)
    m[250:550] = new
    m[ids] = new
    torch.cuda.synchronize()
    assert torch.equal(a.tiled, twin.tiled) and torch.equal(a.emax_sq.view(torch.int32), twin.emax_sq.view(torch.int32))
    assert torch.equal(a._shadow[0], twin._shadow[0]) and torch.equal(a._shadow[1].view(torch.int32), twin._shadow[1].view(torch.int32))
    _assert_identical_to_a_fresh_build(a, m, "(unstamped)", expect_shadow=True)
    for call in (lambda: a.update_rows(0, _dev_rows(new), generation=1), lambda: a.update_rows(0, _dev_rows(new), newest_wins=True),
                 lambda: a.update_rows_at(_dev_ids(ids), _dev_rows(new), generation=1),
                 lambda: a.update_rows_at(_dev_ids(ids), _dev_rows(new), newest_wins=True), lambda: a.begin_refresh(generation=2),
                 lambda: a.generation_stats(5), a.kept_newer,
                 lambda: twin.update_rows(0, _dev_rows(new)), lambda: twin.update_rows_at(_dev_ids(ids), _dev_rows(new)),      # a stamped shard needs the generation
                 lambda: twin.update_rows(0, _dev_rows(new), generation=-1), lambda: twin.update_rows(0, _dev_rows(new), generation=1 << 31)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    _assert_identical_to_a_fresh_build(a, m, "(after the refused calls)", expect_shadow=True)


# -- two ranks on the one GPU over gloo: the reduced statistics --------------------------------------------------------------------------
def _two_rank_worker(rank, world, port):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex, generation_result
    n, dim = 2001, 64
    rng = np.random.default_rng(3)
    m = rng.standard_normal((n, dim)).astype(np.float16)
    index = DistributedBruteForceIndex(dim, None, generations=True)
    index.add_arrays(np.arange(1, n + 1, dtype=np.int32), m)
    lo, hi = index.local_rows()
    assert (lo, hi) == ((0, 1001) if rank == 0 else (1001, 2001)) and index.shard.generation is not None
    stamps = rng.integers(0, 900, n)
    stamps[1500] = 1200                                                  # beyond `now`, on rank 1's shard
    index.shard.generation[:hi - lo] = torch.from_numpy(stamps[lo:hi].astype(np.int32)).cuda()
    now = 1000
    assert index.generation_stats(now) == generation_result(stats_words(stamps, now))
    hits = rng.integers(-1, n, (8, 6))
    hits[0, :2] = hits[1, :2] = [7, 1999]                                # rows of both shards, named twice
    got = index.generation_stats(now, torch.from_numpy(hits).cuda())
    assert got == generation_result(stats_words(stamps, now, 0, hits)) and got["count"] == int((hits >= 0).sum())
    # a list that names rows of rank 0's shard only: rank 1 counts nothing and still reduces
    low = torch.from_numpy(rng.integers(0, 1001, (5,))).cuda()
    assert index.generation_stats(now, low) == generation_result(stats_words(stamps, now, 0, low.cpu().numpy()))
    assert index.generation_stats(now, torch.zeros((0,), dtype=torch.int64, device="cuda"))["count"] == 0
    # the keywords go through to the rank's shard
    new = torch.from_numpy(rng.standard_normal((10, dim)).astype(np.float16)).cuda()
    index.update_rows(lo + 3, new, generation=950, newest_wins=True)
    index.update_rows_at(torch.tensor([7, 1999, 1500], device="cuda"), new[:3], generation=1100, newest_wins=True)
    stamps[3:13] = stamps[1004:1014] = 950                               # each rank's own range
    stamps[[7, 1999]] = 1100                                             # row 1500 holds 1200 and stays
    assert index.kept_newer() == (1 if rank == 1 else 0)
    assert index.generation_stats(1100) == generation_result(stats_words(stamps, 1100))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_reduce_their_shards_statistics():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_two_rank_worker, args=(2, port), nprocs=2, join=True)
