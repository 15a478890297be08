"""GPU: scattered in-place row updates of a finished shard (HipIndexShard.update_rows_at, emdr2_mips_update_rows_scattered).  Whatever the
list -- any order, duplicates, ids of other shards -- an updated shard must hold, byte for byte, what a shard freshly built from the same rows
holds (fp16 image, emax_sq, int8 shadow image, block table) and must search like it on every entry point."""
import numpy as np
import pytest
import torch

from oracle import mips_oracle as mo
from tests.parity import assert_bit_identical
from tests.test_mips_gpu import _search
from tests.test_mips_i8_gpu import MIN_ROWS, _compare_all_entry_points
from tests.test_mips_update_gpu import _assert_identical_to_a_fresh_build, _build

pytestmark = pytest.mark.gpu


def _dev_rows(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float16)).cuda()


def _dev_ids(ids):
    return torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).cuda()


def _scatter(sh, m, ids, new):
    """the scattered update on the shard and, in list order (so that the last occurrence of a row wins), on the host copy of its matrix;
    ids outside [0, n) are skipped on both"""
    ids = np.asarray(ids, dtype=np.int64)
    new = np.ascontiguousarray(new, dtype=np.float16)
    assert ids.shape[0] == new.shape[0]
    sh.update_rows_at(_dev_ids(ids), _dev_rows(new))
    for i, r in enumerate(ids):
        if 0 <= r < m.shape[0]:
            m[r] = new[i]


@pytest.mark.parametrize("n,dim,shadow,row_base", [(1000, 64, False, 0), (1000, 96, False, 0), (9001, 256, True, 70000), (9001, 768, True, 0)])
def test_scattered_update_leaves_the_fresh_build_of_the_same_rows(n, dim, shadow, row_base):
    """The four shapes of the contiguous test (no shadow at dim 64 / 96; a shadow whose last block has 41 rows), every list shape the
    claim / append step can get wrong, then the planted cases of the contiguous test through lists."""
    rng = np.random.default_rng(n + dim + 1)
    m = rng.standard_normal((n, dim)).astype(np.float16)
    m[300] *= 8                                                          # holds emax_sq until it is overwritten
    a = _build(m, row_base=row_base)
    assert (a._shadow is not None) == shadow
    fresh = lambda k: rng.standard_normal((k, dim)).astype(np.float16)
    check = lambda what: _assert_identical_to_a_fresh_build(a, m, what, expect_shadow=shadow)
    n_blocks = (n + 255) // 256
    last_block = (n - 1) // 256 * 256
    keep300 = lambda ids: np.asarray([r for r in ids if r != 300], dtype=np.int64)   # (row 300 keeps the maximum until the whole-shard list)

    _scatter(a, m, [0], fresh(1)); check("(first row)")
    _scatter(a, m, [n - 1], fresh(1)); check("(last row)")
    _scatter(a, m, [n - 1, 0], fresh(2)); check("(both ends in one list)")
    ids = 512 + rng.permutation(256)[:12]
    _scatter(a, m, ids, fresh(12)); check("(12 rows inside one block)")
    ids = keep300(np.minimum(np.arange(n_blocks) * 256 + rng.integers(0, 256, n_blocks), n - 1))
    _scatter(a, m, ids[::-1], fresh(len(ids))); check("(one row in every block)")
    # a permuted range across a block boundary: also what the contiguous update of that range leaves on a second shard
    perm = 128 + rng.permutation(256)
    new = fresh(256)
    twin_m = m.copy()
    twin = _build(twin_m, row_base=row_base)
    _scatter(a, m, perm, new); check("(permuted range 128..383)")
    by_row = np.empty_like(new)
    by_row[perm - 128] = new
    twin.update_rows(128, _dev_rows(by_row))
    torch.cuda.synchronize()
    assert torch.equal(a.tiled, twin.tiled) and torch.equal(a.emax_sq.view(torch.int32), twin.emax_sq.view(torch.int32))
    if shadow:
        assert torch.equal(a._shadow[0], twin._shadow[0]) and torch.equal(a._shadow[1].view(torch.int32), twin._shadow[1].view(torch.int32))
    del twin
    _scatter(a, m, np.arange(last_block, n)[::-1], fresh(n - last_block)); check("(the partial last block)")
    # duplicates: last wins; row 7 is named three times, not next to each other
    ids = np.array([7, 600, 7, 601, 600, 7, 900], dtype=np.int64)
    new = fresh(len(ids))
    _scatter(a, m, ids, new); check("(duplicates)")
    assert np.array_equal(m[7], new[5]) and np.array_equal(m[600], new[4])
    # half the ids invalid: -1, n, n + 5 and one inside the zero padding (which torch.equal on the image checks stays zero)
    padded = (n + 511) // 512 * 512
    assert padded - 1 >= n
    ids = np.array([-1, 10, n, 700, n + 5, 11, padded - 1, 701, -(1 << 40), 12, 1 << 40, 13], dtype=np.int64)
    _scatter(a, m, ids, fresh(len(ids))); check("(half the ids invalid)")
    # nothing valid, and nothing at all: the shard is untouched, emax_sq included
    image, emax = a.tiled.clone(), a.emax_sq.clone()
    _scatter(a, m, [-1, n, padded - 1, n + 5], fresh(4))
    _scatter(a, m, [], fresh(0))
    torch.cuda.synchronize()
    assert torch.equal(a.tiled, image) and torch.equal(a.emax_sq.view(torch.int32), emax.view(torch.int32))
    check("(all-invalid and empty lists)")
    _scatter(a, m, np.arange(n)[::-1], fresh(n)); check("(the whole shard in reverse)")

    # (a) plant the maximum, then overwrite it with an ordinary row: emax_sq must FALL to the fresh build's value
    _scatter(a, m, [5, 300, 800], np.concatenate([fresh(1), fresh(1) * np.float16(8), fresh(1)])); check("(planted x8 row)")
    high = float(a.emax_sq)
    _scatter(a, m, [800, 300], fresh(2)); check("(x8 row replaced)")
    assert float(a.emax_sq) < 0.25 * high
    # (b) one row x16: the block's int8 scale changes, so every int8 row of the block does
    before = a._shadow[0].clone() if shadow else None
    _scatter(a, m, [600, 3], np.concatenate([fresh(1) * np.float16(16), fresh(1)])); check("(x16 row)")
    if shadow:
        assert not torch.equal(before, a._shadow[0]) and float(a._shadow[1][4 * 2]) > 0.2
    # (c) a whole block of zeros: the seal's amax == 0 branch
    _scatter(a, m, 512 + rng.permutation(256), np.zeros((256, dim), dtype=np.float16)); check("(zero block)")
    if shadow:
        assert a._shadow[1][4 * 2:4 * 3].tolist() == [0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("n,dim,nq,k", [(73729, 768, 512, 50)])
def test_search_after_scattered_updates_where_the_int8_kernel_runs(n, dim, nq, k):
    """Scattered rows inside the dense first segment, inside an int8 segment and in the last block; every entry point then returns what a
    fresh fp16-only shard of the final rows returns, and the int8 scan really ran on the re-sealed blocks."""
    rng = np.random.default_rng(n)
    m = rng.standard_normal((n, dim)).astype(np.float16)
    q = torch.from_numpy(rng.standard_normal((nq, dim)).astype(np.float16)).cuda()
    a = _build(m, min_rows=MIN_ROWS)
    assert a._shadow is not None
    last_block = (n - 1) // 256 * 256
    ids = np.concatenate([rng.choice(8192, 300, replace=False), 20000 + rng.choice(40000, 3000, replace=False), np.arange(last_block, n), [-1, n]])
    ids = ids[rng.permutation(len(ids))]
    _scatter(a, m, ids, rng.standard_normal((len(ids), dim)).astype(np.float16))
    assert a._shadow is not None
    b = _build(m, shadow=False)
    flags = b.search(q, k, exact_fallback=False)[3]
    assert int((flags & 2).sum()) == 0                                   # no query is left out of the comparison below
    _compare_all_entry_points(a, b, q, k, expect_int8=True)


def test_search_after_scattered_updates_against_the_oracle():
    """Independent arithmetic: the CPU oracle over the final rows (doc ids through a permuted id map, a non-zero row_base)."""
    n, dim, nq, k = 5000, 128, 16, 10
    rng = np.random.default_rng(dim + 1)
    m = rng.standard_normal((n, dim)).astype(np.float16)
    m[n // 2] *= 8
    ids = (rng.permutation(n) + 1).astype(np.int32)
    a = _build(m, ids=ids, row_base=12345)
    rows = np.concatenate([[0, n - 1, n // 2], rng.choice(np.arange(1, n - 1), 400, replace=False), [n // 2]])
    _scatter(a, m, rows, rng.standard_normal((len(rows), dim)).astype(np.float16))
    q = rng.standard_normal((nq, dim)).astype(np.float16)
    d, i, r, f = _search(a, q, k)
    od, oi = mo.topk(m, q, k, ids=ids, row_base=12345)
    assert_bit_identical(d, i, od, oi)
    assert not f.any()


def test_a_non_finite_scattered_update_takes_the_shard_off_its_shadow():
    rng = np.random.default_rng(6)
    n, dim = 9001, 256
    m = rng.standard_normal((n, dim)).astype(np.float16)
    a = _build(m)
    assert a._shadow is not None
    new = rng.standard_normal((5, dim)).astype(np.float16)
    new[2, 3] = np.inf
    _scatter(a, m, [8000, 17, 4000, 8999, 300], new)
    assert a._shadow is None and a._want_shadow
    torch.cuda.synchronize()
    assert torch.equal(a.rows(np.arange(n)).cpu().view(torch.int16), torch.from_numpy(m).view(torch.int16))
    _scatter(a, m, [10, 4001], rng.standard_normal((2, dim)).astype(np.float16))   # a later finite update does not bring the stale shadow back
    assert a._shadow is None
    _assert_identical_to_a_fresh_build(a, m, "(a shard with an inf row)", expect_shadow=False)


def test_update_rows_at_errors_and_the_index_class():
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex, HipIndexShard
    rng = np.random.default_rng(10)
    n, dim = 9001, 256
    m = rng.standard_normal((n, dim)).astype(np.float16)
    ids4 = _dev_ids([0, 1, 2, 3])
    sh = HipIndexShard(dim, n, 0, shadow_min_rows=1)
    sh.append_rows(m[:5000])
    with pytest.raises(RuntimeError):
        sh.update_rows_at(ids4, _dev_rows(m[:4]))                        # not fully populated
    sh.append_rows(m[5000:])
    sh.update_rows_at(ids4, _dev_rows(m[:4]))
    for rows_ids, rows in ((ids4, _dev_rows(m[:4]).float()), (ids4, torch.from_numpy(m[:4])), (ids4, _dev_rows(m[:4, :128])),
                           (ids4.cpu(), _dev_rows(m[:4])), (ids4.int(), _dev_rows(m[:4])), (ids4[:3], _dev_rows(m[:4])),
                           (ids4.view(2, 2), _dev_rows(m[:4]))):
        with pytest.raises(ValueError):
            sh.update_rows_at(rows_ids, rows)
    sh.begin_refresh()
    sh.refresh_rows(0, _dev_rows(m[:4000]))
    with pytest.raises(RuntimeError):
        sh.update_rows_at(ids4, _dev_rows(m[:4]))                        # a swap refresh is in progress: its commit would discard the update
    sh.refresh_rows(4000, _dev_rows(m[4000:]))
    sh.commit_refresh()
    m2 = m.copy()
    _scatter(sh, m2, [6000, 5, 8999], rng.standard_normal((3, dim)).astype(np.float16))
    _assert_identical_to_a_fresh_build(sh, m2, "(after a commit_refresh)", expect_shadow=True)
    # the index class maps global rows to the rank's shard; what is not in it is skipped
    index = DistributedBruteForceIndex(dim, None)
    index.add_arrays(np.arange(1, n + 1, dtype=np.int32), m)
    index.shard.row_base = 4000                                          # (as the second rank's shard of a larger index would be)
    new = rng.standard_normal((4, dim)).astype(np.float16)
    index.update_rows_at(_dev_ids([3999, 4000, 4000 + n - 1, 4000 + n]), _dev_rows(new))
    want = m.copy()
    want[0], want[n - 1] = new[1], new[2]
    assert torch.equal(index.shard.rows(np.arange(n)).cpu().view(torch.int16), torch.from_numpy(want).view(torch.int16))
