"""GPU: in-place row updates of a finished shard (HipIndexShard.update_rows, emdr2_mips_update_rows).  An updated shard must hold, byte for
byte, what a shard freshly built from the same rows holds -- the fp16 image, emax_sq and, where there is one, the int8 shadow image and its
block table -- and must therefore search like it on every entry point, on the fp16 path and on the int8 path."""
import numpy as np
import pytest
import torch

from oracle import mips_oracle as mo
from tests.parity import assert_bit_identical
from tests.test_mips_gpu import _search
from tests.test_mips_i8_gpu import MIN_ROWS, _compare_all_entry_points

pytestmark = pytest.mark.gpu


def _build(rows, ids=None, row_base=0, shadow=True, min_rows=1):
    from emdr2_amd.data.emdr2_index import HipIndexShard
    sh = HipIndexShard(rows.shape[1], rows.shape[0], row_base, shadow=shadow, shadow_min_rows=min_rows)
    sh.append_rows(rows)
    if ids is not None:
        sh.set_ids(ids)
    return sh


def _update(sh, m, lo, new):
    """the update on the shard and on the host copy of its matrix"""
    new = np.ascontiguousarray(new, dtype=np.float16)
    sh.update_rows(lo, torch.from_numpy(new).cuda())
    m[lo:lo + new.shape[0]] = new


def _assert_identical_to_a_fresh_build(a, m, what, expect_shadow=None):
    b = _build(m, row_base=a.row_base, min_rows=a.shadow_min_rows)
    torch.cuda.synchronize()
    assert torch.equal(a.tiled, b.tiled), "fp16 image differs %s" % what
    assert torch.equal(a.emax_sq.view(torch.int32), b.emax_sq.view(torch.int32)), \
        "emax_sq %r, fresh build %r %s" % (float(a.emax_sq), float(b.emax_sq), what)
    assert (a._shadow is None) == (b._shadow is None), "shadow in use: %s, fresh build: %s %s" % (a._shadow is not None, b._shadow is not None, what)
    if expect_shadow is not None:
        assert (a._shadow is not None) == expect_shadow, what
    if a._shadow is not None:
        assert torch.equal(a._shadow[0], b._shadow[0]), "int8 image differs %s" % what
        assert torch.equal(a._shadow[1].view(torch.int32), b._shadow[1].view(torch.int32)), "block table differs %s" % what
    assert torch.equal(a.rows(np.arange(m.shape[0])).cpu(), torch.from_numpy(m)), "rows read back differ %s" % what
    return b


@pytest.mark.parametrize("n,dim,shadow,row_base", [(1000, 64, False, 0), (1000, 96, False, 0), (9001, 256, True, 70000), (9001, 768, True, 0)])
def test_updated_image_is_the_fresh_build_of_the_same_rows(n, dim, shadow, row_base):
    """The smallest shapes at which the update can go wrong: no shadow (dim 64: less than a wave of 8-element groups; 96: no multiple of a
    chunk pair) and a shadow whose last block has 41 rows; single rows at both ends, a range across a block boundary, exactly one stripe,
    the partial last block, the whole shard; then the planted cases."""
    rng = np.random.default_rng(n + dim)
    m = rng.standard_normal((n, dim)).astype(np.float16)
    m[300] *= 8                                                          # (a) holds emax_sq until it is overwritten
    ids = (rng.permutation(n) + 1).astype(np.int32) if row_base else None
    a = _build(m, ids=ids, row_base=row_base)
    assert (a._shadow is not None) == shadow
    fresh = lambda k: rng.standard_normal((k, dim)).astype(np.float16)
    last_block = (n - 1) // 256 * 256                                    # 8960 at n = 9001 (41 rows), 768 at n = 1000
    for lo, k in ((0, 1), (n - 1, 1), (250, 12), (128, 128), (last_block, n - last_block), (0, n)):
        _update(a, m, lo, fresh(k))                                      # (row 300 keeps the maximum until the whole-shard update)
        _assert_identical_to_a_fresh_build(a, m, "(rows %d..%d)" % (lo, lo + k - 1), expect_shadow=shadow)
    # (a) plant the maximum again, then overwrite it with an ordinary row: emax_sq must FALL to the fresh build's value
    _update(a, m, 300, fresh(1) * np.float16(8))
    _assert_identical_to_a_fresh_build(a, m, "(planted x8 row)", expect_shadow=shadow)
    high = float(a.emax_sq)
    _update(a, m, 300, fresh(1))
    _assert_identical_to_a_fresh_build(a, m, "(x8 row replaced)", expect_shadow=shadow)
    assert float(a.emax_sq) < 0.25 * high
    # (b) one row x16: the block's scale changes, so every int8 row of the block does
    before = a._shadow[0].clone() if shadow else None
    _update(a, m, 600, fresh(1) * np.float16(16))
    _assert_identical_to_a_fresh_build(a, m, "(x16 row)", expect_shadow=shadow)
    if shadow:
        assert not torch.equal(before, a._shadow[0]) and float(a._shadow[1][4 * 2]) > 0.2      # s_b of block 2 = amax / 127: ~0.035 before, ~16 x that now
    # (c) a whole block of zeros: the seal's amax == 0 branch
    _update(a, m, 512, np.zeros((256, dim), dtype=np.float16))
    _assert_identical_to_a_fresh_build(a, m, "(zero block)", expect_shadow=shadow)
    if shadow:
        assert a._shadow[1][4 * 2:4 * 3].tolist() == [0.0, 0.0, 0.0, 0.0]
    # (d) two updates of the same block, one after the other
    _update(a, m, 520, fresh(11))
    _update(a, m, 700, fresh(40))
    _assert_identical_to_a_fresh_build(a, m, "(same block twice)", expect_shadow=shadow)
    if ids is not None:                                                  # ids and row_base are untouched by updates
        q = rng.standard_normal((9, dim)).astype(np.float16)
        d, i, r, f = _search(a, q, 7)
        od, oi = mo.topk(m, q, 7, ids=ids, row_base=row_base)
        assert_bit_identical(d, i, od, oi)


@pytest.mark.parametrize("n,dim,nq,k", [(140000, 256, 130, 101), (73729, 768, 512, 50)])
def test_search_after_updates_where_the_int8_kernel_runs(n, dim, nq, k):
    """Updates inside the dense first segment, inside an int8 segment and up to the last row; every entry point then returns what a fresh
    fp16-only shard of the final rows returns, and the int8 scan really ran on the re-sealed blocks."""
    rng = np.random.default_rng(n)
    m = rng.standard_normal((n, dim)).astype(np.float16)
    q = torch.from_numpy(rng.standard_normal((nq, dim)).astype(np.float16)).cuda()
    a = _build(m, min_rows=MIN_ROWS)
    assert a._shadow is not None
    for lo, cnt in ((1000, 300), (50000, 5376), (n - 700, 700)):
        _update(a, m, lo, rng.standard_normal((cnt, dim)).astype(np.float16))
    assert a._shadow is not None
    b = _build(m, shadow=False)
    flags = b.search(q, k, exact_fallback=False)[3]
    assert int((flags & 2).sum()) == 0                                   # no query is left out of the comparison below
    _compare_all_entry_points(a, b, q, k, expect_int8=True)


@pytest.mark.parametrize("n,dim,nq,k", [(5000, 128, 16, 10), (9001, 256, 130, 20)])
def test_search_after_updates_against_the_oracle(n, dim, nq, k):
    """Independent arithmetic: the CPU oracle over the final rows (doc ids through a permuted id map, a non-zero row_base)."""
    rng = np.random.default_rng(dim)
    m = rng.standard_normal((n, dim)).astype(np.float16)
    m[n // 2] *= 8
    ids = (rng.permutation(n) + 1).astype(np.int32)
    a = _build(m, ids=ids, row_base=12345)
    for lo, cnt in ((0, 1), (250, 12), (n // 2 - 3, 7), (n - 41, 41)):
        _update(a, m, lo, rng.standard_normal((cnt, dim)).astype(np.float16))
    q = rng.standard_normal((nq, dim)).astype(np.float16)
    d, i, r, f = _search(a, q, k)
    od, oi = mo.topk(m, q, k, ids=ids, row_base=12345)
    assert_bit_identical(d, i, od, oi)
    assert not f.any()


def test_a_non_finite_update_takes_the_shard_off_its_shadow():
    rng = np.random.default_rng(5)
    n, dim, nq = 100_000, 256, 200
    m = rng.standard_normal((n, dim)).astype(np.float16)
    q = torch.from_numpy(rng.standard_normal((nq, dim)).astype(np.float16)).cuda()
    a = _build(m, min_rows=MIN_ROWS)
    assert a._shadow is not None
    new = rng.standard_normal((5, dim)).astype(np.float16)
    new[2, 3] = np.inf
    _update(a, m, 77_775, new)
    assert a._shadow is None and a._want_shadow
    b = _build(m, shadow=False)
    _compare_all_entry_points(a, b, q, 50, expect_int8=False)
    _update(a, m, 10, rng.standard_normal((5, dim)).astype(np.float16))  # a later finite update does not bring the stale shadow back
    assert a._shadow is None


def test_update_rows_interplay_with_filling_and_refresh_and_its_errors():
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex, HipIndexShard
    rng = np.random.default_rng(9)
    n, dim = 9001, 256
    m = rng.standard_normal((n, dim)).astype(np.float16)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float16)).cuda()
    sh = HipIndexShard(dim, n, 0, shadow_min_rows=1)
    sh.append_rows(m[:5000])
    with pytest.raises(RuntimeError):
        sh.update_rows(0, dev(m[:4]))                                    # not fully populated
    sh.append_rows(m[5000:])
    sh.update_rows(0, dev(m[:4]))
    for lo, rows in ((-1, dev(m[:4])), (n - 3, dev(m[:4])), (0, dev(m[:4]).float()), (0, torch.from_numpy(m[:4])), (0, dev(m[:4, :128]))):
        with pytest.raises(ValueError):
            sh.update_rows(lo, rows)
    m2 = rng.standard_normal((n, dim)).astype(np.float16)
    sh.begin_refresh()
    sh.refresh_rows(0, dev(m2[:4000]))
    with pytest.raises(RuntimeError):
        sh.update_rows(0, dev(m[:4]))                                    # a swap refresh is in progress: its commit would discard the update
    sh.refresh_rows(4000, dev(m2[4000:]))
    sh.commit_refresh()
    assert sh._block_norms is None                                       # the table described the image that was swapped out
    m2[6000] *= 8
    _update(sh, m2, 6000, m2[6000:6001].copy())
    _update(sh, m2, 6000, rng.standard_normal((1, dim)).astype(np.float16))
    _assert_identical_to_a_fresh_build(sh, m2, "(after a commit_refresh)", expect_shadow=True)
    # the index class maps global rows to the rank's shard and refuses ranges that leave it
    index = DistributedBruteForceIndex(dim, None)
    index.add_arrays(np.arange(1, n + 1, dtype=np.int32), m)
    index.update_rows(8990, dev(m2[:11]))
    assert torch.equal(index.shard.rows(np.arange(8990, 9001)).cpu(), torch.from_numpy(m2[:11]))
    with pytest.raises(ValueError):
        index.update_rows(8991, dev(m2[:11]))
    with pytest.raises(ValueError):
        index.update_rows(-1, dev(m2[:11]))
