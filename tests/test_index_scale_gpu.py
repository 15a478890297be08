"""GPU: the index-maintenance kernels at the sizes where their paths change.

Every result is compared bit for bit with the references the project already has: `oldest_rows_reference`
(tests/test_index_oldest_cpu.py), the numpy generation report `stats_words` (tests/test_index_generations_cpu.py),
`_assert_identical_to_a_fresh_build` (tests/test_mips_update_gpu.py), the host `digest_rows` (emdr2_amd/data/emdr2_index.py) and the
audit's own report.  tests/test_index_scale_cpu.py owns the sizes, the stamp patterns and the (below, n_want) cases and proves, as
arithmetic, that each reaches the path named here:

  oldest_hist / _count / _write_kernel   524,289 rows: slabs of 2 chunks, 257 slabs, the last of one row; 1,050,001: 3 chunks, 342 slabs;
                                         2,626,916 (one rank's shard of the workload): 6 chunks, 428 slabs.  So the `for base` loops run
                                         again, `lt_before` / `eq_before` are carried from chunk to chunk, the early `break` fires (and
                                         must not), and the sum over the slabs in front takes a second lap of its 256-strided loop
  oldest_write_kernel, scalar loads      the stamps as a view 1, 2 and 3 words into a 16-byte-aligned allocation (9,001 and 1,050,001 rows)
  generation_stats_kernel                300,001 and 2,626,916 rows, a list of 400,000: the grid-stride loop behind the 512-workgroup
                                         cap (3 to 21 items per thread), sum_age beyond 2^40
  table_max_kernel                       1,172 blocks: the maximum planted in block 1,100 and in the partial last block 1,171
  pack_rows_at / block_norms<BlockList>  a touched-block list of all 1,172 blocks (cap == table blocks), of 1,500 blocks with one row each
  / seal_shadow<BlockList>               (cap == n_upd), of the 4,102 blocks the oldest-rows selection of 1,050,001 rows spreads over
  audit, export, digest, unpack,         one shard of 2,800,001 x 768 (4.3 GB of fp16 image, 2.15 GB of int8 shadow): rows whose segments
  pack_rows<STAMPED>, search             lie on both sides of 2^31 and of 2^32 bytes, block 10,937

What these tests found and what changed with them.  Nothing: all 147 cases passed at their first run on an MI355X against the kernels
as they were, and no product code changed.  That the cases could have failed was checked on the device as well as in the model of the CPU
module: three builds of csrc/mips_select.hip with one line of oldest_write_kernel changed each (the sum over the slabs in front taking one
lap only; the counts of a slab's first chunk not carried into its second; the chunk loop ending once `take` is reached although rows
below T follow) pass every case of tests/test_index_oldest_gpu.py and fail 38, 47 and 32 of the 128 oldest-rows cases here, among them the
case the CPU module names for each (1,050,001 ties_everywhere; 524,289 equal; 524,289 old_rows_only_in_last_chunks; all below 2^31).

Durations (one MI355X, `--durations=20`, the whole module 30 s for 147 cases).  The 2,800,001 x 768 fixture -- 4.3 GB generated and packed
on the device in blocks of 262,144 rows, the shadow sealed, every block copied to the host and digested there -- is built once, in 7.3 s:

  7.29 s  setup  the 2,800,001 x 768 shard (module scope)
  1.16 s  call   emax falls from a block beyond 1,024 [300,001 x 256]          1.16 s  a selection over 4,102 blocks feeds the writer
  1.04 s  call   oldest rows [2,626,916 full, per `below`: 0.99 .. 1.04 s]     0.68 s  scattered update of every block [300,001 x 256, stamped]
  0.65 s  call   scattered update of every block [300,001 x 256, unstamped]    0.58 s  misaligned stamps [1,050,001, offset 3; 0.57 s offset 1]
  0.49 s  call   oldest rows [2,626,916 small, per `below`: 0.46 .. 0.49 s]    0.48 s  newest-wins list, half the rows newer [300,001 x 256]
  0.36 s  call   oldest rows [1,050,001 full, per `below`: 0.34 .. 0.36 s]     0.34 s  generation statistics [2,626,916]
  0.28 s  call   one row in each of 1,500 blocks [400,001 x 64]                0.26 s  emax falls from a block beyond 1,024 [300,001 x 64]
  every other case, the tests on the large shard included: below 0.25 s
(the oldest-rows cases are one per `below` because the host reference sorts the stamps anew for every call: that, not the kernel, is
their time)
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_index_generations_cpu import U64_NONE, apply_list, stats_words
from tests.test_index_generations_gpu import _dev_ids, _dev_rows, _stamped
from tests.test_index_oldest_cpu import oldest_rows_reference
from tests.test_index_oldest_gpu import MASK, _Device
from tests.test_index_scale_cpu import (BIG_DIM, BIG_FILL_ROWS, BIG_N, FEED_N, MISALIGNED_SIZES, OLDEST_SIZES, PATTERNS, PLANTED_BLOCK, ROWS_A,
                                        ROWS_B, ROWS_C, SCATTER_ALL_BLOCKS, SCATTER_DISTINCT, STATS_N_SEL, STATS_SIZES, UPDATE_SHAPES, belows,
                                        n_wants, oldest_seed, scale_stamps)
from tests.test_mips_audit_gpu import _byte, _half
from tests.test_mips_scatter_update_gpu import _scatter
from tests.test_mips_update_gpu import _assert_identical_to_a_fresh_build, _build, _update

pytestmark = pytest.mark.gpu
ROW_BASE = (1 << 33) + 12345                                             # global rows beyond 2^33


# -- oldest rows ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device():
    dev = _Device()
    nbytes = ctypes.c_size_t()
    dev.native.check(dev.lib.emdr2_mips_oldest_rows_workspace_bytes(max(OLDEST_SIZES), ctypes.byref(nbytes)), "workspace_bytes")
    if nbytes.value > dev.ws.numel():
        dev.ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    return dev


@pytest.mark.parametrize("which_below", range(4), ids=("below_0", "below_min", "below_median", "below_2^31"))
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", OLDEST_SIZES)
def test_oldest_rows_with_slabs_of_several_chunks_is_the_reference_bit_for_bit(device, n, pattern, which_below):
    """(one case per `below`: the host reference sorts the stamps anew for every call, seconds at 2.6 M rows)"""
    stamps = scale_stamps(pattern, n, oldest_seed(n, pattern))
    gen = torch.from_numpy(stamps.astype(np.int32)).cuda()
    for below in belows(stamps)[which_below:which_below + 1]:
        for n_want in n_wants(pattern, n, stamps):
            rows, info = device(gen, ROW_BASE, below, n_want)
            ref_rows, ref_info = oldest_rows_reference(stamps, n_want, below, ROW_BASE)
            what = (n, pattern, below, n_want)
            print("n %7d %-29s below %10d want %7d -> selected %7d eligible %7d max stamp %d" % (what + tuple(info[:3])))
            assert info == ref_info, what
            assert np.array_equal(rows, ref_rows), what


@pytest.mark.parametrize("pattern", ("two_last", "full"))
def test_oldest_rows_at_three_chunks_per_slab_is_a_function_of_the_stamps_alone(device, pattern):
    n = 1050001
    stamps = scale_stamps(pattern, n, 3)
    gen = torch.from_numpy(stamps.astype(np.int32)).cuda()
    below = int(np.quantile(stamps, 0.8)) + 1
    first = device(gen, 77, below, 5000, raw=True)
    assert device(gen, 77, below, 5000, raw=True) == first               # the workspace as the first call left it
    dirty = torch.full_like(device.ws, 0xFF)
    assert device(gen, 77, below, 5000, ws=dirty, raw=True) == first     # a workspace of garbage: the call clears what it needs
    ref_rows, ref_info = oldest_rows_reference(stamps, 5000, below, 77)
    assert first == np.append(ref_rows, -7).tobytes() + np.array(ref_info, dtype=np.uint64).tobytes()


@pytest.mark.parametrize("offset", (1, 2, 3))
@pytest.mark.parametrize("n", MISALIGNED_SIZES)
def test_oldest_rows_of_stamps_that_are_only_four_byte_aligned(device, n, offset):
    """the write pass loads four stamps at once where it can: here it never can, and takes the scalar branch"""
    pattern = "two_last" if offset == 2 else "full"
    stamps = scale_stamps(pattern, n, n + offset)
    buf = torch.full((n + 8,), 0x7fffffff, dtype=torch.int32, device="cuda")      # (what lies around the view is never the oldest)
    assert buf.data_ptr() % 16 == 0
    gen = buf[offset:offset + n]
    gen.copy_(torch.from_numpy(stamps.astype(np.int32)))
    assert gen.data_ptr() % 16 == 4 * offset and gen.is_contiguous()
    for below in (int(np.median(stamps)), 1 << 31):
        for n_want in (1, 1025, n // 2, n):
            rows, info = device(gen, ROW_BASE, below, n_want)
            ref_rows, ref_info = oldest_rows_reference(stamps, n_want, below, ROW_BASE)
            assert info == ref_info and np.array_equal(rows, ref_rows), (n, offset, below, n_want)


def test_a_selection_over_4102_blocks_feeds_the_scattered_writer():
    """test_shard_oldest_rows_feeds_the_scattered_writer at a size where the touched-block list is long"""
    n, dim, base, g, want = FEED_N, 64, 5000, 4, 300000
    rng = np.random.default_rng(11)
    m = rng.standard_normal((n, dim), dtype=np.float32).astype(np.float16)
    sh = _stamped(m, row_base=base)
    stamps = rng.integers(0, 6, size=n)
    sh.generation[:n] = torch.from_numpy(stamps.astype(np.int32)).cuda()
    rows, info = sh.oldest_rows(want, below=g)
    ref_rows, ref_info = oldest_rows_reference(stamps, want, g, base)
    assert np.array_equal(rows.cpu().numpy(), ref_rows) and [int(w) & MASK for w in info.tolist()] == ref_info
    assert np.unique((ref_rows - base) >> 8).size > 4000                 # the list of touched blocks is that long
    new = rng.standard_normal((want, dim), dtype=np.float32).astype(np.float16)
    sh.update_rows_at(rows - base, _dev_rows(new), generation=g, newest_wins=True)
    assert sh.kept_newer() == 0                                          # nothing selected is newer than g
    expect = stamps.copy()
    expect[ref_rows - base] = g
    assert np.array_equal(sh.generation.cpu().numpy()[:n].astype(np.int64), expect)      # exactly the selected stamps rose
    m[ref_rows - base] = new
    assert np.array_equal(sh.rows(np.arange(n)).cpu().numpy(), m)
    audit = sh.audit()
    assert audit["sound"] and audit["canonical"], audit


# -- generation statistics --------------------------------------------------------------------------------------------------------------------------
def _aged_stamps(n, now, rng):
    """stamps whose ages at `now` fill every histogram bin from 0 to 31, with a few stamps above `now`"""
    bits = rng.integers(0, 32, size=n)                                   # the bit length of the age: the bin
    lo = np.where(bits == 0, 0, 1 << np.maximum(bits - 1, 0))
    hi = np.minimum(np.where(bits == 0, 1, 1 << bits), now + 1)
    stamps = now - rng.integers(lo, hi)
    stamps[rng.choice(n, size=40, replace=False)] = now + 1 + rng.integers(0, (1 << 31) - 1 - now, size=40)
    assert stamps.min() >= 0 and stamps.max() < 1 << 31
    return stamps


@pytest.mark.parametrize("n", STATS_SIZES)
def test_generation_stats_behind_the_workgroup_cap_match_the_numpy_report(n):
    from emdr2_amd import _native
    lib = _native.lib()
    rng = np.random.default_rng(n)
    now, row_base = (1 << 31) - 9, 70000
    stamps = _aged_stamps(n, now, rng)
    gen = torch.from_numpy(stamps.astype(np.int32)).cuda()

    def words(global_rows=None):
        report = torch.full((_native.GEN_WORDS,), -7, dtype=torch.int64, device="cuda")
        ids = None if global_rows is None else _dev_ids(global_rows)
        _native.check(lib.emdr2_mips_generation_stats(gen.data_ptr(), n, row_base, None if ids is None else ids.data_ptr(),
                                                      0 if ids is None else ids.numel(), now, report.data_ptr(), _native.stream_ptr()), "generation_stats")
        return [w & U64_NONE for w in report.tolist()]
    want = stats_words(stamps, now)
    assert want[0] == n and want[1] > 1 << 40 and want[4] == 40 and all(w > 0 for w in want[5:5 + 31]) and len(want) == 37
    assert words() == want
    # the list form: duplicates, negatives, rows of the shards on both sides
    hits = row_base + rng.integers(-50000, n + 50000, size=STATS_N_SEL)
    hits[:6] = [-1, -(1 << 40), 1 << 40, row_base - 1, row_base + n, row_base + n - 1]
    hits[6:12] = row_base + 5
    hits[-1] = row_base                                                  # the last item of the last lap
    want = stats_words(stamps, now, row_base, hits)
    assert STATS_N_SEL // 2 < want[0] < STATS_N_SEL and want[1] > 1 << 40 and want[4] > 0 and all(w > 0 for w in want[5:5 + 31])
    assert np.unique(hits).size < hits.size
    assert words(hits) == want


# -- updates beyond 1,024 blocks ----------------------------------------------------------------------------------------------------------------------
_BASE = {}


def _base_matrix(n, dim):
    """fp16 [n, dim] N(0, 1), made once per shape and never modified (the tests copy it)"""
    if (n, dim) not in _BASE:
        m = np.random.default_rng(n + dim).standard_normal((n, dim), dtype=np.float32).astype(np.float16)
        m.setflags(write=False)
        _BASE[(n, dim)] = m
    return _BASE[(n, dim)]


@pytest.mark.parametrize("n,dim,shadow", UPDATE_SHAPES)
def test_emax_falls_when_the_row_that_held_it_sat_in_a_block_beyond_1024(n, dim, shadow):
    rng = np.random.default_rng(n + dim + 1)
    m = _base_matrix(n, dim).copy()
    fresh = lambda k: rng.standard_normal((k, dim)).astype(np.float16)
    a = _build(m)
    assert (a._shadow is not None) == shadow
    for row in (PLANTED_BLOCK * 256 + 77, n - 1):                        # block 1,100; the partial last block 1,171
        for through_list in (False, True):
            write = (lambda r, x: _scatter(a, m, [r], x)) if through_list else (lambda r, x: _update(a, m, r, x))
            what = "(row %d through %s)" % (row, "update_rows_at" if through_list else "update_rows")
            write(row, fresh(1) * np.float16(8))
            _assert_identical_to_a_fresh_build(a, m, "planted " + what, expect_shadow=shadow)
            high = float(a.emax_sq)
            write(row, fresh(1))
            _assert_identical_to_a_fresh_build(a, m, "replaced " + what, expect_shadow=shadow)
            assert float(a.emax_sq) < 0.25 * high


def _ids_with_invalid(valid, n, rng):
    """`valid` with 10 % invalid ids interleaved: -1, n, the zero padding, +-2^40"""
    padded = (n + 511) // 512 * 512
    assert padded - 1 >= n
    bad = rng.choice(np.array([-1, n, padded - 1, n + 5, -(1 << 40), 1 << 40], dtype=np.int64), size=valid.size // 9)
    ids = np.concatenate([valid, bad])
    return ids[rng.permutation(ids.size)]


@pytest.mark.parametrize("stamped", (False, True))
@pytest.mark.parametrize("n,dim,shadow", UPDATE_SHAPES)
def test_scattered_update_that_claims_every_block(n, dim, shadow, stamped):
    rng = np.random.default_rng(n + dim + 2)
    m = _base_matrix(n, dim).copy()
    a = _stamped(m) if stamped else _build(m)
    assert (a._shadow is not None) == shadow
    valid = rng.choice(n, size=SCATTER_ALL_BLOCKS, replace=False)
    assert np.unique(valid >> 8).size == (n + 255) // 256                # every block of the table is claimed
    ids = _ids_with_invalid(valid, n, rng)
    new = rng.standard_normal((ids.size, dim), dtype=np.float32).astype(np.float16)
    if stamped:
        stamps = np.zeros(n, dtype=np.int64)
        a.update_rows_at(_dev_ids(ids), _dev_rows(new), generation=6, newest_wins=True)
        assert a.kept_newer() == apply_list(m, stamps, ids, new, 6, True) == 0
        assert np.array_equal(a.generation.cpu().numpy()[:n].astype(np.int64), stamps) and int(stamps.sum()) == 6 * SCATTER_ALL_BLOCKS
    else:
        _scatter(a, m, ids, new)
    _assert_identical_to_a_fresh_build(a, m, "(200,000 rows over every block, stamped=%s)" % stamped, expect_shadow=shadow)
    audit = a.audit()
    assert audit["sound"] and audit["canonical"], audit


def test_scattered_update_of_one_row_in_each_of_1500_blocks():
    n, dim, n_upd = SCATTER_DISTINCT
    rng = np.random.default_rng(n)
    m = _base_matrix(n, dim).copy()
    a = _build(m)
    blocks = rng.choice((n + 255) // 256, size=n_upd, replace=False)
    ids = np.minimum(blocks * 256 + rng.integers(0, 256, size=n_upd), n - 1)
    assert np.unique(ids >> 8).size == n_upd and (ids >> 8).max() >= 1024
    new = rng.standard_normal((n_upd, dim)).astype(np.float16)
    new[rng.integers(0, n_upd)] *= np.float16(8)                         # emax_sq rises to a row of this list
    _scatter(a, m, ids, new)
    _assert_identical_to_a_fresh_build(a, m, "(1,500 rows in 1,500 blocks)", expect_shadow=False)


@pytest.mark.parametrize("n,dim,shadow", UPDATE_SHAPES)
def test_newest_wins_list_update_in_which_half_the_rows_are_newer(n, dim, shadow):
    rng = np.random.default_rng(n + dim + 3)
    m = _base_matrix(n, dim).copy()
    a = _stamped(m)
    # newer than the writer: every row of the blocks 0, 4, 8, .. (none of them may be listed as touched) and every other row of the
    # blocks 1, 5, 9, ..
    rows = np.arange(n)
    newer = ((rows >> 8) % 4 == 0) | (((rows >> 8) % 4 == 1) & (rows % 2 == 0))
    stamps = np.where(newer, 9, 2).astype(np.int64)
    a.generation[:n] = torch.from_numpy(stamps.astype(np.int32)).cuda()
    valid = rng.choice(n, size=100000, replace=False)
    ids = _ids_with_invalid(valid, n, rng)
    new = rng.standard_normal((ids.size, dim), dtype=np.float32).astype(np.float16)
    new[:] *= np.float16(4)                                              # a kept row's block would show it: its norm entry and scale would move
    a.update_rows_at(_dev_ids(ids), _dev_rows(new), generation=5, newest_wins=True)
    kept = apply_list(m, stamps, ids, new, 5, True)
    assert kept == int(newer[valid].sum()) and 30000 < kept < 45000
    assert a.kept_newer() == kept
    assert np.array_equal(a.generation.cpu().numpy()[:n].astype(np.int64), stamps)
    _assert_identical_to_a_fresh_build(a, m, "(newest-wins list, %d of 100,000 rows kept)" % kept, expect_shadow=shadow)
    audit = a.audit()
    assert audit["sound"] and audit["canonical"], audit


# -- beyond 2 GiB and 4 GiB ---------------------------------------------------------------------------------------------------------------------------
class _BigShard(object):
    """2,800,001 x 768 with shadow and stamps, filled on the device from a seeded generator in blocks of 262,144 rows.  The generator is
    kept, not the rows: rows needed on the host are generated again, block by block.  `written` holds what the tests have written since."""
    SEED = 20240

    def __init__(self):
        from emdr2_amd.data.emdr2_index import HipIndexShard, digest_rows
        import time
        t0 = time.time()
        self.n, self.dim, self.row_base = BIG_N, BIG_DIM, ROW_BASE
        self.sh = HipIndexShard(self.dim, self.n, self.row_base, generations=True)
        self.block_digests = []
        for lo in range(0, self.n, BIG_FILL_ROWS):
            block = self.generated_block(lo // BIG_FILL_ROWS)
            self.sh.append_rows(block)
            self.block_digests.append(digest_rows(block.cpu().numpy(), self.row_base + lo))
        assert self.sh._shadow is not None and self.sh._filled == self.n and self.sh.tiled.numel() > 1 << 32
        assert self.sh._shadow[0].numel() > 1 << 31
        self.written = {}                                                # local row -> fp16 [dim], what a test wrote there
        self.stamped = {}                                                # local row -> stamp
        print("the %d x %d shard: filled, sealed and digested on the host in %.1f s" % (self.n, self.dim, time.time() - t0))

    def generated_block(self, b):
        g = torch.Generator(device="cuda")
        g.manual_seed(self.SEED + b)
        rows = min(BIG_FILL_ROWS, self.n - b * BIG_FILL_ROWS)
        return torch.randn((rows, self.dim), generator=g, device="cuda", dtype=torch.float16)

    def expected(self, rows):
        """the fp16 bits the shard must hold in local `rows` (any order) -> uint16 [len, dim]"""
        rows = np.asarray(rows, dtype=np.int64)
        out = np.empty((rows.size, self.dim), dtype=np.float16)
        for b in np.unique(rows // BIG_FILL_ROWS):
            sel = np.nonzero(rows // BIG_FILL_ROWS == b)[0]
            local = torch.from_numpy(rows[sel] - b * BIG_FILL_ROWS).cuda()
            out[sel] = self.generated_block(int(b))[local].cpu().numpy()
        for i, r in enumerate(rows.tolist()):
            if r in self.written:
                out[i] = self.written[r]
        return out.view(np.uint16)

    def apply_updates(self):
        """once: `update_rows` over A at generation 3, `update_rows_at` over a shuffled B + C with invalid ids at generation 4"""
        if self.written:
            return
        sh, n = self.sh, self.n
        rng = np.random.default_rng(5)
        a_rows = np.arange(*ROWS_A)
        new_a = (rng.standard_normal((a_rows.size, self.dim)) * 2).astype(np.float16)
        sh.update_rows(ROWS_A[0], _dev_rows(new_a), generation=3)
        for i, r in enumerate(a_rows.tolist()):
            self.written[r], self.stamped[r] = new_a[i], 3
        bc = rng.permutation(np.concatenate([np.arange(*ROWS_B), np.arange(*ROWS_C)]))
        padded = (n + 511) // 512 * 512
        ids = np.concatenate([bc, np.array([-1, n, padded - 1, n + 5, -(1 << 40), 1 << 40], dtype=np.int64)])
        ids = ids[rng.permutation(ids.size)]
        new = (rng.standard_normal((ids.size, self.dim)) * 2).astype(np.float16)
        sh.update_rows_at(_dev_ids(ids), _dev_rows(new), generation=4, newest_wins=True)
        assert sh.kept_newer() == 0
        for i, r in enumerate(ids.tolist()):
            if 0 <= r < n:
                self.written[r], self.stamped[r] = new[i], 4


@pytest.fixture(scope="module")
def big():
    shard = _BigShard()
    yield shard
    del shard.sh
    torch.cuda.empty_cache()


RANGES = {"A": ROWS_A, "B": ROWS_B, "C": ROWS_C}


def _bits(t):
    return t.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("name", sorted(RANGES))
def test_rows_on_both_sides_of_2_and_4_gib_read_back_export_and_digest(big, name):
    from emdr2_amd.data.emdr2_index import digest_rows
    lo, hi = RANGES[name]
    rows = np.arange(lo, hi)
    want = big.expected(rows)
    sh = big.sh
    shuffled = np.random.default_rng(lo).permutation(rows)
    assert np.array_equal(_bits(sh.rows(shuffled)), big.expected(shuffled))
    ids = np.concatenate([big.row_base + shuffled, [-1, big.row_base - 1, big.row_base + big.n, shuffled[0]]])      # the last four: not this shard's
    got = _bits(sh.rows_global(torch.from_numpy(ids).cuda()))
    assert np.array_equal(got[:-4], big.expected(shuffled)) and not got[-4:].any()
    assert np.array_equal(_bits(sh.export_rows(lo, hi - lo)), want)
    assert sh.digest(lo, hi - lo) == digest_rows(want.view(np.float16), big.row_base + lo)
    assert sh.digest(lo + 3, 5) == digest_rows(want.view(np.float16)[3:8], big.row_base + lo + 3)


def test_digest_of_the_whole_large_shard_is_the_combination_of_the_host_digests(big):
    from emdr2_amd.data.emdr2_index import combine_digests, digest_rows
    total, x = combine_digests(big.block_digests)
    if big.written:                                                      # rows a test has written since: their old digest out, their new one in
        rows = np.array(sorted(big.written))
        new = big.expected(rows).view(np.float16)
        written, big.written = big.written, {}
        old = big.expected(rows).view(np.float16)
        big.written = written
        for i, r in enumerate(rows.tolist()):
            so, xo = digest_rows(old[i:i + 1], big.row_base + r)
            sn, xn = digest_rows(new[i:i + 1], big.row_base + r)
            total, x = (total - so + sn) & MASK, x ^ xo ^ xn
    assert big.sh.digest() == (total, x)


def test_updates_of_rows_beyond_2_and_4_gib(big):
    sh, n = big.sh, big.n
    big.apply_updates()
    a_rows = np.arange(*ROWS_A)
    # reading back gives the new rows; the rows next to them are unchanged
    for lo, hi in RANGES.values():
        around = np.arange(max(lo - 140, 0), min(hi + 140, n))
        assert np.array_equal(_bits(sh.rows(around)), big.expected(around)), (lo, hi)
        assert np.array_equal(_bits(sh.export_rows(int(around[0]), around.size)), big.expected(around)), (lo, hi)
    assert sorted(big.written) == sorted(np.concatenate([a_rows, np.arange(*ROWS_B), np.arange(*ROWS_C)]).tolist())
    # the stamps of exactly those rows changed
    changed = torch.nonzero(sh.generation[:n]).flatten().cpu().numpy()
    assert np.array_equal(changed, np.array(sorted(big.stamped)))
    assert sh.generation[torch.from_numpy(changed).cuda()].tolist() == [big.stamped[r] for r in changed.tolist()]
    audit = sh.audit()
    assert audit["sound"] and audit["canonical"] and audit["rows_checked"] == n and audit["shadow_in_use"], audit
    assert audit["first_bad_row"] == U64_NONE and audit["first_bad_block"] == U64_NONE


def _clean(sh):
    from emdr2_amd import _native
    a = sh.audit()
    assert [a[w] for w in _native.AUDIT_NAMES] == [sh.n_rows] + [0] * 11 + [U64_NONE, U64_NONE], a
    assert a["sound"] and a["canonical"]


def test_planted_faults_beyond_4_gib_are_reported_with_their_exact_row_and_block(big):
    sh, n = big.sh, big.n
    big.apply_updates()                                                  # (the block-norm table exists after the first in-place update)
    _clean(sh)
    # a nonzero half in a padding row, behind the last row
    cell = _half(sh, n + 5, 3)
    cell.fill_(1)
    a = sh.audit()
    cell.fill_(0)
    assert a["pad_rows_nonzero"] == 1 and a["first_bad_row"] == big.row_base + n + 5 and a["sound"] is False and a["first_bad_block"] == U64_NONE, a
    assert sum(a[w] for w in ("nonfinite_rows", "rows_over_emax", "block_norm_low", "shadow_norm_low", "shadow_resid_low")) == 0, a
    _clean(sh)
    # one int8 byte off, in a row of B, at a byte of the int8 image beyond 2^31
    row, k = ROWS_B[0] + 20, big.dim - 1
    cell = _byte(sh, row, k)
    assert cell.data_ptr() - sh._shadow[0].data_ptr() > 1 << 31
    old = int(cell.item())
    cell.fill_(old + 1 if old < 100 else old - 1)
    a = sh.audit()
    cell.fill_(old)
    assert a["shadow_rows_noncanonical"] == 1 and a["first_bad_row"] == big.row_base + row and a["canonical"] is False, a
    assert a["pad_rows_nonzero"] == a["shadow_pad_rows_nonzero"] == a["shadow_table_noncanonical"] == a["block_norm_noncanonical"] == 0, a
    _clean(sh)
    # the norm entry of the last block too low
    block = (n - 1) >> 8
    assert block == 10937
    old = sh._block_norms[block].clone()
    sh._block_norms[block] = old * 0.5
    a = sh.audit()
    sh._block_norms[block] = old
    x = big.expected(np.arange(block * 256, n)).view(np.float16).astype(np.float64)
    low = np.nonzero((x * x).sum(axis=1) > float(np.float32(float(old) * 0.5)) * (1.001 * 1.001))[0]
    assert low.size > 0
    assert a["block_norm_low"] == low.size and a["block_norm_noncanonical"] == 1 and a["emax_noncanonical"] == 0 and a["first_bad_block"] == block, a
    assert a["first_bad_row"] == big.row_base + block * 256 + int(low[0]) and a["sound"] is False and a["canonical"] is False, a
    _clean(sh)


def test_search_of_the_large_shard_equals_the_all_exact_path(big):
    sh = big.sh
    big.apply_updates()
    nq, k = 16, 20
    rng = np.random.default_rng(9)
    q = rng.standard_normal((nq, big.dim)).astype(np.float16)
    # three queries whose best rows are known: a row of A, of B and the last row
    picked = {0: ROWS_A[0] + 7, 7: ROWS_B[0] + 20, 15: big.n - 1}
    for i, r in picked.items():
        q[i] = big.expected([r]).view(np.float16)[0]
    q = torch.from_numpy(q).cuda()
    dist, idx, row, flags = sh.search(q, k)
    sel = torch.tensor(sorted(picked), dtype=torch.int32, device="cuda")
    xd, xi, xr = torch.zeros_like(dist), torch.zeros_like(idx), torch.zeros_like(row)
    xf = torch.ones(nq, dtype=torch.int32, device="cuda")
    sh.search_exact(q, sel, k, xd, xi, xr, xf)
    torch.cuda.synchronize()
    for i, r in picked.items():
        assert torch.equal(dist[i].view(torch.int16), xd[i].view(torch.int16)) and torch.equal(row[i], xr[i]) and torch.equal(idx[i], xi[i]), i
        assert int(row[i, 0]) == big.row_base + r and int(xf[i]) == 0
    assert int((row < big.row_base).sum()) == 0 and int((row >= big.row_base + big.n).sum()) == 0
