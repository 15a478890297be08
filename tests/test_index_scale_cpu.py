"""CPU: why every size of tests/test_index_scale_gpu.py reaches the path it is there for, as arithmetic.

The index-maintenance kernels have loops and launch geometries that change only beyond the sizes the other suites use (slabs of several
chunks and more than 256 slabs in the oldest-rows select, the grid-stride loop behind the 512-workgroup cap of the generation
statistics, the second lap of table_max_kernel, touched-block lists of more than 1,024 entries, byte offsets beyond 2^31 and 2^32).
This module restates that launch arithmetic in Python, reads the constants it depends on out of the sources with regular expressions
(the way tests/test_abi.py reads the headers), and asserts for every (kernel, size) pair of the GPU module the condition it is named
for -- so a later change of a constant cannot quietly turn those tests back into small-shard tests.

It also holds a numpy model of the oldest-rows write pass WITH its geometry (per-slab counts of rows below / equal to the cut stamp T,
the prefix over the slabs in front, ranks that continue from chunk to chunk, `take`, the two uniform early exits).  The model equals
`oldest_rows_reference` at slabs of 1, 2 and 3 chunks; three faults planted in it are each caught by a named case of the GPU module and
pass every case of tests/test_index_oldest_gpu.py -- the evidence that the new cases close a gap the old ones leave open.

The stamp patterns, sizes and (below, n_want) cases of the GPU module are defined HERE, so both modules speak of the same cases."""
import os
import re

import numpy as np
import pytest

from tests.test_index_oldest_cpu import oldest_rows_reference
from tests.test_index_generations_cpu import U64_NONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "emdr2_amd", "csrc")


# -- the constants, read from the sources ---------------------------------------------------------------------------------------------------
def _source(name):
    return open(os.path.join(CSRC, name)).read()


def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, "%s: %d matches of %r" % (what, len(found), pattern)
    return found[0]


def _constants():
    select, aux, device, kernels = _source("mips_select.hip"), _source("mips_aux.hip"), _source("mips_device.h"), _source("mips_kernels.h")
    c = {}
    c["SEL_THREADS"] = int(_one(r"\bSEL_THREADS\s*=\s*(\d+)\s*,", select, "SEL_THREADS"))
    c["SEL_CHUNK"] = int(_one(r"\bSEL_CHUNK\s*=\s*(\d+)\s*\*\s*SEL_THREADS\s*,", select, "SEL_CHUNK")) * c["SEL_THREADS"]
    c["MAX_SLABS"] = int(_one(r"#define\s+MIPS_OLDEST_MAX_SLABS\s+(\d+)", kernels, "MIPS_OLDEST_MAX_SLABS"))
    # the lap of the write pass's sum over the slabs in front: `w += SEL_THREADS`
    assert re.search(r"for \(unsigned w = tid; w < blockIdx\.x; w \+= SEL_THREADS\)", select)
    stats = aux[aux.index("int mips_launch_generation_stats"):]
    stats = stats[:stats.index("\n}\n")]
    c["STATS_THREADS"] = int(_one(r"\(n_items \+ (\d+)\) / \d+", stats, "threads of the statistics grid")) + 1
    assert _one(r"\(n_items \+ \d+\) / (\d+)", stats, "threads of the statistics grid") == str(c["STATS_THREADS"])
    cap = _one(r"if \(blocks > (\d+)\) blocks = (\d+);", stats, "the block cap of the statistics grid")
    assert cap[0] == cap[1]
    c["STATS_MAX_BLOCKS"] = int(cap[0])
    assert _one(r"dim3\(\(unsigned\)blocks\), dim3\((\d+)\)", stats, "the statistics block") == str(c["STATS_THREADS"])
    tmax = aux[aux.index("__launch_bounds__(", aux.index("*emax_sq = max of the whole table")):]
    tmax = tmax[:tmax.index("\n}\n")]
    c["TABLE_MAX_THREADS"] = int(_one(r"__launch_bounds__\((\d+)\) table_max_kernel", tmax, "table_max_kernel's block"))
    assert _one(r"i < n_blocks; i \+= (\d+)\)", tmax, "table_max_kernel's stride") == str(c["TABLE_MAX_THREADS"])
    assert re.search(r"table_max_kernel, dim3\(1\), dim3\(%d\)" % c["TABLE_MAX_THREADS"], aux)
    c["STRIPE_ROWS"] = int(_one(r"#define\s+STRIPE_ROWS\s+(\d+)", device, "STRIPE_ROWS"))
    c["CHUNK_K"] = int(_one(r"#define\s+CHUNK_K\s+(\d+)", device, "CHUNK_K"))
    return c


C = _constants()
BLOCK_ROWS = 256                                                         # rows of a block of the norm table and of the int8 shadow (`row >> 8`)


def test_the_constants_are_the_ones_this_module_was_written_against():
    """not a requirement of the kernels -- a changed constant is a reason to read the size tables below again, and every condition below
    is asserted from the parsed values anyway"""
    assert C == {"SEL_THREADS": 256, "SEL_CHUNK": 1024, "MAX_SLABS": 512, "STATS_THREADS": 256, "STATS_MAX_BLOCKS": 512,
                 "TABLE_MAX_THREADS": 1024, "STRIPE_ROWS": 128, "CHUNK_K": 32}
    assert re.search(r"const unsigned b = \(unsigned\)\(row >> 8\);", _source("mips_aux.hip")) and BLOCK_ROWS == 1 << 8


# -- the launch arithmetic, restated ----------------------------------------------------------------------------------------------------------
def oldest_geometry(n_rows):
    """mips_launch_oldest_rows -> (chunks, per, slab, grid)"""
    chunks = (n_rows + C["SEL_CHUNK"] - 1) // C["SEL_CHUNK"]
    per = (chunks + C["MAX_SLABS"] - 1) // C["MAX_SLABS"]
    slab = per * C["SEL_CHUNK"]
    return chunks, per, slab, (n_rows + slab - 1) // slab


def stats_geometry(n_items):
    """mips_launch_generation_stats -> (workgroups, the most items one thread walks)"""
    blocks = min((n_items + C["STATS_THREADS"] - 1) // C["STATS_THREADS"], C["STATS_MAX_BLOCKS"])
    threads = blocks * C["STATS_THREADS"]
    return blocks, (n_items + threads - 1) // threads


def table_blocks(n_rows):
    return (n_rows + BLOCK_ROWS - 1) // BLOCK_ROWS


def table_max_laps(n_blocks):
    """mips_launch_table_max: one workgroup; -> the most entries one thread folds"""
    return (n_blocks + C["TABLE_MAX_THREADS"] - 1) // C["TABLE_MAX_THREADS"]


def tiled_seg_offset(row, seg, nch):
    """mips_device.h: the byte offset of the 16-byte segment `seg` (8 fp16 elements) of image row `row`; nch = dim / CHUNK_K"""
    stripe, ri = row // C["STRIPE_ROWS"], row % C["STRIPE_ROWS"]
    c, s = seg >> 2, seg & 3
    sp = s ^ ((ri >> 2) & 3)
    slots = C["STRIPE_ROWS"] * C["CHUNK_K"] * 2 // 16                   # 16-byte slots of one (stripe, chunk) block
    return ((stripe * nch + c) * slots + ri * 4 + sp) * 16


def row_offsets(row, dim):
    """(lowest, highest) byte offset of a segment of `row`"""
    offs = [tiled_seg_offset(row, seg, dim // C["CHUNK_K"]) for seg in range(dim // 8)]
    return min(offs), max(offs)


# -- the cases of the GPU module --------------------------------------------------------------------------------------------------------------
OLDEST_SIZES = (524289, 1050001, 2626916)
OLD_SIZES = (1000, 9001, 70001)                                          # tests/test_index_oldest_gpu.SIZES
OLD_PATTERNS = ("equal", "two_first", "two_last", "small", "full", "descending")
NEW_PATTERNS = ("cut_in_second_chunk", "old_rows_only_in_first_chunks", "old_rows_only_in_last_chunks", "ties_everywhere")
PATTERNS = OLD_PATTERNS + NEW_PATTERNS
MISALIGNED_SIZES = (9001, 1050001)
FEED_N = 1050001                                                         # the selection that feeds the scattered writer (dim 64)
STATS_SIZES = (300001, 2626916)
STATS_N_SEL = 400000
UPDATE_SHAPES = ((300001, 64, False), (300001, 256, True))               # (rows, dim, shadow)
PLANTED_BLOCK = 1100
SCATTER_DISTINCT = (400001, 64, 1500)                                    # (rows, dim, rows of the list: one per block)
SCATTER_ALL_BLOCKS = 200000                                              # distinct rows of the update that claims every block
BIG_N, BIG_DIM = 2800001, 768
BIG_FILL_ROWS = 262144
ROWS_A = (1398090, 1398121)                                              # [lo, hi): straddles 2^31 bytes
ROWS_B = (2796190, 2796221)                                              # straddles 2^32 bytes
ROWS_C = (BIG_N - 300, BIG_N)


def late_slab(n):
    """the slab the new patterns put their cut into: three in front of the last (beyond 256 where the grid is that long)"""
    return oldest_geometry(n)[3] - 3


def ties_slab(n):
    """ties_everywhere: the slab `take` ends in -- 300 where there are that many, else two in front of the last"""
    grid = oldest_geometry(n)[3]
    return 300 if grid > 301 else grid - 2


def _chunk_rows(n, which):
    """rows of the first (`which` = 0) or last existing (-1) chunk of every slab"""
    chunks, per, slab, grid = oldest_geometry(n)
    lo = np.arange(grid, dtype=np.int64) * slab
    if which == -1:
        hi = np.minimum(lo + slab, n)
        lo = lo + (hi - lo - 1) // C["SEL_CHUNK"] * C["SEL_CHUNK"]
    rows = (lo[:, None] + np.arange(C["SEL_CHUNK"])[None, :]).reshape(-1)
    return rows[rows < n]


def scale_stamps(pattern, n, seed):
    """int64 stamps of one case; the six old patterns are those of tests/test_index_oldest_gpu.py"""
    if pattern in OLD_PATTERNS:
        from tests.test_index_oldest_gpu import _stamps
        return _stamps(pattern, n, seed)
    chunks, per, slab, grid = oldest_geometry(n)
    rng = np.random.default_rng(seed)
    if pattern == "ties_everywhere":
        return np.full(n, 7, dtype=np.int64)
    s = np.full(n, 5, dtype=np.int64)
    if pattern == "cut_in_second_chunk":                                 # the old rows are the tail from row 500 of a late slab on
        s[late_slab(n) * slab + 500:] = 3
        return s
    rows = _chunk_rows(n, 0 if pattern == "old_rows_only_in_first_chunks" else -1)
    assert pattern in NEW_PATTERNS
    s[rows[rng.random(rows.size) < 0.5]] = 3
    return s


def n_wants(pattern, n, stamps):
    """{0, 1, 1,025, n // 2, n} and what a pattern adds to reach its path"""
    chunks, per, slab, grid = oldest_geometry(n)
    wants = [0, 1, 1025, n // 2, n]
    if pattern == "cut_in_second_chunk":
        wants.append(1025 + C["SEL_CHUNK"])                             # the cut one chunk further: the third chunk where a slab has three
    elif pattern in ("old_rows_only_in_first_chunks", "old_rows_only_in_last_chunks"):
        wants.append(int((stamps == 3).sum()) + 1)                      # every old row and ONE row of the cut stamp (row 0 or close to it)
    elif pattern == "ties_everywhere":
        wants.append(ties_slab(n) * slab + slab // 2 + 13)
    return wants


def belows(stamps):
    return [0, int(stamps.min()), int(np.median(stamps)), 1 << 31]


def oldest_seed(n, pattern):
    return n + len(pattern)


# -- the numpy model of the select WITH its geometry -------------------------------------------------------------------------------------------
UNWRITTEN = -7                                                           # a slot of the selected set that no workgroup stored


def oldest_rows_model(stamps, n_want, below, row_base=0, per=None, fault=None):
    """oldest_count_kernel / oldest_write_kernel as array arithmetic over [slab, chunk of the slab, row of the chunk].  T and `take` come
    from a sort (the digit passes have no geometry).  `per`: chunks per slab (default: the launch's).  fault: None, or
    "prefix_stops_at_256"  the sum over the slabs in front takes one lap of its SEL_THREADS-strided loop only,
    "carry_dropped"        the counts of a slab's first chunk are not carried into its second,
    "early_break"          the loop over a slab's chunks ends once `take` is reached, although rows below T follow.
    -> (rows int64 [n_want], the four report words)"""
    stamps = np.asarray(stamps, dtype=np.int64)
    n, chunk = stamps.size, C["SEL_CHUNK"]
    if per is None:
        per = oldest_geometry(n)[1]
    slab = per * chunk
    grid = (n + slab - 1) // slab
    eligible = stamps[stamps < below]
    k = min(n_want, eligible.size)
    out = np.full(n_want, UNWRITTEN, dtype=np.int64)
    out[k:] = -1
    if k == 0:
        return out, [0, int(eligible.size), U64_NONE, 0]
    T = int(np.partition(eligible, k - 1)[k - 1])
    take = k - int((eligible < T).sum())
    assert take >= 1
    padded = np.full(grid * slab, (1 << 32) - 1, dtype=np.int64)        # rows past the end are never below or equal to T
    padded[:n] = stamps
    padded = padded.reshape(grid, per, chunk)
    is_lt, is_eq = padded < T, padded == T
    lt_c, eq_c = is_lt.sum(axis=2), is_eq.sum(axis=2)                    # [grid, per]
    LT, EQ = lt_c.sum(axis=1), eq_c.sum(axis=1)                          # oldest_count_kernel: one pair per slab
    front = np.arange(grid)
    if fault == "prefix_stops_at_256":
        front = np.minimum(front, C["SEL_THREADS"])
    lt_front = np.concatenate([[0], np.cumsum(LT)])[front]
    eq_front = np.concatenate([[0], np.cumsum(EQ)])[front]
    skipped = (LT == 0) & ((EQ == 0) | (eq_front >= take))
    carry_lt, carry_eq = lt_c.copy(), eq_c.copy()                        # what a chunk adds to the running counts behind it
    if fault == "carry_dropped" and per > 1:
        carry_lt[:, 0] = 0
        carry_eq[:, 0] = 0
    lt_after = lt_front[:, None] + np.cumsum(carry_lt, axis=1)
    eq_after = eq_front[:, None] + np.cumsum(carry_eq, axis=1)
    lt_in, eq_in = lt_after - carry_lt, eq_after - carry_eq              # (under "carry_dropped" chunk 1 starts from the slab's prefix again)
    exists = (np.arange(grid)[:, None] * slab + np.arange(per)[None, :] * chunk) < n
    done = eq_after >= take
    if fault != "early_break":
        done &= lt_after == (lt_front + LT)[:, None]
    broke_before = np.cumsum(done, axis=1) - done > 0                    # a chunk in front of this one ended the loop
    run = exists & ~skipped[:, None] & ~broke_before
    lt_b = lt_in[:, :, None] + np.cumsum(is_lt, axis=2) - is_lt
    eq_b = eq_in[:, :, None] + np.cumsum(is_eq, axis=2) - is_eq
    pos = lt_b + np.minimum(eq_b, take)
    store = (is_lt | (is_eq & (eq_b < take))) & run[:, :, None] & (pos < n_want)
    rows = np.arange(grid * slab, dtype=np.int64).reshape(grid, per, chunk)
    out[pos[store]] = row_base + rows[store]
    return out, [k, int(eligible.size), T, 0]


FAULTS = ("prefix_stops_at_256", "carry_dropped", "early_break")
# the case of the GPU module that catches each planted fault: (n, pattern, below, n_want or a function of (n, stamps))
CAUGHT_BY = {
    "prefix_stops_at_256": (1050001, "ties_everywhere", 1 << 31, lambda n, s: n),
    "carry_dropped": (524289, "equal", 1 << 31, lambda n, s: n),
    "early_break": (524289, "old_rows_only_in_last_chunks", 1 << 31, lambda n, s: n // 2),
}


# -- 1. the sizes reach their paths -----------------------------------------------------------------------------------------------------------
def test_oldest_rows_sizes_reach_several_chunks_per_slab_and_more_than_256_slabs():
    assert [oldest_geometry(n)[1] for n in OLD_SIZES] == [1, 1, 1] and max(oldest_geometry(n)[3] for n in OLD_SIZES) == 69
    chunks, per, slab, grid = oldest_geometry(524289)
    assert (per, grid) == (2, 257) and 524289 - (grid - 1) * slab == 1  # a last slab of one row
    assert grid > C["SEL_THREADS"]
    chunks, per, slab, grid = oldest_geometry(1050001)
    assert per >= 3 and (per, grid) == (3, 342) and grid > C["SEL_THREADS"] and 0 < 1050001 - (grid - 1) * slab < slab
    chunks, per, slab, grid = oldest_geometry(2626916)
    assert (per, grid) == (6, 428) and grid > C["SEL_THREADS"] and 0 < 2626916 - (grid - 1) * slab < slab
    assert oldest_geometry(21015324)[3] <= C["MAX_SLABS"]               # the whole index on one device still fits the count table
    assert oldest_geometry(FEED_N)[1] >= 3 and oldest_geometry(MISALIGNED_SIZES[0])[1] == 1 and oldest_geometry(MISALIGNED_SIZES[1])[1] == 3
    # a chunk holds at most SEL_CHUNK rows of either kind: the packed 16-bit counts of the write pass cannot carry
    assert C["SEL_CHUNK"] < 1 << 16


@pytest.mark.parametrize("n", OLDEST_SIZES)
def test_the_new_patterns_put_their_cut_where_they_say(n):
    chunks, per, slab, grid = oldest_geometry(n)
    chunk = C["SEL_CHUNK"]
    where = lambda row: (row // slab, row % slab // chunk)              # (slab, chunk of the slab)
    # cut_in_second_chunk: 1,025 -> the second chunk of the late slab; one chunk further -> its third chunk where a slab has three
    s = scale_stamps("cut_in_second_chunk", n, oldest_seed(n, "cut_in_second_chunk"))
    old = np.nonzero(s == 3)[0]
    assert set(np.unique(s)) == {3, 5} and old.size > 1025 + chunk
    assert where(old[1024]) == (late_slab(n), 1) and late_slab(n) >= 254
    assert where(old[1024 + chunk]) == ((late_slab(n), 2) if per >= 3 else (late_slab(n) + 1, 0))
    assert s[old[1024] + 1] == 3                                         # rows of the cut stamp follow the cut in its chunk: `take` decides
    assert 1025 + chunk in n_wants("cut_in_second_chunk", n, s)
    # old rows only in the first / last chunks of their slabs; behind the cut of n // 2 every selected row is such a row
    for pattern, which in (("old_rows_only_in_first_chunks", 0), ("old_rows_only_in_last_chunks", -1)):
        s = scale_stamps(pattern, n, oldest_seed(n, pattern))
        old = np.nonzero(s == 3)[0]
        last_of_slab = (np.minimum((old // slab + 1) * slab, n) - 1) % slab // chunk
        assert (old % slab // chunk == (0 if which == 0 else last_of_slab)).all()
        assert np.unique(old // slab).size >= grid - 1 and old.size < n // 2
        assert (np.bincount(old // slab, minlength=grid)[:grid - 1] > 100).all()
        rows, info = oldest_rows_reference(s, n // 2, 1 << 31)
        cut = int(rows[(s[rows] == 5)].max())                            # the last row of the cut stamp that is selected
        behind = rows[rows > cut]
        assert info[2] == 5 and behind.size > 0 and (s[behind] == 3).all() and np.unique(behind // slab).size > grid // 3
        extra = n_wants(pattern, n, s)[-1]
        rows, info = oldest_rows_reference(s, extra, 1 << 31)
        assert info[2] == 5 and int((s[rows] == 5).sum()) == 1 and rows[s[rows] == 5][0] < slab      # the cut lies in slab 0
    s = scale_stamps("ties_everywhere", n, 0)
    want = n_wants("ties_everywhere", n, s)[-1]
    assert where(want - 1)[0] == ties_slab(n) and where(want)[0] == ties_slab(n) and (ties_slab(n) == 300 or n == 524289)
    assert 0 < want < n


def test_generation_statistics_sizes_walk_the_grid_stride_loop():
    assert max(stats_geometry(n)[1] for n in (1000, 9001)) == 1         # the sizes of tests/test_index_generations_gpu.py
    per_lap = C["STATS_MAX_BLOCKS"] * C["STATS_THREADS"]
    for n_items in STATS_SIZES + (STATS_N_SEL,):
        blocks, laps = stats_geometry(n_items)
        assert blocks == C["STATS_MAX_BLOCKS"] and n_items / per_lap > 1 and laps >= 3, n_items
    assert stats_geometry(2626916)[1] == 21


def test_table_max_and_touched_block_lists_go_beyond_1024_blocks():
    assert table_max_laps(table_blocks(140000)) == 1 and table_blocks(73729) == 289      # the largest shards of the update suites
    for n, dim, shadow in UPDATE_SHAPES:
        nb = table_blocks(n)
        assert nb == 1172 and nb > C["TABLE_MAX_THREADS"] and table_max_laps(nb) == 2
        assert C["TABLE_MAX_THREADS"] <= PLANTED_BLOCK < nb - 1 and (n - 1) // BLOCK_ROWS == nb - 1 >= C["TABLE_MAX_THREADS"]
        assert n % BLOCK_ROWS != 0                                      # the last block is partial
        assert SCATTER_ALL_BLOCKS >= nb                                 # cap = min(n_upd, table blocks) = table blocks
    n, dim, n_upd = SCATTER_DISTINCT
    assert table_blocks(n) >= n_upd > 1024                              # one row per block: cap == n_upd, a list longer than 1,024
    # the selection that feeds the scattered writer: its rows spread over more than 1,024 blocks
    assert table_blocks(FEED_N) > 4 * 1024


def test_the_large_shard_has_rows_on_both_sides_of_2_gib_and_4_gib():
    nch = BIG_DIM // C["CHUNK_K"]
    assert nch == 24 and tiled_seg_offset(0, 0, nch) == 0 and tiled_seg_offset(C["STRIPE_ROWS"], 0, nch) == C["STRIPE_ROWS"] * BIG_DIM * 2
    assert sorted(tiled_seg_offset(5, seg, 1) for seg in range(4)) == [5 * 64 + 16 * j for j in range(4)]   # the swizzle permutes inside a row's 64 bytes
    for (lo, hi), limit in ((ROWS_A, 1 << 31), (ROWS_B, 1 << 32)):
        for row in range(lo, hi):                                        # every row of the set has segments on both sides
            low, high = row_offsets(row, BIG_DIM)
            assert low < limit <= high, (row, low, high)
    low, high = row_offsets(BIG_N - 1, BIG_DIM)
    padded = (BIG_N + 511) // 512 * 512
    assert (1 << 32) < low and high + 16 <= padded * BIG_DIM * 2
    assert ROWS_C[0] > ROWS_B[1] and table_blocks(BIG_N) - 1 == 10937 and (BIG_N - 1) // BLOCK_ROWS == 10937
    # the int8 shadow image (dim bytes per row, 16-element groups, dim / 64 chunks) crosses 2^31 inside the rows of set B
    for row in range(*ROWS_B):
        offs = [tiled_seg_offset(row, g, BIG_DIM // 64) for g in range(BIG_DIM // 16)]
        assert min(offs) < (1 << 31) <= max(offs), row
    # the fill: blocks of BIG_FILL_ROWS rows, a multiple of a stripe, so no block's rows share a stripe with the next
    assert BIG_FILL_ROWS % 512 == 0 and BIG_N > 10 * BIG_FILL_ROWS


# -- 2. the model is the reference; the planted faults -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", (1, 2, 3))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_model_equals_the_reference_at_slabs_of_one_two_and_three_chunks(pattern, per):
    """70,001 rows in slabs of 1, 2 and 3 chunks (69, 35 and 23 slabs); the new patterns, which follow the slabs, are laid out for `per`"""
    n = 70001
    stamps = scale_stamps(pattern, n, oldest_seed(n, pattern)) if pattern in OLD_PATTERNS else None
    if stamps is None:                                                   # lay the pattern out for `per` chunks per slab at this size
        stamps = _small_layout(pattern, n, per)
    for below in belows(stamps):
        for n_want in (0, 1, 64, 1025, n // 2, n - 1, n):
            got = oldest_rows_model(stamps, n_want, below, 1 << 33, per=per)
            want = oldest_rows_reference(stamps, n_want, below, 1 << 33)
            assert got[1] == want[1] and np.array_equal(got[0], want[0]), (pattern, per, below, n_want)


def _small_layout(pattern, n, per):
    slab = per * C["SEL_CHUNK"]
    grid = (n + slab - 1) // slab
    rng = np.random.default_rng(per)
    if pattern == "ties_everywhere":
        return np.full(n, 7, dtype=np.int64)
    s = np.full(n, 5, dtype=np.int64)
    if pattern == "cut_in_second_chunk":
        s[(grid - 3) * slab + 500:] = 3
        return s
    lo = np.arange(grid) * slab
    if pattern == "old_rows_only_in_last_chunks":
        lo = lo + (np.minimum(lo + slab, n) - lo - 1) // C["SEL_CHUNK"] * C["SEL_CHUNK"]
    rows = (lo[:, None] + np.arange(C["SEL_CHUNK"])[None, :]).reshape(-1)
    rows = rows[rows < n]
    s[rows[rng.random(rows.size) < 0.5]] = 3
    return s


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", OLDEST_SIZES[:2])
def test_model_equals_the_reference_at_the_launch_geometry(n, pattern):
    """2 chunks and 257 slabs, 3 chunks and 342 slabs: the patterns as the GPU module lays them out"""
    stamps = scale_stamps(pattern, n, oldest_seed(n, pattern))
    for below in (int(np.median(stamps)), 1 << 31):
        for n_want in n_wants(pattern, n, stamps)[2:]:
            got = oldest_rows_model(stamps, n_want, below, 77)
            want = oldest_rows_reference(stamps, n_want, below, 77)
            assert got[1] == want[1] and np.array_equal(got[0], want[0]), (pattern, below, n_want)


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_caught_by_a_new_case_and_missed_by_every_old_one(fault):
    n, pattern, below, want_of = CAUGHT_BY[fault]
    assert n in OLDEST_SIZES and pattern in PATTERNS
    stamps = scale_stamps(pattern, n, oldest_seed(n, pattern))
    n_want = want_of(n, stamps)
    assert below in belows(stamps) and n_want in n_wants(pattern, n, stamps)       # a case the GPU module runs
    want = oldest_rows_reference(stamps, n_want, below, 1 << 33)
    good = oldest_rows_model(stamps, n_want, below, 1 << 33)
    assert good[1] == want[1] and np.array_equal(good[0], want[0])
    bad = oldest_rows_model(stamps, n_want, below, 1 << 33, fault=fault)
    wrong = int((bad[0] != want[0]).sum())
    print("%s: %d of %d slots wrong at n = %d, %s, below %d, n_want %d" % (fault, wrong, n_want, n, pattern, below, n_want))
    assert wrong > 0
    # every case of tests/test_index_oldest_gpu.py: the faulty model is still the reference
    from tests.test_index_oldest_gpu import PATTERNS as old_patterns, SIZES as old_sizes, _stamps
    assert tuple(old_sizes) == OLD_SIZES and tuple(old_patterns) == OLD_PATTERNS
    for n in old_sizes:
        for pattern in old_patterns:
            stamps = _stamps(pattern, n, seed=n + len(pattern))
            for below in (0, int(stamps.min()), int(np.median(stamps)), 1 << 31):
                for n_want in (0, 1, 64, n - 1, n):
                    bad = oldest_rows_model(stamps, n_want, below, 5, fault=fault)
                    want = oldest_rows_reference(stamps, n_want, below, 5)
                    assert bad[1] == want[1] and np.array_equal(bad[0], want[0]), (fault, n, pattern, below, n_want)
    stamps = _stamps("full", 70001, seed=3)                              # test_result_is_a_function_of_the_stamps_alone
    below = int(np.quantile(stamps, 0.8)) + 1
    assert np.array_equal(oldest_rows_model(stamps, 5000, below, 77, fault=fault)[0], oldest_rows_reference(stamps, 5000, below, 77)[0])
