"""No GPU: the segment schedule of a MIPS search as a value (csrc/mips_plan.h, read through emdr2_mips_search_plan).

`_restated` is the loop search_impl ran before the plan existed, with the launch guards of s8_launch (mips_scan8.h) and mips_launch_scan8i
(mips_scan8i.hip) inlined where that loop tried the launchers in turn: the int8 persistent scan, then the fp16 one, then the lock-step
kernel.  It never calls the plan; every case of the grid compares the two segment by segment.  Product knobs: first segment 8,192 rows,
growth 8, growth 2 once a segment of the int8 threshold's length runs on the shadow image, progress counters coupled."""
import ctypes
import itertools

import pytest

N_ROWS = (1, 511, 512, 8191, 8192, 8193, 12288, 12289, 24575, 24576, 24581, 73733, 98304, 98305, 290003, 21015324, 2 ** 31 - 1025)
N_Q = (1, 128, 129, 256, 257, 512)
DIMS = (64, 96, 128, 256, 768, 1024)
MIN_ROWS = (-1, 1, 16384, 2 ** 19)
CUS = (8, 16, 104, 256, 304)


@pytest.fixture(scope="module")
def native():
    import os
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    _native.lib()
    return _native


def _s8_covers(bn, nch, row_begin, row_end, cus):
    """s8_launch's -4 answers: the query image, the K-tile pairs, the 256-row items, and no fewer items than workgroups"""
    if bn not in (256, 512) or nch & 3 or nch < 4 or row_begin & 255 or row_end <= row_begin:
        return False
    grid = max(cus & ~15, 16)
    return ((row_end + 255) // 256 - row_begin // 256) * (bn // 256) >= grid


def _restated(n_rows, nq, dim, min_rows, cus):
    """-> ([(row_begin, row_end, engine, select_after, prog_slot)], pack_q8); min_rows < 0: no shadow"""
    variant = 2 if nq <= 128 else (1 if nq <= 256 else 0)
    bn = (512, 256, 128)[variant]
    nch = dim // 32
    dense_rows = min(n_rows, 8192)
    shadow_ok = min_rows >= 0 and variant <= 1 and dim % 256 == 0 and n_rows - dense_rows >= min_rows
    segments, scan8_launches, pending = [], 0, False
    done, seg_end, mode = 0, dense_rows, 1
    while done < n_rows:
        engine, slot = None, -1
        if mode == 0 and variant <= 1:
            prog = scan8_launches if scan8_launches < 8 else -1
            if shadow_ok and seg_end - done >= min_rows:
                if not nch & 7 and _s8_covers(bn, nch // 2, done, seg_end, cus):      # mips_launch_scan8i: 64-wide int8 chunks
                    engine = "PERSISTENT_I8"
            if engine is None and _s8_covers(bn, nch, done, seg_end, cus):
                engine = "PERSISTENT_F16"
            if engine is not None:
                scan8_launches += 1
                slot = prog
        if engine is None:
            engine = "DENSE" if mode == 1 else "LOCKSTEP"
        if engine == "PERSISTENT_I8":
            pending = True
        segments.append((done, seg_end, engine, seg_end < n_rows or pending, slot))
        done = seg_end
        seg_end = min(done * (2 if shadow_ok and done * (2 - 1) >= min_rows else 8), n_rows)
        if n_rows - seg_end < seg_end // 2:
            seg_end = n_rows
        mode = 0
    return segments, shadow_ok


_GRID = list(itertools.product(N_ROWS, N_Q, DIMS, MIN_ROWS, CUS))


def test_plan_equals_the_restated_loop_on_the_whole_grid(native):
    engines, longest, unpaced, packed_unused = set(), 0, 0, 0
    for n_rows, nq, dim, min_rows, cus in _GRID:
        want, want_q8 = _restated(n_rows, nq, dim, min_rows, cus)
        got, got_q8 = native.search_plan(n_rows, nq, dim, 50, min_rows, cus)
        case = (n_rows, nq, dim, min_rows, cus)
        assert got_q8 == want_q8, case
        assert got == want, (case, got, want)
        # the segments tile [0, n_rows): no gap, no overlap, none empty
        assert got[0][0] == 0 and got[-1][1] == n_rows, case
        assert all(b < e for b, e, _, _, _ in got) and all(got[i][1] == got[i + 1][0] for i in range(len(got) - 1)), case
        engines |= {s[2] for s in got}
        longest = max(longest, len(got))
        persistent = [s for s in got if s[2].startswith("PERSISTENT")]
        assert [s[4] for s in persistent] == [i if i < 8 else -1 for i in range(len(persistent))], case
        unpaced += len(persistent) > 8
        packed_unused += got_q8 and not any(s[2] == "PERSISTENT_I8" for s in got)
    # what the grid is for (counted on the restatement when the grid was chosen)
    assert engines == set(native.SCAN_ENGINES)
    assert (len(_GRID), longest, unpaced, packed_unused) == (12240, 19, 270, 372)


def _int8(native, n_rows, nq):
    segments, q8 = native.search_plan(n_rows, nq, 256, 50, 16384, 256)
    return q8, sum(s[2] == "PERSISTENT_I8" for s in segments)


def test_the_named_cases_of_the_boundary_test(native):
    """the docstring of tests/test_mips_boundary_gpu.py, on a 256-CU device at dimension 256 with a 16,384-row threshold"""
    for nq in (129, 257, 512):
        assert _int8(native, 24575, nq) == (False, 0)               # one row short of the threshold: nothing packed
        assert _int8(native, 24581, nq) == (True, 0)                # packed, but 65 row tiles are too few for the persistent scan
        assert _int8(native, 73733, nq) == (True, 1)
    assert [_int8(native, 290003, nq) for nq in (129, 256, 257, 512)] == [(True, 2), (True, 2), (True, 3), (True, 3)]
    assert native.search_plan(73733, 512, 256, 50, 16384, 256)[0] == [
        (0, 8192, "DENSE", True, -1), (8192, 73733, "PERSISTENT_I8", True, 0)]
    assert native.search_plan(290003, 512, 256, 50, 16384, 256)[0] == [
        (0, 8192, "DENSE", True, -1), (8192, 65536, "PERSISTENT_I8", True, 0), (65536, 131072, "PERSISTENT_I8", True, 1),
        (131072, 290003, "PERSISTENT_I8", True, 2)]
    assert native.search_plan(290003, 512, 256, 50, -1, 256)[0] == [
        (0, 8192, "DENSE", True, -1), (8192, 65536, "PERSISTENT_F16", True, 0), (65536, 290003, "PERSISTENT_F16", False, 1)]
    assert native.search_plan(290003, 128, 256, 50, 16384, 256) == (
        [(0, 8192, "DENSE", True, -1), (8192, 65536, "LOCKSTEP", True, -1), (65536, 290003, "LOCKSTEP", False, -1)], False)


@pytest.mark.parametrize("min_rows", [1, 16384, 2 ** 19])
@pytest.mark.parametrize("dim", [64, 256, 768])
def test_want_shadow_is_what_the_python_formula_said(native, dim, min_rows):
    """HipIndexShard._want_shadow: pack_q8 of the plan for 512 queries, against the formula the class carried before"""
    for n_rows in N_ROWS:
        want = dim % 256 == 0 and n_rows - 8192 >= min_rows >= 1
        assert native.search_plan(n_rows, 512, dim, 1, min_rows, 256)[1] == want, (n_rows, dim, min_rows)     # (no CU count enters pack_q8)


def test_bad_arguments_are_refused_and_nothing_is_written(native):
    lib = native.lib()
    n, q8 = ctypes.c_int(-7), ctypes.c_int(-7)
    end = (ctypes.c_int64 * 32)(*[-7] * 32)
    eng, sel, slot = ((ctypes.c_int32 * 32)(*[-7] * 32) for _ in range(3))
    outs = [ctypes.byref(n), end, eng, sel, slot, ctypes.byref(q8)]

    def call(n_rows=290003, nq=512, dim=256, k=50, min_rows=16384, cus=256, slots=32, null=None):
        o = [None if i == null else p for i, p in enumerate(outs)]
        return lib.emdr2_mips_search_plan(n_rows, nq, dim, k, min_rows, cus, slots, *o)

    for null in range(6):
        assert call(null=null) == -1
    for bad in (dict(nq=0), dict(nq=513), dict(k=0), dict(k=native.MAX_TOPK + 1), dict(dim=48), dict(dim=8224), dict(n_rows=-1),
                dict(n_rows=2 ** 31 - 1024), dict(cus=-1), dict(slots=3), dict(slots=0)):
        assert call(**bad) == -1, bad
    assert n.value == q8.value == -7 and all(v == -7 for a in (end, eng, sel, slot) for v in a)
    assert call(slots=4) == 0 and n.value == 4 and q8.value == 1 and list(end[:5]) == [8192, 65536, 131072, 290003, -7]
    assert call(n_rows=0) == 0 and n.value == 0 and q8.value == 0
