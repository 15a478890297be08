"""CPU: the numpy restatement of the packed sequence layout (tests/seqpack_ref.py) against a naive loop over the sequences that follows
the words of include/emdr2_ops.h ("packed sequences") one position at a time, and the input families the GPU tests build their grids
from."""
import numpy as np
import pytest

from tests import seqpack_ref as sr


def _naive(ids, types, rows_padded_extra):
    n, S = ids.shape
    lens = []
    for row in ids:
        ln = S                                                         # an all-pad row keeps every position
        for pos in range(S - 1, -1, -1):
            if row[pos] != 0:
                ln = pos + 1
                break
        lens.append(ln)
    cu = [0]
    for ln in lens:
        cu.append(cu[-1] + ln)
    total = cu[-1]
    rows_padded = total + rows_padded_extra
    rowmap, inverse = [-1] * rows_padded, [-1] * (n * S)
    ids_p, types_p = [0] * rows_padded, [0] * rows_padded
    for i in range(n):
        for pos in range(lens[i]):
            t, d = cu[i] + pos, i * S + pos
            rowmap[t], inverse[d] = d, t
            ids_p[t] = int(ids[i, pos])
            if types is not None:
                types_p[t] = int(types[i, pos])
    return cu, total, sum(ln * ln for ln in lens), max(lens), rowmap, inverse, ids_p, (types_p if types is not None else None)


@pytest.mark.parametrize("n,S,extra", [(1, 1, 0), (1, 5, 3), (4, 3, 0), (7, 64, 255), (33, 65, 257), (40, 130, 1)])
def test_restatement_equals_the_naive_loop(n, S, extra):
    rng = np.random.default_rng(n * 100 + S)
    for variant in range(4):
        ids, where = sr.edge_grid(n, S, rng, variant)
        types = rng.integers(0, 2, size=(n, S)).astype(np.int64)
        before = ids.copy()
        cu, total, sq, mx = sr.lengths(ids)
        want = _naive(ids, types, extra)
        assert cu.dtype == np.int32 and cu.tolist() == want[0] and (total, sq, mx) == want[1:4] and isinstance(sq, int)
        rowmap, inverse, ids_p, types_p = sr.layout(ids, types, cu, total + extra)
        assert rowmap.dtype == np.int32 and inverse.dtype == np.int32 and ids_p.dtype == np.int64 and types_p.dtype == np.int64
        assert rowmap.tolist() == want[4] and inverse.tolist() == want[5] and ids_p.tolist() == want[6] and types_p.tolist() == want[7]
        assert sr.layout(ids, None, cu, total + extra)[3] is None
        assert np.array_equal(ids, before)
        ln = np.diff(cu)
        for kind, r in where.items():                                  # the special rows are what they are called
            assert ln[r] == {"all_pad": S, "last_only": S, "first_only": 1}.get(kind, ln[r])
            if kind == "interior_zeros":
                assert ids[r, 1] == 0 and ids[r, ln[r] - 1] != 0 and ln[r] >= 3
    with pytest.raises(ValueError):
        sr.layout(ids, None, cu, total - 1)


def test_every_kind_of_row_is_placed():
    rng = np.random.default_rng(0)
    assert set(sr.edge_grid(15, 63, rng)[1]) == set(sr.KINDS)
    assert set(sr.edge_grid(38000, 2, rng)[1]) == set(sr.KINDS) - {"interior_zeros"}
    assert [list(sr.edge_grid(1, 64, rng, v)[1]) for v in range(4)] == [[k] for k in sr.KINDS]


def test_sum_of_squares_is_a_python_int_past_two_to_the_31():
    ids = np.ones((40, 8192), dtype=np.int64)
    cu, total, sq, mx = sr.lengths(ids)
    assert (total, sq, mx) == (327680, 2684354560, 8192) and sq > 1 << 31


@pytest.mark.parametrize("n,S,total", [(384, 256, 74000), (384, 256, 85000), (384, 256, 98304), (384, 256, 384), (4100, 256, (1 << 20) + 1), (5, 7, 19)])
def test_lengths_with_total_is_exact_and_keeps_its_pins(n, S, total):
    rng = np.random.default_rng(total)
    pins = {1: 1, 2: S} if 384 < total < n * S else {}
    lens = sr.lengths_with_total(n, S, total, rng, pins)
    assert int(lens.sum()) == total and lens.min() >= 1 and lens.max() <= S and all(lens[r] == v for r, v in pins.items())
    ids = sr.grid_from_lengths(lens, S, rng)
    assert np.array_equal(np.diff(sr.lengths(ids)[0]), lens) and ((ids != 0).sum(1) == lens).all()
    with pytest.raises(ValueError):
        sr.lengths_with_total(n, S, n * S + 1, rng)


def test_gather_and_scatter_against_row_loops():
    rng = np.random.default_rng(3)
    inp = rng.integers(0, 1 << 16, size=(9, 8)).astype(np.uint16)
    m = np.array([3, -1, 3, 0, 8, -1, 2], dtype=np.int32)
    got = sr.gather(inp, m, 7)
    for r in range(7):
        assert np.array_equal(got[r], inp[m[r]] if m[r] >= 0 else np.zeros(8, dtype=np.uint16))
    assert np.array_equal(sr.gather(inp, m, 3), got[:3])               # a longer map: only the first rows_out entries count
    out = rng.integers(0, 1 << 16, size=(12, 8)).astype(np.uint16)
    tm = np.array([11, -1, 0, 5, -1, 4, 7, -1, 1], dtype=np.int32)
    new = sr.scatter(inp, tm, out)
    want = out.copy()
    for r in range(9):
        if tm[r] >= 0:
            want[tm[r]] = inp[r]
    assert np.array_equal(new, want) and new is not out and not np.array_equal(new, out)
    with pytest.raises(ValueError):
        sr.scatter(inp, np.array([1, 1, -1, 2, 3, 4, 5, 6, 7], dtype=np.int32), out)
