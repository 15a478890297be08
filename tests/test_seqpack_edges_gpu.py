"""GPU: the packed ("varlen") sequence layout at the sizes a training step runs it with.

B.  The four entry points of csrc/seqpack.hip through the C ABI, bit for bit against the numpy restatement of their contract
    (tests/seqpack_ref.py): every output pre-filled with a sentinel and embedded between guard words that must stay intact (the pattern
    of tests/test_answer_hits_gpu.py), every input compared unchanged after the call.  Sizes are those at which a path of the kernels
    changes: the 16-sequence workgroups of the length kernel and its 64-token ballot chunks, the one-then-two sequences per thread of
    the scan, the LDS opt-in above 16,000 sequences and the limit of 38,000, a sum of squares past 2^31; tails of 0, 1, 255, 256, 257
    and 16,383 rows behind the packed ids; rows of 1, 127, 128, 129 and 288 sixteen-byte lanes, one and two rows per workgroup.
C.  The row-count policy of kernels.PackedSeqs: 256 / 8,192 / 16,384-row granules by token count, and the sticky capacities of a
    training loop (PACKING.sticky), on grids whose totals are exact.  Properties and the row counts of today's rule are asserted; the
    rule itself is not restated.
D.  Packed equals dense with a tail of DOZENS of 256-row tiles.  A step above 65,536 real tokens runs with thousands of tail rows
    (81,920 rows for 74,000 tokens; 86,016 when a larger batch of the same capacity key came first).  What the stacks rely on: tail
    rows of every activation gradient are exactly zero and tail rows of every activation are finite, so the reductions over all `rows`
    (weight and bias gradients, LayerNorm, embedding) add nothing.  Before each packed run the memory torch.empty hands out next is
    filled with NaN, so a tail row nothing wrote shows up.  Arms: 1 dense, 2 packed with sticky off, 3 packed with sticky on after a
    larger grid primed the capacity.  Bounds are those of tests/test_seqpack_gpu.py (test_emdr2_step_packed_equals_dense,
    test_bert_tower_packed_equals_dense_and_oracle, test_packed_self_attention_equals_dense), unchanged.

Measured on an MI355X (the tests print these figures).  EMDR2 step, reader / one-context stack n = 384, S = 256 with 74,000 / 74,200 real
tokens, against the dense arm:

    arm                    rows      tail rows (reader / one-context)     loss    tlp     logits   worst parameter gradient
    2  sticky off          81,920    7,920 (30 whole tiles) / 7,720       0       0       0        1.8e-3  decoder layer 0 self-attention QKV weight
    3  primed capacity     86,016    12,016 (46 whole tiles) / 11,816     0       0       0        1.8e-3  the same parameter
    bound                                                                 2e-3    1e-5    1e-2     3e-2

Arm 2, today's accepted comparison at a larger token count, sits at 6 % of the gradient bound and at zero on the others: nowhere near half
of a bound.  Arm 3 against arm 2: encoder output, tlp and logits are bit-equal; 70 to 74 of the 129 parameter gradients are bit-equal
(the count moves from run to run), the worst of the others differs by 2e-6 of its scale: reductions over the rows, summed in another
order.  BERT tower (74,000 tokens): output equal to the dense arm's in both packed arms, worst gradient about 2e-6 (bound 2e-3), arm
3's output bit-equal to arm 2's.

Sensitivity, checked once on a scratch copy: without `L.ids_q.zero_tail(dqsrc)` in AttentionCoreFn.backward the step test fails in both
arms (the reader's embedding.word_embeddings.weight and further parameters named, ratios of 30 to 1e9 against the bound of 3e-2), as do the tower
test and the attention test (a non-zero tail of the QKV gradient).
"""
import contextlib

import numpy as np
import pytest
import torch

from tests import seqpack_ref as sr

pytestmark = pytest.mark.gpu
GUARD, SENTINEL, SENTINEL16 = 512, -77, 0x5A5A
CFG = dict(layers=2, hidden=128, heads=2, ffn=256, max_pos=256)


def _native():
    from emdr2_amd import _native as nat
    return nat


def _guarded(shape, dtype, fill):
    """(whole buffer, the view handed to the kernel): GUARD words of `fill` on either side."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(shape)


def _guards_intact(whole, n, fill):
    return bool((torch.cat([whole[:GUARD], whole[GUARD + n:]]) == fill).all())


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _host16(t):
    return t.cpu().numpy().view(np.uint16)


# ---- B. emdr2_seq_lengths ---------------------------------------------------------------------------------------------------------------
LENGTH_CASES = [(n, S) for n in (1, 15, 16, 17, 1023, 1024, 1025, 2049) for S in (1, 63, 64, 65, 130)] + [(16000, 2), (16001, 2), (38000, 2)]


def _case_grids(n, S):
    """The grids of a case: one, or one per kind of special row when the grid has a single row."""
    rng = np.random.default_rng(n * 1000 + S)
    grids = [sr.edge_grid(n, S, rng, v) for v in range(4 if n < 4 else 1)]
    kinds = set().union(*(set(w) for _, w in grids))
    assert kinds == set(sr.KINDS) - ({"interior_zeros"} if S < 3 else set())       # rows of every kind appear in every case
    return [g for g, _ in grids]


def abi_lengths(ids, d_ids=None, want_rc=0):
    """emdr2_seq_lengths -> (cu int32 [n + 1], [total, sum len^2, max len]); guards and the untouched input asserted."""
    nat = _native()
    n, S = ids.shape
    d_ids = _dev(ids) if d_ids is None else d_ids
    w_cu, cu = _guarded((n + 1,), torch.int32, SENTINEL)
    w_tot, tot = _guarded((3,), torch.int64, SENTINEL)
    rc = nat.lib().emdr2_seq_lengths(d_ids.data_ptr(), n, S, cu.data_ptr(), tot.data_ptr(), nat.stream_ptr())
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    assert _guards_intact(w_cu, n + 1, SENTINEL) and _guards_intact(w_tot, 3, SENTINEL), "a guard word was written"
    assert np.array_equal(d_ids.cpu().numpy(), ids)
    return cu.cpu().numpy(), [int(v) for v in tot.tolist()]


def check_lengths(ids):
    cu, totals = abi_lengths(ids)
    want_cu, total, sq, mx = sr.lengths(ids)
    assert cu.dtype == want_cu.dtype and np.array_equal(cu, want_cu), np.argwhere(cu != want_cu)[:5].tolist()
    assert totals == [total, sq, mx], (totals, [total, sq, mx])
    return want_cu, total


@pytest.mark.parametrize("n,S", LENGTH_CASES)
def test_seq_lengths(n, S):
    for ids in _case_grids(n, S):
        check_lengths(ids)


def test_seq_lengths_sum_of_squares_past_two_to_the_31():
    """n = 40 full rows of S = 8,192: 128 ballot chunks per row, sum len^2 = 2,684,354,560 > 2^31 -- totals[1] is 64-bit end to end."""
    ids = np.random.default_rng(1).integers(1, 1000, size=(40, 8192)).astype(np.int64)
    cu, totals = abi_lengths(ids)
    assert totals == [40 * 8192, 2684354560, 8192] and totals[1] > 1 << 31
    assert np.array_equal(cu, np.arange(41, dtype=np.int32) * 8192)
    ids[7] = 0                                                         # an all-pad row of 8,192 keeps its positions: the same answer
    ids[9, :8191] = 0                                                  # only the last position of the last chunk
    assert abi_lengths(ids)[1] == [40 * 8192, 2684354560, 8192]


def test_seq_lengths_refuses_more_than_38000_sequences_before_any_launch():
    ids = np.ones((38001, 2), dtype=np.int64)
    cu, totals = abi_lengths(ids, want_rc=-4)
    assert (cu == SENTINEL).all() and totals == [SENTINEL] * 3         # nothing ran


def test_seq_lengths_argument_errors():
    nat = _native()
    lib, sp = nat.lib(), nat.stream_ptr()
    ids = _dev(np.ones((4, 8), dtype=np.int64))
    w_cu, cu = _guarded((5,), torch.int32, SENTINEL)
    w_tot, tot = _guarded((3,), torch.int64, SENTINEL)
    a = (ids.data_ptr(), 4, 8, cu.data_ptr(), tot.data_ptr())
    for i, bad in ((0, None), (3, None), (4, None), (1, 0), (1, -1), (2, 0), (2, -5)):
        args = list(a)
        args[i] = bad
        assert lib.emdr2_seq_lengths(*args, sp) == -1, (i, bad)
    torch.cuda.synchronize()
    assert bool((w_cu == SENTINEL).all()) and bool((w_tot == SENTINEL).all())


# ---- B. emdr2_seq_pack_ids ----------------------------------------------------------------------------------------------------------------
TAILS = (0, 1, 255, 256, 257, 16383)          # no tail workgroup; one partial; one less than full; full; full + 1; 64 groups (the 16,384-row granule's largest)


def abi_pack_ids(d_ids, d_types, d_cu, n, S, total, rows_padded):
    """emdr2_seq_pack_ids -> rowmap, inverse, ids_packed, types_packed (numpy; None without types); guards asserted."""
    nat = _native()
    bufs = [_guarded((rows_padded,), torch.int32, SENTINEL), _guarded((n * S,), torch.int32, SENTINEL), _guarded((rows_padded,), torch.int64, SENTINEL),
            _guarded((rows_padded,), torch.int64, SENTINEL) if d_types is not None else (None, None)]
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = nat.lib().emdr2_seq_pack_ids(d_ids.data_ptr(), ptr(d_types), d_cu.data_ptr(), n, S, total, rows_padded, ptr(bufs[0][1]), ptr(bufs[1][1]),
                                      ptr(bufs[2][1]), ptr(bufs[3][1]), nat.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    for (whole, view), size in zip(bufs, (rows_padded, n * S, rows_padded, rows_padded)):
        assert whole is None or _guards_intact(whole, size, SENTINEL), "a word outside the buffer was written"
    return [None if view is None else view.cpu().numpy() for _, view in bufs]


def check_pack_ids(ids):
    n, S = ids.shape
    rng = np.random.default_rng(n + S)
    types = rng.integers(0, 3, size=(n, S)).astype(np.int64)
    cu, total, _, _ = sr.lengths(ids)
    d_ids, d_types, d_cu = _dev(ids), _dev(types), _dev(cu)
    dropped = (np.arange(S)[None, :] >= np.diff(cu)[:, None]).reshape(-1)
    for tail in TAILS:
        for ty in (types, None):
            got = abi_pack_ids(d_ids, d_types if ty is not None else None, d_cu, n, S, total, total + tail)
            want = sr.layout(ids, ty, cu, total + tail)
            for name, g, w in zip(("rowmap", "inverse", "ids_packed", "types_packed"), got, want):
                assert (g is None and w is None) or (g.dtype == w.dtype and np.array_equal(g, w)), (tail, name, np.argwhere(g != w)[:5].tolist())
            rowmap, inverse, ids_p, types_p = got
            assert (rowmap[total:] == -1).all() and (ids_p[total:] == 0).all() and (types_p is None or (types_p[total:] == 0).all())
            assert (rowmap[:total] >= 0).all() and np.array_equal(inverse == -1, dropped)
    assert np.array_equal(d_ids.cpu().numpy(), ids) and np.array_equal(d_types.cpu().numpy(), types) and np.array_equal(d_cu.cpu().numpy(), cu)


@pytest.mark.parametrize("n,S", LENGTH_CASES)
def test_seq_pack_ids(n, S):
    for ids in _case_grids(n, S):
        check_pack_ids(ids)


def test_seq_pack_ids_rows_of_8192():
    ids = np.random.default_rng(2).integers(1, 1000, size=(40, 8192)).astype(np.int64)
    ids[7] = 0
    ids[9, :8191] = 0
    ids[11, 100:] = 0
    check_pack_ids(ids)


def test_seq_pack_ids_argument_errors():
    nat = _native()
    lib, sp = nat.lib(), nat.stream_ptr()
    ids = np.ones((4, 8), dtype=np.int64)
    cu = sr.lengths(ids)[0]
    d_ids, d_cu = _dev(ids), _dev(cu)
    w_map, rowmap = _guarded((64,), torch.int32, SENTINEL)
    w_inv, inverse = _guarded((32,), torch.int32, SENTINEL)
    w_ids, ids_p = _guarded((64,), torch.int64, SENTINEL)
    w_ty, ty_p = _guarded((64,), torch.int64, SENTINEL)
    call = lambda types, total, rows, tp: lib.emdr2_seq_pack_ids(d_ids.data_ptr(), types, d_cu.data_ptr(), 4, 8, total, rows, rowmap.data_ptr(),
                                                                 inverse.data_ptr(), ids_p.data_ptr(), tp, sp)
    assert call(None, 32, 31, None) == -1                                         # rows_padded < total
    assert call(d_ids.data_ptr(), 32, 32, None) == -1                             # types without types_packed
    assert call(None, 0, 32, None) == -1
    torch.cuda.synchronize()
    for w in (w_map, w_inv, w_ids, w_ty):
        assert bool((w == SENTINEL).all())
    assert call(d_ids.data_ptr(), 32, 32, ty_p.data_ptr()) == 0 and call(None, 32, 32, ty_p.data_ptr()) == 0   # (types_packed without types: not written)
    torch.cuda.synchronize()
    assert np.array_equal(rowmap.cpu().numpy()[:32], np.arange(32)) and bool((rowmap[32:] == SENTINEL).all())


# ---- B. emdr2_gather_rows / emdr2_scatter_rows ---------------------------------------------------------------------------------------------
ROW_WIDTHS = (8, 1016, 1024, 1032, 2304)      # 1, 127, 128, 129 sixteen-byte lanes; 288 = two laps of the 128 lanes and a partial third (QKV at hidden 768)
ROW_COUNTS = (1, 2, 3, 513)                   # a workgroup takes two rows
SPECIAL16 = np.array([0x7FC0, 0x7F81, 0xFFFF, 0xFFC1, 0x7F80, 0xFF80, 0x8000, 0x0000, 0x0001, 0x8001], dtype=np.uint16)   # NaN payloads, +-inf, -0.0, +0.0, denormals


def _rows16(rng, rows, H):
    a = rng.integers(0, 1 << 16, size=(rows, H)).astype(np.uint16)
    flat = a.reshape(-1)
    k = min(flat.size, 8 * len(SPECIAL16))
    flat[rng.choice(flat.size, size=k, replace=False)] = np.resize(SPECIAL16, k)
    flat[:8] = SPECIAL16[:8]
    return a


def _maps(rng, rows, pick):
    """Maps of `rows` entries: pick(rows) draws the non-negative entries.  Few rows: the negative entry at every place and nowhere;
    many: a tenth negative, the last row (alone in its workgroup when rows is odd) once negative and once not."""
    if rows <= 3:
        out = []
        for v in range(rows + 1):
            m = pick(rows)
            if v < rows:
                m[v] = -1 - 5 * v                                       # any negative value, not only -1
            out.append(m)
        return out
    out = []
    for last_negative in (True, False):
        m = pick(rows)
        last = m[rows - 1]
        m[rng.random(rows) < 0.1] = -1
        m[rows - 1] = -1 if last_negative else last
        out.append(m)
    return out


def _move_rows(fn_name, d_in, d_map, rows, H, out0):
    """One emdr2_gather_rows / emdr2_scatter_rows call into a guarded copy of out0 (uint16 [rows_out, H]) -> the buffer afterwards."""
    nat = _native()
    w_out, out = _guarded(out0.shape, torch.int16, SENTINEL16)
    out.copy_(_dev(out0))
    rc = getattr(nat.lib(), fn_name)(d_in.data_ptr(), d_map.data_ptr(), out.data_ptr(), rows, H, nat.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert _guards_intact(w_out, out0.size, SENTINEL16), "a word outside the buffer was written"
    return _host16(out)


@pytest.mark.parametrize("rows", ROW_COUNTS)
@pytest.mark.parametrize("H", ROW_WIDTHS)
def test_gather_rows(H, rows):
    rng = np.random.default_rng(H * 7 + rows)
    rows_in = 37
    inp = _rows16(rng, rows_in, H)
    d_in = _dev(inp)
    repeated = lambda r: np.full(r, int(rng.integers(0, rows_in)), dtype=np.int32) if r <= 3 else rng.integers(0, rows_in, size=r).astype(np.int32)
    for m in _maps(rng, rows, repeated):
        if int((m >= 0).sum()) >= 2:
            assert len(np.unique(m[m >= 0])) < int((m >= 0).sum())      # sources repeat
        d_map = _dev(m)
        got = _move_rows("emdr2_gather_rows", d_in, d_map, rows, H, np.full((rows, H), SENTINEL16, dtype=np.uint16))
        want = sr.gather(inp, m, rows)
        assert np.array_equal(got, want), (m[:8].tolist(), np.argwhere(got != want)[:5].tolist())
        assert not got[m < 0].any()                                     # +0, every bit
        assert np.array_equal(_host16(d_in), inp) and np.array_equal(d_map.cpu().numpy(), m)


@pytest.mark.parametrize("rows", ROW_COUNTS)
@pytest.mark.parametrize("H", ROW_WIDTHS)
def test_scatter_rows(H, rows):
    rng = np.random.default_rng(H * 11 + rows)
    rows_out = rows + 5
    inp = _rows16(rng, rows, H)
    d_in = _dev(inp)
    distinct = lambda r: rng.permutation(rows_out)[:r].astype(np.int32)
    for m in _maps(rng, rows, distinct):
        d_map = _dev(m)
        out0 = np.full((rows_out, H), SENTINEL16, dtype=np.uint16)
        got = _move_rows("emdr2_scatter_rows", d_in, d_map, rows, H, out0)
        want = sr.scatter(inp, m, out0)
        assert np.array_equal(got, want), (m[:8].tolist(), np.argwhere(got != want)[:5].tolist())
        unnamed = np.setdiff1d(np.arange(rows_out), m[m >= 0])
        assert len(unnamed) >= 5 and (got[unnamed] == SENTINEL16).all()  # rows no entry names keep the sentinel
        assert np.array_equal(_host16(d_in), inp) and np.array_equal(d_map.cpu().numpy(), m)


@pytest.mark.parametrize("fn_name", ["emdr2_gather_rows", "emdr2_scatter_rows"])
def test_row_moves_argument_errors(fn_name):
    nat = _native()
    fn, sp = getattr(nat.lib(), fn_name), nat.stream_ptr()
    inp = torch.full((4 * 16 + 8,), 3, dtype=torch.int16, device="cuda")
    w_out, out = _guarded((4 * 16 + 8,), torch.int16, SENTINEL16)
    m = _dev(np.arange(4, dtype=np.int32))
    assert inp.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    assert fn(inp.data_ptr(), m.data_ptr(), out.data_ptr(), 4, 12, sp) == -1                 # H % 8 != 0
    assert fn(inp.data_ptr(), m.data_ptr(), out.data_ptr(), 4, 4, sp) == -1                  # H < 8
    assert fn(inp.data_ptr(), m.data_ptr(), out.data_ptr(), 4, 0, sp) == -1                  # H < 8 and a multiple of 8
    assert fn(inp.data_ptr(), m.data_ptr(), out.data_ptr(), 4, -8, sp) == -1
    assert fn(inp[1:].data_ptr(), m.data_ptr(), out.data_ptr(), 4, 16, sp) == -1             # `in` 2 bytes off 16-byte alignment
    assert fn(inp[4:].data_ptr(), m.data_ptr(), out.data_ptr(), 4, 16, sp) == -1             # 8 bytes off
    assert fn(inp.data_ptr(), m.data_ptr(), out[1:].data_ptr(), 4, 16, sp) == -1             # `out` off
    assert fn(inp.data_ptr(), m.data_ptr(), out[4:].data_ptr(), 4, 16, sp) == -1
    assert fn(None, m.data_ptr(), out.data_ptr(), 4, 16, sp) == -1 and fn(inp.data_ptr(), None, out.data_ptr(), 4, 16, sp) == -1
    assert fn(inp.data_ptr(), m.data_ptr(), None, 4, 16, sp) == -1 and fn(inp.data_ptr(), m.data_ptr(), out.data_ptr(), 0, 16, sp) == -1
    torch.cuda.synchronize()
    assert bool((w_out == SENTINEL16).all())
    assert fn(inp[8:].data_ptr(), m.data_ptr(), out[8:].data_ptr(), 4, 16, sp) == 0          # 16 bytes on: aligned again
    torch.cuda.synchronize()
    assert bool((out[8:] == 3).all()) and bool((out[:8] == SENTINEL16).all()) and _guards_intact(w_out, 4 * 16 + 8, SENTINEL16)


# ---- C. the row-count policy of PackedSeqs -------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _packing_state():
    """PACKING with a clean slate (sticky off, no capacities) inside, what it held before afterwards."""
    from emdr2_amd.model import kernels as K
    P = K.PACKING
    saved = (P.sticky, P.enabled, P.capacity, P.growths, P.history)
    P.sticky, P.enabled, P.capacity, P.growths, P.history = False, True, {}, 0, []
    try:
        yield P
    finally:
        P.sticky, P.enabled, P.capacity, P.growths, P.history = saved


@pytest.fixture
def packing():
    with _packing_state() as P:
        yield P


def _grid(n, S, total, seed, pins=None, vocab=600):
    """(ids int64 [n, S] on the host, lengths) with exactly `total` real tokens."""
    rng = np.random.default_rng(seed)
    lens = sr.lengths_with_total(n, S, total, rng, pins)
    return sr.grid_from_lengths(lens, S, rng, vocab), lens


def _seqs(ids, types=None):
    from emdr2_amd.model import kernels as K
    return K.PackedSeqs(_dev(ids), None if types is None else _dev(types))


def check_layout(seqs, ids, types=None):
    """The PackedSeqs equals the restatement over its WHOLE buffers, tail included."""
    cu, total, sq, mx = sr.lengths(ids)
    assert (seqs.total, seqs.pairs, seqs.max_len) == (total, sq, mx) and seqs.total <= seqs.rows
    rowmap, inverse, ids_p, types_p = sr.layout(ids, types, cu, seqs.rows)
    assert np.array_equal(seqs.cu.cpu().numpy(), cu)
    assert seqs.rowmap.shape == (seqs.rows,) and np.array_equal(seqs.rowmap.cpu().numpy(), rowmap)
    assert np.array_equal(seqs.inverse.cpu().numpy(), inverse)
    assert seqs.ids.shape == (seqs.rows,) and np.array_equal(seqs.ids.cpu().numpy(), ids_p)
    assert (seqs.types is None) == (types is None) and (types is None or np.array_equal(seqs.types.cpu().numpy(), types_p))


@pytest.mark.parametrize("n,S,total,granule,rows", [
    (384, 256, 65000, 256, 65024), (384, 256, 65535, 256, 65536),                           # just below 65,536 tokens: whole GEMM tiles
    (384, 256, 65536, 8192, 65536), (384, 256, 65537, 8192, 73728), (384, 256, 74000, 8192, 81920),
    (4100, 256, (1 << 20) - 8197, 8192, (1 << 20) - 8192),                                  # 127 x 8,192: no multiple of 16,384
    (4100, 256, 1 << 20, 16384, 1 << 20), (4100, 256, (1 << 20) + 1, 16384, (1 << 20) + 16384)])
def test_row_granule_by_token_count(packing, n, S, total, granule, rows):
    ids, _ = _grid(n, S, total, total)
    types = (ids % 2).astype(np.int64) if n < 1000 else None
    seqs = _seqs(ids, types)
    assert seqs.total == total and seqs.rows % granule == 0 and 0 <= seqs.rows - seqs.total < granule and seqs.rows == rows
    assert packing.history[-1] == (n, S, rows) and packing.capacity == {} and packing.growths == 0
    check_layout(seqs, ids, types)


def test_sticky_capacity_policy(packing):
    """n = 384, S = 256: every total in [73,728, 86,016) has the key (384, 256, octile 6)."""
    n, S = 384, 256
    packing.sticky = True
    seen, cap = [], 0
    for step, (total, want_rows) in enumerate([(76800, 77824), (74000, 77824), (80000, 80896), (74000, 80896)]):
        ids, _ = _grid(n, S, total, step)
        before = packing.growths
        seqs = _seqs(ids)
        grew = packing.growths - before
        need = -(-total // 256) * 256
        assert seqs.total == total and seqs.rows >= total and seqs.rows % 256 == 0
        assert grew == (1 if need > cap else 0), (total, cap, grew)               # a growth exactly when the total, in whole tiles, exceeds the capacity
        if grew:
            assert seqs.rows - total <= 0.01 * total + 1024                       # ... and it leaves at most 1 % + 1,024 rows over the total
        else:
            assert seqs.rows == cap                                               # every total that fits runs with the same rows
        assert seqs.rows >= cap                                                   # never shrinks
        cap = seqs.rows
        assert seqs.rows == want_rows and packing.history[-1] == (n, S, want_rows)
        check_layout(seqs, ids)
        seen.append(seqs)
    assert packing.growths == 2 and len(packing.capacity) == 1 and list(packing.capacity.values()) == [80896]
    (key,) = packing.capacity
    # another octile, another n: capacities of their own, this one untouched
    other, _ = _grid(n, S, 90000, 11)
    s_other = _seqs(other)
    assert s_other.rows >= 90000 and s_other.rows % 256 == 0 and s_other.rows - 90000 <= 900 + 1024
    assert packing.growths == 3 and len(packing.capacity) == 2 and packing.capacity[key] == 80896
    fewer, _ = _grid(300, S, 70000, 12)
    s_fewer = _seqs(fewer)
    assert s_fewer.rows >= 70000 and s_fewer.rows % 256 == 0 and s_fewer.rows < 80896
    assert packing.growths == 4 and len(packing.capacity) == 3 and packing.capacity[key] == 80896
    shorter, _ = _grid(768, 128, 74000, 13)
    assert _seqs(shorter).rows < 80896 and packing.growths == 5 and packing.capacity[key] == 80896
    # below 65,536 tokens `sticky` changes nothing: whole tiles, no capacity, no growth
    small, _ = _grid(n, S, 60000, 14)
    s_small = _seqs(small)
    assert s_small.rows == 60160 and packing.growths == 5 and len(packing.capacity) == 4
    check_layout(s_small, small)
    # and the key's capacity still serves it
    again, _ = _grid(n, S, 80896, 15)
    s_again = _seqs(again)
    assert s_again.rows == 80896 == s_again.total and packing.growths == 5
    check_layout(s_again, again)
    # grouped(48): the FiD decoder's view of a sticky layout
    s = seen[-1]
    g = s.grouped(48)
    assert g.n == 8 and g.rows == s.rows == 80896 and g.total == s.total and g.max_len == 48 * s.max_len and g.group == 48
    assert np.array_equal(g.cu.cpu().numpy(), s.cu.cpu().numpy()[::48]) and g.rowmap is s.rowmap


# ---- D. packed equals dense with a tail of dozens of tiles ---------------------------------------------------------------------------------
N, S_READER, TOTAL, TOTAL_ONE, TOTAL_PRIME = 384, 256, 74000, 74200, 85000
ROWS_OFF, ROWS_PRIMED = 81920, 86016          # arm 2: the 8,192-row granule; arm 3: the capacity a grid of 85,000 tokens left behind
PINS = {1: 1, 2: S_READER}                    # one sequence of a single token, one of all 256
POISON_WORDS = 512 << 20                      # 2 GiB of fp32 NaN: the step's largest activation (86,016 x 384 bf16, the QKV projection) is 66 MB and
#                                               everything a step of this model keeps alive at once is under 1 GiB


def _cfg():
    from emdr2_amd.model.transformer import Config
    return Config(num_layers=CFG["layers"], hidden_size=CFG["hidden"], num_attention_heads=CFG["heads"], ffn_hidden_size=CFG["ffn"],
                  max_position_embeddings=CFG["max_pos"], init_method_std=0.05)


def _rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-6))


def _poison():
    """What torch.empty hands out next is NaN: the allocator's cache holds one block, all NaN, and large allocations are cut from it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    junk = torch.full((POISON_WORDS,), float("nan"), device="cuda")
    del junk


def _grads(m):
    out = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    for p in m.parameters():
        p.grad = None
    return out


def _prime(P):
    """sticky on, and the capacity of (384, 256, octile 6) left behind by a LARGER grid: 86,016 rows."""
    P.sticky = True
    big, _ = _grid(N, S_READER, TOTAL_PRIME, 21)
    assert _seqs(big).rows == ROWS_PRIMED and P.growths == 1
    P.history = []


def _arms(P, run):
    """run() under the three arms -> {1: dense, 2: packed, sticky off, 3: packed with the primed capacity}; each with its PACKING.history."""
    res = {}
    P.enabled = False
    res[1] = run() + (list(P.history),)
    assert res[1][-1] == []                                                       # the dense arm built no packed layout
    P.enabled, P.history = True, []
    _poison()
    res[2] = run() + (list(P.history),)
    _prime(P)
    _poison()
    res[3] = run() + (list(P.history),)
    assert P.growths == 1                                                         # the runs fitted the primed capacity
    return res


def _all_finite(grads):
    return [k for k, g in grads.items() if not bool(torch.isfinite(g.float()).all())]


@pytest.fixture(scope="module")
def step_arms():
    """EMDR2Model.forward_assembled + emdr2_loss + backward, B = 8 questions at top-k 48: reader and one-context stack n = 384, S = 256 with
    74,000 / 74,200 real tokens (one capacity key), context tower 384 x 32 (below 65,536 tokens) -- once per arm, same weights, same batch."""
    from emdr2_amd.model import kernels as K
    from emdr2_amd.model.emdr2_model import EMDR2Model, emdr2_loss
    rng = np.random.default_rng(7)
    B, Kk, S_ret, S, L, V = 8, 48, 32, S_READER, 32, 640
    assert B * Kk == N
    torch.manual_seed(0)
    m = EMDR2Model(None, _cfg(), V, 512, Kk, S, S_ret, cls_id=2, sep_id=3)
    m.train()
    ragged = lambda n, s, lo, vocab: sr.grid_from_lengths(rng.integers(lo, s + 1, size=n), s, rng, vocab)
    qb = _dev(ragged(B, S_ret, 3, 512))
    ctx_np = ragged(N, S_ret, 3, 512)
    ctx = _dev(ctx_np).reshape(B, Kk, S_ret)
    typ = torch.zeros_like(ctx)
    qext_np, lens = _grid(N, S, TOTAL, 31, PINS)
    qone_np, _ = _grid(N, S, TOTAL_ONE, 32, PINS)
    qext, qone = _dev(qext_np), _dev(qone_np)
    dec = _dev(ragged(B, L, 2, 600))
    labels = torch.roll(dec, -1, 1)
    labels[:, -1] = 0
    loss_mask = (labels != 0).float()
    reader = m.language_model.language_model
    ctx_rows = -(-int((ctx_np != 0).sum()) // 256) * 256                          # (no interior zeros: real tokens = kept rows)
    assert int((ctx_np != 0).sum()) < 65536 and int(lens.sum()) == TOTAL and int(8.0 * TOTAL / (N * S)) == int(8.0 * TOTAL_ONE / (N * S)) == 6

    def run():
        seen = []
        inner = reader.encode_packed

        def spy(enc_ids, tokentype_ids=None):
            enc, seqs = inner(enc_ids, tokentype_ids)
            seen.append((enc.detach(), seqs))
            return enc, seqs
        reader.encode_packed = spy                                                # the reader's encoder output (training mode does not return it)
        try:
            q_logits = m.retriever_embedder(qb, None, torch.zeros_like(qb), "query")
            lm, tlp, one = m.forward_assembled(q_logits, ctx, typ, qext, qone, dec)
            loss, _ = emdr2_loss(lm, tlp, one, labels, loss_mask, eos_id=601)
            loss.backward()
        finally:
            del reader.encode_packed
        enc = None
        if seen:
            assert len(seen) == 2 and seen[0][1].total == TOTAL and seen[1][1].total == TOTAL_ONE
            with torch.no_grad():
                enc = (K.unpack_rows(seen[0][0], seen[0][1]), seen[0][1].rows, seen[1][1].rows, seen[0][1].cu.clone())
        return [loss.detach(), lm.detach(), tlp.detach(), _grads(m), enc]

    with _packing_state() as P:
        res = _arms(P, lambda: tuple(run()))
    kept = torch.from_numpy(np.arange(S)[None, :] < lens[:, None]).cuda()
    return dict(res=res, dec=dec, kept=kept, ctx_rows=ctx_rows, S_ret=S_ret)


@pytest.mark.parametrize("arm,rows", [(2, ROWS_OFF), (3, ROWS_PRIMED)])
def test_step_row_counts_and_finiteness(step_arms, arm, rows):
    loss, lm, tlp, grads, enc, history = step_arms["res"][arm]
    # the rows the stacks really got: reader and one-context pass, the context tower (whole tiles: under 65,536 tokens) and the query tower
    assert history.count((N, S_READER, rows)) == 2 and (N, step_arms["S_ret"], step_arms["ctx_rows"]) in history, history
    assert (8, step_arms["S_ret"], 256) in history and len(history) == 4
    assert enc[1] == enc[2] == rows
    print("arm %d: rows %d, tails %d (reader, %d whole tiles) and %d (one-context)" % (arm, rows, rows - TOTAL, (rows - TOTAL) // 256, rows - TOTAL_ONE))
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(lm.float()).all()) and bool(torch.isfinite(tlp).all())
    assert _all_finite(grads) == []


@pytest.mark.parametrize("arm", [2, 3])
def test_step_packed_equals_dense_with_a_large_tail(step_arms, arm):
    """The quantities and bounds of test_seqpack_gpu.py::test_emdr2_step_packed_equals_dense, per parameter."""
    loss_d, lm_d, tlp_d, g_d, _, _ = step_arms["res"][1]
    loss_p, lm_p, tlp_p, g_p, _, _ = step_arms["res"][arm]
    dreal = step_arms["dec"] != 0
    assert float(loss_d) > 0 and float(lm_d[dreal].float().std()) > 1e-3 and float(tlp_d.std()) > 0          # (a comparison of live values)
    e_loss = abs(float(loss_p) - float(loss_d)) / abs(float(loss_d))
    e_tlp, e_lm = _rel(tlp_p, tlp_d), _rel(lm_p[dreal], lm_d[dreal])
    assert set(g_p) == set(g_d)
    gmax = max(float(g.abs().max()) for g in g_d.values())
    ratios = {k: float((g_p[k] - g_d[k]).abs().max()) / max(float(g_d[k].abs().max()), 1e-2 * gmax) for k in g_d}
    worst = max(ratios, key=lambda k: ratios[k] if ratios[k] == ratios[k] else float("inf"))
    print("arm %d against dense: loss %.3g (2e-3)  tlp %.3g (1e-5)  logits %.3g (1e-2)  worst gradient %.3g at %s (3e-2)"
          % (arm, e_loss, e_tlp, e_lm, ratios[worst], worst))
    assert e_loss < 2e-3, (float(loss_p), float(loss_d))
    assert e_tlp < 1e-5, e_tlp
    assert e_lm < 1e-2, e_lm
    bad = {k: r for k, r in ratios.items() if not r < 3e-2}
    assert not bad, bad


def test_step_primed_capacity_equals_the_free_running_rows(step_arms):
    """Arm 3 against arm 2: the same cu, the same kernels, only `rows` differs."""
    _, lm2, tlp2, g2, enc2, _ = step_arms["res"][2]
    _, lm3, tlp3, g3, enc3, _ = step_arms["res"][3]
    kept = step_arms["kept"]
    assert torch.equal(enc2[3], enc3[3])
    e_enc, e_tlp, e_lm = _rel(enc3[0][kept], enc2[0][kept]), _rel(tlp3, tlp2), _rel(lm3, lm2)
    gmax = max(float(g.abs().max()) for g in g2.values())
    e_g = max(float((g3[k] - g2[k]).abs().max()) / max(float(g2[k].abs().max()), 1e-2 * gmax) for k in g2)
    print("arm 3 against arm 2: encoder %.3g, tlp %.3g, logits %.3g (1e-5 each); bit-equal: encoder %s, tlp %s, logits %s; worst gradient %.3g, "
          "bit-equal gradients %d of %d" % (e_enc, e_tlp, e_lm, torch.equal(enc3[0], enc2[0]), torch.equal(tlp3, tlp2), torch.equal(lm3, lm2), e_g,
                                            sum(torch.equal(g3[k], g2[k]) for k in g2), len(g2)))
    assert e_enc < 1e-5 and e_tlp < 1e-5 and e_lm < 1e-5, (e_enc, e_tlp, e_lm)
    for enc in (enc2[0], enc3[0]):                                                # dropped positions of the unpacked encoder output: exactly 0
        assert int(kept.sum()) == TOTAL and float(enc[~kept].abs().max()) == 0.0


def test_bert_tower_packed_equals_dense_with_a_large_tail():
    """One level down: PretrainedBertModel over n = 384, S = 256 with 74,000 real tokens; the bounds of
    test_seqpack_gpu.py::test_bert_tower_packed_equals_dense_and_oracle."""
    from emdr2_amd.model.transformer import PretrainedBertModel
    torch.manual_seed(0)
    m = PretrainedBertModel(_cfg(), 512)
    ids_np, _ = _grid(N, S_READER, TOTAL, 41, PINS, vocab=512)
    ids = _dev(ids_np)
    types = _dev((np.arange(S_READER)[None, :] >= 20).astype(np.int64) * (ids_np != 0))
    w = torch.randn((N, CFG["hidden"]), generator=torch.Generator().manual_seed(3)).cuda()

    def run():
        out = m(ids, types)
        (out.float() * w).sum().backward()
        return out.detach(), _grads(m)
    with _packing_state() as P:
        res = _arms(P, run)
    out_d, g_d, _ = res[1]
    for arm, rows in ((2, ROWS_OFF), (3, ROWS_PRIMED)):
        out_p, g_p, history = res[arm]
        assert history == [(N, S_READER, rows)], history
        assert bool(torch.isfinite(out_p.float()).all()) and _all_finite(g_p) == []
        ratios = {k: _rel(g_p[k], g_d[k]) for k in g_d}
        print("BERT tower, arm %d (rows %d): output %.3g (1e-5), worst gradient %.3g at %s (2e-3)"
              % (arm, rows, _rel(out_p, out_d), max(ratios.values()), max(ratios, key=ratios.get)))
        assert _rel(out_p, out_d) < 1e-5, _rel(out_p, out_d)
        bad = {k: r for k, r in ratios.items() if not r < 2e-3}
        assert set(g_p) == set(g_d) and not bad, bad
    print("BERT tower, arm 3 against arm 2: output bit-equal %s" % torch.equal(res[3][0], res[2][0]))
    assert _rel(res[3][0], res[2][0]) < 1e-5


def test_packed_self_attention_with_a_tail_of_46_tiles():
    """Packed self-attention, heads 2, over the arm-3 layout (74,000 tokens in 86,016 rows): the tail of the output and of the QKV gradient
    is exactly 0, and five sequences agree with the dense launch within the bounds of test_packed_self_attention_equals_dense."""
    from emdr2_amd.model import kernels as K
    heads = 2
    ids_np, lens = _grid(N, S_READER, TOTAL, 51, PINS)
    ids_t = _dev(ids_np)
    real = ids_t != 0
    g = torch.Generator(device="cuda").manual_seed(51)
    qkv = torch.randn((N, S_READER, 3, heads, 64), generator=g, device="cuda").bfloat16().requires_grad_(True)
    out_d = K.attention_core(qkv, None, ids_t, ids_t, False)
    w = torch.randn(out_d.shape, generator=g, device="cuda") * real[..., None, None]
    (out_d.float() * w).sum().backward()
    grad_d = qkv.grad.clone()
    qkv.grad = None
    with _packing_state() as P:
        _prime(P)
        seqs = K.PackedSeqs(ids_t)
        assert (seqs.rows, seqs.total) == (ROWS_PRIMED, TOTAL) and (seqs.rows - seqs.total) // 256 == 46
        qkv_p = K.pack_rows(qkv.detach().reshape(N, S_READER, -1), seqs).reshape(seqs.rows, 3, heads, 64).detach().requires_grad_(True)
        _poison()
        out_p = K.attention_core(qkv_p, None, seqs, seqs, False)
        assert out_p.shape == (seqs.rows, heads, 64) and float(out_p.detach()[TOTAL:].float().abs().max()) == 0.0
        back = K.unpack_rows(out_p.reshape(seqs.rows, -1), seqs).reshape(N, S_READER, heads, 64)
        (back.float() * w).sum().backward()
    gp = qkv_p.grad
    assert gp.shape == qkv_p.shape and not bool(gp[TOTAL:].view(torch.int16).any())          # +0 in every bit, NaN included
    assert bool(torch.isfinite(gp.float()).all())
    cu = seqs.cu.cpu().numpy()
    ragged = next(i for i in range(3, N) if 1 < lens[i] < S_READER and lens[i] % 32)
    assert lens[1] == 1 and lens[2] == S_READER
    for i in (0, N - 1, 1, 2, ragged):                                                       # first, last, one token, all 256, a ragged one
        ln, c0 = int(lens[i]), int(cu[i])
        e_out, e_grad = _rel(back[i, :ln], out_d[i, :ln]), _rel(gp[c0:c0 + ln], grad_d[i, :ln])
        assert e_out < 1e-5 and e_grad < 2e-3, (i, ln, e_out, e_grad)
