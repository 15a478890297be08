"""Numpy restatement of the packed ("varlen") sequence layout of include/emdr2_ops.h ("packed sequences", csrc/seqpack.hip) -- the
pattern of tests/answer_match_ref.py: the contract stated once more, vectorised, with no kernel in sight; tests/test_seqpack_ref_cpu.py
checks it against a naive loop over the sequences, tests/test_seqpack_edges_gpu.py holds the kernels to it bit for bit.

The contract.  ids is an [n, S] grid of token ids, 0 = [PAD].  Sequence i keeps its first len[i] positions,

    len[i] = 1 + index of the LAST non-zero id of row i          (zeros before it stay inside the sequence)
    len[i] = S                                                   when the row holds no token at all (the reference's uniform attention)

and the sequences are stored back to back: cu = exclusive prefix sum of len (int32 [n + 1]), total = cu[n],

    packed row t = cu[i] + pos   <->   dense row i * S + pos,    pos < len[i]
    rowmap[t]        (int32 [rows_padded]) = i * S + pos, -1 for total <= t < rows_padded (the tail rows)
    inverse[i*S+pos] (int32 [n * S])       = cu[i] + pos, -1 for pos >= len[i]            (the dropped rows)
    ids_packed[t], types_packed[t] (int64 [rows_padded]) = the grid's value at rowmap[t], 0 in the tail

emdr2_seq_lengths also reports sum len^2 (a 64-bit count: 40 full rows of 8,192 are already past 2^31) and max len.
Rows of H 16-bit words move by   gather: out[r] = map[r] >= 0 ? in[map[r]] : +0   and   scatter: out[map[r]] = in[r] for map[r] >= 0
(distinct targets; rows of `out` that no entry names keep what they held)."""
import numpy as np


def lengths(ids):
    """ids [n, S] -> (cu int32 [n + 1], total, sum len^2 as a Python int, max len)."""
    ids = np.asarray(ids)
    n, S = ids.shape
    token = ids != 0
    last = S - 1 - np.argmax(token[:, ::-1], axis=1)                 # the last non-zero position of a row that has one
    ln = np.where(token.any(axis=1), last + 1, S).astype(np.int64)
    cu = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(ln, out=cu[1:])
    return cu.astype(np.int32), int(cu[n]), sum(int(v) * int(v) for v in ln), int(ln.max())


def layout(ids, types, cu, rows_padded):
    """-> (rowmap int32 [rows_padded], inverse int32 [n * S], ids_packed int64 [rows_padded], types_packed likewise or None)."""
    ids = np.asarray(ids)
    n, S = ids.shape
    cu = np.asarray(cu).astype(np.int64)
    ln, total = np.diff(cu), int(cu[n])
    if rows_padded < total:
        raise ValueError("rows_padded < total")
    seq = np.repeat(np.arange(n, dtype=np.int64), ln)
    pos = np.arange(total, dtype=np.int64) - np.repeat(cu[:-1], ln)
    rowmap = np.full(rows_padded, -1, dtype=np.int32)
    rowmap[:total] = seq * S + pos
    inverse = np.full(n * S, -1, dtype=np.int32)
    inverse[rowmap[:total]] = np.arange(total, dtype=np.int32)

    def packed(grid):
        out = np.zeros(rows_padded, dtype=np.int64)
        out[:total] = np.asarray(grid).reshape(-1)[rowmap[:total]]
        return out
    return rowmap, inverse, packed(ids), (packed(types) if types is not None else None)


# ---- input families -------------------------------------------------------------------------------------------------------------------
KINDS = ("all_pad", "last_only", "first_only", "interior_zeros")


def grid_from_lengths(lens, S, rng, vocab=1000):
    """int64 [n, S]: row i holds lens[i] non-zero ids and zeros behind them."""
    lens = np.asarray(lens)
    ids = rng.integers(5, vocab, size=(len(lens), S)).astype(np.int64)
    ids[np.arange(S)[None, :] >= lens[:, None]] = 0
    return ids


def lengths_with_total(n, S, total, rng, pins=None, lo=1):
    """n lengths in [lo, S] that sum to `total` exactly; pins {row: length} are kept."""
    pins = dict(pins or {})
    lens = rng.integers(lo, S + 1, size=n).astype(np.int64)
    for r, v in pins.items():
        lens[r] = v
    free = np.array([r for r in range(n) if r not in pins])
    diff = int(total - lens.sum())
    while diff:                                                        # spread the difference over the free rows, a pass at a time
        room = (S - lens[free]) if diff > 0 else (lens[free] - lo)
        if int(room.sum()) < abs(diff):
            raise ValueError("no %d lengths in [%d, %d] sum to %d" % (n, lo, S, total))
        step = np.minimum(room, -(-abs(diff) // len(free)))             # an equal share each, as far as a row has room ...
        step = np.clip(abs(diff) - (np.cumsum(step) - step), 0, step)    # ... and no more than is left
        lens[free] += step if diff > 0 else -step
        diff = int(total - lens.sum())
    return lens


def edge_grid(n, S, rng, variant=0):
    """A ragged [n, S] grid that holds one row of every kind of KINDS the shape has room for -> (ids, {kind: row}).  A grid of fewer
    than four rows takes the kinds from `variant` on (n = 1: one kind per variant).  interior_zeros needs S >= 3."""
    ids = grid_from_lengths(rng.integers(1, S + 1, size=n), S, rng)
    rows = sorted({0, n // 3, (2 * n) // 3, n - 1}) if n >= 4 else list(range(n))
    where = {}
    for j, r in enumerate(rows):
        kind = KINDS[(j + variant) % 4]
        if kind == "interior_zeros":
            if S < 3:
                continue
            ln = int(rng.integers(3, S + 1))
            ids[r] = 0
            ids[r, 0], ids[r, ln - 1] = 5, 6                           # zeros in between, and a few tokens among them where there is room
            if ln > 4:
                ids[r, 2:ln - 1:2] = 9
        else:
            ids[r] = 0
            if kind == "last_only":
                ids[r, S - 1] = 7
            elif kind == "first_only":
                ids[r, 0] = 7
        where[kind] = r
    return ids, where


def gather(inp, map, rows_out):
    """inp uint16 [rows_in, H], map int32 [>= rows_out] -> uint16 [rows_out, H]: row map[r] of inp, +0 where map[r] < 0."""
    inp = np.asarray(inp)
    m = np.asarray(map)[:rows_out]
    out = np.zeros((rows_out, inp.shape[1]), dtype=np.uint16)
    out[m >= 0] = inp[m[m >= 0]]
    return out


def scatter(inp, map, out):
    """inp uint16 [rows_in, H], map int32 [rows_in] (distinct non-negative targets), out uint16 [rows, H] -> a copy of out with row
    map[r] = inp[r] for map[r] >= 0."""
    inp, out = np.asarray(inp), np.array(out, copy=True)
    m = np.asarray(map)[:inp.shape[0]]
    if len(np.unique(m[m >= 0])) != int((m >= 0).sum()):
        raise ValueError("scatter targets must be distinct")
    out[m[m >= 0]] = inp[m >= 0]
    return out
