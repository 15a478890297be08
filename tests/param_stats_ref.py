"""numpy restatement of the parameter statistics, written from the text of include/emdr2_ops.h ("Parameter statistics"): the plan (a
parameter is cut into chunks of 8192 elements from its own start), the eight words per parameter and THE ORDER of the float64 additions
(per thread groups and elements ascending, the xor butterfly over a wave, the four waves as (w0 + w1) + (w2 + w3), then per parameter
eight lane groups over the items and a butterfly over the groups).  `fsum_sq` is an independent truth: math.fsum, no order at all."""
import math

import numpy as np

CHUNK = 8192
WORDS = 8
THREADS = 256
INF_BITS = 0x7f800000


def plan(offsets, lengths, n):
    """(items int64 [n_items, 2], first int64 [n_params + 1]); ValueError where the entry returns -1."""
    if len(offsets) < 1 or len(offsets) != len(lengths) or n < 8 or n % 8:
        raise ValueError("malformed")
    items, first, end = [], [0], 0
    for off, length in zip(offsets, lengths):
        if off < end or off % 8 or length < 1 or off + length > n:
            raise ValueError("malformed")
        end = off + length
        items += [(off + at, min(CHUNK, length - at)) for at in range(0, length, CHUNK)]
        first.append(len(items))
    return np.array(items, dtype=np.int64).reshape(-1, 2), np.array(first, dtype=np.int64)


def bias_corrections(beta1, beta2, step):
    """fp32, as csrc/adam_bias.h: 1 - powf(beta, (float)step).  (Exact for the betas the tests use, whatever powf does.)"""
    f = np.float32
    return f(1) - f(np.power(f(beta1), f(step))), f(1) - f(np.power(f(beta2), f(step)))


def direction64(m, v, beta1, beta2, eps, step):
    """d in float64 from the fp32 inputs and the fp32 bc1 / bc2 / eps: what the device's fp32 d is compared with."""
    bc1, bc2 = bias_corrections(beta1, beta2, step)
    return (m.astype(np.float64) / np.float64(bc1)) / (np.sqrt(v.astype(np.float64) / np.float64(bc2)) + np.float64(np.float32(eps)))


def _butterfly(x, offsets):
    """x[..., L]: x += x[lane ^ o] for o in offsets, every lane at once (what __shfl_xor does)."""
    lanes = np.arange(x.shape[-1])
    for o in offsets:
        x = x + x[..., lanes ^ o]
    return x


def _item_sums(sq):
    """sq float64 [items, 8192], masked elements already 0.0 (x + 0.0 == x for the non-negative sums here) -> the items' record sums."""
    k = sq.reshape(sq.shape[0], CHUNK // (4 * THREADS), THREADS, 4)      # element 4 (256 k + t) + j of the item
    acc = np.zeros((sq.shape[0], THREADS), dtype=np.float64)
    for step in range(k.shape[1]):                                       # 1. per thread: groups ascending, elements ascending
        for j in range(4):
            acc = acc + k[:, step, :, j]
    w = _butterfly(acc.reshape(-1, 4, 64), (32, 16, 8, 4, 2, 1))[:, :, 0]    # 2. the wave
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])                     # 3. the four waves


def _fold(records, op, zero):
    """4. eight lane groups over the items (s, s + 8, ... ascending, from `zero`), then the butterfly over the groups: 4, 2, 1."""
    acc = []
    for s in range(8):
        a = zero
        for r in records[s::8]:
            a = op(a, r)
        acc.append(a)
    for o in (4, 2, 1):
        acc = [op(acc[s], acc[s ^ o]) for s in range(8)]
    return acc[0]


def _padded(x, fill=0):
    items = -(-x.size // CHUNK)
    out = np.full(items * CHUNK, fill, dtype=x.dtype)
    out[:x.size] = x
    return out.reshape(items, CHUNK)


def ordered_sum_sq(x):
    """sum x^2 of one parameter (fp32 or float64 values) in the stated order, as a float64."""
    sq = _padded(x.astype(np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        return _fold(list(_item_sums(sq * sq)), lambda a, b: a + b, np.float64(0.0))


def fsum_sq(x):
    return math.fsum(float(t) * float(t) for t in x.astype(np.float64))


def words(g, w, d=None):
    """The eight words of one parameter as Python ints (unsigned): g, w fp32 arrays of its elements; d: its fp32 directions, None for
    step 0.  Word 2 is the ordered sum of the GIVEN d (the device forms its own d in fp32: compare that word with a tolerance)."""
    g, w = np.ascontiguousarray(g, dtype=np.float32), np.ascontiguousarray(w, dtype=np.float32)
    bits = lambda x: int(np.float64(x).view(np.uint64))
    ga, wa = g.view(np.uint32) & np.uint32(0x7fffffff), w.view(np.uint32) & np.uint32(0x7fffffff)
    top = lambda a: int(a[a <= INF_BITS].max()) if (a <= INF_BITS).any() else 0
    return [bits(ordered_sum_sq(g)), bits(ordered_sum_sq(w)), bits(ordered_sum_sq(d)) if d is not None else 0, top(ga), top(wa),
            int((ga == 0).sum()), int((ga >= INF_BITS).sum()), int(g.size)]
