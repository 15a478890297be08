"""numpy restatement of the optimizer-state audit, written from the text of include/emdr2_ops.h ("State audit"): the digest of the three
fp32 arrays (pair terms, block keys, (sum, xor)), f2bf (csrc/prims.h: round to nearest even in software, quiet NaN) and the five checks
with their first offenders.  Every array is handled as its bit patterns (uint32 / uint16)."""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
BLOCK = 8192
TAGS = tuple(np.uint64(t << 32) for t in (0x4D535452, 0x45585041, 0x45585053))       # master, exp_avg, exp_avg_sq
NONE = (1 << 64) - 1
WORDS = 18
CHECKS = ("nonfinite_master", "nonfinite_exp_avg", "nonfinite_exp_avg_sq", "negative_exp_avg_sq", "work_mismatch")


def mix(z):
    """splitmix64's finaliser on uint64 arrays (arithmetic mod 2^64)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def block_keys(w, a):
    """key_a(j) for every block of one array: w uint32 [n], n even."""
    w = np.ascontiguousarray(w, dtype=np.uint32)
    n = w.size
    p = np.arange(n // 2, dtype=np.uint64)
    with np.errstate(over="ignore"):
        e = mix(((w[1::2].astype(np.uint64) << np.uint64(32)) | w[0::2].astype(np.uint64)) + (p + np.uint64(1)) * G)
        n_blocks = (n + BLOCK - 1) // BLOCK
        sums = np.add.reduceat(e, np.arange(0, n // 2, BLOCK // 2))        # uint64 sums wrap mod 2^64
        j = np.arange(n_blocks, dtype=np.uint64)
        return mix(sums ^ ((j + np.uint64(1)) * G) ^ TAGS[a])


def digest(keys):
    """(sum mod 2^64, xor) over an array's block keys, as Python ints."""
    with np.errstate(over="ignore"):
        return int(np.add.reduce(keys)), int(np.bitwise_xor.reduce(keys))


def f2bf(w):
    """bf16 bits of fp32 bits: round to nearest even, a NaN keeps its top payload bits and is made quiet."""
    w = np.asarray(w, dtype=np.uint32)
    nan = (w & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    rounded = (w.astype(np.uint64) + np.uint64(0x7fff) + ((w >> np.uint32(16)) & np.uint32(1)).astype(np.uint64)) >> np.uint64(16)
    return np.where(nan, (w >> np.uint32(16)) | np.uint32(0x40), rounded.astype(np.uint32) & np.uint32(0xffff)).astype(np.uint16)


def checks(master, m, v, work):
    """[(count, first index or NONE)] for the five checks, in the report's order: uint32 bits of master, m, v, uint16 bits of work."""
    nonfinite = lambda w: (w & np.uint32(0x7fffffff)) >= np.uint32(0x7f800000)
    v_abs = v & np.uint32(0x7fffffff)
    negative = ((v >> np.uint32(31)) == 1) & (v_abs != 0) & (v_abs <= np.uint32(0x7f800000))       # v < 0 as IEEE compares: not -0.0, not NaN
    out = []
    for hit in (nonfinite(master), nonfinite(m), nonfinite(v), negative, f2bf(master) != work):
        idx = np.flatnonzero(hit)
        out.append((int(idx.size), int(idx[0]) if idx.size else NONE))
    return out


def report(master, m, v, work):
    """The 18 report words (Python ints, unsigned) and the block keys [3 * n_blocks] of one bucket."""
    keys = [block_keys(x, a) for a, x in enumerate((master, m, v))]
    c = checks(master, m, v, work)
    words = [master.size] + [x[0] for x in c] + [x[1] for x in c]
    for k in keys:
        words += list(digest(k))
    words.append(keys[0].size)
    assert len(words) == WORDS
    return words, np.concatenate(keys)
