"""CPU study of the int8 MFMA filter of csrc/mips_scan8i.hip: a numpy restatement of its quantisation, block constants and
integer threshold, and, on >= 1 M synthetic rows, how loose the rigorous bound is and how many rows pass it compared with the fp16 filter.

    python tools/mips_i8_filter_study.py [--rows 1000192] [--queries 16] [--dim 768]  > profiles/mips_i8_filter_study.txt

The restatement is what tests/test_mips_i8_bound_cpu.py checks against float64 scores; the functions mirror the kernels operation by
operation in float32 (seal_shadow_kernel, pack_queries_i8_kernel, s8i_theta).  No GPU needed.
"""
import argparse
import sys

import numpy as np

BLOCK = 256
F = np.float32


def quantise_blocks(rows):
    """rows fp16 [N, dim] -> (e8 int8 [N, dim], blk float32 [ceil(N / 256), 3] = s_b, N_b, D_b): one scale per 256-row block,
    s_b = max|e| / 127, rows stored as rint(e / s_b) (no clipping), N_b = max row norm, D_b = max ||e_r - s_b e8_r||, both rounded up by
    0.1 % like emax_sq (D_b also by 2^-22 N_b for the float32 evaluation of the residual).  An all-zero block has s_b = 0 and stores zeros."""
    n, dim = rows.shape
    nb = (n + BLOCK - 1) // BLOCK
    e8 = np.zeros((n, dim), dtype=np.int8)
    blk = np.zeros((nb, 3), dtype=F)
    for b in range(nb):
        x = rows[b * BLOCK:(b + 1) * BLOCK].astype(F)
        amax = F(np.abs(x).max()) if x.size else F(0)
        s = F(amax / F(127))
        inv = F(F(127) / amax) if s > 0 else F(0)
        qv = np.clip(np.rint(x * inv), -127, 127).astype(F)
        r = x - s * qv
        n2 = (x * x).sum(axis=1, dtype=F).max()
        d2 = (r * r).sum(axis=1, dtype=F).max()
        e8[b * BLOCK:(b + 1) * BLOCK] = qv.astype(np.int8)
        nrm = np.sqrt(F(n2)) * F(1.001)
        blk[b] = (s, nrm, (np.sqrt(F(d2)) + nrm * F(2.0 ** -22)) * F(1.001))          # (+ 2^-22 N_b: the residual was evaluated in float32)
    return e8, blk


def quantise_queries(queries):
    """queries fp16 [Q, dim] -> (q8 int8 [Q, dim], qc float32 [Q, 3] = t_q, a_q = ||q - t_q q8|| (up), b_q = ||t_q q8|| (up))."""
    x = queries.astype(F)
    amax = np.abs(x).max(axis=1).astype(F)
    t = (amax / F(127)).astype(F)
    inv = np.where(t > 0, F(127) / np.where(amax > 0, amax, F(1)), F(0)).astype(F)
    qv = np.clip(np.rint(x * inv[:, None]), -127, 127).astype(F)
    y = t[:, None] * qv
    r = x - y
    ra, rb = np.sqrt((r * r).sum(axis=1, dtype=F)), np.sqrt((y * y).sum(axis=1, dtype=F))
    a = (ra + (ra + rb) * F(2.0 ** -22)) * F(1.001)
    b = rb * F(1.001)
    return qv.astype(np.int8), np.stack([t, a, b], axis=1).astype(F)


def epsilon(qc, blk):
    """eps(q, b) = (a_q N_b + b_q D_b) * 1.0001 in float32, [Q, blocks]: |S - t_q s_b I| <= eps for every row of the block."""
    return ((qc[:, 1:2] * blk[None, :, 1] + qc[:, 2:3] * blk[None, :, 2]) * F(1.0001)).astype(F)


def theta(tau, qc, blk):
    """Integer thresholds [Q, blocks] (int64 holding int32 values): a row is pruned iff I < Theta.  float32 throughout, every step errs
    downwards; +inf tau prunes everything, a zero scale / -inf tau / NaN prunes nothing (s8i_theta)."""
    tau = np.asarray(tau, dtype=F)[:, None]
    ts = (qc[:, 0:1] * blk[None, :, 0]).astype(F)
    with np.errstate(all="ignore"):
        num = (tau - epsilon(qc, blk)).astype(F)
        num = (num - np.abs(num) * F(1e-6)).astype(F)
        x = (num * (F(1) / ts)).astype(F)
        x = (x - np.abs(x) * F(1e-5)).astype(F)
        x = (np.floor(x) - F(1)).astype(F)
    lo, hi = -(1 << 31), (1 << 31) - 1
    out = np.full(x.shape, lo, dtype=np.int64)
    ok = (ts > 0) & (x > F(-2.0e9))
    out[ok] = np.where(x[ok] > F(2.0e9), hi, x[ok].astype(np.float64)).astype(np.int64)
    out[np.broadcast_to(tau == np.inf, x.shape)] = hi
    return out


def int_scores(e8, q8):
    """I[q, r] = sum_k q8 e8, exact (float64 matmul of small integers: |I| <= dim * 127^2 < 2^53)."""
    return (q8.astype(np.float64) @ e8.astype(np.float64).T).astype(np.int64)


def study(n_rows, n_q, dim, seed, out):
    rng = np.random.default_rng(seed)
    queries = rng.standard_normal((n_q, dim)).astype(np.float16)
    q8, qc = quantise_queries(queries)
    S = np.empty((n_q, n_rows), dtype=np.float64)
    I = np.empty((n_q, n_rows), dtype=np.int64)
    nb = (n_rows + BLOCK - 1) // BLOCK
    blk = np.empty((nb, 3), dtype=F)
    step = 256 * BLOCK
    for lo in range(0, n_rows, step):
        rows = rng.standard_normal((min(step, n_rows - lo), dim)).astype(np.float16)
        e8, b = quantise_blocks(rows)
        blk[lo // BLOCK: lo // BLOCK + b.shape[0]] = b
        S[:, lo:lo + rows.shape[0]] = queries.astype(np.float64) @ rows.astype(np.float64).T
        I[:, lo:lo + rows.shape[0]] = int_scores(e8, q8)
    blk_of = np.arange(n_rows) // BLOCK
    eps = epsilon(qc, blk).astype(np.float64)
    approx = qc[:, 0:1].astype(np.float64) * blk[blk_of, 0].astype(np.float64)[None, :] * I
    err = np.abs(S - approx)
    p = lambda *a: print(*a, file=out)
    p("int8 filter study: %d rows x %d queries, dim %d, rows and queries fp16(N(0,1)), seed %d" % (n_rows, n_q, dim, seed))
    p("score std %.1f; |I| max %d" % (S.std(), np.abs(I).max()))
    p("observed |filter - exact|: max %.2f; rigorous eps: median %.1f, max %.1f; observed / eps max %.3f; bound violations: %d"
      % (err.max(), np.median(eps), eps.max(), (err / eps[:, blk_of]).max(), int((err > eps[:, blk_of]).sum())))
    for label, frac in (("tau = 64th best of the first 20 % of the rows", 0.2), ("tau = 64th best of the first 12.5 %", 0.125), ("final tau (64th best of all rows)", 1.0)):
        head = max(64, int(n_rows * frac))
        tau = np.sort(S[:, :head], axis=1)[:, -64].astype(F)               # (rounding tau to float32 as the kernel holds it)
        th = theta(tau, qc, blk)
        rest = slice(head, n_rows) if frac < 1.0 else slice(0, n_rows)
        pass8 = I[:, rest] >= th[:, blk_of[rest]]
        pass16 = S[:, rest] >= tau[:, None].astype(np.float64)
        missed = int((pass16 & ~pass8).sum())
        p("%s: int8 survivors per query mean %.0f (max %d), fp16 filter %.0f (max %d), ratio %.1f; true candidates missed: %d"
          % (label, pass8.sum(axis=1).mean(), pass8.sum(axis=1).max(), pass16.sum(axis=1).mean(), pass16.sum(axis=1).max(),
             pass8.sum() / max(pass16.sum(), 1), missed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000192)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()
    study(a.rows, a.queries, a.dim, a.seed, sys.stdout)


if __name__ == "__main__":
    main()
