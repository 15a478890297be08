"""Float64 restatement (numpy) and error bounds of the ordered-sum entries of include/emdr2_ops.h (emdr2_gemm_tn_bf16_ordered,
emdr2_layernorm_bwd_ordered, emdr2_embedding_bwd_ordered), from the STORED inputs: bf16 activations widened exactly, fp32 statistics as given.

Every quantity is a sum of n terms into one destination, plus the value p the destination held:

    dW[i, j]   = p + sum_r A[r, i] B[r, j]                 colsum[i] = p + sum_r A[r, i]              (terms exact in fp32: bf16 x bf16)
    dgamma[c]  = p + sum_r dy[r, c] xhat[r, c]             dbeta[c]  = p + sum_r dy[r, c]             xhat = (x - mean) * rstd
    dW[v]      = p + sum_{t: ids[t] = v} g[t]              dP[pos], dT[k] alike                       g = keep ? dout * scale : 0

Bound (the derivation of tests/gemm_ref.py): n terms summed in fp32 in ANY order differ from the exact sum by at most gamma_n sum |term|,
gamma_n = n u / (1 - n u), u = 2^-24.  The add onto the destination is one more term (|p| joins the majorant), and two spare terms cover the
kernels' start from +0.0 and the split of a sum into partials: n + 3 in all.  Where a term is itself computed in fp32 its relative rounding
error e_t is added to first order and carried through the sum:

    bound = (gamma_{n+3} (1 + e_t) + e_t) (sum |term| + |p|) + n TINY
    e_t   = 0 (GEMM, colsum, dbeta);  gamma_3 (dgamma: the subtraction, the product with rstd, the product with dy);  gamma_1 (a kept
            embedding element times the fp32 keep scale; 0 without dropout)

No constant here comes from the kernels' output.  tests/test_ordered_grads_cpu.py checks the restatement against per-element loops."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149


def gamma(n):
    return n * U / (1.0 - n * U)


def sum_bound(majorant, n, prefill_abs=0.0, e_term=0.0):
    return (gamma(n + 3) * (1.0 + e_term) + e_term) * (majorant + prefill_abs) + n * TINY


def to_bf16(a):
    """float -> the nearest bf16 value (ties to even), returned as float32."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return b.astype(np.uint32).view(np.float32)


def bf16_bits(a):
    """the int16 storage of an array of bf16-valued float32."""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


def spread(shape, rng, lo=-20, hi=20):
    """bf16 values whose magnitudes spread over 2^lo .. 2^hi: data on which the order of a sum shows in its last bits."""
    return to_bf16(rng.standard_normal(shape) * np.exp2(rng.integers(lo, hi + 1, size=shape)))


# ---- weight-gradient GEMM ---------------------------------------------------------------------------------------------------------------------
def tn_reference(A, B):
    """A [R, I], B [R, J] (bf16 values) -> dW [I, J], its majorant, colsum [I], its majorant (float64)."""
    a, b = A.astype(np.float64), B.astype(np.float64)
    return a.T @ b, np.abs(a).T @ np.abs(b), a.sum(0), np.abs(a).sum(0)


def tn_reference_loop(A, B, i, j):
    s = m = 0.0
    for r in range(A.shape[0]):
        t = float(A[r, i]) * float(B[r, j])
        s += t
        m += abs(t)
    return s, m


# ---- LayerNorm backward: gain / bias gradients ------------------------------------------------------------------------------------------------
E_XHAT = gamma(3)


def ln_reference(dy, x, mean, rstd):
    """dy, x [rows, H] (bf16 values), mean, rstd [rows] fp32 as stored -> dgamma, its majorant, dbeta, its majorant."""
    d = dy.astype(np.float64)
    xh = (x.astype(np.float64) - mean.astype(np.float64)[:, None]) * rstd.astype(np.float64)[:, None]
    return (d * xh).sum(0), np.abs(d * xh).sum(0), d.sum(0), np.abs(d).sum(0)


def ln_reference_loop(dy, x, mean, rstd, c):
    sg = mg = sb = mb = 0.0
    for r in range(dy.shape[0]):
        t = float(dy[r, c]) * ((float(x[r, c]) - float(mean[r])) * float(rstd[r]))
        sg += t; mg += abs(t); sb += float(dy[r, c]); mb += abs(float(dy[r, c]))
    return sg, mg, sb, mb


# ---- embedding backward -------------------------------------------------------------------------------------------------------------------------
def embedding_reference(ids, types, dout, keep, scale, positions, V, P_rows, n_types):
    """ids, types (or None), positions [tokens] (position of each token in its sequence, -1 = a tail row that belongs to no sequence), dout
    [tokens, H] bf16 values, keep bool [tokens, H], scale = the fp32 keep scale -> {name: (sum, majorant, terms per destination row)}."""
    g = np.where(keep, dout.astype(np.float64) * float(scale), 0.0)
    H = g.shape[1]
    out = {}

    def scatter(rows, idx, sel):
        s, m, n = np.zeros((rows, H)), np.zeros((rows, H)), np.zeros(rows, dtype=np.int64)
        np.add.at(s, idx[sel], g[sel]); np.add.at(m, idx[sel], np.abs(g[sel])); np.add.at(n, idx[sel], 1)
        return s, m, n

    out["dW"] = scatter(V, ids, np.ones(len(ids), dtype=bool))
    real = positions >= 0
    out["dP"] = scatter(P_rows, positions, real)
    if types is not None:
        out["dT"] = scatter(n_types, types, real)
    return out


def embedding_reference_loop(ids, dout, keep, scale, v, c):
    s = m = 0.0
    n = 0
    for t in range(len(ids)):
        if ids[t] == v:
            n += 1
            if keep[t, c]:
                s += float(dout[t, c]) * float(scale); m += abs(float(dout[t, c]) * float(scale))
    return s, m, n
