"""Float64 references and error bounds of the value-norm weighted attention mass (csrc/attention_mass.hip, include/emdr2_ops.h:
emdr2_head_row_norms, emdr2_attention_key_mass_weighted), in the conventions of tests/attention_mass_ref.py, which this module imports and
leaves as it is.

Norms.  norm[h, r] = sqrt(S), S = sum_{d < 64} x[r, h, d]^2.  Bound, from the kernel's order of operations:

  * the 64 squares are exact in fp32 (bf16 x bf16: 16 significant bits);
  * additions: a lane adds its 8 squares in order (7 additions), a 3-level xor butterfly over the 8 lanes of the (row, head) (3):
    NORM_DEPTH = 10 roundings of partial sums that never exceed S (1 + 10 2^-24): |S' - S| <= 10 2^-24 S (1 + 10 2^-24);
  * fp32 flushes below 2^-126: each of the 64 squares and each of the 10 partial sums may lose up to TINY: + 74 TINY on S';
  * |sqrt(S') - sqrt(S)| = |S' - S| / (sqrt(S') + sqrt(S)) <= min(|S' - S| / sqrt(S), sqrt(|S' - S|));
  * the square root's own rounding: one fp32 ulp of the result (<= 2^-23 relative), and TINY for a flushed result.

The contract's range (include/emdr2_ops.h): relative accuracy while S is a normal fp32 number that does not overflow; rows below that are
held by the absolute TINY terms alone (sqrt(74 TINY) ~ 2^-60); an all-zero row gives exactly 0 (bound TINY).

Weighted mass.  attention_mass_ref.mass_reference with every p_ij multiplied by kw[h, j]:

    mass[b, h, g] = sum_{i : ids_q[b, i] != 0} w[b, i] sum_{j in seg g} p_ij kw_hj

  * every per-key term of that bound scales with |kw_hj|: the probability's own error p_bound |kw|, the accumulation depth;
  * one more fp32 rounding per term for the multiplication p kw: the depth grows by 1;
  * TINY per term for p (times |kw|) and for the product;
  * when kw comes from the norms kernel it differs from the true norm by at most the norms bound: + sum |w_i| (p_ij + p_bound_ij)
    kw_err_hj (`kw_errs`), and the reference is computed with the TRUE norms.
"""
import copy
import math

import torch

from tests import attention_mass_ref as MR
from tests import attention_ref as R

NORM_DEPTH = 10
U32 = MR.U32


def norms_reference(x):
    """x [rows, heads, 64] (any float dtype holding bf16 values) -> (norm float64 [heads, rows], bound [heads, rows])."""
    S = (x.double() ** 2).sum(dim=-1).t()
    norm = torch.sqrt(S)
    dS = NORM_DEPTH * U32 * S * (1.0 + NORM_DEPTH * U32) + (64 + NORM_DEPTH) * R.TINY
    through_root = torch.minimum(dS / torch.where(S > 0, norm, torch.ones_like(norm)), torch.sqrt(dS))
    through_root = torch.where(S > 0, through_root, torch.zeros_like(S))               # all-zero row: every square is exactly 0
    bound = through_root + 2.0 ** -23 * (norm + through_root) + R.TINY
    return norm, bound


def weighted_mass_reference(q, ks, ids_q, ids_ks, m, l, seg, kws, w=None, forward_stats=False, kw_errs=None):
    """The arguments of attention_mass_ref.mass_reference plus kws: per sequence, the key weights float64 [len_b, n] (as the kernel is
    given them, or -- with kw_errs, same shapes: a bound on |given - true| -- the true ones).  -> (mass float64 [b, n, G], bound)."""
    b, sq, n, d = q.shape
    G = seg.shape[1] - 1
    dev = q.device
    mass = torch.zeros((b, n, G), dtype=torch.float64, device=dev)
    bound = torch.zeros_like(mass)
    seg_l = seg.tolist()
    for i in range(b):
        k = ks[i]
        if k.shape[0] == 0:
            continue
        r = R.reference(q[i][None], k[None], torch.zeros_like(k)[None], ids_q[i][None], ids_ks[i][None], False)
        p = MR.row_probabilities(r, m[i][None], l[i][None])
        r2 = copy.copy(r)
        r2.P = p
        pb = R.p_bound(r2, R.C_F32, MR.SCORE_ROUND, True)
        counted = (ids_q[i] != 0).double()
        wi = counted if w is None else counted * w[i].double()
        aw = wi.abs()[None, None, :, None]
        kw = kws[i].double().t()[None, :, None, :]                                     # [1, n, 1, len]
        akw = kw.abs()
        kerr = kw_errs[i].double().t()[None, :, None, :] if kw_errs is not None else None
        lse_w = torch.expm1(R.lse_bound(r))[0, :, :, None] if forward_stats else None
        for g in range(G):
            lo, hi = seg_l[i][g], seg_l[i][g + 1]
            if hi <= lo:
                continue
            pg, kg, ag = p[..., lo:hi], kw[..., lo:hi], akw[..., lo:hi]
            mass[i, :, g] = (wi[None, None, :, None] * pg * kg).sum(dim=(-1, -2))[0]
            terms = (aw * pg * ag).sum(dim=(-1, -2))[0]
            bd = (aw * pb[..., lo:hi] * ag).sum(dim=(-1, -2))[0] + (MR.reduction_depth(hi - lo) + 1) * U32 * terms
            bd = bd + R.TINY * float(aw.sum()) * (ag.sum(dim=(-1, -2))[0] + (hi - lo))
            if kerr is not None:
                bd = bd + (aw * (pg + pb[..., lo:hi]) * kerr[..., lo:hi]).sum(dim=(-1, -2))[0]
            if forward_stats:
                bd = bd + (aw[0] * lse_w * pg[0] * ag[0]).sum(dim=(-1, -2))
            bound[i, :, g] = bd
    bound = bound + R._ulp(mass, 23) + R.TINY
    return mass, bound


def brute_force_weighted_mass(q, k, ids_q, ids_k, seg, kw, w=None):
    """The definition without the (m, l) detour, for ONE sequence and tiny inputs: python loops over float64 softmax rows.
    q [sq, n, d], k [sk, n, d], ids [sq] / [sk], seg [G + 1], kw [sk][n], w [sq] or None -> [n, G] as nested lists."""
    sq, n, d = q.shape
    sk = k.shape[0]
    scale = 1.0 / math.sqrt(d)
    G = len(seg) - 1
    out = [[0.0] * G for _ in range(n)]
    for h in range(n):
        for i in range(sq):
            if int(ids_q[i]) == 0:
                continue
            s = [R.MASK_VALUE if int(ids_k[j]) == 0 else scale * float((q[i, h].double() * k[j, h].double()).sum()) for j in range(sk)]
            mx = max(s)
            e = [math.exp(v - mx) for v in s]
            z = sum(e)
            for g in range(G):
                out[h][g] += (1.0 if w is None else float(w[i])) * sum(e[j] * float(kw[j][h]) for j in range(int(seg[g]), int(seg[g + 1]))) / z
    return out


def brute_force_norms(x):
    """x [rows, heads, 64] -> [heads][rows] with python floats (math.fsum: no order to speak of)."""
    rows, heads, _ = x.shape
    xl = x.double().tolist()
    return [[math.sqrt(math.fsum(v * v for v in xl[r][h])) for r in range(rows)] for h in range(heads)]


def distill_kl_reference(logp, target, batch):
    """distill_kl with python floats: logp, target as nested lists [b][K] -> (loss, gradient [b][K] = -t / B)."""
    loss = 0.0
    for lrow, trow in zip(logp, target):
        for lp, t in zip(lrow, trow):
            if t > 0:
                loss += t * (math.log(t) - lp)
    return loss / batch, [[-t / batch for t in trow] for trow in target]
