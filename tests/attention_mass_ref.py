"""Float64 reference and error bound of the attention key-mass kernel (csrc/attention_mass.hip, include/emdr2_ops.h:
emdr2_attention_key_mass), in the conventions of tests/attention_ref.py, which this module imports and leaves as it is.

Reference.  With s = attention_ref.reference(...).s (scaled scores, masked ones REPLACED by -10000), the GIVEN row statistics (m, l)
taken to float64 and the segment table:

    p_ij          = exp(s_ij - (m_i + ln l_i))
    mass[b, h, g] = sum_{i : ids_q[b, i] != 0} w[b, i] sum_{j in seg g} p_ij

Bound, from the kernel's order of operations:

  * p_ij: the score is an fp32 MFMA dot product of 64 exact bf16 products (|ds| <= 64 2^-24 scale sum_d |q_id k_jd|, an error in the
    exponent: score_round = 2 * 64 * 2^-24 on score_abs, as for the fp32 validation path), times scale log2 e (one rounding, relative to
    |s|), minus the offset (m + ln l) log2 e folded once per query as fma(m, log2 e, log2 l) (<= 3 2^-24 (|m| log2 e + |log2 l|), and
    |m + ln l| <= max_j |s_ij| + ln sk), v_exp_f32 (1 ulp): attention_ref.p_bound(r, C_F32, score_round, score_abs=True) with P = p_ij;
    C_F32 = 2^-18 = 64 ulp holds the terms that do not grow with |s|, the score_round term those that do.
  * summed over the segment with |w_i|.
  * fp32 accumulation: depth 2^-24 sum |terms|.  The reduction the kernel builds, for a segment of n keys: a lane adds the 4 keys it
    holds of each 16-key group its wave walks -- 4 ceil(ceil(n / 16) / 4) sequential additions --, multiplies by the weight (1), adds
    its <= 8 query tiles in order (8), a 6-level butterfly over the 64 lanes (6), the 4 waves in order (3): `reduction_depth`.
  * TINY per term (fp32 flushes below 2^-126) and one fp32 ulp of the reference.
  * statistics that come from the project's forward instead of the test carry that forward's own error |m + ln l - lse| <=
    attention_ref.lse_bound(r) in the exponent of every p_ij of the row: + sum_i |w_i| expm1(lse_bound_i) sum_j p_ij (`forward_stats`).

Not covered, by construction of the fold: a row whose keys are ALL masked has |m + ln l| ~ 10000, where one fp32 ulp of the offset is
1e-3 of p; with the forward's statistics the lse term above holds it, with test-made statistics no case builds such a row.
"""
import copy
import math

import torch

from tests import attention_ref as R

SCORE_ROUND = 2.0 * 64 * 2.0 ** -24
U32 = 2.0 ** -24


def reduction_depth(n_keys):
    """Depth of the fp32 reduction of a segment of n_keys keys (module docstring): tensor or int -> same."""
    groups = (n_keys + 15) // 16
    return 4 * ((groups + 3) // 4) + 1 + 8 + 6 + 3


def made_stats(r):
    """(m, l) fp32 [b, n, sq] as a test makes them from the float64 scores: the row maximum and the row sum of exp(s - m)."""
    m = r.s.amax(dim=-1).float()
    l = torch.exp(r.s - m.double()[..., None]).sum(dim=-1).float()
    return m, l


def row_probabilities(r, m, l):
    """p_ij of the module docstring, float64 [b, n, sq, sk]."""
    return torch.exp(r.s - (m.double() + torch.log(l.double()))[..., None])


def mass_reference(q, ks, ids_q, ids_ks, m, l, seg, w=None, forward_stats=False):
    """q [b, sq, n, d]; ks, ids_ks: per sequence, keys [len_b, n, d] and their token ids [len_b] (a dense [b, sk, ...] operand is passed as
    list(k), list(ids_k)); m, l fp32 [b, n, sq]; seg int [b, G + 1]; w [b, sq] or None.
    -> (mass float64 [b, n, G], bound [b, n, G], rows float64 [b, n, sq]: each query's total over ALL keys of its sequence)."""
    b, sq, n, d = q.shape
    G = seg.shape[1] - 1
    dev = q.device
    mass = torch.zeros((b, n, G), dtype=torch.float64, device=dev)
    bound = torch.zeros_like(mass)
    rows = torch.zeros((b, n, sq), dtype=torch.float64, device=dev)
    seg_l = seg.tolist()
    for i in range(b):
        k = ks[i]
        if k.shape[0] == 0:
            continue
        r = R.reference(q[i][None], k[None], torch.zeros_like(k)[None], ids_q[i][None], ids_ks[i][None], False)
        p = row_probabilities(r, m[i][None], l[i][None])
        r2 = copy.copy(r)
        r2.P = p
        pb = R.p_bound(r2, R.C_F32, SCORE_ROUND, True)
        counted = (ids_q[i] != 0).double()
        wi = counted if w is None else counted * w[i].double()
        aw = wi.abs()[None, None, :, None]
        rows[i] = p.sum(dim=-1)[0]
        lse_w = torch.expm1(R.lse_bound(r))[0, :, :, None] if forward_stats else None          # [n, sq, 1]
        for g in range(G):
            lo, hi = seg_l[i][g], seg_l[i][g + 1]
            if hi <= lo:
                continue
            pg = p[..., lo:hi]
            mass[i, :, g] = (wi[None, None, :, None] * pg).sum(dim=(-1, -2))[0]
            terms = (aw * pg).sum(dim=(-1, -2))[0]
            bd = (aw * pb[..., lo:hi]).sum(dim=(-1, -2))[0] + reduction_depth(hi - lo) * U32 * terms + R.TINY * (hi - lo) * float(aw.sum())
            if forward_stats:
                bd = bd + (aw[0] * lse_w * pg[0]).sum(dim=(-1, -2))
            bound[i, :, g] = bd
    bound = bound + R._ulp(mass, 23) + R.TINY
    return mass, bound, rows


def brute_force_mass(q, k, ids_q, ids_k, seg, w=None):
    """The definition without the (m, l) detour, for ONE sequence and tiny inputs: python loops over float64 softmax rows.
    q [sq, n, d], k [sk, n, d], ids [sq] / [sk], seg [G + 1], w [sq] or None -> [n, G] as nested lists."""
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
                out[h][g] += (1.0 if w is None else float(w[i])) * sum(e[j] for j in range(int(seg[g]), int(seg[g + 1]))) / z
    return out


def meter_reference(mass, prior_logp, hits=None):
    """The meter's arithmetic restated with python floats: mass [B][K] (rows sum to 1 or are all zero), prior_logp [B][K], hits [B][K]
    bools or None -> dict questions, entropy, agree, hit_mass, top1_hit (sums over the counted questions)."""
    out = dict(questions=0, entropy=0.0, agree=0, hit_mass=0.0, top1_hit=0)
    for b, row in enumerate(mass):
        if sum(row) <= 0:
            continue
        out["questions"] += 1
        out["entropy"] -= sum(p * math.log(p) for p in row if p > 0)
        top = max(range(len(row)), key=lambda j: (row[j], -j))
        pri = max(range(len(row)), key=lambda j: (prior_logp[b][j], -j))
        out["agree"] += int(top == pri)
        if hits is not None:
            out["hit_mass"] += sum(p for p, h in zip(row, hits[b]) if h)
            out["top1_hit"] += int(bool(hits[b][top]))
    return out
