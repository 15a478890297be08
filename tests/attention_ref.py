"""Float64 reference, row-scaled error bounds and adversarial inputs for the attention tests (CPU and GPU tensors alike).

Reference semantics (transformer.py:283-381, restated in test_ops_gpu._attention_reference): scaled scores, masked_fill(-10000) -- the
mask value REPLACES the score --, softmax, optional multiplicative dropout mask, P V.  A row whose scores are all masked is uniform over
ALL its keys and feeds dV, but receives no dQ / dK (masked_fill cuts the dependence on the score).

Bounds.  An error is judged against a majorant of its own row, never against the largest value of the tensor: with c = 2^-7
(three independent bf16 roundings of 2^-9 each on average (2^-8 at worst) -- P or dS before the second MFMA, the bf16 O inside
D = rowsum(dO o O), the bf16 store -- plus fp32 accumulation, rounded up to a power of two)

    |O  - ref|[i, d] <= c sum_k P_ik |V_kd|
    |dV - ref|[k, d] <= c sum_i Pd_ik |dO_id|                       Pd = dropped and scaled P
    |dQ - ref|[i, d] <= c scale sum_k G_ik |K_kd|                   G_ik = P_ik (|dPd_ik| + sum_d |dO_id| |O_id|), 0 where masked
    |dK - ref|[k, d] <= c scale sum_i G_ik |Q_id|
    |m + ln l - lse|[i] <= 16 2^-24 (1 + |lse_i| + max_k |s_ik|)    fp32 unit roundoff, 16 operations of slack; the max runs over the
                                                                    row's unmasked keys (a fully masked row has |lse| ~ 10000 already)

each plus one ulp (of the output format) of the reference value.  Three terms that the measurements on the kernels asked for, each a
rounding step the list above leaves out:

  * underflow: fp32 and bf16 flush (or lose the mantissa of) anything below 2^-126, so every P_ik -- and every stored value -- carries an
    ABSOLUTE error of up to TINY = 2^-126 next to its relative one: each P_ik in the majorants is (c P_ik + TINY), each floor + TINY.
    (Found by the 4,160-key staircase: keys 90 below the row maximum have P ~ 1e-39, their dK / dV were "57 bounds" off at 1e-38.)
  * a path that rounds its SCORES to bf16 (the GEMM + softmax composition) passes `score_round` = 2^-8, the unit roundoff of bf16:
    |ds_ik| <= 2^-8 |s_ik| sits inside the exponent of P_ik (and, averaged over the row, inside its normaliser), so every P_ik in the
    majorants is weighted (c + 2^-8 |s_ik|) and lse gains 2^-8 max_k |s_ik| (logsumexp is 1-Lipschitz in the sup norm of the scores;
    a causal row 0 has lse = s_00 and shows the full rounding: measured 1.56 x 2^-9 |s|).  Masked scores are replaced, not rounded,
    and carry no such term.
  * the fp32 validation path (c = 2^-18) accumulates its scores in fp32: |ds_ik| <= hn 2^-24 scale sum_d |q_id k_kd| (the standard
    bound of an hn-term dot product), which is an error in the exponent like the one above: `score_round` = 2 hn 2^-24 applied to
    scale sum_d |q_id| |k_kd| (`score_abs`).  At |s| = 42 this is what dominates; on randn scores c alone holds with a factor 10 to spare.
"""
import math

import torch

C_BF16 = 2.0 ** -7
C_F32 = 2.0 ** -18
MASK_VALUE = -10000.0
TINY = 2.0 ** -126


def keep_scale(drop_p):
    """1 / (1 - p) of the surviving elements: p is quantised to 2^-16 (csrc/rng.h)."""
    return 65536.0 / (65536.0 - float(int(drop_p * 65536.0 + 0.5)))


class Ref(object):
    pass


def reference(q, k, v, ids_q, ids_k, causal, drop_mask=None, dO=None):
    """q [b, sq, n, d], k / v [b, sk, n, d] (any float dtype: the VALUES are taken as they are), ids [b, s] (0 = padding),
    drop_mask [b, n, sq, sk] multiplicative (0 or 1 / (1 - p)) or None, dO [b, sq, n, d] or None.  Everything in float64.
    -> Ref with O [b, sq, n, d], lse [b, n, sq], P, Pd, s (masked scaled scores), masked [b, 1|n, sq, sk], and with dO: dQ, dK, dV, dPd."""
    q, k, v = q.double(), k.double(), v.double()
    b, sq, n, d = q.shape
    sk = k.shape[1]
    r = Ref()
    r.scale = 1.0 / math.sqrt(d)
    r.q, r.k, r.v = q, k, v
    s = torch.einsum("bqnd,bknd->bnqk", q, k) * r.scale
    r.sabs = torch.einsum("bqnd,bknd->bnqk", q.abs(), k.abs()) * r.scale
    masked = (ids_q[:, None, :, None] == 0) | (ids_k[:, None, None, :] == 0)
    if causal:
        ar_q, ar_k = torch.arange(sq, device=q.device), torch.arange(sk, device=q.device)
        masked = masked | (ar_k[None, None, None, :] > ar_q[None, None, :, None])
    masked = masked.expand(b, n, sq, sk)
    r.masked = masked
    r.s = s.masked_fill(masked, MASK_VALUE)
    r.lse = torch.logsumexp(r.s, dim=-1)
    r.P = torch.exp(r.s - r.lse[..., None])
    r.Pd = r.P if drop_mask is None else r.P * drop_mask.double()
    r.O = torch.einsum("bnqk,bknd->bqnd", r.Pd, v)
    r.uniform = masked.all(dim=-1)                                       # [b, n, sq]: rows the reference makes uniform over all sk keys
    r.dO = None
    if dO is not None:
        dO = dO.double()
        r.dO = dO
        r.dV = torch.einsum("bnqk,bqnd->bknd", r.Pd, dO)
        dP = torch.einsum("bqnd,bknd->bnqk", dO, v)
        r.dPd = dP if drop_mask is None else dP * drop_mask.double()
        D = (r.P * r.dPd).sum(-1, keepdim=True)                          # == rowsum(dO o O)
        dS = (r.P * (r.dPd - D)).masked_fill(masked, 0.0)
        r.dQ = torch.einsum("bnqk,bknd->bqnd", dS, k) * r.scale
        r.dK = torch.einsum("bnqk,bqnd->bknd", dS, q) * r.scale
    return r


def reference_packed(qs, ks, vs, causal, dOs=None, ids_qs=None):
    """Packed form: lists of per-sequence tensors q [len_q, n, d], k / v [len_k, n, d] (every key is a real token; ids_qs gives the token
    ids of dense query rows, None = all real).  -> list of Ref (batch dimension 1)."""
    out = []
    for i in range(len(qs)):
        lq, lk = qs[i].shape[0], ks[i].shape[0]
        iq = torch.ones((1, lq), dtype=torch.int64, device=qs[i].device) if ids_qs is None else ids_qs[i][None]
        ik = torch.ones((1, lk), dtype=torch.int64, device=qs[i].device)
        out.append(reference(qs[i][None], ks[i][None], vs[i][None], iq, ik, causal, None, None if dOs is None else dOs[i][None]))
    return out


def _ulp(x, mant_bits):
    """One unit in the last place of |x| in a format with `mant_bits` explicit mantissa bits (7 = bf16, 23 = fp32); 0 at 0."""
    ax = x.abs()
    e = torch.floor(torch.log2(torch.where(ax > 0, ax, torch.ones_like(ax))))
    return torch.where(ax > 0, torch.exp2(e - mant_bits), torch.zeros_like(ax))


def _score_term(r, score_abs):
    return (r.sabs if score_abs else r.s.abs()).masked_fill(r.masked, 0.0)


def bounds(r, c=C_BF16, score_round=0.0, mant_bits=7, score_abs=False):
    """Majorant bounds of the module docstring for a Ref -> dict name -> tensor shaped like the reference value."""
    w = torch.full_like(r.P, c)
    if score_round:
        w = w + score_round * _score_term(r, score_abs)
    floor = lambda x: _ulp(x, mant_bits) + TINY
    wP, wPd = w * r.P + TINY, w * r.Pd + TINY
    B = {"O": torch.einsum("bnqk,bknd->bqnd", wP, r.v.abs()) + floor(r.O)}
    if r.dO is not None:
        adO = r.dO.abs()
        B["dV"] = torch.einsum("bnqk,bqnd->bknd", wPd, adO) + floor(r.dV)
        rowdot = torch.einsum("bqnd,bqnd->bnq", adO, r.O.abs())[..., None]
        G = (wP * (r.dPd.abs() + rowdot)).masked_fill(r.masked, 0.0)
        B["dQ"] = r.scale * torch.einsum("bnqk,bknd->bqnd", G, r.k.abs()) + floor(r.dQ)
        B["dK"] = r.scale * torch.einsum("bnqk,bqnd->bknd", G, r.q.abs()) + floor(r.dK)
    return B


def p_bound(r, c, score_round=0.0, score_abs=False):
    """Bound of the probabilities themselves (a path that keeps P): the exponent's own error plus the normaliser's, which is at most the
    row's largest."""
    t = _score_term(r, score_abs)
    return r.P * (c + 0.5 * score_round * (t + t.amax(dim=-1, keepdim=True))) + TINY


def lse_bound(r, score_round=0.0):
    smax = r.s.abs().masked_fill(r.masked, 0.0).amax(dim=-1)
    return 16.0 * 2.0 ** -24 * (1.0 + r.lse.abs() + smax) + score_round * smax


def worst(actual, ref, bound):
    """max(err / bound) and the index where it occurs; an error where the bound is 0 counts as infinite."""
    err = (actual.double() - ref).abs()
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
    flat = int(ratio.reshape(-1).argmax())
    idx = []
    for dim in reversed(ratio.shape):
        idx.append(flat % dim)
        flat //= dim
    return float(ratio.reshape(-1).max()), tuple(reversed(idx))


def worst_uniform(o, v, r, c=C_BF16):
    """Rows the reference makes uniform, directly against the mean of V over ALL sk keys (no reference P involved):
    max |o - mean_k V| / (c mean_k |V|) over those rows, 0 when there are none.  o [b, sq, n, d], v [b, sk, n, d]."""
    uni = r.uniform.permute(0, 2, 1)                                     # [b, sq, n]
    if not bool(uni.any()):
        return 0.0
    vm = v.double().mean(dim=1)[:, None].expand(-1, o.shape[1], -1, -1)
    bd = c * v.double().abs().mean(dim=1)[:, None].expand(-1, o.shape[1], -1, -1)
    return float(((o.double() - vm).abs() / bd)[uni].max())


def old_metric(actual, ref):
    """The global metric the row-scaled bounds replace: max |a - r| / max |r| over the whole tensor."""
    return float((actual.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-6))


# ---- input families ---------------------------------------------------------------------------------------------------------------
FAMILIES = ("stair_up", "stair_under", "stair_mixed", "one_hot", "flat", "randn")


def family(name, b, heads, sq, sk, hn, gen, device="cpu", pos_k=None):
    """q [b, sq, heads, hn], k, v [b, sk, heads, hn], dO [b, sq, heads, hn]: float32 tensors whose values are exact in bf16.
    Planted families: q_i = a_i e_0 + 0.25 randn, k_j = c_j e_0 + 0.25 randn (the noise lives in dimensions 1.., so the planted score is
    exactly a_i c_j / sqrt(hn)), |a_i| = sqrt(hn); v and dO are randn.  `pos_k` [b, sk] replaces the key position j in c_j (packed
    layouts: the position inside the key's own sequence)."""
    rn = lambda *s: torch.randn(s, generator=gen, device=device)
    v, dO = rn(b, sk, heads, hn), rn(b, sq, heads, hn)
    if name == "randn":
        q, k = rn(b, sq, heads, hn), rn(b, sk, heads, hn)
    else:
        q, k = 0.25 * rn(b, sq, heads, hn), 0.25 * rn(b, sk, heads, hn)
        amp = math.sqrt(hn)
        i = torch.arange(sq, device=device)
        j = torch.arange(sk, device=device)[None].expand(b, sk) if pos_k is None else pos_k.to(device)
        if name == "one_hot":                                              # row i: the key planted along e_(i % hn) leads by 40
            q[:, i, :, i % hn] = amp
            for r in range(min(hn, sk)):
                jr = (37 * r + 5) % sk
                k[:, jr] = 0.25 * rn(b, heads, hn)
                k[:, jr, :, r] = 40.0
        else:
            a = torch.full((sq,), amp, device=device)
            step = j // 32
            if name == "stair_up":
                cj = 6.0 * step                                            # the max moves by 6 log2(e) = 8.66 at every 32-key step
            elif name == "stair_under":
                cj = 5.0 * step                                            # 7.2 per step: under the lazy limit, moves every second step
            elif name == "stair_mixed":
                a = torch.where(i % 2 == 0, a, -a)                         # falling for half of a wave's lanes, rising for the other half
                cj = 6.0 * (step + 1)
            elif name == "flat":
                cj = torch.full_like(step, 3).float()
            else:
                raise ValueError(name)
            q[..., 0] = a[None, :, None]
            k[..., 0] = cj.float()[:, :, None]
    bf = lambda t: t.bfloat16().float()
    return bf(q), bf(k), bf(v), bf(dO)


MASK_PATTERNS = ("lead64", "lead32", "mid64", "mid32", "all_keys", "all_queries", "causal_key0", "last_key")


def mask_ids(pattern, b, sq, sk, device="cpu"):
    """Token ids [b, sq], [b, sk] (0 = padding).  Batch row 0 carries the pattern with every query real (so that no padded query switches
    the block skipping off); the other rows have ragged trailing padding and one padded query."""
    ids_q = torch.full((b, sq), 7, dtype=torch.int64, device=device)
    ids_k = torch.full((b, sk), 7, dtype=torch.int64, device=device)
    for i in range(1, b):
        ids_k[i, sk - 3 - 2 * i:] = 0
        ids_q[i, sq - i:] = 0
    if pattern == "trailing":
        ids_k[0, sk - 5:] = 0
    elif pattern == "none":
        ids_q[:], ids_k[:] = 7, 7
    elif pattern == "lead64":
        ids_k[0, :64] = 0
    elif pattern == "lead32":
        ids_k[0, :32] = 0
    elif pattern == "mid64":
        ids_k[0, 64:128] = 0
    elif pattern == "mid32":
        ids_k[0, 96:128] = 0
    elif pattern == "all_keys":
        ids_k[0, :] = 0
    elif pattern == "all_queries":
        ids_q[0, :] = 0
    elif pattern == "causal_key0":
        ids_k[0, 0] = 0
    elif pattern == "last_key":
        ids_k[0, :sk - 1] = 0
    else:
        raise ValueError(pattern)
    return ids_q, ids_k
