"""The attention reference harness has teeth (no GPU needed).

A small pure-torch model of the fused forward's walk over the keys -- 32 keys per step, 32 queries per "wave", a lazy running max kept as a
whole number of log2 units that moves only when a block max exceeds it by more than 8, P rounded to bf16 before P V, a bf16 output,
masked scores replaced by -10000, fully masked steps skipped once every query of the wave has seen a real key -- written from that
description, not from the kernel.  (a) The faithful model and an fp32 torch restatement stay inside the row-scaled bounds of
tests/attention_ref.py on every input family and mask pattern of tests/test_attention_edges_gpu.py; (b) six planted faults are each caught
by the bounds; (c) the padded-row faults and the half-rescale fault pass the old whole-tensor metric max|a - r| / max|r| < 2e-2 on
randn data.  (b) + (c): the row-scaled tests close a real gap.
"""
import math

import pytest
import torch

from tests import attention_ref as R

L2E = 1.4426950408889634
FAULTS = ("half_rescale", "no_l_rescale", "skip_unguarded", "zero_padded_rows", "uniform_real_only", "no_ceil")


def _bf(t):
    return t.bfloat16().float()


def emulate(q, k, v, ids_q, ids_k, causal, fault=None, skip=True):
    """q [b, sq, n, d], k / v [b, sk, n, d] fp32 (bf16 values) -> O [b, sq, n, d] (bf16 values), m, l [b, n, sq] (natural-log units)."""
    b, sq, n, d = q.shape
    sk = k.shape[1]
    sc = L2E / math.sqrt(d)
    O = torch.zeros(b, sq, n, d)
    M, L = torch.zeros(b, n, sq), torch.zeros(b, n, sq)
    for bi in range(b):
        kreal = ids_k[bi] != 0
        for w0 in range(0, sq, 32):
            w1 = min(w0 + 32, sq)
            qpad = ids_q[bi, w0:w1] == 0
            qi = torch.arange(w0, w1)
            for h in range(n):
                m = torch.full((w1 - w0,), -3.0e38)
                l = torch.zeros(w1 - w0)
                o = torch.zeros(w1 - w0, d)
                for s0 in range(0, sk, 32):
                    kr = kreal[s0:s0 + 32]
                    dead = (not bool(kr.any())) or (causal and s0 > w1 - 1)
                    seen = fault == "skip_unguarded" or bool((m > -7000.0).all())
                    if skip and dead and not bool(qpad.any()) and s0 > 0 and seen:
                        continue
                    masked = (~kr)[None, :] | qpad[:, None]
                    if causal:
                        masked = masked | (torch.arange(s0, s0 + 32)[None, :] > qi[:, None])
                    s2 = torch.where(masked, torch.tensor(-10000.0 * L2E), (q[bi, w0:w1, h] @ k[bi, s0:s0 + 32, h].T) * sc)
                    bmax = s2.max(dim=1).values
                    if bool((bmax > m + 8.0).any()):
                        mnew = torch.maximum(m, bmax)
                        if fault == "no_ceil":                       # a fractional reference point, the factor still taken between whole binades
                            alpha = torch.exp2(torch.ceil(m) - torch.ceil(mnew))
                        else:
                            mnew = torch.ceil(mnew)
                            alpha = torch.exp2(m - mnew)
                        if fault != "no_l_rescale":
                            l = l * alpha
                        if fault == "half_rescale":
                            o = torch.cat([o[:, :d // 2] * alpha[:, None], o[:, d // 2:]], dim=1)
                        else:
                            o = o * alpha[:, None]
                        m = mnew
                    p = torch.exp2(s2 - m[:, None])
                    l = l + p.sum(dim=1)
                    o = o + _bf(p) @ v[bi, s0:s0 + 32, h]
                out = _bf(o / l[:, None])
                allowed = kreal[None, :].expand(w1 - w0, sk)
                if causal:
                    allowed = allowed & (torch.arange(sk)[None, :] <= qi[:, None])
                uniform = qpad | ~allowed.any(dim=1)
                if fault == "zero_padded_rows":
                    out[qpad] = 0.0
                if fault == "uniform_real_only" and bool(kreal.any()):
                    out[uniform] = _bf(v[bi, kreal, h].mean(dim=0))
                O[bi, w0:w1, h] = out
                M[bi, h, w0:w1], L[bi, h, w0:w1] = m / L2E, l
    return O, M, L


def _torch_fp32(q, k, v, ids_q, ids_k, causal, dO):
    """fp32 autograd restatement of the reference semantics -> O, dQ, dK, dV."""
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bqnd,bknd->bnqk", q, k) / q.shape[-1] ** 0.5
    masked = (ids_q[:, None, :, None] == 0) | (ids_k[:, None, None, :] == 0)
    if causal:
        masked = masked | (torch.arange(k.shape[1])[None, None, None, :] > torch.arange(q.shape[1])[None, None, :, None])
    o = torch.einsum("bnqk,bknd->bqnd", torch.softmax(s.masked_fill(masked, -10000.0), dim=-1), v)
    o.backward(dO)
    return o.detach(), q.grad, k.grad, v.grad


def _cases():
    """(name, family, pattern, b, heads, sq, sk, causal): the dense, causal and mask-pattern cases of the GPU tests."""
    out = []
    for fam in R.FAMILIES:
        out.append((fam + "-dense", fam, "trailing", 2, 2, 64, 256, False))
        out.append((fam + "-causal96", fam, "trailing", 2, 1, 96, 96, True))
        out.append((fam + "-causal32", fam, "trailing", 2, 1, 32, 32, True))
    for fam in ("randn", "stair_up"):
        for pat in R.MASK_PATTERNS:
            causal = pat == "causal_key0"
            sq, sk = (96, 96) if causal else ((64, 192) if pat == "all_keys" else (64, 256))
            out.append(("%s-%s" % (fam, pat), fam, pat, 2, 1, sq, sk, causal))
    return out


CASES = _cases()
_CACHE = {}


def _case(case):
    """Inputs, float64 reference and bounds of a case, computed once and shared (never modified) by the tests below."""
    name, fam, pat, b, heads, sq, sk, causal = case
    if name not in _CACHE:
        gen = torch.Generator().manual_seed(1000 + CASES.index(case))
        q, k, v, dO = R.family(fam, b, heads, sq, sk, 64, gen)
        ids_q, ids_k = R.mask_ids(pat, b, sq, sk)
        ref = R.reference(q, k, v, ids_q, ids_k, causal, None, dO)
        _CACHE[name] = (q, k, v, dO, ids_q, ids_k, causal, ref, R.bounds(ref), R.lse_bound(ref))
    return _CACHE[name]


def _forward_ratio(case, fault=None, skip=True):
    q, k, v, dO, ids_q, ids_k, causal, ref, B, lb = _case(case)
    o, m, l = emulate(q, k, v, ids_q, ids_k, causal, fault, skip)
    return R.worst(o, ref.O, B["O"])[0], R.worst(m.double() + torch.log(l.double()), ref.lse, lb)[0], o, ref


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_faithful_emulation_and_fp32_torch_stay_inside_the_bounds(case):
    q, k, v, dO, ids_q, ids_k, causal, ref, B, lb = _case(case)
    for skip in (True, False):
        ro, rs, o, _ = _forward_ratio(case, None, skip)
        print("emulation skip=%d  O %.3f  lse %.3f" % (skip, ro, rs))
        assert ro < 1.0 and rs < 1.0, (case[0], skip, ro, rs)
    # rows the reference makes uniform: directly against the mean of V over ALL sk keys
    ru = R.worst_uniform(o, v, ref)
    print("uniform rows vs mean(V) %.3f" % ru)
    assert ru < 1.0, (case[0], ru)
    got = _torch_fp32(q, k, v, ids_q, ids_k, causal, dO)
    for name, a in zip(("O", "dQ", "dK", "dV"), got):
        r, idx = R.worst(a, getattr(ref, name), B[name])
        print("fp32 torch %s %.4f at %s" % (name, r, idx))
        assert r < 1.0, (case[0], name, r, idx)


@pytest.mark.parametrize("fault", FAULTS)
def test_every_planted_fault_is_caught_by_the_row_scaled_bound(fault):
    caught = []
    for case in CASES:
        ro, rs, _, _ = _forward_ratio(case, fault)
        if ro >= 1.0:                                                      # the row-scaled O bound itself, not only the statistics
            caught.append((case[0], round(ro, 2), round(rs, 2)))
    print(fault, "caught on", caught)
    assert caught, "the planted fault %s passes every family" % fault


def _old_metric_case():
    """randn data with the masks the existing tests draw -- trailing padding, padded queries, one batch row that keeps only a few keys
    (test_seqpack_gpu.py: ids_d[2, 37:] = 0) -- at sq = 64, sk = 8192: a uniform row has size ~ 1 / sqrt(sk) next to rows of size ~ 1.
    (How blind the whole-tensor metric is to a padded row depends on max|r| / |row| ~ sqrt(sk): a row that is 100 % wrong reads 0.011
    here, about 0.02 -- the metric's own limit -- at 2,048 to 4,096 keys with masks of this kind, and is seen below that.  The fault that
    averages over the real keys only passes it at every size.)"""
    gen = torch.Generator().manual_seed(77)
    b, heads, sq, sk = 3, 1, 64, 8192
    q, k, v, dO = R.family("randn", b, heads, sq, sk, 64, gen)
    ids_q = torch.full((b, sq), 7, dtype=torch.int64)
    ids_k = torch.full((b, sk), 7, dtype=torch.int64)
    ids_k[0, sk - 3:] = 0
    ids_q[0, sq - 1:] = 0
    ids_k[1, sk - 2048:] = 0
    ids_q[1, sq - 2:] = 0
    ids_k[2, 3:] = 0
    ref = R.reference(q, k, v, ids_q, ids_k, False)
    return q, k, v, ids_q, ids_k, ref, R.bounds(ref)


@pytest.mark.parametrize("fault", ["zero_padded_rows", "uniform_real_only", "half_rescale"])
def test_the_old_whole_tensor_metric_misses_the_fault_on_randn_data(fault):
    q, k, v, ids_q, ids_k, ref, B = _old_metric_case()
    o, _, _ = emulate(q, k, v, ids_q, ids_k, False, fault)
    old = R.old_metric(o, ref.O)
    new = R.worst(o, ref.O, B["O"])[0]
    print("%s: old metric %.4f (limit 2e-2), row-scaled ratio %.2f" % (fault, old, new))
    assert old < 2e-2, (fault, old)                                       # the existing assertion would pass this faulty output
    if fault != "half_rescale":                                           # (on randn data the max never moves twice: that fault changes no bit)
        assert new >= 1.0, (fault, new)
    else:
        o_ok, _, _ = emulate(q, k, v, ids_q, ids_k, False, None)
        assert torch.equal(o, o_ok)
