"""LayerNorm, log-softmax + gather, the LSE combine and the fused LM head, the retriever prior, the marginal and the GELU derivative
against float64 references with PER-ELEMENT structural bounds (tests/elementwise_ref.py; tests/test_elementwise_ref_cpu.py shows what
those bounds catch that max|a - r| / max|r| < 2e-2 lets through, and that the fp32 torch implementation of each op stays within them).
Every case goes through the product entry points of emdr2_amd/model/kernels.py, or through the C ABI where no wrapper exists
(emdr2_layernorm_bwd_mask, emdr2_lse_combine with an lse output, emdr2_gelu_bwd).  Pass criterion: worst err / bound <= 1 for every
quantity of every case; nothing is excluded.

Worst err / bound per kernel, family and quantity, measured on an MI355X.  "before": the kernels as they stood before this file
existed; "after": with the fixes listed below (one column where nothing changed).  LayerNorm rows take the worst over H, row counts,
dy families and both entry points (layer_norm, layer_norm_residual); "768" is the half-wave-per-row fast path incl. 16,393 rows,
"generic" the one-wave-per-row kernels at H = 8, 264, 1024 and (through a gain 4 bytes off alignment) at H = 768.

    LayerNorm      family          y                rstd               dx                 dgamma           mean   dbeta
                                   before   after   before     after   before     after   before   after
    768            randn           0.25     0.25    0.04       0.04    0.25       0.25    0.04     0.04    0.01   0.00
    768            offset8         0.25     0.25    2.04       0.07    0.25       0.25    0.77     0.12    0.02   0.00
    768            offset64        0.27     0.25    125        0.06    0.30       0.25    9.58     0.15    0.02   0.00
    768            offset200       0.42     0.25    748        0.07    0.77       0.25    35.8     0.11    0.01   0.00
    768            const 0/1/256   0.25     0.25    0.01       0.01    0.42       0.42    0.00     0.00    0.00   0.00
    768            outlier8        19.5     0.25    5.8e4      0.00    19.8       0.25    3.5e3    0.17    0.02   0.00
    768            outlier64       405      0.25    1.2e6      0.04    8.9e3      0.25    7.3e4    0.17    0.02   0.00
    768            outlier256      1.8e3    0.25    5.6e6      0.04    5.7e5      0.25    3.4e5    0.17    0.02   0.00
    768            alternating     0.25     0.25    0.01       0.01    0.25       0.25    0.29     0.29    0.00   0.00
    768            tiny            0.25     0.25    0.02       0.02    0.25       0.25    0.04     0.04    0.00   0.00
    generic        randn           0.25     0.25    0.03       0.03    0.25       0.25    0.05     0.05    0.00   0.00
    generic        offset8         0.25     0.25    1.49       0.03    0.25       0.25    0.93     0.10    0.01   0.00
    generic        offset64        0.26     0.25    93.9       0.03    0.28       0.25    11.5     0.11    0.01   0.00
    generic        offset200       0.37     0.25    595        0.02    0.73       0.25    28.0     0.08    0.01   0.00
    generic        const 0/1/256   0.25     0.25    0.01       0.01    0.25       0.25    0.00     0.00    0.00   0.00
    generic        outlier8        14.6     0.25    4.5e4      0.02    15.2       0.25    2.7e3    0.08    0.01   0.00
    generic        outlier64       333      0.25    1.0e6      0.02    4.3e3      0.25    6.2e4    0.08    0.01   0.00
    generic        outlier256      1.6e3    0.25    4.9e6      0.01    2.8e5      0.25    2.9e5    0.08    0.01   0.00
    generic        alternating     0.25     0.25    0.01       0.01    0.25       0.25    0.03     0.03    0.00   0.00
    generic        tiny            0.25     0.25    0.02       0.02    0.25       0.25    0.07     0.07    0.00   0.00
    bwd + mask / bwd (C ABI, offset8, 9 and 16,393 rows)               0.25       0.25    0.46     0.08           0.00

    log-softmax + gather    lse    gold before   gold after   dlogits bf16   dlogits fp32     ("before" exceeds 1 on the two rows
    randn                   0.02   9.0e4         0.02         0.25           0.03             labelled -100 and V + 7 only: the kernel
    shift_up   (+80)        0.01   2.4e5         0.01         0.23           0.01             read a neighbouring row's logit; bf16
    shift_down (-80)        0.01   2.6e5         0.01         0.23           0.01             and fp32 operands gave the same figures)
    dominant   (+60)        0.00   1.1e4         0.00         0.24           0.01
    equal                   0.01   8.0e4         0.01         0.22           0.01
    staircase  (span 200)   0.01   2.5e5         0.01         0.57           0.01

    lse_combine   slots     1             3             64            65            480
                  lse/out   0.00 / 0.01   0.01 / 0.02   0.01 / 0.02   0.02 / 0.01   0.02 / 0.02
    LM head       bias      +-50 blocks: fused 0.01, unfused 0.01          +-30 alternating: fused 0.02, unfused 0.02

    retriever prior         logp   prob   dq     dc         (worst over (B, K, H); K = 1: all exactly 0)
    randn, 1 / sqrt(H)      0.01   0.01   0.24   0.25
    wide (+-300)            0.01   0.27   0.22   0.25
    ties                    0.01   0.27   0.22   0.25
    leader                  0.01   0.00   0.20   0.25

    marginal      (B, K, L)   (2, 1, 1)            (3, 51, 65)          (2, 101, 32)
      value/dprior/identity   0.00 / 0.00 / 0.00   0.03 / 0.02 / 0.00   0.01 / 0.02 / 0.00
    GELU derivative   n       8: 0.00              264: 0.22            65,544: 0.25

The 0.25 of every bf16 column is the store itself (half a bf16 ulp against c = 2^-7 plus one ulp); dx 0.42 on constant rows: rstd is
1 / sqrt(eps) = 316 there and the three terms of dx cancel.

What these tests found and what changed with them:
  * LayerNorm forward, both bf16 kernels: var = E[x^2] - mean^2 in fp32.  On the GPU as in the emulation of the issue: rstd 2 bounds off at
    mean / std = 8, 750 at 200, 6e6 on a row of 256 with one element one bf16 ulp up; y, dx and dgamma follow (table).  Both kernels now
    take a centred second pass (the 768 kernel over its registers, the generic one over the row it re-reads anyway, even and odd
    elements in two accumulation chains).
  * The centred pass of the 768 kernel first missed rstd by 1.2 bounds on the same near-constant rows, at outlier columns >= 512 only:
    with contraction on, the compiler had folded mean = s * (1 / 768) into the subtraction of 18 of a lane's 24 elements (an fma on the
    UNROUNDED product) and subtracted the rounded mean from the other 6, so the first-order cancellation of the mean's rounding error in
    sum (x - mean)^2 was gone.  The mean is now one rounded product for all elements (mul_rounded in prims.h): 0.04.
  * lse_gather forward (loss_tail.hip and fp32_ops.hip) read logits[row, label] unguarded: a label of -100 or >= V read a
    neighbouring row (or outside the tensor on the first / last row).  Guarded: gold = -lse, as the fused LM head defines it.  The
    backward never matched such a label and was right: dlogits = -w softmax.
  * Nothing else: the persistent 768 backward on its second lap, its odd tails, the mask variant (dmask bit-equal to emdr2_dropout(dx),
    dx bit-equal to the kernel without the mask), the combine, the fused LSE epilogue far from 0, the prior at +-300, K = 1 and
    K = 1024, the marginal down to -800 and the GELU derivative all stay within their bounds.
"""
import pytest
import torch

from tests import elementwise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _nat():
    from emdr2_amd import _native
    return _native, _native.lib()


def _assert(tag, ratios):
    print("[ew-edges] %s " % tag + " ".join("%s=%.3f" % (n, r[0]) for n, r in ratios.items()))
    bad = {n: r for n, r in ratios.items() if not r[0] <= 1.0}
    assert not bad, (tag, bad)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
def _ln_run(x, gamma, beta, dy, dres, misaligned):
    """Through K.layer_norm (dres None) or K.layer_norm_residual -> dict y, mean, rstd, dx, dgamma, dbeta."""
    from emdr2_amd.model import kernels as K
    H = x.shape[-1]
    if misaligned:                                                       # a gain 4 bytes off a 16-byte boundary: the generic kernels, whatever H
        buf = torch.zeros(H + 1, device=DEV)
        buf[1:] = gamma
        g = buf[1:].detach().requires_grad_(True)
        assert g.data_ptr() % 16 == 4
    else:
        g = gamma.clone().requires_grad_(True)
    b = beta.clone().requires_grad_(True)
    xb = x.bfloat16().requires_grad_(True)
    if dres is None:
        y = K.layer_norm(xb, g, b, EPS)
        saved = y.grad_fn.saved_tensors
        y.backward(dy.bfloat16())
    else:
        y, xpass = K.layer_norm_residual(xb, g, b, EPS)
        saved = y.grad_fn.saved_tensors
        torch.autograd.backward([y, xpass], [dy.bfloat16(), dres.bfloat16()])
    torch.cuda.synchronize()
    return {"y": y.detach(), "mean": saved[1], "rstd": saved[2], "dx": xb.grad, "dgamma": g.grad, "dbeta": b.grad}


def _ln_case(fam, dyfam, rows, H, misaligned=False):
    x, gamma, beta, dy, dres = R.ln_inputs(fam, dyfam, rows, H, _gen(rows * 7 + H), DEV)
    tag = "ln %s dy=%s rows=%d H=%d%s" % (fam, dyfam, rows, H, " generic" if misaligned else "")
    ref = R.ln_reference(x, gamma, beta, EPS, dy, None)
    ratios = R.worst_all(_ln_run(x, gamma, beta, dy, None, misaligned), ref, R.ln_bounds(ref))
    ref = R.ln_reference(x, gamma, beta, EPS, dy, dres)                  # K.layer_norm_residual: dres rides into dx
    resid = R.worst_all(_ln_run(x, gamma, beta, dy, dres, misaligned), ref, R.ln_bounds(ref))
    ratios.update({"res_" + n: v for n, v in resid.items()})
    _assert(tag, ratios)


# The one-hot and constant dy families run at 3, 33 and 16,393 rows (an odd count below one block, two blocks of the generic backward,
# the second lap of the 768 one); 1, 2 and 9 rows see randn dy only, to keep the suite short.  gamma has zeros and negative entries, so
# a constant dy does not make dx itself vanish: "dx ~ 0 on the scale of its terms" is what the term bound of dx asserts.
def _ln_dy_families(rows):
    return R.LN_DY_FAMILIES if rows in (3, 33) else ("randn",)


LN_CASES = [(fam, dyfam, rows, H) for H in (8, 264, 768, 1024) for rows in (1, 2, 3, 9, 33) for fam in R.LN_X_FAMILIES
            for dyfam in _ln_dy_families(rows)]


@pytest.mark.parametrize("fam,dyfam,rows,H", LN_CASES)
def test_layernorm(fam, dyfam, rows, H):
    _ln_case(fam, dyfam, rows, H)


@pytest.mark.parametrize("fam,dyfam,rows", [(fam, dyfam, rows) for rows in (3, 33) for fam in R.LN_X_FAMILIES for dyfam in _ln_dy_families(rows)])
def test_layernorm_generic_kernels_at_768(fam, dyfam, rows):
    _ln_case(fam, dyfam, rows, 768, misaligned=True)


@pytest.mark.parametrize("dyfam", R.LN_DY_FAMILIES)
@pytest.mark.parametrize("fam", R.LN_X_FAMILIES)
def test_layernorm_second_lap_and_odd_tails(fam, dyfam):
    """16,393 = 2,048 * 8 + 9 rows at H = 768: the persistent backward's second lap, an odd tail, and a tail on lap two."""
    _ln_case(fam, dyfam, 16393, 768)


def _ln_bwd_abi(x, gamma, dy, dres, mean, rstd, mask=None):
    nat, lib = _nat()
    rows, H = x.shape
    dx, dg, db = torch.empty_like(x), torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    if mask is None:
        rc = lib.emdr2_layernorm_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dres.data_ptr(), dx.data_ptr(),
                                     dg.data_ptr(), db.data_ptr(), rows, H, nat.stream_ptr())
        dm = None
    else:
        dm = torch.empty_like(x)
        rc = lib.emdr2_layernorm_bwd_mask(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dres.data_ptr(), dx.data_ptr(),
                                          dg.data_ptr(), db.data_ptr(), rows, H, dm.data_ptr(), mask[0], mask[1], nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, dx, dg, db, dm


@pytest.mark.parametrize("seed", [0x51, 0xBEEF01])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows", [9, 16393])
def test_layernorm_backward_with_dropout_mask(rows, p, seed):
    """emdr2_layernorm_bwd_mask: dmask bit-equal to emdr2_dropout(dx); dx bit-equal to and dgamma / dbeta within the bounds like the
    kernel without the mask (their atomics arrive in any order)."""
    from emdr2_amd.model import kernels as K
    nat, lib = _nat()
    x, gamma, beta, dy, dres = R.ln_inputs("offset8", "randn", rows, 768, _gen(rows + 1), DEV)
    xb, dyb, drb = x.bfloat16(), dy.bfloat16(), dres.bfloat16()
    _, mean, rstd = K._ln_forward(xb, gamma, beta, EPS)
    rc0, dx0, dg0, db0, _ = _ln_bwd_abi(xb, gamma, dyb, drb, mean, rstd)
    rc1, dx1, dg1, db1, dm = _ln_bwd_abi(xb, gamma, dyb, drb, mean, rstd, (p, seed))
    assert rc0 == 0 and rc1 == 0
    assert torch.equal(dx0.view(torch.int16), dx1.view(torch.int16))
    want = torch.empty_like(dx1)
    nat.check(lib.emdr2_dropout(dx1.data_ptr(), want.data_ptr(), dx1.numel(), 768, p, seed, nat.stream_ptr()), "dropout")
    torch.cuda.synchronize()
    assert torch.equal(dm.view(torch.int16), want.view(torch.int16))
    kept = float((dm != 0).float().mean()) / max(float((dx1 != 0).float().mean()), 1e-9)
    assert abs(kept - (1.0 - p)) < (0.05 if rows == 9 else 0.002), kept
    ref = R.ln_reference(x, gamma, beta, EPS, dy, dres)
    B = R.ln_bounds(ref)
    _assert("ln bwd+mask rows=%d p=%g" % (rows, p), R.worst_all({"dx": dx1, "dgamma": dg1, "dbeta": db1}, ref, {n: B[n] for n in ("dx", "dgamma", "dbeta")}))
    _assert("ln bwd rows=%d" % rows, R.worst_all({"dx": dx0, "dgamma": dg0, "dbeta": db0}, ref, {n: B[n] for n in ("dx", "dgamma", "dbeta")}))


def test_layernorm_backward_with_dropout_mask_is_for_768_only():
    from emdr2_amd.model import kernels as K
    x, gamma, beta, dy, dres = R.ln_inputs("randn", "randn", 9, 264, _gen(3), DEV)
    xb = x.bfloat16()
    _, mean, rstd = K._ln_forward(xb, gamma, beta, EPS)
    rc, _, dg, _, _ = _ln_bwd_abi(xb, gamma, dy.bfloat16(), dres.bfloat16(), mean, rstd, (0.1, 7))
    assert rc == -4 and float(dg.abs().max()) == 0.0                      # refused before anything ran


# ---- log-softmax + gather -------------------------------------------------------------------------------------------------------------
LSE_CASES = [(fam, V, rows, False) for fam in R.LSE_FAMILIES for V in (1, 7, 255, 257, 1000) for rows in (1, 5)] + \
            [(fam, V, 5, True) for fam in R.LSE_FAMILIES for V in (255, 257, 1000)]


@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("fam,V,rows,out_of_range", LSE_CASES)
def test_lse_gather(fam, V, rows, out_of_range, fp32):
    """bf16 operands (loss_tail.hip) and fp32 operands (fp32_ops.hip).  In-range labels: 0, V - 1, 255, 256 and a dominant column past
    255 (R.lse_inputs).  out_of_range: -100 and V + 7 on interior rows only, so that a read without the guard stays inside the logits and
    the case fails by value: gold = -lse, dlogits = -w softmax with a non-zero w on both rows."""
    from emdr2_amd.model import kernels as K
    x, labels, w = R.lse_inputs(fam, rows, V, _gen(V + rows), DEV, out_of_range)
    xx = (x if fp32 else x.bfloat16()).clone().requires_grad_(True)
    gold = K.lse_gather(xx, labels)
    lse = gold.grad_fn.saved_tensors[2]
    gold.backward(w)
    torch.cuda.synchronize()
    ref = R.lse_reference(x, labels, w)
    B = R.lse_bounds(ref, R.C_F32 if fp32 else R.C_BF16, 23 if fp32 else 7)
    _assert("lse_gather %s %s V=%d rows=%d out=%d" % ("fp32" if fp32 else "bf16", fam, V, rows, out_of_range),
            R.worst_all({"lse": lse, "gold": gold.detach(), "dlogits": xx.grad}, ref, B))


@pytest.mark.parametrize("slots", [1, 3, 64, 65, 480])
def test_lse_combine(slots):
    nat, lib = _nat()
    rows = 9
    pmax, psum, gold = R.combine_inputs(rows, slots, _gen(slots), DEV)
    out, lse = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    nat.check(lib.emdr2_lse_combine(pmax.data_ptr(), psum.data_ptr(), gold.data_ptr(), out.data_ptr(), lse.data_ptr(), rows, slots, nat.stream_ptr()), "combine")
    out2 = torch.empty(rows, device=DEV)
    nat.check(lib.emdr2_lse_combine(pmax.data_ptr(), psum.data_ptr(), gold.data_ptr(), out2.data_ptr(), None, rows, slots, nat.stream_ptr()), "combine")
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    ref = R.combine_reference(pmax, psum, gold)
    _assert("lse_combine slots=%d" % slots, R.worst_all({"lse": lse, "out": out}, ref, R.combine_bounds(ref)))


@pytest.mark.parametrize("bias_kind", ["blocks", "alternating"])
def test_lm_head_fused_with_structured_bias(bias_kind):
    """The fused LSE epilogue of the LM head at its smallest shape with logits far from 0: one 64-column block at +50 and one at -50, or
    +-30 alternating inside a block (a wrong per-block maximum would pass on N(0, 0.5) logits).  Against the float64 reference of the
    bf16-rounded logits, and against the unfused pair as test_gemm8_gpu does."""
    from emdr2_amd.model import kernels as K
    M, V, H = 256, 512, 128
    g = _gen(77)
    hid = (torch.randn((M, H), generator=g, device=DEV)).bfloat16()
    W = torch.nn.Parameter(torch.randn((V, H), generator=g, device=DEV) * 0.05)
    bias = torch.randn(V, generator=g, device=DEV) * 0.1
    if bias_kind == "blocks":
        bias[128:192] += 50.0
        bias[320:384] -= 50.0
    else:
        bias[128:192] += 30.0 * (1.0 - 2.0 * (torch.arange(64, device=DEV) % 2).float())
    bias = torch.nn.Parameter(bias)
    labels = torch.randint(0, V, (M,), generator=g, device=DEV)
    labels[0::4] = 128 + (torch.arange(M // 4, device=DEV) % 64)          # the high (or alternating) block
    labels[1::4] = 320 + (torch.arange(M // 4, device=DEV) % 64)          # the low block
    labels[2::4] = 448 + (torch.arange(M // 4, device=DEV) % 64)          # a neutral one
    with torch.no_grad():
        fused = K.lm_head_gold_logprob(hid, W, bias, labels)
        logits = K.linear(hid, W, bias)
        unfused = K.lse_gather(logits, labels)
    torch.cuda.synchronize()
    ref = R.lse_reference(logits.float(), labels)
    B = R.lse_bounds(ref)
    _assert("lm_head %s" % bias_kind, {"fused": R.worst(fused, ref.gold, B["gold"]), "unfused": R.worst(unfused, ref.gold, B["gold"])})
    assert torch.allclose(fused, unfused, rtol=0, atol=2e-4), float((fused - unfused).abs().max())


# ---- retriever prior ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 8), (3, 7, 264), (2, 1024, 64), (2, 101, 768)])
@pytest.mark.parametrize("fam", R.PRIOR_FAMILIES)
def test_retriever_prior(fam, shape):
    from emdr2_amd.model import kernels as K
    Bq, Kk, H = shape
    q, c, scale, g = R.prior_inputs(fam, Bq, Kk, H, _gen(Kk + H), DEV)
    qq, cc = q.bfloat16().requires_grad_(True), c.bfloat16().requires_grad_(True)
    logp = K.retriever_prior(qq, cc, scale)
    prob = logp.grad_fn.saved_tensors[2]
    logp.backward(g)
    torch.cuda.synchronize()
    ref = R.prior_reference(q, c, scale, g)
    if fam == "leader" and Kk > 1:
        assert float(ref.prob.sort(-1).values[:, -2].max()) < 1e-45       # every other probability underflows fp32
    _assert("prior %s %s" % (fam, shape), R.worst_all({"logp": logp.detach(), "prob": prob, "dq": qq.grad, "dc": cc.grad}, ref, R.prior_bounds(ref)))
    if Kk == 1:                                                           # one passage: log-probability 0 and no gradient, exactly
        assert float(logp.detach().abs().max()) == 0.0 and float(qq.grad.abs().max()) == 0.0 and float(cc.grad.abs().max()) == 0.0


def test_retriever_prior_refuses_more_than_1024_passages():
    from emdr2_amd import _native
    from emdr2_amd.model import kernels as K
    q, c = torch.zeros((2, 64), device=DEV).bfloat16(), torch.zeros((2, 1025, 64), device=DEV).bfloat16()
    with pytest.raises(_native.NativeError, match="-4"):
        K.retriever_prior(q, c, 1.0)


# ---- EMDR2 marginal -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 1), (3, 51, 65), (2, 101, 32)])
def test_marginal_logsumexp(shape):
    from emdr2_amd.model import kernels as K
    prior, gold, gm = R.marginal_inputs(*shape, gen=_gen(shape[1]), device=DEV)
    p = prior.clone().requires_grad_(True)
    out = K.marginal_logsumexp(p, gold)
    out.backward(gm)
    torch.cuda.synchronize()
    ref = R.marginal_reference(prior, gold, gm)
    B = R.marginal_bounds(ref)
    ratios = R.worst_all({"marginal": out.detach(), "dprior": p.grad}, ref, {"marginal": B["marginal"], "dprior": B["dprior"]})
    ratios["identity"] = R.worst(p.grad.double().sum(-1), gm.double().sum(-1), B["identity"])
    _assert("marginal %s" % (shape,), ratios)


# ---- GELU derivative ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 264, 65544])
def test_gelu_bwd(n):
    nat, lib = _nat()
    x, dact = R.gelu_inputs(n, _gen(n), DEV)
    xb, db = x.bfloat16(), dact.bfloat16()
    out = torch.empty_like(xb)
    nat.check(lib.emdr2_gelu_bwd(xb.data_ptr(), db.data_ptr(), out.data_ptr(), n, nat.stream_ptr()), "gelu_bwd")
    torch.cuda.synchronize()
    ref = R.gelu_bwd_reference(x, dact)
    _assert("gelu_bwd n=%d" % n, R.worst_all({"dpre": out}, ref, R.gelu_bwd_bounds(ref)))
