"""Float64 references, per-element structural bounds and input families for the row and elementwise kernels that are not attention (csrc/layernorm.hip,
loss_tail.hip, elementwise.hip, optimizer.hip): LayerNorm, log-softmax + gather, the LSE combine, the retriever prior, the EMDR2 marginal, the
GELU derivative, AdamW (CPU and GPU tensors alike).  The pattern is that of tests/attention_ref.py, whose constants are imported, not restated.

Bounds.  An error is judged against the sum of the MAGNITUDES of the terms that make the value (never |value|, which can cancel, and never
a whole-tensor maximum), times

    C_BF16 = 2^-7    for an output stored in bf16 (the store, one or two bf16-sized steps before it, fp32 arithmetic),
    C_F32  = 2^-18   for an fp32 output (64 unit roundoffs: a reduction of a few hundred to a few thousand terms and its transcendentals),

plus one ulp of the reference value in the output's format, plus the underflow floor TINY = 2^-126 of attention_ref.py.  Terms added to
the lists of the issue, each a rounding step those lists leave out, with the reasoning:

  * centring (LayerNorm): the mean is an fp32 number.  Whatever computes xhat = (x - mean) rstd from an fp32 mean -- the forward kernel,
    the backward kernel from the SAVED mean, torch -- carries |d xhat| <= C_CENTRE rstd (|x| + |mean|), C_CENTRE = 2^-22 (four unit
    roundoffs: the sum, the division, the subtraction, the product).  On a row of 256 with one element at 258 (H = 768) x - mean is
    -0.0026 for 767 elements and half an ulp of the mean is 1.5e-5 of it: 0.6 % of xhat, the size of C_BF16 itself, and 1,500 times
    C_F32 for the fp32 column sums dgamma.  Every quantity that contains xhat carries this term.  It does NOT excuse a wrong variance:
    the variance moves by the SQUARE of the mean's error, so rstd is held to C_F32 alone.
    Evidence: with C_CENTRE = 0 the fp32 torch reference itself scores y 4.15 (offset200), dx 1.09 (outlier256) and dgamma 2,256
    (outlier8, H = 768) against the remaining terms; with the term, 0.25 / 0.25 / 0.30.  Widening C_F32 for dgamma to twice 2,256 as
    a plain constant would loosen every family 4,500 times; the term loosens only rows whose mean dwarfs their spread.
  * exponent (everything with exp(a - b)): fp32 rounds the argument, |d arg| <= 4 2^-24 (|a| + |b|), which is a RELATIVE error of the
    exponential; with priors at -600 and gold at -200 that is 2e-4, fifty times C_F32.  The error of a logsumexp that enters an exponent
    is added likewise (its bound, not a constant).
  * logsumexp: m + log(sum) -- an error of the sum RELATIVE to it is an ABSOLUTE error of its logarithm, hence the 1 in
    C_F32 (1 + |m| + |lse - m|).
  * GELU derivative: Phi(x) + x phi(x) evaluated in fp32 as the kernel states it (0.5 (1 + erff(x / sqrt 2)) + x 0.39894 expf(-x^2 / 2))
    has an ABSOLUTE error near one fp32 roundoff of 1 where Phi itself is 1e-30 (x = -12): GELU_ABS, measured below.

Constants taken from the fp32 torch implementation of the same op on the CPU (tests/test_elementwise_ref_cpu.py asserts them: worst
err / bound of torch.nn.functional.layer_norm, torch.log_softmax, torch.logsumexp, torch.optim.AdamW in float32, rounded to bf16 where the
kernel stores bf16, over every family below; a bound whose reference ratio exceeds 0.5 is widened to twice that ratio):

    quantity                        worst ratio of the fp32 torch reference      constant
    LayerNorm y / dx (bf16)         0.25 / 0.25                                  C_BF16 (+ centring)
    LayerNorm mean / rstd           0.02 / 0.03                                  C_F32
    LayerNorm dgamma / dbeta        0.30 / 0.01                                  C_F32 (+ centring)
    lse / gold / dlogits            0.02 / 0.02 / 0.25                           C_F32 / C_F32 / C_BF16 (fp32 dlogits: 0.25 of C_F32's)
    combine lse / out               0.01 / 0.02                                  C_F32
    prior logp / prob / dq / dc     0.02 / 0.01 / 0.24 / 0.25                    C_F32 / C_F32 / C_BF16 / C_BF16
    marginal / dprior / identity    0.02 / 0.03 / 0.01                           C_F32
    GELU derivative                 max |fp32 formula - float64| = 9.73e-8       GELU_ABS = 2.0e-7 (twice the measured value, rounded up)
    AdamW m / v                     0.04 / 0.06                                  C_F32
    AdamW master                    1.19 ulp of the master (torch rounds it      ADAM_ULPS = 2.4 ulp (twice the measured value) next to
                                    twice: mul_ by 1 - lr wd, then addcdiv_)     C_F32 lr (|adam term| + wd |w|)
    sum of squares                  0.01                                         C_F32
"""
import math

import numpy as np
import torch

from tests.attention_ref import C_BF16, C_F32, TINY, _ulp, old_metric, worst  # noqa: F401  (re-exported for the tests)

U32 = 2.0 ** -24
C_CENTRE = 4.0 * U32                     # without it the fp32 torch reference scores y 4.15, dx 1.09, dgamma 2,256 (module docstring)
C_EXPARG = 4.0 * U32                     # the fp32 torch reference stays below 0.5 without it (accurate expf; the lse bound in the same weight dominates)
GELU_ABS = 2.0e-7                        # measured 9.73e-8 (test_elementwise_ref_cpu.test_gelu_formula_error), doubled
ADAM_ULPS = 2.4                          # measured 1.19 ulp for torch.optim.AdamW in float32 (weight decay 0.1, step 3), doubled


class Ref(object):
    pass


def bf(t):
    """Round to bf16 and back: fp32 values that a bf16 kernel reads exactly."""
    return t.float().bfloat16().float()


def _floor(ref, mant_bits):
    return _ulp(ref, mant_bits) + TINY


def worst_all(got, ref, bounds):
    """{name: (ratio, index)} for every name of `bounds`."""
    return {n: worst(got[n], getattr(ref, n), bounds[n]) for n in bounds}


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
def ln_reference(x, gamma, beta, eps, dy=None, dres=None):
    """x [rows, H], gamma / beta [H], dy / dres [rows, H] or None -> Ref y, mean, rstd, xhat (+ dx, dgamma, dbeta), all float64."""
    r = Ref()
    r.x, r.gamma, r.beta = x.double(), gamma.double(), beta.double()
    r.mean = r.x.mean(-1)
    xc = r.x - r.mean[:, None]
    r.rstd = ((xc * xc).mean(-1) + eps) ** -0.5
    r.xhat = xc * r.rstd[:, None]
    r.y = r.xhat * r.gamma + r.beta
    r.dy = None
    if dy is not None:
        r.dy = dy.double()
        r.dres = None if dres is None else dres.double()
        r.g = r.dy * r.gamma
        r.m1 = r.g.mean(-1, keepdim=True)
        r.m2 = (r.g * r.xhat).mean(-1, keepdim=True)
        r.dx = r.rstd[:, None] * (r.g - r.m1 - r.xhat * r.m2)
        if dres is not None:
            r.dx = r.dx + r.dres
        r.dgamma = (r.dy * r.xhat).sum(0)
        r.dbeta = r.dy.sum(0)
    return r


def ln_bounds(r, c=C_BF16, mant_bits=7, mean_terms=False, recursive_rows=0):
    """y, mean, rstd (+ dx, dgamma, dbeta).  c / mant_bits describe the format y and dx are stored in.
    mean_terms: weigh the two row means of dx = rstd (g - m1 - xhat m2) by the magnitudes of THEIR terms, mean |g| and mean |g xhat|,
    instead of by their values |m1|, |m2|.  The values cancel (m1 = mean_j g_j), while whatever sums H fp32 terms errs by about
    u mean |g|: with c = C_BF16 that is far below one store and nobody sees it, with c = C_F32 one row in a few hundred has |m1| below
    mean |g| / 600 and the bound by value collapses under ANY fp32 sum (tests/test_elementwise_ref_cpu.py: on const0 at
    1,031 x 768 the fp32 formula scores 167 and fp32 torch 42).  The fp32 tests pass True; the bf16 tests keep the bound as it was.
    recursive_rows: dgamma is summed over that many rows RECURSIVELY in fp32 (one atomic per row, csrc/fp32_ops.hip), so its relative
    constant is max(C_F32, (rows + 2) U32), the (n + 2) u bound of a recursive sum (tests/embedding_ref.py).  C_F32 = 64 U32 assumes a
    tree: on 1,031 `alternating` rows with a constant dy the terms of a column are all alike, every add rounds the same way, and the
    recursive sum is 90 u off -- 1.41 of C_F32's bound on the MI355X, and likewise in a row-by-row fp32 loop on the CPU."""
    rs = r.rstd[:, None]
    exh = C_CENTRE * rs * (r.x.abs() + r.mean.abs()[:, None])            # what an fp32 mean leaves uncertain in xhat
    B = {"y": c * ((r.xhat * r.gamma).abs() + r.beta.abs()) + r.gamma.abs() * exh + _floor(r.y, mant_bits),
         "mean": C_F32 * r.x.abs().mean(-1) + _floor(r.mean, 23),
         "rstd": C_F32 * r.rstd + _floor(r.rstd, 23)}
    if r.dy is not None:
        ag = r.g.abs()
        if mean_terms:
            terms = rs * (ag + ag.mean(-1, keepdim=True) + r.xhat.abs() * (r.g * r.xhat).abs().mean(-1, keepdim=True))
        else:
            terms = rs * (ag + r.m1.abs() + r.xhat.abs() * r.m2.abs())
        if r.dres is not None:
            terms = terms + r.dres.abs()
        centre = rs * (exh * r.m2.abs() + r.xhat.abs() * (ag * exh).mean(-1, keepdim=True))
        B["dx"] = c * terms + centre + _floor(r.dx, mant_bits)
        cg = max(C_F32, (recursive_rows + 2.0) * U32)
        B["dgamma"] = cg * (r.dy * r.xhat).abs().sum(0) + (r.dy.abs() * exh).sum(0) + _floor(r.dgamma, 23)
        B["dbeta"] = C_F32 * r.dy.abs().sum(0) + _floor(r.dbeta, 23)
    return B


LN_X_FAMILIES = ("randn", "offset8", "offset64", "offset200", "const0", "const1", "const256", "outlier8", "outlier64", "outlier256",
                 "alternating", "tiny")
LN_DY_FAMILIES = ("randn", "onehot", "const")


def ln_inputs(fam, dyfam, rows, H, gen, device="cpu"):
    """x, gamma, beta, dy, dres: fp32 tensors; x, dy, dres hold bf16 values.  gamma has zeros and negative entries."""
    rn = lambda *s: torch.randn(s, generator=gen, device=device)
    ar_r, ar_c = torch.arange(rows, device=device), torch.arange(H, device=device)
    if fam == "randn":
        x = rn(rows, H)
    elif fam.startswith("offset"):                                       # mean / std = 8, 64, 200
        x = float(fam[6:]) + rn(rows, H)
    elif fam.startswith("const"):                                        # y must equal beta
        x = torch.full((rows, H), float(fam[5:]), device=device)
    elif fam.startswith("outlier"):                                      # one element one bf16 ulp above the base
        base = float(fam[7:])
        x = torch.full((rows, H), base, device=device)
        x[ar_r, (7 * ar_r + 3) % H] = base * (1.0 + 2.0 ** -7)
    elif fam == "alternating":                                           # +-a, a = 1, 2, 4, 8, 16 by row
        a = (2.0 ** (ar_r % 5).float())[:, None]
        x = torch.where(ar_c[None] % 2 == 0, a, -a).expand(rows, H).contiguous()
    elif fam == "tiny":                                                  # eps dominates the variance
        x = 1.0e-3 * rn(rows, H)
    else:
        raise ValueError(fam)
    gamma = 1.0 + 0.5 * rn(H)
    gamma[::5] = 0.0
    gamma[1::7] = -gamma[1::7].abs() - 0.25
    beta = 0.5 * rn(H)
    if dyfam == "randn":
        dy = rn(rows, H)
    elif dyfam == "onehot":
        dy = torch.zeros((rows, H), device=device)
        dy[ar_r, (3 * ar_r + 1) % H] = 1.0
    elif dyfam == "const":
        dy = torch.full((rows, H), 0.5, device=device)
    else:
        raise ValueError(dyfam)
    return bf(x), gamma, beta, bf(dy), bf(rn(rows, H))


def ln_torch_f32(x, gamma, beta, eps, dy, dres, store_bf16=True):
    """The fp32 torch implementation of the same op (autograd of torch.nn.functional.layer_norm), y and dx rounded to bf16."""
    xx, g, b = x.float().clone().requires_grad_(True), gamma.float().clone().requires_grad_(True), beta.float().clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xx, (x.shape[-1],), g, b, eps)
    y.backward(dy.float())
    dx = xx.grad + (dres.float() if dres is not None else 0.0)
    mean = x.float().mean(-1)
    rstd = torch.rsqrt(x.float().var(-1, unbiased=False) + eps)
    rnd = bf if store_bf16 else (lambda t: t)
    return {"y": rnd(y.detach()), "mean": mean, "rstd": rstd, "dx": rnd(dx), "dgamma": g.grad, "dbeta": b.grad}


def ln_formula_f32(x, gamma, beta, eps, dy, dres):
    """The op as csrc/fp32_ops.hip states it, in fp32 torch: mean, centred sum of squares, dx = rstd (g - m1 - xhat m2) (+ dres), column
    sums of dy xhat and dy.  (torch.nn.functional.layer_norm's own fp32 backward computes dx from x, not from x - mean, and leaves the
    fp32 bounds on rows whose mean dwarfs their spread: ln_torch_f32 is the fp32 reference of the other families only.)"""
    x, gamma, beta, dy = x.float(), gamma.float(), beta.float(), dy.float()
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + eps)
    xhat = xc * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.float()
    return {"y": xhat * gamma + beta, "mean": mean[:, 0], "rstd": rstd[:, 0], "dx": dx, "dgamma": (dy * xhat).sum(0), "dbeta": dy.sum(0)}


# ---- log-softmax + gather -------------------------------------------------------------------------------------------------------------
def lse_reference(logits, labels, w=None):
    """logits [rows, V], labels [rows] (outside [0, V): gold logit 0, as the fused LM head defines it), w [rows] = d loss / d gold."""
    r = Ref()
    r.x = logits.double()
    rows, V = r.x.shape
    r.m = r.x.amax(-1)
    r.lse = torch.logsumexp(r.x, -1)
    r.inside = (labels >= 0) & (labels < V)
    lab = torch.where(r.inside, labels, torch.zeros_like(labels))
    r.xlab = torch.where(r.inside, r.x.gather(1, lab[:, None])[:, 0], torch.zeros_like(r.lse))
    r.gold = r.xlab - r.lse
    r.sm = torch.exp(r.x - r.lse[:, None])
    r.onehot = torch.zeros_like(r.x)
    r.onehot[r.inside, lab[r.inside]] = 1.0
    r.w = None
    if w is not None:
        r.w = w.double()
        r.dlogits = r.w[:, None] * (r.onehot - r.sm)
    return r


def lse_bounds(r, c=C_BF16, mant_bits=7):
    blse = C_F32 * (1.0 + r.m.abs() + (r.lse - r.m).abs())
    B = {"lse": blse + _floor(r.lse, 23), "gold": blse + C_F32 * r.xlab.abs() + _floor(r.gold, 23)}
    if r.w is not None:
        wsm = r.sm * (c + blse[:, None] + C_EXPARG * (r.x.abs() + r.lse.abs()[:, None])) + TINY
        B["dlogits"] = r.w.abs()[:, None] * (c * r.onehot + wsm) + _floor(r.dlogits, mant_bits)
    return B


LSE_FAMILIES = ("randn", "shift_up", "shift_down", "dominant", "equal", "staircase")


def lse_inputs(fam, rows, V, gen, device="cpu", out_of_range=False):
    """logits (fp32 holding bf16 values), labels, w = d loss / d gold.
    Labels, five rows: 0, V - 1, 255, 256 (each clipped to V - 1) and the row's dominant column, which lies PAST 255 whenever V > 256 (the
    second lap of the kernels' 256-thread loops); the dominant family also labels row 0 with its dominant column.  One row: V - 1.
    out_of_range (five rows): rows 1 and 3 -- interior rows, so that even an unguarded read stays inside the logits -- carry -100 and
    V + 7 instead; rows 0, 2, 4 keep their labels.
    w: 0 on row 0 of five, -1.5 on row 1, at least 0.25 in magnitude everywhere else (no backward check is vacuous but row 0's, whose
    dlogits must be exactly 0)."""
    rn = lambda *s: torch.randn(s, generator=gen, device=device)
    ar_r = torch.arange(rows, device=device)
    dom = 256 + (11 * ar_r + 5) % (V - 256) if V > 256 else (11 * ar_r + 5) % V
    if fam == "randn":
        x = rn(rows, V)
    elif fam == "shift_up":
        x = rn(rows, V) + 80.0
    elif fam == "shift_down":
        x = rn(rows, V) - 80.0
    elif fam == "dominant":                                              # one column 60 above the rest
        x = rn(rows, V)
        x[ar_r, dom] += 60.0
    elif fam == "equal":
        x = torch.full((rows, V), 3.0, device=device)
    elif fam == "staircase":                                             # spans 200
        x = (-100.0 + 200.0 * torch.arange(V, device=device).float() / max(V - 1, 1))[None].repeat(rows, 1) + 0.25 * rn(rows, V)
    else:
        raise ValueError(fam)
    picks = [0, V - 1, min(255, V - 1), min(256, V - 1)]
    labels = torch.tensor([V - 1] if rows == 1 else [picks[i % 5] if i % 5 < 4 else int(dom[i]) for i in range(rows)], dtype=torch.int64,
                          device=device)
    if fam == "dominant" and rows > 1:
        labels[0] = dom[0]
    w = rn(rows)
    w = torch.where(w.abs() < 0.25, torch.full_like(w, 0.5), w)
    if rows > 1:
        w[0], w[1] = 0.0, -1.5
    if out_of_range:
        if rows < 5 or V < 128:
            raise ValueError("out-of-range labels go on interior rows of five, V >= 128")
        labels[1], labels[3] = -100, V + 7
    return bf(x), labels, w


def lse_torch_f32(logits, labels, w, store_bf16=True):
    x = logits.float().clone().requires_grad_(True)
    V = x.shape[-1]
    inside = (labels >= 0) & (labels < V)
    lab = torch.where(inside, labels, torch.zeros_like(labels))
    lp = torch.log_softmax(x, -1)
    lse = torch.logsumexp(x, -1)
    gold = torch.where(inside, lp.gather(1, lab[:, None])[:, 0], -lse)
    gold.backward(w.float())
    rnd = bf if store_bf16 else (lambda t: t)
    return {"lse": lse.detach(), "gold": gold.detach(), "dlogits": rnd(x.grad)}


# ---- combine of per-slot (max, sum exp) -----------------------------------------------------------------------------------------------
def combine_reference(pmax, psum, gold):
    r = Ref()
    pm, ps = pmax.double(), psum.double()
    r.m = pm.amax(-1)
    r.s = (ps * torch.exp(pm - r.m[:, None])).sum(-1)
    r.lse = r.m + torch.log(r.s)
    r.gold = gold.double()
    r.out = r.gold - r.lse
    return r


def combine_bounds(r):
    blse = C_F32 * (1.0 + r.m.abs() + r.s.log().abs())
    return {"lse": blse + _floor(r.lse, 23), "out": blse + _floor(r.out, 23)}


def combine_inputs(rows, slots, gen, device="cpu"):
    """Synthetic partials of 64-column blocks: maxima around a per-row level, every third slot 200 below it, one slot with psum = 1
    exactly at the row maximum."""
    rn = lambda *s: torch.randn(s, generator=gen, device=device)
    level = 40.0 * rn(rows, 1)
    pmax = level + rn(rows, slots)
    pmax[:, 2::3] -= 200.0
    psum = 1.0 + 63.0 * torch.rand((rows, slots), generator=gen, device=device)
    top = torch.arange(rows, device=device) % slots
    pmax[torch.arange(rows, device=device), top] = level[:, 0] + 5.0
    psum[torch.arange(rows, device=device), top] = 1.0
    return pmax.float(), psum.float(), rn(rows).float()


# ---- retriever prior ------------------------------------------------------------------------------------------------------------------
def prior_reference(q, c, scale, g=None):
    """q [B, H], c [B, K, H], g [B, K] = d loss / d logp -> logp, prob (+ dq, dc)."""
    r = Ref()
    r.q, r.c, r.scale = q.double(), c.double(), float(scale)
    r.sim = torch.einsum("bh,bkh->bk", r.q, r.c) * r.scale
    r.simabs = torch.einsum("bh,bkh->bk", r.q.abs(), r.c.abs()) * abs(r.scale)
    r.m = r.sim.amax(-1, keepdim=True)
    r.lse = torch.logsumexp(r.sim, -1, keepdim=True)
    r.logp = r.sim - r.lse
    r.prob = torch.exp(r.logp)
    r.g = None
    if g is not None:
        r.g = g.double()
        r.G = r.g.sum(-1, keepdim=True)
        r.dsim = (r.g - r.prob * r.G) * r.scale
        r.dq = torch.einsum("bk,bkh->bh", r.dsim, r.c)
        r.dc = r.dsim[:, :, None] * r.q[:, None, :]
    return r


def prior_bounds(r, c=C_BF16, mant_bits=7):
    dsim = C_F32 * r.simabs                                              # the H-term dot product in fp32
    blogp = dsim + dsim.amax(-1, keepdim=True) + C_F32 * (1.0 + r.m.abs() + (r.lse - r.m).abs())
    bprob = r.prob * (C_F32 + blogp + C_EXPARG * r.logp.abs()) + TINY
    B = {"logp": blogp + _floor(r.logp, 23), "prob": bprob + _floor(r.prob, 23)}
    if r.g is not None:
        sabs = abs(r.scale)
        gabs = r.g.abs().sum(-1, keepdim=True)
        ddsim = sabs * (C_F32 * (r.g.abs() + r.prob * gabs) + bprob * r.G.abs())          # what fp32 leaves uncertain in dsim
        wd = c * r.dsim.abs() + ddsim + TINY
        B["dq"] = torch.einsum("bk,bkh->bh", wd, r.c.abs()) + _floor(r.dq, mant_bits)
        B["dc"] = wd[:, :, None] * r.q.abs()[:, None, :] + _floor(r.dc, mant_bits)
    return B


PRIOR_FAMILIES = ("randn_scaled", "wide", "ties", "leader")


def prior_inputs(fam, B, K, H, gen, device="cpu"):
    """q, c (fp32 holding bf16 values), scale, g.  randn_scaled: the product's 1 / sqrt(H); the others scale 1 with similarities over
    about +-300 (score scaling off); ties: passages duplicated in pairs; leader: one passage far ahead, every other prob underflows."""
    rn = lambda *s: torch.randn(s, generator=gen, device=device)
    q, c = rn(B, H), rn(B, K, H)
    scale = 1.0
    if fam == "randn_scaled":
        scale = 1.0 / math.sqrt(H)
    else:
        amp = math.sqrt(100.0 / math.sqrt(H))                           # <q, c> ~ N(0, amp^4 H) = N(0, 100^2): +-300 at three sigma
        q, c = amp * q, amp * c
        if fam == "ties" and K > 1:
            c[:, 1::2] = c[:, 0:2 * (K // 2):2]
        elif fam == "leader":
            c[:, K // 2] = 2.0 * q                                      # <q, 2 q> = 200 sqrt(H) >= 565
        elif fam not in ("wide", "ties"):
            raise ValueError(fam)
    g = rn(B, K)
    return bf(q), bf(c), scale, g.float()


def prior_torch_f32(q, c, scale, g, store_bf16=True):
    qq, cc = q.float().clone().requires_grad_(True), c.float().clone().requires_grad_(True)
    logp = torch.log_softmax(torch.einsum("bh,bkh->bk", qq, cc) * scale, -1)
    logp.backward(g.float())
    rnd = bf if store_bf16 else (lambda t: t)
    return {"logp": logp.detach(), "prob": logp.detach().exp(), "dq": rnd(qq.grad), "dc": rnd(cc.grad)}


# ---- EMDR2 marginal -------------------------------------------------------------------------------------------------------------------
def marginal_reference(prior, gold, gm=None):
    """prior [B, K], gold [B, K, L], gm [B, L] -> marginal [B, L] (+ dprior [B, K])."""
    r = Ref()
    r.prior, r.gold = prior.double(), gold.double()
    r.z = r.prior[:, :, None] + r.gold
    r.m = r.z.amax(1)
    r.marginal = torch.logsumexp(r.z, 1)
    r.gm = None
    if gm is not None:
        r.gm = gm.double()
        r.e = torch.exp(r.z - r.marginal[:, None, :])
        r.dprior = (r.gm[:, None, :] * r.e).sum(-1)
    return r


def marginal_bounds(r):
    bm = C_F32 * (1.0 + r.m.abs() + (r.marginal - r.m).abs())
    B = {"marginal": bm + _floor(r.marginal, 23)}
    if r.gm is not None:
        argabs = r.prior.abs()[:, :, None] + r.gold.abs() + r.marginal.abs()[:, None, :]
        we = r.e * (C_F32 + bm[:, None, :] + C_EXPARG * argabs) + TINY
        B["dprior"] = (r.gm.abs()[:, None, :] * we).sum(-1) + _floor(r.dprior, 23)
        B["identity"] = B["dprior"].sum(-1) + C_F32 * r.gm.abs().sum(-1)                 # sum_k dprior[b, k] = sum_l gm[b, l]
    return B


def marginal_inputs(B, K, L, gen, device="cpu"):
    """priors: log-softmax of similarities spread over +-300 (down to about -600); gold in [-200, 0] with whole columns at 0."""
    sim = 100.0 * torch.randn((B, K), generator=gen, device=device)
    prior = torch.log_softmax(sim.double(), -1).float()
    gold = -200.0 * torch.rand((B, K, L), generator=gen, device=device)
    gold[:, :, ::4] = 0.0
    gm = torch.randn((B, L), generator=gen, device=device)
    return prior, gold.float(), gm.float()


def marginal_torch_f32(prior, gold, gm):
    p = prior.float().clone().requires_grad_(True)
    out = torch.logsumexp(p[:, :, None] + gold.float(), 1)
    out.backward(gm.float())
    return {"marginal": out.detach(), "dprior": p.grad}


# ---- GELU derivative (exact erf form) -------------------------------------------------------------------------------------------------
def gelu_bwd_reference(x, dact):
    r = Ref()
    r.x, r.dact = x.double(), dact.double()
    r.cdf = 0.5 * torch.special.erfc(-r.x / math.sqrt(2.0))              # erfc: Phi keeps its relative accuracy in the left tail
    r.xpdf = r.x * torch.exp(-0.5 * r.x * r.x) / math.sqrt(2.0 * math.pi)
    r.dpre = r.dact * (r.cdf + r.xpdf)
    return r


def gelu_bwd_bounds(r, c=C_BF16, mant_bits=7):
    return {"dpre": r.dact.abs() * (c * (r.cdf + r.xpdf.abs()) + GELU_ABS) + _floor(r.dpre, mant_bits)}


def gelu_formula_f32(x):
    """The derivative as the kernel states it, in fp32 torch."""
    x = x.float()
    return 0.5 * (1.0 + torch.erf(x * 0.70710678118654752)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


def gelu_inputs(n, gen, device="cpu"):
    """x on a grid over [-12, 12] (bf16 values), +-0 and bf16 denormals among them; dact randn."""
    x = bf(torch.linspace(-12.0, 12.0, n, device=device))
    special = torch.tensor([0.0, -0.0, 2.0 ** -133, -(2.0 ** -133), 2.0 ** -127, -(2.0 ** -130), 12.0, -12.0], device=device)
    x[:8] = special
    return x, bf(torch.randn(n, generator=gen, device=device))


# ---- AdamW with global-norm clip (adam_kernel / adam_flat_kernel) ---------------------------------------------------------------------
def f32(v):
    return float(np.float32(v))


def _host_powf():
    """powf of the C library the host code of the kernels links against (numpy's float32 power as the fallback)."""
    import ctypes
    import ctypes.util
    try:
        fn = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").powf
        fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
        return lambda a, b: float(fn(a, b))
    except (OSError, AttributeError):
        return lambda a, b: float(np.power(np.float32(a), np.float32(b)))


def bias_corrections(b1, b2, step):
    """As the host computes them: 1 - powf(beta, (float)step) in fp32."""
    powf, one = _host_powf(), np.float32(1.0)
    return float(one - np.float32(powf(b1, float(step)))), float(one - np.float32(powf(b2, float(step))))


def adam_reference(master, grad, m, v, lr, b1, b2, eps, wd, step, gnorm_sq=None, clip=0.0, split=None):
    """One step from the given fp32 state, in float64, with the hyper-parameters rounded to fp32 as the kernel receives them.
    gnorm_sq: python float or None; the scale clip / (sqrt(gnorm_sq) + 1e-6) is applied only when < 1; eps outside the sqrt;
    split: elements [0, split) take the weight decay (None: all)."""
    lr, b1, b2, eps, wd, clip = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd), f32(clip)
    bc1, bc2 = bias_corrections(b1, b2, step)
    r = Ref()
    w0, g, m0, v0 = master.double(), grad.double(), m.double(), v.double()
    scale = 1.0
    if gnorm_sq is not None and clip > 0.0:
        cc = clip / (math.sqrt(f32(gnorm_sq)) + f32(1.0e-6))
        if cc < 1.0:
            scale = cc
    r.scale = scale
    g = g * scale
    r.t_m = (b1 * m0).abs() + ((1.0 - b1) * g).abs()
    r.t_v = (b2 * v0).abs() + (1.0 - b2) * g * g
    r.m = b1 * m0 + (1.0 - b1) * g
    r.v = b2 * v0 + (1.0 - b2) * g * g
    wdi = torch.full_like(w0, wd)
    if split is not None:
        wdi[split:] = 0.0
    adam = (r.m / bc1) / (torch.sqrt(r.v / bc2) + eps)
    r.t_w = lr * (adam.abs() + wdi * w0.abs())
    r.master = w0 - lr * (adam + wdi * w0)
    r.w0 = w0
    return r


def adam_bounds(r):
    return {"m": C_F32 * r.t_m + _floor(r.m, 23),
            "v": C_F32 * r.t_v + _floor(r.v, 23),
            "master": C_F32 * r.t_w + ADAM_ULPS * (_ulp(torch.maximum(r.master.abs(), r.w0.abs()), 23) + TINY)}


def sumsq_bound(g):
    s = (g.double() ** 2).sum()
    return s, C_F32 * s + _ulp(s, 23) + TINY
