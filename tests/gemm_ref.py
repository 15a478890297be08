"""Float64 references, per-element majorant bounds and input families for the bf16 GEMM kernels: csrc/gemm.hip, gemm8.hip (NT form with
fused epilogues, the LSE epilogue) and gemm_tn.hip, gemm8t.hip (TN form, weight gradients) -- CPU and GPU tensors alike.  The pattern is
that of tests/attention_ref.py and tests/elementwise_ref.py, whose constants are imported, not restated.

Operations (the reference project's F.linear / bias-GELU / bias-dropout-add, restated in csrc/gemm.hip):

    pre = alpha A B^T + bias                    A [.., M, K], B [.., N, K], bias [N]
    act = gelu(pre) (erf form) | pre            der = gelu'(pre)         (gelu = 2: the derivative goes to the second output)
    v   = act * mask                            mask: 0 or the keep scale, passed in
    out = v | v + R | v * gelu'(R) | v * R      (residual modes 0, 1, 2)
    TN:   dW = A^T B, colsum = sum_r A[r, :]    A [R, I], B [R, J]
    LSE:  gold = pre_bf16[label] - logsumexp(pre_bf16), pre_bf16 = pre rounded to bf16; a label outside [0, V) gives -lse

Bounds.  Per element, against the sum of the MAGNITUDES of the terms (never |value|, never a tensor maximum).  bf16 x bf16 products are
exact in fp32, so for ANY summation order of K of them (tile order, split-K atomics, MFMA-internal order) the first-order error is at
most K 2^-24 S with the majorant S = |alpha| (|A| |B|^T) + |bias| in float64:

    g        = gamma_K S + K TINY,  gamma_K = (K + 8 + slices) 2^-24     (8: the affine step and its neighbours; slices only when > 1)
    pre      : g + C_BF16 |pre| + ulp_bf16 + TINY
    act      : L g + GELU_ABS_X min(|pre|, 14)            L = GELU_SUP = sup |gelu'| with GELU, 1 without (and no absolute term)
    der      : GELU2_SUP g + GELUP_ABS + C_BF16 |der| + ulp_bf16 + TINY
    out bf16 : F mask (act's bound) + |v| GELUP_ABS [mode 1] + C_BF16 T + ulp_bf16 + TINY
               F = 1, |gelu'(R)|, |R| and T = |v| (no residual), |v| + |R|, |v gelu'(R)|, |v R|: the value is rounded to bf16 BEFORE it
               meets the residual and again after
    out fp32 : the same without the C_BF16 term, one fp32 ulp
    TN       : gamma_R (|A|^T |B|) + ulp_fp32 + R TINY;  colsum: gamma_R sum_r |A| + ulp_fp32 + R TINY
    LSE      : elementwise_ref.lse_bounds on the bf16-rounded logits, plus the logits' own bound b = bound(pre): through the gold logit
               directly, through the logsumexp as log sum_n softmax_n exp(b_n) (the exact supremum of lse(x + d) - lse(x) over |d| <= b)

Beyond |x| = 14 the Abramowitz-Stegun form is exact to the underflow floor (exp(-98) is below 2^-126, the result is max(x, 0) to the bit
and the float64 tail is below 1e-43), hence min(|pre|, 14).

Constants.  GELU / GELU' use Abramowitz-Stegun 7.1.26 for erf (gemm_common.h).  Its erfc has a large RELATIVE error in the far tail (leading
coefficient 0.778 / z where 0.564 / z is exact) and a tiny ABSOLUTE one, so each carries an absolute term, measured by
tests/test_gemm_ref_cpu.py as max |fp32 model of the formula - float64| over a dense grid on [-14, 14] (the model is written from the
published coefficients p = 0.3275911, a = 0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429):

    GELU   max |model - float64| / |x|  = 2.97e-7     GELU_ABS_X = 6.0e-7 per unit of |x|   (twice the measured value, rounded up)
    GELU'  max |model - float64|        = 2.98e-7     GELUP_ABS  = 6.0e-7                   (twice the measured value, rounded up)

Worst err / bound of the fp32 torch implementation of the same op on the CPU (matmul, F.gelu, autograd of F.gelu for gelu', log_softmax;
rounded to bf16 where the kernel stores bf16), over every family below, asserted by tests/test_gemm_ref_cpu.py.  All are at or below 0.5,
so nothing is widened:

    quantity                                 worst ratio of the fp32 torch reference        constants
    plain / bias out (bf16, fp32)            0.25 / 0.02                                    C_BF16, gamma_K
    pre, der (bf16)                          0.25 / 0.25                                    C_BF16, GELU2_SUP, GELUP_ABS
    GELU out (bf16, fp32)                    0.25 / 0.03                                    GELU_SUP, GELU_ABS_X
    + R (bf16: plain, bias, dropout; fp32)   0.45 / 0.46 / 0.47; 0.03                       C_BF16 (|v| + |R|)
    * gelu'(R), * R (bf16)                   0.48 / 0.47                                    C_BF16 |v F|, GELUP_ABS
    TN dW / colsum (fp32)                    0.01 / 0.00                                    gamma_R
    LSE gold                                 0.00                                           lse_bounds + the logits' bound

(0.25 = one bf16 rounding, 2^-9, against C_BF16 = 2^-7; the residual recipes round twice.  The LSE ratio is small because the logits' own
bf16 rounding, C_BF16 x 300, dominates its bound: the sharp check of that epilogue is fused against unfused, 2e-4.)

Families (functions of the shape and a seed; operands are fp32 tensors whose values are exact in bf16):

    randn       everything N(0, 1).
    row_scaled  rows of A and rows of B times powers of two stepping through 2^-20 .. 2^20; bias and R scaled alike, bias zero on odd columns:
                the small rows are visible in their own elements.
    cancel      A[m, k + K/2] = -A[m, k], B[n, k + K/2] = B[n, k] except one k0(m) whose partner in A is 0 and whose value is 2^-8 in magnitude:
                the exact sum is A[m, k0] B[n, k0], at least 2^10 times below the majorant, while every partial sum up to K/2 is full-sized.
                bias and R are 2^-8 randn.  An intermediate bf16 rounding shows in bf16 outputs too.
    smooth      operands, bias and R vary slowly along m and n (sines), the product nearly cancels: an off-by-one column or row is a small
                error, not a large one.
    onehot_k    A row m is the unit vector at k(m) = (37 m + 5) % K; B holds the integers ((n K + k) 7 + 3) % 251, bias n % 5: exact in bf16
                and fp32, compared with torch.equal; with M >= K every k position is read exactly once.  TN: the same over r.
    coded       C[m, n] = code(m) + code(n), exact: bf16 8 (m % 32) + (n % 8); fp32 m + 65536 (n % 128) over four k columns.
    poison      a LAYOUT: operands are views into NaN-filled buffers (pad columns, rows before and after, gaps between batches), outputs views
                into sentinel-filled buffers; the sentinel must be bit-identical outside the window afterwards.
"""
import math

import torch

from tests.elementwise_ref import (C_BF16, C_F32, TINY, Ref, _ulp, bf, lse_bounds, lse_reference, old_metric, worst)  # noqa: F401

U32 = 2.0 ** -24
GELU_SUP = 1.13                          # sup |gelu'| = 1.1290 at x = sqrt 2
GELU2_SUP = 0.80                         # sup |gelu''| = 2 phi(0) = 0.7979
GELU_ABS_X = 6.0e-7                      # measured 2.97e-7 per unit of |x| (test_gemm_ref_cpu.test_gelu_formula_constants), doubled
GELUP_ABS = 6.0e-7                       # measured 2.98e-7, doubled
GELU_GRID = 14.0
FAMILIES = ("randn", "row_scaled", "cancel", "smooth")
EXACT_FAMILIES = ("onehot_k", "coded")
SENTINEL = -7777.0


# ---- float64 pieces -------------------------------------------------------------------------------------------------------------------
def gelu64(x):
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))             # erfc: Phi keeps its relative accuracy in the left tail


def gelu_grad64(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_as_f32(x):
    """GELU and GELU' by Abramowitz-Stegun 7.1.26 in fp32, from the published coefficients: erf(z) = 1 - P(t) exp(-z^2), t = 1 / (1 + p z)."""
    x = x.float()
    ax = x.abs()
    t = 1.0 / (1.0 + ax * (0.3275911 * 0.70710678118654752))
    e = torch.exp(-0.5 * x * x)
    hp = 0.5 * t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    gelu = torch.clamp(x, min=0.0) - ax * (hp * e)
    pos = ~torch.signbit(x)                                              # the SIGN BIT on both sides: gelu'(-0.0) = gelu'(+0.0) = 0.5
    grad = e * (x * 0.3989422804014327 - torch.where(pos, hp, -hp)) + pos.float()
    return gelu, grad


# ---- NT ---------------------------------------------------------------------------------------------------------------------------------
def nt_reference(A, B, alpha=1.0, bias=None, gelu=0, mask=None, R=None, rmode=0):
    """A [.., M, K], B [.., N, K] (leading batch dimensions broadcast), bias [N], mask / R [.., M, N] -> Ref, all float64."""
    r = Ref()
    a, b = A.double(), B.double()
    r.K, r.alpha, r.gelu, r.rmode = A.shape[-1], float(alpha), int(gelu), int(rmode)
    bt = b.transpose(-1, -2)
    r.bias = None if bias is None else bias.double()
    r.S = abs(r.alpha) * (a.abs() @ bt.abs())
    r.pre = r.alpha * (a @ bt)
    if bias is not None:
        r.S = r.S + r.bias.abs()
        r.pre = r.pre + r.bias
    r.der = gelu_grad64(r.pre) if r.gelu == 2 else None
    r.act = gelu64(r.pre) if r.gelu else r.pre
    r.mask = None if mask is None else mask.double()
    r.v = r.act if mask is None else r.act * r.mask
    r.R = None if R is None else R.double()
    if R is None:
        r.F, r.out = None, r.v
    elif r.rmode == 0:
        r.F, r.out = None, r.v + r.R
    elif r.rmode == 1:
        r.F = gelu_grad64(r.R)
        r.out = r.v * r.F
    else:
        r.F = r.R
        r.out = r.v * r.F
    return r


def acc_bound(r, slices=1):
    return (r.K + 8 + (slices if slices > 1 else 0)) * U32 * r.S + r.K * TINY


def nt_bounds(r, out_f32=False, slices=1):
    """{"out", "pre" (the bf16 second output without gelu = 2), "der" (with it)} -> bound tensors."""
    g = acc_bound(r, slices)
    B = {"pre": g + C_BF16 * r.pre.abs() + _ulp(r.pre, 7) + TINY}
    if r.der is not None:
        B["der"] = GELU2_SUP * g + GELUP_ABS + C_BF16 * r.der.abs() + _ulp(r.der, 7) + TINY
    e = GELU_SUP * g + GELU_ABS_X * r.pre.abs().clamp(max=GELU_GRID) if r.gelu else g
    if r.mask is not None:
        e = e * r.mask
    stored = r.v.abs()
    if r.R is not None:
        if r.rmode == 0:
            stored = stored + r.R.abs()
        else:
            e = e * r.F.abs()
            if r.rmode == 1:
                e = e + r.v.abs() * GELUP_ABS
            stored = (r.v * r.F).abs()
    B["out"] = e + _ulp(r.out, 23) + TINY if out_f32 else e + C_BF16 * stored + _ulp(r.out, 7) + TINY
    return B


def nt_torch_f32(A, B, alpha=1.0, bias=None, gelu=0, mask=None, R=None, rmode=0, out_f32=False):
    """The fp32 torch implementation of the same op; bf16 wherever the kernel stores bf16 (second output, value before the residual, output)."""
    rnd = (lambda t: t) if out_f32 else bf
    pre = alpha * (A.float() @ B.float().transpose(-1, -2))
    if bias is not None:
        pre = pre + bias.float()
    got = {"pre": bf(pre)}
    v = pre
    if gelu:
        x = pre.clone().requires_grad_(True)
        v = torch.nn.functional.gelu(x)
        if gelu == 2:
            got["der"] = bf(torch.autograd.grad(v.sum(), x)[0])
        v = v.detach()
    if mask is not None:
        v = v * mask.float()
    if R is not None:
        v, Rf = rnd(v), R.float()
        if rmode == 0:
            v = v + Rf
        elif rmode == 2:
            v = v * Rf
        else:
            x = Rf.clone().requires_grad_(True)
            v = v * torch.autograd.grad(torch.nn.functional.gelu(x).sum(), x)[0]
    got["out"] = rnd(v)
    return got


# ---- TN ---------------------------------------------------------------------------------------------------------------------------------
def tn_reference(A, B):
    """A [R, I], B [R, J] -> Ref dW [I, J], colsum [I], their majorants."""
    r = Ref()
    a, b = A.double(), B.double()
    r.R = A.shape[0]
    r.dW, r.S = a.t() @ b, a.abs().t() @ b.abs()
    r.colsum, r.Scol = a.sum(0), a.abs().sum(0)
    return r


def tn_bounds(r, slices=1):
    gam = (r.R + 8 + slices) * U32
    return {"dW": gam * r.S + _ulp(r.dW, 23) + r.R * TINY, "colsum": gam * r.Scol + _ulp(r.colsum, 23) + r.R * TINY}


def tn_torch_f32(A, B):
    return {"dW": A.float().t() @ B.float(), "colsum": A.float().sum(0)}


# ---- LSE epilogue -----------------------------------------------------------------------------------------------------------------------
def lse_nt_reference(A, B, alpha, bias, labels):
    r = nt_reference(A, B, alpha, bias)
    r.logits = bf(r.pre).double()                                        # what the kernel documents: logits rounded to bf16
    r.L = lse_reference(r.logits, labels)
    r.gold = r.L.gold
    return r


def lse_nt_bounds(r):
    b = nt_bounds(r)["pre"]
    viaset = torch.logsumexp(r.logits - r.L.lse[:, None] + b, -1)        # sup of lse(x + d) - lse(x) over |d| <= b
    lab = torch.where(r.L.inside, r.L.onehot.argmax(-1), torch.zeros_like(r.L.onehot.argmax(-1)))
    blab = torch.where(r.L.inside, b.gather(1, lab[:, None])[:, 0], torch.zeros_like(viaset))
    return {"gold": lse_bounds(r.L)["gold"] + viaset + blab}


def lse_torch_f32(A, B, alpha, bias, labels):
    logits = bf(alpha * (A.float() @ B.float().t()) + (0.0 if bias is None else bias.float()))
    V = logits.shape[-1]
    inside = (labels >= 0) & (labels < V)
    lab = torch.where(inside, labels, torch.zeros_like(labels))
    lp = torch.log_softmax(logits, -1)
    return {"gold": torch.where(inside, lp.gather(1, lab[:, None])[:, 0], -torch.logsumexp(logits, -1))}


def boundary_labels(M, V, device="cpu"):
    """Labels on both sides of every 16-, 64- and 256-column boundary (cycled over the rows), plus -100, V and V + 7 on rows 1, 3, 5."""
    edges = sorted(set(c + d for c in range(0, V + 1, 16) for d in (-1, 0) if 0 <= c + d < V))
    if M < len(edges) + 8:
        raise ValueError("need a row per boundary label")
    lab = torch.tensor([edges[(i - 8) % len(edges)] for i in range(M)], dtype=torch.int64, device=device)
    lab[1], lab[3], lab[5] = -100, V, V + 7
    return lab


# ---- families ---------------------------------------------------------------------------------------------------------------------------
def _pow2(idx, mul):
    return torch.exp2((((idx * mul) % 41) - 20).double()).float()


def nt_inputs(fam, M, N, K, seed, device="cpu", f32_codes=False):
    """-> A [M, K], B [N, K], bias [N], R [M, N]: fp32 tensors; A, B, R hold bf16 values.  For the exact families bias and R are None except
    onehot_k's integer bias; `f32_codes` selects the fp32 code of `coded`."""
    gen = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen, device=device)
    am, an, ak = torch.arange(M, device=device), torch.arange(N, device=device), torch.arange(K, device=device)
    if fam == "randn":
        A, B, bias, R = rn(M, K), rn(N, K), rn(N), rn(M, N)
    elif fam == "row_scaled":
        sa, sb = _pow2(am, 7), _pow2(an, 11)
        A, B = rn(M, K) * sa[:, None], rn(N, K) * sb[:, None]
        bias = rn(N) * sb * (an % 2 == 0).float()
        R = rn(M, N) * sa[:, None] * sb[None, :]
    elif fam == "cancel":
        h = K // 2
        A, B = rn(M, K), rn(N, K)
        A, B = bf(A), bf(B)
        A[:, h:], B[:, h:] = -A[:, :h], B[:, :h]
        k0 = (13 * am + 3) % h
        sign = torch.where(am % 2 == 0, 1.0, -1.0).to(A.dtype)
        A[am, k0] = sign * 2.0 ** -8 * (0.5 + 0.5 * torch.rand(M, generator=gen, device=device))
        A[am, k0 + h] = 0.0
        B[:, :h] = B[:, :h].clamp(-3.0, 3.0)
        B[:, h:] = B[:, :h]
        bias, R = 2.0 ** -8 * rn(N), 2.0 ** -8 * rn(M, N)
    elif fam == "smooth":
        th = 2.0 * math.pi * ak.float() / K
        A = 0.125 * torch.sin(3.0 * th[None, :] + 0.011 * am.float()[:, None])
        B = 0.125 * torch.cos(5.0 * th[None, :] + 0.013 * an.float()[:, None])
        bias = 1.0 + 0.5 * torch.sin(0.03 * an.float())
        R = 1.0 + 0.5 * torch.sin(0.03 * am.float()[:, None] + 0.02 * an.float()[None, :])
    elif fam == "onehot_k":
        A = torch.zeros((M, K), device=device)
        A[am, (37 * am + 5) % K] = 1.0
        B = (((an[:, None] * K + ak[None, :]) * 7 + 3) % 251).float()
        return A, B, (an % 5).float(), None
    elif fam == "coded":
        A, B = torch.zeros((M, K), device=device), torch.zeros((N, K), device=device)
        if f32_codes:                                                    # m + 65536 (n % 128), every factor an 8-bit integer times a power of two
            A[:, 0], A[:, 1], A[:, 2] = (am % 256).float(), ((am // 256) % 256).float(), 1.0
            B[:, 0], B[:, 1], B[:, 2] = 1.0, 256.0, (an % 128).float() * 65536.0
        else:                                                            # 8 (m % 32) + (n % 8) <= 255
            A[:, K - 1], A[:, 1] = ((am % 32) * 8).float(), 1.0
            B[:, K - 1], B[:, 1] = 1.0, (an % 8).float()
        return A, B, None, None
    else:
        raise ValueError(fam)
    return bf(A), bf(B), bias.float(), bf(R)


def nt_exact(fam, M, N, K, f32_codes=False, device="cpu"):
    """The exact result of an exact family (float32; onehot_k with its bias added)."""
    am, an = torch.arange(M, device=device), torch.arange(N, device=device)
    if fam == "onehot_k":
        return (((an[None, :] * K + ((37 * am + 5) % K)[:, None]) * 7 + 3) % 251 + (an % 5)[None, :]).float()
    if f32_codes:
        return (am[:, None] % 65536 + 65536 * (an % 128)[None, :]).float()
    return (8 * (am % 32)[:, None] + (an % 8)[None, :]).float()


def tn_inputs(fam, R, I, J, seed, device="cpu"):
    """-> A [R, I], B [R, J] (fp32 holding bf16 values).  onehot_k over r: A[:, i] is the unit vector at r(i) = (37 i + 5) % R, so
    dW[i, j] = B[r(i), j] and colsum = 1, exactly."""
    gen = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen, device=device)
    ar, ai, aj = torch.arange(R, device=device), torch.arange(I, device=device), torch.arange(J, device=device)
    if fam == "randn":
        A, B = rn(R, I), rn(R, J)
    elif fam == "row_scaled":                                            # the scales run along the OUTPUT rows and columns
        A, B = rn(R, I) * _pow2(ai, 7)[None, :], rn(R, J) * _pow2(aj, 11)[None, :]
    elif fam == "cancel":
        h = R // 2
        A, B = bf(rn(R, I)), bf(rn(R, J)).clamp(-3.0, 3.0)
        A[h:2 * h], B[h:2 * h] = -A[:h], B[:h]
        A[2 * h:], B[2 * h:] = 0.0, 0.0
        r0 = (13 * ai + 3) % h
        sign = torch.where(ai % 2 == 0, 1.0, -1.0).to(A.dtype)
        A[r0, ai] = sign * 2.0 ** -8 * (0.5 + 0.5 * torch.rand(I, generator=gen, device=device))
        A[r0 + h, ai] = 0.0
    elif fam == "smooth":
        th = 2.0 * math.pi * ar.float() / R
        A = 0.125 * torch.sin(3.0 * th[:, None] + 0.011 * ai.float()[None, :])
        B = 0.125 * torch.cos(5.0 * th[:, None] + 0.013 * aj.float()[None, :])
    elif fam == "onehot_k":
        A = torch.zeros((R, I), device=device)
        A[(37 * ai + 5) % R, ai] = 1.0
        B = (((ar[:, None] * J + aj[None, :]) * 7 + 3) % 251).float()
    else:
        raise ValueError(fam)
    return bf(A), bf(B)


def keep_mask(M, N, p, seed, device="cpu"):
    """A multiplicative dropout mask for the CPU tests (the GPU tests take emdr2_dropout's): 0 or 1 / (1 - p)."""
    gen = torch.Generator(device=device).manual_seed(seed)
    return (torch.rand((M, N), generator=gen, device=device) >= p).float() / (1.0 - p)


# ---- the poison layout ------------------------------------------------------------------------------------------------------------------
def poisoned(t, ld, before=3, after=3, dtype=torch.bfloat16, fill=float("nan"), batch_gap=0):
    """A view shaped like `t` ([rows, cols] or [batch, rows, cols]) holding its values inside a buffer filled with `fill`: leading dimension
    `ld` > cols, `before` / `after` rows in front of and behind each matrix (`batch_gap` more between batches).  -> (buffer, view)."""
    rows, cols = t.shape[-2], t.shape[-1]
    nb = t.shape[0] if t.dim() == 3 else 1
    per = before + rows + after + batch_gap
    buf = torch.full((nb, per, ld), fill, dtype=dtype, device=t.device)
    view = buf[:, before:before + rows, :cols]
    view.copy_(t.reshape(nb, rows, cols).to(dtype))
    return buf, (view if t.dim() == 3 else view[0])


def sentinel_intact(buf, view_of_buf, before):
    """True when everything of `buf` outside the window `view_of_buf` still holds its fill bit for bit."""
    ints = {2: torch.int16, 4: torch.int32}[buf.element_size()]
    b = buf.view(ints).clone()
    rows, cols = view_of_buf.shape[-2], view_of_buf.shape[-1]
    fill = b[0, 0, -1].item()                                            # the last pad column of a `before` row (or of row 0's padding)
    b[:, before:before + rows, :cols] = fill
    return bool((b == fill).all())


def lse_inputs(fam, M, V, K, seed, device="cpu"):
    """-> hidden [M, K], W [V, K] (bf16 values), bias [V], labels [M] for the LSE epilogue, logits spanning about +-300.
    row_scaled: hidden rows times 2^-3 .. 2^3 (a row's logits span +-4 up to +-300); smooth: the bias is a slow sine of amplitude 300 and
    the product nearly cancels."""
    gen = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen, device=device)
    am, av = torch.arange(M, device=device), torch.arange(V, device=device)
    if fam == "row_scaled":
        A = rn(M, K) * torch.exp2(((am * 5) % 7 - 3).float())[:, None]
        B = rn(V, K) * (300.0 / (8.0 * 3.5 * math.sqrt(K)))
        bias = rn(V)
    elif fam == "smooth":
        A, B, _, _ = nt_inputs("smooth", M, V, K, seed, device)
        bias = 300.0 * torch.sin(0.02 * av.float())
    else:
        raise ValueError(fam)
    return bf(A), bf(B), bias.float(), boundary_labels(M, V, device)
