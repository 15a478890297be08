"""The fp32 validation kernels of csrc/fp32_ops.hip -- the yardstick of "logits within 1e-3 fp32" -- each on its own against the float64
references that already exist (tests/gemm_ref.py, tests/elementwise_ref.py) with their fp32 constants (c = C_F32, mant_bits = 23).  Its
softmax and its log-softmax gather are checked elsewhere (test_attention_edges_gpu.py, test_elementwise_edges_gpu.py::test_lse_gather);
its embedding in test_embedding_edges_gpu.py.  Pass criterion: worst err / bound <= 1 for every quantity of every case.

emdr2_f32_gemm.  (M, N, K) in (1,1,1), (64,64,16), (65,63,17), (130,1,33), (1,130,15), (3,200,2): one tile exactly, one past it in every
dimension, ragged K, single rows and columns.  Six stride patterns, the ones model/kernels_f32.py drives it with: x W^T; dx (B
transposed); dW (both transposed); the bias gradient (B one row with row stride 0); the attention score and context products (2 x 3
batches through the batch and head strides of a packed [b, s, 3, heads, hn] / [b, s, 2, heads, hn] projection).  Operands are strided
views into NaN-filled storage (a read outside the M x K / N x K windows poisons the result), C is a window of a sentinel-filled buffer
(gemm_ref.sentinel_intact: a store outside the M x N window is seen); "full" = alpha 0.37, bias, residual and accumulate = 1 onto a
pre-filled C together.  Bound: gemm_ref.acc_bound on the majorant |alpha| |A| |B|^T + |bias| + |residual| + |C before| (residual and
the previous C are two more terms of the same fp32 sum) plus one fp32 ulp.  The exact families (onehot_k, coded with its fp32 code) are
compared with torch.equal.  Families that do not exist at a shape are not run: cancel at K = 1, coded at K < 3; cancel at odd K is the
family at K - 1 with a zero column.

LayerNorm.  elementwise_ref.ln_bounds(r, C_F32, 23) for y, mean, rstd and dbeta as it is, with two options of that module for dx and
dgamma (tests/test_elementwise_ref_cpu.py holds fp32 implementations on the CPU to both and shows them above 1 without):
  * mean_terms = True.  dx = rstd (g - m1 - xhat m2), and ln_bounds weighs the two row means by their VALUES,
    c rstd (|m1| + |xhat| |m2|), against the rule of these modules (magnitudes of the terms, never the value): m1 = mean_j g_j cancels,
    and whatever sums H fp32 terms errs by about u mean |g|.  With c = 2^-7 nobody sees that; with c = 2^-18 one row in a few hundred
    has |m1| below mean |g| / 600 and the bound collapses under a correct kernel: 63 "bounds" on a const0 row of H = 8, 35 on `tiny` at
    H = 768; on the CPU the fp32 formula scores 167 and fp32 torch 42 on const0 at 1,031 x 768.  With the option the means are weighed by
    the magnitudes of THEIR terms, c rstd (mean |g| + |xhat| mean |g xhat|).
  * recursive_rows = rows.  dgamma is one atomic per row, a recursive fp32 sum, and ln_bounds' C_F32 = 64 U32 proved too tight for it at
    1,031 rows: 1.41 on `alternating` rows with a constant dy at H = 63 (the terms of a column are all alike, every add rounds the same
    way; a row-by-row fp32 loop on the CPU scores the same 1.41).  With the option the constant is max(C_F32, (rows + 2) U32), the
    (n + 2) u bound of tests/embedding_ref.py.  Every other family and shape stays below 0.26 of C_F32's bound; dbeta never left it
    and keeps it.
The two right-hand columns below are ln_bounds without the options.  The bf16 tests do not pass them and are untouched.

Worst err / bound per kernel, family and quantity, measured on an MI355X.  No kernel changed with this file: one column per quantity.

    emdr2_f32_gemm      plain C / "full" C, worst over the six shapes; the same figures for x W^T, dx and dW
    pattern             randn         row_scaled    cancel        smooth        onehot_k, coded
    x W^T, dx, dW       0.05 / 0.10   0.05 / 0.13   0.03 / 0.08   0.02 / 0.11   0 (torch.equal)
    bias gradient       0.03 / 0.12   0.03 / 0.12   0.02 / 0.08   0.02 / 0.11   0 (torch.equal)
    scores, context     0.07 / 0.11   0.07 / 0.17   0.04 / 0.08   0.02 / 0.11   0 (torch.equal)
    every C window: the sentinel around it intact; accumulate = 0 overwrote a NaN pre-fill

    LayerNorm           y      mean   rstd   dx     dgamma   dbeta    without the options: dx      dgamma
    randn               0.13   0.01   0.03   0.10   0.04     0.01                          6.91    0.05
    offset8             0.12   0.01   0.04   0.11   0.10     0.01                          0.17    0.10
    offset64            0.12   0.01   0.04   0.12   0.11     0.01                          0.12    0.11
    offset200           0.08   0.01   0.04   0.08   0.08     0.01                          0.08    0.08
    const 0/1/256       0.00   0.00   0.01   0.05   0.00     0.00                          63.4    0.00
    outlier 8/64/256    0.08   0.01   0.02   0.08   0.08     0.00                          0.08    0.08
    alternating         0.03   0.00   0.03   0.07   0.10     0.00                          0.10    1.41
    tiny                0.08   0.01   0.02   0.06   0.04     0.01                          34.7    0.04
    by rows (worst over H and families), without the options: dx 0.34 at 1 row, 0.41 at 5, 63.4 at 1,031 (more rows, more
    near-cancelling means); dgamma 0.11 at 1 and 5 rows, 1.41 at 1,031 x 63 and 0.26 at 1,031 x 8 / 264 / 768

    GELU   n            1             255           257           65,544
           y / dpre     0.00 / 0.00   0.03 / 0.07   0.04 / 0.07   0.04 / 0.07

    retriever prior     logp   prob   dq     dc       (worst over (B, K, H), K = 1 and K = 1024 among them)
    randn, 1 / sqrt(H)  0.01   0.01   0.01   0.02
    wide (+-300)        0.01   0.01   0.01   0.01
    ties                0.01   0.00   0.01   0.01
    leader              0.01   0.00   0.00   0.01

What these tests found:
  * No wrong value in csrc/fp32_ops.hip: the GEMM's ragged M / N / K guards, its six stride patterns (stride 0 among them), both batch
    levels, alpha, bias, residual and accumulate, the row kernels at H below, at and off a multiple of 64, and the K <= 1024 prior all
    stay within a fifth of their bounds.  The yardstick holds at its edges.
  * The two limits of ln_bounds at the fp32 constant described above (a bound's, not a kernel's).
"""
import pytest
import torch

from tests import elementwise_ref as R
from tests import gemm_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
NAN = float("nan")
C32 = dict(c=R.C_F32, mant_bits=23)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _nat():
    from emdr2_amd import _native
    return _native, _native.lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _assert(tag, ratios):
    print("[f32-edges] %s " % tag + " ".join("%s=%.3f" % (n, r[0]) for n, r in sorted(ratios.items())))
    bad = {n: r for n, r in ratios.items() if not r[0] <= 1.0}
    assert not bad, (tag, bad)


def _merge(into, ratios):
    for n, (v, idx) in ratios.items():
        if not v <= into.get(n, (-1.0, None))[0]:
            into[n] = (v, idx)


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = ((1, 1, 1), (64, 64, 16), (65, 63, 17), (130, 1, 33), (1, 130, 15), (3, 200, 2))
PATTERNS = ("xWt", "dx", "dW", "dbias", "scores", "context")
B1, B2 = 2, 3


def _family(fam, M, N, K, seed, f32_codes=False):
    """gemm_ref.nt_inputs; cancel at odd K: the family at K - 1 and a zero column."""
    if fam == "cancel" and K % 2:
        A, B, bias, Rr = G.nt_inputs(fam, M, N, K - 1, seed, DEV)
        z = lambda t: torch.cat([t, torch.zeros((t.shape[0], 1), device=DEV)], 1)
        return z(A), z(B), bias, Rr
    return G.nt_inputs(fam, M, N, K, seed, DEV, f32_codes=f32_codes)


def _plain(X, transposed):
    """X [R, K] -> a [1, 1, R, K] view into NaN-filled storage, row-major with padding or stored transposed."""
    Rr, K = X.shape
    if transposed:
        buf = torch.full((K + 2, Rr + 3), NAN, device=DEV)
        v = buf[1:1 + K, :Rr].t()
    else:
        buf = torch.full((Rr + 2, K + 3), NAN, device=DEV)
        v = buf[1:1 + Rr, :K]
    v.copy_(X)
    return v[None, None]


def _operands(pattern, As, Bs):
    """As [B1 * B2 or 1][M, K], Bs likewise [N, K] -> logical views Av [b1, b2, M, K], Bv [b1, b2, N, K] laid out as the pattern's caller
    lays them out, and the C buffer geometry: (buf [nb, per, ld], window for sentinel_intact, Cv [b1, b2, M, N])."""
    M, K = As[0].shape
    N = Bs[0].shape[0]
    sent = lambda *s: torch.full(s, G.SENTINEL, device=DEV)
    if pattern in ("xWt", "dx", "dW", "dbias"):
        Av = _plain(As[0], pattern in ("dW", "dbias"))
        if pattern == "dbias":                                           # one row, row stride 0 (kernels_f32._param_grads: the ones vector)
            row = torch.full((K + 3,), NAN, device=DEV)
            row[:K] = Bs[0][0]
            Bv = row[:K].expand(N, K)[None, None]
        else:
            Bv = _plain(Bs[0], pattern in ("dx", "dW"))
        buf = sent(1, M + 6, N + 5)
        win = buf[:, 3:3 + M, :N]
        return Av, Bv, buf, win, win[None]
    A4 = torch.stack(As).reshape(B1, B2, M, K)
    B4 = torch.stack(Bs).reshape(B1, B2, N, K)
    if pattern == "scores":                                              # q, k of a packed [b, s, 3, heads, hn] projection: hn = K
        s = max(M, N) + 1
        qkv = torch.full((B1, s, 3, B2, K), NAN, device=DEV)
        q, k = qkv.select(2, 0)[:, :M], qkv.select(2, 1)[:, :N]
        q.copy_(A4.permute(0, 2, 1, 3))
        k.copy_(B4.permute(0, 2, 1, 3))
        buf = sent(B1 * B2, M + 6, N + 5)
        win = buf[:, 3:3 + M, :N]
        return q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), buf, win, win.unflatten(0, (B1, B2))
    # context: probabilities [b, heads, sq, sk] contiguous, v of a packed [b, sk, 2, heads, hn] projection (hn = N, sk = K), out [b, sq, heads, hn]
    Pm = A4.contiguous()
    kv = torch.full((B1, K + 1, 2, B2, N), NAN, device=DEV)
    v = kv.select(2, 1)[:, :K]
    v.copy_(B4.permute(0, 3, 1, 2))
    buf = sent(B1, M + 6, B2 * N + 5)
    win = buf[:, 3:3 + M, :B2 * N]
    return Pm, v.permute(0, 2, 3, 1), buf, win, win.unflatten(-1, (B2, N)).permute(0, 2, 1, 3)


def _gemm_case(pattern, fam, M, N, K, full, exact=False):
    from emdr2_amd.model import kernels_f32 as K32
    nb = B1 * B2 if pattern in ("scores", "context") else 1
    ins = [_family(fam, M, N, K, 7 + i, f32_codes=True) for i in range(nb)]
    Av, Bv, buf, win, Cv = _operands(pattern, [t[0] for t in ins], [t[1] for t in ins])
    bias = ins[0][2]
    alpha = 0.37 if full else 1.0
    res = rbuf = None
    Cold = None
    if full:
        bias = torch.randn(N, generator=_gen(3), device=DEV) if bias is None else bias
        Rl = torch.stack([t[3] for t in ins]).reshape(Cv.shape)
        rbuf = torch.full(buf.shape, NAN, device=DEV)                     # the residual is indexed like C: the same geometry in its own storage
        res = rbuf.as_strided(Cv.shape, Cv.stride(), Cv.storage_offset())
        res.copy_(Rl)
        Cold = G.bf(torch.randn(Cv.shape, generator=_gen(5), device=DEV))
        Cv.copy_(Cold)
    else:
        Cv.fill_(NAN)                                                    # accumulate = 0 must overwrite, not add
        if fam != "onehot_k":
            bias = None
    b1, b2 = Av.shape[:2]
    ab1, ab2, ars, acs = Av.stride()
    bb1, bb2, brs, bcs = Bv.stride()
    cb1, cb2, crs, ccs = Cv.stride()
    if pattern == "dbias":
        assert brs == 0 or N == 1
        brs = 0
        if N == 1:
            ccs = 0                                                      # as kernels_f32._param_grads passes it
    K32.gemm(Av, ars, acs, Bv, brs, bcs, Cv, crs, ccs, M, N, K, b1, ab1, bb1, cb1, b2, ab2, bb2, cb2, alpha=alpha, bias=bias, residual=res,
             accumulate=full)
    torch.cuda.synchronize()
    assert G.sentinel_intact(buf, win, 3), (pattern, fam, M, N, K, "C written outside its M x N window")
    r = G.nt_reference(Av, Bv, alpha=alpha, bias=bias)
    ref = r.pre
    if full:
        r.S = r.S + res.double().abs() + Cold.double().abs()
        ref = ref + res.double() + Cold.double()
    bound = G.acc_bound(r) + G._ulp(ref, 23) + G.TINY
    if exact:
        assert torch.equal(Cv.double(), ref), (pattern, fam, M, N, K, "exact family")
        if pattern == "xWt":
            assert torch.equal(Cv[0, 0], G.nt_exact(fam, M, N, K, f32_codes=True, device=DEV))
    return {"C_full" if full else "C": G.worst(Cv, ref, bound)}


@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_gemm(pattern, shape):
    M, N, K = shape
    for fam in G.FAMILIES:
        if fam == "cancel" and K < 2:
            continue
        ratios = {}
        for full in (False, True):
            _merge(ratios, _gemm_case(pattern, fam, M, N, K, full))
        _assert("gemm %s %s %dx%dx%d" % (pattern, fam, M, N, K), ratios)
    for fam in G.EXACT_FAMILIES:
        if fam == "coded" and K < 3:
            continue
        _assert("gemm %s %s %dx%dx%d" % (pattern, fam, M, N, K), _gemm_case(pattern, fam, M, N, K, False, exact=True))


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------
def _ln_run(x, gamma, beta, dy, dres):
    nat, lib = _nat()
    rows, H = x.shape
    y, mean, rstd = torch.full_like(x, NAN), torch.full((rows,), NAN, device=DEV), torch.full((rows,), NAN, device=DEV)
    nat.check(lib.emdr2_f32_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, H, EPS,
                                          nat.stream_ptr()), "f32_layernorm_fwd")
    dx, dg, db = torch.full_like(x, NAN), torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    nat.check(lib.emdr2_f32_layernorm_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _ptr(dres), dx.data_ptr(),
                                          dg.data_ptr(), db.data_ptr(), rows, H, nat.stream_ptr()), "f32_layernorm_bwd")
    torch.cuda.synchronize()
    return {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dgamma": dg, "dbeta": db}


def _ln_bounds(r, rows):
    return R.ln_bounds(r, mean_terms=True, recursive_rows=rows, **C32)


@pytest.mark.parametrize("rows", (1, 5, 1031))
@pytest.mark.parametrize("H", (8, 63, 264, 768))
def test_layernorm(H, rows):
    bad = {}
    for fam in R.LN_X_FAMILIES:
        ratios, plain = {}, {}
        for dyfam in R.LN_DY_FAMILIES:
            x, gamma, beta, dy, dres = R.ln_inputs(fam, dyfam, rows, H, _gen(rows * 7 + H), DEV)
            for dr in (None, dres):
                ref = R.ln_reference(x, gamma, beta, EPS, dy, dr)
                got = _ln_run(x, gamma, beta, dy, dr)
                _merge(ratios, R.worst_all(got, ref, _ln_bounds(ref, rows)))
                asis = R.ln_bounds(ref, **C32)
                _merge(plain, {"dx_by_value": R.worst(got["dx"], ref.dx, asis["dx"]), "dgamma_tree": R.worst(got["dgamma"], ref.dgamma, asis["dgamma"])})
        print("[f32-edges] ln %s rows=%d H=%d " % (fam, rows, H) + " ".join("%s=%.3f" % (n, r[0]) for n, r in sorted(ratios.items()))
              + "  (ln_bounds without its options: dx %.3f dgamma %.3f)" % (plain["dx_by_value"][0], plain["dgamma_tree"][0]))
        bad.update({(fam, n): r for n, r in ratios.items() if not r[0] <= 1.0})
    assert not bad, bad


# ---- GELU -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 255, 257, 65544))
def test_gelu(n):
    nat, lib = _nat()
    x, dact = R.gelu_inputs(max(n, 8), _gen(n), DEV)
    x, dact = x[:n].contiguous(), dact[:n].contiguous()
    y, dpre = torch.full((n + 1,), NAN, device=DEV), torch.full((n + 1,), NAN, device=DEV)
    y[n], dpre[n] = G.SENTINEL, G.SENTINEL                               # one element past the end
    nat.check(lib.emdr2_f32_gelu_fwd(x.data_ptr(), y.data_ptr(), n, nat.stream_ptr()), "f32_gelu_fwd")
    nat.check(lib.emdr2_f32_gelu_bwd(x.data_ptr(), dact.data_ptr(), dpre.data_ptr(), n, nat.stream_ptr()), "f32_gelu_bwd")
    torch.cuda.synchronize()
    assert float(y[n]) == G.SENTINEL and float(dpre[n]) == G.SENTINEL
    ref = G.gelu64(x.double())
    by = R.C_F32 * ref.abs() + G.GELU_ABS_X * x.double().abs().clamp(max=G.GELU_GRID) + R._ulp(ref, 23) + R.TINY
    r = R.gelu_bwd_reference(x, dact)
    ratios = {"y": R.worst(y[:n], ref, by)}
    ratios.update(R.worst_all({"dpre": dpre[:n]}, r, R.gelu_bwd_bounds(r, **C32)))
    _assert("gelu n=%d" % n, ratios)


# ---- retriever prior --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", R.PRIOR_FAMILIES)
@pytest.mark.parametrize("shape", ((1, 1, 8), (3, 7, 63), (2, 129, 264), (2, 1024, 64)), ids=lambda s: "%dx%dx%d" % s)
def test_retriever_prior(shape, fam):
    nat, lib = _nat()
    Bq, Kk, H = shape
    q, c, scale, g = R.prior_inputs(fam, Bq, Kk, H, _gen(Kk + H), DEV)
    q, c, g = q.contiguous(), c.contiguous(), g.contiguous()
    logp, prob = torch.full((Bq, Kk), NAN, device=DEV), torch.full((Bq, Kk), NAN, device=DEV)
    nat.check(lib.emdr2_f32_retriever_prior_fwd(q.data_ptr(), c.data_ptr(), logp.data_ptr(), prob.data_ptr(), Bq, Kk, H, float(scale), nat.stream_ptr()),
              "f32_retriever_prior_fwd")
    dq, dc = torch.full_like(q, NAN), torch.full_like(c, NAN)
    nat.check(lib.emdr2_f32_retriever_prior_bwd(g.data_ptr(), prob.data_ptr(), q.data_ptr(), c.data_ptr(), dq.data_ptr(), dc.data_ptr(), Bq, Kk, H,
                                                float(scale), nat.stream_ptr()), "f32_retriever_prior_bwd")
    torch.cuda.synchronize()
    r = R.prior_reference(q, c, scale, g)
    _assert("prior %s %dx%dx%d" % (fam, Bq, Kk, H), R.worst_all({"logp": logp, "prob": prob, "dq": dq, "dc": dc}, r, R.prior_bounds(r, **C32)))
