"""GPU: every dispatch path of the bf16 GEMM kernels (csrc/gemm.hip, gemm8.hip, gemm_tn.hip, gemm8t.hip) against the float64 references and
per-element majorant bounds of tests/gemm_ref.py, on the families randn / row_scaled / cancel / smooth, exactly (torch.equal) on onehot_k /
coded, and in the poison layout (NaN around every operand, a sentinel around every output, bit-identical afterwards).  The float64
reference is computed on the GPU, in row blocks of 2,048.  Each shape is the smallest that reaches its path; the arithmetic that sends it
there stands next to it (dispatch: emdr2_gemm_nt_bf16 / emdr2_gemm8_try / emdr2_gemm_tn_bf16 / emdr2_gemm8t_try).

Worst err / bound per path and family, MI355X, every path in the poison layout (every test prints `RATIO path family output ratio`;
1.0 is the bound; bf16 outputs sit at 0.25 = one rounding of 2^-9 against C_BF16, 0.49 where the residual recipes round twice; fp32
outputs far below their worst-case gamma_K S):

    path (kernel variant, test id)           randn   row_scaled   cancel   smooth   onehot_k / coded
    <8,1>  g81_n40 / g81_n128                0.25    0.48         0.22     0.38     exact, bf16 and fp32
    <2,4>  g24 / g24_m1                      0.25    0.48         0.21     0.38     exact, bf16 and fp32
    <2,1>  g21                               0.25    0.48         0.19     0.38     exact, bf16 and fp32
    <2,2>  g22 / g22_2groups (6 + 5)         0.25    0.49         0.23     0.40     exact, bf16 and fp32
    <4,2>  2-D / one group / 6 + 5 groups    0.25    0.49         0.24     0.40     exact, bf16 and fp32
    the same five, fp32 output (scalar)      0.06    0.07         0.02     0.09
    vector / scalar (ldc 137) / N = 132      0.48    0.48         0.24     0.38     exact (scalar, N = 132); vector - scalar: 0.00 of two bounds
    split-K 5 chunks in 4 / weight_grad_nt   0.01    0.01         0.01     0.01     exact (fp32)
    two-level batch 2 x 3, bf16 / fp32       0.25    0.25 / 0.02  0.08     0.13     exact, six distinct rolls, bf16 and fp32
    gemm8, ten recipes                       0.49    0.49         0.21     0.40     gemm8 - general kernel: 0.00 of two bounds
    general kernel, ten recipes (M + 8)      0.49    0.49         0.21     0.40
    gemm8 K = 128                            0.25    0.25         0.24     0.25     exact (bf16), also at (4096, 512, 256)
    gemm8 strided + poisoned, four recipes   0.49    0.49         0.21     0.40     exact, bf16 (gemm8) and fp32 (general)
    gemm8 in place (radd, bias_radd)         0.49    0.49         0.05     0.38     exact (onehot_k, integer residual); in place == out of place
    gemm8 352-tile seams, groups 6 + 5       -       0.49         -        -        exact (onehot_k)
    LSE fused / unfused, both shapes         -       0.00         -        0.00     fused - unfused: at most 3.8e-6; the limit is 2e-4
    gemm8t R = 128, 2112; gemm_tn 96, 2080   -       0.01         0.01     -        exact (onehot_k over r), dW and colsum
    weight_grad_tn R = 8256 / 8224           0.00    0.00         0.00     0.00

Every sentinel region was bit-identical after its call and no output inside a window was non-finite.  The one fault found: gelu'(-0.0)
came out 1.5 instead of 0.5 (gemm_common.h: the step was taken from `x >= 0`, the sign of P(t) / 2 from the sign bit); the rgelu recipe
carries +0.0 and -0.0 in its saved pre-activations: 166.7 bounds on the parent's library (both kernels), 0.49 after the fix.
"""
import pytest
import torch

from tests import gemm_ref as G
from tests.attention_ref import keep_scale

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
BLOCK = 2048

RECIPES = {                               # the ten recipes of emdr2_gemm8_try's switch, by its enum
    "plain": dict(),                                                     # 0
    "bias": dict(bias=1),                                                # G8_BIAS
    "bias_gelu": dict(bias=1, gelu=1),                                   # G8_BIAS | G8_GELU
    "bias_gelu_pre": dict(bias=1, gelu=1, pre=1),                        # G8_BIAS | G8_GELU | G8_PRE
    "radd": dict(R=1),                                                   # G8_RADD
    "bias_radd": dict(bias=1, R=1),                                      # G8_BIAS | G8_RADD
    "bias_drop_radd": dict(bias=1, R=1, drop=0.1),                       # G8_BIAS | G8_DROP | G8_RADD
    "rgelu": dict(R=1, rmode=1),                                         # G8_RGELU
    "bias_gelu_preg": dict(bias=1, gelu=2, pre=1),                       # G8_BIAS | G8_GELU | G8_PRE | G8_PREG
    "rmul": dict(R=1, rmode=2),                                          # G8_RMUL
}
SEED = 12345


def _lib():
    from emdr2_amd import _native as nat
    return nat, nat.lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _gemm(A, B, C, bias=None, gelu=0, pre=None, R=None, rmode=0, alpha=1.0, split=1, drop_p=0.0, seed=0, batch=None):
    """A [.., M, K], B [.., N, K], C [.., M, N] (bf16 or fp32): possibly strided views; batch = (b1, sA1, sB1, sC1, b2, sA2, sB2, sC2)."""
    nat, lib = _lib()
    M, K = A.shape[-2:]
    N = B.shape[-2]
    assert A.stride(-1) == 1 and B.stride(-1) == 1 and C.stride(-1) == 1
    for t in (pre, R):
        assert t is None or (t.stride(-2) == C.stride(-2) and t.dtype == BF16)          # same indexing as C
    b = batch or (1, 0, 0, 0, 1, 0, 0, 0)
    nat.check(lib.emdr2_gemm_nt_bf16(A.data_ptr(), A.stride(-2), B.data_ptr(), B.stride(-2), C.data_ptr(), C.stride(-2), M, N, K, *b, alpha,
                                     _ptr(bias), int(gelu), _ptr(pre), _ptr(R), int(rmode), int(C.dtype == torch.float32), split, float(drop_p),
                                     int(seed), nat.stream_ptr()), "gemm_nt_bf16")
    return C


def _drop_mask(M, N, p, seed):
    """The multiplicative mask the epilogue applies: keep bits of emdr2_dropout for (seed, row, column), times the fp32 keep scale.
    (The bits are a function of the row and the column alone; the kernel wants a multiple of 8 columns.)"""
    nat, lib = _lib()
    cols = (N + 7) // 8 * 8
    ones = torch.ones((M, cols), dtype=BF16, device=DEV)
    out = torch.empty_like(ones)
    nat.check(lib.emdr2_dropout(ones.data_ptr(), out.data_ptr(), ones.numel(), cols, p, seed, nat.stream_ptr()), "dropout")
    return (out[:, :N] != 0).double() * keep_scale(p)


def _note(path, fam, name, ratio):
    print("RATIO %-22s %-10s %-6s %.3f" % (path, fam, name, ratio))


def _judge(path, fam, A, B, gots, out_f32=False, slices=1, cross=False, **args):
    """gots: list of {name: tensor [.., M, N]} (each judged against the bounds; cross: the first two may differ by at most two bounds).
    args: alpha, bias, gelu, mask, R, rmode with full-size tensors."""
    M = A.shape[-2]
    worst, wcross = {}, 0.0
    for lo in range(0, M, BLOCK):
        sl = slice(lo, min(lo + BLOCK, M))
        a = dict(args)
        for k in ("mask", "R"):
            if a.get(k) is not None:
                a[k] = a[k][..., sl, :]
        r = G.nt_reference(A[..., sl, :], B, **a)
        bd = G.nt_bounds(r, out_f32=out_f32, slices=slices)
        for i, got in enumerate(gots):
            for name, t in got.items():
                ratio, idx = G.worst(t[..., sl, :], getattr(r, name), bd[name])
                worst[(i, name)] = max(worst.get((i, name), 0.0), ratio)
        if cross:
            for name in gots[0]:
                d = (gots[0][name][..., sl, :].double() - gots[1][name][..., sl, :].double()).abs()
                wcross = max(wcross, float((d / (2.0 * bd[name])).max()))
    for (i, name), ratio in sorted(worst.items()):
        _note(path if i == 0 else path + "/general", fam, name, ratio)
    if cross:
        _note(path + "/cross", fam, "diff", wcross)
    assert all(v <= 1.0 for v in worst.values()) and wcross <= 1.0, (path, fam, worst, wcross)


def _run_recipe(path, fam, M, N, K, recipe, out_f32=False, alpha=1.0, ldc=None, poison=False, rows=None, inputs=None, judge=True):
    """One call of the product entry point on family `fam`; rows: run on the first `rows` rows of operands generated for M rows.
    -> (gots, inputs, args): gots = {"out": .., "pre" / "der": ..} as [rows, N] tensors (views of the output buffers)."""
    kw = RECIPES[recipe] if isinstance(recipe, str) else recipe
    A, B, bias, R = inputs or G.nt_inputs(fam, M, N, K, 7, DEV)
    rows = rows or M
    A, R = A[:rows], (R[:rows] if kw.get("R") else None)
    if kw.get("rmode") == 1:                                             # +0.0 and -0.0 among the saved pre-activations: gelu' is 0.5 at both
        R = R.clone()
        if rows > 1:
            R[0, :8], R[1, :8] = 0.0, -0.0
    bias = bias if kw.get("bias") else None
    odt = torch.float32 if out_f32 else BF16
    ldc = ldc or (N + 8 if poison else N)
    if poison:                                                           # lda, ldb > K, ldc > N (all multiples of 8), NaN rows around A, B, R
        _, Ab = G.poisoned(A, K + 8)
        _, Bb = G.poisoned(B, K + 16)
    else:
        Ab, Bb = A.to(BF16).contiguous(), B.to(BF16).contiguous()
    fill = G.SENTINEL
    Cbuf = torch.full((1, rows + 6, ldc), fill, dtype=odt, device=DEV)
    C = Cbuf[0, 3:3 + rows, :N]
    Pbuf = torch.full((1, rows + 6, ldc), fill, dtype=BF16, device=DEV) if kw.get("pre") else None
    P = None if Pbuf is None else Pbuf[0, 3:3 + rows, :N]
    Rb = None if R is None else G.poisoned(R, ldc)[1]
    p = kw.get("drop", 0.0)
    _gemm(Ab, Bb, C, bias=bias, gelu=kw.get("gelu", 0), pre=P, R=Rb, rmode=kw.get("rmode", 0), alpha=alpha, drop_p=p, seed=SEED)
    torch.cuda.synchronize()
    assert G.sentinel_intact(Cbuf, C, 3), (path, fam, recipe, "C written outside its window")
    gots = {"out": C}
    if P is not None:
        assert G.sentinel_intact(Pbuf, P, 3), (path, fam, recipe, "second output written outside its window")
        gots["der" if kw.get("gelu") == 2 else "pre"] = P
    args = dict(alpha=alpha, bias=bias, gelu=kw.get("gelu", 0), mask=_drop_mask(rows, N, p, SEED) if p else None, R=R, rmode=kw.get("rmode", 0))
    if judge:
        _judge(path, fam, A, B, [gots], out_f32=out_f32, **args)
    return gots, (A, B), args


def _exact(path, M, N, K, ldc=None, poison=True):
    """onehot_k and coded, bf16 and fp32 output, compared with torch.equal (in the poison layout unless told otherwise)."""
    for fam in G.EXACT_FAMILIES:
        for f32 in (False, True):
            A, B, bias, _ = G.nt_inputs(fam, M, N, K, 0, DEV, f32_codes=f32)
            gots, _, _ = _run_recipe(path, fam, M, N, K, dict(bias=1) if bias is not None else dict(), out_f32=f32, ldc=ldc,
                                     poison=poison, inputs=(A, B, bias, None), judge=False)
            assert torch.equal(gots["out"].float(), G.nt_exact(fam, M, N, K, f32_codes=f32, device=DEV)), (path, fam, f32)
            _note(path, fam, "f32" if f32 else "bf16", 0.0)


# family -> the bf16 recipe it runs on every path of the general kernel (the ten recipes all run on both kernels in the gemm8 tests)
PATH_RECIPE = {"randn": "bias_gelu_preg", "row_scaled": "bias_radd", "cancel": "bias", "smooth": "bias_drop_radd"}

# Dispatch of emdr2_gemm_nt_bf16 for shapes gemm8 does not take (M % 256 != 0 here): N <= 128 -> <8,1> (512 x 128 tiles); else M <= 128 ->
# <2,4> (128 x 512); else with t256 = ceil(M / 256) ceil(N / 256) and t128 = ceil(M / 128) ceil(N / 256): t256 < 192 -> t128 >= 128 ? <2,2>
# (128 x 256) : <2,1> (128 x 128); else <4,2> (256 x 256).  launch_gemm_v: order = 1 (1-D XCD walk) iff tiles_n > 1 and tiles_m > 8;
# ng = 2560 KiB / (BN K 2 B), one group when ng > tiles_n, 2 ng < tiles_n or N K 2 B <= 4 MiB; groups are balanced.
# gemm8 (emdr2_gemm8_try) takes M % 256 == 0, N % 256 == 0, K % 128 == 0, M >= 4096; gemm8t (emdr2_gemm8t_try) takes R % 64 == 0.
# NOTHING below can see which variant ran: the shapes follow from the thresholds named here -- N <= 128, M <= 128, t256 < 192, t128 >= 128,
# tiles_m > 8, 2560 KiB, 4 MiB, M >= 4096, R % 64 -- as the dispatch code stands today.  Whoever moves one of them re-derives the shapes.
# Every path runs in the poison layout: the overhang rows and columns that the ragged tiles clamp, and the speculative re-reads past the
# last K chunk, have NaN next to them.
GENERAL_PATHS = [
    ("g81_n40", 1030, 40, 96),         # N = 40 <= 128 -> <8,1>; 3 m-tiles of 512, the last with 6 rows; 3 K chunks
    ("g81_n128", 1030, 128, 64),       # N = 128 <= 128 -> <8,1>, a full n-tile
    ("g24", 64, 520, 64),              # N > 128, M = 64 <= 128 -> <2,4>; 2 n-tiles of 512, the last 8 wide
    ("g24_m1", 1, 520, 64),            # the same with a single row
    ("g21", 300, 264, 96),             # t256 = 2 * 2 = 4 < 192, t128 = 3 * 2 = 6 < 128 -> <2,1>; 3 x 3 tiles of 128 x 128
    ("g22", 1660, 2312, 64),           # t256 = 7 * 10 = 70 < 192, t128 = 13 * 10 = 130 >= 128 -> <2,2>; tiles_m = 13 > 8: 1-D order, one group
    ("g42_2d", 49160, 136, 32),        # t256 = 193 * 1 = 193 >= 192 -> <4,2>; tiles_n = 1 -> order 0, the plain 2-D grid
    ("g42_1group", 4360, 3080, 64),    # t256 = 18 * 13 = 234 -> <4,2>; tiles_m = 18 > 8 -> 1-D; N K 2 = 385 KiB <= 4 MiB -> one group
    ("g42_2groups", 4360, 2816, 768),  # t256 = 18 * 11 = 198 -> <4,2>; panel 384 KiB -> ng = 6, 2 * 6 >= 11, N K 2 = 4.1 MiB > 4 MiB -> groups of 6 + 5
]                                      # (M = 4100, the smallest M past 4096 off gemm8, has t256 = 17 * 11 = 187 < 192 and lands on <2,2>)


@pytest.mark.parametrize("path,M,N,K", GENERAL_PATHS, ids=[p[0] for p in GENERAL_PATHS])
def test_general_kernel_paths(path, M, N, K):
    for fam in G.FAMILIES:
        _run_recipe(path, fam, M, N, K, PATH_RECIPE[fam], alpha=0.125 if fam == "cancel" else 1.0, poison=True)   # vector epilogue (N % 8 == 0)
        _run_recipe(path + "_f32", fam, M, N, K, dict(bias=1, R=1), out_f32=True, alpha=0.125, poison=True)       # scalar epilogue (fp32 output)
    _exact(path, M, N, K)


def test_general_kernel_grouped_order_on_the_128_row_tiles():
    """(4100, 2816, 768): t256 = 17 * 11 = 187 < 192, t128 = 33 * 11 >= 128 -> <2,2>; tiles_m = 33 > 8 -> 1-D order; groups of 6 + 5 n-tiles."""
    _run_recipe("g22_2groups", "row_scaled", 4100, 2816, 768, "bias_radd", poison=True)
    _exact("g22_2groups", 4100, 2816, 768)


@pytest.mark.parametrize("recipe", ["bias_gelu_preg", "bias_drop_radd", "rgelu", "bias_gelu_pre"])
def test_vector_and_scalar_epilogue_agree_within_the_bounds(recipe):
    """(300, 136, 96) -> <2,1>.  ldc = 136: vector epilogue; ldc = 137 (not a multiple of 8): the scalar one, same operands, same recipe.
    N = 132 (N % 8 != 0) reaches the scalar epilogue too."""
    for fam in G.FAMILIES:
        inputs = G.nt_inputs(fam, 300, 136, 96, 7, DEV)
        vec, (A, B), args = _run_recipe("g21_vec", fam, 300, 136, 96, recipe, inputs=inputs, poison=True)
        sca, _, _ = _run_recipe("g21_scalar", fam, 300, 136, 96, recipe, ldc=137, inputs=inputs, poison=True)
        _judge("g21_vec_scalar", fam, A, B, [vec, sca], cross=True, **args)
        _run_recipe("g21_n132", fam, 300, 132, 96, recipe, ldc=132, poison=True)
    _exact("g21_scalar", 300, 136, 96, ldc=137)
    _exact("g21_n132", 300, 132, 96, ldc=132)


def test_split_k_with_an_empty_and_a_short_slice():
    """K = 160: chunks = 5, split = 4 -> per = 2: slices of 2, 2, 1 chunks and an EMPTY one.  split_k > 1 skips the small-tile variants:
    <4,2>, tiles_m = 2 <= 8 -> the 2-D grid, fp32 atomics into a pre-zeroed C (scalar epilogue)."""
    M, N, K = 300, 264, 160
    for fam in G.FAMILIES + G.EXACT_FAMILIES:
        A, B, _, _ = G.nt_inputs(fam, M, N, K, 3, DEV, f32_codes=True)
        Cbuf = torch.full((1, M + 6, N + 8), G.SENTINEL, dtype=torch.float32, device=DEV)
        C = Cbuf[0, 3:3 + M, :N]
        C.zero_()
        _gemm(G.poisoned(A, K + 8)[1], G.poisoned(B, K + 8)[1], C, split=4)
        torch.cuda.synchronize()
        assert G.sentinel_intact(Cbuf, C, 3)
        if fam in G.EXACT_FAMILIES:
            exact = G.nt_exact(fam, M, N, K, f32_codes=True, device=DEV)
            if fam == "onehot_k":
                exact = exact - (torch.arange(N, device=DEV) % 5).float()[None, :]          # split-K takes no bias
            assert torch.equal(C, exact), fam
        else:
            _judge("g42_splitk", fam, A, B, [{"out": C}], out_f32=True, slices=4)


def test_weight_grad_nt_splits_the_reduction():
    """kernels.weight_grad_nt: dW [264, 136] = dyT [264, 12320] xT [136, 12320]^T; tiles = 2 * 1, split = min(512 // 2, 12320 // 4096) = 3;
    385 chunks -> slices of 129, 129, 127."""
    from emdr2_amd.model import kernels
    for fam in G.FAMILIES:
        A, B, _, _ = G.nt_inputs(fam, 264, 136, 12320, 5, DEV)
        C = kernels.weight_grad_nt(A.to(BF16), B.to(BF16))
        torch.cuda.synchronize()
        _judge("weight_grad_nt", fam, A, B, [{"out": C}], out_f32=True, slices=3)
    for fam in G.EXACT_FAMILIES:                                         # integer partial sums: the atomics are exact in any order
        A, B, bias, _ = G.nt_inputs(fam, 264, 136, 12320, 0, DEV, f32_codes=True)
        exact = G.nt_exact(fam, 264, 136, 12320, f32_codes=True, device=DEV) - (0.0 if bias is None else bias[None, :])
        assert torch.equal(kernels.weight_grad_nt(A.to(BF16), B.to(BF16)), exact), fam


def test_two_level_batch_in_the_poison_layout():
    """batch1 = 2, batch2 = 3 with independent strides (B indexed by batch2 only: sB1 = 0), alpha = 0.125, (300, 264, 96):
    t256 = 6 * 2 * 2 = 24 < 192, t128 = 6 * 3 * 2 = 36 < 128 -> <2,1>.  NaN between the batches of A and B, sentinel between those of C."""
    M, N, K, b1, b2 = 300, 264, 96, 2, 3
    for fam in G.FAMILIES:
        for f32 in (False, True):
            A = torch.stack([torch.stack([G.nt_inputs(fam, M, N, K, 10 * i + j, DEV)[0] for j in range(b2)]) for i in range(b1)])
            B = torch.stack([G.nt_inputs(fam, M, N, K, 100 + j, DEV)[1] for j in range(b2)])
            Abuf, Av = G.poisoned(A.reshape(b1 * b2, M, K), K + 8, batch_gap=5)
            Bbuf, Bv = G.poisoned(B, K + 24, batch_gap=2)
            Cbuf = torch.full((b1 * b2, M + 6 + 3, N + 8), G.SENTINEL, dtype=torch.float32 if f32 else BF16, device=DEV)
            C = Cbuf[:, 3:3 + M, :N]
            sA, sB, sC = Abuf.stride(0), Bbuf.stride(0), Cbuf.stride(0)
            _gemm(Av, Bv, C, alpha=0.125, batch=(b1, b2 * sA, 0, b2 * sC, b2, sA, sB, sC))
            torch.cuda.synchronize()
            assert G.sentinel_intact(Cbuf, C, 3)
            _judge("g21_batch2x3" + ("_f32" if f32 else ""), fam, A, B[None], [{"out": C.reshape(b1, b2, M, N)}], out_f32=f32, alpha=0.125)
    # placement of every (batch1, batch2, m, n): batch (i, j) takes A's rows rolled by 5 (3 i + j) and B's rows rolled by 7 j, so each of the
    # six results is a different roll of the exact one (times alpha = 0.125: a power of two, still exact)
    for fam in G.EXACT_FAMILIES:
        for f32 in (False, True):
            A0, B0, bias, _ = G.nt_inputs(fam, M, N, K, 0, DEV, f32_codes=f32)
            exact = G.nt_exact(fam, M, N, K, f32_codes=f32, device=DEV) - (0.0 if bias is None else bias[None, :])
            A = torch.stack([torch.roll(A0, -5 * (b2 * i + j), 0) for i in range(b1) for j in range(b2)])
            B = torch.stack([torch.roll(B0, -7 * j, 0) for j in range(b2)])
            want = torch.stack([torch.roll(exact, (-5 * (b2 * i + j), -7 * j), (0, 1)) for i in range(b1) for j in range(b2)]) * 0.125
            Abuf, Av = G.poisoned(A, K + 8, batch_gap=5)
            Bbuf, Bv = G.poisoned(B, K + 24, batch_gap=2)
            Cbuf = torch.full((b1 * b2, M + 6 + 3, N + 8), G.SENTINEL, dtype=torch.float32 if f32 else BF16, device=DEV)
            C = Cbuf[:, 3:3 + M, :N]
            sA, sB, sC = Abuf.stride(0), Bbuf.stride(0), Cbuf.stride(0)
            _gemm(Av, Bv, C, alpha=0.125, batch=(b1, b2 * sA, 0, b2 * sC, b2, sA, sB, sC))
            torch.cuda.synchronize()
            assert G.sentinel_intact(Cbuf, C, 3)
            assert torch.equal(C.float(), want), (fam, f32)


# ---- gemm8.hip: M % 256 == 0, N % 256 == 0, K % 128 == 0, K >= 128, M >= 4096, batch 1, bf16 output, 16-byte aligned, recipe in the switch -----------
@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_gemm8_recipes_and_the_general_kernel_on_the_same_operands(recipe):
    """(4096, 512, 256): 16 x 2 tiles on 32 workgroups.  The general kernel is reached with M + 8 rows (4104 % 256 != 0; t256 = 17 * 2 -> <2,1>);
    the two may differ only where the bounds allow."""
    M, N, K = 4096, 512, 256
    for fam in G.FAMILIES:
        inputs = G.nt_inputs(fam, M + 8, N, K, 7, DEV)
        fast, (A, B), args = _run_recipe("g8_" + recipe, fam, M + 8, N, K, recipe, rows=M, inputs=inputs, judge=False)
        gen, _, _ = _run_recipe("g21_" + recipe, fam, M + 8, N, K, recipe, inputs=inputs)
        _judge("g8_" + recipe, fam, A, B, [fast, {k: v[:M] for k, v in gen.items()}], cross=True, **args)


@pytest.mark.parametrize("recipe", ["radd", "bias_radd"])
def test_gemm8_in_place_residual(recipe):
    """C is R (kernels.FanInFn adds data gradients onto one buffer): bit for bit the out-of-place result."""
    M, N, K = 4096, 512, 256
    for fam in G.FAMILIES + ("onehot_k",):
        A, B, bias, R = G.nt_inputs(fam, M, N, K, 9, DEV)
        bias = bias if RECIPES[recipe].get("bias") else None
        if fam == "onehot_k":                                            # the residual: a column code that keeps the sum an integer <= 255
            R = torch.zeros((M, N), device=DEV) + (torch.arange(N, device=DEV) % 2).float()[None, :]
        Ab, Bb, Rb = A.to(BF16), B.to(BF16), R.to(BF16)
        out = _gemm(Ab, Bb, torch.empty((M, N), dtype=BF16, device=DEV), bias=bias, R=Rb)
        acc = Rb.clone()
        _gemm(Ab, Bb, acc, bias=bias, R=acc)
        torch.cuda.synchronize()
        assert torch.equal(out, acc), (recipe, fam)
        if fam == "onehot_k":
            exact = G.nt_exact(fam, M, N, K, device=DEV) - (0.0 if bias is not None else (torch.arange(N, device=DEV) % 5).float()[None, :]) + R
            assert torch.equal(acc.float(), exact), recipe
            continue
        _judge("g8_inplace_" + recipe, fam, A, B, [{"out": acc}], bias=bias, R=R)


def test_gemm8_minimum_k_and_exact_families():
    """K = 128: two K-tiles of 64, the minimum; (4096, 256, 128) through kernels.matmul_nt / the strided helper."""
    from emdr2_amd.model import kernels
    M, N, K = 4096, 256, 128
    for fam in G.FAMILIES:
        A, B, _, _ = G.nt_inputs(fam, M, N, K, 7, DEV)
        C = kernels.matmul_nt(A.to(BF16), B.to(BF16))
        torch.cuda.synchronize()
        _judge("g8_k128", fam, A, B, [{"out": C}])
        _run_recipe("g8_k128_bias_gelu_preg", fam, M, N, K, "bias_gelu_preg")
    for shape in ((4096, 256, 128), (4096, 512, 256)):
        for fam in G.EXACT_FAMILIES:
            A, B, bias, _ = G.nt_inputs(fam, *shape, 0, DEV)
            gots, _, _ = _run_recipe("g8_exact", fam, *shape, dict(bias=1) if bias is not None else dict(), inputs=(A, B, bias, None), judge=False)
            assert torch.equal(gots["out"].float(), G.nt_exact(fam, *shape, device=DEV)), (shape, fam)


@pytest.mark.parametrize("recipe", ["plain", "bias_drop_radd", "bias_gelu_pre", "bias_gelu_preg"])
def test_gemm8_strided_poisoned(recipe):
    """lda = K + 8, ldb = K + 16, ldc = N + 8 (what the packed QKV slices of the step look like), NaN / sentinel all around."""
    for fam in G.FAMILIES:
        _run_recipe("g8_strided_" + recipe, fam, 4096, 512, 256, recipe, poison=True)
    if recipe == "plain":
        _exact("g8_strided", 4096, 512, 256)                             # bf16: gemm8; fp32 output: the general kernel on the same strided operands


@pytest.mark.parametrize("fam", ["row_scaled", "onehot_k"])
def test_gemm8_tile_seams_and_two_n_groups(fam):
    """(8192, 2816, 768): 32 x 11 = 352 tiles on 256 workgroups (seams); panel 384 KiB -> ng = 6, N K 2 = 4.1 MiB > 4 MiB -> groups of 6 + 5."""
    M, N, K = 8192, 2816, 768
    if fam == "onehot_k":
        A, B, bias, _ = G.nt_inputs(fam, M, N, K, 0, DEV)
        gots, _, _ = _run_recipe("g8_seams", fam, M, N, K, dict(bias=1), inputs=(A, B, bias, None), judge=False)
        assert torch.equal(gots["out"].float(), G.nt_exact(fam, M, N, K, device=DEV))
    else:
        _run_recipe("g8_seams", fam, M, N, K, "bias_radd")


def test_dropout_keep_pattern_is_that_of_emdr2_dropout():
    """G8_BIAS | G8_DROP | G8_RADD with R = 0 and strictly positive operands: the zeros of the output are exactly the zeros of emdr2_dropout's
    mask for the same seed -- persistent kernel, general vector epilogue, general scalar epilogue (ldc = N + 1)."""
    N, K, p = 512, 128, 0.1
    gen = torch.Generator(device=DEV).manual_seed(4)
    for path, M, ldc in (("g8", 4096, N), ("general_vector", 1000, N), ("general_scalar", 1000, N + 1)):
        A = (torch.rand((M, K), generator=gen, device=DEV) + 0.1).to(BF16)
        B = (torch.rand((N, K), generator=gen, device=DEV) + 0.1).to(BF16)
        bias = torch.rand(N, generator=gen, device=DEV) + 0.1
        R = torch.zeros((M, ldc), dtype=BF16, device=DEV)[:, :N]
        C = torch.zeros((M, ldc), dtype=BF16, device=DEV)[:, :N]
        _gemm(A, B, C, bias=bias, R=R, drop_p=p, seed=SEED)
        torch.cuda.synchronize()
        mask = _drop_mask(M, N, p, SEED)
        assert torch.equal(C == 0, mask == 0), path
        assert abs(float((mask == 0).double().mean()) - p) < 5e-3


# ---- the LSE epilogue ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,V,H", [(256, 512, 256), (512, 1024, 128)])
@pytest.mark.parametrize("fam", ["row_scaled", "smooth"])
def test_lse_epilogue(fam, M, V, H):
    """kernels.lm_head_gold_logprob takes M % 256 == 0, V % 256 == 0, H % 128 == 0 to emdr2_gemm_nt_lse_bf16; logits span +-300; labels on
    both sides of every 16-, 64- and 256-column boundary, and -100, V, V + 7."""
    from emdr2_amd.model import kernels
    A, B, bias, labels = G.lse_inputs(fam, M, V, H, 5, DEV)
    W, bp = torch.nn.Parameter(B.clone()), torch.nn.Parameter(bias.clone())
    with torch.no_grad():
        fused = kernels.lm_head_gold_logprob(A.to(BF16), W, bp, labels)
        unfused = kernels.lse_gather(kernels.linear(A.to(BF16), W, bp), labels)
    torch.cuda.synchronize()
    r = G.lse_nt_reference(A, B, 1.0, bias, labels)
    assert float(r.logits.abs().max()) > 200.0
    bd = G.lse_nt_bounds(r)["gold"]
    for name, got in (("fused", fused), ("unfused", unfused)):
        ratio, idx = G.worst(got, r.gold, bd)
        _note("lse_%dx%dx%d_%s" % (M, V, H, name), fam, "gold", ratio)
        assert ratio <= 1.0, (name, ratio, idx)
    d = float((fused - unfused).abs().max())
    print("fused - unfused: %.3g" % d)
    assert d <= 2e-4


# ---- TN: gemm8t.hip (R % 64 == 0) and gemm_tn.hip (R % 64 == 32) ----------------------------------------------------------------------------
def _tn(A, B, C, split, colsum):
    nat, lib = _lib()
    R, I = A.shape
    nat.check(lib.emdr2_gemm_tn_bf16(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0), I, B.shape[1], R, split,
                                     _ptr(colsum), nat.stream_ptr()), "gemm_tn_bf16")


@pytest.mark.parametrize("R", [128, 2112, 96, 2080])
@pytest.mark.parametrize("split", [1, 7])
def test_tn_kernels_in_the_poison_layout(R, split):
    """R = 128, 2112 (multiples of 64) -> gemm8t (2 and 33 K-tiles; 7 slices are capped at 2 for R = 128); R = 96, 2080 (R % 64 == 32) ->
    gemm_tn (3 and 65 chunks; split 7 of 3 chunks: per = 1, four EMPTY slices).  I, J: ragged multiples of 8 -- 8 (one granule), 264 (a
    second tile 8 wide), 520 (a third)."""
    path = ("gemm8t" if R % 64 == 0 else "gemm_tn") + "_R%d_s%d" % (R, split)
    for I, J in ((8, 520), (264, 264), (520, 8), (264, 520)):
        for fam in ("onehot_k", "row_scaled", "cancel"):
            for with_colsum in (False, True):
                A, B = G.tn_inputs(fam, R, I, J, 3, DEV)
                _, Av = G.poisoned(A, I + 8)
                _, Bv = G.poisoned(B, J + 16)
                Cbuf = torch.full((1, I + 6, J + 3), G.SENTINEL, dtype=torch.float32, device=DEV)
                C = Cbuf[0, 3:3 + I, :J]
                if split > 1:
                    C.zero_()
                csbuf = torch.full((1, 1, I + 16), G.SENTINEL, dtype=torch.float32, device=DEV)
                cs = csbuf[0, 0, 8:8 + I]
                cs.zero_()
                _tn(Av, Bv, C, split, cs if with_colsum else None)
                torch.cuda.synchronize()
                assert G.sentinel_intact(Cbuf, C, 3), (path, I, J, fam)
                csb = csbuf.clone()
                csb[0, 0, 8:8 + I] = G.SENTINEL
                assert bool((csb == G.SENTINEL).all()), (path, I, J, fam, "colsum written outside its window")
                r = G.tn_reference(A, B)
                if fam == "onehot_k":
                    assert torch.equal(C, r.dW.float()), (path, I, J)
                    assert torch.equal(cs, r.colsum.float() if with_colsum else torch.zeros_like(cs)), (path, I, J)
                    continue
                bd = G.tn_bounds(r, split)
                ratio, idx = G.worst(C, r.dW, bd["dW"])
                _note(path, fam, "dW", ratio)
                assert ratio <= 1.0, (path, I, J, fam, ratio, idx)
                if with_colsum:
                    ratio, idx = G.worst(cs, r.colsum, bd["colsum"])
                    _note(path, fam, "colsum", ratio)
                    assert ratio <= 1.0, (path, I, J, fam, ratio, idx)
                else:
                    assert not bool(cs.any())


def test_second_device_gets_its_own_lds_opt_in():
    """The dynamic-LDS opt-in of a kernel belongs to (function, device) (csrc/device_attr.h).  One process, the last device first and device 0
    after it: a flag kept per process would launch the 160 KiB kernels on device 0 without the opt-in.  gemm8 (4096, 256, 128) with a bias and
    gemm8t (R 128, I = J = 264, one slice), through emdr2_gemm_nt_bf16 / emdr2_gemm_tn_bf16."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    for dev in (torch.cuda.device_count() - 1, 0):
        with torch.cuda.device(dev):
            for fam in ("randn", "row_scaled"):
                _run_recipe("g8_dev%d" % dev, fam, 4096, 256, 128, "bias")
                A, B = G.tn_inputs(fam, 128, 264, 264, 3, DEV)
                C = torch.full((264, 264), G.SENTINEL, dtype=torch.float32, device=DEV)
                _tn(A.to(BF16), B.to(BF16), C, 1, None)
                torch.cuda.synchronize()
                r = G.tn_reference(A, B)
                ratio, idx = G.worst(C, r.dW, G.tn_bounds(r, 1)["dW"])
                _note("gemm8t_dev%d" % dev, fam, "dW", ratio)
                assert ratio <= 1.0, (dev, fam, ratio, idx)


@pytest.mark.parametrize("R", [8256, 8224])
def test_weight_grad_tn_splits_the_reduction(R):
    """kernels.weight_grad_tn: tiles = 2 * 1, split = min(256, R // 4096) = 2.  R = 8256 = 129 * 64 -> gemm8t, R = 8224 (% 64 == 32) -> gemm_tn."""
    from emdr2_amd.model import kernels
    for fam in ("randn", "row_scaled", "cancel", "smooth"):
        A, B = G.tn_inputs(fam, R, 264, 136, 3, DEV)
        cs = torch.zeros(264, device=DEV)
        C = kernels.weight_grad_tn(A.to(BF16), B.to(BF16), colsum=cs)
        torch.cuda.synchronize()
        r = G.tn_reference(A, B)
        bd = G.tn_bounds(r, 2)
        for name, got in (("dW", C), ("colsum", cs)):
            ratio, idx = G.worst(got, getattr(r, name), bd[name])
            _note("weight_grad_tn_R%d" % R, fam, name, ratio)
            assert ratio <= 1.0, (R, fam, name, ratio, idx)
