// emdr2_amd/csrc/gemm_common.h -- what the bf16 GEMM kernels (gemm.hip, gemm8.hip, gemm_tn.hip, gemm8t.hip) share beside prims.h: the erf-form
// GELU of the reference (transformer.py:80,103-104: F.gelu, not the tanh fusion) and its derivative, the element recipe of
// the NT epilogues, the XCD-contiguous item mapping, and the barrier / transposed-read macros of the 256 x 256 pipelines.
#ifndef EMDR2_GEMM_COMMON_H
#define EMDR2_GEMM_COMMON_H
#include "prims.h"
#include "rng.h"

typedef float floatx4 __attribute__((ext_vector_type(4)));

// erf-form GELU 0.5 x (1 + erf(x / sqrt 2)).  erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7, far below the bf16 output grid) on one
// v_rcp and one v_exp; the library erff costs ~3x.  With erf(|z|) = 1 - P(t) exp(-z^2), t = 1 / (1 + p |z|), both signs of x collapse into
//   gelu(x) = max(x, 0) - |x| * (P(t) / 2) * exp(-x^2 / 2)
// (x >= 0: x - x P e / 2;  x < 0: x P e / 2): 11 full-rate VALU ops (|x| and the negations ride as source modifiers), the 1/2 folded into the
// polynomial's coefficients, exp(-x^2 / 2) = exp2(-(x sqrt(log2(e) / 2))^2).
__device__ __forceinline__ float gelu_half_poly_exp(float x, float &e)
{
    const float t = __builtin_amdgcn_rcpf(fmaf(fabsf(x), 0.3275911f * 0.70710678118654752f, 1.0f));
    const float w = x * 0.84932180028801904f;                                      // sqrt(log2(e) / 2)
    e = __builtin_amdgcn_exp2f(-(w * w));                                          // exp(-x^2 / 2)
    return t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 0.5f * 1.061405429f, 0.5f * -1.453152027f), 0.5f * 1.421413741f), 0.5f * -0.284496736f), 0.5f * 0.254829592f);
}
__device__ __forceinline__ float gelu_erf(float x)
{
    float e;
    const float hp = gelu_half_poly_exp(x, e);
    return fmaf(-fabsf(x), hp * e, fmaxf(x, 0.0f));
}
// step(x) of the derivative, keyed on the SIGN BIT like the copysign beside it: with x >= 0.0f, x = -0.0 took +P(t) / 2 AND the step,
// gelu'(-0.0) = 1.5 instead of 0.5 (a bf16 pre-activation that underflowed from below is -0.0)
__device__ __forceinline__ float gelu_step(float x) { return (int32_t)__float_as_uint(x) >= 0 ? 1.0f : 0.0f; }
// both at once (one rcp, one exp2, one polynomial): the activation and its derivative of the same pre-activation
__device__ __forceinline__ float gelu_erf_with_grad(float x, float &grad)
{
    float e;
    const float hp = gelu_half_poly_exp(x, e);
    grad = fmaf(e, fmaf(x, 0.3989422804014327f, -copysignf(hp, x)), gelu_step(x));
    return fmaf(-fabsf(x), hp * e, fmaxf(x, 0.0f));
}
// d/dx of the erf-form GELU: Phi(x) + x phi(x) = step(x) + exp(-x^2 / 2) (x / sqrt(2 pi) - sign(x) P(t) / 2), same erf approximation and
// the same exponential as the forward
__device__ __forceinline__ float gelu_erf_grad(float x)
{
    float e;
    const float hp = gelu_half_poly_exp(x, e);
    return fmaf(e, fmaf(x, 0.3989422804014327f, -copysignf(hp, x)), gelu_step(x));
}

// ---- the element recipe of the NT epilogues (order of roundings): what gemm.hip's vector and scalar epilogues and gemm8.hip
// share beside gelu_erf / gelu_erf_with_grad above; each keeps its own staging, dropout form and branches on the output mode.
__device__ __forceinline__ float epi_affine(float acc, float alpha, float bias) { return fmaf(acc, alpha, bias); }
// the value meets the residual as the bf16 the reference's F.linear would have stored: one rounding before the combine, one after
__device__ __forceinline__ float round_to_stored_bf16(float v) { return bf2f(f2bf(v)); }
// one packed bf16 pair of the residual.  rmode 0: + r;  1: * gelu'(r) -- r is the saved GELU pre-activation (backward of the FFN's first
// linear, fused);  2: * r.  A run-time rmode costs a uniform branch per pair (and keeps the pair in packed math), a constant folds.
__device__ __forceinline__ floatx2_t epi_residual_pair(floatx2_t x, uint32_t rw, int rmode)
{
    const floatx2_t r = {bf_lo(rw), bf_hi(rw)};
    if (rmode == 0) return x + r;
    if (rmode == 2) return x * r;
    const floatx2_t g = {gelu_erf_grad(r[0]), gelu_erf_grad(r[1])};
    return x * g;
}

// ---- XCD-contiguous item mapping.  Workgroup ids go round-robin to the 8 XCDs (one L2 each); XCD x = id & 7 owns the items
// [x * per, (x + 1) * per) of a sequence, so that consecutive items -- which share operand panels -- run on one L2.  Grids are 8 * per wide.
__host__ __device__ __forceinline__ int xcd_per(int total) { return (total + 7) >> 3; }
// this workgroup's item of a one-item-per-workgroup launch; false: none (ragged tail of the last XCD ranges)
__device__ __forceinline__ bool xcd_item(int total, int &item)
{
    item = ((int)blockIdx.x & 7) * xcd_per(total) + ((int)blockIdx.x >> 3);
    return item < total;
}
// TN kernels: item -> (reduction slice, tile) with the tile index fastest, so the `tiles` workgroups that stream the SAME token rows of dy and x
// run together on one L2 and both operands leave HBM once per slice; tiles are i-fastest
__device__ __forceinline__ void tn_item_coords(int item, int tiles, int tiles_i, int &zs, int &ti, int &tj)
{
    zs = item / tiles;
    const int tile = item - zs * tiles;
    tj = tile / tiles_i; ti = tile - tj * tiles_i;
}

// ---- ds_read_b64_tr_b16 as inline asm (the builtin makes the wait-count pass put vmcnt(0) in front of every read: gemm8t.hip), and the bf16x8
// MFMA operand of two such 8-byte halves
#define TR_FRAG(L, H) __builtin_bit_cast(bf16x8, make_uint4((L).x, (L).y, (H).x, (H).y))

// ---- phase boundary of the 256 x 256 pipelines (gemm8.hip, gemm8t.hip): wait for this phase's DMA, meet, wait for its LDS reads, MFMAs at
// raised priority; the scheduling barriers keep the compiler from moving anything across
#define PIPE_BARRIER()                                                                                                                    \
    __builtin_amdgcn_s_barrier();                                                                                                         \
    __builtin_amdgcn_sched_barrier(0)
#define PIPE_SYNC_COMPUTE(VM_WAIT, LDS_WAIT, MFMAS)                                                                                       \
    VM_WAIT;                                                                                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                                                                    \
    __builtin_amdgcn_s_barrier();                                                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                                                                    \
    LDS_WAIT;                                                                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                                                                    \
    __builtin_amdgcn_s_setprio(1);                                                                                                        \
    MFMAS;                                                                                                                                \
    __builtin_amdgcn_s_setprio(0);                                                                                                        \
    __builtin_amdgcn_sched_barrier(0)
#endif
