// emdr2_amd/csrc/prims.h -- what every kernel family states the same way: bf16 <-> fp32, the packed bf16 pair, streaming 16-byte accesses,
// wave reductions, a product that stays rounded, and the launch check of the C entries.  Included by gemm_common.h, attention_common.h and
// the row-kernel sources; one name per function, no aliases.
#ifndef EMDR2_PRIMS_H
#define EMDR2_PRIMS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

// what an exported entry returns after its last launch (-3: the launch itself was rejected)
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? 0 : -3)

// one launch on `stream` (the void * of the C ABI); every argument is converted to the kernel's own parameter type, so an entry passes its
// ABI types (void * for bf16 rows, int64_t counts) as they are
template <typename... P, typename... A>
static inline void launch(void (*kernel)(P...), dim3 grid, unsigned block, void *stream, A... args)
{
    hipLaunchKernelGGL(kernel, grid, dim3(block), 0, (hipStream_t)stream, (P)args...);
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float floatx2_t __attribute__((ext_vector_type(2)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const void gptr_t;
typedef __attribute__((address_space(3))) void lptr_t;
#define TR_READ(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))

__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
// software round to nearest even, quiet NaN
__device__ __forceinline__ uint16_t f2bf(float f)
{
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }            // the two bf16 of a packed pair
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
// two fp32 -> packed bf16 pair with the hardware converter (v_cvt_pk_bf16_f32, round to nearest even, NaN preserved)
__device__ __forceinline__ uint32_t pack_bf16(float a, float b)
{
    const floatx2_t v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}

// 16 bytes that are touched once per launch (LayerNorm rows: 2 GB each at the reader's shape; GEMM outputs): non-temporal, so that they
// stay out of the way of what the neighbouring tiles and kernels want to find in L2
__device__ __forceinline__ uint4 ld_stream(const uint16_t *p)
{
    const u32x4_t t = __builtin_nontemporal_load((const u32x4_t *)p);
    return make_uint4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ void st_stream(uint16_t *p, uint4 v)
{
    const u32x4_t t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, (u32x4_t *)p);
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// a product that is rounded where it stands: never fused into an addition that consumes it
__device__ __forceinline__ float mul_rounded(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
#endif
