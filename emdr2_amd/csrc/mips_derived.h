// emdr2_amd/csrc/mips_derived.h -- the arithmetic of the structures DERIVED from a shard's fp16 image, one routine each: ||E[r]||^2 of a row
// and of a 256-row block (emax_sq, the block-norm table), and the seal of a block of the int8 shadow image with its {s_b, N_b, D_b}.  Every
// routine hands its results to a SINK.  The kernels that build the structures (block_norms_kernel in mips_aux.hip, seal_shadow_kernel in
// mips_scan8i.hip) pass a storing sink; the audit (mips_audit.hip) passes a comparing one, so "bit for bit what a fresh build leaves" is
// checked against the very code that builds, whatever that code becomes later.
#pragma once
#include "mips_device.h"
#include "mips_kernels.h"

// ||E[r]||^2 of one row by one wave, the same value in every lane: lane l takes the 8-element groups l, l + 64, ... in order, then a
// butterfly over the lanes.  emax_sq of a freshly packed shard (row_norm_max_kernel, row-major rows) and of a shard updated in place
// (block_norms_kernel, rows read back from the tiled image) must agree bit for bit -- the search's validity bound reads it -- so both
// kernels go through this one routine and differ only in where a group comes from.  Whether the compiler contracts `s += x * x` into an
// fma in one instance and not in the other cannot matter: the square of an fp16 value has at most 22 significant bits and is exact in
// fp32, so the fma and the multiply-then-add round the same sum.
struct RowMajorRow {
    const uint4 *row;                                           // rows_rm + r * nseg
    __device__ __forceinline__ uint4 operator()(int seg) const { return row[seg]; }
};
struct TiledRow {
    const char *tiled;
    int64_t row;
    int nch;
    __device__ __forceinline__ uint4 operator()(int seg) const { return *(const uint4 *)(tiled + tiled_seg_offset(row, seg, nch)); }
};
template <class Load>
__device__ __forceinline__ float row_norm_sq_wave(const Load &load, int nseg, int lane)
{
    float s = 0.f;
    for (int seg = lane; seg < nseg; seg += 64) {
        const half8 h = __builtin_bit_cast(half8, load(seg));
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float x = (float)h[j]; s += x * x; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// max over the 256 rows of `block` of ||E[r]||^2, read from the tiled image (rows past the end of the shard are zero there, the image is
// padded to 512 rows).  A workgroup of 256 threads, 64 rows per wave; sh: four floats of LDS.  Thread 0 hands the value to sink.block_norm.
struct StoreBlockNorm {
    float *block_norm_sq;
    __device__ __forceinline__ void block_norm(int64_t block, float v) const { block_norm_sq[block] = v; }
};
template <class Sink>
__device__ __forceinline__ void block_norm_256(const char *__restrict__ tiled, int nseg, int64_t block, float *sh, Sink &sink)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float best = 0.f;
#pragma unroll 4                                                 // (four rows' loads in flight; each row's own arithmetic is untouched)
    for (int i = 0; i < 64; ++i) best = fmaxf(best, row_norm_sq_wave(TiledRow{tiled, block * 256 + wave * 64 + i, nseg >> 2}, nseg, lane));
    if (lane == 0) sh[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) sink.block_norm(block, fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])));
}

__device__ __forceinline__ float block_max_256(float v, float *sh)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();                                           // (sh may still be read from the previous reduction)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// The seal of one 256-row block, one thread per row.  Pass 1: max |e| and max ||e_r||^2 of the block; pass 2 (the block is in L2 now):
// quantise with the block's scale, hand the int8 rows to the sink 16 bytes at a time, measure ||e_r - s_b e8_r||.  Rows past the end of the
// shard are zero in the fp16 image and stay zero here.  Nothing of any other block is read.  The sink receives, per thread, the row's int8
// groups in order (int8_group), then row_done once; thread 0 receives the block's {s_b, N_b, D_b} (block_consts); a thread whose row holds an
// inf / NaN calls nonfinite.
struct StoreSeal {
    char *e8;
    float4 *blk;
    unsigned *bad;
    __device__ __forceinline__ void nonfinite() const { atomicOr(bad, 1u); }
    __device__ __forceinline__ void int8_group(int64_t row, int g, int nch8, uint4 v) const { *(uint4 *)(e8 + tiled_seg_offset(row, g, nch8)) = v; }
    __device__ __forceinline__ void row_done(int64_t) const {}
    __device__ __forceinline__ void block_consts(int64_t block, float4 v) const { blk[block] = v; }
};
//
// D_b is a sum of INEXACT fp32 terms, so which of them the compiler fuses into an fma decides its last bits -- and it decides per instance:
// left to it, the storing instance and a comparing one rounded one block of 34 differently (8,492 x 768 rows).  The roundings are therefore written out, and
// contraction is off in this routine: r = fma(-s_b, e8, e) for every element; of each 16-element group the first four squares enter d2 fused,
// d2 = fma(r, r, d2), the other twelve rounded first, d2 += fl(r * r).  That is, bit for bit, what the seal has always stored (the fusion the
// compiler had chosen for the first build of seal_shadow_kernel, in both of its instances), now independent of instance and compiler.  The
// other sums here are exact products (squares of fp16 values, a multiple of 2^-22) and round the same fused or not.
template <class Sink>
__device__ __forceinline__ void seal_block_256(const char *__restrict__ tiled, int nch, int64_t block, float *sh, Sink &sink)
{
#pragma clang fp contract(off)
    const int64_t row = block * 256 + threadIdx.x;
    const int nseg = nch * 4;
    float amax = 0.f, n2 = 0.f;
    bool bad = false;
    for (int seg = 0; seg < nseg; ++seg) {
        const uint4 v = *(const uint4 *)(tiled + tiled_seg_offset(row, seg, nch));
        const half8 h = __builtin_bit_cast(half8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = (float)h[j];
            bad |= !(fabsf(x) <= 65504.f);
            amax = fmaxf(amax, fabsf(x));
            n2 += x * x;
        }
    }
    if (bad) sink.nonfinite();
    amax = block_max_256(amax, sh);
    n2 = block_max_256(n2, sh);
    const float s = amax / 127.f;
    const float inv = s > 0.f ? 127.f / amax : 0.f;
    float d2 = 0.f;
    const int nch8 = nch >> 1;
    for (int g = 0; g < nseg / 2; ++g) {                       // 16 k-values: fp16 groups 2 g, 2 g + 1 -> int8 group g
        unsigned w[4];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const uint4 v = *(const uint4 *)(tiled + tiled_seg_offset(row, 2 * g + hf, nch));
            const half8 h = __builtin_bit_cast(half8, v);
#pragma unroll
            for (int j = 0; j < 8; j += 4) {
                unsigned pk = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float x = (float)h[j + b];
                    const int qv = quant8(x, inv);
                    const float r = __builtin_fmaf(-s, (float)qv, x);
                    if (hf == 0 && j == 0) d2 = __builtin_fmaf(r, r, d2);
                    else d2 += r * r;
                    pk |= ((unsigned)qv & 255u) << (8 * b);
                }
                w[2 * hf + (j >> 2)] = pk;
            }
        }
        sink.int8_group(row, g, nch8, make_uint4(w[0], w[1], w[2], w[3]));
    }
    sink.row_done(row);
    d2 = block_max_256(d2, sh);
    // the residual e - s e8 was evaluated in fp32: each element is off by up to 2^-24 |s e8| + 2^-24 |e - s e8|, which matters exactly when the
    // quantisation is (nearly) exact -- ternary rows have d2 = 0 while 127 * fl(1 / 127) is not 1.  2^-22 N_b covers it.
    const float nb = sqrtf(n2) * 1.001f;
    if (threadIdx.x == 0) sink.block_consts(block, make_float4(s, nb, (sqrtf(d2) + nb * 0x1p-22f) * 1.001f, 0.f));
}
