// emdr2_amd/csrc/mips_audit.hip -- emdr2_mips_audit: one pass over a shard's live images that re-checks what the search's proof takes for
// granted (the report words are documented in include/emdr2_mips.h).
//
// One workgroup per 256-row block of the padded image, three steps on that block:
//   1. SOUND.  The block's two stripes are streamed from HBM in storage order -- chunk after chunk, a wave reading 1 KiB of consecutive
//      16-byte slots of an 8 KiB block, like digest_rows_kernel -- and every row's ||e_r||^2 and, with a shadow, ||e_r - s_b e8_r||^2 are
//      summed in float64 from the stored bits: the fp16 value widened exactly, the int8 byte as stored, s_b the stored float widened
//      exactly.  Nothing of the seal's or the norm routine's fp32 arithmetic is used, and no tolerance is added: the square of an fp16 value
//      is exact in float64 and the sum of 8,192 of them is off by ~1e-12 relative, nine orders below the 0.1 % slack every stored bound
//      carries.  Four lanes share a row (the four 16-byte slots of its 64 bytes in a chunk) and fold their sums once per stripe.
//   2. CANONICAL, norms.  block_norm_256 (mips_derived.h) -- the routine behind block_norms_kernel -- with a comparing sink: the value goes
//      against the table entry's bits, and into the running maximum that audit_finish_kernel compares with *emax_sq.
//   3. CANONICAL, shadow.  seal_block_256 -- the routine behind seal_shadow_kernel -- with a comparing sink: every 16-byte int8 group against
//      the stored one, {s_b, N_b, D_b} against the table entry.
// Steps 2 and 3 re-read the block the workgroup has just streamed (393 KB + 196 KB at dim 768): out of the caches -- L2, or the Infinity
// Cache behind it when all resident workgroups' blocks together outgrow an XCD's 4 MB -- as the seal's own second pass does; HBM is read once.  Offenders are tallied in
// LDS (a clean image issues no atomic but the row count) and flushed with integer atomics: 64-bit adds for the counters, atomicMin for
// the first offenders.
#include "mips_derived.h"

namespace {

enum {
    W_ROWS = 0, W_PAD = 1, W_NONFINITE = 2, W_OVER_EMAX = 3, W_NORM_LOW = 4, W_NORM_NONCANON = 5, W_EMAX_NONCANON = 6, W_SPAD = 7,
    W_SNORM_LOW = 8, W_SRESID_LOW = 9, W_SROWS_NONCANON = 10, W_STABLE_NONCANON = 11, W_FIRST_ROW = 12, W_FIRST_BLOCK = 13,
    W_EMAX_SCRATCH = 14,                                        // running max of the block norms between the two launches; left 0
    N_TALLY = 12
};

struct AuditShared {
    float red[4];
    unsigned tally[N_TALLY];
    unsigned first_row;                                         // local row; 0xffffffff = none
    unsigned block_bad;                                         // the block is counted in word 5 or 11
};

// eight fp16 values of one 16-byte slot: float64 sum of squares, any bit set, any inf / NaN
__device__ __forceinline__ void audit_slot(uint4 v, double &n2, unsigned &any, unsigned &nf)
{
    const half8 h = __builtin_bit_cast(half8, v);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        any |= w[j];
        nf |= (unsigned)((w[j] & 0x7c00u) == 0x7c00u) | (unsigned)((w[j] & 0x7c000000u) == 0x7c000000u);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { const double x = (double)(float)h[j]; n2 += x * x; }
}

// the same plus the residual against the eight int8 bytes (lo = elements 0..3, hi = 4..7) under the stored scale
__device__ __forceinline__ void audit_slot8(uint4 v, unsigned lo, unsigned hi, double s, double &n2, double &d2, unsigned &any, unsigned &nf)
{
    audit_slot(v, n2, any, nf);
    const half8 h = __builtin_bit_cast(half8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int q = (int)(signed char)(((j < 4 ? lo : hi) >> (8 * (j & 3))) & 255u);
        const double r = (double)(float)h[j] - s * (double)q;
        d2 += r * r;
    }
}

__device__ __forceinline__ double quad_sum(double v) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); return v; }
__device__ __forceinline__ unsigned quad_or(unsigned v) { v |= (unsigned)__shfl_xor((int)v, 1); v |= (unsigned)__shfl_xor((int)v, 2); return v; }

struct CompareBlockNorm {
    const float *block_norm_sq;                                 // may be null: only the running maximum
    unsigned *emax_scratch;
    AuditShared *sh;
    __device__ __forceinline__ void block_norm(int64_t block, float v) const
    {
        if (block_norm_sq && __float_as_uint(block_norm_sq[block]) != __float_as_uint(v)) { sh->tally[W_NORM_NONCANON] = 1u; sh->block_bad = 1u; }
        if (v > 0.f) atomicMax(emax_scratch, __float_as_uint(v));          // non-negative floats order as uints
    }
};

struct CompareSeal {
    const char *e8;
    const float4 *blk;
    AuditShared *sh;
    unsigned differs;
    __device__ __forceinline__ void nonfinite() const {}        // (counted per row by the sound pass)
    __device__ __forceinline__ void int8_group(int64_t row, int g, int nch8, uint4 v)
    {
        const uint4 st = *(const uint4 *)(e8 + tiled_seg_offset(row, g, nch8));
        differs |= (st.x ^ v.x) | (st.y ^ v.y) | (st.z ^ v.z) | (st.w ^ v.w);
    }
    __device__ __forceinline__ void row_done(int64_t row) const
    {
        if (differs) { atomicAdd(&sh->tally[W_SROWS_NONCANON], 1u); atomicMin(&sh->first_row, (unsigned)(row & 0xffffffff)); }
    }
    __device__ __forceinline__ void block_consts(int64_t block, float4 v) const
    {
        const float4 st = blk[block];
        if (__float_as_uint(st.x) != __float_as_uint(v.x) || __float_as_uint(st.y) != __float_as_uint(v.y) || __float_as_uint(st.z) != __float_as_uint(v.z)) {
            sh->tally[W_STABLE_NONCANON] = 1u;
            sh->block_bad = 1u;
        }
    }
};

__global__ void __launch_bounds__(64) audit_init_kernel(unsigned long long *report)
{
    if (threadIdx.x < 16) report[threadIdx.x] = (threadIdx.x == W_FIRST_ROW || threadIdx.x == W_FIRST_BLOCK) ? ~0ull : 0ull;
}

__global__ void __launch_bounds__(64) audit_finish_kernel(const float *__restrict__ emax_sq, unsigned long long *report)
{
    if (threadIdx.x == 0) {
        report[W_EMAX_NONCANON] = ((unsigned)report[W_EMAX_SCRATCH] != __float_as_uint(*emax_sq)) ? 1ull : 0ull;
        report[W_EMAX_SCRATCH] = 0ull;
    }
}

__global__ void __launch_bounds__(256) audit_kernel(AuditParams p)
{
    __shared__ AuditShared sh;
    const int tid = threadIdx.x;
    const int64_t block = blockIdx.x;
    if (tid < N_TALLY) sh.tally[tid] = 0u;
    if (tid == 0) { sh.first_row = 0xffffffffu; sh.block_bad = 0u; }
    __syncthreads();

    const int nch = p.nch, nch8 = nch >> 1;
    const bool sealed = p.e8 && block < p.sealed_blocks;           // (uniform; the seal covers the blocks that hold a row of the shard)
    float4 bc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (sealed) bc = p.table[block];
    const double s_b = (double)bc.x, n_b = (double)bc.y, d_b = (double)bc.z;
    const double emax_bound = (double)(sqrtf(*p.emax_sq) * 1.001f);  // the bound as finalize_kernel forms it, in float
    const double norm_bound = p.block_norm_sq ? (double)p.block_norm_sq[block] * (1.001 * 1.001) : 0.0;

    // ---- 1. sound: float64 from the stored bits, storage order ----
    const int ri = tid >> 2, sp = tid & 3, s = sp ^ ((ri >> 2) & 3);  // this thread's slot of a chunk: row ri (and 64 + ri: same swizzle), group s
    for (int half = 0; half < 2; ++half) {
        const int64_t row0 = block * 256 + half * 128 + ri;
        double n2[2] = {0.0, 0.0}, d2[2] = {0.0, 0.0};
        unsigned any[2] = {0u, 0u}, any8[2] = {0u, 0u}, nf[2] = {0u, 0u};
        if (sealed) {
            // int8 group g = 4 c8 + s holds the 16 k-values of the fp16 groups 2 g and 2 g + 1: the four lanes of a row read its 64 int8 bytes
            // of chunk c8 and its 64 fp16 bytes of each of the chunks 2 c8 and 2 c8 + 1
#pragma unroll 2
            for (int c8 = 0; c8 < nch8; ++c8) {
                const int g = c8 * 4 + s;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int64_t row = row0 + 64 * k;
                    const uint4 q = *(const uint4 *)(p.e8 + tiled_seg_offset(row, g, nch8));
                    const uint4 a = *(const uint4 *)(p.tiled + tiled_seg_offset(row, 2 * g, nch));
                    const uint4 b = *(const uint4 *)(p.tiled + tiled_seg_offset(row, 2 * g + 1, nch));
                    any8[k] |= q.x | q.y | q.z | q.w;
                    audit_slot8(a, q.x, q.y, s_b, n2[k], d2[k], any[k], nf[k]);
                    audit_slot8(b, q.z, q.w, s_b, n2[k], d2[k], any[k], nf[k]);
                }
            }
        } else {
#pragma unroll 2
            for (int c = 0; c < nch; ++c) {
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    audit_slot(*(const uint4 *)(p.tiled + tiled_seg_offset(row0 + 64 * k, c * 4 + s, nch)), n2[k], any[k], nf[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double rn2 = quad_sum(n2[k]), rd2 = quad_sum(d2[k]);
            const unsigned rany = quad_or(any[k]), rany8 = quad_or(any8[k]), rnf = quad_or(nf[k]);
            if (sp != 0) continue;
            const int64_t row = row0 + 64 * k;
            bool bad = false;
            if (row >= p.n_rows) {                                 // the zero padding
                if (rany) { atomicAdd(&sh.tally[W_PAD], 1u); bad = true; }
                if (rany8) { atomicAdd(&sh.tally[W_SPAD], 1u); bad = true; }
            } else if (rnf) {
                atomicAdd(&sh.tally[W_NONFINITE], 1u); bad = true;
            } else {
                const double norm = sqrt(rn2);
                if (norm > emax_bound) { atomicAdd(&sh.tally[W_OVER_EMAX], 1u); bad = true; }
                if (p.block_norm_sq && rn2 > norm_bound) { atomicAdd(&sh.tally[W_NORM_LOW], 1u); bad = true; }
                if (sealed) {
                    if (norm > n_b) { atomicAdd(&sh.tally[W_SNORM_LOW], 1u); bad = true; }
                    if (sqrt(rd2) > d_b) { atomicAdd(&sh.tally[W_SRESID_LOW], 1u); bad = true; }
                }
            }
            if (bad) atomicMin(&sh.first_row, (unsigned)row);
        }
    }
    __syncthreads();

    // ---- 2. and 3. canonical: the project's own routines, comparing instead of storing ----
    CompareBlockNorm norm_sink{p.block_norm_sq, (unsigned *)(p.report + W_EMAX_SCRATCH), &sh};
    block_norm_256(p.tiled, nch * 4, block, sh.red, norm_sink);
    if (sealed) {
        CompareSeal seal_sink{p.e8, p.table, &sh, 0u};
        seal_block_256(p.tiled, nch, block, sh.red, seal_sink);
    }
    __syncthreads();

    if (tid == 0) {
        const int64_t left = p.n_rows - block * 256;
        if (left > 0) atomicAdd(&p.report[W_ROWS], (unsigned long long)(left < 256 ? left : 256));
        if (sh.block_bad) atomicMin(&p.report[W_FIRST_BLOCK], (unsigned long long)block);
        if (sh.first_row != 0xffffffffu) atomicMin(&p.report[W_FIRST_ROW], (unsigned long long)(p.row_base + (int64_t)sh.first_row));
    } else if (tid < N_TALLY && sh.tally[tid]) {
        atomicAdd(&p.report[tid], (unsigned long long)sh.tally[tid]);
    }
}

} // namespace

int mips_launch_audit(const AuditParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(audit_init_kernel, dim3(1), dim3(64), 0, stream, p.report);
    if (p.n_rows > 0) {
        const int64_t blocks = (p.n_rows + 511) / 512 * 2;
        hipLaunchKernelGGL(audit_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
        hipLaunchKernelGGL(audit_finish_kernel, dim3(1), dim3(64), 0, stream, p.emax_sq, p.report);
    }
    return LAUNCH_OK();
}
