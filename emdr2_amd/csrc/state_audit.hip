// emdr2_amd/csrc/state_audit.hip -- the audit of one FlatAdam bucket (include/emdr2_ops.h, "State audit"): ONE streaming pass over the fp32
// masters, both Adam moments and the bf16 working copies -- 14 bytes per element, each read once -- that leaves a position-tagged digest of
// the three fp32 arrays (a key per block of 8192 elements, (sum, xor) over the keys) and five counts with their first offenders.  Integer
// arithmetic only: the folds are sums mod 2^64, xors and minima, so the result is the same for every grid, workgroup order and device.
#include "../../include/emdr2_ops.h"
#include "mips_digest.h"

namespace {

constexpr int AUDIT_BLOCK = 8192;                                        // elements per block key: 8 steps of 256 threads x 4 elements
constexpr int AUDIT_GRID_CAP = 1024;                                     // the grid rule of emdr2_sumsq_f32: a function of n alone
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
// TAG_a of the header: "MSTR", "EXPA", "EXPS" in the high word
__device__ constexpr uint64_t AUDIT_TAG[3] = {0x4D535452ull << 32, 0x45585041ull << 32, 0x45585053ull << 32};
// report words (the header fixes them)
enum { W_N = 0, W_COUNT = 1, W_FIRST = 6, W_DIGEST = 11, W_BLOCKS = 17, W_WORDS = 18 };
enum { C_MASTER = 0, C_M = 1, C_V = 2, C_VNEG = 3, C_WORK = 4, N_CHECKS = 5 };

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += shfl_xor_u64(v, o);
    return v;
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const uint64_t w = shfl_xor_u64(v, o); v = w < v ? w : v; }
    return v;
}
__device__ __forceinline__ bool nonfinite(uint32_t w) { return (w & 0x7fffffffu) >= 0x7f800000u; }

// e(p) + e(p + 1) of the two pairs a 16-byte load holds; `tag` = (p + 1) * GOLDEN
__device__ __forceinline__ uint64_t pair_terms(const uint4 w, uint64_t tag)
{
    return digest_mix((((uint64_t)w.y << 32) | w.x) + tag) + digest_mix((((uint64_t)w.w << 32) | w.z) + (tag + GOLDEN));
}

// sets the report before the pass adds to it: counts and digest words 0, first offenders all ones
__global__ void __launch_bounds__(64) state_audit_init_kernel(unsigned long long *report, unsigned long long n, unsigned long long n_blocks)
{
    const int t = threadIdx.x;
    if (t >= W_WORDS) return;
    report[t] = t == W_N ? n : t == W_BLOCKS ? n_blocks : (t >= W_FIRST && t < W_DIGEST) ? ~0ull : 0ull;
}

// Workgroup g takes blocks g, g + grid, ...; thread t of a block's step k holds elements 4 (256 k + t) .. + 3 of the block: one 16-byte
// load of each fp32 array, one 8-byte load of the working copies.  n % 8 == 0, so a 4-element group is inside the bucket or outside it.
__global__ void __launch_bounds__(256) state_audit_kernel(const uint4 *__restrict__ master, const uint4 *__restrict__ m, const uint4 *__restrict__ v,
                                                          const uint2 *__restrict__ work, long long n4, long long n_blocks,
                                                          unsigned long long *block_keys, unsigned long long *report)
{
    __shared__ uint64_t sh[3][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t dsum[3] = {0, 0, 0}, dxor[3] = {0, 0, 0};                  // thread 0: (sum, xor) over this workgroup's keys
    unsigned cnt[N_CHECKS] = {0, 0, 0, 0, 0};
    uint64_t first[N_CHECKS] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
    for (long long j = blockIdx.x; j < n_blocks; j += gridDim.x) {
        uint64_t acc[3] = {0, 0, 0};
        const long long base4 = j * (AUDIT_BLOCK / 4) + tid;
#pragma unroll 2
        for (int k = 0; k < AUDIT_BLOCK / 1024; ++k) {
            const long long i4 = base4 + k * 256;
            if (i4 >= n4) break;
            const uint4 a = master[i4], b = m[i4], c = v[i4];
            const uint2 w = work[i4];
            const uint64_t tag = (uint64_t)(2 * i4 + 1) * GOLDEN;        // pairs 2 i4 and 2 i4 + 1
            acc[0] += pair_terms(a, tag);
            acc[1] += pair_terms(b, tag);
            acc[2] += pair_terms(c, tag);
            const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w}, cw[4] = {c.x, c.y, c.z, c.w};
            const uint32_t want0 = (uint32_t)f2bf(__uint_as_float(a.x)) | ((uint32_t)f2bf(__uint_as_float(a.y)) << 16);
            const uint32_t want1 = (uint32_t)f2bf(__uint_as_float(a.z)) | ((uint32_t)f2bf(__uint_as_float(a.w)) << 16);
            const uint32_t diff[4] = {(want0 ^ w.x) & 0xffffu, (want0 ^ w.x) >> 16, (want1 ^ w.y) & 0xffffu, (want1 ^ w.y) >> 16};
            uint32_t any = (want0 ^ w.x) | (want1 ^ w.y) | ((cw[0] | cw[1] | cw[2] | cw[3]) & 0x80000000u);
#pragma unroll
            for (int e = 0; e < 4; ++e) any |= (uint32_t)nonfinite(aw[e]) | (uint32_t)nonfinite(bw[e]) | (uint32_t)nonfinite(cw[e]);
            if (any) {                                                 // (rare: a sound bucket never enters)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint64_t idx = (uint64_t)(4 * i4 + e);         // ascends per thread: the first hit is the thread's minimum
                    const uint32_t cabs = cw[e] & 0x7fffffffu;
                    const bool hit[N_CHECKS] = {nonfinite(aw[e]), nonfinite(bw[e]), nonfinite(cw[e]),
                                                (cw[e] >> 31) && cabs != 0u && cabs <= 0x7f800000u, diff[e] != 0u};
#pragma unroll
                    for (int q = 0; q < N_CHECKS; ++q)
                        if (hit[q]) { ++cnt[q]; first[q] = idx < first[q] ? idx : first[q]; }
                }
            }
        }
        // the block's three sums -> thread 0
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] = wave_sum_u64(acc[q]);
        __syncthreads();                                                 // (sh may still be read from the previous block)
        if (lane == 0) { sh[0][wave] = acc[0]; sh[1][wave] = acc[1]; sh[2][wave] = acc[2]; }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint64_t s = sh[q][0] + sh[q][1] + sh[q][2] + sh[q][3];
                const uint64_t key = digest_mix(s ^ ((uint64_t)(j + 1) * GOLDEN) ^ AUDIT_TAG[q]);
                block_keys[q * n_blocks + j] = key;
                dsum[q] += key; dxor[q] ^= key;
            }
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) { atomicAdd(report + W_DIGEST + 2 * q, (unsigned long long)dsum[q]); atomicXor(report + W_DIGEST + 2 * q + 1, (unsigned long long)dxor[q]); }
    }
    const unsigned hits = cnt[0] | cnt[1] | cnt[2] | cnt[3] | cnt[4];
    if (__any((int)hits)) {                                              // wave-uniform; no atomic from a wave that found nothing
#pragma unroll
        for (int q = 0; q < N_CHECKS; ++q) {
            const uint64_t c = wave_sum_u64(cnt[q]), f = wave_min_u64(first[q]);
            if (lane == 0 && c) { atomicAdd(report + W_COUNT + q, (unsigned long long)c); atomicMin(report + W_FIRST + q, (unsigned long long)f); }
        }
    }
}

} // namespace

extern "C" int emdr2_state_audit_ws_bytes(int64_t n, size_t *bytes)
{
    if (!bytes || n < 8 || (n & 7)) return -1;
    *bytes = (size_t)(3 * ((n + AUDIT_BLOCK - 1) / AUDIT_BLOCK)) * 8;
    return 0;
}

extern "C" int emdr2_state_audit(const float *master, const float *m, const float *v, const void *work_bf16, int64_t n, uint64_t *block_keys,
                                 uint64_t *report, void *stream)
{
    if (!master || !m || !v || !work_bf16 || !block_keys || !report || n < 8 || (n & 7)) return -1;
    if ((((uintptr_t)master | (uintptr_t)m | (uintptr_t)v) & 15) || (((uintptr_t)work_bf16 | (uintptr_t)block_keys | (uintptr_t)report) & 7)) return -1;
    const int64_t n_blocks = (n + AUDIT_BLOCK - 1) / AUDIT_BLOCK;
    const int64_t grid = n_blocks < AUDIT_GRID_CAP ? n_blocks : AUDIT_GRID_CAP;
    launch(state_audit_init_kernel, dim3(1), 64, stream, report, n, n_blocks);
    launch(state_audit_kernel, dim3((unsigned)grid), 256, stream, master, m, v, work_bf16, n / 4, n_blocks, block_keys, report);
    return LAUNCH_OK();
}
