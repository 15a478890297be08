// emdr2_amd/csrc/mips_digest.h -- the row hash g(r) and the stamp hash h(r) of include/emdr2_mips.h, stated once, and the walk of one
// 128-row stripe of the tiled image that computes g for its rows.  The walk hands every row's hash to a SINK: the snapshot digest
// (digest_rows_kernel in mips_aux.hip) folds it, the row keys of an incremental snapshot (mips_delta.hip) store it or compare it with the
// key a base snapshot holds -- so "changed" is decided by the very bits the digest is made of, whatever the hash becomes later.
#pragma once
#include "mips_device.h"

// splitmix64's finaliser (include/emdr2_mips.h states the digest in full)
__device__ __forceinline__ uint64_t digest_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    return ((uint64_t)hi << 32) | lo;
}

// h of a stamp g that belongs to the row numbered `number` (row_base + local row)
#define DIGEST_STAMP_TAG (0x47454E53ull << 32)
__device__ __forceinline__ uint64_t digest_stamp(uint32_t g, int64_t number)
{
    return digest_mix(digest_mix((uint64_t)g | DIGEST_STAMP_TAG) ^ ((uint64_t)(number + 1) * 0x9E3779B97F4A7C15ull));
}

// One workgroup of 256 threads walks stripe `stripe` in storage order: chunk after chunk, one contiguous 8 KiB block each (thread t takes
// the 16-byte slots t and t + 256: rows t / 4 and 64 + t / 4).  acc(r) is a sum over position-tagged words, so a thread keeps one partial
// sum for each of its two rows across all chunks, whatever slot the swizzle hands it; the four lanes of a row then fold their partial
// sums and the lane with t % 4 == 0 finishes the row: sink.row(local row, g) is called there, once for each of the stripe's 128 rows --
// the rest of a partly covered stripe and the zero padding past the shard's end included, which the sink leaves out.
template <class Sink>
__device__ __forceinline__ void digest_stripe_walk(const char *__restrict__ tiled, int nch, int64_t stripe, int64_t row_base, Sink &sink)
{
    const int tid = threadIdx.x;
    const uint4 *block = (const uint4 *)(tiled + (size_t)stripe * nch * STRIPE_CHUNK_BYTES);
    const int ri = tid >> 2, sp = tid & 3;                            // (row 64 + ri has the same swizzle: bits 2..3 of the row agree)
    const int s = sp ^ ((ri >> 2) & 3);
    uint64_t acc0 = 0, acc1 = 0;
#pragma unroll 2
    for (int c = 0; c < nch; ++c) {
        const uint4 a = block[(size_t)c * 512 + tid], b = block[(size_t)c * 512 + 256 + tid];
        const uint64_t tag = (uint64_t)((c * 4 + s) * 4 + 1) << 32;    // word j of the row carries (j + 1) << 32
        acc0 += digest_mix(a.x | tag) + digest_mix(a.y | (tag + (1ull << 32))) + digest_mix(a.z | (tag + (2ull << 32))) + digest_mix(a.w | (tag + (3ull << 32)));
        acc1 += digest_mix(b.x | tag) + digest_mix(b.y | (tag + (1ull << 32))) + digest_mix(b.z | (tag + (2ull << 32))) + digest_mix(b.w | (tag + (3ull << 32)));
    }
    acc0 += shfl_xor_u64(acc0, 1); acc0 += shfl_xor_u64(acc0, 2);
    acc1 += shfl_xor_u64(acc1, 1); acc1 += shfl_xor_u64(acc1, 2);
    if (sp == 0) {
        const int64_t r0 = stripe * STRIPE_ROWS + ri, r1 = r0 + 64;
        sink.row(r0, digest_mix(acc0 ^ ((uint64_t)(row_base + r0 + 1) * 0x9E3779B97F4A7C15ull)));
        sink.row(r1, digest_mix(acc1 ^ ((uint64_t)(row_base + r1 + 1) * 0x9E3779B97F4A7C15ull)));
    }
}

// (sum, xor) of one value pair per thread over the workgroup's 256 threads -> thread 0 holds the result after the call (`sh`: 8 words)
__device__ __forceinline__ void digest_block_fold(uint64_t &sum, uint64_t &x, uint64_t *sh)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { sum += shfl_xor_u64(sum, o); x ^= shfl_xor_u64(x, o); }
    __syncthreads();                                                   // (sh may still be read from the previous call)
    if (lane == 0) { sh[wave] = sum; sh[4 + wave] = x; }
    __syncthreads();
    sum = sh[0] + sh[1] + sh[2] + sh[3];
    x = sh[4] ^ sh[5] ^ sh[6] ^ sh[7];
}
