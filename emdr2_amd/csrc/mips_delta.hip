// emdr2_amd/csrc/mips_delta.hip -- incremental index snapshots: the per-row keys of a shard (emdr2_mips_row_keys) and the rows whose key
// differs from the one a base snapshot holds (emdr2_mips_changed_rows; the contract is in include/emdr2_mips.h).
//
//   key(r) = g(r)            on a shard without stamps
//   key(r) = g(r) + h(r)     on one with stamps (mod 2^64): a row re-written with the same bits by newer weights is a change too
//
// g and h are those of the snapshot digests, and g comes out of the same stripe walk as digest_rows_kernel's (mips_digest.h).
//
//   row_keys_kernel        one workgroup per 128-row stripe: the keys of the rows of [row_lo, row_hi)
//   changed_pass_kernel    one workgroup per stripe, the one pass over the image: compares every row's key with its base key and leaves in
//                          the workspace the stripe's 128-bit changed mask, its count and the (sum, xor) of g and of h over its rows
//   changed_slab_kernel    one workgroup per SLAB of consecutive stripes: the slab's count and digests
//   changed_write_kernel   one workgroup per slab: sums the slab counts in front of its own -- its output offset -- and expands its stripes'
//                          masks into global rows at their ranks; fills the slots behind the set with -1; writes the report
//
// The phases are ordered by launch boundaries alone; no workgroup waits on another and nothing is accumulated across workgroups: every
// word of the workspace that a launch reads was stored by exactly one workgroup of the launch before it, so there is nothing to clear and
// the result is a function of the image, the stamps and the keys alone -- not of the order the workgroups run in, nor of the slab size
// (ranks are global).
#include "mips_kernels.h"
#include "mips_digest.h"

enum { SLAB_WORDS = 5 };    // per slab: rows changed, sum g, xor g, sum h, xor h

struct DeltaWorkspace {
    uint4 *mask;                // [n_stripes] bit i of (x, y): row i of the stripe changed; of (z, w): row 64 + i
    unsigned *count;            // [n_stripes]
    uint64_t *digest;           // [n_stripes][4] sum g, xor g, sum h, xor h
    uint64_t *slab;             // [MIPS_DELTA_MAX_SLABS][SLAB_WORDS]
};

static inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// the four parts of the workspace in `base` (16-byte aligned) -> bytes in all
static size_t carve(char *base, int64_t n_stripes, DeltaWorkspace *w)
{
    size_t off = 0;
    w->mask = (uint4 *)(base + off); off += (size_t)n_stripes * sizeof(uint4);
    w->digest = (uint64_t *)(base + off); off += (size_t)n_stripes * 4 * sizeof(uint64_t);
    w->slab = (uint64_t *)(base + off); off += (size_t)MIPS_DELTA_MAX_SLABS * SLAB_WORDS * sizeof(uint64_t);
    w->count = (unsigned *)(base + off); off += align16((size_t)n_stripes * sizeof(unsigned));
    return off;
}

size_t mips_changed_rows_workspace_bytes(int64_t n_rows)
{
    DeltaWorkspace w;
    return carve(nullptr, (n_rows + STRIPE_ROWS - 1) / STRIPE_ROWS, &w);
}

// the key of local row r, whose row hash is g
__device__ __forceinline__ uint64_t row_key(uint64_t g, const uint32_t *__restrict__ generation, int64_t r, int64_t row_base, uint64_t &h)
{
    h = generation ? digest_stamp(generation[r], row_base + r) : 0ull;
    return g + h;
}

struct StoreKeysSink {
    const uint32_t *generation;
    uint64_t *keys;
    int64_t row_lo, row_hi, row_base;
    __device__ __forceinline__ void row(int64_t r, uint64_t g)
    {
        uint64_t h;
        if (r >= row_lo && r < row_hi) keys[r] = row_key(g, generation, r, row_base, h);
    }
};

__global__ void __launch_bounds__(256) row_keys_kernel(const char *__restrict__ tiled, int nch, int64_t first_stripe, int64_t row_lo, int64_t row_hi,
                                                       int64_t row_base, const uint32_t *__restrict__ generation, uint64_t *__restrict__ keys)
{
    StoreKeysSink sink = {generation, keys, row_lo, row_hi, row_base};
    digest_stripe_walk(tiled, nch, first_stripe + blockIdx.x, row_base, sink);
}

int mips_launch_row_keys(const void *tiled, int dim, int64_t row_offset, int64_t n_chunk, int64_t row_base, const uint32_t *generation, uint64_t *keys,
                         hipStream_t stream)
{
    if (n_chunk == 0) return 0;
    const int64_t first = row_offset / STRIPE_ROWS, last = (row_offset + n_chunk - 1) / STRIPE_ROWS;
    hipLaunchKernelGGL(row_keys_kernel, dim3((unsigned)(last - first + 1)), dim3(256), 0, stream, (const char *)tiled, dim / 32, first, row_offset,
                       row_offset + n_chunk, row_base, generation, keys);
    return LAUNCH_OK();
}

// The comparing sink.  Only the 64 lanes that finish rows call it, twice each (rows ri and 64 + ri of the stripe): the changed bits are
// OR-ed into the workgroup's LDS mask, everything else stays in the lane until the workgroup folds it.
struct CompareKeysSink {
    const uint32_t *generation;
    const uint64_t *base_keys;
    int64_t n_rows, row_base;
    unsigned *sh_mask;          // [4] LDS words, zeroed
    uint64_t sum_g, xor_g, sum_h, xor_h;
    __device__ __forceinline__ void row(int64_t r, uint64_t g)
    {
        if (r >= n_rows) return;                                       // the zero padding: read, never counted
        uint64_t h;
        const uint64_t key = row_key(g, generation, r, row_base, h);
        sum_g += g; xor_g ^= g; sum_h += h; xor_h ^= h;
        if (key != base_keys[r]) {
            const int i = (int)(r & (STRIPE_ROWS - 1));
            atomicOr(&sh_mask[i >> 5], 1u << (i & 31));
        }
    }
};

__global__ void __launch_bounds__(256) changed_pass_kernel(const char *__restrict__ tiled, int nch, int64_t n_rows, int64_t row_base,
                                                           const uint32_t *__restrict__ generation, const uint64_t *__restrict__ base_keys,
                                                           DeltaWorkspace ws)
{
    __shared__ unsigned sh_mask[4];
    __shared__ uint64_t sh_fold[8];
    const int tid = threadIdx.x;
    const int64_t stripe = blockIdx.x;
    if (tid < 4) sh_mask[tid] = 0u;
    __syncthreads();
    CompareKeysSink sink = {generation, base_keys, n_rows, row_base, sh_mask, 0, 0, 0, 0};
    digest_stripe_walk(tiled, nch, stripe, row_base, sink);
    digest_block_fold(sink.sum_g, sink.xor_g, sh_fold);
    digest_block_fold(sink.sum_h, sink.xor_h, sh_fold);                 // (its barriers also order the mask's atomics before the read below)
    if (tid == 0) {
        const uint4 m = make_uint4(sh_mask[0], sh_mask[1], sh_mask[2], sh_mask[3]);
        ws.mask[stripe] = m;
        ws.count[stripe] = (unsigned)(__popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w));
        uint64_t *d = ws.digest + stripe * 4;
        d[0] = sink.sum_g; d[1] = sink.xor_g; d[2] = sink.sum_h; d[3] = sink.xor_h;
    }
}

// the stripes of slab w: [w * slab, min((w + 1) * slab, n_stripes))
__device__ __forceinline__ void slab_of(int64_t n_stripes, int64_t slab, int64_t &lo, int64_t &hi)
{
    lo = (int64_t)blockIdx.x * slab;
    hi = lo + slab < n_stripes ? lo + slab : n_stripes;
}

__global__ void __launch_bounds__(256) changed_slab_kernel(int64_t n_stripes, int64_t slab, DeltaWorkspace ws)
{
    __shared__ uint64_t sh_fold[8];
    int64_t lo, hi;
    slab_of(n_stripes, slab, lo, hi);
    uint64_t cnt = 0, none = 0, sum_g = 0, xor_g = 0, sum_h = 0, xor_h = 0;
    for (int64_t t = lo + threadIdx.x; t < hi; t += 256) {
        const uint64_t *d = ws.digest + t * 4;
        cnt += ws.count[t]; sum_g += d[0]; xor_g ^= d[1]; sum_h += d[2]; xor_h ^= d[3];
    }
    digest_block_fold(cnt, none, sh_fold);
    digest_block_fold(sum_g, xor_g, sh_fold);
    digest_block_fold(sum_h, xor_h, sh_fold);
    if (threadIdx.x == 0) {
        uint64_t *s = ws.slab + (size_t)blockIdx.x * SLAB_WORDS;
        s[0] = cnt; s[1] = sum_g; s[2] = xor_g; s[3] = sum_h; s[4] = xor_h;
    }
}

// n_slabs <= MIPS_DELTA_MAX_SLABS = 2 * 256: a thread reads at most two slabs' words.  Launched with ONE workgroup and n_slabs == 0 for an
// empty shard: the report only.
__global__ void __launch_bounds__(256) changed_write_kernel(int64_t n_stripes, int64_t slab, int n_slabs, int64_t row_base, int64_t cap,
                                                            DeltaWorkspace ws, int64_t *__restrict__ out_rows, unsigned long long *__restrict__ info)
{
    __shared__ uint64_t sh_fold[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t before = 0, total = 0, sum_g = 0, xor_g = 0, sum_h = 0, xor_h = 0;
    for (int w = tid; w < n_slabs; w += 256) {
        const uint64_t *s = ws.slab + (size_t)w * SLAB_WORDS;
        total += s[0]; before += w < (int)blockIdx.x ? s[0] : 0ull;
        sum_g += s[1]; xor_g ^= s[2]; sum_h += s[3]; xor_h ^= s[4];
    }
    uint64_t none = 0;
    digest_block_fold(total, none, sh_fold);
    digest_block_fold(before, none, sh_fold);
    const uint64_t stored = total < (uint64_t)cap ? total : (uint64_t)cap;
    // the slots behind the stored rows; the report (word 6 comes from the workgroup that holds the first changed row)
    for (int64_t i = (int64_t)stored + (int64_t)blockIdx.x * 256 + tid; i < cap; i += (int64_t)gridDim.x * 256) out_rows[i] = -1;
    if (blockIdx.x == 0) {
        digest_block_fold(sum_g, xor_g, sh_fold);
        digest_block_fold(sum_h, xor_h, sh_fold);
        if (tid == 0) {
            info[0] = total; info[1] = stored; info[2] = sum_g; info[3] = xor_g; info[4] = sum_h; info[5] = xor_h; info[7] = 0ull;
            if (total == 0) info[6] = ~0ull;
        }
    }
    if (n_slabs == 0) return;
    const uint64_t mine = ws.slab[(size_t)blockIdx.x * SLAB_WORDS];
    if (mine == 0 || (before > 0 && before >= stored)) return;         // uniform: nothing of this slab is stored, nor is its first row the first of all
    int64_t lo, hi;
    slab_of(n_stripes, slab, lo, hi);
    uint64_t running = before;                                         // changed rows in front of the four stripes of this round
    for (int64_t t0 = lo; t0 < hi; t0 += 4) {
        unsigned c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = t0 + j < hi ? ws.count[t0 + j] : 0u;
        uint64_t off = running;
#pragma unroll
        for (int j = 0; j < 4; ++j) off += j < wave ? c[j] : 0u;
        const int64_t t = t0 + wave;                                   // one stripe per wave; lane l ranks rows l and 64 + l
        if (t < hi && c[wave]) {
            const uint4 m = ws.mask[t];
            const uint64_t m0 = ((uint64_t)m.y << 32) | m.x, m1 = ((uint64_t)m.w << 32) | m.z;
            const uint64_t below = (1ull << lane) - 1ull;
            const uint64_t p0 = off + (uint64_t)__popcll(m0 & below), p1 = off + (uint64_t)__popcll(m0) + (uint64_t)__popcll(m1 & below);
            const int64_t r = row_base + t * STRIPE_ROWS + lane;
            if ((m0 >> lane) & 1ull) {
                if (p0 < stored) out_rows[p0] = r;
                if (p0 == 0) info[6] = (unsigned long long)r;
            }
            if ((m1 >> lane) & 1ull) {
                if (p1 < stored) out_rows[p1] = r + 64;
                if (p1 == 0) info[6] = (unsigned long long)(r + 64);
            }
        }
        running += (uint64_t)c[0] + c[1] + c[2] + c[3];
        if (running > 0 && running >= stored) break;                   // uniform: every row behind this round ranks past the stored ones
    }
}

int mips_launch_changed_rows(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const uint32_t *generation, const uint64_t *base_keys,
                             int64_t cap, int64_t *out_rows, uint64_t *out_info, void *workspace, hipStream_t stream)
{
    const int64_t n_stripes = (n_rows + STRIPE_ROWS - 1) / STRIPE_ROWS;
    DeltaWorkspace ws;
    carve((char *)workspace, n_stripes, &ws);
    // slabs of whole stripes, at most MIPS_DELTA_MAX_SLABS of them: the per-slab words stay one short read for every workgroup of the write launch
    const int64_t slab = (n_stripes + MIPS_DELTA_MAX_SLABS - 1) / MIPS_DELTA_MAX_SLABS;
    const int n_slabs = n_stripes ? (int)((n_stripes + slab - 1) / slab) : 0;
    if (n_stripes) {
        hipLaunchKernelGGL(changed_pass_kernel, dim3((unsigned)n_stripes), dim3(256), 0, stream, (const char *)tiled, dim / 32, n_rows, row_base,
                           generation, base_keys, ws);
        hipLaunchKernelGGL(changed_slab_kernel, dim3((unsigned)n_slabs), dim3(256), 0, stream, n_stripes, slab, ws);
    }
    hipLaunchKernelGGL(changed_write_kernel, dim3((unsigned)(n_slabs ? n_slabs : 1)), dim3(256), 0, stream, n_stripes, slab, n_slabs, row_base, cap, ws,
                       out_rows, (unsigned long long *)out_info);
    return LAUNCH_OK();
}
