// emdr2_amd/csrc/mips_aux.hip -- everything around the scan: HBM re-layout, query packing,
// candidate selection, exact integer re-scoring + validity proof, shard merge, all-exact fallback.
#include "mips_device.h"
#include "mips_kernels.h"
#include "mips_derived.h"
#include "mips_digest.h"

// ------------------------------------------------------------------------------------------------
// index re-layout (reference: add_embed_data uploads a dense row-major fp16 matrix,
// megatron/data/emdr2_index.py:248-256; here the upload is re-tiled into scan order)
// ------------------------------------------------------------------------------------------------
// Generation stamps (emdr2_mips_update_rows_stamped, _update_rows_scattered_stamped; RowStamp in mips_kernels.h): one 32-bit word per row, the
// number of optimizer steps behind the weights that wrote it.  A row writer has one thread per 16-byte segment, so a row's threads sit in
// several waves, maybe several workgroups, and each of them takes the newest-wins decision for itself from the row's stamp while the thread of
// segment 0 stores the new stamp.  That is only sound because the rule is NON-STRICT: a thread reads either the old stamp s or, after that
// store, gen; s <= gen and gen <= gen say the same, and for s > gen nobody stores at all -- every thread of the row decides alike, whatever
// it saw.  Under a strict s < gen a thread that read gen would skip its segment while its neighbours wrote theirs: a row mixed of old and
// new segments.  (A strict rule needs the decision taken once per row and a launch boundary between it and the stamp store.)  Ties write,
// which keeps "the last writer of a generation wins".  The stamp is read and stored as relaxed device-scope atomics: plain 4-byte accesses
// for the hardware, and the compiler may neither split nor repeat them.  -> whether this thread moves its segment.
__device__ __forceinline__ bool stamp_admits(const RowStamp &st, int64_t row, int seg)
{
    if (st.newest_wins && __hip_atomic_load(st.generation + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > st.gen) {
        if (seg == 0 && st.n_kept_newer) atomicAdd(st.n_kept_newer, 1u);        // a kept-newer row is counted once
        return false;
    }
    if (seg == 0) __hip_atomic_store(st.generation + row, st.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// (STAMPED = false is the kernel as it was before there were stamps: the stamp argument is an empty struct nobody reads)
template <bool STAMPED>
__global__ void pack_rows_kernel(const uint4 *__restrict__ rows_rm, int64_t n_chunk, int nseg, int64_t row_offset,
                                 char *__restrict__ tiled, typename StampArg<STAMPED>::type st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_chunk * nseg) return;
    const int64_t r = i / nseg;
    const int seg = (int)(i - r * nseg);
    if constexpr (STAMPED) { if (!stamp_admits(st, row_offset + r, seg)) return; }
    *(uint4 *)(tiled + tiled_seg_offset(row_offset + r, seg, nseg >> 2)) = rows_rm[i];
}

// (||E[r]||^2 of a row by a wave, row_norm_sq_wave, and the block routine behind block_norms_kernel: mips_derived.h)
__global__ void row_norm_max_kernel(const uint4 *__restrict__ rows_rm, int64_t n_chunk, int nseg, float *emax_sq)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    float best = 0.f;
    for (int64_t r = wave; r < n_chunk; r += nwaves) best = fmaxf(best, row_norm_sq_wave(RowMajorRow{rows_rm + r * nseg}, nseg, lane));
    if (lane == 0 && best > 0.f) atomicMax((unsigned *)emax_sq, __float_as_uint(best)); // non-negative floats order as uints
}

// In-place row updates (emdr2_mips_update_rows, _update_rows_scattered): block_norm_sq[b] = max over the 256 rows of block b of ||E[r]||^2,
// read from the tiled image (rows past the end of the shard are zero there, the image is padded to 512 rows).  One workgroup per block, 64
// rows per wave.  The block comes from a range or from the list of touched blocks (mips_device.h); the arithmetic is this one routine.
template <class Blocks>
__global__ void __launch_bounds__(256) block_norms_kernel(const char *__restrict__ tiled, int nseg, Blocks blocks, float *__restrict__ block_norm_sq)
{
    __shared__ float sh[4];
    int64_t block;
    if (!blocks.get(block)) return;
    StoreBlockNorm sink{block_norm_sq};
    block_norm_256(tiled, nseg, block, sh, sink);
}

// *emax_sq = max of the whole table (one workgroup: 82,092 entries at the full index), so the bound can FALL when the row that held the
// maximum was overwritten.  The maximum of non-negative floats does not depend on the order they are folded in.
__global__ void __launch_bounds__(1024) table_max_kernel(const float *__restrict__ block_norm_sq, int64_t n_blocks, float *__restrict__ emax_sq)
{
    __shared__ float sh[16];
    float best = 0.f;
    for (int64_t i = threadIdx.x; i < n_blocks; i += 1024) best = fmaxf(best, block_norm_sq[i]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = fmaxf(best, __shfl_xor(best, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) best = fmaxf(best, sh[w]);
        *emax_sq = best;
    }
}

int mips_launch_block_norms(const void *tiled, int dim, int64_t first_block, int64_t n_blocks, float *block_norm_sq, hipStream_t stream)
{
    if (n_blocks == 0) return 0;
    hipLaunchKernelGGL(block_norms_kernel<BlockRange>, dim3((unsigned)n_blocks), dim3(256), 0, stream, (const char *)tiled, dim / 8, BlockRange{first_block},
                       block_norm_sq);
    return LAUNCH_OK();
}

// the same over the touched-block list of a scattered update: `grid` workgroups, those not below *n_touched exit
int mips_launch_block_norms_list(const void *tiled, int dim, const unsigned *touched, const unsigned *n_touched, unsigned grid, float *block_norm_sq,
                                 hipStream_t stream)
{
    if (grid == 0) return 0;
    hipLaunchKernelGGL(block_norms_kernel<BlockList>, dim3(grid), dim3(256), 0, stream, (const char *)tiled, dim / 8, BlockList{touched, n_touched},
                       block_norm_sq);
    return LAUNCH_OK();
}

int mips_launch_table_max(const float *block_norm_sq, int64_t n_blocks, float *emax_sq, hipStream_t stream)
{
    hipLaunchKernelGGL(table_max_kernel, dim3(1), dim3(1024), 0, stream, block_norm_sq, n_blocks, emax_sq);
    return LAUNCH_OK();
}

// pack_rows_kernel alone: rows into the image, emax_sq untouched (the in-place update recomputes it from the block table)
int mips_launch_write_rows(const void *rows_rm, int64_t n_chunk, int dim, int64_t row_offset, void *tiled, const RowStamp *stamp, hipStream_t stream)
{
    const int nseg = dim / 8;
    const int64_t total = n_chunk * nseg;
    if (total == 0) return 0;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (stamp)
        hipLaunchKernelGGL(pack_rows_kernel<true>, grid, dim3(256), 0, stream, (const uint4 *)rows_rm, n_chunk, nseg, row_offset, (char *)tiled, *stamp);
    else
        hipLaunchKernelGGL(pack_rows_kernel<false>, grid, dim3(256), 0, stream, (const uint4 *)rows_rm, n_chunk, nseg, row_offset, (char *)tiled,
                           NoStamp{});
    return LAUNCH_OK();
}

// Scattered in-place updates (emdr2_mips_update_rows_scattered): pack_rows_kernel with the destination row read from row_ids.  Entries whose
// id is outside [0, n_rows_total) are skipped, so nothing is ever written into the zero padding or past the image.  The thread that moves
// a row's first segment also claims the row's 256-row block: an atomic exchange on the block's flag word (zeroed per call), and whoever
// finds it 0 appends the block to `touched` through the counter -- once per block however many rows of the call fall into it.  Both are
// device-scope atomics on words nobody reads in this launch; the list and its count are read by LATER launches on the same stream.  At most
// min(n_upd, table blocks) = `cap` distinct blocks can be claimed, which is the list's length.  STAMPED: a row that stamp_admits leaves
// alone is neither written nor does it claim its block (nothing in the block changed on its account); invalid ids are skipped before the
// stamp is looked at, so they are never counted as kept newer.
template <bool STAMPED>
__global__ void pack_rows_at_kernel(const uint4 *__restrict__ rows_rm, const int64_t *__restrict__ row_ids, int64_t n_upd, int nseg, int64_t n_rows_total,
                                    char *__restrict__ tiled, unsigned *__restrict__ claimed, unsigned *__restrict__ n_touched,
                                    unsigned *__restrict__ touched, unsigned cap, typename StampArg<STAMPED>::type st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_upd * nseg) return;
    const int64_t r = i / nseg;
    const int seg = (int)(i - r * nseg);
    const int64_t row = row_ids[r];
    if (row < 0 || row >= n_rows_total) return;
    if constexpr (STAMPED) { if (!stamp_admits(st, row, seg)) return; }
    *(uint4 *)(tiled + tiled_seg_offset(row, seg, nseg >> 2)) = rows_rm[i];
    if (seg == 0) {
        const unsigned b = (unsigned)(row >> 8);
        if (atomicExch(&claimed[b], 1u) == 0u) {
            const unsigned slot = atomicAdd(n_touched, 1u);
            if (slot < cap) touched[slot] = b;
        }
    }
}

int mips_launch_write_rows_at(const void *rows_rm, const int64_t *row_ids, int64_t n_upd, int dim, int64_t n_rows_total, void *tiled, unsigned *claimed,
                              unsigned *n_touched, unsigned *touched, unsigned cap, const RowStamp *stamp, hipStream_t stream)
{
    const int nseg = dim / 8;
    const int64_t total = n_upd * nseg;
    if (total == 0) return 0;
    if ((total + 255) / 256 > 0x7fffffff) return -4;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (stamp)
        hipLaunchKernelGGL(pack_rows_at_kernel<true>, grid, dim3(256), 0, stream, (const uint4 *)rows_rm, row_ids, n_upd, nseg, n_rows_total,
                           (char *)tiled, claimed, n_touched, touched, cap, *stamp);
    else
        hipLaunchKernelGGL(pack_rows_at_kernel<false>, grid, dim3(256), 0, stream, (const uint4 *)rows_rm, row_ids, n_upd, nseg, n_rows_total,
                           (char *)tiled, claimed, n_touched, touched, cap, NoStamp{});
    return LAUNCH_OK();
}

int mips_launch_pack_rows(const void *rows_rm, int64_t n_chunk, int dim, int64_t row_offset, void *tiled,
                          float *emax_sq, hipStream_t stream)
{
    if (n_chunk == 0) return 0;
    const int rc = mips_launch_write_rows(rows_rm, n_chunk, dim, row_offset, tiled, nullptr, stream);
    if (rc) return rc;
    int nb = (int)((n_chunk + 3) / 4);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(row_norm_max_kernel, dim3(nb), dim3(256), 0, stream, (const uint4 *)rows_rm, n_chunk, dim / 8, emax_sq);
    return LAUNCH_OK();
}

// The one gather out of the image (emdr2_mips_unpack_rows: row_base 0; emdr2_mips_gather_rows: global rows): output row r is image row
// row_ids[r] - row_base when that lies in [0, n_rows), all zero bytes otherwise (-1, a row of another shard, a row of the zero padding).
// One 16-byte segment per thread; the ids are never used as an address unchecked.
__global__ void unpack_rows_kernel(const char *__restrict__ tiled, int nseg, int64_t n_rows, int64_t row_base,
                                   const int64_t *__restrict__ row_ids, int64_t n_out, uint4 *__restrict__ rows_rm)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out * nseg) return;
    const int64_t r = i / nseg;
    const int seg = (int)(i - r * nseg);
    const int64_t id = row_ids[r];
    // (compared before the subtraction: no id, however wild, can wrap into the range)
    const bool mine = id >= row_base && id - row_base < n_rows;
    rows_rm[i] = mine ? *(const uint4 *)(tiled + tiled_seg_offset(id - row_base, seg, nseg >> 2)) : make_uint4(0, 0, 0, 0);
}

int mips_launch_unpack_rows(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const int64_t *row_ids, int64_t n_out,
                            void *rows_rm, hipStream_t stream)
{
    const int nseg = dim / 8;
    const int64_t total = n_out * nseg;
    if (total == 0) return 0;
    hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const char *)tiled, nseg,
                       n_rows, row_base, row_ids, n_out, (uint4 *)rows_rm);
    return LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------------
// generation statistics (emdr2_mips_generation_stats; the report words are documented in include/emdr2_mips.h)
// ------------------------------------------------------------------------------------------------
// One pass over the stamps of a whole shard (global_rows null: item i is local row i) or of a list of GLOBAL rows (item i is global_rows[i]
// when it falls into [row_base, row_base + n_rows), else it is left out -- compared before the subtraction, like unpack_rows_kernel).  A
// thread walks its items grid-stride and keeps its own count / sum / min / max; runs of equal histogram bins go to the workgroup's LDS
// tally with one atomic (the stamps of neighbouring rows are mostly equal: one writer, one pass).  The workgroup flushes its non-zero words
// with 64-bit integer atomics, like the audit: the report does not depend on the order the items are visited in.
enum { G_COUNT = 0, G_SUM = 1, G_MIN = 2, G_MAX = 3, G_FUTURE = 4, G_HIST = 5, G_WORDS = G_HIST + 32 };
static_assert(G_WORDS == MIPS_GEN_WORDS && G_WORDS <= 64, "the report layout of include/emdr2_mips.h, cleared by one wave");

__global__ void __launch_bounds__(64) generation_stats_init_kernel(unsigned long long *report)
{
    if (threadIdx.x < G_WORDS) report[threadIdx.x] = threadIdx.x == G_MIN ? ~0ull : 0ull;
}

__global__ void __launch_bounds__(256) generation_stats_kernel(const uint32_t *__restrict__ generation, int64_t n_rows, int64_t row_base,
                                                               const int64_t *__restrict__ global_rows, int64_t n_items, uint32_t now,
                                                               unsigned long long *__restrict__ report)
{
    __shared__ unsigned long long sh_sum;
    __shared__ unsigned sh_count, sh_future, sh_min, sh_max, sh_hist[32];
    const int tid = threadIdx.x;
    if (tid < 32) sh_hist[tid] = 0u;
    if (tid == 0) { sh_sum = 0ull; sh_count = 0u; sh_future = 0u; sh_min = 0xffffffffu; sh_max = 0u; }
    __syncthreads();
    unsigned long long sum = 0ull;
    unsigned count = 0u, future = 0u, lo = 0xffffffffu, hi = 0u, run_bin = 0u, run = 0u;    // (a thread sees < 2^32 items: the grid is sized for it)
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n_items; i += stride) {
        int64_t row = i;
        if (global_rows) {
            const int64_t id = global_rows[i];
            if (id < row_base || id - row_base >= n_rows) continue;
            row = id - row_base;
        }
        const uint32_t g = generation[row];
        const uint32_t age = g > now ? 0u : now - g;
        future += g > now;
        ++count; sum += age;
        lo = age < lo ? age : lo; hi = age > hi ? age : hi;
        unsigned bin = age ? 32u - (unsigned)__clz(age) : 0u;          // [2^(b-1), 2^b) -> b
        bin = bin > 31u ? 31u : bin;                                    // (ages of 2^31 and more cannot come from stamps below 2^31)
        if (bin != run_bin) {
            if (run) atomicAdd(&sh_hist[run_bin], run);
            run_bin = bin; run = 0u;
        }
        ++run;
    }
    if (run) atomicAdd(&sh_hist[run_bin], run);
    if (count) {
        atomicAdd(&sh_count, count); atomicAdd(&sh_sum, sum); atomicMin(&sh_min, lo); atomicMax(&sh_max, hi);
        if (future) atomicAdd(&sh_future, future);
    }
    __syncthreads();
    if (sh_count == 0u) return;                                         // (uniform: nothing of this workgroup's was covered)
    if (tid == 0) {
        atomicAdd(&report[G_COUNT], (unsigned long long)sh_count);
        atomicAdd(&report[G_SUM], sh_sum);
        atomicMin(&report[G_MIN], (unsigned long long)sh_min);
        atomicMax(&report[G_MAX], (unsigned long long)sh_max);
        if (sh_future) atomicAdd(&report[G_FUTURE], (unsigned long long)sh_future);
    } else if (tid >= 32 && tid < 64 && sh_hist[tid - 32]) {
        atomicAdd(&report[G_HIST + tid - 32], (unsigned long long)sh_hist[tid - 32]);
    }
}

int mips_launch_generation_stats(const uint32_t *generation, int64_t n_rows, int64_t row_base, const int64_t *global_rows, int64_t n_items,
                                 uint32_t now, uint64_t *report, hipStream_t stream)
{
    hipLaunchKernelGGL(generation_stats_init_kernel, dim3(1), dim3(64), 0, stream, (unsigned long long *)report);
    if (n_rows > 0 && n_items > 0) {
        int64_t blocks = (n_items + 255) / 256;
        // two workgroups per CU, a thread then walks n_items / 131,072 items: every workgroup ends in five to a dozen atomics on the SAME
        // 37 words, which serialise -- with 2,048 workgroups they, not the 10 MB of stamps of an N / 8 shard, set the time of the pass
        if (blocks > 512) blocks = 512;
        hipLaunchKernelGGL(generation_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, generation, n_rows, row_base, global_rows, n_items,
                           now, (unsigned long long *)report);
    }
    return LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------------
// index snapshots (emdr2_mips_export_rows / _digest_rows): a contiguous row range back to row-major, and its order-free 64-bit digest
// ------------------------------------------------------------------------------------------------
// The inverse of pack_rows_kernel for rows [row_lo, row_hi).  Eight lanes move one row's two neighbouring chunks: eight rows of a wave
// read 512 contiguous bytes of each of the two 8 KiB blocks (the swizzle only permutes the four 16-byte slots inside a row's 64 bytes)
// and write 128 contiguous bytes of each output row.  Row groups are aligned to 8 image rows, whatever row_lo is.
__global__ void __launch_bounds__(256) export_rows_kernel(const char *__restrict__ tiled, int nch, int npairs, int64_t row_lo, int64_t row_hi,
                                                          int64_t n_items, uint4 *__restrict__ rows_rm)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const int j = (int)(i & 7), rl = (int)((i >> 3) & 7);
    const int64_t q = i >> 6;
    const int64_t group = q / npairs;
    const int pair = (int)(q - group * npairs);
    const int64_t row = (row_lo & ~(int64_t)7) + group * 8 + rl;
    const int seg = pair * 8 + j;
    if (row < row_lo || row >= row_hi || seg >= nch * 4) return;
    rows_rm[(row - row_lo) * (nch * 4) + seg] = *(const uint4 *)(tiled + tiled_seg_offset(row, seg, nch));
}

int mips_launch_export_rows(const void *tiled, int dim, int64_t row_offset, int64_t n_chunk, void *rows_rm, hipStream_t stream)
{
    if (n_chunk == 0) return 0;
    const int nch = dim / 32, npairs = (nch + 1) / 2;
    const int64_t groups = ((row_offset + n_chunk + 7) >> 3) - (row_offset >> 3);
    const int64_t items = groups * npairs * 64;
    hipLaunchKernelGGL(export_rows_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, (const char *)tiled, nch, npairs,
                       row_offset, row_offset + n_chunk, items, (uint4 *)rows_rm);
    return LAUNCH_OK();
}

// g(r), h(r) and the stripe walk are stated once, in mips_digest.h; here the walk's sink folds the rows of [row_lo, row_hi) into the
// workgroup's sum and xor.  One workgroup per 128-row stripe; each row is finished once, and the workgroup issues ONE 64-bit add and ONE
// 64-bit xor.  Rows outside [row_lo, row_hi) -- the rest of a partly covered stripe, the zero padding past the shard's end -- are read and
// left out.
struct DigestFoldSink {
    int64_t row_lo, row_hi;
    uint64_t sum, x;
    __device__ __forceinline__ void row(int64_t r, uint64_t g)
    {
        if (r >= row_lo && r < row_hi) { sum += g; x ^= g; }
    }
};

__global__ void __launch_bounds__(256) digest_rows_kernel(const char *__restrict__ tiled, int nch, int64_t first_stripe, int64_t row_lo, int64_t row_hi,
                                                          int64_t row_base, unsigned long long *__restrict__ digest)
{
    __shared__ uint64_t sh_sum[4], sh_xor[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    DigestFoldSink sink = {row_lo, row_hi, 0, 0};
    digest_stripe_walk(tiled, nch, first_stripe + blockIdx.x, row_base, sink);
    uint64_t sum = sink.sum, x = sink.x;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { sum += shfl_xor_u64(sum, o); x ^= shfl_xor_u64(x, o); }
    if (lane == 0) { sh_sum[wave] = sum; sh_xor[wave] = x; }
    __syncthreads();
    if (tid == 0) {
        atomicAdd(&digest[0], (unsigned long long)(sh_sum[0] + sh_sum[1] + sh_sum[2] + sh_sum[3]));
        atomicXor(&digest[1], (unsigned long long)(sh_xor[0] ^ sh_xor[1] ^ sh_xor[2] ^ sh_xor[3]));
    }
}

int mips_launch_digest_rows(const void *tiled, int dim, int64_t row_offset, int64_t n_chunk, int64_t row_base, uint64_t *digest, hipStream_t stream)
{
    if (n_chunk == 0) return 0;
    const int64_t first = row_offset / STRIPE_ROWS, last = (row_offset + n_chunk - 1) / STRIPE_ROWS;
    hipLaunchKernelGGL(digest_rows_kernel, dim3((unsigned)(last - first + 1)), dim3(256), 0, stream, (const char *)tiled, dim / 32, first, row_offset,
                       row_offset + n_chunk, row_base, (unsigned long long *)digest);
    return LAUNCH_OK();
}

// The digest of the generation stamps of rows [row_lo, row_hi) (emdr2_mips_digest_stamps): h(r) of include/emdr2_mips.h, summed and xor-ed.
// The stamp array is only 4-byte aligned and a range starts at any row, so the range is cut in three: the at most three rows in front of
// the first 16-byte boundary, whole uint4 vectors, and the at most three rows behind the last one.  The vectors are walked grid-stride
// (the grid is capped like generation_stats_kernel's: the workgroups end in two atomics on the same two words); the up to six loose rows go
// to the first threads of workgroup 0.  Per-thread partials, a wave and an LDS reduction, ONE 64-bit add and ONE 64-bit xor per workgroup;
// no workgroup waits on another.
__global__ void __launch_bounds__(256) digest_stamps_kernel(const uint32_t *__restrict__ generation, int64_t row_lo, int64_t row_hi, int64_t body_lo,
                                                            int64_t n_vec, int64_t row_base, unsigned long long *__restrict__ digest)
{
    __shared__ uint64_t sh_sum[4], sh_xor[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t sum = 0, x = 0;
    const uint4 *body = (const uint4 *)(generation + body_lo);         // (16-byte aligned: the launcher chose body_lo so)
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t v = (int64_t)blockIdx.x * 256 + tid; v < n_vec; v += stride) {
        const uint4 s = body[v];
        const int64_t number = row_base + body_lo + v * 4;
        const uint64_t h0 = digest_stamp(s.x, number), h1 = digest_stamp(s.y, number + 1), h2 = digest_stamp(s.z, number + 2),
                       h3 = digest_stamp(s.w, number + 3);
        sum += h0 + h1 + h2 + h3; x ^= h0 ^ h1 ^ h2 ^ h3;
    }
    if (blockIdx.x == 0 && tid < 6) {                                  // the head [row_lo, body_lo) and the tail [body_hi, row_hi): < 4 rows each
        const int64_t n_head = body_lo - row_lo, body_hi = body_lo + n_vec * 4;
        const int64_t r = tid < n_head ? row_lo + tid : body_hi + (tid - n_head);
        if (r < row_hi) { const uint64_t h = digest_stamp(generation[r], row_base + r); sum += h; x ^= h; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { sum += shfl_xor_u64(sum, o); x ^= shfl_xor_u64(x, o); }
    if (lane == 0) { sh_sum[wave] = sum; sh_xor[wave] = x; }
    __syncthreads();
    if (tid == 0) {
        atomicAdd(&digest[0], (unsigned long long)(sh_sum[0] + sh_sum[1] + sh_sum[2] + sh_sum[3]));
        atomicXor(&digest[1], (unsigned long long)(sh_xor[0] ^ sh_xor[1] ^ sh_xor[2] ^ sh_xor[3]));
    }
}

int mips_launch_digest_stamps(const uint32_t *generation, int64_t row_offset, int64_t n_chunk, int64_t row_base, uint64_t *digest, hipStream_t stream)
{
    if (n_chunk == 0) return 0;
    const int64_t row_hi = row_offset + n_chunk;
    // the first row at or behind row_offset whose stamp sits on a 16-byte boundary (the array itself is 4-byte aligned)
    int64_t body_lo = row_offset + (int64_t)((4 - ((((uintptr_t)generation >> 2) + (uint64_t)row_offset) & 3)) & 3);
    if (body_lo > row_hi) body_lo = row_hi;
    const int64_t n_vec = (row_hi - body_lo) >> 2;
    int64_t blocks = (n_vec + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 512 ? 512 : blocks);
    hipLaunchKernelGGL(digest_stamps_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, generation, row_offset, row_hi, body_lo, n_vec, row_base,
                       (unsigned long long *)digest);
    return LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------------
// query packing: [n_q, dim] row-major -> per chunk a [bn rows x 64 B] swizzled block (zero padded)
// ------------------------------------------------------------------------------------------------
// Everything a search sets up before its first scan, in one launch (PrepareParams in mips_kernels.h names the three parts); one wave per
// padded query row, which it reads from memory once.  The fp16 image and ||q|| come straight from the loaded segments; the int8 image needs
// max |q| first, so the row waits in LDS (dim * 2 bytes, only when that part is asked for) and is quantised from there: chunk-tiled like the
// fp16 one with 64 k-values per chunk, per query {t_q, a_q, b_q} of mips_scan8i.hip.  The wave's threads also spread the few thousand words
// of thresholds, counts, flags and zeroed counters over the grid.
__global__ void __launch_bounds__(64) prepare_kernel(PrepareParams p)
{
    extern __shared__ uint4 sh_qrow[];
    const int q = blockIdx.x, lane = threadIdx.x;
    const int n_q = p.n_q, nseg = p.dim / 8, bn = p.bn;
    const uint4 *queries = (const uint4 *)p.queries;
    char *const q_tiled = (char *)p.q_tiled, *const q8 = (char *)p.q8_tiled;
    float s = 0.f, amax = 0.f;
    for (int seg = lane; seg < nseg; seg += 64) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (q < n_q) {
            v = queries[(size_t)q * nseg + seg];
            const half8 h = __builtin_bit_cast(half8, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float x = (float)h[j]; s += x * x; amax = fmaxf(amax, fabsf(x)); }
        }
        const int c = seg >> 2, sp = (seg & 3) ^ ((q >> 2) & 3);
        *(uint4 *)(q_tiled + ((size_t)c * bn * 4 + (size_t)q * 4 + sp) * 16) = v;
        if (q8) sh_qrow[seg] = v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0 && q < n_q) p.qnorm[q] = sqrtf(s) * 1.001f;

    if (p.tau) {
        const unsigned i = (unsigned)q * 64 + lane;
        if (i < (unsigned)bn) {
            p.tau[i] = -__builtin_inff();
            p.count[i] = (i < (unsigned)n_q) ? p.dense_count : 0u;
        }
        if (i < (unsigned)n_q) p.flags[i] = 0u;
        // the sub-list counts, pending counts and pair-progress counters of the persistent scan launches (mips_scan8.hip)
        uint4 *const zero16 = (uint4 *)p.zero;
        const unsigned n_zero16 = (unsigned)(p.n_zero / 4);
        for (unsigned j = i; j < n_zero16; j += gridDim.x * 64) zero16[j] = make_uint4(0u, 0u, 0u, 0u);
    }

    if (!q8) return;
    __syncthreads();                                           // (a lane quantises segments its neighbours staged)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    const float t = amax / 127.f;
    const float inv = t > 0.f ? 127.f / amax : 0.f;
    float a2 = 0.f, b2 = 0.f;
    for (int g = lane; g < nseg / 2; g += 64) {                // 16 k-values: fp16 groups 2 g, 2 g + 1 -> int8 group g
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (q < n_q) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const half8 h = __builtin_bit_cast(half8, sh_qrow[2 * g + hf]);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = (float)h[j];
                    const int qv = quant8(x, inv);
                    const float y = t * (float)qv, r = x - y;
                    a2 += r * r; b2 += y * y;
                    w[2 * hf + (j >> 2)] |= ((unsigned)qv & 255u) << (8 * (j & 3));
                }
            }
        }
        const int c = g >> 2, sp = (g & 3) ^ ((q >> 2) & 3);
        *(uint4 *)(q8 + ((size_t)c * bn * 4 + (size_t)q * 4 + sp) * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { a2 += __shfl_xor(a2, o); b2 += __shfl_xor(b2, o); }
    // (the same fp32 evaluation slack on the residual as in the seal: ||q|| <= ||q - t q8|| + ||t q8||)
    const float ra = sqrtf(a2), rb = sqrtf(b2);
    if (lane == 0)
        ((float4 *)p.qc)[q] = q < n_q ? make_float4(t, (ra + (ra + rb) * 0x1p-22f) * 1.001f, rb * 1.001f, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void pack_queries_frag_kernel(const uint4 *__restrict__ queries, int n_q, int nseg, char *__restrict__ q_frag)
{
    const int q = blockIdx.x; // 512 padded query rows, one wave each
    const int lane0 = threadIdx.x;
    const int wave = q >> 6, ni = (q >> 5) & 1, l31 = q & 31;
    for (int seg = lane0; seg < nseg; seg += 64) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (q < n_q) v = queries[(size_t)q * nseg + seg];
        const int c = seg >> 2, s = seg & 3, ks = s >> 1, hi = s & 1;
        const int lane = hi * 32 + l31;
        *(uint4 *)(q_frag + ((((size_t)(c * 8 + wave) * 2 + ks) * 2 + ni) * 64 + lane) * 16) = v;
    }
}

int mips_launch_pack_queries_frag(const void *queries, int n_q, int dim, void *q_frag, hipStream_t stream)
{
    hipLaunchKernelGGL(pack_queries_frag_kernel, dim3(512), dim3(64), 0, stream, (const uint4 *)queries, n_q, dim / 8, (char *)q_frag);
    return LAUNCH_OK();
}

int mips_launch_prepare(const PrepareParams &p, hipStream_t stream)
{
    if (p.tau && ((p.n_zero & 3) || ((uintptr_t)p.zero & 15) || (p.n_zero && !p.zero))) return -1;
    if (p.q8_tiled && (p.dim % 16)) return -1;
    hipLaunchKernelGGL(prepare_kernel, dim3(p.bn), dim3(64), p.q8_tiled ? (size_t)p.dim * 2 : 0, stream, p);
    return LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------------
// candidate selection: keep the kp largest keys (fp32 score desc, row asc) of each query
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t cand_key(uint2 e)
{
    return ((uint64_t)f32_order(__uint_as_float(e.x)) << 32) | (uint64_t)(0xffffffffu - e.y);
}

// wave 0: find the digit whose descending cumulative count first reaches `need`
__device__ __forceinline__ void pick_digit(const unsigned *hist, unsigned need, unsigned *out_digit, unsigned *out_need)
{
    const int lane = threadIdx.x;
    unsigned h[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { h[j] = hist[255 - (4 * lane + j)]; s += h[j]; }
    unsigned incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    unsigned c = incl - s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c < need && need <= c + h[j]) { *out_digit = 255 - (4 * lane + j); *out_need = need - c; }
        c += h[j];
    }
}

// One block of 256 threads reduces query q's candidate list to its kp largest keys (radix select, 8 digits of 8 bits from the top) and sets
// tau[q] to the kp-th score.  r04: lists of up to SEL_LDS keys (the dense first segment has 8,192) are staged in LDS once instead of being
// re-read from L2 by each of the eight passes, and a thread adds RUNS of equal digits to the histogram with one atomic -- scores of one query
// share their sign / exponent byte, so the first passes used to serialise thousands of LDS atomics on one or two bins (96 us for the first
// select of a search, 18 us for the later ones: a third of what a search on an N / 8 row shard spends outside its scan).
#define SEL_LDS 8192
struct SelectShared {
    uint64_t key[SEL_LDS];
    unsigned hist[256];
    unsigned digit, need, out;
    uint2 keep[128];
};
// entry i of query q's whole candidate set: the main list [0, n_main) followed by the eight per-XCD sub-lists (lengths sub[x])
struct CandView {
    const uint2 *main_list, *sub_lists;   // [capq], [8][SUBCAP]
    unsigned n_main, sub_end[8];          // sub_end[x] = n_main + sub[0] + .. + sub[x]
    __device__ __forceinline__ uint2 at(unsigned i) const
    {
        if (i < n_main) return main_list[i];
        unsigned lo = n_main;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            if (i < sub_end[x]) return sub_lists[x * SUBCAP + (i - lo)];
            lo = sub_end[x];
        }
        return main_list[0];
    }
};

// (a block of NT threads, a multiple of 256: the stand-alone select has 256, finalize_kernel<2> FINISH_THREADS)
template <int NT>
__device__ __forceinline__ void select_block(SelectShared &sh, uint2 *cand_all, unsigned *count, uint2 *cand8, unsigned *count8, float *tau, unsigned *flags,
                                             unsigned capq, int kp, int q)
{
    const int tid = threadIdx.x;
    uint2 *cand = cand_all + (size_t)q * capq;
    CandView cv;
    cv.main_list = cand;
    cv.sub_lists = cand8 ? cand8 + (size_t)q * 8 * SUBCAP : nullptr;
    unsigned n = count[q];
    if (n > capq) { if (tid == 0) { atomicOr(&flags[q], 2u); count[q] = capq; } n = capq; }
    cv.n_main = n;
    bool any_sub = false;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        unsigned m = cand8 ? count8[x * 512 + q] : 0u;
        if (m > SUBCAP) m = SUBCAP;                                     // (a full sub-list spilled its later survivors into the main list: mips_scan8.hip s8_append)
        any_sub |= m != 0;
        n += m;
        cv.sub_end[x] = n;
    }
    __syncthreads();                                                  // (everybody has read the sub-list counts before they are reset below)
    if (any_sub && tid < 8) count8[tid * 512 + q] = 0;                // the next segment appends to empty sub-lists
    if (n <= (unsigned)kp) {
        if (any_sub) {                                                // fewer than kp candidates in all: move the sub-list entries behind the main ones
            for (unsigned i = cv.n_main + tid; i < n; i += NT) cand[i] = cv.at(i);
            if (tid == 0) count[q] = n;
        }
        return;
    }
    const bool staged = n <= SEL_LDS;
    if (staged) {
        // eight loads in flight per thread (one at a time, the 32 rounds of an 8,192-entry list each paid a full L2 latency)
        for (unsigned i0 = tid; i0 < n; i0 += 8 * NT) {
            uint2 e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { const unsigned i = i0 + j * NT; e[j] = cv.at(i < n ? i : n - 1); }
#pragma unroll
            for (int j = 0; j < 8; ++j) { const unsigned i = i0 + j * NT; if (i < n) sh.key[i] = cand_key(e[j]); }
        }
    }
    uint64_t prefix = 0, mask = 0;
    unsigned need = (unsigned)kp;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (NT == 256 || tid < 256) sh.hist[tid] = 0;
        __syncthreads();
        unsigned run_digit = 0xffffffffu, run = 0;
        for (unsigned i = tid; i < n; i += NT) {
            const uint64_t k = staged ? sh.key[i] : cand_key(cv.at(i));
            if ((k & mask) == prefix) {
                const unsigned d = (unsigned)(k >> shift) & 255u;
                if (d != run_digit) {
                    if (run) atomicAdd(&sh.hist[run_digit], run);
                    run_digit = d; run = 0;
                }
                ++run;
            }
        }
        if (run) atomicAdd(&sh.hist[run_digit], run);
        __syncthreads();
        if (tid < 64) pick_digit(sh.hist, need, &sh.digit, &sh.need);
        __syncthreads();
        prefix |= (uint64_t)sh.digit << shift;
        mask |= (uint64_t)0xff << shift;
        need = sh.need;
        const unsigned same = sh.hist[sh.digit];                      // keys that share the prefix so far
        __syncthreads();
        // r05: the upper half of a key is its fp32 score, the lower half only breaks ties by row.  Once the four score digits are fixed and ALL
        // keys with that score are wanted (no tie across the boundary: the usual case), every key >= (score, row bits 0) is in and the four
        // row passes have nothing to decide: half of every select's passes.
        if (pass == 3 && same == need) break;
    }
    // prefix is now the kp-th largest key; keys are unique, so exactly kp keys are >= prefix
    if (tid == 0) sh.out = 0;
    __syncthreads();
    for (unsigned i = tid; i < n; i += NT) {
        const uint64_t k = staged ? sh.key[i] : cand_key(cv.at(i));
        if (k >= prefix) {                                            // (a key is its entry: score bits from the ordered form, row from the low word)
            const unsigned s = atomicAdd(&sh.out, 1u);
            if (s < 128) sh.keep[s] = make_uint2(__float_as_uint(f32_unorder((uint32_t)(k >> 32))), 0xffffffffu - (uint32_t)k);
        }
    }
    __syncthreads();
    if (tid < kp) cand[tid] = sh.keep[tid];
    if (tid == 0) {
        count[q] = (unsigned)kp;
        tau[q] = f32_unorder((uint32_t)(prefix >> 32));
    }
}

__global__ void __launch_bounds__(256) select_kernel(uint2 *cand_all, unsigned *count, uint2 *cand8, unsigned *count8, float *tau, unsigned *flags, unsigned capq, int kp)
{
    __shared__ SelectShared sh;
    select_block<256>(sh, cand_all, count, cand8, count8, tau, flags, capq, kp, blockIdx.x);
}

int mips_launch_select(uint2 *cand, unsigned *count, uint2 *cand8, unsigned *count8, float *tau, unsigned *flags, unsigned capq, int kp, int n_q,
                       hipStream_t stream)
{
    hipLaunchKernelGGL(select_kernel, dim3(n_q), dim3(256), 0, stream, cand, count, cand8, count8, tau, flags, capq, kp);
    return LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------------
// finalize: exact integer re-scoring of <= kp candidates, canonical (fp16 score desc, row asc)
// order, proof that no pruned row can enter the top-k, output
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void exact_dot_wave(const char *e_tiled, int64_t row, const uint16_t *qrow, int nseg, int lane, int64_t &lo_out,
                                               int64_t &hi_out)
{
    int64_t lo = 0, hi = 0;
    for (int seg = lane; seg < nseg; seg += 64) {
        const uint4 ev = *(const uint4 *)(e_tiled + tiled_seg_offset(row, seg, nseg >> 2));
        const uint4 qv = *(const uint4 *)(qrow + seg * 8);
        const uint32_t ew[4] = {ev.x, ev.y, ev.z, ev.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            exact_mac(lo, hi, half_fix((uint16_t)(ew[j] & 0xffff)), half_fix((uint16_t)(qw[j] & 0xffff)));
            exact_mac(lo, hi, half_fix((uint16_t)(ew[j] >> 16)), half_fix((uint16_t)(qw[j] >> 16)));
        }
    }
    lo_out = wave_sum_i64(lo);
    hi_out = wave_sum_i64(hi);
}

// Four candidates of one wave at a time (dim <= 1024: a row is <= 2 segments per lane): all eight row loads go out before the first is
// used.  One candidate after the other, each of a wave's 16 - 32 candidates paid a full memory latency for its scattered 16-byte row segments
// (r04: ~50 of the finalize launch's 82 us on an N / 8 shard); the integer arithmetic itself is a few hundred instructions per candidate.
__device__ __forceinline__ void exact_dot_wave_x4(const char *e_tiled, const unsigned (&rows)[4], int n_valid, const uint16_t *qrow, int nseg, int lane,
                                                  int64_t (&lo_out)[4], int64_t (&hi_out)[4])
{
    const bool two = lane + 64 < nseg, one = lane < nseg;
    uint4 ev[4][2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        ev[c][0] = ev[c][1] = make_uint4(0, 0, 0, 0);
        if (c < n_valid) {
            if (one) ev[c][0] = *(const uint4 *)(e_tiled + tiled_seg_offset((int64_t)rows[c], lane, nseg >> 2));
            if (two) ev[c][1] = *(const uint4 *)(e_tiled + tiled_seg_offset((int64_t)rows[c], lane + 64, nseg >> 2));
        }
    }
    uint4 qv[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    if (one) qv[0] = *(const uint4 *)(qrow + lane * 8);
    if (two) qv[1] = *(const uint4 *)(qrow + (lane + 64) * 8);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int64_t lo = 0, hi = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t ew[4] = {ev[c][h].x, ev[c][h].y, ev[c][h].z, ev[c][h].w}, qw[4] = {qv[h].x, qv[h].y, qv[h].z, qv[h].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {                          // (absent segments hold zeros: mantissa 0, nothing added)
                exact_mac(lo, hi, half_fix((uint16_t)(ew[j] & 0xffff)), half_fix((uint16_t)(qw[j] & 0xffff)));
                exact_mac(lo, hi, half_fix((uint16_t)(ew[j] >> 16)), half_fix((uint16_t)(qw[j] >> 16)));
            }
        }
        lo_out[c] = wave_sum_i64(lo);
        hi_out[c] = wave_sum_i64(hi);
    }
}

// LEAD: what the block does before the exact re-score -- 0: nothing, the list is final; 1: the select behind the last scan segment; 2: the
// deferred pass of the int8 segments, then that select (FINISH_THREADS threads: the pass is a gather of whole rows, 16 waves keep 64 of a
// query's rows in flight, and two such blocks with their SelectShared fit a CU).
#define FINISH_THREADS 1024
template <int LEAD>
__global__ void __launch_bounds__(LEAD == 2 ? FINISH_THREADS : 256) finalize_kernel(FinalizeParams p)
{
    constexpr int NT = LEAD == 2 ? FINISH_THREADS : 256, NW = NT / 64;
    __shared__ uint64_t fkey[128];
    __shared__ uint32_t sh_kth;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (LEAD != 0) {
        __shared__ SelectShared sel;
        if constexpr (LEAD == 2) {
            // The deferred pass: tau_q, from the select behind the last segment, is the tightest threshold the search will have.  A pending
            // entry with U < tau_q is dropped unread -- its fp32 score is below tau_q like that of a row the scan pruned --, the others get
            // their fp32 score and go behind the main list's kp entries (at most kp + PENDCAP < capq), where the select below finds them.
            // All of the list's entries are loaded at once and the kept rows compacted into ONE work list (where the select stages its keys
            // afterwards: PENDCAP words of its 64 KiB), so the gather runs without a barrier between its rows.
            __shared__ unsigned sh_w[NW];
            unsigned *const sh_row = (unsigned *)sel.key;
            static_assert(PENDCAP * sizeof(unsigned) <= sizeof(sel.key) && PENDCAP % NT == 0, "the work list holds a whole pending list");
            unsigned np = p.pcount[q];
            if (np > PENDCAP) np = PENDCAP;
            unsigned next = p.count[q];
            if (next > p.capq) next = p.capq;
            const float tq = p.tau[q];
            const uint2 *const pq = p.pend + (size_t)q * PENDCAP;
            uint2 *const main_list = (uint2 *)p.cand + (size_t)q * p.capq;
            const unsigned capq = p.capq;
            uint2 e[PENDCAP / NT];
#pragma unroll
            for (unsigned r = 0; r < PENDCAP / NT; ++r) { const unsigned i = r * NT + tid; e[r] = i < np ? pq[i] : make_uint2(0u, 0u); }
            unsigned n_keep = 0;
#pragma unroll
            for (unsigned r = 0; r < PENDCAP / NT; ++r) {
                if (r * NT >= np) break;                                      // (block-uniform)
                const bool keep = r * NT + tid < np && !(__uint_as_float(e[r].x) < tq);
                unsigned n_round;
                const unsigned w = block_rank<NW>(keep, sh_w, n_round);
                if (keep) sh_row[n_keep + w] = e[r].y;
                n_keep += n_round;
            }
            __syncthreads();
            rescore_worklist<NW>(p.e_tiled, (const uint4 *)p.queries + (size_t)q * (p.dim / 8), p.dim / 8, sh_row, n_keep,
                                 [&](unsigned j) { return next + j < capq ? main_list + next + j : nullptr; });
            next += n_keep;
            if (tid == 0) ((unsigned *)p.count)[q] = next;
            __threadfence_block();
            __syncthreads();
        }
        // the select that follows the LAST scan segment, run by the block that consumes its result (one launch less per search; the list, its
        // count and tau go through global memory as between two kernels: the fence orders them for this block's own reads below)
        select_block<NT>(sel, (uint2 *)p.cand, (unsigned *)p.count, p.cand8, p.count8, (float *)p.tau, p.flags, p.capq, p.kp, q);
        __threadfence_block();
        __syncthreads();
    }
    const uint2 *cand = p.cand + (size_t)q * p.capq;
    unsigned cnt = p.count[q];
    if (cnt > (unsigned)p.kp) cnt = p.kp;
    const int nseg = p.dim / 8;
    const uint16_t *qrow = p.queries + (size_t)q * p.dim;

    if (nseg <= 128) {
        for (unsigned j0 = wave; j0 < cnt; j0 += 4 * NW) {                    // this wave's candidates j0, j0 + NW, j0 + 2 NW, j0 + 3 NW together
            unsigned rows[4];
            int nv = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) { const unsigned j = j0 + NW * c; rows[c] = j < cnt ? cand[j].y : 0u; nv += j < cnt; }
            int64_t lo[4], hi[4];
            exact_dot_wave_x4(p.e_tiled, rows, nv, qrow, nseg, lane, lo, hi);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned j = j0 + NW * c;
                if (j < cnt && lane == 0) {
                    const uint32_t ord = p.f32 ? f32_order(fixed_to_float(lo[c], hi[c])) : h16_order(fixed_to_half(lo[c], hi[c]));
                    fkey[j] = ((uint64_t)ord << 32) | (uint64_t)(0xffffffffu - rows[c]);
                }
            }
        }
    } else {
        for (unsigned j = wave; j < cnt; j += NW) {
            const unsigned row = cand[j].y;
            int64_t lo, hi;
            exact_dot_wave(p.e_tiled, (int64_t)row, qrow, nseg, lane, lo, hi);
            const uint32_t ord = p.f32 ? f32_order(fixed_to_float(lo, hi)) : h16_order(fixed_to_half(lo, hi));
            if (lane == 0) fkey[j] = ((uint64_t)ord << 32) | (uint64_t)(0xffffffffu - row);
        }
    }
    if (tid == 0) sh_kth = 0;
    __syncthreads();

    const unsigned kk = cnt < (unsigned)p.k ? cnt : (unsigned)p.k;
    if ((unsigned)tid < cnt) {
        const uint64_t mine = fkey[tid];
        unsigned rank = 0;
        for (unsigned i = 0; i < cnt; ++i) rank += (fkey[i] > mine);
        if (rank < kk) {
            const uint32_t row = 0xffffffffu - (uint32_t)mine;
            const size_t o = (size_t)q * p.k + rank;
            const int64_t grow = p.row_base + (int64_t)row;
            const int32_t gid = p.ids ? p.ids[row] : (int32_t)grow;
            if (p.out_rec) {
                const uint32_t bits = p.f32 ? __float_as_uint(f32_unorder((uint32_t)(mine >> 32))) : (uint32_t)h16_unorder((uint32_t)(mine >> 32));
                p.out_rec[o] = make_uint4((uint32_t)grow, (uint32_t)((uint64_t)grow >> 32), (uint32_t)gid, bits);
            } else {
                if (p.f32) ((float *)p.out_dist)[o] = f32_unorder((uint32_t)(mine >> 32));
                else ((uint16_t *)p.out_dist)[o] = h16_unorder((uint32_t)(mine >> 32));
                p.out_row[o] = grow;
                p.out_idx[o] = gid;
            }
            if (rank == kk - 1) sh_kth = (uint32_t)(mine >> 32);
        }
    }
    for (unsigned j = kk + tid; j < (unsigned)p.k; j += NT) { // shard holds fewer than k rows
        const size_t o = (size_t)q * p.k + j;
        if (p.out_rec) { p.out_rec[o] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, p.f32 ? 0xff800000u : 0xfc00u); continue; }
        if (p.f32) ((float *)p.out_dist)[o] = -INFINITY; else ((uint16_t *)p.out_dist)[o] = 0xfc00;
        p.out_row[o] = -1; p.out_idx[o] = -1;
    }
    __syncthreads();
    if (tid == 0 && p.n_rows > (int64_t)cnt) {
        // rows outside the candidate list have MFMA score S~ <= tau (the kp-th best S~), hence exact
        // score <= tau + eps with eps >= |S~ - exact| for a dim-term fp32 accumulation;
        // if even that bound rounds below the k-th canonical score the top-k is proven.
        bool ok = (cnt == (unsigned)p.kp) && (kk == (unsigned)p.k);
        if (ok) {
            const float eps = (float)p.dim * 2.3841858e-07f /* 2^-22 */ * p.qnorm[q] * (sqrtf(*p.emax_sq) * 1.001f);
            const float bound = p.tau[q] + eps * 1.0001f;
            // fp32 mode: a pruned row's exact score is <= bound (a float), so its RNE_fp32 is <= bound as well
            ok = (p.f32 ? f32_order(bound) : h16_order(f32_to_h16_roundup(bound))) < sh_kth;
        }
        if (!ok) atomicOr(&p.flags[q], 1u);
    }
}

int mips_launch_finalize(const FinalizeParams &p, bool select_first, hipStream_t stream)
{
    if (p.pend && (!select_first || !p.pcount)) return -1;
    if (p.pend) hipLaunchKernelGGL(finalize_kernel<2>, dim3(p.n_q), dim3(FINISH_THREADS), 0, stream, p);
    else if (select_first) hipLaunchKernelGGL(finalize_kernel<1>, dim3(p.n_q), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(finalize_kernel<0>, dim3(p.n_q), dim3(256), 0, stream, p);
    return LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------------
// shard merge: [S, n_q, k] per-shard canonical lists -> [n_q, k], (score desc, global row asc)
// ------------------------------------------------------------------------------------------------
#define MERGE_MAX 4096
// Where the per-shard lists come from: three arrays, or the gathered 16-byte records (FinalizeParams::out_rec) -- what a sharded search
// exchanges in its ONE all-gather is the finalize kernel's own output, and the merge reads the gathered buffer as it arrives, no casts /
// stacks between.  Same keys, same order, same outputs from both.
template <class Fmt>
struct SlotArrays {
    const typename Fmt::stored_t *dist;
    const int32_t *idx;
    const int64_t *rows;
    __device__ __forceinline__ int64_t row(size_t i) const { return rows[i]; }
    __device__ __forceinline__ typename Fmt::stored_t score(size_t i) const { return dist[i]; }
    __device__ __forceinline__ int32_t id(size_t i) const { return idx[i]; }
};
template <class Fmt>
struct SlotRecords {
    const uint4 *rec;
    __device__ __forceinline__ int64_t row(size_t i) const { const uint4 r = rec[i]; return (int64_t)(((uint64_t)r.y << 32) | r.x); }
    __device__ __forceinline__ typename Fmt::stored_t score(size_t i) const { return Fmt::from_bits(rec[i].w); }
    __device__ __forceinline__ int32_t id(size_t i) const { return (int32_t)rec[i].z; }
};

template <class Fmt, class Source>
__global__ void __launch_bounds__(256) merge_kernel(Source in, int n_shards, int n_q, int k, typename Fmt::stored_t *out_dist, int32_t *out_idx,
                                                    int64_t *out_row)
{
    __shared__ uint64_t key[MERGE_MAX];
    __shared__ unsigned nvalid;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int n = n_shards * k;
    if (tid == 0) nvalid = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int s = i / k, j = i - s * k;
        const size_t src = ((size_t)s * n_q + q) * k + j;
        const int64_t row = in.row(src);
        uint64_t kv = 0;
        if (row >= 0) {
            kv = Fmt::merge_key(in.score(src), row);
            atomicAdd(&nvalid, 1u);
        }
        key[i] = kv;
    }
    __syncthreads();
    const unsigned nv = nvalid;
    for (int i = tid; i < n; i += 256) {
        const uint64_t mine = key[i];
        if (mine == 0) continue;
        unsigned rank = 0;
        for (int t = 0; t < n; ++t) rank += (key[t] > mine);
        if (rank < (unsigned)k) {
            const int s = i / k, j = i - s * k;
            const size_t src = ((size_t)s * n_q + q) * k + j, o = (size_t)q * k + rank;
            out_dist[o] = in.score(src); out_idx[o] = in.id(src); out_row[o] = in.row(src);
        }
    }
    for (unsigned j = nv + tid; j < (unsigned)k; j += 256) {
        const size_t o = (size_t)q * k + j;
        out_dist[o] = Fmt::pad(); out_idx[o] = -1; out_row[o] = -1;
    }
}

template <class Fmt, class Source>
static int launch_merge(Source in, int n_shards, int n_q, int k, void *out_dist, int32_t *out_idx, int64_t *out_row, hipStream_t stream)
{
    if (n_shards * k > MERGE_MAX) return -4;
    hipLaunchKernelGGL((merge_kernel<Fmt, Source>), dim3(n_q), dim3(256), 0, stream, in, n_shards, n_q, k, (typename Fmt::stored_t *)out_dist, out_idx,
                       out_row);
    return LAUNCH_OK();
}

int mips_launch_merge(const void *dist_in, const int32_t *idx_in, const int64_t *row_in, int n_shards, int n_q, int k, int f32, void *out_dist,
                      int32_t *out_idx, int64_t *out_row, hipStream_t stream)
{
    if (f32) return launch_merge<ScoreF32>(SlotArrays<ScoreF32>{(const float *)dist_in, idx_in, row_in}, n_shards, n_q, k, out_dist, out_idx, out_row, stream);
    return launch_merge<ScoreH16>(SlotArrays<ScoreH16>{(const uint16_t *)dist_in, idx_in, row_in}, n_shards, n_q, k, out_dist, out_idx, out_row, stream);
}

int mips_launch_merge_records(const uint4 *rec_in, int n_shards, int n_q, int k, int f32, void *out_dist, int32_t *out_idx, int64_t *out_row,
                              hipStream_t stream)
{
    if (f32) return launch_merge<ScoreF32>(SlotRecords<ScoreF32>{rec_in}, n_shards, n_q, k, out_dist, out_idx, out_row, stream);
    return launch_merge<ScoreH16>(SlotRecords<ScoreH16>{rec_in}, n_shards, n_q, k, out_dist, out_idx, out_row, stream);
}

__global__ void __launch_bounds__(128) pack_records_kernel(const void *dist, const int32_t *idx, const int64_t *row, const int32_t *sel, int k,
                                                           int f32, uint4 *rec)
{
    const int q = sel[blockIdx.x];
    for (int j = threadIdx.x; j < k; j += 128) {
        const size_t o = (size_t)q * k + j;
        const int64_t r = row[o];
        const uint32_t bits = f32 ? ScoreF32::bits(((const float *)dist)[o]) : ScoreH16::bits(((const uint16_t *)dist)[o]);
        rec[o] = make_uint4((uint32_t)r, (uint32_t)((uint64_t)r >> 32), (uint32_t)idx[o], bits);
    }
}

int mips_launch_pack_records(const void *dist, const int32_t *idx, const int64_t *row, const int32_t *sel, int n_sel, int k, int f32, uint4 *rec,
                             hipStream_t stream)
{
    if (n_sel < 1) return 0;
    hipLaunchKernelGGL(pack_records_kernel, dim3(n_sel), dim3(128), 0, stream, dist, idx, row, sel, k, f32, rec);
    return LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------------
// all-exact fallback: canonical ordered keys for EVERY row in integer arithmetic, then a radix
// threshold (one level per key byte) + ordered collection (first rows win ties).  Up to 8 queries
// per index pass.
// ------------------------------------------------------------------------------------------------
#define XQ 8
template <class Fmt>
__global__ void __launch_bounds__(256) exact_scores_kernel(const char *__restrict__ e_tiled, int64_t n_rows, int dim,
                                                           const uint16_t *__restrict__ queries, const int32_t *__restrict__ sel,
                                                           int n_sel, typename Fmt::key_t *__restrict__ keys)
{
    extern __shared__ int qfix[]; // [n_sel][dim] packed (mant << 8) | shift
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < n_sel * dim; i += 256) {
        const int f = i / dim, d = i - f * dim;
        const HalfFix hf = half_fix(queries[(size_t)sel[f] * dim + d]);
        qfix[i] = (hf.mant << 8) | hf.shift;
    }
    __syncthreads();
    const int nseg = dim / 8;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < n_rows; row += (int64_t)gridDim.x * 4) {
        int64_t lo[XQ], hi[XQ];
#pragma unroll
        for (int f = 0; f < XQ; ++f) { lo[f] = 0; hi[f] = 0; }
        for (int seg = lane; seg < nseg; seg += 64) {
            const uint4 ev = *(const uint4 *)(e_tiled + tiled_seg_offset(row, seg, nseg >> 2));
            const uint32_t ew[4] = {ev.x, ev.y, ev.z, ev.w};
            HalfFix ef[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) { ef[2 * j] = half_fix((uint16_t)(ew[j] & 0xffff)); ef[2 * j + 1] = half_fix((uint16_t)(ew[j] >> 16)); }
#pragma unroll
            for (int f = 0; f < XQ; ++f) {
                if (f < n_sel) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int pq = qfix[f * dim + seg * 8 + j];
                        HalfFix qf; qf.mant = pq >> 8; qf.shift = pq & 0xff;
                        exact_mac(lo[f], hi[f], ef[j], qf);
                    }
                }
            }
        }
#pragma unroll
        for (int f = 0; f < XQ; ++f) {
            if (f < n_sel) {
                const int64_t l = wave_sum_i64(lo[f]), h = wave_sum_i64(hi[f]);
                if (lane == 0) keys[(size_t)f * n_rows + row] = Fmt::fixed_key(l, h);
            }
        }
    }
}

template <class Fmt>
static int launch_exact_scores(const char *e_tiled, int64_t n_rows, int dim, const uint16_t *queries, const int32_t *sel, int n_sel, void *keys,
                               hipStream_t stream)
{
    if (n_sel > XQ) return -1;
    int64_t nb = (n_rows + 3) / 4;
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(exact_scores_kernel<Fmt>, dim3((unsigned)nb), dim3(256), (size_t)n_sel * dim * sizeof(int), stream, e_tiled, n_rows, dim,
                       queries, sel, n_sel, (typename Fmt::key_t *)keys);
    return LAUNCH_OK();
}

int mips_launch_exact_scores(const char *e_tiled, int64_t n_rows, int dim, const uint16_t *queries, const int32_t *sel, int n_sel, int f32, void *keys,
                             hipStream_t stream)
{
    return f32 ? launch_exact_scores<ScoreF32>(e_tiled, n_rows, dim, queries, sel, n_sel, keys, stream)
               : launch_exact_scores<ScoreH16>(e_tiled, n_rows, dim, queries, sel, n_sel, keys, stream);
}

#define XS_THREADS 1024
#define XS_R 8
template <class Fmt>
__global__ void __launch_bounds__(XS_THREADS) exact_select_kernel(const typename Fmt::key_t *__restrict__ keys, int64_t n_rows, int64_t row_base,
                                                                  const int32_t *__restrict__ sel, int k, const int32_t *__restrict__ ids,
                                                                  typename Fmt::stored_t *out_dist, int32_t *out_idx, int64_t *out_row, unsigned *flags)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned sh_digit, sh_need, sh_above, sh_wsum[XS_THREADS / 64];
    __shared__ uint64_t okey[128];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const typename Fmt::key_t *hk = keys + (size_t)f * n_rows;
    const unsigned keff = (int64_t)k < n_rows ? (unsigned)k : (unsigned)n_rows;

    // radix threshold, one level per key byte, most significant first: after a level the k-th key is known to start with `prefix`
    constexpr int TOP = 8 * (int)sizeof(typename Fmt::key_t) - 8;
    uint32_t prefix = 0;
    unsigned need = keff;
#pragma unroll
    for (int sh = TOP; sh >= 0; sh -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int64_t i = tid; i < n_rows; i += XS_THREADS) {
            const uint32_t v = hk[i];
            if (sh == TOP || (v >> (sh + 8)) == (prefix >> (sh + 8))) atomicAdd(&hist[(v >> sh) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) pick_digit(hist, need, &sh_digit, &sh_need);
        __syncthreads();
        prefix |= sh_digit << sh;
        need = sh_need;
        __syncthreads();
    }
    const uint32_t T = prefix;                  // k-th canonical key
    const unsigned need_eq = need;              // how many rows with key == T belong to the top-k
    const unsigned n_above = keff - need_eq;
    if (tid == 0) sh_above = 0;
    __syncthreads();

    // collection in row order: all keys > T, and the first need_eq rows with key == T
    unsigned eq_done = 0;
    for (int64_t base = 0; base < n_rows; base += (int64_t)XS_THREADS * XS_R) {
        const int64_t r0 = base + (int64_t)tid * XS_R;
        unsigned eqm = 0, mycnt = 0;
#pragma unroll
        for (int j = 0; j < XS_R; ++j) {
            const int64_t r = r0 + j;
            const uint32_t v = r < n_rows ? hk[r] : 0;
            if (r < n_rows && v > T) { const unsigned s = atomicAdd(&sh_above, 1u); okey[s] = ((uint64_t)v << 32) | (uint64_t)(0xffffffffu - (uint32_t)r); }
            if (r < n_rows && v == T) { eqm |= 1u << j; ++mycnt; }
        }
        // block exclusive scan of mycnt in thread (= row) order
        unsigned incl = mycnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        if (lane == 63) sh_wsum[wave] = incl;
        __syncthreads();
        unsigned woff = 0, total = 0;
        for (int w = 0; w < XS_THREADS / 64; ++w) { const unsigned s = sh_wsum[w]; if (w < wave) woff += s; total += s; }
        unsigned rank = eq_done + woff + incl - mycnt;
#pragma unroll
        for (int j = 0; j < XS_R; ++j)
            if (eqm & (1u << j)) { if (rank < need_eq) okey[n_above + rank] = ((uint64_t)T << 32) | (uint64_t)(0xffffffffu - (uint32_t)(r0 + j)); ++rank; }
        eq_done += total;
        __syncthreads();
    }
    __syncthreads();
    const int qi = sel[f];
    if ((unsigned)tid < keff) {
        const uint64_t mine = okey[tid];
        unsigned rank = 0;
        for (unsigned i = 0; i < keff; ++i) rank += (okey[i] > mine);
        const uint32_t row = 0xffffffffu - (uint32_t)mine;
        const size_t o = (size_t)qi * k + rank;
        out_dist[o] = Fmt::unorder((uint32_t)(mine >> 32));
        out_row[o] = row_base + (int64_t)row;
        out_idx[o] = ids ? ids[row] : (int32_t)(row_base + (int64_t)row);
    }
    for (unsigned j = keff + tid; j < (unsigned)k; j += XS_THREADS) {
        const size_t o = (size_t)qi * k + j;
        out_dist[o] = Fmt::pad(); out_row[o] = -1; out_idx[o] = -1;
    }
    if (tid == 0) flags[qi] = 0;
}

template <class Fmt>
static int launch_exact_select(const void *keys, int64_t n_rows, int64_t row_base, const int32_t *sel, int n_sel, int k, const int32_t *ids,
                               void *out_dist, int32_t *out_idx, int64_t *out_row, unsigned *flags, hipStream_t stream)
{
    hipLaunchKernelGGL(exact_select_kernel<Fmt>, dim3(n_sel), dim3(XS_THREADS), 0, stream, (const typename Fmt::key_t *)keys, n_rows, row_base, sel, k,
                       ids, (typename Fmt::stored_t *)out_dist, out_idx, out_row, flags);
    return LAUNCH_OK();
}

int mips_launch_exact_select(const void *keys, int64_t n_rows, int64_t row_base, const int32_t *sel, int n_sel, int k, const int32_t *ids, int f32,
                             void *out_dist, int32_t *out_idx, int64_t *out_row, unsigned *flags, hipStream_t stream)
{
    return f32 ? launch_exact_select<ScoreF32>(keys, n_rows, row_base, sel, n_sel, k, ids, out_dist, out_idx, out_row, flags, stream)
               : launch_exact_select<ScoreH16>(keys, n_rows, row_base, sel, n_sel, k, ids, out_dist, out_idx, out_row, flags, stream);
}
