// emdr2_amd/csrc/mips_select.hip -- the n oldest rows of a shard from its generation stamps (emdr2_mips_oldest_rows; the contract is in
// include/emdr2_mips.h).
//
// A radix select over the 32-bit stamps, most significant digit first, in three digits of 11 / 11 / 10 bits, then an ordered compaction:
//
//   oldest_init_kernel       clears the three histograms, the state words and the report
//   oldest_hist_kernel<0>    histogram of the top 11 bits of the ELIGIBLE stamps (stamp < below)
//   oldest_hist_kernel<1>    picks digit 0 from that histogram; histogram of the middle 11 bits of the eligible stamps that carry it
//   oldest_hist_kernel<2>    picks digit 1; histogram of the low 10 bits of the eligible stamps that carry both
//   oldest_count_kernel      picks digit 2: the cut stamp T and `take`, how many rows stamped exactly T belong to the set (>= 1).  Every
//                            workgroup counts the rows below T and the rows equal to T of ITS slab of consecutive rows
//   oldest_write_kernel      sums the per-slab counts in front of its own -- which gives its output offset and how many T rows precede it
//                            -- and stores its selected rows in slab order; fills the slots behind the set with -1, writes the report
//
// FIVE passes over the stamps (p = 5; the write pass skips every slab that holds no selected row).  No digit pass is skipped: which digits
// hold more than one bin is only known on the device, and a pass that ends at once still costs its launch.
//
// The phases are ordered by launch boundaries alone.  A pick is a function of a finished histogram, so every workgroup of the NEXT launch
// computes it for itself from the same words (2,048 of them: an 8 KiB read from L2 and one block scan) instead of waiting for a
// workgroup that would compute it for all: no workgroup ever waits on another, no look-back, no grid barrier, no ticket.  Workgroup 0
// stores what it picked for the launches behind it.  Histograms and counts are integer atomics / plain sums: the result is a function of
// the stamps alone, whatever order the workgroups run in; the slab size enters no output (positions are GLOBAL ranks).
//
// A thread keeps the run of equal bins it is in and adds it to the workgroup's LDS histogram with one atomic when the bin changes: real
// stamps are a few clustered values, where one atomic per row on one LDS word would serialise the whole wave (generation_stats_kernel
// does the same).
#include "mips_kernels.h"

enum {
    SEL_THREADS = 256,
    SEL_CHUNK = 4 * SEL_THREADS,           // rows a workgroup takes at a time: four per thread
    SEL_BINS01 = 2048, SEL_BINS2 = 1024,   // digits 0 and 1: 11 bits, digit 2: 10 bits
    // workspace, in 32-bit words
    WS_HIST0 = 0, WS_HIST1 = WS_HIST0 + SEL_BINS01, WS_HIST2 = WS_HIST1 + SEL_BINS01, WS_STATE = WS_HIST2 + SEL_BINS2,
    WS_COUNTS = WS_STATE + 16,             // uint2 {rows below T, rows equal to T} per slab
    WS_WORDS = WS_COUNTS + 2 * MIPS_OLDEST_MAX_SLABS,
    // state words
    ST_NONE = 0,                           // 1: nothing is selected (n_want == 0 or nothing eligible)
    ST_ELIGIBLE = 1, ST_SELECTED = 2,      // n_eligible, k = min(n_want, n_eligible)
    ST_PREFIX0 = 3, ST_K1 = 4,             // digit 0 of T; the rank of the cut among the eligible stamps that carry it (1-based)
    ST_PREFIX01 = 5, ST_K2 = 6,            // digits 0 and 1 of T (22 bits); the rank among those that carry both
    ST_T = 7, ST_TAKE = 8,                 // T; the rows stamped T that belong to the set
};
static_assert(WS_WORDS * sizeof(unsigned) == MIPS_OLDEST_WS_BYTES, "the workspace size mips_kernels.h announces");

// exclusive prefix of v over the block's 256 threads and the block's total (`sh`: 4 words; two barriers)
__device__ __forceinline__ unsigned block_scan_excl(unsigned v, unsigned *sh, unsigned &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    __syncthreads();                                           // (sh may still be read from the previous call)
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    unsigned off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) { const unsigned s = sh[w]; off += w < wave ? s : 0u; tot += s; }
    total = tot;
    return off + incl - v;
}

// The threshold pick of one digit.  k = min(want, the total of hist[NB]) is returned; for k >= 1: the bin b with (sum of the bins below b)
// < k <= (that sum + hist[b]), and k less that sum -- the rank of the cut inside the bin; for k == 0 both are 0.  Every thread of the
// block gets the result.
template <int NB>
__device__ __forceinline__ unsigned pick_digit(const unsigned *__restrict__ hist, unsigned want, unsigned *sh_scan, unsigned *sh_out, unsigned &bin,
                                               unsigned &k_in_bin, unsigned &total)
{
    constexpr int PER = NB / SEL_THREADS;
    unsigned h[PER], mine = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { h[j] = hist[threadIdx.x * PER + j]; mine += h[j]; }
    if (threadIdx.x == 0) { sh_out[0] = 0u; sh_out[1] = 0u; }  // (ordered before the store below by the scan's barriers)
    unsigned before = block_scan_excl(mine, sh_scan, total);
    const unsigned k = want < total ? want : total;
    if (before < k && k <= before + mine) {                    // (exactly one thread: the prefix sums are monotone and mine > 0 here)
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (before < k && k <= before + h[j]) { sh_out[0] = threadIdx.x * PER + j; sh_out[1] = k - before; }
            before += h[j];
        }
    }
    __syncthreads();
    bin = sh_out[0]; k_in_bin = sh_out[1];
    return k;
}

// the slab of workgroup w: rows [w * slab, min((w + 1) * slab, n_rows)); slab is a multiple of SEL_CHUNK
__device__ __forceinline__ void slab_of(int64_t n_rows, int64_t slab, int64_t &lo, int64_t &hi)
{
    lo = (int64_t)blockIdx.x * slab;
    hi = lo + slab < n_rows ? lo + slab : n_rows;
}

__global__ void __launch_bounds__(SEL_THREADS) oldest_init_kernel(unsigned *__restrict__ ws, unsigned long long *__restrict__ info)
{
    for (unsigned i = blockIdx.x * SEL_THREADS + threadIdx.x; i < WS_WORDS; i += gridDim.x * SEL_THREADS) ws[i] = 0u;
    if (blockIdx.x == 0 && threadIdx.x < 4) info[threadIdx.x] = threadIdx.x == 2 ? ~0ull : 0ull;
}

template <int D>
__global__ void __launch_bounds__(SEL_THREADS) oldest_hist_kernel(const uint32_t *__restrict__ generation, int64_t n_rows, int64_t slab, uint32_t below,
                                                                  unsigned n_want, unsigned *__restrict__ ws)
{
    constexpr int NB = D == 2 ? SEL_BINS2 : SEL_BINS01;
    __shared__ unsigned sh_hist[NB], sh_scan[4], sh_out[2];
    const int tid = threadIdx.x;
    unsigned *const state = ws + WS_STATE;
    unsigned prefix = 0;                                       // the digits of T above this one
    if (D == 1) {
        unsigned k_in, total;                                  // (the histogram's total is n_eligible)
        const unsigned k = pick_digit<SEL_BINS01>(ws + WS_HIST0, n_want, sh_scan, sh_out, prefix, k_in, total);
        if (blockIdx.x == 0 && tid == 0) {
            state[ST_NONE] = k == 0u; state[ST_ELIGIBLE] = total; state[ST_SELECTED] = k; state[ST_PREFIX0] = prefix; state[ST_K1] = k_in;
        }
        if (k == 0u) return;                                   // uniform: nothing to select, the launches behind this one only report
    } else if (D == 2) {
        if (state[ST_NONE]) return;                            // (written by the launch before this one; uniform)
        unsigned bin, k_in, total;
        pick_digit<SEL_BINS01>(ws + WS_HIST1, state[ST_K1], sh_scan, sh_out, bin, k_in, total);
        prefix = (state[ST_PREFIX0] << 11) | bin;
        if (blockIdx.x == 0 && tid == 0) { state[ST_PREFIX01] = prefix; state[ST_K2] = k_in; }
    }
    for (int b = tid; b < NB; b += SEL_THREADS) sh_hist[b] = 0u;
    __syncthreads();
    int64_t lo, hi;
    slab_of(n_rows, slab, lo, hi);
    unsigned run_bin = 0u, run = 0u;
    for (int64_t base = lo; base < hi; base += SEL_CHUNK) {
        uint32_t s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                          // (four loads in flight, each coalesced over the wave)
            const int64_t r = base + j * SEL_THREADS + tid;
            s[j] = r < hi ? generation[r] : 0xffffffffu;       // (never eligible: below <= 2^32 - 1)
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = s[j] < below && (D == 0 || (D == 1 ? s[j] >> 21 : s[j] >> 10) == prefix);
            if (!in) continue;
            const unsigned bin = D == 0 ? s[j] >> 21 : (D == 1 ? (s[j] >> 10) & 2047u : s[j] & 1023u);
            if (bin != run_bin) {
                if (run) atomicAdd(&sh_hist[run_bin], run);
                run_bin = bin; run = 0u;
            }
            ++run;
        }
    }
    if (run) atomicAdd(&sh_hist[run_bin], run);
    __syncthreads();
    unsigned *const hist = ws + (D == 0 ? WS_HIST0 : (D == 1 ? WS_HIST1 : WS_HIST2));
    for (int b = tid; b < NB; b += SEL_THREADS)
        if (sh_hist[b]) atomicAdd(&hist[b], sh_hist[b]);
}

__global__ void __launch_bounds__(SEL_THREADS) oldest_count_kernel(const uint32_t *__restrict__ generation, int64_t n_rows, int64_t slab,
                                                                   unsigned *__restrict__ ws)
{
    __shared__ unsigned sh_scan[4], sh_out[2], sh_lt, sh_eq;
    const int tid = threadIdx.x;
    unsigned *const state = ws + WS_STATE;
    if (state[ST_NONE]) return;                                // (the counts stay 0, as the init launch left them)
    unsigned bin, take, total;
    pick_digit<SEL_BINS2>(ws + WS_HIST2, state[ST_K2], sh_scan, sh_out, bin, take, total);
    const uint32_t T = (state[ST_PREFIX01] << 10) | bin;
    if (blockIdx.x == 0 && tid == 0) { state[ST_T] = T; state[ST_TAKE] = take; }
    if (tid == 0) { sh_lt = 0u; sh_eq = 0u; }
    __syncthreads();
    int64_t lo, hi;
    slab_of(n_rows, slab, lo, hi);
    unsigned lt = 0u, eq = 0u;                                 // (T is an eligible stamp: a stamp below it is eligible too)
    for (int64_t base = lo; base < hi; base += SEL_CHUNK) {
        uint32_t s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t r = base + j * SEL_THREADS + tid;
            s[j] = r < hi ? generation[r] : 0xffffffffu;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool valid = base + j * SEL_THREADS + tid < hi;
            lt += valid && s[j] < T; eq += valid && s[j] == T;
        }
    }
    if (lt) atomicAdd(&sh_lt, lt);
    if (eq) atomicAdd(&sh_eq, eq);
    __syncthreads();
    if (tid == 0) ((uint2 *)(ws + WS_COUNTS))[blockIdx.x] = make_uint2(sh_lt, sh_eq);
}

__global__ void __launch_bounds__(SEL_THREADS) oldest_write_kernel(const uint32_t *__restrict__ generation, int64_t n_rows, int64_t slab, int64_t row_base,
                                                                   unsigned n_want, const unsigned *__restrict__ ws, int64_t *__restrict__ out_rows,
                                                                   unsigned long long *__restrict__ info)
{
    __shared__ unsigned sh_scan[4], sh_lt, sh_eq;
    const int tid = threadIdx.x;
    const unsigned *const state = ws + WS_STATE;
    const bool none = state[ST_NONE] != 0u;
    const unsigned k = state[ST_SELECTED];
    const uint32_t T = state[ST_T];
    const unsigned take = state[ST_TAKE];
    // the slots behind the selected set; the report
    for (unsigned i = k + blockIdx.x * SEL_THREADS + tid; i < n_want; i += gridDim.x * SEL_THREADS) out_rows[i] = -1;
    if (blockIdx.x == 0 && tid == 0) {
        info[0] = k; info[1] = state[ST_ELIGIBLE]; info[2] = none ? ~0ull : (unsigned long long)T; info[3] = 0ull;
    }
    if (none) return;
    // rows below T / equal to T in the slabs in front of this one
    const uint2 *const counts = (const uint2 *)(ws + WS_COUNTS);
    if (tid == 0) { sh_lt = 0u; sh_eq = 0u; }
    __syncthreads();
    unsigned lt = 0u, eq = 0u;
    for (unsigned w = tid; w < blockIdx.x; w += SEL_THREADS) { const uint2 c = counts[w]; lt += c.x; eq += c.y; }
    if (lt) atomicAdd(&sh_lt, lt);
    if (eq) atomicAdd(&sh_eq, eq);
    __syncthreads();
    unsigned lt_before = sh_lt, eq_before = sh_eq;
    const uint2 mine = counts[blockIdx.x];
    if (mine.x == 0u && (mine.y == 0u || eq_before >= take)) return;       // uniform: no row of this slab is selected
    int64_t lo, hi;
    slab_of(n_rows, slab, lo, hi);
    for (int64_t base = lo; base < hi; base += SEL_CHUNK) {
        // slab order: thread t owns rows base + 4 t .. + 3, so ONE scan of the packed (below, equal) counts ranks the whole chunk
        const int64_t r0 = base + 4 * tid;
        uint32_t s[4];
        if (r0 + 4 <= hi && (((uintptr_t)(generation + r0)) & 15) == 0) {
            const uint4 v = *(const uint4 *)(generation + r0);
            s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = r0 + j < hi ? generation[r0 + j] : 0xffffffffu;
        }
        unsigned packed = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool valid = r0 + j < hi;
            packed += (valid && s[j] < T ? 1u : 0u) + (valid && s[j] == T ? 0x10000u : 0u);
        }
        unsigned total;
        const unsigned before = block_scan_excl(packed, sh_scan, total);    // (at most 1,024 of either kind in a chunk: 16 bits each)
        unsigned lt_b = lt_before + (before & 0xffffu), eq_b = eq_before + (before >> 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool valid = r0 + j < hi;
            const bool is_lt = valid && s[j] < T, is_eq = valid && s[j] == T;
            // the rank of this row among the selected ones: every row below T in front of it, and the T rows in front of it up to `take`
            const unsigned pos = lt_b + (eq_b < take ? eq_b : take);
            if ((is_lt || (is_eq && eq_b < take)) && pos < n_want) out_rows[pos] = row_base + r0 + j;
            lt_b += is_lt; eq_b += is_eq;
        }
        lt_before += total & 0xffffu; eq_before += total >> 16;
        if (eq_before >= take && lt_before == sh_lt + mine.x) break;        // uniform: every selected row of the slab is stored
    }
}

int mips_launch_oldest_rows(const uint32_t *generation, int64_t n_rows, int64_t row_base, uint32_t below, int64_t n_want, int64_t *out_rows,
                            uint64_t *out_info, void *workspace, hipStream_t stream)
{
    unsigned *ws = (unsigned *)workspace;
    unsigned long long *info = (unsigned long long *)out_info;
    hipLaunchKernelGGL(oldest_init_kernel, dim3(n_rows > 0 ? 8 : 1), dim3(SEL_THREADS), 0, stream, ws, info);
    if (n_rows > 0) {
        // slabs of whole chunks, at most MIPS_OLDEST_MAX_SLABS of them (two workgroups per CU): the per-slab counts stay one short read
        const int64_t chunks = (n_rows + SEL_CHUNK - 1) / SEL_CHUNK;
        const int64_t per = (chunks + MIPS_OLDEST_MAX_SLABS - 1) / MIPS_OLDEST_MAX_SLABS;
        const int64_t slab = per * SEL_CHUNK;
        const dim3 grid((unsigned)((n_rows + slab - 1) / slab)), block(SEL_THREADS);
        const unsigned want = (unsigned)n_want;
        hipLaunchKernelGGL(oldest_hist_kernel<0>, grid, block, 0, stream, generation, n_rows, slab, below, want, ws);
        hipLaunchKernelGGL(oldest_hist_kernel<1>, grid, block, 0, stream, generation, n_rows, slab, below, want, ws);
        if (n_want > 0) {                                      // (n_want == 0: the launch above has found nothing to select)
            hipLaunchKernelGGL(oldest_hist_kernel<2>, grid, block, 0, stream, generation, n_rows, slab, below, want, ws);
            hipLaunchKernelGGL(oldest_count_kernel, grid, block, 0, stream, generation, n_rows, slab, ws);
        }
        hipLaunchKernelGGL(oldest_write_kernel, grid, block, 0, stream, generation, n_rows, slab, row_base, want, (const unsigned *)ws, out_rows, info);
    }
    return LAUNCH_OK();
}
