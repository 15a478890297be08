// emdr2_amd/csrc/mips_scan8i.hip -- the index scan of mips_scan8.hip on an int8 shadow image of the index: fused int8 MFMA GEMM  I = E8 Q8^T
// + integer threshold filter, for the long filter segments of a 129..512-query search.
//
// The scan is only a filter: it proposes candidates, the triage kernel below gives every likely winner the fp32 score of its fp16
// row before a select sees it and parks the other survivors under a rigorous upper bound (they are read only if that bound still reaches the
// final threshold), and finalize_kernel re-scores exactly and proves the result.  So the filter may be coarse as long as a rigorous
// bound on its error is added before a row is pruned.  Rows are quantised per 256-row block b (this kernel's row tile) with one scale
// s_b = max|e| / 127, queries per query with t_q = max|q| / 127; with the integer sum I of row r and query q
//     S = t_q s_b I + (q - t_q q8).e_r + t_q q8.(e_r - s_b e8_r)    =>    |S - t_q s_b I| <= a_q N_b + b_q D_b =: eps(q, b)
// (a_q = ||q - t_q q8||, b_q = ||t_q q8||, N_b = max ||e_r||, D_b = max ||e_r - s_b e8_r||, all rounded up).  A row is pruned iff
// I < Theta(q, b), Theta = floor((tau_q - eps) / (t_q s_b)) computed ONCE per item and query column with every rounding downwards, so the
// per-accumulator work is the fp16 kernel's: an integer max tree and a ballot.  I is exact (|I| <= dim * 127^2, far inside int32).
//
// Everything else is the kernel template of mips_scan8.h, which mips_scan8.hip describes: the same work item (256 rows x 256 queries), ring,
// slots, phases, barriers, partner coupling, survivor queue and sub-list protocol, instantiated here with Scan8Int8.  The int8 images have the fp16 images' geometry -- 64-byte rows, 16-byte groups XOR-swizzled with
// (row >> 2) & 3 -- with 64 k-values per chunk instead of 32, and a lane's v_mfma_i32_16x16x64_i8 operand is one 16-byte group like the fp16
// kernel's: half the K-tiles per item, half the bytes per MAC at every level.  A survivor's score word holds the INTEGER sum until
// mips_launch_triage has run.
#include "mips_scan8.h"
#include "mips_derived.h"

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));

struct Scan8iParams : Scan8Params {
    const float4 *blk;            // per 256-row block {s_b, N_b, D_b, -}
    const float4 *qc;             // per query {t_q, a_q, b_q, -}
};

// Theta(q, b): the largest integer bound that is certainly <= (tau - eps) / (t s).  Every step errs downwards (more survivors): eps carries
// 1e-4 relative slack over its three fp32 roundings, the difference and the quotient (v_rcp_f32: 1 ulp) 1e-6 / 1e-5 of their magnitude, then
// floor - 1.  tau = +inf (a padded query column) prunes everything; a zero scale, tau = -inf or anything not a number prunes nothing.
__device__ __forceinline__ int s8i_theta(float tau, float t, float a, float b, float s, float n, float d)
{
    if (tau == __builtin_inff()) return 0x7fffffff;
    const float ts = t * s;
    if (!(ts > 0.f)) return (int)0x80000000;
    const float eps = (a * n + b * d) * 1.0001f;
    float num = tau - eps;
    num -= fabsf(num) * 1e-6f;
    float x = num * __builtin_amdgcn_rcpf(ts);
    x -= fabsf(x) * 1e-5f;
    x = floorf(x) - 1.f;
    if (!(x > -2.0e9f)) return (int)0x80000000;
    if (x > 2.0e9f) return 0x7fffffff;
    return (int)x;
}

// The other direction, for a survivor with integer sum I: est = t s I and U(q, b, I) >= est + eps(q, b) + the fp32 accumulation slack of the
// re-score (dim 2^-22 ||q|| N_b, the form finalize_kernel uses; ||q|| <= a_q + b_q).  Every step errs UPWARDS: est carries 1e-6 relative slack
// over its three roundings (t s, the conversion of I, the product), eps and the slack 1e-4 over theirs, the sum 1e-6 over its additions.  So
// U < tau implies that the exact score AND the fp32 sum rescore_wave_x4 would form are below tau.  A zero scale gives est = 0, which is exact.
struct S8iBound { float est, eps, upper; };
__device__ __forceinline__ S8iBound s8i_upper(int isum, float t, float a, float b, float s, float n, float d, float dim)
{
    S8iBound r;
    r.est = t * s * (float)isum;
    r.eps = (a * n + b * d) * 1.0001f;
    const float slack = dim * 0x1p-22f * (a + b) * n * 1.0001f;
    const float u = r.est + fabsf(r.est) * 1e-6f + r.eps + slack;
    r.upper = u + fabsf(u) * 1e-6f;
    return r;
}

// The int8 instance: integer sums against Theta(q, b), formed once per item and query column from the query's and the block's constants.
struct Scan8Int8 {
    typedef Scan8iParams Params;
    typedef intx4 frag_t;
    typedef intx4 acc_t;
    typedef int val_t;
    typedef float4 QConst;                                      // {t_q, a_q, b_q}
    struct ItemConst { float s, n, d; };                        // {s_b, N_b, D_b}
    static __device__ __forceinline__ acc_t mfma(frag_t a, frag_t b, acc_t c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ QConst load_q(const Params &P, int q) { return P.qc[q < P.s.n_q ? q : 0]; }
    // the block's three floats are wave-uniform: scalar loads from the constant address space, which do not queue behind the DMA stream
    static __device__ __forceinline__ ItemConst load_item(const Params &P, int tile)
    {
        const __attribute__((address_space(4))) float *bk = (const __attribute__((address_space(4))) float *)(uintptr_t)(P.blk + tile);
        return {bk[0], bk[1], bk[2]};
    }
    static __device__ __forceinline__ int threshold(float tau, const QConst &qc, const ItemConst &ic) { return s8i_theta(tau, qc.x, qc.y, qc.z, ic.s, ic.n, ic.d); }
    static __device__ __forceinline__ int max2(int a, int b) { return max(a, b); }
    static __device__ __forceinline__ unsigned bits(int v) { return (unsigned)v; }
};

} // namespace

// ------------------------------------------------------------------------------------------------
// shadow image: int8 rows in the stripe-tiled geometry + per 256-row block {s_b, N_b, D_b}, built from the finished fp16 image
// ------------------------------------------------------------------------------------------------
namespace {

// One workgroup per 256-row block, one thread per row; the seal itself is seal_block_256 (mips_derived.h), here with the storing sink.
// Workgroup i seals block first_block + i and reads or writes nothing of any other block: a full seal is the range [0, n_blocks), an
// in-place row update re-seals the blocks it touched with the very same code: a range (emdr2_mips_update_rows) or the touched-block list
// of a scattered update (emdr2_mips_update_rows_scattered), see BlockRange / BlockList in mips_device.h.
template <class Blocks>
__global__ void __launch_bounds__(256) seal_shadow_kernel(const char *__restrict__ tiled, int nch, Blocks blocks, char *__restrict__ e8,
                                                          float4 *__restrict__ blk, unsigned *__restrict__ nonfinite)
{
    __shared__ float sh[4];
    int64_t block;
    if (!blocks.get(block)) return;
    StoreSeal sink{e8, blk, nonfinite};
    seal_block_256(tiled, nch, block, sh, sink);
}

// Triage of what one int8 segment appended.  New entries of query q: the eight sub-lists up to min(count8, SUBCAP) and the main list from `pre`
// to min(count, capq); the entries below `pre` were kept by the select before the segment and keep their scores bit for bit.  `pre` is kp: an
// int8 segment always follows a select over at least the dense segment's rows, which leaves exactly kp entries.  With est = t_q s_b I:
//   est + margin eps >= tau_q (the tau the segment was scanned with): a likely winner.  Its score word becomes the fp32 score, in place, so the
//     select that follows raises tau over the rows that matter;
//   otherwise: (U, row) goes to the query's pending list and the score word becomes -inf, which the select ranks below the kp finite entries
//     the main list holds.  finalize_kernel<2> (mips_aux.hip) reads the row at the end of the search only if U still reaches the final tau;
//   the pending list is full: re-scored in place like a likely winner.  Nothing is ever dropped here and no flag is raised.
// `margin` decides only who is read now and who (perhaps) later.  grid (9 lists, n_q); a block reserves its pending slots with ONE atomic.
__global__ void __launch_bounds__(256) triage_kernel(const char *__restrict__ tiled, const uint4 *__restrict__ queries, int nseg, uint2 *cand,
                                                     const unsigned *__restrict__ count, uint2 *cand8, const unsigned *__restrict__ count8, unsigned capq,
                                                     unsigned pre, const float4 *__restrict__ blk, const float4 *__restrict__ qc,
                                                     const float *__restrict__ tau, uint2 *pend, unsigned *pcount, float margin)
{
    __shared__ unsigned long long sh_def[CAPQ / 64];
    __shared__ unsigned sh4[4], sh_base, sh_row[256], sh_idx[256];
    const int q = blockIdx.y, list = blockIdx.x, tid = threadIdx.x;
    uint2 *ent;
    unsigned lo, hi;
    if (list < 8) {
        ent = cand8 + ((size_t)q * 8 + list) * SUBCAP; lo = 0; hi = count8[list * 512 + q];
        if (hi > SUBCAP) hi = SUBCAP;
    } else {
        ent = cand + (size_t)q * capq; lo = pre; hi = count[q];
        if (hi > capq) hi = capq;
        if (hi > CAPQ) hi = CAPQ;                              // (sh_def covers CAPQ entries; capq is CAPQ)
    }
    if (lo >= hi) return;
    const float4 c = qc[q];
    const float tq = tau[q], dimf = (float)(nseg * 8);
    uint2 *const pq = pend + (size_t)q * PENDCAP;
    auto deferred = [&](unsigned i, uint2 &e, float &upper) {
        e = ent[i];
        const float4 b = blk[e.y >> 8];
        const S8iBound r = s8i_upper((int)e.x, c.x, c.y, c.z, b.x, b.y, b.z, dimf);
        upper = r.upper;
        return !(r.est + margin * r.eps >= tq);
    };
    // pass 1: who is deferred (one ballot word per wave and 256 entries, which pass 2 reads back: the decision is taken once) and how many;
    // one atomic reserves the block's slots (the count may pass PENDCAP: readers clamp it)
    unsigned mine = 0;
    for (unsigned i0 = lo; i0 < hi; i0 += 256) {
        const unsigned i = i0 + tid;
        uint2 e; float u;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(i < hi && deferred(i, e, u));
        if ((tid & 63) == 0) { sh_def[((i0 - lo) >> 6) + (tid >> 6)] = m; mine += (unsigned)__popcll(m); }
    }
    if ((tid & 63) == 0) sh4[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) {
        const unsigned total = sh4[0] + sh4[1] + sh4[2] + sh4[3];
        sh_base = total ? atomicAdd(&pcount[q], total) : 0u;
    }
    __syncthreads();
    unsigned next = sh_base;
    // pass 2: 256 entries at a time
    const uint4 *qrow = queries + (size_t)q * nseg;
    for (unsigned i0 = lo; i0 < hi; i0 += 256) {
        const unsigned i = i0 + tid;
        uint2 e = make_uint2(0u, 0u);
        float u = 0.f;
        if (i < hi) deferred(i, e, u);
        const bool def = (sh_def[((i0 - lo) >> 6) + (tid >> 6)] >> (tid & 63)) & 1ull;
        unsigned n_def;
        const unsigned slot = next + block_rank<4>(def, sh4, n_def);
        next += n_def;
        const bool parked = def && slot < PENDCAP;
        if (parked) {
            pq[slot] = make_uint2(__float_as_uint(u), e.y);
            ent[i].x = 0xff800000u;
        }
        unsigned n_now;
        const unsigned w = block_rank<4>(i < hi && !parked, sh4, n_now);
        if (i < hi && !parked) { sh_row[w] = e.y; sh_idx[w] = i; }
        __syncthreads();
        rescore_worklist<4>(tiled, qrow, nseg, sh_row, n_now, [&](unsigned j) { const unsigned i = sh_idx[j]; return i < hi ? ent + i : nullptr; });
    }
}

} // namespace

int mips_launch_seal_shadow(const void *tiled, int dim, int64_t first_block, int64_t n_blocks, void *e8, float *blk, unsigned *nonfinite,
                            hipStream_t stream)
{
    if (n_blocks == 0) return 0;
    hipLaunchKernelGGL(seal_shadow_kernel<BlockRange>, dim3((unsigned)n_blocks), dim3(256), 0, stream, (const char *)tiled, dim / 32, BlockRange{first_block},
                       (char *)e8, (float4 *)blk, nonfinite);
    return LAUNCH_OK();
}

int mips_launch_seal_shadow_list(const void *tiled, int dim, const unsigned *touched, const unsigned *n_touched, unsigned grid, void *e8, float *blk,
                                 unsigned *nonfinite, hipStream_t stream)
{
    if (grid == 0) return 0;
    hipLaunchKernelGGL(seal_shadow_kernel<BlockList>, dim3(grid), dim3(256), 0, stream, (const char *)tiled, dim / 32, BlockList{touched, n_touched},
                       (char *)e8, (float4 *)blk, nonfinite);
    return LAUNCH_OK();
}

int mips_launch_triage(const ScanParams &p, const void *queries, unsigned pre, const float *blk, const float *qc, void *pend, unsigned *pcount,
                       float margin, hipStream_t stream)
{
    hipLaunchKernelGGL(triage_kernel, dim3(9, p.n_q), dim3(256), 0, stream, p.e_tiled, (const uint4 *)queries, p.nch * 4, p.cand, p.count, p.cand8,
                       p.count8, p.capq, pre, (const float4 *)blk, (const float4 *)qc, p.tau, (uint2 *)pend, pcount, margin);
    return LAUNCH_OK();
}

// Filter scan (mode 0) of rows [row_begin, row_end) on the shadow image, for a query image of `bn` = 256 or 512 rows; `p` is the fp16 scan's
// parameter block (p.nch = dim / 32).  -4 = not covered (mips_int8_covers, mips_plan.h: the plan gives such a segment to the fp16 kernels)
int mips_launch_scan8i(const ScanParams &p, const void *e8_tiled, const float *blk, const void *q8_tiled, const float *qc, int bn, int64_t row_begin,
                       int64_t row_end, int cus, unsigned *prog, hipStream_t stream)
{
    if (!mips_int8_covers(bn, p.nch, cus, row_begin, row_end)) return -4;
    Scan8iParams P;
    P.s = p;
    P.s.e_tiled = (const char *)e8_tiled;
    P.s.q_tiled = (const char *)q8_tiled;
    P.s.nch = p.nch / 2;                                      // 64-wide int8 chunks; a multiple of 4 (K-tiles come in pairs)
    P.blk = (const float4 *)blk;
    P.qc = (const float4 *)qc;
    return s8_launch<Scan8Int8>(P, bn, row_begin, row_end, cus, prog, stream);
}
