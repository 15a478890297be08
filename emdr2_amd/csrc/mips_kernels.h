// emdr2_amd/csrc/mips_kernels.h -- host-visible launch wrappers of the MIPS kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mips_device.h"
#include "mips_plan.h"
#include "device_attr.h"

#define CAPQ 16384u /* candidate slots per query (8 B each) */
#define SUBCAP 1024u /* ... plus 8 sub-lists of this many per query, one per XCD, filled by the persistent scan (mips_scan8.hip) */
#define PENDCAP 8192u /* ... plus this many pending entries (upper bound bits, row) per query: deferred survivors of the int8 segments (mips_scan8i.hip) */

struct ScanParams {
    const char *e_tiled;  // stripe-tiled index image
    const char *q_tiled;  // chunk-tiled queries: [nch][BN*64 B]
    const float *tau;     // [BN] pass iff score >= tau
    uint2 *cand;          // [BN][capq] (fp32 score bits, local row)
    unsigned *count;      // [BN]
    unsigned *flags;      // [n_q]
    float *dense_out;     // MODE 2
    int nch;              // dim / 32
    int tile_begin, tile_end; // workgroup tiles (BM rows each)
    int n_rows;           // valid rows of the shard
    int n_q;
    unsigned capq;
    uint2 *cand8;         // [BN][8][SUBCAP]: per-XCD candidate sub-lists of the persistent scan (nullptr: not used)
    unsigned *count8;     // [8][512]
    int dense_row0;       // MODE 1: first row of the dense segment
    int tune;             // bits (EMDR2_MIPS_TUNE, default 17): 1 = prio on MFMA phase, 2 = prio on load phase, 4 = DMA before reads, 16 = non-temporal index-row loads (+5 % in the HBM-bound regime)
    unsigned long long *trace; // ABL 9: s_memtime stamps [16 chunks][8 waves][10 points]
};

// variant: 0 = 128 rows x 512 queries, 1 = 256 x 256, 2 = 512 x 128 ; mode: see mips_scan.hip
int mips_launch_scan(int variant, int mode, const ScanParams &p, int grid, hipStream_t stream);
// production filter scan (mode 0) for 256- / 512-row query images in the persistent-GEMM pipeline (mips_scan8.hip); -4 = not covered
// (mips_persistent_covers, and mips_int8_covers for mips_launch_scan8i: mips_plan.h)
// `prog`: SCAN8_PROG_UINTS zeroed uints per launch (pair progress counters, one 256-byte line each) or nullptr
#define SCAN8_PROG_UINTS (256 * 64)
int mips_launch_scan8(const ScanParams &p, int bn, int64_t row_begin, int64_t row_end, int cus, unsigned *prog, hipStream_t stream);
// int8 shadow path (mips_scan8i.hip).  Shadow image: the stripe-tiled geometry with 64 int8 k-values per 64-byte row; table: one float4
// {s_b, N_b, D_b, -} per 256-row block; `nonfinite` is OR-ed with 1 if the fp16 image holds an inf / NaN (such a shard stays on fp16)
// Seals the 256-row blocks [first_block, first_block + n_blocks); the whole shard is [0, ceil(n_rows / 256)).
int mips_launch_seal_shadow(const void *tiled, int dim, int64_t first_block, int64_t n_blocks, void *e8, float *blk, unsigned *nonfinite,
                            hipStream_t stream);
// the same seal over a device list of blocks (a scattered row update): `grid` workgroups, workgroup i seals touched[i] if i < *n_touched
int mips_launch_seal_shadow_list(const void *tiled, int dim, const unsigned *touched, const unsigned *n_touched, unsigned grid, void *e8, float *blk,
                                 unsigned *nonfinite, hipStream_t stream);
// mips_launch_scan8 on the shadow image: survivors carry their INTEGER sum in the score word until mips_launch_triage has run
int mips_launch_scan8i(const ScanParams &p, const void *e8_tiled, const float *blk, const void *q8_tiled, const float *qc, int bn, int64_t row_begin,
                       int64_t row_end, int cus, unsigned *prog, hipStream_t stream);
// the entries an int8 segment appended (sub-lists, and the main list from `pre` on): fp32 scores (fp16 products of the fp16 image) for those whose
// estimate + margin * eps reaches tau; the others go to `pend` [n_q][PENDCAP] / `pcount` [n_q] (zeroed per search) with score word -inf; the
// finalize launch reads those whose bound still reaches the final tau (FinalizeParams::pend)
int mips_launch_triage(const ScanParams &p, const void *queries, unsigned pre, const float *blk, const float *qc, void *pend, unsigned *pcount,
                       float margin, hipStream_t stream);
// production filter scan, ping-pong wave schedule (mode 0 only)
int mips_launch_scan_pp(int variant, int depth, const ScanParams &p, int grid, hipStream_t stream);
// production filter scan for 512 queries, query operand streamed straight to registers (mode 0, variant 0 only)
int mips_launch_scan_q8(int abl, const ScanParams &p, int grid, hipStream_t stream);
// fragment-tiled query image for mips_launch_scan_q8: [chunk][wave 8][ks 2][ni 2][lane 64][16 B]
int mips_launch_pack_queries_frag(const void *queries, int n_q, int dim, void *q_frag, hipStream_t stream);
// timing experiments (variant 0, mode 0): see ABL in mips_scan.hip
int mips_launch_scan_ablate(int abl, const ScanParams &p, int grid, hipStream_t stream);

int mips_launch_pack_rows(const void *rows_rm, int64_t n_chunk, int dim, int64_t row_offset, void *tiled,
                          float *emax_sq, hipStream_t stream);
// in-place row updates: rows into the image without touching emax_sq; block_norm_sq[b] = max ||E[r]||^2 over block b's 256 rows for
// b in [first_block, first_block + n_blocks); *emax_sq = max of the table's n_blocks entries
// generation stamps of the two row writers (emdr2_mips_update_rows_stamped, _scattered_stamped): generation[row] = gen for every row written;
// with newest_wins a row whose stamp is above gen is left alone, image and stamp, and counted in *n_kept_newer (may be null).  A null
// RowStamp pointer launches the unstamped kernel, whose stamp argument is the empty NoStamp.
struct RowStamp {
    uint32_t *generation;
    uint32_t gen;
    int newest_wins;
    uint32_t *n_kept_newer;
};
struct NoStamp {};
template <bool STAMPED> struct StampArg { typedef NoStamp type; };
template <> struct StampArg<true> { typedef RowStamp type; };
int mips_launch_write_rows(const void *rows_rm, int64_t n_chunk, int dim, int64_t row_offset, void *tiled, const RowStamp *stamp, hipStream_t stream);
int mips_launch_block_norms(const void *tiled, int dim, int64_t first_block, int64_t n_blocks, float *block_norm_sq, hipStream_t stream);
int mips_launch_table_max(const float *block_norm_sq, int64_t n_blocks, float *emax_sq, hipStream_t stream);
// scattered row updates: rows_rm[i] into image row row_ids[i] (ids outside [0, n_rows_total) skipped); every touched 256-row block is
// claimed once through claimed[table blocks] (zeroed by the caller) and appended to touched[cap] through *n_touched (zeroed too);
// then the block norms of exactly the listed blocks
int mips_launch_write_rows_at(const void *rows_rm, const int64_t *row_ids, int64_t n_upd, int dim, int64_t n_rows_total, void *tiled, unsigned *claimed,
                              unsigned *n_touched, unsigned *touched, unsigned cap, const RowStamp *stamp, hipStream_t stream);
int mips_launch_block_norms_list(const void *tiled, int dim, const unsigned *touched, const unsigned *n_touched, unsigned grid, float *block_norm_sq,
                                 hipStream_t stream);
// rows_rm[i] = image row row_ids[i] - row_base if that lies in [0, n_rows), else zero bytes
int mips_launch_unpack_rows(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const int64_t *row_ids, int64_t n_out,
                            void *rows_rm, hipStream_t stream);
// the report of emdr2_mips_generation_stats (MIPS_GEN_WORDS = EMDR2_GEN_WORDS) over n_items items: local rows 0.. (global_rows null) or the
// entries of global_rows that fall into [row_base, row_base + n_rows); clears the report itself
#define MIPS_GEN_WORDS 37
int mips_launch_generation_stats(const uint32_t *generation, int64_t n_rows, int64_t row_base, const int64_t *global_rows, int64_t n_items,
                                 uint32_t now, uint64_t *report, hipStream_t stream);
// emdr2_mips_oldest_rows (mips_select.hip): the n_want oldest of the rows with generation[r] < below, as global rows in ascending order,
// -1 behind them; out_info as documented in include/emdr2_mips.h.  Six launches at most, phases ordered by launch boundaries alone.
// workspace: MIPS_OLDEST_WS_BYTES whatever n_rows is -- three digit histograms, the state words, one count pair per slab
#define MIPS_OLDEST_MAX_SLABS 512
#define MIPS_OLDEST_WS_BYTES ((2048 + 2048 + 1024 + 16 + 2 * MIPS_OLDEST_MAX_SLABS) * 4)
int mips_launch_oldest_rows(const uint32_t *generation, int64_t n_rows, int64_t row_base, uint32_t below, int64_t n_want, int64_t *out_rows,
                            uint64_t *out_info, void *workspace, hipStream_t stream);
// index snapshots: image rows [row_offset, row_offset + n_chunk) -> row-major fp16; their digest added / xor-ed into digest[0] / digest[1]
int mips_launch_export_rows(const void *tiled, int dim, int64_t row_offset, int64_t n_chunk, void *rows_rm, hipStream_t stream);
int mips_launch_digest_rows(const void *tiled, int dim, int64_t row_offset, int64_t n_chunk, int64_t row_base, uint64_t *digest, hipStream_t stream);
// the digest of the generation stamps of local rows [row_offset, row_offset + n_chunk), folded into digest[0] / digest[1] the same way
int mips_launch_digest_stamps(const uint32_t *generation, int64_t row_offset, int64_t n_chunk, int64_t row_base, uint64_t *digest, hipStream_t stream);
// incremental snapshots (mips_delta.hip): keys[r] = g(r) (+ h(r) with stamps) for local rows [row_offset, row_offset + n_chunk); and
// emdr2_mips_changed_rows: the rows whose key differs from base_keys[r], as global rows in ascending order, -1 behind them; out_info as
// documented in include/emdr2_mips.h.  Three launches (one with n_rows == 0), phases ordered by launch boundaries alone.
// workspace: mips_changed_rows_workspace_bytes(n_rows) -- per stripe a mask, a count and four digest words; five words per slab
#define MIPS_DELTA_MAX_SLABS 512
size_t mips_changed_rows_workspace_bytes(int64_t n_rows);
int mips_launch_row_keys(const void *tiled, int dim, int64_t row_offset, int64_t n_chunk, int64_t row_base, const uint32_t *generation, uint64_t *keys,
                         hipStream_t stream);
int mips_launch_changed_rows(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const uint32_t *generation, const uint64_t *base_keys,
                             int64_t cap, int64_t *out_rows, uint64_t *out_info, void *workspace, hipStream_t stream);
// index audit (mips_audit.hip): the report of emdr2_mips_audit for the padded image of n_rows rows; e8 / table null: no shadow;
// sealed_blocks = ceil(n_rows / 256), the blocks a seal covers; block_norm_sq may be null
struct AuditParams {
    const char *tiled, *e8;
    const float4 *table;
    const float *block_norm_sq, *emax_sq;
    unsigned long long *report;
    int64_t n_rows, row_base, sealed_blocks;
    int nch;
};
int mips_launch_audit(const AuditParams &p, hipStream_t stream);
// The start of a search, one launch that reads every query row once.  Always: queries row-major fp16 [n_q, dim] -> chunk-tiled image for `bn`
// rows (zero padded) + ||q||_2 upper bounds.  With `tau`: thresholds -inf, counts (dense_count for the n_q real queries), flags 0 and `n_zero`
// (a multiple of 4) zeroed uints at `zero` -- sub-list counts, pending counts, pair-progress counters.  With `q8_tiled`: the int8 query image
// [dim / 64][bn * 64 B] + per query float4 {t_q, a_q, b_q, -} for mips_launch_scan8i.
struct PrepareParams {
    const void *queries;
    int n_q, dim, bn;
    void *q_tiled;
    float *qnorm;
    float *tau;              // nullptr: no thresholds / counts / flags / zeroing (emdr2_mips_debug_scores)
    unsigned *count, *flags;
    unsigned dense_count;
    unsigned *zero;
    size_t n_zero;
    void *q8_tiled;          // nullptr: no int8 image
    float *qc;
};
int mips_launch_prepare(const PrepareParams &p, hipStream_t stream);
// keep the kp best candidates of every query (by (score desc,row asc)), publish tau = kp-th score
int mips_launch_select(uint2 *cand, unsigned *count, uint2 *cand8, unsigned *count8, float *tau, unsigned *flags, unsigned capq, int kp, int n_q,
                       hipStream_t stream);
// exact re-scoring of the surviving candidates, canonical order, validity proof, outputs
struct FinalizeParams {
    const char *e_tiled;
    const uint16_t *queries; // row-major [n_q, dim]
    const uint2 *cand;
    const unsigned *count;
    uint2 *cand8;            // per-XCD sub-lists of the last scan segment (select_first), or nullptr
    unsigned *count8;
    const float *tau;
    const float *qnorm;
    const float *emax_sq;
    const int32_t *ids;
    void *out_dist;          // uint16 fp16 bits, or float when f32
    int32_t *out_idx;
    int64_t *out_row;
    unsigned *flags;
    int64_t n_rows, row_base;
    int dim, n_q, k, kp;
    unsigned capq;
    int f32;                 // 1: FaissMIPSIndex-style scores RNE_fp32(exact dot), order (fp32 score desc, row asc)
    uint4 *out_rec;          // non-null: ONE 16-byte record per (query, slot) instead of the three arrays -- {row lo, row hi, idx, score bits
                             // (fp16 in the low half, or fp32)} -- written straight into the all-gather send buffer of a sharded search
    const uint2 *pend;       // non-null (with select_first): the deferred pass of the int8 segments runs first, in the same launch -- a pending
    const unsigned *pcount;  // entry whose bound still reaches tau gets its fp32 score and joins the main list behind its kp entries
};
int mips_launch_finalize(const FinalizeParams &p, bool select_first, hipStream_t stream);      // select_first: run the select of the last scan segment in the same launch
// k-way merge of [n_shards, n_q, k] per-shard canonical lists (f32: float scores, else fp16 bits); -4 = n_shards * k too large
int mips_launch_merge(const void *dist_in, const int32_t *idx_in, const int64_t *row_in, int n_shards, int n_q, int k, int f32, void *out_dist,
                      int32_t *out_idx, int64_t *out_row, hipStream_t stream);
// the same merge over gathered 16-byte records [n_shards, n_q, k] (FinalizeParams::out_rec)
int mips_launch_merge_records(const uint4 *rec_in, int n_shards, int n_q, int k, int f32, void *out_dist, int32_t *out_idx, int64_t *out_row,
                              hipStream_t stream);
// (dist, idx, row) rows sel[i] -> records rows sel[i] (queries re-done by the all-exact path)
int mips_launch_pack_records(const void *dist, const int32_t *idx, const int64_t *row, const int32_t *sel, int n_sel, int k, int f32, uint4 *rec,
                             hipStream_t stream);

// all-exact fallback: ordered keys [n_sel][n_rows] of <= 8 selected queries (uint16 of the fp16 score, or uint32 of the fp32 one when f32),
// then their canonical top-k
int mips_launch_exact_scores(const char *e_tiled, int64_t n_rows, int dim, const uint16_t *queries, const int32_t *sel, int n_sel, int f32, void *keys,
                             hipStream_t stream);
int mips_launch_exact_select(const void *keys, int64_t n_rows, int64_t row_base, const int32_t *sel, int n_sel, int k, const int32_t *ids, int f32,
                             void *out_dist, int32_t *out_idx, int64_t *out_row, unsigned *flags, hipStream_t stream);

// ------------------------------------------------------------------------------------------------
// device code of the int8 segments that two files share: query quantisation (prepare_kernel in mips_aux.hip) and row quantisation (the seal
// in mips_scan8i.hip), the fp32 re-score of survivors right behind a segment (triage_kernel there) and at the end of the search
// (finalize_kernel<2> here)
// ------------------------------------------------------------------------------------------------
// the int8 value of x under the scale 1 / inv: index rows per 256-row block (seal_shadow_kernel), queries per query (prepare_kernel)
__device__ __forceinline__ int quant8(float x, float inv)
{
    int v = (int)rintf(x * inv);
    return v > 127 ? 127 : (v < -127 ? -127 : v);              // (|x| <= 127 / inv up to rounding: the clamp never bites, and D_b is measured on the stored value anyway)
}

// fp32 scores of four (row, query) pairs at a time: the sum of the exact fp16 products of a row of the fp16 image and the query, a lane's
// segments in order, then the xor tree (any fp32 accumulation order satisfies the eps of DESIGN 3.3, so select, finalize and the proof run
// unchanged -- but every caller forms THIS sum, so which of them scores a row never shows in a score word).  All four rows' loads go out
// before the first is used; rows past n_valid repeat rows[0].
__device__ __forceinline__ void rescore_wave_x4(const char *__restrict__ tiled, const unsigned (&rows)[4], const uint4 *__restrict__ qrow, int nseg, int lane,
                                                float (&out)[4])
{
    const int nch = nseg >> 2;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int seg = lane; seg < nseg; seg += 64) {
        uint4 ev[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) ev[c] = *(const uint4 *)(tiled + tiled_seg_offset(rows[c], seg, nch));
        const half8 qv = __builtin_bit_cast(half8, qrow[seg]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const half8 e = __builtin_bit_cast(half8, ev[c]);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[c] += (float)e[j] * (float)qv[j];
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += __shfl_xor(s[c], o);
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = s[c];
}

// exclusive rank of the threads with `flag` among the block's NW waves, and their number (two barriers; `sh` is NW words)
template <int NW>
__device__ __forceinline__ unsigned block_rank(bool flag, unsigned *sh, unsigned &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(flag);
    const unsigned before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
    __syncthreads();                                           // (sh may still be read from the previous call)
    if (lane == 0) sh[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { const unsigned v = sh[w]; off += w < wave ? v : 0u; tot += v; }
    total = tot;
    return off + before;
}

// the work list sh_row[0, n) of a block of NW waves: fp32 score words, four per wave at a time; entry j goes to dst(j) unless that is null
template <int NW, class Dst>
__device__ __forceinline__ void rescore_worklist(const char *__restrict__ tiled, const uint4 *__restrict__ qrow, int nseg, const unsigned *sh_row, unsigned n,
                                                 const Dst &dst)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned j0 = 4 * wave; j0 < n; j0 += 4 * NW) {
        unsigned rows[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) rows[c] = sh_row[j0 + c < n ? j0 + c : j0];
        float sc[4];
        rescore_wave_x4(tiled, rows, qrow, nseg, lane, sc);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (lane == 0 && j0 + c < n) {
                uint2 *const d = dst(j0 + c);
                if (d) *d = make_uint2(__float_as_uint(sc[c]), rows[c]);
            }
    }
}
