// emdr2_amd/csrc/mips_scan8.hip -- the index scan for 129..512 queries per pass in the pipeline of the persistent GEMM (gemm8.hip): fused fp16 MFMA
// GEMM  S = E Q^T  + threshold filter, S never materialised.
//
// Replaces, like mips_scan.hip, the reference's dense  C = Q * E^T  + torch.topk (megatron/data/emdr2_index.py:281-295) for the filter
// segments (mode 0) of a search; same inputs (stripe-tiled index image, chunk-tiled query image, per-query thresholds) and the same
// survivor protocol (LDS queue -> per-query candidate buffers), so the select / finalize kernels downstream are unchanged and the results are
// bit-identical by construction (every (row, query) score is the same fp32 MFMA sum over k in the same order: chunks ascending, the four
// 16-wide k-steps of a K-tile ascending).
//
// What changes against mips_scan.hip (128 rows x 512 queries per workgroup, 32-wide chunks, 3-stage lockstep ring: 915 TFLOP/s, the LDS-DMA
// fill and the MFMA phase nearly additive):
//  * work item = 256 index rows x 256 queries (one half of the 512-query image): 64 KiB of L2->LDS fill per 8.4 MFLOP instead of 40 KiB per
//    4.2 MFLOP.  The two halves of a row tile are adjacent items, taken by two CUs of the same XCD in the same round: the index rows leave
//    HBM once, the partner reads them from L2.
//  * K-tile = 64 (two 8 KiB chunk images per stripe), 2 x 4 half-tile slots, four phases per K-tile with 8 MFMAs behind 12 / 4 / 8 / 0 fragment
//    reads and one half-tile of LDS-DMA six half-tiles ahead (vmcnt(8)), the two wave halves one barrier apart, persistent DMA stream across
//    items: the schedule of gemm8.hip, which the same measurements put at 1,300 TFLOP/s without an output epilogue.
//  * the epilogue is the filter: per accumulator block a max + one ballot in the common case (no survivor).
//  * the two workgroups that share a row tile pace themselves against each other through a progress counter (S8_COUPLE below): without it
//    they drift apart by more than the L2 holds and the index rows are fetched from the fabric 1.77 times; with it 1.015 times.
// LDS: 128 KiB operand ring + 32 KiB survivor queue.
#include "mips_scan8.h"

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

// The fp16 instance: the score is the fp32 MFMA sum itself and the threshold is the query's tau, so there is nothing to load per query or item.
struct Scan8Fp16 {
    typedef Scan8Params Params;
    typedef half8 frag_t;
    typedef floatx4 acc_t;
    typedef float val_t;
    struct QConst {};
    struct ItemConst {};
    static __device__ __forceinline__ acc_t mfma(frag_t a, frag_t b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ QConst load_q(const Params &, int) { return {}; }
    static __device__ __forceinline__ ItemConst load_item(const Params &, int) { return {}; }
    static __device__ __forceinline__ float threshold(float tau, QConst, ItemConst) { return tau; }
    static __device__ __forceinline__ float max2(float a, float b) { return fmaxf(a, b); }
    static __device__ __forceinline__ unsigned bits(float v) { return __float_as_uint(v); }
};

} // namespace

// Filter scan (mode 0) of rows [row_begin, row_end) for a query image of `bn` = 256 or 512 rows; -4 = not covered (mips_persistent_covers, mips_plan.h: the plan gives such a segment to mips_scan.hip)
int mips_launch_scan8(const ScanParams &p, int bn, int64_t row_begin, int64_t row_end, int cus, unsigned *prog, hipStream_t stream)
{
    Scan8Params P;
    P.s = p;
    return s8_launch<Scan8Fp16>(P, bn, row_begin, row_end, cus, prog, stream);
}
