// emdr2_amd/csrc/mips_scan8i.hip -- the index scan of mips_scan8.hip on an int8 shadow image of the index: fused int8 MFMA GEMM  I = E8 Q8^T
// + integer threshold filter, for the long filter segments of a 129..512-query search.
//
// The scan is only a filter: it proposes candidates, the re-score kernel below gives every survivor the fp32 score of its fp16
// row before a select sees it, and finalize_kernel re-scores exactly and proves the result.  So the filter may be coarse as long as a rigorous
// bound on its error is added before a row is pruned.  Rows are quantised per 256-row block b (this kernel's row tile) with one scale
// s_b = max|e| / 127, queries per query with t_q = max|q| / 127; with the integer sum I of row r and query q
//     S = t_q s_b I + (q - t_q q8).e_r + t_q q8.(e_r - s_b e8_r)    =>    |S - t_q s_b I| <= a_q N_b + b_q D_b =: eps(q, b)
// (a_q = ||q - t_q q8||, b_q = ||t_q q8||, N_b = max ||e_r||, D_b = max ||e_r - s_b e8_r||, all rounded up).  A row is pruned iff
// I < Theta(q, b), Theta = floor((tau_q - eps) / (t_q s_b)) computed ONCE per item and query column with every rounding downwards, so the
// per-accumulator work is the fp16 kernel's: an integer max tree and a ballot.  I is exact (|I| <= dim * 127^2, far inside int32).
//
// Everything else is mips_scan8.hip: the same work item (256 rows x 256 queries), ring, slots, phases, barriers, partner coupling, survivor
// queue and sub-list protocol.  The int8 images have the fp16 images' geometry -- 64-byte rows, 16-byte groups XOR-swizzled with
// (row >> 2) & 3 -- with 64 k-values per chunk instead of 32, and a lane's v_mfma_i32_16x16x64_i8 operand is one 16-byte group like the fp16
// kernel's: half the K-tiles per item, half the bytes per MAC at every level.  A survivor's score word holds the INTEGER sum until
// mips_launch_rescore has run.
#include "mips_device.h"
#include "mips_kernels.h"

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));

#define S8_BUF 65536
#define S8_SLOT 16384
#define S8_QCAP 2040              // survivor queue entries (16 B each); the counters sit behind them
#define S8_WCAP 255               // ... in eight wave-private regions: a wave reserves slots by adding to its OWN count, no LDS atomic, no round trip
#define S8_FLUSH_AT 128           // flush when some wave's region is half full

struct Scan8Params {
    ScanParams s;
    int t_begin, t_end;           // 256-row tiles
    int halves;                   // 256-query halves of the query image (1 or 2)
    int bn;                       // rows of the query image (256 or 512)
    int last_stripe;              // highest 128-row stripe that exists
    int total, per;               // items, items per XCD
    unsigned *prog;               // progress counters, one per pair of workgroups that share row tiles, 64 uints apart (zeroed by the caller), or nullptr
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

// A survivor's slot in query q's candidate set.  r04: one sub-list per XCD (ScanParams.cand8 / count8) and an atomic of WORKGROUP scope: it is
// performed by this XCD's L2 on a line no other XCD touches during the launch, instead of going out to the memory side like the agent-scope
// atomic on ONE counter per query did (eight L2s are not coherent among themselves: ~0.2 us each, 380,000 of them in the segment right after
// the dense one = 80 of its 215 us).  The select that follows a segment reads the main list and the eight sub-lists (mips_aux.hip).
__device__ __forceinline__ void s8_append(const ScanParams &p, unsigned xcc, unsigned q, unsigned score_bits, unsigned row)
{
    const unsigned slot = __hip_atomic_fetch_add(&p.count8[xcc * 512 + q], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (slot < SUBCAP) { p.cand8[((size_t)q * 8 + xcc) * SUBCAP + slot] = make_uint2(score_bits, row); return; }
    // r05: a full sub-list SPILLS into the query's main list (CAPQ entries, shared by all XCDs: agent-scope atomic) instead of dropping the
    // survivor.  An XCD owns a CONTIGUOUS range of the row sequence, so in an index whose neighbouring rows are similar (consecutive passages
    // of one article) a query's survivors of a segment pile up in ONE sub-list; before, 1,024 of them sent the query to the all-exact
    // path (a host sync + an integer pass over every row) although the other seven sub-lists and the 16,384-entry main list stood empty.
    // The count keeps growing past SUBCAP (the select clamps it); only a full MAIN list loses candidates and flags the query.
    const unsigned s2 = __hip_atomic_fetch_add(&p.count[q], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (s2 < p.capq) p.cand[(size_t)q * p.capq + s2] = make_uint2(score_bits, row);
}

// queue -> candidate sub-lists; cnt[w] = entries in wave w's region (all 512 threads take part: thread t drains region t >> 6)
__device__ __forceinline__ void s8_flush(const ScanParams &p, const char *qbuf, const unsigned *cnt, int tid, unsigned xcc)
{
    const int region = tid >> 6;
    unsigned m = ((const volatile __attribute__((address_space(3))) unsigned *)cnt)[region];
    if (m > S8_WCAP) m = S8_WCAP;
    for (unsigned i = tid & 63; i < m; i += 64) {
        const uint4 e = ((const uint4 *)qbuf)[region * S8_WCAP + i];
        s8_append(p, xcc, e.z, e.x, e.y);
    }
}

__global__ void __launch_bounds__(512) mips_scan8i_kernel(Scan8Params P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ScanParams &p = P.s;                                  // (p.nch counts 64-wide int8 chunks here)
    char *const qbuf = smem + 2 * S8_BUF;
    unsigned *const qcnt = (unsigned *)(qbuf + S8_QCAP * 16);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;                 // wave grid 2 (rows) x 4 (queries); wr is also the half that runs one barrier behind
    const int l31 = lane & 31, hi = lane >> 5;

    // ---- this workgroup's items: XCD x = id & 7 owns sequence positions [x * per, (x + 1) * per), its workgroups take them round-robin; an item
    // is (row tile, query half) with the half fastest, so both halves of a tile run at the same time on one L2
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, wg_per_xcd = gridDim.x >> 3;
    const int seq_lo = xcd * P.per;
    int seq_hi = seq_lo + P.per; if (seq_hi > P.total) seq_hi = P.total;
    const int first = seq_lo + slot;
    if (first >= seq_hi) return;
    const int my_count = (seq_hi - first + wg_per_xcd - 1) / wg_per_xcd;
    const int KT = p.nch >> 1;                                // K-tiles of 128 = pairs of 64-wide chunks; even (host)
    unsigned *const flagw = qcnt + 8;                          // LDS landing word of the partner-progress DMA (behind the eight region counts)
    if (tid < 8) qcnt[tid] = 0;
    if (tid == 0) *flagw = 0;
    unsigned wq = 0;                                           // entries in this wave's queue region (wave-uniform)
    // the XCD this workgroup really runs on (HW_REG_XCC_ID: id 20, bits 0..3), not the one its block id suggests: the sub-list protocol is
    // only correct if all appenders of a sub-list share an L2
    const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 7u;
    // the workgroups of an XCD stride the sequence by an even count (host) and `per` is even: a workgroup keeps ONE query half for all its items,
    // so its thresholds are loaded once (a load in the filter would wait out the whole DMA queue: vmcnt is in order)
    const int hq = P.halves == 2 ? first & 1 : 0;
    float4 qcv[4];                                             // {t_q, a_q, b_q} of the same four queries
    float tauv[4];                                             // the wave's four 16-query tiles: this lane's query of tile qt is wc * 64 + qt * 16 + l15
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        const int q = hq * 256 + wc * 64 + qt * 16 + ((lane & 3) * 4 + ((lane & 15) >> 2));      // (tile rows are permuted, see the fragment reads)
        tauv[qt] = q < p.n_q ? p.tau[q] : __builtin_inff();
        qcv[qt] = P.qc[q < p.n_q ? q : 0];
    }

    // ---- LDS-DMA addressing.  The operand images in HBM are LDS images already (mips_device.h: 64-byte rows, 16-byte groups XOR-swizzled with
    // (row >> 2) & 3), so every piece is a linear 1 KiB copy.  Half-tile slots:
    //   A_h (rows [64 h, 64 h + 64) of both stripes):  [stripe 2][chunk 2][64 rows x 64 B]     piece pa = stripe * 8 + chunk * 4 + quarter
    //   B_h (queries [32 h, 32 h + 32) of every wave):  [wave column 4][chunk 2][32 rows x 64 B] piece pb = wc * 4 + chunk * 2 + half
    // wave w moves pieces w and w + 8 of every half-tile.
    const int ja = (wave >> 2) & 1, qa = wave & 3;            // A pieces w, w + 8: stripes 0 / 1, chunk ja, quarter qa
    const int jb = (wave >> 1) & 1, qb = wave & 1;            // B pieces w, w + 8: wave columns w >> 2 and 2 + (w >> 2), chunk jb, half qb
    const uint32_t offA = (uint32_t)(ja * STRIPE_CHUNK_BYTES + qa * 1024 + lane * 16);
    const uint32_t q_stage = (uint32_t)P.bn * 64;             // bytes of one 32-wide chunk of the query image
    const uint32_t offB = (uint32_t)(jb * q_stage + ((wave >> 2) * 64) * 64 + qb * 1024 + lane * 16);
    // stage cursor (wave-uniform): item `s_i` of this workgroup's list, K-tile `s_kt`
    int s_i = 0, s_kt = 0;
    const char *sA0, *sA1, *sB;
    auto cursor_item = [&](int i) {
        if (i >= my_count) i = my_count - 1;                  // past the end: harmless re-reads keep the vmcnt arithmetic fixed
        const int pos = first + i * wg_per_xcd;
        const int tile = P.t_begin + (P.halves == 2 ? pos >> 1 : pos);
        int st0 = tile * 2, st1 = tile * 2 + 1;
        if (st0 > P.last_stripe) st0 = P.last_stripe;         // rows past the end of the shard: re-read the last stripe (masked by row < n_rows)
        if (st1 > P.last_stripe) st1 = P.last_stripe;
        sA0 = p.e_tiled + (size_t)st0 * p.nch * STRIPE_CHUNK_BYTES;
        sA1 = p.e_tiled + (size_t)st1 * p.nch * STRIPE_CHUNK_BYTES;
        sB = p.q_tiled + (size_t)hq * 256 * 64;
    };
    cursor_item(0);
#define S8_STAGE(T, SB)                                                                                                                   \
    do {                                                                                                                                  \
        char *dst_ = smem + (SB) * S8_BUF + (T) * S8_SLOT + wave * 1024;                                                                   \
        if ((T) == 0 || (T) == 3) {                                                                                                       \
            const uint32_t o_ = offA + ((T) == 3 ? 4096 : 0);                                                                             \
            __builtin_amdgcn_global_load_lds((gptr_t *)(sA0 + o_), (lptr_t *)dst_, 16, 0, 0);                                             \
            __builtin_amdgcn_global_load_lds((gptr_t *)(sA1 + o_), (lptr_t *)(dst_ + 8192), 16, 0, 0);                                    \
        } else {                                                                                                                          \
            const uint32_t o_ = offB + ((T) == 2 ? 32 * 64 : 0);                                                                          \
            __builtin_amdgcn_global_load_lds((gptr_t *)(sB + o_), (lptr_t *)dst_, 16, 0, 0);                                              \
            __builtin_amdgcn_global_load_lds((gptr_t *)(sB + o_ + 128 * 64), (lptr_t *)(dst_ + 8192), 16, 0, 0);                          \
        }                                                                                                                                 \
        if ((T) == 3) {                                                                                                                   \
            sA0 += 2 * STRIPE_CHUNK_BYTES; sA1 += 2 * STRIPE_CHUNK_BYTES; sB += 2 * q_stage;                                              \
            if (++s_kt == KT) { s_kt = 0; cursor_item(++s_i); }                                                                           \
        }                                                                                                                                 \
    } while (0)

    // ---- fragment reads for v_mfma_i32_16x16x64_i8: a lane holds row (query) l15 of a 16-row tile and k = 16 lq .. 16 lq + 15 of the 64-wide
    // chunk, i.e. the 16-byte group lq ^ ((row >> 2) & 3) of that row's 64 bytes: the addresses of mips_scan8.hip.
    // Operand lane l15 takes tile row prow = 4 (l15 & 3) + (l15 >> 2), not row l15: with consecutive rows on consecutive lanes every
    // ds_read_b128 of this pattern has a 2-way bank conflict on the 64-byte-row image (SQ_LDS_BANK_CONFLICT = half of SQ_LDS_IDX_ACTIVE;
    // tools/lds_conflict_probe.hip), with the rows of a tile dealt four apart none.  Output row m = 4 eq + r of a tile is then index row
    // 4 r + eq, output column e15 query 4 (e15 & 3) + (e15 >> 2): the filter below and the thresholds above follow.
    const int l15 = lane & 15, lq = lane >> 4;
    const int prow = (l15 & 3) * 4 + (l15 >> 2);
    const int frag_rd = prow * 64 + ((lq ^ ((prow >> 2) & 3)) << 4);
    const int a_rd = wr * 8192 + frag_rd;                       // + chunk * 4096 + row tile * 1024
    const int b_rd = wc * 4096 + frag_rd;                       // + chunk * 2048 + query tile * 1024
    intx4 av[2][4], b0v[4], b1v[4];                              // A: [chunk][16-row tile of the 64-row half]; B: [chunk * 2 + 16-query tile of the 32-query half]
#define S8_READ_A(BUF, MH)                                                                                                                \
    _Pragma("unroll") for (int c = 0; c < 2; ++c)                                                                                         \
        _Pragma("unroll") for (int rt = 0; rt < 4; ++rt)                                                                                  \
            av[c][rt] = *(const intx4 *)(smem + (BUF) * S8_BUF + ((MH) ? 3 * S8_SLOT : 0) + c * 4096 + rt * 1024 + a_rd)
#define S8_READ_B(BUF, NH, DST)                                                                                                           \
    _Pragma("unroll") for (int c = 0; c < 2; ++c)                                                                                         \
        _Pragma("unroll") for (int ct = 0; ct < 2; ++ct)                                                                                  \
            DST[2 * c + ct] = *(const intx4 *)(smem + (BUF) * S8_BUF + ((NH) ? 2 * S8_SLOT : S8_SLOT) + c * 2048 + ct * 1024 + b_rd)
    // rows of the MFMA result = index rows (A fragment first), columns = queries: a lane holds ONE query and 4 rows per accumulator tile
#define S8_MFMA(MH, NH, BV)                                                                                                               \
    _Pragma("unroll") for (int c = 0; c < 2; ++c)                                                                                         \
        _Pragma("unroll") for (int rt = 0; rt < 4; ++rt)                                                                                  \
            _Pragma("unroll") for (int ct = 0; ct < 2; ++ct)                                                                              \
                acc[4 * (MH) + rt][2 * (NH) + ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[c][rt], BV[2 * c + ct], acc[4 * (MH) + rt][2 * (NH) + ct], 0, 0, 0)
// first K-tile of a row tile: each accumulator's first MFMA takes C = 0 as an inline constant -- the accumulators are never cleared by
// separate instructions (128 v_mov per wave and item otherwise, inside the filter's VALU time)
#define S8_MFMA_Z(MH, NH, BV)                                                                                                             \
    _Pragma("unroll") for (int c = 0; c < 2; ++c)                                                                                         \
        _Pragma("unroll") for (int rt = 0; rt < 4; ++rt)                                                                                  \
            _Pragma("unroll") for (int ct = 0; ct < 2; ++ct)                                                                              \
                acc[4 * (MH) + rt][2 * (NH) + ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[c][rt], BV[2 * c + ct], c == 0 ? zero4 : acc[4 * (MH) + rt][2 * (NH) + ct], 0, 0, 0)
#define S8_SYNC_COMPUTE(BETWEEN, MFMAS)                                                                                                   \
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                                                    \
    __builtin_amdgcn_s_barrier();                                                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                                                                    \
    BETWEEN;                                                                                                                              \
    __builtin_amdgcn_s_setprio(1);                                                                                                        \
    MFMAS;                                                                                                                                \
    __builtin_amdgcn_s_setprio(0);                                                                                                        \
    __builtin_amdgcn_sched_barrier(0)
#define S8_BARRIER()                                                                                                                      \
    __builtin_amdgcn_s_barrier();                                                                                                         \
    __builtin_amdgcn_sched_barrier(0)
    // Queue high-water check.  Both wave halves run it in the SAME barrier interval -- the first one after all pushes of the finished item
    // (leading half: right behind the first barrier of the next item; trailing half: right behind its seam barrier) -- so the decision is
    // uniform, and the two barriers inside pair up half against half.
    auto maybe_flush = [&]() {
        unsigned n_ = 0;
#pragma unroll
        for (int w = 0; w < 8; ++w) n_ = max(n_, ((const volatile __attribute__((address_space(3))) unsigned *)qcnt)[w]);
        if (n_ >= S8_FLUSH_AT) {
            s8_flush(p, qbuf, qcnt, tid, xcc);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            S8_BARRIER();
            if (tid < 8) qcnt[tid] = 0;
            wq = 0;
            S8_BARRIER();
        }
    };
#define S8_MAYBE_FLUSH() maybe_flush()

    // ---- partner coupling.  The two workgroups that take the two query halves of the same row tiles (slots 2j, 2j + 1 of one XCD) should read
    // the index rows within the L2's residency of each other (~10 us of streaming); nothing else couples them (a miss does not slow the
    // leader down), and uncoupled they drift apart until every row tile is fetched from the fabric twice.  Once per two K-tiles wave 0 adds 1
    // to the pair's counter (no-return atomic) and has the counter DMA'd into an LDS word (no VGPR result, nothing to wait for); the word
    // read one round later gives the partner's progress as of ~4 us ago, and a workgroup that leads by two rounds or more naps in
    // proportion.  The follower never waits, so there is no way to deadlock; a finished workgroup adds 2^20.
    unsigned *const prog = (P.prog && P.halves == 2) ? P.prog + (xcd * (wg_per_xcd >> 1) + (slot >> 1)) * 64 : nullptr;      // 256 B apart: one L2 line each
    int ticks = 0;
#define S8_COUPLE()                                                                                                                       \
    if (prog && wave == 0) {                                                                                                              \
        const int tot_ = __builtin_amdgcn_readfirstlane((int)*(volatile __attribute__((address_space(3))) unsigned *)flagw);               \
        if (lane == 0) {                                                                                                                  \
            atomicAdd(prog, 1u);                                                                                                          \
            __builtin_amdgcn_global_load_lds((gptr_t *)prog, (lptr_t *)flagw, 4, 0, 16);      /* sc1 = agent scope: never from the CU's own L1 */   \
        }                                                                                                                                 \
        const int lead_ = 2 * ticks - tot_;                   /* my rounds minus the partner's, both as of the previous round */           \
        ++ticks;                                                                                                                          \
        if (!(P.s.tune & 64)) for (int i_ = 0; i_ < (lead_ > 6 ? 6 : lead_) - 1; ++i_) __builtin_amdgcn_s_sleep(16);     /* 1,024 cycles each */ \
    }

    intx4 acc[8][4];                                           // [16-row tile of the wave's 128 rows][16-query tile of its 64 queries]
    const intx4 zero4 = {0, 0, 0, 0};

    // ---- prologue: the first six half-tiles of the stream, then everybody meets once; the second half then drops one barrier behind
    S8_STAGE(0, 0); S8_STAGE(1, 0); S8_STAGE(2, 0); S8_STAGE(3, 0); S8_STAGE(0, 1); S8_STAGE(1, 1);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");          // A0, B0 of K-tile 0 have landed (this wave's pieces)
    S8_BARRIER();                                             // (also publishes the queue counter reset)
    if (wr == 1) { S8_BARRIER(); }

    for (int ti = 0; ti < my_count; ++ti) {
        // one pair of K-tiles (buffer 0, buffer 1); HOOK runs behind the first barrier, MF is the MFMA form of the first K-tile
#define S8_KPAIR(HOOK, MF)                                                                                                                \
        do {                                                                                                                              \
            S8_READ_B(0, 0, b0v); S8_READ_A(0, 0);                                                                                        \
            __builtin_amdgcn_sched_barrier(0);                                                                                            \
            S8_STAGE(2, 1);                                                                                                               \
            S8_SYNC_COMPUTE(HOOK, MF(0, 0, b0v));                                                                                         \
            S8_BARRIER();                                                                                                                 \
            S8_READ_B(0, 1, b1v);                                                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                                                            \
            S8_STAGE(3, 1);                                                                                                               \
            S8_SYNC_COMPUTE(, MF(0, 1, b1v));                                                                                             \
            S8_BARRIER();                                                                                                                 \
            S8_READ_A(0, 1);                                                                                                              \
            __builtin_amdgcn_sched_barrier(0);                                                                                            \
            S8_STAGE(0, 0);                                                                                                               \
            S8_SYNC_COMPUTE(, MF(1, 1, b1v));                                                                                             \
            S8_BARRIER();                                                                                                                 \
            S8_STAGE(1, 0);                                                                                                               \
            S8_SYNC_COMPUTE(, MF(1, 0, b0v));                                                                                             \
            S8_BARRIER();                                                                                                                 \
            S8_READ_B(1, 0, b0v); S8_READ_A(1, 0);                                                                                        \
            __builtin_amdgcn_sched_barrier(0);                                                                                            \
            S8_STAGE(2, 0);                                                                                                               \
            S8_SYNC_COMPUTE(, S8_MFMA(0, 0, b0v));                                                                                        \
            S8_BARRIER();                                                                                                                 \
            S8_READ_B(1, 1, b1v);                                                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                                                            \
            S8_STAGE(3, 0);                                                                                                               \
            S8_SYNC_COMPUTE(, S8_MFMA(0, 1, b1v));                                                                                        \
            S8_BARRIER();                                                                                                                 \
            S8_READ_A(1, 1);                                                                                                              \
            __builtin_amdgcn_sched_barrier(0);                                                                                            \
            S8_STAGE(0, 1);                                                                                                               \
            S8_SYNC_COMPUTE(, S8_MFMA(1, 1, b1v));                                                                                        \
            S8_BARRIER();                                                                                                                 \
            S8_STAGE(1, 1);                                                                                                               \
            S8_SYNC_COMPUTE(, S8_MFMA(1, 0, b0v));                                                                                        \
            S8_COUPLE();                                                                                                                  \
        } while (0)
        S8_KPAIR(if (wr == 0 && ti > 0) S8_MAYBE_FLUSH(), S8_MFMA_Z);
        if (2 < KT) { S8_BARRIER(); }
        for (int kt2 = 2; kt2 < KT; kt2 += 2) {
            S8_KPAIR(, S8_MFMA);
            if (kt2 + 2 < KT) { S8_BARRIER(); }
        }
        // ---- item seam.  The leading half is past its last MFMAs one barrier interval before the trailing half: it takes the closing barrier of
        // the last phase first, the trailing half after its filter, so both filters run in the same interval.
        if (wr == 0) { S8_BARRIER(); }

        const int pos = first + ti * wg_per_xcd;
        const int tile = P.t_begin + (P.halves == 2 ? pos >> 1 : pos);
        // lane ids rebuilt per item (v_mbcnt): hoisted to kernel entry they would be live across the whole main loop
        const int elane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const int e15 = elane & 15, eq = elane >> 4;
        const int row_w = tile * 256 + wr * 128 + eq;         // + 16 rt + 4 r
        const bool tail = (tile + 1) * 256 > p.n_rows;          // only the shard's last tile has rows that do not exist
        bool stored = false;
        // the block's three floats are wave-uniform: scalar loads from the constant address space, which do not queue behind the DMA stream
        const __attribute__((address_space(4))) float *bk = (const __attribute__((address_space(4))) float *)(uintptr_t)(P.blk + tile);
        const float bs = bk[0], bn_ = bk[1], bd = bk[2];
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            const unsigned q = (unsigned)(hq * 256 + wc * 64 + qt * 16 + (e15 & 3) * 4 + (e15 >> 2));
            const int tau = s8i_theta(tauv[qt], qcv[qt].x, qcv[qt].y, qcv[qt].z, bs, bn_, bd);
            // one max + one ballot per 128 x 16 accumulator column (31 v_max): the common case has no survivor.  A column with one looks into the
            // 16 x 16 tiles that hold one (their maxes are the partial results of the column's) and there into the four registers.
            int mr[8];
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) mr[rt] = max(max(acc[rt][qt][0], acc[rt][qt][1]), max(acc[rt][qt][2], acc[rt][qt][3]));
            const int m = max(max(max(mr[0], mr[1]), max(mr[2], mr[3])), max(max(mr[4], mr[5]), max(mr[6], mr[7])));
            if (__builtin_amdgcn_ballot_w64(m >= tau) == 0) continue;              // the common case
            // Slots come out of this wave's OWN queue region: the reservation is a scalar add (r03: a ballot, an LDS atomic by lane 0 and a
            // readfirstlane round trip per register that held a survivor); registers without a survivor cost a compare and a scalar branch.
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) {
                if (__builtin_amdgcn_ballot_w64(mr[rt] >= tau) == 0) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int v = acc[rt][qt][r];
                    const int row = row_w + rt * 16 + 4 * r;
                    const unsigned long long mask = __builtin_amdgcn_ballot_w64((v >= tau) && (!tail || row < p.n_rows));
                    if (mask == 0) continue;
                    if ((mask >> elane) & 1ull) {
                        const unsigned mine = wq + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
                        if (mine < S8_WCAP) {                                  // (two writes: no aligned register quad to assemble)
                            ((uint2 *)qbuf)[2 * (wave * S8_WCAP + mine)] = make_uint2((unsigned)v, (unsigned)row);
                            ((unsigned *)qbuf)[4 * (wave * S8_WCAP + mine) + 2] = q;
                        } else {                                               // queue region full: straight to the sub-list
                            s8_append(p, xcc, q, (unsigned)v, (unsigned)row);
                            stored = true;
                        }
                    }
                    wq += (unsigned)__popcll(mask);
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(stored)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (wq > S8_WCAP) wq = S8_WCAP;                        // (the overflow went straight to the candidate buffers)
        if (elane == 0) qcnt[wave] = wq;                       // published before the barrier behind which both halves look at the counts
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (wr == 1) {
            S8_BARRIER();
            if (ti + 1 < my_count) S8_MAYBE_FLUSH();
        }
    }
    if (wr == 0) { S8_BARRIER(); }                            // the leading half pays back the barrier the trailing half took at the start
    if (prog && tid == 0) atomicAdd(prog, 1u << 20);          // done: the partner stops pacing itself against this workgroup
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // speculative half-tiles past the end of the stream
    S8_BARRIER();
    s8_flush(p, qbuf, qcnt, tid, xcc);
}

} // namespace

// ------------------------------------------------------------------------------------------------
// shadow image: int8 rows in the stripe-tiled geometry + per 256-row block {s_b, N_b, D_b}, built from the finished fp16 image
// ------------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ float block_max_256(float v, float *sh)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();                                           // (sh may still be read from the previous reduction)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

__device__ __forceinline__ int quant8(float x, float inv)
{
    int v = (int)rintf(x * inv);
    return v > 127 ? 127 : (v < -127 ? -127 : v);              // (|x| <= 127 / inv up to rounding: the clamp never bites, and D_b is measured on the stored value anyway)
}

// One workgroup per 256-row block, one thread per row.  Pass 1: max |e| and max ||e_r||^2 of the block; pass 2 (the block is in L2 now):
// quantise with the block's scale, write the int8 rows, measure ||e_r - s_b e8_r||.  Rows past the end of the shard are zero in the fp16
// image and stay zero here.
__global__ void __launch_bounds__(256) seal_shadow_kernel(const char *__restrict__ tiled, int nch, char *__restrict__ e8, float4 *__restrict__ blk,
                                                          unsigned *__restrict__ nonfinite)
{
    __shared__ float sh[4];
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
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
    if (bad) atomicOr(nonfinite, 1u);
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
                    const float r = x - s * (float)qv;
                    d2 += r * r;
                    pk |= ((unsigned)qv & 255u) << (8 * b);
                }
                w[2 * hf + (j >> 2)] = pk;
            }
        }
        *(uint4 *)(e8 + tiled_seg_offset(row, g, nch8)) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    d2 = block_max_256(d2, sh);
    // the residual e - s e8 was evaluated in fp32: each element is off by up to 2^-24 |s e8| + 2^-24 |e - s e8|, which matters exactly when the
    // quantisation is (nearly) exact -- ternary rows have d2 = 0 while 127 * fl(1 / 127) is not 1.  2^-22 N_b covers it.
    const float nb = sqrtf(n2) * 1.001f;
    if (threadIdx.x == 0) blk[blockIdx.x] = make_float4(s, nb, (sqrtf(d2) + nb * 0x1p-22f) * 1.001f, 0.f);
}

// int8 query image (chunk-tiled like the fp16 one, 64 k-values per chunk) + per query {t_q, a_q, b_q}; one wave per padded query row
__global__ void pack_queries_i8_kernel(const uint4 *__restrict__ queries, int n_q, int nseg, int bn, char *__restrict__ q8, float4 *__restrict__ qc)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    float amax = 0.f;
    if (q < n_q)
        for (int seg = lane; seg < nseg; seg += 64) {
            const half8 h = __builtin_bit_cast(half8, queries[(size_t)q * nseg + seg]);
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf((float)h[j]));
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    const float t = amax / 127.f;
    const float inv = t > 0.f ? 127.f / amax : 0.f;
    float a2 = 0.f, b2 = 0.f;
    for (int g = lane; g < nseg / 2; g += 64) {
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (q < n_q) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const half8 h = __builtin_bit_cast(half8, queries[(size_t)q * nseg + 2 * g + hf]);
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
    if (lane == 0) qc[q] = q < n_q ? make_float4(t, (ra + (ra + rb) * 0x1p-22f) * 1.001f, rb * 1.001f, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Re-score what one int8 segment appended: the score word of every new entry becomes the fp32 sum of the exact fp16 products of its row and
// query (any fp32 accumulation order satisfies the eps of DESIGN 3.3, so select, finalize and the proof run unchanged).  New entries of query
// q: the eight sub-lists up to min(count8, SUBCAP) and the main list from `pre` to min(count, capq); the entries below `pre` were kept by the
// select before the segment and keep their scores bit for bit.  `pre` is kp: an int8 segment always follows a select over at least the
// dense segment's rows, which leaves exactly kp entries.  grid (9 lists, n_q), one wave per entry.
__global__ void __launch_bounds__(256) rescore_kernel(const char *__restrict__ tiled, const uint4 *__restrict__ queries, int nseg, uint2 *cand,
                                                      const unsigned *__restrict__ count, uint2 *cand8, const unsigned *__restrict__ count8,
                                                      unsigned capq, unsigned pre)
{
    const int q = blockIdx.y, list = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint2 *ent;
    unsigned lo, hi;
    if (list < 8) {
        ent = cand8 + ((size_t)q * 8 + list) * SUBCAP; lo = 0; hi = count8[list * 512 + q];
        if (hi > SUBCAP) hi = SUBCAP;
    } else {
        ent = cand + (size_t)q * capq; lo = pre; hi = count[q];
        if (hi > capq) hi = capq;
    }
    const uint4 *qrow = queries + (size_t)q * nseg;
    const int nch = nseg >> 2;
    for (unsigned i0 = lo + 2 * wave; i0 < hi; i0 += 8) {      // two entries in flight per wave
        const bool two = i0 + 1 < hi;
        const unsigned r0 = ent[i0].y, r1 = ent[two ? i0 + 1 : i0].y;
        float s0 = 0.f, s1 = 0.f;
        for (int seg = lane; seg < nseg; seg += 64) {
            const half8 e0 = __builtin_bit_cast(half8, *(const uint4 *)(tiled + tiled_seg_offset(r0, seg, nch)));
            const half8 e1 = __builtin_bit_cast(half8, *(const uint4 *)(tiled + tiled_seg_offset(r1, seg, nch)));
            const half8 qv = __builtin_bit_cast(half8, qrow[seg]);
#pragma unroll
            for (int j = 0; j < 8; ++j) { s0 += (float)e0[j] * (float)qv[j]; s1 += (float)e1[j] * (float)qv[j]; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
        if (lane == 0) {
            ent[i0].x = __float_as_uint(s0);
            if (two) ent[i0 + 1].x = __float_as_uint(s1);
        }
    }
}

} // namespace

int mips_launch_seal_shadow(const void *tiled, int64_t n_rows, int dim, void *e8, float *blk, unsigned *nonfinite, hipStream_t stream)
{
    const int64_t blocks = (n_rows + 255) / 256;
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(seal_shadow_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const char *)tiled, dim / 32, (char *)e8, (float4 *)blk, nonfinite);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int mips_launch_pack_queries_i8(const void *queries, int n_q, int dim, int bn, void *q8_tiled, float *qc, hipStream_t stream)
{
    hipLaunchKernelGGL(pack_queries_i8_kernel, dim3(bn), dim3(64), 0, stream, (const uint4 *)queries, n_q, dim / 8, bn, (char *)q8_tiled, (float4 *)qc);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int mips_launch_rescore(const ScanParams &p, const void *queries, unsigned pre, hipStream_t stream)
{
    hipLaunchKernelGGL(rescore_kernel, dim3(9, p.n_q), dim3(256), 0, stream, p.e_tiled, (const uint4 *)queries, p.nch * 4, p.cand, p.count, p.cand8,
                       p.count8, p.capq, pre);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// Filter scan (mode 0) of rows [row_begin, row_end) on the shadow image, for a query image of `bn` = 256 or 512 rows; `p` is the fp16 scan's
// parameter block (p.nch = dim / 32).  -4 = not covered (the caller uses the fp16 kernels)
int mips_launch_scan8i(const ScanParams &p, const void *e8_tiled, const float *blk, const void *q8_tiled, const float *qc, int bn, int64_t row_begin,
                       int64_t row_end, int cus, unsigned *prog, hipStream_t stream)
{
    if ((bn != 256 && bn != 512) || (p.nch & 7) || p.nch < 8 || (row_begin & 255) || row_end <= row_begin || !p.cand8 || !p.count8) return -4;
    Scan8Params P;
    P.s = p;
    P.s.e_tiled = (const char *)e8_tiled;
    P.s.q_tiled = (const char *)q8_tiled;
    P.s.nch = p.nch / 2;                                      // 64-wide int8 chunks; a multiple of 4 (K-tiles come in pairs)
    P.blk = (const float4 *)blk;
    P.qc = (const float4 *)qc;
    P.prog = prog;
    P.bn = bn; P.halves = bn / 256;
    P.t_begin = (int)(row_begin >> 8);
    P.t_end = (int)((row_end + 255) >> 8);
    P.last_stripe = (int)((p.n_rows + STRIPE_ROWS - 1) / STRIPE_ROWS) - 1;
    P.total = (P.t_end - P.t_begin) * P.halves;
    int grid = cus & ~15;                                     // a multiple of 8 XCDs x an even number of workgroups each
    if (grid < 16) grid = 16;
    if (P.total < grid) return -4;                            // short segments stay on the non-persistent kernel
    P.per = ((P.total + 7) >> 3);
    P.per = (P.per + 1) & ~1;                                 // both halves of a tile on the same XCD
    constexpr int LDS = 2 * S8_BUF + S8_QCAP * 16 + 128;
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void *)mips_scan8i_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS) != hipSuccess) return -3;
        attr_done = true;
    }
    hipLaunchKernelGGL(mips_scan8i_kernel, dim3(grid), dim3(512), LDS, stream, P);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
