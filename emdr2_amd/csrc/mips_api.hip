// emdr2_amd/csrc/mips_api.hip -- C ABI (include/emdr2_mips.h) over the MIPS kernels.
#include "../../include/emdr2_mips.h"
#include "mips_kernels.h"
#include "exp_hooks.h"
#include <stdlib.h>

namespace {

#define TIMING_SLOTS 2048
struct Timing {
    bool enabled = false;
    hipEvent_t ev[2 * TIMING_SLOTS] = {};
    int created = 0;
    int n = 0;
    int64_t rows[TIMING_SLOTS] = {};
} g_timing;

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Tuning / ablation switches are read from the environment ONLY in -DEMDR2_EXPERIMENTS builds (`make exp`, used by tools/); the production
// library always runs the defaults, so a stray variable cannot change (or, with the ablations, corrupt) results.
// `product`: the defaults in either build (emdr2_mips_search_plan).  false: a knob out of range.
bool search_knobs(SearchKnobs *kn, bool product = false)
{
#define KNOB(name, dflt) (product ? (dflt) : EXP_ENV_INT(name, dflt))
    kn->seg0 = KNOB("EMDR2_MIPS_SEG0", 8192) / 512 * 512;
    kn->growth = KNOB("EMDR2_MIPS_GROWTH", 8);               // r04: 8 (was 16): with cheaper selects a tighter threshold for the next segment pays (tools/mips_timeline.py)
    kn->growth_i8 = KNOB("EMDR2_MIPS_GROWTH_I8", 2);
    kn->margin_i8 = (float)KNOB("EMDR2_MIPS_MARGIN_PCT", 25) * 0.01f;
    kn->force_variant = KNOB("EMDR2_MIPS_VARIANT", -1);
    kn->cus = KNOB("EMDR2_MIPS_GRID", device_cu_count());
    kn->scan_kernel = KNOB("EMDR2_MIPS_KERNEL", 1);          // 1 = lockstep v1, 2 = ping-pong
    kn->ablate = KNOB("EMDR2_MIPS_ABLATE", 0);
    kn->tune = KNOB("EMDR2_MIPS_TUNE", 17);
    kn->couple = product || EXP_MIPS_COUPLE();
#undef KNOB
    return kn->seg0 >= 512 && kn->seg0 <= (int)CAPQ - 512 && kn->growth >= 2 && kn->growth_i8 >= 2;
}

// the timing bracket of one scan segment (emdr2_mips_set_timing): one event pair and the segment's row count
int timing_begin(hipStream_t stream, bool *timed)
{
    *timed = g_timing.enabled && g_timing.n < TIMING_SLOTS;
    if (!*timed) return 0;
    while (g_timing.created <= g_timing.n) {
        if (hipEventCreate(&g_timing.ev[2 * g_timing.created]) != hipSuccess || hipEventCreate(&g_timing.ev[2 * g_timing.created + 1]) != hipSuccess)
            return EMDR2_E_LAUNCH;
        ++g_timing.created;
    }
    return hipEventRecord(g_timing.ev[2 * g_timing.n], stream) == hipSuccess ? 0 : EMDR2_E_LAUNCH;
}

int timing_end(hipStream_t stream, int64_t rows)
{
    if (hipEventRecord(g_timing.ev[2 * g_timing.n + 1], stream) != hipSuccess) return EMDR2_E_LAUNCH;
    g_timing.rows[g_timing.n++] = rows;
    return 0;
}

struct Workspace {
    char *q_frag;
    char *q_tiled;
    float *qnorm, *tau;
    unsigned *count;       // [512] main-list counts, then [8][512] sub-list counts, [512] pending counts, then the pair-progress counters
    uint2 *cand, *cand8, *pend;
    unsigned *count8() const { return count + 512; }
    unsigned *pcount() const { return count + 9 * 512; }
    unsigned *prog0() const { return count + 10 * 512; }
    // the int8 query image and the per-query constants live where the fragment-tiled query image of the experiment kernels would (half its
    // size + 8 KiB)
    char *q8_tiled() const { return q_frag; }
    float *qc(int dim) const { return (float *)(q_frag + (size_t)(dim / 64) * 512 * 64); }
};

size_t carve(char *base, int dim, Workspace *w)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += align_up(bytes, 256); return p; };
    char *f = take((size_t)(dim / 32) * 512 * 64);
    char *a = take((size_t)(dim / 32) * 512 * 64);
    char *b = take(512 * sizeof(float));
    char *c = take(512 * sizeof(float));
    char *d = take((512 + 8 * 512 + 512 + 8 * (size_t)SCAN8_PROG_UINTS) * sizeof(unsigned)); // candidate counts (main, per-XCD, pending) + pair progress counters of up to 8 scan8 launches
    char *e = take((size_t)512 * CAPQ * sizeof(uint2));
    char *g = take((size_t)512 * 8 * SUBCAP * sizeof(uint2));
    char *h = take((size_t)512 * PENDCAP * sizeof(uint2));     // deferred survivors of the int8 segments (mips_scan8i.hip)
    if (w) { w->q_frag = f; w->q_tiled = a; w->qnorm = (float *)b; w->tau = (float *)c; w->count = (unsigned *)d; w->cand = (uint2 *)e; w->cand8 = (uint2 *)g; w->pend = (uint2 *)h; }
    return off;
}

// int8 shadow image of a shard (mips_scan8i.hip): filter segments of at least `min_rows` rows that the persistent fp16 scan would take run on it
struct Shadow {
    const void *image;
    const float *table;
    int64_t min_rows;
};
long g_shadow_launches = 0;

bool bad_shape(int64_t n_rows, int dim) { return n_rows < 0 || n_rows >= ((int64_t)1 << 31) - 1024 || dim < 64 || dim > 8192 || (dim % 32) != 0; }

} // namespace

extern "C" {

int emdr2_abi_version(void) { return EMDR2_ABI_VERSION; }

int emdr2_device_cu_count(void) { return device_cu_count(); }

int emdr2_mips_set_timing(int enabled)
{
    g_timing.enabled = enabled != 0;
    g_timing.n = 0;
    return EMDR2_OK;
}

int emdr2_mips_timing_collect(float *ms, int64_t *rows, int max_n, int *n_out)
{
    const int n = g_timing.n < max_n ? g_timing.n : max_n;
    for (int i = 0; i < n; ++i) {
        if (hipEventSynchronize(g_timing.ev[2 * i + 1]) != hipSuccess) return EMDR2_E_LAUNCH;
        if (hipEventElapsedTime(&ms[i], g_timing.ev[2 * i], g_timing.ev[2 * i + 1]) != hipSuccess) return EMDR2_E_LAUNCH;
        rows[i] = g_timing.rows[i];
    }
    if (n_out) *n_out = n;
    g_timing.n = 0;
    return EMDR2_OK;
}

int emdr2_mips_layout_bytes(int64_t n_rows, int dim, size_t *bytes)
{
    if (!bytes || bad_shape(n_rows, dim)) return EMDR2_E_BADARG;
    const int64_t padded = (n_rows + 511) / 512 * 512;
    *bytes = (size_t)padded * dim * 2;
    return EMDR2_OK;
}

int emdr2_mips_pack_rows(const void *rows_rm, int64_t n_chunk, int dim, int64_t row_offset, int64_t n_rows_total,
                         void *tiled, float *emax_sq, emdr2_stream_t stream)
{
    if (!rows_rm || !tiled || !emax_sq || bad_shape(n_rows_total, dim) || n_chunk < 0 || row_offset < 0 ||
        row_offset + n_chunk > n_rows_total)
        return EMDR2_E_BADARG;
    return mips_launch_pack_rows(rows_rm, n_chunk, dim, row_offset, tiled, emax_sq, (hipStream_t)stream);
}

int emdr2_mips_unpack_rows(const void *tiled, int64_t n_rows_total, int dim, const int64_t *row_ids, int64_t n_out,
                           void *rows_rm, emdr2_stream_t stream)
{
    if (!tiled || !row_ids || !rows_rm || bad_shape(n_rows_total, dim) || n_out < 0) return EMDR2_E_BADARG;
    return mips_launch_unpack_rows(tiled, n_rows_total, dim, 0, row_ids, n_out, rows_rm, (hipStream_t)stream);
}

int emdr2_mips_gather_rows(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const int64_t *global_rows, int64_t n_out,
                           void *rows_rm, emdr2_stream_t stream)
{
    if (!tiled || !global_rows || !rows_rm || bad_shape(n_rows, dim) || row_base < 0 || n_out < 0) return EMDR2_E_BADARG;
    return mips_launch_unpack_rows(tiled, n_rows, dim, row_base, global_rows, n_out, rows_rm, (hipStream_t)stream);
}

int emdr2_mips_export_rows(const void *tiled, int64_t n_rows_total, int dim, int64_t row_offset, int64_t n_chunk, void *rows_rm,
                           emdr2_stream_t stream)
{
    if (!tiled || !rows_rm || bad_shape(n_rows_total, dim) || n_chunk < 0 || row_offset < 0 || row_offset + n_chunk > n_rows_total)
        return EMDR2_E_BADARG;
    return mips_launch_export_rows(tiled, dim, row_offset, n_chunk, rows_rm, (hipStream_t)stream);
}

int emdr2_mips_digest_rows(const void *tiled, int64_t n_rows_total, int dim, int64_t row_offset, int64_t n_chunk, int64_t row_base,
                           uint64_t *digest, emdr2_stream_t stream)
{
    if (!tiled || !digest || ((uintptr_t)digest & 7) || bad_shape(n_rows_total, dim) || n_chunk < 0 || row_offset < 0 ||
        row_offset + n_chunk > n_rows_total)
        return EMDR2_E_BADARG;
    return mips_launch_digest_rows(tiled, dim, row_offset, n_chunk, row_base, digest, (hipStream_t)stream);
}

int emdr2_mips_digest_stamps(const uint32_t *generation, int64_t n_rows_total, int64_t row_offset, int64_t n_chunk, int64_t row_base,
                             uint64_t *digest, emdr2_stream_t stream)
{
    if (!digest || ((uintptr_t)digest & 7) || ((uintptr_t)generation & 3) || n_rows_total < 0 || n_chunk < 0 || row_offset < 0 ||
        row_offset + n_chunk > n_rows_total || row_base < 0 || (n_chunk > 0 && !generation))
        return EMDR2_E_BADARG;
    return mips_launch_digest_stamps(generation, row_offset, n_chunk, row_base, digest, (hipStream_t)stream);
}

int emdr2_mips_workspace_bytes(int n_q, int dim, int k, size_t *bytes)
{
    if (!bytes || n_q < 1 || k < 1 || k > EMDR2_MAX_TOPK || bad_shape(0, dim)) return EMDR2_E_BADARG;
    *bytes = carve(nullptr, dim, nullptr);
    return EMDR2_OK;
}

// The start of a pass: query images and norms; thresholds, counts, flags -- and the sub-list counts, pending counts and pair-progress counters
// of the persistent scan launches -- in one launch
static int prepare_pass(const SearchPlan &plan, const SearchKnobs &kn, const Workspace &w, const uint16_t *qp, int nqp, int dim, uint32_t *flags,
                        hipStream_t stream)
{
    PrepareParams pp;
    pp.queries = qp;
    pp.n_q = nqp;
    pp.dim = dim;
    pp.bn = plan.bn;
    pp.q_tiled = w.q_tiled;
    pp.qnorm = w.qnorm;
    pp.tau = w.tau;
    pp.count = w.count;
    pp.flags = flags;
    pp.dense_count = (unsigned)plan.seg[0].row_end;
    pp.zero = w.count8();
    pp.n_zero = 9 * 512 + (plan.variant == 0 ? 8 * (size_t)SCAN8_PROG_UINTS : 0);
    pp.q8_tiled = plan.pack_q8 ? w.q8_tiled() : nullptr;
    pp.qc = w.qc(dim);
    int rc;
    if ((rc = mips_launch_prepare(pp, stream))) return rc;
    EXP_MIPS_PACK_QUERIES_FRAG(plan.variant, kn.scan_kernel, qp, nqp, dim, w, stream, rc)
    return 0;
}

// The segments of a pass as planned: each on its engine, a triage launch behind an int8 segment, a select launch where the plan says so.
// A launcher that answers -4 for the engine the plan chose contradicts the plan, which asked the launcher's own predicate: an error like any other.
static int scan_segments(const SearchPlan &plan, const SearchKnobs &kn, const Workspace &w, const void *tiled, int64_t n_rows, int dim, const uint16_t *qp,
                         int nqp, uint32_t *flags, const Shadow *shadow, hipStream_t stream)
{
    ScanParams sp;
    sp.e_tiled = (const char *)tiled;
    sp.q_tiled = w.q_tiled;
    sp.tau = w.tau;
    sp.cand = w.cand;
    sp.count = w.count;
    sp.flags = flags;
    sp.dense_out = nullptr;
    sp.nch = dim / 32;
    sp.n_rows = (int)n_rows;
    sp.n_q = nqp;
    sp.capq = CAPQ;
    sp.cand8 = w.cand8;
    sp.count8 = w.count8();
    sp.dense_row0 = 0;
    sp.tune = kn.tune;
    sp.trace = (unsigned long long *)w.cand + (size_t)511 * CAPQ; // scratch tail of the candidate area (ABL 9 only)
    for (int i = 0; i < plan.n_segments; ++i) {
        const SearchSegment &s = plan.seg[i];
        sp.tile_begin = (int)(s.row_begin / plan.bm);
        sp.tile_end = (int)((s.row_end + plan.bm - 1) / plan.bm);
        const int tiles = sp.tile_end - sp.tile_begin;
        const int grid = tiles < kn.cus ? tiles : kn.cus;
        unsigned *const prog = s.prog_slot >= 0 ? w.prog0() + (size_t)SCAN8_PROG_UINTS * s.prog_slot : nullptr;
        bool timed;
        int rc;
        if ((rc = timing_begin(stream, &timed))) return rc;
        switch (s.engine) {
        case DENSE:
            rc = mips_launch_scan(plan.variant, 1, sp, grid, stream);
            break;
        case LOCKSTEP:
            EXP_MIPS_SCAN_VARIANT(plan.variant, kn.ablate, kn.scan_kernel, sp, w, grid, s.row_end, n_rows, s.row_begin, stream, rc)
            rc = mips_launch_scan(plan.variant, 0, sp, grid, stream);
            break;
        case PERSISTENT_F16:
            rc = mips_launch_scan8(sp, plan.bn, s.row_begin, s.row_end, kn.cus, prog, stream);
            break;
        case PERSISTENT_I8:
            rc = mips_launch_scan8i(sp, shadow->image, shadow->table, w.q8_tiled(), w.qc(dim), plan.bn, s.row_begin, s.row_end, kn.cus, prog, stream);
            if (rc == 0) ++g_shadow_launches;
            break;
        }
        if (rc) return rc;
        if (timed && (rc = timing_end(stream, s.row_end - s.row_begin))) return rc;
        // survivors of an int8 segment carry integer sums: the likely winners get their fp32 scores before the select reads them, the others
        // wait in the pending list behind an upper bound
        if (s.engine == PERSISTENT_I8 &&
            (rc = mips_launch_triage(sp, qp, (unsigned)plan.kp, shadow->table, w.qc(dim), w.pend, w.pcount(), kn.margin_i8, stream)))
            return rc;
        if (s.select_after && (rc = mips_launch_select(w.cand, w.count, w.cand8, w.count8(), w.tau, flags, CAPQ, plan.kp, nqp, stream))) return rc;
    }
    return 0;
}

// One search = per pass of up to 512 queries: plan (mips_plan.h), prepare, the plan's segments, finalize.
static int search_impl(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const float *emax_sq,
                       const void *queries, int n_q, int k, const int32_t *ids, void *out_dist, int32_t *out_idx,
                       int64_t *out_row, uint32_t *out_flags, void *workspace, size_t workspace_bytes,
                       emdr2_stream_t stream_, int f32, uint4 *out_rec = nullptr, const Shadow *shadow = nullptr)
{
    if (!tiled || !emax_sq || !queries || !out_flags || !workspace) return EMDR2_E_BADARG;
    if (!out_rec && (!out_dist || !out_idx || !out_row)) return EMDR2_E_BADARG;
    if (out_rec && ((uintptr_t)out_rec & 15)) return EMDR2_E_BADARG;
    if (n_q < 1 || k < 1 || k > EMDR2_MAX_TOPK || bad_shape(n_rows, dim) || n_rows < 1) return EMDR2_E_BADARG;
    Workspace w;
    if (carve((char *)workspace, dim, &w) > workspace_bytes) return EMDR2_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    SearchKnobs kn;
    if (!search_knobs(&kn)) return EMDR2_E_BADARG;

    for (int q0 = 0; q0 < n_q; q0 += EMDR2_MAX_QUERIES_PER_PASS) {
        const int nqp = (n_q - q0) < EMDR2_MAX_QUERIES_PER_PASS ? (n_q - q0) : EMDR2_MAX_QUERIES_PER_PASS;
        const uint16_t *qp = (const uint16_t *)queries + (size_t)q0 * dim;
        int rc;
        SearchPlan plan;
        if (mips_plan_search(n_rows, nqp, dim, k, shadow ? shadow->min_rows : -1, kn, &plan)) return EMDR2_E_UNSUPPORTED;
        if ((rc = prepare_pass(plan, kn, w, qp, nqp, dim, out_flags + q0, stream))) return rc;
        if ((rc = scan_segments(plan, kn, w, tiled, n_rows, dim, qp, nqp, out_flags + q0, shadow, stream))) return rc;

        FinalizeParams fp;
        fp.e_tiled = (const char *)tiled;
        fp.queries = qp;
        fp.cand = w.cand;
        fp.count = w.count;
        fp.cand8 = w.cand8;
        fp.count8 = w.count8();
        fp.tau = w.tau;
        fp.qnorm = w.qnorm;
        fp.emax_sq = emax_sq;
        fp.ids = ids;
        fp.out_rec = out_rec ? out_rec + (size_t)q0 * k : nullptr;
        fp.out_dist = out_rec ? nullptr : (f32 ? (void *)((float *)out_dist + (size_t)q0 * k) : (void *)((uint16_t *)out_dist + (size_t)q0 * k));
        fp.f32 = f32;
        fp.out_idx = out_rec ? nullptr : out_idx + (size_t)q0 * k;
        fp.out_row = out_rec ? nullptr : out_row + (size_t)q0 * k;
        fp.flags = out_flags + q0;
        fp.n_rows = n_rows;
        fp.row_base = row_base;
        fp.dim = dim;
        fp.n_q = nqp;
        fp.k = k;
        fp.kp = plan.kp;
        fp.capq = CAPQ;
        fp.pend = plan.any_pending ? w.pend : nullptr;
        fp.pcount = w.pcount();
        if ((rc = mips_launch_finalize(fp, true, stream))) return rc;
    }
    return EMDR2_OK;
}

static_assert(DENSE == EMDR2_SCAN_DENSE && LOCKSTEP == EMDR2_SCAN_LOCKSTEP && PERSISTENT_F16 == EMDR2_SCAN_PERSISTENT_F16 &&
              PERSISTENT_I8 == EMDR2_SCAN_PERSISTENT_I8, "the engine codes of include/emdr2_mips.h");
int emdr2_mips_search_plan(int64_t n_rows, int n_q, int dim, int k, int64_t shadow_min_rows, int cus, int max_segments, int *n_segments,
                           int64_t *row_end, int32_t *engine, int32_t *select_after, int32_t *prog_slot, int *pack_q8)
{
    if (!n_segments || !row_end || !engine || !select_after || !prog_slot || !pack_q8) return EMDR2_E_BADARG;
    if (n_q < 1 || n_q > EMDR2_MAX_QUERIES_PER_PASS || k < 1 || k > EMDR2_MAX_TOPK || bad_shape(n_rows, dim) || cus < 0) return EMDR2_E_BADARG;
    SearchKnobs kn;
    SearchPlan plan;
    search_knobs(&kn, true);
    if (cus) kn.cus = cus;
    if (mips_plan_search(n_rows, n_q, dim, k, shadow_min_rows, kn, &plan) || plan.n_segments > max_segments) return EMDR2_E_BADARG;
    for (int i = 0; i < plan.n_segments; ++i) {
        row_end[i] = plan.seg[i].row_end;
        engine[i] = plan.seg[i].engine;
        select_after[i] = plan.seg[i].select_after;
        prog_slot[i] = plan.seg[i].prog_slot;
    }
    *n_segments = plan.n_segments;
    *pack_q8 = plan.pack_q8;
    return EMDR2_OK;
}

int emdr2_mips_search(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const float *emax_sq,
                      const void *queries, int n_q, int k, const int32_t *ids, void *out_dist, int32_t *out_idx,
                      int64_t *out_row, uint32_t *out_flags, void *workspace, size_t workspace_bytes,
                      emdr2_stream_t stream)
{
    return search_impl(tiled, n_rows, dim, row_base, emax_sq, queries, n_q, k, ids, out_dist, out_idx, out_row, out_flags, workspace,
                       workspace_bytes, stream, 0);
}

int emdr2_mips_search_f32(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const float *emax_sq,
                          const void *queries, int n_q, int k, const int32_t *ids, float *out_dist, int32_t *out_idx,
                          int64_t *out_row, uint32_t *out_flags, void *workspace, size_t workspace_bytes,
                          emdr2_stream_t stream)
{
    return search_impl(tiled, n_rows, dim, row_base, emax_sq, queries, n_q, k, ids, out_dist, out_idx, out_row, out_flags, workspace,
                       workspace_bytes, stream, 1);
}

int emdr2_mips_search_records(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const float *emax_sq, const void *queries, int n_q,
                              int k, const int32_t *ids, int f32, void *out_records, uint32_t *out_flags, void *workspace,
                              size_t workspace_bytes, emdr2_stream_t stream)
{
    if (!out_records) return EMDR2_E_BADARG;
    return search_impl(tiled, n_rows, dim, row_base, emax_sq, queries, n_q, k, ids, nullptr, nullptr, nullptr, out_flags, workspace,
                       workspace_bytes, stream, f32 ? 1 : 0, (uint4 *)out_records);
}

int emdr2_mips_shadow_bytes(int64_t n_rows, int dim, size_t *image_bytes, size_t *table_bytes)
{
    if (!image_bytes || !table_bytes || bad_shape(n_rows, dim) || (dim % 256) != 0) return EMDR2_E_BADARG;
    const int64_t padded = (n_rows + 511) / 512 * 512;
    *image_bytes = (size_t)padded * dim;
    *table_bytes = (size_t)(padded / 256) * 4 * sizeof(float);
    return EMDR2_OK;
}

int emdr2_mips_seal_shadow(const void *tiled, int64_t n_rows, int dim, void *shadow, void *table, uint32_t *nonfinite, emdr2_stream_t stream)
{
    if (!tiled || !shadow || !table || !nonfinite || ((uintptr_t)table & 15) || bad_shape(n_rows, dim) || (dim % 256) != 0) return EMDR2_E_BADARG;
    return mips_launch_seal_shadow(tiled, dim, 0, (n_rows + 255) / 256, shadow, (float *)table, nonfinite, (hipStream_t)stream);
}

int emdr2_mips_block_norm_bytes(int64_t n_rows, size_t *bytes)
{
    if (!bytes || bad_shape(n_rows, 64)) return EMDR2_E_BADARG;
    *bytes = (size_t)((n_rows + 511) / 512 * 512 / 256) * sizeof(float);
    return EMDR2_OK;
}

int emdr2_mips_block_norms(const void *tiled, int64_t n_rows, int dim, int64_t first_block, int64_t n_blocks, float *block_norm_sq,
                           emdr2_stream_t stream)
{
    const int64_t table_blocks = (n_rows + 511) / 512 * 2;
    if (!tiled || !block_norm_sq || bad_shape(n_rows, dim) || first_block < 0 || n_blocks < 0 || first_block + n_blocks > table_blocks)
        return EMDR2_E_BADARG;
    return mips_launch_block_norms(tiled, dim, first_block, n_blocks, block_norm_sq, (hipStream_t)stream);
}

// both forms of the contiguous update: `stamp` null = emdr2_mips_update_rows as it always was
static int update_rows_impl(const void *rows_rm, int64_t n_chunk, int dim, int64_t row_offset, int64_t n_rows_total, void *tiled, float *block_norm_sq,
                            float *emax_sq, void *shadow, void *table, uint32_t *nonfinite, const RowStamp *stamp, emdr2_stream_t stream_)
{
    if (!rows_rm || !tiled || !block_norm_sq || !emax_sq || bad_shape(n_rows_total, dim) || n_chunk < 0 || row_offset < 0 ||
        row_offset + n_chunk > n_rows_total)
        return EMDR2_E_BADARG;
    if (shadow && (!table || !nonfinite || ((uintptr_t)table & 15) || (dim % 256) != 0)) return EMDR2_E_BADARG;
    if (n_chunk == 0) return EMDR2_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t first_block = row_offset / 256, n_blocks = (row_offset + n_chunk - 1) / 256 - first_block + 1;   // the blocks these rows touch
    int rc;
    if ((rc = mips_launch_write_rows(rows_rm, n_chunk, dim, row_offset, tiled, stamp, stream))) return rc;
    if ((rc = mips_launch_block_norms(tiled, dim, first_block, n_blocks, block_norm_sq, stream))) return rc;
    if ((rc = mips_launch_table_max(block_norm_sq, (n_rows_total + 511) / 512 * 2, emax_sq, stream))) return rc;
    if (shadow) return mips_launch_seal_shadow(tiled, dim, first_block, n_blocks, shadow, (float *)table, nonfinite, stream);
    return EMDR2_OK;
}

int emdr2_mips_update_rows(const void *rows_rm, int64_t n_chunk, int dim, int64_t row_offset, int64_t n_rows_total, void *tiled,
                           float *block_norm_sq, float *emax_sq, void *shadow, void *table, uint32_t *nonfinite, emdr2_stream_t stream)
{
    return update_rows_impl(rows_rm, n_chunk, dim, row_offset, n_rows_total, tiled, block_norm_sq, emax_sq, shadow, table, nonfinite, nullptr, stream);
}

// (stamps are below 2^31; the stamp array and the counter are 4-byte words of device memory)
static bool bad_stamp(const uint32_t *generation, uint32_t gen, const uint32_t *n_kept_newer)
{
    return !generation || ((uintptr_t)generation & 3) || ((uintptr_t)n_kept_newer & 3) || gen >= 0x80000000u;
}

int emdr2_mips_update_rows_stamped(const void *rows_rm, int64_t n_chunk, int dim, int64_t row_offset, int64_t n_rows_total, void *tiled,
                                   float *block_norm_sq, float *emax_sq, void *shadow, void *table, uint32_t *nonfinite, uint32_t *generation,
                                   uint32_t gen, int newest_wins, uint32_t *n_kept_newer, emdr2_stream_t stream)
{
    if (bad_stamp(generation, gen, n_kept_newer)) return EMDR2_E_BADARG;
    const RowStamp stamp = {generation, gen, newest_wins ? 1 : 0, n_kept_newer};
    return update_rows_impl(rows_rm, n_chunk, dim, row_offset, n_rows_total, tiled, block_norm_sq, emax_sq, shadow, table, nonfinite, &stamp, stream);
}

// workspace of a scattered update: one claim word per 256-row block of the padded image, the touched-block counter (a 16-byte slot), then
// the touched-block list, min(n_upd, table blocks) entries
static size_t scatter_claim_bytes(int64_t table_blocks) { return ((size_t)table_blocks * sizeof(unsigned) + 15) / 16 * 16; }
static bool bad_scatter_shape(int64_t n_rows_total, int64_t n_upd) { return bad_shape(n_rows_total, 64) || n_upd < 0 || n_upd >= ((int64_t)1 << 31) - 1024; }

int emdr2_mips_scatter_workspace_bytes(int64_t n_rows_total, int64_t n_upd, size_t *bytes)
{
    if (!bytes || bad_scatter_shape(n_rows_total, n_upd)) return EMDR2_E_BADARG;
    const int64_t table_blocks = (n_rows_total + 511) / 512 * 2;
    *bytes = scatter_claim_bytes(table_blocks) + 16 + (size_t)(n_upd < table_blocks ? n_upd : table_blocks) * sizeof(unsigned);
    return EMDR2_OK;
}

// both forms of the scattered update: `stamp` null = emdr2_mips_update_rows_scattered as it always was
static int update_rows_scattered_impl(const void *rows_rm, const int64_t *row_ids, int64_t n_upd, int dim, int64_t n_rows_total, void *tiled,
                                      float *block_norm_sq, float *emax_sq, void *shadow, void *table, uint32_t *nonfinite, void *workspace,
                                      size_t workspace_bytes, const RowStamp *stamp, emdr2_stream_t stream_)
{
    if (!rows_rm || !row_ids || !tiled || !block_norm_sq || !emax_sq || !workspace || ((uintptr_t)workspace & 15) || bad_shape(n_rows_total, dim) ||
        bad_scatter_shape(n_rows_total, n_upd))
        return EMDR2_E_BADARG;
    if (shadow && (!table || !nonfinite || ((uintptr_t)table & 15) || (dim % 256) != 0)) return EMDR2_E_BADARG;
    if (n_upd == 0) return EMDR2_OK;
    size_t need;
    emdr2_mips_scatter_workspace_bytes(n_rows_total, n_upd, &need);
    if (workspace_bytes < need) return EMDR2_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t table_blocks = (n_rows_total + 511) / 512 * 2;
    const unsigned cap = (unsigned)(n_upd < table_blocks ? n_upd : table_blocks);      // no more distinct blocks than rows, or than there are
    const size_t claim_bytes = scatter_claim_bytes(table_blocks);
    unsigned *claimed = (unsigned *)workspace, *n_touched = (unsigned *)((char *)workspace + claim_bytes), *touched = n_touched + 4;
    if (hipMemsetAsync(workspace, 0, claim_bytes + 16, stream) != hipSuccess) return EMDR2_E_LAUNCH;
    int rc;
    if ((rc = mips_launch_write_rows_at(rows_rm, row_ids, n_upd, dim, n_rows_total, tiled, claimed, n_touched, touched, cap, stamp, stream))) return rc;
    if ((rc = mips_launch_block_norms_list(tiled, dim, touched, n_touched, cap, block_norm_sq, stream))) return rc;
    if ((rc = mips_launch_table_max(block_norm_sq, table_blocks, emax_sq, stream))) return rc;
    if (shadow) return mips_launch_seal_shadow_list(tiled, dim, touched, n_touched, cap, shadow, (float *)table, nonfinite, stream);
    return EMDR2_OK;
}

int emdr2_mips_update_rows_scattered(const void *rows_rm, const int64_t *row_ids, int64_t n_upd, int dim, int64_t n_rows_total, void *tiled,
                                     float *block_norm_sq, float *emax_sq, void *shadow, void *table, uint32_t *nonfinite, void *workspace,
                                     size_t workspace_bytes, emdr2_stream_t stream)
{
    return update_rows_scattered_impl(rows_rm, row_ids, n_upd, dim, n_rows_total, tiled, block_norm_sq, emax_sq, shadow, table, nonfinite, workspace,
                                      workspace_bytes, nullptr, stream);
}

int emdr2_mips_update_rows_scattered_stamped(const void *rows_rm, const int64_t *row_ids, int64_t n_upd, int dim, int64_t n_rows_total, void *tiled,
                                             float *block_norm_sq, float *emax_sq, void *shadow, void *table, uint32_t *nonfinite, void *workspace,
                                             size_t workspace_bytes, uint32_t *generation, uint32_t gen, int newest_wins, uint32_t *n_kept_newer,
                                             emdr2_stream_t stream)
{
    if (bad_stamp(generation, gen, n_kept_newer)) return EMDR2_E_BADARG;
    const RowStamp stamp = {generation, gen, newest_wins ? 1 : 0, n_kept_newer};
    return update_rows_scattered_impl(rows_rm, row_ids, n_upd, dim, n_rows_total, tiled, block_norm_sq, emax_sq, shadow, table, nonfinite, workspace,
                                      workspace_bytes, &stamp, stream);
}

static_assert(MIPS_GEN_WORDS == EMDR2_GEN_WORDS, "the report layout of include/emdr2_mips.h");
int emdr2_mips_generation_stats(const uint32_t *generation, int64_t n_rows, int64_t row_base, const int64_t *global_rows, int64_t n_sel, uint32_t now,
                                uint64_t *report, emdr2_stream_t stream)
{
    if (!report || ((uintptr_t)report & 7) || ((uintptr_t)generation & 3) || n_rows < 0 || row_base < 0 || (n_rows > 0 && !generation) ||
        (global_rows && n_sel < 0))
        return EMDR2_E_BADARG;
    return mips_launch_generation_stats(generation, n_rows, row_base, global_rows, global_rows ? n_sel : n_rows, now, report, (hipStream_t)stream);
}

// (row counts stay below 2^31: the kernels keep ranks and histogram words in 32 bits)
int emdr2_mips_oldest_rows_workspace_bytes(int64_t n_rows, size_t *bytes)
{
    if (!bytes || n_rows < 0 || n_rows >= ((int64_t)1 << 31)) return EMDR2_E_BADARG;
    *bytes = MIPS_OLDEST_WS_BYTES;
    return EMDR2_OK;
}

int emdr2_mips_oldest_rows(const uint32_t *generation, int64_t n_rows, int64_t row_base, uint32_t below, int64_t n_want, int64_t *out_rows,
                           uint64_t *out_info, void *workspace, size_t workspace_bytes, emdr2_stream_t stream)
{
    if (!out_info || ((uintptr_t)out_info & 7) || !workspace || ((uintptr_t)workspace & 15) || ((uintptr_t)generation & 3) || ((uintptr_t)out_rows & 7) ||
        n_rows < 0 || n_rows >= ((int64_t)1 << 31) || row_base < 0 || n_want < 0 || n_want > n_rows || (n_rows > 0 && !generation) ||
        (n_want > 0 && !out_rows))
        return EMDR2_E_BADARG;
    if (workspace_bytes < MIPS_OLDEST_WS_BYTES) return EMDR2_E_WORKSPACE;
    return mips_launch_oldest_rows(generation, n_rows, row_base, below, n_want, out_rows, out_info, workspace, (hipStream_t)stream);
}

int emdr2_mips_row_keys(const void *tiled, int64_t n_rows_total, int dim, int64_t row_offset, int64_t n_chunk, int64_t row_base,
                        const uint32_t *generation, uint64_t *keys, emdr2_stream_t stream)
{
    if (!tiled || !keys || ((uintptr_t)keys & 7) || ((uintptr_t)generation & 3) || bad_shape(n_rows_total, dim) || n_chunk < 0 || row_offset < 0 ||
        row_offset + n_chunk > n_rows_total || row_base < 0)
        return EMDR2_E_BADARG;
    return mips_launch_row_keys(tiled, dim, row_offset, n_chunk, row_base, generation, keys, (hipStream_t)stream);
}

// (row counts stay below 2^31, as for _oldest_rows)
int emdr2_mips_changed_rows_workspace_bytes(int64_t n_rows, size_t *bytes)
{
    if (!bytes || n_rows < 0 || n_rows >= ((int64_t)1 << 31)) return EMDR2_E_BADARG;
    *bytes = mips_changed_rows_workspace_bytes(n_rows);
    return EMDR2_OK;
}

int emdr2_mips_changed_rows(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const uint32_t *generation, const uint64_t *base_keys,
                            int64_t cap, int64_t *out_rows, uint64_t *out_info, void *workspace, size_t workspace_bytes, emdr2_stream_t stream)
{
    if (!out_info || ((uintptr_t)out_info & 7) || !workspace || ((uintptr_t)workspace & 15) || ((uintptr_t)generation & 3) ||
        ((uintptr_t)base_keys & 7) || ((uintptr_t)out_rows & 7) || n_rows >= ((int64_t)1 << 31) || bad_shape(n_rows, dim) || row_base < 0 || cap < 0 ||
        cap > n_rows || (n_rows > 0 && (!tiled || !base_keys)) || (cap > 0 && !out_rows))
        return EMDR2_E_BADARG;
    if (workspace_bytes < mips_changed_rows_workspace_bytes(n_rows)) return EMDR2_E_WORKSPACE;
    return mips_launch_changed_rows(tiled, n_rows, dim, row_base, generation, base_keys, cap, out_rows, out_info, workspace, (hipStream_t)stream);
}

int emdr2_mips_audit(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const float *emax_sq, const float *block_norm_sq,
                     const void *shadow, const void *table, uint64_t *report, emdr2_stream_t stream)
{
    if (!tiled || !emax_sq || !report || ((uintptr_t)report & 7) || row_base < 0 || bad_shape(n_rows, dim)) return EMDR2_E_BADARG;
    if ((shadow == nullptr) != (table == nullptr)) return EMDR2_E_BADARG;
    if (shadow && (((uintptr_t)table & 15) || (dim % 256) != 0)) return EMDR2_E_BADARG;
    const AuditParams p = {(const char *)tiled, (const char *)shadow, (const float4 *)table, block_norm_sq, emax_sq, (unsigned long long *)report,
                           n_rows, row_base, (n_rows + 255) / 256, dim / 32};
    return mips_launch_audit(p, (hipStream_t)stream);
}

int emdr2_mips_search_shadow(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const float *emax_sq, const void *shadow,
                             const void *table, int64_t shadow_min_rows, const void *queries, int n_q, int k, const int32_t *ids, int f32,
                             void *out_dist, int32_t *out_idx, int64_t *out_row, void *out_records, uint32_t *out_flags, void *workspace,
                             size_t workspace_bytes, emdr2_stream_t stream)
{
    if (!shadow || !table || ((uintptr_t)table & 15) || shadow_min_rows < 1 || (dim % 256) != 0) return EMDR2_E_BADARG;
    const Shadow sh = {shadow, (const float *)table, shadow_min_rows};
    return search_impl(tiled, n_rows, dim, row_base, emax_sq, queries, n_q, k, ids, out_dist, out_idx, out_row, out_flags, workspace,
                       workspace_bytes, stream, f32 ? 1 : 0, (uint4 *)out_records, &sh);
}

int emdr2_mips_shadow_launches(void) { return (int)g_shadow_launches; }

int emdr2_mips_merge_records(const void *records_in, int n_shards, int n_q, int k, int f32, void *out_dist, int32_t *out_idx, int64_t *out_row,
                             emdr2_stream_t stream)
{
    if (!records_in || ((uintptr_t)records_in & 15) || !out_dist || !out_idx || !out_row || n_shards < 1 || n_q < 1 || k < 1) return EMDR2_E_BADARG;
    return mips_launch_merge_records((const uint4 *)records_in, n_shards, n_q, k, f32 ? 1 : 0, out_dist, out_idx, out_row, (hipStream_t)stream);
}

int emdr2_mips_pack_records(const void *dist, const int32_t *idx, const int64_t *row, const int32_t *sel, int n_sel, int k, int f32,
                            void *records, emdr2_stream_t stream)
{
    if (!dist || !idx || !row || !sel || !records || ((uintptr_t)records & 15) || n_sel < 0 || k < 1) return EMDR2_E_BADARG;
    return mips_launch_pack_records(dist, idx, row, sel, n_sel, k, f32 ? 1 : 0, (uint4 *)records, (hipStream_t)stream);
}

// the all-exact fallback and the array merge, once for both score formats: the ordered keys of a pass take 2 (fp16) or 4 (fp32) bytes per row
static int exact_workspace_impl(int64_t n_rows, int n_sel, size_t *bytes, size_t key_bytes)
{
    if (!bytes || n_rows < 1 || n_sel < 0) return EMDR2_E_BADARG;
    *bytes = align_up((size_t)8 * (size_t)n_rows * key_bytes, 256);
    return EMDR2_OK;
}

static int search_exact_impl(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const void *queries, int n_q, const int32_t *sel,
                             int n_sel, int k, const int32_t *ids, void *out_dist, int32_t *out_idx, int64_t *out_row, uint32_t *out_flags,
                             void *workspace, size_t workspace_bytes, emdr2_stream_t stream_, int f32)
{
    if (!tiled || !queries || !sel || !out_dist || !out_idx || !out_row || !out_flags || !workspace) return EMDR2_E_BADARG;
    if (n_q < 1 || n_sel < 0 || k < 1 || k > EMDR2_MAX_TOPK || bad_shape(n_rows, dim) || n_rows < 1) return EMDR2_E_BADARG;
    if (workspace_bytes < (size_t)8 * (size_t)n_rows * (f32 ? sizeof(uint32_t) : sizeof(uint16_t))) return EMDR2_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    for (int b = 0; b < n_sel; b += 8) {
        const int nb = (n_sel - b) < 8 ? (n_sel - b) : 8;
        int rc;
        if ((rc = mips_launch_exact_scores((const char *)tiled, n_rows, dim, (const uint16_t *)queries, sel + b, nb, f32, workspace, stream))) return rc;
        if ((rc = mips_launch_exact_select(workspace, n_rows, row_base, sel + b, nb, k, ids, f32, out_dist, out_idx, out_row, out_flags, stream)))
            return rc;
    }
    return EMDR2_OK;
}

static int merge_impl(const void *dist_in, const int32_t *idx_in, const int64_t *row_in, int n_shards, int n_q, int k, void *out_dist,
                      int32_t *out_idx, int64_t *out_row, emdr2_stream_t stream, int f32)
{
    if (!dist_in || !idx_in || !row_in || !out_dist || !out_idx || !out_row || n_shards < 1 || n_q < 1 || k < 1) return EMDR2_E_BADARG;
    return mips_launch_merge(dist_in, idx_in, row_in, n_shards, n_q, k, f32, out_dist, out_idx, out_row, (hipStream_t)stream);
}

int emdr2_mips_exact_workspace_bytes(int64_t n_rows, int n_sel, size_t *bytes) { return exact_workspace_impl(n_rows, n_sel, bytes, sizeof(uint16_t)); }

int emdr2_mips_exact_workspace_bytes_f32(int64_t n_rows, int n_sel, size_t *bytes) { return exact_workspace_impl(n_rows, n_sel, bytes, sizeof(uint32_t)); }

int emdr2_mips_search_exact(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const void *queries,
                            int n_q, const int32_t *sel, int n_sel, int k, const int32_t *ids, void *out_dist,
                            int32_t *out_idx, int64_t *out_row, uint32_t *out_flags, void *workspace,
                            size_t workspace_bytes, emdr2_stream_t stream)
{
    return search_exact_impl(tiled, n_rows, dim, row_base, queries, n_q, sel, n_sel, k, ids, out_dist, out_idx, out_row, out_flags, workspace,
                             workspace_bytes, stream, 0);
}

int emdr2_mips_search_exact_f32(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const void *queries,
                                int n_q, const int32_t *sel, int n_sel, int k, const int32_t *ids, float *out_dist,
                                int32_t *out_idx, int64_t *out_row, uint32_t *out_flags, void *workspace,
                                size_t workspace_bytes, emdr2_stream_t stream)
{
    return search_exact_impl(tiled, n_rows, dim, row_base, queries, n_q, sel, n_sel, k, ids, out_dist, out_idx, out_row, out_flags, workspace,
                             workspace_bytes, stream, 1);
}

int emdr2_mips_merge(const void *dist_in, const int32_t *idx_in, const int64_t *row_in, int n_shards, int n_q, int k,
                     void *out_dist, int32_t *out_idx, int64_t *out_row, emdr2_stream_t stream)
{
    return merge_impl(dist_in, idx_in, row_in, n_shards, n_q, k, out_dist, out_idx, out_row, stream, 0);
}

int emdr2_mips_merge_f32(const float *dist_in, const int32_t *idx_in, const int64_t *row_in, int n_shards, int n_q, int k,
                         float *out_dist, int32_t *out_idx, int64_t *out_row, emdr2_stream_t stream)
{
    return merge_impl(dist_in, idx_in, row_in, n_shards, n_q, k, out_dist, out_idx, out_row, stream, 1);
}

int emdr2_mips_debug_scores(const void *tiled, int64_t n_rows, int dim, const void *queries, int n_q,
                            float *out_scores, void *workspace, size_t workspace_bytes, emdr2_stream_t stream_)
{
    if (!tiled || !queries || !out_scores || !workspace || n_q < 1 || n_q > 512 || bad_shape(n_rows, dim) || n_rows < 1) return EMDR2_E_BADARG;
    Workspace w;
    if (carve((char *)workspace, dim, &w) > workspace_bytes) return EMDR2_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const int variant = mips_scan_variant(n_q, EXP_ENV_INT("EMDR2_MIPS_VARIANT", -1));
    const int BM = kMipsBM[variant], BN = kMipsBN[variant];
    int rc;
    PrepareParams pp = {};                                   // (the query image alone: a dense scan has no thresholds and no lists)
    pp.queries = queries;
    pp.n_q = n_q;
    pp.dim = dim;
    pp.bn = BN;
    pp.q_tiled = w.q_tiled;
    pp.qnorm = w.qnorm;
    if ((rc = mips_launch_prepare(pp, stream))) return rc;
    ScanParams sp;
    sp.e_tiled = (const char *)tiled;
    sp.q_tiled = w.q_tiled;
    sp.tau = w.tau;
    sp.cand = w.cand;
    sp.count = w.count;
    sp.flags = nullptr;
    sp.dense_out = out_scores;
    sp.nch = dim / 32;
    sp.n_rows = (int)n_rows;
    sp.n_q = n_q;
    sp.capq = CAPQ;
    sp.cand8 = nullptr;
    sp.count8 = nullptr;
    sp.dense_row0 = 0;
    sp.tune = 1;
    sp.trace = nullptr;
    sp.tile_begin = 0;
    sp.tile_end = (int)((n_rows + BM - 1) / BM);
    const int cus = device_cu_count();
    return mips_launch_scan(variant, 2, sp, sp.tile_end < cus ? sp.tile_end : cus, stream);
}

} // extern "C"
