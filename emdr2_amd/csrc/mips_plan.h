// emdr2_amd/csrc/mips_plan.h -- the segment schedule of one MIPS search pass (<= 512 queries), as a value.
//
// THE statement of "which rows run on which engine": search_impl (mips_api.hip) plans a pass with mips_plan_search and then only executes
// the plan, the launchers of the persistent scan (mips_scan8.h, mips_scan8i.hip) answer -4 by the two predicates below, and
// emdr2_mips_search_plan (include/emdr2_mips.h) shows the plan to tests and tools.  Host-only and free of HIP: it compiles into a plain C++
// program as it does into the library.
#pragma once
#include <stdint.h>

// Tuning knobs of a search.  The product build runs the defaults (search_knobs in mips_api.hip); only -DEMDR2_EXPERIMENTS builds read them
// from the environment.
struct SearchKnobs {
    int seg0;            // rows of the dense first segment, a multiple of 512
    int growth;          // the next segment ends at `growth` times the rows done so far ...
    int growth_i8;       // ... at `growth_i8` times once a segment of that length runs on the int8 shadow image
    float margin_i8;     // an int8 survivor is re-scored right after its segment iff estimate + margin_i8 * eps reaches tau: speed only
    int cus;             // compute units the scans are sized for
    int force_variant;   // 0..2: that tile variant wherever its query image holds the pass; else the variant follows the query count
    int scan_kernel;     // 1 = the production kernels; other values: experiment kernels that take the LOCKSTEP segments
    int ablate;          // timing experiments only
    int tune;            // ScanParams::tune
    int couple;          // != 0: the first 8 persistent launches of a pass pace their workgroup pairs through progress counters
};

enum ScanEngine {
    DENSE,               // mips_scan_kernel MODE 1: the first segment, every score written
    LOCKSTEP,            // mips_scan_kernel MODE 0: <= 128 queries, and what the persistent scan does not cover
    PERSISTENT_F16,      // mips_scan8_kernel<Scan8Fp16>
    PERSISTENT_I8        // mips_scan8_kernel<Scan8Int8> on the shadow image; a triage launch follows
};

struct SearchSegment {
    int64_t row_begin, row_end;
    ScanEngine engine;
    bool select_after;   // a select launch follows the segment (the select after the LAST segment runs inside the finalize launch -- after a
                         // select of its own when something is pending: the deferred pass, the first thing that launch does then, wants
                         // the tightest tau)
    int prog_slot;       // which of the pass's 8 sets of pair-progress counters a persistent launch paces itself with, or -1: none
};

#define MIPS_PLAN_MAX_SEGMENTS 32 /* seg0 >= 512, growth >= 2 and n_rows < 2^31 give at most 23 */

struct SearchPlan {
    int variant, bm, bn; // tile variant: 0 = 128 rows x 512 queries, 1 = 256 x 256, 2 = 512 x 128
    int kp;              // candidates kept per query: 64 or 128
    bool pack_q8;        // the prepare launch also packs the int8 query image: some segment of this search may take the int8 path
    bool any_pending;    // some int8 segment runs: its deferred survivors wait for the finalize launch
    int n_segments;
    SearchSegment seg[MIPS_PLAN_MAX_SEGMENTS];
};

static const int kMipsBM[3] = {128, 256, 512};
static const int kMipsBN[3] = {512, 256, 128};

inline int mips_scan_variant(int nq, int force_variant)
{
    if (force_variant >= 0 && force_variant <= 2 && kMipsBN[force_variant] >= nq) return force_variant;
    return nq <= 128 ? 2 : (nq <= 256 ? 1 : 0);
}

// workgroups of a persistent scan launch: a multiple of 8 XCDs x an even number of workgroups each
inline int mips_persistent_grid(int cus) { return (cus & ~15) < 16 ? 16 : (cus & ~15); }

// The persistent scan covers rows [b, e) with a query image of `bn` rows and `nch` chunks per row of the image it reads (32 fp16 or 64 int8
// values each): K-tiles come in pairs of pairs, items are 256 rows x 256 queries, and a segment with fewer items than the launch has
// workgroups stays on the lock-step kernel.
inline bool mips_persistent_covers(int bn, int nch, int cus, int64_t b, int64_t e)
{
    if ((bn != 256 && bn != 512) || (nch & 3) || nch < 4 || (b & 255) || e <= b) return false;
    return (((e + 255) >> 8) - (b >> 8)) * (bn / 256) >= mips_persistent_grid(cus);
}

// ... and its int8 instance, whose image has half as many chunks per row as the fp16 image has (`nch` = dim / 32)
inline bool mips_int8_covers(int bn, int nch, int cus, int64_t b, int64_t e) { return (nch & 7) == 0 && mips_persistent_covers(bn, nch / 2, cus, b, e); }

// The plan of one pass of `nq` (1..512) queries over n_rows rows of dimension `dim`; shadow_min_rows < 0: the shard has no int8 shadow
// image, else segments of at least that many rows run on it.  0, or -1 if the plan does not fit (it is never truncated).
inline int mips_plan_search(int64_t n_rows, int nq, int dim, int k, int64_t shadow_min_rows, const SearchKnobs &kn, SearchPlan *plan)
{
    const int v = mips_scan_variant(nq, kn.force_variant), bn = kMipsBN[v], nch = dim / 32;
    const int64_t dense_rows = n_rows < kn.seg0 ? n_rows : kn.seg0;
    // the persistent scan takes 256- and 512-row query images; in experiment builds the other kernels and the ablations take its segments
    const bool persistent = v <= 1 && kn.scan_kernel == 1 && !(v == 0 && kn.ablate > 0);
    plan->variant = v;
    plan->bm = kMipsBM[v];
    plan->bn = bn;
    plan->kp = k <= 56 ? 64 : 128;
    plan->pack_q8 = shadow_min_rows >= 0 && v <= 1 && kn.scan_kernel == 1 && (dim % 256) == 0 && n_rows - dense_rows >= shadow_min_rows;
    plan->n_segments = 0;
    int persistent_launches = 0;                             // (fp16 and int8 launches share the progress counters: both count)
    bool pending = false;
    int64_t done = 0, end = dense_rows;
    while (done < n_rows) {
        if (plan->n_segments == MIPS_PLAN_MAX_SEGMENTS) return -1;
        SearchSegment &s = plan->seg[plan->n_segments++];
        s.row_begin = done;
        s.row_end = end;
        if (done == 0) s.engine = DENSE;
        else if (persistent && plan->pack_q8 && end - done >= shadow_min_rows && mips_int8_covers(bn, nch, kn.cus, done, end)) s.engine = PERSISTENT_I8;
        else if (persistent && mips_persistent_covers(bn, nch, kn.cus, done, end)) s.engine = PERSISTENT_F16;
        else s.engine = LOCKSTEP;
        s.prog_slot = -1;
        if (s.engine == PERSISTENT_F16 || s.engine == PERSISTENT_I8) {
            if (kn.couple && persistent_launches < 8) s.prog_slot = persistent_launches;
            ++persistent_launches;
        }
        pending = pending || s.engine == PERSISTENT_I8;
        s.select_after = end < n_rows || pending;
        done = end;
        // the next segment ends at `growth` times the rows done so far -- at `growth_i8` times once a segment of that length runs on the int8
        // image: its survivors are ~6 x the fp16 filter's and each costs a 1.5 KB gather in the re-score, so a fresher threshold pays there
        const int64_t next = done * ((plan->pack_q8 && done * (kn.growth_i8 - 1) >= shadow_min_rows) ? kn.growth_i8 : kn.growth);
        end = next < n_rows ? next : n_rows;
        if (n_rows - end < end / 2) end = n_rows;            // do not leave a short tail for a last launch (a launch + a select cost ~70 us)
    }
    plan->any_pending = pending;
    return 0;
}
