// emdr2_amd/csrc/tile_order.h -- the L2-group tile order of the NT GEMM kernels (gemm.hip with its 1-D grid, gemm8.hip): the host plans it, the
// device decodes it, both here and nowhere else.  No HIP include: tests/test_tile_order_cpu.py compiles this file as plain host C++.
//
// Workgroup ids are dealt round-robin to the 8 XCDs, each with its own 4 MB L2, and every XCD walks one contiguous range of the tile sequence
// (gemm_common.h: xcd_per).  The sequence is ordered so that what is shared stays in that L2: n-tiles are taken in groups of `ngroup` B panels
// that fit the L2 (a BN x K panel of the weight matrix each), and inside a group the walk is n-fastest, so the tiles sharing an A panel run back
// to back.  A then leaves HBM once per group (N = 3072, K = 768: twice instead of 12 times) and B stays L2-resident instead of cycling through a
// working set larger than the cache.
#ifndef EMDR2_TILE_ORDER_H
#define EMDR2_TILE_ORDER_H
#include <stdint.h>

#ifdef __HIPCC__
#define TILE_ORDER_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define TILE_ORDER_FN inline
#endif

struct TileOrder {
    int tiles_m, tiles_n, ngroup;               // ngroup: n-tiles per group; the last group may be narrower
    uint32_t mg_full, mg_group, mg_last;        // ceil(2^32 / d) for d = ngroup * tiles_m, ngroup, width of the last group; 0 encodes d == 1
};

// Plan for tiles_m x tiles_n tiles of BN columns over a [N, K] bf16 B.  l2_kib: what the B panels of one group may occupy (2560: about half of a
// 4 MB L2, the rest holds the A panels in flight and the output lines in transit).  One group (plain n-fastest) when B is at most single_kib
// (4096: it fits the L2 whole -- N = 2304, K = 768 measured 1.7 % better ungrouped, N = 3072 2.3 % better grouped), or when the panels are so
// large (K = 3072) that grouping would re-read A 3+ times.  force_ng > 0 (experiment builds) replaces that choice.
inline TileOrder tile_order_plan(int tiles_m, int tiles_n, int BN, int K, int N, long long l2_kib, long long single_kib, int force_ng = 0)
{
    const long long panel = (long long)BN * K * 2;
    int ng = (int)(l2_kib * 1024 / panel);
    if (ng < 1) ng = 1;
    if (ng > tiles_n || 2 * ng < tiles_n || (long long)N * K * 2 <= (single_kib << 10)) ng = tiles_n;
    if (force_ng > 0) ng = force_ng < tiles_n ? force_ng : tiles_n;
    if (tiles_m == 1) ng = tiles_n;                             // no A panel to share between groups (and no group of ONE tile for the decoder)
    // balance the groups: e.g. 9 n-tiles with room for 6 -> 5 + 4 rather than 6 + 3
    const int groups = (tiles_n + ng - 1) / ng;
    TileOrder o;
    o.tiles_m = tiles_m; o.tiles_n = tiles_n;
    o.ngroup = (tiles_n + groups - 1) / groups;
    const int last = tiles_n - (groups - 1) * o.ngroup;
    auto magic = [](long long d) { return d > 1 ? (uint32_t)(((1ull << 32) + (unsigned long long)d - 1) / (unsigned long long)d) : 0u; };
    o.mg_full = magic((long long)o.ngroup * tiles_m); o.mg_group = magic(o.ngroup); o.mg_last = magic(last);
    return o;
}

TILE_ORDER_FN uint32_t tile_order_mulhi(uint32_t a, uint32_t b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// x / d by the rounded-up reciprocal mg = ceil(2^32 / d): never too small, and too large by at most one (the excess is < x / 2^32 < 1) -- which it
// IS once x * (mg * d - 2^32) reaches 2^32, e.g. from tile 59,075 on for d = 6 x 12,800 tiles (M = 3.3M rows, N = 3072: top-k 100): one compare
// puts it right for every 0 <= x < 2^31 with x * d inside an int (the callers keep the tile count below 2^24)
TILE_ORDER_FN int tile_order_div(int x, uint32_t mg, int d)
{
    int q = (int)tile_order_mulhi((uint32_t)x, mg);
    if (q * d > x) --q;
    return q;
}

// sequence position -> tile coordinates
TILE_ORDER_FN void tile_order_coords(const TileOrder &o, int pos, int &tm, int &tn)
{
    const int full = o.ngroup * o.tiles_m;                      // tiles in one full group: >= 2, or the only tile (the plan sees to it)
    const int g = tile_order_div(pos, o.mg_full, full);
    const int r = pos - g * full;
    const bool whole = (g + 1) * o.ngroup <= o.tiles_n;
    const int gsize = whole ? o.ngroup : o.tiles_n - g * o.ngroup;
    const uint32_t mg = whole ? o.mg_group : o.mg_last;
    tm = mg ? tile_order_div(r, mg, gsize) : r;
    tn = g * o.ngroup + (r - tm * gsize);
}
#endif
