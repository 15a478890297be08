// emdr2_amd/csrc/param_stats.hip -- per-parameter statistics of one FlatAdam bucket (include/emdr2_ops.h, "Parameter statistics"): ONE
// streaming pass over the fp32 gradients, masters and both Adam moments -- 16 bytes per element, each read once -- that leaves, for every
// parameter of the bucket, the squared sums of its gradient, its weights and its Adam direction, both maxima and two counts.  Two plain
// launches: a record per item (a chunk of at most 8192 elements of ONE parameter) into the workspace, then one wave per parameter that
// folds its items' records.  No atomics and no hand-off between workgroups: the order of every floating-point addition is the one the
// header states, so the words do not depend on the device or on the arrival order of anything.
#include "../../include/emdr2_ops.h"
#include "prims.h"
#include "adam_bias.h"

namespace {

constexpr int PARAM_STATS_CHUNK = 8192;                                  // elements per item: 8 steps of 256 threads x 4 elements
constexpr int PARAM_STATS_GRID_CAP = 1024;
// record / output words (the header fixes them)
enum { W_GSQ = 0, W_WSQ = 1, W_DSQ = 2, W_GMAX = 3, W_WMAX = 4, W_ZEROS = 5, W_NONFINITE = 6, W_COUNT = 7, W_WORDS = 8 };

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v, o); v = w > v ? w : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// Workgroup g takes items g, g + grid, ...; thread t takes the 4-element groups t, t + 256, ... of the item: one 16-byte load of each array
// (item starts are multiples of 8 elements).  Elements at or beyond the item's end -- the tail of a parameter's last group, which is
// padding -- are masked out one by one, by selects: the loads stay whole and the loop has no branch per element.  WITH_D == false (step 0): m and v are not read and the direction's sum stays 0.
template <bool WITH_D>
__global__ void __launch_bounds__(256) param_stats_partial_kernel(const float4 *__restrict__ master, const float4 *__restrict__ grad,
                                                                  const float4 *__restrict__ m, const float4 *__restrict__ v, long long n,
                                                                  const long long *__restrict__ items, long long n_items, float bc1, float bc2,
                                                                  float eps, unsigned long long *__restrict__ records)
{
    __shared__ double shd[3][4];
    __shared__ uint32_t shu[3][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long it = blockIdx.x; it < n_items; it += gridDim.x) {
        const long long start = items[2 * it];
        long long len = items[2 * it + 1];
        if (start < 0 || (start & 7) || len < 0 || len > PARAM_STATS_CHUNK || start + len > n) len = 0;      // (never, with a plan of the entry)
        const int ilen = (int)len, groups = (ilen + 3) >> 2;
        const long long base4 = start >> 2;
        double gsq = 0.0, wsq = 0.0, dsq = 0.0;
        uint32_t gmax = 0u, wmax = 0u, cnt = 0u;                         // cnt: zeros in the low half, non-finite in the high one (<= 8192 each)
#pragma unroll 2
        for (int grp = tid; grp < groups; grp += 256) {
            const float4 g4 = grad[base4 + grp], w4 = master[base4 + grp];
            float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = m4;
            if constexpr (WITH_D) { m4 = m[base4 + grp]; v4 = v[base4 + grp]; }
            const float g[4] = {g4.x, g4.y, g4.z, g4.w}, w[4] = {w4.x, w4.y, w4.z, w4.w};
            const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // branch-free: a masked element enters as g = w = m = v = +0, which adds 0.0 to every sum (d = 0 / (0 + eps)), and is kept
                // out of the counts
                const bool in = 4 * grp + e < ilen;
                const float ge = in ? g[e] : 0.f, we = in ? w[e] : 0.f;
                const double gd = (double)ge, wd = (double)we;
                gsq += gd * gd;                                          // (an fp32 square is exact in double: only the order of the additions counts)
                wsq += wd * wd;
                if constexpr (WITH_D) {
                    const float me = in ? mm[e] : 0.f, ve = in ? vv[e] : 0.f;
                    const float d = (me / bc1) / (sqrtf(ve / bc2) + eps);                // adam_flat_kernel's statement, without weight decay
                    const double dd = (double)d;
                    dsq += dd * dd;
                }
                const uint32_t ga = __float_as_uint(ge) & 0x7fffffffu, wa = __float_as_uint(we) & 0x7fffffffu;
                gmax = (ga <= 0x7f800000u && ga > gmax) ? ga : gmax;     // a NaN stays out of the maxima, an Inf is in
                wmax = (wa <= 0x7f800000u && wa > wmax) ? wa : wmax;
                cnt += ((in && ga == 0u) ? 1u : 0u) + (ga >= 0x7f800000u ? 0x10000u : 0u);
            }
        }
        gsq = wave_sum_f64(gsq); wsq = wave_sum_f64(wsq);
        if constexpr (WITH_D) dsq = wave_sum_f64(dsq);
        gmax = wave_max_u32(gmax); wmax = wave_max_u32(wmax); cnt = wave_sum_u32(cnt);
        __syncthreads();                                                 // (the arrays may still be read from the previous item)
        if (lane == 0) {
            shd[0][wave] = gsq; shd[1][wave] = wsq; shd[2][wave] = dsq;
            shu[0][wave] = gmax; shu[1][wave] = wmax; shu[2][wave] = cnt;
        }
        __syncthreads();
        if (tid < W_WORDS) {
            unsigned long long word;
            if (tid <= W_DSQ) word = (unsigned long long)__double_as_longlong((shd[tid][0] + shd[tid][1]) + (shd[tid][2] + shd[tid][3]));
            else if (tid <= W_WMAX) {
                const uint32_t a = shu[tid - W_GMAX][0] > shu[tid - W_GMAX][1] ? shu[tid - W_GMAX][0] : shu[tid - W_GMAX][1];
                const uint32_t b = shu[tid - W_GMAX][2] > shu[tid - W_GMAX][3] ? shu[tid - W_GMAX][2] : shu[tid - W_GMAX][3];
                word = a > b ? a : b;
            } else {
                const uint32_t c = shu[2][0] + shu[2][1] + shu[2][2] + shu[2][3];
                word = tid == W_ZEROS ? (c & 0xffffu) : tid == W_NONFINITE ? (c >> 16) : (unsigned long long)ilen;
            }
            records[it * W_WORDS + tid] = word;
        }
    }
}

// words 0-2 are double sums, 3-4 integer maxima, 5-7 integer sums
__device__ __forceinline__ unsigned long long fold_word(int word, unsigned long long a, unsigned long long b)
{
    if (word <= W_DSQ) return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
    if (word <= W_WMAX) return a > b ? a : b;
    return a + b;
}

// One wave per parameter.  Lane l holds word (l & 7) of lane group s = l >> 3; group s folds the records of the parameter's items s, s + 8,
// ... in ascending order from 0, then the eight groups meet in the xor butterfly over s: 4, 2, 1 (lane offsets 32, 16, 8).
__global__ void __launch_bounds__(64) param_stats_fold_kernel(const unsigned long long *__restrict__ records, long long n_items,
                                                              const long long *__restrict__ first, unsigned long long *__restrict__ out)
{
    const int word = threadIdx.x & 7, s = threadIdx.x >> 3;
    const long long p = blockIdx.x;
    long long lo = first[p], hi = first[p + 1];
    if (lo < 0 || hi > n_items || hi < lo) hi = lo = 0;                  // (never, with a plan of the entry)
    unsigned long long acc = 0ull;                                       // +0.0 as a double
#pragma unroll 4
    for (long long it = lo + s; it < hi; it += 8) acc = fold_word(word, acc, records[it * W_WORDS + word]);
#pragma unroll
    for (int o = 32; o >= 8; o >>= 1) acc = fold_word(word, acc, __shfl_xor(acc, o));
    if (s == 0) out[p * W_WORDS + word] = acc;
}

} // namespace

extern "C" int emdr2_param_stats_plan(const int64_t *offsets, const int64_t *lengths, int64_t n_params, int64_t n, int64_t *items, int64_t *first,
                                      int64_t *n_items)
{
    if (!offsets || !lengths || !first || !n_items || n_params < 1 || n < 8 || (n & 7)) return -1;
    int64_t end = 0;                                                     // end of the previous parameter
    for (int64_t p = 0; p < n_params; ++p) {
        const int64_t off = offsets[p], len = lengths[p];
        if (off < end || (off & 7) || len < 1 || len > n || off > n - len) return -1;
        end = off + len;
    }
    int64_t count = 0;
    for (int64_t p = 0; p < n_params; ++p) {
        first[p] = count;
        for (int64_t at = 0; at < lengths[p]; at += PARAM_STATS_CHUNK, ++count) {
            if (!items) continue;
            items[2 * count] = offsets[p] + at;
            items[2 * count + 1] = lengths[p] - at < PARAM_STATS_CHUNK ? lengths[p] - at : PARAM_STATS_CHUNK;
        }
    }
    first[n_params] = count;
    *n_items = count;
    return 0;
}

extern "C" int emdr2_param_stats_ws_bytes(int64_t n_items, size_t *bytes)
{
    if (!bytes || n_items < 1) return -1;
    *bytes = (size_t)n_items * W_WORDS * 8;
    return 0;
}

extern "C" int emdr2_param_stats(const float *master, const float *grad, const float *m, const float *v, int64_t n, const int64_t *items,
                                 int64_t n_items, const int64_t *first, int64_t n_params, float beta1, float beta2, float eps, int step,
                                 uint64_t *workspace, uint64_t *out, void *stream)
{
    if (!master || !grad || !m || !v || !items || !first || !workspace || !out) return -1;
    if (n < 8 || (n & 7) || n_items < 1 || n_params < 1 || n_params > n_items || step < 0) return -1;
    if ((((uintptr_t)master | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15) ||
        (((uintptr_t)items | (uintptr_t)first | (uintptr_t)workspace | (uintptr_t)out) & 7)) return -1;
    const int64_t grid = n_items < PARAM_STATS_GRID_CAP ? n_items : PARAM_STATS_GRID_CAP;      // a function of the plan alone
    float bc1 = 1.f, bc2 = 1.f;
    if (step > 0) adam_bias_corrections(beta1, beta2, step, &bc1, &bc2);
    launch(step > 0 ? param_stats_partial_kernel<true> : param_stats_partial_kernel<false>, dim3((unsigned)grid), 256, stream, master, grad, m, v,
           n, items, n_items, bc1, bc2, eps, workspace);
    launch(param_stats_fold_kernel, dim3((unsigned)n_params), 64, stream, workspace, n_items, first, out);
    return LAUNCH_OK();
}
