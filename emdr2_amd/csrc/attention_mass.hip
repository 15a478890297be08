// emdr2_amd/csrc/attention_mass.hip -- attention probability mass per key segment (include/emdr2_ops.h: emdr2_attention_key_mass).
//
// The fused forward never materialises P; it leaves the row statistics (m, l).  This kernel observes a forward launch from the side: it
// rebuilds p_ij = exp(s_ij - (m_i + ln l_i)) from the same q, k, token ids and statistics (the pre-dropout probability, masked scores
// REPLACED by -10000 like the forward) and sums it over the keys of each segment and the weighted real queries:
//     mass[b, h, g] (+)= sum_{i : ids_q[b, i] != 0} w[b, i] sum_{j in seg g} p_ij
// One workgroup per (sequence, head, segment): it alone writes mass[b, h, g], in a fixed order and without atomics, and its division of
// the work depends on that segment's extent and on sq only -- the bits of a question do not depend on what it is batched with.
//   S^T[key, q] = K[key, :] . Q[q, :]   v_mfma_f32_16x16x32_bf16, A = 16 keys, B = 16 queries, two k-steps over the 64 head dims.
//   The C layout gives lane (q = lane & 15, group = lane >> 4) the keys 4 group + {0..3} of its ONE query: the query's offset
//   (m + ln l) log2 e, its weight and its running sum are per-lane scalars and nothing crosses lanes before the final reduction.
// Both operands come straight from global memory in MFMA fragment order (lane: row lane & 15, 16 bytes at d = 32 t + 8 (lane >> 4)): a key
// row's 128 bytes are read whole by four lanes, each key once per pair of 16-query tiles (once in all for the decoder's 32 positions), so
// there is no LDS tile and no barrier in the loop; the four waves take every fourth 16-key group of the segment.
// Reduction order (fixed): a lane adds its 4 keys per group, group after group; times the weight; query tiles in order; the 64 lanes by a
// 6-level butterfly; the 4 waves in order through the LDS.
//
// Key weights (emdr2_attention_key_mass_weighted): the kernel is a template over "has key weights".  The weighted instance multiplies
// each p_ij by kw[h, key row] before the same additions in the same order -- a lane's 4 keys per group belong to ONE head, so kw costs
// four floats per lane and 16-key group, loaded with the next group's key rows (under the current group's MFMAs) from the row index
// CLAMPED like the key-row load: nothing outside [lo_key, hi_key) of the segment is read, four scalar 4-byte loads, no alignment assumed.
// A key past the segment end contributes by SELECT, so kw outside every segment may hold anything.  The unweighted instance compiles
// none of it.
//
// emdr2_head_row_norms: norm[h, r] = sqrt(sum_d x[r, h, d]^2), the per-key weight of value-norm weighted attention (||v_j||_2).  One
// (row, head) = 128 bytes = 8 lanes x 16 bytes; heads fastest, so a wave reads 8 consecutive heads of a row.  Order of additions (fixed):
// a lane squares its 8 values (exact in fp32: bf16 x bf16) and adds them in order d = 0..7 -- 7 additions --, then a 3-level xor
// butterfly over the 8 lanes (1, 2, 4) -- 3 more: depth 10 --, one square root (within one fp32 ulp), lane 0 of the 8 stores.  No atomics.
#include "../../include/emdr2_ops.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attention_common.h"

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

#define MASS_WAVES 4
#define MASS_QT 16      // queries per MFMA tile
#define MASS_KG 16      // keys per MFMA tile

struct MassParams {
    const char *q, *k;
    const long long *ids_q, *ids_k;
    long long q_sb, q_ss, q_sn, k_sb, k_ss, k_sn;
    const int *cu_k, *seg;
    const float *m, *l, *w, *kw;
    long long kw_ld;
    float *mass;
    int batch, heads, sq, sk, n_seg, accumulate;
    float scale;
};

template <bool KW>
__global__ void __launch_bounds__(MASS_WAVES * 64) attention_key_mass_kernel(MassParams p)
{
    __shared__ float wave_sum[MASS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, grp = lane >> 4;
    // heads fastest: the heads of a (sequence, segment) read the 128-byte slices of the SAME key rows, close together in time
    const int n = blockIdx.x % p.heads;
    const int bg = blockIdx.x / p.heads;
    const int g = bg % p.n_seg, b = bg / p.n_seg;

    // this sequence's keys and the segment inside them, clamped to the sequence whatever the table says
    long long krow0 = (long long)b * p.sk, k_off = (long long)b * p.k_sb;
    int len = p.sk;
    if (p.cu_k) { const int c0 = p.cu_k[b]; len = p.cu_k[b + 1] - c0; krow0 = c0; k_off = (long long)c0 * p.k_ss; }
    const int *seg = p.seg + (long long)b * (p.n_seg + 1) + g;
    const int hi_key = max(min(seg[1], len), 0);
    const int lo_key = max(min(seg[0], hi_key), 0);
    const int nkeys = hi_key - lo_key;
    const int ngroups = (nkeys + MASS_KG - 1) / MASS_KG;

    const char *kbase = p.k + (k_off + (long long)n * p.k_sn) * 2 + grp * 16;                 // + key * k_ss * 2 (+ 64: second k-step)
    const char *qbase = p.q + ((long long)b * p.q_sb + (long long)n * p.q_sn) * 2 + grp * 16;
    const long long stat0 = ((long long)b * p.heads + n) * p.sq;
    const float sc2 = p.scale * L2E;
    const float *kwbase = KW ? p.kw + (long long)n * p.kw_ld + krow0 + lo_key : nullptr;   // + key index inside the segment

    float total = 0.f;
    if (wave < ngroups) {
        const int nqt = (p.sq + MASS_QT - 1) / MASS_QT;
        for (int qt0 = 0; qt0 < nqt; qt0 += 2) {                                              // two query tiles per walk over the keys
            bf16x8 qf[2][2];
            float off2[2], wq[2], sum[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int qi = (qt0 + t) * MASS_QT + l15;
                const bool qlive = qi < p.sq;
                const int qc = qlive ? qi : p.sq - 1;
                const char *qrow = qbase + (long long)qc * p.q_ss * 2;
                qf[t][0] = *(const bf16x8 *)qrow;
                qf[t][1] = *(const bf16x8 *)(qrow + 64);
                // the row offset folded once: (m + ln l) log2 e = m log2 e + log2 l
                off2[t] = fmaf(p.m[stat0 + qc], L2E, __builtin_amdgcn_logf(p.l[stat0 + qc]));
                const bool counted = qlive && p.ids_q[(long long)b * p.sq + qc] != 0;
                wq[t] = !counted ? 0.f : (p.w ? p.w[(long long)b * p.sq + qc] : 1.f);
                sum[t] = 0.f;
            }
            const bool two = (qt0 + 1) * MASS_QT < p.sq;                                      // wave-uniform: the second tile exists
            auto load_keys = [&](int kg, bf16x8 (&kf)[2], bool &real, floatx4 &kwv) {
                const int kr = kg * MASS_KG + l15;
                const int key = lo_key + (kr < nkeys ? kr : nkeys - 1);                       // past the segment: re-read its last key, zeroed below
                const char *krow = kbase + (long long)key * p.k_ss * 2;
                kf[0] = *(const bf16x8 *)krow;
                kf[1] = *(const bf16x8 *)(krow + 64);
                real = p.ids_k[krow0 + key] != 0;
                if constexpr (KW) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {                                             // the 4 keys this lane holds in the C layout
                        const int kc = kg * MASS_KG + 4 * grp + r;
                        kwv[r] = kwbase[kc < nkeys ? kc : nkeys - 1];                         // clamped like the key row: inside the segment
                    }
                }
            };
            bf16x8 kf[2], kf_next[2];
            bool real, real_next;
            floatx4 kwv = {0.f, 0.f, 0.f, 0.f}, kwv_next = {0.f, 0.f, 0.f, 0.f};
            load_keys(wave, kf, real, kwv);
            for (int kg = wave; kg < ngroups; kg += MASS_WAVES) {
                const bool more = kg + MASS_WAVES < ngroups;
                if (more) load_keys(kg + MASS_WAVES, kf_next, real_next, kwv_next);           // the next group's rows are in flight under this one's MFMAs
                const uint32_t km = (uint32_t)__builtin_amdgcn_ballot_w64(real) & 0xffffu;   // lanes 0..15 hold keys 0..15 of the group
                const int left = nkeys - kg * MASS_KG;                                        // keys of the group inside the segment (>= 1)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    if (t == 1 && !two) break;
                    const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
                    floatx4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[0], qf[t][0], zero, 0, 0, 0);
                    s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[1], qf[t][1], s, 0, 0, 0);
                    float part = 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int kl = 4 * grp + r;
                        const float s2 = ((km >> kl) & 1u) ? s[r] * sc2 : MASKED2;            // a masked score is REPLACED
                        const float pr = __builtin_amdgcn_exp2f(s2 - off2[t]);
                        if constexpr (KW) part += kl < left ? pr * kwv[r] : 0.f;              // select: kw past the segment is never used
                        else part += kl < left ? pr : 0.f;
                    }
                    sum[t] += part;
                }
                if (more) { kf[0] = kf_next[0]; kf[1] = kf_next[1]; real = real_next; if constexpr (KW) kwv = kwv_next; }
            }
            // select, not multiply: the statistics of a padded or absent query may hold anything
            total += wq[0] != 0.f ? wq[0] * sum[0] : 0.f;
            if (two) total += wq[1] != 0.f ? wq[1] * sum[1] : 0.f;
        }
    }
    // 64 lanes: butterfly (every lane ends with the same bits), then the waves in order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) total += __shfl_xor(total, d, 64);
    if (lane == 0) wave_sum[wave] = total;
    __syncthreads();
    if (tid == 0) {
        float r = wave_sum[0];
#pragma unroll
        for (int wv = 1; wv < MASS_WAVES; ++wv) r += wave_sum[wv];
        float *out = p.mass + ((long long)b * p.heads + n) * p.n_seg + g;
        *out = p.accumulate ? *out + r : r;
    }
}

#define NORM_THREADS 256

__global__ void __launch_bounds__(NORM_THREADS) head_row_norms_kernel(const char *x, long long x_sb, long long x_ss, long long x_sn, float *norm,
                                                                      long long ld, int sk, int heads, long long items)
{
    const long long t = (long long)blockIdx.x * NORM_THREADS + threadIdx.x;
    const long long item = t >> 3;                                  // (row, head), heads fastest; its 8 lanes are one aligned group of the wave
    if (item >= items) return;
    const int sub = (int)(t & 7);
    const int h = (int)(item % heads);
    const long long r = item / heads;
    const long long bi = r / sk, si = r - bi * sk;
    const bf16x8 v = *(const bf16x8 *)(x + (bi * x_sb + si * x_ss + (long long)h * x_sn) * 2 + sub * 16);
    float acc = (float)v[0] * (float)v[0];
#pragma unroll
    for (int d = 1; d < 8; ++d) { const float f = (float)v[d]; acc += f * f; }
#pragma unroll
    for (int d = 1; d <= 4; d <<= 1) acc += __shfl_xor(acc, d, 64);
    if (sub == 0) norm[(long long)h * ld + r] = sqrtf(acc);
}

} // namespace

static int launch_key_mass(const void *q, int64_t q_sb, int64_t q_ss, int64_t q_sn, const void *k, int64_t k_sb, int64_t k_ss, int64_t k_sn,
                           const int64_t *ids_q, const int64_t *ids_k, const int32_t *cu_k, const float *m, const float *l, const int32_t *seg,
                           const float *w, const float *kw, int64_t kw_ld, bool weighted, float *mass, int batch, int heads, int sq, int max_sk,
                           int n_seg, int head_dim, float scale, int accumulate, void *stream)
{
    if (!q || !k || !ids_q || !ids_k || !m || !l || !seg || !mass || batch < 1 || heads < 1 || sq < 1 || n_seg < 1) return -1;
    if (weighted && (!kw || ((uintptr_t)kw & 3))) return -1;
    if (head_dim != 64 || sq > QBLOCK || max_sk < 1 || max_sk > 65536 || (!cu_k && (max_sk & 31))) return -4;
    if ((q_sb | q_ss | q_sn | k_sb | k_ss | k_sn) & 7) return -4;
    if (((uintptr_t)q | (uintptr_t)k) & 15) return -1;
    if ((long long)batch * heads * n_seg > 0x7fffffffLL) return -4;
    if (weighted && (kw_ld < 1 || (!cu_k && kw_ld < (long long)batch * max_sk))) return -4;   // dense: the table holds every key row
    MassParams p;
    p.q = (const char *)q; p.k = (const char *)k; p.ids_q = (const long long *)ids_q; p.ids_k = (const long long *)ids_k;
    p.q_sb = q_sb; p.q_ss = q_ss; p.q_sn = q_sn; p.k_sb = k_sb; p.k_ss = k_ss; p.k_sn = k_sn;
    p.cu_k = cu_k; p.seg = seg; p.m = m; p.l = l; p.w = w; p.kw = weighted ? kw : nullptr; p.kw_ld = weighted ? kw_ld : 0; p.mass = mass;
    p.batch = batch; p.heads = heads; p.sq = sq; p.sk = max_sk; p.n_seg = n_seg; p.accumulate = accumulate; p.scale = scale;
    const dim3 grid((unsigned)(batch * heads * n_seg)), block(MASS_WAVES * 64);
    if (weighted) hipLaunchKernelGGL(attention_key_mass_kernel<true>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(attention_key_mass_kernel<false>, grid, block, 0, (hipStream_t)stream, p);
    return LAUNCH_OK();
}

extern "C" int emdr2_attention_key_mass(const void *q, int64_t q_sb, int64_t q_ss, int64_t q_sn, const void *k, int64_t k_sb, int64_t k_ss, int64_t k_sn,
                                        const int64_t *ids_q, const int64_t *ids_k, const int32_t *cu_k, const float *m, const float *l,
                                        const int32_t *seg, const float *w, float *mass, int batch, int heads, int sq, int max_sk, int n_seg,
                                        int head_dim, float scale, int accumulate, void *stream)
{
    return launch_key_mass(q, q_sb, q_ss, q_sn, k, k_sb, k_ss, k_sn, ids_q, ids_k, cu_k, m, l, seg, w, nullptr, 0, false, mass, batch, heads, sq,
                           max_sk, n_seg, head_dim, scale, accumulate, stream);
}

extern "C" int emdr2_attention_key_mass_weighted(const void *q, int64_t q_sb, int64_t q_ss, int64_t q_sn, const void *k, int64_t k_sb, int64_t k_ss,
                                                 int64_t k_sn, const int64_t *ids_q, const int64_t *ids_k, const int32_t *cu_k, const float *m,
                                                 const float *l, const int32_t *seg, const float *w, const float *kw, int64_t kw_ld, float *mass,
                                                 int batch, int heads, int sq, int max_sk, int n_seg, int head_dim, float scale, int accumulate,
                                                 void *stream)
{
    return launch_key_mass(q, q_sb, q_ss, q_sn, k, k_sb, k_ss, k_sn, ids_q, ids_k, cu_k, m, l, seg, w, kw, kw_ld, true, mass, batch, heads, sq,
                           max_sk, n_seg, head_dim, scale, accumulate, stream);
}

extern "C" int emdr2_head_row_norms(const void *x, int64_t x_sb, int64_t x_ss, int64_t x_sn, float *norm, int64_t ld, int batch, int sk, int heads,
                                    int head_dim, void *stream)
{
    if (!x || !norm || batch < 1 || sk < 1 || heads < 1) return -1;
    if (((uintptr_t)x & 15) || ((uintptr_t)norm & 3)) return -1;
    if (head_dim != 64) return -4;
    if ((x_sb | x_ss | x_sn) & 7) return -4;
    const long long rows = (long long)batch * sk, items = rows * heads;
    if (ld < rows) return -4;
    const long long blocks = (items * 8 + NORM_THREADS - 1) / NORM_THREADS;
    if (blocks > 0x7fffffffLL) return -4;
    hipLaunchKernelGGL(head_row_norms_kernel, dim3((unsigned)blocks), dim3(NORM_THREADS), 0, (hipStream_t)stream, (const char *)x, (long long)x_sb,
                       (long long)x_ss, (long long)x_sn, norm, (long long)ld, sk, heads, items);
    return LAUNCH_OK();
}
