// emdr2_amd/csrc/softmax.hip -- masked softmax over the last dim of the composed attention path (include/emdr2_ops.h: emdr2_softmax_mask_*).
#include "../../include/emdr2_ops.h"
#include "prims.h"
#include "rng.h"

namespace {

// ---- masked softmax over the last dim (reference fallback path: fused_softmax.py:113-125, mask value -10000 REPLACES the score) --
// masked(b, q, k) = ids_q[b,q] == 0 || ids_k[b,k] == 0 || (causal && k > q)     (mask_creation_utils.py:17-42, pad id 0)
// scores [B, np, sq, sk] bf16 in place -> probs; stats m, l fp32 [B, np, sq] (row max and sum of exp), one wave per row
__global__ void __launch_bounds__(256) softmax_fwd_kernel(uint16_t *s, const long long *ids_q, const long long *ids_k, int np, int sq, int sk,
                                                          int causal, float *mstat, float *lstat, long long rows, float drop_p, uint32_t seed)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int q = (int)(row % sq);
    const long long b = row / ((long long)sq * np);
    const bool qpad = ids_q[b * sq + q] == 0;
    uint16_t *sr = s + row * sk;
    const long long *kid = ids_k + b * sk;
    float m = -3.0e38f;
    for (int k = lane; k < sk; k += 64) {
        const bool masked = qpad || kid[k] == 0 || (causal && k > q);
        m = fmaxf(m, masked ? -10000.f : bf2f(sr[k]));
    }
    m = wave_max(m);
    float l = 0.f;
    for (int k = lane; k < sk; k += 64) {
        const bool masked = qpad || kid[k] == 0 || (causal && k > q);
        l += __expf((masked ? -10000.f : bf2f(sr[k])) - m);
    }
    l = wave_sum(l);
    const float inv = 1.f / l;
    for (int k = lane; k < sk; k += 64) {
        const bool masked = qpad || kid[k] == 0 || (causal && k > q);
        float pv = __expf((masked ? -10000.f : bf2f(sr[k])) - m) * inv;
        if (drop_p > 0.f) pv = emdr2_keep(emdr2_row_hash(seed, (unsigned long long)row), (uint32_t)k, emdr2_drop_thr(drop_p)) ? pv * emdr2_keep_scale(drop_p) : 0.f;
        sr[k] = f2bf(pv);
    }
    if (lane == 0 && mstat) { mstat[row] = m; lstat[row] = l; }
}

// register-resident variants (sk % 8 == 0, sk <= 2048): one HBM read + one write per element, 16-byte accesses
template <int NV>
__global__ void __launch_bounds__(256) softmax_fwd_reg_kernel(uint16_t *s, const long long *ids_q, const long long *ids_k, int np, int sq, int sk,
                                                              int causal, float *mstat, float *lstat, long long rows, float drop_p, uint32_t seed)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int q = (int)(row % sq);
    const long long b = row / ((long long)sq * np);
    const bool qpad = ids_q[b * sq + q] == 0;
    uint16_t *sr = s + row * sk;
    const long long *kid = ids_k + b * sk;
    float v[NV][8];
    float m = -3.0e38f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int k0 = (i * 64 + lane) * 8;
        if (k0 < sk) {
            const uint4 x = *(const uint4 *)(sr + k0);
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + j;
                const bool masked = qpad || kid[k] == 0 || (causal && k > q);
                v[i][j] = masked ? -10000.f : bf2f((uint16_t)((j & 1) ? w[j >> 1] >> 16 : w[j >> 1] & 0xffff));
                m = fmaxf(m, v[i][j]);
            }
        }
    }
    m = wave_max(m);
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if ((i * 64 + lane) * 8 < sk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { v[i][j] = __expf(v[i][j] - m); l += v[i][j]; }
        }
    l = wave_sum(l);
    const float inv = 1.f / l;
    const float ik = drop_p > 0.f ? emdr2_keep_scale(drop_p) : 1.f;
    const uint32_t rh = emdr2_row_hash(seed, (unsigned long long)row), thr = emdr2_drop_thr(drop_p);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int k0 = (i * 64 + lane) * 8;
        if (k0 < sk) {
            uint32_t w[4];
            if (drop_p > 0.f) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[i][j] = emdr2_keep(rh, (uint32_t)(k0 + j), thr) ? v[i][j] * ik : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = (uint32_t)f2bf(v[i][2 * j] * inv) | ((uint32_t)f2bf(v[i][2 * j + 1] * inv) << 16);
            *(uint4 *)(sr + k0) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    if (lane == 0 && mstat) { mstat[row] = m; lstat[row] = l; }
}

template <int NV>
__global__ void __launch_bounds__(256) softmax_bwd_reg_kernel(const uint16_t *p, uint16_t *dp, const long long *ids_q, const long long *ids_k, int np,
                                                              int sq, int sk, int causal, float *dstat, long long rows, const float *mstat,
                                                              const float *lstat, float drop_p, uint32_t seed)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int q = (int)(row % sq);
    const long long b = row / ((long long)sq * np);
    const bool qpad = ids_q[b * sq + q] == 0;
    const long long *kid = ids_k + b * sk;
    const uint16_t *pr = p + row * sk;
    uint16_t *dr = dp + row * sk;
    float pv[NV][8], gv[NV][8];
    float d = 0.f;
    const float ms = mstat ? mstat[row] : 0.f, il = mstat ? 1.f / lstat[row] : 1.f;
    const float ik = drop_p > 0.f ? emdr2_keep_scale(drop_p) : 1.f;
    const uint32_t rh = emdr2_row_hash(seed, (unsigned long long)row), thr = emdr2_drop_thr(drop_p);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int k0 = (i * 64 + lane) * 8;
        if (k0 < sk) {
            const uint4 a = *(const uint4 *)(pr + k0), g = *(const uint4 *)(dr + k0);
            const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, gw[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                pv[i][j] = bf2f((uint16_t)((j & 1) ? aw[j >> 1] >> 16 : aw[j >> 1] & 0xffff));
                gv[i][j] = bf2f((uint16_t)((j & 1) ? gw[j >> 1] >> 16 : gw[j >> 1] & 0xffff));
                if (mstat) {                                             // p holds raw scaled scores: rebuild the probability from the row statistics
                    const int k = k0 + j;
                    const bool masked = qpad || kid[k] == 0 || (causal && k > q);
                    pv[i][j] = __expf((masked ? -10000.f : pv[i][j]) - ms) * il;
                }
                if (drop_p > 0.f) gv[i][j] = emdr2_keep(rh, (uint32_t)(k0 + j), thr) ? gv[i][j] * ik : 0.f;
                d += pv[i][j] * gv[i][j];
            }
        }
    }
    d = wave_sum(d);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int k0 = (i * 64 + lane) * 8;
        if (k0 < sk) {
            uint32_t w[4];
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + j;
                const bool masked = qpad || kid[k] == 0 || (causal && k > q);
                o[j] = masked ? 0.f : pv[i][j] * (gv[i][j] - d);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = (uint32_t)f2bf(o[2 * j]) | ((uint32_t)f2bf(o[2 * j + 1]) << 16);
            *(uint4 *)(dr + k0) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    if (lane == 0 && dstat) dstat[row] = d;
}

// dS = P * (dP - sum_k P*dP), in place on dP; masked positions get the same formula (their P is ~0 unless the row is fully
// masked, where the reference's autograd also flows a uniform-softmax gradient into the replaced (constant) scores: those
// are zeroed because masked_fill breaks the dependence on the score).  D[row] is also written.
__global__ void __launch_bounds__(256) softmax_bwd_kernel(const uint16_t *p, uint16_t *dp, const long long *ids_q, const long long *ids_k,
                                                          int np, int sq, int sk, int causal, float *dstat, long long rows, const float *mstat,
                                                          const float *lstat, float drop_p, uint32_t seed)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int q = (int)(row % sq);
    const long long b = row / ((long long)sq * np);
    const bool qpad = ids_q[b * sq + q] == 0;
    const long long *kid = ids_k + b * sk;
    const uint16_t *pr = p + row * sk;
    uint16_t *dr = dp + row * sk;
    float d = 0.f;
    const float ms = mstat ? mstat[row] : 0.f, il = mstat ? 1.f / lstat[row] : 1.f;
    const float ik = drop_p > 0.f ? emdr2_keep_scale(drop_p) : 1.f;
    const uint32_t rh = emdr2_row_hash(seed, (unsigned long long)row), thr = emdr2_drop_thr(drop_p);
    auto prob = [&](int k, bool masked) { return mstat ? __expf((masked ? -10000.f : bf2f(pr[k])) - ms) * il : bf2f(pr[k]); };
    auto grad = [&](int k) { const float g = bf2f(dr[k]); return drop_p > 0.f ? (emdr2_keep(rh, (uint32_t)k, thr) ? g * ik : 0.f) : g; };
    for (int k = lane; k < sk; k += 64) d += prob(k, qpad || kid[k] == 0 || (causal && k > q)) * grad(k);
    d = wave_sum(d);
    for (int k = lane; k < sk; k += 64) {
        const bool masked = qpad || kid[k] == 0 || (causal && k > q);
        dr[k] = masked ? (uint16_t)0 : f2bf(prob(k, masked) * (grad(k) - d));
    }
    if (lane == 0 && dstat) dstat[row] = d;
}

// transposed twin used by the attention backward: from raw scaled scores S^T [B, np, sk, sq] and dP^T, with the forward's
// row statistics m, l and D (all indexed [B, np, sq]): P^T = exp(s - m[q]) / l[q] (masked: exp(-10000 - m[q]) / l[q]),
// dS^T = masked ? 0 : P^T * (dP^T - D[q]).  Writes P^T over S^T and dS^T over dP^T.  Elementwise, 8 elements per thread.
__global__ void __launch_bounds__(256) softmax_t_kernel(uint16_t *st, uint16_t *dpt, const long long *ids_q, const long long *ids_k,
                                                        const float *mstat, const float *lstat, const float *dstat, int np, int sq,
                                                        int sk, int causal, long long total, float drop_p, uint32_t seed)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int q = (int)(i % sq);
    const long long rk = i / sq;             // (b, n, k)
    const int k = (int)(rk % sk);
    const long long bn = rk / sk;
    const long long b = bn / np;
    const long long srow = bn * sq + q;      // stats index
    const bool masked = ids_q[b * sq + q] == 0 || ids_k[b * sk + k] == 0 || (causal && k > q);
    const float pt = __expf((masked ? -10000.f : bf2f(st[i])) - mstat[srow]) / lstat[srow];
    float g = bf2f(dpt[i]), pd = pt;
    if (drop_p > 0.f) {
        const bool keep = emdr2_keep(emdr2_row_hash(seed, (unsigned long long)srow), (uint32_t)k, emdr2_drop_thr(drop_p));
        const float ik = emdr2_keep_scale(drop_p);
        g = keep ? g * ik : 0.f;
        pd = keep ? pt * ik : 0.f;                                        // dropped probabilities (what multiplied V in the forward) for dV
    }
    st[i] = f2bf(pd);
    dpt[i] = masked ? (uint16_t)0 : f2bf(pt * (g - dstat[srow]));
}

} // namespace

// which row kernel a launch takes: the register-resident ones want 16-byte granules (sk % 8 == 0, aligned rows) and hold at most 512 (one
// granule per lane) or 2048 (four) keys; everything else goes to the generic kernel
enum SoftmaxPath { SOFTMAX_REG1 = 0, SOFTMAX_REG4 = 1, SOFTMAX_GENERIC = 2 };
static SoftmaxPath softmax_path(int sk, bool aligned)
{
    if ((sk & 7) || sk > 2048 || !aligned) return SOFTMAX_GENERIC;
    return sk <= 512 ? SOFTMAX_REG1 : SOFTMAX_REG4;
}
static dim3 softmax_grid(long long rows) { return dim3((unsigned)((rows + 3) / 4)); }          // one wave per row

extern "C" int emdr2_softmax_mask_fwd(void *scores, const int64_t *ids_q, const int64_t *ids_k, int batch, int heads, int sq, int sk, int causal,
                                      float *m, float *l, float drop_p, uint32_t seed, void *stream)
{
    if (drop_p < 0.f || drop_p >= 1.f) return -1;
    if (!scores || !ids_q || !ids_k || batch < 1 || heads < 1 || sq < 1 || sk < 1) return -1;
    static const decltype(&softmax_fwd_kernel) kernels[] = {softmax_fwd_reg_kernel<1>, softmax_fwd_reg_kernel<4>, softmax_fwd_kernel};      // by SoftmaxPath
    const long long rows = (long long)batch * heads * sq;
    launch(kernels[softmax_path(sk, !((uintptr_t)scores & 15))], softmax_grid(rows), 256, stream, scores, ids_q, ids_k, heads, sq, sk, causal, m, l,
           rows, drop_p, seed);
    return LAUNCH_OK();
}

extern "C" int emdr2_softmax_mask_bwd(const void *probs, void *dprobs, const int64_t *ids_q, const int64_t *ids_k, const float *m, const float *l,
                                      int batch, int heads, int sq, int sk, int causal, float drop_p, uint32_t seed, float *d, void *stream)
{
    if (drop_p < 0.f || drop_p >= 1.f || (m && !l) || (drop_p > 0.f && !m)) return -1;
    if (!probs || !dprobs || !ids_q || !ids_k || batch < 1 || heads < 1 || sq < 1 || sk < 1) return -1;
    static const decltype(&softmax_bwd_kernel) kernels[] = {softmax_bwd_reg_kernel<1>, softmax_bwd_reg_kernel<4>, softmax_bwd_kernel};      // by SoftmaxPath
    const long long rows = (long long)batch * heads * sq;
    launch(kernels[softmax_path(sk, !(((uintptr_t)probs | (uintptr_t)dprobs) & 15))], softmax_grid(rows), 256, stream, probs, dprobs, ids_q, ids_k,
           heads, sq, sk, causal, d, rows, m, l, drop_p, seed);
    return LAUNCH_OK();
}

extern "C" int emdr2_softmax_mask_t(void *scores_t, void *dprobs_t, const int64_t *ids_q, const int64_t *ids_k, const float *m, const float *l,
                                    const float *d, int batch, int heads, int sq, int sk, int causal, float drop_p, uint32_t seed, void *stream)
{
    if (drop_p < 0.f || drop_p >= 1.f) return -1;
    if (!scores_t || !dprobs_t || !ids_q || !ids_k || !m || !l || !d || batch < 1 || heads < 1 || sq < 1 || sk < 1) return -1;
    const long long total = (long long)batch * heads * sq * sk;
    launch(softmax_t_kernel, dim3((unsigned)((total + 255) / 256)), 256, stream, scores_t, dprobs_t, ids_q, ids_k, m, l, d, heads, sq, sk, causal, total,
           drop_p, seed);
    return LAUNCH_OK();
}
