// emdr2_amd/csrc/loss_tail.hip -- what follows the LM head and the towers: log-softmax + gather over the vocabulary, the combine of the fused
// head's partials, the retriever prior and the EMDR2 marginal (include/emdr2_ops.h).
#include "../../include/emdr2_ops.h"
#include "prims.h"

namespace {

// ---- log-softmax + gather over the vocabulary (train_e2eqa.py:72-123,152-160) --------------------------------------------------
// gold[row] = logits[row, label[row]] - logsumexp(logits[row, :]),  lse[row] kept for the backward; one block per row
__global__ void __launch_bounds__(256) lse_gather_kernel(const uint16_t *logits, const long long *labels, float *gold, float *lse, int V)
{
    __shared__ float red[4];
    const long long row = blockIdx.x;
    const uint16_t *lr = logits + row * V;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float m = -3.0e38f;
    for (int i = threadIdx.x; i < V; i += 256) m = fmaxf(m, bf2f(lr[i]));
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f;
    for (int i = threadIdx.x; i < V; i += 256) s += __expf(bf2f(lr[i]) - m);
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float l = m + __logf(red[0] + red[1] + red[2] + red[3]);
        lse[row] = l;
        const long long lab = labels[row];                               // outside [0, V) (an ignore_index): gold logit 0, as the fused LM head defines it
        gold[row] = (lab >= 0 && lab < V ? bf2f(lr[lab]) : 0.f) - l;
    }
}

// dlogits[row, v] = w[row] * (onehot(label) - softmax)[v]  where w = d(loss)/d(gold[row])
__global__ void __launch_bounds__(256) lse_gather_bwd_kernel(const uint16_t *logits, const long long *labels, const float *lse, const float *w,
                                                             uint16_t *dlogits, int V)
{
    const long long row = blockIdx.x;
    const float l = lse[row], ww = w[row];
    const long long lab = labels[row];
    for (int i = threadIdx.x; i < V; i += 256) {
        const float sm = __expf(bf2f(logits[row * V + i]) - l);
        dlogits[row * V + i] = f2bf(ww * ((i == lab ? 1.f : 0.f) - sm));
    }
}

} // namespace

// ---- retriever prior (emdr2_model.py:134-145): sim[b, k] = <q[b], c[b, k]> * scale, log-softmax over the K retrieved passages --------------------
// One workgroup per question; K <= 1024 (top-k 50 / 100 + 1 in the shipped scripts).  q bf16, everything else fp32.  prob (= exp(logp)) is
// kept for the backward.  The contexts c are bf16 (the context tower's output) or fp16 (rows of the evidence index, --context-embeddings-from-
// index): both widen exactly to fp32, so the kernels are templates over the context element and the arithmetic is stated once.
#define PRIOR_MAX_K 1024
struct CtxBf16 { static __device__ __forceinline__ float widen(uint16_t h) { return bf2f(h); } };
struct CtxFp16 { static __device__ __forceinline__ float widen(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); } };

template <typename Ctx>
__global__ void __launch_bounds__(256) retriever_prior_fwd_kernel(const uint16_t *q, const uint16_t *c, float *logp, float *prob, int K, int H, float scale)
{
    __shared__ float sim[PRIOR_MAX_K];
    __shared__ float stat[2];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint16_t *qb = q + (long long)b * H;
    for (int k = wave; k < K; k += 4) {
        const uint16_t *ck = c + ((long long)b * K + k) * H;
        float s = 0.f;
        for (int i = lane * 8; i < H; i += 512) {
            const uint4 qa = *(const uint4 *)(qb + i), ca = *(const uint4 *)(ck + i);
            const uint32_t qw[4] = {qa.x, qa.y, qa.z, qa.w}, cw[4] = {ca.x, ca.y, ca.z, ca.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                s += bf2f((uint16_t)(qw[j] & 0xffff)) * Ctx::widen((uint16_t)(cw[j] & 0xffff)) + bf2f((uint16_t)(qw[j] >> 16)) * Ctx::widen((uint16_t)(cw[j] >> 16));
        }
        s = wave_sum(s);
        if (lane == 0) sim[k] = s * scale;
    }
    __syncthreads();
    if (wave == 0) {
        float a = -3.0e38f;
        for (int k = lane; k < K; k += 64) a = fmaxf(a, sim[k]);
        const float m = wave_max(a);
        float e = 0.f;
        for (int k = lane; k < K; k += 64) e += __expf(sim[k] - m);
        const float l = wave_sum(e);
        if (lane == 0) { stat[0] = m; stat[1] = __logf(l); }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        const float lp = sim[k] - stat[0] - stat[1];
        logp[(long long)b * K + k] = lp;
        prob[(long long)b * K + k] = __expf(lp);
    }
}

// d sim[k] = (g[k] - prob[k] * sum_j g[j]) * scale;  dq[h] = sum_k dsim[k] c[k, h];  dc[k, h] = dsim[k] q[h]   (bf16 gradients out)
template <typename Ctx>
__global__ void __launch_bounds__(256) retriever_prior_bwd_kernel(const float *g, const float *prob, const uint16_t *q, const uint16_t *c, uint16_t *dq,
                                                                  uint16_t *dc, int K, int H, float scale)
{
    __shared__ float dsim[PRIOR_MAX_K];
    __shared__ float gsum;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *gb = g + (long long)b * K, *pb = prob + (long long)b * K;
    if (wave == 0) {
        float t = 0.f;
        for (int k = lane; k < K; k += 64) t += gb[k];
        t = wave_sum(t);
        if (lane == 0) gsum = t;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) dsim[k] = (gb[k] - pb[k] * gsum) * scale;
    __syncthreads();
    const uint16_t *qb = q + (long long)b * H, *cb = c + (long long)b * K * H;
    for (int h = threadIdx.x; h < H; h += 256) {
        float acc = 0.f;
        const float qh = bf2f(qb[h]);
        for (int k = 0; k < K; ++k) {
            acc += dsim[k] * Ctx::widen(cb[(long long)k * H + h]);
            if (dc) dc[((long long)b * K + k) * H + h] = f2bf(dsim[k] * qh);
        }
        if (dq) dq[(long long)b * H + h] = f2bf(acc);
    }
}

// ---- EMDR2 marginal (train_e2eqa.py:98-123): marginal[b, l] = logsumexp_k( prior[b, k] + gold[b, k, l] ) -------------------------------------------
__global__ void __launch_bounds__(64) marginal_fwd_kernel(const float *prior, const float *gold, float *marginal, int K, int L)
{
    const int b = blockIdx.x;
    for (int l = threadIdx.x; l < L; l += 64) {
        float m = -3.0e38f;
        for (int k = 0; k < K; ++k) m = fmaxf(m, prior[(long long)b * K + k] + gold[((long long)b * K + k) * L + l]);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += __expf(prior[(long long)b * K + k] + gold[((long long)b * K + k) * L + l] - m);
        marginal[(long long)b * L + l] = m + __logf(s);
    }
}

// d prior[b, k] = sum_l gm[b, l] * exp(prior[b, k] + gold[b, k, l] - marginal[b, l])      (gold is a constant of the loss: no-grad pass)
__global__ void __launch_bounds__(128) marginal_bwd_kernel(const float *prior, const float *gold, const float *marginal, const float *gm, float *dprior,
                                                           int K, int L)
{
    const int b = blockIdx.x;
    for (int k = threadIdx.x; k < K; k += 128) {
        const float pk = prior[(long long)b * K + k];
        float acc = 0.f;
        for (int l = 0; l < L; ++l) acc += gm[(long long)b * L + l] * __expf(pk + gold[((long long)b * K + k) * L + l] - marginal[(long long)b * L + l]);
        dprior[(long long)b * K + k] = acc;
    }
}

// out[row] = gold[row] - logsumexp over the row's partials (max_j, sum_j exp(x - max_j)) written by emdr2_gemm_nt_lse_bf16: one wave per row
__global__ void __launch_bounds__(256) lse_combine_kernel(const float *pmax, const float *psum, const float *gold, float *out, float *lse,
                                                           long long rows, int slots)
{
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float *pm = pmax + row * slots, *ps = psum + row * slots;
    float m = -3.0e38f;
    for (int i = lane; i < slots; i += 64) m = fmaxf(m, pm[i]);
    m = wave_max(m);
    float s = 0.f;
    for (int i = lane; i < slots; i += 64) s += ps[i] * __expf(pm[i] - m);
    s = wave_sum(s);
    if (lane == 0) {
        const float l = m + __logf(s);
        if (lse) lse[row] = l;
        out[row] = gold[row] - l;
    }
}

template <typename Ctx>
static int prior_fwd(const void *q, const void *c, float *logp, float *prob, int batch, int K, int H, float scale, void *stream)
{
    if (!q || !c || !logp || !prob || batch < 1 || K < 1 || H < 8 || (H & 7) || ((uintptr_t)q & 15) || ((uintptr_t)c & 15)) return -1;
    if (K > PRIOR_MAX_K) return -4;
    launch(retriever_prior_fwd_kernel<Ctx>, dim3(batch), 256, stream, q, c, logp, prob, K, H, scale);
    return LAUNCH_OK();
}

template <typename Ctx>
static int prior_bwd(const float *dlogp, const float *prob, const void *q, const void *c, void *dq, void *dc, int batch, int K, int H, float scale,
                     void *stream)
{
    launch(retriever_prior_bwd_kernel<Ctx>, dim3(batch), 256, stream, dlogp, prob, q, c, dq, dc, K, H, scale);
    return LAUNCH_OK();
}

extern "C" int emdr2_retriever_prior_fwd(const void *q, const void *c, float *logp, float *prob, int batch, int K, int H, float scale, void *stream)
{
    return prior_fwd<CtxBf16>(q, c, logp, prob, batch, K, H, scale, stream);
}

extern "C" int emdr2_retriever_prior_bwd(const float *dlogp, const float *prob, const void *q, const void *c, void *dq, void *dc, int batch, int K, int H,
                                         float scale, void *stream)
{
    if (!dlogp || !prob || !q || !c || (!dq && !dc) || batch < 1 || K < 1 || H < 8) return -1;
    if (K > PRIOR_MAX_K) return -4;
    return prior_bwd<CtxBf16>(dlogp, prob, q, c, dq, dc, batch, K, H, scale, stream);
}

// fp16 contexts (rows gathered from the evidence index): the same kernels, the same checks as the forward above for both directions.  The
// contexts are constants of the step, so the backward has no dc.
extern "C" int emdr2_retriever_prior_h16_fwd(const void *q, const void *c, float *logp, float *prob, int batch, int K, int H, float scale, void *stream)
{
    return prior_fwd<CtxFp16>(q, c, logp, prob, batch, K, H, scale, stream);
}

extern "C" int emdr2_retriever_prior_h16_bwd(const float *dlogp, const float *prob, const void *q, const void *c, void *dq, int batch, int K, int H,
                                             float scale, void *stream)
{
    if (!dlogp || !prob || !q || !c || !dq || batch < 1 || K < 1 || H < 8 || (H & 7) || ((uintptr_t)q & 15) || ((uintptr_t)c & 15)) return -1;
    if (K > PRIOR_MAX_K) return -4;
    return prior_bwd<CtxFp16>(dlogp, prob, q, c, dq, nullptr, batch, K, H, scale, stream);
}

extern "C" int emdr2_marginal_fwd(const float *prior, const float *gold, float *marginal, int batch, int K, int L, void *stream)
{
    if (!prior || !gold || !marginal || batch < 1 || K < 1 || L < 1) return -1;
    launch(marginal_fwd_kernel, dim3(batch), 64, stream, prior, gold, marginal, K, L);
    return LAUNCH_OK();
}

extern "C" int emdr2_marginal_bwd(const float *prior, const float *gold, const float *marginal, const float *dmarginal, float *dprior, int batch, int K,
                                  int L, void *stream)
{
    if (!prior || !gold || !marginal || !dmarginal || !dprior || batch < 1 || K < 1 || L < 1) return -1;
    launch(marginal_bwd_kernel, dim3(batch), 128, stream, prior, gold, marginal, dmarginal, dprior, K, L);
    return LAUNCH_OK();
}

extern "C" int emdr2_lse_combine(const float *part_max, const float *part_sum, const float *gold, float *out, float *lse, int64_t rows, int slots,
                                 void *stream)
{
    if (!part_max || !part_sum || !gold || !out || rows < 1 || slots < 1) return -1;
    launch(lse_combine_kernel, dim3((unsigned)((rows + 3) / 4)), 256, stream, part_max, part_sum, gold, out, lse, rows, slots);
    return LAUNCH_OK();
}

extern "C" int emdr2_lse_gather_fwd(const void *logits, const int64_t *labels, float *gold, float *lse, int64_t rows, int V, void *stream)
{
    if (!logits || !labels || !gold || !lse || rows < 1 || V < 1) return -1;
    launch(lse_gather_kernel, dim3((unsigned)rows), 256, stream, logits, labels, gold, lse, V);
    return LAUNCH_OK();
}

extern "C" int emdr2_lse_gather_bwd(const void *logits, const int64_t *labels, const float *lse, const float *w, void *dlogits, int64_t rows, int V,
                                    void *stream)
{
    if (!logits || !labels || !lse || !w || !dlogits || rows < 1 || V < 1) return -1;
    launch(lse_gather_bwd_kernel, dim3((unsigned)rows), 256, stream, logits, labels, lse, w, dlogits, V);
    return LAUNCH_OK();
}
