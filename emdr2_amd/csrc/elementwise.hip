// emdr2_amd/csrc/elementwise.hip -- the elementwise kernels around the GEMMs: transpose, GELU backward, dropout (include/emdr2_ops.h).  The
// row kernels have files of their own: layernorm.hip, softmax.hip, embedding.hip, loss_tail.hip, optimizer.hip.
#include "../../include/emdr2_ops.h"
#include "prims.h"
#include "rng.h"

namespace {

// 64 x 64 tiles through LDS (+1 padding), 256 threads: coalesced 128-B rows in, 128-B rows out
__global__ void __launch_bounds__(256) transpose_kernel(const uint16_t *in, long long ld_in, uint16_t *out, long long ld_out, int rows,
                                                        int cols, int batch2, long long sI1, long long sO1, long long sI2, long long sO2,
                                                        float *colsum)
{
    __shared__ uint16_t tile[64][66];
    const int b1 = blockIdx.z / batch2, b2 = blockIdx.z % batch2;
    in += b1 * sI1 + b2 * sI2;
    out += b1 * sO1 + b2 * sO2;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    float cs = 0.f;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        uint16_t v = 0;
        if (r < rows && c < cols) v = in[(long long)r * ld_in + c];
        tile[i][tx] = v;
        cs += bf2f(v);
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows) out[(long long)c * ld_out + r] = tile[tx][i];
    }
    if (colsum) {
        __shared__ float part[4][64];
        part[ty][tx] = cs;
        __syncthreads();
        if (ty == 0 && c0 + tx < cols) atomicAdd(&colsum[c0 + tx], part[0][tx] + part[1][tx] + part[2][tx] + part[3][tx]);
    }
}

// ---- GELU backward on the saved pre-activation (exact erf form; transformer.py:80,103-104) -------------------------------
__global__ void __launch_bounds__(256) gelu_bwd_kernel(const uint16_t *pre, const uint16_t *dact, uint16_t *dpre, long long n)
{
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= n) return;
    const uint4 a = *(const uint4 *)(pre + i), g = *(const uint4 *)(dact + i);
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, gw[4] = {g.x, g.y, g.z, g.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float r[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float u = bf2f((uint16_t)(h ? aw[j] >> 16 : aw[j] & 0xffff)), d = bf2f((uint16_t)(h ? gw[j] >> 16 : gw[j] & 0xffff));
            const float cdf = 0.5f * (1.f + erff(u * 0.70710678118654752f));
            r[h] = d * (cdf + u * 0.3989422804014327f * __expf(-0.5f * u * u));
        }
        o[j] = (uint32_t)f2bf(r[0]) | ((uint32_t)f2bf(r[1]) << 16);
    }
    *(uint4 *)(dpre + i) = make_uint4(o[0], o[1], o[2], o[3]);
}

// ---- dropout mask of a site re-applied to a contiguous bf16 tensor (backward of the fused bias-dropout-add epilogue) --------------
__global__ void __launch_bounds__(256) dropout_kernel(const uint16_t *x, uint16_t *out, long long n, int cols, float drop_p, uint32_t seed)
{
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;     // cols % 8 == 0: the 8 elements share a row
    if (i >= n) return;
    const float ik = emdr2_keep_scale(drop_p);
    const uint32_t thr = emdr2_drop_thr(drop_p), rh = emdr2_row_hash(seed, (unsigned long long)(i / cols)), c0 = (uint32_t)(i % cols);
    const uint4 a = *(const uint4 *)(x + i);
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w};
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t b = emdr2_pair_bits(rh, c0 + 2 * j);
        const float lo = (b & 0xffffu) >= thr ? bf2f((uint16_t)(aw[j] & 0xffff)) * ik : 0.f;
        const float hi = (b >> 16) >= thr ? bf2f((uint16_t)(aw[j] >> 16)) * ik : 0.f;
        w[j] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
    }
    *(uint4 *)(out + i) = make_uint4(w[0], w[1], w[2], w[3]);
}

} // namespace

extern "C" int emdr2_transpose_bf16(const void *in, int64_t ld_in, void *out, int64_t ld_out, int rows, int cols, int batch1,
                                    int64_t sI1, int64_t sO1, int batch2, int64_t sI2, int64_t sO2, float *colsum, void *stream)
{
    if (!in || !out || rows < 1 || cols < 1 || batch1 < 1 || batch2 < 1) return -1;
    launch(transpose_kernel, dim3((cols + 63) / 64, (rows + 63) / 64, batch1 * batch2), 256, stream, in, ld_in, out, ld_out, rows, cols, batch2, sI1, sO1, sI2,
           sO2, colsum);
    return LAUNCH_OK();
}

extern "C" int emdr2_gelu_bwd(const void *pre, const void *dact, void *dpre, int64_t n, void *stream)
{
    if (!pre || !dact || !dpre || n < 8 || (n & 7)) return -1;
    launch(gelu_bwd_kernel, dim3((unsigned)((n / 8 + 255) / 256)), 256, stream, pre, dact, dpre, n);
    return LAUNCH_OK();
}

extern "C" int emdr2_dropout(const void *x, void *out, int64_t n, int cols, float drop_p, uint32_t seed, void *stream)
{
    if (!x || !out || n < 8 || (n & 7) || cols < 8 || (cols & 7) || n % cols || drop_p <= 0.f || drop_p >= 1.f || ((uintptr_t)x & 15) || ((uintptr_t)out & 15)) return -1;
    launch(dropout_kernel, dim3((unsigned)((n / 8 + 255) / 256)), 256, stream, x, out, n, cols, drop_p, seed);
    return LAUNCH_OK();
}
