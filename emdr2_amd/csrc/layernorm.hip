// emdr2_amd/csrc/layernorm.hip -- LayerNorm forward and backward over bf16 rows (include/emdr2_ops.h: emdr2_layernorm_*).
#include "../../include/emdr2_ops.h"
#include "prims.h"
#include "rng.h"
#include "ordered_sum.h"

namespace {

// ---- LayerNorm (torch.nn.LayerNorm semantics, eps inside the sqrt; mpu/layers.py:28-36) -----------------------
// one wave per row, H % 8 == 0, 16-B vector loads
__global__ void __launch_bounds__(256) layernorm_fwd_kernel(const uint16_t *x, const float *gamma, const float *beta, uint16_t *y,
                                                            float *mean, float *rstd, long long rows, int H, float eps)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint16_t *xr = x + row * H;
    float s = 0.f;
    for (int i = lane * 8; i < H; i += 512) {
        const uint4 v = *(const uint4 *)(xr + i);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) s += bf2f((uint16_t)(w[j] & 0xffff)) + bf2f((uint16_t)(w[j] >> 16));
    }
    s = wave_sum(s);
    const float mu = s / H;
    // centred second pass (the row comes back from cache): E[x^2] - mu^2 in fp32 cancels to nothing on a row whose mean dwarfs its spread
    float ss = 0.f, ss1 = 0.f;                                           // two chains: the even and the odd elements
    for (int i = lane * 8; i < H; i += 512) {
        const uint4 v = *(const uint4 *)(xr + i);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float a = bf2f((uint16_t)(w[j] & 0xffff)) - mu, b = bf2f((uint16_t)(w[j] >> 16)) - mu; ss += a * a; ss1 += b * b; }
    }
    ss = wave_sum(ss + ss1);
    const float var = ss / H;
    const float rs = rsqrtf(var + eps);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
    uint16_t *yr = y + row * H;
    for (int i = lane * 8; i < H; i += 512) {
        const uint4 v = *(const uint4 *)(xr + i);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = (bf2f((uint16_t)(w[j] & 0xffff)) - mu) * rs * gamma[i + 2 * j] + beta[i + 2 * j];
            const float b = (bf2f((uint16_t)(w[j] >> 16)) - mu) * rs * gamma[i + 2 * j + 1] + beta[i + 2 * j + 1];
            o[j] = (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16);
        }
        *(uint4 *)(yr + i) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// H == 768 (every LayerNorm of the base configuration): half a wave per row, the row's 96 16-byte granules held in registers (3 per
// lane, all lanes busy, one HBM read), reductions over 32 lanes, gamma / beta fetched once per lane for both rows of the wave.
__global__ void __launch_bounds__(256) layernorm_fwd768_kernel(const uint16_t *x, const float *gamma, const float *beta, uint16_t *y, float *mean,
                                                               float *rstd, long long rows, float eps)
{
    const int lane = threadIdx.x & 63, l31 = lane & 31;
    const long long row = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + (lane >> 5);
    const bool live = row < rows;
    const uint16_t *xr = x + (live ? row : rows - 1) * 768;
    uint4 v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = ld_stream(xr + (i * 32 + l31) * 8);
    float f[3][8], s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f[i][2 * j] = bf2f((uint16_t)(w[j] & 0xffff)); f[i][2 * j + 1] = bf2f((uint16_t)(w[j] >> 16));
            s += f[i][2 * j] + f[i][2 * j + 1];
        }
    }
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) s += __shfl_xor(s, o);                                  // within the 32 lanes of the row
    // centred second reduction over the registers (no memory traffic): E[x^2] - mu^2 in fp32 cancels to nothing on a row whose mean
    // dwarfs its spread.  mul_rounded: ONE rounded mean for every element -- left to contraction, the compiler folds s * (1 / 768) into the
    // subtraction of some elements (an unrounded mean) and not of others, and the first-order cancellation of the mean's rounding error
    // in sum (x - mu)^2 is gone (rstd 5e-6 off on a row of 256 with one element at 258)
    const float mu = mul_rounded(s, 1.0f / 768.0f);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) { f[i][j] -= mu; ss += f[i][j] * f[i][j]; }
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) ss += __shfl_xor(ss, o);
    const float var = ss * (1.0f / 768.0f);
    const float rs = rsqrtf(var + eps);
    if (live && l31 == 0) { mean[row] = mu; rstd[row] = rs; }
    if (!live) return;
    uint16_t *yr = y + row * 768;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = (i * 32 + l31) * 8;
        const float4 g0 = *(const float4 *)(gamma + c), g1 = *(const float4 *)(gamma + c + 4);
        const float4 b0 = *(const float4 *)(beta + c), b1 = *(const float4 *)(beta + c + 4);
        const float gm[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, bt[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = (uint32_t)f2bf(fmaf(f[i][2 * j] * rs, gm[2 * j], bt[2 * j])) |
                   ((uint32_t)f2bf(fmaf(f[i][2 * j + 1] * rs, gm[2 * j + 1], bt[2 * j + 1])) << 16);
        st_stream(yr + c, make_uint4(o[0], o[1], o[2], o[3]));
    }
}

// dx = rstd * (g - mean(g) - xhat * mean(g*xhat)),  g = dy*gamma ; optional residual-branch gradient added on the way out.
// Block = 32 rows: phase 1 one wave per row computes the two row means into LDS; phase 2 every thread owns columns tid, tid+256, ...
// for all 32 rows (dgamma / dbeta partials stay in registers; one global atomicAdd per column per block).
// ORD (emdr2_layernorm_bwd_ordered): no atomics -- workgroup b stores its 2 x H column partials into slot b of dgamma (a workspace,
// [gridDim.x][2][H], dbeta unused); ordered_slot_sum adds the slots.  dx is the same instruction sequence in both instances.
#define LN_ROWS 32
template <bool ORD>
__global__ void __launch_bounds__(256) layernorm_bwd_kernel(const uint16_t *dy, const uint16_t *x, const float *gamma, const float *mean,
                                                            const float *rstd, const uint16_t *dres, uint16_t *dx, float *dgamma,
                                                            float *dbeta, long long rows, int H, int rows_per_block)
{
    __shared__ float s1s[LN_ROWS], s2s[LN_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * LN_ROWS;
    for (int rr = wave; rr < LN_ROWS; rr += 4) {
        const long long row = r0 + rr;
        float s1 = 0.f, s2 = 0.f;
        if (row < rows) {
            const uint16_t *xr = x + row * H, *gr = dy + row * H;
            const float mu = mean[row], rs = rstd[row];
            for (int i = lane; i < H; i += 64) {
                const float xh = (bf2f(xr[i]) - mu) * rs, g = bf2f(gr[i]) * gamma[i];
                s1 += g; s2 += g * xh;
            }
        }
        s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (lane == 0) { s1s[rr] = s1 / H; s2s[rr] = s2 / H; }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < H; c += 256) {
        const float gm = gamma[c];
        float ag = 0.f, ab = 0.f;
        for (int rr = 0; rr < LN_ROWS; ++rr) {
            const long long row = r0 + rr;
            if (row >= rows) break;
            const float mu = mean[row], rs = rstd[row];
            const float xh = (bf2f(x[row * H + c]) - mu) * rs, d = bf2f(dy[row * H + c]);
            float v = rs * (d * gm - s1s[rr] - xh * s2s[rr]);
            if (dres) v += bf2f(dres[row * H + c]);
            dx[row * H + c] = f2bf(v);
            ag += d * xh; ab += d;
        }
        if (ORD) {
            dgamma[((long long)blockIdx.x * 2) * H + c] = ag;
            dgamma[((long long)blockIdx.x * 2 + 1) * H + c] = ab;
        } else {
            atomicAdd(&dgamma[c], ag);
            atomicAdd(&dbeta[c], ab);
        }
    }
}

// H == 768 backward: half a wave per row with dy and x in registers (one HBM read each), persistent waves accumulate the dgamma / dbeta
// partials of their 24 columns per lane in registers across all their rows; one LDS reduction and one atomicAdd per column per workgroup.
// DMASK: also write dx o keep(seed, row, col) / (1 - p) -- the bias-dropout-add below this LayerNorm wants exactly that tensor as the operand of
// its two backward GEMMs (they read operands by LDS-DMA, so the mask cannot ride in their loads), and r03 made it with a kernel of its own
// (read dx, write the masked copy: 21 ms of the step).  Same bits as that kernel: the mask is applied to the bf16-ROUNDED dx.
// ORD: as in layernorm_bwd_kernel -- slot blockIdx.x of dgamma ([gridDim.x][2][768]) takes the workgroup's column partials.
template <bool DMASK, bool ORD = false>
__global__ void __launch_bounds__(256) layernorm_bwd768_kernel(const uint16_t *dy, const uint16_t *x, const float *gamma, const float *mean,
                                                               const float *rstd, const uint16_t *dres, uint16_t *dx, float *dgamma, float *dbeta,
                                                               long long rows, uint16_t *dmask, float drop_p, uint32_t seed)
{
    __shared__ float red[2][4][768];
    const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5, wave = threadIdx.x >> 6;
    float gm[3][8], ag[3][8], ab[3][8];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = (i * 32 + l31) * 8;
        const float4 g0 = *(const float4 *)(gamma + c), g1 = *(const float4 *)(gamma + c + 4);
        gm[i][0] = g0.x; gm[i][1] = g0.y; gm[i][2] = g0.z; gm[i][3] = g0.w; gm[i][4] = g1.x; gm[i][5] = g1.y; gm[i][6] = g1.z; gm[i][7] = g1.w;
#pragma unroll
        for (int j = 0; j < 8; ++j) { ag[i][j] = 0.f; ab[i][j] = 0.f; }
    }
    const long long npairs = (rows + 1) >> 1, stride = (long long)gridDim.x * 4;
    for (long long rp = (long long)blockIdx.x * 4 + wave; rp < npairs; rp += stride) {
        const long long row = rp * 2 + half;
        if (row >= rows) continue;                                       // only the odd tail row's partner half-wave
        const uint16_t *xr = x + row * 768, *dr = dy + row * 768;
        uint4 xv[3], dv[3], rv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { xv[i] = ld_stream(xr + (i * 32 + l31) * 8); dv[i] = ld_stream(dr + (i * 32 + l31) * 8); }
        if (dres) {
#pragma unroll
            for (int i = 0; i < 3; ++i) rv[i] = ld_stream(dres + row * 768 + (i * 32 + l31) * 8);
        }
        const float mu = mean[row], rs = rstd[row];
        float xh[3][8], g[3][8], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t xw[4] = {xv[i].x, xv[i].y, xv[i].z, xv[i].w}, dw[4] = {dv[i].x, dv[i].y, dv[i].z, dv[i].w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xe = bf2f((uint16_t)((j & 1) ? xw[j >> 1] >> 16 : xw[j >> 1] & 0xffff));
                const float de = bf2f((uint16_t)((j & 1) ? dw[j >> 1] >> 16 : dw[j >> 1] & 0xffff));
                xh[i][j] = (xe - mu) * rs;
                g[i][j] = de * gm[i][j];
                s1 += g[i][j]; s2 += g[i][j] * xh[i][j];
                ag[i][j] += de * xh[i][j]; ab[i][j] += de;
            }
        }
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
        const float m1 = s1 * (1.0f / 768.0f), m2 = s2 * (1.0f / 768.0f);
        uint16_t *xo = dx + row * 768;
        const float ik = DMASK ? emdr2_keep_scale(drop_p) : 1.f;
        const uint32_t thr = DMASK ? emdr2_drop_thr(drop_p) : 0u, rh = DMASK ? emdr2_row_hash(seed, (unsigned long long)row) : 0u;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t rw[4] = {rv[i].x, rv[i].y, rv[i].z, rv[i].w};
            uint32_t o[4], om[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = rs * (g[i][2 * j] - m1 - xh[i][2 * j] * m2), b = rs * (g[i][2 * j + 1] - m1 - xh[i][2 * j + 1] * m2);
                if (dres) { a += bf2f((uint16_t)(rw[j] & 0xffff)); b += bf2f((uint16_t)(rw[j] >> 16)); }
                const uint16_t ha = f2bf(a), hb = f2bf(b);
                o[j] = (uint32_t)ha | ((uint32_t)hb << 16);
                if (DMASK) {
                    const uint32_t bits = emdr2_pair_bits(rh, (uint32_t)((i * 32 + l31) * 8 + 2 * j));
                    const float lo = (bits & 0xffffu) >= thr ? bf2f(ha) * ik : 0.f, hi = (bits >> 16) >= thr ? bf2f(hb) * ik : 0.f;
                    om[j] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
                }
            }
            st_stream(xo + (i * 32 + l31) * 8, make_uint4(o[0], o[1], o[2], o[3]));
            if (DMASK) st_stream(dmask + row * 768 + (i * 32 + l31) * 8, make_uint4(om[0], om[1], om[2], om[3]));
        }
    }
    // both half-waves own the same columns: fold, then reduce the 4 waves through LDS
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float a = ag[i][j] + __shfl_xor(ag[i][j], 32), b = ab[i][j] + __shfl_xor(ab[i][j], 32);
            if (half == 0) { red[0][wave][(i * 32 + l31) * 8 + j] = a; red[1][wave][(i * 32 + l31) * 8 + j] = b; }
        }
    __syncthreads();
    for (int c = threadIdx.x; c < 768; c += 256) {
        const float a = red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c], b = red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c];
        if (ORD) {
            dgamma[(long long)blockIdx.x * 1536 + c] = a;
            dgamma[(long long)blockIdx.x * 1536 + 768 + c] = b;
        } else {
            atomicAdd(&dgamma[c], a);
            atomicAdd(&dbeta[c], b);
        }
    }
}

} // namespace

extern "C" int emdr2_layernorm_fwd(const void *x, const float *gamma, const float *beta, void *y, float *mean, float *rstd, int64_t rows,
                                   int H, float eps, void *stream)
{
    if (!x || !gamma || !beta || !y || !mean || !rstd || rows < 1 || H < 8 || (H & 7)) return -1;
    if (H == 768 && !((uintptr_t)x & 15) && !((uintptr_t)y & 15) && !((uintptr_t)gamma & 15) && !((uintptr_t)beta & 15))
        launch(layernorm_fwd768_kernel, dim3((unsigned)((rows + 7) / 8)), 256, stream, x, gamma, beta, y, mean, rstd, rows, eps);
    else
        launch(layernorm_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), 256, stream, x, gamma, beta, y, mean, rstd, rows, H, eps);
    return LAUNCH_OK();
}

// ---- the backward's one launch description: the three exported entries check their own arguments, fill this in and call ln_bwd_launch ----
struct LnBwd {
    const void *dy, *x; const float *gamma, *mean, *rstd; const void *dres; void *dx;
    float *dgamma, *dbeta;            // ordered: dgamma = the slot workspace [slots][2][H], dbeta = nullptr
    long long rows; int H;
    void *dmask; float drop_p; uint32_t seed;      // dmask nullptr: no masked copy of dx
    bool ordered;
};

// the 768 kernel reads and writes 16-byte granules: every row pointer it touches has to be aligned (nullptr counts as aligned)
static bool ln_bwd_k768(const LnBwd &a)
{
    return a.H == 768 && !(((uintptr_t)a.dy | (uintptr_t)a.x | (uintptr_t)a.dx | (uintptr_t)a.dres | (uintptr_t)a.gamma | (uintptr_t)a.dmask) & 15);
}

// workgroups of the launch = slots of the ordered workspace.  768: persistent, each wave walks ~100 row pairs at the reader's shape, and a
// function of `rows` alone (the ORDER below rests on that); otherwise one workgroup per LN_ROWS rows.
static long long ln_bwd_slots(long long rows, int H, bool k768)
{
    if (!k768) return (rows + LN_ROWS - 1) / LN_ROWS;
    const long long b = (rows + 7) / 8;
    return b > 2048 ? 2048 : b;
}

static void ln_bwd_launch(const LnBwd &a, bool k768, void *stream)
{
    const dim3 grid((unsigned)ln_bwd_slots(a.rows, a.H, k768));
    if (!k768) {
        launch(a.ordered ? layernorm_bwd_kernel<true> : layernorm_bwd_kernel<false>, grid, 256, stream, a.dy, a.x, a.gamma, a.mean, a.rstd, a.dres, a.dx,
               a.dgamma, a.dbeta, a.rows, a.H, LN_ROWS);
        return;
    }
    const auto k = a.dmask ? (a.ordered ? layernorm_bwd768_kernel<true, true> : layernorm_bwd768_kernel<true, false>)
                           : (a.ordered ? layernorm_bwd768_kernel<false, true> : layernorm_bwd768_kernel<false, false>);
    launch(k, grid, 256, stream, a.dy, a.x, a.gamma, a.mean, a.rstd, a.dres, a.dx, a.dgamma, a.dbeta, a.rows, a.dmask, a.drop_p, a.seed);
}

extern "C" int emdr2_layernorm_bwd(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd, const void *dres,
                                   void *dx, float *dgamma, float *dbeta, int64_t rows, int H, void *stream)
{
    if (!dy || !x || !gamma || !mean || !rstd || !dx || !dgamma || !dbeta || rows < 1 || H < 1 || H > 8192) return -1;
    const LnBwd a = {dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, rows, H, nullptr, 0.f, 0u, false};
    ln_bwd_launch(a, ln_bwd_k768(a), stream);
    return LAUNCH_OK();
}

// LayerNorm backward that ALSO writes dmask = dropout_mask(seed) o dx / (1 - p): the operand the bias-dropout-add under this LayerNorm needs for
// its backward GEMMs (emdr2_dropout would make it from dx in a launch of its own).  H == 768 only (-4 otherwise: the caller keeps the two launches).
extern "C" int emdr2_layernorm_bwd_mask(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd, const void *dres, void *dx,
                                        float *dgamma, float *dbeta, int64_t rows, int H, void *dmask, float drop_p, uint32_t seed, void *stream)
{
    if (!dy || !x || !gamma || !mean || !rstd || !dx || !dgamma || !dbeta || !dmask || rows < 1 || drop_p <= 0.f || drop_p >= 1.f) return -1;
    const LnBwd a = {dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, rows, H, dmask, drop_p, seed, false};
    if (!ln_bwd_k768(a)) return -4;
    ln_bwd_launch(a, true, stream);
    return LAUNCH_OK();
}

// ---- ordered ("deterministic gradients") form: include/emdr2_ops.h ---------------------------------------------------------------------
extern "C" int emdr2_layernorm_bwd_ordered_ws_bytes(int64_t rows, int H, size_t *bytes)
{
    if (!bytes || rows < 1 || H < 1 || H > 8192) return -1;
    long long slots = ln_bwd_slots(rows, H, false);                      // the caller does not know yet which kernel its pointers will take
    if (H == 768 && ln_bwd_slots(rows, H, true) > slots) slots = ln_bwd_slots(rows, H, true);
    *bytes = (size_t)slots * 2 * H * sizeof(float);
    return 0;
}

// ORDER.  H == 768, aligned: gridDim = min(ceil(rows / 8), 2048) workgroups, a function of `rows` alone; wave w of workgroup b takes the row
// pairs 4 b + w, + 4 gridDim, ... in ascending order, each half-wave one row of the pair; a column's partial is (half 0 + half 1), then
// ((wave 0 + wave 1) + wave 2) + wave 3, stored in slot b.  Otherwise: workgroup b owns rows [32 b, 32 b + 32), summed in ascending order,
// slot b.  Both: dgamma[c] = dgamma[c] + total of the slots as ordered_slot_sum<., 32> adds them (ordered_sum.h), likewise dbeta.
extern "C" int emdr2_layernorm_bwd_ordered(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd, const void *dres, void *dx,
                                           float *dgamma, float *dbeta, int64_t rows, int H, void *dmask, float drop_p, uint32_t seed, void *ws,
                                           size_t ws_bytes, void *stream)
{
    if (!dy || !x || !gamma || !mean || !rstd || !dx || !dgamma || !dbeta || !ws || ((uintptr_t)ws & 15) || rows < 1 || H < 1 || H > 8192) return -1;
    if (dmask && (drop_p <= 0.f || drop_p >= 1.f)) return -1;
    float *part = (float *)ws;
    const LnBwd a = {dy, x, gamma, mean, rstd, dres, dx, part, nullptr, rows, H, dmask, drop_p, seed, true};
    const bool k768 = ln_bwd_k768(a);
    if (dmask && !k768) return -4;
    const long long slots = ln_bwd_slots(rows, H, k768);
    if (slots > 0x7fffffffll) return -4;
    if (ws_bytes < (size_t)slots * 2 * H * sizeof(float)) return -2;
    ln_bwd_launch(a, k768, stream);
    ordered_slot_sum(part, 2ll * H, (int)slots, dgamma, H, H, 1, true, false, (hipStream_t)stream);
    ordered_slot_sum(part + H, 2ll * H, (int)slots, dbeta, H, H, 1, true, false, (hipStream_t)stream);
    return LAUNCH_OK();
}
