// emdr2_amd/csrc/optimizer.hip -- the optimizer's kernels over fp32 masters: the gradient-norm sum, Adam, and the casts of the bf16 gradient
// exchange (include/emdr2_ops.h).
#include "../../include/emdr2_ops.h"
#include "prims.h"
#include "adam_bias.h"

namespace {

// ---- optimizer: fp32 masters, decoupled weight decay Adam (apex FusedAdam defaults, training.py:89; SURVEY 8c: unpinned) -------
// Deterministic: block partials go to scratch[0 .. grid) and the LAST block to finish adds them up in index order, so the sum (and with
// it the clip factor every data-parallel replica derives from it) does not depend on the arrival order of atomics.  scratch: 1024
// partial slots + one counter word at [1024] (zero before the first use; the kernel resets it).
// GUARD (emdr2_sumsq_census_f32): a census of the non-finite elements rides in the same pass -- the sum's own statements, and so its
// bits, are those of the plain form.  census[0] += NaN elements, census[1] += +-Inf elements, census[2] = min(census[2], (bucket << 40) |
// index) over them.  Tallies stay in registers; a wave whose 64 tallies are all zero (every wave of a healthy step) issues no atomic,
// any other wave one per census word.
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const unsigned long long w = __shfl_xor(v, o); v = w < v ? w : v; }
    return v;
}
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool GUARD>
__global__ void __launch_bounds__(256) sumsq_kernel(const float *g, long long n, float *out, float *scratch, unsigned long long *census,
                                                    unsigned long long bucket)
{
    __shared__ float red[4];
    __shared__ bool last;
    float s = 0.f;
    unsigned nan = 0u, inf = 0u;
    unsigned long long first = ~0ull;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float x = g[i];
        s += x * x;
        if constexpr (GUARD) {
            const uint32_t a = __float_as_uint(x) & 0x7fffffffu;
            if (a >= 0x7f800000u) {                                      // (rare: the tallies cost the clean path one compare per element)
                if (a > 0x7f800000u) ++nan; else ++inf;
                const unsigned long long key = (bucket << 40) | (unsigned long long)i;
                first = key < first ? key : first;                       // (i ascends per thread: the first hit is the thread's minimum)
            }
        }
    }
    if constexpr (GUARD) {
        if (__any((int)(nan | inf))) {                                   // wave-uniform
            nan = wave_sum_u32(nan); inf = wave_sum_u32(inf); first = wave_min_u64(first);
            if ((threadIdx.x & 63) == 0) {
                if (nan) atomicAdd(census + 0, (unsigned long long)nan);
                if (inf) atomicAdd(census + 1, (unsigned long long)inf);
                atomicMin(census + 2, first);
            }
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    unsigned *counter = (unsigned *)(scratch + 1024);                  // fixed slot: partials of launches with other grid sizes never alias it
    if (threadIdx.x == 0) {
        scratch[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        __threadfence();
        last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    float t = 0.f;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += 256) t += ((volatile float *)scratch)[i];   // fixed assignment of partials to lanes
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) { *out += (red[0] + red[1]) + (red[2] + red[3]); *counter = 0u; }    // launches on one stream are ordered
}

// The step's verdict (emdr2_step_verdict): ONE rule -- the step is skipped exactly when the summed squared norm is not finite (NaN or
// +-Inf; squares of finite elements that overflow fp32 included) -- applied once per step by one thread, between the last bucket's sum and
// the first Adam launch.  state[0] verdict, [1] skipped in total, [2] current run, [3] longest run, [4..7] the sticky record of the first
// skip since the host cleared it (state[4] == 0: empty; steps count from 1): step, first key, NaN count, Inf count.  The census is left
// ready for the next step.
__global__ void __launch_bounds__(64) step_verdict_kernel(const float *gnorm_sq, unsigned long long *census, unsigned long long *state,
                                                          unsigned long long step)
{
    if (threadIdx.x != 0) return;
    const bool skipped = (__float_as_uint(*gnorm_sq) & 0x7fffffffu) >= 0x7f800000u;
    state[0] = skipped ? 1ull : 0ull;
    if (skipped) {
        const unsigned long long run = state[2] + 1ull;
        state[1] += 1ull;
        state[2] = run;
        if (run > state[3]) state[3] = run;
        if (state[4] == 0ull) { state[4] = step; state[5] = census[2]; state[6] = census[0]; state[7] = census[1]; }
    } else {
        state[2] = 0ull;
    }
    census[0] = 0ull; census[1] = 0ull; census[2] = ~0ull; census[3] = 0ull;
}

__global__ void __launch_bounds__(256) adam_kernel(float *master, const float *grad, float *m, float *v, uint16_t *param_bf16, long long n, float lr,
                                                   float b1, float b2, float eps, float wd, float bc1, float bc2, const float *gnorm_sq,
                                                   float clip)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float scale = 1.f;
    if (gnorm_sq && clip > 0.f) { const float gn = sqrtf(*gnorm_sq); const float c = clip / (gn + 1.0e-6f); if (c < 1.f) scale = c; }
    const float g = grad[i] * scale;
    const float mi = b1 * m[i] + (1.f - b1) * g;
    const float vi = b2 * v[i] + (1.f - b2) * g * g;
    m[i] = mi; v[i] = vi;
    const float upd = (mi / bc1) / (sqrtf(vi / bc2) + eps) + wd * master[i];
    const float w = master[i] - lr * upd;
    master[i] = w;
    if (param_bf16) param_bf16[i] = f2bf(w);
}

// Adam over one FLAT bucket (all tensors of the bucket back to back; n % 4 == 0 by construction of the buckets): four elements per thread,
// 16-byte accesses.  Elements [0, split) take the decoupled weight decay, [split, n) none (LayerNorm parameters and biases,
// megatron/model/utils.py:64-83): the bucket stores its decayed parameters first, so one launch covers both groups.
// GUARD (emdr2_adam_step_flat_guarded): a skipped step (state[0] == 1, written by step_verdict_kernel) returns before the first load of a
// bucket element and stores nothing; an applied one runs the statements below unchanged.
template <bool GUARD>
__global__ void __launch_bounds__(256) adam_flat_kernel(float4 *master, const float4 *grad, float4 *m, float4 *v, uint2 *work_bf16, long long n4,
                                                        long long split4, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2,
                                                        const float *gnorm_sq, float clip, const unsigned long long *state)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    if constexpr (GUARD) { if (state[0] != 0ull) return; }
    float scale = 1.f;
    if (gnorm_sq && clip > 0.f) { const float gn = sqrtf(*gnorm_sq); const float c = clip / (gn + 1.0e-6f); if (c < 1.f) scale = c; }
    const float wdi = i < split4 ? wd : 0.f;
    const float4 g4 = grad[i], m4 = m[i], v4 = v[i], w4 = master[i];
    float g[4] = {g4.x, g4.y, g4.z, g4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w}, w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float gj = g[j] * scale;
        mm[j] = b1 * mm[j] + (1.f - b1) * gj;
        vv[j] = b2 * vv[j] + (1.f - b2) * gj * gj;
        const float upd = (mm[j] / bc1) / (sqrtf(vv[j] / bc2) + eps) + wdi * w[j];
        w[j] = w[j] - lr * upd;
    }
    m[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
    v[i] = make_float4(vv[0], vv[1], vv[2], vv[3]);
    master[i] = make_float4(w[0], w[1], w[2], w[3]);
    if (work_bf16) work_bf16[i] = make_uint2((uint32_t)f2bf(w[0]) | ((uint32_t)f2bf(w[1]) << 16), (uint32_t)f2bf(w[2]) | ((uint32_t)f2bf(w[3]) << 16));
}

// gradient exchange in bf16 (the reference all-reduces fp16 gradients pre-divided by the world size, model/distributed.py:53-62):
// dst_bf16 = bf16(scale * src), and the way back dst_f32 = float(src_bf16); n % 4 == 0
__global__ void __launch_bounds__(256) scale_cast_kernel(const float4 *src, uint2 *dst, long long n4, float scale)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 x = src[i];
    dst[i] = make_uint2((uint32_t)f2bf(x.x * scale) | ((uint32_t)f2bf(x.y * scale) << 16), (uint32_t)f2bf(x.z * scale) | ((uint32_t)f2bf(x.w * scale) << 16));
}

__global__ void __launch_bounds__(256) widen_kernel(const uint2 *src, float4 *dst, long long n4)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const uint2 x = src[i];
    dst[i] = make_float4(bf2f((uint16_t)(x.x & 0xffff)), bf2f((uint16_t)(x.x >> 16)), bf2f((uint16_t)(x.y & 0xffff)), bf2f((uint16_t)(x.y >> 16)));
}

__global__ void __launch_bounds__(256) cast_kernel(const float *src, uint16_t *dst, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = f2bf(src[i]);
}

__global__ void __launch_bounds__(256) accum_bf16_to_f32_kernel(const uint16_t *src, float *dst, long long n, float scale)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] += scale * bf2f(src[i]);
}

} // namespace

// one thread per element (or per group of four): n work items in workgroups of 256
static dim3 grid256(long long n) { return dim3((unsigned)((n + 255) / 256)); }

extern "C" int emdr2_sumsq_f32(const float *g, int64_t n, float *out, float *scratch, void *stream)
{
    if (!g || !out || !scratch || n < 1) return -1;
    int blocks = (int)((n + 2047) / 2048);                               // a function of n only: every replica uses the same grid
    if (blocks > 1024) blocks = 1024;
    launch(sumsq_kernel<false>, dim3(blocks), 256, stream, g, n, out, scratch, nullptr, 0);
    return LAUNCH_OK();
}

extern "C" int emdr2_sumsq_census_f32(const float *g, int64_t n, float *out, float *scratch, uint64_t *census, int bucket, void *stream)
{
    if (!g || !out || !scratch || !census || ((uintptr_t)census & 7) || n < 1 || n >= (1ll << 40) || bucket < 0 || bucket >= (1 << 23)) return -1;
    int blocks = (int)((n + 2047) / 2048);                               // the grid rule of emdr2_sumsq_f32
    if (blocks > 1024) blocks = 1024;
    launch(sumsq_kernel<true>, dim3(blocks), 256, stream, g, n, out, scratch, census, bucket);
    return LAUNCH_OK();
}

extern "C" int emdr2_step_verdict(const float *gnorm_sq, uint64_t *census, uint64_t *state, int64_t step, void *stream)
{
    if (!gnorm_sq || !census || !state || (((uintptr_t)census | (uintptr_t)state) & 7) || step < 1) return -1;
    launch(step_verdict_kernel, dim3(1), 64, stream, gnorm_sq, census, state, step);
    return LAUNCH_OK();
}

extern "C" int emdr2_adam_step(float *master, const float *grad, float *m, float *v, void *param_bf16, int64_t n, float lr, float beta1, float beta2,
                               float eps, float weight_decay, int step, const float *gnorm_sq, float clip, void *stream)
{
    if (!master || !grad || !m || !v || n < 1 || step < 1) return -1;
    float bc1, bc2;
    adam_bias_corrections(beta1, beta2, step, &bc1, &bc2);
    launch(adam_kernel, grid256(n), 256, stream, master, grad, m, v, param_bf16, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2, gnorm_sq, clip);
    return LAUNCH_OK();
}

// both forms of the flat Adam entry: state == NULL is the plain one
static int adam_flat(float *master, const float *grad, float *m, float *v, void *work_bf16, int64_t n, int64_t decay_split, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int step, const float *gnorm_sq, float clip, const uint64_t *state, void *stream)
{
    if (!master || !grad || !m || !v || n < 4 || (n & 3) || (decay_split & 3) || decay_split < 0 || decay_split > n || step < 1) return -1;
    if (((uintptr_t)master | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15 || ((uintptr_t)work_bf16 & 7) || ((uintptr_t)state & 7)) return -1;
    float bc1, bc2;
    adam_bias_corrections(beta1, beta2, step, &bc1, &bc2);
    launch(state ? adam_flat_kernel<true> : adam_flat_kernel<false>, grid256(n / 4), 256, stream, master, grad, m, v, work_bf16, n / 4,
           decay_split / 4, lr, beta1, beta2, eps, weight_decay, bc1, bc2, gnorm_sq, clip, state);
    return LAUNCH_OK();
}

extern "C" int emdr2_adam_step_flat(float *master, const float *grad, float *m, float *v, void *work_bf16, int64_t n, int64_t decay_split, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, int step, const float *gnorm_sq, float clip, void *stream)
{
    return adam_flat(master, grad, m, v, work_bf16, n, decay_split, lr, beta1, beta2, eps, weight_decay, step, gnorm_sq, clip, nullptr, stream);
}

extern "C" int emdr2_adam_step_flat_guarded(float *master, const float *grad, float *m, float *v, void *work_bf16, int64_t n, int64_t decay_split,
                                            float lr, float beta1, float beta2, float eps, float weight_decay, int step, const float *gnorm_sq,
                                            float clip, const uint64_t *state, void *stream)
{
    if (!state) return -1;
    return adam_flat(master, grad, m, v, work_bf16, n, decay_split, lr, beta1, beta2, eps, weight_decay, step, gnorm_sq, clip, state, stream);
}

extern "C" int emdr2_scale_cast_f32_to_bf16(const float *src, void *dst, int64_t n, float scale, void *stream)
{
    if (!src || !dst || n < 4 || (n & 3) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 7)) return -1;
    launch(scale_cast_kernel, grid256(n / 4), 256, stream, src, dst, n / 4, scale);
    return LAUNCH_OK();
}

extern "C" int emdr2_widen_bf16_to_f32(const void *src, float *dst, int64_t n, void *stream)
{
    if (!src || !dst || n < 4 || (n & 3) || ((uintptr_t)dst & 15) || ((uintptr_t)src & 7)) return -1;
    launch(widen_kernel, grid256(n / 4), 256, stream, src, dst, n / 4);
    return LAUNCH_OK();
}

extern "C" int emdr2_cast_f32_to_bf16(const float *src, void *dst, int64_t n, void *stream)
{
    if (!src || !dst || n < 1) return -1;
    launch(cast_kernel, grid256(n), 256, stream, src, dst, n);
    return LAUNCH_OK();
}

extern "C" int emdr2_accum_bf16_to_f32(const void *src, float *dst, int64_t n, float scale, void *stream)
{
    if (!src || !dst || n < 1) return -1;
    launch(accum_bf16_to_f32_kernel, grid256(n), 256, stream, src, dst, n, scale);
    return LAUNCH_OK();
}
