// emdr2_amd/csrc/ordered_sum.h -- the finishing pass of the ordered ("deterministic gradients") entries of include/emdr2_ops.h: partial sums
// that a first launch stored into workspace slots are added up in an order fixed by the slot COUNT alone and the total goes onto the
// destination with one fp32 add per element.  Launched on the stream of the launch that stored the slots: stream order publishes them (no
// ticket, no flag, no workgroup waiting for another).
#ifndef EMDR2_ORDERED_SUM_H
#define EMDR2_ORDERED_SUM_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// dst[r * ld + c] += total(e),  e = r * width + c < count,  slot s at ws + s * slot_stride + e.
// ORDER.  G == 1: total = ((s_0 + s_1) + s_2) + ... in slot order.  G > 1: group g (fixed: lanes [g * 256 / G, (g + 1) * 256 / G) of the
// workgroup) takes slots g, g + G, g + 2 G, ... : part_g = ((s_g + s_{g+G}) + s_{g+2G}) + ...; total = ((part_0 + part_1) + part_2) + ... over
// the groups g < min(G, slots).  V elements (V * 4 bytes) per lane.  skip_zero: a total of exactly zero is not added (the destination keeps
// its bits, -0.0 and NaN payloads included: rows nobody contributed to).
template <int V, int G>
__global__ void __launch_bounds__(256) ordered_slot_sum_kernel(const float *ws, long long slot_stride, int slots, float *dst, long long ld, int width,
                                                               long long count, int skip_zero)
{
    constexpr int L = 256 / G;
    __shared__ float sh[G > 1 ? G : 1][L][V];
    const int el = threadIdx.x % L, g = threadIdx.x / L;
    const long long e = ((long long)blockIdx.x * L + el) * V;
    const bool live = e < count;
    float t[V];
#pragma unroll
    for (int v = 0; v < V; ++v) t[v] = 0.f;
    if (live && g < slots) {
        const float *src = ws + e;
        auto load = [&](int s, float *o) {
            if (V == 4) { const float4 q = *(const float4 *)(src + (long long)s * slot_stride); o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w; }
            else o[0] = src[(long long)s * slot_stride];
        };
        load(g, t);
        int s = g + G;
        for (; s + 3 * G < slots; s += 4 * G) {                      // four loads in flight, added in slot order
            float a[4][V];
#pragma unroll
            for (int u = 0; u < 4; ++u) load(s + u * G, a[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < V; ++v) t[v] += a[u][v];
        }
        for (; s < slots; s += G) {
            float a[V];
            load(s, a);
#pragma unroll
            for (int v = 0; v < V; ++v) t[v] += a[v];
        }
    }
    if (G > 1) {
#pragma unroll
        for (int v = 0; v < V; ++v) sh[g][el][v] = t[v];
        __syncthreads();
        if (g != 0) return;
        const int ng = slots < G ? slots : G;
        for (int k = 1; k < ng; ++k)
#pragma unroll
            for (int v = 0; v < V; ++v) t[v] += sh[k][el][v];
    }
    if (!live) return;
    float *d = dst + (e / width) * ld + (e % width);
    if (V == 4) {
        float4 q = *(float4 *)d;
        if (!skip_zero || t[0] != 0.f) q.x += t[0];
        if (!skip_zero || t[1] != 0.f) q.y += t[1];
        if (!skip_zero || t[2] != 0.f) q.z += t[2];
        if (!skip_zero || t[3] != 0.f) q.w += t[3];
        *(float4 *)d = q;
    } else if (!skip_zero || t[0] != 0.f) {
        *d += t[0];
    }
}

// `grouped`: many slots per element (G = 32) against few (G = 1, strict slot order).  16 bytes per lane when everything is 16-byte aligned.
inline void ordered_slot_sum(const float *ws, long long slot_stride, int slots, float *dst, long long ld, int width, long long rows, bool grouped,
                             bool skip_zero, hipStream_t stream)
{
    const long long count = rows * width;
    const bool vec = !(width & 3) && !(ld & 3) && !(slot_stride & 3) && !(((uintptr_t)ws | (uintptr_t)dst) & 15);
    const int V = vec ? 4 : 1, L = grouped ? 8 : 256;
    const dim3 grid((unsigned)((count + (long long)L * V - 1) / ((long long)L * V)));
#define EMDR2_OSS(VV, GG) hipLaunchKernelGGL((ordered_slot_sum_kernel<VV, GG>), grid, dim3(256), 0, stream, ws, slot_stride, slots, dst, ld, width, count, (int)skip_zero)
    if (vec) { if (grouped) EMDR2_OSS(4, 32); else EMDR2_OSS(4, 1); }
    else { if (grouped) EMDR2_OSS(1, 32); else EMDR2_OSS(1, 1); }
#undef EMDR2_OSS
}

} // namespace
#endif
