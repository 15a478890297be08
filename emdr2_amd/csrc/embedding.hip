// emdr2_amd/csrc/embedding.hip -- word + position (+ token-type) embedding, dense and packed rows, and its backward in the atomic and the
// ordered form (include/emdr2_ops.h: emdr2_embedding_*).
#include "../../include/emdr2_ops.h"
#include "prims.h"
#include "rng.h"
#include "ordered_sum.h"

namespace {

// ---- embedding (language_model.py:169-181): out = W[ids] + P[pos] (+ T[types]) ------------------------------------------------
__global__ void __launch_bounds__(256) embedding_fwd_kernel(const long long *ids, const long long *types, const uint16_t *W, const uint16_t *P,
                                                            const uint16_t *T, uint16_t *out, long long tokens, int S, int H, float drop_p, uint32_t seed,
                                                            const int *rowmap)
{
    // rowmap (packed layout, csrc/seqpack.hip): row t holds the token of dense row rowmap[t] = sequence * S + position; -1 = a tail row (zeros)
    const long long t = blockIdx.x;
    long long pos = t % S;
    if (rowmap) {
        const int src = rowmap[t];
        if (src < 0) {
            for (int i = threadIdx.x; i < H; i += 256) out[t * H + i] = 0;
            return;
        }
        pos = src % S;
    }
    const long long id = ids[t];
    const long long ty = types ? types[t] : 0;
    for (int i = threadIdx.x; i < H; i += 256) {
        float v = bf2f(W[id * H + i]) + bf2f(P[pos * H + i]);
        if (types) v += bf2f(T[ty * H + i]);
        if (drop_p > 0.f) v = emdr2_keep(emdr2_row_hash(seed, (unsigned long long)t), (uint32_t)i, emdr2_drop_thr(drop_p)) ? v * emdr2_keep_scale(drop_p) : 0.f;
        out[t * H + i] = f2bf(v);
    }
}

// word-embedding rows: atomic scatter (ids are spread over the vocabulary, little contention)
__global__ void __launch_bounds__(256) embedding_bwd_kernel(const long long *ids, const long long *types, const uint16_t *dout, float *dW, float *dP,
                                                            float *dT, long long tokens, int S, int H, float drop_p, uint32_t seed)
{
    const long long t = blockIdx.x;
    const long long id = ids[t];
    // In training, padding positions receive exactly zero gradient (masked as keys everywhere, nothing reads their outputs, every backward
    // kernel maps zero rows to zero rows) and half of the reader's tokens are padding: adding their zeros to row 0 serialised ~800k atomics
    // per column on one address.  A row of zeros is skipped whatever its id (adding it changes nothing, so this is exact for any caller).
    int nz = 0;
    for (int i = threadIdx.x; i < H; i += 256) nz |= (dout[t * H + i] & 0x7fff) != 0;
    if (!__syncthreads_or(nz)) return;
    const uint32_t rh = emdr2_row_hash(seed, (unsigned long long)t), thr = emdr2_drop_thr(drop_p);
    const float ik = drop_p > 0.f ? emdr2_keep_scale(drop_p) : 1.f;
    for (int i = threadIdx.x; i < H; i += 256) {
        float g = bf2f(dout[t * H + i]);
        if (drop_p > 0.f) g = emdr2_keep(rh, (uint32_t)i, thr) ? g * ik : 0.f;
        if (g != 0.f) atomicAdd(&dW[id * H + i], g);         // a dropped or zero element adds nothing: x + (+0.0) would turn a -0.0 into +0.0
    }
}

// position and token-type rows: every sequence hits the same S position rows and the same one or two type rows, so an atomic per token
// serialises thousands of adds on a few addresses.  One thread owns (position, column) for ONE SLICE of the batch (gridDim.z slices: a
// single walker per (position, column) made 3,200 dependent loads in a row -- 2.6 ms at the reader's shape), walks its sequences, and adds
// its sums with one atomic per table entry: S x H x slices atomics instead of one per token.
// ORD (emdr2_embedding_bwd_ordered): no atomics -- slice z = blockIdx.z stores its sums, zeros included, into workspaces passed as dP
// ([slices][S][H]) and dT ([S][slices][n_types][H]); ordered_slot_sum adds them (position rows: slice order; type rows: slot pos * slices + z).
template <bool ORD>
__global__ void __launch_bounds__(256) embedding_bwd_pos_kernel(const long long *types, const uint16_t *dout, float *dP, float *dT, long long tokens,
                                                                int S, int H, int n_types, float drop_p, uint32_t seed, const int *cu, int nseq)
{
    // cu (packed layout): sequence b owns rows [cu[b], cu[b+1]); its position `pos` exists iff pos < its length
    const int pos = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;
    if (i >= H) return;
    const long long nb = cu ? nseq : tokens / S;
    const uint32_t thr = emdr2_drop_thr(drop_p);
    const float ik = drop_p > 0.f ? emdr2_keep_scale(drop_p) : 1.f;
    float ap = 0.f, at[4] = {0.f, 0.f, 0.f, 0.f};
    for (long long b = blockIdx.z; b < nb; b += gridDim.z) {
        long long t = b * S + pos;
        if (cu) {
            const int c0 = cu[b];
            if (pos >= cu[b + 1] - c0) continue;
            t = c0 + pos;
        }
        float g = bf2f(dout[t * H + i]);
        if (drop_p > 0.f) g = emdr2_keep(emdr2_row_hash(seed, (unsigned long long)t), (uint32_t)i, thr) ? g * ik : 0.f;
        ap += g;
        if (types) {
            const int ty = (int)types[t];
#pragma unroll
            for (int k = 0; k < 4; ++k) at[k] += (ty == k) ? g : 0.f;
        }
    }
    if (ORD) {
        dP[((long long)blockIdx.z * S + pos) * H + i] = ap;
        if (types) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n_types) dT[(((long long)pos * gridDim.z + blockIdx.z) * n_types + k) * H + i] = at[k];
        }
        return;
    }
    if (ap != 0.f) atomicAdd(&dP[(long long)pos * H + i], ap);
    if (types) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n_types && at[k] != 0.f) atomicAdd(&dT[(long long)k * H + i], at[k]);
    }
}

// ---- ordered word-embedding rows (emdr2_embedding_bwd_ordered): store-and-sum through an inverted index, no atomics ---------------------
// `order` = the stable sort of the token indices by id: position q of the sorted sequence holds token order[q], ids[order[q]] ascending, equal
// ids in ascending token index.  The contribution rows are the rows of dout themselves (the dropout mask is re-applied on the way in).
// ORDER.  The sorted sequence is cut at the multiples of EMB_CHUNK.  A run of equal ids inside one chunk is summed sequentially in sorted
// order, from +0.0.  A run that lies inside one chunk is added onto dW[id] there; a run that crosses a chunk boundary leaves one piece per
// chunk (slot 0 of the chunk: its first run, slot 1: its last run when that is another one) and the finish kernel adds the pieces in
// ascending chunk order, ((piece_0 + piece_1) + piece_2) + ..., then adds the total onto dW[id] once.  A total of exactly zero is not added,
// and a vocabulary row without tokens is never touched.
#define EMB_CHUNK 128
template <bool VEC>
__global__ void __launch_bounds__(128) embedding_bwd_words_ordered_kernel(const long long *ids, const long long *order, const uint16_t *dout, float *dW,
                                                                          float *part, long long tokens, int H, float drop_p, uint32_t seed)
{
    constexpr int NV = VEC ? 8 : 1;
    __shared__ long long s_tok[EMB_CHUNK], s_id[EMB_CHUNK + 2];          // s_id[0] / s_id[n + 1]: the neighbours' ids, -1 = none (ids are >= 0)
    const int tid = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * EMB_CHUNK;
    const int n = (int)(tokens - q0 < EMB_CHUNK ? tokens - q0 : EMB_CHUNK);
    if (tid < n) { const long long t = order[q0 + tid]; s_tok[tid] = t; s_id[1 + tid] = ids[t]; }
    if (tid == 0) s_id[0] = q0 > 0 ? ids[order[q0 - 1]] : -1;
    if (tid == 1) s_id[n + 1] = q0 + n < tokens ? ids[order[q0 + n]] : -1;
    __syncthreads();
    const int col = (blockIdx.y * 128 + tid) * NV;
    if (col >= H) return;
    const uint32_t thr = emdr2_drop_thr(drop_p);
    const float ik = drop_p > 0.f ? emdr2_keep_scale(drop_p) : 1.f;
    float acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.f;
    auto flush = [&](long long id, bool piece, int slot) {
        if (piece) {
            float *o = part + ((long long)blockIdx.x * 2 + slot) * H + col;
            if (VEC) { *(float4 *)o = make_float4(acc[0], acc[1], acc[2], acc[3]); *(float4 *)(o + 4) = make_float4(acc[4 % NV], acc[5 % NV], acc[6 % NV], acc[7 % NV]); }
            else o[0] = acc[0];
        } else {
            float *o = dW + id * H + col;
#pragma unroll
            for (int v = 0; v < NV; ++v)
                if (acc[v] != 0.f) o[v] += acc[v];
        }
    };
    long long run = s_id[1];
    bool first = true;
    for (int q = 0; q < n; ++q) {
        const long long id = s_id[1 + q];
        if (id != run) {                                              // workgroup-uniform
            flush(run, first && s_id[0] == run, 0);
            first = false;
            run = id;
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] = 0.f;
        }
        const long long t = s_tok[q];
        const uint32_t rh = emdr2_row_hash(seed, (unsigned long long)t);
        if (VEC) {
            const uint4 w4 = *(const uint4 *)(dout + t * H + col);
            const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float lo = bf2f((uint16_t)(w[j] & 0xffff)), hi = bf2f((uint16_t)(w[j] >> 16));
                if (drop_p > 0.f) {
                    const uint32_t b = emdr2_pair_bits(rh, (uint32_t)(col + 2 * j));
                    lo = (b & 0xffffu) >= thr ? lo * ik : 0.f;
                    hi = (b >> 16) >= thr ? hi * ik : 0.f;
                }
                acc[(2 * j) % NV] += lo; acc[(2 * j + 1) % NV] += hi;
            }
        } else {
            float g = bf2f(dout[t * H + col]);
            if (drop_p > 0.f) g = emdr2_keep(rh, (uint32_t)col, thr) ? g * ik : 0.f;
            acc[0] += g;
        }
    }
    const bool before = first && s_id[0] == run, after = s_id[n + 1] == run;
    flush(run, before || after, first ? 0 : 1);
}

// one workgroup per chunk; it acts when a run that crosses chunk boundaries STARTS in its chunk
template <bool VEC>
__global__ void __launch_bounds__(128) embedding_bwd_words_finish_kernel(const long long *ids, const long long *order, const float *part, float *dW,
                                                                         long long tokens, int H)
{
    constexpr int NV = VEC ? 4 : 1;
    const long long k = blockIdx.x, q0 = k * EMB_CHUNK, q1 = q0 + EMB_CHUNK;
    if (q1 >= tokens) return;                                         // the last chunk: nothing continues
    const long long id = ids[order[q1 - 1]];
    if (ids[order[q1]] != id) return;                                 // the chunk's last run ends with it
    const bool single = ids[order[q0]] == id;                         // the chunk is one run
    if (single && q0 > 0 && ids[order[q0 - 1]] == id) return;         // a middle piece: the chunk where the run starts does the sum
    long long lo = q1 + 1, hi = tokens;                               // end of the run: the first position past q1 with another id
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (ids[order[mid]] == id) lo = mid + 1; else hi = mid;
    }
    const long long ke = (lo - 1) / EMB_CHUNK;                        // the chunk of the run's last token; pieces k + 1 .. ke sit in slot 0
    const int col = (blockIdx.y * 128 + threadIdx.x) * NV;
    if (col >= H) return;
    float t[NV];
    const float *p0 = part + (k * 2 + (single ? 0 : 1)) * H + col;
#pragma unroll
    for (int v = 0; v < NV; ++v) t[v] = p0[v];
#pragma unroll 4
    for (long long kk = k + 1; kk <= ke; ++kk) {
        const float *pk = part + kk * 2 * H + col;
        if (VEC) { const float4 a = *(const float4 *)pk; t[0] += a.x; t[1 % NV] += a.y; t[2 % NV] += a.z; t[3 % NV] += a.w; }
        else t[0] += pk[0];
    }
    float *o = dW + id * H + col;
#pragma unroll
    for (int v = 0; v < NV; ++v)
        if (t[v] != 0.f) o[v] += t[v];
}

} // namespace

// ---- forward: the dense and the packed entry are one launch, with and without the row map --------------------------------------------------
static int embedding_fwd(const int64_t *ids, const int64_t *types, const int32_t *rowmap, const void *W, const void *P, const void *T, void *out,
                         int64_t rows, int S, int H, float drop_p, uint32_t seed, void *stream)
{
    if (!ids || !W || !P || !out || rows < 1 || S < 1 || H < 1 || (types && !T) || drop_p < 0.f || drop_p >= 1.f) return -1;
    launch(embedding_fwd_kernel, dim3((unsigned)rows), 256, stream, ids, types, W, P, T, out, rows, S, H, drop_p, seed, rowmap);
    return LAUNCH_OK();
}

extern "C" int emdr2_embedding_fwd(const int64_t *ids, const int64_t *types, const void *W, const void *P, const void *T, void *out, int64_t tokens,
                                   int S, int H, float drop_p, uint32_t seed, void *stream)
{
    return embedding_fwd(ids, types, nullptr, W, P, T, out, tokens, S, H, drop_p, seed, stream);
}

extern "C" int emdr2_embedding_packed_fwd(const int64_t *ids, const int64_t *types, const int32_t *rowmap, const void *W, const void *P, const void *T, void *out,
                                          int64_t rows, int S, int H, float drop_p, uint32_t seed, void *stream)
{
    if (!rowmap) return -1;
    return embedding_fwd(ids, types, rowmap, W, P, T, out, rows, S, H, drop_p, seed, stream);
}

// ---- backward: what the atomic (dense, packed) and the ordered entry share -------------------------------------------------------------------
struct EmbBwd {
    const int64_t *ids, *types;
    const int32_t *cu; int nseq;      // cu nullptr: dense rows, rows / S sequences of S tokens; else the packed layout's nseq row offsets
    const void *dout; float *dW, *dP, *dT;
    long long rows; int S, H, n_types; float drop_p; uint32_t seed; void *stream;
};

static int emb_bwd_check(const EmbBwd &a)
{
    if (!a.ids || !a.dout || !a.dW || !a.dP || a.rows < 1 || a.S < 1 || a.H < 1 || (a.types && !a.dT) || (a.cu && a.nseq < 1) || a.drop_p < 0.f ||
        a.drop_p >= 1.f)
        return -1;
    if ((!a.cu && a.rows % a.S) || (a.types && (a.n_types < 1 || a.n_types > 4))) return -4;
    return 0;
}

static long long emb_nseq(const EmbBwd &a) { return a.cu ? a.nseq : a.rows / a.S; }
// batch slices of the position-gradient kernel: ~256 sequences per walker, at most 16 slices
static unsigned pos_slices(long long nseq) { const long long s = (nseq + 255) / 256; return (unsigned)(s < 1 ? 1 : (s > 16 ? 16 : s)); }

// position and type rows onto dP / dT: the gradient tables themselves (atomics) or the ordered entry's slice workspaces
template <bool ORD>
static void emb_bwd_pos_launch(const EmbBwd &a, float *dP, float *dT)
{
    launch(embedding_bwd_pos_kernel<ORD>, dim3((unsigned)a.S, (unsigned)((a.H + 255) / 256), pos_slices(emb_nseq(a))), 256, a.stream, a.types, a.dout, dP, dT,
           a.rows, a.S, a.H, a.n_types, a.drop_p, a.seed, a.cu, a.nseq);
}

// word rows by atomic scatter (a packed tail row carries a zero gradient and is skipped like any zero row), then the position rows
static int emb_bwd_atomic(const EmbBwd &a)
{
    if (const int rc = emb_bwd_check(a)) return rc;
    launch(embedding_bwd_kernel, dim3((unsigned)a.rows), 256, a.stream, a.ids, a.types, a.dout, a.dW, a.dP, a.dT, a.rows, a.S, a.H, a.drop_p, a.seed);
    emb_bwd_pos_launch<false>(a, a.dP, a.dT);
    return LAUNCH_OK();
}

extern "C" int emdr2_embedding_bwd(const int64_t *ids, const int64_t *types, const void *dout, float *dW, float *dP, float *dT, int64_t tokens, int S,
                                   int H, int n_types, float drop_p, uint32_t seed, void *stream)
{
    return emb_bwd_atomic({ids, types, nullptr, 0, dout, dW, dP, dT, tokens, S, H, n_types, drop_p, seed, stream});
}

extern "C" int emdr2_embedding_packed_bwd(const int64_t *ids, const int64_t *types, const int32_t *cu, int nseq, const void *dout, float *dW, float *dP, float *dT,
                                          int64_t rows, int S, int H, int n_types, float drop_p, uint32_t seed, void *stream)
{
    if (!cu || nseq < 1) return -1;
    return emb_bwd_atomic({ids, types, cu, nseq, dout, dW, dP, dT, rows, S, H, n_types, drop_p, seed, stream});
}

// ---- ordered ("deterministic gradients") form: include/emdr2_ops.h ---------------------------------------------------------------------
static inline size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }

static size_t emb_ordered_floats(long long tokens, long long nseq, int S, int H, int n_types, size_t *pos_off, size_t *typ_off)
{
    const size_t chunks = (size_t)((tokens + EMB_CHUNK - 1) / EMB_CHUNK), slices = pos_slices(nseq);
    const size_t words = round4(chunks * 2 * H), pos = round4(slices * S * H), typ = round4((size_t)S * slices * n_types * H);
    if (pos_off) *pos_off = words;
    if (typ_off) *typ_off = words + pos;
    return words + pos + typ;
}

extern "C" int emdr2_embedding_bwd_ordered_ws_bytes(int64_t tokens, int nseq, int S, int H, int n_types, size_t *bytes)
{
    if (!bytes || tokens < 1 || nseq < 1 || S < 1 || H < 1 || n_types < 0 || n_types > 4) return -1;
    *bytes = emb_ordered_floats(tokens, nseq, S, H, n_types, nullptr, nullptr) * sizeof(float);
    return 0;
}

// The order of the word rows stands at embedding_bwd_words_ordered_kernel.  Position rows: slice z of pos_slices(number of sequences) walks the
// sequences z, z + slices, ... in ascending order; dP[pos] += ((slice 0 + slice 1) + ...).  Type rows: the same per-(position, slice) sums,
// slot = pos * slices + z, added as ordered_slot_sum<., 32> adds slots.  Totals of exactly zero are not added (positions nobody reaches).
extern "C" int emdr2_embedding_bwd_ordered(const int64_t *ids, const int64_t *types, const int32_t *cu, int nseq, const int64_t *order, const void *dout,
                                           float *dW, float *dP, float *dT, int64_t tokens, int S, int H, int n_types, float drop_p, uint32_t seed, void *ws,
                                           size_t ws_bytes, void *stream)
{
    if (!order || !ws || ((uintptr_t)ws & 15)) return -1;
    const EmbBwd a = {ids, types, cu, nseq, dout, dW, dP, dT, tokens, S, H, n_types, drop_p, seed, stream};
    if (const int rc = emb_bwd_check(a)) return rc;
    const int nt = types ? n_types : 0;
    size_t pos_off, typ_off;
    if (ws_bytes < emb_ordered_floats(tokens, emb_nseq(a), S, H, nt, &pos_off, &typ_off) * sizeof(float)) return -2;
    float *part_w = (float *)ws, *part_p = part_w + pos_off, *part_t = part_w + typ_off;
    const long long chunks = (tokens + EMB_CHUNK - 1) / EMB_CHUNK;
    if (chunks > 0x7fffffffll) return -4;
    const bool vec = !(H & 7) && !(((uintptr_t)dout | (uintptr_t)dW) & 15);
    const int per = vec ? 128 * 8 : 128, per_fin = vec ? 128 * 4 : 128;                        // columns per workgroup: the sum, the finish
    launch(vec ? embedding_bwd_words_ordered_kernel<true> : embedding_bwd_words_ordered_kernel<false>, dim3((unsigned)chunks, (unsigned)((H + per - 1) / per)),
           128, stream, ids, order, dout, dW, part_w, tokens, H, drop_p, seed);
    launch(vec ? embedding_bwd_words_finish_kernel<true> : embedding_bwd_words_finish_kernel<false>,
           dim3((unsigned)chunks, (unsigned)((H + per_fin - 1) / per_fin)), 128, stream, ids, order, part_w, dW, tokens, H);
    emb_bwd_pos_launch<true>(a, part_p, part_t);
    const unsigned slices = pos_slices(emb_nseq(a));
    ordered_slot_sum(part_p, (long long)S * H, (int)slices, dP, H, H, S, false, true, (hipStream_t)stream);
    if (types) ordered_slot_sum(part_t, (long long)n_types * H, (int)(S * slices), dT, H, H, n_types, true, true, (hipStream_t)stream);
    return LAUNCH_OK();
}
