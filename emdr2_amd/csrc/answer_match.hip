// emdr2_amd/csrc/answer_match.hip -- which retrieved passages hold a reference answer (include/emdr2_answers.h).
// hits_kernel: one workgroup per (question, AH_SLOTS_PER_WG slots).  The workgroup builds, in LDS, a bitset of the FIRST tokens of the
// question's answers, the answers' tokens (as many as AH_TOK_CAP / AH_ANS_CAP hold; the rest is read from global memory) and hash chains of
// the staged answers by first token.  Each wave then takes a slot and streams its passage through an LDS window of AH_WINDOW start
// positions (+ AH_OVERLAP tokens, so that a match may straddle windows; longer matches finish from global memory).  A start position
// costs one bitset lookup unless its token starts an answer; only then are the answers of that token's chain compared.
// best_kernel: one wave per question finds the first slot with a hit and adds one to its histogram bin.
#include "../../include/emdr2_answers.h"
#include "prims.h"

namespace {

#define AH_THREADS 256
#define AH_WAVES 4
#define AH_SLOTS_PER_WG 8
#define AH_WINDOW 256       // start positions per window (4 per lane)
#define AH_OVERLAP 32       // tokens staged behind a window
#define AH_TOK_CAP 2048     // answer tokens staged in LDS
#define AH_ANS_CAP 256      // answers staged in LDS (offsets + hash chains)
#define AH_HEADS 256
#define AH_BITSET_WORDS 2048
#define AH_NONE 0xFFFFFFFFFFFFFFFFull

struct HitParams {
    const uint16_t *passage_tokens;
    const int64_t *passage_off;
    int64_t n_docs;
    const int32_t *doc_ids;
    const uint16_t *ans_tokens;
    const int32_t *ans_off, *q_ans_off;
    const uint32_t *cont_bits;
    int32_t *hit_pos, *hit_ans;
    int n_b, k, groups;
};

__device__ __forceinline__ int head_of(unsigned t) { return (int)((t ^ (t >> 8)) & (AH_HEADS - 1)); }

__global__ void __launch_bounds__(AH_THREADS) hits_kernel(HitParams p)
{
    __shared__ uint32_t s_bits[AH_BITSET_WORDS];
    __shared__ uint16_t s_tok[AH_TOK_CAP];
    __shared__ int s_off[AH_ANS_CAP + 1];
    __shared__ int s_head[AH_HEADS];
    __shared__ int s_next[AH_ANS_CAP];
    __shared__ uint16_t s_win[AH_WAVES][AH_WINDOW + AH_OVERLAP];
    __shared__ int s_nstaged, s_empty;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / p.groups, grp = blockIdx.x % p.groups;
    const int a0 = p.q_ans_off[b], n_ans = p.q_ans_off[b + 1] - a0;

    for (int i = tid; i < AH_BITSET_WORDS; i += AH_THREADS) s_bits[i] = 0u;
    for (int i = tid; i < AH_HEADS; i += AH_THREADS) s_head[i] = -1;
    if (tid == 0) { s_nstaged = 0; s_empty = 0x7FFFFFFF; }
    __syncthreads();

    const uint16_t *atok = p.ans_tokens;                  // (rebased below once the question's first offset is known)
    if (n_ans > 0) {
        const int tok0 = p.ans_off[a0];
        atok = p.ans_tokens + tok0;
        const int total = p.ans_off[a0 + n_ans] - tok0;
        for (int i = tid; i < total && i < AH_TOK_CAP; i += AH_THREADS) s_tok[i] = atok[i];
        for (int a = tid; a < n_ans; a += AH_THREADS) {
            const int o0 = p.ans_off[a0 + a] - tok0, o1 = p.ans_off[a0 + a + 1] - tok0;
            const bool staged = a < AH_ANS_CAP && o1 <= AH_TOK_CAP;            // offsets are monotone: the staged answers are a prefix
            if (a < AH_ANS_CAP) {
                s_off[a] = o0;
                s_off[a + 1] = o1;                                             // (answer a + 1 writes the same value)
            }
            if (staged) atomicAdd(&s_nstaged, 1);
            if (o1 == o0) {
                atomicMin(&s_empty, a);
            } else {
                const unsigned first = atok[o0];
                atomicOr(&s_bits[first >> 5], 1u << (first & 31));
                if (staged) s_next[a] = atomicExch(&s_head[head_of(first)], a);
            }
        }
    }
    __syncthreads();
    const int n_staged = s_nstaged, empty = s_empty;
    uint16_t *win = s_win[wave];

    const int j_end = min(p.k, (grp + 1) * AH_SLOTS_PER_WG);
    for (int j = grp * AH_SLOTS_PER_WG + wave; j < j_end; j += AH_WAVES) {
        const long long out = (long long)b * p.k + j;
        const int d = p.doc_ids[out];
        unsigned long long best = AH_NONE;
        if (d > 0 && (long long)d <= p.n_docs && n_ans > 0) {
            const long long pb = p.passage_off[d - 1];
            const int L = (int)(p.passage_off[d] - pb);
            const uint16_t *g = p.passage_tokens + pb;
            const int last = empty != 0x7FFFFFFF ? L : L - 1;                  // a zero-length answer may occur at position L itself
            for (int wb = 0; wb <= last; wb += AH_WINDOW) {
                const int staged_toks = min(L - wb, AH_WINDOW + AH_OVERLAP);
                __builtin_amdgcn_wave_barrier();                               // (the previous window's reads stay ahead of these writes)
                for (int i = lane; i < staged_toks; i += 64) win[i] = g[wb + i];
                __builtin_amdgcn_wave_barrier();
                // passage token at q < L: from the window when it is there
                auto ptok = [&](int q) -> unsigned { const int r = q - wb; return r < staged_toks ? win[r] : g[q]; };
                auto word_end = [&](int q) -> bool {
                    if (q == L || p.cont_bits == nullptr) return true;
                    const unsigned t = ptok(q);
                    return !((p.cont_bits[t >> 5] >> (t & 31)) & 1u);
                };
                for (int r = 0; r < AH_WINDOW / 64 && best == AH_NONE; ++r) {
                    const int pos = wb + r * 64 + lane;
                    if (pos > last) break;
                    int found = 0x7FFFFFFF;
                    if (pos < L) {
                        const unsigned t = win[pos - wb];
                        if ((s_bits[t >> 5] >> (t & 31)) & 1u) {
                            for (int a = s_head[head_of(t)]; a >= 0; a = s_next[a]) {       // staged answers that may start with t
                                const int o = s_off[a], m = s_off[a + 1] - o;
                                if (a >= found || s_tok[o] != t || pos + m > L) continue;
                                int i = 1;
                                while (i < m && ptok(pos + i) == s_tok[o + i]) ++i;
                                if (i == m && word_end(pos + m)) found = a;
                            }
                            for (int a = n_staged; a < n_ans && a < found; ++a) {           // the answers LDS has no room for
                                const int o = p.ans_off[a0 + a], m = p.ans_off[a0 + a + 1] - o;
                                if (m == 0 || p.ans_tokens[o] != t || pos + m > L) continue;
                                int i = 1;
                                while (i < m && ptok(pos + i) == p.ans_tokens[o + i]) ++i;
                                if (i == m && word_end(pos + m)) found = a;
                            }
                        }
                    }
                    if (empty < found && word_end(pos)) found = empty;
                    if (found != 0x7FFFFFFF) best = ((unsigned long long)(unsigned)pos << 32) | (unsigned)found;
                }
                if (__ballot(best != AH_NONE)) break;                          // windows run in order: the first one with a hit holds the earliest
            }
            for (int o = 32; o >= 1; o >>= 1) {
                const unsigned long long other = __shfl_xor(best, o, 64);
                best = other < best ? other : best;
            }
        }
        if (lane == 0) {
            p.hit_pos[out] = best == AH_NONE ? -1 : (int)(best >> 32);
            p.hit_ans[out] = best == AH_NONE ? -1 : (int)(best & 0xFFFFFFFFu);
        }
    }
}

__global__ void __launch_bounds__(AH_THREADS) best_kernel(const int32_t *hit_pos, int n_b, int k, int32_t *best_slot, int64_t *slot_hist)
{
    const int lane = threadIdx.x & 63, b = blockIdx.x * AH_WAVES + (threadIdx.x >> 6);
    if (b >= n_b) return;
    int best = k;
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int j = j0 + lane;
        const unsigned long long mask = __ballot(j < k && hit_pos[(long long)b * k + j] >= 0);
        if (mask) { best = j0 + __ffsll((long long)mask) - 1; break; }
    }
    if (lane == 0) {
        best_slot[b] = best;
        if (slot_hist) atomicAdd((unsigned long long *)&slot_hist[best], 1ull);
    }
}

} // namespace

extern "C" int emdr2_answer_hits(const emdr2_evidence_arena *arena, const int32_t *doc_ids, int n_b, int k, const uint16_t *ans_tokens,
                                 const int32_t *ans_off, const int32_t *q_ans_off, const uint32_t *cont_bits, int32_t *hit_pos,
                                 int32_t *hit_ans, int32_t *best_slot, int64_t *slot_hist, void *stream)
{
    if (!arena || !doc_ids || !ans_tokens || !ans_off || !q_ans_off || !hit_pos || !hit_ans || !best_slot) return -1;
    if (!arena->passage_tokens || !arena->passage_off) return -1;
    if (n_b < 1 || k < 1) return -1;
    HitParams p;
    p.passage_tokens = arena->passage_tokens; p.passage_off = arena->passage_off; p.n_docs = arena->n_docs;
    p.doc_ids = doc_ids; p.ans_tokens = ans_tokens; p.ans_off = ans_off; p.q_ans_off = q_ans_off; p.cont_bits = cont_bits;
    p.hit_pos = hit_pos; p.hit_ans = hit_ans;
    p.n_b = n_b; p.k = k; p.groups = (k + AH_SLOTS_PER_WG - 1) / AH_SLOTS_PER_WG;
    if ((long long)n_b * p.groups > 0x7FFFFFFFll) return -1;
    hipLaunchKernelGGL(hits_kernel, dim3((unsigned)(n_b * p.groups)), dim3(AH_THREADS), 0, (hipStream_t)stream, p);
    if (const int rc = LAUNCH_OK()) return rc;
    hipLaunchKernelGGL(best_kernel, dim3((unsigned)((n_b + AH_WAVES - 1) / AH_WAVES)), dim3(AH_THREADS), 0, (hipStream_t)stream,
                       (const int32_t *)hit_pos, n_b, k, best_slot, slot_hist);
    return LAUNCH_OK();
}
