/*
 * include/emdr2_answers.h -- C ABI of the answer-hit kernel: which retrieved passages hold a reference answer (libemdr2_hip.so).
 *
 * Replaces, in one launch pair on the device and on the token ids already resident in HBM, the host validation of the reference:
 *   has_answer (match_type 'string') + SimpleTokenizer           tasks/openqa/dense_retriever/evaluation/qa_validation.py:98-125
 *       (regex tokenisation of every retrieved passage's text, one Python list comparison per start position and answer)
 *   check_answer / calculate_matches (top_k_hits)                 tasks/openqa/dense_retriever/evaluation/qa_validation.py:29-95
 *       (a process pool over the questions; needs the evidence text on the host)
 * Integer work only: results are the same bits whatever the launch geometry or the order of the histogram's atomic additions.
 *
 * The matching rule.  Passages are BERT WordPiece ids (lower-cased, accent-stripped) as the evidence arena stores them; answers are
 * tokenised by the same tokenizer.  Answer a (m >= 0 tokens) OCCURS AT position p of a passage t[0..L) iff
 *     p + m <= L  and  t[p + i] == a[i] for all i < m,                                   and
 *     p + m == L  or   t[p + m] is not a continuation piece (a vocabulary entry starting with "##")          -- the word-end rule.
 * No start rule is needed: an answer's first piece is word-initial, and a word-internal occurrence is a different id.
 * Where this differs from the reference's matcher (the only known differences):
 *   CJK        BERT's basic tokenizer isolates every CJK ideograph, the reference's regex takes a run of them as one word: an answer
 *              that is part of a longer CJK run matches here and not there (tests/golden/retrieval_ref.json, the one such case).
 *   [UNK]      an answer whose tokenisation holds [UNK] could match any unknown word: the host packer leaves such answers out
 *              (emdr2_amd/data/answer_match.py); the kernel knows nothing of [UNK].
 * A zero-length answer occurs at the first position the word-end rule admits: position 0 of every passage that starts with a
 * word-initial piece -- an empty passage included -- as `a == words[i:i+0]` does in the reference.
 *
 * Same conventions as emdr2_mips.h: device pointers, caller-owned buffers, nothing allocated, no host synchronisation, int status,
 * enqueue on stream.
 */
#ifndef EMDR2_ANSWERS_H
#define EMDR2_ANSWERS_H
#include <stdint.h>
#include "emdr2_assembly.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * arena       only passage_tokens, passage_off and n_docs are read; the other tables may be null
 * doc_ids     device int32 [n_b, k]      1-based doc ids, e.g. kept_ids of emdr2_assemble_evidence.  An id <= 0 or > n_docs is never a
 *                                        hit and no table is read for it.
 * ans_tokens  device uint16, ans_off device int32: answer a = ans_tokens[ans_off[a] .. ans_off[a + 1])
 * q_ans_off   device int32 [n_b + 1]     question b owns the answers q_ans_off[b] .. q_ans_off[b + 1)
 * cont_bits   device uint32 [2048]       bit t (word t >> 5, bit t & 31) set = token t is a continuation piece; NULL = no word-end rule
 * hit_pos     device int32 [n_b, k]      the smallest position at which any of the question's answers occurs in the slot's passage
 * hit_ans     device int32 [n_b, k]      the lowest-numbered answer (index within the question's own answers) occurring there;
 *                                        both are -1 when there is no hit
 * best_slot   device int32 [n_b]         the smallest slot with a hit, k when there is none
 * slot_hist   device int64 [k + 1]       slot_hist[best_slot[b]] += 1 for every question (added INTO: the reference's top_k_hits[i] is
 *                                        the prefix sum of bins 0..i); NULL = not wanted
 *
 * Returns -1 before any launch for a null required pointer (cont_bits and slot_hist are the optional ones; passage_tokens and
 * passage_off inside *arena are required), n_b < 1 or k < 1; -3 when a launch fails.  Every word of hit_pos, hit_ans and best_slot is
 * written, and nothing else except the slot_hist additions.
 *
 * Caller obligations, NOT checked on the device: q_ans_off and ans_off are monotone and lie inside their tables (ans_off has
 * q_ans_off[n_b] + 1 entries); the arena's passage offsets are monotone, lie inside passage_tokens, and no passage is 2^31 tokens long.
 */
int emdr2_answer_hits(const emdr2_evidence_arena *arena, const int32_t *doc_ids, int n_b, int k,
                      const uint16_t *ans_tokens, const int32_t *ans_off, const int32_t *q_ans_off, const uint32_t *cont_bits,
                      int32_t *hit_pos, int32_t *hit_ans, int32_t *best_slot, int64_t *slot_hist, void *stream);

#ifdef __cplusplus
}
#endif
#endif
