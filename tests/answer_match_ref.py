"""Shared by tests/test_answer_match_cpu.py, tests/test_answer_hits_gpu.py and tests/test_answer_hits_task_gpu.py (no test functions here).

A numpy restatement of the matching rule of include/emdr2_answers.h, all four outputs:

  answer a (m >= 0 tokens) occurs at position p of a passage t[0..L)  iff  p + m <= L, t[p + i] == a[i] for all i < m, and
  (word-end rule) p + m == L or t[p + m] is not a continuation piece.
  hit_pos = the smallest such p over the question's answers, hit_ans = the lowest-numbered answer occurring there (-1, -1: none);
  a doc id <= 0 or > n_docs is never a hit; best_slot = the smallest slot with a hit, k if none; slot_hist[best_slot] += 1.

It restates the RULE, not the kernel: whole-passage array comparisons, no windows, no bitset, no capacities.  Also here: the two
vocabularies the fixture agreement is checked under, and the seeded random ASCII corpus of the `has_answer` agreement."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")
CJK_CASE = "東京"                                  # the one fixture case on which the two matchers differ (see the header)


def cont_flags(tokens, cont_bits):
    """bool per token: is it a continuation piece (all False when cont_bits is None: no word-end rule)."""
    t = np.asarray(tokens, dtype=np.int64)
    if cont_bits is None:
        return np.zeros(t.shape, dtype=bool)
    return ((np.asarray(cont_bits, dtype=np.uint32)[t >> 5] >> (t & 31).astype(np.uint32)) & 1).astype(bool)


def occurrences(t, a, cont_bits=None):
    """Ascending positions at which answer `a` occurs in passage `t`."""
    t, a = np.asarray(t, dtype=np.int64), np.asarray(a, dtype=np.int64)
    L, m = len(t), len(a)
    if m > L:
        return np.zeros(0, dtype=np.int64)
    ok = np.ones(L - m + 1, dtype=bool)
    for i in range(m):
        ok &= t[i:L - m + 1 + i] == a[i]
    ok[:L - m] &= ~cont_flags(t[m:], cont_bits)                              # position L - m ends the passage: always a word end
    return np.nonzero(ok)[0]


def first_hit(t, answers, cont_bits=None):
    """(hit_pos, hit_ans) of one passage against one question's answers (a list of token sequences)."""
    best = (-1, -1)
    for ai, a in enumerate(answers):
        occ = occurrences(t, a, cont_bits)
        if occ.size and (best[0] < 0 or int(occ[0]) < best[0]):              # a later answer wins only with a strictly smaller position
            best = (int(occ[0]), ai)
    return best


def question_answers(ans_tokens, ans_off, q_ans_off, b):
    return [np.asarray(ans_tokens[ans_off[a]:ans_off[a + 1]], dtype=np.int64) for a in range(int(q_ans_off[b]), int(q_ans_off[b + 1]))]


def answer_hits(passage_tokens, passage_off, n_docs, doc_ids, ans_tokens, ans_off, q_ans_off, cont_bits=None):
    """-> hit_pos [B, K] int32, hit_ans [B, K] int32, best_slot [B] int32, hist [K + 1] int64 (what the call ADDS to slot_hist)."""
    doc_ids = np.asarray(doc_ids)
    B, K = doc_ids.shape
    ptok = np.asarray(passage_tokens).view(np.uint16) if np.asarray(passage_tokens).dtype == np.int16 else np.asarray(passage_tokens)
    hit_pos = np.full((B, K), -1, dtype=np.int32)
    hit_ans = np.full((B, K), -1, dtype=np.int32)
    best = np.full(B, K, dtype=np.int32)
    hist = np.zeros(K + 1, dtype=np.int64)
    for b in range(B):
        answers = question_answers(ans_tokens, ans_off, q_ans_off, b)
        seen = {}
        for j in range(K):
            d = int(doc_ids[b, j])
            if 0 < d <= n_docs:
                if d not in seen:
                    seen[d] = first_hit(ptok[int(passage_off[d - 1]):int(passage_off[d])], answers, cont_bits)
                hit_pos[b, j], hit_ans[b, j] = seen[d]
        found = np.nonzero(hit_pos[b] >= 0)[0]
        if found.size:
            best[b] = found[0]
        hist[best[b]] += 1
    return hit_pos, hit_ans, best, hist


def lay_out(passages):
    """passages: list of token sequences -> (tokens uint16, offsets int64), doc d = passages[d - 1]."""
    off = np.zeros(len(passages) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in passages])
    tok = np.zeros(int(off[-1]), dtype=np.uint16)
    for d, p in enumerate(passages):
        tok[off[d]:off[d + 1]] = p
    return tok, off


def pack_token_answers(answer_lists):
    """answer_lists: per question a list of token sequences -> (tokens uint16, ans_off int32, q_ans_off int32)."""
    tokens, ans_off, q_ans_off = [], [0], [0]
    for answers in answer_lists:
        for a in answers:
            tokens.extend(int(x) for x in a)
            ans_off.append(len(tokens))
        q_ans_off.append(len(ans_off) - 1)
    return np.asarray(tokens, dtype=np.uint16), np.asarray(ans_off, dtype=np.int32), np.asarray(q_ans_off, dtype=np.int32)


# ---- vocabularies ------------------------------------------------------------------------------------------------------------------------
def basic_words(texts):
    """Every word BERT's basic tokenizer (lower-casing, accent stripping, punctuation and CJK splitting) makes of `texts`, first-seen order."""
    from emdr2_amd.tokenizer import BasicTokenizer
    basic, words = BasicTokenizer(True), []
    for text in texts:
        for w in basic.tokenize(text):
            if w not in words:
                words.append(w)
    return words


def write_vocab(path, words, pieces):
    """pieces False: every word is one vocabulary entry.  True: single characters and `##` characters only, so that every word of two or
    more characters is split into pieces."""
    entries = list(SPECIALS)
    if pieces:
        chars = sorted({c for w in words for c in w})
        entries += chars + ["##" + c for c in chars]
    else:
        entries += list(words)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(entries) + "\n")
    return path


def tokenizer_for(tmp, texts, pieces):
    from emdr2_amd.tokenizer import BertWordPieceTokenizer
    return BertWordPieceTokenizer(write_vocab(os.path.join(str(tmp), "vocab_%s.txt" % ("pieces" if pieces else "words")), basic_words(texts), pieces))


def token_has_answer(answers, text, tokenizer):
    """The rule applied to strings: does any answer occur in `text` (answers holding [UNK] left out, as the packer does)."""
    from emdr2_amd.data.answer_match import continuation_bits, pack_answers
    pack = pack_answers([answers], tokenizer)
    got = first_hit(tokenizer.tokenize(text), question_answers(pack.tokens, pack.ans_off, pack.q_ans_off, 0), continuation_bits(tokenizer))
    return got[0] >= 0


# ---- the random ASCII corpus of the `has_answer` agreement ------------------------------------------------------------------------------
def ascii_corpus(words, seed=7, n_passages=400, n_glued=100, n_sets=60):
    """(passages, answer sets): passages of 12-30 words from `words`; in the first `n_glued`, a few neighbouring words are glued together
    (an answer inside a glued word must not match: the word-end rule and the `##` ids); answer sets of 1-3 answers of 1-3 words."""
    rng = np.random.default_rng(seed)
    passages = []
    for i in range(n_passages):
        ws = [str(w) for w in rng.choice(words, size=int(rng.integers(12, 31)))]
        if i < n_glued:
            for _ in range(3):
                at = int(rng.integers(0, len(ws) - 1))
                ws[at:at + 2] = [ws[at] + ws[at + 1]]
        passages.append(" ".join(ws))
    sets = [[" ".join(str(w) for w in rng.choice(words, size=int(rng.integers(1, 4)))) for _ in range(int(rng.integers(1, 4)))]
            for _ in range(n_sets)]
    return passages, sets
