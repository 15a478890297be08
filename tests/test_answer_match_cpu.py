"""CPU: the matching rule of include/emdr2_answers.h, restated in numpy (tests/answer_match_ref.py), against the reference's own results
(tests/golden/retrieval_ref.json) and against the host string matcher `qa_validation.has_answer`; the host side of the feature
(`pack_answers`, `continuation_bits`, `HitMeter`); the argument refusals of the C entry; and the kernel's window / capacity constants,
read from the source so that tests/test_answer_hits_gpu.py can be seen to cross them."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import answer_match_ref as ar
from tests.test_task_gpu import WORDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = json.load(open(os.path.join(ar.GOLD, "retrieval_ref.json"), encoding="utf-8"))
STRING_CASES = [c for c in REF["cases"] if c[2] == "string"]


def source_constants():
    """The #define AH_* integers of csrc/answer_match.hip."""
    text = open(os.path.join(ROOT, "emdr2_amd", "csrc", "answer_match.hip")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (AH_[A-Z_]+) (\d+)\b", text, flags=re.M)}


def _fixture_texts():
    texts = [t for answers, text, _, _ in STRING_CASES for t in answers + [text]]
    texts += [d[0] for d in REF["docs"].values()] + [a for q in REF["questions"] for a in q[0]]
    return texts


@pytest.mark.parametrize("pieces", [False, True], ids=["whole-word vocabulary", "single-character pieces"])
def test_restatement_agrees_with_the_reference_fixture_except_on_the_cjk_case(tmp_path, pieces):
    assert len(STRING_CASES) == 10
    tok = ar.tokenizer_for(tmp_path, _fixture_texts(), pieces)
    if pieces:                                                           # every longer word really is split, and `##` pieces are flagged
        from emdr2_amd.data.answer_match import continuation_bits
        assert len(tok.tokenize("paris")) == 5 and ar.cont_flags(tok.tokenize("paris"), continuation_bits(tok)).tolist() == [False] + [True] * 4
    differ = [answers for answers, text, _, expect in STRING_CASES if ar.token_has_answer(answers, text, tok) != expect]
    assert differ == [[ar.CJK_CASE]]                                     # the only exclusion: a CJK run is one word to the reference's regex
    # the questions of the fixture: per-document hits and top_k_hits
    from emdr2_amd.data.answer_match import continuation_bits, pack_answers
    passages = [tok.tokenize(REF["docs"][str(d)][0]) for d in range(1, 5)]
    ptok, poff = ar.lay_out(passages)
    pack = pack_answers([q[0] for q in REF["questions"]], tok)
    ids = np.asarray([q[1] for q in REF["questions"]], dtype=np.int32)
    hit_pos, _, best, hist = ar.answer_hits(ptok, poff, 4, ids, pack.tokens, pack.ans_off, pack.q_ans_off, continuation_bits(tok))
    assert (hit_pos >= 0).tolist() == REF["questions_doc_hits"]
    assert np.cumsum(hist)[:3].tolist() == REF["top_k_hits"] == [1, 2, 2] and best.tolist() == [1, 0, 3]


@pytest.mark.parametrize("pieces", [False, True], ids=["whole-word vocabulary", "single-character pieces"])
def test_restatement_agrees_with_has_answer_on_a_random_ascii_corpus(tmp_path, pieces):
    from emdr2_amd.tasks.openqa.dense_retriever.evaluation.qa_validation import has_answer
    passages, sets = ar.ascii_corpus(WORDS)
    assert len(passages) == 400 and len(sets) == 60
    tok = ar.tokenizer_for(tmp_path, WORDS, pieces)
    from emdr2_amd.data.answer_match import continuation_bits, pack_answers
    cont = continuation_bits(tok)
    ptoks = [np.asarray(tok.tokenize(p)) for p in passages]
    hits = disagreements = 0
    for answers in sets:
        pack = pack_answers([answers], tok)
        assert pack.dropped == 0
        qa = ar.question_answers(pack.tokens, pack.ans_off, pack.q_ans_off, 0)
        for text, t in zip(passages, ptoks):
            mine, theirs = ar.first_hit(t, qa, cont)[0] >= 0, has_answer(answers, text)
            hits += theirs
            disagreements += mine != theirs
    assert disagreements == 0 and 2000 < hits < 12000                    # 24,000 pairs, both outcomes well represented


def test_pack_answers_drops_unk_keeps_empty_answers_and_refuses_wide_ids(tmp_path):
    from emdr2_amd.data.answer_match import pack_answers
    tok = ar.tokenizer_for(tmp_path, ["paris france", "rome"], pieces=False)
    v = tok.vocab
    pack = pack_answers([["paris", "berlin", "", "rome"], [], ["berlin wall"], ["paris france"]], tok)
    assert pack.dropped == 2                                             # "berlin", "berlin wall": [UNK]
    assert pack.q_ans_off.tolist() == [0, 3, 3, 3, 4] and pack.orig.tolist() == [0, 2, 3, 0]
    assert pack.ans_off.tolist() == [0, 1, 1, 2, 4]                      # the empty answer is kept, with no tokens
    assert pack.tokens.tolist() == [v["paris"], v["rome"], v["paris"], v["france"]]
    assert (pack.tokens.dtype, pack.ans_off.dtype, pack.q_ans_off.dtype, pack.orig.dtype) == (np.uint16, np.int32, np.int32, np.int32)

    class Wide(object):
        vocab = {"[UNK]": 1}

        def tokenize(self, text):
            return [5, 65536]
    with pytest.raises(ValueError):
        pack_answers([["x"]], Wide())


def test_continuation_bits_flag_exactly_the_double_hash_entries(tmp_path):
    from emdr2_amd.data.answer_match import continuation_bits
    tok = ar.tokenizer_for(tmp_path, ["ab"], pieces=True)
    bits = continuation_bits(tok)
    assert bits.dtype == np.uint32 and bits.shape == (2048,)
    flagged = {i for i in range(65536) if (int(bits[i >> 5]) >> (i & 31)) & 1}
    assert flagged == {i for i, t in tok.inv_vocab.items() if t.startswith("##")} == {tok.vocab["##a"], tok.vocab["##b"]}

    class High(object):
        inv_vocab = {31: "##x", 32: "y", 32768: "##z", 65535: "##w", 65536: "##beyond", 7: "#"}
    bits = continuation_bits(High())
    assert {i for i in range(65536) if (int(bits[i >> 5]) >> (i & 31)) & 1} == {31, 32768, 65535}


def test_hit_meter_reports_the_prefix_sums_calculate_matches_reports():
    from emdr2_amd.data.answer_match import HitMeter
    from emdr2_amd.tasks.openqa.dense_retriever.evaluation.qa_validation import calculate_matches
    docs = {int(k): tuple(v) for k, v in REF["docs"].items()}
    stats = calculate_matches(docs, [q[0] for q in REF["questions"]], [(q[1], q[2]) for q in REF["questions"]], match_type="string")
    best = [next((i for i, x in enumerate(h) if x), 3) for h in stats.questions_doc_hits]
    meter = HitMeter(3)
    meter.update(torch.tensor(best[:2], dtype=torch.int32))
    meter.update(torch.tensor(best[2:], dtype=torch.int32))
    rep = meter.report((1, 2, 3, 7))
    assert [rep[1], rep[2], rep[3]] == stats.top_k_hits == [1, 2, 2] and rep[7] == rep[3] and rep["total"] == 3
    assert int(meter.hist.sum()) == 0 and meter.count == 0               # a report starts the meter again
    meter.hist[1] += 2                                                   # what a kernel launch with hist=meter.hist leaves behind
    meter.update(n=2)
    assert meter.report((1, 2)) == {1: 0, 2: 2, "total": 2}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    return _native.lib()


def test_answer_hits_refuses_bad_arguments_before_any_launch(lib):
    from emdr2_amd import _native
    one = ctypes.c_void_p(4096)
    arena = _native.EvidenceArenaStruct()
    arena.passage_tokens = arena.passage_off = 4096                      # the other tables may be null
    arena.n_docs = 10

    def call(arena_p=ctypes.byref(arena), req=(one,) * 7, cont=None, hist=None, n_b=2, k=3):
        ids, atok, aoff, qoff, pos, ans, best = req
        return lib.emdr2_answer_hits(arena_p, ids, n_b, k, atok, aoff, qoff, cont, pos, ans, best, hist, None)
    assert call(arena_p=None) == -1
    for i in range(7):                                                   # doc_ids, ans_tokens, ans_off, q_ans_off, hit_pos, hit_ans, best_slot
        assert call(req=tuple(None if j == i else one for j in range(7))) == -1, i
    assert call(n_b=0) == -1 and call(n_b=-2) == -1 and call(k=0) == -1 and call(k=-1) == -1
    for t in ("passage_tokens", "passage_off"):
        setattr(arena, t, None)
        assert call() == -1, t
        setattr(arena, t, 4096)
    # both optional pointers null pass validation: with every required pointer in place, the only refusals left are the shape ones
    assert call(cont=None, hist=None, k=0) == -1 and call(cont=one, hist=one, k=0) == -1


def test_the_product_path_has_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from emdr2_amd import _native
    from emdr2_amd.data.answer_match import AnswerMatcher
    from emdr2_amd.data.evidence_arena import EvidenceArena
    with pytest.raises(_native.NativeError):
        AnswerMatcher(EvidenceArena([[5, 6]], [[7]]), None)


def test_source_constants_are_the_ones_the_gpu_sizes_cross():
    c = source_constants()
    assert set(c) >= {"AH_WINDOW", "AH_OVERLAP", "AH_TOK_CAP", "AH_ANS_CAP", "AH_SLOTS_PER_WG", "AH_WAVES", "AH_THREADS"}
    assert c["AH_THREADS"] == 64 * c["AH_WAVES"] and c["AH_WINDOW"] % 64 == 0 and c["AH_OVERLAP"] >= 1
    # what tests/test_answer_hits_gpu.py relies on: its passage lengths reach past two windows, its longest answer does not fit the
    # overlap, 300 answers exceed the staged answers, and 120 slots need more than one workgroup per question
    assert 300 > c["AH_ANS_CAP"] and 120 > c["AH_SLOTS_PER_WG"] and c["AH_WINDOW"] >= 129
    assert c["AH_TOK_CAP"] < 300 * 8
