"""GPU: emdr2_answer_hits (csrc/answer_match.hip, include/emdr2_answers.h) bit for bit against the numpy restatement of its rule
(tests/answer_match_ref.py), through the C ABI: all four outputs, pre-filled with a sentinel and embedded in larger buffers whose guard
words must stay intact.  Sizes are the smallest at which each path of the kernel changes: the staging window and its overlap, the LDS
capacities for answers and answer tokens, the slots one workgroup serves (constants read from the source by
tests/test_answer_match_cpu.py::source_constants)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import answer_match_ref as ar
from tests.test_answer_match_cpu import REF, STRING_CASES, _fixture_texts, source_constants
from tests.test_task_gpu import WORDS

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 16, -77
C = source_constants()
W, OV = C["AH_WINDOW"], C["AH_OVERLAP"]
PLENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, W - 1, W, W + 1, 2 * W + 3)
ALENS = (1, 2, 3, 7, OV + 2)                              # the last: too long to be verified inside one staged window from every start


def _guarded(shape, dtype, fill):
    """(whole buffer, the view handed to the kernel): GUARD words of `fill` on either side."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(shape)


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, dtype=a.dtype)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view is not None else a).cuda()


def run_abi(ptok, poff, n_docs, doc_ids, atok, aoff, qoff, cont=None, hist0=None, want_hist=True, calls=1):
    """One (or `calls`) launches through the C ABI -> hit_pos, hit_ans, best_slot, hist (numpy); guards and untouched inputs asserted."""
    from emdr2_amd import _native
    lib = _native.lib()
    doc_ids = np.ascontiguousarray(doc_ids, dtype=np.int32)
    B, K = doc_ids.shape
    arena = _native.EvidenceArenaStruct()                  # only passage_tokens, passage_off and n_docs: the other tables stay null
    d_ptok, d_poff = _dev(ptok), _dev(poff)
    arena.passage_tokens, arena.passage_off, arena.n_docs = d_ptok.data_ptr(), d_poff.data_ptr(), n_docs
    d_ids, d_atok, d_aoff, d_qoff = _dev(doc_ids), _dev(atok), _dev(aoff), _dev(qoff)
    d_cont = _dev(cont) if cont is not None else None
    w_pos, pos = _guarded((B, K), torch.int32, SENTINEL)
    w_ans, ans = _guarded((B, K), torch.int32, SENTINEL)
    w_best, best = _guarded((B,), torch.int32, SENTINEL)
    w_hist, hist = _guarded((K + 1,), torch.int64, SENTINEL)
    hist.copy_(torch.from_numpy(np.asarray(hist0 if hist0 is not None else np.zeros(K + 1), dtype=np.int64)))
    for _ in range(calls):
        rc = lib.emdr2_answer_hits(ctypes.byref(arena), d_ids.data_ptr(), B, K, d_atok.data_ptr(), d_aoff.data_ptr(), d_qoff.data_ptr(),
                                   d_cont.data_ptr() if d_cont is not None else None, pos.data_ptr(), ans.data_ptr(), best.data_ptr(),
                                   hist.data_ptr() if want_hist else None, _native.stream_ptr())
        assert rc == 0
    torch.cuda.synchronize()
    for whole, n in ((w_pos, B * K), (w_ans, B * K), (w_best, B), (w_hist, K + 1)):
        g = torch.cat([whole[:GUARD], whole[GUARD + n:]]).cpu().numpy()
        assert (g == SENTINEL).all(), "a guard word was written"
    assert np.array_equal(d_ids.cpu().numpy(), doc_ids)
    return pos.cpu().numpy(), ans.cpu().numpy(), best.cpu().numpy(), hist.cpu().numpy()


def check(passages, doc_ids, answer_lists, cont=None, hist0=None):
    """Kernel == restatement on all four outputs; -> (hit_pos, hit_ans, best_slot) for the case's own assertions."""
    ptok, poff = ar.lay_out(passages)
    atok, aoff, qoff = ar.pack_token_answers(answer_lists)
    doc_ids = np.asarray(doc_ids, dtype=np.int32)
    K = doc_ids.shape[1]
    hist0 = np.zeros(K + 1, dtype=np.int64) if hist0 is None else np.asarray(hist0, dtype=np.int64)
    got = run_abi(ptok, poff, len(passages), doc_ids, atok, aoff, qoff, cont, hist0)
    exp = ar.answer_hits(ptok, poff, len(passages), doc_ids, atok, aoff, qoff, cont)
    for name, g, e in zip(("hit_pos", "hit_ans", "best_slot"), got, exp):
        assert g.dtype == e.dtype and np.array_equal(g, e), (name, np.argwhere(g != e)[:5].tolist())
    assert np.array_equal(got[3], hist0 + exp[3]), "slot_hist"
    assert not (got[0] == SENTINEL).any() and not (got[2] == SENTINEL).any()          # every word written
    return got[0], got[1], got[2]


def cont_of(tokens):
    bits = np.zeros(2048, dtype=np.uint32)
    for t in tokens:
        bits[t >> 5] |= np.uint32(1 << (t & 31))
    return bits


# ---- the length and position sweep --------------------------------------------------------------------------------------------------------
def sweep(alphabet, seed):
    """One question per answer length (several rows of 64 slots each); one document per (passage length, planted position): position 0,
    the last possible one, every start from which the answer (or the token behind it) straddles a window boundary, and absent.
    alphabet None: filler tokens disjoint from the answers' (the answer occurs exactly where it was planted); else filler AND answers
    are drawn from `alphabet`, so self-overlaps and further occurrences arise and only the restatement knows the result.
    -> passages, doc_ids [B, 64], answer_lists, planted [B, 64] (position, -1 absent, -2 empty slot)"""
    rng = np.random.default_rng(seed)
    passages, rows, answer_lists, planted = [], [], [], []
    for m in ALENS:
        answer = (1000 + 100 * ALENS.index(m) + np.arange(m)).tolist() if alphabet is None else rng.choice(alphabet, size=m).tolist()
        docs = []
        for L in PLENS:
            fill = (lambda n: rng.integers(3000, 60000, size=n).tolist()) if alphabet is None else (lambda n: rng.choice(alphabet, size=n).tolist())
            starts = {-1}
            if m <= L:
                starts |= {0, L - m}
                for edge in (W, 2 * W):                                       # tokens p .. p + m (the word-end token included) cross `edge`
                    starts |= {p for p in range(edge - m - 1, edge + 1) if 0 <= p <= L - m}
            for p in sorted(starts):
                t = fill(L)
                if p >= 0:
                    t[p:p + m] = answer
                passages.append(t)
                docs.append((len(passages), p))
        for at in range(0, len(docs), 64):
            chunk = docs[at:at + 64]
            rows.append([d for d, _ in chunk] + [0] * (64 - len(chunk)))
            planted.append([p for _, p in chunk] + [-2] * (64 - len(chunk)))
            answer_lists.append([answer])
    return passages, np.asarray(rows, dtype=np.int32), answer_lists, np.asarray(planted)


def test_sweep_of_passage_lengths_answer_lengths_and_planted_positions():
    passages, ids, answers, planted = sweep(None, 11)
    assert max(len(p) for p in passages) == 2 * W + 3 and (planted >= W - 1).any() and ids.shape[0] > len(ALENS)
    hit_pos, hit_ans, _ = check(passages, ids, answers)
    assert np.array_equal(hit_pos, np.where(planted >= 0, planted, -1))      # disjoint alphabets: found exactly where planted, nowhere else
    assert np.array_equal(hit_ans, np.where(planted >= 0, 0, -1))


def test_sweep_on_a_four_token_alphabet_with_the_word_end_rule():
    alphabet = [40000, 7, 32768, 65535]
    passages, ids, answers, planted = sweep(alphabet, 12)
    hit_pos, _, _ = check(passages, ids, answers, cont=cont_of([65535]))
    pairs = planted > -2
    rate = float((hit_pos[pairs] >= 0).mean())
    assert 0.10 <= rate <= 0.90, rate                                        # neither outcome goes untested
    assert (hit_pos[planted >= 0] != planted[planted >= 0]).any()            # earlier occurrences / rejected plants do arise


def test_self_overlapping_patterns():
    a, b = 50, 60
    hit_pos, _, _ = check([[a, a, a, b], [a, b, a, b, a, b], [a, a, b, a, a, a, b]], [[1, 2, 3], [1, 2, 3]], [[[a, a, b]], [[a, b, a, b]]])
    assert hit_pos.tolist() == [[1, -1, 0], [-1, 0, -1]]


# ---- the word-end rule ----------------------------------------------------------------------------------------------------------------------
def test_word_end_rule():
    x, y, c, f = 900, 901, 950, 500                                          # c: a continuation piece
    passages = [[f, x, y, c, f, x, y, f],                                    # rejected at 1 (followed by ##), clean at 5
                [f, f, x, y],                                                # ends the passage
                [x, y, c],                                                   # only a rejected occurrence
                [f, 32768, 65535, f, 32768, f]]
    ids = [[1, 2, 3, 4]]
    hit_pos, _, _ = check(passages, ids, [[[x, y]]], cont=cont_of([c]))
    assert hit_pos.tolist() == [[5, 2, -1, -1]]
    hit_pos, _, _ = check(passages, ids, [[[x, y]]], cont=None)              # no rule: the first occurrence
    assert hit_pos.tolist() == [[1, 2, 0, -1]]
    # ids 32768 and 65535 (uint16 kept in int16 tensors), with and without their bit
    for flagged, expect in (([], 1), ([65535], 4), ([32768], 1), ([32768, 65535], 4)):
        hit_pos, _, _ = check(passages, ids, [[[32768]]], cont=cont_of(flagged))
        assert hit_pos[0, 3] == expect, flagged
    hit_pos, _, _ = check(passages, ids, [[[32768, 65535]]], cont=cont_of([65535, f]))
    assert hit_pos[0, 3] == -1                                               # followed by f, flagged here
    hit_pos, _, _ = check(passages, ids * 2, [[[32768, 65535]], [[65535]]], cont=cont_of([32768]))
    assert hit_pos[:, 3].tolist() == [1, 2]


# ---- answer sets ----------------------------------------------------------------------------------------------------------------------------
def test_answer_sets_of_0_1_2_33_and_300_answers_and_past_the_token_capacity():
    rng = np.random.default_rng(5)
    alphabet = np.arange(100, 130)
    passages = [rng.choice(alphabet, size=int(n)).tolist() for n in rng.integers(0, 200, size=48)]
    draw = lambda n, lo, hi: [rng.choice(alphabet, size=int(rng.integers(lo, hi + 1))).tolist() for _ in range(n)]
    long_set = draw(200, 12, 12)                                             # 2,400 tokens: the token capacity ends before the answer capacity
    assert 200 < C["AH_ANS_CAP"] < 300 and 200 * 12 > C["AH_TOK_CAP"] > 300 * 4
    for a in long_set[180:]:                                                 # some of the answers LDS has no room for do occur
        passages[int(rng.integers(0, 48))][3:15] = a
    answers = [[], draw(1, 1, 2), draw(2, 1, 3), draw(33, 2, 4), draw(300, 3, 4), long_set]
    for i, a in enumerate(answers[4][290:]):                                 # and some of the answers beyond the answer capacity
        passages[i] = passages[i] + a
    ids = np.stack([rng.permutation(48)[:40] + 1 for _ in answers])
    hit_pos, hit_ans, best = check(passages, ids, answers, cont=cont_of(alphabet[::7].tolist()))
    assert (hit_pos[0] == -1).all() and best[0] == 40
    assert (hit_ans[4] >= C["AH_ANS_CAP"]).any() and (hit_ans[5] >= 180).any() and (hit_ans[3] >= 0).any()


@pytest.mark.parametrize("n", [33, 300])
def test_answers_sharing_one_first_token_of_which_only_the_last_occurs(n):
    first, fill = 777, 5
    answers = [[first, 2000 + i, 3000 + i] for i in range(n)]
    passages = [[fill, first, fill, first, 2000 + n - 1, 3000 + n - 1, fill], [first] * 9, [fill, first, 2000, 3001]]
    hit_pos, hit_ans, _ = check(passages, [[1, 2, 3]], [answers])
    assert hit_pos.tolist() == [[3, -1, -1]] and hit_ans.tolist() == [[n - 1, -1, -1]]


def test_lowest_answer_at_the_smallest_position_prefixes_and_duplicates():
    x, y, z, f = 10, 11, 12, 99
    p = [[f, x, y, z, f], [f, f, f, x, y, f, f, f, f, f, z, z]]
    # one answer is a prefix of another at the same position: the lower index wins, whichever is longer
    _, hit_ans, _ = check(p, [[1]], [[[x, y, z], [x, y]]])
    assert hit_ans.tolist() == [[0]]
    _, hit_ans, _ = check(p, [[1]], [[[x, y], [x, y, z]]])
    assert hit_ans.tolist() == [[0]]
    # answer 5 at position 3, answer 0 at position 10
    hit_pos, hit_ans, _ = check(p, [[2]], [[[z, z], [7], [8], [9], [13], [x, y]]])
    assert (hit_pos.tolist(), hit_ans.tolist()) == ([[3]], [[5]])
    # duplicates: the first copy
    _, hit_ans, _ = check(p, [[1, 2]], [[[4], [y, z], [y, z], [y, z]]])
    assert hit_ans.tolist() == [[1, -1]]


def test_zero_length_answer_hits_every_valid_document_and_no_invalid_id():
    c, f = 70, 71
    passages = [[], [f, f, f], [c, c, f], [c, c]]                            # (a passage that starts with continuation pieces: the rule decides)
    ids = [[1, 2, 0, 3, -1, 4, 5, 2]]
    hit_pos, hit_ans, best = check(passages, ids, [[[]]], cont=cont_of([c]))
    assert hit_pos.tolist() == [[0, 0, -1, 2, -1, 2, -1, 0]] and best.tolist() == [0]
    hit_pos, hit_ans, _ = check(passages, ids, [[[f], []]], cont=None)
    assert hit_pos.tolist() == [[0, 0, -1, 0, -1, 0, -1, 0]] and hit_ans.tolist() == [[1, 0, -1, 1, -1, 1, -1, 0]]


def test_invalid_doc_ids_give_no_hit_and_a_repeated_doc_gives_equal_results():
    f, x = 30, 31
    passages = [[x], [f, x], [f, f, x]]
    ids = [[0, -1, 4, 2 ** 31 - 1, 3, 2, 3, -(2 ** 31)]]
    hit_pos, hit_ans, best = check(passages, ids, [[[x]]])
    assert hit_pos.tolist() == [[-1, -1, -1, -1, 2, 1, 2, -1]] and best.tolist() == [4]
    hit_pos, _, best = check(passages, [[0, -1, 4, 2 ** 31 - 1]], [[[x]]])
    assert (hit_pos == -1).all() and best.tolist() == [4]


# ---- launch geometry and the histogram -----------------------------------------------------------------------------------------------------
def _random_case(B, K, seed, n_docs=300):
    rng = np.random.default_rng(seed)
    alphabet = np.arange(200, 230)
    passages = [rng.choice(alphabet, size=int(n)).tolist() for n in rng.integers(0, 301, size=n_docs)]
    answers = [[rng.choice(alphabet, size=int(rng.integers(1, 4))).tolist() for _ in range(int(rng.integers(0, 6)))] for _ in range(B)]
    ids = rng.integers(-1, n_docs + 3, size=(B, K)).astype(np.int32)
    return passages, ids, answers, cont_of(alphabet[::5].tolist())


@pytest.mark.parametrize("B,K", [(1, 1), (3, 7), (70, 120)])
def test_launch_geometry(B, K):
    assert 7 < C["AH_SLOTS_PER_WG"] < 120                                    # less than one workgroup's slots, and many workgroups per question
    passages, ids, answers, cont = _random_case(B, K, 100 + B)
    hit_pos, _, best = check(passages, ids, answers, cont)
    if B > 1:
        assert (hit_pos >= 0).any() and (hit_pos < 0).any() and len(set(best.tolist())) > 1


def test_histogram_is_added_onto_what_is_there_across_calls_and_may_be_null():
    passages, ids, answers, cont = _random_case(9, 13, 3)
    ptok, poff = ar.lay_out(passages)
    atok, aoff, qoff = ar.pack_token_answers(answers)
    exp = ar.answer_hits(ptok, poff, len(passages), ids, atok, aoff, qoff, cont)
    hist0 = np.arange(14, dtype=np.int64) * 1000003 + (1 << 40)
    got = run_abi(ptok, poff, len(passages), ids, atok, aoff, qoff, cont, hist0, calls=2)
    assert np.array_equal(got[3], hist0 + 2 * exp[3]) and exp[3].sum() == 9
    got = run_abi(ptok, poff, len(passages), ids, atok, aoff, qoff, cont, hist0, want_hist=False)
    assert np.array_equal(got[3], hist0) and np.array_equal(got[2], exp[2]) and np.array_equal(got[0], exp[0])


# ---- the Python path ------------------------------------------------------------------------------------------------------------------------
class _Tok(object):
    """Token-level stand-in for the tokenizer: `tokenize` takes a space-separated id string; every third id is a continuation piece."""
    vocab = {"[UNK]": 1}
    inv_vocab = {i: ("##p" if i % 3 == 0 else "p") for i in range(65536)}

    def tokenize(self, text):
        return [int(t) for t in text.split()]


def _python_case(arena, passages_of, n_docs, seed):
    """AnswerMatcher.hits on `arena` against the restatement fed from the DEVICE tables copied back."""
    from emdr2_amd.data.answer_match import AnswerMatcher, HitMeter, continuation_bits, pack_answers
    rng = np.random.default_rng(seed)
    ptok = arena.dev["passage_tokens"].cpu().numpy().view(np.uint16)
    poff = arena.dev["passage_off"].cpu().numpy()
    B, K = 6, 10
    ids = rng.integers(0, n_docs + 2, size=(B, K))
    lists = []
    for b in range(B):                                                       # answers cut out of the question's own passages, and random ones
        answers = []
        for d in ids[b, :3]:
            if 0 < d <= n_docs and poff[d] - poff[d - 1] >= 4:
                at = int(rng.integers(0, poff[d] - poff[d - 1] - 3))
                answers.append(" ".join(str(int(t)) for t in ptok[poff[d - 1] + at:poff[d - 1] + at + int(rng.integers(1, 4))]))
        answers.append(" ".join(str(int(t)) for t in rng.integers(5, 30000, size=2)))
        lists.append(answers[b % 2:])
    pack = pack_answers(lists, _Tok())
    matcher = AnswerMatcher(arena, _Tok())
    meter = HitMeter(K, device="cuda")
    for dtype in (torch.int64, torch.int32):
        hit_pos, hit_ans, best = matcher.hits(torch.from_numpy(ids).cuda().to(dtype), pack, hist=meter.hist)
        meter.update(n=B)
    exp = ar.answer_hits(ptok, poff, n_docs, ids, pack.tokens, pack.ans_off, pack.q_ans_off, continuation_bits(_Tok()))
    assert np.array_equal(hit_pos.cpu().numpy(), exp[0]) and np.array_equal(hit_ans.cpu().numpy(), exp[1])
    assert np.array_equal(best.cpu().numpy(), exp[2]) and (exp[0] >= 0).any() and (exp[0] < 0).any()
    rep = meter.report((1, 3, K))
    assert rep == {1: 2 * int(exp[3][:1].sum()), 3: 2 * int(exp[3][:3].sum()), K: 2 * int(exp[3][:K].sum()), "total": 2 * B}
    with pytest.raises(TypeError):
        matcher.hits(torch.from_numpy(ids).cuda().float(), pack)
    with pytest.raises(TypeError):
        matcher.hits(torch.from_numpy(ids), pack)
    with pytest.raises(ValueError):
        matcher.hits(torch.from_numpy(ids).cuda()[:3], pack)
    with pytest.raises(ValueError):
        matcher.hits(torch.from_numpy(ids).cuda(), pack, hist=torch.zeros(K, dtype=torch.int64, device="cuda"))


def test_python_path_on_an_arena_from_lists_from_indexed_datasets_and_synthetic(tmp_path):
    from emdr2_amd.data.evidence_arena import EvidenceArena
    from emdr2_amd.data.indexed_dataset import MMapIndexedDatasetBuilder, make_dataset
    rng = np.random.default_rng(21)
    n = 200
    passages = [rng.integers(5, 65536, size=int(m)).tolist() for m in rng.integers(0, 90, size=n)]
    titles = [rng.integers(5, 65536, size=2).tolist() for _ in range(n)]
    _python_case(EvidenceArena(passages, titles).to_device(), passages, n, 1)
    pb, tb = MMapIndexedDatasetBuilder(str(tmp_path / "text.bin")), MMapIndexedDatasetBuilder(str(tmp_path / "title.bin"))
    small = [p or [7] for p in passages]                                     # (no empty documents in the dataset files)
    for p, t in zip(small, titles):
        pb.add_item(p); pb.end_document()
        tb.add_item(t); tb.end_document()
    pb.finalize(str(tmp_path / "text.idx")); tb.finalize(str(tmp_path / "title.idx"))
    arena = EvidenceArena.from_indexed(make_dataset(str(tmp_path / "text")), make_dataset(str(tmp_path / "title")), ["t%d" % (d // 3) for d in range(n)])
    _python_case(arena.to_device(), small, n, 2)
    _python_case(EvidenceArena.synthetic(500, seed=9), None, 500, 3)


# ---- the reference's fixture and the host string matcher, through the kernel -------------------------------------------------------------
def test_fixture_and_has_answer_agreement_through_the_kernel(tmp_path):
    from emdr2_amd.data.answer_match import AnswerMatcher, HitMeter, pack_answers
    from emdr2_amd.data.evidence_arena import EvidenceArena
    from emdr2_amd.tasks.openqa.dense_retriever.evaluation.qa_validation import has_answer
    # the fixture: one question per string case, its text the only document; then the fixture's own questions
    tok = ar.tokenizer_for(tmp_path, _fixture_texts(), pieces=True)
    texts = [c[1] for c in STRING_CASES] + [REF["docs"][str(d)][0] for d in range(1, 5)]
    arena = EvidenceArena([tok.tokenize(t) for t in texts], [[5]] * len(texts)).to_device()
    matcher = AnswerMatcher(arena, tok)
    ids = torch.arange(1, 11, dtype=torch.int32, device="cuda").reshape(10, 1)
    hit_pos, _, _ = matcher.hits(ids, pack_answers([c[0] for c in STRING_CASES], tok))
    differ = [c[0] for c, h in zip(STRING_CASES, (hit_pos[:, 0] >= 0).tolist()) if h != c[3]]
    assert differ == [[ar.CJK_CASE]]
    meter = HitMeter(3, device="cuda")
    qids = torch.tensor([q[1] for q in REF["questions"]], dtype=torch.int64, device="cuda") + 10
    hit_pos, _, best = matcher.hits(qids, pack_answers([q[0] for q in REF["questions"]], tok), hist=meter.hist)
    meter.update(n=3)
    assert (hit_pos >= 0).tolist() == REF["questions_doc_hits"]
    rep = meter.report((1, 2, 3))
    assert [rep[1], rep[2], rep[3]] == REF["top_k_hits"] and rep["total"] == 3
    # the random ASCII corpus: 60 answer sets x 400 passages in one launch
    passages, sets = ar.ascii_corpus(WORDS)
    tok = ar.tokenizer_for(tmp_path, WORDS, pieces=True)
    arena = EvidenceArena([tok.tokenize(p) for p in passages], [[5]] * len(passages)).to_device()
    ids = torch.arange(1, 401, dtype=torch.int32, device="cuda").repeat(60, 1)
    hit_pos, _, _ = AnswerMatcher(arena, tok).hits(ids, pack_answers(sets, tok))
    theirs = np.asarray([[has_answer(answers, text) for text in passages] for answers in sets])
    assert np.array_equal(hit_pos.cpu().numpy() >= 0, theirs) and 2000 < theirs.sum() < 12000
