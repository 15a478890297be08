"""GPU: the evidence fetch + token assembly kernel (csrc/assembly.hip: assemble_kernel, behind EvidenceArena.assemble and
IndexBuilder.context_inputs) against oracle/assembly_oracle.py, bit for bit, at sequence lengths in the tens, where every branch of the
reference's list functions is reached by a few thousand rows and the Python-list oracle costs a fraction of a second.  The cases are
built by tests/assembly_edges.py; tests/test_assembly_edges_cpu.py asserts, without a device, that they reach what is claimed below.

What each test is for:

  branch sweep       two case sets on non-contiguous title groups (S 24, S_ret 12, token ids 5..65535, empty passages / titles / queries):
                     64 x 40 rows with short prefixes (ql + tl <= 22) for the extended-context branches, 12 x 40 rows with long prefixes
                     for the prefix cuts.  thread 0's segment lists: SegList::add / truncate and every `ext` branch, with the two `+ 1`
                     left-cut offsets and doc_row[-1:2].  Rows per label (3,040 rows, 321 = 10.6 % of them overlong):
                       ctx  fit 850  eq 166  cut_in_title 246  cut_at_sep 417  cut_in_passage 1361
                       one  fit 1743  eq 94  cut_in_query 80  cut_in_title 195  cut_at_sep 46  cut_in_passage 882
                       ext  overlong 321  single 205  single_eq 14  single_cut 129  main_cut 694  main_cut_by1 59
                            first_fit_2 63  first_eq_2 7  first_cut_2 52  first_fit_3 77  first_eq_3 10  first_cut_3 261
                            last_fit 102  last_eq 12  last_cut 95  last_cut_skipwhole 151  mid_leftcut 335  mid_leftcut_by1 21
                            mid_rightfit 184  mid_righteq 16  mid_rightcut 188  mid_lefteq_righteq 7  mid_lefteq_rightcut 37
  copy loop          the 128-thread copy phase and the row addressing: (S_ret, S) = (2, 2), (12, 24), (127, 129), (128, 128), (129, 300)
                     x (n_b, topk) = (1, 1), (300, 1), (3, 130) on one corpus with passages of up to 290 tokens and queries of up to
                     S + 5, so that `fetch` walks segment borders in the second and third pass of the loop too; pad_id 7, [CLS] / [SEP]
                     above 32767, the query rows a column slice of a wider tensor; context types = pad_id on padding, 0 elsewhere.
  high token ids     every passage, title and query token in 32768..65535: the uint16 tables travel through an int16 view
                     (EvidenceArena.to_device) and must come back unsigned.
  fewer than topk    k_retrieved == topk with the query's own uid among the ids (slot 0, last slot, twice): the last slots are
                     kept == -1 with all-pad_id rows.
  rejected ids       0, -1, n_docs + 1, INT32_MAX: what the guard `eid > 0 && eid <= n_docs` keeps away from the tables.  Their rows are
                     all padding, kept_ids holds the id as retrieved, the valid ids of the same launch are unaffected.  (query_len outside
                     [0, q_stride] and table offsets outside the tables are NOT guarded on the device and not tested: caller obligations,
                     include/emdr2_assembly.h.)
  no stray writes    the C ABI with each output an interior window of a sentinel-filled buffer, query_t5 a pointer into a wider storage
                     (q_stride > the row width): guards bit-identical afterwards, no sentinel left inside, contents = oracle.
  synthetic arena    EvidenceArena.synthetic(500): the invariants the kernel assumes of the tables, then one assemble call against an
                     oracle Corpus read back from those tables.
  indexer            IndexBuilder.context_inputs (topk == k_retrieved == n, seq_len 8, empty query) for n = 1, 127, 128, 129, 1000 doc ids
                     with repeats against context_bert_format(title + [sep] + passage).

Found: nothing.  Every test passed against the kernel and the host table builders as they stood, on an MI355X.  Planted on a scratch
copy, one at a time: the `+ 1` dropped from the `kind == -1` offset fails the branch sweep (222 rows of the first case set, all of them
last_cut or last_cut_skipwhole, the first a last_cut row) and 14 more tests; passage tokens read as int16_t fail 22 of the 28 tests
(the sweep first in ctx; the high-token-id, indexer, copy-loop, stray-write, fewer-than-topk and rejected-id tests); and
`rowi = b * k_retrieved + j` fails the stray-write test (the rows of b >= 1 land k_retrieved - topk rows late, the last ones in the
trailing guard: "ctx: a write outside the output").  That fault was run against the stray-write test alone, whose guard rows keep the
misplaced rows inside the buffer.  `>=` -> `>` in SegList::truncate changes no output and no test can see it: when a segment ends
exactly at the cap, the next iteration cuts the following segment (add() never stores an empty one, and total > cap says there is one)
to length 0 and drops it -- the same list.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import assembly_oracle as ao
from tests import assembly_edges as ae

pytestmark = pytest.mark.gpu
NAMES = ("ctx", "types", "ext", "one", "kept")
INT32_MAX = 2 ** 31 - 1


def _arena(corp):
    from emdr2_amd.data.evidence_arena import EvidenceArena
    return EvidenceArena(corp["passages"], corp["titles"], title_keys=corp["title_keys"]).to_device()


def _assemble(arena, case, q_t5=None):
    cfg = case["cfg"]
    q = torch.from_numpy(case["q_t5"]) if q_t5 is None else q_t5
    out = arena.assemble(torch.from_numpy(case["topk_ids"]).cuda(), cfg["topk"], torch.from_numpy(case["query_uid"]), q,
                         torch.from_numpy(case["q_len"]), cfg["seq_length_ret"], cfg["seq_length"], cfg["cls_id"], cfg["sep_id"], cfg["pad_id"])
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check(case, got, exp=None, labs=None):
    """got == expected(case) bit for bit; on a mismatch, the first differing (row, position) with that row's labels."""
    exp = ae.expected(case) if exp is None else exp
    K = case["cfg"]["topk"]
    for name, g, e in zip(NAMES, got, exp):
        assert g.shape == e.shape and g.dtype == e.dtype, (name, g.shape, e.shape, g.dtype, e.dtype)
        if np.array_equal(g, e):
            continue
        width = e.shape[-1] if name != "kept" else 1
        g2, e2 = g.reshape(-1, width), e.reshape(-1, width)
        r, p = (int(v) for v in np.argwhere(g2 != e2)[0])
        labs = ae.row_labels(case) if labs is None else labs
        pytest.fail("%s differs first at row %d (query %d, slot %d) position %d: got %d, oracle %d; labels (ctx, one, ext) of the row: %s; "
                    "%d elements in %d rows differ" % (name, r, r // K, r % K, p, g2[r, p], e2[r, p], labs[r], int((g2 != e2).sum()),
                                                       int((g2 != e2).any(axis=1).sum())))


@pytest.fixture(scope="module")
def sweep():
    """(case, arena, expected, labels) of the two case sets; computed once, left unchanged."""
    return [(c, _arena(c), ae.expected(c), ae.row_labels(c)) for c in ae.case_sets()]


@pytest.fixture(scope="module")
def long_corpus():
    """The corpus of the copy-loop and stray-write cases: passages long enough for rows that are tokens, not padding, beyond position 256."""
    corp = ae.corpus(21, n_docs=600, plens=ae.PLENS + (100, 126, 127, 128, 140, 290), tlens=(0, 1, 3, 9, 13))
    return corp, _arena(corp)


def test_branch_sweep(sweep):
    for case, arena, exp, labs in sweep:
        _check(case, _assemble(arena, case), exp, labs)


def _copy_case(corp, s_ret, s, n_b, topk, seed):
    qlens = tuple(sorted({max(0, v) for v in (s // 2, 0, 1, s - 3, s - 2, s - 1, s, s + 5)}, key=lambda v: (v != s // 2, v)))
    return ae.build(seed, n_b=n_b, topk=topk, S=s, S_ret=s_ret, qlens=qlens, q_stride=s + 5, cls_id=40001, sep_id=65000, pad_id=7, corp=corp)


@pytest.mark.parametrize("n_b,topk", [(1, 1), (300, 1), (3, 130)])
@pytest.mark.parametrize("s_ret,s", [(2, 2), (12, 24), (127, 129), (128, 128), (129, 300)])
def test_copy_loop_and_addressing(long_corpus, s_ret, s, n_b, topk):
    corp, arena = long_corpus
    case = _copy_case(corp, s_ret, s, n_b, topk, seed=1000 * s + n_b)
    # the query rows as a column slice of a wider tensor: width != storage stride
    wide = torch.randint(5, 65536, (n_b, s + 5 + 6), dtype=torch.int64)
    view = wide[:, 4:4 + s + 5]
    view.copy_(torch.from_numpy(case["q_t5"]))
    assert view.stride(0) != view.shape[1] and (n_b == 1 or not view.is_contiguous())
    got = _assemble(arena, case, q_t5=view)
    exp = ae.expected(case)
    _check(case, got, exp)
    # the reference's quirk: the types of the padding are pad_id, everything else is 0 -- on the device's own rows
    ctx, typ = got[0].reshape(-1, s_ret), got[1].reshape(-1, s_ret)
    n_tok = np.array([min(s_ret - 1, 2 + len(corp["titles"][e - 1]) + len(corp["passages"][e - 1])) + 1 for e in exp[4].reshape(-1).tolist()])
    pos = np.arange(s_ret)[None, :]
    assert np.array_equal(typ, np.where(pos < n_tok[:, None], 0, 7)) and (ctx[pos >= n_tok[:, None]] == 7).all()


def test_high_token_ids_come_back_unsigned():
    case = ae.build(31, n_docs=300, n_b=8, topk=10, tok_lo=32768, tok_hi=65535)
    assert case["passages"][0][0] == 65535 and min(min(p) for p in case["passages"] if p) >= 32768
    case["topk_ids"][1, 0] = 1                                              # the passage that starts with 65535 is retrieved
    got = _assemble(_arena(case), case)
    _check(case, got)
    assert min(g.min() for g in got[:4]) == 0 and max(g.max() for g in got[:4]) == 65535
    assert (got[2] >= 32768).sum() > got[2].size // 2                       # the rows really are made of such tokens


def test_fewer_than_topk_kept():
    """k_retrieved == topk: every skipped id leaves a slot at the end empty."""
    case = ae.build(41, n_docs=200, n_b=4, topk=6, k_retrieved=6, pad_id=7)
    ids, uid = case["topk_ids"], case["query_uid"]
    uid[0] = ids[0, 0]                                                      # the uid at slot 0
    uid[1] = ids[1, 5]                                                      # at the last slot
    ids[2, 4] = ids[2, 1]; uid[2] = ids[2, 1]                               # twice
    got = _assemble(_arena(case), case)
    _check(case, got)
    ctx, typ, ext, one, kept = got
    assert kept[0].tolist() == ids[0, 1:].tolist() + [-1] and kept[1].tolist() == ids[1, :5].tolist() + [-1]
    assert kept[2].tolist() == [int(ids[2, 0]), int(ids[2, 2]), int(ids[2, 3]), int(ids[2, 5]), -1, -1] and kept[3].tolist() == ids[3].tolist()
    for b, j in ((0, 5), (1, 5), (2, 4), (2, 5)):
        assert (ctx[b, j] == 7).all() and (typ[b, j] == 7).all() and (ext[b * 6 + j] == 7).all() and (one[b * 6 + j] == 7).all()


def test_rejected_ids_give_padding_and_leave_the_rest_alone():
    """The ids the guard of assemble_kernel keeps away from the tables (a search over an index with fewer than k rows can return them)."""
    case = ae.build(51, n_docs=200, n_b=3, topk=6, k_retrieved=7, pad_id=7)
    ids = case["topk_ids"]
    case["query_uid"][:] = [-11, -12, -13]                                  # no uid equals an id, -1 included
    ids[0, 1], ids[0, 4], ids[1, 0], ids[1, 3] = 0, -1, 201, INT32_MAX
    clean = dict(case, topk_ids=ids.copy())
    clean["topk_ids"][0, 1], clean["topk_ids"][0, 4], clean["topk_ids"][1, 0], clean["topk_ids"][1, 3] = 1, 2, 3, 4
    arena = _arena(case)
    got = _assemble(arena, case)
    _check(case, got)
    ctx, typ, ext, one, kept = got
    assert kept[0, 1] == 0 and kept[0, 4] == -1 and kept[1, 0] == 201 and kept[1, 3] == INT32_MAX      # the id as retrieved
    bad = np.zeros((3, 6), dtype=bool)
    bad[0, 1] = bad[0, 4] = bad[1, 0] = bad[1, 3] = True
    for g in (ctx.reshape(18, -1), typ.reshape(18, -1), ext, one):
        assert (g[bad.reshape(-1)] == 7).all()
    # every other row is what a launch without the rejected ids gives
    ref = _assemble(arena, clean)
    for g, r in zip(got, ref):
        g, r = g.reshape(18, -1), r.reshape(18, -1)
        assert np.array_equal(g[~bad.reshape(-1)], r[~bad.reshape(-1)])


SENT64, SENT32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


@pytest.mark.parametrize("n_b,topk,s_ret,s", [(1, 1, 2, 2), (5, 3, 12, 24), (3, 130, 127, 129)])
def test_no_stray_writes_through_the_c_abi(long_corpus, n_b, topk, s_ret, s):
    from emdr2_amd import _native
    corp, arena = long_corpus
    case = _copy_case(corp, s_ret, s, n_b, topk, seed=77 + n_b)
    cfg, guard = case["cfg"], 6                                             # guard rows before and behind every window
    rows = n_b * topk

    def window(n_rows, width, dtype, sentinel):
        big = torch.full(((n_rows + 2 * guard) * width,), sentinel, dtype=dtype, device="cuda")
        return big, big[guard * width:(guard + n_rows) * width]
    bufs = [window(rows, s_ret, torch.int64, SENT64), window(rows, s_ret, torch.int64, SENT64), window(rows, s, torch.int64, SENT64),
            window(rows, s, torch.int64, SENT64), window(n_b, topk, torch.int32, SENT32)]
    ids = torch.from_numpy(case["topk_ids"]).cuda()
    uid, ql = torch.from_numpy(case["query_uid"]).cuda(), torch.from_numpy(case["q_len"]).cuda()
    width = case["q_t5"].shape[1]
    wide = torch.randint(5, 65536, (n_b, width + 9), dtype=torch.int64)
    wide[:, 5:5 + width] = torch.from_numpy(case["q_t5"])
    wide = wide.cuda()
    q_ptr = wide.data_ptr() + 5 * 8                                         # row b of the query starts at q_ptr + b * q_stride words
    rc = _native.lib().emdr2_assemble_evidence(ctypes.byref(arena._struct), ids.data_ptr(), n_b, ids.shape[1], topk, uid.data_ptr(), q_ptr,
                                               width + 9, ql.data_ptr(), s_ret, s, cfg["cls_id"], cfg["sep_id"], cfg["pad_id"],
                                               bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), bufs[2][1].data_ptr(), bufs[3][1].data_ptr(),
                                               bufs[4][1].data_ptr(), _native.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    exp = ae.expected(case)
    got = []
    for name, (big, _), e, sent in zip(NAMES, bufs, exp, (SENT64,) * 4 + (SENT32,)):
        h = big.cpu().numpy()
        w = e.shape[-1]
        assert (h[:guard * w] == sent).all() and (h[(guard + e.size // w) * w:] == sent).all(), "%s: a write outside the output" % name
        inside = h[guard * w:(guard + e.size // w) * w]
        assert not (inside == sent).any(), "%s: %d words were never written" % (name, int((inside == sent).sum()))
        got.append(inside.reshape(e.shape))
    _check(case, tuple(got), exp)


def test_synthetic_arena_tables_and_one_assemble_call():
    from emdr2_amd.data.evidence_arena import EvidenceArena
    n = 500
    arena = EvidenceArena.synthetic(n, seed=9)
    h = {k: v.cpu().numpy() for k, v in arena.dev.items()}
    g_off, g_docs, d_group, d_pos = h["group_off"], h["group_docs"], h["doc_group"], h["doc_pos"]
    assert g_off[0] == 0 and g_off[-1] == n and (np.diff(g_off) > 0).all() and len(g_docs) == n
    assert len(d_group) == len(d_pos) == n + 1 and d_group[1:].min() == 0 and d_group[1:].max() == len(g_off) - 2
    d = np.arange(1, n + 1)
    assert np.array_equal(g_docs[g_off[d_group[d]] + d_pos[d]], d)
    assert (d_pos[d] >= 0).all() and (d_pos[d] < np.diff(g_off)[d_group[d]]).all()
    for g in range(len(g_off) - 1):
        assert (np.diff(g_docs[g_off[g]:g_off[g + 1]]) > 0).all()           # ascending inside a group
    for off, tok in ((h["passage_off"], h["passage_tokens"]), (h["title_off"], h["title_tokens"])):
        assert off.dtype == np.int64 and len(off) == n + 1 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(tok)
        assert tok.dtype == np.int16 and tok.min() >= 5
    assert g_docs.dtype == d_group.dtype == d_pos.dtype == np.int32 and g_off.dtype == np.int64
    # an oracle corpus from the tables, then one call at lengths where these passages (100..160 tokens) are cut and are not
    u = lambda a: (a.astype(np.int64) & 0xffff).tolist()
    corp = dict(passages=[u(h["passage_tokens"][h["passage_off"][i]:h["passage_off"][i + 1]]) for i in range(n)],
                titles=[u(h["title_tokens"][h["title_off"][i]:h["title_off"][i + 1]]) for i in range(n)],
                group_of_doc={int(doc): g_docs[g_off[d_group[doc]]:g_off[d_group[doc] + 1]].tolist() for doc in d})
    case = ae.build(61, n_b=8, topk=12, S=300, S_ret=150, qlens=(0, 9, 20, 33, 60, 120), corp=corp)
    _check(case, _assemble(arena, case))


@pytest.mark.parametrize("n", [1, 127, 128, 129, 1000])
def test_indexer_context_inputs(sweep, n):
    from emdr2_amd.indexer_emdr2 import IndexBuilder
    case, arena = sweep[0][0], sweep[0][1]
    s_ret, cls, sep, pad = 12, 40001, 65000, 7
    builder = IndexBuilder(None, arena, s_ret, cls, sep, pad)
    ids = np.random.default_rng(n).integers(1, len(case["passages"]) + 1, size=n)
    ids[-1] = ids[0]                                                        # repeats
    ids[n // 2] = ids[0]
    ctx, typ = builder.context_inputs(torch.from_numpy(ids))
    torch.cuda.synchronize()
    exp = [ao.context_bert_format(case["titles"][e - 1] + [sep] + case["passages"][e - 1], s_ret, cls, sep, pad) for e in ids.tolist()]
    assert ctx.shape == typ.shape == (n, s_ret) and ctx.dtype == typ.dtype == torch.int64
    e_ctx, e_typ = np.array([e[0] for e in exp], dtype=np.int64), np.array([e[1] for e in exp], dtype=np.int64)
    for name, g, e in (("ctx", ctx.cpu().numpy(), e_ctx), ("types", typ.cpu().numpy(), e_typ)):
        if not np.array_equal(g, e):
            r, p = (int(v) for v in np.argwhere(g != e)[0])
            pytest.fail("%s differs first at row %d (doc %d) position %d: got %d, oracle %d" % (name, r, ids[r], p, g[r, p], e[r, p]))
