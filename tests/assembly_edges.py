"""Shared by tests/test_assembly_edges_cpu.py and tests/test_assembly_edges_gpu.py (no test functions here).

Small-sequence cases for the evidence fetch + token assembly (csrc/assembly.hip, include/emdr2_assembly.h) in which every branch of the
reference's list functions -- as restated by oracle/assembly_oracle.py -- is reached by construction rather than by luck:

  build(seed, ...)      corpus (passages, titles, NON-CONTIGUOUS title groups: doc ids are dealt to groups of 1..5 through a permutation and
                        each group is sorted ascending), queries, topk ids, query uids and cfg.  Lengths come from small explicit sets
                        that include 0 and the values around every boundary; token ids are drawn from 5..65535 (the upper half of uint16
                        included); the query rows carry random tokens BEHIND query_len, so an over-read shows.
  labels(cfg, ...)      the branch one row takes in each of the three outputs.  It restates the ORACLE's conditions (the slicing rules of
                        query_extended_context_t5_format, query_single_context_t5_format, context_bert_format), not the kernel's.
  expected(case)        oracle.assembly_oracle.postprocess, shaped like the device outputs, plus the three things the reference leaves
                        undefined and include/emdr2_assembly.h pins: overlong rows, rejected ids, empty slots (see there).
"""
import numpy as np

from oracle import assembly_oracle as ao

PLENS = (0, 1, 2, 3, 5, 8, 11, 14, 19, 23)
# S 24 / S_ret 12.  "short" prefixes: ql + tl <= 22, so no row is overlong and the extended-context budget R = 22 - ql - tl sweeps 0..22;
# "long" prefixes: the prefix cuts of the one-context row (cap 23) and of the context-encoder row (cap 11: title 10 = cut at [SEP])
SHORT = dict(tlens=(0, 1, 2, 3, 4, 6, 9, 10), qlens=(0, 1, 2, 3, 5, 7, 8, 10, 12))
LONG = dict(tlens=(9, 10, 11, 13), qlens=(0, 3, 10, 11, 12, 13, 14, 17, 22, 23, 24, 30))

EXT_LABELS = ("overlong", "single", "single_eq", "single_cut", "main_cut", "main_cut_by1",
              "first_fit_2", "first_eq_2", "first_cut_2", "first_fit_3", "first_eq_3", "first_cut_3",
              "last_fit", "last_eq", "last_cut", "last_cut_skipwhole", "mid_leftcut", "mid_leftcut_by1",
              "mid_rightfit", "mid_righteq", "mid_rightcut", "mid_lefteq_righteq", "mid_lefteq_rightcut")
CTX_LABELS = ("fit", "eq", "cut_in_title", "cut_at_sep", "cut_in_passage")
ONE_LABELS = ("fit", "eq", "cut_in_query", "cut_in_title", "cut_at_sep", "cut_in_passage")


def _cut(total, cap, bounds, names):
    """`total` elements capped to `cap`: fit / eq, else the segment that holds the first dropped element (index cap)."""
    if total < cap:
        return "fit"
    if total == cap:
        return "eq"
    for end, name in zip(bounds, names):
        if cap < end:
            return name
    raise AssertionError("cap beyond the row")


def labels(cfg, ql, title, docs, main):
    """-> (ctx label, one label, ext label) of the row the oracle builds from a query of `ql` tokens, `title`, the neighbour passages `docs`
    and `main` (what Corpus.evidence returns)."""
    S, S_ret = cfg["seq_length"], cfg["seq_length_ret"]
    tl, nd, cl = len(title), len(docs), len(docs[main])
    # context_bert_format: [CLS] title [SEP] passage, `enc_ids[0: max_seq_length - 1]`
    ctx = _cut(1 + tl + 1 + cl, S_ret - 1, (1, 1 + tl, 2 + tl, 2 + tl + cl), ("cut_in_cls", "cut_in_title", "cut_at_sep", "cut_in_passage"))
    # query_single_context_t5_format: query title [SEP] passage, `enc_ids[0: max_seq_length - 1]`
    one = _cut(ql + tl + 1 + cl, S - 1, (ql, ql + tl, ql + tl + 1, ql + tl + 1 + cl), ("cut_in_query", "cut_in_title", "cut_at_sep", "cut_in_passage"))
    # query_extended_context_t5_format
    if ql + tl + 2 > S:
        return ctx, one, "overlong"                      # query + title + 2 [SEP] alone exceed S: the reference's list is longer than S
    R = S - (ql + tl + 1) - 1                            # remaining_len
    if nd == 1:
        ext = "single" if cl < R else ("single_eq" if cl == R else "single_cut")
    elif cl > R:
        ext = "main_cut_by1" if cl == R + 1 else "main_cut"
    else:
        extra_len = R - cl
        if main == 0:
            E = sum(len(d) for d in docs[1:])
            ext = "first_%s_%d" % ("fit" if E < extra_len else ("eq" if E == extra_len else "cut"), nd)
        elif main == -1:
            E = sum(len(d) for d in docs[:-1])
            if E < extra_len:
                ext = "last_fit"
            elif E == extra_len:
                ext = "last_eq"
            else:
                offset = E - extra_len + 1
                ext = "last_cut_skipwhole" if 0 < len(docs[0]) <= offset else "last_cut"
        else:
            left, right = len(docs[0]), len(docs[2])     # a middle document always has both neighbours
            if left > extra_len:
                ext = "mid_leftcut_by1" if left == extra_len + 1 else "mid_leftcut"
            elif left == extra_len:
                ext = "mid_lefteq_righteq" if right == 0 else "mid_lefteq_rightcut"
            else:
                rem = extra_len - left
                ext = "mid_rightfit" if right < rem else ("mid_righteq" if right == rem else "mid_rightcut")
    return ctx, one, ext


def corpus(seed, n_docs=3000, plens=PLENS, tlens=SHORT["tlens"], tok_lo=5, tok_hi=65535):
    """passages, titles (one per title group), group_of_doc (doc -> ascending ids of its group), title_keys (strings).  Groups of 1..5 docs
    whose ids are scattered over the corpus."""
    rng = np.random.default_rng(seed)
    perm = (rng.permutation(n_docs) + 1).tolist()
    groups, at = [], 0
    while at < n_docs:
        s = int(min(n_docs - at, rng.integers(1, 6)))
        groups.append(sorted(perm[at:at + s])); at += s
    tok = lambda n: rng.integers(tok_lo, tok_hi + 1, size=int(n)).tolist()
    passages = [tok(rng.choice(plens)) for _ in range(n_docs)]
    titles, keys, group_of_doc = [None] * n_docs, [None] * n_docs, {}
    for gi, g in enumerate(groups):
        t = tok(rng.choice(tlens))
        for doc in g:
            titles[doc - 1], keys[doc - 1], group_of_doc[doc] = t, "title-%d" % gi, g
    # the extreme token values occur whatever the draw
    for d, v in ((0, tok_hi), (1, tok_lo)):
        if passages[d]:
            passages[d][0] = v
    return dict(passages=passages, titles=titles, group_of_doc=group_of_doc, title_keys=keys)


def build(seed, n_docs=3000, n_b=64, topk=40, k_retrieved=None, S=24, S_ret=12, plens=PLENS, tlens=SHORT["tlens"], qlens=SHORT["qlens"],
          q_stride=None, cls_id=2, sep_id=3, pad_id=0, tok_lo=5, tok_hi=65535, corp=None):
    """One case: corpus (or `corp`, to put other queries / shapes on the same corpus) + queries + retrieval result + cfg."""
    case = dict(corp if corp is not None else corpus(seed, n_docs, plens, tlens, tok_lo, tok_hi))
    n_docs = len(case["passages"])
    rng = np.random.default_rng(seed + 100003)
    kr = topk + 1 if k_retrieved is None else k_retrieved
    q_stride = max(max(qlens), 1) if q_stride is None else q_stride
    q_len = rng.choice(qlens, size=n_b).astype(np.int64)
    q_len[:min(n_b, len(qlens))] = qlens[:n_b]                                    # every query length occurs when there is room
    q_t5 = rng.integers(tok_lo, tok_hi + 1, size=(n_b, q_stride)).astype(np.int64)   # random tokens behind q_len too
    if kr <= n_docs:
        ids = np.stack([rng.permutation(n_docs)[:kr] + 1 for _ in range(n_b)]).astype(np.int32)
    else:
        ids = rng.integers(1, n_docs + 1, size=(n_b, kr)).astype(np.int32)
    uid = -np.arange(1, n_b + 1, dtype=np.int64)
    if kr > topk:
        for b in range(0, n_b, 16):                                               # the trivial-document skip, at varying slots
            uid[b] = int(ids[b, (b // 16) % kr])
    case.update(q_t5=q_t5, q_len=q_len, topk_ids=ids, query_uid=uid,
                cfg=dict(topk=topk, seq_length_ret=S_ret, seq_length=S, cls_id=cls_id, sep_id=sep_id, pad_id=pad_id))
    return case


def case_sets():
    """The branch sweep: short prefixes for the extended-context branches, a smaller long-prefix set for the prefix cuts."""
    return [build(1, n_b=64, topk=40, **SHORT), build(2, n_b=12, topk=40, **LONG)]


class _TolerantCorpus(ao.Corpus):
    """Ids the kernel's guard rejects get a placeholder here so that postprocess itself decides which ids fill which slot; expected()
    then overwrites their rows."""

    def evidence(self, doc_id):
        if not 0 < doc_id <= len(self.passages):
            return [[]], 0, []
        return ao.Corpus.evidence(self, doc_id)


def expected(case):
    """-> ctx [B,K,S_ret], types, ext [B*K,S], one [B*K,S] (int64), kept [B,K] (int32), overlong [B*K] (bool), as the device must give them.
    Everything is oracle.assembly_oracle.postprocess except, as include/emdr2_assembly.h states:
      overlong rows (query + title + 2 > S): the oracle's extended row is longer than S; the first S tokens are expected
      rejected ids (<= 0 or > n_docs):       all-pad rows (types too), kept = the id as retrieved
      slots with no evidence left:           all-pad rows, kept = -1"""
    cfg = case["cfg"]
    K, S, S_ret, pad = cfg["topk"], cfg["seq_length"], cfg["seq_length_ret"], cfg["pad_id"]
    n_docs, B = len(case["passages"]), len(case["topk_ids"])
    corp = _TolerantCorpus(case["passages"], case["titles"], case["group_of_doc"])
    octx, otyp, oext, oone, okept = ao.postprocess(case["query_uid"].tolist(), case["q_t5"].tolist(), case["q_len"].tolist(),
                                                   case["topk_ids"].tolist(), corp, K, S_ret, S, cfg["cls_id"], cfg["sep_id"], pad)
    ctx = np.full((B, K, S_ret), pad, dtype=np.int64)
    typ = np.full((B, K, S_ret), pad, dtype=np.int64)
    ext = np.full((B * K, S), pad, dtype=np.int64)
    one = np.full((B * K, S), pad, dtype=np.int64)
    kept = np.full((B, K), -1, dtype=np.int32)
    overlong = np.zeros(B * K, dtype=bool)
    flat = 0
    for b in range(B):
        for j, eid in enumerate(okept[b]):
            kept[b, j] = eid
            if 0 < eid <= n_docs:
                ctx[b, j], typ[b, j], one[b * K + j] = octx[b][j], otyp[b][j], oone[flat]
                row = oext[flat]
                if int(case["q_len"][b]) + len(case["titles"][eid - 1]) + 2 > S:
                    assert len(row) > S, "an overlong row is one the reference cannot batch"
                    overlong[b * K + j] = True
                    row = row[:S]
                ext[b * K + j] = row
            flat += 1
    return ctx, typ, ext, one, kept, overlong


def row_labels(case):
    """[B*K] list of (ctx, one, ext) labels; None for slots without a valid evidence."""
    cfg, K = case["cfg"], case["cfg"]["topk"]
    corp = ao.Corpus(case["passages"], case["titles"], case["group_of_doc"])
    out = [None] * (len(case["topk_ids"]) * K)
    for b, (uid, ids) in enumerate(zip(case["query_uid"].tolist(), case["topk_ids"].tolist())):
        j = 0
        for eid in ids:
            if eid != uid and j < K:
                if 0 < eid <= len(case["passages"]):
                    docs, main, title = corp.evidence(eid)
                    out[b * K + j] = labels(cfg, int(case["q_len"][b]), title, docs, main)
                j += 1
    return out


def label_counts(cases):
    """-> ({label: rows} for ctx, one, ext; rows with a label)."""
    counts = (dict.fromkeys(CTX_LABELS, 0), dict.fromkeys(ONE_LABELS, 0), dict.fromkeys(EXT_LABELS, 0))
    rows = 0
    for case in cases:
        for lab in row_labels(case):
            if lab is not None:
                rows += 1
                for c, l in zip(counts, lab):
                    c[l] += 1
    return counts, rows
