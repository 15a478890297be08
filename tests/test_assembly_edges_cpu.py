"""CPU: what keeps tests/test_assembly_edges_gpu.py honest.  The branch sweep there is only as good as its case sets, so the conditions
are asserted here, on the oracle alone: every label of tests/assembly_edges.py occurs in at least 4 rows of the union of the case sets,
overlong rows (whose expected value is the oracle's row cut to S) are at most 25 % of all rows, and nothing else is excluded.  The host
side of EvidenceArena -- the production constructor `from_indexed` against `__init__`, `neighbour_paragraphs` against the oracle's
get_neighbour_paragraphs on non-contiguous title groups -- needs no device either."""
import numpy as np
import pytest

from tests import assembly_edges as ae
from oracle import assembly_oracle as ao


@pytest.fixture(scope="module")
def cases():
    return ae.case_sets()


def test_every_label_occurs_and_overlong_rows_are_few(cases):
    (ctx, one, ext), rows = ae.label_counts(cases)
    print("\nrows with a label: %d (of %d slots)" % (rows, sum(len(c["topk_ids"]) * c["cfg"]["topk"] for c in cases)))
    for name, d in (("ctx", ctx), ("one", one), ("ext", ext)):
        print("%s: %s" % (name, "  ".join("%s %d" % kv for kv in d.items())))
    print("overlong share: %.1f %%" % (100.0 * ext["overlong"] / rows))
    assert set(ctx) == set(ae.CTX_LABELS) and set(one) == set(ae.ONE_LABELS) and set(ext) == set(ae.EXT_LABELS)
    for name, d in (("ctx", ctx), ("one", one), ("ext", ext)):
        for label, n in d.items():
            assert n >= 4, "%s label %s occurs in %d rows" % (name, label, n)
        assert sum(d.values()) == rows                          # one label per row and output: no row is left out
    assert ext["overlong"] <= 0.25 * rows


def test_labels_agree_with_what_the_oracle_rows_look_like(cases):
    """The labels restate the oracle's conditions; tie them to its rows: `fit` rows end in padding and no other does, and an overlong
    oracle row really is longer than S (so the `[:S]` rule of expected() rests on a fact, and only there)."""
    n_over = 0
    for case in cases:
        cfg = case["cfg"]
        S, pad = cfg["seq_length"], cfg["pad_id"]
        corp = ao.Corpus(case["passages"], case["titles"], case["group_of_doc"])
        ctx, typ, ext, one, kept, overlong = ae.expected(case)
        labs = ae.row_labels(case)
        K = cfg["topk"]
        for r, lab in enumerate(labs):
            if lab is None:
                continue
            b, j = divmod(r, K)
            assert (lab[0] == "fit") == (ctx[b, j, -1] == pad) and (lab[1] == "fit") == (one[r, -1] == pad)
            assert (lab[2] == "overlong") == bool(overlong[r])
            docs, main, title = corp.evidence(int(kept[b, j]))
            q = case["q_t5"][b, :case["q_len"][b]].tolist()
            row = ao.query_extended_context_t5_format(q, title, docs, main, S, cfg["sep_id"], pad)
            if lab[2] == "overlong":
                n_over += 1
                assert len(row) == len(q) + len(title) + 2 > S and ext[r].tolist() == row[:S]
            else:
                assert len(row) == S and ext[r].tolist() == row
            n = int(np.count_nonzero(ctx[b, j] != pad))          # tokens are >= 5, [CLS] 2, [SEP] 3, pad 0 in these case sets
            assert (typ[b, j, :n] == 0).all() and (typ[b, j, n:] == pad).all()
    assert n_over >= 4


def test_expected_pins_empty_slots_and_rejected_ids():
    """expected(): a slot with no evidence left is -1 with all-pad rows; a rejected id keeps its slot and its value, rows all pad."""
    case = ae.build(3, n_docs=50, n_b=2, topk=3, k_retrieved=3, pad_id=7)
    case["topk_ids"][0] = [4, 51, 9]
    case["topk_ids"][1] = [5, 6, 8]
    case["query_uid"][:] = [-1, 6]
    ctx, typ, ext, one, kept, _ = ae.expected(case)
    assert kept.tolist() == [[4, 51, 9], [5, 8, -1]]
    for b, j in ((0, 1), (1, 2)):
        assert (ctx[b, j] == 7).all() and (typ[b, j] == 7).all() and (ext[b * 3 + j] == 7).all() and (one[b * 3 + j] == 7).all()
    assert (ctx[0, 2] != 7).any() and (ctx[1, 1] != 7).any()


class _Flat(object):
    """What EvidenceArena.from_indexed needs of the memory-mapped datasets: flat_tokens()."""

    def __init__(self, seqs, dtype=np.uint16):
        self.off = np.zeros(len(seqs) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in seqs], out=self.off[1:])
        self.tok = np.array([t for s in seqs for t in s], dtype=dtype)

    def flat_tokens(self):
        return self.tok, self.off


TABLES = ("passage_tokens", "passage_off", "title_tokens", "title_off", "group_docs", "group_off", "doc_group", "doc_pos")


@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_from_indexed_builds_the_tables_of_init(dtype):
    from emdr2_amd.data.evidence_arena import EvidenceArena
    c = ae.corpus(11, n_docs=400)
    small = dict(passages=[[5, 65535], [], [40000]], titles=[[9], [7, 8], [9]], title_keys=["a", "b", "a"])    # docs 1 and 3 share a title
    for corp in (c, small):
        a = EvidenceArena(corp["passages"], corp["titles"], title_keys=corp["title_keys"])
        f = EvidenceArena.from_indexed(_Flat(corp["passages"], dtype), _Flat(corp["titles"], dtype), corp["title_keys"])
        assert a.n_docs == f.n_docs == len(corp["passages"]) and sorted(a.host) == sorted(f.host) == sorted(TABLES)
        for k in TABLES:
            assert a.host[k].dtype == f.host[k].dtype and np.array_equal(a.host[k], f.host[k]), k
        assert f.host["passage_tokens"].dtype == np.uint16 and f.host["title_tokens"].dtype == np.uint16
    assert f.host["group_docs"].tolist() == [1, 3, 2] and f.host["doc_pos"].tolist() == [0, 0, 0, 1] and f.host["doc_group"].tolist() == [0, 0, 1, 0]
    assert f.host["passage_tokens"].tolist() == [5, 65535, 40000]


@pytest.mark.parametrize("bad", [65536, -1])
def test_tokens_outside_uint16_are_refused(bad):
    from emdr2_amd.data.evidence_arena import EvidenceArena
    good, keys = [[5, 6], [7]], ["a", "b"]
    for where in ("passage", "title"):
        p = [[5, bad], [7]] if where == "passage" else good
        t = [[5, bad], [7]] if where == "title" else good
        with pytest.raises(ValueError):
            EvidenceArena(p, t, title_keys=keys)
        with pytest.raises(ValueError):
            EvidenceArena.from_indexed(_Flat(p, np.int64), _Flat(t, np.int64), keys)
    with pytest.raises(ValueError):
        EvidenceArena.from_indexed(_Flat(good), _Flat(good[:1]), keys)            # one title per passage


def test_neighbour_paragraphs_on_non_contiguous_groups():
    from emdr2_amd.data.evidence_arena import EvidenceArena
    c = ae.corpus(12, n_docs=600)
    assert any(g[-1] - g[0] >= len(g) for g in c["group_of_doc"].values())        # the groups really are scattered
    arena = EvidenceArena(c["passages"], c["titles"], title_keys=c["title_keys"])
    for doc in range(1, 601):
        assert arena.neighbour_paragraphs(doc) == ao.get_neighbour_paragraphs(c["group_of_doc"][doc], doc)
        assert arena.passage(doc) == c["passages"][doc - 1] and arena.title(doc) == c["titles"][doc - 1]
