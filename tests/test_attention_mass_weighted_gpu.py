"""GPU: emdr2_attention_key_mass_weighted and emdr2_head_row_norms (csrc/attention_mass.hip) against the float64 references and bounds of
tests/attention_mass_weighted_ref.py.

Pass criterion: worst |kernel - reference| / bound < 1 over every element; the bounds are derived there from the kernels' order of
operations and are not tuned; the worst ratios measured per family are recorded in profiles/retriever_distill.txt.  Where the claim is
about bits (kw = 1 against the unweighted entry, poisoned against clean tables, repeat, batching) the criterion is torch.equal.
Shapes: those of tests/test_attention_mass_gpu.py, whose `Case` this module reuses: segment boundaries inside a 16-key group, empty
segments, a 700-key segment, 100 short segments, 4,200 keys with uncovered lead and trail keys, dense keys with padding.
Norms: the contract's range is sum of squares normal and finite in fp32 (2^-59 <= max |v|, |v| <= 2^60: include/emdr2_ops.h); the 2^-70
family lies below it and is held by the absolute term of the bound alone."""
import pytest
import torch

from tests import attention_mass_ref as MR
from tests import attention_mass_weighted_ref as WR
from tests import attention_ref as R
from tests.test_attention_mass_gpu import DEV, HEADS, SEG_100, SEG_A, SEG_LONG, _case, _gen

pytestmark = pytest.mark.gpu

SEG_END = ([100, 27], [100, 29])                  # 256 keys in all: the packed layout has exactly 256 rows, the last segment ends at the last one
LONG_KW = dict(lead=[50, 10], trail=[50, 40], seed=9, pos_div=8)


def _check(tag, got, ref, bound):
    ratio, idx = R.worst(got, ref, bound)
    print("[attn-mass-kw] %s worst err/bound %.3f at %s (ref %.4g, got %.4g)" % (tag, ratio, idx, float(ref[idx]), float(got[idx])))
    assert ratio < 1.0, (tag, ratio, idx)
    return ratio


def _table(c, kind, seed=0):
    """A key-weight table fp32 [HEADS, rows] of a Case: random in [0.25, 4]; `zeros`: a fifth of the entries exactly 0."""
    g = _gen(500 + seed)
    kw = torch.rand((HEADS, c.seqs.rows), generator=g, device=DEV) * 3.75 + 0.25
    if kind == "zeros":
        kw = torch.where(torch.rand((HEADS, c.seqs.rows), generator=g, device=DEV) < 0.2, torch.zeros_like(kw), kw)
    return kw.contiguous()


def _per_sequence(c, kw):
    cu = c.seqs.cu.tolist()
    return [kw[:, cu[i]:cu[i + 1]].t().double() for i in range(c.b)]


def _covered(c):
    """bool [rows]: the key rows that lie inside some segment of their question."""
    cov = torch.zeros(c.seqs.rows, dtype=torch.bool, device=DEV)
    cu, seg = c.seqs.cu.tolist(), c.seg.tolist()
    for i in range(c.b):
        cov[cu[i] + seg[i][0]:cu[i] + seg[i][-1]] = True
    return cov


def _run(c, m, l, w, kw, mass=None, accumulate=False, which=None):
    from emdr2_amd.model import kernels as K
    if which is None:
        mass = torch.full((c.b, HEADS, c.G), float("nan"), device=DEV) if mass is None else mass
        return K.attention_key_mass(c.q, c.kv[:, 0], c.ids_q, c.seqs, m, l, c.seg, w, mass, accumulate=accumulate, kw=kw)
    i = which                                                              # question `which` alone: its own PackedSeqs, rows and table
    n = c.k32[i].shape[0]
    seqs = K.PackedSeqs(torch.zeros((1, n), dtype=torch.int64, device=DEV) + 7)
    kv = torch.zeros((seqs.rows, 2, HEADS, 64), device=DEV)
    kv[:seqs.total, 0] = c.k32[i]
    c0 = int(c.seqs.cu[i])
    kw1 = torch.full((HEADS, seqs.rows), float("nan"), device=DEV)
    kw1[:, :n] = kw[:, c0:c0 + n]
    return K.attention_key_mass(c.q[i:i + 1].contiguous(), kv.bfloat16()[:, 0], c.ids_q[i:i + 1].contiguous(), seqs, m[i:i + 1].contiguous(),
                                l[i:i + 1].contiguous(), c.seg[i:i + 1].contiguous(), None if w is None else w[i:i + 1].contiguous(),
                                torch.full((1, HEADS, c.G), float("nan"), device=DEV), kw=kw1)


@pytest.mark.parametrize("sq", [1, 32, 100])
def test_unit_weights_give_the_unweighted_entrys_bits(sq):
    c = _case("randn", SEG_A, sq, seed=sq)
    m, l = c.made_stats()
    ones = torch.ones((HEADS, c.seqs.rows), device=DEV)
    for w in (c.w, None):
        plain = c.run(m, l, w)
        assert torch.equal(_run(c, m, l, w, ones), plain)
        acc = _run(c, m, l, w, ones, mass=plain.clone(), accumulate=True)
        assert torch.equal(acc, c.run(m, l, w, mass=plain.clone(), accumulate=True))


@pytest.mark.parametrize("kind", ["rand", "zeros"])
@pytest.mark.parametrize("shape", ["A/sq32", "A/sq100", "100seg", "long", "end"])
def test_random_weights_against_the_reference(shape, kind):
    c = {"A/sq32": lambda: _case("randn", SEG_A, 32, seed=32), "A/sq100": lambda: _case("randn", SEG_A, 100, seed=100),
         "100seg": lambda: _case("randn", SEG_100, 32, seed=7), "long": lambda: _case("stair_up", SEG_LONG, 32, **LONG_KW),
         "end": lambda: _case("randn", SEG_END, 32, seed=3)}[shape]()
    m, l = c.made_stats()
    kw = _table(c, kind, seed=len(shape))
    if shape == "end":                                                     # the table has exactly `rows` elements per head and the last segment
        assert c.seqs.rows == c.seqs.total == 256 and kw.numel() == HEADS * 256      # ends at the allocation's last element
        assert int(c.seqs.cu[-1]) == 256 and int(c.seg[1, -1]) == 129
    ref, bound = WR.weighted_mass_reference(c.q32, c.k32, c.ids_q, c.ids_k, m, l, c.seg.cpu(), _per_sequence(c, kw), c.w)
    got = _run(c, m, l, c.w, kw)
    _check("%s/%s" % (shape, kind), got, ref, bound)
    if shape.startswith("A/"):
        assert float(got[0, :, 4].abs().max()) == 0.0 and float(got[2, :, 1:3].abs().max()) == 0.0     # empty segments: exactly 0


@pytest.mark.parametrize("shape", ["A", "long"])
def test_nan_on_every_uncovered_key_and_past_the_last_sequence_changes_no_bit(shape):
    """The clamp (the kw load never leaves the segment) and the select (a clamped lane's product is not added)."""
    c = _case("randn", SEG_A, 32, seed=32) if shape == "A" else _case("stair_up", SEG_LONG, 32, **LONG_KW)
    m, l = c.made_stats()
    kw = _table(c, "rand", seed=1)
    poisoned = torch.where(_covered(c)[None], kw, torch.full_like(kw, float("nan"))).contiguous()
    assert bool(torch.isnan(poisoned[:, c.seqs.total:]).all()) and c.seqs.rows > c.seqs.total
    if shape == "long":
        assert bool(torch.isnan(poisoned[:, :10]).all())                   # lead keys of question 0 belong to no segment
    clean = _run(c, m, l, c.w, kw)
    got = _run(c, m, l, c.w, poisoned)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, clean)


@pytest.mark.parametrize("sq", [1, 32])
def test_dense_keys_with_padding_carry_finite_weights(sq):
    """sk = 96 = three segments of S = 32, pad ids in every segment's tail and one all-pad segment (the dense case of the unweighted tests)."""
    from emdr2_amd.model import kernels as K
    b, sk, S = 2, 96, 32
    g = _gen(40 + sq)
    q, k, _, _ = R.family("randn", b, HEADS, sq, sk, 64, g, DEV)
    ids_k = torch.full((b, sk), 7, dtype=torch.int64, device=DEV)
    for s_, pad in enumerate((5, 1, 17)):
        ids_k[0, (s_ + 1) * S - pad:(s_ + 1) * S] = 0
    ids_k[1, S:2 * S] = 0
    ids_k[1, 2 * S + 20:] = 0
    ids_q = torch.full((b, sq), 7, dtype=torch.int64, device=DEV)
    if sq > 1:
        ids_q[1, 3] = 0
    seg = (torch.arange(4, dtype=torch.int32, device=DEV) * S)[None].expand(b, 4).contiguous()
    r = R.reference(q, k, torch.zeros_like(k), ids_q, ids_k, False)
    m, l = MR.made_stats(r)
    w = (torch.rand((b, sq), generator=g, device=DEV) + 0.25).contiguous()
    kw = (torch.rand((HEADS, b * sk), generator=g, device=DEV) * 3.75 + 0.25).contiguous()
    kv = torch.stack([k, torch.zeros_like(k)], dim=2).bfloat16()
    kws = [kw[:, i * sk:(i + 1) * sk].t().double() for i in range(b)]
    ref, bound = WR.weighted_mass_reference(q, list(k), ids_q, list(ids_k), m, l, seg.cpu(), kws, w)
    got = K.attention_key_mass(q.bfloat16(), kv[:, :, 0], ids_q, ids_k, m, l, seg, w, torch.full((b, HEADS, 3), float("nan"), device=DEV), kw=kw)
    _check("dense/sq%d" % sq, got, ref, bound)
    assert float(got[1, :, 1].max()) == 0.0                               # the all-pad segment: p underflows to exactly 0, times a finite kw


def test_repeat_accumulate_and_each_question_alone():
    c = _case("randn", SEG_A, 100, seed=100)
    m, l = c.made_stats()
    kw, kw2 = _table(c, "rand", seed=2), _table(c, "zeros", seed=3)
    first = _run(c, m, l, c.w, kw)
    assert torch.equal(first, _run(c, m, l, c.w, kw))                      # repeat call: bit-identical
    acc = _run(c, m, l, None, kw2, mass=first.clone(), accumulate=True)
    assert torch.equal(acc, first + _run(c, m, l, None, kw2))              # the second call adds: exactly the fp32 sum
    for i in range(c.b):                                                   # each question alone: its rows in the batch of 3, bit for bit
        assert torch.equal(_run(c, m, l, c.w, kw, which=i)[0], first[i]), i


# ---- norms ------------------------------------------------------------------------------------------------------------------------------
def _values(fam, rows, heads, g):
    x = torch.randn((rows, heads, 64), generator=g, device=DEV)
    if fam == "zero_row":
        x[rows // 2] = 0
        x[0, heads - 1] = 0
    elif fam == "tiny":
        x = x * 2.0 ** -70
    elif fam == "huge":
        x = x * 2.0 ** 60
    return x.bfloat16()


@pytest.mark.parametrize("fam", ["randn", "zero_row", "tiny", "huge"])
@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("rows", [1, 7, 64, 65, 1000])
def test_head_row_norms(rows, heads, fam):
    from emdr2_amd.model import kernels as K
    x = _values(fam, rows, heads, _gen(rows * 16 + heads))
    ref, bound = WR.norms_reference(x.float())
    kv = torch.zeros((rows, 2, heads, 64), dtype=torch.bfloat16, device=DEV)
    kv[:, 0] = float("nan")                                                # the K half next to it is not read
    kv[:, 1] = x
    got = K.head_row_norms(kv[:, 1])                                       # the strided view of the packed KV projection
    assert got.shape == (heads, rows) and got.dtype == torch.float32
    _check("norms/packed/%s/%dx%d" % (fam, rows, heads), got, ref, bound)
    assert torch.equal(got, K.head_row_norms(kv[:, 1]))                    # no atomics: identical bits
    b = 8 if rows % 8 == 0 else 1                                          # the dense [b, sk, ...] form: row r = b * sk + s
    dense = K.head_row_norms(kv.reshape(b, rows // b, 2, heads, 64)[:, :, 1])
    assert torch.equal(dense, got)
    out = torch.full((heads, rows + 3), -1.0, device=DEV)                  # a wider table: ld > rows, the columns behind stay untouched
    assert K.head_row_norms(kv[:, 1], out=out) is out and torch.equal(out[:, :rows], got) and bool((out[:, rows:] == -1.0).all())
    if fam == "zero_row":
        assert float(got[:, rows // 2].abs().max()) == 0.0 and float(got[heads - 1, 0]) == 0.0
    if fam in ("randn", "huge"):                                           # inside the contract's range the bound is relative
        live = ref > 0
        assert float((bound[live] / ref[live]).max()) < 12.1 * 2.0 ** -24


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_norms_from_the_kernel_fed_to_the_weighted_mass():
    """kw = head_row_norms(v view); the reference takes the TRUE norms of V in float64 and the norms bound as kw_errs."""
    from emdr2_amd.model import kernels as K
    c = _case("randn", SEG_A, 32, seed=32)
    m, l = c.made_stats()
    kw = K.head_row_norms(c.kv[:, 1])
    assert kw.shape == (HEADS, c.seqs.rows) and float(kw[:, c.seqs.total:].abs().max()) == 0.0     # the layout's zero tail rows
    true, err = WR.norms_reference(c.kv[:, 1].float())
    cu = c.seqs.cu.tolist()
    ref, bound = WR.weighted_mass_reference(c.q32, c.k32, c.ids_q, c.ids_k, m, l, c.seg.cpu(), [true[:, cu[i]:cu[i + 1]].t() for i in range(c.b)],
                                            c.w, kw_errs=[err[:, cu[i]:cu[i + 1]].t() for i in range(c.b)])
    _check("end-to-end", _run(c, m, l, c.w, kw), ref, bound)
