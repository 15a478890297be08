"""GPU: emdr2_attention_key_mass (csrc/attention_mass.hip) against the float64 reference and bound of tests/attention_mass_ref.py.

Pass criterion everywhere: worst |kernel - reference| / bound < 1 over every (question, head, segment).  The bound is derived there from
the kernel's order of operations and is not tuned; the worst ratios measured per family are recorded in
profiles/reader_attention_mass.txt.  Shapes: segment boundaries inside a 16-key MFMA group and inside a 32-key step, groups that straddle
several segments, empty segments, 100 short segments, one segment of 4,200 keys (66 groups per wave), uncovered keys before the first
and after the last boundary, every query-tile count (sq 1, 32, 100, 128), dense keys with padding in every segment's tail and one
all-pad segment.  Statistics: made by the test, and taken from the project's own forward on its split-key and on its varlen route."""
import pytest
import torch

from tests import attention_mass_ref as MR
from tests import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
HEADS = 2

SEG_A = ([1, 31, 33, 64, 0], [65, 127, 128, 129, 3], [512, 0, 0, 1, 700])
SEG_100 = ([(7 * i) % 40 + 1 for i in range(100)], [(11 * i + 5) % 40 + 1 for i in range(100)])
SEG_LONG = ([4200], [100])


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


class Case(object):
    """Packed keys: question b owns `lead[b]` uncovered keys, its segments, `trail[b]` uncovered keys."""

    def __init__(self, fam, seg_lens, sq, lead=None, trail=None, seed=0, pos_div=1):
        from emdr2_amd.model import kernels as K
        b = len(seg_lens)
        lead, trail = lead or [0] * b, trail or [0] * b
        lens = [lead[i] + sum(seg_lens[i]) + trail[i] for i in range(b)]
        ids = torch.zeros((b, max(lens)), dtype=torch.int64, device=DEV)
        for i, n in enumerate(lens):
            ids[i, :n] = 7
        self.seqs = K.PackedSeqs(ids)
        g = _gen(100 + seed)
        parts = [R.family(fam, 1, HEADS, sq, n, 64, g, DEV, (torch.arange(n, device=DEV) // pos_div)[None]) for n in lens]
        self.q32 = torch.cat([p[0] for p in parts])                                    # [b, sq, heads, 64] fp32 holding bf16 values
        self.k32 = [p[1][0] for p in parts]
        kv = torch.zeros((self.seqs.rows, 2, HEADS, 64), device=DEV)
        kv[:self.seqs.total, 0] = torch.cat(self.k32)
        kv[:self.seqs.total, 1] = torch.cat([p[2][0] for p in parts])
        self.kv = kv.bfloat16()
        self.q = self.q32.bfloat16()
        self.ids_q = torch.full((b, sq), 7, dtype=torch.int64, device=DEV)
        for i in range(b):                                                             # some id-0 queries (never all of a question's)
            self.ids_q[i, (3 * i + 1) % sq:(3 * i + 1) % sq + (1 if sq > 1 and i else 0)] = 0
        if sq >= 32:
            self.ids_q[0, sq - 5:] = 0
        seg = torch.zeros((b, len(seg_lens[0]) + 1), dtype=torch.int64)
        for i in range(b):
            seg[i] = torch.tensor([lead[i]] + seg_lens[i]).cumsum(0)
        self.seg = seg.to(torch.int32).to(DEV)
        self.w = (torch.rand((b, sq), generator=g, device=DEV) + 0.25).contiguous()
        self.ids_k = [torch.full((n,), 7, dtype=torch.int64, device=DEV) for n in lens]
        self.b, self.sq, self.G = b, sq, len(seg_lens[0])
        self._stats = {}

    def made_stats(self):
        if "made" not in self._stats:
            ml = []
            for i in range(self.b):
                r = R.reference(self.q32[i][None], self.k32[i][None], torch.zeros_like(self.k32[i])[None], self.ids_q[i][None], self.ids_k[i][None], False)
                ml.append(MR.made_stats(r))
            self._stats["made"] = (torch.cat([m for m, _ in ml]).contiguous(), torch.cat([l for _, l in ml]).contiguous())
        return self._stats["made"]

    def forward_stats(self):
        """(m, l) of the project's forward over these operands, on the route its dispatch takes."""
        from emdr2_amd.model import kernels as K
        out = K.attention_core(self.q.clone().requires_grad_(True), self.kv.clone().requires_grad_(True), self.ids_q, self.seqs, False)
        m, l = (t.detach().clone() for t in out.grad_fn.saved_tensors[2:4])
        return m, l, out.grad_fn.launch.ksplit

    def run(self, m, l, w, mass=None, accumulate=False, which=None):
        from emdr2_amd.model import kernels as K
        if which is None:
            mass = torch.full((self.b, HEADS, self.G), float("nan"), device=DEV) if mass is None else mass
            return K.attention_key_mass(self.q, self.kv[:, 0], self.ids_q, self.seqs, m, l, self.seg, w, mass, accumulate=accumulate)
        # question `which` alone: its own PackedSeqs, its own rows
        i = which
        ids = torch.zeros((1, self.k32[i].shape[0]), dtype=torch.int64, device=DEV) + 7
        seqs = K.PackedSeqs(ids)
        kv = torch.zeros((seqs.rows, 2, HEADS, 64), device=DEV)
        kv[:seqs.total, 0] = self.k32[i]
        mass = torch.full((1, HEADS, self.G), float("nan"), device=DEV)
        return K.attention_key_mass(self.q[i:i + 1].contiguous(), kv.bfloat16()[:, 0], self.ids_q[i:i + 1].contiguous(), seqs, m[i:i + 1].contiguous(),
                                    l[i:i + 1].contiguous(), self.seg[i:i + 1].contiguous(), None if w is None else w[i:i + 1].contiguous(), mass)

    def reference(self, m, l, w, forward_stats=False):
        key = ("ref", id(m), w is None, forward_stats)
        if key not in self._stats:
            self._stats[key] = (m, MR.mass_reference(self.q32, self.k32, self.ids_q, self.ids_k, m, l, self.seg.cpu(), w, forward_stats))   # (m kept alive: its id is the key)
        return self._stats[key][1]


_CASES = {}


def _case(*key, **kw):
    k = repr((key, sorted(kw.items())))
    if k not in _CASES:
        _CASES[k] = Case(*key, **kw)
    return _CASES[k]


def _check(tag, got, ref, bound):
    ratio, idx = R.worst(got, ref, bound)
    print("[attn-mass] %s worst err/bound %.3f at %s (ref %.4g, got %.4g)" % (tag, ratio, idx, float(ref[idx]), float(got[idx])))
    assert ratio < 1.0, (tag, ratio, idx)
    return ratio


# scores: randn; one_hot = a key that leads its row by 40 (|s| up to ~40); stair_up = 6 per 32 keys: P underflows 90 below the maximum
@pytest.mark.parametrize("fam", ["randn", "one_hot", "stair_up"])
@pytest.mark.parametrize("sq", [1, 32, 100, 128])
def test_segment_shapes_and_query_tiles(fam, sq):
    c = _case(fam, SEG_A, sq, seed=sq)
    m, l = c.made_stats()
    for tag, w in (("w", c.w), ("w=NULL", None)):
        ref, bound, _ = c.reference(m, l, w)
        _check("A/%s/sq%d/%s" % (fam, sq, tag), c.run(m, l, w), ref, bound)
    assert float(c.run(m, l, None)[0, :, 4].abs().max()) == 0.0 and float(c.run(m, l, None)[2, :, 1:3].abs().max()) == 0.0      # empty segments: exactly 0


@pytest.mark.parametrize("fam", ["randn", "stair_up"])
def test_hundred_short_segments(fam):
    c = _case(fam, SEG_100, 32, seed=7)
    m, l = c.made_stats()
    ref, bound, _ = c.reference(m, l, c.w)
    _check("100seg/%s" % fam, c.run(m, l, c.w), ref, bound)


@pytest.mark.parametrize("fam", ["randn", "stair_up"])
def test_long_segment_and_uncovered_keys(fam):
    """One segment of 4,200 keys; 50 / 10 keys before the first boundary and 50 / 40 after the last belong to no segment."""
    c = _case(fam, SEG_LONG, 32, lead=[50, 10], trail=[50, 40], seed=9, pos_div=8)
    m, l = c.made_stats()
    ref, bound, rows = c.reference(m, l, None)
    got = c.run(m, l, None)
    _check("long/%s" % fam, got, ref, bound)
    real = (c.ids_q != 0).sum(dim=1).double()
    assert bool((ref.sum(dim=2) < real[:, None] - 1e-9).any())            # the uncovered keys hold mass the segments do not see


def test_covering_segments_sum_to_the_number_of_real_queries():
    c = _case("randn", SEG_A, 100, seed=100)
    m, l = c.made_stats()
    ref, bound, _ = c.reference(m, l, None)
    got = c.run(m, l, None)
    real = (c.ids_q != 0).sum(dim=1).double()[:, None].expand(c.b, HEADS)
    err = (got.double().sum(dim=2) - real).abs()
    # the reference's own rows sum to 1 up to the fp32 rounding of the test-made l: one more 2^-24 per real query
    assert bool((err <= bound.sum(dim=2) + real * 2.0 ** -24).all()), (err, bound.sum(dim=2))


def test_accumulate_repeat_and_alone():
    c = _case("randn", SEG_A, 100, seed=100)
    m, l = c.made_stats()
    first = c.run(m, l, c.w)
    again = c.run(m, l, c.w)
    assert torch.equal(first, again)                                     # repeat call: bit-identical
    acc = c.run(m, l, None, mass=first.clone(), accumulate=True)
    assert torch.equal(acc, first + c.run(m, l, None))                   # the second call adds: exactly the fp32 sum
    for i in range(c.b):                                                 # each question alone: bit-identical to its rows in the batch of 3
        assert torch.equal(c.run(m, l, c.w, which=i)[0], first[i]), i


@pytest.mark.parametrize("fam", ["randn", "stair_up"])
def test_statistics_of_the_projects_forward_on_both_routes(fam, monkeypatch):
    """The same operands through the split-key forward (4,300 keys: three ranges) and, with the plan forced to 1, through the varlen
    forward.  The forward's own error in m + ln l enters the bound (attention_mass_ref: forward_stats)."""
    from emdr2_amd.model import kernels as K
    c = _case(fam, SEG_LONG, 32, lead=[50, 10], trail=[50, 40], seed=9, pos_div=8)
    m, l, ksplit = c.forward_stats()
    assert ksplit > 1
    ref, bound, _ = c.reference(m, l, c.w, forward_stats=True)
    _check("fwd-split/%s" % fam, c.run(m, l, c.w), ref, bound)
    monkeypatch.setattr(K, "_splitkv_plan", lambda *a: (1, 0, 0))
    m1, l1, ksplit1 = c.forward_stats()
    assert ksplit1 == 1
    ref1, bound1, _ = c.reference(m1, l1, c.w, forward_stats=True)
    _check("fwd-varlen/%s" % fam, c.run(m1, l1, c.w), ref1, bound1)
    # and against the TRUE softmax (no statistics given): both routes' masses are the float64 probabilities' within the same bound
    r_true = []
    for i in range(c.b):
        r = R.reference(c.q32[i][None], c.k32[i][None], torch.zeros_like(c.k32[i])[None], c.ids_q[i][None], c.ids_k[i][None], False)
        r_true.append((r.lse, torch.ones_like(r.lse)))                      # float64 "statistics": m + ln l = lse exactly
    mt, lt = torch.cat([a for a, _ in r_true]), torch.cat([b_ for _, b_ in r_true])
    ref_t, bound_t, _ = MR.mass_reference(c.q32, c.k32, c.ids_q, c.ids_k, mt, lt, c.seg.cpu(), c.w, True)
    _check("fwd-split-vs-softmax/%s" % fam, c.run(m, l, c.w), ref_t, bound_t)


@pytest.mark.parametrize("fam", ["randn", "stair_up"])
@pytest.mark.parametrize("sq", [1, 32])
def test_dense_keys_with_padding(fam, sq):
    """sk = 96 = three segments of S = 32; question 0: pad ids in every segment's tail; question 1: segment 1 all padding."""
    from emdr2_amd.model import kernels as K
    b, sk, S = 2, 96, 32
    g = _gen(40 + sq)
    q, k, _, _ = R.family(fam, b, HEADS, sq, sk, 64, g, DEV)
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
    kv = torch.stack([k, torch.zeros_like(k)], dim=2).bfloat16()
    ref, bound, _ = MR.mass_reference(q, list(k), ids_q, list(ids_k), m, l, seg.cpu(), w)
    got = K.attention_key_mass(q.bfloat16(), kv[:, :, 0], ids_q, ids_k, m, l, seg, w, torch.full((b, HEADS, 3), float("nan"), device=DEV))
    _check("dense/%s/sq%d" % (fam, sq), got, ref, bound)
    assert float(got[1, :, 1].max()) == 0.0                               # the all-pad segment: exp(-10000 - lse) underflows to exactly 0
