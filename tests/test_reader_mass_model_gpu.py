"""GPU: `EMDR2Model.reader_attention_mass` -- the FiD decoder's cross-attention mass per retrieved passage (kernels.ATTN_MASS,
csrc/attention_mass.hip) through the model: what is recorded and what is not, the result against a float64 recomputation from the kept
operands, and that the flag changes nothing else.

The model is the tiny EMDR2 model of tests/test_microbatch_gpu.py (2 layers, hidden 128, two heads of 64 channels) with K = 3 passages:
the fixture of tests/model_fixture.py has heads of 16 channels, which the flag refuses (tests/test_attention_mass_cpu.py)."""
import re

import numpy as np
import pytest
import torch

from tests import attention_mass_ref as MR
from tests import attention_ref as R
from tests.test_microbatch_gpu import _FixedRetriever, _cfg, _clear, _fb, _grads, _ids

pytestmark = pytest.mark.gpu
LAYERS, KK = 2, 3
_ATOMIC = re.compile(r"layernorm\.(weight|bias)$|embeddings\.weight$")      # gradients accumulated by fp32 atomics (csrc/layernorm.hip, csrc/embedding.hip)


def _case(flag=True, seed=7, B=4, S_ret=32, S=64, L=32, V=640, checkpoint=False, qext=None):
    from emdr2_amd.model import kernels as K
    from emdr2_amd.model.emdr2_model import EMDR2Model
    rng = np.random.default_rng(seed)
    qb, ctx = _ids(rng, (B, S_ret), 512), _ids(rng, (B, KK, S_ret), 512)
    qext_, qone = _ids(rng, (B * KK, S), 600), _ids(rng, (B * KK, S), 600)
    qext = qext_ if qext is None else qext
    dec = _ids(rng, (B, L), 600)
    labels = torch.roll(dec, -1, 1); labels[:, -1] = 0
    retr = _FixedRetriever(ctx, torch.zeros_like(ctx), qext, qone)
    torch.manual_seed(0)
    K.DROPOUT._sites = 0
    m = EMDR2Model(retr, _cfg(0.0), V, 512, KK, S, S_ret, cls_id=2, sep_id=3, checkpoint_activations=checkpoint, reader_attention_mass=flag)
    g = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.05 * torch.randn(q.shape, generator=g, device="cuda"))
    m.train()
    batch = dict(uid=-torch.arange(1, B + 1, device="cuda"), q=qb, types=torch.zeros_like(qb), qlen=(qb != 0).sum(1), dec=dec, labels=labels,
                 mask=(labels != 0).float())
    return m, retr, batch


@pytest.fixture()
def keep():
    from emdr2_amd.model import kernels as K
    K.ATTN_MASS.keep, K.ATTN_MASS.calls = True, []
    yield K.ATTN_MASS
    K.ATTN_MASS.keep, K.ATTN_MASS.calls = False, []
    assert K.ATTN_MASS.ids_k is None                                     # nothing leaves the collector armed


def _recompute(calls):
    """The calls of ONE question group (its decoder layers, or its decoding steps x layers) -> (normalised mass float64 [b, K], bound):
    float64 masses from the kept operands and the kept statistics, summed over calls and heads, normalised per question."""
    from emdr2_amd.model import kernels as K
    x = bx = None
    for c in calls:
        q, k, ids_k = c["q"].float(), c["k"].float(), c["ids_k"]
        b = q.shape[0]
        if isinstance(ids_k, K.PackedSeqs):
            cu = ids_k.cu.tolist()
            ks, iks = [k[cu[i]:cu[i + 1]] for i in range(b)], [ids_k.ids[cu[i]:cu[i + 1]] for i in range(b)]
        else:
            ks, iks = list(k), list(ids_k)
        mass, bound, _ = MR.mass_reference(q, ks, c["ids_q"], iks, c["m"], c["l"], c["seg"].cpu(), c["w"])
        x = mass.sum(1) if x is None else x + mass.sum(1)
        bx = bound.sum(1) if bx is None else bx + bound.sum(1)
    tot = x.sum(1, keepdim=True)
    live = tot > 0
    xn = torch.where(live, x / torch.where(live, tot, torch.ones_like(tot)), torch.zeros_like(x))
    # d(x / tot) <= (dx + (x / tot) sum dx) / tot; plus the fp32 sums over calls and heads and the division (8 roundings)
    bn = torch.where(live, (bx + xn * bx.sum(1, keepdim=True)) / torch.where(live, tot, torch.ones_like(tot)), torch.zeros_like(x))
    return xn, bn + 8 * 2.0 ** -24 * xn + R.TINY


def _check(tag, got, ref, bound):
    ratio, idx = R.worst(got, ref, bound)
    print("[reader-mass] %s worst err/bound %.3f at %s" % (tag, ratio, idx))
    assert ratio < 1.0, (tag, ratio, idx)


@pytest.mark.parametrize("packing", [True, False])
def test_recorded_calls_and_the_mass_against_the_kept_operands(packing, keep):
    from emdr2_amd.model import kernels as K
    K.PACKING.enabled = packing
    try:
        m, _, bt = _case()
        _fb(m, bt, 2)
        groups = 2
        assert len(keep.calls) == LAYERS * groups                         # decoder layers x groups: nothing from the one-context pass
        for c in keep.calls:
            assert tuple(c["q"].shape[:2]) == (2, 32) and c["seg"].shape == (2, KK + 1)     # a group's questions, not its B K one-context sequences
            assert (c["ids_k"].group == KK) if packing else (tuple(c["ids_k"].shape) == (2, KK * 64))
        mass = m.last_attention_mass
        assert mass.shape == (4, KK) and mass.dtype == torch.float32
        assert torch.allclose(mass.sum(1), torch.ones(4, device="cuda"), atol=1e-5)
        for gi in range(groups):
            ref, bound = _recompute(keep.calls[gi * LAYERS:(gi + 1) * LAYERS])
            _check("train/packing=%s/group%d" % (packing, gi), mass[2 * gi:2 * gi + 2], ref, bound)
    finally:
        K.PACKING.enabled = True


def test_flag_on_changes_no_logit_no_loss_and_no_gradient():
    from emdr2_amd.model.emdr2_model import emdr2_loss
    res = []
    for flag in (False, True):
        m, _, bt = _case(flag)
        lm, tlp, one = m(bt["uid"], bt["q"], bt["types"], None, bt["q"], bt["qlen"], bt["dec"])
        loss, _ = emdr2_loss(lm, tlp, one, bt["labels"], bt["mask"], 601)
        loss.backward()
        res.append((lm.detach().clone(), loss.detach().clone(), _grads(m), m.last_attention_mass))
    (lm0, loss0, g0, mass0), (lm1, loss1, g1, mass1) = res
    assert mass0 is None and mass1 is not None
    assert torch.equal(lm0, lm1) and torch.equal(loss0, loss1)
    assert set(g0) == set(g1)
    n_exact = 0
    for k in g0:
        if _ATOMIC.search(k):
            # LayerNorm weights / biases and the embedding tables: the blocks of their backward kernels add their partial sums into the
            # gradient with fp32 atomics (csrc/layernorm.hip, csrc/embedding.hip), in whatever order the blocks finish, so these gradients are not
            # bit-reproducible between two runs of the SAME code (measured on this very case, four runs with the flag off: 26 - 29 of
            # the 129 gradients differ from the first run, all of them of this kind, by 7e-9 .. 2e-7 of the tensor's largest value;
            # four runs with the flag on: 26 - 27, same tensors, same size).  The partial sums themselves are deterministic, so what
            # two runs can differ by is the reordering of N <= 32 of them: 2 (N - 1) 2^-24 sum |partials| <= 2^-18 sum |partials|;
            # with 2^-16 of the largest gradient value the test allows the partials a cancellation of four.
            tol = 2.0 ** -16 * float(g0[k].abs().max())
            assert float((g0[k] - g1[k]).abs().max()) <= tol, k
        else:
            assert torch.equal(g0[k], g1[k]), k                          # every GEMM weight and bias, of every layer and tower: bit-identical
            n_exact += 1
    assert n_exact >= 70, n_exact


def test_a_questions_mass_does_not_depend_on_its_group():
    m, retr, bt = _case()
    _fb(m, bt, 1)
    one = m.last_attention_mass.clone()
    _clear(m)
    _fb(m, bt, 2)
    assert torch.equal(one, m.last_attention_mass)                         # training: micro_batches 1 against 2
    m.eval()
    with torch.no_grad():
        m(bt["uid"], bt["q"], bt["types"], None, bt["q"], bt["qlen"], bt["dec"])
        whole = m.last_attention_mass.clone()
        full = retr.out
        halves = []
        for lo, hi in ((0, 2), (2, 4)):                                    # evaluation mode: the batch of 4 against two batches of 2
            retr.out = (full[0][lo:hi], full[1][lo:hi], full[2][lo * KK:hi * KK], full[3][lo * KK:hi * KK], None, None)
            m(bt["uid"][lo:hi], bt["q"][lo:hi], bt["types"][lo:hi], None, bt["q"][lo:hi], bt["qlen"][lo:hi], bt["dec"][lo:hi])
            halves.append(m.last_attention_mass.clone())
        retr.out = full
    assert torch.equal(whole, torch.cat(halves))


def test_checkpointed_activations_do_not_count_twice(keep):
    from emdr2_amd.model.emdr2_model import emdr2_loss
    masses = []
    for ckpt in (False, True):
        keep.calls = []
        m, _, bt = _case(checkpoint=ckpt)
        lm, tlp, one = m(bt["uid"], bt["q"], bt["types"], None, bt["q"], bt["qlen"], bt["dec"])
        loss, _ = emdr2_loss(lm, tlp, one, bt["labels"], bt["mask"], 601)
        loss.backward()                                                   # the checkpointed layers are re-run here: nothing may be recorded
        assert len(keep.calls) == LAYERS, (ckpt, len(keep.calls))
        masses.append(m.last_attention_mass.clone())
    assert torch.equal(masses[0], masses[1])


def test_greedy_decoding_accumulates_over_steps_with_the_stated_weights(keep):
    from emdr2_amd.model.search_strategy import SampleOrGreedySearch
    m, _, bt = _case()
    m.eval()
    L, args = 6, (bt["uid"], bt["q"], bt["types"], None, bt["q"], bt["qlen"])
    probe = SampleOrGreedySearch(max_decode_len=L, bos_id=1, eos_id=639, topk_evidence=KK, keep_logits=True)
    probe.generate_output(m, *args)
    tokens = torch.stack([lg.argmax(1) for lg in probe.last_logits]).T     # [b, steps]
    # an [EOS] id under which some hypothesis ends while another goes on: the weights then differ between the questions of a step
    eos = None
    for cand in tokens.unique().tolist():
        ends = [min([i for i in range(tokens.shape[1]) if int(tokens[b, i]) == cand] + [L]) for b in range(4)]
        if min(ends) < max(ends) and min(ends) < L - 1:
            eos = cand
            break
    assert eos is not None, tokens
    keep.calls = []
    search = SampleOrGreedySearch(max_decode_len=L, bos_id=1, eos_id=eos, topk_evidence=KK, keep_logits=True)
    search.generate_output(m, *args)
    steps = len(search.last_logits)
    assert len(keep.calls) == steps * LAYERS
    tokens = torch.stack([lg.argmax(1) for lg in search.last_logits]).T
    ended = torch.zeros(4, dtype=torch.bool, device="cuda")
    for i in range(steps):                                                 # weight 1 for hypotheses that had not emitted [EOS] BEFORE step i
        for c in keep.calls[i * LAYERS:(i + 1) * LAYERS]:
            assert tuple(c["q"].shape[:2]) == (4, 1) and not isinstance(c["ids_k"], type(None))
            assert torch.equal(c["w"][:, 0], (~ended).float()), i
        ended = ended | (tokens[:, i] == eos)
    assert bool(ended.any()) and steps >= 2
    ref, bound = _recompute(keep.calls)
    _check("greedy", m.last_attention_mass, ref, bound)


def test_a_dominating_passage_is_the_most_read_one():
    """Question b's passage (b % K) keeps its tokens, its other passages are cut to two tokens: the decoder can hardly read anything else.
    The most-read slot is that passage, and the meter's `read top1 hit` says so when the hit slots name it -- and 0 when they name another."""
    from emdr2_amd.tasks.openqa.e2eqa.reader_mass import ReaderMassMeter
    B = 4
    rng = np.random.default_rng(11)
    qext = _ids(rng, (B * KK, 64), 600)
    gold = torch.arange(B, device="cuda") % KK
    for b in range(B):
        for g in range(KK):
            if g != int(gold[b]):
                qext[b * KK + g, 2:] = 0
    m, _, bt = _case(qext=qext)
    hits = torch.zeros((B, KK), dtype=torch.bool, device="cuda")
    hits[torch.arange(B), gold] = True

    class Tracker(object):
        _step_hits = hits
    for tracker_hits, want in ((hits, B), (hits.roll(1, dims=1), 0)):
        Tracker._step_hits = tracker_hits
        m.reader_mass = ReaderMassMeter(KK, Tracker())
        m.reader_mass.begin()
        m(bt["uid"], bt["q"], bt["types"], None, bt["q"], bt["qlen"], bt["dec"])
        m.reader_mass.commit()
        assert torch.equal(m.last_attention_mass.argmax(1), gold)
        line = m.reader_mass.line()
        assert " read top1 hit: %d/%d |" % (want, B) in line, line
        read_mass = float(line.split("read mass:")[1].split("|")[0])
        assert (read_mass > 0.5) == (want == B), line
