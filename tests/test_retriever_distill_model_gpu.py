"""GPU: `EMDR2Model.retriever_distill_attention` and `attention_mass_value_norms` through the model -- the retriever trained towards the
reader's cross-attention mass (FiD-KD), with no one-context pass.

The model is the tiny EMDR2 model of tests/test_reader_mass_model_gpu.py (2 layers, hidden 128, two heads of 64 channels, K = 3), built
here with the same seeds, so that a model with the new switches holds the weights of the one without."""
import math

import numpy as np
import pytest
import torch

from tests import attention_mass_weighted_ref as WR
from tests import attention_ref as R
from tests.test_microbatch_gpu import _FixedRetriever, _cfg, _clear, _fb, _grads, _ids, _rel
from tests.test_reader_mass_model_gpu import _ATOMIC, KK, LAYERS, _recompute, keep  # noqa: F401  (keep: a fixture)

pytestmark = pytest.mark.gpu


def _model(distill=True, norms=False, reader=False, seed=7, B=4, S_ret=32, S=64, L=32, V=640, qext=None):
    """test_reader_mass_model_gpu._case with the new switches."""
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
    m = EMDR2Model(retr, _cfg(0.0), V, 512, KK, S, S_ret, cls_id=2, sep_id=3, reader_attention_mass=reader, retriever_distill_attention=distill,
                   attention_mass_value_norms=norms)
    g = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.05 * torch.randn(q.shape, generator=g, device="cuda"))
    m.train()
    batch = dict(uid=-torch.arange(1, B + 1, device="cuda"), q=qb, types=torch.zeros_like(qb), qlen=(qb != 0).sum(1), dec=dec, labels=labels,
                 mask=(labels != 0).float())
    return m, retr, batch


def _forward(m, bt):
    return m(bt["uid"], bt["q"], bt["types"], None, bt["q"], bt["qlen"], bt["dec"])


def _count_encoder(m, monkeypatch):
    """Counts the entries into the reader encoder (either layout)."""
    n = {"calls": 0}
    lm = m.language_model
    for name in ("encode_packed", "encode"):
        orig = getattr(lm, name)

        def counted(*a, _orig=orig, **kw):
            n["calls"] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(lm, name, counted)
    return n


def _kl64(tlp, target, batch):
    """distill_kl in float64 on a float64 target; differentiable in tlp."""
    t = target.double()
    pos = t > 0
    return torch.where(pos, t * (torch.log(torch.where(pos, t, torch.ones_like(t))) - tlp.double()), torch.zeros_like(t)).sum() / batch


def _kl_tolerance(tlp, ref, bound, batch):
    """|distill_kl(fp32 target) - _kl64(ref)| given |target - ref| <= bound: f(t) = t (ln t - logp), |f'| <= |ln t_lo| + 1 + |logp| on the
    interval (t <= 1: |ln| is largest at its lower end, taken no lower than TINY); plus distill_kl's own fp32 roundings: ln, the
    subtraction, the product and a sum of b K terms."""
    t_lo = torch.clamp(ref - bound, min=R.TINY)
    slope = torch.log(t_lo).abs() + 1.0 + tlp.double().abs()
    terms = ref * (torch.log(torch.clamp(ref, min=R.TINY)).abs() + tlp.double().abs())
    return float((bound * slope).sum() / batch + (ref.numel() + 5) * 2.0 ** -24 * terms.sum() / batch)


def test_no_one_context_pass_and_the_fid_pass_is_unchanged(keep, monkeypatch):  # noqa: F811
    from emdr2_amd.model.emdr2_model import OneContextLogits, ReadTarget
    m0, _, bt = _model(distill=False)
    n0 = _count_encoder(m0, monkeypatch)
    lm0, tlp0, one0 = _forward(m0, bt)
    assert isinstance(one0, OneContextLogits) and n0["calls"] == 2 and len(keep.calls) == 0      # FiD pass + one-context pass, nothing recorded
    m1, _, bt = _model(distill=True)
    n1 = _count_encoder(m1, monkeypatch)
    lm1, tlp1, one1 = _forward(m1, bt)
    assert n1["calls"] == 1 and len(keep.calls) == LAYERS
    assert isinstance(one1, ReadTarget) and one1.shape == (4, KK) and not one1.mass.requires_grad
    assert torch.equal(lm0, lm1) and torch.equal(tlp0, tlp1)
    assert torch.equal(one1.mass, m1.last_attention_mass)
    assert m1.reader_mass is None and not m1.reader_attention_mass          # the meter stays tied to the reader-attention-mass switch
    # under forward_backward: once per group, and the collector's calls are decoder layers x groups
    keep.calls = []
    n1["calls"] = 0
    _fb(m1, bt, 2)
    assert n1["calls"] == 2 and len(keep.calls) == LAYERS * 2
    n0["calls"] = 0
    _fb(m0, bt, 2)
    assert n0["calls"] == 4
    # evaluation mode: the eval-mode 4-tuple, the mass still collected
    m1.eval()
    with torch.no_grad():
        out = _forward(m1, bt)
    assert len(out) == 4 and m1.last_attention_mass.shape == (4, KK)


def test_loss_against_the_float64_target_and_where_its_gradients_go(keep):  # noqa: F811
    from emdr2_amd.model.emdr2_model import emdr2_loss
    m, _, bt = _model()
    B = 4
    lm, tlp, one = _forward(m, bt)
    tlp.retain_grad()
    loss, stats = emdr2_loss(lm, tlp, one, bt["labels"], bt["mask"], 601)
    ref, bound = _recompute(keep.calls)
    want = float(_kl64(tlp.detach(), ref, B))
    tol = _kl_tolerance(tlp.detach(), ref, bound, B)
    got = float(stats["retriever_loss"])
    print("[distill] retriever_loss %.7f, float64 %.7f, |diff| %.3g, tolerance %.3g" % (got, want, abs(got - want), tol))
    assert got > 0 and abs(got - want) <= tol
    assert abs(float(loss.detach()) - (float(stats["lm_loss"]) + got)) <= 2.0 ** -23 * abs(float(loss.detach()))
    loss.backward()
    g = _grads(m)
    # the gradient that enters the prior is -t / B: the target's own bound and two fp32 roundings
    err = (tlp.grad.double() + ref / B).abs()
    assert bool((err <= bound / B + 2 * 2.0 ** -24 * ref / B + R.TINY).all())
    # the towers: the same float64-built loss back-propagated through the model's own prior.  The towers' backward runs in bf16: a change of
    # the incoming gradient the size of the target's bound can move individual bf16 roundings, so the two agree to one bf16 ulp (2^-8) of
    # each gradient's norm, not to fp32 -- a wrong target (another question's row, an unnormalised mass) is off by O(1)
    _clear(m)
    lm2, tlp2, _ = _forward(m, bt)
    _kl64(tlp2, ref, B).float().backward()
    g2 = _grads(m)
    towers = [k for k in g if k.startswith("retriever_model.")]
    assert len(towers) > 20 and set(towers) == set(k for k in g2 if k.startswith("retriever_model."))
    assert any("query_model" in k for k in towers) and any("context_model" in k for k in towers)
    worst = max(_rel(g[k], g2[k]) for k in towers)
    print("[distill] tower gradients against the float64-built loss: worst relative difference %.3g" % worst)
    assert worst <= 2.0 ** -8
    assert not any(k.startswith("language_model.") for k in g2)             # the float64 loss alone reaches no reader parameter
    # the reader: exactly the gradients of the LM loss alone -- the target is a constant
    _clear(m)
    lm3, tlp3, _ = _forward(m, bt)
    lm_only, _ = emdr2_loss(lm3, tlp3, None, bt["labels"], bt["mask"], 601)
    lm_only.backward()
    g3 = _grads(m)
    reader = [k for k in g if k.startswith("language_model.")]
    assert len(reader) > 40 and set(reader) == set(g3)
    for k in reader:
        if _ATOMIC.search(k):                                              # fp32 atomics: test_reader_mass_model_gpu's tolerance and reasons
            assert float((g[k] - g3[k]).abs().max()) <= 2.0 ** -16 * float(g3[k].abs().max()), k
        else:
            assert torch.equal(g[k], g3[k]), k


def test_groups_of_questions_give_the_same_loss_and_gradients():
    """micro_batches 1, 2 and 3 (4 questions: 2 + 1 + 1); the tolerances of test_microbatch_gpu.test_kl_div_variant_and_argument_checks."""
    m, _, bt = _model()
    l1, s1 = _fb(m, bt, 1)
    g1 = _grads(m)
    mass1 = m.last_attention_mass.clone()
    assert float(s1["retriever_loss"]) > 0
    for micro in (2, 3):
        _clear(m)
        l2, s2 = _fb(m, bt, micro)
        assert abs(float(l1) - float(l2)) < 2e-6 * abs(float(l1)) and abs(float(s1["retriever_loss"]) - float(s2["retriever_loss"])) < 1e-6, micro
        g2 = _grads(m)
        assert set(g2) == set(g1) and max(_rel(g2[k], g1[k]) for k in g1) < 2e-5, micro
        assert torch.equal(m.last_attention_mass, mass1)                    # a question's target does not depend on its group


def _recompute_weighted(calls):
    """test_reader_mass_model_gpu._recompute for value-norm weighted calls: the float64 mass from the kept q, k, v -- the TRUE norms of v,
    the norms kernel's bound as the table's error -- and the kept table itself against that bound."""
    from emdr2_amd.model import kernels as K
    x = bx = None
    for c in calls:
        q, k, v, ids_k = c["q"].float(), c["k"].float(), c["v"].float(), c["ids_k"]
        b = q.shape[0]
        true, err = WR.norms_reference(v.reshape((-1,) + tuple(v.shape[-2:])))
        ratio = R.worst(c["kw"][:, :true.shape[1]], true, err)[0]
        assert ratio < 1.0, ratio
        if isinstance(ids_k, K.PackedSeqs):
            cu = ids_k.cu.tolist()
            cut = [(cu[i], cu[i + 1]) for i in range(b)]
            ks, iks = [k[lo:hi] for lo, hi in cut], [ids_k.ids[lo:hi] for lo, hi in cut]
        else:
            sk = k.shape[1]
            cut = [(i * sk, (i + 1) * sk) for i in range(b)]
            ks, iks = list(k), list(ids_k)
        mass, bound = WR.weighted_mass_reference(q, ks, c["ids_q"], iks, c["m"], c["l"], c["seg"].cpu(), [true[:, lo:hi].t() for lo, hi in cut], c["w"],
                                                 kw_errs=[err[:, lo:hi].t() for lo, hi in cut])
        x = mass.sum(1) if x is None else x + mass.sum(1)
        bx = bound.sum(1) if bx is None else bx + bound.sum(1)
    tot = x.sum(1, keepdim=True)
    live = tot > 0
    xn = torch.where(live, x / torch.where(live, tot, torch.ones_like(tot)), torch.zeros_like(x))
    bn = torch.where(live, (bx + xn * bx.sum(1, keepdim=True)) / torch.where(live, tot, torch.ones_like(tot)), torch.zeros_like(x))
    return xn, bn + 8 * 2.0 ** -24 * xn + R.TINY


def _check(tag, got, ref, bound):
    ratio, idx = R.worst(got, ref, bound)
    print("[distill] %s worst err/bound %.3f at %s" % (tag, ratio, idx))
    assert ratio < 1.0, (tag, ratio, idx)


@pytest.mark.parametrize("packing", [True, False])
def test_value_norms_through_the_model(packing, keep):  # noqa: F811
    from emdr2_amd.model import kernels as K
    K.PACKING.enabled = packing
    try:
        m, _, bt = _model(norms=True)
        plain, _, _ = _model(norms=False)
        _fb(m, bt, 2)
        assert len(keep.calls) == LAYERS * 2 and all("v" in c and "kw" in c for c in keep.calls)
        assert K.ATTN_MASS.norms == {}                                      # disarm dropped the cache
        mass = m.last_attention_mass
        assert torch.allclose(mass.sum(1), torch.ones(4, device="cuda"), atol=1e-5)
        for gi in range(2):
            ref, bound = _recompute_weighted(keep.calls[gi * LAYERS:(gi + 1) * LAYERS])
            _check("norms/packing=%s/group%d" % (packing, gi), mass[2 * gi:2 * gi + 2], ref, bound)
        _fb(plain, bt, 2)
        assert not torch.equal(plain.last_attention_mass, mass)             # it IS another quantity
    finally:
        K.PACKING.enabled = True


def test_value_norms_under_greedy_decoding_are_computed_once_per_layer(keep):  # noqa: F811
    from emdr2_amd.model import kernels as K
    from emdr2_amd.model.search_strategy import SampleOrGreedySearch
    m, _, bt = _model(norms=True)
    m.eval()
    search = SampleOrGreedySearch(max_decode_len=5, bos_id=1, eos_id=639, topk_evidence=KK, keep_logits=True)
    search.generate_output(m, bt["uid"], bt["q"], bt["types"], None, bt["q"], bt["qlen"])
    steps = len(search.last_logits)
    assert steps >= 2 and len(keep.calls) == steps * LAYERS
    assert K.ATTN_MASS.norm_launches == LAYERS                              # not steps x layers: the cached K/V projection is one tensor per layer
    for layer in range(LAYERS):
        assert all(c["kw"] is keep.calls[layer]["kw"] for c in keep.calls[layer::LAYERS])
    ref, bound = _recompute_weighted(keep.calls)
    _check("norms/greedy", m.last_attention_mass, ref, bound)


def test_it_trains_the_prior_towards_the_most_read_passage():
    """The dominating-passage inputs of test_reader_mass_model_gpu (question b reads passage b % K), the reader frozen so that the target
    is constant, 8 Adam steps (torch.optim.Adam, learning rate 1e-3: every weight moves by about 1e-3 per step, a few bf16 ulps of the
    0.07-sized weights, whatever the gradient's scale) on the retriever's parameters alone, fixed seeds, no dropout: the distillation loss
    falls and the prior moves onto the most-read slots."""
    from emdr2_amd.model.emdr2_model import distill_kl
    from emdr2_amd.model import kernels as K
    B, steps, lr = 4, 8, 1e-3
    rng = np.random.default_rng(11)
    qext = _ids(rng, (B * KK, 64), 600)
    gold = torch.arange(B, device="cuda") % KK
    for b in range(B):
        for g in range(KK):
            if g != int(gold[b]):
                qext[b * KK + g, 2:] = 0
    m, _, bt = _model(qext=qext)
    for p in m.language_model.parameters():
        p.requires_grad_(False)
    opt = torch.optim.Adam([p for p in m.retriever_model.parameters()], lr=lr)
    losses, on_gold, target = [], [], None
    for _ in range(steps + 1):
        _clear(m)
        lm, tlp, one = _forward(m, bt)
        if target is None:
            target = one.mass.clone()
            assert torch.equal(target.argmax(1), gold)
        assert torch.equal(one.mass, target)                                # the frozen reader: a constant target
        loss = distill_kl(tlp, one.mass, B)
        losses.append(float(loss.detach()))
        on_gold.append(float(tlp.detach().exp()[torch.arange(B), gold].sum()))
        loss.backward()
        opt.step()
        K.WEIGHTS.invalidate()                                              # (the bf16 working copies follow the masters)
    print("[distill] loss %s; prior on the most-read slots %s" % (["%.4f" % v for v in losses], ["%.3f" % v for v in on_gold]))
    assert losses[-1] < losses[0] and on_gold[-1] > on_gold[0]
    assert math.isfinite(losses[-1])
