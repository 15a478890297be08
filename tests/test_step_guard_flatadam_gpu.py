"""GPU: FlatAdam(skip_nonfinite=True) on the two-layer T5Model of tests/test_dist_gpu.py with 1 MiB buckets (several of them).  Clean steps
are the unguarded optimizer's, bit for bit; a step with one NaN among its gradients changes no master, moment or working copy while
every counter moves on, and the report names the element; without the guard the same step poisons the masters; and two data-parallel
ranks, of which one produced the NaN, skip together and stay bit-identical.  Twins are compared under kernels.ORDERED
(--deterministic-gradients): two backward passes then give the same gradient bits."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.test_dist_gpu import _init

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture()
def ordered():
    from emdr2_amd.model import kernels as K
    K.ORDERED.enabled = True
    yield K.ORDERED
    K.ORDERED.enabled = False
    K.ORDERED.release()
    K.GRAD_SINK = None
    K.DROPOUT.step = 0


def _build(guard):
    from emdr2_amd.model import kernels as K
    from emdr2_amd.model.transformer import Config, T5Model
    from emdr2_amd.training import FlatAdam
    torch.manual_seed(0)
    cfg = Config(num_layers=2, hidden_size=128, num_attention_heads=2, ffn_hidden_size=256, max_position_embeddings=128, init_method_std=0.05)
    m = T5Model(cfg, 512, checkpoint_activations=True).train()
    opt = K.GRAD_SINK = FlatAdam(m, lr=1e-3, bucket_bytes=1 << 20, skip_nonfinite=guard)
    K.DROPOUT.step = 0
    assert len(opt.buckets) > 1
    return m, opt


def _step(m, opt, batch, poison=None, nan_loss=False):
    """One training step on batch number `batch`; `poison` = (parameter name, element): one NaN into that gradient after finish()."""
    rng = np.random.default_rng(100 + batch)
    enc, dec = torch.from_numpy(rng.integers(5, 512, size=(8, 64))).cuda(), torch.from_numpy(rng.integers(5, 512, size=(8, 32))).cuda()
    opt.zero_grad()
    logits, _ = m(enc, dec)
    loss = logits.float().square().mean()
    (loss * NAN if nan_loss else loss).backward()
    opt.finish()
    if poison is not None:
        dict(m.named_parameters())[poison[0]].grad.view(-1)[poison[1]] = NAN
    return opt.step()


def _snap(opt):
    torch.cuda.synchronize()
    return [b[k].clone() for b in opt.buckets for k in ("master", "m", "v", "work")]


def _same(a, b):
    bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)
    return len(a) == len(b) and all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def _victim(m, opt):
    """After the first step: a large tensor that receives gradients and is not the first of the first bucket, so that the key must carry
    a bucket number or an offset."""
    named = [(n, p) for n, p in m.named_parameters() if opt.expected.get(p, 0) > 0 and p.numel() > 5000
             and (opt.slot[p][0]["idx"] > 0 or opt.slot[p][1] > 0)]
    name, p = named[len(named) // 2]
    return name, p.numel() - 3


def test_clean_steps_with_the_guard_equal_the_unguarded_optimizer(ordered):
    m, opt = _build(True)
    for batch in (1, 2, 3):
        _step(m, opt, batch)
        assert not bool(opt.last_step_skipped)
    on, launches_on = _snap(opt), opt.optimizer_launches
    rep = opt.guard_report()
    assert rep["skipped_total"] == 0 and rep["longest_run"] == 0 and rep["step"] is None
    assert opt.state_dict()["skipped_steps"] == 0
    m2, opt2 = _build(False)
    for batch in (1, 2, 3):
        _step(m2, opt2, batch)
    assert _same(on, _snap(opt2))
    assert launches_on == opt2.optimizer_launches + 1                    # the verdict: one launch per step
    assert "skipped_steps" not in opt2.state_dict()


def test_a_poisoned_step_changes_nothing_and_the_next_one_is_the_unguarded_twins(ordered):
    from emdr2_amd.model import kernels as K
    m, opt = _build(True)
    _step(m, opt, 1)
    victim = _victim(m, opt)
    after1 = _snap(opt)
    _step(m, opt, 2, poison=victim)
    assert bool(opt.last_step_skipped)
    assert _same(after1, _snap(opt))                                     # masters, both moments, working copies: what step 1 left
    assert opt.step_count == 2 and K.DROPOUT.step == 2                   # the counters moved all the same
    rep = opt.guard_report()
    assert rep == {"skipped_total": 1, "consecutive": 1, "longest_run": 1, "step": 2, "parameter": victim[0], "element": victim[1], "nan": 1,
                   "inf": 0}
    assert opt.guard_report()["step"] is None                            # cleared by the read above
    assert opt.state_dict()["skipped_steps"] == 1
    _step(m, opt, 3)
    assert not bool(opt.last_step_skipped)
    after3 = _snap(opt)
    assert opt.guard_report() == {"skipped_total": 1, "consecutive": 0, "longest_run": 1, "step": None, "parameter": None, "element": None,
                                  "nan": 0, "inf": 0}
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    # the twin never saw step 2: its counters are bumped by hand, as the skipped step bumped them
    m2, opt2 = _build(False)
    _step(m2, opt2, 1)
    opt2.step_count += 1
    K.DROPOUT.step = opt2.step_count
    _step(m2, opt2, 3)
    assert opt2.step_count == 3
    assert _same(after3, _snap(opt2))


def test_without_the_guard_the_same_poison_reaches_the_masters(ordered):
    m, opt = _build(False)
    _step(m, opt, 1)
    _step(m, opt, 2, poison=_victim(m, opt))
    torch.cuda.synchronize()
    assert not all(bool(torch.isfinite(b["master"]).all()) for b in opt.buckets)


def _rank(rank, world, port, out_dir):
    _init(rank, world, port, "gloo")
    from emdr2_amd.model import kernels as K
    m, opt = _build(True)
    _step(m, opt, 10 + rank)                                             # different data per rank
    after1 = _snap(opt)
    _step(m, opt, 20 + rank, nan_loss=rank == 1)                         # rank 1's backward alone produces NaN: the exchange carries it
    skipped = bool(opt.last_step_skipped)
    unchanged = _same(after1, _snap(opt))
    params2 = [p.detach().cpu().clone() for p in m.parameters()]
    rep = opt.guard_report()
    _step(m, opt, 30 + rank)
    applied = not bool(opt.last_step_skipped)
    torch.save({"skipped": skipped, "unchanged": unchanged, "applied": applied, "report": rep, "after_skip": params2,
                "after_next": [p.detach().cpu() for p in m.parameters()]}, os.path.join(out_dir, "r%d.pt" % rank))
    K.GRAD_SINK = None
    torch.distributed.destroy_process_group()


def test_two_ranks_skip_together_when_one_produced_the_nan(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "r%d.pt" % r), weights_only=False) for r in (0, 1))
    for r in (r0, r1):
        assert r["skipped"] and r["unchanged"] and r["applied"]
        assert r["report"]["skipped_total"] == 1 and r["report"]["step"] == 2 and r["report"]["nan"] > 0
    assert r0["report"] == r1["report"]                                  # the same verdict from the same exchanged bits: no collective
    assert len(r0["after_skip"]) == len(r1["after_skip"]) > 10
    for key in ("after_skip", "after_next"):
        for a, b in zip(r0[key], r1[key]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(bool(torch.isfinite(p).all()) for p in r0["after_next"])
    assert any(not torch.equal(a, b) for a, b in zip(r0["after_skip"], r0["after_next"]))      # the clean step did move them
