"""GPU: --deterministic-gradients through the model (kernels.ORDERED; include/emdr2_ops.h, "Ordered sums").  With the switch on, the same
training step from the same parameters and batch gives every gradient tensor bit for bit, undivided and in question groups; optimizer steps
repeat bit for bit; against the switch off the losses are bit-equal and the gradients agree to the 1e-6 relative norm that
tests/test_config2_gpu.py allows two runs of the atomic path; and two runs of the task entry point write byte-identical checkpoints.

The model is the small EMDR2 model of tests/test_microbatch_gpu.py (2 layers, hidden 128, two heads of 64 channels, dropout 0.1, packed
layout) with 16 questions x 8 passages x 128 tokens: the reader encoder sees more than 8,192 token rows, so its weight-gradient GEMMs split
their reduction (kernels.weight_grad_tn: tokens // 4096 slices)."""
import os

import pytest
import torch

from tests.test_microbatch_gpu import _case, _clear, _fb, _grads
from tests.test_task_gpu import _argv, _make_world

pytestmark = pytest.mark.gpu
SHAPE = dict(p=0.1, B=16, Kk=8, S=128)


@pytest.fixture()
def ordered():
    from emdr2_amd.model import kernels as K
    assert K.PACKING.enabled
    K.ORDERED.enabled, K.ORDERED.calls, K.ORDERED.max_split = True, 0, 0
    yield K.ORDERED
    K.ORDERED.enabled = False
    K.ORDERED.release()
    K.GRAD_SINK = None


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


@pytest.mark.parametrize("micro", (1, 2))
def test_three_backward_passes_give_every_gradient_bit_for_bit(ordered, micro):
    m, _, bt = _case(**SHAPE)
    runs = []
    for _ in range(3):
        _clear(m)
        loss, _stats = _fb(m, bt, micro)
        runs.append((loss.detach().clone(), _grads(m)))
    assert ordered.calls > 0
    if micro == 1:
        assert ordered.max_split > 1, ordered.max_split                # the reader encoder's rows: the split is really taken
    assert len(runs[0][1]) > 100
    for loss, g in runs[1:]:
        assert _same_bits(loss, runs[0][0])
        assert set(g) == set(runs[0][1])
        differ = [k for k in g if not _same_bits(g[k], runs[0][1][k])]
        assert not differ, differ


def test_switch_off_gives_the_same_losses_and_gradients_to_the_atomic_paths_own_noise(ordered):
    m, _, bt = _case(**SHAPE)
    loss_on, _ = _fb(m, bt, 1)
    g_on = _grads(m)
    calls = ordered.calls
    ordered.enabled = False
    _clear(m)
    loss_off, _ = _fb(m, bt, 1)
    g_off = _grads(m)
    assert ordered.calls == calls                                        # off: no ordered launch, no workspace request
    assert _same_bits(loss_on.detach(), loss_off.detach())
    assert set(g_on) == set(g_off)
    num = sum(float((g_on[k] - g_off[k]).double().pow(2).sum()) for k in g_on) ** 0.5
    den = sum(float(g_off[k].double().pow(2).sum()) for k in g_on) ** 0.5
    print("ordered against atomic: relative gradient norm %.3e" % (num / den))
    assert num / den < 1e-6, num / den


def test_three_optimizer_steps_repeat_bit_for_bit(ordered):
    from emdr2_amd.model import kernels as K
    from emdr2_amd.training import FlatAdam
    finals, state = [], None
    for _ in range(2):
        m, _, bt = _case(**SHAPE)
        if state is None:
            state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        else:
            m.load_state_dict(state)
        opt = K.GRAD_SINK = FlatAdam(m, lr=1e-3, weight_decay=0.1, clip_grad=1.0, bucket_bytes=1 << 20)
        for step in range(3):
            K.DROPOUT.step = step
            opt.zero_grad()
            _fb(m, bt, 1)
            opt.finish()
            opt.step()
        torch.cuda.synchronize()
        finals.append(([b["master"].clone() for b in opt.buckets], [b["grad"].clone() for b in opt.buckets]))
        K.GRAD_SINK = None
        K.DROPOUT.step = 0
    for a, b in zip(finals[0][0] + finals[0][1], finals[1][0] + finals[1][1]):
        assert _same_bits(a, b)
    assert any(float(g.abs().max()) > 0 for g in finals[0][1])


def _tensors(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict):
            for item in _tensors(v, prefix + k + "/"):
                yield item
        elif torch.is_tensor(v):
            yield prefix + k, v


def test_two_runs_of_the_task_write_byte_identical_checkpoints(tmp_path):
    from emdr2_amd import checkpointing
    from emdr2_amd.model import kernels as K
    from emdr2_amd.tasks import run as task_run
    saved = []
    try:
        for name in ("a", "b"):
            tmp = str(tmp_path / name)
            os.makedirs(tmp)
            vocab, ev, emb = _make_world(tmp, n_train=12, n_valid=4)
            # a run is a process: its dropout sites are numbered from 0 and its first step draws the masks of optimizer step 0 (the
            # optimizer moves DROPOUT.step only when it steps or loads a state, so the second run would start from the first run's count)
            K.DROPOUT._sites, K.DROPOUT.step = 0, 0
            argv = [a for a in _argv(tmp, vocab, ev, emb, extra=["--deterministic-gradients"]) if a != "--async-indexer"]   # no side-stream indexer
            task_run.main(argv)
            assert K.ORDERED.enabled and K.ORDERED.calls > 0
            it, _ = checkpointing.read_tracker(os.path.join(tmp, "ckpt"))
            assert it == 3                                               # 12 questions / batch 4, one epoch
            state = torch.load(checkpointing.get_checkpoint_name(os.path.join(tmp, "ckpt"), it), map_location="cpu", weights_only=False)
            saved.append(dict(_tensors(state["model"])))
    finally:
        K.ORDERED.enabled = False
        K.ORDERED.release()
    assert len(saved[0]) > 100 and set(saved[0]) == set(saved[1])
    differ = [k for k in saved[0] if not _same_bits(saved[0][k], saved[1][k])]
    assert not differ, differ
