"""GPU: --skip-nonfinite-steps through the task entry point on the synthetic corpus of tests/test_task_gpu.py, with --index-writeback.  A
forward step whose loss is NaN at iteration 3 of 6 is skipped: the run finishes with finite parameters and an index without a
non-finite row, the log counts the skip in the reference's words, keeps it out of the averages and names the offender, and
--max-consecutive-skipped-steps ends the run at the log boundary.  And `index_writeback` itself on a 512 x 256 shard: a non-finite row is
not written, a skipped step writes none."""
import re

import numpy as np
import pytest
import torch

from tests.test_task_gpu import _argv, _make_world

pytestmark = pytest.mark.gpu
FLAGS = ("--skip-nonfinite-steps", "--index-writeback", "--index-refresh-in-place", "--disable-retriever-dropout", "--log-interval", "2")


def _run(tmp, monkeypatch, extra=()):
    """The task with a forward step that multiplies the loss (and the losses it reports) by NaN in the third training step."""
    from emdr2_amd.tasks import run as task_run
    from emdr2_amd.tasks.openqa.e2eqa import run as e2eqa_run
    from emdr2_amd.tasks.openqa.e2eqa import train_e2eqa
    calls = []

    def forward_step(batch, model, eos_id):
        loss, stats = train_e2eqa._cross_entropy_forward_step(batch, model, eos_id)
        calls.append(1)
        if len(calls) == 3:
            nan = float("nan")
            return loss * nan, {k: v * nan for k, v in stats.items()}
        return loss, stats

    def train(*a, **kw):
        return train_e2eqa.train(*a, forward_step=forward_step, **kw)
    monkeypatch.setattr(e2eqa_run, "train", train)
    vocab, ev, emb = _make_world(tmp, n_valid=4)                         # 24 questions / batch 4: six steps
    return task_run.main(_argv(tmp, vocab, ev, emb, extra=FLAGS + tuple(extra)))


def test_a_nan_step_is_skipped_counted_named_and_kept_out_of_the_index(tmp_path, monkeypatch, capsys):
    from emdr2_amd.model import kernels as K
    try:
        model, _ = _run(str(tmp_path), monkeypatch)
    finally:
        K.GRAD_SINK = None
    out = capsys.readouterr().out
    lines = {int(m.group(1)): m.group(0) for m in re.finditer(r" iteration +(\d+)/ +\d+ \|.*", out)}
    assert sorted(lines) == [2, 4, 6], out[-3000:]
    assert "number of skipped iterations:   1 | number of nan iterations:   1 |" in lines[4]
    for it in (2, 6):
        assert "number of skipped iterations:   0 | number of nan iterations:   0 |" in lines[it]
    for it in (2, 4, 6):                                                 # the skipped step's NaN losses stay out of the interval's averages
        for key in ("lm_loss", "retriever_loss"):
            value = float(re.search(r" %s: (\S+) \|" % key, lines[it]).group(1))
            assert np.isfinite(value), lines[it]
    offender = re.findall(r"skipped step at iteration (\d+): first non-finite gradient element: (\S+)\[(\d+)\] \| NaN elements: (\d+) \| Inf elements: (\d+)", out)
    assert len(offender) == 1 and offender[0][0] == "3" and int(offender[0][3]) > 0, out[-3000:]
    assert offender[0][1] in dict(model.named_parameters())
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert model.evidence_retriever.mips_index.audit()["nonfinite_rows"] == 0


def test_max_consecutive_skipped_steps_ends_the_run_at_the_log_boundary(tmp_path, monkeypatch, capsys):
    from emdr2_amd.model import kernels as K
    try:
        with pytest.raises(RuntimeError, match=r"--max-consecutive-skipped-steps 1\), seen at iteration 4"):
            _run(str(tmp_path), monkeypatch, extra=("--max-consecutive-skipped-steps", "1"))
    finally:
        K.GRAD_SINK = None
    out = capsys.readouterr().out
    assert "skipped step at iteration 3" in out and " iteration        6/" not in out


class _Stub(object):
    """What index_writeback asks of a model: the retriever with its index, the hidden size, the step's (rows, embeddings)."""

    def __init__(self, index, hidden, kept):
        self.hidden_size, self.kept = hidden, kept
        self.evidence_retriever = type("R", (), {"mips_index": index, "process_group": None, "_world": staticmethod(lambda: (0, 1))})()

    def take_writeback(self):
        return self.kept


def test_index_writeback_leaves_out_non_finite_rows_and_skipped_steps():
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex
    from emdr2_amd.tasks.openqa.e2eqa.train_e2eqa import index_writeback
    n, d = 512, 256
    rng = np.random.default_rng(0)
    m = rng.standard_normal((n, d)).astype(np.float16)
    index = DistributedBruteForceIndex(d, None, use_gpu=True)
    index.add_arrays(np.arange(1, n + 1, dtype=np.int32), m)
    stored = lambda: index.shard.rows(np.arange(n)).cpu().numpy().view(np.uint16)
    assert np.array_equal(stored(), m.view(np.uint16))
    rows = torch.tensor([3, 500, 77, 129, 7, 300, 41, 0], dtype=torch.int64, device="cuda")
    new = rng.standard_normal((8, d)).astype(np.float16)
    new[2, 100] = np.nan                                                 # row 77 of the index would receive it
    new[5, 0] = np.inf                                                   # ... and row 300 this
    emb = torch.from_numpy(new).cuda()
    true, false = torch.tensor(True, device="cuda"), torch.tensor(False, device="cuda")
    index_writeback(_Stub(index, d, (rows, emb)), 2, 4, skipped=true)    # a skipped step: none is written
    assert np.array_equal(stored(), m.view(np.uint16))
    index_writeback(_Stub(index, d, (rows, emb)), 2, 4, skipped=false)
    want = m.copy()
    for i, r in enumerate(rows.tolist()):
        if i not in (2, 5):
            want[r] = new[i]
    assert np.array_equal(stored(), want.view(np.uint16))                # rows 77 and 300 keep their bits, the six others are written
    assert index.audit()["nonfinite_rows"] == 0
    index_writeback(_Stub(index, d, (rows, emb)), 2, 4)                  # without the flag the writer is what it was: the list as it stands
    got = stored().view(np.float16)
    assert np.isnan(got[77, 100]) and np.isinf(got[300, 0])
