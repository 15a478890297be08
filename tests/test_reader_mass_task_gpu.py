"""GPU: `--reader-attention-mass` with `--retrieval-answer-hits` through the task entry point, on the synthetic world of
tests/test_task_gpu.py: the training log line gains `read entropy`, `read-prior agree`, `read mass` and `read top1 hit`, the evaluation
gains `Read Top-1 Hit` beside `Answer Hits@k`."""
import contextlib
import io
import math
import os
import re

import pytest

from tests.test_task_gpu import _argv, _make_world

pytestmark = pytest.mark.gpu
FLAGS = ("--reader-attention-mass", "--retrieval-answer-hits", "--report-topk-accuracies", "1", "4")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from emdr2_amd.model import kernels as K
    from emdr2_amd.tasks import run as task_run
    tmp = os.path.join(str(tmp_path_factory.mktemp("reader_mass")), "flagged")
    os.makedirs(tmp)
    # the task entry point configures the process for training (sticky packed capacities, the dropout seed and step, the gradient sink);
    # the modules that run after this one get back what they would have found without it
    packing = (K.PACKING.sticky, K.PACKING.enabled, dict(K.PACKING.capacity))
    dropout = (K.DROPOUT.base_seed, K.DROPOUT.step)
    try:
        vocab, ev, emb = _make_world(tmp, n_train=8)                     # two training steps of four questions: one --log-interval line
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            model, results = task_run.main(_argv(tmp, vocab, ev, emb, extra=FLAGS))
        armed = K.ATTN_MASS.ids_k is not None
        del model
    finally:
        K.PACKING.sticky, K.PACKING.enabled, K.PACKING.capacity = packing
        K.DROPOUT.base_seed, K.DROPOUT.step = dropout
        K.GRAD_SINK = None
        K.WEIGHTS.invalidate()
        K.ATTN_MASS.disarm()
    return dict(results=results, out=out.getvalue(), armed=armed)


def test_training_log_line_carries_the_four_items(run):
    lines = [l for l in run["out"].splitlines() if "read entropy" in l]
    assert lines and all("lm_loss" in l and "hit mass: " in l for l in lines)                  # part of the --log-interval line
    for line in lines:
        ent = float(re.search(r" read entropy: ([0-9.]+) \|", line).group(1))
        agree, total = (int(v) for v in re.search(r" read-prior agree: (\d+)/(\d+) \|", line).groups())
        mass = float(re.search(r" read mass: ([0-9.]+) \|", line).group(1))
        top1, total2 = (int(v) for v in re.search(r" read top1 hit: (\d+)/(\d+) \|", line).groups())
        assert total == total2 == 8                                                             # two steps of four questions per line
        assert 0 <= agree <= total and 0 <= top1 <= total
        assert 0.0 <= mass <= 1.0 and 0.0 <= ent <= math.log(4) + 1e-4                          # a distribution over K = 4 slots
    assert not run["armed"]                                                                     # nothing leaves the collector armed


def test_evaluation_prints_read_top1_hit(run):
    stats, total = run["results"]["validation"]
    assert set(stats) == {"Exact Match Score", "Answer Hits@1", "Answer Hits@4", "Read Top-1 Hit"}
    n = stats["Read Top-1 Hit"]
    assert total == 8 and int(n) == n and 0 <= n <= stats["Answer Hits@4"]                      # the most-read slot holds an answer: some slot does
    assert "|Read Top-1 Hit = %.2f" % (n * 100 / total) in run["out"]
