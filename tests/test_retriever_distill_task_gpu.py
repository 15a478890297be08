"""GPU: `--retriever-distill-attention` (and `--attention-mass-value-norms`) through the task entry point, on the synthetic world of
tests/test_task_gpu.py: the run says which retriever loss is in force, its --log-interval line carries a non-zero `retriever_loss`, with
`--reader-attention-mass` the read fields appear beside it, and a run without the new flags prints none of this."""
import contextlib
import io
import os
import re

import pytest

from tests.test_task_gpu import _argv, _make_world

pytestmark = pytest.mark.gpu
RUNS = {"plain": (),
        "distill": ("--retriever-distill-attention",),
        "all": ("--retriever-distill-attention", "--attention-mass-value-norms", "--reader-attention-mass", "--retrieval-answer-hits",
                "--report-topk-accuracies", "1", "4")}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from emdr2_amd.model import kernels as K
    from emdr2_amd.tasks import run as task_run
    base = str(tmp_path_factory.mktemp("retriever_distill"))
    # the task entry point configures the process for training (sticky packed capacities, the dropout seed and step, the gradient sink);
    # the modules that run after this one get back what they would have found without it
    packing = (K.PACKING.sticky, K.PACKING.enabled, dict(K.PACKING.capacity))
    dropout = (K.DROPOUT.base_seed, K.DROPOUT.step)
    res = {}
    try:
        for name, flags in RUNS.items():
            tmp = os.path.join(base, name)
            os.makedirs(tmp)
            vocab, ev, emb = _make_world(tmp, n_train=8)                 # two training steps of four questions: one --log-interval line
            out = io.StringIO()
            with contextlib.redirect_stdout(out):
                model, results = task_run.main(_argv(tmp, vocab, ev, emb, extra=flags))
            res[name] = dict(out=out.getvalue(), results=results, armed=K.ATTN_MASS.ids_k is not None,
                             switches=(model.retriever_distill_attention, model.attention_mass_value_norms, model.reader_attention_mass))
            del model
    finally:
        K.PACKING.sticky, K.PACKING.enabled, K.PACKING.capacity = packing
        K.DROPOUT.base_seed, K.DROPOUT.step = dropout
        K.GRAD_SINK = None
        K.WEIGHTS.invalidate()
        K.ATTN_MASS.disarm()
    return res


def _log_lines(out):
    return [l for l in out.splitlines() if "lm_loss" in l and "iteration" in l]


def _retriever_loss(line):
    return float(re.search(r" retriever_loss: ([0-9.E+-]+) \|", line).group(1))


@pytest.mark.parametrize("name", ["distill", "all"])
def test_flagged_run_says_its_loss_and_logs_a_non_zero_retriever_loss(runs, name):
    r = runs[name]
    assert r["switches"] == (True, name == "all", name == "all")
    said = [l for l in r["out"].splitlines() if l.startswith("retriever loss:")]
    assert len(said) == 1 and "--retriever-distill-attention" in said[0] and ("value-norm weighted" in said[0]) == (name == "all")
    lines = _log_lines(r["out"])
    assert lines
    for line in lines:
        v = _retriever_loss(line)
        assert v > 0.0 and v == v                                           # KL(read || prior) of a fresh model: positive, not NaN
    assert not r["armed"]
    assert r["results"]["validation"][1] == 8                              # the evaluation ran


def test_with_reader_attention_mass_the_read_fields_appear(runs):
    for line in _log_lines(runs["all"]["out"]):
        assert " read entropy: " in line and " read-prior agree: " in line and " read mass: " in line and " read top1 hit: " in line
    assert "Read Top-1 Hit" in runs["all"]["out"]
    for line in _log_lines(runs["distill"]["out"]):                        # the meter stays tied to --reader-attention-mass
        assert "read entropy" not in line
    assert "Read Top-1 Hit" not in runs["distill"]["out"]


def test_a_run_without_the_new_flags_prints_what_it_printed(runs):
    r = runs["plain"]
    assert r["switches"] == (False, False, False)
    assert "retriever loss:" not in r["out"] and "read entropy" not in r["out"] and "Read Top-1 Hit" not in r["out"]
    lines = _log_lines(r["out"])
    assert lines and all(" lm_loss: " in l and " retriever_loss: " in l and "read" not in l for l in lines), lines
