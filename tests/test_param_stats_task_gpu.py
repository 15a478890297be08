"""GPU: --log-param-stats-interval / --param-stats-file in the task.  The synthetic world of tests/test_task_gpu.py through tasks.run for
two iterations: the summary line and the group lines in the log, two JSON lines whose parameters are exactly the model's; without the flag,
none of the lines."""
import json
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture()
def sink():
    from emdr2_amd.model import kernels as K
    yield K
    K.GRAD_SINK = None
    K.DROPOUT.step = 0


def test_task_logs_the_summary_the_groups_and_one_json_line_per_call(tmp_path, capsys, sink):
    from emdr2_amd.tasks import run as task_run
    from tests.test_task_gpu import _argv, _make_world
    tmp = str(tmp_path)
    vocab, ev, emb = _make_world(tmp, n_train=8, n_valid=4)              # 8 questions / batch 4: two steps
    path = os.path.join(tmp, "param_stats.jsonl")
    model, _ = task_run.main(_argv(tmp, vocab, ev, emb, extra=("--log-param-stats-interval", "1", "--param-stats-file", path)))
    out = capsys.readouterr().out
    heads = re.findall(r"^ param stats at iteration (\d+) \(step (\d+), gradients current\): grad norm: (\S+) \| params norm: (\S+) \| "
                       r"num zeros: (\d+) \| non-finite: 0 \| clip factor: (\S+) \| largest lr\*\|d\|/\|w\|: (.+?) \| "
                       r"largest share of grad norm\^2: (.+)$", out, flags=re.M)
    assert [(int(h[0]), int(h[1])) for h in heads] == [(1, 1), (2, 2)], out[-3000:]
    names = [n for n, _ in model.named_parameters()]
    for h in heads:
        assert float(h[2]) > 0.0 and float(h[3]) > 0.0 and 0.0 < float(h[5]) <= 1.0
        assert len(h[7].split(", ")) == 5 and all(x.split(" ")[0] in names for x in h[7].split(", "))
    for h in heads:                                                      # (the first update of a warm-up may run at lr 0: its ratios are zeros)
        assert len(h[6].split(", ")) == 5 and all(x.split(" ")[0] in names for x in h[6].split(", "))
    groups = re.findall(r"^ param stats group (\S+): (\d+) tensors, (\d+) elements \| grad norm: \S+ \| params norm: \S+ \| direction rms: \S+ \| "
                        r"max abs grad: \S+ \| num zeros: \d+ \| non-finite: 0$", out, flags=re.M)
    assert len(groups) % 2 == 0 and groups[:len(groups) // 2] == groups[len(groups) // 2:]              # the same groups at both iterations
    groups = groups[:len(groups) // 2]
    assert sum(int(g[2]) for g in groups) == sum(p.numel() for p in model.parameters()) and sum(int(g[1]) for g in groups) == len(names)
    assert any(re.search(r"layers\.1$", g[0]) for g in groups) and len(set(g[0] for g in groups)) == len(groups)
    assert " iteration        2/" in out and "lm_loss" in out            # it trained on
    with open(path) as f:
        lines = [json.loads(x) for x in f]
    assert [x["iteration"] for x in lines] == [1, 2] and [x["step"] for x in lines] == [1, 2]
    for x, h in zip(lines, heads):
        assert sorted(x["params"]) == sorted(names) and x["grads_current"] is True and "lr" in x and x["lr_note"]
        assert all(r["n"] == p.numel() for r, p in ((x["params"][n], p) for n, p in model.named_parameters()))
        total = sum(r["grad_sq"] for r in x["params"].values())
        assert "%.6E" % total ** 0.5 == h[2]                             # the line's norm is the file's records
        assert any(r["active"] for r in x["params"].values())


def test_task_without_the_flag_prints_none_of_it(tmp_path, capsys, sink):
    from emdr2_amd.tasks import run as task_run
    from tests.test_task_gpu import _argv, _make_world
    tmp = str(tmp_path)
    vocab, ev, emb = _make_world(tmp, n_train=8, n_valid=4)
    task_run.main(_argv(tmp, vocab, ev, emb))
    out = capsys.readouterr().out
    assert " iteration        2/" in out and "param stats" not in out
    assert not any(name.endswith(".jsonl") for name in os.listdir(tmp))
    from emdr2_amd.model import kernels as K
    assert not hasattr(K.GRAD_SINK, "_pstats")                           # no buffer either
