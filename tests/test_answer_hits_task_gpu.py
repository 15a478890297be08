"""GPU: `--retrieval-answer-hits` through the task entry point, on the synthetic world of tests/test_task_gpu.py: the training log gains
`answer hits@k`, the evaluation gains `Answer Hits@k`, both agree with the host string matcher run on the evidence TEXT of the passages
the model retrieved -- and without the flag nothing of it appears and the evaluation is unchanged."""
import contextlib
import io
import os

import pytest

from tests.test_task_gpu import _argv, _make_world

pytestmark = pytest.mark.gpu
FLAGS = ("--retrieval-answer-hits", "--report-topk-accuracies", "1", "2", "4")


def _run(tmp, extra):
    from emdr2_amd.tasks import run as task_run
    os.makedirs(tmp)
    vocab, ev, emb = _make_world(tmp, n_train=8)                         # (seeded: the same world in either directory; two training steps)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        model, results = task_run.main(_argv(tmp, vocab, ev, emb, extra=extra))
    return model, results, out.getvalue(), ev


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from emdr2_amd.global_vars import get_args, get_tokenizer
    from emdr2_amd.tasks.openqa.e2eqa.answer_hits import answer_hit_table
    from emdr2_amd.tasks.openqa.e2eqa.train_data_utils import OpenQADataset
    from emdr2_amd.tasks.openqa.e2eqa.train_e2eqa import build_data_loader
    from emdr2_amd.model import kernels as K
    root = str(tmp_path_factory.mktemp("answer_hits"))
    tmp = os.path.join(root, "flagged")
    # the task entry point configures the process for training (sticky packed capacities, the dropout seed and step, the gradient sink);
    # the modules that run after this one get back what they would have found without it
    packing = (K.PACKING.sticky, K.PACKING.enabled, dict(K.PACKING.capacity))
    dropout = (K.DROPOUT.base_seed, K.DROPOUT.step)
    try:
        model, results, out, ev = _run(tmp, FLAGS)
        args = get_args()
        ds = OpenQADataset("OPENQA_DATASET", "valid", [os.path.join(tmp, "valid.tsv")], get_tokenizer(), args.seq_length_ret,
                           args.decoder_seq_length, seed=args.seed)
        table = answer_hit_table(model, build_data_loader(ds, args.eval_batch_size, num_workers=0, drop_last=False, shuffle=False))
        del model
        _, plain_results, plain_out, _ = _run(os.path.join(root, "plain"), ())
    finally:
        K.PACKING.sticky, K.PACKING.enabled, K.PACKING.capacity = packing
        K.DROPOUT.base_seed, K.DROPOUT.step = dropout
        K.GRAD_SINK = None
        K.WEIGHTS.invalidate()
    return dict(results=results, out=out, ev=ev, table=table, plain_results=plain_results, plain_out=plain_out)


def test_training_log_and_evaluation_report_answer_hits(runs):
    lines = [l for l in runs["out"].splitlines() if "answer hits@" in l]
    assert lines and all("lm_loss" in l and "hit mass: " in l for l in lines)                 # part of the --log-interval line
    for k in (1, 2, 4):
        assert all(" answer hits@%d: " % k in l for l in lines)
    assert " answer hits@4: " in lines[0] and "/8 |" in lines[0]                               # two steps of four questions per line
    stats, total = runs["results"]["validation"]
    counts = [stats["Answer Hits@%d" % k] for k in (1, 2, 4)]
    assert total == 8 and all(int(c) == c for c in counts) and 0 <= counts[0] <= counts[1] <= counts[2] <= total
    assert "|Answer Hits@4 = %.2f" % (counts[2] * 100 / total) in runs["out"]                   # metrics_func prints every stat


def test_hits_equal_the_host_string_matcher_on_the_text_of_the_retrieved_passages(runs):
    from emdr2_amd.tasks.openqa.dense_retriever.evaluation.evaluate import read_evidence_text
    from emdr2_amd.tasks.openqa.dense_retriever.evaluation.qa_validation import has_answer
    docs, table = read_evidence_text(runs["ev"]), runs["table"]
    assert len(table) == 8 and len({r["uid"] for r in table}) == 8 and all(len(r["kept_ids"]) == 4 for r in table)
    pairs = [(r["hit_pos"][j] >= 0, has_answer(r["answers"], docs[d][0])) for r in table for j, d in enumerate(r["kept_ids"])]
    assert any(h for _, h in pairs) and not all(h for _, h in pairs)                           # this world yields hits and misses
    assert all(mine == theirs for mine, theirs in pairs)
    for r in table:
        first = next((j for j, p in enumerate(r["hit_pos"]) if p >= 0), 4)
        assert r["best_slot"] == first
    stats, _ = runs["results"]["validation"]
    for k in (1, 2, 4):                                                                        # the reported counts are the table's prefix sums
        assert stats["Answer Hits@%d" % k] == sum(1 for r in table if r["best_slot"] < k)


def test_without_the_flag_nothing_is_reported_and_the_evaluation_is_the_same(runs):
    assert "answer hits@" not in runs["plain_out"] and "Answer Hits@" not in runs["plain_out"] and "hit mass" not in runs["plain_out"]
    stats, total = runs["plain_results"]["validation"]
    assert set(stats) == {"Exact Match Score"}
    flagged, flagged_total = runs["results"]["validation"]
    assert total == flagged_total == 8 and stats["Exact Match Score"] == flagged["Exact Match Score"]
    assert set(flagged) == {"Exact Match Score", "Answer Hits@1", "Answer Hits@2", "Answer Hits@4"}
