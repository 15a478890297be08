"""GPU: --index-generations / --index-newest-wins through the task entry point.  The synthetic-corpus run of tests/test_index_writeback_gpu.py
with both in-place writers, paced so that the rolling refresher's pass takes five steps (five batches of 64 rows, one per pump): rows that
the write-back stamped with the weights of step t - 1 are reached boundaries later by a pass whose snapshot is older.  With
--index-generations alone -- stamps kept, every writer overwrites: the semantics before there were stamps -- some row's stamp FALLS; with
--index-newest-wins no row's stamp ever does."""
import os
import re

import numpy as np
import pytest

from tests.test_task_gpu import _argv, _make_world

pytestmark = pytest.mark.gpu
LINE = re.compile(r"index generations at iteration (\d+): retrieved rows mean age ([0-9.]+) max (\d+) \((\d+) rows\) \| "
                  r"whole index mean age ([0-9.]+) max (\d+) \((\d+) rows\) \| kept newer (\d+)")


def _run(tmp, flag, monkeypatch, capsys):
    """-> (stamps [boundary, row] after every writer of each boundary, the parsed age lines, the output)"""
    from emdr2_amd import checkpointing
    from emdr2_amd.tasks import run as task_run
    from emdr2_amd.tasks.openqa.e2eqa import train_e2eqa
    os.makedirs(tmp)
    vocab, ev, emb = _make_world(tmp)
    argv = _argv(tmp, vocab, ev, emb, extra=("--index-refresh-in-place", "--index-writeback", "--disable-retriever-dropout", flag,
                                             "--index-reload-interval", "6", "--indexer-batch-size", "64", "--log-interval", "1",
                                             "--audit-index-interval", "1"))
    recorded = []
    inner = train_e2eqa.index_generation_line

    def spy(index, iteration, retrieved):
        recorded.append(index.shard.generation[:index.shard.n_rows].cpu().numpy().astype(np.int64))
        return inner(index, iteration, retrieved)
    monkeypatch.setattr(train_e2eqa, "index_generation_line", spy)
    model, results = task_run.main(argv)
    out = capsys.readouterr().out
    print("\n".join(l for l in out.splitlines() if l.startswith("index generations")))
    assert checkpointing.read_tracker(os.path.join(tmp, "ckpt"))[0] == 6 and results["validation"][1] == 8      # all six steps trained
    index = model.evidence_retriever.mips_index
    assert index.generations and index.shard.generation is not None
    lines = [tuple(float(v) if "." in v else int(v) for v in m.groups()) for m in LINE.finditer(out)]
    return np.stack(recorded), lines, out


def _check_lines(stamps, lines, out):
    assert [l[0] for l in lines] == [1, 2, 3, 4, 5, 6], out               # the age line, at every --log-interval boundary
    for (it, r_mean, r_max, r_count, w_mean, w_max, w_count, kept), after in zip(lines, stamps):
        assert r_count == 4 * 4 and w_count == 300
        assert 0 <= r_mean <= r_max <= it - 1                             # as the search found them, against the weights of the forward
        assert w_max == it - int(after.min()) and abs(w_mean - float((it - after).mean())) < 0.006
    assert out.count("sound, canonical") == 7 and "FAILED" not in out    # the audit: before the first step and at every boundary
    assert (stamps[-1] <= 5).all() and stamps[-1].max() == 5             # the last write-back stamped 6 - 1


def test_with_newest_wins_no_row_s_stamp_ever_falls(tmp_path, capsys, monkeypatch):
    stamps, lines, out = _run(str(tmp_path / "newest"), "--index-newest-wins", monkeypatch, capsys)
    _check_lines(stamps, lines, out)
    assert (np.diff(stamps, axis=0) >= 0).all()                           # monotone per row, boundary after boundary
    assert sum(l[7] for l in lines) > 0                                   # and the refresher did come round to newer rows: it left them alone


def test_without_it_the_refresher_makes_written_back_rows_older(tmp_path, capsys, monkeypatch):
    """the case the feature exists for, on the semantics before it: stamps are kept, every writer overwrites"""
    stamps, lines, out = _run(str(tmp_path / "plain"), "--index-generations", monkeypatch, capsys)
    _check_lines(stamps, lines, out)
    fell = np.nonzero((np.diff(stamps, axis=0) < 0).any(axis=0))[0]
    assert fell.size > 0
    assert sum(l[7] for l in lines) == 0                                  # nobody is ever left alone
