"""GPU: generation stamps in `--save-index-snapshot` through the task entry point, on the synthetic world of tests/test_task_gpu.py.  The
six-step run of tests/test_index_newest_wins_task_gpu.py (300 rows, both in-place writers, newest-wins) with the oldest-first refresher and
a snapshot, ended by --exit-interval: the sidecar is next to the checkpoint, a retriever started from it holds every row's own stamp -- so
its first oldest-first selection is the genuinely oldest rows, not the row range uniform stamps would give -- and the run resumes."""
import argparse
import os

import numpy as np
import pytest

from tests.test_index_newest_wins_task_gpu import LINE
from tests.test_index_oldest_cpu import oldest_rows_reference
from tests.test_task_gpu import _argv, _make_world

pytestmark = pytest.mark.gpu
M64 = 2 ** 64 - 1
STAMPED = ("--index-generations", "--index-refresh-in-place", "--index-writeback", "--index-newest-wins", "--index-refresh-oldest-first",
           "--save-index-snapshot")
# two epochs of six steps are scheduled; --exit-interval ends the first run after six and the resumed one after eight
PACE = ("--disable-retriever-dropout", "--index-reload-interval", "6", "--indexer-batch-size", "64", "--log-interval", "1", "--epochs", "2")


class _Arena(object):
    n_docs = 300


def _retriever(emb, ckpt, generations, capsys):
    from emdr2_amd.model.emdr2_model import PreComputedEvidenceDocsRetriever
    args = argparse.Namespace(topk_retrievals=4, hidden_size=128, allow_trivial_doc=True, embedding_path=emb, faiss_use_gpu=True,
                              save_index_snapshot=True, load=ckpt, index_generations=generations)
    capsys.readouterr()
    r = PreComputedEvidenceDocsRetriever(args, evidence_arena=_Arena())
    return r.mips_index, capsys.readouterr().out


def test_a_stamped_run_saves_its_stamps_and_a_resume_restores_them(tmp_path, capsys):
    from emdr2_amd import checkpointing
    from emdr2_amd.data.emdr2_index import digest_stamps
    from emdr2_amd.data.index_snapshot import StampFile, index_digest, read_snapshot_meta
    from emdr2_amd.tasks import run as task_run
    tmp = str(tmp_path)
    vocab, ev, emb = _make_world(tmp)
    ckpt = os.path.join(tmp, "ckpt")
    model, _ = task_run.main(_argv(tmp, vocab, ev, emb, extra=STAMPED + PACE + ("--exit-interval", "6")))
    out = capsys.readouterr().out
    assert "exiting the program at iteration 6" in out and checkpointing.read_tracker(ckpt)[0] == 6
    path = os.path.join(ckpt, "evidence_index.flat")
    assert sorted(n for n in os.listdir(ckpt) if n.startswith("evidence_index")) == [
        "evidence_index.flat", "evidence_index.flat.gen", "evidence_index.flat.meta"]
    meta = read_snapshot_meta(path)
    side = np.array(StampFile(path + ".gen").stamps)
    assert (meta["iteration"], meta["mode"], meta["n"]) == (6, "rolling", 300)
    assert (int(meta["stamps"]["digest_sum"], 16), int(meta["stamps"]["digest_xor"], 16)) == digest_stamps(side)
    print("stamps in the snapshot:", dict(zip(*[v.tolist() for v in np.unique(side, return_counts=True)])))
    assert np.unique(side).size > 1 and side.max() == 5 and side.min() >= 1                # both writers have written: the refresher's pass, the last write-back
    live = model.evidence_retriever.mips_index
    assert np.array_equal(live.shard.generation[:300].cpu().numpy().view(np.uint32), side)

    # a retriever built from the same arguments with load = <save>
    index, said = _retriever(emb, ckpt, True, capsys)
    assert "index snapshot %s loaded" % path in said and "generation stamps restored" in said and meta["stamps"]["digest_sum"] in said
    assert "stamped beyond" not in said                                                    # nothing is newer than the checkpoint's iteration 6
    assert index.stamps_restored and np.array_equal(index.shard.generation[:300].cpu().numpy().view(np.uint32), side)
    assert index_digest(index) == (int(meta["digest_sum"], 16), int(meta["digest_xor"], 16)) == index_digest(live)
    n, below = 200, 6                                                                      # the resumed refresher's first selection: G = 6
    rows, info = index.oldest_rows(n, below)
    want_rows, want_info = oldest_rows_reference(side, n, below)
    assert np.array_equal(rows.cpu().numpy(), want_rows) and [w & M64 for w in info.tolist()] == want_info
    assert set(want_rows.tolist()) != set(range(n))                                        # (what the uniform stamp of a snapshot without stamps selects)
    assert index.generation_stats(6) == live.generation_stats(6)

    # without --index-generations the snapshot loads and the sidecar is ignored
    plain, said = _retriever(emb, ckpt, False, capsys)
    assert "index snapshot %s loaded" % path in said and "stamps" not in said
    assert plain.shard.generation is None and not plain.stamps_restored and index_digest(plain) == index_digest(live)

    # resumed for two more steps with the same flags
    model2, _ = task_run.main(_argv(tmp, vocab, ev, emb, extra=STAMPED + PACE + ("--exit-interval", "8")))
    out2 = capsys.readouterr().out
    assert "index snapshot %s loaded" % path in out2 and "generation stamps restored" in out2
    assert "exiting the program at iteration 8" in out2 and checkpointing.read_tracker(ckpt)[0] == 8
    lines = [m.groups() for m in LINE.finditer(out2)]
    assert [int(l[0]) for l in lines] == [7, 8]                                            # `kept newer` is reported at both boundaries
    assert "stamped beyond" not in out2                                                    # from_future is 0 in its generation lines
    # the age line no longer under-reports: boundary 7 rewrites at most 64 refreshed + 16 written-back rows, so a row among the 81 oldest of
    # the snapshot is still there (a uniform stamp of 6 would have made every age at iteration 7 at most 1)
    assert 1 < 7 - int(np.sort(side)[80]) <= int(lines[0][5]) <= 7 - int(side.min())

    # the same resume without --index-generations (and so without the flags that need stamps): it loads the snapshot, whatever sidecar is there
    assert os.path.exists(path + ".gen")
    plain_flags = ("--index-refresh-in-place", "--index-writeback", "--save-index-snapshot")
    task_run.main(_argv(tmp, vocab, ev, emb, extra=plain_flags + PACE + ("--exit-interval", "10")))
    out3 = capsys.readouterr().out
    assert "index snapshot %s loaded" % path in out3 and "stamps restored" not in out3 and "index generations at" not in out3
    assert "exiting the program at iteration 10" in out3
