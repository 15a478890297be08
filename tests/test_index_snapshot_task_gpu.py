"""GPU: `--save-index-snapshot` through the task entry point on the synthetic world of tests/test_task_gpu.py -- the index the side-stream
refresher committed last is on disk next to the checkpoint, and a resumed run starts from it instead of from the original pickle."""
import os

import numpy as np
import pytest
import torch

from tests.test_task_gpu import _argv, _make_world

pytestmark = pytest.mark.gpu


def _pair(meta):
    return int(meta["digest_sum"], 16), int(meta["digest_xor"], 16)


def _pickle_digest(emb):
    from emdr2_amd.data.emdr2_index import OpenRetreivalDataStore, digest_rows
    ids, rows = OpenRetreivalDataStore(emb, load_from_path=True, rank=0).to_arrays()
    return digest_rows(rows)


def _queries():
    return torch.from_numpy(np.random.default_rng(7).standard_normal((9, 128)).astype(np.float16)).cuda()


def _search(model):
    dist, idx = model.evidence_retriever.mips_index.search_mips_index(_queries(), 4, reconstruct=False)
    return dist.view(torch.int16).cpu(), idx.cpu()


def test_snapshot_is_written_at_the_last_update_and_a_resumed_run_searches_it(tmp_path, capsys):
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
    from emdr2_amd.data.index_snapshot import index_digest, read_snapshot_meta
    from emdr2_amd.tasks import run as task_run
    tmp = str(tmp_path)
    vocab, ev, emb = _make_world(tmp)
    model, results = task_run.main(_argv(tmp, vocab, ev, emb, extra=["--save-index-snapshot"]))
    out = capsys.readouterr().out
    assert "MIPS Index Updated at iteration 6" in out
    path = os.path.join(tmp, "ckpt", "evidence_index.flat")
    meta = read_snapshot_meta(path)
    assert (meta["iteration"], meta["mode"], meta["n"], meta["dim"], meta["world"]) == (6, "swap", 300, 128, 1) and meta["refreshes"] >= 1
    flat = FlatEmbeddingFile(path)
    live = index_digest(model.evidence_retriever.mips_index)
    assert flat.digest() == _pair(meta) == live
    assert live != _pickle_digest(emb)                                    # the refresher's rows, not the initial embeddings
    assert np.array_equal(flat.ids, np.arange(1, 301))
    assert sorted(n for n in os.listdir(os.path.join(tmp, "ckpt")) if n.startswith("evidence_index")) == ["evidence_index.flat", "evidence_index.flat.meta"]
    first = _search(model)
    # resume: iteration 6, nothing left to train; the index comes from the snapshot
    model2, results2 = task_run.main(_argv(tmp, vocab, ev, emb, extra=["--save-index-snapshot"]))
    out2 = capsys.readouterr().out
    assert "index snapshot %s loaded" % path in out2
    assert index_digest(model2.evidence_retriever.mips_index) == _pair(meta)
    second = _search(model2)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    s1, t1 = results["validation"]
    s2, t2 = results2["validation"]
    assert t1 == t2 == 8 and set(s1) == set(s2)
    for k in s1:                                                         # the comparison tests/test_task_gpu.py says it cannot make
        assert float(s1[k]) == float(s2[k]), k
    assert read_snapshot_meta(path) == meta                               # the resumed run, with nothing to train, left the snapshot alone


def test_a_snapshot_newer_than_the_checkpoint_or_without_meta_is_not_used(tmp_path, capsys):
    """The fall-backs of the start-up, on a retriever alone: an incomplete snapshot, one newer than the tracker's iteration, one of another
    size -- each time `--embedding-path` is loaded as without the flag, and one log line says why."""
    import argparse
    from emdr2_amd import checkpointing
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex, digest_rows
    from emdr2_amd.data.index_snapshot import index_digest, meta_path
    from emdr2_amd.model.emdr2_model import PreComputedEvidenceDocsRetriever
    tmp = str(tmp_path)
    vocab, ev, emb = _make_world(tmp, n_docs=40)
    ckpt = os.path.join(tmp, "ckpt")
    os.makedirs(ckpt)
    with open(checkpointing.get_checkpoint_tracker_filename(ckpt), "w") as fh:
        fh.write("4")
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((40, 128)).astype(np.float16)
    index = DistributedBruteForceIndex(128, None, use_gpu=True)
    index.add_arrays(np.arange(1, 41, dtype=np.int32), rows)
    path = os.path.join(ckpt, "evidence_index.flat")

    class _Arena(object):
        n_docs = 40
    args = argparse.Namespace(topk_retrievals=4, hidden_size=128, allow_trivial_doc=True, embedding_path=emb, faiss_use_gpu=True,
                              save_index_snapshot=True, load=ckpt)

    def start():
        r = PreComputedEvidenceDocsRetriever(args, evidence_arena=_Arena())
        return index_digest(r.mips_index), capsys.readouterr().out

    index.save_flat_file(path, {"iteration": 4, "refreshes": 2, "mode": "swap"})
    got, out = start()
    assert got == digest_rows(rows) and "loaded" in out
    index.save_flat_file(path, {"iteration": 6, "refreshes": 3, "mode": "swap"})
    got, out = start()
    assert got == _pickle_digest(emb) and "not used" in out and "iteration 6" in out and out.count("\n") == 1
    index.save_flat_file(path, {"iteration": 2, "refreshes": 1, "mode": "swap"})
    os.remove(meta_path(path))
    got, out = start()
    assert got == _pickle_digest(emb) and "incomplete" in out
    index.add_arrays(np.arange(1, 31, dtype=np.int32), rows[:30])
    index.save_flat_file(path, {"iteration": 2, "refreshes": 1, "mode": "swap"})
    got, out = start()
    assert got == _pickle_digest(emb) and "not used" in out
    args.save_index_snapshot = False                                      # a valid snapshot, no flag: as today, silently
    index.add_arrays(np.arange(1, 41, dtype=np.int32), rows)
    index.save_flat_file(path, {"iteration": 4, "refreshes": 2, "mode": "swap"})
    got, out = start()
    assert got == _pickle_digest(emb) and out == ""


def test_without_the_flag_nothing_is_written_and_a_resume_loads_the_pickle(tmp_path, capsys):
    from emdr2_amd.data.index_snapshot import index_digest
    from emdr2_amd.tasks import run as task_run
    tmp = str(tmp_path)
    vocab, ev, emb = _make_world(tmp)
    model, _ = task_run.main(_argv(tmp, vocab, ev, emb))
    assert not [n for n in os.listdir(os.path.join(tmp, "ckpt")) if n.startswith("evidence_index")]
    assert index_digest(model.evidence_retriever.mips_index) != _pickle_digest(emb)
    model2, _ = task_run.main(_argv(tmp, vocab, ev, emb))
    out = capsys.readouterr().out
    assert "index snapshot" not in out
    assert index_digest(model2.evidence_retriever.mips_index) == _pickle_digest(emb)
    assert not [n for n in os.listdir(os.path.join(tmp, "ckpt")) if n.startswith("evidence_index")]
