"""GPU: `--save-index-deltas` through the task entry point, on the synthetic world of tests/test_task_gpu.py: both in-place writers (the
rolling refresher and the write-back) change the live index at every step boundary, checkpoints fall between index updates, and a resumed
run searches the index its checkpoint was searching -- the published snapshot plus the delta of that checkpoint."""
import os

import pytest
import torch

from tests.test_task_gpu import _argv, _make_world

pytestmark = pytest.mark.gpu
# (later flags override _argv's: --save-interval 3 puts a checkpoint at iterations 3 and 6, index updates fall on 2, 4 and 6)
FLAGS = ("--save-index-snapshot", "--save-index-deltas", "--index-refresh-in-place", "--index-writeback", "--index-generations",
         "--disable-retriever-dropout", "--save-interval", "3")


def test_a_resumed_run_searches_the_index_of_its_checkpoint(tmp_path, capsys):
    from emdr2_amd import checkpointing
    from emdr2_amd.data import index_snapshot as snap
    from emdr2_amd.tasks import run as task_run
    tmp = str(tmp_path)
    vocab, ev, emb = _make_world(tmp)
    ckpt = os.path.join(tmp, "ckpt")
    path = os.path.join(ckpt, "evidence_index.flat")
    model, _ = task_run.main(_argv(tmp, vocab, ev, emb, extra=FLAGS))
    out = capsys.readouterr().out
    last = checkpointing.read_tracker(ckpt)[0]
    assert last == 6 and "index delta: " in out
    print("\n".join(line for line in out.splitlines() if "index delta" in line or "index snapshot" in line))
    assert sorted(n for n in os.listdir(ckpt) if n.startswith("evidence_index")) == [
        "evidence_index.flat", "evidence_index.flat.delta", "evidence_index.flat.delta.meta", "evidence_index.flat.gen", "evidence_index.flat.meta"]
    meta = snap.read_delta_meta(path)
    assert meta["iteration"] == last and meta["n"] == 300 and meta["base"] == snap.base_of(snap.read_snapshot_meta(path))
    live = model.evidence_retriever.mips_index
    digest, stamp_digest = snap.index_digest(live), snap.index_stamp_digest(live)
    assert (int(meta["result"]["digest_sum"], 16), int(meta["result"]["digest_xor"], 16)) == digest
    assert (int(meta["result"]["stamps"]["digest_sum"], 16), int(meta["result"]["stamps"]["digest_xor"], 16)) == stamp_digest
    queries = torch.randn((9, 128), generator=torch.Generator().manual_seed(3)).half().cuda()
    found = live.search_mips_index(queries, 4)

    # the same arguments again: the checkpoint of iteration 6 is loaded, nothing is left to train, the index is base + delta
    model2, _ = task_run.main(_argv(tmp, vocab, ev, emb, extra=FLAGS))
    out2 = capsys.readouterr().out
    assert "index snapshot %s loaded" % path in out2 and "delta of iteration %d applied" % last in out2
    assert "stamped beyond" not in out2                                                    # no row is newer than the checkpoint
    index = model2.evidence_retriever.mips_index
    assert index.delta_applied == meta
    assert snap.index_digest(index) == digest and snap.index_stamp_digest(index) == stamp_digest
    again = index.search_mips_index(queries, 4)
    assert torch.equal(found[0], again[0]) and torch.equal(found[1], again[1])
    assert index.generation_stats(last)["from_future"] == 0


def test_without_the_flag_the_directory_holds_what_it_held(tmp_path, capsys):
    from emdr2_amd.tasks import run as task_run
    tmp = str(tmp_path)
    vocab, ev, emb = _make_world(tmp)
    flags = tuple(f for f in FLAGS if f != "--save-index-deltas")
    model, _ = task_run.main(_argv(tmp, vocab, ev, emb, extra=flags))
    out = capsys.readouterr().out
    assert "index delta" not in out and model.evidence_retriever.mips_index.delta_base is None
    assert sorted(n for n in os.listdir(os.path.join(tmp, "ckpt")) if n.startswith("evidence_index")) == [
        "evidence_index.flat", "evidence_index.flat.gen", "evidence_index.flat.meta"]


def test_the_flag_needs_the_snapshot_flag(tmp_path):
    from emdr2_amd.arguments import parse_args
    tmp = str(tmp_path)
    argv = _argv(tmp, "vocab", "ev", "emb", extra=("--save-index-deltas",))
    with pytest.raises(ValueError, match="--save-index-snapshot"):
        parse_args(argv)
    assert parse_args(argv + ["--save-index-snapshot"]).save_index_deltas
