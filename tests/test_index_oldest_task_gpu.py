"""GPU: --index-refresh-oldest-first at the builder and through the task entry point.

Builder: on an index whose stamps are all 0 the oldest-first refresher IS the sequential rolling refresher -- the same rows at the same
boundaries, so the same image and the same stamps after one pass.

Task: the six-step run of tests/test_index_newest_wins_task_gpu.py (300 rows, batches of 64, one per pump, both in-place writers,
newest-wins, an audit at every boundary) with the new flag.  The builder is constructed at iteration 0: its first pass has generation 0,
finds no row older than that and ends at its first boundary; the real pass takes its snapshot at step 2 (generation 1) and, skipping what
the write-back stamps meanwhile, has covered the shard by boundary 6.  The refresher never embeds a row it will not write: `kept newer`
stays 0, where the sequential refresher's run counts some."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_index_newest_wins_task_gpu import LINE, _check_lines, _run
from tests.test_task_gpu import _argv, _make_world

pytestmark = pytest.mark.gpu
PASS_LINE = re.compile(r"oldest-first pass (\d+) complete at iteration (\d+): (\d+) rows embedded, (\d+) slots padded")


def _world_builder(tmp, oldest_first):
    """the synthetic world's evidence, its embeddings in a stamped index (all stamps 0), a small context encoder -> a rolling refresher
    constructed at iteration 1, 64 rows per pump"""
    from emdr2_amd import arguments
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex, OpenRetreivalDataStore
    from emdr2_amd.model.transformer import Config, PretrainedBertModel
    from emdr2_amd.tasks.openqa.e2eqa.async_indexer import AsyncIndexBuilder
    from emdr2_amd.tasks.openqa.e2eqa.run import build_evidence_arena
    from emdr2_amd.tokenizer import BertWordPieceTokenizer
    vocab, ev, emb = _make_world(tmp)
    args = arguments.parse_args(_argv(tmp, vocab, ev, emb))
    t = BertWordPieceTokenizer(vocab)
    arena = build_evidence_arena(args)
    torch.manual_seed(5)
    cfg = Config(num_layers=2, hidden_size=128, num_attention_heads=2, ffn_hidden_size=256, max_position_embeddings=64, init_method_std=0.2)
    model = PretrainedBertModel(cfg, (t.vocab_size + 127) // 128 * 128)
    ids, rows = OpenRetreivalDataStore(emb, load_from_path=True).to_arrays()
    index = DistributedBruteForceIndex(128, None, generations=True)
    index.add_arrays(ids, rows)
    assert int(index.shard.generation.abs().max()) == 0
    return index, AsyncIndexBuilder(model, arena, index, 32, t.cls, t.sep, t.pad, batch_size=64, index_reload_interval=100, batches_per_pump=1,
                                    in_place=True, iteration=1, oldest_first=oldest_first)


def test_on_uniform_stamps_oldest_first_is_the_sequential_pass(tmp_path):
    built = []
    for name, oldest_first in (("seq", False), ("old", True)):
        tmp = str(tmp_path / name)
        os.makedirs(tmp)
        built.append(_world_builder(tmp, oldest_first))
    (index_s, seq), (index_o, old) = built
    assert index_s.shard.digest() == index_o.shard.digest()
    start = index_s.shard.digest()
    for it in range(2, 9):                                               # 300 rows at 64 per pump: the pass is complete at the fifth boundary
        for b in (seq, old):
            b.pump()
            b.maybe_swap(it)
        stamps_s, stamps_o = index_s.shard.generation.cpu().numpy(), index_o.shard.generation.cpu().numpy()
        assert np.array_equal(stamps_s, stamps_o), it                    # the same rows at the same boundaries
        assert index_s.shard.digest() == index_o.shard.digest(), it
        if old.passes:
            break
    assert it == 6 and seq.passes == 1 and old.passes == 1
    assert index_o.shard.digest() != start and (stamps_o[:300] == 1).all()
    assert (old.rows_selected, old.rows_padded) == (300, 5 * 64 - 300) and old.rows_padded < 64
    for index in (index_s, index_o):
        audit = index.audit()
        assert audit["sound"] and audit["canonical"], audit


def test_task_run_embeds_only_rows_it_will_write_and_covers_the_shard(tmp_path, capsys, monkeypatch):
    from emdr2_amd import arguments
    # `_run` puts ONE flag of the caller's on its command line: the second one is appended where the task's entry point parses it
    inner = arguments.parse_args
    monkeypatch.setattr(arguments, "parse_args", lambda argv=None: inner(list(argv) + ["--index-refresh-oldest-first"]))
    stamps, lines, out = _run(str(tmp_path / "oldest"), "--index-newest-wins", monkeypatch, capsys)
    _check_lines(stamps, lines, out)                                     # six steps trained, seven audits sound and canonical, the age lines parse
    assert len(LINE.findall(out)) == 6
    assert (np.diff(stamps, axis=0) >= 0).all()                          # monotone per row
    assert sum(l[7] for l in lines) == 0                                 # no row was embedded and then refused
    assert lines[-1][0] == 6 and lines[-1][5] <= 5                       # whole-index max age at iteration 6: every row written since step 1
    assert (stamps[-1] >= 1).all()
    passes = [tuple(int(v) for v in m.groups()) for m in PASS_LINE.finditer(out)]
    print(passes)
    assert passes[0] == (1, 1, 0, 64)                                    # generation 0: nothing is older, the pass ends at once
    # the pass of generation 1: 64 slots per pump from step 2 on; at most 16 rows per boundary are written back, at the four boundaries
    # 2..5 with a stamp the pass then skips -- between 236 and 300 rows are left to it, which takes four or five pumps
    number, iteration, embedded, padded = passes[1]
    assert number == 2 and iteration in (5, 6) and (embedded + padded) == (iteration - 1) * 64
    assert 300 - 4 * 16 <= embedded <= 300 and padded < 64


def test_without_the_flag_the_run_prints_no_new_line(tmp_path, capsys, monkeypatch):
    """the sequential refresher's run on this commit: the lines the existing test's expectations describe, and nothing of the new form"""
    stamps, lines, out = _run(str(tmp_path / "sequential"), "--index-newest-wins", monkeypatch, capsys)
    _check_lines(stamps, lines, out)
    assert (np.diff(stamps, axis=0) >= 0).all() and sum(l[7] for l in lines) > 0
    assert "oldest-first" not in out
