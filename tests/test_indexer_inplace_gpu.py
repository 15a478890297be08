"""GPU: the rolling evidence refresh (--index-refresh-in-place).  `IndexBuilder.build_into_index(in_place=True)` and the side-stream
`AsyncIndexBuilder(in_place=True)` write re-embedded rows into the image that is being searched (`update_rows`): no spare image is ever
allocated, what the index holds at a step is a function of the step number alone, and a completed pass leaves exactly the index a
synchronous rebuild leaves."""
import ctypes
import gc
import os

import numpy as np
import pytest
import torch

from tests.test_indexer_gpu import CLS, PAD, S_RET, SEP, _search, _setup
from tests.test_task_gpu import _argv, _make_world

pytestmark = pytest.mark.gpu


def _embed_all(builder, n_docs, batch=128):
    return torch.cat([builder.embed(torch.arange(s, min(s + batch, n_docs + 1))) for s in range(1, n_docs + 1, batch)]).cpu().numpy()


def _index_of(ids, rows, cls=None):
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex
    index = (cls or DistributedBruteForceIndex)(rows.shape[1], None)
    index.add_arrays(ids, rows)
    return index


def _same_search(a, b, dim):
    (d0, i0), (d1, i1) = _search(a, dim=dim), _search(b, dim=dim)
    return np.array_equal(d0, d1) and np.array_equal(i0, i1)


def _stored(index):
    return index.shard.rows(np.arange(index.shard.n_rows)).cpu().numpy()


def _move_weights(model):
    """"training": the live weights move after the snapshot was taken (raw-pointer style update + cache invalidation)"""
    from emdr2_amd.model import kernels as K
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    K.WEIGHTS.invalidate()


def _main_stream_work(model):
    return model(torch.randint(1, 2000, (4, S_RET), device="cuda"), torch.zeros((4, S_RET), dtype=torch.int64, device="cuda"))


def test_rolling_refresher_applies_what_was_pumped_at_the_next_step_boundary():
    from emdr2_amd.indexer_emdr2 import IndexBuilder
    from emdr2_amd.tasks.openqa.e2eqa.async_indexer import AsyncIndexBuilder
    model, arena = _setup(n_docs=1000, seed=3)
    n = arena.n_docs
    sync = IndexBuilder(model, arena, S_RET, CLS, SEP, PAD, batch_size=128)
    ids = np.arange(1, n + 1, dtype=np.int32)
    rows0 = _embed_all(sync, n)                                          # embeddings of the weights the first snapshot takes
    old = np.random.default_rng(0).standard_normal(rows0.shape).astype(np.float16)
    index = _index_of(ids, old)
    indexer = AsyncIndexBuilder(model, arena, index, S_RET, CLS, SEP, PAD, batch_size=128, index_reload_interval=3, batches_per_pump=2,
                                in_place=True)
    _move_weights(model)
    no_spare = lambda: index.shard._spare is None and index.shard._spare_shadow_buf is None
    returned = []
    for it in range(1, 7):                                               # 8 batches at 2 per step: the pass completes at step 4
        indexer.pump()
        _ = _main_stream_work(model)
        if it <= 4:                                                      # nothing enters the image before the boundary
            done = 256 * (it - 1)
            assert np.array_equal(_stored(index), np.concatenate([rows0[:done], old[done:]]))
        returned.append(indexer.maybe_swap(it))
        assert no_spare()
        if it == 1:                                                      # rows 0..255 of the snapshot's embeddings, then the old rows
            mixed = np.concatenate([rows0[:256], old[256:]])
            assert np.array_equal(_stored(index), mixed)
            assert _same_search(index, _index_of(ids, mixed), 128)
        if it == 4:                                                      # the pass is complete: a synchronous rebuild from the snapshot
            assert np.array_equal(_stored(index), rows0)
            assert _same_search(index, _index_of(ids, rows0), 128)
            assert indexer.passes == 1
    assert returned == [False, False, True, False, False, True]          # the interval condition alone, whatever the state of the pass
    # the second pass started, at once, from the weights that had moved: drain it and compare with a synchronous build from the live model
    assert indexer.maybe_swap(100, force=True)
    rows1 = _embed_all(sync, n)
    assert not np.array_equal(rows1, rows0)
    assert np.array_equal(_stored(index), rows1)
    assert _same_search(index, _index_of(ids, rows1), 128)
    assert no_spare() and indexer.passes == 2
    assert indexer.maybe_swap(101) is False and indexer.maybe_swap(103) is True


def _setup_256(n_docs):
    from emdr2_amd.data.evidence_arena import EvidenceArena
    from emdr2_amd.model.transformer import Config, PretrainedBertModel
    torch.manual_seed(7)
    cfg = Config(num_layers=2, hidden_size=256, num_attention_heads=4, ffn_hidden_size=512, max_position_embeddings=S_RET, init_method_std=0.2,
                 hidden_dropout=0.1, attention_dropout=0.1)
    return PretrainedBertModel(cfg, 2000), EvidenceArena.synthetic(n_docs, seed=5, vocab=2000)


def _shadowed_index_class():
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex, HipIndexShard

    class ShadowedIndex(DistributedBruteForceIndex):
        def _make_shard(self, dim, n_rows, row_base):
            return HipIndexShard(dim, n_rows, row_base, shadow_min_rows=1)
    return ShadowedIndex


def _refresh_with_a_shadow(in_place):
    """One pass of the side-stream refresher over a 9,000-row shard that has an int8 shadow, then a forced second pass, in either mode.
    -> peak bytes allocated over the whole run, from the refresher's construction to the last comparison."""
    from emdr2_amd.indexer_emdr2 import IndexBuilder
    from emdr2_amd.tasks.openqa.e2eqa.async_indexer import AsyncIndexBuilder
    n, dim = 9000, 256
    gc.collect()                                                         # both runs start from the same allocator state: nothing of an earlier
    torch.cuda.synchronize()                                             # run alive, no cached block that a request could be served from unsplit
    torch.cuda.empty_cache()                                             # (such a request is counted at the size of the block it got)
    model, arena = _setup_256(n)
    sync = IndexBuilder(model, arena, S_RET, CLS, SEP, PAD, batch_size=128)
    ids = np.arange(1, n + 1, dtype=np.int32)
    rows0 = _embed_all(sync, n)
    cls = _shadowed_index_class()
    index = _index_of(ids, np.random.default_rng(0).standard_normal(rows0.shape).astype(np.float16), cls)
    assert index.shard._shadow is not None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    trace = []
    mark = lambda what: trace.append("%-28s allocated %11d B, peak so far %11d B" % (what, torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()))
    mark("start")
    indexer = AsyncIndexBuilder(model, arena, index, S_RET, CLS, SEP, PAD, batch_size=128, index_reload_interval=2, batches_per_pump=12,
                                in_place=in_place)
    _move_weights(model)
    mark("refresher constructed")
    for it in range(1, 7):                                               # 71 batches at 12 per step: the pass is in at the sixth boundary
        if indexer.pump() and not in_place:
            indexer.stream.synchronize()                                 # (the swap mode asks whether the pass HAS finished)
        _ = _main_stream_work(model)
        indexer.maybe_swap(it)
        mark("boundary %d" % it)
        if in_place:
            assert index.shard._spare is None and index.shard._spare_shadow_buf is None
    fresh = _index_of(ids, rows0, cls)
    torch.cuda.synchronize()
    assert np.array_equal(_stored(index), rows0)
    for mine, theirs in zip(index.shard._shadow, fresh.shard._shadow):   # int8 image and block table as a fresh shard seals them
        assert torch.equal(mine.view(torch.uint8), theirs.view(torch.uint8))
    assert _same_search(index, fresh, dim)
    mark("compared with a fresh index")
    del fresh
    assert indexer.maybe_swap(100, force=True)
    mark("second pass forced")
    rows1 = _embed_all(sync, n)                                          # (the run's peak: one batch's activations on top of 4 MB of embeddings)
    assert np.array_equal(_stored(index), rows1) and index.shard._shadow is not None
    torch.cuda.synchronize()
    mark("end")
    peak = torch.cuda.max_memory_allocated()
    print("\n%s refresh of %d x %d with a shadow:\n  %s" % ("rolling" if in_place else "swap", n, dim, "\n  ".join(trace)))
    assert (index.shard._spare is None and index.shard._spare_shadow_buf is None) == in_place
    return peak, index.shard


def test_rolling_refresher_with_a_shadow_reseals_in_place_and_holds_no_spare_images():
    """After a full rolling pass the shadow buffers are byte-equal to a fresh shard's, and the run's peak of allocated device memory lies
    below the swap mode's by at least the spare fp16 image plus the spare int8 shadow (image and block table) of the shard."""
    peak_swap, shard = _refresh_with_a_shadow(in_place=False)
    del shard
    peak_rolling, shard = _refresh_with_a_shadow(in_place=True)
    image, shadow_image, shadow_table = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert shard.lib.emdr2_mips_layout_bytes(shard.n_rows, shard.dim, ctypes.byref(image)) == 0
    assert shard.lib.emdr2_mips_shadow_bytes(shard.n_rows, shard.dim, ctypes.byref(shadow_image), ctypes.byref(shadow_table)) == 0
    spare = image.value + shadow_image.value + shadow_table.value
    print("max_memory_allocated: swap %d B, rolling %d B, difference %d B; spare image + spare shadow %d B" %
          (peak_swap, peak_rolling, peak_swap - peak_rolling, spare))
    # (both peaks fall into the comparison with a fresh index, whose search allocates a workspace: the rolling run holds no staging rows then,
    # only its block-norm table; the swap run holds the spare image, the spare shadow and the spare emax_sq)
    assert peak_swap - peak_rolling >= spare


def test_synchronous_in_place_build_equals_the_swap_build():
    from emdr2_amd.indexer_emdr2 import IndexBuilder
    model, arena = _setup(n_docs=700, seed=2)
    builder = IndexBuilder(model, arena, S_RET, CLS, SEP, PAD, batch_size=96)
    ids = (np.random.default_rng(4).permutation(arena.n_docs) + 1).astype(np.int32)            # rows are not in doc-id order
    stale = np.random.default_rng(0).standard_normal((arena.n_docs, 128)).astype(np.float16)
    a, b = _index_of(ids, stale), _index_of(ids, stale)
    builder.build_into_index(a, in_place=True)
    builder.build_into_index(b)
    assert a.shard._spare is None and b.shard._spare is not None
    assert np.array_equal(_stored(a), _stored(b)) and not np.array_equal(_stored(a), stale)
    assert torch.equal(a.shard.tiled, b.shard.tiled) and torch.equal(a.shard.emax_sq.view(torch.int32), b.shard.emax_sq.view(torch.int32))
    assert _same_search(a, b, 128)


def test_task_entry_point_with_the_in_place_refresh(tmp_path, capsys):
    from emdr2_amd import checkpointing
    from emdr2_amd.data.emdr2_index import OpenRetreivalDataStore
    from emdr2_amd.tasks import run as task_run
    tmp = str(tmp_path)
    vocab, ev, emb = _make_world(tmp)
    _, initial = OpenRetreivalDataStore(emb, load_from_path=True).to_arrays()
    model, results = task_run.main(_argv(tmp, vocab, ev, emb, extra=("--index-refresh-in-place",)))
    out = capsys.readouterr().out
    assert "MIPS Index Updated" in out and "lm_loss" in out and "Exact Match Score" in out
    assert results["validation"][1] == 8
    assert checkpointing.read_tracker(os.path.join(tmp, "ckpt"))[0] == 6   # 24 questions / batch 4: all six steps trained
    shard = model.evidence_retriever.mips_index.shard
    now = shard.rows(np.arange(shard.n_rows)).cpu().numpy()
    assert now.shape == initial.shape and not np.array_equal(now, initial)
    assert (now != initial).any(axis=1).all()                            # a whole pass went in: every row was re-embedded
    assert shard._spare is None and shard._spare_shadow_buf is None
