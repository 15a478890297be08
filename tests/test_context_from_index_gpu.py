"""GPU: --context-embeddings-from-index.  With the context encoder frozen, the prior over the K retrieved passages is computed from the
index rows the search returned (PreComputedEvidenceDocsRetriever.kept_embeddings -> kernels.retriever_prior_h16) and the context tower is
not run, in training or in evaluation mode.  The world is the tiny one of tests/test_index_writeback_gpu.py (2 layers, H 256, 9,000
passages, top-k 4, 4 questions), rebuilt here."""
import math
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.test_indexer_gpu import CLS, PAD, S_RET, SEP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DOCS, H, TOPK, B, S, L, VOCAB, EOS = 9000, 256, 4, 4, 128, 32, 2048, 2040


def _world(allow_trivial_doc=True, dropout=0.1, from_index=True, seed=0):
    """(model, retriever, index, host matrix, doc ids).  The index holds random fp16 rows: mantissa bits beyond bf16 in every value."""
    from emdr2_amd.data.emdr2_index import OpenRetreivalDataStore
    from emdr2_amd.data.evidence_arena import EvidenceArena
    from emdr2_amd.model import kernels as K
    from emdr2_amd.model.emdr2_model import EMDR2Model, PreComputedEvidenceDocsRetriever
    from emdr2_amd.model.transformer import Config
    arena = EvidenceArena.synthetic(N_DOCS, seed=5, vocab=2000)
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((N_DOCS, H)).astype(np.float16)
    ids = (rng.permutation(N_DOCS) + 1).astype(np.int32)                 # rows are not in doc-id order
    args = types.SimpleNamespace(topk_retrievals=TOPK, hidden_size=H, allow_trivial_doc=allow_trivial_doc, embedding_path=None, faiss_use_gpu=True,
                                 seq_length=S, seq_length_ret=S_RET)
    store = OpenRetreivalDataStore(embedding_path="/tmp/_emdr2_unused_from_index.pkl", load_from_path=False, rank=0)     # (never written)
    store.add_block_data(ids.tolist(), m)
    retr = PreComputedEvidenceDocsRetriever(args, arena, embed_data=store)
    cfg = Config(num_layers=2, hidden_size=H, num_attention_heads=4, ffn_hidden_size=512, max_position_embeddings=S, init_method_std=0.1,
                 hidden_dropout=dropout, attention_dropout=dropout)
    torch.manual_seed(1)
    K.DROPOUT._sites = 0
    model = EMDR2Model(retr, cfg, VOCAB, VOCAB, TOPK, S, S_RET, cls_id=CLS, sep_id=SEP, pad_id=PAD, disable_retriever_dropout=True,
                       no_context_embedder_training=True, context_embeddings_from_index=from_index)
    model.train()
    return model, retr, retr.mips_index, m, ids


def _batch(seed=0, uid=None, b=B):
    rng = np.random.default_rng(100 + seed)

    def tokens(shape, hi):
        x = rng.integers(5, hi, size=shape)
        for r in x:
            r[int(rng.integers(shape[1] // 2, shape[1] + 1)):] = 0
        return x
    q = tokens((B, S_RET // 2), 2000)
    q[1] = q[0]                                                          # two identical questions retrieve the same passages
    q = torch.from_numpy(q.astype(np.int64)).cuda()
    dec = torch.from_numpy(tokens((B, L), 600).astype(np.int64)).cuda()
    labels = torch.roll(dec, -1, 1); labels[:, -1] = 0
    uid = -torch.arange(1, B + 1, device="cuda") if uid is None else uid
    bt = dict(uid=uid, q=q, types=torch.zeros_like(q), qlen=(q != 0).sum(1), dec=dec, labels=labels, mask=(labels != 0).float())
    return {k: v[:b] for k, v in bt.items()}


def _forward(model, bt):
    return model(bt["uid"], bt["q"], bt["types"], None, bt["q"], bt["qlen"], bt["dec"])


def _step(model, bt):
    from emdr2_amd.model.emdr2_model import emdr2_loss
    lm, tlp, one = _forward(model, bt)
    loss, _ = emdr2_loss(lm, tlp, one, bt["labels"], bt["mask"], EOS)
    loss.backward()
    return loss, tlp


def _grouped_step(model, bt, groups):
    return model.forward_backward(bt["uid"], bt["q"], bt["types"], None, bt["q"], bt["qlen"], bt["dec"], bt["labels"], bt["mask"], EOS,
                                  micro_batches=groups)[0]


def _count_embedder_calls(model):
    calls, inner = {"query": 0, "context": 0}, model.retriever_embedder

    def wrapped(tokens, mask, types_, kind, disable_dropout=False):
        calls[kind] += 1
        return inner(tokens, mask, types_, kind, disable_dropout)
    model.retriever_embedder = wrapped
    return calls


def _query_embeddings(model, bt):
    with torch.no_grad():
        return model.retriever_embedder(bt["q"], None, bt["types"], "query", True)


def _reference_log_probs(index, q, kept):
    """float64 log_softmax_k(<q, E[kept rows]> / sqrt(H)) from the rows as the shard's local-row reader returns them"""
    e = index.shard.rows(kept.reshape(-1).clamp(min=0) - index.shard.row_base).reshape(kept.shape + (H,)).double()
    e = e * (kept >= 0).unsqueeze(-1)
    scores = torch.einsum("bh,bkh->bk", q.double(), e) / math.sqrt(H)
    return torch.log_softmax(scores, dim=1), scores


def _clear(model):
    for p in model.parameters():
        p.grad = None


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def test_the_prior_is_computed_from_the_stored_rows_and_the_context_tower_is_not_run():
    model, retr, index, m, ids = _world()
    calls = _count_embedder_calls(model)
    bt = _batch()
    q = _query_embeddings(model, bt)
    calls["query"] = 0
    lm, tlp, one = _forward(model, bt)
    assert calls == {"query": 1, "context": 0}
    kept = retr.last_kept_rows
    assert tuple(kept.shape) == (B, TOPK) and int(kept.min()) >= 0
    assert np.array_equal(index.shard.rows(kept.reshape(-1)).cpu().numpy().view(np.uint16), m[kept.reshape(-1).cpu().numpy()].view(np.uint16))
    ref, _ = _reference_log_probs(index, q, kept)
    worst = float((tlp.detach().double() - ref).abs().max())
    print("training mode: max |topk_log_probs - float64 reference| = %.3e" % worst)
    assert tlp.dtype == torch.float32 and tlp.requires_grad and worst <= 1e-4
    assert (m[kept.cpu().numpy()].astype(np.float32) != torch.from_numpy(m[kept.cpu().numpy()]).bfloat16().float().numpy()).any()   # bits beyond bf16
    # evaluation mode: the reference's four-tuple, the same prior, still no context call
    model.eval()
    with torch.no_grad():
        out = _forward(model, bt)
    assert len(out) == 4 and calls == {"query": 2, "context": 0}
    assert tuple(out[2].shape) == (B, TOPK * S, H) and tuple(out[3].shape) == (B, TOPK * S)
    assert float((out[1].double() - ref).abs().max()) <= 1e-4


def test_flag_on_and_flag_off_agree_over_an_index_built_from_the_frozen_tower():
    """The premise of the mode, stated on the log-probs: an index built by the indexer from the model's own (frozen, dropout-free) context
    tower holds that tower's outputs, so reading them back gives the prior the tower would have given -- to the project's bf16 bar, atol =
    2e-2 x max |score| (tests/test_index_writeback_gpu.py), not bitwise: the two paths run the tower at different batch sizes."""
    from emdr2_amd.indexer_emdr2 import IndexBuilder
    model, retr, index, m, ids = _world()
    random_rows = index.shard.digest()
    IndexBuilder(model.retriever_model.context_model, retr.arena, S_RET, CLS, SEP, PAD, batch_size=128).build_into_index(index, in_place=True)
    assert index.shard.digest() != random_rows                           # the index now holds the tower's embeddings
    bt = _batch()
    with torch.no_grad():
        on = _forward(model, bt)[1]
        kept_on = retr.last_kept_rows.clone()
        _, scores = _reference_log_probs(index, _query_embeddings(model, bt), kept_on)
        model.context_embeddings_from_index = False
        calls = _count_embedder_calls(model)
        off = _forward(model, bt)[1]
    assert calls["context"] == 1
    bar = 2e-2 * float(scores.abs().max())
    worst = float((on - off).abs().max())
    print("flag on vs off: max |log-prob difference| = %.3e, largest |score| %.3e (bar %.3e)" % (worst, float(scores.abs().max()), bar))
    assert worst <= bar


def test_gradients_reach_the_query_tower_only_and_equal_torch_autograd_of_the_formula(monkeypatch):
    from emdr2_amd.model import kernels as K
    model, retr, index, m, ids = _world(dropout=0.0)
    bt = _batch()
    _step(model, bt)
    for name, p in model.retriever_model.context_model.named_parameters():
        assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
    got = {k: p.grad.detach().clone() for k, p in model.retriever_model.query_model.named_parameters() if p.grad is not None}
    assert len(got) > 10 and all(float(g.abs().max()) > 0 for g in got.values())
    _clear(model)
    seen = []

    def by_autograd(q, c, scale):                                        # the same gathered rows, widened, through torch autograd
        assert c.dtype == torch.float16 and not c.requires_grad
        seen.append(c)
        return torch.log_softmax(torch.einsum("bh,bkh->bk", q.float(), c.float()) * scale, dim=1)
    monkeypatch.setattr(K, "retriever_prior_h16", by_autograd)
    _step(model, bt)
    assert len(seen) == 1
    want = {k: p.grad.detach().clone() for k, p in model.retriever_model.query_model.named_parameters() if p.grad is not None}
    assert set(got) == set(want)
    worst = max(float((got[k].double() - want[k].double()).abs().max() / want[k].double().abs().max()) for k in want)
    print("query-tower gradients, kernel vs torch autograd: worst relative difference %.3e" % worst)
    assert worst <= 2e-2


def test_question_groups_see_their_own_rows_of_the_one_gathered_buffer():
    """forward_backward in 2 groups against 1 group with the mode on, at the bars tests/test_microbatch_gpu.py uses for the same comparison
    (loss 2e-6 relative, gradients 2e-5 in relative norm; dropout off, so the groups' activations are those of the undivided step)."""
    model, retr, index, m, ids = _world(dropout=0.0)
    calls = _count_embedder_calls(model)
    bt = _batch()
    loss1 = _grouped_step(model, bt, 1)
    g1 = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    _clear(model)
    gathers, inner = [], retr.kept_embeddings
    retr.kept_embeddings = lambda: (gathers.append(1), inner())[1]
    loss2 = _grouped_step(model, bt, 2)
    g2 = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert len(gathers) == 1 and calls["context"] == 0                   # fetched once for all B questions, right after the one search
    assert abs(float(loss2) - float(loss1)) <= 2e-6 * abs(float(loss1))
    rel = lambda a, b: float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
    qt = [k for k in g1 if k.startswith("retriever_model.query_model.")]
    assert len(qt) > 10 and set(g1) == set(g2)
    worst = max(rel(g2[k], g1[k]) for k in qt)
    print("2 groups vs 1: loss %.9g vs %.9g, worst query-tower gradient difference %.3e (relative norm)" % (float(loss2), float(loss1), worst))
    assert worst < 2e-5
    assert not any(k.startswith("retriever_model.context_model.") for k in g2)
    # uneven groups: 3 questions in 2 groups (2 + 1)
    _clear(model)
    loss3 = _grouped_step(model, _batch(b=3), 2)
    assert math.isfinite(float(loss3)) and tuple(retr.last_kept_rows.shape) == (3, TOPK)


def test_without_trivial_docs_the_kept_rows_are_the_ones_used():
    model, retr, index, m, ids = _world(allow_trivial_doc=False)
    assert retr.topk == TOPK + 1
    bt = _batch()
    q = _query_embeddings(model, bt)
    with torch.no_grad():
        _, top = index.search_mips_index(q, TOPK + 1)
    searched_rows = index.last_search_rows.cpu().numpy()
    top = top.cpu().numpy()
    uid = torch.tensor([int(top[0, 1]), int(top[1, 1]), -3, -4], device="cuda")      # questions 0 and 1: their second hit is "their own" passage
    used, inner = [], retr.kept_embeddings
    retr.kept_embeddings = lambda: (used.append(inner()), used[-1])[1]
    bt = _batch(uid=uid)
    lm, tlp, one = _forward(model, bt)
    kept = retr.last_kept_rows
    kept_h = kept.cpu().numpy()
    for qi in range(B):
        dropped = 1 if qi < 2 else TOPK                                 # the trivial doc, or the surplus (K + 1)-th slot
        assert kept_h[qi].tolist() == [r for j, r in enumerate(searched_rows[qi].tolist()) if j != dropped]
    (emb,) = used
    assert emb.dtype == torch.float16 and tuple(emb.shape) == (B, TOPK, H)
    assert np.array_equal(emb.cpu().numpy().view(np.uint16), m[kept_h].view(np.uint16))
    ref, _ = _reference_log_probs(index, q, kept)
    assert float((tlp.detach().double() - ref).abs().max()) <= 1e-4
    assert torch.equal(tlp[0], tlp[1])                                   # two identical questions: identical priors


def test_frozen_means_frozen_over_two_optimizer_steps():
    from emdr2_amd.model import kernels as K
    from emdr2_amd.training import FlatAdam
    model, retr, index, m, ids = _world()
    try:
        opt = K.GRAD_SINK = FlatAdam(model, lr=1e-3, weight_decay=0.1, clip_grad=1.0, bucket_bytes=1 << 20)
        ctx0 = {k: p.detach().clone() for k, p in model.retriever_model.context_model.named_parameters()}
        qry0 = {k: p.detach().clone() for k, p in model.retriever_model.query_model.named_parameters()}
        digest0 = index.shard.digest()
        for step in range(2):
            opt.zero_grad()
            _grouped_step(model, _batch(seed=step), 2)
            opt.finish()
            opt.step()
        for k, p in model.retriever_model.context_model.named_parameters():
            assert torch.equal(_bits(p), _bits(ctx0[k])), k
        assert any(not torch.equal(p.detach(), qry0[k]) for k, p in model.retriever_model.query_model.named_parameters())     # the query tower learns
        assert index.shard.digest() == digest0
        assert np.array_equal(index.shard.rows(np.arange(N_DOCS)).cpu().numpy().view(np.uint16), m.view(np.uint16))
    finally:
        K.GRAD_SINK = None


# -- two ranks on the one GPU over gloo: a rank's kept rows live on both shards ------------------------------------------------------------
def _two_rank_worker(rank, world, port):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    model, retr, index, m, ids = _world(allow_trivial_doc=False)         # K + 1 searched, K kept: the slots are cut down on the device
    assert index.local_rows() == ((0, N_DOCS // 2) if rank == 0 else (N_DOCS // 2, N_DOCS))
    reduces, inner = [], torch.distributed.all_reduce
    torch.distributed.all_reduce = lambda t, *a, **kw: (reduces.append(tuple(t.shape)), inner(t, *a, **kw))[1]
    used, fetch = [], retr.kept_embeddings
    retr.kept_embeddings = lambda: (used.append(fetch()), used[-1])[1]
    bt = _batch(seed=10 + rank)                                          # each rank its own questions
    q = _query_embeddings(model, bt)
    lm, tlp, one = _forward(model, bt)
    torch.distributed.all_reduce = inner
    kept = retr.last_kept_rows
    kept_h = kept.cpu().numpy()
    assert (kept_h >= 0).all() and (kept_h < N_DOCS // 2).any() and (kept_h >= N_DOCS // 2).any()       # rows of both shards
    assert len(reduces) == 1                                             # ONE more collective per forward
    (emb,) = used
    assert tuple(emb.shape) == (B, TOPK, H) and np.array_equal(emb.cpu().numpy().view(np.uint16), m[kept_h].view(np.uint16))
    e = torch.from_numpy(m[kept_h]).cuda().double()
    ref = torch.log_softmax(torch.einsum("bh,bkh->bk", q.double(), e) / math.sqrt(H), dim=1)
    assert float((tlp.detach().double() - ref).abs().max()) <= 1e-4
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_fetch_their_kept_rows_through_one_exchange():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_two_rank_worker, args=(2, port), nprocs=2, join=True)


def test_the_task_s_model_provider_hands_the_flag_to_the_model():
    from emdr2_amd.data.emdr2_index import OpenRetreivalDataStore
    from emdr2_amd.data.evidence_arena import EvidenceArena
    from emdr2_amd.tasks.openqa.e2eqa.run import model_provider
    n = 600
    rng = np.random.default_rng(2)
    store = OpenRetreivalDataStore(embedding_path="/tmp/_emdr2_unused_from_index_task.pkl", load_from_path=False, rank=0)     # (never written)
    store.add_block_data(list(range(1, n + 1)), rng.standard_normal((n, 64)).astype(np.float16))
    tok = types.SimpleNamespace(cls=CLS, sep=SEP, pad=PAD)
    args = types.SimpleNamespace(task="OPENQA", topk_retrievals=TOPK, hidden_size=64, allow_trivial_doc=True, embedding_path=None, faiss_use_gpu=True,
                                 seq_length=S, seq_length_ret=S_RET, num_layers=1, num_attention_heads=1, ffn_hidden_size=128,
                                 max_position_embeddings=S, layernorm_epsilon=1e-5, init_method_std=0.02, hidden_dropout=0.1, attention_dropout=0.1,
                                 seed=1, t5_padded_vocab_size=VOCAB, bert_padded_vocab_size=VOCAB, update_retriever=True, retriever_score_scaling=True,
                                 checkpoint_activations=False, disable_retriever_dropout=True, no_query_embedder_training=False,
                                 no_context_embedder_training=True, context_embeddings_from_index=True)
    model = model_provider(args, tok, tok, arena=EvidenceArena.synthetic(n, seed=5, vocab=2000), embed_data=store)
    assert model.context_embeddings_from_index is True and model.no_context_embedder_training is True


def test_the_model_refuses_the_mode_over_a_trained_context_tower():
    from emdr2_amd.model.emdr2_model import EMDR2Model
    from emdr2_amd.model.transformer import Config
    cfg = Config(num_layers=1, hidden_size=64, num_attention_heads=1, ffn_hidden_size=128, max_position_embeddings=S)
    with pytest.raises(ValueError, match="no_context_embedder_training"):
        EMDR2Model(None, cfg, 128, 128, TOPK, S, S_RET, cls_id=CLS, sep_id=SEP, context_embeddings_from_index=True)
