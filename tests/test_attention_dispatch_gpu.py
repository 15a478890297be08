"""The attention dispatch (kernels._AttnLaunch): one launch description per call, built at the forward and read by the backward.

What the numbers are is tests/test_attention_edges_gpu.py's business; these tests pin the DECISIONS: a checkpointed layer's re-run (the stash's
consume branch) launches the backward the first run's forward planned, a call's backward runs the route its forward chose whatever happens to
the plan table in between, and both precisions refuse token ids their kernels would misread."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(q0, kv0, ids_q, ids_k, dO, drop_p, stash, between=None):
    """attention_core forward + backward on fresh leaves -> (O, dQ, dKV, the call's launch).  stash: the way transformer._CheckpointedLayer runs
    a layer -- a no-grad first run that stores, then the re-run that consumes.  between: called between the forward and the backward."""
    from emdr2_amd.model import kernels as K
    q, kv = q0.clone().requires_grad_(True), kv0.clone().requires_grad_(True)
    mode, key = K.ATTN_STASH.mode, K.ATTN_STASH.key
    try:
        if stash:
            K.ATTN_STASH.mode, K.ATTN_STASH.key = 'store', 'dispatch-test'
            with torch.no_grad():
                first = K.attention_core(q, kv, ids_q, ids_k, False, drop_p, 11, site=1)
            assert len(K.ATTN_STASH.store) == 1
            K.ATTN_STASH.mode = 'consume'
        out = K.attention_core(q, kv, ids_q, ids_k, False, drop_p, 11, site=1)
        if stash:
            assert out.data_ptr() == first.data_ptr()                    # the re-run launched nothing: it is the first run's output
        if between is not None:
            between()
        out.backward(dO)
    finally:
        K.ATTN_STASH.mode, K.ATTN_STASH.key = mode, key
    torch.cuda.synchronize()
    assert len(K.ATTN_STASH.store) == 0
    return out.detach(), q.grad, kv.grad, out.grad_fn.launch


def _same(a, b):
    for name, x, y in zip(("O", "dQ", "dKV"), a, b):
        assert torch.equal(x, y), name


def test_checkpoint_rerun_of_a_split_key_launch():
    """b 1, one head, 32 queries over 4,096 dense keys: the smallest shape that splits (two ranges, the second ending in padding), with
    dropout.  The consume branch used to re-derive the route with its own copy of the fused-eligibility rule."""
    from emdr2_amd.model import kernels as K
    K.ATTN_STASH.store.clear()
    g = torch.Generator(device=DEV).manual_seed(5)
    q = torch.randn((1, 32, 1, 64), generator=g, device=DEV).bfloat16()
    kv = torch.randn((1, 4096, 2, 1, 64), generator=g, device=DEV).bfloat16()
    dO = torch.randn((1, 32, 1, 64), generator=g, device=DEV).bfloat16()
    ids_q = torch.full((1, 32), 7, dtype=torch.int64, device=DEV)
    ids_k = torch.full((1, 4096), 7, dtype=torch.int64, device=DEV)
    ids_k[0, 4000:] = 0
    assert K._splitkv_plan(1, 1, 32, 4096)[0] == 2
    a = _run(q, kv, ids_q, ids_k, dO, 0.1, stash=False)
    b = _run(q, kv, ids_q, ids_k, dO, 0.1, stash=True)
    assert a[3].ksplit == b[3].ksplit == 2
    _same(a, b)


@pytest.mark.parametrize("clear_between", [False, True])
def test_forced_unsplit_plan_over_packed_grouped_keys(clear_between):
    """Dense decoder queries over PackedSeqs.grouped keys (question 0: 4,224 keys, question 1: three) with the plan forced to `do not split`:
    a varlen launch in both directions, also in the checkpointed re-run, also when the plan table is emptied between a call's forward and its
    backward (the backward reads the plan its forward captured, not the table)."""
    from emdr2_amd.model import kernels as K
    B, Kk, S, L, heads = 2, 3, 1408, 32, 1
    ids = torch.zeros((B * Kk, S), dtype=torch.int64, device=DEV)
    ids[:Kk] = 7
    ids[Kk:, 0] = 7
    seqs = K.PackedSeqs(ids)
    gk = seqs.grouped(Kk)
    assert gk.max_len >= 4096
    g = torch.Generator(device=DEV).manual_seed(6)
    q = torch.randn((B, L, heads, 64), generator=g, device=DEV).bfloat16()
    kv = seqs.zero_tail(torch.randn((seqs.rows, 2, heads, 64), generator=g, device=DEV).bfloat16())
    dO = torch.randn((B, L, heads, 64), generator=g, device=DEV).bfloat16()
    dec = torch.full((B, L), 7, dtype=torch.int64, device=DEV)
    dec[1, L - 2:] = 0
    key = (B, heads, L, gk.max_len)
    K.ATTN_STASH.store.clear()
    K._SPLITKV_PLANS.clear()
    try:
        assert K._splitkv_plan(*key)[0] > 1                             # left alone this shape splits
        split = _run(q, kv, dec, gk, dO, 0.1, stash=False)
        assert split[3].ksplit > 1
        K._SPLITKV_PLANS[key] = (1, 0, 0)
        ref = _run(q, kv, dec, gk, dO, 0.1, stash=False)
        assert ref[3].ksplit == 1
        between = K._SPLITKV_PLANS.clear if clear_between else None
        for stash in (False, True):
            K._SPLITKV_PLANS[key] = (1, 0, 0)
            got = _run(q, kv, dec, gk, dO, 0.1, stash=stash, between=between)
            assert got[3].ksplit == 1
            _same(ref, got)
    finally:
        K._SPLITKV_PLANS.clear()


def test_both_precisions_refuse_token_ids_the_kernels_would_misread():
    """The kernels read token ids as contiguous int64 [batch, s]: anything else would give silently wrong masks or reads out of bounds."""
    from emdr2_amd.model import kernels as K
    g = torch.Generator(device=DEV).manual_seed(7)
    qkv = torch.randn((1, 32, 3, 1, 32), generator=g, device=DEV)
    ids = torch.full((1, 32), 7, dtype=torch.int64, device=DEV)
    ids[0, 30:] = 0
    strided = torch.full((1, 64), 7, dtype=torch.int64, device=DEV)[:, ::2]
    assert strided.shape == ids.shape and not strided.is_contiguous()
    with pytest.raises(TypeError):
        K.attention_core(qkv, None, ids.int(), ids.int())
    with pytest.raises(TypeError):
        K.attention_core(qkv, None, strided, strided)
    with pytest.raises(TypeError):
        K.attention_core(qkv, None, ids, strided)
    for x in (qkv, qkv.bfloat16()):
        with pytest.raises(ValueError):
            K.attention_core(x, None, ids[:, :16].contiguous(), ids[:, :16].contiguous())
        with pytest.raises(ValueError):
            K.attention_core(x, None, ids, ids[:, :16].contiguous())
        out = K.attention_core(x, None, ids, ids)
        torch.cuda.synchronize()
        assert out.shape == (1, 32, 1, 32) and out.dtype == x.dtype and bool(torch.isfinite(out.float()).all())
