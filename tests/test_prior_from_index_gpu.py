"""GPU: the retriever prior over fp16 contexts (kernels.retriever_prior_h16; csrc/loss_tail.hip: the prior kernels instantiated for the
index's element type).  With --context-embeddings-from-index the K contexts of a question are rows gathered from the evidence index: fp16
constants, widened exactly inside the kernel -- not cast to bf16, which would drop three mantissa bits of every stored value.  The
references are float64 torch computations of the same formula on the same bits."""
import hashlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _reference(q, c, scale, w):
    """float64: log_softmax_k(<q, c_k> * scale) and d/dq of sum(logp * w)"""
    qr = q.detach().double().requires_grad_(True)
    ref = torch.log_softmax(torch.einsum("bh,bkh->bk", qr, c.double()) * scale, dim=1)
    (ref * w.double()).sum().backward()
    return ref.detach(), qr.grad


@pytest.mark.parametrize("B,Kk,H,scaled", [(64, 50, 768, True), (8, 101, 768, True), (3, 7, 128, False), (4, 129, 64, True), (2, 1000, 128, True),
                                           (1, 1, 64, True)])
def test_values_and_query_gradient_against_float64(B, Kk, H, scaled):
    """The bars are those of the bf16-context kernel (test_ops_gpu.py): values rtol = atol = 1e-4 (fp32 accumulation of exact products);
    dq, which is stored as bf16 (relative spacing 2^-8), 2e-2 relative to the largest gradient magnitude."""
    from emdr2_amd.model import kernels as K
    g = torch.Generator(device=DEV).manual_seed(B * Kk + H)
    q = torch.randn((B, H), generator=g, device=DEV).bfloat16().requires_grad_(True)
    c = torch.randn((B, Kk, H), generator=g, device=DEV).half()
    w = torch.randn((B, Kk), generator=g, device=DEV)
    scale = 1.0 / H ** 0.5 if scaled else 1.0
    out = K.retriever_prior_h16(q, c, scale)
    (out * w).sum().backward()
    ref, dq = _reference(q, c, scale, w)
    worst = float((out.detach().double() - ref).abs().max())
    gworst, gmax = float((q.grad.double() - dq).abs().max()), float(dq.abs().max())
    print("prior_h16 %s: max |logp - ref| = %.3e; max |dq - ref| = %.3e of %.3e" % ((B, Kk, H), worst, gworst, gmax))
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, Kk) and q.grad.dtype == torch.bfloat16
    assert torch.allclose(out.detach().double(), ref, rtol=1e-4, atol=1e-4)
    assert torch.allclose(q.grad.double(), dq, rtol=2e-2, atol=2e-2 * gmax)
    if Kk == 1:                                                          # one passage: log-probability 0 and no gradient, exactly
        assert float(out.detach().abs().max()) == 0.0 and float(q.grad.abs().max()) == 0.0


def test_the_fp16_bits_are_used():
    """c[k] = (1 + k/1024) e0 is exact in fp16; in bf16 (8 significant bits) c[0..3] and c[4..7] collapse onto 1 and 1.03125.  q = 64 e0:
    every product and sum is exact in fp32, so logp[k] - logp[0] = 64 k / 1024 = k / 16.  A kernel that reads the contexts as bf16, or a
    caller that casts them, gives 0 for k < 4."""
    from emdr2_amd.model import kernels as K
    q = torch.zeros((1, 64), device=DEV); q[0, 0] = 64.0
    c = torch.zeros((1, 8, 64), device=DEV); c[0, :, 0] = 1.0 + torch.arange(8, device=DEV) / 1024.0
    ch = c.half()
    assert torch.equal(ch.float(), c)                                    # exact in fp16 ...
    assert int(torch.unique(c.bfloat16().float()[0, :, 0]).numel()) < 8  # ... and not in bf16
    logp = K.retriever_prior_h16(q.bfloat16(), ch, 1.0)
    want = torch.arange(8, device=DEV) / 16.0
    got = logp[0] - logp[0, 0]
    print("logp[k] - logp[0]:", got.tolist())
    assert float((got - want).abs().max()) <= 1e-5


def test_more_than_1024_passages_and_contexts_that_require_grad_are_refused():
    from emdr2_amd import _native
    from emdr2_amd.model import kernels as K
    q, c = torch.zeros((2, 64), device=DEV).bfloat16(), torch.zeros((2, 1025, 64), device=DEV).half()
    with pytest.raises(_native.NativeError, match="-4"):
        K.retriever_prior_h16(q, c, 1.0)
    with pytest.raises(ValueError, match="require grad"):
        K.retriever_prior_h16(q, torch.zeros((2, 8, 64), device=DEV).half().requires_grad_(True), 1.0)
    with pytest.raises(TypeError):
        K.retriever_prior_h16(q, torch.zeros((2, 8, 64), device=DEV).bfloat16(), 1.0)     # bf16 contexts belong to retriever_prior
    # the query may be a constant too (--no-query-embedder-training): nothing to differentiate, nothing launched in the backward
    out = K.retriever_prior_h16(q, torch.zeros((2, 8, 64), device=DEV).half(), 1.0)
    assert not out.requires_grad


# sha256 over (logp fp32, dq bf16, dc bf16) of kernels.retriever_prior on the seeded input below, taken from the library as it was built
# BEFORE the prior kernels became templates over the context element
_BF16_DIGESTS = {
    (8, 101, 768): "abb478310e39930978dedc1dbf88b5d74d9cff80861dc0eea2f8b7716a9f299a",
    (3, 7, 128): "264a4f8ffb4bbb0a60018bd692f4b1a0ec9660f58ef2e4837fc554ffa2d44f7a",
}


@pytest.mark.parametrize("shape", sorted(_BF16_DIGESTS))
def test_the_bf16_entry_is_bit_identical_to_what_it_was_before_the_kernels_became_templates(shape):
    from emdr2_amd.model import kernels as K
    B, Kk, H = shape
    g = torch.Generator().manual_seed(20260 + B * Kk + H)                # (the CPU generator: the same stream on every machine)
    q = torch.randn((B, H), generator=g).bfloat16().to(DEV).requires_grad_(True)
    c = torch.randn((B, Kk, H), generator=g).bfloat16().to(DEV).requires_grad_(True)
    w = torch.randn((B, Kk), generator=g).to(DEV)
    out = K.retriever_prior(q, c, 1.0 / H ** 0.5)
    (out * w).sum().backward()
    h = hashlib.sha256()
    for t in (out.detach(), q.grad.view(torch.int16), c.grad.view(torch.int16)):
        h.update(t.cpu().numpy().tobytes())
    assert h.hexdigest() == _BF16_DIGESTS[shape]
