"""CPU: the value-norm weighted attention mass and the attention-distillation retriever loss without a GPU.

  * tests/attention_mass_weighted_ref.py against brute-force python loops on tiny inputs;
  * `distill_kl` against python floats: zero rows, zero entries, its gradient -t / B;
  * the argument rules of --retriever-distill-attention and --attention-mass-value-norms at the parser and at the model build;
  * argument validation of emdr2_attention_key_mass_weighted and emdr2_head_row_norms through the library (-1 / -4, no launch);
  * register budget: both instances of the mass kernel and the norms kernel exist, without spills or a private segment."""
import ctypes
import math
import os
import sys

import pytest
import torch

from tests import attention_mass_ref as MR
from tests import attention_mass_weighted_ref as WR
from tests import attention_ref as R
from tests.test_attention_mass_cpu import _tiny
from tests.test_context_from_index_cpu import BASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the references ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["randn", "one_hot"])
@pytest.mark.parametrize("weighted", [False, True])
def test_weighted_reference_against_brute_force(fam, weighted):
    q, k, ids_q, ids_k, seg, w = _tiny(5, fam=fam)
    w = w if weighted else None
    g = torch.Generator().manual_seed(11)
    kw = torch.rand((k.shape[1], k.shape[2]), generator=g, dtype=torch.float64) * 3.75 + 0.25
    kw[4, 0] = 0.0                                                          # an exact zero inside a segment
    r = R.reference(q, k, torch.zeros_like(k), ids_q, ids_k, False)
    m, l = MR.made_stats(r)
    mass, bound = WR.weighted_mass_reference(q, list(k), ids_q, list(ids_k), m, l, seg, [kw], w)
    brute = torch.tensor(WR.brute_force_weighted_mass(q[0], k[0], ids_q[0], ids_k[0], seg[0].tolist(), kw.tolist(), None if w is None else w[0]),
                         dtype=torch.float64)
    # (m, l) are fp32 roundings of the float64 statistics: the two agree to that rounding, far inside the bound
    assert float((mass[0] - brute).abs().max()) <= 4 * 2.0 ** -24 * float(brute.abs().max())
    assert float(mass[0, :, 1].abs().max()) == 0.0                          # the empty segment
    assert bool((bound > 0).all())
    # kw = 1: the unweighted reference itself, and a bound that is larger by the one multiplication only
    ones = torch.ones_like(kw)
    mass1, bound1 = WR.weighted_mass_reference(q, list(k), ids_q, list(ids_k), m, l, seg, [ones], w)
    mass0, bound0, _ = MR.mass_reference(q, list(k), ids_q, list(ids_k), m, l, seg, w)
    assert torch.equal(mass1, mass0) and bool((bound1 >= bound0).all()) and bool((bound1 <= bound0 * 1.5 + 1e-30).all())
    # a table that is off by kw_errs is held by the kw_errs term
    off = kw * (1 + 1e-3)
    mass_off, _ = WR.weighted_mass_reference(q, list(k), ids_q, list(ids_k), m, l, seg, [off], w)
    _, bound_err = WR.weighted_mass_reference(q, list(k), ids_q, list(ids_k), m, l, seg, [kw], w, kw_errs=[kw * 1e-3])
    assert bool(((mass_off - mass).abs() <= bound_err).all())


def test_norms_reference_against_python_floats_and_its_bound():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((9, 3, 64), generator=g).bfloat16().float()
    x[2] = 0
    x[3] *= 2.0 ** -70
    x[4] *= 2.0 ** 60
    norm, bound = WR.norms_reference(x)
    brute = torch.tensor(WR.brute_force_norms(x), dtype=torch.float64)
    assert float(((norm - brute).abs() / (brute + 1e-300)).max()) < 1e-14
    assert float(norm[:, 2].abs().max()) == 0.0 and float(bound[:, 2].max()) == R.TINY       # the all-zero row: exactly 0
    # a torch fp32 model of the kernel's order (8 lanes x 8 squares in order, butterfly 1, 2, 4) is inside the bound; inside the range the
    # bound is relative (12.1 2^-24 of the norm: 10 / 2 through the root, 2 for the root, rounding up of the two), below it absolute
    lanes = x.reshape(9, 3, 8, 8)
    acc = lanes[..., 0] * lanes[..., 0]
    for d in range(1, 8):
        acc = acc + lanes[..., d] * lanes[..., d]
    for d in (1, 2, 4):
        acc = acc + acc[..., [i ^ d for i in range(8)]]
    model = torch.sqrt(acc[..., 0]).t()
    assert R.worst(model, norm, bound)[0] < 1.0
    inside = [0, 1, 4, 5, 6, 7, 8]
    assert float((bound[:, inside] / norm[:, inside]).max()) < 12.1 * 2.0 ** -24
    assert float(bound[:, 3].max()) < 2.0 ** -59                                                # 2^-70 values: the absolute TINY terms alone
    # planted defects: a dropped lane, the sum instead of the root
    assert R.worst(torch.sqrt(acc[..., 0] - lanes[..., 7, 7] ** 2).t(), norm, bound)[0] > 1.0
    assert R.worst(acc[..., 0].t(), norm, bound)[0] > 1.0


# ---- distill_kl -------------------------------------------------------------------------------------------------------------------------
def test_distill_kl_against_python_floats_zero_rows_zero_entries_and_gradient():
    from emdr2_amd.model.emdr2_model import distill_kl
    g = torch.Generator().manual_seed(0)
    logits = torch.randn((5, 7), generator=g)
    logp = torch.log_softmax(logits, dim=1).requires_grad_(True)
    t = torch.rand((5, 7), generator=g)
    t[:, 2] = 0.0                                                           # zero entries
    t[0, 5] = 0.0
    t = t / t.sum(dim=1, keepdim=True)
    t[3] = 0.0                                                              # a question without a weighted position
    B = 11                                                                  # the batch-wide count: this group is 5 of 11 questions
    loss = distill_kl(logp, t, B)
    want, want_grad = WR.distill_kl_reference(logp.detach().double().tolist(), t.double().tolist(), B)
    # fp32: ln t and the subtraction (2 roundings on |ln t| + |logp|), the product, the sum of 35 terms (depth <= 35): 40 2^-24 of sum |terms|
    scale = sum(tv * (abs(math.log(tv)) + abs(lp)) for lr, tr in zip(logp.tolist(), t.tolist()) for lp, tv in zip(lr, tr) if tv > 0) / B
    assert abs(float(loss.detach()) - want) <= 40 * 2.0 ** -24 * scale, (float(loss.detach()), want)
    loss.backward()
    # the gradient is -t / B: one division (and torch's 1 / B reciprocal-multiply: two roundings) per element
    err = (logp.grad.double() - torch.tensor(want_grad, dtype=torch.float64)).abs()
    assert bool((err <= 2 * 2.0 ** -24 * t.double() / B).all())
    assert float(logp.grad[3].abs().max()) == 0.0 and float(logp.grad[:, 2].abs().max()) == 0.0    # exactly 0 where the target is 0
    # an all-zero target: exactly 0 loss and gradient; the target never receives a gradient
    logp2 = logp.detach().clone().requires_grad_(True)
    t0 = torch.zeros((5, 7), requires_grad=True)
    z = distill_kl(logp2, t0, B)
    z.backward()
    assert float(z.detach()) == 0.0 and float(logp2.grad.abs().max()) == 0.0 and t0.grad is None
    # the kl_div(..., reduction='sum') / batch form of the --ret-kldiv line
    ref = torch.nn.functional.kl_div(logp.detach(), t, reduction='sum') / B
    assert abs(float(ref) - float(loss.detach())) <= 40 * 2.0 ** -24 * scale
    # the groups of a step sum to the undivided step
    whole = distill_kl(logp.detach(), t, B)
    parts = distill_kl(logp.detach()[:2], t[:2], B) + distill_kl(logp.detach()[2:], t[2:], B)
    assert abs(float(whole) - float(parts)) <= 40 * 2.0 ** -24 * scale


def test_emdr2_loss_dispatches_on_the_read_target():
    from emdr2_amd.model.emdr2_model import ReadTarget, distill_kl
    t = torch.tensor([[0.5, 0.5, 0.0]])
    rt = ReadTarget(t.clone().requires_grad_(True))
    assert rt.shape == (1, 3) and not rt.mass.requires_grad
    logp = torch.log_softmax(torch.tensor([[1.0, 0.0, 2.0]]), dim=1)
    assert abs(float(distill_kl(logp, rt.mass, 1)) - (0.5 * (math.log(0.5) - float(logp[0, 0])) + 0.5 * (math.log(0.5) - float(logp[0, 1])))) < 1e-6


# ---- the flags --------------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_are_off_by_default():
    from emdr2_amd import arguments
    a = arguments.parse_args(BASE)
    assert a.retriever_distill_attention is False and a.attention_mass_value_norms is False
    a = arguments.parse_args(BASE + ["--retriever-distill-attention"])
    assert a.retriever_distill_attention is True and a.attention_mass_value_norms is False and a.reader_attention_mass is False
    a = arguments.parse_args(BASE + ["--retriever-distill-attention", "--attention-mass-value-norms"])
    assert a.retriever_distill_attention and a.attention_mass_value_norms
    a = arguments.parse_args(BASE + ["--reader-attention-mass", "--attention-mass-value-norms"])
    assert a.attention_mass_value_norms and not a.retriever_distill_attention
    assert arguments.parse_args(BASE + ["--reader-attention-mass", "--retriever-distill-attention"]).reader_attention_mass is True
    text = arguments.get_parser().format_help()
    assert "--retriever-distill-attention" in text and "--attention-mass-value-norms" in text


def test_refused_flag_combinations():
    from emdr2_amd import arguments
    no_update = [a for a in BASE if a != "--update-retriever"]
    with pytest.raises(ValueError, match="update-retriever"):
        arguments.parse_args(no_update + ["--retriever-distill-attention"])
    with pytest.raises(ValueError, match="ret-kldiv"):
        arguments.parse_args(BASE + ["--retriever-distill-attention", "--ret-kldiv"])
    with pytest.raises(ValueError, match="fp32-validation"):
        arguments.parse_args(BASE + ["--retriever-distill-attention", "--fp32-validation"])
    narrow = [a for a in BASE]
    narrow[narrow.index("--kv-channels") + 1] = "32"
    narrow[narrow.index("--num-attention-heads") + 1] = "24"
    with pytest.raises(ValueError, match="kv-channels 64"):
        arguments.parse_args(narrow + ["--retriever-distill-attention"])
    with pytest.raises(ValueError, match="attention-mass-value-norms"):
        arguments.parse_args(BASE + ["--attention-mass-value-norms"])


def test_the_model_build_refuses_the_same():
    from emdr2_amd.model.emdr2_model import EMDR2Model
    from emdr2_amd.model.transformer import Config
    kw = dict(topk=3, seq_length=64, seq_length_ret=32, cls_id=1, sep_id=2)
    for flags in (dict(retriever_distill_attention=True), dict(reader_attention_mass=True, attention_mass_value_norms=True)):
        with pytest.raises(ValueError, match="64 channels"):
            EMDR2Model(None, Config(hidden_size=128, num_attention_heads=4), 512, 512, **kw, **flags)
        with pytest.raises(ValueError, match="fp32"):
            EMDR2Model(None, Config(hidden_size=128, num_attention_heads=2, compute_dtype="fp32"), 512, 512, **kw, **flags)
    with pytest.raises(ValueError, match="attention_mass_value_norms"):
        EMDR2Model(None, Config(hidden_size=128, num_attention_heads=2), 512, 512, attention_mass_value_norms=True, **kw)
    with pytest.raises(ValueError, match="update_retriever"):
        EMDR2Model(None, Config(hidden_size=128, num_attention_heads=2), 512, 512, retriever_distill_attention=True, update_retriever=False, **kw)


# ---- the entry points' argument validation ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    return _native.lib()


MASS_ARGS = ("q", "q_sb", "q_ss", "q_sn", "k", "k_sb", "k_ss", "k_sn", "ids_q", "ids_k", "cu_k", "m", "l", "seg", "w", "kw", "kw_ld", "mass", "batch",
             "heads", "sq", "max_sk", "n_seg", "head_dim", "scale", "accumulate", "stream")


def _mass(lib, **over):
    one = ctypes.c_void_p(4096)
    a = dict(q=one, q_sb=2048, q_ss=64, q_sn=64, k=one, k_sb=4096, k_ss=64, k_sn=64, ids_q=one, ids_k=one, cu_k=None, m=one, l=one, seg=one,
             w=None, kw=one, kw_ld=64, mass=one, batch=1, heads=1, sq=32, max_sk=64, n_seg=2, head_dim=64, scale=0.125, accumulate=0, stream=None)
    a.update(over)
    return lib.emdr2_attention_key_mass_weighted(*[a[n] for n in MASS_ARGS])


def test_weighted_entry_validates_its_arguments_without_a_gpu(lib):
    for name in ("q", "k", "ids_q", "ids_k", "m", "l", "seg", "mass", "kw"):
        assert _mass(lib, **{name: None}) == -1, name
    for name in ("batch", "heads", "sq", "n_seg"):
        assert _mass(lib, **{name: 0}) == -1, name
    assert _mass(lib, q=ctypes.c_void_p(4096 + 8)) == -1 and _mass(lib, kw=ctypes.c_void_p(4096 + 2)) == -1
    assert _mass(lib, head_dim=32) == -4
    assert _mass(lib, sq=129) == -4
    assert _mass(lib, max_sk=65537, cu_k=ctypes.c_void_p(4096)) == -4
    assert _mass(lib, max_sk=48) == -4
    assert _mass(lib, k_ss=60) == -4
    assert _mass(lib, kw_ld=0) == -4
    assert _mass(lib, kw_ld=63) == -4                                         # dense keys: the table must hold batch * sk rows per head


def _norms(lib, **over):
    one = ctypes.c_void_p(4096)
    a = dict(x=one, x_sb=0, x_ss=128, x_sn=64, norm=one, ld=10, batch=1, sk=10, heads=2, head_dim=64, stream=None)
    a.update(over)
    return lib.emdr2_head_row_norms(*[a[n] for n in ("x", "x_sb", "x_ss", "x_sn", "norm", "ld", "batch", "sk", "heads", "head_dim", "stream")])


def test_norms_entry_validates_its_arguments_without_a_gpu(lib):
    for name in ("x", "norm"):
        assert _norms(lib, **{name: None}) == -1, name
    for name in ("batch", "sk", "heads"):
        assert _norms(lib, **{name: 0}) == -1, name
    assert _norms(lib, x=ctypes.c_void_p(4096 + 8)) == -1 and _norms(lib, norm=ctypes.c_void_p(4096 + 2)) == -1
    assert _norms(lib, head_dim=32) == -4 and _norms(lib, head_dim=128) == -4
    assert _norms(lib, x_ss=100) == -4
    assert _norms(lib, ld=9) == -4
    assert _norms(lib, batch=2, ld=19) == -4


def test_abi_version_is_unchanged(lib):
    assert lib.emdr2_abi_version() == 4


# ---- registers --------------------------------------------------------------------------------------------------------------------------
def test_both_mass_instances_and_the_norms_kernel_have_no_spills_and_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not (os.path.exists(kr.DEFAULT_LIB) and os.path.exists(os.path.join(kr.LLVM, "llvm-readelf"))):
        import __graft_entry__ as g
        g.build()
    table = kr.kernels()
    mass = [e for e in table if "attention_key_mass_kernel" in e["name"]]
    norms = [e for e in table if "head_row_norms_kernel" in e["name"]]
    assert len(mass) == 2 and any("Lb0E" in e["name"] for e in mass) and any("Lb1E" in e["name"] for e in mass), [e["name"] for e in mass]
    assert len(norms) == 1
    for e in mass + norms:
        print("[mass-weighted-cpu] %s: %d VGPRs + %d AGPRs, %d SGPRs" % (e["name"], e["vgpr_count"], e["agpr_count"], e["sgpr_count"]))
        assert e["vgpr_spill_count"] == 0 and e["sgpr_spill_count"] == 0 and e["private_segment_fixed_size"] == 0, e
    # four waves per SIMD, like the forward the kernel follows: at most 128 registers
    assert all(e["vgpr_count"] + e["agpr_count"] <= 128 for e in mass)
