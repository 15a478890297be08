"""GPU: the optimizer-state audit.  emdr2_state_audit against its numpy restatement (tests/state_audit_ref.py) bit for bit -- report, digests
and block keys -- at the sizes where its paths change (one short block, a block less one group, exactly one block, one group more, several
blocks with a short tail, more blocks than the capped grid has workgroups); single flipped bits; planted offenders; FlatAdam.audit() after
real training steps on the two-layer T5Model of tests/test_dist_gpu.py, after a checkpoint load, and on two data-parallel ranks of which
one then flips a bit; the checkpoint digest; the task flag."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import state_audit_ref as R
from tests.test_dist_gpu import _init

pytestmark = pytest.mark.gpu
GRID_CAP = 1024                                                          # workgroups of the pass (include/emdr2_ops.h)
SPECIAL = (0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0x7fc00001, 0xffa5a5a5)   # -0.0, denormals, +-Inf, NaNs


def _device_audit(master, m, v, work):
    """One call on uint32 / uint16 bit patterns -> (the 18 words as unsigned ints, the block keys as uint64)."""
    from emdr2_amd import _native
    lib = _native.lib()
    n = master.size
    dev = [torch.from_numpy(x.view(np.int32)).cuda() for x in (master, m, v)] + [torch.from_numpy(work.view(np.int16)).cuda()]
    keys = torch.zeros(3 * -(-n // 8192), dtype=torch.int64, device="cuda")
    report = torch.full((R.WORDS,), 0x5555, dtype=torch.int64, device="cuda")        # (the call sets every word itself)
    before = [x.clone() for x in dev]
    _native.check(lib.emdr2_state_audit(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), n, keys.data_ptr(),
                                        report.data_ptr(), _native.stream_ptr()), "state_audit")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(dev, before))           # it reads the bucket and writes nothing of it
    return [int(x) & R.NONE for x in report.tolist()], keys.cpu().numpy().view(np.uint64)


def _random_bits(n, seed):
    """Every bit pattern there is (a random word is a NaN or an Inf once in 256), the special values planted, a few working copies wrong."""
    rng = np.random.default_rng(seed)
    arrays = [rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    for a, x in enumerate(arrays):
        at = rng.choice(n, size=min(n, len(SPECIAL)), replace=False)
        x[at] = np.array(SPECIAL, np.uint32)[:at.size]
    work = R.f2bf(arrays[0])
    work[rng.choice(n, size=max(1, n // 1000), replace=False)] ^= np.uint16(1)
    return arrays + [work]


@pytest.mark.parametrize("n", [8, 8184, 8192, 8200, 3 * 8192 + 40, GRID_CAP * 8192 + 8200])
def test_report_digests_and_block_keys_equal_the_restatement(n):
    master, m, v, work = _random_bits(n, seed=n)
    words, keys = _device_audit(master, m, v, work)
    want_words, want_keys = R.report(master, m, v, work)
    print("n = %d: device words %s" % (n, words))
    assert np.array_equal(keys, want_keys)
    assert words == want_words
    if n >= 8192:
        assert all(words[1 + c] > 0 for c in range(5))                   # every check had something to count


def _sound(n, seed=1):
    rng = np.random.default_rng(seed)
    master = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 * 1e-6).astype(np.float32)
    master[:4], m[:4], v[:4] = 0.0, 0.0, 0.0
    bits = [x.view(np.uint32).copy() for x in (master, m, v)]
    return bits + [R.f2bf(bits[0])]


@pytest.fixture(scope="module")
def sound():
    n = 3 * 8192 + 40
    arrays = _sound(n)
    words, keys = _device_audit(*arrays)
    assert words[:11] == [n, 0, 0, 0, 0, 0] + [R.NONE] * 5 and words[17] == 4
    return n, arrays, words, keys


@pytest.mark.parametrize("a", [0, 1, 2])
def test_one_flipped_bit_changes_its_array_digest_and_exactly_its_block_key(sound, a):
    n, arrays, words0, keys0 = sound
    for index, bit in ((0, 0), (n - 1, 31), (8191, 13), (8192, 22), (2 * 8192 - 1, 7), (2 * 8192, 30)):      # ends, both sides of two seams
        changed = [x.copy() for x in arrays]
        changed[a][index] ^= np.uint32(1 << bit)
        if a == 0:
            changed[3] = R.f2bf(changed[0])
        words, keys = _device_audit(*changed)
        differs = np.flatnonzero(keys != keys0)
        assert differs.tolist() == [a * 4 + index // 8192], (index, bit)
        for b in range(3):
            same = words[11 + 2 * b:13 + 2 * b] == words0[11 + 2 * b:13 + 2 * b]
            assert same == (b != a), (index, bit, b)
        assert (words[11 + 2 * a] - words0[11 + 2 * a]) % (1 << 64) == (int(keys[differs[0]]) - int(keys0[differs[0]])) % (1 << 64)
        assert words[12 + 2 * a] ^ words0[12 + 2 * a] == int(keys[differs[0]]) ^ int(keys0[differs[0]])


PLANTS = {"nan_master": (0, 0, 0x7fc00000), "inf_exp_avg": (1, 1, 0xff800000), "negative_exp_avg_sq": (3, 2, 0xbf800000),
          "negative_denormal_exp_avg_sq": (3, 2, 0x80000001), "work_one_ulp_off": (4, 3, None)}


@pytest.mark.parametrize("what", sorted(PLANTS))
@pytest.mark.parametrize("at", [(5, 8192 + 3), (8191, 3 * 8192 + 39), (2 * 8192, 2 * 8192 + 1)])
def test_planted_offenders_are_counted_exactly_and_the_first_is_named(sound, what, at):
    n, arrays, words0, _ = sound
    check, array, value = PLANTS[what]
    x = [y.copy() for y in arrays]
    for i in at:
        if value is None:
            x[3][i] ^= np.uint16(1)                                      # one bf16 ulp off its master's rounding
        else:
            x[array][i] = value
    if array == 0:
        x[3] = R.f2bf(x[0])                                              # (the working copy follows: this case is about the master alone)
    words, _ = _device_audit(*x)
    counts, firsts = [0] * 5, [R.NONE] * 5
    counts[check], firsts[check] = 2, min(at)
    assert words[1:6] == counts and words[6:11] == firsts
    assert words[1:11] == R.report(*x)[0][1:11]


def test_negative_zero_in_the_second_moment_is_not_counted_but_minus_infinity_is_twice(sound):
    n, arrays, _, _ = sound
    x = [y.copy() for y in arrays]
    x[2][[7, 9000]] = 0x80000000
    assert _device_audit(*x)[0][1:11] == [0] * 5 + [R.NONE] * 5
    x[2][[100, 20000]] = 0xff800000                                      # -Inf: not finite AND below zero
    assert _device_audit(*x)[0][1:11] == [0, 0, 2, 2, 0, R.NONE, R.NONE, 100, 100, R.NONE]


# ---- FlatAdam.audit -------------------------------------------------------------------------------------------------------------------------
def _build(seed=0, **kw):
    from emdr2_amd.model import kernels as K
    from emdr2_amd.model.transformer import Config, T5Model
    from emdr2_amd.training import FlatAdam
    torch.manual_seed(seed)
    cfg = Config(num_layers=2, hidden_size=128, num_attention_heads=2, ffn_hidden_size=256, max_position_embeddings=128, init_method_std=0.05)
    m = T5Model(cfg, 512, checkpoint_activations=True).train()
    opt = K.GRAD_SINK = FlatAdam(m, lr=1e-3, bucket_bytes=1 << 20, **kw)
    K.DROPOUT.step = 0
    assert len(opt.buckets) > 1
    return m, opt


def _train(m, opt, rank=0, steps=3):
    rng = np.random.default_rng(100 + rank)
    for _ in range(steps):
        enc = torch.from_numpy(rng.integers(5, 512, size=(8, 64))).cuda(); dec = torch.from_numpy(rng.integers(5, 512, size=(8, 32))).cuda()
        opt.zero_grad()
        logits, _ = m(enc, dec)
        logits.float().square().mean().backward()
        opt.finish()
        opt.step()


@pytest.fixture()
def sink():
    from emdr2_amd.model import kernels as K
    yield K
    K.GRAD_SINK = None
    K.DROPOUT.step = 0


def test_after_real_training_steps_the_state_is_sound_and_so_after_a_checkpoint_load(sink):
    from emdr2_amd import checkpointing
    m, opt = _build()
    _train(m, opt)
    res = opt.audit()
    print({k: v for k, v in res.items() if k != "digests"})
    assert res["sound"] and res["world"] == 1 and res["buckets"] == len(opt.buckets) and res["elements"] == sum(b["n"] for b in opt.buckets)
    assert res["work_mismatch"] == 0                                     # the Adam kernel's working-copy write IS the cast kernel's rounding
    assert all(res[c] == 0 and res["first"][c] is None for c in R.CHECKS)
    assert torch.equal(opt.audit()["digests"], res["digests"])           # the same state: the same words
    for b, words in zip(opt.buckets, res["digests"].tolist()):           # ... and they are the restatement's, on a trained bucket
        want = [w for a, k in enumerate(("master", "m", "v")) for w in R.digest(R.block_keys(b[k].cpu().numpy().view(np.uint32), a))]
        assert [w & R.NONE for w in words] == want
    model_sd, opt_sd = checkpointing.t5_state_dict(m), opt.state_dict()
    assert "state_digest" not in opt_sd
    model_sd = {k: v for k, v in torch.load(_roundtrip(model_sd), weights_only=False).items()}
    m2, opt2 = _build(seed=5)
    assert not torch.equal(opt2.audit()["digests"], res["digests"])
    checkpointing.load_t5_state_dict(m2, model_sd)
    checkpointing._invalidate_weight_caches()                            # what every loader does: the working copies are stale now
    opt2.load_state_dict(opt_sd)
    res2 = opt2.audit()
    assert res2["sound"] and res2["work_mismatch"] == 0 and torch.equal(res2["digests"], res["digests"])
    # a working copy that is not its master's rounding, in the padding-free middle of a tensor
    name, p = max(m2.named_parameters(), key=lambda kv: kv[1].numel())
    b, o, n = opt2.slot[p]
    b["work"].view(torch.int16)[o + 77] ^= 1
    res3 = opt2.audit()
    assert not res3["sound"] and res3["work_mismatch"] == 1 and res3["first"]["work_mismatch"] == (name, 77)
    assert torch.equal(res3["digests"], res["digests"])                  # (the working copies are checked, not digested)


def _roundtrip(obj):
    import io
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return buf


def _rank(rank, world, port, out_dir):
    _init(rank, world, port, "gloo")
    from emdr2_amd.model import kernels as K
    m, opt = _build()
    _train(m, opt, rank=rank)                                            # different data per rank, the same averaged gradients
    res = opt.audit()
    first = {"sound": res["sound"], "world": res["world"], "digests": res["digests"]}
    name, p = max(m.named_parameters(), key=lambda kv: kv[1].numel())
    b, o, n = opt.slot[p]
    if rank == 1:
        b["master"].view(torch.int32)[o + 12345] ^= 1 << 2               # one mantissa bit of one master element, on one rank
    try:
        opt.audit()
        raised = None
    except RuntimeError as exc:
        raised = str(exc)
    torch.save({"first": first, "raised": raised, "victim": (name, 12345)}, os.path.join(out_dir, "r%d.pt" % rank))
    K.GRAD_SINK = None
    torch.distributed.destroy_process_group()


def test_two_ranks_are_identical_after_three_steps_and_both_name_the_bit_one_of_them_flips(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "r%d.pt" % r), weights_only=False) for r in (0, 1))
    for r in (r0, r1):
        assert r["first"]["sound"] and r["first"]["world"] == 2
    assert torch.equal(r0["first"]["digests"], r1["first"]["digests"])
    assert r0["raised"] is not None and r0["raised"] == r1["raised"]
    name, element = r0["victim"]
    assert "master of %s[%d] holds the bit patterns" % (name, element) in r0["raised"], r0["raised"]
    lo, hi = (int(x, 16) for x in re.search(r"0x([0-9a-f]{8}) and 0x([0-9a-f]{8})", r0["raised"]).groups())
    assert lo ^ hi == 1 << 2


# ---- the checkpoint ---------------------------------------------------------------------------------------------------------------------------
def _emdr2(audit_state, seed, bucket_bytes=64 << 10):
    from emdr2_amd.model.emdr2_model import EMDR2Model
    from emdr2_amd.model.transformer import Config
    from emdr2_amd.training import FlatAdam
    meta = np.load(os.path.join(os.path.dirname(__file__), "golden", "model_ref.npz"))["meta"]
    torch.manual_seed(seed)
    cfg = Config(num_layers=2, hidden_size=32, num_attention_heads=2, ffn_hidden_size=128, max_position_embeddings=64)
    model = EMDR2Model(None, cfg, int(meta[1]), int(meta[0]), 3, 48, 24, cls_id=2, sep_id=3)
    opt = FlatAdam(model, bucket_bytes=bucket_bytes, audit_state=audit_state)
    g = torch.Generator(device="cuda").manual_seed(seed)
    for b in opt.buckets:                                                # moments as a run would have left them
        for p in b["params"]:
            mm, vv = opt._moments(p)
            mm.copy_(torch.randn(p.shape, generator=g, device="cuda") * 1e-3)
            vv.copy_(torch.randn(p.shape, generator=g, device="cuda").square() * 1e-6)
    opt.step_count = 9
    return model, opt


def test_checkpoint_carries_the_digest_and_a_load_verifies_it(tmp_path, sink, capsys):
    from emdr2_amd import checkpointing
    d = str(tmp_path / "on")
    model, opt = _emdr2(True, 1)
    assert len(opt.buckets) > 1
    checkpointing.save_checkpoint(d, 5, model, opt)
    name = checkpointing.get_checkpoint_name(d, 5)
    saved = torch.load(name, map_location="cpu", weights_only=False)
    digest = saved["optimizer"]["state_digest"]
    assert digest["layout"] == [b["n"] for b in opt.buckets] and digest["words"] == opt.audit()["digests"].tolist()
    other, opt2 = _emdr2(True, 2)
    assert checkpointing.load_checkpoint(d, other, opt2) == 5 and opt2.step_count == 9
    assert opt2.audit()["sound"] and opt2.audit()["digests"].tolist() == digest["words"]
    # another bucket layout cannot be compared: one line, and the load goes through
    other3, opt3 = _emdr2(True, 3, bucket_bytes=256 << 10)
    capsys.readouterr()
    assert checkpointing.load_checkpoint(d, other3, opt3) == 5
    assert capsys.readouterr().out.count("optimizer state digest not verified") == 1
    # without the flag: no key, and a file with the key loads as before; a file without it loads into an auditing optimizer
    off, opt_off = _emdr2(False, 4)
    assert checkpointing.load_checkpoint(d, off, opt_off) == 5
    d_off = str(tmp_path / "off")
    checkpointing.save_checkpoint(d_off, 6, off, opt_off)
    plain = torch.load(checkpointing.get_checkpoint_name(d_off, 6), map_location="cpu", weights_only=False)
    assert set(plain["optimizer"]) == {"step", "state"}
    assert checkpointing.load_checkpoint(d_off, other, opt2) == 6
    # one exp_avg element altered in the file
    victim = max(saved["optimizer"]["state"], key=lambda i: saved["optimizer"]["state"][i]["exp_avg"].numel())
    saved["optimizer"]["state"][victim]["exp_avg"].view(-1)[11] += 1.0
    torch.save(saved, name)
    with pytest.raises(ValueError, match=r"the digest of exp_avg in bucket \d+ differs"):
        checkpointing.load_checkpoint(d, other, opt2)


# ---- the task -----------------------------------------------------------------------------------------------------------------------------------
def test_task_audits_before_the_first_step_and_at_every_second_iteration(tmp_path, capsys, sink):
    from emdr2_amd import checkpointing
    from emdr2_amd.tasks import run as task_run
    from tests.test_task_gpu import _argv, _make_world
    tmp = str(tmp_path)
    vocab, ev, emb = _make_world(tmp, n_valid=4)                         # 24 questions / batch 4: six steps
    model, _ = task_run.main(_argv(tmp, vocab, ev, emb, extra=("--audit-optimizer-state-interval", "2")))
    out = capsys.readouterr().out
    lines = re.findall(r"optimizer state audit at iteration (\d+): (\d+) elements in (\d+) buckets, sound, replicas identical \(world 1\) \(\S+ ms\)", out)
    assert [int(l[0]) for l in lines] == [0, 2, 4, 6], out[-3000:]
    assert len(set(l[1:] for l in lines)) == 1 and int(lines[0][1]) >= sum(p.numel() for p in model.parameters() if p.requires_grad)
    assert " iteration        6/" in out and "lm_loss" in out            # it trained on
    it, _ = checkpointing.read_tracker(os.path.join(tmp, "ckpt"))
    state = torch.load(checkpointing.get_checkpoint_name(os.path.join(tmp, "ckpt"), it), map_location="cpu", weights_only=False)
    assert "state_digest" in state["optimizer"] and len(state["optimizer"]["state_digest"]["layout"]) == int(lines[0][2])
