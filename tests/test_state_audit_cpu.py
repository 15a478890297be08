"""No GPU: the optimizer-state audit (--audit-optimizer-state-interval).  The entry points' argument checks, the flag and its rules, the
numpy restatement of the digest (tests/state_audit_ref.py; the GPU tests compare the device with it) on the properties the header claims,
the locate logic on synthetic MIN / MAX words over a host-built slot table, and the replica comparison itself on two gloo ranks."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import state_audit_ref as R
from tests.test_step_guard_cpu import BASE, _host_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_bound_and_validate_their_arguments():
    from emdr2_amd import _native
    lib = _native.lib()
    al, off8, off4 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8), ctypes.c_void_p(4096 + 4)
    assert lib.emdr2_abi_version() == 4                                  # new entry points do not move it
    good = [al, al, al, al, 8192, al, al, None]
    for i in (0, 1, 2, 3, 5, 6):                                         # a null pointer in every place
        args = list(good)
        args[i] = None
        assert lib.emdr2_state_audit(*args) == -1
    for n in (0, 4, 12, 8191, -8):                                       # n % 8 != 0, nothing to audit
        assert lib.emdr2_state_audit(al, al, al, al, n, al, al, None) == -1
    for i in (0, 1, 2):                                                  # fp32 arrays: 16 bytes
        args = list(good)
        args[i] = off8
        assert lib.emdr2_state_audit(*args) == -1
    for i in (3, 5, 6):                                                  # working copies, keys, report: 8 bytes
        args = list(good)
        args[i] = off4
        assert lib.emdr2_state_audit(*args) == -1
    size = ctypes.c_size_t()
    for n in (8, 8184, 8192, 8200, 3 * 8192 + 40, 440388096):
        assert lib.emdr2_state_audit_ws_bytes(n, ctypes.byref(size)) == 0
        assert size.value == 3 * -(-n // 8192) * 8
    assert lib.emdr2_state_audit_ws_bytes(12, ctypes.byref(size)) == -1 and lib.emdr2_state_audit_ws_bytes(8, None) == -1


def test_flag_and_its_rules():
    from emdr2_amd import arguments
    assert arguments.parse_args(BASE).audit_optimizer_state_interval == 0                 # off by default
    assert arguments.parse_args(BASE + ["--audit-optimizer-state-interval", "50"]).audit_optimizer_state_interval == 50
    with pytest.raises(ValueError, match="audit-optimizer-state-interval"):
        arguments.parse_args(BASE + ["--audit-optimizer-state-interval", "-1"])
    with pytest.raises(ValueError, match="fp32-validation"):
        arguments.parse_args(BASE + ["--audit-optimizer-state-interval", "2", "--fp32-validation"])


def _arrays(n, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32) for _ in range(3)]


def test_reference_digest_sees_positions_blocks_and_arrays():
    n = 2 * 8192 + 40
    master, m, v = _arrays(n)
    keys = lambda: [R.block_keys(x, a) for a, x in enumerate((master, m, v))]
    base = keys()
    assert [k.size for k in base] == [3, 3, 3]
    assert all(np.array_equal(a, b) for a, b in zip(base, keys()))       # nothing swapped: nothing changes
    # two pairs of one block exchanged: that block's key changes, and with it the digest; the multiset of values does not
    swapped = master.copy()
    swapped[[10, 11, 20, 21]] = master[[20, 21, 10, 11]]
    k = R.block_keys(swapped, 0)
    assert k[0] != base[0][0] and np.array_equal(k[1:], base[0][1:]) and R.digest(k) != R.digest(base[0])
    # the two halves of one pair exchanged
    flipped = master.copy()
    flipped[[10, 11]] = master[[11, 10]]
    assert master[10] != master[11] and R.block_keys(flipped, 0)[0] != base[0][0]
    # two whole blocks exchanged
    moved = master.copy()
    moved[:8192], moved[8192:16384] = master[8192:16384], master[:8192]
    assert R.digest(R.block_keys(moved, 0)) != R.digest(base[0])
    # a value moved from master to exp_avg: the same bits hash differently under another tag
    assert not np.array_equal(R.block_keys(master, 0), R.block_keys(master, 1))
    a2, b2 = master.copy(), m.copy()
    a2[5], b2[5] = m[5], master[5]
    assert R.digest(R.block_keys(a2, 0)) != R.digest(base[0]) and R.digest(R.block_keys(b2, 1)) != R.digest(base[1])
    # -0.0 is not +0.0, and two NaN payloads are two values
    z = np.zeros(8, np.uint32)
    for bits in (0x80000000, 0x7fc00001):
        y = z.copy()
        y[3] = bits
        assert R.digest(R.block_keys(y, 0)) != R.digest(R.block_keys(z, 0))
    y2 = z.copy()
    y2[3] = 0x7fc00002
    assert R.digest(R.block_keys(y2, 0)) != R.digest(R.block_keys(y, 0))


def test_reference_f2bf_and_checks():
    f = np.array([1.0, -0.0, 1.00390625, 1.01171875, np.inf, 3.4028235e38], np.float32)      # ties go to the even neighbour; overflow rounds to Inf
    assert R.f2bf(f.view(np.uint32)).tolist() == [0x3f80, 0x8000, 0x3f80, 0x3f82, 0x7f80, 0x7f80]
    assert R.f2bf(np.array([0x7f800001, 0xffc12345], np.uint32)).tolist() == [0x7fc0, 0xffc1]   # NaN: quiet, payload top bits kept
    same = torch.tensor([1.0, 0.3, -2.7e-5, 65504.1, 1e-40]).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.f2bf(np.array([1.0, 0.3, -2.7e-5, 65504.1, 1e-40], np.float32).view(np.uint32)), same)
    master = np.linspace(-1, 1, 16, dtype=np.float32)
    m, v = np.zeros(16, np.float32), np.full(16, 0.5, np.float32)
    work = R.f2bf(master.view(np.uint32))
    bits = lambda x: x.view(np.uint32)
    assert R.checks(bits(master), bits(m), bits(v), work) == [(0, R.NONE)] * 5
    master[9] = np.nan; m[4] = -np.inf; m[12] = np.inf
    v[2] = -0.0; v[6] = -1e-42; v[7] = -np.inf; v[11] = np.nan; bits(v)[13] = 0xffc00000       # -0.0 and NaNs are not "below zero"
    work[1] ^= 1
    assert R.checks(bits(master), bits(m), bits(v), work) == [(1, 9), (2, 4), (3, 7), (2, 6), (2, 1)]      # (work[9] no longer rounds master[9])


def test_locate_on_synthetic_minimum_and_maximum_words():
    from emdr2_amd import training as T
    mod, opt = _host_optimizer()
    B = len(opt.buckets)
    assert B >= 3
    lo = torch.arange(B * T.AUDIT_WORDS, dtype=torch.int64).reshape(B, T.AUDIT_WORDS)
    assert T.first_digest_difference(lo, lo.clone()) is None
    hi = lo.clone()
    hi[1, 5] += 1                                                        # a count differs: not a digest word
    assert T.first_digest_difference(lo, hi) is None
    hi[2, 16] += 1; hi[1, 14] -= 9                                       # xor word of exp_avg in bucket 1 comes first
    assert T.first_digest_difference(lo, hi) == (1, 1)
    hi[1, 11] = -1
    assert T.first_digest_difference(lo, hi) == (1, 0)
    assert T.first_difference(torch.tensor([3, -1, 7]), torch.tensor([3, -1, 7])) is None
    assert T.first_difference(torch.tensor([3, -1, 7]), torch.tensor([3, 5, 9])) == 1
    named = dict(mod.named_parameters())
    for name, p in named.items():
        b, o, n = opt.slot[p]
        assert opt.locate_element(b["idx"], o + n - 1) == (name, n - 1)
    b, o, n = opt.slot[named["b1"]]                                      # 61 elements in a slice of 64
    assert opt.locate_element(b["idx"], o + 62) == (None, o + 62)
    msg = T.replica_mismatch_message("exp_avg", 1, "w2", 17, 0x3f800000, 0x3f800001)
    assert "exp_avg of w2[17]" in msg and "0x3f800000 and 0x3f800001" in msg
    assert "element 62 of bucket 1 (padding" in T.replica_mismatch_message("master", 1, None, 62, 0, 1)
    # the words of an audit, by hand: bucket 1 reports two bad masters from element o + 3 on, the worst replica one more
    words = torch.zeros((3, B, T.AUDIT_WORDS), dtype=torch.int64)
    words[:, :, 6:11] = -1
    words[:, :, 0] = torch.tensor([bk["n"] for bk in opt.buckets])
    b, o, n = opt.slot[named["w2"]]
    words[0, b["idx"], 1], words[0, b["idx"], 6] = 2, o + 3
    words[2, b["idx"], 1], words[2, b["idx"], 6] = 3, o + 3
    words[2, B - 1, 5], words[2, B - 1, 10] = 1, 0
    res = opt.audit_from_words(words)
    assert res["elements"] == sum(bk["n"] for bk in opt.buckets) and res["buckets"] == B
    assert res["nonfinite_master"] == 2 and res["first"]["nonfinite_master"] == ("w2", 3) and res["first"]["work_mismatch"] is None
    assert res["worst"]["nonfinite_master"] == 3 and res["worst"]["work_mismatch"] == 1 and not res["sound"]
    assert res["worst_first"]["work_mismatch"] == (opt.names[opt.buckets[B - 1]["params"][0]], 0)
    assert res["digests"].shape == (B, 6)


def test_audit_on_host_tensors_raises_like_step():
    from emdr2_amd import _native
    mod, opt = _host_optimizer()
    assert opt.audit_state is False and "state_digest" not in opt.state_dict()
    with pytest.raises(_native.NativeError):
        opt.audit()


def _gloo_rank(rank, port, out_dir, differ):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    from emdr2_amd import training as T
    torch.distributed.init_process_group("gloo", rank=rank, world_size=2)
    B, n = 3, 2 * 8192 + 40
    state = [[np.random.default_rng(10 * b + a).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32) for a in range(3)] for b in range(B)]
    if differ and rank == 1:
        state[1][2][8192 + 77] ^= 1 << 3                                 # one bit of exp_avg_sq, bucket 1, block 1
    report = torch.zeros((B, T.AUDIT_WORDS), dtype=torch.int64)
    keys = {}
    for b in range(B):
        words, k = R.report(state[b][0], state[b][1], state[b][2], R.f2bf(state[b][0]))
        report[b] = torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64))
        keys[b] = torch.from_numpy(k.view(np.int64).copy())
    calls = []

    def block_keys(b, a):
        calls.append(("keys", b, a))
        return keys[b][a * 3:(a + 1) * 3]

    def block_bits(b, a, j):
        calls.append(("bits", b, a, j))
        return torch.from_numpy(state[b][a][j * 8192:(j + 1) * 8192].astype(np.int64))
    try:
        words = T.compare_state_replicas(report, None, block_keys, block_bits, lambda b, i: ("p%d" % b, i - 8000))
        result = ("returned", bool(torch.equal(words[0], report) and torch.equal(words[1], words[2])))
    except RuntimeError as exc:
        result = ("raised", str(exc))
    torch.save((result, calls, int(state[1][2][8192 + 77])), os.path.join(out_dir, "r%d.pt" % rank))
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("differ", [False, True])
def test_two_gloo_ranks_compare_their_digests(tmp_path, differ):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_gloo_rank, args=(r, port, str(tmp_path), differ)) for r in (0, 1)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    hung = [p.is_alive() for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert not any(hung) and [p.exitcode for p in procs] == [0, 0]      # neither rank hangs in a collective its peer never joins
    (r0, c0, v0), (r1, c1, v1) = (torch.load(os.path.join(str(tmp_path), "r%d.pt" % r), weights_only=False) for r in (0, 1))
    if not differ:
        assert r0 == r1 == ("returned", True) and c0 == c1 == []         # level 1 alone: no further collective
        return
    assert r0[0] == r1[0] == "raised" and r0[1] == r1[1]                 # the identical message on both ranks
    assert c0 == c1 == [("keys", 1, 2), ("bits", 1, 2, 1)]
    lo, hi = sorted((v0, v1))
    assert "exp_avg_sq of p1[%d]" % (8192 + 77 - 8000) in r0[1] and "0x%08x and 0x%08x" % (lo, hi) in r0[1]
