"""GPU: stored index vectors by GLOBAL row.  emdr2_mips_gather_rows / HipIndexShard.rows_global: a row of this shard comes back bit for
bit, anything else -- -1, a row of another shard, the zero padding -- as zero bytes.  DistributedBruteForceIndex.reconstruct_rows: the same at any
world size through ONE integer all-reduce of the gathered buffer (two gloo ranks on one device, like tests/test_dist_gpu.py), which is what
FaissMIPSIndex.search_mips_index(..., reconstruct=True) over a sharded index returns its vectors through."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SHARD = 1300                                                           # three 512-row blocks of the image, the last one mostly padding
NEG_ZERO, INF, NAN = 0x8000, 0x7c00, 0x7e01


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _shard_matrix(dim):
    m = np.random.default_rng(dim).standard_normal((N_SHARD, dim)).astype(np.float16)
    b = m.view(np.uint16)
    b[0, 3], b[0, 5], b[0, dim - 1] = NEG_ZERO, INF, NAN                 # the first and the last row carry the special bit patterns
    b[N_SHARD - 1, 0], b[N_SHARD - 1, 9], b[N_SHARD - 1, dim - 2] = NAN, NEG_ZERO, INF | 0x8000
    b[700, :] = NEG_ZERO                                                 # a whole row of -0.0
    return m


@pytest.mark.parametrize("row_base", [0, 7000])
@pytest.mark.parametrize("dim", [64, 768])
def test_gather_by_global_row_against_the_host_matrix(dim, row_base):
    from emdr2_amd.data.emdr2_index import HipIndexShard
    m = _shard_matrix(dim)
    shard = HipIndexShard(dim, N_SHARD, row_base)
    shard.append_rows(m)
    outside = [-1, row_base - 1, row_base + N_SHARD, row_base + 1535]    # empty slot, the shard before, the shard after, the zero padding
    inside = [row_base, row_base + N_SHARD - 1, row_base + 700, row_base + 5, row_base + 5, row_base + 511, row_base + 512, row_base + 1024]
    extra = (row_base + np.random.default_rng(1).integers(0, N_SHARD, size=300)).tolist()
    rows = np.array(inside[:2] + outside + inside[2:] + extra + outside[::-1], dtype=np.int64)
    want = np.zeros((rows.size, dim), dtype=np.float16)
    ok = (rows >= row_base) & (rows < row_base + N_SHARD)
    assert int((~ok).sum()) == 8 and ok[:2].all()
    want[ok] = m[rows[ok] - row_base]
    got = shard.rows_global(torch.from_numpy(rows).cuda())
    assert got.dtype == torch.float16 and tuple(got.shape) == (rows.size, dim)
    got = got.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert not _bits(got[~ok]).any()                                     # zero BYTES, not -0.0
    assert _bits(got[0])[3] == NEG_ZERO and _bits(got[0])[5] == INF and _bits(got[0])[dim - 1] == NAN
    # any shape of row tensor, and into a caller's buffer whose old contents must not survive in the zero rows
    two_d = torch.from_numpy(rows[:12].reshape(3, 4)).cuda()
    out = torch.full((3, 4, dim), 7.0, dtype=torch.float16, device="cuda")
    assert shard.rows_global(two_d, out=out) is out
    assert np.array_equal(_bits(out.cpu().numpy().reshape(12, dim)), _bits(want[:12]))
    # the local-row entry is the same kernel: unchanged for rows of the shard
    assert np.array_equal(_bits(shard.rows(np.arange(N_SHARD)).cpu().numpy()), _bits(m))


def test_gather_entry_point_argument_checks_and_the_empty_list():
    from emdr2_amd import _native
    from emdr2_amd.data.emdr2_index import HipIndexShard
    lib = _native.lib()
    shard = HipIndexShard(64, N_SHARD, 0)
    shard.append_rows(_shard_matrix(64))
    ids = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = torch.full((4, 64), 3.0, dtype=torch.float16, device="cuda")
    t, sp = shard.tiled.data_ptr(), _native.stream_ptr()
    assert lib.emdr2_mips_gather_rows(t, N_SHARD, 64, 0, ids.data_ptr(), 0, out.data_ptr(), sp) == 0       # n_out == 0: a no-op
    torch.cuda.synchronize()
    assert float((out - 3.0).abs().max()) == 0.0
    assert lib.emdr2_mips_gather_rows(None, N_SHARD, 64, 0, ids.data_ptr(), 4, out.data_ptr(), sp) == -1
    assert lib.emdr2_mips_gather_rows(t, N_SHARD, 64, 0, None, 4, out.data_ptr(), sp) == -1
    assert lib.emdr2_mips_gather_rows(t, N_SHARD, 64, 0, ids.data_ptr(), 4, None, sp) == -1
    assert lib.emdr2_mips_gather_rows(t, N_SHARD, 100, 0, ids.data_ptr(), 4, out.data_ptr(), sp) == -1     # dim % 32
    assert lib.emdr2_mips_gather_rows(t, N_SHARD, 32, 0, ids.data_ptr(), 4, out.data_ptr(), sp) == -1      # dim < 64
    assert lib.emdr2_mips_gather_rows(t, N_SHARD, 64, -1, ids.data_ptr(), 4, out.data_ptr(), sp) == -1
    empty = shard.rows_global(torch.zeros((0,), dtype=torch.int64, device="cuda"))
    assert tuple(empty.shape) == (0, 64)
    with pytest.raises(ValueError):
        shard.rows_global(torch.zeros(4, dtype=torch.int32, device="cuda"))


def test_one_rank_reconstruct_gives_zero_vectors_in_empty_slots():
    """k larger than the index: the slots past the last row are (-inf, -1) and their vectors zero -- not row 0's"""
    from emdr2_amd.data.emdr2_index import FaissMIPSIndex
    rng = np.random.default_rng(3)
    rows, q = rng.standard_normal((3, 128)).astype(np.float16), rng.standard_normal((2, 128)).astype(np.float16)
    f = FaissMIPSIndex(128, None, use_gpu=True)
    f.add_with_ids(rows, np.array([11, 12, 13]))
    D, I, R = f.search_mips_index(torch.from_numpy(q), 5, reconstruct=True)
    assert (I[:, 3:] == -1).all() and np.isneginf(D[:, 3:]).all() and not R[:, 3:].view(np.uint32).any()
    assert np.array_equal(R[:, :3], rows[I[:, :3] - 11].astype(np.float32))


# -- two ranks ------------------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, backend="gloo"):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = rank if backend == "nccl" else 0
    torch.cuda.set_device(dev)
    extra = {"device_id": torch.device("cuda", dev)} if backend == "nccl" else {}
    torch.distributed.init_process_group(backend, rank=rank, world_size=world, **extra)
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex, FaissMIPSIndex
    from oracle import mips_oracle as mo
    rng = np.random.default_rng(0)
    n, d, nq = 30011, 128, 37
    rows = rng.standard_normal((n, d)).astype(np.float16)
    rows.view(np.uint16)[[100, 20000], :] = NEG_ZERO                     # a row of -0.0 on each rank's shard
    q = rng.standard_normal((nq, d)).astype(np.float16)
    ids = (rng.permutation(n) + 1).astype(np.int64)
    row_of = np.empty(n + 1, dtype=np.int64); row_of[ids] = np.arange(n)

    b = DistributedBruteForceIndex(d, None, use_gpu=True)
    b.add_arrays(ids.astype(np.int32), rows)
    lo, hi = b.local_rows()
    assert (lo, hi) == ((0, 15006) if rank == 0 else (15006, 30011))
    b.search_mips_index(torch.from_numpy(q).cuda(), 50)
    merged = b.last_search_rows
    mh = merged.cpu().numpy()
    assert tuple(mh.shape) == (nq, 50) and (mh < 15006).any() and (mh >= 15006).any()
    got = b.reconstruct_rows(merged)
    assert got.dtype == torch.float16 and tuple(got.shape) == (nq, 50, d)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(rows[mh]))
    # the planted rows (one of them on the OTHER rank's shard, whichever rank this is), the shard seam, and empty slots
    special = np.array([100, 20000, -1, 15005, 15006, 0, n - 1, -1], dtype=np.int64)
    got = b.reconstruct_rows(torch.from_numpy(special).cuda()).cpu().numpy()
    want = np.where((special >= 0)[:, None], rows[special.clip(0)], np.float16(0))
    assert np.array_equal(_bits(got), _bits(want)) and (_bits(got[:2]) == NEG_ZERO).all() and not _bits(got[2]).any()
    # this rank's slice of the leading dimension only
    mine = b.reconstruct_rows(merged[:36], scatter=True)
    assert tuple(mine.shape) == (18, 50, d) and np.array_equal(_bits(mine.cpu().numpy()), _bits(rows[mh[rank * 18:(rank + 1) * 18]]))
    try:
        b.reconstruct_rows(merged, scatter=True)                         # 37 rows over 2 ranks: refused before any collective, on every rank
        raise AssertionError("an uneven scatter was accepted")
    except ValueError:
        pass

    f = FaissMIPSIndex(d, None, use_gpu=True)
    f.add_with_ids(rows, ids)
    D, I, R = f.search_mips_index(torch.from_numpy(q), 5, reconstruct=True)
    od, oi = mo.topk_f32(rows, q, 5, ids=ids)
    assert np.array_equal(D.view(np.uint32), np.ascontiguousarray(od).view(np.uint32)) and np.array_equal(I, oi)
    assert R.dtype == np.float32 and np.array_equal(R.view(np.uint32), rows[row_of[oi]].astype(np.float32).view(np.uint32))

    tiny = FaissMIPSIndex(d, None, use_gpu=True)                         # 3 rows over 2 ranks, k = 5: two empty slots per query
    tiny.add_with_ids(rows[:3], ids[:3])
    D, I, R = tiny.search_mips_index(torch.from_numpy(q[:4]), 5, reconstruct=True)
    od, oi = mo.topk_f32(rows[:3], q[:4], 3, ids=ids[:3])
    assert np.array_equal(D[:, :3].view(np.uint32), np.ascontiguousarray(od).view(np.uint32)) and np.array_equal(I[:, :3], oi)
    assert (I[:, 3:] == -1).all() and not R[:, 3:].view(np.uint32).any()
    assert np.array_equal(R[:, :3].view(np.uint32), rows[row_of[oi]].astype(np.float32).view(np.uint32))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_reconstruct_the_merged_rows_bit_for_bit():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)


def _two_gpus():
    return torch.cuda.is_available() and torch.cuda.device_count() >= 2


@pytest.mark.skipif(not _two_gpus(), reason="needs two GPUs (RCCL)")
def test_two_ranks_reconstruct_over_rccl():
    """the same worker over RCCL: the int32 all-reduce and, for the slice, reduce_scatter_tensor"""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, "nccl"), nprocs=2, join=True)
