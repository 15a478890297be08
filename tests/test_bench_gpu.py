"""GPU: the plain `python bench.py` run -- headline only, everything else behind --full -- and --dump-outputs, whose arrays must be what the
timed operator returned in its last step: bit-identical to the CPU oracle over the same seeded rows and queries."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import mips_oracle as mo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_prints_the_headline_and_dumps_the_last_step_bit_identical_to_the_oracle(tmp_path):
    n, nq, k = 200_000, 256, 50                                          # > 128 queries: the benchmark's persistent filter scan
    out_dir = tmp_path / "out"
    env = dict(os.environ)
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(key, None)
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", str(n), "--queries", str(nq), "--topk", str(k),
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    r = json.loads(lines[0])
    assert r["metric"] == "mips_queries_per_sec" and r["unit"] == "queries/s" and r["higher_is_better"] is True and r["dtype"] == "f16"
    assert r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert abs(r["value"] - nq * 1e3 / r["ms_per_step"]) <= 1e-9 * r["value"]
    assert not {"roofline", "roofline_hbm_regime", "cpu_baseline", "clustered", "e2e", "e2e_k100"} & set(r), sorted(r)     # --full only

    scores, ids = np.load(str(out_dir / "scores.npy")), np.load(str(out_dir / "doc_ids.npy"))
    assert scores.dtype == np.float32 and ids.dtype == np.float64 and scores.shape == ids.shape == (nq, k)
    # the same inputs, regenerated here: bench.synth_rows and the benchmark's query generator; doc ids are rows + 1
    sys.path.insert(0, ROOT)
    import bench
    rows = torch.cat([block.clone() for block in bench.synth_rows(0, n)]).cpu().numpy()
    gq = torch.Generator(device="cuda").manual_seed(4321)
    queries = torch.randn((nq, bench.DIM), generator=gq, device="cuda", dtype=torch.float32).to(torch.float16).cpu().numpy()
    od, oi = mo.topk(rows, queries, k, ids=np.arange(1, n + 1, dtype=np.int32))
    assert np.array_equal(scores.astype(np.float16).view(np.uint16), od.view(np.uint16))
    assert np.array_equal(ids.astype(np.int32), oi)
