"""bench.py's N > 1 path on the DEVICE before a multi-GPU node runs it: two ranks under torch.distributed.run sharing this box's one
MI355X, collective backend gloo (RCCL refuses two ranks on one device; ACE_DIST_BACKEND=gloo, ace_amd/distributed.py).  Everything
but RCCL itself is the code of `bench.py --gpus 2`: one RolloutEngine per rank on device buffers, the two warm-up all-reduces and
the timed one through AsyncEnsembleMean's side stream and events, barrier / synchronise bracket, max over ranks, gather of the
per-rank records, ONE JSON line from rank 0."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_sharing_one_device():
    env = dict(os.environ, ACE_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 30500 + (os.getpid() % 1000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--precision", "f16x3",
           "--full"]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "weak" and d["value"] > 0
    mg = d["multi_gpu"]
    assert mg["world_size"] == 2 and [r["rank"] for r in mg["ranks"]] == [0, 1] and mg["allreduce_bytes"] == 50 * 180 * 360 * 4
    assert all(r["backend"] == "gloo" and r["allreduce_ms"] is not None and r["allreduce_ms"] > 0 for r in mg["ranks"])
    assert abs(d["value"] - 2 * 4 / (d["ms_per_step"] * 4e-3)) < 1e-2 * d["value"]      # whole-job aggregate over the slower rank's time
    assert d["cpu_baseline"] is None and d["roofline"] is not None                      # single-GPU legs skipped, rank 0's stage times kept


def test_plain_bench_line_is_the_headline_only(tmp_path):
    """`bench.py` without --full: the headline mode's K timed steps and its dumped outputs, none of the --full legs."""
    import numpy as np
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["unit"] == "steps/s"
    assert d["value"] > 0 and abs(d["value"] - 3 / (d["ms_per_step"] * 3e-3)) < 1e-2 * d["value"]
    assert d["config"]["precision"] == "f16x3" and d["dtype"].startswith("f32 (contractions")
    assert d["stages"] is None and d["roofline"] is None and d["roofline_sht"] is None and d["cpu_baseline"] is None
    assert not any(k.startswith("mode_") for k in d) and "one_year_rollout" not in d and "state_s80" not in d
    files = sorted(os.listdir(out))
    assert len(files) == 50 and "prog_0.npy" in files and "diag_13.npy" in files
    a = np.load(out / "prog_0.npy")
    assert a.dtype == np.float32 and a.shape == (1, 180, 360) and np.isfinite(a).all()
