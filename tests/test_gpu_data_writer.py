"""ace_amd/data_writer.py on the GPU: the fused path (``ace_diag_time_segments``) against the torch path of the same module - the fp64
sums and the fp32 means bit for bit, since both follow the header's order in IEEE fp64 - the writers on CUDA windows against their own
CPU-path files, the routing, and one ``run_evaluator`` with the default fan-out on a small real stepper."""
import datetime
import os

import numpy as np
import pytest
import torch

import _data_writer_cases as C
from _util import load_golden
from ace_amd import data_writer as DW
from ace_amd.timeaxis import TimeAxis
from test_gpu_diag_kernels import dev  # noqa: F401

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def test_fused_path_equals_torch_path(dev):
    g = torch.Generator().manual_seed(0)
    B, T, H, W = 3, 9, 7, 147                                           # 1029 pixels: more than one chunk, not a multiple of 4
    wide = {"a": torch.randn(B, T + 2, H, W, generator=g), "b": (1e5 + 900 * torch.randn(B, T + 2, H, W, generator=g)).float()}
    wide["a"][:, :, 2, 5:9] = float("nan")
    data = {n: x[:, 1:T + 1] for n, x in wide.items()}                   # strided views, as run_evaluator's targets
    edges = np.array([[0, 2, 2, 9], [1, 4, 3, 12], [-2, 0, 8, 9]])
    cpu = DW.SegmentReducer()
    ref = cpu(data, ["b", "a"], edges)
    assert cpu.last_path == "torch"
    gpu = DW.SegmentReducer()
    cuda = {n: x.to(dev)[:, 1:T + 1] for n, x in wide.items()}
    for _ in range(2):                                                  # the second call reuses the tables and the staging
        got = gpu(cuda, ["b", "a"], edges)
        assert gpu.last_path == "fused"
        for k in ("sums", "means"):
            assert got[k].device.type == "cpu" and got[k].shape == (2, B, 3, H, W) and torch.equal(bits(got[k]), bits(ref[k])), k
    assert gpu.launches == 2 and gpu.bytes_to_host == 2 * 2 * B * 3 * H * W * 12
    only = gpu(cuda, ["a"], edges, want=("sums",))
    assert only["means"] is None and torch.equal(bits(only["sums"][0]), bits(ref["sums"][1]))


def test_pick_fallbacks(dev):
    c = C.coarsen()["data"]
    red = DW.SegmentReducer()
    edges = np.array([[0, 5, 10]] * C.B)
    want = red(c, ["t"], edges)
    assert red.last_path == "torch"
    want = {k: v.clone() for k, v in want.items()}
    assert red.route([c["t"].to(dev)]) == "fused"
    assert red.route([c["t"].to(dev).double()]) == "torch" and red.route([c["t"].to(dev), c["pr"]]) == "torch"
    got = red({"t": c["t"].to(dev).double()}, ["t"], edges)               # fp64 on the device: the torch ops there
    assert red.last_path == "torch" and red.launches == 0 and torch.equal(bits(got["sums"]), bits(want["sums"]))
    red.fused = False
    got = red({"t": c["t"].to(dev)}, ["t"], edges)
    assert red.last_path == "torch" and red.launches == 0 and torch.equal(bits(got["means"]), bits(want["means"]))


class KeepTimed:
    uses_time = True

    def append_batch(self, batch, time=None):
        self.batch, self.time = batch, time


@pytest.mark.parametrize("f", C.FACTORS)
def test_time_coarsen_on_cuda_equals_the_cpu_path(dev, f):
    c = C.coarsen()
    a, b = KeepTimed(), KeepTimed()
    DW.TimeCoarsen(a, f).append_batch(c["data"], time=c["time"])
    tc = DW.TimeCoarsen(b, f)
    tc.append_batch({n: x.to(dev) for n, x in c["data"].items()}, time=c["time"])
    assert tc.reducer.last_path == "fused" and a.time == b.time
    for n in C.NAMES:
        assert b.batch[n].device.type == "cpu" and torch.equal(bits(a.batch[n]), bits(b.batch[n])), n


@pytest.mark.parametrize("key", list(C.MONTHLY))
def test_monthly_writer_on_cuda_equals_the_cpu_path(dev, tmp_path, key):
    c = C.monthly(key)
    files = {}
    for where in ("cpu", dev):
        w = DW.MonthlyDataWriter(str(tmp_path / str(where).replace(":", "")), "monthly_mean_predictions")
        for a, b in C.windows(c["n"], 40):
            w.append_batch({n: x.to(where)[:, a:b] for n, x in c["data"].items()}, time=c["time"][:, a:b])
        assert w.reducer.last_path == ("torch" if where == "cpu" else "fused")
        w.finalize()
        files[str(where)] = (w, torch.load(w.path, weights_only=True))
    (wc, dc), (wg, dg) = files.values()
    assert set(dc) == set(dg) and torch.equal(dc["counts"], dg["counts"]) and torch.equal(dc["valid_time"], dg["valid_time"])
    for n in C.NAMES:
        assert torch.equal(bits(wc._totals[n]), bits(wg._totals[n])) and torch.equal(bits(dc[n]), bits(dg[n])), n
    # 40 steps in, about two months out: the record that crosses to the host is the reduced one
    assert wg.reducer.bytes_to_host < sum(x.numel() * 4 for x in c["data"].values())


def test_run_evaluator_with_the_default_fan_out_on_a_real_stepper(dev, tmp_path):
    import ace_amd
    from ace_amd.inference import EnginePredict, ForcingWindows, InferenceData, run_evaluator
    g = load_golden("gen_checkpoint.pt")["ace2_like"]
    loaded = ace_amd.load_stepper(g["state"], device=dev)
    ic = {k: v.to(dev) for k, v in g["ic"].items()}
    total, T = 6, 2                                                       # three windows of two steps
    record = {n: torch.cat([x, x[:, 1:]], dim=1) for n, x in g["forcing"].items()}            # 7 time levels of 8 x 16
    record.update({n: x.cpu().expand(-1, total + 1, -1, -1).contiguous() for n, x in g["ic"].items() if n not in record})
    time = TimeAxis.regular((2020, 1, 31, 0), datetime.timedelta(hours=6), total + 1, n_samples=2)

    class Agg:
        def record_initial_condition(self, initial_condition):
            return []

        def record_batch(self, prediction, target):
            return []

    cfg = DW.DataWriterConfig(time_coarsen=DW.TimeCoarsenConfig(2))
    cfg.validate_time_coarsen(T, total)
    w = cfg.build_paired(str(tmp_path))
    run_evaluator(EnginePredict(loaded.stepper, batch=2, graph="step"),
                  InferenceData(ic, ForcingWindows(record, total_forward_steps=total, forward_steps_in_memory=T, device=dev, time=time)),
                  Agg(), writer=w)
    assert sorted(os.listdir(tmp_path)) == ["autoregressive_predictions.pt", "autoregressive_target.pt", "initial_condition.pt",
                                            "monthly_mean_predictions.pt", "monthly_mean_target.pt", "restart.pt"]
    raw = torch.load(tmp_path / "autoregressive_predictions.pt", weights_only=True)
    mon = torch.load(tmp_path / "monthly_mean_predictions.pt", weights_only=True)
    tgt = torch.load(tmp_path / "monthly_mean_target.pt", weights_only=True)
    names = set(raw)
    assert names >= set(g["steps"][0]) and set(mon) == names | {"counts", "time", "valid_time", "calendar"}
    for n in names:
        assert raw[n].shape == (2, total // 2, 8, 16) and mon[n].shape == (2, 2, 8, 16) and bool(torch.isfinite(raw[n]).all()), n
    assert mon["counts"].tolist() == [[3, 3], [3, 3]] and int(mon["counts"].sum()) == 2 * total
    assert torch.equal(tgt["counts"], mon["counts"]) and set(tgt) - {"counts", "time", "valid_time", "calendar"} <= names
    # the monthly mean of the block means is the monthly mean only where blocks do not straddle a month: here they do (3 + 3
    # steps in blocks of 2), so only the overall mean can be compared
    for n in names:
        torch.testing.assert_close(mon[n].mean(1), raw[n].mean(1), rtol=1e-5, atol=1e-5 * float(raw[n].abs().max()))
    assert w._writers[0].reducer.last_path == "fused" and w._writers[1]._prediction_writer.reducer.last_path == "fused"
