"""The region- and time-selected file writers of ace_amd/data_writer.py on the GPU: the fused path (``ace_diag_region_segments``)
against the torch path of the same module - bit for bit, since both follow the header's order in IEEE fp64 - each writer on CUDA
windows against its own CPU-path file, the launch count (one per window and side), the bytes that cross to the host (exactly the
kept record: names * B * n_kept * nlat_r * nlon_r * 4), and one ``run_evaluator`` on a small real stepper with a box entry, a
coarsened entry and a ``MonthSelector`` entry beside the default fan-out."""
import datetime
import os

import numpy as np
import pytest
import torch

from _util import load_golden
from ace_amd import data_writer as DW
from ace_amd.timeaxis import TimeAxis
from test_gpu_diag_kernels import dev  # noqa: F401

pytestmark = pytest.mark.gpu

B, T, H, W = 2, 8, 9, 20
COORDS = {"lat": np.linspace(-80.0, 80.0, H), "lon": np.arange(W) * 18.0}
NAMES = ["a", "b", "c"]


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def windows(n=3, b=B):
    """``n`` windows of T steps as strided views of wider records (as run_evaluator's targets), one name with a NaN patch"""
    g = torch.Generator().manual_seed(0)
    wide = {"a": torch.randn(b, n * T + 2, H, W, generator=g), "b": (1e5 + 900 * torch.randn(b, n * T + 2, H, W, generator=g)).float(),
            "c": 1e-3 * torch.randn(b, n * T + 2, H, W, generator=g)}
    wide["a"][:, :, 4, 5:9] = float("nan")
    time = TimeAxis.regular((2021, 5, 20, 0), datetime.timedelta(days=5), n * T + 2, n_samples=b)
    return wide, [(slice(1 + i * T, 1 + (i + 1) * T)) for i in range(n)], time


def test_fused_region_path_equals_torch_path(dev):
    wide, cuts, _ = windows(1)
    data = {n: x[:, cuts[0]] for n, x in wide.items()}
    cuda = {n: x.to(dev)[:, cuts[0]] for n, x in wide.items()}
    bounds = np.array([[[0, 1], [3, 3], [2, 8], [5, 7], [-4, 2], [6, 40]], [[7, 8], [0, 8], [4, 2], [1, 2], [1, 2], [0, 0]]])
    for region in ((2, 5, 4, 8), (2, 5, 5, 7), (8, 1, 19, 1), None):
        cpu, gpu = DW.SegmentReducer(region=region), DW.SegmentReducer(region=region)
        ref = cpu(data, ["b", "a", "c"], bounds=bounds)
        assert cpu.last_path == "torch"
        for _ in range(2):                                              # the second call reuses the tables and the staging
            got = gpu(cuda, ["b", "a", "c"], bounds=bounds)
            assert gpu.last_path == "fused"
            for k in ("sums", "means"):
                assert got[k].device.type == "cpu" and got[k].shape == ref[k].shape and torch.equal(bits(got[k]), bits(ref[k])), (region, k)
        h, w = (region[1], region[3]) if region else (H, W)
        assert gpu.launches == 2 and gpu.bytes_to_host == 2 * 3 * B * 6 * h * w * 12
        gpu.fused = False
        got = gpu(cuda, ["a"], bounds=bounds, want=("means",))           # the torch ops on the device
        assert gpu.last_path == "torch" and gpu.launches == 2 and torch.equal(bits(got["means"][0]), bits(ref["means"][1]))


CASES = {
    "box": (dict(lat_extent=(-45, 45), lon_extent=(72, 200)), 1),                                       # rows 2 .. 6, columns 4 .. 11
    "box_unaligned": (dict(names=["a", "c"], lat_extent=(-45, 45), lon_extent=(90, 200)), 1),           # columns 5 .. 11
    "box_coarse_sliced": (dict(lat_extent=(-45, 45), lon_extent=(72, 200), time_coarsen=DW.TimeCoarsenConfig(4),
                               time_selection=DW.Slice(1, 5)), 1),
    "strided": (dict(time_selection=DW.Slice(None, None, 3)), 2),
    "jja": (dict(names=["a", "b"], time_selection=DW.MonthSelector(["JJA"])), 1),
    "coarse": (dict(time_coarsen=DW.TimeCoarsenConfig(2)), 2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_file_writer_on_cuda_equals_the_cpu_path(dev, tmp_path, case):
    kwargs, b = CASES[case]
    wide, cuts, time = windows(3, b)
    files, writers = {}, {}
    for where in ("cpu", dev):
        w = DW.FileWriterConfig("out", **kwargs).build(str(tmp_path / str(where).replace(":", "")), coords=COORDS)
        for cut in cuts:
            w.append_batch({n: x.to(where)[:, cut] for n, x in wide.items()}, time=time[:, cut])
            assert w.reducer.last_path == ("torch" if where == "cpu" else "fused")
        w.finalize()
        writers[str(where)], files[str(where)] = w, torch.load(w.path, weights_only=True)
    (wc, wg), (dc, dg) = writers.values(), files.values()
    names = kwargs.get("names", NAMES)
    assert set(dc) == set(dg) == set(names) | {"time", "calendar", "lat", "lon"}
    for n in names:
        assert dg[n].dtype == torch.float32 and torch.equal(bits(dc[n]), bits(dg[n])), n
    for k in ("time", "lat", "lon"):
        assert torch.equal(dc[k], dg[k])
    n_kept, (h, w_) = dg["time"].shape[1], dg[names[0]].shape[2:]
    assert n_kept > 0 and dg[names[0]].shape == (b, n_kept, len(dg["lat"]), len(dg["lon"]))
    assert wg.reducer.launches == 3 and wc.reducer.launches == 0          # one per window
    assert wg.reducer.bytes_to_host == len(names) * b * n_kept * h * w_ * 4


def test_regional_monthly_writer_on_cuda_equals_the_cpu_path(dev, tmp_path):
    wide, cuts, time = windows(3)
    out = {}
    for where in ("cpu", dev):
        w = DW.FileWriterConfig("out", lat_extent=(-45, 45), lon_extent=(90, 200), time_coarsen=DW.MonthlyCoarsenConfig()
                                ).build(str(tmp_path / str(where).replace(":", "")), coords=COORDS)
        for cut in cuts:
            w.append_batch({n: x.to(where)[:, cut] for n, x in wide.items()}, time=time[:, cut])
        w.finalize()
        out[str(where)] = (w, torch.load(w.path, weights_only=True))
    (wc, dc), (wg, dg) = out.values()
    assert wg.reducer.last_path == "fused" and wg.reducer.launches == 3 and set(dc) == set(dg)
    assert torch.equal(dc["counts"], dg["counts"]) and int(dg["counts"].sum()) == B * 3 * T
    for n in NAMES:
        assert dg[n].shape == (B, dg["counts"].shape[1], 5, 7) and torch.equal(bits(dc[n]), bits(dg[n])), n
        assert torch.equal(bits(wc._monthly._totals[n]), bits(wg._monthly._totals[n])), n
    n_months = int(np.diff(wg._monthly._month_indices(time[:, 1:3 * T + 1])[:, [0, -1]]).max()) + 1
    assert wg.reducer.bytes_to_host <= 3 * len(NAMES) * B * n_months * 5 * 7 * 8


def test_paired_file_writer_launches_once_per_window_and_side(dev, tmp_path):
    wide, cuts, time = windows(2, 1)
    w = DW.FileWriterConfig("box", lat_extent=(-45, 45), lon_extent=(72, 200)).build_paired(str(tmp_path), coords=COORDS)
    for cut in cuts:
        w.append_batch(batch={n: x.to(dev)[:, cut] for n, x in wide.items()}, target={"a": wide["a"].to(dev)[:, cut]}, time=time[:, cut])
    w.finalize()
    assert w.prediction_writer.reducer.launches == 2 and w.reference_writer.reducer.launches == 2
    gen, tgt = torch.load(tmp_path / "box_predictions.pt", weights_only=True), torch.load(tmp_path / "box_target.pt", weights_only=True)
    assert set(tgt) == {"a", "time", "calendar", "lat", "lon"} and torch.equal(bits(gen["a"]), bits(tgt["a"]))
    assert torch.equal(bits(gen["a"]), bits(torch.cat([wide["a"][:, c] for c in cuts], dim=1)[:, :, 2:7, 4:12]))


def test_run_evaluator_with_file_entries_on_a_real_stepper(dev, tmp_path):
    import ace_amd
    from ace_amd.inference import EnginePredict, ForcingWindows, InferenceData, run_evaluator
    g = load_golden("gen_checkpoint.pt")["ace2_like"]
    loaded = ace_amd.load_stepper(g["state"], device=dev)
    ic = {k: v[:1].to(dev) for k, v in g["ic"].items()}                  # one initial condition: a MonthSelector takes no more
    total, Tm = 6, 2                                                      # three windows of two steps
    record = {n: torch.cat([x, x[:, 1:]], dim=1)[:1] for n, x in g["forcing"].items()}          # 7 time levels of 8 x 16
    record.update({n: x[:1].cpu().expand(-1, total + 1, -1, -1).contiguous() for n, x in g["ic"].items() if n not in record})
    time = TimeAxis.regular((2020, 1, 31, 0), datetime.timedelta(hours=6), total + 1, n_samples=1)
    coords = {"lat": np.linspace(-78.75, 78.75, 8), "lon": np.arange(16) * 22.5}

    class Agg:
        def record_initial_condition(self, initial_condition):
            return []

        def record_batch(self, prediction, target):
            return []

    box = dict(lat_extent=(-40, 40), lon_extent=(90, 250))               # rows 2 .. 5, columns 4 .. 11
    cfg = DW.DataWriterConfig(files=[
        DW.FileWriterConfig("box", **box),
        DW.FileWriterConfig("box_daily", time_coarsen=DW.TimeCoarsenConfig(2), time_selection=DW.Slice(1, None), **box),
        DW.FileWriterConfig("february", time_selection=DW.MonthSelector(["Feb"]), save_reference=False)])
    cfg.validate_time_coarsen(Tm, total)
    w = cfg.build_paired(str(tmp_path), coords=coords)
    run_evaluator(EnginePredict(loaded.stepper, batch=1, graph="step"),
                  InferenceData(ic, ForcingWindows(record, total_forward_steps=total, forward_steps_in_memory=Tm, device=dev, time=time)),
                  Agg(), writer=w)
    assert sorted(os.listdir(tmp_path)) == [
        "autoregressive_predictions.pt", "autoregressive_target.pt", "box_daily_predictions.pt", "box_daily_target.pt",
        "box_predictions.pt", "box_target.pt", "february.pt", "initial_condition.pt", "monthly_mean_predictions.pt",
        "monthly_mean_target.pt", "restart.pt"]
    load = lambda name: torch.load(tmp_path / name, weights_only=True)      # noqa: E731
    raw, raw_t, mon = load("autoregressive_predictions.pt"), load("autoregressive_target.pt"), load("monthly_mean_predictions.pt")
    names = set(raw)
    extra = {"time", "calendar", "lat", "lon"}
    for side, full in (("predictions", raw), ("target", raw_t)):
        got, daily = load(f"box_{side}.pt"), load(f"box_daily_{side}.pt")
        assert set(got) == set(full) | extra and set(daily) == set(full) | extra
        for n in full:
            assert torch.equal(bits(got[n]), bits(full[n].cpu()[:, :, 2:6, 4:12])), (side, n)
            assert daily[n].shape == (1, 2, 4, 8) and bool(torch.isfinite(daily[n]).all())
            # the block means of two steps, rounded once from the fp64 sum: within one fp32 rounding of torch's fp32 mean
            want = full[n].cpu()[:, 2:, 2:6, 4:12].unfold(1, 2, 2).mean(-1)
            torch.testing.assert_close(daily[n], want, rtol=2 ** -22, atol=2 ** -22 * float(want.abs().max()))
        assert np.array_equal(got["time"].numpy(), time.us[:, 1:]) and np.array_equal(got["lat"].numpy(), coords["lat"][2:6])
    feb = load("february.pt")
    assert set(feb) == names | extra and mon["counts"].tolist() == [[3, 3]]
    for n in names:
        assert torch.equal(bits(feb[n]), bits(raw[n].cpu()[:, 3:])), n       # 06, 12, 18 on 31 January, then February
    files = w._writers[2:]
    assert [f.prediction_writer.reducer.last_path for f in files] == ["fused"] * 3
    # one launch per window with something kept: the first window holds no coarsened step past the first, and no step of February
    assert [f.prediction_writer.reducer.launches for f in files] == [3, 2, 2]
    assert files[0].reference_writer.reducer.launches == 3 and files[2].reference_writer is None
    n_pred = len(names)
    assert files[0].prediction_writer.reducer.bytes_to_host == n_pred * 1 * total * 4 * 8 * 4
    assert files[1].prediction_writer.reducer.bytes_to_host == n_pred * 1 * 2 * 4 * 8 * 4
