"""ace_amd/data_writer.py on its torch path: the configs and their errors, the coarsened values and time labels and the monthly file
against tests/golden/gen_data_writer.pt (the reference's own ``_coarsen_tensor_dict`` and ``add_data`` on the records of
tests/_data_writer_cases.py), the ``names`` filter, the fan-out of ``DataWriterConfig`` and the drivers of ace_amd/inference.py.

Bars as tests/test_timeseg_ref_cpu.py (u = 2^-24, m = max |x| over the steps of one output pixel): block means within
(f + 2) u m of the reference; monthly means within (N + 3 k + 1) u m of it for a month of N steps delivered in k windows and within
u |mean| of the exact mean; counts and valid_time exact; the fp64 totals bitwise independent of the cut (the records' fp64 sums are
exact)."""
import datetime
import os
import warnings

import numpy as np
import pytest
import torch

import _data_writer_cases as C
from ace_amd import data_writer as DW
from ace_amd.inference import ForcingWindows, InferenceData, TensorFileWriter, run_evaluator, run_inference
from ace_amd.timeaxis import TimeAxis
from test_inference_cpu import fake_predict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_data_writer.pt")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def within(got, ref, bar, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN pattern")
    err = np.nan_to_num(np.abs(got - ref))
    assert np.all(err <= bar), (what, float(np.max(err / np.maximum(bar, 1e-300))))


class Keep:
    """a writer of the old call shape"""

    def __init__(self):
        self.batches = []

    def append_batch(self, batch):
        self.batches.append(batch)


class KeepTimed(Keep):
    uses_time = True

    def __init__(self):
        super().__init__()
        self.times = []

    def append_batch(self, batch, time=None):
        self.batches.append(batch)
        self.times.append(time)


# ---- configs --------------------------------------------------------------------------------------------------------------
def test_time_coarsen_config():
    with pytest.raises(ValueError, match="coarsen_factor must be 1 or greater, got 0"):
        DW.TimeCoarsenConfig(0)
    cfg = DW.TimeCoarsenConfig(4)
    assert cfg.method == "block_mean" and cfg.n_coarsened_timesteps(10) == 2
    cfg.validate(8, 40)
    with pytest.raises(ValueError, match=r"forward_steps_in_memory must be divisible by time_coarsen.coarsen_factor. Got 6 and 4\."):
        cfg.validate(6, 40)
    with pytest.raises(ValueError, match=r"n_forward_steps must be divisible by time_coarsen.coarsen_factor. Got 42 and 4\."):
        cfg.validate(8, 42)
    assert isinstance(cfg.build(Keep()), DW.TimeCoarsen) and isinstance(cfg.build_paired(Keep()), DW.PairedTimeCoarsen)
    assert DW.MonthlyCoarsenConfig().method == "monthly_mean" and DW.MonthlyCoarsenConfig().validate(7, 13) is None


def test_data_writer_config_defaults_refusals_and_warning(tmp_path):
    cfg = DW.DataWriterConfig()
    assert (cfg.save_prediction_files, cfg.save_monthly_files, cfg.save_step_diagnostics, cfg.names, cfg.time_coarsen, cfg.files) == \
        (True, True, False, None, None, None)
    for bad in (DW.DataWriterConfig(save_step_diagnostics=True), DW.DataWriterConfig(files=[]), DW.DataWriterConfig(files=[object()])):
        for build in (bad.build, bad.build_paired):
            with pytest.raises(NotImplementedError):
                build(str(tmp_path))
    with pytest.warns(UserWarning, match="names provided but all options to save subsettable output files are False"):
        DW.DataWriterConfig(save_prediction_files=False, save_monthly_files=False, names=["t"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        DW.DataWriterConfig(save_prediction_files=False, save_monthly_files=False)
    DW.DataWriterConfig(time_coarsen=DW.TimeCoarsenConfig(2)).validate_time_coarsen(4, 8)
    with pytest.raises(ValueError, match="n_forward_steps must be divisible"):
        DW.DataWriterConfig(time_coarsen=DW.TimeCoarsenConfig(2)).validate_time_coarsen(4, 9)
    DW.DataWriterConfig().validate_time_coarsen(3, 7)


# ---- segment_sums ---------------------------------------------------------------------------------------------------------
def test_segment_sums_torch_path_is_the_statement():
    import _timeseg_ref as R
    data = C.coarsen()["data"]
    edges = np.array([[-3, 2, 2, 1, 7, 12], [0, 10, 4, 4, 5, 5]])
    red = DW.SegmentReducer()
    out = red(data, list(C.NAMES), edges)
    assert red.last_path == "torch" and red.launches == 0
    sums, means = np.zeros((3, C.B, 5, C.H * C.W)), np.zeros((3, C.B, 5, C.H * C.W), np.float32)
    R.time_segments([data[n].numpy().reshape(C.B, 10, -1) for n in C.NAMES], [0, 1, 2], 3, edges, sums=sums, means=means)
    assert out["sums"].dtype == torch.float64 and out["means"].dtype == torch.float32 and out["sums"].shape == (3, C.B, 5, C.H, C.W)
    assert np.array_equal(out["sums"].numpy().reshape(sums.shape), sums, equal_nan=True)
    assert np.array_equal(out["means"].numpy().reshape(means.shape), means, equal_nan=True)
    # a strided view is taken as it is
    wide = {n: torch.cat([x, x], dim=1) for n, x in data.items()}
    view = {n: x[:, 3:13] for n, x in wide.items()}
    again = DW.segment_sums(view, list(C.NAMES), np.array([[7, 10], [0, 7]]), want=("sums",))
    assert again["means"] is None
    assert np.array_equal(again["sums"][0, 0, 0].numpy(), data["t"][0, :3].double().sum(0).numpy())
    with pytest.raises(ValueError, match="want"):
        red(data, ["t"], edges, want=("median",))
    with pytest.raises(ValueError, match="edges"):
        red(data, ["t"], edges[:1])


# ---- time coarsening ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", C.FACTORS)
def test_time_coarsen_values_and_labels(golden, f):
    c = C.coarsen()
    inner = KeepTimed()
    DW.TimeCoarsen(inner, f).append_batch(c["data"], time=c["time"])
    (got,), (time,) = inner.batches, inner.times
    assert set(got) == set(C.NAMES)
    for n in C.NAMES:
        assert got[n].dtype == torch.float32 and got[n].device.type == "cpu" and got[n].shape == (C.B, 10 // f, C.H, C.W)
        m = np.abs(np.nan_to_num(c["data"][n].double().numpy())).reshape(C.B, 10 // f, f, C.H, C.W).max(axis=2)
        within(got[n], golden["coarsen"]["ref"][f][n], (f + 2) * U * m, (f, n, "reference"))
        exact = golden["coarsen"]["exact"][f][n].numpy()
        within(got[n], exact, U * np.abs(np.nan_to_num(exact)), (f, n, "exact"))
    us = c["time"].us.reshape(C.B, 10 // f, f)
    want = np.array([[sum(int(v) for v in blk) // f for blk in row] for row in us])           # python integers: no overflow, floor
    assert time.calendar == c["time"].calendar and np.array_equal(time.us, want)
    if f == 1:
        assert all(torch.equal(got[n].view(torch.int32), c["data"][n].view(torch.int32)) for n in C.NAMES)


def test_time_coarsen_hands_down_tensors_the_writer_owns(tmp_path):
    c = C.coarsen()
    raw = TensorFileWriter(str(tmp_path))
    tc = DW.TimeCoarsen(raw, 5)
    other = {n: x + 1 for n, x in c["data"].items()}
    tc.append_batch(c["data"], time=c["time"])                # TensorFileWriter takes no time: the old call shape
    tc.append_batch(other)
    tc.flush()
    out = torch.load(os.path.join(tmp_path, "autoregressive_predictions.pt"), weights_only=True)
    assert out["t"].shape == (C.B, 4, C.H, C.W)
    a, b = KeepTimed(), KeepTimed()
    DW.TimeCoarsen(a, 5).append_batch(c["data"])
    DW.TimeCoarsen(b, 5).append_batch(other)
    assert torch.equal(out["t"][:, :2], a.batches[0]["t"]) and torch.equal(out["t"][:, 2:], b.batches[0]["t"])
    assert a.times == [None]
    with pytest.raises(ValueError, match="not a multiple of coarsen_factor 4"):
        DW.TimeCoarsen(Keep(), 4).append_batch(c["data"])


def test_paired_time_coarsen():
    c = C.coarsen()

    class Pair:
        paired = True

        def append_batch(self, batch, target):
            self.got = (batch, target)

    inner = Pair()
    tc = DW.PairedTimeCoarsen(inner, 2)
    assert tc.paired and tc.uses_time and not tc.needs_time
    target = {"t": torch.cat([c["data"]["t"], c["data"]["t"]], dim=1)[:, 1:11]}             # a strided view, as run_evaluator's
    tc.append_batch(batch=c["data"], target=target, time=c["time"])
    single = KeepTimed()
    DW.TimeCoarsen(single, 2).append_batch(target)
    assert set(inner.got[0]) == set(C.NAMES) and torch.equal(inner.got[1]["t"], single.batches[0]["t"])


# ---- monthly --------------------------------------------------------------------------------------------------------------
def run_monthly(tmp_path, key, cut, names=None, flush_after=None, sub=""):
    c = C.monthly(key)
    w = DW.MonthlyDataWriter(os.path.join(tmp_path, sub), "monthly_mean_predictions", names=names)
    for i, (a, b) in enumerate(C.windows(c["n"], cut)):
        w.append_batch({n: x[:, a:b] for n, x in c["data"].items()}, time=c["time"][:, a:b])
        if flush_after is not None and i == flush_after:
            w.flush()
    w.finalize()
    return w, torch.load(w.path, weights_only=True)


@pytest.mark.parametrize("key", list(C.MONTHLY))
@pytest.mark.parametrize("cut", C.CUTS)
def test_monthly_file_against_the_reference(tmp_path, golden, key, cut):
    g = golden["monthly"][key]
    w, ds = run_monthly(str(tmp_path), key, cut)
    assert w.path.endswith("monthly_mean_predictions.pt") and not os.path.exists(w.path + ".tmp")
    n_months = g["counts"].shape[1]
    assert set(ds) == set(C.NAMES) | {"counts", "time", "valid_time", "calendar"}
    assert ds["counts"].dtype == torch.int64 and torch.equal(ds["counts"], g["counts"]) and torch.equal(ds["counts"], g["ref"][cut]["counts"])
    assert torch.equal(ds["time"], torch.arange(n_months))
    assert ds["valid_time"].dtype == torch.int64 and torch.equal(ds["valid_time"], g["valid_time"])
    assert ds["calendar"] == C.MONTHLY[key]["calendar"]
    for n in C.NAMES:
        assert ds[n].dtype == torch.float32 and ds[n].shape == (C.B, n_months, C.H, C.W)
        exact = g["exact"][n].numpy()
        within(ds[n], exact, U * np.abs(np.nan_to_num(exact)), (n, "exact"))
        bar = (g["counts"].numpy() + 3 * g["windows"][cut].numpy() + 1)[:, :, None, None] * U * g["absmax"][n].numpy()
        within(ds[n], g["ref"][cut][n], bar, (n, "reference"))
    if key == "sixhourly":
        assert ds["counts"][1, 3] == 0 and bool((ds["t"][1, 3] == 0).all())          # a month without steps stays 0, as the reference's


@pytest.mark.parametrize("key", list(C.MONTHLY))
def test_monthly_result_does_not_depend_on_the_windows(tmp_path, key):
    runs = [run_monthly(str(tmp_path), key, cut, sub=str(cut)) for cut in C.CUTS]
    runs.append(run_monthly(str(tmp_path), key, 7, flush_after=1, sub="flushed"))          # a flush mid-run, then more windows
    w0, ds0 = runs[0]
    for w, ds in runs[1:]:
        assert np.array_equal(w._counts, w0._counts)
        for n in C.NAMES:
            assert torch.equal(w._totals[n].view(torch.int64), w0._totals[n].view(torch.int64)), (n, "fp64 totals, bitwise")
            assert torch.equal(ds[n].view(torch.int32), ds0[n].view(torch.int32))
        assert torch.equal(ds["valid_time"], ds0["valid_time"])


def test_monthly_flush_mid_run_writes_what_there_is(tmp_path):
    c = C.monthly("fivedaily")
    w = DW.MonthlyDataWriter(str(tmp_path), "monthly_mean_target")
    w.flush()
    assert not os.path.exists(w.path)
    w.append_batch({"t": c["data"]["t"][:, :7]}, time=c["time"][:, :7])
    w.flush()
    ds = torch.load(w.path, weights_only=True)
    assert int(ds["counts"].sum()) == 7 * C.B and w.path.endswith("monthly_mean_target.pt")


def test_monthly_names_filter_and_size_checks(tmp_path):
    with pytest.warns(UserWarning, match=r"Requested variable\(s\) not present in data: \['absent'\]"):
        _, ds = run_monthly(str(tmp_path), "fivedaily", 40, names=["t", "absent"])
    assert set(ds) == {"t", "counts", "time", "valid_time", "calendar"}
    c = C.monthly("fivedaily")
    w = DW.MonthlyDataWriter(str(tmp_path), "x")
    with pytest.raises(ValueError, match="Batch size mismatch, data has 2 samples and batch_time has 1 samples."):
        w.append_batch(c["data"], time=c["time"][:1])
    with pytest.raises(ValueError, match="Batch time dimension mismatch, data has 30 times and batch_time has 29 times."):
        w.append_batch(c["data"], time=c["time"][:, :29])
    with pytest.raises(ValueError, match="needs the windows' time axis"):
        w.append_batch(c["data"])


def test_paired_monthly_writes_both_files(tmp_path):
    c = C.monthly("fivedaily")
    w = DW.PairedMonthlyDataWriter(str(tmp_path))
    assert w.paired and w.needs_time
    w.append_batch(batch=c["data"], target={"t": c["data"]["t"] + 1}, time=c["time"])
    w.finalize()
    gen = torch.load(os.path.join(tmp_path, "monthly_mean_predictions.pt"), weights_only=True)
    tgt = torch.load(os.path.join(tmp_path, "monthly_mean_target.pt"), weights_only=True)
    assert set(tgt) == {"t", "counts", "time", "valid_time", "calendar"} and set(gen) >= set(C.NAMES)
    assert torch.equal(tgt["counts"], gen["counts"])
    torch.testing.assert_close(tgt["t"][:, 0], gen["t"][:, 0] + 1)


# ---- the fan-out and the drivers ------------------------------------------------------------------------------------------
def record(n_steps=8, B=1):
    """forcing, initial condition and a 6-hourly axis from 2020-01-31T06: the month changes after the third step"""
    g = torch.Generator().manual_seed(3)
    f = torch.randn(B, n_steps + 1, 2, 2, generator=g)
    time = TimeAxis.regular((2020, 1, 31, 0), datetime.timedelta(hours=6), n_steps + 1, n_samples=B)
    return f, {"x": torch.zeros(B, 1, 2, 2)}, time


def paired_predict(ic, win, compute_derived_variables=False):
    return fake_predict(ic, win)


def test_data_writer_config_fan_out_through_run_inference(tmp_path):
    f, ic, time = record()
    one, _ = fake_predict(ic, {"f": f})
    w = DW.DataWriterConfig(time_coarsen=DW.TimeCoarsenConfig(2)).build(str(tmp_path))
    assert isinstance(w, DW.DataWriter) and w.uses_time and w.needs_time and not getattr(w, "paired", False)
    state = run_inference(fake_predict, InferenceData(ic, ForcingWindows({"f": f}, 8, 4, device="cpu", time=time)), writer=w)
    assert sorted(os.listdir(tmp_path)) == ["autoregressive_predictions.pt", "initial_condition.pt", "monthly_mean_predictions.pt",
                                            "restart.pt"]
    raw = torch.load(os.path.join(tmp_path, "autoregressive_predictions.pt"), weights_only=True)
    assert raw["x"].shape == (1, 4, 2, 2)
    torch.testing.assert_close(raw["x"], one["x"].unfold(1, 2, 2).mean(-1))
    mon = torch.load(os.path.join(tmp_path, "monthly_mean_predictions.pt"), weights_only=True)
    assert mon["counts"].tolist() == [[3, 5]]                                # 06, 12, 18 on 31 January, then five steps of February
    torch.testing.assert_close(mon["d"][:, 0], one["d"][:, :3].mean(1))
    assert torch.equal(torch.load(os.path.join(tmp_path, "restart.pt"), weights_only=True)["x"], state["x"])


@pytest.mark.parametrize("kwargs, files", [
    (dict(save_monthly_files=False), ["autoregressive_predictions.pt"]),
    (dict(save_prediction_files=False), ["monthly_mean_predictions.pt"]),
    (dict(save_prediction_files=False, save_monthly_files=False), []),
    (dict(names=["d"]), ["autoregressive_predictions.pt", "monthly_mean_predictions.pt"])])
def test_data_writer_config_sub_writers(tmp_path, kwargs, files):
    f, ic, time = record()
    w = DW.DataWriterConfig(**kwargs).build(str(tmp_path))
    run_inference(fake_predict, InferenceData(ic, ForcingWindows({"f": f}, 8, 3, device="cpu", time=time)), writer=w)
    assert sorted(os.listdir(tmp_path)) == sorted(files + ["initial_condition.pt", "restart.pt"])          # restart.pt always
    if "names" in kwargs:
        for name in files:
            ds = torch.load(os.path.join(tmp_path, name), weights_only=True)
            assert {k for k in ds if k in ("x", "d")} == {"d"}


def test_a_writer_that_needs_time_on_a_loader_without(tmp_path):
    f, ic, _ = record()
    with pytest.raises(ValueError, match="needs the windows' time axis: build the ForcingWindows with time="):
        run_inference(fake_predict, InferenceData(ic, ForcingWindows({"f": f}, 8, 4, device="cpu")),
                      writer=DW.DataWriterConfig().build(str(tmp_path)))
    # without the monthly writer nothing needs it: the coarsened raw file is written as ever
    w = DW.DataWriterConfig(save_monthly_files=False, time_coarsen=DW.TimeCoarsenConfig(4)).build(str(tmp_path / "raw"))
    run_inference(fake_predict, InferenceData(ic, ForcingWindows({"f": f}, 8, 4, device="cpu")), writer=w)
    assert torch.load(os.path.join(tmp_path, "raw", "autoregressive_predictions.pt"), weights_only=True)["x"].shape == (1, 2, 2, 2)


def test_drivers_keep_the_old_call_shape_and_pass_time_where_asked(tmp_path):
    f, ic, time = record()
    seen = []

    class Old(TensorFileWriter):
        def append_batch(self, batch):                      # no time, no target: exactly the call of before
            seen.append(sorted(batch))
            super().append_batch(batch)

    class Agg:
        def record_initial_condition(self, initial_condition):
            return []

        def record_batch(self, prediction, target):
            return []

    loader = lambda with_time: ForcingWindows({"f": f, "x": torch.zeros(1, 9, 2, 2)}, 8, 4, device="cpu",      # noqa: E731
                                              time=time if with_time else None)
    for with_time in (False, True):
        run_inference(fake_predict, InferenceData(ic, loader(with_time)), writer=Old(str(tmp_path / "a")))
        run_evaluator(paired_predict, InferenceData(ic, loader(with_time)), Agg(), writer=Old(str(tmp_path / "b")))
    assert seen == [["d", "x"]] * 8
    timed = KeepTimed()
    timed.write = lambda data, filename: None
    run_inference(fake_predict, InferenceData(ic, loader(True)), writer=timed)
    assert [t.shape for t in timed.times] == [(1, 4), (1, 4)] and np.array_equal(timed.times[1].us, time.us[:, 5:9])
    timed = KeepTimed()
    timed.write = lambda data, filename: None
    run_inference(fake_predict, InferenceData(ic, loader(False)), writer=timed)
    assert timed.times == [None, None]


def test_run_evaluator_with_the_paired_fan_out(tmp_path):
    f, ic, time = record()
    tgt = torch.arange(9, dtype=torch.float32).reshape(1, 9, 1, 1).expand(1, 9, 2, 2).contiguous()

    class Agg:
        def record_initial_condition(self, initial_condition):
            return []

        def record_batch(self, prediction, target):
            return []

    w = DW.DataWriterConfig(time_coarsen=DW.TimeCoarsenConfig(2)).build_paired(str(tmp_path))
    assert isinstance(w, DW.PairedDataWriter) and w.paired
    run_evaluator(paired_predict, InferenceData(ic, ForcingWindows({"f": f, "x": tgt}, 8, 4, device="cpu", time=time)), Agg(), writer=w)
    assert sorted(os.listdir(tmp_path)) == ["autoregressive_predictions.pt", "autoregressive_target.pt", "initial_condition.pt",
                                            "monthly_mean_predictions.pt", "monthly_mean_target.pt", "restart.pt"]
    raw = torch.load(os.path.join(tmp_path, "autoregressive_target.pt"), weights_only=True)
    assert set(raw) == {"x"} and torch.equal(raw["x"][0, :, 0, 0], torch.tensor([1.5, 3.5, 5.5, 7.5]))
    mon = torch.load(os.path.join(tmp_path, "monthly_mean_target.pt"), weights_only=True)
    assert mon["counts"].tolist() == [[3, 5]] and torch.equal(mon["x"][0, :, 0, 0], torch.tensor([2.0, 6.0]))
    assert set(torch.load(os.path.join(tmp_path, "monthly_mean_predictions.pt"), weights_only=True)) >= {"x", "d"}
