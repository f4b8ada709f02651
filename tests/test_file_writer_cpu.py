"""The region- and time-selected file writers of ace_amd/data_writer.py on their torch path: the selection logic against
tests/golden/gen_file_writer.pt (the reference's own ``Slice.shift_left``, ``_month_string_to_int`` and ``_get_time_mask``, and
``pandas.Index.slice_indexer`` for the extents), the region statement of ``SegmentReducer`` against tests/_region_ref.py, and the
writers through ``run_inference`` / ``run_evaluator``: file names, keys, shapes, ``time`` / ``lat`` / ``lon`` contents, a regional
coarsened and sliced file against the slice of the existing ``TimeCoarsen`` file and a regional monthly file against the slice of
the existing monthly file (both bit for bit: the same fp64 sums in the same order, rounded once), the paired files, the cap on the
empty-window warning, and every refusal."""
import datetime
import logging
import os

import numpy as np
import pytest
import torch

import _region_ref as RR
from ace_amd import data_writer as DW
from ace_amd.inference import ForcingWindows, InferenceData, run_evaluator, run_inference
from ace_amd.timeaxis import TimeAxis
from test_inference_cpu import fake_predict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_file_writer.pt")
H, W = 6, 12
COORDS = {"lat": np.arange(-75.0, 90.0, 30.0), "lon": np.arange(15.0, 360.0, 30.0)}
BOX = dict(lat_extent=(-50, 50), lon_extent=(40, 200))                   # rows 1 .. 4 (-45 .. 45), columns 1 .. 6 (45 .. 195)
ROWS, COLS = slice(1, 5), slice(1, 7)


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def record(n_steps=12, B=1, start=(2020, 1, 29, 0), step=datetime.timedelta(hours=6)):
    g = torch.Generator().manual_seed(5)
    f = torch.randn(B, n_steps + 1, H, W, generator=g)
    time = TimeAxis.regular(start, step, n_steps + 1, n_samples=B)
    return f, {"x": torch.zeros(B, 1, H, W)}, time


def paired_predict(ic, win, compute_derived_variables=False):
    return fake_predict(ic, win)


class Agg:
    def record_initial_condition(self, initial_condition):
        return []

    def record_batch(self, prediction, target):
        return []


def infer(tmp_path, cfg, n_steps=12, in_memory=4, B=1, coords=COORDS, with_time=True, **rec):
    f, ic, time = record(n_steps, B, **rec)
    w = cfg.build(str(tmp_path), coords=coords)
    run_inference(fake_predict, InferenceData(ic, ForcingWindows({"f": f}, n_steps, in_memory, device="cpu",
                                                                 time=time if with_time else None)), writer=w)
    return w, time


def load(tmp_path, name):
    return torch.load(os.path.join(tmp_path, name), weights_only=True)


# ---- the selection logic against the reference's ---------------------------------------------------------------------------
def test_slice_shift_left_against_the_reference(golden):
    assert len(golden["slice"]) > 1000
    for (start, stop, step, n_seen, T), want in golden["slice"].items():
        try:
            got = list(range(T)[DW.Slice.shift_left(DW.Slice(start, stop, step), n_seen).slice])
        except ValueError as e:
            got = "ValueError"
            assert "Negative slice bounds as an initial value are not supported" in str(e)
        assert got == want, (start, stop, step, n_seen, T)
    s = DW.Slice(2, 9, 3)
    assert s.slice == slice(2, 9, 3) and s.contains(5) and not s.contains(4) and not s.contains(11) and DW.Slice().contains(10**9)
    assert DW.Slice.shift_left(DW.Slice(0, 10, 1), 5) == DW.Slice(None, 5, 1)
    # a step > 1 starts anew at a window whose start lies past ``start``: steps 0, 3, 6, 9 of 12 in windows of 4 keep 0, 3 | 4, 7 | 8, 11
    kept = [n + k for n in (0, 4, 8) for k in range(4)[DW.Slice.shift_left(DW.Slice(0, None, 3), n).slice]]
    assert kept == [0, 3, 4, 7, 8, 11]


def test_month_names_against_the_reference(golden):
    for name, want in golden["month_string"].items():
        if want == "ValueError":
            with pytest.raises(ValueError, match="Invalid month string"):
                DW._month_string_to_int(name)
        else:
            assert DW._month_string_to_int(name) == want, name
    assert sum(1 for v in golden["month_string"].values() if v != "ValueError") >= 24


def test_month_and_season_masks_against_the_reference(golden):
    month = np.array(golden["mask"]["month"])
    for sel, want in golden["mask"]["masks"]:
        assert DW.MonthSelector(sel).mask(month).tolist() == want, sel
    assert DW.MonthSelector([]).mask(month).all()                         # file_writer.py:116-117: no months, no selection
    with pytest.raises(ValueError, match="Invalid month string: Juno"):
        DW.MonthSelector(["Juno"]).mask(month)


def test_extents_against_pandas(golden):
    coords = golden["extent"]["coords"]
    assert len(golden["extent"]["cases"]) >= 100
    for key, lo, hi, want in golden["extent"]["cases"]:
        start, stop = DW.extent_indices(coords[key], lo, hi)
        assert list(range(start, max(stop, start))) == want, (key, lo, hi)
    assert DW.extent_indices(np.arange(-89.5, 90.0), -10, 10.5) == (80, 101)          # rows 80 .. 100
    with pytest.raises(ValueError, match="monotonic"):
        DW.extent_indices([0.0, 2.0, 1.0], 0, 1)


# ---- the region statement on the torch path --------------------------------------------------------------------------------
def test_segment_reducer_region_and_bounds_are_the_statement():
    g = torch.Generator().manual_seed(0)
    data = {"a": torch.randn(2, 11, H, W, generator=g), "b": (1e5 + 900 * torch.randn(2, 11, H, W, generator=g)).float()}
    data["a"][0, 3, 2, 4] = float("nan")
    bounds = np.array([[[0, 1], [4, 4], [3, 9], [5, 7], [-4, 2], [9, 40], [8, 2]]] * 2)
    region = (1, 4, 2, 7)
    red = DW.SegmentReducer(region=region)
    out = red(data, ["b", "a"], bounds=bounds)
    assert red.last_path == "torch" and red.launches == 0 and red.bytes_to_host == 0
    sums, means = np.zeros((2, 2, 7, 4, 7)), np.zeros((2, 2, 7, 4, 7), np.float32)
    RR.region_segments([data["b"].numpy(), data["a"].numpy()], [0, 1], 2, bounds, region, sums=sums, means=means)
    assert out["sums"].dtype == torch.float64 and out["means"].dtype == torch.float32 and out["sums"].shape == sums.shape
    assert np.array_equal(out["sums"].numpy(), sums, equal_nan=True) and np.array_equal(out["means"].numpy(), means, equal_nan=True)
    # edges on a region: the touching segments; bounds without a region: the whole plane; both equal today's path, cut
    edges = np.array([[0, 2, 2, 11], [1, 4, 3, 12]])
    whole = DW.SegmentReducer()(data, ["a", "b"], edges)
    cut = red(data, ["a", "b"], edges)
    full = DW.segment_sums(data, ["a", "b"], bounds=RR.bounds_of_edges(edges), reducer=DW.SegmentReducer())
    for k in ("sums", "means"):
        assert torch.equal(bits(cut[k]), bits(whole[k][..., 1:5, 2:9])) and torch.equal(bits(full[k]), bits(whole[k])), k
    assert red(data, ["a"], bounds=np.zeros((2, 0, 2), int))["means"].shape == (1, 2, 0, 4, 7)
    for bad, match in ((dict(bounds=bounds[:1]), "bounds must be"), (dict(edges=edges, bounds=bounds), "exactly one"), ({}, "exactly one")):
        with pytest.raises(ValueError, match=match):
            red(data, ["a"], **bad)
    with pytest.raises(ValueError, match="does not lie in a 6 x 12 plane"):
        DW.SegmentReducer(region=(3, 4, 0, 12))(data, ["a"], edges)
    with pytest.raises(ValueError, match="lat0, nlat_r, lon0, nlon_r"):
        DW.SegmentReducer(region=(1, 2, 3))


# ---- the config ------------------------------------------------------------------------------------------------------------
def test_file_writer_config_defaults_and_checks():
    cfg = DW.FileWriterConfig("box")
    assert (cfg.names, cfg.lat_extent, cfg.lon_extent, cfg.time_selection, cfg.save_reference, cfg.time_coarsen,
            cfg.separate_ensemble_members) == (None, None, None, None, True, None, False)
    assert isinstance(cfg.format, DW.NetCDFWriterConfig) and (cfg.format.name, cfg.format.suffix) == ("netcdf", "nc")
    assert cfg.filenames == ["box.pt", "box_target.pt", "box_predictions.pt"]
    assert (DW.Slice().start, DW.Slice().stop, DW.Slice().step) == (None, None, None)
    with pytest.raises(ValueError, match=r"lat_extent must be a tuple of \(min_lat, max_lat\)"):
        DW.FileWriterConfig("box", lat_extent=(1, 2, 3))
    with pytest.raises(ValueError, match=r"lon_extent must be a tuple of \(min_lon, max_lon\)"):
        DW.FileWriterConfig("box", lon_extent=(1,))
    with pytest.raises(NotImplementedError, match="Time selection is not currently supported when using monthly coarsening"):
        DW.FileWriterConfig("box", time_selection=DW.Slice(0, 4), time_coarsen=DW.MonthlyCoarsenConfig())
    with pytest.raises(NotImplementedError, match="Time selection is not currently supported when writing to zarr"):
        DW.FileWriterConfig("box", time_selection=DW.Slice(0, 4), format=DW.ZarrWriterConfig())
    with pytest.raises(NotImplementedError, match="Monthly coarsening is not currently supported for the zarr format"):
        DW.FileWriterConfig("box", time_coarsen=DW.MonthlyCoarsenConfig(), format=DW.ZarrWriterConfig())
    cfg = DW.FileWriterConfig("box", time_coarsen=DW.TimeCoarsenConfig(4))
    cfg.validate_time_coarsen(8, 40)
    with pytest.raises(ValueError, match="forward_steps_in_memory must be divisible"):
        cfg.validate_time_coarsen(6, 40)
    DW.FileWriterConfig("box", time_coarsen=DW.MonthlyCoarsenConfig()).validate_time_coarsen(7, 13)
    DW.FileWriterConfig("box").validate_time_coarsen(7, 13)


def test_build_time_refusals(tmp_path):
    d = str(tmp_path)
    for cfg, match in ((DW.FileWriterConfig("a", time_selection=DW.TimeSlice("2020-01", "2020-02")), "TimeSlice"),
                       (DW.FileWriterConfig("a", format=DW.ZarrWriterConfig()), "zarr"),
                       (DW.FileWriterConfig("a", separate_ensemble_members=True), "separate ensemble members")):
        for build in (cfg.build, cfg.build_paired):
            with pytest.raises(NotImplementedError, match=match):
                build(d, coords=COORDS)
    for cfg in (DW.FileWriterConfig("a", lat_extent=(-50, 50)), DW.FileWriterConfig("a", lon_extent=(0, 50))):
        for coords in (None, {"face": np.arange(12), "height": np.arange(4), "width": np.arange(4)}):          # HEALPix
            with pytest.raises(ValueError, match="Coordinates must include 'lat' and 'lon' if using lat/lon extents"):
                cfg.build(d, coords=coords)
    for extent in (dict(lat_extent=(50, -50)), dict(lat_extent=(-50, 50), lon_extent=(200, 40)), dict(lat_extent=(-40, -20)),
                   dict(lon_extent=(350, 400))):
        with pytest.raises(ValueError, match="the region of 'a' is empty"):
            DW.FileWriterConfig("a", **extent).build(d, coords=COORDS)
    north_first = {"lat": COORDS["lat"][::-1].copy(), "lon": COORDS["lon"]}
    w = DW.FileWriterConfig("a", lat_extent=(50, -50)).build(d, coords=north_first)                          # the coordinate's order
    assert w._region == (1, 4, 0, 12)
    with pytest.raises(ValueError, match="the region of 'a' is empty"):
        DW.FileWriterConfig("a", lat_extent=(-50, 50)).build(d, coords=north_first)
    with pytest.raises(ValueError, match="Unsupported time selection type"):
        DW.FileWriterConfig("a", time_selection=slice(0, 4)).build(d)


def test_data_writer_config_with_files(tmp_path):
    a, b = DW.FileWriterConfig("a", time_coarsen=DW.TimeCoarsenConfig(3)), DW.FileWriterConfig("b")
    cfg = DW.DataWriterConfig(files=[a, b])
    cfg.validate_time_coarsen(6, 12)
    with pytest.raises(ValueError, match="n_forward_steps must be divisible by time_coarsen.coarsen_factor. Got 13 and 3"):
        cfg.validate_time_coarsen(6, 13)
    for files in ([a, DW.FileWriterConfig("a")], [b, DW.FileWriterConfig("b_target")]):
        with pytest.raises(ValueError, match="Duplicate filenames found in file writer configurations"):
            DW.DataWriterConfig(files=files)
    w = cfg.build(str(tmp_path))                                         # no extent: no coords needed, one positional argument
    assert [type(x) for x in w._writers] == [DW._RawSubset, DW.MonthlyDataWriter, DW.FileWriter, DW.FileWriter] and w.needs_time
    p = DW.DataWriterConfig(save_monthly_files=False, files=[b]).build_paired(str(tmp_path))
    assert isinstance(p._writers[-1], DW.PairedFileWriter) and p.paired and not p.needs_time
    assert DW.DataWriterConfig(save_monthly_files=False, files=[DW.FileWriterConfig("m", time_selection=DW.MonthSelector(["JJA"]))]
                               ).build(str(tmp_path)).needs_time
    with pytest.raises(ValueError, match="Coordinates must include"):
        DW.DataWriterConfig(files=[DW.FileWriterConfig("c", **BOX)]).build(str(tmp_path))
    with pytest.raises(NotImplementedError):
        DW.DataWriterConfig(files=[b, object()]).build(str(tmp_path))


# ---- the writers through the drivers ---------------------------------------------------------------------------------------
def test_a_box_file_through_run_inference(tmp_path):
    cfg = DW.DataWriterConfig(save_monthly_files=False, files=[DW.FileWriterConfig("box", names=["x"], **BOX), DW.FileWriterConfig("all")])
    w, time = infer(tmp_path, cfg)
    assert sorted(os.listdir(tmp_path)) == ["all.pt", "autoregressive_predictions.pt", "box.pt", "initial_condition.pt", "restart.pt"]
    raw, box, full = load(tmp_path, "autoregressive_predictions.pt"), load(tmp_path, "box.pt"), load(tmp_path, "all.pt")
    assert set(box) == {"x", "time", "calendar", "lat", "lon"} and set(full) == {"x", "d", "time", "calendar", "lat", "lon"}
    assert box["x"].dtype == torch.float32 and box["x"].shape == (1, 12, 4, 6) and full["d"].shape == (1, 12, H, W)
    assert torch.equal(bits(box["x"]), bits(raw["x"][:, :, ROWS, COLS])) and torch.equal(bits(full["d"]), bits(raw["d"]))
    assert box["time"].dtype == torch.int64 and np.array_equal(box["time"].numpy(), time.us[:, 1:]) and box["calendar"] == time.calendar
    assert np.array_equal(box["lat"].numpy(), [-45.0, -15.0, 15.0, 45.0]) and np.array_equal(box["lon"].numpy(), COORDS["lon"][COLS])
    assert np.array_equal(full["lat"].numpy(), COORDS["lat"]) and np.array_equal(full["lon"].numpy(), COORDS["lon"])
    fw = w._writers[1]
    assert fw._n_timesteps_seen == 12 and fw.reducer.last_path == "torch" and not os.path.exists(fw.path + ".tmp")


def test_no_coords_and_no_time_leave_their_keys_out(tmp_path):
    cfg = DW.DataWriterConfig(save_monthly_files=False, save_prediction_files=False,
                              files=[DW.FileWriterConfig("all", names=["d", "absent"])])
    infer(tmp_path, cfg, coords=None, with_time=False)
    assert set(load(tmp_path, "all.pt")) == {"d"}


@pytest.mark.parametrize("sel", [DW.Slice(1, 5), DW.Slice(None, None, 2), DW.Slice(3), DW.Slice(0, 6, 4)])
def test_box_coarsened_and_sliced_equals_the_slice_of_the_time_coarsen_file(tmp_path, sel):
    cfg = DW.DataWriterConfig(save_monthly_files=False, time_coarsen=DW.TimeCoarsenConfig(2), files=[
        DW.FileWriterConfig("box", time_selection=sel, time_coarsen=DW.TimeCoarsenConfig(2), **BOX)])
    cfg.validate_time_coarsen(4, 12)
    w, time = infer(tmp_path, cfg)
    raw, box = load(tmp_path, "autoregressive_predictions.pt"), load(tmp_path, "box.pt")
    # two coarsened steps a window: the kept ones, window by window, as the reference shifts the slice
    kept = [n + k for n in (0, 2, 4) for k in range(2)[DW.Slice.shift_left(sel, n).slice]]
    assert kept and box["x"].shape == (1, len(kept), 4, 6)
    for n in ("x", "d"):
        assert torch.equal(bits(box[n]), bits(raw[n][:, kept][:, :, ROWS, COLS])), n
    assert np.array_equal(box["time"].numpy(), DW.coarsen_time(time[:, 1:], 2).us[:, kept])
    assert w._writers[1]._n_timesteps_seen == 6                           # coarsened steps


def test_regional_monthly_equals_the_slice_of_the_monthly_file(tmp_path):
    cfg = DW.DataWriterConfig(save_prediction_files=False, files=[
        DW.FileWriterConfig("box_monthly", names=["x", "d"], time_coarsen=DW.MonthlyCoarsenConfig(), **BOX)])
    w, _ = infer(tmp_path, cfg, n_steps=12, in_memory=5, B=2)            # windows of 5, 5 and 2 steps; February starts at step 12
    mon, box = load(tmp_path, "monthly_mean_predictions.pt"), load(tmp_path, "box_monthly.pt")
    assert set(box) == set(mon) | {"lat", "lon"} and mon["counts"].tolist() == [[11, 1]] * 2
    for k in ("counts", "time", "valid_time"):
        assert torch.equal(box[k], mon[k])
    for n in ("x", "d"):
        assert box[n].shape == (2, 2, 4, 6) and torch.equal(bits(box[n]), bits(mon[n][:, :, ROWS, COLS])), n
        assert torch.equal(bits(w._writers[1]._monthly._totals[n]), bits(w._writers[0]._totals[n][:, :, ROWS, COLS])), n
    assert np.array_equal(box["lat"].numpy(), COORDS["lat"][ROWS]) and w._writers[1]._n_timesteps_seen == 12


def test_month_selector_through_run_inference(tmp_path):
    cfg = DW.DataWriterConfig(save_monthly_files=False, files=[DW.FileWriterConfig("jja", time_selection=DW.MonthSelector(["JJA"]))])
    rec = dict(start=(2020, 5, 15, 0), step=datetime.timedelta(days=10))
    w, time = infer(tmp_path, cfg, **rec)
    raw, jja = load(tmp_path, "autoregressive_predictions.pt"), load(tmp_path, "jja.pt")
    month = time[:, 1:].year_month()[1][0]
    kept = [int(i) for i in np.nonzero((month >= 6) & (month <= 8))[0]]
    assert kept == list(range(1, 10))                                     # 25 May | 4 June .. 23 August | 2 and 12 September
    assert torch.equal(bits(jja["x"]), bits(raw["x"][:, kept])) and np.array_equal(jja["time"].numpy(), time.us[:, 1:][:, kept])
    with pytest.raises(ValueError, match="needs the windows' time axis"):
        infer(tmp_path / "notime", cfg, with_time=False, **rec)
    with pytest.raises(NotImplementedError, match="MonthSelector selection is not currently supported for multiple initial conditions"):
        infer(tmp_path / "two", cfg, B=2, **rec)
    # after coarsening the labels are the block means: blocks of 2 from 25 May have their label 5 days before their second step
    cfg = DW.DataWriterConfig(save_monthly_files=False, time_coarsen=DW.TimeCoarsenConfig(2), files=[
        DW.FileWriterConfig("jja", time_selection=DW.MonthSelector(["Jun", "August"]), time_coarsen=DW.TimeCoarsenConfig(2))])
    _, time = infer(tmp_path / "coarse", cfg, **rec)
    coarse = DW.coarsen_time(time[:, 1:], 2)
    kept = [int(i) for i in np.nonzero(np.isin(coarse.year_month()[1][0], (6, 8)))[0]]
    raw, jja = load(tmp_path / "coarse", "autoregressive_predictions.pt"), load(tmp_path / "coarse", "jja.pt")
    assert 0 < len(kept) < 6 and torch.equal(bits(jja["d"]), bits(raw["d"][:, kept]))
    assert np.array_equal(jja["time"].numpy(), coarse.us[:, kept])


@pytest.mark.parametrize("save_reference", [True, False])
def test_paired_files_through_run_evaluator(tmp_path, save_reference):
    f, ic, time = record(8)
    tgt = torch.arange(9 * H * W, dtype=torch.float32).reshape(1, 9, H, W)
    cfg = DW.DataWriterConfig(save_monthly_files=False, files=[
        DW.FileWriterConfig("box", save_reference=save_reference, time_selection=DW.Slice(2, 7), **BOX)])
    w = cfg.build_paired(str(tmp_path), coords=COORDS)
    run_evaluator(paired_predict, InferenceData(ic, ForcingWindows({"f": f, "x": tgt}, 8, 4, device="cpu", time=time)), Agg(), writer=w)
    mine = ["box_predictions.pt", "box_target.pt"] if save_reference else ["box.pt"]
    assert sorted(os.listdir(tmp_path)) == sorted(mine + ["autoregressive_predictions.pt", "autoregressive_target.pt",
                                                          "initial_condition.pt", "restart.pt"])
    raw = load(tmp_path, "autoregressive_predictions.pt")
    gen = load(tmp_path, mine[0])
    assert set(gen) == {"x", "d", "time", "calendar", "lat", "lon"}
    assert torch.equal(bits(gen["x"]), bits(raw["x"][:, 2:7, ROWS, COLS])) and np.array_equal(gen["time"].numpy(), time.us[:, 3:8])
    if save_reference:
        ref = load(tmp_path, "box_target.pt")
        assert set(ref) == {"x", "time", "calendar", "lat", "lon"} and torch.equal(ref["x"], tgt[:, 3:8, ROWS, COLS])
        assert torch.equal(ref["time"], gen["time"])
    pw = w._writers[-1]
    assert (pw.reference_writer is not None) == save_reference and pw.prediction_writer._n_timesteps_seen == 8


def test_the_empty_window_warning_is_capped(tmp_path, caplog):
    f, _, time = record(4)
    w = DW.FileWriterConfig("late", time_selection=DW.Slice(1000, None)).build(str(tmp_path))
    with caplog.at_level(logging.WARNING, logger=DW.__name__):
        for _ in range(14):
            w.append_batch({"x": f[:, 1:]}, time=time[:, 1:])
    lines = [r.getMessage() for r in caplog.records]
    assert [m for m in lines if m.startswith("No data to write for region late at timestep")] == \
        [f"No data to write for region late at timestep {4 * i}." for i in range(9)]
    assert lines.count("Further warnings about empty data will be suppressed.") == 1 and len(lines) == 10
    assert w._n_timesteps_seen == 56 and w._no_write_count == 14
    w.finalize()
    assert not os.path.exists(w.path)                                     # nothing kept, nothing written
    with caplog.at_level(logging.WARNING, logger=DW.__name__):
        DW.FileWriterConfig("both", time_selection=DW.Slice(0, 2), time_coarsen=DW.TimeCoarsenConfig(2))
    assert "Time subselection is applied *after* time coarsening" in caplog.records[-1].getMessage()


def test_window_checks(tmp_path):
    f, _, time = record(4)
    w = DW.FileWriterConfig("box", **BOX).build(str(tmp_path), coords={"lat": np.arange(8.0), "lon": np.arange(12.0) * 30})
    with pytest.raises(ValueError, match="8 x 12, the fields are 6 x 12"):
        w.append_batch({"x": f[:, 1:]})
    w = DW.FileWriterConfig("box", time_coarsen=DW.TimeCoarsenConfig(3)).build(str(tmp_path))
    with pytest.raises(ValueError, match="a window of 4 steps is not a multiple of coarsen_factor 3"):
        w.append_batch({"x": f[:, 1:]})
    with pytest.raises(ValueError, match="time must be"):
        DW.FileWriterConfig("box").build(str(tmp_path)).append_batch({"x": f[:, 1:]}, time=time)
