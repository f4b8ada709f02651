"""The fused inference aggregator (csrc/diag.hip: ace_diag_window, ace_diag_spectrum) against fp64 restatements of the reference's
no-target InferenceAggregator, against its own torch path, bitwise against itself, and under ``run_inference`` on the SFNO and
Samudra fixtures (tests/golden/gen_checkpoint.pt, gen_ocean_rollout.pt)."""
import copy

import pytest
import torch

from ace_amd.aggregator import InferenceAggregatorConfig
from ace_amd.dataset_info import DatasetInfo
from ace_amd.masking import SpatialMaskProvider
from oracle.sht import RealSHT as OracleSHT
from _util import load_golden

pytestmark = pytest.mark.gpu

NLAT, NLON = 180, 360


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def one_degree_info():
    lat = torch.tensor([-89.5 + i for i in range(NLAT)], dtype=torch.float64)
    lon = torch.tensor([0.5 + j for j in range(NLON)], dtype=torch.float64)
    mask = torch.ones(NLAT, NLON)
    mask[40:120, 100:200] = 0.0
    return DatasetInfo((NLAT, NLON), lat=lat, lon=lon, mask_provider=SpatialMaskProvider({"mask_sst": mask}))


def fields(g, B, T, dev):
    """six names: noise, a smooth field, a positive one, a surface-pressure-like one, a masked one (NaN on land), a derived one"""
    lat = torch.linspace(-1.5, 1.5, NLAT)[:, None]
    lon = torch.linspace(0, 6.28, NLON)[None, :]
    d = {"a": torch.randn(B, T, NLAT, NLON, generator=g),
         "smooth": torch.cos(lat) * torch.sin(2 * lon) + 0.01 * torch.randn(B, T, NLAT, NLON, generator=g),
         "q": torch.rand(B, T, NLAT, NLON, generator=g) * 1e-3,
         "PRESsfc": 1e5 + 1e2 * torch.randn(B, T, NLAT, NLON, generator=g),
         "sst": 290 + 5 * torch.randn(B, T, NLAT, NLON, generator=g),
         "derived": torch.randn(B, T, NLAT, NLON, generator=g) ** 2}
    mask = one_degree_info().mask_provider.get_mask_tensor_for("sst")
    d["sst"] = d["sst"].where(mask.expand_as(d["sst"]) != 0, torch.tensor(float("nan")))
    return {k: v.to(dev) for k, v in d.items()}


def moments64(x, w):
    """metrics.py weighted_mean / weighted_std per (sample, step) in fp64, batch mean"""
    x = x.double().cpu()
    w = w.double().cpu()
    m = (x.where(w != 0, 0.0) * w).sum((-2, -1)) / w.sum()
    v = (((x - m[..., None, None]) ** 2).where(w != 0, 0.0) * w).sum((-2, -1)) / w.sum()
    return m.mean(0), v.sqrt().mean(0)


def build(info, n_time, fused=True):
    agg = InferenceAggregatorConfig().build(info, n_time)
    agg.fused = fused
    return agg


def test_series_match_fp64(dev):
    info = one_degree_info()
    win = fields(torch.Generator().manual_seed(0), 2, 5, dev)
    agg = build(info, 5)
    assert agg.route(win) == "fused"
    agg.record_batch(win)
    ds = agg.get_dataset()["mean"]
    for n, x in win.items():
        w = agg.weights_for(n, "cpu")
        m64, s64 = moments64(x, w)
        gm, gs = ds[f"weighted_mean_gen-{n}"].double(), ds[f"weighted_std_gen-{n}"].double()
        assert float(((gm - m64).abs() / m64.abs()).max()) <= 1e-6, n
        assert float(((gs - s64).abs() / s64.abs()).max()) <= 1e-5, n
    # the tolerance tells a sound std from the one-pass E[x^2] - m^2 in fp32, which loses surface pressure's digits
    x, w = win["PRESsfc"], agg.weights_for("PRESsfc", dev)
    m = (x * w).sum((-2, -1)) / w.sum()
    naive = ((x * x * w).sum((-2, -1)) / w.sum() - m * m).clamp_min(0).sqrt().mean(0)
    _, s64 = moments64(x, w.cpu())
    assert float(((naive.double().cpu() - s64).abs() / s64).max()) > 1e-5


def _run(info, ic, wins, n_time, fused=True):
    agg = build(info, n_time, fused)
    agg.record_initial_condition(ic)
    for win in wins:
        agg.record_batch(win)
    return agg


def _record(dev):
    g = torch.Generator().manual_seed(1)
    ic = {k: v for k, v in fields(g, 2, 1, dev).items() if k != "derived"}
    wins = [fields(g, 2, t, dev) for t in (3, 3, 2)]
    return ic, wins


def test_time_mean_maps_match_fp64_and_runs_are_bitwise_equal(dev):
    info = one_degree_info()
    ic, wins = _record(dev)
    agg = _run(info, ic, wins, 9)
    ds = agg.get_dataset()
    for n in wins[0]:
        want = sum(w[n].double().cpu().sum((0, 1)) for w in wins) / 8 / 2
        got = ds["time_mean"][f"gen_map-{n}"]
        ok = ~torch.isnan(want)
        assert torch.equal(torch.isnan(got), ~ok), n
        assert float((got.double()[ok] - want[ok]).abs().max() / want[ok].abs().max()) <= 1e-6, n
    again = _run(info, ic, wins, 9).get_dataset()
    for sub, d in ds.items():
        for k, v in d.items():
            assert torch.equal(v.view(torch.int32), again[sub][k].view(torch.int32)), (sub, k)


def test_spectrum_matches_fp64_sht(dev):
    info = one_degree_info()
    ic, wins = _record(dev)
    agg = _run(info, ic, wins, 9)
    spec = agg.get_dataset()["power_spectrum"]
    assert agg.omitted == ["sst"] and "sst" not in spec
    sht = OracleSHT(NLAT, NLON, grid="legendre-gauss", dtype=torch.float64)
    for n, got in spec.items():
        tot = 0
        for w in wins:
            c = sht(w[n].double().cpu())
            tot = tot + (c.real ** 2 + c.imag ** 2).sum(-1).sum((0, 1))
        want = tot / (8 * 2)
        assert got.shape == (NLAT,)
        assert float((got.double() - want).abs().max() / want.abs().max()) <= 1e-5, n


def _agree(fused, reference, magnitude=None):
    """fused get_dataset against another one (fp64 restatement or torch path).  Series errors are relative to the series'
    largest magnitude (a std of a field that is constant at a step is 0 there) or, with ``magnitude`` (name -> weighted mean of
    |x|), to the larger of that and the summands' size: the torch path sums in fp32, and a mean that cancels (a tendency) keeps
    only the digits fp32 leaves of its summands."""
    for k, v in reference["mean"].items():
        g, r = fused["mean"][k].double(), v.double()
        tol = 1e-6 if k.startswith("weighted_mean") else 1e-5
        scale = float(r.abs().max())
        if magnitude is not None:
            scale = max(scale, magnitude[k.split("-", 1)[1]])
        assert float((g - r).abs().max()) <= tol * max(scale, 1e-30), k
    for k, v in reference["time_mean"].items():
        g, r = fused["time_mean"][k].double(), v.double()
        ok = ~torch.isnan(r)
        assert torch.equal(torch.isnan(g), ~ok), k
        assert float((g[ok] - r[ok]).abs().max() / r[ok].abs().max()) <= 1e-6, k
    assert set(fused["power_spectrum"]) == set(reference["power_spectrum"])
    for k, v in reference["power_spectrum"].items():
        g, r = fused["power_spectrum"][k].double(), v.double()
        assert float((g - r).abs().max() / r.abs().max()) <= 1e-5, k


def _fp64_of_writer(agg, ic, series, n_time):
    """the reference's reductions in fp64 of the run's TensorFileWriter output (initial condition + all windows)"""
    mean, std = {}, {}
    for n in sorted(series):
        w = agg.weights_for(n, "cpu")
        m, s = moments64(series[n], w)
        if n in ic:
            m0, s0 = moments64(ic[n].cpu(), w)
        else:
            m0, s0 = torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
        mean[f"weighted_mean_gen-{n}"] = torch.cat([m0, m])
        std[f"weighted_std_gen-{n}"] = torch.cat([s0, s])
    magnitude = {n: float(moments64(x.abs(), agg.weights_for(n, "cpu"))[0].max()) for n, x in series.items()}
    B, T = next(iter(series.values())).shape[:2]
    maps = {f"gen_map-{n}": x.double().sum((0, 1)) / T / B for n, x in series.items()}
    nlat, nlon = next(iter(series.values())).shape[-2:]
    sht = OracleSHT(nlat, nlon, grid="legendre-gauss", dtype=torch.float64)
    spec = {}
    for n, x in series.items():
        if n in agg.omitted:
            continue
        c = sht(x.double())
        spec[n] = (c.real ** 2 + c.imag ** 2).sum(-1).mean((0, 1))
    return {"mean": {**mean, **std}, "time_mean": maps, "power_spectrum": spec}, magnitude


def _end_to_end(dev, tmp_path, stepper, dataset_info, ic, forcing, total, T, derived):
    from ace_amd.inference import EnginePredict, ForcingWindows, InferenceData, TensorFileWriter, run_inference
    results = {}
    for fused in (True, False):
        loader = ForcingWindows(forcing, total_forward_steps=total, forward_steps_in_memory=T, device=dev)
        assert len(loader) == 2
        agg = InferenceAggregatorConfig().build(dataset_info, total + 1)
        agg.fused = fused
        writer = TensorFileWriter(str(tmp_path / str(fused)))
        run_inference(EnginePredict(stepper, batch=2, graph="step"), InferenceData(ic, loader), aggregator=agg, writer=writer,
                      compute_derived_variables=derived)
        results[fused] = (agg, torch.load(tmp_path / str(fused) / "autoregressive_predictions.pt", weights_only=True))
    agg, series = results[True]
    assert agg.launches() >= 2 and agg._path == "fused" and results[False][0]._path == "torch"
    fused = agg.get_dataset()
    want, magnitude = _fp64_of_writer(agg, ic, series, total + 1)
    _agree(fused, want)
    _agree(fused, results[False][0].get_dataset(), magnitude)
    return agg


def test_end_to_end_sfno_fixture(dev, tmp_path):
    import ace_amd
    g = load_golden("gen_checkpoint.pt")["ace2_like"]
    loaded = ace_amd.load_stepper(g["state"], device=dev)
    ic = {k: v.to(dev) for k, v in g["ic"].items()}
    _end_to_end(dev, tmp_path, loaded.stepper, loaded.dataset_info, ic, g["forcing"], len(g["steps"]), 2, derived=True)


def test_end_to_end_samudra_fixture(dev, tmp_path):
    from ace_amd.checkpoint import load_stepper
    case = load_golden("gen_ocean_rollout.pt")
    state = copy.deepcopy(case["stepper"])
    state["step"]["module"] = {k: (v.float() if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
                               for k, v in state["step"]["module"].items()}
    di = state["dataset_info"]
    di["mask_provider"]["masks"] = {k: v.float() for k, v in di["mask_provider"]["masks"].items()}
    di["vertical_coordinate"]["mask"] = di["vertical_coordinate"]["mask"].float()
    loaded = load_stepper({"stepper": state}, device=dev)
    ic = {k: v.to(dev) for k, v in case["initial_condition"].items()}
    agg = _end_to_end(dev, tmp_path, loaded.stepper, loaded.dataset_info, ic, case["forcing"], 4, 2, derived=False)
    assert agg.omitted                                          # masked ocean outputs are listed, not dropped silently


def test_launches_per_window_are_bounded(dev):
    info = one_degree_info()
    g = torch.Generator().manual_seed(2)
    for T, names in ((2, ["a", "q"]), (6, ["a", "q", "smooth", "PRESsfc", "sst", "derived"])):
        win = {k: v for k, v in fields(g, 1, T, dev).items() if k in names}
        agg = build(info, 2 * T)
        agg.record_batch(win)
        assert agg.launches() == 3                  # ace_diag_window + one SHT + one ace_diag_spectrum
        agg.record_batch(win)
        assert agg.launches() == 6
    small = build(info, 6)
    small.spectrum_chunk_bytes = 1                  # one name per SHT chunk: 1 + 2 launches per chunk
    small.record_batch({k: v for k, v in fields(g, 1, 3, dev).items() if k in ("a", "q", "sst")})
    assert small.launches() == 1 + 2 * 2


# ---- other grids, strided fields, chunked spectra, late names ------------------------------------------------------------------
def grid_info(nlat, nlon):
    lat = torch.tensor([-90 + (i + 0.5) * 180 / nlat for i in range(nlat)], dtype=torch.float64)
    lon = torch.tensor([(j + 0.5) * 360 / nlon for j in range(nlon)], dtype=torch.float64)
    mask = torch.ones(nlat, nlon)
    mask[nlat // 4:nlat // 2, nlon // 3:nlon // 2] = 0.0
    return DatasetInfo((nlat, nlon), lat=lat, lon=lon, mask_provider=SpatialMaskProvider({"mask_sst": mask}))


GRID_NAMES = ("a", "PRESsfc", "sst", "static")


def grid_packed(g, B, T, nlat, nlon):
    """one packed (B, T, C, H, W) CPU tensor, C in the order of GRID_NAMES; "sst" is NaN on land, "static" the same at every step"""
    p = torch.randn(B, T, len(GRID_NAMES), nlat, nlon, generator=g)
    p[:, :, 1] = 1e5 + 1e2 * p[:, :, 1]
    mask = grid_info(nlat, nlon).mask_provider.get_mask_tensor_for("sst")
    p[:, :, 2] = (290 + 5 * p[:, :, 2]).where(mask != 0, torch.tensor(float("nan")))
    p[:, :, 3] = p[:, :1, 3]
    return p


def strided_window(packed, dev):
    """channel slices of the packed device tensor, an expanded static field, rows that are not contiguous"""
    p = packed.to(dev)
    win = {n: p[:, :, c] for c, n in enumerate(GRID_NAMES)}
    win["static"] = p[:, :1, 3].expand(-1, p.shape[1], -1, -1)
    win["a"] = p[:, :, 0].transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not win["PRESsfc"].is_contiguous() and win["static"].stride(1) == 0 and win["a"].stride(-1) != 1
    return win


def _bitwise(a, b):
    assert set(a) == set(b)
    for sub, d in a.items():
        assert set(d) == set(b[sub]), sub
        for k, v in d.items():
            assert torch.equal(v.view(torch.int32), b[sub][k].view(torch.int32)), (sub, k)


@pytest.mark.parametrize("nlat,nlon", [(45, 90), (13, 27), (NLAT, NLON)])
def test_grids_and_strided_fields(dev, nlat, nlon):
    """45 x 90 (hw % 4 == 2) and 13 x 27 (odd nlat, odd hw) beside 180 x 360: the fused path on channel slices of a packed tensor,
    an expanded static field and non-contiguous rows gives the contiguous run's bits, which agree with the fp64 restatement"""
    info = grid_info(nlat, nlon)
    g = torch.Generator().manual_seed(nlat)
    B = 2
    ic_p = grid_packed(g, B, 1, nlat, nlon)
    packs = [grid_packed(g, B, T, nlat, nlon) for T in (3, 2)]
    ic = {n: ic_p[:, :, c].contiguous().to(dev) for c, n in enumerate(GRID_NAMES)}
    plain = [{n: p[:, :, c].contiguous().to(dev) for c, n in enumerate(GRID_NAMES)} for p in packs]
    strided = [strided_window(p, dev) for p in packs]
    aggs = []
    for wins in (plain, strided):
        agg = build(info, 6)
        agg.record_initial_condition(ic)
        for win in wins:
            assert agg.route(win) == "fused"
            agg.record_batch(win)
        assert agg._path == "fused"
        aggs.append(agg)
    ds = aggs[0].get_dataset()
    _bitwise(ds, aggs[1].get_dataset())
    series = {n: torch.cat([p[:, :, c] for p in packs], dim=1) for c, n in enumerate(GRID_NAMES)}
    want, _ = _fp64_of_writer(aggs[0], {n: v.cpu() for n, v in ic.items()}, series, 6)
    assert aggs[0].omitted == ["sst"]
    _agree(ds, want)


def _three_windows(dev, nlat=45, nlon=90, B=2):
    g = torch.Generator().manual_seed(11)
    info = grid_info(nlat, nlon)
    wins = []
    for T in (2, 3, 2):
        p = grid_packed(g, B, T, nlat, nlon)
        wins.append({n: p[:, :, c].contiguous().to(dev) for c, n in enumerate(GRID_NAMES)})
    return info, wins


@pytest.mark.parametrize("nlat,nlon", [(45, 90), (NLAT, NLON)])
def test_chunked_spectrum_is_bitwise_the_unchunked_one(dev, nlat, nlon):
    """each (row, l) is one workgroup's fixed-order sum over one name's coefficients: one name per SHT chunk changes no bit"""
    info, wins = _three_windows(dev, nlat, nlon)
    out = []
    for chunk in (None, 1):
        agg = build(info, 7)
        if chunk:
            agg.spectrum_chunk_bytes = chunk
        for win in wins:
            agg.record_batch(win)
        assert agg.launches() == (3 * (1 + 2 * 3) if chunk else 3 * 3)          # "sst" is omitted: three names in the spectrum
        out.append(agg.get_dataset())
    _bitwise({"power_spectrum": out[0]["power_spectrum"]}, {"power_spectrum": out[1]["power_spectrum"]})
    _bitwise(out[0], out[1])


def test_name_that_first_appears_in_the_third_window(dev):
    """the accumulators grow and are copied: the late name reads 0 before it appears and its own values are right; every earlier
    name's series, map and spectrum keep the bits of a run without it"""
    info, wins = _three_windows(dev)
    g = torch.Generator().manual_seed(12)
    late = (3.0 + torch.randn(2, 2, 45, 90, generator=g)).to(dev)
    base = build(info, 7)
    grown = build(info, 7)
    for i, win in enumerate(wins):
        base.record_batch(win)
        grown.record_batch({**win, "late": late} if i == 2 else win)
    assert grown._path == "fused" and len(grown._rows) == len(base._rows) + 1
    a, b = base.get_dataset(), grown.get_dataset()
    for sub in a:
        _bitwise({sub: a[sub]}, {sub: {k: v for k, v in b[sub].items() if not k.endswith("late")}})
    m64, s64 = moments64(late, grown.weights_for("late", "cpu"))
    gm, gs = b["mean"]["weighted_mean_gen-late"].double(), b["mean"]["weighted_std_gen-late"].double()
    assert bool((gm[:5] == 0).all()) and bool((gs[:5] == 0).all())
    assert float(((gm[5:] - m64).abs() / m64.abs()).max()) <= 1e-6 and float(((gs[5:] - s64).abs() / s64.abs()).max()) <= 1e-5
    sht = OracleSHT(45, 90, grid="legendre-gauss", dtype=torch.float64)
    c = sht(late.double().cpu())
    want = (c.real ** 2 + c.imag ** 2).sum(-1).mean((0, 1))
    assert float((b["power_spectrum"]["late"].double() - want).abs().max() / want.abs().max()) <= 1e-5


def test_fused_without_time_series(dev):
    """log_global_mean_time_series=False on the fused path (the window's series go to scratch): no "mean", and the maps and spectra
    keep the bits of the run with the series on"""
    info, wins = _three_windows(dev)
    ic = {n: x[:, :1] for n, x in wins[0].items()}
    out = []
    for log in (True, False):
        agg = InferenceAggregatorConfig(log_global_mean_time_series=log).build(info, 8)
        agg.record_initial_condition(ic)
        for win in wins:
            assert agg.route(win) == "fused"
            agg.record_batch(win)
        assert agg._path == "fused"
        out.append(agg.get_dataset())
    assert set(out[0]) == {"mean", "time_mean", "power_spectrum"} and set(out[1]) == {"time_mean", "power_spectrum"}
    _bitwise({k: out[0][k] for k in out[1]}, out[1])


def test_torch_window_after_a_fused_one_is_refused(dev):
    info, wins = _three_windows(dev)
    agg = build(info, 7)
    agg.record_batch(wins[0])
    assert agg._path == "fused"
    with pytest.raises(ValueError, match="fused path.*torch path"):
        agg.record_batch({n: x.double() for n, x in wins[1].items()})


# ---- the spectrum's tail, degree by degree --------------------------------------------------------------------------------
def temperature_like(nlat, nlon, seed=0):
    """two samples, one step, fp32: power per degree about (l + 1)^-3 (coefficients randn * (l + 1)^-2, zero for m > l, real at
    m = 0, through the fp64 inverse transform) plus 250"""
    from oracle.sht import InverseRealSHT
    g = torch.Generator().manual_seed(seed)
    L, M = nlat, nlon // 2 + 1
    c = torch.complex(torch.randn(2, 1, L, M, generator=g, dtype=torch.float64), torch.randn(2, 1, L, M, generator=g, dtype=torch.float64))
    l, m = torch.arange(L)[:, None], torch.arange(M)[None, :]
    c = c * (l + 1.0) ** -2 * (m <= l)
    c[..., 0] = c[..., 0].real + 0j
    x = InverseRealSHT(nlat, nlon, grid="legendre-gauss", dtype=torch.float64)(c) + 250.0
    return x.float()


@pytest.mark.parametrize("nlat,nlon", [(45, 90), (NLAT, NLON)])
def test_spectrum_tail_per_degree(dev, nlat, nlon):
    """e(l) = |S(l) - S64(l)| / S64(l) per degree, not normalised by the spectrum's peak: the fused spectrum (native fp32 SHT +
    ace_diag_spectrum) and the torch path on the device (native SHT + torch sums) are held to 4x the error of the reference's own
    formula in fp32 (the CPU oracle), in the maximum and in the median over the degrees.  The factor is a margin for two fp32
    computations that round in different orders, over the reference's error, not the kernel's."""
    x = temperature_like(nlat, nlon)

    def spectrum(dtype):
        c = OracleSHT(nlat, nlon, grid="legendre-gauss", dtype=dtype)(x)
        return (c.real.double() ** 2 + c.imag.double() ** 2).sum(-1).mean((0, 1))

    s64 = spectrum(torch.float64)
    e32 = (spectrum(torch.float32) - s64).abs() / s64
    print(f"DIAGACC tail {nlat}x{nlon} fp32 oracle: max {float(e32.max()):.3e} (l = {int(e32.argmax())}) median "
          f"{float(e32.median()):.3e}, spectrum range {float(s64.max() / s64.min()):.1e}")
    assert float(e32.max()) <= 2e-2                      # the yardstick itself resolves every degree
    info = grid_info(nlat, nlon)
    failures = []
    for fused in (True, False):
        agg = build(info, 2, fused)
        agg.record_initial_condition({"t": x[:, 0].to(dev)})
        agg.record_batch({"t": x.to(dev)})
        assert agg._path == ("fused" if fused else "torch")
        e = (agg.get_dataset()["power_spectrum"]["t"].double() - s64).abs() / s64
        print(f"DIAGACC tail {nlat}x{nlon} {'fused' if fused else 'torch path on the device'}: max {float(e.max()):.3e} "
              f"(l = {int(e.argmax())}) median {float(e.median()):.3e}; ratios to the oracle {float(e.max() / e32.max()):.2f} "
              f"{float(e.median() / e32.median()):.2f}")
        if not (float(e.max()) <= 4 * float(e32.max()) and float(e.median()) <= 4 * float(e32.median())):
            failures.append(("fused" if fused else "torch", float(e.max() / e32.max()), float(e.median() / e32.median())))
    assert not failures, failures
