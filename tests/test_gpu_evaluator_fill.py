"""The masked-spectrum fill of both aggregators on the GPU at 180 x 360 with a masked "sst", B = 2, T = 3: the fused path
(ace_diag_fill_planes in place of the torch.stack) against the torch path (``smooth_flood_fill`` before the SHT), the launch
counts the docstrings state, chunked against unchunked, and the reuse of the cached tables.

Bars.  Spectra: 1e-5 x the spectrum's max, the bar of the fused-versus-torch spectrum test of test_gpu_evaluator_aggregator.py.
Bias scores: every score is a mean over l of r_l = g_l / t_l - 1 (or r at the last l), g the prediction's and t the target's
spectrum; with both spectra held to e = 1e-5 x max, |d r_l| <= e / t_l + g_l e / t_l^2, so a score is held to the largest of
that over l - the spectrum bar carried through the ratio, nothing wider."""
import pytest
import torch

from ace_amd.aggregator import InferenceAggregatorConfig
from ace_amd.evaluator import InferenceEvaluatorAggregatorConfig, PowerSpectrumMetricConfig
from test_gpu_aggregator import dev, fields, one_degree_info  # noqa: F401
from test_gpu_evaluator_aggregator import STATS, normalizer

pytestmark = pytest.mark.gpu

B, T = 2, 3
NAMES = ("a", "smooth", "q", "PRESsfc", "sst", "derived")


@pytest.fixture(scope="module")
def windows(dev):
    g = torch.Generator().manual_seed(21)
    wins = [fields(g, B, T, dev) for _ in range(2)]
    tgts = [{n: x + (0.05 * STATS[n][1]) * torch.randn(x.shape, generator=g).to(dev) for n, x in w.items() if n in STATS} for w in wins]
    return wins, tgts


def plain(wins, fused, fill=True, chunk=None):
    agg = InferenceAggregatorConfig(fill_masked_spectrum=fill).build(one_degree_info(), 2 * T)
    agg.fused = fused
    if chunk:
        agg.spectrum_chunk_bytes = chunk
    for w in wins:
        assert agg.route(w) == ("fused" if fused else "torch")
        agg.record_batch(w)
    return agg


def paired(wins, tgts, dev, fused, fill=True, chunk=None):
    cfg = InferenceEvaluatorAggregatorConfig(power_spectrum=PowerSpectrumMetricConfig(fill_masked=fill))
    agg = cfg.build(one_degree_info(), 1, 2 * T, normalize=normalizer(dev))
    agg.fused = fused
    if chunk:
        agg.spectrum_chunk_bytes = chunk
    agg.record_initial_condition({n: x[:, :1] for n, x in wins[0].items() if n != "derived"})
    for w, t in zip(wins, tgts):
        assert agg.route(w, t) == ("fused" if fused else "torch")
        agg.record_batch(w, t)
    return agg


def spectra_close(got, want, label):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)), label
    ok = ~torch.isnan(want)
    err, bar = float((got[ok] - want[ok]).abs().max()), 1e-5 * float(want[ok].abs().max())
    print(f"FILLACC fused-vs-torch {label}: {err / bar:.4f} of the bar")
    assert err <= bar, label


def test_the_plain_aggregator_fused_against_torch(dev, windows):
    wins, _ = windows
    fused, torch_path = plain(wins, True), plain(wins, False)
    assert fused._path == "fused" and torch_path._path == "torch"
    for agg in (fused, torch_path):
        assert agg.omitted == [] and agg.filled == ["sst"]
    assert fused.launches() == 2 * (1 + 3)              # per window: ace_diag_window, then fill, SHT and spectrum of one chunk
    assert plain(wins, True, fill=False).launches() == 2 * (1 + 2)
    got, want = fused.get_dataset()["power_spectrum"], torch_path.get_dataset()["power_spectrum"]
    assert set(got) == set(want) == set(NAMES)
    for n in NAMES:
        spectra_close(got[n], want[n], f"plain {n}")
    assert bool(torch.isfinite(got["sst"]).all())


def test_the_evaluator_fused_against_torch(dev, windows):
    wins, tgts = windows
    fused, torch_path, off = paired(wins, tgts, dev, True), paired(wins, tgts, dev, False), paired(wins, tgts, dev, True, fill=False)
    assert fused._path == "fused" and torch_path._path == "torch"
    assert fused.omitted == [] and fused.filled == ["sst"] and off.omitted == ["sst"] and off.filled == []
    # one chunk per side and window: the option turns 2 launches (SHT, spectrum) into 3 (fill, SHT, spectrum)
    assert fused.launches() == off.launches() + 2 * 2
    got, want = fused.get_dataset()["power_spectrum"], torch_path.get_dataset()["power_spectrum"]
    assert set(got) == set(want) == set(NAMES) and set(off.get_dataset()["power_spectrum"]) == set(NAMES) - {"sst"}
    for n in NAMES:
        spectra_close(got[n], want[n], f"paired {n}")
    logs, tlogs = fused.get_summary_logs(), torch_path.get_summary_logs()
    scores = [k for k in tlogs if k.startswith("power_spectrum/") and k.count("/") == 2]
    assert {k for k in logs if k.startswith("power_spectrum/")} == {k for k in tlogs if k.startswith("power_spectrum/")}
    assert "power_spectrum/mean_abs_norm_bias/sst" in scores and "power_spectrum/smallest_scale_norm_bias/sst" in scores
    for k in scores:
        g, t = want[k.rsplit("/", 1)[1]].double()
        e = 1e-5 * max(float(g.abs().max()), float(t.abs().max()))
        bar = float((e / t + g * e / t ** 2).max())
        print(f"FILLACC fused-vs-torch {k}: {abs(logs[k] - tlogs[k]) / bar:.4f} of the bar {bar:.3g}")
        assert abs(logs[k] - tlogs[k]) <= bar, k


def test_chunked_is_bitwise_the_unchunked_one(dev, windows):
    wins, tgts = windows
    whole, parts = plain(wins, True), plain(wins, True, chunk=1)
    assert parts.launches() == 2 * (1 + 3 * len(NAMES))
    a, b = whole.get_dataset()["power_spectrum"], parts.get_dataset()["power_spectrum"]
    for n in NAMES:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
    whole, parts = paired(wins, tgts, dev, True), paired(wins, tgts, dev, True, chunk=1)
    assert parts.launches() - whole.launches() == 2 * 3 * (len(NAMES) + len(STATS) - 2)      # one chunk per name, not per side
    a, b = whole.get_dataset()["power_spectrum"], parts.get_dataset()["power_spectrum"]
    for n in NAMES:
        assert torch.equal(a[n].nan_to_num(-1.0).view(torch.int32), b[n].nan_to_num(-1.0).view(torch.int32)), n


def test_the_tables_are_uploaded_once(dev, windows):
    wins, tgts = windows
    agg = plain(wins[:1], True)
    assert agg._fill.uploads == 1
    layers = agg._fill.stacks(dev)[0]
    agg.record_batch({n: x + 1 for n, x in wins[1].items()})
    assert agg._fill.uploads == 1 and agg._fill.stacks(dev)[0] is layers and agg._fill.stacks(dev)[2] == 1
    ev = paired(wins, tgts, dev, True)
    assert ev._fill.uploads == 1 and ev._fill.stacks(dev)[2] == 1
