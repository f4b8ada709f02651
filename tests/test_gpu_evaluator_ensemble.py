"""The evaluator's ensemble metrics and step means on the fused path (csrc/ensemble.hip: one ace_diag_ensemble_step per entry and
window that holds its step; the step means are columns of the paired pass's series) on the records of tests/_ensemble_cases.py.

The ensemble outputs are compared two ways, as tests/test_gpu_evaluator_calendar.py compares the calendar metrics:
  * against a twin whose device buffers are filled by tests/_ensemble_ref.py, the numpy statement of the header contract, window by
    window through the class's own bookkeeping, and then read by the same host post-processing: 1e-9 relative to the largest value
    of each output (both sides see the same fp32 inputs and add in the same order; a square root or a division may differ by an
    ulp, which the spread-skill ratio's division by a small clamped skill amplifies);
  * against the aggregator's own torch path on the same device: within 3 x the torch path's own fp32 error against the fp64 twin,
    that floor computed on the CPU (tests/test_evaluator_ensemble_cpu.py holds the torch path to the reference).  The floor of a
    map is its largest error.  A scalar is the torch path's fp32 area-weighted mean of its map, so its own floor can vanish by
    chance; its error is at most the map's largest error plus the rounding of the weighted mean - 35 products, two sums of 35
    terms and a division in fp32, at most 70 x 2^-24 of the map's largest value - so it is held to 3 x the map's floor plus that
    rounding.  A ``channel_mean`` is the average of per-name scalars and is held to the largest of their bars.
The step means are scalars of the paired pass (tests/test_gpu_evaluator_aggregator.py holds that pass to fp64): they are held to
the torch path run on the fp64 cast of the windows on the CPU, within one rounding to fp32 of the value (``_series_data`` returns
fp32) plus 1e-12 of the magnitude the sums are formed from (the field's values; 100 for the percent difference), the diag kernels'
bar for fp64 sums of fp32 inputs in another order."""
import math

import numpy as np
import pytest
import torch

import _ensemble_cases as C
import _ensemble_ref as R
from ace_amd.evaluator import EnsembleMetricConfig, StepMeanMetricConfig
from test_evaluator_calendar_cpu import config
from test_evaluator_ensemble_cpu import run
from test_gpu_diag_kernels import dev  # noqa: F401
from test_gpu_evaluator_calendar import err_of, flatten

pytestmark = pytest.mark.gpu
HW = C.H * C.W


def entries():
    return dict(ensembles=[EnsembleMetricConfig(step=2, log_mean_maps=True),
                           EnsembleMetricConfig(step=5, target="norm", log_mean_maps=True),
                           EnsembleMetricConfig(step=5, log_mean_maps=True, variables=["a", "c"], name="late")])


def twin(c, metrics):
    """the contract in numpy behind the class's bookkeeping and host post-processing: what the fused path must give"""
    agg = config(**metrics).build(c["info"], c["n_ic_steps"], C.N_FORWARD, C.stats(), n_ensemble_per_ic=C.E)
    ens = agg._ensembles
    ens._rows = {n: i for i, n in enumerate(C.NAMES)}
    ens._maps = torch.zeros(len(ens.configs), 4, len(C.NAMES), HW, dtype=torch.float64)
    ens._seen = torch.zeros(len(ens.configs), len(C.NAMES), dtype=torch.int32)
    for gen, tgt, i0 in c["windows"]:
        T = gen["a"].shape[1]
        flat = lambda d: [d[n].reshape(C.B, T, HW).numpy() for n in C.NAMES]          # noqa: E731
        for i, k in ens._selected(i0, T):
            R.ensemble_step(flat(gen), flat(tgt), [0, 1, 2], ens._maps.numpy(), ens._seen.numpy(), i, k, C.N_IC, C.E)
            ens._n[i] += 1
    return agg


def map_keys(k, floors):
    """the keys of the maps a scalar output is formed from: its own map, or for a channel mean the maps of the names that have a
    number; in the logs ``label/metric/name``, in the dataset ``dataset:label/metric-name``"""
    sep = "-" if k.startswith("dataset:") else "/"
    head, name = k.rsplit(sep, 1)
    if name != "channel_mean":
        return [f"{head}{sep}mean_map{sep}{name}"]
    return [f"{head}{sep}mean_map{sep}{n}" for n in C.NAMES if not math.isnan(float(floors[f"{head}{sep}{n}"]))]


def torch_bar(k, floors, low):
    """3 x the torch path's own fp32 error against the fp64 twin (module docstring)"""
    if torch.is_tensor(floors[k]) and floors[k].dim() > 0:
        return 3 * err_of(low[k], floors[k])
    top = lambda m: float(torch.as_tensor(floors[m]).double().abs().nan_to_num().max())      # noqa: E731
    return max(3 * err_of(low[m], floors[m]) + 70 * 2.0 ** -24 * top(m) for m in map_keys(k, floors))


def compare(name, got, want, rel=None, floors=None, low=None):
    """``rel``: every output of ``want`` in ``got``, NaN in the same places and |got - want| <= rel x max|want|.  Otherwise
    |got - want| <= ``torch_bar`` of the same output"""
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    worst, checked = 0.0, 0
    for k, w in want.items():
        g, w = torch.as_tensor(got[k], dtype=torch.float64).cpu(), torch.as_tensor(w, dtype=torch.float64).cpu()
        assert g.shape == w.shape and torch.equal(g.isnan(), w.isnan()), (name, k)
        err, top = float((g - w).abs().nan_to_num().max()), float(w.abs().nan_to_num().max())
        bar = rel * top if rel is not None else torch_bar(k, floors, low)
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else math.inf)
        print(f"ENSEVAL {name}: {k} err {err:.3e} bar {bar:.3e}")
        worst, checked = max(worst, ratio), checked + 1
        assert err <= bar, (name, k, err, bar)
    print(f"ENSEVAL {name}: {checked} outputs, worst err / bar {worst:.3e}")


@pytest.mark.parametrize("n_ic_steps", [1, 2])
def test_ensembles_against_the_contract_and_the_torch_path(dev, n_ic_steps):
    c, metrics = C.case(n_ic_steps), entries()
    truth, cpu_torch = flatten(twin(c, metrics)), flatten(run(c, **metrics))
    fused, torch_ = run(c, fused=True, device=dev, **metrics), run(c, fused=False, device=dev, **metrics)
    assert fused._path == "fused" and torch_._path == "torch"
    got = flatten(fused)
    ssr = got["ensemble_step_2/ssr_bias/mean_map/a"]
    assert ssr.dtype == torch.float64 and bool((ssr[C.PRESCRIBED] == 0).all()) and bool((ssr[C.CALM] == -1).all())
    assert "ensemble_step_5_norm/crps/channel_mean" in got and "late/crps/a" in got and "late/crps/b" not in got
    assert math.isnan(got["ensemble_step_5_norm/crps/c"]) and not math.isnan(got["ensemble_step_5_norm/crps/channel_mean"])
    compare(f"fused vs contract, n_ic_steps {n_ic_steps}", got, truth, rel=1e-9)
    compare(f"fused vs torch, n_ic_steps {n_ic_steps}", got, flatten(torch_), floors=truth, low=cpu_torch)


def test_one_native_call_per_entry_and_selected_step(dev):
    c, metrics = C.case(), entries()
    on = lambda d: {n: v.to(dev) for n, v in d.items()}                             # noqa: E731
    agg = config(**metrics).build(c["info"], 1, C.N_FORWARD, C.stats(), n_ensemble_per_ic=C.E)
    bare = config().build(c["info"], 1, C.N_FORWARD, C.stats(), n_ensemble_per_ic=C.E)
    for a in (agg, bare):
        a.record_initial_condition(on(c["ic"][0]), on(c["ic"][1]))
    want = [1, 3]                                       # the first window holds step 2, the second step 5 twice
    for (gen, tgt, _), calls in zip(c["windows"], want):
        agg.record_batch(on(gen), on(tgt))
        bare.record_batch(on(gen), on(tgt))
        assert agg._ensembles.calls == calls and agg.launches() - bare.launches() == calls
    assert agg._ensembles._n == [1, 1, 1]
    late = config(ensembles=[EnsembleMetricConfig(step=5)]).build(c["info"], 1, C.N_FORWARD, C.stats(), n_ensemble_per_ic=C.E)
    late.record_batch(on(c["windows"][0][0]), on(c["windows"][0][1]))
    assert late._ensembles.calls == 0 and late.get_summary_logs() == {}             # no call for a window without the step
    none = run(c, fused=True, device=dev, n_members=1, **metrics)                   # one member: accepted, never recorded
    assert none._ensembles is None and none.launches() == bare.launches() and none.get_summary_logs() == {}


def test_more_members_than_the_kernel_holds_are_refused(dev):
    c = C.case()
    gen, tgt, _ = c["windows"][0]
    wide = lambda d: {n: v.repeat(3, 1, 1, 1)[:33].to(dev) for n, v in d.items()}     # noqa: E731
    agg = config(ensembles=[EnsembleMetricConfig(step=2)]).build(c["info"], 1, C.N_FORWARD, C.stats(), n_ensemble_per_ic=33)
    with pytest.raises(ValueError, match="at most 32"):
        agg.record_batch(wide(gen), wide(tgt))


@pytest.mark.parametrize("n_ic_steps", [1, 2])
def test_step_means_on_the_fused_path(dev, n_ic_steps):
    c = C.case(n_ic_steps)
    metrics = dict(step_means=[StepMeanMetricConfig(step=2), StepMeanMetricConfig(step=2, target="norm", name="early_norm"),
                               StepMeanMetricConfig(step=5, target="norm", channel_mean_names=["a", "b"], variables=["a"])])
    fused = run(c, fused=True, device=dev, **metrics)
    assert fused._path == "fused"
    got = fused.get_summary_logs()
    c64 = dict(c, ic=tuple({n: v.double() for n, v in d.items()} for d in c["ic"]),
               windows=[({n: v.double() for n, v in g.items()}, {n: v.double() for n, v in t.items()}, i0) for g, t, i0 in c["windows"]])
    want = run(c64, **metrics).get_summary_logs()
    assert sorted(got) == sorted(want) and len(fused.get_inference_logs()) == 1
    assert "mean_step_5_norm/weighted_rmse/channel_mean" in got and "mean_step_5_norm/weighted_rmse/b" not in got
    assert math.isnan(got["early_norm/weighted_rmse/channel_mean"])                 # b's NaN is not a NaN target: b stays in
    for k, w in want.items():
        label, metric, name = k.split("/")
        size = {n: (abs(m) + 3 * C.STDS[n]) / (1.0 if label == "mean_step_2" else C.STDS[n]) for n, m in C.MEANS.items()}
        scale = 100.0 if "percent" in metric else max(size.values()) if name == "channel_mean" else size[name]
        assert math.isnan(got[k]) == math.isnan(w), k
        if not math.isnan(w):
            bar = 2.0 ** -23 * abs(w) + 1e-12 * scale
            print(f"ENSEVAL step mean {k}: err {abs(got[k] - w):.3e} bar {bar:.3e}")
            assert abs(got[k] - w) <= bar, (k, got[k], w)
