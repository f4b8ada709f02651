"""tests/golden/gen_ensemble.pt from the reference's own classes (imported through oracle/ref_loader.load_stepper_ref's stubs, the
aggregator packages as bare namespaces and their plotting / build-context / data modules as permissive stubs, the stub
``Distributed`` given an identity ``reduce_mean`` here), on the records of tests/_ensemble_cases.py (exact arithmetic, rebuilt by
every test; the file pins their checksums and holds results only):
  * ``MeanAggregator`` (fme/ace/aggregator/one_step/reduced.py:24-183) built as ``StepMeanMetricConfig.build`` builds it
    (reduced.py:225-249: target_time = step + n_ic_steps - 1, bias and gradient magnitude for "denorm" only), fed window by window;
  * ``get_one_step_ensemble_aggregator`` (one_step/ensemble.py:31-50) built as ``EnsembleMetricConfig.build`` builds it
    (ensemble.py:485-505: target_time = step), fed the windows unfolded by ``unfold_ensemble_dim`` (fme/core/tensors.py:135-155),
    and the per-pixel maps of its ``CRPSMetric``, ``EnsembleMeanRMSEMetric`` and ``SSRBiasMetric``.
The normalised windows come from the reference's ``StandardNormalizer``.

Everything is computed twice: "f32" in the reference's dtypes, and "f64" with the same classes on fp64 inputs under a fp64 default
dtype.  tests/test_evaluator_ensemble_cpu.py takes its bars from the gap between the two."""
import importlib
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import _ensemble_cases as C  # noqa: E402
from oracle import ref_loader  # noqa: E402

# (key, n_ic_steps, step, target, channel_mean_names, variables): the entries tests/test_evaluator_ensemble_cpu.py builds
STEP_MEANS = [("sm_2", 1, 2, "denorm", None, None), ("sm_2_only_a", 1, 2, "denorm", None, ["a"]),
              ("sm_5_norm", 1, 5, "norm", None, None), ("sm_5_norm_names", 1, 5, "norm", ["a"], ["b"]),
              ("sm_2_ic2", 2, 2, "denorm", None, None)]
ENSEMBLES = [("en_2", 1, 2, "denorm", None, None), ("en_5_norm", 1, 5, "norm", None, None),
             ("en_5_norm_names", 1, 5, "norm", ["a"], None), ("en_2_ic2", 2, 2, "denorm", None, None)]


def load():
    ref_loader.load_stepper_ref()
    ref = os.path.join(ref_loader.REF, "fme", "ace", "aggregator")
    for name, path in (("fme.ace.aggregator", ref), ("fme.ace.aggregator.inference", os.path.join(ref, "inference")),
                       ("fme.ace.aggregator.one_step", os.path.join(ref, "one_step"))):
        ref_loader._ns(name, path)
    permissive = type(sys.modules["xarray"])
    for name in ("fme.ace.aggregator.plotting", "fme.ace.aggregator.inference.build_context", "fme.ace.aggregator.inference.data",
                 "fme.ace.aggregator.one_step.build_context"):
        sys.modules[name] = permissive(name)
    sys.modules["fme.core.distributed"].Distributed.reduce_mean = lambda self, t: t
    return types.SimpleNamespace(
        ensemble=importlib.import_module("fme.ace.aggregator.one_step.ensemble"),
        reduced=importlib.import_module("fme.ace.aggregator.one_step.reduced"),
        tensors=importlib.import_module("fme.core.tensors"),
        ops=importlib.import_module("fme.core.gridded_ops"),
        normalizer=importlib.import_module("fme.core.normalizer"))


def plain(v):
    return float(v) if not isinstance(v, torch.Tensor) or v.dim() == 0 else v.detach().cpu()


def run(R, dtype):
    torch.set_default_dtype(dtype)
    try:
        out = {}
        norm = R.normalizer.StandardNormalizer(means={k: torch.tensor(v, dtype=dtype) for k, v in C.MEANS.items()},
                                               stds={k: torch.tensor(v, dtype=dtype) for k, v in C.STDS.items()})
        for n_ic_steps in (1, 2):
            c = C.case(n_ic_steps)
            ops = R.ops.LatLonOperations(c["info"].area_weights.to(dtype))
            windows = [({n: v.to(dtype) for n, v in g.items()}, {n: v.to(dtype) for n, v in t.items()}, i0) for g, t, i0 in c["windows"]]
            for key, n_ic, step, target, names, variables in STEP_MEANS:
                if n_ic != n_ic_steps:
                    continue
                is_norm = target == "norm"
                agg = R.reduced.MeanAggregator(ops, target_time=step + n_ic_steps - 1, target=target, log_loss=False,
                                               include_bias=not is_norm, include_grad_mag_percent_diff=not is_norm,
                                               channel_mean_names=names if is_norm else None, report_variables=variables)
                for g, t, i0 in windows:
                    agg.record_batch(target_data=t, gen_data=g, target_data_norm=norm.normalize(t), gen_data_norm=norm.normalize(g),
                                     i_time_start=i0)
                out[key] = {k: plain(v) for k, v in agg.get_logs("x").items()}
            for key, n_ic, step, target, names, variables in ENSEMBLES:
                if n_ic != n_ic_steps:
                    continue
                agg = R.ensemble.get_one_step_ensemble_aggregator(ops, target_time=step, log_mean_maps=False, target=target,
                                                                  channel_mean_names=names if target == "norm" else None)
                unfold = lambda d: R.tensors.unfold_ensemble_dim(dict(d), C.E)      # noqa: E731
                for g, t, i0 in windows:
                    agg.record_batch(target_data=unfold(t), gen_data=unfold(g), target_data_norm=unfold(norm.normalize(t)),
                                     gen_data_norm=unfold(norm.normalize(g)), i_time_start=i0)
                logs = {k: plain(torch.as_tensor(v)) for k, v in agg.get_logs("x").items()}
                for metric, per in agg._aggregator._variable_metrics.items():
                    for name, m in per.items():
                        logs[f"x/{metric}/mean_map/{name}"] = m.get().detach().cpu()
                out[key] = logs
        return out
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    R = load()
    out = {"checksum": {n: C.checksum(C.case(n)) for n in (1, 2)}, "f32": run(R, torch.float32), "f64": run(R, torch.float64)}
    dst = os.path.join(HERE, "gen_ensemble.pt")
    torch.save(out, dst)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
