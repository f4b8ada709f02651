"""tests/golden/gen_video.pt from the reference's own ``VideoAggregator`` and ``_make_video``
(fme/ace/aggregator/inference/video.py:33-519), imported as make_golden_regress.py imports its modules (oracle/ref_loader's stubs,
the aggregator packages as bare namespaces, permissive stubs for build_context and data).  The stub distribution has no
reduce_mean / reduce_min / reduce_max, so the three recorders get identity ones, and the module's ``wandb`` is replaced by a
stand-in whose ``Video`` returns its arguments.

n_timesteps = 7 on a (5, 9) grid, B = 3, two names: "a" and "m", whose target is NaN at a fixed mask.  Windows (t0, T) = (1, 2),
(3, 3), (6, 1), each visited twice with fresh data; slot 0 is never visited.  Fields 280 + 15 randn, target = gen + 2 randn."""
import importlib
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402

N_TIME, H, W, B = 7, 5, 9, 3
WINDOWS = ((1, 2), (3, 3), (6, 1))
NAMES = ("a", "m")


def inputs():
    g = torch.Generator().manual_seed(11)
    mask = torch.rand(H, W, generator=g) < 0.25
    visits = []
    for _ in range(2):
        for t0, T in WINDOWS:
            gen = {n: (280.0 + 15.0 * torch.randn(B, T, H, W, generator=g)).float() for n in NAMES}
            tgt = {n: (gen[n] + 2.0 * torch.randn(B, T, H, W, generator=g)).float() for n in NAMES}
            tgt["m"][..., mask] = float("nan")
            visits.append((t0, gen, tgt))
    return mask, visits


class _Identity:
    reduce_mean = reduce_min = reduce_max = staticmethod(lambda t: t)


def main():
    ref_loader.load_stepper_ref()
    ref = os.path.join(ref_loader.REF, "fme", "ace", "aggregator")
    for name, path in (("fme.ace.aggregator", ref), ("fme.ace.aggregator.inference", os.path.join(ref, "inference"))):
        ref_loader._ns(name, path)
    permissive = type(sys.modules["xarray"])
    for name in ("fme.ace.aggregator.inference.build_context", "fme.ace.aggregator.inference.data"):
        sys.modules[name] = permissive(name)
    video = importlib.import_module("fme.ace.aggregator.inference.video")
    video.wandb = types.SimpleNamespace(Video=lambda data, **kw: (data, kw))

    mask, visits = inputs()
    agg = video.VideoAggregator(n_timesteps=N_TIME, enable_extended_videos=True)
    for part in (agg._mean_data, agg._error_data, agg._variance_data):
        part._dist = _Identity()
    for t0, gen, tgt in visits:
        agg.record_batch(types.SimpleNamespace(prediction=gen, target=tgt, i_time_start=t0))
    out = {"n_timesteps": N_TIME, "mask": mask, "visits": visits, "n_batches": agg._mean_data._n_batches.clone(),
           "acc": {"gen": agg._mean_data._gen_data, "target": agg._mean_data._target_data, "mse": agg._error_data._mse_data,
                   "min_err": agg._error_data._min_err_data, "max_err": agg._error_data._max_err_data,
                   "gen_sq": agg._variance_data._gen_squares, "target_sq": agg._variance_data._target_squares,
                   "var_gen": agg._variance_data._gen_means, "var_target": agg._variance_data._target_means}}
    data = agg._get_data()
    out["keys"] = list(data)
    out["data"] = {k: (d.gen, d.target) for k, d in data.items()}
    frames, kw = data["a"].make_video()
    alone, kw_alone = data["rmse/a"].make_video()
    masked, kw_masked = data["m"].make_video()
    out["make_video"] = {"a": (torch.from_numpy(frames.copy()), kw["caption"]), "rmse/a": (torch.from_numpy(alone.copy()), kw_alone["caption"]),
                         "m": (torch.from_numpy(masked.copy()), kw_masked["caption"])}
    dst = os.path.join(HERE, "gen_video.pt")
    torch.save(out, dst)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
