"""tests/golden/gen_step_diagnostics.pt from the REAL reference (imported through oracle/ref_loader's stubs; build container only):

  "corrector"  for each of make_golden_corrector.py's nine corrector configurations on its synthetic atmosphere (2 samples, 8 x 16,
               4 layers): the reference's ``diagnostics.delta`` (keys and values) of two chained steps;
  "rollout"    a 3-step rollout of the reference ``Stepper`` (the 16-wide 2-layer SFNO of make_golden_checkpoint.py) with the
               ace2_like corrector, a prescribed-SST ocean and one prescribed prognostic name: its state, inputs, outputs and
               ``step_diagnostics.delta``;
  "aggregator" the outputs of the reference's CorrectionDeltaAggregator / CorrectionDeltaTimeMeanAggregator /
               CorrectionDeltaMeanAggregator over two windows of deltas (the second at a non-zero ``i_time_start``), scalars, maps
               and series: once in fp32 as the reference runs ("fp32"), and once with the fp32-formed ``delta / std`` cast to float64
               and fed to the same classes over the same area weights widened to float64 ("fp64").

Data only: plain dicts / lists / numbers / tensors."""
import datetime
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from oracle import ref_loader  # noqa: E402

import make_golden_checkpoint as ck  # noqa: E402
import make_golden_corrector as mc  # noqa: E402


def corrector_deltas():
    ref = ref_loader.load_corrector()
    lat = torch.linspace(-78.75, 78.75, 8)
    lon = torch.arange(16.0) * 22.5
    vc = ref.HybridSigmaPressureCoordinate(ak=torch.tensor([100.0, 5000.0, 12000.0, 6000.0, 0.0]),
                                           bk=torch.tensor([0.0, 0.05, 0.35, 0.75, 1.0]))
    ops = ref.LatLonCoordinates(lat=lat, lon=lon).get_gridded_operations()
    timestep = datetime.timedelta(hours=6)
    inp0, gen0, gen1 = mc.synthetic(1), mc.synthetic(2), mc.synthetic(3)
    forcing = {"DSWRFtoa": mc.synthetic(4)["DSWRFtoa"], "HGTsfc": inp0["HGTsfc"]}
    for d in (gen0, gen1):
        del d["DSWRFtoa"], d["HGTsfc"]
    inp0 = {**inp0, **forcing}
    out = {}
    for name, kw in mc.CONFIGS.items():
        kw = dict(kw)
        if "total_energy_budget_correction" in kw:
            kw["total_energy_budget_correction"] = ref.EnergyBudgetConfig(**kw["total_energy_budget_correction"])
        corrector = ref.AtmosphereCorrectorConfig(**kw)._build(ops, vc, timestep)
        r0 = corrector(inp0, gen0, forcing, None)
        r1 = corrector({**r0.corrected, **forcing}, gen1, forcing, r0.corrector_state)
        out[name] = {"step0": {k: v.clone() for k, v in r0.diagnostics.delta.items()},
                     "step1": {k: v.clone() for k, v in r1.diagnostics.delta.items()}}
        print(f"{name}: delta keys {list(out[name]['step0'])}")
    return out


def rollout():
    ref = ref_loader.load_stepper_ref()
    H, W, B, T, NZ = ck.H, ck.W, ck.B, ck.T, ck.NZ
    lat = torch.linspace(-78.75, 78.75, H)
    lon = torch.arange(float(W)) * (360.0 / W)
    info = ref.DatasetInfo(
        horizontal_coordinates=ref.LatLonCoordinates(lat=lat, lon=lon),
        vertical_coordinate=ref.HybridSigmaPressureCoordinate(ak=torch.tensor([100.0, 8000.0, 0.0]), bk=torch.tensor([0.0, 0.3, 1.0])),
        timestep=datetime.timedelta(hours=6))
    sfno = {"type": "SphericalFourierNeuralOperatorNet",
            "config": {"embed_dim": 16, "num_layers": 2, "operator_type": "dhconv", "scale_factor": 1,
                       "filter_type": "linear", "data_grid": "legendre-gauss"}}
    prescribed = "specific_total_water_1"
    cfg = {"step": ck.step_config(
        sfno, next_step_forcing_names=["DSWRFtoa"], prescribed_prognostic_names=[prescribed],
        ocean={"surface_temperature_name": "surface_temperature", "ocean_fraction_name": "ocean_fraction"},
        corrector={"type": "atmosphere_corrector", "config": {
            "conserve_dry_air": True, "moisture_budget_correction": "advection_and_precipitation",
            "force_positive_names": ["PRATEsfc"] + [f"specific_total_water_{k}" for k in range(NZ)],
            "total_energy_budget_correction": {"method": "constant_temperature", "constant_unaccounted_heating": 0.1}}})}
    torch.manual_seed(0)
    stepper = ref.StepperConfig.from_stepper_state({"config": cfg}).get_stepper(dataset_info=info)
    with torch.no_grad():
        g = torch.Generator().manual_seed(1)
        for p in stepper.modules.parameters():
            if p.ndim <= 1 or p.abs().max() == 0:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    g = torch.Generator().manual_seed(2)
    ic = {n: ck.field(g, n, B, 1) for n in ck.PROGNOSTIC}
    forcing = {n: ck.field(g, n, B, T + 1) for n in ck.FORCING}
    forcing["HGTsfc"] = forcing["HGTsfc"][:, :1].expand(B, T + 1, H, W).clone()
    forcing["surface_temperature"] = ck.field(g, "surface_temperature", B, T + 1)
    forcing[prescribed] = ck.field(g, prescribed, B, T + 1)
    steps, deltas = [], []
    with torch.no_grad():
        for res in stepper.predict_generator(ic, forcing, T, ref.NullOptimization(), labels=None):
            steps.append({k: v.clone() for k, v in res.output.items()})
            deltas.append({k: v.clone() for k, v in res.corrector_diagnostics.delta.items()})
    delta = {k: torch.stack([d[k] for d in deltas], dim=1) for k in deltas[0]}
    print("rollout: delta keys", sorted(delta))
    assert prescribed not in delta
    stds = {n: 0.2 * ck.SCALES[n][1] for n in delta}
    return {"state": ck.plain(stepper.get_state()), "ic": ic, "forcing": forcing, "steps": steps, "delta": delta,
            "prescribed": prescribed, "stds": stds}, lat, lon


def aggregators(delta, stds, lat, lon):
    ref_loader.load_stepper_ref()
    root = os.path.join(ref_loader.REF, "fme", "ace", "aggregator")
    for name, path in (("fme.ace.aggregator", root), ("fme.ace.aggregator.inference", os.path.join(root, "inference"))):
        if name not in sys.modules:
            ref_loader._ns(name, path)
    permissive = type(sys.modules["xarray"])
    for name in ("fme.ace.aggregator.plotting", "fme.core.wandb"):
        if name not in sys.modules:
            sys.modules[name] = permissive(name)
    sys.modules["fme.core.distributed"].Distributed.reduce_mean = lambda self, t: t      # non-distributed: the tensor itself
    sd = importlib.import_module("fme.ace.aggregator.inference.step_diagnostics")
    sd_core = importlib.import_module("fme.core.step.step_diagnostics")
    coords = importlib.import_module("fme.core.coordinates")
    ops32 = coords.LatLonCoordinates(lat=lat, lon=lon).get_gridded_operations()
    # two windows: steps [0, 2) of the rollout's deltas at i_time_start = 1, the last step at i_time_start = 3, of n_timesteps = 5
    windows = [({k: v[:, :2] for k, v in delta.items()}, 1), ({k: v[:, 2:] for k, v in delta.items()}, 3)]
    n_timesteps = 5
    std_t = {k: torch.tensor(v, dtype=torch.float) for k, v in stds.items()}

    def run(dtype):
        # float64: the same fp32 area weights, widened, so that every operation behind the quotient is float64
        ops = ops32 if dtype == torch.float32 else type(ops32)(ops32._cpu_area_global.to(dtype))

        def normalize(d, apply_mean=True):
            assert not apply_mean
            return {k: (v / std_t[k]).to(dtype) for k, v in d.items()}      # the fp32-formed quotient, then the cast
        time_mean = sd.CorrectionDeltaTimeMeanAggregator(gridded_operations=ops, record_scalars=True, record_maps=True)
        series = sd.CorrectionDeltaMeanAggregator(gridded_operations=ops, n_timesteps=n_timesteps)
        agg = sd.CorrectionDeltaAggregator(normalize=normalize, time_mean=time_mean, time_series=series)
        for d, i0 in windows:
            agg.record_batch(sd_core.StepDiagnostics(delta=d), i0)
        signed, magnitude = time_mean._get_time_means()
        scalars = {n: ops.area_weighted_mean(magnitude[n], name=n).clone() for n in signed}
        ser = {m: {n: v.clone() for n, v in metric.get().items()} for m, metric in series._variable_metrics.items()}
        return {"signed": {n: v.clone() for n, v in signed.items()}, "magnitude": {n: v.clone() for n, v in magnitude.items()},
                "correction_magnitude": scalars, "series": ser,
                "signed_sum": {n: v.clone() for n, v in time_mean._signed_sum.items()},
                "magnitude_sum": {n: v.clone() for n, v in time_mean._magnitude_sum.items()}}

    return {"area_weights": ops32._cpu_area_global.clone(), "i_time_start": [1, 3], "n_timesteps": n_timesteps, "fp32": run(torch.float32), "fp64": run(torch.float64)}


def main():
    out = {"corrector": corrector_deltas()}
    out["rollout"], lat, lon = rollout()
    out["aggregator"] = aggregators(out["rollout"]["delta"], out["rollout"]["stds"], lat, lon)
    path = os.path.join(HERE, "gen_step_diagnostics.pt")
    torch.save(out, path)
    torch.load(path, weights_only=True)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
