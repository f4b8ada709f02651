"""tests/golden/gen_gmr.pt from the REAL reference stepper (oracle/ref_loader.load_stepper_ref - build container only): the small
SphericalFourierNeuralOperatorNet stepper of make_golden_step_options.py (8 x 16, B = 2, T = 3) with ``global_mean_removal``
(fme/core/step/global_mean_removal.py) in three configurations - its ``get_state()``, the inputs, and the reference's own
``predict_generator`` output of every step, on CPU:
  "shared"       kind shared: the reference field a prognostic input; field_names hold a prognostic, an output-only diagnostic and
                 a name that is neither; append_as_input; residual_prediction
  "per_channel"  kind per_channel over all inputs (field_names None); append_as_input
  "subset"       kind per_channel over an explicit subset (a prognostic and a forcing), no synthetic channels, with a corrector
                 (force_positive_names) and a prescribed-SST ocean behind it
The temperature-like fields sit near 288 / 250 with a few units of spread and a different offset per sample, so a removed mean
matters.  Data only."""
import datetime
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402

B, H, W, T = 2, 8, 16, 3
FORCING = ["co2", "f0", "ofrac"]
PROGNOSTIC = ["Ts", "T_1"]
DIAGNOSTIC = ["TMP2m", "h_3"]
# (centre, spread, per-sample offset) of the generated fields; (mean, std) of the normalisation
FIELD = {"co2": (2.0, 1.0, 0.0), "f0": (0.0, 1.0, 0.5), "ofrac": (0.5, 0.3, 0.0), "Ts": (288.0, 3.0, 2.5), "T_1": (250.0, 4.0, -1.5)}
STATS = {"co2": (2.1, 1.2), "f0": (0.1, 1.1), "ofrac": (0.5, 0.3), "Ts": (287.0, 5.0), "T_1": (251.0, 6.0), "TMP2m": (286.0, 4.0),
         "h_3": (5.0, 2.0)}


def plain(o):
    if isinstance(o, dict):
        return {k: plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [plain(v) for v in o]
    if isinstance(o, torch.Tensor):
        return o.detach().clone()
    assert o is None or isinstance(o, (bool, int, float, str)), type(o)
    return o


def field(g, name, nt):
    centre, spread, offset = FIELD[name]
    x = centre + spread * torch.randn(B, nt, H, W, generator=g) + offset * torch.tensor([1.0, -1.0]).view(B, 1, 1, 1)
    return x.clamp(0.0, 1.0) if name == "ofrac" else x


CASES = {
    "shared": dict(residual_prediction=True,
                   global_mean_removal={"kind": "shared", "reference_field": "Ts", "field_names": ["T_1", "TMP2m", "nowhere", "Ts"],
                                        "append_as_input": True}),
    "per_channel": dict(global_mean_removal={"kind": "per_channel", "field_names": None, "append_as_input": True}),
    "subset": dict(global_mean_removal={"kind": "per_channel", "field_names": ["Ts", "f0"], "append_as_input": False},
                   ocean={"surface_temperature_name": "Ts", "ocean_fraction_name": "ofrac"},
                   corrector={"type": "atmosphere_corrector", "config": {"force_positive_names": ["h_3"]}}),
}


def main():
    ref = ref_loader.load_stepper_ref()
    info = ref.DatasetInfo(horizontal_coordinates=ref.LatLonCoordinates(lat=torch.linspace(-78.75, 78.75, H),
                                                                       lon=torch.arange(float(W)) * (360.0 / W)),
                           vertical_coordinate=ref.HybridSigmaPressureCoordinate(ak=torch.tensor([100.0, 8000.0, 0.0]),
                                                                                 bk=torch.tensor([0.0, 0.3, 1.0])),
                           timestep=datetime.timedelta(hours=6))
    out = {}
    for seed, (case, options) in enumerate(CASES.items()):
        step = {"type": "single_module", "config": dict(
            builder={"type": "SphericalFourierNeuralOperatorNet",
                     "config": {"embed_dim": 12, "num_layers": 2, "operator_type": "dhconv", "data_grid": "legendre-gauss"}},
            in_names=FORCING + PROGNOSTIC, out_names=PROGNOSTIC + DIAGNOSTIC,
            normalization={"network": {"means": {n: m for n, (m, _) in STATS.items()}, "stds": {n: s for n, (_, s) in STATS.items()}}},
            **options)}
        torch.manual_seed(seed)
        stepper = ref.StepperConfig.from_stepper_state({"config": {"step": step}}).get_stepper(dataset_info=info)
        with torch.no_grad():       # the reference's zero-initialised biases / unit norm weights: make them non-trivial
            g = torch.Generator().manual_seed(10 + seed)
            for p in stepper.modules.parameters():
                if p.ndim <= 1 or p.abs().max() == 0:
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
        g = torch.Generator().manual_seed(20 + seed)
        ic = {n: field(g, n, 1) for n in PROGNOSTIC}
        forcing = {n: field(g, n, T + 1) for n in FORCING}
        if "ocean" in options:
            forcing["Ts"] = field(g, "Ts", T + 1)          # the ocean's prescribed SST target
        steps = []
        with torch.no_grad():
            for res in stepper.predict_generator(ic, forcing, T, ref.NullOptimization(), labels=None):
                steps.append({k: v.clone() for k, v in res.output.items()})
        for k in steps[0]:
            assert all(torch.isfinite(s[k]).all() for s in steps), (case, k)
        print(case, "outputs", sorted(steps[0]), "| Ts sample means of the last step", steps[-1]["Ts"].mean(dim=(1, 2)).tolist())
        out[case] = {"state": plain(stepper.get_state()), "ic": ic, "forcing": forcing, "steps": steps}
    path = os.path.join(HERE, "gen_gmr.pt")
    torch.save(out, path)
    torch.load(path, weights_only=True)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
