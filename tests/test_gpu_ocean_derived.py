"""The fused path of ace_amd/ocean_derived_variables.py (one ace_ocean_derive_window per window) on the device: against the
reference's outputs on the golden cases and against the torch path (``fused=False``) within the bars of
tests/test_ocean_derive_ref_cpu.py, bitwise where the contract is bitwise; through ``Stepper.predict``, ``EnginePredict`` and its
``derive_target``, and the coupled stepper; and bitwise reproducible."""
import os

import pytest
import torch

from ace_amd import ocean_derived_variables as ODV
import _ocean_derive_cases as C
from _coupled import coupled_checkpoint, coupled_data, same
from test_ocean_derive_ref_cpu import check_against_reference, flat
from test_ocean_derived_cpu import OHC, TEND, derive_fn

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ADV = "implied_tendency_of_ocean_heat_content_due_to_advection"
BITWISE = ("net_energy_flux_into_ocean_column", "sea_ice_fraction", "hfds")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(os.path.join(golden_dir, "gen_ocean_derived.pt"), weights_only=False)


def to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_against_the_reference_and_the_torch_path(dev, gold, name):
    rec = gold["cases"][name]
    data, forcing = to(rec["data"], dev), to(rec["forcing"], dev)
    fused, plain = derive_fn(rec, name, fused=True), derive_fn(rec, name, fused=False)
    out, ref = fused(data, forcing), plain(data, forcing)
    assert fused.launches == 1 and plain.launches == 0
    assert list(out) == list(ref) == list(rec["data"]) + [n for n in C.OUTPUTS if n in C.CASES[name]["derived"]]
    for k in rec["data"]:
        assert out[k] is data[k]
    new = {n: flat(out[n].cpu()) for n in out if n not in rec["data"]}
    check_against_reference(rec, new, gold["timestep_seconds"], name)                                  # the reference's own outputs
    check_against_reference(rec, new, gold["timestep_seconds"], name + " / torch path on the device",
                            expected={n: ref[n].cpu() for n in new})
    for n in BITWISE:
        if n in new:
            assert same(out[n], ref[n]), n
    assert derive_fn(rec, name, fused=None)(data, forcing).keys() == out.keys()                          # None: fused on the device


def test_window_reads_the_initial_condition_where_it_lies(dev, gold):
    rec = gold["cases"]["all_seven"]
    fn = derive_fn(rec, "all_seven", fused=True)
    series, forcing = to(rec["data"], dev), to(rec["forcing"], dev)
    ic = {k: v[:, :1] for k, v in series.items() if k != "thetao_2"}           # a level the initial condition does not hold
    data = {k: v[:, 1:] for k, v in series.items()}
    got = fn.window(data, ic, forcing, 1, C.T - 1)
    assert fn.launches == 1 and list(got) == list(rec["data"]) + list(C.OUTPUTS)
    whole = fn({**series, "thetao_2": torch.cat([torch.full_like(series["thetao_2"][:, :1], float("nan")), data["thetao_2"]], 1)},
               forcing)
    for n in C.OUTPUTS:                                                        # the same sums in the same order: the same bits
        assert got[n].shape[1] == C.T - 1 and same(got[n], whole[n][:, 1:]), n
    # against the concatenation path (what ``window`` is on the torch path): the heat budget within the bars, the rest bitwise
    torch_fn = derive_fn(rec, "all_seven", fused=False)
    plain = torch_fn.window(data, ic, forcing, 1, C.T - 1)
    assert list(plain) == list(got) and torch_fn.launches == 0
    for n in BITWISE:
        assert same(got[n], plain[n]), n
    dz, dt = rec["dz"].to(dev), gold["timestep_seconds"]
    th = torch.stack([series[n] for n in C.THETAO], dim=-1).clone()
    th[:, 0, :, :, 2] = float("nan")
    _budget_close(got, plain, th, dz, dt)
    # a thetao level that is a forcing field: its head is the forcing's time level n_ic - 1, as in the concatenated window
    moved = {**forcing, "thetao_3": series["thetao_3"]}
    less = {k: v for k, v in data.items() if k != "thetao_3"}
    a = fn.window(less, ic, moved, 1, C.T - 1)
    b = torch_fn.window(less, ic, moved, 1, C.T - 1)
    assert list(a) == list(b) and "thetao_3" not in a and OHC in a
    _budget_close(a, b, th, dz, dt)
    # a derived name that the forcing holds is left out, as the concatenation path leaves it out
    held = {**forcing, OHC: series["thetao_0"]}
    a, b = fn.window(data, ic, held, 1, C.T - 1), torch_fn.window(data, ic, held, 1, C.T - 1)
    assert list(a) == list(b) and OHC not in a and TEND in a
    assert same(a[TEND], got[TEND])
    # every chunking of time gives the same bytes
    for t_chunk in (1, 3):
        fn.t_chunk = t_chunk
        again = fn.window(data, ic, forcing, 1, C.T - 1)
        for n in C.OUTPUTS:
            assert same(again[n], got[n]), (t_chunk, n)
    fn.t_chunk = 0


def test_without_a_choice_only_what_the_launch_takes_is_fused(dev, gold):
    """``fused=None``: float64 fields, or a forcing on another device, take the torch path instead of raising"""
    rec = gold["cases"]["budget_hfds_ssf_geo"]
    fn = derive_fn(rec, "budget_hfds_ssf_geo", fused=None)
    data, forcing = to(rec["data"], dev), to(rec["forcing"], dev)
    out = fn({k: v.double() for k, v in data.items()}, forcing)
    assert fn.launches == 0 and out[OHC].dtype == torch.float64
    assert fn(data, forcing)[OHC].dtype == torch.float32 and fn.launches == 1
    fn.fused = True
    with pytest.raises(TypeError, match="float32"):
        fn({k: v.double() for k, v in data.items()}, forcing)


def test_two_calls_on_the_same_tensors_give_identical_bytes(dev, gold):
    rec = gold["cases"]["all_seven"]
    fn = derive_fn(rec, "all_seven", fused=True)
    data, forcing = to(rec["data"], dev), to(rec["forcing"], dev)
    a, b = fn(data, forcing), fn(data, forcing)
    for n in C.OUTPUTS:
        assert a[n].data_ptr() != b[n].data_ptr() and torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
    assert len(fn._plans) == 1 and len(fn._static) == 1                        # tables built once, not per window


def test_views_and_static_fields_are_read_in_place(dev, gold):
    """a forcing constant in time (an expanded view) and fields that are slices of a longer record"""
    rec = gold["cases"]["all_seven"]
    fn = derive_fn(rec, "all_seven", fused=True)
    data, forcing = to(rec["data"], dev), to(rec["forcing"], dev)
    forcing["land_fraction"] = forcing["land_fraction"][:, :1].expand(-1, C.T, -1, -1)
    longer = {k: torch.cat([v, v], dim=1) for k, v in data.items()}
    got = fn({k: v[:, 2:2 + C.T] for k, v in longer.items()}, forcing)
    want = fn({k: v[:, 2:2 + C.T].contiguous() for k, v in longer.items()}, {k: v.contiguous() for k, v in forcing.items()})
    for n in C.OUTPUTS:
        assert same(got[n], want[n]), n


def _budget_close(got, ref, thetao, dz, dt):
    """fused against torch path over a window of T steps: the bars of tests/test_ocean_derive_ref_cpu.py from the thetao series
    (B, 1 + T, H, W, L), the initial condition in front (one rounding in the fused path, L + 2 in the torch path)"""
    L = thetao.shape[-1]
    A = (thetao.double().abs().nan_to_num() * dz.double()).sum(-1) * 3992.0 * 1035.0
    ok = ~torch.isnan(ref[OHC])
    assert torch.equal(torch.isnan(got[OHC]), torch.isnan(ref[OHC])) and torch.equal(torch.isnan(got[TEND]), torch.isnan(ref[TEND]))
    assert bool(ok.any()) and bool(((got[OHC].double() - ref[OHC].double()).abs() <= (L + 3) * U * A[:, 1:])[ok].all())
    bar = (L + 3) * U * (A[:, 1:] + A[:, :-1]) / dt + 2 * U * ref[TEND].double().abs().nan_to_num()
    assert bool(((got[TEND].double() - ref[TEND].double()).abs() <= bar)[ok].all())
    if ADV in ref:                                         # the tendency's bar and one rounding of the difference on either side
        assert torch.equal(torch.isnan(got[ADV]), torch.isnan(ref[ADV]))
        bar = bar + 2 * U * ref[ADV].double().abs().nan_to_num()
        assert bool(((got[ADV].double() - ref[ADV].double()).abs() <= bar)[ok].all())


def test_through_stepper_predict_and_engine_predict(dev):
    from ace_amd.inference import EnginePredict
    from test_gpu_ocean_rollout import _predict_setup
    stepper, ic, forcing = _predict_setup(dev, 3)
    fn = stepper.derive_func
    assert isinstance(fn, ODV.OceanDeriveFn) and fn.fused is None
    plain, _ = stepper.predict(ic, forcing)
    out, _ = stepper.predict(ic, forcing, compute_derived_variables=True)
    assert fn.launches == 1
    new = set(out) - set(plain)
    assert {OHC, TEND, "net_energy_flux_into_ocean_column", "sea_ice_fraction"} <= new and new <= set(C.OUTPUTS)
    for k in plain:
        assert same(out[k], plain[k]), k
    fn.fused = False
    ref, _ = stepper.predict(ic, forcing, compute_derived_variables=True)
    fn.fused = None
    assert fn.launches == 1 and list(ref) == list(out)
    depth = stepper._dataset_info.ocean_vertical_coordinate
    dz = depth.dz.to(dev)
    # the window's fields with the initial condition in front: what the tendency's first step is taken against
    series = torch.stack([torch.cat([ic[f"thetao_{k}"], out[f"thetao_{k}"]], dim=1) for k in range(depth.nlev)], dim=-1)
    _budget_close(out, ref, series, dz, fn.timestep.total_seconds())
    for n in BITWISE:
        if n in new:
            assert same(out[n], ref[n]), n
    # the engine's predict function goes through the same derive function: one more launch, on the engine's own fields
    pred = EnginePredict(stepper, batch=2, graph=None)
    eng_out, _ = pred(ic, forcing, compute_derived_variables=True)
    assert fn.launches == 2 and set(eng_out) == set(out)
    again = fn.window({k: eng_out[k] for k in plain}, ic, forcing, 1, 3)
    for n in new:
        assert same(eng_out[n], again[n]), n
    # derive_target: every time level of a target window, the first tendency zero
    window = {**{k: torch.cat([ic[k], v], dim=1) for k, v in plain.items()}, **forcing}
    target = pred.derive_target(window, list(plain))
    assert fn.launches == 4 and OHC in target and not target[TEND][:, 0].any()
    assert same(target[OHC][:, 1:], out[OHC]) and same(target[TEND][:, 1:], out[TEND])


def test_through_the_coupled_stepper(dev):
    from ace_amd import coupled
    ckpt = coupled_checkpoint()
    ckpt["stepper"]["atmosphere_state"]["dataset_info"]["vertical_coordinate"] = {"ak": torch.tensor([0.0, 0.0]),
                                                                                  "bk": torch.tensor([0.0, 1.0])}
    stepper = coupled.load_coupled_stepper(ckpt, device=dev)
    ic, forcing = coupled_data()
    ic = {r: to(v, dev) for r, v in ic.items()}
    forcing = {r: to(v, dev) for r, v in forcing.items()}
    fn = stepper.ocean.derive_func
    out, _ = stepper.predict(ic, forcing, compute_derived_variables=True)
    assert fn.launches == 1 and {OHC, TEND} <= set(out["ocean"])
    fn.fused = False
    ref, _ = stepper.predict(ic, forcing, compute_derived_variables=True)
    assert fn.launches == 1 and list(ref["ocean"]) == list(out["ocean"])
    depth = stepper.ocean._dataset_info.ocean_vertical_coordinate
    series = torch.stack([torch.cat([ic["ocean"][f"thetao_{k}"], out["ocean"][f"thetao_{k}"]], dim=1) for k in range(depth.nlev)], dim=-1)
    _budget_close(out["ocean"], ref["ocean"], series, depth.dz.to(dev), fn.timestep.total_seconds())
    for k in out["atmosphere"]:
        assert same(out["atmosphere"][k], ref["atmosphere"][k]), k


def test_through_the_coupled_engine(dev):
    """``CoupledEnginePredict`` / ``CoupledRolloutEngine.predict`` derive both realms through the components' derive functions"""
    from ace_amd import coupled
    from ace_amd.coupled_rollout import CoupledEnginePredict
    from ace_amd.stepper import derive_over_window
    from _coupled import B, N_INNER, N_OUTER
    ckpt = coupled_checkpoint()
    ckpt["stepper"]["atmosphere_state"]["dataset_info"]["vertical_coordinate"] = {"ak": torch.tensor([0.0, 0.0]),
                                                                                  "bk": torch.tensor([0.0, 1.0])}
    stepper = coupled.load_coupled_stepper(ckpt, device=dev)
    ic, forcing = coupled_data()
    ic = {r: to(v, dev) for r, v in ic.items()}
    forcing = {r: to(v, dev) for r, v in forcing.items()}
    fn = stepper.ocean.derive_func
    predict = CoupledEnginePredict(stepper, B, graph="step")
    plain, _ = predict(ic, forcing)
    assert fn.launches == 0 and not {OHC, TEND} & set(plain["ocean"])
    out, state = predict(ic, forcing, compute_derived_variables=True)
    assert fn.launches == 1                                                     # one launch for the ocean's window
    assert {OHC, TEND} <= set(out["ocean"]) and out["ocean"][OHC].shape == plain["ocean"]["thetao_0"].shape
    for realm in ("atmosphere", "ocean"):
        assert set(plain[realm]) <= set(out[realm]) and set(state[realm]) == set(getattr(stepper, realm).prognostic_names)
        for k in plain[realm]:
            assert same(out[realm][k], plain[realm][k]), (realm, k)                 # the generated fields are untouched
    # the ocean's derived variables are the derive function's window on the engine's own fields
    again = fn.window(dict(plain["ocean"]), ic["ocean"], forcing["ocean"], 1, N_OUTER)
    assert fn.launches == 2 and list(again) == list(out["ocean"])
    for k in again:
        assert same(out["ocean"][k], again[k]), k
    # and the atmosphere's are its own derive function's, as before
    atmosphere = derive_over_window(stepper.atmosphere.derive_func, dict(plain["atmosphere"]), ic["atmosphere"], forcing["atmosphere"],
                                    1, N_OUTER * N_INNER)
    assert list(atmosphere) == list(out["atmosphere"])
    for k in atmosphere:
        assert same(out["atmosphere"][k], atmosphere[k]), k
    # against the torch path, within the bars
    fn.fused = False
    ref, _ = predict(ic, forcing, compute_derived_variables=True)
    assert fn.launches == 2 and list(ref["ocean"]) == list(out["ocean"])
    depth = stepper.ocean._dataset_info.ocean_vertical_coordinate
    series = torch.stack([torch.cat([ic["ocean"][f"thetao_{k}"], out["ocean"][f"thetao_{k}"]], dim=1) for k in range(depth.nlev)], dim=-1)
    _budget_close(out["ocean"], ref["ocean"], series, depth.dz.to(dev), fn.timestep.total_seconds())
