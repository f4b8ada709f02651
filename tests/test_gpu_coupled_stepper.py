"""The coupled stepper on the device: the tiny pair of tests/_coupled.py (the shipped name layout in small) loaded by
``load_coupled_stepper`` and run over 2 coupled steps with n_inner = 3, the fused exchange (csrc/coupler.hip) against the torch
ops of ``Coupler(fused=False)`` on the same device."""
import pytest
import torch

import ace_amd
from ace_amd import coupled
from _coupled import A_DIAG, H, N_INNER, N_OUTER, STATS, W, coupled_checkpoint, coupled_data, same, with_cpu_networks
from _util import rel_max

pytestmark = pytest.mark.gpu

# The exchanged means differ between the two paths by rounding only.  Against the fp64 mean m64 the kernel's is within
# 2^-23 |m64| + 2^-50 sum|x| and the reference's fp32 mean within n_inner 2^-24 mean|x| (tests/test_gpu_coupler_kernels.py), so for
# fields of one sign (|m64| = mean|x|) the two means differ by at most (2 + n_inner) 2^-24 relative to the field's magnitude.
MEAN_BOUND = (2 + N_INNER) * 2.0 ** -24
# One ocean step turns that into a difference of its outputs: the normaliser divides by the standard deviation, which scales a
# difference relative to the field's magnitude by |mean| / std - at most 330 / 20 = 16.5 among the exchanged fields (DLWRFsfc) - and
# the network, the corrector's global budgets and the de-normalisation are allowed a further factor of 8.
OCEAN_STEP_FACTOR = 16.5 * 8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def runs(dev):
    """the fused and the torch-path rollout of one stepper, with what went through the coupler in the fused one"""
    stepper = ace_amd.load_coupled_stepper(coupled_checkpoint(), device=dev)
    ic, forcing = coupled_data()
    to = lambda d: {realm: {k: v.to(dev) for k, v in fields.items()} for realm, fields in d.items()}
    ic, forcing = to(ic), to(forcing)
    coupler = stepper.coupler
    assert coupler.fused and coupler.launches() == 0
    seen = {"o2a": [], "a2o": []}
    o2a, a2o = coupler.atmosphere_forcings, coupler.ocean_forcings

    def record_o2a(window, ocean_state, atmos_ic):
        out = o2a(window, ocean_state, atmos_ic)
        seen["o2a"].append(((window, ocean_state, atmos_ic), out))
        return out

    def record_a2o(ocean_window, steps, window):
        out = a2o(ocean_window, steps, window)
        seen["a2o"].append(((ocean_window, steps, window), out))
        return out

    coupler.atmosphere_forcings, coupler.ocean_forcings = record_o2a, record_a2o
    fused, fused_state = stepper.predict(ic, forcing)
    launches = coupler.launches()
    del coupler.atmosphere_forcings, coupler.ocean_forcings
    coupler.fused = False
    plain, plain_state = stepper.predict(ic, forcing)
    assert coupler.launches() == launches                    # the torch path makes no native call
    coupler.fused = True
    torch.cuda.synchronize()
    return dict(stepper=stepper, ic=ic, forcing=forcing, seen=seen, fused=fused, fused_state=fused_state, plain=plain,
                plain_state=plain_state, launches=launches)


def test_two_native_calls_per_coupled_step(runs):
    assert runs["launches"] == 2 * N_OUTER
    assert len(runs["seen"]["o2a"]) == N_OUTER and len(runs["seen"]["a2o"]) == N_OUTER
    assert runs["stepper"].coupler.route(runs["ic"]["ocean"]["sst"]) == "fused"


def test_ocean_to_atmosphere_products_are_bitwise_the_torch_paths(runs):
    """what the fused rollout's coupler produced, recomputed by the torch path from the very same inputs, at every coupled step"""
    stepper = runs["stepper"]
    plain = coupled.Coupler(stepper.config, stepper.training_dataset_info.ocean_spatial_mask_provider,
                            stepper.atmosphere._step_obj._ocean.prescriber, (H, W), fused=False)
    for i, ((window, ocean_state, atmos_ic), (forcings, new_ic)) in enumerate(runs["seen"]["o2a"]):
        want, want_ic = plain.atmosphere_forcings(window, ocean_state, atmos_ic)
        assert set(forcings) == set(want) >= {"surface_temperature", "ocean_fraction", "sea_ice_fraction", "ocean_sea_ice_fraction"}
        for k, v in want.items():
            assert same(forcings[k], v), (i, k)
        assert set(new_ic) == set(want_ic)
        for k, v in want_ic.items():
            assert same(new_ic[k], v), (i, k)
        assert getattr(new_ic, "stepper_state", None) is getattr(atmos_ic, "stepper_state", None)
    assert plain.launches() == 0
    # the means of the same inputs: [NaN, mean] / [mean, NaN] as the torch path lays them out, the numbers within the derived bounds
    for i, ((ocean_window, steps, window), forcings) in enumerate(runs["seen"]["a2o"]):
        want = plain.ocean_forcings(ocean_window, steps, window)
        assert set(forcings) == set(want) >= {"hfds", "DLWRFsfc", "land_fraction", "DSWRFtoa", "hfgeou"}
        for k, v in want.items():
            if k == "hfgeou":
                assert forcings[k] is ocean_window[k]
                continue
            assert torch.equal(torch.isnan(forcings[k]), torch.isnan(v)), (i, k)
            x = torch.stack([s[k] for s in steps] if k in A_DIAG else [window[k][:, 1 + t] for t in range(N_INNER)], dim=1).double()
            bound = (2.0 ** -23 * x.mean(1).abs() + 2.0 ** -50 * x.abs().sum(1) + N_INNER * 2.0 ** -24 * x.abs().mean(1)).unsqueeze(1)
            slot = 1 if k in ("hfds", "DLWRFsfc", "land_fraction") else 0
            err = (forcings[k][:, slot:slot + 1].double() - v[:, slot:slot + 1].double()).abs()
            assert bool((err <= bound).all()), (i, k, float((err / bound).max()))


def test_fused_rollout_matches_the_torch_path_rollout(runs, dev):
    """Measured on an MI355X: kernel rounding (below) 3.99e-7; the fused rollout from the torch-path one 4.1e-7 (ocean) and 5.9e-7
    (atmosphere) after one ocean step and 3.0e-6 (ocean) after two, against allowances of 4.0e-5 and 7.9e-5 (per step and field;
    over whole rollouts 1.8e-6 / 5.5e-7: profiles/coupler_bench.json, "tiny_pair").

    Until the first ocean step both rollouts compute the same bits (the ocean -> atmosphere products are bitwise equal).  From there
    on they differ by the rounding of the exchanged means, MEAN_BOUND relative to a field's magnitude, carried through the ocean step
    (OCEAN_STEP_FACTOR) and, in the second coupled step, through what the first one's difference has become.  The allowance is the
    kernel-rounding figure plus OCEAN_STEP_FACTOR * MEAN_BOUND per coupled step taken.  The kernel-rounding figure is the largest
    relative difference of the torch-path device run from a CPU run of the same stepper; neither network has a CPU evaluation in
    this repository, the SFNO has the CPU oracle (oracle/sfno.py), so it is measured on the atmosphere's first n_inner steps,
    which no ocean step has touched yet (and which read the CPU coupler's exchange of the same initial state)."""
    fused, plain = runs["fused"], runs["plain"]
    for k in plain["atmosphere"]:
        assert same(fused["atmosphere"][k][:, :N_INNER], plain["atmosphere"][k][:, :N_INNER]), k
    # the kernel-rounding figure
    cpu = with_cpu_networks(ace_amd.load_coupled_stepper(coupled_checkpoint(), device="cpu"))
    ic, forcing = coupled_data()
    with torch.no_grad():
        steps = [p for p, _ in zip(cpu.predict_generator(ic, forcing), range(N_INNER))]
    figure = max(rel_max(plain["atmosphere"][k][:, t], steps[t].data[k]) for k in steps[0].data for t in range(N_INNER))
    print(f"kernel rounding (device torch-path run vs CPU oracle, atmosphere steps 0..{N_INNER - 1}): {figure:.3e}")
    assert figure <= N_INNER * 1e-5                                       # the per-step parity bar of the network tests, per step taken
    worst = {}
    for realm, first_ocean_step in (("ocean", 0), ("atmosphere", N_INNER)):
        for k, want in plain[realm].items():
            for t in range(first_ocean_step, want.shape[1]):
                n_ocean_steps = t + 1 if realm == "ocean" else t // N_INNER
                a, b = fused[realm][k][:, t], want[:, t]
                assert torch.equal(torch.isnan(a), torch.isnan(b)), (realm, k, t)
                diff = rel_max(a.nan_to_num(), b.nan_to_num())
                worst[(realm, n_ocean_steps)] = max(worst.get((realm, n_ocean_steps), 0.0), diff)
                allowed = figure + n_ocean_steps * OCEAN_STEP_FACTOR * MEAN_BOUND
                assert diff <= allowed, (realm, k, t, diff, allowed)
    for key, value in sorted(worst.items()):
        print(f"fused vs torch path, {key[0]} after {key[1]} ocean step(s): {value:.3e} "
              f"(allowed {figure + key[1] * OCEAN_STEP_FACTOR * MEAN_BOUND:.3e})")


def test_the_returned_state_chains(runs):
    stepper, ic, forcing = runs["stepper"], runs["ic"], runs["forcing"]
    first = {"atmosphere": {k: v[:, :N_INNER + 1] for k, v in forcing["atmosphere"].items()},
             "ocean": {k: v[:, :2] for k, v in forcing["ocean"].items()}}
    second = {"atmosphere": {k: v[:, N_INNER:] for k, v in forcing["atmosphere"].items()},
              "ocean": {k: v[:, 1:] for k, v in forcing["ocean"].items()}}
    a, state = stepper.predict(ic, first)
    b, end = stepper.predict(state, second)
    for realm in ("atmosphere", "ocean"):
        for k, v in runs["fused"][realm].items():
            assert same(torch.cat([a[realm][k], b[realm][k]], dim=1), v), (realm, k)
        for k, v in runs["fused_state"][realm].items():
            assert same(end[realm][k], v), (realm, k)
    assert stepper.coupler.launches() == runs["launches"] + 2 * N_OUTER
    assert STATS["DLWRFsfc"][0] / STATS["DLWRFsfc"][1] == 16.5           # the factor OCEAN_STEP_FACTOR states
