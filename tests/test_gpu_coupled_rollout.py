"""CoupledRolloutEngine on the device, on the tiny pair of tests/_coupled.py (16 x 32, B = 2, n_inner = 3, 2 coupled steps), in
every graph mode: bitwise against a composition of parts that do not contain it (the fused ``Coupler``, ``RolloutEngine`` and
``OceanRolloutEngine`` on one coupled step at a time), against ``CoupledStepper.predict`` at the project's parity bar, chained
windows, a repeated window, the route query, reloaded weights, and ``CoupledEnginePredict``."""
import pytest
import torch

import ace_amd
from ace_amd.coupled_rollout import CoupledEnginePredict, CoupledRolloutEngine
from _coupled import B, N_INNER, N_OUTER, coupled_checkpoint, coupled_data, same
from _util import rel_max

pytestmark = pytest.mark.gpu

GRAPHS = [None, "step", "window"]
PARITY = 1e-5             # the per-step parity bar of the network tests (BASELINE.json's north_star), per network step taken


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _to(d, dev):
    return {realm: {k: v.to(dev) for k, v in fields.items()} for realm, fields in d.items()}


def _windows(forcing, bounds):
    """the forcing records cut at coupled steps: bounds (0, 2, 3) -> the windows of coupled steps 0 .. 1 and 2"""
    return [{"atmosphere": {k: v[:, a * N_INNER:b * N_INNER + 1] for k, v in forcing["atmosphere"].items()},
             "ocean": {k: v[:, a:b + 1] for k, v in forcing["ocean"].items()}} for a, b in zip(bounds[:-1], bounds[1:])]


def _keep(data, state):
    """copies of an engine's outputs and state (the next window reuses its buffers)"""
    kept = {}
    for realm, s in state.items():
        kept[realm] = type(s)({k: v.clone() for k, v in s.items()})
        kept[realm].stepper_state = getattr(s, "stepper_state", None)
    return {realm: {k: v.clone() for k, v in fields.items()} for realm, fields in data.items()}, kept


def _keep1(out, state):
    data, kept = _keep({"x": out}, {"x": state})
    return data["x"], kept["x"]


def _same_stepper_state(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    ca, cb = getattr(a, "corrector_state", None), getattr(b, "corrector_state", None)
    if ca is None or cb is None:
        return ca is None and cb is None
    return same(ca.global_dry_air_mass.float(), cb.global_dry_air_mass.float())


def _assert_same_run(got, want, what):
    (data, state), (want_data, want_state) = got, want
    for realm in ("atmosphere", "ocean"):
        assert set(data[realm]) == set(want_data[realm]), (what, realm)
        for k, v in want_data[realm].items():
            assert same(data[realm][k], v), (what, realm, k)
        assert set(state[realm]) == set(want_state[realm]), (what, realm)
        for k, v in want_state[realm].items():
            assert same(state[realm][k], v), (what, "state", realm, k)
        assert _same_stepper_state(getattr(state[realm], "stepper_state", None), getattr(want_state[realm], "stepper_state", None)), \
            (what, "stepper_state", realm)


def _composition(stepper, ic, forcing, graph, n_outer):
    """the coupled window out of parts the parent commit has: per coupled step the fused ``Coupler.atmosphere_forcings``, a
    ``RolloutEngine`` window of n_inner steps, ``Coupler.ocean_forcings`` and an ``OceanRolloutEngine`` window of one step"""
    from ace_amd.ocean_rollout import OceanRolloutEngine
    from ace_amd.rollout import RolloutEngine
    coupler = stepper.coupler
    assert coupler.fused
    atmosphere = RolloutEngine(stepper.atmosphere, B, N_INNER, graph=graph)
    ocean = OceanRolloutEngine(stepper.ocean, B, 1, graph=graph)
    a_ic, o_ic = ic["atmosphere"], ic["ocean"]
    outs = {"atmosphere": [], "ocean": []}
    for i in range(n_outer):
        window = {k: v[:, i * N_INNER:(i + 1) * N_INNER + 1] for k, v in forcing["atmosphere"].items()}
        a_forcing, a_ic = coupler.atmosphere_forcings(window, o_ic, a_ic)
        a_out, a_ic = _keep1(*atmosphere.predict(a_ic, a_forcing))
        steps = [{k: v[:, t] for k, v in a_out.items()} for t in range(N_INNER)]
        o_forcing = coupler.ocean_forcings({k: v[:, i:i + 2] for k, v in forcing["ocean"].items()}, steps, window)
        o_out, o_ic = _keep1(*ocean.predict(o_ic, o_forcing))
        outs["atmosphere"].append(a_out)
        outs["ocean"].append(o_out)
    torch.cuda.synchronize()
    data = {realm: {k: torch.cat([o[k] for o in parts], dim=1) for k in parts[0]} for realm, parts in outs.items()}
    return data, {"atmosphere": a_ic, "ocean": o_ic}


@pytest.fixture(scope="module")
def pair(dev):
    stepper = ace_amd.load_coupled_stepper(coupled_checkpoint(), device=dev)
    ic, forcing = coupled_data()
    ic, forcing = _to(ic, dev), _to(forcing, dev)
    reference = stepper.predict(ic, forcing)
    torch.cuda.synchronize()
    return dict(stepper=stepper, ic=ic, forcing=forcing, reference=reference, engines={}, runs={}, compositions={})


def _engine(pair, graph):
    if graph not in pair["engines"]:
        eng = pair["engines"][graph] = CoupledRolloutEngine(pair["stepper"], B, N_OUTER, graph=graph)
        pair["runs"][graph] = _keep(*eng.predict(pair["ic"], pair["forcing"]))
        torch.cuda.synchronize()
    return pair["engines"][graph], pair["runs"][graph]


def _composed(pair, graph):
    if graph not in pair["compositions"]:
        pair["compositions"][graph] = _composition(pair["stepper"], pair["ic"], pair["forcing"], graph, N_OUTER)
    return pair["compositions"][graph]


@pytest.mark.parametrize("graph", GRAPHS)
def test_bitwise_the_composition_of_the_parts(pair, graph):
    """the engine adds no arithmetic of its own: equality, not a tolerance"""
    eng, run = _engine(pair, graph)
    data = run[0]
    assert data["atmosphere"]["PRESsfc"].shape[1] == N_OUTER * N_INNER and data["ocean"]["sst"].shape[1] == N_OUTER
    assert torch.isfinite(data["atmosphere"]["PRESsfc"]).all() and torch.isfinite(data["ocean"]["sst"]).float().mean() > 0.5
    assert not same(data["ocean"]["sst"][:, 0], data["ocean"]["sst"][:, 1])               # not degenerate
    _assert_same_run(run, _composed(pair, graph), graph)


def _steps_taken(realm, t):
    """network steps behind output t of a realm (0-based): every atmosphere and ocean step evaluated up to and including it"""
    if realm == "ocean":
        return (t + 1) * N_INNER + (t + 1)
    return (t + 1) + t // N_INNER


@pytest.mark.parametrize("graph", GRAPHS)
def test_against_the_coupled_stepper(pair, graph):
    """Against ``CoupledStepper.predict``: the atmosphere's first n_inner steps bitwise (no ocean step has run), NaN patterns equal
    everywhere, and from the first ocean step on the difference of ``OceanRolloutEngine`` from ``Stepper.predict`` - the
    normalisation's division rounding (ocean_rollout.py) - carried on.  The bar is the project's per-step parity bar, 1e-5 in
    ``rel_max``, times the network steps taken up to the output (every atmosphere and ocean step behind it: a step either makes
    such a difference or carries one on), the compounding tests/test_gpu_coupled_stepper.py uses.  The composition of
    ``test_bitwise_the_composition_of_the_parts`` - independent of the engine - is measured against the same reference in the
    same test; were it over the bar, the bar would be twice its figure.

    Measured on an MI355X, in every graph mode: 0.0 for the engine and for the composition, in both realms after one and after two
    ocean steps, against bars of 4.0e-5 / 8.0e-5 (ocean) and 7.0e-5 (atmosphere): at the tiny pair's statistics the two roundings of
    the normalisation's division agree, and both rollouts run the same fused exchange."""
    _, (data, _) = _engine(pair, graph)
    want = pair["reference"][0]
    comp = _composed(pair, graph)[0]
    for k, v in want["atmosphere"].items():
        assert same(data["atmosphere"][k][:, :N_INNER], v[:, :N_INNER]), k
    worst = {}
    for realm, first in (("ocean", 0), ("atmosphere", N_INNER)):
        for k, v in want[realm].items():
            assert torch.equal(torch.isnan(data[realm][k]), torch.isnan(v)), (realm, k)
            for t in range(first, v.shape[1]):
                n_ocean = t + 1 if realm == "ocean" else t // N_INNER
                b = v[:, t].nan_to_num()
                got, composed = rel_max(data[realm][k][:, t].nan_to_num(), b), rel_max(comp[realm][k][:, t].nan_to_num(), b)
                bar = PARITY * _steps_taken(realm, t)
                if composed > bar:
                    bar = 2.0 * composed
                key = (realm, n_ocean)
                seen = worst.get(key, (0.0, 0.0))
                worst[key] = (max(seen[0], got), max(seen[1], composed), bar)
                assert got <= bar, (realm, k, t, got, bar)
    for (realm, n_ocean), (got, composed, bar) in sorted(worst.items()):
        print(f"graph={graph}: engine vs CoupledStepper.predict, {realm} after {n_ocean} ocean step(s): {got:.3e} "
              f"(composition {composed:.3e}, bar at the last such step {bar:.3e})")


@pytest.mark.parametrize("graph", GRAPHS)
def test_two_windows_of_one_chain_into_one_of_two(pair, graph):
    _, whole = _engine(pair, graph)
    one = CoupledRolloutEngine(pair["stepper"], B, 1, graph=graph)
    first, second = _windows(pair["forcing"], (0, 1, 2))
    a, state = _keep(*one.predict(pair["ic"], first))
    b, end = _keep(*one.predict(state, second))
    chained = {realm: {k: torch.cat([a[realm][k], b[realm][k]], dim=1) for k in a[realm]} for realm in a}
    _assert_same_run((chained, end), whole, graph)


@pytest.mark.parametrize("graph", GRAPHS)
def test_a_second_predict_is_the_first_and_the_route(pair, graph):
    """the replay is deterministic and no exchange level of the first window leaks into the second"""
    eng, run = _engine(pair, graph)
    again = _keep(*eng.predict(pair["ic"], pair["forcing"]))
    _assert_same_run(again, run, graph)
    assert eng.launches() == 2 * N_OUTER
    assert (eng._window_graph is not None) == (graph == "window")


def _reweighted(realm):
    """the tiny checkpoint with the weights of one component scaled"""
    ckpt = coupled_checkpoint()
    module = ckpt["stepper"][f"{realm}_state"]["step"]["module"]
    for k, v in module.items():
        if torch.is_tensor(v) and v.is_floating_point() and k.endswith("weight"):
            module[k] = v * 1.05
    return ckpt


@pytest.mark.parametrize("graph", ["step", "window"])
def test_reloaded_weights_are_followed(dev, graph):
    """``load_state`` on a component after the engine has captured its graphs: the graphs are rebuilt and the result is that of a
    stepper loaded with the new weights from the start"""
    ic, forcing = coupled_data()
    ic, forcing = _to(ic, dev), _to(forcing, dev)
    stepper = ace_amd.load_coupled_stepper(coupled_checkpoint(), device=dev)
    eng = CoupledRolloutEngine(stepper, B, N_OUTER, graph=graph)
    before = _keep(*eng.predict(ic, forcing))
    held = eng._window_graph
    ckpt = _reweighted("ocean")
    stepper.ocean.load_state(ckpt["stepper"]["ocean_state"])
    after = _keep(*eng.predict(ic, forcing))
    if graph == "window":
        assert held is not None and eng._window_graph is not None and eng._window_graph is not held
    assert not same(after[0]["ocean"]["sst"], before[0]["ocean"]["sst"])
    fresh = CoupledRolloutEngine(ace_amd.load_coupled_stepper(ckpt, device=dev), B, N_OUTER, graph=graph)
    _assert_same_run(after, _keep(*fresh.predict(ic, forcing)), (graph, "ocean"))
    ckpt["stepper"]["atmosphere_state"] = _reweighted("atmosphere")["stepper"]["atmosphere_state"]
    stepper.atmosphere.load_state(ckpt["stepper"]["atmosphere_state"])
    both = _keep(*eng.predict(ic, forcing))
    assert not same(both[0]["atmosphere"]["PRESsfc"][:, :1], after[0]["atmosphere"]["PRESsfc"][:, :1])
    fresh = CoupledRolloutEngine(ace_amd.load_coupled_stepper(ckpt, device=dev), B, N_OUTER, graph=graph)
    _assert_same_run(both, _keep(*fresh.predict(ic, forcing)), (graph, "atmosphere"))


def test_engine_predict_over_windows_of_two_and_one(dev):
    stepper = ace_amd.load_coupled_stepper(coupled_checkpoint(), device=dev)
    ic, forcing = coupled_data(n_outer=3)
    ic, forcing = _to(ic, dev), _to(forcing, dev)
    whole = _keep(*CoupledRolloutEngine(stepper, B, 3, graph="step").predict(ic, forcing))
    predict = CoupledEnginePredict(stepper, B, graph="step")
    first, second = _windows(forcing, (0, 2, 3))
    a, state = predict(ic, first)
    b, end = predict(state, second)
    assert sorted(predict._engines) == [1, 2]
    chained = {realm: {k: torch.cat([a[realm][k], b[realm][k]], dim=1) for k in a[realm]} for realm in a}
    _assert_same_run((chained, end), whole, "2 + 1")
    assert chained["ocean"]["sst"].shape[1] == 3 and chained["atmosphere"]["PRESsfc"].shape[1] == 3 * N_INNER
