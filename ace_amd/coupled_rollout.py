"""CoupledRolloutEngine: the coupled loop (``CoupledStepper.predict_generator``, coupled.py) on static windows - a ``RolloutEngine``
for the SFNO atmosphere over ``n_coupled_steps * n_inner`` steps and an ``OceanRolloutEngine`` for the Samudra ocean over
``n_coupled_steps`` - with the exchange written in place into the two engines' own buffers.

Per coupled step i the engine enqueues, in the reference's order:
  1. ace_couple_ocean_to_atmosphere_window   the ocean's state (its initial condition, or its output of step i - 1) into the
                                             atmosphere window's time levels i * n_inner .. (i + 1) * n_inner: ``forcing[name]`` for
                                             a network forcing, ``target[name]`` for the surface temperature the fused physics
                                             reads as next-step data; the prescribed initial surface temperature into level i of
                                             a (B, n_coupled_steps, H, W) scratch
  2. n_inner atmosphere steps                ``RolloutEngine._enqueue_step``; the first one reads the prescribed surface temperature
                                             from the scratch (``WindowEngine.in_plane``'s override), not the previous step's
                                             output, which stays as generated - the reference edits only the initial condition
  3. ace_couple_atmosphere_to_ocean          the means of the atmosphere's outputs / shared forcings of these n_inner steps into the
                                             two levels i, i + 1 of the ocean's forcing window: ``[NaN, mean]`` or ``[mean, NaN]``,
                                             the NaN half on a level already consumed or about to be rewritten
  4. one ocean step                          ``OceanRolloutEngine._enqueue_step``
Both windows span the whole coupled window, so each component's state is carried by its own ``in_plane``; nothing is copied
between coupled steps, nothing is allocated, no table is uploaded and the host never synchronises inside a window.  The engine adds
no arithmetic: its numbers are those of the two engines and of the two exchange kernels.

``plan_coupled_window`` is the host plan - which plane every input of every step reads and which levels every exchange writes - in
names and indices, without a device: the engine resolves it to addresses once, at construction."""
import collections
from typing import Any, Container, Dict, List, Mapping, Optional, Tuple

import torch

from . import _lib
from .coupled import (MAX_NAMES, OFRAC_CARRIED, OFRAC_FROM_OCEAN_SIF, OFRAC_FROM_SIF, CoupledStepper, CoupledStepperConfig,
                      TensorDict, TensorMapping, _check)
from .ocean_rollout import OceanRolloutEngine
from .rollout import RolloutEngine, WindowEngine
from .ocean_derived_variables import OceanDeriveFn
from .stepper import PrognosticState, derive_over_window

# a (B, H, W) plane - or, as a destination, the first level of a window - of an engine: realm "atmosphere" / "ocean"; buffer "ic",
# "out", "forcing", "target" (WindowEngine's), or the coupled engine's own "prescribed" (the initial surface temperatures, one level
# per coupled step) and "scratch" (an ocean-supplied field the atmosphere holds no buffer for, n_inner + 1 levels)
Ref = collections.namedtuple("Ref", "realm buffer name level")
# one slot of the ocean -> atmosphere exchange: the source and its time levels, the destination window (None: not wanted) and its
# time levels, the name whose mask applies (None: no mask)
Slot = collections.namedtuple("Slot", "src src_levels dst dst_levels mask")
# one name of the atmosphere -> ocean exchange: the n_inner source planes, the two-level destination, the level the mean lands on
Mean = collections.namedtuple("Mean", "name srcs dst slot")


def _refuse(what: str) -> NotImplementedError:
    return NotImplementedError(f"CoupledRolloutEngine: {what}; run the coupled pair through CoupledStepper.predict")


class _Layout:
    """The name sets of a component's window, as ``WindowEngine`` lays them out."""

    def __init__(self, step_config, next_data=()):
        ins, outs = list(step_config.in_names), list(step_config.out_names)
        self.prognostic = [n for n in outs if n in ins]
        self.forcing = [n for n in ins if n not in outs]
        self.target = sorted(set(next_data) - set(self.forcing))
        self.next_step = set(step_config.next_step_forcing_names)

    def buffer_of(self, name: str) -> Optional[str]:
        return "forcing" if name in self.forcing else "target" if name in self.target else None


class CoupledWindowPlan:
    """What a coupled window of ``n_outer`` coupled steps reads and writes, per coupled step i and atmosphere step s."""

    def __init__(self, config: CoupledStepperConfig, n_outer: int, masked: Container[str] = ()):
        a_cfg, o_cfg = config.atmosphere.stepper, config.ocean.stepper
        self.n_inner, self.n_outer = config.n_inner_steps, n_outer
        n = self.n_inner
        if n_outer < 1:
            raise ValueError("a coupled window holds at least one coupled step")
        extra = set(a_cfg.ocean.forcing_names) | set(a_cfg.prescribed_prognostic_names)
        self.atmosphere, self.ocean = A, _ = _Layout(a_cfg, extra), _Layout(o_cfg)
        ts, of, sst = config.surface_temperature_name, config.ocean_fraction_name, config.sst_name
        ofp = config.ocean_fraction_prediction
        # -- ocean -> atmosphere: the slots of Coupler._atmosphere_forcings_fused, name for name
        if ofp is None:
            self.mode = OFRAC_CARRIED
            passed = [k for k in config.ocean_to_atmosphere_forcing_names if k != sst]
        else:
            ocean_sif = ofp.canonical_sea_ice_fraction_name() == "ocean_sea_ice_fraction"
            self.mode = OFRAC_FROM_OCEAN_SIF if ocean_sif else OFRAC_FROM_SIF
            passed = [k for k in config.ocean_to_atmosphere_forcing_names if k not in (sst, ofp.sea_ice_fraction_name)]
        self.passed = passed
        means = list(config.atmosphere_to_ocean_forcing_names)
        means += [k for k in config.shared_forcing_exogenous_names if k not in means]
        if len(passed) > MAX_NAMES or len(means) > MAX_NAMES:
            raise _refuse(f"{max(len(passed), len(means))} exchanged fields, the coupler kernels take {MAX_NAMES} "
                          "(ACE_COUPLE_MAX_NAMES)")
        self.prescribed_name = ts
        self.scratch: List[str] = []

        def dst(name: Optional[str], i: int, nullable: bool) -> Optional[Ref]:
            if name is None:
                return None
            buffer = A.buffer_of(name)
            if buffer is not None:
                return Ref("atmosphere", buffer, name, i * n)
            if nullable:
                return None
            if name not in self.scratch:
                self.scratch.append(name)
            return Ref("atmosphere", "scratch", name, 0)

        def mask(name: Optional[str]) -> Optional[str]:
            return name if name is not None and name in masked else None

        self.o2a: List[List[Slot]] = []
        for i in range(n_outer):
            state = lambda k: Ref("ocean", "ic", k, 0) if i == 0 else Ref("ocean", "out", k, i - 1)
            current_ts = Ref("atmosphere", "ic", ts, 0) if i == 0 else Ref("atmosphere", "out", ts, i * n - 1)
            slots = [Slot(state(sst), 1, dst(ts, i, False), n + 1, mask(ts)),
                     Slot(current_ts, 1, Ref("atmosphere", "prescribed", ts, i), 1, None)]
            if ofp is None:
                own = Ref("atmosphere", A.buffer_of(of), of, i * n)
                slots.append(Slot(own, n + 1, own if mask(of) else None, n + 1, mask(of)))       # masked in place, or left alone
            else:
                si, raw = ofp.atmosphere_sea_ice_fraction_name, ofp.sea_ice_fraction_name
                land = Ref("atmosphere", A.buffer_of(ofp.land_fraction_name), ofp.land_fraction_name, i * n)
                slots.append(Slot(land, n + 1, dst(of, i, False), n + 1, mask(of)))
                slots.append(Slot(state(raw), 1, dst(si, i, False), n + 1, mask(si)))
                raw_dst = dst(raw, i, True) if si != raw else None
                slots.append(Slot(state(raw), 1, raw_dst, n + 1, mask(raw) if raw_dst is not None else None))
            slots += [Slot(state(k), 1, dst(k, i, False), n + 1, mask(k)) for k in passed]
            self.o2a.append(slots)
        # -- atmosphere -> ocean
        generated = set(config.atmosphere_to_ocean_forcing_names)
        next_step = set(config.ocean_next_step_forcing_names)
        self.a2o: List[List[Mean]] = []
        for i in range(n_outer):
            row = []
            for k in means:
                if k in generated:
                    srcs = [Ref("atmosphere", "out", k, i * n + t) for t in range(n)]
                else:
                    srcs = [Ref("atmosphere", A.buffer_of(k), k, i * n + 1 + t) for t in range(n)]
                row.append(Mean(k, srcs, Ref("ocean", "forcing", k, i), 1 if k in next_step else 0))
            self.a2o.append(row)
        # -- what the exchange supplies (and load() therefore does not copy): every level of these buffers is written in a window
        self.supplied = {"atmosphere": {s.dst.name for s in self.o2a[0] if s.dst is not None and s.dst.buffer in ("forcing", "target")
                                        and s.dst != s.src},
                         "ocean": set(means)}

    def overrides(self) -> Dict[Tuple[str, int], Ref]:
        """``WindowEngine.in_plane``'s overrides of the atmosphere window: the first step of coupled step i reads the prescribed
        initial surface temperature."""
        return {(self.prescribed_name, i * self.n_inner): Ref("atmosphere", "prescribed", self.prescribed_name, i)
                for i in range(self.n_outer)}

    def atmosphere_in(self, name: str, s: int) -> Ref:
        """The plane input ``name`` of atmosphere step s is read from (``WindowEngine.in_plane`` with the overrides)."""
        over = self.overrides().get((name, s))
        if over is not None:
            return over
        return _in_plane(self.atmosphere, "atmosphere", name, s)

    def ocean_in(self, name: str, i: int) -> Ref:
        return _in_plane(self.ocean, "ocean", name, i)

    def written(self, i: int) -> Dict[Tuple[str, str, str], List[int]]:
        """(realm, buffer, name) -> the time levels the two exchanges of coupled step i write."""
        out: Dict[Tuple[str, str, str], List[int]] = {}
        for s in self.o2a[i]:
            if s.dst is not None:
                out[tuple(s.dst[:3])] = list(range(s.dst.level, s.dst.level + s.dst_levels))
        for m in self.a2o[i]:
            out[tuple(m.dst[:3])] = [m.dst.level, m.dst.level + 1]
        return out


def _in_plane(layout: _Layout, realm: str, name: str, s: int) -> Ref:
    if name in layout.prognostic:
        return Ref(realm, "ic", name, 0) if s == 0 else Ref(realm, "out", name, s - 1)
    return Ref(realm, "forcing", name, s + 1 if name in layout.next_step else s)


def plan_coupled_window(config: CoupledStepperConfig, n_coupled_steps: int, masked: Container[str] = ()) -> CoupledWindowPlan:
    """The host plan of a coupled window; ``masked``: the names the ocean's mask provider holds a mask for."""
    return CoupledWindowPlan(config, n_coupled_steps, masked)


def _exchange_masks(stepper: CoupledStepper) -> Dict[str, torch.Tensor]:
    """name -> mask of every atmosphere-side name of the exchange that has one (``Coupler._mask_plane``'s rule)."""
    cfg = stepper.config
    provider = stepper.coupler._mask_provider
    shape = stepper.coupler._img_shape
    names = set(cfg._ocean_supplied_atmosphere_names())
    if cfg.ocean_fraction_prediction is not None:
        names.add(cfg.ocean_fraction_prediction.sea_ice_fraction_name)
    masks = {}
    for name in sorted(names):
        mask = provider.get_mask_tensor_for(name)
        if mask is not None:
            if tuple(mask.shape) != tuple(shape):
                raise _refuse(f"the mask of '{name}' of shape {tuple(mask.shape)} is not a 2-D {tuple(shape)} plane")
            masks[name] = mask
    return masks


def check_supported(stepper: CoupledStepper, n_coupled_steps: int, graph: Optional[str]):
    """Every refusal of the engine, raised before any device work.  Returns (the plan, the masks of the exchanged names)."""
    WindowEngine._check_graph(graph)
    atmosphere, ocean = stepper.atmosphere, stepper.ocean
    a_step = atmosphere._step_obj
    net = a_step.module.torch_module
    for realm, component in (("atmosphere", atmosphere), ("ocean", ocean)):
        if getattr(component._step_obj, "global_mean_removal", None) is not None:
            raise _refuse(f"global_mean_removal on the {realm} component is not supported")
        from .ice_corrector import IceCorrector
        if isinstance(component._step_obj._corrector, IceCorrector):
            raise _refuse(f"a sea-ice corrector (ice_corrector) on the {realm} component is not supported")
    if not hasattr(net, "_ensure_native"):
        raise _refuse(f"the atmosphere's module is a {type(net).__name__}, not of the SFNO family")
    if hasattr(net, "draw_noise"):
        raise _refuse("a noise-conditioned atmosphere is not supported")
    if getattr(a_step.module, "_label_encoding", None) is not None:
        raise _refuse("a label-conditioned atmosphere is not supported")
    if getattr(atmosphere, "_multi_call_config", None) is not None:
        raise _refuse("multi-call diagnostics are not supported")
    if getattr(a_step, "secondary_decoder", None) is not None:
        raise _refuse("a secondary decoder is not supported")
    try:
        RolloutEngine.check_supported(atmosphere, graph)
    except NotImplementedError as e:
        raise _refuse(f"the atmosphere engine refuses this stepper ({e})") from e
    masks = _exchange_masks(stepper)
    plan = plan_coupled_window(stepper.config, n_coupled_steps, masked=masks)
    try:
        OceanRolloutEngine.check_supported(ocean)        # its RuntimeError for a CPU stepper comes last
    except NotImplementedError as e:
        raise _refuse(f"the ocean engine refuses this stepper ({e})") from e
    if next(net.parameters()).device.type != "cuda":
        raise RuntimeError("CoupledRolloutEngine runs on an MI355X: load the stepper onto a 'cuda' device (there is no CPU path)")
    return plan, masks


class CoupledRolloutEngine:
    def __init__(self, stepper: CoupledStepper, batch: int, n_coupled_steps: int, graph: Optional[str] = "step",
                 step_diagnostics: bool = False):
        if step_diagnostics:
            raise NotImplementedError("CoupledRolloutEngine: step_diagnostics (the corrector deltas) are built for RolloutEngine "
                                      "only, not for the coupled stepper")
        self.plan, masks = check_supported(stepper, n_coupled_steps, graph)
        plan = self.plan
        self.stepper, self.graph_mode = stepper, graph
        self.B, self.n_outer, self.n_inner = B, n_outer, n = batch, n_coupled_steps, plan.n_inner
        self.device = dev = next(stepper.atmosphere._step_obj.module.torch_module.parameters()).device
        H, W = stepper.coupler._img_shape
        self.HW = H * W
        f32 = dict(dtype=torch.float32, device=dev)
        self.prescribed = torch.zeros(B, n_outer, H, W, **f32)         # the initial surface temperature of each coupled step
        self.scratch = {k: torch.zeros(B, n + 1, H, W, **f32) for k in plan.scratch}
        override = {key: self.prescribed[:, ref.level] for key, ref in plan.overrides().items()}
        self.atmosphere = RolloutEngine(stepper.atmosphere, batch, n_outer * n, graph, in_override=override)
        self.ocean = OceanRolloutEngine(stepper.ocean, batch, n_outer, graph)
        for eng, layout in ((self.atmosphere, plan.atmosphere), (self.ocean, plan.ocean)):       # the plan's layout is the engines'
            assert (eng.prognostic, eng.forcing_names, eng.target_names) == (layout.prognostic, layout.forcing, layout.target)
        self._masks = {k: m.to(dev).to(torch.float32).contiguous() for k, m in masks.items()}
        # -- the exchange's tables, one row per coupled step, built and uploaded once
        i64 = dict(dtype=torch.int64, device=dev)
        rows = []
        for slots in plan.o2a:
            srcs = [self._window(s.src) for s in slots]
            dsts = [self._window(s.dst) if s.dst is not None else None for s in slots]
            rows.append([t.data_ptr() for t in srcs] + [x for t in srcs for x in (t.stride(0), t.stride(1))]
                        + [t.data_ptr() if t is not None else 0 for t in dsts]
                        + [x for t in dsts for x in ((t.stride(0), t.stride(1)) if t is not None else (0, 0))]
                        + [self._masks[s.mask].data_ptr() if s.mask is not None else 0 for s in slots])
        self._o2a_tab = torch.tensor(rows, **i64)
        ns = len(plan.o2a[0])
        base = [self._o2a_tab.data_ptr() + 8 * i * self._o2a_tab.shape[1] for i in range(n_outer)]
        self._o2a_addr = [(a, a + 8 * ns, a + 24 * ns, a + 32 * ns, a + 48 * ns) for a in base]
        self._n_means = nm = len(plan.a2o[0])
        if nm:
            rows = []
            for means in plan.a2o:
                srcs = [self._window(r) for m in means for r in m.srcs]
                dsts = [self._window(m.dst) for m in means]
                rows.append([t.data_ptr() for t in srcs] + [t.stride(0) for t in srcs] + [t.data_ptr() for t in dsts]
                            + [x for t in dsts for x in (t.stride(0), t.stride(1))])
            self._a2o_tab = torch.tensor(rows, **i64)
            base = [self._a2o_tab.data_ptr() + 8 * i * self._a2o_tab.shape[1] for i in range(n_outer)]
            self._a2o_addr = [(a, a + 8 * nm * n, a + 16 * nm * n, a + 16 * nm * n + 8 * nm) for a in base]
            self._a2o_slot = torch.tensor([m.slot for m in plan.a2o[0]], dtype=torch.int32, device=dev)
        self._window_graph = None
        self._graph_key = None
        self._launches = 0

    def _window(self, ref: Ref) -> torch.Tensor:
        """The (B, levels, H, W) buffer of a plan reference from its level on: data_ptr / stride(0) / stride(1) are the plane's
        address and its (sample, step) strides."""
        if ref.buffer == "prescribed":
            return self.prescribed[:, ref.level:]
        if ref.buffer == "scratch":
            return self.scratch[ref.name][:, ref.level:]
        eng = self.atmosphere if ref.realm == "atmosphere" else self.ocean
        return getattr(eng, ref.buffer)[ref.name][:, ref.level:]

    def launches(self) -> int:
        """Native exchange calls (``ace_couple_*``) in one window, as last enqueued or captured: the route query of the tests."""
        return self._launches

    # -- one coupled step, enqueued on the current stream
    def _enqueue_step(self, i: int, replay: bool, interpolate: int):
        L = _lib.lib()
        plan, n = self.plan, self.n_inner
        _check(L.ace_couple_ocean_to_atmosphere_window(*self._o2a_addr[i], len(plan.passed), plan.mode, interpolate, n, self.B,
                                                       self.HW, _lib.current_stream()))
        self._launches += 1
        for t in range(n):
            self.atmosphere._enqueue_step(i * n + t, replay)
        if self._n_means:
            _check(L.ace_couple_atmosphere_to_ocean(*self._a2o_addr[i], self._a2o_slot.data_ptr(), self._n_means, n, self.B,
                                                    self.HW, _lib.current_stream()))
            self._launches += 1
        self.ocean._enqueue_step(i, replay)

    def run_window(self):
        """Enqueue the coupled window on the current stream (no host synchronisation)."""
        with torch.no_grad(), torch.cuda.device(self.device):
            keys = []
            for eng in (self.atmosphere, self.ocean):
                key = eng._prepare_window()
                if key != eng._graph_key:
                    eng._window_graph = None
                    eng._graph_key = key
                keys.append(key)
            a = self.atmosphere
            interpolate = int(self.stepper.coupler._prescriber.interpolate)
            # what the window graph holds besides the components' keys: the atmosphere's hooks (a replaced one rebuilds its fused
            # physics without a new key) and the prescriber's mode
            key = (*keys, id(a._ocean), id(a._corrector), id(a._physics), interpolate)
            if key != self._graph_key:
                self._window_graph = None
                self._graph_key = key
            if self.graph_mode == "window":
                if self._window_graph is None:
                    # warm up outside capture (first-touch allocations, workspaces, weight handles), then capture once
                    side = torch.cuda.Stream(device=self.device)
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        self._enqueue_step(0, False, interpolate)
                    torch.cuda.current_stream().wait_stream(side)
                    self._launches = 0
                    g = torch.cuda.CUDAGraph()
                    with _lib.capture_without_gc(), torch.cuda.graph(g):
                        for i in range(self.n_outer):
                            self._enqueue_step(i, False, interpolate)
                    self._window_graph = g
                self._window_graph.replay()
            else:
                self._launches = 0
                for i in range(self.n_outer):
                    self._enqueue_step(i, self.graph_mode == "step", interpolate)
            a._after_window()

    def load(self, initial_condition: Mapping[str, TensorMapping], forcing: Mapping[str, TensorMapping]):
        """Copies what the exchange does not produce: the prognostic initial conditions and the exogenous forcing records
        (``atmosphere_forcing_window_names`` / ``ocean_forcing_window_names``)."""
        for realm, eng in (("atmosphere", self.atmosphere), ("ocean", self.ocean)):
            ic, record, supplied = initial_condition[realm], forcing[realm], self.plan.supplied[realm]
            for k in eng.prognostic:
                eng.ic[k].copy_(ic[k].reshape(eng.B, 1, eng.H, eng.W))
            for buffers in (eng.forcing, eng.target):
                for k, buf in buffers.items():
                    if k not in supplied:
                        buf.copy_(record[k][:, : eng.T + 1])
        self.atmosphere._after_load()

    def predict(self, initial_condition: Mapping[str, TensorMapping], forcing: Mapping[str, TensorMapping],
                compute_derived_variables: bool = False) -> Tuple[Dict[str, TensorDict], Dict[str, PrognosticState]]:
        """The contract of ``CoupledStepper.predict`` for one window of ``n_coupled_steps``: ({"atmosphere": name -> (B, n_outer *
        n_inner, H, W), "ocean": name -> (B, n_outer, H, W)} as views of the static buffers, the final ``PrognosticState`` per realm
        with its ``stepper_state``, which chains into the next window).  As there, forcings derived from the time axis are the
        caller's to apply beforehand."""
        for realm in ("atmosphere", "ocean"):
            nt = next(iter(initial_condition[realm].values())).shape[1]
            if nt != 1:
                raise ValueError(f"{realm.capitalize()} initial condition must have 1 timesteps, got {nt}.")
        for realm, eng in (("atmosphere", self.atmosphere), ("ocean", self.ocean)):
            for k, v in forcing[realm].items():
                if v.shape[1] != eng.T + 1:
                    raise ValueError(f"the {realm} forcing '{k}' has {v.shape[1]} time levels, this engine's window of "
                                     f"{self.n_outer} coupled steps takes {eng.T + 1}")
        carried = {realm: getattr(initial_condition[realm], "stepper_state", None) for realm in ("atmosphere", "ocean")}
        with torch.no_grad():
            self.load(initial_condition, forcing)
            self.atmosphere._carry_in(carried["atmosphere"])
            self.ocean._carry_in(carried["ocean"])
            self.run_window()
            carried = {"atmosphere": self.atmosphere._carry_out(carried["atmosphere"]),
                       "ocean": self.ocean._carry_out(carried["ocean"])}
        data: Dict[str, TensorDict] = {"atmosphere": self.atmosphere.out, "ocean": self.ocean.out}
        state: Dict[str, PrognosticState] = {}
        for realm, eng in (("atmosphere", self.atmosphere), ("ocean", self.ocean)):
            state[realm] = PrognosticState({k: eng.out[k][:, -1:] for k in eng.prognostic})
            state[realm].stepper_state = carried[realm]
        if compute_derived_variables:
            for realm, eng in (("atmosphere", self.atmosphere), ("ocean", self.ocean)):
                derive_func = getattr(self.stepper, realm).derive_func
                if realm == "ocean" and not isinstance(derive_func, OceanDeriveFn):
                    continue              # an ocean without a depth coordinate derives nothing (the reference's NullDeriveFn)
                data[realm] = derive_over_window(derive_func, data[realm], initial_condition[realm], forcing[realm], 1, eng.T)
        return data, state


class CoupledEnginePredict:
    """``CoupledStepper.predict`` on ``CoupledRolloutEngine`` (as ``inference.EnginePredict`` is for one component): one engine per
    number of coupled steps (the last window of a rollout may be shorter), built on first use.  Outputs are copied out of the
    engine's buffers (the next window reuses them)."""

    def __init__(self, stepper: CoupledStepper, batch: int, graph: Optional[str] = "step"):
        self._stepper = stepper
        self._batch = batch
        self._graph = graph
        self._engines: Dict[int, Any] = {}

    def __call__(self, initial_condition: Mapping[str, TensorMapping], forcing: Mapping[str, TensorMapping],
                 compute_derived_variables: bool = False) -> Tuple[Dict[str, TensorDict], Dict[str, PrognosticState]]:
        if forcing["ocean"]:
            n_outer = next(iter(forcing["ocean"].values())).shape[1] - 1
        else:
            n_outer = (next(iter(forcing["atmosphere"].values())).shape[1] - 1) // self._stepper.n_inner_steps
        eng = self._engines.get(n_outer)
        if eng is None:
            eng = self._engines[n_outer] = CoupledRolloutEngine(self._stepper, self._batch, n_outer, graph=self._graph)
        data, state = eng.predict(initial_condition, forcing, compute_derived_variables)
        kept = {}
        for realm, s in state.items():
            kept[realm] = PrognosticState({k: v.clone() for k, v in s.items()})
            kept[realm].stepper_state = getattr(s, "stepper_state", None)
        return {realm: {k: v.clone() for k, v in fields.items()} for realm, fields in data.items()}, kept
