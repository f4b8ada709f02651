"""RolloutEngine: the stepper loop (fme/ace/stepper/single_module.py:1124-1167) on static HBM
buffers with the per-step forward replayed from a hipGraph.

Per step s the engine enqueues
  1. ace_pack_normalize    gather state (previous output or the initial condition) and the forcing
                           slice (index s, or s+1 for next_step_forcing_names) -> packed, normalised input
  2. the SFNO forward      (`graph="step"`: the library's captured hipGraph; `graph="window"`: steps 1-3
                           of the whole window live in one torch-captured hipGraph; `graph=None`: eager launches)
  3. ace_unpack_denormalize  network output -> out[name][:, s] (denormalised), which is also step s+1's state
     (residual_prediction: the normalised prognostic inputs are added to the network output first; post-step hooks and
     prescribed prognostics then edit out[name][:, s] in place)
so the numbers are bit-identical to `Stepper.predict` (same kernels, same (x-mean)/std and y*std+mean roundings).
Nothing is allocated and the host never synchronises inside the window.

A stepper with global-mean removal (ace_amd/global_mean_removal.py) replaces 1 by ace_gmr_partials + ace_gmr_pack_normalize (the
per-sample means of the step's own inputs, the shift added in front of the normaliser, the synthetic channels written behind
the in_names) and 3 by ace_gmr_unpack_denormalize (the shift taken off the listed outputs): csrc/gmr.hip.  Without the option the
engine issues exactly the calls above.

`WindowEngine` is what every static-buffer engine shares (`OceanRolloutEngine`, ocean_rollout.py, and `LandRolloutEngine`,
land_rollout.py, are the others; `MaskedWindowEngine` holds the static-masking tables those two share): the buffers,
the one statement of the window layout (`in_plane` / `next_plane` / `out_plane`), the tail of a forward, the window graph and
load / predict / continue_from_last.  An engine supplies its pack and forward (`_enqueue_step`), what its captured graphs depend
on (`_prepare_window`) and what `predict` carries in `stepper_state`."""

import os
from typing import Dict, Mapping, Optional, Tuple

import torch

from . import _lib
from .stepper import Stepper


def _nan_to_zero(t: torch.Tensor) -> None:
    torch.nan_to_num_(t, nan=0.0, posinf=float("inf"), neginf=float("-inf"))


class WindowEngine:
    """A window of T steps of B samples on static buffers: `x` (the packed, normalised network input), `ic[name]` (B, 1, H, W) for
    the prognostic names, `forcing[name]` / `target[name]` (B, T + 1, H, W) for the input-only names / the next-step data the
    post-step work reads besides them, `out[name]` (B, T, H, W).

    An engine supplies ``_enqueue_step(s, replay)`` (step s on the current stream; `replay`: the forward from its per-step
    captured graph) and ``_prepare_window()`` (its checks and uploads before every window; returns the key of what its captured
    graphs hold - a new key drops the window graph)."""

    @staticmethod
    def _check_graph(graph: Optional[str]) -> None:
        if graph not in (None, "step", "window"):
            raise ValueError("graph must be None, 'step' or 'window'")

    def __init__(self, stepper: Stepper, net, batch: int, n_forward_steps: int, graph: Optional[str], next_data=(),
                 in_override: Optional[Mapping[Tuple[str, int], torch.Tensor]] = None):
        """``in_override``: (name, s) -> the (B, H, W) plane input `name` of step s is read from instead of the window's own
        (a coupled rollout's prescribed initial surface temperature, coupled_rollout.py); none by default."""
        step = stepper._step_obj
        cfg = step.config
        self.stepper, self.net, self.graph_mode = stepper, net, graph
        self._in_override = dict(in_override or {})
        self.device = dev = next(net.parameters()).device
        self.B, self.T = B, T = batch, n_forward_steps
        self.H, self.W = H, W = step._img_shape
        self.HW = H * W
        self.in_names, self.out_names = list(cfg.in_names), list(cfg.out_names)
        self.prognostic = [n for n in self.out_names if n in self.in_names]
        self.forcing_names = [n for n in self.in_names if n not in self.out_names]
        self.next_step_forcing = set(cfg.next_step_forcing_names)
        self.target_names = sorted(set(next_data) - set(self.forcing_names))
        f32 = dict(dtype=torch.float32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        # global-mean removal (ace_amd/global_mean_removal.py): its synthetic channels are packed behind the in_names
        gmr = getattr(step, "global_mean_removal", None)
        self.extra_names = list(gmr.extra_channel_names) if gmr is not None else []
        self._gmr = None                # RolloutEngine's tables of the fused pack / unpack (_build_gmr)
        self.x = torch.zeros(B, len(self.in_names) + len(self.extra_names), H, W, **f32)
        self.ic = {n: torch.zeros(B, 1, H, W, **f32) for n in self.prognostic}
        self.forcing = {n: torch.zeros(B, T + 1, H, W, **f32) for n in self.forcing_names}
        self.target = {n: torch.zeros(B, T + 1, H, W, **f32) for n in self.target_names}
        self.out = {n: torch.zeros(B, T, H, W, **f32) for n in self.out_names}
        norm = step.normalizer
        # normalizer.py:212-242: NaNs become 0 in normalised space (inputs) / the variable's mean (outputs).  The fused pack / unpack
        # kernels do not replace NaNs: one in-place pass over the packed tensor on either side when the normaliser asks for it
        self._fill_in, self._fill_out = bool(norm.fill_nans_on_normalize), bool(norm.fill_nans_on_denormalize)
        self.in_mean = torch.stack([norm.means[n].to(dev) for n in self.in_names]).contiguous()
        self.in_std = torch.stack([norm.stds[n].to(dev) for n in self.in_names]).contiguous()
        self.out_mean = torch.stack([norm.means[n].to(dev) for n in self.out_names]).contiguous()
        self.out_std = torch.stack([norm.stds[n].to(dev) for n in self.out_names]).contiguous()
        # residual prediction (single_module.py:663-664): normalised prognostic inputs are added to the network output
        self._res_in = self._res_out = None
        if cfg.residual_prediction:
            self._res_in = torch.tensor([self.in_names.index(n) for n in self.prognostic], **i64)
            self._res_out = torch.tensor([self.out_names.index(n) for n in self.prognostic], **i64)
        # the unpack's per-step pointer tables and per-sample strides
        self._dst_ptrs, self._dst_ptr_addr = self._table([[self.out_plane(n, s).data_ptr() for n in self.out_names] for s in range(T)])
        self._dst_strides = torch.full((len(self.out_names),), T * self.HW, **i64)
        self._window_graph = None
        self._graph_key = None          # what the window graph was captured against (_prepare_window)

    # -- the window layout: the (B, H, W) plane of a name at window position s
    def in_plane(self, n: str, s: int, forcing: Optional[Mapping[str, torch.Tensor]] = None) -> torch.Tensor:
        """Input n of step s: the initial condition / step s - 1's output, or the forcing at s (s + 1 for next_step_forcing_names);
        an override of (n, s) given at construction comes first."""
        if (n, s) in self._in_override:
            return self._in_override[(n, s)]
        if n in self.ic:
            return self.ic[n][:, 0] if s == 0 else self.out[n][:, s - 1]
        return (self.forcing if forcing is None else forcing)[n][:, s + 1 if n in self.next_step_forcing else s]

    def next_plane(self, n: str, s: int, forcing: Optional[Mapping[str, torch.Tensor]] = None) -> torch.Tensor:
        """Next-step datum n of step s: the forcing or target at s + 1."""
        return (self.target if n in self.target else self.forcing if forcing is None else forcing)[n][:, s + 1]

    def out_plane(self, n: str, s: int) -> torch.Tensor:
        """Output n of step s (also step s + 1's state)."""
        return self.out[n][:, s]

    def _table(self, rows):
        """int64 device table of one row per window position, and the address of each row (plain ints for the per-step launches)"""
        tab = torch.tensor(rows, dtype=torch.int64, device=self.device)
        return tab, [tab.data_ptr() + 8 * s * tab.shape[1] for s in range(tab.shape[0])]

    def _unpack(self, L, stream, y: torch.Tensor, dst: int, dst_strides: torch.Tensor) -> None:
        """The tail of a forward: residual add, NaN fill and ace_unpack_denormalize of the normalised output y into the planes of
        the pointer table row `dst`."""
        if self._res_in is not None:
            y.index_add_(1, self._res_out, self.x.index_select(1, self._res_in))
        if self._fill_out:      # 0 in normalised space denormalises to the mean
            _nan_to_zero(y)
        if self._gmr is not None:       # ... minus the shift of the listed outputs (single_module.py:666-668)
            g = self._gmr
            _lib.check(L.ace_gmr_unpack_denormalize(y.data_ptr(), self.out_mean.data_ptr(), self.out_std.data_ptr(), dst,
                                                    dst_strides.data_ptr(), g["out_idx"].data_ptr(), g["shift"].data_ptr(), self.B,
                                                    len(self.out_names), g["K"], self.HW, stream))
            return
        _lib.check(L.ace_unpack_denormalize(y.data_ptr(), self.out_mean.data_ptr(), self.out_std.data_ptr(), dst,
                                            dst_strides.data_ptr(), self.B, len(self.out_names), self.HW, stream))

    def _carry_in(self, carried) -> None:
        """predict(): the initial condition's stepper_state, after load()."""

    def _carry_out(self, carried):
        """predict(): the stepper_state of the returned prognostic state."""
        return carried

    # -- the window
    def run_window(self):
        """Enqueue the T steps of the window on the current stream (no host synchronisation)."""
        with torch.no_grad():
            key = self._prepare_window()
            if key != self._graph_key:
                self._window_graph = None
                self._graph_key = key
            if self.graph_mode == "window":
                if self._window_graph is None:
                    # warm up outside capture (first-touch allocations, workspaces, weight handles), then capture once
                    side = torch.cuda.Stream(device=self.device)
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        self._enqueue_step(0, False)
                    torch.cuda.current_stream().wait_stream(side)
                    g = torch.cuda.CUDAGraph()
                    with _lib.capture_without_gc(), torch.cuda.graph(g):
                        for s in range(self.T):
                            self._enqueue_step(s, False)
                    self._window_graph = g
                self._window_graph.replay()
            else:
                for s in range(self.T):
                    self._enqueue_step(s, self.graph_mode == "step")

    def load(self, initial_condition: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor]):
        for n in self.prognostic:
            self.ic[n].copy_(initial_condition[n].reshape(self.B, 1, self.H, self.W))
        for n in self.forcing_names:
            self.forcing[n].copy_(forcing[n][:, : self.T + 1])
        for n in self.target_names:
            self.target[n].copy_(forcing[n][:, : self.T + 1])

    def predict(self, initial_condition, forcing, time=None) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
        """Same contract as Stepper.predict for one window of n_forward_steps: (out name -> (B, T, H, W) static buffers, the final
        prognostic state; a ``PrognosticState`` initial condition carries the previous window's stepper_state in, the returned one
        carries this window's out).  ``time``: the window's TimeAxis when the stepper derives forcings from it (or `forcing` is a
        ForcingWindow)."""
        from .stepper import PrognosticState
        deriver = self.stepper.forcing_deriver
        # ALWAYS computed - a data field of the same name in the forcing record is overwritten, as Insolation.compute and
        # Stepper.predict do (fme/core/step/derived_forcings: the derived field wins) - unless this very window has been through
        # the deriver already (EnginePredict derives in front of the engine and marks the window)
        if deriver.needs_time and not getattr(forcing, "derived", False):
            forcing = deriver(forcing, time, device=self.device)      # once per window, in front of the captured steps
        carried = getattr(initial_condition, "stepper_state", None)
        with torch.no_grad():
            self.load(initial_condition, forcing)
            self._carry_in(carried)
            self.run_window()
            stepper_state = self._carry_out(carried)
        state = PrognosticState({n: self.out[n][:, -1:] for n in self.prognostic})
        if stepper_state is not None:
            state.stepper_state = stepper_state
        return self.out, state

    def continue_from_last(self):
        """Carry the final prognostic state into the initial-condition slot (next window of a long rollout)."""
        for n in self.prognostic:
            self.ic[n].copy_(self.out[n][:, -1:])


class MaskedWindowEngine(WindowEngine):
    """What the engines of steppers with static spatial masking share (``OceanRolloutEngine``, ``LandRolloutEngine``): the steppers'
    maskers and their shape check, the device tables of the masking pack (ace_mask_pack_normalize) and of the provider's output
    masker (ace_mask_planes, in place on out[:, s]), and the two launches."""

    @staticmethod
    def _static_maskers(stepper: Stepper, refuse):
        """The stepper's (input masker, output masker), each None when it is no static spatial masking; ``refuse(what)`` builds the
        engine's exception for a mask that is not a 2-D plane of the grid."""
        from .masking import StaticSpatialMasking
        step = stepper._step_obj
        in_mask = stepper._input_process_func if isinstance(stepper._input_process_func, StaticSpatialMasking) else None
        out_mask = stepper._output_masking if isinstance(stepper._output_masking, StaticSpatialMasking) else None
        for m in (in_mask, out_mask):
            if m is not None:
                for k, t in m._mask.masks.items():
                    if tuple(t.shape) != tuple(step._img_shape):
                        raise refuse(f"the mask '{k}' of shape {tuple(t.shape)} is not a 2-D {tuple(step._img_shape)} plane")
        return in_mask, out_mask

    def _build_input_mask(self, in_mask, planes) -> None:
        """mask index, fill and hit planes of ``planes`` (the names the pack walks) for ace_mask_pack_normalize"""
        dev, n = self.device, len(planes)
        if in_mask is not None:
            self._in_idx, self._in_fill = in_mask.device_tables(planes, dev, (self.H, self.W))
            _, self._in_hits = in_mask.hit_planes(dev, (self.H, self.W))
        else:
            self._in_idx = torch.full((n,), -1, dtype=torch.int32, device=dev)
            self._in_fill = torch.zeros(n, dtype=torch.float32, device=dev)
            self._in_hits = None

    def _mask_pack_normalize(self, L, stream, srcs, src_strides, stage, stage_strides, nplanes: int) -> None:
        """One ace_mask_pack_normalize of the table rows at these addresses into self.x (``stage``: None for no staged planes)."""
        from .masking import _check
        hits = self._in_hits
        _check(L.ace_mask_pack_normalize(srcs, src_strides, self._in_idx.data_ptr(), hits.data_ptr() if hits is not None else None,
                                         hits.shape[0] if hits is not None else 0, self._in_fill.data_ptr(), stage, stage_strides,
                                         self.in_mean.data_ptr(), self.in_std.data_ptr(), self.x.data_ptr(), len(self.in_names),
                                         nplanes, self.B, self.HW, stream))

    def _build_output_mask(self, out_mask) -> None:
        """the output names the provider masks, and their per-step pointer tables"""
        dev, T, HW = self.device, self.T, self.HW
        self._out_names_masked = []
        if out_mask is not None:
            self._out_names_masked = [o for o, (k, _) in zip(self.out_names, out_mask.plan(self.out_names)) if k is not None]
        self._out_mask = out_mask
        if self._out_names_masked:
            self._out_idx, self._out_fill = out_mask.device_tables(self._out_names_masked, dev, (self.H, self.W))
            _, self._out_hits = out_mask.hit_planes(dev, (self.H, self.W))
            self._omask_ptrs, self._omask_addr = self._table([[self.out_plane(o, s).data_ptr() for o in self._out_names_masked]
                                                              for s in range(T)])
            self._omask_strides = torch.full((len(self._out_names_masked),), T * HW, dtype=torch.int64, device=dev)

    def _mask_outputs(self, L, stream, s: int) -> None:
        """The provider's output masker on out[:, s], in place: one ace_mask_planes, none when no output is masked."""
        from .masking import _check
        if self._out_names_masked:
            a = self._omask_addr[s]
            st = self._omask_strides.data_ptr()
            _check(L.ace_mask_planes(a, st, a, st, self._out_idx.data_ptr(), self._out_hits.data_ptr(), self._out_hits.shape[0],
                                     self._out_fill.data_ptr(), len(self._out_names_masked), self.B, self.HW, stream))

    def set_labels(self, labels) -> None:
        if labels is not None:
            raise TypeError("Labels are not allowed for unconditional models")


class RolloutEngine(WindowEngine):
    # graph="window" with a noise-conditioned net keeps the conditioning fields of all T steps of a window in one static device
    # buffer (T x B x cond_channels x H x W fp32) that the captured steps read; beyond this size the engine refuses and names
    # graph="step" (ADVICE r05).  8 GiB = a 40-step window of ~290 conditioning channels at 1 degree.
    max_window_conditioning_bytes = 8 << 30

    @staticmethod
    def check_supported(stepper: Stepper, graph: Optional[str]) -> None:
        """What the engine refuses of a stepper as it stands, raised before any device work (the constructor's first act)."""
        step = stepper._step_obj
        if getattr(step, "secondary_decoder", None) is not None and graph == "window":
            raise NotImplementedError("graph='window' with a secondary decoder: its module call is not captured; use graph='step'")
        from .ice_corrector import IceCorrector
        from .ocean_corrector import OceanCorrector
        if isinstance(step._corrector, IceCorrector):
            raise NotImplementedError("RolloutEngine: a stepper with a sea-ice corrector (ice_corrector) runs through "
                                      "Stepper.predict (or, with a Samudra module, OceanRolloutEngine)")
        if isinstance(step._corrector, OceanCorrector):
            raise NotImplementedError("RolloutEngine: a stepper with an ocean corrector (ocean_corrector) runs through "
                                      "Stepper.predict; the fused post-step physics of the engine is the atmosphere corrector's")
        if getattr(stepper, "_masks", False):
            raise NotImplementedError("RolloutEngine: static spatial masking of the step inputs / outputs (input_masking, the dataset's "
                                      "mask provider) is applied by Stepper.predict")
        if getattr(stepper, "_multi_call_config", None) is not None and graph == "window":
            raise NotImplementedError("graph='window' with multi-call diagnostics is not captured; use graph='step'")

    def __init__(self, stepper: Stepper, batch: int, n_forward_steps: int, graph: Optional[str] = "step",
                 in_override: Optional[Mapping[Tuple[str, int], torch.Tensor]] = None, step_diagnostics: bool = False):
        """``step_diagnostics``: ``predict`` returns its outputs as a ``WindowData`` whose ``.step_diagnostics`` holds the corrector
        deltas of the window (ace_amd/step_diagnostics.py: views of a static buffer, overwritten by the next window); ``None`` when
        the stepper has no corrector or it writes nothing.  Off by default - the reference always attaches them - and then the engine
        enqueues exactly what it did before the option existed."""
        self._check_graph(graph)
        self.check_supported(stepper, graph)
        step = stepper._step_obj
        cfg = step.config
        # secondary decoder (fme/core/step/secondary_decoder.py): column-local diagnostics decoded from the network's normalised
        # output tensor - one more native module call on the static y buffer per step and a second fused unpack
        self._secondary = getattr(step, "secondary_decoder", None)
        # multi-call diagnostics (fme/core/step/multi_call.py): per multiplier one more pack (the scaled forcing) / forward / unpack
        # into scratch planes / hooks per step, selected outputs copied under their suffixed names
        self._mc = getattr(stepper, "_multi_call_config", None)
        # post-step hooks (corrector, prescribed-SST ocean): torch ops on the static buffers between the fused unpack of
        # step s and the pack of step s + 1 - stream ordered, no host synchronisation.  The corrector state (dry-air
        # reference mass) is seeded by the first step after load() and survives continue_from_last().
        self._corrector = step._corrector
        self._ocean = step._ocean
        self._corrector_state = None
        # graph="window" captures the hooks with the steps.  The one piece of hook state - the dry-air reference mass the
        # corrector seeds on its first step (fme/core/corrector/state.py) - lives in a static device buffer with a device
        # flag, selected branch-free inside the captured region, so a replay neither re-seeds nor forgets it.
        self._ref_mass = None       # (B, 1, 1) fp64, allocated on first use
        self._have_ref = None       # device bool scalar
        net = step.module.torch_module
        self._conditioned = hasattr(net, "draw_noise")
        self._labels = None          # (B, n_labels) tensor in the module's label encoding: set_labels()
        # seedable random source of a stochastic module (fme/core/random_state.py; StepperState.random_state): active around every
        # network call of a window, as Stepper.step activates it (single_module.py:1063-1068).  The draw happens on the host,
        # outside any captured region, and reaches the device as a plain copy.
        self._random_state = None
        # graph="window" with a noise-conditioned net: the draws of the whole window are made on the host BEFORE the replay, in step
        # order (the same generator consumption as the eager loop), into a static (T, B, cond, H, W) buffer the captured steps read
        self._cond_window = None
        self.sec_names = list(cfg.secondary_decoder.secondary_diagnostic_names) if self._secondary is not None else []
        # The secondary decoder's diagnostics are unpacked straight into their output planes: they do not pass through the post-step
        # hooks here (the reference and Stepper.predict put them in the dict the corrector and the ocean see).  Refuse the
        # configurations where that difference would show instead of raising KeyError mid-rollout.
        # (the ocean's surface temperature cannot clash: OceanConfig.build requires it among the step's in_names AND out_names,
        # and a secondary diagnostic may be neither - step.py's configuration checks)
        hooked = set(getattr(self._corrector, "force_positive_names", []) or [])
        clash = sorted(hooked.intersection(self.sec_names))
        if clash:
            raise NotImplementedError(f"secondary-decoder diagnostics {clash} are also touched by the post-step hooks (force_positive / "
                                      "ocean): use Stepper.predict for this configuration")
        # next-step data the hooks read that is not a network forcing input (e.g. the prescribed SST: prognostic AND target)
        self.prescribed = list(cfg.prescribed_prognostic_names)
        extra = set(cfg.ocean.forcing_names) if cfg.ocean is not None else set()
        super().__init__(stepper, net, batch, n_forward_steps, graph, next_data=extra | set(self.prescribed), in_override=in_override)
        dev, B, T, H, W = self.device, batch, n_forward_steps, self.H, self.W
        f32 = dict(dtype=torch.float32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        self.y = torch.zeros(B, len(self.out_names), H, W, **f32)   # network output (normalised)
        # the pack's per-step pointer tables and per-sample strides
        planes = [[self.in_plane(n, s) for n in self.in_names] for s in range(T)]
        self._src_ptrs, self._src_ptr_addr = self._table([[p.data_ptr() for p in row] for row in planes])
        self._src_strides, self._src_stride_addr = self._table([[p.stride(0) for p in row] for row in planes])
        if self.sec_names:
            for n in self.sec_names:
                self.out[n] = torch.zeros(B, T, H, W, **f32)
            norm = step.normalizer
            self.sec_mean = torch.stack([norm.means[n].to(dev) for n in self.sec_names]).contiguous()
            self.sec_std = torch.stack([norm.stds[n].to(dev) for n in self.sec_names]).contiguous()
            self._sec_dst_ptrs, self._sec_dst_ptr_addr = self._table([[self.out_plane(n, s).data_ptr() for n in self.sec_names]
                                                                      for s in range(T)])
            self._sec_dst_strides = torch.full((len(self.sec_names),), T * self.HW, **i64)
        self._gmr = self._build_gmr(step)
        self._mc_state = None
        if self._mc is not None:
            from .multi_call import get_multi_call_name
            mc = self._mc
            if mc.forcing_name not in self.forcing_names:
                raise NotImplementedError(f"RolloutEngine: the multi-call forcing '{mc.forcing_name}' must be an input-only network input")
            if any(n not in self.out_names for n in mc.output_names):
                raise NotImplementedError("RolloutEngine: multi-call outputs must be network outputs (not secondary-decoder diagnostics)")
            self._mc_factors = list(mc.forcing_multipliers.items())
            self._mc_copy = [[(n, get_multi_call_name(n, suffix)) for n in mc.output_names] for suffix, _ in self._mc_factors]
            for pairs in self._mc_copy:
                for _, new in pairs:
                    self.out[new] = torch.zeros(B, T, H, W, **f32)
            self.forcing_mc = [torch.zeros(B, T + 1, H, W, **f32) for _ in self._mc_factors]     # the scaled forcing, per multiplier
            self._mc_forcing = [{**self.forcing, mc.forcing_name: f} for f in self.forcing_mc]    # ... in place of the plain one
            self.mc_scratch = {n: torch.zeros(B, 1, H, W, **f32) for n in self.out_names}        # one step's outputs of a re-evaluation
            self._mc_src_ptrs, self._mc_src_ptr_addr = zip(*[
                self._table([[self.in_plane(n, s, f).data_ptr() for n in self.in_names] for s in range(T)]) for f in self._mc_forcing])
            self._mc_dst_ptrs = torch.tensor([self.mc_scratch[n].data_ptr() for n in self.out_names], **i64)
            self._mc_dst_strides = torch.full((len(self.out_names),), self.HW, **i64)
        # Post-step physics as four HIP kernels per step (ace_amd/physics.py, csrc/physics.hip) instead of captured torch ops
        # (round 2: +29 % step time).  ACE_NO_FUSED_PHYSICS=1 keeps the torch ops (A/B).
        self._physics = None
        slab = self._ocean is not None and getattr(self._ocean, "is_slab", False)   # the fused kernel knows the prescribed SST only
        if (self._corrector is not None or self._ocean is not None or self.prescribed) and not slab and not os.environ.get("ACE_NO_FUSED_PHYSICS"):
            self._physics = self._build_physics()
        # corrector deltas (step_diagnostics.py): the uncorrected planes are copied aside between the unpack and the physics
        self._step_diagnostics = bool(step_diagnostics)
        self._recorder = self._build_recorder() if self._step_diagnostics else None
        self.net._ensure_native(dev, B)
        self.net.sync_weights()

    def _build_recorder(self):
        from .step_diagnostics import CorrectionDeltaRecorder, diagnosed_names
        names = diagnosed_names(self._corrector, self._ocean, self.out_names, self.prescribed)

        def locate(name, s):
            p = self.out_plane(name, s)
            return p.data_ptr(), p.stride(0)

        return CorrectionDeltaRecorder(names, self.B, (self.H, self.W), self.T, locate, self.device) if names else None

    def _build_physics(self):
        from .physics import FusedPhysics

        def locate(plane):      # (data_ptr, per-sample stride) of the plane, None for a name the window does not hold
            def at(name, s):
                try:
                    p = plane(name, s)
                except KeyError:
                    return None
                return p.data_ptr(), p.stride(0)
            return at

        return FusedPhysics(self._corrector, self._ocean, self.prescribed, self.B, (self.H, self.W), self.T,
                            gen_names=self.out_names, in_names=self.in_names,
                            next_names=self.forcing_names + self.target_names, locate_gen=locate(self.out_plane),
                            locate_in=locate(self.in_plane), locate_next=locate(self.next_plane), device=self.device)

    def _build_gmr(self, step):
        """The device tables of the fused global-mean removal (csrc/gmr.hip; include/ace_sfno.h "Global-mean removal"): the K
        reduced planes as indices into the pack's pointer-table row, the k of every shifted input / output channel, the
        climatological means and the synthetic channels' sources, the fp64 partials and the (B, K) shift buffer.  None when the
        stepper has no global-mean removal (or it processes nothing)."""
        gmr = getattr(step, "global_mean_removal", None)
        if gmr is None:
            return None
        from .global_mean_removal import SharedGlobalMeanRemoval, extra_channel_source_field
        if isinstance(gmr, SharedGlobalMeanRemoval):    # one offset, from the reference field, for every listed name
            reduced = [gmr.reference_field]
            k_of = {n: 0 for n in gmr.field_names}
        else:                                           # per channel: every processed input has its own
            reduced = [n for n in gmr.field_names if n in self.in_names]
            k_of = {n: k for k, n in enumerate(reduced)}
        # The secondary decoder's diagnostics are unpacked by their own launch, which knows no shift (cf. the force-positive clash)
        clash = sorted(set(k_of).intersection(self.sec_names))
        if clash:
            raise NotImplementedError(f"secondary-decoder diagnostics {clash} are un-shifted by global_mean_removal: use "
                                      "Stepper.predict for this configuration")
        if not reduced:
            return None
        dev, norm = self.device, step.normalizer
        i32 = dict(dtype=torch.int32, device=dev)
        sources = [extra_channel_source_field(n) for n in self.extra_names]
        stat = lambda table, names: torch.stack([table[n].to(dev) for n in names]).to(torch.float32).contiguous()   # noqa: E731
        K = len(reduced)
        return {
            "K": K,
            "planes": torch.tensor([self.in_names.index(n) for n in reduced], **i32),
            "in_idx": torch.tensor([k_of.get(n, -1) for n in self.in_names], **i32),
            "out_idx": torch.tensor([k_of.get(n, -1) for n in self.out_names], **i32),
            "clim": stat(norm.means, reduced),
            "extra_idx": torch.tensor([reduced.index(n) for n in sources], **i32) if sources else None,
            "extra_std": stat(norm.stds, sources) if sources else None,
            "partials": torch.zeros(self.B * K * int(_lib.lib().ace_gmr_chunks(self.HW)), dtype=torch.float64, device=dev),
            "shift": torch.zeros(self.B, K, dtype=torch.float32, device=dev),
        }

    # -- one step, enqueued on the current stream
    def _enqueue_step(self, s: int, use_library_graph: bool):
        L = _lib.lib()
        stream = _lib.current_stream()
        self._evaluate(L, stream, s, use_library_graph, self._src_ptr_addr[s], self._dst_ptr_addr[s], self._dst_strides, True)
        if self._recorder is not None:  # the network output of step s, before the corrector edits it in place
            self._recorder.snapshot(s, stream)
        if self._physics is not None:   # corrector -> ocean -> prescribed prognostics (single_module.py:669-716), four launches
            self._physics.apply(s, stream)
        elif self._corrector is not None or self._ocean is not None or self.prescribed:
            gen = {n: self.out_plane(n, s) for n in self.out_names}
            new, self._corrector_state = self._post_step(s, self.forcing, gen, self._corrector_state)
            for n in self.out_names:
                if new[n] is not gen[n] and n not in self.prescribed:
                    gen[n].copy_(new[n])
            for n in self.prescribed:
                gen[n].copy_(new[n])
        if self._mc is not None:
            self._multi_call_step(L, stream, s, use_library_graph)

    def _evaluate(self, L, stream, s: int, use_library_graph: bool, src: int, dst: int, dst_strides: torch.Tensor, secondary: bool):
        """Pack -> forward -> unpack of window position s: the inputs from the planes of the pointer table row `src`, the outputs
        into those of `dst` (and, with `secondary`, the secondary decoder's diagnostics into their output planes)."""
        if self._gmr is not None:
            # forward_transform + normalize + pack (single_module.py:651-659): the shifts of THIS evaluation's inputs - a multi-call
            # re-evaluation with a scaled forcing has its own - reduced in one launch, applied by the pack
            g = self._gmr
            nin, nextra = len(self.in_names), len(self.extra_names)
            _lib.check(L.ace_gmr_partials(src, self._src_stride_addr[s], g["planes"].data_ptr(), nin, g["partials"].data_ptr(),
                                          self.B, g["K"], self.HW, stream))
            _lib.check(L.ace_gmr_pack_normalize(src, self._src_stride_addr[s], self.in_mean.data_ptr(), self.in_std.data_ptr(),
                                                g["in_idx"].data_ptr(), g["partials"].data_ptr(), g["clim"].data_ptr(),
                                                g["extra_idx"].data_ptr() if nextra else None,
                                                g["extra_std"].data_ptr() if nextra else None, self.x.data_ptr(),
                                                g["shift"].data_ptr(), self.B, nin, nextra, g["K"], self.HW, stream))
        else:
            _lib.check(L.ace_pack_normalize(src, self._src_stride_addr[s], self.in_mean.data_ptr(), self.in_std.data_ptr(),
                                            self.x.data_ptr(), self.B, len(self.in_names), self.HW, stream))
        if self._fill_in:
            _nan_to_zero(self.x)
        if self._conditioned:   # NoiseConditionedSFNO: fresh conditioning noise every evaluation (stochastic_sfno.py:128-146), merged
            if self.graph_mode == "window":      # drawn for the whole window by _draw_window_conditioning(), static address per step
                noise = self._cond_window[s]
            else:
                noise = self.net.conditioning_field(self.B, self.device, labels=self._labels)   # with the label / positional context
            _lib.check(L.ace_sfno_forward_conditioned(self.net._native, self.x.data_ptr(), noise.data_ptr(), self.y.data_ptr(),
                                                      self.B, stream))
        else:
            fwd = L.ace_sfno_forward_graph if use_library_graph else L.ace_sfno_forward
            _lib.check(fwd(self.net._native, self.x.data_ptr(), self.y.data_ptr(), self.B, stream))
        if secondary and self._secondary is not None:   # from the raw network output, before the residual (single_module.py:430-434)
            sec = self._secondary._module(self.y).contiguous()
            _lib.check(L.ace_unpack_denormalize(sec.data_ptr(), self.sec_mean.data_ptr(), self.sec_std.data_ptr(),
                                                self._sec_dst_ptr_addr[s], self._sec_dst_strides.data_ptr(),
                                                self.B, len(self.sec_names), self.HW, stream))
        self._unpack(L, stream, self.y, dst, dst_strides)

    def _multi_call_step(self, L, stream, s: int, use_library_graph: bool):
        """_multi_call.py:164-188 on the static buffers: the step of window position s evaluated again with the scaled forcing - same
        x / y buffers as the plain evaluation (whose outputs are already unpacked), outputs into scratch planes, the post-step hooks
        as torch ops on them (their corrector state is seeded like the plain path's and never fed back), selected fields copied."""
        hooked = self._corrector is not None or self._ocean is not None or self.prescribed
        for k, forcing in enumerate(self._mc_forcing):
            self._evaluate(L, stream, s, use_library_graph, self._mc_src_ptr_addr[k][s], self._mc_dst_ptrs.data_ptr(),
                           self._mc_dst_strides, False)
            gen = {n: self.mc_scratch[n][:, 0] for n in self.out_names}
            if hooked:
                gen, state = self._post_step(s, forcing, gen, self._mc_state)
                if self._mc_state is None:
                    self._mc_state = state
            for src_name, dst_name in self._mc_copy[k]:
                self.out[dst_name][:, s].copy_(gen[src_name])

    def _post_step(self, s: int, forcing, gen, state):
        """step_with_adjustments' tail (fme/core/step/single_module.py:669-716) as torch ops: corrector -> ocean -> prescribed
        prognostics on the outputs `gen` of window position s, reading its inputs and next-step data with `forcing` as the forcing
        buffers.  Returns the new fields and corrector state."""
        inp = {n: self.in_plane(n, s, forcing) for n in self.prognostic + self.forcing_names}
        nxt = {n: self.next_plane(n, s, forcing) for n in self.forcing_names + self.target_names}
        new = gen
        if self._corrector is not None:
            if self.graph_mode == "window" and "conserve_dry_air" in self._corrector.corrections:
                state = self._captured_reference(inp, state)
            new, state = self._corrector(inp, new, nxt, state)
        if self._ocean is not None:
            new = self._ocean(inp, new, nxt)
        for n in self.prescribed:     # after the ocean (single_module.py:700-716): the data of step s + 1
            new = {**new, n: nxt[n]}
        return new, state

    def _captured_reference(self, inp, state):
        """graph="window": the dry-air reference mass in its static buffer - the carried or first seeded one, selected on the device"""
        from .corrector import CorrectorState, _seed_global_dry_air_mass
        c = self._corrector
        seeded = _seed_global_dry_air_mass(inp, None, c._mean, c._vcoord(self.device), torch.float64).global_dry_air_mass
        if self._ref_mass is None:
            self._ref_mass = torch.zeros_like(seeded)
            self._have_ref = torch.zeros((), dtype=torch.bool, device=self.device)
            if state is not None and state.global_dry_air_mass is not None:
                self._ref_mass.copy_(state.global_dry_air_mass)
                self._have_ref.fill_(True)
        self._ref_mass.copy_(torch.where(self._have_ref, self._ref_mass, seeded))
        self._have_ref.fill_(True)
        return CorrectorState(global_dry_air_mass=self._ref_mass)

    def set_labels(self, labels) -> None:
        """Labels of a conditional module (fme/core/labels.py BatchLabels, or a (B, n_labels) tensor already in the module's
        encoding) for the following windows; conformed to the module's LabelEncoding as Module.__call__ does."""
        if labels is None:
            self._labels = None
            return
        enc = getattr(self.stepper._step_obj.module, "_label_encoding", None)
        if hasattr(labels, "conform_to_encoding"):
            if enc is None:
                raise TypeError("Labels are not allowed for unconditional models")
            labels = labels.conform_to_encoding(enc).tensor
        self._labels = labels.to(device=self.device, dtype=torch.float32).contiguous()
        if self._labels.shape[0] != self.B:
            raise ValueError(f"labels for {self._labels.shape[0]} samples, engine batch is {self.B}")

    def load(self, initial_condition: Mapping[str, torch.Tensor], forcing: Mapping[str, torch.Tensor]):
        super().load(initial_condition, forcing)
        self._after_load()

    def _after_load(self):
        """What a freshly loaded window resets besides its buffers."""
        self._corrector_state = None        # a new initial condition re-seeds the corrector
        self._mc_state = None
        if self._mc is not None:
            for k, (_, factor) in enumerate(self._mc_factors):
                torch.mul(self.forcing[self._mc.forcing_name], factor, out=self.forcing_mc[k])
        if self._have_ref is not None:
            self._have_ref.fill_(False)
        if self._physics is not None and self._physics.tracks_dry_air:
            self._physics.reset(_lib.current_stream())

    def set_random_state(self, random_state) -> None:
        """``ace_amd.rand.RandomState`` (or None: the global RNG) the conditioning noise of the following windows is drawn from."""
        self._random_state = random_state

    def _draw_window_conditioning(self):
        """graph="window": the conditioning fields of the T steps, drawn now (through fme.core.rand's contract: the active CPU
        generator of a seeded rollout, else the device RNG) in step order and copied into the static buffer the captured steps read"""
        for s in range(self.T):
            field = self.net.conditioning_field(self.B, self.device, labels=self._labels)
            if self._cond_window is None:
                nbytes = 4 * self.T * field.numel()
                if nbytes > self.max_window_conditioning_bytes:
                    raise RuntimeError(f"graph='window' would hold {nbytes / 2**30:.1f} GiB of conditioning fields ({self.T} steps x "
                                       f"{tuple(field.shape)} fp32) in device memory; use graph='step' (the same captured step, one "
                                       f"draw per replay) or raise RolloutEngine.max_window_conditioning_bytes")
                self._cond_window = torch.empty(self.T, *field.shape, dtype=torch.float32, device=self.device)
            self._cond_window[s].copy_(field)

    def run_window(self):
        """Enqueue the T steps of the window on the current stream (no host synchronisation)."""
        from .rand import use_generator
        with use_generator(None if self._random_state is None else self._random_state.generator):
            if self._conditioned and self.graph_mode == "window":
                self._draw_window_conditioning()
            super().run_window()
        self._after_window()

    def _after_window(self):
        if self._recorder is not None:  # one launch per window, after the replay: the snapshots become out - snapshot
            self._recorder.finish_window(_lib.current_stream())
        if self.graph_mode == "window" and self._have_ref is not None and self._physics is None:
            # host-side view of the hook state the captured region keeps in its static buffer (a replay does not run
            # the Python that set it at capture time); a copy, so that a state handed out survives the next load()
            from .corrector import CorrectorState
            self._corrector_state = CorrectorState(global_dry_air_mass=self._ref_mass.clone())

    def _prepare_window(self):
        # parameters changed since the last window (load_state_dict / stepper.load_state): upload them; the library drops
        # its captured per-step graphs itself, the window graph captured here is dropped too
        self.net.sync_weights()
        step = self.stepper._step_obj   # Stepper.replace_ocean / overrides after construction take effect here
        if step._ocean is not self._ocean or step._corrector is not self._corrector:
            # The engine's forcing / target name sets and static buffers were laid out for the ocean it was built with: a
            # replacement that reads other fields (a slab ocean's q_flux / mixed-layer depth, an SST the old configuration did not
            # prescribe) or that the fused kernels do not know cannot be swapped in - ask for a new engine instead of failing
            # mid-run on a missing buffer.
            new_ocean = step._ocean
            needed = set(getattr(new_ocean, "forcing_names", None) or [])      # ace_amd.ocean.Ocean.forcing_names, however it was swapped in
            missing = sorted(needed - set(self.forcing_names) - set(self.target_names))
            if missing or (self._physics is not None and new_ocean is not None and getattr(new_ocean, "is_slab", False)):
                raise RuntimeError("the stepper's ocean was replaced after this RolloutEngine was built and the new one needs fields / "
                                   f"a path the engine's static buffers were not laid out for ({missing or 'slab ocean with fused physics'}): "
                                   "build a new RolloutEngine for the modified stepper")
            self._ocean, self._corrector = step._ocean, step._corrector
            self._window_graph = None
            if self._physics is not None:
                self._physics = self._build_physics()
            if self._step_diagnostics:      # the new corrector writes other names
                self._recorder = self._build_recorder()
        # The captured forwards hold scalars derived from the weights by value (ace_sfno_set_weight): whoever uploaded last -
        # this call, net.forward, Stepper.predict, another engine on the same net - the library's generation counter tells.
        return (int(self.net._native.value or 0) if hasattr(self.net._native, "value") else int(self.net._native),
                int(_lib.lib().ace_sfno_weights_generation(self.net._native)))

    def predict(self, initial_condition, forcing, time=None):
        """``WindowEngine.predict``; with ``step_diagnostics`` the outputs come back as a ``WindowData`` carrying the window's deltas."""
        out, state = super().predict(initial_condition, forcing, time)
        if not self._step_diagnostics:
            return out, state
        from .step_diagnostics import WindowData
        diags = self._recorder.step_diagnostics() if self._recorder is not None else None
        return WindowData(out, step_diagnostics=diags), state

    def _carry_in(self, carried):
        carried_random = getattr(carried, "random_state", None)
        if carried_random is not None:      # a state that carries only the corrector's part keeps set_random_state()'s generator
            self._random_state = carried_random
        if carried is not None:
            cs = self._mc_state = self._corrector_state = carried.corrector_state
            if self._have_ref is not None and cs is not None and cs.global_dry_air_mass is not None:
                self._ref_mass.copy_(cs.global_dry_air_mass)     # carried reference: the captured region keeps it
                self._have_ref.fill_(True)
            if self._physics is not None and self._physics.tracks_dry_air and cs is not None and cs.global_dry_air_mass is not None:
                self._physics.set_reference(cs.global_dry_air_mass, _lib.current_stream())

    def _carry_out(self, carried):
        from .step import StepperState
        if self._physics is not None and self._physics.tracks_dry_air:
            from .corrector import CorrectorState
            mass = self._physics.get_reference(_lib.current_stream())   # (synchronises: once per window, with the result)
            self._corrector_state = CorrectorState(global_dry_air_mass=mass) if mass is not None else None
        if self._corrector_state is not None or self._random_state is not None:
            return StepperState(corrector_state=self._corrector_state, random_state=self._random_state)
        return None
