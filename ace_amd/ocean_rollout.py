"""OceanRolloutEngine: the stepper loop of a Samudra ocean stepper (fme/ace/stepper/single_module.py:1045-1075, 1124-1167) on
static HBM buffers, with the static spatial masking and the ocean corrector fused around the network.

Per step s the engine enqueues, in the order of ``Stepper.step`` and ``step_with_adjustments``:
  1. ace_mask_pack_normalize  the step's inputs (previous output or the initial condition, the forcing at s or s + 1 for
                              next_step_forcing_names) masked with the input masker's fill and normalised into the packed
                              network input; the masked inputs and next-step forcings the corrector reads are staged on the way
                              (unmasked or excluded planes are read where they lie)
  2. the Samudra forward      (`graph="step"`: a captured forward replayed; `graph="window"`: all T steps in one torch graph;
                              `graph=None`: eager launches)
  3. ace_unpack_denormalize   network output -> out[name][:, s] (residual_prediction adds the normalised prognostic inputs first)
  4. ace_ocean_phys_*         the ocean corrector (O1, plus O2 with the heat-content budget), in place on out[:, s], reading the
                              masked input and the masked next-step forcing; with a sea-ice corrector ace_ice_budget_apply instead
                              (its flags stay on the device: no readback, so the step is capturable)
  5. ace_mask_planes          the provider's output masker (NaN where the mask is 0), in place on out[:, s], which is also the
                              state of step s + 1
Every handle, hit plane and workspace is made at construction or in a warm-up outside capture; nothing is allocated and the host
never synchronises inside a window.  The masking kernels only select (their hit planes are computed with the reference's own
torch expression), the corrector and the glue are the kernels ``Stepper.predict`` runs, so the engine differs from it only by the
normalisation's rounding (torch division against ``__fdiv_rn``) - see tests/test_gpu_ocean_rollout.py.
The buffers, the window layout, the tail of the forward (3.), the graph modes and load / predict are rollout.WindowEngine's."""

from typing import Optional

import torch

from . import _lib
from .rollout import MaskedWindowEngine, _nan_to_zero
from .stepper import Stepper


class _Reads(dict):
    """A dict that records the keys read from it (which input / forcing planes the corrector resolves)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.read = set()

    def __getitem__(self, key):
        self.read.add(key)
        return super().__getitem__(key)

    def get(self, key, default=None):
        if key in self:
            self.read.add(key)
        return super().get(key, default)


def _refuse(what: str) -> NotImplementedError:
    return NotImplementedError(f"OceanRolloutEngine: {what}; run this stepper through Stepper.predict")


class OceanRolloutEngine(MaskedWindowEngine):
    @staticmethod
    def check_supported(stepper: Stepper):
        """The refusals that need no device, raised before any device work (the constructor's first act).  Returns the stepper's
        (input masker, output masker), each None when it is no static spatial masking."""
        from .ice_corrector import IceCorrector
        from .ocean_corrector import OceanCorrector
        from .samudra import Samudra
        step = stepper._step_obj
        cfg = step.config
        net = step.module.torch_module
        if getattr(step, "global_mean_removal", None) is not None:      # whatever the module: the fused masking pack knows no shift
            raise _refuse("global_mean_removal is not supported")
        if not isinstance(net, Samudra):
            if hasattr(net, "_ensure_native"):      # the SFNO family
                raise NotImplementedError(f"OceanRolloutEngine runs Samudra steppers; a {type(net).__name__} stepper runs through "
                                          "RolloutEngine (or Stepper.predict)")
            raise _refuse(f"the module is a {type(net).__name__}, not Samudra")
        if getattr(stepper, "_multi_call_config", None) is not None:
            raise _refuse("multi-call diagnostics are not supported")
        if getattr(step, "secondary_decoder", None) is not None:
            raise _refuse("a secondary decoder is not supported")
        if getattr(step.module, "_label_encoding", None) is not None:
            raise _refuse("a label-conditioned module is not supported")
        if step._ocean is not None or cfg.ocean is not None:
            raise _refuse("an atmosphere `ocean` configuration (prescribed SST / slab ocean) is not supported")
        if list(cfg.prescribed_prognostic_names):
            raise _refuse("prescribed prognostic names are not supported")
        corrector = step._corrector
        if corrector is not None and not isinstance(corrector, (OceanCorrector, IceCorrector)):
            raise _refuse(f"a {type(corrector).__name__} is not an ocean corrector (nor a sea-ice corrector)")
        in_mask, out_mask = MaskedWindowEngine._static_maskers(stepper, _refuse)
        if next(net.parameters()).device.type != "cuda":
            raise RuntimeError("OceanRolloutEngine runs on an MI355X: load the stepper onto a 'cuda' device (there is no CPU path)")
        return in_mask, out_mask

    def __init__(self, stepper: Stepper, batch: int, n_forward_steps: int, graph: Optional[str] = "step",
                 step_diagnostics: bool = False):
        if step_diagnostics:
            raise NotImplementedError("OceanRolloutEngine: step_diagnostics (the corrector deltas) are built for the atmosphere "
                                      "corrector on RolloutEngine only, not for the ocean corrector")
        self._check_graph(graph)
        in_mask, out_mask = self.check_supported(stepper)
        step = stepper._step_obj
        net = step.module.torch_module
        corrector = step._corrector

        super().__init__(stepper, net, batch, n_forward_steps, graph)
        dev, B, T, H, W, HW = self.device, batch, n_forward_steps, self.H, self.W, self.HW
        f32 = dict(dtype=torch.float32, device=dev)

        # ---- the corrector: which masked planes it reads (probed once on the unmasked views), staged by the pack
        in_plan = in_mask.plan(self.in_names) if in_mask is not None else [(None, None)] * len(self.in_names)
        in_masked = {n for n, (k, _) in zip(self.in_names, in_plan) if k is not None}
        self._corrector = corrector
        self._fused_corrector = None
        stage_in, stage_next = [], []
        if corrector is not None and corrector.corrections:
            from .ice_corrector import FusedIceCorrector, IceCorrector
            from .ocean_phys import FusedOceanCorrector
            diag = [n for n in self.out_names if n not in self.in_names]
            inp = _Reads({**{n: self.in_plane(n, 0) for n in self.in_names}, **{n: self.out_plane(n, 0) for n in diag}})
            nxt = _Reads({n: self.next_plane(n, 0) for n in self.forcing_names})
            gen = {n: self.out_plane(n, 0) for n in self.out_names}
            try:
                # both fused handles have fields(inp, gen, nxt) -> a struct of planes and apply(struct, stream)
                fc = (FusedIceCorrector if isinstance(corrector, IceCorrector) else FusedOceanCorrector)(corrector, B, (H, W), dev)
                fc.fields(inp, gen, nxt)
            except (ValueError, KeyError, TypeError, NotImplementedError) as e:
                raise _refuse(f"the {type(corrector).__name__} configuration is not supported by the fused corrector ({e})") from e
            read_diag = sorted(inp.read.intersection(diag))
            if read_diag:
                raise _refuse(f"the ocean corrector reads the step outputs {read_diag} from the input, which only a step after the "
                              "first holds")
            self._fused_corrector = fc
            stage_in = [n for n in self.in_names if n in inp.read and n in in_masked]
            stage_next = [n for n in self.forcing_names if n in nxt.read and in_mask is not None and in_mask.plan((n,))[0][0] is not None]
        self.stage = {n: torch.zeros(B, H, W, **f32) for n in stage_in}
        # a next-step forcing that is also this step's input (next_step_forcing_names) is the same masked plane: staged once
        self.stage_next = {n: (self.stage[n] if n in self.stage and n in self.next_step_forcing else torch.zeros(B, H, W, **f32))
                           for n in stage_next}
        extra = [n for n in stage_next if self.stage_next[n] is not self.stage.get(n)]

        # ---- step tables of ace_mask_pack_normalize: planes = the inputs (packed), then the extra staged next-step planes
        planes = self.in_names + extra
        self._nplanes = n = len(planes)
        self._build_input_mask(in_mask, planes)
        rows = []
        for s in range(T):
            srcs = [self.in_plane(o, s) for o in self.in_names] + [self.next_plane(o, s) for o in extra]
            stages = [self.stage.get(o) for o in self.in_names] + [self.stage_next[o] for o in extra]
            rows.append([t.data_ptr() for t in srcs] + [t.stride(0) if B > 1 else HW for t in srcs]
                        + [t.data_ptr() if t is not None else 0 for t in stages] + [HW] * len(stages))
        self._pack_tab, addr = self._table(rows)
        self._pack_addr = [(a, a + 8 * n, a + 16 * n, a + 24 * n) for a in addr]

        # ---- the corrector's planes per step (static: resolved once)
        self._fields = []
        if self._fused_corrector is not None:
            for s in range(T):
                inp = {o: (self.stage[o] if o in self.stage else self.in_plane(o, s)) for o in self.in_names}
                nxt = {o: (self.stage_next[o] if o in self.stage_next else self.next_plane(o, s)) for o in self.forcing_names}
                gen = {o: self.out_plane(o, s) for o in self.out_names}
                self._fields.append(self._fused_corrector.fields(inp, gen, nxt))

        # ---- the output masker, in place on out[:, s]
        self._build_output_mask(out_mask)

        self._captured = None          # graph="step": CapturedSamudraForward on self.x

    # -- one step, enqueued on the current stream
    def _enqueue_step(self, s: int, replay_forward: bool):
        L = _lib.lib()
        stream = _lib.current_stream()
        srcs, src_strides, stage, stage_strides = self._pack_addr[s]
        self._mask_pack_normalize(L, stream, srcs, src_strides, stage, stage_strides, self._nplanes)
        if self._fill_in:
            _nan_to_zero(self.x)
        if replay_forward:
            self._captured.graph.replay()
            y = self._captured.y
        else:
            y = self.net(self.x)
        self._unpack(L, stream, y, self._dst_ptr_addr[s], self._dst_strides)
        if self._fused_corrector is not None:
            self._fused_corrector.apply(self._fields[s], stream)
        self._mask_outputs(L, stream, s)

    def _prepare_window(self):
        step = self.stepper._step_obj
        if step._corrector is not self._corrector or step._ocean is not None:
            raise RuntimeError("the stepper's corrector / ocean was replaced after this OceanRolloutEngine was built: build a new one")
        # the parameters a captured graph was made with: a change (load_state) drops the graphs holding the old weight handles
        key = tuple((t.data_ptr(), t._version) for t in list(self.net.parameters()) + list(self.net.buffers()))
        if self.graph_mode == "step" and (self._captured is None or key != self._graph_key):
            from .samudra import CapturedSamudraForward
            self._captured = CapturedSamudraForward(self.net, self.x)       # warm-up outside capture, then capture
            self.x = self._captured.x
        return key
