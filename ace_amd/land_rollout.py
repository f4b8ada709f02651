"""LandRolloutEngine: the stepper loop of a LandNet land stepper (fme/ace/stepper/single_module.py:1045-1075, 1124-1167) on static
HBM buffers - the counterpart of OceanRolloutEngine for the per-pixel family.

Per step s the engine enqueues, in the order of ``Stepper.step`` and ``step_with_adjustments``:
  1. ace_mask_pack_normalize  the step's inputs (previous output or the initial condition, the forcing at s or s + 1 for
                              next_step_forcing_names) masked with the input masker's fill and normalised into the packed input
  2. ace_pixel_mlp_forward    the whole network, one launch (`graph="step"`: that launch replayed from a captured graph;
                              `graph="window"`: all T steps in one torch graph; `graph=None`: eager launches)
  3. ace_unpack_denormalize   network output -> out[name][:, s] (residual_prediction adds the normalised prognostic inputs first)
  4. ace_mask_planes          the provider's output masker (NaN where the mask is 0), in place on out[:, s], which is also the
                              state of step s + 1
Nothing is allocated and the host never synchronises inside a window.  No corrector runs here: a land stepper with one goes
through ``Stepper.predict``.  The buffers, the window layout, the tail of the forward (3.), the graph modes and load / predict
are rollout.WindowEngine's; the masking tables and their two launches are rollout.MaskedWindowEngine's, shared with the ocean engine."""

from typing import Optional

import torch

from . import _lib
from .rollout import MaskedWindowEngine, _nan_to_zero
from .stepper import Stepper


def _refuse(what: str) -> NotImplementedError:
    return NotImplementedError(f"LandRolloutEngine: {what}; run this stepper through Stepper.predict")


def _on_gpu(net) -> bool:
    return next(net.parameters()).device.type == "cuda"


class _CapturedForward:
    """graph="step": the one launch of the forward from x into y, captured after a warm-up (which prepares the weight handle)."""

    def __init__(self, net, x: torch.Tensor, y: torch.Tensor):
        side = torch.cuda.Stream(device=x.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net.forward_into(x, y)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with _lib.capture_without_gc(), torch.cuda.graph(self.graph):
            net.forward_into(x, y)


class LandRolloutEngine(MaskedWindowEngine):
    @staticmethod
    def check_supported(stepper: Stepper):
        """The refusals that need no device, raised before any device work (the constructor's first act).  Returns the stepper's
        (input masker, output masker), each None when it is no static spatial masking."""
        from .landnet import LandNet
        step = stepper._step_obj
        cfg = step.config
        net = step.module.torch_module
        corrector = step._corrector
        if corrector is not None:       # whatever it would correct: _prepare_window holds the stepper to "no corrector"
            raise _refuse(f"a corrector ({type(corrector).__name__}: {', '.join(getattr(corrector, 'corrections', None) or [])}) is not supported")
        if step._ocean is not None or cfg.ocean is not None:
            raise _refuse("an `ocean` configuration (prescribed SST / slab ocean) is not supported")
        if getattr(step, "global_mean_removal", None) is not None:
            raise _refuse("global_mean_removal is not supported")
        if getattr(stepper, "_multi_call_config", None) is not None:
            raise _refuse("multi-call diagnostics are not supported")
        if getattr(step, "secondary_decoder", None) is not None:
            raise _refuse("a secondary decoder is not supported")
        if getattr(step.module, "_label_encoding", None) is not None:
            raise _refuse("a label-conditioned module is not supported")
        if list(cfg.prescribed_prognostic_names):
            raise _refuse("prescribed prognostic names are not supported")
        if not isinstance(net, LandNet):
            raise _refuse(f"the module is a {type(net).__name__}, not LandNet")
        in_mask, out_mask = MaskedWindowEngine._static_maskers(stepper, _refuse)
        if not _on_gpu(net):
            raise RuntimeError("LandRolloutEngine runs on an MI355X: load the stepper onto a 'cuda' device (there is no CPU path)")
        return in_mask, out_mask

    def __init__(self, stepper: Stepper, batch: int, n_forward_steps: int, graph: Optional[str] = "step",
                 step_diagnostics: bool = False):
        if step_diagnostics:
            raise NotImplementedError("LandRolloutEngine: step_diagnostics (the corrector deltas) are built for the atmosphere "
                                      "corrector on RolloutEngine only; this engine runs no corrector")
        self._check_graph(graph)
        in_mask, out_mask = self.check_supported(stepper)
        step = stepper._step_obj
        net = step.module.torch_module
        super().__init__(stepper, net, batch, n_forward_steps, graph)
        dev, B, T, H, W, HW = self.device, batch, n_forward_steps, self.H, self.W, self.HW
        self.y = torch.zeros(B, len(self.out_names), H, W, dtype=torch.float32, device=dev)       # network output (normalised)

        # ---- step tables of ace_mask_pack_normalize: the inputs, all packed, none staged
        n = len(self.in_names)
        self._build_input_mask(in_mask, self.in_names)
        rows = []
        for s in range(T):
            srcs = [self.in_plane(o, s) for o in self.in_names]
            rows.append([t.data_ptr() for t in srcs] + [t.stride(0) if B > 1 else HW for t in srcs])
        self._pack_tab, addr = self._table(rows)
        self._pack_addr = [(a, a + 8 * n) for a in addr]

        # ---- the output masker, in place on out[:, s]
        self._build_output_mask(out_mask)

        self._captured = None          # graph="step": _CapturedForward on (self.x, self.y)

    # -- one step, enqueued on the current stream
    def _enqueue_step(self, s: int, replay_forward: bool):
        L = _lib.lib()
        stream = _lib.current_stream()
        srcs, src_strides = self._pack_addr[s]
        self._mask_pack_normalize(L, stream, srcs, src_strides, None, None, len(self.in_names))
        if self._fill_in:
            _nan_to_zero(self.x)
        if replay_forward:
            self._captured.graph.replay()
        else:
            self.net.forward_into(self.x, self.y)
        self._unpack(L, stream, self.y, self._dst_ptr_addr[s], self._dst_strides)
        self._mask_outputs(L, stream, s)

    def _prepare_window(self):
        step = self.stepper._step_obj
        if step._corrector is not None or step._ocean is not None:
            raise RuntimeError("the stepper's corrector / ocean was replaced after this LandRolloutEngine was built: build a new one")
        # the parameters a captured graph was made with: a change (load_state) drops the graphs holding the old weight handle
        key = self.net._stamp()
        if self.graph_mode == "step" and (self._captured is None or key != self._graph_key):
            self._captured = _CapturedForward(self.net, self.x, self.y)      # warm-up outside capture, then capture
        return key
