"""What more than one metric family of the evaluator uses, and the window handed to every family."""
from typing import Callable, Dict, List, Mapping, Optional, Sequence

import torch


class Window:
    """One paired window as every family's ``record`` gets it: ``gen`` and ``tgt`` name -> (B, T, H, W) (with contiguous planes
    when ``fused``), the time index of its first step, its ``TimeAxis`` or None, ``with_maps`` False for the initial condition
    (which feeds the time series only) and whether the HIP kernels or the torch ops take it."""

    def __init__(self, gen: Dict[str, torch.Tensor], tgt: Dict[str, torch.Tensor], i_time_start: int, time, with_maps: bool,
                 fused: bool, normalize: Optional[Callable]):
        self.gen, self.tgt, self.i_time_start, self.time, self.with_maps, self.fused = gen, tgt, i_time_start, time, with_maps, fused
        first = next(iter(gen.values()))
        self.device, (self.B, self.T), self.HW = first.device, first.shape[:2], first.shape[-2] * first.shape[-1]
        self._normalize, self._norm = normalize, None

    def kind(self, kind: str):
        """(gen, tgt) as they came ("denorm") or normalised ("norm", main.py:594-598: formed when first asked for, once)"""
        if kind == "denorm":
            return self.gen, self.tgt
        if self._norm is None:
            self._norm = (self._normalize(self.gen), self._normalize(self.tgt))
        return self._norm


def _only(d: Mapping[str, torch.Tensor], variables: Optional[Sequence[str]]) -> List[str]:
    """maybe_filter (build_context.py:19-46): the names of ``d`` a metric's ``variables`` keeps"""
    return [n for n in d if variables is None or n in variables]


def _check_time(time, B: int, T: int) -> None:
    if tuple(time.shape) != (B, T):
        raise ValueError(f"time must be (samples, steps) = {(B, T)}, got {tuple(time.shape)}")


def _wmean(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """metrics.py:63-90 over the last two dimensions"""
    w = w.expand(x.shape)
    return (x.where(w != 0.0, 0.0) * w).sum(dim=(-2, -1)) / w.sum(dim=(-2, -1))


def _wstd(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """metrics.py:118-143"""
    return _wmean((x - _wmean(x, w)[..., None, None]) ** 2, w).sqrt()


def _channel_mean(values: Mapping[str, float], own: Optional[Sequence[str]], fallback: Optional[Sequence[str]],
                  nan_targets) -> Optional[float]:
    """reduced_metrics.py:76-116 and ensemble.py:313-332: the mean of ``values`` over ``own`` names, else ``fallback``, else all,
    without the names whose target is all NaN; a name that is not present raises KeyError; None when no name is left"""
    names = own or fallback
    if names is None:
        names = list(values)
    missing = [n for n in names if n not in values]
    if missing:
        raise KeyError(f"channel_mean_names contains entries not present in the recorded data: {missing}. "
                       f"Available: {sorted(values)}.")
    names = [n for n in names if n not in nan_targets]
    return sum(values[n] for n in names) / len(names) if names else None
