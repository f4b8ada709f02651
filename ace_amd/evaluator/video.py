"""The ``video`` metric of the evaluator (``_Video``) and ``video_frames``, the frames the reference hands to its logger.

Accumulator memory: names x n_timesteps x H x W x 16 bytes for the basic videos (two fp64 means per slot and pixel), x 48 with
``enable_extended_videos`` (five fp64 sums and two fp32 extrema); 8 names, 1460 steps, 1 degree: 6.1 GB / 18.2 GB.  It is compared
with ``video_max_bytes`` before anything is allocated or grown; ``VideoMetricConfig.variables`` keeps it in bounds."""
import math
from typing import Any, Dict, List

import numpy as np
import torch

from ..aggregator import _check, _grow_rows, _upload_planes
from .common import _only


class _Video:
    """``video`` (VideoAggregator, video.py:290-472): per time index of the inference and per pixel, the mean over the samples of
    the prediction and of the target and, with ``enable_extended_videos``, the bias, the RMSE over the samples, the smallest and
    the largest error and the prediction's variance over the samples as a fraction of the target's.  A time index a window visits
    more than once averages its visits (video.py:155-171).

    The torch path states the reference's formulas in the reference's dtypes (fp32 means over the samples added into fp64
    accumulators; the extrema, fp32 values, are kept in fp32), with the accumulators on the fields' device where the reference
    moves every result to the host.  The fused path makes one ``ace_diag_video_window`` per window for all kept names and both
    sides (csrc/video.hip; the header contract in include/ace_sfno.h): fp64 sums over the samples, rounded once.  The visit
    counts stay on the host; a window none of whose slots has been visited is assigned, not accumulated.

    A prediction name without a target is recorded on the generated side only: the target half of ``<name>`` is NaN and its five
    extended keys are absent.  A name keeps that state: a target that appears or disappears between windows is refused."""
    needs_norm = False
    counted = True                                                        # its calls are part of ``launches()``
    needs_time = uses_time = False

    def __init__(self, agg, cfg, max_bytes: int):
        self._agg, self.cfg, self._max_bytes = agg, cfg, int(max_bytes)
        self.extended = bool(cfg.enable_extended_videos)
        self._n = np.zeros(agg._n_time, np.int64)                         # visits per time index (video.py: _n_batches)
        self._pairs: Dict[str, bool] = {}                                 # kept name -> whether it has a target, in order seen
        # torch path: channel -> name -> (n_time, H, W)
        self._t: Dict[str, Dict[str, torch.Tensor]] = {}
        # fused path: _mean (2, rows, n_time, H W) fp64, _sq (3, rows, n_time, H W) fp64, _err (2, rows, n_time, H W) fp32
        self._rows: Dict[str, int] = {}
        self._mean = self._sq = self._err = None

    def _bytes(self, names: int) -> int:
        H, W = self._agg._shape
        return names * self._agg._n_time * H * W * (48 if self.extended else 16)

    def _admit(self, w) -> List[str]:
        """the kept names of a window, after the checks that come before any allocation"""
        t0, T, n_time = w.i_time_start, w.T, self._agg._n_time
        if t0 < 0 or t0 + T > n_time:
            raise ValueError(f"steps {t0}..{t0 + T - 1} are past the video's n_timesteps {n_time}")
        names = _only(w.gen, self.cfg.variables)
        for n in names:
            if self._pairs.get(n, n in w.tgt) != (n in w.tgt):
                raise ValueError(f"the video of '{n}' was started {'with' if self._pairs[n] else 'without'} a target; a later "
                                 "window must keep that")
        count = len(self._pairs) + sum(n not in self._pairs for n in names)
        need = self._bytes(count)
        if need > self._max_bytes:
            H, W = self._agg._shape
            raise ValueError(
                f"the video accumulators need {need} bytes = {count} names x {n_time} steps x {H} x {W} x "
                f"{48 if self.extended else 16} bytes, above video_max_bytes = {self._max_bytes}; keep fewer names with "
                "VideoMetricConfig.variables, or record fewer steps")
        self._pairs.update({n: n in w.tgt for n in names})
        return names

    def record(self, w) -> int:
        names = self._admit(w)
        made = (self._record_fused if w.fused else self._record_torch)(w, names)
        self._n[w.i_time_start:w.i_time_start + w.T] += 1
        return made

    # ---- the torch path -----------------------------------------------------------------------------------------------
    def _buffer(self, channel: str, name: str, like: torch.Tensor, fill: float = 0.0, dtype=torch.float64) -> torch.Tensor:
        d = self._t.setdefault(channel, {})
        if name not in d:
            d[name] = torch.full((self._agg._n_time, *like.shape[-2:]), fill, dtype=dtype, device=like.device)
        return d[name]

    def _record_torch(self, w, names) -> int:
        sl = slice(w.i_time_start, w.i_time_start + w.T)
        for n in names:
            g, y = w.gen[n], w.tgt.get(n)
            self._buffer("gen", n, g)[sl] += g.mean(dim=0)                # video.py:150-153
            if self.extended:
                self._buffer("gen_sq", n, g)[sl] += (g ** 2).mean(dim=0)  # video.py:221-226
            if y is None:
                continue
            self._buffer("target", n, g)[sl] += y.mean(dim=0)
            if self.extended:
                self._buffer("target_sq", n, g)[sl] += (y ** 2).mean(dim=0)
                d = g - y                                                 # video.py:74-85
                self._buffer("mse", n, g)[sl] += torch.mean(torch.square(d), dim=0)
                lo, hi = self._buffer("min_err", n, g, math.inf, g.dtype), self._buffer("max_err", n, g, -math.inf, g.dtype)
                lo[sl] = torch.minimum(lo[sl], d.min(dim=0)[0])
                hi[sl] = torch.maximum(hi[sl], d.max(dim=0)[0])
        return 0

    # ---- the fused path -----------------------------------------------------------------------------------------------
    def _record_fused(self, w, names) -> int:
        """one ``ace_diag_video_window`` for all kept names and both sides; returns the launches made"""
        from .. import _lib
        if not names:
            return 0
        dev, HW, n_time = w.device, w.HW, self._agg._n_time
        buffers = {"_mean": lambda R: (2, R, n_time, HW)}
        if self.extended:
            buffers["_sq"] = lambda R: (3, R, n_time, HW)
        if _grow_rows(self, names, dev, **buffers) and self.extended:
            old, R = self._err, self._mean.shape[1]
            self._err = torch.empty((2, R, n_time, HW), dtype=torch.float32, device=dev)      # ``_grow`` zero-fills: not for these
            self._err[0] = math.inf
            self._err[1] = -math.inf
            if old is not None:
                self._err[:, :old.shape[1]] = old
        t0 = w.i_time_start
        assign = int(not self._n[t0:t0 + w.T].any())
        at, (p_rows,) = _upload_planes(names, w.gen, w.tgt, dev, [np.asarray([self._rows[n] for n in names], np.int32)])
        _check(_lib.lib().ace_diag_video_window(
            at["gen"], at["gen_strides"], at["target"], at["target_strides"], p_rows, self._mean.data_ptr(),
            self._sq.data_ptr() if self.extended else None, self._err.data_ptr() if self.extended else None, self._mean.shape[1],
            n_time, t0, assign, len(names), w.B, w.T, HW, _lib.current_stream()))
        return 1

    # ---- results ------------------------------------------------------------------------------------------------------
    def _channel(self, channel: str, name: str) -> torch.Tensor:
        """an accumulator of ``name`` as (n_time, H, W)"""
        if self._mean is None:
            return self._t[channel][name]
        buf, c = {"gen": (self._mean, 0), "target": (self._mean, 1), "gen_sq": (self._sq, 0), "target_sq": (self._sq, 1),
                  "mse": (self._sq, 2), "min_err": (self._err, 0), "max_err": (self._err, 1)}[channel]
        return buf[c, self._rows[name]].reshape(self._agg._n_time, *self._agg._shape)

    def _data(self) -> Dict[str, Any]:
        """video.py:363-441, ``_get_data``: log key -> (n_time, H, W) fp64, or for ``<name>`` the (prediction, target) pair; the
        reference's order - per name ``<name>`` then ``bias/<name>``, then all rmse, min_err, max_err, gen_var"""
        from ..distributed import Distributed
        dist, mean = Distributed.get_instance(), self._agg._reduce_mean
        out: Dict[str, Any] = {}
        if not self._pairs:
            return out
        names = sorted(self._pairs)
        dev = self._channel("gen", names[0]).device
        n = torch.from_numpy(self._n).to(dev)[:, None, None]
        over = lambda channel, name: mean(self._channel(channel, name) / n)      # noqa: E731  (0 / 0: an unvisited slot is NaN)
        for name in names:
            gen = over("gen", name)
            tgt = over("target", name) if self._pairs[name] else torch.full_like(gen, math.nan)
            out[name] = (gen, tgt)
            if self.extended and self._pairs[name]:
                out[f"bias/{name}"] = gen - tgt
        paired = [name for name in names if self.extended and self._pairs[name]]
        for name in paired:
            out[f"rmse/{name}"] = torch.sqrt(over("mse", name))
        for name in paired:
            out[f"min_err/{name}"] = -dist.reduce_max(-self._channel("min_err", name).double())
        for name in paired:
            out[f"max_err/{name}"] = dist.reduce_max(self._channel("max_err", name).double())
        for name in paired:
            gen_var = over("gen_sq", name) - over("gen", name) ** 2      # E[x^2] - E[x]^2, video.py:240-255
            out[f"gen_var/{name}"] = gen_var / (over("target_sq", name) - over("target", name) ** 2)
        return out

    def dataset(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """label -> variables (video.py:444-472), CPU fp64: ``<name>`` (2, n_time, H, W), the leading axis source = [prediction,
        target], and with ``enable_extended_videos`` ``bias_<name>``, ``rmse_<name>``, ``min_err_<name>``, ``max_err_<name>``,
        ``gen_var_<name>`` (n_time, H, W).  A time index no window visited is NaN, +inf in ``min_err`` and -inf in ``max_err``."""
        data = self._data()
        if not data:
            return {}
        return {self.cfg.name or "video": {k.strip("/").replace("/", "_"): (torch.stack(v) if isinstance(v, tuple) else v).cpu()
                                           for k, v in data.items()}}

    def logs(self) -> Dict[str, Dict[str, Any]]:
        """label -> logs (video.py:349-360) with the tensors of ``dataset()`` where the reference logs videos: ``<name>``,
        ``bias/<name>``, ``rmse/<name>``, ``min_err/<name>``, ``max_err/<name>``, ``gen_var/<name>``; ``video_frames`` turns one into
        the frames of the reference's video."""
        data = self._data()
        if not data:
            return {}
        return {self.cfg.name or "video": {k: (torch.stack(v) if isinstance(v, tuple) else v).cpu() for k, v in data.items()}}


def video_frames(gen, target=None):
    """``_make_video`` (video.py:486-519) up to the ``wandb.Video`` call: ``gen`` and ``target`` (n_time, H, W) arrays ->
    (frames, vmin, vmax) with frames (n_time, 3, H, W or 2 W + 10) fp64 brightness on a 0-255 scale - the prediction left of a
    10-column gap and the target; the colour scale from the target, or from the data when there is none (nanmin / nanmax);
    clamped to 0-255, NaN to 0; three repeated channels; latitude flipped."""
    as_np = lambda x: np.expand_dims(x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x), axis=1)      # noqa: E731
    if target is None:
        data = as_np(gen)
        vmin, vmax = np.nanmin(data), np.nanmax(data)
    else:
        gen, target = as_np(gen), as_np(target)
        gap = np.zeros([gen.shape[0], 1, gen.shape[2], 10])
        data = np.concatenate([gen, gap, target], axis=-1)
        vmin, vmax = np.nanmin(target), np.nanmax(target)                 # the target sets the colour scale
    data = 255 * (data - vmin) / (vmax - vmin)
    data = np.maximum(np.minimum(data, 255), 0)
    data[np.isnan(data)] = 0
    return np.flip(data.repeat(3, axis=1), axis=-2), vmin, vmax
