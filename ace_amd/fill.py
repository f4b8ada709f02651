"""The smooth flood fill of masked fields ahead of the power spectrum (fme/core/fill.py: ``SmoothFloodFill(num_steps=4)``, the
reference's only instantiation, wired in fme/ace/aggregator/inference/spectrum.py:331): masked pixels are filled from the valid
ones - the plane mean deep inside a masked region, four rings of 3 x 3 neighbour averages at its rim - and the seam is smoothed by
blending with a 5-tap Gaussian blur, so that the SHT sees a finite field without a cliff at the coast.

The valid set is supplied, not read off the data: where the name's mask is non-zero, the rule ``InferenceAggregator.weights_for``
and ``omitted`` follow.  (The reference takes the NaN pattern of the first plane it sees; the two agree when the data is NaN
exactly where the mask is zero.)  Values at masked pixels never enter the result.

``fill_tables`` builds the two static tables of a mask on the host, ``smooth_flood_fill`` is the torch path (any device), the
fused path is ``ace_diag_fill_planes`` (csrc/fill.hip; the contract is in include/ace_sfno.h), and ``FillTables`` caches the tables
per mask key and device for both."""
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

STEPS = 4                 # expansion steps (ACE_DIAG_FILL_STEPS)
TAPS = 5                  # the Gaussian's taps, sigma 1
INTERIOR = STEPS + 1      # layer of a masked pixel the expansion does not reach


def gaussian_taps() -> np.ndarray:
    """the normalised fp64 taps exp(-q^2 / 2), q = -2..2"""
    q = np.arange(TAPS, dtype=np.float64) - TAPS // 2
    g = np.exp(-q * q / 2.0)
    return g / g.sum()


def _grow(known: np.ndarray) -> np.ndarray:
    """every pixel with a known pixel in its 3 x 3 neighbourhood: longitude circular, nothing beyond the poles"""
    rows = known | np.roll(known, 1, axis=1) | np.roll(known, -1, axis=1)
    out = rows.copy()
    out[1:] |= rows[:-1]
    out[:-1] |= rows[1:]
    return out


def _blur64(x: np.ndarray) -> np.ndarray:
    """the separable blur of an (H, W) fp64 plane: latitude with replicated rows, then longitude, circular"""
    g, h = gaussian_taps(), TAPS // 2
    H = x.shape[0]
    rows = np.clip(np.arange(H)[:, None] + np.arange(-h, h + 1)[None], 0, H - 1)           # (H, TAPS)
    v = sum(g[i] * x[rows[:, i]] for i in range(TAPS))
    return sum(g[i] * np.roll(v, h - i, axis=1) for i in range(TAPS))


def fill_layers(valid: np.ndarray, interior_first: bool = True) -> np.ndarray:
    """The uint8 layer plane of a boolean valid plane: 0 valid, k = 1..4 filled at expansion step k, 5 interior.  Two simulations:
    A grows the valid set for four steps and what it leaves out is the interior; B starts from valid and interior together, as the
    reference marks the interior valid before its expansion loop (fill.py:267-268), and the step at which B reaches a masked pixel
    is its layer - a pixel beside the interior is filled from the inside at step 1.  ``interior_first=False`` reads the layers off
    simulation A alone, which is wrong wherever an interior exists; kept so that a test can show the difference."""
    valid = np.asarray(valid, dtype=bool)
    known = valid.copy()
    first = np.where(valid, 0, INTERIOR).astype(np.uint8)          # simulation A: the step that reaches a pixel
    for k in range(1, STEPS + 1):
        grown = _grow(known)
        first[grown & ~known] = k
        known = grown
    interior = ~known
    if not interior_first or not interior.any():
        return first
    layers = np.where(valid, 0, INTERIOR).astype(np.uint8)
    known = valid | interior
    for k in range(1, STEPS + 1):
        grown = _grow(known)
        layers[grown & ~known] = k
        known = grown
    return layers


def fill_tables(valid) -> Tuple[torch.Tensor, torch.Tensor]:
    """(layers uint8 (H, W), blurred fp32 (H, W)) of a valid plane (a mask: non-zero is valid), on the CPU: the layer plane of
    ``fill_layers`` and the blur of the 0 / 1 valid plane, computed in fp64 and rounded once."""
    v = torch.as_tensor(valid).detach().cpu()
    if v.dim() != 2:
        raise ValueError(f"the valid plane must be (H, W), got {tuple(v.shape)}")
    if v.shape[1] < TAPS // 2:
        raise ValueError(f"the circular blur needs at least {TAPS // 2} longitudes, got {v.shape[1]}")
    v = (v != 0).numpy()
    return (torch.from_numpy(fill_layers(v)), torch.from_numpy(_blur64(v.astype(np.float64)).astype(np.float32)))


def _ring(x: torch.Tensor) -> torch.Tensor:
    """the 3 x 3 neighbourhood sums of (N, 1, H, W): longitude circular, zero rows beyond the poles"""
    x = F.pad(F.pad(x, (1, 1, 0, 0), mode="circular"), (0, 0, 1, 1))
    return F.conv2d(x, torch.ones(1, 1, 3, 3, dtype=x.dtype, device=x.device))


def _blur(x: torch.Tensor) -> torch.Tensor:
    g, h = torch.from_numpy(gaussian_taps()).to(x.device, x.dtype), TAPS // 2
    x = F.conv2d(F.pad(x, (0, 0, h, h), mode="replicate"), g.view(1, 1, TAPS, 1))
    return F.conv2d(F.pad(x, (h, h, 0, 0), mode="circular"), g.view(1, 1, 1, TAPS))


def smooth_flood_fill(tensor: torch.Tensor, valid, tables: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """``tensor`` (..., H, W) with its masked pixels filled: the reference's sequence of torch ops in the dtype of ``tensor`` on its
    device, with the valid set supplied (``valid``: an (H, W) mask, non-zero is valid; or ``tables`` = ``fill_tables(valid)``, from
    a ``FillTables`` cache).  A plane without a valid pixel comes out all NaN."""
    layers, bv = fill_tables(valid) if tables is None else tables
    H, W = tensor.shape[-2:]
    if tuple(layers.shape) != (H, W):
        raise ValueError(f"fields of shape {(H, W)} with fill tables of {tuple(layers.shape)}")
    layers = layers.to(tensor.device)
    bv = bv.to(tensor.device, tensor.dtype)
    x = tensor.reshape(-1, 1, H, W)
    ok = layers == 0
    x = torch.where(ok, x, torch.zeros((), dtype=x.dtype, device=x.device))
    mean = x.sum(dim=(-2, -1), keepdim=True) / ok.sum()
    x = torch.where(layers == INTERIOR, mean, x)
    for k in range(1, STEPS + 1):
        known = ((layers < k) | (layers == INTERIOR)).to(x.dtype)[None, None]
        # the pixels not known yet still hold 0, so the plain neighbourhood sum is the sum over the known ones
        x = torch.where(layers == k, _ring(x) / _ring(known), x)
    x = x * bv + _blur(x) * (1.0 - bv)
    return x.reshape(tensor.shape)


class FillTables:
    """The fill tables of an aggregator's masks, built once per mask key on the host and uploaded once per (mask key, device).  The
    torch path takes a key's pair (``on``); the fused path takes the row of a key (``row``) in the per-device stacks (``stacks``)
    that ``ace_diag_fill_planes`` reads.  ``uploads`` counts host-to-device copies of a table pair."""

    def __init__(self):
        self._host: Dict[Any, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._dev: Dict[Tuple[Any, str], Tuple[torch.Tensor, torch.Tensor]] = {}
        self._rows: Dict[str, List[Any]] = {}
        self._stacks: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        self.uploads = 0

    def host(self, key, mask) -> Tuple[torch.Tensor, torch.Tensor]:
        t = self._host.get(key)
        if t is None:
            t = self._host[key] = fill_tables(mask)
        return t

    def has_valid(self, key, mask) -> bool:
        return bool((self.host(key, mask)[0] == 0).any())

    def on(self, key, mask, device) -> Tuple[torch.Tensor, torch.Tensor]:
        t = self._dev.get((key, str(device)))
        if t is None:
            layers, blurred = self.host(key, mask)
            t = self._dev[(key, str(device))] = (layers.to(device), blurred.to(device))
            self.uploads += 1
        return t

    def row(self, key, mask, device) -> int:
        rows = self._rows.setdefault(str(device), [])
        if key not in rows:
            layers, blurred = (t.reshape(1, -1) for t in self.on(key, mask, device))
            old = self._stacks.get(str(device))
            self._stacks[str(device)] = (layers.clone(), blurred.clone()) if old is None else \
                (torch.cat([old[0], layers]), torch.cat([old[1], blurred]))
            rows.append(key)
        return rows.index(key)

    def stacks(self, device) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], int]:
        """(layers uint8 (nmasks, H * W), blurred fp32 (nmasks, H * W), nmasks) on ``device``; (None, None, 0) before any row"""
        s = self._stacks.get(str(device))
        return (None, None, 0) if s is None else (s[0], s[1], s[0].shape[0])
