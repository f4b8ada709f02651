"""HEALPix variant (BASELINE configs[4]): the reference's HEALPixUNet behind the same registry / stepper
API - ``ModuleSelector(type="HEALPixUNet", config=...)`` (fme/ace/registry/hpx.py:14-111) - on the native operators of
``csrc/healpix.hip`` (include/ace_sfno.h: ace_hpx_*): neighbourhood convolutions on the 12-face mesh in place of the
spherical harmonic transform.

Host side mirrored here, name for name, so that reference configurations and checkpoints load (strict ``load_state_dict``;
seeded construction consumes the RNG in the reference's order): the configuration dataclasses and block classes of
fme/ace/models/healpix/{healpix_blocks.py, healpix_encoder.py, healpix_decoder.py, healpix_layers.py, healpix_activations.py,
healpix_unet.py} that the reference's own test configuration uses - ConvNeXtBlock, BasicConvBlock, AvgPool / MaxPool,
TransposedConvUpsample, CappedGELU, face padding modes "karlbauer" and "earth2grid" (which the reference documents as giving
the same result; one gather table serves both) and "isolatitude" (its own table, same gather kernel), and the
DealiasedDownsample / SmoothedInterpolateConv resamplers (composed from the same operators).  Not built (raise at
construction): interpolation modes other than "nearest" / "nearest-exact" / "bilinear" (bicubic, area).  The symmetric ConvNeXt
variants (residual added after the last activation) close with an identity contraction that carries the residual; the "Interpolate"
upsampling block is the transposed convolution with identity taps.

Runtime layout: an activation of one UNet level is ``[image = item * 12 + face][channel][row][pitch]`` fp32 with the row pitch
of that level's padded faces rounded up to a multiple of 4 (``Hpx``), so every k x k convolution is ONE contraction over
(tap, channel) on shifted views of the padded tensor (a row-offset table, no im2col copy) in the compensated-fp16 MFMA mode of
the SFNO path; every tensor carries a 64-word "bound slot" (max |x|, produced by the kernel that wrote the tensor) from which the
consuming convolution derives its power-of-two scale.  There is no CPU path: tensors must live on an MI355X."""
import ctypes
import dataclasses
import functools
import os
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib
from .registry import ModuleConfig, ModuleSelector

ACT_NONE, ACT_GELU = 0, 1
_INF = float("inf")


_check = functools.partial(_lib.check, family="hpx")


@dataclasses.dataclass
class Hpx:
    """An activation in the runtime layout: data [images, channels, rows, pitch] (contiguous, pitch % 4 == 0, gap columns
    [width, pitch) defined), valid columns [0, width); amax: its bound slot (64 int32 words) or None (not produced yet)."""
    data: torch.Tensor
    width: int
    amax: Optional[torch.Tensor] = None

    @property
    def pitch(self) -> int:
        return self.data.stride(-2) if self.data.shape[-2] > 1 else self.data.shape[-1]

    @property
    def rows(self) -> int:
        return self.data.shape[-2]


@dataclasses.dataclass
class HpxPlanes:
    """An activation that exists ONLY as the packed engine's operand: fp16 hi / lo planes (2, images * channels * rows * pitch halves),
    entries [image][channel / 8][rows x pitch cells][8 channels], scaled by the bound in `amax`.  Produced by a k x k convolution whose
    consumer is a 1 x 1 convolution (HEALPixLayer.conv_padded(out="planes") -> HEALPixLayer.conv_planes)."""
    planes: torch.Tensor
    images: int
    channels: int
    rows: int
    width: int
    pitch: int
    amax: torch.Tensor


@dataclasses.dataclass
class PaddedPlanes:
    """A face-PADDED activation as the packed engine's operand: fp16 hi / lo planes (2, images * cpad * m * pitch + slack halves),
    entries [image][channel / 8][m x pitch cells][8], m = width + 2 p, scaled by the bound in `amax`; `channels` of the `cpad`
    (a multiple of 8) are real.  Made by HEALPixLayer.pad_planes (a gather from fp32 tensors) or by a k x k convolution that
    writes its result into the interior and lets ace_hpx_halo_planes gather the halo."""
    planes: torch.Tensor
    images: int
    channels: int
    cpad: int
    rows: int        # unpadded rows (= width: faces are square)
    width: int
    p: int
    pitch: int
    amax: torch.Tensor
    mode: str

    @property
    def m(self) -> int:
        return self.width + 2 * self.p

    @property
    def cells(self) -> int:
        return self.m * self.pitch

    def origin(self, k: int, dil: int) -> int:
        """entry offset of the window origin of a (k, dil) convolution whose own padding is (k - 1) dil / 2 <= p"""
        q = self.p - (k - 1) * dil // 2
        return q * self.pitch + q


def _round4(n: int) -> int:
    return (n + 3) & ~3


def isolatitude_pad_table(nside: int, p: int) -> Tuple[np.ndarray, np.ndarray]:
    """Gather table of the ISOLATITUDE face padding (healpix_paddings.py:613-1140) in the format of ace_hpx_pad_table_host: for every
    cell of the padded mesh [12][nside + 2p][nside + 2p] two source cells packed face << 24 | row << 12 | column (equal where the
    cell is a plain copy); padded = 0.5 a + 0.5 b.  The rules, restated on index arrays:
      * polar faces take the strip across their polar edges from the rotated neighbour with a shift along the edge that grows
        with the distance from it - halo line i (0 = nearest) reads position max(j - (2i + 1), 0) (north: top / left strips) or
        min(j + (2i + 1), nside - 1) (south: bottom / right strips), so that cells of one latitude ring stay aligned;
      * equatorial faces take plain strips; their two neighbourless corners are filled diagonal by diagonal with the MEAN of one
        cell of each adjacent face (every corner cell has two sources);
      * the other corners and strips are the plain (for the far polar corner: twice rotated) neighbour blocks.
    Needs p <= nside / 2 (the reference's own bound)."""
    H = int(nside)
    if not (1 <= p and 2 * p <= H):
        raise ValueError(f"Padding {p} must not exceed half the face height/width {H}")
    rr, cc = np.meshgrid(np.arange(H), np.arange(H), indexing="ij")
    f = [((k << 24) | (rr << 12) | cc).astype(np.int64) for k in range(12)]
    ar = np.arange(H)

    def north(c, t, tl, lft, bl, b, br, rgt, tr):
        tt = np.rot90(t, 1)[-p:, :].copy()
        ll = np.rot90(lft, -1)[:, -p:].copy()
        for i in range(p):
            src = np.maximum(ar - (2 * i + 1), 0)
            tt[-i - 1, :] = tt[-i - 1, src]
            ll[:, -i - 1] = ll[src, -i - 1]
        centre = np.vstack((tt, c, b[:p, :]))
        left = np.vstack((np.rot90(tl, 2)[-p:, -p:], ll, bl[:p, -p:]))
        right = np.vstack((tr[-p:, :p], rgt[:, :p], br[:p, :p]))
        return np.hstack((left, centre, right))

    def south(c, t, tl, lft, bl, b, br, rgt, tr):
        bb = np.rot90(b, 1)[:p, :].copy()
        rg = np.rot90(rgt, -1)[:, :p].copy()
        for i in range(p):
            src = np.minimum(ar + (2 * i + 1), H - 1)
            bb[i, :] = bb[i, src]
            rg[:, i] = rg[src, i]
        centre = np.vstack((t[-p:, :], c, bb))
        left = np.vstack((tl[-p:, -p:], lft[:, -p:], bl[:p, -p:]))
        right = np.vstack((tr[-p:, :p], rg, np.rot90(br, 2)[:p, :p]))
        return np.hstack((left, centre, right))

    def corner(first, second, rot):       # p x p block, diagonal k = p - 1 - i holds sample i of each of the two faces
        a = np.zeros((p, p), np.int64)
        b = np.zeros((p, p), np.int64)
        for i in range(2 * p - 1):
            k = p - 1 - i
            rows = np.arange(max(-k, 0), min(p, p - k))
            a[rows, rows + k] = first(i)
            b[rows, rows + k] = second(i)
        return np.rot90(a, rot), np.rot90(b, rot)

    def equator(c, t, tl_ab, lft, bl, b, br_ab, rgt, tr):
        out = []
        for which in (0, 1):
            centre = np.vstack((t[-p:, :], c, b[:p, :]))
            left = np.vstack((tl_ab[which], lft[:, -p:], bl[:p, -p:]))
            right = np.vstack((tr[-p:, :p], rgt[:, :p], br_ab[which]))
            out.append(np.hstack((left, centre, right)))
        return out

    def tl(top, lft):
        return corner(lambda i: top[H - i - 2, 0], lambda i: lft[0, H - i - 2], -1)

    def br(bot, rgt):
        return corner(lambda i: bot[i + 1, H - 1], lambda i: rgt[H - 1, i + 1], 1)

    A, B = [None] * 12, [None] * 12
    for k, (t, tl_, lf, bl, b, br_, rg, tr) in enumerate([(1, 2, 3, 3, 4, 8, 5, 1), (2, 3, 0, 0, 5, 9, 6, 2), (3, 0, 1, 1, 6, 10, 7, 3),
                                                          (0, 1, 2, 2, 7, 11, 4, 0)]):
        A[k] = B[k] = north(f[k], f[t], f[tl_], f[lf], f[bl], f[b], f[br_], f[rg], f[tr])
    for k, (t, lf, bl, b, rg, tr, brn) in zip(range(4, 8), [(0, 3, 7, 11, 8, 5, 8), (1, 0, 4, 8, 9, 6, 9), (2, 1, 5, 9, 10, 7, 10),
                                                           (3, 2, 6, 10, 11, 4, 11)]):
        A[k], B[k] = equator(f[k], f[t], tl(f[t], f[lf]), f[lf], f[bl], f[b], br(f[b], f[rg]), f[rg], f[tr])
    for k, (t, tl_, lf, bl, b, br_, rg, tr) in zip(range(8, 12), [(5, 0, 4, 11, 11, 10, 9, 9), (6, 1, 5, 8, 8, 11, 10, 10),
                                                                  (7, 2, 6, 9, 9, 8, 11, 11), (4, 3, 7, 10, 10, 9, 8, 8)]):
        A[k] = B[k] = south(f[k], f[t], f[tl_], f[lf], f[bl], f[b], f[br_], f[rg], f[tr])
    ia = np.stack(A).reshape(-1).astype(np.int32)
    ib = np.stack(B).reshape(-1).astype(np.int32)
    return ia, ib


class _Runtime:
    """Per-forward context: row pitch per face width (a level's tensors share the pitch of that level's padded faces), the
    padding gather tables (device copies, cached per (nside, padding)) and the pool of bound slots (zeroed once per forward)."""

    SLOTS = 512

    def __init__(self):
        self.pitch: Dict[int, int] = {}
        self._tables: Dict[Tuple[int, int, str, str], Tuple[torch.Tensor, torch.Tensor]] = {}
        self._pool: Optional[torch.Tensor] = None
        self._next = 0

    def begin(self, device) -> None:
        self._pool = torch.zeros(self.SLOTS * 64, dtype=torch.int32, device=device)
        self._next = 0

    def slot(self, device) -> torch.Tensor:
        if self._pool is None or self._next >= self.SLOTS or self._pool.device != device:
            self.begin(device)
        v = self._pool[self._next * 64:(self._next + 1) * 64]
        self._next += 1
        return v

    def pitch_for(self, width: int) -> int:
        return self.pitch.get(width, _round4(width))

    def table(self, nside: int, p: int, device, mode: str = "karlbauer") -> Tuple[torch.Tensor, torch.Tensor]:
        key = (nside, p, str(device), mode)
        if key not in self._tables:
            if mode == "isolatitude":         # same table format, other neighbour rules (built on the host in Python)
                ia, ib = isolatitude_pad_table(nside, p)
            else:
                m = nside + 2 * p
                ia = np.zeros(12 * m * m, dtype=np.int32)
                ib = np.zeros_like(ia)
                _check(_lib.lib().ace_hpx_pad_table_host(nside, p, ia.ctypes.data, ib.ctypes.data))
            self._tables[key] = (torch.from_numpy(ia).to(device), torch.from_numpy(ib).to(device))
        return self._tables[key]


_RT = _Runtime()
_SLACK = 16   # ACE_HPX_SLACK_FLOATS
_PACKED_CONV = os.environ.get("ACE_HPX_NO_PACKED", "0") in ("", "0")   # k x k convolutions on the packed engine (ACE_HPX_NO_PACKED=1: gemm3, fp32 operand)


def _repitch(x: Hpx, pitch: int) -> Hpx:
    if x.pitch == pitch and x.data.is_contiguous():
        return x
    out = torch.zeros(*x.data.shape[:-1], pitch, dtype=torch.float32, device=x.data.device)
    out[..., : x.width] = x.data[..., : x.width]
    return Hpx(out, x.width, x.amax)


def _dense(x: Hpx) -> Hpx:
    """`x` as a contiguous [images][channels][rows][pitch % 4 == 0] tensor (a trimmed view of a larger tensor is copied; only
    the padding gather reads arbitrary strides)"""
    if x.data.is_contiguous() and x.pitch % 4 == 0:
        return x
    return _repitch(x, _round4(max(x.width, 1)) if not x.data.is_contiguous() else _round4(x.pitch))


def _bound(x: Hpx) -> torch.Tensor:
    """The tensor's bound slot; a tensor nothing native produced (the network input) gets one from a reduction pass."""
    if x.amax is None:
        x.amax = _RT.slot(x.data.device)
        d = x.data if x.data.is_contiguous() else x.data.contiguous()
        _check(_lib.lib().ace_hpx_absmax(d.data_ptr(), d.numel(), x.amax.data_ptr(), _lib.current_stream()))
    return x.amax


# ---------------------------------------------------------------------------------------------------------------------
# activations (healpix_activations.py)
@dataclasses.dataclass
class CappedGELUConfig:
    cap_value: int = 10

    def build(self) -> nn.Module:
        return CappedGELU(cap_value=self.cap_value)


class CappedGELU(nn.Module):
    """GELU clamped from above (healpix_activations.py:41-85); applied inside the producing convolution's epilogue."""

    def __init__(self, cap_value=1.0, **kwargs):
        super().__init__()
        self.add_module("gelu", torch.nn.GELU(**kwargs))
        self.register_buffer("cap", torch.tensor(cap_value, dtype=torch.float32))

    def code(self) -> Tuple[int, float]:
        # the buffer lives on the device: its value is read back once per change, not per call (a device -> host copy in every
        # forward costs a synchronisation, and is not allowed inside a graph capture)
        stamp = (self.cap.data_ptr(), self.cap._version)
        if getattr(self, "_cap_host", None) is None or self._cap_host[0] != stamp:
            self._cap_host = (stamp, float(self.cap.item()))
        return ACT_GELU, self._cap_host[1]


# ---------------------------------------------------------------------------------------------------------------------
# layers (healpix_layers.py:48-125, healpix_paddings.py)
class HEALPixPadding(nn.Module):
    """Face padding as a gather (no parameters; keeps the reference's ``layers.0`` slot): the Karlbauer / earth2grid rules
    (healpix_paddings.py:239-611) or, with ``nside`` given, the isolatitude rules (healpix_paddings.py:613-1140) - one gather
    kernel, two tables."""

    def __init__(self, padding: int, mode: str = "karlbauer", nside: Optional[int] = None):
        super().__init__()
        if not isinstance(padding, int) or padding < 1:
            raise ValueError(f"invalid value for 'padding', expected int > 0 but got {padding}")
        if mode == "isolatitude" and (not isinstance(nside, int) or nside < 1):
            raise ValueError(f"nside must be a positive int, got {nside!r}")
        self.p = padding
        self.mode = mode
        self._nside = nside


def make_hpx_padding_layer(padding: int, hpx_padding_mode: str, nside: Optional[int] = None) -> nn.Module:
    """healpix_paddings.py:79-130."""
    if hpx_padding_mode in ("earth2grid", "karlbauer"):
        return HEALPixPadding(padding)
    if hpx_padding_mode == "isolatitude":
        if nside is None:
            raise ValueError('hpx_padding_mode="isolatitude" requires nside (positive int, native face height/width)')
        return HEALPixPadding(padding, "isolatitude", int(nside))
    raise ValueError(f"Unknown hpx_padding_mode: {hpx_padding_mode!r}; expected one of 'earth2grid', 'karlbauer', 'isolatitude'.")


class HEALPixLayer(nn.Module):
    """healpix_layers.py:48-125: [padding,] base layer on folded faces.  The base layers are torch modules used as PARAMETER
    HOLDERS (their initialisation is the reference's); the arithmetic runs in csrc/healpix.hip."""

    def __init__(self, layer, hpx_padding_mode: str = "earth2grid", nside: Optional[int] = None, **kwargs):
        super().__init__()
        layers: List[nn.Module] = []
        if "nside" in kwargs:
            ns = kwargs.pop("nside")
            nside = int(ns) if ns is not None else None
        kernel_size = 3 if "kernel_size" not in kwargs else kwargs["kernel_size"]
        dilation = 1 if "dilation" not in kwargs else kwargs["dilation"]
        padding = ((kernel_size - 1) // 2) * dilation
        if padding > 0:
            if issubclass(layer, torch.nn.modules.conv._ConvNd):
                kwargs["padding"] = 0
            layers.append(make_hpx_padding_layer(padding=padding, hpx_padding_mode=hpx_padding_mode, nside=nside))
        layers.append(layer(**kwargs))
        self.layers = torch.nn.Sequential(*layers)
        self._pad = padding
        self._k, self._dil = kernel_size, dilation
        self._prep: Optional[Tuple[Tuple[int, int], int, Any]] = None       # (weight stamp, native prepared-weight handle, its destroyer)
        self._prep_pk: Optional[Tuple[Tuple[int, int, int], int, Any]] = None   # the same for the packed engine's (tap, padded channel) form
        self._rows: Dict[Tuple[int, int, int, str], torch.Tensor] = {}

    def __del__(self):
        try:
            for prep in (self._prep, self._prep_pk):
                if prep is not None:
                    prep[2](ctypes.c_void_p(prep[1]))
        except Exception:
            pass

    # -- native execution
    @property
    def base(self) -> nn.Module:
        return self.layers[-1]

    def _weight(self) -> ctypes.c_void_p:
        """The weight prepared for the compensated-fp16 engine (fp16 hi / lo planes), rows = output channels (x 4 taps for the
        transposed convolution), columns = (tap, input channel); re-made when the parameter changes."""
        w = self.base.weight
        stamp = (w.data_ptr(), w._version)
        if self._prep is None or self._prep[0] != stamp:
            if isinstance(self.base, nn.ConvTranspose2d):      # [cin][cout][dy][dx] -> [(dy, dx, cout)][cin]
                t = w.detach().permute(2, 3, 1, 0).reshape(4 * w.shape[1], w.shape[0]).contiguous().float()
            else:                                              # [cout][cin][ky][kx] -> [cout][(ky, kx, cin)]
                t = w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous().float()
            h = ctypes.c_void_p()
            _check(_lib.lib().ace_hpx_weight_create(t.data_ptr(), t.shape[0], t.shape[1], _lib.current_stream(), ctypes.byref(h)))
            if self._prep is not None:
                self._prep[2](ctypes.c_void_p(self._prep[1]))
            self._prep = (stamp, h.value, _lib.lib().ace_hpx_weight_destroy)      # freed by the library that made it
        return ctypes.c_void_p(self._prep[1])

    def _weight_packed(self, cpad: int) -> ctypes.c_void_p:
        """The k x k weight for the packed engine: columns = (tap, channel padded to `cpad`), zero columns for the padding."""
        w = self.base.weight
        stamp = (w.data_ptr(), w._version, cpad)
        if self._prep_pk is None or self._prep_pk[0] != stamp:
            cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
            t = torch.zeros(cout, k * k, cpad, dtype=torch.float32, device=w.device)
            t[:, :, :cin] = w.detach().permute(0, 2, 3, 1).reshape(cout, k * k, cin).float()
            t = t.reshape(cout, k * k * cpad).contiguous()
            h = ctypes.c_void_p()
            _check(_lib.lib().ace_hpx_weight_create(t.data_ptr(), t.shape[0], t.shape[1], _lib.current_stream(), ctypes.byref(h)))
            if self._prep_pk is not None:
                self._prep_pk[2](ctypes.c_void_p(self._prep_pk[1]))
            self._prep_pk = (stamp, h.value, _lib.lib().ace_hpx_weight_destroy)
        return ctypes.c_void_p(self._prep_pk[1])

    def _row_offsets(self, cin: int, rows_in: int, pitch: int, device) -> torch.Tensor:
        key = (cin, rows_in, pitch, str(device))
        if key not in self._rows:
            k, d = self._k, self._dil
            taps = torch.tensor([ky * d * pitch + kx * d for ky in range(k) for kx in range(k)], dtype=torch.int64)
            chan = torch.arange(cin, dtype=torch.int64) * (rows_in * pitch)
            self._rows[key] = (taps[:, None] + chan[None, :]).reshape(-1).contiguous().to(device)
        return self._rows[key]

    def _bias_max(self) -> float:
        b = self.base.bias
        if b is None:
            return 0.0
        stamp = (b.data_ptr(), b._version)
        if getattr(self, "_bmax", None) is None or self._bmax[0] != stamp:
            self._bmax = (stamp, float(b.detach().abs().max().item()))
        return self._bmax[1]

    def conv_planes(self, x: HpxPlanes, residual: Optional[Hpx] = None, act: Tuple[int, float] = (ACT_NONE, _INF)) -> Hpx:
        """this 1 x 1 convolution on an input that exists as planes (no cap on the activation: the engine's plain form has none)"""
        base = self.base
        if not isinstance(base, nn.Conv2d) or self._k != 1 or self._pad > 0 or act[1] != _INF:
            raise TypeError("conv_planes(): a 1 x 1 convolution without a capped activation")
        dev = x.planes.device
        cout = base.out_channels
        if residual is not None:
            residual = _repitch(residual, x.pitch)
        y = torch.empty(x.images, cout, x.rows, x.pitch, dtype=torch.float32, device=dev)
        ymax = _RT.slot(dev)
        _check(_lib.lib().ace_hpx_conv1_packed(x.planes[0].data_ptr(), x.planes[1].data_ptr(), x.channels, self._weight(),
                                               _lib.ptr(base.bias) if base.bias is not None else None,
                                               residual.data.data_ptr() if residual is not None else None, y.data_ptr(), x.images, cout, x.rows,
                                               x.width, x.pitch, act[0], x.amax.data_ptr(), ymax.data_ptr(), _lib.current_stream()))
        return Hpx(y, x.width, ymax)

    def pad_planes(self, x: Hpx, x2: Optional[Hpx] = None) -> PaddedPlanes:
        """face padding of x (and x2 behind it: the skip concatenation) for THIS k x k convolution, written as the packed engine's planes"""
        dev = x.data.device
        imgs, W = x.data.shape[0], x.width
        cin = x.data.shape[1]
        cin2 = x2.data.shape[1] if x2 is not None else 0
        p, m = self._pad, W + 2 * self._pad
        mp = max(_RT.pitch_for(W), _round4(m))
        pad_layer = self.layers[0]
        if pad_layer.mode == "isolatitude" and W != pad_layer._nside:
            raise ValueError(f"HEALPixPaddingIsolatitude expected face size H={pad_layer._nside} (from init), but input has H={W}. "
                             "Make sure that nside was set correctly in the model config.")
        ia, ib = _RT.table(W, p, dev, pad_layer.mode)
        cpad = (cin + cin2 + 7) // 8 * 8
        planes = torch.empty(2, imgs * cpad * m * mp + _SLACK * 8, dtype=torch.float16, device=dev)
        pmax = _RT.slot(dev)
        d, d2 = x.data, (x2.data if x2 is not None else None)
        _check(_lib.lib().ace_hpx_pad_planes(d.data_ptr(), d.stride(0), d.stride(1), x.pitch,
                                             d2.data_ptr() if d2 is not None else None, d2.stride(0) if d2 is not None else 0,
                                             d2.stride(1) if d2 is not None else 0, x2.pitch if x2 is not None else 0, cin, cin2,
                                             planes[0].data_ptr(), planes[1].data_ptr(), ia.data_ptr(), ib.data_ptr(), imgs // 12, W, p, mp,
                                             _bound(x).data_ptr(), _bound(x2).data_ptr() if x2 is not None else None, pmax.data_ptr(),
                                             _lib.current_stream()))
        return PaddedPlanes(planes, imgs, cin + cin2, cpad, x.rows, W, p, mp, pmax, pad_layer.mode)

    def packable(self) -> bool:
        """does the packed engine cover this convolution when it pads its own input?  Odd-reach kernels (k = 4 ...) and paddings other
        than reach / 2 keep the fp32-operand route (gemm3 with a row-offset table), which handles any k / padding."""
        reach = (self._k - 1) * self._dil
        return (_PACKED_CONV and isinstance(self.base, nn.Conv2d) and self._pad > 0 and reach % 2 == 0 and reach <= _SLACK
                and self._pad == reach // 2)

    def accepts(self, pp: PaddedPlanes) -> bool:
        """can this convolution read `pp` (padded for a convolution with at least its own reach, in its own padding mode)?"""
        if not (_PACKED_CONV and isinstance(self.base, nn.Conv2d) and self.base.in_channels == pp.channels):
            return False
        reach = (self._k - 1) * self._dil
        if reach % 2 or reach // 2 > pp.p or reach > _SLACK:
            return False
        return self._pad == 0 if self._k == 1 else (self._pad == reach // 2 and self.layers[0].mode == pp.mode)

    def conv_padded(self, pp: PaddedPlanes, act: Tuple[int, float] = (ACT_NONE, _INF), out: str = "fp32",
                    pad_for: Optional["HEALPixLayer"] = None):
        """this convolution on an already padded input.  out: "fp32" -> Hpx; "planes" -> HpxPlanes (operand of a 1 x 1 convolution);
        "padded" -> PaddedPlanes for the k x k convolution `pad_for` (result written into the interior, halo gathered in place)."""
        base = self.base
        L = _lib.lib()
        st = _lib.current_stream()
        dev = pp.planes.device
        imgs, H, W, mp, cout, bias = pp.images, pp.rows, pp.width, pp.pitch, base.out_channels, base.bias
        w = self._weight_packed(pp.cpad)
        bptr = _lib.ptr(bias) if bias is not None else None
        xo = pp.origin(self._k, self._dil) * 16                      # bytes: one entry = 8 halves
        xhi, xlo = pp.planes[0].data_ptr() + xo, pp.planes[1].data_ptr() + xo
        ymax = _RT.slot(dev)
        if out == "fp32":
            y = torch.empty(imgs, cout, H, mp, dtype=torch.float32, device=dev)
            _check(L.ace_hpx_conv_packed(xhi, xlo, pp.cpad, pp.cells, w, bptr, 0.0, y.data_ptr(), None, None, 0, imgs, cout, H, W, mp, self._k,
                                         self._dil, act[0], act[1], pp.amax.data_ptr(), ymax.data_ptr(), st))
            return Hpx(y, W, ymax)
        if cout % 8:
            raise ValueError("a packed-planes result needs out_channels % 8 == 0")
        if out == "planes":
            o = torch.empty(2, imgs * cout * H * mp, dtype=torch.float16, device=dev)
            _check(L.ace_hpx_conv_packed(xhi, xlo, pp.cpad, pp.cells, w, bptr, self._bias_max(), None, o[0].data_ptr(), o[1].data_ptr(), 0, imgs,
                                         cout, H, W, mp, self._k, self._dil, act[0], act[1], pp.amax.data_ptr(), ymax.data_ptr(), st))
            return HpxPlanes(o, imgs, cout, H, W, mp, ymax)
        # "padded": the next convolution's padded planes - same face size and pitch rule, its own padding width
        if pad_for.layers[0].mode == "isolatitude" and W != pad_for.layers[0]._nside:       # the check pad_planes() makes
            raise ValueError(f"HEALPixPaddingIsolatitude expected face size H={pad_for.layers[0]._nside} (from init), but input has H={W}. "
                             "Make sure that nside was set correctly in the model config.")
        q = pad_for._pad
        m2 = W + 2 * q
        mp2 = max(_RT.pitch_for(W), _round4(m2))
        if mp2 != mp:
            raise ValueError("padded hand-over needs the same row pitch on both sides")
        nxt = PaddedPlanes(torch.empty(2, imgs * cout * m2 * mp2 + _SLACK * 8, dtype=torch.float16, device=dev), imgs, cout, cout, H, W, q, mp2,
                           ymax, pad_for.layers[0].mode)
        yo = (q * mp2 + q) * 16
        _check(L.ace_hpx_conv_packed(xhi, xlo, pp.cpad, pp.cells, w, bptr, self._bias_max(), None, nxt.planes[0].data_ptr() + yo,
                                     nxt.planes[1].data_ptr() + yo, nxt.cells, imgs, cout, H, W, mp, self._k, self._dil, act[0], act[1],
                                     pp.amax.data_ptr(), ymax.data_ptr(), st))
        ia, ib = _RT.table(W, q, dev, nxt.mode)
        _check(L.ace_hpx_halo_planes(nxt.planes[0].data_ptr(), nxt.planes[1].data_ptr(), cout, ia.data_ptr(), ib.data_ptr(), imgs // 12, W, q, mp2, st))
        return nxt

    def conv(self, x: Hpx, x2: Optional[Hpx] = None, residual: Optional[Hpx] = None, act: Tuple[int, float] = (ACT_NONE, _INF),
             planes_out: bool = False):
        base = self.base
        if not isinstance(base, nn.Conv2d):
            raise TypeError("conv() on a non-convolution HEALPixLayer")
        L = _lib.lib()
        st = _lib.current_stream()
        dev = x.data.device
        imgs, H, W = x.data.shape[0], x.rows, x.width
        cin = x.data.shape[1]
        cin2 = x2.data.shape[1] if x2 is not None else 0
        cout = base.out_channels
        bias = base.bias
        if self._pad > 0:
            p, m = self._pad, W + 2 * self._pad
            mp = max(_RT.pitch_for(W), _round4(m))
            pad_layer = self.layers[0]
            if pad_layer.mode == "isolatitude" and W != pad_layer._nside:
                raise ValueError(f"HEALPixPaddingIsolatitude expected face size H={pad_layer._nside} (from init), but input has H={W}. "
                                 "Make sure that nside was set correctly in the model config.")
            ia, ib = _RT.table(W, p, dev, pad_layer.mode)
            ctot = cin + cin2
            if self.packable():
                return self.conv_padded(self.pad_planes(x, x2), act=act, out="planes" if planes_out else "fp32")
            ymax = _RT.slot(dev)
            flat = torch.empty(imgs * ctot * m * mp + _SLACK, dtype=torch.float32, device=dev)
            xmax = _RT.slot(dev)
            for src, c0 in ((x, 0), (x2, cin)):
                if src is None:
                    continue
                d = src.data
                _check(L.ace_hpx_pad(d.data_ptr(), d.stride(0), d.stride(1), src.pitch, flat.data_ptr(), ctot, c0, d.shape[1],
                                     ia.data_ptr(), ib.data_ptr(), imgs // 12, W, p, mp, xmax.data_ptr(), st))
            y = torch.empty(imgs, cout, H, mp, dtype=torch.float32, device=dev)
            rows = self._row_offsets(ctot, m, mp, dev)
            _check(L.ace_hpx_conv(flat.data_ptr(), None, ctot, 0, self._weight(), rows.data_ptr(), _lib.ptr(bias) if bias is not None else None, None,
                                  y.data_ptr(), imgs, cout, H, W, mp, self._k, self._dil, act[0], act[1], xmax.data_ptr(), None,
                                  ymax.data_ptr(), st))
            return Hpx(y, W, ymax)
        x = _dense(x)
        pitch = x.pitch
        if x2 is not None:
            x2 = _repitch(x2, pitch)
        if residual is not None:
            residual = _repitch(residual, pitch)
        ymax = _RT.slot(dev)
        y = torch.empty(imgs, cout, H, pitch, dtype=torch.float32, device=dev)
        _check(L.ace_hpx_conv(x.data.data_ptr(), x2.data.data_ptr() if x2 is not None else None, cin, cin2, self._weight(), None,
                              _lib.ptr(bias) if bias is not None else None, residual.data.data_ptr() if residual is not None else None,
                              y.data_ptr(), imgs, cout, H, W, pitch, 1, 1, act[0], act[1], _bound(x).data_ptr(),
                              _bound(x2).data_ptr() if x2 is not None else None, ymax.data_ptr(), st))
        return Hpx(y, W, ymax)

    def pool(self, x: Hpx) -> Hpx:
        base = self.base
        k = base.kernel_size if isinstance(base.kernel_size, int) else base.kernel_size[0]
        if k != 2:
            raise NotImplementedError("only 2 x 2 pooling (the reference's configurations) is built")
        x = _dense(x)
        imgs, C, H, W = x.data.shape[0], x.data.shape[1], x.rows, x.width
        po = _RT.pitch_for(W // 2)
        y = torch.zeros(imgs, C, H // 2, po, dtype=torch.float32, device=x.data.device)
        _check(_lib.lib().ace_hpx_pool2(x.data.data_ptr(), y.data_ptr(), imgs * C, H, W, x.pitch, H * x.pitch, po, (H // 2) * po,
                                        1 if isinstance(base, nn.MaxPool2d) else 0, _lib.current_stream()))
        return Hpx(y, W // 2, x.amax)      # |mean| and max of four values are bounded by the input's bound

    def tconv(self, x: Hpx, act: Tuple[int, float]) -> Hpx:
        base = self.base
        if not (isinstance(base, nn.ConvTranspose2d) and base.kernel_size == (2, 2) and base.stride == (2, 2)):
            raise NotImplementedError("only the 2 x 2 stride-2 transposed convolution (the reference's configurations) is built")
        x = _dense(x)
        imgs, cin, H, W = x.data.shape[0], x.data.shape[1], x.rows, x.width
        cout = base.out_channels
        po = _RT.pitch_for(2 * W)
        dev = x.data.device
        tmp = torch.empty(4 * imgs * cout * H * x.pitch, dtype=torch.float32, device=dev)
        y = torch.zeros(imgs, cout, 2 * H, po, dtype=torch.float32, device=dev)
        ymax = _RT.slot(dev)
        _check(_lib.lib().ace_hpx_tconv2(x.data.data_ptr(), self._weight(), _lib.ptr(base.bias) if base.bias is not None else None,
                                         tmp.data_ptr(), y.data_ptr(), imgs, cin, cout, H, W, x.pitch, po, 2 * H * po, act[0], act[1],
                                         _bound(x).data_ptr(), ymax.data_ptr(), _lib.current_stream()))
        return Hpx(y, 2 * W, ymax)


def _act_code(m: Optional[nn.Module]) -> Tuple[int, float]:
    if m is None:
        return ACT_NONE, _INF
    if isinstance(m, CappedGELU):
        return m.code()
    raise NotImplementedError(f"activation {type(m).__name__} is not built")


def _run_convblock(convblock: nn.Sequential, x, x2: Optional[Hpx] = None, residual: Optional[Hpx] = None) -> Hpx:
    """A Sequential of HEALPixLayer(conv) [+ activation] pairs: each activation is fused into its convolution; `residual` is
    added by the last convolution (k = 1).  On the packed engine the activations BETWEEN the convolutions never exist in fp32:
    a k x k convolution writes the next k x k one's padded planes (interior; the halo is gathered in place) or the planes a 1 x 1
    one reads.  x: Hpx, or the PaddedPlanes already made for the first convolution (shared with the block's skip convolution)."""
    mods = list(convblock)
    convs = [(i, m) for i, m in enumerate(mods) if isinstance(m, HEALPixLayer)]
    cur = x
    for n_, (i, layer) in enumerate(convs):
        nxt_act = mods[i + 1] if i + 1 < len(mods) and not isinstance(mods[i + 1], HEALPixLayer) else None
        act = _act_code(nxt_act)
        follower = convs[n_ + 1][1] if n_ + 1 < len(convs) else None
        last = follower is None
        if isinstance(cur, HpxPlanes):                         # 1 x 1 convolution on planes
            cur = layer.conv_planes(cur, residual=residual if last else None, act=act)
            continue
        if isinstance(cur, Hpx) and layer.packable():
            cur = layer.pad_planes(cur, x2)
            x2 = None
        if isinstance(cur, PaddedPlanes):
            if not layer.accepts(cur):
                raise TypeError("padded planes handed to a convolution that cannot read them")
            out = "fp32"
            if follower is not None and layer.base.out_channels % 8 == 0 and isinstance(follower.base, nn.Conv2d):
                fact = mods[convs[n_ + 1][0] + 1] if convs[n_ + 1][0] + 1 < len(mods) and not isinstance(mods[convs[n_ + 1][0] + 1], HEALPixLayer) else None
                if follower._k == 1 and follower._pad == 0 and _act_code(fact)[1] == _INF and follower.base.in_channels % 8 == 0:
                    out = "planes"
                elif (follower._k > 1 and follower.packable()
                      and max(_RT.pitch_for(cur.width), _round4(cur.width + 2 * follower._pad)) == cur.pitch):
                    out = "padded"
            if last and residual is not None:
                raise NotImplementedError("a residual on a k x k convolution")
            cur = layer.conv_padded(cur, act=act, out=out, pad_for=follower if out == "padded" else None)
            continue
        cur = layer.conv(cur, x2=x2, residual=residual if last else None, act=act)
        x2 = None
    return cur


# ---------------------------------------------------------------------------------------------------------------------
# blocks (healpix_blocks.py)
@dataclasses.dataclass(frozen=True)
class HEALPixLayerBuildContext:
    hpx_padding_mode: str = "earth2grid"
    nside: Optional[int] = None
    nside_after: Optional[int] = None


@dataclasses.dataclass(frozen=True)
class HEALPixBuildContext:
    hpx_padding_mode: str = "earth2grid"
    nside_levels: Optional[Tuple[int, ...]] = None

    def layer(self, level: int, *, nside_after: Optional[int] = None) -> HEALPixLayerBuildContext:
        nside = None if self.nside_levels is None else self.nside_levels[level]
        return HEALPixLayerBuildContext(hpx_padding_mode=self.hpx_padding_mode, nside=nside, nside_after=nside_after)


def _kw(ctx: HEALPixLayerBuildContext) -> dict:
    out: dict = {"hpx_padding_mode": ctx.hpx_padding_mode}
    if ctx.nside is not None:
        out["nside"] = ctx.nside
    return out


class MaxPool(nn.Module):
    def __init__(self, pooling: int = 2, hpx_padding_mode: str = "earth2grid", nside: Optional[int] = None):
        super().__init__()
        self.maxpool = HEALPixLayer(layer=nn.MaxPool2d, kernel_size=pooling, **_kw(HEALPixLayerBuildContext(hpx_padding_mode, nside)))

    def forward(self, x: Hpx) -> Hpx:
        return self.maxpool.pool(x)


class AvgPool(nn.Module):
    def __init__(self, pooling: int = 2, hpx_padding_mode: str = "earth2grid", nside: Optional[int] = None):
        super().__init__()
        self.avgpool = HEALPixLayer(layer=nn.AvgPool2d, kernel_size=pooling, **_kw(HEALPixLayerBuildContext(hpx_padding_mode, nside)))

    def forward(self, x: Hpx) -> Hpx:
        return self.avgpool.pool(x)


class TransposedConvUpsample(nn.Module):
    """healpix_blocks.py:636-697."""

    def __init__(self, in_channels: int = 3, out_channels: int = 1, upsampling: int = 2,
                 activation_factory: Optional[Callable[[], nn.Module]] = None, hpx_padding_mode: str = "earth2grid",
                 nside: Optional[int] = None):
        super().__init__()
        upsampler: List[nn.Module] = [HEALPixLayer(layer=nn.ConvTranspose2d, in_channels=in_channels, out_channels=out_channels,
                                                   kernel_size=upsampling, stride=upsampling, padding=0,
                                                   **_kw(HEALPixLayerBuildContext(hpx_padding_mode, nside)))]
        if activation_factory is not None:
            upsampler.append(activation_factory())
        self.upsampler = nn.Sequential(*upsampler)

    def forward(self, x: Hpx) -> Hpx:
        act = self.upsampler[1] if len(self.upsampler) > 1 else None
        return self.upsampler[0].tconv(x, _act_code(act))


class BasicConvBlock(nn.Module):
    """healpix_blocks.py:868-930."""

    def __init__(self, in_channels=3, out_channels=1, kernel_size=3, dilation=1, n_layers=1, latent_channels=None,
                 activation_factory: Optional[Callable[[], nn.Module]] = None, hpx_padding_mode="earth2grid", nside=None):
        super().__init__()
        if latent_channels is None:
            latent_channels = max(in_channels, out_channels)
        convblock: List[nn.Module] = []
        for n in range(n_layers):
            convblock.append(HEALPixLayer(layer=torch.nn.Conv2d, in_channels=in_channels if n == 0 else latent_channels,
                                          out_channels=out_channels if n == n_layers - 1 else latent_channels,
                                          kernel_size=kernel_size, dilation=dilation,
                                          **_kw(HEALPixLayerBuildContext(hpx_padding_mode, nside))))
            if activation_factory is not None:
                convblock.append(activation_factory())
        self.convblock = nn.Sequential(*convblock)

    def forward(self, x: Hpx, x2: Optional[Hpx] = None) -> Hpx:
        return _run_convblock(self.convblock, x, x2=x2)


class ConvNeXtBlock(nn.Module):
    """healpix_blocks.py:932-1043: skip(x) + [k x k conv, act, k x k conv, act, 1 x 1 conv](x)."""

    def __init__(self, in_channels: int = 3, latent_channels: int = 1, out_channels: int = 1, kernel_size: int = 3,
                 dilation: int = 1, upscale_factor: int = 4, activation_factory: Optional[Callable[[], nn.Module]] = None,
                 hpx_padding_mode: str = "earth2grid", nside: Optional[int] = None):
        super().__init__()
        kw = _kw(HEALPixLayerBuildContext(hpx_padding_mode, nside))
        if in_channels == out_channels:
            self.skip_module = None
        else:
            self.skip_module = HEALPixLayer(layer=torch.nn.Conv2d, in_channels=in_channels, out_channels=out_channels, kernel_size=1, **kw)
        lat = int(latent_channels * upscale_factor)
        convblock: List[nn.Module] = [HEALPixLayer(layer=torch.nn.Conv2d, in_channels=in_channels, out_channels=lat,
                                                   kernel_size=kernel_size, dilation=dilation, **kw)]
        if activation_factory is not None:
            convblock.append(activation_factory())
        convblock.append(HEALPixLayer(layer=torch.nn.Conv2d, in_channels=lat, out_channels=lat, kernel_size=kernel_size,
                                      dilation=dilation, **kw))
        if activation_factory is not None:
            convblock.append(activation_factory())
        convblock.append(HEALPixLayer(layer=torch.nn.Conv2d, in_channels=lat, out_channels=out_channels, kernel_size=1, **kw))
        self.convblock = nn.Sequential(*convblock)

    def forward(self, x: Hpx, x2: Optional[Hpx] = None) -> Hpx:
        # the convolutions' outputs carry the pitch of this level's padded faces; the skip branch is brought to it
        first = self.convblock[0]
        target = max(_RT.pitch_for(x.width), _round4(x.width + 2 * first._pad)) if first._pad > 0 else _round4(x.pitch)
        if self.skip_module is None:
            if x2 is not None:   # identity skip of a concatenated input (decoder level with 2 C_in == C_out): the residual IS the
                cat = torch.zeros(x.data.shape[0], x.data.shape[1] + x2.data.shape[1], x.rows, target, dtype=torch.float32,
                                  device=x.data.device)                       # concatenation, materialised once in the target pitch
                cat[:, : x.data.shape[1], :, : x.width] = x.data[..., : x.width]
                cat[:, x.data.shape[1]:, :, : x.width] = x2.data[..., : x.width]
                skip = Hpx(cat, x.width)
            else:
                skip = _repitch(x, target)
        else:
            packed_first = first.packable()
            if packed_first:
                # ONE padded, packed copy of the block input serves both branches: the k x k convolution reads it whole, the 1 x 1
                # skip convolution its interior (pitch of the padded faces = `target`)
                pp = first.pad_planes(x, x2)
                if self.skip_module.accepts(pp):
                    skip = self.skip_module.conv_padded(pp)
                    return _run_convblock(self.convblock, pp, residual=skip)
                skip = self.skip_module.conv(_repitch(x, target), x2=_repitch(x2, target) if x2 is not None else None)
                return _run_convblock(self.convblock, pp, residual=skip)
            skip = self.skip_module.conv(_repitch(x, target), x2=_repitch(x2, target) if x2 is not None else None)
        return _run_convblock(self.convblock, x, x2=x2, residual=skip)


_IDENTITY: Dict[Tuple[int, str], ctypes.c_void_p] = {}


def _add_after_activation(y: Hpx, skip: Hpx) -> Hpx:
    """y + skip, both in the runtime layout.  The convolution epilogues add a residual BEFORE the activation; a block whose
    residual comes after it (the symmetric ConvNeXt variants) closes with one more native contraction - the identity over the
    channels, residual = skip, no activation: exact in the compensated-fp16 mode up to its 22-bit operand split."""
    C = y.data.shape[1]
    dev = y.data.device
    key = (C, str(dev))
    if key not in _IDENTITY:
        h = ctypes.c_void_p()
        eye = torch.eye(C, dtype=torch.float32, device=dev)
        _check(_lib.lib().ace_hpx_weight_create(eye.data_ptr(), C, C, _lib.current_stream(), ctypes.byref(h)))
        _IDENTITY[key] = h
    y = _dense(y)
    skip = _repitch(skip, y.pitch)
    imgs, H, W = y.data.shape[0], y.rows, y.width
    out = torch.empty(imgs, C, H, y.pitch, dtype=torch.float32, device=dev)
    omax = _RT.slot(dev)
    _check(_lib.lib().ace_hpx_conv(y.data.data_ptr(), None, C, 0, _IDENTITY[key], None, None, skip.data.data_ptr(), out.data_ptr(), imgs, C, H, W,
                                   y.pitch, 1, 1, ACT_NONE, _INF, _bound(y).data_ptr(), None, omax.data_ptr(), _lib.current_stream()))
    return Hpx(out, W, omax)


_UPSAMPLE_MODES = {"nearest": 0, "nearest-exact": 0, "bilinear": 1}   # (at an integer factor "nearest-exact" picks the same cells as "nearest")


class NearestUpsample(nn.Module):
    """nn.Upsample(scale_factor=2, mode=...) on folded faces (healpix_blocks.py:229-253, the "Interpolate" upsampling block; also the
    resize inside SmoothedInterpolate): "nearest" - every cell becomes a 2 x 2 block of itself - or "bilinear" with torch's source
    index and align_corners, one elementwise launch (ace_hpx_upsample2); exact fp32 in both arithmetic modes.  The input's bound also
    bounds the result.  (Round 5 ran "nearest" as a transposed convolution with identity taps on the matrix engine.)"""

    def __init__(self, stride: int = 2, mode: str = "nearest", align_corners: bool = False):
        super().__init__()
        if stride != 2 or mode not in _UPSAMPLE_MODES:
            raise NotImplementedError(f"Interpolate upsampling: stride 2 with mode 'nearest' / 'nearest-exact' / 'bilinear' is built (got stride={stride}, "
                                      f"mode={mode!r})")
        if align_corners and _UPSAMPLE_MODES[mode] == 0:
            raise ValueError("align_corners option can only be set with the interpolating modes: linear | bilinear | bicubic | trilinear")   # torch's own
        self.mode, self.align_corners = mode, bool(align_corners)

    def forward(self, x: Hpx, slack: bool = False) -> Hpx:
        """slack: leave the readable slack of a k > 1 contraction's input behind the result (and give it the exact pitch % 4)"""
        C = x.data.shape[1]
        dev = x.data.device
        x = _dense(x)
        imgs, H, W = x.data.shape[0], x.rows, x.width
        po = _round4(2 * W) if slack else _RT.pitch_for(2 * W)
        flat = torch.zeros(imgs * C * 2 * H * po + (_SLACK if slack else 0), dtype=torch.float32, device=dev)
        y = flat[: imgs * C * 2 * H * po].view(imgs, C, 2 * H, po)
        _check(_lib.lib().ace_hpx_upsample2(x.data.data_ptr(), y.data_ptr(), imgs * C, H, W, x.pitch, H * x.pitch, po, 2 * H * po,
                                            _UPSAMPLE_MODES[self.mode], int(self.align_corners), _lib.current_stream()))
        return Hpx(y, 2 * W, _bound(x))


# ---------------------------------------------------------------------------------------------------------------------
# resamplers built from the same operators (healpix_blocks.py:499-634, 699-866)
def _diagonal_taps(taps: torch.Tensor, channels: int, device) -> torch.Tensor:
    """[channels][(ky, kx, channel)] weight of a DEPTHWISE k x k filter for the dense (tap, channel) contraction: the filter's tap
    on the diagonal of every tap block.  (channels x more multiplications than a depthwise kernel would do; these layers are a
    few percent of a UNet level's convolutions.)"""
    k2 = taps.numel()
    w = torch.zeros(channels, k2, channels, dtype=torch.float32, device=device)
    idx = torch.arange(channels, device=device)
    w[idx, :, idx] = taps.reshape(1, k2).to(device=device, dtype=torch.float32)
    return w.reshape(channels, k2 * channels).contiguous()


class _FixedFilter:
    """A prepared depthwise filter per (device, channels): handle cache for the parameter-free resampling filters."""

    def __init__(self):
        self._h: Dict[Tuple[str, int], Tuple[ctypes.c_void_p, Any]] = {}

    def get(self, taps: torch.Tensor, channels: int, device) -> ctypes.c_void_p:
        key = (str(device), channels)
        if key not in self._h or self._h[key][1] is not _lib.lib():
            h = ctypes.c_void_p()
            w = _diagonal_taps(taps, channels, device)
            _check(_lib.lib().ace_hpx_weight_create(w.data_ptr(), w.shape[0], w.shape[1], _lib.current_stream(), ctypes.byref(h)))
            self._h[key] = (h, _lib.lib())
        return self._h[key][0]


def _valid_depthwise(x_flat: torch.Tensor, imgs: int, C: int, rows_in: int, pitch: int, k: int, w: ctypes.c_void_p,
                     xmax: torch.Tensor, device) -> Hpx:
    """k x k 'valid' depthwise filter of a [imgs][C][rows_in][pitch] tensor (+ slack behind it): -> Hpx of (rows_in - k + 1)^2"""
    Ho = rows_in - k + 1
    taps = torch.tensor([ky * pitch + kx for ky in range(k) for kx in range(k)], dtype=torch.int64)
    rows = (taps[:, None] + (torch.arange(C, dtype=torch.int64) * (rows_in * pitch))[None, :]).reshape(-1).contiguous().to(device)
    y = torch.empty(imgs, C, Ho, pitch, dtype=torch.float32, device=device)
    ymax = _RT.slot(device)
    _check(_lib.lib().ace_hpx_conv(x_flat.data_ptr(), None, C, 0, w, rows.data_ptr(), None, None, y.data_ptr(), imgs, C, Ho, Ho, pitch, k, 1,
                                   ACT_NONE, _INF, xmax.data_ptr(), None, ymax.data_ptr(), _lib.current_stream()))
    return Hpx(y, Ho, ymax)


class DealiasBlurConv2d(nn.Module):
    """healpix_blocks.py:499-559: fixed separable blur f f^T / sum, depthwise, strided (parameter holder: the buffer ``weight`` keeps
    the reference's state-dict entry)."""

    def __init__(self, in_channels: int, stride: int = 1, resample_filter: Optional[Sequence[float]] = None, **kwargs):
        super().__init__()
        filt = tuple(float(v) for v in (resample_filter if resample_filter is not None else [1.0, 2.0, 1.0]))
        if len(filt) < 1:
            raise ValueError("resample_filter must be non-empty")
        if sum(filt) == 0:
            raise ValueError("resample_filter must not sum to zero")
        self.in_channels = in_channels
        self.stride = stride
        f = torch.as_tensor(filt, dtype=torch.float32)
        f2d = f[:, None] * f[None, :]
        f2d = f2d / f2d.sum()
        self.register_buffer("weight", f2d.unsqueeze(0).unsqueeze(0).expand(in_channels, 1, len(filt), len(filt)).clone())


_SUBSAMPLE: Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]] = {}


def _subsample2(y: Hpx, out_width: int) -> Hpx:
    """out[r][c] = y[2 r][2 c] for r, c < out_width, per face and channel - the padding GATHER with a table that points at every
    second cell (ace_hpx_pad places a (nside' + 2 p')^2 mesh; here nside' = out_width - 2, p' = 1)."""
    dev = y.data.device
    imgs, C = y.data.shape[0], y.data.shape[1]
    po = _RT.pitch_for(out_width)
    if out_width < 3:          # a mesh this small has no (nside' >= 1, p' >= 1) form: the handful of cells is copied by torch
        out = torch.zeros(imgs, C, out_width, po, dtype=torch.float32, device=dev)
        out[..., :out_width] = y.data[:, :, 0:2 * out_width:2, 0:2 * out_width:2]
        return Hpx(out, out_width)
    key = (out_width, str(dev))
    if key not in _SUBSAMPLE:
        r, c = np.meshgrid(np.arange(out_width), np.arange(out_width), indexing="ij")
        cell = ((2 * r) << 12) | (2 * c)
        t = np.stack([(f << 24) | cell for f in range(12)]).reshape(-1).astype(np.int32)
        _SUBSAMPLE[key] = (torch.from_numpy(t).to(dev), torch.from_numpy(t.copy()).to(dev))
    ia, ib = _SUBSAMPLE[key]
    d = y.data
    flat = torch.empty(imgs * C * out_width * po + _SLACK, dtype=torch.float32, device=dev)
    omax = _RT.slot(dev)
    _check(_lib.lib().ace_hpx_pad(d.data_ptr(), d.stride(0), d.stride(1), y.pitch, flat.data_ptr(), C, 0, C, ia.data_ptr(), ib.data_ptr(),
                                  imgs // 12, out_width - 2, 1, po, omax.data_ptr(), _lib.current_stream()))
    return Hpx(flat[: imgs * C * out_width * po].view(imgs, C, out_width, po), out_width, omax)


class DealiasedDownsample(nn.Module):
    """healpix_blocks.py:562-634: log2(stride) stages of [face padding, fixed depthwise blur with stride 2].  Native form of a stage:
    the padding gather, the blur as one (tap, channel) contraction with a diagonal weight at stride 1, every second cell taken by
    the gather kernel again (a table that points at cells (2 r, 2 c))."""

    def __init__(self, in_channels: int = 3, resample_filter: Optional[Sequence[float]] = None, stride: int = 2,
                 hpx_padding_mode: str = "earth2grid", nside: Optional[int] = None):
        super().__init__()
        filt = tuple(float(v) for v in (resample_filter if resample_filter is not None else [1.0, 2.0, 1.0]))
        if len(filt) < 1:
            raise ValueError("resample_filter must be non-empty")
        if sum(filt) == 0:
            raise ValueError("resample_filter must not sum to zero")
        if stride < 1 or (stride & (stride - 1)) != 0:
            raise ValueError("stride must be a positive power of 2")
        n_layers = stride.bit_length() - 1
        kw = _kw(HEALPixLayerBuildContext(hpx_padding_mode, nside))
        self.pool = nn.Sequential(*[
            HEALPixLayer(layer=DealiasBlurConv2d, in_channels=in_channels, out_channels=in_channels, kernel_size=len(filt), stride=2,
                         padding=0, groups=in_channels, bias=False, dilation=1, resample_filter=filt, **kw) for _ in range(n_layers)])
        self.downsample_factor = stride
        self._filters = _FixedFilter()

    def _stage(self, layer: HEALPixLayer, x: Hpx) -> Hpx:
        dev = x.data.device
        imgs, C, W = x.data.shape[0], x.data.shape[1], x.width
        k, p = layer._k, layer._pad
        w = self._filters.get(layer.base.weight[0, 0], C, dev)
        if p > 0:
            pad_layer = layer.layers[0]
            if pad_layer.mode == "isolatitude" and W != pad_layer._nside:
                raise ValueError(f"HEALPixPaddingIsolatitude expected face size H={pad_layer._nside} (from init), but input has H={W}. "
                                 "Make sure that nside was set correctly in the model config.")
            m = W + 2 * p
            mp = max(_RT.pitch_for(W), _round4(m))
            ia, ib = _RT.table(W, p, dev, pad_layer.mode)
            flat = torch.empty(imgs * C * m * mp + _SLACK, dtype=torch.float32, device=dev)
            xmax = _RT.slot(dev)
            d = x.data
            _check(_lib.lib().ace_hpx_pad(d.data_ptr(), d.stride(0), d.stride(1), x.pitch, flat.data_ptr(), C, 0, C, ia.data_ptr(),
                                          ib.data_ptr(), imgs // 12, W, p, mp, xmax.data_ptr(), _lib.current_stream()))
        else:
            xd = _dense(x)
            m, mp = W, xd.pitch
            flat = torch.zeros(imgs * C * m * mp + _SLACK, dtype=torch.float32, device=dev)
            flat[: imgs * C * m * mp] = xd.data.reshape(-1)
            xmax = _bound(xd)
        blurred = _valid_depthwise(flat, imgs, C, m, mp, k, w, xmax, dev)
        return _subsample2(blurred, (m - k) // 2 + 1)

    def forward(self, x: Hpx) -> Hpx:
        for layer in self.pool:
            x = self._stage(layer, x)
        return x


class SmoothedInterpolate(nn.Module):
    """healpix_blocks.py:699-759 (parameter holder: the buffer ``smoother_kernel`` keeps the reference's state-dict entry)."""

    def __init__(self, in_channels: int = 3, scale_factor: int = 2, mode: str = "nearest", trim_size: int = 0):
        super().__init__()
        if scale_factor != 2 or mode not in _UPSAMPLE_MODES:
            raise NotImplementedError(f"SmoothedInterpolate: scale_factor 2 with mode 'nearest' / 'nearest-exact' / 'bilinear' is built (got {scale_factor}, {mode!r})")
        self.in_channels, self.scale_factor, self.mode, self.trim_size = in_channels, scale_factor, mode, trim_size
        cross = torch.tensor([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
        self.register_buffer("smoother_kernel", cross.unsqueeze(0).unsqueeze(0).repeat((in_channels, 1, 1, 1)))


class SmoothedInterpolateConv(nn.Module):
    """healpix_blocks.py:762-866: [face padding (1 cell), nearest x 2, four-point smoother / 4, trim 1 cell], then a k x k convolution
    on padded faces of the doubled mesh [+ activation].  Native form: the padding gather; the x 2 replication of the PADDED faces as
    the transposed convolution with identity taps; the smoother as one 'valid' (tap, channel) contraction with a diagonal weight; the
    trim is a view (the next padding gather reads any strides); the convolution as everywhere."""

    def __init__(self, in_channels: int = 3, out_channels: int = 3, kernel_size: int = 3, dilation: int = 1, scale_factor: int = 2,
                 mode: str = "nearest", activation_factory: Optional[Callable[[], nn.Module]] = None,
                 hpx_padding_mode: str = "earth2grid", nside: Optional[int] = None, nside_after: Optional[int] = None):
        super().__init__()
        if dilation > 1:
            raise ValueError(f"dilation > 1 is not supported for HEALPix resize convolutions, got {dilation}")
        if nside is not None and nside_after is None:
            if hpx_padding_mode == "isolatitude":
                raise ValueError('SmoothedInterpolateConv requires nside_after when nside is set and hpx_padding_mode="isolatitude"')
            nside_after = nside
        if nside is not None and nside_after is not None and nside_after != nside * scale_factor:
            raise ValueError(f"nside_after ({nside_after}) must equal nside ({nside}) * scale_factor ({scale_factor})")
        block: List[nn.Module] = [
            HEALPixLayer(layer=SmoothedInterpolate, in_channels=in_channels, scale_factor=scale_factor, mode=mode, trim_size=1,
                         **_kw(HEALPixLayerBuildContext(hpx_padding_mode, nside))),
            HEALPixLayer(layer=nn.Conv2d, in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, dilation=dilation,
                         **_kw(HEALPixLayerBuildContext(hpx_padding_mode, nside_after)))]
        if activation_factory is not None:
            block.append(activation_factory())
        self.block = nn.Sequential(*block)
        self._filters = _FixedFilter()
        self._up = NearestUpsample(2, mode)

    def forward(self, x: Hpx) -> Hpx:
        dev = x.data.device
        layer = self.block[0]
        imgs, C, W = x.data.shape[0], x.data.shape[1], x.width
        pad_layer = layer.layers[0]
        if pad_layer.mode == "isolatitude" and W != pad_layer._nside:
            raise ValueError(f"HEALPixPaddingIsolatitude expected face size H={pad_layer._nside} (from init), but input has H={W}. "
                             "Make sure that nside was set correctly in the model config.")
        m = W + 2                                                    # faces padded by one cell
        mp = max(_RT.pitch_for(W), _round4(m))
        ia, ib = _RT.table(W, 1, dev, pad_layer.mode)
        flat = torch.empty(imgs * C * m * mp + _SLACK, dtype=torch.float32, device=dev)
        xmax = _RT.slot(dev)
        d = x.data
        _check(_lib.lib().ace_hpx_pad(d.data_ptr(), d.stride(0), d.stride(1), x.pitch, flat.data_ptr(), C, 0, C, ia.data_ptr(), ib.data_ptr(),
                                      imgs // 12, W, 1, mp, xmax.data_ptr(), _lib.current_stream()))
        padded = Hpx(flat[: imgs * C * m * mp].view(imgs, C, m, mp), m, xmax)
        up = self._up(padded, slack=True)                            # (2 W + 4)^2, every cell a 2 x 2 block of itself
        cross = layer.base.smoother_kernel[0, 0] / 4.0
        smooth = _valid_depthwise(up.data, imgs, C, up.rows, up.pitch, 3, self._filters.get(cross, C, dev), _bound(up), dev)   # (2 W + 2)^2
        t = layer.base.trim_size
        trimmed = Hpx(smooth.data[:, :, t:smooth.rows - t, t:smooth.width - t], smooth.width - 2 * t, smooth.amax)
        act = self.block[2] if len(self.block) > 2 else None
        return self.block[1].conv(trimmed, act=_act_code(act))


class SymmetricConvNeXtBlock(nn.Module):
    """healpix_blocks.py:1214-1335: skip(x) + [k x k conv, act, 1 x 1 conv (latent -> latent * upscale), act, 1 x 1 conv (back), act,
    k x k conv (-> out), act](x); the residual is added AFTER the last activation.  The skip is the identity when
    in_channels == latent_channels (the reference's condition), a 1 x 1 convolution in -> out otherwise."""

    def __init__(self, in_channels: int = 3, latent_channels: int = 1, out_channels: int = 1, kernel_size: int = 3,
                 dilation: int = 1, upscale_factor: int = 4, activation_factory: Optional[Callable[[], nn.Module]] = None,
                 hpx_padding_mode: str = "earth2grid", nside: Optional[int] = None):
        super().__init__()
        kw = _kw(HEALPixLayerBuildContext(hpx_padding_mode, nside))
        lat = int(latent_channels)
        if in_channels == lat:
            self.skip_module = None
        else:
            self.skip_module = HEALPixLayer(layer=torch.nn.Conv2d, in_channels=in_channels, out_channels=out_channels, kernel_size=1, **kw)
        convblock: List[nn.Module] = []
        for cin, cout, k in ((in_channels, lat, kernel_size), (lat, int(lat * upscale_factor), 1), (int(lat * upscale_factor), lat, 1),
                             (lat, out_channels, kernel_size)):
            convblock.append(HEALPixLayer(layer=torch.nn.Conv2d, in_channels=cin, out_channels=cout, kernel_size=k, dilation=dilation, **kw))
            if activation_factory is not None:
                convblock.append(activation_factory())
        self.convblock = nn.Sequential(*convblock)

    def forward(self, x: Hpx, x2: Optional[Hpx] = None) -> Hpx:
        if self.skip_module is None:
            if x2 is not None:      # identity skip of a concatenated input: the residual IS the concatenation
                cat = torch.zeros(x.data.shape[0], x.data.shape[1] + x2.data.shape[1], x.rows, x.pitch, dtype=torch.float32,
                                  device=x.data.device)
                cat[:, : x.data.shape[1], :, : x.width] = x.data[..., : x.width]
                cat[:, x.data.shape[1]:, :, : x.width] = x2.data[..., : x.width]
                skip = Hpx(cat, x.width)
            else:
                skip = x
        else:
            pitch = _round4(x.pitch)
            skip = self.skip_module.conv(_repitch(x, pitch), x2=_repitch(x2, pitch) if x2 is not None else None)
        return _add_after_activation(_run_convblock(self.convblock, x, x2=x2), skip)


class Multi_SymmetricConvNeXtBlock(nn.Module):
    """healpix_blocks.py:1337-1402: n_layers SymmetricConvNeXtBlocks in sequence (the first takes in_channels)."""

    def __init__(self, in_channels: int = 3, latent_channels: int = 1, out_channels: int = 1, kernel_size: int = 3,
                 dilation: int = 1, upscale_factor: int = 4, n_layers: int = 1,
                 activation_factory: Optional[Callable[[], nn.Module]] = None, hpx_padding_mode: str = "earth2grid",
                 nside: Optional[int] = None):
        super().__init__()
        self.blocks = nn.ModuleList([
            SymmetricConvNeXtBlock(in_channels=in_channels if i == 0 else out_channels, latent_channels=latent_channels,
                                   out_channels=out_channels, kernel_size=kernel_size, dilation=dilation, upscale_factor=upscale_factor,
                                   activation_factory=activation_factory, hpx_padding_mode=hpx_padding_mode, nside=nside)
            for i in range(n_layers)])

    def forward(self, x: Hpx, x2: Optional[Hpx] = None) -> Hpx:
        for i, block in enumerate(self.blocks):
            x = block(x, x2 if i == 0 else None)
        return x


def _not_built(name: str):
    def build(*a, **k):
        raise NotImplementedError(f"{name} is outside the accelerated path (ConvNeXtBlock, BasicConvBlock, AvgPool, MaxPool and "
                                  "TransposedConvUpsample are built)")
    return build


@dataclasses.dataclass
class MaxPoolDownsamplingBlockConfig:
    block_type: str = "MaxPool"
    pooling: int = 2

    def downsample_spatial_factor(self) -> int:
        return self.pooling

    def build(self, *, in_channels: Optional[int] = None, ctx: Optional[HEALPixLayerBuildContext] = None) -> nn.Module:
        c = ctx or HEALPixLayerBuildContext()
        return MaxPool(pooling=self.pooling, hpx_padding_mode=c.hpx_padding_mode, nside=c.nside)


@dataclasses.dataclass
class AvgPoolDownsamplingBlockConfig:
    block_type: str = "AvgPool"
    pooling: int = 2

    def downsample_spatial_factor(self) -> int:
        return self.pooling

    def build(self, *, in_channels: Optional[int] = None, ctx: Optional[HEALPixLayerBuildContext] = None) -> nn.Module:
        c = ctx or HEALPixLayerBuildContext()
        return AvgPool(pooling=self.pooling, hpx_padding_mode=c.hpx_padding_mode, nside=c.nside)


@dataclasses.dataclass
class DealiasedDownsampleBlockConfig:
    """healpix_blocks.py:129-160."""
    block_type: str = "DealiasedDownsample"
    pooling: int = 2
    resample_filter: Sequence[float] = dataclasses.field(default_factory=lambda: [1.0, 2.0, 1.0])

    def downsample_spatial_factor(self) -> int:
        return self.pooling

    def build(self, *, in_channels: Optional[int] = None, ctx: Optional[HEALPixLayerBuildContext] = None) -> nn.Module:
        if in_channels is None:
            raise ValueError("DealiasedDownsample requires in_channels to be passed to build()")
        c = ctx or HEALPixLayerBuildContext()
        return DealiasedDownsample(in_channels=in_channels, resample_filter=self.resample_filter, stride=self.pooling,
                                   hpx_padding_mode=c.hpx_padding_mode, nside=c.nside)


@dataclasses.dataclass
class SmoothedInterpolateConvBlockConfig:
    """healpix_blocks.py:195-226."""
    block_type: str = "SmoothedInterpolateConv"
    stride: int = 2
    kernel_size: int = 3
    dilation: int = 1
    upsample_mode: str = "nearest"
    activation: Optional[CappedGELUConfig] = None

    def build(self, in_channels: int, out_channels: int, *, ctx: Optional[HEALPixLayerBuildContext] = None) -> nn.Module:
        c = ctx or HEALPixLayerBuildContext()
        return SmoothedInterpolateConv(in_channels=in_channels, out_channels=out_channels, kernel_size=self.kernel_size,
                                       dilation=self.dilation, scale_factor=self.stride, mode=self.upsample_mode,
                                       activation_factory=self.activation.build if self.activation else None,
                                       hpx_padding_mode=c.hpx_padding_mode, nside=c.nside, nside_after=c.nside_after)


@dataclasses.dataclass
class TransposedConvUpsampleBlockConfig:
    block_type: str = "TransposedConvUpsample"
    stride: int = 2
    activation: Optional[CappedGELUConfig] = None

    def build(self, in_channels: int, out_channels: int, *, ctx: Optional[HEALPixLayerBuildContext] = None) -> nn.Module:
        c = ctx or HEALPixLayerBuildContext()
        return TransposedConvUpsample(in_channels=in_channels, out_channels=out_channels, upsampling=self.stride,
                                      activation_factory=self.activation.build if self.activation else None,
                                      hpx_padding_mode=c.hpx_padding_mode, nside=c.nside)


@dataclasses.dataclass
class BasicConvBlockConfig:
    block_type: str = "BasicConvBlock"
    kernel_size: int = 3
    n_layers: int = 1
    activation: Optional[CappedGELUConfig] = None

    def build(self, in_channels: int, out_channels: int, *, latent_channels: Optional[int] = None, dilation: int = 1,
              n_layers: Optional[int] = None, ctx: Optional[HEALPixLayerBuildContext] = None) -> nn.Module:
        c = ctx or HEALPixLayerBuildContext()
        return BasicConvBlock(in_channels=in_channels, out_channels=out_channels, kernel_size=self.kernel_size, dilation=dilation,
                              n_layers=self.n_layers if n_layers is None else n_layers, latent_channels=latent_channels,
                              activation_factory=self.activation.build if self.activation else None,
                              hpx_padding_mode=c.hpx_padding_mode, nside=c.nside)


@dataclasses.dataclass
class ConvNeXtBlockConfig:
    block_type: str = "ConvNeXtBlock"
    kernel_size: int = 3
    upscale_factor: int = 4
    activation: Optional[CappedGELUConfig] = None

    def build(self, in_channels: int, out_channels: int, *, latent_channels: Optional[int] = None, dilation: int = 1,
              n_layers: Optional[int] = None, ctx: Optional[HEALPixLayerBuildContext] = None) -> nn.Module:
        c = ctx or HEALPixLayerBuildContext()
        return ConvNeXtBlock(in_channels=in_channels, latent_channels=1 if latent_channels is None else latent_channels,
                             out_channels=out_channels, kernel_size=self.kernel_size, dilation=dilation,
                             upscale_factor=self.upscale_factor,
                             activation_factory=self.activation.build if self.activation else None,
                             hpx_padding_mode=c.hpx_padding_mode, nside=c.nside)


@dataclasses.dataclass
class InterpolateUpsampleBlockConfig:
    """healpix_blocks.py:229-253."""
    block_type: str = "Interpolate"
    stride: int = 2
    upsample_mode: str = "nearest"
    align_corners: bool = False

    def build(self, in_channels: int, out_channels: int, *, ctx: Optional[HEALPixLayerBuildContext] = None) -> nn.Module:
        return NearestUpsample(self.stride, self.upsample_mode, self.align_corners)


@dataclasses.dataclass
class SymmetricConvNeXtBlockConfig:
    """healpix_blocks.py:335-369."""
    block_type: str = "SymmetricConvNeXtBlock"
    kernel_size: int = 3
    upscale_factor: int = 4
    activation: Optional[CappedGELUConfig] = None

    def build(self, in_channels: int, out_channels: int, *, latent_channels: Optional[int] = None, dilation: int = 1,
              n_layers: Optional[int] = None, ctx: Optional[HEALPixLayerBuildContext] = None) -> nn.Module:
        c = ctx or HEALPixLayerBuildContext()
        return SymmetricConvNeXtBlock(in_channels=in_channels, latent_channels=1 if latent_channels is None else latent_channels,
                                      out_channels=out_channels, kernel_size=self.kernel_size, dilation=dilation,
                                      upscale_factor=self.upscale_factor,
                                      activation_factory=self.activation.build if self.activation else None,
                                      hpx_padding_mode=c.hpx_padding_mode, nside=c.nside)


@dataclasses.dataclass
class MultiSymmetricConvNeXtBlockConfig:
    """healpix_blocks.py:371-416."""
    block_type: str = "Multi_SymmetricConvNeXtBlock"
    kernel_size: int = 3
    n_layers: int = 1
    upscale_factor: int = 4
    activation: Optional[CappedGELUConfig] = None

    def build(self, in_channels: int, out_channels: int, *, latent_channels: Optional[int] = None, dilation: int = 1,
              n_layers: Optional[int] = None, ctx: Optional[HEALPixLayerBuildContext] = None) -> nn.Module:
        c = ctx or HEALPixLayerBuildContext()
        return Multi_SymmetricConvNeXtBlock(in_channels=in_channels, latent_channels=1 if latent_channels is None else latent_channels,
                                            out_channels=out_channels, kernel_size=self.kernel_size, dilation=dilation,
                                            upscale_factor=self.upscale_factor, n_layers=self.n_layers if n_layers is None else n_layers,
                                            activation_factory=self.activation.build if self.activation else None,
                                            hpx_padding_mode=c.hpx_padding_mode, nside=c.nside)


_BLOCK_CONFIGS = {"MaxPool": MaxPoolDownsamplingBlockConfig, "AvgPool": AvgPoolDownsamplingBlockConfig,
                  "TransposedConvUpsample": TransposedConvUpsampleBlockConfig, "BasicConvBlock": BasicConvBlockConfig,
                  "ConvNeXtBlock": ConvNeXtBlockConfig, "SymmetricConvNeXtBlock": SymmetricConvNeXtBlockConfig,
                  "Multi_SymmetricConvNeXtBlock": MultiSymmetricConvNeXtBlockConfig, "Interpolate": InterpolateUpsampleBlockConfig,
                  "DealiasedDownsample": DealiasedDownsampleBlockConfig, "SmoothedInterpolateConv": SmoothedInterpolateConvBlockConfig}
_KNOWN_UNBUILT: set = set()


def _block_from_state(state: Any, default: Optional[type] = None):
    """A block configuration from its serialised form (the reference's dacite Union dispatch on ``block_type``)."""
    if state is None or dataclasses.is_dataclass(state):
        return state
    state = dict(state)
    bt = state.get("block_type", None)
    if bt is None and default is not None:
        bt = default().block_type
    if bt in _KNOWN_UNBUILT:
        raise NotImplementedError(f"block_type '{bt}' is outside the accelerated path")
    if bt not in _BLOCK_CONFIGS:
        raise ValueError(f"unknown block_type {bt!r}")
    cls = _BLOCK_CONFIGS[bt]
    names = {f.name for f in dataclasses.fields(cls)}
    extra = set(state) - names
    if extra:
        raise ValueError(f'can not match {sorted(extra)} to any data class field of "{cls.__name__}"')
    if isinstance(state.get("activation"), Mapping):
        state["activation"] = CappedGELUConfig(**state["activation"])
    return cls(**state)


# ---------------------------------------------------------------------------------------------------------------------
# encoder / decoder (healpix_encoder.py, healpix_decoder.py)
@dataclasses.dataclass
class UNetEncoderConfig:
    conv_block: Any
    down_sampling_block: Any
    n_channels: List[int] = dataclasses.field(default_factory=lambda: [136, 68, 34])
    n_layers: List[int] = dataclasses.field(default_factory=lambda: [2, 2, 1])
    dilations: Optional[list] = None

    def __post_init__(self):
        self.conv_block = _block_from_state(self.conv_block)
        self.down_sampling_block = _block_from_state(self.down_sampling_block)

    def build(self, input_channels: int, *, ctx: HEALPixBuildContext) -> nn.Module:
        if ctx.nside_levels is not None and len(ctx.nside_levels) != len(self.n_channels):
            raise ValueError(f"nside length must match encoder levels; got {len(ctx.nside_levels)} vs {len(self.n_channels)}")
        dilations = self.dilations if self.dilations is not None else [1 for _ in self.n_channels]
        down_factor = self.down_sampling_block.downsample_spatial_factor()
        old = input_channels
        levels: List[nn.Sequential] = []
        for n, cur in enumerate(self.n_channels):
            modules: List[nn.Module] = []
            if n > 0:
                if ctx.nside_levels is not None and ctx.nside_levels[n - 1] != ctx.nside_levels[n] * down_factor:
                    raise ValueError(f"encoder nside[{n - 1}]={ctx.nside_levels[n - 1]} must equal nside[{n}] * downsample factor "
                                     f"({down_factor}), but nside[{n}]={ctx.nside_levels[n]}")
                modules.append(self.down_sampling_block.build(in_channels=old, ctx=ctx.layer(n - 1)))
            modules.append(self.conv_block.build(in_channels=old, out_channels=cur, latent_channels=cur, dilation=dilations[n],
                                                 n_layers=self.n_layers[n], ctx=ctx.layer(n)))
            old = cur
            levels.append(nn.Sequential(*modules))
        return UNetEncoder(encoder=levels)


class UNetEncoder(nn.Module):
    def __init__(self, encoder: List[nn.Sequential]):
        super().__init__()
        self.encoder = nn.ModuleList(encoder)

    def forward(self, x: Hpx) -> Sequence[Hpx]:
        outs = []
        for level in self.encoder:
            for mod in level:
                x = mod(x)
            outs.append(x)
        return outs


@dataclasses.dataclass
class UNetDecoderConfig:
    conv_block: Any
    up_sampling_block: Any
    output_layer: Any
    n_channels: List[int] = dataclasses.field(default_factory=lambda: [34, 68, 136])
    n_layers: List[int] = dataclasses.field(default_factory=lambda: [1, 2, 2])
    dilations: Optional[list] = None

    def __post_init__(self):
        self.conv_block = _block_from_state(self.conv_block)
        self.up_sampling_block = _block_from_state(self.up_sampling_block)
        self.output_layer = _block_from_state(self.output_layer)

    def build(self, output_channels: int, *, ctx: HEALPixBuildContext) -> nn.Module:
        if ctx.nside_levels is not None and len(ctx.nside_levels) != len(self.n_channels):
            raise ValueError(f"nside length must match decoder levels; got {len(ctx.nside_levels)} vs {len(self.n_channels)}")
        dilations = self.dilations if self.dilations is not None else [1 for _ in self.n_channels]
        nside_levels = ctx.nside_levels
        up_factor = self.up_sampling_block.stride
        nlev = len(self.n_channels)
        decoder: List[DecoderLevel] = []
        cur = self.n_channels[0]
        for n, cur in enumerate(self.n_channels):
            up = None
            level_nside = None if nside_levels is None else nside_levels[nlev - 1 - n]
            if n != 0:
                if nside_levels is not None and nside_levels[nlev - n] * up_factor != level_nside:
                    raise ValueError(f"decoder nside upsample: nside[{nlev - 1 - n}]={level_nside} must equal nside[{nlev - n}] * "
                                     f"upsample factor ({up_factor}), but nside[{nlev - n}]={nside_levels[nlev - n]}")
                up = self.up_sampling_block.build(in_channels=cur, out_channels=cur, ctx=ctx.layer(nlev - n, nside_after=level_nside))
            nxt = self.n_channels[n + 1] if n < nlev - 1 else self.n_channels[-1]
            conv = self.conv_block.build(in_channels=cur * 2 if n > 0 else cur, out_channels=nxt, latent_channels=cur,
                                         dilation=dilations[n], n_layers=self.n_layers[n], ctx=ctx.layer(nlev - 1 - n))
            decoder.append(DecoderLevel(upsamp=up, conv=conv))
        output_layer = self.output_layer.build(in_channels=cur, out_channels=output_channels, dilation=dilations[-1], ctx=ctx.layer(0))
        return UNetDecoder(decoder=decoder, output_layer=output_layer)


class DecoderLevel(nn.Module):
    """healpix_decoder.py: upsample, concatenate the encoder skip along the channels, convolve.  The concatenation is never
    materialised: the two sources are written into one padded tensor / read as two row sources of one GEMM."""

    def __init__(self, upsamp: Optional[nn.Module], conv: nn.Module):
        super().__init__()
        self.upsamp = upsamp
        self.conv = conv
        self.channel_dim = 1

    def forward(self, x: Hpx, skip: Hpx) -> Hpx:
        if self.upsamp is not None:
            return self.conv(self.upsamp(x), skip)
        return self.conv(x)


class UNetDecoder(nn.Module):
    def __init__(self, decoder: List[DecoderLevel], output_layer: nn.Module):
        super().__init__()
        self.decoder = nn.ModuleList(decoder)
        self.output_layer = output_layer

    def forward(self, inputs: Sequence[Hpx]) -> Hpx:
        x = inputs[-1]
        for n, level in enumerate(self.decoder):
            x = level(x, inputs[-1 - n])
        return self.output_layer(x)


# ---------------------------------------------------------------------------------------------------------------------
class HEALPixUNet(nn.Module):
    """healpix_unet.py:14-94: [B, 12, C, H, W] -> [B, 12, C_out, H, W]."""

    CHANNEL_DIM = 2

    def __init__(self, encoder: nn.Module, decoder: nn.Module, input_channels: int, output_channels: int,
                 nside: Optional[Tuple[int, ...]] = None):
        super().__init__()
        self.input_channels = input_channels
        self.output_channels = output_channels
        self.nside = nside
        self.encoder = encoder
        self.decoder = decoder

    def _level_pitches(self, width: int) -> Dict[int, int]:
        """row pitch per face width: the width of that level's padded faces (the largest padding any layer of the level uses)"""
        pads: Dict[int, int] = {}
        w = width
        for level in self.encoder.encoder:
            for mod in level:
                if isinstance(mod, (AvgPool, MaxPool)):
                    w //= 2
                elif isinstance(mod, DealiasedDownsample):
                    w //= mod.downsample_factor
            p = max([m._pad for m in level.modules() if isinstance(m, HEALPixLayer)] + [0])
            pads[w] = max(pads.get(w, 0), p)
        for n, level in enumerate(self.decoder.decoder):
            if level.upsamp is not None:
                w *= 2
            p = max([m._pad for m in level.conv.modules() if isinstance(m, HEALPixLayer)] + [0])
            pads[w] = max(pads.get(w, 0), p)
        return {wd: _round4(wd + 2 * p) for wd, p in pads.items()}

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        if inputs.ndim != 5:
            raise ValueError(f"HEALPixUNet expects a 5D input [B, F, C, H, W]; got tensor with shape {tuple(inputs.shape)}")
        if inputs.shape[self.CHANNEL_DIM] != self.input_channels:
            raise ValueError(f"Expected input to have {self.input_channels} channels at dim {self.CHANNEL_DIM}, got "
                             f"{inputs.shape[self.CHANNEL_DIM]}.")
        if inputs.shape[1] != 12:
            raise ValueError(f"expected 12 HEALPix faces at dim 1, got {inputs.shape[1]}")
        h, w = inputs.shape[-2], inputs.shape[-1]
        if self.nside is not None and (h != self.nside[0] or w != self.nside[0]):
            raise ValueError(f"Input face size ({h}, {w}) does not match nside[0]={self.nside[0]}")
        if h != w:
            raise ValueError("HEALPix faces are square")
        if not inputs.is_cuda:
            raise RuntimeError("HEALPixUNet (ace_amd) runs on an MI355X only: move the module and its input to 'cuda'. There is no "
                               "CPU fallback.")
        if torch.is_grad_enabled() and inputs.requires_grad:
            raise RuntimeError("ace_amd implements the inference forward only; call under torch.no_grad()")
        return self._run(inputs)

    def _run(self, inputs: torch.Tensor) -> torch.Tensor:
        """fold the faces into the batch, encoder, decoder, unfold (the checks are forward's)"""
        B = inputs.shape[0]
        h, w = inputs.shape[-2], inputs.shape[-1]
        _RT.pitch = self._level_pitches(w)
        _RT.begin(inputs.device)
        x = Hpx(inputs.reshape(B * 12, self.input_channels, h, w).float().contiguous(), w)   # fold (healpix_paddings.py:133-151)
        out = self.decoder(self.encoder(x))
        y = out.data[..., : out.width]
        return y.reshape(B, 12, self.output_channels, h, w).contiguous()                     # unfold


class CapturedHEALPixForward:
    """One forward of a HEALPix network captured in a hipGraph with static input / output buffers.

    At nside 64 the eager forward is ~150 launches of 5 - 40 us kernels driven from Python and is bound by the host; every
    native call of the forward is asynchronous on the current stream (weight handles and padding tables are built once, in the
    warm-up), so the whole forward captures, and a replay costs the device time only.  The result is the same kernels on the
    same data: bit-identical to the eager forward.  Inference only; the input shape is fixed at capture.
    """

    def __init__(self, net: nn.Module, example: torch.Tensor, warmup: int = 2):
        if not example.is_cuda:
            raise RuntimeError("CapturedHEALPixForward needs a device tensor (MI355X); there is no CPU path")
        self.net = net
        self.x = example.detach().clone()
        with torch.no_grad():
            side = torch.cuda.Stream(device=example.device)
            side.wait_stream(torch.cuda.current_stream(example.device))
            with torch.cuda.stream(side):
                for _ in range(max(warmup, 1)):
                    net(self.x)
            torch.cuda.current_stream(example.device).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with _lib.capture_without_gc(), torch.cuda.graph(self.graph):
                self.y = net(self.x)

    def __call__(self, inputs: torch.Tensor) -> torch.Tensor:
        if inputs.shape != self.x.shape:
            raise ValueError(f"captured for inputs of shape {tuple(self.x.shape)}, got {tuple(inputs.shape)}")
        self.x.copy_(inputs)
        self.graph.replay()
        return self.y


@ModuleSelector.register("HEALPixUNet")
@dataclasses.dataclass
class HEALPixUNetBuilder(ModuleConfig):
    """fme/ace/registry/hpx.py:14-111."""

    encoder: Any
    decoder: Any
    hpx_padding_mode: str = "earth2grid"
    nside: Optional[Sequence[int]] = None

    def __post_init__(self):
        if isinstance(self.encoder, Mapping):
            self.encoder = UNetEncoderConfig(**self.encoder)
        if isinstance(self.decoder, Mapping):
            self.decoder = UNetDecoderConfig(**self.decoder)
        if self.hpx_padding_mode not in ("earth2grid", "karlbauer", "isolatitude"):
            raise ValueError(f"Unknown hpx_padding_mode: {self.hpx_padding_mode!r}")

    def build(self, n_in_channels: int, n_out_channels: int, dataset_info) -> nn.Module:
        if len(getattr(dataset_info, "all_labels", ())) > 0:
            raise ValueError("HEALPixUNet does not support labels")
        return self._build(input_channels=n_in_channels, output_channels=n_out_channels)

    def _build(self, input_channels: int, output_channels: int) -> HEALPixUNet:
        levels = len(self.encoder.n_channels)
        if len(self.decoder.n_channels) != levels:
            raise ValueError(f"encoder and decoder must have same number of levels; got {levels} vs {len(self.decoder.n_channels)}")
        if self.hpx_padding_mode == "isolatitude" and self.nside is None:
            raise ValueError('hpx_padding_mode="isolatitude" requires nside (one int per UNet level)')
        nside_resolved: Optional[Tuple[int, ...]] = None
        if self.nside is not None:
            nside_resolved = tuple(int(v) for v in self.nside)
            if len(nside_resolved) != levels:
                raise ValueError(f"nside length must match UNet levels; got {len(nside_resolved)} vs {levels}")
            if any(v < 1 for v in nside_resolved):
                raise ValueError(f"nside values must be positive; got {nside_resolved}")
        ctx = HEALPixBuildContext(hpx_padding_mode=self.hpx_padding_mode, nside_levels=nside_resolved)
        encoder = self.encoder.build(input_channels=input_channels, ctx=ctx)
        decoder = self.decoder.build(output_channels=output_channels, ctx=ctx)
        return HEALPixUNet(encoder=encoder, decoder=decoder, input_channels=input_channels, output_channels=output_channels,
                           nside=nside_resolved)
