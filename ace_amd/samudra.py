"""Samudra (M2Lines ocean emulator, the ocean half of the CM4 piControl baseline): the reference's network
(fme/ace/models/ocean/m2lines/samudra.py, layers.py; builder fme/ace/registry/m2lines.py) behind the same registry / stepper API -
``ModuleSelector(type="Samudra", config=...)`` - on native operators: the packed compensated-fp16 implicit-GEMM convolution of
``csrc/healpix.hip`` (ace_hpx_conv_packed / ace_hpx_conv1_packed) and the lat-lon glue of ``csrc/latlon.hip`` (ace_ll_*).

Host side mirrored module for module, so that reference checkpoints load with strict ``load_state_dict``: ``layers`` holds the
ConvNeXt blocks (``skip_module`` 1 x 1 convolution when the width changes, ``convblock`` = [conv k x k, norm, CappedGELU, conv k x k,
norm, CappedGELU, conv 1 x 1]), the pooling and upsampling slots and the closing 3 x 3 convolution.  The torch modules are parameter
holders; the arithmetic of a block is

    P0 = pad(x)                        ace_ll_pad_planes (longitude circular / zero, latitude zero) -> P-format planes
    skip = 1 x 1 conv of P0's interior  (or x itself)
    y1 = conv k x k (P0)               fp32, then ace_ll_norm_stats -> per-(image, channel) scale / shift
    P1 = pad(CappedGELU(norm(y1)))     the affine and the activation fused into the padding pass
    y2 = conv k x k (P1);  Q = CappedGELU(norm(y2)) as planes (p = 0)
    out = skip + 1 x 1 conv (Q)        the residual added in the GEMM epilogue

with 2 x 2 average pooling (floor at odd sizes) on the way down and bilinear x 2 upsampling fused with the pad-to-skip-shape and
the skip addition on the way up.  There is no CPU path: tensors must live on an MI355X."""
import ctypes
import dataclasses
import functools
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib
from .healpix import CappedGELU
from .healpix import _check as _check_hpx
from .registry import ModuleConfig, ModuleSelector

ACT_NONE, ACT_GELU = 0, 1
_INF = float("inf")
_SLACK = 16          # ACE_HPX_SLACK_FLOATS: zero 16-byte entries behind every padded operand
_MAX_REACH = 16      # (k - 1) dil the packed engine reads past a row
_SLOTS = 512


_check = functools.partial(_lib.check, family="ll")


def _round4(n: int) -> int:
    return (n + 3) & ~3


def _round8(n: int) -> int:
    return (n + 7) & ~7


# ---------------------------------------------------------------------------------------------------------------------
# layers (layers.py): parameter holders with the reference's names
class AvgPool(nn.Module):
    def __init__(self, pooling: int = 2):
        super().__init__()
        if pooling != 2:
            raise NotImplementedError(f"AvgPool(pooling={pooling}): only 2 is built")
        self.avgpool = nn.AvgPool2d(pooling)


class BilinearUpsample(nn.Module):
    periodic = False

    def __init__(self, upsampling: int = 2, **kwargs):
        super().__init__()
        if upsampling != 2:
            raise NotImplementedError(f"upsampling={upsampling}: only 2 is built")
        self.upsampler = nn.Upsample(scale_factor=upsampling, mode="bilinear")


class ZonallyPeriodicBilinearUpsample(nn.Module):
    periodic = True

    def __init__(self, upsampling: int = 2, **kwargs):
        super().__init__()
        if upsampling != 2:
            raise NotImplementedError(f"upsampling={upsampling}: only 2 is built")
        self.upsampling = upsampling


def _make_norm(norm: Optional[str], channels: int, norm_kwargs: Mapping[str, Any]) -> Optional[nn.Module]:
    if norm is None:
        return None
    if norm == "instance":
        m = nn.InstanceNorm2d(channels, **norm_kwargs)
        if m.track_running_stats:
            raise NotImplementedError("Samudra norm='instance' with track_running_stats=True is not built (instance statistics only)")
        return m
    if norm == "batch":
        m = nn.BatchNorm2d(channels, **norm_kwargs)
        if not m.track_running_stats:
            raise NotImplementedError("Samudra norm='batch' with track_running_stats=False is not built (eval-mode running statistics only)")
        return m
    if norm == "layer":
        raise NotImplementedError("Samudra norm='layer' (per-pixel LayerNorm over channels) is not built")
    raise NotImplementedError(f"Normalization {norm} not implemented")


class ConvNeXtBlock(nn.Module):
    """layers.py ConvNeXtBlock: skip(x) + [pad, conv, norm, CappedGELU, pad, conv, norm, CappedGELU, conv 1 x 1](x)."""

    def __init__(self, in_channels: int = 300, out_channels: int = 1, kernel_size: int = 3, dilation: int = 1, n_layers: int = 1,
                 pad: str = "circular", norm: Optional[str] = "instance", norm_kwargs: Optional[Mapping[str, Any]] = None,
                 upscale_factor: int = 4, checkpoint_strategy: Optional[str] = None):
        super().__init__()
        assert kernel_size % 2 != 0, "Cannot use even kernel sizes!"
        assert n_layers == 1, "Can only use a single layer here!"
        if (kernel_size - 1) * dilation > _MAX_REACH:
            raise NotImplementedError(f"ConvNeXtBlock(kernel_size={kernel_size}, dilation={dilation}): (k - 1) dilation > {_MAX_REACH} is not built")
        self.N_in = in_channels
        self.N_pad = (kernel_size - 1) * dilation // 2
        self.k, self.dil = kernel_size, dilation
        self.pad = pad
        self.norm = norm
        self.norm_kwargs = dict(norm_kwargs or {})
        self.skip_module = nn.Conv2d(in_channels, out_channels, kernel_size=1) if in_channels != out_channels else None
        lat = int(in_channels * upscale_factor)
        convblock: List[nn.Module] = [nn.Conv2d(in_channels, lat, kernel_size=kernel_size, dilation=dilation)]
        n1 = _make_norm(norm, lat, self.norm_kwargs)
        if n1 is not None:
            convblock.append(n1)
        convblock.append(CappedGELU())
        convblock.append(nn.Conv2d(lat, lat, kernel_size=kernel_size, dilation=dilation))
        n2 = _make_norm(norm, lat, self.norm_kwargs)
        if n2 is not None:
            convblock.append(n2)
        convblock.append(CappedGELU())
        convblock.append(nn.Conv2d(lat, out_channels, kernel_size=1))
        self.convblock = nn.Sequential(*convblock)

    def stages(self) -> Tuple[nn.Conv2d, Optional[nn.Module], CappedGELU, nn.Conv2d, Optional[nn.Module], CappedGELU, nn.Conv2d]:
        m = list(self.convblock)
        if self.norm is None:
            return m[0], None, m[1], m[2], None, m[3], m[4]
        return m[0], m[1], m[2], m[3], m[4], m[5], m[6]


# ---------------------------------------------------------------------------------------------------------------------
# native execution
@dataclasses.dataclass
class _T:
    """an activation: data [imgs][channels][H][pitch] fp32 (gap columns defined), its bound slot"""
    data: torch.Tensor
    H: int
    W: int
    amax: torch.Tensor

    @property
    def pitch(self) -> int:
        return self.data.shape[-1]


class _Workspace:
    """Buffers and bound slots of one forward at one input shape: the same sequence of requests every forward, so buffer i is
    the same tensor each time (graph capture sees static addresses).  The slots are zeroed at the start of every forward."""

    def __init__(self, device):
        self.device = device
        self.bufs: List[torch.Tensor] = []
        self.i = 0
        self.slots = torch.zeros(_SLOTS * 64, dtype=torch.int32, device=device)
        self.nslot = 0

    def begin(self) -> None:
        self.i = 0
        self.nslot = 0
        self.slots.zero_()

    def get(self, shape: Sequence[int], dtype=torch.float32) -> torch.Tensor:
        if self.i < len(self.bufs):
            b = self.bufs[self.i]
            if tuple(b.shape) != tuple(shape) or b.dtype != dtype:
                raise RuntimeError("Samudra workspace: the sequence of buffers changed between forwards")
        else:
            b = torch.empty(*shape, dtype=dtype, device=self.device)
            self.bufs.append(b)
        self.i += 1
        return b

    def slot(self) -> torch.Tensor:
        if self.nslot >= _SLOTS:
            raise RuntimeError("Samudra workspace: out of bound slots")
        v = self.slots[self.nslot * 64:(self.nslot + 1) * 64]
        self.nslot += 1
        return v


class _Weights:
    """prepared weights (ace_hpx_weight handles) per convolution, re-made when the parameter changes"""

    def __init__(self):
        self.h: Dict[int, Tuple[Tuple[int, int, int], int]] = {}
        self._destroy = None

    def __del__(self):
        try:
            for _, (_, h) in self.h.items():
                self._destroy(ctypes.c_void_p(h))
        except Exception:
            pass

    def get(self, conv: nn.Conv2d, cpad: int) -> ctypes.c_void_p:
        w = conv.weight
        stamp = (w.data_ptr(), w._version, cpad)
        cur = self.h.get(id(conv))
        if cur is None or cur[0] != stamp:
            cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
            t = torch.zeros(cout, k * k, cpad, dtype=torch.float32, device=w.device)   # columns (tap, channel padded to cpad)
            t[:, :, :cin] = w.detach().permute(0, 2, 3, 1).reshape(cout, k * k, cin).float()
            t = t.reshape(cout, k * k * cpad).contiguous()
            h = ctypes.c_void_p()
            L = _lib.lib()
            _check_hpx(L.ace_hpx_weight_create(t.data_ptr(), t.shape[0], t.shape[1], _lib.current_stream(), ctypes.byref(h)))
            if cur is not None:
                L.ace_hpx_weight_destroy(ctypes.c_void_p(cur[1]))
            self._destroy = L.ace_hpx_weight_destroy
            self.h[id(conv)] = (stamp, h.value)
        return ctypes.c_void_p(self.h[id(conv)][1])


def _stamp(*ts: Optional[torch.Tensor]) -> tuple:
    return tuple((t.data_ptr(), t._version) if t is not None else None for t in ts)


@dataclasses.dataclass(frozen=True)
class LevelPlan:
    """sizes of every UNet level, the row pitch of its tensors and which blocks run there"""
    sizes: Tuple[Tuple[int, int], ...]          # (H, W) per level, level 0 = the input grid
    pitch: Tuple[int, ...]                      # row pitch per level (the widest padded row of the level, % 4 == 0)
    skip_pads: Tuple[Tuple[int, int], ...]      # (rows, columns) the upsampled tensor is padded by to reach the skip, per level < n


class Samudra(nn.Module):
    """samudra.py:18-204: [B, C_in, H, W] -> [B, C_out, H, W]."""

    def __init__(self, input_channels: int, output_channels: int, ch_width: Sequence[int] = (200, 250, 300, 400),
                 dilation: Sequence[int] = (1, 2, 4, 8), n_layers: Sequence[int] = (1, 1, 1, 1), pad: str = "circular",
                 norm: Optional[str] = "instance", norm_kwargs: Optional[Mapping[str, Any]] = None, upscale_factor: int = 4,
                 checkpoint_strategy: Optional[str] = None, zonally_periodic_upsample: bool = False):
        super().__init__()
        if pad in ("reflect", "replicate"):
            raise NotImplementedError(f"Samudra pad='{pad}' is not built (circular and constant are)")
        if pad not in ("circular", "constant"):
            raise NotImplementedError(f"Samudra pad='{pad}' is not built (circular and constant are)")
        if len(ch_width) < 1 or len(dilation) < len(ch_width) or len(n_layers) < len(ch_width):
            raise ValueError("Samudra needs one dilation and one n_layers entry per ch_width level")
        self.input_channels = input_channels
        self.output_channels = output_channels
        self.hist = 0
        self.ch_width = list(ch_width)
        self.dilation = list(dilation)
        self.n_layers = list(n_layers)
        self.pad = pad
        self.norm = norm
        self.norm_kwargs = norm_kwargs
        self.last_kernel_size = 3
        self.N_pad = 1
        self.upscale_factor = upscale_factor
        self.checkpoint_strategy = checkpoint_strategy      # training only: no effect on the forward
        self.zonally_periodic_upsample = zonally_periodic_upsample
        up_cls = ZonallyPeriodicBilinearUpsample if zonally_periodic_upsample else BilinearUpsample
        kw = dict(pad=pad, norm=norm, norm_kwargs=norm_kwargs, upscale_factor=upscale_factor, checkpoint_strategy=checkpoint_strategy)
        widths = (input_channels, *self.ch_width)
        n = len(self.ch_width)
        layers: List[nn.Module] = []
        for i in range(n):
            layers.append(ConvNeXtBlock(widths[i], widths[i + 1], dilation=self.dilation[i], n_layers=self.n_layers[i], **kw))
            layers.append(AvgPool())
        b, i = widths[n], n - 1
        layers.append(ConvNeXtBlock(b, b, dilation=self.dilation[i], n_layers=self.n_layers[i], **kw))
        layers.append(up_cls(in_channels=b, out_channels=b))
        rev, dil_rev, nl_rev = widths[::-1], self.dilation[::-1], self.n_layers[::-1]
        for i in range(n - 1):
            a, b = rev[i], rev[i + 1]
            layers.append(ConvNeXtBlock(a, b, dilation=dil_rev[i], n_layers=nl_rev[i], **kw))
            layers.append(up_cls(in_channels=b, out_channels=b))
        if n == 1:
            i = 0   # the reference's loop variable is left over from the way down
        layers.append(ConvNeXtBlock(b, b, dilation=dil_rev[i], n_layers=nl_rev[i], **kw))
        layers.append(nn.Conv2d(b, output_channels, self.last_kernel_size))
        self.layers = nn.ModuleList(layers)
        self.num_steps = n
        self._weights = _Weights()
        self._ws: Dict[Tuple, _Workspace] = {}
        self._aff: Dict[int, Tuple[tuple, torch.Tensor, float, float]] = {}

    # -- structure
    def blocks_by_level(self) -> List[Tuple[ConvNeXtBlock, int]]:
        """(block, level) in execution order"""
        n = self.num_steps
        out = [(self.layers[2 * i], i) for i in range(n)]
        out.append((self.layers[2 * n], n))
        out += [(self.layers[2 * n + 2 + 2 * j], n - 1 - j) for j in range(n - 1)]
        out.append((self.layers[4 * n], 0))
        return out

    def plan(self, H: int, W: int) -> LevelPlan:
        """level sizes (floor pooling), row pitches and skip pads; ValueError where the reference could not run: a level too small to
        pool, or a circular pad that would wrap more than once"""
        n = self.num_steps
        sizes = [(H, W)]
        for lvl in range(n):
            h, w = sizes[-1]
            if h < 2 or w < 2:
                raise ValueError(f"Samudra: level {lvl} is {h} x {w}, too small for 2 x 2 pooling")
            sizes.append((h // 2, w // 2))
        pads: Dict[int, int] = {0: self.N_pad}
        for blk, lvl in self.blocks_by_level():
            pads[lvl] = max(pads.get(lvl, 0), blk.N_pad)
        if self.pad == "circular":
            for lvl, p in pads.items():
                if p > sizes[lvl][1]:
                    raise ValueError(f"Samudra: a circular pad of {p} columns would wrap more than once around the {sizes[lvl][1]} "
                                     f"longitudes of level {lvl} (grid {H} x {W})")
        pitch = tuple(_round4(sizes[lvl][1] + 2 * pads.get(lvl, 0)) for lvl in range(n + 1))
        skip_pads = tuple((sizes[lvl][0] - 2 * sizes[lvl + 1][0], sizes[lvl][1] - 2 * sizes[lvl + 1][1]) for lvl in range(n))
        return LevelPlan(tuple(sizes), pitch, skip_pads)

    # -- forward
    def forward(self, fts: torch.Tensor) -> torch.Tensor:
        if self.training:
            raise NotImplementedError("Samudra (ace_amd) is built for inference: call .eval() (a module in training mode is not built)")
        if fts.ndim != 4:
            raise ValueError(f"Samudra expects a 4D input [B, C, H, W]; got shape {tuple(fts.shape)}")
        if fts.shape[1] != self.input_channels:
            raise ValueError(f"Samudra expected {self.input_channels} input channels, got {fts.shape[1]}")
        if not fts.is_cuda:
            raise RuntimeError("Samudra (ace_amd) runs on an MI355X only: move the module and its input to 'cuda'. There is no CPU fallback.")
        if torch.is_grad_enabled() and fts.requires_grad:
            raise RuntimeError("ace_amd implements the inference forward only; call under torch.no_grad()")
        B, _, H, W = fts.shape
        plan = self.plan(H, W)
        key = (B, H, W, str(fts.device), fts.dtype == torch.float32 and fts.is_contiguous())
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = _Workspace(fts.device)
        ws.begin()
        with torch.no_grad():
            return self._run(fts, plan, ws)

    def _run(self, fts: torch.Tensor, plan: LevelPlan, ws: _Workspace) -> torch.Tensor:
        L = _lib.lib()
        st = _lib.current_stream()
        B, _, H, W = fts.shape
        n = self.num_steps
        x = fts if fts.dtype == torch.float32 and fts.is_contiguous() else ws.get(fts.shape).copy_(fts)
        amax = ws.slot()
        _check_hpx(L.ace_hpx_absmax(x.data_ptr(), x.numel(), amax.data_ptr(), st))
        cur = _T(x, H, W, amax)
        skips: List[_T] = []
        blocks = self.blocks_by_level()
        for i in range(n):
            cur = self._block(blocks[i][0], cur, plan.pitch[i], ws)
            skips.append(cur)
            cur = self._pool(cur, plan.pitch[i + 1], ws)
        cur = self._block(blocks[n][0], cur, plan.pitch[n], ws)
        periodic = int(self.zonally_periodic_upsample)
        for j in range(n):
            lvl = n - 1 - j
            cur = self._upsample_add(cur, skips[lvl], periodic, ws)
            cur = self._block(blocks[n + 1 + j][0], cur, plan.pitch[lvl], ws)
        # the closing 3 x 3 convolution: one cell of circular / zero padding, no activation
        conv = self.layers[4 * n + 1]
        y = self._conv_kxk(self._pad(cur, self.N_pad, plan.pitch[0], ws), conv, 1, ws)
        return y.data[..., : cur.W].contiguous()

    def _pad(self, x: _T, p: int, pitch: int, ws: _Workspace, ss: Optional[torch.Tensor] = None, ss_img_stride: int = 0,
             act: Tuple[int, float] = (ACT_NONE, _INF), bound: Optional[Tuple[torch.Tensor, float, float]] = None) -> dict:
        imgs, c = x.data.shape[0], x.data.shape[1]
        cpad = _round8(c)
        rows = x.H + 2 * p
        planes = ws.get((2, imgs * cpad * rows * pitch + _SLACK * 8), torch.float16)
        pmax = ws.slot()
        bslot, bscale, boff = bound if bound is not None else (x.amax, 1.0, 0.0)
        d = x.data
        _check(_lib.lib().ace_ll_pad_planes(d.data_ptr(), d.stride(0), d.stride(1), d.stride(2), c, x.H, x.W, p, int(self.pad == "circular"),
                                            planes[0].data_ptr(), planes[1].data_ptr(), pitch, imgs,
                                            ss.data_ptr() if ss is not None else None, ss_img_stride, act[0], act[1], bslot.data_ptr(),
                                            bscale, boff, pmax.data_ptr(), _lib.current_stream()))
        return dict(planes=planes, imgs=imgs, cpad=cpad, H=x.H, W=x.W, p=p, pitch=pitch, amax=pmax)

    def _conv_kxk(self, pp: dict, conv: nn.Conv2d, dil: int, ws: _Workspace, k: Optional[int] = None) -> _T:
        """conv (k x k, or 1 x 1 reading the interior of planes padded for a wider one) on padded planes -> fp32"""
        k = conv.kernel_size[0] if k is None else k
        imgs, H, W, pitch, cout = pp["imgs"], pp["H"], pp["W"], pp["pitch"], conv.out_channels
        q = pp["p"] - (k - 1) * dil // 2                     # origin of the window inside the padded planes
        xo = (q * pitch + q) * 16
        y = ws.get((imgs, cout, H, pitch))
        ymax = ws.slot()
        planes = pp["planes"]
        _check_hpx(_lib.lib().ace_hpx_conv_packed(planes[0].data_ptr() + xo, planes[1].data_ptr() + xo, pp["cpad"], (H + 2 * pp["p"]) * pitch,
                                                  self._weights.get(conv, pp["cpad"]), _lib.ptr(conv.bias) if conv.bias is not None else None,
                                                  0.0, y.data_ptr(), None, None, 0, imgs, cout, H, W, pitch, k, dil, ACT_NONE, _INF,
                                                  pp["amax"].data_ptr(), ymax.data_ptr(), _lib.current_stream()))
        return _T(y, H, W, ymax)

    def _affine(self, norm: Optional[nn.Module], y: _T, ws: _Workspace):
        """-> (ss, ss_img_stride, (bound slot, bscale, boff)) of the norm's affine on y, or (None, 0, None)"""
        if norm is None:
            return None, 0, None
        if isinstance(norm, nn.InstanceNorm2d):
            imgs, c = y.data.shape[0], y.data.shape[1]
            ss = ws.get((imgs * c * 2,))
            slot = ws.slot()
            g = norm.weight if norm.affine else None
            b = norm.bias if norm.affine else None
            d = y.data
            _check(_lib.lib().ace_ll_norm_stats(d.data_ptr(), d.stride(0), d.stride(1), d.stride(2), imgs, c, y.H, y.W, float(norm.eps),
                                                _lib.ptr(g) if g is not None else None, _lib.ptr(b) if b is not None else None,
                                                ss.data_ptr(), None, slot.data_ptr(), _lib.current_stream()))
            return ss, c, (slot, 1.0, 0.0)
        # BatchNorm2d in eval: the running statistics folded into one affine per channel, once per parameter version
        stamp = _stamp(norm.weight, norm.bias, norm.running_mean, norm.running_var)
        cur = self._aff.get(id(norm))
        if cur is None or cur[0] != stamp:
            rv, rm = norm.running_var.double(), norm.running_mean.double()
            g = norm.weight.detach().double() if norm.weight is not None else torch.ones_like(rv)
            b = norm.bias.detach().double() if norm.bias is not None else torch.zeros_like(rv)
            sc = g / torch.sqrt(rv + norm.eps)
            sh = b - rm * sc
            ss = torch.stack([sc, sh], dim=1).float().contiguous()
            cur = (stamp, ss, float(sc.abs().max().item()) * (1 + 1e-6), float(sh.abs().max().item()) * (1 + 1e-6))
            self._aff[id(norm)] = cur
        return cur[1], 0, (y.amax, cur[2], cur[3])

    def _block(self, blk: ConvNeXtBlock, x: _T, pitch: int, ws: _Workspace) -> _T:
        c1, n1, a1, c2, n2, a2, c3 = blk.stages()
        d = blk.dil
        p0 = self._pad(x, blk.N_pad, pitch, ws)
        if blk.skip_module is not None:
            skip = self._conv_kxk(p0, blk.skip_module, 1, ws, k=1)
        elif x.pitch == pitch:
            skip = x
        else:                       # identity skip of the network input: brought to the level's pitch once
            s = ws.get((x.data.shape[0], x.data.shape[1], x.H, pitch))
            s.zero_()
            s[..., : x.W] = x.data[..., : x.W]
            skip = _T(s, x.H, x.W, x.amax)
        y1 = self._conv_kxk(p0, c1, d, ws)
        ss, sst, bound = self._affine(n1, y1, ws)
        p1 = self._pad(y1, blk.N_pad, pitch, ws, ss, sst, a1.code(), bound)
        y2 = self._conv_kxk(p1, c2, d, ws)
        ss, sst, bound = self._affine(n2, y2, ws)
        q = self._pad(y2, 0, pitch, ws, ss, sst, a2.code(), bound)
        imgs, cout = x.data.shape[0], c3.out_channels
        out = ws.get((imgs, cout, x.H, pitch))
        omax = ws.slot()
        planes = q["planes"]
        _check_hpx(_lib.lib().ace_hpx_conv1_packed(planes[0].data_ptr(), planes[1].data_ptr(), q["cpad"], self._weights.get(c3, q["cpad"]),
                                                   _lib.ptr(c3.bias) if c3.bias is not None else None, skip.data.data_ptr(), out.data_ptr(),
                                                   imgs, cout, x.H, x.W, pitch, ACT_NONE, q["amax"].data_ptr(), omax.data_ptr(),
                                                   _lib.current_stream()))
        return _T(out, x.H, x.W, omax)

    def _pool(self, x: _T, pitch: int, ws: _Workspace) -> _T:
        imgs, c = x.data.shape[0], x.data.shape[1]
        Ho, Wo = x.H // 2, x.W // 2
        y = ws.get((imgs, c, Ho, pitch))
        amax = ws.slot()
        _check(_lib.lib().ace_ll_pool2(x.data.data_ptr(), y.data_ptr(), imgs * c, x.H, x.W, x.pitch, x.H * x.pitch, pitch, Ho * pitch,
                                       amax.data_ptr(), _lib.current_stream()))
        return _T(y, Ho, Wo, amax)

    def _upsample_add(self, x: _T, skip: _T, periodic: int, ws: _Workspace) -> _T:
        imgs, c = x.data.shape[0], x.data.shape[1]
        if skip.data.shape[1] != c:
            raise ValueError(f"Samudra: upsampled {c} channels against a skip of {skip.data.shape[1]}")
        y = ws.get((imgs, c, skip.H, skip.pitch))
        amax = ws.slot()
        _check(_lib.lib().ace_ll_upsample2_add(x.data.data_ptr(), imgs * c, x.H, x.W, x.pitch, x.H * x.pitch, skip.data.data_ptr(), skip.pitch,
                                               skip.H * skip.pitch, y.data_ptr(), skip.H, skip.W, skip.pitch, skip.H * skip.pitch,
                                               int(self.pad == "circular"), periodic, amax.data_ptr(), _lib.current_stream()))
        return _T(y, skip.H, skip.W, amax)


class CapturedSamudraForward:
    """One Samudra forward captured in a hipGraph with static input / output buffers (the HEALPix helper's recipe).  Every native
    call of the forward is asynchronous on the current stream and the weights, caps and norm affines are prepared in the warm-up,
    so the whole forward captures; a replay runs the same kernels on the same data: bit-identical to the eager forward.
    Inference only; the input shape is fixed at capture."""

    def __init__(self, net: nn.Module, example: torch.Tensor, warmup: int = 2):
        if not example.is_cuda:
            raise RuntimeError("CapturedSamudraForward needs a device tensor (MI355X); there is no CPU path")
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


@ModuleSelector.register("Samudra")
@dataclasses.dataclass
class SamudraBuilder(ModuleConfig):
    """fme/ace/registry/m2lines.py:12-56."""

    ch_width: List[int] = dataclasses.field(default_factory=lambda: [200, 250, 300, 400])
    n_layers: List[int] = dataclasses.field(default_factory=lambda: [1, 1, 1, 1])
    dilation: List[int] = dataclasses.field(default_factory=lambda: [1, 2, 4, 8])
    pad: str = "circular"
    norm: str = "instance"
    norm_kwargs: Mapping[str, Any] = dataclasses.field(default_factory=dict)
    upscale_factor: int = 4
    checkpoint_strategy: Optional[str] = None
    zonally_periodic_upsample: bool = False

    def __post_init__(self):
        if "num_features" in self.norm_kwargs:
            raise ValueError("norm_kwargs should not have num_features")
        if "normalized_shape" in self.norm_kwargs:
            raise ValueError("norm_kwargs should not have normalized_shape")

    def build(self, n_in_channels: int, n_out_channels: int, dataset_info) -> nn.Module:
        if len(getattr(dataset_info, "all_labels", ())) > 0:
            raise ValueError("Samudra does not support labels")
        return Samudra(input_channels=n_in_channels, output_channels=n_out_channels, ch_width=self.ch_width, dilation=self.dilation,
                       n_layers=self.n_layers, pad=self.pad, norm=self.norm, norm_kwargs=self.norm_kwargs,
                       upscale_factor=self.upscale_factor, checkpoint_strategy=self.checkpoint_strategy,
                       zonally_periodic_upsample=self.zonally_periodic_upsample)
