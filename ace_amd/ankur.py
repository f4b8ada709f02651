"""AnkurLocalNet (registry type "AnkurLocalNet": fme/ace/registry/local_net.py:47-100, fme/core/models/conditional_sfno/ankur.py) -
three hidden layers of one width and a last 1 x 1 convolution without bias; the first layer is a grouped DISCO convolution on the
sphere (groups = gcd(in, embed_dim), morlet basis, no bias) or, with ``use_disco_encoder=False``, a 1 x 1 convolution; an optional
learned (1, embed_dim, H, W) positional embedding is added BEFORE the first activation; the activation is ReLU, GELU or SiLU.

The forward is ``ace_disco_forward`` (csrc/disco.hip: contraction with the psi table, grouped mix, embedding, activation - one
launch) into a hidden buffer and one ``ace_pixel_mlp_forward`` (csrc/pixel_mlp.hip) over layers 1 to 3; without the DISCO encoder
one ``ace_pixel_mlp_forward`` over all four layers (``ace_pixel_mlp_create2``: the embedding in front of the activation).

The module holds the reference's parameters under the reference's state-dict keys - those of its ``_ContextWrappedModule``:
"module.mlp.0.conv.weight" (out, in / groups, K) or "module.mlp.0.weight" / ".bias", "module.mlp.1.pos_embed", then
"module.mlp.N.weight" / ".bias" with N shifted by the embedding - in the reference's construction order; the psi table is not a
parameter and not in the state dict.  ``forward(x, labels=None)`` ignores the labels, as the reference does.  No CPU path."""
import ctypes
import dataclasses
import math
from typing import Optional, Tuple

import torch
from torch import nn

from . import _lib
from . import disco as _disco
from .landnet import MAX_WIDTH
from .landnet import _check as _check_mlp
from .registry import ModuleConfig, ModuleSelector
from .sfno import trunc_normal_

ACTIVATIONS = {"relu": (nn.ReLU, _disco.ACT_RELU), "gelu": (nn.GELU, _disco.ACT_GELU), "silu": (nn.SiLU, _disco.ACT_SILU)}


def check_limits(in_chans: int, embed_dim: int, out_chans: int, use_disco_encoder: bool, disco_kernel_size: int) -> None:
    """What the kernels' exported limits refuse, by name."""
    widest = max(in_chans, embed_dim, out_chans)
    if widest > MAX_WIDTH:
        raise NotImplementedError(f"AnkurLocalNet: a width of {widest} channels exceeds ACE_PIXEL_MLP_MAX_WIDTH = {MAX_WIDTH}")
    if use_disco_encoder:
        _disco.check_limits(in_chans, embed_dim, disco_kernel_size, who="AnkurLocalNet")


class _DiscoWeight(nn.Module):
    """The parameter holder of DiscreteContinuousConvS2 (_convolution.py:231-235): weight (out, in / groups, K), no bias."""

    def __init__(self, in_chans: int, out_chans: int, kernel_size: int):
        super().__init__()
        self.groups = math.gcd(in_chans, out_chans)
        self.groupsize = in_chans // self.groups
        K = kernel_size * kernel_size
        scale = math.sqrt(1.0 / self.groupsize / K)
        self.weight = nn.Parameter(scale * torch.randn(out_chans, self.groupsize, K))


class _GroupedDisco(nn.Module):
    """ankur.py:43-72: key "conv.weight"."""

    def __init__(self, in_chans: int, out_chans: int, kernel_size: int):
        super().__init__()
        self.conv = _DiscoWeight(in_chans, out_chans, kernel_size)


class _AddPosEmbed(nn.Module):
    """ankur.py:75-84: key "pos_embed", truncated normal of std 0.02."""

    def __init__(self, embed_dim: int, img_shape):
        super().__init__()
        self.pos_embed = nn.Parameter(torch.zeros(1, embed_dim, img_shape[0], img_shape[1]))
        trunc_normal_(self.pos_embed, std=0.02)


class AnkurLocalNetModel(nn.Module):
    """The net proper (keys "mlp.N..."); ``AnkurLocalNet`` wraps it under "module."."""

    def __init__(self, img_shape, in_chans: int, out_chans: int, embed_dim: int = 256, use_disco_encoder: bool = True,
                 disco_kernel_size: int = 3, pos_embed: bool = False, activation_function: str = "gelu",
                 data_grid: str = "legendre-gauss"):
        super().__init__()
        if activation_function not in ACTIVATIONS:
            raise ValueError(f"Unknown activation function {activation_function}")
        check_limits(in_chans, embed_dim, out_chans, use_disco_encoder, disco_kernel_size)
        self.img_shape = (int(img_shape[0]), int(img_shape[1]))
        self.use_disco_encoder, self.use_pos_embed, self.kernel_size = use_disco_encoder, pos_embed, disco_kernel_size
        self.dims = [in_chans, embed_dim, embed_dim, embed_dim, out_chans]
        act_layer, self.act = ACTIVATIONS[activation_function]
        # refused by name before any parameter is drawn: another grid, a grid the table cannot be built on
        self.table = _disco.disco_table(self.img_shape, disco_kernel_size, grid=data_grid) if use_disco_encoder else None
        mods = []
        cur = in_chans
        for i in range(3):
            if i == 0 and use_disco_encoder:
                mods.append(_GroupedDisco(cur, embed_dim, disco_kernel_size))
            else:
                mods.append(nn.Conv2d(cur, embed_dim, 1, bias=True))
            if i == 0 and pos_embed:
                mods.append(_AddPosEmbed(embed_dim, self.img_shape))
            mods.append(act_layer())
            cur = embed_dim
        mods.append(nn.Conv2d(cur, out_chans, 1, bias=False))
        self.mlp = nn.Sequential(*mods)
        self._prepared: Optional[Tuple[tuple, object, int, object]] = None      # (stamp, disco handle, mlp handle, mlp destroyer)
        self._hidden: Optional[torch.Tensor] = None

    # -- parameters in the net's order
    @property
    def _first(self) -> nn.Module:
        return self.mlp[0]

    @property
    def _convs(self):
        return [m for m in list(self.mlp)[1:] if isinstance(m, nn.Conv2d)]

    @property
    def _embed(self) -> Optional[torch.Tensor]:
        return self.mlp[1].pos_embed.detach() if self.use_pos_embed else None

    def _release(self, cur) -> None:
        if cur is None:
            return
        if cur[1] is not None:
            cur[1].close()
        cur[3](ctypes.c_void_p(cur[2]))

    def __del__(self):
        try:
            self._release(self.__dict__.get("_prepared"))
        except Exception:
            pass

    def __getstate__(self):
        """A copy (``copy.deepcopy``, pickling) prepares its own weights: the handles are one module's and die with it."""
        state = self.__dict__.copy()
        state["_prepared"] = None
        state["_hidden"] = None
        return state

    def _stamp(self) -> tuple:
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _handles(self):
        """(disco handle or None, pixel-mlp handle): rebuilt when any parameter's (data_ptr, _version) changed."""
        stamp = self._stamp()
        cur = self._prepared
        if cur is None or cur[0] != stamp:
            L = _lib.lib()
            dh = None
            convs = self._convs
            if self.use_disco_encoder:
                dw = self._first.conv
                dh = _disco.DiscoHandle(self.table, dw.weight, self.dims[0], self.dims[1], dw.groups, self.act, self.use_pos_embed)
                dims, acts, embed_layer = self.dims[1:], [self.act, self.act, _disco.ACT_NONE], -1
            else:
                convs = [self._first] + convs
                dims, acts, embed_layer = self.dims, [self.act, self.act, self.act, _disco.ACT_NONE], 0 if self.use_pos_embed else -1
            n = len(convs)
            ws = [c.weight.detach().reshape(c.out_channels, c.in_channels).float().contiguous() for c in convs]
            bs = [c.bias.detach().float().contiguous() if c.bias is not None else None for c in convs]
            h = ctypes.c_void_p()
            try:
                _check_mlp(L.ace_pixel_mlp_create2(
                    n, (ctypes.c_int * (n + 1))(*dims), (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws]),
                    (ctypes.c_void_p * n)(*[b.data_ptr() if b is not None else None for b in bs]), (ctypes.c_int * n)(*acts),
                    embed_layer, 1, _lib.current_stream(), ctypes.byref(h)))
            except Exception:
                if dh is not None:
                    dh.close()
                raise
            self._release(cur)
            self._prepared = (stamp, dh, h.value, L.ace_pixel_mlp_destroy)
        return self._prepared[1], ctypes.c_void_p(self._prepared[2])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4:
            raise ValueError(f"expected (batch, channels, rows, columns), got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("the AnkurLocalNet (ace_amd) runs on an MI355X only: move the module and its input to 'cuda'. There is no "
                               "CPU fallback.")
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("ace_amd implements the inference forward only; call under torch.no_grad()")
        return self._run(x)

    def _run(self, x: torch.Tensor) -> torch.Tensor:
        B, C, H, W = x.shape
        if C != self.dims[0]:
            raise ValueError(f"expected {self.dims[0]} input channels, got {C}")
        if (self.use_disco_encoder or self.use_pos_embed) and (H, W) != self.img_shape:
            raise ValueError(f"the module was built for {self.img_shape}, the input is {(H, W)}")
        y = torch.empty(B, self.dims[-1], H, W, dtype=torch.float32, device=x.device)
        self.forward_into(x.float().contiguous(), y)
        return y

    def forward_into(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """From the contiguous fp32 x (B, C, H, W) into y: one or two launches, no allocation after the first call of a batch size."""
        B, hw = x.shape[0], x.shape[2] * x.shape[3]
        dh, mh = self._handles()
        embed = self._embed
        ep = embed.data_ptr() if embed is not None else None
        src = x
        if dh is not None:
            hid = self._hidden
            if hid is None or hid.shape[0] != B or hid.device != x.device:
                hid = self._hidden = torch.empty(B, self.dims[1], x.shape[2], x.shape[3], dtype=torch.float32, device=x.device)
            dh.forward(x.data_ptr(), ep, hid.data_ptr(), B)
            src, ep = hid, None
        _check_mlp(_lib.lib().ace_pixel_mlp_forward(mh, src.data_ptr(), ep, y.data_ptr(), B, hw, _lib.current_stream()))


class AnkurLocalNet(nn.Module):
    """local_net.py:24-44: the wrapper whose forward takes (x, labels=None); keys "module.mlp...".  Labels are ignored."""

    def __init__(self, module: AnkurLocalNetModel):
        super().__init__()
        self.module = module

    def forward(self, x: torch.Tensor, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.module(x)

    def forward_into(self, x: torch.Tensor, y: torch.Tensor) -> None:
        self.module.forward_into(x, y)


@ModuleSelector.register("AnkurLocalNet")
@dataclasses.dataclass
class AnkurLocalNetBuilder(ModuleConfig):
    """fme/ace/registry/local_net.py:47-100 (same type string, same fields and defaults)."""
    embed_dim: int = 256
    use_disco_encoder: bool = True
    disco_kernel_size: int = 3
    pos_embed: bool = False
    activation_function: str = "gelu"

    def build(self, n_in_channels: int, n_out_channels: int, dataset_info) -> nn.Module:
        check_limits(n_in_channels, self.embed_dim, n_out_channels, self.use_disco_encoder, self.disco_kernel_size)
        return AnkurLocalNet(AnkurLocalNetModel(
            img_shape=dataset_info.img_shape, in_chans=n_in_channels, out_chans=n_out_channels, embed_dim=self.embed_dim,
            use_disco_encoder=self.use_disco_encoder, disco_kernel_size=self.disco_kernel_size, pos_embed=self.pos_embed,
            activation_function=self.activation_function, data_grid="legendre-gauss"))
