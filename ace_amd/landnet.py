"""LandNet (registry type "LandNet": fme/ace/registry/land_net.py, fme/ace/models/land/land_net.py) - a per-pixel chain of
Conv2d(1 x 1) + ReLU per hidden width, an optional learned (1, hidden_dims[0], H, W) positional embedding added after the first
ReLU, and a last Conv2d(1 x 1) - on the fused per-pixel MLP kernel (``ace_pixel_mlp_*``, csrc/pixel_mlp.hip): one launch per
forward in exact fp32, the hidden activations never leaving the registers.

The module holds the reference's parameters in the reference's construction order (same seeded initialisation, same state-dict
keys: "pos_embed.pos_embed", "model.0.layers.0.weight", "model.0.layers.0.bias", "model.1.layers.0.weight", ...); only
``forward`` is native.  No CPU path."""
import ctypes
import dataclasses
import functools
from typing import List, Optional, Tuple

import torch
from torch import nn

from . import _lib
from .registry import ModuleConfig, ModuleSelector

# include/ace_sfno.h
MAX_LAYERS, MAX_WIDTH = 8, 256
ACT_NONE, ACT_RELU = 0, 1


_check = functools.partial(_lib.check, family="pixel_mlp")


class _PositionalEmbedding(nn.Module):
    """layers.py:5-12: the parameter's holder (key "pos_embed.pos_embed")."""

    def __init__(self, channels: int, height: int, width: int):
        super().__init__()
        self.pos_embed = nn.Parameter(torch.randn(1, channels, height, width))


class _PixelLayer(nn.Module):
    """layers.py:15-36: the parameters' holder of one Conv2d(1 x 1) + activation (keys "layers.0.weight", "layers.0.bias")."""

    def __init__(self, input_dim: int, output_dim: int, relu: bool):
        super().__init__()
        self.layers = nn.Sequential(nn.Conv2d(input_dim, output_dim, kernel_size=(1, 1)), nn.ReLU() if relu else nn.Identity())
        self.relu = relu

    @property
    def conv(self) -> nn.Conv2d:
        return self.layers[0]


def check_limits(input_channels: int, hidden_dims: List[int], output_channels: int) -> None:
    """What the kernel's exported limits refuse, by name."""
    if len(hidden_dims) + 1 > MAX_LAYERS:
        raise NotImplementedError(f"LandNet: {len(hidden_dims) + 1} layers exceed ACE_PIXEL_MLP_MAX_LAYERS = {MAX_LAYERS}")
    widest = max([input_channels, output_channels] + list(hidden_dims))
    if widest > MAX_WIDTH:
        raise NotImplementedError(f"LandNet: a width of {widest} channels exceeds ACE_PIXEL_MLP_MAX_WIDTH = {MAX_WIDTH}")


class LandNet(nn.Module):
    def __init__(self, img_shape: tuple, input_channels: int, hidden_dims: List[int], output_channels: int,
                 network_type: str = "MLP", activation=nn.ReLU, use_positional_embedding: bool = False):
        super().__init__()
        if network_type != "MLP":
            raise ValueError(f"Unsupported network type: {network_type}")
        if activation is not nn.ReLU:
            raise NotImplementedError("LandNet (ace_amd): the fused kernel's hidden activation is ReLU (the registry's only one)")
        hidden_dims = list(hidden_dims)
        check_limits(input_channels, hidden_dims, output_channels)
        self.img_shape = tuple(img_shape)
        self.use_positional_embedding = use_positional_embedding
        if use_positional_embedding:
            self.pos_embed = _PositionalEmbedding(hidden_dims[0], img_shape[0], img_shape[1])
        self.num_layers = len(hidden_dims)
        dims = [input_channels] + hidden_dims
        layers = [_PixelLayer(a, b, relu=True) for a, b in zip(dims[:-1], dims[1:])]
        layers.append(_PixelLayer(dims[-1], output_channels, relu=False))
        self.model = nn.Sequential(*layers)
        self.dims = dims + [output_channels]
        self._prepared: Optional[Tuple[tuple, int, object]] = None      # (stamp, handle, destroyer)

    def __del__(self):
        try:
            cur = self.__dict__.get("_prepared")
            if cur is not None:
                cur[2](ctypes.c_void_p(cur[1]))
        except Exception:
            pass

    def __getstate__(self):
        """A copy (``copy.deepcopy``, pickling) prepares its own weights: the handle is one module's and dies with it."""
        state = self.__dict__.copy()
        state["_prepared"] = None
        return state

    def _stamp(self) -> tuple:
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _handle(self) -> ctypes.c_void_p:
        """The prepared weights: rebuilt when any parameter's (data_ptr, _version) changed."""
        stamp = self._stamp()
        cur = self._prepared
        if cur is None or cur[0] != stamp:
            L = _lib.lib()
            n = len(self.model)
            convs = [m.conv for m in self.model]
            ws = [c.weight.detach().reshape(c.out_channels, c.in_channels).float().contiguous() for c in convs]
            bs = [c.bias.detach().float().contiguous() if c.bias is not None else None for c in convs]
            h = ctypes.c_void_p()
            _check(L.ace_pixel_mlp_create(
                n, (ctypes.c_int * (n + 1))(*self.dims), (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws]),
                (ctypes.c_void_p * n)(*[b.data_ptr() if b is not None else None for b in bs]),
                (ctypes.c_int * n)(*[ACT_RELU if m.relu else ACT_NONE for m in self.model]),
                0 if self.use_positional_embedding else -1, _lib.current_stream(), ctypes.byref(h)))
            if cur is not None:
                cur[2](ctypes.c_void_p(cur[1]))
            self._prepared = (stamp, h.value, L.ace_pixel_mlp_destroy)
        return ctypes.c_void_p(self._prepared[1])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4:
            raise ValueError(f"expected (batch, channels, rows, columns), got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("the LandNet (ace_amd) runs on an MI355X only: move the module and its input to 'cuda'. There is no CPU "
                               "fallback.")
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("ace_amd implements the inference forward only; call under torch.no_grad()")
        return self._run(x)

    def _run(self, x: torch.Tensor) -> torch.Tensor:
        B, C, H, W = x.shape
        if C != self.dims[0]:
            raise ValueError(f"expected {self.dims[0]} input channels, got {C}")
        if self.use_positional_embedding and (H, W) != self.img_shape:
            raise ValueError(f"the positional embedding is {self.img_shape}, the input {(H, W)}")
        y = torch.empty(B, self.dims[-1], H, W, dtype=torch.float32, device=x.device)
        self.forward_into(x.float().contiguous(), y)
        return y

    def forward_into(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """One ``ace_pixel_mlp_forward`` from the contiguous fp32 x (B, C, H, W) into y: no allocation (the engine's call)."""
        embed = self.pos_embed.pos_embed.detach() if self.use_positional_embedding else None
        _check(_lib.lib().ace_pixel_mlp_forward(self._handle(), x.data_ptr(), embed.data_ptr() if embed is not None else None,
                                                y.data_ptr(), x.shape[0], x.shape[2] * x.shape[3], _lib.current_stream()))


@ModuleSelector.register("LandNet")
@dataclasses.dataclass
class LandNetBuilder(ModuleConfig):
    """fme/ace/registry/land_net.py:9-37 (same type string, same fields and defaults)."""
    hidden_dims: List[int] = dataclasses.field(default_factory=lambda: [64, 64])
    network_type: str = "MLP"
    use_positional_embedding: bool = False

    def build(self, n_in_channels: int, n_out_channels: int, dataset_info) -> nn.Module:
        if len(getattr(dataset_info, "all_labels", ())) > 0:
            raise ValueError("LandNet does not support labels")
        if self.network_type != "MLP":
            raise ValueError(f"LandNet: network_type must be MLP, got {self.network_type!r}")
        check_limits(n_in_channels, list(self.hidden_dims), n_out_channels)
        return LandNet(img_shape=dataset_info.img_shape, input_channels=n_in_channels, output_channels=n_out_channels,
                       hidden_dims=list(self.hidden_dims), network_type=self.network_type,
                       use_positional_embedding=self.use_positional_embedding)
