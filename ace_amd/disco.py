"""The psi table of the DISCO convolution on the sphere (fme/core/disco/_convolution.py:101-197, _filter_basis.py:169-226 - the
morlet basis - and _quadrature.py), built on the host for the fused DISCO kernel (``ace_disco_*``, csrc/disco.hip).

Settings are the reference's for ``AnkurLocalNet`` and the "disco" blocks of ``LocalNet``: basis "morlet", kernel_shape (ks, ks),
K = ks * ks, theta_cutoff = (ks + 1) * 0.5 * pi / (nlat - 1), theta_eps = 1e-3, basis_norm_mode "mean", the quadrature merged,
input shape == output shape.  Everything else is refused by name.

Roundings, as the reference takes them: Gauss nodes and weights from numpy in fp64, the geometry in fp64, the norm table
vnorm[k, row] held in fp32 with its mean over rows taken in fp32 and eps = 1e-9 added in fp32, the quadrature merged in fp64, one
rounding to fp32 at the end.  All K basis functions share one support per output row (the disk theta <= (1 + theta_eps) cutoff),
so the table is, per output row ho, the support points (hi, wi) in ascending (hi, wi) and K fp32 values per point; a value that is
exactly 0 stays (it decides where a NaN of the input spreads)."""
import ctypes
import dataclasses
import functools
import math
from typing import Tuple

import numpy as np
import torch

from . import _lib

THETA_EPS = 1e-3
NORM_EPS = 1e-9


@dataclasses.dataclass(frozen=True)
class DiscoTable:
    img_shape: Tuple[int, int]
    kernel_size: int
    row_offsets: np.ndarray        # int64 [H + 1]: points of output row ho are row_offsets[ho] .. row_offsets[ho + 1]
    hi: np.ndarray                 # int32 [P] input row of a point
    wi: np.ndarray                 # int32 [P] input column of a point at output column 0 (column (wi + wo) mod W at wo)
    vals: np.ndarray               # float32 [P][K]

    @property
    def K(self) -> int:
        return self.kernel_size * self.kernel_size


def theta_cutoff(nlat: int, kernel_size: int) -> float:
    return (kernel_size + 1) * 0.5 * math.pi / float(nlat - 1)


def _refuse(img_shape, kernel_size, grid, basis, basis_norm_mode, out_shape):
    if basis != "morlet":
        raise NotImplementedError(f"disco_table: basis {basis!r} is not built (only 'morlet')")
    if basis_norm_mode != "mean":
        raise NotImplementedError(f"disco_table: basis_norm_mode {basis_norm_mode!r} is not built (only 'mean')")
    if grid != "legendre-gauss":
        raise NotImplementedError(f"disco_table: grid {grid!r} is not built (only 'legendre-gauss')")
    if out_shape is not None and tuple(out_shape) != tuple(img_shape):
        raise NotImplementedError(f"disco_table: out_shape {tuple(out_shape)} differs from the input shape {tuple(img_shape)}")
    if len(img_shape) != 2 or img_shape[0] < 2 or img_shape[1] < 1:
        raise ValueError(f"disco_table: img_shape must be (nlat >= 2, nlon >= 1), got {tuple(img_shape)}")
    if kernel_size < 1:
        raise ValueError(f"disco_table: kernel_size must be >= 1, got {kernel_size}")


def disco_table(img_shape, kernel_size: int, grid: str = "legendre-gauss", basis: str = "morlet", basis_norm_mode: str = "mean",
                out_shape=None) -> DiscoTable:
    _refuse(img_shape, kernel_size, grid, basis, basis_norm_mode, out_shape)
    return _table(int(img_shape[0]), int(img_shape[1]), int(kernel_size))


@functools.lru_cache(maxsize=8)
def _table(H: int, W: int, ks: int) -> DiscoTable:
    K = ks * ks
    nodes, wts = np.polynomial.legendre.leggauss(H)
    colat = torch.flip(torch.arccos(torch.as_tensor(nodes).clone()), dims=(0,))          # ascending colatitude, fp64
    quad = torch.flip(torch.as_tensor(wts).clone(), dims=(0,)) / W / 2.0                   # per input row
    lon = torch.linspace(0, 2 * math.pi, W + 1, dtype=torch.float64)[:-1]
    r_cut = (1.0 + THETA_EPS) * theta_cutoff(H, ks)

    cb, sb = torch.cos(lon)[None, :], torch.sin(lon)[None, :]
    cg, sg = torch.cos(colat)[:, None], torch.sin(colat)[:, None]
    kk = torch.arange(K)
    n_mode = (kk % ks)[:, None]
    m_mode = (kk // ks)[:, None]
    n_freq = torch.ceil(n_mode / 2) * math.pi
    m_freq = torch.ceil(m_mode / 2) * math.pi

    rows_hi, rows_wi, rows_raw = [], [], []
    vnorm = torch.zeros(K, H)                                                              # fp32, as the reference holds it
    for ho in range(H):
        # the grid seen from output point (colat[ho], lon 0): a rotation about y by -colat[ho]
        a = -colat[ho]
        ca, sa = torch.cos(a), torch.sin(a)
        x = ca * cb * sg + cg * sa
        y = sb * sg
        z = -cb * sa * sg + ca * cg
        nrm = torch.sqrt(x * x + y * y + z * z)
        x, y, z = x / nrm, y / nrm, z / nrm
        theta = torch.arccos(z)
        phi = torch.arctan2(y, x)
        phi = torch.where(phi < 0.0, phi + 2 * torch.pi, phi)
        pts = torch.argwhere(theta <= r_cut)                                               # ascending (hi, wi)
        hi, wi = pts[:, 0], pts[:, 1]
        r = theta[hi, wi] / r_cut
        ph = phi[hi, wi]
        px, py = r * torch.sin(ph), r * torch.cos(ph)
        harm = torch.where(n_mode % 2 == 1, torch.sin(n_freq * px), torch.cos(n_freq * px))
        harm = harm * torch.where(m_mode % 2 == 1, torch.sin(m_freq * py), torch.cos(m_freq * py))
        raw = torch.cos(0.5 * torch.pi * r) ** 2 * harm                                    # [K][points], fp64
        q = quad[hi]
        for k in range(K):
            vnorm[k, ho] = torch.sum(raw[k].abs() * q)
        rows_hi.append(hi)
        rows_wi.append(wi)
        rows_raw.append((raw, q))
    denom = torch.stack([vnorm[k, :].mean() + NORM_EPS for k in range(K)])                 # fp32: the mean and the eps
    denom = denom.double()[:, None]
    vals = [((raw / denom) * q[None, :]).to(torch.float32).t().contiguous() for raw, q in rows_raw]
    offs = np.zeros(H + 1, np.int64)
    offs[1:] = np.cumsum([len(h) for h in rows_hi])
    return DiscoTable((H, W), ks, offs, torch.cat(rows_hi).numpy().astype(np.int32), torch.cat(rows_wi).numpy().astype(np.int32),
                      torch.cat(vals).numpy())


# include/ace_sfno.h
ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU = 0, 1, 2, 3
MAX_K, MAX_PRODUCTS = 25, 512
ACTIVATIONS = {"relu": ACT_RELU, "gelu": ACT_GELU, "silu": ACT_SILU}


def check_limits(in_chans: int, out_chans: int, kernel_size: int, who: str = "disco") -> None:
    """What ``ace_disco_create`` refuses for its limits, by name, before anything is built."""
    K = kernel_size * kernel_size
    if kernel_size < 1 or K > MAX_K:
        raise NotImplementedError(f"{who}: kernel_size {kernel_size} gives K = {K} basis functions, over ACE_DISCO_MAX_K = {MAX_K}")
    gs = in_chans // math.gcd(in_chans, out_chans)
    if gs * K > MAX_PRODUCTS:
        raise NotImplementedError(f"{who}: {in_chans} -> {out_chans} channels give groupsize * K = {gs * K} products per output, over "
                                  f"ACE_DISCO_MAX_PRODUCTS = {MAX_PRODUCTS}")


_check = functools.partial(_lib.check, family="disco")


class DiscoHandle:
    """One ``ace_disco_create`` handle: the table, the DEVICE weight [out][in / groups][K] (read once, now), the activation and
    whether an embedding [out][H][W] is added before it.  ``forward`` is the one launch."""
    handle = None

    def __init__(self, table: DiscoTable, weight: torch.Tensor, in_chans: int, out_chans: int, groups: int, act: int = ACT_NONE,
                 has_embed: bool = False):
        self._destroy = _lib.lib().ace_disco_destroy
        self.table, self.in_chans, self.out_chans = table, in_chans, out_chans
        offs = np.ascontiguousarray(table.row_offsets, dtype=np.int64)
        hi = np.ascontiguousarray(table.hi, dtype=np.int32)
        wi = np.ascontiguousarray(table.wi, dtype=np.int32)
        vals = np.ascontiguousarray(table.vals, dtype=np.float32)
        w = weight.detach().float().contiguous()
        if tuple(w.shape) != (out_chans, in_chans // max(groups, 1), table.K):
            raise ValueError(f"the weight is {tuple(w.shape)}, expected {(out_chans, in_chans // max(groups, 1), table.K)}")
        h = ctypes.c_void_p()
        _check(_lib.lib().ace_disco_create(table.img_shape[0], table.img_shape[1], table.K, offs.ctypes.data, hi.ctypes.data,
                                           wi.ctypes.data, vals.ctypes.data, w.data_ptr(), in_chans, out_chans, groups, act,
                                           1 if has_embed else 0, _lib.current_stream(), ctypes.byref(h)))
        self.handle = h.value

    def forward(self, x_ptr, embed_ptr, y_ptr, batch: int) -> None:
        _check(_lib.lib().ace_disco_forward(ctypes.c_void_p(self.handle), x_ptr, embed_ptr, y_ptr, batch, _lib.current_stream()))

    def info(self) -> dict:
        out = (ctypes.c_long * 4)()
        _check(_lib.lib().ace_disco_info(ctypes.c_void_p(self.handle), out))
        return {"units": out[0], "heaviest_unit_cost": out[1], "total_cost": out[2], "lds_bytes": out[3]}

    def close(self) -> None:
        if self.handle:
            self._destroy(ctypes.c_void_p(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
