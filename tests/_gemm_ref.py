"""The fused contract of the tile GEMM engines (ace_amd/csrc/kernels.h `GemmArgs`, C ABI `ace_conv1x1_fused`) stated in plain torch, the
cases tests/test_gpu_gemm_engines.py holds the three kernels to, and their inputs.  tests/test_gemm_ref_cpu.py holds this file itself.

    y = min(act(W . affine(x || x2) + bias + (res * res_scale + res_shift)), cap) * out_scale + out_shift

A case names a shape, the options that are switched on, the activation and the pitches; it is the same for every engine.  An engine
that does not take an option of a case (the direct-to-LDS engine has no input affine) runs the case without that option
(`for_engine`), or does not run it at all when nothing would be left of it."""

import dataclasses
import functools
import math
import zlib

import torch

OP_TOL = 2e-6   # the operator bar of tests/test_gpu_parity.py
ENGINES = (0, 1, 2)   # 0 fp32 register-staged, 1 fp32 direct to LDS, 2 f16x3
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SILU = 0, 1, 2, 3
OPTIONS = ("bias", "in_affine", "res", "res_affine", "out_affine", "absmax")
G3_KAFF = 1024   # rows of the f16x3 kernel's affine table in LDS


@dataclasses.dataclass(frozen=True)
class Case:
    sweep: str
    n: int
    cin: int
    cin2: int
    cout: int
    hw: int
    opts: tuple = ()
    act: int = ACT_NONE
    cap: float = math.inf
    in_extra: int = 0      # in_pitch - hw
    out_extra: int = 0     # out_pitch - hw
    misalign: bool = False   # x starts 4 bytes off a 16-byte boundary

    @property
    def K(self):
        return self.cin + self.cin2

    @property
    def id(self):
        o = "+".join(self.opts) if self.opts else "plain"
        s = f"{self.sweep}-n{self.n}-k{self.cin}+{self.cin2}-m{self.cout}-hw{self.hw}-{o}-act{self.act}"
        if self.cap != math.inf:
            s += f"-cap{self.cap:g}"
        if self.in_extra or self.out_extra:
            s += f"-pitch+{self.in_extra}+{self.out_extra}"
        return s + ("-misaligned" if self.misalign else "")


def tile_rule(M):
    """1 = 128 x 128 iff M >= 128 and the rows wasted at 128 are no more than at 64, else 0 = 64 x 256"""
    waste128 = -M % 128
    waste64 = -M % 64
    return 1 if M >= 128 and waste128 <= waste64 else 0


def takes(case, engine):
    """does `engine` take the case as it stands (ace_conv1x1_fused returns ACE_ERR_INVALID otherwise)"""
    aligned = case.hw % 4 == 0 and (case.hw + case.in_extra) % 4 == 0 and not case.misalign
    if engine == 0:
        return True
    if engine == 1:
        return aligned and "in_affine" not in case.opts
    return aligned and ("in_affine" not in case.opts or -(-case.K // 32) * 32 <= G3_KAFF)


def for_engine(case, engine):
    """the case as `engine` runs it, or None: engine 1 runs a case without its input affine unless that was all the case switched on"""
    if engine == 1 and "in_affine" in case.opts:
        rest = tuple(o for o in case.opts if o != "in_affine")
        if not rest:
            return None
        case = dataclasses.replace(case, opts=rest)
    return case if takes(case, engine) else None


def expected_route(case, engine):
    """(family, tile) the launch must take: family 0 register-staged 4-byte loads, 1 register-staged 16-byte loads, 2 direct to LDS,
    3 f16x3 (the operands of the tests are 16-byte aligned unless the case says otherwise)"""
    if engine == 0:
        vec = case.hw % 4 == 0 and (case.hw + case.in_extra) % 4 == 0 and case.K % 4 == 0 and not case.misalign
        return (1 if vec else 0, tile_rule(case.cout))
    return (2 if engine == 1 else 3, tile_rule(case.cout))


# --------------------------------------------------------------------------------------------- the case lists
ALL = OPTIONS
ROWS_M = (1, 63, 64, 65, 127, 128, 129, 192, 200, 250, 256, 257)
ROWS_M_TILE128 = (128, 200, 250, 256)
COLS_HW = (4, 8, 124, 128, 132, 252, 256, 260, 516)
COLS_HW_SCALAR = (1, 3, 13, 257)   # engine 0 only: the 4-byte family
CONTRACTION = ((1, 0), (3, 0), (4, 0), (15, 0), (16, 0), (17, 0), (28, 0), (32, 0), (36, 0), (64, 0), (68, 0),
               (32, 32), (30, 6), (16, 1), (1, 16), (33, 31))
OPTION_SHAPES = ((65, 260, 30, 6), (200, 132, 30, 6))   # (cout, hw, cin, cin2): one ragged shape per tile


def _both(sweep, cin, cin2, cout, hw):
    """a shape once with no option (batch 1) and once with all of them (batch 3: the per-sample strides of the affines are used)"""
    return [Case(sweep, 1, cin, cin2, cout, hw),
            Case(sweep, 3, cin, cin2, cout, hw, opts=ALL, act=ACT_GELU, cap=1.5)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for m in ROWS_M:
        out += _both("rows", 36, 0, m, 260)
    for m in (65, 200):
        for hw in COLS_HW + COLS_HW_SCALAR:
            out += _both("cols", 36, 0, m, hw)
    for cin, cin2 in CONTRACTION:
        out += _both("k", cin, cin2, 65, 132)
    # the last entry of the f16x3 kernel's 1024-row affine table (engine 2; engine 0 runs it as well, engine 1 without the affine)
    out.append(Case("k", 3, 1020, 4, 64, 256, opts=ALL, act=ACT_GELU, cap=1.5))
    for cout, hw, cin, cin2 in OPTION_SHAPES:
        one = functools.partial(Case, "opt", 3, cin, cin2, cout, hw)
        out += [one(opts=("in_affine",)), one(opts=("res",)), one(opts=("res", "res_affine")), one(opts=("out_affine",)),
                one(opts=("absmax",))]
        out += [one(act=a, cap=1.5) for a in (ACT_NONE, ACT_GELU, ACT_RELU, ACT_SILU)]
        out += [one(opts=ALL, act=ACT_GELU, cap=1.5, in_extra=e, out_extra=e) for e in (4, 36)]
        # beyond the pitches that keep every row 16-byte aligned: a y pitch that does not (the engines' 4-byte stores) and an x that
        # starts off a 16-byte boundary (engine 0 only: the 4-byte family at a size that would take 16-byte loads)
        out += [one(opts=ALL, act=ACT_GELU, cap=1.5, out_extra=3), one(opts=ALL, act=ACT_GELU, cap=1.5, misalign=True)]
    assert len({c.id for c in out}) == len(out)
    return tuple(out)


def engine_cases():
    """every (case as the engine runs it, engine) pair of the GPU tests"""
    out = []
    for c in cases():
        for e in ENGINES:
            ce = for_engine(c, e)
            if ce is not None:
                out.append((ce, e))
    return out


# what each engine refuses (ACE_ERR_INVALID): (case, engine)
REFUSALS = (
    (Case("refuse", 1, 36, 0, 65, 132, opts=("in_affine",)), 1),              # no input affine on the direct-to-LDS engine
    (Case("refuse", 1, 36, 0, 65, 130), 1),                                   # hw % 4 != 0
    (Case("refuse", 1, 36, 0, 65, 130), 2),
    (Case("refuse", 1, 36, 0, 65, 132, in_extra=2), 1),                       # rows off 16-byte boundaries
    (Case("refuse", 1, 36, 0, 65, 132, in_extra=2), 2),
    (Case("refuse", 1, 36, 0, 65, 132, misalign=True), 1),                    # a base off a 16-byte boundary
    (Case("refuse", 1, 36, 0, 65, 132, misalign=True), 2),
    (Case("refuse", 1, 1024, 4, 64, 256, opts=("in_affine",)), 2),            # 1056 padded rows do not fit the 1024-row affine table
)


# --------------------------------------------------------------------------------------------- inputs and the formula
@functools.lru_cache(maxsize=None)
def inputs(case):
    """the case's operands, fp32, seeded by the case: x, x2, res ~ N(0, 1); W ~ N(0, 1) / sqrt(K); scales uniform in [0.5, 1.5];
    shifts 0.3 N(0, 1); bias and out_shift N(0, 1).  Built once per case and only read afterwards."""
    g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    n, K, M, hw = case.n, case.K, case.cout, case.hw

    def randn(*shape):
        return torch.randn(*shape, generator=g)

    def scale(*shape):
        return 0.5 + torch.rand(*shape, generator=g)

    d = {"x": randn(n, case.cin, hw), "x2": randn(n, case.cin2, hw) if case.cin2 else None, "weight": randn(M, K) / K ** 0.5}
    d["bias"] = randn(M) if "bias" in case.opts else None
    d["in_scale"], d["in_shift"] = (scale(n, K), 0.3 * randn(n, K)) if "in_affine" in case.opts else (None, None)
    d["res"] = randn(n, M, hw) if "res" in case.opts else None
    d["res_scale"], d["res_shift"] = (scale(n, M), 0.3 * randn(n, M)) if "res_affine" in case.opts else (None, None)
    d["out_scale"], d["out_shift"] = (scale(M), randn(M)) if "out_affine" in case.opts else (None, None)
    return d


def activation(v, act):
    F = torch.nn.functional
    return [v, F.gelu(v), torch.relu(v), F.silu(v)][act]


def fused(d, act, cap, dtype):
    """the formula, every operand converted to `dtype` first"""
    t = {k: (v.to(dtype) if v is not None else None) for k, v in d.items()}
    x = t["x"] if t["x2"] is None else torch.cat([t["x"], t["x2"]], dim=1)
    if t["in_scale"] is not None:
        x = x * t["in_scale"][:, :, None] + t["in_shift"][:, :, None]
    v = torch.einsum("ok,nkp->nop", t["weight"], x)
    if t["bias"] is not None:
        v = v + t["bias"][None, :, None]
    if t["res"] is not None:
        r = t["res"]
        if t["res_scale"] is not None:
            r = r * t["res_scale"][:, :, None] + t["res_shift"][:, :, None]
        v = v + r
    v = activation(v, act)
    if cap != math.inf:
        v = torch.minimum(v, torch.tensor(cap, dtype=dtype))
    if t["out_scale"] is not None:
        v = v * t["out_scale"][None, :, None] + t["out_shift"][None, :, None]
    return v


@functools.lru_cache(maxsize=None)
def truth(case):
    """the fp64 result of the case, computed once and only read afterwards"""
    return fused(inputs(case), case.act, case.cap, torch.float64)
