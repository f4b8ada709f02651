"""TEST INFRASTRUCTURE: the grids and channel counts the DISCO kernel is held to, seeded operands, and the numpy statement's
pre-activation computed once per case (tests/_disco_ref.py) and shared by the tests that need it."""
import functools
import math

import numpy as np

import _disco_ref as R
from ace_amd.disco import disco_table

# (H, W, kernel_size): (6, 8) four rows wrap every longitude, band 5 of 6 rows, W below any pixel run; (9, 20) K = 4, band of 3;
# (24, 70) K = 16, W no multiple of the run
GRIDS = [(6, 8, 3), (8, 16, 3), (9, 20, 2), (16, 36, 3), (24, 70, 4)]
# (in, hidden): 6 groups of 1 with 4 outputs each; 1 group of 5 (45 / 20 / 80 products); 4 groups of 3; depthwise
CHANNELS = [(6, 24), (5, 24), (12, 32), (8, 8)]
BIG = ((8, 16, 3), (30, 256))                                 # 2 groups of 15: 135 products, 128 outputs per group
CASES = [(g, c) for g in GRIDS for c in CHANNELS] + [BIG]


def case_id(case) -> str:
    (H, W, ks), (cin, cout) = case
    return f"{H}x{W}k{ks}-{cin}to{cout}"


def batch_of(case) -> int:
    return 1 + (CASES.index(case) % 2)


@functools.lru_cache(maxsize=None)
def operands(case):
    """(table, x [B][in][H][W], w [out][gs][K], embed [out][H][W], groups), seeded by the case."""
    (H, W, ks), (cin, cout) = case
    groups = math.gcd(cin, cout)
    rng = np.random.default_rng(1000 + CASES.index(case))
    t = disco_table((H, W), ks)
    B = batch_of(case)
    x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    w = rng.standard_normal((cout, cin // groups, ks * ks)).astype(np.float32)
    e = rng.standard_normal((cout, H, W)).astype(np.float32)
    for a in (x, w, e):
        a.setflags(write=False)
    return t, x, w, e, groups


@functools.lru_cache(maxsize=None)
def statement_mix(case):
    """The statement's accumulator before embedding and activation (read-only, shared)."""
    t, x, w, _, groups = operands(case)
    y = R.disco_mix(R.disco_z(x, t), w, groups)
    y.setflags(write=False)
    return y


def statement(case, act, embed: bool, pre_activation=False):
    t, x, w, e, groups = operands(case)
    acc = statement_mix(case)
    if embed:
        acc = (acc + e[None]).astype(np.float32)
    if pre_activation or act == R.ACT_NONE:
        return np.array(acc)
    assert act == R.ACT_RELU
    return R.relu(acc)
