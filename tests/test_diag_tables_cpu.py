"""The host side every fused diag call shares (ace_amd/aggregator.py): the pointer / stride table of a window's planes with its
named byte offsets, and the accumulator that grows when a new name comes in.  Both are pure torch on CPU tensors."""
import torch

from ace_amd.aggregator import _grow, _plane_table

NAMES = ["a", "b", "c"]


def fields():
    a = torch.zeros(2, 3, 4, 5)
    b = torch.zeros(2, 6, 4, 5)[:, ::2]                 # a time-strided view: stride(0), stride(1) = 120, 40
    c = torch.zeros(2, 3, 4, 5)
    assert b.shape == a.shape and b.stride(1) == 40 and not b.is_contiguous()
    gen = {"a": a, "b": b, "c": c}
    tgt = {"a": torch.zeros(2, 3, 4, 5), "b": torch.zeros(2, 6, 4, 5)[:, ::2]}      # "c" has no target
    return gen, tgt


def test_plane_table_of_two_sides():
    gen, tgt = fields()
    values, off = _plane_table(NAMES, gen, tgt)
    n = len(NAMES)
    want = [gen[k].data_ptr() for k in NAMES]
    want += [60, 20, 120, 40, 60, 20]
    want += [tgt["a"].data_ptr(), tgt["b"].data_ptr(), 0]
    want += [60, 20, 120, 40, 0, 0]
    assert values == want and all(type(v) is int for v in values)
    assert off == {"gen": 0, "gen_strides": 8 * n, "target": 24 * n, "target_strides": 32 * n, "end": 48 * n}
    # the missing target: pointer 0 and strides 0, 0
    assert values[off["target"] // 8 + 2] == 0 and values[off["target_strides"] // 8 + 4:off["end"] // 8] == [0, 0]
    assert torch.tensor(values, dtype=torch.int64).tolist() == values


def test_plane_table_of_one_side_and_name_order():
    gen, _ = fields()
    values, off = _plane_table(NAMES, gen)
    n = len(NAMES)
    assert values == [gen[k].data_ptr() for k in NAMES] + [60, 20, 120, 40, 60, 20]
    assert off == {"gen": 0, "gen_strides": 8 * n, "end": 24 * n}
    # the order is that of the names given, not of the mapping
    back, _ = _plane_table(NAMES[::-1], gen)
    assert back[:n] == values[:n][::-1] and back[n:] == [60, 20, 120, 40, 60, 20]


def test_grow_keeps_the_old_block_in_the_leading_corner():
    old = torch.arange(14, dtype=torch.int64).reshape(2, 1, 7) + 1
    new = _grow(old, (2, 3, 7), torch.int64, "cpu")
    assert new.shape == (2, 3, 7) and new.dtype == torch.int64
    assert torch.equal(new[:, :1], old) and int(new[:, 1:].abs().sum()) == 0
    assert new.data_ptr() != old.data_ptr()
    fresh = _grow(None, (2, 3), torch.float64, "cpu")
    assert fresh.dtype == torch.float64 and fresh.shape == (2, 3) and not bool(fresh.any())
