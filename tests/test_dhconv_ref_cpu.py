"""tests/_dhconv_ref.py, the torch statement of the spectral filter contraction that tests/test_gpu_dhconv_strip.py holds
ace_amd/csrc/dhconv_strip.hip to.

1. Conditioning (test_fp32_evaluation_is_within_half_the_bar): for EVERY case of the list a plain fp32 evaluation of the einsum stays
   within OP_TOL / 2 = 1e-6 of the fp64 one in the PER-DEGREE metric.  This is what makes OP_TOL = 2e-6 a fair bar for the kernel on
   these inputs: a correct fp32-class kernel has half the bar to spare.  A case that breaks it gets other inputs, not another bar.
2. The two einsums against loops that share no code with them, the grouped one against the dense one on the expanded filter, and the
   zeroing of the coefficients with m > l.
3. The metric: a defect confined to one weak degree shows in full in the per-degree figure and vanishes in the whole-tensor one.
4. The case list takes the branches it is meant to take (expected_route restated on its own)."""

import pytest
import torch

import _dhconv_ref as R


def unique_inputs():
    seen = {}
    for c in R.cases():
        seen.setdefault(c.data_key, c)
    return list(seen.values())


@pytest.mark.parametrize("case", unique_inputs(), ids=lambda c: c.id)
def test_fp32_evaluation_is_within_half_the_bar(case):
    x, w = R.inputs(case)
    ref = R.truth(case)
    assert torch.isfinite(torch.view_as_real(ref)).all()
    err, l, whole = R.degree_errors(R.contract(x, w, case.groups, torch.float32), ref)
    print(f"{case.id}: fp32 einsum vs fp64, worst degree {err:.3e} (l = {l}), whole tensor {whole:.3e}")
    assert err <= R.OP_TOL / 2, (case.id, err, l)


def test_einsums_against_loops_and_each_other():
    n, C, L, Mm, G = 2, 8, 5, 4, 2
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, C, L, Mm, 2, generator=g)            # m > l NOT zeroed: contract() has to
    wg = torch.randn(G, L, C // G, C // G, 2, generator=g)
    wd = R.expand_grouped(wg, C, G)
    xc, wc = torch.view_as_complex(x.double()), torch.view_as_complex(wd.double())
    want = torch.zeros(n, C, L, Mm, dtype=torch.complex128)
    for b in range(n):
        for o in range(C):
            for l in range(L):
                for m in range(min(l + 1, Mm)):
                    want[b, o, l, m] = sum(xc[b, i, l, m] * wc[i, o, l] for i in range(C))
    dense = R.contract(x, wd, 1, torch.float64)
    grouped = R.contract(x, wg, G, torch.float64)
    assert float((dense - want).abs().max()) <= 1e-13
    assert float((grouped - want).abs().max()) <= 1e-13
    assert float(want[:, :, 0, 1:].abs().max()) == 0.0 and float(dense[:, :, 1, 2:].abs().max()) == 0.0
    # the blocks between groups are exact zeros, the diagonal blocks the parameter transposed
    cg = C // G
    assert float(wd[:cg, cg:].abs().max()) == 0.0 and float(wd[cg:, :cg].abs().max()) == 0.0
    assert torch.equal(wd[cg + 1, cg + 2, 3], wg[1, 3, 2, 1])


def test_metric_sees_a_weak_degree():
    case = R.Case("cols", 5, 128, 24, 25)
    ref = R.truth(case)
    bad = ref.clone()
    bad[:, :, 23] *= 1.0 + 1e-4              # a relative error of 1e-4 in the weakest degree only
    err, l, whole = R.degree_errors(bad, ref)
    assert l == 23 and 0.99e-4 <= err <= 1.01e-4
    assert whole < R.OP_TOL / 100, whole     # ... which the whole-tensor ratio does not see at all
    assert R.degree_errors(ref.clone(), ref)[0] == 0.0
    worse = ref.clone()
    worse[0, 0, 3, 5] += 1.0                 # m > l: outside the comparison
    assert R.degree_errors(worse, ref)[0] == 0.0


def test_case_list_takes_its_branches():
    cs = R.cases()
    assert len({c.id for c in cs}) == len(cs)
    by = {}
    for c in cs:
        by.setdefault(c.family, []).append(c)
    # strips: every row count 1 .. 96 once, 32 units of each strip count
    (s,) = by["strips"]
    assert [R.rows_of(s, l) for l in range(s.L)] == list(range(1, 97))
    assert R.expected_route(s) == (0, 128, (32, 32, 32), 1)
    # chunks: a second chunk of 1 .. 24 rows, a third chunk at row0 = 192, rows capped by Mm n
    c3, c5, cap = by["chunks"]
    assert max(R.rows_of(c3, l) for l in range(c3.L)) == 120 and R.expected_route(c3)[3] == 2
    assert max(R.rows_of(c5, l) for l in range(c5.L)) == 200 and R.expected_route(c5)[3] == 3
    assert max(R.rows_of(cap, l) for l in range(cap.L)) == 20 < cap.L * cap.n
    # column groups and loop trips: C / 32 = 4, 8, 12, 16 stages, every strip count, two chunks, ragged three-strip chunks
    assert [c.C for c in by["cols"]] == [128, 256, 384, 512]
    for c in by["cols"]:
        st, kspan, hist, most = R.expected_route(c)
        assert kspan == c.C and all(h > 0 for h in hist) and most == 2
        assert any(64 < R.rows_of(c, l) < 96 and R.rows_of(c, l) % 32 for l in range(c.L))
    assert sorted(c.L for c in by["xcd"]) == [1, 5, 8, 9]
    # groups: the skipping forms and the two that walk the zeros; native only where the kernel takes it
    spans = {(c.C, c.groups): R.expected_route(c)[1] for c in by["gdense"]}
    assert spans == {(256, 4): 128, (256, 2): 128, (512, 2): 256, (384, 2): 384, (384, 4): 384}
    assert all(R.native_ok(c.C, c.groups) and R.expected_route(c)[1] == max(c.C // c.groups, 128) for c in by["gnative"])
    assert not R.native_ok(384, 4) and not R.native_ok(384, 2) and not R.native_ok(256, 1) and not R.native_ok(256, 16)
    for fam in ("gdense", "gnative"):
        assert {(c.n, c.L, c.Mm) for c in by[fam]} == {R.T_SHAPE, R.SMALL_SHAPE}
    # range: the bound sits in one element, exactly, at the two ends
    for v, top in (("xmax2^-95", 2.0 ** -95), ("xmax2^115", 2.0 ** 115)):
        x, _ = R.inputs(R.Case("range", 3, 128, 24, 25, variant=v))
        a = x.abs().flatten()
        assert float(a.max()) == top and int((a == top).sum()) == 1 and float(a.sort().values[-2]) <= top / 4
    # no case is large: the fp64 truth of the largest takes about a second
    assert max(c.C * c.C * c.L // c.groups for c in cs) <= 25_000_000 // 2
