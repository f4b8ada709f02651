"""csrc/ocean_phys.hip (ocean_o1, ocean_o2 through OceanCorrector's fused path) against the fp64 truth of tests/_ocean_phys_ref.py
at every shape the kernels branch on: planes smaller than a wave, ragged tails in the last wave and the last workgroup, an odd row
length under the ``px / W`` weight lookup, many workgroups per sample (the [q][NBLK_MAX] partials and their b * NQ * NBLK_MAX
offset at b > 0), more than 256 workgroups (second trip of O2's re-sum), the NBLK_MAX cap with the grid-stride loop in O1 and O2,
and 1, 2, 4, 8 and 64 levels - with every flux source and field switch of O1 at each of them.

Bar, per changed field: max|got - ref64| / max|ref64| over the non-NaN points <= max(2e-6, 3 * floor), ``floor`` the restatement's
own fp32-to-fp64 distance on the same inputs (capped on the CPU: test_ocean_phys_ref_cpu.test_floor_cap, which also shows in fp64
that a lost partial sum, a lost grid-stride tail and another sample's means each pass this bar many times over).  NaN patterns
equal the truth's.  Fields the truth leaves alone, the step's input, the forcing and the other steps of the output window come
back bitwise; the outputs are corrected in place; a repeat of the run gives the same bits.  Each test prints its largest error as
a fraction of its bar (OCEANACC)."""
import pytest
import torch

import _ocean_phys_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_against(t, gen, c, tag, samples=None):
    """every changed field within its bar and with the truth's NaN pattern, every other field bitwise; the worst err / tol"""
    worst = (0.0, "-")
    for k, v in c["gen"].items():
        got = gen[k].cpu()
        if k not in t["fields"]:
            assert torch.equal(_bits(got), _bits(v)), (tag, k, "a field the truth leaves alone was written")
            continue
        want = t["fields"][k]
        if samples is not None:
            got, want = got[samples], want[samples]
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (tag, k, "NaN pattern")
        err, tol = R.rel_err(got, want), R.tolerance(t["floor"][k])
        worst = max(worst, (err / tol, f"{k} err {err:.3e} tol {tol:.3e}"))
        assert err <= tol, (tag, k, err, tol)
    return worst


def _bystanders_untouched(whole, c, T=2):
    for n, v in c["input"].items():
        assert torch.equal(_bits(whole["input"][n][:, 0].cpu()), _bits(v)), (n, "the step's input was written")
    for n, v in c["forcing"].items():
        for s in range(T + 1):
            assert torch.equal(whole["forcing"][n][:, s].cpu(), v if s == T else v + 1.0 + s), (n, s, "the forcing was written")
    for n, v in c["gen"].items():
        for s in range(T - 1):
            assert torch.equal(whole["gen"][n][:, s].cpu(), v + 1.0 + s), (n, s, "another step of the output window was written")


def _run(dev, c, budget):
    corrector = R.fused_corrector(c)
    inp, gen, forcing, whole = R.ocean_buffers(dev, c)
    B, H, W = next(iter(gen.values())).shape
    where = {n: (v.data_ptr(), v.stride()) for n, v in gen.items()}
    out, state = corrector(inp, gen, forcing)
    torch.cuda.synchronize()
    assert state is None and corrector.launches() == (1, int(budget))
    for n, v in out.items():               # in place, on the strided step views
        assert (v.data_ptr(), v.stride()) == where[n] and v.stride() == (2 * H * W, W, 1), n
    return corrector, inp, gen, forcing, whole


@pytest.mark.parametrize("shape,name", R.shape_variant_grid(), ids=lambda v: R.shape_id(v) if isinstance(v, tuple) else v)
def test_corrector_vs_fp64(dev, shape, name):
    c = R.case(*shape, name)
    t = R.truth_for(shape, name)
    budget = name != "column_local"
    corrector, inp, gen, forcing, whole = _run(dev, c, budget)
    worst = _check_against(t, gen, c, (shape, name))
    print(f"OCEANACC {R.shape_id(shape)} {name}: worst err/tol {worst[0]:.3f} ({worst[1]})")
    _bystanders_untouched(whole, c)
    # fixed-order reductions: the same step again gives the same bits
    first = {k: v.clone() for k, v in gen.items()}
    for n, v in c["gen"].items():
        gen[n].copy_(v.to(dev))
    corrector(inp, gen, forcing)
    torch.cuda.synchronize()
    assert corrector.launches() == (2, 2 * int(budget))
    for k in gen:
        assert torch.equal(_bits(gen[k]), _bits(first[k])), (k, "a repeat gave other bits")


def test_partials_are_isolated_per_sample(dev):
    """A NaN in the net flux of ONE ocean column of sample 1 (its geothermal flux), at a non-zero heat-content weight: truth and
    kernel give all-NaN thetao and sst for sample 1 only, and samples 0 and 2 stay within the bar - no partial of sample 1 reaches
    another sample's sums.  (The depth mask is shared by the samples, so a masked top level under a non-zero weight - the second
    half - poisons every sample, in the truth and in the kernel alike.)"""
    shape, name = (3, 9, 57, 4), "gen_total_area"
    base = R.case(*shape, name)
    wet = (base["mask"][..., 0] > 0).nonzero()
    i, j = (int(x) for x in wet[len(wet) // 2])
    hfgeou = base["forcing"]["hfgeou"].clone()
    hfgeou[1, i, j] = float("nan")
    c = {**base, "forcing": {**base["forcing"], "hfgeou": hfgeou}}
    t = R.truth(c["config"], c)
    th = [f"thetao_{k}" for k in range(4)] + ["sst"]
    for k in th:
        assert torch.isnan(t["fields"][k][1]).all() and not torch.isnan(t["fields"][k][[0, 2]]).any()
        assert torch.equal(t["fields"][k][[0, 2]], R.truth_for(shape, name)["fields"][k][[0, 2]])
    _, _, gen, _, _ = _run(dev, c, True)
    worst = _check_against(t, gen, c, "nan in sample 1")
    for k in th:
        assert torch.isnan(gen[k][1]).all()
    print(f"OCEANACC isolated samples {R.shape_id(shape)} {name}: worst err/tol {worst[0]:.3f} ({worst[1]})")
    # a land column (masked top level) given a heat-content weight
    dry = (base["mask"][..., 0] == 0).nonzero()
    i, j = (int(x) for x in dry[len(dry) // 2])
    m = base["masks"]["mask_ocean_heat_content"].clone()
    m[i, j] = 1.0
    c = {**base, "masks": {"mask_ocean_heat_content": m}}
    t = R.truth(c["config"], c)
    _, _, gen, _, _ = _run(dev, c, True)
    _check_against(t, gen, c, "masked top level")
    for k in th:
        assert torch.isnan(t["fields"][k]).all() and torch.isnan(gen[k]).all()


def test_one_field_more_than_the_kernel_takes_is_refused(dev):
    shape, name = (2, 5, 13, 2), "column_local"
    base = R.case(*shape, name)
    cfg = base["config"]
    sic = cfg["sea_ice_fraction_correction"]
    assert len(cfg["force_positive_names"]) == R.MAX_POSITIVE and len(sic["zero_where_ice_free_names"]) == R.MAX_ZERO
    more = [{**cfg, "force_positive_names": cfg["force_positive_names"] + [f"tracer_{R.MAX_POSITIVE - 1}"]},
            {**cfg, "sea_ice_fraction_correction": {**sic, "zero_where_ice_free_names": sic["zero_where_ice_free_names"]
                                                    + [f"icevar_{R.MAX_ZERO - 1}"]}}]
    for config in more:
        c = {**base, "config": config}
        corrector = R.fused_corrector(c)
        inp, gen, forcing, _ = R.ocean_buffers(dev, c)
        with pytest.raises(NotImplementedError, match="fused ocean corrector"):
            corrector(inp, gen, forcing)
        assert corrector.launches() == (0, 0)
        for n, v in c["gen"].items():
            assert torch.equal(gen[n].cpu(), v), n
