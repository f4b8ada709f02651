"""csrc/physics.hip (phys_p1 .. phys_p4 through FusedPhysics) against the fp64 truth of tests/_physics_ref.py at every shape the
kernels branch on: planes smaller than a wave, ragged tails in the last wave and the last workgroup, an odd row length under the
``px / W`` weight lookup, many workgroups per sample (the [q][NBLK_MAX] partials and their (pass * max_batch + b) * NQ offset at
b > 0), more than 256 workgroups (second trip of block_load_sums), the NBLK_MAX cap with the grid-stride loop, and 1, 2, 4, 8 and
16 layers.  The golden 8 x 16 x 4 case of test_gpu_parity.py is one workgroup with two live waves.

Bar, per changed field and step: max|got - ref64| / max|ref64| <= max(2e-6, 3 * floor), 2e-6 being what
test_fused_physics_vs_reference_corrector holds and ``floor`` the restatement's own fp32-to-fp64 distance on the same inputs
(capped on the CPU: test_physics_ref_cpu.test_floor_cap).  Fields the truth leaves alone, the step's inputs and the forcing come
back bitwise; a repeat of the run gives the same bits.  Each test prints its largest error as a fraction of its bar (PHYSACC)."""
import pytest
import torch

import _physics_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _stream():
    from ace_amd import _lib
    return _lib.current_stream()


def _run_steps(phys, out, c, steps, dev):
    for s in range(steps):
        for n, v in c[f"gen{s}"].items():
            out[n][:, s].copy_(v.to(dev))
        phys.apply(s, _stream())
    torch.cuda.synchronize()


def _check_against(t, out, c, steps, tag):
    """every changed field within its bar, every other field bitwise; returns the worst err / tol"""
    worst = (0.0, "-")
    for s in range(steps):
        ref, floor = t["fields"][s], t["floor"][s]
        for k, v in c[f"gen{s}"].items():
            got = out[k][:, s].cpu()
            if k not in ref:
                assert torch.equal(got, v), (tag, s, k, "a field the truth leaves alone was written")
                continue
            want = ref[k]
            err = float((got.double() - want).abs().max()) / float(want.abs().max())
            tol = R.tolerance(floor[k])
            worst = max(worst, (err / tol, f"step {s} {k} err {err:.3e} tol {tol:.3e}"))
            assert err <= tol, (tag, s, k, err, tol)
    return worst


def _inputs_untouched(keep, c, T):
    ic, forcing = keep
    for n, v in ic.items():
        assert torch.equal(v[:, 0].cpu(), c["input0"][n]), (n, "the initial condition was written")
    for n, v in forcing.items():
        for s in range(T + 1):
            assert torch.equal(v[:, s].cpu(), c["forcing"][n]), (n, "the forcing was written")


@pytest.mark.parametrize("shape,name", R.shape_config_grid(), ids=lambda v: R.shape_id(v) if isinstance(v, tuple) else v)
def test_two_steps_vs_fp64(dev, shape, name):
    """Two chained steps (the dry-air reference seeded on the first and carried to the second; step 1 reads step 0's output in
    place) of every corrector configuration at the small shapes, and of the four that between them write every reduction slot of
    every pass at the large ones."""
    c = R.case(*shape)
    t = R.truth_for(shape, name)
    phys, out, keep = R.physics_buffers(dev, c, R.config_for(name, shape[3]))
    phys.reset(_stream())
    _run_steps(phys, out, c, 2, dev)
    worst = _check_against(t, out, c, 2, (shape, name))
    print(f"PHYSACC two_steps {R.shape_id(shape)} {name}: worst err/tol {worst[0]:.3f} ({worst[1]})")
    _inputs_untouched(keep, c, 2)
    mass = phys.get_reference(_stream())
    if t["mass"] is None:
        assert mass is None
    else:
        torch.testing.assert_close(mass.cpu().reshape(-1), t["mass"].reshape(-1), rtol=1e-6, atol=0.0)
    # fixed-order reductions: the same two steps again give the same bits, now with many workgroups
    first = {k: v.clone() for k, v in out.items()}
    phys.reset(_stream())
    _run_steps(phys, out, c, 2, dev)
    assert all(torch.equal(out[k], first[k]) for k in out)
    mass2 = phys.get_reference(_stream())
    assert (mass is None and mass2 is None) or torch.equal(mass, mass2)


@pytest.mark.parametrize("shape", R.VARIANT_SHAPES, ids=R.shape_id)
def test_frozen_parts_and_geopotential(dev, shape):
    """ace2_like on data that carries the frozen precipitation as ICEsfc + GRAUPELsfc + SNOWsfc (no
    total_frozen_precipitation_rate, so the clip has no target) and the surface height as PHIS: the kernel's ``frozen_parts`` sum
    and its 1 / 9.80616 height scale."""
    c = R.case(*shape, frozen="parts", height="PHIS")
    assert "total_frozen_precipitation_rate" not in c["gen0"] and "HGTsfc" not in c["input0"]
    t = R.truth_for(shape, "ace2_like", "parts", "PHIS")
    assert not {"ICEsfc", "GRAUPELsfc", "SNOWsfc", "PHIS"} & set(t["fields"][0])
    phys, out, keep = R.physics_buffers(dev, c, R.config_for("ace2_like", shape[3]))
    phys.reset(_stream())
    _run_steps(phys, out, c, 2, dev)
    worst = _check_against(t, out, c, 2, (shape, "parts/PHIS"))       # the three components come back bitwise (unchanged fields)
    print(f"PHYSACC frozen_parts_phis {R.shape_id(shape)} ace2_like: worst err/tol {worst[0]:.3f} ({worst[1]})")
    _inputs_untouched(keep, c, 2)                                     # PHIS among them
    torch.testing.assert_close(phys.get_reference(_stream()).cpu().reshape(-1), t["mass"].reshape(-1), rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("shape", R.VARIANT_SHAPES, ids=R.shape_id)
def test_carried_dry_air_reference(dev, shape):
    """ace_physics_set_reference: a dry-air mass carried in from a previous window - not the input's own, each sample's a
    different one - is what the first step closes to."""
    c = R.case(*shape)
    cfg = R.config_for("ace2_like", shape[3])
    own = R.truth_for(shape, "ace2_like")["mass"].reshape(-1)
    mass = own * (1.0 + 1e-4 * torch.arange(1, shape[0] + 1, dtype=torch.float64))
    t = R.truth(cfg, c, steps=1, mass=mass)
    assert "PRESsfc" in t["fields"][0] and torch.equal(t["mass"].reshape(-1), mass)
    phys, out, keep = R.physics_buffers(dev, c, cfg)                  # a fresh handle: nothing seeded
    assert phys.get_reference(_stream()) is None
    phys.set_reference(mass.to(dev), _stream())
    _run_steps(phys, out, c, 1, dev)
    worst = _check_against(t, out, c, 1, (shape, "carried"))
    print(f"PHYSACC carried_reference {R.shape_id(shape)} ace2_like: worst err/tol {worst[0]:.3f} ({worst[1]})")
    assert torch.equal(phys.get_reference(_stream()).cpu().reshape(-1), mass)


@pytest.mark.parametrize("interpolate", [False, True])
@pytest.mark.parametrize("shape", [(2, 9, 57), (2, 182, 721)], ids=lambda s: "B%d-%dx%d" % s)
def test_ocean_and_prescribed_at_multi_block_shapes(dev, shape, interpolate):
    """Prescribed SST (a select on the half-to-even rounded mask, or one lerp with contraction off) and a prescribed prognostic,
    without a corrector: bitwise against ace_amd.ocean's torch result in fp32."""
    from ace_amd.ocean import OceanConfig
    from ace_amd.physics import FusedPhysics
    B, H, W = shape
    HW = H * W
    g = torch.Generator().manual_seed(7)
    frac = torch.rand(B, H, W, generator=g)
    frac[0, :2] = 0.5          # ties: torch.round is half-to-even
    frac[1, :2] = 1.5
    gen = {"sst": torch.randn(B, H, W, generator=g) + 288.0, "q": torch.randn(B, H, W, generator=g)}
    target = {"sst": torch.randn(B, H, W, generator=g) + 285.0, "frac": frac}
    ocean = OceanConfig(surface_temperature_name="sst", ocean_fraction_name="frac", interpolate=interpolate).build(
        ["sst", "frac", "q"], ["sst", "q"])
    want = ocean({"sst": gen["sst"] + 2.0}, gen, target)
    assert set(want) == {"sst", "q"} and torch.equal(want["q"], gen["q"])
    out = {k: v.reshape(B, 1, H, W).to(dev).contiguous().clone() for k, v in gen.items()}
    nxt = {k: torch.stack([v - 3.0, v], dim=1).to(dev).contiguous() for k, v in target.items()}      # step s + 1's data is read
    nxt["q"] = torch.stack([gen["q"] - 2.0, gen["q"] + 1.0], dim=1).to(dev).contiguous()
    before = {k: v.clone() for k, v in nxt.items()}
    phys = FusedPhysics(None, ocean, ["q"], B, (H, W), 1, gen_names=list(out), in_names=list(out),
                        next_names=list(nxt), locate_gen=lambda n, s: (out[n].data_ptr(), HW) if n in out else None,
                        locate_in=lambda n, s: None,
                        locate_next=lambda n, s: (nxt[n].data_ptr() + 4 * HW, 2 * HW) if n in nxt else None, device=dev)
    phys.apply(0, _stream())
    torch.cuda.synchronize()
    assert torch.equal(out["sst"][:, 0].cpu(), want["sst"])
    assert torch.equal(out["q"][:, 0].cpu(), gen["q"] + 1.0)
    assert all(torch.equal(nxt[k], before[k]) for k in nxt)
