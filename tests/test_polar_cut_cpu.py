"""The polar cut of the spherical transform on the CPU (ace_amd/csrc/strip_pack.h: derive_polar_cut; strip_fold.hip, fft.hip):
tests/emul/polar_cut_emul.cpp derives the cut from the packed fragments of the REAL Legendre tables and restates the kernels'
index formulas with it.

Grids: 24 x 48, 46 x 92, 45 x 90 and 23 x 48 (odd nlat) legendre-gauss, 180 x 360 for the three quadratures.  Asserted there: the cut
is prefix-shaped and monotone, every packed element inside it is zero (hi and lo, both packs), row r0(m) holds a live element, the
dead share at 180 x 360 legendre-gauss lies in [0.23, 0.26]; with the dead entries of X set to NaN the emulated forward and
inverse equal the emulation without the cut bit for bit, every live element written exactly once and no dead one at all.

The big form of the folded kernel (units of 12, 18, 24 k16-steps, the inverse falling through to 2 / 4 / 6 at high wavenumbers; no
dropped k16-steps, whole 128-column groups) runs the same assertions at 194 x 48, 360 x 720 and 385 x 720 legendre-gauss and 361 x 720
equiangular, 128 columns each; the dead shares of the three 720-wide grids lie within 0.01 of 0.2850, 0.2586 and 0.2860.  The whole
program takes about a minute on one core."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_polar_cut_tables_and_data_movement(tmp_path):
    exe = str(tmp_path / "polar_cut_emul")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "emul", "polar_cut_emul.cpp"),
                    os.path.join(ROOT, "ace_amd", "csrc", "tables.cpp")], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "polar cut ok" in res.stdout
    assert "FAIL" not in res.stdout
