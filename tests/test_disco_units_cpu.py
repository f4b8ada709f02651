"""The plan of an ``ace_disco_forward`` launch (ace_amd/csrc/disco_units.h) on the CPU: tests/emul/disco_units_emul.cpp compiles the
header the kernel's ``create`` runs and checks, on every grid and channel case of tests/_disco_cases.py and on 180 x 360 with
40 -> 256 channels, that every (ho, wo, o) is produced by exactly one unit, that costs are non-increasing along the list, that
every LDS address the kernel forms lies in the unit's stage and holds the input element the statement names, that stage and z fit
their budgets - and that what the limits exclude is refused by name."""
import math
import os
import shutil
import subprocess

import pytest

import _disco_cases as C
from ace_amd.disco import disco_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    out = str(tmp_path_factory.mktemp("disco_units") / "disco_units_emul")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "emul", "disco_units_emul.cpp")], check=True)
    return out


def _write_table(path, grid):
    H, W, ks = grid
    t = disco_table((H, W), ks)
    with open(path, "w") as f:
        f.write(f"{H} {W} {ks * ks} {len(t.hi)}\n")
        for a in (t.row_offsets, t.hi, t.wi):
            f.write(" ".join(str(int(v)) for v in a) + "\n")


@pytest.mark.parametrize("grid", C.GRIDS + [(180, 360, 3)], ids=lambda g: f"{g[0]}x{g[1]}k{g[2]}")
def test_every_output_in_exactly_one_unit(exe, tmp_path, grid):
    chans = [c for g, c in C.CASES if g == grid] or [(40, 256), (40, 40), (7, 256)]
    path = str(tmp_path / "table.txt")
    _write_table(path, grid)
    args = [str(v) for cin, cout in chans for v in (cin, cout, math.gcd(cin, cout))]
    res = subprocess.run([exe, path] + args, capture_output=True, text=True, timeout=600)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.count("units ok") == len(chans) and "FAILED" not in res.stdout


def test_limits_are_refused(exe):
    res = subprocess.run([exe, "refuse"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "refusals ok" in res.stdout, res.stdout + res.stderr
