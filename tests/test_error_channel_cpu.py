"""The library's one error channel (ace_amd/csrc/errors.h, errors.cpp) without a GPU.  The library loads without a device and every
argument refusal below happens before the first HIP call: one refused call per family, read back through that family's getter and
through ``ace_last_error`` - the same bytes, the text the family has always reported; the channel is one string per thread for the
whole library; ``_lib.check`` maps the code to the exception through the family's getter, looked up on ``lib()`` at call time.
tests/emul/errors_emul.cpp compiles errors.cpp alone for the pointer and thread properties."""
import ctypes
import os
import shutil
import subprocess
import threading

import pytest

from ace_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = (ctypes.c_double * 16)()
FAMILIES = ("mask", "couple", "diag", "physics", "hpx", "ll", "ocean_phys", "ocean_derive", "ice_budget", "pixel_mlp", "disco")


def _getters(L):
    return [L.ace_last_error] + [getattr(L, f"ace_{f}_last_error") for f in FAMILIES]


# family -> (a call refused with ACE_ERR_INVALID on the host, the message it leaves)
REFUSALS = {
    None: (lambda L: L.ace_sht_tables_host(4, 8, 0, 0, b"nonsense", 2, ctypes.cast(_BUF, ctypes.c_void_p)), b"Unknown quadrature"),
    "mask": (lambda L: L.ace_mask_planes(*[None] * 6, 0, None, 1, 1, 4, None), b"ace_mask_planes: null argument"),
    "couple": (lambda L: L.ace_couple_ocean_to_atmosphere(*[None] * 5, 0, 0, 0, 1, 1, 4, None),
               b"ace_couple_ocean_to_atmosphere: null argument"),
    "diag": (lambda L: L.ace_diag_hist_window(*[None] * 10, 1, 7, 1, 1, 1, 4, None), b"ace_diag_hist_window: need an even n_bins"),
    "physics": (lambda L: L.ace_physics_create(None, None, None, None, None), b"null argument"),
    "hpx": (lambda L: L.ace_hpx_pad_table_host(0, 1, None, None), b"ace_hpx_pad_table_host: need 1 <= padding <= nside <= 4095"),
    "ll": (lambda L: L.ace_ll_pool2(None, None, 1, 2, 2, 2, 4, 1, 1, None, None), b"ace_ll_pool2: bad argument (H, W >= 2)"),
    "ocean_phys": (lambda L: L.ace_ocean_phys_create(None, None, None, None, None, None), b"null argument"),
    "ocean_derive": (lambda L: L.ace_ocean_derive_window(None, None), b"ace_ocean_derive_window: null argument"),
    "ice_budget": (lambda L: L.ace_ice_budget_apply(None, 1.0, 1, 1, 1, None, None), b"null fields"),
    "pixel_mlp": (lambda L: L.ace_pixel_mlp_forward(None, None, None, None, 1, 4, None), b"ace_pixel_mlp_forward: null handle"),
    "disco": (lambda L: L.ace_disco_forward(None, None, None, None, 1, None), b"ace_disco_forward: null handle"),
}


@pytest.mark.parametrize("family", list(REFUSALS), ids=lambda f: f or "sht")
def test_a_refusal_is_read_through_its_own_getter_and_through_ace_last_error(family):
    L = _lib.lib()
    call, text = REFUSALS[family]
    other = REFUSALS["couple" if family != "couple" else "diag"]
    assert other[0](L) == _lib.ACE_ERR_INVALID               # something else in the channel first
    assert call(L) == _lib.ACE_ERR_INVALID
    own = getattr(L, f"ace_{family}_last_error" if family else "ace_last_error")()
    assert own and own == L.ace_last_error()
    assert own.startswith(text), own


def test_every_getter_returns_the_latest_failure_of_the_thread():
    L = _lib.lib()
    for first, second in (("couple", "diag"), ("diag", None), (None, "ice_budget"), ("pixel_mlp", "hpx")):
        assert REFUSALS[first][0](L) == _lib.ACE_ERR_INVALID
        assert all(g().startswith(REFUSALS[first][1]) for g in _getters(L))
        assert REFUSALS[second][0](L) == _lib.ACE_ERR_INVALID
        got = {g() for g in _getters(L)}
        assert len(got) == 1 and got.pop().startswith(REFUSALS[second][1])


def test_a_failure_on_another_thread_leaves_this_threads_message():
    L = _lib.lib()
    assert REFUSALS["couple"][0](L) == _lib.ACE_ERR_INVALID
    before = [g() for g in _getters(L)]
    seen = {}

    def other():
        seen["rc"] = REFUSALS["diag"][0](L)
        seen["msg"] = [g() for g in _getters(L)]

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["rc"] == _lib.ACE_ERR_INVALID and all(m.startswith(REFUSALS["diag"][1]) for m in seen["msg"])
    assert [g() for g in _getters(L)] == before and before[0].startswith(REFUSALS["couple"][1])


def test_check_maps_the_code_and_reads_the_familys_getter():
    L = _lib.lib()
    _lib.check(_lib.ACE_OK, "couple")
    assert REFUSALS["couple"][0](L) == _lib.ACE_ERR_INVALID
    with pytest.raises(ValueError, match="^ace_couple_ocean_to_atmosphere: null argument"):
        _lib.check(-1, "couple")
    with pytest.raises(RuntimeError, match="^ace_couple_ocean_to_atmosphere: null argument"):
        _lib.check(-2, "couple")
    assert REFUSALS[None][0](L) == _lib.ACE_ERR_INVALID
    with pytest.raises(ValueError, match="Unknown quadrature"):
        _lib.check(-1)


def test_check_asks_only_for_the_familys_getter(monkeypatch):
    """an emulation standing in for ``lib()`` has its own family's getter and nothing else (tests/_fake_ice.py)"""
    class OnlyIce:
        def ace_ice_budget_last_error(self):
            return b"(emulated) null fields"

    fake = OnlyIce()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    with pytest.raises(ValueError, match=r"^\(emulated\) null fields$"):
        _lib.check(-1, "ice_budget")
    with pytest.raises(RuntimeError, match=r"^\(emulated\) null fields$"):
        _lib.check(-2, "ice_budget")
    with pytest.raises(AttributeError):
        _lib.check(-1)                       # ace_last_error is not what a family's call is read through


def test_errors_cpp_alone(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "errors_emul")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "emul", "errors_emul.cpp"),
                    os.path.join(ROOT, "ace_amd", "csrc", "errors.cpp")], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "error channel ok" in res.stdout and "FAILED" not in res.stdout, res.stdout + res.stderr
