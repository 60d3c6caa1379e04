"""nb_sim_diagnostics / nb_runner_diagnostics at the C-ABI boundary, without a device: the entry
points are exported, the Python mirror of nb_diagnostics has the C layout, bad arguments are
refused before any device is touched, and the tests' own fp64 psi (tests/diag_ref.py) is the
integral it claims to be."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.diag_ref import psi64
from tests.helpers import ROOT

FIELDS = ["step_num", "n", "nonfinite", "mass", "com", "momentum", "angular_momentum", "kinetic",
          "max_speed", "pair_sum", "potential", "total", "flags", "reserved"]

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(x) printf("%s %zu %zu\n", #x, offsetof(nb_diagnostics, x), sizeof(((nb_diagnostics *)0)->x));
int main(void) {
    printf("sizeof %zu %zu\n", sizeof(nb_diagnostics), _Alignof(nb_diagnostics));
    F(step_num) F(n) F(nonfinite) F(mass) F(com) F(momentum) F(angular_momentum) F(kinetic)
    F(max_speed) F(pair_sum) F(potential) F(total) F(flags) F(reserved)
    printf("NB_DIAG %u %u\n", NB_DIAG_MOMENTS, NB_DIAG_POTENTIAL);
    return 0;
}
"""


def test_diagnostics_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in ("nb_sim_diagnostics", "nb_runner_diagnostics"):
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS


def test_python_mirror_matches_the_c_layout(nb, tmp_path):
    from wgpu_n_body_amd import _lib
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    cc = os.environ.get("CC", "gcc")
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rows = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                check=True).stdout.splitlines()]
    info = {r[0]: (int(r[1]), int(r[2])) for r in rows}
    S = _lib.nb_diagnostics
    assert info["sizeof"][0] == C.sizeof(S) == 152
    assert info["sizeof"][1] == C.alignment(S)
    assert [f for f, _ in S._fields_] == FIELDS
    for f in FIELDS:
        assert info[f] == (getattr(S, f).offset, getattr(S, f).size), f
    assert info["NB_DIAG"] == (_lib.NB_DIAG_MOMENTS, _lib.NB_DIAG_POTENTIAL)


def test_bad_arguments_are_invalid_without_a_device(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    d = _lib.nb_diagnostics()
    assert L.nb_sim_diagnostics(None, 1, C.byref(d)) == _lib.NB_ERR_INVALID
    assert L.nb_sim_diagnostics(None, 3, None) == _lib.NB_ERR_INVALID
    assert L.nb_sim_diagnostics(None, 4, C.byref(d)) == _lib.NB_ERR_INVALID
    assert b"unknown flag" in L.nb_last_error()
    assert L.nb_sim_diagnostics(None, 0x80000001, C.byref(d)) == _lib.NB_ERR_INVALID
    assert L.nb_runner_diagnostics(None, 1, C.byref(d)) == _lib.NB_ERR_INVALID
    assert L.nb_last_error() == b"null runner"
    # the arguments are looked at before the handle, as in every other pass
    assert L.nb_runner_diagnostics(None, 8, C.byref(d)) == _lib.NB_ERR_INVALID
    assert L.nb_last_error() == b"diagnostics: unknown flag bits 0x8"
    assert L.nb_runner_diagnostics(None, 3, None) == _lib.NB_ERR_INVALID
    assert L.nb_last_error() == b"diagnostics: out is null"
    # nothing was written
    assert bytes(d) == bytes(C.sizeof(d))


def test_diagnostics_dataclass_is_frozen(nb):
    import dataclasses
    assert dataclasses.is_dataclass(nb.Diagnostics)
    assert nb.Diagnostics.__dataclass_params__.frozen
    assert "Diagnostics" in nb.__all__


def _quad_psi(r, e):
    """integral_r^inf ds / (s^3 + e) by composite Gauss-Legendre on s = r + t / (1 - t), t in [0, 1)."""
    t, w = np.polynomial.legendre.leggauss(64)
    edges = np.concatenate([np.linspace(0.0, 0.9, 91), 1.0 - np.geomspace(0.1, 1e-12, 120)])
    total = 0.0
    for a, b in zip(edges[:-1], edges[1:]):
        tt = 0.5 * (b - a) * t + 0.5 * (b + a)
        s = r + tt / (1.0 - tt)
        total += 0.5 * (b - a) * np.sum(w / (s ** 3 + e) / (1.0 - tt) ** 2)
    # the tail t > 1 - 1e-12 (s > 1e12): integral ~ 1 / (2 s^2)
    s_end = r + (1.0 - 1e-12) / 1e-12
    return total + 0.5 / s_end ** 2


@pytest.mark.parametrize("r", [0.0, 0.01, np.cbrt(1e-4), 0.1, 0.5, 2.0, 0.0928, 0.0929])
def test_host_psi_matches_quadrature(r):
    e = 1e-4
    got = psi64(np.array([r]), e)[0]
    ref = _quad_psi(r, e)
    assert abs(got / ref - 1.0) < 1e-10, (r, got, ref)


def test_host_psi_limits():
    e = 1e-4
    a = np.cbrt(e)
    assert abs(psi64(np.array([0.0]), e)[0] / (2 * np.pi / (3 * np.sqrt(3) * a * a)) - 1) < 1e-14
    r = np.array([10.0, 100.0])
    assert np.allclose(psi64(r, e), 0.5 / r ** 2, rtol=1e-6)
    assert np.isinf(psi64(np.array([0.0]), 0.0)[0])
