"""Smoothed maps at the C-ABI boundary, without a device: the two numpy restatements of the rule
(tests/smooth_ref.py) agree bit for bit, the constants and the Python mirrors are the header's, the pixel centres
come out by the formula, bad arguments are refused before any handle is looked at, the result class derives what
it says, and the sampling error that the default floor of two pixels rests on is reproduced."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import smooth_ref as S
from tests.helpers import ROOT

NAMES = ("nb_sim_smooth_map", "nb_runner_smooth_map", "nb_smooth_centres")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_smooth_params) F(nb_smooth_params, width) F(nb_smooth_params, height) F(nb_smooth_params, flags)
    F(nb_smooth_params, reserved) F(nb_smooth_params, center) F(nb_smooth_params, velocity) F(nb_smooth_params, axis)
    F(nb_smooth_params, x_range) F(nb_smooth_params, y_range) F(nb_smooth_params, depth_range)
    F(nb_smooth_params, s_min) F(nb_smooth_params, s_max)
    S(nb_smooth_stats) F(nb_smooth_stats, step_num) F(nb_smooth_stats, n) F(nb_smooth_stats, nonfinite)
    F(nb_smooth_stats, bad_smoothing) F(nb_smooth_stats, skipped) F(nb_smooth_stats, deposited)
    F(nb_smooth_stats, raised) F(nb_smooth_stats, lowered) F(nb_smooth_stats, pairs) F(nb_smooth_stats, tile_entries)
    F(nb_smooth_stats, mass) F(nb_smooth_stats, deposited_mass) F(nb_smooth_stats, center) F(nb_smooth_stats, velocity)
    F(nb_smooth_stats, n_hat) F(nb_smooth_stats, e1) F(nb_smooth_stats, e2) F(nb_smooth_stats, s_min)
    F(nb_smooth_stats, s_max) F(nb_smooth_stats, width) F(nb_smooth_stats, height) F(nb_smooth_stats, flags)
    F(nb_smooth_stats, max_count)
    printf("NB_SMOOTH_CENTER_COM %u 0\n", NB_SMOOTH_CENTER_COM);
    printf("NB_SMOOTH_VELOCITY %u 0\n", NB_SMOOTH_VELOCITY);
    printf("NB_SMOOTH_MAX_ENTRIES %llu 0\n", (unsigned long long)NB_SMOOTH_MAX_ENTRIES);
    printf("NB_SMOOTH_K %a 0\n", NB_SMOOTH_K);
    return 0;
}
"""


def _state(n, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 10), np.float32)
    s[:, 0:3] = rng.uniform(-spread, spread, (n, 3))
    s[:, 3:6] = rng.normal(0.0, 0.7, (n, 3))
    s[:, 9] = rng.uniform(0.5, 2.0, n)
    return s, rng


def _same(a, b):
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), key
        else:
            assert x == y, key


CASES = [  # n, grid, extent, axis, s range, (s_min, s_max), depth
    (200, (37, 21), (-1.0, 1.0, -0.5, 0.5), (1.0, 2.0, 3.0), (0.01, 0.5), (0.05, 0.4), (-math.inf, math.inf)),
    (64, (8, 8), (-1.0, 1.0, -1.0, 1.0), (0.0, 0.0, 1.0), (0.1, 3.0), (0.3, 2.5), (-0.5, 0.25)),
    (150, (17, 33), (-0.3, 0.45, -0.6, 0.2), (0.0, 1.0, 0.0), (0.001, 0.2), (0.02, 0.1), (-math.inf, 0.5)),
    (1, (1, 1), (-1.0, 1.0, -1.0, 1.0), (0.0, 0.0, 1.0), (0.5, 2.0), (0.1, 5.0), (-math.inf, math.inf)),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_two_restatements_agree_bit_for_bit(case):
    """The per-body loop over a pruned window and the dense (body, pixel) product: equal counts, equal single
    terms, equal sums (both add in body order), equal stats -- on random states with non-finite bodies and with
    NaN, 0, negative and infinite smoothing lengths."""
    n, (W, H), extent, axis, (s0, s1), (s_min, s_max), depth = CASES[case]
    state, rng = _state(n, seed=case + 3)
    s = rng.uniform(s0, s1, n)
    if n >= 64:
        s[3], s[4], s[5], s[6], s[9] = np.nan, 0.0, np.inf, -1.0, np.nan
        state[7, 0], state[8, 4], state[9, 9] = np.nan, np.inf, -np.inf   # (body 9: non-finite wins over a NaN s)
        state[11, 0:3] = state[12, 0:3]                                     # coincident bodies
    kw = dict(s_min=s_min, s_max=s_max, axis=axis, center=(0.02, -0.01, 0.03), velocity=(1e-3, 0.0, -2e-3), depth=depth,
              keep=True)
    a, b = S.smooth64(state, s, W, H, extent, **kw), S.smooth64_dense(state, s, W, H, extent, **kw)
    _same(a, b)
    assert a["nonfinite"] + a["bad_smoothing"] + a["skipped"] + a["deposited"] == n
    assert a["pairs"] == int(a["reach"].sum()) and np.array_equal(a["counts"], a["reach"].sum(axis=0))
    assert np.array_equal(a["deposited_body"], a["reach"].any(axis=(1, 2)))
    if n >= 64:
        assert (a["nonfinite"], a["bad_smoothing"]) == (3, 1) and a["raised"] >= 2 and a["lowered"] >= 1
        assert a["deposited"] > 0 and a["skipped"] > 0 and 0.0 < a["deposited_mass"] < a["mass"]
        # a term is zero exactly where the body does not reach, and plane 0 is positive where it does
        assert np.all((a["terms"][:, 0] > 0.0) == a["reach"])


def test_the_restatement_by_hand():
    """One body of mass 2 on a pixel centre of a 4 x 4 grid of unit pixels, s = 1.5: the centre pixel at r2 = 0,
    its four neighbours at r2 = 1; the diagonal ones at r2 = 2 < 2.25 as well; nothing at distance 2."""
    state = np.zeros((1, 10), np.float32)
    state[0, 0:3], state[0, 5], state[0, 9] = (0.5, 0.5, 0.0), 3.0, 2.0
    r = S.smooth64(state, 1.5, 4, 4, (-2.0, 2.0, -2.0, 2.0), s_min=0.1, s_max=10.0, axis=(0.0, 0.0, 1.0))
    want = np.zeros((4, 4), np.uint32)
    want[1:4, 1:4] = 1
    assert np.array_equal(r["counts"], want) and (r["deposited"], r["pairs"], r["max_count"]) == (1, 9, 1)
    k = 3.0 / math.pi / 2.25
    assert r["planes"][0][2, 2] == pytest.approx(2.0 * k) and r["planes"][0][2, 1] == pytest.approx(2.0 * k * (1 - 1 / 2.25) ** 2)
    assert r["planes"][0][1, 1] == pytest.approx(2.0 * k * (1 - 2 / 2.25) ** 2)
    assert r["planes"][3][2, 2] == pytest.approx(2.0 * k * 3.0) and r["planes"][4][2, 2] == pytest.approx(2.0 * k * 9.0)
    # the strict comparison: with s = 1 the four neighbours sit at r2 == s2 exactly and drop out
    r = S.smooth64(state, 1.0, 4, 4, (-2.0, 2.0, -2.0, 2.0), s_min=0.1, s_max=10.0, axis=(0.0, 0.0, 1.0))
    assert r["pairs"] == 1 and r["counts"][2, 2] == 1


def test_entry_points_and_constants(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    for name in ("SmoothedMap", "SmoothStats", "smooth_centres", "SMOOTH_K", "SMOOTH_PLANES"):
        assert name in nb.__all__ and hasattr(nb, name)
    for cls in (nb.Simulator, nb.OfflineHeadless):
        assert hasattr(cls, "smoothed_map")
    assert nb.SMOOTH_K == _lib.NB_SMOOTH_K == S.K and S.K.hex() == "0x1.e8ec8a4aeacc4p-1"
    assert abs(S.K - 3.0 / math.pi) <= 2.0 ** -53 and _lib.NB_SMOOTH_MAX_ENTRIES == S.MAX_ENTRIES == 1 << 28
    assert nb.SMOOTH_PLANES == S.PLANES


def test_python_mirrors_match_the_c_layout(nb, tmp_path):
    from wgpu_n_body_amd import _lib
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    cc = os.environ.get("CC", "gcc")
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rows = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                check=True).stdout.splitlines()]
    info = {r[0]: r[1:] for r in rows}
    for T, size in ((_lib.nb_smooth_params, 152), (_lib.nb_smooth_stats, 248)):
        name = T.__name__
        assert [int(x) for x in info[name]] == [C.sizeof(T), C.alignment(T)] and C.sizeof(T) == size, name
        for f, _ in T._fields_:
            assert [int(x) for x in info[f"{name}.{f}"]] == [getattr(T, f).offset, getattr(T, f).size], (name, f)
        assert len(T._fields_) == sum(1 for k in info if k.startswith(name + "."))
    assert int(info["NB_SMOOTH_CENTER_COM"][0]) == _lib.NB_SMOOTH_CENTER_COM == _lib.NB_MAP_CENTER_COM
    assert int(info["NB_SMOOTH_VELOCITY"][0]) == _lib.NB_SMOOTH_VELOCITY == _lib.NB_MAP_VELOCITY
    assert int(info["NB_SMOOTH_MAX_ENTRIES"][0]) == _lib.NB_SMOOTH_MAX_ENTRIES
    assert float.fromhex(info["NB_SMOOTH_K"][0]) == S.K


def test_centres_against_the_formula(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for lo, hi, cells in ((-1.0, 1.0, 16), (-0.3, 0.45, 37), (0.1, 0.7, 1), (-5.0, 3.0, 4096), (1.0, 1.0 + 2.0 ** -40, 21)):
        e = nb.map_edges(lo, hi, cells)
        got = nb.smooth_centres(lo, hi, cells)
        assert got.tobytes() == (0.5 * (e[:-1] + e[1:])).tobytes() == S.centres(lo, hi, cells).tobytes()
        assert np.all(got > e[:-1]) and np.all(got < e[1:])
    out = (C.c_double * 4)()
    for lo, hi, cells in ((0.0, 1.0, 0), (0.0, 1.0, 4097), (1.0, 1.0, 4), (math.nan, 1.0, 4), (0.0, math.inf, 4),
                          (1.0, 1.0 + 4e-16, 16)):
        assert L.nb_smooth_centres(lo, hi, cells, out) == _lib.NB_ERR_INVALID and b"smooth_centres" in L.nb_last_error()
    assert L.nb_smooth_centres(0.0, 1.0, 4, None) == _lib.NB_ERR_INVALID
    with pytest.raises(nb.NBodyError):
        nb.smooth_centres(0.0, 1.0, 5000)


def good_params(_lib, **change):
    p = _lib.nb_smooth_params()
    p.width, p.height, p.flags, p.reserved = 16, 8, _lib.NB_SMOOTH_VELOCITY, 0
    p.s_min, p.s_max = 0.25, 2.0
    vals = dict(center=(0, 0, 0), velocity=(0, 0, 0), axis=(0, 1, 0), x_range=(-1, 1), y_range=(-2, 2),
                depth_range=(-math.inf, math.inf))
    for k, v in change.items():
        if k in vals:
            vals[k] = v
        else:
            setattr(p, k, v)
    for k, v in vals.items():
        for i, x in enumerate(v):
            getattr(p, k)[i] = x
    return p


def test_refusals_without_a_device(nb):
    """The parameters are checked before the handle is looked at: a fake handle is never dereferenced, the outputs
    are never written, and a null handle with good parameters is the one refusal that names the handle."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID
    nan, inf = math.nan, math.inf
    fake = C.c_void_p(1)
    s = np.full(4, 0.5)
    counts = np.full(16 * 8, 7, np.uint32)
    planes = np.full(6 * 16 * 8, 7.0)
    st = _lib.nb_smooth_stats()
    for call, who in ((L.nb_sim_smooth_map, b"simulator"), (L.nb_runner_smooth_map, b"runner")):
        def bad(word, p, handle=fake, lengths=s):
            rc = call(handle, C.byref(p) if p is not None else None, lengths.ctypes.data if lengths is not None else None,
                      counts.ctypes.data, planes.ctypes.data, C.byref(st))
            assert rc == INV and word in L.nb_last_error(), (word, rc, L.nb_last_error())
            assert np.all(counts == 7) and np.all(planes == 7.0) and bytes(st) == bytes(C.sizeof(st))

        for s_min, s_max in ((0.0, 1.0), (-1.0, 1.0), (nan, 1.0), (0.5, nan), (0.5, inf), (inf, inf), (2.0, 1.0),
                             (-2.0, -1.0)):
            bad(b"s_min", good_params(_lib, s_min=s_min, s_max=s_max))
        bad(b"flag", good_params(_lib, flags=4))
        bad(b"flag", good_params(_lib, flags=3 | 8))
        bad(b"reserved", good_params(_lib, reserved=1))
        for w, h in ((0, 8), (8, 0), (4097, 1), (1, 4097)):
            bad(b"side", good_params(_lib, width=w, height=h))
        bad(b"cells", good_params(_lib, width=4096, height=2048))
        bad(b"params", None)
        for axis in ((0, 0, 0), (nan, 1, 0)):
            bad(b"axis", good_params(_lib, axis=axis))
        bad(b"center", good_params(_lib, center=(0, nan, 0)))
        bad(b"x_range", good_params(_lib, x_range=(1, 1)))
        bad(b"y_range", good_params(_lib, y_range=(0, inf)))
        bad(b"depth", good_params(_lib, depth_range=(nan, 1)))
        assert L.nb_last_error().startswith(b"smooth_map: ")  # in the pass's own words
        # good parameters: the handle is the fault, with or without s (a null s is refused for n > 0, behind it)
        bad(b"null " + who, good_params(_lib), handle=None)
        bad(b"null " + who, good_params(_lib, s_min=0.5, s_max=0.5), handle=None, lengths=None)
        bad(b"null " + who, good_params(_lib, flags=_lib.NB_SMOOTH_CENTER_COM, center=(nan, nan, nan)), handle=None)


def test_result_class(nb):
    planes = np.zeros((6, 2, 3))
    planes[0] = [[2.0, 0.0, 4.0], [1.0, 1.0, 0.0]]
    planes[3] = [[4.0, 0.0, -4.0], [0.5, 0.0, 0.0]]
    planes[4] = [[10.0, 0.0, 8.0], [0.25, 0.0, 0.0]]
    stats = nb.SmoothStats(3, 10, 1, 1, 2, 6, 1, 1, 12, 40, 9.0, 6.0, np.zeros(3), np.zeros(3), np.zeros(3),
                           np.zeros(3), np.zeros(3), 0.1, 1.0, 3, 4)
    m = nb.SmoothedMap(np.ones((2, 3), np.uint32), planes, np.arange(3.0), np.arange(2.0), np.ones(10), stats)
    assert np.shares_memory(m.surface_density, planes[0]) and np.array_equal(m.surface_density, planes[0])
    empty = planes[0] == 0.0
    assert np.array_equal(np.isnan(m.mean_w), empty) and np.array_equal(np.isnan(m.sigma_w), empty)
    assert m.mean_w[0, 0] == 2.0 and m.mean_w[0, 2] == -1.0 and m.mean_w[1, 1] == 0.0
    assert m.sigma_w[0, 0] == 1.0 and m.sigma_w[0, 2] == 1.0
    assert m.sigma_w[1, 0] == 0.0          # 0.25 - 0.25
    s = m.stats
    assert s.nonfinite + s.bad_smoothing + s.skipped + s.deposited == s.n
    mass_only = nb.SmoothedMap(m.counts, planes[:1], m.x_centres, m.y_centres, m.smoothing, stats)
    assert mass_only.surface_density is not None
    with pytest.raises(ValueError):
        mass_only.mean_w
    with pytest.raises(ValueError):
        mass_only.sigma_w


def test_sampling_error_behind_the_default_floor():
    """The kernel is point-sampled at the pixel centres.  Over 400 random sub-pixel offsets of the body the sum of
    wgt times the pixel area stays within the figures of DESIGN.md 6j, which fall with s_eff in pixels: two pixels
    is the first length at which the error is of the order of a per cent.  Below half a pixel diagonal a body at
    a pixel corner misses every centre."""
    offsets = np.random.default_rng(0).uniform(0.0, 1.0, (400, 2))
    bounds = {1: (-0.045, 0.074), 2: (-0.007, 0.015), 4: (-0.002, 0.002), 8: (-0.0002, 0.0002)}
    for s_pixels, (lo, hi) in bounds.items():
        err = S.sampled_integral(float(s_pixels), offsets) - 1.0
        print(f"s_eff {s_pixels} pixels: {100 * err.min():+.3f} % .. {100 * err.max():+.3f} %")
        assert 1.02 * lo <= err.min() and err.max() <= 1.02 * hi, (s_pixels, err.min(), err.max())  # (two-digit figures)
        assert err.min() < 0.0 < err.max()
        if s_pixels <= 2:  # the quoted figures are the extremes, not loose bounds
            assert err.min() <= 0.9 * lo and err.max() >= 0.9 * hi
    assert S.sampled_integral(0.70, [[0.0, 0.0]])[0] == 0.0 < S.sampled_integral(0.71, [[0.0, 0.0]])[0]
