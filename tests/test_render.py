"""The renderer at the C-ABI boundary, without a device: the entry points are exported, the Python
mirrors have the C layout, the camera is the reference's, bad arguments are refused before any
device is touched, and the tests' own restatement of the drawing rule (tests/render_ref.py) gives
the answers that can be worked out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import render_ref as R
from tests.helpers import ROOT, make_state

NAMES = ("nb_camera_default", "nb_camera_view_proj", "nb_render_params_default", "nb_sim_render", "nb_runner_render")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_camera) F(nb_camera, eye) F(nb_camera, target) F(nb_camera, up) F(nb_camera, aspect)
    F(nb_camera, fovy_deg) F(nb_camera, znear) F(nb_camera, zfar)
    S(nb_render_params) F(nb_render_params, width) F(nb_render_params, height) F(nb_render_params, view_proj)
    F(nb_render_params, half_size) F(nb_render_params, clear) F(nb_render_params, alpha)
    F(nb_render_params, flags) F(nb_render_params, reserved)
    S(nb_render_stats) F(nb_render_stats, step_num) F(nb_render_stats, n) F(nb_render_stats, drawn)
    F(nb_render_stats, clipped) F(nb_render_stats, oversize) F(nb_render_stats, nonfinite)
    F(nb_render_stats, fragments) F(nb_render_stats, max_count) F(nb_render_stats, reserved)
    printf("NB_RENDER_SRGB %u 0\n", NB_RENDER_SRGB);
    return 0;
}
"""


def test_render_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    for name in ("Camera", "RenderParams", "RenderStats", "write_ppm"):
        assert name in nb.__all__ and hasattr(nb, name)
    assert hasattr(nb.Simulator, "render") and hasattr(nb.OfflineHeadless, "render")


def test_python_mirrors_match_the_c_layout(nb, tmp_path):
    from wgpu_n_body_amd import _lib
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    cc = os.environ.get("CC", "gcc")
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rows = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                check=True).stdout.splitlines()]
    info = {r[0]: (int(r[1]), int(r[2])) for r in rows}
    for S, size in ((_lib.nb_camera, 52), (_lib.nb_render_params, 100), (_lib.nb_render_stats, 64)):
        name = S.__name__
        assert info[name] == (C.sizeof(S), C.alignment(S)) and C.sizeof(S) == size, name
        for f, _ in S._fields_:
            assert info[f"{name}.{f}"] == (getattr(S, f).offset, getattr(S, f).size), (name, f)
        assert len(S._fields_) == sum(1 for k in info if k.startswith(name + "."))
    assert info["NB_RENDER_SRGB"][0] == _lib.NB_RENDER_SRGB


def test_default_camera_holds_the_reference_numbers(nb):
    from wgpu_n_body_amd import _lib
    c = _lib.nb_camera()
    assert _lib.lib().nb_camera_default(C.byref(c), 1280, 720) == 0
    # online_renderer.rs:231-239
    assert tuple(c.eye) == (0.0, 1.0, 2.0) and tuple(c.target) == (0.0, 0.0, 0.0) and tuple(c.up) == (0.0, 1.0, 0.0)
    assert np.float32(c.aspect) == np.float32(1280) / np.float32(720)
    assert c.fovy_deg == 45.0 and np.float32(c.znear) == np.float32(0.00001) and c.zfar == 100.0
    p = _lib.nb_render_params()
    assert _lib.lib().nb_render_params_default(C.byref(p), 1280, 720) == 0
    assert (p.width, p.height, p.flags, p.reserved) == (1280, 720, _lib.NB_RENDER_SRGB, 0)
    assert np.float32(p.half_size) == np.float32(0.006) and np.float32(p.alpha) == np.float32(0.25)
    assert [np.float32(v) for v in p.clear] == [np.float32(0.01), np.float32(0.0), np.float32(0.05)]
    assert np.array_equal(np.array(list(p.view_proj), np.float32), nb.Camera.default(1280, 720).view_proj())


CAMERAS = [
    R.default_camera(1280, 720),
    dict(eye=(0.0, 0.0, 0.0), target=(0.3, 0.1, -1.0), up=(0.0, 1.0, 0.0), aspect=1.0, fovy_deg=60.0, znear=0.01,
         zfar=10.0),
    dict(eye=(-3.0, 0.5, 0.25), target=(1.0, -2.0, 0.5), up=(0.1, 0.2, 1.0), aspect=2.35, fovy_deg=20.0, znear=0.5,
         zfar=1000.0),
    dict(eye=(5.0, 5.0, 5.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), aspect=0.5625, fovy_deg=100.0, znear=1e-3,
         zfar=50.0),
]


@pytest.mark.parametrize("k", range(len(CAMERAS)))
def test_view_proj_matches_the_float64_restatement(nb, k):
    cam = CAMERAS[k]
    got = nb.Camera(**cam).view_proj()
    ref = R.view_proj(cam)
    # double evaluation rounded once: the same float, or its neighbour where the two libms' tan differ
    ulp = np.spacing(np.abs(ref)).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulp), (got, ref)
    assert np.all((ref == 0) == (got == 0))


def test_default_view_proj_known_structure(nb):
    m = nb.Camera.default(1280, 720).view_proj().reshape(4, 4).T.astype(np.float64)  # M[r, c]
    # the camera target maps to the screen centre at distance |eye| = sqrt(5)
    c = m @ np.array([0.0, 0.0, 0.0, 1.0])
    assert c[0] == 0 and c[1] == 0 and abs(c[3] - np.sqrt(5.0)) < 1e-6 and 0 < c[2] < c[3]
    assert abs(m[0, 0] - 1.0 / np.tan(np.pi / 8) / (1280 / 720)) < 1e-6


def test_bad_arguments_are_invalid_without_a_device(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID

    def params():
        p = _lib.nb_render_params()
        assert L.nb_render_params_default(C.byref(p), 64, 32) == 0
        return p

    st = _lib.nb_render_stats()
    for call in (L.nb_sim_render, L.nb_runner_render):
        assert call(None, None, None, None, C.byref(st)) == INV and b"params" in L.nb_last_error()
        for field, value, word in (("width", 0, b"width"), ("height", 0, b"width"), ("width", 16385, b"width"),
                                   ("height", 1 << 20, b"width"), ("flags", 2, b"flag"), ("flags", 0x80000001, b"flag"),
                                   ("alpha", -0.01, b"alpha"), ("alpha", 1.5, b"alpha"), ("alpha", float("nan"), b"alpha"),
                                   ("half_size", float("inf"), b"half_size"), ("half_size", float("nan"), b"half_size")):
            p = params()
            setattr(p, field, value)
            assert call(None, C.byref(p), None, None, C.byref(st)) == INV, (field, value)
            assert word in L.nb_last_error(), (field, L.nb_last_error())
        for k, bad in ((0, float("nan")), (7, float("inf")), (15, -float("inf"))):
            p = params()
            p.view_proj[k] = bad
            assert call(None, C.byref(p), None, None, C.byref(st)) == INV and b"view_proj" in L.nb_last_error()
        p = params()
        p.clear[1] = 2.0
        assert call(None, C.byref(p), None, None, C.byref(st)) == INV and b"clear" in L.nb_last_error()
        # good parameters, no simulator
        p = params()
        assert call(None, C.byref(p), None, None, C.byref(st)) == INV and b"null" in L.nb_last_error()
    assert bytes(st) == bytes(C.sizeof(st))  # nothing was written
    cam = _lib.nb_camera()
    assert L.nb_camera_default(None, 4, 4) == INV
    assert L.nb_camera_default(C.byref(cam), 0, 4) == INV and L.nb_camera_default(C.byref(cam), 4, 16385) == INV
    assert L.nb_camera_view_proj(None, (C.c_float * 16)()) == INV
    assert L.nb_camera_view_proj(C.byref(cam), None) == INV
    assert L.nb_render_params_default(None, 4, 4) == INV
    assert L.nb_render_params_default(C.byref(_lib.nb_render_params()), 4, 0) == INV
    # eye == target: no direction, no finite matrix
    L.nb_camera_default(C.byref(cam), 4, 4)
    for k in range(3):
        cam.target[k] = cam.eye[k]
    assert L.nb_camera_view_proj(C.byref(cam), (C.c_float * 16)()) == INV and b"finite" in L.nb_last_error()
    assert L.nb_sim_set_tuning(None, b"render_design", 1) == INV


# ---------------------------------------------------------------------------------------------
# known answers of the restatement
# ---------------------------------------------------------------------------------------------
def _px(i, j):
    """The snapped coordinates of the centre of pixel (i, j)."""
    return (256 * i + 128, 256 * j + 128)


@pytest.mark.parametrize("diagonal", [0, 1])
@pytest.mark.parametrize("flip", [False, True])
def test_rectangle_on_pixel_centres_covers_each_pixel_once(diagonal, flip):
    a, b, c, d = _px(1, 1), _px(6, 1), _px(6, 5), _px(1, 5)  # clockwise on screen (y down)
    tris = [(a, b, c), (a, c, d)] if diagonal == 0 else [(a, b, d), (b, c, d)]
    if flip:
        tris = [t[::-1] for t in tris]
    counts, per = R.rasterize(np.array(tris), 9, 8, per_triangle=True)
    want = np.zeros((8, 9), np.uint32)
    want[1:5, 1:6] = 1  # top row and left column in, bottom row and right column out
    assert np.array_equal(counts, want)
    assert per.sum() == 20


@pytest.mark.parametrize("centre", [_px(4, 4), (256 * 4 + 37, 256 * 4 + 200)])
def test_fan_of_eight_covers_every_pixel_once(centre):
    ring = [_px(0, 0), _px(4, 0), _px(8, 0), _px(8, 4), _px(8, 8), _px(4, 8), _px(0, 8), _px(0, 4)]
    # pushed out so that the fan covers the whole 9 x 9 image, its rim off the pixel grid
    ring = [(x + (x - 1152) * 3 + 5, y + (y - 1152) * 3 - 7) for x, y in ring]
    tris = [(centre, ring[k], ring[(k + 1) % 8]) for k in range(8)]
    for order in (tris, [t[::-1] for t in tris], [t if k % 2 else t[::-1] for k, t in enumerate(tris)]):
        assert np.array_equal(R.rasterize(np.array(order), 9, 9), np.ones((9, 9), np.uint32))


def test_degenerate_triangles_cover_nothing():
    tris = [(_px(1, 1), _px(3, 3), _px(5, 5)), (_px(2, 2), _px(2, 2), _px(2, 2)), (_px(0, 3), _px(7, 3), _px(3, 3))]
    assert R.rasterize(np.array(tris), 8, 8).sum() == 0


def test_scissor_discards_pixels_outside_the_image():
    t = np.array([[(-5000, -5000), (10000, -5000), (-5000, 10000)]])
    counts, per = R.rasterize(t, 4, 3, per_triangle=True)
    assert counts.shape == (3, 4) and per[0] == counts.sum() > 0
    full = R.rasterize(t + 256 * 40, 100, 100)  # the same triangle well inside a larger image
    assert np.array_equal(counts, full[40:43, 40:44])


def test_one_body_at_the_camera_target():
    """Default camera, 1280 x 720, one body at the origin (the camera target).  By hand: c = M[:, 3],
    c_x = c_y = 0, c_w = |eye| = sqrt(5) = 2.236068.  s / c_w = 0.006 / 2.236068 = 0.00268328, so the
    vertices fall at sx = 640 -+ 0.00268328 * 640 = 638.2827, 641.7173 (and 640 for the apex),
    sy = 360 + 0.00268328 * 360 = 360.9660 for the two lower vertices and 359.0340 for the apex: an
    upright triangle 3.43 pixels wide and 1.93 high.  Rows of pixel centres: y = 359.5 is 0.466 below
    the apex, where the triangle is 2 * 1.7173 * 0.466 / 1.932 = 0.83 wide, centred on x = 640, i.e.
    (639.586, 640.414): no centre (639.5, 640.5 miss).  y = 360.5 is 1.466 below the apex, width 2.606:
    (638.697, 641.303) holds the centres 639.5 and 640.5.  y = 361.5 is below the base.  So exactly
    the pixels (639, 360) and (640, 360) are covered."""
    vp = R.view_proj(R.default_camera(1280, 720))
    counts, st = R.render_counts(np.zeros((1, 3), np.float32), vp, 1280, 720)
    assert st == dict(n=1, drawn=1, clipped=0, oversize=0, nonfinite=0, fragments=2, max_count=1)
    assert sorted(zip(*np.nonzero(counts))) == [(360, 639), (360, 640)]  # (row, column)
    tri, cls = R.project(np.zeros((1, 3), np.float32), vp, 1280, 720)
    assert cls[0] == 0
    want = np.array([[638.2827, 360.9660], [641.7173, 360.9660], [640.0, 359.0340]]) * 256
    assert np.all(np.abs(tri[0] - want) <= 1.0)


def test_classes_clipped_oversize_nonfinite():
    cam = R.default_camera(1280, 720)
    vp = R.view_proj(cam)
    eye = np.array(cam["eye"])
    fwd = -eye / np.linalg.norm(eye)
    bodies = np.array([eye - 0.5 * fwd,        # behind the eye
                       eye + 1.0 * fwd,        # drawn
                       [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf]], dtype=np.float32)
    _, cls = R.project(bodies, vp, 1280, 720)
    assert list(cls) == [1, 0, 3, 3, 3]
    _, st = R.render_counts(bodies, vp, 1280, 720)
    assert (st["drawn"], st["clipped"], st["oversize"], st["nonfinite"]) == (1, 1, 0, 3)
    assert st["drawn"] + st["clipped"] + st["oversize"] + st["nonfinite"] == st["n"]
    # A body 1e-7 in front of the eye plane.  (With the eye at (0, 1, 2) float32 positions are 1.2e-7
    # apart and znear = 1e-5 clips it first: the eye goes to the origin and znear to 1e-9.)  c_w = 1e-7,
    # s / c_w = 6e4 in NDC, 3.8e7 pixels from the centre: beyond 2^22, not drawn, `oversize`.
    near = dict(cam, eye=(0.0, 0.0, 0.0), target=(0.0, 0.0, -1.0), znear=1e-9)
    close = np.array([[0.0, 0.0, -1e-7], [0.0, 0.0, -1e-4], [0.0, 0.0, 1e-7]], dtype=np.float32)
    tri, cls = R.project(close, R.view_proj(near), 1280, 720)
    assert list(cls) == [2, 0, 1]
    assert np.abs(tri[1]).max() < 2 ** 30 and R.rasterize(tri[1:2], 1280, 720).sum() > 1000
    # The far plane.  With the reference's znear = 1e-5, c_z / c_w = 1 - znear (1/d - 1/zfar) differs
    # from 1 by less than one float32 ulp at any distance d, so whether a body beyond zfar is clipped
    # is decided by rounding; the far plane is a plane again with a nearer one further out.
    far = dict(cam, znear=0.1)
    depth = np.array([eye + 99.0 * fwd, eye + 101.0 * fwd, eye + 150.0 * fwd, eye + 0.05 * fwd], dtype=np.float32)
    _, cls = R.project(depth, R.view_proj(far), 1280, 720)
    assert list(cls) == [0, 1, 1, 1]  # inside, beyond zfar twice, nearer than znear


def test_sum_of_counts_is_the_sum_over_triangles(nb):
    xyz = make_state("uniform", 10000, 4)[:, 0:3]
    vp = R.view_proj(R.default_camera(640, 360))
    tri, cls = R.project(xyz, vp, 640, 360)
    drawn = tri[cls == 0]
    counts, per = R.rasterize(drawn, 640, 360, per_triangle=True)
    assert counts.sum(dtype=np.uint64) == per.sum() and per.sum() > 5000
    # one triangle at a time over the whole image agrees with the windowed path
    whole = [int(R.cover(drawn[k:k + 1], [0], [0], 640, 360).sum()) for k in range(50)]
    assert whole == [int(v) for v in per[:50]]


def test_order_of_the_bodies_does_not_matter(nb):
    xyz = make_state("disc", 5000, 2)[:, 0:3]
    vp = R.view_proj(R.default_camera(320, 200))
    a, sa = R.render_counts(xyz, vp, 320, 200)
    b, sb = R.render_counts(xyz[np.random.default_rng(0).permutation(5000)], vp, 320, 200)
    assert np.array_equal(a, b) and sa == sb


# ---------------------------------------------------------------------------------------------
# colour and files
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("srgb", [True, False])
def test_colour_closed_form_equals_sequential_blends(srgb):
    clear = np.array([float(np.float32(c)) for c in R.CLEAR])
    dst = clear.copy()
    for k in range(9):
        want = 255.0 * (R.srgb_encode(dst) if srgb else dst)
        assert np.allclose(R.colour64(np.array(k), srgb=srgb), want, rtol=0, atol=1e-12)
        dst = 1.0 * 0.25 + dst * (1.0 - 0.25)  # ALPHA_BLENDING: src * src.a + dst * (1 - src.a)
    px = R.rgba8(np.array([[0, 1, 1000]]))
    assert px.shape == (1, 3, 4) and np.all(px[..., 3] == 255)
    assert tuple(px[0, 2]) == (255, 255, 255, 255)
    assert tuple(px[0, 0]) == (25, 0, 63, 255)  # sRGB bytes of the clear colour: 255 enc(0.01) = 25.46, 255 enc(0.05) = 63.19


def test_write_ppm_round_trips(nb, tmp_path):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(7, 13, 4), dtype=np.uint8)
    path = tmp_path / "f.ppm"
    nb.write_ppm(str(path), img)
    raw = path.read_bytes()
    assert raw.startswith(b"P6\n13 7\n255\n") and len(raw) == len(b"P6\n13 7\n255\n") + 7 * 13 * 3
    assert np.array_equal(R.read_ppm(str(path)), img[:, :, :3])
    nb.write_ppm(str(path), img[:, :, :3])
    assert np.array_equal(R.read_ppm(str(path)), img[:, :, :3])
    with pytest.raises(ValueError):
        nb.write_ppm(str(path), img.astype(np.float32))
