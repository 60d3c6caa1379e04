"""nb_sim_render on the device (csrc/nb_render.hip), all through the C ABI: the coverage counts
against the numpy restatement of the drawing rule (tests/render_ref.py), every pixel and every
statistic, exactly -- the rule is integer after a float32 projection that numpy reproduces, so no
tolerance applies; both kernel designs kept in the tree ("render_design" 1 direct, 2 tiled); the
colours against the float64 closed form of the device's own counts; that a render neither perturbs
nor overtakes the steps; the refusals; the CLI.  `-m gpu`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import render_ref as R
from tests.helpers import ROOT, bits, make_state

pytestmark = pytest.mark.gpu

DESIGNS = (1, 2)  # direct, tiled


def _naive(nb, state, **sp):
    return nb.NaiveSim.from_particles(nb.SimParams(particle_num=state.shape[0], **sp), None, state)


def _params(width, height, vp, half_size=R.HALF_SIZE, clear=R.CLEAR, alpha=R.ALPHA, flags=1):
    from wgpu_n_body_amd import _lib
    p = _lib.nb_render_params()
    p.width, p.height = width, height
    for k in range(16):
        p.view_proj[k] = float(vp[k])
    p.half_size, p.alpha, p.flags = float(half_size), float(alpha), flags
    for k in range(3):
        p.clear[k] = float(clear[k])
    return p


def _render(sim, p, rgba=True, counts=True, stats=True, call="nb_sim_render"):
    """One call through the C ABI: (rgba uint8 [H, W, 4] | None, counts uint32 [H, W] | None, stats dict | None)."""
    from wgpu_n_body_amd import _lib
    img = np.full((p.height, p.width, 4), 0xA5, np.uint8) if rgba else None
    cnt = np.full((p.height, p.width), 0xA5A5A5A5, np.uint32) if counts else None
    st = _lib.nb_render_stats() if stats else None
    rc = getattr(_lib.lib(), call)(sim._h, C.byref(p), img.ctypes.data if rgba else None,
                                   cnt.ctypes.data if counts else None, C.byref(st) if stats else None)
    assert rc == 0, _lib.lib().nb_last_error()
    sd = None
    if stats:
        assert st.reserved == 0
        sd = {k: int(getattr(st, k)) for k in ("step_num", "n", "drawn", "clipped", "oversize", "nonfinite",
                                                "fragments", "max_count")}
    return img, cnt, sd


def _check(sim, xyz, width, height, vp, half_size=R.HALF_SIZE, step=0, designs=DESIGNS):
    """Counts and stats of every design against the restatement; returns the restatement's stats."""
    ref, want = R.render_counts(xyz, vp, width, height, half_size)
    want = dict(want, step_num=step)
    assert want["drawn"] + want["clipped"] + want["oversize"] + want["nonfinite"] == want["n"]
    for design in designs:
        sim.set_tuning("render_design", design)
        _, got, st = _render(sim, _params(width, height, vp, half_size), rgba=False)
        print(f"design {design} {width}x{height} n {want['n']}: {st}; pixels differing {int((got != ref).sum())}")
        assert st == want, (design, st, want)
        assert np.array_equal(got, ref), (design, int((got != ref).sum()))
    return want


SIZES = ((256, 144), (1280, 720), (333, 77))


@pytest.mark.parametrize("n", [64, 1000, 100000])
@pytest.mark.parametrize("init", ["uniform", "disc", "spherical"])
def test_counts_equal_the_restatement(gpu, init, n):
    state = make_state(init, n, seed=3)
    sim = _naive(gpu, state)
    for width, height in SIZES:
        want = _check(sim, state[:, 0:3], width, height, R.view_proj(R.default_camera(width, height)))
        assert want["drawn"] == n
    sim.destroy()


def _inside_cloud():
    """A uniform cloud around a camera at the origin that looks down -z with znear 1e-9 and zfar 1:
    half of it behind the eye, the corners beyond zfar, and by hand, on the axis: bodies at depth
    1e-7 and 3e-7 (oversize), 1e-4 and 3e-3 (triangles larger than the screen and a fifth of it),
    0.05 (a box a lane does not walk) and nearer than znear."""
    state = make_state("uniform", 100000, seed=5)
    hand = np.array([[0, 0, -1e-7], [1e-8, 0, -3e-7], [0, 0, -1e-4], [1e-4, -2e-4, -3e-3], [0.001, 0.001, -0.05],
                     [0, 0, -1e-10], [0, 0, 1e-7], [0.5, 0.5, -0.999], [0.9, 0.9, -0.9]], dtype=np.float32)
    state[:hand.shape[0], 0:3] = hand
    cam = dict(eye=(0.0, 0.0, 0.0), target=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), aspect=640.0 / 360.0, fovy_deg=45.0,
               znear=1e-9, zfar=1.0)
    return state, R.view_proj(cam)


def test_camera_inside_the_cloud(gpu):
    state, vp = _inside_cloud()
    sim = _naive(gpu, state)
    want = _check(sim, state[:, 0:3], 640, 360, vp)
    sim.destroy()
    assert want["oversize"] >= 2 and want["clipped"] > 40000 and want["drawn"] > 10000
    assert want["max_count"] >= 2 and want["fragments"] > 640 * 360  # the whole screen at least once


def test_a_matrix_that_is_no_camera(gpu):
    state = make_state("uniform", 100000, seed=6)
    rng = np.random.default_rng(11)
    sim = _naive(gpu, state)
    seen = 0
    for _ in range(3):
        vp = rng.normal(size=16).astype(np.float32)
        seen += _check(sim, state[:, 0:3], 512, 512, vp)["fragments"]
    # ... and one that overflows float32: inf - inf and inf / inf are not below 2^22
    vp = R.view_proj(R.default_camera(512, 512)).copy()
    vp[0], vp[4] = 3e38, -3e38
    _check(sim, state[:, 0:3], 512, 512, vp)
    sim.destroy()
    assert seen > 0


def test_nonfinite_bodies_are_counted_and_not_drawn(gpu):
    state = make_state("disc", 5000, seed=7)
    state[::7, 0] = np.nan
    state[3::11, 2] = np.inf
    state[5::13, 1] = -np.inf
    state[1::17, 9] = np.nan   # the mass is not a coordinate
    state[2::19, 4] = np.inf   # nor is a velocity
    sim = _naive(gpu, state)
    want = _check(sim, state[:, 0:3], 640, 360, R.view_proj(R.default_camera(640, 360)))
    sim.destroy()
    assert want["nonfinite"] == int((~np.isfinite(state[:, 0:3])).any(axis=1).sum()) > 1000


def test_half_size_zero_and_large(gpu):
    state = make_state("spherical", 20000, seed=8)
    sim = _naive(gpu, state)
    vp = R.view_proj(R.default_camera(640, 360))
    zero = _check(sim, state[:, 0:3], 640, 360, vp, half_size=0.0)
    assert zero["fragments"] == 0 and zero["drawn"] == 20000  # three equal vertices: no area
    big = _check(sim, state[:, 0:3], 640, 360, vp, half_size=0.05)
    assert big["fragments"] > 50 * 20000
    sim.destroy()


def test_a_million_bodies_at_1080p(gpu):
    state = make_state("uniform", 1 << 20, seed=9)
    sim = _naive(gpu, state)
    # design 0: left to itself the renderer bins a frame of this size
    want = _check(sim, state[:, 0:3], 1920, 1080, R.view_proj(R.default_camera(1920, 1080)), designs=(0, 1, 2))
    sim.destroy()
    assert want["fragments"] > 7 * (1 << 20)


def test_order_of_the_bodies_does_not_matter(gpu):
    nb = gpu
    state = make_state("disc", 50000, seed=10)
    perm = np.random.default_rng(3).permutation(state.shape[0])
    p = _params(800, 600, R.view_proj(R.default_camera(800, 600)))
    out = []
    for s in (state, state[perm]):
        sim = _naive(nb, s)
        for design in DESIGNS:
            sim.set_tuning("render_design", design)
            out.append(_render(sim, p))
        sim.destroy()
    for img, cnt, st in out[1:]:
        assert np.array_equal(cnt, out[0][1]) and np.array_equal(img, out[0][0]) and st == out[0][2]


def test_tree_order_after_steps(gpu):
    nb = gpu
    state = make_state("disc", 100000, seed=12)
    sim = nb.TreeSim.from_particles(nb.SimParams(particle_num=100000), nb.AddParams.TreeSimParams(0.75), state)
    for _ in range(5):
        sim.encode()
    vp = R.view_proj(R.default_camera(1280, 720))
    sim.set_tuning("render_design", 1)
    _, first, st = _render(sim, _params(1280, 720, vp), rgba=False)  # enqueued behind the five steps
    after = nb.as_floats(sim.read_particles())
    assert st["step_num"] == 5
    assert not np.array_equal(after[:, 9], state[:, 9]) or not np.array_equal(after[:, 0:3], state[:, 0:3])
    _check(sim, after[:, 0:3], 1280, 720, vp, step=5)
    assert np.array_equal(first, R.render_counts(after[:, 0:3], vp, 1280, 720)[0])
    sim.destroy()


@pytest.mark.parametrize("flags", [1, 0])
def test_rgba_is_the_closed_form_of_the_counts(gpu, flags):
    state, vp = _inside_cloud()
    state[100:1100, 0:3] = (0.01, 0.02, -0.5)  # a thousand coincident bodies: counts from 0 to beyond 1000
    sim = _naive(gpu, state)
    for clear, alpha in ((R.CLEAR, R.ALPHA), ((0.0, 1.0, 0.5), 0.01), ((0.2, 0.3, 0.4), 0.0), ((0.2, 0.3, 0.4), 1.0)):
        img, cnt, st = _render(sim, _params(640, 360, vp, clear=clear, alpha=alpha, flags=flags))
        exact = R.colour64(cnt, clear, alpha, srgb=bool(flags))
        err = np.abs(img[..., 0:3].astype(np.float64) - exact)
        print(f"flags {flags} clear {clear} alpha {alpha}: max count {st['max_count']}, max |byte - 255 enc| {err.max():.4f}")
        # one rounding boundary: the byte is round(exact) unless exact is within the float32 error of a half
        assert err.max() <= 0.5 + 1e-3
        assert np.all(np.abs(img[..., 0:3].astype(np.int64) - R.rgba8(cnt, clear, alpha, bool(flags))[..., 0:3]) <= 1)
        assert np.all(img[..., 3] == 255)
        assert st["max_count"] == cnt.max() and st["fragments"] == int(cnt.sum(dtype=np.uint64))
    assert st["max_count"] > 1000
    sim.destroy()


def test_repeatable_and_every_output_optional(gpu):
    state = make_state("uniform", 30000, seed=13)
    sim = _naive(gpu, state)
    p = _params(333, 77, R.view_proj(R.default_camera(333, 77)))
    for design in DESIGNS:
        sim.set_tuning("render_design", design)
        a, b = _render(sim, p), _render(sim, p)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
        assert _render(sim, p, rgba=True, counts=False, stats=False)[0].tobytes() == a[0].tobytes()
        assert _render(sim, p, rgba=False, counts=True, stats=False)[1].tobytes() == a[1].tobytes()
        assert _render(sim, p, rgba=False, counts=False, stats=True)[2] == a[2]
        assert _render(sim, p, rgba=False, counts=False, stats=False) == (None, None, None)
    # the Python mirror returns the same frame
    sim.set_tuning("render_design", 0)
    frame, counts = sim.render(333, 77, counts=True)
    assert frame.shape == (77, 333, 4) and frame.dtype == np.uint8 and np.array_equal(np.asarray(frame), a[0])
    assert np.array_equal(counts, a[1]) and frame.stats.fragments == a[2]["fragments"] and frame.stats.n == 30000
    assert np.array_equal(np.asarray(sim.render(333, 77, camera=gpu.Camera.default(333, 77))), a[0])
    with pytest.raises(gpu.NBodyError):
        sim.set_tuning("render_design", 3)
    sim.destroy()


@pytest.mark.parametrize("kind", ["tree", "naive"])
def test_render_does_not_touch_the_trajectory(gpu, kind):
    nb = gpu
    n = 20000 if kind == "tree" else 4096
    state = make_state("disc", n, seed=14)
    sp = nb.SimParams(particle_num=n)
    p = _params(640, 360, R.view_proj(R.default_camera(640, 360)))
    ends = []
    for with_render in (False, True):
        sim = (nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state) if kind == "tree"
               else nb.NaiveSim.from_particles(sp, None, state))
        for step in range(20):
            sim.encode()
            if with_render:
                sim.set_tuning("render_design", 1 + step % 2)
                _, _, st = _render(sim, p, rgba=False, counts=False)
                assert st["step_num"] == step + 1 and st["n"] == n
        ends.append((nb.as_floats(sim.read_particles()).copy(), sim.step_num()))
        sim.destroy()
    assert ends[0][1] == ends[1][1] == 20
    assert np.array_equal(bits(ends[0][0]), bits(ends[1][0]))


def test_render_is_ordered_after_enqueued_steps(gpu):
    nb = gpu
    sp = nb.SimParams(particle_num=50000)
    runner = nb.OfflineHeadless(nb.TreeSim, sp, nb.AddParams.TreeSimParams(0.75),
                                lambda q: nb.inits.disc_init(q, seed=15))
    runner.step_n(5)
    vp = R.view_proj(R.default_camera(640, 360))

    class H:  # the runner's handle where _render expects a simulator's
        _h = runner._h
    _, cnt, st = _render(H, _params(640, 360, vp), rgba=False, call="nb_runner_render")
    after = nb.as_floats(runner.read_particles())
    ref, want = R.render_counts(after[:, 0:3], vp, 640, 360)
    assert st == dict(want, step_num=5) and np.array_equal(cnt, ref)
    frame = runner.render(640, 360)
    assert frame.stats.step_num == 5 and frame.stats.fragments == want["fragments"]
    runner.destroy()


def test_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    state = make_state("uniform", 64, seed=1)
    p = _params(64, 32, R.view_proj(R.default_camera(64, 32)))
    st = _lib.nb_render_stats()
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, state, placement=nb.Placement(world=2))
    assert L.nb_sim_render(sharded._h, C.byref(p), None, None, C.byref(st)) == _lib.NB_ERR_UNSUPPORTED
    assert b"sharded" in L.nb_last_error()
    p.width = 0  # the argument check comes first
    assert L.nb_sim_render(sharded._h, C.byref(p), None, None, C.byref(st)) == _lib.NB_ERR_INVALID
    sharded.destroy()
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda q: nb.inits.uniform_init(q, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.render(64, 32)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()
    assert bytes(st) == bytes(C.sizeof(st))


def test_cli_frames(gpu, tmp_path):
    nb = gpu
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    frames = tmp_path / "frames"
    frames.mkdir()
    base = ["--sim", "tree", "--n", "20000", "--init", "disc", "--seed", "4", "--g", "1e-5", "--e", "2e-4", "--dt",
            "0.0016", "--theta", "0.75", "--steps", "4"]
    with_frames = subprocess.run([cli] + base + ["--frames", str(frames), "--frame-every", "2", "--frame-size", "320x200"],
                                 capture_output=True, text=True, timeout=300)
    plain = subprocess.run([cli] + base, capture_output=True, text=True, timeout=300)
    assert with_frames.returncode == 0 and plain.returncode == 0, with_frames.stderr + plain.stderr
    assert sorted(os.listdir(frames)) == ["frame_000000.ppm", "frame_000002.ppm", "frame_000004.ppm"]
    blank = lambda text: [re.sub(r"\d+ µs", "N µs", ln) for ln in text.splitlines()]  # noqa: E731
    lines = blank(with_frames.stdout)
    frame_lines = [ln for ln in lines if ln.startswith("Frame ")]
    assert [ln for ln in lines if not ln.startswith("Frame ")] == blank(plain.stdout)
    assert plain.stdout.count("Step Duration: ") == 4 and "Frame" not in plain.stdout
    # the same run in Python
    sp = nb.SimParams(particle_num=20000, g=1e-5, e=2e-4, dt=0.0016)
    runner = nb.OfflineHeadless(nb.TreeSim, sp, nb.AddParams.TreeSimParams(0.75), lambda q: nb.inits.disc_init(q, seed=4))
    for k, step in enumerate((0, 2, 4)):
        if step:
            runner.step_n(2)
        frame = runner.sim.render(320, 200)
        assert np.array_equal(R.read_ppm(str(frames / f"frame_{step:06d}.ppm")), np.asarray(frame)[:, :, 0:3])
        s = frame.stats
        assert frame_lines[k] == (f"Frame {step}: drawn {s.drawn} clipped {s.clipped} oversize {s.oversize} "
                                  f"nonfinite {s.nonfinite} fragments {s.fragments} max_count {s.max_count}")
        assert s.fragments > 0
    runner.destroy()
    assert len(frame_lines) == 3
