"""The C-ABI boundary (include/nbody.h <-> libnbody_hip.so) -- CPU only, no compute calls.

Checks that the library builds and loads, exports every function the header declares, that
the POD layouts match the reference's #[repr(C)] structs byte for byte, the shard arithmetic,
and the error behaviour without a device (the product must fail loudly: no CPU fallback).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT

HEADER = os.path.join(ROOT, "include", "nbody.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(nb_[a-z0-9_]+)\s*\(", src)
    return sorted(set(n for n in names if n != "nb_init_fn"))


def test_library_exports_every_declared_symbol(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    decl = declared_functions()
    assert len(decl) >= 30
    for name in decl:
        assert hasattr(L, name), f"{name} declared in nbody.h but not exported"
    assert sorted(_lib.ABI_SYMBOLS) == decl, "python binding list out of sync with the header"


def test_exports_are_plain_c_symbols(nb):
    from wgpu_n_body_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(declared_functions()) <= exported
    # nothing C++-mangled leaks out as part of the intended surface
    assert all(not s.startswith("_Z") or "nb" in s for s in exported)


def test_pod_layouts_match_the_reference(nb):
    from wgpu_n_body_amd import _lib
    # Particle: src/sims/mod.rs:9-16 -- 10 x f32 = 40 B, order pos/vel/acc/mass
    d = nb.PARTICLE_DTYPE
    assert d.itemsize == 40
    assert [d.fields[k][1] for k in ("position", "velocity", "acceleration", "mass")] == [0, 12, 24, 36]
    # SimParams: src/sims/mod.rs:51-58 -- u32 + 3 x f32 = 16 B
    assert C.sizeof(_lib.nb_sim_params) == 16
    assert [getattr(_lib.nb_sim_params, f).offset for f in ("particle_num", "g", "e", "dt")] == [0, 4, 8, 12]
    # Octant: src/sims/tree.rs:605-622 -- 52 B
    o = nb.OCTANT_DTYPE
    assert o.itemsize == 52
    assert [o.fields[k][1] for k in ("cog", "mass", "bodies", "children")] == [0, 12, 16, 20]
    assert C.sizeof(_lib.nb_add_params) == 8


def test_defaults_match_the_reference(nb):
    sp = nb.SimParams()  # SimParams::default, src/sims/mod.rs:62-71
    assert (sp.particle_num, sp.g, sp.e, sp.dt) == (10000, 0.000001, 0.0001, 0.016)
    assert nb.PARTICLES_PER_GROUP == 64  # src/sims/mod.rs:7
    hdr = open(HEADER).read()
    assert "#define NB_DEFAULT_THETA 0.75f" in hdr  # src/sims/tree.rs:42-51


def test_version_and_variants(nb):
    assert nb.version().startswith("nbody_hip") and "gfx950" in nb.version()
    # the library carries the hash of the sources it was built from: a stale .so shipped beside
    # newer sources (the .so is git-ignored and travels with the snapshot) fails here
    from wgpu_n_body_amd.build import source_hash
    assert nb.version().endswith("src:" + source_hash()), (nb.version(), source_hash())
    v = nb.naive_variants()
    assert len(v) >= 4 and len(set(v)) == len(v)


@pytest.mark.parametrize("n,world", [(65536, 1), (65536, 8), (262144, 8), (1000, 3), (1, 1),
                                     (0, 2), (255, 2), (257, 2), (4194304, 8)])
def test_shard_arithmetic(nb, n, world):
    per = nb.shard_bodies_per_rank(n, world)
    pad = nb.shard_padded_bodies(n, world)
    assert per % 256 == 0 and per > 0
    assert pad == per * world and pad >= n
    assert per * (world - 1) <= max(n, 1) + 256 * world   # not grossly over-padded
    # ranges are disjoint, ordered and cover [0, n)
    covered = 0
    for r in range(world):
        lo, hi = min(n, r * per), min(n, (r + 1) * per)
        assert lo == covered or lo == n
        covered = hi
    assert covered == n


def test_no_device_fails_loudly(nb):
    """Without a HIP device nb_sim_create must return NB_ERR_NO_DEVICE -- never fall back."""
    if nb.device_count() > 0:
        pytest.skip("this machine has a GPU; covered by the -m gpu tests")
    sp = nb.SimParams(particle_num=8)
    with pytest.raises(nb.NBodyError) as ei:
        nb.NaiveSim.new(sp, nb.AddParams.NaiveSimParams(), nb.inits.uniform_init)
    assert ei.value.code == 2 and "no CPU fallback" in str(ei.value)
    with pytest.raises(nb.NBodyError):
        nb.OfflineHeadless(nb.NaiveSim, sp, None, nb.inits.uniform_init)


def test_argument_errors_are_status_codes_not_crashes(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.nb_sim_create(C.byref(h), None, None, None, None, None) == _lib.NB_ERR_INVALID
    assert b"non-null" in L.nb_last_error() or b"null" in L.nb_last_error()
    assert L.nb_sim_encode(None) == _lib.NB_ERR_INVALID
    assert L.nb_sim_wait(None) == _lib.NB_ERR_INVALID
    assert L.nb_runner_step(None) == _lib.NB_ERR_INVALID
    assert L.nb_sim_destroy(None) == _lib.NB_OK and L.nb_runner_destroy(None) == _lib.NB_OK
    sp = _lib.nb_sim_params(4, 1e-6, 1e-4, 0.016)
    bad = _lib.nb_add_params(7, 0.0)
    buf = np.zeros(4, dtype=nb.PARTICLE_DTYPE)
    rc = L.nb_sim_create_from_particles(C.byref(h), C.byref(sp), C.byref(bad), None,
                                        buf.ctypes.data, 4)
    assert rc == _lib.NB_ERR_INVALID and b"kind" in L.nb_last_error()


def test_init_fn_exceptions_do_not_cross_the_abi(nb):
    def boom(_sp):
        raise KeyError("init exploded")

    with pytest.raises(KeyError):
        nb.NaiveSim.new(nb.SimParams(particle_num=4), None, boom)

    def short(_sp):
        return np.zeros(3, dtype=nb.PARTICLE_DTYPE)

    with pytest.raises(ValueError):
        nb.NaiveSim.new(nb.SimParams(particle_num=4), None, short)


PASS_METHODS = ["diagnostics", "radial_profile", "field", "circular_velocity", "projected_map", "fof_groups",
                "bound_groups", "hop_groups", "knn_density", "halo_profiles", "group_profiles", "shapes_of",
                "group_shapes", "smoothed_map", "render"]
# nb_sim_* entry points that are not analysis passes: the runner has its own protocol for them, or none
NOT_PASSES = {"create", "create_from_particles", "encode", "encode_phase", "let_set_imports", "let_set_import_stride",
              "let_set_owners", "let_set_arrivals", "cleanup", "wait", "sim_params", "read_particles",
              "write_particles", "read_tree", "exchange_region", "exchange_count", "exchange_region_i", "step_num",
              "encode_n_timed", "set_tuning", "debug_buffer", "destroy"}


def test_a_pass_is_stated_once_for_simulator_and_runner(nb):
    """Every analysis pass is one Python method shared by Simulator and OfflineHeadless, and one set of argument
    types shared by nb_sim_<pass> and nb_runner_<pass>."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for m in PASS_METHODS:
        assert getattr(nb.Simulator, m) is getattr(nb.OfflineHeadless, m), m
    passes = [s[len("nb_sim_"):] for s in _lib.ABI_SYMBOLS if s.startswith("nb_sim_")]
    passes = [p for p in passes if p not in NOT_PASSES]
    assert len(passes) == 12, passes
    for p in passes:
        assert "nb_runner_" + p in _lib.ABI_SYMBOLS, p
        a, b = getattr(L, "nb_sim_" + p).argtypes, getattr(L, "nb_runner_" + p).argtypes
        assert a is not None and list(a) == list(b), p


def test_product_does_not_import_the_oracle():
    """The oracle is test infrastructure: nothing under wgpu_n_body_amd/ may reference it."""
    pkg = os.path.join(ROOT, "wgpu_n_body_amd")
    for dirpath, _dirs, files in os.walk(pkg):
        if "_build" in dirpath or "__pycache__" in dirpath:
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "nbody_oracle" not in text and "from oracle" not in text \
                    and "import oracle" not in text and "libnbody_oracle" not in text, f
