"""What the seven analysis passes share (csrc/nb_analysis.hpp: the workspace slots of a simulator, the moments
pass behind every centre of mass, the buffers that grow; csrc/nb_analysis_sort.hpp: the sort of the three that sort
their bodies) must not let one pass leak into another: every entry point returns the same bytes whichever pass touched the simulator first and whatever ran in between.  And the
one state the centre rule treats on the host, a simulator without bodies, for the two passes whose suites do
not cover it.  `-m gpu`."""
import dataclasses

import numpy as np
import pytest

from tests.helpers import make_state

pytestmark = pytest.mark.gpu

CENTER, VELOCITY = (0.05, -0.02, 0.01), (0.01, 0.0, -0.02)


def _sim(nb, kind, state):
    sp = nb.SimParams(particle_num=state.shape[0])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state)


def _blob(x):
    """Every bit an entry point returned: the arrays' bytes, the scalars as float64 / int64."""
    if dataclasses.is_dataclass(x):
        return b"".join(_blob(getattr(x, f.name)) for f in dataclasses.fields(x))
    if isinstance(x, (tuple, list)):
        return b"".join(_blob(v) for v in x)
    if x is None:
        return b"-"
    if isinstance(x, float):
        return np.float64(x).tobytes()
    if isinstance(x, int):
        return np.int64(x).tobytes()
    return np.ascontiguousarray(x).tobytes() + _blob(getattr(x, "stats", None))  # (a Frame carries its stats)


def _passes(pts):
    return {
        "diagnostics": lambda s: s.diagnostics(potential=True),
        "render": lambda s: s.render(64, 48, counts=True),
        "radial": lambda s: s.radial_profile(nbins=7, rmin=0.02, rmax=1.5),
        "field": lambda s: s.field(pts),
        "map": lambda s: s.projected_map(17, 33, extent=(-1.0, 1.0, -1.0, 1.0)),
        "fof": lambda s: s.fof_groups(0.02, min_members=2),
        "knn": lambda s: s.knn_density(6),
    }


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_every_first_use_order_gives_the_same_bytes(gpu, kind):
    nb = gpu
    state = make_state("spherical", 4097, seed=21)
    passes = _passes(state[::64, 0:3].copy() + np.float32(0.01))
    names = list(passes)
    seen = {}
    for order in (names, names[3:] + names[:3][::-1]):  # map and field before the moments' own pass, and after
        sim = _sim(nb, kind, state)
        for name in order + order[::-1]:
            got = _blob(passes[name](sim))
            assert seen.setdefault(name, got) == got, f"{name} differs (first use order {order})"
        sim.destroy()
    assert sorted(seen) == sorted(names)


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_no_bodies(gpu, kind):
    nb = gpu
    sim = _sim(nb, kind, np.zeros((0, 10), np.float32))
    for cylindrical in (False, True):
        p = sim.radial_profile(nbins=7, rmin=0.02, rmax=1.5, cylindrical=cylindrical, center=CENTER, velocity=VELOCITY)
        assert np.array_equal(p.center, CENTER) and np.array_equal(p.velocity, VELOCITY)
        assert (p.n, p.nonfinite, p.inside_count, p.outside_count) == (0, 0, 0, 0)
        assert (p.mass, p.inside_mass, p.outside_mass) == (0.0, 0.0, 0.0) and not p.shape.any()
        sums = (p.bin_mass, p.m_r, p.m_ur, p.m_ur2, p.m_uphi, p.m_uphi2, p.m_u2, p.ang)
        assert not p.count.any() and not any(s.any() for s in sums)
        p = sim.radial_profile(nbins=7, rmin=0.02, rmax=1.5, cylindrical=cylindrical)
        assert np.isnan(p.center).all() and np.isnan(p.velocity).all()
        assert p.n == 0 and p.mass == 0.0 and not p.count.any() and not p.bin_mass.any()
    for velocities in (True, False):
        m = sim.projected_map(17, 33, extent=(-1.0, 1.0, -1.0, 1.0), center=CENTER, velocity=VELOCITY,
                              velocities=velocities)
        assert np.array_equal(m.center, CENTER) and np.array_equal(m.velocity, VELOCITY)
        assert (m.n, m.nonfinite, m.binned_count, m.outside_count, m.max_count) == (0, 0, 0, 0, 0)
        assert (m.total_mass, m.binned_mass, m.outside_mass) == (0.0, 0.0, 0.0)
        planes = (m.mass, m.m_ua, m.m_ub, m.m_w, m.m_w2, m.m_u2) if velocities else (m.mass,)
        assert m.counts.shape == (33, 17) and not m.counts.any() and not any(q.any() for q in planes)
        m = sim.projected_map(17, 33, extent=(-1.0, 1.0, -1.0, 1.0), velocities=velocities)
        assert np.isnan(m.center).all() and np.isnan(m.velocity).all()
        assert m.n == 0 and m.total_mass == 0.0 and not m.counts.any() and not m.mass.any()
    sim.destroy()
