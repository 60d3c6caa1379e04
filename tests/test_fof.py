"""Friends-of-friends groups at the C-ABI boundary, without a device: the entry points are exported, the Python
mirrors have the C layout, bad arguments are refused before any device is touched, and the two numpy
restatements of the rule (tests/fof_ref.py) agree with each other."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import fof_ref as F
from tests.helpers import ROOT, make_state

NAMES = ("nb_sim_fof", "nb_runner_fof")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_fof_params) F(nb_fof_params, link) F(nb_fof_params, min_members) F(nb_fof_params, flags)
    F(nb_fof_params, reserved)
    S(nb_fof_group) F(nb_fof_group, label) F(nb_fof_group, count) F(nb_fof_group, mass) F(nb_fof_group, mx)
    F(nb_fof_group, mv) F(nb_fof_group, mr2) F(nb_fof_group, mv2)
    S(nb_fof_stats) F(nb_fof_stats, step_num) F(nb_fof_stats, n) F(nb_fof_stats, nonfinite)
    F(nb_fof_stats, components) F(nb_fof_stats, groups) F(nb_fof_stats, grouped_bodies)
    F(nb_fof_stats, largest_count) F(nb_fof_stats, largest_label) F(nb_fof_stats, cells) F(nb_fof_stats, reserved)
    F(nb_fof_stats, cell_side)
    printf("NB_FOF_NONE %u 0\n", NB_FOF_NONE);
    printf("NB_FOF_MAX_CELLS_PER_AXIS %u 0\n", NB_FOF_MAX_CELLS_PER_AXIS);
    return 0;
}
"""


def test_fof_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    for name in ("FofGroups", "FofStats", "FOF_NONE"):
        assert name in nb.__all__ and hasattr(nb, name)
    for cls in (nb.Simulator, nb.OfflineHeadless):
        assert hasattr(cls, "fof_groups")
    assert nb.FOF_NONE == F.NONE == 0xFFFFFFFF


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
    for S, size in ((_lib.nb_fof_params, 24), (_lib.nb_fof_group, 80), (_lib.nb_fof_stats, 80)):
        name = S.__name__
        assert info[name] == (C.sizeof(S), C.alignment(S)) and C.sizeof(S) == size, name
        for f, _ in S._fields_:
            assert info[f"{name}.{f}"] == (getattr(S, f).offset, getattr(S, f).size), (name, f)
        assert len(S._fields_) == sum(1 for k in info if k.startswith(name + "."))
    dt = _lib.FOF_GROUP_DTYPE
    assert dt.itemsize == 80
    for f, _ in _lib.nb_fof_group._fields_:
        assert dt.fields[f][1] == getattr(_lib.nb_fof_group, f).offset, f
    assert info["NB_FOF_NONE"][0] == _lib.NB_FOF_NONE == 0xFFFFFFFF
    assert info["NB_FOF_MAX_CELLS_PER_AXIS"][0] == _lib.NB_FOF_MAX_CELLS_PER_AXIS == 1 << 21


def good_params(_lib, **change):
    p = _lib.nb_fof_params()
    p.link, p.min_members, p.flags, p.reserved = 0.1, 20, 0, 0
    for k, v in change.items():
        setattr(p, k, v)
    return p


def test_bad_arguments_are_invalid_without_a_device(nb):
    """Every refusal that needs no simulator: the parameters are checked before the handle is looked at, so a
    null handle with good parameters is the one refusal that names the handle."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID
    labels = np.full(8, 7, np.uint32)
    group_of = np.full(8, 7, np.uint32)
    rows = np.zeros(4, _lib.FOF_GROUP_DTYPE)
    st = _lib.nb_fof_stats()
    for call, who in ((L.nb_sim_fof, b"simulator"), (L.nb_runner_fof, b"runner")):
        def bad(word, p):
            assert call(None, C.byref(p) if p is not None else None, labels.ctypes.data, group_of.ctypes.data,
                        rows.ctypes.data, 4, C.byref(st)) == INV, word
            assert word in L.nb_last_error(), (word, L.nb_last_error())
        bad(b"null params", None)
        for link in (0.0, -1.0, math.nan, math.inf, -math.inf, 1e-200, 1e200):  # (the last two: link * link is 0, inf)
            bad(b"link", good_params(_lib, link=link))
        bad(b"min_members", good_params(_lib, min_members=0))
        bad(b"flag", good_params(_lib, flags=1))
        bad(b"flag", good_params(_lib, flags=0x80000000))
        bad(b"reserved", good_params(_lib, reserved=1))
        bad(b"reserved", good_params(_lib, reserved=1 << 40))
        bad(b"null " + who, good_params(_lib))
    assert np.all(labels == 7) and np.all(group_of == 7) and not rows.tobytes().strip(b"\0")


def _agree(a, b):
    for k in ("n", "nonfinite", "components", "groups", "grouped_bodies", "largest_count", "largest_label"):
        assert a[k] == b[k], k
    for k in ("labels", "group_of", "rows_label", "rows_count"):
        assert np.array_equal(a[k], b[k]), k
    assert np.all(np.abs(a["sums"] - b["sums"]) <= 1e-12 * a["scale"])


CASES = F.synthetic_cases(small=True)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_the_two_restatements_agree(idx):
    name, state, link, components = CASES[idx]
    assert state.shape[0] <= 2048
    for mm in (1, 2, 20):
        a, b = F.fof_brute(state, link, mm), F.fof_grid(state, link, mm)
        _agree(a, b)
        if components is not None:
            assert a["components"] == components, name
        assert a["nonfinite"] + int(np.unique(a["labels"][a["labels"] != F.NONE], return_counts=True)[1].sum()) == a["n"]
        assert a["grouped_bodies"] == int(a["rows_count"].sum())


@pytest.mark.parametrize("init", ["spherical", "disc"])
def test_the_two_restatements_agree_on_the_inits(nb, init):
    state = make_state(init, 2048, seed=11)
    state[[5, 77, 900], [0, 4, 9]] = (np.nan, np.inf, -np.inf)
    link = 0.02
    a, b = F.fof_brute(state, link, 2), F.fof_grid(state, link, 2)
    _agree(a, b)
    assert a["nonfinite"] == 3 and 1 < a["groups"] < a["components"] < 2045
    assert all(a["labels"][i] == F.NONE and a["group_of"][i] == F.NONE for i in (5, 77, 900))
