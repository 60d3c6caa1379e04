"""Phase-space groups at the C-ABI boundary, without a device: the entry points are exported, the Python mirror has
the C layout, bad arguments are refused before any device is touched, and the two numpy restatements of the rule
(tests/fof6_ref.py) agree with each other, reduce to the friends-of-friends restatement under equal velocities, refine
it, and separate two crossing streams it joins."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import fof6_ref as F6
from tests import fof_ref as F
from tests.helpers import ROOT

NAMES = ("nb_fof6_sim", "nb_fof6_runner")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_fof6_params) F(nb_fof6_params, link) F(nb_fof6_params, vlink) F(nb_fof6_params, min_members)
    F(nb_fof6_params, flags) F(nb_fof6_params, reserved)
    return 0;
}
"""


def test_fof6_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    assert "PhaseSpaceGroups" in nb.__all__ and issubclass(nb.PhaseSpaceGroups, nb.FofGroups)
    assert nb.Simulator.phase_space_groups is nb.OfflineHeadless.phase_space_groups


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
    S = _lib.nb_fof6_params
    assert info["nb_fof6_params"] == (C.sizeof(S), C.alignment(S)) == (32, 8)
    for f, _ in S._fields_:
        assert info[f"nb_fof6_params.{f}"] == (getattr(S, f).offset, getattr(S, f).size), f
    assert len(S._fields_) == len(info) - 1


def good_params(_lib, **change):
    p = _lib.nb_fof6_params()
    p.link, p.vlink, p.min_members, p.flags, p.reserved = 0.1, 0.2, 20, 0, 0
    for k, v in change.items():
        setattr(p, k, v)
    return p


def test_bad_arguments_are_invalid_without_a_device(nb):
    """Every refusal that needs no simulator: the parameters are checked before the handle is looked at, so a null
    handle with good parameters is the one refusal that names the handle."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID
    labels = np.full(8, 7, np.uint32)
    group_of = np.full(8, 7, np.uint32)
    rows = np.zeros(4, _lib.FOF_GROUP_DTYPE)
    st = _lib.nb_fof_stats()
    for call, who in ((L.nb_fof6_sim, b"simulator"), (L.nb_fof6_runner, b"runner")):
        def bad(word, p):
            assert call(None, C.byref(p) if p is not None else None, labels.ctypes.data, group_of.ctypes.data,
                        rows.ctypes.data, 4, C.byref(st)) == INV, word
            assert word in L.nb_last_error(), (word, L.nb_last_error())
        bad(b"null params", None)
        for x in (0.0, -1.0, math.nan, math.inf, -math.inf, 1e-200, 1e200):  # (the last two: the square is 0, inf)
            bad(b"link", good_params(_lib, link=x))
            bad(b"vlink", good_params(_lib, vlink=x))
        # b2 and v2 are positive finite doubles, their product is not
        bad(b"product", good_params(_lib, link=1e-100, vlink=1e-100))
        bad(b"product", good_params(_lib, link=1e100, vlink=1e100))
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


CASES = F6.synthetic_cases(small=True)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_the_two_restatements_agree_and_refine_fof(idx):
    name, state, link, vlink = CASES[idx]
    assert state.shape[0] <= 2048
    for mm in (1, 2, 20):
        a, b = F6.fof6_brute(state, link, vlink, mm), F6.fof6_grid(state, link, vlink, mm)
        _agree(a, b)
        assert a["nonfinite"] + int(np.unique(a["labels"][a["labels"] != F.NONE], return_counts=True)[1].sum()) == a["n"]
        assert a["grouped_bodies"] == int(a["rows_count"].sum())
    fof = F.fof_grid(state, link, 1)
    assert F6.refines(a["labels"], fof["labels"]) and a["components"] >= fof["components"]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_equal_velocities_give_fof(idx):
    name, state, link, vlink = CASES[idx]
    state = state.copy()
    state[:, 3:6] = np.float32([0.25, -1.5, 3.0])
    want = F.fof_brute(state, link, 2)
    _agree(F6.fof6_brute(state, link, vlink, 2), want)
    _agree(F6.fof6_grid(state, link, vlink * 1e-3, 2), want)  # (however small vlink is)


def test_constructed_partitions():
    s = F6.crossing_streams()
    assert F.fof_brute(s, 0.015)["components"] == 1
    a = F6.fof6_brute(s, 0.015, 0.5)
    assert a["components"] == 2 and set(a["labels"][:200]) == {0} and set(a["labels"][200:]) == {200}
    for n in (63, 64, 65, 130):
        assert F6.fof6_brute(F6.one_cell(n, "cold"), 1.0, 1.0)["components"] == 1
        assert sorted(F6.fof6_brute(F6.one_cell(n, "parity"), 1.0, 1.0, 2)["rows_count"]) == [n // 2, n - n // 2]
        last = F6.fof6_brute(F6.one_cell(n, "last"), 1.0, 1.0, 2)
        assert last["components"] == n - 1 and last["rows_label"].tolist() == [n // 3] and last["labels"][n - 1] == n // 3
    p = F6.fof6_brute(F6.partial_joins(), 1.0, 1.0, 2)
    assert p["components"] == 100 and p["rows_label"].tolist() == [37, 81] and p["rows_count"].tolist() == [51, 51]
    assert set(p["labels"][100::2]) == {37} and set(p["labels"][101::2]) == {81}
    assert F.fof_brute(F6.partial_joins(), 1.0)["components"] == 1


def test_the_rule_at_its_edge():
    """link = vlink = 1, dx = (0.5, 0.5, 0.5), dv = (0.5, 0, 0): 0.75 + 0.25 = 1 exactly, friends; the next float32 up
    in one component of either difference is not; and with dv = 0, dx = (1, 0, 0) is the edge of clause 1."""
    up = np.nextafter(np.float32(0.5), np.float32(1.0))
    for dx, dv, friends in (((0.5, 0.5, 0.5), (0.5, 0, 0), True), ((0.5, up, 0.5), (0.5, 0, 0), False),
                            ((0.5, 0.5, 0.5), (up, 0, 0), False), ((1, 0, 0), (0, 0, 0), True),
                            ((np.nextafter(np.float32(1.0), np.float32(2.0)), 0, 0), (0, 0, 0), False)):
        s = F6.state_of([(0, 0, 0), dx], [(0, 0, 0), dv])
        assert F6.fof6_brute(s, 1.0, 1.0)["components"] == (1 if friends else 2), (dx, dv)
