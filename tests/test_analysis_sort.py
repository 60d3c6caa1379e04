"""The shape of the sort the key-sorting analysis passes share (csrc/nb_analysis_sort.hpp: sort_shape, plain host
arithmetic that needs no HIP), through a small C++ probe, against the rule as DESIGN.md 6f states it: chunks of
max(256, ceil(n / 2048) rounded up to 64) elements, one wave each.  No GPU needed."""
import os
import subprocess

import pytest

from tests.helpers import ROOT

SIZES = [1, 63, 64, 65, 255, 256, 257, 262144, 262145, 524288, 524289, 4000000, 2**31 - 1]

PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include "nb_analysis_sort.hpp"
int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        const uint32_t n = (uint32_t)std::strtoul(argv[i], nullptr, 10);
        const nb::SortShape s = nb::sort_shape(n);
        std::printf("%u %u %u %zu %zu\n", n, s.chunk, s.blocks, s.hist_size(), s.totals_at());
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    d = tmp_path_factory.mktemp("sort_shape")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "wgpu_n_body_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)] + [str(n) for n in SIZES], capture_output=True, text=True, check=True).stdout
    rows = [tuple(int(x) for x in ln.split()) for ln in out.splitlines()]
    assert [r[0] for r in rows] == SIZES
    return {r[0]: r[1:] for r in rows}


@pytest.mark.parametrize("n", SIZES)
def test_sort_shape(shapes, n):
    chunk, blocks, hist, totals = shapes[n]
    assert chunk % 64 == 0 and chunk >= 256          # whole wave-loads, at least four
    assert 1 <= blocks <= 2048                       # at most 2,048 chunks
    assert blocks * chunk >= n > (blocks - 1) * chunk  # they cover the elements, and the last one is not empty
    per = -(-n // 2048)
    assert chunk == max(256, -(-per // 64) * 64)     # the rule itself
    assert totals == 256 * blocks and hist == totals + 256  # [256][blocks] counts, then the 256 digit totals
