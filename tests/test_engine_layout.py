"""The engine's host-side arithmetic (skirt_amd/csrc/host/engine_layout.cpp) on the CPU: tools/engine_layout_cpu.py
builds tools/engine_layout_check.cpp, which holds the cases, with the address and undefined-behaviour sanitizers and
this runs it, one group a test. The groups: the pool's layout (counted = carved, ordered, disjoint, aligned), the
instruments' tally layout, the tree numbering with the engine's refusals, the leaf-map plan, the Voronoi packing
decoded entry by entry, and the thresholds of the Labs and LDS plans. No GPU."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import engine_layout_cpu as E  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return E.build(str(tmp_path_factory.mktemp("layout_cpu")))


@pytest.mark.parametrize("group", E.GROUPS)
def test_engine_layout(exe, group):
    out = E.run(exe, group)
    assert out.startswith(group + ": "), out


def test_unknown_group_is_an_error(exe):
    with pytest.raises(RuntimeError, match="unknown group"):
        E.run(exe, "nothing")
