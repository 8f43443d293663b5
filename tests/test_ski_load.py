"""The host set-up (skirt_amd/csrc/host/build.cpp and the files it drives) on the CPU under the address and
undefined-behaviour sanitizers: tools/ski_load_cpu.py builds tools/ski_load_check.cpp, a program of its own, from the
set-up's sources and this runs it directly on every model of tests/golden/ski/. The program must end with status 0
(no sanitizer report, no refused model) and print one line per model: name, cell count, sum of the densities.
No GPU."""
import math
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import ski_load_cpu as S  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return S.build(str(tmp_path_factory.mktemp("ski_load")))


def test_every_model_loads_clean(exe):
    output = S.run(exe, S.models())
    names = [os.path.basename(p) for p in S.models()]
    assert names, "no fixture models"
    lines = output.splitlines()
    assert [ln.split()[0] for ln in lines] == names, output
    for ln in lines:
        name, cells, rho = ln.split()
        assert int(cells) >= 0 and math.isfinite(float(rho)) and float(rho) >= 0, ln


def test_a_refused_model_is_an_error(exe, tmp_path):
    bad = tmp_path / "empty.ski"
    bad.write_text("<?xml version='1.0'?>\n<skirt-simulation-hierarchy type='MonteCarloSimulation'>"
                   "<NoSimulation/></skirt-simulation-hierarchy>\n")
    with pytest.raises(RuntimeError, match="refused: unsupported simulation type NoSimulation"):
        S.run(exe, [str(bad)])
