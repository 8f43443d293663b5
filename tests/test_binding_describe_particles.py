"""The maintainer binding's data extraction for imported particle dust (SPHDustDistribution), by the method of
test_binding_describe_geom.py: integration/describe_main.cpp sets the .ski up through the reference's own classes
and writes the descriptors the binding (integration/GpuPhotonEngine.cpp, unchanged) builds from the live items --
the densities from DustSystem::density, the tree, the Voronoi sites -- and skirt_sim_describe writes what the .ski
driver uploads. The two dumps must agree field by field; media.rho bit for bit on the tree and Cartesian models,
which pins the host's particle densities and masses in boxes (all three tree modes) to the reference's beyond the six
digits of ds_cellprops. The harness runs with the particle folder as its working directory: the reference looks
input files up in its -i folder, by default the working directory. Needs the reference's sources (the build
container), no GPU."""
import os
import subprocess

import numpy as np
import pytest

import descriptors as D
import skirt_amd as S
import test_binding_describe as B

pytestmark = B.pytestmark
harness = B.harness
PART = os.path.join(B.REPO, "tests", "golden", "particles")

MODELS = {"part_oct": (S.GRID_OCTREE, 2479), "part_oct_neg": (S.GRID_OCTREE, 2451), "part_oct_bary": (S.GRID_OCTREE, 2458),
          "part_cart": (S.GRID_CARTESIAN, 4096), "part_vor": (S.GRID_VORONOI, 1343), "part_vor_dd": (S.GRID_VORONOI, 400),
          "part_few": (S.GRID_OCTREE, 519)}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_binding_describes_the_model_as_the_ski_driver_does(harness, tmp_path, name):
    ski = B._ski(name, tmp_path)
    ours, binding = str(tmp_path / "driver.bin"), str(tmp_path / "binding.bin")
    S.Simulation(ski, input_path=PART).describe(ours)
    r = subprocess.run([harness, ski, binding, str(tmp_path)], capture_output=True, text=True, timeout=850, cwd=PART)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = D.read(ours), D.read(binding)
    diffs = D.differences(a, b)
    kind, ncells = MODELS[name]
    if kind == S.GRID_VORONOI:
        # as test_binding_describe_geom.py judges a Voronoi model: the reference samples a cell's density at points
        # of the bounding box Voro++ gives it, the host driver at points of the box of its own clipping of the same
        # cell; every other field is equal bit for bit (the sites among them: the particles inside the extent, or
        # the positions SPHDustDistribution::generatePosition drew)
        assert [k for k, _ in diffs] in ([], ["media.rho"]), diffs
        np.testing.assert_allclose(b["media.rho"], a["media.rho"], rtol=1e-12, atol=0)
    else:
        assert diffs == []
        assert np.array_equal(a["media.rho"], b["media.rho"])
    assert a["grid.kind"][0] == kind and a["grid.ncells"][0] == ncells and a["media.ncomp"][0] == 1
    assert a["media.rho"].sum() > 0 and a["sources.lumtot"].sum() > 0 and a["instruments.n"][0] == 2
