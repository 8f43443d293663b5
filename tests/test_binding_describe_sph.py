"""The maintainer binding's data extraction for a Sphere1DDustGrid and a Sphere2DDustGrid, by the method of
test_binding_describe.py: integration/describe_main.cpp sets the .ski up through the reference's own classes and
writes the descriptors the binding (integration/GpuPhotonEngine.cpp) builds from the live items -- the shells from
meshR()->mesh()*maxR(), the polar borders and their cosines from meshTheta()->mesh() with the fix-up of
Sphere2DDustGrid::setupSelfAfter restated, the densities from DustSystem::density -- and skirt_sim_describe writes
what the .ski driver uploads. The two dumps must agree bit for bit, media.rho included: that pins the host's
(direction, r) and (r, theta, phi) density sampling, the LogMesh and the inserted border at pi/2 to the reference's.
Needs the reference's sources (the build container), no GPU."""
import subprocess

import pytest

import descriptors as D
import skirt_amd as S
import test_binding_describe as B

pytestmark = B.pytestmark
harness = B.harness

MODELS = {"pan_sph1": (S.GRID_SPHERE1D, 20), "pan_sph1_log": (S.GRID_SPHERE1D, 20),
          "disk_sph2": (S.GRID_SPHERE2D, 120), "oligo_sph2": (S.GRID_SPHERE2D, 192)}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_binding_describes_the_spherical_model_as_the_ski_driver_does(harness, tmp_path, name):
    ski = B._ski(name, tmp_path)
    ours, binding = str(tmp_path / "driver.bin"), str(tmp_path / "binding.bin")
    S.Simulation(ski).describe(ours)
    r = subprocess.run([harness, ski, binding, str(tmp_path)], capture_output=True, text=True, timeout=850)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = D.read(ours), D.read(binding)
    assert D.differences(a, b) == []
    kind, ncells = MODELS[name]
    assert a["grid.kind"][0] == kind and a["grid.ncells"][0] == ncells and a["grid.xv"][0] == 0.0
    assert a["grid.extent"][3] > 0 and (kind == S.GRID_SPHERE1D or 0.0 in a["grid.yv"])
    assert a["media.rho"].sum() > 0 and a["sources.lumtot"].sum() > 0 and a["instruments.n"][0] >= 1
