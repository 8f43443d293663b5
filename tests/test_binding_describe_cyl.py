"""The maintainer binding's data extraction for a Cylinder2DDustGrid, by the method of test_binding_describe.py:
integration/describe_main.cpp sets the .ski up through the reference's own classes and writes the descriptors the
binding (integration/GpuPhotonEngine.cpp) builds from the live items -- the borders from meshR()->mesh()*maxR() and
meshZ()->mesh()*(maxZ()-minZ())+minZ(), the densities from DustSystem::density -- and skirt_sim_describe writes
what the .ski driver uploads. The two dumps must agree bit for bit, media.rho included: that pins the host's
(R, phi, z) density sampling, and the LogMesh, to the reference's. Needs /root/reference (the build container), no
GPU."""
import subprocess

import pytest

import descriptors as D
import skirt_amd as S
import test_binding_describe as B

pytestmark = B.pytestmark
harness = B.harness

MODELS = ["pan_cyl", "disk_cyl", "disk_cyl_log", "oligo_cyl"]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", MODELS)
def test_binding_describes_the_cylindrical_model_as_the_ski_driver_does(harness, tmp_path, name):
    ski = B._ski(name, tmp_path)
    ours, binding = str(tmp_path / "driver.bin"), str(tmp_path / "binding.bin")
    S.Simulation(ski).describe(ours)
    r = subprocess.run([harness, ski, binding, str(tmp_path)], capture_output=True, text=True, timeout=850)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = D.read(ours), D.read(binding)
    assert D.differences(a, b) == []
    assert a["grid.kind"][0] == S.GRID_CYLINDER2D and a["grid.ncells"][0] == 192
    assert a["grid.nx"][0] == 12 and a["grid.nz"][0] == 16 and a["grid.xv"][0] == 0.0
    assert a["media.rho"].sum() > 0 and a["sources.lumtot"].sum() > 0 and a["instruments.n"][0] >= 1
