"""The maintainer binding's data extraction for the six closed-form geometries (Shell, Gamma, Gaussian, TTauriDisk,
Torus, ConicalShell), by the method of test_binding_describe.py: integration/describe_main.cpp sets the .ski up
through the reference's own classes and writes the descriptors the binding (integration/GpuPhotonEngine.cpp) builds
from the live items -- a source's parameters from the geometry's getters and cached constants (_smin, _sdiff, _A,
_rho0, the sines), the densities from DustSystem::density -- and skirt_sim_describe writes what the .ski driver
uploads. The two dumps must agree field by field, media.rho included: that pins the host's densities of the new
kinds, on every grid kind the models use, and the Voronoi sites drawn by the six samplers, to the reference's.
Needs the reference's sources (the build container), no GPU."""
import subprocess

import numpy as np
import pytest

import descriptors as D
import skirt_amd as S
import test_binding_describe as B

pytestmark = B.pytestmark
harness = B.harness

MODELS = {"torus_sph2": (S.GRID_SPHERE2D, 192, [S.GEOM_POINT]), "cone_cyl": (S.GRID_CYLINDER2D, 192, [S.GEOM_POINT]),
          "vor_geoms": (S.GRID_VORONOI, 600, [S.GEOM_PLUMMER]),
          "gauss_gamma_cart": (S.GRID_CARTESIAN, 4096, [S.GEOM_GAUSSIAN, S.GEOM_GAMMA])}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_binding_describes_the_model_as_the_ski_driver_does(harness, tmp_path, name):
    ski = B._ski(name, tmp_path)
    ours, binding = str(tmp_path / "driver.bin"), str(tmp_path / "binding.bin")
    S.Simulation(ski).describe(ours)
    r = subprocess.run([harness, ski, binding, str(tmp_path)], capture_output=True, text=True, timeout=850)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = D.read(ours), D.read(binding)
    diffs = D.differences(a, b)
    kind, ncells, sources = MODELS[name]
    if kind == S.GRID_VORONOI:
        # as test_binding_describe.py judges a Voronoi model: the reference samples a cell's density at points of
        # the bounding box Voro++ gives it, the host driver at points of the box of its own clipping of the same
        # cell, so the sampled densities differ in their last digits; every other field is equal bit for bit
        # (the sites among them, which the six samplers drew)
        assert [k for k, _ in diffs] in ([], ["media.rho"]), diffs
        np.testing.assert_allclose(b["media.rho"], a["media.rho"], rtol=1e-12, atol=0)
    else:
        assert diffs == []
    assert a["grid.kind"][0] == kind and a["grid.ncells"][0] == ncells
    assert list(a["sources.geom_kind"]) == sources
    assert a["media.rho"].sum() > 0 and a["sources.lumtot"].sum() > 0 and a["instruments.n"][0] >= 1


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", ["free_shell", "free_ttauri", "free_torus", "free_cone"])
def test_binding_describes_the_sources_of_the_dust_free_models(harness, tmp_path, name):
    """the four kinds no dusty fixture has as a source: the parameter rows and, for the torus and the cone, the
    first words of their geom_table rows"""
    ski = B._ski(name, tmp_path)
    ours, binding = str(tmp_path / "driver.bin"), str(tmp_path / "binding.bin")
    S.Simulation(ski).describe(ours)
    r = subprocess.run([harness, ski, binding, str(tmp_path)], capture_output=True, text=True, timeout=850)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = D.read(ours), D.read(binding)
    assert D.differences(a, b) == []
    t = a.get("sources.geom_table", [])  # a NULL table is written as an empty record
    assert (len(t) > 0) == (name in ("free_torus", "free_cone"))
    if len(t):
        assert len(t) == 202 and 0 < t[0] < 1 and t[3] > 0 and not t[4:].any()
        assert (t[1] == -1.0) == (name == "free_torus")
