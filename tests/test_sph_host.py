"""Host set-up of the spherical dust grids (Sphere1DDustGrid, Sphere2DDustGrid): .ski parsing, the meshes, the polar
fix-up of Sphere2DDustGrid::setupSelfAfter (exact cosines, the inserted border at pi/2), the reference's errors, and
the cell volumes and densities -- sampled at (direction, r) and (r, theta, phi) positions from the sequential MT19937
stream in the reference's order -- through the written ds_cellprops.dat, which must equal the reference's file
(tests/golden/ref_sph, `skirt -t 1`) byte for byte. No GPU."""
import math
import os
import re

import numpy as np
import pytest

import descriptors as D
import skirt_amd as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
# model -> (grid kind, cells)
MODELS = {"pan_sph1": (4, 20), "pan_sph1_sa": (4, 20), "pan_sph1_log": (4, 20), "pan_sph2": (5, 192),
          "disk_sph2": (5, 120), "pan_sph2_sa": (5, 192), "pan_sph2_cs": (5, 192), "oligo_sph2": (5, 192)}
PC = 3.08567758e16


def _ski(name):
    return os.path.join(GOLD, "ski", name + ".ski")


def _describe(tmp_path, ski, tag):
    path = str(tmp_path / (tag + ".bin"))
    S.Simulation(ski).describe(path)
    return D.read(path)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_loads_and_cell_properties_equal_the_reference(tmp_path, name):
    kind, ncells = MODELS[name]
    sim = S.Simulation(_ski(name), seed=4357)  # the fixtures' seed
    assert (S.GRID_SPHERE1D, S.GRID_SPHERE2D) == (4, 5)
    assert sim.info.grid_kind == kind and sim.info.ncells == ncells and sim.info.nnodes == 0
    rho = sim.density()
    assert rho.shape == (ncells, sim.info.ncomp) and np.all(rho >= 0) and rho.sum() > 0
    ref = os.path.join(GOLD, "ref_sph", name + "_s4357_ds_cellprops.dat")
    writes = 'writeCellProperties="true"' in open(_ski(name)).read()
    assert os.path.exists(ref) == writes
    if writes:
        sim.write(str(tmp_path / "o"))
        assert open(str(tmp_path / "o_ds_cellprops.dat"), "rb").read() == open(ref, "rb").read()


def test_cell_properties_are_pinned_for_both_grids():
    written = [n for n in MODELS if 'writeCellProperties="true"' in open(_ski(n)).read()]
    assert {MODELS[n][0] for n in written} == {4, 5}
    assert "disk_sph2" in written and "pan_sph1_log" in written  # the inserted border, the LogMesh


def test_sphere1d_descriptor_holds_the_borders(tmp_path):
    """skirt_sim_describe: kind 4, nx = N_r with the radial borders in xv, no angular arrays, extent = +-maxR"""
    for name, first_bin in (("pan_sph1", 500.0 / 20), ("pan_sph1_log", 0.02 * 500.0)):
        d = _describe(tmp_path, _ski(name), name)
        assert d["grid.kind"][0] == 4 and d["grid.ncells"][0] == 20 and d["grid.nx"][0] == 20
        assert "grid.yv" not in d and "grid.zv" not in d and "grid.eps" not in d
        xv = d["grid.xv"]
        assert len(xv) == 21 and xv[0] == 0.0 and np.all(np.diff(xv) > 0)
        np.testing.assert_allclose([xv[1], xv[-1]], np.array([first_bin, 500.0]) * PC, rtol=1e-14)
        np.testing.assert_array_equal(d["grid.extent"], np.array([-1, -1, -1, 1, 1, 1]) * (500.0 * PC))
        assert d["media.rho"].shape == (20 * d["media.ncomp"][0],)


def test_sphere2d_descriptor_holds_the_borders_and_the_exact_cosines(tmp_path):
    """kind 5: r borders in xv, the polar borders in zv, their fixed-up cosines (exact 1, 0, -1) in yv,
    eps = 1e-11 maxR, extent = +-maxR"""
    d = _describe(tmp_path, _ski("pan_sph2"), "pan_sph2")
    assert d["grid.kind"][0] == 5 and d["grid.ncells"][0] == 192
    assert d["grid.nx"][0] == 12 and d["grid.ny"][0] == 16 and d["grid.nz"][0] == 16
    xv, cv, tv = d["grid.xv"], d["grid.yv"], d["grid.zv"]
    assert len(xv) == 13 and len(cv) == 17 and len(tv) == 17
    assert xv[0] == 0.0 and np.all(np.diff(xv) > 0) and np.all(np.diff(tv) > 0) and np.all(np.diff(cv) < 0)
    np.testing.assert_allclose(xv[-1], 500.0 * PC, rtol=1e-14)
    np.testing.assert_array_equal(tv, np.array([k * (1.0 / 16) for k in range(17)]) * math.pi)  # LinMesh * pi
    assert cv[0] == 1.0 and cv[8] == 0.0 and cv[16] == -1.0
    assert math.cos(tv[8]) != 0.0 and math.cos(tv[16]) == -1.0  # (cos(pi/2) in f64 is 6e-17: the fix-up made it 0)
    inner = [k for k in range(1, 16) if k != 8]
    np.testing.assert_array_equal(cv[inner], np.cos(tv[inner]))
    assert d["grid.eps"][0] == 1e-11 * (500.0 * PC)
    np.testing.assert_array_equal(d["grid.extent"], np.array([-1, -1, -1, 1, 1, 1]) * (500.0 * PC))
    assert d["media.rho"].shape == (192 * d["media.ncomp"][0],)


def test_nine_polar_bins_become_ten_with_a_border_at_half_pi(tmp_path):
    d = _describe(tmp_path, _ski("disk_sph2"), "disk_sph2")
    assert d["grid.kind"][0] == 5 and d["grid.ncells"][0] == 120
    assert d["grid.nx"][0] == 12 and d["grid.ny"][0] == 10 and d["grid.nz"][0] == 10
    cv, tv = d["grid.yv"], d["grid.zv"]
    assert len(cv) == 11 and len(tv) == 11
    assert tv[5] == math.pi / 2 and cv[5] == 0.0 and cv[0] == 1.0 and cv[10] == -1.0
    lin9 = np.array([k * (1.0 / 9) for k in range(10)]) * math.pi
    np.testing.assert_array_equal(np.delete(tv, 5), lin9)
    np.testing.assert_array_equal(np.delete(cv, 5)[1:-1], np.cos(lin9[1:-1]))
    assert np.all(np.diff(tv) > 0) and np.all(np.diff(cv) < 0)


def _variant(tmp_path, base, tag, pattern, repl):
    text, n = re.subn(pattern, repl, open(_ski(base)).read())
    assert n == 1
    path = str(tmp_path / (tag + ".ski"))
    with open(path, "w") as f:
        f.write(text)
    return path


@pytest.mark.parametrize("base", ["pan_sph1", "pan_sph2"])
@pytest.mark.parametrize("maxr", ["0 pc", "-5 pc"])
def test_non_positive_outer_radius_is_refused_with_the_reference_error(tmp_path, base, maxr):
    path = _variant(tmp_path, base, "maxr", r'maxR="500 pc"', 'maxR="%s"' % maxr)
    with pytest.raises(S.SkirtError, match="The outer radius of the grid should be positive"):
        S.Simulation(path)


def test_two_borders_close_to_half_pi_are_refused_with_the_reference_error(tmp_path):
    """a SymPowMesh with 4 bins and a huge ratio puts borders 1 and 3 within 1e-9 of the middle one"""
    path = _variant(tmp_path, "pan_sph2", "twozero", r'<meshTheta type="Mesh"><LinMesh numBins="16"/>',
                    '<meshTheta type="Mesh"><SymPowMesh numBins="4" ratio="1e11"/>')
    with pytest.raises(S.SkirtError, match="There are multiple grid points very close to pi/2"):
        S.Simulation(path)


def test_polar_meshes_pow_and_sympow_load(tmp_path):
    """PowMesh (no border at pi/2: one is inserted) and SymPowMesh (an even count has its middle border there)"""
    for tag, mesh, ntheta in (("pow", '<PowMesh numBins="8" ratio="3"/>', 9),
                              ("sym", '<SymPowMesh numBins="8" ratio="3"/>', 8)):
        path = _variant(tmp_path, "pan_sph2", tag, r'<meshTheta type="Mesh"><LinMesh numBins="16"/>',
                        '<meshTheta type="Mesh">' + mesh)
        d = _describe(tmp_path, path, tag)
        assert d["grid.nz"][0] == ntheta and d["grid.ncells"][0] == 12 * ntheta
        cv = d["grid.yv"]
        assert np.count_nonzero(cv == 0.0) == 1 and cv[0] == 1.0 and cv[-1] == -1.0 and np.all(np.diff(cv) < 0)
