"""Host set-up of the axisymmetric R-z dust grid (Cylinder2DDustGrid): .ski parsing, the meshes (LogMesh
included), the reference's errors, and the cell volumes and densities -- sampled at (R, phi, z) positions from the
sequential MT19937 stream in the reference's order -- through the written ds_cellprops.dat, which must equal the
reference's file (tests/golden/ref_cyl, `skirt -t 1`) byte for byte. No GPU."""
import os
import re

import numpy as np
import pytest

import descriptors as D
import skirt_amd as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
MODELS = ["pan_cyl", "pan_cyl_sa", "pan_cyl_cs", "disk_cyl", "disk_cyl_log", "oligo_cyl"]
PC = 3.08567758e16


def _ski(name):
    return os.path.join(GOLD, "ski", name + ".ski")


@pytest.mark.parametrize("name", MODELS)
def test_model_loads_and_cell_properties_equal_the_reference(tmp_path, name):
    sim = S.Simulation(_ski(name), seed=4357)  # the fixtures' seed (oligo_cyl.ski keeps oligo_2comp's own)
    assert sim.info.grid_kind == S.GRID_CYLINDER2D == 3
    assert sim.info.ncells == 192 and sim.info.nnodes == 0
    rho = sim.density()
    assert rho.shape == (192, sim.info.ncomp) and np.all(rho >= 0) and rho.sum() > 0
    ref = os.path.join(GOLD, "ref_cyl", name + "_s4357_ds_cellprops.dat")
    writes = 'writeCellProperties="true"' in open(_ski(name)).read()
    assert os.path.exists(ref) == writes
    if writes:
        sim.write(str(tmp_path / "o"))
        assert open(str(tmp_path / "o_ds_cellprops.dat"), "rb").read() == open(ref, "rb").read()


def test_descriptor_holds_the_borders(tmp_path):
    """skirt_sim_describe: kind 3, nx = N_R with the radial borders in xv (xv[0] = 0), nz = N_z with zv"""
    for name, first_bin in (("pan_cyl", 500.0 / 12), ("disk_cyl_log", 0.02 * 500.0)):
        path = str(tmp_path / (name + ".bin"))
        S.Simulation(_ski(name)).describe(path)
        d = D.read(path)
        assert d["grid.kind"][0] == 3 and d["grid.ncells"][0] == 192
        assert d["grid.nx"][0] == 12 and d["grid.nz"][0] == 16 and "grid.yv" not in d
        xv, zv = d["grid.xv"], d["grid.zv"]
        assert len(xv) == 13 and len(zv) == 17 and xv[0] == 0.0
        assert np.all(np.diff(xv) > 0) and np.all(np.diff(zv) > 0)
        np.testing.assert_allclose([xv[1], xv[-1], zv[0], zv[-1]], np.array([first_bin, 500.0, -500.0, 500.0]) * PC,
                                   rtol=1e-14)
        assert d["media.rho"].shape == (192 * d["media.ncomp"][0],)


def _variant(tmp_path, tag, pattern, repl):
    text, n = re.subn(pattern, repl, open(_ski("pan_cyl")).read())
    assert n == 1
    path = str(tmp_path / (tag + ".ski"))
    with open(path, "w") as f:
        f.write(text)
    return path


@pytest.mark.parametrize("tag,pattern,repl,message", [
    ("maxr", r'maxR="500 pc"', 'maxR="0 pc"', "outer radius of the grid should be positive"),
    ("zext", r'minZ="-500 pc" maxZ="500 pc"', 'minZ="500 pc" maxZ="500 pc"', "should be positive in the Z direction"),
    ("logfrac", r'<meshR type="Mesh"><LinMesh numBins="12"/>',
     '<meshR type="Mesh"><LogMesh numBins="12" centralBinFraction="1"/>', "central bin width fraction"),
])
def test_invalid_grids_are_refused_with_the_reference_errors(tmp_path, tag, pattern, repl, message):
    with pytest.raises(S.SkirtError, match=message):
        S.Simulation(_variant(tmp_path, tag, pattern, repl))


def test_log_mesh_belongs_to_the_radial_mesh_only(tmp_path):
    """meshZ is a MoveableMesh; LogMesh is an AnchoredMesh, which the reference's hierarchy does not accept there"""
    path = _variant(tmp_path, "logz", r'<meshZ type="MoveableMesh"><LinMesh numBins="16"/>',
                    '<meshZ type="MoveableMesh"><LogMesh numBins="16" centralBinFraction="0.1"/>')
    with pytest.raises(S.SkirtError, match="unsupported mesh LogMesh"):
        S.Simulation(path)


def test_log_mesh_with_one_bin_is_a_linear_grid(tmp_path):
    path = _variant(tmp_path, "log1", r'<meshR type="Mesh"><LinMesh numBins="12"/>',
                    '<meshR type="Mesh"><LogMesh numBins="1" centralBinFraction="0.3"/>')
    sim = S.Simulation(path)
    assert sim.info.grid_kind == S.GRID_CYLINDER2D and sim.info.ncells == 16
    out = str(tmp_path / "d.bin")
    sim.describe(out)
    np.testing.assert_array_equal(D.read(out)["grid.xv"], [0.0, 500.0 * PC])
