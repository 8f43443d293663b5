"""Imported particle dust (SPHDustDistribution) on the host: every fixture model loads (before the feature: "unsupported
dust distribution"); node, leaf, particle and Voronoi cell counts equal the reference's log excerpt; ds_cellprops
written by sim.write equals the reference's (tests/golden/ref_particles, `skirt -t 1 -i`), row for row; the refusals
give their messages; input_path and the default folder both find the particle file. ds_convergence is not compared
here: the "actual" values in that file are column densities walked by the engine, so sim.write produces it only with
a device attached, and tests/test_gpu_particles.py compares it with the reference's file, text for text, on all seven
models (as tests/test_gpu_geom.py does for its kinds). No GPU."""
import gzip
import os
import re
import shutil

import numpy as np
import pytest

import skirt_amd as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
PART = os.path.join(GOLD, "particles")
# model -> (grid kind, cells)
MODELS = {"part_oct": (S.GRID_OCTREE, 2479), "part_oct_neg": (S.GRID_OCTREE, 2451), "part_oct_bary": (S.GRID_OCTREE, 2458),
          "part_cart": (S.GRID_CARTESIAN, 4096), "part_vor": (S.GRID_VORONOI, 1343), "part_vor_dd": (S.GRID_VORONOI, 400),
          "part_few": (S.GRID_OCTREE, 519)}


def _ski(name):
    return os.path.join(GOLD, "ski", name + ".ski")


def _ref(name, what):
    path = os.path.join(GOLD, "ref_particles", "%s_s4357_%s" % (name, what))
    if os.path.exists(path):
        return open(path, "rb").read()
    return gzip.open(path + ".gz", "rb").read()


def _load(name, **kw):
    return S.Simulation(_ski(name), seed=4357, input_path=PART, **kw)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_loads_with_the_reference_counts(name):
    kind, ncells = MODELS[name]
    sim = _load(name)
    assert sim.info.grid_kind == kind and sim.info.ncells == ncells and sim.info.ncomp == 1
    log = _ref(name, "log_excerpt.txt").decode()
    info = sim.particle_info()
    assert int(re.search(r"particles ignored: (\d+)", log).group(1)) == info["nignored"]
    assert int(re.search(r"containing dust: (\d+)", log).group(1)) == info["nparticles"]
    if kind == S.GRID_OCTREE:
        assert int(re.search(r"Total number of nodes: (\d+)", log).group(1)) == sim.info.nnodes
        assert int(re.search(r"Total number of leaves: (\d+)", log).group(1)) == sim.info.ncells
    if kind == S.GRID_VORONOI:
        assert int(re.search(r"tesselation with (\d+) cells", log).group(1)) == sim.info.ncells
    assert info["mass_interface"] == (name != "part_oct_neg")
    rho = sim.density()
    assert rho.shape == (ncells, 1) and np.all(rho >= 0) and rho.sum() > 0 and np.all(np.isfinite(rho))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_cell_properties_equal_the_reference(tmp_path, name):
    """every row of ds_cellprops (volume, density, mass fraction, optical depth) as the reference printed it; the
    four statistics lines that close the reference's file are not written for these grid kinds (test_geom_host.py)"""
    sim = _load(name)
    sim.write(str(tmp_path / "o"))
    got = open(str(tmp_path / "o_ds_cellprops.dat"), "rb").read().split(b"\n")
    ref = [l for l in _ref(name, "ds_cellprops.dat").split(b"\n")
           if not re.match(rb"# (smallest|largest|average|90 %)", l)]
    assert len(got) == len(ref) == MODELS[name][1] + 5
    if MODELS[name][0] == S.GRID_VORONOI:
        # as test_geom_host.py judges a Voronoi model: a volume may differ in its last printed digit (the host clips
        # convex cells, Voro++ builds them its own way); every other column token for token
        g = [l.split() for l in got if l and not l.startswith(b"#")]
        r = [l.split() for l in ref if l and not l.startswith(b"#")]
        assert [t[1:] for t in g] == [t[1:] for t in r]
        np.testing.assert_allclose([float(t[0]) for t in g], [float(t[0]) for t in r], rtol=1e-5)
        np.testing.assert_allclose(sum(float(t[0]) for t in g), sum(float(t[0]) for t in r), rtol=1e-12)
        return
    assert got == ref


def _cell_boxes(sim, tmp_path):
    """the boxes of a tree model's cells, in cell order, from the descriptors the driver uploads"""
    import descriptors as D
    path = str(tmp_path / "d.bin")
    sim.describe(path)
    d = D.read(path)
    box, cell = d["grid.box"].reshape(-1, 6), d["grid.cellnumber"]
    out = np.zeros((sim.info.ncells, 6))
    out[cell[cell >= 0]] = box[cell >= 0]
    return out


@pytest.mark.parametrize("name", ["part_oct", "part_oct_bary", "part_oct_neg"])
def test_interface_densities_are_mass_in_box_over_volume(tmp_path, name):
    """with the mass-in-box interface (no negative mass) a tree cell's density is massInBox(cell) / volume exactly,
    also on a barycentric tree; with negative masses the densities are sampled, so they are not"""
    sim = _load(name)
    b = _cell_boxes(sim, tmp_path)
    mass, _ = sim.particle_mass_in_box(b)
    want = mass / ((b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1]) * (b[:, 5] - b[:, 2]))
    rho = sim.density()[:, 0]
    assert np.count_nonzero(rho) > 2000
    if name == "part_oct_neg":
        assert not np.array_equal(rho, want)
        np.testing.assert_allclose(rho.sum(), want.sum(), rtol=0.2)  # (sampled: the same cloud, roughly)
    else:
        assert np.array_equal(rho, want)


def _variant(tmp_path, name, old, new, count=1):
    text = open(_ski(name)).read()
    assert text.count(old) >= count
    p = tmp_path / "v.ski"
    p.write_text(text.replace(old, new))
    return str(p)


def test_input_path_and_the_default_folder_find_the_file(tmp_path):
    """the fixture models name their file "../particles/<file>": from the default folder (the .ski file's own,
    tests/golden/ski) and from the input folder the fixtures were made with (tests/golden/particles) alike"""
    b = _load("part_few")
    a = S.Simulation(_ski("part_few"), seed=4357)  # the default folder
    np.testing.assert_array_equal(a.density(), b.density())
    with pytest.raises(S.SkirtError, match=r"Could not open the SPH gas particles data file .*few\.dat"):
        S.Simulation(_ski("part_few"), input_path=str(tmp_path / "nowhere" / "deeper"))
    # a plain name: found beside the .ski file by default, in input_path when given, nowhere else
    plain = _variant(tmp_path, "part_few", 'filename="../particles/few.dat"', 'filename="few.dat"')
    with pytest.raises(S.SkirtError, match=r"Could not open the SPH gas particles data file .*few\.dat"):
        S.Simulation(plain)
    c = S.Simulation(plain, seed=4357, input_path=PART)
    np.testing.assert_array_equal(c.density(), b.density())
    shutil.copy(os.path.join(PART, "few.dat"), str(tmp_path / "few.dat"))
    d = S.Simulation(plain, seed=4357)
    np.testing.assert_array_equal(d.density(), b.density())
    e = S.Simulation(_variant(tmp_path, "part_few", 'filename="../particles/few.dat"',
                              'filename="%s"' % os.path.join(PART, "few.dat")), seed=4357, input_path=str(tmp_path))
    np.testing.assert_array_equal(e.density(), b.density())


def test_a_short_or_broken_file_names_itself(tmp_path):
    (tmp_path / "m.ski").write_text(open(_ski("part_few")).read().replace("../particles/few.dat", "few.dat"))
    (tmp_path / "few.dat").write_text("# header\n1 2 3 4 5\n")
    with pytest.raises(S.SkirtError, match=r"required value\(s\) on text line are missing in .*few\.dat"):
        S.Simulation(str(tmp_path / "m.ski"))
    (tmp_path / "few.dat").write_text("1 2 3 4 5 x 7\n")
    with pytest.raises(S.SkirtError, match=r"not formatted as a floating point number in .*few\.dat"):
        S.Simulation(str(tmp_path / "m.ski"))
    (tmp_path / "few.dat").write_text("# nothing\n\n")
    with pytest.raises(S.SkirtError, match=r"few\.dat holds no particle"):
        S.Simulation(str(tmp_path / "m.ski"))


REFUSALS = [
    ("part_oct", 'dustFraction="0.3"', 'dustFraction="0"', "The dust fraction should be positive"),
    ("part_oct", "<OctTreeDustGrid", "<ParticleTreeDustGrid", "ParticleTreeDustGrid is not supported"),
    ("part_vor", 'distribution="SPHParticles"', 'distribution="DustTesselation"', "DustTesselation is not supported"),
    ("part_vor", 'distribution="SPHParticles"', 'distribution="File"', "File is not supported"),
]


@pytest.mark.parametrize("name,old,new,message", REFUSALS, ids=[r[3][:24] for r in REFUSALS])
def test_refusals_give_their_messages(tmp_path, name, old, new, message):
    with pytest.raises(S.SkirtError) as e:
        S.Simulation(_variant(tmp_path, name, old, new), input_path=PART)
    assert message in str(e.value)


def test_particle_stars_are_refused(tmp_path):
    text = open(_ski("part_vor")).read()
    a = text.index("<OligoStellarComp")
    b = text.index("</OligoStellarComp>") + len("</OligoStellarComp>")
    p = tmp_path / "s.ski"
    p.write_text(text[:a] + '<SPHStellarComp filename="stars.dat" velocity="false" writeLuminosities="false"/>' + text[b:])
    with pytest.raises(S.SkirtError, match="SPHStellarComp is not supported: its SED family tables"):
        S.Simulation(str(p), input_path=PART)


@pytest.mark.parametrize("grid,dim", [
    ('<Sphere1DDustGrid writeGrid="false" maxR="500 pc"><meshR type="Mesh"><LinMesh numBins="10"/></meshR></Sphere1DDustGrid>', 1),
    ('<Sphere2DDustGrid writeGrid="false" maxR="500 pc"><meshR type="Mesh"><LinMesh numBins="10"/></meshR>'
     '<meshTheta type="Mesh"><LinMesh numBins="8"/></meshTheta></Sphere2DDustGrid>', 2),
    ('<Cylinder2DDustGrid writeGrid="false" maxR="500 pc" minZ="-500 pc" maxZ="500 pc"><meshR type="Mesh">'
     '<LinMesh numBins="10"/></meshR><meshZ type="MoveableMesh"><LinMesh numBins="10"/></meshZ></Cylinder2DDustGrid>', 2),
])
def test_particle_dust_on_a_1d_or_2d_grid_is_refused_in_the_reference_words(tmp_path, grid, dim):
    text = open(_ski("part_few")).read()
    a = text.index("<OctTreeDustGrid")
    b = text.index("/>", a) + 2
    p = tmp_path / "g.ski"
    p.write_text(text[:a] + grid + text[b:])
    with pytest.raises(S.SkirtError, match="The grid dimension %d is lower than the geometry dimension 3" % dim):
        S.Simulation(str(p), input_path=PART)


def test_models_without_particles_have_no_particle_probes():
    sim = S.Simulation(_ski("c1_oligo16"), packages=10)
    with pytest.raises(S.SkirtError, match="no particle dust"):
        sim.particle_info()
