"""Host side of the six closed-form geometries (ShellGeometry, GammaGeometry, GaussianGeometry, TTauriDiskGeometry,
TorusGeometry, ConicalShellGeometry): every fixture model loads; the cell densities -- sampled from the sequential
MT19937 stream in the reference's order -- equal the reference's ds_cellprops.dat (tests/golden/ref_geom, `skirt -t
1`); the Voronoi model's sites, drawn by the six host samplers from the same stream, give the reference's cells; the
host's position templates equal the plain-Python restatement (geom_ref.py) on the same Philox deviates, over every
branch of gln / gexp and of the polar sampling; the reference's setup errors; the load-time refusal of a torus that
admits (almost) no position. No GPU."""
import json
import os

import numpy as np
import pytest

import geom_ref as R
import oracle_lib as O
import skirt_amd as S
from golden import bench_digest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
PC = 3.08567758e16
TAG = 0x504f5331  # SKIRT_POSITIONS_TAG
# model -> (grid kind or None, cells)
DUSTY = {"shell_sph1": (S.GRID_SPHERE1D, 20), "torus_sph2": (S.GRID_SPHERE2D, 192), "torus_oct": (S.GRID_OCTREE, 1632),
         "cone_cyl": (S.GRID_CYLINDER2D, 192), "ttauri_cyl": (S.GRID_CYLINDER2D, 192),
         "gauss_gamma_cart": (S.GRID_CARTESIAN, 4096), "vor_geoms": (S.GRID_VORONOI, 600)}
FREE = ["free_shell", "free_gamma", "free_gauss", "free_ttauri", "free_torus", "free_cone"]


def _ski(name):
    return os.path.join(GOLD, "ski", name + ".ski")


def _ref(name, what):
    return os.path.join(GOLD, "ref_geom", "%s_s4357_%s" % (name, what))


def test_geometry_constants():
    assert (S.GEOM_PLUMMER, S.GEOM_EXPDISK, S.GEOM_SERSIC, S.GEOM_POINT) == (0, 1, 2, 3)
    assert (S.GEOM_SHELL, S.GEOM_GAMMA, S.GEOM_GAUSSIAN, S.GEOM_TTAURIDISK, S.GEOM_TORUS, S.GEOM_CONICALSHELL) == \
        (4, 5, 6, 7, 8, 9)
    assert {"skirt_mcrt_sample_positions", "skirt_sim_sample_positions"} <= set(S.ABI_SYMBOLS)
    assert all(hasattr(S.lib(), s) for s in ("skirt_mcrt_sample_positions", "skirt_sim_sample_positions"))


@pytest.mark.parametrize("name", FREE)
def test_dust_free_model_loads(name):
    sim = S.Simulation(_ski(name), seed=4357)
    assert not sim.info.has_dust and sim.info.nlambda == 1 and sim.info.ninstruments == 3 and sim.info.npp == 4000


@pytest.mark.parametrize("name", sorted(DUSTY))
def test_model_loads_and_cell_properties_equal_the_reference(tmp_path, name):
    kind, ncells = DUSTY[name]
    sim = S.Simulation(_ski(name), seed=4357)  # the fixtures' seed
    assert sim.info.grid_kind == kind and sim.info.ncells == ncells
    rho = sim.density()
    assert rho.shape == (ncells, sim.info.ncomp) and np.all(rho >= 0) and np.all(rho.sum(0) > 0) and np.all(np.isfinite(rho))
    sim.write(str(tmp_path / "o"))
    got, ref = str(tmp_path / "o_ds_cellprops.dat"), _ref(name, "ds_cellprops.dat")
    if kind in (S.GRID_SPHERE1D, S.GRID_SPHERE2D, S.GRID_CYLINDER2D):
        assert open(got, "rb").read() == open(ref, "rb").read()
        return
    # the larger tables are committed as digests (tests/golden/bench_digest.py, as the benchmark models' are): equal
    # SHA-256 values of the rows mean files equal byte for byte, but for the four statistics lines that close the
    # reference's file, which the host writes only for the grid kinds above
    have, want = bench_digest.cellprops_digest(got), json.load(open(_ref(name, "ds_cellprops_digest.json")))
    assert have["rows"] == want["rows"] == ncells
    if kind == S.GRID_VORONOI:
        # as the benchmark's Voronoi model is judged (test_oracle_golden.py): the host tessellation clips convex
        # cells, Voro++ builds them its own way, so a volume can differ in its last printed digit; every other
        # column is equal token for token, which pins the 600 sites -- and with them the six samplers' draws
        assert have["sha256_columns"][1:] == want["sha256_columns"][1:]
        np.testing.assert_allclose(have["sums"][0], want["sums"][0], rtol=1e-12)
        return
    assert have["sha256"] == want["sha256"]


def test_every_new_kind_is_a_dust_component_and_a_source(tmp_path):
    import descriptors as D
    path = str(tmp_path / "d.bin")
    S.Simulation(_ski("vor_geoms"), seed=4357).describe(path)
    assert D.read(path)["media.ncomp"][0] == 6
    kinds = set()
    for name in FREE + ["gauss_gamma_cart"]:
        S.Simulation(_ski(name), seed=4357).describe(path)
        kinds |= set(int(k) for k in D.read(path)["sources.geom_kind"])
    assert kinds == {4, 5, 6, 7, 8, 9}


# ---------------------------------------------------------------- positions against the restatement
def _geoms():
    """(id, geometry in pc, its .ski element) over expon in {0, 1, 2, 3, 3.0005} and index in {0, 1}: p - 2 = 1 - q'
    runs gln / gexp at q' = 3, 2, 1, 0 (the logarithm) and -0.0005 (the series), the index both polar branches"""
    out = []
    for p in (0, 1, 2, 3, 3.0005):
        out.append(("shell-p%s" % p, dict(kind="shell", rmin=50.0, rmax=400.0, p=float(p)),
                    '<ShellGeometry minRadius="50 pc" maxRadius="400 pc" expon="%s"/>' % p))
        for q in (0, 1):
            out.append(("torus-p%s-q%d" % (p, q),
                        dict(kind="torus", p=float(p), q=float(q), Delta=np.deg2rad(50.0), rmin=50.0, rmax=400.0),
                        '<TorusGeometry expon="%s" index="%d" openAngle="50 deg" minRadius="50 pc" maxRadius="400 pc" '
                        'anisoRadius="false" cutRadius="0 pc"/>' % (p, q)))
            out.append(("cone-p%s-q%d" % (p, q),
                        dict(kind="cone", p=float(p), q=float(q), DeltaIn=np.deg2rad(20.0), DeltaOut=np.deg2rad(50.0),
                             rmin=50.0, rmax=400.0),
                        '<ConicalShellGeometry expon="%s" index="%d" inAngle="20 deg" outAngle="50 deg" '
                        'minRadius="50 pc" maxRadius="400 pc" anisoRadius="false" cutRadius="0 pc"/>' % (p, q)))
    out.append(("torus-aniso", dict(kind="torus", p=1.0, q=0.0, Delta=np.deg2rad(50.0), rmin=50.0, rmax=400.0, rani=True,
                                    rcut=30.0),
                '<TorusGeometry expon="1" index="0" openAngle="50 deg" minRadius="50 pc" maxRadius="400 pc" '
                'anisoRadius="true" cutRadius="30 pc"/>'))
    for gamma in (0, 1, 2.5):
        out.append(("gamma-%s" % gamma, dict(kind="gamma", b=100.0, gamma=float(gamma)),
                    '<GammaGeometry scale="100 pc" gamma="%s"/>' % gamma))
    out.append(("gaussian", dict(kind="gaussian", sigma=100.0, q=0.5), '<GaussianGeometry dispersion="100 pc" flattening="0.5"/>'))
    out.append(("ttauri", dict(kind="ttauri", Rinn=20.0, Rout=400.0, Rd=100.0, zd=10.0),
                '<TTauriDiskGeometry minRadius="20 pc" maxRadius="400 pc" radialScale="100 pc" axialScale="10 pc"/>'))
    return out


GEOMS = _geoms()
N_POS = 300


def _free_ski(tmp_path, element):
    text = open(_ski("free_shell")).read()
    start = text.index("<ShellGeometry")
    end = text.index("/>", start) + 2
    path = tmp_path / "g.ski"
    path.write_text(text[:start] + element + text[end:])
    return str(path)


def _in_metres(g):
    g = dict(g)
    for k in ("rmin", "rmax", "rcut", "b", "sigma", "Rinn", "Rout", "Rd", "zd"):
        if k in g:
            g[k] = g[k] * PC
    return g


@pytest.mark.parametrize("gid,geom,element", GEOMS, ids=[g[0] for g in GEOMS])
def test_host_positions_equal_the_restatement_on_the_same_deviates(tmp_path, gid, geom, element):
    sim = S.Simulation(_free_ski(tmp_path, element))
    pos, draws = sim.positions(0, N_POS, seed=77, first=5)
    g = R.setup(_in_metres(geom))
    want = np.zeros((N_POS, 3))
    wdraws = np.zeros(N_POS, dtype=np.int64)
    for i in range(N_POS):
        u = R.PhiloxStream(O.philox, 77, TAG, 5 + i)
        want[i] = R.position(g, u)
        wdraws[i] = u.draws
    np.testing.assert_array_equal(draws, wdraws)
    np.testing.assert_allclose(pos, want, rtol=1e-12, atol=1e-12 * R.outer_scale(g))
    # every position lies where the geometry has density
    assert all(R.density(g, *p) > 0 for p in want)
    if geom["kind"] == "cone":
        assert wdraws.mean() > 3  # the loop rejects: the polar law covers |cos theta| < sin(outAngle), the cone less
    if geom["kind"] in ("shell", "gamma"):
        assert np.all(wdraws == 3)


def test_streams_depend_on_seed_and_packet_only(tmp_path):
    sim = S.Simulation(_ski("free_cone"))
    a, da = sim.positions(0, 64, seed=3, first=0)
    b, db = sim.positions(0, 32, seed=3, first=32)
    np.testing.assert_array_equal(a[32:], b)
    np.testing.assert_array_equal(da[32:], db)
    c, _ = sim.positions(0, 64, seed=4, first=0)
    assert not np.any(a == c)


def test_existing_kinds_sample_through_the_same_interface():
    sim = S.Simulation(_ski("gauss_gamma_cart"))
    with pytest.raises(S.SkirtError, match="no stellar component 2"):
        sim.positions(2, 4)
    plummer = S.Simulation(_ski("torus_oct"))
    pos, draws = plummer.positions(0, 1000)
    assert np.all(draws == 3)
    r = np.sqrt((pos ** 2).sum(1)) / (100 * PC)
    assert 0.9 < np.median(r) / 1.3048 < 1.1  # PlummerGeometry: half-mass radius 1.3048 c


# ---------------------------------------------------------------- surface densities (the normalizations)
def test_normalizations_use_the_reference_surface_densities(tmp_path):
    def nf_ratio(name, comp_kind):
        """cell densities scale with the normalization factor tau / (Sigma kappa): compare two optical depths"""
        text = open(_ski(name)).read()
        assert comp_kind in text
        out = []
        for tau in ("1", "0.7", "3"):
            p = tmp_path / ("n%s.ski" % tau)
            p.write_text(text.replace('opticalDepth="1"', 'opticalDepth="%s"' % tau).replace('opticalDepth="0.7"', 'opticalDepth="%s"' % tau))
            out.append(S.Simulation(str(p), seed=4357).density().sum())
        return out

    a = nf_ratio("shell_sph1", "RadialDustCompNormalization")
    np.testing.assert_allclose(a[2] / a[0], 3.0, rtol=1e-12)
    # the restatement's surface densities against closed forms and quadrature of its own density
    g = R.setup(dict(kind="shell", rmin=2.0, rmax=7.0, p=2.0))
    np.testing.assert_allclose(R.Sigmar(g), g["A"] * (1 / 2.0 - 1 / 7.0), rtol=1e-13)
    g = R.setup(dict(kind="gaussian", sigma=3.0, q=0.5))
    zs = np.linspace(-40, 40, 4001)  # the whole z axis to 26 dispersions: the rectangle rule is exact to rounding
    np.testing.assert_allclose(R.SigmaZ(g), sum(R.density(g, 0, 0, z) for z in zs) * (zs[1] - zs[0]), rtol=1e-9)
    assert R.SigmaZ(R.setup(dict(kind="ttauri", Rinn=1.0, Rout=5.0, Rd=2.0, zd=0.1))) == 0.0
    assert R.Sigmar(R.setup(dict(kind="gamma", b=1.0, gamma=1.0))) == float("inf")
    np.testing.assert_allclose(R.Sigmar(R.setup(dict(kind="gamma", b=2.0, gamma=0.0))), 1 / (2 * np.pi * 4 * 2), rtol=1e-15)


def _dust_ski(tmp_path, element, norm=None):
    text = open(_ski("cone_cyl")).read()
    start = text.index("<ConicalShellGeometry")
    end = text.index("/>", start) + 2
    text = text[:start] + element + text[end:]
    if norm:
        a = text.index("<DustMassDustCompNormalization")
        text = text[:a] + norm + text[text.index("/>", a) + 2:]
    path = tmp_path / "d.ski"
    path.write_text(text)
    return str(path)


def test_normalizations_by_the_wrong_symmetry_fail_as_in_the_reference(tmp_path):
    """{FaceOn,EdgeOn}DustCompNormalization dynamic_cast to AxGeometry, RadialDustCompNormalization to SpheGeometry"""
    shell = '<ShellGeometry minRadius="50 pc" maxRadius="400 pc" expon="2"/>'
    torus = '<TorusGeometry expon="1" index="1" openAngle="50 deg" minRadius="50 pc" maxRadius="400 pc"/>'
    with pytest.raises(S.SkirtError, match="Geometry is not axisymmetric"):
        S.Simulation(_dust_ski(tmp_path, shell, '<EdgeOnDustCompNormalization wavelength="0.55 micron" opticalDepth="1"/>'))
    with pytest.raises(S.SkirtError, match="Geometry is not spherically symmetric"):
        S.Simulation(_dust_ski(tmp_path, torus, '<RadialDustCompNormalization wavelength="0.55 micron" opticalDepth="1"/>'))
    # a torus has SigmaZ = 0 and a gamma model with gamma >= 1 an infinite Sigmar: the reference divides by them
    sim = S.Simulation(_dust_ski(tmp_path, torus, '<FaceOnDustCompNormalization wavelength="0.55 micron" opticalDepth="1"/>'))
    rho = sim.density()
    assert np.all(np.isinf(rho[rho > 0])) and np.any(rho > 0)


# ---------------------------------------------------------------- setup errors
BAD = [
    ('<ShellGeometry minRadius="0 pc" maxRadius="400 pc" expon="2"/>', "the inner radius of the shell should be positive"),
    ('<ShellGeometry minRadius="50 pc" maxRadius="50 pc" expon="2"/>',
     "the outer radius of the shell should be larger than the inner radius"),
    ('<ShellGeometry minRadius="50 pc" maxRadius="400 pc" expon="-1"/>', "the power law exponent p should be positive"),
    ('<GammaGeometry scale="0 pc" gamma="1"/>', "the scale length b should be positive"),
    ('<GammaGeometry scale="10 pc" gamma="3"/>', "the central density slope gamma should be between 0 and 3"),
    ('<GaussianGeometry dispersion="0 pc" flattening="0.5"/>', "the dispersion parameter sigma should be positive"),
    ('<GaussianGeometry dispersion="10 pc" flattening="1.5"/>', "the flattening parameter q should be between 0 and 1"),
    ('<TTauriDiskGeometry minRadius="0 pc" maxRadius="400 pc" radialScale="100 pc" axialScale="10 pc"/>',
     "the inner radius of the disk should be positive"),
    ('<TTauriDiskGeometry minRadius="20 pc" maxRadius="20 pc" radialScale="100 pc" axialScale="10 pc"/>',
     "the outer radius of the disk must be larger than the inner radius"),
    ('<TTauriDiskGeometry minRadius="20 pc" maxRadius="400 pc" radialScale="0 pc" axialScale="10 pc"/>',
     "the radial scale length Rd should be positive"),
    ('<TTauriDiskGeometry minRadius="20 pc" maxRadius="400 pc" radialScale="100 pc" axialScale="0 pc"/>',
     "the axial scale height zd should be positive"),
    ('<TorusGeometry expon="-1" index="1" openAngle="50 deg" minRadius="50 pc" maxRadius="400 pc"/>',
     "The radial power law exponent p of the torus should be positive"),
    ('<TorusGeometry expon="1" index="-1" openAngle="50 deg" minRadius="50 pc" maxRadius="400 pc"/>',
     "The polar index q of the torus should be positive"),
    ('<TorusGeometry expon="1" index="1" openAngle="-5 deg" minRadius="50 pc" maxRadius="400 pc"/>',
     "The half opening angle of the torus should be positive"),
    ('<TorusGeometry expon="1" index="1" openAngle="50 deg" minRadius="0 pc" maxRadius="400 pc"/>',
     "The minimum radius of the torus should be positive"),
    ('<TorusGeometry expon="1" index="1" openAngle="50 deg" minRadius="50 pc" maxRadius="40 pc"/>',
     "The maximum radius of the torus should be larger than the minimum radius"),
    ('<TorusGeometry expon="1" index="1" openAngle="50 deg" minRadius="50 pc" maxRadius="400 pc" anisoRadius="true"/>',
     "The inner cutoff radius of the torus should be positive"),
    ('<ConicalShellGeometry expon="-1" index="1" inAngle="20 deg" outAngle="50 deg" minRadius="50 pc" maxRadius="400 pc"/>',
     "The radial power law exponent p of the conical shell should be positive"),
    ('<ConicalShellGeometry expon="1" index="-1" inAngle="20 deg" outAngle="50 deg" minRadius="50 pc" maxRadius="400 pc"/>',
     "The polar index q of the conical shell should be positive"),
    ('<ConicalShellGeometry expon="1" index="1" inAngle="-2 deg" outAngle="50 deg" minRadius="50 pc" maxRadius="400 pc"/>',
     "The inner angle of the conical shell should be positive"),
    ('<ConicalShellGeometry expon="1" index="1" inAngle="50 deg" outAngle="20 deg" minRadius="50 pc" maxRadius="400 pc"/>',
     "the outer angle of the shell should be larger than the inner angle"),
    ('<ConicalShellGeometry expon="1" index="1" inAngle="20 deg" outAngle="50 deg" minRadius="0 pc" maxRadius="400 pc"/>',
     "The minimum radius of the conical shell should be positive"),
    ('<ConicalShellGeometry expon="1" index="1" inAngle="20 deg" outAngle="50 deg" minRadius="50 pc" maxRadius="50 pc"/>',
     "The maximum radius of the conical shell should be larger than the minimum radius"),
    ('<ConicalShellGeometry expon="1" index="1" inAngle="20 deg" outAngle="50 deg" minRadius="50 pc" maxRadius="400 pc" '
     'anisoRadius="true" cutRadius="0 pc"/>', "The inner cutoff radius of the torus should be positive"),
]


@pytest.mark.parametrize("element,message", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_parameters_fail_with_the_reference_messages(tmp_path, element, message):
    with pytest.raises(S.SkirtError) as e:
        S.Simulation(_free_ski(tmp_path, element))
    assert message in str(e.value)


def test_restatement_raises_the_reference_messages():
    with pytest.raises(ValueError, match="the inner radius of the shell should be positive"):
        R.setup(dict(kind="shell", rmin=0.0, rmax=1.0, p=2.0))
    with pytest.raises(ValueError, match="the outer angle of the shell should be larger than the inner angle"):
        R.setup(dict(kind="cone", p=1.0, q=1.0, DeltaIn=0.5, DeltaOut=0.2, rmin=1.0, rmax=2.0))


@pytest.mark.parametrize("element", [
    # an anisotropic inner radius cut at or beyond the outer radius: no radius is left
    '<TorusGeometry expon="1" index="1" openAngle="50 deg" minRadius="50 pc" maxRadius="400 pc" anisoRadius="true" cutRadius="400 pc"/>',
    '<ConicalShellGeometry expon="1" index="1" inAngle="20 deg" outAngle="50 deg" minRadius="50 pc" maxRadius="400 pc" anisoRadius="true" cutRadius="500 pc"/>',
    # a cone of 0.01 deg between its angles: fewer than 1 in 1000 candidates
    '<ConicalShellGeometry expon="1" index="0" inAngle="20 deg" outAngle="20.01 deg" minRadius="50 pc" maxRadius="400 pc"/>',
])
def test_a_geometry_that_admits_no_position_is_refused_at_load(tmp_path, element):
    """the reference would spin in generatePosition; the engine's loops end at 2^16 attempts, and the loader refuses a
    torus or cone whose acceptance (estimated on a private stream) is below 1e-3, so no loaded model comes near"""
    with pytest.raises(S.SkirtError, match="fewer than 1 in 1000 candidate positions"):
        S.Simulation(_free_ski(tmp_path, element))
    with pytest.raises(S.SkirtError, match="fewer than 1 in 1000 candidate positions"):
        S.Simulation(_dust_ski(tmp_path, element))


def test_the_refusal_leaves_the_setup_stream_alone(tmp_path):
    """the acceptance estimate draws from a stream of its own: the cell densities of a torus model equal the
    reference's (test_model_loads_and_cell_properties_equal_the_reference), and a thin but admissible cone loads"""
    thin = ('<ConicalShellGeometry expon="1" index="0" inAngle="20 deg" outAngle="21 deg" minRadius="50 pc" '
            'maxRadius="400 pc"/>')
    sim = S.Simulation(_free_ski(tmp_path, thin))
    pos, draws = sim.positions(0, 200)
    assert draws.min() >= 3 and draws.mean() > 30 and np.all(draws % 3 == 0)
