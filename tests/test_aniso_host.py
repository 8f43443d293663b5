"""Anisotropic emission on the host: the loader (the six geometries, their refusals in the reference's words, the grid
dimension check), the host's launches and emission-peel-off probabilities against the plain-Python restatement of the
reference (tests/aniso_ref.py) on the same deviates, the restatement's own properties (each probability integrates to
1, the generated directions follow it), what the reference's fixtures hold, and the maintainer binding."""
import math
import os
import subprocess

import numpy as np
import pytest

import aniso_ref as A
import geom_ref as R
import oracle_lib as O
import skirt_files as F
import skirt_amd as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKI = os.path.join(REPO, "tests", "golden", "ski")
REF = os.path.join(REPO, "tests", "golden", "ref_aniso")
PC = 3.08567758e16
TAG = 0x4c4e4331  # SKIRT_LAUNCHES_TAG
FREE = {"free_netzer": "netzer", "free_surface": "surface", "free_sphebg": "sphebg", "free_cubbg": "cubbg",
        "free_patch": "patch", "free_laser": "laser"}
DUSTY = {"netzer_torus_sph2": ("i30", "i80"), "netzer_cone_cyl": ("i30", "i80"), "surface_shell_sph1": ("i30",),
         "sphebg_plummer_cart": ("i30",), "cubbg_oct": ("i30",)}
R0_PC = 300.0
N = 20000


def _ski(name):
    return os.path.join(SKI, name + ".ski")


def _with(tmp_path, base, old, new, name="m.ski"):
    text = open(_ski(base)).read()
    assert text.count(old) == 1, (base, old)
    path = tmp_path / name
    path.write_text(text.replace(old, new))
    return str(path)


# ---------------------------------------------------------------- loader
def test_constants():
    assert (S.GEOM_NETZER, S.GEOM_STELLARSURFACE, S.GEOM_SPHEBACKGROUND, S.GEOM_CUBBACKGROUND, S.GEOM_SOLARPATCH,
            S.GEOM_LASER) == (10, 11, 12, 13, 14, 15)
    assert [A.KIND_CODE[k] for k in A.KINDS] == [10, 11, 12, 13, 14, 15]
    header = open(os.path.join(REPO, "include", "skirt_mcrt.h")).read()
    assert "SKIRT_GEOM_NETZER = 10" in header and "SKIRT_GEOM_LASER = 15" in header


@pytest.mark.parametrize("name", list(FREE) + list(DUSTY))
def test_every_model_loads(name):
    sim = S.Simulation(_ski(name))
    assert sim.info.ninstruments == (5 if name in FREE else len(DUSTY[name]))
    assert (sim.info.ncells > 0) == (name in DUSTY)


@pytest.mark.parametrize("element,message", [
    ('<StellarSurfaceGeometry radius="0 pc"/>', "the stellar radius rstar should be positive"),
    ('<StellarSurfaceGeometry radius="-1 pc"/>', "the stellar radius rstar should be positive"),
    ('<SpheBackgroundGeometry radius="0 pc"/>', "the background sphere radius rbg should be positive"),
    ('<CubBackgroundGeometry extent="0 pc"/>', "the background cube extent h should be positive"),
    ('<SolarPatchGeometry radius="-2 pc"/>', "the patch radius Rmax should be positive"),
])
def test_bad_parameters_fail_with_the_reference_messages(tmp_path, element, message):
    with pytest.raises(S.SkirtError, match=message):
        S.Simulation(_with(tmp_path, "free_netzer", "<NetzerAccretionDiskGeometry/>", element))


@pytest.mark.parametrize("kind", A.KINDS)
def test_each_kind_is_refused_as_a_dust_component(tmp_path, kind):
    element = A.element(kind, 100)
    dust = '<TorusGeometry expon="1" index="1" openAngle="50 deg" minRadius="50 pc" maxRadius="400 pc" anisoRadius="false" cutRadius="0 pc"/>'
    with pytest.raises(S.SkirtError, match=element[1:element.index("Geometry") + 8] + " is not supported for dust components"):
        S.Simulation(_with(tmp_path, "netzer_torus_sph2", dust, element))


GRIDS = {
    1: '<Sphere1DDustGrid writeGrid="false" maxR="500 pc"><meshR type="Mesh"><LinMesh numBins="20"/></meshR></Sphere1DDustGrid>',
    2: ('<Cylinder2DDustGrid writeGrid="false" maxR="500 pc" minZ="-500 pc" maxZ="500 pc"><meshR type="Mesh"><LinMesh '
        'numBins="12"/></meshR><meshZ type="MoveableMesh"><LinMesh numBins="16"/></meshZ></Cylinder2DDustGrid>'),
}
SPH2 = ('<Sphere2DDustGrid writeGrid="false" maxR="500 pc"><meshR type="Mesh"><LinMesh numBins="12"/></meshR><meshTheta '
        'type="Mesh"><LinMesh numBins="16"/></meshTheta></Sphere2DDustGrid>')


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("dim_grid", [1, 2])
def test_grid_dimension_check(tmp_path, kind, dim_grid):
    """DustGrid::setupSelfBefore for the new sources: a CubBackground (3) on a Cylinder2D grid (2), a Netzer disk (2)
    on a Sphere1D grid (1), ... fail in the reference's words; a grid of the geometry's dimension or more loads"""
    path = _with(tmp_path, "netzer_torus_sph2", "<NetzerAccretionDiskGeometry/>", A.element(kind, 100))
    text = open(path).read()
    assert text.count(SPH2) == 1
    open(path, "w").write(text.replace(SPH2, GRIDS[dim_grid]))
    dim = A.DIMENSION[kind]
    if dim > dim_grid:
        with pytest.raises(S.SkirtError,
                           match="The grid dimension %d is lower than the geometry dimension %d" % (dim_grid, dim)):
            S.Simulation(path)
    else:
        assert S.Simulation(path).info.ncells == (20 if dim_grid == 1 else 192)


def test_a_refusal_leaves_the_setup_stream_alone(tmp_path):
    """the octree of cubbg_oct draws from the setup's generator; a model refused before it (a cube on a Cylinder2D
    grid; a bad radius) changes nothing for the next load: the same cells and densities as a first load's"""
    first = S.Simulation(_ski("cubbg_oct"))
    bad = _with(tmp_path, "netzer_cone_cyl", "<NetzerAccretionDiskGeometry/>", '<CubBackgroundGeometry extent="600 pc"/>')
    with pytest.raises(S.SkirtError, match="The grid dimension 2 is lower than the geometry dimension 3"):
        S.Simulation(bad)
    with pytest.raises(S.SkirtError, match="should be positive"):
        S.Simulation(_with(tmp_path, "cubbg_oct", 'extent="600 pc"', 'extent="0 pc"', "z.ski"))
    again = S.Simulation(_ski("cubbg_oct"))
    assert again.info.ncells == first.info.ncells and again.info.nnodes == first.info.nnodes
    np.testing.assert_array_equal(again.density(), first.density())


def test_voronoi_grids_are_refused(tmp_path):
    """the engine's own limit: no anisotropic event kernel for Voronoi grids"""
    text = open(_ski("vor_pan")).read()
    start = text.index("<PlummerGeometry")
    end = text.index("/>", start) + 2
    path = tmp_path / "v.ski"
    path.write_text(text[:start] + "<NetzerAccretionDiskGeometry/>" + text[end:])
    with pytest.raises(S.SkirtError, match="anisotropic sources are not supported on a VoronoiDustGrid"):
        S.Simulation(str(path))


# ---------------------------------------------------------------- the host against the restatement
def _restated(kind, r0, n, seed, first):
    pos, dirs, draws = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=np.int64)
    for i in range(n):
        u = R.PhiloxStream(O.philox, seed, TAG, first + i)
        pos[i] = A.position(kind, r0, u)
        dirs[i] = A.direction(kind, r0, tuple(pos[i]), u)
        draws[i] = u.draws
    return pos, dirs, draws


@pytest.mark.parametrize("name", list(FREE))
def test_host_launches_equal_the_restatement_on_the_same_deviates(name):
    kind = FREE[name]
    sim = S.Simulation(_ski(name))
    r0 = R0_PC * PC
    pos, dirs, draws = sim.launches(0, N, seed=77, first=5)
    wpos, wdirs, wdraws = _restated(kind, r0, N, 77, 5)
    np.testing.assert_array_equal(draws, wdraws)
    assert np.all(wdraws == A.DRAWS[kind])
    np.testing.assert_allclose(pos, wpos, rtol=1e-9, atol=1e-12 * r0)
    np.testing.assert_allclose(dirs, wdirs, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose((dirs ** 2).sum(axis=1), 1.0, rtol=0, atol=1e-14)
    # probabilityForDirection: at the launched positions towards other packets' directions, and at the adversarial
    # positions towards the adversarial directions
    pairs = [(tuple(wpos[i]), tuple(wdirs[N - 1 - i])) for i in range(N)] if kind != "laser" else []
    pairs += [(p, k) for p in A.adversarial_positions(kind, r0) for k in A.adversarial_directions(kind)]
    got = sim.emission_probability(0, [p for p, _ in pairs], [k for _, k in pairs])
    want = np.array([A.probability(kind, r0, p, k) for p, k in pairs])
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    assert np.all(got >= 0)
    # every launch direction has a positive probability at its own position (Netzer: but for kz = 0 exactly)
    own = sim.emission_probability(0, wpos, wdirs)
    assert np.all(own > 0)


def test_streams_depend_on_seed_and_packet_only():
    sim = S.Simulation(_ski("free_cubbg"))
    a = sim.launches(0, 64, seed=3, first=0)
    b = sim.launches(0, 32, seed=3, first=32)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x[32:], y)
    c = sim.launches(0, 64, seed=4, first=0)
    assert not np.any(a[1] == c[1])


def test_isotropic_kinds_launch_through_the_same_interface():
    sim = S.Simulation(_ski("torus_oct"))  # a Plummer star
    pos, dirs, draws = sim.launches(0, 2000)
    assert np.all(draws == 5)
    np.testing.assert_allclose((dirs ** 2).sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert abs(dirs.mean(axis=0)).max() < 0.05
    np.testing.assert_array_equal(sim.emission_probability(0, pos, dirs), 1.0)
    with pytest.raises(S.SkirtError, match="no stellar component 3"):
        sim.launches(3, 4)


@pytest.mark.parametrize("name,position,message", [
    ("free_surface", (0.0, 0.0, 1 + 3e-8), "not defined for positions not on the stellar surface"),
    ("free_sphebg", (1 - 3e-8, 0.0, 0.0), "not defined for positions not on the background sphere"),
    ("free_cubbg", (0.5, 0.5, 0.5), "not defined for positions not on the background cube"),
    ("free_cubbg", (1.0, 1 + 1e-6, 0.0), "not defined for positions not on the background cube"),
    ("free_netzer", (0.0, 1e-20, 0.0), "not defined for positions besides the origin"),
    ("free_laser", (1e-20, 0.0, 0.0), "not defined for positions besides the origin"),
])
def test_a_position_off_the_surface_is_an_error(name, position, message):
    sim = S.Simulation(_ski(name))
    r0 = R0_PC * PC
    p = [c * r0 for c in position]
    with pytest.raises(S.SkirtError, match=message):
        sim.emission_probability(0, [[0.0, 0.0, 0.0] if name in ("free_netzer", "free_laser") else _on(name, r0), p],
                                 [[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    with pytest.raises(A.FatalError, match=message):
        A.probability(FREE[name], r0, tuple(p), (1.0, 0.0, 0.0))


def _on(name, r0):
    return [r0, 0.0, 0.0]


def test_positions_within_the_tolerance_are_accepted():
    sim = S.Simulation(_ski("free_surface"))
    r0 = R0_PC * PC
    got = sim.emission_probability(0, [[0.0, 0.0, r0 * (1 + 3e-9)]], [[0.0, 0.0, 1.0]])
    np.testing.assert_allclose(got, 4.0 * (1 + 3e-9), rtol=1e-12)
    cube = S.Simulation(_ski("free_cubbg"))
    got = cube.emission_probability(0, [[-r0 * (1 + 3e-9), 0.2 * r0, 0.1 * r0]], [[1.0, 0.0, 0.0]])
    np.testing.assert_allclose(got, 4.0, rtol=1e-12)


# ---------------------------------------------------------------- properties of the restatement
def _sphere_quadrature(nt=200, nphi=256):
    """Gauss-Legendre in cos theta, uniform in phi: (directions [m, 3], weights summing to 1)"""
    c, w = np.polynomial.legendre.leggauss(nt)
    phi = (np.arange(nphi) + 0.5) * 2 * math.pi / nphi
    cc, pp = np.meshgrid(c, phi, indexing="ij")
    s = np.sqrt(1 - cc ** 2)
    k = np.stack([s * np.cos(pp), s * np.sin(pp), cc], axis=-1).reshape(-1, 3)
    return k, (np.repeat(w, nphi) / (2 * nphi))


@pytest.mark.parametrize("kind", [k for k in A.KINDS if k != "laser"])
def test_probability_integrates_to_one(kind):
    """the mean of probabilityForDirection over the unit sphere is 1, at every kind of position. The integrands have
    a kink (cos theta' = 0, the Netzer law's sign), where both rules are of second order: 200 Gauss-Legendre nodes
    in cos theta and 256 midpoints in phi leave an error of a few 1e-5, so the bound is 1e-4"""
    k, w = _sphere_quadrature()
    r0 = 2.5
    for p in A.adversarial_positions(kind, r0)[:9] + [A.position(kind, r0, R.PhiloxStream(O.philox, 1, TAG, 3))]:
        total = sum(wi * A.probability(kind, r0, tuple(p), tuple(ki)) for ki, wi in zip(k, w))
        assert abs(total - 1.0) < 1e-4, (kind, p, total)


@pytest.mark.parametrize("kind", [k for k in A.KINDS if k != "laser"])
def test_generated_directions_follow_the_probability(kind):
    """at a fixed position: the histogram of cos(angle to the emission axis) of 40000 generated directions against
    the probability integrated over each of 10 bins; chi^2 with 9 degrees of freedom below 33.7 (p = 1e-4)"""
    r0 = 2.5
    pos = {"netzer": (0.0, 0.0, 0.0), "surface": (0.6 * r0, 0.0, 0.8 * r0), "sphebg": (0.0, -0.6 * r0, -0.8 * r0),
           "cubbg": (0.3 * r0, r0, -0.2 * r0), "patch": (0.5 * r0, 0.1 * r0, 0.0)}[kind]
    axis = {"netzer": (0.0, 0.0, 1.0), "surface": (0.6, 0.0, 0.8), "sphebg": (0.0, 0.6, 0.8), "cubbg": (0.0, -1.0, 0.0),
            "patch": (0.0, 0.0, 1.0)}[kind]
    n = 40000
    mu = np.zeros(n)
    for i in range(n):
        u = R.PhiloxStream(O.philox, 5, TAG, i)
        d = A.direction(kind, r0, pos, u)
        mu[i] = d[0] * axis[0] + d[1] * axis[1] + d[2] * axis[2]
    edges = np.linspace(-1.0, 1.0, 11)
    counts, _ = np.histogram(mu, bins=edges)
    # the probability depends on mu alone: p(mu) from directions in the plane of the axis, integrated per bin (Simpson)
    e1 = np.cross(axis, (0.3, 0.5, 0.7))
    e1 /= np.linalg.norm(e1)
    expected = np.zeros(10)
    for b in range(10):
        xs = np.linspace(edges[b], edges[b + 1], 201)
        ps = [A.probability(kind, r0, pos, tuple(x * np.array(axis) + math.sqrt(max(0.0, 1 - x * x)) * e1)) for x in xs]
        h = xs[1] - xs[0]
        expected[b] = n * 0.5 * (h / 3) * (ps[0] + ps[-1] + 4 * sum(ps[1:-1:2]) + 2 * sum(ps[2:-1:2]))
    assert abs(expected.sum() - n) < 1e-3 * n
    lit = expected > 0
    assert counts[~lit].sum() == 0
    chi2 = float((((counts - expected) ** 2)[lit] / expected[lit]).sum())
    print("%s: chi^2 %.2f over %d bins" % (kind, chi2, lit.sum()))
    assert chi2 < 33.7


def test_netzer_table_and_law():
    thetav, Xv = A.netzer_table()
    assert len(thetav) == 401 and Xv[0] == 0.0 and Xv[-1] == 1.0 and all(b >= a for a, b in zip(Xv, Xv[1:]))
    assert abs(Xv[200] - 0.5) < 1e-15
    np.testing.assert_allclose(A.netzer_probability(1.0), 18. / 7.)
    np.testing.assert_allclose(A.netzer_probability(-1.0), 18. / 7.)
    assert abs(A.netzer_probability(0.0)) == 0.0
    assert A.probability("laser", 0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)) == math.inf
    assert A.probability("laser", 0.0, (0.0, 0.0, 0.0), (0.0, 1e-8, 1.0 - 2.0 ** -53)) == 0.0  # theta = acos(kz) > 0
    assert A.probability("laser", 0.0, (0.0, 0.0, 0.0), (0.6, 0.0, 0.8)) == 0.0


# ---------------------------------------------------------------- what the reference's fixtures hold
def test_reference_fluxes_of_the_disk_follow_its_law():
    """free_netzer in the reference itself: every packet leaves the origin, so the printed fluxes are in the ratio of
    the probabilities (to the 9 printed digits)"""
    f = {i: F.read_text_table(os.path.join(REF, "free_netzer_s4357_sed%d_sed.dat" % i))[0, 1] for i in (30, 60, 120)}
    P = {i: A.netzer_probability(math.cos(math.radians(i))) for i in (30, 60, 120)}
    np.testing.assert_allclose(f[30] / f[60], P[30] / P[60], rtol=2e-9)
    np.testing.assert_allclose(f[60] / f[120], P[60] / P[120], rtol=2e-9)
    laser = [F.read_text_table(os.path.join(REF, "free_laser_s4357_sed%d_sed.dat" % i))[0, 1] for i in (30, 60, 120)]
    assert laser == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("name", list(DUSTY))
def test_reference_seds_have_enough_entries_to_score(name):
    """the GPU test scores at least 15 SED entries per dusty model: the reference's own tables hold at least that many
    above the 1e-12 max cut in columns that vary from seed to seed (scattered, dust, total; not the direct and
    transparent fluxes of a source at the origin, which every seed prints alike)"""
    count = 0
    for i in DUSTY[name]:
        t = F.read_text_table(os.path.join(REF, "%s_s4357_%s_sed.dat" % (name, i)))
        assert t.shape[0] == 10
        cols = [1, 3, 4, 5, 7] if name.startswith("netzer") else range(1, t.shape[1])
        for c in cols:
            count += int(np.count_nonzero(t[:, c] > 1e-12 * t[:, c].max()))
    print("%s: %d entries" % (name, count))
    assert count >= 15


# ---------------------------------------------------------------- the maintainer binding
@pytest.mark.skipif(not os.path.isdir(os.environ.get("SKIRT_REFERENCE", "/root/reference")),
                    reason="needs the reference's headers (build container)")
def test_binding_compiles_with_the_six_kinds(tmp_path):
    src = open(os.path.join(REPO, "integration", "GpuPhotonEngine.cpp")).read()
    for cls, kind in (("NetzerAccretionDiskGeometry", "NETZER"), ("StellarSurfaceGeometry", "STELLARSURFACE"),
                      ("SpheBackgroundGeometry", "SPHEBACKGROUND"), ("CubBackgroundGeometry", "CUBBACKGROUND"),
                      ("SolarPatchGeometry", "SOLARPATCH"), ("LaserGeometry", "LASER")):
        assert "dynamic_cast<%s*>" % cls in src and "SKIRT_GEOM_" + kind in src
    r = subprocess.run(["bash", os.path.join(REPO, "integration", "check_binding.sh"), str(tmp_path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
