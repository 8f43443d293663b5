"""The spherical dust grids (Sphere1DDustGrid, Sphere2DDustGrid) on the GPU: the trace kernel's spherical walks
(skirt_amd/csrc/device/sph_walk.hpp in Grid<SKIRT_GRID_SPHERE1D> and Grid<SKIRT_GRID_SPHERE2D>), the event kernel's
cell lookups and cell sources, and every phase, against

1. the plain-Python restatements of Sphere1DDustGrid::path and Sphere2DDustGrid::path (sph_ref.py): column densities
   along the CPU logic test's rays, rtol 1e-9 (the project's engine-against-CPU tolerance), exactly 0 where the path
   crosses no cell;
2. the reference's own outputs (`skirt -t 1`, tests/golden/ref_sph): ds_convergence as text, and the statistical
   checks of test_gpu_parity.py with the same seeds, bounds and masks (the CPU oracle does not know these grids, so
   there is no same-stream comparison);
3. invariants that need no checker: shards sum to the whole, a second run equals a fresh one, the counts."""
import os

import numpy as np
import pytest

import descriptors as D
import skirt_files as F
import skirt_amd as S
import sph_ref as R
import test_gpu_parity as P
from skirt_amd.sharding import shard_slice

pytestmark = pytest.mark.gpu
REF = os.path.join(P.GOLD, "ref_sph")
ALL = ["pan_sph1", "pan_sph1_sa", "pan_sph1_log", "pan_sph2", "disk_sph2", "pan_sph2_sa", "pan_sph2_cs"]
WALK = {"pan_sph1": 7, "pan_sph1_sa": 7, "pan_sph2": 8, "pan_sph2_sa": 8, "disk_sph2": 8}
GRID = {"pan_sph1": (20, 0), "pan_sph2": (12, 16)}  # N_r, N_theta


def _run(name, packages=0.0, dust=False, seed=0):
    sim = S.Simulation(P.ski(name), packages=packages, seed=seed)
    sim.attach(0)
    sim.run_stellar()
    if dust:
        sim.run_dust()
    sim.fetch()
    return sim


# ---------------------------------------------------------------- the walks against the restatements
@pytest.fixture(scope="module")
def rays_pc():
    """the CPU logic test's rays: 2,000 of the random ones and every explicit case (pc)"""
    return R.all_rays(2000)


def _want(d, rho, rays):
    rv, rmax = d["grid.xv"].tolist(), float(d["grid.extent"][3])
    if d["grid.kind"][0] == S.GRID_SPHERE1D:
        return [R.column1(rv, rmax, rho, r) for r in rays.tolist()]
    thv, cv = d["grid.zv"].tolist(), d["grid.yv"].tolist()
    return [R.column2(rv, thv, cv, rmax, rho, r) for r in rays.tolist()]


def test_ray_set_has_empty_and_crossing_paths_on_the_cpu(rays_pc):
    """the restatement alone: more than 100 of the rays cross no cell and more than 100 cross at least one, on the
    test grids of both kinds (checked again on the models' own grids below)"""
    unit = [1.0] * 200
    for rv in R.grids1().values():
        w = [R.column1(rv, R.RMAX, unit, r) for r in rays_pc.tolist()]
        assert sum(x is None for x in w) > 100 and sum(x is not None for x in w) > 100
    for rv, thv, cv in R.grids2().values():
        w = [R.column2(rv, thv, cv, R.RMAX, unit, r) for r in rays_pc.tolist()]
        assert sum(x is None for x in w) > 100 and sum(x is not None for x in w) > 100


@pytest.mark.parametrize("name", ["pan_sph1", "pan_sph2", "disk_sph2"])
def test_column_densities_equal_the_restatement(tmp_path, rays_pc, name):
    sim = S.Simulation(P.ski(name), packages=100)
    dump = str(tmp_path / "d.bin")
    sim.describe(dump)
    d = D.read(dump)
    rho = sim.density().sum(axis=1).tolist()
    rays = rays_pc.copy()
    rays[:, :3] *= R.PC
    want = _want(d, rho, rays)
    empty = np.array([w is None for w in want])
    assert empty.sum() > 100 and (~empty).sum() > 100
    sim.attach(0)
    got = sim.column_densities(rays)
    print("%s: %d rays, %d cross no cell, largest column %.3e kg/m2" % (name, len(rays), empty.sum(), got.max()))
    assert np.all(got[empty] == 0.0)
    np.testing.assert_allclose(got[~empty], np.array([w for w in want if w is not None]), rtol=1e-9, atol=0)
    sim.run_stellar()  # (stats() names the walk of the last phase: 100 packages per wavelength)
    st = sim.stats()
    assert st["map_level"] == -1 and st["grid_walk"] == WALK[name]


def test_setup_device_keeps_the_host_sampling():
    """Simulation(setup_device=N) with these grids samples the densities on the host (the device sampler draws in
    boxes): the same densities, bit for bit, as without it"""
    for name in ("pan_sph1_log", "disk_sph2"):
        a = S.Simulation(P.ski(name), setup_device=0).density()
        b = S.Simulation(P.ski(name)).density()
        assert a.tobytes() == b.tobytes() and a.sum() > 0


# ---------------------------------------------------------------- against the reference's outputs
@pytest.mark.parametrize("name", ["pan_sph1", "disk_sph2"])
def test_ds_convergence_equals_the_reference_file(tmp_path, name):
    sim = _run(name, packages=10)
    sim.write(str(tmp_path / "gpu"))
    got = open(str(tmp_path / "gpu_ds_convergence.dat")).read()
    assert got == open(os.path.join(REF, name + "_s4357_ds_convergence.dat")).read()
    assert "surface density" in got
    for out in ("ds_isrf", "ds_cellprops", "ds_crossed", "i30_sed"):
        assert os.path.getsize(str(tmp_path / ("gpu_%s.dat" % out))) > 0
    assert os.path.getsize(str(tmp_path / "gpu_i30_total.fits")) > 0


@pytest.mark.parametrize("name", ALL)
def test_engine_matches_reference_statistically(tmp_path, name):
    """test_gpu_parity.test_engine_matches_reference_statistically for the spherical models: per-wavelength ISRF
    sums and every SED column as z-scores against the spread of 16 independently seeded engine runs"""
    J, seds = P._engine_seed_runs(tmp_path, name)
    Jsum = J.sum(axis=1)
    ref_J = P._isrf_sums(os.path.join(REF, name + "_s4357_ds_isrf.dat"))
    ref_sed = F.read_text_table(os.path.join(REF, name + "_s4357_i30_sed.dat"))
    infl = np.sqrt(1 + 1.0 / len(P.SEEDS))
    m, s = Jsum.mean(axis=0), Jsum.std(axis=0, ddof=1)
    good = (s > 0) & (s <= 0.5 * m)
    z = (ref_J[good] - m[good]) / (s[good] * infl)
    print("%s ISRF sums: max |z| %.2f over %d" % (name, np.abs(z).max(), len(z)))
    assert len(z) >= 5
    assert np.all(np.abs(z) < P.Z_BOUND), z
    P._assert_aggregate(z, "ISRF sums")
    for col in (1, 2, 3, 4, 5, 6):  # total, direct, scattered, dust, dust scattered, transparent
        m, s = seds[:, :, col].mean(axis=0), seds[:, :, col].std(axis=0, ddof=1)
        good = (s > 0) & (m > 1e-12 * m.max()) & (s <= 0.5 * m)
        zz = (ref_sed[good, col] - m[good]) / (s[good] * infl)
        print("%s SED column %d: max |z| %.2f over %d" % (name, col, np.abs(zz).max() if len(zz) else 0.0, len(zz)))
        assert np.all(np.abs(zz) < P.Z_BOUND), (col, zz)
        P._assert_aggregate(zz, "SED column %d" % col)


@pytest.mark.parametrize("name", ["pan_sph1", "pan_sph2", "pan_sph2_sa"])
def test_per_cell_mean_intensity_matches_reference(tmp_path, name):
    """test_gpu_parity.test_per_cell_mean_intensity_matches_reference for the spherical models, with the cylinder
    test's bounds"""
    seeds = [1000 + 37 * k for k in range(16)]
    J, _ = P._engine_seed_runs(tmp_path, name, seeds)
    ref = P._isrf_cells(os.path.join(REF, name + "_s4357_ds_isrf.dat"), J.shape[1])
    K = len(seeds)
    infl = np.sqrt(1 + 1.0 / K)
    z = []
    for ell in range(J.shape[2]):
        for p in P._pools(J[:, :, ell], 0.25):
            tot = J[:, p, ell].sum(axis=1)
            m, s = tot.mean(), tot.std(ddof=1)
            if s > 0:
                z.append((ref[p, ell].sum() - m) / (s * infl))
    z = np.array(z)
    nu = K - 1
    chi2 = float(np.mean(z ** 2))
    tail = int(np.count_nonzero(np.abs(z) > 4))
    print("per-cell J %s: %d pools, mean z^2 %.3f (t_%d: %.3f), |z|>4: %d" % (name, len(z), chi2, nu, nu / (nu - 2),
                                                                             tail))
    assert len(z) > 100
    assert chi2 < 1.35 * nu / (nu - 2), chi2
    assert tail <= max(3, 0.005 * len(z)), tail


def test_two_component_oligo_model_matches_reference_statistically(tmp_path):
    """oligo_sph2 (two stellar and two dust components, three scattering levels): every SED column z-scored with
    the rule of the statistical test above. The fixture ran at seed 4357, so the set-up (the sampled densities)
    uses that seed; the photon streams use the 16 seeds."""
    name = "oligo_sph2"
    seds = []
    for k, sd in enumerate(P.SEEDS):
        r = S.Simulation(P.ski(name), seed=4357)
        r.set_photon_seed(sd)
        r.attach(0)
        r.run_stellar()
        r.fetch()
        prefix = str(tmp_path / ("%s_%d" % (name, k)))
        r.write(prefix)
        seds.append(F.read_text_table(prefix + "_a_sed.dat"))
    seds = np.array(seds)
    ref_sed = F.read_text_table(os.path.join(REF, name + "_s4357_a_sed.dat"))
    assert seds.shape[1:] == ref_sed.shape and ref_sed.shape[0] == 2
    infl = np.sqrt(1 + 1.0 / len(P.SEEDS))
    scored = 0
    for col in range(1, ref_sed.shape[1]):
        m, s = seds[:, :, col].mean(axis=0), seds[:, :, col].std(axis=0, ddof=1)
        good = (s > 0) & (m > 1e-12 * m.max()) & (s <= 0.5 * m)
        zz = (ref_sed[good, col] - m[good]) / (s[good] * infl)
        print("%s SED column %d: z %s" % (name, col, np.round(zz, 2)))
        assert np.all(np.abs(zz) < P.Z_BOUND), (col, zz)
        P._assert_aggregate(zz, "SED column %d" % col)
        scored += len(zz)
    assert scored >= 8  # total, direct, scattered and the scattering levels at both wavelengths


# ---------------------------------------------------------------- invariants without a checker
@pytest.mark.parametrize("name", ["pan_sph1", "pan_sph2"])
def test_three_shards_sum_to_the_unsharded_run(name):
    packages = 2000
    full = _run(name, packages=packages)
    st = full.stats()
    assert st["grid_walk"] == WALK[name] and st["map_level"] == -1
    lit = np.count_nonzero(full.labs().sum(axis=0) > 0)
    assert lit >= 5 and st["packets"] == packages * lit  # packages x the wavelengths with luminosity
    assert st["segments_fill"] > 0 and st["segments_peel"] > 0 and st["absorb_adds"] > 0
    parts = []
    for r in range(3):
        sim = S.Simulation(P.ski(name), packages=packages)
        sim.attach(0)
        sim.set_reducer(lambda tally, ptr, n, stream: None)  # single process: the test sums
        sim.run_stellar_shard(r, 3)
        sim.fetch()
        lo, n = shard_slice(packages, r, 3)
        assert sim.stats()["packets"] == n * lit
        parts.append(sim)
    np.testing.assert_allclose(sum(p.labs() for p in parts), full.labs(), rtol=1e-12, atol=1e-300)
    ff, sf = full.instrument(0)
    np.testing.assert_allclose(sum(p.instrument(0)[1] for p in parts), sf, rtol=1e-12)
    np.testing.assert_allclose(sum(p.instrument(0)[0] for p in parts), ff, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("name", ["pan_sph1_sa", "pan_sph2_sa"])
def test_second_run_equals_a_fresh_run(name):
    """stellar emission, the self-absorption cycles and dust emission twice on one engine: dust-phase cell sources,
    the no-store trace kernel and the cell launches (randomPositionInCell of each grid) included"""
    sim = S.Simulation(P.ski(name), packages=1000)
    sim.attach(0)
    for _ in range(2):
        sim.zero_tallies()
        sim.run_stellar()
        sim.run_dust()
        sim.fetch()
    assert sim.stats()["grid_walk"] == WALK[name]
    fresh = _run(name, packages=1000, dust=True)
    assert len(fresh.selfabs_totals()) > 0 and fresh.labs_dust().sum() > 0
    assert fresh.instrument(0)[1][3:5].sum() > 0  # the dust emission reached the instrument
    P._assert_equal_runs(sim, fresh)


@pytest.mark.parametrize("name", ["pan_sph1", "pan_sph2"])
def test_cells_crossed_histogram_counts_every_fill_and_peel_path(name):
    """set_crossed: each FILL path and each peel-off path counts once, in the bin of its number of segments. In the
    stellar phase with one instrument every emission and every scattering is followed by one peel-off and one FILL
    path (MonteCarloSimulation.cpp:265-301), so the paths are twice the detections. The longest path stays under
    2 N_r + 2 segments (Sphere1D: inward, outward) and 2 (N_r + 1) + 2 (N_theta + 1) + 1 (Sphere2D: a line meets
    each sphere and each cone twice at most)."""
    bins = 256
    sim = S.Simulation(P.ski(name), packages=2000)
    sim.attach(0)
    sim.set_crossed(bins)
    sim.zero_tallies()
    sim.run_stellar()
    sim.fetch()
    st = sim.stats()
    hist = sim.crossed(bins)
    longest = int(np.flatnonzero(hist).max())
    print("%s crossed: paths %d, detects %d, packets %d, longest path %d segments" % (
        name, hist.sum(), st["detects"], st["packets"], longest))
    Nr, Nt = GRID[name]
    assert hist[bins - 1] == 0 and longest < (2 * Nr + 2 if Nt == 0 else 2 * (Nr + 1) + 2 * (Nt + 1) + 1)
    assert int((hist * np.arange(bins, dtype=np.uint64)).sum()) == st["segments_fill"] + st["segments_peel"]
    assert int(hist.sum()) == 2 * st["detects"]
    assert st["detects"] >= st["packets"] > 0
