"""The six closed-form geometries (Shell, Gamma, Gaussian, TTauriDisk, Torus, ConicalShell) on the device: the launch
routine's positions against the host's on the same per-packet streams; the set-up's density sampling on the device
against the host's; the engine's outputs against the reference's (tests/golden/ref_geom, `skirt -t 1`) statistically,
by the rules of test_gpu_parity / test_gpu_sph; and the invariants that need no checker (shards, repeated runs, packet
counts). The CPU oracle knows none of these kinds (it treats them as Plummer), so nothing here calls it."""
import gzip
import os

import numpy as np
import pytest

import skirt_files as F
import skirt_amd as S
import test_gpu_parity as P
from skirt_amd.sharding import shard_slice

pytestmark = pytest.mark.gpu
REF = os.path.join(P.GOLD, "ref_geom")
PC = 3.08567758e16
FREE = ["free_shell", "free_gamma", "free_gauss", "free_ttauri", "free_torus", "free_cone"]
ISRF_MODELS = ["shell_sph1", "torus_sph2", "cone_cyl", "ttauri_cyl", "gauss_gamma_cart"]
# the outer scale of each stellar component (geom_ref.outer_scale), in pc
SCALE = {"free_shell": 400.0, "free_gamma": 100.0, "free_gauss": 100.0, "free_ttauri": 400.0, "free_torus": 400.0,
         "free_cone": 400.0, "gauss_gamma_cart": 100.0}


def _run(name, packages=0.0, dust=False, seed=0):
    sim = S.Simulation(P.ski(name), packages=packages, seed=seed)
    sim.attach(0)
    sim.run_stellar()
    if dust:
        sim.run_dust()
    sim.fetch()
    return sim


# ---------------------------------------------------------------- positions: the launch routine against the host
@pytest.mark.parametrize("name,comp", [(n, 0) for n in FREE] + [("gauss_gamma_cart", 0), ("gauss_gamma_cart", 1)])
def test_device_positions_equal_host_positions(name, comp):
    n = 20000
    sim = S.Simulation(P.ski(name))
    host, hdraws = sim.positions(comp, n, seed=9, first=7)
    dev, ddraws = sim.positions(comp, n, seed=9, first=7, device=0)
    same = hdraws == ddraws
    flips = int(n - same.sum())
    print("%s[%d]: %.3f draws per position, %d packets with another draw count" % (name, comp, hdraws.mean(), flips))
    # a device ulp may flip a rejection (the cone's, the polar Box-Muller's): at most 1e-4 of the packets
    assert flips <= 1e-4 * n
    np.testing.assert_allclose(dev[same], host[same], rtol=1e-9, atol=1e-12 * SCALE[name] * PC)
    assert np.all(np.isfinite(dev)) and np.abs(dev).max() > 0


def test_existing_kinds_keep_their_positions_on_the_device():
    """the same interface over a Plummer component: the launch routine's existing branch"""
    sim = S.Simulation(P.ski("torus_oct"))
    host, hdraws = sim.positions(0, 5000)
    dev, ddraws = sim.positions(0, 5000, device=0)
    np.testing.assert_array_equal(hdraws, ddraws)
    np.testing.assert_allclose(dev, host, rtol=1e-9, atol=1e-12 * 100 * PC)


# ---------------------------------------------------------------- set-up on the device
@pytest.mark.parametrize("name", ["torus_oct", "vor_geoms"])
def test_device_setup_matches_host(name):
    host = S.Simulation(P.ski(name), seed=4357)
    dev = S.Simulation(P.ski(name), seed=4357, setup_device=0)
    assert dev.info.ncells == host.info.ncells and dev.info.nnodes == host.info.nnodes
    rh, rd = host.density(), dev.density()
    assert rh.shape == rd.shape and rh.sum() > 0
    np.testing.assert_allclose(rd, rh, rtol=1e-13, atol=0)


# ---------------------------------------------------------------- against the reference's outputs
@pytest.mark.parametrize("name", ["shell_sph1", "torus_sph2"])
def test_ds_convergence_equals_the_reference_file(tmp_path, name):
    sim = _run(name, packages=10, seed=4357)
    sim.write(str(tmp_path / "gpu"))
    got = open(str(tmp_path / "gpu_ds_convergence.dat")).read()
    assert got == open(os.path.join(REF, name + "_s4357_ds_convergence.dat")).read()
    assert "surface density" in got


def _ref_isrf(tmp_path, name):
    """the reference's ds_isrf.dat (gauss_gamma_cart's 4096-cell table is committed gzipped)"""
    path = os.path.join(REF, name + "_s4357_ds_isrf.dat")
    if os.path.exists(path):
        return path
    out = str(tmp_path / (name + "_ref_ds_isrf.dat"))
    with gzip.open(path + ".gz", "rb") as f, open(out, "wb") as o:
        o.write(f.read())
    return out


_RUNS = {}


def _seed_runs(tmp_path, name):
    """P._engine_seed_runs, once per model for the two tests that read it"""
    if name not in _RUNS:
        _RUNS[name] = P._engine_seed_runs(tmp_path, name)
    return _RUNS[name]


def _score_sed(name, seds, ref_sed, cols):
    infl = np.sqrt(1 + 1.0 / len(P.SEEDS))
    scored = 0
    for col in cols:
        m, s = seds[:, :, col].mean(axis=0), seds[:, :, col].std(axis=0, ddof=1)
        good = (s > 0) & (m > 1e-12 * m.max()) & (s <= 0.5 * m)
        zz = (ref_sed[good, col] - m[good]) / (s[good] * infl)
        print("%s SED column %d: max |z| %.2f over %d" % (name, col, np.abs(zz).max() if len(zz) else 0.0, len(zz)))
        assert np.all(np.abs(zz) < P.Z_BOUND), (col, zz)
        P._assert_aggregate(zz, "SED column %d" % col)
        scored += len(zz)
    return scored


@pytest.mark.parametrize("name", ISRF_MODELS)
def test_engine_matches_reference_statistically(tmp_path, name):
    """test_gpu_sph.test_engine_matches_reference_statistically: per-wavelength ISRF sums and every SED column as
    z-scores against the spread of 16 independently seeded engine runs on the reference's grid (seed 4357)"""
    J, seds = _seed_runs(tmp_path, name)
    Jsum = J.sum(axis=1)
    ref_J = P._isrf_sums(_ref_isrf(tmp_path, name))
    ref_sed = F.read_text_table(os.path.join(REF, name + "_s4357_i30_sed.dat"))
    infl = np.sqrt(1 + 1.0 / len(P.SEEDS))
    m, s = Jsum.mean(axis=0), Jsum.std(axis=0, ddof=1)
    good = (s > 0) & (s <= 0.5 * m)
    z = (ref_J[good] - m[good]) / (s[good] * infl)
    print("%s ISRF sums: max |z| %.2f over %d" % (name, np.abs(z).max(), len(z)))
    assert len(z) >= 5
    assert np.all(np.abs(z) < P.Z_BOUND), z
    P._assert_aggregate(z, "ISRF sums")
    _score_sed(name, seds, ref_sed, (1, 2, 3, 4, 5, 6))


@pytest.mark.parametrize("name,instr", [("torus_oct", "i30"), ("vor_geoms", "a")])
def test_models_without_isrf_match_reference_seds(tmp_path, name, instr):
    """torus_oct and vor_geoms write no ISRF: every SED column by the same rule (as test_gpu_sph scores oligo_sph2),
    the set-up at the fixture's seed 4357, the photon streams at the 16 seeds"""
    seds = []
    for k, sd in enumerate(P.SEEDS):
        r = S.Simulation(P.ski(name), seed=4357)
        r.set_photon_seed(sd)
        r.attach(0)
        r.run_stellar()
        r.run_dust()
        r.fetch()
        prefix = str(tmp_path / ("%s_%d" % (name, k)))
        r.write(prefix)
        seds.append(F.read_text_table(prefix + "_%s_sed.dat" % instr))
    seds = np.array(seds)
    ref_sed = F.read_text_table(os.path.join(REF, "%s_s4357_%s_sed.dat" % (name, instr)))
    assert seds.shape[1:] == ref_sed.shape
    scored = _score_sed(name, seds, ref_sed, range(1, ref_sed.shape[1]))
    assert scored >= (3 if name == "vor_geoms" else 15)


@pytest.mark.parametrize("name", ISRF_MODELS)
def test_per_cell_mean_intensity_matches_reference(tmp_path, name):
    """test_gpu_sph.test_per_cell_mean_intensity_matches_reference: pools of cells at 0.25, mean z^2 and the tail"""
    J, _ = _seed_runs(tmp_path, name)
    ref = P._isrf_cells(_ref_isrf(tmp_path, name), J.shape[1])
    K = len(P.SEEDS)
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


@pytest.mark.parametrize("name", FREE)
def test_dust_free_frames_match_reference(tmp_path, name):
    """the launch positions seen through the instruments: both frames of a dust-free model as pools of pixels
    (P._pools at 0.25 over the 16 seeds), z-scored against the reference's total.fits with the per-cell test's
    bounds; at least 30 pools per frame"""
    frames = {"face": [], "edge": []}
    for k, sd in enumerate(P.SEEDS):
        r = S.Simulation(P.ski(name), seed=4357)
        r.set_photon_seed(sd)
        r.attach(0)
        r.run_stellar()
        r.fetch()
        assert r.stats()["packets"] == 4000
        prefix = str(tmp_path / ("%s_%d" % (name, k)))
        r.write(prefix)
        for f in frames:
            frames[f].append(F.read_fits("%s_%s_total.fits" % (prefix, f)).astype(np.float64).reshape(-1))
    K = len(P.SEEDS)
    nu = K - 1
    infl = np.sqrt(1 + 1.0 / K)
    for f, runs in frames.items():
        A = np.array(runs)
        ref = F.read_fits(os.path.join(REF, "%s_s4357_%s_total.fits" % (name, f))).astype(np.float64).reshape(-1)
        assert A.shape == (K, 1024) and ref.shape == (1024,)
        z = []
        for p in P._pools(A, 0.25):
            tot = A[:, p].sum(axis=1)
            m, s = tot.mean(), tot.std(ddof=1)
            if s > 0:
                z.append((ref[p].sum() - m) / (s * infl))
        z = np.array(z)
        chi2 = float(np.mean(z ** 2))
        tail = int(np.count_nonzero(np.abs(z) > 4))
        print("%s %s frame: %d pools, mean z^2 %.3f (t_%d: %.3f), |z|>4: %d" % (name, f, len(z), chi2, nu, nu / (nu - 2), tail))
        assert len(z) >= 30
        assert chi2 < 1.35 * nu / (nu - 2), chi2
        assert tail <= max(3, 0.005 * len(z)), tail


# ---------------------------------------------------------------- invariants without a checker
@pytest.mark.parametrize("name", ["torus_sph2", "gauss_gamma_cart"])
def test_three_shards_sum_to_the_unsharded_run(name):
    packages = 2000
    full = _run(name, packages=packages, seed=4357)
    st = full.stats()
    lit = np.count_nonzero(full.labs().sum(axis=0) > 0)
    assert lit >= 5 and st["packets"] == packages * lit  # packages x the wavelengths with luminosity
    assert st["segments_fill"] > 0 and st["segments_peel"] > 0 and st["absorb_adds"] > 0
    parts = []
    for r in range(3):
        sim = S.Simulation(P.ski(name), packages=packages, seed=4357)
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


def test_second_run_equals_a_fresh_run():
    """shell_sph1 with its dust phases (one self-absorption cycle, dust emission) twice on one engine"""
    name = "shell_sph1"
    sim = S.Simulation(P.ski(name), packages=1000)
    sim.attach(0)
    for _ in range(2):
        sim.zero_tallies()
        sim.run_stellar()
        sim.run_dust()
        sim.fetch()
    fresh = _run(name, packages=1000, dust=True)
    assert len(fresh.selfabs_totals()) > 0 and fresh.labs_dust().sum() > 0
    assert fresh.instrument(0)[1][3:5].sum() > 0  # the dust emission reached the instrument
    P._assert_equal_runs(sim, fresh)
