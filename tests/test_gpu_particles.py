"""Imported particle dust (SPHDustDistribution) on the device. The set-up through setup_device=0 -- tree subdivision
and tree cell densities by mass in box (particleMassKernel), sampled densities on Cartesian, tree and Voronoi grids
(particleSampleKernel) -- against the host's, bit for bit; the probes on the adversarial points and boxes of
tests/test_particles_logic.py, with the handed-back count; the photon phases against the oracle on the same Philox
streams; and the engine's outputs against the reference's (tests/golden/ref_particles, `skirt -t 1 -i`) by the
statistic and thresholds of tests/test_gpu_geom.py. Reads nothing outside the repository."""
import gzip
import os
import time

import numpy as np
import pytest

import descriptors as D
import oracle_lib as O
import particles_ref as R
import skirt_files as F
import skirt_amd as S
import test_gpu_geom as G
import test_gpu_parity as P
from parity import DUST_OUTLIERS, STELLAR_OUTLIERS, assert_parity

pytestmark = pytest.mark.gpu
GOLD = P.GOLD
PART = os.path.join(GOLD, "particles")
REF = os.path.join(GOLD, "ref_particles")
MODELS = ["part_oct", "part_oct_neg", "part_oct_bary", "part_cart", "part_vor", "part_vor_dd", "part_few"]


def _ski(name):
    return os.path.join(GOLD, "ski", name + ".ski")


def _load(name, **kw):
    return S.Simulation(_ski(name), input_path=PART, **kw)


def _absolute(tmp_path, name):
    """the model with its particle file named by its full path: what the oracle, which knows no input folder, loads"""
    text = open(_ski(name)).read()
    a = text.index('filename="') + len('filename="')
    b = text.index('"', a)
    p = tmp_path / (name + ".ski")
    p.write_text(text[:a] + os.path.join(PART, text[a:b]) + text[b:])
    return str(p)


# ---------------------------------------------------------------- device set-up against host set-up
@pytest.mark.parametrize("name", MODELS)
def test_device_setup_equals_host_setup(tmp_path, name):
    t0 = time.time()
    host = _load(name, seed=4357)
    t1 = time.time()
    dev = _load(name, seed=4357, setup_device=0)
    t2 = time.time()
    print("%s set-up: host %.3f s, device %.3f s (with the upload and the first kernel's load)" % (name, t1 - t0, t2 - t1))
    assert dev.info.nnodes == host.info.nnodes and dev.info.ncells == host.info.ncells
    assert np.array_equal(dev.density(), host.density())
    assert host.density().sum() > 0
    if host.info.grid_kind == S.GRID_VORONOI:
        host.describe(str(tmp_path / "h.bin"))
        dev.describe(str(tmp_path / "d.bin"))
        assert np.array_equal(D.read(str(tmp_path / "h.bin"))["grid.site"], D.read(str(tmp_path / "d.bin"))["grid.site"])


def test_handed_back_share_of_the_octree_set_up():
    """part_oct's nodes and cells through the probe: how many boxes exceed the merge cap (reported, not bounded)"""
    sim = _load("part_oct", seed=4357)
    P_ = R.Particles(os.path.join(PART, "cloud.dat"), 0.3, 8e4)
    # the octree's node boxes of levels 3 .. 5 over the 1000 pc extent
    boxes = []
    for level in (3, 4, 5):
        n = 1 << level
        w = 1000.0 * R.PC / n
        idx = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
        lo = -500.0 * R.PC + idx * w
        boxes.append(np.concatenate([lo, lo + w], axis=1))
    boxes = np.concatenate(boxes)
    t0 = time.time()
    host, _ = sim.particle_mass_in_box(boxes)
    t1 = time.time()
    dev, back = sim.particle_mass_in_box(boxes, device=0)
    t2 = time.time()
    dev, back = sim.particle_mass_in_box(boxes, device=0)
    t3 = time.time()
    print("mass in %d octree boxes: host %.3f s, device %.3f s (first call, with the upload), %.3f s (second); "
          "%d handed back (%.1f %%)" % (len(boxes), t1 - t0, t2 - t1, t3 - t2, back, 100.0 * back / len(boxes)))
    assert np.array_equal(dev, host)
    assert back == sum(1 for b in boxes if P_.spanned([float(t) for t in b]) > S.particle_merge_cap())


# ---------------------------------------------------------------- the probes on the device
@pytest.mark.parametrize("model,file", [("part_oct", "cloud.dat"), ("part_oct_neg", "cloud_neg.dat")])
def test_device_probes_equal_the_host_bit_for_bit(model, file):
    sim = _load(model, seed=4357)
    Pr = R.Particles(os.path.join(PART, file), 0.3, 8e4)
    sep = sim.particle_info()["separators"]
    assert np.array_equal(sep, np.array(Pr.sep))  # the boxes below are placed on the read-back separators
    pts = R.adversarial_points(Pr)
    assert np.array_equal(sim.particle_density(pts, device=0), sim.particle_density(pts))
    within, beyond = R.adversarial_boxes(Pr)
    m, back = sim.particle_mass_in_box(within, device=0)
    assert back == 0  # within the cap: all computed on the device
    assert np.array_equal(m, sim.particle_mass_in_box(within)[0])
    m, back = sim.particle_mass_in_box(beyond, device=0)
    assert back == len(beyond)  # built to exceed it: exactly the handed-back count
    assert np.array_equal(m, sim.particle_mass_in_box(beyond)[0])
    both = np.concatenate([within[:300], beyond, within[300:600]])
    m, back = sim.particle_mass_in_box(both, device=0)
    assert back == len(beyond) and np.array_equal(m, sim.particle_mass_in_box(both)[0])


def test_device_probes_on_unsorted_separators():
    sim = _load("part_few", seed=4357)
    Pr = R.Particles(os.path.join(PART, "few.dat"), 0.3, 8e4)
    pts = R.adversarial_points(Pr, nrandom=2000)
    assert np.array_equal(sim.particle_density(pts, device=0), sim.particle_density(pts))
    rng = np.random.RandomState(3)
    lo, hi = np.full(3, 230.0 * R.PC), np.full(3, 370.0 * R.PC)
    a, b = lo + rng.rand(500, 3) * (hi - lo), lo + rng.rand(500, 3) * (hi - lo)
    a[::5] = -600.0 * R.PC * rng.rand(100, 3)
    boxes = np.concatenate([np.minimum(a, b), np.maximum(a, b)], axis=1)
    host, _ = sim.particle_mass_in_box(boxes)
    dev, back = sim.particle_mass_in_box(boxes, device=0)
    assert np.array_equal(dev, host) and np.count_nonzero(host) > 50
    assert back == sum(1 for bx in boxes if Pr.spanned([float(t) for t in bx]) > S.particle_merge_cap())


# ---------------------------------------------------------------- photon phases against the oracle, same streams
@pytest.mark.parametrize("name", ["part_oct", "part_cart", "part_vor"])
def test_photon_phases_match_oracle_same_streams(tmp_path, name):
    packages = 2000
    path = _absolute(tmp_path, name)
    sim = S.Simulation(path, packages=packages)
    sim.attach(0)
    sim.run_stellar()
    sim.run_dust()
    sim.fetch()
    dust = name == "part_cart"
    orc = O.run(path, rng=O.RNG_PHILOX, threads=16, packages=packages, phases=O.PHASES_ALL if dust else O.PHASES_STELLAR)
    rtol, budget = (1e-8, DUST_OUTLIERS) if dust else (1e-9, STELLAR_OUTLIERS)
    assert sim.stats()["packets"] > 0
    if orc.labs is not None:
        np.testing.assert_allclose(sim.labs().sum(axis=0), orc.labs.sum(axis=0), rtol=1e-9)
        assert_parity(sim.labs(), orc.labs, 1e-9, STELLAR_OUTLIERS, "labs")
    for i in range(sim.info.ninstruments):
        frames, seds = sim.instrument(i)
        if seds is not None:
            np.testing.assert_allclose(seds, orc.seds[i], rtol=rtol, atol=1e-300)
        if frames is not None:
            np.testing.assert_allclose(frames.sum(axis=2), orc.frames[i].sum(axis=2), rtol=rtol, atol=1e-300)
            assert_parity(frames, orc.frames[i], rtol, budget, "frames")
    if dust:
        assert sim.instrument(0)[1][3:5].sum() > 0  # the dust emission reached the instrument


def test_device_setup_then_photon_phase_matches_host_setup():
    """tests/test_gpu_setup.py's test on part_oct: the same tree and (here) the same densities bit for bit"""
    out = []
    for dev in (None, 0):
        sim = _load("part_oct", packages=2000, setup_device=dev)
        sim.attach(0)
        sim.run_stellar()
        sim.fetch()
        out.append(sim.instrument(0)[1])
    np.testing.assert_allclose(out[1], out[0], rtol=1e-9, atol=1e-300)


# ---------------------------------------------------------------- against the reference's own outputs
def _ref_file(tmp_path, name, what):
    path = os.path.join(REF, "%s_s4357_%s" % (name, what))
    if os.path.exists(path):
        return path
    out = str(tmp_path / ("ref_%s_%s" % (name, what)))
    with gzip.open(path + ".gz", "rb") as f, open(out, "wb") as o:
        o.write(f.read())
    return out


_RUNS = {}


def _seed_runs(tmp_path, name):
    """P._engine_seed_runs with the input folder: all phases on the grid of the fixture's seed with 16 independent
    photon seeds, written in SKIRT format; (ds_isrf J [K, ncells, nlambda] or None, i30 SEDs, i90 SEDs, a prefix)"""
    if name not in _RUNS:
        J, s30, s90 = [], [], []
        for k, sd in enumerate(P.SEEDS):
            r = _load(name, seed=4357)
            r.set_photon_seed(sd)
            r.attach(0)
            r.run_stellar()
            r.run_dust()
            r.fetch()
            prefix = str(tmp_path / ("%s_%d" % (name, k)))
            r.write(prefix)
            if os.path.exists(prefix + "_ds_isrf.dat"):
                J.append(P._isrf_cells(prefix + "_ds_isrf.dat", r.info.ncells))
            s30.append(F.read_text_table(prefix + "_i30_sed.dat"))
            s90.append(F.read_text_table(prefix + "_i90_sed.dat"))
        _RUNS[name] = (np.array(J) if J else None, np.array(s30), np.array(s90), prefix)
    return _RUNS[name]


@pytest.mark.parametrize("name", MODELS)
def test_seds_and_convergence_match_the_reference(tmp_path, name):
    J, s30, s90, prefix = _seed_runs(tmp_path, name)
    ref30 = F.read_text_table(os.path.join(REF, name + "_s4357_i30_sed.dat"))
    ref90 = F.read_text_table(os.path.join(REF, name + "_s4357_i90_sed.dat")).reshape(s90.shape[1], -1)
    assert s30.shape[1:] == ref30.reshape(s30.shape[1], -1).shape
    scored = G._score_sed(name, s30, ref30.reshape(s30.shape[1], -1), range(1, s30.shape[2]))
    scored += G._score_sed(name, s90.reshape(len(P.SEEDS), s90.shape[1], -1), ref90, range(1, ref90.shape[1]))
    assert scored >= 3
    # ds_convergence: the 3D form, the expected values from the particles' SigmaX/Y/Z, the actual ones from the
    # engine's column densities through the grid
    got = open(prefix + "_ds_convergence.dat").read()
    assert got == open(os.path.join(REF, name + "_s4357_ds_convergence.dat")).read()
    assert "X-axis surface density" in got and "Z-axis surface density" in got


def test_isrf_sums_match_the_reference(tmp_path):
    """part_cart, the one model whose reference run writes a ds_isrf (the others are Pan without dust emission, or
    Oligo): the per-wavelength ISRF sums of test_gpu_geom.test_engine_matches_reference_statistically"""
    name = "part_cart"
    J, _, _, _ = _seed_runs(tmp_path, name)
    Jsum = J.sum(axis=1)
    ref_J = P._isrf_sums(_ref_file(tmp_path, name, "ds_isrf.dat"))
    infl = np.sqrt(1 + 1.0 / len(P.SEEDS))
    m, s = Jsum.mean(axis=0), Jsum.std(axis=0, ddof=1)
    good = (s > 0) & (s <= 0.5 * m)
    z = (ref_J[good] - m[good]) / (s[good] * infl)
    print("%s ISRF sums: max |z| %.2f over %d" % (name, np.abs(z).max(), len(z)))
    assert len(z) >= 5
    assert np.all(np.abs(z) < P.Z_BOUND), z
    P._assert_aggregate(z, "ISRF sums")


def test_per_cell_mean_intensity_matches_reference(tmp_path):
    """part_cart, the model that writes an ISRF (the per-cell absorption): test_gpu_geom's per-cell statistic"""
    name = "part_cart"
    J, _, _, _ = _seed_runs(tmp_path, name)
    ref = P._isrf_cells(_ref_file(tmp_path, name, "ds_isrf.dat"), J.shape[1])
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
    print("per-cell J %s: %d pools, mean z^2 %.3f (t_%d: %.3f), |z|>4: %d" % (name, len(z), chi2, nu, nu / (nu - 2), tail))
    assert len(z) > 100
    assert chi2 < 1.35 * nu / (nu - 2), chi2
    assert tail <= max(3, 0.005 * len(z)), tail
