"""Anisotropic emission (NetzerAccretionDiskGeometry, StellarSurfaceGeometry, SpheBackgroundGeometry,
CubBackgroundGeometry, SolarPatchGeometry, LaserGeometry) on the device: the launch routine's positions, directions
and emission-peel-off probabilities against the host's on the same per-packet streams; the analytic identities of a
source at the origin; the engine's outputs against the reference's (tests/golden/ref_aniso, `skirt -t 1`)
statistically, by the rules of test_gpu_geom; and the invariants that need no checker (shards, repeated runs). The
CPU oracle knows none of these kinds, so nothing here calls it."""
import gzip
import math
import os

import numpy as np
import pytest

import aniso_ref as A
import skirt_files as F
import skirt_amd as S
import test_gpu_parity as P
from skirt_amd.sharding import shard_slice

pytestmark = pytest.mark.gpu
REF = os.path.join(P.GOLD, "ref_aniso")
PC = 3.08567758e16
FREE = {"free_netzer": "netzer", "free_surface": "surface", "free_sphebg": "sphebg", "free_cubbg": "cubbg",
        "free_patch": "patch", "free_laser": "laser"}
R0_PC = 300.0  # the radius / extent of the dust-free models' sources
# dusty models: the instruments whose SEDs are scored
DUSTY = {"netzer_torus_sph2": ("i30", "i80"), "netzer_cone_cyl": ("i30", "i80"), "surface_shell_sph1": ("i30",),
         "sphebg_plummer_cart": ("i30",), "cubbg_oct": ("i30",)}
SED_FLOOR = 15  # scored SED entries per dusty model, at least


def _run(name, packages=0.0, dust=False, seed=0):
    sim = S.Simulation(P.ski(name), packages=packages, seed=seed)
    sim.attach(0)
    sim.run_stellar()
    if dust:
        sim.run_dust()
    sim.fetch()
    return sim


def _netzer_p(deg):
    return A.netzer_probability(math.cos(math.radians(deg)))


# ---------------------------------------------------------------- the launch probe: device against host
@pytest.mark.parametrize("name", list(FREE))
def test_device_launches_equal_host_launches(name):
    kind = FREE[name]
    n = 20000
    sim = S.Simulation(P.ski(name))
    hpos, hdir, hdraws = sim.launches(0, n, seed=9, first=7)
    dpos, ddir, ddraws = sim.launches(0, n, seed=9, first=7, device=0)
    np.testing.assert_array_equal(ddraws, hdraws)  # no kind has a rejection loop
    assert np.all(hdraws == A.DRAWS[kind])
    np.testing.assert_allclose(dpos, hpos, rtol=1e-9, atol=1e-12 * R0_PC * PC)
    np.testing.assert_allclose(ddir, hdir, rtol=1e-9, atol=1e-12)
    assert np.all(np.isfinite(dpos)) and np.all(np.isfinite(ddir))
    np.testing.assert_allclose((ddir ** 2).sum(axis=1), 1.0, rtol=0, atol=1e-14)
    # probabilityForDirection at the launched positions, towards the launch directions of other packets, and at the
    # adversarial positions (poles, axes; edges and corners of the cube) towards the adversarial directions
    r0 = R0_PC * PC
    pos = [hpos]
    dirs = [hdir[::-1]]
    for p in A.adversarial_positions(kind, r0):
        for k in A.adversarial_directions(kind):
            pos.append(np.array([p]))
            dirs.append(np.array([k]))
    pos, dirs = np.vstack(pos), np.vstack(dirs)
    if kind == "laser":  # (the launch directions are the axis itself, where the probability is infinite)
        pos, dirs = pos[n:], dirs[n:]
    hp = sim.emission_probability(0, pos, dirs)
    dp = sim.emission_probability(0, pos, dirs, device=0)
    assert np.all(np.isfinite(dp)) and np.all(dp >= 0)
    np.testing.assert_allclose(dp, hp, rtol=1e-9, atol=1e-12)
    assert dp.max() > 0 or kind == "laser"


def test_device_refuses_a_position_off_the_surface():
    sim = S.Simulation(P.ski("free_surface"))
    sim.attach(0)
    r0 = R0_PC * PC
    with pytest.raises(S.SkirtError, match="not defined for positions not on the stellar surface"):
        sim.emission_probability(0, [[0.0, 0.0, r0 * (1 + 3e-8)]], [[0.0, 0.0, 1.0]], device=0)
    ok = sim.emission_probability(0, [[0.0, 0.0, r0 * (1 + 3e-9)]], [[0.0, 0.0, 1.0]], device=0)
    np.testing.assert_allclose(ok, 4.0, rtol=1e-8)
    with pytest.raises(S.SkirtError, match="anisotropic component"):
        sim.positions(0, 4, device=0)


def test_existing_kinds_launch_as_before():
    """launches on a Plummer component: the parent's positions (the positions probe's, on its own tag, cannot be
    compared stream for stream; the host's launch can) and isotropic directions; and the isotropic event kernel ran:
    the model's results equal the oracle's packet for packet in test_gpu_parity"""
    sim = S.Simulation(P.ski("torus_oct"))
    hpos, hdir, hdraws = sim.launches(0, 5000)
    dpos, ddir, ddraws = sim.launches(0, 5000, device=0)
    np.testing.assert_array_equal(hdraws, ddraws)
    assert np.all(ddraws == 5)  # radius, two for the position's direction, two for the emission direction
    np.testing.assert_allclose(dpos, hpos, rtol=1e-9, atol=1e-12 * 100 * PC)
    np.testing.assert_allclose(ddir, hdir, rtol=1e-9, atol=1e-12)
    assert abs(ddir.mean(axis=0)).max() < 0.03 and abs((ddir ** 2).mean(axis=0) - 1 / 3.).max() < 0.02  # isotropic
    np.testing.assert_array_equal(sim.emission_probability(0, dpos, ddir, device=0), 1.0)
    r = np.sqrt((dpos ** 2).sum(1)) / (100 * PC)
    assert 0.9 < np.median(r) / 1.3048 < 1.1  # PlummerGeometry: half-mass radius 1.3048 c


# ---------------------------------------------------------------- analytic identities
def _seds(sim, names):
    """the one SED entry of each SEDInstrument of a dust-free model"""
    return {n: sim.instrument(i)[1][0, 0] for i, n in enumerate(names) if n.startswith("sed")}


INSTR = ["face", "edge", "sed30", "sed60", "sed120"]


def test_netzer_fluxes_follow_the_probability(tmp_path):
    """every packet of free_netzer leaves the origin, so an SED entry is Ltot P(i) / (4 pi d^2) up to the order of
    4e3 equal terms: the flux ratios equal the probability ratios to 4e3 2^-53 < 1e-12"""
    sim = _run("free_netzer")
    assert sim.stats()["packets"] == 4000
    s = _seds(sim, INSTR)
    assert s["sed30"] > 0 and s["sed60"] > 0 and s["sed120"] > 0
    np.testing.assert_allclose(s["sed30"] / s["sed60"], _netzer_p(30) / _netzer_p(60), rtol=1e-12)
    np.testing.assert_allclose(s["sed60"] / s["sed120"], _netzer_p(60) / _netzer_p(120), rtol=1e-12)
    sim.write(str(tmp_path / "gpu"))
    for n in ("sed30", "sed60", "sed120"):
        got = open(str(tmp_path / ("gpu_%s_sed.dat" % n))).read()
        assert got == open(os.path.join(REF, "free_netzer_s4357_%s_sed.dat" % n)).read()


def test_surface_emits_the_same_both_ways_and_a_laser_nothing_off_axis(tmp_path):
    up, down = [], []
    for sd in P.SEEDS:
        sim = S.Simulation(P.ski("free_surface"))
        sim.set_photon_seed(sd)
        sim.attach(0)
        sim.run_stellar()
        sim.fetch()
        s = _seds(sim, INSTR)
        up.append(s["sed60"])
        down.append(s["sed120"])
    up, down = np.array(up), np.array(down)
    z = (up.mean() - down.mean()) / np.sqrt(up.var(ddof=1) / len(up) + down.var(ddof=1) / len(down))
    print("free_surface: SED at 60 deg %.6g, at 120 deg %.6g, z %.2f" % (up.mean(), down.mean(), z))
    assert abs(z) < P.Z_BOUND
    laser = _run("free_laser")
    assert laser.stats()["packets"] == 4000
    for i in range(5):
        frames, seds = laser.instrument(i)
        assert (frames is None or not np.any(frames)) and (seds is None or not np.any(seds))


def test_laser_fill_rays_leave_along_the_axis():
    """a laser inside dust: every packet's first path runs up the z axis, so no cell off the axis absorbs anything
    unless a packet scattered first; with the albedo's share removed: the cells of the Cartesian grid that the axis
    does not touch receive only scattered light, the ones it touches (x, y indices 7 and 8, z > 0) the direct beam"""
    text = open(P.ski("sphebg_plummer_cart")).read().replace('<SpheBackgroundGeometry radius="1000 pc"/>', '<LaserGeometry/>')
    assert "LaserGeometry" in text
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "laser_cart.ski")
        open(path, "w").write(text)
        sim = S.Simulation(path, packages=2000)
        sim.attach(0)
        sim.run_stellar()
        sim.fetch()
        dirs = sim.launches(0, 100, device=0)[1]
    np.testing.assert_array_equal(dirs, np.tile([0.0, 0.0, 1.0], (100, 1)))
    labs = sim.labs().sum(axis=1).reshape(16, 16, 16)  # m = k + nz j + nz ny i
    beam = labs[7:9, 7:9, 8:].sum()
    below = labs[7:9, 7:9, :8].sum()
    assert beam > 0 and beam > 2 * below  # the half of the axis below the source sees scattered light only
    # the peel-offs of the emission carry probability 0 towards the instrument at 30 deg: its direct flux is 0
    assert not np.any(sim.instrument(0)[1][1])


# ---------------------------------------------------------------- against the reference's outputs
@pytest.mark.parametrize("name", list(FREE))
def test_dust_free_frames_and_seds_match_reference(tmp_path, name):
    """test_gpu_geom.test_dust_free_frames_match_reference: both frames as pools of pixels (P._pools at 0.25 over the
    16 seeds) z-scored against the reference's total.fits, at least 30 pools per frame; and the three SEDs as
    z-scores. A point source lights one pixel, the same in every run: compared entry by entry."""
    frames = {"face": [], "edge": []}
    seds = {"sed30": [], "sed60": [], "sed120": []}
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
        for s in seds:
            seds[s].append(F.read_text_table("%s_%s_sed.dat" % (prefix, s))[0, 1])
    K = len(P.SEEDS)
    nu = K - 1
    infl = np.sqrt(1 + 1.0 / K)
    point = FREE[name] in ("netzer", "laser")
    for s, runs in seds.items():
        v = np.array(runs)
        ref = F.read_text_table(os.path.join(REF, "%s_s4357_%s_sed.dat" % (name, s)))[0, 1]
        if v.std(ddof=1) > 0:
            z = (ref - v.mean()) / (v.std(ddof=1) * infl)
            print("%s %s: z %.2f" % (name, s, z))
            assert abs(z) < P.Z_BOUND
        else:  # the same flux whatever the seed, to the printed digits: a point source, or a direction without emission
            # (or a patch, whose probability does not depend on the position)
            assert np.all(v == ref), (s, v[0], ref)
    for f, runs in frames.items():
        Aall = np.array(runs)
        ref = F.read_fits(os.path.join(REF, "%s_s4357_%s_total.fits" % (name, f))).astype(np.float64).reshape(-1)
        assert Aall.shape == (K, 1024) and ref.shape == (1024,)
        if point:  # one lit pixel (or none), the same in every run
            assert np.count_nonzero(ref) <= 1
            np.testing.assert_array_equal(Aall[0] != 0, ref != 0)
            np.testing.assert_allclose(Aall, np.tile(ref, (K, 1)), rtol=1e-6)  # (FITS frames are float32)
            continue
        z = []
        for p in P._pools(Aall, 0.25):
            tot = Aall[:, p].sum(axis=1)
            m, sdev = tot.mean(), tot.std(ddof=1)
            if sdev > 0:
                z.append((ref[p].sum() - m) / (sdev * infl))
        z = np.array(z)
        chi2 = float(np.mean(z ** 2))
        tail = int(np.count_nonzero(np.abs(z) > 4))
        print("%s %s frame: %d pools, mean z^2 %.3f (t_%d: %.3f), |z|>4: %d" % (name, f, len(z), chi2, nu, nu / (nu - 2), tail))
        # at least 30 pools per frame, the rule's floor; the patch seen edge-on is a line of 20 pixels, which cannot
        # make 30 pools of whole pixels: there, half its lit pixels (a pool may take two)
        lit = int(np.count_nonzero(ref))
        assert len(z) >= (30 if lit >= 60 else lit // 2), (len(z), lit)
        assert chi2 < 1.35 * nu / (nu - 2), chi2
        assert tail <= max(3, 0.005 * len(z)), tail


def _ref_isrf(tmp_path, name):
    path = os.path.join(REF, name + "_s4357_ds_isrf.dat")
    if os.path.exists(path):
        return path
    out = str(tmp_path / (name + "_ref_ds_isrf.dat"))
    with gzip.open(path + ".gz", "rb") as f, open(out, "wb") as o:
        o.write(f.read())
    return out


@pytest.mark.parametrize("name", list(DUSTY))
def test_dusty_models_match_reference_statistically(tmp_path, name):
    """test_gpu_geom.test_engine_matches_reference_statistically and test_models_without_isrf_match_reference_seds:
    the per-wavelength ISRF sums and every SED column of every instrument as z-scores against the spread of 16
    independently seeded engine runs on the reference's grid (seed 4357); at least SED_FLOOR SED entries scored"""
    J, seds = [], {i: [] for i in DUSTY[name]}
    for k, sd in enumerate(P.SEEDS):
        r = S.Simulation(P.ski(name), seed=4357)
        r.set_photon_seed(sd)
        r.attach(0)
        r.run_stellar()
        r.run_dust()
        r.fetch()
        prefix = str(tmp_path / ("%s_%d" % (name, k)))
        r.write(prefix)
        J.append(P._isrf_cells(prefix + "_ds_isrf.dat", r.info.ncells))
        for i in seds:
            seds[i].append(F.read_text_table(prefix + "_%s_sed.dat" % i))
    J = np.array(J)
    Jsum = J.sum(axis=1)
    ref_J = P._isrf_sums(_ref_isrf(tmp_path, name))
    infl = np.sqrt(1 + 1.0 / len(P.SEEDS))
    m, s = Jsum.mean(axis=0), Jsum.std(axis=0, ddof=1)
    good = (s > 0) & (s <= 0.5 * m)
    z = (ref_J[good] - m[good]) / (s[good] * infl)
    print("%s ISRF sums: max |z| %.2f over %d" % (name, np.abs(z).max(), len(z)))
    assert len(z) >= 5
    assert np.all(np.abs(z) < P.Z_BOUND), z
    P._assert_aggregate(z, "ISRF sums")
    scored = 0
    for i, runs in seds.items():
        runs = np.array(runs)
        ref_sed = F.read_text_table(os.path.join(REF, "%s_s4357_%s_sed.dat" % (name, i)))
        assert runs.shape[1:] == ref_sed.shape
        for col in range(1, ref_sed.shape[1]):
            mm, ss = runs[:, :, col].mean(axis=0), runs[:, :, col].std(axis=0, ddof=1)
            ok = (ss > 0) & (mm > 1e-12 * mm.max()) & (ss <= 0.5 * mm)
            zz = (ref_sed[ok, col] - mm[ok]) / (ss[ok] * infl)
            print("%s %s SED column %d: max |z| %.2f over %d" % (name, i, col, np.abs(zz).max() if len(zz) else 0.0, len(zz)))
            assert np.all(np.abs(zz) < P.Z_BOUND), (i, col, zz)
            P._assert_aggregate(zz, "%s SED column %d" % (i, col))
            scored += len(zz)
            # the transparent flux of a source at the origin is the same whatever the seed, to the last printed digit
            if name.startswith("netzer") and col == 6:
                assert mm.max() > 0
                np.testing.assert_allclose(runs[:, :, col], np.tile(ref_sed[:, col], (len(runs), 1)), rtol=2e-9)
    print("%s: %d SED entries scored" % (name, scored))
    assert scored >= SED_FLOOR


def test_anisotropy_shows_in_the_torus_model():
    """netzer_torus_sph2: the transparent fluxes at 30 and 80 deg are Ltot P(i) each, so their ratio is P(30)/P(80)
    to the summation order; the direct flux at 80 deg looks through the torus, so its ratio to the one at 30 deg
    exceeds even that"""
    sim = _run("netzer_torus_sph2", dust=False)
    s30, s80 = sim.instrument(0)[1], sim.instrument(1)[1]
    lit = s30[0] > 0
    assert lit.sum() >= 5
    want = _netzer_p(30) / _netzer_p(80)
    assert want > 9  # (a point source's would be 1)
    np.testing.assert_allclose(s30[0][lit] / s80[0][lit], want, rtol=1e-12)  # slot 0: transparent
    direct = s30[1][lit] / s80[1][lit]
    assert np.all(direct >= want * (1 - 1e-12)) and direct.max() > 1.5 * want


@pytest.mark.parametrize("name,star", [("pol_torus_cart", "<PointGeometry/>"),
                                       ("pol_2comp_sph2", '<PlummerGeometry scale="50 pc"/>'),
                                       ("torus_sph2", "<PointGeometry/>")])
def test_direct_flux_of_a_disk_is_a_point_source_times_the_probability(tmp_path, name, star):
    """A Netzer disk and a point source of the same spectrum send every packet from the origin, so towards one
    instrument all their emission peel-offs see the same optical depth: the disk's transparent and direct fluxes are
    the point source's times P(inclination), to the summation order (2000 equal terms: 1e-12). Through the polarised
    ANISO kernels with one dust component (pol_torus_cart, ElectronDustMix on a Cartesian grid) and with two
    (pol_2comp_sph2, Sphere2D), and the unpolarised one (torus_sph2)."""
    import re
    text = open(P.ski(name)).read()
    assert text.count(star) == 1
    runs = {}
    for kind, element in (("point", "<PointGeometry/>"), ("disk", "<NetzerAccretionDiskGeometry/>")):
        path = str(tmp_path / (kind + ".ski"))
        open(path, "w").write(text.replace(star, element))
        sim = S.Simulation(path, packages=2000)
        sim.attach(0)
        sim.run_stellar()
        sim.fetch()
        runs[kind] = sim
    incl = [float(v) for v in re.findall(r'Instrument instrumentName="[^"]*" distance="[^"]*" inclination="([0-9.]+) deg"', text)]
    assert len(incl) == runs["disk"].info.ninstruments
    assert runs["disk"].polarization == name.startswith("pol_")
    checked = 0
    for i, deg in enumerate(incl):
        sd, sp = runs["disk"].instrument(i)[1], runs["point"].instrument(i)[1]
        assert np.all(np.isfinite(sd)) and np.all(sd >= 0) or runs["disk"].polarization  # (Stokes slots have a sign)
        c = math.cos(math.radians(deg))
        if abs(c) < 1e-6 or len(sd) < 5:  # edge-on: P hangs on the last bit of cos(90 deg); an SEDInstrument: total only
            continue
        lit = sp[0] > 0
        assert lit.any()
        for slot in (0, 1):  # transparent, direct stellar
            np.testing.assert_allclose(sd[slot][lit], sp[slot][lit] * A.netzer_probability(c), rtol=1e-12)
        assert sd[2][lit].sum() > 0  # scattered light arrived too
        checked += 1
    assert checked >= 1
    if runs["disk"].polarization:
        frames, seds = runs["disk"].stokes(0)
        assert np.all(np.isfinite(seds)) and np.any(seds[:2] != 0)


# ---------------------------------------------------------------- invariants without a checker
@pytest.mark.parametrize("name", ["netzer_torus_sph2", "sphebg_plummer_cart"])
def test_three_shards_sum_to_the_unsharded_run(name):
    packages = 2000
    full = _run(name, packages=packages, seed=4357)
    st = full.stats()
    lit = np.count_nonzero(full.labs().sum(axis=0) > 0)
    assert lit >= 5 and st["packets"] == packages * lit
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


@pytest.mark.parametrize("name", ["netzer_torus_sph2", "sphebg_plummer_cart"])
def test_second_run_equals_a_fresh_run(name):
    sim = S.Simulation(P.ski(name), packages=1000)
    sim.attach(0)
    for _ in range(2):
        sim.zero_tallies()
        sim.run_stellar()
        sim.run_dust()
        sim.fetch()
    fresh = _run(name, packages=1000, dust=True)
    assert fresh.instrument(0)[1][3:5].sum() > 0  # the dust emission reached the instrument
    # P._assert_equal_runs without the dust Labs (neither model has self-absorption cycles)
    np.testing.assert_allclose(sim.labs(), fresh.labs(), rtol=1e-10, atol=1e-300)
    for i in range(sim.info.ninstruments):
        fa, sa = sim.instrument(i)
        fb, sb = fresh.instrument(i)
        np.testing.assert_allclose(sa, sb, rtol=1e-10, atol=1e-300)
        np.testing.assert_allclose(fa, fb, rtol=1e-10, atol=1e-300)
