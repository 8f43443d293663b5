"""Polarised scattering (ElectronDustMix) on the GPU: the event kernel's POL instantiations (Stokes vector per packet,
table-driven theta and phi, Mueller matrix and frame rotations per peel-off; skirt_amd/csrc/device/polarization.hpp)
and the detect kernel's Stokes slots, against

1. the host's compilation of the same routines through the scatterings probe: rtol 1e-9 (the project's
   engine-against-CPU tolerance), atol 1e-12 on the unit-scale values;
2. the reference's own outputs (`skirt -t 1`, tests/golden/ref_pol), statistically, with the seeds, the bound and the
   aggregate rule of test_gpu_parity.py: every SED column, Q and U included, and Q, U and the scattered flux summed
   over blocks of 4 x 4 pixels; V is exactly 0;
3. invariants that need no checker: V = 0, sqrt(Q^2 + U^2 + V^2) <= scattered flux in every pixel, shards sum to the
   whole, a second run equals a fresh one, the counts;
4. unchanged ground: unpolarised models keep their tallies' shapes."""
import ctypes
import os

import numpy as np
import pytest

import descriptors
import pol_ref
import skirt_files as F
import skirt_amd as S
import test_gpu_parity as P
from skirt_amd.sharding import shard_slice

pytestmark = pytest.mark.gpu
_INSTR_DOUBLES = ("sinphi", "cosphi", "sintheta", "costheta", "sinpa", "cospa", "xpmin", "xpsiz", "ypmin", "ypsiz")
REF = os.path.join(P.GOLD, "ref_pol")
# model -> its FullInstruments: (name, scattering levels)
MODELS = {"pol_torus_cart": [("i30", 1), ("i90", 0)], "pol_2comp_sph2": [("i30", 2)], "pol_pan_cart": [("i30", 1), ("i90", 0)]}


# ---------------------------------------------------------------- 1. the probe
@pytest.mark.parametrize("name,instrument,angles", [("pol_torus_cart", 1, (90.0, 40.0, 25.0)),
                                                    ("pol_2comp_sph2", 0, (60.0, 0.0, 0.0))])
def test_device_probe_equals_the_host_compilation(name, instrument, angles):
    sim = S.Simulation(P.ski(name), packages=10)
    nl, nc = sim.info.nlambda, sim.info.ncomp
    mixes = [pol_ref.electron_mix(nl)] * nc
    kobs, ky = pol_ref.instrument_axes(*angles)
    states, devs = pol_ref.make_states(mixes, nl, kobs)  # the logic test's states, on every component
    assert len(states) > pol_ref.N_RANDOM + 50 and set(states[:, 11]) == set(range(nc))
    del pol_ref.INDEX_ARGS[:]
    pol_ref.probe(mixes, states, devs, kobs, ky)
    assert pol_ref.near_integer_count() == 0  # the condition of the comparison; nothing is left out
    host = sim.scatterings(states, devs, instrument)
    dev = sim.scatterings(states, devs, instrument, device=0)
    assert np.isfinite(host).all() and np.isfinite(dev).all()
    print("%s: %d states, largest difference %.3g" % (name, len(states), np.abs(dev - host).max()))
    assert np.array_equal(dev[:, 9], host[:, 9])
    np.testing.assert_allclose(dev, host, rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------- 2. against the reference's outputs
def _blocks(frame):
    """[nl, 16, 16] -> [nl, 16]: sums over blocks of 4 x 4 pixels"""
    nl = frame.shape[0]
    return frame.reshape(nl, 4, 4, 4, 4).sum(axis=(2, 4)).reshape(nl, 16)


def _read_run(prefix, name):
    out = {}
    for ins, _ in MODELS[name]:
        out[ins] = {"sed": F.read_text_table("%s_%s_sed.dat" % (prefix, ins))}
        for kind in ("stokesQ", "stokesU", "stokesV", "scattered"):
            out[ins][kind] = F.read_fits("%s_%s_%s.fits" % (prefix, ins, kind)).astype(np.float64)
    return out


_RUNS = {}


def _seed_runs(tmp_path_factory, name):
    """the model on the grid of the ski's own seed with independent photon streams per seed of P.SEEDS, written in
    SKIRT format; computed once per model and shared by the tests below"""
    if name not in _RUNS:
        d = tmp_path_factory.mktemp(name)
        runs = []
        for k, sd in enumerate(P.SEEDS):
            r = S.Simulation(P.ski(name))
            r.set_photon_seed(sd)
            r.attach(0)
            r.run_stellar()
            r.fetch()
            prefix = str(d / ("%s_%d" % (name, k)))
            r.write(prefix)
            runs.append(_read_run(prefix, name))
            r.close()
        _RUNS[name] = runs
    return _RUNS[name]


@pytest.mark.parametrize("name", ["pol_torus_cart", "pol_2comp_sph2"])
def test_ds_convergence_equals_the_reference_file(tmp_path, name):
    sim = S.Simulation(P.ski(name), packages=10)
    sim.attach(0)
    sim.run_stellar()
    sim.fetch()
    sim.write(str(tmp_path / "gpu"))
    got = open(str(tmp_path / "gpu_ds_convergence.dat")).read()
    assert got == open(os.path.join(REF, name + "_s4357_ds_convergence.dat")).read()


@pytest.mark.parametrize("name,ins", [("pol_torus_cart", "i30"), ("pol_torus_cart", "i90"), ("pol_2comp_sph2", "i30")])
def test_sed_columns_match_reference_statistically(tmp_path_factory, name, ins):
    runs = _seed_runs(tmp_path_factory, name)
    seds = np.array([r[ins]["sed"] for r in runs])
    ref = F.read_text_table(os.path.join(REF, "%s_s4357_%s_sed.dat" % (name, ins)))
    assert seds.shape[1:] == ref.shape
    infl = np.sqrt(1 + 1.0 / len(P.SEEDS))
    scored = {}
    for col in range(1, ref.shape[1]):
        m, s = seds[:, :, col].mean(axis=0), seds[:, :, col].std(axis=0, ddof=1)
        if col in (7, 8):  # Stokes Q and U (columns 8 and 9 of the file) are signed
            good = s > 0
        else:
            good = (s > 0) & (m > 1e-12 * m.max()) & (s <= 0.5 * m)
        zz = (ref[good, col] - m[good]) / (s[good] * infl)
        print("%s %s SED column %d: mean %s ref %s z %s" % (name, ins, col + 1, m, ref[:, col], np.round(zz, 2)))
        assert np.all(np.abs(zz) < P.Z_BOUND), (col, zz)
        P._assert_aggregate(zz, "SED column %d" % (col + 1))
        scored[col] = len(zz)
    nl = ref.shape[0]
    # total, scattered, Q and U at every wavelength (a point star's direct flux is the same in every run: no spread)
    assert scored[1] == scored[3] == scored[7] == scored[8] == nl
    # column 10, Stokes V: exactly 0 in every run and in the fixture
    assert np.all(seds[:, :, 9] == 0) and np.all(ref[:, 9] == 0)


@pytest.mark.parametrize("name", ["pol_torus_cart", "pol_2comp_sph2"])
def test_frames_match_reference_statistically(tmp_path_factory, name):
    runs = _seed_runs(tmp_path_factory, name)
    K = len(P.SEEDS)
    infl = np.sqrt(1 + 1.0 / K)
    z = []
    for ins, _ in MODELS[name]:
        for kind in ("stokesQ", "stokesU", "scattered"):
            got = np.array([_blocks(r[ins][kind]) for r in runs])
            ref = _blocks(F.read_fits(os.path.join(REF, "%s_s4357_%s_%s.fits" % (name, ins, kind))).astype(np.float64))
            m, s = got.mean(axis=0), got.std(axis=0, ddof=1)
            good = s > 0
            zz = (ref[good] - m[good]) / (s[good] * infl)
            print("%s %s %s: %d blocks, max |z| %.2f" % (name, ins, kind, len(zz), np.abs(zz).max()))
            assert len(zz) >= 8 and np.all(np.abs(zz) < P.Z_BOUND), (ins, kind, zz)
            z.append(zz)
        v = np.array([r[ins]["stokesV"] for r in runs])
        assert np.all(v == 0)
        assert np.all(F.read_fits(os.path.join(REF, "%s_s4357_%s_stokesV.fits" % (name, ins))) == 0)
    z = np.concatenate(z)
    nu = K - 1
    chi2 = float(np.mean(z ** 2))
    print("%s: %d blocks, mean z^2 %.3f (t_%d: %.3f)" % (name, len(z), chi2, nu, nu / (nu - 2)))
    assert chi2 < 1.35 * nu / (nu - 2), chi2


def test_stokes_q_is_not_noise(tmp_path_factory):
    """pol_torus_cart i30: |mean Q| > 10 s / 4 at both wavelengths (the mean of 16 runs has spread s / 4), so that a
    passing z-score above cannot come from noise alone; the reference's Q there is -3 % of the scattered flux"""
    runs = _seed_runs(tmp_path_factory, "pol_torus_cart")
    q = np.array([r["i30"]["sed"][:, 7] for r in runs])
    sca = np.array([r["i30"]["sed"][:, 3] for r in runs])
    m, s = q.mean(axis=0), q.std(axis=0, ddof=1)
    print("Q %s spread %s, Q / scattered %s" % (m, s, m / sca.mean(axis=0)))
    assert np.all(np.abs(m) > 10 * s / 4)
    assert np.all(m < 0)


# ---------------------------------------------------------------- 3. invariants
def _run(name, packages, seed=0):
    sim = S.Simulation(P.ski(name), packages=packages, seed=seed)
    sim.attach(0)
    sim.run_stellar()
    sim.fetch()
    return sim


@pytest.mark.parametrize("name", sorted(MODELS))
def test_invariants(name):
    packages = 20000
    full = _run(name, packages)
    assert full.polarization
    st = full.stats()
    lit = full.info.nlambda  # every wavelength of these models has luminosity
    assert st["packets"] == packages * lit and st["detects"] >= st["packets"] * len(MODELS[name])
    for i, (ins, levels) in enumerate(MODELS[name]):
        frames, seds = full.instrument(i)
        assert frames.shape[0] == seds.shape[0] == 5 + levels + 3
        (fq, fu, fv), (sq, su, sv) = full.stokes(i)
        # V: exactly 0 (S34 = 0 and no packet starts with V)
        assert np.all(fv == 0) and np.all(sv == 0)
        # |Stokes| <= I for every detection, hence (triangle inequality) for their sums over the scattered flux;
        # direct light carries none: where nothing scattered arrived, Q = U = 0
        fsca, ssca = frames[2], seds[2]
        assert np.all(np.sqrt(fq ** 2 + fu ** 2 + fv ** 2) <= fsca * (1 + 1e-12))
        assert np.all(np.sqrt(sq ** 2 + su ** 2 + sv ** 2) <= ssca * (1 + 1e-12))
        assert np.all(fq[fsca == 0] == 0) and np.all(fu[fsca == 0] == 0)
        assert np.abs(sq).max() > 0 and np.abs(fq).max() > 0 and np.abs(fu).max() > 0
        assert np.all(frames[1] >= 0) and frames[1].sum() > 0  # the direct light is there and unpolarised
    # shards sum to the whole
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
    for i in range(len(MODELS[name])):
        ff, sf = full.instrument(i)
        np.testing.assert_allclose(sum(p.instrument(i)[1] for p in parts), sf, rtol=1e-12, atol=1e-300)
        scale = np.abs(ff).max()
        np.testing.assert_allclose(sum(p.instrument(i)[0] for p in parts), ff, rtol=1e-12, atol=1e-12 * scale)
    # A second run on one engine equals a fresh one. Every packet adds the same numbers in both (its stream and its
    # arithmetic do not depend on the run), but the f64 atomics add them in the order the lanes arrive, so only this
    # is exact: the counts, V = 0 (above), and which entries received nothing. For the sums the bound is that of
    # the order of summation alone. An entry is a plain sum of n <= `detects` terms x_i; recursive summation in any
    # order errs by at most lam sqrt(n) u sum |x_i|, u = 2^-53, with probability 1 - 2 exp(-lam^2 / 2) (Higham and
    # Mary 2019, theorem 2.4, rounding errors as independent zero-mean variables; the certain bound has n for
    # lam sqrt(n)). With lam = 10 that fails once in 1e21 entries; two orders differ by at most twice that. sum |x_i|
    # is the entry itself for the luminosity slots and at most the scattered flux of the same pixel for Q, U and V
    # (|Q/I| <= 1 per detection), so a small signed Q or U is held to its own pixel's scale.
    again = S.Simulation(P.ski(name), packages=packages)
    again.attach(0)
    for _ in range(2):
        again.zero_tallies()
        again.run_stellar()
        again.fetch()
    assert again.stats()["packets"] == st["packets"] and again.stats()["detects"] == st["detects"]
    order = 2 * 10 * np.sqrt(st["detects"]) * 2.0 ** -53
    assert order < 1e-11  # (2e5 detections: 1e-12)
    for i in range(len(MODELS[name])):
        worst = 0.0
        for a, b in zip(again.instrument(i), full.instrument(i)):  # frames [slot, nl, npix], then SEDs [slot, nl]
            assert np.array_equal(a == 0, b == 0)
            scale = np.abs(b)
            scale[-3:] = b[2]  # Q, U, V: the scattered flux of the same entry
            bad = np.abs(a - b) > order * scale
            assert not bad.any(), (i, np.argwhere(bad)[:5], a[bad][:5], b[bad][:5])
            worst = max(worst, float((np.abs(a - b)[scale > 0] / scale[scale > 0]).max()))
        print("%s instrument %d: largest difference %.3g of the entry's scale (bound %.3g)" % (name, i, worst, order))


_KDTREE = ('<BinTreeDustGrid writeGrid="false" minX="-500 pc" maxX="500 pc" minY="-500 pc" maxY="500 pc" minZ="-500 pc" '
           'maxZ="500 pc" minLevel="6" maxLevel="12" searchMethod="Neighbor" sampleCount="100" maxOpticalDepth="0" '
           'maxMassFraction="2e-3" maxDensDispFraction="0" directionMethod="Alternating"/>')
_OCTREE = ('<OctTreeDustGrid writeGrid="false" minX="-500 pc" maxX="500 pc" minY="-500 pc" maxY="500 pc" minZ="-500 pc" '
           'maxZ="500 pc" minLevel="2" maxLevel="4" searchMethod="Neighbor" sampleCount="100" maxOpticalDepth="0" '
           'maxMassFraction="2e-3" maxDensDispFraction="0" barycentric="false"/>')


@pytest.mark.parametrize("grid,walk", [("voronoi", S.WALK_VORONOI), ("octree", S.WALK_OCTREE_MAP),
                                       ("kdtree", S.WALK_KDTREE_MAP)])
def test_invariants_with_several_components_on_voronoi_and_tree_grids(tmp_path, grid, walk):
    """the event kernel's polarised instantiations for several components on a Voronoi grid (the one that runs at one
    wave per SIMD) and on the leaf maps of an octree and a k-d tree: vor_geoms (six components, 600 cells, one
    FullInstrument with one level) with electrons for its dust, on its own grid and on the two trees; no reference
    ran these, so the invariants only"""
    import re

    text = open(P.ski("vor_geoms")).read()
    text, n = re.subn(r"<SimpleOligoDustMix [^>]*/>", '<ElectronDustMix writeMix="false" writeMeanMix="false"/>', text)
    assert n == 6
    if grid != "voronoi":
        text, n = re.subn(r"<VoronoiDustGrid [^>]*/>", _OCTREE if grid == "octree" else _KDTREE, text)
        assert n == 1
    path = str(tmp_path / ("pol_%s.ski" % grid))
    open(path, "w").write(text)
    packages = 4000
    sim = S.Simulation(path, packages=packages)
    assert sim.polarization and sim.info.ncomp == 6
    sim.attach(0)
    sim.run_stellar()
    sim.fetch()
    st = sim.stats()
    assert st["grid_walk"] == walk  # the instantiation that ran
    assert st["packets"] == packages * sim.info.nlambda and st["detects"] > st["packets"]
    frames, seds = sim.instrument(0)
    assert frames.shape[0] == seds.shape[0] == 5 + 1 + 3
    (fq, fu, fv), (sq, su, sv) = sim.stokes(0)
    assert np.all(fv == 0) and np.all(sv == 0)
    fsca, ssca = frames[2], seds[2]
    assert ssca.sum() > 0 and np.isfinite(frames).all() and np.isfinite(seds).all()
    assert np.all(np.sqrt(fq ** 2 + fu ** 2) <= fsca * (1 + 1e-12))
    assert np.all(np.sqrt(sq ** 2 + su ** 2) <= ssca * (1 + 1e-12))
    assert np.all(fq[fsca == 0] == 0) and np.all(fu[fsca == 0] == 0)
    assert np.abs(sq).max() > 0 and np.abs(fq).max() > 0 and np.abs(fu).max() > 0
    print("%s: Q / scattered %s, detections %d" % (grid, sq / ssca, st["detects"]))


class _InstrDesc(ctypes.Structure):  # SkirtInstrDesc, include/skirt_mcrt.h
    _fields_ = [("kind", ctypes.c_int), ("nx", ctypes.c_int), ("ny", ctypes.c_int), ("scattering_levels", ctypes.c_int),
                ("kobs", ctypes.c_double * 3)] + [(f, ctypes.c_double) for f in _INSTR_DOUBLES]


class _MuellerDesc(ctypes.Structure):  # SkirtMuellerDesc
    _fields_ = [("ncomp", ctypes.c_int), ("nlambda", ctypes.c_int), ("ntheta", ctypes.c_int)] + \
               [(f, ctypes.POINTER(ctypes.c_double)) for f in ("S11", "S12", "S33", "S34", "thetaX", "pfnorm")]


def test_two_components_with_different_tables(tmp_path):
    """pol_2comp_sph2 with its second component's tables replaced, through skirt_mcrt_set_mueller, by pol_ref's made-up
    mix (forward-peaked, S34 != 0): the model's own two components have the same tables, so only this shows that
    the device takes each component's own. The probe against pol_ref on both tables at the probe's tolerance; a run
    whose V is no longer 0, with |Stokes| <= scattered still (the made-up rows have S11^2 >= S12^2 + S33^2 + S34^2,
    so each scattering keeps |Stokes| <= I)"""
    sim = S.Simulation(P.ski("pol_2comp_sph2"), packages=20000)
    nl, nc = sim.info.nlambda, sim.info.ncomp
    assert nc == 2
    dump = str(tmp_path / "descriptors")
    sim.describe(dump)
    d = descriptors.read(dump)
    ins = (_InstrDesc * int(d["instruments.n"][0]))()
    for k, x in enumerate(ins):
        pre = "instrument%d." % k
        x.kind, x.nx, x.ny = (int(d[pre + f][0]) for f in ("kind", "nx", "ny"))
        x.scattering_levels = int(d[pre + "scattering_levels"][0])
        x.kobs[:] = list(d[pre + "kobs"])
        for f in _INSTR_DOUBLES:
            setattr(x, f, float(d[pre + f][0]))
    mixes = [pol_ref.electron_mix(nl), pol_ref.madeup_mix(nl)]
    tabs = {f: np.array([m[f] for m in mixes], dtype=np.float64).ravel()
            for f in ("S11", "S12", "S33", "S34", "thetaX", "pfnorm")}
    assert np.array_equal(tabs["S11"][:nl * pol_ref.NTHETA], d["mueller.S11"][:nl * pol_ref.NTHETA])
    mu = _MuellerDesc(nc, nl, pol_ref.NTHETA, *(tabs[f].ctypes.data_as(ctypes.POINTER(ctypes.c_double))
                                                for f in ("S11", "S12", "S33", "S34", "thetaX", "pfnorm")))
    sim.attach(0)
    L = S.lib()
    L.skirt_mcrt_set_instruments.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.skirt_mcrt_set_mueller.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert L.skirt_mcrt_set_mueller(sim.engine, ctypes.byref(mu)) == 3  # SKIRT_ERR_STATE: the instruments are set
    assert L.skirt_mcrt_set_instruments(sim.engine, None, 0) == 0
    assert L.skirt_mcrt_set_mueller(sim.engine, ctypes.byref(mu)) == 0, L.skirt_mcrt_last_error(sim.engine)
    assert L.skirt_mcrt_set_instruments(sim.engine, ctypes.byref(ins), len(ins)) == 0
    # the probe: each state by its own component's tables
    kobs, ky = pol_ref.instrument_axes(60.0, 0.0, 0.0)
    states, devs = pol_ref.make_states(mixes, nl, kobs)
    del pol_ref.INDEX_ARGS[:]
    want = pol_ref.probe(mixes, states, devs, kobs, ky)
    assert pol_ref.near_integer_count() == 0
    dev = sim.scatterings(states, devs, 0, device=0)
    print("two tables: %d states, largest difference %.3g" % (len(states), np.abs(dev - want).max()))
    np.testing.assert_allclose(dev, want, rtol=1e-9, atol=1e-12)
    second = states[:, 11] == 1
    electrons = sim.scatterings(states, devs, 0)  # the host's side keeps the model's own tables
    np.testing.assert_allclose(dev[~second], electrons[~second], rtol=1e-9, atol=1e-12)
    assert np.abs(dev[second] - electrons[second]).max() > 0.1
    # a run
    sim.zero_tallies()
    sim.run_stellar()
    sim.fetch()
    frames, seds = sim.instrument(0)
    (fq, fu, fv), (sq, su, sv) = sim.stokes(0)
    fsca, ssca = frames[2], seds[2]
    assert np.isfinite(frames).all() and np.isfinite(seds).all() and ssca.sum() > 0
    assert np.abs(sv).max() > 0 and np.abs(fv).max() > 0  # S34 of the second component
    assert np.all(np.sqrt(fq ** 2 + fu ** 2 + fv ** 2) <= fsca * (1 + 1e-12))
    assert np.all(np.sqrt(sq ** 2 + su ** 2 + sv ** 2) <= ssca * (1 + 1e-12))
    assert np.all(fq[fsca == 0] == 0) and np.all(fu[fsca == 0] == 0) and np.all(fv[fsca == 0] == 0)
    print("two tables: Q, U, V / scattered %s %s %s" % (sq / ssca, su / ssca, sv / ssca))


def test_continuous_scattering_and_dust_phases_are_refused_by_the_engine():
    """the engine's own refusals (a caller of the C ABI that sets Mueller tables): not run unpolarised"""
    import ctypes

    sim = S.Simulation(P.ski("pol_torus_cart"), packages=100)
    sim.attach(0)
    L = S.lib()
    L.skirt_mcrt_run_phase.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                       ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]

    class Params(ctypes.Structure):
        _fields_ = [("min_weight_reduction", ctypes.c_double), ("min_scatt_events", ctypes.c_int),
                    ("scatt_bias", ctypes.c_double), ("store_absorption", ctypes.c_int), ("has_dust", ctypes.c_int),
                    ("continuous_scattering", ctypes.c_int)]

    p = Params(1e4, 0, 0.5, 0, 1, 1)
    assert L.skirt_mcrt_run_phase(sim.engine, 0, 0, 100, 0, 200, 1, ctypes.byref(p)) == 5  # SKIRT_ERR_UNSUPPORTED
    assert b"continuous scattering is not supported with polarised" in L.skirt_mcrt_last_error(sim.engine)
    p = Params(1e4, 0, 0.5, 0, 1, 0)
    assert L.skirt_mcrt_run_phase(sim.engine, 1, 0, 100, 0, 200, 1, ctypes.byref(p)) == 5
    assert b"dust emission phases are not supported with polarised" in L.skirt_mcrt_last_error(sim.engine)


# ---------------------------------------------------------------- 4. unchanged ground
@pytest.mark.parametrize("name,nslots", [("c1_oligo16", 7), ("pan_oct", 6)])
def test_unpolarised_models_keep_their_shapes(name, nslots):
    """a FullInstrument without polarisation: 5 slots + its scattering levels, as before. The comparison of the
    tallies with the parent commit's library on the same seed is recorded in profiles/pol_first.txt: the same shapes
    and counts, the sums equal to 3e-16 .. 4e-15 of the largest value and not bit for bit, which is the order of the
    f64 atomics and differs as much between two runs of one library"""
    sim = S.Simulation(P.ski(name), packages=2000)
    assert not sim.polarization and sim.stokes(0) == (None, None)
    sim.attach(0)
    sim.run_stellar()
    sim.fetch()
    frames, seds = sim.instrument(0)
    assert seds.shape == (nslots, sim.info.nlambda) and frames.shape[:2] == (nslots, sim.info.nlambda)
    assert seds.sum() > 0
