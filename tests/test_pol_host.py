"""The host side of polarised scattering (ElectronDustMix) without a device: the Mueller tables and what
DustMix::setupSelfAfter derives from them against the plain-Python restatement (pol_ref.py; same libm, same order),
the Thomson opacity, the set-up's outputs against the reference's own files (tests/golden/ref_pol), the three
refusals, the host's compilation of the scatterings probe, and the writers: Stokes Q, U, V files and SED columns where
the reference puts them."""
import json
import os

import numpy as np
import pytest

import descriptors as D
import pol_ref
import skirt_files as F
import skirt_amd as S
from golden import bench_digest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
REF = os.path.join(GOLD, "ref_pol")


def ski(name):
    return os.path.join(GOLD, "ski", name + ".ski")


def _variant(tmp_path, name, old, new, tag):
    text = open(ski(name)).read()
    assert text.count(old) >= 1
    path = str(tmp_path / (tag + ".ski"))
    open(path, "w").write(text.replace(old, new, 1))
    return path


def test_new_symbols_are_exported():
    new = {"skirt_mcrt_set_mueller", "skirt_mcrt_scatterings", "skirt_sim_polarization", "skirt_sim_scatterings",
           "skirt_host_write_mueller"}
    assert new <= set(S.ABI_SYMBOLS) and all(hasattr(S.lib(), s) for s in new)


@pytest.mark.parametrize("name,nlambda", [("pol_torus_cart", 2), ("pol_pan_cart", 10), ("pol_2comp_sph2", 1)])
def test_described_tables_equal_the_restatement(tmp_path, name, nlambda):
    sim = S.Simulation(ski(name), packages=10)
    assert sim.polarization and sim.info.nlambda == nlambda
    dump = str(tmp_path / "d.bin")
    sim.describe(dump)
    d = D.read(dump)
    nc = sim.info.ncomp
    assert (d["mueller.ncomp"], d["mueller.nlambda"], d["mueller.ntheta"]) == (nc, nlambda, pol_ref.NTHETA)
    mix = pol_ref.electron_mix(nlambda)
    for key in ("S11", "S12", "S33", "S34", "thetaX"):
        got = d["mueller." + key].reshape(nc, nlambda, pol_ref.NTHETA)
        for h in range(nc):
            np.testing.assert_allclose(got[h], np.array(mix[key]), rtol=1e-13, atol=0, err_msg=key)
    np.testing.assert_allclose(d["mueller.pfnorm"].reshape(nc, nlambda), np.array([mix["pfnorm"]] * nc), rtol=1e-13)
    for key, want in zip(("phi", "phi1", "phis", "phic"), pol_ref.phi_tables()):
        assert len(d["mueller." + key]) == pol_ref.NPHI
        np.testing.assert_allclose(d["mueller." + key], np.array(want), rtol=1e-13, atol=0, err_msg=key)
    assert np.all(d["mueller.S34"] == 0) and d["mueller.thetaX"][0] == 0 and d["mueller.thetaX"][pol_ref.NTHETA - 1] == 1
    # Thomson scattering: kappa_ext = kappa_sca = sigma_T / m_e at every wavelength, albedo 1, g = 0
    kappa = pol_ref.SIGMA_THOMSON / pol_ref.MASS_ELECTRON
    np.testing.assert_allclose(d["media.kext"], kappa, rtol=1e-15)
    np.testing.assert_allclose(d["media.ksca"], kappa, rtol=1e-15)
    assert np.all(d["media.albedo"] == 1) and np.all(d["media.g"] == 0)


def test_unpolarised_dump_has_no_new_fields(tmp_path):
    sim = S.Simulation(ski("c1_oligo16"), packages=10)
    assert not sim.polarization and sim.stokes(0) == (None, None)
    dump = str(tmp_path / "d.bin")
    sim.describe(dump)
    assert not [k for k in D.read(dump) if k.startswith("mueller")]
    with pytest.raises(S.SkirtError, match="do not polarise"):
        sim.scatterings(np.zeros((1, 12)), np.zeros((1, 2)), 0)


def test_cell_properties_equal_the_reference_file(tmp_path):
    """ds_cellprops (volume, density, mass fraction and optical depth of every cell, so the mix's kappa as well) equals
    the reference's file row for row (its digest). ds_convergence comes from the engine's walk: test_gpu_pol.py."""
    name = "pol_torus_cart"
    sim = S.Simulation(ski(name), packages=10)
    sim.write(str(tmp_path / "o"))
    have = bench_digest.cellprops_digest(str(tmp_path / "o_ds_cellprops.dat"))
    want = json.load(open(os.path.join(REF, name + "_s4357_ds_cellprops_digest.json")))
    assert have["rows"] == want["rows"] == 4096
    assert have["sha256"] == want["sha256"]


def test_mixed_polarising_and_other_components_are_refused(tmp_path):
    path = _variant(tmp_path, "pol_2comp_sph2", '<ElectronDustMix writeMix="false" writeMeanMix="false"/>',
                    '<SimpleOligoDustMix opacities="40 m2/kg" albedos="0.6" asymmetryParameters="0.5"/>', "mixed")
    with pytest.raises(S.SkirtError, match="All dust mixes must consistenly support polarization, or not support polarization"):
        S.Simulation(path, packages=10)


def test_continuous_scattering_with_polarisation_is_refused(tmp_path):
    path = _variant(tmp_path, "pol_torus_cart", 'continuousScattering="false"', 'continuousScattering="true"', "cs")
    with pytest.raises(S.SkirtError, match="continuous scattering is not supported with polarised dust mixes"):
        S.Simulation(path, packages=10)


def test_dust_emission_with_polarisation_is_refused(tmp_path):
    path = _variant(tmp_path, "pol_pan_cart", "</dustGrid>",
                    '</dustGrid>\n<dustEmissivity type="DustEmissivity"><GreyBodyDustEmissivity/></dustEmissivity>'
                    '<dustLib type="DustLib"><AllCellsDustLib/></dustLib>', "emis")
    with pytest.raises(S.SkirtError, match="dust emission is not supported with polarised dust mixes"):
        S.Simulation(path, packages=10)


def test_host_probe_equals_the_restatement(tmp_path):
    """Simulation.scatterings(device=None): the host's compilation of the engine's routines on the model's own
    tables and instrument axes, on the logic test's states (test_pol_logic.py holds the argument for the bounds)"""
    sim = S.Simulation(ski("pol_torus_cart"), packages=10)
    dump = str(tmp_path / "d.bin")
    sim.describe(dump)
    d = D.read(dump)
    mixes = [pol_ref.electron_mix(2)]
    for i, angles in ((0, (30.0, 0.0, 0.0)), (1, (90.0, 40.0, 25.0))):
        kobs = d["instrument%d.kobs" % i]
        _, ky = pol_ref.instrument_axes(*angles)
        states, devs = pol_ref.make_states(mixes, 2, tuple(kobs))
        del pol_ref.INDEX_ARGS[:]
        want = pol_ref.probe(mixes, states, devs, kobs, ky)
        assert pol_ref.near_integer_count() == 0
        got = sim.scatterings(states, devs, i)
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)
    with pytest.raises(S.SkirtError, match="out of range"):
        bad = states[:1].copy()
        bad[0, 11] = 1
        sim.scatterings(bad, devs[:1], 0)


def test_writers_put_the_stokes_arrays_where_the_reference_does(tmp_path):
    name = "pol_torus_cart"
    sim = S.Simulation(ski(name), packages=10)
    nl = 2
    blocks = []
    for i, nslots in ((0, 9), (1, 8)):  # 5 + levels + Q, U, V
        frames, seds = sim.instrument(i)
        assert frames.shape == (nslots, nl, 256) and seds.shape == (nslots, nl)
        q, sq = sim.stokes(i)
        assert q.shape == (3, nl, 256) and sq.shape == (3, nl)
        # (luminosities of a galaxy's order, W: the frames are written as 32-bit floats)
        f = (np.arange(frames.size, dtype=np.float64).reshape(frames.shape) + 1.0) * 1e30
        s = -(np.arange(seds.size, dtype=np.float64).reshape(seds.shape) + 1.0) * (i + 1) * 1e30
        blocks += [f.ravel(), s.ravel()]
    sim.set_tallies(instr=np.concatenate(blocks))
    prefix = str(tmp_path / "w")
    sim.write(prefix)
    for i, (ins, nslots, levels) in enumerate((("i30", 9, 1), ("i90", 8, 0))):
        ref_sed = os.path.join(REF, "%s_s4357_%s_sed.dat" % (name, ins))
        head = [ln for ln in open(ref_sed) if ln.startswith("#")]
        assert [ln for ln in open("%s_%s_sed.dat" % (prefix, ins)) if ln.startswith("#")] == head
        assert len(head) == 10 + levels and "column 8: total Stokes Q" in head[7] and "column 10: total Stokes V" in head[9]
        got, ref = F.read_text_table("%s_%s_sed.dat" % (prefix, ins)), F.read_text_table(ref_sed)
        assert got.shape == ref.shape
        # the known tallies: Stokes slots follow the levels in the tally and precede them in the file; signs survive
        seds = sim.instrument(i)[1]
        stokes, scattered = seds[5 + levels:], seds[2]
        np.testing.assert_allclose(got[:, 7:10] / got[:, 3:4], (stokes / scattered).T, rtol=1e-7)
        if levels:
            np.testing.assert_allclose(got[:, 10] / got[:, 3], seds[5] / scattered, rtol=1e-7)
        kinds = ["total", "direct", "scattered", "transparent", "stokesQ", "stokesU", "stokesV"]
        kinds += ["scatteringlevel%d" % (k + 1) for k in range(levels)]
        written = sorted(n for n in os.listdir(str(tmp_path)) if n.startswith("w_%s_" % ins) and n.endswith(".fits"))
        assert written == sorted("w_%s_%s.fits" % (ins, k) for k in kinds)
        assert written == sorted("w_" + n[len(name + "_s4357_"):] for n in os.listdir(REF)
                                 if n.startswith("%s_s4357_%s_" % (name, ins)) and n.endswith(".fits"))
        for k in kinds:
            a = F.read_fits("%s_%s_%s.fits" % (prefix, ins, k))
            b = F.read_fits(os.path.join(REF, "%s_s4357_%s_%s.fits" % (name, ins, k)))
            assert a.shape == b.shape == (nl, 16, 16)
        fq = F.read_fits("%s_%s_stokesU.fits" % (prefix, ins))
        fs = F.read_fits("%s_%s_scattered.fits" % (prefix, ins))
        frames = sim.instrument(i)[0]
        np.testing.assert_allclose((fq / fs).reshape(nl, 256), frames[5 + levels + 1] / frames[2], rtol=1e-5)
