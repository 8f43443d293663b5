"""Rays queued as 16-byte slot references (RayRef): the trace lane reads a ray's origin, direction and luminosity
from its packet slot's state instead of from a record of its own.

The other GPU tests run with the default pool, which holds every packet of their small phases at once: a FILL ray's
queue position then mostly follows its slot, and most models have one instrument. These cases cover the rest:

* a pool far smaller than the phase, so that slots are reclaimed many times, the active list goes ragged and a
  ray's queue position has nothing to do with its slot -- also with every odd slot falling back to a queued WALK ray
  (SKIRT_AMD_FUSE_WALK=2), whose optical depth then comes from the slot as well, and through the dust phases, where
  the origin is a dust cell's and the emission phase runs the kernel without Labs adds;
* four instruments, one of which drops the peel-offs outside its field of view: several rays share one slot's state,
  a varying number per visit, and each takes its direction from its own instrument.

The packets, their random streams and their paths do not depend on the pool: every count is equal and the tallies
agree up to the order of the f64 atomic additions. The four-instrument model is compared with the oracle on the same
Philox streams, by the tolerance and outlier rule of test_engine_matches_oracle_same_streams.
"""
import numpy as np
import pytest

import oracle_lib as O
from parity import STELLAR_OUTLIERS, assert_parity
import skirt_amd as S
from test_gpu_parity import _assert_same_packets, ski

pytestmark = pytest.mark.gpu

SMALL_POOL = 1024  # slots; the engine's minimum is 64, the phases below shoot 5000 packets or more

_cache = {}  # finished runs, shared between the tests (read only)


def _run(monkeypatch, name, packages, dust=False, slots=0, fuse=None):
    key = (name, packages, dust, slots, fuse)
    if key not in _cache:
        if fuse is None:
            monkeypatch.delenv("SKIRT_AMD_FUSE_WALK", raising=False)
        else:
            monkeypatch.setenv("SKIRT_AMD_FUSE_WALK", fuse)
        sim = S.Simulation(ski(name), packages=packages)
        sim.attach(0)
        if slots:
            sim.configure(slots=slots)
        sim.run_stellar()
        if dust:
            sim.run_dust()
        sim.fetch()
        _cache[key] = sim
    return _cache[key]


@pytest.mark.parametrize("fuse", [None, "2"])
@pytest.mark.parametrize("name", ["pan_oct", "pan_cart16"])
def test_reused_slots_do_not_change_results(name, fuse, monkeypatch):
    """2000 packages per wavelength through 1024 slots against the default pool."""
    whole = _run(monkeypatch, name, 2000, fuse=fuse)
    small = _run(monkeypatch, name, 2000, slots=SMALL_POOL, fuse=fuse)
    print(name, fuse, "packets", whole.stats()["packets"], "iterations", whole.stats()["iterations"],
          small.stats()["iterations"])
    assert whole.stats()["packets"] > 4 * SMALL_POOL
    assert small.stats()["iterations"] > whole.stats()["iterations"]  # (the slots were indeed reused)
    _assert_same_packets(whole, small)


def test_reused_slots_in_the_dust_phases(monkeypatch):
    """Self-absorption and dust emission (launchCell origins; the no-store kernel) through 1024 slots."""
    whole = _run(monkeypatch, "pan_oct_sa", 500, dust=True)
    small = _run(monkeypatch, "pan_oct_sa", 500, dust=True, slots=SMALL_POOL)
    # (every phase shoots 500 packets at each wavelength with a luminosity: several times the pool)
    print("packets", whole.stats()["packets"], "trace launches of all phases", whole.stats()["trace_launches"],
          small.stats()["trace_launches"])
    assert small.stats()["trace_launches"] > whole.stats()["trace_launches"]  # (the slots were indeed reused)
    _assert_same_packets(whole, small)


def test_four_instruments_match_oracle_same_streams(monkeypatch):
    """Full, Simple, SED and Frame instruments on pan_oct's model; the frame sees 400 pc of the 1000 pc grid."""
    name, packages, bins = "pan_oct_4instr", 2000, 4096
    monkeypatch.delenv("SKIRT_AMD_FUSE_WALK", raising=False)
    sim = S.Simulation(ski(name), packages=packages)
    sim.attach(0)
    sim.set_crossed(bins)  # the cells-crossed histogram: one count per FILL and per peel-off path
    sim.zero_tallies()
    sim.run_stellar()
    sim.fetch()
    orc = O.run(ski(name), rng=O.RNG_PHILOX, threads=16, packages=packages)
    st = sim.stats()
    assert st["packets"] == orc.packets
    assert sim.info.ninstruments == 4 and len(orc.frames) == 4
    # Detections: the oracle keeps no count of them, but it counts every path it builds. The same histogram of
    # segments per path means the same number of FILL plus peel-off paths, with the same segments; the engine's
    # own count of detections then lies between 3 and 4 per FILL path, as the frame instrument drops some
    got = {k: st[k] for k in ("segments_fill", "segments_peel", "absorb_adds")}
    assert got == {"segments_fill": orc.segments_fill, "segments_peel": orc.segments_peel, "absorb_adds": orc.absorb_adds}
    hist = sim.crossed(bins)
    n = len(orc.crossed)
    np.testing.assert_array_equal(hist[:n], orc.crossed)
    assert hist[n:].sum() == 0
    fills = int(hist.sum()) - st["detects"]
    print("paths %d, detections %d, FILL paths %d" % (hist.sum(), st["detects"], fills))
    assert 3 * fills < st["detects"] < 4 * fills
    # the frame instrument loses peel-offs: its frame holds less than the FullInstrument's total frame
    full_total, frame_total = orc.frames[0][0].sum(), orc.frames[3][0].sum()
    print("oracle frame totals: full %.6g, frame instrument %.6g" % (full_total, frame_total))
    assert 0 < frame_total < full_total
    labs = sim.labs()
    np.testing.assert_allclose(labs.sum(axis=0), orc.labs.sum(axis=0), rtol=1e-9)
    assert_parity(labs, orc.labs, 1e-9, STELLAR_OUTLIERS, "labs")
    for i in range(4):
        frames, seds = sim.instrument(i)
        assert (seds is None) == (orc.seds[i] is None) and (frames is None) == (orc.frames[i] is None)
        if seds is not None:
            np.testing.assert_allclose(seds, orc.seds[i], rtol=1e-9, atol=1e-300)
        if frames is not None:
            np.testing.assert_allclose(frames.sum(axis=2), orc.frames[i].sum(axis=2), rtol=1e-9, atol=1e-300)
            assert_parity(frames, orc.frames[i], 1e-9, STELLAR_OUTLIERS, "frames %d" % i)
    # detections: the engine's count is one for all instruments; the oracle counts peel-off paths with segments
    small = _run(monkeypatch, name, packages, slots=SMALL_POOL)
    _assert_same_packets(sim, small)
    assert st["detects"] == small.stats()["detects"] > 3 * st["packets"]
