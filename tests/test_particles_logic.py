"""The host's particle dust (skirt_amd/csrc/host/particles.hpp over device/particle_density.hpp) against the
plain-Python restatement (particles_ref.py), bit for bit: the particle grid's separators, the density at 10^4 random
and the adversarial points, the mass in 10^4 random and the adversarial boxes (one cell; 2, 8, 27 and 64 cells; beyond
the device's merge cap; the whole grid; zero width; table index 4999 / 5000), and the same through the CPU build of
the device header (tools/particle_density_cpu.py), with its handed-back count. No GPU."""
import os
import sys

import numpy as np
import pytest

import particles_ref as R
import skirt_amd as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
PART = os.path.join(GOLD, "particles")
sys.path.insert(0, os.path.join(REPO, "tools"))

_CACHE = {}


def setup(model, file):
    """(the host simulation, the restatement, the adversarial points, the boxes within and beyond the cap), once"""
    if model not in _CACHE:
        sim = S.Simulation(os.path.join(GOLD, "ski", model + ".ski"), input_path=PART, seed=4357)
        P = R.Particles(os.path.join(PART, file), 0.3, 8e4)
        pts = R.adversarial_points(P, nrandom=10000 if file == "cloud.dat" else 2000)
        within, beyond = R.adversarial_boxes(P) if file != "few.dat" else (None, None)
        _CACHE[model] = (sim, P, pts, within, beyond)
    return _CACHE[model]


MODELS = [("part_oct", "cloud.dat"), ("part_oct_neg", "cloud_neg.dat"), ("part_few", "few.dat")]


@pytest.mark.parametrize("model,file", MODELS)
def test_grid_and_counts_equal_the_restatement(model, file):
    sim, P, _, _, _ = setup(model, file)
    info = sim.particle_info()
    assert info["nparticles"] == P.n and info["nignored"] == P.nignored
    assert info["mass_interface"] == (not P.negative)
    np.testing.assert_array_equal(info["separators"], np.array(P.sep))
    if file == "few.dat":  # the equal-count cuts ran out: zero-filled separators remain, the array is not sorted
        inner = info["separators"][:, 1:-1]
        assert np.any(inner == 0.0) and np.any(np.diff(inner, axis=1) < 0)
    else:
        assert np.all(np.diff(info["separators"][:, 1:-1], axis=1) > 0) and P.nignored == 99


@pytest.mark.parametrize("model,file", MODELS)
def test_host_density_equals_the_restatement_bit_for_bit(model, file):
    sim, P, pts, _, _ = setup(model, file)
    got = sim.particle_density(pts)
    want = np.array([P.density(*map(float, p)) for p in pts])
    np.testing.assert_array_equal(got, want)
    # (few.dat: the random points spread over the 5000 pc that its far particle spans; those at kernel radii hit)
    assert np.count_nonzero(got) > (len(pts) // 4 if file != "few.dat" else 100) and np.all(got >= 0)


@pytest.mark.parametrize("model,file", MODELS[:2])
def test_host_mass_in_box_equals_the_restatement_bit_for_bit(model, file):
    sim, P, _, within, beyond = setup(model, file)
    for boxes in (within, beyond):
        got, back = sim.particle_mass_in_box(boxes)
        assert back == 0  # the host hands nothing back
        want = np.array([P.mass_in_box([float(t) for t in b]) for b in boxes])
        np.testing.assert_array_equal(got, want)
    spans = np.array([P.spanned([float(t) for t in b]) for b in within])
    assert spans.max() == S.particle_merge_cap() and {1, 2, 8, 27, 64} <= set(spans.tolist())
    assert min(P.spanned([float(t) for t in b]) for b in beyond) > S.particle_merge_cap()
    whole, _ = sim.particle_mass_in_box(beyond[-1:])
    if not P.negative:  # the whole grid holds every particle's mass, but for the table's 1 - erf(2.5) steps
        np.testing.assert_allclose(whole[0], P.mass(), rtol=2e-3)


def test_few_particles_mass_in_box_on_unsorted_separators():
    sim, P, pts, _, _ = setup("part_few", "few.dat")
    rng = np.random.RandomState(3)
    # around the 36 particles at (300, 300, 300) pc, across the separators there and the zero-filled ones
    lo, hi = np.full(3, 230.0 * R.PC), np.full(3, 370.0 * R.PC)
    a, b = lo + rng.rand(500, 3) * (hi - lo), lo + rng.rand(500, 3) * (hi - lo)
    a[::5] = -600.0 * R.PC * rng.rand(100, 3)  # (some reach below zero)
    boxes = np.concatenate([np.minimum(a, b), np.maximum(a, b)], axis=1)
    got, _ = sim.particle_mass_in_box(boxes)
    want = np.array([P.mass_in_box([float(t) for t in bx]) for bx in boxes])
    np.testing.assert_array_equal(got, want)
    assert np.count_nonzero(got) > 50


@pytest.mark.parametrize("model,file", MODELS[:2])
def test_cpu_build_of_the_device_header_equals_the_host(model, file):
    import particle_density_cpu as C
    sim, P, pts, within, beyond = setup(model, file)
    dev = C.Build(os.path.join(PART, file), 0.3, 8e4)
    np.testing.assert_array_equal(dev.density(pts), sim.particle_density(pts))
    m, back = dev.mass_in_box(within)
    assert back == 0
    np.testing.assert_array_equal(m, sim.particle_mass_in_box(within)[0])
    m, back = dev.mass_in_box(beyond)
    assert back == len(beyond) and np.all(m == -1.0)
    both = np.concatenate([within[:50], beyond, within[50:100]])
    m, back = dev.mass_in_box(both)
    assert back == len(beyond)
    keep = m >= 0
    np.testing.assert_array_equal(m[keep], sim.particle_mass_in_box(both[keep])[0])
