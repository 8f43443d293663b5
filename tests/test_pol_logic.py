"""The device's polarised scattering (skirt_amd/csrc/device/polarization.hpp) compiled for the CPU (tools/pol_cpu.py)
against the plain-Python restatement of the reference (tests/pol_ref.py): one scattering and one scattering peel-off
of 4,096 random packet states and of the explicit ones pol_ref.make_states lists -- directions along and next to the
z axis on both sides of rotateStokes's 0.99999 branch, unpolarised packets, Q = 1, U = -1 and V != 0 with a made-up
mix whose S34 != 0, peel-offs exactly forward and backward, deviates 0, 1 - 2^-53 and entries of thetaX."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pol_cpu  # noqa: E402
import pol_ref  # noqa: E402

NLAMBDA = 2


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pol_cpu"))
    mixes = [pol_ref.electron_mix(NLAMBDA), pol_ref.madeup_mix(NLAMBDA)]
    kobs, ky = pol_ref.instrument_axes(90.0, 40.0, 25.0)
    states, devs = pol_ref.make_states(mixes, NLAMBDA, kobs)
    del pol_ref.INDEX_ARGS[:]
    want = pol_ref.probe(mixes, states, devs, kobs, ky)
    near = pol_ref.near_integer_count()
    got = pol_cpu.run(pol_cpu.build(d), pol_ref.pack(mixes), len(mixes), NLAMBDA, pol_ref.NTHETA, states, devs, kobs,
                      ky, d)
    return states, devs, want, got, near


def test_states_cover_the_branches(case):
    states, devs, want, _, _ = case
    assert len(states) >= pol_ref.N_RANDOM + 100
    kz = states[:, 2]
    for v in (1.0, -1.0, 0.999995, -0.999995, 0.99998, -0.99998):
        assert (kz == v).any()
    assert (states[:, 9] == 0).sum() > 1000 and (states[:, 9] == 1).sum() > 3000
    assert ((states[:, 5] != 0) & (states[:, 11] == 1)).any()  # V != 0 meets S34 != 0
    assert (devs == 0.0).any() and (devs == 1.0 - 2.0 ** -53).any()
    assert (want[:, 5] != 0).any() and (want[:, 13] != 0).any()  # and V comes out of it


def test_no_state_sits_on_a_table_row_boundary(case):
    # a condition of the comparison, not a measurement: no theta / dt + 0.5 within 1e-9 of an integer, where a
    # last-bit difference would pick another row of the Mueller tables; nothing is left out below
    assert case[4] == 0


def test_cpu_build_matches_reference_restatement(case):
    _, _, want, got, _ = case
    assert np.isfinite(want).all() and np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)


def test_results_are_physical(case):
    states, _, want, _, _ = case
    for block in (want[:, 0:3], want[:, 6:9]):
        np.testing.assert_allclose((block ** 2).sum(1), 1.0, rtol=0, atol=1e-14)
    # the normal stays perpendicular to the direction (rotateStokes's first normal next to the z axis, (1, 0, 0),
    # is so only approximately)
    away = np.abs(states[:, 2]) <= 0.99999
    np.testing.assert_allclose((want[:, 0:3] * want[:, 6:9]).sum(1)[away], 0.0, atol=1e-14)
    assert ((want[:, 3:6] ** 2).sum(1) <= 1 + 1e-12).all()
    assert ((want[:, 11:14] ** 2).sum(1) <= 1 + 1e-12).all()
    assert (want[:, 10] >= 0).all()
