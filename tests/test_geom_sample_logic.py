"""The device's geometry samplers (skirt_amd/csrc/device/geom_sample.hpp) compiled for the CPU
(tools/geom_sample_cpu.py): 20,000 positions per kind on the engine's per-packet Philox streams against the host
library's position templates on the same streams -- identical draw counts, so that not one rejection decision
differs and the loops' cap hides nothing, and equal coordinates -- and the densities at those positions and at
points on and beside every cut (r = rmin, rmax, rcut, |cos theta| = sin Delta) against the plain-Python restatement
of the reference (geom_ref.py). No GPU."""
import math
import os
import sys

import numpy as np
import pytest

import geom_ref as R
import skirt_amd as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import geom_sample_cpu as G  # noqa: E402

PC = 3.08567758e16
N = 20000
ELEMENTS = {
    "shell": '<ShellGeometry minRadius="50 pc" maxRadius="400 pc" expon="2"/>',
    "gamma": '<GammaGeometry scale="100 pc" gamma="1"/>',
    "gaussian": '<GaussianGeometry dispersion="100 pc" flattening="0.5"/>',
    "ttauri": '<TTauriDiskGeometry minRadius="20 pc" maxRadius="400 pc" radialScale="100 pc" axialScale="10 pc"/>',
    "torus": '<TorusGeometry expon="1" index="0" openAngle="50 deg" minRadius="50 pc" maxRadius="400 pc" '
             'anisoRadius="true" cutRadius="30 pc"/>',
    "cone": '<ConicalShellGeometry expon="1" index="2" inAngle="20 deg" outAngle="50 deg" minRadius="50 pc" '
            'maxRadius="400 pc" anisoRadius="false" cutRadius="0 pc"/>',
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return G.build(str(tmp_path_factory.mktemp("geom_cpu")))


def _metres(g):
    g = dict(g)
    for k in ("rmin", "rmax", "rcut", "b", "sigma", "Rinn", "Rout", "Rd", "zd"):
        if k in g:
            g[k] = g[k] * PC
    return R.setup(g)


def _host(tmp_path, kind):
    text = open(os.path.join(REPO, "tests", "golden", "ski", "free_shell.ski")).read()
    start = text.index("<ShellGeometry")
    path = tmp_path / (kind + ".ski")
    path.write_text(text[:start] + ELEMENTS[kind] + text[text.index("/>", start) + 2:])
    return S.Simulation(str(path))


def _cut_points(g, rng):
    """2,000 points on and beside the geometry's cuts: radii at each cut radius times 1 -+ {0, 1e-15, 1e-9, 1e-3},
    polar angles at each cut angle likewise, and random ones"""
    k = g["kind"]
    radii = {"shell": ["rmin", "rmax"], "ttauri": ["Rinn", "Rout"], "torus": ["rmin", "rmax", "rcut"],
             "cone": ["rmin", "rmax"]}.get(k, [])
    scale = R.outer_scale(g)
    f = np.array([1.0, 1 - 1e-15, 1 + 1e-15, 1 - 1e-9, 1 + 1e-9, 1 - 1e-3, 1 + 1e-3])
    rs = np.concatenate([g[n] * f for n in radii] + [scale * np.array([1e-3, 0.1, 0.5, 0.9, 1.5])])
    cuts = {"torus": [g.get("sinDelta")], "cone": [g.get("sinDeltaOut"), g.get("sinDeltaIn")]}.get(k, [])
    cts = np.concatenate([c * f for c in cuts] + [np.array([0.0, 0.05, 0.3, 0.6, 0.95, 1.0])])
    cts = np.concatenate([cts, -cts])
    pts = []
    while len(pts) < 2000:
        r = rs[rng.integers(len(rs))]
        ct = min(1.0, max(-1.0, cts[rng.integers(len(cts))]))
        phi = 2 * math.pi * rng.random()
        st = math.sqrt((1 - ct) * (1 + ct))
        if k == "ttauri":  # the cuts are in the cylindrical radius
            pts.append((r * math.cos(phi), r * math.sin(phi), scale * 0.05 * (rng.random() - 0.5)))
        else:
            pts.append((r * st * math.cos(phi), r * st * math.sin(phi), r * ct))
    return np.array(pts)


@pytest.mark.parametrize("example", R.EXAMPLES, ids=[e["kind"] for e in R.EXAMPLES])
def test_device_header_on_the_cpu_equals_the_host_and_the_restatement(tmp_path, exe, example):
    g = _metres(example)
    gp, tab = R.params(g)
    code = R.KIND_CODE[g["kind"]]
    pos, draws, ok, _ = G.sample(exe, code, gp, tab, N, str(tmp_path), seed=11, first=3)
    assert np.all(ok == 1)
    hpos, hdraws = _host(tmp_path, g["kind"]).positions(0, N, seed=11, first=3)
    # identical draw counts: zero flipped rejections among N packets
    np.testing.assert_array_equal(draws, hdraws)
    np.testing.assert_allclose(pos, hpos, rtol=1e-12, atol=1e-12 * R.outer_scale(g))
    if g["kind"] == "cone":
        assert draws.mean() > 3
    # densities at the sampled positions and on and beside the cuts, against the restatement
    pts = np.concatenate([pos[:2000], _cut_points(g, np.random.default_rng(5))])
    _, _, _, dens = G.sample(exe, code, gp, tab, 0, str(tmp_path), points=pts)
    want = np.array([R.density(g, *p) for p in pts])
    np.testing.assert_array_equal(dens == 0, want == 0)
    np.testing.assert_allclose(dens, want, rtol=1e-13, atol=0)
    assert np.all(dens[:2000] > 0)
    assert (want[2000:] == 0).sum() > 100 or g["kind"] in ("gamma", "gaussian")  # the cut points do fall outside


def test_special_functions_cover_their_three_branches(tmp_path, exe):
    """gln / gexp through the shell sampler at expon 3 (q = 0), 3.0005 (|q| < 1e-3) and 1 (general): radii inside
    the shell, equal to the restatement's"""
    for p in (3.0, 3.0005, 2.9995, 1.0, 0.0):
        g = _metres(dict(kind="shell", rmin=50.0, rmax=400.0, p=p))
        gp, tab = R.params(g)
        pos, draws, ok, _ = G.sample(exe, 4, gp, tab, 500, str(tmp_path), seed=2)
        r = np.sqrt((pos ** 2).sum(1))
        assert np.all(draws == 3) and np.all(r > g["rmin"] * (1 - 1e-12)) and np.all(r < g["rmax"] * (1 + 1e-12))
        if abs(3.0 - p) >= 1e-3 or p == 3.0:  # the exact branches invert each other (the series is the reference's own approximation)
            for X in np.linspace(0.01, 0.99, 50):
                s = g["smin"] + X * g["sdiff"]
                np.testing.assert_allclose(R.gln(p - 2.0, R.gexp(p - 2.0, s)), s, rtol=1e-9)


def test_cap_returns_failure_not_a_position(tmp_path, exe):
    """a cone without volume (inner = outer angle): every attempt is rejected, the routine ends at its cap of 2^16
    attempts (3 deviates each) and reports failure; CPU only"""
    g = R.setup(dict(kind="cone", p=1.0, q=0.0, DeltaIn=0.3, DeltaOut=0.3 + 1e-12, rmin=1.0, rmax=2.0))
    g["sinDeltaIn"] = g["sinDeltaOut"]
    gp, tab = R.params(g)
    pos, draws, ok, _ = G.sample(exe, 9, gp, tab, 2, str(tmp_path))
    assert np.all(ok == 0) and np.all(draws == 3 * 65536) and np.all(pos == 0)
