"""The cylindrical grid walk of the device (skirt_amd/csrc/device/cyl2d_walk.hpp) compiled as host C++
(tools/cyl2d_walk_cpu.py) against the plain-Python restatement of Cylinder2DDustGrid::path (cyl2d_ref.py).

Required: the same cell sequence for every ray, the m = -1 segments and the empty paths included, and every ds
within rtol 1e-12 plus atol 1e-12 R_max: both sides do the same handful of f64 operations per segment, p, q, k_q
and q_N in the reference's order, so they differ by the compilers' choice of operations at most."""
import importlib.util
import os

import numpy as np
import pytest

import cyl2d_ref as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12


def _tool():
    spec = importlib.util.spec_from_file_location("cyl2d_walk_cpu", os.path.join(REPO, "tools", "cyl2d_walk_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cyl2d"))
    tool = _tool()
    exe = tool.build(d)
    return lambda Rv, zv, rays: tool.walk(exe, Rv, zv, rays, d)


def _compare(walker, Rv, zv, rays):
    counts, where, cells, lens = walker(Rv, zv, rays)
    atol = 1e-12 * Rv[-1]
    off = 0
    for r, ray in enumerate(rays):
        ref = C.path(Rv, zv, tuple(ray[:3]), tuple(ray[3:]))
        n = int(counts[r])
        got_m = cells[off:off + n].tolist()
        got_ds = lens[off:off + n]
        off += n
        assert got_m == [m for m, _ in ref], (r, ray.tolist(), got_m, ref)
        ref_ds = np.array([ds for _, ds in ref])
        assert np.all(np.abs(got_ds - ref_ds) <= atol + RTOL * np.abs(ref_ds)), (r, ray.tolist(), got_ds, ref_ds)
        assert where[r] == C.whichcell(Rv, zv, *ray[:3]), (r, ray.tolist())
    return counts, cells, lens


@pytest.mark.parametrize("gridname", ["lin", "pow"])
def test_walk_matches_the_restatement(walker, gridname):
    Rv, zv = C.lin_grid() if gridname == "lin" else C.pow_grid()
    rays = C.all_rays()
    assert len(rays) == 20000 + len(C.explicit_rays())
    counts, cells, lens = _compare(walker, Rv, zv, rays)
    # the rays cover every kind of start: inside, one segment before the grid, empty paths. (No path keeps two
    # outside segments: after the radial one the ray stands on the far side of the cylinder, and a z segment
    # from there ends at R > R_max, which empties the path.)
    ray_of = np.repeat(np.arange(len(counts)), counts)
    outside = np.bincount(ray_of[cells < 0], minlength=len(counts))
    assert set(np.unique(outside).tolist()) == {0, 1}
    assert (counts == 0).any()
    # a path that starts at R >= R_max crosses no dust
    ingrid = np.bincount(ray_of[cells >= 0], weights=lens[cells >= 0], minlength=len(counts))
    far = np.hypot(rays[:, 0], rays[:, 1]) >= Rv[-1]
    assert (far & (counts > 0)).sum() > 100 and np.all(ingrid[far] == 0.0)


@pytest.mark.parametrize("NR,Nz", [(1, 1), (1, 16), (12, 1)])
def test_single_bin_grids(walker, NR, Nz):
    Rv, zv = C.grid(C.lin_mesh(NR), C.lin_mesh(Nz))
    _compare(walker, Rv, zv, C.all_rays(2000))


def test_reference_behaviours(walker):
    """the three behaviours of the reference's routine that the walk reproduces, on the 12 x 16 Lin grid"""
    Rv, zv = C.lin_grid()
    named = dict(C.explicit_rays())
    rays = np.array([named["mirror_up"], named["mirror_down"], named["outside_R_far_side"], named["kz_zero_inside"],
                     named["along_plus_z"], named["origin_minus_z"]])
    counts, where, cells, lens = walker(Rv, zv, rays)
    off = np.concatenate([[0], np.cumsum(counts)])
    seg = [(cells[off[r]:off[r + 1]], lens[off[r]:off[r + 1]]) for r in range(len(rays))]
    # 2. a downward path ends on entering the last radial shell: the mirror image of an upward path is one
    # shell (500/12 pc in R, so 52.0833 pc along the ray) shorter
    assert seg[0][1].sum() == pytest.approx(625.0, rel=1e-12)
    assert seg[1][1].sum() == pytest.approx(625.0 - 625.0 / 12, rel=1e-12)
    assert len(seg[0][0]) == len(seg[1][0]) + 1
    assert seg[0][0][-1] // 16 == 11 and seg[1][0][-1] // 16 == 10
    # 1. a start at R >= R_max: one outside segment to the far side of the cylinder, no dust crossed
    assert seg[2][0][0] == -1
    assert seg[2][1][0] == pytest.approx(800.0 + np.sqrt((500.0 - 100.0) * (500.0 + 100.0)), rel=1e-14)
    assert seg[2][1][0] == pytest.approx(1289.8979, abs=1e-4)
    assert seg[2][1][seg[2][0] >= 0].sum() == 0.0
    # 3. k_z = 0 counts as upward with k_z = 1e-20: the path stays in its z bin and leaves through R_max
    assert np.all(seg[3][0] % 16 == seg[3][0][0] % 16) and seg[3][0][-1] // 16 == 11
    assert seg[3][1].sum() == pytest.approx(300.0 + np.sqrt(500.0**2 - 55.0**2), rel=1e-12)
    # k_q = 0 becomes 1e-20: a vertical ray from below crosses one column of 16 cells, 1000 pc
    assert seg[4][0][0] == -1 and len(seg[4][0]) == 17 and np.all(seg[4][0][1:] // 16 == seg[4][0][1] // 16)
    assert seg[4][1][1:].sum() == pytest.approx(1000.0 - 1e-8 * 62.5, rel=1e-12)  # (the entry steps 1e-8 bins in)
    # a start on a z border going down: the zero-length first segment is no segment (addSegment)
    assert np.all(seg[5][1] > 0) and seg[5][1].sum() == pytest.approx(500.0, rel=1e-12)
