"""The spherical grid walks of the device (skirt_amd/csrc/device/sph_walk.hpp) compiled as host C++
(tools/sph_walk_cpu.py) against the plain-Python restatements of Sphere1DDustGrid::path and Sphere2DDustGrid::path
(sph_ref.py).

Required: the same cell sequence for every ray, the m = -1 segments and the empty paths included, the same origin
cell, and every ds within rtol 1e-12 plus atol 1e-12 r_max (the cylinder test's tolerance): both sides do the same
f64 operations per segment in the reference's order, so they differ by the compilers' choice of operations at most.
The Sphere2D walk's step cap (the engine's one choice) must not be reached by any ray with a finite direction."""
import importlib.util
import math
import os

import numpy as np
import pytest

import sph_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12
NAMED = dict(R.explicit_rays())


def _tool():
    spec = importlib.util.spec_from_file_location("sph_walk_cpu", os.path.join(REPO, "tools", "sph_walk_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sph"))
    tool = _tool()
    exe = tool.build(d)
    return lambda rv, rays, thv=None, cv=None, rmax=R.RMAX: tool.walk(exe, rv, rmax, rays, d, thv=thv, cv=cv)


def _split(counts, cells, lens):
    off = np.concatenate([[0], np.cumsum(counts)])
    return [(cells[off[r]:off[r + 1]], lens[off[r]:off[r + 1]]) for r in range(len(counts))]


def _same(got, ref, atol, what):
    got_m, got_ds = got
    assert got_m.tolist() == [m for m, _ in ref], (what, got_m, ref)
    ref_ds = np.array([ds for _, ds in ref])
    assert np.all(np.abs(got_ds - ref_ds) <= atol + RTOL * np.abs(ref_ds)), (what, got_ds, ref_ds)


def _compare1(walker, rv, rays, rmax=R.RMAX):
    counts, where, steps, cells, lens = walker(rv, rays, rmax=rmax)
    for r, (ray, got) in enumerate(zip(rays.tolist(), _split(counts, cells, lens))):
        _same(got, R.path1(rv, rmax, tuple(ray[:3]), tuple(ray[3:])), 1e-12 * rmax, (r, ray))
        assert where[r] == R.whichcell1(rv, *ray[:3]), (r, ray)
    assert steps.max() <= 2 * (len(rv) - 1)  # i moves monotonically in each part: no guard needed
    return counts, steps, cells, lens


def _compare2(walker, grid, rays):
    """the walk with its cap against the restatement without one (the reference), for the rays it returns on; the
    others (a NaN component: the reference spins) must give no segment"""
    rv, thv, cv = grid
    cap = R.step_cap(len(rv) - 1, len(thv) - 1)
    counts, where, steps, cells, lens = walker(rv, rays, thv=thv, cv=cv)
    ok = R.finite(rays)
    for r, (ray, got) in enumerate(zip(rays.tolist(), _split(counts, cells, lens))):
        if not ok[r]:  # no segment; the cap's steps if the loop is entered at all
            inside = ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2] <= R.RMAX * R.RMAX
            assert len(got[0]) == 0 and steps[r] == (cap if inside else 0), (r, ray, got, steps[r])
            continue
        ref, nref = R.path2(rv, thv, cv, R.RMAX, tuple(ray[:3]), tuple(ray[3:]))
        _same(got, ref, 1e-12 * R.RMAX, (r, ray))
        assert steps[r] == nref, (r, ray, steps[r], nref)
        assert where[r] == R.whichcell2(rv, thv, *ray[:3]), (r, ray)
    return counts, steps, cells, lens


@pytest.mark.parametrize("gridname", ["lin", "pow"])
def test_sphere1d_walk_matches_the_restatement(walker, gridname):
    rv = R.grids1()[gridname]
    rays = R.all_rays()
    assert len(rays) == 20000 + len(R.explicit_rays())
    counts, steps, cells, lens = _compare1(walker, rv, rays)
    ray_of = np.repeat(np.arange(len(counts)), counts)
    outside = np.bincount(ray_of[cells < 0], minlength=len(counts))
    assert set(np.unique(outside).tolist()) == {0, 1} and (counts == 0).any()
    # a path that starts at r > r_max crosses no dust
    ingrid = np.bincount(ray_of[cells >= 0], weights=lens[cells >= 0], minlength=len(counts))
    far = np.sqrt((rays[:, :3] ** 2).sum(axis=1)) > rv[-1]
    assert (far & (counts > 0)).sum() > 100 and np.all(ingrid[far] == 0.0)
    assert (ingrid > 0).sum() > 1000


@pytest.mark.parametrize("gridname", ["lin16", "pow9"])
def test_sphere2d_walk_matches_the_restatement(walker, gridname):
    grid = R.grids2()[gridname]
    assert len(grid[1]) - 1 == {"lin16": 16, "pow9": 10}[gridname] and 0.0 in grid[2]
    rays = R.all_rays()
    counts, steps, cells, lens = _compare2(walker, grid, rays)
    ray_of = np.repeat(np.arange(len(counts)), counts)
    ingrid = np.bincount(ray_of[cells >= 0], weights=lens[cells >= 0], minlength=len(counts))
    # unlike the 1D grid's, a path from outside enters on the near side and crosses dust
    far = (rays[:, :3] ** 2).sum(axis=1) > R.RMAX ** 2
    assert (far & (ingrid > 0)).sum() > 1000 and (far & (counts == 0)).sum() > 1000
    # nearly every cell is crossed (the Pow grid's innermost shell is 0.7 pc wide)
    ncells = (len(grid[0]) - 1) * (len(grid[1]) - 1)
    assert len(set(cells[cells >= 0].tolist())) >= 0.95 * ncells and cells.max() == ncells - 1


@pytest.mark.parametrize("gridname", ["lin16", "pow9"])
def test_sphere2d_step_cap_is_never_reached(walker, gridname):
    """the cap of 4 (N_r + N_theta) + 16 steps ends no path of a ray with finite components: the longest one stays
    under the border count 2 (N_r + 1) + 2 (N_theta + 1) it was derived from, and the restatement without a cap
    (compared in _compare2) gives the same paths. Only the rays with a NaN direction inside the grid, on which
    the reference does not return, end at the cap, without a segment."""
    rv, thv, cv = R.grids2()[gridname]
    Nr, Nt = len(rv) - 1, len(thv) - 1
    cap = R.step_cap(Nr, Nt)
    rays = R.all_rays()
    counts, steps, cells, lens = _compare2(walker, (rv, thv, cv), rays)
    ok = R.finite(rays)
    assert steps[ok].max() <= 2 * (Nr + 1) + 2 * (Nt + 1) < cap
    print("%s: longest path %d steps, cap %d" % (gridname, steps[ok].max(), cap))
    nan_in = [i for i in np.flatnonzero(~ok) if (rays[i, :3] ** 2).sum() <= R.RMAX ** 2]
    assert nan_in and all(steps[i] == cap and counts[i] == 0 for i in nan_in)


def test_single_bin_and_small_grids(walker):
    rays = R.all_rays(2000)
    for n in (1, 2, 3):
        _compare1(walker, R.radial(R.lin_mesh(n)), rays)
    for nr, nt in ((1, 1), (1, 2), (3, 1), (2, 5)):
        _compare2(walker, (R.radial(R.lin_mesh(nr)),) + R.theta_grid(R.lin_mesh(nt)), rays)


def test_log_mesh_outer_border_is_not_rmax(walker):
    """maxR(), not the last border, bounds the Sphere1D grid: with the last border one ulp inside r_max the walk and
    the restatement still agree (a start between the two lies in the outermost shell)"""
    rv = R.radial(R.lin_mesh(20))
    rv[-1] = math.nextafter(rv[-1], 0.0)
    rays = np.concatenate([R.all_rays(500), [[R.RMAX, 0.0, 0.0, -0.8, 0.6, 0.0]]])
    _compare1(walker, rv, rays)


def test_reference_behaviours(walker):
    """the behaviours of the reference's routines that the walks reproduce, with worked numbers"""
    rv = R.grids1()["lin"]  # 20 shells of 25 pc
    names1 = ["outside_hitting", "start_in_shell_before_last", "start_in_outermost_shell", "nan_p",
              "radial_inward_through_centre", "outside_grazing"]
    rays = np.array([NAMED[n] for n in names1])
    counts, where, steps, cells, lens = walker(rv, rays)
    seg = dict(zip(names1, _split(counts, cells, lens)))
    # 1. Sphere1D from r > r_max: the outside segment runs to the FAR side, q_max - q with q = -800 and
    #    p^2 = 100^2 + 50^2; then one zero-length segment in the outermost shell (no segment); in-grid length 0
    m, ds = seg["outside_hitting"]
    assert m.tolist() == [-1]
    assert ds[0] == pytest.approx(800.0 + math.sqrt(500.0 ** 2 - 12500.0), rel=1e-14)
    assert ds[0] == pytest.approx(1287.3397, abs=1e-4)
    m, ds = seg["outside_grazing"]
    assert m.tolist() == [-1] and ds[0] == pytest.approx(800.0 + math.sqrt((500.0 - 499.9999999) * 999.9999999), rel=1e-9)
    # 2. the outward loop ends at i >= N_r - 1: from shell 18 the path is the chord to r = 475 and never crosses
    #    shell 19; from shell 19 it crosses that shell once, to r = 500
    m, ds = seg["start_in_shell_before_last"]
    assert m.tolist() == [18] and ds[0] == pytest.approx(math.sqrt(475.0 ** 2 - 460.0 ** 2), rel=1e-14)
    m, ds = seg["start_in_outermost_shell"]
    assert m.tolist() == [19] and ds[0] == pytest.approx(math.sqrt(500.0 ** 2 - 490.0 ** 2), rel=1e-14)
    # 3. p is not clamped: r - q = -2.8e-14 for this radial ray, p is NaN, every q_N and so every ds is NaN and
    #    dropped; the walk ends after the shells from the start's (9: r = 234.8) to N_r - 2
    x, y, z, kx, ky, kz = NAMED["nan_p"]
    r, q = math.sqrt(x * x + y * y + z * z), x * kx + y * ky + z * kz
    assert (r - q) * (r + q) < 0 and R.locate_clip(rv, r) == 9
    assert len(seg["nan_p"][0]) == 0 and steps[names1.index("nan_p")] == 19 - 9 <= 20
    assert R.path1(rv, R.RMAX, (x, y, z), (kx, ky, kz)) == []
    assert R.locate_clip(rv, R.NAN) == 19 and R.locate_fail(rv, R.NAN) == 19  # NR::locate_* on a NaN: the last bin
    #    (an exactly radial ray has p = 0: 300 pc inward through the centre, then out to r = 475; the start lies on
    #    border 12, so shell 12's segment has length zero and is no segment)
    m, ds = seg["radial_inward_through_centre"]
    assert m.tolist() == list(range(11, 0, -1)) + list(range(0, 19))
    assert ds.sum() == pytest.approx(300.0 + 475.0, rel=1e-14)

    # 4. Sphere2D, the 12 x 16 grid: shells of 41.67 pc, polar bins of 11.25 degrees, eps = 5e-9 pc
    grid = R.grids2()["lin16"]
    rv2, thv, cv = grid
    eps = 1e-11 * R.RMAX
    names2 = ["origin_plus_x", "in_xy_plane_kz_zero", "kz_zero_above_plane", "kz_plus_border_cosine", "nan_direction",
              "nan_direction_outside", "outside_hitting"]
    rays = np.array([NAMED[n] for n in names2])
    counts, where, steps, cells, lens = walker(rv2, rays, thv=thv, cv=cv)
    seg = dict(zip(names2, _split(counts, cells, lens)))
    #    the r^2 == 0 nudge: the start moves eps along +x, into the polar bin below the xy-plane's border (theta =
    #    pi/2 belongs to bin 8); eps is added to every advance but not to ds, so the first segment is eps short
    #    of the first border and each later one eps short of a shell's width: the 12 ds sum to r_max - 12 eps
    m, ds = seg["origin_plus_x"]
    assert m.tolist() == [8 + 16 * i for i in range(12)]
    assert ds[0] == pytest.approx(500.0 / 12 - eps, rel=1e-14)
    assert ds.sum() == pytest.approx(500.0 - 12 * eps, rel=1e-14)
    assert 500.0 - ds.sum() == pytest.approx(12 * eps, rel=1e-3)
    #    k_z = 0 in the xy-plane: the plane's candidate -z/k_z is NaN (0/0), above the plane -inf; both are
    #    discarded by s > 0 && s < DBL_MAX, and the cones with c != 0 are not met: the path stays in its polar bin
    assert math.isnan(R._div(-0.0, 0.0)) and R._div(-21.0, 0.0) == -R.INF
    m, ds = seg["in_xy_plane_kz_zero"]
    assert np.all(m % 16 == 8) and ds.sum() == pytest.approx(300.0 + math.sqrt(500.0 ** 2 - 55.0 ** 2), rel=1e-9)
    m, ds = seg["kz_zero_above_plane"]
    assert np.all(m % 16 == 7) and m[-1] // 16 == 11
    #    k_z = c of border 4: a = c^2 - k_z^2 = 0 exactly, the linear branch; the ray (parallel to the cone's
    #    generator through it) meets the cone at x = -c'/(2 b') only if that is positive
    a = R.C4 * R.C4 - rays[3, 5] * rays[3, 5]
    assert abs(a) <= 1e-9
    ray = rays[3].tolist()
    _same(seg["kz_plus_border_cosine"], R.path2(rv2, thv, cv, R.RMAX, tuple(ray[:3]), tuple(ray[3:]))[0],
          1e-12 * R.RMAX, "kz_plus_border_cosine")
    assert len(seg["kz_plus_border_cosine"][0]) >= 2
    #    a NaN direction: from outside the entry finds no intersection (empty path); inside, every candidate is NaN,
    #    the nudged position is NaN, and locate_fail puts a NaN radius in the last shell: the reference's loop
    #    does not return; the walk ends at its cap of 4 (12 + 16) + 16 = 128 steps without a segment
    assert len(seg["nan_direction_outside"][0]) == 0 and steps[names2.index("nan_direction_outside")] == 0
    assert len(seg["nan_direction"][0]) == 0 and steps[names2.index("nan_direction")] == 128 == R.step_cap(12, 16)
    #    (the restatement, stopped after 5 iterations: they nudge and add a segment of DBL_MAX in cell 15 + 16 * 11
    #    in turn, because the reference keeps the stale (inext, knext) of before the nudge)
    ref, nref = R.path2(rv2, thv, cv, R.RMAX, tuple(rays[4, :3].tolist()), tuple(rays[4, 3:].tolist()), cap=5)
    assert nref == 5 and ref == [(191, R.DBL_MAX)] * 2
    #    from outside the near side is entered (unlike Sphere1D): ds = -b - sqrt(b^2 - c) as c / x1
    m, ds = seg["outside_hitting"]
    assert m[0] == -1 and ds[0] == pytest.approx(800.0 - math.sqrt(500.0 ** 2 - 12500.0), rel=1e-12)
    assert ds[1:].sum() == pytest.approx(2 * math.sqrt(500.0 ** 2 - 12500.0), rel=1e-9)
