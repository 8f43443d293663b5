"""Test support: the reference's paths through the two spherical dust grids, restated in plain Python.

Written from the routines' descriptions (Sphere1DDustGrid::path, SKIRTcore/Sphere1DDustGrid.cpp:111-187, and
Sphere2DDustGrid::path with its two smallestPositiveSolution forms, SKIRTcore/Sphere2DDustGrid.cpp:186-359, of
SKIRT 7.3), as cyl2d_ref.py restates the cylindrical grid's. Python floats are IEEE doubles and each line below is
one reference statement, so the segments equal the reference's up to the compiler's choice of operations. Where
compiled code yields a NaN or an infinity (the square root of a negative number, a division by zero) Python raises,
so those two operations go through helpers that return what the hardware returns. Also the rays and grids that
the CPU and GPU tests share.
"""
import math

import numpy as np

NAN = float("nan")
INF = float("inf")
DBL_MAX = 1.7976931348623157e308


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else NAN  # (NaN too: the comparison is false)


def _div(a, b):
    if b != 0.0:  # (a NaN divisor too)
        return a / b
    if a != a or a == 0.0:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def locate_basic(xv, x, n):
    jl, ju = -1, n
    while ju - jl > 1:
        jm = (ju + jl) >> 1
        if x < xv[jm]:
            ju = jm
        else:
            jl = jm
    return jl


def locate_clip(xv, x):
    if x < xv[0]:
        return 0
    return locate_basic(xv, x, len(xv) - 1)


def locate_fail(xv, x):
    if x > xv[-1]:
        return -1
    return locate_basic(xv, x, len(xv) - 1)


def _add(segs, m, ds):  # DustGridPath::addSegment
    if ds > 0:
        segs.append((m, ds))


# ---------------------------------------------------------------- Sphere1D
def whichcell1(rv, x, y, z):
    return locate_fail(rv, math.sqrt(x * x + y * y + z * z))


def path1(rv, rmax, pos, direction):
    """[(m, ds)] of the Sphere1DDustGrid path from pos along direction; m = -1 outside the grid; [] for an empty
    path. rv: the N_r + 1 radial borders; rmax: maxR()."""
    Nr = len(rv) - 1
    segs = []
    x, y, z = pos
    kx, ky, kz = direction
    r = math.sqrt(x * x + y * y + z * z)
    q = x * kx + y * ky + z * kz
    p = _sqrt((r - q) * (r + q))
    if r > rmax:
        if q > 0.0 or p > rmax:
            return []
        r = rmax - 1e-8 * (rv[Nr] - rv[Nr - 1])
        qmax = _sqrt((rmax - p) * (rmax + p))
        ds = qmax - q
        _add(segs, -1, ds)
        q = qmax
    i = locate_clip(rv, r)
    if q < 0.0:
        imin = locate_clip(rv, p)
        rN = rv[i]
        qN = -_sqrt((rN - p) * (rN + p))
        while i > imin:
            _add(segs, i, qN - q)
            i -= 1
            q = qN
            rN = rv[i]
            qN = -_sqrt((rN - p) * (rN + p))
    rN = rv[i + 1]
    qN = _sqrt((rN - p) * (rN + p))
    while True:
        _add(segs, i, qN - q)
        i += 1
        if i >= Nr - 1:
            return segs
        q = qN
        rN = rv[i + 1]
        qN = _sqrt((rN - p) * (rN + p))


# ---------------------------------------------------------------- Sphere2D
def theta_grid(tt):
    """(thetav, cv) as Sphere2DDustGrid::setupSelfAfter makes them from a unit mesh tt: exact cosines at the poles,
    a cosine within 1e-9 of zero made zero, and a border at pi/2 inserted where there is none"""
    N = len(tt) - 1
    thv = [t * math.pi for t in tt]
    cv = [math.cos(t) for t in thv]
    cv[0] = 1.0
    cv[N] = -1.0
    zeroes = 0
    for k in range(1, N):
        if abs(cv[k]) < 1e-9:
            zeroes += 1
            cv[k] = 0.0
    if zeroes > 1:
        raise ValueError("There are multiple grid points very close to pi/2")
    if zeroes == 0:
        oth, oc = thv, cv
        N += 1
        thv = [math.pi / 2] * (N + 1)
        cv = [0.0] * (N + 1)
        for k in range(N):
            target = k if oc[k] > 0 else k + 1
            thv[target] = oth[k]
            cv[target] = oc[k]
    return thv, cv


def _spherical(x, y, z):  # Position::spherical: r and theta
    r = math.sqrt(x * x + y * y + z * z)
    theta = 0.0 if r == 0 else math.acos(z / r)
    return r, theta


def whichcell2(rv, thv, x, y, z):
    r, theta = _spherical(x, y, z)
    i = locate_fail(rv, r)
    if i < 0:
        return -1
    return locate_clip(thv, theta) + (len(thv) - 1) * i


def _sps2(b, c):  # smallest positive solution of x^2 + 2 b x + c = 0, or 0
    if b * b > c:
        if b > 0:
            if c < 0:
                x1 = -b - math.sqrt(b * b - c)
                return c / x1
        else:
            x2 = -b + math.sqrt(b * b - c)
            if c > 0:
                x1 = c / x2
                if x1 < x2:
                    return x1
            return x2
    return 0.0


def _sps3(a, b, c):  # of a x^2 + 2 b x + c = 0
    if abs(a) > 1e-9:
        return _sps2(b / a, c / a)
    x = _div(-0.5 * c, b)
    if x > 0:
        return x
    return 0.0


def step_cap(Nr, Nt):
    """the engine's bound on a Sphere2D path, in steps (segments and eps nudges alike)"""
    return 4 * (Nr + Nt) + 16


def path2(rv, thv, cv, rmax, pos, direction, cap=None):
    """([(m, ds)], steps) of the Sphere2DDustGrid path: the segments as DustGridPath holds them and the number of
    loop iterations (segments and nudges). cap=None is the reference (no bound on the iterations). As in the
    reference, the exit found by one iteration (inext, knext) is not forgotten by the next: they equal (i, k) except
    after a nudge that changed the cell, and if the iteration after such a nudge finds no exit either, the reference
    adds a segment of DBL_MAX. The device's step starts from (i, k) instead; the two differ on no ray with finite
    components in the tests, and with a NaN direction the reference does not return at all."""
    Nr, Nt = len(rv) - 1, len(thv) - 1
    eps = 1e-11 * rmax
    segs = []
    x, y, z = pos
    kx, ky, kz = direction

    def sphere(radius):
        return _sps2(x * kx + y * ky + z * kz, (x * x + y * y + z * z) - radius * radius)

    def cone(c):
        if c:
            return _sps3(c * c - kz * kz, c * c * (x * kx + y * ky + z * kz) - z * kz,
                         c * c * (x * x + y * y + z * z) - z * z)
        return _div(-z, kz)

    r2 = x * x + y * y + z * z
    if r2 > rmax * rmax:
        ds = sphere(rmax)
        if not ds:
            return [], 0
        _add(segs, -1, ds)
        x += kx * (ds + eps); y += ky * (ds + eps); z += kz * (ds + eps)
    elif r2 == 0:
        x += kx * eps; y += ky * eps; z += kz * eps
    r, theta = _spherical(x, y, z)
    i = locate_fail(rv, r)
    k = locate_clip(thv, theta)
    inext, knext = i, k
    steps = 0
    while i < Nr and i >= 0:
        if cap is not None and steps >= cap:
            break
        steps += 1
        ds = DBL_MAX
        if i > 0:
            s = sphere(rv[i])
            if s > 0 and s < ds:
                ds, inext, knext = s, i - 1, k
        s = sphere(rv[i + 1])
        if s > 0 and s < ds:
            ds, inext, knext = s, i + 1, k
        if k > 0:
            s = cone(cv[k])
            if s > 0 and s < ds:
                ds, inext, knext = s, i, k - 1
        if k < Nt - 1:
            s = cone(cv[k + 1])
            if s > 0 and s < ds:
                ds, inext, knext = s, i, k + 1
        if inext != i or knext != k:
            _add(segs, k + Nt * i, ds)
            x += kx * (ds + eps); y += ky * (ds + eps); z += kz * (ds + eps)
            i, k = inext, knext
        else:
            x += kx * eps; y += ky * eps; z += kz * eps
            r, theta = _spherical(x, y, z)
            i = locate_fail(rv, r)
            k = locate_clip(thv, theta)
    return segs, steps


# ---------------------------------------------------------------- the grids and rays of the tests
PC = 3.08567758e16  # m (Units.cpp)
RMAX = 500.0  # pc


def lin_mesh(n):
    dx = (1.0 - 0.0) / n
    return [0.0 + i * dx for i in range(n + 1)]


def pow_mesh(n, ratio):
    q = math.pow(ratio, 1.0 / (n - 1))
    qn = math.pow(q, n)
    return [0.0 + (1.0 - math.pow(q, i)) / (1.0 - qn) * 1.0 for i in range(n + 1)]


def radial(tr, rmax=RMAX):
    return [t * rmax for t in tr]


def grids1():
    """name -> rv: the Lin and the Pow grid of 20 shells"""
    return {"lin": radial(lin_mesh(20)), "pow": radial(pow_mesh(20, 20.0))}


def grids2():
    """name -> (rv, thv, cv): 12 x 16 (Lin, a border at pi/2) and 12 x 9 (Pow in r; the border is inserted)"""
    return {"lin16": (radial(lin_mesh(12)),) + theta_grid(lin_mesh(16)),
            "pow9": (radial(pow_mesh(12, 20.0)),) + theta_grid(lin_mesh(9))}


def random_rays(n=20000, seed=20261019):
    """origins uniform in [-700, 700]^3 (inside the sphere of 500 and outside it), isotropic directions"""
    rng = np.random.RandomState(seed)
    o = rng.uniform(-700.0, 700.0, size=(n, 3))
    ct = rng.uniform(-1.0, 1.0, size=n)
    ph = rng.uniform(0.0, 2.0 * math.pi, size=n)
    st = np.sqrt(1.0 - ct * ct)
    d = np.stack([st * np.cos(ph), st * np.sin(ph), ct], axis=1)
    return np.concatenate([o, d], axis=1)


def _unit(x, y, z):
    n = math.sqrt(x * x + y * y + z * z)
    return (x / n, y / n, z / n)


C4 = math.cos(4 * (1.0 / 16) * math.pi)  # the cosine of border 4 of the 16-bin polar mesh, as theta_grid has it
# a start whose direction is its own normalised position, found by search: r - q = -2.8e-14 < 0, so p is NaN
NAN_P = (50.0, 90.0, 211.0) + _unit(50.0, 90.0, 211.0)


def explicit_rays():
    """the named cases of the two walks: [(name, (x, y, z, kx, ky, kz))], lengths in pc. 125 pc is a border of both
    Lin grids (5 x 25 pc and 3 x 41.67 pc)."""
    s2 = math.sqrt(0.5)
    sin4 = math.sqrt((1.0 - C4) * (1.0 + C4))
    return [
        # both grids
        ("origin_plus_x", (0.0, 0.0, 0.0, 1.0, 0.0, 0.0)),
        ("origin_plus_z", (0.0, 0.0, 0.0, 0.0, 0.0, 1.0)),
        ("origin_minus_z", (0.0, 0.0, 0.0, 0.0, 0.0, -1.0)),
        ("origin_oblique", (0.0, 0.0, 0.0, 0.48, 0.6, 0.64)),
        ("on_border_outward", (125.0, 0.0, 0.0, 0.6, 0.0, 0.8)),
        ("on_border_inward", (125.0, 0.0, 0.0, -0.6, 0.0, 0.8)),
        ("on_rmax_inward", (500.0, 0.0, 0.0, -0.8, 0.6, 0.0)),
        ("tangent_to_shell", (-300.0, 125.0, 0.0, 1.0, 0.0, 0.0)),
        ("tangent_to_shell_oblique", (-300.0, 75.0, 100.0, 1.0, 0.0, 0.0)),
        ("outside_hitting", (-800.0, 100.0, 50.0, 1.0, 0.0, 0.0)),
        ("outside_grazing", (-800.0, 499.9999999, 0.0, 1.0, 0.0, 0.0)),
        ("outside_missing", (-800.0, 600.0, 0.0, 1.0, 0.0, 0.0)),
        ("outside_pointing_away", (800.0, 0.0, 0.0, 1.0, 0.0, 0.0)),
        ("outside_oblique", (600.0, 0.0, 600.0, -0.6, 0.0, -0.8)),
        # Sphere1D
        ("radial_outward", (100.0, 0.0, 0.0, 1.0, 0.0, 0.0)),
        ("radial_inward_through_centre", (300.0, 0.0, 0.0, -1.0, 0.0, 0.0)),
        ("start_in_outermost_shell", (490.0, 0.0, 0.0, 0.0, 1.0, 0.0)),
        ("start_in_outermost_shell_inward", (490.0, 0.0, 0.0, -0.8, 0.6, 0.0)),
        ("start_in_shell_before_last", (460.0, 0.0, 0.0, 0.0, 1.0, 0.0)),
        ("nan_p", NAN_P),
        # Sphere2D
        ("along_plus_z", (30.0, 40.0, -100.0, 0.0, 0.0, 1.0)),
        ("along_minus_z", (30.0, 40.0, 100.0, 0.0, 0.0, -1.0)),
        ("on_axis_from_outside", (0.0, 0.0, -650.0, 0.0, 0.0, 1.0)),
        ("in_xy_plane_kz_zero", (-300.0, 55.0, 0.0, 1.0, 0.0, 0.0)),
        ("kz_zero_above_plane", (-300.0, 55.0, 21.0, 0.8, 0.6, 0.0)),
        ("kz_zero_from_outside", (-650.0, 120.0, -140.0, 0.8, 0.6, 0.0)),
        ("crossing_xy_plane", (100.0, 50.0, 80.0, 0.0, 0.6, -0.8)),
        ("through_origin", (-200.0, -100.0, -50.0) + _unit(2.0, 1.0, 0.5)),
        ("kz_plus_border_cosine", (100.0, 20.0, 90.0, sin4, 0.0, C4)),
        ("kz_minus_border_cosine", (100.0, 20.0, 90.0, -sin4, 0.0, -C4)),
        ("kz_border_cosine_lower_half", (100.0, 20.0, -90.0, 0.0, sin4, C4)),
        ("cap_cell_top", (5.0, 5.0, 300.0, s2, 0.0, -s2)),
        ("cap_cell_bottom", (5.0, -5.0, -300.0, 0.0, s2, s2)),
        ("cap_cell_top_upward", (5.0, 5.0, 300.0, 0.0, 0.6, 0.8)),
        ("nan_direction", (100.0, 50.0, 20.0, NAN, 0.0, 1.0)),
        ("nan_direction_outside", (100.0, 50.0, 900.0, NAN, 0.0, -1.0)),
    ]


def all_rays(nrandom=20000):
    """float64 [n, 6]: the random rays, then the explicit cases"""
    ex = np.array([r for _, r in explicit_rays()], dtype=np.float64)
    return np.concatenate([random_rays(nrandom), ex], axis=0)


def finite(rays):
    """mask of the rays without a NaN component (the reference's Sphere2D loop does not return on the others)"""
    return np.all(np.isfinite(rays), axis=1)


def _column(segs, rho):
    segs = [(m, ds) for m, ds in segs if m >= 0]
    if not segs:
        return None
    return math.fsum(rho[m] * ds for m, ds in segs)


def column1(rv, rmax, rho, ray):
    """sum of rho[m] ds over the in-grid segments of a ray, or None if the path crosses no cell"""
    return _column(path1(rv, rmax, tuple(ray[:3]), tuple(ray[3:])), rho)


def column2(rv, thv, cv, rmax, rho, ray):
    """the same through a Sphere2D grid. A ray with a NaN component crosses no cell in the engine (its path ends at
    the step cap without a segment); the reference does not return on it inside the grid."""
    if not all(math.isfinite(v) for v in ray):
        return None
    return _column(path2(rv, thv, cv, rmax, tuple(ray[:3]), tuple(ray[3:]))[0], rho)
