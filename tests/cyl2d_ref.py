"""Test support: the reference's path through an axisymmetric R-z dust grid, restated in plain Python.

Written from the routine's description (Cylinder2DDustGrid::path of SKIRT 7.3, SKIRTcore/Cylinder2DDustGrid.cpp:
135-362), as oracle/oracle.cpp restates the other grids' paths: the entry (a start at R >= R_max, below z_min,
above z_max), then per vertical direction an inward loop down to the shell of the closest approach and an outward
loop. Python floats are IEEE doubles and each line below is one reference statement, so the segments equal the
reference's up to the compiler's choice of operations. Also the rays and grids that the CPU and GPU tests share.
"""
import math

import numpy as np

NAN = float("nan")


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else NAN  # (NaN too: the comparison is false)


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


def whichcell(Rv, zv, x, y, z):
    i = locate_fail(Rv, math.sqrt(x * x + y * y))
    k = locate_fail(zv, z)
    if i < 0 or k < 0:
        return -1
    return k + (len(zv) - 1) * i


def path(Rv, zv, pos, direction):
    """[(m, ds)] of the path from pos along direction; m = -1 outside the grid; [] for an empty path.
    Rv, zv: sequences of floats, the N_R + 1 radial and N_z + 1 vertical borders (R_max = Rv[-1] etc.)."""
    NR, Nz = len(Rv) - 1, len(zv) - 1
    segs = []

    def add(m, ds):  # DustGridPath::addSegment
        if ds > 0:
            segs.append((m, ds))

    kx, ky, kz = direction
    x, y, z = pos
    kq = math.sqrt(kx * kx + ky * ky)
    if kz == 0.0:
        kz = 1e-20
    if kq == 0.0:
        kq = 1e-20
    R = math.sqrt(x * x + y * y)
    q = (x * kx + y * ky) / kq
    p2 = (R - q) * (R + q)
    p = math.sqrt(p2 if 0.0 < p2 else 0.0)  # std::max(0.0, p2)
    Rmax, zmin, zmax = Rv[NR], zv[0], zv[Nz]

    if R >= Rmax:
        if q > 0.0 or p > Rmax:
            return []
        R = Rmax - 1e-8 * (Rv[NR] - Rv[NR - 1])
        qmax = _sqrt((Rmax - p) * (Rmax + p))
        ds = (qmax - q) / kq
        add(-1, ds)
        q = qmax
        z += kz * ds
    if z < zmin:
        if kz <= 0.0:
            return []
        ds = (zmin - z) / kz
        add(-1, ds)
        q += kq * ds
        R = _sqrt(p * p + q * q)
        z = zmin + 1e-8 * (zv[1] - zv[0])
    elif z > zmax:
        if kz >= 0.0:
            return []
        ds = (zmax - z) / kz
        add(-1, ds)
        q += kq * ds
        R = _sqrt(p * p + q * q)
        z = zmax - 1e-8 * (zv[Nz] - zv[Nz - 1])
    if math.isinf(R) or math.isnan(R) or math.isinf(z) or math.isnan(z) or R >= Rmax or z <= zmin or z >= zmax:
        return []

    i = locate_clip(Rv, R)
    k = locate_clip(zv, z)

    def index(i, k):
        return k + Nz * i

    if kz >= 0.0:  # upward
        if q < 0.0:
            imin = locate_clip(Rv, p)
            RN = Rv[i]
            qN = -_sqrt((RN - p) * (RN + p))
            zN = zv[k + 1]
            while i > imin:
                m = index(i, k)
                dsq = (qN - q) / kq
                dsz = (zN - z) / kz
                if dsq < dsz:
                    ds = dsq
                    add(m, ds)
                    i -= 1
                    q = qN
                    z += kz * ds
                    RN = Rv[i]
                    qN = -_sqrt((RN - p) * (RN + p))
                else:
                    ds = dsz
                    add(m, ds)
                    k += 1
                    if k >= Nz:
                        return segs
                    q += kq * ds
                    z = zN
                    zN = zv[k + 1]
        RN = Rv[i + 1]
        qN = _sqrt((RN - p) * (RN + p))
        zN = zv[k + 1]
        while True:
            m = index(i, k)
            dsq = (qN - q) / kq
            dsz = (zN - z) / kz
            if dsq < dsz:
                ds = dsq
                add(m, ds)
                i += 1
                if i >= NR:
                    return segs
                q = qN
                z += kz * ds
                RN = Rv[i + 1]
                qN = _sqrt((RN - p) * (RN + p))
            else:
                ds = dsz
                add(m, ds)
                k += 1
                if k >= Nz:
                    return segs
                q += kq * ds
                z = zN
                zN = zv[k + 1]
    else:  # downward
        if q < 0.0:
            imin = locate_clip(Rv, p)
            RN = Rv[i]
            qN = -_sqrt((RN - p) * (RN + p))
            zN = zv[k]
            while i > imin:
                m = index(i, k)
                dsq = (qN - q) / kq
                dsz = (zN - z) / kz
                if dsq < dsz:
                    ds = dsq
                    add(m, ds)
                    i -= 1
                    q = qN
                    z += kz * ds
                    RN = Rv[i]
                    qN = -_sqrt((RN - p) * (RN + p))
                else:
                    ds = dsz
                    add(m, ds)
                    k -= 1
                    if k < 0:
                        return segs
                    q += kq * ds
                    z = zN
                    zN = zv[k]
        RN = Rv[i + 1]
        qN = _sqrt((RN - p) * (RN + p))
        zN = zv[k]
        while True:
            m = index(i, k)
            dsq = (qN - q) / kq
            dsz = (zN - z) / kz
            if dsq < dsz:
                ds = dsq
                add(m, ds)
                i += 1
                if i >= NR - 1:  # (the reference's downward loop ends on entering the last shell)
                    return segs
                q = qN
                z += kz * ds
                RN = Rv[i + 1]
                qN = _sqrt((RN - p) * (RN + p))
            else:
                ds = dsz
                add(m, ds)
                k -= 1
                if k < 0:
                    return segs
                q += kq * ds
                z = zN
                zN = zv[k]


# ---------------------------------------------------------------- the grids and rays of the tests
PC = 3.08567758e16  # m (Units.cpp)


def lin_mesh(n):
    dx = (1.0 - 0.0) / n
    return [0.0 + i * dx for i in range(n + 1)]


def pow_mesh(n, ratio):
    q = math.pow(ratio, 1.0 / (n - 1))
    qn = math.pow(q, n)
    return [0.0 + (1.0 - math.pow(q, i)) / (1.0 - qn) * 1.0 for i in range(n + 1)]


def sympow_mesh(n, ratio):
    assert n % 2 == 0
    M = n // 2
    q = math.pow(ratio, 1.0 / (M - 1.0))
    qM = math.pow(q, M)
    tv = [0.0] * (n + 1)
    tv[M] = 0.5
    for i in range(1, M + 1):
        dxi = (1.0 - math.pow(q, i)) / (1.0 - qM) * 0.5 * 1.0
        tv[M + i] = 0.5 + dxi
        tv[M - i] = 0.5 - dxi
    return tv


def grid(tR, tz, Rmax=500.0, zmin=-500.0, zmax=500.0):
    """(Rv, zv) as Cylinder2DDustGrid::setupSelfAfter computes them (lengths here in pc)"""
    return [t * Rmax for t in tR], [t * (zmax - zmin) + zmin for t in tz]


def lin_grid():
    return grid(lin_mesh(12), lin_mesh(16))


def pow_grid():
    return grid(pow_mesh(12, 20.0), sympow_mesh(16, 20.0))


def random_rays(n=20000, seed=20261019):
    """origins uniform in [-700, 700]^3 (inside, outside in R, in z, in both), isotropic directions"""
    rng = np.random.RandomState(seed)
    o = rng.uniform(-700.0, 700.0, size=(n, 3))
    ct = rng.uniform(-1.0, 1.0, size=n)
    ph = rng.uniform(0.0, 2.0 * math.pi, size=n)
    st = np.sqrt(1.0 - ct * ct)
    d = np.stack([st * np.cos(ph), st * np.sin(ph), ct], axis=1)
    return np.concatenate([o, d], axis=1)


def explicit_rays():
    """the named cases of the walk: [(name, (x, y, z, kx, ky, kz))]"""
    s2 = math.sqrt(0.5)
    return [
        ("axis_start_oblique", (0.0, 0.0, 13.0, 0.6, 0.0, 0.8)),
        ("axis_start_horizontal", (0.0, 0.0, -77.0, s2, s2, 0.0)),
        ("along_plus_z", (120.0, 30.0, -650.0, 0.0, 0.0, 1.0)),
        ("along_minus_z", (120.0, 30.0, 650.0, 0.0, 0.0, -1.0)),
        ("along_plus_z_inside", (-40.0, 10.0, 3.0, 0.0, 0.0, 1.0)),
        ("kz_zero_inside", (-300.0, 55.0, 21.0, 1.0, 0.0, 0.0)),
        ("kz_zero_from_outside", (-650.0, 120.0, -140.0, 0.8, 0.6, 0.0)),
        ("origin_plus_x", (0.0, 0.0, 0.0, 1.0, 0.0, 0.0)),
        ("origin_minus_x", (0.0, 0.0, 0.0, -1.0, 0.0, 0.0)),
        ("origin_plus_z", (0.0, 0.0, 0.0, 0.0, 0.0, 1.0)),
        ("origin_minus_z", (0.0, 0.0, 0.0, 0.0, 0.0, -1.0)),
        ("mirror_up", (0.0, 0.0, 0.0, 0.8, 0.0, 0.6)),
        ("mirror_down", (0.0, 0.0, 0.0, 0.8, 0.0, -0.6)),
        ("outside_R_far_side", (800.0, 100.0, 50.0, -1.0, 0.0, 0.0)),
        ("p_in_innermost_shell", (-400.0, 5.0, -90.0, 0.96, 0.0, 0.28)),
        ("p_in_innermost_shell_down", (-400.0, -5.0, 90.0, 0.96, 0.0, -0.28)),
        ("outside_z_up", (100.0, -50.0, -900.0, 0.0, 0.6, 0.8)),
        ("outside_z_away", (100.0, -50.0, -900.0, 0.0, 0.6, -0.8)),
        ("outside_both", (600.0, 0.0, 600.0, -0.6, 0.0, -0.8)),
    ]


def all_rays(nrandom=20000):
    """float64 [n, 6]: the random rays, then the explicit cases"""
    ex = np.array([r for _, r in explicit_rays()], dtype=np.float64)
    return np.concatenate([random_rays(nrandom), ex], axis=0)


def column(Rv, zv, rho, ray):
    """sum of rho[m] ds over the in-grid segments of a ray, or None if the path crosses no cell"""
    segs = [(m, ds) for m, ds in path(Rv, zv, ray[:3], ray[3:]) if m >= 0]
    if not segs:
        return None
    return math.fsum(rho[m] * ds for m, ds in segs)
