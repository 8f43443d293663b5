"""Plain-Python restatement of the reference's imported particle dust (SKIRTcore/SPHDustDistribution.cpp,
SPHGasParticle.cpp, SPHGasParticleGrid.cpp, TextInFile.cpp): the file reader, the cached particle constants, the
20 x 20 x 20 grid of particle lists with its equal-count separators, metalDensity, myerf, metalMassInBox, density and
massInBox. Python floats are IEEE doubles and numpy's elementwise +, -, *, sqrt round as C's, so every value equals
the host's bit for bit; sums run left to right (np.cumsum accumulates sequentially). Also the adversarial points and
boxes that the host, the CPU build of the device header and the device are all checked on."""
import math

import numpy as np

PC = 3.08567758e16
MSUN = 1.9891e30
GRID = 20
ERF_N = 5000
ERF_MAX = 2.5
INF = float("inf")


def read_rows(path):
    """TextInFile::readRow(1, x, y, z, h, M, Z, T): blank and comment lines skipped, the last column optional"""
    rows = []
    for line in open(path):
        s = line.strip(" \t\n")
        if not s or s[0] == "#":
            continue
        v = [float(t) for t in s.split()]
        if len(v) < 6:
            raise ValueError("One or more required value(s) on text line are missing")
        rows.append(tuple(v[:6]) + ((v[6],) if len(v) > 6 else (0.0,)))
    return rows


def locate_clip(xv, x):
    """NR::locate_clip, on an array that need not be sorted (zero-filled separators)"""
    if x < xv[0]:
        return 0
    jl, ju = -1, len(xv) - 1
    while ju - jl > 1:
        jm = (ju + jl) >> 1
        if x < xv[jm]:
            ju = jm
        else:
            jl = jm
    return jl


def _intersects(b, c, r):
    sq = r * r
    for a in range(3):
        if c[a] < b[a][0]:
            sq -= (c[a] - b[a][0]) * (c[a] - b[a][0])
        elif c[a] > b[a][1]:
            sq -= (c[a] - b[a][1]) * (c[a] - b[a][1])
    return sq > 0.0


class Particles:
    def __init__(self, path, fdust, Tmax):
        self.fdust = fdust
        c, h, M, Z = [], [], [], []
        self.nignored = 0
        self.negative = False
        for x, y, z, hh, m, zz, T in read_rows(path):
            if T > 0 and Tmax > 0 and T > Tmax:
                self.nignored += 1
                continue
            c.append((x * PC, y * PC, z * PC))
            h.append(hh * PC)
            M.append(m * MSUN)
            Z.append(zz)
            if m < 0:
                self.negative = True
        self.n = len(c)
        self.c = np.array(c)
        self.h = np.array(h)
        M, Z = np.array(M), np.array(Z)
        self.norm = 1 / (self.h * self.h)
        self.rho0 = 8.0 / math.pi * M / (self.h * self.h * self.h) * Z
        self.rho2 = self.rho0 * 2.0
        self.s = 2.42 / self.h
        self.mz8 = M * Z / 8.0
        self.metal = M * Z
        self.erf = np.array([math.erf((i * ERF_MAX) / ERF_N) for i in range(ERF_N + 1)])
        self.sep, self.cmin, self.cmax = [], [], []
        for a in range(3):
            g, lo, hi = self._makegrid(a)
            self.sep.append(g)
            self.cmin.append(lo)
            self.cmax.append(hi)
        lists = [[] for _ in range(GRID ** 3)]
        for p in range(self.n):
            cc, r = [float(t) for t in self.c[p]], float(self.h[p])
            rng = [(locate_clip(self.sep[a], cc[a] - r), locate_clip(self.sep[a], cc[a] + r)) for a in range(3)]
            for i in range(rng[0][0], rng[0][1] + 1):
                for j in range(rng[1][0], rng[1][1] + 1):
                    for k in range(rng[2][0], rng[2][1] + 1):
                        b = ((self.sep[0][i], self.sep[0][i + 1]), (self.sep[1][j], self.sep[1][j + 1]),
                             (self.sep[2][k], self.sep[2][k + 1]))
                        if _intersects(b, cc, r):
                            lists[(i * GRID + j) * GRID + k].append(p)
        self.lists = [np.array(l, dtype=np.int64) for l in lists]

    def _makegrid(self, a):
        ctr = [float(t) for t in self.c[:, a]]
        hs = [float(t) for t in self.h]
        cmin, cmax = INF, -INF
        for p in range(self.n):
            cmin = min(cmin, ctr[p] - hs[p])
            cmax = max(cmax, ctr[p] + hs[p])
        nbins = GRID * 100
        binwidth = (cmax - cmin) / nbins
        bins = [0] * nbins
        for p in range(self.n):
            bins[int((ctr[p] - cmin) / binwidth)] += 1
        grid = [0.0] * (GRID + 1)
        grid[0] = -INF
        percell = self.n // GRID
        cumul, gi = 0, 1
        for b in range(nbins):
            cumul += bins[b]
            if cumul > percell * gi:
                grid[gi] = cmin + (b + 1) * binwidth
                gi += 1
                if gi >= GRID:
                    break
        grid[GRID] = INF
        return grid, cmin, cmax

    # ------------------------------------------------------------ the distribution's functions
    def cell(self, x, y, z):
        return (locate_clip(self.sep[0], x) * GRID + locate_clip(self.sep[1], y)) * GRID + locate_clip(self.sep[2], z)

    def density(self, x, y, z):
        ids = self.lists[self.cell(x, y, z)]
        if len(ids) == 0:
            return 0.0
        d = np.array([x, y, z]) - self.c[ids]
        u2 = self.norm[ids] * (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        u = np.sqrt(u2)
        u1m = 1.0 - u
        inner = self.rho0[ids] * (1.0 - 6.0 * u2 * u1m)
        outer = self.rho2[ids] * u1m * u1m * u1m
        t = np.where(u2 < 1.0, np.where(u < 0.5, inner, outer), 0.0)
        s = float(np.cumsum(t)[-1]) * self.fdust
        return max(s, 0.0)

    def myerf(self, x):
        x = np.asarray(x, dtype=np.float64)
        ax = np.minimum(np.abs(x), 2.4999)  # (only to keep the unused branch's index in range)
        pos = self.erf[(np.where(x >= 0, x, ax) * (ERF_N / ERF_MAX)).astype(np.int64).clip(0, ERF_N)]
        neg = -self.erf[(np.where(x < 0, -x, ax) * (ERF_N / ERF_MAX)).astype(np.int64).clip(0, ERF_N)]
        return np.where(x >= ERF_MAX, 1.0, np.where(x >= 0, pos, np.where(x > -ERF_MAX, neg, -1.0)))

    def box_cells(self, b):
        lo = [locate_clip(self.sep[a], b[a]) for a in range(3)]
        hi = [locate_clip(self.sep[a], b[3 + a]) for a in range(3)]
        return lo, hi

    def spanned(self, b):
        lo, hi = self.box_cells(b)
        if lo == hi:
            return 1
        n = 1
        for a in range(3):
            n *= max(0, hi[a] - lo[a] + 1)
        return n

    def mass_in_box(self, b):
        lo, hi = self.box_cells(b)
        if lo == hi:
            ids = self.lists[(lo[0] * GRID + lo[1]) * GRID + lo[2]]
        else:
            joined = set()
            for i in range(lo[0], hi[0] + 1):
                for j in range(lo[1], hi[1] + 1):
                    for k in range(lo[2], hi[2] + 1):
                        joined.update(self.lists[(i * GRID + j) * GRID + k].tolist())
            ids = np.array(sorted(joined), dtype=np.int64)
        if len(ids) == 0:
            return 0.0
        s, c = self.s[ids], self.c[ids]
        f = self.mz8[ids]
        for a in range(3):
            f = f * (self.myerf(s * (b[3 + a] - c[:, a])) - self.myerf(s * (b[a] - c[:, a])))
        return max(float(np.cumsum(f)[-1]) * self.fdust, 0.0)

    def mass(self):
        return max(float(np.cumsum(self.metal)[-1]) * self.fdust, 0.0)


# ---------------------------------------------------------------- the adversarial inputs
def _ulps(v):
    return [float(np.nextafter(v, -INF)), v, float(np.nextafter(v, INF))]


def adversarial_points(P, nrandom=10000, seed=5):
    """random points over (and a little beyond) the particles' range; points on every separator and one ulp either
    side; points at kernel radius u = 0.5 and 1 of some particles, and one ulp either side; points far outside"""
    rng = np.random.RandomState(seed)
    lo, hi = np.array(P.cmin), np.array(P.cmax)
    pts = [lo - 0.05 * (hi - lo) + rng.rand(nrandom, 3) * 1.1 * (hi - lo)]
    some = P.c[:: max(1, P.n // 7)]
    extra = []
    for a in range(3):
        for s in P.sep[a][1:-1]:
            for v in _ulps(s):
                for c in some:
                    p = [float(t) for t in c]
                    p[a] = v
                    extra.append(p)
    for p in range(0, P.n, max(1, P.n // 40)):
        c, h = [float(t) for t in P.c[p]], float(P.h[p])
        for a in range(3):
            for f in (0.5, 1.0, -0.5, -1.0):
                for v in _ulps(c[a] + f * h):
                    q = list(c)
                    q[a] = v
                    extra.append(q)
    for v in (1e30, -1e30):
        extra += [[v, 0.0, 0.0], [0.0, v, 0.0], [0.0, 0.0, v], [v, v, v], [v, -v, v]]
    pts.append(np.array(extra))
    return np.concatenate(pts)


def _mid(sep, i):
    """a coordinate inside cell i of a sorted axis (the end cells reach to infinity)"""
    lo, hi = sep[i], sep[i + 1]
    if lo == -INF:
        return hi - 1e18
    if hi == INF:
        return lo + 1e18
    return 0.5 * (lo + hi)


def span_box(P, i, j, k, ni, nj, nk):
    """a box from inside cell (i, j, k) to inside cell (i + ni - 1, j + nj - 1, k + nk - 1)"""
    return [_mid(P.sep[0], i), _mid(P.sep[1], j), _mid(P.sep[2], k),
            _mid(P.sep[0], i + ni - 1), _mid(P.sep[1], j + nj - 1), _mid(P.sep[2], k + nk - 1)]


def adversarial_boxes(P, nrandom=10000, seed=6):
    """(boxes within the device's merge cap, boxes built to exceed it). Within: random boxes (mostly small), boxes
    inside one cell, boxes spanning 2, 8, 27 and 64 cells, a zero-width box, boxes whose scaled edges fall at +-2.5
    of a particle and one ulp either side (table index 4999 / 5000). Beyond: 5 x 5 x 3 cells and more, the whole
    grid. Needs sorted separators (the cloud files)."""
    rng = np.random.RandomState(seed)
    lo, hi = np.array(P.cmin), np.array(P.cmax)
    ctr = lo + rng.rand(nrandom, 3) * (hi - lo)
    half = (hi - lo) * (10.0 ** rng.uniform(-3.5, -1.3, size=(nrandom, 1))) * rng.rand(nrandom, 3)
    boxes = [list(map(float, np.concatenate([c - w, c + w]))) for c, w in zip(ctr, half)]
    large = [b for b in boxes if P.spanned(b) > 64]  # (the particle grid's central cells are small)
    boxes = [b for b in boxes if P.spanned(b) <= 64]
    for i, j, k in ((3, 4, 5), (9, 9, 9), (0, 0, 0), (19, 19, 19), (10, 0, 19)):
        boxes.append(span_box(P, i, j, k, 1, 1, 1))
    for i, j, k in ((3, 4, 5), (9, 9, 9), (0, 10, 18)):
        boxes += [span_box(P, i, j, k, 2, 1, 1), span_box(P, i, j, k, 1, 2, 1), span_box(P, i, j, k, 1, 1, 2),
                  span_box(P, i, j, k, 2, 2, 2)]
    boxes += [span_box(P, 8, 8, 8, 3, 3, 3), span_box(P, 0, 0, 0, 3, 3, 3), span_box(P, 17, 17, 17, 3, 3, 3),
              span_box(P, 8, 8, 8, 4, 4, 4), span_box(P, 2, 9, 16, 4, 4, 4)]
    c0 = [float(t) for t in P.c[0]]
    boxes.append([c0[0], c0[1] - 1e17, c0[2] - 1e17, c0[0], c0[1] + 1e17, c0[2] + 1e17])  # zero width
    for p in range(0, P.n, max(1, P.n // 25)):
        c, s = [float(t) for t in P.c[p]], float(P.s[p])
        for a in range(3):
            for sign in (1.0, -1.0):
                for e in _ulps(c[a] + sign * (ERF_MAX / s)):
                    b = [c[0] - 1e17, c[1] - 1e17, c[2] - 1e17, c[0] + 1e17, c[1] + 1e17, c[2] + 1e17]
                    b[a if sign < 0 else 3 + a] = e
                    boxes.append(b)
    beyond = [span_box(P, 8, 8, 8, 5, 5, 3), span_box(P, 0, 0, 0, 5, 5, 3), span_box(P, 3, 3, 3, 13, 2, 3),
              span_box(P, 0, 0, 0, 20, 20, 20)] + large + [[-1e30] * 3 + [1e30] * 3]
    return np.array(boxes), np.array(beyond)
