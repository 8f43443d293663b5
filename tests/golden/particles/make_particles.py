#!/usr/bin/env python3
"""Writes the particle files of the particle-dust fixtures (cloud.dat, cloud_neg.dat, few.dat) beside this script.
Deterministic: a 64-bit linear congruential generator of its own, fixed formats, no library random numbers. The files
are committed; run it again only to change them (and then regenerate tests/golden/ref_particles).

Rows are x y z h M Z T (pc, pc, pc, pc, Msun, -, K), the columns of the reference's SPHDustDistribution.
  cloud.dat      about 1500 gas particles: a Plummer-like cloud (scale 120 pc) with five clumps, smoothing lengths
                 from 8 to 240 pc (a factor of 30, smaller where the cloud is denser), a comment line and a blank line
                 inside the data, one row in fifteen hotter than the models' maximumTemperature of 8e4 K, some rows
                 outside the models' 500 pc grid extent, and some rows without the optional temperature column
  cloud_neg.dat  the same rows, seven of them with a negative mass (the distribution then offers no mass-in-box)
  few.dat        37 particles: 37 / 20 = 1 particle per cell, and all but one fall into the last few of the 2000
                 bins, so the equal-count cuts run out of bins and separators keep the array's zero fill (the
                 separator array is then not sorted)
"""
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))


class Lcg:
    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def u(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return ((self.s >> 11) + 0.5) / float(1 << 53)

    def gauss(self):
        return math.sqrt(-2.0 * math.log(self.u())) * math.cos(2.0 * math.pi * self.u())


def direction(r):
    ct = 2.0 * r.u() - 1.0
    ph = 2.0 * math.pi * r.u()
    st = math.sqrt(1.0 - ct * ct)
    return st * math.cos(ph), st * math.sin(ph), ct


def cloud_rows():
    r = Lcg(20240607)
    clumps = [(150.0, 80.0, -40.0, 25.0), (-200.0, 120.0, 60.0, 40.0), (60.0, -230.0, 110.0, 30.0),
              (-90.0, -60.0, -260.0, 20.0), (310.0, -20.0, 30.0, 35.0)]
    rows = []
    for i in range(1500):
        if i % 4 == 3:
            cx, cy, cz, s = clumps[(i // 4) % 5]
            x, y, z = cx + s * r.gauss(), cy + s * r.gauss(), cz + s * r.gauss()
            h = 8.0 + 40.0 * r.u()
        else:
            t = r.u() ** (1.0 / 3.0)
            rad = 120.0 * t / math.sqrt(max(1e-12, (1.0 - t) * (1.0 + t)))
            rad = min(rad, 900.0)  # (a few land outside the 500 pc extent)
            kx, ky, kz = direction(r)
            x, y, z = rad * kx, rad * ky, rad * kz
            h = min(240.0, 8.0 + 0.6 * rad + 30.0 * r.u())
        M = 600.0 + 1000.0 * r.u()
        Z = 0.01 + 0.02 * r.u()
        T = 2.0e5 * r.u() + 9.0e4 if i % 15 == 7 else 1.0e4 + 5.0e4 * r.u()
        rows.append((x, y, z, h, M, Z, T))
    return rows


def write(name, rows, header, no_T=()):
    with open(os.path.join(HERE, name), "w") as f:
        f.write("# %s\n# x(pc) y(pc) z(pc) h(pc) M(Msun) Z T(K)\n" % header)
        for i, (x, y, z, h, M, Z, T) in enumerate(rows):
            if i == 100:
                f.write("# a comment line inside the data\n\n")
            line = "%.4f %.4f %.4f %.4f %.3f %.5f" % (x, y, z, h, M, Z)
            if i not in no_T:
                line += " %.1f" % T
            f.write(line + "\n")


def main():
    rows = cloud_rows()
    no_T = set(range(5, 1500, 97))
    write("cloud.dat", rows, "clumpy Plummer-like gas cloud, 1500 rows", no_T)
    neg = list(rows)
    for i in (11, 222, 333, 640, 901, 1203, 1444):
        x, y, z, h, M, Z, T = neg[i]
        neg[i] = (x, y, z, h, -0.5 * M, Z, 2.0e4)
    write("cloud_neg.dat", neg, "cloud.dat with seven negative masses", no_T)
    # one wide particle far below the grid stretches the binned range to 5000 pc and more, so a bin is 2.7 pc wide;
    # the other 36 sit within a parsec of (300, 300, 300) pc with h <= 40 pc, fewer than 19 bins below the top
    r = Lcg(37)
    few = [(-3000.0, -3000.0, -3000.0, 2000.0, 4.0e4, 0.02, 1.0e4)]
    for i in range(36):
        few.append((300.0 + r.gauss(), 300.0 + r.gauss(), 300.0 + r.gauss(), 20.0 + 20.0 * r.u(),
                    3.0e4 + 2.0e4 * r.u(), 0.02, 1.0e4))
    write("few.dat", few, "37 particles, 36 of them in the last bins of the particle grid")


if __name__ == "__main__":
    main()
