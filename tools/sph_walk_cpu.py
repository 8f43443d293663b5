"""CPU run of the device's spherical grid walks (skirt_amd/csrc/device/sph_walk.hpp): the header compiled as plain
C++ (-ffp-contract=off, as the device build) with a small driver that walks rays through a Sphere1D or Sphere2D
grid and returns each ray's segments as DustGridPath holds them (ds > 0 only), the cell of each ray's origin and the
number of steps each path took. tests/test_sph_walk_logic.py compares them with the plain-Python restatement of the
reference's routines (tests/sph_ref.py); the GPU test (tests/test_gpu_sph.py) repeats the comparison through the
engine.
Usage: python tools/sph_walk_cpu.py   (walks the tests' rays through the tests' four grids and prints totals)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "skirt_amd", "csrc", "device", "sph_walk.hpp")

MAIN = r'''
#include <cstdio>
#include <cstdint>
#include <vector>
#include "%s"
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[3];
    double par[2];
    if (fread(hdr, 8, 3, f) != 3 || fread(par, 8, 2, f) != 2) return 2;
    const int Nr = (int)hdr[0], Nt = (int)hdr[1];  // Nt = 0: Sphere1D
    const size_t n = (size_t)hdr[2];
    const double rmax = par[0], eps = par[1];
    std::vector<double> rv(Nr + 1), cv(Nt + 1), thv(Nt + 1), rays(6 * n);
    if (fread(rv.data(), 8, rv.size(), f) != rv.size()) return 2;
    if (Nt > 0 && (fread(cv.data(), 8, cv.size(), f) != cv.size() || fread(thv.data(), 8, thv.size(), f) != thv.size()))
        return 2;
    if (fread(rays.data(), 8, rays.size(), f) != rays.size()) return 2;
    fclose(f);
    std::vector<int64_t> counts(n), cells, where(n), steps(n);
    std::vector<double> lens;
    for (size_t r = 0; r < n; r++) {
        const double* y = &rays[6 * r];
        int64_t c = 0, st = 0;
        auto add = [&](int m, double ds) {  // DustGridPath::addSegment
            if (ds > 0) { cells.push_back(m); lens.push_back(ds); c++; }
        };
        if (Nt == 0) {
            Sph1dState s;
            if (sph1dEnter(rv.data(), Nr, rmax, y[0], y[1], y[2], y[3], y[4], y[5], s, add)) {
                bool more = true;
                while (more) {
                    int m; double ds;
                    more = sph1dStep(rv.data(), Nr, s, m, ds);
                    add(m, ds);
                    st++;
                }
            }
            where[r] = sph1dWhichCell(rv.data(), Nr, y[0], y[1], y[2]);
        } else {
            Sph2dState s;
            if (sph2dEnter(rv.data(), Nr, thv.data(), Nt, rmax, eps, y[0], y[1], y[2], y[3], y[4], y[5], s, add)) {
                bool more = true;
                while (more) {
                    int m; double ds;
                    more = sph2dStep(rv.data(), Nr, cv.data(), thv.data(), Nt, eps, y[3], y[4], y[5], s, m, ds);
                    add(m, ds);
                    st++;
                }
            }
            where[r] = sph2dWhichCell(rv.data(), Nr, thv.data(), Nt, y[0], y[1], y[2]);
        }
        counts[r] = c;
        steps[r] = st;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(counts.data(), 8, n, o);
    fwrite(where.data(), 8, n, o);
    fwrite(steps.data(), 8, n, o);
    fwrite(cells.data(), 8, cells.size(), o);
    fwrite(lens.data(), 8, lens.size(), o);
    fclose(o);
    return 0;
}
'''


def build(workdir):
    """compiles the driver into workdir; returns the program's path"""
    cpp, exe = os.path.join(workdir, "sph_walk.cpp"), os.path.join(workdir, "sph_walk")
    with open(cpp, "w") as f:
        f.write(MAIN % HEADER)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, cpp], check=True)
    return exe


def walk(exe, rv, rmax, rays, workdir, thv=None, cv=None):
    """(counts[n], origin cells[n], steps[n], segment cells[total], segment lengths[total]) of rays [n, 6] through
    the Sphere1D grid rv, or the Sphere2D grid (rv, thv, cv) when thv is given; eps = 1e-11 rmax"""
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    n = rays.shape[0]
    inp, out = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(inp, "wb") as f:
        np.array([len(rv) - 1, 0 if thv is None else len(thv) - 1, n], dtype=np.int64).tofile(f)
        np.array([rmax, 1e-11 * rmax], dtype=np.float64).tofile(f)
        np.asarray(rv, dtype=np.float64).tofile(f)
        if thv is not None:
            np.asarray(cv, dtype=np.float64).tofile(f)
            np.asarray(thv, dtype=np.float64).tofile(f)
        rays.tofile(f)
    subprocess.run([exe, inp, out], check=True)
    with open(out, "rb") as f:
        counts = np.fromfile(f, dtype=np.int64, count=n)
        where = np.fromfile(f, dtype=np.int64, count=n)
        steps = np.fromfile(f, dtype=np.int64, count=n)
        total = int(counts.sum())
        cells = np.fromfile(f, dtype=np.int64, count=total)
        lens = np.fromfile(f, dtype=np.float64, count=total)
    assert len(lens) == total
    return counts, where, steps, cells, lens


def main():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import sph_ref

    with tempfile.TemporaryDirectory(prefix="sph_") as d:
        exe = build(d)
        rays = sph_ref.all_rays()
        runs = [("sphere1d " + k, walk(exe, rv, sph_ref.RMAX, rays, d)) for k, rv in sph_ref.grids1().items()]
        runs += [("sphere2d " + k, walk(exe, g[0], sph_ref.RMAX, rays, d, thv=g[1], cv=g[2]))
                 for k, g in sph_ref.grids2().items()]
        for name, (counts, where, steps, cells, lens) in runs:
            print("%s: %d rays, %d with a path, %d segments (%d outside), origins in a cell: %d, longest path %d "
                  "steps, in-grid length %.6f" % (
                      name, len(counts), int((counts > 0).sum()), len(cells), int((cells < 0).sum()),
                      int((where >= 0).sum()), int(steps.max()), float(lens[cells >= 0].sum())))


if __name__ == "__main__":
    main()
