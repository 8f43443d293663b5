"""CPU run of the device's cylindrical grid walk (skirt_amd/csrc/device/cyl2d_walk.hpp): the header compiled as
plain C++ (-ffp-contract=off, as the device build) with a small driver that walks rays through an R-z grid and
returns each ray's segments as DustGridPath holds them (ds > 0 only) and the cell of each ray's origin.
tests/test_cyl2d_walk_logic.py compares them with the plain-Python restatement of the reference's routine
(tests/cyl2d_ref.py); the GPU test (tests/test_gpu_cyl.py) repeats the comparison through the engine.
Usage: python tools/cyl2d_walk_cpu.py   (walks the tests' rays through the two 12 x 16 grids and prints totals)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "skirt_amd", "csrc", "device", "cyl2d_walk.hpp")

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
    if (fread(hdr, 8, 3, f) != 3) return 2;
    const int NR = (int)hdr[0], Nz = (int)hdr[1];
    const size_t n = (size_t)hdr[2];
    std::vector<double> Rv(NR + 1), zv(Nz + 1), rays(6 * n);
    if (fread(Rv.data(), 8, Rv.size(), f) != Rv.size() || fread(zv.data(), 8, zv.size(), f) != zv.size() ||
        fread(rays.data(), 8, rays.size(), f) != rays.size()) return 2;
    fclose(f);
    std::vector<int64_t> counts(n), cells, where(n);
    std::vector<double> lens;
    for (size_t r = 0; r < n; r++) {
        const double* y = &rays[6 * r];
        int64_t c = 0;
        auto add = [&](int m, double ds) {  // DustGridPath::addSegment
            if (ds > 0) { cells.push_back(m); lens.push_back(ds); c++; }
        };
        Cyl2dState s;
        if (cyl2dEnter(Rv.data(), NR, zv.data(), Nz, y[0], y[1], y[2], y[3], y[4], y[5], s, add)) {
            bool more = true;
            while (more) {
                int m; double ds;
                more = cyl2dStep(Rv.data(), NR, zv.data(), Nz, s, m, ds);
                add(m, ds);
            }
        }
        counts[r] = c;
        where[r] = cyl2dWhichCell(Rv.data(), NR, zv.data(), Nz, y[0], y[1], y[2]);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(counts.data(), 8, n, o);
    fwrite(where.data(), 8, n, o);
    fwrite(cells.data(), 8, cells.size(), o);
    fwrite(lens.data(), 8, lens.size(), o);
    fclose(o);
    return 0;
}
'''


def build(workdir):
    """compiles the driver into workdir; returns the program's path"""
    cpp, exe = os.path.join(workdir, "cyl2d_walk.cpp"), os.path.join(workdir, "cyl2d_walk")
    with open(cpp, "w") as f:
        f.write(MAIN % HEADER)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, cpp], check=True)
    return exe


def walk(exe, Rv, zv, rays, workdir):
    """(counts[n], origin cells[n], segment cells[total], segment lengths[total]) of rays [n, 6]"""
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    n = rays.shape[0]
    inp, out = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(inp, "wb") as f:
        np.array([len(Rv) - 1, len(zv) - 1, n], dtype=np.int64).tofile(f)
        np.asarray(Rv, dtype=np.float64).tofile(f)
        np.asarray(zv, dtype=np.float64).tofile(f)
        rays.tofile(f)
    subprocess.run([exe, inp, out], check=True)
    with open(out, "rb") as f:
        counts = np.fromfile(f, dtype=np.int64, count=n)
        where = np.fromfile(f, dtype=np.int64, count=n)
        total = int(counts.sum())
        cells = np.fromfile(f, dtype=np.int64, count=total)
        lens = np.fromfile(f, dtype=np.float64, count=total)
    assert len(lens) == total
    return counts, where, cells, lens


def main():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import cyl2d_ref

    with tempfile.TemporaryDirectory(prefix="cyl2d_") as d:
        exe = build(d)
        rays = cyl2d_ref.all_rays()
        for name, (Rv, zv) in (("lin", cyl2d_ref.lin_grid()), ("pow", cyl2d_ref.pow_grid())):
            counts, where, cells, lens = walk(exe, Rv, zv, rays, d)
            print("%s: %d rays, %d with a path, %d segments (%d outside), origins in a cell: %d, in-grid length %.6f" % (
                name, len(counts), int((counts > 0).sum()), len(cells), int((cells < 0).sum()), int((where >= 0).sum()),
                float(lens[cells >= 0].sum())))


if __name__ == "__main__":
    main()
