"""CPU run of the device's geometry samplers (skirt_amd/csrc/device/geom_sample.hpp): the header compiled as plain
C++ (-ffp-contract=off, as the device build) with philox.hpp's PacketRng and a small driver that, for one geometry
given as its parameter rows (include/skirt_mcrt.h: 7 words of geom_param, 4 of geom_table), draws positions on the
streams PacketRng::start(seed, tag, first + i) and evaluates the density at given points.
tests/test_geom_sample_logic.py compares both with the host library and with the plain-Python restatement of the
reference (tests/geom_ref.py); the GPU test (tests/test_gpu_geom.py) repeats the comparison through the engine.
Usage: python tools/geom_sample_cpu.py   (samples 20000 positions of six example geometries and prints totals)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(REPO, "skirt_amd", "csrc", "device")
TAG = 0x504f5331  # SKIRT_POSITIONS_TAG

MAIN = r'''
#include <cstdio>
#include <cstdint>
#include <vector>
#define __host__
#define __device__
#include "%s"
#include "%s"
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[6];  // kind, seed, tag, first, n positions, m density points
    double gp[7], tab[4];
    if (fread(hdr, 8, 6, f) != 6 || fread(gp, 8, 7, f) != 7 || fread(tab, 8, 4, f) != 4) return 2;
    const int kind = (int)hdr[0];
    const size_t n = (size_t)hdr[4], m = (size_t)hdr[5];
    std::vector<double> pts(3 * m), pos(3 * n), dens(m);
    std::vector<int64_t> draws(n), ok(n);
    if (fread(pts.data(), 8, pts.size(), f) != pts.size()) return 2;
    fclose(f);
    for (size_t i = 0; i < n; i++) {
        skirt_dev::PacketRng rng;
        rng.start((uint64_t)hdr[1], (uint32_t)hdr[2], (uint64_t)hdr[3] + i);
        ok[i] = geomPositionOf(kind, gp, tab, rng, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
        draws[i] = 2 * (int64_t)rng.block - (rng.have ? 1 : 0);
    }
    for (size_t i = 0; i < m; i++) dens[i] = geomDensityOf(kind, gp, tab, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(pos.data(), 8, pos.size(), o);
    fwrite(draws.data(), 8, n, o);
    fwrite(ok.data(), 8, n, o);
    fwrite(dens.data(), 8, m, o);
    fclose(o);
    return 0;
}
'''


def build(workdir):
    """compiles the driver into workdir; returns the program's path"""
    cpp, exe = os.path.join(workdir, "geom_sample.cpp"), os.path.join(workdir, "geom_sample")
    stub = os.path.join(workdir, "hip")
    os.makedirs(stub, exist_ok=True)
    with open(os.path.join(stub, "hip_runtime.h"), "w") as f:  # philox.hpp includes it; nothing of it is used
        f.write("#pragma once\n")
    with open(cpp, "w") as f:
        f.write(MAIN % (os.path.join(DEVICE, "philox.hpp"), os.path.join(DEVICE, "geom_sample.hpp")))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", workdir, "-o", exe, cpp],
                   check=True)
    return exe


def sample(exe, kind, gp, tab, n, workdir, seed=1, first=0, points=None, tag=TAG):
    """(pos[n, 3], draws[n], ok[n], density[m]) of geometry `kind` (SKIRT_GEOM_*) with the parameter rows gp, tab:
    n positions, and the density at points [m, 3]"""
    pts = np.zeros((0, 3)) if points is None else np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    inp, out = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(inp, "wb") as f:
        np.array([kind, seed, tag, first, n, len(pts)], dtype=np.int64).tofile(f)
        np.asarray(gp, dtype=np.float64).tofile(f)
        np.asarray(tab, dtype=np.float64).tofile(f)
        pts.tofile(f)
    subprocess.run([exe, inp, out], check=True)
    with open(out, "rb") as f:
        pos = np.fromfile(f, dtype=np.float64, count=3 * n).reshape(n, 3)
        draws = np.fromfile(f, dtype=np.int64, count=n)
        ok = np.fromfile(f, dtype=np.int64, count=n)
        dens = np.fromfile(f, dtype=np.float64, count=len(pts))
    assert len(dens) == len(pts)
    return pos, draws, ok, dens


def main():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import geom_ref

    with tempfile.TemporaryDirectory(prefix="geom_") as d:
        exe = build(d)
        for g in geom_ref.EXAMPLES:
            g = geom_ref.setup(g)
            gp, tab = geom_ref.params(g)
            pos, draws, ok, dens = sample(exe, geom_ref.KIND_CODE[g["kind"]], gp, tab, 20000, d)
            _, _, _, dens = sample(exe, geom_ref.KIND_CODE[g["kind"]], gp, tab, 0, d, points=pos)
            print("%s: %d positions (%d capped), %.3f draws each, mean radius %.6g, mean density there %.6g" % (
                g["kind"], len(pos), int((ok == 0).sum()), draws.mean(), np.sqrt((pos ** 2).sum(1)).mean(), dens.mean()))


if __name__ == "__main__":
    main()
