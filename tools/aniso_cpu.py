"""CPU run of the device's anisotropic-emission routines (skirt_amd/csrc/device/aniso_emission.hpp): the header
compiled as plain C++ (-ffp-contract=off, as the device build) with philox.hpp's PacketRng and a small driver that,
for one geometry given as (kind, r0), launches packets on the streams PacketRng::start(seed, tag, first + i)
(generatePosition, then generateDirection there), generates directions at given positions on the streams
first + j, and evaluates probabilityForDirection for given (position, direction) pairs.
tests/test_aniso_logic.py compares all three with the host library and with the plain-Python restatement of the
reference (tests/aniso_ref.py); the GPU test (tests/test_gpu_aniso.py) repeats the comparison through the engine.
Usage: python tools/aniso_cpu.py   (launches 20000 packets of each kind and prints totals)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(REPO, "skirt_amd", "csrc", "device")
TAG = 0x4c4e4331  # SKIRT_LAUNCHES_TAG

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
    int64_t hdr[7];  // kind, seed, tag, first, n launches, q positions for directions, m probability pairs
    double r0;
    if (fread(hdr, 8, 7, f) != 7 || fread(&r0, 8, 1, f) != 1) return 2;
    const int kind = (int)hdr[0];
    const size_t n = (size_t)hdr[4], q = (size_t)hdr[5], m = (size_t)hdr[6];
    std::vector<double> at(3 * q), pairs(6 * m), pos(3 * n), dir(3 * n), dirAt(3 * q), prob(m), valid(q + m);
    std::vector<int64_t> draws(n);
    if (fread(at.data(), 8, at.size(), f) != at.size() || fread(pairs.data(), 8, pairs.size(), f) != pairs.size()) return 2;
    fclose(f);
    std::vector<double> netzer(anisoNetzerWords);
    anisoNetzerTable(netzer.data());
    for (size_t i = 0; i < n; i++) {
        skirt_dev::PacketRng rng;
        rng.start((uint64_t)hdr[1], (uint32_t)hdr[2], (uint64_t)hdr[3] + i);
        double* p = &pos[3 * i];
        double* k = &dir[3 * i];
        anisoPositionOf(kind, r0, rng, p[0], p[1], p[2]);
        anisoDirectionOf(kind, r0, netzer.data(), rng, p[0], p[1], p[2], k[0], k[1], k[2]);
        draws[i] = 2 * (int64_t)rng.block - (rng.have ? 1 : 0);
    }
    for (size_t j = 0; j < q; j++) {
        skirt_dev::PacketRng rng;
        rng.start((uint64_t)hdr[1], (uint32_t)hdr[2], (uint64_t)hdr[3] + j);
        const double* p = &at[3 * j];
        double* k = &dirAt[3 * j];
        valid[j] = anisoPositionValid(kind, r0, p[0], p[1], p[2]);
        anisoDirectionOf(kind, r0, netzer.data(), rng, p[0], p[1], p[2], k[0], k[1], k[2]);
    }
    for (size_t j = 0; j < m; j++) {
        const double* v = &pairs[6 * j];
        valid[q + j] = anisoPositionValid(kind, r0, v[0], v[1], v[2]);
        prob[j] = anisoProbabilityOf(kind, r0, v[0], v[1], v[2], v[3], v[4], v[5]);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(pos.data(), 8, pos.size(), o);
    fwrite(dir.data(), 8, dir.size(), o);
    fwrite(draws.data(), 8, n, o);
    fwrite(dirAt.data(), 8, dirAt.size(), o);
    fwrite(prob.data(), 8, m, o);
    fwrite(valid.data(), 8, valid.size(), o);
    fwrite(netzer.data(), 8, netzer.size(), o);
    fclose(o);
    return 0;
}
'''


def build(workdir):
    """compiles the driver into workdir; returns the program's path"""
    cpp, exe = os.path.join(workdir, "aniso_cpu.cpp"), os.path.join(workdir, "aniso_cpu")
    stub = os.path.join(workdir, "hip")
    os.makedirs(stub, exist_ok=True)
    with open(os.path.join(stub, "hip_runtime.h"), "w") as f:  # philox.hpp includes it; nothing of it is used
        f.write("#pragma once\n")
    with open(cpp, "w") as f:
        f.write(MAIN % (os.path.join(DEVICE, "philox.hpp"), os.path.join(DEVICE, "aniso_emission.hpp")))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", workdir, "-o", exe, cpp],
                   check=True)
    return exe


def run(exe, kind, r0, n, workdir, seed=1, first=0, at=None, pairs=None, tag=TAG):
    """dict(pos[n, 3], dir[n, 3], draws[n]; dir_at[q, 3] for positions at [q, 3]; prob[m] for pairs [m, 6] = position,
    direction; valid[q + m]: anisoPositionValid of each given position; netzer[802]: the table) of geometry `kind`
    (SKIRT_GEOM_*) with parameter r0"""
    at = np.zeros((0, 3)) if at is None else np.ascontiguousarray(at, dtype=np.float64).reshape(-1, 3)
    pairs = np.zeros((0, 6)) if pairs is None else np.ascontiguousarray(pairs, dtype=np.float64).reshape(-1, 6)
    inp, out = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(inp, "wb") as f:
        np.array([kind, seed, tag, first, n, len(at), len(pairs)], dtype=np.int64).tofile(f)
        np.array([r0], dtype=np.float64).tofile(f)
        at.tofile(f)
        pairs.tofile(f)
    subprocess.run([exe, inp, out], check=True)
    q, m = len(at), len(pairs)
    with open(out, "rb") as f:
        res = dict(pos=np.fromfile(f, dtype=np.float64, count=3 * n).reshape(n, 3),
                   dir=np.fromfile(f, dtype=np.float64, count=3 * n).reshape(n, 3),
                   draws=np.fromfile(f, dtype=np.int64, count=n),
                   dir_at=np.fromfile(f, dtype=np.float64, count=3 * q).reshape(q, 3),
                   prob=np.fromfile(f, dtype=np.float64, count=m),
                   valid=np.fromfile(f, dtype=np.float64, count=q + m),
                   netzer=np.fromfile(f, dtype=np.float64, count=802))
    assert len(res["netzer"]) == 802
    return res


def main():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import aniso_ref

    with tempfile.TemporaryDirectory(prefix="aniso_") as d:
        exe = build(d)
        for kind in aniso_ref.KINDS:
            r = run(exe, aniso_ref.KIND_CODE[kind], 300.0, 20000, d)
            pairs = np.hstack([r["pos"], r["dir"]])
            p = run(exe, aniso_ref.KIND_CODE[kind], 300.0, 0, d, pairs=pairs)["prob"]
            print("%s: %d launches, %.3f draws each, mean radius %.6g, mean kz %.6g, mean probability along the "
                  "launch direction %.6g" % (kind, len(r["pos"]), r["draws"].mean(), np.sqrt((r["pos"] ** 2).sum(1)).mean(),
                                             r["dir"][:, 2].mean(), p.mean()))


if __name__ == "__main__":
    main()
