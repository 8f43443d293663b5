"""CPU run of the device's particle density (skirt_amd/csrc/device/particle_density.hpp): the header compiled as
plain C++ (-ffp-contract=off, as the device build) with a small driver that reads a particle file through the host's
reader (host/particles.hpp, which builds the uploaded arrays), then runs the two kernels' bodies as the device does:
partDensity per point, and partMassInBox per box in blocks of partMassBlock "threads" that share one cursor array
with the kernel's strided layout. A box beyond the merge cap gets -1 and is counted, as on the device.
tests/test_particles_logic.py compares both with the host library; the GPU test repeats it through the engine.
Usage: python tools/particle_density_cpu.py   (the fixture cloud: totals over a few points and boxes)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "skirt_amd", "csrc")

MAIN = r'''
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "%s"
#include "%s"
int main(int argc, char** argv) {
    if (argc < 6) return 2;
    auto ps = skirt::readParticles(argv[1], std::atof(argv[2]), std::atof(argv[3]));
    const PartView v = ps->view();
    FILE* f = fopen(argv[4], "rb");
    if (!f) return 2;
    int64_t hdr[2];  // n points, m boxes
    if (fread(hdr, 8, 2, f) != 2) return 2;
    const size_t n = (size_t)hdr[0], m = (size_t)hdr[1];
    std::vector<double> pts(3 * n), boxes(6 * m), dens(n), mass(m);
    if (fread(pts.data(), 8, pts.size(), f) != pts.size() || fread(boxes.data(), 8, boxes.size(), f) != boxes.size()) return 2;
    fclose(f);
    for (size_t i = 0; i < n; i++) dens[i] = partDensity(v, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    int64_t back = 0;
    std::vector<int> cursors((size_t)partMergeCap * partMassBlock);  // one block's LDS
    for (size_t q = 0; q < m; q++) {
        const int lane = (int)(q %% partMassBlock);  // threadIdx.x
        double out = 0.0;
        if (partMassInBox(v, &boxes[6 * q], cursors.data() + lane, partMassBlock, &out)) mass[q] = out;
        else { mass[q] = -1.0; back++; }
    }
    FILE* o = fopen(argv[5], "wb");
    if (!o) return 2;
    fwrite(dens.data(), 8, n, o);
    fwrite(mass.data(), 8, m, o);
    fwrite(&back, 8, 1, o);
    fclose(o);
    return 0;
}
'''


class Build:
    """the compiled driver over one particle file (relative to nothing: give the path), dust fraction and Tmax"""

    def __init__(self, particle_file, fdust, Tmax):
        self.dir = tempfile.TemporaryDirectory(prefix="partcpu_")
        d = self.dir.name
        cpp, self.exe = os.path.join(d, "particle_density.cpp"), os.path.join(d, "particle_density")
        with open(cpp, "w") as f:
            f.write(MAIN % (os.path.join(CSRC, "device", "particle_density.hpp"), os.path.join(CSRC, "host", "particles.hpp")))
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", self.exe, cpp], check=True)
        self.args = [particle_file, repr(float(fdust)), repr(float(Tmax))]

    def run(self, points, boxes):
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        bxs = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
        inp, out = os.path.join(self.dir.name, "in.bin"), os.path.join(self.dir.name, "out.bin")
        with open(inp, "wb") as f:
            np.array([len(pts), len(bxs)], dtype=np.int64).tofile(f)
            pts.tofile(f)
            bxs.tofile(f)
        subprocess.run([self.exe] + self.args + [inp, out], check=True)
        with open(out, "rb") as f:
            dens = np.fromfile(f, dtype=np.float64, count=len(pts))
            mass = np.fromfile(f, dtype=np.float64, count=len(bxs))
            back = int(np.fromfile(f, dtype=np.int64, count=1)[0])
        return dens, mass, back

    def density(self, points):
        return self.run(points, np.zeros((0, 6)))[0]

    def mass_in_box(self, boxes):
        """(masses, -1 where the box was handed back; the handed-back count)"""
        _, mass, back = self.run(np.zeros((0, 3)), boxes)
        return mass, back


def main():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import particles_ref as R

    path = os.path.join(REPO, "tests", "golden", "particles", "cloud.dat")
    P = R.Particles(path, 0.3, 8e4)
    b = Build(path, 0.3, 8e4)
    pts = R.adversarial_points(P, nrandom=1000)
    within, beyond = R.adversarial_boxes(P, nrandom=1000)
    dens, mass, back = b.run(pts, np.concatenate([within, beyond]))
    print("%d points, density sum %.9g; %d boxes, %d handed back, mass sum of the others %.9g" % (
        len(pts), dens.sum(), len(mass), back, mass[mass >= 0].sum()))


if __name__ == "__main__":
    main()
