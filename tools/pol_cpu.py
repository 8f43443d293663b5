"""CPU run of the device's polarised scattering (skirt_amd/csrc/device/polarization.hpp): the header compiled as
plain C++ (-ffp-contract=off, as the device build) with a small driver that runs polProbeOne -- one scattering and
one scattering peel-off towards (kobs, ky) -- on given packet states with given deviates and given tables.
tests/test_pol_logic.py compares the results with the plain-Python restatement of the reference (tests/pol_ref.py);
the GPU test (tests/test_gpu_pol.py) repeats the comparison through the engine's probe.
Usage: python tools/pol_cpu.py   (runs the logic test's states and prints the largest deviation from pol_ref)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(REPO, "skirt_amd", "csrc", "device")

MAIN = r'''
#include <cstdio>
#include <cstdint>
#include <vector>
#include "%s"
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[4];  // ncomp, nlambda, ntheta, n states
    double axes[6];  // kobs, ky
    if (fread(hdr, 8, 4, f) != 4 || fread(axes, 8, 6, f) != 6) return 2;
    const int ncomp = (int)hdr[0], nlambda = (int)hdr[1], nt = (int)hdr[2];
    const size_t n = (size_t)hdr[3];
    std::vector<double> tab(polTableWords(ncomp, nlambda, nt)), st(polStateWords * n), dv(2 * n), out(polResultWords * n);
    if (fread(tab.data(), 8, tab.size(), f) != tab.size() || fread(st.data(), 8, st.size(), f) != st.size() ||
        fread(dv.data(), 8, dv.size(), f) != dv.size()) return 2;
    fclose(f);
    for (size_t i = 0; i < n; i++)
        polProbeOne(tab.data(), ncomp, nlambda, nt, &st[polStateWords * i], &dv[2 * i], axes, axes + 3,
                    &out[polResultWords * i]);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(out.data(), 8, out.size(), o);
    fclose(o);
    return 0;
}
'''


def build(workdir):
    """compiles the driver into workdir; returns the program's path"""
    cpp, exe = os.path.join(workdir, "pol_cpu.cpp"), os.path.join(workdir, "pol_cpu")
    with open(cpp, "w") as f:
        f.write(MAIN % os.path.join(DEVICE, "polarization.hpp"))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, cpp], check=True)
    return exe


def run(exe, tables, ncomp, nlambda, ntheta, states, deviates, kobs, ky, workdir):
    """results [n, 14] of polProbeOne for states [n, 12] and deviates [n, 2]"""
    states = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 12)
    deviates = np.ascontiguousarray(deviates, dtype=np.float64).reshape(-1, 2)
    assert len(states) == len(deviates)
    inp, out = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(inp, "wb") as f:
        np.array([ncomp, nlambda, ntheta, len(states)], dtype=np.int64).tofile(f)
        np.array([*kobs, *ky], dtype=np.float64).tofile(f)
        np.ascontiguousarray(tables, dtype=np.float64).tofile(f)
        states.tofile(f)
        deviates.tofile(f)
    subprocess.run([exe, inp, out], check=True)
    return np.fromfile(out, dtype=np.float64).reshape(len(states), 14)


def main():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import pol_ref

    nlambda = 2
    mixes = [pol_ref.electron_mix(nlambda), pol_ref.madeup_mix(nlambda)]
    kobs, ky = pol_ref.instrument_axes(90.0, 40.0, 25.0)
    states, devs = pol_ref.make_states(mixes, nlambda, kobs)
    with tempfile.TemporaryDirectory(prefix="pol_") as d:
        got = run(build(d), pol_ref.pack(mixes), len(mixes), nlambda, pol_ref.NTHETA, states, devs, kobs, ky, d)
    want = pol_ref.probe(mixes, states, devs, kobs, ky)
    both = np.isfinite(want) & np.isfinite(got)
    print("%d states, %d values not finite in both, largest difference %.3g" % (
        len(states), int((~both).sum()), np.abs(got - want)[both].max()))


if __name__ == "__main__":
    main()
