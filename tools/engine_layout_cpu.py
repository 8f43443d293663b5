"""CPU run of the engine's host-side arithmetic (skirt_amd/csrc/host/engine_layout.cpp): the pool's layout, the
instruments' tally layout, the tree numbering and leaf-map plan, the Voronoi packing and the Labs and LDS plans of a
phase, which the engine runs between its allocations and copies. None of it needs HIP, so tools/engine_layout_check.cpp
(a program of its own, with the cases) is built from it and host/voronoi.cpp with the address and
undefined-behaviour sanitizers and run directly. tests/test_engine_layout.py runs it group by group.
Usage: python tools/engine_layout_cpu.py [group ...]   (pool instruments trees leafmap voronoi labs lds; none: all)"""
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "skirt_amd", "csrc", "host")
GROUPS = ("pool", "instruments", "trees", "leafmap", "voronoi", "labs", "lds")


def build(workdir):
    """compiles the check program into workdir; returns its path"""
    exe = os.path.join(workdir, "engine_layout_check")
    # (the sanitizers' runtimes linked into the program: it then runs the same whatever else a machine preloads)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe,
                    os.path.join(REPO, "tools", "engine_layout_check.cpp"),
                    os.path.join(HOST, "engine_layout.cpp"), os.path.join(HOST, "voronoi.cpp"), "-lpthread"], check=True)
    return exe


def run(exe, *groups):
    """runs the groups' checks; returns the program's output, raises with it if a check or a sanitizer failed"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SKIRT_AMD_")}  # the cases set their own
    p = subprocess.run([exe, *groups], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    if p.returncode != 0:
        raise RuntimeError("engine_layout_check %s: exit %d\n%s" % (" ".join(groups), p.returncode, p.stdout))
    return p.stdout


def main():
    with tempfile.TemporaryDirectory(prefix="layout_") as d:
        sys.stdout.write(run(build(d), *sys.argv[1:]))


if __name__ == "__main__":
    main()
