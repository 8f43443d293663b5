"""CPU run of the host set-up (skirt_amd/csrc/host: build.cpp and the files it drives, down to the worker threads)
under the address and undefined-behaviour sanitizers: tools/ski_load_check.cpp (a program of its own) is built from
those sources and run directly on every model of tests/golden/ski/; it prints a model's cell count and the sum of
its densities. None of it needs HIP. tests/test_ski_load.py runs it.
Usage: python tools/ski_load_cpu.py [model.ski ...]   (none: every fixture model)"""
import glob
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "skirt_amd", "csrc", "host")
DATA = os.path.join(REPO, "skirt_amd", "data")
# the set-up's sources: what oracle/Makefile takes from host/, the oracle itself left out
SOURCES = ("xml", "units", "build", "geometry", "sources", "dustmix", "dustgrid", "treegrid", "densities", "outputs",
           "dustemission", "voronoi")


def models():
    return sorted(glob.glob(os.path.join(REPO, "tests", "golden", "ski", "*.ski")))


def build(workdir):
    """compiles the check program into workdir, one compiler per source file side by side; returns its path"""
    exe = os.path.join(workdir, "ski_load_check")
    # (the sanitizers' runtimes linked into the program: it then runs the same whatever else a machine preloads)
    flags = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    srcs = [os.path.join(REPO, "tools", "ski_load_check.cpp")] + [os.path.join(HOST, s + ".cpp") for s in SOURCES]
    objs = [os.path.join(workdir, "%d.o" % i) for i in range(len(srcs))]
    jobs = [subprocess.Popen(["g++", *flags, "-c", "-o", o, s]) for s, o in zip(srcs, objs)]
    if any([j.wait() != 0 for j in jobs]):
        raise RuntimeError("ski_load_check does not compile")
    subprocess.run(["g++", *flags, "-static-libasan", "-static-libubsan", "-o", exe, *objs, "-lpthread", "-ldl"],
                   check=True)
    return exe


def run(exe, skis):
    """loads the models; returns the program's output, raises with it if a model or a sanitizer failed"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SKIRT_AMD_")}
    p = subprocess.run([exe, DATA, *skis], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    if p.returncode != 0:
        raise RuntimeError("ski_load_check: exit %d\n%s" % (p.returncode, p.stdout))
    return p.stdout


def main():
    with tempfile.TemporaryDirectory(prefix="skiload_") as d:
        sys.stdout.write(run(build(d), sys.argv[1:] or models()))


if __name__ == "__main__":
    main()
