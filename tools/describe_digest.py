"""Digest of what the host set-up builds, model by model: Simulation(ski).describe() writes the grid arrays, rho, the
source tables, the instruments and the Mueller tables (no device needed), and this prints `name sha256 size` of that
dump for every model under tests/golden/ski/ and benchmarks/, or the error text of a model that refuses to load.
The host-side counterpart of tools/device_asm_diff.py: run it on two builds and diff the listings; a set-up change
that is meant to keep every stored double must leave them equal.
Usage: python tools/describe_digest.py [model.ski ...] > listing.txt
       SKIRT_AMD_LIB=/path/to/another/libskirt_amd.so python tools/describe_digest.py > other.txt"""
import glob
import hashlib
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import skirt_amd  # noqa: E402


def models():
    found = []
    for d in ("tests/golden/ski", "benchmarks"):
        found += sorted(glob.glob(os.path.join(REPO, d, "*.ski")))
    return found


def digest(ski, workdir):
    """`sha256 size` of the model's descriptor dump, or its load error"""
    out = os.path.join(workdir, "descriptors.bin")
    try:
        skirt_amd.Simulation(ski).describe(out)
    except skirt_amd.SkirtError as e:
        return "error: %s" % e
    h = hashlib.sha256()
    with open(out, "rb") as f:
        for block in iter(lambda: f.read(1 << 20), b""):
            h.update(block)
    return "%s %d" % (h.hexdigest(), os.path.getsize(out))


def main():
    with tempfile.TemporaryDirectory(prefix="describe_") as d:
        for ski in sys.argv[1:] or models():
            print(os.path.relpath(os.path.abspath(ski), REPO), digest(ski, d), flush=True)


if __name__ == "__main__":
    main()
