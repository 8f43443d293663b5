"""The particle-dust fixtures are reproducible from the repository: the reference SKIRT v7.3 binary rebuilt from its
own sources (oracle/ref.mk) regenerates every committed file under tests/golden/ref_particles byte for byte
(tests/golden/make_particle_fixtures.sh, which runs it with -i tests/golden/particles), and make_particles.py
regenerates the committed particle files. Needs the reference sources and the image's Qt: build container only, as
tests/test_reference_rebuild.py."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

from golden import compare_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REPO, "tests", "golden", "make_particle_fixtures.sh")
GOLD = os.path.join(REPO, "tests", "golden", "ref_particles")
PART = os.path.join(REPO, "tests", "golden", "particles")
REF_SRC = os.environ.get("SKIRT_REFERENCE", "/root/reference")
MOC = "/opt/conda/bin/moc"
MODELS = ["part_oct", "part_oct_neg", "part_oct_bary", "part_cart", "part_vor", "part_vor_dd", "part_few"]
needs_reference = pytest.mark.skipif(not (os.path.isdir(REF_SRC) and os.path.exists(MOC)),
                                     reason="needs the reference sources and the image's Qt (build container)")


def _fixtures():
    out = subprocess.run(["bash", SCRIPT], env=dict(os.environ, LIST="1"), check=True, capture_output=True, text=True)
    return [line.split() for line in out.stdout.splitlines() if line.strip()]


def test_fixture_list_covers_every_committed_file():
    fixtures = _fixtures()
    assert [f[0] for f in fixtures] == MODELS
    assert all(f[1] == "4357" and f[2] == f[0] + "_s4357" and f[3] == "1" for f in fixtures)
    committed = [n for n in os.listdir(GOLD) if os.path.isfile(os.path.join(GOLD, n))]
    assert committed and not [n for n in committed if not any(n.startswith(f[2] + "_") for f in fixtures)]
    for f in fixtures:
        text = open(os.path.join(REPO, "tests", "golden", "ski", f[0] + ".ski")).read()
        assert 'seed="4357"' in text and 'packages="4e3"' in text and 'pixelsX="32"' in text
        assert 'writeCellProperties="true"' in text and 'writeConvergence="true"' in text
        for what in ("i30_sed.dat", "i90_sed.dat", "ds_convergence.dat", "log_excerpt.txt"):
            assert f[2] + "_" + what in committed, (f, what)
        assert f[2] + "_ds_cellprops.dat" in committed or f[2] + "_ds_cellprops.dat.gz" in committed
    assert "part_cart_s4357_ds_isrf.dat.gz" in committed
    assert max(os.path.getsize(os.path.join(GOLD, n)) for n in committed) < 1 << 18
    assert max(os.path.getsize(os.path.join(PART, n)) for n in os.listdir(PART)) < 1 << 18


def test_particle_files_are_what_the_generator_writes(tmp_path):
    shutil.copy(os.path.join(PART, "make_particles.py"), str(tmp_path / "make_particles.py"))
    subprocess.run([sys.executable, str(tmp_path / "make_particles.py")], check=True)
    for name in ("cloud.dat", "cloud_neg.dat", "few.dat"):
        assert open(str(tmp_path / name), "rb").read() == open(os.path.join(PART, name), "rb").read(), name
    assert sorted(os.listdir(PART)) == ["cloud.dat", "cloud_neg.dat", "few.dat", "make_particles.py"]


@needs_reference
def test_rebuilt_reference_regenerates_every_fixture(tmp_path):
    jobs = str(min(8, os.cpu_count() or 1))
    subprocess.run(["make", "-s", "-f", "oracle/ref.mk", "-j", jobs, "REF=" + REF_SRC], cwd=REPO, check=True)
    binary = os.path.join(REPO, "oracle", "_ref", "skirt")
    assert os.access(binary, os.X_OK)
    env = dict(os.environ, SKIRT_REF_BIN=binary, DEST=str(tmp_path))
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda f: subprocess.run(["bash", SCRIPT, f[0]], env=env, check=True, capture_output=True),
                      _fixtures()))
    assert compare_ref.differing(GOLD, str(tmp_path)) == []
    assert compare_ref.differing(str(tmp_path), GOLD) == []
