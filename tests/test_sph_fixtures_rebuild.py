"""The Sphere1DDustGrid and Sphere2DDustGrid fixtures are reproducible from the repository: the reference SKIRT v7.3
binary rebuilt from its own sources (oracle/ref.mk) regenerates every committed file under tests/golden/ref_sph byte
for byte (tests/golden/make_sph_fixtures.sh; time stamps masked, tests/golden/compare_ref.py). Needs the reference
sources and the image's Qt: build container only, as tests/test_reference_rebuild.py."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from golden import compare_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REPO, "tests", "golden", "make_sph_fixtures.sh")
GOLD = os.path.join(REPO, "tests", "golden", "ref_sph")
REF_SRC = os.environ.get("SKIRT_REFERENCE", "/root/reference")
MOC = "/opt/conda/bin/moc"
MODELS = ["pan_sph1", "pan_sph1_sa", "pan_sph1_log", "pan_sph2", "disk_sph2", "pan_sph2_sa", "pan_sph2_cs", "oligo_sph2"]

pytestmark = pytest.mark.skipif(not (os.path.isdir(REF_SRC) and os.path.exists(MOC)),
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
        assert os.path.exists(os.path.join(REPO, "tests", "golden", "ski", f[0] + ".ski"))
        assert any(n.startswith(f[2] + "_") and n.endswith("_sed.dat") for n in committed), f
    assert max(os.path.getsize(os.path.join(GOLD, n)) for n in committed) == 46080  # the 32 x 32 total frames


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
