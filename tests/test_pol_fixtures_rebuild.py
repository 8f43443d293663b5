"""The fixtures of the polarised models are reproducible from the repository: the reference SKIRT v7.3 binary rebuilt
from its own sources (oracle/ref.mk) regenerates every committed file under tests/golden/ref_pol byte for byte
(tests/golden/make_pol_fixtures.sh; time stamps masked, tests/golden/compare_ref.py). Needs the reference sources and
the image's Qt: build container only, as tests/test_geom_fixtures_rebuild.py."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from golden import compare_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REPO, "tests", "golden", "make_pol_fixtures.sh")
GOLD = os.path.join(REPO, "tests", "golden", "ref_pol")
REF_SRC = os.environ.get("SKIRT_REFERENCE", "/root/reference")
MOC = "/opt/conda/bin/moc"
MODELS = ["pol_torus_cart", "pol_2comp_sph2"]

pytestmark = pytest.mark.skipif(not (os.path.isdir(REF_SRC) and os.path.exists(MOC)),
                                reason="needs the reference sources and the image's Qt (build container)")


def _fixtures():
    out = subprocess.run(["bash", SCRIPT], env=dict(os.environ, LIST="1"), check=True, capture_output=True, text=True)
    return [line.split() for line in out.stdout.splitlines() if line.strip()]


def test_fixture_list_covers_every_committed_file():
    fixtures = _fixtures()
    assert [f[0] for f in fixtures] == MODELS
    assert all(f[1] == "4357" and f[2] == f[0] + "_s4357" and f[3] == "0" for f in fixtures)  # not lean
    committed = [n for n in os.listdir(GOLD) if os.path.isfile(os.path.join(GOLD, n))]
    assert committed and not [n for n in committed if not any(n.startswith(f[2] + "_") for f in fixtures)]
    for f in fixtures:
        text = open(os.path.join(REPO, "tests", "golden", "ski", f[0] + ".ski")).read()
        assert 'seed="4357"' in text and "<ElectronDustMix" in text and 'pixelsX="16"' in text
        for kind in ("sed.dat", "stokesQ.fits", "stokesU.fits", "stokesV.fits", "scattered.fits"):
            assert f[2] + "_i30_" + kind in committed, (f, kind)
        assert f[2] + "_ds_convergence.dat" in committed and f[2] + "_log_excerpt.txt" in committed
    assert 'packages="1e6"' in open(os.path.join(REPO, "tests", "golden", "ski", "pol_torus_cart.ski")).read()
    assert 'packages="2e5"' in open(os.path.join(REPO, "tests", "golden", "ski", "pol_2comp_sph2.ski")).read()
    # every frame whole (16 x 16 pixels); the one 4096-cell ds_cellprops as a digest
    assert [n for n in committed if n.endswith("_digest.json")] == ["pol_torus_cart_s4357_ds_cellprops_digest.json"]
    assert not [n for n in committed if n.endswith("_ds_cellprops.dat")]
    assert max(os.path.getsize(os.path.join(GOLD, n)) for n in committed) <= 5760


def test_rebuilt_reference_regenerates_every_fixture(tmp_path):
    jobs = str(min(8, os.cpu_count() or 1))
    subprocess.run(["make", "-s", "-f", "oracle/ref.mk", "-j", jobs, "REF=" + REF_SRC], cwd=REPO, check=True)
    binary = os.path.join(REPO, "oracle", "_ref", "skirt")
    assert os.access(binary, os.X_OK)
    env = dict(os.environ, SKIRT_REF_BIN=binary, DEST=str(tmp_path))
    with ThreadPoolExecutor(max_workers=2) as pool:
        list(pool.map(lambda f: subprocess.run(["bash", SCRIPT, f[0]], env=env, check=True, capture_output=True),
                      _fixtures()))
    assert compare_ref.differing(GOLD, str(tmp_path)) == []
    assert compare_ref.differing(str(tmp_path), GOLD) == []
