"""The trace lane of a finished FILL ray walks on to the interaction point (SKIRT_AMD_FUSE_WALK).

Unfused (0), a scattering order costs a packet two pipeline iterations: the FILL ray returns the path's optical
depth to the event kernel, which draws the interaction depth and queues a WALK ray along the same path. Fused
(1), the lane decides with the deviates the event kernel drew ahead for it, by the same function the event
kernel then decides with, and walks its own ray record again; 2 forces every odd slot to fall back to the
queued WALK ray, so both routes mix in one run. The packets, their random streams and their paths are the
same in all three: every count is equal and the tallies agree up to the order of the f64 atomic additions.
"""
import pytest

from test_gpu_parity import _assert_same_packets, run_gpu

pytestmark = pytest.mark.gpu

CASES = [
    ("pan_oct", 2000, False, None),
    ("pan_cart16", 2000, False, None),
    ("bin_pan", 1000, False, None),
    ("vor_pan", 1000, False, None),
    ("oligo_2comp", 3000, False, None),  # several components, minScattEvents 2, scattering bias 0.3
    ("pan_oct_sa", 500, True, None),     # the dust phases: self-absorption and the no-store kernel
    ("pan_oct", 2000, False, "1"),       # global atomics
]


_cache = {}  # finished runs, shared between the tests (read only)


def _runs(monkeypatch, name, packages, dust, modes, labs_global=None):
    if labs_global is not None:
        monkeypatch.setenv("SKIRT_AMD_LABS_GLOBAL", labs_global)
    runs = []
    for mode in modes:
        key = (name, packages, dust, labs_global, mode)
        if key not in _cache:
            monkeypatch.setenv("SKIRT_AMD_FUSE_WALK", mode)
            _cache[key] = run_gpu(name, packages=packages, dust=dust)
        runs.append(_cache[key])
    return runs


@pytest.mark.parametrize("name,packages,dust,labs_global", CASES)
def test_fused_equals_unfused(name, packages, dust, labs_global, monkeypatch):
    unfused, fused, mixed = _runs(monkeypatch, name, packages, dust, ("0", "1", "2"), labs_global)
    print(name, {m: r.stats()["iterations"] for m, r in (("0", unfused), ("1", fused), ("2", mixed))},
          {k: unfused.stats()[k] for k in ("segments_fill", "segments_walk", "segments_peel")})
    # (segments_walk equal, not bounded: the re-entered WALK is the same walk)
    _assert_same_packets(unfused, fused)
    _assert_same_packets(unfused, mixed)


def test_fused_packets_need_fewer_iterations(monkeypatch):
    """A packet with k scatterings visits the event kernel k + 1 times instead of 2 k + 1."""
    unfused, fused = _runs(monkeypatch, "pan_oct", 2000, False, ("0", "1"))
    print("iterations", unfused.stats()["iterations"], fused.stats()["iterations"])
    assert fused.stats()["iterations"] < unfused.stats()["iterations"]


@pytest.mark.parametrize("name,packages,dust", [("vor_pan_cs", 150, False), ("pan_oct_cs", 200, True)])
def test_continuous_scattering_is_not_fused(name, packages, dust, monkeypatch):
    """The continuous peel-off kernel draws a path-dependent number of deviates between the FILL ray and the
    interaction depth: those phases keep the two visits whatever the knob says."""
    unfused, fused = _runs(monkeypatch, name, packages, dust, ("0", "1"))
    _assert_same_packets(unfused, fused)
    assert fused.stats()["iterations"] == unfused.stats()["iterations"]
