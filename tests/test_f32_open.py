"""The FP32 opener of the element solves (LFG_F32_OPEN, lfg_device.hpp) on the
host build of the device algorithm (cpu_baseline, -DLFC_COUNT): built with
the switch on and off, 64 walkers of config 2's ball and of a grazing ball
(tests/f32_open_cases.py), one thread for the interval dumps.

Measured here (x86-64, IEEE 1/sqrt and 1/x in place of v_rsq_f32/v_rcp_f32):
config 2: intervals within 2.2e-12 in phase of the switch-off build, mean
wave-max FP64 lane steps 2.036 (switch off: 3.429), no nested-solver
fallback in either build; grazing ball: 94 % of the central walker's disc
elements eclipsed, intervals within 3.2e-12, wave-max 2.77 (3.97)."""
import ctypes

import numpy as np
import pytest

from tests import f32_open_cases as cases
from tests.test_gpu_lnprob import LNP_RTOL

AB_TOL = 6e-12       # phase: two solves, each within 3e-12 of a 1e-12 solve
WAVE_MAX_STEPS = 2.2  # mean over chunks of 64 items of the largest FP64 lane step count, cone step included
_dp = ctypes.POINTER(ctypes.c_double)


def _run(port, grazing):
    t, walk, ref, _ = cases.case(grazing)
    c0, d0 = (ctypes.c_ulonglong * 28)(), (ctypes.c_ulonglong * 5)()
    port.lib.lfc_counts(c0)
    port.lib.lfc_counts2(d0)
    ab = np.zeros(cases.W * 800 * 2)
    port.lib.lfc_dump(ab.ctypes.data_as(_dp), ctypes.c_long(0))  # clear
    lnp, _ = port.lnprob_batch(walk, t, nthreads=1)
    n = port.lib.lfc_dump(ab.ctypes.data_as(_dp), ctypes.c_long(ab.size))
    assert n == ab.size
    c1, d1 = (ctypes.c_ulonglong * 28)(), (ctypes.c_ulonglong * 5)()
    port.lib.lfc_counts(c1)
    port.lib.lfc_counts2(d1)
    c = np.array(c1[:4], dtype=np.int64) - np.array(c0[:4], dtype=np.int64)
    d = np.array(d1[:], dtype=np.int64) - np.array(d0[:], dtype=np.int64)
    return {"lnp": lnp, "ref": ref, "ab": ab.reshape(-1, 2), "lane": c[1] / c[0], "wave_max": c[3] / c[2],
            "f32_lane": d[0] / c[0], "fallbacks": int(d[1]), "root64": d[3] / d[2], "root32": d[4] / d[2]}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from cpu_baseline import cpu
    out = {}
    for on in (1, 0):
        path = cpu.build(out=str(tmp_path_factory.mktemp("f32open") / ("liblfc_%d.so" % on)),
                         extra=["-DLFC_COUNT", "-DLFG_F32_OPEN=%d" % on])
        port = cpu.CpuPort(path)
        for grazing in (False, True):
            out[on, grazing] = _run(port, grazing)
    return out


def _interval_diff(runs, grazing):
    on, off = runs[1, grazing]["ab"], runs[0, grazing]["ab"]
    ecl = off[:, 0] < off[:, 1]
    assert np.array_equal(on[:, 0] < on[:, 1], ecl)  # the same elements are eclipsed
    assert ecl.sum() > 0.5 * len(ecl)
    return float(np.abs(on - off)[ecl].max())


def _lnp_ok(r):
    assert np.all(np.isfinite(r["ref"])) and np.all(np.isfinite(r["lnp"]))
    np.testing.assert_allclose(r["lnp"], r["ref"], rtol=LNP_RTOL, atol=1e-9)


@pytest.mark.parametrize("grazing", [False, True], ids=["config2", "grazing"])
def test_intervals_match_the_switch_off_build(runs, grazing):
    d = _interval_diff(runs, grazing)
    print("max interval difference (phase): %.2e" % d)
    assert d <= AB_TOL


@pytest.mark.parametrize("grazing", [False, True], ids=["config2", "grazing"])
@pytest.mark.parametrize("on", [1, 0], ids=["on", "off"])
def test_lnprob_matches_oracle(runs, on, grazing):
    _lnp_ok(runs[on, grazing])


@pytest.mark.parametrize("grazing", [False, True], ids=["config2", "grazing"])
def test_no_more_fallbacks_than_switched_off(runs, grazing):
    print("nested-solver fallbacks on / off: %d / %d" % (runs[1, grazing]["fallbacks"], runs[0, grazing]["fallbacks"]))
    assert runs[1, grazing]["fallbacks"] <= runs[0, grazing]["fallbacks"]


def test_wave_max_steps(runs):
    on, off = runs[1, False], runs[0, False]
    print("wave-max FP64 lane steps on / off: %.3f / %.3f; FP32 steps per lane %.2f; donor root FP64 steps %.2f / %.2f"
          % (on["wave_max"], off["wave_max"], on["f32_lane"], on["root64"], off["root64"]))
    assert on["wave_max"] <= WAVE_MAX_STEPS
    assert off["f32_lane"] == 0 and off["root32"] == 0  # the switch-off build runs no float step
    assert on["f32_lane"] > 0


def test_donor_root_opener(runs, tmp_path):
    """-DLFG_F32_ROOT_STEPS=3 (not the default: it did not shorten k_pair):
    fewer FP64 steps of the donor radius root, the same ln_prob."""
    from cpu_baseline import cpu
    path = cpu.build(out=str(tmp_path / "liblfc_root.so"), extra=["-DLFC_COUNT", "-DLFG_F32_ROOT_STEPS=3"])
    r = _run(cpu.CpuPort(path), False)
    print("donor root FP64 steps per tile: %.2f opened with %.0f FP32 steps, %.2f without"
          % (r["root64"], r["root32"], runs[0, False]["root64"]))
    assert r["root32"] == 3
    # float lands ~1e-7 off: one FP64 step over ROOT_LAST and the last one, a third at float's worst
    assert r["root64"] <= 2.5 and r["root64"] < runs[0, False]["root64"] - 1.5
    _lnp_ok(r)


def test_grazing_population_holds_both_classes(runs):
    """the oracle's table of the central walker, and the ball's own disc
    elements (items 200..699 of each walker's 800 solves; the mirror images
    share their partners' class)"""
    _, _, _, frac = cases.case(True)
    ab = runs[0, True]["ab"].reshape(cases.W, 800, 2)[:, 200:700]
    ball = float(np.mean(ab[..., 0] < ab[..., 1]))
    print("eclipsed fraction of the disc elements: central walker %.3f, ball %.3f" % (frac, ball))
    assert cases.MIN_CLASS <= frac <= 1.0 - cases.MIN_CLASS
    assert cases.MIN_CLASS <= ball <= 1.0 - cases.MIN_CLASS
