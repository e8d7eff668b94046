"""The tabulated start of the element solves (LFG_TAB_START, lfg_device.hpp)
on the host build of the device algorithm (cpu_baseline, -DLFC_COUNT): the
direction function unit_dir against extended-precision cos and sin, and the
element intervals, ln_prob, nested-solver fallbacks and FP64 step counts of
the switch-on build against -DLFG_TAB_START=0, on the 64-walker populations
of tests/f32_open_cases.py (config 2's ball and the grazing ball), one thread
for the interval dumps.

Measured here (x86-64): unit_dir within 1.6e-16 of cos, sin over [-5, 5];
config 2: intervals within 2.3e-12 in phase of the switch-off build, mean
wave-max FP64 lane steps 2.036 (switch off: 2.036); grazing ball: within
3.2e-12, wave-max 2.764 (2.766); with -DLFG_F32_OPEN=0 as well 2.2e-12 and
3.2e-12; no nested-solver fallback in any build."""
import ctypes

import numpy as np
import pytest

from tests.test_f32_open import AB_TOL, WAVE_MAX_STEPS, _lnp_ok, _run

# the table's <= 1 ulp, and the roundings of cd, sd, the two products and the
# final add / fma of rotate(), each <= 1.1e-16
DIR_TOL = 6e-16
UNIT_MAX = 5.0
# a float direction that disagrees with its float angle costs a second FP64
# step: the mean wave-max may not rise by more than this over the switch-off build
WAVE_MAX_RISE = 0.02
_dp = ctypes.POINTER(ctypes.c_double)

BUILDS = {"on": [], "off": ["-DLFG_TAB_START=0"], "on_f64": ["-DLFG_F32_OPEN=0", "-DLFG_TAB_START=1"]}


@pytest.fixture(scope="module")
def ports(tmp_path_factory):
    from cpu_baseline import cpu
    d = tmp_path_factory.mktemp("tabstart")
    return {k: cpu.CpuPort(cpu.build(out=str(d / ("liblfc_%s.so" % k)), extra=["-DLFC_COUNT"] + extra))
            for k, extra in BUILDS.items()}


@pytest.fixture(scope="module")
def runs(ports):
    return {(k, grazing): _run(ports[k], grazing) for k in BUILDS for grazing in (False, True)}


def _unit_dir(port, th):
    th = np.ascontiguousarray(th, dtype=np.float64)
    cs, sn = np.full(th.size, 7.0), np.full(th.size, 7.0)  # 7: not a cosine
    ok = np.zeros(th.size, dtype=np.int32)
    port.lib.lfc_unit_dir(th.ctypes.data_as(_dp), ctypes.c_long(th.size), cs.ctypes.data_as(_dp),
                          sn.ctypes.data_as(_dp), ok.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return cs, sn, ok


def _grid():
    k = np.arange(-80, 81) / 16.0
    g = np.concatenate([k, k - 1.0 / 32, k + 1.0 / 32, [0.0], np.linspace(-UNIT_MAX, UNIT_MAX, 40001),
                        np.random.default_rng(11).uniform(-UNIT_MAX, UNIT_MAX, 20000)])
    g = np.concatenate([g, np.nextafter(g, np.inf), np.nextafter(g, -np.inf)])
    return g


def test_unit_dir_matches_cos_sin(ports):
    assert np.finfo(np.longdouble).eps < 1e-18  # the reference: 64-bit significands or better
    g = _grid()
    th = g[np.abs(g) <= UNIT_MAX]
    assert th.size > 120000 and np.any(th == UNIT_MAX) and np.any(th == -UNIT_MAX) and np.any(th == 0.0)
    cs, sn, ok = _unit_dir(ports["on"], th)
    assert np.all(ok == 1)
    x = th.astype(np.longdouble)
    ec = float(np.max(np.abs(cs.astype(np.longdouble) - np.cos(x))))
    es = float(np.max(np.abs(sn.astype(np.longdouble) - np.sin(x))))
    print("unit_dir: max |cs - cos| %.2e, max |sn - sin| %.2e over %d angles" % (ec, es, th.size))
    assert ec <= DIR_TOL and es <= DIR_TOL


def test_unit_dir_refuses_what_the_table_does_not_cover(ports):
    g = _grid()
    out = g[np.abs(g) > UNIT_MAX]
    assert out.size >= 4  # +-5 and +-(5 + 1/32) with their neighbours
    th = np.concatenate([out, [np.nextafter(UNIT_MAX, np.inf), -np.nextafter(UNIT_MAX, np.inf), 1e3, -1e3, 3e9, -3e9,
                               1e300, -1e300, np.nan, np.inf, -np.inf]])
    cs, sn, ok = _unit_dir(ports["on"], th)
    assert np.all(ok == 0)
    assert np.all(cs == 7.0) and np.all(sn == 7.0)  # nothing written, hence nothing read


def _interval_diff(on, off):
    ecl = off[:, 0] < off[:, 1]
    assert np.array_equal(on[:, 0] < on[:, 1], ecl)  # the same elements are eclipsed
    assert ecl.sum() > 0.5 * len(ecl)
    return float(np.abs(on - off)[ecl].max())


@pytest.mark.parametrize("grazing", [False, True], ids=["config2", "grazing"])
@pytest.mark.parametrize("build", ["on", "on_f64"])
def test_intervals_match_the_switch_off_build(runs, build, grazing):
    """on_f64: -DLFG_F32_OPEN=0 -DLFG_TAB_START=1, the FP64 start from the float guess"""
    d = _interval_diff(runs[build, grazing]["ab"], runs["off", grazing]["ab"])
    print("%s: max interval difference (phase): %.2e" % (build, d))
    assert d <= AB_TOL


@pytest.mark.parametrize("grazing", [False, True], ids=["config2", "grazing"])
@pytest.mark.parametrize("build", ["on", "on_f64"])
def test_lnprob_matches_oracle(runs, build, grazing):
    _lnp_ok(runs[build, grazing])


@pytest.mark.parametrize("grazing", [False, True], ids=["config2", "grazing"])
@pytest.mark.parametrize("build", ["on", "on_f64"])
def test_no_more_fallbacks_than_switched_off(runs, build, grazing):
    on, off = runs[build, grazing]["fallbacks"], runs["off", grazing]["fallbacks"]
    print("%s: nested-solver fallbacks on / off: %d / %d" % (build, on, off))
    assert on <= off


def test_wave_max_steps(runs):
    on, off = runs["on", False], runs["off", False]
    print("wave-max FP64 lane steps on / off: %.3f / %.3f (grazing ball: %.3f / %.3f); FP32 steps per lane %.2f"
          % (on["wave_max"], off["wave_max"], runs["on", True]["wave_max"], runs["off", True]["wave_max"],
             on["f32_lane"]))
    assert on["wave_max"] <= WAVE_MAX_STEPS
    assert on["wave_max"] <= off["wave_max"] + WAVE_MAX_RISE
    assert on["f32_lane"] > 0 and runs["on_f64", False]["f32_lane"] == 0
