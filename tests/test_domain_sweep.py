"""The host build of the device algorithm (cpu_baseline, default switches)
against the oracle over the whole parameter domain (tests/domain_cases.py):
statuses, finite masks and flux on wide_box(400), prior_box(400) and the four
disputed sets, and the status rules of MODEL_SPEC 6 at their edges.  What the
GPU tests of tests/test_gpu_domain.py compare on the device is compared here
without one.

The flux bound is derived, not measured: a contact phase may differ by
PHASE_ATOL = 1e-10, an exposure of half-width h cut into nsub sub-bins turns
a contact shift d into a visibility change d / (2h / nsub), and if all the
weight of the light curve had an edge in that sub-bin the flux would move by
PHASE_ATOL / (2h / nsub) of its scale: 5e-8 at nsub = 1, 1.5e-7 at nsub = 3.

Measured after the fixes this sweep led to (x86-64, default build):
- contacts: the oracle within 3.0e-12 in phase of the arbiter on the 400
  points of tests/test_contact_double.py; on an MI355X the device's contacts
  within 2.5e-11 of the oracle's over the 96 sets of tests/test_gpu_domain.py
  (flux there: 1.6e-11 of the scale);
- flux, port against oracle, worst over a population, in units of the flux
  scale: wide_box(400) 5.7e-11, prior_box(400) 5.0e-11, the disputed sets
  2.6e-12, the 14-parameter forms 1.6e-11 and 1.3e-11; the same at nsub = 3;
- statuses: 332 of wide_box(400) are OK and 68 have status 4; all of
  prior_box(400) are OK; no status differs, no set is on the exception list.

Findings (each resolved with the arbiter, element by element, from the
port's lfc_dump intervals of a -DLFC_COUNT build):
- the oracle lost a shallow donor well between the 32 samples of a chord
  that starts on rising Phi (the disputed sets; MODEL_SPEC 4.2): oracle wrong;
- the oracle's warm-started ray minimum kept the wrong one of two wells on
  chords that pass L1 (q = 5.5, a point 6e-4 a from L1: egress 0.05 early):
  oracle wrong;
- prior_box sets 105 and 191 (q = 6.5, i = 69 and 71 degrees) and the status
  edge q = 6, rdisc = r0 (1 - 1e-9) with the simple spot: bright-spot
  elements next to L1 whose ingress the port had 0.018 and 0.004 late, 7e-3
  of the flux scale: the tangency solve converged on the contact of one well
  while the line of sight was inside the lobe in the other: device algorithm
  wrong (lfg_device.hpp: tangency_near_l1, ray_min<3>).
"""
import functools

import numpy as np
import pytest

from tests import contact_double as cd
from tests import domain_cases as dc

PHASE_ATOL = 1e-10    # tests/test_gpu_parity.py
FLUX_RTOL = 1e-6      # the contract (tests/test_gpu_parity.py)
N, H = 301, 1e-3
NBOX = 400

# Sets above the derived bound whose excess the arbiter attributes to a
# vanishing chord (an element eclipsed for less than 1e-6 in phase, which one
# solver finds and the other does not): (population, index).  At most 1 % of
# a population, and each still within FLUX_RTOL.
EXCEPTIONS = {
}


def grid():
    x = np.linspace(-0.3, 0.3, N)
    return x, np.full(N, H)


def flux_bound(nsub):
    return PHASE_ATOL / (2.0 * H / nsub)


@pytest.fixture(scope="module")
def port(tmp_path_factory):
    from cpu_baseline import cpu
    path = cpu.build(out=str(tmp_path_factory.mktemp("sweep") / "liblfg_cpu.so"))
    return cpu.CpuPort(path)


def populations():
    return {"wide": dc.wide_box(NBOX), "prior": dc.prior_box(NBOX), "disputed": np.array(dc.DISPUTED),
            "wide14": dc.simple(dc.wide_box(NBOX)[:100]), "prior14": dc.simple(dc.prior_box(NBOX)[:100])}


@functools.lru_cache(maxsize=None)
def oracle_flux(name, nsub):
    """(status [W], flux [W, N]) of a population; computed once, read-only"""
    from oracle.oracle import Oracle
    O = Oracle()
    x, w = grid()
    pars = populations()[name]
    st = np.empty(len(pars), dtype=np.int32)
    fl = np.empty((len(pars), N))
    for i, p in enumerate(pars):
        st[i], fl[i] = O.flux(p, x, w, nsub=nsub)
    st.setflags(write=False)
    fl.setflags(write=False)
    return st, fl


def compare(name, nsub, got, gst):
    """asserts statuses and finite masks; returns the per-set flux difference in units of the flux scale"""
    ost, ofl = oracle_flux(name, nsub)
    assert np.array_equal(gst, ost), np.flatnonzero(gst != ost)
    assert np.array_equal(np.isfinite(got), np.isfinite(ofl))
    err = np.zeros(len(ost))
    for i in np.flatnonzero(ost == 0):
        fin = np.isfinite(ofl[i])
        if fin.any():
            err[i] = np.max(np.abs(got[i][fin] - ofl[i][fin])) / np.max(np.abs(ofl[i][fin]))
    return err


@pytest.mark.parametrize("nsub", [1, 3])
@pytest.mark.parametrize("name", ["wide", "prior", "disputed", "wide14", "prior14"])
def test_port_matches_oracle_over_the_domain(port, name, nsub):
    pars = populations()[name]
    x, w = grid()
    got, gst = port.flux(pars, x, w, nsub=nsub, nthreads=4)
    err = compare(name, nsub, got, gst)
    ost, _ = oracle_flux(name, nsub)
    n_ok = int(np.sum(ost == 0))
    print("%s nsub %d: %d sets, %d status-OK, statuses %s, worst flux difference %.2e of the scale (set %d)"
          % (name, nsub, len(pars), n_ok, sorted(set(ost.tolist())), err.max(), int(np.argmax(err))))
    assert n_ok >= 0.3 * len(pars)
    if name == "prior":
        assert n_ok == len(pars)      # the Roche priors imply a valid model
    listed = sorted(k for (pop, k) in EXCEPTIONS if pop == name)
    assert len(listed) <= 0.01 * len(pars)
    over = np.flatnonzero(err > flux_bound(nsub))
    assert set(over.tolist()) <= set(listed), [(int(k), float(err[k])) for k in over]
    assert np.all(err[listed] <= FLUX_RTOL) if listed else True


def test_findphi_edge_is_unambiguous(oracle):
    """status_edges() straddles findphi(q, 90) by a relative 1e-9: the
    oracle's value and the arbiter's (bisection) agree far inside that, so
    the side each case lies on does not depend on the solver"""
    for q in (0.003, 0.1, 1.0, 6.0):
        fo, fa = oracle.findphi(q, 90.0), cd.findphi(q, 90.0)
        print("q %g: findphi(q, 90) oracle %.15f arbiter %.15f (relative %.1e)" % (q, fo, fa, abs(fo - fa) / fo))
        assert abs(fo - fa) <= 1e-10 * fo


def _edge_sets(npar):
    edges = [e for e in dc.status_edges() if npar == 18 or not e[3]]
    pars = np.array([e[1] for e in edges])
    return edges, (pars if npar == 18 else dc.simple(pars))


@pytest.mark.parametrize("npar", [18, 14])
def test_status_edges(oracle, port, npar):
    edges, pars = _edge_sets(npar)
    x, w = grid()
    rng = np.random.default_rng(2)
    y = 0.1 + 0.01 * rng.standard_normal(N)
    ye = np.full(N, 0.01)
    fl, st = port.flux(pars, x, w, nthreads=4)
    ll, st2 = port.lnlike(pars, x, w, y, ye, nthreads=4)
    for k, (name, _, want, _) in enumerate(edges):
        ost, ofl = oracle.flux(pars[k], x, w)
        assert ost == want, (name, ost, want)                # the oracle follows the spec
        assert st[k] == want and st2[k] == want, (name, st[k], st2[k], want)
        if want != 0:
            assert np.all(np.isnan(fl[k])) and np.isneginf(ll[k]), name
            assert np.all(np.isnan(ofl)), name
        else:
            assert np.all(np.isfinite(fl[k])) and np.isfinite(ll[k]), name
            assert np.max(np.abs(fl[k] - ofl)) <= flux_bound(1) * np.max(np.abs(ofl)), name
    assert {e[2] for e in edges} == {0, 1, 2, 3, 4, 5}
