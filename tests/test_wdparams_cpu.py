"""CPU: the white-dwarf atmosphere fit (MODEL_SPEC section 13) without a GPU.

  * the fixed batch holds every category the tests rely on;
  * the scipy double (tests/wd_double.py) against the reference's own
    wdparams_new.py on that batch (tests/golden/wdparams_ref.npz, made by
    tools/make_wd_golden.py), at ten times the largest difference measured
    when the fixture was made (profiles/wdparams/README.md);
  * the host twin lfg_cpu_wd_lnprob (lfg_wd.hpp compiled for the host)
    against the double, within the double's per-row bounds, and against the
    golden;
  * the input parser on the shipped wdinput.dat, fluxes_from_chain against a
    plain numpy restatement, the table readers, and the export sets.
"""
import os

import numpy as np
import pytest

from tests import wd_double as wdd

# double against golden: ten times the largest relative difference measured
# (relative to max(|golden|, 1)); the magnitudes and the Flux members agreed
# to the last bit
GOLD_RTOL = {"chisq": 1.6e-14, "ln_prior": 6.8e-15, "ln_like": 1.7e-14, "ln_prob": 1.6e-14}
CATEGORIES = ("interior", "node", "logg_knot", "teff_nonknot_node", "clamped", "plax_edge", "ebv_zero", "prior_edge",
              "gauss_tail", "nonfinite")


@pytest.fixture(scope="module")
def port():
    from cpu_baseline import cpu
    cpu.build()
    return cpu.CpuPort()


@pytest.fixture(scope="module")
def golden():
    return np.load(wdd.GOLDEN)


def test_batch_holds_every_category():
    b, ref = wdd.shared("A", False)
    th, cat = b["theta"], b["cat"]
    assert set(cat) == set(CATEGORIES) and all(m.any() for m in cat.values())
    loggs, teffs, _ = wdd.load_table()
    assert all(t in teffs and g in loggs for t, g in th[cat["node"], :2])
    assert np.all(th[cat["logg_knot"], 1] == 8.0)
    assert set(th[cat["teff_nonknot_node"], 0]) == {2750.0, 85000.0} and 2750.0 in teffs and 85000.0 in teffs
    c = th[cat["clamped"]]
    assert {1000.0, 95000.0} <= set(c[:, 0]) and {6.5, 9.6} <= set(c[:, 1])
    assert teffs[0] > 1000 and teffs[-1] < 95000 and loggs[0] > 6.5 and loggs[-1] < 9.6
    assert {0.0, -1.0, 1e-6} <= set(th[cat["plax_edge"], 2])
    assert np.all(th[cat["ebv_zero"], 3] == 0.0)
    assert not np.isfinite(th[cat["nonfinite"]]).all(axis=1).any()
    assert np.isfinite(th[~cat["nonfinite"]]).all()
    for s, c in wdd.COMBOS:
        r = wdd.shared(s, c)[1]
        assert np.isfinite(r["ln_prob"]).sum() >= len(th) / 2
        tail = r["ln_prob"][cat["gauss_tail"]]
        assert np.isfinite(tail).any() and (tail == -np.inf).any()   # each side of a Gaussian's underflow
        edge = r["ln_prob"][cat["prior_edge"]]
        assert np.isfinite(edge).any() and (edge == -np.inf).any()
    # plax <= 0 under the Gaussian prior of set A: F = 0 and a finite chi^2
    pe = ref["ln_prob"][cat["plax_edge"]]
    assert np.isfinite(pe).all() and np.all(ref["F"][cat["plax_edge"]][:2] == 0.0)


@pytest.mark.parametrize("prior_set,corrected", wdd.COMBOS)
def test_double_against_reference(golden, prior_set, corrected):
    b, ref = wdd.shared(prior_set, corrected)
    tag = prior_set + ("1" if corrected else "0")
    assert np.array_equal(golden["theta"], b["theta"], equal_nan=True)
    fin = ref["status"] == wdd.ST_OK
    assert np.array_equal(golden["mags_" + tag][fin], ref["mags"][fin])
    assert np.array_equal(golden["obs_mag_" + tag], ref["mag"]) and np.array_equal(golden["obs_err_" + tag], ref["err"])
    for k, rtol in GOLD_RTOL.items():
        g = golden[k + "_" + tag][fin]
        r = ref["ln_like_raw" if k == "ln_like" else k][fin]
        if k == "ln_prior":
            r = np.where(np.isfinite(ref["ln_prob"][fin]), r, -np.inf)
        assert np.array_equal(np.isfinite(g), np.isfinite(r)), k
        ok = np.isfinite(g)
        assert np.all(g[~ok] == -np.inf), k
        err = np.abs(g[ok] - r[ok]) / np.maximum(np.abs(g[ok]), 1.0)
        print(k, tag, "largest relative difference %.3g" % err.max())
        assert err.max() <= rtol, (k, float(err.max()))


@pytest.mark.parametrize("prior_set,corrected", wdd.COMBOS)
def test_twin_against_double_and_golden(port, golden, prior_set, corrected):
    b, ref = wdd.shared(prior_set, corrected)
    M = wdd.build_model(prior_set, corrected)
    lnp, ll, mags, st = port.wd_lnprob(b["theta"], M)
    dm, rel = wdd.check_against(lnp, mags, ll, st, ref, "twin")
    print("twin - double: magnitudes %.3g, ln_prob %.3g of its bound" % (dm, rel))
    tag = prior_set + ("1" if corrected else "0")
    g = golden["ln_prob_" + tag]
    fin = ref["status"] == wdd.ST_OK
    ok = np.isfinite(g) & fin
    assert np.array_equal(np.isfinite(lnp[fin]), np.isfinite(g[fin]))
    assert np.all(np.abs(lnp[ok] - g[ok]) <= ref["bound"][ok] + GOLD_RTOL["ln_prob"] * np.maximum(np.abs(g[ok]), 1.0))
    gm = golden["mags_" + tag][fin]
    inf = np.isinf(gm)
    assert np.max(np.abs(mags[fin][~inf] - gm[~inf])) <= wdd.DM
    # threads and strides: the same bits
    chain = np.full((len(lnp), 9), np.nan)
    chain[:, :4] = b["theta"]
    lnp2, ll2, mags2, st2 = port.wd_lnprob(chain.reshape(-1), M, ld=9, n=len(lnp), nthreads=3)
    assert np.array_equal(lnp, lnp2) and np.array_equal(ll, ll2) and np.array_equal(mags, mags2, equal_nan=True)
    assert np.array_equal(st, st2)


def test_parser_reads_the_shipped_input():
    from lfit_python_amd import wdparams
    path = os.path.join(wdd.WD_ATMOS, "wdinput.dat")
    cfg = wdparams.parse_input(path)   # (a byte that is not UTF-8: test_parser_optional_keys)
    assert cfg == {"fit": "1", "nburn": "2000", "nprod": "1000", "nwalkers": "200", "nthread": "6", "scatter": "0.10",
                   "flat": "0", "thin": "1", "teff": "20000     uniform     5000     90000.0",
                   "logg": "7.5       uniform     7.01     9.49", "ebv": "0.01      uniform     0.00     0.0137",
                   "plax": "2.4041     gauss     2.4041     0.1564", "syserr": "0.03",
                   "chain": "../hierarchical_FinalFit/chain_prod.txt"}
    assert set(cfg) <= set(wdparams.INPUT_KEYS)
    from lfit_python_amd.tree import Param
    p = Param.fromString("plax", cfg["plax"])
    assert (p.currVal, p.prior.type, p.prior.p1, p.prior.p2) == (2.4041, "gauss", 2.4041, 0.1564)
    assert wdd.PRIOR_SETS["A"] == {k: " ".join(cfg[k].split()) for k in ("teff", "logg", "plax", "ebv")}


def test_parser_optional_keys(tmp_path):
    from lfit_python_amd import wdparams
    f = tmp_path / "in.dat"
    f.write_bytes(b"# a comment \xb5\nflux_kg5 = 0.05 0.001  # mJy\ncorrect_g = tnt uspec g\nntemps=1\n\nnoequals\n")
    assert wdparams.parse_input(str(f)) == {"flux_kg5": "0.05 0.001", "correct_g": "tnt uspec g", "ntemps": "1"}


def test_fluxes_from_chain_against_numpy():
    from lfit_python_amd import wdparams
    rng = np.random.default_rng(11)
    n = 4000
    names = ["wdFlux_u", "q", "wdFlux_g", "wdFlux_kg5", "wdflux_r"]
    chain = np.column_stack([rng.normal(0.07, 0.002, n), rng.uniform(0, 1, n), rng.normal(0.09, 0.001, n),
                             rng.normal(0.05, 0.001, n), rng.normal(0.073, 0.0009, n)])
    chain[::97, 0] += 0.05          # outliers the clipping drops
    chain[::131, 4] -= 0.02
    got = wdparams.fluxes_from_chain(chain, names, syserr=0.03)
    assert [f.orig_band for f in got] == ["u", "g", "r"] and [f.band for f in got] == ["u_s", "g_s", "r_s"]
    for f, col in zip(got, (0, 2, 4)):
        x = chain[:, col]
        for _ in range(5):
            med, sd = np.median(x), x.std()
            keep = np.abs(x - med) <= 3.0 * sd
            if keep.all():
                break
            x = x[keep]
        assert len(x) < n or col == 2
        assert f.flux == x.mean()
        assert f.err == np.sqrt(x.std() ** 2 + (x.mean() * 0.03) ** 2)
        assert f.mag == 2.5 * np.log10(3631e3 / x.mean())
    assert abs(got[0].flux - 0.07) < 2e-4        # the outliers are gone


def test_tables_and_packing():
    from lfit_python_amd import wdparams
    t = wdparams.load_da_table(os.path.join(wdd.WD_ATMOS, "Bergeron", "Table_DA_sdss"))
    loggs, teffs, cols = wdd.load_table()
    assert np.array_equal(t.loggs, loggs) and np.array_equal(t.teffs, teffs) and (len(loggs), len(teffs)) == (5, 51)
    for band in cols:
        assert np.array_equal(t.band(band), cols[band])
    assert np.array_equal(t.band("kg5"), cols["g_s"] - 0.2240 * (cols["g_s"] - cols["r_s"]) ** 2 -
                          0.3590 * (cols["g_s"] - cols["r_s"]) + 0.0460)
    M = wdd.build_model("A", True)
    assert (M.arrays["tx"].size, M.arrays["ty"].size, M.arrays["c"].size) == (9, 55, 5 * 5 * 51)
    assert (M.arrays["ctx1"].size, M.arrays["cty1"].size, M.arrays["cc1"].size) == (86, 17, 82 * 13)
    S = M.host_struct()
    assert [bool(S.cc[b]) for b in range(5)] == [False, True, True, False, False]
    kg5 = wdd.build_model("A", False, fluxes=[(0.09, 0.001, "kg5", None)])
    assert kg5.obs_fluxes[0].band == "kg5" and kg5.host_struct().k[0] == 3.5


def test_export_sets():
    from lfit_python_amd import _native
    assert set(_native.EXPORTS_WD) == {"lfg_wd_lnprob", "lfg_wd_step_half"}
    assert not set(_native.EXPORTS_WD) & set(_native.EXPORTS)
    assert not set(_native.EXPORTS_WD) & set(_native.EXPORTS_PHYSPAR)
    header = open(os.path.join(_native.REPO, "include", "lfg_wd.h")).read()
    lfg_h = open(os.path.join(_native.REPO, "include", "lfg.h")).read()
    for name in _native.EXPORTS_WD:
        assert "int %s(" % name in header and name not in lfg_h
    assert os.path.join(_native.REPO, "include", "lfg_wd.h") in _native.HEADERS
    assert any(p.endswith("lfg_wd.hip") for p in _native.SOURCES)
    assert ("#define LFG_WD_MAX_BANDS  %d" % _native.WD_MAX_BANDS) in header
    assert ("#define LFG_WD_MAX_KNOTS  %d" % _native.WD_MAX_KNOTS) in header
