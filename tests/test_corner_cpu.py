"""CPU: the corner-plot data (MODEL_SPEC section 16) without a GPU.

  * the double's bin rule (tests/corner_double.py) against np.histogram and
    np.histogram2d;
  * the host twin lfg_cpu_corner_hist / lfg_cpu_corner_levels (lfg_corner.hpp
    compiled for the host) against the double on the shared case list, and on
    the constructed level cases;
  * the export set and the header's functions; corner_columns on the golden
    input; thumb_plot on twin-made data.

Every comparison of counts is integer equality.
"""
import os
import re

import numpy as np
import pytest

from tests import chain_double as cd
from tests import corner_double as co

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_test_data", "mcmc_input.dat")


@pytest.fixture(scope="module")
def port():
    from cpu_baseline import cpu
    cpu.build()
    return cpu.CpuPort()


@pytest.fixture(scope="module")
def twin(port):
    def backend(buf, off, steps, W, row_len, sld, wld, cols, rng, nb):
        out = port.corner_hist(buf, steps, W, row_len, sld, wld, cols, rng, nb, offset=off)
        out["levels"] = port.corner_levels(out["h2"], co.FRACS)
        return out
    return backend


def test_bin_rule_is_numpys():
    """on random ranges, with values on, just below and just above every edge:
    the rule's bins count to np.histogram's, and pairs of them to
    np.histogram2d's"""
    rng = np.random.default_rng(3)
    for trial in range(60):
        nb = int(rng.choice(co.NBS + (3, 7, 33)))
        lo = rng.normal() * 10.0 ** rng.integers(-3, 7)
        hi = lo + abs(rng.normal()) * 10.0 ** rng.integers(-6, 4) + 1e-9 * abs(lo)
        e = np.linspace(lo, hi, nb + 1)
        assert np.all(np.diff(e) > 0)
        v = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), rng.uniform(lo, hi, 200),
                            [np.nan, np.inf, -np.inf]])
        u = rng.permutation(v)
        b, bu = co.bin_rule(v, lo, hi, nb), co.bin_rule(u, lo, hi, nb)
        assert np.array_equal(np.bincount(b[b >= 0], minlength=nb), np.histogram(v, bins=nb, range=(lo, hi))[0])
        both = (b >= 0) & (bu >= 0)
        want = np.histogram2d(v, u, bins=nb, range=((lo, hi), (lo, hi)))[0]
        got = np.zeros((nb, nb), dtype=np.int64)
        np.add.at(got, (b[both], bu[both]), 1)
        assert np.array_equal(got, want)
    # the narrow range repeats edges; the rule still agrees with histogram2d's searchsorted
    lo, hi = co.NARROW_RANGE
    assert np.any(np.diff(np.linspace(lo, hi, 51)) == 0)
    v = co.value_column("narrow", np.random.default_rng(1), 500)
    b = co.bin_rule(v, lo, hi, 50)
    got = np.zeros((50, 50), dtype=np.int64)
    np.add.at(got, (b[b >= 0], b[b >= 0]), 1)
    assert np.array_equal(got, np.histogram2d(v, v, bins=50, range=((lo, hi), (lo, hi)))[0])
    assert (b < 0).any() and got.sum() > 400


def test_pair_tile_constants_split_the_case_list():
    """the K of the case list meet one tile, a tile and a remainder, several tiles"""
    for nb, ks in ((50, (5, 6, 18)), (64, (4, 5))):
        T = co.PAIR_TILE[nb]
        assert ks[0] * (ks[0] - 1) // 2 <= T < ks[1] * (ks[1] - 1) // 2 < 2 * T
    assert 18 * 17 // 2 > 2 * co.PAIR_TILE[50]
    assert any(c[3] == 64 and c[4] == 4 for c in co.CASES) and {c[4] for c in co.CASES} >= {1, 2, 50, 64}


@pytest.mark.parametrize("c", co.CASES, ids=lambda c: "%dx%d-%s-C%d-K%d-nb%d-%s" % (c[0] + c[1:]))
def test_twin_case_list(twin, c):
    got, want = co.run_case(twin, c)
    size, kind, C, K, nb, mode = c
    x, cols, rng, _ = co.case(*c)
    # the identities: a pair's sum is the rows both columns use; summing out a column whose
    # every row is in range gives the other's marginal
    used = [co.bin_rule(x[:, :, cc].reshape(-1), rng[k][0], rng[k][1], nb) >= 0 if co.mobile(*rng[k])
            else np.zeros(x.shape[0] * x.shape[1], dtype=bool) for k, cc in enumerate(cols)]
    for p, (a, b) in enumerate(co.pairs(K)):
        assert got["h2"][p].sum() == int((used[a] & used[b]).sum())
        if used[b].all():
            assert np.array_equal(got["h2"][p].sum(axis=1), got["h1"][a])
        if used[a].all():
            assert np.array_equal(got["h2"][p].sum(axis=0), got["h1"][b])
    if mode == "immobile":
        assert got["flag"][1] == 1 and not got["h1"][1].any() and got["flag"][0] == 0 and got["h1"][0].any()
        for p, (a, b) in enumerate(co.pairs(K)):
            if 1 in (a, b):
                assert not got["h2"][p].any()


def test_case_list_meets_its_purposes():
    """the edge column puts values on both sides of the range and on its
    edges; the narrow range repeats edges at 50 bins; the default range of the
    constant columns is immobile"""
    x, cols, rng, want = co.case((64, 64), "chain_dev", 10, 10, 50, "cut")
    kinds = [co.COLUMNS[c % len(co.COLUMNS)] for c in cols]
    k = kinds.index("onedge")
    v = x[:, :, cols[k]].reshape(-1)
    assert (v < rng[k][0]).any() and (v > rng[k][1]).any() and (v == rng[k][1]).any() and (v == rng[k][0]).any()
    assert tuple(rng[k]) == co.ONEDGE_RANGE and tuple(rng[kinds.index("narrow")]) == co.NARROW_RANGE
    assert want["flag"][kinds.index("same")] == 1 and want["flag"][kinds.index("equal")] == 1
    assert want["flag"].sum() == 2 and want["h1"][kinds.index("nonfinite")].sum() > 0
    for kind in ("normal", "offset", "nonfinite"):     # cut on both sides
        kk = kinds.index(kind)
        assert 0 < want["h1"][kk].sum() < np.isfinite(x[:, :, cols[kk]]).sum()


def test_twin_everything_in_one_bin(twin):
    x = np.full((64, 64, 3), 0.25)
    x[:, :, 1] = 7.01
    buf, off, sld, wld = cd.layout(x, "chain_dev")
    got = twin(buf, off, 64, 64, 3, sld, wld, (2, 0, 1), [(0.0, 1.0), (0.0, 1.0), (6.0, 8.0)], 50)
    assert got["h2"][0, 12, 12] == 4096 and got["h2"].sum() == 3 * 4096 and got["h2"][1, 12, 25] == 4096
    assert np.array_equal(got["levels"], np.tile([4096, 4096, 4096, 4096], (3, 1)))


def test_twin_levels_constructed(port):
    for h, fracs, want in co.level_cases():
        assert tuple(co.levels(h, fracs)) == want
        got = port.corner_levels(h[None], fracs)
        assert got.shape == (1, len(fracs)) and tuple(got[0]) == want, (h, fracs, got)
    for bad in ((), (0.5,) * 9, (-0.1,), (1.5,), (np.nan,)):
        with pytest.raises(ValueError):
            port.corner_levels(np.zeros((1, 2, 2), np.int64), bad)
    assert port.corner_levels(np.zeros((0, 2, 2), np.int64), (0.5,)).shape == (0, 1)


def test_twin_refusals(port):
    v = np.arange(48.0)
    ok = dict(buf=v, steps=4, W=2, row_len=3, step_ld=6, walker_ld=3, cols=(2, 0), ranges=[(0, 50), (0, 50)], nb=5)
    assert port.corner_hist(**ok)["h2"].sum() == 8
    for change in (dict(steps=-1), dict(W=-1), dict(row_len=0), dict(step_ld=0), dict(walker_ld=0), dict(nb=0),
                   dict(nb=65), dict(cols=(0, 3)), dict(cols=(-1, 0)), dict(cols=(1, 1)), dict(cols=(), ranges=[]),
                   dict(cols=tuple(range(65)), ranges=[(0, 1)] * 65, row_len=65, buf=np.zeros(8 * 65), step_ld=130,
                        walker_ld=65)):
        with pytest.raises(ValueError):
            port.corner_hist(**dict(ok, **change))
    r = port.corner_hist(v, 0, 2, 3, 6, 3, (2, 0), [(0, 50), (1, 1)], 5)
    assert not r["h1"].any() and not r["h2"].any() and list(r["flag"]) == [0, 1]


def test_export_set_and_header():
    from lfit_python_amd import _native
    assert set(_native.EXPORTS_CORNER) == {"lfg_corner_workspace_size", "lfg_corner_tile_rows",
                                           "lfg_corner_pair_tile", "lfg_corner_hist", "lfg_corner_levels"}
    for other in (_native.EXPORTS, _native.EXPORTS_PHYSPAR, _native.EXPORTS_WD, _native.EXPORTS_CHAIN,
                  _native.EXPORTS_LIMBDARK):
        assert not set(_native.EXPORTS_CORNER) & set(other)
    path = os.path.join(_native.REPO, "include", "lfg_corner.h")
    header = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(lfg_\w+)\s*\(", code)) == set(_native.EXPORTS_CORNER)
    for name in ("lfg.h", "lfg_chain.h"):
        text = open(os.path.join(_native.REPO, "include", name)).read()
        assert not any(f in text for f in _native.EXPORTS_CORNER)
    assert path in _native.HEADERS and os.path.join(_native._HERE, "csrc", "lfg_corner.hpp") in _native.HEADERS
    assert any(p.endswith("lfg_corner.hip") for p in _native.SOURCES)
    for macro, value in (("LFG_CORNER_MAX_K", _native.CORNER_MAX_K), ("LFG_CORNER_MAX_BINS", _native.CORNER_MAX_BINS),
                         ("LFG_CORNER_MAX_LEVELS", _native.CORNER_MAX_LEVELS)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), header)


def test_corner_columns_on_the_golden_input():
    """the reference's rule written out by hand: the eclipse's parameters,
    then its band's, then the core's, those of the chain header only"""
    from lfit_python_amd import corner, cvmodel
    model = cvmodel.construct_model(GOLDEN)
    names = model.dynasty_par_names
    ecl = ["dFlux", "sFlux", "rdisc", "scale", "az", "fis", "dexp", "phi0", "exp1", "exp2", "yaw", "tilt"]
    band = ["wdFlux", "rsFlux", "ulimb"]
    core = ["q", "dphi", "rwd", "ln_ampin_gp", "ln_ampout_gp", "ln_tau_gp"]
    bands = {"0": "g", "1": "g", "2": "KG5", "3": "KG5", "4": "r", "5": "r"}
    got = corner.corner_columns(model, names)
    assert [e.label for e, _ in got] == ["0", "1", "2", "3", "4", "5"]
    for e, labels in got:
        want = ["%s_%s" % (p, e.label) for p in ecl] + ["%s_%s" % (p, bands[e.label]) for p in band] + \
               ["%s_core" % p for p in core]
        assert labels == [w for w in want if w in names] and len(labels) >= 18
    # a header that lacks some labels, in another order: the rule's order, the header's members
    short = ["q_core", "ulimb_g", "ln_prob_like", "phi0_1", "dFlux_1", "rwd_core", "wdFlux_r"]
    got = dict((e.label, labels) for e, labels in corner.corner_columns(model, short))
    assert got["1"] == ["dFlux_1", "phi0_1", "ulimb_g", "q_core", "rwd_core"]
    assert got["0"] == ["ulimb_g", "q_core", "rwd_core"] and got["4"] == ["wdFlux_r", "q_core", "rwd_core"]
    assert corner.corner_columns(model, []) == [(e, []) for e, _ in corner.corner_columns(model, names)]


def twin_data(port, K=4, immobile=False):
    """a CornerData from the twin's counts"""
    from lfit_python_amd import corner
    x = np.random.default_rng(9).normal(size=(500, 1, 6))
    cols = (4, 1, 5, 0)[:K]
    rng = np.array([(x[:, 0, c].min(), x[:, 0, c].max()) for c in cols])
    if immobile:
        rng[1] = 2.0, 2.0
    r = port.corner_hist(x.reshape(-1), 500, 1, 6, 6, 1, cols, rng, 20)
    mob = r["flag"] == 0
    edges = np.array([np.linspace(lo, hi, 21) if m else np.full(21, np.nan) for (lo, hi), m in zip(rng, mob)])
    return corner.CornerData(cols=np.array(cols), names=["p%d" % c for c in cols], edges=edges, hist1d=r["h1"],
                             hist2d=r["h2"], levels=port.corner_levels(r["h2"], corner.DEFAULT_LEVELS),
                             fracs=np.array(corner.DEFAULT_LEVELS), mobile=mob)


def test_corner_data_container(port, tmp_path):
    from lfit_python_amd import corner
    assert np.allclose(corner.DEFAULT_LEVELS, co.FRACS, rtol=0, atol=0)
    d = twin_data(port, immobile=True)
    assert [d.pair(a, b) for a, b in co.pairs(4)] == list(range(6))
    with pytest.raises(IndexError):
        d.pair(2, 2)
    back = corner.CornerData.load(d.save(str(tmp_path / "c.npz")))
    for k in corner.CornerData.FIELDS:
        assert np.array_equal(np.asarray(getattr(back, k)), np.asarray(getattr(d, k)), equal_nan=(k == "edges")), k
    s = d.select([0, 2, 3])
    assert s.names == ["p4", "p5", "p0"] and s.mobile.all()
    assert np.array_equal(s.hist2d, d.hist2d[[d.pair(0, 2), d.pair(0, 3), d.pair(2, 3)]])


def test_thumb_plot_draws_the_triangle(port):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    from lfit_python_amd import corner
    d = twin_data(port)
    fig = corner.thumb_plot(d)
    drawn = [ax for ax in fig.axes if ax.axison]
    assert len(fig.axes) == len(drawn) == 4 * 5 // 2
    assert sum(1 for ax in drawn if ax.collections) >= 6       # contours below the diagonal
    d = twin_data(port, immobile=True)                          # an immobile column is left out
    assert len([ax for ax in corner.thumb_plot(d).axes if ax.axison]) == 3 * 4 // 2
