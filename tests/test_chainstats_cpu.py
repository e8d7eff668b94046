"""CPU: the chain summary (MODEL_SPEC section 14) without a GPU.

  * the host twin lfg_cpu_chain_stats / lfg_cpu_chain_clip
    (lfg_chain.hpp compiled for the host) against the numpy double
    (tests/chain_double.py) on the shared case list: sizes, layouts, value
    columns, quantile ranks, windows, the sigma clip, R-hat, refusals;
  * the export set, the header's functions, and modparams.csv's bytes.

Accuracy of mean, m2 and rhat: chain_double.moment_bound (8 times plain FP64
numpy's own deviation from the np.longdouble evaluation of the same column,
floor 8 ulp; measured figures: profiles/chainstats/README.md).
"""
import os
import re

import numpy as np
import pytest

from tests import chain_double as cd


@pytest.fixture(scope="module")
def port():
    from cpu_baseline import cpu
    cpu.build()
    return cpu.CpuPort()


@pytest.fixture(scope="module")
def twin(port):
    def backend(buf, off, steps, W, C, sld, wld, window, fracs, rhat):
        return port.chain_stats(buf, steps, W, C, sld, wld, offset=off, window=window, fracs=fracs, rhat=rhat)
    return backend


@pytest.mark.parametrize("size", cd.SIZES)
@pytest.mark.parametrize("kind", cd.LAYOUTS)
def test_twin_sizes_and_layouts(twin, size, kind):
    x, want = cd.shared(size[0], size[1], 7)
    cd.run_case(twin, x, kind, want=want)


@pytest.mark.parametrize("C", (1, 14, 18, 21, 87))
def test_twin_column_counts(twin, C):
    x, want = cd.shared(37, 6, C)
    cd.run_case(twin, x, "chain_dev", want=want)
    cd.run_case(twin, x, "padded", want=want)


def test_twin_flat_chain(twin):
    x, want = cd.shared(5003, 1, 18)
    cd.run_case(twin, x, "chain_dev", want=want)


def test_naive_sum_of_squares_fails_the_offset_column():
    """keeps the 1e6 + 1e-3 N(0, 1) column honest: the formula the issue rules
    out misses the bound the summary must meet"""
    x, want = cd.shared(64, 64, 7)
    c = cd.VALUE_COLUMNS.index("offset")
    v = x[:, :, c].reshape(-1)
    naive = np.sum(v * v) - np.sum(v) ** 2 / v.size
    assert abs(naive - want["m2"][c]) > cd.moment_bound(want["m2"][c], want["m2_np"][c])


def test_twin_quantile_ranks(twin):
    """f * (n - 1) on an integer and just beside one, and the ends"""
    rng = np.random.default_rng(11)
    fr = (0.0, 0.16, 0.5, 0.84, 1.0)
    hit = 0
    for n in range(2, 61):
        x = rng.normal(size=(n, 1, 1))
        cd.run_case(twin, x, fracs=fr)
        hit += sum(float(f * (n - 1)).is_integer() for f in fr[1:4])
    assert hit >= 30


@pytest.mark.parametrize("column", ("skewed", "gapped"))
def test_twin_sigma_clip_matches_astropy_restated(port, twin, column):
    from lfit_python_amd import wdparams
    v = getattr(cd, column)()
    x = v.reshape(-1, 1, 1)
    win = None
    for _ in range(5):
        r = twin(v, 0, v.size, 1, 1, 1, 1, win, (0.5,), False)
        win = port.chain_clip(r["n"], r["m2"], r["quant"][:, 0], 3.0, win)
    r = cd.run_case(twin, x, window=win, fracs=(0.5,))
    mean, med, std = wdparams.sigma_clipped_stats(v)
    keep = cd.clip_survivors(v)
    assert r["n"][0] == keep.size < v.size
    if column == "gapped":   # the intersection matters on this column (chain_double.gapped)
        assert cd.clip_no_intersection(v) != keep.size
    assert abs(r["mean"][0] - mean) <= 8 * cd.ulp(np.abs(keep).max())   # (np.mean's own rounding)
    assert abs(r["quant"][0, 0] - med) <= 4 * cd.ulp(np.abs(r["ostat"][0, 0]).max())   # (np.median is (a + b) / 2)
    assert abs(np.sqrt(r["m2"][0] / r["n"][0]) - std) <= 8 * cd.ulp(std)


def test_twin_window_that_excludes_everything(twin):
    x, _ = cd.shared(37, 6, 7)
    win = np.tile([1e301, 1e302], (7, 1))
    r = cd.run_case(twin, x, window=win)
    assert np.all(r["n"] == 0) and np.all(np.isnan(r["mean"])) and np.all(np.isnan(r["quant"]))
    assert r["n_bad"][cd.VALUE_COLUMNS.index("nonfinite")] > 0


def rhat_chains():
    rng = np.random.default_rng(5)
    mixed = rng.normal(size=(64, 64, 3))
    offset = mixed + np.linspace(-2.0, 2.0, 64)[None, :, None]
    return mixed, offset


def test_twin_rhat(twin):
    mixed, offset = rhat_chains()
    r = cd.run_case(twin, mixed, rhat=True)
    assert np.all(np.abs(r["rhat"] - 1.0) < 0.05)
    r = cd.run_case(twin, offset, "walker_major", rhat=True)
    assert np.all(r["rhat"] > 1.5)
    for steps, W in ((1, 5), (5, 1)):
        r = cd.run_case(twin, cd.chain(steps, W, 2), rhat=True)
        assert np.all(np.isnan(r["rhat"]))


def test_twin_refusals(port):
    v = np.arange(24.0)
    ok = dict(buf=v, steps=4, W=2, C=3, step_ld=6, walker_ld=3, fracs=(0.5,))
    port.chain_stats(**ok)
    for change in (dict(steps=-1), dict(W=-1), dict(C=0), dict(C=4097), dict(step_ld=0), dict(walker_ld=0),
                   dict(fracs=(0.5, 1.5)), dict(fracs=(-0.1,)), dict(fracs=(np.nan,)), dict(fracs=(0.5,) * 9),
                   dict(window=np.zeros((3, 2)), rhat=True)):
        args = dict(ok, **change)
        if args["C"] > 3:
            args["buf"] = np.zeros(8 * 4097)
            args["step_ld"], args["walker_ld"] = 2 * 4097, 4097
        with pytest.raises(ValueError):
            port.chain_stats(**args)
    r = port.chain_stats(v, 0, 2, 3, 6, 3, fracs=(0.5,), rhat=True)
    assert np.all(r["n"] == 0) and np.all(np.isnan(r["quant"])) and np.all(np.isnan(r["rhat"]))


def test_export_set_and_header():
    from lfit_python_amd import _native
    assert set(_native.EXPORTS_CHAIN) == {"lfg_chain_workspace_size", "lfg_chain_tile_rows", "lfg_chain_hist_tile",
                                          "lfg_chain_stats", "lfg_chain_clip"}
    for other in (_native.EXPORTS, _native.EXPORTS_PHYSPAR, _native.EXPORTS_WD):
        assert not set(_native.EXPORTS_CHAIN) & set(other)
    path = os.path.join(_native.REPO, "include", "lfg_chain.h")
    header = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(lfg_\w+)\s*\(", code)) == set(_native.EXPORTS_CHAIN)
    lfg_h = open(os.path.join(_native.REPO, "include", "lfg.h")).read()
    assert not any(name in lfg_h for name in _native.EXPORTS_CHAIN)
    assert path in _native.HEADERS and os.path.join(_native._HERE, "csrc", "lfg_chain.hpp") in _native.HEADERS
    assert any(p.endswith("lfg_chain.hip") for p in _native.SOURCES)
    assert ("#define LFG_CHAIN_MAX_C   %d" % _native.CHAIN_MAX_C) in header
    assert ("#define LFG_CHAIN_MAX_NQ  %d" % _native.CHAIN_MAX_NQ) in header


def test_modparams_csv_bytes(port, tmp_path):
    """the twin's numbers through chainstats.write_modparams against pandas'
    own mean / quantile / to_csv.  The values are multiples of 1/8 and the row
    count a power of two, so the mean is exact whatever the summation order."""
    import pandas as pd
    from lfit_python_amd import chainstats
    names = ["wdFlux_0", "dFlux_0", "q", "dphi"]
    rng = np.random.default_rng(2)
    flat = rng.integers(-400, 400, size=(64, 4)) / 8.0
    r = port.chain_stats(flat, 64, 1, 4, 4, 1, fracs=(0.16, 0.84))
    path, _ = chainstats.write_modparams(names, r["mean"], r["quant"][:, 1], r["quant"][:, 0], str(tmp_path))
    data = pd.DataFrame(flat, columns=names)
    result = pd.DataFrame()
    result["mean"] = data.mean()
    result["84th percentile"] = data.quantile(0.84)
    result["16th percentile"] = data.quantile(0.16)
    want = tmp_path / "pandas.csv"
    result.loc[names, :].to_csv(want, header=True)
    assert open(path, "rb").read() == open(want, "rb").read()
    assert open(path).readline().strip() == ",mean,84th percentile,16th percentile"
