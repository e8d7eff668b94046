"""CPU: the host twins of the C ABI (cpu_baseline/lfg_cpu.cpp: lfg_device.hpp
and lfg_tables.hpp compiled for the host) as a stand-alone program under the
host's address, undefined-behaviour and float-cast sanitizers.

tests/abi_host_main.cpp reads cases from a file, allocates every buffer from
the heap at exactly its size, calls lfg_cpu_flux, lfg_cpu_lnlike,
lfg_cpu_lnprob and lfg_cpu_gp_predict and writes their outputs.  It is built
twice, -O2 and -O1 -g -fsanitize=address,undefined,float-cast-overflow
-fno-sanitize-recover=all, and both are run as that program (no sanitizer is
ever applied to code loaded into Python).  A finding in the shared headers is
a finding about the device code: the setup, stream table, element solver,
prior lanes and table lookups are the text the GPU compiles.

Cases
  flux, lnlike   sets of domain_cases.wide_box / prior_box / DISPUTED /
                 status_edges(), 12 per configuration taken in turn, in the
                 14- and 18-parameter forms, N of 1, 65, 512, 513, nsub of 1
                 and 3, and the window kinds of tests/test_gpu_pointmajor.py
                 (shuffled, descending, wrap, ragged, one NaN width) plus zero
                 and 1e-300 widths and w = NULL;
  lnprob         a chi^2 tree with every prior type at its edges
                 (prior_double's chunk cases), the Roche limit walkers, and two
                 GP trees of tests/gp_trees.py;
  gp_predict     a tests/gp_smoother.py case, with and without the variance.
Every second case asks for one thread and the others for four; the -O2 build
runs them the other way round.

Bounds.  Flux: tests/test_domain_sweep.py's derived bound for this port, a
contact shift of PHASE_ATOL seen through a sub-bin of width 2h / nsub, h the
narrowest window of the case, and never more than the FLUX_RTOL contract,
which is also the bound where a window has no width (point evaluation).
ln_like: what that flux bound B allows, sum_p |r_p| B scale / ye_p + N (B
scale / ye)^2 / 2 with r the oracle's residuals.  ln_prob: the bounds of
tests/test_cpu_baseline.py.  The GP posterior: gp_smoother's bar.  The two
builds must agree with each other within the same bounds.

The populations are sized from a measurement: 100 sets x 60 configurations
took 45 s single-threaded under these sanitizers here, 7.5 ms per set and
configuration; 96 configurations x 12 sets x (flux + lnlike) is 17 s of that
on one thread.  Measured with half the cases on four threads: the sanitized
program builds in 5 s and runs its 207 cases in 8 s, the whole test (the
oracle's references included) in 35 s.
"""
import os
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import domain_cases as dc
from tests import gp_smoother as gs
from tests import gp_trees
from tests import prior_double as pd
from tests.test_domain_sweep import FLUX_RTOL, PHASE_ATOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]
SETS_PER_CONFIG = 12
KINDS = ["regular", "shuffled", "descending", "wrap", "ragged", "nan_width", "zero", "tiny", "null_w"]
NEEDS_TWO = ("shuffled", "descending", "wrap", "ragged")
YE = 0.01


def build(tmp_path, tag, flags):
    exe = str(tmp_path / ("abi_host_" + tag))
    t0 = time.time()
    subprocess.run(["g++", "-std=c++17", "-fopenmp", "-march=x86-64-v3", "-Wno-unknown-pragmas"] + flags +
                   ["-I", os.path.join(ROOT, "cpu_baseline"), "-I", os.path.join(ROOT, "cpu_baseline", "shim"),
                    "-I", os.path.join(ROOT, "lfit_python_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "abi_host_main.cpp"),
                    os.path.join(ROOT, "cpu_baseline", "lfg_cpu.cpp")], check=True)
    return exe, time.time() - t0


# ------------------------------------------------------------------ the case file
class Cases:
    def __init__(self):
        self.blob, self.shapes = [], []

    def ints(self, *v):
        self.blob.append(np.asarray(v, dtype=np.int32).tobytes())

    def f64(self, *arrays):
        for a in arrays:
            self.blob.append(np.ascontiguousarray(a, dtype=np.float64).tobytes())

    def i32(self, *arrays):
        for a in arrays:
            self.blob.append(np.ascontiguousarray(a, dtype=np.int32).tobytes())

    def head(self, kind):
        self.ints(kind, 1 if len(self.shapes) % 2 == 0 else 4)

    def flux(self, pars, x, w, nsub, y=None, ye=None):
        W, P = pars.shape
        self.head(0 if y is None else 1)
        self.ints(W, P, x.size, nsub, int(w is not None))
        self.f64(pars, x)
        if w is not None:             # None: the twin is handed w = NULL (point evaluation)
            self.f64(w)
        if y is not None:
            self.f64(y, ye)
        self.shapes.append([("f8", (W, x.size) if y is None else (W,)), ("i4", (W,))])

    def lnprob(self, t, walkers):
        W = walkers.shape[0]
        consts = t.consts if len(t.consts) else np.zeros(1)
        self.head(2)
        self.ints(t.E, t.ndim, t.nsub, t.max_n, int(t.roche_priors), int(t.gp), int(t.fixed_invalid), consts.size,
                  t.x.size, W)
        self.i32(t.gather.reshape(-1), t.npars, t.offsets, t.prior_type)
        if t.gp:
            self.i32(t.gp_gather.reshape(-1), t.gp_ecl.reshape(-1))
        self.f64(consts, t.x, t.y, t.ye, t.w, t.prior_p1, t.prior_p2, t.prior_norm)
        if t.gp:
            self.f64(t.gp_base.reshape(-1))
        self.f64(walkers)
        self.shapes.append([("f8", (W,))])

    def predict(self, x, ye, obs, res, hyp, blocks, has_var):
        W, n = res.shape
        self.head(3)
        self.ints(W, n, blocks.shape[1], int(has_var))
        self.i32(obs)
        self.f64(x, ye, res, hyp, blocks)
        self.shapes.append([("f8", (W, n))] + ([("f8", (W, n))] if has_var else []) + [("i4", (W,))])

    def write(self, path):
        with open(path, "wb") as fh:
            fh.write(np.asarray([len(self.shapes)], dtype=np.int32).tobytes())
            fh.write(b"".join(self.blob))

    def read(self, path):
        """[(rc, [arrays])] per case"""
        data = open(path, "rb").read()
        pos, out = 0, []
        for shapes in self.shapes:
            rc = int(np.frombuffer(data, np.int32, 1, pos)[0])
            pos += 4
            arrs = []
            for dt, shape in shapes:
                n = int(np.prod(shape))
                arrs.append(np.frombuffer(data, dt, n, pos).reshape(shape).copy())
                pos += n * int(dt[1])
            out.append((rc, arrs))
        assert pos == len(data)
        return out


def run(exe, cases, tmp_path, tag, swap):
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / ("results_%s.bin" % tag))
    if not os.path.exists(src):
        cases.write(src)
    t0 = time.time()
    r = subprocess.run([exe, src, dst] + (["swap"] if swap else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return cases.read(dst), time.time() - t0


# ------------------------------------------------------------------ flux and lnlike
def windows(kind, N):
    rng = np.random.default_rng(17 + N)
    if N == 1:
        x, w = np.array([0.013]), np.array([1e-3])
    elif kind == "descending":        # a descending file: w = mean(diff(x))/2 < 0
        x = np.linspace(0.3, -0.3, N)
        w = np.mean(np.diff(x)) * np.ones(N) / 2.0
    elif kind == "wrap":              # phases run past 0.5
        x = np.linspace(0.45, 1.1, N)
        w = np.mean(np.diff(x)) * np.ones(N) / 2.0
    elif kind == "ragged":            # sorted centres, ragged widths
        x = np.sort(rng.uniform(-0.25, 0.25, N))
        w = rng.uniform(1e-4, 4e-3, N)
    else:
        x = np.linspace(-0.3, 0.3, N)
        w = np.mean(np.diff(x)) * np.ones(N) / 2.0
    if kind == "shuffled":
        p = rng.permutation(N)
        x, w = x[p], w[p]
    if kind == "nan_width":
        w = w.copy()
        w[N // 2] = np.nan
    if kind == "zero":
        w = np.zeros(N)
    if kind == "tiny":
        w = np.full(N, 1e-300)
    if kind == "null_w":
        w = None
    return x, w


def flux_bound(w, nsub):
    """the module docstring's bound, in units of the flux scale"""
    h = np.nanmin(w) if w is not None and np.isfinite(w).any() else 0.0
    if not h > 1e-6:                  # no width (zero, 1e-300, negative): point evaluation
        return FLUX_RTOL
    return min(FLUX_RTOL, PHASE_ATOL / (2.0 * h / nsub))


def population():
    edges = [np.asarray(e[1], dtype=float) for e in dc.status_edges()]
    return np.concatenate([dc.wide_box(48), dc.prior_box(48), np.array(dc.DISPUTED), np.array(edges)])


def configurations():
    out = []
    for P in (18, 14):
        for nsub in (1, 3):
            for N in (1, 65, 512, 513):
                for kind in KINDS:
                    if (N == 512 and kind != "regular") or (N == 1 and kind in NEEDS_TWO):
                        continue
                    out.append((P, nsub, N, kind))
    return out


def flux_cases(cases, oracle):
    """adds a flux and an lnlike case per configuration; returns what to compare them with"""
    pop = population()
    confs = configurations()
    assert len(pop) >= 120 and len(confs) == 96
    jobs, want = [], []
    k = 0
    for P, nsub, N, kind in confs:
        sets = pop[(k + np.arange(SETS_PER_CONFIG)) % len(pop)]
        k += SETS_PER_CONFIG
        pars = np.ascontiguousarray(sets if P == 18 else dc.simple(sets))
        x, w = windows(kind, N)
        jobs.append((pars, x, w, nsub))
        want.append(dict(conf=(P, nsub, N, kind), pars=pars, x=x, w=w, nsub=nsub))
    assert k >= 6 * len(pop)              # every set serves in at least six configurations

    def reference(job):
        pars, x, w, nsub = job
        return [oracle.flux(p, x, np.zeros_like(x) if w is None else w, nsub=nsub) for p in pars]
    with ThreadPoolExecutor(8) as pool:   # (the oracle's calls release the interpreter lock)
        refs = list(pool.map(reference, jobs))
    rng = np.random.default_rng(4)
    for d, ref in zip(want, refs):
        d["status"] = np.array([st for st, _ in ref], dtype=np.int32)
        d["flux"] = np.array([f for _, f in ref])
        ok = [f for st, f in ref if st == 0 and np.all(np.isfinite(f))]
        d["y"] = (ok[0] if ok else np.full(d["x"].size, 0.05)) + YE * rng.standard_normal(d["x"].size)
        d["ye"] = np.full(d["x"].size, YE)
        d["first"] = len(cases.shapes)
        cases.flux(d["pars"], d["x"], d["w"], d["nsub"])
        cases.flux(d["pars"], d["x"], d["w"], d["nsub"], d["y"], d["ye"])
    return want


def check_flux(want, results, label):
    worst = 0.0
    n_ok = 0
    for d in want:
        (rc_f, (flux, st_f)), (rc_l, (ll, st_l)) = results[d["first"]], results[d["first"] + 1]
        tag = (label,) + d["conf"]
        assert rc_f == 0 and rc_l == 0, tag
        assert np.array_equal(st_f, d["status"]) and np.array_equal(st_l, d["status"]), (tag, st_f, d["status"])
        assert np.array_equal(np.isfinite(flux), np.isfinite(d["flux"])), tag
        B = flux_bound(d["w"], d["nsub"])
        for i in np.flatnonzero(d["status"] == 0):
            of = d["flux"][i]
            fin = np.isfinite(of)
            n_ok += 1
            if not fin.any():
                assert np.isneginf(ll[i]), tag
                continue
            scale = np.max(np.abs(of[fin]))
            err = np.max(np.abs(flux[i][fin] - of[fin])) / scale
            worst = max(worst, err / B)
            assert err <= B, (tag, i, err, B)
            if not fin.all():             # a NaN flux: chi^2 = +inf (CVModel.py:163-171)
                assert np.isneginf(ll[i]), tag
                continue
            r = (d["y"] - of) / d["ye"]
            room = np.sum(np.abs(r)) * B * scale / YE + 0.5 * of.size * (B * scale / YE) ** 2
            ref = -0.5 * np.sum(r * r)
            assert abs(ll[i] - ref) <= room + 1e-12 * abs(ref), (tag, i, ll[i], ref, room)
        bad = d["status"] != 0
        assert np.all(np.isnan(flux[bad])) and np.all(np.isneginf(ll[bad])), tag
    assert n_ok >= 0.5 * len(want) * SETS_PER_CONFIG
    return worst


# ------------------------------------------------------------------ trees and the GP posterior
def tree_cases(cases, oracle):
    from lfit_python_amd import batch, synthetic

    def flux_fn(p, x, w, nsub):
        st, f = oracle.flux(p, x, w, nsub=nsub)
        assert st == 0
        return f
    m = synthetic.config_single(32, flux_fn=flux_fn)
    base, p0 = batch.compile_tree(m), np.array(m.dynasty_par_vals)
    want = []

    def add(name, t, walk, rtol, atol):
        ref, _, _ = oracle.lnprob_batch(walk, t, nsub=t.nsub)
        want.append(dict(name=name, ref=ref, rtol=rtol, atol=atol, at=len(cases.shapes)))
        cases.lnprob(t, walk)
    for case in pd.CHUNK_IDS:             # every prior type at its edges, around the lanes' chunks of 16
        types, p1, p2, walk = pd.chunk_case(case)
        add("chunk " + case, pd.table_tree(base, p0, types, p1, p2), walk, 1e-10, 1e-8)
    wide = pd.widen(base)
    _, walk = pd.roche_limit_walkers(oracle, wide, p0)
    assert wide.roche_priors
    add("roche limits", wide, walk, 1e-10, 1e-8)
    for name in ("tiny", "cuts"):
        gm, nsub, walk = gp_trees.case(oracle, name)
        add("gp " + name, batch.compile_tree(gm, nsub=nsub), walk, 1e-9, 1e-8)
    return want


def check_trees(want, results, label):
    for d in want:
        rc, (lnp,) = results[d["at"]]
        assert rc == 0, (label, d["name"])
        ref = d["ref"]
        assert np.array_equal(np.isfinite(lnp), np.isfinite(ref)), (label, d["name"], np.flatnonzero(
            np.isfinite(lnp) != np.isfinite(ref)))
        assert np.all(np.isneginf(lnp[~np.isfinite(ref)])), (label, d["name"])
        fin = np.isfinite(ref)
        assert fin.sum() >= 2
        np.testing.assert_allclose(lnp[fin], ref[fin], rtol=d["rtol"], atol=d["atol"], err_msg="%s %s" % (label, d["name"]))


def predict_cases(cases):
    W, N, nb = 3, 65, 2
    made = [gs.make_case(77 + 1000 * k, N, nb) for k in range(W)]
    x, ye, t = made[0][0], made[0][1], made[0][5]
    res, hyp, blocks = (np.stack([c[k] for c in made]) for k in (2, 3, 4))
    n = N + t.size
    z = np.concatenate([x, t])
    order = np.argsort(z, kind="stable")
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    rm, yem = np.zeros((W, n)), np.zeros(n)
    rm[:, inv[:N]] = res
    yem[inv[:N]] = ye
    at = len(cases.shapes)
    for has_var in (True, False):
        cases.predict(z[order], yem, (order < N).astype(np.int32), rm, hyp, blocks, has_var)
    return dict(at=at, it=inv[N:], raw=(x, ye, res, hyp, blocks, t))


def check_predict(want, results, label):
    x, ye, res, hyp, blocks, t = want["raw"]
    (rc1, (mean, var, st1)), (rc2, (mean2, st2)) = results[want["at"]], results[want["at"] + 1]
    assert rc1 == 0 and rc2 == 0 and not st1.any() and not st2.any(), label
    for k in range(res.shape[0]):
        gs.check(mean[k][want["it"]], var[k][want["it"]], x, ye, res[k], hyp[k], blocks[k], t)
        gs.check(mean2[k][want["it"]], None, x, ye, res[k], hyp[k], blocks[k], t)


# ------------------------------------------------------------------ the test
def test_host_twins_plain_and_under_sanitizers(oracle, tmp_path):
    cases = Cases()
    flux_want = flux_cases(cases, oracle)
    tree_want = tree_cases(cases, oracle)
    pred_want = predict_cases(cases)
    out = {}
    for tag, flags, swap in (("O2", ["-O2"], True), ("sanitized", SAN, False)):
        exe, t_build = build(tmp_path, tag, flags)
        out[tag], t_run = run(exe, cases, tmp_path, tag, swap)
        worst = check_flux(flux_want, out[tag], tag)
        check_trees(tree_want, out[tag], tag)
        check_predict(pred_want, out[tag], tag)
        print("%s: built in %.1f s, %d cases run in %.1f s; worst flux difference %.2f of its bound"
              % (tag, t_build, len(cases.shapes), t_run, worst))
    # the two builds (and the two thread counts) against each other, within the same bounds
    for d in flux_want:
        B = flux_bound(d["w"], d["nsub"])
        for at in (d["first"], d["first"] + 1):
            (_, (a, sa)), (_, (b, sb)) = out["O2"][at], out["sanitized"][at]
            assert np.array_equal(sa, sb) and np.array_equal(np.isfinite(a), np.isfinite(b)), d["conf"]
        fa, fb = out["O2"][d["first"]][1][0], out["sanitized"][d["first"]][1][0]
        for i in np.flatnonzero(d["status"] == 0):
            fin = np.isfinite(fa[i])
            if fin.any():
                assert np.max(np.abs(fa[i][fin] - fb[i][fin])) <= B * np.max(np.abs(d["flux"][i][fin])), d["conf"]
    for d in tree_want:
        a, b = out["O2"][d["at"]][1][0], out["sanitized"][d["at"]][1][0]
        fin = np.isfinite(a)
        assert np.array_equal(fin, np.isfinite(b))
        np.testing.assert_allclose(a[fin], b[fin], rtol=d["rtol"], atol=d["atol"])
    for k in (0, 1):
        a, b = out["O2"][pred_want["at"] + k][1][0], out["sanitized"][pred_want["at"] + k][1][0]
        scale = np.sqrt(pred_want["raw"][3][:, 0] + pred_want["raw"][3][:, 1])[:, None]
        assert np.max(np.abs(a - b) / scale) <= gs.BAR
