"""The GPU path's algorithm on CPU cores (cpu_baseline/lfg_cpu.cpp): a fair
CPU baseline for bench.py, beside the oracle.  Not a product path: nothing
in lfit_python_amd loads it.

    build(out=None, march="x86-64-v3", extra=()) -> path of liblfg_cpu.so
    CpuPort(path).lnprob_batch(walkers, tree, nthreads=0) -> (lnp, threads)
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(HERE, "liblfg_cpu.so")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


def build(out=None, march="x86-64-v3", extra=()):
    """extra: further compiler flags (diagnostic builds: -DLFC_COUNT, -DLFG_F32_OPEN=0)"""
    out = out or LIB_PATH
    cmd = ["g++", "-O3", "-march=%s" % march, "-fopenmp", "-std=c++17", "-fPIC", "-shared"] + list(extra) + [
           "-I", HERE, "-I", os.path.join(HERE, "shim"), "-I", os.path.join(ROOT, "lfit_python_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), "-o", out, os.path.join(HERE, "lfg_cpu.cpp"),
           os.path.join(HERE, "lfg_cpu_physpar.cpp"), os.path.join(HERE, "lfg_cpu_wd.cpp"),
           os.path.join(HERE, "lfg_cpu_chain.cpp"), os.path.join(HERE, "lfg_cpu_limbdark.cpp"),
           os.path.join(HERE, "lfg_cpu_corner.cpp"), os.path.join(HERE, "lfg_cpu_chaintext.cpp"),
           os.path.join(HERE, "lfg_cpu_chainparse.cpp")]
    subprocess.run(cmd, check=True)
    return out


class CpuPort:
    def __init__(self, path=None):
        self.lib = ctypes.CDLL(path or LIB_PATH)
        f = self.lib.lfc_lnprob_batch
        f.restype = ctypes.c_int
        f.argtypes = [_dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _ip, _ip, _dp, _ip, _dp, _dp, _dp, _dp,
                      ctypes.c_int, _ip, _dp, _dp, _dp, ctypes.c_int, _dp, ctypes.c_int]
        for name in ("lfg_cpu_flux", "lfg_cpu_lnlike", "lfg_cpu_lnprob"):
            getattr(self.lib, name).restype = ctypes.c_int
        self.lib.lfg_cpu_flux.argtypes = [_dp, ctypes.c_int, ctypes.c_int, _dp, _dp, ctypes.c_int, ctypes.c_int,
                                          _dp, _ip, ctypes.c_int]
        self.lib.lfg_cpu_lnlike.argtypes = [_dp, ctypes.c_int, ctypes.c_int, _dp, _dp, ctypes.c_int, ctypes.c_int,
                                            _dp, _dp, _dp, _ip, ctypes.c_int]
        g = self.lib.lfc_lnprob_batch_gp
        g.restype = ctypes.c_int
        g.argtypes = [_dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _ip, _ip, _dp, _ip, _dp, _dp, _dp, _dp,
                      ctypes.c_int, _ip, _dp, _dp, _dp, ctypes.c_int, _ip, _dp, _ip, _dp, ctypes.c_int]

    def lnprob_batch(self, walkers, tree, nthreads=0):
        """ln_prob of walkers [W, ndim] of a compiled tree
        (lfit_python_amd.batch.CompiledTree), chi^2 or GP."""
        keep = []

        def F(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            keep.append(a)
            return a.ctypes.data_as(_dp)

        def I(a):
            a = np.ascontiguousarray(a, dtype=np.int32)
            keep.append(a)
            return a.ctypes.data_as(_ip)
        w = np.ascontiguousarray(walkers, dtype=np.float64)
        W, ndim = w.shape
        lnp = np.empty(W)
        gp = bool(getattr(tree, "gp", False))
        used = self.lib.lfc_lnprob_batch_gp(
            F(w), W, ndim, tree.E, I(tree.gather.reshape(-1)), I(tree.npars),
            F(tree.consts if len(tree.consts) else np.zeros(1)), I(tree.offsets), F(tree.x), F(tree.y), F(tree.ye),
            F(tree.w), int(tree.nsub), I(tree.prior_type), F(tree.prior_p1), F(tree.prior_p2), F(tree.prior_norm),
            int(tree.roche_priors), I(tree.gp_gather.reshape(-1)) if gp else None,
            F(tree.gp_base.reshape(-1)) if gp else None, I(tree.gp_ecl.reshape(-1)) if gp else None,
            lnp.ctypes.data_as(_dp), int(nthreads))
        if getattr(tree, "fixed_invalid", False):
            lnp[:] = -np.inf
        return lnp, used

    def gp_dcp(self, q, dphi, rwd):
        """the port's dist_cp of (q, dphi, rwd) (MODEL_SPEC 10.3), NaN on failure"""
        f = self.lib.lfc_gp_dcp
        f.restype = ctypes.c_double
        f.argtypes = [ctypes.c_double] * 3
        return f(float(q), float(dphi), float(rwd))

    # ---- the lfg_cpu_* twins (cpu_baseline/lfg_cpu.h) of lfg_flux,
    # lfg_lnlike and lfg_lnprob: host arrays, the same argument meaning
    def flux(self, pars, x, w, nsub=1, nthreads=0):
        """lfg_cpu_flux: (flux [W, N], status [W])"""
        pars = np.ascontiguousarray(np.atleast_2d(pars), dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64)
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        W, P = pars.shape
        flux = np.empty((W, x.size))
        st = np.empty(W, dtype=np.int32)
        rc = self.lib.lfg_cpu_flux(pars.ctypes.data_as(_dp), W, P, x.ctypes.data_as(_dp),
                                   None if w is None else w.ctypes.data_as(_dp), x.size, int(nsub),
                                   flux.ctypes.data_as(_dp), st.ctypes.data_as(_ip), int(nthreads))
        if rc != 0:
            raise ValueError("lfg_cpu_flux: code %d" % rc)
        return flux, st

    def lnlike(self, pars, x, w, y, ye, nsub=1, nthreads=0):
        """lfg_cpu_lnlike: (ln_like [W], status [W])"""
        pars = np.ascontiguousarray(np.atleast_2d(pars), dtype=np.float64)
        arr = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, ye)]
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        W, P = pars.shape
        out = np.empty(W)
        st = np.empty(W, dtype=np.int32)
        rc = self.lib.lfg_cpu_lnlike(pars.ctypes.data_as(_dp), W, P, arr[0].ctypes.data_as(_dp),
                                     None if w is None else w.ctypes.data_as(_dp), arr[0].size, int(nsub),
                                     arr[1].ctypes.data_as(_dp), arr[2].ctypes.data_as(_dp), out.ctypes.data_as(_dp),
                                     st.ctypes.data_as(_ip), int(nthreads))
        if rc != 0:
            raise ValueError("lfg_cpu_lnlike: code %d" % rc)
        return out, st

    def gp_predict(self, x, ye, obs, res, hyp, blocks, return_var=True, nthreads=0):
        """lfg_cpu_gp_predict over a sorted merged grid: (mean [W, n],
        var [W, n] or None, status [W])"""
        x, ye = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (x, ye))
        obs = np.ascontiguousarray(obs, dtype=np.int32).reshape(-1)
        res = np.ascontiguousarray(np.atleast_2d(res), dtype=np.float64)
        W, n = res.shape
        hyp = np.ascontiguousarray(hyp, dtype=np.float64).reshape(W, 3)
        blocks = np.ascontiguousarray(blocks, dtype=np.float64).reshape(W, -1, 2)
        nb = blocks.shape[1]
        mean = np.empty((W, n))
        var = np.empty((W, n)) if return_var else None
        st = np.empty(W, dtype=np.int32)
        f = self.lib.lfg_cpu_gp_predict
        f.restype = ctypes.c_int
        f.argtypes = [_dp, _dp, _ip, _dp, ctypes.c_int, ctypes.c_int, _dp, _dp, ctypes.c_int, _dp, _dp, _ip,
                      ctypes.c_int]
        rc = f(x.ctypes.data_as(_dp), ye.ctypes.data_as(_dp), obs.ctypes.data_as(_ip), res.ctypes.data_as(_dp), W, n,
               hyp.ctypes.data_as(_dp), blocks.ctypes.data_as(_dp) if nb else None, nb, mean.ctypes.data_as(_dp),
               var.ctypes.data_as(_dp) if return_var else None, st.ctypes.data_as(_ip), int(nthreads))
        if rc != 0:
            raise ValueError("lfg_cpu_gp_predict: code %d" % rc)
        return mean, var, st

    def physpar(self, q, dphi, rwd, twd, p, tables, ld=1, n=None, nthreads=0):
        """lfg_cpu_physpar: (table [n, 10], model [n], status [n]).  tables:
        a lfit_python_amd.physpar.MRTables; q, dphi and rwd are read at
        element i * ld (n rows; default: their length with ld = 1)."""
        from lfit_python_amd import _native
        q, dphi, rwd, twd, p = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (q, dphi, rwd, twd, p))
        n = twd.size if n is None else int(n)
        assert p.size >= n and twd.size >= n and all(a.size == 0 or a.size > (n - 1) * ld for a in (q, dphi, rwd))
        out = np.empty((10, n))
        model = np.empty(n, dtype=np.int32)
        st = np.empty(n, dtype=np.int32)
        f = self.lib.lfg_cpu_physpar
        f.restype = ctypes.c_int
        f.argtypes = [_dp, _dp, _dp, ctypes.c_size_t, _dp, _dp, ctypes.c_int, ctypes.POINTER(_native.LfgMrTables),
                      _dp, _ip, _ip, ctypes.c_int]
        T = tables.host_struct()
        rc = f(q.ctypes.data_as(_dp), dphi.ctypes.data_as(_dp), rwd.ctypes.data_as(_dp), int(ld),
               twd.ctypes.data_as(_dp), p.ctypes.data_as(_dp), n, ctypes.byref(T), out.ctypes.data_as(_dp),
               model.ctypes.data_as(_ip), st.ctypes.data_as(_ip), int(nthreads))
        if rc != 0:
            raise ValueError("lfg_cpu_physpar: code %d" % rc)
        return np.ascontiguousarray(out.T), model, st

    def limbdark(self, logg, teff, tables, ld=1, n=None, nthreads=0):
        """lfg_cpu_limbdark: (table [n, 25], status [n]).  tables: a
        lfit_python_amd.limbdark.LDTables; logg and teff are read at element
        i * ld (n rows; default: their length with ld = 1)."""
        from lfit_python_amd import _native
        logg, teff = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (logg, teff))
        n = teff.size if n is None else int(n)
        assert all(n == 0 or a.size > (n - 1) * ld for a in (logg, teff))
        out = np.empty((n, 25))
        st = np.empty(n, dtype=np.int32)
        f = self.lib.lfg_cpu_limbdark
        f.restype = ctypes.c_int
        f.argtypes = [_dp, _dp, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(_native.LfgLdTables), _dp, _ip,
                      ctypes.c_int]
        T = tables.host_struct()
        rc = f(logg.ctypes.data_as(_dp), teff.ctypes.data_as(_dp), int(ld), n, ctypes.byref(T),
               out.ctypes.data_as(_dp), st.ctypes.data_as(_ip), int(nthreads))
        if rc != 0:
            raise ValueError("lfg_cpu_limbdark: code %d" % rc)
        return out, st

    def wd_lnprob(self, theta, model, ld=None, n=None, nthreads=0):
        """lfg_cpu_wd_lnprob: (lnp [n], lnlike [n], mags [n, B], status [n]).
        model: a lfit_python_amd.wdparams.WDModel; theta [n, ld], or flat with
        row i at element i * ld."""
        from lfit_python_amd import _native
        th = np.ascontiguousarray(theta, dtype=np.float64)
        if ld is None:
            n, ld = th.shape
        th = th.reshape(-1)
        n = int(n)
        assert n == 0 or th.size >= (n - 1) * ld + 4
        lnp, ll, st = np.empty(n), np.empty(n), np.empty(n, dtype=np.int32)
        mags = np.empty((model.B, n))
        f = self.lib.lfg_cpu_wd_lnprob
        f.restype = ctypes.c_int
        f.argtypes = [_dp, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(_native.LfgWdModel), _dp, _dp, _dp, _ip,
                      ctypes.c_int]
        M = model.host_struct()
        rc = f(th.ctypes.data_as(_dp), int(ld), n, ctypes.byref(M), lnp.ctypes.data_as(_dp), ll.ctypes.data_as(_dp),
               mags.ctypes.data_as(_dp), st.ctypes.data_as(_ip), int(nthreads))
        if rc != 0:
            raise ValueError("lfg_cpu_wd_lnprob: code %d" % rc)
        return lnp, ll, np.ascontiguousarray(mags.T), st

    def chain_stats(self, buf, steps, W, C, step_ld, walker_ld, offset=0, window=None, fracs=(), rhat=False):
        """lfg_cpu_chain_stats on the view (include/lfg_chain.h) of the flat
        float64 array `buf` that starts at element `offset`: a dict of n,
        n_bad, mean, m2, min, max, ostat [C, nq, 2], quant [C, nq] and rhat."""
        buf = np.ascontiguousarray(buf, dtype=np.float64).reshape(-1)
        steps, W, C = int(steps), int(W), int(C)
        if steps > 0 and W > 0:
            assert offset + (steps - 1) * step_ld + (W - 1) * walker_ld + C <= buf.size
        fr = np.ascontiguousarray(fracs, dtype=np.float64).reshape(-1)
        nq = fr.size
        win = None if window is None else np.ascontiguousarray(window, dtype=np.float64).reshape(C, 2)
        out = {"n": np.empty(C, np.int64), "n_bad": np.empty(C, np.int64)}
        for k in ("mean", "m2", "min", "max"):
            out[k] = np.empty(C)
        out["ostat"], out["quant"] = np.empty((C, nq, 2)), np.empty((C, nq))
        out["rhat"] = np.empty(C) if rhat else None
        f = self.lib.lfg_cpu_chain_stats
        f.restype = ctypes.c_int
        vp, i64 = ctypes.c_void_p, ctypes.c_longlong
        f.argtypes = [vp, i64, i64, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int] + [vp] * 9

        def P(a):
            return None if a is None else ctypes.c_void_p(a.ctypes.data)
        rc = f(ctypes.c_void_p(buf.ctypes.data + 8 * int(offset)), steps, W, C, int(step_ld), int(walker_ld), P(win),
               P(fr) if nq else None, nq, P(out["n"]), P(out["n_bad"]), P(out["mean"]), P(out["m2"]), P(out["min"]),
               P(out["max"]), P(out["ostat"]), P(out["quant"]), P(out["rhat"]))
        if rc != 0:
            raise ValueError("lfg_cpu_chain_stats: code %d" % rc)
        return out

    def chain_clip(self, n, m2, med, sigma, window=None):
        """lfg_cpu_chain_clip: the next window [C, 2]"""
        n = np.ascontiguousarray(n, dtype=np.int64)
        m2, med = (np.ascontiguousarray(a, dtype=np.float64) for a in (m2, med))
        C = n.size
        win = None if window is None else np.ascontiguousarray(window, dtype=np.float64).reshape(C, 2)
        out = np.empty((C, 2))
        f = self.lib.lfg_cpu_chain_clip
        f.restype = ctypes.c_int
        vp = ctypes.c_void_p
        f.argtypes = [vp, vp, vp, ctypes.c_longlong, ctypes.c_double, vp, vp, ctypes.c_int]
        rc = f(n.ctypes.data, m2.ctypes.data, med.ctypes.data, 1, float(sigma),
               None if win is None else win.ctypes.data, out.ctypes.data, C)
        if rc != 0:
            raise ValueError("lfg_cpu_chain_clip: code %d" % rc)
        return out

    def corner_hist(self, buf, steps, W, row_len, step_ld, walker_ld, cols, ranges, nb, offset=0):
        """lfg_cpu_corner_hist on the view (include/lfg_corner.h) of the flat
        float64 array `buf` that starts at element `offset`: a dict of h1
        [K, nb], h2 [P, nb, nb] (int64) and flag [K]."""
        buf = np.ascontiguousarray(buf, dtype=np.float64).reshape(-1)
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        K, nb = int(cols.size), int(nb)
        rng = np.ascontiguousarray(ranges, dtype=np.float64).reshape(-1, 2)
        assert rng.shape[0] == K
        if steps > 0 and W > 0 and K and 0 <= cols.min() and cols.max() < row_len:
            assert offset + (steps - 1) * step_ld + (W - 1) * walker_ld + cols.max() < buf.size
        P = max(K * (K - 1) // 2, 0)
        m = max(nb, 1)   # (the outputs of a refused nb only have to exist)
        out = {"h1": np.full((K, m), -1, np.int64), "h2": np.full((P, m, m), -1, np.int64),
               "flag": np.full(K, -1, np.int32)}
        f = self.lib.lfg_cpu_corner_hist
        f.restype = ctypes.c_int
        vp, i64, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
        f.argtypes = [vp, i64, i64, ci, i64, i64, vp, ci, vp, ci, vp, vp, vp]
        rc = f(ctypes.c_void_p(buf.ctypes.data + 8 * int(offset)), int(steps), int(W), int(row_len), int(step_ld),
               int(walker_ld), cols.ctypes.data, K, rng.ctypes.data, nb, out["h1"].ctypes.data,
               out["h2"].ctypes.data if K > 1 else None, out["flag"].ctypes.data)
        if rc != 0:
            raise ValueError("lfg_cpu_corner_hist: code %d" % rc)
        return out

    def corner_levels(self, h2, fracs):
        """lfg_cpu_corner_levels: level [P, nl] (int64) of h2 [P, nb, nb]"""
        h2 = np.ascontiguousarray(h2, dtype=np.int64)
        P, nb = h2.shape[0], h2.shape[1]
        fr = np.ascontiguousarray(fracs, dtype=np.float64).reshape(-1)
        out = np.full((P, fr.size), -1, np.int64)
        f = self.lib.lfg_cpu_corner_levels
        f.restype = ctypes.c_int
        vp, ci = ctypes.c_void_p, ctypes.c_int
        f.argtypes = [vp, ci, ci, vp, ci, vp]
        keep = np.zeros(1, np.int64)   # (a valid pointer for P = 0)
        rc = f(h2.ctypes.data if h2.size else keep.ctypes.data, P, nb, fr.ctypes.data, fr.size,
               out.ctypes.data if out.size else keep.ctypes.data)
        if rc != 0:
            raise ValueError("lfg_cpu_corner_levels: code %d" % rc)
        return out

    def chain_text(self, buf, steps, W, ndim, step_ld, walker_ld, lnp, lnp_step_ld, lnp_walker_ld, walker0=0,
                   offset=0, lnp_offset=0, nthreads=0):
        """lfg_cpu_chain_text on the views (include/lfg_chaintext.h) of the
        flat float64 arrays `buf` and `lnp` that start at elements `offset`
        and `lnp_offset`: the rows' bytes"""
        buf = np.ascontiguousarray(buf, dtype=np.float64).reshape(-1)
        lnp = np.ascontiguousarray(lnp, dtype=np.float64).reshape(-1)
        steps, W, ndim = int(steps), int(W), int(ndim)
        vp, i64, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
        b = self.lib.lfg_cpu_chain_text_bound
        b.restype = i64
        b.argtypes = [i64, i64, ci, i64]
        bound = b(steps, W, ndim, int(walker0))
        if bound < 0:
            raise ValueError("lfg_cpu_chain_text: refused shape")
        if steps > 0 and W > 0:
            assert offset + (steps - 1) * step_ld + (W - 1) * walker_ld + ndim <= buf.size
            assert lnp_offset + (steps - 1) * lnp_step_ld + (W - 1) * lnp_walker_ld < lnp.size
            # the bound leaves out '%f' of 2^63 and beyond (at most 317 characters)
            with np.errstate(invalid="ignore"):
                big = np.isfinite(lnp) & (np.abs(lnp) >= 2.0 ** 63)
            bound += 320 * int(big.sum())
        out = np.empty(max(bound, 1), dtype=np.uint8)
        nb = np.zeros(2, dtype=np.int64)
        f = self.lib.lfg_cpu_chain_text
        f.restype = ci
        f.argtypes = [vp, i64, i64, ci, i64, i64, vp, i64, i64, i64, vp, ctypes.c_size_t, vp, ci]
        rc = f(ctypes.c_void_p(buf.ctypes.data + 8 * int(offset)), steps, W, ndim, int(step_ld), int(walker_ld),
               ctypes.c_void_p(lnp.ctypes.data + 8 * int(lnp_offset)), int(lnp_step_ld), int(lnp_walker_ld),
               int(walker0), out.ctypes.data, bound, nb.ctypes.data, int(nthreads))
        if rc != 0:
            raise ValueError("lfg_cpu_chain_text: code %d" % rc)
        return out[:int(nb[0])].tobytes()

    def lnprob(self, walkers, tree, nthreads=0):
        """lfg_cpu_lnprob through a struct lfg_tree of host arrays"""
        from lfit_python_amd import _native
        keep = []

        def F(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            keep.append(a)
            return ctypes.c_void_p(a.ctypes.data)

        def I(a):
            a = np.ascontiguousarray(a, dtype=np.int32)
            keep.append(a)
            return ctypes.c_void_p(a.ctypes.data)
        gp = bool(tree.gp)
        T = _native.LfgTree(tree.E, tree.ndim, tree.nsub, tree.max_n, I(tree.gather.reshape(-1)), I(tree.npars),
                            F(tree.consts if len(tree.consts) else np.zeros(1)), I(tree.offsets), F(tree.x),
                            F(tree.y), F(tree.ye), F(tree.w), I(tree.prior_type), F(tree.prior_p1), F(tree.prior_p2),
                            F(tree.prior_norm), int(tree.roche_priors), int(gp),
                            I(tree.gp_gather.reshape(-1)) if gp else None, F(tree.gp_base.reshape(-1)) if gp else None,
                            I(tree.gp_ecl.reshape(-1)) if gp else None, int(tree.fixed_invalid), None)
        w = np.ascontiguousarray(walkers, dtype=np.float64)
        lnp = np.empty(w.shape[0])
        self.lib.lfg_cpu_lnprob.argtypes = [_dp, ctypes.c_int, ctypes.POINTER(_native.LfgTree), _dp, ctypes.c_int]
        rc = self.lib.lfg_cpu_lnprob(w.ctypes.data_as(_dp), w.shape[0], ctypes.byref(T), lnp.ctypes.data_as(_dp),
                                     int(nthreads))
        if rc != 0:
            raise ValueError("lfg_cpu_lnprob: code %d" % rc)
        return lnp
