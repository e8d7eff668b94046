"""A chain's summary on the device (include/lfg_chain.h, MODEL_SPEC.md
section 14): what the reference does to a finished chain on the host with
pandas, numpy and astropy.

    stats(chain, ...)                per column n, mean, m2, min, max, exact
                                     quantiles and R-hat, read in place
    gr_diagnostic(chain)             mcmc_utils.GR_diagnostic
    sigma_clipped_stats(chain, ...)  astropy's (mean, median, std) per column
    wd_fluxes(chain, names, ...)     wdparams.fluxes_from_chain
    fit_summary(chain, names, ...)   plot_lc_model.fit_summary's numbers:
                                     modparams.csv and the two report blocks

A chain is the sampler's chain_dev [steps][W][ndim] (a torch tensor on the
device, summarised where it lies), a walker-major array [W][steps][ndim]
(mcmc_utils.readchain's; walker_major=True) or a flat chain [rows][ndim].  A
host array is moved to the device once, as it is; nothing is transposed,
gathered or sorted.  `cols` picks a contiguous run of columns (None: all, an
int: the first so many, a slice); nskip and thin drop leading steps and keep
every thin-th, as a view.
"""
import ctypes
import os

import numpy as np

from . import _native

DEFAULT_QUANTILES = (0.16, 0.5, 0.84)


class ChainStats:
    """Host numpy arrays per column: n, n_bad (int64), mean, m2 (sum of squared
    deviations), min, max, quant [C, nq], ostat [C, nq, 2], rhat (or None);
    quantiles: the fractions.  var() / std() divide m2 by n - ddof."""

    def __init__(self, quantiles, **arrays):
        self.quantiles = tuple(float(q) for q in quantiles)
        for k, v in arrays.items():
            setattr(self, k, v)

    def var(self, ddof=0):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.n - ddof > 0, self.m2 / (self.n - ddof), np.nan)

    def std(self, ddof=0):
        return np.sqrt(self.var(ddof))

    def quantile(self, q):
        return self.quant[:, self.quantiles.index(float(q))]


class _View:
    """The C ABI's view of a device tensor (kept alive here)."""

    def __init__(self, chain, cols=None, walker_major=False, nskip=0, thin=1, device=None):
        import torch
        _native.require_gpu()
        if not isinstance(chain, torch.Tensor):
            a = np.asarray(chain, dtype=np.float64)
            chain = torch.from_numpy(a if a.flags.writeable else a.copy())
        if chain.dtype != torch.float64:
            raise TypeError("a chain is float64, not %s" % chain.dtype)
        if chain.dim() not in (2, 3):
            raise ValueError("a chain is [steps][W][ndim], [W][steps][ndim] or [rows][ndim], not %s" %
                             (tuple(chain.shape),))
        if not chain.is_cuda:
            chain = chain.to(torch.device(device) if device is not None else
                             torch.device("cuda", torch.cuda.current_device()))
        if int(thin) < 1 or int(nskip) < 0:
            raise ValueError("nskip >= 0 and thin >= 1")
        t = chain
        if t.dim() == 2:
            t = t.unsqueeze(1)                      # [rows][1][ndim]
        elif walker_major:
            t = t.permute(1, 0, 2)                  # a view: [steps][W][ndim]
        t = t[int(nskip)::int(thin)]
        ndim = t.shape[2]
        if cols is None:
            c0, c1 = 0, ndim
        elif isinstance(cols, slice):
            c0, c1, step = cols.indices(ndim)
            if step != 1:
                raise ValueError("cols must be a contiguous run of columns")
        else:
            c0, c1 = 0, int(cols)
        if not 0 <= c0 < c1 <= ndim:
            raise ValueError("columns %d:%d of a chain with %d" % (c0, c1, ndim))
        if ndim > 1 and t.stride(2) != 1:
            raise ValueError("a chain's columns must be contiguous in memory")
        self.tensor = t
        self.device = t.device
        self.steps, self.W, self.C = int(t.shape[0]), int(t.shape[1]), c1 - c0
        self.step_ld = int(t.stride(0)) if self.steps > 1 else 1
        self.walker_ld = int(t.stride(1)) if self.W > 1 else 1
        if self.step_ld < 1 or self.walker_ld < 1:
            raise ValueError("a chain with a zero stride (an expanded tensor) cannot be summarised in place")
        self.ptr = t.data_ptr() + 8 * c0 if t.numel() else 0


def _fracs(quantiles):
    q = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
    if q.size > _native.CHAIN_MAX_NQ or not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError("at most %d quantile fractions, each in [0, 1]" % _native.CHAIN_MAX_NQ)
    return q


def _run(v, q, window=None, rhat=False):
    """lfg_chain_stats on view v: a dict of device tensors (nothing is read
    back, nothing synchronises)."""
    import torch
    L = _native.lib()
    C, nq, dev = v.C, q.size, v.device
    with torch.cuda.device(dev):
        out = {"n": torch.empty(C, dtype=torch.int64, device=dev),
               "n_bad": torch.empty(C, dtype=torch.int64, device=dev)}
        for k in ("mean", "m2", "min", "max"):
            out[k] = torch.empty(C, dtype=torch.float64, device=dev)
        out["ostat"] = torch.empty((C, nq, 2), dtype=torch.float64, device=dev)
        out["quant"] = torch.empty((C, nq), dtype=torch.float64, device=dev)
        out["rhat"] = torch.empty(C, dtype=torch.float64, device=dev) if rhat else None
        nbytes = L.lfg_chain_workspace_size(v.steps, v.W, C, nq)
        if nbytes == 0:
            raise ValueError("lfg_chain_stats refuses %d columns (at most %d)" % (C, _native.CHAIN_MAX_C))
        ws = _native.Workspace.get(nbytes, dev)

        def P(t):
            return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
        rc = L.lfg_chain_stats(ctypes.c_void_p(v.ptr), v.steps, v.W, C, v.step_ld, v.walker_ld, P(window),
                               q.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if nq else None, nq,
                               P(out["n"]), P(out["n_bad"]), P(out["mean"]), P(out["m2"]), P(out["min"]),
                               P(out["max"]), P(out["ostat"]), P(out["quant"]), P(out["rhat"]), P(ws), nbytes,
                               _native.stream_ptr(dev))
    _native.check(rc, "lfg_chain_stats")
    return out


def _to_host(out, q):
    return ChainStats(q, **{k: (None if t is None else t.cpu().numpy()) for k, t in out.items()})


def stats(chain, cols=None, quantiles=DEFAULT_QUANTILES, window=None, rhat=False, nskip=0, thin=1, device=None,
          walker_major=False):
    """Per-column summary of a chain (module docstring) -> ChainStats.
    window: [C, 2] inclusive bounds (host or device), values outside are not
    used; rhat: Gelman-Rubin over the walkers (not with a window)."""
    import torch
    v = _View(chain, cols, walker_major, nskip, thin, device)
    q = _fracs(quantiles)
    if window is not None:
        if rhat:
            raise ValueError("R-hat is not defined for a windowed chain")
        window = torch.as_tensor(window, dtype=torch.float64).to(v.device).reshape(v.C, 2).contiguous()
    return _to_host(_run(v, q, window, rhat), q)


def gr_diagnostic(chain):
    """mcmc_utils.GR_diagnostic: R-hat per parameter of a chain shaped
    (nwalkers, nsteps, ndim)."""
    return stats(chain, quantiles=(), rhat=True, walker_major=True).rhat


def _clip_rounds(v, sigma, maxiters):
    """maxiters rounds of (stats, clip) and the final stats, all on the device"""
    import torch
    L = _native.lib()
    q = np.array([0.5])
    win = None
    for _ in range(int(maxiters)):
        r = _run(v, q, win)
        nxt = torch.empty((v.C, 2), dtype=torch.float64, device=v.device)
        with torch.cuda.device(v.device):
            rc = L.lfg_chain_clip(ctypes.c_void_p(r["n"].data_ptr()), ctypes.c_void_p(r["m2"].data_ptr()),
                                  ctypes.c_void_p(r["quant"].data_ptr()), 1, float(sigma),
                                  None if win is None else ctypes.c_void_p(win.data_ptr()),
                                  ctypes.c_void_p(nxt.data_ptr()), v.C, _native.stream_ptr(v.device))
        _native.check(rc, "lfg_chain_clip")
        win = nxt
    return _run(v, q, win), q


def sigma_clipped_stats(chain, sigma=3.0, maxiters=5, cols=None, nskip=0, thin=1, device=None, walker_major=False,
                        full=False):
    """astropy.stats.sigma_clipped_stats at its defaults, per column: maxiters
    rounds dropping what lies further than sigma standard deviations from the
    median, then (mean, median, std) of what survives (std with ddof 0).  The
    rounds never leave the device.  full=True returns the last round's
    ChainStats as a fourth item."""
    v = _View(chain, cols, walker_major, nskip, thin, device)
    out, q = _clip_rounds(v, sigma, maxiters)
    s = _to_host(out, q)
    res = (s.mean, s.quant[:, 0], s.std(0))
    return res + (s,) if full else res


def wd_fluxes(chain, names, syserr=0.03, corrections=None):
    """wdparams.fluxes_from_chain on the device: a Flux per wdFlux_* column
    (kg5 columns are skipped), from its sigma-clipped mean and standard
    deviation."""
    from .wdparams import Flux
    picked = [(i, key.lower().replace("wdflux_", "")) for i, key in enumerate(names)
              if "wdflux" in key.lower() and "kg5" not in key.lower()]
    if not picked:
        return []
    c0, c1 = picked[0][0], picked[-1][0] + 1
    mean, _, std = sigma_clipped_stats(chain, cols=slice(c0, c1))
    return [Flux(mean[i - c0], std[i - c0], band, syserr=syserr, correction=(corrections or {}).get(band))
            for i, band in picked]


def write_modparams(names, mean, q84, q16, out_dir="."):
    """modparams.csv in the reference's format: one row per parameter, the
    columns 'mean', '84th percentile', '16th percentile'."""
    import pandas as pd
    result = pd.DataFrame({"mean": np.asarray(mean, dtype=np.float64),
                           "84th percentile": np.asarray(q84, dtype=np.float64),
                           "16th percentile": np.asarray(q16, dtype=np.float64)}, index=list(names))
    path = os.path.join(out_dir, "modparams.csv")
    result.to_csv(path, header=True)
    return path, result


def model_report(model, heading):
    """one block of the reference's before/after report"""
    dof = int(np.sum([ecl.lc.x.size for ecl in model.search_node_type('Eclipse')]))
    dof -= len(model.dynasty_par_vals) + 1
    text = "\n\n{} has a chisq of {:.3f} ({:d} D.o.F.).\n".format(heading, model.chisq(), dof)
    text += "\nEvaluating the model, we get;\n"
    text += "a ln_prior of {:.3f}\n".format(model.ln_prior())
    text += "a ln_like of {:.3f}\n".format(model.ln_like())
    text += "a ln_prob of {:.3f}\n".format(model.ln_prob())
    return text


def fit_summary(chain, names, input_file=None, nskip=0, thin=1, out_dir=".", lnprob=None, walker_major=False,
                log=print, corners=False, corner_plots=True):
    """The numbers of the reference's fit_summary.  Writes modparams.csv (mean,
    84th and 16th percentile of every chain parameter, in header order) into
    out_dir.  With input_file the model is rebuilt and evaluated at its start
    and at the chain means: the two report blocks are printed and returned.
    With lnprob [steps][W] the per-step mean and ddof-0 standard deviation of
    ln_prob are returned (the reference's ln_prob.pdf).

    A row of the chain may be wider than len(names) (a chain file's trailing
    ln_prob): the columns beyond are not read.

    One deliberate difference: thin thins, [nskip::thin], as flatchain does.
    In the reference thin never reaches the summarised frame; at the default
    thin = 1 the two agree.  The model plots and e-mail are out of scope.

    corners=True (with input_file) adds the reference's corner plots, from
    counts made on the device (corner.eclipse_corners): per eclipse
    <out_dir>/Final_figs/<lightcurve stem>_corners.npz and, where matplotlib
    imports, _corners.png (corner_plots=False: the counts alone; matplotlib
    needs seconds per eclipse for a 20-column triangle).  The reference draws
    them by default; here they are opt-in, so that existing callers see no
    change.

    -> dict: modparams (the path), result (the DataFrame), stats (ChainStats),
    initial_report, final_report, lnprob_mean, lnprob_std, and with corners
    the list of files written."""
    names = list(names)
    s = stats(chain, cols=len(names), quantiles=(0.16, 0.84), nskip=nskip, thin=thin, walker_major=walker_major)
    path, result = write_modparams(names, s.mean, s.quant[:, 1], s.quant[:, 0], out_dir)
    out = {"modparams": path, "result": result, "stats": s, "initial_report": None, "final_report": None,
           "lnprob_mean": None, "lnprob_std": None}
    if input_file is not None:
        from . import cvmodel
        model = cvmodel.construct_model(input_file)
        out["initial_report"] = model_report(model, "Initial guess")
        log(out["initial_report"])
        model.dynasty_par_dict = {k: float(m) for k, m in zip(names, s.mean)}
        out["final_report"] = model_report(model, "MCMC result")
        log(out["final_report"])
        if corners:
            from . import corner
            out["corners"] = corner.eclipse_corners(chain, names, model, os.path.join(out_dir, "Final_figs"),
                                                    nskip=nskip, thin=thin, walker_major=walker_major,
                                                    plot=corner_plots, log=log)
    if lnprob is not None:
        import torch
        lp = torch.as_tensor(lnprob, dtype=torch.float64)
        lp = lp.t() if walker_major else lp
        out["lnprob_mean"] = lp.mean(dim=1).cpu().numpy()
        out["lnprob_std"] = lp.std(dim=1, unbiased=False).cpu().numpy()
    return out
