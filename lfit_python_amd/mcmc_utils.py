"""The sampler utilities of the reference's mcmc_utils.py over the
device-resident EnsembleSampler: same names, arguments and file formats.

  initialise_walkers(p, scatter, nwalkers, ln_prior, model)   mcmc_utils.py:46-72
  initialise_walkers_pt(p, scatter, nwalkers, ntemps, ln_prior, model)
                                                                mcmc_utils.py:75-111
  run_burnin(sampler, startPos, nSteps, storechain=False)      mcmc_utils.py:114-132
  run_mcmc_save(sampler, startPos, nSteps, rState, file, col_names)
                                                                mcmc_utils.py:135-183
  run_ptmcmc_save(sampler, startPos, nSteps, file, col_names=)  mcmc_utils.py:186-239
  flatchain(chain, npars=None, nskip=0, thin=1)                 mcmc_utils.py:242-249
  readchain(file) / readchain_dask(file)                        mcmc_utils.py:252-300
  readflatchain(file)                                           mcmc_utils.py:303-306
  GR_diagnostic(sampler_chain)   (chainstats.gr_diagnostic)     mcmc_utils.py:317-351
  posterior_predictive(ev, samples, chunk=)   the numbers behind
                                              plot_lc_model.plot_GP_eclipse

The emcee RNG state the reference threads from the burn-in into production
(`state` -> `rstate0`) is the sampler's Philox counter here
(EnsembleSampler.random_state).  run_mcmc_save keeps the chain on the device
and writes it in bulk chunks instead of re-opening the file for every row
(mcmc_utils.py:157-164); the rows are the reference's format.
"""
import numpy as np

from . import sampler as _sampler
from .chainstats import gr_diagnostic
from .chainstats import gr_diagnostic as GR_diagnostic  # the reference's name


def initialise_walkers(p, scatter, nwalkers, ln_prior, model=None, seed=0):
    """A Gaussian ball around p resampled until every walker has a finite
    ln_prior (mcmc_utils.py:46-72).  ln_prior(p, model) as mcmcfit.ln_prior
    (one vector), or -- marked with `ln_prior.batched = True` -- a function
    of the whole [n, ndim] batch (e.g. batched_ln_prior(evaluator))."""
    if getattr(ln_prior, "batched", False):
        fn = lambda x: np.asarray(ln_prior(x, model))  # noqa: E731
    else:
        fn = lambda x: np.array([ln_prior(v, model) for v in x])  # noqa: E731
    return _sampler.initialise_walkers(p, scatter, nwalkers, fn, seed=seed)


def initialise_walkers_pt(p, scatter, nwalkers, ntemps, ln_prior, model=None, seed=0):
    """A Gaussian ball per temperature level, all ntemps * nwalkers walkers
    resampled together until every ln_prior is finite (mcmc_utils.py:75-111);
    returns [ntemps, nwalkers, ndim].  ln_prior as in initialise_walkers."""
    p0 = initialise_walkers(p, scatter, int(nwalkers) * int(ntemps), ln_prior, model, seed=seed)
    return p0.reshape(int(ntemps), int(nwalkers), -1)


def batched_ln_prior(evaluator):
    """mcmcfit.ln_prior (mcmcfit.py:30-34) for a whole batch on the device
    (lfg_lnprior through a batch.LnProbEvaluator); usable as the ln_prior of
    initialise_walkers."""
    import torch

    def ln_prior(x, model=None):
        return evaluator.ln_prior(torch.as_tensor(np.asarray(x, dtype=np.float64),
                                                  device=evaluator.device)).cpu().numpy()
    ln_prior.batched = True
    return ln_prior


def run_burnin(sampler, startPos, nSteps, storechain=False, progress=False):
    """Burn-in (mcmc_utils.py:114-132): returns (pos, prob, state), with
    state the RNG counter to hand to run_mcmc_save.  The steps run back to
    back on the device (EnsembleSampler.run_mcmc); the reference's
    `for pos, prob, state in sampler.sample(...)` loop also works on the
    sampler, one host copy per step."""
    return sampler.run_mcmc(startPos, nSteps, storechain=storechain)


def run_mcmc_save(sampler, startPos, nSteps, rState, file, col_names='', progress=False, chunk=None,
                  lnprob0=None, **kwargs):
    """Production run written to `file` (mcmc_utils.py:135-183): the header
    line col_names, then '{k:4d} {values} {ln_prob:f}' per walker per step.
    rState (from run_burnin) continues the burn-in's random stream; None
    keeps the sampler's own.  Afterwards sampler.chain holds every step, as
    (nwalkers, nSteps, npars) like emcee's.  With torch.distributed every rank
    runs the steps (the ensemble is replicated) and rank 0 alone writes."""
    if rState is not None:
        sampler.random_state = rState
    W, ndim = sampler.W, sampler.ndim
    writer = bool(file) and getattr(sampler, "rank", 0) == 0
    if writer:
        with open(file, "w") as fh:
            fh.write(col_names)
            if col_names:
                fh.write("\n")
    chunk = chunk or max(1, min(nSteps, (1 << 28) // max(1, W * (ndim + 1) * 8)))
    done, first = 0, True
    while done < nSteps:
        k = min(chunk, nSteps - done)
        sampler.run_mcmc(startPos if first else None, k, storechain=True, lnprob0=lnprob0 if first else None)
        if writer:
            ch, lp = sampler.last_run()
            _sampler.write_chain(file, None, ch, lp, mode="a")  # formatted where the chunk lies
        first = False
        done += k
    return sampler


def run_ptmcmc_save(sampler, startPos, nSteps, file, col_names='', chunk=None):
    """Parallel-tempered production run, the cold level written to `file`
    (mcmc_utils.py:186-239): the header line col_names, then per step and
    cold walker '{k:4d} {values} {ln_prob:f}' with the cold level's log
    posterior (beta = 1: ln_like + ln_prior) as ln_prob.  startPos
    [ntemps, nwalkers, ndim], or None to carry on from the sampler's state.
    The steps run in bulk chunks (PTSampler.run_mcmc) instead of one file
    open per row; the rows are the reference's format.  (The reference's
    progress-bar switch is not taken: there is no bar.)"""
    if startPos is None and not sampler.has_state:
        raise ValueError("startPos is None and the sampler holds no state to carry on from")
    if file:
        with open(file, "w") as fh:
            fh.write(col_names)
            if col_names:
                fh.write("\n")
    W, ndim, T = sampler.W, sampler.ndim, (1 if sampler.cold_only else sampler.T)
    chunk = chunk or max(1, min(nSteps, (1 << 28) // max(1, T * W * (ndim + 2) * 8)))
    done, first = 0, True
    while done < nSteps:
        k = min(chunk, nSteps - done)
        sampler.run_mcmc(startPos if first else None, k, storechain=True)
        if file:
            ch, lp, _ = sampler.last_run()
            _sampler.write_chain(file, None, ch[:, 0].numpy(), lp[:, 0].numpy(), mode="a")
        first = False
        done += k
    return sampler


def flatchain(chain, npars=None, nskip=0, thin=1):
    """All walkers' samples as one [n, npars] array, skipping the first nskip
    steps and keeping every thin-th (mcmc_utils.py:242-249)."""
    if hasattr(chain, "cpu"):  # a device tensor
        chain = chain.cpu().numpy()
    chain = np.asarray(chain)
    if npars is None:
        npars = chain.shape[2]
    return chain[:, nskip::thin, :].reshape((-1, npars))


def posterior_predictive(ev, samples, chunk=1024):
    """Per data point, over the flat chain samples [n, ndim], the 16 / 50 /
    84 percentiles of the model flux and of flux + GP mean, and the mean GP
    standard deviation: the bands of the reference's plot_GP_eclipse
    (plot_lc_model.py:208-265) from the whole posterior instead of one
    parameter set.  ev is a batch.LnProbEvaluator of a GP tree; the samples go
    through ev.predict `chunk` at a time.  Samples the priors or the model
    reject (status != 0) are left out.  Returns numpy arrays in the tree's
    point order: {"x", "off", "flux" [3, N], "flux_gp" [3, N], "gp_std" [N],
    "used": the number of samples kept}."""
    import torch
    if hasattr(samples, "cpu"):
        samples = samples.cpu().numpy()
    samples = np.ascontiguousarray(np.asarray(samples, dtype=np.float64).reshape(-1, ev.tree.ndim))
    flux, mean, std = [], [], []
    for lo in range(0, len(samples), int(chunk)):
        r = ev.predict(torch.as_tensor(samples[lo:lo + int(chunk)], device=ev.device))
        ok = (r["status"] == 0).cpu().numpy()
        flux.append(r["flux"].cpu().numpy()[ok])
        mean.append(r["gp_mean"].cpu().numpy()[ok])
        std.append(np.sqrt(r["gp_var"].cpu().numpy()[ok]))
    flux, mean, std = (np.concatenate(a) for a in (flux, mean, std))
    if not len(flux):
        raise ValueError("no sample has a posterior: every status is non-zero")
    q = (16.0, 50.0, 84.0)
    return {"x": ev.tree.x, "off": ev.tree.offsets, "flux": np.percentile(flux, q, axis=0),
            "flux_gp": np.percentile(flux + mean, q, axis=0), "gp_std": std.mean(axis=0), "used": len(flux)}


def readchain(file, **kwargs):
    """chain_prod.txt -> [nwalkers, nprod, npars + 1] (mcmc_utils.py:252-272);
    the last column is ln_prob."""
    return _sampler.read_chain(file)


def readchain_dask(file, **kwargs):
    """The reference's threaded reader (mcmc_utils.py:275-300) falls back to
    readchain when dask is absent; so does this one (same result)."""
    return readchain(file, **kwargs)


def readflatchain(file):
    """A whitespace-separated table read with no header row (e.g. a
    flattened chain) as one array (mcmc_utils.py:303-306: pandas, header=None).

    Parsed in bulk (chainparse.read_table) where that gives what pandas gives:
    a table of numbers that are not all whole (pandas keeps a table of whole
    numbers as integers).  Everything else goes through pandas as before."""
    from . import chainparse
    t = chainparse.try_table(file)
    if t is not None and not np.all(np.isfinite(t) & (t == np.floor(np.where(np.isfinite(t), t, 0.0)))):
        return t
    import pandas as pd
    return np.array(pd.read_csv(file, header=None, sep=r"\s+", float_precision="round_trip"))
