#!/usr/bin/env python3
"""Generate tests/golden/wdparams_ref.npz from the reference's own
wdparams_new.py.

    python tools/make_wd_golden.py REFERENCE_DIR

Runs only where a checkout of the reference is at hand (it imports
REFERENCE_DIR/wdparams_new.py, which imports the reference's mcmc_utils.py and
model.py; nothing of the reference travels).  Third-party modules that are
absent are replaced by empty stand-ins (ptemcee, emcee, astropy, seaborn,
past, dask, corner, george, and whatever else fails to import from that
list): the functions recorded here use none of them.  The reference's Flux
asks its questions through input(); a stand-in answers them ("n", or "y",
"tnt", "uspec", <filter> for a corrected band).

For every setup of tests/wd_double.py (prior sets A and B, without corrections
and with g and r corrected) it records, over the fixed batch's finite rows:
gen_apparent_mags, chisq, ln_prior, ln_likelihood, ln_prob, and the Flux
objects' mag and err.  Non-finite rows stay NaN: the spec's rule for them is
not the reference's.
"""
import builtins
import importlib.abc
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from tests import wd_double as wdd  # noqa: E402

STUBS = {"ptemcee", "emcee", "astropy", "seaborn", "past", "dask", "corner", "george", "tqdm"}


class _Anything:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Anything()

    def __getattr__(self, k):
        return _Anything()


class _Stub(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _Anything


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in STUBS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "wdparams_new.py")):
        sys.exit("usage: make_wd_golden.py REFERENCE_DIR (the directory that holds wdparams_new.py)")
    refdir = os.path.abspath(sys.argv[1])
    for name in sorted(STUBS):
        try:
            importlib.import_module(name)
            STUBS.discard(name)      # the real one is here
        except ImportError:
            pass
    sys.meta_path.insert(0, _Finder())
    sys.path.insert(0, refdir)
    spec = importlib.util.spec_from_file_location("ref_wdparams_new", os.path.join(refdir, "wdparams_new.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    from model import Param  # the reference's own

    answers = []
    builtins.input = lambda prompt="": answers.pop(0)
    batch = wdd.fixed_batch()
    theta = batch["theta"]
    fin = np.isfinite(theta).all(axis=1)
    out = {"theta": theta}
    for prior_set, corrected in wdd.COMBOS:
        fluxes = []
        for val, err, band, corr in wdd.fixed_fluxes(corrected):
            answers[:] = ["y", "tnt", "uspec", corr] if corr else ["n"]
            fluxes.append(ref.Flux(val, err, band, syserr=wdd.SYSERR))
            assert not answers
        pars = [Param.fromString(k, wdd.PRIOR_SETS[prior_set][k]) for k in ("teff", "logg", "plax", "ebv")]
        model = ref.wdModel(*pars, fluxes)
        n = len(theta)
        rec = {k: np.full(n, np.nan) for k in ("chisq", "ln_prior", "ln_like", "ln_prob")}
        mags = np.full((n, len(fluxes)), np.nan)
        with np.errstate(all="ignore"):
            for i in np.flatnonzero(fin):
                v = [float(x) for x in theta[i]]
                for k in range(4):
                    model[k] = v[k]
                mags[i] = model.gen_apparent_mags()
                rec["chisq"][i] = model.chisq()
                rec["ln_prior"][i] = ref.ln_prior(v, model)
                rec["ln_like"][i] = ref.ln_likelihood(v, model)
                rec["ln_prob"][i] = ref.ln_prob(v, model)
        tag = prior_set + ("1" if corrected else "0")
        out["mags_" + tag] = mags
        for k, a in rec.items():
            out[k + "_" + tag] = a
        out["obs_mag_" + tag] = np.array([f.mag for f in fluxes])
        out["obs_err_" + tag] = np.array([f.err for f in fluxes])
        out["bands_" + tag] = np.array([f.band for f in fluxes])
        print("%s: %d rows, %d with a finite ln_prob" % (tag, int(fin.sum()), int(np.isfinite(rec["ln_prob"]).sum())))
    np.savez_compressed(wdd.GOLDEN, **out)
    print("wrote %s" % wdd.GOLDEN)


if __name__ == "__main__":
    main()
