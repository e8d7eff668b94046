"""Walker populations of the FP32-opener tests (test_f32_open.py on the host
build, test_gpu_f32_open.py on the device): config 2's ball as
tools/tol_study.py builds it, and a grazing ball, the same tree with dphi
(hence the inclination) lowered until the oracle's element table of the
central walker holds both eclipsed and uneclipsed disc elements.  Each case
is built once per session and shared; nothing in it is modified afterwards."""
import functools

import numpy as np

from lfit_python_amd import batch, sampler, synthetic

NWD, NDISC = 400, 1000  # MODEL_SPEC 5
W = 64
MIN_CLASS = 0.05  # each class (eclipsed, not eclipsed) of the grazing walker's disc elements


def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


def disc_eclipsed_fraction(O, cv_pars):
    st, a, b, _, _, _ = O.elements(cv_pars)
    assert st == 0
    d = slice(NWD, NWD + NDISC)
    return float(np.mean(a[d] < b[d]))


@functools.lru_cache(maxsize=None)
def case(grazing):
    """(tree, walkers [W, ndim], oracle ln_prob [W], eclipsed fraction of the
    central walker's disc elements)"""
    O = _oracle()
    f = lambda p, x, w, nsub: O.flux(p, x, w, nsub=nsub)[1]  # noqa: E731
    if not grazing:
        m = synthetic.config_single(300, flux_fn=f)
    else:
        m = synthetic.config_single(300)
        names = m.dynasty_par_names
        k = [i for i, n in enumerate(names) if n.startswith("dphi")][0]
        vals = np.array(m.dynasty_par_vals)
        leaf = m.leaves()[0]
        for dphi in np.arange(0.038, 0.0105, -0.001):
            vals[k] = dphi
            m.dynasty_par_vals = list(vals)
            fr = disc_eclipsed_fraction(O, leaf.cv_parlist)
            if MIN_CLASS <= fr <= 1.0 - MIN_CLASS:
                break
        rng = np.random.default_rng(synthetic.SEED)
        y = f(leaf.cv_parlist, leaf.lc.x, leaf.lc.w, 1)
        leaf.lc.y = y + synthetic.NOISE * rng.standard_normal(y.shape)
    frac = disc_eclipsed_fraction(O, m.leaves()[0].cv_parlist)
    t = batch.compile_tree(m)
    p0 = np.array(m.dynasty_par_vals)
    walk = sampler.initialise_walkers(p0, sampler.comp_scatter(m.dynasty_par_names, 0.1), W,
                                      lambda p: O.lnprob_batch(p, t)[0], seed=3)
    ref, _, _ = O.lnprob_batch(walk, t)
    walk.setflags(write=False)
    ref.setflags(write=False)
    return t, walk, ref, frac
