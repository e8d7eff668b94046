"""GPU: the Python layer's scratch on more than one stream.

include/lfg.h's entry points are re-entrant on the caller's stream; the
Python layer hands them the scratch of _native.Workspace.  Two callers on two
streams must therefore never share a scratch buffer (nothing orders their
kernels), and a buffer a stream has outgrown must outlive the work queued on
it.  The first two tests pin that rule deterministically; the third makes the
calls overlap (a large batch on stream A, a small one of another shape on
stream B, no synchronisation between) and compares with the serial results
bit for bit: it can only catch a race when the kernels happen to overlap.
lfit.flux_batch, lfit.lnlike_batch and LnProbEvaluator.predict return device
tensors, so their two calls are both in flight; gp.predict_batch copies its
result to the host before it returns, so its call on stream A has finished
when stream B's begins: for it the test shows only that a side stream gives
the serial result and that the two streams worked in different scratch."""
import numpy as np
import pytest

from tests.helpers import random_pars

pytestmark = pytest.mark.gpu


def _storage(t):
    return t.untyped_storage().data_ptr()


def test_two_streams_never_get_the_same_scratch():
    import torch
    from lfit_python_amd._native import Workspace
    dev = torch.device("cuda", torch.cuda.current_device())
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        a = Workspace.get(4096, dev)
        assert _storage(Workspace.get(1024, dev)) == _storage(a)       # grow-only: reused on its own stream
        assert _storage(Workspace.get(4096, "cuda")) == _storage(a)    # however the device is spelled
    with torch.cuda.stream(sb):
        b = Workspace.get(1024, dev)
    d = Workspace.get(1024, dev)                                        # the default stream
    assert len({_storage(a), _storage(b), _storage(d)}) == 3
    with torch.cuda.stream(sa):
        assert _storage(Workspace.get(4096, dev)) == _storage(a)
    with torch.cuda.stream(sb):
        assert _storage(Workspace.get(512, dev)) == _storage(b)


def test_outgrown_scratch_outlives_the_work_queued_on_it():
    import torch
    from lfit_python_amd._native import Workspace
    dev = torch.device("cuda", torch.cuda.current_device())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        small = Workspace.get(1 << 16, dev)
        old = _storage(small)
        small.fill_(3)                      # work queued on it
        del small
        big = Workspace.get(1 << 20, dev)   # outgrown: replaced ...
        assert big.numel() >= 1 << 20 and _storage(big) != old
        held = [(e, b) for e, b in Workspace._retired if _storage(b) == old]
        assert len(held) == 1               # ... and kept, with an event on its stream
        s.synchronize()
        assert held[0][0].query()           # the event completes once that work has run
        del held
        Workspace.get(16, dev)              # the next request lets it go
        assert not any(_storage(b) == old for _, b in Workspace._retired)


def _pairs(oracle):
    """(call on stream A, call on stream B) for each Python entry point that takes Workspace scratch"""
    import torch
    from lfit_python_amd import batch, gp, lfit
    from tests import gp_smoother as gs
    from tests import gp_trees
    xa = np.linspace(-0.3, 0.3, 300)
    xb = np.linspace(-0.2, 0.25, 65)
    pa, pb = random_pars(2048, seed=5), random_pars(8, complex_bs=False, seed=6)
    rng = np.random.default_rng(8)
    ya, yb = 0.05 + 0.01 * rng.standard_normal(300), 0.05 + 0.01 * rng.standard_normal(65)

    def flux(p, x):
        return lambda: list(lfit.flux_batch(p, x))             # device tensors: nothing waits

    def lnlike(p, x, y):
        return lambda: list(lfit.lnlike_batch(p, x, y, 1e-3 * np.ones_like(y)))

    def predict(seed, N, W):
        cases = [gs.make_case(seed + 1000 * k, N, 2) for k in range(W)]
        x, ye, t = cases[0][0], cases[0][1], cases[0][5]
        res, hyp, bl = (np.stack([c[k] for c in cases]) for k in (2, 3, 4))
        return lambda: list(gp.predict_batch(x, ye, res, hyp, bl, t))   # host arrays: it waits on its stream

    def tree_predict(W, seed):
        # LnProbEvaluator.predict (lfg_gp_predict_tree in Workspace scratch): device tensors
        m, nsub, walk = gp_trees.case(oracle, "cuts")
        ev = batch.LnProbEvaluator(batch.compile_tree(m, nsub=nsub))
        p0 = np.array(m.dynasty_par_vals)
        walkers = p0 * (1.0 + 0.005 * np.random.default_rng(seed).standard_normal((W, p0.size)))

        def call():
            out = ev.predict(torch.as_tensor(walkers, device="cuda"))
            return [out[k] for k in ("flux", "gp_mean", "gp_var", "status")]
        return call

    return {"flux_batch": lambda: (flux(pa, xa), flux(pb, xb)),
            "lnlike_batch": lambda: (lnlike(pa, xa, ya), lnlike(pb, xb, yb)),
            "evaluator_predict": lambda: (tree_predict(1024, 1), tree_predict(3, 2)),
            "gp_predict_batch": lambda: (predict(3, 300, 2048), predict(4, 65, 3))}


@pytest.mark.parametrize("entry", ["flux_batch", "lnlike_batch", "evaluator_predict", "gp_predict_batch"])
def test_two_streams_give_the_serial_results(oracle, entry):
    import torch
    call_a, call_b = _pairs(oracle)[entry]()
    host = lambda ts: [t.cpu().numpy() if hasattr(t, "cpu") else t for t in ts]
    want_a = host(call_a())
    torch.cuda.synchronize()
    want_b = host(call_b())
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    # enqueue on A, then at once on B; the results are fetched after both
    from lfit_python_amd import _native
    for rep in range(3):
        with torch.cuda.stream(sa):
            got_a = call_a()
        with torch.cuda.stream(sb):
            got_b = call_b()
        torch.cuda.synchronize()
        for g, w in ((host(got_a), want_a), (host(got_b), want_b)):
            assert len(g) == len(w)
            for u, v in zip(g, w):
                np.testing.assert_array_equal(u, v)
    with torch.cuda.stream(sa):
        wa = _native.Workspace.get(256, "cuda")
    with torch.cuda.stream(sb):
        wb = _native.Workspace.get(256, "cuda")
    assert _storage(wa) != _storage(wb)     # the two calls above worked in different scratch
