"""GPU: ln_prob with the FP32 opener of the element solves (LFG_F32_OPEN,
lfg_device.hpp; the library's default build) against the oracle, on the
populations of tests/f32_open_cases.py (64 walkers x 1 eclipse x 300 points)
through k_pair and through k_elements + k_lnlike, and on a simple-spot
eclipse and an E = 3 tree, which reach k_pair's other instantiations and
k_combine_walkers."""
import numpy as np
import pytest

from tests import f32_open_cases as cases
from tests.test_gpu_lnprob import LAYOUTS, LNP_RTOL, _flux_fn, _same, layout  # noqa: F401 (layout: a fixture)

pytestmark = pytest.mark.gpu


def _gpu_lnprob(t, walk):
    import torch
    from lfit_python_amd import batch
    return batch.LnProbEvaluator(t)(torch.as_tensor(np.array(walk), device="cuda")).cpu().numpy()


@LAYOUTS
@pytest.mark.parametrize("grazing", [False, True], ids=["config2", "grazing"])
def test_lnprob_matches_oracle(grazing, layout):
    t, walk, ref, frac = cases.case(grazing)
    assert np.all(np.isfinite(ref))
    if grazing:
        assert cases.MIN_CLASS <= frac <= 1.0 - cases.MIN_CLASS
    _same(_gpu_lnprob(t, walk), ref, LNP_RTOL)


@pytest.mark.parametrize("cfg", ["simple_spot", "tree_e3"])
def test_other_instantiations_match_oracle(oracle, cfg):
    from lfit_python_amd import batch, synthetic
    if cfg == "simple_spot":
        m = synthetic.config_single(300, complex_bs=False, flux_fn=_flux_fn)
    else:
        m = synthetic.config_tree(1, 300, flux_fn=_flux_fn)
    t = batch.compile_tree(m)
    assert t.E == (1 if cfg == "simple_spot" else 3)
    rng = np.random.default_rng(5)
    p0 = np.array(m.dynasty_par_vals)
    walk = p0 * (1.0 + 0.01 * rng.standard_normal((16, p0.size)))
    ref, _, _ = oracle.lnprob_batch(walk, t)
    assert np.isfinite(ref).sum() >= 8
    _same(_gpu_lnprob(t, walk), ref, LNP_RTOL)
