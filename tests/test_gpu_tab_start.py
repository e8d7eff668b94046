"""GPU: the element tables of wide eclipses with the tabulated start of the
tangency solves (LFG_TAB_START, lfg_device.hpp; the library's default build)
against the oracle, as test_gpu_parity.py::test_element_tables compares them.
The (q, dphi, rdisc) sets below reach the largest contact angles the model
produces (+-0.105 in phase: cells of the direction table up to k = 11); the
oracle finds all 1500 elements of each eclipsed."""
import numpy as np
import pytest

from tests.helpers import TRUTH18
from tests.test_gpu_parity import PHASE_ATOL, _elements_gpu

pytestmark = pytest.mark.gpu

WIDE = ((0.6, 0.10, 0.45), (1.0, 0.115, 0.40), (0.3, 0.085, 0.55), (2.0, 0.13, 0.30))


@pytest.mark.parametrize("q,dphi,rdisc", WIDE)
def test_element_tables_wide_eclipse(oracle, q, dphi, rdisc):
    pars = np.array(TRUTH18, dtype=float)
    pars[4], pars[5], pars[6] = q, dphi, rdisc
    st, a, b, wg, don, geo = _elements_gpu(pars)
    ost, oa, ob, ow, odon, ogeo = oracle.elements(pars)
    assert ost == 0 and st[0] == 0
    ecl = oa < ob
    assert ecl.sum() > 50
    assert np.array_equal(a[0] < b[0], ecl)
    da, db = np.max(np.abs(a[0][ecl] - oa[ecl])), np.max(np.abs(b[0][ecl] - ob[ecl]))
    print("q %.2f dphi %.3f rdisc %.2f: %d eclipsed, contacts %.4f .. %.4f, max |da| %.2e, |db| %.2e"
          % (q, dphi, rdisc, ecl.sum(), a[0][ecl].min(), b[0][ecl].max(), da, db))
    assert da < PHASE_ATOL and db < PHASE_ATOL
