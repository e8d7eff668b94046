"""The GP posterior of MODEL_SPEC 10.5 on the CPU: the numpy restatement of
the filter and the modified Bryson-Frazier pass (tests/gp_smoother.py), and
the host twin lfg_cpu_gp_predict (the device text of lfg_device.hpp compiled
for the host), against the dense conditional; and the prior-path simulation
at zero and tiny steps."""
import numpy as np
import pytest

from tests import gp_smoother as gs

from tests.gp_smoother import make_case, check

SHAPES = [(1, 0), (1, 2), (2, 3), (17, 0), (63, 2), (64, 3), (65, 2), (300, 3)]


@pytest.mark.parametrize("N,nb", SHAPES)
def test_restatement_matches_dense(N, nb):
    x, ye, r, hyp, blocks, t = make_case(N + nb, N, nb)
    xm, obs, ix, it = gs.merge(x, t)
    rm = np.zeros(xm.size)
    rm[ix] = r
    yem = np.ones(xm.size)
    yem[ix] = ye
    mean, var = gs.smooth(xm, yem, obs, rm, *hyp, blocks)
    check(mean[it], var[it], x, ye, r, hyp, blocks, t)
    check(mean[ix], var[ix], x, ye, r, hyp, blocks, x)   # t = x, the reference's call


@pytest.fixture(scope="module")
def port(tmp_path_factory):
    from cpu_baseline import cpu
    return cpu.CpuPort(cpu.build(out=str(tmp_path_factory.mktemp("cpu") / "liblfg_cpu.so")))


@pytest.mark.parametrize("N,nb", SHAPES)
def test_cpu_twin_matches_dense(port, N, nb):
    W = 3
    cases = [make_case(100 * w + N + nb, N, nb) for w in range(W)]
    x, ye, _, _, _, t = cases[0]
    xm, obs, ix, it = gs.merge(x, t)
    res = np.full((W, xm.size), np.nan)   # res is ignored where obs = 0
    yem = np.full(xm.size, np.nan)
    yem[ix] = ye
    for w in range(W):
        res[w, ix] = cases[w][2]
    hyp = np.stack([c[3] for c in cases])
    blocks = np.stack([c[4] for c in cases]) if nb else np.zeros((W, 0, 2))
    mean, var, st = port.gp_predict(xm, yem, obs, res, hyp, blocks)
    mean1, none, st1 = port.gp_predict(xm, yem, obs, res, hyp, blocks, return_var=False)
    assert none is None and not st.any() and not st1.any()
    for w in range(W):
        check(mean[w, it], var[w, it], x, ye, cases[w][2], hyp[w], blocks[w], t)
        check(mean1[w, it], None, x, ye, cases[w][2], hyp[w], blocks[w], t)


def test_cpu_twin_failures(port):
    x, ye, r, hyp, blocks, t = make_case(5, 40, 2)
    xm, obs, ix, it = gs.merge(x, t)
    res = np.zeros((4, xm.size))
    res[:, ix] = r
    yem = np.ones(xm.size)
    yem[ix] = ye
    res[1, ix[3]] = np.nan          # a datum
    res[3, it[0]] = np.nan          # a test point: ignored
    H = np.tile(hyp, (4, 1))
    H[2, 2] = 0.0                   # tau = 0
    mean, var, st = port.gp_predict(xm, yem, obs, res, H, np.tile(blocks, (4, 1, 1)))
    assert st[0] == 0 and st[3] == 0 and st[1] != 0 and st[2] != 0
    assert np.isnan(mean[1:3]).all() and np.isnan(var[1:3]).all()
    check(mean[0, it], var[0, it], x, ye, r, hyp, blocks, t)
    assert np.array_equal(mean[0], mean[3]) and np.array_equal(var[0], var[3])
    _, _, st = port.gp_predict(xm[::-1].copy(), yem[::-1].copy(), obs[::-1].copy(), res[:1, ::-1].copy(), H[:1],
                               blocks[None])
    assert st[0] != 0               # descending x


def test_prior_path_zero_and_tiny_steps():
    """A step of d = 0 reproduces the state exactly; d = 1e-12 stays finite
    and moves it by ~sqrt(Q) only; no NaN either way."""
    rng = np.random.default_rng(0)
    for tau in (np.exp(-6.9), np.exp(-2.0)):
        lam = np.sqrt(3.0 / tau)
        assert np.array_equal(gs.step_noise(lam, 0.0), np.zeros((2, 2)))
        c = gs.step_noise(lam, 1e-12)
        assert np.isfinite(c).all() and c[0, 0] > 0 and c[1, 1] > 0
        # against Q = Pinf - Phi Pinf Phi^T where that form is still accurate
        d = 0.4 / lam
        F2 = gs._phi(lam, d)[:2, :2]
        pinf = np.diag([1.0, lam * lam])
        c = gs.step_noise(lam, d)
        assert np.allclose(c @ c.T, pinf - F2 @ pinf @ F2.T, rtol=1e-9, atol=0)
        x = np.array([0.0, 0.0, 1e-12, 1e-12, 0.05, 0.05, 0.3])
        blocks = [(0.04, 0.2)]
        f, st = gs.prior_path(x, 1e-4, 2e-4, tau, blocks, rng.standard_normal((len(x), 4)))
        assert np.isfinite(f).all() and np.isfinite(st).all()
        assert np.array_equal(st[1], st[0]) and np.array_equal(st[3], st[2]) and np.array_equal(st[5], st[4])
        assert f[1] == f[0] and f[5] == f[4]
        assert np.max(np.abs(st[2] - st[1]) / np.array([1.0, lam, 1.0, lam])) < 1e-3 * np.sqrt(2e-4)


def test_prior_path_covariance_is_the_kernel():
    """The simulated path has the kernel's covariance: the linear map from the
    normals to f* is L with L L^T = K (exact, no sampling)."""
    tau, ain, aout = np.exp(-4.0), 3e-5, 8e-5
    x = np.array([-0.2, -0.1, -0.1, 0.0, 0.02, 0.05, 0.11, 0.2, 0.3])
    blocks = [(-0.15, -0.01), (0.01, 0.25)]
    n = len(x)
    L = np.zeros((n, 4 * n))
    for j in range(4 * n):
        xi = np.zeros(4 * n)
        xi[j] = 1.0
        L[:, j] = gs.prior_path(x, ain, aout, tau, blocks, xi.reshape(n, 4))[0]
    K = gs.kernel(x, x, ain, aout, tau, blocks)
    assert np.max(np.abs(L @ L.T - K)) <= 1e-12 * (ain + aout)
