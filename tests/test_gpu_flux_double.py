"""GPU: the device against the flux double (tests/flux_double.py) directly,
not through the oracle: lfg_elements, lfg_flux with components, the
component objects and the fused likelihood.

Needs numpy and tests/golden/flux_double.npz only: no arbiter call and no
scipy here.  The sets, the grids, the bound and its derivation are those of
tests/test_flux_double.py; W = the number of recorded sets.
"""
import numpy as np
import pytest

from tests import flux_double as fd
from tests import test_flux_double as t
from tests.test_gpu_parity import GEO_PAIRS, _elements_gpu

pytestmark = pytest.mark.gpu

SIZES = [1, 65, 512, 513]     # one point, one past a wave, the full k_pair tile, the first LONG shape


def all_pars():
    """the recorded sets as one [W, 18] batch (14 values: the simple spot spelt out)"""
    return np.array([fd.full_pars(t.records()[n]["pars"]) for n in t.NAMES])


def test_elements():
    st, a, b, wg, don, geo = _elements_gpu(all_pars())
    for i, name in enumerate(t.NAMES):
        m = t.the_model(name)
        t.assert_elements(name, m, st[i], a[i], b[i], wg[i], don[i])
        d = {k: geo[i][GEO_PAIRS[k][1]] for k in ("xl1", "inc", "bs_x", "bs_y", "upk", "umax", "bden")}
        t.assert_geometry(name, m, d["xl1"], d["inc"], d["bs_x"], d["bs_y"], d["upk"], d["umax"], d["bden"])


def test_elements_of_14_parameters():
    """the 14-value form takes its own path through the setup lane"""
    rec = t.records()["truth14"]
    st, a, b, wg, don, geo = _elements_gpu(rec["pars"])
    t.assert_elements("truth14", t.the_model("truth14"), st[0], a[0], b[0], wg[0], don[0])


@pytest.mark.parametrize("nsub", [1, 3])
@pytest.mark.parametrize("N", SIZES)
def test_flux_batch(N, nsub):
    from lfit_python_amd.lfit import flux_batch
    pars = all_pars()
    for kind in t.KINDS:
        x, w = t.grid(kind, N)
        flux, status, comps = flux_batch(pars, x, w, nsub=nsub, components=True)
        flux, status, comps = flux.cpu().numpy(), status.cpu().numpy(), comps.cpu().numpy()
        for i, name in enumerate(t.NAMES):
            rec = t.records()[name]
            t.assert_points_clear(rec, x, w)
            assert status[i] == 0
            ref = t.double_curve(name, kind, N, nsub)
            t.assert_light_curve((name, kind, N, nsub), [flux[i]] + [comps[k, i] for k in range(4)], ref, x, w,
                                 nsub, t.flux_params(rec))


def test_flux_batch_14_parameters():
    from lfit_python_amd.lfit import flux_batch
    rec = t.records()["truth14"]
    x, w = t.grid("ragged", 65)
    flux, status, comps = flux_batch(rec["pars"][None, :], x, w, nsub=3, components=True)
    assert status[0].item() == 0
    got = [flux[0].cpu().numpy()] + [comps[k, 0].cpu().numpy() for k in range(4)]
    t.assert_light_curve("truth14", got, fd.light_curve(t.the_model("truth14"), x, w, 3), x, w, 3, t.flux_params(rec))


def _objects(pars, disc_npts=1000, donor_npts=400):
    from lfit_python_amd import lfit
    q, _, _, cps = t.split(pars)
    return [lfit.PyWhiteDwarf(*cps[0]), lfit.PyDisc(q, *cps[1], npts=disc_npts),
            lfit.PySpot(q, *cps[2][:4], exp1=cps[2][4], exp2=cps[2][5], tilt=cps[2][6], yaw=cps[2][7], complex=True),
            lfit.PyDonor(q, donor_npts)]


@pytest.mark.parametrize("kind", ["regular", "wrap", "edges"])
def test_component_objects(kind):
    x, w = t.grid(kind, 300)
    for name in t.NAMES:
        rec = t.records()[name]
        q, phi0, _, _ = t.split(rec["pars"])
        xs = x - phi0
        t.assert_points_clear(dict(rec, pars=np.zeros(14)), xs, w)
        for k, obj in enumerate(_objects(rec["pars"])):
            y = obj.calcFlux(q, float(rec["inc"]), xs, w)
            r, e = t.worst(y, t.double_component(name, k, xs, w), xs, w, 1, 1.0)
            assert r <= 1.0, (name, kind, k, e)


@pytest.mark.parametrize("npts", [250, 777])
def test_component_objects_caller_grids(npts):
    rec = t.records()["truth18"]
    q = float(rec["pars"][4])
    objs = _objects(rec["pars"], npts, npts)
    assert (objs[1].n1, objs[1].n2) == t.DISC_GRIDS[npts] and (objs[3].n1, objs[3].n2) == t.DONOR_GRIDS[npts]
    ab = (rec["disc%d_a" % npts], rec["disc%d_b" % npts])
    for kind in ("regular", "points"):
        x, w = t.grid(kind, 300)
        t.assert_points_clear(dict(rec, pars=np.zeros(14)), x, w, *ab)
        for k, n12, ab_k in ((1, t.DISC_GRIDS[npts], ab), (3, t.DONOR_GRIDS[npts], None)):
            y = objs[k].calcFlux(q, float(rec["inc"]), x, w)
            r, e = t.worst(y, t.double_component("truth18", k, x, w, *n12, ab=ab_k), x, w, 1, 1.0)
            assert r <= 1.0, (npts, kind, k, e)


@pytest.mark.parametrize("kind", ["ragged", "tiny", "edges"])
@pytest.mark.parametrize("N,nsub", [(300, 1), (513, 3)])
def test_fused_likelihood(N, nsub, kind):
    """lfg_lnlike (no flux array leaves the device) on data = the double's
    flux plus seeded noise: chi^2 within the flux bound propagated through
    sum 2 |r| / ye^2 df.  300 points, S = 1 is k_pair's one tile; 513
    points, S = 3 its LONG variant.  The edges grid goes without its NaN
    width, which makes chi^2 infinite: that is the last assertion."""
    from lfit_python_amd.lfit import lnlike_batch
    x, w = t.grid(kind, N)
    ok = ~np.isnan(w)
    for i, name in enumerate(t.NAMES):
        rec = t.records()[name]
        t.assert_points_clear(rec, x, w)
        ref = t.double_curve(name, kind, N, nsub)[0]
        y, ye = t.noisy(np.where(ok, ref, 0.0), 23 + i)
        ll, st = lnlike_batch(rec["pars"][None, :], x[ok], y[ok], ye[ok], w[ok], nsub=nsub)
        want = float(np.sum(((y - ref)[ok] / ye[ok]) ** 2))
        assert st[0].item() == 0
        assert abs(-2.0 * ll[0].item() - want) <= t.chisq_bound(y[ok], ye[ok], ref[ok], x[ok], w[ok], nsub,
                                                                 t.flux_params(rec)), (name, -2.0 * ll[0].item(), want)
        assert 0.5 * N < want < 2.0 * N      # the noise is what it was meant to be
        if not ok.all():
            ll, _ = lnlike_batch(rec["pars"][None, :], x, y, ye, w, nsub=nsub)
            assert ll[0].item() == -np.inf


@pytest.mark.parametrize("mutate", fd.MUTATIONS)
def test_every_mutation_is_seen(mutate):
    """the device misses each mutated double by 100 bounds or more"""
    from lfit_python_amd.lfit import flux_batch
    rec = t.records()["truth18"]
    x, w = t.grid("regular", 300)
    _, _, comps = flux_batch(rec["pars"][None, :], x, w, nsub=1, components=True)
    got = comps[t.TOUCHES[mutate], 0].cpu().numpy()
    assert t.miss(mutate, "regular", 1, ref=got) >= 100.0
