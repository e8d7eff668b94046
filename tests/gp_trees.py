"""Test helper: synthetic GP trees (GPLCModel -> Band -> ComplexGPEclipse /
SimpleGPEclipse) at the shapes where the GP likelihood kernels take another
path than on the shipped useGP = 1 example: fewer points than k_gp_like has
segments, a segment cut on a block's first point, tied phases, three blocks,
eclipses over one tile, sub-bins, one eclipse per walker.

Parameter values and priors are lfit_python_amd.synthetic's (the example
input's); the three GP hyper-parameters start at the example's values with
priors widened for the tests.  Every leaf has its own phases x, w = 0.001,
ye ~ U(0.003, 0.006) (seeded) and
    y = oracle flux at the start values + ye N(0, 1) + 0.003 sin(20 x),
so that the GP has something to absorb.

case(oracle, name) -> (model, nsub, walkers).  The walkers are p0 (1 + 0.005
N(0, 1)) with five designated rows (ROW_*) overwritten.  CALL_W[name] is the
number of walkers a GPU test hands to one call: the walkers go through in
consecutive chunks of that size (chunks()), so that the launch has the
case's walker count (a lone pair, a dead second pair in the last wave) while
every case still holds all five designated rows.

rule_case(oracle, name) -> (model, walkers): the rule family at the end of
this file, the 120 % cache rule at its edges with data laddered around every
block edge the independent double's dist_cp gives.
"""
import numpy as np

from lfit_python_amd import synthetic
from lfit_python_amd.cvmodel import Band, ComplexGPEclipse, GPLCModel, Lightcurve, SimpleGPEclipse
from lfit_python_amd.tree import Param

# The hyper-parameter ranges of the designated row (d).  The bar of the GPU
# tests (1e-9 relative) rests on two CPU forms of the filter (the segment form
# of tests/gp_kalman.py and a restatement of the kernel's adjugate combine)
# agreeing with the dense oracle to <= 8e-14 in these ranges at ye ~ U(0.003,
# 0.006), and to <= 9e-13 at ye x 0.1 in SHARP's.  They must not be widened:
# at ye x 0.1 with ln_amp up to -4 the adjugate form is already 8e-10 off, and
# at ye x 0.01 the dense oracle and the Cholesky-form filter differ by 4e-7
# themselves, so that no reference is left to measure against.
LN_AMP = (-16.0, -4.0)
LN_TAU = (-10.0, -1.0)
LN_AMP_SHARP = (-12.0, -7.0)   # case "sharp" (ye x 0.1)

GP_CORE = {  # the example's start values; priors widened
    'ln_ampin_gp': '-9.5118 uniform -25.0 -1.0 1',
    'ln_ampout_gp': '-9.0953 uniform -25.0 -1.0 1',
    'ln_tau_gp': '-2.2131 uniform -15.0 0.0 1',
}
WIDTH = 0.001
WIGGLE = 0.003
EDGE_GAP = 1e-7   # no datum closer than this to a changepoint (device and oracle agree on dist_cp to ~1e-11)

ROW_DPHI, ROW_Q, ROW_RWD, ROW_HYPER, ROW_OUT = 0, 1, 2, 3, 4   # rows (a) .. (e)
FINITE_ROWS = (ROW_DPHI, ROW_Q, ROW_RWD, ROW_HYPER)

CASES = ("tiny", "cuts", "seam", "cycles", "subbin", "sharp", "one")
CALL_W = {"tiny": 7, "cuts": 8, "seam": 4, "cycles": 3, "subbin": 4, "sharp": 8, "one": 1}
TOTAL_W = {"tiny": 7, "cuts": 8, "seam": 8, "cycles": 6, "subbin": 8, "sharp": 8, "one": 6}
TWO_KERNEL = ("seam", "cycles", "subbin")   # lfg_layout(tree) == 0 whatever lfg_set_layout says


def chunks(name, W):
    k = CALL_W[name]
    return [slice(i, min(i + k, W)) for i in range(0, W, k)]


def build_tree(oracle, leaves, nsub=1, complex_bs=True, ye_scale=1.0, fixed=(), seed=0):
    """leaves: [(label of synthetic's eclipse values, x)]; fixed: eclipse
    parameter names that get isVar = 0"""
    rng = np.random.default_rng(seed)
    pars = [Param.fromString(k, synthetic.CORE[k]) for k in ('q', 'dphi', 'rwd')]
    pars += [Param.fromString(k, GP_CORE[k]) for k in ('ln_ampin_gp', 'ln_ampout_gp', 'ln_tau_gp')]
    core = GPLCModel('core', pars)
    leaf_cls = ComplexGPEclipse if complex_bs else SimpleGPEclipse
    bands = {}
    for label, x in leaves:
        band, pstr = synthetic.eclipse_param_strings(label, complex_bs=complex_bs)
        if band not in bands:
            bands[band] = Band(band, [Param.fromString(k, synthetic.BANDS[band][k]) for k in Band.node_par_names],
                               parent=core)
        x = np.asarray(x, dtype=np.float64)
        ye = ye_scale * rng.uniform(0.003, 0.006, x.size)
        lc = Lightcurve('synthetic_gp_%s' % label, x, np.zeros_like(x), ye, np.full(x.size, WIDTH))
        ps = [Param.fromString(k, pstr[k]) for k in leaf_cls.node_par_names]
        for p in ps:
            if p.name in fixed:
                p.isVar = False
        leaf = leaf_cls(lc, label, ps, parent=bands[band])
        leaf.nsub = nsub
        st, f = oracle.flux(leaf.cv_parlist, lc.x, lc.w, nsub=nsub)
        assert st == 0
        lc.y = f + ye * rng.standard_normal(x.size) + WIGGLE * np.sin(20.0 * x)
    return core


def _uniform_sorted(rng, n, lo=-0.3, hi=0.3):
    return np.sort(rng.uniform(lo, hi, n))


def cuts_phases(oracle, seed=5):
    """64 phases for the start values' blocks [-1 + dcp + phi0, -dcp + phi0],
    [dcp + phi0, 1 - dcp + phi0]: 32 points at or below edge - 1e-7 and 32 at
    or above edge + 1e-7 (edge = dcp + phi0), so that block 1 opens on point
    32 = 64 * 4 / 8, a segment's first point; one point 1e-7 inside and one
    1e-7 outside the ingress edge -dcp + phi0; points 39, 40, 41 (in block 1,
    across the cut at 40) tied."""
    rng = np.random.default_rng(seed)
    q, dphi, rwd = (float(synthetic.CORE[k].split()[0]) for k in ('q', 'dphi', 'rwd'))
    phi0 = synthetic._EVALS['0'][1][7]
    dcp = oracle.gp_base_dcp(q, dphi, rwd)
    ing, edge = -dcp + phi0, dcp + phi0
    x = np.concatenate([
        _uniform_sorted(rng, 12, -0.3, ing - 0.002), [ing - EDGE_GAP],              # 13 in block 0
        [ing + EDGE_GAP], _uniform_sorted(rng, 17, ing + 0.002, edge - 0.002), [edge - EDGE_GAP],  # 19 in eclipse
        [edge + EDGE_GAP], _uniform_sorted(rng, 31, edge + 0.002, 0.3)])            # 32 in block 1
    x[40] = x[41] = x[39]
    assert x.size == 64 and np.all(np.diff(x) >= 0) and x[31] < edge < x[32]
    return x


def _tree(oracle, name):
    rng = np.random.default_rng(100 + CASES.index(name))
    if name == "tiny":       # fewer points than segments; ragged: max_n = 9
        return build_tree(oracle, [(str(k), _uniform_sorted(rng, n)) for k, n in enumerate((1, 2, 7, 9))],
                          complex_bs=False, seed=11), 1
    if name in ("cuts", "sharp", "one"):
        return build_tree(oracle, [('0', cuts_phases(oracle))], ye_scale=0.1 if name == "sharp" else 1.0,
                          fixed=('phi0',), seed=12), 1
    if name == "seam":       # one point in the second tile; L.N = 513 against n = 40
        return build_tree(oracle, [('0', _uniform_sorted(rng, 513)), ('2', _uniform_sorted(rng, 40))], seed=13), 1
    if name == "cycles":     # three tiles, the last partial; gp_ecl = [0, 2]: three blocks, two eclipses in view
        return build_tree(oracle, [('0', np.linspace(-0.3, 1.3, 1100))], seed=14), 1
    if name == "subbin":     # k_lnlike<2, true>: one tile and two
        return build_tree(oracle, [('0', np.linspace(-0.3, 0.3, 300)), ('2', np.linspace(-0.3, 0.3, 600))], nsub=3,
                          seed=15), 3
    raise KeyError(name)


def case(oracle, name):
    model, nsub = _tree(oracle, name)
    names = model.dynasty_par_names
    col = lambda prefix: [i for i, n in enumerate(names) if n.startswith(prefix)]
    rng = np.random.default_rng(200 + CASES.index(name))
    p0 = np.array(model.dynasty_par_vals)
    W = TOTAL_W[name]
    walk = p0 * (1.0 + 0.005 * rng.standard_normal((W, p0.size)))
    # (a), (b), (c): the start values with one of dphi, q, rwd moved by more
    # than 120 %: the changepoint cache rule trips (k_gp_dcp)
    for row, nm in ((ROW_DPHI, 'dphi_'), (ROW_Q, 'q_'), (ROW_RWD, 'rwd_')):
        walk[row] = p0
        walk[row, col(nm)[0]] /= 2.3
    # the Roche prior wants rwd / 3 <= scale <= 3 rwd (SimpleEclipse.ln_prior)
    walk[ROW_RWD, col('scale_')] = 2.5 * walk[ROW_RWD, col('rwd_')[0]]
    # (d): hyper-parameters from their whole range
    amp = LN_AMP_SHARP if name == "sharp" else LN_AMP
    walk[ROW_HYPER, col('ln_ampin_gp')[0]] = rng.uniform(*amp)
    walk[ROW_HYPER, col('ln_ampout_gp')[0]] = rng.uniform(*amp)
    walk[ROW_HYPER, col('ln_tau_gp')[0]] = rng.uniform(*LN_TAU)
    # (e): a dFlux outside its prior uniform(0.001, 0.2): -inf
    walk[ROW_OUT, col('dFlux_')[0]] = 0.3
    return model, nsub, walk


def eclipse_pars(tree, e, v):
    return np.array([v[g] if g >= 0 else tree.consts[-1 - g] for g in tree.gather[e, :tree.npars[e]]])


def hyper(tree, e, v):
    return np.exp([v[g] if g >= 0 else tree.consts[-1 - g] for g in tree.gp_gather[e]])


def blocks(oracle, tree, e, v):
    """The blocks of eclipse e for walker v as lfo_lnprob_batch_gp forms
    them: dist_cp at the cache's base values, or at the walker's own when one
    of q, dphi, rwd is more than 120 % off the base."""
    p = eclipse_pars(tree, e, v)
    q, dphi, rwd, phi0 = p[4], p[5], p[8], p[13]
    B = tree.gp_base[e]
    if abs(B[1] - dphi) / dphi > 1.2 or abs(B[0] - q) / q > 1.2 or abs(B[2] - rwd) / rwd > 1.2:
        dcp = oracle.gp_base_dcp(q, dphi, rwd)
    else:
        dcp = oracle.gp_base_dcp(*B[:3])
    return np.array([[((ec - 1) + dcp) + phi0, (ec - dcp) + phi0]
                     for ec in range(tree.gp_ecl[e, 0], tree.gp_ecl[e, 1] + 1)]).reshape(-1, 2)


def edge_clearance(oracle, tree, walkers):
    """the smallest distance of a datum to a changepoint over all walkers"""
    best = np.inf
    for v in walkers:
        if not np.all(np.isfinite(v)):
            continue
        for e in range(tree.E):
            x = tree.x[tree.offsets[e]:tree.offsets[e + 1]]
            try:
                b = blocks(oracle, tree, e, v)
            except ValueError:
                continue
            if b.size and x.size:
                best = min(best, np.min(np.abs(x[:, None] - b.reshape(-1)[None, :])))
    return best


def check_case(name, walkers, ref):
    """what keeps a test of the case from passing empty: the share of finite
    walkers and the designated rows, in the oracle's ln_prob"""
    fin = np.isfinite(ref)
    assert 4 * fin.sum() >= 3 * len(ref), (name, fin)
    assert fin[list(FINITE_ROWS)].all(), (name, fin)
    assert np.isneginf(ref[ROW_OUT]), (name, ref[ROW_OUT])


# ---------------------------------------------------------------- the rule family
# MODEL_SPEC 10.3's cache rule |base - v| / v > 1.2 at its edges, through the
# likelihood.  |B - v| / v = B / v - 1 for v < B, so the threshold is v = B / 2.2:
# a divisor of 2.2 (1 + 1e-3) trips the rule (1.2022), 2.2 (1 - 1e-3) does not
# (1.1978); no row lies within 1e-6 relative of the threshold, whose own
# verdict depends on a rounding.  v > B can never trip (|B - v| / v < 1).
#
# Every dist_cp here is the independent double's (tests/wdphases_double.py),
# recorded in tests/golden/wdphases_double.npz under rule_*; the blocks are the
# double's Python rule, not oracle.gp_base_dcp.  Each leaf's phases are 64
# random ones plus a ladder: for the cached dist_cp and for every tripped
# row's own, at both block edges inside the data (-dcp + phi0, dcp + phi0),
# points at edge +- RUNGS.  The smallest rung is 100 PHASE_ATOL, so a dist_cp
# off by more than 1e-8 moves a datum across an edge.
RULE_CASES = ("rule_e1", "rule_e3")
RULE_CALL_W = {"rule_e1": 12, "rule_e3": 7}    # e3: 21 pairs, k_gp_dcp's blocks of 4 mix pending and cached pairs
RULE_LEAVES = {"rule_e1": ("0",), "rule_e3": ("0", "1", "2")}
RUNGS = (1e-8, 1e-7, 1e-6, 1e-5, 1e-4)
TRIP, KEEP = 2.2 * (1.0 + 1e-3), 2.2 * (1.0 - 1e-3)
RULE_ROWS = ("trip_q", "keep_q", "high_q", "trip_dphi", "keep_dphi", "high_dphi", "trip_rwd", "keep_rwd", "high_rwd",
             "two", "hyper", "out")
RULE_TRIPPED = ("trip_q", "trip_dphi", "trip_rwd", "two")
RULE_FINITE = RULE_ROWS[:-1]
HIGH = {"q": 0.49, "rwd": 0.0999}   # the priors' upper ends (synthetic.CORE); dphi: findphi(q, 90) - 1e-5
RULE_GOLDEN = "wdphases_double.npz"


def rule_values(high_dphi=None):
    """name -> (q, dphi, rwd) of the rows the double's dist_cp is recorded
    for (the base, the tripped rows, the rows just short of tripping)"""
    q, dphi, rwd = (float(synthetic.CORE[k].split()[0]) for k in ('q', 'dphi', 'rwd'))
    out = {"base": (q, dphi, rwd),
           "trip_q": (q / TRIP, dphi, rwd), "trip_dphi": (q, dphi / TRIP, rwd), "trip_rwd": (q, dphi, rwd / TRIP),
           "two": (q, dphi / 2.3, rwd / 2.3),
           "keep_q": (q / KEEP, dphi, rwd), "keep_dphi": (q, dphi / KEEP, rwd), "keep_rwd": (q, dphi, rwd / KEEP)}
    if high_dphi is not None:
        out.update(high_q=(HIGH["q"], dphi, rwd), high_dphi=(q, high_dphi, rwd), high_rwd=(q, dphi, HIGH["rwd"]))
    return out


def rule_dcp():
    """name -> the double's recorded dist_cp, held to rule_values() bit for bit"""
    import os
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", RULE_GOLDEN))
    vals = rule_values()
    out = {}
    for k, name in enumerate(d["rule_name"]):
        assert (d["rule_q"][k], d["rule_dphi"][k], d["rule_rwd"][k]) == vals[str(name)], name
        out[str(name)] = float(d["rule_dcp"][k])
    assert set(out) == set(vals)
    return out


def rule_phases(label, dcp, rng):
    phi0 = synthetic._EVALS[label][1][7]
    x = [_uniform_sorted(rng, 64)]
    for name in ("base",) + RULE_TRIPPED:
        for edge in (-dcp[name] + phi0, dcp[name] + phi0):
            x.append([edge + sg * r for r in RUNGS for sg in (-1.0, 1.0)])
    x = np.sort(np.concatenate(x))
    assert x.size == 64 + 20 * 5 and np.min(np.diff(x)) >= 0.9 * RUNGS[0]
    return x


def rule_case(oracle, name):
    """(model, walkers [12, ndim]) of a rule tree; the rows are RULE_ROWS"""
    dcp = rule_dcp()
    rng = np.random.default_rng(300 + RULE_CASES.index(name))
    leaves = RULE_LEAVES[name]
    # e1: a simple bright-spot leaf; e3: complex leaves
    model = build_tree(oracle, [(lab, rule_phases(lab, dcp, rng)) for lab in leaves], complex_bs=len(leaves) > 1,
                       seed=16)
    names = model.dynasty_par_names
    col = lambda prefix: [i for i, n in enumerate(names) if n.startswith(prefix)]  # noqa: E731
    p0 = np.array(model.dynasty_par_vals)
    vals = rule_values(high_dphi=oracle.findphi(p0[col('q_')[0]], 90.0) - 1e-5)
    walk = np.tile(p0, (len(RULE_ROWS), 1))
    for row, rname in enumerate(RULE_ROWS):
        if rname in vals:
            for nm, v in zip(('q', 'dphi', 'rwd'), vals[rname]):
                walk[row, col(nm + '_')[0]] = v
            # the Roche prior wants rwd / 3 <= scale <= 3 rwd (SimpleEclipse.ln_prior)
            walk[row, col('scale_')] = walk[row, col('rwd_')[0]]
    hrng = np.random.default_rng(400 + RULE_CASES.index(name))
    row = RULE_ROWS.index("hyper")
    walk[row, col('ln_ampin_gp')[0]] = hrng.uniform(*LN_AMP)
    walk[row, col('ln_ampout_gp')[0]] = hrng.uniform(*LN_AMP)
    walk[row, col('ln_tau_gp')[0]] = hrng.uniform(*LN_TAU)
    walk[RULE_ROWS.index("out"), col('dFlux_')[0]] = 0.3     # outside uniform(0.001, 0.2): -inf
    return model, walk


def rule_blocks(tree, e, v, dcp):
    """the blocks of eclipse e for walker v by the double's rule and recorded
    dist_cp values (dcp: rule_dcp()); a tripped walker must be a recorded one"""
    from tests import wdphases_double as wd
    p = eclipse_pars(tree, e, v)
    q, dphi, rwd, phi0 = p[4], p[5], p[8], p[13]
    base = tuple(tree.gp_base[e, :3]) + (dcp["base"],)
    assert base[:3] == rule_values()["base"]
    own = None
    if wd.tripped(base, q, dphi, rwd):
        own = [dcp[n] for n, val in rule_values().items() if val == (q, dphi, rwd)][0]
    return np.array(wd.blocks(base, q, dphi, rwd, phi0, int(tree.gp_ecl[e, 0]), int(tree.gp_ecl[e, 1]), own=own))


def rule_reference(oracle, tree, walk, dcp, nsub=1, blocks_fn=None):
    """lnlike_e [W, E] on the host: y - oracle.flux through the dense GP with
    the double's blocks; NaN where the flux fails"""
    out = np.full((len(walk), tree.E), np.nan)
    for i, v in enumerate(walk):
        for e in range(tree.E):
            sl = slice(tree.offsets[e], tree.offsets[e + 1])
            st, f = oracle.flux(eclipse_pars(tree, e, v), tree.x[sl], tree.w[sl], nsub=nsub)
            if st != 0:
                continue
            b = (blocks_fn or rule_blocks)(tree, e, v, dcp)
            out[i, e] = oracle.gp_lnlike(tree.x[sl], tree.y[sl] - f, tree.ye[sl], *hyper(tree, e, v), b)
    return out
