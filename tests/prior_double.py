"""Host double of the device's prior lanes: ln_prior of a compiled tree in
numpy on oracle primitives, term by term, so that a test can say which term
rejected a walker; and the edge walkers the prior tests share.

ln_prior restates MODEL_SPEC 8 (model.py:426-474, CVModel.py:193-324,
440-491) directly; tests/test_prior_double.py pins it against the reference's
own ln_prior before anything on the device is compared with it."""
import dataclasses

import numpy as np

DISC_MAX_A = 0.46    # CVModel.py:217
AZ_SLOPE = 80.0      # CVModel.py:282
DPHI_TOL = 1e-6      # CVModel.py:452
GAUSS, GAUSSPOS, UNIFORM, LOG_UNIFORM, MOD_JEFF = range(5)
# ln of the smallest positive double and of the smallest normal one: between
# them a pdf is a denormal and the reference's log(pdf) is coarse (MODEL_SPEC 8)
LN_DENORM_MIN = float(np.log(5e-324))
LN_NORMAL_MIN = float(np.log(np.finfo(np.float64).tiny))
LN_SQRT_2PI = 0.5 * float(np.log(2.0 * np.pi))


def cv_pars(tree, walkers):
    """[W, E, 18] CV parameters as oracle.lnprob_batch routes them (gather >= 0:
    a walker column, < 0: consts[-1 - g])."""
    walkers = np.asarray(walkers, np.float64)
    g = tree.gather
    consts = tree.consts if len(tree.consts) else np.zeros(1)
    cols = walkers[:, np.clip(g, 0, walkers.shape[1] - 1)]
    return np.where(g[None] >= 0, cols, consts[np.clip(-1 - g, 0, len(consts) - 1)][None])


def ln_prior(oracle, tree, walkers, roche_priors=None):
    """(total [W], parts) of mcmcfit.ln_prior for the walkers [W, ndim].

    parts["box"] [W, ndim]: the Prior.ln_prob term of every variable parameter;
    parts["dphi"] [W], parts["rdisc"], ["scale"], ["bspot"], ["az"] [W, E]:
    True where that Roche check rejects (all of them are evaluated, not only
    the first that fails); parts["fixed"]: the tree's fixed_invalid flag;
    parts["margin"]: the distance of every Roche check from its limit
    (positive = inside), NaN where it cannot be formed."""
    walkers = np.asarray(walkers, np.float64)
    W = walkers.shape[0]
    roche = tree.roche_priors if roche_priors is None else roche_priors
    E = tree.E
    box = np.zeros((W, tree.ndim))
    if tree.prior_type is not None:
        for d in range(tree.ndim):
            ty, p1, p2, nm = tree.prior_type[d], tree.prior_p1[d], tree.prior_p2[d], tree.prior_norm[d]
            box[:, d] = [oracle.prior_lnprob(ty, p1, p2, nm, v) for v in walkers[:, d]]
    parts = {"box": box, "fixed": bool(tree.fixed_invalid)}
    for k in ("rdisc", "scale", "bspot", "az"):
        parts[k] = np.zeros((W, E), bool)
    parts["dphi"] = np.zeros(W, bool)
    mg = {k: np.full((W, E), np.nan) for k in ("rdisc", "scale_hi", "scale_lo", "az_lo", "az_hi")}
    mg["dphi"] = np.full(W, np.nan)
    parts["margin"] = mg
    if roche:
        P = cv_pars(tree, walkers)
        for w in range(W):
            q, dphi = P[w, 0, 4], P[w, 0, 5]
            try:
                mg["dphi"][w] = (oracle.findphi(q, 90.0) - DPHI_TOL) - dphi
                parts["dphi"][w] = dphi > oracle.findphi(q, 90.0) - DPHI_TOL
            except ValueError:
                parts["dphi"][w] = True
            for e in range(E):
                p = P[w, e]
                q, rdisc, rwd, scale, az = p[4], p[6], p[8], p[9], p[10]
                if not (q > 0.0 and np.isfinite(q)):   # no Roche geometry: every check fails
                    for k in ("rdisc", "scale", "bspot", "az"):
                        parts[k][w, e] = True
                    continue
                rdisc_a = rdisc * oracle.xl1(q)
                mg["rdisc"][w, e] = DISC_MAX_A - rdisc_a
                parts["rdisc"][w, e] = rdisc_a > DISC_MAX_A
                mg["scale_hi"][w, e] = rwd * 3.0 - scale
                mg["scale_lo"][w, e] = scale - rwd / 3.0
                parts["scale"][w, e] = scale > rwd * 3.0 or scale < rwd / 3.0
                try:
                    x, y = oracle.bspot(q, rdisc_a)[:2]
                except ValueError:
                    parts["bspot"][w, e] = True
                    continue
                alpha = np.degrees(np.arctan2(y, x))
                if alpha < 0.0:
                    alpha = 90.0 - alpha
                tangent = alpha + 90.0
                minaz, maxaz = max(0.0, tangent - AZ_SLOPE), min(178.0, tangent + AZ_SLOPE)
                mg["az_lo"][w, e], mg["az_hi"][w, e] = az - minaz, maxaz - az
                parts["az"][w, e] = az < minaz or az > maxaz
    bad = parts["dphi"] | parts["rdisc"].any(1) | parts["scale"].any(1) | parts["bspot"].any(1) | parts["az"].any(1)
    total = box.sum(1)
    total[~np.isfinite(total)] = -np.inf
    total[bad] = -np.inf
    if parts["fixed"]:
        total[:] = -np.inf
    return total, parts


def rejected_by(parts, w):
    """names of the terms that make walker w -inf (for assertion messages)"""
    out = ["box[%d]" % d for d in np.nonzero(~np.isfinite(parts["box"][w]))[0]]
    out += ["dphi"] if parts["dphi"][w] else []
    for k in ("rdisc", "scale", "bspot", "az"):
        out += ["%s[%d]" % (k, e) for e in np.nonzero(parts[k][w])[0]]
    return out + (["fixed"] if parts["fixed"] else [])


# ---------------------------------------------------------------- prior tables
def prior_norm(ty, p1, p2):
    from lfit_python_amd.tree import PRIOR_TYPES, Prior
    return Prior(PRIOR_TYPES[ty], p1, p2).normalise


def table_tree(base, start, types, p1, p2, roche_priors=False):
    """`base` with every CV parameter a constant (its value in the walker
    `start`) and a prior table of len(types) free-standing parameters: the
    prior lanes see the walker columns, the model sees `start`."""
    types = np.asarray(types, np.int32)
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    nd = len(types)
    consts = cv_pars(base, np.asarray(start, np.float64)[None, :])[0].reshape(-1).copy()
    gather = -1 - np.arange(base.E * 18, dtype=np.int32).reshape(base.E, 18)
    return dataclasses.replace(
        base, ndim=nd, names=["p%d" % d for d in range(nd)], gather=gather, consts=consts,
        prior_type=types, prior_p1=p1, prior_p2=p2,
        prior_norm=np.array([prior_norm(t, a, b) for t, a, b in zip(types, p1, p2)], np.float64),
        roche_priors=roche_priors)


# one prior of each type with both limits away from 0 where the type allows,
# so that 0.0, -0.0 and a negative value are distinct edge cases
TYPE_PRIORS = {GAUSS: (0.284, 0.001), GAUSSPOS: (0.32, 0.03), UNIFORM: (-0.2, 0.5),
               LOG_UNIFORM: (0.001, 0.2), MOD_JEFF: (0.01, 1.0)}


def interior(ty, p1, p2):
    if ty <= GAUSSPOS:
        return p1 + 0.5 * p2
    if ty == UNIFORM:
        return 0.5 * (p1 + p2) + 0.01
    return np.sqrt(p1 * p2) if ty == LOG_UNIFORM else 0.3 * p2


def edge_values(ty, p1, p2):
    """the edge list of one prior: p1, p2, their neighbours, zeros, a negative
    value, the non-finite values, and for the Gaussians z = 0, 37, 40 (the pdf
    underflows between the last two, at 38.6 sigma for p2 = 1)"""
    inf = np.inf
    v = [p1, p2, np.nextafter(p1, inf), np.nextafter(p1, -inf), np.nextafter(p2, inf), np.nextafter(p2, -inf),
         0.0, -0.0, -0.05, inf, -inf, np.nan]
    if ty <= GAUSSPOS:
        v += [p1 + z * p2 for z in (0.0, 37.0, 40.0)]
    return v


def edge_walkers(types, p1, p2, seed):
    """interior point; every dimension at every edge value of its type in
    turn; 64 random rows with each coordinate an edge value with probability
    0.2"""
    nd = len(types)
    mid = np.array([interior(t, a, b) for t, a, b in zip(types, p1, p2)])
    edges = [edge_values(t, a, b) for t, a, b in zip(types, p1, p2)]
    rows = [mid.copy()]
    for d in range(nd):
        for v in edges[d]:
            r = mid.copy()
            r[d] = v
            rows.append(r)
    rng = np.random.default_rng(seed)
    for _ in range(64):
        r = mid.copy()
        for d in np.nonzero(rng.random(nd) < 0.2)[0]:
            r[d] = edges[d][rng.integers(len(edges[d]))]
        rows.append(r)
    return np.array(rows)


# ---------------------------------------------------- Roche priors at their limits
# Margins of the cases below against what the suite pins between the device's
# and the oracle's primitives (tests/test_gpu_parity.py): findphi 1e-11 ->
# dphi +-1e-9; bspot position 1e-12 (an angle of < 1e-9 degrees at r >= 0.05)
# -> az +-1e-7 degrees; xl1 1e-13 relative -> rdisc +-1e-9 relative; the scale
# window is plain double arithmetic (1e-16) -> +-1e-12 relative.  A case whose
# reference margin is non-zero and smaller than these is a construction error.
MARGIN = {"dphi": 1e-10, "rdisc": 1e-10, "scale_hi": 1e-15, "scale_lo": 1e-15, "az_lo": 1e-8, "az_hi": 1e-10}
Q_LO, Q_HI, Q_PATCHES = 0.002, 5.0, 10     # the stream table's q range (MODEL_SPEC 4.5)
LQW = 0.7824046                            # ln(Q_HI / Q_LO) / Q_PATCHES
WIDE = {"q": (UNIFORM, -1.0, 10.0), "dphi": (UNIFORM, 0.0, 0.5), "rdisc": (UNIFORM, 0.01, 0.99),
        "scale": (LOG_UNIFORM, 1e-4, 1.0), "az": (UNIFORM, -10.0, 200.0)}


def widen(tree):
    """the box priors of q, dphi, rdisc, scale and az widened so that only the
    Roche terms decide at their limits"""
    ty, p1, p2, nm = (np.array(a) for a in (tree.prior_type, tree.prior_p1, tree.prior_p2, tree.prior_norm))
    for d, name in enumerate(tree.names):
        key = name.split("_")[0]
        if key in WIDE:
            ty[d], p1[d], p2[d] = WIDE[key]
            nm[d] = prior_norm(ty[d], p1[d], p2[d])
    return dataclasses.replace(tree, prior_type=ty, prior_p1=p1, prior_p2=p2, prior_norm=nm)


def az_window(oracle, q, rdisc):
    x, y = oracle.bspot(q, rdisc * oracle.xl1(q))[:2]
    alpha = np.degrees(np.arctan2(y, x))
    if alpha < 0.0:
        alpha = 90.0 - alpha
    return max(0.0, alpha + 90.0 - AZ_SLOPE), min(178.0, alpha + 90.0 + AZ_SLOPE)


def eclipse_limit_cases(oracle, tree, p0, label):
    """[(name, column name, value)]: one parameter of eclipse `label` moved
    from the walker p0 to each side of its Roche limits"""
    ix = {n: d for d, n in enumerate(tree.names)}
    q, rwd = p0[ix["q_core"]], p0[ix["rwd_core"]]
    rd, sc, az = "rdisc_" + label, "scale_" + label, "az_" + label
    minaz, maxaz = az_window(oracle, q, p0[ix[rd]])
    assert maxaz == 178.0 and minaz > 1.0
    rmax = DISC_MAX_A / oracle.xl1(q)
    c = [("rdisc-", rd, rmax * (1 - 1e-9)), ("rdisc+", rd, rmax * (1 + 1e-9)),
         ("scale_hi-", sc, 3 * rwd * (1 - 1e-12)), ("scale_hi+", sc, 3 * rwd * (1 + 1e-12)),
         ("scale_lo+", sc, rwd / 3 * (1 + 1e-12)), ("scale_lo-", sc, rwd / 3 * (1 - 1e-12)),
         ("scale_hi=", sc, rwd * 3.0), ("scale_lo=", sc, rwd / 3.0),
         ("az_lo-", az, minaz - 1e-7), ("az_lo+", az, minaz + 1e-7),
         ("az_hi-", az, 178.0 - 1e-9), ("az_hi+", az, 178.0 + 1e-9), ("az0", az, 0.0)]
    return c


def dphi_limit_qs():
    """(name, q) for the dphi <= findphi(q, 90) - 1e-6 cases: the middle of
    every table patch, both sides of two patch boundaries, the table's ends
    and the solver fallback beyond them"""
    qs = [("mid%d" % k, Q_LO * np.exp(LQW * (k + 0.5))) for k in range(Q_PATCHES)]
    for k in (3, 7):
        qb = Q_LO * np.exp(LQW * k)
        qs += [("edge%d-" % k, qb * (1 - 1e-6)), ("edge%d+" % k, qb * (1 + 1e-6))]
    return qs + [("qlo", Q_LO), ("qhi", Q_HI), ("below", 0.0015), ("above", 6.0)]


def roche_limit_walkers(oracle, tree, p0):
    """(names, walkers) of the one-eclipse tree: the truth p0, every limit of
    eclipse_limit_cases, the dphi limit at the truth's q and at every q of
    dphi_limit_qs (rdisc, az and scale re-chosen inside their windows where
    one exists: below q ~ 0.01 no disc radius passes both bspot and the 0.46
    limit, and the reference rejects both sides), q = 0, -0.1, NaN, inf, and
    a disc inside the stream's periastron (bspot fails)."""
    ix = {n.split("_")[0]: d for d, n in enumerate(tree.names)}
    p0 = np.asarray(p0, np.float64)
    names, rows = ["truth"], [p0.copy()]
    for name, col, v in eclipse_limit_cases(oracle, tree, p0, tree.names[ix["rdisc"]].split("_", 1)[1]):
        r = p0.copy()
        r[tree.names.index(col)] = v
        names.append(name)
        rows.append(r)
    for qn, q in [("truth", p0[ix["q"]])] + dphi_limit_qs():
        r = p0.copy()
        r[ix["q"]] = q
        if qn != "truth":
            x1 = oracle.xl1(q)
            for rdisc_a in (0.3, 0.2, 0.4, 0.455, 0.1):
                try:
                    oracle.bspot(q, rdisc_a)
                except ValueError:
                    continue
                r[ix["rdisc"]] = rdisc_a / x1
                lo, hi = az_window(oracle, q, r[ix["rdisc"]])
                r[ix["az"]] = 0.5 * (lo + hi)
                break
            r[ix["scale"]] = r[ix["rwd"]]
        lim = oracle.findphi(q, 90.0) - DPHI_TOL
        for s, sign in (("-", -1.0), ("+", 1.0)):
            rr = r.copy()
            rr[ix["dphi"]] = lim + sign * 1e-9
            names.append("dphi_%s%s" % (qn, s))
            rows.append(rr)
    for qn, q in (("q0", 0.0), ("qneg", -0.1), ("qnan", np.nan), ("qinf", np.inf)):
        r = p0.copy()
        r[ix["q"]] = q
        names.append(qn)
        rows.append(r)
    r = p0.copy()
    r[ix["rdisc"]] = 0.05
    names.append("bspot_fails")
    rows.append(r)
    return names, np.array(rows)


def assert_clear_of_limits(parts, names=None):
    """no Roche margin of the reference lies within MARGIN of its limit
    (exact zeros are the deliberately placed equalities)"""
    for k, tol in MARGIN.items():
        m = parts["margin"][k]
        close = np.isfinite(m) & (m != 0.0) & (np.abs(m) < tol)
        assert not close.any(), (k, np.argwhere(close), m[close], names)


# ------------------------------------------------------- chunk and lane edges
CHUNK_NDIMS = (1, 15, 16, 17, 31, 32, 33, 48)   # around the prior lanes' chunks of 16 parameters
CHUNK_IDS = ["nd%d" % n for n in CHUNK_NDIMS] + ["first16_log_uniform", "first16_gauss"]
# the shuffles' seed: nd1's single parameter is a log_uniform, the one type whose
# edge list rejects often enough for a quarter of that table's rows to be -inf
CHUNK_SEED = 106
LANE_W = (1, 5, 64, 257)                        # k_setup's lane bounds: slices of the walker set


def chunk_table(case):
    """(types, p1, p2) of one prior table of CHUNK_IDS: the five types cycling
    in a seeded shuffle, so that every chunk mixes them; the two named tables
    start with 16 parameters of one type."""
    k = CHUNK_IDS.index(case)
    rng = np.random.default_rng(CHUNK_SEED + k)
    nd = CHUNK_NDIMS[k] if k < len(CHUNK_NDIMS) else 48
    order = rng.permutation(5)
    types = np.array([order[d % 5] for d in range(nd)], np.int32)
    if case == "first16_log_uniform":
        types[:16] = LOG_UNIFORM
    elif case == "first16_gauss":
        types[:16] = GAUSS
    p1 = np.array([TYPE_PRIORS[t][0] for t in types])
    p2 = np.array([TYPE_PRIORS[t][1] for t in types])
    return types, p1, p2


def chunk_case(case):
    """(types, p1, p2, walkers) of one table of CHUNK_IDS"""
    types, p1, p2 = chunk_table(case)
    return types, p1, p2, edge_walkers(types, p1, p2, 200 + CHUNK_IDS.index(case))


def assert_chunk_case_balanced(types, walkers, ref, parts):
    """on the reference alone: the case cannot hide a failure behind rows
    that are all finite or all -inf, for the table or for any of its types"""
    fin = np.isfinite(ref)
    W = len(ref)
    assert 4 * fin.sum() >= W and 4 * (~fin).sum() >= W, (W, fin.sum())
    for ty in np.unique(types):
        cols = types == ty
        # a row this type decides: its own terms finite or -inf, the others' finite
        others = np.isfinite(parts["box"][:, ~cols]).all(1)
        mine = np.isfinite(parts["box"][:, cols]).all(1)
        assert (others & mine).any() and (others & ~mine).any(), ty


# --------------------------------------------------- the Gaussian underflow rule
UNDERFLOW_P2 = (1e-3, 0.03, 1.0, 100.0, 1e6)
UNDERFLOW_HALF_Z2 = (684.5, 700.0, 740.0, 750.0, 760.0)
# finite rows whose pdf is a denormal: z^2/2 = 740 for p2 = 1e-3, 0.03, 1 and
# z^2/2 = 700 for p2 = 1e6, for gauss and gaussPos each
UNDERFLOW_BAND_ROWS = 8


def underflow_case():
    """(types, p1, p2, walkers, e): one gauss and one gaussPos parameter
    per p2; walker k puts every parameter at z^2 / 2 = UNDERFLOW_HALF_Z2[k] in
    turn, the others at their mean.  e [W, ndim] = -z^2/2 - ln sqrt(2 pi) of
    the moved parameter (NaN elsewhere)."""
    types = np.array([GAUSS, GAUSSPOS] * len(UNDERFLOW_P2), np.int32)
    p2 = np.repeat(UNDERFLOW_P2, 2)
    p1 = 50.0 * p2                    # gaussPos: v stays positive (z <= 39 < 50)
    rows, e = [], []
    for d in range(len(types)):
        for h in UNDERFLOW_HALF_Z2:
            r = p1.copy()
            r[d] = p1[d] + np.sqrt(2.0 * h) * p2[d]
            z = (r[d] - p1[d]) / p2[d]
            er = np.full(len(types), np.nan)
            er[d] = -z * z / 2.0 - LN_SQRT_2PI
            rows.append(r)
            e.append(er)
    return types, p1, p2, np.array(rows), np.array(e)


# ------------------------------------------------------- attribution in a tree
def tree_attribution_walkers(oracle, tree, p0):
    """(names, walkers, where) of a many-eclipse tree: every Roche limit case
    of one eclipse at a time, and a box violation in a band-level and in an
    eclipse-level parameter.  where[k] = (part, eclipse) the case is aimed at
    (eclipse None: a box term)."""
    p0 = np.asarray(p0, np.float64)
    names, rows, where = ["truth"], [p0.copy()], [None]
    for label in tree.leaf_labels:
        for name, col, v in eclipse_limit_cases(oracle, tree, p0, label):
            r = p0.copy()
            r[tree.names.index(col)] = v
            names.append("%s@%s" % (name, label))
            rows.append(r)
            where.append((col.split("_")[0], tree.leaf_labels.index(label)))
    band = [n for n in tree.names if n.startswith("wdFlux_")][1]
    leaf = "fis_" + tree.leaf_labels[-1]
    for col, v in ((band, 0.3), (leaf, 1.5)):   # uniform(0.001, 0.2), uniform(0.001, 1)
        r = p0.copy()
        r[tree.names.index(col)] = v
        names.append("box:" + col)
        rows.append(r)
        where.append(("box", tree.names.index(col)))
    return names, np.array(rows), where
