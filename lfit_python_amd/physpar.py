"""Physical parameters from a chain, on the device (MODEL_SPEC.md section 12;
the reference's calcPhysicalParams.py).

    tables = load_mr_tables(base_dir)            the white-dwarf mass-radius tables
    table, model, status = solve(q, dphi, rwd, twd, p, tables)
    table, model, status = from_chain(S.chain_dev, names, twd, e_twd, p, e_p, tables)
    s = summary(table, status); write_results(table, status)

Every row goes through lfg_physpar (include/lfg_physpar.h), one lane per row:
Kepler's law, xl1, the white-dwarf mass at which the geometric radius meets
the first of the Wood 95 / Panei / Hamada-Salpeter relations that brackets
one, then Mw, Rw, logg, Mr, Rr, a, Kw, Kr, incl.  The host's part is reading
and packing the tables (numpy, scipy), once.

The constants are astropy >= 4's values, stated here and not imported (astropy
is not a dependency); CONSTANTS is the one place that holds them, and
load_mr_tables(constants=...) overrides them.
"""
import ctypes
import os

import numpy as np

from . import _native

COLUMNS = ("q", "Mw", "Rw", "logg", "Mr", "Rr", "a", "Kw", "Kr", "incl")
MODELS = ("wood", "panei", "hamada")
# SI; astropy.constants (CODATA 2018, IAU 2015): G, GM_sun, R_sun; units.d
CONSTANTS = {"G": 6.67430e-11, "GMsun": 1.3271244e20, "Rsun": 6.957e8, "day": 86400.0}
ST_NO_MR_SOLUTION = 6

WOOD_FILES = tuple("Wood95/co%03d.2.04dt1" % m for m in (40, 50, 60, 70, 80, 90, 100))
WOOD_MASSES = np.array([0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0])
HAMADA_FILE = "Hamada/mr_hamada.dat"
PANEI_FILES = ("Panei/12C-MR-H-He/12C-MR-H-He.dat", "Panei/12C-MR-H-He/12C-MR-H-He.saver")
BRACKETS = {"wood": (0.4, 1.0), "panei": (0.4, 1.2), "hamada": (0.14, 1.44)}
MAX_ROWS = 2 ** 31 - 1  # rows of one lfg_physpar call (int n)


def read_wood_file(path, rsun_cm):
    """One Wood 95 file: (T [K] increasing, R [R_sun]) from columns 6 and 5
    (calcPhysicalParams.py:17-24), cut at the first temperature that does not
    increase (np.interp is undefined from there on); the number of rows cut
    is the third value."""
    x, y = np.loadtxt(path, usecols=(5, 6)).T
    temp, radius = (10.0 ** y)[::-1], (10.0 ** x / rsun_cm)[::-1]
    bad = np.flatnonzero(np.diff(temp) <= 0.0)
    keep = len(temp) if not bad.size else int(bad[0]) + 1
    return temp[:keep].copy(), radius[:keep].copy(), len(temp) - keep


def cardinal_cubics(masses=WOOD_MASSES):
    """[n-1][n][4]: on interval j the cardinal spline of node k of scipy's
    interp1d(kind='cubic') (the not-a-knot interpolating cubic) is
    sum_p c[j][k][p] (m - m_j)^p, so that interp1d(m, r)(x) = sum_k r_k L_k(x)."""
    from scipy.interpolate import make_interp_spline
    n = len(masses)
    out = np.empty((n - 1, n, 4))
    for k in range(n):
        spl = make_interp_spline(masses, np.eye(n)[k], k=3)
        for p, fact in enumerate((1.0, 1.0, 2.0, 6.0)):
            out[:, k, p] = spl(masses[:-1], nu=p) / fact
    return out


def eval_cardinal(card, rk, m, masses=WOOD_MASSES):
    """numpy form of the device's evaluation (lfg_physpar.hpp, pp_wood)"""
    m = np.asarray(m, dtype=np.float64)
    j = np.clip(((m - masses[0]) * 10.0).astype(int), 0, len(masses) - 2)
    d = m - masses[j]
    c = np.einsum("k,...kp->...p", np.asarray(rk, dtype=np.float64), card[j])
    return ((c[..., 3] * d + c[..., 2]) * d + c[..., 1]) * d + c[..., 0]


def eval_bispline(tx, ty, c, x, y):
    """numpy de Boor over a FITPACK bicubic (tx, ty, c) at the pairs (x, y):
    the device's evaluation (lfg_physpar.hpp, pp_panei)"""
    def basis(t, v):
        v = np.clip(np.asarray(v, dtype=np.float64), t[3], t[-4])
        l = np.clip(np.searchsorted(t, v, side="right") - 1, 3, len(t) - 5)
        h = np.zeros(v.shape + (4,))
        h[..., 0] = 1.0
        for j in range(1, 4):
            hh = h.copy()
            h[..., 0] = 0.0
            for i in range(1, j + 1):
                thi, tlo = t[l + i], t[l + i - j]
                f = hh[..., i - 1] / (thi - tlo)
                h[..., i - 1] += f * (thi - v)
                h[..., i] = f * (v - tlo)
        return l, h
    x, y = np.broadcast_arrays(x, y)
    lx, hx = basis(tx, x)
    ly, hy = basis(ty, y)
    C = np.asarray(c).reshape(len(tx) - 4, len(ty) - 4)
    z = np.zeros(x.shape)
    for i in range(4):
        for j in range(4):
            z = z + hx[..., i] * hy[..., j] * C[lx - 3 + i, ly - 3 + j]
    return z


class MRTables:
    """The packed mass-radius tables: numpy arrays on the host, uploaded once
    per device, and the struct lfg_mr_tables that names them."""

    def __init__(self, wood, hamada, panei, constants, wood_cut):
        self.constants = dict(constants)
        self.wood = wood                       # [(T, R)] per file
        self.wood_cut = tuple(wood_cut)        # rows cut at each file's hot end
        self.wood_off = np.concatenate([[0], np.cumsum([len(t) for t, _ in wood])]).astype(np.int32)
        self.arrays = {
            "wood_t": np.concatenate([t for t, _ in wood]), "wood_r": np.concatenate([r for _, r in wood]),
            "wood_card": np.ascontiguousarray(cardinal_cubics().reshape(-1)),
            "ham_m": np.ascontiguousarray(hamada[0]), "ham_r": np.ascontiguousarray(hamada[1]),
            "pan_tx": np.ascontiguousarray(panei[0]), "pan_ty": np.ascontiguousarray(panei[1]),
            "pan_c": np.ascontiguousarray(panei[2]),
        }
        self.panei_data = panei[3]             # (teff, mass, radius) as read
        nx, ny = len(panei[0]), len(panei[1])
        if not (8 <= nx <= _native.MR_MAX_KNOTS and 8 <= ny <= _native.MR_MAX_KNOTS):
            raise ValueError("the Panei spline has %d x %d knots; the kernel takes 8 to %d per axis"
                             % (nx, ny, _native.MR_MAX_KNOTS))
        total = sum(a.size for a in self.arrays.values())
        if total > _native.MR_MAX_DOUBLES:
            raise ValueError("the tables hold %d doubles; the kernel stages at most %d"
                             % (total, _native.MR_MAX_DOUBLES))
        self._dev = {}

    def struct_over(self, ptr):
        """lfg_mr_tables whose array `name` lies at address ptr(name)"""
        T = _native.LfgMrTables()
        for name in self.arrays:
            setattr(T, name, ptr(name))
        T.wood_off = (ctypes.c_int * (_native.MR_NWOOD + 1))(*[int(v) for v in self.wood_off])
        T.n_ham = self.arrays["ham_m"].size
        T.pan_nx, T.pan_ny = self.arrays["pan_tx"].size, self.arrays["pan_ty"].size
        for k, v in self.constants.items():
            setattr(T, k, float(v))
        return T

    def host_struct(self):
        """lfg_mr_tables over the host arrays (lfg_cpu_physpar)"""
        return self.struct_over(lambda n: self.arrays[n].ctypes.data)

    def device_struct(self, device):
        """lfg_mr_tables over this device's copy of the arrays, uploaded on first use"""
        import torch
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._dev:
            dev = torch.device("cuda", key)
            t = {n: torch.as_tensor(a, device=dev) for n, a in self.arrays.items()}
            self._dev[key] = (self.struct_over(lambda n: t[n].data_ptr()), t)
        return self._dev[key][0]


def load_mr_tables(base_dir, constants=None):
    """Read the reference's directory layout under base_dir: Wood95/co*.2.04dt1,
    Hamada/mr_hamada.dat and Panei/12C-MR-H-He/12C-MR-H-He.dat (or .saver, the
    name the reference ships the table under; .dat first).  A missing file
    raises FileNotFoundError."""
    from scipy.interpolate import SmoothBivariateSpline
    const = dict(CONSTANTS, **(constants or {}))
    rsun_cm = const["Rsun"] * 100.0
    wood, cut = [], []
    for f in WOOD_FILES:
        path = os.path.join(base_dir, f)
        if not os.path.isfile(path):
            raise FileNotFoundError(path)
        t, r, c = read_wood_file(path, rsun_cm)
        wood.append((t, r))
        cut.append(c)
    path = os.path.join(base_dir, HAMADA_FILE)
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    hm, hr = np.loadtxt(path, usecols=(0, 5)).T
    order = np.argsort(hm, kind="stable")      # interp1d sorts
    hm, hr = hm[order], hr[order] / 100.0
    lo, hi = BRACKETS["hamada"]
    if np.any(np.diff(hm) <= 0.0) or hm[0] > lo or hm[-1] < hi:
        raise ValueError("%s: masses must be distinct and cover [%g, %g]" % (path, lo, hi))
    found = [p for p in (os.path.join(base_dir, f) for f in PANEI_FILES) if os.path.isfile(p)]
    if not found:
        raise FileNotFoundError(os.path.join(base_dir, PANEI_FILES[0]))
    teff, mass, radius = np.loadtxt(found[0]).T
    teff, radius = 1000.0 * teff, radius / 100.0
    spl = SmoothBivariateSpline(teff, mass, radius)
    tx, ty = spl.get_knots()
    return MRTables(wood, (hm, hr), (np.array(tx), np.array(ty), np.array(spl.get_coeffs()), (teff, mass, radius)),
                    const, cut)


def _device(device):
    import torch
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())


def _launch(qt, dt, rt, ld, twd, p, n, tables, out, model, status, dev):
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    T = tables.device_struct(dev)
    rc = _native.lib().lfg_physpar(vp(qt), vp(dt), vp(rt), int(ld), vp(twd), vp(p), int(n), ctypes.byref(T),
                                   vp(out), vp(model), vp(status), _native.stream_ptr(dev))
    _native.check(rc, "lfg_physpar")


def solve(q, dphi, rwd, twd, p, tables, device=None):
    """(table [n, 10] in COLUMNS' order, model [n], status [n]) as tensors on
    the device.  Inputs: arrays or tensors of one length (scalars broadcast);
    twd in K, p in days.  A row whose status is not 0 is NaN with model -1."""
    import torch
    _native.require_gpu()
    dev = _device(device)
    cols = [torch.as_tensor(a, dtype=torch.float64, device=dev).reshape(-1) for a in (q, dphi, rwd, twd, p)]
    n = max(c.numel() for c in cols)
    cols = [c.expand(n).contiguous() if c.numel() == 1 and n != 1 else c.contiguous() for c in cols]
    if any(c.numel() != n for c in cols):
        raise ValueError("q, dphi, rwd, twd and p must have one length")
    out = torch.empty((len(COLUMNS), n), dtype=torch.float64, device=dev)
    model = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for lo in range(0, n, MAX_ROWS):
            k = min(MAX_ROWS, n - lo)
            if lo == 0 and k == n:
                o = out
            else:  # a chunk's [10][k] block, copied into place afterwards
                o = torch.empty((len(COLUMNS), k), dtype=torch.float64, device=dev)
            _launch(cols[0][lo:], cols[1][lo:], cols[2][lo:], 1, cols[3][lo:], cols[4][lo:], k, tables, o,
                    model[lo:], status[lo:], dev)
            if o is not out:
                out[:, lo:lo + k] = o
    return out.t(), model, status


def find_wdmass(q, rwd, twd, p, tables, device=None):
    """The white-dwarf mass [M_sun] alone (NaN where no relation brackets
    one) and the model that gave it: the reference's find_wdmass through its
    wood / panei / hamada cascade."""
    import torch
    dev = _device(device)
    q = torch.as_tensor(q, dtype=torch.float64, device=dev).reshape(-1)
    # the mass does not depend on dphi: a narrow eclipse, which every q admits, stands in for it
    table, model, status = solve(q, torch.full_like(q, 0.01), rwd, twd, p, tables, device=dev)
    return table[:, 1].clone(), model, status


def from_chain(chain, names, twd, e_twd, p, e_p, tables, thin=1, seed=0, device=None):
    """Physical parameters of every (thinned) sample of a chain.

    chain: S.chain_dev [steps][W][ndim], a host chain of that shape, or a
    flat chain [rows][ndim]; tensors or arrays.  names: the parameter names
    of the last axis (the chain file's header); q_core, dphi_core and rwd_core
    are found by name and read in place through the row stride (a flat chain
    thinned by rows: ld = thin * ndim; a [steps][W][ndim] chain is thinned by
    steps, as the reference's flatchain does, and for thin > 1 its three
    columns are gathered first).  twd and p are drawn per sample as normals
    (twd, e_twd) and (p, e_p) on the device from a torch.Generator seeded with
    `seed`: the reference draws them with an unseeded np.random.normal, so
    its draws cannot be reproduced, only their distribution.  Chains longer
    than 2^31 - 1 rows are cut into chunks.  Returns solve()'s triple."""
    import torch
    _native.require_gpu()
    dev = _device(device)
    names = list(names)
    idx = [names.index(k) for k in ("q_core", "dphi_core", "rwd_core")]
    c = torch.as_tensor(chain, dtype=torch.float64)
    if c.device != dev:
        c = c.to(dev)
    if c.dim() not in (2, 3) or c.shape[-1] < max(idx) + 1:
        raise ValueError("chain must be [steps][W][ndim] or [rows][ndim] with the named columns")
    thin = int(thin)
    if thin < 1:
        raise ValueError("thin must be at least 1")
    ndim = c.shape[-1]
    if c.dim() == 3 and thin > 1:
        c = c[::thin][:, :, idx].reshape(-1, 3).contiguous()
        idx, ndim, thin = [0, 1, 2], 3, 1
    c = c.contiguous().reshape(-1, ndim)
    n = (c.shape[0] + thin - 1) // thin
    ld = thin * ndim
    flat = c.reshape(-1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))

    def draw(mean, sd, k):
        if float(sd) == 0.0:
            return torch.full((k,), float(mean), dtype=torch.float64, device=dev)
        return torch.normal(float(mean), float(sd), (k,), generator=gen, dtype=torch.float64, device=dev)

    out = torch.empty((len(COLUMNS), n), dtype=torch.float64, device=dev)
    model = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for lo in range(0, n, MAX_ROWS):
            k = min(MAX_ROWS, n - lo)
            t_k, p_k = draw(twd, e_twd, k), draw(p, e_p, k)
            o = out if k == n else torch.empty((len(COLUMNS), k), dtype=torch.float64, device=dev)
            base = lo * ld
            _launch(flat[base + idx[0]:], flat[base + idx[1]:], flat[base + idx[2]:], ld, t_k, p_k, k, tables, o,
                    model[lo:], status[lo:], dev)
            if o is not out:
                out[:, lo:lo + k] = o
    return out.t(), model, status


def summary(table, status):
    """Per column, the mean and the ddof = 1 standard deviation over the
    solved rows (status 0), as the reference's pandas .mean() / .std(), and
    the solved fraction: {"columns", "mean", "std", "solved", "n", "fraction"}."""
    import torch
    table, status = torch.as_tensor(table), torch.as_tensor(status)
    ok = status == 0
    rows = table[ok.to(table.device)]
    k, n = int(rows.shape[0]), int(status.numel())
    mean = rows.mean(dim=0) if k else torch.full((len(COLUMNS),), float("nan"), dtype=torch.float64)
    std = rows.std(dim=0, unbiased=True) if k > 1 else torch.full((len(COLUMNS),), float("nan"), dtype=torch.float64)
    return {"columns": COLUMNS, "mean": mean.cpu().numpy(), "std": std.cpu().numpy(), "solved": k, "n": n,
            "fraction": (k / n) if n else float("nan")}


def summary_lines(s):
    """the reference's summary format, one line per column"""
    return ["{:>5s}: {:.5f} +/- {:.5f}".format(c, m, e) for c, m, e in zip(s["columns"], s["mean"], s["std"])]


def write_results(table, status, directory=".", stats=None):
    """physicalparams.log (a header line `q Mw Rw logg Mr Rr a Kw Kr incl`,
    then one space-separated row per solved sample) and
    physicalparams_summary.log (summary_lines) in `directory`.  The table
    file follows astropy's basic ascii writer as closely as can be said
    without astropy (shortest round-trip decimals): its exact bytes against
    astropy's are unpinned.  Returns the two paths."""
    import pandas as pd
    import torch
    table, status = torch.as_tensor(table), torch.as_tensor(status)
    rows = table[(status == 0).to(table.device)].cpu().numpy()
    log = os.path.join(directory, "physicalparams.log")
    pd.DataFrame(rows, columns=list(COLUMNS)).to_csv(log, sep=" ", index=False)
    stats = stats or summary(table, status)
    path = os.path.join(directory, "physicalparams_summary.log")
    with open(path, "w") as fh:
        for line in summary_lines(stats):
            fh.write(line + "\n")
    return log, path
