"""The white dwarf's limb-darkening coefficients per band, on the device
(MODEL_SPEC.md section 15; the reference's limbdark.py, the tables of
Gianninas et al. 2013).

    tables = load_ld_tables(base_dir)             Gianninas13/ld_coeffs_<band>.txt
    table, status = coefficients(logg, teff, tables)
    table, status = from_chain(chain_wd, names, tables)    every row of a wdparams chain
    table, status = from_normal(8.1, 0.05, 14300., 300., tables, size=100000)
    s = summary(table, status); summary_lines(s); update_input("mcmc_input.dat", ...)

    python -m lfit_python_amd.limbdark --dir TABLES (--chain chain_wd.txt [--nskip N --thin N] |
        LOGG GERR TEFF TERR) [--size 100] [--seed 0] [--update mcmc_input.dat]

Every row goes through lfg_limbdark (include/lfg_limbdark.h), one lane per
row: 25 bicubic splines with shared knots, column band * 5 + coef.  The
medians and spreads come from chainstats.stats on the table where it lies.
The host's part is reading the five tables and fitting the splines (numpy,
scipy), once.  The reference's ld() re-reads a table and rebuilds a spline on
every call and looks at 100 unseeded draws.
"""
import argparse
import ctypes
import os
import re
import sys

import numpy as np

from . import _native

BANDS = ("u", "g", "r", "i", "z")
COEFS = ("linear", "quad_a", "quad_b", "sqr_d", "sqr_f")   # table columns 2 ... 6
COLUMNS = tuple("%s_%s" % (b, c) for b in BANDS for c in COEFS)
LAW_COEFS = {"linear": (0,), "quad": (1, 2), "sqr": (3, 4)}
TABLE_FILE = "Gianninas13/ld_coeffs_%s.txt"
ST_OK, ST_BAD_ARGS, ST_CLAMPED = 0, 5, _native.ST_LD_CLAMPED
MAX_ROWS = 2 ** 31 - 1  # rows of one lfg_limbdark call (int n)
LINE_FORMATS = ("%s band LD coeff = %f +/- %f", "%s band quad coeff a = %f +/- %f",
                "%s band quad coeff b = %f +/- %f", "%s band sqr coeff d = %f +/- %f",
                "%s band sqr coeff f = %f +/- %f")
SEPARATOR = "-------------------"


class LDTables:
    """The packed tables: the nodes and values as read (logg [ng], teff [nt],
    values [25, ng, nt]), the shared FITPACK knots tx, ty and the coefficients
    c [25, (nx-4)(ny-4)] on the host, uploaded once per device, and the struct
    lfg_ld_tables that names them."""

    def __init__(self, logg, teff, values, tx, ty, c):
        self.logg, self.teff, self.values = logg, teff, values
        self.arrays = {"tx": np.ascontiguousarray(tx, dtype=np.float64),
                       "ty": np.ascontiguousarray(ty, dtype=np.float64),
                       "c": np.ascontiguousarray(c, dtype=np.float64)}
        nx, ny = self.arrays["tx"].size, self.arrays["ty"].size
        if not (8 <= nx <= _native.LD_MAX_KNOTS and 8 <= ny <= _native.LD_MAX_KNOTS):
            raise ValueError("the splines have %d x %d knots; the kernel takes 8 to %d per axis"
                             % (nx, ny, _native.LD_MAX_KNOTS))
        if self.arrays["c"].shape != (_native.LD_NCOL, (nx - 4) * (ny - 4)):
            raise ValueError("the coefficients must be [%d][(nx-4)(ny-4)]" % _native.LD_NCOL)
        self.c_max = float(np.max(np.abs(self.arrays["c"])))
        self._dev = {}

    tx = property(lambda self: self.arrays["tx"])
    ty = property(lambda self: self.arrays["ty"])
    c = property(lambda self: self.arrays["c"])

    def struct_over(self, ptr):
        """lfg_ld_tables whose array `name` lies at address ptr(name)"""
        return _native.LfgLdTables(ptr("tx"), ptr("ty"), self.arrays["tx"].size, self.arrays["ty"].size, ptr("c"))

    def host_struct(self):
        """lfg_ld_tables over the host arrays (lfg_cpu_limbdark)"""
        return self.struct_over(lambda n: self.arrays[n].ctypes.data)

    def device_struct(self, device):
        """lfg_ld_tables over this device's copy of the arrays, uploaded on first use"""
        import torch
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._dev:
            dev = torch.device("cuda", key)
            t = {n: torch.as_tensor(a, device=dev) for n, a in self.arrays.items()}
            self._dev[key] = (self.struct_over(lambda n: t[n].data_ptr()), t)
        return self._dev[key][0]

    def eval_numpy(self, logg, teff):
        """[n, 25]: the device's evaluation in numpy (physpar.eval_bispline per surface)"""
        from .physpar import eval_bispline
        logg, teff = np.broadcast_arrays(np.asarray(logg, dtype=np.float64).reshape(-1),
                                         np.asarray(teff, dtype=np.float64).reshape(-1))
        return np.stack([eval_bispline(self.tx, self.ty, c, logg, teff) for c in self.c], axis=1)


def read_table(path):
    """One ld_coeffs_<band>.txt: (logg [ng], teff [nt], values [5, ng, nt]).
    ValueError unless the rows are a full rectangular grid, logg-major."""
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    data = np.loadtxt(path, ndmin=2)
    if data.shape[1] < 2 + len(COEFS):
        raise ValueError("%s: %d columns, expected logg, teff and %d coefficients" % (path, data.shape[1], len(COEFS)))
    g1, t1 = np.unique(data[:, 0]), np.unique(data[:, 1])
    ng, nt = len(g1), len(t1)
    if (len(data) != ng * nt or not np.array_equal(data[:, 0], np.repeat(g1, nt))
            or not np.array_equal(data[:, 1], np.tile(t1, ng))):
        raise ValueError("%s: %d rows are not a full %d x %d (logg x teff) grid, logg-major" % (path, len(data), ng, nt))
    return g1, t1, np.ascontiguousarray(data[:, 2:2 + len(COEFS)].T).reshape(len(COEFS), ng, nt)


def load_ld_tables(base_dir):
    """Read base_dir/Gianninas13/ld_coeffs_{u,g,r,i,z}.txt and fit the 25
    interpolating bicubics the reference's ld() fits, RectBivariateSpline(kx=3,
    ky=3).  A missing file raises FileNotFoundError naming it; a file that is
    not a full grid, or five files whose grids differ, ValueError."""
    from scipy.interpolate import RectBivariateSpline
    g1 = t1 = None
    values, knots, coeffs = [], None, []
    for band in BANDS:
        path = os.path.join(base_dir, TABLE_FILE % band)
        g, t, z = read_table(path)
        if g1 is None:
            g1, t1 = g, t
        elif not (np.array_equal(g, g1) and np.array_equal(t, t1)):
            raise ValueError("%s: its (logg, teff) grid differs from %s's" % (path, TABLE_FILE % BANDS[0]))
        values.append(z)
        for k in range(len(COEFS)):
            spl = RectBivariateSpline(g1, t1, z[k], kx=3, ky=3)
            tx, ty = (np.array(a) for a in spl.get_knots())
            if knots is None:
                knots = (tx, ty)
            elif not (np.array_equal(tx, knots[0]) and np.array_equal(ty, knots[1])):
                raise ValueError("%s: the splines do not share their knots" % path)
            coeffs.append(np.array(spl.get_coeffs()))
    return LDTables(g1, t1, np.concatenate(values), knots[0], knots[1], np.stack(coeffs))


def _device(device):
    import torch
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())


def _launch(lg, tf, ld, n, tables, out, status, dev):
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    T = tables.device_struct(dev)
    rc = _native.lib().lfg_limbdark(vp(lg), vp(tf), int(ld), int(n), ctypes.byref(T), vp(out), vp(status),
                                    _native.stream_ptr(dev))
    _native.check(rc, "lfg_limbdark")


def _run(lg, tf, ld, n, tables, dev):
    """rows i = 0 .. n-1 at lg[i * ld], tf[i * ld] (flat device tensors), in chunks of MAX_ROWS"""
    import torch
    out = torch.empty((n, _native.LD_NCOL), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for lo in range(0, n, MAX_ROWS):
            k = min(MAX_ROWS, n - lo)
            _launch(lg[lo * ld:], tf[lo * ld:], ld, k, tables, out[lo:], status[lo:], dev)
    return out, status


def coefficients(logg, teff, tables, device=None):
    """(table [n, 25] in COLUMNS' order, status [n]) as tensors on the device.
    Inputs: arrays or tensors of one length (scalars broadcast).  Status 0, 5
    (a non-finite input: the row is NaN) or 7 (an argument outside the tables:
    the row is the value at the tables' edge)."""
    import torch
    _native.require_gpu()
    dev = _device(device)
    cols = [torch.as_tensor(a, dtype=torch.float64, device=dev).reshape(-1) for a in (logg, teff)]
    n = max(c.numel() for c in cols)
    cols = [c.expand(n).contiguous() if c.numel() == 1 and n != 1 else c.contiguous() for c in cols]
    if any(c.numel() != n for c in cols):
        raise ValueError("logg and teff must have one length")
    return _run(cols[0], cols[1], 1, n, tables, dev)


_default_tables = {}


def ld(band, logg, teff, law="linear", tables=None):
    """The reference's ld(): a float for 'linear', a 2-tuple for 'quad' (a, b)
    and 'sqr' (d, f).  tables: an LDTables (None: the tables beside this
    module, where the reference keeps its own, loaded once)."""
    assert band in ["u", "g", "r", "i", "z"]
    assert law in ["linear", "quad", "sqr"]
    if tables is None:
        here = os.path.dirname(os.path.abspath(__file__))
        if here not in _default_tables:
            _default_tables[here] = load_ld_tables(here)
        tables = _default_tables[here]
    table, _ = coefficients(float(logg), float(teff), tables)
    row = table[0].cpu().numpy()
    vals = tuple(float(row[BANDS.index(band) * len(COEFS) + k]) for k in LAW_COEFS[law])
    return vals[0] if law == "linear" else vals


def _column(names, key):
    found = [i for i, n in enumerate(names) if n.lower().replace("_", "") == key]
    if len(found) != 1:
        raise ValueError("the chain needs exactly one %r column (names: %s)" % (key, ", ".join(names)))
    return found[0]


def from_chain(chain, names, tables, nskip=0, thin=1, device=None):
    """Coefficients of every (thinned) sample of a white-dwarf chain.

    chain: [steps][W][ndim] or a flat chain [rows][ndim], host or device.
    names: the names of the last axis (chain_wd.txt's header: Teff, log_g, ...,
    compared in lower case without underscores); the teff and logg columns are
    read in place through the row stride.  nskip drops leading steps (rows of
    a flat chain).  Thinning follows physpar.from_chain: a flat chain is
    thinned by rows in place (ld = thin * ndim); a [steps][W][ndim] chain by
    steps, and for thin > 1 its two columns are gathered first.  Returns
    coefficients()'s pair."""
    import torch
    _native.require_gpu()
    dev = _device(device)
    names = list(names)
    it, ig = _column(names, "teff"), _column(names, "logg")
    c = torch.as_tensor(chain, dtype=torch.float64)
    if c.device != dev:
        c = c.to(dev)
    if c.dim() not in (2, 3) or c.shape[-1] < max(it, ig) + 1:
        raise ValueError("chain must be [steps][W][ndim] or [rows][ndim] with the named columns")
    thin, nskip = int(thin), int(nskip)
    if thin < 1 or nskip < 0:
        raise ValueError("nskip >= 0 and thin >= 1")
    c = c[nskip:]
    ndim = c.shape[-1]
    if c.dim() == 3 and thin > 1:
        c = c[::thin][:, :, [it, ig]].reshape(-1, 2).contiguous()
        it, ig, ndim, thin = 0, 1, 2, 1
    c = c.contiguous().reshape(-1, ndim)
    n = (c.shape[0] + thin - 1) // thin
    flat = c.reshape(-1)
    return _run(flat[ig:], flat[it:], thin * ndim, n, tables, dev)


def from_normal(logg, gerr, teff, terr, tables, size=100, seed=0, device=None):
    """The reference's main(): `size` pairs (logg, teff) drawn from two
    normals, on the device from a torch.Generator seeded with `seed` (the
    reference's draws are unseeded: only their distribution can be met).  A
    zero error gives constants.  Returns coefficients()'s pair."""
    import torch
    _native.require_gpu()
    dev = _device(device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    size = int(size)

    def draw(mean, sd):
        if float(sd) == 0.0:
            return torch.full((size,), float(mean), dtype=torch.float64, device=dev)
        return torch.normal(float(mean), float(sd), (size,), generator=gen, dtype=torch.float64, device=dev)
    g = draw(logg, gerr)
    t = draw(teff, terr)
    return _run(g, t, 1, size, tables, dev)


def summary(table, status):
    """Per column the median (np.median's value) and the ddof = 0 standard
    deviation over the rows whose status is not BAD_ARGS, from one
    chainstats.stats call on the table where it lies (its non-finite rows are
    the BAD_ARGS rows, which it leaves out): {"columns", "median", "std", "n",
    "n_bad", "clamped"}, clamped the fraction of all rows with status 7."""
    import torch
    from . import chainstats
    status = torch.as_tensor(status)
    n = int(status.numel())
    s = chainstats.stats(table, quantiles=(0.5,))
    # np.median: the middle value of an odd count (ostat's first), the mean of the two middle values of an even one
    with np.errstate(invalid="ignore"):
        median = np.where(s.n % 2 == 1, s.ostat[:, 0, 0], (s.ostat[:, 0, 0] + s.ostat[:, 0, 1]) / 2.0)
    n_clamped = int((status == ST_CLAMPED).sum())
    return {"columns": COLUMNS, "median": median, "std": s.std(0), "n": n, "n_bad": int((status == ST_BAD_ARGS).sum()),
            "clamped": (n_clamped / n) if n else float("nan")}


def summary_lines(s):
    """the reference's main() output: a separator, then per band five lines and a separator"""
    lines = [SEPARATOR]
    for b, band in enumerate(BANDS):
        for k, fmt in enumerate(LINE_FORMATS):
            col = b * len(COEFS) + k
            lines.append(fmt % (band, s["median"][col], s["std"][col]))
        lines.append(SEPARATOR)
    return lines


def linear_medians(s):
    """band -> the linear coefficient's median of a summary()"""
    return {band: float(s["median"][b * len(COEFS)]) for b, band in enumerate(BANDS)}


_ULIMB = re.compile(rb"^(\s*ulimb_(\w+)\s*=)(\s*)(\S+)(\s+)(\S+)(\s+)(\S+)(.*)$", re.S)


def _refit(sep, old, new):
    """`new` in the columns of sep + old, right-aligned, where it fits"""
    width = len(sep) + len(old)
    if len(new) + (1 if sep else 0) <= width:
        return new.rjust(width)
    return sep[:1] + new


def update_input(path, linear_medians, out=None, fmt="%.4f"):
    """Put the linear coefficients back into an mcmc_input.dat.  For every
    `ulimb_<label> = value prior p1 p2 [isVar]` line whose label, lower-cased,
    is a key of linear_medians (a dict band -> value; bands u, g, r, i, z) the
    start value becomes the median, and so does p1 when the prior is gauss.
    Everything else stays byte for byte: the prior's width, isVar, comments,
    other labels (ulimb_KG5 has no table) and every other line.  The new text
    is right-aligned in the old text's columns where it fits.  Written to
    `out` (default: over `path`); returns the labels changed."""
    with open(path, "rb") as fh:
        lines = fh.read().splitlines(keepends=True)
    changed = []
    for k, line in enumerate(lines):
        m = _ULIMB.match(line)
        if not m:
            continue
        label = m.group(2).decode("ascii", "replace")
        if label.lower() not in BANDS or label.lower() not in linear_medians:
            continue
        new = (fmt % float(linear_medians[label.lower()])).encode()
        head, s1, val, s2, prior, s3, p1, rest = m.group(1, 3, 4, 5, 6, 7, 8, 9)
        text = head + _refit(s1, val, new) + s2 + prior
        text += (_refit(s3, p1, new) if prior.lower() == b"gauss" else s3 + p1) + rest
        lines[k] = text
        changed.append(label)
    with open(out or path, "wb") as fh:
        fh.write(b"".join(lines))
    return changed


def read_chain_file(path, device=None):
    """chain_wd.txt as lfit_python_amd.wdparams writes it -> (chain
    [steps][W][ncol], names): the header's names without walker_no, ln_prob
    included, so that a row is the file's row.  With device= the file is
    parsed there (chainparse.read_chain) and the chain is a device tensor; a
    file the parser will not take is read on the host as without it."""
    from . import chainparse, sampler
    if device is not None:
        try:
            return chainparse.read_chain(path, device=device)
        except ValueError:
            pass                              # (bad, ragged or irregular: the host reader decides)
    with open(path) as fh:
        names = fh.readline().split()[1:]
    chain = sampler.read_chain(path)          # [W][steps][ncol]
    return np.ascontiguousarray(chain.transpose(1, 0, 2)), names


def main(argv=None):
    parser = argparse.ArgumentParser(description="Limb-darkening coefficients of a white dwarf per band")
    parser.add_argument("values", nargs="*", type=float, metavar="LOGG GERR TEFF TERR",
                        help="log g, its error, the effective temperature and its error")
    parser.add_argument("--dir", "-d", default=".", help="directory with Gianninas13/")
    parser.add_argument("--chain", help="a chain_wd.txt of lfit_python_amd.wdparams: every row is evaluated")
    parser.add_argument("--nskip", type=int, default=0, help="leading steps of the chain to drop")
    parser.add_argument("--thin", type=int, default=1, help="keep every thin-th step of the chain")
    parser.add_argument("--size", type=int, default=100, help="number of normal draws")
    parser.add_argument("--seed", type=int, default=0, help="seed of the draws")
    parser.add_argument("--update", metavar="mcmc_input.dat",
                        help="put the linear coefficients' medians into this file's ulimb_<band> lines")
    args = parser.parse_args(argv)
    if args.chain and args.values:
        parser.error("give --chain or LOGG GERR TEFF TERR, not both")
    if args.values and len(args.values) != 4:
        parser.error("LOGG GERR TEFF TERR are four numbers")

    tables = load_ld_tables(args.dir)
    if args.chain:
        from . import chainparse
        chain, names = read_chain_file(args.chain, device="cuda" if chainparse.device_available() else None)
        table, status = from_chain(chain, names, tables, nskip=args.nskip, thin=args.thin)
    else:
        if args.values:
            logg, gerr, teff, terr = args.values
        else:
            logg, gerr = (float(v) for v in input("> Give log g and error: ").split())
            teff, terr = (float(v) for v in input("> Give eff. temp. and error: ").split())
        table, status = from_normal(logg, gerr, teff, terr, tables, size=args.size, seed=args.seed)
    s = summary(table, status)
    for line in summary_lines(s):
        print(line)
    if s["clamped"] > 0.0 or s["n_bad"]:
        print("%.2f percent of the %d rows lie outside the tables and were clamped to their edge; "
              "%d non-finite rows were dropped" % (100.0 * s["clamped"], s["n"], s["n_bad"]))
    if args.update:
        changed = update_input(args.update, linear_medians(s))
        print("%s: updated %s" % (args.update, ", ".join("ulimb_" + c for c in changed) or "nothing"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
