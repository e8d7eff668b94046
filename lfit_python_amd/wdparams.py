"""python -m lfit_python_amd.wdparams wdinput.dat [--summarise] [--no-chain] [--dir TABLES]

The reference's wdparams_new.py on the device (MODEL_SPEC.md section 13):
Bergeron DA model-atmosphere magnitudes are fitted to the white-dwarf fluxes
of an eclipse-fit chain, giving teff, logg, plax and ebv -- the temperature
that python -m lfit_python_amd.calcPhysicalParams asks for.

    table  = load_da_table("Bergeron/Table_DA_sdss")
    fluxes = fluxes_from_chain(flat_chain, names, syserr=0.03)
    model  = WDModel(teff, logg, plax, ebv, fluxes, table)   # tree.Param each
    ev     = WDEvaluator(model)                               # ln_prob on the GPU
    S      = sampler.EnsembleSampler(nwalkers, 4, ev)         # or pt.PTSampler

The reference's interactive prompts are keys of the input file here:
`flux_<band> = value err` adds an observation, `correct_<band> = telescope
instrument filter` applies that colour-correction table to a band, `ntemps`
sets the parallel-tempering ladder (default 10 as the reference; 1 selects
the plain ensemble sampler).  `nthread` is read and ignored.  No plots.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

from . import _native
from .tree import Param

ZP = 3631e3  # AB zero point [mJy]
EXTINCTION = {"u_s": 5.155, "g_s": 3.793, "r_s": 2.751, "i_s": 2.086, "z_s": 1.479, "kg5": 3.5}
NAMES = ["Teff", "log_g", "Parallax", "E(B-V)"]
DA_TABLE = os.path.join("Bergeron", "Table_DA_sdss")
CORRECTION_FILE = os.path.join("color_correction_tables", "color_corrections_HCAM-GTC-super_minus_{}_{}.csv")
INPUT_KEYS = ("fit", "nburn", "nprod", "nwalkers", "scatter", "thin", "flat", "syserr", "chain", "teff", "logg",
              "plax", "ebv", "nthread", "ntemps")


def sdss2kg5(g, r):
    return g - 0.2240 * (g - r) ** 2 - 0.3590 * (g - r) + 0.0460


def sdssmag2flux(mag):
    return ZP * np.power(10.0, -0.4 * np.asarray(mag, dtype=np.float64))


class DATable:
    """A Bergeron grid: loggs [nlogg], teffs [nteff] and each named column as
    [nlogg, nteff] (the file's rows run over teff within each logg)."""

    def __init__(self, names, data):
        self.names = names
        self.loggs = np.unique(data[:, names.index("log_g")])
        self.teffs = np.unique(data[:, names.index("Teff")])
        if len(data) != len(self.loggs) * len(self.teffs):
            raise ValueError("the table is not a full log g x Teff grid")
        self._data = data

    def column(self, name):
        # a repeated heading (J, H appear twice) names its first column, as pandas does
        return self._data[:, self.names.index(name)].reshape(len(self.loggs), len(self.teffs))

    def band(self, band):
        if band == "kg5":
            return sdss2kg5(self.column("g_s"), self.column("r_s"))
        if band not in self.names:
            raise KeyError("the table has no column %r" % band)
        return self.column(band)


def load_da_table(path):
    """Read Bergeron/Table_DA_sdss: a title line, a line of column names, then
    whitespace-separated rows (numpy only)."""
    with open(path, "r") as fh:
        fh.readline()
        names = fh.readline().split()
        data = np.loadtxt(fh, ndmin=2)
    if data.shape[1] != len(names):
        raise ValueError("%s: %d names for %d columns" % (path, len(names), data.shape[1]))
    return DATable(names, data)


class Correction:
    """color_correction_tables/*.csv, one filter's column: the magnitude
    (HiPERCAM/GTC/super - observed), a grid [nteff, nlogg] sorted by Teff,
    then logg."""

    def __init__(self, path, filt):
        with open(path, "r") as fh:
            names = fh.readline().strip().split(",")
            data = np.loadtxt(fh, delimiter=",", ndmin=2)
        if filt not in names:
            raise KeyError("%s has no column %r" % (path, filt))
        self.filt = filt
        self.teffs = np.unique(data[:, names.index("Teff")])
        self.loggs = np.unique(data[:, names.index("logg")])
        self.z = data[:, names.index(filt)].reshape(len(self.teffs), len(self.loggs))


def load_correction(base_dir, telescope, instrument, filt):
    return Correction(os.path.join(base_dir, CORRECTION_FILE.format(telescope, instrument)), filt)


class Flux:
    """One observed flux [mJy] (wdparams_new.py Flux): err takes the
    systematic error in quadrature, mag = 2.5 log10(3631e3 / flux).  With a
    Correction the band is the correction's filter; `band` is then the
    Bergeron column, the '_s' name ('kg5' stays 'kg5')."""

    def __init__(self, val, err, band, syserr=0.03, correction=None):
        self.flux = float(val)
        self.err = float(np.sqrt(float(err) ** 2 + (float(val) * syserr) ** 2))
        self.mag = float(2.5 * np.log10(ZP / self.flux))
        self.magerr = 2.5 * 0.434 * (self.err / self.flux)
        self.correction = correction
        self.orig_band = correction.filt if correction is not None else band
        self.band = self.orig_band if ("_s" in self.orig_band or self.orig_band == "kg5") else self.orig_band + "_s"
        if self.band not in EXTINCTION:
            raise KeyError("no extinction coefficient for band %r" % self.band)

    def __repr__(self):
        return "Flux(%s: %.5f +/- %.5f mJy%s)" % (self.orig_band, self.flux, self.err,
                                                   ", corrected" if self.correction is not None else "")


def sigma_clipped_stats(x, sigma=3.0, maxiters=5):
    """astropy.stats.sigma_clipped_stats at its defaults, restated: up to
    `maxiters` rounds dropping what lies further than sigma standard
    deviations from the median; (mean, median, std) of what survives."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    x = x[np.isfinite(x)]
    for _ in range(maxiters):
        med, std = np.median(x), np.std(x)
        keep = (x >= med - sigma * std) & (x <= med + sigma * std)
        if keep.all():
            break
        x = x[keep]
    return float(np.mean(x)), float(np.median(x)), float(np.std(x))


def fluxes_from_chain(chain, names, syserr=0.03, corrections=None):
    """A Flux per wdFlux_* column of a flat chain [rows, columns] (kg5 columns
    are skipped, as the reference does): the sigma-clipped mean and standard
    deviation.  corrections: {band: Correction}."""
    chain = np.asarray(chain, dtype=np.float64)
    out = []
    for index, key in enumerate(names):
        if "wdflux" not in key.lower() or "kg5" in key.lower():
            continue
        band = key.lower().replace("wdflux_", "")
        mean, _, std = sigma_clipped_stats(chain[:, index])
        out.append(Flux(mean, std, band, syserr=syserr, correction=(corrections or {}).get(band)))
    return out


def _prior_consts(prior):
    """lfg.h's (c0, c1) of one Prior (batch.prior_consts)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        if prior.code <= 1:
            return float(-np.log(np.sqrt(2.0 * np.pi) * prior.p2)), float(1.0 / prior.p2)
        if prior.code == 2:
            return float(np.log(1.0 / abs(prior.p1 - prior.p2))), 0.0
        return float(-np.log(prior.normalise)), 0.0


class WDModel:
    """The fit's model: four Params (teff, logg, plax [mas], ebv), the
    observed Flux list and the Bergeron table.  The splines are packed once
    (scipy's RectBivariateSpline knots and coefficients) and uploaded once per
    device.  Behaves like the list of the current parameter values."""

    def __init__(self, teff, logg, plax, ebv, fluxes, table):
        from scipy.interpolate import RectBivariateSpline
        self.teff, self.logg, self.plax, self.ebv = teff, logg, plax, ebv
        self.variables = [teff, logg, plax, ebv]
        self.obs_fluxes = list(fluxes)
        self.table = table
        self.B = len(self.obs_fluxes)
        if not 1 <= self.B <= _native.WD_MAX_BANDS:
            raise ValueError("%d fluxes: the kernels take 1 to %d bands" % (self.B, _native.WD_MAX_BANDS))
        tx = ty = None
        coef = []
        for f in self.obs_fluxes:
            s = RectBivariateSpline(table.loggs, table.teffs, table.band(f.band), kx=3, ky=3)
            tx, ty, c = s.tck
            coef.append(np.asarray(c, dtype=np.float64))
        self.arrays = {"tx": np.ascontiguousarray(tx, dtype=np.float64),
                       "ty": np.ascontiguousarray(ty, dtype=np.float64), "c": np.concatenate(coef)}
        self._check_knots(self.arrays["tx"], self.arrays["ty"])
        for b, f in enumerate(self.obs_fluxes):
            if f.correction is None:
                continue
            k = f.correction
            cx, cy, cc = RectBivariateSpline(k.teffs, k.loggs, k.z, kx=3, ky=3).tck
            self._check_knots(cx, cy)
            self.arrays.update({"ctx%d" % b: np.ascontiguousarray(cx, dtype=np.float64),
                                "cty%d" % b: np.ascontiguousarray(cy, dtype=np.float64),
                                "cc%d" % b: np.ascontiguousarray(cc, dtype=np.float64)})
        self._dev = {}

    @staticmethod
    def _check_knots(tx, ty):
        if not (8 <= len(tx) <= _native.WD_MAX_KNOTS and 8 <= len(ty) <= _native.WD_MAX_KNOTS):
            raise ValueError("a spline has %d x %d knots; the kernels take 8 to %d per axis"
                             % (len(tx), len(ty), _native.WD_MAX_KNOTS))

    # the reference's list behaviour
    def __getitem__(self, i):
        return self.variables[i].currVal

    def __setitem__(self, i, v):
        self.variables[i].currVal = v

    def __len__(self):
        return len(self.variables)

    npars = property(__len__)

    def struct_over(self, ptr):
        """lfg_wd_model whose array `name` lies at address ptr(name); the
        priors are read from the Params now"""
        M = _native.LfgWdModel()
        M.B, M.nx, M.ny = self.B, self.arrays["tx"].size, self.arrays["ty"].size
        M.tx, M.ty, M.c = ptr("tx"), ptr("ty"), ptr("c")
        lnnorm = 0.0
        for b, f in enumerate(self.obs_fluxes):
            if f.correction is not None:
                M.cnx[b], M.cny[b] = self.arrays["ctx%d" % b].size, self.arrays["cty%d" % b].size
                M.ctx[b], M.cty[b], M.cc[b] = ptr("ctx%d" % b), ptr("cty%d" % b), ptr("cc%d" % b)
            M.k[b], M.mag[b], M.err[b] = EXTINCTION[f.band], f.mag, f.err
            lnnorm += np.log(2.0 * np.pi * f.err ** 2)
        M.lnnorm = float(lnnorm)
        for d, p in enumerate(self.variables):
            M.prior_type[d], M.prior_p1[d], M.prior_p2[d] = p.prior.code, p.prior.p1, p.prior.p2
            M.prior_c0[d], M.prior_c1[d] = _prior_consts(p.prior)
        return M

    def host_struct(self):
        """lfg_wd_model over the host arrays (lfg_cpu_wd_lnprob)"""
        return self.struct_over(lambda n: self.arrays[n].ctypes.data)

    def device_struct(self, device):
        """lfg_wd_model over this device's copy of the arrays, uploaded on first use"""
        import torch
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._dev:
            dev = torch.device("cuda", key)
            t = {n: torch.as_tensor(a, device=dev) for n, a in self.arrays.items()}
            self._dev[key] = (self.struct_over(lambda n: t[n].data_ptr()), t)
        return self._dev[key][0]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class WDEvaluator:
    """ln_prob of walkers [n, 4] on the device (lfg_wd_lnprob), with the
    evaluator surface sampler.EnsembleSampler and pt.PTSampler drive: E = 1
    likelihood term, and step_half, the one-launch half-step
    (lfg_wd_step_half)."""

    E = 1
    generation = 0  # no workspace: a captured graph never goes stale

    def __init__(self, model, device=None):
        import torch
        _native.require_gpu()
        self.L = _native.lib()
        self.model = model
        self.device = (torch.device(device) if device is not None
                       else torch.device("cuda", torch.cuda.current_device()))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.M = model.device_struct(self.device)

    def evaluate(self, x, ld=None, n=None, out=None, lnlike=None, mags=None, status=None):
        """lfg_wd_lnprob over rows of x: [n, ld] or, with ld and n given, a
        flat tensor read in place at row stride ld"""
        import torch
        if ld is None:
            if x.dim() != 2 or x.stride(1) != 1 or x.shape[1] < 4:
                x = x.contiguous()
            n, ld = x.shape[0], (x.stride(0) if x.shape[0] > 1 else max(x.shape[1], 4))
        if x.dtype != torch.float64 or x.device != self.device:
            raise ValueError("x must be a float64 tensor on %s" % self.device)
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=self.device)
        rc = self.L.lfg_wd_lnprob(_vp(x), int(ld), int(n), ctypes.byref(self.M), _vp(out), _vp(lnlike), _vp(mags),
                                  _vp(status), _native.stream_ptr(self.device))
        _native.check(rc, "lfg_wd_lnprob")
        return out

    def __call__(self, x, out=None, lnlike_e=None):
        return self.evaluate(x, out=out, lnlike=lnlike_e)

    def step_half(self, pos, lnp, half, a, seed, step, q, zfac, naccept, lnp_new=None, **kw):
        import torch
        if lnp_new is None:
            lnp_new = torch.empty(pos.shape[0] // 2, dtype=torch.float64, device=self.device)
        rc = self.L.lfg_wd_step_half(_vp(pos), _vp(lnp), pos.shape[0], int(half), float(a), int(seed), int(step),
                                     None, ctypes.byref(self.M), _vp(q), _vp(zfac), _vp(lnp_new), _vp(naccept),
                                     _native.stream_ptr(self.device))
        _native.check(rc, "lfg_wd_step_half")
        return lnp_new

    def chisq(self, x):
        """chi^2 of rows x (from ln_like)"""
        import torch
        ll = torch.empty(x.shape[0], dtype=torch.float64, device=self.device)
        self.evaluate(x, lnlike=ll)
        return -2.0 * ll - self.M.lnnorm


def parse_input(path):
    """The reference's input format: `key = value` lines, # comments.  The
    file is read as bytes: what is not UTF-8 is replaced, not an error."""
    with open(path, "rb") as fh:
        text = fh.read().decode("utf-8", errors="replace")
    out = {}
    for line in text.splitlines():
        line = line.split("#", 1)[0].strip()
        if not line or "=" not in line:
            continue
        k, v = line.split("=", 1)
        out[k.strip()] = v.strip()
    return out


def _read_chain_fluxes(cfg, syserr, corrections):
    from . import mcmc_utils
    chain_file = cfg["chain"]
    print("Reading in the chain file,", chain_file)
    with open(chain_file, "r") as fh:
        line = fh.readline()
        while line.startswith("#"):
            line = fh.readline()
        keys = line.strip().split()[1:]
    if int(cfg.get("flat", 0)):
        from . import chainparse
        fchain = chainparse.try_table(chain_file, skip_lines=1)   # (None: the earlier reader decides)
        if fchain is None:
            fchain = np.loadtxt(chain_file, skiprows=1, ndmin=2)
    else:
        chain = mcmc_utils.readchain(chain_file)
        print("The chain has the {} walkers, {} steps, and {} pars.".format(*chain.shape))
        fchain = mcmc_utils.flatchain(chain, chain.shape[2], thin=int(cfg.get("thin", 1)))
    print("Done!")
    return fluxes_from_chain(fchain, keys[:fchain.shape[1]], syserr, corrections)


def main(argv=None):
    import torch
    from . import pt, sampler
    parser = argparse.ArgumentParser(description="Fit WD Fluxes")
    parser.add_argument("file", help="input file")
    parser.add_argument("--summarise", action="store_true",
                        help="Summarise existing chain file without running a new fit.")
    parser.add_argument("--no-chain", dest="nochain", action="store_true", help="No chain file is being used")
    parser.add_argument("--dir", "-d", default=".", help="directory with Bergeron/ and color_correction_tables/")
    parser.add_argument("--seed", type=int, default=0, help="seed of the walkers' start and the sampler")
    args = parser.parse_args(argv)

    cfg = parse_input(args.file)
    nburn, nprod, nwalkers = int(cfg["nburn"]), int(cfg["nprod"]), int(cfg["nwalkers"])
    scatter, to_fit, syserr = float(cfg["scatter"]), int(cfg["fit"]), float(cfg["syserr"])
    ntemps = int(cfg.get("ntemps", 10))
    pars = [Param.fromString(k, cfg[k]) for k in ("teff", "logg", "plax", "ebv")]

    corrections = {}
    for key, v in cfg.items():
        if key.startswith("correct_"):
            tel, inst, filt = v.split()
            corrections[key[len("correct_"):]] = load_correction(args.dir, tel, inst, filt)
    fluxes = [] if args.nochain else _read_chain_fluxes(cfg, syserr, corrections)
    for key, v in cfg.items():
        if key.startswith("flux_"):
            band = key[len("flux_"):]
            val, err = (float(s) for s in v.split())
            fluxes.append(Flux(val, err, band, syserr=syserr, correction=corrections.get(band)))
    if not fluxes:
        raise SystemExit("no fluxes: give a chain with wdFlux_* columns or flux_<band> keys")

    table_loc = os.path.join(args.dir, DA_TABLE)
    print("--->> I am using the WD model atmosphere table found here: {} <<---".format(table_loc))
    model = WDModel(*pars, fluxes, load_da_table(table_loc))
    ev = WDEvaluator(model)
    dev = ev.device

    def at(values):
        x = torch.tensor([values], dtype=torch.float64, device=dev)
        mags = torch.empty((model.B, 1), dtype=torch.float64, device=dev)
        ev.evaluate(x, mags=mags)
        return mags[:, 0].cpu().numpy(), float(ev.chisq(x)[0])

    mags, chisq = at(list(model))
    print("\n\n\nFor a Teff, logg = {:.0f}, {:.3f}".format(model.teff.currVal, model.logg.currVal))
    print("I generated these magnitudes: {}".format(mags))
    print("This corresponds to the fluxes: {}".format(sdssmag2flux(mags)))
    print("My chisq is {:.3f}".format(chisq))
    print("I'm using the filters:")
    for obs in fluxes:
        print("{:>4s}: Flux {:.3f}+/-{:.3f}".format(obs.orig_band, obs.flux, obs.err))

    flat = None
    if args.summarise:
        chain = sampler.read_chain("chain_wd.txt")
        flat = chain[:, :, :-1].reshape(-1, 4)
    elif to_fit:
        guess = np.array(list(model), dtype=np.float64)

        def ln_prior_ok(p):  # a start needs a finite ln_prob: ln_like is finite wherever ln_prior is
            return ev(torch.as_tensor(p, dtype=torch.float64, device=dev)).cpu().numpy()
        if ntemps > 1:
            p0 = np.stack([sampler.initialise_walkers(guess, scatter, nwalkers, ln_prior_ok, seed=args.seed + t)
                           for t in range(ntemps)])
            S = pt.PTSampler(nwalkers, 4, ev, ntemps=ntemps, seed=args.seed)
            S.run_mcmc(p0, nburn, storechain=False)
            S.reset()
            S.run_mcmc(None, nprod)
            chain, lnpost, _ = S.last_run()
            chain, lnprob = chain[:, 0].numpy(), lnpost[:, 0].numpy()
        else:
            p0 = sampler.initialise_walkers(guess, scatter, nwalkers, ln_prior_ok, seed=args.seed)
            S = sampler.EnsembleSampler(nwalkers, 4, ev, seed=args.seed)
            S.run_mcmc(p0, nburn, storechain=False)
            S.reset()
            S.run_mcmc(None, nprod)
            chain, lnprob = (t.cpu().numpy() for t in S.last_run())
        sampler.write_chain("chain_wd.txt", NAMES, chain, lnprob)
        flat = chain.reshape(-1, 4)

    if flat is not None:
        best = []
        for i in range(4):
            lolim, b, uplim = np.percentile(flat[:, i], [16, 50, 84])
            model[i] = float(b)
            best.append((b, uplim - b, b - lolim))
            print("%s = %f +%f -%f" % (NAMES[i], b, uplim - b, b - lolim))
    print("Done!")
    _, chisq = at(list(model))
    print("Chisq = {:.3f}".format(chisq))
    if flat is not None:
        t, up, lo = best[0]
        print("calcPhysicalParams arguments: twd = {:.0f} e_twd = {:.0f}".format(t, 0.5 * (up + lo)))
        print("  python -m lfit_python_amd.calcPhysicalParams {} {:.0f} {:.0f} <p> <e_p> --dir <WD models>".format(
            cfg.get("chain", "<chain_prod.txt>"), t, 0.5 * (up + lo)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
