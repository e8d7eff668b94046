#!/usr/bin/env python3
"""Generate tests/golden/physpar_ref.npz from the reference's own
calcPhysicalParams.py.

    python tools/make_physpar_golden.py REFERENCE_DIR

Runs only where a checkout of the reference is at hand (it imports
REFERENCE_DIR/calcPhysicalParams.py; nothing of the reference travels).  The reference's
third-party imports are replaced by stand-ins, in the manner of
tools/make_golden.py:
  seaborn, mcmc_utils   empty stubs (only the script part uses them)
  trm.roche             xl1 / findi -> this repo's CPU oracle
  astropy               a minimal quantity class: a value and a unit that
                        carries an SI scale factor and dimensions, with the
                        constants MODEL_SPEC 12.1 states (G, GM_sun, R_sun,
                        the day); astropy itself is absent
It runs the reference's solve() on the fixed batch of tests/physpar_double.py
against a temporary copy of tests/golden/wd_models in which the Panei table
has the name the code opens (.dat), and records the inputs, the ten columns,
the rows that returned None and the rows on which it raised.

So the fixture pins the reference's composition with the constants we state:
the cascade's order, the brackets, the Panei gate, logg's legacy constants
and the column order.  It does not pin astropy's constants or arithmetic.
"""
import importlib.util
import os
import shutil
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "physpar_ref.npz")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from oracle.oracle import Oracle  # noqa: E402
from tests import physpar_double as ppd  # noqa: E402

ORC = Oracle()
C = ppd.CONST


# ------------------------------------------------------------------ astropy
def _dims(a, b, sign):
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0.0) + sign * v
    return {k: v for k, v in out.items() if abs(v) > 1e-12}


class Unit:
    __array_ufunc__ = None   # numpy leaves `array * unit` to __rmul__

    def __init__(self, scale, dims):
        self.scale, self.dims = float(scale), dict(dims)

    def __mul__(self, o):
        if isinstance(o, Unit):
            return Unit(self.scale * o.scale, _dims(self.dims, o.dims, 1))
        return Quantity(o, self)

    __rmul__ = __mul__

    def __truediv__(self, o):
        if isinstance(o, Unit):
            return Unit(self.scale / o.scale, _dims(self.dims, o.dims, -1))
        return Quantity(1.0 / np.asarray(o, dtype=float), self)

    def __pow__(self, p):
        return Unit(self.scale ** p, {k: v * p for k, v in self.dims.items()})

    def same(self, o):
        return not _dims(self.dims, o.dims, -1)


ONE = Unit(1.0, {})


class Quantity:
    __array_ufunc__ = None

    def __init__(self, value, unit):
        if isinstance(value, Quantity):
            value, unit = value.value, value.unit * unit
        self.value = np.asarray(value, dtype=float) if np.ndim(value) else float(value)
        self.unit = unit

    def __array__(self, dtype=None, copy=None):
        return np.asarray(self.value, dtype=dtype)

    def __float__(self):
        return float(self.value)

    def __len__(self):
        return len(self.value)

    def __getitem__(self, k):
        return Quantity(self.value[k], self.unit)

    def to(self, unit):
        assert self.unit.same(unit), (self.unit.dims, unit.dims)
        return Quantity(self.value * (self.unit.scale / unit.scale), unit)

    def _pair(self, o):
        if isinstance(o, Quantity):
            return o.value, o.unit
        if isinstance(o, Unit):
            return 1.0, o
        return o, ONE

    def __mul__(self, o):
        v, u = self._pair(o)
        return Quantity(self.value * v, self.unit * u)

    __rmul__ = __mul__

    def __truediv__(self, o):
        v, u = self._pair(o)
        return Quantity(self.value / v, self.unit / u)

    def __rtruediv__(self, o):
        return Quantity(o / self.value, ONE / self.unit)

    def __pow__(self, p):
        return Quantity(self.value ** p, self.unit ** p)

    def _cmp(self, o):
        return o.to(self.unit).value if isinstance(o, Quantity) else o

    def __ge__(self, o):
        return self.value >= self._cmp(o)

    def __lt__(self, o):
        return self.value < self._cmp(o)


def install_standins():
    for name in ("seaborn",):
        sys.modules[name] = types.ModuleType(name)
    mu = types.ModuleType("mcmc_utils")
    mu.readchain_dask = mu.readflatchain = mu.flatchain = None
    sys.modules["mcmc_utils"] = mu
    trm = types.ModuleType("trm")
    trm.roche = types.SimpleNamespace(xl1=ORC.xl1, findi=ORC.findi)
    sys.modules["trm"] = trm
    sys.modules["trm.roche"] = trm.roche

    m, kg, s, K = (Unit(1.0, {d: 1.0}) for d in ("m", "kg", "s", "K"))
    units = types.ModuleType("astropy.units")
    units.K, units.m, units.s, units.kg = K, m, s, kg
    units.cm, units.km = Unit(1e-2, m.dims), Unit(1e3, m.dims)
    units.d = Unit(C["day"], s.dims)
    units.R_sun = Unit(C["Rsun"], m.dims)
    units.M_sun = Unit(C["GMsun"] / C["G"], kg.dims)
    const = types.ModuleType("astropy.constants")
    const.G = Quantity(C["G"], m ** 3 / kg / s ** 2)
    const.R_sun = Quantity(C["Rsun"], m)
    table = types.ModuleType("astropy.table")
    table.Table = object
    console = types.ModuleType("astropy.utils.console")
    console.ProgressBar = object
    utils = types.ModuleType("astropy.utils")
    utils.console = console
    astropy = types.ModuleType("astropy")
    astropy.constants, astropy.units, astropy.table, astropy.utils = const, units, table, utils
    sys.modules.update({"astropy": astropy, "astropy.constants": const, "astropy.units": units,
                        "astropy.table": table, "astropy.utils": utils, "astropy.utils.console": console})
    return units


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "calcPhysicalParams.py")):
        sys.exit("usage: make_physpar_golden.py REFERENCE_DIR (the directory that holds calcPhysicalParams.py)")
    units = install_standins()
    spec = importlib.util.spec_from_file_location("ref_calcPhysicalParams",
                                                  os.path.join(sys.argv[1], "calcPhysicalParams.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    b = ppd.fixed_batch(ORC)
    n = len(b["q"])
    table = np.full((n, 10), np.nan)
    none, raised = np.zeros(n, bool), np.zeros(n, bool)
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "wd_models")
        shutil.copytree(ppd.WD_MODELS, base)
        pdir = os.path.join(base, "Panei", "12C-MR-H-He")
        shutil.copy(os.path.join(pdir, "12C-MR-H-He.saver"), os.path.join(pdir, "12C-MR-H-He.dat"))
        for i in range(n):
            row = (b["q"][i], b["dphi"][i], b["rw"][i], b["T"][i] * units.K, b["P"][i] * units.d)
            try:
                with np.errstate(all="ignore"):
                    got = ref.solve(row, base + os.sep)
            except FileNotFoundError:
                raise
            except Exception:
                raised[i] = True
                continue
            if got is None:
                none[i] = True
            else:
                table[i] = [float(getattr(v, "value", v)) for v in got]
            if i % 200 == 0:
                print("row %d of %d" % (i, n), flush=True)
    np.savez_compressed(OUT, q=b["q"], dphi=b["dphi"], rw=b["rw"], T=b["T"], P=b["P"], table=table, none=none,
                        raised=raised)
    print("wrote %s: %d rows, %d solved, %d None, %d raised" % (OUT, n, int(np.isfinite(table[:, 1]).sum()),
                                                              int(none.sum()), int(raised.sum())))


if __name__ == "__main__":
    main()
