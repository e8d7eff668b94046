#!/usr/bin/env python
"""The observed distance of the oracle, the host twin and (with --gpu) the
device from the flux double, over the cases of tests/test_flux_double.py and
tests/test_gpu_flux_double.py: the figures of profiles/flux_double/README.md.

    python tools/flux_double_report.py [--gpu] [--out report.json]

Per implementation: the largest interval and weight difference of the element
tables, and per component the largest |difference| / flux parameter, plainly
and in units of the tests' bound."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_flux_double as t      # noqa: E402
from tests import flux_double as fd          # noqa: E402

COMP = ["total", "wd", "disc", "spot", "donor"]


def fold(seen, got5, ref5, x, w, nsub, pars4):
    for k, name in enumerate(COMP):
        if got5[k] is None:
            continue
        scale = sum(pars4) if k == 0 else pars4[k - 1]
        r, e = t.worst(got5[k], ref5[k], x, w, nsub, scale)
        cur = seen.setdefault(name, [0.0, 0.0])
        cur[0], cur[1] = max(cur[0], e), max(cur[1], r)


def elements(seen, m, a, b, wg, don):
    e = m.ecl
    seen["interval"] = max(seen.get("interval", 0.0), float(np.max(np.abs(a[e] - m.a[e]))),
                           float(np.max(np.abs(b[e] - m.b[e]))))
    seen["weight_rel"] = max(seen.get("weight_rel", 0.0), float(np.max(np.abs(wg / m.w - 1.0))))
    seen["donor_abs"] = max(seen.get("donor_abs", 0.0), float(np.max(np.abs(don - m.donor))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    from oracle.oracle import Oracle
    from cpu_baseline import cpu
    oracle = Oracle()
    if not os.path.exists(cpu.LIB_PATH):
        cpu.build()
    port = cpu.CpuPort()
    rep = {"oracle": {}, "host_twin": {}}
    sizes = [300]
    if args.gpu:
        from lfit_python_amd.lfit import flux_batch
        from tests.test_gpu_flux_double import SIZES, all_pars
        from tests.test_gpu_parity import _elements_gpu
        rep["device"] = {}
        sizes = sorted(set(SIZES + [300]))
        st, a, b, wg, don, _ = _elements_gpu(all_pars())
        for i, name in enumerate(t.NAMES):
            elements(rep["device"], t.the_model(name), a[i], b[i], wg[i], don[i])
    for name in t.NAMES:
        _, a, b, wg, don, _ = oracle.elements(t.records()[name]["pars"])
        elements(rep["oracle"], t.the_model(name), a, b, wg, don)
    for N in sizes:
        for nsub in (1, 3, 5):
            for kind in t.KINDS:
                x, w = t.grid(kind, N)
                if args.gpu and nsub != 5:
                    f, _, c = flux_batch(all_pars(), x, w, nsub=nsub, components=True)
                    f, c = f.cpu().numpy(), c.cpu().numpy()
                for i, name in enumerate(t.NAMES):
                    rec = t.records()[name]
                    ref = fd.light_curve(t.the_model(name), x, w, nsub)
                    p4 = t.flux_params(rec)
                    if args.gpu and nsub != 5:
                        fold(rep["device"], [f[i]] + [c[k, i] for k in range(4)], ref, x, w, nsub, p4)
                    if N == 300:
                        _, got = oracle.flux(rec["pars"], x, w, nsub=nsub, components=True)
                        fold(rep["oracle"], got, ref, x, w, nsub, p4)
                        flux, _ = port.flux(rec["pars"], x, w, nsub=nsub)
                        fold(rep["host_twin"], [flux[0], None, None, None, None], ref, x, w, nsub, p4)
    text = json.dumps(rep, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
