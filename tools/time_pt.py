"""Device timing of one parallel-tempered iteration against the model cost
alone (recorded, not asserted).

    python tools/time_pt.py [--temps 8] [--walkers 1024] [--iters 50] [--rounds 5] [--out profiles/pt/time_pt.json]

On config 2's tree (one eclipse, complex bright spot, 300 points) it times,
with device events over `iters` iterations per round after a warm-up, the
rounds of the five measurements alternating in one process:
  pt_iteration     PTSampler.step(): 2 x (lfg_pt_propose, lfg_lnprob with
                   lnlike_e on T W/2 proposals, lfg_pt_accept) + lfg_pt_swap
  lnprob_pair      two plain lfg_lnprob calls on T W/2 walkers: the model
                   cost a run of that many walkers pays without tempering
  lnprob_pair_lle  the same two calls with the lnlike_e output
  moves            2 x (lfg_pt_propose + lfg_pt_accept), no model
  swap             lfg_pt_swap alone (its three kernels)
overhead = pt_iteration - lnprob_pair is the tempering machinery's cost.
`moves` and `swap` are launch-and-kernel times only: they run on a copy of
the state with the last real iteration's proposals and ln_prob as stand-ins,
so their acceptance rates are not a real run's (the JSON says so too), and
they reach into the sampler's private buffers to do it.
The parent process never opens the GPU: the measurement runs in a child
under its own time limit, and nothing follows a child that failed.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args):
    import numpy as np
    import torch
    from lfit_python_amd import batch, sampler, synthetic
    from lfit_python_amd.lfit import flux_batch

    dev = torch.device("cuda", 0)

    def flux_fn(pars, x, w, nsub):
        f, st = flux_batch(np.asarray(pars)[None, :], x, w, nsub=nsub, device=dev)
        return f[0].cpu().numpy()

    T, W = args.temps, args.walkers
    n = T * (W // 2)
    model = synthetic.config_single(npts=300, flux_fn=flux_fn)
    tree = batch.compile_tree(model)
    ev = batch.LnProbEvaluator(tree, device=dev, max_walkers=T * W)
    p = np.array(model.dynasty_par_vals)
    lnprob = lambda x: ev(torch.as_tensor(x, device=dev)).cpu().numpy()  # noqa: E731
    p0 = sampler.initialise_walkers(p, 1e-3, T * W, lnprob, seed=0).reshape(T, W, -1)
    S = sampler.PTSampler(W, tree.ndim, ev, ntemps=T, seed=0)
    S.run_mcmc(p0, args.warmup, storechain=False)
    x = S.pos[:, :W // 2].reshape(n, tree.ndim).contiguous()   # T W/2 walkers of the warmed-up ensemble
    out = torch.empty(n, dtype=torch.float64, device=dev)
    lle = torch.empty((n, tree.E), dtype=torch.float64, device=dev)

    # `moves` and `swap` run on a copy of the state (with the last iteration's
    # proposals and ln_prob as stand-ins), so the sampled ensemble stays valid
    c = dict(pos=S._pos.clone(), alt=S._alt.clone(), lnl=S._lnl.clone(), lnpr=S._lnpr.clone(),
             nacc=S._naccept.clone(), nswap=S._nswap.clone(), step=1 << 40)

    def moves():
        for half in (0, 1):
            S.ops.propose(c["pos"], half, S.a, S.seed, c["step"], S.q, S.zfac)
            S.ops.accept(c["pos"], c["lnl"], c["lnpr"], half, S._betas, S.q, S.zfac, S.lnp_new, S.lle, S.seed,
                         c["step"], c["nacc"])
        c["step"] += 1

    def swap():
        S.ops.swap(c["pos"], c["alt"], c["lnl"], c["lnpr"], S._betas, S.seed, c["step"], c["nswap"])
        c["pos"], c["alt"] = c["alt"], c["pos"]
        c["step"] += 1

    def pair(lle_out):
        ev(x, out=out, lnlike_e=lle_out)
        ev(x, out=out, lnlike_e=lle_out)

    kinds = [("pt_iteration", S.step), ("lnprob_pair", lambda: pair(None)), ("lnprob_pair_lle", lambda: pair(lle)),
             ("moves", moves), ("swap", swap)]
    for _, f in kinds:   # every shape warmed up
        f()
    torch.cuda.synchronize()
    us = {k: [] for k, _ in kinds}
    for _ in range(args.rounds):
        for k, f in kinds:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                f()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / args.iters)
    med = {k: float(np.median(v)) for k, v in us.items()}
    over = med["pt_iteration"] - med["lnprob_pair"]
    res = {"device": torch.cuda.get_device_name(0), "tree": "config 2 (1 eclipse, 18 parameters, 300 points)",
           "ntemps": T, "nwalkers": W, "proposals_per_half": n, "iters_per_round": args.iters, "rounds": args.rounds,
           "warmup_iterations": args.warmup, "median_us": med,
           "range_us": {k: [float(min(v)), float(max(v))] for k, v in us.items()},
           "overhead_us": over, "overhead_share": over / med["pt_iteration"],
           "note": "moves and swap run on a copy of the state with stale proposals and ln_prob as stand-ins: "
                   "kernel and launch time only, their acceptance rates are not a real run's",
           "betas": S.betas.tolist(), "acceptance": S.acceptance_fraction.mean(1).tolist()}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--temps", type=int, default=8)
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="time limit of the measuring child, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pt", "time_pt.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("the measuring step failed (exit status %d): nothing written" % r.returncode)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    m = res["median_us"]
    print("T = %d, W = %d: PT iteration %.1f us, two plain lfg_lnprob calls on %d walkers %.1f us (with lnlike_e %.1f), "
          "overhead %.1f us = %.1f %% (moves %.1f us, swap %.1f us) -> %s"
          % (res["ntemps"], res["nwalkers"], m["pt_iteration"], res["proposals_per_half"], m["lnprob_pair"],
             m["lnprob_pair_lle"], res["overhead_us"], 100 * res["overhead_share"], m["moves"], m["swap"], args.out))


if __name__ == "__main__":
    main()
