"""The summary of a finished chain file: modparams.csv and the before/after
report of the reference's fit_summary (chainstats.fit_summary).

    python -m lfit_python_amd.fit_summary CHAIN INPUT [--nskip N] [--thin K] [--dir D] [--corners]

--corners adds, per eclipse, the corner plot's counts made on the device
(D/Final_figs/<lightcurve>_corners.npz, and .png where matplotlib imports).
The reference draws corner plots by default; here they are opt-in.
"""
import argparse
import sys

from . import chainparse, chainstats, sampler


def main(argv=None):
    ap = argparse.ArgumentParser(description="Summarise a chain file: modparams.csv and the model's report.")
    ap.add_argument("chain", help="a chain file as the MCMC driver writes it (chain_prod.txt)")
    ap.add_argument("input", help="the MCMC parameters' input file of that run")
    ap.add_argument("--nskip", type=int, default=0)
    ap.add_argument("--thin", type=int, default=1)
    ap.add_argument("--dir", default=".", help="where modparams.csv goes")
    ap.add_argument("--corners", action="store_true", help="write the corner plots' data (and figures) per eclipse")
    args = ap.parse_args(argv)
    with open(args.chain) as fh:
        names = fh.readline().split()[1:-1]   # 'walker_no <names> ln_prob'
    chain, walker_major = None, False
    if chainparse.device_available():
        # the file's bytes to the device once, the doubles formed there: [steps][W][npars + 1],
        # the same logical view as the host reader's [W][steps] under walker_major
        try:
            chain = chainparse.read_chain(args.chain, device="cuda")[0]
        except ValueError:
            chain = None                      # (bad, ragged or irregular: the host reader decides)
    if chain is None:
        chain, walker_major = sampler.read_chain(args.chain), True    # [W][steps][npars + 1]
    out = chainstats.fit_summary(chain, names, input_file=args.input, nskip=args.nskip, thin=args.thin,
                                 out_dir=args.dir, walker_major=walker_major, corners=args.corners)
    print("Result of the chain:")
    print(out["result"].to_string())
    print("Wrote {}".format(out["modparams"]))
    for path in out.get("corners", ()):
        print("Wrote {}".format(path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
