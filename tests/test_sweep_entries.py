"""CPU: the entries k_pair's sinks add to the difference arrays
(lfit_python_amd/csrc/lfg_sweep.hpp), as a host program.

tests/sweep_entries_main.cpp includes the header through cpu_baseline/shim
and, for six window sets (exactly tiling; tiling with the joins a unit in the
last place apart; gaps of 0.6 of the spacing; overlap, width 3.5 of the
spacing; zero widths; alternating widths 0.6 / 1.4) and m = 1, 2, 3, 64, 65,
300 and 512 windows, fills one difference array with apply_runs (the
reference) and two with apply_runs_merged: one voting with the lane's own
predicate, so that the merged path runs wherever it applies, and one forced
onto apply_runs_batched.  About 3 600 intervals per (set, m), each with its
mirror as PairSink::wd_disc passes them and alone as PairSink::spot does:
random ones that hang over either side, ones inside one window, ones with an
end on a window's edge, ones that cover every window, ones wholly left or
right of them.  The arrays must be equal integer for integer on [0, m) after
every interval, and the canary in the slots from m on must survive.  The
program also pins kRingOf (lfg_tables.hpp) against the two functions it
replaced, for every item.

The second test builds the same program with the host's address and
undefined-behaviour sanitizers and runs it as that program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sweep_entries_main.cpp")
SETS = ["tiling", "jitter", "gaps", "overlap", "zero", "alternating"]


def _run(tmp_path, flags):
    exe = str(tmp_path / "sweep_entries")
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags +
                   ["-I", os.path.join(ROOT, "cpu_baseline", "shim"), "-I", os.path.join(ROOT, "lfit_python_amd", "csrc"),
                    "-o", exe, SRC], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {ln.split()[0]: tuple(map(int, ln.split()[1:])) for ln in r.stdout.splitlines()}
    assert list(rows) == SETS, r.stdout
    return rows


def _check(rows):
    for name, (n, merged, batched) in rows.items():
        assert n >= 7 * 3000 and merged + batched == n, (name, n, merged, batched)
    # windows that tile or leave gaps never leave the merged path; overlapping
    # ones take both (an element short of two windows has ends of one window)
    assert rows["tiling"][2] == 0 and rows["gaps"][2] == 0 and rows["zero"][2] == 0
    assert rows["overlap"][1] > 1000 and rows["overlap"][2] > 1000


def test_merged_entries_equal_the_reference(tmp_path):
    _check(_run(tmp_path, ["-O2"]))


def test_merged_entries_under_host_sanitizers(tmp_path):
    _check(_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
