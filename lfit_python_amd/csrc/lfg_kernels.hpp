// lfg_kernels.hpp -- everything k_pair is made of: the prelude (block
// constants, the weight block, the sweep permutation), Philox, the sections
// of k_setup, k_elements and k_lnlike (device functions and the k_lnlike
// template; no __global__ definition), k_pair's own section, and the
// declaration of the split launcher.  Needs nothing before it.  Compiled
// twice: by lfg.hip (the host unit; it adds the other kernels, the host code
// and the C ABI) and by lfg_pair_split.hip (without machine LICM, k_pair's
// fold and LONG instantiations only).  Nothing here emits code unless a unit
// instantiates or calls it.
#pragma once

#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "lfg.h"
#include "lfg_device.hpp"
#include "lfg_tables.hpp"
#include "lfg_sweep.hpp"

using namespace lfg;

// k_pair's sinks (LFG_PAIR_SINK_MERGE, default on; -DLFG_PAIR_SINK_MERGE=0
// compiles the code as it was): a run end's adjacent entries are summed
// before they go into the difference array (apply_runs_merged), the sink's
// per-pair constants (1 / disc total, itwd, the two phase indices' origin
// and cell density) are formed once per pair ahead of the barrier B0 and read
// from LDS, not once per wave or per disc lane, and an item's ring comes from
// a table (kRingOf), not from a square root or a division.
#ifndef LFG_PAIR_SINK_MERGE
#define LFG_PAIR_SINK_MERGE 1
#endif

// Diagnostic builds that read device counters back (lfg_debug_*,
// lfg_diag_iters) keep every kernel in lfg.hip's translation unit (see
// lfg_pair_launch_split below): LFG_ONE_TU, by the one rule of lfg_diag.hpp,
// which both units see through this header
#include "lfg_diag.hpp"

namespace {

constexpr int SETUP_BLOCK = 64;
#ifndef LFG_ELEM_BLOCK
#define LFG_ELEM_BLOCK 64  // one wave: the item chunks dispatch at wave granularity (36.0 vs 37.6 us at 256, 36.5 at 128)
#endif
constexpr int ELEM_BLOCK = LFG_ELEM_BLOCK;
#ifndef LFG_ELEM_IPL
#define LFG_ELEM_IPL 1  // items per k_elements lane
#endif
#ifndef ELEM_MINW
#define ELEM_MINW 4  // minimum waves per SIMD of k_elements: <= 128 VGPRs, no spill (at 5 waves / 96 VGPRs the
                     // speculative setup lanes spilled ~100 B/lane; 4 waves measured 3 % faster)
#endif
// per-pair weight block written by k_elements: disc ring weights, the disc
// total 2 pi [P(rdisc) - P(rin)], spot element weights
constexpr int WT_DISC = 0, WT_TD = NDISC_R, WT_BS = 24, WT_N = WT_BS + NBS;
// Eclipse intervals are stored once per mirror pair (MODEL_SPEC 5: the
// mirrored element's interval is [-b, -a]): NU_WDD symmetry-unique WD/disc
// items, then the NBS spot elements, NELU (a, b) pairs per pair in all.  The
// WD/disc slots are in sweep order: slot g holds unique item uitem(g), a
// stride-37 permutation (a wave's lanes sweep items of different rings and
// azimuths, so their LDS atomics spread), and k_lnlike's sweep element g in
// [0, NWD + NDISC) is slot g mod NU_WDD, mirrored for g >= NU_WDD: it reads
// its items as coalesced rows, half the bytes of a table of every element.
constexpr int NU_WDD = (NWD + NDISC) / 2, NELU = NU_WDD + NBS;
__device__ __forceinline__ int uitem(int g) { return (g * 37) % NU_WDD; }
__device__ __forceinline__ int uslot(int u) { return (u * 473) % NU_WDD; }
static_assert(NU_WDD == 700 && (37 * 473) % 700 == 1, "sweep permutation inverse");
__device__ __forceinline__ double2 mirror_ab(double2 ab)
{
    return (ab.x < ab.y) ? make_double2(-ab.y, -ab.x) : make_double2(1.0, -1.0);
}
// sweep element g of a pair's table (g < NWD + NDISC)
__device__ __forceinline__ double2 sweep_ab(const double2* __restrict__ AB, int g)
{
    return (g < NU_WDD) ? AB[g] : mirror_ab(AB[g - NU_WDD]);
}
// per unique donor tile: vx, vy, vz, arc centre, arc half-width (phase units)
constexpr int DON_STRIDE = 5;

#include "lfg_philox.hpp"  // philox, u53, draw (shared with lfg_pt.hip)

// one header per section, in the order they need each other
#include "lfg_k_setup.hpp"     // SetupArgs, Prop, the setup / prior / stream lanes
#include "lfg_k_elements.hpp"  // ElemSpec, ElemOut, MemSink, element_lane, elem_ab
#include "lfg_k_lnlike.hpp"    // LikeArgs, the sweeps, TileBufs, the sub-bin tables, k_lnlike<MODE, SUB>
#include "lfg_k_pair.hpp"  // the section of k_pair (its LONG tables: lfg_k_pair_long.hpp)

}  // namespace

// k_pair's fold and LONG instantiations are compiled in lfg_pair_split.hip:
// the kernels header, compiled a second time without machine LICM (-mllvm
// -disable-machine-licm).
// At the 128-VGPR ceiling the pass hoisted literal constants and cheap loop
// invariants into VGPRs and the register allocator then spilled: LONG's
// point loop reloaded five doubles from scratch per point (48 B per lane,
// 41.6 MB of PMC traffic per config-5 launch), the fold variant 32 B.
// Without it LONG spills 16 B and the fold variant none: config 5
// 3.39 -> 3.52 M evals/s; config 4's one-of-eight fold shard 12.71 -> 12.76
// and 12.36 -> 12.77 M on two boxes (profiles/r06/ab_split_nolicm.txt).  The
// speculative one-tile k_pair (config 2) measured no different and GP trees
// 5 % slower, so they stay in lfg.hip, compiled with the pass.
enum { PAIR_SPLIT_LONG = 0, PAIR_SPLIT_FOLD = 1, PAIR_SPLIT_FOLD_LONG = 2 };
__attribute__((visibility("hidden"))) void lfg_pair_launch_split(int variant, unsigned grid, hipStream_t st,
                                                                   const void* args);
