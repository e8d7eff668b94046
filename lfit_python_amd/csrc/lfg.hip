// lfg.hip -- MI355X (gfx950) kernels and the C ABI of liblfg_hip.so.
//
// Pipeline for one batch of walkers (one emcee half-step), on the caller's
// stream only:
//   k_setup     one lane per (walker, eclipse): parameter gather, L1, findi,
//               strip/beam frame, eclipse Roche priors; one lane per walker:
//               LCModel dphi prior + Prior.ln_prob sum; one lane per
//               (walker, eclipse): the ballistic stream to the disc edge
//   k_elements  one lane per (walker, eclipse, element): eclipse interval of
//               every WD / disc / bright-spot element, donor surface tiles
//   k_lnlike    one workgroup per (walker, eclipse): element tables staged in
//               LDS, lanes stride the phase axis (coalesced), exposure
//               integration, fused chi^2 with a wavefront/LDS reduction
//               and, for the walker's last eclipse, ln_prob = ln_prior + sum_e ln_like_e
// Here: the sections of k_setup, k_elements (with k_expand) and k_lnlike,
// then the host code and extern "C".  In headers, included where they stood:
//   lfg_k_pair.hpp      k_pair (its LONG tables: lfg_k_pair_long.hpp)
//   lfg_k_gp.hpp        k_gp_dcp, k_gp_like, k_combine_walkers, k_combine
//   lfg_k_stretch.hpp   k_propose, k_accept, k_accept_regen, k_apply_verdicts, k_verdict
//   lfg_k_misc.hpp      k_gp, k_wdphases, k_roche; launch_ok, mark_event, run_front
// Replaces, per walker, mcmcfit.ln_prob (mcmcfit.py:37-41) -> Node.ln_prob
// (model.py:476-498) -> lfit.CV.calcFlux (CVModel.py:138).
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
// lfg_diag_iters) keep every kernel in this translation unit (see
// lfg_pair_launch_split below): LFG_ONE_TU, by the one rule of lfg_diag.hpp,
// which lfg_pair_split.hip sees through this file
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


struct Ws {
    double* geo;
    int* status;
    int* bstatus;   // [pairs] stream status (k_setup stream lanes), folded into status by k_elements
    double2* ab;    // [pairs][NELU] eclipse intervals (a, b) of the symmetry-unique elements
    double* donor;  // [pairs][NDONOR/4][DON_STRIDE] symmetry-unique donor tiles
    double* wts;    // [pairs][WT_N] ring / spot weights
    double* prior;
    double* lle;
    double* res;    // [pairs][gp_n] GP trees: residuals y - flux (k_lnlike<2> -> k_gp_like)
    double* gpx;    // [pairs][gp_n] GP trees: e^{-lam dx} of each point (k_lnlike<2> -> k_gp_like)
    int* gpb;       // [pairs][gp_n] GP trees: each point's changepoint block
    // speculative setup (lfg_stretch_step_half_spec): per half parity h and
    // candidate c (the partner's move rejected / accepted) the k_setup
    // outputs of the next half, formed inside the previous half's k_elements
    double* geoC;   // [2][2][pairs][NGEO]
    int* statusC;   // [2][2][pairs]
    int* bstatusC;  // [2][2][pairs]
    double* priorC; // [2][2][W]
    double* qC;     // [2][2][W][ndim]
    double* zfC;    // [2][2][W]
    int* jk;        // [2][W] the partner (in the other half) of walker w's proposal
    int* accflag;   // [2][accstride] by the parity of the half that wrote it: 1 where walker
                    // j accepted its move (a rank's shard of W walkers needs every partner's:
                    // nacc = the half); two copies, so a launch that accepts moves of half h
                    // while it selects candidates by half 1 - h's flags reads one, writes the other
    size_t accstride;
    double* snap;   // [2][accstride][ndim] k_pair: the rows of each half of pos as they were
                    // when the launch that reads them began (SetupArgs.ppos)
    size_t total;
};

inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

Ws carve(void* base, int W, int E, int gp_n = 0, int ndim_spec = 0, int nacc = 0)
{
    const size_t pairs = size_t(W) * size_t(E);
    Ws ws{};
    char* p = static_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += align256(bytes); return r; };
    ws.geo = reinterpret_cast<double*>(take(pairs * LFG_NGEO * sizeof(double)));
    ws.status = reinterpret_cast<int*>(take(pairs * sizeof(int)));
    ws.bstatus = reinterpret_cast<int*>(take(pairs * sizeof(int)));
    ws.ab = reinterpret_cast<double2*>(take(pairs * NELU * sizeof(double2)));
    ws.donor = reinterpret_cast<double*>(take(pairs * (NDONOR / 4) * DON_STRIDE * sizeof(double)));
    ws.wts = reinterpret_cast<double*>(take(pairs * WT_N * sizeof(double)));
    ws.prior = reinterpret_cast<double*>(take(size_t(W) * sizeof(double)));
    ws.lle = reinterpret_cast<double*>(take(pairs * sizeof(double)));
    ws.res = gp_n > 0 ? reinterpret_cast<double*>(take(pairs * size_t(gp_n) * sizeof(double))) : nullptr;
    ws.gpx = gp_n > 0 ? reinterpret_cast<double*>(take(pairs * size_t(gp_n) * sizeof(double))) : nullptr;
    ws.gpb = gp_n > 0 ? reinterpret_cast<int*>(take(pairs * size_t(gp_n) * sizeof(int))) : nullptr;
    if (ndim_spec > 0) {
        ws.geoC = reinterpret_cast<double*>(take(4 * pairs * LFG_NGEO * sizeof(double)));
        ws.statusC = reinterpret_cast<int*>(take(4 * pairs * sizeof(int)));
        ws.bstatusC = reinterpret_cast<int*>(take(4 * pairs * sizeof(int)));
        ws.priorC = reinterpret_cast<double*>(take(4 * size_t(W) * sizeof(double)));
        ws.qC = reinterpret_cast<double*>(take(4 * size_t(W) * ndim_spec * sizeof(double)));
        ws.zfC = reinterpret_cast<double*>(take(4 * size_t(W) * sizeof(double)));
        ws.jk = reinterpret_cast<int*>(take(2 * size_t(W) * sizeof(int)));
        ws.accstride = size_t(W > nacc ? W : nacc);
        ws.accflag = reinterpret_cast<int*>(take(2 * ws.accstride * sizeof(int)));
        ws.snap = reinterpret_cast<double*>(take(2 * ws.accstride * ndim_spec * sizeof(double)));
    }
    ws.total = off;
    return ws;
}

#include "lfg_philox.hpp"  // philox, u53, draw (shared with lfg_pt.hip)

// ---------------------------------------------------------------- k_setup
struct SetupArgs {
    const double* walkers;
    int W, ndim, E, P;
    const int* gather;  // nullptr -> identity
    const int* npars;   // nullptr -> P
    const double* consts;
    const int* prior_type;
    const double* prior_p1;
    const double* prior_p2;
    const double* prior_norm;
    int roche_priors;
    double* geo;
    int* status;
    double* prior;
    int* bstatus;  // stream lanes' status
    int gp;        // GP likelihood: per-pair hyper-parameters and changepoints
    const int* gp_gather;
    const double* gp_base;
    // inline stretch-move proposal (lfg_stretch_step_half; pos nullptr: off):
    // walker w of the batch is the proposal for ensemble walker half * W + w,
    // formed from pos as k_propose does; the walker lanes store it in qout
    const double* pos;
    double a;
    unsigned long long seed, step;
    int half;
    double* qout;
    double* zfout;
    // the batch is walkers lo .. lo + W - 1 of the ns-walker half (ns = W,
    // lo = 0 on one process; a rank's shard with lfg_stretch_step_shard)
    int lo, ns;
    int fixed_invalid;  // lfg_tree.fixed_invalid: every prior lane gives -inf
    const double* prior_c;  // lfg_tree.prior_c (nullable): [ndim][2] Prior.ln_prob constants
    // speculative setup of the next half (lfg_stretch_step_half_spec): cand 1
    // forms the proposal from the partner's own proposal of the half before
    // (step_prev, the other half), i.e. as if the partner's move is accepted;
    // cand 0 from the partner's current position.  jkout: the partner index.
    int cand;
    unsigned long long step_prev;
    int* jkout;
    // nullable: the partner half's positions as they were when this launch
    // began ([ns][ndim]; k_pair's speculative lanes, whose launch accepts
    // moves of that half while they read it)
    const double* ppos;
    // deferred acceptance (k_pair<_, true>, lfg_stretch_step_shard_fold):
    // this half's previous moves are accepted by the launch these lanes run
    // in, so a row of this half is its snapshot fsnap [ns][ndim] (taken by
    // the launch before) re-formed as the proposal of step fstep where the
    // gathered verdict fv [ns] says accepted (not NaN).  fv nullptr: nothing
    // pending, the rows are read from pos
    const double* fv;
    const double* fsnap;
    unsigned long long fstep;
};

// where a lane reads walker w's parameters: the walker row, or the
// stretch-move proposal s + z (c_j - s) ... written as k_propose writes it;
// with ci the partner's position is itself the proposal cj + zj (ci - cj)...
// of the half before (speculative setup, candidate 1)
struct Prop {
    const double* s;
    const double* cj;
    double z;
    const double* ci;
    double zj;
    // deferred acceptance (FOLD): s and ci are snapshot rows; where their
    // pending move was accepted, the row is the proposal spp + sz (s - spp)
    // (cpp, cz for ci), as k_apply_verdicts will write it
    const double* spp;
    double sz;
    const double* cpp;
    double cz;
};

// the stretch-move draw of walker i of half h at step t: z and the partner
__device__ __forceinline__ int stretch_draw(const SetupArgs& A, unsigned long long t, int h, int i, double& z)
{
    const uint4 r = draw(A.seed, t, h, 0, i);
    const double zr = (A.a - 1.0) * u53(r.x, r.y) + 1.0;
    z = zr * zr / A.a;
    return int(__umulhi(r.z, unsigned(A.ns)));
}

template <bool FOLD = false>
__device__ inline Prop make_prop(const SetupArgs& A, int w)
{
    if (!A.pos) return Prop{A.walkers + size_t(w) * A.ndim, nullptr, 0.0, nullptr, 0.0, nullptr, 0.0, nullptr, 0.0};
    const int ns = A.ns, i = A.lo + w;  // walker i of the half, as k_propose's lane i
    const uint4 r = draw(A.seed, A.step, A.half, 0, i);
    const double u = u53(r.x, r.y);
    const double zr = (A.a - 1.0) * u + 1.0;
    const int j = int(__umulhi(r.z, unsigned(ns)));
    if (A.jkout && A.cand == 0) A.jkout[w] = j;
    Prop P{A.pos + size_t(A.half * ns + i) * A.ndim,
           A.ppos ? A.ppos + size_t(j) * A.ndim : A.pos + size_t((1 - A.half) * ns + j) * A.ndim, zr * zr / A.a,
           nullptr, 0.0, nullptr, 0.0, nullptr, 0.0};
    const double* other = A.pos + size_t(1 - A.half) * ns * A.ndim;  // the partner half's rows (FOLD: final)
    if (FOLD && A.fv) {  // this half's rows as the pending verdicts leave them
        P.s = A.fsnap + size_t(i) * A.ndim;
        if (!isnan(A.fv[i])) P.spp = other + size_t(stretch_draw(A, A.fstep, A.half, i, P.sz)) * A.ndim;
    }
    if (A.cand) {  // partner j's proposal in the other half (step_prev), as its own make_prop forms it
        const int hp = 1 - A.half;
        const uint4 rj = draw(A.seed, A.step_prev, hp, 0, j);
        const double zrj = (A.a - 1.0) * u53(rj.x, rj.y) + 1.0;
        const int ij = int(__umulhi(rj.z, unsigned(ns)));
        P.ci = A.pos + size_t(A.half * ns + ij) * A.ndim;
        P.zj = zrj * zrj / A.a;
        if (FOLD && A.fv) {
            P.ci = A.fsnap + size_t(ij) * A.ndim;
            if (!isnan(A.fv[ij])) P.cpp = other + size_t(stretch_draw(A, A.fstep, A.half, ij, P.cz)) * A.ndim;
        }
    }
    return P;
}

// CV parameter count of eclipse e.  P is pinned to a register first: written
// as `npars ? npars[e] : P` the compiler selected between the two ADDRESSES
// and, to give the kernel argument P one, copied it into scratch
// column of eclipse parameter k of (walker-eclipse) gather row r: the tree's
// gather map, or the identity (lfg_flux / lfg_lnprob without a tree).  A
// branch, not a pointer select: a select between the kernel argument and the
// constant identity table made every read a flat load
__device__ __forceinline__ int gat_at(const SetupArgs& A, int i)
{
    return A.gather ? A.gather[i] : i % 18;
}

__device__ __forceinline__ int npars_of(const SetupArgs& A, int e)
{
    int P = A.P;
    asm volatile("" : "+s"(P));
    return A.npars ? A.npars[e] : P;
}

template <bool FOLD = false>
__device__ __forceinline__ double gather_par(const SetupArgs& A, const Prop& P, int g)
{
    if (g < 0) return A.consts[-1 - g];
    if (!P.cj) return P.s[g];
    if (!FOLD) {
        const double cj = P.ci ? fma(P.cj[g] - P.ci[g], P.zj, P.ci[g]) : P.cj[g];
        return fma(P.s[g] - cj, P.z, cj);
    }
    // FOLD: an accepted pending move re-formed exactly as k_apply_verdicts
    // (k_accept_regen) writes it: fma(old - partner, z, partner)
    double s = P.s[g], cj = P.cj[g];
    if (P.spp) s = fma(s - P.spp[g], P.sz, P.spp[g]);
    if (P.ci) {
        double ci = P.ci[g];
        if (P.cpp) ci = fma(ci - P.cpp[g], P.cz, P.cpp[g]);
        cj = fma(cj - ci, P.zj, ci);
    }
    return fma(s - cj, P.z, cj);
}

// Diagnostic build only (-DLFG_PROFILE_SETUP): s_memtime cycle counts of the
// phases of each lane into g_setup_cyc[slot][lane] (lfg_debug_setup_cycles):
//  0-3 setup lane: gather, roche_init, findi, total; 4-7 stream lane: gather,
//  roche_init, bspot, total; 8 prior lane total, 9 the same in 100 MHz
//  s_memrealtime ticks (calibrates the shader clock), 10 its roche_init + findphi
#ifdef LFG_PROFILE_SETUP
__device__ unsigned long long g_setup_cyc[11][4096];
#define LFG_T0(v) unsigned long long v = __builtin_amdgcn_s_memtime()
#define LFG_CY(slot, i, v) \
    do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
         if ((i) < 4096) g_setup_cyc[slot][i] = now_ - (v); (v) = now_; } while (0)
#else
#define LFG_T0(v)
#define LFG_CY(slot, i, v)
#endif

// ------------------------------------------------------- stream lanes of k_setup
// One lane per (walker, eclipse): the ballistic stream to the disc edge
// (MODEL_SPEC 4.5, the stream table), the spot-dependent Roche prior
// (CVModel.py:215-316) and the strip shape (MODEL_SPEC 5.3: peak, tail end).
// Needs only q, rdisc, az, exp1 and exp2, so these lanes run beside the setup
// lanes of the same launch; the stream status goes to bstatus and is folded
// into the pair status by k_elements.
template <bool FOLD = false>
__device__ inline void bspot_lane(const SetupArgs& A, int t)
{
    LFG_T0(tl);
    const int w = t / A.E, e = t - w * A.E;
    const Prop P = make_prop<FOLD>(A, w);
    const int np = npars_of(A, e);
    const double q = gather_par<FOLD>(A, P, gat_at(A, e * 18 + 4));
    const double rdisc = gather_par<FOLD>(A, P, gat_at(A, e * 18 + 6));
    const double az = gather_par<FOLD>(A, P, gat_at(A, e * 18 + 10));
    const double a1 = (np == 18) ? gather_par<FOLD>(A, P, gat_at(A, e * 18 + 14)) : 2.0;  // MODEL_SPEC 5.3 simple: 2, 1
    const double a2 = (np == 18) ? gather_par<FOLD>(A, P, gat_at(A, e * 18 + 15)) : 1.0;
    double* G = A.geo + size_t(t) * LFG_NGEO;
#ifdef LFG_PROFILE_SETUP
    unsigned long long tb = tl;
    LFG_CY(4, t, tb);
#endif
    Roche R;
    QPatch qp;
    int st = (isfinite(q) && isfinite(rdisc) && isfinite(az)) ? roche_init(R, q, &qp) : ST_BAD_ARGS;
    LFG_CY(5, t, tb);
    double bs[4] = {0.0, 0.0, 0.0, 0.0};
    if (st == ST_OK) st = bspot<false>(R, rdisc * R.xl1, bs, &qp);
    LFG_CY(6, t, tb);
    double rprior = 0.0;
    if (st != ST_OK) {
        rprior = -INFINITY;
    } else {
        double alpha = atan2(bs[1], bs[0]) / DEG;
        if (alpha < 0.0) alpha = 90.0 - alpha;
        const double tangent = alpha + 90.0;
        const double minaz = fmax(0.0, tangent - AZ_SLOPE), maxaz = fmin(178.0, tangent + AZ_SLOPE);
        if (az < minaz || az > maxaz) rprior = -INFINITY;
    }
    G[G_BSX] = bs[0]; G[G_BSY] = bs[1];
    G[G_RPRIOR_BS] = A.roche_priors ? rprior : 0.0;
    if (a1 > 0.0 && a2 > 0.0 && isfinite(a1) && isfinite(a2)) {  // else the setup lane fails the pair
        const double upk = pow(a1 / a2, 1.0 / a2);
        const double lnpk = a1 * log(upk) - pow(upk, a2);
        const double umax = bs_umax(a1, a2, lnpk);
        G[G_UPK] = upk; G[G_UMAX] = umax; G[G_LNPK] = lnpk;
        G[G_EXP1] = a1; G[G_EXP2] = a2;
        // a profile that over- or underflows (exp2 -> 0) is bad geometry,
        // checked after the stream as the oracle does (MODEL_SPEC 6)
        if (st == ST_OK && !(isfinite(upk) && isfinite(lnpk) && isfinite(umax))) st = ST_BAD_GEOMETRY;
    }
    A.bstatus[t] = st;
    LFG_CY(7, t, tl);
}

// per-walker lane: LCModel.ln_prior dphi check (CVModel.py:452-473) and
// Node.ln_prior over the variable parameters (model.py:439-449); with the
// fused stretch move it also stores the proposal
template <bool FOLD = false>
__device__ inline void prior_lane(const SetupArgs& A, int w)
{
    LFG_T0(tl);
#ifdef LFG_PROFILE_SETUP
    unsigned long long trl = __builtin_amdgcn_s_memrealtime(), tr = tl;  // 100 MHz: calibrates s_memtime
#endif
    const Prop P = make_prop<FOLD>(A, w);
    double lp = 0.0;
    if (A.roche_priors) {
        // LCModel.ln_prior: dphi <= findphi(q, 90) - 1e-6, findphi from the
        // q series of the stream table (~1e-16; the solver outside its range)
        const double q = gather_par<FOLD>(A, P, gat_at(A, 4));
        const double dphi = gather_par<FOLD>(A, P, gat_at(A, 5));
        const QPatch qp = q_patch(q);
        double maxphi;
        if (qp.iq >= 0) {
            maxphi = q_series(kStPhi90, qp);
        } else {
            Roche R;
            if (roche_init(R, q) != ST_OK || findphi_fast(R, 90.0, maxphi) != ST_OK) maxphi = -INFINITY;
        }
        if (!(dphi <= maxphi - DPHI_TOL)) lp = -INFINITY;
        LFG_CY(10, w, tr);
    }
    // the walker's parameters in chunks of PCH: each chunk's loads are issued
    // back to back (one memory latency per chunk, not per parameter), then
    // the proposal is stored and the chunk's prior terms summed in order
    constexpr int PCH = 16;
    double* qo = A.pos ? A.qout + size_t(w) * A.ndim : nullptr;
    for (int d0 = 0; d0 < A.ndim; d0 += PCH) {
        double v[PCH];
#pragma unroll
        for (int k = 0; k < PCH; ++k) v[k] = (d0 + k < A.ndim) ? gather_par<FOLD>(A, P, d0 + k) : 0.0;
        if (qo) {  // store the proposal: k_lnlike copies an accepted one into pos
#pragma unroll
            for (int k = 0; k < PCH; ++k)
                if (d0 + k < A.ndim) qo[d0 + k] = v[k];
        }
        if (A.prior_type && A.prior_c) {
            // Prior.ln_prob from the tree's constants (include/lfg.h): the
            // terms c0 - z^2/2 (gauss) or c0, summed in order, and one log of
            // the chunk's product of log_uniform / mod_jeff arguments.  The
            // product is kept as mantissa x 2^pex (frexp per factor: the
            // mantissas lie in [1/2, 1), so 16 of them never leave the normal
            // range and no partial product loses digits)
            double prod = 1.0;
            int pex = 0;
            bool ok = true;
#pragma unroll
            for (int k = 0; k < PCH; ++k) {
                const int d = d0 + k;
                if (d < A.ndim) {
                    const int ty = A.prior_type[d];
                    const double p1 = A.prior_p1[d], p2 = A.prior_p2[d], c0 = A.prior_c[2 * d];
                    const double z = (v[k] - p1) * A.prior_c[2 * d + 1];
                    const double term = (ty <= 1) ? fma(-0.5 * z, z, c0) : c0;
                    lp += term;
                    int fe;
                    const double fm = frexp((ty == 3) ? v[k] : (ty == 4 ? v[k] + p1 : 1.0), &fe);
                    prod *= fm;
                    pex += fe;
                    // scipy's pdf underflows to 0 (log -> -inf) once the unit
                    // normal's density e = term + ln p2 or its quotient by p2 (term) is
                    // below e^-745.13: e decides for p2 < 1 (c1 > 1), -ln p2 = c0 + ln sqrt(2 pi)
                    const double thr = (A.prior_c[2 * d + 1] > 1.0) ? PDF_LN_MIN + (c0 + LN_SQRT_2PI) : PDF_LN_MIN;
                    ok = ok && ((ty <= 1) ? (term > thr && (ty == 0 || v[k] > 0.0))
                                          : (ty == 4 ? (v[k] > 0.0 && v[k] < p2)
                                                     : (ty <= 3 && v[k] > p1 && v[k] < p2)));
                }
            }
            lp = ok ? lp - fma(double(pex), LN2, log(prod)) : -INFINITY;
        } else if (A.prior_type) {
#pragma unroll
            for (int k = 0; k < PCH; ++k) {
                const int d = d0 + k;
                if (d < A.ndim)
                    lp += prior_lnprob(A.prior_type[d], A.prior_p1[d], A.prior_p2[d], A.prior_norm[d], v[k]);
            }
        }
    }
    if (qo) A.zfout[w] = (A.ndim - 1.0) * log(P.z);
    A.prior[w] = A.fixed_invalid ? -INFINITY : lp;
    LFG_CY(8, w, tl);
#ifdef LFG_PROFILE_SETUP
    if (w < 4096) g_setup_cyc[9][w] = __builtin_amdgcn_s_memrealtime() - trl;
#endif
}

// one lane of k_setup: t < npairs setup lanes, then W prior lanes, then
// npairs stream lanes
template <bool FOLD = false>
__device__ __forceinline__ void setup_any(const SetupArgs& A, int t)
{
    const int npairs = A.W * A.E;
    if (t >= 2 * npairs + A.W) return;
    if (t >= npairs + A.W) {  // stream lanes (own waves: npairs + W is a multiple of 64 in the bench)
        bspot_lane<FOLD>(A, t - npairs - A.W);
        return;
    }
    if (t >= npairs) {
        prior_lane<FOLD>(A, t - npairs);
        return;
    }

    // setup lane: one per (walker, eclipse)
    LFG_T0(tl);
    const int w = t / A.E, e = t - (t / A.E) * A.E;
    const Prop P = make_prop<FOLD>(A, w);
    const int np = npars_of(A, e);
    double p[18];
    bool finite = (np == 14 || np == 18);
#pragma unroll  // p[] stays in registers (a rolled loop kept it in scratch)
    for (int k = 0; k < 18; ++k) {
        p[k] = (k < np) ? gather_par<FOLD>(A, P, gat_at(A, e * 18 + k)) : 0.0;
        finite = finite && isfinite(p[k]);
    }
    if (np == 14) { p[14] = 2.0; p[15] = 1.0; p[16] = 90.0; p[17] = 0.0; }  // MODEL_SPEC 5.3
    double* G = A.geo + size_t(t) * LFG_NGEO;
#ifdef LFG_PROFILE_SETUP
    unsigned long long tf = tl;
    LFG_CY(0, t, tf);
#endif
    // what does not depend on the inclination is formed and stored before
    // findi, so that only q's Roche record and dphi stay live through the
    // solve (this lane also runs, twice, inside k_elements' register budget:
    // lfg_stretch_step_half_spec); the few values needed after it are read
    // back from the record
    {
        const double tilt = p[16] * DEG, psi = (p[10] - 90.0 + p[17]) * DEG;
        double st_, ct_, sp_, cp_, saz, caz;
        sincos(tilt, &st_, &ct_);
        sincos(psi, &sp_, &cp_);
        sincos(p[10] * DEG, &saz, &caz);
        G[G_CAZ] = caz; G[G_SAZ] = saz;
        G[G_NB0] = st_ * cp_; G[G_NB1] = st_ * sp_; G[G_NB2] = ct_;
        G[G_BDEN] = fabs(st_);  // |sin tilt| until the inclination is known
        G[G_ULIMB] = p[7]; G[G_DEXP] = p[12];
        G[G_FIS] = p[11]; G[G_PHI0] = p[13];
        G[G_WDF] = p[0]; G[G_DF] = p[1]; G[G_SF] = p[2]; G[G_RSF] = p[3];
    }
    int st = ST_OK;
    double rprior = 0.0;
    Roche R;
    if (!finite) st = ST_BAD_ARGS;
    else st = roche_init(R, p[4]);
    LFG_CY(1, t, tf);
    bool bad_geo = false;
    if (st == ST_OK) {
        // SimpleEclipse.ln_prior Roche checks not involving the stream (CVModel.py:215-316)
        if (p[6] * R.xl1 > DISC_MAX_A) rprior = -INFINITY;
        const double rwd = p[8], scale = p[9];
        if (scale > rwd * 3.0 || scale < rwd / 3.0) rprior = -INFINITY;
        // geometry (MODEL_SPEC 6), reported after findi's status
        const double rwd_a = p[8] * R.xl1, rdisc_a = p[6] * R.xl1;
        bad_geo = !(rwd_a > 0.0) || !(rdisc_a > rwd_a) || !(rdisc_a < R.xl1) || !(p[9] > 0.0) || !(p[14] > 0.0) ||
                  !(p[15] > 0.0);
        G[G_Q] = R.q; G[G_CA] = R.cA; G[G_CB] = R.cB; G[G_MU] = R.mu;
        G[G_XL1] = R.xl1; G[G_PL1] = R.pl1; G[G_RS] = R.Rs; G[G_RS2] = R.Rs2;
        G[G_RWD] = rwd_a; G[G_RDISC] = rdisc_a; G[G_REFF] = eggleton(R.q);
        G[G_L] = p[9] * R.xl1;
    } else {
        rprior = -INFINITY;
    }
    const double dphi = p[5];
    double inc = 0.0;
    if (st == ST_OK) st = findi_fast(R, dphi, inc);
    LFG_CY(2, t, tf);
    if (st == ST_OK && bad_geo) st = ST_BAD_GEOMETRY;

    A.status[t] = st;
    G[G_RPRIOR] = A.roche_priors ? rprior : 0.0;
    if (st != ST_OK) return;

    double s, c;
    sincos(inc * DEG, &s, &c);
    const double fis = G[G_FIS];
    const double nmax = G[G_BDEN] * s + G[G_NB2] * c;
    G[G_S] = s; G[G_C] = c; G[G_INC] = inc;
    G[G_BDEN] = fis + (1.0 - fis) * fmax(nmax, 0.0);
    const double sce = s * cos(PI * dphi);
    // (negative: no WD or disc element's line of sight comes near L1, element_interval_fast)
    const double rcal = sqrt(1.0 - sce * sce);
    G[G_RCAL] = l1_out_of_reach(R, s, c, G[G_RWD], G[G_RDISC]) ? -rcal : rcal;
    if (A.gp) {
        // SimpleGPEclipse.create_GP / calcChangepoints (CVModel.py:529-648):
        // amplitudes exp(ln_amp), metric exp(ln_tau); the changepoint
        // distance from the cache unless q, dphi or rwd moved > 120 %.  A
        // walker that trips the rule needs wdphases (ten nested eclipse
        // solves): it is marked pending (G_GP_OK = 2) and k_gp_dcp solves the
        // ten limb points in parallel lanes before k_lnlike<2> (kept out of
        // this lane, whose registers the speculative copies inside
        // k_elements share)
        const int* gg = A.gp_gather + e * 3;
        const double ain = exp(gather_par<FOLD>(A, P, gg[0])), aout = exp(gather_par<FOLD>(A, P, gg[1]));
        const double tau = exp(gather_par<FOLD>(A, P, gg[2]));
        const double* B = A.gp_base + e * 4;
        const double q = R.q, rwd = p[8];
        const bool pend = fabs(B[1] - dphi) / dphi > 1.2 || fabs(B[0] - q) / q > 1.2 || fabs(B[2] - rwd) / rwd > 1.2;
        const bool ok = tau > 0.0 && isfinite(ain) && isfinite(aout);
        G[G_GP_AIN] = ain;
        G[G_GP_AOUT] = aout;
        G[G_GP_LAM] = sqrt(3.0 / tau);
        G[G_GP_DCP] = B[3];
        G[G_GP_DPHI] = dphi;
        G[G_GP_RWD] = rwd;
        G[G_GP_OK] = !ok ? 0.0 : (pend ? 2.0 : (isfinite(B[3]) ? 1.0 : 0.0));
    }
    LFG_CY(3, t, tl);
}

#ifndef LFG_NOLICM_TU  // (lfg_pair_split.hip compiles k_pair only)
__global__ __launch_bounds__(SETUP_BLOCK) void k_setup(SetupArgs A)
{
    setup_any(A, blockIdx.x * SETUP_BLOCK + threadIdx.x);
}
#endif

// ------------------------------------------------------------- k_elements
// One lane per symmetry-unique element.  The WD/disc grids are mirror
// symmetric under y -> -y and the donor grid under y -> -y and z -> -z; the
// Roche potential shares those symmetries, so a mirrored element's eclipse
// interval is [-b, -a] and a mirrored tile's vector has y (and/or z) negated.
// Unique items per (walker, eclipse): WD 200, disc 500, spot 100, donor 100.
// Output: eclipse intervals as (a, b) pairs and the 100 unique donor tile
// vectors; weights depend on ring only and are formed in k_lnlike.
#ifdef LFG_COUNT_ITERS
__device__ unsigned long long g_iter_dbg[64];

#endif
constexpr int U_WD = NWD / 2, U_DISC = NDISC / 2, U_BS = NBS, U_DON = NDONOR / 4;
constexpr int NUNIQ = U_WD + U_DISC + U_BS + U_DON;
// unique-item order: WD, disc, donor, then the spot
constexpr int U_MAIN = U_WD + U_DISC + U_DON;

__device__ __forceinline__ int wd_ring_of(int u)  // ring of unique WD tile u (ring ir starts at 2 ir^2)
{
#if LFG_PAIR_SINK_MERGE
    return kRingOf[u];
#else
    int ir = int(sqrt(u * 0.5));
    if (2 * (ir + 1) * (ir + 1) <= u) ++ir;
    if (2 * ir * ir > u) --ir;
    return ir;
#endif
}

// element weights (MODEL_SPEC 5.1-5.3): per WD ring, per disc ring, per spot element
__device__ inline double wd_ring_weight(int ir, double ul) { return fma(kWdA[ir], 1.0 - ul, kWdB[ir] * ul); }

// radial integral of r^(1 - dexp) dr over the disc annuli (MODEL_SPEC 5.2):
// the boundary term P(r) = r^ex / ex, or ln r when ex = 2 - dexp vanishes
template <typename GPtr>
__device__ inline double disc_boundary(int i, GPtr G)
{
    const double rin = G[G_RWD];
    const double r = rin + i * ((G[G_RDISC] - rin) / NDISC_R);
    const double ex = 2.0 - G[G_DEXP];
    // the integral of r^(1 - dexp) from the inner edge, as rin^ex expm1(ex ln(r / rin)) / ex: the difference of
    // two powers, r^ex / ex - rin^ex / ex, loses 1 / (ex ln(r1 / r0)) of its digits as dexp -> 2
    const double lr = log(r / rin);
    return (fabs(ex) < 1e-10) ? lr : pow(rin, ex) * expm1(ex * lr) / ex;
}

template <typename GPtr>
__device__ inline double disc_ring_weight(int ir, GPtr G)
{
    return (TWO_PI / NDISC_AZ) * (disc_boundary(ir + 1, G) - disc_boundary(ir, G));
}

template <typename GPtr>
__device__ inline double bs_weight(int j, GPtr G)
{
    const double uk = (j + 0.5) * (G[G_UMAX] / NBS);
    return exp(G[G_EXP1] * log(uk) - pow(uk, G[G_EXP2]) - G[G_LNPK]);
}

// A walker whose ln_prior is -inf (a Prior.ln_prob term, the LCModel dphi
// check, or a Roche prior of this eclipse) has ln_prob = -inf whatever its
// likelihood: Node.ln_prob never calls ln_like for it (model.py:476-498).
// Tree calls skip such pairs in k_elements, k_lnlike and k_gp_like alike, so
// that no kernel reads tables the others did not write.  (Stretch proposals
// outside the prior box are common: in a long config-2 chain most of the
// proposals that sent element solves to the nested fallback were of this
// kind, tools/fallback_hunt.py.)
__device__ __forceinline__ bool prior_rejects(double lprior, const double* G)
{
    return !(lprior + G[G_RPRIOR] + G[G_RPRIOR_BS] > -INFINITY);
}

// k_elements' side jobs in lfg_stretch_step_half_spec:
//  - sel: this half's k_setup outputs were formed speculatively inside the
//    previous half's k_elements for both fates of each walker's partner;
//    the pair takes candidate c = accflag[jk[w]] and its first block copies
//    it into the standard workspace slots k_lnlike reads
//  - spec: the leading nspecblk blocks run the k_setup lanes of the next half
//    for both candidates (setup_any on S[0], S[1])
struct ElemSpec {
    const int* jk;  // nullptr: no selection
    const int* accflag;
    const double* geoC;
    const int* statusC;
    const int* bstatusC;
    const double* priorC;
    const double* qC;
    const double* zfC;
    double* prior;
    double* q;
    double* zf;
    int* bstatus;
    int E, ndim;
    const double* lprior;  // tree calls: the batch's Prior sums (k_setup), prior_rejects skips; nullptr: none
    SetupArgs S[2];
    int nspec;     // lanes per candidate (0: no speculative setup)
    int nspecblk;  // leading blocks that run them
};

// where one pair's element results go: the global workspace tables
// (k_elements) or the block's LDS (k_pair)
struct ElemOut {
    double2* abw;  // [NU_WDD] WD/disc intervals, slot uslot(u)
    double2* abs;  // [NBS] spot intervals
    double* don;   // [U_DON][DON_STRIDE] donor tiles
    double* wtd;   // [NDISC_R + 1] disc ring weights, then the disc total
    double* wbs;   // [NBS] spot element weights
};

// the disc ring weights (MODEL_SPEC 5.2) by the lanes of items v = NUNIQ +
// i, i = 0..NDISC_R, consecutive lanes of one wave: lane i holds the boundary
// term P(r_i) and ring i's weight is the difference of neighbours (one pow
// per lane of one wave, instead of two in a ring-start lane of every disc wave)
// (k_pair, LFG_PAIR_SINK_MERGE: the total's lane also writes its reciprocal,
// which every disc lane of the sink formed for itself, to wtd[NDISC_R + 1])
template <bool RCP = false, typename GPtr>
__device__ __forceinline__ void ring_weight_lane(int rb, GPtr G, double* __restrict__ wtd)
{
    const double P = disc_boundary(rb, G);
    const int lane = int(threadIdx.x) & 63, l0 = lane - rb;  // lane of P(r_0)
    const double Pn = __shfl(P, min(lane + 1, l0 + NDISC_R), 64);
    const double Pt = __shfl(P, l0 + NDISC_R, 64);
    if (rb < NDISC_R) wtd[rb] = (TWO_PI / NDISC_AZ) * (Pn - P);
    if (rb == 0) wtd[NDISC_R] = TWO_PI * (Pt - P);
    if (RCP && rb == 0) wtd[NDISC_R + 1] = 1.0 / (TWO_PI * (Pt - P));
}

// results of an item go to a sink: wd_disc(u, a, b), spot(j, a, b, w),
// donor(uu, vx, vy, vz, centre, half-width)
template <typename GPtr, typename Sink>
__device__ __forceinline__ void element_item_to(int v, GPtr G, Sink& K);

// the sink of k_elements (and k_pair's point-major fallback): the tables
struct MemSink {
    const ElemOut& O;
    __device__ __forceinline__ void mark() {}
    __device__ __forceinline__ void wd_disc(int u, double a, double b) { O.abw[uslot(u)] = make_double2(a, b); }
    __device__ __forceinline__ void spot(int j, double a, double b, double w)
    {
        O.abs[j] = make_double2(a, b);
        O.wbs[j] = w;
    }
    __device__ __forceinline__ void donor(int uu, double vx, double vy, double vz, double cen, double hw)
    {
        double* D = O.don + uu * DON_STRIDE;
        D[0] = vx;
        D[1] = vy;
        D[2] = vz;
        D[3] = cen;
        D[4] = hw;
    }
};

template <typename GPtr>
__device__ __forceinline__ void element_item(int v, GPtr G, const ElemOut& O)
{
    MemSink K{O};
    element_item_to(v, G, K);
}

// one k_elements lane's item v of pair `pair` (v >= NUNIQ: the disc ring
// weights of the last chunk's spare lanes)
__device__ __forceinline__ void element_lane(int v, int pair, int npairs, const double* __restrict__ G, int st0, int bst,
                                             int* status, double2* __restrict__ AB, double* __restrict__ DON,
                                             double* __restrict__ WT, const ElemSpec& X)
{
    double* Wp = WT + size_t(pair) * WT_N;
    if (v >= NUNIQ) {  // the last chunk's spare lanes
        const int rb = v - NUNIQ;
        if (rb > NDISC_R || st0 != ST_OK) return;
        ring_weight_lane(rb, G, Wp + WT_DISC);
        return;
    }
    static_assert((NUNIQ % ELEM_BLOCK) + NDISC_R + 1 <= ELEM_BLOCK, "ring-weight lanes fit in the last chunk");
    static_assert(WT_TD == WT_DISC + NDISC_R, "disc total follows the ring weights");
    if (st0 != ST_OK) return;
    if (bst != ST_OK) {
        if (v == 0 && !X.jk) status[pair] = bst;
        return;
    }
    if (X.lprior) {  // the walker's ln_prior is -inf: nothing to evaluate (k_lnlike skips it too)
        const int w = pair / X.E;
        const double lp = X.jk ? X.priorC[size_t(X.accflag[X.jk[w]]) * (npairs / X.E) + w] : X.lprior[w];
        if (prior_rejects(lp, G)) return;
    }
    double2* ABp = AB + size_t(pair) * NELU;
    element_item(v, G, ElemOut{ABp, ABp + NU_WDD, DON + size_t(pair) * U_DON * DON_STRIDE, Wp + WT_DISC, Wp + WT_BS});
}

// item v (v < NUNIQ) of a pair: item order WD, disc, spot, donor; k_elements
// deals the chunks of 64 items out in its own dispatch order (kOrder)
template <typename GPtr, typename Sink>
__device__ __forceinline__ void element_item_to(int v, GPtr G, Sink& K)
{
    constexpr int V_BS = U_WD + U_DISC;
    const int u = (v < V_BS) ? v : (v < V_BS + U_BS ? U_MAIN + (v - V_BS) : v - U_BS);
    const Roche R{G[G_Q], G[G_CA], G[G_CB], G[G_MU], G[G_XL1], G[G_PL1], G[G_RS], G[G_RS2]};
    const double s = G[G_S], c = G[G_C];

    if (u >= U_WD + U_DISC && u < U_MAIN) {  // donor tile (MODEL_SPEC 5.4), phi' in (0, pi/2)
        const int uu = u - (U_WD + U_DISC);
        const int it = uu / (NDONOR_P / 4), ip = uu - it * (NDONOR_P / 4);
        const double stc = kDonSt[it], ctc = kDonCt[it];
        const double dx = -ctc, dy = stc * kDonCp[ip], dz = stc * kDonSp[ip];
        double lo = 0.0, hi = R.Rs, r = G[G_REFF];
        if (!(r > lo && r < hi)) r = 0.5 * hi;
#if LFG_F32_OPEN && LFG_F32_ROOT_STEPS > 0
        r = root_open32<LFG_F32_ROOT_STEPS>(R, dx, dy, dz, hi, r);  // to ~1e-7 of the root in float
#endif
        double gx, gy, gz;
        for (int itr = 0; itr < ROOT_MAXIT; ++itr) {
            const double X0 = fma(r, dx, 1.0), X1 = r * dy, X2 = r * dz;
            const double f = rpot_grad(R, X0, X1, X2, gx, gy, gz) - R.pl1;
            const double df = gx * dx + gy * dy + gz * dz;
            if (f > 0.0) hi = r; else lo = r;
            const double stp = f * rcp_fast(df);  // (an IEEE quotient: ~10 dependent issue slots more a step)
            if (df > 0.0 && fabs(stp) <= ROOT_LAST) { r -= stp; break; }  // last Newton step
            double rn = (df > 0.0) ? r - stp : 0.5 * (lo + hi);
            if (!(rn > lo && rn < hi)) rn = 0.5 * (lo + hi);
            r = rn;
        }
        rgrad(R, fma(r, dx, 1.0), r * dy, r * dz, gx, gy, gz);
        const double ig = rsqrt(gx * gx + gy * gy + gz * gz);
        const double nx = gx * ig, ny = gy * ig, nz = gz * ig;
        const double dA = r * r * kDonOmega[it] / (nx * dx + ny * dy + nz * dz);
        const double vx = dA * nx, vy = dA * ny, vz = dA * nz;
        // visibility arc: v.e = s rho cos(theta + alpha) + c vz > 0 with
        // rho cos(alpha) = vx, rho sin(alpha) = vy  ->  |theta + alpha| < acos(kappa)
        const double srho = s * sqrt(vx * vx + vy * vy);
        const double kap = (srho > 0.0) ? -c * vz / srho : (c * vz > 0.0 ? -2.0 : 2.0);
        const double cen = -atan2(vy, vx) * (1.0 / TWO_PI), hw = acos(fmin(fmax(kap, -1.0), 1.0)) * (1.0 / TWO_PI);
        K.mark();
        K.donor(uu, vx, vy, vz, cen, hw);
        return;
    }

    // the element of unique item u (its mirror's interval is implied)
    double Px, Py, Pz, rcal = G[G_RCAL];
    if (u < U_WD) {  // white dwarf tile (MODEL_SPEC 5.1), cos(psi) > 0 half
        const int ir = wd_ring_of(u);
        const double rc = kWdRc[ir], mu0 = kWdMu0[ir];
        const double cp = kWdCos[u], sp = kWdSin[u];
        const double rw = G[G_RWD];
        Px = rw * (-rc * sp * c + mu0 * s);
        Py = rw * (rc * cp);
        Pz = rw * (rc * sp * s + mu0 * c);
    } else if (u < U_WD + U_DISC) {  // disc (MODEL_SPEC 5.2), alpha in (0, pi)
        const int uu = u - U_WD;
#if LFG_PAIR_SINK_MERGE
        const int ir = kRingOf[u] - NWD_RINGS, j = uu - ir * (NDISC_AZ / 2);
#else
        const int ir = uu / (NDISC_AZ / 2), j = uu - ir * (NDISC_AZ / 2);
#endif
        const double rin = G[G_RWD];
        const double rc = rin + (ir + 0.5) * ((G[G_RDISC] - rin) / NDISC_R);
        Px = rc * kDiscCos[j];
        Py = rc * kDiscSin[j];
        Pz = 0.0;
    } else {  // bright-spot strip (MODEL_SPEC 5.3): no mirror partner
        const int j = u - U_MAIN;
        const double uk = (j + 0.5) * (G[G_UMAX] / NBS);
        const double off = G[G_L] * (uk - G[G_UPK]);
        Px = fma(off, G[G_CAZ], G[G_BSX]);
        Py = fma(off, G[G_SAZ], G[G_BSY]);
        Pz = 0.0;
        rcal = fabs(rcal);  // the strip is not bound by the disc's radius: test each element for L1
    }
    double a, b;
#ifdef LFG_COUNT_ITERS
    // diagnostic build: per region (WD, disc, spot) sums of iterations
    // [cone, ingress, egress], their per-wave maxima, fallbacks, items, eclipsed
    bool fb = false;
    int nit[3] = {0, 0, 0};
    double gs[2] = {0.0, 0.0};
    element_interval_fast(R, Px, Py, Pz, s, c, rcal, G[G_REFF], a, b, &fb, nit, gs);
    {
        const int reg = (u < U_WD) ? 0 : (u < U_WD + U_DISC ? 1 : 2);
        unsigned long long* C = g_iter_dbg + reg * 16;
        for (int i = 0; i < 3; ++i) {
            const int ni = i ? nit[i] : nit[0] % 1000;  // (the FP32 opener's steps sit x 1000 in nit[0])
            atomicAdd(C + i, (unsigned long long)ni);
            int m = ni;
            for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
            if ((threadIdx.x & 63) == 0) atomicAdd(C + 3 + i, (unsigned long long)m);
        }
        if ((threadIdx.x & 63) == 0) atomicAdd(C + 9, 1ull);
        atomicAdd(C + 6, fb ? 1ull : 0ull);
        if (fb) {  // slots 48..63: count, then up to 15 (pair << 16 | item) records
            const unsigned long long k = atomicAdd(g_iter_dbg + 48, 1ull);
            if (k < 15) g_iter_dbg[49 + k] = (static_cast<unsigned long long>(blockIdx.x) << 16) | unsigned(u);
        }
        atomicAdd(C + 7, 1ull);
        atomicAdd(C + 8, (a < b) ? 1ull : 0ull);
        if (a < b && !fb) {  // initial-guess error of the tangency solves: bins < 1e-4, 1e-3, 1e-2, 3e-2, 1e-1, more
            const double er = fmax(fabs(gs[0] - a * TWO_PI), fabs(gs[1] - b * TWO_PI));
            const int bin = er < 1e-4 ? 0 : er < 1e-3 ? 1 : er < 1e-2 ? 2 : er < 3e-2 ? 3 : er < 1e-1 ? 4 : 5;
            atomicAdd(C + 10 + bin, 1ull);
        }
    }
#else
    element_interval_fast(R, Px, Py, Pz, s, c, rcal, G[G_REFF], a, b);
#endif
    K.mark();
    if (u >= U_MAIN) K.spot(u - U_MAIN, a, b, bs_weight(u - U_MAIN, G));
    else K.wd_disc(u, a, b);
}

#ifdef LFG_PROFILE_ELEM  // diagnostic build only: per-wave start / end (s_memrealtime, 100 MHz), HW_ID, kind
__device__ unsigned long long g_elem_wav[4][32768];
__device__ __forceinline__ void elem_stamp(unsigned long long t0, int kind)
{
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 32768) {
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        g_elem_wav[0][blockIdx.x] = t0;
        g_elem_wav[1][blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        g_elem_wav[2][blockIdx.x] = hw;
        g_elem_wav[3][blockIdx.x] = kind;
    }
}
#endif

#ifndef LFG_NOLICM_TU  // (lfg_pair_split.hip compiles k_pair only)
__global__ __launch_bounds__(ELEM_BLOCK) __attribute__((amdgpu_waves_per_eu(ELEM_MINW))) void k_elements(const double* __restrict__ geo, int* status, int npairs,
                                                         double2* __restrict__ AB, double* __restrict__ DON,
                                                         double* __restrict__ WT, const int* __restrict__ bstatus,
                                                         ElemSpec X)
{
#ifdef LFG_PROFILE_ELEM
    const unsigned long long pt0 = __builtin_amdgcn_s_memrealtime();
#endif
    if (int(blockIdx.x) < X.nspecblk) {  // speculative setup lanes of the next half
        // candidate c's lanes fill blocks [c * nb, (c + 1) * nb): c is uniform
        // in a block, so X.S[c] is selected in scalar registers (a lane-varying
        // c made the compiler keep both SetupArgs in a private array)
        const int nb = (X.nspec + int(blockDim.x) - 1) / int(blockDim.x);
        const int c = int(blockIdx.x) < nb ? 0 : 1;
        const int t = (int(blockIdx.x) - c * nb) * int(blockDim.x) + int(threadIdx.x);
        if (t < X.nspec) setup_any(X.S[__builtin_amdgcn_readfirstlane(c)], t);
#ifdef LFG_PROFILE_ELEM
        elem_stamp(pt0, 0);
#endif
        return;
    }
    const unsigned bid = blockIdx.x - unsigned(X.nspecblk);
    // blocks cover the NUNIQ unique items of every pair in chunks of
    // blockDim.x (the spot items fill the last chunk); block b takes pair
    // b % npairs, so that (with npairs a multiple of 8 and blocks dealt
    // round-robin over the XCDs) a pair's tables are written on the XCD whose
    // L2 k_lnlike block `pair` reads them from -- speed only.  Item 0 folds
    // the stream lanes' status into the pair status (MODEL_SPEC 6 order:
    // setup failures first); every item skips a pair that failed either.
    const int pair = int(bid % unsigned(npairs));
    // LFG_ELEM_IPL items per lane, one after the other (chunks of
    // ELEM_BLOCK * LFG_ELEM_IPL items)
    // chunks in dispatch order: the donor's (latency-bound 1-D roots, few
    // VALU instructions) and the spot's and outer disc's (four Newton steps)
    // first, the WD's and inner disc's (three) last, so that the second
    // round of waves ends on short ones (profiles/r03/elem_timeline_*.txt:
    // the kernel span 27.4 -> 25.2 us at config 2)
    static_assert(ELEM_BLOCK * LFG_ELEM_IPL == 64 && (NUNIQ + NDISC_R + 1 + 63) / 64 == 15, "chunk order table");
    constexpr int kOrder[15] = {13, 14, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0};
    const int ck = kOrder[bid / unsigned(npairs)];
    const int v0 = ck * (int(blockDim.x) * LFG_ELEM_IPL) + int(threadIdx.x);
    const double* G = geo + size_t(pair) * LFG_NGEO;
    int st0, bst;
    if (X.jk) {
        const int w = pair / X.E, e = pair - w * X.E;
        const size_t cp = size_t(X.accflag[X.jk[w]]) * npairs + pair;  // candidate slot of the pair
        G = X.geoC + cp * LFG_NGEO;
        st0 = X.statusC[cp];
        bst = X.bstatusC[cp];
        if (bid < unsigned(npairs)) {  // the pair's first block: the selected candidate into the standard slots
            const int l = int(threadIdx.x);
            double* Gd = const_cast<double*>(geo) + size_t(pair) * LFG_NGEO;
            if (l < LFG_NGEO) Gd[l] = G[l];
            if (l == LFG_NGEO) status[pair] = (st0 != ST_OK) ? st0 : bst;
            if (l == LFG_NGEO + 1) X.bstatus[pair] = bst;
            if (e == 0) {
                const size_t cw = size_t(X.accflag[X.jk[w]]) * (npairs / X.E) + w;
                for (int d = l; d < X.ndim; d += int(blockDim.x)) X.q[size_t(w) * X.ndim + d] = X.qC[cw * X.ndim + d];
                if (l == LFG_NGEO + 2) X.prior[w] = X.priorC[cw];
                if (l == LFG_NGEO + 3) X.zf[w] = X.zfC[cw];
            }
        }
    } else {
        st0 = status[pair];
        bst = bstatus[pair];
    }
#pragma unroll 1
    for (int k = 0; k < LFG_ELEM_IPL; ++k)
        element_lane(v0 + k * int(blockDim.x), pair, npairs, G, st0, bst, status, AB, DON, WT, X);
#ifdef LFG_PROFILE_ELEM
    elem_stamp(pt0, 1 + ck);  // 1 + chunk of the pair's items
#endif
}
#endif

// interval of element k (MODEL_SPEC 5 numbering) from a pair's table: the
// unique item of k's mirror pair, mirrored when k is the partner
__device__ inline double2 elem_ab(const double2* __restrict__ AB, int k)
{
    if (k >= NWD + NDISC) return AB[NU_WDD + (k - NWD - NDISC)];
    int u;
    bool mir;
    if (k < NWD) {  // ring ir holds 4 (2 ir + 1) tiles; j in [0, q4) u [3 q4, nk) are the unique ones
        int ir = int(sqrt(k * 0.25));
        if (4 * (ir + 1) * (ir + 1) <= k) ++ir;
        if (4 * ir * ir > k) --ir;
        const int nk = 4 * (2 * ir + 1), q4 = nk / 4;
        int j = k - 4 * ir * ir;
        mir = j >= q4 && j < 3 * q4;
        if (mir) j = (j < nk / 2) ? nk / 2 - 1 - j : 3 * nk / 2 - 1 - j;
        u = 2 * ir * ir + ((j < q4) ? j : j - 2 * q4);
    } else {
        const int ir = (k - NWD) / NDISC_AZ;
        int j = k - NWD - ir * NDISC_AZ;
        mir = j >= NDISC_AZ / 2;
        if (mir) j = NDISC_AZ - 1 - j;
        u = U_WD + ir * (NDISC_AZ / 2) + j;
    }
    const double2 ab = AB[uslot(u)];
    return mir ? mirror_ab(ab) : ab;
}

// test/inspection only: per-element weights and the full 400-tile donor
#ifndef LFG_NOLICM_TU  // (lfg_pair_split.hip compiles k_pair only)
__global__ void k_expand(const double* __restrict__ geo, const int* __restrict__ status, int npairs,
                         const double2* __restrict__ AB, const double* __restrict__ DON, double* __restrict__ A,
                         double* __restrict__ B, double* __restrict__ WG, double* __restrict__ DFULL)
{
    const long t = long(blockIdx.x) * blockDim.x + threadIdx.x;
    const int pair = int(t / NEL), k = int(t - long(pair) * NEL);
    if (pair >= npairs || status[pair] != ST_OK) return;
    const double* G = geo + size_t(pair) * LFG_NGEO;
    const double2 ab = elem_ab(AB + size_t(pair) * NELU, k);
    if (A) A[size_t(pair) * NEL + k] = ab.x;
    if (B) B[size_t(pair) * NEL + k] = ab.y;
    double w;
    if (k < NWD) {
        int ir = int(sqrt(k * 0.25));
        if (4 * (ir + 1) * (ir + 1) <= k) ++ir;
        if (4 * ir * ir > k) --ir;
        w = wd_ring_weight(ir, G[G_ULIMB]);
    } else if (k < NWD + NDISC) {
        w = disc_ring_weight((k - NWD) / NDISC_AZ, G);
    } else {
        w = bs_weight(k - NWD - NDISC, G);
    }
    if (WG) WG[size_t(pair) * NEL + k] = w;
    if (DFULL && k < U_DON) {
        const int it = k / (NDONOR_P / 4), ip = k - it * (NDONOR_P / 4);
        const double* v = DON + (size_t(pair) * U_DON + k) * DON_STRIDE;
        const int base = it * NDONOR_P;
        const int ks[4] = {base + ip, base + NDONOR_P - 1 - ip, base + NDONOR_P / 2 - 1 - ip,
                           base + NDONOR_P / 2 + ip};
        const double sy[4] = {1.0, 1.0, -1.0, -1.0}, sz[4] = {1.0, -1.0, 1.0, -1.0};
        double* D = DFULL + size_t(pair) * NDONOR * 3;
        for (int m = 0; m < 4; ++m) {
            D[3 * ks[m]] = v[0];
            D[3 * ks[m] + 1] = sy[m] * v[1];
            D[3 * ks[m] + 2] = sz[m] * v[2];
        }
    }
}
#endif

// --------------------------------------------------------------- k_lnlike
// Cross-lane sums and scans by DPP (no LDS round trips; __shfl_xor /
// __shfl_up would also hoist one address VGPR per offset out of every loop
// and keep it live through k_lnlike).
// v of the lane CTRL's DPP pattern names (0 where the source lane is outside
// the row or the row is not in RM): two 32-bit DPP moves, no LDS round trip
template <int CTRL, int RM>
__device__ __forceinline__ long long dpp64(long long v)
{
    if constexpr (RM == 0xf) {
        // every row enabled: bound_ctrl writes the 0 itself where the source
        // lane is outside the row (no v_mov of an "old" 0 per move)
        const int lo = __builtin_amdgcn_mov_dpp(static_cast<int>(v), CTRL, 0xf, 0xf, true);
        const int hi = __builtin_amdgcn_mov_dpp(static_cast<int>(v >> 32), CTRL, 0xf, 0xf, true);
        return (static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo);
    } else {  // disabled rows keep the old value: 0
        const int lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, RM, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(v >> 32), CTRL, RM, 0xf, false);
        return (static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo);
    }
}

template <int CTRL, int RM>
__device__ __forceinline__ double dppd(double v)
{
    return __longlong_as_double(dpp64<CTRL, RM>(__double_as_longlong(v)));
}

// sum over the wave, the same value in every lane: the DPP inclusive scan
// (row_shr 1, 2, 4, 8, row_bcast:15, row_bcast:31; no LDS round trips, the
// bpermute butterfly waited one per step) and lane 63's total read back
__device__ __forceinline__ double wave_sum(double v)
{
    v += dppd<0x111, 0xf>(v);
    v += dppd<0x112, 0xf>(v);
    v += dppd<0x114, 0xf>(v);
    v += dppd<0x118, 0xf>(v);
    v += dppd<0x142, 0xa>(v);
    v += dppd<0x143, 0xc>(v);
    const long long t = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane(static_cast<int>(t), 63);
    const int hi = __builtin_amdgcn_readlane(static_cast<int>(t >> 32), 63);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}

struct LikeArgs {
    const double* geo;
    const int* status;
    const double2* AB;
    const double* DON;
    const double* WT;
    int E;
    const int* off;  // nullptr: every pair uses x[0..N)
    int N;
    const double* x;
    const double* y;
    const double* ye;
    const double* w;
    int nsub;
    double* flux;   // nullable, [pairs][N]
    double* comps;  // nullable, [4][pairs][N]
    double* lle;    // nullable, [pairs]
    int npairs;
    const int* gp_ecl;  // GP mode: [E][2] first and last changepoint eclipse numbers
    // fused k_combine (MODE 1, 2): ln_prob = ln_prior + sum_e ln_like_e
    const double* prior;  // [W] Prior.ln_prob sums + LCModel prior (k_setup)
    double* lnp;          // nullable, [W]
    bool combine;         // form ln_prob at all
    // fused stretch-move acceptance (lfg_stretch_lnprob_accept; pos nullptr:
    // off): walker w of this batch is the proposal for ensemble walker
    // half * W + w, with W = the batch size = half the ensemble
    double* pos;
    double* lnp_ens;
    const double* qprop;
    const double* zfac;
    int ndim, half;
    unsigned long long seed, step;
    int* naccept;
    double* res;  // MODE 2: [pairs][N] residuals for k_gp_like
    double* gpx;  // MODE 2: [pairs][N] e^{-lam dx} per point (the filter's transitions)
    int* gpb;     // MODE 2: [pairs][N] changepoint block per point
    const int* bstatus;  // fused element phase: the stream lanes' status (folded into status here)
    int* accflag;        // nullable, [W]: 1 where the walker's move was accepted (speculative setup)
};



// ln_prob of walker w once all its eclipses' ln_like are in lle
// (Node.ln_prob, model.py:476-498; what k_combine does), then the
// Metropolis step of the stretch move for it when fused (k_accept's rule)
__device__ inline void combine_walker(const LikeArgs& L, int w)
{
    double lp = L.prior[w];
    for (int e = 0; e < L.E; ++e) {
        const double* G = L.geo + (size_t(w) * L.E + e) * LFG_NGEO;
        lp += G[G_RPRIOR] + G[G_RPRIOR_BS];
    }
    double v;
    if (!isfinite(lp)) {
        for (int e = 0; e < L.E; ++e) L.lle[size_t(w) * L.E + e] = -INFINITY;
        v = -INFINITY;
    } else {
        double ll = 0.0;
        for (int e = 0; e < L.E; ++e) ll += L.lle[size_t(w) * L.E + e];
        v = lp + ll;
    }
    if (L.lnp) L.lnp[w] = v;
    if (L.pos) {
        const int wg = L.half * L.npairs / L.E + w;  // ensemble index (npairs / E = batch walkers)
        const uint4 r = draw(L.seed, L.step, L.half, 1, w);
        const double lu = log(u53(r.x, r.y));
        if (lu < L.zfac[w] + v - L.lnp_ens[wg]) {
            double* p = L.pos + size_t(wg) * L.ndim;
            const double* qi = L.qprop + size_t(w) * L.ndim;
            for (int d = 0; d < L.ndim; ++d) p[d] = qi[d];
            L.lnp_ens[wg] = v;
            if (L.naccept) L.naccept[wg] += 1;
            if (L.accflag) L.accflag[w] = 1;
        } else if (L.accflag) {
            L.accflag[w] = 0;
        }
    }
}

// end of k_lnlike (all threads; lle[pair] written by thread 0): with one
// eclipse per walker and fused acceptance, thread 0 decides with the
// prefetched draw and the copy of the accepted proposal is spread over the
// first ndim lanes; otherwise thread 0 runs combine_after
__device__ inline void finish_walker(const LikeArgs& L, int pair, int tid, bool acc1, const double* sq,
                                     const double* sacc1, int* sflag);

__device__ inline void combine_after(const LikeArgs& L, int pair)
{
    // one eclipse per walker: at once; E > 1: k_combine_walkers does it
    // after the launch (L.combine is false then)
    if (L.combine) combine_walker(L, pair / L.E);
}

// ---- sweeps over phase-sorted tiles of points (MODEL_SPEC 6 restated) ----
// Every eclipse / visibility term is a sum over elements of w_k g_k(p), where
// g_k is non-zero on a contiguous run of points once the points are sorted:
//  * window mode (exposure windows [lo_p, hi_p], lo and hi non-decreasing):
//    element [a, b] overlaps points [P1, P4) and covers [P2, P3) whole, with
//    P1 = #{hi <= a}, P2 = #{lo < a}, P3 = #{hi <= b}, P4 = #{lo < b};
//  * point mode (zero widths, or the donor's visibility arcs): a < ph < b on
//    points [#{ph <= a}, #{ph < b}).
// Whole-covered runs go into a difference array, partly covered points get
// w |[a,b] n [lo,hi]| / (hi - lo) directly.  Sums are 2^-61 fixed point in
// int64 so LDS atomics add them exactly, independent of order.
constexpr int ACC_LDS = 24;  // proposal coordinates of the fused acceptance kept in LDS (the rest re-read)
#ifndef LIKE_MINW
#define LIKE_MINW 4  // minimum waves per SIMD: two 512-lane blocks per CU (<= 128 VGPRs; LDS < 80 KB)
#endif

__device__ __forceinline__ void build_cells(const double* __restrict__ v, int m, int* __restrict__ cell, int tid)
{
    const PhaseIndex X = phase_index(v, cell, m);
    const double t0 = X.t0, ginv = X.ginv;
    auto ci = [&](double x) {
        const double u = (x - t0) * ginv;
        return u < 0.0 ? -1 : (u >= double(LIKE_NC) ? LIKE_NC : int(u));
    };
    if (tid < m) {
        const int g0 = tid ? ci(v[tid - 1]) : -1, g1 = ci(v[tid]);
        for (int g = g0 + 1; g <= g1; ++g) cell[g] = tid;
        if (tid == m - 1)
            for (int g = g1 + 1; g <= LIKE_NC; ++g) cell[g] = m;
    }
}

__device__ __forceinline__ void fx_add(unsigned long long* acc, int p, long long q)
{
    atomicAdd(acc + p, static_cast<unsigned long long>(q));
}

// the sweep's entries (lfg_sweep.hpp) into an LDS difference array
struct FxAdd {
    unsigned long long* acc;
    __device__ __forceinline__ void operator()(int p, long long q) const { fx_add(acc, p, q); }
};

__device__ __forceinline__ void apply_runs(const Runs& R, double a, double b, double wn, const PhaseIndex& X,
                                           const double* __restrict__ hi, const double* __restrict__ iw,
                                           unsigned long long* acc)
{
    lfg::apply_runs(R, a, b, wn, X, hi, iw, FxAdd{acc});
}

template <int NI>
__device__ __forceinline__ void apply_runs_batched(const Runs (&R)[NI], const double (&a)[NI], const double (&b)[NI],
                                                   double wn, const PhaseIndex& X, const double* __restrict__ hi,
                                                   const double* __restrict__ iw, unsigned long long* acc)
{
    lfg::apply_runs_batched<NI>(R, a, b, wn, X, hi, iw, FxAdd{acc});
}

#if LFG_PAIR_SINK_MERGE
// k_pair's sinks: the run ends' adjacent entries summed before they are
// added, where no lane of the wave has a run end of two windows or more (one
// vote of the lanes that hold an eclipsed item; a lane without one is not there)
template <int NI>
__device__ __forceinline__ void apply_runs_merged(const Runs (&R)[NI], const double (&a)[NI], const double (&b)[NI],
                                                  double wn, const PhaseIndex& X, const double* __restrict__ hi,
                                                  const double* __restrict__ iw, unsigned long long* acc)
{
    lfg::apply_runs_merged<NI>(R, a, b, wn, X, hi, iw, FxAdd{acc}, [](bool slow) { return __any(slow) != 0; });
}
#endif

// ring of unique WD/disc item u: WD ring r holds 2 r^2 <= u < 2 (r + 1)^2,
// disc rings follow (NDISC_AZ / 2 items each)
__device__ __forceinline__ int uring(int u)
{
    if (u >= U_WD) return NWD_RINGS + (u - U_WD) / (NDISC_AZ / 2);
    int r = int(sqrtf(float(u) * 0.5f));
    r += (2 * (r + 1) * (r + 1) <= u) ? 1 : 0;
    r -= (2 * r * r > u) ? 1 : 0;
    return r;
}

// the same from the table (k_pair, LFG_PAIR_SINK_MERGE).  k_lnlike keeps
// uring: with the table's load in its sweep the TAB instantiations went from
// 0 / 16 to 16 / 32 B of scratch per lane
__device__ __forceinline__ int pair_ring(int u)
{
#if LFG_PAIR_SINK_MERGE
    return kRingOf[u];
#else
    return uring(u);
#endif
}

// inclusive wave prefix sum: Hillis-Steele within each row of 16 lanes
// (row_shr 1, 2, 4, 8), then row_bcast:15 into rows 1 and 3 and
// row_bcast:31 into rows 2 and 3 (gfx9 DPP).  Six dependent VALU steps; the
// ds_bpermute form waited an LDS round trip per step.
__device__ __forceinline__ long long wave_scan_incl(long long v, int lane)
{
    (void)lane;
    v += dpp64<0x111, 0xf>(v);
    v += dpp64<0x112, 0xf>(v);
    v += dpp64<0x114, 0xf>(v);
    v += dpp64<0x118, 0xf>(v);
    v += dpp64<0x142, 0xa>(v);
    v += dpp64<0x143, 0xc>(v);
    return v;
}

// the wave's total of v (all 64 lanes active), in every lane
__device__ __forceinline__ long long wave_total(long long v)
{
    v = wave_scan_incl(v, 0);
    const int lo = __builtin_amdgcn_readlane(static_cast<int>(v), 63);
    const int hi = __builtin_amdgcn_readlane(static_cast<int>(v >> 32), 63);
    return (static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo);
}

// inclusive prefix of NA difference arrays at index tid (one entry per thread)
// (ext, nullable: second copies of arrays 0 and 1, summed in; the integer
// sums are exact, so the split changes no bit of the result)
template <int NA>
__device__ __forceinline__ void block_scan(unsigned long long (*acc)[LIKE_TILE + 1], long long (*part)[LIKE_THREADS / 64],
                                           int tid, long long* out,
                                           const unsigned long long (*ext)[LIKE_TILE + 1] = nullptr)
{
    const int lane = tid & 63, wv = tid >> 6;
    constexpr int NW = LIKE_THREADS / 64;
    for (int i = 0; i < NA; ++i) {
        const unsigned long long a = acc[i][tid] + ((ext && i < 2) ? ext[i][tid] : 0ull);
        out[i] = wave_scan_incl(static_cast<long long>(a), lane);
        if (lane == 63) part[i][wv] = out[i];
    }
    __syncthreads();
    // exclusive prefix over the waves, formed by every wave for itself (one
    // barrier, not three): lanes 0..NW-1 read the NW wave totals of an array
    // in one LDS read, a 3-step DPP row scan sums them, and lane wv - 1's
    // inclusive prefix is this wave's offset
    static_assert(NW == 8, "wave totals fit one DPP row");
    for (int i = 0; i < NA; ++i) {
        long long t = (lane < NW) ? part[i][lane] : 0;
        t += dpp64<0x111, 0xf>(t);
        t += dpp64<0x112, 0xf>(t);
        t += dpp64<0x114, 0xf>(t);
        if (wv > 0) {
            const int lo = __builtin_amdgcn_readlane(static_cast<int>(t), wv - 1);
            const int hi = __builtin_amdgcn_readlane(static_cast<int>(t >> 32), wv - 1);
            out[i] += (static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo);
        }
    }
}

// k_pair's one-tile likelihood phase (LFG_PAIR_RUNSCAN, default on;
// -DLFG_PAIR_RUNSCAN=0 compiles block_scan<6> by all eight waves, every wave
// running the whole phase, as before).  A config-2 eclipse has 300 points in a
// tile of 512: block_scan<6> cost each of the 8 waves six 6-step 64-bit DPP
// scans and six cross-wave scans for about 1 800 prefix sums in all, and the
// waves above the last point ran the conversions, sincospi, the flux and the
// quotient for nothing.  With the switch on a wave scans one array (run_scan)
// and a wave without a point only reaches the barriers.
#ifndef LFG_PAIR_RUNSCAN
#define LFG_PAIR_RUNSCAN 1
#endif

// inclusive prefix of one difference array over [0, m), in place, by one
// wave (all 64 lanes call it): lane l owns the run [l R, min((l + 1) R, m)),
// R = ceil(m / 64) <= RUN_MAX; it sums its run (ext, nullable: the array's
// second copy, summed in), one wave scan runs over the run totals, and the
// lane writes the running prefix back (long_tables' step (f)).  The sums are
// int64: the order changes no bit.
constexpr int RUN_MAX = LIKE_TILE / 64;
__device__ __forceinline__ void run_scan(unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ ext,
                                         int m, int lane)
{
    const int R = (m + 63) >> 6, p0 = lane * R;
    long long v[RUN_MAX];
    long long own = 0;
#pragma unroll
    for (int k = 0; k < RUN_MAX; ++k) {
        const int p = p0 + k;
        const bool in = k < R && p < m;
        v[k] = in ? static_cast<long long>(acc[p] + (ext ? ext[p] : 0ull)) : 0;
        own += v[k];
    }
    long long run = wave_scan_incl(own, lane) - own;
#pragma unroll
    for (int k = 0; k < RUN_MAX; ++k) {
        const int p = p0 + k;
        run += v[k];
        if (k < R && p < m) acc[p] = static_cast<unsigned long long>(run);
    }
}

__device__ __forceinline__ double wrap_phase(double ph) { return ph - floor(ph + 0.5); }

// sincospi out of line: inlined into the tile loop, its polynomial constants
// are hoisted into ~20 loop-invariant VGPRs
// sin, cos of pi x and of pi y in one call (the sub-bin queries: the line of
// sight at the first sub-bin and its turn per sub-bin)
__device__ __noinline__ double4 sincospi2_ool(double x, double y)
{
    double sx, cx, sy, cy;
    sincospi(x, &sx, &cx);
    sincospi(y, &sy, &cy);
    return make_double4(sx, cx, sy, cy);
}

__device__ __noinline__ double2 sincospi_ool(double x)
{
    double sn, cs;
    sincospi(x, &sn, &cs);
    return make_double2(sn, cs);
}

// tile buffers of one sweep pass: windows [lo, hi] with inverse widths, and
// the sub-bin centre phases (donor), each with its cell index
struct TileBufs {
    double lo[LIKE_TILE], hi[LIKE_TILE], iw[LIKE_TILE];
    int cell[LIKE_NC + 1];
};

// writes this thread's window; returns 4 for an invalid width (check_sorted
// returns 4 for an out-of-order window): either sends the tile to the direct path
__device__ __forceinline__ int put_window(TileBufs& T, int tid, bool own, double ph, double hw)
{
    if (!own) return 0;
    T.lo[tid] = ph - hw;
    T.hi[tid] = ph + hw;
    T.iw[tid] = 1.0 / (2.0 * hw);
    return (hw >= 0.0) ? 0 : 4;  // negative or NaN widths take the direct path
}

__device__ __forceinline__ int check_sorted(const TileBufs& T, int tid, bool own)
{
    return (own && tid && (T.lo[tid] < T.lo[tid - 1] || T.hi[tid] < T.hi[tid - 1])) ? 4 : 0;
}

// spot element (lane < NBS) and donor tile (last NDONOR lanes) contributions
// of one sub-bin pass into acc[0] (spot eclipse) and acc[1..3] (donor sum v)
__device__ __forceinline__ void sweep_spot_donor(int tid, const PhaseIndex& XW, const TileBufs& TW,
                                                 const PhaseIndex& XP, const double2* sab, const double* sbw,
                                                 double itb, const double* sdq, double ivs,
                                                 unsigned long long (*acc)[LIKE_TILE + 1])
{
    if (tid < NBS) {
        const double2 abB = sab[tid];
        const double wB = sbw[tid] * itb;
        if (abB.x < abB.y) apply_runs(element_runs(abB.x, abB.y, XW, TW.hi), abB.x, abB.y, wB, XW, TW.hi, TW.iw, acc[0]);
    } else if (tid >= LIKE_THREADS - NDONOR) {
        const int mr = (tid - (LIKE_THREADS - NDONOR)) & 3;
        const double* dq = sdq + ((tid - (LIKE_THREADS - NDONOR)) >> 2) * DON_STRIDE;
        const double vx = dq[0], vy = (mr & 1) ? -dq[1] : dq[1], vz = (mr & 2) ? -dq[2] : dq[2];
        const double cen = (mr & 1) ? -dq[3] : dq[3];
        const double hw = (mr & 2) ? 0.5 - dq[4] : dq[4];
        if (hw > 0.0) {
            const long long qx = to_fx(vx * ivs), qy = to_fx(vy * ivs), qz = to_fx(vz * ivs);
            // visible for phases in (cen - hw, cen + hw) mod 1
            double x1 = -INFINITY, x2 = INFINITY, y1 = 0.0, y2 = 0.0;
            bool two = false;
            if (hw < 0.5) {
                const double lo = cen - hw, hi = cen + hw;
                if (lo < -0.5) { x2 = hi; y1 = lo + 1.0; y2 = INFINITY; two = true; }
                else if (hi > 0.5) { x1 = lo; y1 = -INFINITY; y2 = hi - 1.0; two = true; }
                else { x1 = lo; x2 = hi; }
            }
            for (int i = 0; i < (two ? 2 : 1); ++i) {
                const int P = count_below<true>(XP, i ? y1 : x1), Q = count_below<false>(XP, i ? y2 : x2);
                if (P < Q) {
                    fx_add(acc[1], P, qx);
                    fx_add(acc[2], P, qy);
                    fx_add(acc[3], P, qz);
                    if (Q < XP.m) {
                        fx_add(acc[1], Q, -qx);
                        fx_add(acc[2], Q, -qy);
                        fx_add(acc[3], Q, -qz);
                    }
                }
            }
        }
    }
}

// direct (point-major) WD and disc eclipse fractions of one window: the
// fallback for unsorted or mixed windows.  Inlined: k_lnlike takes it as a
// whole pass of its own, where little is live (an out-of-line call anywhere
// in the kernel spilled ~14 live values to scratch in every block)
__device__ __forceinline__ double2 direct_wd_disc(const double2* __restrict__ AB, const double* __restrict__ swr,
                                               double phc, double wk, double twd, double td)
{
    double ewd = 0.0, ed = 0.0;
    const double lo = phc - wk, hi = phc + wk;
    // MODEL_SPEC 3: a width below the spacing of the doubles at phc (hi == lo) leaves no window either and is
    // the point evaluation, as a zero one is; "nothing overlaps" would be flux 1 inside an eclipse
    const bool window = hi > lo;
    auto cover = [&](double2 ab) {
        return window ? fmax(fmin(ab.y, hi) - fmax(ab.x, lo), 0.0) : ((phc > ab.x && phc < ab.y) ? 1.0 : 0.0);
    };
    for (int ring = 0; ring < NWD_RINGS + NDISC_R; ++ring) {  // each unique item and its mirror
        const int u0 = ring < NWD_RINGS ? 2 * ring * ring : U_WD + (ring - NWD_RINGS) * (NDISC_AZ / 2);
        const int u1 = ring < NWD_RINGS ? 2 * (ring + 1) * (ring + 1) : u0 + NDISC_AZ / 2;
        double acc = 0.0;
        for (int u = u0; u < u1; ++u) {
            const double2 ab = AB[uslot(u)];
            acc += cover(ab) + cover(mirror_ab(ab));
        }
        if (ring < NWD_RINGS) ewd = fma(swr[ring], acc, ewd); else ed = fma(swr[ring], acc, ed);
    }
    const double nrm = window ? 1.0 / (2.0 * wk) : 1.0;
    return make_double2(ewd * nrm * (1.0 / twd), ed * nrm * (1.0 / td));
}

// direct (point-major) spot eclipse fraction of one window
__device__ __forceinline__ double direct_spot(const double2* ABs, const double* sbw, double ph, double h, double itb)
{
    double eb = 0.0;
    const double l2 = ph - h, h2 = ph + h;
    for (int k = 0; k < NBS; ++k) {
        const double2 ab = ABs[k];
        eb = fma(sbw[k], (h2 > l2) ? fmax(fmin(ab.y, h2) - fmax(ab.x, l2), 0.0)  // MODEL_SPEC 3, as direct_wd_disc
                                   : ((ph > ab.x && ph < ab.y) ? 1.0 : 0.0), eb);
    }
    return eb * ((h2 > l2) ? 1.0 / (2.0 * h) : 1.0) * itb;
}

// direct donor sum for one line of sight e = (e0, e1, c)
__device__ __forceinline__ double direct_donor(const double* DONp, double e0, double e1, double c)
{
    double D = 0.0;
    for (int q = 0; q < U_DON; ++q) {
        // max(A + Y, 0) + max(A - Y, 0) = max(A + max(Y, A), 0), A = vx e0 +- vz c
        const double* d5 = DONp + q * DON_STRIDE;
        const double y = fabs(d5[1] * e1), z = d5[2] * c;
        const double A1 = fma(d5[0], e0, z), A2 = fma(d5[0], e0, -z);
        D += fmax(A1 + fmax(y, A1), 0.0) + fmax(A2 + fmax(y, A2), 0.0);
    }
    return D;
}



// ---- S > 1: the spot and donor from per-pair breakpoint tables ----
// With sub-bins the spot's eclipse and the donor's visibility are needed at
// N S sub-phases.  Instead of one sweep (every spot element and donor tile
// located in the pass's windows, a block scan) per tile and sub-bin, the
// pair's breakpoints are bucketed once into TCELLS uniform cells (counting
// sort in LDS) with int64 fixed-point prefix sums per cell, and every
// sub-bin is a lookup: the prefix of its cell plus the few entries of the
// cell (MODEL_SPEC 3, 5.3-5.4 restated; the sums are exact integers, so
// entry order inside a cell does not matter).
//  * donor (point mode at the sub-bin centre th): V(th) = sum of the tile
//    vectors visible at th; tile arc (cen - hw, cen + hw) mod 1: +q at its
//    start (counted for th > start), -q at its end (counted for th >= end);
//    arcs wrapping past +-1/2 and always-visible tiles go into V0, and
//    breakpoints outside the cells' range [t0, t1] are folded into V0 or dropped;
//  * spot (window [lo, hi]): E = C(lo) + [sum over elements with a
//    breakpoint inside (lo, hi) of the partial overlaps] / (hi - lo), with
//    C(x) = the weight of the elements covering x (a_k <= x < b_k): +W_k at
//    a_k, -W_k at b_k, both counted for x >= pos.  Zero-width windows: the
//    elements with a_k < ph < b_k.
constexpr int TCELLS = 256;
constexpr int TD_MAX = 2 * NDONOR, TS_MAX = 2 * NBS;
struct SubTables {
    long long dpre[TCELLS][3];   // donor: V at each cell's start (V0 + cells below), fixed point
    long long spre[TCELLS];      // spot: covering weight at each cell's start
    int dend[TCELLS], send[TCELLS];  // entry counts -> exclusive offsets -> (after the scatter) cell ends
    double spos[TS_MAX];
    int scode[TS_MAX];           // element k: 2 k + (1: end b_k)
    long long dv0[3];
    double dt0, dginv, st0, sginv;
};
struct SubEntries {              // donor entries (in sacc rows 2..5: free when S > 1)
    double dpos[TD_MAX];
    int dcode[TD_MAX];           // tile t (0..399 as the donor lanes number them): 2 t + (1: end)
};
static_assert(sizeof(SubEntries) <= 4 * (LIKE_TILE + 1) * sizeof(unsigned long long), "donor entries fit sacc[2..5]");

__device__ __forceinline__ int tcell(double x, double t0, double ginv)
{
    const double u = (x - t0) * ginv;
    return u <= 0.0 ? 0 : (u >= double(TCELLS - 1) ? TCELLS - 1 : int(u));
}

// donor tile t's fixed-point vector (mirror image t & 3 of unique tile t >> 2),
// exactly as its lane forms it
__device__ __forceinline__ void donor_q(const double* sdq, int t, double ivs, long long& qx, long long& qy, long long& qz)
{
    const int mr = t & 3;
    const double* dq = sdq + (t >> 2) * DON_STRIDE;
    qx = to_fx(dq[0] * ivs);
    qy = to_fx(((mr & 1) ? -dq[1] : dq[1]) * ivs);
    qz = to_fx(((mr & 2) ? -dq[2] : dq[2]) * ivs);
}

// wave-wide min / max, every lane: DPP row shifts as wave_sum does, with each
// lane's own value standing in where the source lane is absent (the
// min / max identity), then lane 63's result
template <bool MAX>
__device__ __forceinline__ double wave_ext(double v)
{
    auto step = [&](auto ctrl_tag, auto rm_tag) {
        constexpr int CTRL = decltype(ctrl_tag)::value, RM = decltype(rm_tag)::value;
        const long long b = __double_as_longlong(v);
        const int lo = __builtin_amdgcn_update_dpp(static_cast<int>(b), static_cast<int>(b), CTRL, RM, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp(static_cast<int>(b >> 32), static_cast<int>(b >> 32), CTRL, RM, 0xf,
                                                   false);
        const double o = __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
        v = MAX ? fmax(v, o) : fmin(v, o);
    };
    using I = std::integral_constant<int, 0>;
    (void)sizeof(I);
    step(std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});
    step(std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});
    const long long t = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane(static_cast<int>(t), 63);
    const int hi = __builtin_amdgcn_readlane(static_cast<int>(t >> 32), 63);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}
// OR of the low four bits of v over the wave (four ballots)
__device__ __forceinline__ int wave_or4(int v)
{
    return (__ballot(v & 1) ? 1 : 0) | (__ballot(v & 2) ? 2 : 0) | (__ballot(v & 4) ? 4 : 0) | (__ballot(v & 8) ? 8 : 0);
}
__device__ __forceinline__ double wave_min(double v) { return wave_ext<false>(v); }
__device__ __forceinline__ double wave_max(double v) { return wave_ext<true>(v); }

// exclusive prefix over TCELLS cells of NA int64 arrays held one cell per
// thread (threads >= TCELLS pass zeros); totals of each wave through part[]
template <int NA>
__device__ __forceinline__ void cell_scan(long long (&v)[NA], long long (*part)[LIKE_THREADS / 64], int tid)
{
    const int lane = tid & 63, wv = tid >> 6;
    long long incl[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        incl[i] = wave_scan_incl(v[i], lane);
        if (lane == 63) part[i][wv] = incl[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        long long off = 0;
        for (int k = 0; k < wv; ++k) off += part[i][k];
        v[i] = incl[i] - v[i] + off;
    }
}

// spot eclipse fraction of window [lo, hi] (h = (hi - lo) / 2; h = 0: point ph = lo)
__device__ __forceinline__ double sub_spot(const SubTables& T, const double2* sab, const double* sbw, double itb,
                                           double lo, double hi, double amin, double bmax)
{
    const bool pt = !(hi > lo);
    if (pt ? !(lo > amin && lo < bmax) : !(hi > amin && lo < bmax)) return 0.0;
    const int g0 = tcell(lo, T.st0, T.sginv), g1 = pt ? g0 : tcell(hi, T.st0, T.sginv);
    long long C = T.spre[g0];
    double corr = 0.0;
    for (int g = g0; g <= g1; ++g) {
        for (int i = g ? T.send[g - 1] : 0; i < T.send[g]; ++i) {
            const double pos = T.spos[i];
            const int code = T.scode[i], k = code >> 1;
            const bool end = code & 1;
            if (g == g0 && pos <= lo) {
                const long long W = to_fx(sbw[k] * itb);
                // point mode: eclipsed when a_k < ph < b_k (MODEL_SPEC 5; the oracle's rule)
                C += end ? -W : ((pt && pos == lo) ? 0 : W);
            } else if (!pt && pos < hi) {
                const double2 ab = sab[k];
                const double wn = sbw[k] * itb;
                if (!end) corr = fma(wn, fmin(ab.y, hi) - ab.x, corr);
                else if (ab.x <= lo) corr = fma(-wn, hi - ab.y, corr);
            }
        }
    }
    const double e = double(C) * FX_INV;
    return pt ? e : fma(corr, 1.0 / (hi - lo), e);
}

// covering weight C(lo) of the spot (fixed point) from the cell table, and
// the cursor: the first entry (cells sorted by position) past lo
__device__ __forceinline__ long long spot_C(const SubTables& T, const double* sbw, double itb, double lo, int& cur)
{
    const int g = tcell(lo, T.st0, T.sginv);
    long long C = T.spre[g];
    int i = g ? T.send[g - 1] : 0;
    for (const int ie = T.send[g]; i < ie && T.spos[i] <= lo; ++i) {
        const int code = T.scode[i];
        const long long W = to_fx(sbw[code >> 1] * itb);
        C += (code & 1) ? -W : W;
    }
    cur = i;
    return C;
}

// donor entries sorted (after step (e) of the table build) by position,
// an end before a start at equal positions: the entries counted at phase th
// (starts with pos < th, ends with pos <= th) are then a prefix of the list,
// and a lane walking up in phase keeps a cursor into it
__device__ __forceinline__ bool donor_counted(double pos, int code, double th)
{
    return (code & 1) ? pos <= th : pos < th;
}

__device__ __forceinline__ void donor_apply(const double* sdq, int code, double ivs, long long& vx, long long& vy,
                                            long long& vz)
{
    long long qx, qy, qz;
    donor_q(sdq, code >> 1, ivs, qx, qy, qz);
    if (code & 1) { vx -= qx; vy -= qy; vz -= qz; }
    else { vx += qx; vy += qy; vz += qz; }
}

// donor sum vector V (fixed point) at phase th, and the cursor: the first
// entry not counted at th
__device__ __forceinline__ int sub_donor(const SubTables& T, const SubEntries& D, const double* sdq, double ivs,
                                         double th, long long& vx, long long& vy, long long& vz)
{
    const int g = tcell(th, T.dt0, T.dginv);
    vx = T.dpre[g][0];
    vy = T.dpre[g][1];
    vz = T.dpre[g][2];
    int i = g ? T.dend[g - 1] : 0;
    for (const int ie = T.dend[g]; i < ie; ++i) {
        const int code = D.dcode[i];
        if (!donor_counted(D.dpos[i], code, th)) break;
        donor_apply(sdq, code, ivs, vx, vy, vz);
    }
    return i;
}


// this lane's breakpoints of the S > 1 tables (<= 2): donor tile t (lanes
// nt - NDONOR ..) or spot element (lanes < NBS); formed twice (count, then
// scatter) instead of held across the barriers between.  v0: how many times
// the tile's vector goes into V0 (+-1, 0)
__device__ __forceinline__ void lane_breakpoints(int tid, const double* sdq, const double2* sab, double t0d, double t1d,
                                                 double& p0, double& p1, bool& in0, bool& in1, int& v0)
{
    // slot 0: the start (code 2 x), slot 1: the end (code 2 x + 1); fixed
    // slots (a compacted pair indexed by a count went to scratch)
    in0 = in1 = false;
    p0 = p1 = 0.0;
    v0 = 0;
    if (tid >= LIKE_THREADS - NDONOR) {
        const int t = tid - (LIKE_THREADS - NDONOR), mr = t & 3;
        const double* dq5 = sdq + (t >> 2) * DON_STRIDE;
        const double cen = (mr & 1) ? -dq5[3] : dq5[3];
        const double hw = (mr & 2) ? 0.5 - dq5[4] : dq5[4];
        if (!(hw > 0.0)) return;
        double sp = NAN, ep = NAN;  // start (counted for th > sp), end (counted for th >= ep)
        if (hw >= 0.5) {
            v0 = 1;
        } else {
            const double lo = cen - hw, hi = cen + hw;
            if (lo < -0.5) { v0 = 1; ep = hi; sp = lo + 1.0; }
            else if (hi > 0.5) { v0 = 1; ep = hi - 1.0; sp = lo; }
            else { sp = lo; ep = hi; }
        }
        if (sp == sp) {  // a start below the range counts for every phase; at or above t1 for none
            if (sp < t0d) v0 += 1;
            else if (sp < t1d) { p0 = sp; in0 = true; }
        }
        if (ep == ep) {
            if (ep <= t0d) v0 -= 1;
            else if (ep <= t1d) { p1 = ep; in1 = true; }
        }
    } else if (tid < NBS) {
        const double2 ab = sab[tid];
        if (ab.x < ab.y) {
            p0 = ab.x;
            p1 = ab.y;
            in0 = in1 = true;
        }
    }
}


// S > 1: the spot and donor terms of one point, summed over its S sub-bins
// (spot eclipse over each sub-bin window, donor at each sub-bin centre, from
// the tables).  The donor vector is looked up at the first sub-bin and
// carried forward by the sorted-entry cursor (the next entry's position in
// registers: usually one compare per sub-bin), and the line of sight is
// rotated from sub-bin to sub-bin (one sincospi per point); a sub-bin past
// +-1/2 starts over.  The beaming denominator and the donor normalisation
// divide the point's sums once.
__device__ __forceinline__ double2 sub_point(const SubTables& T, const SubEntries& D, const double2* sab, const double* sbw,
                                             const double* sdq, const double* snorm, const double* shull, const double* SG,
                                             double ph0, double wk, int S)
{
    // the pair's constants are read from LDS at each use (volatile: held in
    // registers over the loop they pushed k_lnlike past its budget)
    // (LDS address space spelled out: through volatile generic pointers the
    // reads were flat loads, which wait on the vector-memory counter too)
    using lds_cvd = const volatile __attribute__((address_space(3))) double*;
    const lds_cvd VG = (lds_cvd)SG;
    const lds_cvd VN = (lds_cvd)snorm;
    const int nd = T.dend[TCELLS - 1], nsp = T.send[TCELLS - 1];
    const double h = wk / S, ih = 0.5 / h;
    double sbs = 0.0, srs = 0.0, ph = 0.0, sn = 0.0, cs = 1.0, rs = 0.0, rc = 1.0;
    double fx = 0.0, fy = 0.0, fz = 0.0, npos = INFINITY;
    long long vx = 0, vy = 0, vz = 0, Cs = 0;
    int cur = 0, ncode = 0, scur = 0;
    bool sv = false;  // Cs / scur hold C at this sub-bin's lo
    for (int j = 0; j < S; ++j) {
        const double phn = wrap_phase(ph0 - wk + (2 * j + 1) * h);
        bool chg = false;
        if (j == 0 || !(phn >= ph)) {  // a fresh lookup
            sv = false;
#ifdef LFG_ABL_FRESH  // diagnostic ablation: no donor table lookup
            cur = nd;
#else
            cur = sub_donor(T, D, sdq, VN[1], phn, vx, vy, vz);
#endif
            chg = true;
            const double4 e4 = sincospi2_ool(2.0 * phn, 4.0 * h);  // the turn per sub-bin: 2 pi (2 h)
            sn = e4.x;
            cs = e4.y;
            rs = e4.z;
            rc = e4.w;
        } else {
            while (donor_counted(npos, ncode, phn)) {  // npos = inf past the last entry
                donor_apply(sdq, ncode, VN[1], vx, vy, vz);
                chg = true;
                ++cur;
                npos = cur < nd ? D.dpos[cur] : INFINITY;
                ncode = cur < nd ? D.dcode[cur] : 0;
            }
            const double c2 = fma(cs, rc, -sn * rs);
            sn = fma(sn, rc, cs * rs);
            cs = c2;
        }
        if (chg) {
            if (j == 0 || !(phn >= ph)) {
                npos = cur < nd ? D.dpos[cur] : INFINITY;
                ncode = cur < nd ? D.dcode[cur] : 0;
            }
            fx = double(vx);
            fy = double(vy);
            fz = double(vz);
        }
        ph = phn;
        // spot: windows of a point abut, so C(lo) is carried from window to
        // window by a cursor over the position-sorted entries (the entries
        // inside a window give its partial overlaps); zero widths: points
        double ebj = 0.0;
        const double lo = ph - h, hi = ph + h;
#ifdef LFG_ABL_SPOT  // diagnostic ablation: no spot eclipse
        if (false) {
#else
        if (!(h > 0.0)) {
#endif
            ebj = sub_spot(T, sab, sbw, VN[0], lo, hi, shull[2], shull[3]);
        } else if (hi > shull[2] && lo < shull[3]) {
            const double itb = VN[0];
            if (!sv) Cs = spot_C(T, sbw, itb, lo, scur);
            sv = true;
            long long Cn = Cs;
            double corr = 0.0;
            for (; scur < nsp && T.spos[scur] <= hi; ++scur) {
                const int code = T.scode[scur], k = code >> 1;
                const double wn = sbw[k] * itb;
                const double2 ab = sab[k];
                const long long W = to_fx(wn);
                if (!(code & 1)) {
                    Cn += W;
                    corr = fma(wn, fmin(ab.y, hi) - ab.x, corr);
                } else {
                    Cn -= W;
                    if (ab.x <= lo) corr = fma(-wn, hi - ab.y, corr);
                }
            }
            ebj = fma(corr, ih, double(Cs) * FX_INV);
            Cs = Cn;
        } else {
            sv = false;
        }
        const double sg = VG[G_S], cg = VG[G_C];
        const double e0 = sg * cs, e1 = -sg * sn;
        srs = fma(e0, fx, fma(e1, fy, fma(cg, fz, srs)));
        const double fis = VG[G_FIS];
        sbs = fma(fis + (1.0 - fis) * fmax(VG[G_NB0] * e0 + VG[G_NB1] * e1 + VG[G_NB2] * cg, 0.0), 1.0 - ebj, sbs);
    }
    const double bden = VG[G_BDEN];
    return make_double2(bden > 0.0 ? sbs / bden : 0.0, srs * (FX_INV * VN[3]) / VN[2]);
}

#ifdef LFG_PROFILE_LIKE  // diagnostic build only: phase stamps (first tile) into spare geo slots 41..46
// (thread 0), and the earliest / latest wave of each block per phase (g_like_wav)
__device__ unsigned long long g_like_wav[2][6][4096];
#ifdef LFG_PROFILE_LIKE_WAVES  // per-wave stamps (global atomics: they perturb the timing)
constexpr bool LIKE_WAVES = true;
#else
constexpr bool LIKE_WAVES = false;
#endif
#define LIKE_STAMP(i)                                                                                       \
    if (t0 == 0) {                                                                                          \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime() - tstart;                             \
        if (tid == 0) const_cast<double*>(G)[41 + (i)] = double(now_);                                       \
        if (LIKE_WAVES && lane == 0 && blockIdx.x < 4096) {                                                  \
            atomicMin(&g_like_wav[0][i][blockIdx.x], now_);                                                  \
            atomicMax(&g_like_wav[1][i][blockIdx.x], now_);                                                  \
        }                                                                                                   \
    }
// prologue stamps of thread 0 (and of the block's last lane) per block: lfg_debug_like_cycles
__device__ unsigned long long g_like_cyc[8][4096];
#define LIKE_PRO(k)                                                                                 \
    if ((tid == 0 || tid == LIKE_THREADS - 1) && blockIdx.x < 4096)                                  \
        g_like_cyc[(k) + (tid ? 4 : 0)][blockIdx.x] = __builtin_amdgcn_s_memtime() - tstart
#else
#define LIKE_STAMP(i)
#define LIKE_PRO(k)
#endif

__device__ inline void finish_walker(const LikeArgs& L, int pair, int tid, bool acc1, const double* sq,
                                     const double* sacc1, int* sflag)
{
    if (!acc1) {
        if (tid == 0) combine_after(L, pair);
        return;
    }
    __syncthreads();  // sflag is free; lle[pair] is this block's own write
    const int wg = L.half * L.npairs + pair;
    if (tid == 0) {
        const double* G = L.geo + size_t(pair) * LFG_NGEO;
        const double lp = L.prior[pair] + G[G_RPRIOR] + G[G_RPRIOR_BS];
        double v;
        if (!isfinite(lp)) {
            L.lle[pair] = -INFINITY;
            v = -INFINITY;
        } else {
            v = lp + L.lle[pair];
        }
        if (L.lnp) L.lnp[pair] = v;
        const bool a = sacc1[0] < sacc1[1] + v - sacc1[2];
        if (a) {
            L.lnp_ens[wg] = v;
            if (L.naccept) L.naccept[wg] += 1;
        }
        sflag[0] = a ? 1 : 0;
        if (L.accflag) L.accflag[pair] = a ? 1 : 0;
    }
    __syncthreads();
    if (sflag[0] && tid < L.ndim)
        L.pos[size_t(wg) * L.ndim + tid] = (tid < ACC_LDS) ? sq[tid] : L.qprop[size_t(pair) * L.ndim + tid];
}

// MODE 0: flux (and components) only; 1: fused chi^2 -> ln_like; 2: GP
// ln_like of the residuals (a Kalman filter over each tile's sorted points,
// run by wave 0 while the other waves wait at the tile barrier)
// SUB: nsub > 1 (the table path for the spot and donor, MODE as above); the
// host launches SUB = (nsub > 1), so each instantiation holds only its path
template <int MODE, bool SUB>
__global__ __launch_bounds__(LIKE_THREADS, LIKE_MINW) void k_lnlike(LikeArgs L)
{
    constexpr bool CHI = MODE != 0, GP = MODE == 2;
#ifdef LFG_PROFILE_LIKE
    const unsigned long long tstart = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) {  // block start (100 MHz wall clock) and the CU it runs on
        const_cast<double*>(L.geo)[size_t(blockIdx.x) * LFG_NGEO + 47] = double(__builtin_amdgcn_s_memrealtime());
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        const_cast<double*>(L.geo)[size_t(blockIdx.x) * LFG_NGEO + 40] = double(hw);
    }
#endif
    __shared__ double swr[NWD_RINGS + NDISC_R];
    __shared__ double swn[NWD_RINGS + NDISC_R];  // ring weights / component totals (the sweep's wn)
    __shared__ double sbw[NBS];
    __shared__ double2 sab[NBS];                  // spot intervals
    __shared__ double sdq[U_DON * DON_STRIDE];    // unique donor tiles
    __shared__ double sacc1[3];                   // fused acceptance: ln u, zfac, old ln_prob
    __shared__ double snorm[4];                   // 1 / spot total, 1 / donor |v| sum, donor norm, |v| sum
    __shared__ double sgeo[LFG_NGEO];             // the pair's geometry record, read at use in the tile loop
    // TA: WD/disc windows.  S = 1: the spot sweep reuses TA's windows, and
    // SU.s1.X holds second copies of the WD and disc difference arrays, taken
    // by the odd lanes of the sweep (half the same-address LDS atomics where
    // contacts cluster; four WD copies measured no faster), sph / scp the
    // donor's phases and their cells.  S > 1: SU.tb, the pair's breakpoint
    // tables (spot and donor), with the donor entries in sacc rows 2..5.
    __shared__ TileBufs TA;
    __shared__ union SubU_ {
        struct {
            unsigned long long X[2][LIKE_TILE + 1];
            double sph[LIKE_TILE];  // point phases (donor)
            int scp[LIKE_NC + 1];
        } s1;
        SubTables tb;
    } SU;
    double* const sph = SU.s1.sph;
    int* const scp = SU.s1.scp;
    __shared__ double shull[4];  // WD/disc and spot element hulls: min a, max b (eclipsed elements)
    __shared__ double shw[4][LIKE_THREADS / 64];  // their wave partials
    __shared__ double sqr[2][LIKE_THREADS / 64];  // S > 1: wave partials of the sub-bin phase range
    __shared__ unsigned long long sacc[6][LIKE_TILE + 1];
    __shared__ long long spart[6][LIKE_THREADS / 64];
    __shared__ double red[3][LIKE_THREADS / 64];
    __shared__ int sflag[2];

    constexpr int nt = LIKE_THREADS, nw = LIKE_THREADS / 64;
    const int pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int e = (L.E == 1) ? 0 : pair % L.E;  // (one eclipse: no division constants held)
    // one eclipse: off = {0, max_n} (lfg.h), so the point loads need not
    // wait on a load of the offsets (one memory round trip of the prologue)
    const bool offs = L.off && L.E > 1;
    const int o0 = offs ? L.off[e] : 0;
    const int n = offs ? L.off[e + 1] - o0 : L.N;
    const double* G = L.geo + size_t(pair) * LFG_NGEO;
    const double* Wt = L.WT + size_t(pair) * WT_N;
    const double2* AB = L.AB + size_t(pair) * NELU;
    const double* DONp = L.DON + size_t(pair) * U_DON * DON_STRIDE;
    // tree calls: a walker whose ln_prior is -inf was not solved by k_elements
    // (prior_rejects); the pair goes straight to the -inf finish (a local
    // status value only: the status array keeps the model's own code)
    constexpr int ST_PRIOR_SKIP = -1;
    const bool prej = CHI && L.prior && prior_rejects(L.prior[L.E == 1 ? pair : pair / L.E], G);
    if constexpr (GP) {
        // the Kalman filter's state-independent factors of the pair's points
        // (e^{-lam dx}, changepoint block), for k_gp_like: one point per
        // thread here instead of ~60 instructions per point in the filter's
        // serial lane (formed before the prologue: no registers held)
        const double lam = G[G_GP_LAM], dcp = G[G_GP_DCP], ph0 = G[G_PHI0];
        const int ge0 = L.gp_ecl[2 * e], ge1 = L.gp_ecl[2 * e + 1];
        for (int p = tid; p < n; p += LIKE_THREADS) {
            const double xp = L.x[o0 + p];
            const double dx = xp - (p > 0 ? L.x[o0 + p - 1] : xp);
            const size_t q = size_t(pair) * L.N + p;
            L.gpx[q] = exp(-(lam * dx));
            L.gpb[q] = gp_block(xp, ge0, ge1, dcp, ph0);
        }
    }

    // fused acceptance with one eclipse per walker: the proposal's coordinates
    // (one per lane), the uniform draw and the old ln_prob are fetched here,
    // off the tail of the block (combine_walker does it for E > 1)
    const bool acc1 = CHI && !GP && L.pos && L.E == 1;
    // the proposal's coordinates wait in LDS (a register held through the
    // whole block would be spilled: the kernel is at its 128-VGPR budget)
    __shared__ double sq[ACC_LDS];
    if (acc1 && tid < L.ndim && tid < ACC_LDS) sq[tid] = L.qprop[size_t(pair) * L.ndim + tid];
    // each thread's own data point y, ye: fetched with the prologue's loads
    // into this thread's LDS slot (no registers held through the passes, and
    // no memory round trip where chi^2 is formed)
    __shared__ double sy[CHI ? LIKE_TILE : 1], sye[CHI ? LIKE_TILE : 1];
    if (CHI && tid < n) {
        sy[tid] = L.y[o0 + tid];
        if (!GP) sye[tid] = L.ye[o0 + tid];
    }
    int st;
    double s, c, ul, td;
    double px = 0.0, pw = 0.0;  // tile-0 point of this thread (y, ye: read where chi^2 is formed)
    // this thread's sweep items, held in registers for every tile: WD/disc
    // elements tid + i nt (sweep_ab) with their ring weights, spot element
    // tid (< NBS), donor tile (last NDONOR lanes)
    constexpr int NI = (NWD + NDISC + nt - 1) / nt;
    double2 abk[NI];
    double2 abB = make_double2(1.0, -1.0);
    double wB = 0.0;
    double dq[DON_STRIDE] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double gv = 0.0;     // one geometry word per lane for sgeo
    double wring = 0.0;  // ring weights for the direct path
    // every global load of the prologue is issued before anything waits on
    // one (the status included): a single memory round trip
    st = L.status[pair];
    if (st == ST_OK && prej) st = ST_PRIOR_SKIP;
    s = G[G_S];
    c = G[G_C];
    ul = G[G_ULIMB];
    td = Wt[WT_TD];
    if (!SUB && tid < n) {  // (S > 1: at the first tile, after the table build it would be held through)
        px = L.x[o0 + tid];
        pw = L.w ? L.w[o0 + tid] : 0.0;
    }
    for (int i = 0; i < NI; ++i) {
        const int g = tid + i * nt;
        abk[i] = (g < NWD + NDISC) ? sweep_ab(AB, g) : make_double2(1.0, -1.0);
    }
    if (tid < NBS) {
        abB = AB[NU_WDD + tid];
        wB = Wt[WT_BS + tid];
    } else if (tid >= nt - NDONOR) {
        const int t = tid - (nt - NDONOR);
        for (int i = 0; i < DON_STRIDE; ++i) dq[i] = DONp[(t >> 2) * DON_STRIDE + i];
    }
    if (tid >= NBS + NWD_RINGS + NDISC_R && tid < NBS + NWD_RINGS + NDISC_R + G_COUNT)
        gv = G[tid - (NBS + NWD_RINGS + NDISC_R)];
    if (tid >= NBS && tid < NBS + NWD_RINGS) wring = wd_ring_weight(tid - NBS, ul);
    else if (tid >= NBS + NWD_RINGS && tid < NBS + NWD_RINGS + NDISC_R)
        wring = Wt[WT_DISC + tid - NBS - NWD_RINGS];
    // the acceptance draw by the block's last lane, after its prologue loads
    // are in flight (in wave 0 the Philox rounds and the log delayed every
    // load of that wave's prologue)
    if (acc1 && tid == nt - 1) {
        const uint4 r = draw(L.seed, L.step, L.half, 1, pair);
        sacc1[0] = log(u53(r.x, r.y));
        sacc1[1] = L.zfac[pair];
        sacc1[2] = L.lnp_ens[L.half * L.npairs + pair];
    }

    LIKE_PRO(0);
    if (st != ST_OK) {
        for (int p = tid; p < n && !CHI; p += nt) {  // flux outputs: MODE 0 only (the tree paths pass none)
            if (L.flux) L.flux[size_t(pair) * n + p] = NAN;
            if (L.comps)
                for (int m = 0; m < 4; ++m) L.comps[(size_t(m) * L.npairs + pair) * n + p] = NAN;
        }
        if (CHI && !GP) {  // GP trees: k_gp_like sees the status and finishes the pair
            if (tid == 0) L.lle[pair] = -INFINITY;
            finish_walker(L, pair, tid, acc1, sq, sacc1, sflag);
        }
        return;
    }
    double tb = 0.0, dn = 0.0, vs = 0.0;
    if (tid < NBS) {
        sbw[tid] = wB;
        tb = wB;
    } else if (tid >= nt - NDONOR) {
        // donor normalisation at quadrature (theta = pi/2): e = (0, -s, c)
        const int mr = (tid - (nt - NDONOR)) & 3;
        const double vy = (mr & 1) ? -dq[1] : dq[1], vz = (mr & 2) ? -dq[2] : dq[2];
        dn = fmax(-s * vy + c * vz, 0.0);
        vs = fabs(dq[0]) + fabs(dq[1]) + fabs(dq[2]);
    }
    if (tid >= NBS && tid < NBS + NWD_RINGS + NDISC_R) swr[tid - NBS] = wring;
    {
        if (tid >= NBS + NWD_RINGS + NDISC_R && tid < NBS + NWD_RINGS + NDISC_R + G_COUNT)
            sgeo[tid - (NBS + NWD_RINGS + NDISC_R)] = gv;
        if (tid < NBS) sab[tid] = abB;
        else if (tid >= nt - NDONOR && ((tid - (nt - NDONOR)) & 3) == 0)
            for (int i = 0; i < DON_STRIDE; ++i) sdq[((tid - (nt - NDONOR)) >> 2) * DON_STRIDE + i] = dq[i];
    }
    // hulls of the eclipsed WD/disc and spot intervals (tiles outside skip
    // them): only when there is more than one tile or sub-bin tables
    const bool hull = SUB || n > LIKE_TILE;
    if (hull) {
        double wa = INFINITY, wb = -INFINITY, sa = INFINITY, sb = -INFINITY;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (abk[i].x < abk[i].y) { wa = fmin(wa, abk[i].x); wb = fmax(wb, abk[i].y); }
        if (tid < NBS && abB.x < abB.y) { sa = abB.x; sb = abB.y; }
        wa = wave_min(wa); wb = wave_max(wb); sa = wave_min(sa); sb = wave_max(sb);
        if (lane == 0) { shw[0][wv] = wa; shw[1][wv] = wb; shw[2][wv] = sa; shw[3][wv] = sb; }
    }
    tb = wave_sum(tb);
    dn = wave_sum(dn);
    vs = wave_sum(vs);
    if (lane == 0) { red[0][wv] = tb; red[1][wv] = dn; red[2][wv] = vs; }
    LIKE_PRO(1);
    __syncthreads();
    LIKE_PRO(2);
    if (wv == 0) {  // block-uniform normalisers live in LDS (read at use: no registers held)
        // the nw wave partials: lanes 0..nw-1 read them at once and three
        // independent DPP wave sums add them (a serial loop in one lane
        // waited on every LDS read in turn)
        double p0 = 0.0, p1 = 0.0, p2 = 0.0;
        if (lane < nw) { p0 = red[0][lane]; p1 = red[1][lane]; p2 = red[2][lane]; }
        p0 = wave_sum(p0);
        p1 = wave_sum(p1);
        p2 = wave_sum(p2);
        if (lane == 0) {
            snorm[0] = 1.0 / p0;
            snorm[1] = 1.0 / p2;
            snorm[2] = p1;
            snorm[3] = p2;
        }
        if (hull && lane < 4) {
            double h = (lane & 1) ? -INFINITY : INFINITY;
            for (int k = 0; k < nw; ++k) h = (lane & 1) ? fmax(h, shw[lane][k]) : fmin(h, shw[lane][k]);
            shull[lane] = h;
        }
    }
    const double twd = TWO_PI * ((1.0 - ul) * 0.5 + ul / 3.0);  // 2 pi [F(1) - F(0)]
    if (tid >= NBS && tid < NBS + NWD_RINGS + NDISC_R)  // visible to the sweep after the pass barrier
        swn[tid - NBS] = wring * ((tid - NBS < NWD_RINGS) ? 1.0 / twd : 1.0 / td);

    // geometry constants of the tile loop come from sgeo at each use (vector
    // loads of G would hold ~13 doubles in VGPRs through every pass)
    const double* SG = sgeo;
    const int S = L.nsub;
    constexpr bool TAB = SUB;  // sub-bins: the spot and donor from breakpoint tables
    SubEntries& DE = *reinterpret_cast<SubEntries*>(&sacc[2][0]);
    if (TAB) {
        SubTables& T = SU.tb;
        // (a) the range of every sub-bin centre of the pair (the donor cells
        // span it), and the tables zeroed
        double qlo = INFINITY, qhi = -INFINITY;
        for (int p = tid; p < n; p += nt) {
            const double xp = L.x[o0 + p], wp = L.w ? L.w[o0 + p] : 0.0;
            const double a0 = xp - SG[G_PHI0], hp = wp / S;
            for (int j = 0; j < S; ++j) {
                const double ph = wrap_phase(a0 - wp + (2 * j + 1) * hp);
                qlo = fmin(qlo, ph);
                qhi = fmax(qhi, ph);
            }
        }
        for (int g = tid; g < TCELLS; g += nt) {
            T.dpre[g][0] = T.dpre[g][1] = T.dpre[g][2] = 0;
            T.spre[g] = 0;
            T.dend[g] = T.send[g] = 0;
        }
        if (tid < 3) T.dv0[tid] = 0;
        qlo = wave_min(qlo);
        qhi = wave_max(qhi);
        if (lane == 0) { sqr[0][wv] = qlo; sqr[1][wv] = qhi; }
        __syncthreads();
        double t0d = INFINITY, t1d = -INFINITY;
        for (int k = 0; k < nw; ++k) { t0d = fmin(t0d, sqr[0][k]); t1d = fmax(t1d, sqr[1][k]); }
        const double dginv = (t1d > t0d) ? TCELLS / (t1d - t0d) : 0.0;
        const double st0 = shull[2], sginv = (shull[3] > shull[2]) ? TCELLS / (shull[3] - shull[2]) : 0.0;
        if (tid == 0) { T.dt0 = t0d; T.dginv = dginv; T.st0 = st0; T.sginv = sginv; }
        // (b) this lane's breakpoints (<= 2): counts and fixed-point sums per cell
        {
            const double itb = snorm[0], ivs = snorm[1];
            double p0, p1;
            bool in0, in1;
            int v0;
            lane_breakpoints(tid, sdq, sab, t0d, t1d, p0, p1, in0, in1, v0);
            if (tid >= nt - NDONOR) {
                long long q[3];
                donor_q(sdq, tid - (nt - NDONOR), ivs, q[0], q[1], q[2]);
                if (v0)
                    for (int k = 0; k < 3; ++k)
                        atomicAdd(reinterpret_cast<unsigned long long*>(&T.dv0[k]),
                                  static_cast<unsigned long long>(v0 * q[k]));
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    if (!(b ? in1 : in0)) continue;
                    const int g = tcell(b ? p1 : p0, t0d, dginv);
                    atomicAdd(&T.dend[g], 1);
                    for (int k = 0; k < 3; ++k)
                        atomicAdd(reinterpret_cast<unsigned long long*>(&T.dpre[g][k]),
                                  static_cast<unsigned long long>(b ? -q[k] : q[k]));
                }
            } else if (in0) {
                const long long W = to_fx(sbw[tid] * itb);
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int g = tcell(b ? p1 : p0, st0, sginv);
                    atomicAdd(&T.send[g], 1);
                    atomicAdd(reinterpret_cast<unsigned long long*>(&T.spre[g]),
                              static_cast<unsigned long long>(b ? -W : W));
                }
            }
        }
        __syncthreads();
        // (c) exclusive prefixes over the cells: entry offsets, V0 + sums below, covering weights
        long long v[6] = {0, 0, 0, 0, 0, 0};
        if (tid < TCELLS) {
            v[0] = T.dend[tid];
            v[1] = T.send[tid];
            v[2] = T.dpre[tid][0];
            v[3] = T.dpre[tid][1];
            v[4] = T.dpre[tid][2];
            v[5] = T.spre[tid];
        }
        cell_scan<6>(v, spart, tid);
        if (tid < TCELLS) {
            T.dend[tid] = int(v[0]);
            T.send[tid] = int(v[1]);
            T.dpre[tid][0] = v[2] + T.dv0[0];
            T.dpre[tid][1] = v[3] + T.dv0[1];
            T.dpre[tid][2] = v[4] + T.dv0[2];
            T.spre[tid] = v[5];
        }
        __syncthreads();
        // (d) the entries into cell order; afterwards dend / send hold each cell's end
        {
            double p0, p1;
            bool in0, in1;
            int v0;
            lane_breakpoints(tid, sdq, sab, t0d, t1d, p0, p1, in0, in1, v0);
            const int base = (tid >= nt - NDONOR) ? 2 * (tid - (nt - NDONOR)) : 2 * tid;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                if (!(b ? in1 : in0)) continue;
                const double pos = b ? p1 : p0;
                if (tid >= nt - NDONOR) {
                    const int slot = atomicAdd(&T.dend[tcell(pos, t0d, dginv)], 1);
                    DE.dpos[slot] = pos;
                    DE.dcode[slot] = base + b;
                } else {
                    const int slot = atomicAdd(&T.send[tcell(pos, st0, sginv)], 1);
                    T.spos[slot] = pos;
                    T.scode[slot] = base + b;
                }
            }
        }
        __syncthreads();
        // (e) each cell's donor entries in order (sub_point's cursor): position,
        // an end before a start at equal positions; a few entries per cell.
        // The spot's entries by position too
        if (tid < TCELLS) {
            const int i0 = tid ? T.dend[tid - 1] : 0, i1 = T.dend[tid];
            for (int i = i0 + 1; i < i1; ++i) {
                const double p = DE.dpos[i];
                const int c = DE.dcode[i];
                int k = i;
                for (; k > i0; --k) {
                    const double pk = DE.dpos[k - 1];
                    const int ck = DE.dcode[k - 1];
                    if (!(pk > p || (pk == p && (c & 1) && !(ck & 1)))) break;
                    DE.dpos[k] = pk;
                    DE.dcode[k] = ck;
                }
                DE.dpos[k] = p;
                DE.dcode[k] = c;
            }
            // the spot's entries of the cell by position (sub_point's spot cursor)
            const int j0 = tid ? T.send[tid - 1] : 0, j1 = T.send[tid];
            for (int i = j0 + 1; i < j1; ++i) {
                const double p = T.spos[i];
                const int c = T.scode[i];
                int k = i;
                for (; k > j0 && T.spos[k - 1] > p; --k) {
                    T.spos[k] = T.spos[k - 1];
                    T.scode[k] = T.scode[k - 1];
                }
                T.spos[k] = p;
                T.scode[k] = c;
            }
        }
        __syncthreads();
    }
    for (int t0 = 0; t0 < n; t0 += LIKE_TILE) {
        double chi = 0.0;  // this tile's chi^2 (summed per wave into red[1] at the tile's end)
        const int m = min(LIKE_TILE, n - t0);
        LIKE_STAMP(0);
        const bool own = tid < m;
        if ((t0 > 0 || SUB) && own) {
            // the point index re-formed from a fresh (volatile) read of the
            // offset: o0 + tid would otherwise be held, spilled, over the tiles
            const int p = (offs ? *reinterpret_cast<const volatile int*>(L.off + e) : 0) + t0 + tid;
            px = L.x[p];
            pw = L.w ? L.w[p] : 0.0;
            if (CHI && t0 > 0) {
                sy[tid] = L.y[p];
                if (!GP) sye[tid] = L.ye[p];
            }
        }
        // MODEL_SPEC 3: a negative width is a zero one (point evaluation at the
        // centre for every S); NaN stays NaN
        const double wk = own ? (pw < 0.0 ? 0.0 : pw) : 0.0;
        const double ph0 = own ? px - SG[G_PHI0] : 0.0;
        const double phc = wrap_phase(ph0);
        double fw = 0.0, fd = 0.0, sbs = 0.0, srs = 0.0;
        // the pass over the points' own windows: the WD and disc (and, S = 1,
        // the spot on the same windows and the donor at the point phases)
        if (tid == 0) { sflag[0] = 0; sflag[1] = 0; }
        int flA = put_window(TA, tid, own, phc, wk);
        if (!TAB && own) sph[tid] = phc;
        for (int i = 0; i < (TAB ? 2 : 6); ++i) sacc[i][tid] = 0ull;
        if (!TAB) {
            SU.s1.X[0][tid] = 0ull;
            SU.s1.X[1][tid] = 0ull;
        }
        if (tid == 0)
            for (int i = 0; i < (TAB ? 2 : 6); ++i) sacc[i][nt] = 0ull;
        // does this point's window reach the WD/disc hull?  (any does: the tile
        // sweeps; one tile and no sub-bins: always)
        if (hull && own && wk >= 0.0 && !(phc + wk < shull[0] || phc - wk > shull[1])) flA |= 8;
        __syncthreads();
        flA |= check_sorted(TA, tid, own);
        // the flags OR-ed over the wave first: one LDS atomic per wave
        // (a same-address atomic per point serialised the hull bit)
        const int wfA = wave_or4(flA);
        if (lane == 0 && wfA) atomicOr(&sflag[0], wfA);
        build_cells(TA.lo, m, TA.cell, tid);
        if (!TAB) {
            const int flB = (flA & 7) | ((own && tid && sph[tid] < sph[tid - 1]) ? 4 : 0);
            const int wfB = wave_or4(flB);
            if (lane == 0 && wfB) atomicOr(&sflag[1], wfB);
            build_cells(sph, m, scp, tid);
        }
        __syncthreads();
        // any unsorted / mixed window (or invalid width) of the tile: the
        // pass goes point-major (every element against each point)
        const bool dir = (sflag[0] & 7) != 0 || (!TAB && sflag[1] != 0);
#ifdef LFG_ABL_WDD  // diagnostic ablation: no WD/disc sweep
        const bool wdd = false;
#else
        const bool wdd = !hull || (sflag[0] & 8) != 0;  // the WD/disc elements touch the tile
#endif
        LIKE_STAMP(1);
        double eb = 0.0, R3 = 0.0, R4 = 0.0, R5 = 0.0;
        if (dir) {
            if (own) {
                const double ulg = SG[G_ULIMB];
                const double2 f2 = direct_wd_disc(AB, swr, phc, wk, TWO_PI * ((1.0 - ulg) * 0.5 + ulg / 3.0), Wt[WT_TD]);
                fw = f2.x;
                fd = f2.y;
                if (!TAB) eb = direct_spot(sab, sbw, phc, wk, snorm[0]);
            }
            __syncthreads();  // every wave has read sflag before the next tile resets it
        } else {
            if (wdd) {
                if constexpr (TAB) {
                    // re-read per tile (L2): held over the tiles they would not
                    // leave the sub-bin queries their registers.  The pointer is
                    // laundered through an empty asm so that the compiler cannot
                    // reuse the prologue's loads of the same (restrict) table:
                    // it kept those values live through the table build, 48 B
                    // of scratch per lane
                    const double2* ABt = AB;
                    asm volatile("" : "+s"(ABt));
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        const int g = tid + i * nt;
                        abk[i] = (g < NWD + NDISC) ? sweep_ab(ABt, g) : make_double2(1.0, -1.0);
                    }
                }
                const PhaseIndex X = phase_index(TA.lo, TA.cell, m);
                double qx[2 * NI];
                int J[2 * NI], Jb[2 * NI];
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    qx[2 * i] = abk[i].x;
                    qx[2 * i + 1] = abk[i].y;
                }
                count_lt_multi<2 * NI>(X, qx, J);
                count_le_back_multi<2 * NI>(TA.hi, qx, J, Jb);
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    if (abk[i].x < abk[i].y) {
                        const int g = tid + i * nt;
                        const int u = uitem(g < NU_WDD ? g : g - NU_WDD);
                        apply_runs(Runs{Jb[2 * i], J[2 * i], Jb[2 * i + 1], J[2 * i + 1]}, abk[i].x, abk[i].y,
                                   swn[uring(u)], X, TA.hi, TA.iw,
                                   ((!TAB && (lane & 1)) ? SU.s1.X : sacc)[(u < U_WD) ? 0 : 1]);
                    }
            }
            LIKE_STAMP(2);
            if (!TAB)
                sweep_spot_donor(tid, phase_index(TA.lo, TA.cell, m), TA, phase_index(sph, scp, m), sab, sbw,
                                 snorm[0], sdq, snorm[1], sacc + 2);
            __syncthreads();
            LIKE_STAMP(3);
            long long r[6] = {0, 0, 0, 0, 0, 0};
            if (!TAB) block_scan<6>(sacc, spart, tid, r, SU.s1.X);
            else if (wdd) block_scan<2>(sacc, spart, tid, r);
            LIKE_STAMP(4);
            fw = double(r[0]) * FX_INV;
            fd = double(r[1]) * FX_INV;
            eb = double(r[2]) * FX_INV;
            R3 = double(r[3]);
            R4 = double(r[4]);
            R5 = double(r[5]);
        }
        const double sg = SG[G_S], cg = SG[G_C];
        const double bden = SG[G_BDEN], fis = SG[G_FIS];
        if (!TAB) {
            const double2 scp2 = sincospi_ool(2.0 * phc);  // |2 ph| <= 1: cheap exact reduction
            const double e0 = sg * scp2.y, e1 = -sg * scp2.x;
            double D = 0.0;
            if (!dir) D = (e0 * R3 + e1 * R4 + cg * R5) * (FX_INV * snorm[3]);
            else if (own) D = direct_donor(sdq, e0, e1, cg);
            double beam = 0.0;
            if (bden > 0.0)
                beam = (fis + (1.0 - fis) * fmax(SG[G_NB0] * e0 + SG[G_NB1] * e1 + SG[G_NB2] * cg, 0.0)) / bden;
            sbs = beam * (1.0 - eb);
            srs = D / snorm[2];
        } else if (own) {
#ifdef LFG_ABL_SUBPOINT  // diagnostic ablation: no sub-bin spot / donor terms
            const double2 r2 = make_double2(ph0 * 1e-30, wk * 1e-30);
#else
            const double2 r2 = sub_point(SU.tb, DE, sab, sbw, sdq, snorm, shull, SG, ph0, wk, S);
#endif
            sbs = r2.x;
            srs = r2.y;
        }
        // no barrier before the next tile rewrites the tile buffers: every
        // read of TA / sph / scp / sacc / sflag of this tile precedes the
        // block scan's barriers or the direct path's barrier (after them only
        // registers, part[], the tables and the pass-invariant LDS are read,
        // none of which the next tile's prologue writes); a table tile that
        // skipped the scan waits here instead
        if (TAB && !dir && !wdd) __syncthreads();
        if (own) {
            const double nw0 = isnan(wk) ? NAN : 1.0;  // MODEL_SPEC 3: a NaN width gives a NaN flux
            const double fwv = nw0 * SG[G_WDF] * (1.0 - fw), fdv = nw0 * SG[G_DF] * (1.0 - fd);
            const double fb = nw0 * SG[G_SF] * sbs / S, fr = nw0 * SG[G_RSF] * srs / S;
            const double f = fwv + fdv + fb + fr;
            const int pi = t0 + tid;
            if (!CHI && L.flux) L.flux[size_t(pair) * n + pi] = f;
            if (!CHI && L.comps) {
                L.comps[(size_t(0) * L.npairs + pair) * n + pi] = fwv;
                L.comps[(size_t(1) * L.npairs + pair) * n + pi] = fdv;
                L.comps[(size_t(2) * L.npairs + pair) * n + pi] = fb;
                L.comps[(size_t(3) * L.npairs + pair) * n + pi] = fr;
            }
            if (CHI && !GP) {
                const double r = (sy[tid] - f) / sye[tid];
                chi += isnan(f) ? INFINITY : r * r;
            }
            if (GP) L.res[size_t(pair) * L.N + pi] = sy[tid] - f;  // the filter runs in k_gp_like
        }
        if (CHI && !GP) {  // red[1] is free after the prologue; each wave owns its slot
            chi = wave_sum(chi);
            if (lane == 0) red[1][wv] = (t0 == 0) ? chi : red[1][wv] + chi;
        }
        LIKE_STAMP(5);
    }
    if (CHI && !GP) {
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
            // an eclipse without points ran no tile: red[1] still holds the
            // prologue's partial sums, and chi^2 is the empty sum
            if (n > 0)
                for (int i = 0; i < nw; ++i) tot += red[1][i];
            L.lle[pair] = -0.5 * tot;
        }
        finish_walker(L, pair, tid, acc1, sq, sacc1, sflag);
    }
}

#include "lfg_k_pair.hpp"  // the section of k_pair (its LONG tables: lfg_k_pair_long.hpp)

// the kernels k_pair needs nothing of, and the host's run_front: one header per section
#ifndef LFG_NOLICM_TU  // (lfg_pair_split.hip compiles k_pair only)
#include "lfg_k_gp.hpp"
#include "lfg_k_stretch.hpp"
#include "lfg_k_misc.hpp"
#endif

}  // namespace

// k_pair's fold and LONG instantiations are compiled in lfg_pair_split.hip:
// this source again, without machine LICM (-mllvm -disable-machine-licm).
// At the 128-VGPR ceiling the pass hoisted literal constants and cheap loop
// invariants into VGPRs and the register allocator then spilled: LONG's
// point loop reloaded five doubles from scratch per point (48 B per lane,
// 41.6 MB of PMC traffic per config-5 launch), the fold variant 32 B.
// Without it LONG spills 16 B and the fold variant none: config 5
// 3.39 -> 3.52 M evals/s; config 4's one-of-eight fold shard 12.71 -> 12.76
// and 12.36 -> 12.77 M on two boxes (profiles/r06/ab_split_nolicm.txt).  The
// speculative one-tile k_pair (config 2) measured no different and GP trees
// 5 % slower, so they stay here, compiled with the pass.
enum { PAIR_SPLIT_LONG = 0, PAIR_SPLIT_FOLD = 1, PAIR_SPLIT_FOLD_LONG = 2 };
__attribute__((visibility("hidden"))) void lfg_pair_launch_split(int variant, unsigned grid, hipStream_t st,
                                                                   const void* args);

#ifndef LFG_NOLICM_TU
namespace {
// launch k_pair<false, FOLD, LONG> (not both false) with the arguments A
void launch_pair_split(int variant, unsigned grid, hipStream_t st, const PairArgs& A)
{
#ifdef LFG_ONE_TU
    if (variant == PAIR_SPLIT_LONG) hipLaunchKernelGGL((k_pair<false, false, true>), dim3(grid), dim3(LIKE_THREADS), 0, st, A);
    else if (variant == PAIR_SPLIT_FOLD) hipLaunchKernelGGL((k_pair<false, true>), dim3(grid), dim3(LIKE_THREADS), 0, st, A);
    else hipLaunchKernelGGL((k_pair<false, true, true>), dim3(grid), dim3(LIKE_THREADS), 0, st, A);
#else
    lfg_pair_launch_split(variant, grid, st, &A);
#endif
}
}  // namespace

extern "C" {

size_t lfg_workspace_size(int W, int E)
{
    if (W <= 0 || E <= 0) return 0;
    return carve(nullptr, W, E).total;
}

size_t lfg_workspace_size_tree(int W, const lfg_tree* T)
{
    if (W <= 0 || !T || T->E <= 0) return 0;
    return carve(nullptr, W, T->E, T->gp ? T->max_n : 0, T->ndim).total;  // + lfg_stretch_step_half_spec's
}

// k_setup's arguments for a flat batch: W vectors of P eclipse parameters,
// one eclipse each, no tree (lfg_flux, lfg_lnlike, lfg_elements)
static SetupArgs setup_args_flat(const double* pars, int W, int P, const Ws& ws)
{
    SetupArgs S{};
    S.walkers = pars;
    S.W = W;
    S.ndim = P;
    S.E = 1;
    S.P = P;
    S.geo = ws.geo;
    S.status = ws.status;
    S.prior = ws.prior;
    S.bstatus = ws.bstatus;
    return S;
}

// the likelihood kernels' arguments for such a batch: every pair on the
// points x[0..N) of widths w; the caller adds its outputs (flux and comps,
// or y, ye and lle)
static LikeArgs like_args_flat(const Ws& ws, int W, const double* x, const double* w, int N, int nsub)
{
    LikeArgs L{};
    L.geo = ws.geo;
    L.status = ws.status;
    L.AB = ws.ab;
    L.DON = ws.donor;
    L.WT = ws.wts;
    L.E = 1;
    L.N = N;
    L.x = x;
    L.w = w;
    L.nsub = nsub;
    L.npairs = W;
    L.bstatus = ws.bstatus;
    return L;
}

int lfg_flux(const double* pars, int W, int P, const double* x, const double* w, int N, int nsub,
             double* flux, double* comps, int* status, void* wsp, size_t ws_bytes, void* stream)
{
    if (W <= 0 || N < 0 || nsub < 1 || (P != 14 && P != 18) || !pars || (!x && N > 0)) return LFG_E_ARGS;
    Ws ws = carve(wsp, W, 1);
    if (!wsp || ws_bytes < ws.total) return LFG_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SetupArgs S = setup_args_flat(pars, W, P, ws);
    int rc = run_front(S, ws, st, nullptr);
    if (rc) return rc;
    if (N > 0) {
        LikeArgs L = like_args_flat(ws, W, x, w, N, nsub);
        L.flux = flux;
        L.comps = comps;
        if (nsub > 1) hipLaunchKernelGGL((k_lnlike<0, true>), dim3(W), dim3(LIKE_THREADS), 0, st, L);
        else hipLaunchKernelGGL((k_lnlike<0, false>), dim3(W), dim3(LIKE_THREADS), 0, st, L);
        if ((rc = launch_ok())) return rc;
    }
    if (status && hipMemcpyAsync(status, ws.status, sizeof(int) * W, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return LFG_E_LAUNCH;
    return LFG_OK;
}

// k_pair serves trees whose eclipses fit one tile with S = 1 (GP trees
// included); k_elements + k_lnlike serve the rest, and every tree when
// LFG_PAIR=0 is in the environment (the A/B switch of the two layouts)
// k_pair's workgroups all resident at once: two per CU (72.9 KB of LDS each)
// PairArgs.prio: the workgroups that take the wave-priority scheme
// (PAIR_PRIO).  Launches of at most two rounds (two workgroups per CU
// resident): all of them -- the one-round launches of config 2 and of the
// weak-scaling shards, and the two-round 1 024-pair shard of config 4 over 8
// ranks, whose projected 1 -> 8 speed-up rose 5.7x -> 6.1x with it (A/B,
// rounds 1 and 2 both prioritised vs none: 173 vs 183 us per step).  Longer
// launches none: there an early finish lets the next round's workgroup in
// (the GP example's 6 rounds: 1.92 vs 1.95 M evals/s with the scheme on)
static int pair_prio(int npairs)
{
    int dev = 0, cus = 0;  // the current device's (the runtime caches the attribute)
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus = 0;
    return npairs <= 4 * cus ? npairs : 0;
}

// the trees k_pair can serve: one-tile eclipses, S = 1 (kind 1); and, with
// the LONG tables, chi^2 trees of any eclipse length and sub-binning (kind 2)
static bool pair_fits(int nsub, int max_n, int ndim) { return nsub == 1 && max_n <= LIKE_TILE && ndim <= LIKE_THREADS; }
static int pair_eligible(int gp, int nsub, int max_n, int ndim)
{
    if (pair_fits(nsub, max_n, ndim)) return 1;
    return (!gp && nsub >= 1 && ndim <= LIKE_THREADS) ? 2 : 0;
}

// k_pair's arguments but for the proposal and fold fields (pair_args_move):
// nbc blocks per candidate carry the speculative lanes, a whole wave each
static PairArgs pair_args(const LikeArgs& L, const ElemSpec& X, int nbc, int npairs)
{
    PairArgs A{};
    A.L = L;
    A.X = X;
    A.spl = 64;
    A.nbc = nbc;
    A.prio = pair_prio(npairs);
    return A;
}

static bool pair_env()
{
    const char* e = getenv("LFG_PAIR");
    return !(e && e[0] == '0');
}
static std::atomic<int> g_pair_layout{-2};  // -2: not read yet; 0 / 1: lfg_set_layout or the environment

// the kernels a tree runs on: 0 k_elements + k_lnlike, 1 k_pair, 2 k_pair LONG
static int pair_kind(int gp, int nsub, int max_n, int ndim)
{
    int m = g_pair_layout.load(std::memory_order_relaxed);
    if (m == -2) {
        m = pair_env() ? 1 : 0;
        g_pair_layout.store(m, std::memory_order_relaxed);
    }
    return m == 1 ? pair_eligible(gp, nsub, max_n, ndim) : 0;
}

int lfg_set_layout(int mode)
{
    if (mode < -1 || mode > 1) return LFG_E_ARGS;
    int prev = g_pair_layout.load();
    if (prev == -2) prev = pair_env() ? 1 : 0;
    g_pair_layout.store(mode == -1 ? (pair_env() ? 1 : 0) : mode);
    return prev;
}

int lfg_layout(const lfg_tree* T)
{
    if (!T || T->E <= 0) return LFG_E_ARGS;
    return pair_kind(T->gp, T->nsub, T->max_n, T->ndim);
}

int lfg_lnlike(const double* pars, int W, int P, const double* x, const double* w, int N, int nsub, const double* y,
               const double* ye, double* lnlike, int* status, void* wsp, size_t ws_bytes, void* stream)
{
    if (W <= 0 || N < 0 || nsub < 1 || (P != 14 && P != 18) || !pars || !lnlike || (N > 0 && (!x || !y || !ye)))
        return LFG_E_ARGS;
    Ws ws = carve(wsp, W, 1);
    if (!wsp || ws_bytes < ws.total) return LFG_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SetupArgs S = setup_args_flat(pars, W, P, ws);
    const int kind = pair_kind(0, nsub, N, 0);
    const bool pair = kind > 0;
    int rc = run_front(S, ws, st, nullptr, !pair);
    if (rc) return rc;
    LikeArgs L = like_args_flat(ws, W, x, w, N, nsub);
    L.y = y;
    L.ye = ye;
    L.lle = lnlike;
    PairArgs A = pair_args(L, ElemSpec{}, 0, W);
    fill_hot(A);
    if (kind == 2) launch_pair_split(PAIR_SPLIT_LONG, unsigned(W), st, A);
    else if (pair) hipLaunchKernelGGL(k_pair<false>, dim3(W), dim3(LIKE_THREADS), 0, st, A);
    else if (nsub > 1) hipLaunchKernelGGL((k_lnlike<1, true>), dim3(W), dim3(LIKE_THREADS), 0, st, L);
    else hipLaunchKernelGGL((k_lnlike<1, false>), dim3(W), dim3(LIKE_THREADS), 0, st, L);
    if ((rc = launch_ok())) return rc;
    if (status && hipMemcpyAsync(status, ws.status, sizeof(int) * W, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return LFG_E_LAUNCH;
    return LFG_OK;
}

struct Accept {  // fused stretch-move acceptance of lfg_stretch_lnprob_accept
    double* pos;
    double* lnp;
    const double* zfac;
    int half;
    unsigned long long seed, step;
    int* naccept;
};

struct Propose {  // inline proposal of lfg_stretch_step_half / _shard
    const double* pos;
    double a;
    double* q;
    double* zfac;
    int half;
    unsigned long long seed, step;
    int lo, ns;  // the batch: walkers lo .. lo + W - 1 of the ns-walker half
};

struct SpecCtl {  // lfg_stretch_step_half_spec
    bool in;   // this half's setup candidates are in the workspace (skip k_setup)
    bool out;  // form the next half's candidates inside this k_elements
};

struct FoldCtl {  // lfg_stretch_step_shard_fold: deferred acceptance
    const double* fv;  // [ns] the partner half's pending verdicts (nullptr: none)
    double* vout;      // [n] this shard's verdicts
    double* pos;       // the ensemble the verdicts apply to
    double* lnp;
    int* naccept;
};

static int apply_verdicts(double* pos, double* lnp, int W, int ndim, int half, double a, const double* verdict,
                          unsigned long long seed, unsigned long long step, int* naccept, int* accflag,
                          hipStream_t st)
{
    const int ns = W / 2;
    hipLaunchKernelGGL(k_apply_verdicts, dim3((ns + REGEN_WAVES - 1) / REGEN_WAVES), dim3(64 * REGEN_WAVES), 0, st,
                       pos, lnp, W, ndim, half, a, verdict, seed, step, naccept, accflag);
    return launch_ok();
}

// k_setup's arguments for W walkers of a tree; gp: with the tree's GP
// hyper-parameter gather (lfg_lnprior leaves it out); prop (nullable): the
// walkers are formed inline as the stretch-move proposals of prop
static SetupArgs setup_args_tree(const double* walkers, int W, const lfg_tree* T, const Ws& ws, bool gp,
                                 const Propose* prop)
{
    SetupArgs S{};
    S.walkers = walkers;
    S.W = W;
    S.ndim = T->ndim;
    S.E = T->E;
    S.P = 18;
    S.gather = T->gather;
    S.npars = T->npars;
    S.consts = T->consts;
    S.prior_type = T->prior_type;
    S.prior_p1 = T->prior_p1;
    S.prior_p2 = T->prior_p2;
    S.prior_norm = T->prior_norm;
    S.roche_priors = T->roche_priors;
    S.geo = ws.geo;
    S.status = ws.status;
    S.prior = ws.prior;
    S.bstatus = ws.bstatus;
    if (gp) {
        S.gp = T->gp;
        S.gp_gather = T->gp_gather;
        S.gp_base = T->gp_base;
    }
    S.fixed_invalid = T->fixed_invalid;
    S.prior_c = T->prior_c;
    if (prop) {
        S.pos = prop->pos;
        S.a = prop->a;
        S.seed = prop->seed;
        S.step = prop->step;
        S.half = prop->half;
        S.qout = prop->q;
        S.zfout = prop->zfac;
        S.lo = prop->lo;
        S.ns = prop->ns;
    }
    return S;
}

// the likelihood kernels' arguments for W walkers of a tree: ln_like per
// pair into lle, ln_prob into lnp (nullable), the fused acceptance of acc
// (nullable) with the walkers as its proposals
static LikeArgs like_args_tree(const Ws& ws, int W, const lfg_tree* T, double* lle, double* lnp, const double* walkers,
                               const Accept* acc)
{
    LikeArgs L{};
    L.geo = ws.geo;
    L.status = ws.status;
    L.AB = ws.ab;
    L.DON = ws.donor;
    L.WT = ws.wts;
    L.E = T->E;
    L.off = T->off;
    L.N = T->max_n;
    L.x = T->x;
    L.y = T->y;
    L.ye = T->ye;
    L.w = T->w;
    L.nsub = T->nsub;
    L.lle = lle;
    L.npairs = W * T->E;
    L.prior = ws.prior;
    L.lnp = lnp;
    L.combine = T->E == 1;  // E > 1: k_combine_walkers after the likelihood kernels
    L.qprop = walkers;
    L.ndim = T->ndim;
    if (acc) {
        L.pos = acc->pos;
        L.lnp_ens = acc->lnp;
        L.zfac = acc->zfac;
        L.half = acc->half;
        L.seed = acc->seed;
        L.step = acc->step;
        L.naccept = acc->naccept;
    }
    if (T->gp) {  // the residuals and transitions k_gp_like filters
        L.gp_ecl = T->gp_ecl;
        L.res = ws.res;
        L.gpx = ws.gpx;
        L.gpb = ws.gpb;
    }
    L.bstatus = ws.bstatus;
    return L;
}

// the workspace's snapshot of the rows of one half of the ensemble
static double* snap_rows(const Ws& ws, int which_half, int ndim)
{
    return ws.snap + size_t(which_half) * ws.accstride * ndim;
}

// take it: copy the ns rows of that half of pos ([2 ns][ndim]) on the stream
static bool snapshot_half(const Ws& ws, const double* pos, int which_half, int ns, int ndim, hipStream_t st)
{
    const size_t rows = size_t(ns) * ndim;
    return hipMemcpyAsync(snap_rows(ws, which_half, ndim), pos + size_t(which_half) * rows, rows * sizeof(double),
                          hipMemcpyDeviceToDevice, st) == hipSuccess;
}

// k_elements' / k_pair's side jobs of the speculative setup (sp nullable:
// none): sp->in selects this half's candidates from the workspace, sp->out
// forms the next half's from copies of S; fold_fv (nullable): the pending
// verdicts a fold k_pair launch applies, which the next half's rows follow
static ElemSpec spec_args(const Ws& ws, const SetupArgs& S, int W, const lfg_tree* T, const Propose* prop,
                          const SpecCtl* sp, const double* fold_fv)
{
    const int npairs = W * T->E;
    ElemSpec X{};
    X.E = T->E;
    X.ndim = T->ndim;
    X.lprior = ws.prior;
    if (!sp) return X;
    const int h = prop->half, hn = 1 - prop->half;
    const size_t P48 = size_t(npairs) * LFG_NGEO;
    if (sp->in) {
        X.jk = ws.jk + size_t(h) * W;
        X.accflag = ws.accflag + size_t(hn) * ws.accstride;  // the partner half's acceptances
        X.geoC = ws.geoC + 2 * h * P48;
        X.statusC = ws.statusC + 2 * h * size_t(npairs);
        X.bstatusC = ws.bstatusC + 2 * h * size_t(npairs);
        X.priorC = ws.priorC + 2 * h * size_t(W);
        X.qC = ws.qC + 2 * h * size_t(W) * T->ndim;
        X.zfC = ws.zfC + 2 * h * size_t(W);
        X.prior = ws.prior;
        X.q = prop->q;
        X.zf = prop->zfac;
        X.bstatus = ws.bstatus;
    }
    if (sp->out) {
        for (int c = 0; c < 2; ++c) {
            SetupArgs& N = X.S[c];
            N = S;
            const size_t k = size_t(2 * hn + c);
            N.half = hn;
            N.step = hn == 0 ? prop->step + 1 : prop->step;
            N.step_prev = prop->step;
            N.cand = c;
            N.geo = ws.geoC + k * P48;
            N.status = ws.statusC + k * npairs;
            N.bstatus = ws.bstatusC + k * npairs;
            N.prior = ws.priorC + k * W;
            N.qout = ws.qC + k * size_t(W) * T->ndim;
            N.zfout = ws.zfC + k * W;
            N.jkout = ws.jk + size_t(hn) * W;
            if (fold_fv) {  // the next half's rows as the pending verdicts leave them
                N.fv = fold_fv;
                N.fsnap = snap_rows(ws, hn, T->ndim);
                N.fstep = N.step - 1;
            }
        }
        X.nspec = 2 * npairs + W;
        X.nspecblk = (2 * ((X.nspec + ELEM_BLOCK - 1) / ELEM_BLOCK) + 7) / 8 * 8;  // keeps the pair -> XCD map
    }
    return X;
}

// PairArgs' proposal fields (prop nullable: the partner draw of the candidate
// choice) and fold fields (fold nullable: the deferred acceptance inside
// k_pair, applying the pending verdicts fv of step fstep)
static void pair_args_move(PairArgs& A, const Ws& ws, int ndim, const Propose* prop, const FoldCtl* fold,
                           const double* fv, unsigned long long fstep)
{
    if (prop) {
        A.jseed = prop->seed;
        A.jstep = prop->step;
        A.jhalf = prop->half;
        A.jlo = prop->lo;
        A.jns = prop->ns;
    }
    if (fold) {
        A.fv = fv;
        A.vout = fold->vout;
        A.fpos = fold->pos;
        A.flnp = fold->lnp;
        A.fnacc = fold->naccept;
        A.fsnap = snap_rows(ws, prop->half, ndim);
        A.fstep = fstep;
        A.fa = prop->a;
        A.L.seed = prop->seed;
        A.L.step = prop->step;
        A.L.half = prop->half;
        A.L.zfac = prop->zfac;
    }
}

// what follows the likelihood kernel(s) of either layout: the GP filter of a
// GP tree, ln_prob of walkers of E > 1 eclipses, the shard's verdicts from
// its ln_prob (fold nullable: not folding, or k_pair formed them), event 3.
// prop is read only with fold, which needs one (lnprob_impl's validation)
static int launch_tail(const LikeArgs& L, int W, const lfg_tree* T, double* lnp, const Propose* prop,
                       const FoldCtl* fold, hipStream_t st, void* const* ev)
{
    int rc;
    if (T->gp) {
        hipLaunchKernelGGL(k_gp_like, dim3(T->E * ((W + GP_PAIRS - 1) / GP_PAIRS)), dim3(GP_BLOCK), 0, st, L);
        if ((rc = launch_ok())) return rc;
    }
    if (T->E > 1) {
        hipLaunchKernelGGL(k_combine_walkers, dim3((W + 3) / 4), dim3(256), 0, st, L);
        if ((rc = launch_ok())) return rc;
    }
    if (fold) {
        hipLaunchKernelGGL(k_verdict, dim3((W + 63) / 64), dim3(64), 0, st, lnp, fold->lnp, prop->zfac, W, prop->lo,
                           prop->ns, prop->half, prop->seed, prop->step, fold->vout);
        if (launch_ok()) return LFG_E_LAUNCH;
    }
    mark_event(ev, 3, st);
    return LFG_OK;
}

static int lnprob_impl(const double* walkers, int W, const lfg_tree* T, double* lnp, double* lnlike_e, void* wsp,
                       size_t ws_bytes, void* stream, void* const* ev, const Accept* acc = nullptr,
                       const Propose* prop = nullptr, const SpecCtl* sp = nullptr, const FoldCtl* fold = nullptr)
{
    if (W <= 0 || !T || T->E <= 0 || T->ndim <= 0 || T->nsub < 1 || !walkers || (!lnp && !acc)) return LFG_E_ARGS;
    if (sp && (!prop || (acc && (prop->lo != 0 || prop->ns != W)))) return LFG_E_ARGS;
    if (fold && (!sp || !prop || acc || !lnp || !fold->vout || !fold->pos || !fold->lnp || (sp->in && !fold->fv)))
        return LFG_E_ARGS;
    Ws ws = carve(wsp, W, T->E, T->gp ? T->max_n : 0, sp ? T->ndim : 0, prop ? prop->ns : 0);
    if (!wsp || ws_bytes < ws.total) return LFG_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the deferred acceptance runs inside k_pair for one-eclipse chi^2 trees
    // on the k_pair layout; otherwise (and when no candidates are in the
    // workspace: k_setup reads the rows directly) the pending verdicts are
    // applied first, recording the acceptances for the candidate choice, and
    // the shard's verdicts are formed after its ln_prob (k_verdict)
    const double* fv = fold ? fold->fv : nullptr;
    const int kind = pair_kind(T->gp, T->nsub, T->max_n, T->ndim);
    const bool fold_pair = fold && T->E == 1 && !T->gp && kind > 0 &&
                           (!sp->out || 2 * ((2 * W + W + 63) / 64) <= W);
    const unsigned long long fstep = prop && prop->half == 0 ? prop->step - 1 : (prop ? prop->step : 0);
    if (fv && (!fold_pair || !sp->in)) {
        const int rc = apply_verdicts(fold->pos, fold->lnp, 2 * prop->ns, T->ndim, 1 - prop->half, prop->a, fv,
                                      prop->seed, fstep, fold->naccept,
                                      ws.accflag + size_t(1 - prop->half) * ws.accstride, st);
        if (rc) return rc;
        fv = nullptr;
    }
    const SetupArgs S = setup_args_tree(walkers, W, T, ws, true, prop);
    const ElemSpec X = spec_args(ws, S, W, T, prop, sp, fold_pair ? fv : nullptr);
    // k_pair: the element solve and the likelihood of a pair in one
    // workgroup (one-tile eclipses, S = 1; GP trees through k_pair<true> and
    // k_gp_like).  The speculative lanes fill whole waves: wave 0 of blocks
    // [0, 2 nbc), nbc blocks per candidate, so there must be 2 nbc pairs
    const int npairs = W * T->E, nbc = (X.nspec + 63) / 64;
    const bool pair_path = kind > 0 && (X.nspec == 0 || 2 * nbc <= npairs);
    if (fold_pair && !pair_path) return LFG_E_ARGS;  // (fold_pair's test is pair_path's)
    int rc = run_front(S, ws, st, ev, !pair_path, &X, !(sp && sp->in));
    if (rc) return rc;
    LikeArgs L = like_args_tree(ws, W, T, lnlike_e ? lnlike_e : ws.lle, lnp, walkers, acc);
    // sharded: k_accept_regen records them
    L.accflag = (sp && acc) ? ws.accflag + size_t(prop->half) * ws.accstride : nullptr;
    // the speculative lanes of a k_pair launch read partner rows from the
    // workspace's snapshots; on the two-kernel layout a k_pair-eligible tree
    // leaves the snapshot a k_pair launch would have left, so that a layout
    // switch (lfg_set_layout) before the chain's next half reads valid rows
    const bool snaps = sp && sp->out && T->E == 1 && (pair_path || pair_eligible(T->gp, T->nsub, T->max_n, T->ndim));
    if (pair_path) {
        PairArgs A = pair_args(L, X, nbc, npairs);
        pair_args_move(A, ws, T->ndim, prop, fold_pair ? fold : nullptr, fv, fstep);
        if (snaps && acc) {
            // this launch accepts moves of half h while its speculative lanes
            // read half h's rows: they read the snapshot of them instead (taken
            // by the launch before, or here), and the launch snapshots half 1 - h
            const int h = prop->half, hn = 1 - h;
            if (!sp->in && !snapshot_half(ws, prop->pos, h, prop->ns, T->ndim, st)) return LFG_E_LAUNCH;
            A.X.S[0].ppos = A.X.S[1].ppos = snap_rows(ws, h, T->ndim);
            A.snap_src = prop->pos + size_t(hn) * prop->ns * T->ndim;
            A.snap_dst = snap_rows(ws, hn, T->ndim);
        }
        fill_hot(A);
        if (fold_pair) launch_pair_split(kind == 2 ? PAIR_SPLIT_FOLD_LONG : PAIR_SPLIT_FOLD, unsigned(npairs), st, A);
        else if (T->gp) hipLaunchKernelGGL(k_pair<true>, dim3(npairs), dim3(LIKE_THREADS), 0, st, A);
        else if (kind == 2) launch_pair_split(PAIR_SPLIT_LONG, unsigned(npairs), st, A);
        else hipLaunchKernelGGL(k_pair<false>, dim3(npairs), dim3(LIKE_THREADS), 0, st, A);
    } else {
        // the partner half's rows, as the fused acceptance's k_pair leaves them
        if (snaps && acc && !snapshot_half(ws, prop->pos, 1 - prop->half, prop->ns, T->ndim, st)) return LFG_E_LAUNCH;
        // the deferred acceptance: a fold k_pair launch snapshots its own
        // half's rows (final until its verdicts are applied) for the next
        // launch's speculative lanes
        if (snaps && fold && !snapshot_half(ws, prop->pos, prop->half, prop->ns, T->ndim, st)) return LFG_E_LAUNCH;
        if (T->gp) {
            hipLaunchKernelGGL(k_gp_dcp, dim3((npairs + 64 / DCP_LANES - 1) / (64 / DCP_LANES)), dim3(64), 0, st, ws.geo,
                               ws.status, npairs);
            if ((rc = launch_ok())) return rc;
            if (T->nsub > 1) hipLaunchKernelGGL((k_lnlike<2, true>), dim3(npairs), dim3(LIKE_THREADS), 0, st, L);
            else hipLaunchKernelGGL((k_lnlike<2, false>), dim3(npairs), dim3(LIKE_THREADS), 0, st, L);
        } else {
            if (T->nsub > 1) hipLaunchKernelGGL((k_lnlike<1, true>), dim3(npairs), dim3(LIKE_THREADS), 0, st, L);
            else hipLaunchKernelGGL((k_lnlike<1, false>), dim3(npairs), dim3(LIKE_THREADS), 0, st, L);
        }
    }
    if ((rc = launch_ok())) return rc;
    return launch_tail(L, W, T, lnp, prop, fold_pair ? nullptr : fold, st, ev);
}

int lfg_lnprior(const double* walkers, int W, const lfg_tree* T, double* lnprior, void* wsp, size_t ws_bytes,
                void* stream)
{
    if (W <= 0 || !T || T->E <= 0 || T->ndim <= 0 || !walkers || !lnprior) return LFG_E_ARGS;
    Ws ws = carve(wsp, W, T->E);
    if (!wsp || ws_bytes < ws.total) return LFG_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SetupArgs S = setup_args_tree(walkers, W, T, ws, false, nullptr);
    const int nlanes = 2 * W * T->E + W;
    hipLaunchKernelGGL(k_setup, dim3((nlanes + SETUP_BLOCK - 1) / SETUP_BLOCK), dim3(SETUP_BLOCK), 0, st, S);
    int rc = launch_ok();
    if (rc) return rc;
    hipLaunchKernelGGL(k_combine, dim3((W + 255) / 256), dim3(256), 0, st, W, T->E, ws.prior, ws.geo, nullptr,
                       lnprior);
    return launch_ok();
}

int lfg_lnprob(const double* walkers, int W, const lfg_tree* T, double* lnp, double* lnlike_e, void* wsp,
               size_t ws_bytes, void* stream)
{
    return lnprob_impl(walkers, W, T, lnp, lnlike_e, wsp, ws_bytes, stream, nullptr);
}

int lfg_lnprob_timed(const double* walkers, int W, const lfg_tree* T, double* lnp, double* lnlike_e, void* wsp,
                     size_t ws_bytes, void* stream, void* const* ev)
{
    return lnprob_impl(walkers, W, T, lnp, lnlike_e, wsp, ws_bytes, stream, ev);
}

int lfg_stretch_step_half(double* pos, double* lnp, int W, int half, double a, unsigned long long seed,
                          unsigned long long step, double* q, double* zfac, const lfg_tree* T, int* naccept,
                          double* lnp_new, void* wsp, size_t ws_bytes, void* stream, void* const* ev)
{
    if (W < 4 || (W & 1) || (half != 0 && half != 1) || !(a > 1.0) || !pos || !lnp || !q || !zfac || !T)
        return LFG_E_ARGS;
    const Accept acc{pos, lnp, zfac, half, seed, step, naccept};
    const Propose prop{pos, a, q, zfac, half, seed, step, 0, W / 2};
    return lnprob_impl(q, W / 2, T, lnp_new, nullptr, wsp, ws_bytes, stream, ev, &acc, &prop);
}

int lfg_stretch_step_half_spec(double* pos, double* lnp, int W, int half, double a, unsigned long long seed,
                               unsigned long long step, double* q, double* zfac, const lfg_tree* T, int* naccept,
                               double* lnp_new, int spec_in, int spec_out, void* wsp, size_t ws_bytes, void* stream,
                               void* const* ev)
{
    if (W < 4 || (W & 1) || (half != 0 && half != 1) || !(a > 1.0) || !pos || !lnp || !q || !zfac || !T)
        return LFG_E_ARGS;
    const Accept acc{pos, lnp, zfac, half, seed, step, naccept};
    const Propose prop{pos, a, q, zfac, half, seed, step, 0, W / 2};
    const SpecCtl sp{spec_in != 0, spec_out != 0};
    return lnprob_impl(q, W / 2, T, lnp_new, nullptr, wsp, ws_bytes, stream, ev, &acc, &prop, &sp);
}

int lfg_stretch_step_shard(const double* pos, int W, int half, double a, unsigned long long seed,
                           unsigned long long step, int lo, int n, double* q, double* zfac, const lfg_tree* T,
                           double* lnp_new, void* wsp, size_t ws_bytes, void* stream, void* const* ev)
{
    if (W < 4 || (W & 1) || (half != 0 && half != 1) || !(a > 1.0) || !pos || !q || !zfac || !T || !lnp_new ||
        n <= 0 || lo < 0 || lo + n > W / 2)
        return LFG_E_ARGS;
    const Propose prop{pos, a, q, zfac, half, seed, step, lo, W / 2};
    return lnprob_impl(q, n, T, lnp_new, nullptr, wsp, ws_bytes, stream, ev, nullptr, &prop);
}

int lfg_stretch_step_shard_spec(const double* pos, int W, int half, double a, unsigned long long seed,
                                unsigned long long step, int lo, int n, double* q, double* zfac, const lfg_tree* T,
                                double* lnp_new, int spec_in, int spec_out, void* wsp, size_t ws_bytes,
                                void* stream, void* const* ev)
{
    if (W < 4 || (W & 1) || (half != 0 && half != 1) || !(a > 1.0) || !pos || !q || !zfac || !T || !lnp_new ||
        n <= 0 || lo < 0 || lo + n > W / 2)
        return LFG_E_ARGS;
    const Propose prop{pos, a, q, zfac, half, seed, step, lo, W / 2};
    const SpecCtl sp{spec_in != 0, spec_out != 0};
    return lnprob_impl(q, n, T, lnp_new, nullptr, wsp, ws_bytes, stream, ev, nullptr, &prop, &sp);
}

int lfg_stretch_step_shard_fold(double* pos, double* lnp, int W, int half, double a, unsigned long long seed,
                                unsigned long long step, int lo, int n, double* q, double* zfac, const lfg_tree* T,
                                const double* verdict_prev, double* verdict, double* lnp_new, int* naccept,
                                int spec_in, int spec_out, void* wsp, size_t ws_bytes, void* stream, void* const* ev)
{
    if (W < 4 || (W & 1) || (half != 0 && half != 1) || !(a > 1.0) || !pos || !lnp || !q || !zfac || !T ||
        !lnp_new || !verdict || n <= 0 || lo < 0 || lo + n > W / 2 || (spec_in && !verdict_prev) ||
        (verdict_prev && half == 0 && step == 0))
        return LFG_E_ARGS;
    const Propose prop{pos, a, q, zfac, half, seed, step, lo, W / 2};
    const SpecCtl sp{spec_in != 0, spec_out != 0};
    const FoldCtl fold{verdict_prev, verdict, pos, lnp, naccept};
    return lnprob_impl(q, n, T, lnp_new, nullptr, wsp, ws_bytes, stream, ev, nullptr, &prop, &sp, &fold);
}

int lfg_stretch_apply_verdicts(double* pos, double* lnp, int W, int ndim, int half, double a, unsigned long long seed,
                               unsigned long long step, const double* verdict, int* naccept, void* stream)
{
    if (W < 4 || (W & 1) || ndim <= 0 || (half != 0 && half != 1) || !(a > 1.0) || !pos || !lnp || !verdict)
        return LFG_E_ARGS;
    return apply_verdicts(pos, lnp, W, ndim, half, a, verdict, seed, step, naccept, nullptr,
                          static_cast<hipStream_t>(stream));
}

int lfg_stretch_lnprob_accept(double* pos, double* lnp, int W, int half, const double* q, const double* zfac,
                              const lfg_tree* T, unsigned long long seed, unsigned long long step, int* naccept,
                              double* lnp_new, void* wsp, size_t ws_bytes, void* stream, void* const* ev)
{
    if (W < 4 || (W & 1) || (half != 0 && half != 1) || !pos || !lnp || !q || !zfac || !T) return LFG_E_ARGS;
    const Accept acc{pos, lnp, zfac, half, seed, step, naccept};
    return lnprob_impl(q, W / 2, T, lnp_new, nullptr, wsp, ws_bytes, stream, ev, &acc);
}

static int propose_impl(const double* pos, int W, int ndim, int half, double a, unsigned long long seed,
                        unsigned long long step, const unsigned long long* stepp, double* q, double* zfac,
                        void* stream)
{
    if (W < 4 || (W & 1) || ndim <= 0 || (half != 0 && half != 1) || !(a > 1.0) || !pos || !q || !zfac)
        return LFG_E_ARGS;
    const int ns = W / 2;
    hipLaunchKernelGGL(k_propose, dim3((ns + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), pos, W,
                       ndim, half, a, seed, step, stepp, q, zfac);
    return launch_ok();
}

static int accept_impl(double* pos, double* lnp, int W, int ndim, int half, const double* q, const double* zfac,
                       const double* lnp_new, unsigned long long seed, unsigned long long step,
                       const unsigned long long* stepp, int* naccept, void* stream)
{
    if (W < 4 || (W & 1) || ndim <= 0 || (half != 0 && half != 1) || !pos || !lnp || !q || !zfac || !lnp_new)
        return LFG_E_ARGS;
    const int ns = W / 2;
    hipLaunchKernelGGL(k_accept, dim3((ns + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), pos, lnp,
                       W, ndim, half, q, zfac, lnp_new, seed, step, stepp, naccept);
    return launch_ok();
}

int lfg_stretch_accept_regen(double* pos, double* lnp, int W, int ndim, int half, double a,
                             unsigned long long seed, unsigned long long step, const double* lnp_new, int* naccept,
                             void* stream)
{
    if (W < 4 || (W & 1) || ndim <= 0 || (half != 0 && half != 1) || !(a > 1.0) || !pos || !lnp || !lnp_new)
        return LFG_E_ARGS;
    const int ns = W / 2;
    hipLaunchKernelGGL(k_accept_regen, dim3((ns + REGEN_WAVES - 1) / REGEN_WAVES), dim3(64 * REGEN_WAVES), 0,
                       static_cast<hipStream_t>(stream), pos, lnp, W, ndim, half, a, lnp_new, seed, step, naccept,
                       nullptr);
    return launch_ok();
}

int lfg_stretch_accept_regen_spec(double* pos, double* lnp, int W, int half, double a, unsigned long long seed,
                                  unsigned long long step, const double* lnp_new, int* naccept, const lfg_tree* T,
                                  int n, void* wsp, size_t ws_bytes, void* stream)
{
    if (W < 4 || (W & 1) || (half != 0 && half != 1) || !(a > 1.0) || !pos || !lnp || !lnp_new || !T ||
        T->ndim <= 0 || n <= 0 || n > W / 2)
        return LFG_E_ARGS;
    const Ws ws = carve(wsp, n, T->E, T->gp ? T->max_n : 0, T->ndim, W / 2);
    if (!wsp || ws_bytes < ws.total) return LFG_E_WORKSPACE;
    const int ns = W / 2;
    hipLaunchKernelGGL(k_accept_regen, dim3((ns + REGEN_WAVES - 1) / REGEN_WAVES), dim3(64 * REGEN_WAVES), 0,
                       static_cast<hipStream_t>(stream), pos, lnp, W, T->ndim, half, a, lnp_new, seed, step, naccept,
                       ws.accflag + size_t(half) * ws.accstride);
    return launch_ok();
}

int lfg_stretch_propose(const double* pos, int W, int ndim, int half, double a, unsigned long long seed,
                        unsigned long long step, double* q, double* zfac, void* stream)
{
    return propose_impl(pos, W, ndim, half, a, seed, step, nullptr, q, zfac, stream);
}

int lfg_stretch_accept(double* pos, double* lnp, int W, int ndim, int half, const double* q, const double* zfac,
                       const double* lnp_new, unsigned long long seed, unsigned long long step, int* naccept,
                       void* stream)
{
    return accept_impl(pos, lnp, W, ndim, half, q, zfac, lnp_new, seed, step, nullptr, naccept, stream);
}

int lfg_stretch_propose_dev(const double* pos, int W, int ndim, int half, double a, unsigned long long seed,
                            const unsigned long long* step_dev, double* q, double* zfac, void* stream)
{
    if (!step_dev) return LFG_E_ARGS;
    return propose_impl(pos, W, ndim, half, a, seed, 0, step_dev, q, zfac, stream);
}

int lfg_stretch_accept_dev(double* pos, double* lnp, int W, int ndim, int half, const double* q,
                           const double* zfac, const double* lnp_new, unsigned long long seed,
                           const unsigned long long* step_dev, int* naccept, void* stream)
{
    if (!step_dev) return LFG_E_ARGS;
    return accept_impl(pos, lnp, W, ndim, half, q, zfac, lnp_new, seed, 0, step_dev, naccept, stream);
}

int lfg_event_create(void** ev)
{
    if (!ev) return LFG_E_ARGS;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return LFG_E_LAUNCH;
    *ev = static_cast<void*>(e);
    return LFG_OK;
}

int lfg_event_destroy(void* ev)
{
    return hipEventDestroy(static_cast<hipEvent_t>(ev)) == hipSuccess ? LFG_OK : LFG_E_LAUNCH;
}

int lfg_event_elapsed_ms(void* start, void* stop, float* ms)
{
    if (!ms) return LFG_E_ARGS;
    return hipEventElapsedTime(ms, static_cast<hipEvent_t>(start), static_cast<hipEvent_t>(stop)) == hipSuccess
               ? LFG_OK
               : LFG_E_LAUNCH;
}

int lfg_elements(const double* pars, int W, int P, double* a, double* b, double* wgt, double* donor,
                 double* geo, int* status, void* wsp, size_t ws_bytes, void* stream)
{
    if (W <= 0 || (P != 14 && P != 18) || !pars) return LFG_E_ARGS;
    Ws ws = carve(wsp, W, 1);
    if (!wsp || ws_bytes < ws.total) return LFG_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SetupArgs S = setup_args_flat(pars, W, P, ws);
    // k_setup writes the slots a set's model defines and stops at a failure:
    // the rest of the record is copied out below, so it must not be whatever
    // the scratch held (lfg.h: those slots are 0)
    if (geo && hipMemsetAsync(ws.geo, 0, size_t(W) * LFG_NGEO * sizeof(double), st) != hipSuccess) return LFG_E_LAUNCH;
    int rc = run_front(S, ws, st, nullptr, true);  // the white-box tables come from k_elements
    if (rc) return rc;
    if (a || b || wgt || donor) {
        const long nt = long(W) * NEL;
        hipLaunchKernelGGL(k_expand, dim3(unsigned((nt + 255) / 256)), dim3(256), 0, st, ws.geo, ws.status, W, ws.ab,
                           ws.donor, a, b, wgt, donor);
        if ((rc = launch_ok())) return rc;
    }
    bool ok = true;
    if (geo)
        ok &= hipMemcpyAsync(geo, ws.geo, size_t(W) * LFG_NGEO * sizeof(double), hipMemcpyDeviceToDevice, st) ==
              hipSuccess;
    if (status) ok &= hipMemcpyAsync(status, ws.status, sizeof(int) * W, hipMemcpyDeviceToDevice, st) == hipSuccess;
    return ok ? LFG_OK : LFG_E_LAUNCH;
}

int lfg_roche(int op, const double* a, const double* b, int n, double* out, int* status, void* stream)
{
    if (op < 0 || op > 3 || n < 0 || !a || !out || !status || (op > 0 && !b)) return LFG_E_ARGS;
    if (n == 0) return LFG_OK;
    hipLaunchKernelGGL(k_roche, dim3((n + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), op, a, b, n,
                       out, status);
    return launch_ok();
}

int lfg_wdphases(const double* q, const double* inc, const double* r1, int n, int ntheta, double* phi3,
                 double* phi4, int* status, void* stream)
{
    if (n < 0 || ntheta < 1 || (n > 0 && (!q || !inc || !r1 || !phi3 || !phi4 || !status))) return LFG_E_ARGS;
    if (n == 0) return LFG_OK;
    hipLaunchKernelGGL(k_wdphases, dim3((n + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), q, inc, r1,
                       n, ntheta, phi3, phi4, status);
    return launch_ok();
}

int lfg_gp_lnlike(const double* x, const double* ye, const double* res, int W, int N, const double* hyp,
                  const double* blocks, int nb, double* lnlike, void* stream)
{
    if (W <= 0 || N < 0 || nb < 0 || !hyp || !lnlike || (N > 0 && (!x || !ye || !res)) || (nb > 0 && !blocks))
        return LFG_E_ARGS;
    hipLaunchKernelGGL(k_gp, dim3(W), dim3(64), 0, static_cast<hipStream_t>(stream), x, ye, res, N, hyp, blocks, nb,
                       lnlike);
    return launch_ok();
}

// lfg_gp_predict.hip's window on what lfg_lnprob leaves in a GP tree's
// workspace (carve()'s layout; not part of include/lfg.h): every pair's
// record, status, residuals [pairs][max_n] and block indices, and the
// walkers' ln_prior
int lfg_tree_gp_views(void* wsp, int W, const lfg_tree* T, const double** geo, const int** status,
                      const double** prior, const double** res, const int** gpb)
{
    if (!wsp || W <= 0 || !T || T->E <= 0 || !T->gp) return LFG_E_ARGS;
    const Ws ws = carve(wsp, W, T->E, T->max_n);
    *geo = ws.geo;
    *status = ws.status;
    *prior = ws.prior;
    *res = ws.res;
    *gpb = ws.gpb;
    return LFG_OK;
}

#ifdef LFG_PROFILE_LIKE
// diagnostic build only: k_lnlike prologue stamps
int lfg_debug_like_cycles(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_like_cyc), sizeof(g_like_cyc)) == hipSuccess ? 0 : -1;
}

// per-wave phase stamps: host [2][6][4096] (min, max over the block's waves);
// reset (host == nullptr): min slots to ~0, max slots to 0
int lfg_debug_like_waves(unsigned long long* host)
{
    static unsigned long long buf[2][6][4096];
    if (!host) {
        for (int i = 0; i < 6 * 4096; ++i) { (&buf[0][0][0])[i] = ~0ull; (&buf[1][0][0])[i] = 0ull; }
        return hipMemcpyToSymbol(HIP_SYMBOL(g_like_wav), buf, sizeof(buf)) == hipSuccess ? 0 : -1;
    }
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_like_wav), sizeof(g_like_wav)) == hipSuccess ? 0 : -1;
}
#endif

#ifdef LFG_PROFILE_PAIR
// diagnostic build only: k_pair's phase stamps of the last launch, host [20][4096]
int lfg_debug_pair(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pair_t), sizeof(g_pair_t)) == hipSuccess ? 0 : -1;
}
// its per-chunk job stamps (start, sink entry, end), host [3][16][4096]
int lfg_debug_pair_jobs(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pair_j), sizeof(g_pair_j)) == hipSuccess ? 0 : -1;
}
// and its per-wave sweep stamps, host [4][8][4096]
int lfg_debug_pair_waves(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pair_w), sizeof(g_pair_w)) == hipSuccess ? 0 : -1;
}
int lfg_debug_long_tables(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_long_t), sizeof(g_long_t)) == hipSuccess ? 0 : -1;
}
#endif

#ifdef LFG_PROFILE_ELEM
// diagnostic build only: k_elements' per-wave stamps of the last launch, host [4][32768]
int lfg_debug_elem_waves(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_elem_wav), sizeof(g_elem_wav)) == hipSuccess ? 0 : -1;
}
#endif

#ifdef LFG_PROFILE_SETUP
// diagnostic build only: copy the k_setup lane stamps to the host
int lfg_debug_setup_cycles(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_setup_cyc), sizeof(g_setup_cyc)) == hipSuccess ? 0 : -1;
}
#endif

// the hash of the sources and flags this library was built from
// (lfit_python_amd._native.source_hash, passed by build()); the tag string
// lets build() read it back from the file without loading it
#ifndef LFG_SRC_HASH
#define LFG_SRC_HASH "unhashed"
#endif
__attribute__((used)) const char lfg_src_hash_tag[] = "lfg-src-hash:" LFG_SRC_HASH;

const char* lfg_version(void)
{
    // the layout named is the one lfg_set_layout / LFG_PAIR currently select
    // for eligible trees (pair: k_pair and k_pair LONG; two_kernel: k_elements
    // + k_lnlike); lfg_layout(T) gives a given tree's kernels
    int m = g_pair_layout.load(std::memory_order_relaxed);
    if (m == -2) m = pair_env() ? 1 : 0;
    return m == 1 ? "lfg 0.5.0 gfx950 fp64 layout=pair src=" LFG_SRC_HASH
                  : "lfg 0.5.0 gfx950 fp64 layout=two_kernel src=" LFG_SRC_HASH;
}

#ifdef LFG_COUNT_ITERS
// diagnostic builds only: read and clear the iteration counters of k_elements
int lfg_diag_iters(unsigned long long* out)
{
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out, HIP_SYMBOL(g_iter_dbg), sizeof(g_iter_dbg)) != hipSuccess)
        return LFG_E_LAUNCH;
    unsigned long long z[64] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_iter_dbg), z, sizeof(z)) == hipSuccess ? LFG_OK : LFG_E_LAUNCH;
}
#endif

}  // extern "C"
#endif  // LFG_NOLICM_TU
