// lfg.hip -- the host unit of liblfg_hip.so for MI355X (gfx950): the
// workspace layout, the launches and the C ABI of include/lfg.h.
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
// Here: Ws and carve (the workspace), then launch_pair_split, extern "C" and
// the lfg_debug_* / lfg_diag_iters readers.  No device code is written in
// this file; the kernels come through headers:
//   lfg_kernels.hpp     all that k_pair is made of, also compiled by
//                       lfg_pair_split.hip: the prelude, lfg_philox.hpp, and
//     lfg_k_setup.hpp     SetupArgs, Prop, the setup / prior / stream lanes
//     lfg_k_elements.hpp  ElemSpec, ElemOut, MemSink, element_lane, elem_ab
//     lfg_k_lnlike.hpp    LikeArgs, the sweeps, TileBufs, the sub-bin tables, k_lnlike<MODE, SUB>
//     lfg_k_pair.hpp      k_pair (its LONG tables: lfg_k_pair_long.hpp)
//   lfg_k_front.hpp     the __global__ definitions of k_setup, k_elements, k_expand
//   lfg_k_gp.hpp        k_gp_dcp, k_gp_like, k_combine_walkers, k_combine
//   lfg_k_stretch.hpp   k_propose, k_accept, k_accept_regen, k_apply_verdicts, k_verdict
//   lfg_k_misc.hpp      k_gp, k_wdphases, k_roche; launch_ok, mark_event, run_front
// Replaces, per walker, mcmcfit.ln_prob (mcmcfit.py:37-41) -> Node.ln_prob
// (model.py:476-498) -> lfit.CV.calcFlux (CVModel.py:138).
#include "lfg_kernels.hpp"

namespace {

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

#include "lfg_k_front.hpp"  // the __global__ definitions of k_setup, k_elements, k_expand

// the kernels k_pair needs nothing of, and the host's run_front: one header per section
#include "lfg_k_gp.hpp"
#include "lfg_k_stretch.hpp"
#include "lfg_k_misc.hpp"

}  // namespace

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
