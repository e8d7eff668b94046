// lfg_k_setup.hpp -- k_setup's section: SetupArgs, Prop, and the setup, prior
// and stream lanes behind setup_any.  No __global__ definition (k_setup
// itself: lfg_k_front.hpp).  Needs before it: lfg_device.hpp, lfg_philox.hpp
// and lfg_kernels.hpp's prelude; included by lfg_kernels.hpp, in its
// anonymous namespace.
#pragma once

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


