// lfg_k_elements.hpp -- k_elements' section: ElemSpec, ElemOut, MemSink,
// element_lane, elem_ab and the LFG_PROFILE_ELEM / LFG_COUNT_ITERS globals.
// No __global__ definition (k_elements and k_expand: lfg_k_front.hpp).  Needs
// before it: lfg_kernels.hpp's prelude and lfg_k_setup.hpp (SetupArgs,
// setup_any); included by lfg_kernels.hpp, in its anonymous namespace.
#pragma once

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

