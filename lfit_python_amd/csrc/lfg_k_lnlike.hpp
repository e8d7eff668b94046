// lfg_k_lnlike.hpp -- k_lnlike's section: the DPP sums and scans, LikeArgs,
// the sweeps, TileBufs, the sub-bin tables and the template k_lnlike<MODE,
// SUB> (instantiated by lfg.hip's launches only).  Needs before it:
// lfg_sweep.hpp, lfg_kernels.hpp's prelude and lfg_k_elements.hpp; included
// by lfg_kernels.hpp, in its anonymous namespace.
#pragma once

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
