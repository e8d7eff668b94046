// lfg_k_pair.hpp -- k_pair: PairHot, PairArgs, fill_hot, PairSink and the
// point-major sinks, the LONG tables (lfg_k_pair_long.hpp, included where
// they stood) and the kernel.  Needs before it: lfg_k_setup.hpp,
// lfg_k_elements.hpp and lfg_k_lnlike.hpp.  Included by lfg_kernels.hpp, in
// its anonymous namespace, and so in both lfg.hip's and lfg_pair_split.hip's
// units.
#pragma once

// ------------------------------------------------------------------ k_pair
// k_elements and k_lnlike<1, false> of one (walker, eclipse) pair in ONE
// workgroup, for trees whose eclipses fit one tile (max_n <= LIKE_TILE, S =
// 1, no GP): the element intervals never leave the workgroup, the half-step
// is one launch instead of two (no kernel boundary behind a 10 MB table
// write-back, no re-fetch of the tables), and the interval sweep runs inside
// the element phase: a lane that has solved an element adds its runs to the
// LDS difference arrays at once, while other waves are still solving.
//  * prologue: every thread forms its point's window and phase (and its
//    predecessor's, for the sortedness flags and the phase-index cells, so
//    no barrier is needed for them), the disc ring weights (21 lanes);
//  * element phase: 16 jobs, wave w takes job w and grabs the next free one
//    from an LDS counter twice more.  Job 0: this block's share of the
//    speculative setup lanes of the next half (setup_any, as k_elements'
//    leading blocks run them); jobs 1..15: the 15 chunks of 64 items, longest
//    first.  Each solved item is swept (element and mirror for WD/disc, the
//    four mirrored donor tiles) with k_lnlike's run / point-mode rules.  The
//    spot and donor sums are accumulated unnormalised (int64 fixed point at
//    2^-54 / 2^-58, exact) with their totals, and normalised per point;
//  * after the phase barrier: the block scan, each point's flux, chi^2, the
//    fused acceptance.  Unsorted or invalid windows: the tables go to LDS and
//    the point-major pass runs instead (as k_lnlike's).
// With the fused acceptance the block writes its walker's row of pos while
// the speculative lanes of other blocks read partner rows of the same half:
// those lanes read the snapshot (SetupArgs.ppos) that the launch before took
// of that half, and this launch snapshots the other half for the next one.
typedef const __attribute__((address_space(4))) double* CGeo;
constexpr int DCP_LANES = 16, DCP_NTHETA = 10;  // k_gp_dcp / k_pair<true>: limb points of wdphases

// The arguments of k_pair's prologue chains, contiguous, read at the entry in
// one batch of scalar loads (kernarg_copy): the compiler otherwise issued them
// in ~10 rounds, each behind an s_waitcnt for every outstanding load, ahead of
// the candidate chain.  Copies of the LikeArgs / ElemSpec / PairArgs fields
// of the same names (fill_hot, on the host, before each launch), typed by
// address space: the uniform read-only words constant (scalar loads), the
// points global (a copied generic pointer would make flat loads)
typedef const __attribute__((address_space(4))) int* KInt;
typedef const __attribute__((address_space(4))) double* KDbl;
typedef const __attribute__((address_space(1))) double* GDbl;
struct PairHot {
    KInt accflag;   // X.accflag (the partner half's flags: this launch writes the other half's)
    KDbl fv;        // fv (FOLD)
    KInt jk;        // X.jk
    KInt statusC;   // X.statusC, X.bstatusC, X.priorC, X.geoC (this half's candidates; the
    KInt bstatusC;  //   speculative lanes write the next half's)
    KDbl priorC;
    KDbl geoC;
    KDbl geo;       // L.geo, L.status, L.bstatus, L.prior (read before B0; wave 7 writes
    KInt status;    //   the standard slots after it)
    KInt bstatus;
    KDbl prior;
    KInt off;       // L.off, L.x, L.w
    GDbl x;
    GDbl w;
    unsigned long long jseed, jstep;
    int jhalf, jlo, jns, E, N, npairs;
};

struct PairArgs {
    LikeArgs L;
    ElemSpec X;                // candidate selection (X.jk) and speculative lanes (X.nspec, X.S)
    const double* snap_src;    // nullable: rows [ns][ndim] of the other half of pos, copied to snap_dst
    double* snap_dst;
    int spl;                   // speculative lanes per block that has them (64: wave 0's job 0)
    int nbc;                   // blocks [0, nbc) carry candidate 0's lanes, [nbc, 2 nbc) candidate 1's
    // with X.jk: walker w's partner j in the other half, drawn here as the
    // speculative lanes drew it (make_prop: draw(seed, step, half, 0, lo + w),
    // j = umulhi(r.z, ns)) instead of read back from X.jk, one dependent
    // global load less before the candidate is known
    unsigned long long jseed, jstep;
    int jhalf, jlo, jns;
    int prio;  // blocks [0, prio) take the wave priorities (PAIR_PRIO; pair_prio)
    // FOLD (lfg_stretch_step_shard_fold): the partner half's moves of the
    // half-step before are accepted here, from the verdicts every rank
    // gathered (fv [jns]: ln_prob where accepted, NaN where not; nullptr:
    // nothing pending), each workgroup taking rows w, w + nwk, ...; the pair's
    // candidate is chosen by the same verdicts, and the launch leaves its own
    // verdicts in vout [npairs] (the next exchange's payload)
    const double* fv = nullptr;
    double* vout = nullptr;
    double* fpos = nullptr;   // the ensemble [W][ndim], ln_prob [W], counters [W]
    double* flnp = nullptr;
    int* fnacc = nullptr;
    double* fsnap = nullptr;  // [jns][ndim]: this half's rows, for the next launch's speculative lanes
    unsigned long long fstep = 0;  // the step of the pending moves' proposals
    double fa = 2.0;               // the stretch scale a
    PairHot hot{};                 // fill_hot
};

// PairArgs.hot from the fields it copies (every k_pair launch, last)
static void fill_hot(PairArgs& A)
{
    PairHot& H = A.hot;
    H.accflag = (KInt)A.X.accflag;
    H.fv = (KDbl)A.fv;
    H.jk = (KInt)A.X.jk;
    H.statusC = (KInt)A.X.statusC;
    H.bstatusC = (KInt)A.X.bstatusC;
    H.priorC = (KDbl)A.X.priorC;
    H.geoC = (KDbl)A.X.geoC;
    H.geo = (KDbl)A.L.geo;
    H.status = (KInt)A.L.status;
    H.bstatus = (KInt)A.L.bstatus;
    H.prior = (KDbl)A.L.prior;
    H.off = (KInt)A.L.off;
    H.x = (GDbl)A.L.x;
    H.w = (GDbl)A.L.w;
    H.jseed = A.jseed;
    H.jstep = A.jstep;
    H.jhalf = A.jhalf;
    H.jlo = A.jlo;
    H.jns = A.jns;
    H.E = A.L.E;
    H.N = A.L.N;
    H.npairs = A.L.npairs;
}

// The kernel-argument segment as a typed constant pointer whose value the
// compiler cannot see through.  k_pair's arguments are ~1 KB; the compiler
// loaded the speculative lanes' two SetupArgs (560 B, used by wave 0 of a few
// blocks) at every wave's entry and spilled them into VGPR lanes, a chain of
// ~15 dependent scalar-load waits (~3 us) ahead of the candidate chain.
// Fields read through this pointer are loaded where they are used.
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(4))) T* opaque_kernargs()
{
    auto p = (const __attribute__((address_space(4))) T*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// a by-value copy of a kernel-argument struct read through such a pointer
// (word by word: the struct's copy constructor takes a generic reference)
template <typename T>
__device__ __forceinline__ T kernarg_copy(const __attribute__((address_space(4))) T* p)
{
    static_assert(sizeof(T) % 8 == 0, "whole words");
    const auto* src = reinterpret_cast<const __attribute__((address_space(4))) unsigned long long*>(p);
    unsigned long long w[sizeof(T) / 8];
#pragma unroll
    for (int i = 0; i < int(sizeof(T) / 8); ++i) w[i] = src[i];
    T out;
    __builtin_memcpy(&out, w, sizeof(T));
    return out;
}

// the chunks of k_pair's element jobs 1..15, longest first (spot, outer
// disc, donor, inner disc, WD: the Newton steps per region)
__constant__ int kJobChunk[15] = {11, 12, 10, 9, 8, 13, 14, 7, 6, 5, 4, 3, 2, 1, 0};

// fixed-point scales of k_pair's unnormalised spot and donor sums, as
// factors into to_fx's 2^61: spot weights <= 1 (100 of them: 2^54), donor
// vectors (their |v| sums stay far below 2^5: 2^58)
constexpr double PAIR_SPOT_S = 1.0 / 128.0, PAIR_DON_S = 1.0 / 8.0;

#ifdef LFG_PROFILE_PAIR  // diagnostic build only: s_memrealtime (100 MHz) stamps of each block's phases
__device__ unsigned long long g_pair_t[24][4096];
#define PAIR_STAMP(slot, cond)                                                     \
    do {                                                                           \
        if ((cond) && blockIdx.x < 4096) g_pair_t[slot][blockIdx.x] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
__device__ unsigned long long g_pair_w[4][8][4096];
__device__ unsigned long long g_long_t[8][4096];  // the LONG table build's steps (thread 0 after each barrier)
#define LONG_TSTAMP(k)                                                                      \
    do {                                                                                    \
        if (tid == 0 && blockIdx.x < 4096) g_long_t[k][blockIdx.x] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
__device__ unsigned long long g_pair_j[3][16][4096];  // per chunk: job start, sink entry, end
#define PAIR_WSTAMP(k)                                                                                  \
    do {                                                                                                \
        if (lane == 0 && blockIdx.x < 4096) g_pair_w[k][wv][blockIdx.x] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define PAIR_STAMP(slot, cond)
#define LONG_TSTAMP(k)
#define PAIR_WSTAMP(k)
#endif

// wave priority in a launch of at most two rounds (blocks [0, A.prio)): the
// issue arbiter favours the older of a CU's two workgroups, so one finished
// ~10 us before the other and the CU ran its last phases on half its waves.
// Element waves drop their priority with each job they start (3, 2, 1, then
// 0), so both workgroups advance together; the speculative setup waves
// (latency-bound, and the longest job) keep 3.  In a launch of many rounds
// the older workgroup's early finish lets the next round's start, so the
// default order stays (pair_prio)
#define PAIR_PRIO(p)                                                    \
    do {                                                                \
        if (int(blockIdx.x) < A.prio) __builtin_amdgcn_s_setprio(p);    \
    } while (0)

// k_pair's sweep of one solved item (the element phase's sink): element runs
// over the tile's windows (WD, disc, spot) and the donor tiles' visibility
// arcs over the point phases, into the LDS difference arrays; or, for a tile
// that goes point-major, the tables
struct PairSink {
    bool dir;
    int lane;
    PhaseIndex XW, XP;      // windows (lo, cells) and point phases (sph, scp)
    const double* hi;
    const double* iw;
    unsigned long long (*acc)[LIKE_TILE + 1];   // sacc
    unsigned long long (*acc2)[LIKE_TILE + 1];  // second WD/disc copies (odd lanes)
    unsigned long long* tot;                    // [2] spot weight and donor quadrature sums
    const double* swt;      // disc ring weights, disc total
    double ul, itwd, s, c;  // ulimb, 1 / (2 pi (F(1) - F(0))), sin / cos i
    double2* ab;            // point-major: the WD/disc intervals, spot intervals and weights, donor tiles
    double2* sab;
    double* sbw;
    double* sdq;
    unsigned long long* mk;  // diagnostic builds: where mark() stamps the sink's entry
    // lane-local sums flushed once per wave (flush): the spot weight and donor
    // quadrature totals, and the donor arcs that open at the tile's first point
    // (all 64 lanes of a wave added these to the same LDS word: 64-way conflicts)
    long long tspot, tdon, bx, by, bz;

    __device__ __forceinline__ void mark()
    {
#ifdef LFG_PROFILE_PAIR
        if (mk) *mk = __builtin_amdgcn_s_memrealtime();
#endif
    }
    __device__ __forceinline__ void wd_disc(int u, double a, double b)
    {
#ifdef LFG_ABL_SINK_WD  // (diagnostic builds) the sink skipped: LDS counter attribution only
        return;
#endif
        if (dir) {
            ab[uslot(u)] = make_double2(a, b);
            return;
        }
        if (!(a < b)) return;
        const int ir = pair_ring(u);
#if LFG_PAIR_SINK_MERGE
        const double wn = (u < U_WD) ? wd_ring_weight(ir, ul) * itwd : swt[ir - NWD_RINGS] * swt[NDISC_R + 1];
#else
        const double wn = (u < U_WD) ? wd_ring_weight(ir, ul) * itwd : swt[ir - NWD_RINGS] * (1.0 / swt[NDISC_R]);
#endif
        double q[4] = {a, b, -b, -a};  // the element and its mirror [-b, -a]
        int J[4], Jb[4];
        count_lt_multi<4>(XW, q, J);
        count_le_back_multi<4>(hi, q, J, Jb);
        unsigned long long* A = ((lane & 1) ? acc2 : acc)[(u < U_WD) ? 0 : 1];
        const Runs RR[2] = {Runs{Jb[0], J[0], Jb[1], J[1]}, Runs{Jb[2], J[2], Jb[3], J[3]}};
        const double aa[2] = {a, -b}, bb[2] = {b, -a};
#if LFG_PAIR_SINK_MERGE
        apply_runs_merged<2>(RR, aa, bb, wn, XW, hi, iw, A);
#else
        apply_runs_batched<2>(RR, aa, bb, wn, XW, hi, iw, A);
#endif
    }
    __device__ __forceinline__ void spot(int j, double a, double b, double w)
    {
        sab[j] = make_double2(a, b);
        sbw[j] = w;
        tspot += to_fx(w * PAIR_SPOT_S);
#ifdef LFG_ABL_SINK_SPOT  // (diagnostic builds) the runs skipped: LDS counter attribution only
        if (false) {
#else
        if (!dir && a < b) {
#endif
            const Runs RR[1] = {element_runs(a, b, XW, hi)};
            const double aa[1] = {a}, bb[1] = {b};
#if LFG_PAIR_SINK_MERGE
            apply_runs_merged<1>(RR, aa, bb, w * PAIR_SPOT_S, XW, hi, iw, acc[2]);
#else
            apply_runs_batched<1>(RR, aa, bb, w * PAIR_SPOT_S, XW, hi, iw, acc[2]);
#endif
        }
    }
    __device__ __forceinline__ void donor(int uu, double vx0, double vy0, double vz0, double cen0, double hw0)
    {
        double* D = sdq + uu * DON_STRIDE;
        D[0] = vx0;
        D[1] = vy0;
        D[2] = vz0;
        D[3] = cen0;
        D[4] = hw0;
        long long tn = 0;
        // the arcs' point ranges first (LDS reads), then their entries
        int PA[4][2], QA[4][2];
#pragma unroll
        for (int mr = 0; mr < 4; ++mr) {  // the tile's mirror images, as k_lnlike's donor lanes form them
            const double vy = (mr & 1) ? -vy0 : vy0, vz = (mr & 2) ? -vz0 : vz0;
            const double cen = (mr & 1) ? -cen0 : cen0;
            const double hw = (mr & 2) ? 0.5 - hw0 : hw0;
            tn += to_fx(fmax(-s * vy + c * vz, 0.0) * PAIR_DON_S);
            PA[mr][0] = QA[mr][0] = PA[mr][1] = QA[mr][1] = 0;
#ifdef LFG_ABL_SINK_DON  // (diagnostic builds) the arcs skipped: LDS counter attribution only
            continue;
#endif
            if (dir || !(hw > 0.0)) continue;
            // visible for phases in (cen - hw, cen + hw) mod 1
            double x1 = -INFINITY, x2 = INFINITY, y1 = 0.0, y2 = 0.0;
            bool two = false;
            if (hw < 0.5) {
                const double lo = cen - hw, hi2 = cen + hw;
                if (lo < -0.5) { x2 = hi2; y1 = lo + 1.0; y2 = INFINITY; two = true; }
                else if (hi2 > 0.5) { x1 = lo; y1 = -INFINITY; y2 = hi2 - 1.0; two = true; }
                else { x1 = lo; x2 = hi2; }
            }
            PA[mr][0] = count_below<true>(XP, x1);
            QA[mr][0] = count_below<false>(XP, x2);
            if (two) {
                PA[mr][1] = count_below<true>(XP, y1);
                QA[mr][1] = count_below<false>(XP, y2);
            }
        }
        const long long qx = to_fx(vx0 * PAIR_DON_S), qy0 = to_fx(vy0 * PAIR_DON_S), qz0 = to_fx(vz0 * PAIR_DON_S);
#pragma unroll
        for (int mr = 0; mr < 4; ++mr) {
            const long long qy = (mr & 1) ? -qy0 : qy0, qz = (mr & 2) ? -qz0 : qz0;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int P = PA[mr][i], Q = QA[mr][i];
                if (P < Q) {
                    if (P == 0) {
                        bx += qx;
                        by += qy;
                        bz += qz;
                    } else {
                        fx_add(acc[3], P, qx);
                        fx_add(acc[4], P, qy);
                        fx_add(acc[5], P, qz);
                    }
                    if (Q < XP.m) {
                        fx_add(acc[3], Q, -qx);
                        fx_add(acc[4], Q, -qy);
                        fx_add(acc[5], Q, -qz);
                    }
                }
            }
        }
        tdon += tn;
    }
    // the lane-local sums into LDS: every lane of the wave calls it, after its
    // last item (the integer sums are exact in any order)
    __device__ __forceinline__ void flush()
    {
        const long long t0 = wave_total(tspot), t1 = wave_total(tdon);
        const long long x = wave_total(bx), y = wave_total(by), z = wave_total(bz);
        if (lane == 0) {
            if (t0) atomicAdd(tot, static_cast<unsigned long long>(t0));
            if (t1) atomicAdd(tot + 1, static_cast<unsigned long long>(t1));
            if (x) fx_add(acc[3], 0, x);
            if (y) fx_add(acc[4], 0, y);
            if (z) fx_add(acc[5], 0, z);
        }
    }
};

// point-major WD and disc eclipse fractions of one window (k_pair's
// unsorted-tile pass: direct_wd_disc with the ring weights formed here)
__device__ __forceinline__ double2 pair_direct_wd_disc(const double2* __restrict__ AB, double ul,
                                                       const double* __restrict__ swt, double phc, double wk,
                                                       double twd, double td)
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
        const double wr = ring < NWD_RINGS ? wd_ring_weight(ring, ul) : swt[ring - NWD_RINGS];
        if (ring < NWD_RINGS) ewd = fma(wr, acc, ewd); else ed = fma(wr, acc, ed);
    }
    const double nrm = window ? 1.0 / (2.0 * wk) : 1.0;
    return make_double2(ewd * nrm * (1.0 / twd), ed * nrm * (1.0 / td));
}

// a point's window: phase, lo, hi (k_lnlike's put_window arithmetic)
__device__ __forceinline__ void pair_window(double x, double w, double phi0, double& ph, double& lo, double& hi,
                                            double& hw)
{
    ph = wrap_phase(x - phi0);
    hw = w;
    lo = ph - hw;
    hi = ph + hw;
}

// the cells of phase index (v sorted, v[0] = v0, v[m-1] = v1) that point p
// fills, as build_cells does, from p's own value and its predecessor's
__device__ __forceinline__ void pair_cells(int* cell, int p, int m, double vprev, double vown, double v0, double v1)
{
    const double span = v1 - v0, ginv = span > 0.0 ? LIKE_NC / span : 0.0;
    auto ci = [&](double x) {
        const double u = (x - v0) * ginv;
        return u < 0.0 ? -1 : (u >= double(LIKE_NC) ? LIKE_NC : int(u));
    };
    const int g0 = p ? ci(vprev) : -1, g1 = ci(vown);
    for (int g = g0 + 1; g <= g1; ++g) cell[g] = p;
    if (p == m - 1)
        for (int g = g1 + 1; g <= LIKE_NC; ++g) cell[g] = m;
}

#include "lfg_k_pair_long.hpp"

// GP (GP trees, MODE 2 of k_lnlike): instead of chi^2 the residuals, each
// point's e^{-lam dx} and changepoint block go to the workspace for
// k_gp_like, and a walker that tripped the changepoint cache rule has its
// distance solved here (k_gp_dcp's ten limb points, on wave 0's lanes 32..)
// LONG: eclipses longer than a tile and sub-binned exposures (the LONG
// tables above, long_tables / long_wd_disc / sub_point): the element phase
// keeps the point-major sinks, and after the phase barrier the tables are
// built and every wave evaluates a cost-balanced range of the points
template <bool GP, bool FOLD = false, bool LONG = false>
__global__ __launch_bounds__(LIKE_THREADS, LIKE_MINW) void k_pair(PairArgs A)
{
    static_assert(!(GP && LONG), "GP trees keep the one-tile layout or the two kernels");
    const LikeArgs& L = A.L;
    const ElemSpec& X = A.X;
#if LFG_PAIR_SINK_MERGE
    // disc ring weights, the disc total and (one-tile sinks) its reciprocal (prologue)
    __shared__ double swt[NDISC_R + (LONG ? 1 : 2)];
    // the sinks' per-pair constants (wave 6, ahead of B0): itwd, then t0 and
    // ginv of the windows' and of the point phases' index (phase_index)
    __shared__ double skc[5];
#else
    __shared__ double swt[NDISC_R + 1];           // disc ring weights and the disc total (prologue)
#endif
    __shared__ double sbw[NBS];
    __shared__ double2 sab[NBS];
    __shared__ double sdq[U_DON * DON_STRIDE];
    __shared__ double sacc1[3];
    __shared__ TileBufs TA;
    __shared__ double sph[LIKE_TILE];
    // the second WD/disc difference arrays and the point-phase cells; or,
    // for a tile that goes point-major, the WD/disc intervals
    __shared__ union PairU_ {
        struct {
            unsigned long long X[2][LIKE_TILE + 1];
            int scp[LIKE_NC + 1];
        } s;
        double2 ab[NU_WDD];
    } SU;
    __shared__ unsigned long long sacc[6][LIKE_TILE + 1];
    __shared__ unsigned long long stot[2];
#if !LFG_PAIR_RUNSCAN
    __shared__ long long spart[6][LIKE_THREADS / 64];
#endif
    __shared__ double red[LIKE_THREADS / 64];
    __shared__ int sflagw[LIKE_THREADS / 64];
    __shared__ int sflag[1];
    __shared__ int sjob;
    __shared__ double sq[ACC_LDS];
    __shared__ double sy[LIKE_TILE], sye[LIKE_TILE];
    // LONG only (the one-tile instantiations reference none of these)
    __shared__ LongTabs LT;
    __shared__ SubTables LST;
    __shared__ SubEntries LSE;
    __shared__ double2 Lab[NU_WDD];
    __shared__ long long lspart[10][LIKE_THREADS / 64];

    constexpr int nt = LIKE_THREADS, nw = LIKE_THREADS / 64;
    // the prologue's arguments in one batch of scalar loads (PairHot)
    const PairHot H = kernarg_copy(&opaque_kernargs<PairArgs>()->hot);
    const int pair = blockIdx.x, npairs = H.npairs;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#ifdef LFG_ABL_EMPTY  // (diagnostic builds) the launch alone: traffic and instructions of an empty k_pair
    if (pair >= 0) return;
#endif
    PAIR_STAMP(0, tid == 0);
#ifdef LFG_PROFILE_PAIR
    if (tid == 0 && blockIdx.x < 4096) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_pair_t[14][blockIdx.x] = hw;
        g_pair_t[18][blockIdx.x] = xcc;
    }
#endif
    const int E = H.E;
    const int w = (E == 1) ? pair : pair / E, e = (E == 1) ? 0 : pair - w * E;
    const int nwk = npairs / E;  // walkers of the batch
    const bool offs = H.off && E > 1;
    const int o0 = offs ? H.off[e] : 0;
    const int n = offs ? H.off[e + 1] - o0 : H.N;

    // the point loads the windows need, issued first: they overlap the
    // candidate chain below (own point, predecessor, first and last)
    const bool own = !LONG && tid < n;
    const int m = n;
    const int pl = own ? tid : 0;
    const GDbl xe = H.x + o0;
    double xw_own = 0.0, xw_prv = 0.0, xw_0 = 0.0, xw_1 = 0.0;
    double ww_own = 0.0, ww_prv = 0.0, ww_0 = 0.0, ww_1 = 0.0;
    if (!LONG && n > 0) {
        xw_own = xe[pl];
        xw_prv = xe[pl > 0 ? pl - 1 : 0];
        xw_0 = xe[0];
        xw_1 = xe[n - 1];
    }
    PAIR_STAMP(20, tid == 0 && n != -7);
    if (!LONG && H.w && n > 0) {
        const GDbl we = H.w + o0;
        ww_own = we[pl];
        ww_prv = we[pl > 0 ? pl - 1 : 0];
        ww_0 = we[0];
        ww_1 = we[n - 1];
    }
    // ---- prologue: the pair's candidate (speculative setup) or standard
    // slots.  Only what the phase barrier B0 waits for is done here (the
    // barrier waits for every wave's outstanding memory operations): both
    // candidates' per-pair words are loaded alongside the selection chain
    // (jk -> accflag), and the copies into the standard slots, the snapshot
    // and the acceptance's prefetch follow B0 (wave 7's first task)
    const double* G;
    int st0, bst, cand = 0;
    double lpr = 0.0, zf = 0.0, rpr, phi0;
    if (H.jk) {
        const size_t c0 = size_t(pair), c1 = size_t(npairs) + pair;
        const int sa0 = H.statusC[c0], sa1 = H.statusC[c1], sb0 = H.bstatusC[c0], sb1 = H.bstatusC[c1];
        const double lp0 = H.priorC[w], lp1 = H.priorC[size_t(nwk) + w];
        const KDbl G0 = H.geoC + c0 * LFG_NGEO;
        const KDbl G1 = H.geoC + c1 * LFG_NGEO;
        const double rp0 = G0[G_RPRIOR] + G0[G_RPRIOR_BS], rp1 = G1[G_RPRIOR] + G1[G_RPRIOR_BS];
        const double ph0 = G0[G_PHI0], ph1 = G1[G_PHI0];
        const int jw = int(__umulhi(draw(H.jseed, H.jstep, H.jhalf, 0, H.jlo + w).z, unsigned(H.jns)));
        PAIR_STAMP(21, tid == 0 && jw != -7);
        if (FOLD)  // the partner's pending verdict: accepted unless NaN
            cand = __builtin_amdgcn_readfirstlane(int(!isnan(H.fv[__builtin_amdgcn_readfirstlane(jw)])));
        else
            cand = __builtin_amdgcn_readfirstlane(H.accflag[__builtin_amdgcn_readfirstlane(jw)]);
        PAIR_STAMP(10, tid == 0 && cand >= 0);
        G = (const double*)(cand ? G1 : G0);
        st0 = cand ? sa1 : sa0;
        bst = cand ? sb1 : sb0;
        lpr = cand ? lp1 : lp0;
        rpr = cand ? rp1 : rp0;
        phi0 = cand ? ph1 : ph0;
    } else {
        G = (const double*)(H.geo + size_t(pair) * LFG_NGEO);
        st0 = H.status[pair];
        bst = H.bstatus[pair];
        if (H.prior) lpr = H.prior[w];
        rpr = G[G_RPRIOR] + G[G_RPRIOR_BS];
        phi0 = G[G_PHI0];
    }
    // the record through the constant address space: its reads are scalar
    // loads into SGPRs, as in k_elements (the launch writes no record it
    // reads: the standard slot it copies into is not G when X.jk is set)
    const CGeo Gc = (CGeo)(G);
    const int stp = (st0 != ST_OK) ? st0 : bst;  // MODEL_SPEC 6 order: setup failures first
    const bool prej = H.prior && !(lpr + rpr > -INFINITY);  // prior_rejects
    const int st = (stp == ST_OK && prej) ? -1 : stp;  // -1: prior-rejected, straight to the -inf finish
    const bool acc1 = L.pos && E == 1;
    // this thread's point (one tile: m = n points): window and phase into LDS,
    // its sortedness against the predecessor, and the cells it fills of the
    // two phase indices (windows' lo, point phases), formed from its own and
    // its predecessor's windows, so that no barrier separates them
    int fl = 0;
    if (own) {
        double ph, lo, hi, hw;
        pair_window(xw_own, ww_own, phi0, ph, lo, hi, hw);
        PAIR_STAMP(11, tid == 0 && ph != 12345.0);
        TA.lo[tid] = lo;
        TA.hi[tid] = hi;
        TA.iw[tid] = 1.0 / (2.0 * hw);
        sph[tid] = ph;
        double php = 0.0, lop = 0.0, hip = 0.0, hwp, ph0, lo0, hi0, hw0, ph1, lo1, hi1, hw1;
        if (tid) pair_window(xw_prv, ww_prv, phi0, php, lop, hip, hwp);
        pair_window(xw_0, ww_0, phi0, ph0, lo0, hi0, hw0);
        pair_window(xw_1, ww_1, phi0, ph1, lo1, hi1, hw1);
        fl = (hw >= 0.0) ? 0 : 4;  // negative or NaN widths: point-major
        if (tid && (lo < lop || hi < hip || ph < php)) fl = 4;
        pair_cells(TA.cell, tid, m, lop, lo, lo0, lo1);
        pair_cells(SU.s.scp, tid, m, php, ph, ph0, ph1);
    }
    {
        const int wf = wave_or4(fl);
        if (lane == 0) sflagw[wv] = wf;
    }
    if constexpr (LONG) {  // the tables' counters and sums; the record for sub_point's LDS reads
        for (int i = tid; i < 2 * LONG_FC; i += nt) (&LT.fend[0][0])[i] = 0;
        if (tid < TCELLS) {
            LST.dpre[tid][0] = LST.dpre[tid][1] = LST.dpre[tid][2] = 0;
            LST.spre[tid] = 0;
            LST.dend[tid] = LST.send[tid] = 0;
        } else if (tid < TCELLS + 3) {
            LST.dv0[tid - TCELLS] = 0;
        } else if (tid >= nt - LFG_NGEO) {
            LT.sgeo[tid - (nt - LFG_NGEO)] = G[tid - (nt - LFG_NGEO)];
        }
    } else {
#if LFG_PAIR_RUNSCAN
        // the sinks add at indices < m only (apply_runs_batched and
        // apply_runs_merged, donor, flush)
        // and run_scan reads [0, m): the slots above m stay as they are, and
        // a wave wholly above m stores nothing
        if (tid <= m) {
            for (int i = 0; i < 6; ++i) sacc[i][tid] = 0ull;
            SU.s.X[0][tid] = 0ull;
            SU.s.X[1][tid] = 0ull;
        }
#else
        for (int i = 0; i < 6; ++i) sacc[i][tid] = 0ull;
        SU.s.X[0][tid] = 0ull;
        SU.s.X[1][tid] = 0ull;
#endif
    }
    if (tid == 0) {
#if !LFG_PAIR_RUNSCAN  // (no sink adds at slot nt and no scan reads it)
        if constexpr (!LONG) {
            for (int i = 0; i < 6; ++i) sacc[i][nt] = 0ull;
            SU.s.X[0][nt] = 0ull;
            SU.s.X[1][nt] = 0ull;
        }
#endif
        stot[0] = stot[1] = 0ull;
        sjob = (X.nspec > 0 && pair < 2 * A.nbc) ? 8 : 9;
    }
    PAIR_STAMP(19, tid == 0);
    // the disc ring weights (MODEL_SPEC 5.2): wave 7's lanes 0..NDISC_R
#if LFG_PAIR_SINK_MERGE
    if (st == ST_OK && wv == 7 && lane <= NDISC_R) ring_weight_lane<!LONG>(lane, Gc, swt);
    // the sinks' constants, once per pair and not once per wave: phase_index's
    // and itwd's expressions on the first and last windows, which every
    // thread holds (lane 0: itwd; 1: the windows' lo; 2: the point phases;
    // one IEEE quotient for the three).  Wave 6: wave 7's prologue is the
    // longest (the ring weights' pow), and B0 waits for it
    if (!LONG && st == ST_OK && m > 0 && wv == 6 && lane < 3) {
        double ph0, lo0, hi0, hw0, ph1, lo1, hi1, hw1;
        pair_window(xw_0, ww_0, phi0, ph0, lo0, hi0, hw0);
        pair_window(xw_1, ww_1, phi0, ph1, lo1, hi1, hw1);
        const double ulk = Gc[G_ULIMB];
        const double v0 = lane == 1 ? lo0 : ph0, span = (lane == 1 ? lo1 : ph1) - v0;
        const double num = lane ? double(LIKE_NC) : 1.0;
        const double den = lane ? span : TWO_PI * ((1.0 - ulk) * 0.5 + ulk / 3.0);
        const double quo = num / den;
        if (lane == 0) skc[0] = quo;
        else {
            skc[2 * lane - 1] = v0;
            skc[2 * lane] = span > 0.0 ? quo : 0.0;
        }
    }
#else
    if (st == ST_OK && wv == 7 && lane <= NDISC_R) ring_weight_lane(lane, Gc, swt);
#endif
    __syncthreads();  // B0: windows, cells, flags, zeroed sums, ring weights, sjob
    PAIR_STAMP(16, tid == 0);

    bool dir = LONG;  // LONG: the point-major sinks always
    if (!LONG)
        for (int k = 0; k < nw; ++k) dir = dir || sflagw[k] != 0;
    // this thread's data point (read after the phase barrier), the GP
    // filter's transition factor of the point (k_gp_like)
    if (own) {
        sy[tid] = L.y[o0 + tid];
        if (!GP) sye[tid] = L.ye[o0 + tid];
        if (GP) {
            const double xp = L.x[o0 + tid], dx = xp - (tid ? L.x[o0 + tid - 1] : xp);
            L.gpx[size_t(pair) * L.N + tid] = exp(-(Gc[G_GP_LAM] * dx));
        }
    }
    // GP: the changepoint distance is solved in this launch (the cache rule
    // tripped, G_GP_OK = 2); wave 0 then owns the slot's G_GP_DCP / G_GP_OK
    const bool pend = GP && st == ST_OK && Gc[G_GP_OK] == 2.0;
    // FOLD: rows w, w + nwk, ... of each half (wave 7's lanes): the snapshot
    // of this half's (final in this launch) for the next launch's speculative
    // lanes, and the pending verdicts of the partner half's, an accepted row
    // becoming its proposal (k_accept_regen's arithmetic)
    auto fold_rows = [&](int l) {
        const int ns = A.jns, h = L.half, hp = 1 - h, nd = L.ndim, r = (ns + nwk - 1) / nwk;
        for (int f = l; f < r * nd; f += 64) {
            const int k = f / nd, d = f - k * nd, j = w + k * nwk;
            if (j < ns) A.fsnap[size_t(j) * nd + d] = A.fpos[(size_t(h) * ns + j) * nd + d];
        }
        if (A.fv) {
            for (int f = l; f < r * nd; f += 64) {
                const int k = f / nd, d = f - k * nd, j = w + k * nwk;
                if (j >= ns) continue;
                const double v = A.fv[j];
                const uint4 rr = draw(L.seed, A.fstep, hp, 0, j);
                if (isnan(v)) continue;
                const double zr = (A.fa - 1.0) * u53(rr.x, rr.y) + 1.0, z = zr * zr / A.fa;
                const double* cj = A.fpos + (size_t(h) * ns + int(__umulhi(rr.z, unsigned(ns)))) * nd;
                double* row = A.fpos + (size_t(hp) * ns + j) * nd;
                row[d] = fma(row[d] - cj[d], z, cj[d]);
                if (d == 0) {
                    A.flnp[size_t(hp) * ns + j] = v;
                    if (A.fnacc) A.fnacc[size_t(hp) * ns + j] += 1;
                }
            }
        }
    };
    if (wv == 7) {
        // housekeeping off the prologue's critical path: the selected candidate
        // into the standard slots (API readers, k_combine_walkers, k_gp_like),
        // the pair status, the snapshot of the other half's rows for the next
        // launch's speculative lanes, the fused acceptance's prefetch
        const int l = lane;
        if (X.jk) {
            const size_t cw = size_t(cand) * nwk + w;
            double* Gd = const_cast<double*>(L.geo) + size_t(pair) * LFG_NGEO;
            // (a pending changepoint's two words are wave 0's: one writer each)
            if (l < LFG_NGEO && !(pend && (l == G_GP_DCP || l == G_GP_OK))) Gd[l] = G[l];
            if (l == 48) X.bstatus[pair] = bst;
            if (e == 0) {
                const double* qc = X.qC + cw * X.ndim;
                for (int d = l; d < X.ndim; d += 64) X.q[size_t(w) * X.ndim + d] = qc[d];
                if (l == 49) X.prior[w] = lpr;
                if (l == 50) X.zf[w] = X.zfC[cw];
            }
        }
        if (l == 51) const_cast<int*>(L.status)[pair] = stp;
        if (A.snap_dst && e == 0)
            for (int d = l; d < L.ndim; d += 64) A.snap_dst[size_t(w) * L.ndim + d] = A.snap_src[size_t(w) * L.ndim + d];
        if (FOLD) {
            fold_rows(l);
            if (l == 63) {  // the verdict's draw, zf and old ln_prob
                const int ns = A.jns, h = L.half;
                const uint4 r1 = draw(L.seed, L.step, h, 1, A.jlo + w);
                sacc1[0] = log(u53(r1.x, r1.y));
                sacc1[1] = X.jk ? X.zfC[size_t(cand) * nwk + w] : L.zfac[w];
                sacc1[2] = A.flnp[size_t(h) * ns + A.jlo + w];
            }
        }
        if (acc1) {
            const double* qsrc = X.jk ? X.qC + (size_t(cand) * nwk + w) * X.ndim : L.qprop + size_t(w) * L.ndim;
            for (int d = l; d < L.ndim && d < ACC_LDS; d += 64) sq[d] = qsrc[d];
            if (l == 63) {
                const uint4 r = draw(L.seed, L.step, L.half, 1, pair);
                sacc1[0] = log(u53(r.x, r.y));
                sacc1[1] = X.jk ? X.zfC[size_t(cand) * nwk + w] : L.zfac[w];
                sacc1[2] = L.lnp_ens[L.half * npairs + pair];
            }
        }
    }
    // ---- element phase: 16 jobs.  Job 0: this block's speculative setup
    // lanes of the next half; jobs 1..15: the 15 item chunks, longest first
    // (kJobChunk).  Wave w takes job w, then grabs the next free job from
    // sjob, at most twice (8 waves x 3 >= 16): the waves finish together
    // whatever the pair's Newton counts (a static two-chunk split waited
    // ~8 us at the phase barrier on its slowest wave)
    // the speculative lanes fill whole waves: wave 0 of the first 2 nbc blocks
    // (a few lanes in every block's wave 0 cost each of them the lanes' whole
    // instruction stream: SIMD issue slots of ~10x the work)
    const bool specblk = X.nspec > 0 && pair < 2 * A.nbc;
    if (wv == 0 && specblk) {
        PAIR_PRIO(3);
        if (lane < A.spl) {
            // candidate uniform per block: X.S[c] stays in scalar registers
            const int c = pair < A.nbc ? 0 : 1;
            const int t = (pair - c * A.nbc) * A.spl + lane;
            if (t < X.nspec) {  // the SetupArgs loaded here, not at the kernel's entry (opaque_kernargs)
                const SetupArgs Sc = kernarg_copy(&opaque_kernargs<PairArgs>()->X.S[__builtin_amdgcn_readfirstlane(c)]);
                setup_any<FOLD>(Sc, t);
            }
#ifdef LFG_PROFILE_PAIR
            if (lane == 0 && blockIdx.x < 4096) {
                const int np = X.S[0].W * X.S[0].E;
                g_pair_t[17][blockIdx.x] = t >= X.nspec ? 9 : (t < np ? 0 : (t < np + X.S[0].W ? 1 : 2));
            }
#endif
        }
    }
    __shared__ double sdcp;
    if (GP) {
        // the changepoint distance: the cache's, or (cache rule tripped,
        // G_GP_OK = 2) dist_cp = (dphi + phi4 - phi3) / 2 from ten limb
        // points' egress phases (CVModel.py:561-570; k_gp_dcp's solve)
        if (pend && wv == 0 && lane >= 32 && lane < 32 + DCP_LANES) {
            const int k = lane - 32;
            bool ok = Gc[G_GP_RWD] > 0.0;
            double b = NAN;
            if (ok && k < DCP_NTHETA) {
                const Roche R{Gc[G_Q], Gc[G_CA], Gc[G_CB], Gc[G_MU], Gc[G_XL1], Gc[G_PL1], Gc[G_RS], Gc[G_RS2]};
                const double s = Gc[G_S], c = Gc[G_C], r1 = Gc[G_GP_RWD];
                double dphi_c;
                if (findphi_fast(R, Gc[G_INC], dphi_c) == ST_OK) {
                    double sth, cth, sp, cp, a;
                    sincos(PI * dphi_c, &sth, &cth);
                    sincos(TWO_PI * k / DCP_NTHETA, &sp, &cp);
                    if (!element_interval(R, r1 * (cp * sth - sp * c * cth), r1 * (cp * cth + sp * c * sth),
                                          r1 * (sp * s), s, c, eggleton(R.q), a, b))
                        b = NAN;
                }
            }
            double lo = isnan(b) ? INFINITY : b, hi = isnan(b) ? -INFINITY : b;
            for (int off = DCP_LANES / 2; off > 0; off >>= 1) {
                lo = fmin(lo, __shfl_xor(lo, off, DCP_LANES));
                hi = fmax(hi, __shfl_xor(hi, off, DCP_LANES));
            }
            if (k == 0) {
                ok = ok && lo <= hi;  // no eclipsed limb point: wdphases fails
                const double d = ok ? (Gc[G_GP_DPHI] + (hi - lo)) / 2.0 : NAN;
                double* Gd = const_cast<double*>(L.geo) + size_t(pair) * LFG_NGEO;  // the standard slot
                Gd[G_GP_DCP] = d;
                Gd[G_GP_OK] = ok ? 1.0 : 0.0;
                sdcp = d;
            }
        } else if (!pend && tid == 0) {
            sdcp = Gc[G_GP_DCP];
        }
    }
    if (st == ST_OK && m > 0) {
        const double ul = Gc[G_ULIMB];
#if LFG_PAIR_SINK_MERGE
        const double itwd = LONG ? 1.0 / (TWO_PI * ((1.0 - ul) * 0.5 + ul / 3.0)) : skc[0];
#else
        const double itwd = 1.0 / (TWO_PI * ((1.0 - ul) * 0.5 + ul / 3.0));
#endif
        auto make_sink = [&]() {
            if constexpr (LONG)  // the point-major sinks only (no tile arrays in this instantiation)
                return PairSink{true, lane, PhaseIndex{}, PhaseIndex{}, nullptr, nullptr, nullptr, nullptr, stot, swt,
                                ul, itwd, Gc[G_S], Gc[G_C], Lab, sab, sbw, sdq};
#if LFG_PAIR_SINK_MERGE
            else
                return PairSink{dir, lane, PhaseIndex{TA.lo, TA.cell, m, skc[1], skc[2]},
                                PhaseIndex{sph, SU.s.scp, m, skc[3], skc[4]}, TA.hi,
                                TA.iw, sacc, SU.s.X, stot, swt, ul, itwd, Gc[G_S], Gc[G_C], SU.ab, sab, sbw, sdq};
#else
            else
                return PairSink{dir, lane, phase_index(TA.lo, TA.cell, m), phase_index(sph, SU.s.scp, m), TA.hi,
                                TA.iw, sacc, SU.s.X, stot, swt, ul, itwd, Gc[G_S], Gc[G_C], SU.ab, sab, sbw, sdq};
#endif
        };
        PairSink K = make_sink();
        // chunk c: items v = 64 c + lane of one region each (c < 11: WD and
        // disc; 11, 12: spot; 13, 14: donor), so that no wave runs two
        // regions' code one after the other
        auto chunk = [&](int j) {
            const int c = kJobChunk[j - 1];
            constexpr int V_BS = U_WD + U_DISC, V_DON = V_BS + U_BS;
            const int r0 = c < 11 ? 0 : (c < 13 ? V_BS : V_DON), c0 = c < 11 ? 0 : (c < 13 ? 11 : 13);
            const int r1 = c < 11 ? V_BS : (c < 13 ? V_DON : NUNIQ);
            const int v = r0 + (c - c0) * 64 + lane < r1 ? r0 + (c - c0) * 64 + lane : -1;
#ifdef LFG_PROFILE_PAIR
            const bool rec = lane == 0 && blockIdx.x < 4096;
            if (rec) g_pair_j[0][c][blockIdx.x] = __builtin_amdgcn_s_memrealtime();
            K.mk = rec ? &g_pair_j[1][c][blockIdx.x] : nullptr;
#endif
            if (v >= 0) element_item_to(v, Gc, K);
#ifdef LFG_PROFILE_PAIR
            if (rec) g_pair_j[2][c][blockIdx.x] = __builtin_amdgcn_s_memrealtime();
#endif
        };
        auto grab = [&]() {
            int j = 0;
            if (lane == 0) j = atomicAdd(&sjob, 1);
            return __builtin_amdgcn_readfirstlane(j);  // every lane is active: the first is lane 0
        };
        // straight-line calls, not a loop: a loop's invariant constants (the
        // transcendental polynomials) were hoisted and spilled to scratch
        // (a block without speculative lanes starts wave w on job w + 1)
        // wave priority falls with each job a wave starts, so that the two
        // workgroups of a CU advance together (the issue arbiter otherwise
        // favours the older workgroup's waves)
#ifndef LFG_ABL_ELEM  // (diagnostic builds) no element jobs: the prologue, setup lanes and likelihood alone
        PAIR_PRIO(3);
        if (!specblk) chunk(wv + 1);
        else if (wv > 0) chunk(wv);
        int j = grab();
        PAIR_PRIO(2);
        if (j < 16) chunk(j);
        j = grab();
        PAIR_PRIO(1);
        if (j < 16) chunk(j);
        PAIR_PRIO(0);
#else
        (void)chunk;
        (void)grab;
#endif
        K.flush();
    }
    static_assert(11 * 64 >= U_WD + U_DISC && 10 * 64 < U_WD + U_DISC, "11 chunks of WD/disc");
    static_assert(U_BS > 64 && U_BS <= 128 && U_DON > 64 && U_DON <= 128, "two spot and two donor chunks");
    PAIR_STAMP(1 + wv, lane == 0);
    __syncthreads();  // B1: the sums (or the tables)
    PAIR_STAMP(9, tid == 0);

    if (st != ST_OK) {
        if (GP) return;  // k_gp_like sees the status (or the prior) and finishes the pair
        if (FOLD) {  // ln_prob -inf (combine_walker's value): rejected unless the old one is -inf too
            if (tid == 0) {
                L.lle[pair] = -INFINITY;
                if (L.lnp) L.lnp[pair] = -INFINITY;
                const double v = -INFINITY;
                A.vout[pair] = (sacc1[0] < sacc1[1] + v - sacc1[2]) ? v : NAN;
            }
            return;
        }
        if (tid == 0) L.lle[pair] = -INFINITY;
        finish_walker(L, pair, tid, acc1, sq, sacc1, sflag);
        return;
    }
    // ---- each point's flux and chi^2 (GP: residual, changepoint block)
    double chi = 0.0;
#ifdef LFG_ABL_LIKE  // (diagnostic builds) no likelihood phase: chi^2 = 0
    if (false) {
    } else
#endif
    if constexpr (LONG) {
        // the pair's tables, then this wave's range of the points (lanes interleaved)
        const double ul = Gc[G_ULIMB];
        long_tables(LT, LST, LSE, Lab, sab, sbw, sdq, swt, stot, ul, 1.0 / (TWO_PI * ((1.0 - ul) * 0.5 + ul / 3.0)),
                    lspart, tid);
        PAIR_STAMP(12, tid == 0);
        const int S = L.nsub;
        const double* xe = L.x + o0;
        const double* we = L.w ? L.w + o0 : nullptr;
        const double* ye = L.y + o0;
        const double* ee = L.ye + o0;
        const double fwd = Gc[G_WDF], fds = Gc[G_DF], fsp = Gc[G_SF], frs = Gc[G_RSF];
#ifdef LFG_PROFILE_PAIR
        unsigned long long tl_wd = 0, tl_sub = 0;
        int lctr[3] = {0, 0, 0};
#endif
        SubCur SC{INFINITY, INFINITY, INFINITY, {0, 0, 0}, LongV(0), LongV(0), LongV(0), 0, 0, 0
        };
        const LongU KU = long_uniforms(LT, LST, S);
        const double fspS = uni(fsp / S), frsS = uni(frs / S);
        // each wave a contiguous range of the points, its lanes interleaved
        // (a thread's points follow one another 64 apart, and its donor
        // cursor walks on from point to point).  A dynamic queue of 4-point
        // chunks balanced the eclipse's points over the waves but doubled the
        // total (every chunk starts with fresh lookups; and its chi^2 order
        // was not fixed)
        // The runs are cut where the running estimated cost (long_weight, in
        // index order) passes equal shares: a thread in the eclipse takes
        // fewer points, and the waves end together (the eclipse's waves took
        // 2-3 times the others' time with equal counts)
        // The points in blocks of 64 (one step of a wave's loop): each block's
        // estimated cost (long_weight, one coalesced pass, a wave per block),
        // their prefix, and each wave takes the blocks where the running cost
        // passes its eighth of the total; its lanes interleaved, so every step
        // reads 64 consecutive points and the lanes of a wave stand at
        // neighbouring phases (the same branches of the lookups)
        constexpr int LAB_INTS = int(NU_WDD * sizeof(double2) / sizeof(int));  // the spent interval table, as ints
        int p0, p1;
        {
            constexpr int nw = LIKE_THREADS / 64;
            const int nch = (n + 63) >> 6;
            int* cw = reinterpret_cast<int*>(Lab);  // the WD/disc intervals are spent
            int b0, b1;
            if (nch + 1 <= LAB_INTS - 8 * 128) {  // (the point phase's queues take the last 8 x 128 ints)
                for (int c = wv; c < nch; c += nw) {
                    const int p = c * 64 + lane;
                    int wt = p < n ? long_weight(KU, xe[p] - phi0, we ? we[p] : 0.0) : 0;
                    for (int off = 32; off > 0; off >>= 1) wt += __shfl_xor(wt, off);
                    if (lane == 0) cw[c] = wt;
                }
                __syncthreads();
                if (wv == 0) {  // exclusive prefix over the blocks, in place; the total at nch
                    const int B = (nch + 63) >> 6, q0 = min(lane * B, nch), q1 = min(q0 + B, nch);
                    long long own = 0;
                    for (int c = q0; c < q1; ++c) own += cw[c];
                    long long run = wave_scan_incl(own, lane) - own;
                    for (int c = q0; c < q1; ++c) {
                        const int v = cw[c];
                        cw[c] = int(run);
                        run += v;
                    }
                    if (lane == 63) cw[nch] = int(run);
                }
                __syncthreads();
                const long long T = cw[nch];
                auto first = [&](int w) {  // the first block whose cost before it reaches w / nw of the total
                    const long long tgt = (T * w) / nw;
                    int a = 0, b = nch;
                    while (a < b) {
                        const int mid = (a + b) >> 1;
                        if (cw[mid] >= tgt) b = mid;
                        else a = mid + 1;
                    }
                    return a;
                };
                b0 = wv ? first(wv) : 0;
                b1 = wv + 1 < nw ? first(wv + 1) : nch;
            } else {  // more blocks than the spent LDS holds: equal shares
                b0 = nch * wv / nw;
                b1 = nch * (wv + 1) / nw;
            }
            p0 = __builtin_amdgcn_readfirstlane(b0) * 64 + lane;
            p1 = min(__builtin_amdgcn_readfirstlane(b1) * 64, n);
        }
        // Pass 1 over the wave's points (steps of 64, lanes interleaved): the
        // WD/disc windows, and the sub-bin sums in closed form where the point
        // is quiet (sub_point_quiet).  The other points go to the wave's queue
        // (a ring of LQ_CAP indices in the spent interval table, in index
        // order); each time it holds 64 they run sub_point_c with every lane
        // busy (pass 2), and the rest after the last step.  Every point's
        // chi^2 term is added once, by the lane that finishes it.
        constexpr int LQ_CAP = 128;
        int* const lq = reinterpret_cast<int*>(Lab) + (LAB_INTS - 8 * LQ_CAP) + wv * LQ_CAP;
        const LongB KB = long_beam_zeros(KU);
        int qhead = 0, qtail = 0;  // uniform over the wave
        auto full_point = [&](int p) {  // sub_point_c's path for point p
            const double xp = xe[p], wp = we ? we[p] : 0.0, yp = ye[p], ep = ee[p];
            const double wk = wp < 0.0 ? 0.0 : wp;  // MODEL_SPEC 3 (NaN stays NaN)
            const double ph0 = xp - phi0, phc = wrap_phase(ph0);
            const double2 f2 = long_wd_disc(LT, KU, phc, wk);
            const double2 r2 = sub_point_c(LST, LSE, sab, sbw, sdq, KU, ph0, wk, S, SC);
            const double f = isnan(wk) ? NAN : fwd * (1.0 - f2.x) + fds * (1.0 - f2.y) + fspS * r2.x + frsS * r2.y;
            const double rr = (yp - f) / ep;
            chi += isnan(f) ? INFINITY : rr * rr;
        };
        auto run_queue = [&](int cnt) {  // pass 2: cnt <= 64 queued points, one per lane
            if (lane < cnt) full_point(lq[(qhead + lane) & (LQ_CAP - 1)]);
            qhead += cnt;
            // the queued points lie behind pass 1 (the cursor's fresh lookup
            // took them), and walking the cursor back up from there re-crossed
            // every entry in between: pass 1's next point looks afresh (one cell)
            SC.ph = INFINITY;
        };
        const int pw0 = p0 - lane;  // the wave's first point (uniform)
        // the next step's phase and width, in flight during this one
        double xn = p0 < p1 ? xe[p0] : 0.0, wn = (p0 < p1 && we) ? we[p0] : 0.0;
        for (int base = pw0; base < p1; base += 64) {
            const int p = base + lane;
            bool defer = false;
            if (p < p1) {
#ifdef LFG_ABL_GLOAD  // (diagnostic builds) no global loads in the point loop: a synthetic grid
                const double xp = -0.3 + p * 6.0006e-5, wp = 3.0003e-5, yp = 1.0, ep = 0.004;
                (void)xn; (void)wn;
#else
                const double xp = xn, wp = wn, yp = ye[p], ep = ee[p];
                if (p + 64 < p1) {
                    xn = xe[p + 64];
                    wn = we ? we[p + 64] : 0.0;
                }
#endif
                const double wk = wp < 0.0 ? 0.0 : wp;  // MODEL_SPEC 3 (NaN stays NaN)
                const double ph0 = xp - phi0, phc = wrap_phase(ph0);
                double2 r2;
#ifdef LFG_ABL_LSUB
                r2 = make_double2(phc * 1e-30, wk * 1e-30);
                const bool quiet = true;
#else
                const bool quiet = sub_point_quiet(LST, LSE, sbw, sdq, KU, KB, ph0, wk, S, SC, r2);
#endif
                if (quiet) {
#ifdef LFG_ABL_LWD
                    const double2 f2 = make_double2(phc * 1e-30, wk * 1e-30);
#else
                    const double2 f2 = long_wd_disc(LT, KU, phc, wk);
#endif
                    // k_lnlike's sum, term for term (MODEL_SPEC 3: a NaN width, a NaN flux)
                    const double f = fwd * (1.0 - f2.x) + fds * (1.0 - f2.y) + fspS * r2.x + frsS * r2.y;
                    const double rr = (yp - f) / ep;
                    chi += isnan(f) ? INFINITY : rr * rr;
                } else {
                    defer = true;
                }
            }
            const unsigned long long m = __ballot(defer);
            if (defer)
                lq[(qtail + __builtin_amdgcn_mbcnt_hi(unsigned(m >> 32), __builtin_amdgcn_mbcnt_lo(unsigned(m), 0u))) &
                   (LQ_CAP - 1)] = p;
            qtail += __popcll(m);
#ifdef LFG_PROFILE_PAIR  // (diagnostic builds) the block's quiet and queued points
            const unsigned long long mact = __ballot(p < p1);
            if (lane == 0 && blockIdx.x < 4096) {
                atomicAdd(&g_pair_t[22][blockIdx.x], (unsigned long long)__popcll(mact & ~m));
                atomicAdd(&g_pair_t[23][blockIdx.x], (unsigned long long)__popcll(m));
            }
#endif
            if (qtail - qhead >= 64) run_queue(64);
        }
        if (qtail > qhead) run_queue(qtail - qhead);
        PAIR_WSTAMP(0);  // (diagnostic builds) this wave's points done
#ifdef LFG_PROFILE_PAIR
        {
            unsigned long long a = tl_wd, b = tl_sub;
            for (int off = 32; off > 0; off >>= 1) {
                a = max(a, (unsigned long long)__shfl_xor((long long)a, off));
                b = max(b, (unsigned long long)__shfl_xor((long long)b, off));
            }
            if (lane == 0 && blockIdx.x < 4096) { g_pair_w[1][wv][blockIdx.x] = a; g_pair_w[2][wv][blockIdx.x] = b; }
            // walk steps / window entries / windows in a hull: the wave's max lane (16 bits each)
            int c0 = lctr[0], c1 = lctr[1], c2 = lctr[2];
            for (int off = 32; off > 0; off >>= 1) {
                c0 = max(c0, __shfl_xor(c0, off));
                c1 = max(c1, __shfl_xor(c1, off));
                c2 = max(c2, __shfl_xor(c2, off));
            }
            if (lane == 0 && blockIdx.x < 4096)
                g_pair_w[3][wv][blockIdx.x] = (unsigned long long)(c0 & 0xffff) | ((unsigned long long)(c1 & 0xffff) << 16) |
                                              ((unsigned long long)(c2 & 0xffff) << 32);
        }
#endif
    } else if (m > 0) {
        const double s = Gc[G_S], c = Gc[G_C], ul = Gc[G_ULIMB];
        const double twd = TWO_PI * ((1.0 - ul) * 0.5 + ul / 3.0);  // 2 pi [F(1) - F(0)]
        const double wspot = double(static_cast<long long>(stot[0])) * (FX_INV / PAIR_SPOT_S);
        const double dn = double(static_cast<long long>(stot[1])) * (FX_INV / PAIR_DON_S);
        const double phc = own ? sph[tid] : 0.0;
        double fw = 0.0, fd = 0.0, eb = 0.0, R3 = 0.0, R4 = 0.0, R5 = 0.0;
#if LFG_PAIR_RUNSCAN
        // A wave whose first thread is past the last point (wave-uniform)
        // does nothing from here on except reach the barriers; its chi^2 is 0.
        // BARRIER INVARIANT: no __syncthreads() may sit inside an if (pw)
        // branch.  Every wave of the workgroup reaches every barrier on every
        // path after B1: st != ST_OK (finish_walker's, all threads call it),
        // the scan's barrier below (dir and m are uniform over the workgroup),
        // GP's return, the chi^2 barrier, and acc1's.  A skipped barrier hangs
        // the workgroup.
        const bool pw = wv * 64 < m;
        // the terms that depend on no sum, ahead of the scan's barrier: their
        // FP64 latency overlaps the scanning waves
        double e0 = 0.0, e1 = 0.0, beam = 0.0;
        if (pw) {
            const double2 scp2 = sincospi_ool(2.0 * phc);
            e0 = s * scp2.y;
            e1 = -s * scp2.x;
            const double bden = Gc[G_BDEN], fis = Gc[G_FIS];
            if (bden > 0.0) beam = (fis + (1.0 - fis) * fmax(Gc[G_NB0] * e0 + Gc[G_NB1] * e1 + Gc[G_NB2] * c, 0.0)) / bden;
        }
        if (dir) {
            if (own) {
                const double wk = L.w ? L.w[o0 + tid] : 0.0;
                const double2 f2 = pair_direct_wd_disc(SU.ab, ul, swt, phc, wk, twd, swt[NDISC_R]);
                // MODEL_SPEC 3: a NaN width gives a NaN flux (such a tile is
                // always point-major: its window fails the sortedness test)
                fw = isnan(wk) ? NAN : f2.x;
                fd = f2.y;
                eb = direct_spot(sab, sbw, phc, wk, 1.0 / wspot);
            }
        } else {
            // wave i < 6 scans difference array i in place (arrays 0 and 1
            // with their second copies); after the barrier (the one block_scan
            // has between its stages) a point's six prefixes are LDS reads
            if (wv < 6) run_scan(sacc[wv], wv < 2 ? SU.s.X[wv] : nullptr, m, lane);
            __syncthreads();  // every wave, on every path through this branch
            PAIR_STAMP(12, tid == 0);
            if (own) {
                fw = double(static_cast<long long>(sacc[0][tid])) * FX_INV;
                fd = double(static_cast<long long>(sacc[1][tid])) * FX_INV;
                eb = double(static_cast<long long>(sacc[2][tid])) * (FX_INV / PAIR_SPOT_S) / wspot;
                R3 = double(static_cast<long long>(sacc[3][tid]));
                R4 = double(static_cast<long long>(sacc[4][tid]));
                R5 = double(static_cast<long long>(sacc[5][tid]));
            }
        }
        if (pw) {
            double D = 0.0;
            if (!dir) D = (e0 * R3 + e1 * R4 + c * R5) * (FX_INV / PAIR_DON_S);
            else if (own) D = direct_donor(sdq, e0, e1, c);
            const double sbs = beam * (1.0 - eb), srs = D / dn;
            if (own) {
                const double f = Gc[G_WDF] * (1.0 - fw) + Gc[G_DF] * (1.0 - fd) + Gc[G_SF] * sbs + Gc[G_RSF] * srs;
                if (GP) {
                    const size_t q = size_t(pair) * L.N + tid;
                    L.res[q] = sy[tid] - f;
                    L.gpb[q] = gp_block(L.x[o0 + tid], L.gp_ecl[2 * e], L.gp_ecl[2 * e + 1], sdcp, Gc[G_PHI0]);
                } else {
                    const double rr = (sy[tid] - f) / sye[tid];
                    chi = isnan(f) ? INFINITY : rr * rr;
                }
            }
        }
#else
        if (dir) {
            if (own) {
                const double wk = L.w ? L.w[o0 + tid] : 0.0;
                const double2 f2 = pair_direct_wd_disc(SU.ab, ul, swt, phc, wk, twd, swt[NDISC_R]);
                // MODEL_SPEC 3: a NaN width gives a NaN flux (such a tile is
                // always point-major: its window fails the sortedness test)
                fw = isnan(wk) ? NAN : f2.x;
                fd = f2.y;
                eb = direct_spot(sab, sbw, phc, wk, 1.0 / wspot);
            }
        } else {
            long long r[6] = {0, 0, 0, 0, 0, 0};
            block_scan<6>(sacc, spart, tid, r, SU.s.X);
            PAIR_STAMP(12, tid == 0);
            fw = double(r[0]) * FX_INV;
            fd = double(r[1]) * FX_INV;
            eb = double(r[2]) * (FX_INV / PAIR_SPOT_S) / wspot;
            R3 = double(r[3]);
            R4 = double(r[4]);
            R5 = double(r[5]);
        }
        const double2 scp2 = sincospi_ool(2.0 * phc);
        const double e0 = s * scp2.y, e1 = -s * scp2.x;
        double D = 0.0;
        if (!dir) D = (e0 * R3 + e1 * R4 + c * R5) * (FX_INV / PAIR_DON_S);
        else if (own) D = direct_donor(sdq, e0, e1, c);
        double beam = 0.0;
        const double bden = Gc[G_BDEN], fis = Gc[G_FIS];
        if (bden > 0.0) beam = (fis + (1.0 - fis) * fmax(Gc[G_NB0] * e0 + Gc[G_NB1] * e1 + Gc[G_NB2] * c, 0.0)) / bden;
        const double sbs = beam * (1.0 - eb), srs = D / dn;
        if (own) {
            const double f = Gc[G_WDF] * (1.0 - fw) + Gc[G_DF] * (1.0 - fd) + Gc[G_SF] * sbs + Gc[G_RSF] * srs;
            if (GP) {
                const size_t q = size_t(pair) * L.N + tid;
                L.res[q] = sy[tid] - f;
                L.gpb[q] = gp_block(L.x[o0 + tid], L.gp_ecl[2 * e], L.gp_ecl[2 * e + 1], sdcp, Gc[G_PHI0]);
            } else {
                const double rr = (sy[tid] - f) / sye[tid];
                chi = isnan(f) ? INFINITY : rr * rr;
            }
        }
#endif  // LFG_PAIR_RUNSCAN
    }
    if (GP) return;  // k_gp_like forms ln_like from the residuals
#if LFG_PAIR_RUNSCAN
    if (LONG || wv * 64 < m) chi = wave_sum(chi);  // (a wave without a point holds chi = 0)
#else
    chi = wave_sum(chi);
#endif
    if (lane == 0) red[wv] = chi;
    __syncthreads();
    // the finish (finish_walker's arithmetic) from the values thread 0
    // holds: its ln_like, and the prior terms of the candidate it selected
    // (what the standard slots hold now), without a barrier and a global
    // round trip for each
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < nw; ++i) tot += red[i];
        const double lp = lpr + Gc[G_RPRIOR] + Gc[G_RPRIOR_BS];  // finish_walker's sum, term for term
        const double lle = isfinite(lp) ? -0.5 * tot : -INFINITY;
        L.lle[pair] = lle;
        PAIR_STAMP(13, true);
        if (FOLD) {  // this pair's verdict for the exchange (k_accept_regen's test)
            const double v = isfinite(lp) ? lp + lle : -INFINITY;
            if (L.lnp) L.lnp[pair] = v;
            A.vout[pair] = (sacc1[0] < sacc1[1] + v - sacc1[2]) ? v : NAN;
        } else if (!acc1) {
            combine_after(L, pair);
        } else {
            const int wg = L.half * L.npairs + pair;
            const double v = isfinite(lp) ? lp + lle : -INFINITY;
            if (L.lnp) L.lnp[pair] = v;
            const bool a = sacc1[0] < sacc1[1] + v - sacc1[2];
            if (a) {
                L.lnp_ens[wg] = v;
                if (L.naccept) L.naccept[wg] += 1;
            }
            sflag[0] = a ? 1 : 0;
            if (L.accflag) L.accflag[pair] = a ? 1 : 0;
        }
    }
    if (acc1) {
        __syncthreads();
        const int wg = L.half * L.npairs + pair;
        if (sflag[0] && tid < L.ndim)
            L.pos[size_t(wg) * L.ndim + tid] = (tid < ACC_LDS) ? sq[tid] : L.qprop[size_t(pair) * L.ndim + tid];
    }
    PAIR_STAMP(15, tid == 0);
}
