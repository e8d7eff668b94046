// lfg_k_pair_long.hpp -- k_pair's LONG part: LongTabs, long_find,
// long_window, long_point, long_wd_disc, the point phase's helpers and
// long_tables.  Needs before it: the first part of lfg_k_pair.hpp (the
// sinks) and lfg.hip's section k_lnlike (SubTables, SubEntries, sub_point).
// Included by lfg_k_pair.hpp, ahead of the kernel.
#pragma once

// ---- LONG: eclipses of any length and sub-binned exposures in k_pair ----
// The element phase stores every solved item (k_pair's point-major sinks:
// WD/disc intervals, spot intervals and weights, donor tiles) and the pair's
// breakpoints are then bucketed into per-pair tables in LDS, so that every
// point is evaluated on its own, with no tile loop, block scan or barrier per
// 512 points (config 5: 10 000 points x 5 sub-bins):
//  * WD and disc (one table each, the symmetry-unique elements; a mirror
//    element [-b, -a] is the unique one seen from -phase): the eclipsed
//    fraction of window [lo, hi] is the integral of the covering weight,
//      int_lo^hi C(t) dt = C(lo) (hi - lo) + sum_{lo <= pos < hi} q (hi - pos),
//    with q = +w at a start a_k and -w at an end b_k; each sorted entry holds
//    C just after it (int64 fixed point, exact), so C(lo) is one read once the
//    first entry at or above lo is found -- in its cell (1 024 per table over
//    the table's own hull, a few entries even where the WD contacts crowd);
//    a zero-width window takes the elements with a_k < ph < b_k;
//  * spot and donor at the sub-bins: the S > 1 breakpoint tables of k_lnlike
//    (SubTables, SubEntries, sub_point), built here from LDS.
// Each wave takes a range of blocks of 64 points, its lanes interleaved
// (MODEL_SPEC 3 for every width, order and wrap: no sortedness is assumed).
constexpr int NE_W = 2 * U_WD, NE_D = 2 * U_DISC;  // WD / disc table entries (two per unique element)
constexpr int LONG_FC = 4 * TCELLS;                 // cells per WD/disc table (the sub-bin tables: TCELLS)
struct LongTabs {
    int fend[2][LONG_FC];       // WD / disc cells: counts -> exclusive offsets -> (after the scatter) cell ends
    double epos[NE_W + NE_D];   // entries: WD [0, NE_W), disc after
    long long ecb[NE_W + NE_D];  // build: q; after the sort and scan: C just after the entry
    double t0[2], ginv[2], amin[2], bmax[2];  // per table: LONG_FC cells over its hull
    double snorm[4];            // sub_point's: 1 / spot total, 1 / donor |v| sum, donor norm, |v| sum
    double shull[4];            // [2], [3]: the spot hull (sub_point)
    double sgeo[LFG_NGEO];      // the record, for sub_point's LDS reads
    double part[8][LIKE_THREADS / 64];  // wave partials of the hulls and sums
};

// the WD/disc cell of x in table t (clamped to the table's cells)
__device__ __forceinline__ int long_cell(double x, double t0, double ginv)
{
    const double u = (x - t0) * ginv;
    return u <= 0.0 ? 0 : (u >= double(LONG_FC - 1) ? LONG_FC - 1 : int(u));
}

// a value the whole block holds alike, into scalar registers
__device__ __forceinline__ double uni(double x)
{
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readfirstlane(static_cast<int>(b));
    const int hi = __builtin_amdgcn_readfirstlane(static_cast<int>(b >> 32));
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}

// the point phase's per-pair constants, read once from LDS into scalar
// registers: every lane's lookups and sub-bin terms use them, and the LDS
// pipe -- which the lookups keep busy -- serves no broadcasts in the loop
struct LongU {
    double t0[2], gf[2], amin[2], bmax[2];  // WD/disc tables: cells and hulls
    int n[2];                               // entries per table
    double itb, ivs, dnorm, vsum, sa, sb;   // spot / donor norms, the spot hull
    double nbs0, nbs1, nbc, fis, omf;       // the record's terms of the sub-bin sums (MODEL_SPEC 6), folded
    double sg, cg, ibden, dsc;              // the sums' scales
    double invS;                            // 1 / sub-bins
    int nd, nsp;                            // donor / spot entries
};

__device__ __forceinline__ LongU long_uniforms(const LongTabs& W, const SubTables& T, int S)
{
    LongU K;
    K.invS = uni(1.0 / S);
    for (int t = 0; t < 2; ++t) {
        K.t0[t] = uni(W.t0[t]);
        K.gf[t] = uni(W.ginv[t]);
        K.amin[t] = uni(W.amin[t]);
        K.bmax[t] = uni(W.bmax[t]);
        K.n[t] = __builtin_amdgcn_readfirstlane(W.fend[t][LONG_FC - 1]);
    }
    K.itb = uni(W.snorm[0]); K.ivs = uni(W.snorm[1]); K.dnorm = uni(W.snorm[2]); K.vsum = uni(W.snorm[3]);
    K.sa = uni(W.shull[2]); K.sb = uni(W.shull[3]);
    const double sg = W.sgeo[G_S], cg = W.sgeo[G_C], fis = W.sgeo[G_FIS], bden = W.sgeo[G_BDEN];
    K.sg = uni(sg); K.cg = uni(cg); K.fis = uni(fis); K.omf = uni(1.0 - fis);
    K.nbs0 = uni(W.sgeo[G_NB0] * sg); K.nbs1 = uni(-W.sgeo[G_NB1] * sg); K.nbc = uni(W.sgeo[G_NB2] * cg);
    K.ibden = uni(bden > 0.0 ? 1.0 / bden : 0.0);
    K.dsc = uni(FX_INV * W.snorm[3] / W.snorm[2]);
    K.nd = __builtin_amdgcn_readfirstlane(T.dend[TCELLS - 1]);
    K.nsp = __builtin_amdgcn_readfirstlane(T.send[TCELLS - 1]);
    return K;
}

// the first entry of table t at or above x: the entries of the cells below
// x's all lie below it, those of the cells above all above (the cell index
// is monotone in position)
#ifdef LFG_PROFILE_PAIR
#define LONG_CNT(c, k) (c)[k]++
#else
#define LONG_CNT(c, k)
#endif
__device__ __forceinline__ int long_find(const LongTabs& W, const LongU& K, int t, double x, int* ctr = nullptr)
{
    const int f = long_cell(x, K.t0[t], K.gf[t]);
    const double* ep = W.epos + (t ? NE_W : 0);
    int i = f ? W.fend[t][f - 1] : 0;
    const int ie = W.fend[t][f];
    while (i < ie && ep[i] < x) {
        ++i;
        LONG_CNT(ctr, 0);
    }
    return i;
}

// eclipsed fraction of table t over window [lo, hi] (hi > lo): the integral
// of the covering weight over the window / its width (iw = FX_INV / (hi - lo))
__device__ __forceinline__ double long_window(const LongTabs& W, const LongU& K, int t, double lo, double hi,
                                              double iw, int* ctr = nullptr)
{
    if (!(hi > K.amin[t] && lo < K.bmax[t])) return 0.0;
    LONG_CNT(ctr, 2);
    const int base = t ? NE_W : 0, n = K.n[t];
    int i = long_find(W, K, t, lo, ctr);
    long long Cp = i ? W.ecb[base + i - 1] : 0;
    const long long C = Cp;
    double corr = 0.0;
    for (; i < n && W.epos[base + i] < hi; ++i) {
        const long long cb = W.ecb[base + i];
        corr = fma(double(cb - Cp), hi - W.epos[base + i], corr);
        Cp = cb;
        LONG_CNT(ctr, 1);
    }
    return fma(corr, iw, double(C) * FX_INV);
}

// table t at a point (zero-width window): the elements with a_k < ph < b_k
// (the starts below ph, the ends at or below it)
__device__ __forceinline__ double long_point(const LongTabs& W, const LongU& K, int t, double ph)
{
    if (!(ph > K.amin[t] && ph < K.bmax[t])) return 0.0;
    const int base = t ? NE_W : 0, n = K.n[t];
    int i = long_find(W, K, t, ph);
    long long Cp = i ? W.ecb[base + i - 1] : 0, C = Cp;
    for (; i < n && W.epos[base + i] == ph; ++i) {
        const long long cb = W.ecb[base + i];
        if (cb - Cp < 0) C += cb - Cp;
        Cp = cb;
    }
    return double(C) * FX_INV;
}

// WD and disc eclipsed fractions of a point's window (phase phc, half-width
// wk >= 0): the unique elements over [lo, hi] and, for their mirrors, over
// [-hi, -lo]
__device__ __forceinline__ double2 long_wd_disc(const LongTabs& W, const LongU& K, double phc, double wk,
                                               int* ctr = nullptr)
{
    const double lo = phc - wk, hi = phc + wk;
    if (hi > lo) {  // not wk > 0: a width below the spacing of the doubles at phc is a point (MODEL_SPEC 3)
        const double iw = FX_INV / (hi - lo);  // -lo - -hi = hi - lo exactly
        return make_double2(long_window(W, K, 0, lo, hi, iw, ctr) + long_window(W, K, 0, -hi, -lo, iw, ctr),
                            long_window(W, K, 1, lo, hi, iw, ctr) + long_window(W, K, 1, -hi, -lo, iw, ctr));
    }
    return make_double2(long_point(W, K, 0, phc) + long_point(W, K, 0, -phc),
                        long_point(W, K, 1, phc) + long_point(W, K, 1, -phc));
}

// sub_point with its donor cursor carried from point to point (SubCur): a
// point whose first sub-bin lies at or above the last one's phase walks on
// from there instead of a fresh lookup (a thread's run of sorted points);
// the line of sight is formed afresh at each point's first sub-bin
// the donor cursor runs two entries ahead: the next entry's position, code
// and tile vector (fixed point as a double: long_tables' step (g)) and the one after's
// position and code are in registers, their loads issued a crossing earlier
// -- a crossing applies the vector and moves the pipe on without waiting on LDS
// the donor sum V of the point phase, in fixed-point units but held as a
// double: the sub-bin sums take it without an int64 -> double conversion per
// sub-bin (12 instructions; 2.72 -> 2.91 M evals/s at config 5).  The sum
// over a thread's crossings rounds, ~1e-15 of V's scale, against exact int64
// (the tables' cell prefixes and the tiles' vectors stay exact)
using LongV = double;
struct SubCur {
    double ph, npos, n2pos;
    LongV nq[3];  // the next entry's tile vector (fixed point, before the mirror's signs)
    LongV vx, vy, vz;
    int cur, ncode, n2code;
    double dkw = -1.0, dk = 0.0;  // sub_point_quiet's Dirichlet kernel of width dkw
};

__device__ __forceinline__ void subcur_fill(const SubEntries& D, const double* sdq, int nd, SubCur& U)
{
    U.npos = U.cur < nd ? D.dpos[U.cur] : INFINITY;
    U.ncode = U.cur < nd ? D.dcode[U.cur] : 0;
    U.n2pos = U.cur + 1 < nd ? D.dpos[U.cur + 1] : INFINITY;
    U.n2code = U.cur + 1 < nd ? D.dcode[U.cur + 1] : 0;
    const LongV* dq = reinterpret_cast<const LongV*>(sdq + ((U.ncode >> 1) >> 2) * DON_STRIDE);
    U.nq[0] = dq[0]; U.nq[1] = dq[1]; U.nq[2] = dq[2];
}

#ifndef LFG_LW_BASE
#define LFG_LW_BASE 3
#endif
#ifndef LFG_LW_WD
#define LFG_LW_WD 2
#endif
#ifndef LFG_LW_SPOT
#define LFG_LW_SPOT 3
#endif
// a point's estimated cost in the LONG point phase (the partition of the
// points over the threads): windows in the WD/disc hulls walk the tables,
// those in the spot hull the spot entries at every sub-bin
__device__ __forceinline__ int long_weight(const LongU& K, double ph0, double w)
{
    const double phc = wrap_phase(ph0), wk = w < 0.0 ? 0.0 : w, lo = phc - wk, hi = phc + wk;
    bool wd = false;
    for (int t = 0; t < 2; ++t)
        wd = wd || (hi >= K.amin[t] && lo <= K.bmax[t]) || (-lo >= K.amin[t] && -hi <= K.bmax[t]);
    const bool sp = hi >= K.sa && lo <= K.sb;
    // weights from A/B runs at config 5 (wave ranges with interleaved lanes):
    // 5/3/1 2.39 M evals/s, 5/8/2 2.34, 5/1/1 2.31, uniform 2.36 (round 5);
    // round 6, with the quiet points in closed form: the spot hull's points
    // all take the sub-bin loop (LFG_LW_* to retune)
    return LFG_LW_BASE + (wd ? LFG_LW_WD : 0) + (sp ? LFG_LW_SPOT : 0);
}

// a crossing of entry cur: its vector into V (the mirror image's signs on the
// unique tile's fixed-point vector), then the pipe one entry on
__device__ __forceinline__ void subcur_cross(const SubEntries& D, const double* sdq, int nd, SubCur& U)
{
    const int code = U.ncode, mr = (code >> 1) & 3;
    const LongV qx = U.nq[0], qy = (mr & 1) ? -U.nq[1] : U.nq[1], qz = (mr & 2) ? -U.nq[2] : U.nq[2];
    if (code & 1) { U.vx -= qx; U.vy -= qy; U.vz -= qz; }
    else { U.vx += qx; U.vy += qy; U.vz += qz; }
    ++U.cur;
    U.npos = U.n2pos;
    U.ncode = U.n2code;
    const LongV* dq = reinterpret_cast<const LongV*>(sdq + ((U.ncode >> 1) >> 2) * DON_STRIDE);
    U.nq[0] = dq[0]; U.nq[1] = dq[1]; U.nq[2] = dq[2];
    U.n2pos = U.cur + 1 < nd ? D.dpos[U.cur + 1] : INFINITY;
    U.n2code = U.cur + 1 < nd ? D.dcode[U.cur + 1] : 0;
}

__device__ __forceinline__ double2 sub_point_c(const SubTables& T, const SubEntries& D, const double2* sab,
                                               const double* sbw, const double* sdq, const LongU& K, double ph0,
                                               double wk, int S, SubCur& U)
{
    const int nd = K.nd, nsp = K.nsp;
    const double h = wk * K.invS, ih = 0.5 / h;
    // the first sub-bin's line of sight and the turn per sub-bin
    const double phA = wrap_phase(ph0 - wk + h);
    const double4 eA = sincospi2_ool(2.0 * phA, 4.0 * h);
    double sbs = 0.0, srs1 = 0.0, srs2 = 0.0, sn = 0.0, cs = 1.0, rs = 0.0, rc = 1.0;
    long long Cs = 0;
    int scur = 0;
    bool sv = false;  // Cs / scur hold C at this sub-bin's lo
    for (int j = 0; j < S; ++j) {
        const double phn = wrap_phase(ph0 - wk + (2 * j + 1) * h);
        if (!(phn >= U.ph)) {  // a fresh lookup (the first point, a step back in phase)
            {  // sub_donor with the tiles' fixed-point vectors
                const int g = tcell(phn, T.dt0, T.dginv);
                U.vx = LongV(T.dpre[g][0]);
                U.vy = LongV(T.dpre[g][1]);
                U.vz = LongV(T.dpre[g][2]);
                int i = g ? T.dend[g - 1] : 0;
                for (const int ie = T.dend[g]; i < ie; ++i) {
                    const int code = D.dcode[i];
                    if (!donor_counted(D.dpos[i], code, phn)) break;
                    const int mr = (code >> 1) & 3;
                    const LongV* dq = reinterpret_cast<const LongV*>(sdq + ((code >> 1) >> 2) * DON_STRIDE);
                    const LongV qx = dq[0], qy = (mr & 1) ? -dq[1] : dq[1], qz = (mr & 2) ? -dq[2] : dq[2];
                    if (code & 1) { U.vx -= qx; U.vy -= qy; U.vz -= qz; }
                    else { U.vx += qx; U.vy += qy; U.vz += qz; }
                }
                U.cur = i;
            }
            subcur_fill(D, sdq, nd, U);
        } else {
            while (donor_counted(U.npos, U.ncode, phn))  // npos = inf past the last entry
                subcur_cross(D, sdq, nd, U);
        }
        if (j == 0 || !(phn >= U.ph)) {
            const double4 e4 = j == 0 ? eA : sincospi2_ool(2.0 * phn, 4.0 * h);  // the turn per sub-bin: 2 pi (2 h)
            sn = e4.x;
            cs = e4.y;
            rs = e4.z;
            rc = e4.w;
        } else {
            const double c2 = fma(cs, rc, -sn * rs);
            sn = fma(sn, rc, cs * rs);
            cs = c2;
        }
        U.ph = phn;
        // spot: as sub_point (the windows of a point abut; each point starts afresh)
        double ebj = 0.0;
        const double lo = phn - h, hi = phn + h;
        if (!(h > 0.0)) {
            ebj = sub_spot(T, sab, sbw, K.itb, lo, hi, K.sa, K.sb);
        } else if (hi > K.sa && lo < K.sb) {
            const double itb = K.itb;
            if (!sv) Cs = spot_C(T, sbw, itb, lo, scur);
            sv = true;
            long long Cn = Cs;
            double corr = 0.0;
            for (; scur < nsp && T.spos[scur] <= hi; ++scur) {
                const int code = T.scode[scur], k = code >> 1;
                const double wn = sbw[k] * itb;
                const double2 ab = sab[k];
                const long long Wq = to_fx(wn);
                if (!(code & 1)) {
                    Cn += Wq;
                    corr = fma(wn, fmin(ab.y, hi) - ab.x, corr);
                } else {
                    Cn -= Wq;
                    if (ab.x <= lo) corr = fma(-wn, hi - ab.y, corr);
                }
            }
            ebj = fma(corr, ih, double(Cs) * FX_INV);
            Cs = Cn;
        } else {
            sv = false;
        }
        // e = (s cos, -s sin, c) at the sub-phase: the donor term V . e and
        // the spot's beaming term fis + (1 - fis) max(nb . e, 0) (sg, cg folded in)
        srs1 = fma(cs, double(U.vx), fma(-sn, double(U.vy), srs1));
        srs2 += double(U.vz);
        sbs = fma(fma(K.omf, fmax(fma(K.nbs0, cs, fma(K.nbs1, sn, K.nbc)), 0.0), K.fis), 1.0 - ebj, sbs);
    }
    return make_double2(sbs * K.ibden, fma(K.sg, srs1, K.cg * srs2) * K.dsc);
}

// ---- LONG quiet points: sub_point_c's sums in closed form ----
// A point is quiet when, over its window [ph - w, ph + w] (S sub-bins):
//  * no donor entry is counted between its first and its last sub-bin (the
//    donor vector V is the same at every sub-bin),
//  * the window is off the spot's hull (no sub-bin sees the spot eclipsed),
//  * the beaming term b(phi) = nbs0 cos 2 pi phi + nbs1 sin 2 pi phi + nbc
//    keeps one sign (neither of its two zero crossings lies in the window),
//  * the window neither wraps at +-0.5 nor has a zero or NaN width.
// The sub-bins' lines of sight then sum to D (cos, sin)(2 pi ph) with the
// Dirichlet kernel D = sin(2 pi w) / sin(2 pi w / S) (the sub-bin centres lie
// symmetrically about ph, 2 h apart), every sum of sub_point_c is linear in
// them, and the point costs one sincospi instead of S sub-bin steps.
// (Config 5: ~80 % of the points; the sub-bin sums were 57 % of the point
// phase's VALU instructions.)  The others run sub_point_c.
struct LongB {          // the beaming term's zero crossings, per pair (uniform)
    double z0, z1;      // phases in [-0.5, 0.5)
    int any;            // 0: b keeps one sign over the orbit
};

__device__ __forceinline__ LongB long_beam_zeros(const LongU& K)
{
    LongB B{0.0, 0.0, 0};
    const double R = sqrt(K.nbs0 * K.nbs0 + K.nbs1 * K.nbs1);
    if (R > fabs(K.nbc)) {  // b = R cos(2 pi phi - t) + nbc crosses zero twice
        const double t = atan2(K.nbs1, K.nbs0), a = acos(-K.nbc / R);
        B.z0 = uni(wrap_phase((t - a) * (1.0 / TWO_PI)));
        B.z1 = uni(wrap_phase((t + a) * (1.0 / TWO_PI)));
        B.any = 1;
    }
    return B;
}

// sin(x) / x, |x| < 0.1: the series to x^10 (error < 2e-22)
__device__ __forceinline__ double sinc_small(double x)
{
    const double x2 = x * x;
    return fma(x2, fma(x2, fma(x2, fma(x2, fma(x2, -1.0 / 39916800.0, 1.0 / 362880.0), -1.0 / 5040.0),
                               1.0 / 120.0), -1.0 / 6.0), 1.0);
}

// true and the sums (as sub_point_c returns them) for a quiet point; false
// for the others.  Either way U is left at the point's first sub-bin, as
// sub_point_c's first step leaves it (the cursor walks on from there)
__device__ __forceinline__ bool sub_point_quiet(const SubTables& T, const SubEntries& D, const double* sbw,
                                                const double* sdq, const LongU& K, const LongB& B, double ph0,
                                                double wk, int S, SubCur& U, double2& out)
{
    const double h = wk * K.invS;
#ifdef LFG_COUNT_QUIET  // (diagnostic builds, with LFG_COUNT_ITERS: lfg_diag_iters) why points are not quiet
#define QCNT(k) atomicAdd(g_iter_dbg + 56 + (k), 1ull)
    QCNT(0);
#else
#define QCNT(k)
#endif
#ifdef LFG_ABL_QNONE  // (diagnostic builds) every point through the queue and sub_point_c
    return false;
#endif
    if (!(h > 0.0)) { QCNT(1); return false; }  // zero or NaN widths
    const double phc = wrap_phase(ph0), lo = phc - wk, hi = phc + wk;
    constexpr double EPS = 1e-9;   // margins on the phase tests (the sub-bin loop's own phases round)
#ifndef LFG_ABL_QALL  // (diagnostic builds: every point in closed form, a timing floor; wrong sums)
    if (!(lo > -0.5 + EPS && hi < 0.5 - EPS)) { QCNT(2); return false; }
    // the spot: the window off its hull, or inside it (then no spot entry may lie in the window)
    const bool inspot = hi + EPS > K.sa && lo - EPS < K.sb;
    if (inspot && !(lo - EPS > K.sa && hi + EPS < K.sb)) { QCNT(3); return false; }
    if (B.any && ((B.z0 > lo - EPS && B.z0 < hi + EPS) || (B.z1 > lo - EPS && B.z1 < hi + EPS))) { QCNT(4); return false; }
#endif
    // the donor vector at the first sub-bin, as sub_point_c finds it
    const int nd = K.nd;
    const double ph1 = wrap_phase(ph0 - wk + h);
    if (!(ph1 >= U.ph)) {
        const int g = tcell(ph1, T.dt0, T.dginv);
        U.vx = LongV(T.dpre[g][0]);
        U.vy = LongV(T.dpre[g][1]);
        U.vz = LongV(T.dpre[g][2]);
        int i = g ? T.dend[g - 1] : 0;
        for (const int ie = T.dend[g]; i < ie; ++i) {
            const int code = D.dcode[i];
            if (!donor_counted(D.dpos[i], code, ph1)) break;
            const int mr = (code >> 1) & 3;
            const LongV* dq = reinterpret_cast<const LongV*>(sdq + ((code >> 1) >> 2) * DON_STRIDE);
            const LongV qx = dq[0], qy = (mr & 1) ? -dq[1] : dq[1], qz = (mr & 2) ? -dq[2] : dq[2];
            if (code & 1) { U.vx -= qx; U.vy -= qy; U.vz -= qz; }
            else { U.vx += qx; U.vy += qy; U.vz += qz; }
        }
        U.cur = i;
        subcur_fill(D, sdq, nd, U);
    } else {
        while (donor_counted(U.npos, U.ncode, ph1)) subcur_cross(D, sdq, nd, U);
    }
    U.ph = ph1;
    const double phS = wrap_phase(ph0 - wk + (2 * S - 1) * h);  // the last sub-bin
#ifndef LFG_ABL_QALL
    // an entry counted by a later sub-bin moves V inside the window: the
    // sub-bin loop (a closed form per crossing, Dirichlet kernels of the
    // sub-bins after it, held more registers than the loop has: 25-42
    // spilled VGPRs, slower than the loop on 4 % of the points)
    if (donor_counted(U.npos, U.ncode, phS)) { QCNT(5); return false; }
#endif
    // the spot's covering weight at the first sub-bin's lo, as sub_point_c
    // takes it (spot_C); with no entry up to the last sub-bin's hi it is the
    // eclipsed fraction of every sub-bin
    double E = 0.0;
    if (inspot) {
        int cur;
        const long long C = spot_C(T, sbw, K.itb, ph1 - h, cur);
        if (cur < K.nsp && T.spos[cur] <= phS + h + EPS) { QCNT(3); return false; }
        E = double(C) * FX_INV;
    }
    // the Dirichlet kernel of the sub-bins' turn (2 pi 2 h per sub-bin)
    const double x = TWO_PI * wk, xs = TWO_PI * h;
    double Dk;
    if (wk == U.dkw) {  // the lane's last width (the cursor keeps its kernel): config 5 +1.5 %
        Dk = U.dk;
    } else {
        if (x < 0.1) {
            Dk = S * (sinc_small(x) / sinc_small(xs));
        } else {
            // w >= 0.0159: reached at S = 1 only (Dk = 1).  With sub-bins a
            // quiet window has no donor entry over 2 w (1 - 1 / S) >= w of
            // phase, and the longest stretch without one is 0.0134 (edge-on;
            // tests/test_long_windows.py surveys the prior's q and dphi)
            const double2 a = sincospi_ool(2.0 * wk), b = sincospi_ool(2.0 * h);
            Dk = a.x / b.x;
        }
        U.dkw = wk;
        U.dk = Dk;
    }
    // (sin, cos) at the window's centre, inlined: out of line while the
    // unit was compiled with machine LICM (inlined, its hoisted constants
    // spilled: config 5 -13 %); without the pass inlined is +0.7 %
    // (profiles/r06/long/ab_sincospi_inline_nolicm.txt)
    double esn, ecs;
    sincospi(2.0 * phc, &esn, &ecs);
    const double2 e = make_double2(esn, ecs);
    const double Scs = Dk * e.y, Ssn = Dk * e.x;
    const double srs1 = fma(Scs, double(U.vx), -Ssn * double(U.vy)), srs2 = S * double(U.vz);
    const double bc = fma(K.nbs0, e.y, fma(K.nbs1, e.x, K.nbc));  // b at the centre: its sign in the window
    const double sbs = (1.0 - E) * (bc > 0.0 ? fma(K.omf, fma(K.nbs0, Scs, fma(K.nbs1, Ssn, S * K.nbc)), S * K.fis)
                                             : S * K.fis);
    out = make_double2(sbs * K.ibden, fma(K.sg, srs1, K.cg * srs2) * K.dsc);
    QCNT(6);
    return true;
#undef QCNT
}

// the LONG tables from the element phase's results in LDS (all threads of
// the block, after the phase barrier; seven barriers).  abw: the WD/disc
// intervals by sweep slot; the spot (sab, sbw), the donor tiles (sdq), the
// disc ring weights (swt) and the spot / donor fixed-point totals (stot) as
// k_pair's point-major sinks leave them.  The tables must be zero (k_pair's
// prologue clears them).  Step (g) rewrites each unique donor tile's first
// three sdq words as its fixed-point vector in doubles (the point phase's form)
__device__ __forceinline__ void long_tables(LongTabs& W, SubTables& T, SubEntries& D, const double2* abw,
                                            const double2* sab, const double* sbw, double* sdq,
                                            const double* swt, const unsigned long long* stot, double ul, double itwd,
                                            long long (*spart)[LIKE_THREADS / 64], int tid)
{
    constexpr int nt = LIKE_THREADS, nw = LIKE_THREADS / 64;
    const int lane = tid & 63, wv = tid >> 6;
    // (a) hulls of the WD/disc and spot intervals, the donor |v| sum
    double amin[2] = {INFINITY, INFINITY}, bmax[2] = {-INFINITY, -INFINITY}, sa = INFINITY, sb = -INFINITY, vs = 0.0;
    for (int g = tid; g < NU_WDD; g += nt) {
        const double2 ab = abw[g];
        const int t = uitem(g) < U_WD ? 0 : 1;
        if (ab.x < ab.y) {
            amin[t] = fmin(amin[t], ab.x);
            bmax[t] = fmax(bmax[t], ab.y);
        }
    }
    if (tid < NBS && sab[tid].x < sab[tid].y) { sa = sab[tid].x; sb = sab[tid].y; }
    if (tid < U_DON)  // the four mirror images of a tile have the same |vx| + |vy| + |vz|
        vs = 4.0 * (fabs(sdq[tid * DON_STRIDE]) + fabs(sdq[tid * DON_STRIDE + 1]) + fabs(sdq[tid * DON_STRIDE + 2]));
    for (int t = 0; t < 2; ++t) {
        amin[t] = wave_min(amin[t]);
        bmax[t] = wave_max(bmax[t]);
    }
    sa = wave_min(sa); sb = wave_max(sb); vs = wave_sum(vs);
    if (lane == 0) {
        W.part[0][wv] = amin[0]; W.part[1][wv] = bmax[0]; W.part[2][wv] = sa; W.part[3][wv] = sb; W.part[4][wv] = vs;
        W.part[5][wv] = amin[1]; W.part[6][wv] = bmax[1];
    }
    __syncthreads();
    LONG_TSTAMP(0);
    amin[0] = amin[1] = INFINITY; bmax[0] = bmax[1] = -INFINITY; sa = INFINITY; sb = -INFINITY; vs = 0.0;
    for (int k = 0; k < nw; ++k) {  // every thread forms the block's values (no barrier for a broadcast)
        amin[0] = fmin(amin[0], W.part[0][k]); bmax[0] = fmax(bmax[0], W.part[1][k]);
        amin[1] = fmin(amin[1], W.part[5][k]); bmax[1] = fmax(bmax[1], W.part[6][k]);
        sa = fmin(sa, W.part[2][k]); sb = fmax(sb, W.part[3][k]); vs += W.part[4][k];
    }
    // the cells of table t over its own hull (the WD contacts crowd a narrower one)
    double t0[2], ginv[2];
    for (int t = 0; t < 2; ++t) {
        t0[t] = amin[t];
        ginv[t] = (bmax[t] > amin[t]) ? LONG_FC / (bmax[t] - amin[t]) : 0.0;
    }
    const double st0 = sa, sginv = (sb > sa) ? TCELLS / (sb - sa) : 0.0;
    constexpr double t0d = -0.5, t1d = 0.5, dginv = TCELLS;  // donor cells: the whole phase circle
    const double itb = 1.0 / (double(static_cast<long long>(stot[0])) * (FX_INV / PAIR_SPOT_S)), ivs = 1.0 / vs;
    if (tid == 0) {
        for (int t = 0; t < 2; ++t) { W.t0[t] = t0[t]; W.ginv[t] = ginv[t]; W.amin[t] = amin[t]; W.bmax[t] = bmax[t]; }
        W.snorm[0] = itb;
        W.snorm[1] = ivs;
        W.snorm[2] = double(static_cast<long long>(stot[1])) * (FX_INV / PAIR_DON_S);
        W.snorm[3] = vs;
        W.shull[0] = fmin(amin[0], amin[1]); W.shull[1] = fmax(bmax[0], bmax[1]); W.shull[2] = sa; W.shull[3] = sb;
        T.dt0 = t0d; T.dginv = dginv; T.st0 = st0; T.sginv = sginv;
    }
    // (b) counts and fixed-point sums per cell
    auto wd_entry = [&](int g, double2& ab, int& t, long long& q) {
        ab = abw[g];
        if (!(ab.x < ab.y)) return false;
        const int u = uitem(g), ir = pair_ring(u);
        t = u < U_WD ? 0 : 1;
        q = to_fx(u < U_WD ? wd_ring_weight(ir, ul) * itwd : swt[ir - NWD_RINGS] * (1.0 / swt[NDISC_R]));
        return true;
    };
    for (int g = tid; g < NU_WDD; g += nt) {
        double2 ab;
        int t;
        long long q;
        if (!wd_entry(g, ab, t, q)) continue;
        (void)q;
        atomicAdd(&W.fend[t][long_cell(ab.x, t0[t], ginv[t])], 1);
        atomicAdd(&W.fend[t][long_cell(ab.y, t0[t], ginv[t])], 1);
    }
    {
        double p0, p1;
        bool in0, in1;
        int v0;
        lane_breakpoints(tid, sdq, sab, t0d, t1d, p0, p1, in0, in1, v0);
        long long c0[3] = {0, 0, 0};  // this lane's share of V0, summed per wave below
        if (tid >= nt - NDONOR) {
            long long q[3];
            donor_q(sdq, tid - (nt - NDONOR), ivs, q[0], q[1], q[2]);
            for (int k = 0; k < 3; ++k) c0[k] = v0 * q[k];
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
            const long long Wq = to_fx(sbw[tid] * itb);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int g = tcell(b ? p1 : p0, st0, sginv);
                atomicAdd(&T.send[g], 1);
                atomicAdd(reinterpret_cast<unsigned long long*>(&T.spre[g]), static_cast<unsigned long long>(b ? -Wq : Wq));
            }
        }
        // V0: the wave's sum, one atomic per component (half the donor lanes
        // add to these three words; per-lane atomics serialised on them)
        for (int k = 0; k < 3; ++k) {
            const long long w = wave_scan_incl(c0[k], lane);
            if (lane == 63 && w != 0)
                atomicAdd(reinterpret_cast<unsigned long long*>(&T.dv0[k]), static_cast<unsigned long long>(w));
        }
    }
    __syncthreads();
    LONG_TSTAMP(1);
    // (c) exclusive prefixes over the cells: each wave scans one whole array
    // (a lane its run of consecutive cells, then the wave's 64 sums), so no
    // part sums cross waves and one barrier ends the step
    static_assert(TCELLS == 4 * 64 && LONG_FC == 16 * 64 && nw == 8, "eight arrays, one per wave");
    (void)spart;
    {
        const int a = wv;  // 0, 1: the WD/disc cells; 2..7: the sub-bin tables' cells
        auto get = [&](int g) -> long long {
            switch (a) {
            case 0: return W.fend[0][g];
            case 1: return W.fend[1][g];
            case 2: return T.dend[g];
            case 3: return T.send[g];
            case 4: return T.dpre[g][0];
            case 5: return T.dpre[g][1];
            case 6: return T.dpre[g][2];
            default: return T.spre[g];
            }
        };
        auto set = [&](int g, long long x) {
            switch (a) {
            case 0: W.fend[0][g] = int(x); break;
            case 1: W.fend[1][g] = int(x); break;
            case 2: T.dend[g] = int(x); break;
            case 3: T.send[g] = int(x); break;
            case 4: T.dpre[g][0] = x + T.dv0[0]; break;
            case 5: T.dpre[g][1] = x + T.dv0[1]; break;
            case 6: T.dpre[g][2] = x + T.dv0[2]; break;
            default: T.spre[g] = x; break;
            }
        };
        if (a < 2) {  // 16 cells per lane, int counts: loaded once, in one round trip
            constexpr int PER = LONG_FC / 64;
            int* f = W.fend[a] + PER * lane;
            int c[PER];
            int own = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                c[j] = f[j];
                own += c[j];
            }
            int run = int(wave_scan_incl(own, lane)) - own;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                f[j] = run;
                run += c[j];
            }
        } else {
            constexpr int PER = TCELLS / 64;
            const int g0 = PER * lane;
            long long c[PER];
            long long own = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                c[j] = get(g0 + j);
                own += c[j];
            }
            long long run = wave_scan_incl(own, lane) - own;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                set(g0 + j, run);
                run += c[j];
            }
        }
    }
    __syncthreads();
    LONG_TSTAMP(2);
    // (d) the entries into cell order; afterwards cend / dend / send hold the cell ends
    for (int g = tid; g < NU_WDD; g += nt) {
        double2 ab;
        int t;
        long long q;
        if (!wd_entry(g, ab, t, q)) continue;
        const int base = t ? NE_W : 0;
        const int ia = atomicAdd(&W.fend[t][long_cell(ab.x, t0[t], ginv[t])], 1);
        W.epos[base + ia] = ab.x;
        W.ecb[base + ia] = q;
        const int ib = atomicAdd(&W.fend[t][long_cell(ab.y, t0[t], ginv[t])], 1);
        W.epos[base + ib] = ab.y;
        W.ecb[base + ib] = -q;
    }
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
                D.dpos[slot] = pos;
                D.dcode[slot] = base + b;
            } else {
                const int slot = atomicAdd(&T.send[tcell(pos, st0, sginv)], 1);
                T.spos[slot] = pos;
                T.scode[slot] = base + b;
            }
        }
    }
    __syncthreads();
    LONG_TSTAMP(3);
    // (e) every cell's entries in order: each entry counts the entries of its
    // cell that sort before it and moves to that rank (all entries at once;
    // an insertion sort per cell took O(n^2) steps in the cells where the WD
    // contacts crowd).  WD/disc by (position, weight), donor by position with
    // an end before a start (sub_point's cursor), spot by (position, code):
    // total orders, so the tables (and long_window's double sums) do not
    // depend on the atomics' slot order
    {
        constexpr int RW = (NE_W + NE_D + nt - 1) / nt, RD = (TD_MAX + nt - 1) / nt;
        double wp[RW], dp[RD], sp = 0.0;
        long long wq[RW];
        int wslot[RW], dc[RD], dslot[RD], sc = 0, sslot = -1;
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            wslot[r] = -1;
            wp[r] = 0.0;
            wq[r] = 0;
            const int i = tid + r * nt, t = i < NE_W ? 0 : 1, base = t ? NE_W : 0, li = i - base;
            if (i >= NE_W + NE_D || li >= W.fend[t][LONG_FC - 1]) continue;
            const double p = W.epos[i];
            const long long q = W.ecb[i];
            const int g = long_cell(p, t0[t], ginv[t]), c0 = g ? W.fend[t][g - 1] : 0, c1 = W.fend[t][g];
            int rank = 0;
#pragma unroll 4
            for (int k = c0; k < c1; ++k) {
                const double pk = W.epos[base + k];
                const long long qk = W.ecb[base + k];
                rank += (pk < p || (pk == p && (qk < q || (qk == q && k < li)))) ? 1 : 0;
            }
            wp[r] = p;
            wq[r] = q;
            wslot[r] = base + c0 + rank;
        }
        const int ndn = T.dend[TCELLS - 1], nsn = T.send[TCELLS - 1];
#pragma unroll
        for (int r = 0; r < RD; ++r) {
            dslot[r] = -1;
            dp[r] = 0.0;
            dc[r] = 0;
            const int i = tid + r * nt;
            if (i >= ndn) continue;
            const double p = D.dpos[i];
            const int c = D.dcode[i], g = tcell(p, t0d, dginv), c0 = g ? T.dend[g - 1] : 0, c1 = T.dend[g];
            int rank = 0;
#pragma unroll 4
            for (int k = c0; k < c1; ++k) {
                const double pk = D.dpos[k];
                const int ck = D.dcode[k];
                rank += (pk < p || (pk == p && ((ck & 1) > (c & 1) || ((ck & 1) == (c & 1) && (ck < c || (ck == c && k < i))))))
                            ? 1 : 0;
            }
            dp[r] = p;
            dc[r] = c;
            dslot[r] = c0 + rank;
        }
        if (tid < nsn) {
            const double p = T.spos[tid];
            const int c = T.scode[tid], g = tcell(p, st0, sginv), c0 = g ? T.send[g - 1] : 0, c1 = T.send[g];
            int rank = 0;
#pragma unroll 4
            for (int k = c0; k < c1; ++k) {
                const double pk = T.spos[k];
                const int ck = T.scode[k];
                rank += (pk < p || (pk == p && (ck < c || (ck == c && k < tid)))) ? 1 : 0;
            }
            sp = p;
            sc = c;
            sslot = c0 + rank;
        }
        __syncthreads();
    LONG_TSTAMP(4);
#pragma unroll
        for (int r = 0; r < RW; ++r)
            if (wslot[r] >= 0) {
                W.epos[wslot[r]] = wp[r];
                W.ecb[wslot[r]] = wq[r];
            }
#pragma unroll
        for (int r = 0; r < RD; ++r)
            if (dslot[r] >= 0) {
                D.dpos[dslot[r]] = dp[r];
                D.dcode[dslot[r]] = dc[r];
            }
        if (sslot >= 0) {
            T.spos[sslot] = sp;
            T.scode[sslot] = sc;
        }
    }
    __syncthreads();
    LONG_TSTAMP(5);
    // (f) C just after each sorted WD/disc entry: the running sum of the
    // weights in table order (exact int64), a wave per table, a lane a run
    if (wv < 2) {
        const int t = wv, n = W.fend[t][LONG_FC - 1], B = (n + 63) >> 6, k0 = min(lane * B, n), k1 = min(k0 + B, n);
        long long* q = W.ecb + (t ? NE_W : 0);
        long long own = 0;
        for (int k = k0; k < k1; ++k) own += q[k];
        long long run = wave_scan_incl(own, lane) - own;
        for (int k = k0; k < k1; ++k) {
            run += q[k];
            q[k] = run;
        }
    }
    // (g) each unique donor tile's vector in fixed point (held as doubles),
    // in place of its raw components (the point phase adds them at its donor
    // crossings; a mirror image's components differ in sign only, and to_fx
    // is odd)
    if (tid >= 128 && tid < 128 + U_DON) {  // waves 2.. (0 and 1 run (f))
        double* dq = sdq + (tid - 128) * DON_STRIDE;
        const long long q0 = to_fx(dq[0] * ivs), q1 = to_fx(dq[1] * ivs), q2 = to_fx(dq[2] * ivs);
        LongV* dl = reinterpret_cast<LongV*>(dq);
        dl[0] = q0;
        dl[1] = q1;
        dl[2] = q2;
    }
    __syncthreads();
    LONG_TSTAMP(6);
}
