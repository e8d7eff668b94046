// lfg_sweep.hpp -- the tile sweep's arithmetic: the phase index over a tile's
// sorted windows, an element's runs over them, and the entries the runs add to
// a difference array (int64 fixed point, so that the sums are exact in any
// order).  Shared by k_lnlike (lfg.hip), k_pair's sinks (lfg_k_pair.hpp) and, through
// cpu_baseline/shim, host programs: the add itself goes through a functor
// (an LDS atomic on the device) and the wave vote of apply_runs_merged through
// another (the lane's own predicate on the host).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace lfg {

constexpr int LIKE_THREADS = 512;
constexpr int LIKE_TILE = LIKE_THREADS;  // one point per thread per tile
constexpr int LIKE_NC = 2 * LIKE_TILE;   // cells of the phase index
#ifndef LFG_WALK
#define LFG_WALK 2  // unrolled forward steps of the cell walk before the loop
#endif
constexpr double FX_SCALE = 2305843009213693952.0;  // 2^61
constexpr double FX_INV = 1.0 / FX_SCALE;

struct PhaseIndex {  // sorted phases v[0..m) with a uniform-cell start table
    const double* v;
    const int* cell;
    int m;
    double t0, ginv;
};

__device__ __forceinline__ int cell_of(const PhaseIndex& X, double v)
{
    const double u = (v - X.t0) * X.ginv;
    return u <= 0.0 ? 0 : (u >= double(LIKE_NC) ? LIKE_NC : int(u));
}

// #{v_p < x} (or #{v_p <= x} when LE).  cell[ci(x)] counts the points whose
// cell index is below x's, all of which lie below x (ci is monotone), so the
// walk only goes forward: usually zero or one point, two unrolled steps
template <bool LE>
__device__ __forceinline__ int count_below(const PhaseIndex& X, double x)
{
    int j = X.cell[cell_of(X, x)];
    const int last = X.m - 1;
    bool adv = false;
#pragma unroll
    for (int k = 0; k < LFG_WALK; ++k) {
        const double vj = X.v[min(j, last)];
        adv = (j <= last) & (LE ? (vj <= x) : (vj < x));
        j += adv ? 1 : 0;
    }
    if (adv)  // clustered points: keep walking
        while (j <= last && (LE ? (X.v[j] <= x) : (X.v[j] < x))) ++j;
    return j;
}

// count_below<false> for Q queries in lockstep, so that their LDS chains overlap
template <int Q>
__device__ __forceinline__ void count_lt_multi(const PhaseIndex& X, const double (&x)[Q], int (&j)[Q])
{
    const int last = X.m - 1;
#pragma unroll
    for (int q = 0; q < Q; ++q) j[q] = X.cell[cell_of(X, x[q])];
    bool adv[Q];
#pragma unroll
    for (int k = 0; k < LFG_WALK; ++k) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const double vj = X.v[min(j[q], last)];
            adv[q] = (j[q] <= last) & (vj < x[q]);
            j[q] += adv[q] ? 1 : 0;
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
        if (adv[q])
            while (j[q] <= last && X.v[j[q]] < x[q]) ++j[q];
}

// count_le_back for Q queries in lockstep
template <int Q>
__device__ __forceinline__ void count_le_back_multi(const double* __restrict__ hi, const double (&x)[Q],
                                                    const int (&J)[Q], int (&out)[Q])
{
    bool back[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        back[q] = (J[q] > 0) & (hi[max(J[q] - 1, 0)] > x[q]);
        out[q] = J[q] - (back[q] ? 1 : 0);
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
        if (back[q])
            while (out[q] > 0 && hi[out[q] - 1] > x[q]) --out[q];
}

// #{hi <= x} given J = #{lo < x}: hi > lo, so the answer is <= J; the points
// straddling x (usually one) are stepped over backwards
__device__ __forceinline__ int count_le_back(const double* __restrict__ hi, int J, double x)
{
    const bool back = (J > 0) & (hi[max(J - 1, 0)] > x);
    J -= back ? 1 : 0;
    if (back)
        while (J > 0 && hi[J - 1] > x) --J;
    return J;
}

// cell[g] = #{p : ci(v_p) < g} with ci(v) = floor((v - t0) ginv) clamped to
// [-1, NC] exactly as cell_of computes it: point p fills the cells
// (ci(v_{p-1}), ci(v_p)], the last point also the cells above its own
__device__ __forceinline__ PhaseIndex phase_index(const double* v, const int* cell, int m)
{
    const double span = v[m - 1] - v[0];
    return PhaseIndex{v, cell, m, v[0], span > 0.0 ? LIKE_NC / span : 0.0};
}

__device__ __forceinline__ long long to_fx(double x) { return static_cast<long long>(rint(x * FX_SCALE)); }

// the runs of element [a, b] over the tile's windows [lo_p, hi_p] (lo, hi
// sorted, hi >= lo): it overlaps [P1, P4) and covers [P2, P3) whole.  A
// zero-width window is a point: covered when a <= ph <= b, never partial.
struct Runs {
    int P1, P2, P3, P4;
};

__device__ __forceinline__ Runs element_runs(double a, double b, const PhaseIndex& X, const double* __restrict__ hi)
{
    Runs R;
    R.P2 = count_below<false>(X, a);
    R.P4 = count_below<false>(X, b);
    R.P1 = count_le_back(hi, R.P2, a);
    R.P3 = count_le_back(hi, R.P4, b);
    return R;
}

// adds wn * (covered fraction) of element [a, b] given its runs: add(p, q)
// adds the int64 q to slot p of the difference array
template <class Add>
__device__ __forceinline__ void apply_runs(const Runs& R, double a, double b, double wn, const PhaseIndex& X,
                                           const double* __restrict__ hi, const double* __restrict__ iw, Add add)
{
    const int P1 = R.P1, P2 = R.P2, P3 = R.P3, P4 = R.P4;
    int e0 = P4, s1 = P4;  // partial runs [P1, e0) and [s1, P4)
    if (P2 < P3) {         // whole-covered run (slot m is never read)
        const long long q = to_fx(wn);
        add(P2, q);
        if (P3 < X.m) add(P3, -q);
        e0 = P2;
        s1 = P3;
    }
    for (int r = 0; r < 2; ++r) {
        const int pe = r ? P4 : e0;
        for (int p = r ? s1 : P1; p < pe; ++p) {
            const double ov = fmin(b, hi[p]) - fmax(a, X.v[p]);
            if (ov > 0.0) {
                const long long q = to_fx(wn * ov * iw[p]);
                add(p, q);
                if (p + 1 < X.m) add(p + 1, -q);
            }
        }
    }
}

// apply_runs for NI intervals of one lane with every LDS read issued before
// the first atomic: a read waits for all the lane's earlier LDS operations
// (one in-order counter), so reads between atomics waited for each atomic's
// round trip.  The first K windows of each partial run are read up front
// (windows that tile the phase axis give one at each end); longer partial
// runs finish one window at a time after the atomics.  The same entries as
// apply_runs: identical integer sums.
template <int NI, class Add>
__device__ __forceinline__ void apply_runs_batched(const Runs (&R)[NI], const double (&a)[NI], const double (&b)[NI],
                                                   double wn, const PhaseIndex& X, const double* __restrict__ hi,
                                                   const double* __restrict__ iw, Add add)
{
    constexpr int K = 2;
    const int last = X.m - 1;
    int ps[NI][2], pn[NI][2];
    long long q[NI][2][K];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const bool whole = R[k].P2 < R[k].P3;
        const int e0 = whole ? R[k].P2 : R[k].P4, s1 = whole ? R[k].P3 : R[k].P4;
        ps[k][0] = R[k].P1;
        pn[k][0] = e0 - R[k].P1;
        ps[k][1] = s1;
        pn[k][1] = R[k].P4 - s1;
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const int p = min(ps[k][e] + i, last);
                const double ov = fmin(b[k], hi[p]) - fmax(a[k], X.v[p]);
                q[k][e][i] = (i < pn[k][e] && ov > 0.0) ? to_fx(wn * ov * iw[p]) : 0;
            }
    }
    const long long qw = to_fx(wn);
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        if (R[k].P2 < R[k].P3) {
            add(R[k].P2, qw);
            if (R[k].P3 < X.m) add(R[k].P3, -qw);
        }
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const int p = ps[k][e] + i;
                if (q[k][e][i] != 0) {
                    add(p, q[k][e][i]);
                    if (p + 1 < X.m) add(p + 1, -q[k][e][i]);
                }
            }
    }
#pragma unroll
    for (int k = 0; k < NI; ++k)
#pragma unroll
        for (int e = 0; e < 2; ++e)
            for (int p = ps[k][e] + K; p < ps[k][e] + pn[k][e]; ++p) {
                const double ov = fmin(b[k], hi[p]) - fmax(a[k], X.v[p]);
                if (ov > 0.0) {
                    const long long qq = to_fx(wn * ov * iw[p]);
                    add(p, qq);
                    if (p + 1 < X.m) add(p + 1, -qq);
                }
            }
}

// apply_runs_batched with the adjacent entries of a run end summed before
// they are added (k_pair's sinks, LFG_PAIR_SINK_MERGE).  Windows that tile the
// phase axis or leave gaps give partial runs of at most one window; an
// interval end then has the entries +q, -q of its partial window at P and
// P + 1 and the whole run's +qw (left end, at P2) or -qw (right end, at P3) at
// one of the same two slots.  The sums are int64 and exact in any order, so
// each end adds two summed values, not three (a zero sum is skipped; nothing
// is added at an index >= m, as before), and one window per end is read, not
// K.  An element that covers no window whole has one partial run [P1, P4) and
// no right end: its first window is taken as the left end and its second, if
// it has one, as the right end (an element across one join of two windows).
// any_lane(slow) is the wave's vote: where a lane of the wave has an end of
// two windows or more (overlapping windows), the whole wave runs
// apply_runs_batched as it is.  A lane reads its own bit in the vote, so no
// lane with such a run takes the merged path, whichever lanes vote with it.
// Identical integer sums.
template <int NI, class Add, class Vote>
__device__ __forceinline__ void apply_runs_merged(const Runs (&R)[NI], const double (&a)[NI], const double (&b)[NI],
                                                  double wn, const PhaseIndex& X, const double* __restrict__ hi,
                                                  const double* __restrict__ iw, Add add, Vote any_lane)
{
    bool slow = false;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const bool whole = R[k].P2 < R[k].P3;
        const int cut = min(R[k].P1 + 1, R[k].P4);  // no whole run: [P1, P4) as [P1, cut) and [cut, P4)
        const int e0 = whole ? R[k].P2 : cut, s1 = whole ? R[k].P3 : cut;
        slow = slow | (e0 - R[k].P1 > 1) | (R[k].P4 - s1 > 1);
    }
    if (any_lane(slow)) {
        apply_runs_batched<NI>(R, a, b, wn, X, hi, iw, add);
        return;
    }
    const int last = X.m - 1;
    int ps[NI][2];
    long long s[NI][2][2];  // the sums at ps and ps + 1 of each end
    const long long qw = to_fx(wn);
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const bool whole = R[k].P2 < R[k].P3;
        const int cut = min(R[k].P1 + 1, R[k].P4);
        const int e0 = whole ? R[k].P2 : cut, s1 = whole ? R[k].P3 : cut;
        ps[k][0] = R[k].P1;
        ps[k][1] = s1;
        const int pn[2] = {e0 - R[k].P1, R[k].P4 - s1};  // 0 or 1
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int p = min(ps[k][e], last);
            const double ov = fmin(b[k], hi[p]) - fmax(a[k], X.v[p]);
            const long long q = (pn[e] > 0 && ov > 0.0) ? to_fx(wn * ov * iw[p]) : 0;
            // the whole run's entries: +qw at P2 = P1 + pn[0], -qw at P3 = s1
            const long long w0 = !whole ? 0 : (e ? -qw : (pn[0] == 0 ? qw : 0));
            const long long w1 = (whole && e == 0 && pn[0] == 1) ? qw : 0;
            s[k][e][0] = q + w0;
            s[k][e][1] = w1 - q;
        }
    }
#pragma unroll
    for (int k = 0; k < NI; ++k)
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (s[k][e][i] != 0 && ps[k][e] + i < X.m) add(ps[k][e] + i, s[k][e][i]);
}

}  // namespace lfg
