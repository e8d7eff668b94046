// lfg_corner.hpp -- the rules of a corner plot's data (MODEL_SPEC.md section
// 16) that the gfx950 kernels (lfg_corner.hip) and the host twin
// (cpu_baseline/lfg_cpu_corner.cpp, through the cpu_baseline shim) must agree
// on: which columns are immobile, numpy's bin edges, the bin of a value, the
// numbering of the pairs and the contour level of a fraction.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lfg_corner.h"

// No fused multiply-add anywhere below (nor in the unit that includes this
// last): np.linspace's edge is i * step rounded, then + lo rounded.
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace lfg {

__host__ __device__ inline bool corner_finite(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return ((u >> 52) & 0x7ff) != 0x7ff;
}

// A column's binning: its range, the step of its edges and whether it moves.
// Immobile: a bound that is not finite, hi <= lo, or a width hi - lo that is
// not finite (numpy cannot form edges for it either).
struct CornerCol {
    double lo, hi, step;
    int mobile;
};

__host__ __device__ inline CornerCol corner_col(double lo, double hi, int nb)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    CornerCol c;
    c.lo = lo;
    c.hi = hi;
    c.step = (hi - lo) / double(nb);
    c.mobile = corner_finite(lo) && corner_finite(hi) && hi > lo && corner_finite(hi - lo);
    return c;
}

// np.linspace(lo, hi, nb + 1)[i]: i * step + lo in two roundings, the last
// edge hi itself
__host__ __device__ inline double corner_edge(const CornerCol& c, int nb, int i)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (i >= nb) return c.hi;
    const double t = double(i) * c.step;
    return t + c.lo;
}

// The bin of x in a mobile column, -1 when x is not used: the largest i < nb
// with e[i] <= x (searchsorted(e, x, 'right') - 1, x == hi in the last bin).
// The guess is within one bin where the edges are distinct; a range a few ulp
// wide repeats edges, and the walk then goes as far as it must.
__host__ __device__ inline int corner_bin(const CornerCol& c, int nb, double x)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (!corner_finite(x) || !(x >= c.lo && x <= c.hi)) return -1;
    const double g = (x - c.lo) / (c.hi - c.lo) * double(nb);
    int i = g >= double(nb - 1) ? nb - 1 : (g > 0.0 ? int(g) : 0);
    while (i + 1 < nb && corner_edge(c, nb, i + 1) <= x) ++i;
    while (i > 0 && corner_edge(c, nb, i) > x) --i;
    return i;
}

// pairs (a, b), a < b < K, numbered (0,1), (0,2), ..., (K-2,K-1)
__host__ __device__ inline int corner_pair_count(int K) { return K * (K - 1) / 2; }

__host__ __device__ inline int corner_pair_index(int K, int a, int b) { return a * (2 * K - a - 1) / 2 + (b - a - 1); }

__host__ __device__ inline void corner_pair_of(int K, int p, int& a, int& b)
{
    a = 0;
    while (p >= K - 1 - a) {
        p -= K - 1 - a;
        ++a;
    }
    b = a + 1 + p;
}

// does position m of the descending counts, whose running sum is cum, lie
// inside fraction f?  One IEEE division, as numpy's sm /= sm[-1] gives.
// (total = 0: 0 / 0 is NaN, no position qualifies.)
__host__ __device__ inline bool corner_level_inside(long long cum, long long total, double f)
{
    return double(cum) / double(total) <= f;
}

// the argument checks both sides make before anything runs
__host__ inline bool corner_view_ok(long long steps, long long W, int row_len, long long step_ld, long long walker_ld,
                                    const int* cols, int K, int nb)
{
    if (steps < 0 || W < 0 || row_len < 1 || step_ld < 1 || walker_ld < 1) return false;
    if (K < 1 || K > LFG_CORNER_MAX_K || nb < 1 || nb > LFG_CORNER_MAX_BINS || !cols) return false;
    for (int i = 0; i < K; ++i) {
        if (cols[i] < 0 || cols[i] >= row_len) return false;
        for (int j = 0; j < i; ++j)
            if (cols[j] == cols[i]) return false;
    }
    return true;
}

__host__ inline bool corner_fracs_ok(const double* fracs, int nl)
{
    if (nl < 1 || nl > LFG_CORNER_MAX_LEVELS || !fracs) return false;
    for (int i = 0; i < nl; ++i)
        if (!(fracs[i] >= 0.0 && fracs[i] <= 1.0)) return false;
    return true;
}

}  // namespace lfg
