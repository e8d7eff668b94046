// lfg_chain.hpp -- the rules of a chain's summary (MODEL_SPEC.md section 14)
// that the gfx950 kernels (lfg_chain.hip) and the host twin
// (cpu_baseline/lfg_cpu_chain.cpp, through the cpu_baseline shim) must agree
// on: the order-preserving key of a double, the rank and interpolation rule
// of a quantile, the two sweeps of the moments and how their partial results
// combine, Welford's and Chan's forms for the walkers, the clip rule and R-hat
// from the per-walker moments.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lfg_chain.h"

// No fused multiply-add anywhere below (nor in the unit that includes this
// last): numpy's quantile weight is f * (n - 1) rounded, then the difference.
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace lfg {

// A double's key: unsigned keys order as the doubles do (-0.0 just below
// +0.0).  All bits of a negative are flipped, the sign bit of the rest.
__host__ __device__ inline uint64_t chain_key(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__host__ __device__ inline double chain_unkey(uint64_t k)
{
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    __builtin_memcpy(&x, &u, 8);
    return x;
}

__host__ __device__ inline bool chain_finite(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return ((u >> 52) & 0x7ff) != 0x7ff;
}

// used: finite and inside the window (inclusive)
__host__ __device__ inline bool chain_used(double x, double lo, double hi) { return chain_finite(x) && x >= lo && x <= hi; }

// numpy's and pandas' 'linear' quantile of n >= 1 sorted values: the ranks
// lo and hi whose values a and b it interpolates, and the weight g
__host__ __device__ inline void chain_rank(double f, long long n, long long& lo, long long& hi, double& g)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double pos = f * double(n - 1);
    double fl = floor(pos);
    if (fl > double(n - 1)) fl = double(n - 1);
    if (fl < 0.0) fl = 0.0;
    lo = (long long)fl;
    hi = lo + 1 < n ? lo + 1 : n - 1;
    g = pos - fl;
}

__host__ __device__ inline double chain_lerp(double a, double b, double g)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double d = b - a;
    return g < 0.5 ? a + d * g : b - d * (1.0 - g);
}

// A compensated sum (Neumaier): s + c is the sum of what was added, to about
// one rounding.  An overflowed sum stays +-inf in s (c is then meaningless:
// chain_sum_value looks at s first).
__host__ __device__ inline void chain_sum_add(double& s, double& c, double x)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double t = s + x;
    c += fabs(s) >= fabs(x) ? (s - t) + x : (x - t) + s;
    s = t;
}

__host__ __device__ inline void chain_sum_merge(double& s, double& c, double sb, double cb)
{
    chain_sum_add(s, c, sb);
    c += cb;
}

__host__ __device__ inline double chain_sum_value(double s, double c) { return chain_finite(s) ? s + c : s; }

// The first sweep's state of a set of values: the count, the non-finite
// count, the compensated sum and the extremes
struct ChainMom {
    long long n, bad;
    double sum, comp, lo, hi;
};

__host__ __device__ inline ChainMom chain_mom_empty()
{
    ChainMom a;
    a.n = 0;
    a.bad = 0;
    a.sum = 0.0;
    a.comp = 0.0;
    a.lo = INFINITY;
    a.hi = -INFINITY;
    return a;
}

__host__ __device__ inline void chain_mom_add(ChainMom& a, double x)
{
    a.n += 1;
    chain_sum_add(a.sum, a.comp, x);
    a.lo = fmin(a.lo, x);
    a.hi = fmax(a.hi, x);
}

__host__ __device__ inline void chain_mom_merge(ChainMom& a, const ChainMom& b)
{
    a.n += b.n;
    a.bad += b.bad;
    chain_sum_merge(a.sum, a.comp, b.sum, b.comp);
    a.lo = fmin(a.lo, b.lo);
    a.hi = fmax(a.hi, b.hi);
}

__host__ __device__ inline double chain_mean(const ChainMom& a)
{
    return a.n ? chain_sum_value(a.sum, a.comp) / double(a.n) : NAN;
}

// The second sweep: with d = x - mean, s1 = sum d (plain) and (s2, c2) = sum
// d^2 (compensated); m2 = s2 - s1^2 / n, the corrected two-pass form
struct ChainDev {
    double s1, s2, c2;
};

__host__ __device__ inline void chain_dev_add(ChainDev& a, double x, double mean)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double d = x - mean;
    a.s1 += d;
    chain_sum_add(a.s2, a.c2, d * d);
}

__host__ __device__ inline void chain_dev_merge(ChainDev& a, const ChainDev& b)
{
    a.s1 += b.s1;
    chain_sum_merge(a.s2, a.c2, b.s2, b.c2);
}

__host__ __device__ inline double chain_m2(const ChainDev& a, long long n)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (n < 1) return NAN;
    if (!chain_finite(a.s2)) return a.s2;  // the squares overflowed
    return fmax(chain_sum_value(a.s2, a.c2) - a.s1 * (a.s1 / double(n)), 0.0);
}

// Welford's update of (n, mean, m2) with one value: a walker's moments for R-hat
__host__ __device__ inline void chain_pair_add(double& n, double& mean, double& m2, double x)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    n += 1.0;
    const double d = x - mean;
    mean += d / n;
    m2 += d * (x - mean);
}

// Chan's combination of two (n, mean, m2)
__host__ __device__ inline void chain_pair_merge(double& na, double& ma, double& sa, double nb, double mb, double sb)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (nb == 0.0) return;
    if (na == 0.0) {
        na = nb;
        ma = mb;
        sa = sb;
        return;
    }
    const double nt = na + nb, d = mb - ma;
    ma += d * (nb / nt);
    sa += sb + d * d * (na * nb / nt);
    na = nt;
}

// the next window of a sigma clip; false: the window stays
__host__ __device__ inline bool chain_clip(long long n, double m2, double med, double sigma, double& lo, double& hi)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (n < 1) return false;
    const double sd = sqrt(m2 / double(n));
    if (!chain_finite(sd) || !chain_finite(med)) return false;
    const double w = sigma * sd;
    lo = fmax(lo, med - w);
    hi = fmin(hi, med + w);
    return true;
}

// Gelman-Rubin from m walkers of n steps each: between = sum over walkers of
// (walker mean - mean of the walker means)^2, within = sum of the walkers' m2
__host__ __device__ inline double chain_rhat(long long m, long long n, double between, double within)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (m < 2 || n < 2) return NAN;
    const double dm = double(m), dn = double(n);
    const double B = between / (dm - 1.0);
    const double Wv = within / (dm * (dn - 1.0));
    const double sigma2 = (dn - 1.0) / dn * Wv + B;
    return (dm + 1.0) * sigma2 / (dm * Wv) - (dn - 1.0) / (dm * dn);
}

// the argument checks both sides make before anything runs
__host__ inline bool chain_view_ok(long long steps, long long W, int C, long long step_ld, long long walker_ld)
{
    return steps >= 0 && W >= 0 && C >= 1 && C <= LFG_CHAIN_MAX_C && step_ld >= 1 && walker_ld >= 1;
}

__host__ inline bool chain_fracs_ok(const double* fracs, int nq)
{
    if (nq < 0 || nq > LFG_CHAIN_MAX_NQ || (nq > 0 && !fracs)) return false;
    for (int i = 0; i < nq; ++i)
        if (!(fracs[i] >= 0.0 && fracs[i] <= 1.0)) return false;
    return true;
}

}  // namespace lfg
