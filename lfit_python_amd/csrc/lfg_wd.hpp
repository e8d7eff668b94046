// lfg_wd.hpp -- ln_prob of one (teff, logg, plax, ebv) row of the white-dwarf
// atmosphere fit (MODEL_SPEC.md section 13; the reference's wdparams_new.py).
// Shared by the gfx950 kernels (lfg_wd.hip) and the host twin
// (cpu_baseline/lfg_cpu_wd.cpp, through the cpu_baseline shim).  FP64, every
// fused multiply-add spelled out and contraction off, so that the text gives
// the same bits wherever it is inlined; no local array is indexed at run
// time: nothing here needs scratch.
#pragma once
#include "lfg_device.hpp"
#include "lfg_wd.h"

namespace lfg {

constexpr double WD_ZP = 3631e3;  // AB zero point [mJy]: F = ZP 10^(-0.4 m)

// FITPACK fpbisp's argument handling: x clamped into [t[3], t[n-4]] and the
// span l, 3 <= l <= n-5, with t[l] <= x < t[l+1] (the last one closed).  The
// knots are non-decreasing, so l is the largest index <= n-5 with t[l] <= x:
// a branch-free bisection, the same trips for every lane
__device__ inline int wd_span(const double* __restrict__ t, int n, double& x)
{
    x = fmin(fmax(x, t[3]), t[n - 4]);
    const int last = n - 5;
    int l = 3;
    for (int s = LFG_WD_MAX_KNOTS / 2; s >= 1; s >>= 1) {
        const int cnd = l + s;
        const double tc = t[min(cnd, last)];
        l = (cnd <= last && tc <= x) ? cnd : l;
    }
    return l;
}

// FITPACK fpbspl, k = 3: the four cubic B-splines that are non-zero on
// [t[l], t[l+1]] (de Boor - Cox), in registers
__device__ inline void wd_bspl(const double* __restrict__ t, int l, double x, double& h0, double& h1, double& h2,
                               double& h3)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double tm2 = t[l - 2], tm1 = t[l - 1], t0 = t[l], t1 = t[l + 1], t2 = t[l + 2], t3 = t[l + 3];
    // j = 1
    double f = 1.0 / (t1 - t0);
    double a0 = f * (t1 - x), a1 = f * (x - t0);
    // j = 2
    f = a0 / (t1 - tm1);
    double b0 = f * (t1 - x), b1 = f * (x - tm1);
    f = a1 / (t2 - t0);
    b1 = fma(f, t2 - x, b1);
    double b2 = f * (x - t0);
    // j = 3
    f = b0 / (t1 - tm2);
    h0 = f * (t1 - x);
    h1 = f * (x - tm2);
    f = b1 / (t2 - tm1);
    h1 = fma(f, t2 - x, h1);
    h2 = f * (x - tm1);
    f = b2 / (t3 - t0);
    h2 = fma(f, t3 - x, h2);
    h3 = f * (x - t0);
}

// sum_ij c[(lx-3+i) nky + (ly-3+j)] hx_i hy_j: 16 coefficients, read through the cache
__device__ inline double wd_tensor(const double* __restrict__ c, int nky, int lx, int ly, double hx0, double hx1,
                                   double hx2, double hx3, double hy0, double hy1, double hy2, double hy3)
{
    const double* r = c + (lx - 3) * nky + (ly - 3);
    double z = 0.0;
    const double hx[4] = {hx0, hx1, hx2, hx3};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double* ri = r + i * nky;
        const double zi = fma(ri[3], hy3, fma(ri[2], hy2, fma(ri[1], hy1, ri[0] * hy0)));
        z = fma(hx[i], zi, z);
    }
    return z;
}

// Prior.ln_prob of one parameter from lfg_wd_model's constants: the term and
// whether it is finite (MODEL_SPEC 8: open intervals; a Gaussian is -inf once
// the reference's pdf underflows, lfg.hip's prior-lane rule)
__device__ inline double wd_prior(int ty, double p1, double p2, double c0, double c1, double v, bool& ok)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (ty <= 1) {
        const double z = (v - p1) * c1;
        const double term = fma(-0.5 * z, z, c0);
        const double thr = (c1 > 1.0) ? PDF_LN_MIN + (c0 + LN_SQRT_2PI) : PDF_LN_MIN;
        ok = ok && term > thr && (ty == 0 || v > 0.0);
        return term;
    }
    if (ty == 2) {
        ok = ok && v > p1 && v < p2;
        return c0;
    }
    if (ty == 3) {
        ok = ok && v > p1 && v < p2;
        return c0 - log(v);
    }
    ok = ok && ty == 4 && v > 0.0 && v < p2;
    return c0 - log(v + p1);
}

// One row.  Returns ln_prob; lnlike = -0.5 (lnnorm + chisq), or -inf where
// ln_prob is -inf; sink(b, m_b) takes the apparent model magnitudes (NaN for
// a non-finite row); st the row's status.  The bands run in a rolled loop:
// the model's per-band fields are read by a wave-uniform index.
template <class Sink>
__device__ inline double wd_row(const lfg_wd_model& M, double teff, double logg, double plax, double ebv,
                                double& lnlike, int& st, Sink&& sink)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (!(isfinite(teff) && isfinite(logg) && isfinite(plax) && isfinite(ebv))) {
        for (int b = 0; b < M.B; ++b) sink(b, double(NAN));
        lnlike = -INFINITY;
        st = LFG_ST_BAD_ARGS;
        return -INFINITY;
    }
    st = LFG_ST_OK;
    bool ok = true;
    double lp = 0.0;
    lp += wd_prior(M.prior_type[0], M.prior_p1[0], M.prior_p2[0], M.prior_c0[0], M.prior_c1[0], teff, ok);
    lp += wd_prior(M.prior_type[1], M.prior_p1[1], M.prior_p2[1], M.prior_c0[1], M.prior_c1[1], logg, ok);
    lp += wd_prior(M.prior_type[2], M.prior_p1[2], M.prior_p2[2], M.prior_c0[2], M.prior_c1[2], plax, ok);
    lp += wd_prior(M.prior_type[3], M.prior_p1[3], M.prior_p2[3], M.prior_c0[3], M.prior_c1[3], ebv, ok);

    // the Bergeron bicubics share their knots: one span and one basis per axis
    double g = logg, t = teff;
    const int lx = wd_span(M.tx, M.nx, g), ly = wd_span(M.ty, M.ny, t);
    double gx0, gx1, gx2, gx3, ty0, ty1, ty2, ty3;
    wd_bspl(M.tx, lx, g, gx0, gx1, gx2, gx3);
    wd_bspl(M.ty, ly, t, ty0, ty1, ty2, ty3);
    const int nky = M.ny - 4, ncoef = (M.nx - 4) * nky;
    // d = 1000 / plax pc, +inf for plax <= 0: m = +inf and F = 0
    const double dmod = (plax > 0.0) ? 5.0 * log10((1000.0 / plax) / 10.0) : INFINITY;

    double chisq = 0.0;
#pragma unroll 1
    for (int b = 0; b < M.B; ++b) {
        const double Mb = wd_tensor(M.c + size_t(b) * ncoef, nky, lx, ly, gx0, gx1, gx2, gx3, ty0, ty1, ty2, ty3);
        const double mb = fma(M.k[b], ebv, Mb + dmod);
        sink(b, mb);
        double corr = 0.0;
        if (M.cc[b]) {  // C_b(teff, logg): the arguments the other way round
            double ct = teff, cg = logg;
            const int cx = wd_span(M.ctx[b], M.cnx[b], ct), cy = wd_span(M.cty[b], M.cny[b], cg);
            double a0, a1, a2, a3, e0, e1, e2, e3;
            wd_bspl(M.ctx[b], cx, ct, a0, a1, a2, a3);
            wd_bspl(M.cty[b], cy, cg, e0, e1, e2, e3);
            corr = wd_tensor(M.cc[b], M.cny[b] - 4, cx, cy, a0, a1, a2, a3, e0, e1, e2, e3);
        }
        const double F = WD_ZP * pow(10.0, -0.4 * mb);
        const double Fobs = WD_ZP * pow(10.0, -0.4 * (M.mag[b] + corr));
        const double r = (F - Fobs) / M.err[b];
        chisq = fma(r, r, chisq);
    }
    const double ll = -0.5 * (M.lnnorm + chisq);
    if (!ok) {
        lnlike = -INFINITY;
        return -INFINITY;
    }
    lnlike = ll;
    return lp + ll;
}

// the limits of lfg_wd.h; the kernels index by these counts alone
inline bool wd_model_ok(const lfg_wd_model* M)
{
    if (!M || M->B < 1 || M->B > LFG_WD_MAX_BANDS || !M->tx || !M->ty || !M->c) return false;
    if (M->nx < 8 || M->nx > LFG_WD_MAX_KNOTS || M->ny < 8 || M->ny > LFG_WD_MAX_KNOTS) return false;
    for (int b = 0; b < M->B; ++b) {
        const bool any = M->ctx[b] || M->cty[b] || M->cc[b], all = M->ctx[b] && M->cty[b] && M->cc[b];
        if (any != all) return false;
        if (all && (M->cnx[b] < 8 || M->cnx[b] > LFG_WD_MAX_KNOTS || M->cny[b] < 8 || M->cny[b] > LFG_WD_MAX_KNOTS))
            return false;
        if (!(M->err[b] > 0.0)) return false;
    }
    for (int d = 0; d < LFG_WD_NPAR; ++d)
        if (M->prior_type[d] < 0 || M->prior_type[d] > 4) return false;
    return true;
}

}  // namespace lfg
