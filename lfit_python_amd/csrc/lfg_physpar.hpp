// lfg_physpar.hpp -- one chain row to its physical parameters (MODEL_SPEC.md
// section 12; the reference's calcPhysicalParams.py solve()).  Shared by the
// gfx950 kernel (lfg_physpar.hip, tables in LDS) and the host twin
// (cpu_baseline/lfg_cpu_physpar.cpp, through the cpu_baseline shim).  FP64,
// no recursion, no arrays indexed at run time: nothing here needs scratch.
#pragma once
#include "lfg_device.hpp"
#include "lfg_physpar.h"

namespace lfg {

constexpr int ST_NO_MR_SOLUTION = LFG_ST_NO_MR_SOLUTION;
constexpr int PP_MAXIT = 400;  // pp_root's cap: the bracket halves at least every six steps
// the reference's brackets (find_wdmass), in the cascade's order
constexpr double PP_WOOD_LO = 0.4, PP_WOOD_HI = 1.0;
constexpr double PP_PANEI_LO = 0.4, PP_PANEI_HI = 1.2;
constexpr double PP_HAMADA_LO = 0.14, PP_HAMADA_HI = 1.44;
constexpr double PP_PANEI_TLO = 5000.0, PP_PANEI_THI = 45000.0;  // panei_mr's assertion
// logg()'s own constants (cgs), not the tables'
constexpr double PP_LOGG_G = 6.67384e-8, PP_LOGG_MSUN = 1.9891e33, PP_LOGG_RSUN = 6.95508e10;

// np.interp / interp1d(kind='linear') over x increasing, clamped at the ends
__device__ inline double pp_interp(const double* x, const double* y, int n, double v)
{
    if (v <= x[0]) return y[0];
    if (v >= x[n - 1]) return y[n - 1];
    int lo = 0, hi = n - 1;  // x[lo] <= v < x[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] <= v) lo = mid; else hi = mid;
    }
    return fma((y[lo + 1] - y[lo]) / (x[lo + 1] - x[lo]), v - x[lo], y[lo]);
}

// FITPACK fpbisp's argument handling: x clamped into [t[3], t[n-4]], and the
// interval l, 3 <= l <= n-5, with t[l] <= x < t[l+1] (the last one closed)
__device__ inline int pp_knot_interval(const double* t, int n, double& x)
{
    x = fmin(fmax(x, t[3]), t[n - 4]);
    int l = 3;
    while (l < n - 5 && x >= t[l + 1]) ++l;
    return l;
}

// FITPACK fpbspl, k = 3: the four cubic B-splines that are non-zero on
// [t[l], t[l+1]] (de Boor - Cox)
__device__ inline void pp_bspl(const double* t, int l, double x, double h[4])
{
    double hh[3];
    h[0] = 1.0;
#pragma unroll
    for (int j = 1; j <= 3; ++j) {
#pragma unroll
        for (int i = 0; i < j; ++i) hh[i] = h[i];
        h[0] = 0.0;
#pragma unroll
        for (int i = 1; i <= j; ++i) {
            const double thi = t[l + i], tlo = t[l + i - j];
            const double f = hh[i - 1] / (thi - tlo);
            h[i - 1] = fma(f, thi - x, h[i - 1]);
            h[i] = f * (x - tlo);
        }
    }
}

// what a row keeps for its model radii: the seven Wood radii at its
// temperature and the Panei spline's T side
struct PPRow {
    double rk[LFG_MR_NWOOD];
    double hx[4];
    int lx;
    double rw_a, K;  // geo(m) = rw_a cbrt(K m) / Rsun
};

// Wood: sum_k r_k(T) L_k(m), the cardinal cubics of interp1d(kind='cubic')
__device__ inline double pp_wood(const lfg_mr_tables& V, const PPRow& W, double m)
{
    const int j = min(max(int((m - PP_WOOD_LO) * 10.0), 0), LFG_MR_NWOOD - 2);
    const double d = m - double(j + 4) / 10.0;  // the knot 0.4 + 0.1 j as numpy holds it
    const double* c = V.wood_card + j * (LFG_MR_NWOOD * 4);
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
#pragma unroll
    for (int k = 0; k < LFG_MR_NWOOD; ++k) {
        c0 = fma(W.rk[k], c[4 * k + 0], c0);
        c1 = fma(W.rk[k], c[4 * k + 1], c1);
        c2 = fma(W.rk[k], c[4 * k + 2], c2);
        c3 = fma(W.rk[k], c[4 * k + 3], c3);
    }
    return fma(fma(fma(c3, d, c2), d, c1), d, c0);
}

// Panei: the bicubic spline (tx, ty, c) at (T, m), T's basis kept in the row
__device__ inline double pp_panei(const lfg_mr_tables& V, const PPRow& W, double m)
{
    double hy[4];
    const int ly = pp_knot_interval(V.pan_ty, V.pan_ny, m);
    pp_bspl(V.pan_ty, ly, m, hy);
    const int nky = V.pan_ny - 4;
    const double* c = V.pan_c + (W.lx - 3) * nky + (ly - 3);
    double z = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double zi = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) zi = fma(c[i * nky + j], hy[j], zi);
        z = fma(W.hx[i], zi, z);
    }
    return z;
}

// f(m) = geo(m) - R_model(m), R_sun
__device__ inline double pp_f(const lfg_mr_tables& V, const PPRow& W, int model, double m)
{
    const double geo = W.rw_a * cbrt(W.K * m) / V.Rsun;
    double r;
    if (model == LFG_MR_WOOD) r = pp_wood(V, W, m);
    else if (model == LFG_MR_PANEI) r = pp_panei(V, W, m);
    else r = pp_interp(V.ham_m, V.ham_r, V.n_ham, m);
    return geo - r;
}

// The root of f in [a, b], fa fb <= 0: the secant through the bracket's ends
// (regula falsi) with the Illinois weight, the bracket kept.  A step that
// leaves the bracket is replaced by bisection, and so is every step after
// four that did not halve the bracket: it halves at least every six steps,
// so PP_MAXIT steps bring any bracket below an ulp.  Ends when f is 0, when
// a step moves by less than an ulp of b, or when the bracket is two ulp
// wide: the root's error is then f's own rounding over f'.
__device__ inline double pp_root(const lfg_mr_tables& V, const PPRow& W, int model, double a, double b, double fa,
                                 double fb)
{
    if (fa == 0.0) return a;
    if (fb == 0.0) return b;
    const bool up = fb > 0.0;
    const double ulp = 2.3e-16 * b;
    int side = 0, stall = 0;
    double wref = b - a, xprev = a;
    for (int it = 0; it < PP_MAXIT; ++it) {
        const double w = b - a;
        if (w <= 2.0 * ulp) break;
        if (w <= 0.5 * wref) { wref = w; stall = 0; } else ++stall;
        double x = b - fb * (w / (fb - fa));
        if (!(x > a && x < b) || stall > 4) x = a + 0.5 * w;
        if (!(x > a && x < b)) break;  // a and b are neighbours
        const double fx = pp_f(V, W, model, x);
        if (fx == 0.0 || (it > 0 && fabs(x - xprev) <= ulp)) return x;
        xprev = x;
        if ((fx > 0.0) == up) {
            b = x;
            fb = fx;
            if (side == 1) fa *= 0.5;
            side = 1;
        } else {
            a = x;
            fa = fx;
            if (side == -1) fb *= 0.5;
            side = -1;
        }
    }
    return (fabs(fa) <= fabs(fb)) ? a : b;
}

// findi_fast ends on a Newton step of at most TH_LAST = 1e-6 of its 2-D
// tangency system, which is nearly singular in cos i towards i = 90 degrees:
// what is left of dphi is below 1e-12, but of the inclination up to 1.5e-9
// degrees at i = 89, over the 1e-9 degrees this section promises.  One Newton
// step on findi's own h(cos i) from there; a step that is not small (h is
// even in cos i: no slope at 90 degrees) is not taken.
__device__ inline double pp_polish_inc(const Roche& R, double dphi, double inc_deg)
{
    double sth, cth;
    sincos(PI * dphi, &sth, &cth);
    const double c = cos(inc_deg * DEG);
    double tw = -1.0, h, dh;
    if (!h_eval(R, cth, sth, c, tw, h, dh) || !(dh != 0.0)) return inc_deg;
    const double step = h / dh, cn = c - step;
    if (!(fabs(step) <= 1e-9) || !(cn >= 0.0 && cn < 1.0)) return inc_deg;
    return acos(cn) / DEG;
}

// One row.  out: the LFG_PP_* columns; returns the status (lfg_physpar.h's
// order of rules) and the model that gave the mass (-1: none).
__device__ inline int physpar_row(const lfg_mr_tables& V, double q, double dphi, double rw, double T, double P,
                                  double out[LFG_PP_NCOL], int& model)
{
    model = -1;
#pragma unroll
    for (int c = 0; c < LFG_PP_NCOL; ++c) out[c] = NAN;
    if (!isfinite(q) || !isfinite(dphi) || !isfinite(rw) || !isfinite(T) || !isfinite(P) || !(rw > 0.0) ||
        !(T > 0.0) || !(P > 0.0))
        return ST_BAD_ARGS;
    Roche R;
    if (roche_init(R, q) != ST_OK) return ST_BAD_Q;

    PPRow W;
    const double Ps = P * V.day;
    const double S = V.G * (1.0 + q) * Ps * Ps / (4.0 * PI * PI);  // a^3 / M_wd, SI
    W.K = S * (V.GMsun / V.G);
    W.rw_a = rw * R.xl1;
#pragma unroll
    for (int k = 0; k < LFG_MR_NWOOD; ++k) {
        const int o = V.wood_off[k];
        W.rk[k] = pp_interp(V.wood_t + o, V.wood_r + o, V.wood_off[k + 1] - o, T);
    }
    const bool gate = T >= PP_PANEI_TLO && T < PP_PANEI_THI;
    W.lx = 3;
    W.hx[0] = W.hx[1] = W.hx[2] = W.hx[3] = 0.0;
    if (gate) {
        double Tc = T;
        W.lx = pp_knot_interval(V.pan_tx, V.pan_nx, Tc);
        pp_bspl(V.pan_tx, W.lx, Tc, W.hx);
    }

    // the cascade: the first model whose bracket holds a sign change
    double lo = 0.0, hi = 0.0, flo = 0.0, fhi = 0.0;
    for (int k = LFG_MR_WOOD; k <= LFG_MR_HAMADA && model < 0; ++k) {
        if (k == LFG_MR_PANEI && !gate) continue;
        lo = k == LFG_MR_WOOD ? PP_WOOD_LO : k == LFG_MR_PANEI ? PP_PANEI_LO : PP_HAMADA_LO;
        hi = k == LFG_MR_WOOD ? PP_WOOD_HI : k == LFG_MR_PANEI ? PP_PANEI_HI : PP_HAMADA_HI;
        flo = pp_f(V, W, k, lo);
        fhi = pp_f(V, W, k, hi);
        if (!(flo * fhi > 0.0)) model = k;
    }
    if (model < 0) return ST_NO_MR_SOLUTION;
    const double Mw = pp_root(V, W, model, lo, hi, flo, fhi);

    double inc = 0.0;
    if (findi_fast(R, dphi, inc) != ST_OK) {
        model = -1;
        return ST_BAD_DPHI;
    }
    inc = pp_polish_inc(R, dphi, inc);
    const double a = cbrt(W.K * Mw) / V.Rsun;  // R_sun
    const double Rw = W.rw_a * a;
    const double Rcm = Rw * PP_LOGG_RSUN;
    const double Kw = TWO_PI * sin(inc * DEG) * q * (a * V.Rsun) / ((1.0 + q) * Ps) * 1e-3;  // km/s
    out[LFG_PP_Q] = q;
    out[LFG_PP_MW] = Mw;
    out[LFG_PP_RW] = Rw;
    out[LFG_PP_LOGG] = log10(PP_LOGG_G * (Mw * PP_LOGG_MSUN) / (Rcm * Rcm));
    out[LFG_PP_MR] = q * Mw;
    out[LFG_PP_RR] = a * eggleton(q);
    out[LFG_PP_A] = a;
    out[LFG_PP_KW] = Kw;
    out[LFG_PP_KR] = Kw / q;
    out[LFG_PP_INCL] = inc;
    return ST_OK;
}

}  // namespace lfg
