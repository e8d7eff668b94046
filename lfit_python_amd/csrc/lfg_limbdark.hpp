// lfg_limbdark.hpp -- one (logg, teff) row to its 25 limb-darkening
// coefficients (MODEL_SPEC.md section 15; the reference's limbdark.py ld()).
// Shared by the gfx950 kernel (lfg_limbdark.hip, tables in LDS) and the host
// twin (cpu_baseline/lfg_cpu_limbdark.cpp, through the cpu_baseline shim).
// FITPACK's bicubic evaluation is lfg_physpar.hpp's (pp_knot_interval,
// pp_bspl).  FP64, no arrays indexed at run time: nothing here needs scratch.
#pragma once
#include "lfg_limbdark.h"
#include "lfg_physpar.hpp"

namespace lfg {

constexpr int ST_LD_CLAMPED = LFG_ST_LD_CLAMPED;

// the limits of lfg_limbdark.h (the kernel and the twin index by these counts alone)
__host__ __device__ inline bool ld_tables_ok(const lfg_ld_tables* t)
{
    if (!t || !t->tx || !t->ty || !t->c) return false;
    return t->nx >= 8 && t->nx <= LFG_LD_MAX_KNOTS && t->ny >= 8 && t->ny <= LFG_LD_MAX_KNOTS;
}

// One row.  tx, ty, c: lfg_ld_tables' arrays, wherever they lie.  The knot
// interval and the four basis values of each axis are computed once; the 25
// surfaces' 4 x 4 contractions reuse them.  Returns the status.
__device__ inline int limbdark_row(const double* tx, int nx, const double* ty, int ny, const double* c, double logg,
                                   double teff, double out[LFG_LD_NCOL])
{
    if (!isfinite(logg) || !isfinite(teff)) {
#pragma unroll
        for (int s = 0; s < LFG_LD_NCOL; ++s) out[s] = NAN;
        return ST_BAD_ARGS;
    }
    const bool outside = logg < tx[3] || logg > tx[nx - 4] || teff < ty[3] || teff > ty[ny - 4];
    double hx[4], hy[4];
    const int lx = pp_knot_interval(tx, nx, logg);
    const int ly = pp_knot_interval(ty, ny, teff);
    pp_bspl(tx, lx, logg, hx);
    pp_bspl(ty, ly, teff, hy);
    const int nky = ny - 4, nk = (nx - 4) * nky;
    const double* c0 = c + (lx - 3) * nky + (ly - 3);
#pragma unroll
    for (int s = 0; s < LFG_LD_NCOL; ++s) {
        const double* cs = c0 + s * nk;
        double z = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double zi = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) zi = fma(cs[i * nky + j], hy[j], zi);
            z = fma(hx[i], zi, z);
        }
        out[s] = z;
    }
    return outside ? ST_LD_CLAMPED : ST_OK;
}

}  // namespace lfg
