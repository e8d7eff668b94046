/*
 * lfg_limbdark.h -- the white dwarf's limb-darkening coefficients per band
 * from (logg, teff) rows (MODEL_SPEC.md section 15; the reference's
 * limbdark.py ld(), the tables of Gianninas et al. 2013).
 *
 * A header of its own: include/lfg.h's function set is pinned by the ABI
 * tests, and this entry point shares none of its workspace conventions.  The
 * status codes are lfg.h's LFG_ST_* plus LFG_ST_LD_CLAMPED below.
 *
 * Per row, 25 bicubic splines that share their knots are evaluated at
 * (logg, teff): five bands (u, g, r, i, z), five coefficients each (linear,
 * quadratic a and b, square-root d and f).
 */
#ifndef LFG_LIMBDARK_H
#define LFG_LIMBDARK_H

#include <stddef.h>

#include "lfg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* logg or teff outside the knot span: the row holds the value at the clamped
 * argument, which is what the reference returns */
#define LFG_ST_LD_CLAMPED 7

#define LFG_LD_NBAND 5  /* u, g, r, i, z in that order */
#define LFG_LD_NCOEF 5  /* linear, quad a, quad b, sqr d, sqr f: table columns 2 ... 6 */
#define LFG_LD_NCOL  25 /* column band * LFG_LD_NCOEF + coef */
#define LFG_LD_MAX_KNOTS 64 /* knots per axis: 8 ... 64 */

/*
 * The tables, packed by the host (lfit_python_amd/limbdark.py).  Pointers are
 * [dev] for lfg_limbdark and host pointers for lfg_cpu_limbdark.
 *   tx, ty   FITPACK knots of the bicubic splines z(logg, teff), shared by
 *            all surfaces: nx and ny of them (8 .. LFG_LD_MAX_KNOTS), not
 *            decreasing, with t[3] < t[n - 4]
 *   c        [LFG_LD_NCOL][(nx - 4)(ny - 4)]: surface `col`'s coefficients,
 *            logg-major
 */
typedef struct lfg_ld_tables {
    const double* tx;
    const double* ty;
    int nx, ny;
    const double* c;
} lfg_ld_tables;

/*
 * logg, teff   [dev] row i at element i * ld (ld >= 1: the columns of a chain
 *              [rows][ndim] are read in place with ld = ndim, a thinned chain
 *              with ld = thin * ndim)
 * tab          HOST pointer to the struct; the arrays it names are [dev]
 * out          [dev] [n][LFG_LD_NCOL] row-major: out[i * LFG_LD_NCOL + col]
 * status       [dev] n
 * Every element of out and status is written.  Status, first match:
 *   LFG_ST_BAD_ARGS     a non-finite logg or teff; the row is all NaN
 *   LFG_ST_LD_CLAMPED   logg outside [tx[3], tx[nx-4]] or teff outside
 *                       [ty[3], ty[ny-4]]; the row is the value at the
 *                       argument clamped to that span
 *   LFG_ST_OK
 * Asynchronous on stream, re-entrant, allocates nothing and needs no
 * workspace.  LFG_E_ARGS (and no launch) for a null pointer, n < 0, ld < 1 or
 * knots beyond the limits above; n = 0 returns LFG_OK.
 */
int lfg_limbdark(const double* logg, const double* teff, size_t ld, int n, const lfg_ld_tables* tab,
                 double* out, int* status, void* stream);

/* lanes of one launch: rows beyond it take further trips of the grid-stride loop */
int lfg_limbdark_lanes(void);

#ifdef __cplusplus
}
#endif
#endif
