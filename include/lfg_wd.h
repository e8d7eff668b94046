/*
 * lfg_wd.h -- white-dwarf atmosphere fit (MODEL_SPEC.md section 13; the
 * reference's wdparams_new.py): ln_prob of (teff, logg, plax, ebv) against
 * observed white-dwarf fluxes through the Bergeron DA magnitude tables, and
 * one stretch-move half-step on it in one launch.
 *
 * A header of its own: include/lfg.h's function set is pinned by the ABI
 * tests.  Return and status codes are lfg.h's (LFG_OK, LFG_E_*, LFG_ST_*).
 */
#ifndef LFG_WD_H
#define LFG_WD_H

#include <stddef.h>

#include "lfg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LFG_WD_NPAR       4    /* teff [K], logg, plax [mas], ebv */
#define LFG_WD_MAX_BANDS  8
#define LFG_WD_MAX_KNOTS  128  /* FITPACK knots per axis of any spline here */

/*
 * The model, packed by the host (lfit_python_amd/wdparams.py).  Passed by
 * HOST pointer; the arrays it names are [dev] for lfg_wd_* and host arrays
 * for lfg_cpu_wd_lnprob.
 *   B            observed bands, 1 .. LFG_WD_MAX_BANDS
 *   tx, ty, c    the bands' absolute magnitudes M_b(logg, teff): FITPACK
 *                bicubics over one knot pair, tx (logg axis, nx knots) and ty
 *                (teff axis, ny knots), 8 .. LFG_WD_MAX_KNOTS each, and
 *                coefficients c[B][(nx - 4)][(ny - 4)]
 *   ctx, cty, cc per band, all three NULL for a band without a colour
 *                correction: the bicubic C_b(teff, logg), knots ctx (TEFF
 *                axis, cnx[b]) and cty (logg axis, cny[b]), coefficients
 *                [(cnx - 4)][(cny - 4)]
 *   k            extinction coefficient: m_b = M_b + 5 log10(d / 10) + k_b ebv
 *   mag, err     observed magnitude 2.5 log10(3631e3 / flux) and the flux
 *                error [mJy], err > 0
 *   lnnorm       sum_b ln(2 pi err_b^2)
 *   prior_*      Prior.ln_prob of the four parameters: type, p1, p2 as
 *                lfg_tree's, and lfg.h's constants of lfg_tree.prior_c:
 *                gauss, gaussPos c0 = -ln(sqrt(2 pi) p2), c1 = 1 / p2;
 *                uniform c0 = ln(1 / |p1 - p2|); log_uniform, mod_jeff
 *                c0 = -ln(normalise)
 */
typedef struct lfg_wd_model {
    int B;
    int nx, ny;
    const double* tx;
    const double* ty;
    const double* c;
    int cnx[LFG_WD_MAX_BANDS], cny[LFG_WD_MAX_BANDS];
    const double* ctx[LFG_WD_MAX_BANDS];
    const double* cty[LFG_WD_MAX_BANDS];
    const double* cc[LFG_WD_MAX_BANDS];
    double k[LFG_WD_MAX_BANDS], mag[LFG_WD_MAX_BANDS], err[LFG_WD_MAX_BANDS];
    double lnnorm;
    int prior_type[LFG_WD_NPAR];
    double prior_p1[LFG_WD_NPAR], prior_p2[LFG_WD_NPAR], prior_c0[LFG_WD_NPAR], prior_c1[LFG_WD_NPAR];
} lfg_wd_model;

/*
 * theta    [dev] row i is the four doubles at theta + i * ld (ld >= 4: a chain
 *          [rows][ld] is read in place)
 * model    HOST pointer
 * lnp      [dev] n: ln_prior, plus ln_like where ln_prior is finite
 * lnlike   [dev] n, nullable: -0.5 (lnnorm + chisq); -inf where lnp is -inf
 * mags     [dev] [B][n], nullable: the apparent model magnitudes m_b (+inf for
 *          plax <= 0; NaN for a LFG_ST_BAD_ARGS row)
 * status   [dev] n, nullable: LFG_ST_OK, or LFG_ST_BAD_ARGS for a row with a
 *          non-finite parameter (lnp = -inf)
 * Every element of every non-null output is written.  Asynchronous on
 * stream, re-entrant, allocates nothing, needs no workspace.  LFG_E_ARGS (and
 * no launch) for a null required pointer, n < 0, ld < 4 or a model beyond
 * the limits above; n = 0 returns LFG_OK.
 */
int lfg_wd_lnprob(const double* theta, size_t ld, int n, const lfg_wd_model* model, double* lnp,
                  double* lnlike, double* mags, int* status, void* stream);

/*
 * One stretch-move half-step of W walkers [W][4] in ONE launch, one lane per
 * walker of the half: lfg_stretch_propose's draws and arithmetic, the
 * model's ln_prob, lfg_stretch_accept's draw and rule.  A lane reads only
 * rows of the other half and writes only its own walker's.  pos, lnp,
 * naccept (nullable), q [W/2][4], zfac [W/2] and lnp_new [W/2] are left
 * bit-identical to lfg_stretch_propose -> lfg_wd_lnprob -> lfg_stretch_accept.
 * stepp: nullable [dev] step counter read instead of `step`.
 * LFG_E_ARGS for W < 4 or odd, half not 0 or 1, a <= 1, a null pointer
 * (other than stepp, naccept) or a model beyond the limits.
 */
int lfg_wd_step_half(double* pos, double* lnp, int W, int half, double a, unsigned long long seed,
                     unsigned long long step, const unsigned long long* stepp, const lfg_wd_model* model,
                     double* q, double* zfac, double* lnp_new, int* naccept, void* stream);

#ifdef __cplusplus
}
#endif
#endif
