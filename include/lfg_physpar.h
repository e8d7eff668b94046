/*
 * lfg_physpar.h -- physical parameters from chain rows (MODEL_SPEC.md
 * section 12; the reference's calcPhysicalParams.py solve()).
 *
 * A header of its own: include/lfg.h's function set is pinned by the ABI
 * tests, and this entry point shares none of its workspace conventions.  The
 * status codes are lfg.h's LFG_ST_* plus LFG_ST_NO_MR_SOLUTION below.
 *
 * Per row (q, dphi, rwd, twd [K], p [days]) the white-dwarf mass is the root
 * of  geo(m) - R_model(m)  in the first of the Wood 95 / Panei / Hamada-
 * Salpeter mass-radius relations whose bracket holds a sign change; the ten
 * derived columns follow (LFG_PP_* below, the reference's column order).
 */
#ifndef LFG_PHYSPAR_H
#define LFG_PHYSPAR_H

#include <stddef.h>

#include "lfg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* no mass-radius relation brackets a root (the reference returns None) */
#define LFG_ST_NO_MR_SOLUTION 6

/* output columns: out[c * n + i] */
#define LFG_PP_Q     0
#define LFG_PP_MW    1  /* M_sun */
#define LFG_PP_RW    2  /* R_sun */
#define LFG_PP_LOGG  3  /* cgs, the reference's legacy constants */
#define LFG_PP_MR    4  /* M_sun */
#define LFG_PP_RR    5  /* R_sun */
#define LFG_PP_A     6  /* R_sun */
#define LFG_PP_KW    7  /* km/s */
#define LFG_PP_KR    8  /* km/s */
#define LFG_PP_INCL  9  /* degrees */
#define LFG_PP_NCOL  10

/* model[i]: the relation that gave row i's mass, -1 for an unsolved row */
#define LFG_MR_WOOD    0
#define LFG_MR_PANEI   1
#define LFG_MR_HAMADA  2

#define LFG_MR_NWOOD      7   /* Wood 95 files: 0.4 ... 1.0 M_sun */
#define LFG_MR_MAX_KNOTS  32  /* Panei spline: knots per axis */
/* everything the kernel stages into LDS, in doubles (64 KiB) */
#define LFG_MR_MAX_DOUBLES 8192

/*
 * The mass-radius tables, packed by the host (lfit_python_amd/physpar.py).
 * Pointers are [dev] for lfg_physpar and host pointers for lfg_cpu_physpar.
 *   wood_t, wood_r   the seven files' rows one after another, T [K]
 *                    increasing within a file, R [R_sun]; file k holds rows
 *                    wood_off[k] .. wood_off[k+1]-1 (at least two)
 *   wood_card        [6][7][4]: on mass interval j the cardinal cubic of file
 *                    k is sum_p card[j][k][p] (m - m_j)^p, m_j = 0.4 + 0.1 j
 *   ham_m, ham_r     n_ham >= 2 rows, mass [M_sun] increasing, R [R_sun]
 *   pan_tx, pan_ty   FITPACK knots of the bicubic spline R(T, m): pan_nx and
 *   pan_c            pan_ny of them (8 .. LFG_MR_MAX_KNOTS), coefficients
 *                    [(nx - 4)][(ny - 4)]
 *   G, GMsun, Rsun, day   SI constants (MODEL_SPEC 12.1)
 */
typedef struct lfg_mr_tables {
    const double* wood_t;
    const double* wood_r;
    int wood_off[LFG_MR_NWOOD + 1];
    const double* wood_card;
    const double* ham_m;
    const double* ham_r;
    int n_ham;
    const double* pan_tx;
    const double* pan_ty;
    const double* pan_c;
    int pan_nx, pan_ny;
    double G, GMsun, Rsun, day;
} lfg_mr_tables;

/*
 * q, dphi, rwd   [dev] row i at element i * ld (ld >= 1: the columns of a
 *                chain [rows][ndim] are read in place with ld = ndim, a
 *                thinned chain with ld = thin * ndim)
 * twd, p         [dev] n, contiguous
 * tab            HOST pointer to the struct; the arrays it names are [dev]
 * out            [dev] [LFG_PP_NCOL][n]; model, status [dev] n
 * Every element of out, model and status is written.  A row whose status is
 * not LFG_ST_OK is all NaN with model -1.  Status, first match:
 *   LFG_ST_BAD_ARGS         a non-finite input, or rwd, twd or p <= 0
 *   LFG_ST_BAD_Q            q <= 0
 *   LFG_ST_NO_MR_SOLUTION   no relation's bracket holds a sign change
 *   LFG_ST_BAD_DPHI         findi fails
 * Asynchronous on stream, re-entrant, allocates nothing and needs no
 * workspace.  LFG_E_ARGS (and no launch) for a null pointer, n < 0, ld < 1
 * or tables beyond the limits above; n = 0 returns LFG_OK.
 */
int lfg_physpar(const double* q, const double* dphi, const double* rwd, size_t ld,
                const double* twd, const double* p, int n, const lfg_mr_tables* tab,
                double* out, int* model, int* status, void* stream);

/* lanes of one launch: rows beyond it take further trips of the grid-stride loop */
int lfg_physpar_lanes(void);

#ifdef __cplusplus
}
#endif
#endif
