/*
 * lfg_chain.h -- a chain's summary on the device (MODEL_SPEC.md section 14):
 * per column the count, mean, second moment, minimum and maximum, exact order
 * statistics with numpy's linear quantiles, Gelman-Rubin's R-hat over the
 * walkers, and the windows of a sigma clip.
 *
 * A header of its own: include/lfg.h's function set is pinned by the ABI
 * tests.  Its conventions hold: plain pointers, the caller's stream, no
 * allocation, a size function for the scratch, LFG_E_ARGS before any launch
 * with nothing written, no host synchronisation.
 *
 * The chain view.  Element (s, w, c) is base[s * step_ld + w * walker_ld + c],
 * 0 <= s < steps, 0 <= w < W, 0 <= c < C, leading dimensions in elements and
 * >= 1; columns are contiguous, and elements of a row beyond C are never
 * read.  The sampler's chain [steps][W][ndim] is (step_ld = W * ndim,
 * walker_ld = ndim), a walker-major array [W][steps][ndim] is (step_ld =
 * ndim, walker_ld = steps * ndim), a flat chain has W = 1; skipping rows
 * offsets base, thinning multiplies step_ld.  steps * W counts as int64.
 */
#ifndef LFG_CHAIN_H
#define LFG_CHAIN_H

#include <stddef.h>

#include "lfg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LFG_CHAIN_MAX_C   4096  /* columns of one call */
#define LFG_CHAIN_MAX_NQ  8     /* quantile fractions of one call */

/* bytes of scratch lfg_chain_stats needs (256-byte aligned base); 0 for a
 * refused shape */
size_t lfg_chain_workspace_size(long long steps, long long W, int C, int nq);

/* rows one workgroup of the sweeps takes at the least: a chain of more rows
 * is shared among several workgroups */
int lfg_chain_tile_rows(void);
/* columns one workgroup of the histogram sweep takes for nq fractions: more
 * columns are split into tiles (0 for a refused nq) */
int lfg_chain_hist_tile(int nq);

/*
 * base, steps, W, C, step_ld, walker_ld   the view, base [dev]
 * window   [dev] C x 2 (lo, hi inclusive) or NULL.  A value is used when it
 *          is finite and inside its column's window.
 * fracs    HOST array of nq fractions in [0, 1] (NULL with nq = 0)
 * Outputs, all [dev], all written for every column:
 *   n, n_bad   [C] int64: the values used; the non-finite values
 *   mean, m2   [C]: m2 = sum (x - mean)^2 over the used values
 *   vmin, vmax [C]
 *   ostat      [C][nq][2]: the order statistics at the two ranks bracketing
 *              each fraction (rank rule: MODEL_SPEC 14.2), exactly the values
 *              a sort of the used values holds there
 *   quant      [C][nq]: numpy's 'linear' interpolation of the two
 *   rhat       [C] or NULL: Gelman-Rubin with the W walkers as chains of
 *              length steps.  NaN for W < 2, steps < 2 or a column holding a
 *              non-finite value.  Must be NULL with a window.
 * ostat and quant may be NULL when nq = 0.  A column with n = 0 gives NaN
 * mean, m2, vmin, vmax, ostat and quant.  steps = 0 or W = 0 writes those
 * values (rhat NaN) and returns LFG_OK.
 *
 * LFG_E_ARGS, and no launch, for: a null required pointer, negative sizes,
 * C < 1 or C > LFG_CHAIN_MAX_C, nq < 0 or nq > LFG_CHAIN_MAX_NQ, a fraction
 * outside [0, 1] or NaN, a leading dimension < 1, rhat with a window,
 * ws_bytes below lfg_chain_workspace_size(steps, W, C, nq).
 *
 * The results are a function of the arguments alone: the same call on the
 * same data gives the same bits whatever ws held on entry.
 */
int lfg_chain_stats(const double* base, long long steps, long long W, int C, long long step_ld, long long walker_ld,
                    const double* window, const double* fracs, int nq, long long* n, long long* n_bad, double* mean,
                    double* m2, double* vmin, double* vmax, double* ostat, double* quant, double* rhat, void* ws,
                    size_t ws_bytes, void* stream);

/*
 * The next round's window of a sigma clip, from one round's stats:
 *   sd = sqrt(m2 / n),  lo' = max(lo, med - sigma * sd),  hi' = min(hi, med + sigma * sd)
 * with (lo, hi) = win_in's, or (-inf, +inf) for win_in = NULL.  A column with
 * n = 0 or a non-finite med or sd keeps its window.
 * n, m2 [dev] C; med [dev] column c's median at med[c * med_ld]; win_in [dev]
 * C x 2 or NULL; win_out [dev] C x 2 (may be win_in).  LFG_E_ARGS for a null
 * required pointer, C < 1 or > LFG_CHAIN_MAX_C, med_ld < 1, sigma negative or NaN.
 */
int lfg_chain_clip(const long long* n, const double* m2, const double* med, long long med_ld, double sigma,
                   const double* win_in, double* win_out, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
