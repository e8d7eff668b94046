/*
 * lfg_corner.h -- a corner plot's data on the device (MODEL_SPEC.md section
 * 16): per chosen column a marginal histogram, per pair of chosen columns a
 * two-dimensional histogram, and per pair the counts at which the contours
 * are drawn.  Everything is an integer: the counts equal numpy's histogram
 * and histogram2d bin for bin.
 *
 * A header of its own: include/lfg.h's and include/lfg_chain.h's function
 * sets are pinned by the ABI tests.  Their conventions hold: plain pointers,
 * the caller's stream, no allocation, a size function for the scratch,
 * LFG_E_ARGS before any launch with nothing written, no host synchronisation.
 *
 * The view is lfg_chain.h's: element (s, w, c) is base[s * step_ld + w *
 * walker_ld + c], 0 <= c < row_len.  cols[K] names the columns to plot:
 * distinct, in any order, not necessarily adjacent.  Only those elements of
 * a row are read.
 */
#ifndef LFG_CORNER_H
#define LFG_CORNER_H

#include <stddef.h>

#include "lfg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LFG_CORNER_MAX_K       64  /* columns of one call */
#define LFG_CORNER_MAX_BINS    64  /* bins per axis */
#define LFG_CORNER_MAX_LEVELS  8   /* contour fractions of one call */

/* bytes of scratch lfg_corner_hist needs (256-byte aligned base); 0 for a
 * refused shape */
size_t lfg_corner_workspace_size(long long steps, long long W, int K, int nb);

/* rows one workgroup of the histogram sweep takes at the least: a chain of
 * more rows is shared among several workgroups */
int lfg_corner_tile_rows(void);
/* pair histograms one workgroup keeps on chip for nb bins: more pairs are
 * split into tiles, each of which reads the chain once (0 for a refused nb) */
int lfg_corner_pair_tile(int nb);

/*
 * base, steps, W, row_len, step_ld, walker_ld   the view, base [dev]
 * cols    HOST array of K distinct column indices in [0, row_len)
 * range   [dev] K x 2: column k's (lo, hi).  A value x is used when it is
 *         finite and lo <= x <= hi; its bin is the largest i < nb with
 *         e[i] <= x, where e[i] = i * ((hi - lo) / nb) + lo (a multiply,
 *         then an add) and x == hi goes to bin nb - 1.  A column whose range
 *         is not finite, or has hi <= lo, is immobile: its flag is 1 and its
 *         counts are all zero.  Not an error.
 * Outputs, all [dev], all written in full:
 *   h1    [K][nb] int64: column k's used values per bin
 *   h2    [P][nb][nb] int64, P = K (K - 1) / 2: for pair p = (a, b), a < b in
 *         cols order, numbered (0,1), (0,2), ..., (K-2,K-1), the rows whose
 *         two values are both used, by a's bin then b's.  NULL iff K == 1.
 *   flag  [K] int: 1 for an immobile column, else 0
 * steps = 0 or W = 0 writes zeros and the flags and returns LFG_OK.
 *
 * LFG_E_ARGS, and no launch, for: a null required pointer, negative sizes,
 * K < 1 or K > LFG_CORNER_MAX_K, nb < 1 or nb > LFG_CORNER_MAX_BINS, a
 * column index outside [0, row_len) or repeated, a leading dimension < 1,
 * ws_bytes below lfg_corner_workspace_size(steps, W, K, nb).
 *
 * The results are a function of the arguments alone: the same call on the
 * same data gives the same bits whatever ws and the outputs held on entry.
 */
int lfg_corner_hist(const double* base, long long steps, long long W, int row_len, long long step_ld,
                    long long walker_ld, const int* cols, int K, const double* range, int nb, long long* h1,
                    long long* h2, int* flag, void* ws, size_t ws_bytes, void* stream);

/*
 * The contour levels of P histograms of nb x nb counts (corner's hist2d
 * rule).  For each pair and each fraction f: sort the counts descending, sum
 * them cumulatively in integers; the level is the count at the last position
 * m with (double)cum[m] / (double)total <= f, or the largest count if there
 * is no such position (total = 0 gives 0).
 *   h2 [dev] [P][nb][nb] int64 (counts >= 0); fracs HOST [nl];
 *   level [dev] [P][nl] int64.
 * LFG_E_ARGS for a null pointer, P < 0, nb outside 1..LFG_CORNER_MAX_BINS,
 * nl outside 1..LFG_CORNER_MAX_LEVELS, a fraction outside [0, 1] or NaN.
 * P = 0 launches nothing.
 */
int lfg_corner_levels(const long long* h2, int P, int nb, const double* fracs, int nl, long long* level, void* stream);

#ifdef __cplusplus
}
#endif
#endif
