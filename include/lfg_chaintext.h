/*
 * lfg_chaintext.h -- the rows of chain_prod.txt formatted on the device
 * (MODEL_SPEC.md section 17), byte for byte what Python writes:
 *
 *   '{0:4d}'.format(walker0 + w), then ' ' + repr(float(x)) for each of the
 *   ndim values, then ' ' + '{:f}'.format(lnp) and '\n'
 *
 * for step s = 0 .. steps-1 in order and, within it, walker w = 0 .. W-1.
 * repr is CPython's short repr (the shortest digits that read back, the
 * closest of those; fixed notation for -4 < decpt <= 16), '{:f}' the exact
 * value rounded half-even at the sixth decimal.  The header line of the file
 * stays with the caller.
 *
 * A header of its own: include/lfg.h's function set is pinned by the ABI
 * tests.  Its conventions hold: plain pointers, the caller's stream, no
 * allocation, size functions, LFG_E_ARGS before any launch with nothing
 * written, no host synchronisation.
 *
 * The chain is the view of lfg_chain.h: element (s, w, c) is
 * base[s * step_ld + w * walker_ld + c].  ln_prob has two leading dimensions
 * of its own: lnp[s * lnp_step_ld + w * lnp_walker_ld].  The sampler's
 * [steps][W] is (W, 1); the cold level of a tempered [steps][T][W] is
 * (T * W, 1); thinning multiplies the step dimensions.
 *
 * '{:f}' of a finite |lnp| >= 2^63 needs more than 128-bit integers.  The
 * device REFUSES such a row instead of carrying a bignum: it writes '?' in
 * the place of that number and counts the row in nbytes[1].  A caller that
 * finds nbytes[1] != 0 formats on the host (lfit_python_amd.chaintext does).
 * Every other double, the non-finite ones included, is formatted exactly.
 */
#ifndef LFG_CHAINTEXT_H
#define LFG_CHAINTEXT_H

#include <stddef.h>

#include "lfg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LFG_CHAIN_TEXT_MAX_NDIM 1023 /* values of one row */

/* an upper bound on the bytes of steps * W rows whose walker numbers run from
 * walker0; -1 for a refused shape (negative sizes, ndim < 1 or >
 * LFG_CHAIN_TEXT_MAX_NDIM, walker0 < 0, or a bound beyond int64) */
long long lfg_chain_text_bound(long long steps, long long W, int ndim, long long walker0);

/* bytes of scratch lfg_chain_text needs (256-byte aligned base); 0 for a
 * refused shape */
size_t lfg_chain_text_workspace_size(long long steps, long long W, int ndim);

/* rows one workgroup formats: more rows are shared among several workgroups */
int lfg_chain_text_tile_rows(int ndim);

/*
 * base, steps, W, ndim, step_ld, walker_ld          the chain view, base [dev]
 * lnp, lnp_step_ld, lnp_walker_ld                   ln_prob's view, lnp [dev]
 * walker0    the number of walker 0 (>= 0)
 * out        [dev] out_bytes bytes, out_bytes >= lfg_chain_text_bound(...).
 *            Any alignment.  Bytes at and beyond the total are not written.
 * nbytes     [dev] 2 int64: the total bytes; the rows refused (see above)
 * ws         [dev] ws_bytes >= lfg_chain_text_workspace_size(...)
 *
 * LFG_E_ARGS, and no launch, for: a null required pointer, a refused shape,
 * a leading dimension < 1, out_bytes below the bound, ws_bytes short.
 * steps = 0 or W = 0 writes nbytes = {0, 0} and returns LFG_OK.
 *
 * The result is a function of the arguments alone, whatever ws and out held
 * on entry.  Offsets and totals are int64.
 */
int lfg_chain_text(const double* base, long long steps, long long W, int ndim, long long step_ld,
                   long long walker_ld, const double* lnp, long long lnp_step_ld, long long lnp_walker_ld,
                   long long walker0, unsigned char* out, size_t out_bytes, long long* nbytes, void* ws,
                   size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
