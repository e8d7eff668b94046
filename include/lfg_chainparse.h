/*
 * lfg_chainparse.h -- the numbers of chain_prod.txt read on the device
 * (MODEL_SPEC.md section 18): every field becomes the IEEE double that
 * Python's float(token) gives, bit for bit.  The inverse of lfg_chaintext.h.
 *
 * A header of its own: include/lfg.h's function set is pinned by the ABI
 * tests.  Its conventions hold: plain pointers, the caller's stream, no
 * allocation, size functions, LFG_E_ARGS before any launch with nothing
 * written, no host synchronisation.
 *
 * The text.  Runs of space or tab separate fields; '\n' ends a row; a '\r'
 * directly before a '\n' (or as the last byte) is blank, any other '\r' is a
 * bad byte.  A missing final newline is fine; whitespace-only lines at the end
 * are ignored.  The header line of the file stays with the caller, which
 * passes text + offset: text may have any alignment.
 *
 * A field is  [+-]? ( digits [. digits?]? | . digits ) ( [eE] [+-]? digits )?
 * or inf / infinity / nan in any letter case with an optional sign.  Anything
 * else is BAD: NaN is stored and the field is counted in info[2].
 *
 * The value is the correctly rounded double: the sign of zero is kept,
 * overflow gives +-inf, underflow goes through the subnormals to +-0, an
 * exponent field of any length is clamped.  The device decides every token of
 * at most LFG_CHAIN_PARSE_MAX_TOKEN bytes whose mantissa has at most 19
 * significant decimal digits (from the first to the last non-zero digit,
 * across the point), and a longer mantissa whenever its first 19 digits
 * already decide the rounding.  Every other token is REFUSED: NaN is stored,
 * the field is counted in info[3], and it is never given a wrong value.  A
 * token longer than LFG_CHAIN_PARSE_MAX_TOKEN bytes is refused without being
 * read to its end, whether or not it is a number: the host decides (the twin
 * cpu_baseline/lfg_cpu_chainparse.cpp refuses nothing).
 *
 * Two calls, because the number of rows is known only after a pass over the
 * bytes: lfg_chain_parse_count, one device read of info by the caller, then
 * lfg_chain_parse into an `out` of info[0] rows.
 */
#ifndef LFG_CHAINPARSE_H
#define LFG_CHAINPARSE_H

#include <stddef.h>

#include "lfg.h"
#include "lfg_chaintext.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LFG_CHAIN_PARSE_MAX_TOKEN 64                           /* bytes of a token the device reads */
#define LFG_CHAIN_PARSE_MAX_NCOL (LFG_CHAIN_TEXT_MAX_NDIM + 2) /* fields of one row */
#define LFG_CHAIN_PARSE_MAX_BYTES (1ll << 46)                  /* bytes of one text */

/* bytes one workgroup scans.  Tiles are cut at multiples of it counted from
 * the 16-byte boundary at or below text. */
int lfg_chain_parse_tile_bytes(void);

/* bytes of scratch both calls need (256-byte aligned base); 0 for a refused
 * size (nbytes < 0 or > LFG_CHAIN_PARSE_MAX_BYTES) */
size_t lfg_chain_parse_workspace_size(long long nbytes);

/*
 * text, nbytes   [dev] the bytes, any alignment; nbytes = 0 or blanks only:
 *                zero rows and LFG_OK
 * ncol           fields of a row, 1 .. LFG_CHAIN_PARSE_MAX_NCOL
 * info           [dev] 8 int64, all written:
 *                  [0] rows    [1] fields    [2] 0    [3] 0
 *                  [4] ragged: the row ends at which the running number of
 *                      fields is not ncol times the running number of rows;
 *                      non-zero exactly when some row has not ncol fields (a
 *                      blank line that is not at the end is such a row)
 *                  [5] the first ragged row, or -1    [6] 0    [7] 0
 * ws             [dev] ws_bytes >= lfg_chain_parse_workspace_size(nbytes).
 *                Afterwards it holds what lfg_chain_parse needs: per tile the
 *                fields and lines before it, as int64.
 *
 * LFG_E_ARGS, and no launch, for: a null info or ws, a null text with
 * nbytes > 0, a refused nbytes, ncol out of range, ws_bytes short.
 */
int lfg_chain_parse_count(const unsigned char* text, long long nbytes, int ncol, long long* info, void* ws,
                          size_t ws_bytes, void* stream);

/*
 * Called with the text, nbytes, ncol and ws of lfg_chain_parse_count, and the
 * info it filled.
 *
 * out, out_rows  [dev] out_rows * ncol doubles; row-major out[rows][ncol] is
 *                written, nothing beyond rows * ncol doubles.  info[0] lives
 *                on the device, so the host side refuses only out_rows < 0;
 *                out_rows < info[0] is found on the device: nothing is
 *                written to out and info[6] = 1.
 * info           [2] bad fields  [3] refused fields  [5] the first row with a
 *                bad field or -1 (a refused field is not bad), [6] as above.
 *                When info[4] != 0, nothing is written but info[2] = info[3]
 *                = info[6] = 0, and info[5] keeps the first ragged row.
 *
 * LFG_E_ARGS, and no launch, for what lfg_chain_parse_count refuses, for
 * out_rows < 0 and for a null out with out_rows > 0.
 *
 * The results of both calls are a function of the arguments alone, whatever
 * ws and out held on entry; calling lfg_chain_parse again gives the same.
 */
int lfg_chain_parse(const unsigned char* text, long long nbytes, int ncol, double* out, long long out_rows,
                    long long* info, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
