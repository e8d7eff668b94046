// lfg_cpu_chainparse.cpp -- lfg_chain_parse's host twin (cpu_baseline/lfg_cpu.h):
// the rules of lfit_python_amd/csrc/lfg_chainparse.hpp, the text the gfx950
// kernels compile, tile after tile over the OpenMP threads.  The same two
// calls and the same ws: a count pass, the sums over the tiles, a pass that
// checks every row's end; then the pass that forms the doubles.  It refuses
// nothing: a token the shared rules leave undecided (a mantissa of more than
// 19 digits whose cut does not decide the rounding) is finished by strtod in
// the C locale, which glibc rounds correctly.
#include <locale.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "lfg_cpu.h"
#include "lfg_chainparse.hpp"

using namespace lfg;

namespace {

struct Text {
    const unsigned char* p;
    long long n;
    int at(long long x) const { return x < n ? p[x] : '\n'; }
    bool sep(long long x) const { return cp_sep(at(x), at(x + 1)); }
    bool start(long long x) const { return !sep(x) && (x == 0 || sep(x - 1)); }
};

struct Get {
    Text t;
    long long x;
    int operator()(int j) const { return t.at(x + j); }
};

uint64_t by_strtod(const Text& t, long long x)
{
    static locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    long long e = x;
    while (e < t.n && !t.sep(e)) ++e;
    const std::string tok(reinterpret_cast<const char*>(t.p + x), size_t(e - x));
    const double v = strtod_l(tok.c_str(), nullptr, c_locale);
    uint64_t u;
    memcpy(&u, &v, 8);
    return u;
}

bool args_ok(const unsigned char* text, long long nbytes, int ncol, const long long* info, const void* ws,
             size_t ws_bytes)
{
    const size_t need = cp_ws_bytes(nbytes);
    return need != 0 && info && ws && ws_bytes >= need && (text || nbytes == 0) && ncol >= 1 &&
           ncol <= LFG_CHAIN_PARSE_MAX_NCOL;
}

}  // namespace

extern "C" int lfg_cpu_chain_parse_tile_bytes(void) { return CP_TILE; }

extern "C" size_t lfg_cpu_chain_parse_workspace_size(long long nbytes) { return cp_ws_bytes(nbytes); }

extern "C" int lfg_cpu_chain_parse_count(const unsigned char* text, long long nbytes, int ncol, long long* info,
                                         void* ws, size_t ws_bytes)
{
    if (!args_ok(text, nbytes, ncol, info, ws, ws_bytes)) return LFG_E_ARGS;
    const Text t{text, nbytes};
    const CpWs w = cp_ws(ws, nbytes);
    const long long nt = cp_ntiles(nbytes, 0);
#pragma omp parallel for schedule(static)
    for (long long k = 0; k < nt; ++k) {
        const long long b = k * CP_TILE, e = b + CP_TILE < nbytes ? b + CP_TILE : nbytes;
        long long nf = 0, nl = 0, nla = 0, nb = -1;
        for (long long x = b; x < e; ++x) {
            if (text[x] == '\n') {
                ++nl;
            } else if (!t.sep(x)) {
                nf += t.start(x) ? 1 : 0;
                nb = x;
                nla = nl;
            }
        }
        w.tf[k] = nf, w.tl[k] = nl, w.tla[k] = nla, w.tnb[k] = nb;
    }
    long long fields = 0, lines = 0, last = -1, rows = 0;
    for (long long k = 0; k < nt; ++k) {
        w.of[k] = fields, w.ol[k] = lines;
        if (w.tnb[k] >= 0) {
            last = w.tnb[k];
            rows = lines + w.tla[k] + 1;
        }
        fields += w.tf[k], lines += w.tl[k];
    }
    w.glob[0] = last;
    long long ragged = 0, first = -1;
    if (fields != rows * ncol) ragged = 1, first = rows - 1;
#pragma omp parallel for schedule(static)
    for (long long k = 0; k < nt; ++k) {
        const long long b = k * CP_TILE, e = b + CP_TILE < nbytes ? b + CP_TILE : nbytes;
        long long F = w.of[k], L = w.ol[k], bad = 0, row = -1;
        for (long long x = b; x < e && x < last; ++x) {
            if (text[x] == '\n') {
                if (F != ncol * (L + 1)) {
                    if (!bad) row = L;
                    ++bad;
                }
                ++L;
            } else if (t.start(x)) {
                ++F;
            }
        }
        if (bad) {
#pragma omp critical
            {
                ragged += bad;
                if (first < 0 || row < first) first = row;
            }
        }
    }
    info[0] = rows, info[1] = fields, info[2] = 0, info[3] = 0;
    info[4] = ragged, info[5] = first, info[6] = 0, info[7] = 0;
    return LFG_OK;
}

extern "C" int lfg_cpu_chain_parse(const unsigned char* text, long long nbytes, int ncol, double* out,
                                   long long out_rows, long long* info, void* ws, size_t ws_bytes)
{
    if (!args_ok(text, nbytes, ncol, info, ws, ws_bytes) || out_rows < 0 || (!out && out_rows > 0)) return LFG_E_ARGS;
    info[2] = info[3] = info[6] = 0;
    if (info[4] != 0) return LFG_OK;
    info[5] = -1;
    if (info[0] > out_rows) {
        info[6] = 1;
        return LFG_OK;
    }
    const Text t{text, nbytes};
    const CpWs w = cp_ws(ws, nbytes);
    const long long nt = cp_ntiles(nbytes, 0), cap = out_rows * ncol;
    long long nbad = 0, first = -1;
#pragma omp parallel for schedule(static)
    for (long long k = 0; k < nt; ++k) {
        const long long b = k * CP_TILE, e = b + CP_TILE < nbytes ? b + CP_TILE : nbytes;
        long long rank = w.of[k], bad = 0, row = -1;
        for (long long x = b; x < e; ++x) {
            if (!t.start(x)) continue;
            CpVal v = cp_token<false>(Get{t, x});
            if (v.status == CP_REFUSED) v.bits = by_strtod(t, x);
            if (v.status == CP_BAD) {
                if (!bad) row = rank / ncol;
                ++bad;
            }
            if (rank < cap) memcpy(out + rank, &v.bits, 8);
            ++rank;
        }
        if (bad) {
#pragma omp critical
            {
                nbad += bad;
                if (first < 0 || row < first) first = row;
            }
        }
    }
    info[2] = nbad, info[5] = first;
    return LFG_OK;
}
