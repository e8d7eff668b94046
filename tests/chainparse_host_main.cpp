// The chain-parse host twin (cpu_baseline/lfg_cpu_chainparse.cpp) as a
// stand-alone program for the host's sanitizers (tests/test_chainparse_host.py).
//
//   chainparse_host CASES RESULTS
//
// CASES: int32 count, then per case  int64 {nbytes, ncol, extra_rows,
// ws_short}  followed by nbytes bytes of text.  The text lives in a heap block
// of exactly its size, so that a read past its last byte is caught; ws in a
// block of exactly the size function's value (less ws_short); the output, of
// info[0] + extra_rows rows, between guard bands of 64 bytes that are checked
// after the call, and its doubles beyond rows * ncol must keep their fill.
// RESULTS: per case int32 rc of count, int32 rc of parse (-99: not called),
// int64 info[8], then info[0] * ncol doubles when parse ran and info[4] = info[6] = 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lfg_cpu.h"

namespace {

constexpr size_t GUARD = 64;
constexpr unsigned char FILL = 0xA5;

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t ncase = 0;
    if (fread(&ncase, 4, 1, in) != 1) return 3;
    for (int k = 0; k < ncase; ++k) {
        int64_t h[4];
        if (fread(h, 8, 4, in) != 4) return 3;
        const size_t n = size_t(h[0]);
        const int ncol = int(h[1]);
        unsigned char* text = static_cast<unsigned char*>(malloc(n ? n : 1));
        if (n && fread(text, 1, n, in) != n) return 3;
        const size_t need = lfg_cpu_chain_parse_workspace_size(h[0]);
        const size_t have = need - size_t(h[3]);
        unsigned char* ws = static_cast<unsigned char*>(malloc(have ? have : 1));
        memset(ws, FILL, have);
        long long info[8] = {-7, -7, -7, -7, -7, -7, -7, -7};
        const int32_t rc1 = lfg_cpu_chain_parse_count(text, h[0], ncol, info, ws, have);
        int32_t rc2 = -99;
        size_t used = 0;
        unsigned char* raw = nullptr;
        if (rc1 == LFG_OK) {
            const size_t rows = size_t(info[0]), cap = (rows + size_t(h[2])) * size_t(ncol) * 8;
            raw = static_cast<unsigned char*>(malloc(cap + 2 * GUARD));
            memset(raw, FILL, cap + 2 * GUARD);
            rc2 = lfg_cpu_chain_parse(text, h[0], ncol, reinterpret_cast<double*>(raw + GUARD),
                                      (long long)(rows + size_t(h[2])), info, ws, have);
            used = (rc2 == LFG_OK && info[4] == 0 && info[6] == 0) ? rows * size_t(ncol) * 8 : 0;
            for (size_t i = 0; i < GUARD; ++i)
                if (raw[i] != FILL || raw[GUARD + cap + i] != FILL) {
                    fprintf(stderr, "case %d: a guard band was written\n", k);
                    return 5;
                }
            for (size_t i = used; i < cap; ++i)
                if (raw[GUARD + i] != FILL) {
                    fprintf(stderr, "case %d: a double beyond rows * ncol was written\n", k);
                    return 5;
                }
        }
        fwrite(&rc1, 4, 1, out);
        fwrite(&rc2, 4, 1, out);
        fwrite(info, 8, 8, out);
        if (used) fwrite(raw + GUARD, 1, used, out);
        free(text), free(ws), free(raw);
    }
    fclose(in);
    return fclose(out) ? 6 : 0;
}
