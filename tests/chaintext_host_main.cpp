// The chain-text host twin (cpu_baseline/lfg_cpu_chaintext.cpp) as a
// stand-alone program for the host's sanitizers (tests/test_chaintext_host.py).
//
//   chaintext_host CASES RESULTS
//
// CASES: int32 count, then per case  int64 {steps, W, ndim, step_ld,
// walker_ld, offset, nbuf, lnp_step_ld, lnp_walker_ld, lnp_offset, nlnp,
// walker0, out_bytes}  followed by nbuf doubles of chain and nlnp doubles of
// ln_prob.  Either input lives in a heap block of exactly its size, the output
// between guard bands of 64 bytes that are checked after the call; the bytes
// of the output beyond the total must keep their fill as well.  RESULTS: per
// case int32 rc, int64 nbytes[2], then nbytes[0] bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lfg_cpu.h"

namespace {

constexpr size_t GUARD = 64;
constexpr unsigned char FILL = 0xA5;

template <class T>
T* exact(FILE* f, size_t count)
{
    T* p = static_cast<T*>(malloc(count ? count * sizeof(T) : 1));
    if (count && fread(p, sizeof(T), count, f) != count) exit(3);
    return p;
}

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
        int64_t h[13];
        if (fread(h, 8, 13, in) != 13) return 3;
        double* buf = exact<double>(in, size_t(h[6]));
        double* lnp = exact<double>(in, size_t(h[10]));
        const size_t cap = size_t(h[12]);
        unsigned char* raw = static_cast<unsigned char*>(malloc(cap + 2 * GUARD));
        memset(raw, FILL, cap + 2 * GUARD);
        long long nb[2] = {-7, -7};
        const int32_t rc = lfg_cpu_chain_text(buf + h[5], h[0], h[1], int(h[2]), h[3], h[4], lnp + h[9], h[7], h[8],
                                              h[11], raw + GUARD, cap, nb, 2);
        const size_t used = rc == LFG_OK ? size_t(nb[0]) : 0;
        if (used > cap) {
            fprintf(stderr, "case %d: a total beyond the output\n", k);
            return 5;
        }
        for (size_t i = 0; i < GUARD; ++i)
            if (raw[i] != FILL || raw[GUARD + cap + i] != FILL) {
                fprintf(stderr, "case %d: a guard band was written\n", k);
                return 5;
            }
        for (size_t i = used; i < cap; ++i)
            if (raw[GUARD + i] != FILL) {
                fprintf(stderr, "case %d: a byte beyond the total was written\n", k);
                return 5;
            }
        fwrite(&rc, 4, 1, out);
        fwrite(nb, 8, 2, out);
        fwrite(raw + GUARD, 1, used, out);
        free(buf), free(lnp), free(raw);
    }
    fclose(in);
    return fclose(out) ? 6 : 0;
}
