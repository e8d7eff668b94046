// The corner-plot data's host twin (cpu_baseline/lfg_cpu_corner.cpp) as a
// stand-alone program for the host's sanitizers (tests/test_corner_host.py).
//
//   corner_host CASES RESULTS
//
// CASES: int32 count, then per case  int64 {steps, W, row_len, step_ld,
// walker_ld, offset, nbuf, K, nb, nl}  followed by nbuf doubles, K int32
// columns, 2 K doubles of ranges and nl fractions.  Every input lives in a
// heap block of exactly its size, every output between guard bands of 64
// elements that are checked after the call.  RESULTS: per case int32 rc of
// the histograms, int32 rc of the levels, then h1 [K][nb], h2 [P][nb][nb],
// level [P][nl] (int64) and flag [K] (int32).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lfg_cpu.h"

namespace {

constexpr size_t GUARD = 64;
constexpr unsigned char FILL = 0xA5;

template <class T>
struct Guarded {
    size_t n;
    unsigned char* raw;
    explicit Guarded(size_t count) : n(count)
    {
        raw = static_cast<unsigned char*>(malloc((n + 2 * GUARD) * sizeof(T)));
        memset(raw, FILL, (n + 2 * GUARD) * sizeof(T));
    }
    ~Guarded() { free(raw); }
    T* data() { return reinterpret_cast<T*>(raw) + GUARD; }
    bool intact() const
    {
        for (size_t i = 0; i < GUARD * sizeof(T); ++i)
            if (raw[i] != FILL || raw[(GUARD + n) * sizeof(T) + i] != FILL) return false;
        return true;
    }
    void write(FILE* f) { fwrite(data(), sizeof(T), n, f); }
};

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
        int64_t h[10];
        if (fread(h, 8, 10, in) != 10) return 3;
        const long long steps = h[0], W = h[1], sld = h[3], wld = h[4], off = h[5];
        const int row_len = int(h[2]), K = int(h[7]), nb = int(h[8]), nl = int(h[9]);
        const size_t P = size_t(K) * (K - 1) / 2;
        double* buf = exact<double>(in, size_t(h[6]));
        int32_t* cols = exact<int32_t>(in, size_t(K));
        double* range = exact<double>(in, size_t(2 * K));
        double* fr = exact<double>(in, size_t(nl));
        Guarded<long long> h1(size_t(K) * nb), h2(P * nb * nb), level(P * nl);
        Guarded<int> flag(K);
        const int32_t rc = lfg_cpu_corner_hist(buf + off, steps, W, row_len, sld, wld, cols, K, range, nb, h1.data(),
                                               K > 1 ? h2.data() : nullptr, flag.data());
        const int32_t rl = rc == LFG_OK ? lfg_cpu_corner_levels(h2.data(), int(P), nb, fr, nl, level.data()) : -1;
        if (!(h1.intact() && h2.intact() && level.intact() && flag.intact())) {
            fprintf(stderr, "case %d: a guard band was written\n", k);
            return 5;
        }
        fwrite(&rc, 4, 1, out);
        fwrite(&rl, 4, 1, out);
        h1.write(out), h2.write(out), level.write(out), flag.write(out);
        free(buf), free(cols), free(range), free(fr);
    }
    fclose(in);
    return fclose(out) ? 6 : 0;
}
