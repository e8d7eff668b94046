// The chain summary's host twin (cpu_baseline/lfg_cpu_chain.cpp) as a
// stand-alone program for the host's sanitizers (tests/test_chain_host.py).
//
//   chain_host CASES RESULTS
//
// CASES: int32 count, then per case  int64 {steps, W, C, step_ld, walker_ld,
// offset, nbuf, has_window, nq, rhat, clip}  followed by nbuf doubles, the
// window (2 C doubles, if any) and nq fractions.  Every input lives in a heap
// block of exactly its size, every output between guard bands of 64 doubles
// that are checked after the call.  RESULTS: per case int32 rc, then n, n_bad
// (int64), mean, m2, min, max, ostat, quant, rhat (if asked), and with clip
// the next window from lfg_cpu_chain_clip (sigma 3, median = fraction 0).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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
        int64_t h[11];
        if (fread(h, 8, 11, in) != 11) return 3;
        const long long steps = h[0], W = h[1], sld = h[3], wld = h[4], off = h[5];
        const int C = int(h[2]), nq = int(h[8]);
        double* buf = exact<double>(in, size_t(h[6]));
        double* win = h[7] ? exact<double>(in, size_t(2 * C)) : nullptr;
        double* fr = exact<double>(in, size_t(nq));
        Guarded<long long> n(C), bad(C);
        Guarded<double> mean(C), m2(C), lo(C), hi(C), ostat(size_t(C) * nq * 2), quant(size_t(C) * nq), rhat(C), next(2 * C);
        const int32_t rc = lfg_cpu_chain_stats(buf + off, steps, W, C, sld, wld, win, nq ? fr : nullptr, nq, n.data(),
                                               bad.data(), mean.data(), m2.data(), lo.data(), hi.data(), ostat.data(),
                                               quant.data(), h[9] ? rhat.data() : nullptr);
        if (rc == LFG_OK && h[10] && lfg_cpu_chain_clip(n.data(), m2.data(), quant.data(), nq, 3.0, win, next.data(), C))
            return 4;
        if (!(n.intact() && bad.intact() && mean.intact() && m2.intact() && lo.intact() && hi.intact() &&
              ostat.intact() && quant.intact() && rhat.intact() && next.intact())) {
            fprintf(stderr, "case %d: a guard band was written\n", k);
            return 5;
        }
        fwrite(&rc, 4, 1, out);
        n.write(out), bad.write(out), mean.write(out), m2.write(out), lo.write(out), hi.write(out);
        ostat.write(out), quant.write(out);
        if (h[9]) rhat.write(out);
        if (h[10]) next.write(out);
        free(buf), free(win), free(fr);
    }
    fclose(in);
    return fclose(out) ? 6 : 0;
}
