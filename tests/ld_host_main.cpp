// ld_host_main.cpp -- stand-alone driver of lfg_cpu_limbdark for
// tests/test_limbdark_host.py: built with the host's address and undefined-
// behaviour sanitizers together with cpu_baseline/lfg_cpu_limbdark.cpp (and so
// with lfg_limbdark.hpp and lfg_physpar.hpp, the text the GPU compiles).
//
//   ld_host_main <cases.bin> <results.bin>
//
// cases.bin: int32 {nx, ny, rows, ld}, then doubles: tx, ty, c [25 (nx-4)
// (ny-4)], chain [rows * ld] (teff in column 0, logg in column 1).  Every table
// and every buffer is a heap block of exactly its size (an overrun is the
// sanitizer's to report); out and status also carry the byte 0xA5 in guard
// bands before and behind and a fill byte inside, which are checked here.  For
// n of 0, 1, 65 and 257 the first n rows are evaluated and {rc, out [n][25],
// status [n]} appended to results.bin.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lfg_cpu.h"

namespace {

constexpr size_t BAND = 256;

void die(const char* what)
{
    fprintf(stderr, "ld_host_main: %s\n", what);
    exit(2);
}

template <class T>
T* read_block(FILE* fh, size_t n)
{
    T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
    if (!p || fread(p, sizeof(T), n, fh) != n) die("short case file");
    return p;
}

// a payload of `bytes` between two guard bands
struct Guarded {
    unsigned char* raw;
    size_t bytes;
    explicit Guarded(size_t b) : raw(static_cast<unsigned char*>(malloc(b + 2 * BAND))), bytes(b)
    {
        if (!raw) die("out of memory");
        memset(raw, 0xA5, b + 2 * BAND);
        memset(raw + BAND, 0xFF, b);
    }
    ~Guarded() { free(raw); }
    void* data() { return raw + BAND; }
    bool intact() const
    {
        for (size_t i = 0; i < BAND; ++i)
            if (raw[i] != 0xA5 || raw[BAND + bytes + i] != 0xA5) return false;
        return true;
    }
    // no element of `size` bytes still holds the fill (a NaN the twin writes is 0x7ff8...: never all ones)
    bool all_written(size_t size) const
    {
        for (size_t e = 0; e + size <= bytes; e += size) {
            bool untouched = true;
            for (size_t k = 0; k < size; ++k) untouched = untouched && raw[BAND + e + k] == 0xFF;
            if (untouched) return false;
        }
        return true;
    }
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) die("usage: ld_host_main cases.bin results.bin");
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) die("cannot open the case file");
    int32_t head[4];
    if (fread(head, 4, 4, fh) != 4) die("short header");
    const int nx = head[0], ny = head[1], rows = head[2], ld = head[3];
    if (nx < 8 || ny < 8 || rows < 0 || ld < 2) die("bad header");
    double* tx = read_block<double>(fh, nx);
    double* ty = read_block<double>(fh, ny);
    double* c = read_block<double>(fh, size_t(LFG_LD_NCOL) * (nx - 4) * (ny - 4));
    double* chain = read_block<double>(fh, size_t(rows) * ld);
    fclose(fh);
    lfg_ld_tables T;
    T.tx = tx; T.ty = ty; T.nx = nx; T.ny = ny; T.c = c;

    FILE* out = fopen(argv[2], "wb");
    if (!out) die("cannot open the result file");
    const int counts[4] = {0, 1, 65, 257};
    for (int ci = 0; ci < 4; ++ci) {
        const int n = counts[ci];
        if (n > rows) die("too few rows");
        // the chain of exactly n rows: it ends on row n - 1's last used column
        const size_t used = n ? size_t(n - 1) * ld + 2 : 0;
        double* ch = static_cast<double*>(malloc(used ? used * sizeof(double) : 1));
        if (!ch) die("out of memory");
        memcpy(ch, chain, used * sizeof(double));
        Guarded o(size_t(n) * LFG_LD_NCOL * sizeof(double)), s(size_t(n) * sizeof(int));
        const int32_t rc = lfg_cpu_limbdark(ch + 1, ch, size_t(ld), n, &T, static_cast<double*>(o.data()),
                                            static_cast<int*>(s.data()), ci % 2 ? 4 : 1);
        if (!o.intact() || !s.intact()) die("a guard band was written");
        if (!o.all_written(sizeof(double)) || !s.all_written(sizeof(int))) die("an output element was left unwritten");
        if (memcmp(ch, chain, used * sizeof(double))) die("an input was changed");
        fwrite(&rc, 4, 1, out);
        fwrite(o.data(), 1, o.bytes, out);
        fwrite(s.data(), 1, s.bytes, out);
        free(ch);
    }
    // the argument checks return before anything is read
    Guarded o(LFG_LD_NCOL * sizeof(double)), s(sizeof(int));
    double* od = static_cast<double*>(o.data());
    int* sd = static_cast<int*>(s.data());
    lfg_ld_tables B = T;
    B.nx = 7;
    int bad = lfg_cpu_limbdark(chain + 1, chain, ld, 1, &B, od, sd, 1) != LFG_E_ARGS;
    B.nx = nx; B.ny = LFG_LD_MAX_KNOTS + 1;
    bad += lfg_cpu_limbdark(chain + 1, chain, ld, 1, &B, od, sd, 1) != LFG_E_ARGS;
    bad += lfg_cpu_limbdark(chain + 1, chain, ld, -1, &T, od, sd, 1) != LFG_E_ARGS;
    bad += lfg_cpu_limbdark(chain + 1, chain, 0, 1, &T, od, sd, 1) != LFG_E_ARGS;
    bad += lfg_cpu_limbdark(nullptr, chain, ld, 1, &T, od, sd, 1) != LFG_E_ARGS;
    bad += lfg_cpu_limbdark(chain + 1, chain, ld, 1, nullptr, od, sd, 1) != LFG_E_ARGS;
    bad += lfg_cpu_limbdark(chain + 1, chain, ld, 1, &T, nullptr, sd, 1) != LFG_E_ARGS;
    if (bad || o.all_written(sizeof(double)) || !o.intact() || !s.intact()) die("a refused call misbehaved");
    fclose(out);
    free(tx); free(ty); free(c); free(chain);
    return 0;
}
