// physpar_host_main.cpp -- stand-alone driver of lfg_cpu_physpar for
// tests/test_physpar_host.py: built with the host's address and undefined-
// behaviour sanitizers together with cpu_baseline/lfg_cpu_physpar.cpp (and so
// with lfg_physpar.hpp and lfg_device.hpp, the text the GPU compiles).
//
//   physpar_host_main <cases.bin> <results.bin>
//
// cases.bin: int32 {n_wood, n_ham, nx, ny, rows, ld}, int32 wood_off[8], then
// doubles: wood_t, wood_r, card [168], ham_m, ham_r, tx, ty, c, {G, GMsun,
// Rsun, day}, chain [rows * ld] (q, dphi, rwd in columns 0, 1, 2), twd, p.
// Every table and every buffer is a heap block of exactly its size (an
// overrun is the sanitizer's to report); out, model and status also carry the
// byte 0xA5 in guard bands before and behind and a fill byte inside, which are
// checked here.  For n of 0, 1, 65 and 257 the first n rows are solved and
// {rc, out [10][n], model [n], status [n]} appended to results.bin.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lfg_cpu.h"

namespace {

constexpr size_t BAND = 256;

void die(const char* what)
{
    fprintf(stderr, "physpar_host_main: %s\n", what);
    exit(2);
}

template <class T>
T* read_block(FILE* fh, size_t n)
{
    T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
    if (!p || fread(p, sizeof(T), n, fh) != n) die("short case file");
    return p;
}

// a payload of `bytes` between two guard bands, each its own heap block's part
struct Guarded {
    unsigned char* raw;
    size_t bytes;
    unsigned char fill;
    explicit Guarded(size_t b, unsigned char f = 0xFF)
        : raw(static_cast<unsigned char*>(malloc(b + 2 * BAND))), bytes(b), fill(f)
    {
        if (!raw) die("out of memory");
        memset(raw, 0xA5, b + 2 * BAND);
        memset(raw + BAND, fill, b);
    }
    ~Guarded() { free(raw); }
    void* data() { return raw + BAND; }
    bool intact() const
    {
        for (size_t i = 0; i < BAND; ++i)
            if (raw[i] != 0xA5 || raw[BAND + bytes + i] != 0xA5) return false;
        return true;
    }
    // no element of `size` bytes still holds the fill
    bool all_written(size_t size) const
    {
        for (size_t e = 0; e + size <= bytes; e += size) {
            bool untouched = true;
            for (size_t k = 0; k < size; ++k) untouched = untouched && raw[BAND + e + k] == fill;
            if (untouched) return false;
        }
        return true;
    }
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) die("usage: physpar_host_main cases.bin results.bin");
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) die("cannot open the case file");
    int32_t head[6], off[8];
    if (fread(head, 4, 6, fh) != 6 || fread(off, 4, 8, fh) != 8) die("short header");
    const int n_wood = head[0], n_ham = head[1], nx = head[2], ny = head[3], rows = head[4], ld = head[5];
    lfg_mr_tables T;
    memset(&T, 0, sizeof T);
    double* wood_t = read_block<double>(fh, n_wood);
    double* wood_r = read_block<double>(fh, n_wood);
    double* card = read_block<double>(fh, 168);
    double* ham_m = read_block<double>(fh, n_ham);
    double* ham_r = read_block<double>(fh, n_ham);
    double* tx = read_block<double>(fh, nx);
    double* ty = read_block<double>(fh, ny);
    double* c = read_block<double>(fh, size_t(nx - 4) * (ny - 4));
    double* k = read_block<double>(fh, 4);
    double* chain = read_block<double>(fh, size_t(rows) * ld);
    double* twd = read_block<double>(fh, rows);
    double* p = read_block<double>(fh, rows);
    fclose(fh);
    T.wood_t = wood_t; T.wood_r = wood_r; T.wood_card = card; T.ham_m = ham_m; T.ham_r = ham_r;
    T.pan_tx = tx; T.pan_ty = ty; T.pan_c = c;
    for (int i = 0; i < 8; ++i) T.wood_off[i] = off[i];
    T.n_ham = n_ham; T.pan_nx = nx; T.pan_ny = ny;
    T.G = k[0]; T.GMsun = k[1]; T.Rsun = k[2]; T.day = k[3];

    FILE* out = fopen(argv[2], "wb");
    if (!out) die("cannot open the result file");
    const int counts[4] = {0, 1, 65, 257};
    for (int ci = 0; ci < 4; ++ci) {
        const int n = counts[ci];
        if (n > rows) die("too few rows");
        // the inputs of exactly n rows: the chain ends on row n - 1's last used column
        const size_t used = n ? size_t(n - 1) * ld + 3 : 0;
        double* ch = static_cast<double*>(malloc(used ? used * sizeof(double) : 1));
        double* tw = static_cast<double*>(malloc(n ? n * sizeof(double) : 1));
        double* pp = static_cast<double*>(malloc(n ? n * sizeof(double) : 1));
        if (!ch || !tw || !pp) die("out of memory");
        memcpy(ch, chain, used * sizeof(double));
        memcpy(tw, twd, n * sizeof(double));
        memcpy(pp, p, n * sizeof(double));
        Guarded o(size_t(n) * LFG_PP_NCOL * sizeof(double)), m(size_t(n) * sizeof(int), 0x7E);
        Guarded s(size_t(n) * sizeof(int));
        const int32_t rc = lfg_cpu_physpar(ch, ch + 1, ch + 2, size_t(ld), tw, pp, n, &T,
                                           static_cast<double*>(o.data()), static_cast<int*>(m.data()),
                                           static_cast<int*>(s.data()), ci % 2 ? 4 : 1);
        if (!o.intact() || !m.intact() || !s.intact()) die("a guard band was written");
        // (a NaN the twin writes is 0x7ff8...: never the all-ones fill; model's fill is 0x7E, as -1 is all ones)
        if (!o.all_written(sizeof(double)) || !m.all_written(sizeof(int)) || !s.all_written(sizeof(int)))
            die("an output element was left unwritten");
        if (memcmp(ch, chain, used * sizeof(double)) || memcmp(tw, twd, n * sizeof(double)) ||
            memcmp(pp, p, n * sizeof(double)))
            die("an input was changed");
        fwrite(&rc, 4, 1, out);
        fwrite(o.data(), 1, o.bytes, out);
        fwrite(m.data(), 1, m.bytes, out);
        fwrite(s.data(), 1, s.bytes, out);
        free(ch); free(tw); free(pp);
    }
    fclose(out);
    free(wood_t); free(wood_r); free(card); free(ham_m); free(ham_r); free(tx); free(ty); free(c); free(k);
    free(chain); free(twd); free(p);
    return 0;
}
