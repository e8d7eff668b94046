// wd_host_main.cpp -- stand-alone driver of lfg_cpu_wd_lnprob for
// tests/test_wd_host.py: built with the host's address and undefined-
// behaviour sanitizers together with cpu_baseline/lfg_cpu_wd.cpp (and so with
// lfg_wd.hpp and lfg_device.hpp, the text the GPU compiles).
//
//   wd_host_main <cases.bin> <results.bin>
//
// cases.bin: int32 {B, nx, ny, rows, ld}, int32 cnx[8], cny[8], prior_type[4],
// then doubles: tx, ty, c [B (nx-4)(ny-4)], per corrected band (cnx > 0) ctx,
// cty, cc, then k[8], mag[8], err[8], lnnorm, p1[4], p2[4], c0[4], c1[4],
// theta [rows * ld].  Every table and every buffer is a heap block of exactly
// its size (an overrun is the sanitizer's to report); the outputs also carry
// the byte 0xA5 in guard bands before and behind and a fill byte inside,
// which are checked here.  For n of 0, 1, 65 and 257 the first n rows are
// evaluated and {rc, lnp [n], lnlike [n], mags [B][n], status [n]} appended
// to results.bin.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lfg_cpu.h"

namespace {

constexpr size_t BAND = 256;

void die(const char* what)
{
    fprintf(stderr, "wd_host_main: %s\n", what);
    exit(2);
}

template <class T>
T* read_block(FILE* fh, size_t n)
{
    T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
    if (!p || fread(p, sizeof(T), n, fh) != n) die("short case file");
    return p;
}

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
    if (argc < 3) die("usage: wd_host_main cases.bin results.bin");
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) die("cannot open the case file");
    int32_t head[5], cnx[8], cny[8], ptype[4];
    if (fread(head, 4, 5, fh) != 5 || fread(cnx, 4, 8, fh) != 8 || fread(cny, 4, 8, fh) != 8 ||
        fread(ptype, 4, 4, fh) != 4)
        die("short header");
    const int B = head[0], nx = head[1], ny = head[2], rows = head[3], ld = head[4];
    if (B < 1 || B > LFG_WD_MAX_BANDS) die("bad band count");
    lfg_wd_model M;
    memset(&M, 0, sizeof M);
    M.B = B; M.nx = nx; M.ny = ny;
    double* tx = read_block<double>(fh, nx);
    double* ty = read_block<double>(fh, ny);
    double* c = read_block<double>(fh, size_t(B) * (nx - 4) * (ny - 4));
    M.tx = tx; M.ty = ty; M.c = c;
    double* corr[3 * LFG_WD_MAX_BANDS] = {};
    for (int b = 0; b < B; ++b) {
        if (cnx[b] <= 0) continue;
        M.cnx[b] = cnx[b]; M.cny[b] = cny[b];
        M.ctx[b] = corr[3 * b] = read_block<double>(fh, cnx[b]);
        M.cty[b] = corr[3 * b + 1] = read_block<double>(fh, cny[b]);
        M.cc[b] = corr[3 * b + 2] = read_block<double>(fh, size_t(cnx[b] - 4) * (cny[b] - 4));
    }
    double* s = read_block<double>(fh, 8 * 3 + 1 + 4 * 4);
    for (int b = 0; b < 8; ++b) { M.k[b] = s[b]; M.mag[b] = s[8 + b]; M.err[b] = s[16 + b]; }
    M.lnnorm = s[24];
    for (int d = 0; d < 4; ++d) {
        M.prior_type[d] = ptype[d];
        M.prior_p1[d] = s[25 + d]; M.prior_p2[d] = s[29 + d]; M.prior_c0[d] = s[33 + d]; M.prior_c1[d] = s[37 + d];
    }
    double* theta = read_block<double>(fh, size_t(rows) * ld);
    fclose(fh);

    FILE* out = fopen(argv[2], "wb");
    if (!out) die("cannot open the result file");
    const int counts[4] = {0, 1, 65, 257};
    for (int ci = 0; ci < 4; ++ci) {
        const int n = counts[ci];
        if (n > rows) die("too few rows");
        // the input of exactly n rows: it ends on row n - 1's fourth column
        const size_t used = n ? size_t(n - 1) * ld + 4 : 0;
        double* th = static_cast<double*>(malloc(used ? used * sizeof(double) : 1));
        if (!th) die("out of memory");
        memcpy(th, theta, used * sizeof(double));
        Guarded lp(size_t(n) * sizeof(double)), ll(size_t(n) * sizeof(double));
        Guarded mg(size_t(n) * B * sizeof(double)), st(size_t(n) * sizeof(int));
        const int32_t rc = lfg_cpu_wd_lnprob(th, size_t(ld), n, &M, static_cast<double*>(lp.data()),
                                             static_cast<double*>(ll.data()), static_cast<double*>(mg.data()),
                                             static_cast<int*>(st.data()), ci % 2 ? 4 : 1);
        if (!lp.intact() || !ll.intact() || !mg.intact() || !st.intact()) die("a guard band was written");
        // (a NaN or an infinity the twin writes is never the all-ones fill)
        if (!lp.all_written(sizeof(double)) || !ll.all_written(sizeof(double)) || !mg.all_written(sizeof(double)) ||
            !st.all_written(sizeof(int)))
            die("an output element was left unwritten");
        if (memcmp(th, theta, used * sizeof(double))) die("an input was changed");
        // the nullable outputs left out: lnp alone, and the same bits
        Guarded lp2(size_t(n) * sizeof(double));
        if (lfg_cpu_wd_lnprob(th, size_t(ld), n, &M, static_cast<double*>(lp2.data()), nullptr, nullptr, nullptr, 2) != rc)
            die("the return code depends on the nullable outputs");
        if (!lp2.intact() || memcmp(lp.data(), lp2.data(), lp.bytes)) die("lnp depends on the nullable outputs");
        fwrite(&rc, 4, 1, out);
        fwrite(lp.data(), 1, lp.bytes, out);
        fwrite(ll.data(), 1, ll.bytes, out);
        fwrite(mg.data(), 1, mg.bytes, out);
        fwrite(st.data(), 1, st.bytes, out);
        free(th);
    }
    // argument checks launch nothing and touch nothing
    if (lfg_cpu_wd_lnprob(theta, 3, 1, &M, theta, nullptr, nullptr, nullptr, 1) != LFG_E_ARGS) die("ld < 4 accepted");
    if (lfg_cpu_wd_lnprob(theta, size_t(ld), -1, &M, theta, nullptr, nullptr, nullptr, 1) != LFG_E_ARGS)
        die("n < 0 accepted");
    if (lfg_cpu_wd_lnprob(theta, size_t(ld), 1, nullptr, theta, nullptr, nullptr, nullptr, 1) != LFG_E_ARGS)
        die("a null model accepted");
    if (lfg_cpu_wd_lnprob(nullptr, size_t(ld), 1, &M, nullptr, nullptr, nullptr, nullptr, 1) != LFG_E_ARGS)
        die("null required pointers accepted");
    fclose(out);
    free(tx); free(ty); free(c); free(s); free(theta);
    for (double* p : corr) free(p);
    return 0;
}
