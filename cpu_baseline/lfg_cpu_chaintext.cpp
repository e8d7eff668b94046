// lfg_cpu_chaintext.cpp -- lfg_chain_text's host twin (cpu_baseline/lfg_cpu.h):
// the rules of lfit_python_amd/csrc/lfg_chaintext.hpp, the text the gfx950
// kernels compile, row after row.  A step's bytes are counted first, the
// steps' offsets summed, then every step is written at its place; both loops
// run over the OpenMP threads.  Exact for every double: a finite ln_prob of
// 2^63 and beyond, which the device refuses, goes through snprintf("%f")
// (exact in glibc).
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "lfg_cpu.h"
#include "lfg_chaintext.hpp"

using namespace lfg;

namespace {

struct BufPut {
    unsigned char* p;
    void operator()(int pos, char ch) const { p[pos] = (unsigned char)ch; }
};

// '%f' of x at p (p = NULL: the length alone)
inline int put_fixed(double x, unsigned char* p)
{
    const CtDec d = ct_fixed6(x);
    if (d.kind != CT_REFUSED) {
        if (p) ct_emit(d, BufPut{p});
        return ct_len(d);
    }
    char big[400];  // DBL_MAX has 309 digits before the point
    const int n = snprintf(big, sizeof big, "%f", x);
    if (p) memcpy(p, big, size_t(n));
    return n;
}

// one row at p (p = NULL: its length alone)
inline long long put_row(const double* row, int ndim, double lnp, long long walker, unsigned char* p)
{
    const int wl = ct_walker_len(walker);
    long long n = wl;
    if (p) ct_emit_walker(walker, wl, BufPut{p});
    for (int c = 0; c < ndim; ++c) {
        const CtDec d = ct_repr(row[c]);
        if (p) {
            p[n] = ' ';
            ct_emit(d, BufPut{p + n + 1});
        }
        n += 1 + ct_len(d);
    }
    if (p) p[n] = ' ';
    n += 1;
    n += put_fixed(lnp, p ? p + n : nullptr);
    if (p) p[n] = '\n';
    return n + 1;
}

}  // namespace

extern "C" int lfg_cpu_chain_text(const double* base, long long steps, long long W, int ndim, long long step_ld,
                                  long long walker_ld, const double* lnp, long long lnp_step_ld,
                                  long long lnp_walker_ld, long long walker0, unsigned char* out, size_t out_bytes,
                                  long long* nbytes, int nthreads)
{
    const long long bound = ct_bound(steps, W, ndim, walker0);
    if (bound < 0 || step_ld < 1 || walker_ld < 1 || lnp_step_ld < 1 || lnp_walker_ld < 1 || !nbytes) return LFG_E_ARGS;
    const bool empty = steps == 0 || W == 0;
    if (!empty && (!base || !lnp || !out)) return LFG_E_ARGS;
#ifdef _OPENMP
    const int nt = nthreads > 0 ? nthreads : omp_get_max_threads();
#else
    const int nt = 1;
    (void)nthreads;
#endif
    (void)nt;
    std::vector<long long> off(size_t(steps) + 1, 0);
#pragma omp parallel for schedule(static) num_threads(nt)
    for (long long s = 0; s < steps; ++s) {
        long long n = 0;
        for (long long w = 0; w < W; ++w)
            n += put_row(base + (s * step_ld + w * walker_ld), ndim, lnp[s * lnp_step_ld + w * lnp_walker_ld],
                         walker0 + w, nullptr);
        off[size_t(s) + 1] = n;
    }
    for (long long s = 0; s < steps; ++s) off[size_t(s) + 1] += off[size_t(s)];
    const long long total = off[size_t(steps)];
    // (the device's bound leaves out the rows it refuses; these may be longer)
    if ((unsigned long long)out_bytes < (unsigned long long)total) return LFG_E_ARGS;
#pragma omp parallel for schedule(static) num_threads(nt)
    for (long long s = 0; s < steps; ++s) {
        unsigned char* p = out + off[size_t(s)];
        for (long long w = 0; w < W; ++w)
            p += put_row(base + (s * step_ld + w * walker_ld), ndim, lnp[s * lnp_step_ld + w * lnp_walker_ld],
                         walker0 + w, p);
    }
    nbytes[0] = total;
    nbytes[1] = 0;
    return LFG_OK;
}

// the total alone: what a caller sizes `out` by when ln_prob may hold values
// the bound leaves out
extern "C" long long lfg_cpu_chain_text_bound(long long steps, long long W, int ndim, long long walker0)
{
    return ct_bound(steps, W, ndim, walker0);
}
