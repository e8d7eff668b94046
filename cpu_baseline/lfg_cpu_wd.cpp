// lfg_cpu_wd.cpp -- lfg_wd_lnprob's host twin (cpu_baseline/lfg_cpu.h):
// lfit_python_amd/csrc/lfg_wd.hpp's wd_row, the text the gfx950 kernels
// compile, run over the rows with OpenMP.  The model's arrays are host arrays.
#include <omp.h>
#include <stddef.h>

#include "lfg_cpu.h"
#include "lfg_wd.hpp"

using namespace lfg;

extern "C" int lfg_cpu_wd_lnprob(const double* theta, size_t ld, int n, const lfg_wd_model* model, double* lnp,
                                 double* lnlike, double* mags, int* status, int nthreads)
{
    if (n < 0 || ld < LFG_WD_NPAR || !wd_model_ok(model)) return LFG_E_ARGS;
    if (n == 0) return LFG_OK;
    if (!theta || !lnp) return LFG_E_ARGS;
    const int nt = nthreads > 0 ? nthreads : omp_get_max_threads();
    const lfg_wd_model M = *model;
    const size_t N = size_t(n);
#pragma omp parallel for schedule(static) num_threads(nt)
    for (long long i = 0; i < static_cast<long long>(N); ++i) {
        const double* th = theta + size_t(i) * ld;
        double ll;
        int st;
        lnp[i] = wd_row(M, th[0], th[1], th[2], th[3], ll, st, [&](int b, double mb) {
            if (mags) mags[size_t(b) * N + size_t(i)] = mb;
        });
        if (lnlike) lnlike[i] = ll;
        if (status) status[i] = st;
    }
    return LFG_OK;
}
