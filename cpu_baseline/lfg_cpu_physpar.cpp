// lfg_cpu_physpar.cpp -- lfg_physpar's host twin (cpu_baseline/lfg_cpu.h):
// lfit_python_amd/csrc/lfg_physpar.hpp's physpar_row, the text the gfx950
// kernel compiles, run over the rows with OpenMP.  The tables are read where
// the caller holds them (the kernel stages them into LDS first).
#include <omp.h>
#include <stddef.h>

#include "lfg_cpu.h"
#include "lfg_physpar.hpp"

using namespace lfg;

namespace {

// lfg_physpar.hip's tables_ok: the limits of lfg_physpar.h
bool tables_ok(const lfg_mr_tables* t)
{
    if (!t || !t->wood_t || !t->wood_r || !t->wood_card || !t->ham_m || !t->ham_r || !t->pan_tx || !t->pan_ty ||
        !t->pan_c)
        return false;
    if (t->wood_off[0] != 0) return false;
    for (int k = 0; k < LFG_MR_NWOOD; ++k)
        if (t->wood_off[k + 1] - t->wood_off[k] < 2 || t->wood_off[k + 1] > LFG_MR_MAX_DOUBLES) return false;
    if (t->n_ham < 2 || t->n_ham > LFG_MR_MAX_DOUBLES) return false;
    if (t->pan_nx < 8 || t->pan_nx > LFG_MR_MAX_KNOTS || t->pan_ny < 8 || t->pan_ny > LFG_MR_MAX_KNOTS) return false;
    if (!(t->G > 0.0) || !(t->GMsun > 0.0) || !(t->Rsun > 0.0) || !(t->day > 0.0)) return false;
    const long long total = 2LL * t->wood_off[LFG_MR_NWOOD] + (LFG_MR_NWOOD - 1) * LFG_MR_NWOOD * 4 + 2LL * t->n_ham +
                            t->pan_nx + t->pan_ny + (t->pan_nx - 4) * (t->pan_ny - 4);
    return total <= LFG_MR_MAX_DOUBLES;
}

}  // namespace

extern "C" int lfg_cpu_physpar(const double* q, const double* dphi, const double* rwd, size_t ld, const double* twd,
                               const double* p, int n, const lfg_mr_tables* tab, double* out, int* model,
                               int* status, int nthreads)
{
    if (n < 0 || ld < 1 || !tables_ok(tab)) return LFG_E_ARGS;
    if (n == 0) return LFG_OK;
    if (!q || !dphi || !rwd || !twd || !p || !out || !model || !status) return LFG_E_ARGS;
    const int nt = nthreads > 0 ? nthreads : omp_get_max_threads();
    const lfg_mr_tables V = *tab;
    const size_t N = size_t(n);
#pragma omp parallel for schedule(dynamic, 64) num_threads(nt)
    for (long long i = 0; i < static_cast<long long>(N); ++i) {
        double o[LFG_PP_NCOL];
        int m;
        status[i] = physpar_row(V, q[size_t(i) * ld], dphi[size_t(i) * ld], rwd[size_t(i) * ld], twd[i], p[i], o, m);
        for (int c = 0; c < LFG_PP_NCOL; ++c) out[size_t(c) * N + size_t(i)] = o[c];
        model[i] = m;
    }
    return LFG_OK;
}
