// lfg_physpar.hip -- physical parameters of every chain row on gfx950
// (include/lfg_physpar.h; MODEL_SPEC.md section 12).  A unit of its own:
// nothing here takes part in lfg.hip's code generation.
//
// k_physpar: one lane per row, workgroups persistent over a grid-stride loop.
// Each workgroup stages the mass-radius tables into LDS once (the Wood rows,
// the cardinal cubics, the Hamada table, the Panei knots and coefficients:
// ~32 KB on the shipped tables) and its lanes then only read LDS: the table
// walks are divergent binary searches, which LDS serves per lane where the
// vector cache would serve a line per distinct address.  The per-row
// arithmetic is lfg_physpar.hpp's physpar_row, the text the host twin
// compiles.  A row's cascade picks its model first (at most six evaluations
// of f) and the root-finder then runs one loop whose f dispatches on the
// model, so lanes of different models share the loop's trips; findi runs
// only for rows that found a mass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lfg_physpar.hpp"

using namespace lfg;

namespace {

constexpr int PP_BLOCK = 256;
constexpr int PP_MAX_BLOCKS = 512;  // two workgroups for each of the 256 CUs

inline int launch_ok() { return hipGetLastError() == hipSuccess ? LFG_OK : LFG_E_LAUNCH; }

// where each table lies in LDS, in doubles
struct Layout {
    int wood_t, wood_r, card, ham_m, ham_r, tx, ty, c, total;
};

__host__ __device__ inline Layout layout_of(const lfg_mr_tables& T)
{
    const int nw = T.wood_off[LFG_MR_NWOOD];
    Layout L;
    L.wood_t = 0;
    L.wood_r = L.wood_t + nw;
    L.card = L.wood_r + nw;
    L.ham_m = L.card + (LFG_MR_NWOOD - 1) * LFG_MR_NWOOD * 4;
    L.ham_r = L.ham_m + T.n_ham;
    L.tx = L.ham_r + T.n_ham;
    L.ty = L.tx + T.pan_nx;
    L.c = L.ty + T.pan_ny;
    L.total = L.c + (T.pan_nx - 4) * (T.pan_ny - 4);
    return L;
}

__device__ inline void stage(double* dst, const double* __restrict__ src, int n)
{
    for (int i = threadIdx.x; i < n; i += PP_BLOCK) dst[i] = src[i];
}

__global__ __launch_bounds__(PP_BLOCK) void k_physpar(const double* __restrict__ q, const double* __restrict__ dphi,
                                                      const double* __restrict__ rwd, size_t ld,
                                                      const double* __restrict__ twd, const double* __restrict__ p,
                                                      int n, lfg_mr_tables T, double* __restrict__ out,
                                                      int* __restrict__ model, int* __restrict__ status)
{
    extern __shared__ double lds[];
    const Layout L = layout_of(T);
    const int nw = T.wood_off[LFG_MR_NWOOD];
    stage(lds + L.wood_t, T.wood_t, nw);
    stage(lds + L.wood_r, T.wood_r, nw);
    stage(lds + L.card, T.wood_card, (LFG_MR_NWOOD - 1) * LFG_MR_NWOOD * 4);
    stage(lds + L.ham_m, T.ham_m, T.n_ham);
    stage(lds + L.ham_r, T.ham_r, T.n_ham);
    stage(lds + L.tx, T.pan_tx, T.pan_nx);
    stage(lds + L.ty, T.pan_ty, T.pan_ny);
    stage(lds + L.c, T.pan_c, (T.pan_nx - 4) * (T.pan_ny - 4));
    lfg_mr_tables V = T;
    V.wood_t = lds + L.wood_t;
    V.wood_r = lds + L.wood_r;
    V.wood_card = lds + L.card;
    V.ham_m = lds + L.ham_m;
    V.ham_r = lds + L.ham_r;
    V.pan_tx = lds + L.tx;
    V.pan_ty = lds + L.ty;
    V.pan_c = lds + L.c;
    __syncthreads();

    const size_t N = size_t(n), stride = size_t(gridDim.x) * PP_BLOCK;
    for (size_t i = size_t(blockIdx.x) * PP_BLOCK + threadIdx.x; i < N; i += stride) {
        double o[LFG_PP_NCOL];
        int m;
        const int st = physpar_row(V, q[i * ld], dphi[i * ld], rwd[i * ld], twd[i], p[i], o, m);
#pragma unroll
        for (int c = 0; c < LFG_PP_NCOL; ++c) out[size_t(c) * N + i] = o[c];
        model[i] = m;
        status[i] = st;
    }
}

}  // namespace

// the table limits of lfg_physpar.h; the kernel indexes by these counts alone
static bool tables_ok(const lfg_mr_tables* t)
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
    return layout_of(*t).total <= LFG_MR_MAX_DOUBLES;
}

extern "C" {

int lfg_physpar_lanes(void) { return PP_BLOCK * PP_MAX_BLOCKS; }

int lfg_physpar(const double* q, const double* dphi, const double* rwd, size_t ld, const double* twd, const double* p,
                int n, const lfg_mr_tables* tab, double* out, int* model, int* status, void* stream)
{
    if (n < 0 || ld < 1 || !tables_ok(tab)) return LFG_E_ARGS;
    if (n == 0) return LFG_OK;
    if (!q || !dphi || !rwd || !twd || !p || !out || !model || !status) return LFG_E_ARGS;
    const int blocks = int(std::min<long long>((static_cast<long long>(n) + PP_BLOCK - 1) / PP_BLOCK, PP_MAX_BLOCKS));
    const size_t lds_bytes = size_t(layout_of(*tab).total) * sizeof(double);
    hipLaunchKernelGGL(k_physpar, dim3(blocks), dim3(PP_BLOCK), lds_bytes, static_cast<hipStream_t>(stream), q, dphi,
                       rwd, ld, twd, p, n, *tab, out, model, status);
    return launch_ok();
}

}  // extern "C"
