// lfg_wd.hip -- the white-dwarf atmosphere fit on gfx950 (include/lfg_wd.h;
// MODEL_SPEC.md section 13).  A unit of its own: nothing here takes part in
// lfg.hip's code generation.
//
// k_wd_lnprob: one lane per row over a grid-stride loop.  The model struct is
// a kernel argument (scalar loads); the spline tables stay in global memory
// and are read through the cache: a lane touches 16 coefficients per band out
// of ~12 KB (+ ~8.5 KB per corrected band), which the vector L1 holds, and
// the 200-walker sampler runs one or two workgroups, where staging 12 KB into
// LDS per launch would cost more loads than the launch makes.
//
// k_wd_step_half: one lane per walker of the half: k_propose's draws and
// arithmetic (lfg_k_stretch.hpp), wd_row, k_accept's draw and rule.  A lane reads rows
// of the other half only, and writes only its own walker's row, so no lane
// waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lfg_wd.hpp"

using namespace lfg;

namespace {

#include "lfg_philox.hpp"  // philox, u53, draw: the samplers' counter layout

constexpr int WD_BLOCK = 256;
constexpr int WD_MAX_BLOCKS = 2048;
constexpr int WD_STEP_BLOCK = 64;

inline int launch_ok() { return hipGetLastError() == hipSuccess ? LFG_OK : LFG_E_LAUNCH; }

__global__ __launch_bounds__(WD_BLOCK) void k_wd_lnprob(const double* __restrict__ theta, size_t ld, int n,
                                                        lfg_wd_model M, double* __restrict__ lnp,
                                                        double* __restrict__ lnlike, double* __restrict__ mags,
                                                        int* __restrict__ status)
{
    const size_t N = size_t(n), stride = size_t(gridDim.x) * WD_BLOCK;
    for (size_t i = size_t(blockIdx.x) * WD_BLOCK + threadIdx.x; i < N; i += stride) {
        const double* th = theta + i * ld;
        double ll;
        int st;
        const double lp = wd_row(M, th[0], th[1], th[2], th[3], ll, st, [&](int b, double mb) {
            if (mags) mags[size_t(b) * N + i] = mb;
        });
        lnp[i] = lp;
        if (lnlike) lnlike[i] = ll;
        if (status) status[i] = st;
    }
}

__global__ __launch_bounds__(WD_STEP_BLOCK) void k_wd_step_half(double* __restrict__ pos, double* __restrict__ lnp,
                                                                int W, int half, double a, unsigned long long seed,
                                                                unsigned long long step,
                                                                const unsigned long long* __restrict__ stepp,
                                                                lfg_wd_model M, double* __restrict__ q,
                                                                double* __restrict__ zfac,
                                                                double* __restrict__ lnp_new,
                                                                int* __restrict__ naccept)
{
    constexpr int ndim = LFG_WD_NPAR;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ns = W / 2;
    if (i >= ns) return;
    if (stepp) step = *stepp;
    // k_propose
    const uint4 r = draw(seed, step, half, 0, i);
    const double u = u53(r.x, r.y);
    const double zr = fma(a - 1.0, u, 1.0);  // (a - 1) u + 1 as k_propose's unit contracts it
    const double z = zr * zr / a;
    const int j = int(__umulhi(r.z, unsigned(ns)));  // partner in the other half
    const int w = half * ns + i;
    double* s = pos + size_t(w) * ndim;
    const double* cj = pos + size_t((1 - half) * ns + j) * ndim;
    double p[ndim];
#pragma unroll
    for (int d = 0; d < ndim; ++d) p[d] = fma(s[d] - cj[d], z, cj[d]);
    const double zf = (ndim - 1.0) * log(z);
    // the model
    double ll;
    int st;
    const double lpn = wd_row(M, p[0], p[1], p[2], p[3], ll, st, [](int, double) {});
    double* out = q + size_t(i) * ndim;
#pragma unroll
    for (int d = 0; d < ndim; ++d) out[d] = p[d];
    zfac[i] = zf;
    lnp_new[i] = lpn;
    // k_accept
    const uint4 r2 = draw(seed, step, half, 1, i);
    const double lu = log(u53(r2.x, r2.y));
    const double diff = zf + lpn - lnp[w];
    if (lu < diff) {
#pragma unroll
        for (int d = 0; d < ndim; ++d) s[d] = p[d];
        lnp[w] = lpn;
        if (naccept) naccept[w] += 1;
    }
}

}  // namespace

extern "C" {

int lfg_wd_lnprob(const double* theta, size_t ld, int n, const lfg_wd_model* model, double* lnp, double* lnlike,
                  double* mags, int* status, void* stream)
{
    if (n < 0 || ld < LFG_WD_NPAR || !wd_model_ok(model)) return LFG_E_ARGS;
    if (n == 0) return LFG_OK;
    if (!theta || !lnp) return LFG_E_ARGS;
    const int blocks = int(std::min<long long>((static_cast<long long>(n) + WD_BLOCK - 1) / WD_BLOCK, WD_MAX_BLOCKS));
    hipLaunchKernelGGL(k_wd_lnprob, dim3(blocks), dim3(WD_BLOCK), 0, static_cast<hipStream_t>(stream), theta, ld, n,
                       *model, lnp, lnlike, mags, status);
    return launch_ok();
}

int lfg_wd_step_half(double* pos, double* lnp, int W, int half, double a, unsigned long long seed,
                     unsigned long long step, const unsigned long long* stepp, const lfg_wd_model* model, double* q,
                     double* zfac, double* lnp_new, int* naccept, void* stream)
{
    if (W < 4 || (W & 1) || (half != 0 && half != 1) || !(a > 1.0) || !pos || !lnp || !q || !zfac || !lnp_new ||
        !wd_model_ok(model))
        return LFG_E_ARGS;
    const int ns = W / 2;
    hipLaunchKernelGGL(k_wd_step_half, dim3((ns + WD_STEP_BLOCK - 1) / WD_STEP_BLOCK), dim3(WD_STEP_BLOCK), 0,
                       static_cast<hipStream_t>(stream), pos, lnp, W, half, a, seed, step, stepp, *model, q, zfac,
                       lnp_new, naccept);
    return launch_ok();
}

}  // extern "C"
