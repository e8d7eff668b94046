// lfg_k_misc.hpp -- k_gp, k_wdphases and k_roche, and the host's launch_ok
// and run_front (k_setup then k_elements).  Needs before it: lfg_device.hpp
// (Roche, GPFilter, wdphases), lfg_k_setup.hpp (SetupArgs), lfg_k_elements.hpp
// (ElemSpec, NUNIQ) and lfg_k_front.hpp (the kernels k_setup and k_elements).
// Included by lfg.hip only, in its anonymous namespace.
#pragma once

// ------------------------------------------------------ k_gp, k_wdphases
__device__ __forceinline__ double readlane_f64(double v, int j)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane(int(b), j), hi = __builtin_amdgcn_readlane(int(b >> 32), j);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}

// one wave per residual vector: lanes load 64 points at a time, every lane
// runs the (wave-uniform) filter over them through readlane broadcasts
__global__ __launch_bounds__(64) void k_gp(const double* __restrict__ x, const double* __restrict__ ye,
                                           const double* __restrict__ res, int N, const double* __restrict__ hyp,
                                           const double* __restrict__ blocks, int nb, double* __restrict__ lnlike)
{
    const int w = blockIdx.x, lane = threadIdx.x;
    const double* r = res + size_t(w) * N;
    const double* bk = blocks + size_t(w) * nb * 2;
    GPFilter F;
    F.init(hyp[3 * w], hyp[3 * w + 1], hyp[3 * w + 2]);
    for (int c0 = 0; c0 < N; c0 += 64) {
        const int p = c0 + lane;
        double xv = 0.0, yv = 1.0, rv = 0.0;
        int bv = -1;
        if (p < N) {
            xv = x[p];
            yv = ye[p];
            rv = r[p];
            for (int k = 0; k < nb; ++k)
                if (xv >= bk[2 * k] && xv <= bk[2 * k + 1]) bv = k;
        }
        const int m = min(64, N - c0);
        for (int j = 0; j < m; ++j)
            F.step(readlane_f64(xv, j), readlane_f64(yv, j), readlane_f64(rv, j), __builtin_amdgcn_readlane(bv, j));
    }
    if (lane == 0) lnlike[w] = F.lnlike();
}

__global__ void k_wdphases(const double* __restrict__ q, const double* __restrict__ inc,
                           const double* __restrict__ r1, int n, int ntheta, double* __restrict__ ph3,
                           double* __restrict__ ph4, int* __restrict__ status)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Roche R;
    double a = NAN, b = NAN;
    int st = roche_init(R, q[i]);
    if (st == ST_OK) st = wdphases(R, inc[i], r1[i], ntheta, a, b);
    ph3[i] = (st == ST_OK) ? a : NAN;
    ph4[i] = (st == ST_OK) ? b : NAN;
    status[i] = st;
}

// ---------------------------------------------------------------- k_roche
__global__ void k_roche(int op, const double* __restrict__ a, const double* __restrict__ b, int n,
                        double* __restrict__ out, int* __restrict__ status)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Roche R;
    int st = roche_init(R, a[i]);
    if (op == 0) {
        out[i] = (st == ST_OK) ? R.xl1 : NAN;
    } else if (op == 1) {
        double v = NAN;
        if (st == ST_OK) st = findphi(R, b[i], v);
        out[i] = (st == ST_OK) ? v : NAN;
    } else if (op == 2) {
        double v = NAN;
        if (st == ST_OK) st = findi(R, b[i], v);
        out[i] = (st == ST_OK) ? v : NAN;
    } else {
        double v[4] = {NAN, NAN, NAN, NAN};
        if (st == ST_OK) st = bspot(R, b[i], v);
        if (st != ST_OK) v[0] = v[1] = v[2] = v[3] = NAN;
        for (int m = 0; m < 4; ++m) out[4 * size_t(i) + m] = v[m];
    }
    status[i] = st;
}

inline int launch_ok() { return hipGetLastError() == hipSuccess ? LFG_OK : LFG_E_LAUNCH; }

// record event i of ev (nullable, LFG_NEV events, each nullable) on the stream
inline void mark_event(void* const* ev, int i, hipStream_t st)
{
    if (ev && ev[i]) (void)hipEventRecord(static_cast<hipEvent_t>(ev[i]), st);
}

// k_setup (setup, prior and stream lanes) then k_elements, on the caller's
// stream.  ev (nullable, LFG_NEV events): 0 before k_setup, 1 after k_setup,
// 2 after k_elements
// k_setup (unless the speculative candidates stand in for it) then k_elements
int run_front(const SetupArgs& S, const Ws& ws, hipStream_t st, void* const* ev, bool elements = true,
              const ElemSpec* X = nullptr, bool setup = true)
{
    const int npairs = S.W * S.E;
    const int nlanes = 2 * npairs + S.W;
    mark_event(ev, 0, st);
    if (setup) {
        hipLaunchKernelGGL(k_setup, dim3((nlanes + SETUP_BLOCK - 1) / SETUP_BLOCK), dim3(SETUP_BLOCK), 0, st, S);
        if (launch_ok() != LFG_OK) return LFG_E_LAUNCH;
    }
    mark_event(ev, 1, st);
    if (elements) {
        constexpr int chunks = (NUNIQ + ELEM_BLOCK * LFG_ELEM_IPL - 1) / (ELEM_BLOCK * LFG_ELEM_IPL);
        ElemSpec none{};
        const ElemSpec& XS = X ? *X : none;
        hipLaunchKernelGGL(k_elements, dim3(unsigned(npairs) * chunks + unsigned(XS.nspecblk)), dim3(ELEM_BLOCK), 0,
                           st, ws.geo, ws.status, npairs, ws.ab, ws.donor, ws.wts, ws.bstatus, XS);
        if (launch_ok() != LFG_OK) return LFG_E_LAUNCH;
    }
    mark_event(ev, 2, st);
    return LFG_OK;
}
