// lfg_gp_predict.hip -- the GP's posterior on gfx950 (include/lfg.h,
// lfg_gp_predict / lfg_gp_sample; MODEL_SPEC 10.5): conditional mean and
// variance of the kernel SimpleGPEclipse.create_GP builds, at every point of
// a merged grid of data and test phases, and conditional draws by Matheron's
// rule.  Exact and O(n) per residual vector: GPForward, then the modified
// Bryson-Frazier pass GPBackward (lfg_device.hpp).  A unit of its own:
// nothing here takes part in lfg.hip's code generation.
//
// k_gp_smooth<SAMPLE, VAR>: one lane per vector, one wave per workgroup.
// The recursion is serial in the points and independent across vectors; x,
// ye and obs are wave-uniform (scalar loads).
//   forward   tiles of 64 vectors x GP_TP points of res[V][n] come in through
//             LDS (coalesced along n, transposed for the lanes); each point
//             leaves its GPRecord in the workspace, point-major
//             [n][NREC][V padded to 64], so both passes read and write whole
//             rows of 64 lanes
//   backward  the records last point first; mean and var leave through the
//             same LDS tiles
// SAMPLE: vector v = (row v / S, draw v % S); the forward pass simulates a
// prior path over the grid, filters r - f*_obs - eps, and keeps f* as an
// eighth record; the backward pass is mean-only and adds f*.
//
// k_gp_smooth_tree: the same two passes over every (walker, eclipse) pair of
// a GP tree after lfg_lnprob's kernels have left the pairs' residuals, block
// indices and hyper-parameters in the workspace; a wave is 64 walkers of one
// eclipse, so x and ye stay wave-uniform.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfg.h"
#include "lfg_device.hpp"

using namespace lfg;

namespace {

#include "lfg_philox.hpp"

constexpr int GP_TP = 32;          // points per LDS tile
constexpr int GP_TS = 65;          // tile row stride (64 lanes + 1: no bank conflicts on the transposed side)
constexpr size_t GP_MAX_V = size_t(1) << 30;

inline int launch_ok() { return hipGetLastError() == hipSuccess ? LFG_OK : LFG_E_LAUNCH; }
inline size_t pad64(size_t v) { return (v + 63) & ~size_t(63); }

struct SmoothArgs {
    const double* x;
    const double* ye;
    const int* obs;
    const double* res;
    int V, n, S;
    const double* hyp;
    const double* blocks;
    int nb;
    double* mean;
    double* var;
    int* status;
    double* rec;
    size_t Vpad;
    unsigned long long seed;
    unsigned first;  // SAMPLE: the key's vector index of row 0
};

// two standard normals from one Philox block (Box-Muller)
__device__ inline void normal2(uint4 r, double& a, double& b)
{
    const double rad = sqrt(-2.0 * log(1.0 - u53(r.x, r.y)));  // 1 - u in (0, 1]
    double s, c;
    sincospi(2.0 * u53(r.z, r.w), &s, &c);
    a = rad * c;
    b = rad * s;
}

// a point's record in the workspace: field c of vector v at q[c * stride]
__device__ inline void store_rec(double* q, size_t stride, const GPRecord& o)
{
    q[0] = o.k0;
    q[stride] = o.k1;
    q[2 * stride] = o.k2;
    q[3 * stride] = o.k3;
    q[4 * stride] = o.S;
    q[5 * stride] = o.v;
    q[6 * stride] = o.yhat;
}

// (the backward passes load point p - 1's record before they work on point
// p's, so the loads wait behind the step's dependent chain: 2-4 % of a call,
// the chain itself is what a call costs)
__device__ inline void load_rec(const double* q, size_t stride, GPRecord& o, double& extra, bool with_extra)
{
    o.k0 = q[0];
    o.k1 = q[stride];
    o.k2 = q[2 * stride];
    o.k3 = q[3 * stride];
    o.S = q[4 * stride];
    o.v = q[5 * stride];
    o.yhat = q[6 * stride];
    if (with_extra) extra = q[7 * stride];
}

template <bool SAMPLE, bool VAR>
__global__ __launch_bounds__(64) void k_gp_smooth(SmoothArgs A)
{
    constexpr int NREC = SAMPLE ? 8 : 7;
    __shared__ double tm[GP_TP * GP_TS];
    __shared__ double tv[VAR ? GP_TP * GP_TS : 1];
    extern __shared__ double sblk[];  // [nb][2][64]: the lanes' block intervals
    const int lane = threadIdx.x, n = A.n, nb = A.nb;
    const size_t v0 = size_t(blockIdx.x) * 64, v = v0 + lane;
    // lanes past V shadow row 0: they compute, and write to the padding of rec only
    const size_t row = v < size_t(A.V) ? (SAMPLE ? v / size_t(A.S) : v) : 0;
    const unsigned smp = SAMPLE ? unsigned(v - row * size_t(A.S)) : 0u;
    for (int k = 0; k < nb; ++k) {
        sblk[(2 * k) * 64 + lane] = A.blocks[(row * nb + k) * 2];
        sblk[(2 * k + 1) * 64 + lane] = A.blocks[(row * nb + k) * 2 + 1];
    }
    auto blk_of = [&](double xv) {
        int b = -1;
        for (int k = 0; k < nb; ++k)
            if (xv >= sblk[(2 * k) * 64 + lane] && xv <= sblk[(2 * k + 1) * 64 + lane]) b = k;
        return b;
    };
    double* rec = A.rec + v;

    GPForward F;
    F.init(A.hyp[3 * row], A.hyp[3 * row + 1], A.hyp[3 * row + 2]);
    const double sa_in = sqrt(F.ain), sa_out = sqrt(F.aout);
    double sg0 = 0.0, sg1 = 0.0, sh0 = 0.0, sh1 = 0.0;  // SAMPLE: the prior path's state
    for (int p0 = 0; p0 < n; p0 += GP_TP) {
        const int p1 = min(p0 + GP_TP, n);
        for (int idx = lane; idx < 64 * GP_TP; idx += 64) {
            const int vv = idx / GP_TP, pp = idx % GP_TP;
            const size_t gv = v0 + vv;
            if (gv < size_t(A.V) && p0 + pp < p1)
                tm[pp * GP_TS + vv] = A.res[(SAMPLE ? gv / size_t(A.S) : gv) * n + p0 + pp];
        }
        __syncthreads();
        for (int p = p0; p < p1; ++p) {
            const double xv = A.x[p], yv = A.ye[p];
            const bool ob = A.obs[p] != 0;
            double r = (v < size_t(A.V)) ? tm[(p - p0) * GP_TS + lane] : 0.0;
            const int blk = blk_of(xv);
            double f = 0.0;
            if (SAMPLE) {
                const uint2 key = make_uint2(unsigned(A.seed), unsigned(A.seed >> 32));
                const unsigned vkey = A.first + unsigned(row);
                double z0, z1, z2, z3, z4, z5;
                normal2(philox(make_uint4(unsigned(p), smp, vkey, 0u), key), z0, z1);
                normal2(philox(make_uint4(unsigned(p), smp, vkey, 1u), key), z2, z3);
                normal2(philox(make_uint4(unsigned(p), smp, vkey, 2u), key), z4, z5);
                if (p == 0) {
                    sg0 = sa_in * z0;
                    sg1 = sa_in * F.lam * z1;
                    sh0 = sa_out * z2;
                    sh1 = sa_out * F.lam * z3;
                } else {
                    const double d = xv - F.xp, u = F.lam * d, e = exp(-u);
                    const double f00 = e * (1.0 + u), f01 = e * d, f10 = -e * F.lam * u, f11 = e * (1.0 - u);
                    double c00, c10, c11;
                    gp_step_noise(F.lam, d, c00, c10, c11);
                    double t = f00 * sg0 + f01 * sg1 + sa_in * (c00 * z0);
                    sg1 = f10 * sg0 + f11 * sg1 + sa_in * (c10 * z0 + c11 * z1);
                    sg0 = t;
                    t = f00 * sh0 + f01 * sh1 + sa_out * (c00 * z2);
                    sh1 = f10 * sh0 + f11 * sh1 + sa_out * (c10 * z2 + c11 * z3);
                    sh0 = t;
                }
                if (blk >= 0 && blk != F.bp && p > 0) {  // a block opens: a fresh stationary h
                    sh0 = sa_out * z2;
                    sh1 = sa_out * F.lam * z3;
                }
                f = sg0 + (blk >= 0 ? sh0 : 0.0);
                r -= f + yv * z4;
            }
            GPRecord o;
            F.step(xv, yv, r, blk, ob, o);
            double* q = rec + size_t(p) * NREC * A.Vpad;
            store_rec(q, A.Vpad, o);
            if (SAMPLE) q[7 * A.Vpad] = f;
        }
        __syncthreads();
    }
    const bool bad = F.bad;
    if (v < size_t(A.V) && smp == 0) A.status[row] = bad ? 1 : 0;

    GPBackward<VAR> B;
    B.init();
    int bcur = blk_of(A.x[n - 1]);
    GPRecord nxt;
    double nxf = 0.0;
    load_rec(rec + size_t(n - 1) * NREC * A.Vpad, A.Vpad, nxt, nxf, SAMPLE);
    for (int p0 = ((n - 1) / GP_TP) * GP_TP; p0 >= 0; p0 -= GP_TP) {
        const int p1 = min(p0 + GP_TP, n);
        for (int p = p1 - 1; p >= p0; --p) {
            const GPRecord o = nxt;
            const double fstar = nxf;
            if (p > 0) load_rec(rec + size_t(p - 1) * NREC * A.Vpad, A.Vpad, nxt, nxf, SAMPLE);
            double mean, var = 0.0;
            B.point(o, bcur >= 0, A.obs[p] != 0, mean, var);
            if (SAMPLE) mean += fstar;
            tm[(p - p0) * GP_TS + lane] = bad ? NAN : mean;
            if (VAR) tv[(p - p0) * GP_TS + lane] = bad ? NAN : var;
            if (p > 0) {
                const double xq = A.x[p - 1];
                const int bprev = blk_of(xq);
                B.carry(F.lam, A.x[p] - xq, bcur >= 0 && bcur != bprev);
                bcur = bprev;
            }
        }
        __syncthreads();
        for (int idx = lane; idx < 64 * GP_TP; idx += 64) {
            const int vv = idx / GP_TP, pp = idx % GP_TP;
            const size_t gv = v0 + vv;
            if (gv < size_t(A.V) && p0 + pp < p1) {
                A.mean[gv * n + p0 + pp] = tm[pp * GP_TS + vv];
                if (VAR) A.var[gv * n + p0 + pp] = tv[pp * GP_TS + vv];
            }
        }
        __syncthreads();
    }
}

struct TreeArgs {
    const double* geo;   // [pairs][LFG_NGEO]
    const int* status;   // [pairs]
    const double* prior; // [W]
    const double* res;   // [pairs][max_n]
    const int* gpb;      // [pairs][max_n]
    int W, E, max_n;
    const int* off;
    const double* x;
    const double* y;
    const double* ye;
    double* flux;
    double* mean;
    double* var;
    int* wstatus;
    double* rec;         // [E][max_n][8][Wpad]
    size_t Wpad;
};

// per-walker status of lfg_gp_predict_tree beyond the model's LFG_ST_* codes
constexpr int GP_ST_PRIOR = 6, GP_ST_GP = 7;

__global__ __launch_bounds__(64) void k_gp_smooth_tree(TreeArgs A)
{
    constexpr int NREC = 8;  // GPRecord + (in a block | 2 * opens a block)
    __shared__ double tm[GP_TP * GP_TS];
    __shared__ double tv[GP_TP * GP_TS];
    __shared__ int tb[GP_TP * GP_TS];
    __shared__ int sbad[64];
    const int lane = threadIdx.x, nwb = int(A.Wpad / 64);
    const int e = int(blockIdx.x) / nwb, w0 = (int(blockIdx.x) - e * nwb) * 64, w = w0 + lane;
    const bool live = w < A.W;
    const size_t pair = size_t(live ? w : 0) * A.E + e;  // lanes past W shadow walker 0
    const int o0 = A.off ? A.off[e] : 0;
    const int n = A.off ? A.off[e + 1] - o0 : A.max_n;
    const int ntot = A.off ? A.off[A.E] : A.max_n;
    if (n <= 0) return;  // (uniform)
    const double* G = A.geo + pair * LFG_NGEO;
    const int mst = A.status[pair];
    const bool rej = !(A.prior[live ? w : 0] + G[G_RPRIOR] + G[G_RPRIOR_BS] > -INFINITY);
    const bool ok = mst == ST_OK && !rej && G[G_GP_OK] != 0.0;  // k_gp_like's test: the pair's tables were written
    const double* xs = A.x + o0;
    const double* yes = A.ye + o0;
    double* rec = A.rec + size_t(e) * A.max_n * NREC * A.Wpad + w;

    GPForward F;
    F.init(G[G_GP_AIN], G[G_GP_AOUT], 1.0);
    F.lam = G[G_GP_LAM];
    F.bad = F.bad || !ok;
    for (int p0 = 0; p0 < n; p0 += GP_TP) {
        const int p1 = min(p0 + GP_TP, n);
        for (int idx = lane; idx < 64 * GP_TP; idx += 64) {
            const int vv = idx / GP_TP, pp = idx % GP_TP;
            if (w0 + vv < A.W && p0 + pp < p1) {
                const size_t src = (size_t(w0 + vv) * A.E + e) * A.max_n + p0 + pp;
                tm[pp * GP_TS + vv] = A.res[src];
                tb[pp * GP_TS + vv] = A.gpb[src];
            }
        }
        __syncthreads();
        for (int p = p0; p < p1; ++p) {
            const double r = live ? tm[(p - p0) * GP_TS + lane] : 0.0;
            const int blk = live ? tb[(p - p0) * GP_TS + lane] : -1;
            const int flag = (blk >= 0 ? 1 : 0) | ((blk >= 0 && blk != F.bp) ? 2 : 0);
            GPRecord o;
            F.step(xs[p], yes[p], r, blk, true, o);
            double* q = rec + size_t(p) * NREC * A.Wpad;
            store_rec(q, A.Wpad, o);
            q[7 * A.Wpad] = double(flag);
        }
        __syncthreads();
    }
    const bool bad = F.bad;
    sbad[lane] = bad;
    if (live && bad) atomicMax(A.wstatus + w, mst != ST_OK ? mst : (rej ? GP_ST_PRIOR : GP_ST_GP));

    GPBackward<true> B;
    B.init();
    GPRecord nxt;
    double nxflag = 0.0;
    load_rec(rec + size_t(n - 1) * NREC * A.Wpad, A.Wpad, nxt, nxflag, true);
    for (int p0 = ((n - 1) / GP_TP) * GP_TP; p0 >= 0; p0 -= GP_TP) {
        const int p1 = min(p0 + GP_TP, n);
        for (int p = p1 - 1; p >= p0; --p) {
            const GPRecord o = nxt;
            const int flag = int(nxflag);
            if (p > 0) load_rec(rec + size_t(p - 1) * NREC * A.Wpad, A.Wpad, nxt, nxflag, true);
            double mean, var;
            B.point(o, (flag & 1) != 0, true, mean, var);
            tm[(p - p0) * GP_TS + lane] = mean;
            tv[(p - p0) * GP_TS + lane] = var;
            if (p > 0) B.carry(F.lam, xs[p] - xs[p - 1], (flag & 2) != 0);
        }
        __syncthreads();
        for (int idx = lane; idx < 64 * GP_TP; idx += 64) {
            const int vv = idx / GP_TP, pp = idx % GP_TP;
            if (w0 + vv < A.W && p0 + pp < p1) {
                const size_t dst = size_t(w0 + vv) * ntot + o0 + p0 + pp;
                const bool nan = sbad[vv] != 0;
                A.mean[dst] = nan ? NAN : tm[pp * GP_TS + vv];
                if (A.var) A.var[dst] = nan ? NAN : tv[pp * GP_TS + vv];
                if (A.flux)
                    A.flux[dst] = nan ? NAN : A.y[o0 + p0 + pp] - A.res[(size_t(w0 + vv) * A.E + e) * A.max_n + p0 + pp];
            }
        }
        __syncthreads();
    }
}

// a walker any of whose eclipses failed has ln_prob = -inf as a whole
// (Node.ln_prob): all its rows are NaN, not those eclipses' alone
__global__ __launch_bounds__(256) void k_gp_nan_rows(const int* __restrict__ wstatus, const int* __restrict__ off, int E,
                                                     int max_n, double* __restrict__ flux, double* __restrict__ mean,
                                                     double* __restrict__ var)
{
    const int w = blockIdx.x;
    if (wstatus[w] == 0) return;
    const int ntot = off ? off[E] : max_n;
    for (int p = threadIdx.x; p < ntot; p += 256) {
        mean[size_t(w) * ntot + p] = NAN;
        if (var) var[size_t(w) * ntot + p] = NAN;
        if (flux) flux[size_t(w) * ntot + p] = NAN;
    }
}

bool bad_common(const double* x, const double* ye, const int* obs, const double* res, int W, int n,
                const double* hyp, const double* blocks, int nb, const int* status, const void* ws)
{
    return W <= 0 || n <= 0 || nb < 0 || nb > LFG_GP_PREDICT_MAX_NB || !x || !ye || !obs || !res || !hyp ||
           (nb > 0 && !blocks) || !status || !ws;
}

inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

}  // namespace

extern "C" {

// lfg.hip: where lfg_lnprob leaves a GP tree's pairs in its workspace
int lfg_tree_gp_views(void* wsp, int W, const lfg_tree* T, const double** geo, const int** status,
                      const double** prior, const double** res, const int** gpb);

size_t lfg_gp_predict_workspace_size(int W, int n)
{
    if (W <= 0 || n <= 0 || size_t(W) > GP_MAX_V) return 0;
    return size_t(7) * size_t(n) * pad64(size_t(W)) * sizeof(double);
}

size_t lfg_gp_sample_workspace_size(int W, int n, int S)
{
    if (W <= 0 || n <= 0 || S <= 0 || size_t(W) * size_t(S) > GP_MAX_V) return 0;
    return size_t(8) * size_t(n) * pad64(size_t(W) * size_t(S)) * sizeof(double);
}

int lfg_gp_predict(const double* x, const double* ye, const int* obs, const double* res, int W, int n,
                   const double* hyp, const double* blocks, int nb, double* mean, double* var, int* status,
                   void* ws, size_t ws_bytes, void* stream)
{
    if (bad_common(x, ye, obs, res, W, n, hyp, blocks, nb, status, ws) || !mean) return LFG_E_ARGS;
    const size_t need = lfg_gp_predict_workspace_size(W, n);
    if (need == 0 || ws_bytes < need) return LFG_E_ARGS;
    SmoothArgs A{x, ye, obs, res, W, n, 1, hyp, blocks, nb, mean, var, status, static_cast<double*>(ws),
                 pad64(size_t(W)), 0ull, 0u};
    const dim3 grid(unsigned(pad64(size_t(W)) / 64));
    const size_t lds = size_t(nb) * 2 * 64 * sizeof(double);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (var)
        hipLaunchKernelGGL((k_gp_smooth<false, true>), grid, dim3(64), lds, st, A);
    else
        hipLaunchKernelGGL((k_gp_smooth<false, false>), grid, dim3(64), lds, st, A);
    return launch_ok();
}

int lfg_gp_sample(const double* x, const double* ye, const int* obs, const double* res, int W, int n,
                  const double* hyp, const double* blocks, int nb, int S, unsigned long long seed, int first,
                  double* out, int* status, void* ws, size_t ws_bytes, void* stream)
{
    if (bad_common(x, ye, obs, res, W, n, hyp, blocks, nb, status, ws) || !out || S <= 0 || first < 0)
        return LFG_E_ARGS;
    const size_t need = lfg_gp_sample_workspace_size(W, n, S);
    if (need == 0 || ws_bytes < need) return LFG_E_ARGS;
    const size_t V = size_t(W) * size_t(S);
    SmoothArgs A{x, ye, obs, res, int(V), n, S, hyp, blocks, nb, out, nullptr, status, static_cast<double*>(ws),
                 pad64(V), seed, unsigned(first)};
    hipLaunchKernelGGL((k_gp_smooth<true, false>), dim3(unsigned(pad64(V) / 64)), dim3(64),
                       size_t(nb) * 2 * 64 * sizeof(double), static_cast<hipStream_t>(stream), A);
    return launch_ok();
}

size_t lfg_gp_predict_tree_workspace_size(int W, const lfg_tree* T)
{
    if (W <= 0 || !T || T->E <= 0 || !T->gp || T->max_n <= 0) return 0;
    const size_t front = lfg_workspace_size_tree(W, T);
    if (front == 0) return 0;
    return align256(front) + align256(size_t(W) * sizeof(double)) +
           size_t(8) * size_t(T->E) * size_t(T->max_n) * pad64(size_t(W)) * sizeof(double);
}

int lfg_gp_predict_tree(const double* walkers, int W, const lfg_tree* T, double* flux, double* mean, double* var,
                        int* status, void* ws, size_t ws_bytes, void* stream)
{
    if (!walkers || W <= 0 || !T || T->E <= 0 || T->ndim <= 0 || !T->gp || T->max_n <= 0 || !mean || !status || !ws)
        return LFG_E_ARGS;
    const size_t need = lfg_gp_predict_tree_workspace_size(W, T);
    if (need == 0 || ws_bytes < need) return LFG_E_ARGS;
    const size_t front = align256(lfg_workspace_size_tree(W, T));
    char* base = static_cast<char*>(ws);
    double* lnp = reinterpret_cast<double*>(base + front);
    double* rec = reinterpret_cast<double*>(base + front + align256(size_t(W) * sizeof(double)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the tree's own front, in whichever layout is active: it leaves every
    // pair's residuals, block indices and hyper-parameters in the workspace
    int rc = lfg_lnprob(walkers, W, T, lnp, nullptr, ws, front, stream);
    if (rc) return rc;
    TreeArgs A{};
    if ((rc = lfg_tree_gp_views(ws, W, T, &A.geo, &A.status, &A.prior, &A.res, &A.gpb))) return rc;
    A.W = W;
    A.E = T->E;
    A.max_n = T->max_n;
    A.off = T->off;
    A.x = T->x;
    A.y = T->y;
    A.ye = T->ye;
    A.flux = flux;
    A.mean = mean;
    A.var = var;
    A.wstatus = status;
    A.rec = rec;
    A.Wpad = pad64(size_t(W));
    if (hipMemsetAsync(status, 0, size_t(W) * sizeof(int), st) != hipSuccess) return LFG_E_LAUNCH;
    hipLaunchKernelGGL(k_gp_smooth_tree, dim3(unsigned(size_t(T->E) * (A.Wpad / 64))), dim3(64), 0, st, A);
    if ((rc = launch_ok())) return rc;
    hipLaunchKernelGGL(k_gp_nan_rows, dim3(W), dim3(256), 0, st, status, T->off, T->E, T->max_n, flux, mean, var);
    return launch_ok();
}

}  // extern "C"
