// lfg_pt.hip -- parallel-tempered ensemble sampler (gfx950): the stretch
// move of every temperature level in one launch, the tempered Metropolis
// step, and the temperature swaps (include/lfg.h, lfg_pt_*).  A unit of its
// own: nothing here takes part in lfg.hip's code generation.
//
// One iteration = half 0, half 1, swaps.  A half-step is
//   k_pt_propose  one wave per (level, walker of the half): proposal row
//   lfg_lnprob    of all T * W/2 proposals (the caller's call, with lnlike_e)
//   k_pt_accept   one wave per proposal: ln u < zfac + beta dlnl + dlnpr
// and the swap phase three launches whatever T and W are:
//   k_pt_perm     one workgroup per (pair, side): the side's random
//                 permutation, a bitonic sort of (key << 32 | slot) in LDS,
//                 and the pair's ln u_k
//   k_pt_walk     one workgroup: the T - 1 pairs in order (pair i - 1 sees
//                 pair i's result) over lnl, lnpr and a slot-origin map
//   k_pt_gather   one wave per slot: its row from the origin slot into the
//                 second position buffer (rows move once per iteration)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfg.h"

namespace {

#include "lfg_philox.hpp"

constexpr int PT_WAVES = 4;        // waves (walkers) per block of the row kernels
constexpr int PT_SORT_MAX = 1024;  // lanes of a sort / walk workgroup

inline int launch_ok() { return hipGetLastError() == hipSuccess ? LFG_OK : LFG_E_LAUNCH; }

// the swap draw of (pair level, slot k): x, y the sort keys of the two
// permutations, (z, w) the uniform of the k-th exchange
__device__ inline uint4 swap_draw(unsigned long long seed, unsigned long long step, int level, int k)
{
    return philox(make_uint4(unsigned(k), unsigned(step), unsigned(step >> 32), 4u + unsigned(level)),
                  make_uint2(unsigned(seed), unsigned(seed >> 32)));
}

// k_propose for every level at once: proposal g = t * W/2 + i is walker i of
// half `half` of level t against a partner of that level's other half
__global__ __launch_bounds__(64 * PT_WAVES) void k_pt_propose(const double* __restrict__ pos, int T, int W, int ndim,
                                                              int half, double a, unsigned long long seed,
                                                              unsigned long long step, double* __restrict__ q,
                                                              double* __restrict__ zfac)
{
    const int g = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * PT_WAVES + int(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int ns = W / 2;
    if (g >= T * ns) return;
    const int t = g / ns, i = g - t * ns;
    const uint4 r = draw(seed, step, half, 0, g);
    const double u = u53(r.x, r.y);
    const double zr = (a - 1.0) * u + 1.0;
    const double z = zr * zr / a;
    const int j = int(__umulhi(r.z, unsigned(ns)));  // partner in the other half
    const double* s = pos + (size_t(t) * W + size_t(half * ns + i)) * ndim;
    const double* cj = pos + (size_t(t) * W + size_t((1 - half) * ns + j)) * ndim;
    double* out = q + size_t(g) * ndim;
    for (int d = lane; d < ndim; d += 64) out[d] = fma(s[d] - cj[d], z, cj[d]);  // c_j + z (s - c_j)
    if (lane == 0) zfac[g] = (ndim - 1.0) * log(z);
}

// tempered Metropolis step: lnl' = sum_e lnlike_e, lnpr' = lnp' - lnl';
// a proposal whose ln_prob is not finite is rejected whatever lnlike_e holds
__global__ __launch_bounds__(64 * PT_WAVES) void k_pt_accept(double* __restrict__ pos, double* __restrict__ lnl,
                                                             double* __restrict__ lnpr, int T, int W, int ndim,
                                                             int half, const double* __restrict__ betas,
                                                             const double* __restrict__ q,
                                                             const double* __restrict__ zfac,
                                                             const double* __restrict__ lnp_new,
                                                             const double* __restrict__ lnlike_e, int E,
                                                             unsigned long long seed, unsigned long long step,
                                                             int* __restrict__ naccept)
{
    const int g = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * PT_WAVES + int(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int ns = W / 2;
    if (g >= T * ns) return;
    const int t = g / ns, i = g - t * ns;
    const size_t w = size_t(t) * W + size_t(half * ns + i);
    const double lp = lnp_new[g];
    if (!isfinite(lp)) return;
    double ll = 0.0;
    for (int e = 0; e < E; ++e) ll += lnlike_e[size_t(g) * E + e];
    const double lpr = lp - ll;
    const uint4 r = draw(seed, step, half, 1, g);
    const double lu = log(u53(r.x, r.y));
    const double diff = zfac[g] + betas[t] * (ll - lnl[w]) + (lpr - lnpr[w]);
    if (!(lu < diff)) return;
    double* p = pos + w * ndim;
    const double* qi = q + size_t(g) * ndim;
    for (int d = lane; d < ndim; d += 64) p[d] = qi[d];
    if (lane == 0) {
        lnl[w] = ll;
        lnpr[w] = lpr;
        if (naccept) naccept[w] += 1;
    }
}

// block b = (pair - 1) * 2 + side: side 0 the permutation A of level `pair`
// (keys r.x), side 1 the permutation B of level pair - 1 (keys r.y); the
// stable argsort of the W keys = a sort of the distinct (key << 32 | slot),
// padded to P = 2^k >= W with ~0 (above every real entry).  perm[b * W + k].
// Side 0 also leaves ln u_k of its pair in lnu[(pair - 1) * W + k], so the
// serial walk below has no Philox round or log on its chain, and all the
// blocks together set the slot-origin map org[s] = s of the T * W slots
__global__ __launch_bounds__(PT_SORT_MAX) void k_pt_perm(int T, int W, int P, unsigned long long seed,
                                                         unsigned long long step, int* __restrict__ perm,
                                                         double* __restrict__ lnu, int* __restrict__ org)
{
    extern __shared__ unsigned long long keys[];
    const int b = blockIdx.x, level = b / 2 + 1, side = b & 1;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int s = b * nt + tid; s < T * W; s += int(gridDim.x) * nt) org[s] = s;
    for (int k = tid; k < P; k += nt) {
        unsigned long long key = ~0ull;
        if (k < W) {
            const uint4 r = swap_draw(seed, step, level, k);
            key = (static_cast<unsigned long long>(side ? r.y : r.x) << 32) | unsigned(k);
            if (side == 0) lnu[size_t(level - 1) * W + k] = log(u53(r.z, r.w));
        }
        keys[k] = key;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int c = tid; c < P / 2; c += nt) {
                const int lo = 2 * c - (c & (stride - 1)), hi = lo + stride;  // bit `stride` clear / set
                const unsigned long long x = keys[lo], y = keys[hi];
                if ((x > y) == ((lo & size) == 0)) {
                    keys[lo] = y;
                    keys[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    for (int k = tid; k < W; k += nt) perm[size_t(b) * W + k] = int(unsigned(keys[k]));
}

// the pairs in order, by one workgroup: within a pair the W exchanges touch
// disjoint slots (A and B are permutations), between pairs a barrier.  Only
// scalars move here: lnl, lnpr and org (the slot of the iteration's start
// whose row ends in each slot; k_pt_perm set it to the identity).  nswap[2 i], nswap[2 i + 1]: exchanges
// proposed and accepted between levels i and i - 1
__global__ __launch_bounds__(PT_SORT_MAX) void k_pt_walk(double* lnl, double* lnpr, int T, int W,
                                                         const double* __restrict__ betas,
                                                         const int* __restrict__ perm,
                                                         const double* __restrict__ lnu, int* org,
                                                         unsigned long long* nswap)
{
    __shared__ unsigned nacc;
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) nacc = 0;
    __syncthreads();
    for (int i = T - 1; i >= 1; --i) {
        const int* A = perm + size_t(i - 1) * 2 * W;
        const int* B = A + W;
        const double db = betas[i - 1] - betas[i];
        unsigned mine = 0;
        for (int k = tid; k < W; k += nt) {
            const int sa = i * W + A[k], sb = (i - 1) * W + B[k];
            const double la = lnl[sa], lb = lnl[sb];
            if (lnu[size_t(i - 1) * W + k] < db * (la - lb)) {
                lnl[sa] = lb;
                lnl[sb] = la;
                const double pa = lnpr[sa];
                lnpr[sa] = lnpr[sb];
                lnpr[sb] = pa;
                const int oa = org[sa];
                org[sa] = org[sb];
                org[sb] = oa;
                ++mine;
            }
        }
        if (mine) atomicAdd(&nacc, mine);
        __syncthreads();
        if (tid == 0) {
            nswap[2 * i] += static_cast<unsigned long long>(W);
            nswap[2 * i + 1] += nacc;
            nacc = 0;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64 * PT_WAVES) void k_pt_gather(const double* __restrict__ pin, double* __restrict__ pout,
                                                             const int* __restrict__ org, int n, int ndim)
{
    const int s = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * PT_WAVES + int(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (s >= n) return;
    const double* src = pin + size_t(org[s]) * ndim;
    double* dst = pout + size_t(s) * ndim;
    for (int d = lane; d < ndim; d += 64) dst[d] = src[d];
}

// T levels of W walkers: W even, 4 <= W <= LFG_PT_MAX_W (the LDS sort),
// T * W <= 2^30 (int slot numbers, 32-bit Philox walker counter)
inline bool shape_ok(int T, int W, int ndim)
{
    return T >= 1 && W >= 4 && !(W & 1) && W <= LFG_PT_MAX_W && ndim >= 1 &&
           static_cast<long long>(T) * W <= (1ll << 30);
}

inline size_t perm_ints(int T, int W) { return size_t(T - 1) * 2 * size_t(W); }

}  // namespace

extern "C" {

size_t lfg_pt_workspace_size(int T, int W)
{
    if (!shape_ok(T, W, 1)) return 0;
    return ((perm_ints(T, W) + size_t(T) * W) * sizeof(int) + size_t(T - 1) * W * sizeof(double) + 255) & ~size_t(255);
}

int lfg_pt_propose(const double* pos, int T, int W, int ndim, int half, double a, unsigned long long seed,
                   unsigned long long step, double* q, double* zfac, void* stream)
{
    if (!shape_ok(T, W, ndim) || (half != 0 && half != 1) || !(a > 1.0) || !pos || !q || !zfac) return LFG_E_ARGS;
    const int n = T * (W / 2);
    hipLaunchKernelGGL(k_pt_propose, dim3((n + PT_WAVES - 1) / PT_WAVES), dim3(64 * PT_WAVES), 0,
                       static_cast<hipStream_t>(stream), pos, T, W, ndim, half, a, seed, step, q, zfac);
    return launch_ok();
}

int lfg_pt_accept(double* pos, double* lnl, double* lnpr, int T, int W, int ndim, int half, const double* betas,
                  const double* q, const double* zfac, const double* lnp_new, const double* lnlike_e, int E,
                  unsigned long long seed, unsigned long long step, int* naccept, void* stream)
{
    if (!shape_ok(T, W, ndim) || (half != 0 && half != 1) || E < 1 || !pos || !lnl || !lnpr || !betas || !q ||
        !zfac || !lnp_new || !lnlike_e)
        return LFG_E_ARGS;
    const int n = T * (W / 2);
    hipLaunchKernelGGL(k_pt_accept, dim3((n + PT_WAVES - 1) / PT_WAVES), dim3(64 * PT_WAVES), 0,
                       static_cast<hipStream_t>(stream), pos, lnl, lnpr, T, W, ndim, half, betas, q, zfac, lnp_new,
                       lnlike_e, E, seed, step, naccept);
    return launch_ok();
}

int lfg_pt_swap(const double* pos_in, double* pos_out, double* lnl, double* lnpr, int T, int W, int ndim,
                const double* betas, unsigned long long seed, unsigned long long step, unsigned long long* nswap,
                void* wsp, size_t ws_bytes, void* stream)
{
    if (!shape_ok(T, W, ndim) || !pos_in || !pos_out || pos_in == pos_out || !lnl || !lnpr || !betas || !nswap)
        return LFG_E_ARGS;
    if (!wsp || ws_bytes < lfg_pt_workspace_size(T, W)) return LFG_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (T == 1) {  // no pair: the state is unchanged, pos_out a copy
        return hipMemcpyAsync(pos_out, pos_in, size_t(W) * ndim * sizeof(double), hipMemcpyDeviceToDevice, st) ==
                       hipSuccess ? LFG_OK : LFG_E_LAUNCH;
    }
    int* perm = static_cast<int*>(wsp);
    int* org = perm + perm_ints(T, W);
    double* lnu = reinterpret_cast<double*>(org + size_t(T) * W);  // (3 T - 2) W ints before it, W even: 8-byte aligned
    int P = 4;
    while (P < W) P <<= 1;
    const int sort_lanes = P / 2 < 64 ? 64 : (P / 2 > PT_SORT_MAX ? PT_SORT_MAX : P / 2);
    int rc;
    hipLaunchKernelGGL(k_pt_perm, dim3(2 * (T - 1)), dim3(sort_lanes), size_t(P) * sizeof(unsigned long long), st, T, W,
                       P, seed, step, perm, lnu, org);
    if ((rc = launch_ok())) return rc;
    const int walk_lanes = W < 64 ? 64 : (W > PT_SORT_MAX ? PT_SORT_MAX : (W + 63) / 64 * 64);
    hipLaunchKernelGGL(k_pt_walk, dim3(1), dim3(walk_lanes), 0, st, lnl, lnpr, T, W, betas, perm, lnu, org, nswap);
    if ((rc = launch_ok())) return rc;
    const int n = T * W;
    hipLaunchKernelGGL(k_pt_gather, dim3((n + PT_WAVES - 1) / PT_WAVES), dim3(64 * PT_WAVES), 0, st, pos_in, pos_out,
                       org, n, ndim);
    return launch_ok();
}

}  // extern "C"
