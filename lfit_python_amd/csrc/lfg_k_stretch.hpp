// lfg_k_stretch.hpp -- the stretch-move sampler's kernels: k_propose,
// k_accept, k_accept_regen, k_apply_verdicts, k_verdict.  Needs
// lfg_philox.hpp before it; included by lfg.hip only, in its anonymous
// namespace.
#pragma once

// ------------------------------------------------------- stretch-move sampler
// emcee StretchMove.get_proposal: z = ((a-1) u + 1)^2 / a,
// q = c_j - (c_j - s) z = c_j + z (s - c_j), factor = (ndim - 1) ln z
// step counter: by value, or (stepp != nullptr) from device memory so that
// a captured HIP graph replays with the current step
__global__ void k_propose(const double* __restrict__ pos, int W, int ndim, int half, double a,
                          unsigned long long seed, unsigned long long step,
                          const unsigned long long* __restrict__ stepp, double* __restrict__ q,
                          double* __restrict__ zfac)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ns = W / 2;
    if (i >= ns) return;
    if (stepp) step = *stepp;
    const uint4 r = draw(seed, step, half, 0, i);
    const double u = u53(r.x, r.y);
    const double zr = (a - 1.0) * u + 1.0;
    const double z = zr * zr / a;
    const int j = int(__umulhi(r.z, unsigned(ns)));  // partner in the other half
    const double* s = pos + size_t(half * ns + i) * ndim;
    const double* cj = pos + size_t((1 - half) * ns + j) * ndim;
    double* out = q + size_t(i) * ndim;
    for (int d = 0; d < ndim; ++d) out[d] = fma(s[d] - cj[d], z, cj[d]);  // c_j + z (s - c_j), as make_prop
    zfac[i] = (ndim - 1.0) * log(z);
}

// Metropolis acceptance: accept if ln u < factor + lnp_new - lnp_old
__global__ void k_accept(double* __restrict__ pos, double* __restrict__ lnp, int W, int ndim, int half,
                         const double* __restrict__ q, const double* __restrict__ zfac,
                         const double* __restrict__ lnp_new, unsigned long long seed, unsigned long long step,
                         const unsigned long long* __restrict__ stepp, int* __restrict__ naccept)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ns = W / 2;
    if (i >= ns) return;
    if (stepp) step = *stepp;
    const int w = half * ns + i;
    const uint4 r = draw(seed, step, half, 1, i);
    const double lu = log(u53(r.x, r.y));
    const double diff = zfac[i] + lnp_new[i] - lnp[w];
    if (lu < diff) {
        double* p = pos + size_t(w) * ndim;
        const double* qi = q + size_t(i) * ndim;
        for (int d = 0; d < ndim; ++d) p[d] = qi[d];
        lnp[w] = lnp_new[i];
        if (naccept) naccept[w] += 1;
    }
}

// k_accept with the proposal re-formed from the same draws (k_propose's
// arithmetic): the sharded half-step keeps only its own shard of q, and the
// partner half is unchanged until this half is accepted
// one wave per walker of the half (four per 256-lane block): the draws and
// the decision are wave-uniform (scalar ALU and scalar loads), and an
// accepted walker's row moves with one load round over the lanes (lane d:
// dimension d) instead of one lane's serial chunks of 8
constexpr int REGEN_WAVES = 4;
__global__ __launch_bounds__(64 * REGEN_WAVES) void k_accept_regen(double* __restrict__ pos, double* __restrict__ lnp, int W, int ndim, int half,
                               double a, const double* __restrict__ lnp_new, unsigned long long seed,
                               unsigned long long step, int* __restrict__ naccept, int* __restrict__ accflag)
{
    const int i = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * REGEN_WAVES + int(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int ns = W / 2;
    if (i >= ns) return;
    const int w = half * ns + i;
    const uint4 r0 = draw(seed, step, half, 0, i);
    const double zr = (a - 1.0) * u53(r0.x, r0.y) + 1.0;
    const double z = zr * zr / a;
    const uint4 r = draw(seed, step, half, 1, i);
    const double lu = log(u53(r.x, r.y));
    const double diff = (ndim - 1.0) * log(z) + lnp_new[i] - lnp[w];
    const bool acc = lu < diff;
    if (acc) {
        const int j = int(__umulhi(r0.z, unsigned(ns)));
        double* p = pos + size_t(w) * ndim;
        const double* cj = pos + size_t((1 - half) * ns + j) * ndim;
        for (int d = lane; d < ndim; d += 64) p[d] = fma(p[d] - cj[d], z, cj[d]);
        if (lane == 0) {
            lnp[w] = lnp_new[i];
            if (naccept) naccept[w] += 1;
        }
    }
    if (accflag && lane == 0) accflag[i] = acc ? 1 : 0;  // the speculative setup's candidate choice
}

// the deferred acceptance's two halves outside k_pair<_, true>:
//  k_apply_verdicts: half `half`'s gathered verdicts (ln_prob where the move
//  was accepted, NaN where not) applied to the ensemble, the proposal
//  re-formed from its draws as k_accept_regen does (the flush at a chain's
//  end, and the fold's fallback); one wave per walker
//  k_verdict: a shard's verdicts from its ln_prob (k_accept_regen's test)
__global__ __launch_bounds__(64 * REGEN_WAVES) void k_apply_verdicts(double* __restrict__ pos, double* __restrict__ lnp,
                                                                      int W, int ndim, int half, double a,
                                                                      const double* __restrict__ verdict,
                                                                      unsigned long long seed, unsigned long long step,
                                                                      int* __restrict__ naccept, int* __restrict__ accflag)
{
    const int i = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * REGEN_WAVES + int(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int ns = W / 2;
    if (i >= ns) return;
    const double v = verdict[i];
    const bool acc = !isnan(v);
    if (acc) {
        const int w = half * ns + i;
        const uint4 r0 = draw(seed, step, half, 0, i);
        const double zr = (a - 1.0) * u53(r0.x, r0.y) + 1.0;
        const double z = zr * zr / a;
        const int j = int(__umulhi(r0.z, unsigned(ns)));
        double* p = pos + size_t(w) * ndim;
        const double* cj = pos + size_t((1 - half) * ns + j) * ndim;
        for (int d = lane; d < ndim; d += 64) p[d] = fma(p[d] - cj[d], z, cj[d]);
        if (lane == 0) {
            lnp[w] = v;
            if (naccept) naccept[w] += 1;
        }
    }
    if (accflag && lane == 0) accflag[i] = acc ? 1 : 0;
}

__global__ void k_verdict(const double* __restrict__ lnp_new, const double* __restrict__ lnp,
                          const double* __restrict__ zfac, int n, int lo, int ns, int half, unsigned long long seed,
                          unsigned long long step, double* __restrict__ vout)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint4 r = draw(seed, step, half, 1, lo + k);
    const double v = lnp_new[k];
    vout[k] = (log(u53(r.x, r.y)) < zfac[k] + v - lnp[size_t(half) * ns + lo + k]) ? v : NAN;
}
