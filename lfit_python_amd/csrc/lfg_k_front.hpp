// lfg_k_front.hpp -- the __global__ definitions of k_setup, k_elements and
// k_expand; their device code is in lfg_k_setup.hpp and lfg_k_elements.hpp.
// Needs lfg_kernels.hpp before it; included by lfg.hip only, in its
// anonymous namespace.
#pragma once

__global__ __launch_bounds__(SETUP_BLOCK) void k_setup(SetupArgs A)
{
    setup_any(A, blockIdx.x * SETUP_BLOCK + threadIdx.x);
}

__global__ __launch_bounds__(ELEM_BLOCK) __attribute__((amdgpu_waves_per_eu(ELEM_MINW))) void k_elements(const double* __restrict__ geo, int* status, int npairs,
                                                         double2* __restrict__ AB, double* __restrict__ DON,
                                                         double* __restrict__ WT, const int* __restrict__ bstatus,
                                                         ElemSpec X)
{
#ifdef LFG_PROFILE_ELEM
    const unsigned long long pt0 = __builtin_amdgcn_s_memrealtime();
#endif
    if (int(blockIdx.x) < X.nspecblk) {  // speculative setup lanes of the next half
        // candidate c's lanes fill blocks [c * nb, (c + 1) * nb): c is uniform
        // in a block, so X.S[c] is selected in scalar registers (a lane-varying
        // c made the compiler keep both SetupArgs in a private array)
        const int nb = (X.nspec + int(blockDim.x) - 1) / int(blockDim.x);
        const int c = int(blockIdx.x) < nb ? 0 : 1;
        const int t = (int(blockIdx.x) - c * nb) * int(blockDim.x) + int(threadIdx.x);
        if (t < X.nspec) setup_any(X.S[__builtin_amdgcn_readfirstlane(c)], t);
#ifdef LFG_PROFILE_ELEM
        elem_stamp(pt0, 0);
#endif
        return;
    }
    const unsigned bid = blockIdx.x - unsigned(X.nspecblk);
    // blocks cover the NUNIQ unique items of every pair in chunks of
    // blockDim.x (the spot items fill the last chunk); block b takes pair
    // b % npairs, so that (with npairs a multiple of 8 and blocks dealt
    // round-robin over the XCDs) a pair's tables are written on the XCD whose
    // L2 k_lnlike block `pair` reads them from -- speed only.  Item 0 folds
    // the stream lanes' status into the pair status (MODEL_SPEC 6 order:
    // setup failures first); every item skips a pair that failed either.
    const int pair = int(bid % unsigned(npairs));
    // LFG_ELEM_IPL items per lane, one after the other (chunks of
    // ELEM_BLOCK * LFG_ELEM_IPL items)
    // chunks in dispatch order: the donor's (latency-bound 1-D roots, few
    // VALU instructions) and the spot's and outer disc's (four Newton steps)
    // first, the WD's and inner disc's (three) last, so that the second
    // round of waves ends on short ones (profiles/r03/elem_timeline_*.txt:
    // the kernel span 27.4 -> 25.2 us at config 2)
    static_assert(ELEM_BLOCK * LFG_ELEM_IPL == 64 && (NUNIQ + NDISC_R + 1 + 63) / 64 == 15, "chunk order table");
    constexpr int kOrder[15] = {13, 14, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0};
    const int ck = kOrder[bid / unsigned(npairs)];
    const int v0 = ck * (int(blockDim.x) * LFG_ELEM_IPL) + int(threadIdx.x);
    const double* G = geo + size_t(pair) * LFG_NGEO;
    int st0, bst;
    if (X.jk) {
        const int w = pair / X.E, e = pair - w * X.E;
        const size_t cp = size_t(X.accflag[X.jk[w]]) * npairs + pair;  // candidate slot of the pair
        G = X.geoC + cp * LFG_NGEO;
        st0 = X.statusC[cp];
        bst = X.bstatusC[cp];
        if (bid < unsigned(npairs)) {  // the pair's first block: the selected candidate into the standard slots
            const int l = int(threadIdx.x);
            double* Gd = const_cast<double*>(geo) + size_t(pair) * LFG_NGEO;
            if (l < LFG_NGEO) Gd[l] = G[l];
            if (l == LFG_NGEO) status[pair] = (st0 != ST_OK) ? st0 : bst;
            if (l == LFG_NGEO + 1) X.bstatus[pair] = bst;
            if (e == 0) {
                const size_t cw = size_t(X.accflag[X.jk[w]]) * (npairs / X.E) + w;
                for (int d = l; d < X.ndim; d += int(blockDim.x)) X.q[size_t(w) * X.ndim + d] = X.qC[cw * X.ndim + d];
                if (l == LFG_NGEO + 2) X.prior[w] = X.priorC[cw];
                if (l == LFG_NGEO + 3) X.zf[w] = X.zfC[cw];
            }
        }
    } else {
        st0 = status[pair];
        bst = bstatus[pair];
    }
#pragma unroll 1
    for (int k = 0; k < LFG_ELEM_IPL; ++k)
        element_lane(v0 + k * int(blockDim.x), pair, npairs, G, st0, bst, status, AB, DON, WT, X);
#ifdef LFG_PROFILE_ELEM
    elem_stamp(pt0, 1 + ck);  // 1 + chunk of the pair's items
#endif
}

// test/inspection only: per-element weights and the full 400-tile donor
__global__ void k_expand(const double* __restrict__ geo, const int* __restrict__ status, int npairs,
                         const double2* __restrict__ AB, const double* __restrict__ DON, double* __restrict__ A,
                         double* __restrict__ B, double* __restrict__ WG, double* __restrict__ DFULL)
{
    const long t = long(blockIdx.x) * blockDim.x + threadIdx.x;
    const int pair = int(t / NEL), k = int(t - long(pair) * NEL);
    if (pair >= npairs || status[pair] != ST_OK) return;
    const double* G = geo + size_t(pair) * LFG_NGEO;
    const double2 ab = elem_ab(AB + size_t(pair) * NELU, k);
    if (A) A[size_t(pair) * NEL + k] = ab.x;
    if (B) B[size_t(pair) * NEL + k] = ab.y;
    double w;
    if (k < NWD) {
        int ir = int(sqrt(k * 0.25));
        if (4 * (ir + 1) * (ir + 1) <= k) ++ir;
        if (4 * ir * ir > k) --ir;
        w = wd_ring_weight(ir, G[G_ULIMB]);
    } else if (k < NWD + NDISC) {
        w = disc_ring_weight((k - NWD) / NDISC_AZ, G);
    } else {
        w = bs_weight(k - NWD - NDISC, G);
    }
    if (WG) WG[size_t(pair) * NEL + k] = w;
    if (DFULL && k < U_DON) {
        const int it = k / (NDONOR_P / 4), ip = k - it * (NDONOR_P / 4);
        const double* v = DON + (size_t(pair) * U_DON + k) * DON_STRIDE;
        const int base = it * NDONOR_P;
        const int ks[4] = {base + ip, base + NDONOR_P - 1 - ip, base + NDONOR_P / 2 - 1 - ip,
                           base + NDONOR_P / 2 + ip};
        const double sy[4] = {1.0, 1.0, -1.0, -1.0}, sz[4] = {1.0, -1.0, 1.0, -1.0};
        double* D = DFULL + size_t(pair) * NDONOR * 3;
        for (int m = 0; m < 4; ++m) {
            D[3 * ks[m]] = v[0];
            D[3 * ks[m] + 1] = sy[m] * v[1];
            D[3 * ks[m] + 2] = sz[m] * v[2];
        }
    }
}
