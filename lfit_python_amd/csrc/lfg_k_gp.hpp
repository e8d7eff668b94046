// lfg_k_gp.hpp -- the GP tree kernels k_gp_dcp and k_gp_like, and the two
// combines k_combine_walkers and k_combine.  Needs before it: lfg_device.hpp
// (findphi_fast, element_interval, eggleton), lfg_philox.hpp (draw, u53),
// lfg_k_elements.hpp (prior_rejects), lfg_k_lnlike.hpp (LikeArgs,
// combine_walker, combine_after) and lfg_k_pair.hpp (DCP_LANES, DCP_NTHETA).
// Included by lfg.hip only, in its anonymous namespace.
#pragma once

// -------------------------------------------------------------- k_gp_dcp
// GP trees: the changepoint distance of pairs whose walker tripped the
// cache rule (k_setup marked them G_GP_OK = 2): dist_cp = (dphi + phi4 -
// phi3) / 2 with phi3 / phi4 = wdphases(q, i, rwd, 10) (CVModel.py:561-570,
// MODEL_SPEC 10.2-10.3).  16 lanes per pair, lane k < 10 solves limb point k
// (the nested eclipse solver), min / max by shuffles; other pairs return at
// once.  Runs after k_elements (the pair's record is in the standard slot)
// and before k_lnlike<2>, which reads G_GP_DCP.
__global__ __launch_bounds__(64) void k_gp_dcp(double* __restrict__ geo, const int* __restrict__ status, int npairs)
{
    const int pair = int(blockIdx.x) * (64 / DCP_LANES) + int(threadIdx.x) / DCP_LANES;
    const int k = int(threadIdx.x) % DCP_LANES;
    if (pair >= npairs) return;
    double* G = geo + size_t(pair) * LFG_NGEO;
    if (G[G_GP_OK] != 2.0) return;  // uniform over the pair's 16 lanes
    bool ok = status[pair] == ST_OK && G[G_GP_RWD] > 0.0;
    double b = NAN;
    if (ok && k < DCP_NTHETA) {
        const Roche R{G[G_Q], G[G_CA], G[G_CB], G[G_MU], G[G_XL1], G[G_PL1], G[G_RS], G[G_RS2]};
        const double s = G[G_S], c = G[G_C], r1 = G[G_GP_RWD];
        double dphi_c;
        if (findphi_fast(R, G[G_INC], dphi_c) == ST_OK) {  // as wdphases: the egress phase of the WD centre
            double sth, cth, sp, cp, a;
            sincos(PI * dphi_c, &sth, &cth);
            sincos(TWO_PI * k / DCP_NTHETA, &sp, &cp);
            if (!element_interval(R, r1 * (cp * sth - sp * c * cth), r1 * (cp * cth + sp * c * sth), r1 * (sp * s), s,
                                  c, eggleton(R.q), a, b))
                b = NAN;
        }
    }
    double lo = isnan(b) ? INFINITY : b, hi = isnan(b) ? -INFINITY : b;
    for (int off = DCP_LANES / 2; off > 0; off >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, off, DCP_LANES));
        hi = fmax(hi, __shfl_xor(hi, off, DCP_LANES));
    }
    if (k == 0) {
        ok = ok && lo <= hi;  // no eclipsed limb point: wdphases fails
        G[G_GP_DCP] = ok ? (G[G_GP_DPHI] + (hi - lo)) / 2.0 : NAN;
        G[G_GP_OK] = ok ? 1.0 : 0.0;
    }
}

// -------------------------------------------------------------- k_gp_like
// GP trees (MODEL_SPEC 10.4): the Kalman filter over each pair's residuals
// (k_lnlike<2> wrote them), parallel in time.  The recursion is serial in
// the points and its dependent chain (D -> S -> 1/S -> D, ~14 FP64 ops of
// 32-48 cycles each for a lone wave, tools/lat_probe.hip) set the time when
// one lane or one quad ran a pair's 300 points.  So a pair's points are cut
// into GP_SEG segments, each filtered by a quad of lanes at once:
//  * element pass (per segment s, its quad): the filter conditioned on the
//    unknown prior state x_s at the segment's first point -- the mean is
//    A x_s + c, the covariance starts at 0, and the segment's data give
//    exp(-1/2 x_s^T J x_s + eta^T x_s - kappa / 2).  Lane r owns row r of
//    D (= P - P_inf), column r of A, c_r, row r of J and eta_r; rows and
//    gains travel by DPP quad permutes.
//  * combine (one lane per pair, serial over the segments, 4x4 algebra):
//    integrate x_s against its prior N(mu, Sigma), add the segment's ln_like,
//    carry the filtered end state (A mu_post + c, A Sigma_post A^T + P_end)
//    through the gap's transition (and a block start) to the next segment.
// tests/gp_kalman.py:gp_lnlike_segments restates it; equal to the dense
// likelihood to ~1e-15.
//
// Coordinates: Jordan form of each 2-state block.  With K = [[lam, 1],
// [-lam^2, -lam]] (K^2 = 0), Phi(d) = e^{-u} (I + d K); z = (x0, lam x0 + x1)
// turns it into e^{-u} T, T = [[1, d], [0, 1]].  The observation is still z0
// and P_inf = a [[1, lam], [lam, 2 lam^2]] per block.
//
// Then ln_like = sum of the segments' and, as k_lnlike does, ln_prob and the
// acceptance of the walker once its last eclipse is in.  Pairs of a wave
// take one eclipse of consecutive walkers (equal point counts, shared x / ye).
constexpr int GP_BLOCK = 64;
#ifndef LFG_GP_CHUNK
#define LFG_GP_CHUNK 8
#endif
constexpr int GP_CHUNK = LFG_GP_CHUNK;
constexpr int GP_SEG = 8;                     // segments per pair
constexpr int GP_LPP = 4 * GP_SEG;            // lanes per pair: a quad per segment
constexpr int GP_PAIRS = GP_BLOCK / GP_LPP;   // pairs per wave
constexpr int GP_EL = 16;                     // doubles of a lane's element row in LDS

// v of lane (quad base + PERM's selector for this lane): DPP quad_perm on both halves
template <int PERM>
__device__ __forceinline__ double quad_perm(double v)
{
    // every lane of a quad is a valid source: no "old" value (update_dpp's
    // copy of it cost a v_mov per permute)
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp(static_cast<int>(b), PERM, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp(static_cast<int>(b >> 32), PERM, 0xf, 0xf, false);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}
constexpr int QP_NEXT = 0xF5;  // [1, 1, 3, 3]: the odd row of each block
constexpr int QP_B0 = 0x00, QP_B1 = 0x55, QP_B2 = 0xAA, QP_B3 = 0xFF;  // broadcast lane 0 / 1 / 2 / 3

// P_inf (z coordinates) entry (i, j) of a pair: blocks ain, aout
__device__ __forceinline__ double gp_pinf(int i, int j, double ain, double aout, double lam)
{
    if ((i >> 1) != (j >> 1)) return 0.0;
    const double a = (i >> 1) ? aout : ain;
    const int k = (i & 1) + (j & 1);
    return k == 0 ? a : (k == 1 ? a * lam : 2.0 * a * lam * lam);
}

__global__ __launch_bounds__(GP_BLOCK) __attribute__((amdgpu_waves_per_eu(2))) void k_gp_like(LikeArgs L)
{
    __shared__ double sel[GP_PAIRS][GP_SEG][4][GP_EL];
    __shared__ double sgap[GP_PAIRS][GP_SEG][4];  // the gap into each segment (the combine's transition)
    const int nw = L.npairs / L.E, nwb = (nw + GP_PAIRS - 1) / GP_PAIRS;
    const int e = int(blockIdx.x) / nwb;
    const int lane = int(threadIdx.x), pp = lane / GP_LPP, sg = (lane / 4) % GP_SEG, r = lane & 3;
    const int w = (int(blockIdx.x) - e * nwb) * GP_PAIRS + pp;
    const bool live = w < nw;
    const int pair = live ? w * L.E + e : 0;
    const int o0 = L.off ? L.off[e] : 0;
    const int n = L.off ? L.off[e + 1] - o0 : L.N;
    const double* G = L.geo + size_t(pair) * LFG_NGEO;
    const bool run = live && L.status[pair] == ST_OK && G[G_GP_OK] != 0.0 &&
                     !(L.prior && prior_rejects(L.prior[pair / L.E], G));
    const double ain = G[G_GP_AIN], aout = G[G_GP_AOUT], lam = G[G_GP_LAM];
    const double* res = L.res + size_t(pair) * L.N;
    const double* gx = L.gpx + size_t(pair) * L.N;
    const int* gb = L.gpb + size_t(pair) * L.N;
    const double* xs = L.x + o0;
    const double* yes = L.ye + o0;
    if (run) {
        // ---- element pass: segment sg of the pair, lane r of its quad
        const int i0 = (n * sg) / GP_SEG, i1 = (n * (sg + 1)) / GP_SEG;
        const double pc0 = gp_pinf(r, 0, ain, aout, lam), pc2 = gp_pinf(r, 2, ain, aout, lam);
        const bool even = (r & 1) == 0, hrow = r >= 2;
        // P starts at 0: D = -P_inf; A = I; c = 0
        double D0 = -gp_pinf(r, 0, ain, aout, lam), D1 = -gp_pinf(r, 1, ain, aout, lam);
        double D2 = -gp_pinf(r, 2, ain, aout, lam), D3 = -gp_pinf(r, 3, ain, aout, lam);
        double A0 = r == 0 ? 1.0 : 0.0, A1 = r == 1 ? 1.0 : 0.0, A2 = r == 2 ? 1.0 : 0.0, A3 = r == 3 ? 1.0 : 0.0;
        double c = 0.0, J0 = 0.0, J1 = 0.0, J2 = 0.0, J3 = 0.0, eta = 0.0;
        double q2 = 0.0, lnS = 0.0, xprev = (i0 > 0 && i0 < n) ? xs[i0 - 1] : 0.0;
        int bp = (i0 > 0 && i0 < n) ? gb[i0 - 1] : -1;
        bool bad = false;
        double cx[GP_CHUNK], cy[GP_CHUNK], cr[GP_CHUNK], ce[GP_CHUNK];
        int cb[GP_CHUNK];
        auto fetch = [&](int p0) {
#pragma unroll
            for (int k = 0; k < GP_CHUNK; ++k) {
                const int q = min(p0 + k, i1 - 1);
                cx[k] = xs[q];
                cy[k] = yes[q];
                cr[k] = res[q];
                ce[k] = gx[q];
                cb[k] = gb[q];
            }
        };
        if (i1 > i0) fetch(i0);
        if (i1 > i0) {  // the gap into this segment (the combine's transition): lane r of the quad
            // writes entry r (d, e^{-lam d}, block start), read back in the combine
            // instead of a dependent global load per segment (k_gp_like 42.0 -> 40.4 us,
            // profiles/r06/ab_gp_combine.txt)
            const bool fr = cb[0] >= 0 && cb[0] != bp;
            sgap[pp][sg][r] = r == 0 ? cx[0] - xprev : (r == 1 ? ce[0] : (fr ? 1.0 : 0.0));
        }
        for (int p0 = i0; p0 < i1; p0 += GP_CHUNK) {
            double dk[GP_CHUNK], ek[GP_CHUNK], Ek[GP_CHUNK], ye2[GP_CHUNK], rv[GP_CHUNK];
            int blk[GP_CHUNK];
#pragma unroll
            for (int k = 0; k < GP_CHUNK; ++k) {
                const double dd = cx[k] - (k ? cx[k - 1] : xprev);
                dk[k] = dd;
                ek[k] = ce[k];  // e^{-lam dd}, formed in k_lnlike<2>
                Ek[k] = ce[k] * ce[k];
                ye2[k] = cy[k] * cy[k];
                rv[k] = cr[k];
                blk[k] = cb[k];
                bad = bad || (p0 + k < i1 && p0 + k > 0 && !(dd >= 0.0)) || (p0 + k < i1 && !isfinite(cr[k]));
            }
            xprev = cx[GP_CHUNK - 1];
            if (p0 + GP_CHUNK < i1) fetch(p0 + GP_CHUNK);  // in flight during the recursion
            double prodS = 1.0;  // one log per chunk (S ~ ye^2: eight factors stay far from underflow)
#pragma unroll
            for (int k = 0; k < GP_CHUNK; ++k) {
                if (p0 + k >= i1) break;
                // a new block: its process starts stationary and independent
                // of x_s: rows / columns 2, 3 of D and rows 2, 3 of A and c
                // restart at 0 (zero scales in the prediction; the block
                // start at the segment's first point is the combine's)
                const bool fresh = blk[k] >= 0 && blk[k] != bp;
                bp = blk[k];
                if (p0 + k > i0) {  // predict: D <- e^{-2u} T D T^T, A <- e^{-u} T A, c <- e^{-u} T c
                    const double d = dk[k], dr = even ? d : 0.0, ex = ek[k];
                    const double kr = (fresh && hrow) ? 0.0 : 1.0, kc = fresh ? 0.0 : 1.0;
                    const double n0 = quad_perm<QP_NEXT>(D0), n1 = quad_perm<QP_NEXT>(D1);
                    const double n2 = quad_perm<QP_NEXT>(D2), n3 = quad_perm<QP_NEXT>(D3);
                    const double nc = quad_perm<QP_NEXT>(c);
                    const double t0 = fma(dr, n0, D0), t1 = fma(dr, n1, D1);
                    const double t2 = fma(dr, n2, D2), t3 = fma(dr, n3, D3);
                    const double Eg = Ek[k] * kr, Eh = Eg * kc;
                    D0 = Eg * fma(d, t1, t0);
                    D1 = Eg * t1;
                    D2 = Eh * fma(d, t3, t2);
                    D3 = Eh * t3;
                    const double exh = ex * kc;
                    A0 = ex * fma(d, A1, A0);
                    A1 = ex * A1;
                    A2 = exh * fma(d, A3, A2);
                    A3 = exh * A3;
                    c = (ex * kr) * fma(dr, nc, c);
                }
                const double a = (blk[k] >= 0) ? 1.0 : 0.0;
                // k = P h, h = (1, 0, a, 0), P = D + P_inf: this row's gain
                const double kk = (D0 + pc0) + a * (D2 + pc2);
                const double k0 = quad_perm<QP_B0>(kk), k1 = quad_perm<QP_B1>(kk);
                const double k2 = quad_perm<QP_B2>(kk), k3 = quad_perm<QP_B3>(kk);
                const double c0 = quad_perm<QP_B0>(c), c2 = quad_perm<QP_B2>(c);
                const double hA = fma(a, A2, A0);  // (h^T A)_r
                const double h0 = quad_perm<QP_B0>(hA), h1 = quad_perm<QP_B1>(hA);
                const double h2 = quad_perm<QP_B2>(hA), h3 = quad_perm<QP_B3>(hA);
                const double S = fma(a, k2, k0) + ye2[k];
                const double vt = rv[k] - fma(a, c2, c0);
                const double iS = rcp_fast(S);  // v_rcp_f64 (2.5e-8) + one Newton step: ~1 ulp
                bad = bad || !(S > 0.0) || !isfinite(vt);
                q2 = fma(vt * vt, iS, q2);
                prodS *= S;
                const double g = hA * iS;
                J0 = fma(g, h0, J0);
                J1 = fma(g, h1, J1);
                J2 = fma(g, h2, J2);
                J3 = fma(g, h3, J3);
                eta = fma(g, vt, eta);
                c = fma(kk, vt * iS, c);
                A0 = fma(-k0, g, A0);
                A1 = fma(-k1, g, A1);
                A2 = fma(-k2, g, A2);
                A3 = fma(-k3, g, A3);
                const double j = kk * iS;
                D0 = fma(-j, k0, D0);
                D1 = fma(-j, k1, D1);
                D2 = fma(-j, k2, D2);
                D3 = fma(-j, k3, D3);
            }
            lnS += log(prodS);
        }
        double* o = sel[pp][sg][r];
        o[0] = D0; o[1] = D1; o[2] = D2; o[3] = D3;
        o[4] = A0; o[5] = A1; o[6] = A2; o[7] = A3;
        o[8] = c;
        o[9] = J0; o[10] = J1; o[11] = J2; o[12] = J3;
        o[13] = eta;
        o[14] = q2 + lnS;
        o[15] = bad ? 1.0 : 0.0;
    }
    __syncthreads();
    // ---- combine: serial over the segments, the 4x4 algebra spread over 16
    // lanes of the pair (lane (ci, cj) holds entry (ci, cj) of Sigma and of
    // each product; rows / columns are exchanged through LDS; vectors are
    // formed in every lane).  Every lane of the wave runs it (barriers):
    // lanes 16..31 of a pair repeat 0..15 without writing, and pairs that
    // are not evaluated compute on unset data and are discarded.
    __shared__ double smat[GP_PAIRS][5][16];
    double* const SGb = smat[pp][0];  // Sigma
    double* const CBb = smat[pp][1];  // C = I + J Sigma
    double* const CIb = smat[pp][2];  // C^-1
    double* const SPb = smat[pp][3];  // Sigma_post
    double* const ASb = smat[pp][4];  // A Sigma_post
    const int q16 = lane % GP_LPP, e16 = q16 & 15, ci = e16 >> 2, cj = e16 & 3;
    const bool wr = q16 < 16;
    const double pij = gp_pinf(ci, cj, ain, aout, lam);
    double sgm = pij;  // Sigma_{ci cj}: the stationary prior of the first point
    double mu[4] = {0.0, 0.0, 0.0, 0.0};
    double ll = 0.0;
    bool bad = false;
    for (int s = 0; s < GP_SEG; ++s) {
        const int i0 = (n * s) / GP_SEG, i1 = (n * (s + 1)) / GP_SEG;
        if (i1 <= i0) continue;  // an empty segment: nothing observed, no transition (n is the wave's)
        const double* El = &sel[pp][s][0][0];
        bad = bad || El[15] != 0.0 || El[GP_EL + 15] != 0.0;
        if (s > 0 && i0 > 0) {  // the gap from the previous segment's last point
            const double d = sgap[pp][s][0], ex = sgap[pp][s][1], E = ex * ex;
            const bool fresh = sgap[pp][s][2] != 0.0;
            mu[0] = ex * fma(d, mu[1], mu[0]);
            mu[1] = ex * mu[1];
            mu[2] = fresh ? 0.0 : ex * fma(d, mu[3], mu[2]);
            mu[3] = fresh ? 0.0 : ex * mu[3];
            // Sigma <- E T (Sigma - P_inf) T^T + P_inf, T = [[1, d], [0, 1]] per block
            if (wr) SGb[e16] = sgm - pij;
            __syncthreads();
            const bool ei = (ci & 1) == 0, ej = (cj & 1) == 0;
            const double t0 = SGb[e16] + (ei ? d * SGb[e16 + 4] : 0.0);
            const double t1 = ej ? SGb[e16 + 1] + (ei ? d * SGb[e16 + 5] : 0.0) : 0.0;
            const double sgx = fma(E, ej ? fma(d, t1, t0) : t0, pij);
            sgm = (fresh && (ci >= 2 || cj >= 2)) ? pij : sgx;
            __syncthreads();
        }
        // C = I + J Sigma
        if (wr) SGb[e16] = sgm;
        __syncthreads();
        {
            double v = (ci == cj) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v = fma(El[ci * GP_EL + 9 + k], SGb[k * 4 + cj], v);
            if (wr) CBb[e16] = v;
        }
        __syncthreads();
        // det C by 2x2 minors (every lane), C^-1_{ci cj} = cof_{cj ci} / det
        // with the cofactor a 3x3 determinant of C less row cj, column ci
        double det;
        {
            const double* m = CBb;
            const double s0 = fma(m[0], m[5], -m[4] * m[1]), s1 = fma(m[0], m[6], -m[4] * m[2]);
            const double s2 = fma(m[0], m[7], -m[4] * m[3]), s3 = fma(m[1], m[6], -m[5] * m[2]);
            const double s4 = fma(m[1], m[7], -m[5] * m[3]), s5 = fma(m[2], m[7], -m[6] * m[3]);
            const double c5 = fma(m[10], m[15], -m[14] * m[11]), c4 = fma(m[9], m[15], -m[13] * m[11]);
            const double c3 = fma(m[9], m[14], -m[13] * m[10]), c2 = fma(m[8], m[15], -m[12] * m[11]);
            const double c1 = fma(m[8], m[14], -m[12] * m[10]), c0 = fma(m[8], m[13], -m[12] * m[9]);
            det = (fma(s0, c5, -s1 * c4) + fma(s2, c3, s3 * c2)) + fma(s5, c0, -s4 * c1);
            const int r0 = cj == 0 ? 1 : 0, r1 = cj <= 1 ? 2 : 1, r2 = cj <= 2 ? 3 : 2;
            const int k0 = ci == 0 ? 1 : 0, k1 = ci <= 1 ? 2 : 1, k2 = ci <= 2 ? 3 : 2;
            const double a00 = m[r0 * 4 + k0], a01 = m[r0 * 4 + k1], a02 = m[r0 * 4 + k2];
            const double a10 = m[r1 * 4 + k0], a11 = m[r1 * 4 + k1], a12 = m[r1 * 4 + k2];
            const double a20 = m[r2 * 4 + k0], a21 = m[r2 * 4 + k1], a22 = m[r2 * 4 + k2];
            const double d3 = a00 * fma(a11, a22, -a12 * a21) - a01 * fma(a10, a22, -a12 * a20) +
                              a02 * fma(a10, a21, -a11 * a20);
            const double cof = ((ci + cj) & 1) ? -d3 : d3;
            if (wr) CIb[e16] = cof / det;
        }
        bad = bad || !(det > 0.0);
        __syncthreads();
        // Sigma_post = Sigma C^-1
        {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v = fma(SGb[ci * 4 + k], CIb[k * 4 + cj], v);
            if (wr) SPb[e16] = v;
        }
        __syncthreads();
        // vectors (every lane): u = eta - J mu, Sigma_post u, the segment's ln_like
        double u[4], emu = 0.0, mJm = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double jm = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) jm = fma(El[i * GP_EL + 9 + k], mu[k], jm);
            const double et = El[i * GP_EL + 13];
            u[i] = et - jm;
            emu = fma(et, mu[i], emu);
            mJm = fma(mu[i], jm, mJm);
        }
        double uSu = 0.0, mp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double su = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) su = fma(SPb[i * 4 + k], u[k], su);
            uSu = fma(u[i], su, uSu);
            mp[i] = mu[i] + su;
        }
        ll += (emu - 0.5 * log(det)) + 0.5 * (uSu - mJm - El[14]);
        // the filtered end state: A mp + c (every lane), A Sigma_post A^T + P_end
        // (lane j of the element's quad wrote column j of A: A_ik = El[k][4 + i])
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double v = El[i * GP_EL + 8];
#pragma unroll
            for (int k = 0; k < 4; ++k) v = fma(El[k * GP_EL + 4 + i], mp[k], v);
            mu[i] = v;
        }
        {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v = fma(El[k * GP_EL + 4 + ci], SPb[k * 4 + cj], v);
            if (wr) ASb[e16] = v;
        }
        __syncthreads();
        {
            double v = El[ci * GP_EL + cj] + pij;  // P_end = D_end + P_inf
#pragma unroll
            for (int k = 0; k < 4; ++k) v = fma(ASb[ci * 4 + k], El[k * GP_EL + 4 + cj], v);
            sgm = v;
        }
        __syncthreads();
    }
    if (!live || q16 != 0) return;
    double lle = -INFINITY;
    if (run) {
        const double v = ll - 0.5 * n * 1.8378770664093454836;  // log(2 pi)
        lle = (bad || !isfinite(v)) ? -INFINITY : v;
    }
    L.lle[pair] = lle;
    combine_after(L, pair);
}

// -------------------------------------------------------------- k_combine
// E > 1: ln_prob (and the fused acceptance) of every walker once all its
// eclipses' ln_like are written, one lane per walker, in a launch of its own.
// (The last-finishing block of each walker used to do it after a device-scope
// fence: on MI355X that fence writes back the block's whole L2, and the 12 288
// fences of a config-3 launch cost a third of k_lnlike: 898 -> 587 us.)
// One wave per walker: the lanes fetch the E Roche priors and ln_like at
// once (the walker's chain of 2E dependent-latency loads in one lane was 43 us
// per config-3 launch), lane 0 adds them in combine_walker's order (the
// same sums, bit for bit), and the lanes copy an accepted proposal.
__global__ __launch_bounds__(256) void k_combine_walkers(LikeArgs L)
{
    const int w = int(blockIdx.x) * 4 + int(threadIdx.x >> 6), lane = int(threadIdx.x & 63);
    if (w >= L.npairs / L.E) return;
    const size_t p0 = size_t(w) * L.E;
    double lp = L.prior[w];
    double ll = 0.0;
    for (int e0 = 0; e0 < L.E; e0 += 64) {
        const int e = e0 + lane;
        double g = 0.0, l = 0.0;
        if (e < L.E) {
            const double* G = L.geo + (p0 + e) * LFG_NGEO;
            g = G[G_RPRIOR] + G[G_RPRIOR_BS];
            l = L.lle[p0 + e];
        }
        const int m = min(64, L.E - e0);
        for (int k = 0; k < m; ++k) {  // in eclipse order, as combine_walker
            lp += __shfl(g, k, 64);
            ll += __shfl(l, k, 64);
        }
    }
    double v;
    if (!isfinite(lp)) {
        for (int e = lane; e < L.E; e += 64) L.lle[p0 + e] = -INFINITY;
        v = -INFINITY;
    } else {
        v = lp + ll;
    }
    if (L.lnp && lane == 0) L.lnp[w] = v;
    if (!L.pos) return;
    const int wg = L.half * L.npairs / L.E + w;  // ensemble index (npairs / E = batch walkers)
    bool acc = false;
    if (lane == 0) {
        const uint4 r = draw(L.seed, L.step, L.half, 1, w);
        acc = log(u53(r.x, r.y)) < L.zfac[w] + v - L.lnp_ens[wg];
        if (acc) {
            L.lnp_ens[wg] = v;
            if (L.naccept) L.naccept[wg] += 1;
        }
        if (L.accflag) L.accflag[w] = acc ? 1 : 0;
    }
    if (__shfl(acc ? 1 : 0, 0, 64))
        for (int d = lane; d < L.ndim; d += 64) L.pos[size_t(wg) * L.ndim + d] = L.qprop[size_t(w) * L.ndim + d];
}

__global__ void k_combine(int W, int E, const double* __restrict__ prior, const double* __restrict__ geo,
                          double* __restrict__ lle, double* __restrict__ lnp)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    double lp = prior[w];
    for (int e = 0; e < E; ++e) {
        const double* G = geo + (size_t(w) * E + e) * LFG_NGEO;
        lp += G[G_RPRIOR] + G[G_RPRIOR_BS];
    }
    if (!lle) {  // ln_prior only (lfg_lnprior)
        lnp[w] = isfinite(lp) ? lp : -INFINITY;
        return;
    }
    if (!isfinite(lp)) {
        for (int e = 0; e < E; ++e) lle[size_t(w) * E + e] = -INFINITY;
        lnp[w] = -INFINITY;
        return;
    }
    double ll = 0.0;
    for (int e = 0; e < E; ++e) ll += lle[size_t(w) * E + e];
    lnp[w] = lp + ll;
}
