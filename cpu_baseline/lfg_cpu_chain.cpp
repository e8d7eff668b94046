// lfg_cpu_chain.cpp -- lfg_chain_stats' and lfg_chain_clip's host twins
// (cpu_baseline/lfg_cpu.h): the rules of lfit_python_amd/csrc/lfg_chain.hpp,
// the text the gfx950 kernels compile, in their plainest form.  Per column:
// one sweep for the counts, the compensated sum and the extremes, a second
// for the deviations from the mean; the order statistics from a sort by key;
// R-hat from each walker's Welford moments.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")  // as the device unit: no fused multiply-add
#endif
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "lfg_cpu.h"
#include "lfg_chain.hpp"

using namespace lfg;

extern "C" int lfg_cpu_chain_stats(const double* base, long long steps, long long W, int C, long long step_ld,
                                   long long walker_ld, const double* window, const double* fracs, int nq,
                                   long long* n, long long* n_bad, double* mean, double* m2, double* vmin,
                                   double* vmax, double* ostat, double* quant, double* rhat)
{
    if (!chain_view_ok(steps, W, C, step_ld, walker_ld) || !chain_fracs_ok(fracs, nq)) return LFG_E_ARGS;
    if (!n || !n_bad || !mean || !m2 || !vmin || !vmax || (nq > 0 && (!ostat || !quant))) return LFG_E_ARGS;
    if (rhat && window) return LFG_E_ARGS;
    if (steps > 0 && W > 0 && !base) return LFG_E_ARGS;
    std::vector<uint64_t> keys;
    for (int c = 0; c < C; ++c) {
        const double lo = window ? window[2 * c] : -INFINITY, hi = window ? window[2 * c + 1] : INFINITY;
        // first sweep: counts, the compensated sum, the extremes, the keys
        ChainMom col = chain_mom_empty();
        keys.clear();
        for (long long w = 0; w < W; ++w)
            for (long long s = 0; s < steps; ++s) {
                const double x = base[s * step_ld + w * walker_ld + c];
                if (!chain_finite(x)) {
                    col.bad += 1;
                } else if (x >= lo && x <= hi) {
                    chain_mom_add(col, x);
                    keys.push_back(chain_key(x));
                }
            }
        const double mu = chain_mean(col);
        // second sweep: the deviations from that mean
        ChainDev dev = {0.0, 0.0, 0.0};
        for (long long w = 0; w < W && col.n; ++w)
            for (long long s = 0; s < steps; ++s) {
                const double x = base[s * step_ld + w * walker_ld + c];
                if (chain_used(x, lo, hi)) chain_dev_add(dev, x, mu);
            }
        n[c] = col.n;
        n_bad[c] = col.bad;
        mean[c] = mu;
        m2[c] = chain_m2(dev, col.n);
        vmin[c] = col.n ? col.lo : NAN;
        vmax[c] = col.n ? col.hi : NAN;
        if (rhat) {
            // Welford per walker; the walkers' means by Chan with unit weights
            double nw = 0.0, mw = 0.0, sw = 0.0, within = 0.0;
            for (long long w = 0; w < W; ++w) {
                double na = 0.0, ma = 0.0, sa = 0.0;
                for (long long s = 0; s < steps; ++s) chain_pair_add(na, ma, sa, base[s * step_ld + w * walker_ld + c]);
                chain_pair_merge(nw, mw, sw, 1.0, ma, 0.0);
                within += sa;
            }
            rhat[c] = col.bad ? NAN : chain_rhat(W, steps, sw, within);
        }
        std::sort(keys.begin(), keys.end());
        for (int q = 0; q < nq; ++q) {
            double a = NAN, b = NAN, v = NAN;
            if (col.n) {
                long long rl, rh;
                double g;
                chain_rank(fracs[q], col.n, rl, rh, g);
                a = chain_unkey(keys[size_t(rl)]);
                b = chain_unkey(keys[size_t(rh)]);
                v = chain_lerp(a, b, g);
            }
            ostat[(size_t(c) * nq + q) * 2] = a;
            ostat[(size_t(c) * nq + q) * 2 + 1] = b;
            quant[size_t(c) * nq + q] = v;
        }
    }
    return LFG_OK;
}

extern "C" int lfg_cpu_chain_clip(const long long* n, const double* m2, const double* med, long long med_ld,
                                  double sigma, const double* win_in, double* win_out, int C)
{
    if (!n || !m2 || !med || !win_out || C < 1 || C > LFG_CHAIN_MAX_C || med_ld < 1 || !(sigma >= 0.0))
        return LFG_E_ARGS;
    for (int c = 0; c < C; ++c) {
        double lo = win_in ? win_in[2 * c] : -INFINITY, hi = win_in ? win_in[2 * c + 1] : INFINITY;
        chain_clip(n[c], m2[c], med[size_t(c) * size_t(med_ld)], sigma, lo, hi);
        win_out[2 * c] = lo;
        win_out[2 * c + 1] = hi;
    }
    return LFG_OK;
}
