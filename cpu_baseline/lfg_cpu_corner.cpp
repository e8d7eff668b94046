// lfg_cpu_corner.cpp -- lfg_corner_hist's and lfg_corner_levels' host twins
// (cpu_baseline/lfg_cpu.h): the rules of lfit_python_amd/csrc/lfg_corner.hpp,
// the text the gfx950 kernels compile, in their plainest form.  Per row the K
// bins, then one count per column and per pair; the levels from a sort.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")  // as the device unit: no fused multiply-add
#endif
#include <stddef.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "lfg_cpu.h"
#include "lfg_corner.hpp"

using namespace lfg;

extern "C" int lfg_cpu_corner_hist(const double* base, long long steps, long long W, int row_len, long long step_ld,
                                   long long walker_ld, const int* cols, int K, const double* range, int nb,
                                   long long* h1, long long* h2, int* flag)
{
    if (!corner_view_ok(steps, W, row_len, step_ld, walker_ld, cols, K, nb)) return LFG_E_ARGS;
    if (!range || !h1 || !flag || (K > 1) != (h2 != nullptr)) return LFG_E_ARGS;
    if (steps > 0 && W > 0 && !base) return LFG_E_ARGS;
    const int P = corner_pair_count(K);
    std::vector<CornerCol> col(K);
    for (int k = 0; k < K; ++k) {
        col[k] = corner_col(range[2 * k], range[2 * k + 1], nb);
        flag[k] = col[k].mobile ? 0 : 1;
    }
    std::fill(h1, h1 + size_t(K) * nb, 0ll);
    if (h2) std::fill(h2, h2 + size_t(P) * nb * nb, 0ll);
    std::vector<int> bin(K);
    for (long long s = 0; s < steps; ++s)
        for (long long w = 0; w < W; ++w) {
            const double* row = base + (s * step_ld + w * walker_ld);
            for (int k = 0; k < K; ++k) {
                bin[k] = col[k].mobile ? corner_bin(col[k], nb, row[cols[k]]) : -1;
                if (bin[k] >= 0) h1[size_t(k) * nb + bin[k]] += 1;
            }
            for (int a = 0; a < K; ++a)
                for (int b = a + 1; b < K && bin[a] >= 0; ++b)
                    if (bin[b] >= 0) h2[(size_t(corner_pair_index(K, a, b)) * nb + bin[a]) * nb + bin[b]] += 1;
        }
    return LFG_OK;
}

extern "C" int lfg_cpu_corner_levels(const long long* h2, int P, int nb, const double* fracs, int nl, long long* level)
{
    if (!h2 || !level || P < 0 || nb < 1 || nb > LFG_CORNER_MAX_BINS || !corner_fracs_ok(fracs, nl)) return LFG_E_ARGS;
    const size_t n = size_t(nb) * nb;
    std::vector<long long> c(n);
    for (int p = 0; p < P; ++p) {
        c.assign(h2 + size_t(p) * n, h2 + size_t(p + 1) * n);
        std::sort(c.begin(), c.end(), std::greater<long long>());
        long long total = 0;
        for (size_t i = 0; i < n; ++i) total += c[i];
        for (int l = 0; l < nl; ++l) {
            long long cum = 0, lev = c[0];
            for (size_t i = 0; i < n; ++i) {
                cum += c[i];
                if (corner_level_inside(cum, total, fracs[l])) lev = c[i];
            }
            level[size_t(p) * nl + l] = lev;
        }
    }
    return LFG_OK;
}
