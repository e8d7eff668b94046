// Host program of tests/test_sweep_entries.py: the entries of the sweep's
// difference arrays (lfit_python_amd/csrc/lfg_sweep.hpp, through
// cpu_baseline/shim).  For each window set and each m it fills one array with
// apply_runs (the reference), one with apply_runs_merged voting with the
// lane's own predicate (the merged path wherever it applies) and one with
// apply_runs_merged forced onto apply_runs_batched, and compares them integer
// for integer on [0, m); the slots from m on hold a canary that must survive.
// It also pins kRingOf (lfg_tables.hpp) against the two functions it replaced.
// Prints one line per window set: name, intervals, merged-path count, batched-
// path count.  Exit status 1 on the first difference.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "lfg_sweep.hpp"
#include "lfg_tables.hpp"

using namespace lfg;

namespace {

constexpr unsigned long long CANARY = 0xC0FFEE0DDF00Dull;
constexpr int PAD = 4;

struct Add {
    unsigned long long* acc;
    void operator()(int p, long long q) const { acc[p] += static_cast<unsigned long long>(q); }
};

struct Windows {
    std::vector<double> lo, hi, iw;
    std::vector<int> cell;
};

// cell[g] = #{p : ci(v_p) < g}, ci as cell_of clamps it (lfg_k_lnlike.hpp: build_cells)
void build_cells(Windows& W, int m)
{
    W.cell.assign(LIKE_NC + 1, 0);
    const PhaseIndex X = phase_index(W.lo.data(), W.cell.data(), m);
    for (int g = 0; g <= LIKE_NC; ++g) {
        int n = 0;
        for (int p = 0; p < m; ++p) {
            const double u = (W.lo[p] - X.t0) * X.ginv;
            const int ci = u < 0.0 ? -1 : (u >= double(LIKE_NC) ? LIKE_NC : int(u));
            n += ci < g;
        }
        W.cell[g] = n;
    }
}

const char* const SETS[] = {"tiling", "jitter", "gaps", "overlap", "zero", "alternating"};

Windows make_windows(int set, int m, std::mt19937_64& rng)
{
    Windows W;
    const double x0 = -0.1, d = 0.2 / m;
    std::vector<double> edge(m + 1);
    for (int p = 0; p <= m; ++p) edge[p] = x0 + p * d;
    W.lo.resize(m);
    W.hi.resize(m);
    W.iw.resize(m);
    for (int p = 0; p < m; ++p) {
        const double c = x0 + (p + 0.5) * d;
        double f = 1.0;
        switch (set) {
        case 0: W.lo[p] = edge[p]; W.hi[p] = edge[p + 1]; continue;
        case 1:  // the joins a unit in the last place apart, either way
            W.lo[p] = std::nextafter(edge[p], (rng() & 1) ? 1.0 : -1.0);
            W.hi[p] = std::nextafter(edge[p + 1], (rng() & 1) ? 1.0 : -1.0);
            continue;
        case 2: f = 0.4; break;
        case 3: f = 3.5; break;
        case 4: f = 0.0; break;
        default: f = (p & 1) ? 1.4 : 0.6; break;
        }
        W.lo[p] = c - 0.5 * f * d;
        W.hi[p] = c + 0.5 * f * d;
    }
    for (int p = 0; p < m; ++p) W.iw[p] = 1.0 / (W.hi[p] - W.lo[p]);
    build_cells(W, m);
    return W;
}

int ring_sqrt(int u)  // lfg_k_elements.hpp: wd_ring_of
{
    int ir = int(std::sqrt(u * 0.5));
    if (2 * (ir + 1) * (ir + 1) <= u) ++ir;
    if (2 * ir * ir > u) --ir;
    return ir;
}

int ring_sqrtf(int u)  // lfg_k_lnlike.hpp: uring
{
    if (u >= 200) return 10 + (u - 200) / 25;
    int r = int(std::sqrt(float(u) * 0.5f));
    r += (2 * (r + 1) * (r + 1) <= u) ? 1 : 0;
    r -= (2 * r * r > u) ? 1 : 0;
    return r;
}

}  // namespace

int main()
{
    for (int u = 0; u < 700; ++u) {
        const int want = u < 200 ? ring_sqrt(u) : 10 + (u - 200) / 25;
        if (kRingOf[u] != want || kRingOf[u] != ring_sqrtf(u) || (u < 200 && !(2 * want * want <= u && u < 2 * (want + 1) * (want + 1)))) {
            std::printf("kRingOf[%d] = %d, the functions give %d and %d\n", u, int(kRingOf[u]), want, ring_sqrtf(u));
            return 1;
        }
    }
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const int MS[] = {1, 2, 3, 64, 65, 300, 512};
    for (int set = 0; set < 6; ++set) {
        long n_iv = 0, n_fast = 0, n_slow = 0;
        for (int m : MS) {
            Windows W = make_windows(set, m, rng);
            const PhaseIndex X = phase_index(W.lo.data(), W.cell.data(), m);
            const double* hi = W.hi.data();
            const double* iw = W.iw.data();
            std::vector<unsigned long long> ref(m + PAD, CANARY), nat(m + PAD, CANARY), bat(m + PAD, CANARY);
            for (int p = 0; p < m; ++p) ref[p] = nat[p] = bat[p] = 0;
            std::vector<double> as, bs;
            auto push = [&](double a, double b) {
                as.push_back(a);
                bs.push_back(b);
            };
            const double d = 0.2 / m;
            for (int i = 0; i < 3000; ++i) {  // anywhere, hanging over either side
                const double a = -0.15 + 0.3 * U(rng), len = 0.3 * U(rng) * U(rng);
                push(a, a + len);
            }
            for (int i = 0; i < 300; ++i) {  // inside one window
                const int p = int(U(rng) * m) % m;
                const double a = W.lo[p] + (W.hi[p] - W.lo[p]) * 0.5 * U(rng);
                push(a, a + (W.hi[p] - a) * U(rng));
            }
            for (int i = 0; i < 300; ++i) {  // a or b (or both) on a window's edge
                const int p = int(U(rng) * m) % m, q = int(U(rng) * m) % m, k = i % 6;
                const double ea = (k & 1) ? W.lo[p] : W.hi[p], eb = (i & 8) ? W.lo[q] : W.hi[q];
                if (k < 2) push(ea, ea + 3.0 * d * U(rng));
                else if (k < 4) push(ea - 3.0 * d * U(rng), ea);
                else push(std::fmin(ea, eb), std::fmax(ea, eb));
            }
            push(-0.2, 0.2);                        // covers every window
            push(W.lo[0], W.hi[m - 1]);             // ... exactly
            push(-0.3, -0.2);                       // wholly left
            push(-0.3, W.lo[0]);                    // left, touching
            push(0.2, 0.3);                         // wholly right
            push(W.hi[m - 1], 0.3);                 // right, touching
            for (size_t i = 0; i < as.size(); ++i) {
                const double a = as[i], b = bs[i], wn = 1e-3 * (0.1 + U(rng));
                if (!(a < b)) continue;
                // the element and its mirror, as PairSink::wd_disc passes them
                const Runs RR[2] = {element_runs(a, b, X, hi), element_runs(-b, -a, X, hi)};
                const double aa[2] = {a, -b}, bb[2] = {b, -a};
                for (int k = 0; k < 2; ++k) apply_runs(RR[k], aa[k], bb[k], wn, X, hi, iw, Add{ref.data()});
                bool took_slow = false;
                apply_runs_merged<2>(RR, aa, bb, wn, X, hi, iw, Add{nat.data()}, [&](bool slow) { return took_slow = slow; });
                apply_runs_merged<2>(RR, aa, bb, wn, X, hi, iw, Add{bat.data()}, [](bool) { return true; });
                // one interval alone, as PairSink::spot passes it
                const Runs R1[1] = {RR[0]};
                const double a1[1] = {a}, b1[1] = {b};
                apply_runs(RR[0], a, b, wn, X, hi, iw, Add{ref.data()});
                apply_runs_merged<1>(R1, a1, b1, wn, X, hi, iw, Add{nat.data()}, [](bool slow) { return slow; });
                apply_runs_merged<1>(R1, a1, b1, wn, X, hi, iw, Add{bat.data()}, [](bool) { return true; });
                ++n_iv;
                ++(took_slow ? n_slow : n_fast);
                for (int p = 0; p < m + PAD; ++p) {
                    const unsigned long long want = p < m ? ref[p] : CANARY;
                    if (ref[p] != want || nat[p] != want || bat[p] != want) {
                        std::printf("%s m=%d interval %zu [%.17g, %.17g] slot %d: reference %lld, merged %lld, batched %lld%s\n",
                                    SETS[set], m, i, a, b, p, (long long)ref[p], (long long)nat[p], (long long)bat[p],
                                    p < m ? "" : " (slot >= m: canary)");
                        return 1;
                    }
                }
            }
        }
        std::printf("%s %ld %ld %ld\n", SETS[set], n_iv, n_fast, n_slow);
    }
    return 0;
}
