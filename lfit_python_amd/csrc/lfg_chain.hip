// lfg_chain.hip -- a chain's summary on gfx950 (include/lfg_chain.h;
// MODEL_SPEC.md section 14).  A unit of its own: nothing here takes part in
// lfg.hip's code generation.  The job is memory bound: every sweep reads the
// chain once, in place, and keeps everything else on chip.
//
// How a sweep walks the chain.  A workgroup takes a run of rows (row r is
// step r / W, walker r % W) and a tile of columns.  A lane owns V adjacent
// columns of the tile for good (V = 2 where every address is 16-byte aligned:
// one 16-byte load per row) and steps through the rows: with Lc lane-columns
// in the tile, BLOCK / Lc rows are in flight per trip and neighbouring lanes
// read neighbouring elements, in the sampler's layout as in a flat chain.  A
// lane's (step, walker) advances by a fixed (ds, dw) with one carry, so no
// element costs an integer division, and a lane's column never changes, so
// its accumulators stay in registers.
//
//   k_moments   counts, extremes and a compensated sum per lane, folded over
//               the workgroup in lane order: one partial per (workgroup,
//               column) into ws
//   k_combine   one wave per column: the partials in a fixed order; writes
//               n, n_bad, mean, vmin, vmax and sets up the selection
//   k_deviations / k_combine_m2   the same two steps for the squared
//               deviations from that mean: m2 (numpy's own two passes)
//   k_hist      one radix pass: a 256-bin histogram of one key byte per
//               (column, distinct prefix), privatised in LDS, flushed with
//               integer atomics (exact, order-free)
//   k_pick      per column one wave per tracked rank: scans the histogram,
//               extends the rank's prefix by a byte, clears the histogram;
//               the last pass writes ostat and quant
//   k_walker / k_rhat   per-walker moments and Gelman-Rubin from them
//   k_clip      the next window of a sigma clip
// Eight passes whatever the data holds.  Ranks of a column that still share
// a prefix share a histogram, and an element's key can match one prefix at
// most, so it costs one LDS atomic per pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lfg_chain.hpp"

using namespace lfg;

namespace {

constexpr int MO_BLOCK = 256;        // k_moments
constexpr int MO_MAX_BLOCKS = 1024;  // four workgroups for each of the 256 CUs
constexpr int MO_TILE = 256;         // columns of one k_moments workgroup
constexpr int HI_BLOCK = 512;        // k_hist
constexpr int HI_MAX_BLOCKS = 512;
constexpr int HI_SLOTS = 128;  // histograms of one workgroup: 128 KiB of the CU's 160 KiB
constexpr int TILE_ROWS = 256;       // rows of one workgroup at the least
constexpr int NBIN = 256;
constexpr int MAX_TR = 2 * LFG_CHAIN_MAX_NQ;
constexpr int RH_BLOCK = 256;
constexpr int RH_MAX_CHUNKS = 64;
constexpr long long RH_LANES = 262144;  // k_walker splits the steps until it has this many lanes

inline int launch_ok() { return hipGetLastError() == hipSuccess ? LFG_OK : LFG_E_LAUNCH; }
inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }
inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

struct View {
    const double* base;
    long long steps, W, step_ld, walker_ld, rows;
    int C;
};

struct Fracs {
    double f[LFG_CHAIN_MAX_NQ];
};

// what a call launches and where its scratch lies: a function of the sizes alone
struct Plan {
    int mo_blocks, hi_blocks, ntr, rh_chunks;
    long long rh_len;
    size_t part, pref, rank, rep, hist, wmean, wm2, total;
};

Plan plan_of(long long steps, long long W, int C, int nq)
{
    Plan P;
    const long long rows = steps * W;
    P.mo_blocks = int(std::min<long long>(MO_MAX_BLOCKS, std::max<long long>(1, ceil_div(rows, TILE_ROWS))));
    P.hi_blocks = int(std::min<long long>(HI_MAX_BLOCKS, std::max<long long>(1, ceil_div(rows, TILE_ROWS))));
    P.ntr = 2 * nq;
    const long long wc = std::max<long long>(1, W * C);
    P.rh_chunks = int(std::max<long long>(1, std::min<long long>(std::min<long long>(RH_MAX_CHUNKS, steps),
                                                                 ceil_div(RH_LANES, wc))));
    P.rh_len = std::max<long long>(1, ceil_div(steps, P.rh_chunks));
    size_t o = 0;
    P.part = o;
    o += up256(size_t(P.mo_blocks) * 6 * C * 8);
    P.pref = o;
    o += up256(size_t(C) * MAX_TR * 8);
    P.rank = o;
    o += up256(size_t(C) * MAX_TR * 8);
    P.rep = o;
    o += up256(size_t(C) * MAX_TR * 4);
    P.hist = o;
    o += up256(size_t(C) * P.ntr * NBIN * 8);
    P.wmean = o;
    o += up256(size_t(P.rh_chunks) * size_t(wc) * 8);
    P.wm2 = o;
    o += up256(size_t(P.rh_chunks) * size_t(wc) * 8);
    P.total = o;
    return P;
}

// tiles of at most `cap` (even) columns, of one even size
inline void tiles_of(int C, int cap, int& ntile, int& ct)
{
    ntile = (C + cap - 1) / cap;
    ct = (C + ntile - 1) / ntile;
    ct += ct & 1;
    ntile = (C + ct - 1) / ct;
}

inline int hist_cap(int ntr) { return (HI_SLOTS / ntr) & ~1; }

// ---- a lane's walk over its rows (file comment) ----
template <int V, int BLOCK>
struct Lane {
    bool active;
    int col;            // first of the lane's V columns
    long long r, rend;  // next row, end of the workgroup's rows
    long long s, w;     // r's step and walker
    long long ds, dw;
    int rpi;

    __device__ Lane(const View& v, int c0, int ct, int blocks)
    {
        const int lc_n = ct / V, tid = threadIdx.x;
        rpi = BLOCK / lc_n;
        active = tid < rpi * lc_n;
        col = c0 + (tid % lc_n) * V;
        const long long chunk = (v.rows + blocks - 1) / blocks;
        const long long r0 = chunk * blockIdx.x;
        rend = min(v.rows, r0 + chunk);
        r = r0 + tid / lc_n;
        s = r / v.W;
        w = r - s * v.W;
        ds = rpi / v.W;
        dw = rpi - ds * v.W;
    }
    __device__ bool more() const { return active && r < rend; }
    __device__ const double* at(const View& v) const { return v.base + (s * v.step_ld + w * v.walker_ld + col); }
    __device__ void next(const View& v)
    {
        r += rpi;
        s += ds;
        w += dw;
        if (w >= v.W) {
            w -= v.W;
            s += 1;
        }
    }
};

template <int V>
__device__ inline void load_v(const double* p, double (&x)[V])
{
    if constexpr (V == 2) {
        const double2 t = *reinterpret_cast<const double2*>(p);
        x[0] = t.x;
        x[1] = t.y;
    } else {
        x[0] = *p;
    }
}

// ---- moments ----
// Two sweeps, as numpy's own var: the first for the counts, the compensated
// sum and the extremes, the second for the deviations from the mean the
// first one gave.  part: [6][blocks][C] (n, bad as int64; sum, comp, lo, hi),
// then [3][blocks][C] (s1, s2, c2).
template <int V>
__global__ __launch_bounds__(MO_BLOCK) void k_moments(View v, const double* __restrict__ window, int ct, int blocks,
                                                      double* __restrict__ part)
{
    __shared__ long long sh_n[MO_BLOCK * V], sh_bad[MO_BLOCK * V];
    __shared__ double sh_sum[MO_BLOCK * V], sh_comp[MO_BLOCK * V], sh_lo[MO_BLOCK * V], sh_hi[MO_BLOCK * V];
    const int c0 = blockIdx.y * ct;
    const int ctile = min(ct, v.C - c0);
    Lane<V, MO_BLOCK> L(v, c0, ctile, blocks);
    ChainMom a[V];
    double wl[V], wh[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        a[k] = chain_mom_empty();
        wl[k] = (window && L.active) ? window[2 * (L.col + k)] : -INFINITY;
        wh[k] = (window && L.active) ? window[2 * (L.col + k) + 1] : INFINITY;
    }
    while (L.more()) {
        double x[V];
        load_v<V>(L.at(v), x);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (!chain_finite(x[k]))
                a[k].bad += 1;
            else if (x[k] >= wl[k] && x[k] <= wh[k])
                chain_mom_add(a[k], x[k]);
        }
        L.next(v);
    }
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        sh_n[tid * V + k] = a[k].n;
        sh_bad[tid * V + k] = a[k].bad;
        sh_sum[tid * V + k] = a[k].sum;
        sh_comp[tid * V + k] = a[k].comp;
        sh_lo[tid * V + k] = a[k].lo;
        sh_hi[tid * V + k] = a[k].hi;
    }
    __syncthreads();
    const int lc_n = ctile / V;
    if (tid < lc_n) {
        const size_t plane = size_t(blocks) * v.C;
        long long* pi = reinterpret_cast<long long*>(part);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            ChainMom t = a[k];
            for (int j = 1; j < L.rpi; ++j) {
                const int i = (j * lc_n + tid) * V + k;
                ChainMom b;
                b.n = sh_n[i];
                b.bad = sh_bad[i];
                b.sum = sh_sum[i];
                b.comp = sh_comp[i];
                b.lo = sh_lo[i];
                b.hi = sh_hi[i];
                chain_mom_merge(t, b);
            }
            const size_t o = size_t(blockIdx.x) * v.C + (L.col + k);
            pi[o] = t.n;
            pi[plane + o] = t.bad;
            part[2 * plane + o] = t.sum;
            part[3 * plane + o] = t.comp;
            part[4 * plane + o] = t.lo;
            part[5 * plane + o] = t.hi;
        }
    }
}

template <int V>
__global__ __launch_bounds__(MO_BLOCK) void k_deviations(View v, const double* __restrict__ window, int ct, int blocks,
                                                         const double* __restrict__ mean, double* __restrict__ part)
{
    __shared__ double sh_s1[MO_BLOCK * V], sh_s2[MO_BLOCK * V], sh_c2[MO_BLOCK * V];
    const int c0 = blockIdx.y * ct;
    const int ctile = min(ct, v.C - c0);
    Lane<V, MO_BLOCK> L(v, c0, ctile, blocks);
    ChainDev a[V];
    double wl[V], wh[V], mu[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        a[k].s1 = a[k].s2 = a[k].c2 = 0.0;
        wl[k] = (window && L.active) ? window[2 * (L.col + k)] : -INFINITY;
        wh[k] = (window && L.active) ? window[2 * (L.col + k) + 1] : INFINITY;
        mu[k] = L.active ? mean[L.col + k] : 0.0;
    }
    while (L.more()) {
        double x[V];
        load_v<V>(L.at(v), x);
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (chain_used(x[k], wl[k], wh[k])) chain_dev_add(a[k], x[k], mu[k]);
        L.next(v);
    }
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        sh_s1[tid * V + k] = a[k].s1;
        sh_s2[tid * V + k] = a[k].s2;
        sh_c2[tid * V + k] = a[k].c2;
    }
    __syncthreads();
    const int lc_n = ctile / V;
    if (tid < lc_n) {
        const size_t plane = size_t(blocks) * v.C;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            ChainDev t = a[k];
            for (int j = 1; j < L.rpi; ++j) {
                const int i = (j * lc_n + tid) * V + k;
                ChainDev b;
                b.s1 = sh_s1[i];
                b.s2 = sh_s2[i];
                b.c2 = sh_c2[i];
                chain_dev_merge(t, b);
            }
            const size_t o = size_t(blockIdx.x) * v.C + (L.col + k);
            part[o] = t.s1;
            part[plane + o] = t.s2;
            part[2 * plane + o] = t.c2;
        }
    }
}

__device__ inline ChainMom mom_shfl_down(const ChainMom& a, int off)
{
    ChainMom b;
    b.n = __shfl_down(a.n, off);
    b.bad = __shfl_down(a.bad, off);
    b.sum = __shfl_down(a.sum, off);
    b.comp = __shfl_down(a.comp, off);
    b.lo = __shfl_down(a.lo, off);
    b.hi = __shfl_down(a.hi, off);
    return b;
}

// one wave per column: lane l takes partials l, l + 64, ... in order, the
// lanes then fold as a fixed tree.  Lane 0 writes the column's outputs and
// the selection's starting state; the wave clears the column's histograms.
__global__ __launch_bounds__(64) void k_combine(int C, int blocks, const double* __restrict__ part, Fracs fr, int nq,
                                                long long* __restrict__ n, long long* __restrict__ n_bad,
                                                double* __restrict__ mean, double* __restrict__ vmin,
                                                double* __restrict__ vmax, unsigned long long* __restrict__ pref,
                                                long long* __restrict__ rank, int* __restrict__ rep,
                                                unsigned long long* __restrict__ hist)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    const size_t plane = size_t(blocks) * C;
    const long long* pi = reinterpret_cast<const long long*>(part);
    ChainMom a = chain_mom_empty();
    for (int b = lane; b < blocks; b += 64) {
        const size_t o = size_t(b) * C + c;
        ChainMom t;
        t.n = pi[o];
        t.bad = pi[plane + o];
        t.sum = part[2 * plane + o];
        t.comp = part[3 * plane + o];
        t.lo = part[4 * plane + o];
        t.hi = part[5 * plane + o];
        chain_mom_merge(a, t);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const ChainMom b = mom_shfl_down(a, off);
        if (lane + off < 64) chain_mom_merge(a, b);
    }
    const int ntr = 2 * nq;
    for (int i = lane; i < ntr * NBIN; i += 64) hist[size_t(c) * ntr * NBIN + i] = 0ull;
    if (lane == 0) {
        n[c] = a.n;
        n_bad[c] = a.bad;
        mean[c] = chain_mean(a);
        vmin[c] = a.n ? a.lo : NAN;
        vmax[c] = a.n ? a.hi : NAN;
        for (int q = 0; q < nq; ++q) {
            long long lo = -1, hi = -1;
            double g;
            if (a.n) chain_rank(fr.f[q], a.n, lo, hi, g);
            rank[c * MAX_TR + 2 * q] = lo;
            rank[c * MAX_TR + 2 * q + 1] = hi;
        }
        for (int t = 0; t < ntr; ++t) {
            pref[c * MAX_TR + t] = 0ull;
            rep[c * MAX_TR + t] = 0;  // no byte chosen yet: every rank shares histogram 0
        }
    }
}

// the second sweep's partials, in the same fixed order
__global__ __launch_bounds__(64) void k_combine_m2(int C, int blocks, const double* __restrict__ part,
                                                   const long long* __restrict__ n, double* __restrict__ m2)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    const size_t plane = size_t(blocks) * C;
    ChainDev a = {0.0, 0.0, 0.0};
    for (int b = lane; b < blocks; b += 64) {
        const size_t o = size_t(b) * C + c;
        ChainDev t = {part[o], part[plane + o], part[2 * plane + o]};
        chain_dev_merge(a, t);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        ChainDev b;
        b.s1 = __shfl_down(a.s1, off);
        b.s2 = __shfl_down(a.s2, off);
        b.c2 = __shfl_down(a.c2, off);
        if (lane + off < 64) chain_dev_merge(a, b);
    }
    if (lane == 0) m2[c] = chain_m2(a, n[c]);
}

// ---- the radix passes ----
// pass p counts key byte 7 - p of the used values whose higher bytes equal a
// tracked prefix.  LDS: hist u32 [ctile * ntr][256], then the prefixes, the
// list of distinct-prefix slots per column and its length.
template <int V>
__global__ __launch_bounds__(HI_BLOCK) void k_hist(View v, const double* __restrict__ window, int ct, int blocks,
                                                   int ntr, int pass, const unsigned long long* __restrict__ pref,
                                                   const int* __restrict__ rep,
                                                   unsigned long long* __restrict__ hist)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int c0 = blockIdx.y * ct;
    const int ctile = min(ct, v.C - c0);
    const int nslot = ctile * ntr;
    unsigned int* h = reinterpret_cast<unsigned int*>(lds);
    unsigned long long* spref = reinterpret_cast<unsigned long long*>(lds + size_t(ct) * ntr * NBIN * 4);
    int* snu = reinterpret_cast<int*>(spref + ct * ntr);
    unsigned char* slist = reinterpret_cast<unsigned char*>(snu + ct);
    const int tid = threadIdx.x;
    for (int i = tid; i < nslot * NBIN; i += HI_BLOCK) h[i] = 0u;
    for (int i = tid; i < nslot; i += HI_BLOCK) {
        const int lc = i / ntr, t = i - lc * ntr;
        spref[i] = pref[(c0 + lc) * MAX_TR + t];
    }
    for (int lc = tid; lc < ctile; lc += HI_BLOCK) {
        int nu = 0;
        for (int t = 0; t < ntr; ++t)
            if (rep[(c0 + lc) * MAX_TR + t] == t) slist[lc * ntr + nu++] = (unsigned char)t;
        snu[lc] = nu;
    }
    __syncthreads();

    Lane<V, HI_BLOCK> L(v, c0, ctile, blocks);
    double wl[V], wh[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        wl[k] = (window && L.active) ? window[2 * (L.col + k)] : -INFINITY;
        wh[k] = (window && L.active) ? window[2 * (L.col + k) + 1] : INFINITY;
    }
    const int shift = 56 - 8 * pass;
    const int lcol = L.col - c0;
    while (L.more()) {
        double x[V];
        load_v<V>(L.at(v), x);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (chain_used(x[k], wl[k], wh[k])) {
                const uint64_t key = chain_key(x[k]);
                const uint64_t top = pass ? (key >> (shift + 8)) : 0ull;
                const unsigned digit = unsigned(key >> shift) & 255u;
                const int lc = lcol + k, nu = snu[lc];
                for (int j = 0; j < nu; ++j) {
                    const int t = slist[lc * ntr + j];
                    if (spref[lc * ntr + t] == top) {
                        atomicAdd(&h[(lc * ntr + t) * NBIN + digit], 1u);
                        break;  // distinct prefixes of one length are disjoint
                    }
                }
            }
        }
        L.next(v);
    }
    __syncthreads();
    unsigned long long* g = hist + size_t(c0) * ntr * NBIN;
    for (int i = tid; i < nslot * NBIN; i += HI_BLOCK) {
        const unsigned int cnt = h[i];
        if (cnt) atomicAdd(&g[i], (unsigned long long)cnt);
    }
}

// one workgroup per column, wave t for tracked rank t
__global__ __launch_bounds__(64 * MAX_TR) void k_pick(int ntr, int nq, int last, Fracs fr, const long long* __restrict__ n,
                       unsigned long long* __restrict__ pref, long long* __restrict__ rank, int* __restrict__ rep,
                       unsigned long long* __restrict__ hist, double* __restrict__ ostat, double* __restrict__ quant)
{
    __shared__ unsigned long long snew[MAX_TR];
    __shared__ long long srank[MAX_TR];
    const int c = blockIdx.x, t = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = c * MAX_TR + t;
    unsigned long long* hc = hist + size_t(c) * ntr * NBIN;
    long long k = rank[slot];
    unsigned long long p = pref[slot];
    if (k >= 0) {
        const unsigned long long* hh = hc + size_t(rep[slot]) * NBIN + 4 * lane;
        const unsigned long long c0 = hh[0], c1 = hh[1], c2 = hh[2], c3 = hh[3];
        const unsigned long long mine = c0 + c1 + c2 + c3;
        unsigned long long incl = mine;
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        const unsigned long long uk = (unsigned long long)k;
        const unsigned long long m = __ballot(incl > uk);
        if (m == 0ull) {
            k = -1;  // (cannot happen: the rank lies inside its prefix's count)
        } else {
            const int src = __ffsll((long long)m) - 1;
            unsigned long long before = incl - mine;  // exclusive
            int d = 0;
            if (uk >= before + c0) {
                before += c0;
                d = 1;
                if (uk >= before + c1) {
                    before += c1;
                    d = 2;
                    if (uk >= before + c2) {
                        before += c2;
                        d = 3;
                    }
                }
            }
            const unsigned long long bsel = __shfl(before, src);
            const int dsel = __shfl(d, src);
            k = (long long)(uk - bsel);
            p = (p << 8) | (unsigned long long)(4 * src + dsel);
        }
    }
    if (lane == 0) {
        snew[t] = p;
        srank[t] = k;
        pref[slot] = p;
        rank[slot] = k;
    }
    __syncthreads();  // every wave has read its histogram
#pragma unroll
    for (int i = 0; i < 4; ++i) hc[size_t(t) * NBIN + 4 * lane + i] = 0ull;
    if (threadIdx.x < ntr) {
        const int me = threadIdx.x;
        int r = me;
        for (int j = me - 1; j >= 0; --j)
            if (snew[j] == snew[me]) r = j;
        rep[c * MAX_TR + me] = r;
    }
    if (last && threadIdx.x < nq) {
        const int q = threadIdx.x;
        double a = NAN, b = NAN, val = NAN;
        const long long nc = n[c];
        if (nc > 0 && srank[2 * q] >= 0 && srank[2 * q + 1] >= 0) {
            long long lo, hi;
            double g;
            chain_rank(fr.f[q], nc, lo, hi, g);
            a = chain_unkey(snew[2 * q]);
            b = chain_unkey(snew[2 * q + 1]);
            val = chain_lerp(a, b, g);
        }
        ostat[(size_t(c) * nq + q) * 2] = a;
        ostat[(size_t(c) * nq + q) * 2 + 1] = b;
        quant[size_t(c) * nq + q] = val;
    }
}

// ---- R-hat ----
// lane e = w * C + c of chunk j: Welford over the chunk's steps of walker w,
// column c.  A non-finite value marks the pair with NaN.
__global__ __launch_bounds__(RH_BLOCK) void k_walker(View v, long long len, double* __restrict__ wmean,
                                                     double* __restrict__ wm2)
{
    const long long wc = v.W * v.C;
    const long long e = (long long)blockIdx.x * RH_BLOCK + threadIdx.x;
    if (e >= wc) return;
    const long long w = e / v.C;
    const int c = int(e - w * v.C);
    const long long s0 = len * blockIdx.y, s1 = min(v.steps, s0 + len);
    const double* p = v.base + (s0 * v.step_ld + w * v.walker_ld + c);
    double na = 0.0, ma = 0.0, sa = 0.0;
    bool bad = false;
    for (long long s = s0; s < s1; ++s, p += v.step_ld) {
        const double x = *p;
        if (!chain_finite(x))
            bad = true;
        else
            chain_pair_add(na, ma, sa, x);
    }
    const size_t o = size_t(blockIdx.y) * size_t(wc) + size_t(e);
    wmean[o] = bad ? NAN : ma;
    wm2[o] = bad ? NAN : sa;
}

// one workgroup per column: lane l takes walkers l, l + 256, ...; a walker's
// chunks combine in step order, the lanes fold as a fixed tree
__global__ __launch_bounds__(RH_BLOCK) void k_rhat(View v, long long len, int chunks,
                                                   const double* __restrict__ wmean, const double* __restrict__ wm2,
                                                   double* __restrict__ rhat)
{
    __shared__ double sn[RH_BLOCK], sm[RH_BLOCK], ss[RH_BLOCK], sw[RH_BLOCK];
    __shared__ int sbad[RH_BLOCK];
    const int c = blockIdx.x, tid = threadIdx.x;
    const long long wc = v.W * v.C;
    double gn = 0.0, gm = 0.0, gs = 0.0, within = 0.0;
    int bad = 0;
    for (long long w = tid; w < v.W; w += RH_BLOCK) {
        double na = 0.0, ma = 0.0, sa = 0.0;
        for (int j = 0; j < chunks; ++j) {
            const long long s0 = len * j, s1 = min(v.steps, s0 + len);
            if (s1 <= s0) break;
            const size_t o = size_t(j) * size_t(wc) + size_t(w * v.C + c);
            const double mb = wmean[o], sb = wm2[o];
            if (mb != mb) bad = 1;
            chain_pair_merge(na, ma, sa, double(s1 - s0), mb, sb);
        }
        chain_pair_merge(gn, gm, gs, 1.0, ma, 0.0);
        within += sa;
    }
    sn[tid] = gn;
    sm[tid] = gm;
    ss[tid] = gs;
    sw[tid] = within;
    sbad[tid] = bad;
    __syncthreads();
    for (int off = RH_BLOCK / 2; off >= 1; off >>= 1) {
        if (tid < off) {
            chain_pair_merge(sn[tid], sm[tid], ss[tid], sn[tid + off], sm[tid + off], ss[tid + off]);
            sw[tid] += sw[tid + off];
            sbad[tid] |= sbad[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) rhat[c] = sbad[0] ? NAN : chain_rhat(v.W, v.steps, ss[0], sw[0]);
}

// steps = 0 or W = 0
__global__ void k_empty(int C, int nq, long long* n, long long* n_bad, double* mean, double* m2, double* vmin,
                        double* vmax, double* ostat, double* quant, double* rhat)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    n[c] = 0;
    n_bad[c] = 0;
    mean[c] = m2[c] = vmin[c] = vmax[c] = NAN;
    if (rhat) rhat[c] = NAN;
    for (int q = 0; q < nq; ++q) {
        ostat[(size_t(c) * nq + q) * 2] = ostat[(size_t(c) * nq + q) * 2 + 1] = NAN;
        quant[size_t(c) * nq + q] = NAN;
    }
}

__global__ void k_clip(const long long* __restrict__ n, const double* __restrict__ m2, const double* __restrict__ med,
                       long long med_ld, double sigma, const double* win_in, double* win_out, int C)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double lo = win_in ? win_in[2 * c] : -INFINITY, hi = win_in ? win_in[2 * c + 1] : INFINITY;
    chain_clip(n[c], m2[c], med[size_t(c) * size_t(med_ld)], sigma, lo, hi);
    win_out[2 * c] = lo;
    win_out[2 * c + 1] = hi;
}

size_t hist_lds_bytes(int ct, int ntr)
{
    size_t b = size_t(ct) * ntr * NBIN * 4 + size_t(ct) * ntr * 8 + size_t(ct) * 4 + size_t(ct) * ntr;
    return (b + 15) & ~size_t(15);
}

// k_hist asks for more dynamic LDS than the default limit.  Set on every call
// (a host-side table entry of the current device, no synchronisation): a
// process may drive several devices.
template <int V>
bool hist_lds_allowed()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hist<V>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               HI_SLOTS * NBIN * 4 + 4096) == hipSuccess;
}

}  // namespace

extern "C" {

size_t lfg_chain_workspace_size(long long steps, long long W, int C, int nq)
{
    if (steps < 0 || W < 0 || C < 1 || C > LFG_CHAIN_MAX_C || nq < 0 || nq > LFG_CHAIN_MAX_NQ) return 0;
    return plan_of(steps, W, C, nq).total;
}

int lfg_chain_tile_rows(void) { return TILE_ROWS; }

int lfg_chain_hist_tile(int nq) { return (nq < 1 || nq > LFG_CHAIN_MAX_NQ) ? 0 : hist_cap(2 * nq); }

int lfg_chain_stats(const double* base, long long steps, long long W, int C, long long step_ld, long long walker_ld,
                    const double* window, const double* fracs, int nq, long long* n, long long* n_bad, double* mean,
                    double* m2, double* vmin, double* vmax, double* ostat, double* quant, double* rhat, void* ws,
                    size_t ws_bytes, void* stream)
{
    if (!chain_view_ok(steps, W, C, step_ld, walker_ld) || !chain_fracs_ok(fracs, nq)) return LFG_E_ARGS;
    if (!n || !n_bad || !mean || !m2 || !vmin || !vmax || (nq > 0 && (!ostat || !quant))) return LFG_E_ARGS;
    if (rhat && window) return LFG_E_ARGS;
    const Plan P = plan_of(steps, W, C, nq);
    if (!ws || ws_bytes < P.total) return LFG_E_ARGS;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (steps == 0 || W == 0) {
        hipLaunchKernelGGL(k_empty, dim3((C + 255) / 256), dim3(256), 0, st, C, nq, n, n_bad, mean, m2, vmin, vmax,
                           ostat, quant, rhat);
        return launch_ok();
    }
    if (!base) return LFG_E_ARGS;
    View v;
    v.base = base;
    v.steps = steps;
    v.W = W;
    v.step_ld = step_ld;
    v.walker_ld = W == 1 ? 1 : walker_ld;  // (never multiplied by anything but 0 then)
    v.rows = steps * W;
    v.C = C;
    // a lane takes two columns per load where every such address is 16-byte aligned
    const bool wide = (reinterpret_cast<uintptr_t>(base) % 16 == 0) && C % 2 == 0 && step_ld % 2 == 0 &&
                      (W == 1 || walker_ld % 2 == 0);
    Fracs fr;
    for (int i = 0; i < LFG_CHAIN_MAX_NQ; ++i) fr.f[i] = i < nq ? fracs[i] : 0.0;
    unsigned char* wsb = static_cast<unsigned char*>(ws);
    double* part = reinterpret_cast<double*>(wsb + P.part);
    unsigned long long* pref = reinterpret_cast<unsigned long long*>(wsb + P.pref);
    long long* rank = reinterpret_cast<long long*>(wsb + P.rank);
    int* rep = reinterpret_cast<int*>(wsb + P.rep);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(wsb + P.hist);
    double* wmean = reinterpret_cast<double*>(wsb + P.wmean);
    double* wm2 = reinterpret_cast<double*>(wsb + P.wm2);

    if (nq > 0 && !(wide ? hist_lds_allowed<2>() : hist_lds_allowed<1>())) return LFG_E_LAUNCH;

    int ntile, ct;
    tiles_of(C, MO_TILE, ntile, ct);
    if (wide)
        hipLaunchKernelGGL(k_moments<2>, dim3(P.mo_blocks, ntile), dim3(MO_BLOCK), 0, st, v, window, ct, P.mo_blocks,
                           part);
    else
        hipLaunchKernelGGL(k_moments<1>, dim3(P.mo_blocks, ntile), dim3(MO_BLOCK), 0, st, v, window, ct, P.mo_blocks,
                           part);
    hipLaunchKernelGGL(k_combine, dim3(C), dim3(64), 0, st, C, P.mo_blocks, part, fr, nq, n, n_bad, mean, vmin, vmax,
                       pref, rank, rep, hist);
    if (wide)
        hipLaunchKernelGGL(k_deviations<2>, dim3(P.mo_blocks, ntile), dim3(MO_BLOCK), 0, st, v, window, ct,
                           P.mo_blocks, mean, part);
    else
        hipLaunchKernelGGL(k_deviations<1>, dim3(P.mo_blocks, ntile), dim3(MO_BLOCK), 0, st, v, window, ct,
                           P.mo_blocks, mean, part);
    hipLaunchKernelGGL(k_combine_m2, dim3(C), dim3(64), 0, st, C, P.mo_blocks, part, n, m2);
    if (rhat) {
        const long long wc = W * C;
        hipLaunchKernelGGL(k_walker, dim3((unsigned)ceil_div(wc, RH_BLOCK), P.rh_chunks), dim3(RH_BLOCK), 0, st, v,
                           P.rh_len, wmean, wm2);
        hipLaunchKernelGGL(k_rhat, dim3(C), dim3(RH_BLOCK), 0, st, v, P.rh_len, P.rh_chunks, wmean, wm2, rhat);
    }
    if (nq > 0) {
        tiles_of(C, hist_cap(P.ntr), ntile, ct);
        const size_t lds = hist_lds_bytes(ct, P.ntr);
        for (int pass = 0; pass < 8; ++pass) {
            if (wide)
                hipLaunchKernelGGL(k_hist<2>, dim3(P.hi_blocks, ntile), dim3(HI_BLOCK), lds, st, v, window, ct,
                                   P.hi_blocks, P.ntr, pass, pref, rep, hist);
            else
                hipLaunchKernelGGL(k_hist<1>, dim3(P.hi_blocks, ntile), dim3(HI_BLOCK), lds, st, v, window, ct,
                                   P.hi_blocks, P.ntr, pass, pref, rep, hist);
            hipLaunchKernelGGL(k_pick, dim3(C), dim3(64 * P.ntr), 0, st, P.ntr, nq, int(pass == 7), fr, n, pref, rank,
                               rep, hist, ostat, quant);
        }
    }
    return launch_ok();
}

int lfg_chain_clip(const long long* n, const double* m2, const double* med, long long med_ld, double sigma,
                   const double* win_in, double* win_out, int C, void* stream)
{
    if (!n || !m2 || !med || !win_out || C < 1 || C > LFG_CHAIN_MAX_C || med_ld < 1 || !(sigma >= 0.0))
        return LFG_E_ARGS;
    hipLaunchKernelGGL(k_clip, dim3((C + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), n, m2, med,
                       med_ld, sigma, win_in, win_out, C);
    return launch_ok();
}

}  // extern "C"
