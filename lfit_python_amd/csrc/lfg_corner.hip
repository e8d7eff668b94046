// lfg_corner.hip -- a corner plot's data on gfx950 (include/lfg_corner.h;
// MODEL_SPEC.md section 16).  A unit of its own: nothing here takes part in
// lfg.hip's code generation.
//
//   k_prepare   zeroes h1 and h2, turns the K ranges into the columns'
//               binning (lo, hi, step, mobile) in ws and writes the flags
//   k_corner    the sweep.  A workgroup takes a run of rows and a tile of
//               pairs, lfg_corner_pair_tile(nb) of them, whose histograms it
//               keeps in LDS as uint32.  Rows go through in stages: a lane
//               owns one of the K columns for good and loads and bins that
//               column's value of CO_TRIPS rows (neighbouring lanes read
//               neighbouring columns of a row; (step, walker) advance by a
//               fixed stride with one carry, no division), leaving one byte
//               per (row, column) in LDS.  Then every (row, pair of the
//               tile) takes one LDS add, lanes running over the pairs first
//               so that a wave spreads over the tile's histograms.  Tile 0
//               also counts the marginals.  At the end of its rows the
//               workgroup adds its non-zero bins to h1 / h2 with 64-bit
//               integer atomics: exact in any order.
//   k_levels    one workgroup per pair: a bitonic sort of the counts in LDS,
//               descending, a scan, and per fraction the last position inside
//
// The chain is read once per pair tile.  No floating-point atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lfg_corner.hpp"

using namespace lfg;

namespace {

constexpr int CO_BLOCK = 1024;       // k_corner: one workgroup per CU, sixteen waves
constexpr int CO_TRIPS = 8;          // rows a lane loads per stage
constexpr int CO_WORKGROUPS = 256;   // workgroups of a large call: one for each CU
constexpr int TILE_ROWS = 256;       // rows of one workgroup at the least
constexpr int CO_MAX_TILE = 512;     // pairs of one tile at the most
// LDS of one workgroup, of the CU's 160 KiB: the pair histograms and the
// marginals in 144 KiB, then the stage's bins (CO_BLOCK * CO_TRIPS bytes),
// the tile's pair list and the columns' binning
constexpr int CO_HIST_BYTES = 144 * 1024;
constexpr int CO_STAGE_BYTES = CO_BLOCK * CO_TRIPS;
constexpr int CO_LDS_BYTES = CO_HIST_BYTES + CO_STAGE_BYTES + CO_MAX_TILE * 2 + 1024;
static_assert(CO_LDS_BYTES <= 160 * 1024, "k_corner's LDS exceeds the CU's");
constexpr int LV_BLOCK = 256;        // k_levels
constexpr int LV_MAX = LFG_CORNER_MAX_BINS * LFG_CORNER_MAX_BINS;

inline int launch_ok() { return hipGetLastError() == hipSuccess ? LFG_OK : LFG_E_LAUNCH; }
inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }
inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

inline int pair_tile(int nb)
{
    const int room = CO_HIST_BYTES - LFG_CORNER_MAX_K * nb * 4;  // the marginals of the most columns
    return std::min(CO_MAX_TILE, room / (nb * nb * 4));
}

struct Cols {
    int c[LFG_CORNER_MAX_K];
};

struct Fracs {
    double f[LFG_CORNER_MAX_LEVELS];
};

struct View {
    const double* base;
    long long steps, W, step_ld, walker_ld, rows;
};

__global__ void k_prepare(const double* __restrict__ range, int K, int nb, CornerCol* __restrict__ col,
                          int* __restrict__ flag, long long* __restrict__ h1, long long* __restrict__ h2,
                          long long n2)
{
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long n1 = (long long)K * nb;
    for (long long i = i0; i < n1; i += stride) h1[i] = 0;
    for (long long i = i0; i < n2; i += stride) h2[i] = 0;
    if (i0 < K) {
        const CornerCol c = corner_col(range[2 * i0], range[2 * i0 + 1], nb);
        if (col) col[i0] = c;
        flag[i0] = c.mobile ? 0 : 1;
    }
}

// LDS: h2 u32 [tp][nb * nb], h1 u32 [K][nb], bins u8 [rows of a stage][K],
// pairs u16 [tp]
__global__ __launch_bounds__(CO_BLOCK) void k_corner(View v, Cols cols, int K, int nb, int tile, int blocks,
                                                     const CornerCol* __restrict__ col,
                                                     unsigned long long* __restrict__ h1,
                                                     unsigned long long* __restrict__ h2)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int P = corner_pair_count(K);
    const int p0 = blockIdx.y * tile;
    const int tp = min(tile, P - p0);  // (0 for K = 1: the marginals alone)
    const int nb2 = nb * nb;
    const bool marg = blockIdx.y == 0;
    unsigned int* sh2 = reinterpret_cast<unsigned int*>(lds);
    unsigned int* sh1 = sh2 + size_t(tile) * nb2;
    unsigned char* sbin = reinterpret_cast<unsigned char*>(sh1 + K * nb);
    unsigned short* spair = reinterpret_cast<unsigned short*>(lds + CO_HIST_BYTES + CO_STAGE_BYTES);
    const int tid = threadIdx.x;
    for (int i = tid; i < tp * nb2; i += CO_BLOCK) sh2[i] = 0u;
    for (int i = tid; i < K * nb; i += CO_BLOCK) sh1[i] = 0u;
    for (int i = tid; i < tp; i += CO_BLOCK) {
        int a, b;
        corner_pair_of(K, p0 + i, a, b);
        spair[i] = (unsigned short)(a | (b << 8));
    }

    // the lane's column and its walk over the rows
    const int rpi = CO_BLOCK / K;  // rows in flight per trip
    const bool active = tid < rpi * K;
    const int k = tid % K, lr = tid / K;
    const CornerCol my = col[k];
    const int gcol = cols.c[k];
    // this workgroup's rows.  A bin is a uint32: between the zeroing above
    // and the flush below a workgroup sees chunk rows, and the host keeps
    // chunk <= 2^31 (blocks >= rows / 2^31), so no bin can wrap.
    const long long chunk = (v.rows + blocks - 1) / blocks;
    const long long r0 = chunk * blockIdx.x;
    const long long rend = min(v.rows, r0 + chunk);
    long long r = r0 + lr;
    long long s = r / v.W, w = r - s * v.W;
    const long long ds = rpi / v.W, dw = rpi - ds * v.W;
    const int stage_rows = rpi * CO_TRIPS;
    // a lane's walk over the (row, pair) items of a stage: item = row * tp + pair
    const int tpd = max(tp, 1);
    const int it_dr = CO_BLOCK / tpd, it_dp = CO_BLOCK % tpd;
    __syncthreads();

    for (long long base_r = r0; base_r < rend; base_r += stage_rows) {
        double x[CO_TRIPS];
        bool have[CO_TRIPS];
#pragma unroll
        for (int t = 0; t < CO_TRIPS; ++t) {
            have[t] = active && r < rend;
            x[t] = have[t] ? v.base[s * v.step_ld + w * v.walker_ld + gcol] : 0.0;
            r += rpi;
            s += ds;
            w += dw;
            if (w >= v.W) {
                w -= v.W;
                s += 1;
            }
        }
#pragma unroll
        for (int t = 0; t < CO_TRIPS; ++t) {
            if (have[t]) {
                const int b = my.mobile ? corner_bin(my, nb, x[t]) : -1;
                sbin[(t * rpi + lr) * K + k] = (unsigned char)(b < 0 ? 255 : b);
                if (marg && b >= 0) atomicAdd(&sh1[k * nb + b], 1u);
            }
        }
        __syncthreads();
        const int nrow = int(min((long long)stage_rows, rend - base_r));
        int ir = tid / tpd, ip = tid % tpd;
        while (tp > 0 && ir < nrow) {
            const unsigned int ab = spair[ip];
            const unsigned int ba = sbin[ir * K + (ab & 255u)], bb = sbin[ir * K + (ab >> 8)];
            if (ba != 255u && bb != 255u) atomicAdd(&sh2[ip * nb2 + ba * nb + bb], 1u);
            ir += it_dr;
            ip += it_dp;
            if (ip >= tp) {
                ip -= tp;
                ir += 1;
            }
        }
        __syncthreads();
    }

    unsigned long long* g2 = h2 + size_t(p0) * nb2;
    for (int i = tid; i < tp * nb2; i += CO_BLOCK) {
        const unsigned int cnt = sh2[i];
        if (cnt) atomicAdd(&g2[i], (unsigned long long)cnt);
    }
    if (marg)
        for (int i = tid; i < K * nb; i += CO_BLOCK) {
            const unsigned int cnt = sh1[i];
            if (cnt) atomicAdd(&h1[i], (unsigned long long)cnt);
        }
}

// one workgroup per pair
__global__ __launch_bounds__(LV_BLOCK) void k_levels(const long long* __restrict__ h2, int nb, Fracs fr, int nl,
                                                     long long* __restrict__ level)
{
    __shared__ long long sc[LV_MAX];
    __shared__ long long ssum[LV_BLOCK];
    __shared__ int slast[LFG_CORNER_MAX_LEVELS];
    const int n = nb * nb, tid = threadIdx.x;
    int N = LV_BLOCK;  // a power of two >= n, and one element per lane at the least
    while (N < n) N <<= 1;
    const long long* h = h2 + size_t(blockIdx.x) * n;
    for (int i = tid; i < N; i += LV_BLOCK) sc[i] = i < n ? h[i] : -1;  // (the padding sorts behind every count)
    if (tid < LFG_CORNER_MAX_LEVELS) slast[tid] = -1;
    __syncthreads();
    for (int kk = 2; kk <= N; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += LV_BLOCK) {
                const int o = i ^ j;
                if (o > i) {
                    const long long a = sc[i], b = sc[o];
                    const bool down = (i & kk) == 0;  // descending overall
                    if ((a < b) == down) {
                        sc[i] = b;
                        sc[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    // the running sum: a lane's run of positions, then the lanes' sums
    const int ch = N / LV_BLOCK, i0 = tid * ch;
    long long mine = 0;
    for (int i = i0; i < i0 + ch; ++i)
        if (i < n) mine += sc[i];
    ssum[tid] = mine;
    __syncthreads();
    for (int off = 1; off < LV_BLOCK; off <<= 1) {
        const long long up = tid >= off ? ssum[tid - off] : 0;
        __syncthreads();
        ssum[tid] += up;
        __syncthreads();
    }
    const long long total = ssum[LV_BLOCK - 1];
    long long cum = ssum[tid] - mine;
    int last[LFG_CORNER_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < LFG_CORNER_MAX_LEVELS; ++l) last[l] = -1;
    for (int i = i0; i < i0 + ch && i < n; ++i) {
        cum += sc[i];
#pragma unroll
        for (int l = 0; l < LFG_CORNER_MAX_LEVELS; ++l)
            if (l < nl && corner_level_inside(cum, total, fr.f[l])) last[l] = i;
    }
#pragma unroll
    for (int l = 0; l < LFG_CORNER_MAX_LEVELS; ++l)
        if (last[l] >= 0) atomicMax(&slast[l], last[l]);
    __syncthreads();
    if (tid < nl) level[size_t(blockIdx.x) * nl + tid] = sc[slast[tid] >= 0 ? slast[tid] : 0];
}

size_t corner_lds_bytes() { return CO_LDS_BYTES; }

// k_corner asks for more dynamic LDS than the default limit.  Set on every
// call (a host-side table entry of the current device, no synchronisation):
// a process may drive several devices.
bool corner_lds_allowed()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_corner), hipFuncAttributeMaxDynamicSharedMemorySize,
                               CO_LDS_BYTES) == hipSuccess;
}

}  // namespace

extern "C" {

size_t lfg_corner_workspace_size(long long steps, long long W, int K, int nb)
{
    if (steps < 0 || W < 0 || K < 1 || K > LFG_CORNER_MAX_K || nb < 1 || nb > LFG_CORNER_MAX_BINS) return 0;
    return up256(size_t(K) * sizeof(CornerCol));
}

int lfg_corner_tile_rows(void) { return TILE_ROWS; }

int lfg_corner_pair_tile(int nb) { return (nb < 1 || nb > LFG_CORNER_MAX_BINS) ? 0 : pair_tile(nb); }

int lfg_corner_hist(const double* base, long long steps, long long W, int row_len, long long step_ld,
                    long long walker_ld, const int* cols, int K, const double* range, int nb, long long* h1,
                    long long* h2, int* flag, void* ws, size_t ws_bytes, void* stream)
{
    if (!corner_view_ok(steps, W, row_len, step_ld, walker_ld, cols, K, nb)) return LFG_E_ARGS;
    if (!range || !h1 || !flag || (K > 1) != (h2 != nullptr)) return LFG_E_ARGS;
    if (!ws || ws_bytes < lfg_corner_workspace_size(steps, W, K, nb)) return LFG_E_ARGS;
    const bool empty = steps == 0 || W == 0;
    if (!empty && !base) return LFG_E_ARGS;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int P = corner_pair_count(K);
    const long long n2 = (long long)P * nb * nb;
    CornerCol* col = static_cast<CornerCol*>(ws);
    const int zb = int(std::min<long long>(1024, std::max<long long>(1, ceil_div(n2 + (long long)K * nb, 256))));
    if (!empty && !corner_lds_allowed()) return LFG_E_LAUNCH;
    hipLaunchKernelGGL(k_prepare, dim3(zb), dim3(256), 0, st, range, K, nb, col, flag, h1, h2, n2);
    if (empty) return launch_ok();
    View v;
    v.base = base;
    v.steps = steps;
    v.W = W;
    v.step_ld = step_ld;
    v.walker_ld = W == 1 ? 1 : walker_ld;  // (never multiplied by anything but 0 then)
    v.rows = steps * W;
    Cols cc;
    for (int i = 0; i < LFG_CORNER_MAX_K; ++i) cc.c[i] = i < K ? cols[i] : 0;
    const int tile = pair_tile(nb);
    const int ntile = std::max(1, int(ceil_div(P, tile)));
    // about one workgroup per CU, TILE_ROWS rows each at the least, and never
    // more than 2^31 rows in one (k_corner: a bin is a uint32)
    long long blocks = std::min<long long>(ceil_div(v.rows, TILE_ROWS), std::max(1, CO_WORKGROUPS / ntile));
    blocks = std::max<long long>(blocks, ceil_div(v.rows, 1ll << 31));
    hipLaunchKernelGGL(k_corner, dim3((unsigned)blocks, ntile), dim3(CO_BLOCK), corner_lds_bytes(), st, v, cc, K, nb,
                       tile, int(blocks), col, reinterpret_cast<unsigned long long*>(h1),
                       reinterpret_cast<unsigned long long*>(h2));
    return launch_ok();
}

int lfg_corner_levels(const long long* h2, int P, int nb, const double* fracs, int nl, long long* level, void* stream)
{
    if (!h2 || !level || P < 0 || nb < 1 || nb > LFG_CORNER_MAX_BINS || !corner_fracs_ok(fracs, nl)) return LFG_E_ARGS;
    if (P == 0) return LFG_OK;
    Fracs fr;
    for (int i = 0; i < LFG_CORNER_MAX_LEVELS; ++i) fr.f[i] = i < nl ? fracs[i] : 0.0;
    hipLaunchKernelGGL(k_levels, dim3(P), dim3(LV_BLOCK), 0, static_cast<hipStream_t>(stream), h2, nb, fr, nl, level);
    return launch_ok();
}

}  // extern "C"
