// lfg_chaintext.hip -- chain_prod.txt's rows on gfx950 (include/lfg_chaintext.h;
// MODEL_SPEC.md section 17).  A unit of its own: nothing here takes part in
// lfg.hip's code generation.
//
//   k_text<false>  the length pass.  A workgroup takes a tile of whole rows,
//                  at most CT_TILE_ELEMS numbers: a lane forms the decimal
//                  digits of CT_EPT of them (neighbouring lanes take
//                  neighbouring numbers of a row) and their lengths, the
//                  workgroup sums them: one int64 per tile, and the tile's
//                  refused rows.
//   k_scan         one workgroup: the exclusive int64 scan over the tiles,
//                  the total and the refused rows into nbytes.
//   k_text<true>   the emit pass.  The digits again (cheaper than 16 bytes of
//                  scratch per number written and read back), a scan of the
//                  tile's lengths in LDS, then every lane writes its numbers'
//                  characters into the tile's byte range in LDS.  The range
//                  is laid out at the same offset modulo 16 as its place in
//                  `out`, so the workgroup stores it as aligned 16-byte words;
//                  only the ragged head and tail go byte by byte.
//
// Integer arithmetic only; no atomics on global memory; nothing depends on
// what ws or out held.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lfg_chaintext.hpp"

using namespace lfg;

namespace {

constexpr int CT_BLOCK = 256;
constexpr int CT_EPT = 4;                          // numbers of one lane
constexpr int CT_TILE_ELEMS = CT_BLOCK * CT_EPT;   // numbers of one tile at the most
constexpr int CT_MAX_TILE_ROWS = 256;
// the tile's bytes at the most, and the 16 of the alignment offset
constexpr int CT_OUT_LDS = CT_MAX_TILE_ROWS * (CT_WALKER_MAX + 2 + CT_FIXED_MAX) + CT_TILE_ELEMS * (1 + CT_REPR_MAX) + 16;
static_assert(CT_OUT_LDS % 16 == 0 && CT_OUT_LDS + CT_TILE_ELEMS * 4 + CT_BLOCK * 4 <= 64 * 1024, "k_text's LDS");
static_assert(LFG_CHAIN_TEXT_MAX_NDIM + 1 <= CT_TILE_ELEMS, "a row must fit a tile");
constexpr int SC_BLOCK = 1024;
constexpr long long CT_MAX_GRID = 1 << 20;

inline int launch_ok() { return hipGetLastError() == hipSuccess ? LFG_OK : LFG_E_LAUNCH; }
inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }
inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }
inline int tile_rows(int ndim) { return std::min(CT_MAX_TILE_ROWS, CT_TILE_ELEMS / (ndim + 1)); }

struct TextArgs {
    const double* base;
    const double* lnp;
    long long W, step_ld, walker_ld, lnp_step_ld, lnp_walker_ld, walker0, rows, ntiles;
    int ndim, tile_rows;
};

struct LdsPut {
    unsigned char* p;
    __device__ void operator()(int pos, char ch) const { p[pos] = (unsigned char)ch; }
};

template <bool EMIT>
__global__ __launch_bounds__(CT_BLOCK) void k_text(TextArgs a, long long* __restrict__ tilesum,
                                                   long long* __restrict__ tileref,
                                                   const long long* __restrict__ tileoff,
                                                   unsigned char* __restrict__ out)
{
    __shared__ unsigned int slen[CT_TILE_ELEMS];  // the numbers' lengths, then their offsets in the tile
    __shared__ unsigned int spart[CT_BLOCK];
    __shared__ unsigned int sref;
    __shared__ __attribute__((aligned(16))) unsigned char sout[EMIT ? CT_OUT_LDS : 16];
    const int tid = threadIdx.x;
    const int C1 = a.ndim + 1;
    for (long long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const long long r0 = t * a.tile_rows;
        const int nrows = int(min((long long)a.tile_rows, a.rows - r0));
        const int ne = nrows * C1;
        CtDec d[CT_EPT];
        long long wk[CT_EPT];
        int wl[CT_EPT];
        bool last[CT_EPT];
        unsigned int nref = 0;
        if (tid == 0) sref = 0;
#pragma unroll
        for (int i = 0; i < CT_EPT; ++i) {
            const int e = i * CT_BLOCK + tid;
            unsigned int len = 0;
            wl[i] = 0;
            wk[i] = 0;
            last[i] = false;
            d[i].kind = CT_ZERO, d[i].neg = 0, d[i].nd = 0, d[i].sig = 0, d[i].pt = 0;
            if (e < ne) {
                const int rl = e / C1, c = e - rl * C1;
                const long long r = r0 + rl;
                const long long s = r / a.W, w = r - s * a.W;
                if (c < a.ndim) {
                    d[i] = ct_repr(a.base[s * a.step_ld + w * a.walker_ld + c]);
                    len = 1;
                } else {
                    d[i] = ct_fixed6(a.lnp[s * a.lnp_step_ld + w * a.lnp_walker_ld]);
                    nref += d[i].kind == CT_REFUSED ? 1 : 0;
                    last[i] = true;
                    len = 2;  // (the space before and the newline behind)
                }
                if (c == 0) {
                    wk[i] = a.walker0 + w;
                    wl[i] = ct_walker_len(wk[i]);
                }
                len += ct_len(d[i]) + wl[i];
            }
            slen[e] = len;
        }
        __syncthreads();
        // the exclusive scan: a lane's run of CT_EPT lengths, then the lanes' sums
        unsigned int v[CT_EPT], mine = 0;
#pragma unroll
        for (int j = 0; j < CT_EPT; ++j) {
            v[j] = slen[tid * CT_EPT + j];
            mine += v[j];
        }
        spart[tid] = mine;
        __syncthreads();
        for (int off = 1; off < CT_BLOCK; off <<= 1) {
            const unsigned int up = tid >= off ? spart[tid - off] : 0;
            __syncthreads();
            spart[tid] += up;
            __syncthreads();
        }
        const unsigned int total = spart[CT_BLOCK - 1];
        if (!EMIT) {
            if (nref) atomicAdd(&sref, nref);  // (LDS, integer: any order gives the same count)
            __syncthreads();
            if (tid == 0) {
                tilesum[t] = total;
                tileref[t] = sref;
            }
            __syncthreads();
            continue;
        }
        unsigned int run = spart[tid] - mine;
#pragma unroll
        for (int j = 0; j < CT_EPT; ++j) {
            slen[tid * CT_EPT + j] = run;
            run += v[j];
        }
        __syncthreads();
        const long long g0 = tileoff[t];
        const unsigned int pad = (unsigned int)((reinterpret_cast<uintptr_t>(out) + (unsigned long long)g0) & 15);
#pragma unroll
        for (int i = 0; i < CT_EPT; ++i) {
            const int e = i * CT_BLOCK + tid;
            if (e < ne) {
                unsigned char* p = sout + pad + slen[e];
                if (wl[i]) {
                    ct_emit_walker(wk[i], wl[i], LdsPut{p});
                    p += wl[i];
                }
                p[0] = ' ';
                ct_emit(d[i], LdsPut{p + 1});
                if (last[i]) p[1 + ct_len(d[i])] = '\n';
            }
        }
        __syncthreads();
        // sout[pad .. pad + total) goes to out[g0 ..): chunk k of sout and of
        // ga are both 16-byte aligned
        unsigned char* ga = out + g0 - pad;
        const unsigned int end = pad + total;
        const int nchunk = int((end + 15) / 16);
        for (int k = tid; k < nchunk; k += CT_BLOCK) {
            const unsigned int lo = k * 16u, hi = lo + 16u;
            if (lo >= pad && hi <= end) {
                *reinterpret_cast<uint4*>(ga + lo) = *reinterpret_cast<const uint4*>(sout + lo);
            } else {
                for (unsigned int j = max(lo, pad); j < min(hi, end); ++j) ga[j] = sout[j];
            }
        }
        __syncthreads();
    }
}

// one workgroup: tileoff = the exclusive scan of tilesum, nbytes = {the
// total, the refused rows}
__global__ __launch_bounds__(SC_BLOCK) void k_scan(const long long* __restrict__ tilesum,
                                                   const long long* __restrict__ tileref,
                                                   long long* __restrict__ tileoff, long long ntiles,
                                                   long long* __restrict__ nbytes)
{
    __shared__ long long s[SC_BLOCK];
    const int tid = threadIdx.x;
    long long carry = 0, ref = 0;
    for (long long b = 0; b < ntiles; b += SC_BLOCK) {
        const long long i = b + tid;
        const long long v = i < ntiles ? tilesum[i] : 0;
        ref += i < ntiles ? tileref[i] : 0;
        s[tid] = v;
        __syncthreads();
        for (int off = 1; off < SC_BLOCK; off <<= 1) {
            const long long up = tid >= off ? s[tid - off] : 0;
            __syncthreads();
            s[tid] += up;
            __syncthreads();
        }
        if (i < ntiles) tileoff[i] = carry + s[tid] - v;
        carry += s[SC_BLOCK - 1];
        __syncthreads();
    }
    s[tid] = ref;
    __syncthreads();
    for (int off = SC_BLOCK / 2; off > 0; off >>= 1) {
        if (tid < off) s[tid] += s[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        nbytes[0] = carry;
        nbytes[1] = s[0];
    }
}

}  // namespace

extern "C" {

long long lfg_chain_text_bound(long long steps, long long W, int ndim, long long walker0)
{
    return ct_bound(steps, W, ndim, walker0);
}

int lfg_chain_text_tile_rows(int ndim) { return (ndim < 1 || ndim > LFG_CHAIN_TEXT_MAX_NDIM) ? 0 : tile_rows(ndim); }

size_t lfg_chain_text_workspace_size(long long steps, long long W, int ndim)
{
    if (ct_bound(steps, W, ndim, 0) < 0) return 0;
    const long long ntiles = ceil_div(steps * W, tile_rows(ndim));
    return up256(size_t(std::max<long long>(ntiles, 1)) * 3 * sizeof(long long));
}

int lfg_chain_text(const double* base, long long steps, long long W, int ndim, long long step_ld,
                   long long walker_ld, const double* lnp, long long lnp_step_ld, long long lnp_walker_ld,
                   long long walker0, unsigned char* out, size_t out_bytes, long long* nbytes, void* ws,
                   size_t ws_bytes, void* stream)
{
    const long long bound = ct_bound(steps, W, ndim, walker0);
    if (bound < 0 || step_ld < 1 || walker_ld < 1 || lnp_step_ld < 1 || lnp_walker_ld < 1 || !nbytes) return LFG_E_ARGS;
    if (!ws || ws_bytes < lfg_chain_text_workspace_size(steps, W, ndim)) return LFG_E_ARGS;
    if ((unsigned long long)out_bytes < (unsigned long long)bound) return LFG_E_ARGS;
    const bool empty = steps == 0 || W == 0;
    if (!empty && (!base || !lnp || !out)) return LFG_E_ARGS;
    hipStream_t st = static_cast<hipStream_t>(stream);
    TextArgs a;
    a.base = base;
    a.lnp = lnp;
    a.W = std::max<long long>(W, 1);
    a.step_ld = step_ld;
    a.walker_ld = walker_ld;
    a.lnp_step_ld = lnp_step_ld;
    a.lnp_walker_ld = lnp_walker_ld;
    a.walker0 = walker0;
    a.rows = steps * W;
    a.ndim = ndim;
    a.tile_rows = tile_rows(ndim);
    a.ntiles = ceil_div(a.rows, a.tile_rows);
    long long* tilesum = static_cast<long long*>(ws);
    long long* tileref = tilesum + a.ntiles;
    long long* tileoff = tileref + a.ntiles;
    const unsigned grid = unsigned(std::min(a.ntiles, CT_MAX_GRID));
    if (!empty) hipLaunchKernelGGL(k_text<false>, dim3(grid), dim3(CT_BLOCK), 0, st, a, tilesum, tileref, tileoff, out);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(SC_BLOCK), 0, st, tilesum, tileref, tileoff, a.ntiles, nbytes);
    if (!empty) hipLaunchKernelGGL(k_text<true>, dim3(grid), dim3(CT_BLOCK), 0, st, a, tilesum, tileref, tileoff, out);
    return launch_ok();
}

}  // extern "C"
