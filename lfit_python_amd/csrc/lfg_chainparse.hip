// lfg_chainparse.hip -- chain_prod.txt's numbers on gfx950 (include/lfg_chainparse.h;
// MODEL_SPEC.md section 18).  A unit of its own: nothing here takes part in
// lfg.hip's code generation.
//
// A tile is CP_TILE bytes cut at the 16-byte boundary at or below text, so
// that every tile is loaded as aligned 16-byte words (only the text's ragged
// head and tail go byte by byte) and a lane's 32 bytes are two such words in
// LDS.  A lane classifies its bytes into three 32-bit masks: newlines, field
// starts (a byte that does not separate behind one that does) and non-blanks.
//
//   k_count   the tile's field starts and newlines, its last non-blank byte
//             and the newlines before that: four int64 per tile
//   k_scan    one workgroup: the text's last non-blank byte (what lies behind
//             it is trailing blank lines), the exclusive int64 sums over the
//             tiles, rows and fields into info
//   k_check   every newline before the last non-blank byte ends a row: the
//             fields up to it must be ncol times the rows up to it
//   k_begin   info[2], [3], [5], [6] of lfg_chain_parse at their start values
//   k_parse   the tile and a halo of CP_MAX_TOKEN bytes in LDS; a lane walks
//             the tokens that start in its 32 bytes (a token that begins in
//             the tile is this tile's, wherever it ends) and stores each
//             double at out[fields before the tile + its rank in the tile]
//
// Integer arithmetic only.  The global atomics are integer adds and minima on
// info: any order gives the same values.  Nothing depends on what ws or out
// held.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lfg_chainparse.hpp"

using namespace lfg;

namespace {

constexpr int CP_BLOCK = 256;
constexpr int CP_LANE = CP_TILE / CP_BLOCK;  // bytes of one lane
constexpr int CP_HALO = 80;                  // bytes behind the tile k_parse reads: a token, its end and one more
constexpr int SC_BLOCK = 1024;
constexpr long long CP_MAX_GRID = 1 << 20;
static_assert(CP_LANE == 32, "a lane's bytes are one 32-bit mask");
static_assert(CP_HALO % 16 == 0 && CP_HALO >= CP_MAX_TOKEN + 3, "the halo holds a token, its end and the byte behind");

inline int launch_ok() { return hipGetLastError() == hipSuccess ? LFG_OK : LFG_E_LAUNCH; }

// sbuf[16 + k] = the byte x0 + k of the text for k in [-16, CP_TILE + HALO),
// '\n' outside [0, nbytes).  text + x0 is 16-byte aligned.
template <int HALO>
__device__ inline void load_tile(unsigned char* sbuf, const unsigned char* text, long long nbytes, long long x0)
{
    constexpr int NCHUNK = (16 + CP_TILE + HALO) / 16;
    for (int k = threadIdx.x; k < NCHUNK; k += CP_BLOCK) {
        const long long x = x0 - 16 + 16ll * k;
        if (x >= 0 && x + 16 <= nbytes) {
            *reinterpret_cast<uint4*>(sbuf + 16 * k) = *reinterpret_cast<const uint4*>(text + x);
        } else {
            for (int j = 0; j < 16; ++j) {
                const long long y = x + j;
                sbuf[16 * k + j] = (y >= 0 && y < nbytes) ? text[y] : (unsigned char)'\n';
            }
        }
    }
}

struct Masks {
    unsigned int nl, start, nonblank;
};

// the masks of lane tid's 32 bytes (sbuf as load_tile left it); bytes outside
// the text are '\n' there and count as nothing
__device__ inline Masks classify(const unsigned char* sbuf, int tid, long long x0, long long nbytes)
{
    const unsigned char* p = sbuf + 16 + CP_LANE * tid;
    const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 16);
    const unsigned int wd[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const long long xl = x0 + CP_LANE * tid;  // the lane's first byte
    const int lo = int(min(max(-xl, 0ll), (long long)CP_LANE)), hi = int(min(max(nbytes - xl, 0ll), (long long)CP_LANE));
    const unsigned int valid = (hi > lo) ? ((hi == 32 ? 0xffffffffu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u)) : 0u;
    Masks m;
    m.nl = m.start = m.nonblank = 0;
    int c = wd[0] & 0xff;
    bool psep = cp_sep(p[-1], c);
#pragma unroll
    for (int i = 0; i < CP_LANE; ++i) {
        const int next = i + 1 < CP_LANE ? int((wd[(i + 1) >> 2] >> (8 * ((i + 1) & 3))) & 0xff) : int(p[CP_LANE]);
        const bool sep = cp_sep(c, next);
        m.nl |= (c == '\n' ? 1u : 0u) << i;
        m.start |= ((!sep && psep) ? 1u : 0u) << i;
        m.nonblank |= (sep ? 0u : 1u) << i;
        psep = sep;
        c = next;
    }
    m.nl &= valid;  // (start and nonblank are never set outside the text: its filler separates)
    return m;
}

__device__ inline unsigned int below(int i) { return i >= 32 ? 0xffffffffu : ((1u << i) - 1u); }

struct ParseArgs {
    const unsigned char* text;
    long long nbytes, ntiles;
    int pad0, ncol;
};

__global__ __launch_bounds__(CP_BLOCK) void k_count(ParseArgs a, CpWs w)
{
    __shared__ __attribute__((aligned(16))) unsigned char sbuf[16 + CP_TILE + 16];
    __shared__ unsigned int sf, sl, sla;
    __shared__ int snb;
    const int tid = threadIdx.x;
    for (long long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const long long x0 = t * CP_TILE - a.pad0;
        if (tid == 0) sf = 0, sl = 0, sla = 0, snb = -1;
        load_tile<16>(sbuf, a.text, a.nbytes, x0);
        __syncthreads();
        const Masks m = classify(sbuf, tid, x0, a.nbytes);
        if (m.start) atomicAdd(&sf, (unsigned int)__popc(m.start));  // (LDS, integer: any order gives the same)
        if (m.nl) atomicAdd(&sl, (unsigned int)__popc(m.nl));
        if (m.nonblank) atomicMax(&snb, CP_LANE * tid + 31 - __clz(m.nonblank));
        __syncthreads();
        const int nb = snb;  // the tile's last non-blank byte: the newlines before it
        if (m.nl && nb >= 0) {
            const int k = nb - CP_LANE * tid;
            const unsigned int before = m.nl & (k <= 0 ? 0u : below(min(k, 32)));
            if (before) atomicAdd(&sla, (unsigned int)__popc(before));
        }
        __syncthreads();
        if (tid == 0) {
            w.tf[t] = sf;
            w.tl[t] = sl;
            w.tla[t] = sla;
            w.tnb[t] = nb >= 0 ? x0 + nb : -1;
        }
        __syncthreads();
    }
}

// one workgroup: glob[0], of and ol, and info
__global__ __launch_bounds__(SC_BLOCK) void k_scan(CpWs w, long long ntiles, int ncol, long long* __restrict__ info)
{
    __shared__ long long s[SC_BLOCK], s2[SC_BLOCK];
    __shared__ long long srows;
    const int tid = threadIdx.x;
    long long last = -1;
    for (long long i = tid; i < ntiles; i += SC_BLOCK) last = max(last, w.tnb[i]);
    s[tid] = last;
    if (tid == 0) srows = 0;
    __syncthreads();
    for (int off = SC_BLOCK / 2; off > 0; off >>= 1) {
        if (tid < off) s[tid] = max(s[tid], s[tid + off]);
        __syncthreads();
    }
    last = s[0];
    __syncthreads();
    long long cf = 0, cl = 0;
    for (long long b = 0; b < ntiles; b += SC_BLOCK) {
        const long long i = b + tid;
        const long long vf = i < ntiles ? w.tf[i] : 0, vl = i < ntiles ? w.tl[i] : 0;
        s[tid] = vf;
        s2[tid] = vl;
        __syncthreads();
        for (int off = 1; off < SC_BLOCK; off <<= 1) {
            const long long uf = tid >= off ? s[tid - off] : 0, ul = tid >= off ? s2[tid - off] : 0;
            __syncthreads();
            s[tid] += uf;
            s2[tid] += ul;
            __syncthreads();
        }
        if (i < ntiles) {
            const long long of = cf + s[tid] - vf, ol = cl + s2[tid] - vl;
            w.of[i] = of;
            w.ol[i] = ol;
            if (last >= 0 && w.tnb[i] == last) srows = ol + w.tla[i] + 1;  // (one tile holds that byte)
        }
        cf += s[SC_BLOCK - 1];
        cl += s2[SC_BLOCK - 1];
        __syncthreads();
    }
    if (tid == 0) {
        const long long rows = srows, fields = cf;
        const bool off = fields != rows * ncol;  // the last row's end, which no newline before `last` marks
        w.glob[0] = last;
        info[0] = rows;
        info[1] = fields;
        info[2] = 0;
        info[3] = 0;
        info[4] = off ? 1 : 0;
        info[5] = off ? rows - 1 : -1;
        info[6] = 0;
        info[7] = 0;
    }
}

// the LDS scan the two kernels below share: the exclusive prefix of v over the lanes
__device__ inline unsigned int scan_lanes(unsigned int* sp, unsigned int v)
{
    const int tid = threadIdx.x;
    sp[tid] = v;
    __syncthreads();
    for (int off = 1; off < CP_BLOCK; off <<= 1) {
        const unsigned int up = tid >= off ? sp[tid - off] : 0;
        __syncthreads();
        sp[tid] += up;
        __syncthreads();
    }
    const unsigned int r = sp[tid] - v;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(CP_BLOCK) void k_check(ParseArgs a, CpWs w, long long* __restrict__ info)
{
    __shared__ __attribute__((aligned(16))) unsigned char sbuf[16 + CP_TILE + 16];
    __shared__ unsigned int sp[CP_BLOCK];
    const int tid = threadIdx.x;
    const long long last = w.glob[0];
    for (long long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const long long x0 = t * CP_TILE - a.pad0;
        if (x0 >= last) break;  // (tiles only grow: nothing to check from here on)
        load_tile<16>(sbuf, a.text, a.nbytes, x0);
        __syncthreads();
        const Masks m = classify(sbuf, tid, x0, a.nbytes);
        const unsigned int pf = scan_lanes(sp, (unsigned int)__popc(m.start));
        const unsigned int pl = scan_lanes(sp, (unsigned int)__popc(m.nl));
        const long long F0 = w.of[t] + pf, L0 = w.ol[t] + pl, xl = x0 + CP_LANE * tid;
        long long bad = 0, row = -1;
        for (unsigned int rest = m.nl; rest; rest &= rest - 1) {
            const int i = __ffs(rest) - 1;
            if (xl + i >= last) break;
            const long long F = F0 + __popc(m.start & below(i)), L = L0 + __popc(m.nl & below(i));
            if (F != a.ncol * (L + 1)) {
                if (!bad) row = L;
                ++bad;
            }
        }
        if (bad) {
            atomicAdd(reinterpret_cast<unsigned long long*>(info + 4), (unsigned long long)bad);
            atomicMin(reinterpret_cast<unsigned long long*>(info + 5), (unsigned long long)row);  // (-1 is the largest)
        }
        __syncthreads();
    }
}

__global__ void k_begin(long long* __restrict__ info, long long out_rows)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        info[2] = 0;
        info[3] = 0;
        if (info[4] == 0) info[5] = -1;
        info[6] = (info[4] == 0 && info[0] > out_rows) ? 1 : 0;
    }
}

struct LdsGet {
    const unsigned char* p;
    __device__ int operator()(int j) const { return j <= CP_MAX_TOKEN + 2 ? int(p[j]) : -1; }
};

__global__ __launch_bounds__(CP_BLOCK) void k_parse(ParseArgs a, CpWs w, double* __restrict__ out, long long out_rows,
                                                    long long* __restrict__ info)
{
    __shared__ __attribute__((aligned(16))) unsigned char sbuf[16 + CP_TILE + CP_HALO];
    __shared__ unsigned int sp[CP_BLOCK];
    const int tid = threadIdx.x;
    // (k_begin wrote the other entries; these two are lfg_chain_parse_count's)
    if (info[4] != 0 || info[0] > out_rows) return;
    const long long cap = min(out_rows * a.ncol, info[1]);
    unsigned long long* outb = reinterpret_cast<unsigned long long*>(out);
    for (long long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const long long x0 = t * CP_TILE - a.pad0;
        load_tile<CP_HALO>(sbuf, a.text, a.nbytes, x0);
        __syncthreads();
        const Masks m = classify(sbuf, tid, x0, a.nbytes);
        long long rank = w.of[t] + scan_lanes(sp, (unsigned int)__popc(m.start));
        long long bad = 0, refused = 0, row = -1;
        for (unsigned int rest = m.start; rest; rest &= rest - 1, ++rank) {
            const int i = __ffs(rest) - 1;
            const CpVal v = cp_token<true>(LdsGet{sbuf + 16 + CP_LANE * tid + i});
            if (v.status == CP_BAD) {
                if (!bad) row = rank / a.ncol;
                ++bad;
            }
            refused += v.status == CP_REFUSED ? 1 : 0;
            if (rank < cap) outb[rank] = v.bits;
        }
        if (bad) {
            atomicAdd(reinterpret_cast<unsigned long long*>(info + 2), (unsigned long long)bad);
            atomicMin(reinterpret_cast<unsigned long long*>(info + 5), (unsigned long long)row);
        }
        if (refused) atomicAdd(reinterpret_cast<unsigned long long*>(info + 3), (unsigned long long)refused);
        __syncthreads();
    }
}

bool args_ok(const unsigned char* text, long long nbytes, int ncol, const long long* info, const void* ws,
             size_t ws_bytes)
{
    const size_t need = cp_ws_bytes(nbytes);
    return need != 0 && info && ws && ws_bytes >= need && (text || nbytes == 0) && ncol >= 1 &&
           ncol <= LFG_CHAIN_PARSE_MAX_NCOL;
}

ParseArgs make_args(const unsigned char* text, long long nbytes, int ncol)
{
    ParseArgs a;
    a.text = text;
    a.nbytes = nbytes;
    a.pad0 = nbytes ? int(reinterpret_cast<uintptr_t>(text) & 15) : 0;
    a.ntiles = cp_ntiles(nbytes, a.pad0);
    a.ncol = ncol;
    return a;
}

}  // namespace

extern "C" {

int lfg_chain_parse_tile_bytes(void) { return CP_TILE; }

size_t lfg_chain_parse_workspace_size(long long nbytes) { return cp_ws_bytes(nbytes); }

int lfg_chain_parse_count(const unsigned char* text, long long nbytes, int ncol, long long* info, void* ws,
                          size_t ws_bytes, void* stream)
{
    if (!args_ok(text, nbytes, ncol, info, ws, ws_bytes)) return LFG_E_ARGS;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ParseArgs a = make_args(text, nbytes, ncol);
    const CpWs w = cp_ws(ws, nbytes);
    const unsigned grid = unsigned(std::min(a.ntiles, CP_MAX_GRID));
    if (a.ntiles) hipLaunchKernelGGL(k_count, dim3(grid), dim3(CP_BLOCK), 0, st, a, w);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(SC_BLOCK), 0, st, w, a.ntiles, ncol, info);
    if (a.ntiles) hipLaunchKernelGGL(k_check, dim3(grid), dim3(CP_BLOCK), 0, st, a, w, info);
    return launch_ok();
}

int lfg_chain_parse(const unsigned char* text, long long nbytes, int ncol, double* out, long long out_rows,
                    long long* info, void* ws, size_t ws_bytes, void* stream)
{
    if (!args_ok(text, nbytes, ncol, info, ws, ws_bytes) || out_rows < 0 || (!out && out_rows > 0)) return LFG_E_ARGS;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ParseArgs a = make_args(text, nbytes, ncol);
    const CpWs w = cp_ws(ws, nbytes);
    const unsigned grid = unsigned(std::min(a.ntiles, CP_MAX_GRID));
    hipLaunchKernelGGL(k_begin, dim3(1), dim3(1), 0, st, info, out_rows);
    if (a.ntiles && out_rows > 0)
        hipLaunchKernelGGL(k_parse, dim3(grid), dim3(CP_BLOCK), 0, st, a, w, out, out_rows, info);
    return launch_ok();
}

}  // extern "C"
