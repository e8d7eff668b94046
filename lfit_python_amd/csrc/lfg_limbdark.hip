// lfg_limbdark.hip -- limb-darkening coefficients of every (logg, teff) row on
// gfx950 (include/lfg_limbdark.h; MODEL_SPEC.md section 15).  A unit of its
// own: nothing here takes part in lfg.hip's code generation.
//
// k_limbdark: one lane per row, workgroups persistent over a grid-stride loop.
//
// What is staged.  All 25 surfaces and the knots, once per workgroup: 125 KB
// on the shipped tables, so one workgroup of LD_BLOCK lanes owns a CU's LDS.
// Staging one band's five surfaces (25 KB) would let several workgroups share
// a CU, but every row would then be visited once per band and its knot
// intervals and basis values, twelve FP64 divides, recomputed five times; with
// all surfaces resident a row computes them once and its 25 contractions are
// 400 independent LDS reads, which is the instruction-level parallelism that
// the few resident waves need.  The surfaces keep the ABI's [25][nkx][nky]
// order: a lane reads sixteen values of a cell from each, rows of a chain fall
// into one or a few cells, and equal addresses broadcast; lanes in different
// cells meet bank conflicts at random, whatever the order.  Tables too large
// for the LDS (LFG_LD_MAX_KNOTS allows 25 surfaces of 60 x 60) leave their
// coefficients in global memory and stage the knots alone: the same kernel
// text, instantiated with STAGE_C = false.
//
// How a row's 200 bytes reach memory.  A lane that stored its own row would
// write 8 bytes into each of 64 different 200-byte rows per instruction.  The
// rows go through an LDS tile instead: LD_TILE rows at a time, their owners
// put the 25 values at tile[row * 25 + col] (lane stride 50 dwords: the 16
// lanes of a ds_write_b64 group fall on 16 different bank pairs), and after a
// barrier the whole workgroup copies the tile, which is a contiguous piece of
// out, with lane l at double l: 512 contiguous bytes per wave and
// instruction.  The tile is 25 KB; with the surfaces that is 151 KB of the
// CU's 160 KB, which is why a tile holds LD_TILE rows and the LD_BLOCK rows of
// a trip leave in LD_BLOCK / LD_TILE phases.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lfg_limbdark.hpp"

using namespace lfg;

namespace {

constexpr int LD_BLOCK = 512;
constexpr int LD_TILE = 128;                // rows of one store phase
constexpr int LD_MAX_BLOCKS = 256;          // one workgroup for each of the 256 CUs
constexpr int LD_LDS_BYTES = 160 * 1024;    // a CU's LDS
static_assert(LD_BLOCK % LD_TILE == 0, "a trip's rows leave in whole phases");

inline int launch_ok() { return hipGetLastError() == hipSuccess ? LFG_OK : LFG_E_LAUNCH; }

// doubles of LDS: the knots, the tile, and the surfaces when they are staged
__host__ __device__ inline int lds_doubles(int nx, int ny, bool stage_c)
{
    return nx + ny + LD_TILE * LFG_LD_NCOL + (stage_c ? LFG_LD_NCOL * (nx - 4) * (ny - 4) : 0);
}

__device__ inline void stage(double* dst, const double* __restrict__ src, int n)
{
    for (int i = threadIdx.x; i < n; i += LD_BLOCK) dst[i] = src[i];
}

template <bool STAGE_C>
__global__ __launch_bounds__(LD_BLOCK) void k_limbdark(const double* __restrict__ logg,
                                                       const double* __restrict__ teff, size_t ld, int n,
                                                       lfg_ld_tables T, double* __restrict__ out,
                                                       int* __restrict__ status)
{
    extern __shared__ double lds[];
    double* const tx = lds;
    double* const ty = tx + T.nx;
    double* const tile = ty + T.ny;
    double* const cl = tile + LD_TILE * LFG_LD_NCOL;
    stage(tx, T.tx, T.nx);
    stage(ty, T.ty, T.ny);
    if (STAGE_C) stage(cl, T.c, LFG_LD_NCOL * (T.nx - 4) * (T.ny - 4));
    __syncthreads();

    const int tid = threadIdx.x;
    const size_t N = size_t(n), stride = size_t(gridDim.x) * LD_BLOCK;
    // every lane of a workgroup takes the same trips: the barriers below are uniform
    for (size_t base = size_t(blockIdx.x) * LD_BLOCK; base < N; base += stride) {
        const size_t i = base + tid;
        const bool live = i < N;
        double o[LFG_LD_NCOL];
        if (live) {
            int st;
            if (STAGE_C) st = limbdark_row(tx, T.nx, ty, T.ny, cl, logg[i * ld], teff[i * ld], o);
            else st = limbdark_row(tx, T.nx, ty, T.ny, T.c, logg[i * ld], teff[i * ld], o);
            status[i] = st;
        }
#pragma unroll
        for (int p = 0; p < LD_BLOCK / LD_TILE; ++p) {
            if (live && tid / LD_TILE == p) {
                double* row = tile + (tid % LD_TILE) * LFG_LD_NCOL;
#pragma unroll
                for (int s = 0; s < LFG_LD_NCOL; ++s) row[s] = o[s];
            }
            __syncthreads();
            const size_t r0 = base + size_t(p) * LD_TILE;  // the tile's first row
            if (r0 < N) {
                const int count = int(std::min<size_t>(LD_TILE, N - r0)) * LFG_LD_NCOL;
                double* dst = out + r0 * LFG_LD_NCOL;
                for (int e = tid; e < count; e += LD_BLOCK) dst[e] = tile[e];
            }
            __syncthreads();
        }
    }
}

template <bool STAGE_C>
int launch(const double* logg, const double* teff, size_t ld, int n, const lfg_ld_tables& T, double* out, int* status,
           hipStream_t stream)
{
    const int blocks = int(std::min<long long>((static_cast<long long>(n) + LD_BLOCK - 1) / LD_BLOCK, LD_MAX_BLOCKS));
    const int lds_bytes = lds_doubles(T.nx, T.ny, STAGE_C) * int(sizeof(double));
    // beyond the 64 KB every kernel may ask for, the size is set on the kernel first
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_limbdark<STAGE_C>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return LFG_E_LAUNCH;
    }
    hipLaunchKernelGGL(k_limbdark<STAGE_C>, dim3(blocks), dim3(LD_BLOCK), size_t(lds_bytes), stream, logg, teff, ld, n,
                       T, out, status);
    return launch_ok();
}

}  // namespace

extern "C" {

int lfg_limbdark_lanes(void) { return LD_BLOCK * LD_MAX_BLOCKS; }

int lfg_limbdark(const double* logg, const double* teff, size_t ld, int n, const lfg_ld_tables* tab, double* out,
                 int* status, void* stream)
{
    if (n < 0 || ld < 1 || !ld_tables_ok(tab)) return LFG_E_ARGS;
    if (n == 0) return LFG_OK;
    if (!logg || !teff || !out || !status) return LFG_E_ARGS;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lds_doubles(tab->nx, tab->ny, true) * int(sizeof(double)) <= LD_LDS_BYTES)
        return launch<true>(logg, teff, ld, n, *tab, out, status, s);
    return launch<false>(logg, teff, ld, n, *tab, out, status, s);
}

}  // extern "C"
