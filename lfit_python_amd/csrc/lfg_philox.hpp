// lfg_philox.hpp -- the samplers' counter-based random numbers, shared by
// lfg.hip (stretch move: ahead of k_setup, whose speculative lanes draw
// too) and lfg_pt.hip (parallel tempering).  Included inside each unit's
// anonymous namespace, after <hip/hip_runtime.h>.
// The counter layout of every draw is documented in include/lfg.h.
#ifndef LFG_PHILOX_HPP
#define LFG_PHILOX_HPP

// Philox4x32-10 (Salmon et al. 2011), counter = (walker, step lo, step hi,
// half | purpose), key = seed.  Stateless: any rank reproduces any draw.
__device__ inline uint4 philox(uint4 c, uint2 k)
{
    for (int r = 0; r < 10; ++r) {
        const unsigned lo0 = c.x * 0xD2511F53u, hi0 = __umulhi(c.x, 0xD2511F53u);
        const unsigned lo1 = c.z * 0xCD9E8D57u, hi1 = __umulhi(c.z, 0xCD9E8D57u);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

__device__ inline double u53(unsigned a, unsigned b)  // uniform on [0, 1)
{
    return double((static_cast<unsigned long long>(a >> 5) << 26) | (b >> 6)) * (1.0 / 9007199254740992.0);
}

__device__ inline uint4 draw(unsigned long long seed, unsigned long long step, int half, int purpose, int i)
{
    return philox(make_uint4(unsigned(i), unsigned(step), unsigned(step >> 32), unsigned(half * 2 + purpose)),
                  make_uint2(unsigned(seed), unsigned(seed >> 32)));
}

#endif
