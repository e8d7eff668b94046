// lfg_diag.hpp -- the one rule for one-unit diagnostic builds, seen by lfg.hip
// and lfg_pair_split.hip alike (through lfg_kernels.hpp: the kernels header,
// compiled a second time without machine LICM).  The diagnostic device globals are per-unit
// copies (anonymous namespace), so a kernel compiled in lfg_pair_split.hip
// would write a copy that lfg_debug_* / lfg_diag_iters, in lfg.hip, never
// read.  LFG_ONE_TU keeps every kernel in lfg.hip; it is set whenever a
// macro that declares such a global is defined.  A new one belongs here.
#ifndef LFG_DIAG_HPP
#define LFG_DIAG_HPP

#if defined(LFG_PROFILE_PAIR) || defined(LFG_PROFILE_SETUP) || defined(LFG_PROFILE_ELEM) || \
    defined(LFG_PROFILE_LIKE) || defined(LFG_PROFILE_LIKE_WAVES) || defined(LFG_COUNT_ITERS) || \
    defined(LFG_COUNT_QUIET)
#define LFG_ONE_TU 1
#endif

#endif  // LFG_DIAG_HPP
