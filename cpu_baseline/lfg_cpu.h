/*
 * lfg_cpu.h -- the CPU port of the GPU path (cpu_baseline/lfg_cpu.cpp):
 * lfg_device.hpp's setup, stream table and envelope-Newton element solver
 * compiled for the host, mirror symmetry and the interval sweep, OpenMP over
 * parameter sets / walkers.  It is bench.py's CPU baseline and the host twin
 * (lfg_cpu_*) of include/lfg.h's entry points: same argument meaning and
 * status codes, HOST pointers, no workspace or stream; nthreads <= 0: every
 * OpenMP thread.  Not a product path: lfit_python_amd never loads it.
 */
#ifndef LFG_CPU_H
#define LFG_CPU_H

#include "lfg.h"
#include "lfg_physpar.h"
#include "lfg_wd.h"
#include "lfg_chain.h"
#include "lfg_limbdark.h"
#include "lfg_corner.h"
#include "lfg_chaintext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lfg_flux's twin (lfit.CV.calcFlux, CVModel.py:132-147): flux [W][N] */
int lfg_cpu_flux(const double* pars, int W, int P, const double* x,
                 const double* w, int N, int nsub, double* flux, int* status,
                 int nthreads);

/* lfg_lnlike's twin (SimpleEclipse.chisq / ln_like, CVModel.py:157-191) */
int lfg_cpu_lnlike(const double* pars, int W, int P, const double* x,
                   const double* w, int N, int nsub, const double* y,
                   const double* ye, double* lnlike, int* status,
                   int nthreads);

/* lfg_lnprob's twin (mcmcfit.ln_prob -> Node.ln_prob) over a tree whose
 * arrays are host pointers; chi^2 or GP trees */
int lfg_cpu_lnprob(const double* walkers, int W, const lfg_tree* tree,
                   double* lnp, int nthreads);

/* lfg_gp_predict's twin (gp.predict over a merged grid, MODEL_SPEC 10.5):
 * mean, var [W][n] (var NULL: mean only), status [W]; any nb */
int lfg_cpu_gp_predict(const double* x, const double* ye, const int* obs,
                       const double* res, int W, int n, const double* hyp,
                       const double* blocks, int nb, double* mean, double* var,
                       int* status, int nthreads);

/* lfg_physpar's twin (include/lfg_physpar.h; calcPhysicalParams.py solve()):
 * the same arguments on host pointers, the tables' arrays included */
int lfg_cpu_physpar(const double* q, const double* dphi, const double* rwd,
                    size_t ld, const double* twd, const double* p, int n,
                    const lfg_mr_tables* tab, double* out, int* model,
                    int* status, int nthreads);

/* lfg_wd_lnprob's twin (include/lfg_wd.h; wdparams_new.py ln_prob): the same
 * arguments on host pointers, the model's arrays included */
int lfg_cpu_wd_lnprob(const double* theta, size_t ld, int n,
                      const lfg_wd_model* model, double* lnp, double* lnlike,
                      double* mags, int* status, int nthreads);

/* lfg_chain_stats' and lfg_chain_clip's twins (include/lfg_chain.h;
 * MODEL_SPEC 14): the same arguments on host pointers, no scratch */
int lfg_cpu_chain_stats(const double* base, long long steps, long long W, int C,
                        long long step_ld, long long walker_ld,
                        const double* window, const double* fracs, int nq,
                        long long* n, long long* n_bad, double* mean, double* m2,
                        double* vmin, double* vmax, double* ostat, double* quant,
                        double* rhat);
int lfg_cpu_chain_clip(const long long* n, const double* m2, const double* med,
                       long long med_ld, double sigma, const double* win_in,
                       double* win_out, int C);

/* lfg_limbdark's twin (include/lfg_limbdark.h; limbdark.py ld()): the same
 * arguments on host pointers, the tables' arrays included */
int lfg_cpu_limbdark(const double* logg, const double* teff, size_t ld, int n,
                     const lfg_ld_tables* tab, double* out, int* status,
                     int nthreads);

/* lfg_corner_hist's and lfg_corner_levels' twins (include/lfg_corner.h;
 * MODEL_SPEC 16): the same arguments on host pointers, range included, no
 * scratch */
int lfg_cpu_corner_hist(const double* base, long long steps, long long W,
                        int row_len, long long step_ld, long long walker_ld,
                        const int* cols, int K, const double* range, int nb,
                        long long* h1, long long* h2, int* flag);
int lfg_cpu_corner_levels(const long long* h2, int P, int nb,
                          const double* fracs, int nl, long long* level);

/* lfg_chain_text's twin (include/lfg_chaintext.h; MODEL_SPEC 17): the same
 * arguments on host pointers, no scratch.  Exact for every double: a finite
 * |lnp| >= 2^63 goes through snprintf("%f"), so nbytes[1] is always 0 */
int lfg_cpu_chain_text(const double* base, long long steps, long long W,
                       int ndim, long long step_ld, long long walker_ld,
                       const double* lnp, long long lnp_step_ld,
                       long long lnp_walker_ld, long long walker0,
                       unsigned char* out, size_t out_bytes, long long* nbytes,
                       int nthreads);
/* lfg_chain_text_bound's twin.  The bound leaves out what the device refuses:
 * a caller adds 320 bytes per finite |lnp| >= 2^63 */
long long lfg_cpu_chain_text_bound(long long steps, long long W, int ndim,
                                   long long walker0);

/* lfg_chain_parse_count's and lfg_chain_parse's twins (include/lfg_chainparse.h,
 * MODEL_SPEC.md section 18): the same arguments without the stream, every
 * pointer a host pointer.  The twin refuses no token (info[3] stays 0): what
 * the shared rules leave undecided is finished by strtod in the C locale. */
int lfg_cpu_chain_parse_tile_bytes(void);
size_t lfg_cpu_chain_parse_workspace_size(long long nbytes);
int lfg_cpu_chain_parse_count(const unsigned char* text, long long nbytes,
                              int ncol, long long* info, void* ws,
                              size_t ws_bytes);
int lfg_cpu_chain_parse(const unsigned char* text, long long nbytes, int ncol,
                        double* out, long long out_rows, long long* info,
                        void* ws, size_t ws_bytes);

/* the batch form bench.py times (the oracle's lfo_lnprob_batch arguments);
 * returns the OpenMP threads used */
int lfc_lnprob_batch(const double* walkers, int W, int ndim, int E,
                     const int* gather, const int* npars, const double* consts,
                     const int* off, const double* x, const double* y,
                     const double* ye, const double* w, int nsub,
                     const int* prior_type, const double* prior_p1,
                     const double* prior_p2, const double* prior_norm,
                     int roche_priors, double* lnp, int nthreads);
int lfc_lnprob_batch_gp(const double* walkers, int W, int ndim, int E,
                        const int* gather, const int* npars,
                        const double* consts, const int* off, const double* x,
                        const double* y, const double* ye, const double* w,
                        int nsub, const int* prior_type,
                        const double* prior_p1, const double* prior_p2,
                        const double* prior_norm, int roche_priors,
                        const int* gp_gather, const double* gp_base,
                        const int* gp_ecl, double* lnp, int nthreads);

#ifdef __cplusplus
}
#endif
#endif
