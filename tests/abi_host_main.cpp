// Host program of tests/test_abi_host.py: the lfg_cpu_* twins of
// cpu_baseline/lfg_cpu.cpp (lfg_device.hpp and lfg_tables.hpp compiled for
// the host through cpu_baseline/shim) on cases read from a file, every buffer
// allocated from the heap at exactly its size, so that a host sanitizer sees
// any read or write outside what include/lfg.h and lfg_cpu.h promise.
//
//   abi_host <cases> <results> [swap]
//
// <cases> is a stream of 32-bit ints and doubles (host byte order):
//   int ncases, then per case: int kind, int nthreads, and
//   kind 0 lfg_cpu_flux:    W P N nsub has_w | pars[W P] x[N] (w[N])
//   kind 1 lfg_cpu_lnlike:  W P N nsub has_w | pars x (w) y[N] ye[N]
//   kind 2 lfg_cpu_lnprob:  E ndim nsub max_n roche gp fixed_invalid nconst ntot W |
//                           gather[E 18] npars[E] off[E + 1] prior_type[ndim] (gp_gather[E 3] gp_ecl[E 2]) |
//                           consts[nconst] x y ye w [ntot each] prior_p1 p2 norm [ndim each] (gp_base[E 4])
//                           walkers[W ndim]
//   kind 3 lfg_cpu_gp_predict: W n nb has_var | obs[n] | x[n] ye[n] res[W n] hyp[W 3] blocks[W nb 2]
// <results> receives per case: int rc, then the outputs in the header's order
// (flux, status | lnlike, status | lnp | mean, (var), status).
// swap: run a case given nthreads = 1 with 4 threads and the others with 1.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "lfg_cpu.h"

namespace {

FILE* fin;
FILE* fout;

void die(const char* what)
{
    std::fprintf(stderr, "abi_host: %s\n", what);
    std::exit(2);
}

int geti()
{
    int v;
    if (std::fread(&v, sizeof v, 1, fin) != 1) die("short read (int)");
    return v;
}

// exactly n elements from the heap (n = 0: a valid pointer to nothing)
template <class T>
std::unique_ptr<T[]> alloc(size_t n)
{
    return std::unique_ptr<T[]>(new T[n]);
}

template <class T>
std::unique_ptr<T[]> get(size_t n)
{
    auto p = alloc<T>(n);
    if (n && std::fread(p.get(), sizeof(T), n, fin) != n) die("short read (array)");
    return p;
}

template <class T>
void put(const T* p, size_t n)
{
    if (n && std::fwrite(p, sizeof(T), n, fout) != n) die("short write");
}

void flux_case(int kind, int nthreads)
{
    const int W = geti(), P = geti(), N = geti(), nsub = geti(), has_w = geti();
    auto pars = get<double>(size_t(W) * P);
    auto x = get<double>(N);
    auto w = has_w ? get<double>(N) : nullptr;
    auto status = alloc<int>(W);
    if (kind == 0) {
        auto flux = alloc<double>(size_t(W) * N);
        const int rc = lfg_cpu_flux(pars.get(), W, P, x.get(), w.get(), N, nsub, flux.get(), status.get(), nthreads);
        put(&rc, 1);
        put(flux.get(), size_t(W) * N);
    } else {
        auto y = get<double>(N);
        auto ye = get<double>(N);
        auto ll = alloc<double>(W);
        const int rc = lfg_cpu_lnlike(pars.get(), W, P, x.get(), w.get(), N, nsub, y.get(), ye.get(), ll.get(),
                                      status.get(), nthreads);
        put(&rc, 1);
        put(ll.get(), W);
    }
    put(status.get(), W);
}

void lnprob_case(int nthreads)
{
    lfg_tree T{};
    T.E = geti();
    T.ndim = geti();
    T.nsub = geti();
    T.max_n = geti();
    T.roche_priors = geti();
    T.gp = geti();
    T.fixed_invalid = geti();
    const int nconst = geti(), ntot = geti(), W = geti();
    auto gather = get<int>(size_t(T.E) * 18);
    auto npars = get<int>(T.E);
    auto off = get<int>(T.E + 1);
    auto ptype = get<int>(T.ndim);
    auto gpg = T.gp ? get<int>(size_t(T.E) * 3) : nullptr;
    auto gpe = T.gp ? get<int>(size_t(T.E) * 2) : nullptr;
    auto consts = get<double>(nconst);
    auto x = get<double>(ntot);
    auto y = get<double>(ntot);
    auto ye = get<double>(ntot);
    auto w = get<double>(ntot);
    auto p1 = get<double>(T.ndim);
    auto p2 = get<double>(T.ndim);
    auto pn = get<double>(T.ndim);
    auto gpb = T.gp ? get<double>(size_t(T.E) * 4) : nullptr;
    auto walkers = get<double>(size_t(W) * T.ndim);
    T.gather = gather.get();
    T.npars = npars.get();
    T.consts = consts.get();
    T.off = off.get();
    T.x = x.get();
    T.y = y.get();
    T.ye = ye.get();
    T.w = w.get();
    T.prior_type = ptype.get();
    T.prior_p1 = p1.get();
    T.prior_p2 = p2.get();
    T.prior_norm = pn.get();
    T.gp_gather = gpg.get();
    T.gp_base = gpb.get();
    T.gp_ecl = gpe.get();
    T.prior_c = nullptr;
    auto lnp = alloc<double>(W);
    const int rc = lfg_cpu_lnprob(walkers.get(), W, &T, lnp.get(), nthreads);
    put(&rc, 1);
    put(lnp.get(), W);
}

void predict_case(int nthreads)
{
    const int W = geti(), n = geti(), nb = geti(), has_var = geti();
    auto obs = get<int>(n);
    auto x = get<double>(n);
    auto ye = get<double>(n);
    auto res = get<double>(size_t(W) * n);
    auto hyp = get<double>(size_t(W) * 3);
    auto blocks = get<double>(size_t(W) * nb * 2);
    auto mean = alloc<double>(size_t(W) * n);
    auto var = has_var ? alloc<double>(size_t(W) * n) : nullptr;
    auto status = alloc<int>(W);
    const int rc = lfg_cpu_gp_predict(x.get(), ye.get(), obs.get(), res.get(), W, n, hyp.get(),
                                      nb ? blocks.get() : nullptr, nb, mean.get(), var.get(), status.get(), nthreads);
    put(&rc, 1);
    put(mean.get(), size_t(W) * n);
    if (has_var) put(var.get(), size_t(W) * n);
    put(status.get(), W);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) die("usage: abi_host <cases> <results> [swap]");
    fin = std::fopen(argv[1], "rb");
    fout = std::fopen(argv[2], "wb");
    if (!fin || !fout) die("cannot open the files");
    const bool swap = argc > 3;
    const int ncases = geti();
    for (int c = 0; c < ncases; ++c) {
        const int kind = geti();
        int nthreads = geti();
        if (swap) nthreads = nthreads == 1 ? 4 : 1;
        if (kind == 0 || kind == 1) flux_case(kind, nthreads);
        else if (kind == 2) lnprob_case(nthreads);
        else if (kind == 3) predict_case(nthreads);
        else die("unknown case kind");
    }
    if (std::fclose(fout) != 0) die("close");
    std::fclose(fin);
    std::printf("%d cases\n", ncases);
    return 0;
}
