"""A corner plot's data on the device (include/lfg_corner.h, MODEL_SPEC.md
section 16): what the reference's fit_summary hands to corner.corner(chain,
bins=50) for every eclipse, reduced where the chain lies.

    corner_data(chain, cols, names, ...)  per column a marginal histogram, per
                                          pair a 2-D histogram and its contour
                                          levels -> CornerData (host arrays)
    corner_columns(model, names)          per eclipse the labels the reference
                                          plots (pure: no GPU)
    thumb_plot(data)                      the triangle, from the counts alone

A chain is what chainstats accepts (the sampler's [steps][W][ndim] on the
device, a walker-major array, a flat chain); it is read in place and only
the counts leave the device.  The counts equal np.histogram's and
np.histogram2d's bin for bin.
"""
import ctypes
import os

import numpy as np

from . import _native

DEFAULT_LEVELS = tuple(float(f) for f in 1.0 - np.exp(-0.5 * np.arange(0.5, 2.1, 0.5) ** 2))  # corner's own


class CornerData:
    """Host arrays of K columns, P = K (K - 1) / 2 pairs and nb bins:
    cols [K] (indices into the chain's row), names [K], edges [K, nb + 1] (NaN
    for an immobile column), hist1d [K, nb], hist2d [P, nb, nb] (first axis:
    the pair's first column), levels [P, nl] (int64 counts, in the order of
    fracs), fracs [nl], mobile [K] (False: no dynamic range, all counts
    zero)."""

    FIELDS = ("cols", "names", "edges", "hist1d", "hist2d", "levels", "fracs", "mobile")

    def __init__(self, **arrays):
        for k in self.FIELDS:
            setattr(self, k, arrays[k])

    @property
    def K(self):
        return len(self.cols)

    def pair(self, a, b):
        """the index into hist2d and levels of columns a < b (positions in cols)"""
        K = self.K
        if not 0 <= a < b < K:
            raise IndexError("a pair is (a, b) with 0 <= a < b < %d" % K)
        return a * (2 * K - a - 1) // 2 + (b - a - 1)

    def select(self, keep):
        """the data of the columns at positions `keep` (ascending) alone: a
        pair's counts do not depend on the other columns"""
        keep = [int(k) for k in keep]
        pp = [self.pair(a, b) for i, a in enumerate(keep) for b in keep[i + 1:]]
        return CornerData(cols=np.asarray(self.cols)[keep], names=[self.names[k] for k in keep],
                          edges=self.edges[keep], hist1d=self.hist1d[keep], hist2d=self.hist2d[pp],
                          levels=self.levels[pp], fracs=self.fracs, mobile=np.asarray(self.mobile)[keep])

    def save(self, path):
        np.savez(path, **{k: np.asarray(getattr(self, k)) for k in self.FIELDS})
        return path

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in cls.FIELDS}
        d["names"] = [str(n) for n in d["names"]]
        return cls(**d)


def _pick(cols, names, ndim):
    """-> (column indices, their names)"""
    names = None if names is None else [str(n) for n in names]
    if cols is None:
        cols = range(len(names) if names is not None else ndim)
    idx = []
    for c in cols:
        if isinstance(c, str):
            if names is None or c not in names:
                raise KeyError("no column named %r in the chain" % c)
            idx.append(names.index(c))
        else:
            idx.append(int(c))
    if not 1 <= len(idx) <= _native.CORNER_MAX_K:
        raise ValueError("a corner plot takes 1 to %d columns, not %d" % (_native.CORNER_MAX_K, len(idx)))
    if len(set(idx)) != len(idx) or min(idx) < 0 or max(idx) >= ndim:
        raise ValueError("columns must be distinct and inside the chain's %d" % ndim)
    return idx, [names[i] if names is not None and i < len(names) else "col%d" % i for i in idx]


def _default_range(v, idx):
    """[K][2] on the device: each column's minimum and maximum, from
    lfg_chain_stats over the run of columns that holds them"""
    import torch
    from . import chainstats
    c0, c1 = min(idx), max(idx) + 1
    # (the same rows: v.tensor is [steps][W][ndim], already skipped and thinned)
    span = chainstats._View(v.tensor, slice(c0, c1), False, 0, 1, v.device)
    r = chainstats._run(span, np.empty(0))
    at = torch.as_tensor([i - c0 for i in idx], dtype=torch.int64, device=v.device)
    return torch.stack([r["min"][at], r["max"][at]], dim=1).contiguous()


def _device_counts(v, idx, rng, nb, fracs):
    """lfg_corner_hist and lfg_corner_levels on view v -> device tensors"""
    import torch
    L = _native.lib()
    K, dev = len(idx), v.device
    P = K * (K - 1) // 2
    fr = np.ascontiguousarray(fracs, dtype=np.float64).reshape(-1)
    cols = (ctypes.c_int * K)(*idx)
    with torch.cuda.device(dev):
        h1 = torch.empty((K, nb), dtype=torch.int64, device=dev)
        h2 = torch.empty((P, nb, nb), dtype=torch.int64, device=dev)
        flag = torch.empty(K, dtype=torch.int32, device=dev)
        lev = torch.empty((P, fr.size), dtype=torch.int64, device=dev)
        nbytes = L.lfg_corner_workspace_size(v.steps, v.W, K, nb)
        if nbytes == 0:
            raise ValueError("lfg_corner_hist refuses %d columns of %d bins (at most %d and %d)" %
                             (K, nb, _native.CORNER_MAX_K, _native.CORNER_MAX_BINS))
        ws = _native.Workspace.get(nbytes, dev)
        st = _native.stream_ptr(dev)
        rc = L.lfg_corner_hist(ctypes.c_void_p(v.ptr), v.steps, v.W, v.C, v.step_ld, v.walker_ld, cols, K,
                               ctypes.c_void_p(rng.data_ptr()), nb, ctypes.c_void_p(h1.data_ptr()),
                               ctypes.c_void_p(h2.data_ptr()) if K > 1 else None, ctypes.c_void_p(flag.data_ptr()),
                               ctypes.c_void_p(ws.data_ptr()), nbytes, st)
        _native.check(rc, "lfg_corner_hist")
        if P:
            rc = L.lfg_corner_levels(ctypes.c_void_p(h2.data_ptr()), P, nb,
                                     fr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), fr.size,
                                     ctypes.c_void_p(lev.data_ptr()), st)
            _native.check(rc, "lfg_corner_levels")
    return h1, h2, flag, lev


def corner_data(chain, cols=None, names=None, bins=50, range=None, levels=DEFAULT_LEVELS, nskip=0, thin=1,
                walker_major=False, device=None):
    """The data of corner.corner(chain[:, cols], bins=bins) -> CornerData.

    cols: column indices or names (names: the chain's header), in the order
    the plot shows them; None: every named column (every column without
    names).  range: [K, 2] (lo, hi) per column, host or device; None: each
    column's minimum and maximum, taken on the device.  levels: the fractions
    of the total inside each contour (corner's default).  nskip, thin,
    walker_major as in chainstats.  A column without dynamic range (hi <= lo,
    or no finite value) is flagged immobile and counts nothing, as the
    reference drops it."""
    import torch
    from . import chainstats
    nb = int(bins)
    fr = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    if not 1 <= nb <= _native.CORNER_MAX_BINS:
        raise ValueError("1 to %d bins, not %d" % (_native.CORNER_MAX_BINS, nb))
    if not 1 <= fr.size <= _native.CORNER_MAX_LEVELS or not np.all((fr >= 0.0) & (fr <= 1.0)):
        raise ValueError("1 to %d level fractions, each in [0, 1]" % _native.CORNER_MAX_LEVELS)
    v = chainstats._View(chain, None, walker_major, nskip, thin, device)
    idx, picked = _pick(cols, names, v.C)
    K = len(idx)
    if range is None:
        rng = _default_range(v, idx)
    else:
        rng = torch.as_tensor(range, dtype=torch.float64).to(v.device).reshape(K, 2).contiguous()
    h1, h2, flag, lev = _device_counts(v, idx, rng, nb, fr)
    lohi = rng.cpu().numpy()
    mobile = flag.cpu().numpy() == 0
    edges = np.full((K, nb + 1), np.nan)
    for k in np.nonzero(mobile)[0]:
        edges[k] = np.linspace(lohi[k, 0], lohi[k, 1], nb + 1)
    return CornerData(cols=np.asarray(idx, dtype=np.int64), names=picked, edges=edges, hist1d=h1.cpu().numpy(),
                      hist2d=h2.cpu().numpy(), levels=lev.cpu().numpy(), fracs=fr, mobile=mobile)


def corner_columns(model, names):
    """Per eclipse of the model, the labels the reference's fit_summary plots:
    '<par>_<label>' for the eclipse's, then its band's, then the core's
    node_par_names, keeping only those in the chain header `names`, in that
    order.  -> [(eclipse node, [labels])] in the tree's order (an eclipse
    with no label in the chain has an empty list)."""
    have = set(str(n) for n in names)
    out = []
    for ecl in (n for n in model.walk() if "Eclipse" in type(n).__name__):
        band = ecl.parent
        core = band.parent
        labels = ["{}_{}".format(p, node.label) for node in (ecl, band, core) for p in node.node_par_names]
        out.append((ecl, [lab for lab in labels if lab in have]))
    return out


def thumb_plot(data, figsize=None):
    """The triangle of a CornerData, from its counts alone: stairs on the
    diagonal, contours of hist2d at the levels below it.  Immobile columns are
    left out.  A figure has K (K + 1) / 2 axes; at the reference's 20 columns
    matplotlib needs several seconds for them.  -> matplotlib Figure."""
    try:
        import matplotlib
        from matplotlib.figure import Figure
    except ImportError as e:
        raise RuntimeError("thumb_plot needs matplotlib, which does not import here (%s); the counts are in "
                           "CornerData and its .npz" % e)
    del matplotlib
    keep = [k for k in range(data.K) if data.mobile[k]]
    n = len(keep)
    fig = Figure(figsize=figsize or (2.2 * n + 1, 2.2 * n + 1))
    if n == 0:
        return fig
    grid = fig.add_gridspec(n, n, wspace=0.05, hspace=0.05)
    axes = [[fig.add_subplot(grid[i, j]) for j in range(i + 1)] for i in range(n)]   # the lower triangle only
    for i, ki in enumerate(keep):
        ax = axes[i][i]
        ax.stairs(data.hist1d[ki], data.edges[ki], color="k")
        ax.set_yticks([])
        for j, kj in enumerate(keep[:i]):
            ax = axes[i][j]          # x: column kj, y: column ki
            h = data.hist2d[data.pair(kj, ki)]
            ex, ey = data.edges[kj], data.edges[ki]
            # corner's fudge, which belongs to drawing: equal levels are told apart
            lv = np.sort(np.asarray(data.levels[data.pair(kj, ki)], dtype=np.float64))
            if h.sum() > 0:
                for m in np.nonzero(lv[1:] == lv[:-1])[0]:
                    lv[m] *= 1.0 - 1e-4
                lv = np.unique(lv[lv > 0])
                if lv.size and h.shape[0] > 1:
                    ax.contour(0.5 * (ex[1:] + ex[:-1]), 0.5 * (ey[1:] + ey[:-1]), h.T, levels=lv, colors="k",
                               linewidths=0.8)
            ax.set_xlim(ex[0], ex[-1])
            ax.set_ylim(ey[0], ey[-1])
        for j in range(i + 1):
            ax = axes[i][j]
            if i == n - 1:
                ax.set_xlabel(data.names[keep[j]])
            else:
                ax.set_xticklabels([])
            if j == 0 and i > 0:
                ax.set_ylabel(data.names[ki])
            elif j > 0 or i == 0:
                ax.set_yticklabels([])
    return fig


def save_plot(data, path):
    """thumb_plot as a .png (Agg canvas: no display needed)"""
    fig = thumb_plot(data)
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    FigureCanvasAgg(fig)
    fig.savefig(path, dpi=80)
    return path


def eclipse_corners(chain, names, model, out_dir="Final_figs", nskip=0, thin=1, walker_major=False, bins=50,
                    plot=True, log=print):
    """fit_summary's corner step: for every eclipse corner_columns' labels,
    the immobile ones dropped as the reference drops them, written as
    <out_dir>/<lightcurve stem>_corners.npz and, where matplotlib imports,
    _corners.png.  -> the list of files written."""
    import torch
    _native.require_gpu()
    if not (isinstance(chain, torch.Tensor) and chain.is_cuda):   # one transfer for all the eclipses
        chain = torch.as_tensor(np.asarray(chain, dtype=np.float64)).cuda()
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for ecl, labels in corner_columns(model, names):
        if not labels:
            continue
        d = corner_data(chain, cols=labels, names=names, bins=bins, nskip=nskip, thin=thin, walker_major=walker_major)
        d = d.select(np.nonzero(d.mobile)[0])
        if d.K == 0:
            continue
        fname = getattr(ecl.lc, "fname", None) or str(ecl.lc.name)
        stem = os.path.splitext(os.path.split(fname)[1])[0]
        path = os.path.join(out_dir, stem + "_corners.npz")
        written.append(d.save(path))
        log("Corner data of eclipse {}: {} columns -> {}".format(ecl.label, d.K, path))
        if plot:
            try:
                written.append(save_plot(d, os.path.join(out_dir, stem + "_corners.png")))
            except RuntimeError as e:
                log(str(e))
    return written
