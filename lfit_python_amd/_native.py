"""Loader for liblfg_hip.so, the gfx950 HIP library behind include/lfg.h.

The product path has no CPU fallback: every public entry point of this
package goes through the HIP kernels, and fails loudly when the library or a
GPU is missing.
"""
import ctypes
import hashlib
import os
import re
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(_HERE)
LIB_DIR = os.path.join(_HERE, "_lib")
LIB_PATH = os.path.join(LIB_DIR, "liblfg_hip.so")
# diagnostic builds (e.g. -DLFG_PROFILE_SETUP) are loaded through LFG_LIB,
# and only with LFG_DIAGNOSTIC=1 set as well: a stray LFG_LIB must not swap
# the product library silently
LOAD_PATH = LIB_PATH
if os.environ.get("LFG_LIB"):
    if os.environ.get("LFG_DIAGNOSTIC") != "1":
        raise RuntimeError("LFG_LIB=%s is set without LFG_DIAGNOSTIC=1: diagnostic builds are loaded only on "
                           "request (unset LFG_LIB to load %s)" % (os.environ["LFG_LIB"], LIB_PATH))
    LOAD_PATH = os.environ["LFG_LIB"]
SOURCES = [os.path.join(_HERE, "csrc", "lfg.hip"), os.path.join(_HERE, "csrc", "lfg_components.hip"),
           os.path.join(_HERE, "csrc", "lfg_pt.hip"),  # lfg_pt.hip: the parallel-tempering kernels, a unit of their own
           os.path.join(_HERE, "csrc", "lfg_gp_predict.hip"),  # the GP smoother and conditional sampler
           os.path.join(_HERE, "csrc", "lfg_physpar.hip"),  # physical parameters from chain rows (lfg_physpar.h)
           os.path.join(_HERE, "csrc", "lfg_wd.hip"),  # the white-dwarf atmosphere fit (lfg_wd.h)
           os.path.join(_HERE, "csrc", "lfg_chain.hip"),  # a chain's summary (lfg_chain.h)
           os.path.join(_HERE, "csrc", "lfg_limbdark.hip"),  # limb-darkening coefficients (lfg_limbdark.h)
           os.path.join(_HERE, "csrc", "lfg_corner.hip"),  # a corner plot's histograms and levels (lfg_corner.h)
           os.path.join(_HERE, "csrc", "lfg_chaintext.hip"),  # chain_prod.txt's rows (lfg_chaintext.h)
           os.path.join(_HERE, "csrc", "lfg_chainparse.hip")]  # chain_prod.txt's numbers read back (lfg_chainparse.h)
# k_pair's fold and LONG instantiations: the kernels header, compiled a second
# time without machine LICM (the reason: lfg_kernels.hpp, lfg_pair_launch_split)
SPLIT_SOURCE = os.path.join(_HERE, "csrc", "lfg_pair_split.hip")
SPLIT_FLAGS = ["-mllvm", "-disable-machine-licm"]
# every header a unit can include: whatever csrc/ holds, and the C ABI
HEADERS = sorted(os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))
                 if f.endswith((".hpp", ".h"))) + [os.path.join(REPO, "include", "lfg.h"),
                                                   os.path.join(REPO, "include", "lfg_physpar.h"),
                                                   os.path.join(REPO, "include", "lfg_wd.h"),
                                                   os.path.join(REPO, "include", "lfg_chain.h"),
                                                   os.path.join(REPO, "include", "lfg_limbdark.h"),
                                                   os.path.join(REPO, "include", "lfg_corner.h"),
                                                   os.path.join(REPO, "include", "lfg_chaintext.h"),
                                                   os.path.join(REPO, "include", "lfg_chainparse.h")]
INCLUDE = os.path.join(REPO, "include")
ARCH = "gfx950"

# element grid (MODEL_SPEC.md section 5; mirrors include/lfg.h)
NWD, NDISC, NBS, NDONOR = 400, 1000, 100, 400
NEL = NWD + NDISC + NBS
NGEO = 48
GP_PREDICT_MAX_NB = 16  # LFG_GP_PREDICT_MAX_NB (include/lfg.h)

STATUS_TEXT = {
    0: "ok",
    1: "invalid mass ratio q",
    2: "dphi has no inclination solution (dphi >= findphi(q, 90) or <= 0)",
    3: "invalid geometry (rwd, rdisc, scale or bright-spot exponents)",
    4: "the gas stream does not reach the disc radius",
    5: "non-finite or wrong-length parameter vector",
}
# lfg_physpar's rows (include/lfg_physpar.h) add one code
STATUS_TEXT_PHYSPAR = {**STATUS_TEXT, 5: "non-finite input, or rwd, twd or p not positive",
                       6: "no mass-radius relation brackets a white-dwarf mass"}


class LfgTree(ctypes.Structure):
    """ctypes mirror of struct lfg_tree (include/lfg.h)."""
    _fields_ = [
        ("E", ctypes.c_int), ("ndim", ctypes.c_int), ("nsub", ctypes.c_int),
        ("max_n", ctypes.c_int),
        ("gather", ctypes.c_void_p), ("npars", ctypes.c_void_p),
        ("consts", ctypes.c_void_p), ("off", ctypes.c_void_p),
        ("x", ctypes.c_void_p), ("y", ctypes.c_void_p),
        ("ye", ctypes.c_void_p), ("w", ctypes.c_void_p),
        ("prior_type", ctypes.c_void_p), ("prior_p1", ctypes.c_void_p),
        ("prior_p2", ctypes.c_void_p), ("prior_norm", ctypes.c_void_p),
        ("roche_priors", ctypes.c_int),
        ("gp", ctypes.c_int),
        ("gp_gather", ctypes.c_void_p), ("gp_base", ctypes.c_void_p),
        ("gp_ecl", ctypes.c_void_p),
        ("fixed_invalid", ctypes.c_int),
        ("prior_c", ctypes.c_void_p),
    ]


EXPORTS = ("lfg_workspace_size", "lfg_workspace_size_tree", "lfg_flux", "lfg_lnlike", "lfg_lnprob", "lfg_lnprior", "lfg_lnprob_timed",
           "lfg_stretch_lnprob_accept", "lfg_stretch_step_half", "lfg_stretch_step_half_spec",
           "lfg_stretch_step_shard", "lfg_stretch_step_shard_spec", "lfg_stretch_accept_regen_spec",
           "lfg_stretch_accept_regen", "lfg_stretch_step_shard_fold", "lfg_stretch_apply_verdicts",
           "lfg_elements", "lfg_roche", "lfg_stretch_propose", "lfg_stretch_accept",
           "lfg_stretch_propose_dev", "lfg_stretch_accept_dev", "lfg_event_create", "lfg_event_destroy",
           "lfg_event_elapsed_ms", "lfg_wdphases", "lfg_gp_lnlike", "lfg_component_workspace_size",
           "lfg_component", "lfg_version", "lfg_layout", "lfg_set_layout",
           "lfg_pt_workspace_size", "lfg_pt_propose", "lfg_pt_accept", "lfg_pt_swap",
           "lfg_gp_predict_workspace_size", "lfg_gp_predict", "lfg_gp_sample_workspace_size", "lfg_gp_sample",
           "lfg_gp_predict_tree_workspace_size", "lfg_gp_predict_tree")


# include/lfg_physpar.h: a set of its own (EXPORTS is include/lfg.h's, and pinned to it)
EXPORTS_PHYSPAR = ("lfg_physpar", "lfg_physpar_lanes")
MR_NWOOD, MR_MAX_KNOTS, MR_MAX_DOUBLES = 7, 32, 8192  # LFG_MR_* (include/lfg_physpar.h)


class LfgMrTables(ctypes.Structure):
    """ctypes mirror of struct lfg_mr_tables (include/lfg_physpar.h)."""
    _fields_ = [
        ("wood_t", ctypes.c_void_p), ("wood_r", ctypes.c_void_p), ("wood_off", ctypes.c_int * (MR_NWOOD + 1)),
        ("wood_card", ctypes.c_void_p), ("ham_m", ctypes.c_void_p), ("ham_r", ctypes.c_void_p),
        ("n_ham", ctypes.c_int),
        ("pan_tx", ctypes.c_void_p), ("pan_ty", ctypes.c_void_p), ("pan_c", ctypes.c_void_p),
        ("pan_nx", ctypes.c_int), ("pan_ny", ctypes.c_int),
        ("G", ctypes.c_double), ("GMsun", ctypes.c_double), ("Rsun", ctypes.c_double), ("day", ctypes.c_double),
    ]


# include/lfg_wd.h: a set of its own as well
EXPORTS_WD = ("lfg_wd_lnprob", "lfg_wd_step_half")
WD_NPAR, WD_MAX_BANDS, WD_MAX_KNOTS = 4, 8, 128  # LFG_WD_* (include/lfg_wd.h)


class LfgWdModel(ctypes.Structure):
    """ctypes mirror of struct lfg_wd_model (include/lfg_wd.h)."""
    _fields_ = [
        ("B", ctypes.c_int), ("nx", ctypes.c_int), ("ny", ctypes.c_int),
        ("tx", ctypes.c_void_p), ("ty", ctypes.c_void_p), ("c", ctypes.c_void_p),
        ("cnx", ctypes.c_int * WD_MAX_BANDS), ("cny", ctypes.c_int * WD_MAX_BANDS),
        ("ctx", ctypes.c_void_p * WD_MAX_BANDS), ("cty", ctypes.c_void_p * WD_MAX_BANDS),
        ("cc", ctypes.c_void_p * WD_MAX_BANDS),
        ("k", ctypes.c_double * WD_MAX_BANDS), ("mag", ctypes.c_double * WD_MAX_BANDS),
        ("err", ctypes.c_double * WD_MAX_BANDS), ("lnnorm", ctypes.c_double),
        ("prior_type", ctypes.c_int * WD_NPAR), ("prior_p1", ctypes.c_double * WD_NPAR),
        ("prior_p2", ctypes.c_double * WD_NPAR), ("prior_c0", ctypes.c_double * WD_NPAR),
        ("prior_c1", ctypes.c_double * WD_NPAR),
    ]


# include/lfg_chain.h: the chain's summary, a set of its own too
EXPORTS_CHAIN = ("lfg_chain_workspace_size", "lfg_chain_tile_rows", "lfg_chain_hist_tile", "lfg_chain_stats",
                 "lfg_chain_clip")
CHAIN_MAX_C, CHAIN_MAX_NQ = 4096, 8  # LFG_CHAIN_* (include/lfg_chain.h)

# include/lfg_limbdark.h: limb-darkening coefficients, a set of its own too
EXPORTS_LIMBDARK = ("lfg_limbdark", "lfg_limbdark_lanes")
LD_NBAND, LD_NCOEF, LD_NCOL, LD_MAX_KNOTS = 5, 5, 25, 64  # LFG_LD_* (include/lfg_limbdark.h)
ST_LD_CLAMPED = 7  # LFG_ST_LD_CLAMPED
STATUS_TEXT_LIMBDARK = {0: "ok", 5: "non-finite logg or teff", 7: "logg or teff outside the tables: clamped"}


class LfgLdTables(ctypes.Structure):
    """ctypes mirror of struct lfg_ld_tables (include/lfg_limbdark.h)."""
    _fields_ = [("tx", ctypes.c_void_p), ("ty", ctypes.c_void_p), ("nx", ctypes.c_int), ("ny", ctypes.c_int),
                ("c", ctypes.c_void_p)]

# include/lfg_corner.h: a corner plot's data, a set of its own too
EXPORTS_CORNER = ("lfg_corner_workspace_size", "lfg_corner_tile_rows", "lfg_corner_pair_tile", "lfg_corner_hist",
                  "lfg_corner_levels")
CORNER_MAX_K, CORNER_MAX_BINS, CORNER_MAX_LEVELS = 64, 64, 8  # LFG_CORNER_* (include/lfg_corner.h)

# include/lfg_chaintext.h: chain_prod.txt's rows, a set of its own too
EXPORTS_CHAINTEXT = ("lfg_chain_text_bound", "lfg_chain_text_workspace_size", "lfg_chain_text_tile_rows",
                     "lfg_chain_text")
CHAIN_TEXT_MAX_NDIM = 1023  # LFG_CHAIN_TEXT_MAX_NDIM (include/lfg_chaintext.h)

# include/lfg_chainparse.h: chain_prod.txt's numbers read back, a set of its own too
EXPORTS_CHAINPARSE = ("lfg_chain_parse_tile_bytes", "lfg_chain_parse_workspace_size", "lfg_chain_parse_count",
                      "lfg_chain_parse")
CHAIN_PARSE_MAX_TOKEN, CHAIN_PARSE_MAX_NCOL = 64, CHAIN_TEXT_MAX_NDIM + 2  # LFG_CHAIN_PARSE_* (include/lfg_chainparse.h)


FLAGS = ["--offload-arch=%s" % ARCH, "-O3", "-std=c++17", "-fPIC", "-shared"]
HASH_TAG = b"lfg-src-hash:"


def source_hash():
    """16 hex digits of SHA-256 over the library's sources, headers and
    compile flags: compiled into the library (lfg_version, and a tag string
    build() reads back), so a stale or foreign binary is told apart from
    the one this tree builds."""
    h = hashlib.sha256()
    for p in SOURCES + [SPLIT_SOURCE] + HEADERS:
        h.update(os.path.relpath(p, REPO).encode())
        with open(p, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(FLAGS + SPLIT_FLAGS).encode())
    return h.hexdigest()[:16]


def file_hash(path):
    """the source hash compiled into the library at `path` (None: no tag)"""
    try:
        with open(path, "rb") as fh:
            data = fh.read()
    except OSError:
        return None
    m = re.search(re.escape(HASH_TAG) + rb"([0-9a-f]{16})", data)
    return m.group(1).decode() if m else None


def needs_build():
    return file_hash(LIB_PATH) != source_hash()


def build(force=False, verbose=False):
    """Compile liblfg_hip.so in-tree for gfx950 (hipcc cross-compiles
    offline) unless the library there was built from exactly these sources
    and flags (its compiled-in source hash, not file times, decides)."""
    os.makedirs(LIB_DIR, exist_ok=True)
    want = source_hash()
    if not force and file_hash(LIB_PATH) == want:
        return LIB_PATH
    tmp = LIB_PATH + ".tmp"
    obj = LIB_PATH + ".split.tmp.o"
    cmds = [["hipcc"] + [f for f in FLAGS if f != "-shared"] + SPLIT_FLAGS + ["-I", INCLUDE, "-c", "-o", obj,
                                                                            SPLIT_SOURCE],
            ["hipcc"] + FLAGS + ['-DLFG_SRC_HASH="%s"' % want, "-I", INCLUDE, "-o", tmp] + SOURCES + ["-x", "none", obj]]
    try:
        for cmd in cmds:
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


def loaded_hash():
    """the source hash of the library this process loaded (lfg_version's src=)"""
    v = lib().lfg_version().decode()
    m = re.search(r"src=([0-9a-f]{16}|unhashed)", v)
    return m.group(1) if m else None


def verify():
    """Raise unless the loaded library is the one this tree's sources build
    (smoke() and the GPU test session check it before any kernel runs)."""
    got, want = loaded_hash(), source_hash()
    if got != want:
        raise RuntimeError("loaded %s carries source hash %s, the tree's sources hash to %s: a stale or foreign "
                           "library (rebuild with __graft_entry__.build())" % (LOAD_PATH, got, want))
    return got


_lib = None
_lock = threading.Lock()


def lib():
    """The loaded library; raises if it was never built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LOAD_PATH):
            raise RuntimeError(
                "liblfg_hip.so is missing (%s): run __graft_entry__.build() or "
                "lfit_python_amd._native.build(); there is no CPU fallback" % LOAD_PATH)
        L = ctypes.CDLL(LOAD_PATH)
        vp, ip, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        L.lfg_workspace_size.restype = sz
        L.lfg_workspace_size.argtypes = [ip, ip]
        L.lfg_workspace_size_tree.restype = sz
        L.lfg_workspace_size_tree.argtypes = [ip, ctypes.POINTER(LfgTree)]
        L.lfg_flux.restype = ip
        L.lfg_flux.argtypes = [vp, ip, ip, vp, vp, ip, ip, vp, vp, vp, vp, sz, vp]
        L.lfg_lnlike.restype = ip
        L.lfg_lnlike.argtypes = [vp, ip, ip, vp, vp, ip, ip, vp, vp, vp, vp, vp, sz, vp]
        L.lfg_lnprob.restype = ip
        L.lfg_lnprob.argtypes = [vp, ip, ctypes.POINTER(LfgTree), vp, vp, vp, sz, vp]
        L.lfg_lnprior.restype = ip
        L.lfg_lnprior.argtypes = [vp, ip, ctypes.POINTER(LfgTree), vp, vp, sz, vp]
        L.lfg_elements.restype = ip
        L.lfg_elements.argtypes = [vp, ip, ip, vp, vp, vp, vp, vp, vp, vp, sz, vp]
        L.lfg_roche.restype = ip
        L.lfg_roche.argtypes = [ip, vp, vp, ip, vp, vp, vp]
        L.lfg_lnprob_timed.restype = ip
        L.lfg_lnprob_timed.argtypes = [vp, ip, ctypes.POINTER(LfgTree), vp, vp, vp, sz, vp,
                                       ctypes.POINTER(vp)]
        u64, f64 = ctypes.c_ulonglong, ctypes.c_double
        L.lfg_stretch_propose.restype = ip
        L.lfg_stretch_propose.argtypes = [vp, ip, ip, ip, f64, u64, u64, vp, vp, vp]
        L.lfg_stretch_accept.restype = ip
        L.lfg_stretch_accept.argtypes = [vp, vp, ip, ip, ip, vp, vp, vp, u64, u64, vp, vp]
        L.lfg_stretch_lnprob_accept.restype = ip
        L.lfg_stretch_lnprob_accept.argtypes = [vp, vp, ip, ip, vp, vp, ctypes.POINTER(LfgTree), u64, u64, vp,
                                                vp, vp, sz, vp, ctypes.POINTER(vp)]
        L.lfg_stretch_step_half.restype = ip
        L.lfg_stretch_step_half.argtypes = [vp, vp, ip, ip, f64, u64, u64, vp, vp, ctypes.POINTER(LfgTree), vp,
                                            vp, vp, sz, vp, ctypes.POINTER(vp)]
        L.lfg_stretch_step_half_spec.restype = ip
        L.lfg_stretch_step_half_spec.argtypes = [vp, vp, ip, ip, f64, u64, u64, vp, vp, ctypes.POINTER(LfgTree),
                                                 vp, vp, ip, ip, vp, sz, vp, ctypes.POINTER(vp)]
        L.lfg_stretch_step_shard.restype = ip
        L.lfg_stretch_step_shard.argtypes = [vp, ip, ip, f64, u64, u64, ip, ip, vp, vp, ctypes.POINTER(LfgTree),
                                             vp, vp, sz, vp, ctypes.POINTER(vp)]
        L.lfg_stretch_step_shard_spec.restype = ip
        L.lfg_stretch_step_shard_spec.argtypes = [vp, ip, ip, f64, u64, u64, ip, ip, vp, vp,
                                                  ctypes.POINTER(LfgTree), vp, ip, ip, vp, sz, vp, ctypes.POINTER(vp)]
        L.lfg_stretch_accept_regen_spec.restype = ip
        L.lfg_stretch_accept_regen_spec.argtypes = [vp, vp, ip, ip, f64, u64, u64, vp, vp, ctypes.POINTER(LfgTree),
                                                    ip, vp, sz, vp]
        L.lfg_stretch_step_shard_fold.restype = ip
        L.lfg_stretch_step_shard_fold.argtypes = [vp, vp, ip, ip, f64, u64, u64, ip, ip, vp, vp,
                                                  ctypes.POINTER(LfgTree), vp, vp, vp, vp, ip, ip, vp, sz, vp,
                                                  ctypes.POINTER(vp)]
        L.lfg_stretch_apply_verdicts.restype = ip
        L.lfg_stretch_apply_verdicts.argtypes = [vp, vp, ip, ip, ip, f64, u64, u64, vp, vp, vp]
        L.lfg_stretch_accept_regen.restype = ip
        L.lfg_stretch_accept_regen.argtypes = [vp, vp, ip, ip, ip, f64, u64, u64, vp, vp, vp]
        L.lfg_stretch_propose_dev.restype = ip
        L.lfg_stretch_propose_dev.argtypes = [vp, ip, ip, ip, f64, u64, vp, vp, vp, vp]
        L.lfg_stretch_accept_dev.restype = ip
        L.lfg_stretch_accept_dev.argtypes = [vp, vp, ip, ip, ip, vp, vp, vp, u64, vp, vp, vp]
        L.lfg_pt_workspace_size.restype = sz
        L.lfg_pt_workspace_size.argtypes = [ip, ip]
        L.lfg_pt_propose.restype = ip
        L.lfg_pt_propose.argtypes = [vp, ip, ip, ip, ip, f64, u64, u64, vp, vp, vp]
        L.lfg_pt_accept.restype = ip
        L.lfg_pt_accept.argtypes = [vp, vp, vp, ip, ip, ip, ip, vp, vp, vp, vp, vp, ip, u64, u64, vp, vp]
        L.lfg_pt_swap.restype = ip
        L.lfg_pt_swap.argtypes = [vp, vp, vp, vp, ip, ip, ip, vp, u64, u64, vp, vp, sz, vp]
        L.lfg_event_create.restype = ip
        L.lfg_event_create.argtypes = [ctypes.POINTER(vp)]
        L.lfg_event_destroy.restype = ip
        L.lfg_event_destroy.argtypes = [vp]
        L.lfg_event_elapsed_ms.restype = ip
        L.lfg_event_elapsed_ms.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_float)]
        L.lfg_wdphases.restype = ip
        L.lfg_wdphases.argtypes = [vp, vp, vp, ip, ip, vp, vp, vp, vp]
        L.lfg_gp_lnlike.restype = ip
        L.lfg_gp_lnlike.argtypes = [vp, vp, vp, ip, ip, vp, vp, ip, vp, vp]
        L.lfg_gp_predict_workspace_size.restype = sz
        L.lfg_gp_predict_workspace_size.argtypes = [ip, ip]
        L.lfg_gp_predict.restype = ip
        L.lfg_gp_predict.argtypes = [vp, vp, vp, vp, ip, ip, vp, vp, ip, vp, vp, vp, vp, sz, vp]
        L.lfg_gp_sample_workspace_size.restype = sz
        L.lfg_gp_sample_workspace_size.argtypes = [ip, ip, ip]
        L.lfg_gp_sample.restype = ip
        L.lfg_gp_sample.argtypes = [vp, vp, vp, vp, ip, ip, vp, vp, ip, ip, u64, ip, vp, vp, vp, sz, vp]
        L.lfg_gp_predict_tree_workspace_size.restype = sz
        L.lfg_gp_predict_tree_workspace_size.argtypes = [ip, ctypes.POINTER(LfgTree)]
        L.lfg_gp_predict_tree.restype = ip
        L.lfg_gp_predict_tree.argtypes = [vp, ip, ctypes.POINTER(LfgTree), vp, vp, vp, vp, vp, sz, vp]
        L.lfg_component_workspace_size.restype = sz
        L.lfg_component_workspace_size.argtypes = [ip, ip, ip, ip]
        L.lfg_component.restype = ip
        L.lfg_component.argtypes = [ip, vp, ip, vp, vp, ip, ip, ip, vp, vp, ip, vp, vp, vp, sz, vp]
        L.lfg_version.restype = ctypes.c_char_p
        L.lfg_version.argtypes = []
        L.lfg_layout.restype = ip
        L.lfg_layout.argtypes = [ctypes.POINTER(LfgTree)]
        L.lfg_physpar.restype = ip
        L.lfg_physpar.argtypes = [vp, vp, vp, sz, vp, vp, ip, ctypes.POINTER(LfgMrTables), vp, vp, vp, vp]
        L.lfg_physpar_lanes.restype = ip
        L.lfg_physpar_lanes.argtypes = []
        L.lfg_wd_lnprob.restype = ip
        L.lfg_wd_lnprob.argtypes = [vp, sz, ip, ctypes.POINTER(LfgWdModel), vp, vp, vp, vp, vp]
        L.lfg_wd_step_half.restype = ip
        L.lfg_wd_step_half.argtypes = [vp, vp, ip, ip, f64, u64, u64, vp, ctypes.POINTER(LfgWdModel), vp, vp, vp, vp,
                                       vp]
        i64 = ctypes.c_longlong
        L.lfg_chain_workspace_size.restype = sz
        L.lfg_chain_workspace_size.argtypes = [i64, i64, ip, ip]
        L.lfg_chain_tile_rows.restype = ip
        L.lfg_chain_tile_rows.argtypes = []
        L.lfg_chain_hist_tile.restype = ip
        L.lfg_chain_hist_tile.argtypes = [ip]
        L.lfg_chain_stats.restype = ip
        L.lfg_chain_stats.argtypes = [vp, i64, i64, ip, i64, i64, vp, ctypes.POINTER(f64), ip, vp, vp, vp, vp, vp, vp,
                                      vp, vp, vp, vp, sz, vp]
        L.lfg_chain_clip.restype = ip
        L.lfg_chain_clip.argtypes = [vp, vp, vp, i64, f64, vp, vp, ip, vp]
        L.lfg_limbdark.restype = ip
        L.lfg_limbdark.argtypes = [vp, vp, sz, ip, ctypes.POINTER(LfgLdTables), vp, vp, vp]
        L.lfg_limbdark_lanes.restype = ip
        L.lfg_limbdark_lanes.argtypes = []
        L.lfg_corner_workspace_size.restype = sz
        L.lfg_corner_workspace_size.argtypes = [i64, i64, ip, ip]
        L.lfg_corner_tile_rows.restype = ip
        L.lfg_corner_tile_rows.argtypes = []
        L.lfg_corner_pair_tile.restype = ip
        L.lfg_corner_pair_tile.argtypes = [ip]
        L.lfg_corner_hist.restype = ip
        L.lfg_corner_hist.argtypes = [vp, i64, i64, ip, i64, i64, ctypes.POINTER(ip), ip, vp, ip, vp, vp, vp, vp, sz,
                                      vp]
        L.lfg_corner_levels.restype = ip
        L.lfg_corner_levels.argtypes = [vp, ip, ip, ctypes.POINTER(f64), ip, vp, vp]
        L.lfg_chain_text_bound.restype = i64
        L.lfg_chain_text_bound.argtypes = [i64, i64, ip, i64]
        L.lfg_chain_text_workspace_size.restype = sz
        L.lfg_chain_text_workspace_size.argtypes = [i64, i64, ip]
        L.lfg_chain_text_tile_rows.restype = ip
        L.lfg_chain_text_tile_rows.argtypes = [ip]
        L.lfg_chain_text.restype = ip
        L.lfg_chain_text.argtypes = [vp, i64, i64, ip, i64, i64, vp, i64, i64, i64, vp, sz, vp, vp, sz, vp]
        L.lfg_chain_parse_tile_bytes.restype = ip
        L.lfg_chain_parse_tile_bytes.argtypes = []
        L.lfg_chain_parse_workspace_size.restype = sz
        L.lfg_chain_parse_workspace_size.argtypes = [i64]
        L.lfg_chain_parse_count.restype = ip
        L.lfg_chain_parse_count.argtypes = [vp, i64, ip, vp, vp, sz, vp]
        L.lfg_chain_parse.restype = ip
        L.lfg_chain_parse.argtypes = [vp, i64, ip, vp, i64, vp, vp, sz, vp]
        if hasattr(L, "lfg_set_layout"):  # (older experiment builds lack it)
            L.lfg_set_layout.restype = ip
            L.lfg_set_layout.argtypes = [ip]
        _lib = L
        return L


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (what, rc))


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("lfit_python_amd needs a HIP GPU (MI355X): no device visible, "
                           "and the product path has no CPU fallback")


def stream_ptr(device=None):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Workspace:
    """Grow-only scratch buffers for the lfg_* entry points, one per device
    and stream.

    The rule: get() hands out the buffer of the stream that is current on
    `device` when it is called, and the caller launches on that same stream
    (stream_ptr).  Two streams therefore never share scratch, so calls made
    under different streams need no ordering between them, and calls on one
    stream are ordered by the stream itself.  When a request outgrows the
    stream's buffer, the old one is retired, not dropped: it stays alive,
    paired with an event recorded on its stream at that moment, until the
    event has completed, i.e. until every kernel queued on it has run.
    (torch hands out pooled streams, at most a few dozen per device, so the
    pool stays small.)"""

    _pool = {}     # (device index, stream handle) -> buffer
    _retired = []  # (event, buffer) of outgrown buffers whose queued work may not have finished

    @classmethod
    def get(cls, nbytes, device):
        import torch
        device = torch.device(device)
        index = device.index if device.index is not None else torch.cuda.current_device()
        stream = torch.cuda.current_stream(index)
        key = (index, stream.cuda_stream)
        cls._retired = [(e, b) for e, b in cls._retired if not e.query()]
        buf = cls._pool.get(key)
        if buf is None or buf.numel() < nbytes:
            if buf is not None:
                done = torch.cuda.Event()
                done.record(stream)
                cls._retired.append((done, buf))
            with torch.cuda.stream(stream):  # allocated for this stream, whatever device is current
                buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=torch.device("cuda", index))
            cls._pool[key] = buf
        return buf
