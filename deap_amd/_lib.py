"""ctypes binding of ``libgpeval.so`` (C ABI declared in ``include/gpeval.h``).

The library is built in-tree by ``__graft_entry__.build()`` /
``python -m deap_amd.build``.  There is no fallback: if the shared object is
missing or fails to load, every evaluator entry point raises.
"""
import ctypes
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DEAP_AMD_LIB: an alternative build of the same library (A/B runs)
LIB_PATH = os.environ.get("DEAP_AMD_LIB") or os.path.join(_HERE, "libgpeval.so")

GPE_MACHINE_F = 0
GPE_MACHINE_B = 1
GPE_MODE_MSE = 0
GPE_MODE_HITS_BOOL = 1
GPE_MODE_HITS_BITS = 2
GPE_MODE_SSE_NUMPY = 3
GPE_MODE_SSE_SEQ = 4
GPE_PREC_F64 = 0
GPE_PREC_F32 = 1
GPE_NO_ERROR = 0xFFFFFFFFFFFFFFFF
GPE_ERR_VALUE = 1
GPE_ERR_OVERFLOW = 2
GPE_ERR_XINT_RANGE = 3
GPE_XINT_WORDS = 34
GPE_FLAG_NONFINITE_TERM = 1
GPE_FLAG_NAN_TERM = 2
GPE_FLAG_INF_TERM = 4
GPE_FLAG_MOMENT_RANGE = 8

# every symbol include/gpeval.h declares, with (restype, argtypes)
_P = ctypes.c_void_p
_I = ctypes.c_int
_I64 = ctypes.c_int64
SIGNATURES = {
    "gpe_create": (_I, [_I, ctypes.POINTER(_P)]),
    "gpe_destroy": (None, [_P]),
    "gpe_last_error": (ctypes.c_char_p, [_P]),
    "gpe_device_info": (_I, [_P, ctypes.POINTER(_I), ctypes.POINTER(_I),
                             ctypes.c_char_p, ctypes.c_size_t]),
    "gpe_set_cases": (_I, [_P, _I, _P, _I, _I64, _P, _I]),
    "gpe_select_cases": (_I, [_P, _P, _I64]),
    "gpe_case_subset": (_I, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "gpe_set_trig_leaves": (_I, [_P, _I]),
    "gpe_set_precision": (_I, [_P, _I]),
    "gpe_load_programs": (_I, [_P, _P, _I64, _P, _I64, _P]),
    "gpe_run": (_I, [_P, _I, _P, _P, _P, _P]),
    "gpe_run_device": (_I, [_P, _I, _P, _P, _P, _P]),
    "gpe_run_cases": (_I, [_P, _I, _P, _P, _P, _P, _P]),
    "gpe_run_values": (_I, [_P, _P, _P]),
    "gpe_run_values_device": (_I, [_P, _P, _P]),
    "gpe_run_values_bits": (_I, [_P, _P]),
    "gpe_run_moments": (_I, [_P, _P, _P, _P]),
    "gpe_run_scaled": (_I, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "gpe_run_scaled_device": (_I, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "gpe_host_scaled_from_moments": (_I, [_P, _I64, _I64, _P, _P, _P, _P, _P,
                                          _P]),
    "gpe_run_abserr": (_I, [_P, ctypes.c_double, _P, _P, _P]),
    "gpe_run_abserr_device": (_I, [_P, ctypes.c_double, _P, _P, _P]),
    "gpe_host_abserr": (_I, [_P, _P, _I64, _I64, ctypes.c_double, _P, _P]),
    "gpe_run_abserr_cases": (_I, [_P, ctypes.c_double, _P, _P, _P, _P]),
    "gpe_host_abserr_cases": (_I, [_P, _P, _I64, _I64, _P]),
    "gpe_lexicase": (_I, [_P, _P, _I64, _I64, _P, _I, ctypes.c_double, _P,
                          _I64, _P, ctypes.POINTER(_I64)]),
    "gpe_run_hit_planes": (_I, [_P, _P, _P, _P, _P]),
    "gpe_run_typed_hit_planes": (_I, [_P, _P, _P, _P, _P]),
    "gpe_host_typed_hit_planes": (_I, [_P, _P, _I64, _I64, _P]),
    "gpe_read_hit_planes": (_I, [_P, _P]),
    "gpe_host_hit_planes": (_I, [_P, _P, _I64, _I64, _P]),
    "gpe_lexicase_bits": (_I, [_P, _P, _I64, _I64, _P, _I64, _P,
                               ctypes.POINTER(_I64)]),
    "gpe_informed_cases": (_I, [_P, _P, _I64, _I64, ctypes.c_double,
                                ctypes.c_uint64, _I64, _P, _P]),
    "gpe_host_informed_cases": (_I, [_P, _I64, _I64, ctypes.c_uint64, _I64,
                                     _P, _P]),
    "gpe_host_hit_threshold": (_I, [_P, _I64, _I64, ctypes.c_double, _P]),
    "gpe_lexicase_par": (_I, [_P, _P, _I64, _I64, _P, _I, ctypes.c_double,
                              ctypes.c_uint64, _I64, _P, _P]),
    "gpe_lexicase_bits_par": (_I, [_P, _P, _I64, _I64, ctypes.c_uint64, _I64,
                                   _P, _P]),
    "gpe_host_lexicase_par": (_I, [_P, _I64, _I64, _P, _I, ctypes.c_double,
                                   ctypes.c_uint64, _I64, _P, _P]),
    "gpe_lexicase_par_lds_values": (_I64, []),
    "gpe_dalex": (_I, [_P, _P, _I64, _I64, ctypes.c_uint64, ctypes.c_double,
                       _I, _I64, _P, _P]),
    "gpe_dalex_bits": (_I, [_P, _P, _I64, _I64, ctypes.c_uint64,
                            ctypes.c_double, _I, _I64, _P, _P]),
    "gpe_dalex_weights": (_I, [_P, _I64, _I64, ctypes.c_uint64,
                               ctypes.c_double, _P, _P]),
    "gpe_dalex_sigma": (_I, [_P, _P, _I64, _I64, _P]),
    "gpe_weighted_errors": (_I, [_P, _P, _I64, _I64, _P, _I64, _P]),
    "gpe_last_dalex_ms": (_I, [_P, ctypes.POINTER(ctypes.c_float)]),
    "gpe_host_dalex_weights": (_I, [_I64, _I64, ctypes.c_uint64,
                                    ctypes.c_double, _P, _P]),
    "gpe_host_dalex_sigma": (_I, [_P, _I64, _I64, _P]),
    "gpe_host_dalex": (_I, [_P, _I64, _I64, ctypes.c_uint64, ctypes.c_double,
                            _I, _I64, _P, _P]),
    "gpe_nd_sort": (_I, [_P, _P, _P, _I64, _I64, _I64, _I, _P, _P,
                         ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "gpe_last_nd_sort_ms": (_I, [_P, ctypes.POINTER(ctypes.c_float)]),
    "gpe_last_nd_sort_fronts": (_I, [_P, ctypes.POINTER(_I64)]),
    "gpe_host_nd_sort": (_I, [_P, _P, _I64, _I64, _I64, _I, _P, _P,
                              ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "gpe_hit_group_counts": (_I, [_P, _P, _I64, _I64, _P, _I, _P]),
    "gpe_host_hit_group_counts": (_I, [_P, _I64, _I64, _P, _I, _P]),
    "gpe_last_hit_group_ms": (_I, [_P, ctypes.POINTER(ctypes.c_float)]),
    "gpe_case_solve_counts": (_I, [_P, _P, _I64, _I64, ctypes.c_double, _P,
                                   _P]),
    "gpe_hit_weighted_sums": (_I, [_P, _P, _I64, _I64, ctypes.c_double, _P,
                                   _I, _P]),
    "gpe_hit_shared_sums": (_I, [_P, _P, _I64, _I64, ctypes.c_double, _P, _P,
                                 _P]),
    "gpe_last_case_weights_ms": (_I, [_P, ctypes.POINTER(ctypes.c_float)]),
    "gpe_host_case_solve_counts": (_I, [_P, _I64, _I64, _P, _P]),
    "gpe_host_hit_weighted_sums": (_I, [_P, _I64, _I64, _P, _I, _P, _P]),
    "gpe_host_hit_shared_sums": (_I, [_P, _I64, _I64, _P, _P, _P, _P]),
    "gpe_set_lowering": (_I, [_P, _I, _I, _P, _I, _P, _I]),
    "gpe_lower_programs": (_I, [_P, _P, _P, _I64, _P, _P, _P, _P, _P]),
    "gpe_lower_begin": (_I, [_P, _I64]),
    "gpe_lower_begin_into": (_I, [_P, _I64, _P, _P, _P]),
    "gpe_lower_add": (_I, [_P, _P, _P, _I64, _P, _P]),
    "gpe_lower_end": (_I, [_P, _P, _P, _P]),
    "gpe_tournament": (_I, [_P, _P, _I64, _I, ctypes.c_double, _I64, _I, _P,
                            _P]),
    "gpe_eval": (_I, [_P, _I, _P, _I64, _P, _I64, _P, _P, _P, _P, _P]),
    "gpe_last_timing": (_I, [_P, ctypes.POINTER(ctypes.c_float)]),
    "gpe_last_geometry": (_I, [_P, ctypes.POINTER(ctypes.c_int64)]),
    "gpe_last_geometry_ex": (_I, [_P, ctypes.POINTER(ctypes.c_int64), _I]),
    "gpe_last_launch_shape": (_I, [_P, _I, ctypes.POINTER(ctypes.c_int64), _I]),
    "gpe_math_probe": (_I, [_P, _I, _P, _P, _I64]),
    "gpe_host_math": (_I, [_I, _P, _P, _I64]),
    "gpe_host_np_sum": (_I, [_P, _I64, _I64, _P]),
    "gpe_debug_translate": (_I, [_P, _I64, _P, _I64, _P, _I, _P, _I, _P,
                                 _I64, _P, _P]),
    "gpe_debug_translate_ranges": (_I, [_P, _I64, _P, _I64, _P, _I, _P, _I, _P,
                                        _I64, _P, _P, _P, _P]),
    "gpe_debug_trig_classes": (_I, [_P, _I64, _P, _P, _I, _P, _I64]),
    "gpe_last_trig_classes": (_I, [_P, ctypes.POINTER(ctypes.c_int64)]),
    "gpe_debug_translate_mode": (_I, [_P, _I64, _P, _I64, _P, _I, _P, _I, _P,
                                         _I64, _P, _P, _P, _P, _I]),
    "gpe_debug_trig_classes_mode": (_I, [_P, _I64, _P, _P, _I, _I, _P, _I64]),
    "gpe_debug_trig_picks": (_I, [_P, _I64, _P, _P, _I, _I, _P, _I64]),
    "gpe_last_trig_picked": (_I, [_P, ctypes.POINTER(ctypes.c_int64)]),
    "gpe_comm_unique_id": (_I, [_P]),
    "gpe_comm_init": (_I, [_P, _I, _I, _P]),
    "gpe_comm_info": (_I, [_P, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "gpe_run_sharded_device": (_I, [_P, _I, _I64, _P, _P, _P, _P]),
    "gpe_run_sharded": (_I, [_P, _I, _I64, _P, _P, _P, _P]),
    "gpe_run_gathered": (_I, [_P, _I, _I64, _P, _P, _P, _P, _P]),
    "gpe_load_exact": (_I, [_P, _P, _I64, _P, _I64, _P, _P, _P, _I64]),
    "gpe_load_exact_v": (_I, [_P, _P, _I64, _P, _I64, _P, _P, _P, _P, _I64]),
    "gpe_last_exact_host_runs": (_I, [_P, ctypes.POINTER(ctypes.c_int64)]),
    "gpe_last_exact_host_ms": (_I, [_P, ctypes.POINTER(ctypes.c_double)]),
    "gpe_last_lower_flags": (_I, [_P, ctypes.POINTER(ctypes.c_int64),
                                  ctypes.POINTER(ctypes.c_int64)]),
    "gpe_debug_shard_combine": (_I, [_P, _I, _I64, _P, _P, _P, _P, _P, _P,
                                     _P, _P]),
    "gpe_debug_redo_union": (_I, [_P, _P, _I64]),
    "gpe_host_exact_eval": (_I, [_P, _P, _P, _I64, _P, _I, _P, _P,
                                 ctypes.POINTER(_I)]),
    "gpe_host_bigint_eval": (_I, [_P, _P, _P, _I64, _P, _I, _P, _P,
                                  ctypes.POINTER(ctypes.c_int64),
                                  ctypes.POINTER(_I)]),
    "gpe_last_comm_timing": (_I, [_P, ctypes.POINTER(ctypes.c_float)]),
    "gpe_debug_bounded_wait": (_I, [ctypes.c_double, _I64, ctypes.c_char_p,
                                    ctypes.c_size_t]),
}
GPE_E_INVALID = -1
GPE_E_COMM = -5
GPE_E_ARG = -6
GPE_UNIQUE_ID_BYTES = 128

_lib = None


class GpeError(RuntimeError):
    pass


def load(path=LIB_PATH):
    """Load the HIP library (raises if it is absent — no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise GpeError("libgpeval.so not built (%s); run "
                       "`python -m deap_amd.build`" % path)
    # one HIP runtime per process: torch ships its own libamdhip64.so.7 and
    # whichever loads first serves both, so let torch (needed for RCCL
    # collectives in deap_amd.distributed) load it first when present
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def debug_bounded_wait(timeout_s, busy_polls):
    """The library's bounded wait on collectives, on a fake stream busy for
    *busy_polls* queries (< 0: forever): (return code, message)."""
    lib = load()
    buf = ctypes.create_string_buffer(512)
    rc = lib.gpe_debug_bounded_wait(float(timeout_s), int(busy_polls), buf,
                                    len(buf))
    return rc, buf.value.decode()


def host_math(fn, x):
    """Host-compiled twin of the kernels' sin/cos/square (CPU, no GPU)."""
    lib = load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.zeros_like(x)
    rc = lib.gpe_host_math(int(fn), _ptr(x), _ptr(y), len(x))
    if rc != 0:
        raise GpeError("gpe_host_math failed (%d)" % rc)
    return y


def host_np_sum(rows):
    """Host twin of the GPE_MODE_SSE_NUMPY reduction: numpy.sum of each row
    in numpy's own order (CPU, no GPU)."""
    x = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float64)
    out = np.zeros(x.shape[0])
    rc = load().gpe_host_np_sum(_ptr(x), x.shape[0], x.shape[1], _ptr(out))
    if rc != 0:
        raise GpeError("gpe_host_np_sum failed (%d)" % rc)
    return out


def _dd(x):
    """A (hi, lo) double-double as the float64[2] the library reads."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape != (2,):
        raise ValueError("a double-double is (hi, lo)")
    return x


def host_scaled_from_moments(m6, n_cases, sy, syy, flags=None):
    """Host twin of the formula gpe_run_scaled applies on the device (CPU, no
    GPU): moments ``[n, 6]``, the target's ``Sy``, ``Syy`` as (hi, lo) →
    ``(mse, a, b)`` float64 ``[n]``."""
    m6 = np.ascontiguousarray(np.atleast_2d(m6), dtype=np.float64)
    if m6.shape[1] != 6:
        raise ValueError("moments must be [n, 6]")
    n = m6.shape[0]
    sy, syy = _dd(sy), _dd(syy)
    fl = None if flags is None else \
        np.ascontiguousarray(flags, dtype=np.uint32)
    mse, a, b = np.zeros(n), np.zeros(n), np.zeros(n)
    rc = load().gpe_host_scaled_from_moments(
        _ptr(m6), n, int(n_cases), _ptr(sy), _ptr(syy),
        None if fl is None else _ptr(fl), _ptr(mse), _ptr(a), _ptr(b))
    if rc != 0:
        raise GpeError("gpe_host_scaled_from_moments failed (%d)" % rc)
    return mse, a, b


def host_abserr(f, terms, hit_eps):
    """Host twin of the abs-error rows reduction (CPU, no GPU): one program's
    per-case values ``f[n]`` against ``terms[n_terms, n]`` →
    ``(out4 float64[4] = (sum hi, sum lo, max, hits), flags)``."""
    f = np.ascontiguousarray(f, dtype=np.float64)
    t = np.ascontiguousarray(np.atleast_2d(terms), dtype=np.float64)
    if f.ndim != 1 or t.shape[1] != len(f):
        raise ValueError("f is [n] and terms [n_terms, n]")
    out4 = np.zeros(4, dtype=np.float64)
    flags = np.zeros(1, dtype=np.uint32)
    rc = load().gpe_host_abserr(_ptr(f), _ptr(t), t.shape[0], len(f),
                                float(hit_eps), _ptr(out4), _ptr(flags))
    if rc != 0:
        raise GpeError("gpe_host_abserr failed (%d)" % rc)
    return out4, int(flags[0])


def host_abserr_cases(f, terms):
    """Host twin of a cases run's per-case value (CPU, no GPU): one program's
    per-case values ``f[n]`` against ``terms[n_terms, n]`` → ``e[n]``."""
    f = np.ascontiguousarray(f, dtype=np.float64)
    t = np.ascontiguousarray(np.atleast_2d(terms), dtype=np.float64)
    if f.ndim != 1 or t.shape[1] != len(f):
        raise ValueError("f is [n] and terms [n_terms, n]")
    out = np.zeros(len(f), dtype=np.float64)
    rc = load().gpe_host_abserr_cases(_ptr(f), _ptr(t), t.shape[0], len(f),
                                      _ptr(out))
    if rc != 0:
        raise GpeError("gpe_host_abserr_cases failed (%d)" % rc)
    return out


def host_hit_planes(result_planes, out_plane, n_cases):
    """Host twin of a hit-planes run's plane arithmetic (CPU, no GPU): result
    planes ``uint32[n, ceil(n_cases / 32)]`` against the output plane →
    hit planes of the same shape (pad bits 0)."""
    r = np.ascontiguousarray(np.atleast_2d(result_planes), dtype=np.uint32)
    o = np.ascontiguousarray(out_plane, dtype=np.uint32)
    units = (int(n_cases) + 31) // 32
    if n_cases < 1 or r.shape[1] != units or o.shape != (units,):
        raise ValueError("planes are [n, %d] and the output plane [%d] for "
                         "%d cases" % (units, units, n_cases))
    out = np.zeros_like(r)
    rc = load().gpe_host_hit_planes(_ptr(r), _ptr(o), r.shape[0],
                                    int(n_cases), _ptr(out))
    if rc != 0:
        raise GpeError("gpe_host_hit_planes failed (%d)" % rc)
    return out


def host_typed_hit_planes(values, labels):
    """Host twin of a typed hit-planes run's word arithmetic (CPU, no GPU):
    program outputs ``float64[n, n_cases]`` against *labels* → hit planes
    ``uint32[n, ceil(n_cases / 32)]``, bit c set where ``bool(value)`` is
    ``bool(label)`` (a nan output is true); pad bits 0."""
    v = np.ascontiguousarray(np.atleast_2d(values), dtype=np.float64)
    lab = np.ascontiguousarray(labels, dtype=np.float64)
    if lab.ndim != 1 or len(lab) < 1 or v.shape[1] != len(lab):
        raise ValueError("values are [n, n_cases] and labels [n_cases]")
    out = np.zeros((v.shape[0], (len(lab) + 31) // 32), dtype=np.uint32)
    rc = load().gpe_host_typed_hit_planes(_ptr(v), _ptr(lab), v.shape[0],
                                          len(lab), _ptr(out))
    if rc != 0:
        raise GpeError("gpe_host_typed_hit_planes failed (%d)" % rc)
    return out


def _check_planes(what, planes, n_cases):
    units = (int(n_cases) + 31) // 32
    planes = np.ascontiguousarray(planes, dtype=np.uint32)
    if n_cases < 1 or planes.ndim != 2 or planes.shape[1] != units:
        raise ValueError("%s: planes must be uint32 [n, %d] for %d cases"
                         % (what, units, n_cases))
    return planes


def host_informed_cases(planes, n_cases, seed, m):
    """Host twin of :meth:`Context.informed_cases` (CPU, no GPU): the
    farthest-first subset of *m* cases of a program-major hit matrix
    ``uint32[n, ceil(n_cases / 32)]`` → ``(idx int64[m], dist int32[m])``."""
    planes = _check_planes("host_informed_cases", planes, n_cases)
    idx = np.zeros(max(int(m), 1), dtype=np.int64)
    dist = np.zeros(max(int(m), 1), dtype=np.int32)
    rc = load().gpe_host_informed_cases(
        _ptr(planes), planes.shape[0], int(n_cases),
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(m), _ptr(idx), _ptr(dist))
    if rc != 0:
        raise GpeError("gpe_host_informed_cases failed (%d)" % rc)
    return idx[:int(m)], dist[:int(m)]


def host_hit_threshold(cases, eps):
    """Host twin of the thresholding ``gpe_informed_cases`` applies to the F
    machine's per-case matrix (CPU, no GPU): ``cases[n, n_cases]`` float64 →
    hit planes ``uint32[n, ceil(n_cases / 32)]``, a bit set where the value is
    finite and ``<= eps``."""
    e = np.ascontiguousarray(np.atleast_2d(cases), dtype=np.float64)
    out = np.zeros((e.shape[0], (e.shape[1] + 31) // 32), dtype=np.uint32)
    rc = load().gpe_host_hit_threshold(_ptr(e), e.shape[0], e.shape[1],
                                       float(eps), _ptr(out))
    if rc != 0:
        raise GpeError("gpe_host_hit_threshold failed (%d)" % rc)
    return out


HIT_GROUPS_MAX = 8


def _check_group_masks(what, masks, n_cases):
    """The masks of a hit_group_counts call as uint32 ``[G, n_units]``."""
    units = (int(n_cases) + 31) // 32
    masks = np.ascontiguousarray(masks, dtype=np.uint32)
    if masks.ndim != 2 or masks.shape[1] != units:
        raise ValueError("%s: masks must be uint32 [G, %d] for %d cases"
                         % (what, units, n_cases))
    return masks


def host_hit_group_counts(planes, n_cases, masks):
    """Host twin of :meth:`Context.hit_group_counts` (CPU, no GPU): a
    program-major hit matrix ``uint32[n, ceil(n_cases / 32)]`` and masks
    ``uint32[G, ceil(n_cases / 32)]`` → ``int64[n, G]``,
    ``popcount(row & mask)`` with the masks' pad bits cleared."""
    planes = _check_planes("host_hit_group_counts", planes, n_cases)
    masks = _check_group_masks("host_hit_group_counts", masks, n_cases)
    n, G = planes.shape[0], masks.shape[0]
    out = np.zeros((n, max(G, 1)), dtype=np.int32)
    rc = load().gpe_host_hit_group_counts(
        _ptr(planes) if n else None, n, int(n_cases), _ptr(masks), G,
        _ptr(out) if n else None)
    if rc != 0:
        raise GpeError("gpe_host_hit_group_counts failed (%d)" % rc)
    return out[:, :G].astype(np.int64)


HIT_WEIGHTS_MAX = 8


def check_case_weights(what, weights, n_cases):
    """The weights of a weighted-hits call as float64 ``[G, n_cases]``
    (``-0.0`` as ``0.0``): 1-D or 2-D, every weight finite and ``>= 0``,
    ``math.fsum`` of every row finite; ``ValueError`` otherwise."""
    try:
        w = np.array(weights, dtype=np.float64, order="C", ndmin=2)
    except (TypeError, ValueError):
        raise ValueError("%s: weights must be a float array [n_cases] or "
                         "[G, n_cases]" % what)
    if w.ndim != 2 or w.shape[1] != int(n_cases):
        raise ValueError("%s: weights must be float64 [%d] or [G, %d] (got "
                         "shape %r)" % (what, n_cases, n_cases,
                                        np.shape(weights)))
    if not np.isfinite(w).all():
        raise ValueError("%s: every weight must be finite (got a nan or an "
                         "inf)" % what)
    if (w < 0.0).any():
        raise ValueError("%s: every weight must be >= 0 (got %r)"
                         % (what, float(w[w < 0.0][0])))
    w += 0.0                                      # (-0.0 + 0.0 is +0.0)
    for g in range(w.shape[0]):
        # (fsum only where the sum can be near the top of the range)
        if float(w[g].max(initial=0.0)) * w.shape[1] >= 1e308:
            try:
                total = math.fsum(w[g].tolist())
            except OverflowError:
                total = math.inf
            if not math.isfinite(total):
                raise ValueError("%s: the sum of weights[%d] overflows a "
                                 "float" % (what, g))
    return w


def pack_live_mask(live):
    """``bool[n]`` → uint64 ``[ceil(n / 64)]``, individual i at bit i % 64 of
    word i / 64 (the live mask of the solve counts)."""
    live = np.ascontiguousarray(live, dtype=bool)
    by = np.packbits(live, bitorder="little")
    out = np.zeros((len(live) + 63) // 64 * 8, dtype=np.uint8)
    out[:len(by)] = by
    return out.view("<u8").astype(np.uint64)


def _check_live(what, live, n):
    if live is None:
        return None
    live = np.ascontiguousarray(live, dtype=np.uint64)
    if live.shape != ((int(n) + 63) // 64,):
        raise ValueError("%s: live must be uint64 [%d] for %d individuals"
                         % (what, (int(n) + 63) // 64, n))
    return live


def host_case_solve_counts(planes, n_cases, live=None):
    """Host twin of :meth:`Context.case_solve_counts` (CPU, no GPU): a
    program-major hit matrix ``uint32[n, ceil(n_cases / 32)]`` and an
    optional live mask ``uint64[ceil(n / 64)]`` → ``int64[n_cases]``."""
    planes = _check_planes("host_case_solve_counts", planes, n_cases)
    n = planes.shape[0]
    live = _check_live("host_case_solve_counts", live, n)
    out = np.zeros(int(n_cases), dtype=np.int32)
    rc = load().gpe_host_case_solve_counts(
        _ptr(planes) if n else None, n, int(n_cases), _ptr(live), _ptr(out))
    if rc != 0:
        raise GpeError("gpe_host_case_solve_counts failed (%d)" % rc)
    return out.astype(np.int64)


def host_hit_weighted_sums(planes, n_cases, weights, pair=False):
    """Host twin of :meth:`Context.hit_weighted_sums` (CPU, no GPU): the
    same double-double sum in the same order → ``float64[n, G]``; with
    *pair* ``(hi, lo)``, the final normalised pair."""
    planes = _check_planes("host_hit_weighted_sums", planes, n_cases)
    w = check_case_weights("host_hit_weighted_sums", weights, n_cases)
    n, G = planes.shape[0], w.shape[0]
    hi = np.zeros((max(n, 1), max(G, 1)), dtype=np.float64)
    lo = np.zeros_like(hi)
    rc = load().gpe_host_hit_weighted_sums(
        _ptr(planes) if n else None, n, int(n_cases), _ptr(w), G,
        _ptr(hi), _ptr(lo))
    if rc != 0:
        raise GpeError("gpe_host_hit_weighted_sums failed (%d)" % rc)
    hi, lo = hi[:n, :G], lo[:n, :G]
    return (hi, lo) if pair else hi


def host_hit_shared_sums(planes, n_cases, live=None, pair=False):
    """Host twin of :meth:`Context.hit_shared_sums` (CPU, no GPU) →
    ``(counts int64[n_cases], sums float64[n])``; with *pair* the sums are
    ``(hi, lo)``."""
    planes = _check_planes("host_hit_shared_sums", planes, n_cases)
    n = planes.shape[0]
    live = _check_live("host_hit_shared_sums", live, n)
    cnt = np.zeros(int(n_cases), dtype=np.int32)
    hi = np.zeros(max(n, 1), dtype=np.float64)
    lo = np.zeros_like(hi)
    rc = load().gpe_host_hit_shared_sums(
        _ptr(planes) if n else None, n, int(n_cases), _ptr(live), _ptr(cnt),
        _ptr(hi), _ptr(lo))
    if rc != 0:
        raise GpeError("gpe_host_hit_shared_sums failed (%d)" % rc)
    hi, lo = hi[:n], lo[:n]
    return cnt.astype(np.int64), ((hi, lo) if pair else hi)


def lexicase_par_lds_values():
    """The number of compacted candidate values a ``gpe_lexicase_par`` block
    keeps in LDS (larger candidate sets go through device scratch)."""
    return int(load().gpe_lexicase_par_lds_values())


def _check_lexicase_par(what, n, n_cases, k, mode):
    if n < 1 or n > 2 ** 31 - 1:
        raise ValueError("%s: n = %d individuals (need 1 .. 2^31 - 1)"
                         % (what, n))
    if n_cases < 1 or n_cases > 2 ** 31 - 1:
        raise ValueError("%s: n_cases = %d (need 1 .. 2^31 - 1)"
                         % (what, n_cases))
    if k < 0:
        raise ValueError("%s: k = %d selections (need >= 0)" % (what, k))
    if mode not in (0, 1, 2):
        raise ValueError("%s: mode must be 0, 1 or 2 (got %r)" % (what, mode))


def host_lexicase_par(values, maximise, k, seed, mode=0, epsilon=0.0):
    """Host twin of :meth:`Context.lexicase_par` (CPU, no GPU): the rule of
    ``gpe_lexicase_par`` in plain C++ on ``values`` [n, n_cases] →
    ``(indices int32[k], failed)``: -1 where a selection ended with no
    candidate, *failed* the first such selection or -1.  ``ValueError`` for
    what the library refuses: an empty matrix, ``k < 0``, a mode outside
    0..2, a *maximise* of another length."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    if values.ndim != 2:
        raise ValueError("host_lexicase_par: values must be [n, n_cases] "
                         "(got %d dimensions)" % values.ndim)
    n, c = values.shape
    k, mode = int(k), int(mode)
    _check_lexicase_par("host_lexicase_par", n, c, k, mode)
    maximise = np.ascontiguousarray(maximise, dtype=np.uint8)
    if maximise.shape != (c,):
        raise ValueError("host_lexicase_par: maximise must have one entry per "
                         "case (%d), got shape %r" % (c, maximise.shape))
    out = np.zeros(max(k, 1), dtype=np.int32)
    failed = ctypes.c_int64(-1)
    rc = load().gpe_host_lexicase_par(
        _ptr(values), n, c, _ptr(maximise), mode, float(epsilon),
        int(seed) & 0xFFFFFFFFFFFFFFFF, k, _ptr(out), ctypes.byref(failed))
    if rc != 0:
        raise GpeError("gpe_host_lexicase_par failed (%d)" % rc)
    return out[:k], failed.value


_U64 = 0xFFFFFFFFFFFFFFFF


def _check_dalex(what, n, n_cases, k, pressure, k_name="k selections"):
    """The sizes and the pressure of a DALex call, in the library's words."""
    if n < 1 or n > 2 ** 31 - 1:
        raise ValueError("%s: n = %d individuals (need 1 .. 2^31 - 1)"
                         % (what, n))
    if n_cases < 1 or n_cases > 2 ** 31 - 1:
        raise ValueError("%s: n_cases = %d (need 1 .. 2^31 - 1)"
                         % (what, n_cases))
    if k < 0 or k > 2 ** 31 - 1:
        raise ValueError("%s: %s = %d (need 0 .. 2^31 - 1)"
                         % (what, k_name, k))
    if pressure is not None and \
            not (pressure >= 0.0 and math.isfinite(pressure)):
        raise ValueError("%s: pressure must be finite and >= 0 (got %r)"
                         % (what, pressure))


def _dalex_values(what, values):
    values = np.ascontiguousarray(values, dtype=np.float64)
    if values.ndim != 2:
        raise ValueError("%s: values must be [n, n_cases] (got %d "
                         "dimensions)" % (what, values.ndim))
    return values


def _dalex_sigma_arg(what, sigma, n_cases):
    if sigma is None:
        return None
    sigma = np.ascontiguousarray(sigma, dtype=np.float64)
    if sigma.shape != (int(n_cases),):
        raise ValueError("%s: sigma must have one entry per case (%d), got "
                         "shape %r" % (what, n_cases, sigma.shape))
    return sigma


def host_dalex_weights(n_cases, k, seed, pressure, sigma=None):
    """Host twin of :meth:`Context.dalex_weights` (CPU, no GPU): steps 1 - 4
    of the DALex rule (include/gpeval.h) in plain C++ with libm →
    ``float64[n_cases, k]``, case-major: column *s* holds selection *s*'s
    effective weights.  *sigma* ``[n_cases]`` standardises (a zero gives
    weight 0); None leaves the softmax weights."""
    n_cases, k, pressure = int(n_cases), int(k), float(pressure)
    _check_dalex("host_dalex_weights", 1, n_cases, k, pressure)
    sigma = _dalex_sigma_arg("host_dalex_weights", sigma, n_cases)
    out = np.zeros((n_cases, max(k, 1)), dtype=np.float64)
    rc = load().gpe_host_dalex_weights(n_cases, k, int(seed) & _U64, pressure,
                                       _ptr(sigma), _ptr(out))
    if rc != 0:
        raise GpeError("gpe_host_dalex_weights failed (%d)" % rc)
    return out if k else out[:, :0]


def host_dalex_sigma(values):
    """Host twin of :meth:`Context.dalex_sigma` (CPU, no GPU): each case's
    population standard deviation over the fit rows of *values*
    ``[n, n_cases]`` (step 4 of the rule) → ``float64[n_cases]``."""
    values = _dalex_values("host_dalex_sigma", values)
    n, c = values.shape
    _check_dalex("host_dalex_sigma", n, c, 0, None)
    out = np.zeros(c, dtype=np.float64)
    rc = load().gpe_host_dalex_sigma(_ptr(values), n, c, _ptr(out))
    if rc != 0:
        raise GpeError("gpe_host_dalex_sigma failed (%d)" % rc)
    return out


def host_dalex(values, k, seed, pressure, standardize=True):
    """Host twin of :meth:`Context.dalex` (CPU, no GPU): the DALex rule of
    include/gpeval.h on *values* ``[n, n_cases]`` (non-negative errors), every
    score summed in ascending case order in fp64 → ``(indices int32[k],
    failed)``: -1 where no row is fit, *failed* the first such selection or
    -1.  ``ValueError`` for what the library refuses: an empty matrix,
    ``k < 0``, a *pressure* that is negative, nan or infinite."""
    values = _dalex_values("host_dalex", values)
    n, c = values.shape
    k, pressure = int(k), float(pressure)
    _check_dalex("host_dalex", n, c, k, pressure)
    out = np.zeros(max(k, 1), dtype=np.int32)
    failed = ctypes.c_int64(-1)
    rc = load().gpe_host_dalex(_ptr(values), n, c, int(seed) & _U64, pressure,
                               1 if standardize else 0, k, _ptr(out),
                               ctypes.byref(failed))
    if rc != 0:
        raise GpeError("gpe_host_dalex failed (%d)" % rc)
    return out[:k], failed.value


ND_SORT_MAX_OBJECTIVES = 32


def _nd_sort_args(what, w, mult, k):
    """The arguments of a non-dominated sort, checked in the library's words
    → ``(w float64[n, m], mult int32[n] or None, k)``."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.ndim != 2:
        raise ValueError("%s: w must be [n, m] (got %d dimensions)"
                         % (what, w.ndim))
    n, m = w.shape
    if n < 1 or n > 2 ** 31 - 1:
        raise ValueError("%s: n = %d rows (need 1 .. 2^31 - 1)" % (what, n))
    if m < 1 or m > ND_SORT_MAX_OBJECTIVES:
        raise ValueError("%s: m = %d objectives (need 1 .. %d)"
                         % (what, m, ND_SORT_MAX_OBJECTIVES))
    k = int(k)
    if k < 0:
        raise ValueError("%s: k = %d (need >= 0)" % (what, k))
    if mult is not None:
        mult = np.ascontiguousarray(mult, dtype=np.int32)
        if mult.shape != (n,):
            raise ValueError("%s: mult must have one entry per row (%d), got "
                             "shape %r" % (what, n, mult.shape))
    return w, mult, k


def _nd_sort_result(order, front_end, n_fronts):
    """``order`` cut at ``front_end`` → a list of int32 arrays, one a front."""
    ends = front_end[:n_fronts].tolist()
    return [order[a:b].copy() for a, b in zip([0] + ends[:-1], ends)]


def host_nd_sort(w, k, mult=None, first_front_only=False):
    """Host twin of :meth:`Context.nd_sort` (CPU, no GPU): the non-dominated
    sorting rule of include/gpeval.h in plain C++ → a list of int32 arrays,
    the rows of each front in the rule's order.  ``ValueError`` for what the
    library refuses: an empty matrix, m outside 1 .. 32, ``k < 0``, a nan, a
    multiplicity below 1."""
    w, mult, k = _nd_sort_args("host_nd_sort", w, mult, k)
    n, m = w.shape
    order = np.zeros(n, dtype=np.int32)
    front_end = np.zeros(n, dtype=np.int64)
    nf, nr = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = load().gpe_host_nd_sort(_ptr(w), _ptr(mult), n, m, k,
                                 1 if first_front_only else 0, _ptr(order),
                                 _ptr(front_end), ctypes.byref(nf),
                                 ctypes.byref(nr))
    if rc == GPE_E_ARG:
        raise ValueError("host_nd_sort: a nan in w or a multiplicity < 1")
    if rc != 0:
        raise GpeError("gpe_host_nd_sort failed (%d)" % rc)
    return _nd_sort_result(order, front_end, nf.value)


TRIG_CLASSES =("general", "mid", "small")
# the classes GPE_TRIG_RANGES=2 and 3 (the default) pick handlers by
TRIG_PICKED = TRIG_CLASSES + ("midlo", "wide")


def _trig_pass(fn, words, lo, hi, mode):
    """One of the library's two range-pass diagnostics over one program."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    assert lo.shape == hi.shape and lo.ndim == 1
    out = np.zeros(max(len(words), 1), dtype=np.int32)
    n = fn(_ptr(words), len(words), _ptr(lo), _ptr(hi), len(lo), int(mode), _ptr(out), len(out))
    if n < 0:
        raise GpeError("gpe_debug_trig_classes: malformed program or unknown mode")
    return out[:n]


def debug_trig_classes(words, lo, hi, mode=1):
    """Host-only: the range pass (csrc/trig_ranges.h) over one program's
    flattener words with column bounds lo[v], hi[v]: the class index of each
    sin/cos node, in word order.  ``mode`` 1: the base classes
    (``TRIG_CLASSES``); 2: ``TRIG_PICKED``, midlo a cos class.  (This entry
    point's contract stops at mode 2; mode 3: ``debug_trig_picks``.)"""
    return _trig_pass(load().gpe_debug_trig_classes_mode, words, lo, hi, mode)


def debug_trig_picks(words, lo, hi, mode=3):
    """``debug_trig_classes`` for every mode of the pass: 1, 2, 3, the
    library's default — mode 2's classes with midlo for a sin node too — and
    4 (mode 2's classes; mode 3's handlers in ``debug_translate``)."""
    return _trig_pass(load().gpe_debug_trig_picks, words, lo, hi, mode)


def debug_translate(batch, nv, table, bounds=None, mode=1):
    """Host-only: threaded code the asm core would run (see header).
    ``bounds`` = (lo, hi) per column: the exact cores' translation, sin/cos
    words by proven range (gpe_debug_translate_mode; ``mode`` as
    ``debug_trig_classes``)."""
    lib = load()
    code = np.ascontiguousarray(batch.code, dtype=np.uint32)
    off = np.ascontiguousarray(batch.offsets, dtype=np.int64)
    depth = np.ascontiguousarray(batch.depth, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.uint32)
    # (every program starts on a 16-word window)
    cap = 3 * len(code) + 16 * (len(depth) + 1)
    out = np.zeros(cap, dtype=np.uint32)
    starts = np.zeros(len(depth), dtype=np.int64)
    n_out = ctypes.c_int64()
    lo = hi = None
    if bounds is not None:
        lo = np.ascontiguousarray(bounds[0], dtype=np.float64)
        hi = np.ascontiguousarray(bounds[1], dtype=np.float64)
        assert len(lo) == len(hi) == int(nv)
    rc = lib.gpe_debug_translate_mode(
        _ptr(code), len(code), _ptr(off), len(depth), _ptr(depth), int(nv),
        _ptr(table), len(table), _ptr(out), cap, _ptr(starts),
        ctypes.byref(n_out), None if lo is None else _ptr(lo),
        None if hi is None else _ptr(hi), int(mode))
    if rc != 0:
        raise GpeError("gpe_debug_translate failed (%d)" % rc)
    return out[:n_out.value], starts


def _int_rows(ints):
    """(words, off, n) of an exact pass's int table (flatten.IntTable)."""
    if ints is None or not len(ints):
        return (np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int64), 0)
    return (np.ascontiguousarray(ints.words, dtype=np.uint32),
            np.ascontiguousarray(ints.off, dtype=np.int64), len(ints))


def _exact_raise(rc, name):
    if rc == GPE_ERR_VALUE:
        raise ValueError("math domain error")
    if rc == GPE_ERR_OVERFLOW:
        raise OverflowError("int too large to convert to float")
    if rc == GPE_ERR_XINT_RANGE:
        from .flatten import ExactIntRangeError
        raise ExactIntRangeError("an int past the device's 1088 bits")
    if rc != 0:
        raise GpeError("%s failed (%d)" % (name, rc))


def _twos(words):
    bits = 32 * len(words)
    u = sum(int(w) << (32 * i) for i, w in enumerate(words))
    return u - (1 << bits) if bits and u >> (bits - 1) else u


def host_exact_eval(code, ints, x):
    """Host twin of the exact pass's device interpreter (test
    infrastructure, CPU): one program of Flattener.exact_programs on one
    case ``x``.  Returns the Python number the reference's evaluation gives
    (an int or a float), or raises what it raises: ValueError for sin/cos of
    an infinity, OverflowError for float(int) or int / int past the float
    range — and ExactIntRangeError where an int passes the device's 1088
    bits (the library then evaluates the program with host_bigint_eval's
    code)."""
    code = np.ascontiguousarray(code, dtype=np.uint32)
    words, off, n = _int_rows(ints)
    x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
    f = ctypes.c_double()
    out = np.zeros(GPE_XINT_WORDS, dtype=np.uint32)
    isint = _I()
    rc = load().gpe_host_exact_eval(_ptr(code), _ptr(words), _ptr(off), n,
                                    _ptr(x), len(x), ctypes.byref(f),
                                    _ptr(out), ctypes.byref(isint))
    _exact_raise(rc, "gpe_host_exact_eval")
    return _twos(out.tolist()) if isint.value else f.value


def host_bigint_eval(code, ints, x):
    """The exact pass's host evaluator with unbounded ints (the one the
    library runs for programs past the device's 1088 bits), on one case:
    the Python number or the exception, as host_exact_eval."""
    code = np.ascontiguousarray(code, dtype=np.uint32)
    words, off, n = _int_rows(ints)
    x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
    f = ctypes.c_double()
    isint = _I()
    cap = ctypes.c_int64(64)
    lib = load()
    while True:
        out = np.zeros(max(cap.value, 1), dtype=np.uint32)
        want = cap.value
        rc = lib.gpe_host_bigint_eval(_ptr(code), _ptr(words), _ptr(off), n,
                                      _ptr(x), len(x), ctypes.byref(f),
                                      _ptr(out), ctypes.byref(cap),
                                      ctypes.byref(isint))
        if rc == GPE_E_INVALID and cap.value > want:
            continue                          # a wider int: again, with room
        break
    _exact_raise(rc, "gpe_host_bigint_eval")
    return _twos(out[:cap.value].tolist()) if isint.value else f.value


def comm_unique_id():
    """The communicator id rank 0 creates (gpe_comm_unique_id): bytes."""
    buf = ctypes.create_string_buffer(GPE_UNIQUE_ID_BYTES)
    rc = load().gpe_comm_unique_id(buf)
    if rc != 0:
        raise GpeError("gpe_comm_unique_id failed (%d): is librccl.so.1 "
                       "available?" % rc)
    return buf.raw


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class _Buffers(object):
    """Output arrays kept across calls (grown, never shrunk): a fresh
    million-entry array per call is fresh pages, and their first-touch
    faults (and the unmapping when Python frees them) were ~3 ms of an
    ``evaluate`` at pop 1M.  The caller owns the contents only until its
    next call with the same buffers."""
    dtypes = ()

    def __init__(self):
        self._arrays = [np.zeros(0, dtype=d) for d in self.dtypes]

    def views(self, n):
        if len(self._arrays[0]) < n:
            cap = max(n, 2 * len(self._arrays[0]))
            self._arrays = [np.zeros(cap, dtype=d) for d in self.dtypes]
        return tuple(a[:n] for a in self._arrays)


class ResultBuffers(_Buffers):
    """(hi, lo, err, flags) of :meth:`Context.run`."""
    dtypes = (np.float64, np.float64, np.uint64, np.uint32)


class LoweringBuffers(_Buffers):
    """(depth, err, status) of :meth:`Context.lower_programs`."""
    dtypes = (np.int32, np.uint8, np.uint8)


class Context(object):
    """One device context (one per process/GPU)."""

    def __init__(self, device=0):
        self.lib = load()
        handle = ctypes.c_void_p()
        rc = self.lib.gpe_create(int(device), ctypes.byref(handle))
        if rc != 0:
            raise GpeError("gpe_create(%d) failed with %d" % (device, rc))
        self.h = handle
        self.device = device
        self.machine = None
        self.n_prog = 0
        self.n_cases = 0
        # the ProgramBatch whose programs are loaded (identity; None after a
        # device lowering until its caller names the batch it built)
        self.resident = None
        # an open chunked lowering: its tree count, and the output arrays
        # gpe_lower_begin_into was given (None: outputs at lower_end)
        self._lw_n = 0
        self._lw_into = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.gpe_last_error(self.h)
            raise GpeError("%s failed (%d): %s" % (what, rc,
                                                   msg.decode() if msg else ""))

    def device_info(self):
        cu, clk = ctypes.c_int(), ctypes.c_int()
        name = ctypes.create_string_buffer(256)
        self._check(self.lib.gpe_device_info(self.h, ctypes.byref(cu),
                                             ctypes.byref(clk), name, 256),
                    "gpe_device_info")
        return {"cu": cu.value, "clock_khz": clk.value,
                "arch": name.value.decode()}

    def set_cases(self, machine, X, terms):
        X = np.ascontiguousarray(X)
        terms = None if terms is None else np.ascontiguousarray(terms)
        if machine == GPE_MACHINE_F:
            X = X.astype(np.float64, copy=False)
            n_vars, n_cases = X.shape
            if terms is not None:
                terms = terms.astype(np.float64, copy=False)
                if terms.ndim == 1:
                    terms = terms[None, :]
                assert terms.shape[1] == n_cases
            n_terms = 0 if terms is None else terms.shape[0]
        else:
            raise ValueError("use set_bitplanes for the B machine")
        self._check(self.lib.gpe_set_cases(self.h, machine, _ptr(X), n_vars,
                                           n_cases, _ptr(terms), n_terms),
                    "gpe_set_cases")
        self.machine = machine
        self.n_cases = int(n_cases)
        self._keep = (X, terms)

    def select_cases(self, idx):
        """gpe_select_cases: run on rows *idx* (int64, validated by the
        library) of the uploaded cases; None: the full set again.  The loaded
        programs stay loaded."""
        if idx is None:
            rc = self.lib.gpe_select_cases(self.h, None, 0)
        else:
            idx = np.ascontiguousarray(idx, dtype=np.int64)
            rc = self.lib.gpe_select_cases(self.h, _ptr(idx), len(idx))
        self._check(rc, "gpe_select_cases")
        self.n_cases = self.case_subset()[0]

    def case_subset(self):
        """gpe_case_subset → (active case count, full case count, whether a
        subset is active)."""
        m, full = ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.gpe_case_subset(self.h, ctypes.byref(m),
                                             ctypes.byref(full)),
                    "gpe_case_subset")
        return (m.value if m.value >= 0 else full.value, full.value,
                m.value >= 0)

    def set_trig_leaves(self, enable):
        """Device columns sin(x_v), cos(x_v) per run (see gpeval.h)."""
        self._check(self.lib.gpe_set_trig_leaves(self.h, int(bool(enable))),
                    "gpe_set_trig_leaves")
        self.n_prog = 0
        self.resident = None
        if self.machine is not None:      # (an active case subset is dropped)
            self.n_cases = self.case_subset()[0]

    def set_precision(self, prec):
        """GPE_PREC_F64 (default) or GPE_PREC_F32 for the F machine."""
        self._check(self.lib.gpe_set_precision(self.h, int(prec)),
                    "gpe_set_precision")

    def set_bitplanes(self, planes, out_plane, n_cases):
        planes = np.ascontiguousarray(planes, dtype=np.uint32)
        out_plane = np.ascontiguousarray(out_plane, dtype=np.uint32)
        self._check(self.lib.gpe_set_cases(self.h, GPE_MACHINE_B,
                                           _ptr(planes), planes.shape[0],
                                           int(n_cases), _ptr(out_plane), 1),
                    "gpe_set_cases")
        self.machine = GPE_MACHINE_B
        self.n_cases = int(n_cases)
        self._keep = (planes, out_plane)

    def load_programs(self, batch):
        code = np.ascontiguousarray(batch.code, dtype=np.uint32)
        off = np.ascontiguousarray(batch.offsets, dtype=np.int64)
        depth = np.ascontiguousarray(batch.depth, dtype=np.int32)
        self._check(self.lib.gpe_load_programs(self.h, _ptr(code), len(code),
                                               _ptr(off), len(depth),
                                               _ptr(depth)),
                    "gpe_load_programs")
        self.n_prog = len(depth)
        self.resident = batch

    def load_exact(self, progs, code, offsets, depth, ints):
        """gpe_load_exact_v: re-evaluate the loaded programs ``progs`` with
        Python-int semantics after every run (Flattener.exact_programs)."""
        progs = np.ascontiguousarray(progs, dtype=np.int32)
        code = np.ascontiguousarray(code, dtype=np.uint32)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        depth = np.ascontiguousarray(depth, dtype=np.int32)
        words, woff, n = _int_rows(ints)
        self._check(self.lib.gpe_load_exact_v(
            self.h, _ptr(progs), len(progs), _ptr(code), len(code), _ptr(off),
            _ptr(depth), _ptr(words), _ptr(woff), n), "gpe_load_exact_v")

    def lower_flags(self):
        """(trees with a nonzero error code, with a nonzero status) of the
        last device lowering (gpe_last_lower_flags)."""
        ne, ns = ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.gpe_last_lower_flags(self.h, ctypes.byref(ne), ctypes.byref(ns)),
                    "gpe_last_lower_flags")
        return ne.value, ns.value

    def exact_host_runs(self):
        """Exact-pass programs the last run evaluated on the host (ints past
        the device's 1088 bits)."""
        n = ctypes.c_int64()
        self._check(self.lib.gpe_last_exact_host_runs(self.h, ctypes.byref(n)),
                    "gpe_last_exact_host_runs")
        return n.value

    def exact_host_ms(self):
        """Wall time of the last run's host exact pass, ms."""
        ms = ctypes.c_double()
        self._check(self.lib.gpe_last_exact_host_ms(self.h, ctypes.byref(ms)),
                    "gpe_last_exact_host_ms")
        return ms.value

    def debug_shard_combine(self, parts, errs, flags, case_offsets):
        """gpe_debug_shard_combine (test infrastructure): the case-sharded
        combine of ``world`` ranks' outputs on this device.  parts
        [world, 2, n] float64, errs [world, n] uint64, flags [world, n]
        uint32, case_offsets [world]; returns (hi, lo, err, flags)."""
        parts = np.ascontiguousarray(parts, dtype=np.float64)
        errs = np.ascontiguousarray(errs, dtype=np.uint64)
        flags = np.ascontiguousarray(flags, dtype=np.uint32)
        offs = np.ascontiguousarray(case_offsets, dtype=np.int64)
        world, _, n = parts.shape
        hi, lo = np.zeros(n), np.zeros(n)
        err = np.zeros(n, dtype=np.uint64)
        fl = np.zeros(n, dtype=np.uint32)
        self._check(self.lib.gpe_debug_shard_combine(
            self.h, world, n, _ptr(parts), _ptr(errs), _ptr(flags), _ptr(offs),
            _ptr(hi), _ptr(lo), _ptr(err), _ptr(fl)), "gpe_debug_shard_combine")
        return hi, lo, err, fl

    def debug_redo_union(self, flags):
        """gpe_debug_redo_union (test infrastructure): redo flags other
        ranks raised, ORed into every later run's own (None clears)."""
        f = np.zeros(0, dtype=np.uint32) if flags is None else \
            np.ascontiguousarray(flags, dtype=np.uint32)
        self._check(self.lib.gpe_debug_redo_union(self.h, _ptr(f) if len(f) else None,
                                                  len(f)), "gpe_debug_redo_union")

    def run(self, mode, out=None, want=None):
        """gpe_run → (hi, lo, err, flags).  *out*: a :class:`ResultBuffers`
        to write into (views of its arrays are returned), else fresh arrays.
        *want*: the names of the outputs to copy back (default all); the
        others are returned as None (gpe_run's NULL outputs)."""
        n = self.n_prog
        if out is not None:
            arrs = list(out.views(n))
        else:
            arrs = [np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64),
                    np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)]
        if want is not None:
            arrs = [a if name in want else None
                    for a, name in zip(arrs, ("hi", "lo", "err", "flags"))]
        if n:
            self._check(self.lib.gpe_run(self.h, mode, *[
                _ptr(a) if a is not None else None for a in arrs]), "gpe_run")
        return tuple(arrs)

    def run_cases(self, mode, n_cases):
        """gpe_run plus the per-case terms ``[n_prog, n_cases]``."""
        n = self.n_prog
        cases = np.zeros((n, n_cases), dtype=np.float64)
        hi = np.zeros(n, dtype=np.float64)
        lo = np.zeros(n, dtype=np.float64)
        err = np.zeros(n, dtype=np.uint64)
        flags = np.zeros(n, dtype=np.uint32)
        if n:
            self._check(self.lib.gpe_run_cases(self.h, mode, _ptr(cases),
                                               _ptr(hi), _ptr(lo), _ptr(err),
                                               _ptr(flags)), "gpe_run_cases")
        return cases, hi, lo, err, flags

    def run_values(self, out=None):
        """gpe_run_values → (values float64 [n_prog, n_cases], err uint64
        [n_prog]): what each loaded program computes on each resident case
        (NaN at an erroring case) and its first erroring case.  *out*: a
        C-contiguous float64 array of that shape to write into."""
        n, nc = self.n_prog, self.n_cases
        if out is None:
            out = np.empty((n, nc), dtype=np.float64)
        if out.shape != (n, nc) or out.dtype != np.float64 or \
                not out.flags.c_contiguous:
            raise ValueError("run_values: out must be C-contiguous float64 "
                             "[%d, %d]" % (n, nc))
        err = np.full(n, GPE_NO_ERROR, dtype=np.uint64)
        self._check(self.lib.gpe_run_values(self.h, _ptr(out), _ptr(err)),
                    "gpe_run_values")
        return out, err

    def run_values_device(self, ptr, err_ptr=None):
        """gpe_run_values_device: the kernels write float64
        [n_prog, n_cases] at device address *ptr* (a torch tensor's
        ``data_ptr()``) and uint64 [n_prog] first errors at *err_ptr*."""
        self._check(self.lib.gpe_run_values_device(
            self.h, ctypes.c_void_p(int(ptr)),
            ctypes.c_void_p(int(err_ptr)) if err_ptr else None),
            "gpe_run_values_device")

    def run_moments(self):
        """gpe_run_moments → (moments float64 [n_prog, 6] = (Sf hi, lo,
        Sff hi, lo, Sfy hi, lo), err uint64 [n_prog], flags uint32
        [n_prog])."""
        n = self.n_prog
        m6 = np.zeros((n, 6), dtype=np.float64)
        err = np.full(n, GPE_NO_ERROR, dtype=np.uint64)
        flags = np.zeros(n, dtype=np.uint32)
        self._check(self.lib.gpe_run_moments(self.h, _ptr(m6), _ptr(err),
                                             _ptr(flags)), "gpe_run_moments")
        return m6, err, flags

    def run_scaled(self, sy, syy):
        """gpe_run_scaled → (mse, a, b float64 [n_prog], err uint64, flags
        uint32): the linear-scaling fitness of the loaded programs; *sy*,
        *syy*: the target's sum y and sum y^2 as (hi, lo)."""
        n = self.n_prog
        sy, syy = _dd(sy), _dd(syy)
        mse, a, b = np.zeros(n), np.zeros(n), np.zeros(n)
        err = np.full(n, GPE_NO_ERROR, dtype=np.uint64)
        flags = np.zeros(n, dtype=np.uint32)
        if n:
            self._check(self.lib.gpe_run_scaled(
                self.h, _ptr(sy), _ptr(syy), _ptr(mse), _ptr(a), _ptr(b),
                _ptr(err), _ptr(flags)), "gpe_run_scaled")
        return mse, a, b, err, flags

    def run_scaled_device(self, sy, syy, mse_ptr, a_ptr, b_ptr, err_ptr=None,
                          flags_ptr=None):
        """gpe_run_scaled_device: the results at device addresses (torch
        tensors' ``data_ptr()``)."""
        sy, syy = _dd(sy), _dd(syy)
        self._check(self.lib.gpe_run_scaled_device(
            self.h, _ptr(sy), _ptr(syy), *[
                ctypes.c_void_p(int(p)) if p else None
                for p in (mse_ptr, a_ptr, b_ptr, err_ptr, flags_ptr)]),
            "gpe_run_scaled_device")

    def run_abserr(self, hit_eps):
        """gpe_run_abserr → (out4 float64 [n_prog, 4] = (sum |d| hi, lo,
        max |d|, hits), err uint64 [n_prog], flags uint32 [n_prog])."""
        n = self.n_prog
        out4 = np.zeros((n, 4), dtype=np.float64)
        err = np.full(n, GPE_NO_ERROR, dtype=np.uint64)
        flags = np.zeros(n, dtype=np.uint32)
        if n:
            self._check(self.lib.gpe_run_abserr(
                self.h, float(hit_eps), _ptr(out4), _ptr(err), _ptr(flags)),
                "gpe_run_abserr")
        return out4, err, flags

    def run_abserr_cases(self, hit_eps, n_cases, want_cases=True):
        """gpe_run_abserr_cases → (cases float64 [n_prog, n_cases] or None,
        out4, err, flags): :meth:`run_abserr` that also leaves each case's
        ``|d|`` in the context's per-case matrix (``lexicase(None, ...)``
        selects on it).  *want_cases* False: no host copy of the matrix is
        made or allocated."""
        n = self.n_prog
        cases = np.zeros((n, n_cases), dtype=np.float64) if want_cases \
            else None
        out4 = np.zeros((n, 4), dtype=np.float64)
        err = np.full(n, GPE_NO_ERROR, dtype=np.uint64)
        flags = np.zeros(n, dtype=np.uint32)
        if n:
            if n_cases != self.n_cases:
                raise ValueError("run_abserr_cases: the context holds %d "
                                 "cases, not %d" % (self.n_cases, n_cases))
            self._check(self.lib.gpe_run_abserr_cases(
                self.h, float(hit_eps),
                _ptr(cases) if want_cases else None, _ptr(out4), _ptr(err),
                _ptr(flags)), "gpe_run_abserr_cases")
        return cases, out4, err, flags

    def run_abserr_device(self, hit_eps, out4_ptr, err_ptr=None,
                          flags_ptr=None):
        """gpe_run_abserr_device: the results at device addresses (torch
        tensors' ``data_ptr()``)."""
        self._check(self.lib.gpe_run_abserr_device(
            self.h, float(hit_eps), *[
                ctypes.c_void_p(int(p)) if p else None
                for p in (out4_ptr, err_ptr, flags_ptr)]),
            "gpe_run_abserr_device")

    def run_values_bits(self):
        """gpe_run_values_bits → uint32 [n_prog, ceil(n_cases / 32)]: the B
        machine's result planes (pad bits 0)."""
        n = self.n_prog
        planes = np.zeros((n, (self.n_cases + 31) // 32), dtype=np.uint32)
        self._check(self.lib.gpe_run_values_bits(self.h, _ptr(planes)),
                    "gpe_run_values_bits")
        return planes

    def lexicase(self, values, maximise, k, rng, mode=0, epsilon=0.0):
        """gpe_lexicase: k selections on ``values`` [n, n_cases] (None: the
        last run_cases / run_abserr_cases matrix), drawing from the ``random.Random``-compatible
        ``rng`` exactly as the reference does and advancing its state.
        Returns (indices, failed): failed is -1 or the selection at which no
        candidate was left (the reference's IndexError)."""
        version, words, gauss = rng.getstate()
        st = np.asarray(words, dtype=np.uint32)
        maximise = np.ascontiguousarray(maximise, dtype=np.uint8)
        if values is None:
            n, c, ptr = 0, len(maximise), None
        else:
            values = np.ascontiguousarray(values, dtype=np.float64)
            n, c = values.shape
            ptr = _ptr(values)
        out = np.zeros(max(int(k), 1), dtype=np.int32)
        failed = ctypes.c_int64(-1)
        self._check(self.lib.gpe_lexicase(self.h, ptr, n, c, _ptr(maximise),
                                          int(mode), float(epsilon),
                                          _ptr(st), int(k), _ptr(out),
                                          ctypes.byref(failed)),
                    "gpe_lexicase")
        rng.setstate((version, tuple(int(w) for w in st), gauss))
        done = int(k) if failed.value < 0 else failed.value
        return out[:done], failed.value

    def run_hit_planes(self, want_planes=True):
        """gpe_run_hit_planes → (planes uint32 [n_prog, ceil(n_cases / 32)]
        or None, hits float64 [n_prog]): a HITS_BITS run that also leaves
        every program's hit plane on the device (``lexicase_bits(None, ...)``
        selects on it).  *want_planes* False: no host copy of the matrix is
        made or allocated."""
        n = self.n_prog
        units = (self.n_cases + 31) // 32
        planes = np.zeros((n, units), dtype=np.uint32) if want_planes \
            else None
        hits = np.zeros(n, dtype=np.float64)
        # (with no programs too: the library then drops its matrix)
        self._check(self.lib.gpe_run_hit_planes(
            self.h, _ptr(planes) if want_planes and n else None,
            _ptr(hits) if n else None, None, None), "gpe_run_hit_planes")
        return planes, hits

    def run_typed_hit_planes(self, want_planes=True, want_err=True):
        """gpe_run_typed_hit_planes → (planes uint32 [n_prog,
        ceil(n_cases / 32)] or None, hits float64 [n_prog], first_err uint64
        [n_prog] or None): a HITS_BOOL run of the F machine that also leaves
        every program's hit plane on the device.  *want_planes* /
        *want_err* False: no host copy of the matrix / the error words is
        made or allocated."""
        n = self.n_prog
        units = (self.n_cases + 31) // 32
        planes = np.zeros((n, units), dtype=np.uint32) if want_planes \
            else None
        hits = np.zeros(n, dtype=np.float64)
        err = np.zeros(n, dtype=np.uint64) if want_err else None
        self._check(self.lib.gpe_run_typed_hit_planes(
            self.h, _ptr(planes) if want_planes and n else None,
            _ptr(hits) if n else None, _ptr(err) if want_err and n else None,
            None),
            "gpe_run_typed_hit_planes")
        return planes, hits, err

    def hit_planes(self, n):
        """gpe_read_hit_planes → uint32 [n, ceil(n_cases / 32)]: the bit
        matrix the last run_hit_planes (of *n* programs) left on the
        device."""
        planes = np.zeros((int(n), (self.n_cases + 31) // 32), dtype=np.uint32)
        self._check(self.lib.gpe_read_hit_planes(self.h, _ptr(planes)),
                    "gpe_read_hit_planes")
        return planes

    def lexicase_bits(self, planes, n, n_cases, k, rng):
        """gpe_lexicase_bits: k lexicase selections on 0/1 values, every case
        maximised.  *planes*: a program-major hit matrix uint32
        [n, ceil(n_cases / 32)], or None for the last run_hit_planes' matrix
        on the device (*n*, *n_cases* are then the context's).  Draws from
        the ``random.Random``-compatible *rng* as the reference does and
        advances its state.  Returns (indices, failed) as :meth:`lexicase`."""
        version, words, gauss = rng.getstate()
        st = np.asarray(words, dtype=np.uint32)
        rows, n, n_cases, cases, ptr, keep = self._planes_arg(
            "lexicase_bits", planes, n, n_cases)
        out = np.zeros(max(int(k), 1), dtype=np.int32)
        failed = ctypes.c_int64(-1)
        self._check(self.lib.gpe_lexicase_bits(self.h, ptr, n, n_cases,
                                               _ptr(st), int(k), _ptr(out),
                                               ctypes.byref(failed)),
                    "gpe_lexicase_bits")
        rng.setstate((version, tuple(int(w) for w in st), gauss))
        done = int(k) if failed.value < 0 else failed.value
        return out[:done], failed.value

    def lexicase_par(self, values, maximise, k, seed, mode=0, epsilon=0.0):
        """gpe_lexicase_par: k independent selections on ``values``
        [n, n_cases] (None: the last run_cases / run_abserr_cases matrix), one
        workgroup each; case orders and choices are SplitMix64 keys of the
        64-bit *seed* (the rule: include/gpeval.h), no ``random`` draw is
        made.  Returns (indices int32[k], failed): -1 where a selection ended
        with no candidate, *failed* the first such selection or -1."""
        maximise = np.ascontiguousarray(maximise, dtype=np.uint8)
        if values is None:
            n, c, ptr = 0, len(maximise), None
        else:
            values = np.ascontiguousarray(values, dtype=np.float64)
            n, c = values.shape
            ptr = _ptr(values)
            if maximise.shape != (c,):
                raise ValueError("lexicase_par: maximise must have one entry "
                                 "per case (%d)" % c)
        out = np.zeros(max(int(k), 1), dtype=np.int32)
        failed = ctypes.c_int64(-1)
        self._check(self.lib.gpe_lexicase_par(
            self.h, ptr, n, c, _ptr(maximise), int(mode), float(epsilon),
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(k), _ptr(out),
            ctypes.byref(failed)), "gpe_lexicase_par")
        return out[:int(k)], failed.value

    def lexicase_bits_par(self, planes, n, n_cases, k, seed):
        """gpe_lexicase_bits_par: :meth:`lexicase_par`'s rule on 0/1 hits,
        every case maximised.  *planes* as :meth:`lexicase_bits` takes them
        (None: the last run_hit_planes' matrix on the device)."""
        rows, n, n_cases, cases, ptr, keep = self._planes_arg(
            "lexicase_bits_par", planes, n, n_cases)
        out = np.zeros(max(int(k), 1), dtype=np.int32)
        failed = ctypes.c_int64(-1)
        self._check(self.lib.gpe_lexicase_bits_par(
            self.h, ptr, n, n_cases,
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(k), _ptr(out),
            ctypes.byref(failed)), "gpe_lexicase_bits_par")
        return out[:int(k)], failed.value

    def _values_arg(self, what, values):
        """The *values* argument of the DALex calls → ``(rows, cases, n,
        n_cases, ptr, keep)``: None is the resident per-case matrix, whose
        sizes the library knows."""
        if values is None:
            return self.n_prog, self.n_cases, 0, 0, None, None
        values = _dalex_values(what, values)
        n, c = values.shape
        return n, c, n, c, _ptr(values), values

    def dalex(self, values, k, seed, pressure, standardize=True):
        """gpe_dalex: k DALex selections (the rule: include/gpeval.h) on
        ``values`` [n, n_cases] of non-negative errors (None: the last
        run_cases / run_abserr_cases matrix) — weights on the device, one fp64
        MFMA product with a fused argmin; no ``random`` draw is made.  Returns
        (indices int32[k], failed): -1 where no row is fit, *failed* the first
        such selection or -1.  Cost grows as n * n_cases * k."""
        rows, cases, n, c, ptr, keep = self._values_arg("dalex", values)
        out = np.zeros(max(int(k), 1), dtype=np.int32)
        failed = ctypes.c_int64(-1)
        self._check(self.lib.gpe_dalex(
            self.h, ptr, n, c, int(seed) & _U64, float(pressure),
            1 if standardize else 0, int(k), _ptr(out),
            ctypes.byref(failed)), "gpe_dalex")
        return out[:int(k)], failed.value

    def dalex_bits(self, planes, n, n_cases, k, seed, pressure,
                   standardize=True):
        """gpe_dalex_bits: :meth:`dalex` on 0/1 hits with error ``1 - hit``.
        *planes* as :meth:`lexicase_bits` takes them (None: the resident hit
        planes)."""
        rows, n, n_cases, cases, ptr, keep = self._planes_arg(
            "dalex_bits", planes, n, n_cases)
        out = np.zeros(max(int(k), 1), dtype=np.int32)
        failed = ctypes.c_int64(-1)
        self._check(self.lib.gpe_dalex_bits(
            self.h, ptr, n, n_cases, int(seed) & _U64, float(pressure),
            1 if standardize else 0, int(k), _ptr(out),
            ctypes.byref(failed)), "gpe_dalex_bits")
        return out[:int(k)], failed.value

    def dalex_weights(self, n_cases, k, seed, pressure, sigma=None):
        """gpe_dalex_weights → ``float64[n_cases, k]``: the effective weights
        the device makes for k selections, case-major (column *s* is
        selection *s*).  *sigma* ``[n_cases]`` standardises
        (:meth:`dalex_sigma` gives the device's); None: the softmax
        weights."""
        n_cases, k = int(n_cases), int(k)
        sigma = _dalex_sigma_arg("dalex_weights", sigma, n_cases)
        out = np.zeros((max(n_cases, 1), max(k, 1)), dtype=np.float64)
        self._check(self.lib.gpe_dalex_weights(
            self.h, n_cases, k, int(seed) & _U64, float(pressure),
            _ptr(sigma), _ptr(out)), "gpe_dalex_weights")
        return out[:n_cases] if k else out[:n_cases, :0]

    def dalex_sigma(self, values):
        """gpe_dalex_sigma → ``float64[n_cases]``: each case's population
        standard deviation over the fit rows, as :meth:`dalex` standardises
        by.  *values* as :meth:`dalex`."""
        rows, cases, n, c, ptr, keep = self._values_arg("dalex_sigma", values)
        out = np.zeros(max(cases, 1), dtype=np.float64)
        self._check(self.lib.gpe_dalex_sigma(self.h, ptr, n, c, _ptr(out)),
                    "gpe_dalex_sigma")
        return out[:cases]

    def weighted_errors(self, values, weights):
        """gpe_weighted_errors → ``float64[n, G]``: every row's sum of
        ``weights[g][c] * values[i][c]``, *weights* float64 ``[G, n_cases]``
        (or 1-D), any ``G >= 1``, checked by :func:`check_case_weights`.  A
        row with an error that is not finite gives ``nan``.  *values* as
        :meth:`dalex`."""
        rows, cases, n, c, ptr, keep = self._values_arg("weighted_errors",
                                                        values)
        w = check_case_weights("weighted_errors", weights, cases)
        G = w.shape[0]
        out = np.zeros((max(rows, 1), max(G, 1)), dtype=np.float64)
        self._check(self.lib.gpe_weighted_errors(
            self.h, ptr, n, c, _ptr(w), G, _ptr(out)), "gpe_weighted_errors")
        return out[:rows, :G]

    def dalex_ms(self):
        """Device ms of the last :meth:`dalex` / :meth:`dalex_bits` /
        :meth:`weighted_errors` call's kernels."""
        ms = ctypes.c_float(0.0)
        self._check(self.lib.gpe_last_dalex_ms(self.h, ctypes.byref(ms)),
                    "gpe_last_dalex_ms")
        return float(ms.value)

    def nd_sort(self, w, k, mult=None, first_front_only=False):
        """gpe_nd_sort: the non-dominated fronts of the rows of *w* float64
        ``[n, m]`` (weighted fitness values, one row per distinct fitness; the
        rule: include/gpeval.h) until they cover ``min(total, k)``
        individuals, *mult* int32 ``[n]`` giving the individuals per row
        (None: one each).  Returns a list of int32 arrays, the rows of each
        front in the reference's order.  ``ValueError`` for the sizes the
        library refuses, for a nan and for a multiplicity below 1.  Nothing
        resident on the context is disturbed; cost grows as m * n^2."""
        w, mult, k = _nd_sort_args("nd_sort", w, mult, k)
        n, m = w.shape
        order = np.zeros(n, dtype=np.int32)
        front_end = np.zeros(n, dtype=np.int64)
        nf, nr = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self.lib.gpe_nd_sort(self.h, _ptr(w), _ptr(mult), n, m, k,
                                  1 if first_front_only else 0, _ptr(order),
                                  _ptr(front_end), ctypes.byref(nf),
                                  ctypes.byref(nr))
        if rc == GPE_E_ARG:
            msg = self.lib.gpe_last_error(self.h)
            raise ValueError(msg.decode() if msg else "nd_sort: bad values")
        self._check(rc, "gpe_nd_sort")
        return _nd_sort_result(order, front_end, nf.value)

    def nd_sort_ms(self):
        """Device ms of the last :meth:`nd_sort` call's kernels."""
        ms = ctypes.c_float(0.0)
        self._check(self.lib.gpe_last_nd_sort_ms(self.h, ctypes.byref(ms)),
                    "gpe_last_nd_sort_ms")
        return float(ms.value)

    def nd_sort_fronts(self):
        """The number of fronts of the last :meth:`nd_sort` call."""
        nf = ctypes.c_int64(0)
        self._check(self.lib.gpe_last_nd_sort_fronts(self.h, ctypes.byref(nf)),
                    "gpe_last_nd_sort_fronts")
        return int(nf.value)

    def hit_group_counts(self, planes, n, n_cases, masks):
        """gpe_hit_group_counts → ``int64[n, G]``: ``popcount(row & mask)``
        of every program's hit plane and each of the *G* (1 .. 8) *masks*
        uint32 ``[G, ceil(n_cases / 32)]``.  *planes* as :meth:`lexicase_bits`
        takes them, or None for the resident matrix of the loaded programs
        (*n*, *n_cases* are then the context's).  The masks' pad bits are
        cleared by the library; nothing resident is disturbed."""
        # (the masks first: that order of errors is the call's)
        masks = _check_group_masks("hit_group_counts", masks,
                                   self.n_cases if planes is None else n_cases)
        rows, n, n_cases, cases, ptr, keep = self._planes_arg(
            "hit_group_counts", planes, n, n_cases)
        G = masks.shape[0]
        out = np.zeros((max(rows, 1), max(G, 1)), dtype=np.int32)
        self._check(self.lib.gpe_hit_group_counts(
            self.h, ptr, n, n_cases, _ptr(masks), G, _ptr(out)),
            "gpe_hit_group_counts")
        return out[:rows, :G].astype(np.int64)

    def hit_group_ms(self):
        """Device ms of the last :meth:`hit_group_counts`' kernel."""
        ms = ctypes.c_float(0.0)
        self._check(self.lib.gpe_last_hit_group_ms(self.h, ctypes.byref(ms)),
                    "gpe_last_hit_group_ms")
        return float(ms.value)

    def _planes_arg(self, what, planes, n, n_cases):
        """The *planes* argument of every call on a hit matrix →
        ``(rows, n, n_cases, cases, ptr, keep)``: *rows* / *cases* the shape
        the outputs need, *n* / *n_cases* / *ptr* the library's arguments
        (None: the resident matrix, whose sizes the library knows; *keep*
        holds what *ptr* points into).  The sizes themselves are the
        library's to refuse."""
        if planes is None:
            return self.n_prog, 0, 0, self.n_cases, None, None
        units = (int(n_cases) + 31) // 32
        planes = np.ascontiguousarray(planes, dtype=np.uint32)
        if planes.shape != (int(n), units):
            raise ValueError("%s: planes must be uint32 [%d, %d]"
                             % (what, n, units))
        # (a matrix of no rows is still the caller's, not the resident one)
        keep = planes if planes.size else np.zeros(1, dtype=np.uint32)
        return int(n), int(n), int(n_cases), int(n_cases), _ptr(keep), keep

    def case_solve_counts(self, planes, n, n_cases, eps=0.0, live=None):
        """gpe_case_solve_counts → ``int64[n_cases]``: the live individuals
        that hit each case.  *planes*: a program-major hit matrix uint32
        [n, ceil(n_cases / 32)], or None for the resident matrix of the
        loaded programs (*n*, *n_cases* are then the context's; *eps*
        thresholds the F machine's per-case matrix, as
        :meth:`informed_cases`).  *live*: uint64 [ceil(n / 64)]
        (:func:`pack_live_mask`) or None.  Nothing resident is disturbed."""
        rows, n, n_cases, cases, ptr, keep = self._planes_arg(
            "case_solve_counts", planes, n, n_cases)
        live = _check_live("case_solve_counts", live, rows)
        out = np.zeros(max(cases, 1), dtype=np.int32)
        self._check(self.lib.gpe_case_solve_counts(
            self.h, ptr, n, n_cases, float(eps), _ptr(live), _ptr(out)),
            "gpe_case_solve_counts")
        return out[:cases].astype(np.int64)

    def hit_weighted_sums(self, planes, n, n_cases, weights, eps=0.0):
        """gpe_hit_weighted_sums → ``float64[n, G]``: every program's sum of
        ``weights[g]`` over the cases it hits, *weights* float64
        ``[G, n_cases]`` (or 1-D), *G* in 1 .. 8, checked by
        :func:`check_case_weights`.  The matrix as
        :meth:`case_solve_counts`."""
        rows, n, n_cases, cases, ptr, keep = self._planes_arg(
            "hit_weighted_sums", planes, n, n_cases)
        w = check_case_weights("hit_weighted_sums", weights, cases)
        G = w.shape[0]
        out = np.zeros((max(rows, 1), max(G, 1)), dtype=np.float64)
        self._check(self.lib.gpe_hit_weighted_sums(
            self.h, ptr, n, n_cases, float(eps), _ptr(w), G, _ptr(out)),
            "gpe_hit_weighted_sums")
        return out[:rows, :G]

    def hit_shared_sums(self, planes, n, n_cases, eps=0.0, live=None):
        """gpe_hit_shared_sums → ``(counts int64[n_cases], sums
        float64[n])``: the solve counts over the *live* individuals and every
        program's sum of ``1 / counts[c]`` over the cases it hits (implicit
        fitness sharing), the weights made on the device.  The matrix and
        *live* as :meth:`case_solve_counts`."""
        rows, n, n_cases, cases, ptr, keep = self._planes_arg(
            "hit_shared_sums", planes, n, n_cases)
        live = _check_live("hit_shared_sums", live, rows)
        cnt = np.zeros(max(cases, 1), dtype=np.int32)
        out = np.zeros(max(rows, 1), dtype=np.float64)
        self._check(self.lib.gpe_hit_shared_sums(
            self.h, ptr, n, n_cases, float(eps), _ptr(live), _ptr(cnt),
            _ptr(out)), "gpe_hit_shared_sums")
        return cnt[:cases].astype(np.int64), out[:rows]

    def case_weights_ms(self):
        """Device ms of the last case-weight call's kernels."""
        ms = ctypes.c_float(0.0)
        self._check(self.lib.gpe_last_case_weights_ms(self.h, ctypes.byref(ms)),
                    "gpe_last_case_weights_ms")
        return float(ms.value)

    def informed_cases(self, planes, n, n_cases, eps, seed, m):
        """gpe_informed_cases: the farthest-first subset of *m* cases
        (informed down-sampling) → ``(idx int64[m], dist int32[m])``: the
        cases in pick order and each pick's Hamming distance to the nearest
        case picked before it (``dist[0] == -1``).  *planes*: a program-major
        hit matrix uint32 [n, ceil(n_cases / 32)], or None for the resident
        matrix of the loaded programs (*n*, *n_cases* are then the
        context's): the last run_hit_planes' on the B machine, the last
        run_abserr_cases' thresholded at *eps* on the F machine.  *seed*: the
        64-bit seed of the tie-break keys.  Nothing resident is disturbed."""
        rows, n, n_cases, cases, ptr, keep = self._planes_arg(
            "informed_cases", planes, n, n_cases)
        idx = np.zeros(max(int(m), 1), dtype=np.int64)
        dist = np.zeros(max(int(m), 1), dtype=np.int32)
        self._check(self.lib.gpe_informed_cases(
            self.h, ptr, n, n_cases, float(eps),
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(m), _ptr(idx), _ptr(dist)),
            "gpe_informed_cases")
        return idx[:int(m)], dist[:int(m)]

    def set_lowering(self, machine, nv, leaf, entries, n_entries):
        """gpe_set_lowering: the pset tables of device lowering (``leaf``
        one byte per argument, ``entries`` packed gpe_entry records)."""
        leaf = bytes(leaf)
        self._lw = (leaf, bytes(entries))        # keep the buffers alive
        lb = ctypes.create_string_buffer(leaf, max(len(leaf), 1))
        eb = ctypes.create_string_buffer(self._lw[1], max(len(self._lw[1]), 1))
        self._check(self.lib.gpe_set_lowering(self.h, int(machine), int(nv), lb,
                                              len(leaf), eb, int(n_entries)),
                    "gpe_set_lowering")

    def lower_programs(self, codes, node_off, evals, eph_off, out=None):
        """gpe_lower_programs: lower the trees on the device and load them.
        Returns (depth int32[n], err uint8[n], status uint8[n]) — views of
        *out*'s (a :class:`LoweringBuffers`) arrays when given."""
        node_off = np.frombuffer(node_off, dtype=np.int64)
        eph_off = np.frombuffer(eph_off, dtype=np.int64)
        n = len(node_off) - 1
        if out is not None:
            depth, err, status = out.views(max(n, 1))
        else:
            depth = np.zeros(max(n, 1), dtype=np.int32)
            err = np.zeros(max(n, 1), dtype=np.uint8)
            status = np.zeros(max(n, 1), dtype=np.uint8)
        cb = np.frombuffer(codes, dtype=np.uint8) if len(codes) else \
            np.zeros(1, dtype=np.uint8)
        eb = np.frombuffer(evals, dtype=np.uint8) if len(evals) else \
            np.zeros(1, dtype=np.uint8)
        self.resident = None
        self.n_prog = 0
        self._check(self.lib.gpe_lower_programs(
            self.h, _ptr(cb), _ptr(node_off), n, _ptr(eb), _ptr(eph_off),
            _ptr(depth), _ptr(err), _ptr(status)), "gpe_lower_programs")
        self.n_prog = n
        return depth[:n], err[:n], status[:n]

    def lower_begin(self, n_total, out=None):
        """gpe_lower_begin: a device lowering of n_total trees, added in
        chunks (:meth:`lower_add`) and finished by :meth:`lower_end`.  With
        *out* (a :class:`LoweringBuffers`), gpe_lower_begin_into: the chunks
        are decoded into *out*'s arrays as they are added, and lower_end
        returns views of them."""
        self.resident = None
        self.n_prog = 0
        self._lw_n = int(n_total)
        self._lw_into = None
        if out is not None and n_total > 0:
            depth, err, status = out.views(int(n_total))
            self._check(self.lib.gpe_lower_begin_into(
                self.h, int(n_total), _ptr(depth), _ptr(err), _ptr(status)),
                "gpe_lower_begin_into")
            self._lw_into = (depth, err, status)
            return
        self._check(self.lib.gpe_lower_begin(self.h, int(n_total)), "gpe_lower_begin")

    def lower_add(self, codes, node_off, evals, eph_off):
        """gpe_lower_add: the next chunk (read_codes' four buffers, offsets
        from 0); its upload and lowering run on the device asynchronously."""
        node_off = np.frombuffer(node_off, dtype=np.int64)
        eph_off = np.frombuffer(eph_off, dtype=np.int64)
        n = len(node_off) - 1
        cb = np.frombuffer(codes, dtype=np.uint8) if len(codes) else \
            np.zeros(1, dtype=np.uint8)
        eb = np.frombuffer(evals, dtype=np.uint8) if len(evals) else \
            np.zeros(1, dtype=np.uint8)
        self._check(self.lib.gpe_lower_add(self.h, _ptr(cb), _ptr(node_off), n,
                                           _ptr(eb), _ptr(eph_off)), "gpe_lower_add")

    def lower_add_addr(self):
        """The address of gpe_lower_add (for the native read-and-lower
        pipeline, Flattener.read_lower)."""
        return ctypes.cast(self.lib.gpe_lower_add, ctypes.c_void_p).value

    def handle_addr(self):
        return ctypes.cast(self.h, ctypes.c_void_p).value

    def check_rc(self, rc, what):
        self._check(int(rc), what)

    def lower_end(self, out=None):
        """gpe_lower_end → (depth int32[n], err uint8[n], status uint8[n])
        for all the lowering's trees (views of *out*'s arrays when given)."""
        n = self._lw_n
        into, self._lw_into = self._lw_into, None
        if into is not None:
            depth, err, status = into
        elif out is not None:
            depth, err, status = out.views(max(n, 1))
        else:
            depth = np.zeros(max(n, 1), dtype=np.int32)
            err = np.zeros(max(n, 1), dtype=np.uint8)
            status = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self.lib.gpe_lower_end(self.h, _ptr(depth), _ptr(err), _ptr(status)),
                    "gpe_lower_end")
        self.n_prog = n
        self.resident = None
        return depth[:n], err[:n], status[:n]

    def tournament(self, wvalues, k, tournsize, rng, weight=1.0):
        """gpe_tournament: k tournaments of ``tournsize`` on ``wvalues``
        [n] or [n, nobj] (None: the last run's fitness on the device times
        ``weight``), drawing from the ``random.Random``-compatible ``rng`` as
        the reference's selTournament does and advancing its state.
        Returns the selected indices."""
        version, words, gauss = rng.getstate()
        st = np.asarray(words, dtype=np.uint32)
        if wvalues is None:
            n, nobj, ptr = 0, 1, None
        else:
            wvalues = np.ascontiguousarray(wvalues, dtype=np.float64)
            if wvalues.ndim == 1:
                wvalues = wvalues[:, None]
            n, nobj = wvalues.shape
            ptr = _ptr(wvalues)
        out = np.zeros(max(int(k), 1), dtype=np.int32)
        self._check(self.lib.gpe_tournament(self.h, ptr, n, nobj, float(weight),
                                            int(k), int(tournsize), _ptr(st),
                                            _ptr(out)), "gpe_tournament")
        rng.setstate((version, tuple(int(w) for w in st), gauss))
        return out[:int(k)]

    def run_device(self, mode, hi_ptr, lo_ptr, err_ptr, flags_ptr):
        self._check(self.lib.gpe_run_device(self.h, mode, hi_ptr, lo_ptr,
                                            err_ptr, flags_ptr),
                    "gpe_run_device")

    # ---- multi-GPU (include/gpeval.h: gpe_comm_*, gpe_run_sharded*) ----
    def comm_init(self, rank, world, unique_id):
        """Join the RCCL communicator ``unique_id`` (from rank 0's
        :func:`comm_unique_id`) as ``rank`` of ``world``.  Collective."""
        uid = ctypes.create_string_buffer(bytes(unique_id),
                                          GPE_UNIQUE_ID_BYTES)
        self._check(self.lib.gpe_comm_init(self.h, int(rank), int(world),
                                           uid), "gpe_comm_init")

    def comm_info(self):
        r, w = _I(), _I()
        self._check(self.lib.gpe_comm_info(self.h, ctypes.byref(r),
                                           ctypes.byref(w)), "gpe_comm_info")
        return r.value, w.value

    def run_sharded(self, mode, case_offset):
        """Case-sharded gpe_run: whole-population (hi, lo, err, flags),
        identical on every rank.  Collective."""
        n = self.n_prog
        hi = np.zeros(n, dtype=np.float64)
        lo = np.zeros(n, dtype=np.float64)
        err = np.zeros(n, dtype=np.uint64)
        flags = np.zeros(n, dtype=np.uint32)
        self._check(self.lib.gpe_run_sharded(self.h, mode, int(case_offset),
                                             _ptr(hi), _ptr(lo), _ptr(err),
                                             _ptr(flags)), "gpe_run_sharded")
        return hi, lo, err, flags

    def run_sharded_device(self, mode, case_offset, hi_ptr=None, lo_ptr=None,
                           err_ptr=None, flags_ptr=None):
        self._check(self.lib.gpe_run_sharded_device(
            self.h, mode, int(case_offset), hi_ptr, lo_ptr, err_ptr,
            flags_ptr), "gpe_run_sharded_device")

    def run_gathered(self, mode, width, world, tags=None, want=None):
        """Population-sharded gpe_run: every rank's results, rank r's
        program i at r * width + i; ``tags`` (uint8 per loaded program)
        come back in bits 8..15 of the flags.  *want*: the outputs to copy
        (default all; the others are None — the flags always come, they
        carry the tags).  Collective."""
        m = int(width) * int(world)
        if tags is not None:
            tags = np.ascontiguousarray(tags, dtype=np.uint8)
        names = ("hi", "lo", "err", "flags")
        dts = (np.float64, np.float64, np.uint64, np.uint32)
        arrs = [np.zeros(m, dtype=d) if (want is None or nm in want or
                                         nm == "flags") else None
                for nm, d in zip(names, dts)]
        self._check(self.lib.gpe_run_gathered(self.h, mode, int(width),
                                              _ptr(tags), *[
                                                  _ptr(a) if a is not None else None
                                                  for a in arrs]),
                    "gpe_run_gathered")
        return tuple(arrs)

    def timing(self):
        ms = (ctypes.c_float * 3)()
        self._check(self.lib.gpe_last_timing(self.h, ms), "gpe_last_timing")
        return {"kernel_ms": ms[0], "reduce_ms": ms[1], "total_ms": ms[2]}

    def comm_timing(self):
        """Collective time of the last sharded / gathered run (waits for it,
        bounded by GPE_COMM_TIMEOUT_S)."""
        ms = (ctypes.c_float * 2)()
        self._check(self.lib.gpe_last_comm_timing(self.h, ms),
                    "gpe_last_comm_timing")
        return {"comm_ms": ms[0], "redo_ms": ms[1]}

    def math_probe(self, fn, x):
        """gpe_math_probe (include/gpeval.h lists the function numbers; 15 /
        16: the C++ kernels' fp64 / fp32 square root; 17 / 18: the exact and the
        fp32 asm cores' SQRT handlers)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        self._check(self.lib.gpe_math_probe(self.h, int(fn), _ptr(x), _ptr(y),
                                            len(x)), "gpe_math_probe")
        return y

    def geometry(self):
        g = (ctypes.c_int64 * 17)()
        self._check(self.lib.gpe_last_geometry_ex(self.h, g, 17),
                    "gpe_last_geometry_ex")
        return dict(zip(("asm", "fast", "deep", "redo", "P", "groups",
                         "redo_tiles", "waves_per_block", "asm_deep",
                         "asm_deep_P", "asm_deep_groups",
                         "asm_deep_waves_per_block", "redo_exact_cpp",
                         "asm_typed", "asm_typed_P", "asm_typed_groups",
                         "typed_const"),
                        list(g)))

    LAUNCHES = ("asm_fast", "asm_deep", "typed", "cpp_fast", "cpp_deep",
                "fasm", "dasm", "moments", "moments_deep", "abserr",
                "abserr_deep")

    def trig_classes(self, picked=False):
        """sin/cos words of the last exact-core translation per base class
        (gpe_last_trig_classes): {"general", "mid", "small"}; ``picked``: per
        class whose handler was picked (gpe_last_trig_picked): those three
        and {"midlo", "wide"}."""
        if picked:
            g = (ctypes.c_int64 * len(TRIG_PICKED))()
            self._check(self.lib.gpe_last_trig_picked(self.h, g),
                        "gpe_last_trig_picked")
            return dict(zip(TRIG_PICKED, (int(v) for v in g)))
        g = (ctypes.c_int64 * 3)()
        self._check(self.lib.gpe_last_trig_classes(self.h, g),
                    "gpe_last_trig_classes")
        return dict(zip(TRIG_CLASSES, (int(v) for v in g)))

    def launch_shape(self, which):
        """One launch of the last run as planned (gpe_last_launch_shape):
        ``which`` is an index or one of ``LAUNCHES``."""
        if isinstance(which, str):
            which = self.LAUNCHES.index(which)
        g = (ctypes.c_int64 * 13)()
        self._check(self.lib.gpe_last_launch_shape(self.h, int(which), g, 13),
                    "gpe_last_launch_shape")
        return dict(zip(("programs", "P", "wpb", "waves", "n_slots", "K",
                         "sdepth", "n_tiles", "tiles_per_group", "groups",
                         "dbuf", "lds_bytes", "tile_loop"), list(g)))
