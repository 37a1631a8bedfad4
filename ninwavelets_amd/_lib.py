"""ctypes binding of libninwave.so (the C ABI declared in include/ninwave.h).

The shared library is built in-tree by ``__graft_entry__.build()`` (or
``make -C ninwavelets_amd/csrc``).  There is no fallback: if the library is
missing or a GPU is absent, calls raise instead of computing on the CPU.

Mixing with PyTorch in one process: torch wheels bundle their own HIP runtime.
Import torch BEFORE this package, so libninwave.so binds to torch's already
loaded libamdhip64/librocfft (same sonames) and the process keeps one runtime.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NINWAVE_LIB', os.path.join(_HERE, 'libninwave.so'))

# status codes / constants (ninwave.h)
NW_OK = 0
NW_E_INVALID = -1
NW_E_HIP = -2
NW_E_ROCFFT = -3
NW_E_NOMEM = -4
NW_E_STATE = -5
NW_E_NODEVICE = -6
NW_E_BOUNDS = -7

NW_F32, NW_F64 = 0, 1
NW_MORSE, NW_MORLET, NW_SHANNON, NW_TABLE = 1, 2, 3, 4
NW_MEXICAN_HAT, NW_HAAR = 5, 6
NW_INTERPOLATE = 0x1
NW_ENGINE_ROCFFT = 0x10
NW_ENGINE_FUSED = 0x20
NW_TIMING = 0x100
NW_TIMING_CHAIN = 0x800
NW_NO_DEDUP = 0x200
NW_NO_CHIRP = 0x400
NW_OUT_CWT, NW_OUT_ABS, NW_OUT_POWER = 0, 1, 2
NW_OUT_POWER_MEAN, NW_OUT_ITC, NW_OUT_POWER_SUM, NW_OUT_PHASE_SUM = 3, 4, 5, 6
NW_OUT_CROSS_SUM, NW_OUT_PLV_SUM = 7, 8          # nw_execute_pair only
NW_OUT_LAG_SUM = 9                               # ... and nw_execute_conn: the phase-lag sums
NW_REDUCE_NONE, NW_REDUCE_ROWS, NW_REDUCE_PARTIALS = 0, 1, 2   # nw_stats.reduce_path
NW_REDUCE_CONN = 3                                              # ... of nw_execute_conn
NW_REDUCE_CONN_TIME = 4                                         # ... of nw_execute_conn_time
NW_REDUCE_PAC = 5                                               # ... of nw_execute_pac
NW_REDUCE_ENV = 6                                               # ... of nw_execute_env_time
NW_REDUCE_PAC_BINS = 7                                          # ... of nw_execute_pac_bins
NW_REDUCE_ERPAC = 8                                             # ... of nw_execute_erpac
NW_REDUCE_PAC_SURR = 9                                          # ... of nw_execute_pac_surr
NW_PAC_MAX_LAGS = 4096                                          # nw_execute_pac_surr: at most this many lags
NW_PAC_SURR_PLAIN, NW_PAC_SURR_DEBIASED = 0, 1                  # nw_execute_pac_surr's centre
NW_PAC_MAX_BINS = 36                                            # nw_execute_pac_bins: nbins even, 2 .. 36
NW_ENV_PLAIN, NW_ENV_ORTH = 0, 1                                # nw_execute_env_time's env_kind
NW_MEM_HOST, NW_MEM_DEVICE = 0, 1
# nw_stats.kernel -> the kernel name rocprofv3 shows
KERNEL_NAMES = {0: None, 1: 'nw_fused_kernel', 2: 'nw_fused_pair_kernel', 3: 'nw_chirp_kernel',
                4: 'cols_kernel', 5: 'k1_multiply', 6: 'nw_fused_decim_kernel'}
NW_BL = {'mean': 0, 'ratio': 1, 'percent': 2, 'log': 3, 'zscore': 4, 'zlog': 5}


class nw_grid(ctypes.Structure):
    _fields_ = [('delta', ctypes.c_double), ('len_full', ctypes.c_int64), ('len_valid', ctypes.c_int64)]


class nw_stats(ctypes.Structure):
    _fields_ = [('executes', ctypes.c_int64), ('chunks', ctypes.c_int64),
                ('ms_forward', ctypes.c_double), ('ms_multiply', ctypes.c_double),
                ('ms_inverse', ctypes.c_double), ('ms_epilogue', ctypes.c_double),
                ('ms_fused', ctypes.c_double), ('ms_copy', ctypes.c_double),
                ('launches_multiply', ctypes.c_int64), ('launches_fused', ctypes.c_int64),
                ('engine', ctypes.c_int64), ('ms_rows', ctypes.c_double),
                ('launches_rows', ctypes.c_int64), ('ms_expand', ctypes.c_double),
                ('launches_expand', ctypes.c_int64), ('unique_rows', ctypes.c_int64),
                ('kernel', ctypes.c_int64), ('device_bytes', ctypes.c_int64),
                ('reduce_path', ctypes.c_int64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# every symbol of include/ninwave.h: (name, restype, argtypes)
_P = ctypes.c_void_p
_I64 = ctypes.c_int64
SIGNATURES = [
    ('nw_last_error', ctypes.c_char_p, []),
    ('nw_version', ctypes.c_char_p, []),
    ('nw_set_log_level', ctypes.c_int, [ctypes.c_int]),
    ('nw_debug_bounds', ctypes.c_int, []),
    ('nw_debug_selftest', ctypes.c_int, [ctypes.c_int]),
    ('nw_device_count', ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    ('nw_trans_grid', ctypes.c_int, [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.POINTER(nw_grid)]),
    ('nw_fused_supported', ctypes.c_int, [_I64, ctypes.c_int]),
    ('nw_decim_supported', ctypes.c_int, [_I64, ctypes.c_int, ctypes.c_int]),
    ('nw_plan_set_decim', ctypes.c_int, [_P, ctypes.c_int]),
    ('nw_pair_partials_supported', ctypes.c_int, [_I64, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    ('nw_plan_create', ctypes.c_int, [ctypes.POINTER(_P), ctypes.c_int, _I64, _I64, ctypes.c_int32,
                                      ctypes.c_int, ctypes.c_uint32]),
    ('nw_plan_set_wavelet', ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_double), ctypes.POINTER(nw_grid), _P,
                                           ctypes.POINTER(ctypes.c_int64)]),
    ('nw_plan_wavelet_shape', ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    ('nw_plan_wavelet_rows', ctypes.c_int, [_P, _P]),
    ('nw_plan_row_support', ctypes.c_int, [_P, ctypes.c_int, _P]),
    ('nw_execute', ctypes.c_int, [_P, _P, _I64, _P, ctypes.c_int, ctypes.c_int]),
    ('nw_execute_pair', ctypes.c_int, [_P, _P, _P, _I64, _P, ctypes.c_int, ctypes.c_int]),
    ('nw_conn_tiles', ctypes.c_int, [ctypes.c_int32, _P, _P, _I64, _P, ctypes.POINTER(_I64), _P]),
    ('nw_execute_conn', ctypes.c_int, [_P, _P, _I64, ctypes.c_int32, _P, _P, _I64, _P, _P, ctypes.c_int, ctypes.c_int]),
    ('nw_conn_time_count', ctypes.c_int, [_I64, _I64, _I64, _I64, ctypes.POINTER(_I64)]),
    ('nw_execute_conn_time', ctypes.c_int, [_P, _P, _I64, ctypes.c_int32, _P, _P, _I64, _I64, _I64, _I64, _P, _P,
                                            ctypes.c_int, ctypes.c_int]),
    ('nw_execute_env_time', ctypes.c_int, [_P, _P, _I64, ctypes.c_int32, _P, _P, _I64, _I64, _I64, _I64, _P, _P,
                                           ctypes.c_int, ctypes.c_int]),
    ('nw_execute_pac', ctypes.c_int, [_P, _P, _I64, ctypes.c_int32, _P, _P, _I64, _P, ctypes.c_int32, _P, ctypes.c_int32,
                                      _I64, _I64, _I64, _P, _P, _P, ctypes.c_int]),
    ('nw_execute_pac_surr', ctypes.c_int, [_P, _P, _I64, ctypes.c_int32, _P, _P, _I64, _P, ctypes.c_int32, _P,
                                           ctypes.c_int32, _I64, _I64, _I64, _P, ctypes.c_int32, ctypes.c_int, _P, _P, _P,
                                           _P, _P, ctypes.c_int]),
    ('nw_execute_erpac', ctypes.c_int, [_P, _P, _I64, ctypes.c_int32, _P, _P, _I64, _P, ctypes.c_int32, _P, ctypes.c_int32,
                                        _I64, _I64, _I64, _P, _P, _P, ctypes.c_int]),
    ('nw_pac_bin_edges', ctypes.c_int, [ctypes.c_int32, _P]),
    ('nw_execute_pac_bins', ctypes.c_int, [_P, _P, _I64, ctypes.c_int32, _P, _P, _I64, _P, ctypes.c_int32, _P,
                                           ctypes.c_int32, _I64, _I64, _I64, ctypes.c_int32, _P, _P, ctypes.c_int]),
    ('nw_execute_multi',ctypes.c_int, [ctypes.POINTER(_P), ctypes.c_int, _P, _I64, _P, ctypes.c_int]),
    ('nw_execute_multi_scales', ctypes.c_int, [ctypes.POINTER(_P), ctypes.c_int, _P, _I64, _P, ctypes.c_int]),
    ('nw_execute_multi_device', ctypes.c_int, [ctypes.POINTER(_P), ctypes.c_int, ctypes.POINTER(_P),
                                               ctypes.POINTER(_I64), ctypes.POINTER(_P), ctypes.c_int]),
    ('nw_baseline', ctypes.c_int, [ctypes.c_int, ctypes.c_int, _P, _I64, _I64, _I64, _I64, ctypes.c_int, _P,
                                   ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    ('nw_make_wavelets', ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_double,
                                        ctypes.c_double, _P, ctypes.POINTER(ctypes.c_int64),
                                        ctypes.POINTER(ctypes.c_int64)]),
    ('nw_host_alloc', ctypes.c_int, [_I64, ctypes.POINTER(_P)]),
    ('nw_host_free', ctypes.c_int, [_P]),
    ('nw_host_advise', ctypes.c_int, [_P, _I64, ctypes.POINTER(_I64)]),
    ('nw_plan_set_stream', ctypes.c_int, [_P, _P]),
    ('nw_plan_get_stream', ctypes.c_int, [_P, ctypes.POINTER(_P)]),
    ('nw_plan_sync', ctypes.c_int, [_P]),
    ('nw_plan_stats', ctypes.c_int, [_P, ctypes.POINTER(nw_stats)]),
    ('nw_plan_reset_stats', ctypes.c_int, [_P]),
    ('nw_plan_destroy', ctypes.c_int, [_P]),
]


class NinwaveError(RuntimeError):
    """A non-zero status from libninwave.so (message from nw_last_error())."""

    def __init__(self, code, msg):
        super().__init__(f'libninwave status {code}: {msg}')
        self.code = code


_lib = None


def lib():
    """Load libninwave.so once; raise loudly if it is missing (no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f'{LIB_PATH} not found: build it with '
                              '`python -c "import __graft_entry__ as g; g.build()"` '
                              'or `make -C ninwavelets_amd/csrc`')
        handle = ctypes.CDLL(LIB_PATH)
        # the product library must export every entry point; a diagnostic build of an older
        # tree (NINWAVE_LIB, tools/ab.sh A/B against a past round) may lack the newer ones,
        # which then stay unbound (calling one raises AttributeError)
        product = os.path.abspath(LIB_PATH) in (os.path.join(_HERE, 'libninwave.so'),
                                                os.path.join(_HERE, 'libninwave_debug.so'))
        for name, res, args in SIGNATURES:
            fn = getattr(handle, name, None)
            if fn is None:
                if product:
                    raise ImportError(f'{LIB_PATH} does not export {name}: rebuild it')
                continue
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc):
    if rc != NW_OK:
        msg = lib().nw_last_error().decode(errors='replace')
        if rc == NW_E_INVALID:
            raise ValueError(msg)
        raise NinwaveError(rc, msg)


def set_log_level(level: int) -> int:
    """NW_LOG diagnostics on stderr (0 silent, 1 decisions and errors, 2 every launch); returns
    the previous level."""
    return int(lib().nw_set_log_level(int(level)))


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = lib().nw_device_count(ctypes.byref(n))
    return n.value if rc == NW_OK else 0


def trans_grid(real_length: float, sfreq: float, interpolate: bool) -> nw_grid:
    g = nw_grid()
    check(lib().nw_trans_grid(float(real_length), float(sfreq), int(bool(interpolate)), ctypes.byref(g)))
    return g


def fused_supported(n: int, dtype: int) -> bool:
    return bool(lib().nw_fused_supported(int(n), int(dtype)))


def decim_supported(n: int, dtype: int, decim: int) -> bool:
    """Whether a plan of (n, dtype) decimates by ``decim`` on the device (nw_decim_supported;
    host-only, no GPU needed)."""
    return bool(lib().nw_decim_supported(int(n), int(dtype), int(decim)))


def pair_partials_supported(n: int, dtype: int, kind: int, out_kind: int) -> bool:
    """Whether nw_execute_pair forms the sums of ``out_kind`` as block partial sums inside the
    transform kernel for (n, dtype, wavelet kind) (nw_pair_partials_supported; host-only)."""
    return bool(lib().nw_pair_partials_supported(int(n), int(dtype), int(kind), int(out_kind)))


def conn_tiles(nchan: int, ia, ib):
    """The pair tiling nw_execute_conn uses for the pairs (ia[p], ib[p]) of ``nchan`` channels
    (nw_conn_tiles; host-only): (tile_of_pair int32 [npairs], ntiles, (kConnCh, kConnPairs,
    sample tile)).  ValueError for nchan < 1 or an index outside [0, nchan)."""
    import numpy as np
    ia = np.ascontiguousarray(ia, dtype=np.int32)
    ib = np.ascontiguousarray(ib, dtype=np.int32)
    if ia.ndim != 1 or ia.shape != ib.shape:
        raise ValueError(f'ia and ib must be 1-D index lists of equal length, got {ia.shape} and {ib.shape}')
    tile = np.empty(ia.size, dtype=np.int32)
    ntiles = ctypes.c_int64()
    limits = (ctypes.c_int32 * 3)()
    check(lib().nw_conn_tiles(int(nchan), ia.ctypes.data_as(_P), ib.ctypes.data_as(_P), int(ia.size),
                              tile.ctypes.data_as(_P), ctypes.byref(ntiles), ctypes.cast(limits, _P)))
    return tile, int(ntiles.value), tuple(limits)


def conn_time_count(n_out: int, t0: int, t1: int, step: int = 1) -> int:
    """T, the number of samples t0, t0 + step, ... < t1 that nw_execute_conn_time sums
    (nw_conn_time_count; host-only).  ValueError unless 0 <= t0 <= t1 <= n_out and step >= 1."""
    count = ctypes.c_int64()
    check(lib().nw_conn_time_count(int(n_out), int(t0), int(t1), int(step), ctypes.byref(count)))
    return int(count.value)


def check_nbins(nbins) -> int:
    """``nbins`` of the phase-binned calls as an int: even, 2 <= nbins <= NW_PAC_MAX_BINS; ValueError for
    anything else, before any device work."""
    import operator
    try:
        if isinstance(nbins, bool):
            raise TypeError
        nb = operator.index(nbins)
    except TypeError:
        nb = None
    if nb is None or nb < 2 or nb > NW_PAC_MAX_BINS or nb % 2:
        raise ValueError(f'nbins must be an even integer with 2 <= nbins <= {NW_PAC_MAX_BINS}, got {nbins!r}')
    return nb


def pac_bin_edges(nbins: int):
    """The edge table of nw_execute_pac_bins (nw_pac_bin_edges; host-only): float64 (nbins, 2) =
    {cos theta_b, sin theta_b}, theta_b = -pi + 2 pi b / nbins: the doubles the device tests a sample against.
    ValueError unless nbins is an even integer with 2 <= nbins <= NW_PAC_MAX_BINS (check_nbins)."""
    import numpy as np
    nb = check_nbins(nbins)
    cs = np.empty((nb, 2), dtype=np.float64)
    check(lib().nw_pac_bin_edges(nb, cs.ctypes.data_as(_P)))
    return cs
