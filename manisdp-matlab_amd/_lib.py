"""ctypes binding of ``include/manisdp_hip.h`` (libmanisdp_hip.so).

There is no CPU fallback: if the shared library is missing or no HIP device is
visible, every entry point raises.  The library is looked up in-tree
(``manisdp-matlab_amd/lib/libmanisdp_hip.so``) so the GPU box loads exactly the
file that ``__graft_entry__.build()`` produced.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmanisdp_hip.so")

KIND_ONLYUNITDIAG, KIND_UNITDIAG, KIND_UNITTRACE, KIND_GENERIC, KIND_MULTIBLOCK, KIND_DUAL_UNITDIAG, KIND_DUAL = 1, 2, 3, 4, 5, 6, 7
KIND_DUAL_MULTIBLOCK = 8


class RtrOpts(C.Structure):
    _fields_ = [("maxiter", C.c_int32), ("maxinner", C.c_int32), ("mininner", C.c_int32),
                ("reserved0", C.c_int32), ("tolgradnorm", C.c_double), ("kappa", C.c_double),
                ("theta", C.c_double), ("rho_prime", C.c_double), ("rho_regularization", C.c_double),
                ("Delta_bar", C.c_double), ("Delta0", C.c_double)]


class RtrStats(C.Structure):
    _fields_ = [("cost", C.c_double), ("gradnorm", C.c_double), ("Delta", C.c_double),
                ("seconds", C.c_double), ("iters", C.c_int32), ("hessvecs", C.c_int32),
                ("accepted", C.c_int32), ("rejected", C.c_int32), ("cost_evals", C.c_int32),
                ("last_stop_inner", C.c_int32), ("reserved", C.c_int32 * 2)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class MsdpError(RuntimeError):
    code = None                     # the library's return code where the error came from a call (MSDP_E* of the header)


ESTATE, EUNSUPPORTED = -4, -6
EINVAL = -1
ROUND_MAX_TRIALS = 4096             # MSDP_ROUND_MAX_TRIALS
LOWRANK_MAX = 8                     # MSDP_LOWRANK_MAX
ROUND_PHASES_MAX_TRIALS = 1024      # MSDP_ROUND_PHASES_MAX_TRIALS
ROUND_PHASES_MAX_M = 64             # MSDP_ROUND_PHASES_MAX_M


_P = C.POINTER
_dp = _P(C.c_double)
_i64p = _P(C.c_int64)
_i32p = _P(C.c_int32)

# name -> (restype, argtypes); this table is also what tests/test_cabi_symbols.py
# checks against the declarations in include/manisdp_hip.h.
SIGNATURES = {
    "msdp_rtr_default_opts": (None, [_P(RtrOpts)]),
    "msdp_set_device": (C.c_int, [C.c_int32]),
    "msdp_device_count": (C.c_int, [_P(C.c_int32)]),
    "msdp_create_onlyunitdiag_csc": (C.c_int, [C.c_int64, _i64p, _i64p, _dp, C.c_int32, _P(C.c_void_p)]),
    "msdp_create_onlyunitdiag_csc_lowrank": (C.c_int, [C.c_int64, _i64p, _i64p, _dp, C.c_int32, _dp, _dp, C.c_int32, _P(C.c_void_p)]),
    "msdp_create_onlyunitdiag_csc_hermitian": (C.c_int, [C.c_int64, _i64p, _i64p, _dp, C.c_int32, _P(C.c_void_p)]),
    "msdp_create_onlyunitblockdiag_csc": (C.c_int, [C.c_int64, C.c_int32, _i64p, _i64p, _dp, C.c_int32, _P(C.c_void_p)]),
    "msdp_get_blockmult": (C.c_int, [C.c_void_p, _dp]),
    "msdp_create_posegraph_csc": (C.c_int, [C.c_int64, C.c_int32, _i64p, _i64p, _dp, C.c_int32, _P(C.c_void_p)]),
    "msdp_create_onlyunitdiag_dense": (C.c_int, [C.c_int64, _dp, C.c_int32, _P(C.c_void_p)]),
    "msdp_create_onlyunitdiag_dense_synthetic": (C.c_int, [C.c_int64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                                                          _P(C.c_void_p)]),
    "msdp_synthetic_dense_entry": (C.c_double, [C.c_int64, C.c_int64, C.c_int64, C.c_uint64]),
    "msdp_debug_set_full_rows": (C.c_int, [C.c_void_p, _dp]),
    "msdp_debug_p2p_self": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    "msdp_create_affine": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, _dp,
                                     C.c_int32, _P(C.c_void_p)]),
    "msdp_create_multiblock": (C.c_int, [C.c_int32, _i64p, C.c_int32, C.c_int64, _i64p, _i64p, _dp, _dp, _dp,
                                         C.c_int32, _P(C.c_void_p)]),
    "msdp_destroy": (C.c_int, [C.c_void_p]),
    "msdp_set_multipliers": (C.c_int, [C.c_void_p, _dp, C.c_double]),
    "msdp_set_point": (C.c_int, [C.c_void_p, C.c_int32, _dp]),
    "msdp_get_point": (C.c_int, [C.c_void_p, _dp]),
    "msdp_get_p": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "msdp_get_kind": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "msdp_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "msdp_rtr": (C.c_int, [C.c_void_p, _P(RtrOpts), _P(RtrStats)]),
    "msdp_rtr_host": (C.c_int, [C.c_void_p, C.c_int32, _dp, _P(RtrOpts), _P(RtrStats)]),
    "msdp_cost": (C.c_int, [C.c_void_p, _dp]),
    "msdp_rgrad": (C.c_int, [C.c_void_p, _dp]),
    "msdp_hessvec": (C.c_int, [C.c_void_p, _dp, _dp]),
    "msdp_proj": (C.c_int, [C.c_void_p, _dp, _dp]),
    "msdp_precon_apply": (C.c_int, [C.c_void_p, _dp, _dp]),
    "msdp_retr": (C.c_int, [C.c_void_p, _dp, _dp]),
    "msdp_get_z": (C.c_int, [C.c_void_p, _dp]),
    "msdp_linesearch_cost": (C.c_int, [C.c_void_p, _dp, C.c_double, _dp]),
    "msdp_linesearch_accept": (C.c_int, [C.c_void_p]),
    "msdp_round_hyperplane": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp, _dp, _i32p, _P(C.c_uint64), _i32p,
                                        _P(C.c_int8)]),
    "msdp_round_phases": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, _dp, _i32p, _dp, _i32p, _dp, _i32p]),
    "msdp_round_coloring": (C.c_int, [C.c_void_p, _i32p, _i32p]),
    "msdp_escape_eigs": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_int32, _dp, _dp, _dp, _P(C.c_int32)]),
    "msdp_escape_eigs_matrix": (C.c_int, [C.c_void_p, _dp, C.c_int32, C.c_double, C.c_int32, _dp, _dp, _dp,
                                         _P(C.c_int32)]),
    "msdp_escape_info": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), _dp]),
    "msdp_escape_lower_bound": (C.c_int, [C.c_void_p, _dp]),
    "msdp_escape_method": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "msdp_debug_collective_calls": (C.c_int, [C.c_void_p, _P(C.c_int64)]),
    "msdp_debug_last_rtr_device_ms": (C.c_int, [C.c_void_p, _dp]),
    "msdp_debug_persist_trace": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_uint64), C.c_int64, _P(C.c_int32), _dp]),
    "msdp_debug_time_collective": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _P(C.c_double)]),
    "msdp_debug_get_tcg_step": (C.c_int, [C.c_void_p, _dp, _dp]),
    "msdp_debug_sym_eig": (C.c_int, [C.c_int32, _dp, _dp, _dp]),
    "msdp_debug_ritz": (C.c_int, [C.c_int32, _dp, _dp, _dp, _dp, _P(C.c_int32)]),
    "msdp_debug_ritz_herm": (C.c_int, [C.c_int32, _dp, _dp, _dp, _dp, _P(C.c_int32)]),
    "msdp_debug_ritz_device": (C.c_int, [C.c_int32, _dp, _dp, _dp, _dp, _P(C.c_int32), _P(C.c_int32)]),
    "msdp_debug_ritz_stages": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int64), _P(C.c_int64)]),
    "msdp_debug_be_step_blk_instances": (C.c_int, [_P(C.c_int32), C.c_int32]),
    "msdp_debug_be_step_blk": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_int32]),
    "msdp_get_dual_slack": (C.c_int, [C.c_void_p, _dp]),
    "msdp_get_dual_slack_block": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _dp]),
    "msdp_block_eigs": (C.c_int, [C.c_void_p, C.c_int32, _i64p, _i64p, C.c_int32, C.c_int32, _dp, _dp]),
    "msdp_block_eigs_large": (C.c_int, [C.c_void_p, C.c_int32, _i64p, _i64p, C.c_int32, _dp, _dp]),
    "msdp_block_eigs_large_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "msdp_block_reshape": (C.c_int, [C.c_void_p, C.c_int32, _i64p, _i64p, _i32p, _dp, _dp, C.c_int32, C.c_double, C.c_int32,
                                     C.c_int32, C.c_double, C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _dp]),
    "msdp_release_cache": (C.c_int, []),
    "msdp_debug_pool_stats": (C.c_int, [_P(C.c_int64), _P(C.c_int64), _P(C.c_int64)]),
    "msdp_debug_mem_info": (C.c_int, [_P(C.c_int64), _P(C.c_int64)]),
    "msdp_comm_init_local": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "msdp_comm_init_ipc": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p]),
    "msdp_get_point_all": (C.c_int, [C.c_void_p, _dp]),
    "msdp_get_z_all": (C.c_int, [C.c_void_p, _dp]),
    "msdp_factor_gram": (C.c_int, [C.c_void_p, _dp]),
    "msdp_factor_rotate": (C.c_int, [C.c_void_p, C.c_int32, _dp]),
    "msdp_factor_append": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_double, C.c_int32]),
    "msdp_hfactor_gram": (C.c_int, [C.c_void_p, _dp]),
    "msdp_hfactor_rotate": (C.c_int, [C.c_void_p, C.c_int32, _dp]),
    "msdp_hfactor_append": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_double]),
    "msdp_blockfactor_gram": (C.c_int, [C.c_void_p, _dp]),
    "msdp_blockfactor_rotate": (C.c_int, [C.c_void_p, C.c_int32, _dp, _i32p]),
    "msdp_blockfactor_append": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_double, _i32p]),
    "msdp_blockfactor_round": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _i32p, _i32p]),
    "msdp_create_dual_unitdiag": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, _dp, _dp, C.c_int32, _i64p, _i64p, _dp,
                                            _dp, C.c_int32, C.POINTER(C.c_void_p)]),
    "msdp_create_dual": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, _dp, _dp, C.c_int32, _i64p, _i64p, _dp,
                                   _dp, C.c_int32, C.POINTER(C.c_void_p)]),
    "msdp_create_dual_multiblock": (C.c_int, [C.c_int32, _i64p, C.c_int32, C.c_int64, _i64p, _i64p, _dp, _dp, _dp, _dp, C.c_int32,
                                              _i64p, _i64p, _dp, _dp, C.c_int32, C.POINTER(C.c_void_p)]),
    "msdp_dual_info": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "msdp_dual_set_penalty": (C.c_int, [C.c_void_p, C.c_double, _dp]),
    "msdp_dual_outer_step": (C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    "msdp_dual_get_y": (C.c_int, [C.c_void_p, _dp]),
    "msdp_comm_unique_id": (C.c_int, [C.c_void_p]),
    "msdp_comm_init": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "msdp_local_rows": (C.c_int, [C.c_void_p, _i64p, _i64p]),
    "msdp_debug_shard": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "msdp_tcg_path": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "msdp_debug_persist_form": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "msdp_debug_block_persist_form": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "msdp_debug_block_persist_plan": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "msdp_debug_affine_plan": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "msdp_debug_trip_form": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "msdp_debug_fused_own": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "msdp_debug_fused_plan": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32)]),
    "msdp_debug_fused_wide_rule": (C.c_int, [C.c_int32, C.c_int32, _P(C.c_int32), _P(C.c_int32)]),
    "msdp_point_snapshot": (C.c_int, [C.c_void_p]),
    "msdp_point_restore": (C.c_int, [C.c_void_p]),
    "msdp_al_primal": (C.c_int, [C.c_void_p, _dp, _dp]),
    "msdp_al_dual": (C.c_int, [C.c_void_p, _dp, _dp]),
    "msdp_escape_eigs_dual": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_int32, _dp, _dp, _dp, _P(C.c_int32)]),
    "msdp_bench_hessvec": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, _dp]),
    "msdp_bench_tcg_trip": (C.c_int, [C.c_void_p, C.c_int32, _dp]),
    "msdp_bench_kernel": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp]),
    "msdp_last_error": (C.c_char_p, []),
    "msdp_version": (C.c_char_p, []),
}

AFFINE_PLAN_FIELDS = ("usym", "ntp", "nlong_e", "bW", "packed", "bnlong", "nsup", "nlong", "nshort", "nlit", "n", "nS",
                      "last_hess_path", "last_A_route")

_lib = None


def load():
    """Load libmanisdp_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MsdpError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(or `make -C manisdp-matlab_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    # the library parks one escape workspace per process between handles (msdp_release_cache): give it back when the
    # interpreter exits, and let callers do so earlier (release_cache()) before large allocations of their own
    import atexit
    atexit.register(lambda: lib.msdp_release_cache())
    return lib


def release_cache():
    """Free the device memory the library keeps between handles (the parked Lanczos workspace of the escape; the arenas of
    uncached memory, when no handle of the process holds a block of them)."""
    _check(load().msdp_release_cache())


def pool_stats():
    """(bytes the uncached-memory arenas hold, bytes handed out to live handles, number of arenas) -- msdp_debug_pool_stats."""
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    _check(load().msdp_debug_pool_stats(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def mem_info():
    """(free, total) bytes of the current device -- msdp_debug_mem_info."""
    a, b = C.c_int64(), C.c_int64()
    _check(load().msdp_debug_mem_info(C.byref(a), C.byref(b)))
    return a.value, b.value


def _check(rc):
    if rc != 0:
        err = MsdpError(f"libmanisdp_hip error {rc}: {load().msdp_last_error().decode()}")
        err.code = rc
        raise err


def _dptr(a):
    return a.ctypes.data_as(_dp)


def set_device(dev):
    _check(load().msdp_set_device(int(dev)))


def fused_wide_rule(n_loc, cus=0):
    """(G, cus_used) of the wide plan's planning rule alone (msdp_debug_fused_wide_rule): host arithmetic, no handle, no launch.
    G = 0 where the wide plan does not apply; cus <= 0 asks for the current device's CU count."""
    g, c = C.c_int32(), C.c_int32()
    _check(load().msdp_debug_fused_wide_rule(int(n_loc), int(cus), C.byref(g), C.byref(c)))
    return g.value, c.value


def device_count():
    n = C.c_int32()
    _check(load().msdp_device_count(C.byref(n)))
    return n.value


def ritz_device(G, H):
    """The kernel of the device Rayleigh-Ritz stage alone (msdp_debug_ritz_device; b = 32 or 64): H c = theta G c for the b x b
    matrices G, H.  Returns (theta, W, rank, status): status 0 = ok (theta ascending, W'GW = I, rank = b), 1 = the kernel asks
    for the host stage (dependent columns or Jacobi not converged), 2 = breakdown; theta and W are zero unless status is 0."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    H = np.ascontiguousarray(H, dtype=np.float64)
    b = G.shape[0]
    if G.shape != (b, b) or H.shape != (b, b):
        raise ValueError("ritz_device: G and H must be square and of the same order")
    theta, W = np.zeros(b), np.zeros((b, b))
    rank, status = C.c_int32(), C.c_int32()
    _check(load().msdp_debug_ritz_device(b, _dptr(G), _dptr(H), _dptr(theta), _dptr(W), C.byref(rank), C.byref(status)))
    return theta, W, rank.value, status.value


def be_step_blk_instances():
    """The (panel width, lanes per block) pairs the block eigen-solver's filter step on block storage is instantiated for
    (msdp_debug_be_step_blk_instances; no GPU touched), in the order of the dispatch."""
    buf = (C.c_int32 * 64)()
    cnt = load().msdp_debug_be_step_blk_instances(buf, 32)
    if cnt < 0 or cnt > 32:
        raise RuntimeError(f"be_step_blk_instances: {cnt} instances reported")
    return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(cnt)]


def ritz_herm(G, H):
    """The host Rayleigh-Ritz stage of the block eigen-solver's complex panel alone (msdp_debug_ritz_herm; no GPU touched):
    H c = theta G c for complex Hermitian G, H of order bc.  Returns (theta, W, rank): theta ascending and +inf beyond rank, W
    complex with W^H G W = I on its first rank columns and zero columns beyond."""
    G = np.ascontiguousarray(G, dtype=np.complex128)
    H = np.ascontiguousarray(H, dtype=np.complex128)
    bc = G.shape[0]
    if G.shape != (bc, bc) or H.shape != (bc, bc):
        raise ValueError("ritz_herm: G and H must be square and of the same order")
    theta, W = np.zeros(bc), np.zeros((bc, bc), dtype=np.complex128)
    rank = C.c_int32()
    _check(load().msdp_debug_ritz_herm(bc, _dptr(G), _dptr(H), _dptr(theta), _dptr(W), C.byref(rank)))
    return theta, W, rank.value


def hermitian_csc(Cmat):
    """The CSC form (sorted indices, complex128) of a scipy sparse matrix that must be Hermitian: C == C^H exactly and a real
    diagonal, else ValueError.  No library call."""
    import scipy.sparse as sp
    if not sp.issparse(Cmat):
        raise ValueError("the Hermitian cost matrix must be a scipy sparse matrix")
    Cc = sp.csc_matrix(Cmat, dtype=np.complex128)
    if Cc.shape[0] != Cc.shape[1]:
        raise ValueError(f"the cost matrix is not Hermitian: shape {Cc.shape}")
    Cc.sum_duplicates()
    Cc.sort_indices()
    if np.any(Cc.diagonal().imag != 0.0):
        raise ValueError("the cost matrix is not Hermitian: its diagonal has imaginary parts")
    D = (Cc - Cc.conj().T).tocsr()
    if D.nnz and np.any(D.data != 0):
        raise ValueError("the cost matrix is not Hermitian: C != C^H")
    return Cc


def default_opts(**kw):
    o = RtrOpts()
    load().msdp_rtr_default_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class Handle:
    """Owning wrapper of an ``msdp_handle``.  Factors cross this boundary in the
    reference layout: (n, p) C-contiguous NumPy arrays for the oblique kinds (the
    bytes of MATLAB's p x n column-major Y), (n, p) arrays for unittrace as well
    (converted to MATLAB's n x p column-major, i.e. Fortran order, on the way in)."""

    def __init__(self, ptr, kind, n):
        self._h = C.c_void_p(ptr)
        self.kind = kind
        self.n = n
        self.p = 0
        self.hermitian = False            # onlyunitdiag_hermitian: factors are complex (n, p) arrays, p counts complex columns
        self.blk = 0                      # onlyunitblockdiag / posegraph: the block order of the factor and of the storage, as
        self.efree = 0                    # Dev.blk (0: no blocks), and how many of a block's rows are free (posegraph: 1, blk = d + 1)
        self._lib = load()

    # ---- construction
    @classmethod
    def onlyunitdiag(cls, Cmat, pcap=32):
        import scipy.sparse as sp
        lib = load()
        out = C.c_void_p()
        n = Cmat.shape[0]
        if sp.issparse(Cmat):
            Cc = Cmat.tocsc()
            Cc.sort_indices()
            jc = np.ascontiguousarray(Cc.indptr, dtype=np.int64)
            ir = np.ascontiguousarray(Cc.indices, dtype=np.int64)
            pr = np.ascontiguousarray(Cc.data, dtype=np.float64)
            _check(lib.msdp_create_onlyunitdiag_csc(n, jc.ctypes.data_as(_i64p), ir.ctypes.data_as(_i64p),
                                                    _dptr(pr), pcap, C.byref(out)))
        else:
            Cd = np.ascontiguousarray(Cmat, dtype=np.float64)
            _check(lib.msdp_create_onlyunitdiag_dense(n, _dptr(Cd), pcap, C.byref(out)))
        return cls(out.value, KIND_ONLYUNITDIAG, n)

    @classmethod
    def onlyunitdiag_lowrank(cls, Cs, V, s, pcap=32):
        """C = Cs + V diag(s) V' held implicitly (msdp_create_onlyunitdiag_csc_lowrank): Cs sparse symmetric n x n, V n x q
        with 1 <= q <= LOWRANK_MAX (a vector counts as one column), s of length q.  q is checked by the library."""
        import scipy.sparse as sp
        lib = load()
        out = C.c_void_p()
        n = Cs.shape[0]
        Cc = sp.csc_matrix(Cs)
        Cc.sort_indices()
        V = np.asarray(V, dtype=np.float64)
        if V.ndim == 1:
            V = V[:, None]
        s = np.ascontiguousarray(np.atleast_1d(s), dtype=np.float64)
        if V.ndim != 2 or V.shape[0] != n or s.shape != (V.shape[1],):
            raise ValueError(f"V must be {n} x q and s of length q, not {V.shape} and {s.shape}")
        Vf = np.asfortranarray(V)                      # n x q column-major
        jc = np.ascontiguousarray(Cc.indptr, dtype=np.int64)
        ir = np.ascontiguousarray(Cc.indices, dtype=np.int64)
        pr = np.ascontiguousarray(Cc.data, dtype=np.float64)
        _check(lib.msdp_create_onlyunitdiag_csc_lowrank(n, jc.ctypes.data_as(_i64p), ir.ctypes.data_as(_i64p), _dptr(pr),
                                                        V.shape[1], Vf.ctypes.data_as(_dp), _dptr(s), pcap, C.byref(out)))
        return cls(out.value, KIND_ONLYUNITDIAG, n)

    @classmethod
    def onlyunitdiag_hermitian(cls, Cmat, pcap=32):
        """min <C, X> over Hermitian PSD X with unit diagonal, C a scipy sparse complex Hermitian matrix
        (msdp_create_onlyunitdiag_csc_hermitian).  C == C^H is checked exactly.  On this handle set_point, get_point, rgrad,
        hessvec, proj, retr and the V of escape_eigs take or return complex (n, p) arrays (they cross the C ABI as their real
        views of width 2p); cost and get_z stay real.  pcap counts complex columns."""
        Cc = hermitian_csc(Cmat)
        lib = load()
        out = C.c_void_p()
        n = Cc.shape[0]
        jc = np.ascontiguousarray(Cc.indptr, dtype=np.int64)
        ir = np.ascontiguousarray(Cc.indices, dtype=np.int64)
        val = np.ascontiguousarray(Cc.data, dtype=np.complex128).view(np.float64)      # nnz (re, im) pairs
        _check(lib.msdp_create_onlyunitdiag_csc_hermitian(n, jc.ctypes.data_as(_i64p), ir.ctypes.data_as(_i64p), _dptr(val), pcap,
                                                          C.byref(out)))
        h = cls(out.value, KIND_ONLYUNITDIAG, n)
        h.hermitian = True
        return h

    @classmethod
    def _block_csc(cls, create, Cmat, d, efree, pcap):
        """A block-CSR handle from a symmetric scipy sparse (or dense) matrix through `create` (one of the two msdp_create_*_csc
        calls with the signature (N, d, jc, ir, val, pcap, out)): blocks of d + efree rows, efree of them free."""
        import scipy.sparse as sp
        lib = load()
        out = C.c_void_p()
        Cc = sp.csc_matrix(Cmat, dtype=np.float64)
        Cc.sum_duplicates()
        Cc.sort_indices()
        N = Cc.shape[0]
        jc = np.ascontiguousarray(Cc.indptr, dtype=np.int64)
        ir = np.ascontiguousarray(Cc.indices, dtype=np.int64)
        val = np.ascontiguousarray(Cc.data, dtype=np.float64)
        _check(getattr(lib, create)(N, int(d), jc.ctypes.data_as(_i64p), ir.ctypes.data_as(_i64p), _dptr(val), pcap, C.byref(out)))
        h = cls(out.value, KIND_ONLYUNITDIAG, N)
        h.blk = int(d) + int(efree)
        h.efree = int(efree)
        return h

    @classmethod
    def onlyunitblockdiag(cls, Cmat, d, pcap=32):
        """min <C, X> over PSD X of order N = n d with identity diagonal blocks X_[ii] = I_d, d = 2 or 3
        (msdp_create_onlyunitblockdiag_csc): C a symmetric scipy sparse (or dense) N x N matrix.  Factors are (N, p) arrays whose
        blocks of d consecutive rows are orthonormal; get_z returns the N diagonal entries of the multiplier blocks, get_blockmult
        the blocks.  d, N % d and pcap <= 256 are checked by the library."""
        return cls._block_csc("msdp_create_onlyunitblockdiag_csc", Cmat, d, 0, pcap)

    @classmethod
    def posegraph(cls, Cmat, d, pcap=32):
        """min <C, X> over PSD X of order N = n (d + 1) whose diagonal blocks have the leading d x d part I_d, d = 2 or 3
        (msdp_create_posegraph_csc): C a symmetric scipy sparse (or dense) N x N matrix.  Factors are (N, p) arrays of blocks of
        d orthonormal rows followed by one free row; get_z returns N values (the diagonals of the d x d multiplier blocks, 0 for
        the free rows: their sum is the dual value), get_blockmult the (n, d, d) blocks.  d, N % (d + 1) and pcap <= 256 are
        checked by the library."""
        return cls._block_csc("msdp_create_posegraph_csc", Cmat, d, 1, pcap)

    @classmethod
    def dense_synthetic(cls, n, seed, nranks=1, rank=0, pcap=32):
        """Pre-sharded synthetic dense-C problem (rank `rank` of `nranks` holds its rows only)."""
        lib = load()
        out = C.c_void_p()
        _check(lib.msdp_create_onlyunitdiag_dense_synthetic(n, seed, nranks, rank, pcap, C.byref(out)))
        return cls(out.value, KIND_ONLYUNITDIAG, n)

    def debug_shard(self, nranks, rank):
        """Test-only: rank `rank` of `nranks` without a communicator (sparse C)."""
        _check(self._lib.msdp_debug_shard(self._h, nranks, rank))

    def debug_p2p_self(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        _check(self._lib.msdp_debug_p2p_self(self._h, x.size, _dptr(x), _dptr(out)))
        return out

    def debug_set_full_rows(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        _check(self._lib.msdp_debug_set_full_rows(self._h, _dptr(rows)))

    @classmethod
    def affine(cls, kind, At, b, c, n, pcap=32):
        lib = load()
        out = C.c_void_p()
        Atc = At.tocsc()
        Atc.sort_indices()
        jc = np.ascontiguousarray(Atc.indptr, dtype=np.int64)
        ir = np.ascontiguousarray(Atc.indices, dtype=np.int64)
        pr = np.ascontiguousarray(Atc.data, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        c = np.ascontiguousarray(c, dtype=np.float64)
        _check(lib.msdp_create_affine(kind, n, Atc.shape[1], jc.ctypes.data_as(_i64p), ir.ctypes.data_as(_i64p),
                                      _dptr(pr), _dptr(b), _dptr(c), pcap, C.byref(out)))
        return cls(out.value, kind, n)

    @classmethod
    def multiblock(cls, At, b, c, block_n, nob, pcap=32):
        """Block-diagonal X = diag(X_1..X_nb), unit diagonal on the first `nob` blocks (ManiSDP_multiblock.m).  At is
        (sum n_i^2) x m over the concatenated vecs of the blocks.  The factor is one (N, p) array, N = sum n_i."""
        lib = load()
        out = C.c_void_p()
        Atc = At.tocsc()
        Atc.sort_indices()
        jc = np.ascontiguousarray(Atc.indptr, dtype=np.int64)
        ir = np.ascontiguousarray(Atc.indices, dtype=np.int64)
        pr = np.ascontiguousarray(Atc.data, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        c = np.ascontiguousarray(c, dtype=np.float64)
        bn = np.ascontiguousarray(block_n, dtype=np.int64)
        _check(lib.msdp_create_multiblock(len(bn), bn.ctypes.data_as(_i64p), int(nob), Atc.shape[1], jc.ctypes.data_as(_i64p),
                                          ir.ctypes.data_as(_i64p), _dptr(pr), _dptr(b), _dptr(c), pcap, C.byref(out)))
        return cls(out.value, KIND_MULTIBLOCK, int(bn.sum()))

    @classmethod
    def dual_unitdiag(cls, A, b, c, dAAt, B=None, cf=None, pcap=32):
        """Dual approach, diag(S) = 1 (ManiDSDP_unitdiag.m).  ``A`` is the m x n^2 PSD part (rows = vec(A_k)), ``c`` its
        cost (n^2), ``B`` the m x nf free part with costs ``cf``, ``dAAt = diag(A A')``.  The factor of S is (n, p)."""
        return cls._dual_create(KIND_DUAL_UNITDIAG, A, b, c, dAAt, B, cf, pcap)

    @classmethod
    def dual(cls, A, b, c, dAAt, B=None, cf=None, pcap=32):
        """Generic dual approach (ManiDSDP.m): the data of :meth:`dual_unitdiag`, S = Y Y' with Y (n, p) on the
        Euclidean manifold."""
        return cls._dual_create(KIND_DUAL, A, b, c, dAAt, B, cf, pcap)

    @classmethod
    def _dual_create(cls, kind, A, b, c, dAAt, B, cf, pcap):
        import scipy.sparse as sp
        lib = load()
        out = C.c_void_p()
        Atc = sp.csc_matrix(sp.csr_matrix(A).T)
        Atc.sort_indices()
        n = int(round(np.sqrt(Atc.shape[0])))
        jc = np.ascontiguousarray(Atc.indptr, dtype=np.int64)
        ir = np.ascontiguousarray(Atc.indices, dtype=np.int64)
        pr = np.ascontiguousarray(Atc.data, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        c = np.ascontiguousarray(c, dtype=np.float64)
        d = np.ascontiguousarray(dAAt, dtype=np.float64)
        nf = 0 if B is None else int(B.shape[1])
        if nf:
            Bc = sp.csc_matrix(B)
            Bc.sort_indices()
            bjc = np.ascontiguousarray(Bc.indptr, dtype=np.int64)
            bir = np.ascontiguousarray(Bc.indices, dtype=np.int64)
            bpr = np.ascontiguousarray(Bc.data, dtype=np.float64)
            cfv = np.ascontiguousarray(cf, dtype=np.float64)
            args = (bjc.ctypes.data_as(_i64p), bir.ctypes.data_as(_i64p), _dptr(bpr), _dptr(cfv))
        else:
            args = (None, None, None, None)
        create = lib.msdp_create_dual if kind == KIND_DUAL else lib.msdp_create_dual_unitdiag
        _check(create(n, Atc.shape[1], jc.ctypes.data_as(_i64p), ir.ctypes.data_as(_i64p), _dptr(pr), _dptr(d),
                      _dptr(b), _dptr(c), nf, *args, pcap, C.byref(out)))
        hd = cls(out.value, kind, n)
        hd.m = Atc.shape[1]
        hd.nf = nf
        return hd

    @classmethod
    def dual_multiblock(cls, A, b, c, dAAt, block_n, nob, B=None, cf=None, pcap=32):
        """Multiblock dual approach (ManiDSDP_multiblock.m): ``A`` is the m x sum(n_i^2) PSD part (rows = the concatenated
        column-major vecs of the blocks), ``c`` its cost, ``B`` / ``cf`` the free part, ``dAAt = diag(A A')``; S_i = Y_i Y_i'
        with unit diagonal on the first ``nob`` blocks.  The factor is one (N, p) array, N = sum n_i, zero beyond each block's
        own width (as :meth:`multiblock`)."""
        import scipy.sparse as sp
        lib = load()
        out = C.c_void_p()
        Atc = sp.csc_matrix(sp.csr_matrix(A).T)
        Atc.sort_indices()
        jc = np.ascontiguousarray(Atc.indptr, dtype=np.int64)
        ir = np.ascontiguousarray(Atc.indices, dtype=np.int64)
        pr = np.ascontiguousarray(Atc.data, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        c = np.ascontiguousarray(c, dtype=np.float64)
        d = np.ascontiguousarray(dAAt, dtype=np.float64)
        bn = np.ascontiguousarray(block_n, dtype=np.int64)
        nf = 0 if B is None else int(B.shape[1])
        if nf:
            Bc = sp.csc_matrix(B)
            Bc.sort_indices()
            bjc = np.ascontiguousarray(Bc.indptr, dtype=np.int64)
            bir = np.ascontiguousarray(Bc.indices, dtype=np.int64)
            bpr = np.ascontiguousarray(Bc.data, dtype=np.float64)
            cfv = np.ascontiguousarray(cf, dtype=np.float64)
            args = (bjc.ctypes.data_as(_i64p), bir.ctypes.data_as(_i64p), _dptr(bpr), _dptr(cfv))
        else:
            args = (None, None, None, None)
        _check(lib.msdp_create_dual_multiblock(len(bn), bn.ctypes.data_as(_i64p), int(nob), Atc.shape[1], jc.ctypes.data_as(_i64p),
                                               ir.ctypes.data_as(_i64p), _dptr(pr), _dptr(d), _dptr(b), _dptr(c), nf, *args, pcap,
                                               C.byref(out)))
        hd = cls(out.value, KIND_DUAL_MULTIBLOCK, int(bn.sum()))
        hd.m = Atc.shape[1]
        hd.nf = nf
        hd.zrows = int(bn[:int(nob)].sum())
        return hd

    def dual_set_penalty(self, sigma, w=None):
        w = np.ascontiguousarray(w if w is not None else np.zeros(max(self.nf, 1)), dtype=np.float64)
        _check(self._lib.msdp_dual_set_penalty(self._h, float(sigma), _dptr(w)))

    def dual_outer_step(self):
        """Outer step of ManiDSDP_unitdiag.m:70-81 (ManiDSDP.m:66-77) on the device: returns (b'y, <C,eX>, |As|^2, Af, z);
        z is None for the generic kind."""
        scal = np.zeros(3)
        Af = np.zeros(max(self.nf, 1))
        z = np.zeros(self.n) if self.kind == KIND_DUAL_UNITDIAG else None
        if self.kind == KIND_DUAL_MULTIBLOCK:
            z = np.zeros(max(self.zrows, 1))            # the rows of the first nob blocks (ManiDSDP_multiblock.m:115-118)
        _check(self._lib.msdp_dual_outer_step(self._h, _dptr(scal), _dptr(Af), _dptr(z) if z is not None else None))
        if self.kind == KIND_DUAL_MULTIBLOCK:
            z = z[:self.zrows]
        return float(scal[0]), float(scal[1]), float(scal[2]), Af[:self.nf], z

    def dual_g_identity(self):
        """Whether the setup proved D\\A*A' = I (the Hess-vec of the generic dual kind then skips the G terms)."""
        g = C.c_int32(0)
        _check(self._lib.msdp_dual_info(self._h, C.byref(g)))
        return bool(g.value)

    def dual_get_y(self):
        y = np.zeros(self.m)
        _check(self._lib.msdp_dual_get_y(self._h, _dptr(y)))
        return y

    def close(self):
        if self._h is not None and self._h.value:
            self._lib.msdp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- layout helpers
    def _to_boundary(self, Y):
        if self.hermitian:                        # complex (n, p) -> its real view (n, 2p)
            Y = np.ascontiguousarray(Y, dtype=np.complex128)
            return Y.view(np.float64).reshape(Y.shape[0], -1)
        Y = np.asarray(Y, dtype=np.float64)
        if self.kind in (KIND_UNITTRACE, KIND_GENERIC, KIND_DUAL):
            return np.asfortranarray(Y)           # MATLAB n x p column-major
        return np.ascontiguousarray(Y)            # bytes of MATLAB p x n column-major

    def _empty(self):
        # zero-initialised: a row-sharded handle (comm_init / debug_shard) only writes its own rows
        if self.hermitian:
            return np.zeros((self.n, 2 * self.p), dtype=np.float64, order="C")
        if self.kind in (KIND_UNITTRACE, KIND_GENERIC, KIND_DUAL):
            return np.zeros((self.n, self.p), dtype=np.float64, order="F")
        return np.zeros((self.n, self.p), dtype=np.float64, order="C")

    def _from_boundary(self, out):
        out = np.ascontiguousarray(out)
        return out.view(np.complex128) if self.hermitian else out

    # ---- point I/O
    def set_point(self, Y):
        Yb = self._to_boundary(Y)
        assert Yb.shape[0] == self.n
        self.p = Yb.shape[1] // 2 if self.hermitian else Yb.shape[1]
        _check(self._lib.msdp_set_point(self._h, Yb.shape[1], _dptr(Yb)))

    def get_point(self):
        out = self._empty()
        _check(self._lib.msdp_get_point(self._h, _dptr(out)))
        return self._from_boundary(out)

    def get_point_all(self):
        """All n rows of the resident point on every rank of a row-sharded handle (one all-gather + download)."""
        out = self._empty()
        _check(self._lib.msdp_get_point_all(self._h, _dptr(out)))
        return np.ascontiguousarray(out)

    def factor_gram(self):
        """p x p Gram matrix of the columns of the resident factor (computed on the device)."""
        G = np.zeros((self.p, self.p))
        _check(self._lib.msdp_factor_gram(self._h, _dptr(G)))
        return G

    def factor_rotate(self, Q):
        """Resident factor <- factor @ Q (Q: p x r): the rank cut, on the device."""
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        assert Q.shape[0] == self.p
        _check(self._lib.msdp_factor_rotate(self._h, Q.shape[1], _dptr(Q)))
        self.p = Q.shape[1]

    def factor_append(self, V, alpha, normalize=True):
        """Resident factor <- [factor, alpha*V] (V: n x k), rows renormalised (oblique kinds), on the device."""
        Vf = np.asfortranarray(V, dtype=np.float64)
        assert Vf.shape[0] == self.n
        _check(self._lib.msdp_factor_append(self._h, Vf.shape[1], _dptr(Vf), float(alpha), 1 if normalize else 0))
        self.p += Vf.shape[1]

    # ---- the Hermitian kind's factor between two trustregions() calls (msdp_hfactor_*); p counts complex columns
    def hfactor_gram(self):
        """Y^H Y of the resident factor of an onlyunitdiag_hermitian handle: a complex p x p array (computed on the device)."""
        pc = self.p if self.hermitian else max(self.p // 2, 1)      # (any other handle: the library refuses the call)
        G = np.zeros((pc, pc), dtype=np.complex128)
        _check(self._lib.msdp_hfactor_gram(self._h, _dptr(G.view(np.float64))))
        return G

    def hfactor_rotate(self, Q):
        """Resident factor <- factor @ Q (Q: p x r complex): the rank cut, on the device (msdp_hfactor_rotate)."""
        Q = np.ascontiguousarray(Q, dtype=np.complex128)
        if Q.ndim != 2 or (self.hermitian and self.p and Q.shape[0] != self.p):   # (no point yet, or another kind: the library refuses the call)
            raise ValueError(f"hfactor_rotate: Q must be p x r with p = {self.p}, not {Q.shape}")
        _check(self._lib.msdp_hfactor_rotate(self._h, Q.shape[1], _dptr(Q.view(np.float64))))
        self.p = Q.shape[1]

    def hfactor_append(self, V, alpha):
        """Resident factor <- [factor, alpha * V] (V: n x k complex) with the rows renormalised, on the device
        (msdp_hfactor_append)."""
        Vf = np.asfortranarray(V, dtype=np.complex128)
        if Vf.ndim != 2 or Vf.shape[0] != self.n:
            raise ValueError(f"hfactor_append: V must be n x k with n = {self.n}, not {Vf.shape}")
        Vb = np.ascontiguousarray(Vf.T)                           # k columns of n (re, im) pairs
        _check(self._lib.msdp_hfactor_append(self._h, Vf.shape[1], _dptr(Vb.view(np.float64)), float(alpha)))
        self.p += Vf.shape[1]

    def round_phases(self, R, M=0, sweeps=0, phases=False):
        """Rounding of the resident point of an onlyunitdiag_hermitian handle to phases on the device (msdp_round_phases):
        z_t = round(Y r_t) for the rows r_t of R (trials x p complex, trials a multiple of 64) to the unit circle (M = 0) or the
        M-th roots of unity, the values z_t^H C z_t, then up to `sweeps` Gauss-Seidel sweeps of coordinate minimisation.
        Returns a dict: values0 (after the rounding), values (final), info (2 x trials/64: sweeps run and changes of the last
        sweep, per word of 64 trials), best (trial of the smallest value), z (its phases, complex n), k (their table indices,
        int32; M >= 2 only) and, when asked for, phases (all final phases, a (trials/64, n, 64) complex array)."""
        R = np.ascontiguousarray(R, dtype=np.complex128)
        if R.ndim != 2 or (self.hermitian and self.p and R.shape[1] != self.p):   # (no point yet, or another kind: the library refuses the call)
            raise ValueError(f"round_phases: R must be trials x p = {self.p}, not {R.shape}")
        T = R.shape[0]
        W = max(T // 64, 1)
        values0, values = np.zeros(T), np.zeros(T)
        info = np.zeros((2, W), dtype=np.int32)
        P = np.zeros((W, self.n, 64), dtype=np.complex128) if phases else None
        z = np.zeros(self.n, dtype=np.complex128)
        k = np.zeros(self.n, dtype=np.int32) if M else None
        best = C.c_int32()
        _check(self._lib.msdp_round_phases(self._h, int(M), T, _dptr(R.view(np.float64)), int(sweeps), _dptr(values0), _dptr(values),
                                           info.ctypes.data_as(_i32p), _dptr(P.view(np.float64)) if phases else None,
                                           C.byref(best), _dptr(z.view(np.float64)), k.ctypes.data_as(_i32p) if M else None))
        out = {"values0": values0, "values": values, "info": info, "best": best.value, "z": z}
        if M:
            out["k"] = k
        if phases:
            out["phases"] = P
        return out

    # ---- the block kinds' factor between two trustregions() calls, and their rounding (msdp_blockfactor_*)
    def blockfactor_gram(self):
        """p x p Gram matrix Y'Y of the resident factor of an onlyunitblockdiag / posegraph handle (computed on the device)."""
        G = np.zeros((self.p, self.p))
        _check(self._lib.msdp_blockfactor_gram(self._h, _dptr(G)))
        return G

    def blockfactor_rotate(self, Q):
        """Resident factor <- polar_blocks(factor @ Q) (Q: p x r, d <= r <= p), on the device.  Returns the number of degenerate
        blocks; when it is not 0 the resident point and its width are unchanged (msdp_blockfactor_rotate)."""
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        if Q.ndim != 2 or (self.p and Q.shape[0] != self.p):      # (no point yet: the library refuses the call)
            raise ValueError(f"blockfactor_rotate: Q must be p x r with p = {self.p}, not {Q.shape}")
        ndeg = C.c_int32()
        _check(self._lib.msdp_blockfactor_rotate(self._h, Q.shape[1], _dptr(Q), C.byref(ndeg)))
        if ndeg.value == 0:
            self.p = Q.shape[1]
        return ndeg.value

    def blockfactor_append(self, V, alpha):
        """Resident factor <- polar_blocks([factor, alpha * V]) (V: N x k), on the device.  Returns the number of degenerate
        blocks; when it is not 0 the resident point and its width are unchanged (msdp_blockfactor_append)."""
        Vf = np.asfortranarray(V, dtype=np.float64)
        if Vf.ndim != 2 or Vf.shape[0] != self.n:
            raise ValueError(f"blockfactor_append: V must be N x k with N = {self.n}, not {Vf.shape}")
        ndeg = C.c_int32()
        _check(self._lib.msdp_blockfactor_append(self._h, Vf.shape[1], _dptr(Vf), float(alpha), C.byref(ndeg)))
        if ndeg.value == 0:
            self.p += Vf.shape[1]
        return ndeg.value

    def round_blocks(self, W=None):
        """Rotations (and positions, posegraph) from the resident factor, on the device (msdp_blockfactor_round): Z_i = Y_i W for
        W p x d -- None: the top-d eigenvectors of blockfactor_gram() --, the determinant sign by the majority of the blocks,
        R_i the nearest rotation to Z_i.  Returns (R, t, flipped, ndeg): R (n, d, d), t (n, d) or None, flipped 1 when the global
        reflection was applied, ndeg the number of degenerate blocks (not 0: R and t are not to be used)."""
        d = max(self.blk - self.efree, 1)                 # (a handle without blocks: the library refuses the call)
        if W is None:
            w, Q = np.linalg.eigh(self.blockfactor_gram())
            W = Q[:, np.argsort(w)[::-1][:d]]
        W = np.ascontiguousarray(W, dtype=np.float64)
        if self.blk and self.p and W.shape != (self.p, d):
            raise ValueError(f"round_blocks: W must be p x d = {self.p} x {d}, not {W.shape}")
        nb = self.n // self.blk if self.blk else 0
        R = np.zeros((max(nb, 1), d, d))
        t = np.zeros((max(nb, 1), d)) if self.efree else None
        flipped, ndeg = C.c_int32(), C.c_int32()
        _check(self._lib.msdp_blockfactor_round(self._h, _dptr(W), _dptr(R), _dptr(t) if self.efree else None,
                                                C.byref(flipped), C.byref(ndeg)))
        return R, t, flipped.value, ndeg.value

    def set_multipliers(self, y, sigma):
        y = np.ascontiguousarray(y, dtype=np.float64)
        _check(self._lib.msdp_set_multipliers(self._h, _dptr(y), float(sigma)))

    # ---- hot path
    def rtr(self, opts):
        st = RtrStats()
        _check(self._lib.msdp_rtr(self._h, C.byref(opts), C.byref(st)))
        return st

    # ---- fine-grained
    def cost(self):
        f = C.c_double()
        _check(self._lib.msdp_cost(self._h, C.byref(f)))
        return f.value

    def rgrad(self):
        out = self._empty()
        _check(self._lib.msdp_rgrad(self._h, _dptr(out)))
        return self._from_boundary(out)

    def _vec_op(self, fn, U):
        Ub = self._to_boundary(U)
        out = self._empty()
        _check(fn(self._h, _dptr(Ub), _dptr(out)))
        return self._from_boundary(out)

    def hessvec(self, U):
        return self._vec_op(self._lib.msdp_hessvec, U)

    def proj(self, U):
        return self._vec_op(self._lib.msdp_proj, U)

    def retr(self, U):
        return self._vec_op(self._lib.msdp_retr, U)

    def precon_apply(self, R):
        """tangent_Y(blockdiag(M_i^-1) R) at the resident point of a posegraph handle with set_option("precon", 1): the
        preconditioner of its tCG (msdp_precon_apply), M_i = sym(C_[ii])."""
        return self._vec_op(self._lib.msdp_precon_apply, R)

    def round_hyperplane(self, R, sweeps=0, masks=False):
        """Hyperplane rounding of the resident point on the device (msdp_round_hyperplane): x_t = sign(Y r_t) for the rows r_t
        of R (trials x p, trials a multiple of 64), the values x_t' C x_t, then up to `sweeps` sweeps of 1-opt local search.
        Returns a dict: values0 (after the rounding), values (final), info (2 x trials/64: sweeps run and flips of the last
        sweep, per word of 64 trials), best (trial of the smallest value), x (its +1/-1 vector, int8) and masks (trials/64 x n
        uint64 sign bits, bit t of masks[w, i] set when x_i = -1 in trial 64 w + t; None unless asked for)."""
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.ndim != 2 or (self.p and R.shape[1] != self.p and not self.hermitian):   # (no point yet, or a Hermitian handle: the library refuses the call)
            raise ValueError(f"round_hyperplane: R must be trials x p = {self.p}, not {R.shape}")
        T = R.shape[0]
        W = max(T // 64, 1)
        values0, values = np.zeros(T), np.zeros(T)
        info = np.zeros((2, W), dtype=np.int32)
        M = np.zeros((W, self.n), dtype=np.uint64) if masks else None
        x = np.zeros(self.n, dtype=np.int8)
        best = C.c_int32()
        _check(self._lib.msdp_round_hyperplane(self._h, T, _dptr(R), int(sweeps), _dptr(values0), _dptr(values),
                                               info.ctypes.data_as(_i32p), M.ctypes.data_as(_P(C.c_uint64)) if masks else None,
                                               C.byref(best), x.ctypes.data_as(_P(C.c_int8))))
        return {"values0": values0, "values": values, "info": info, "best": best.value, "x": x, "masks": M}

    def round_coloring(self):
        """(ncolors, color): the greedy first-fit colouring of the rows of C behind set_option("round_order", 1)
        (msdp_round_coloring) -- color an int32 array of n entries; computed once per handle, no resident point needed."""
        nc = C.c_int32()
        color = np.zeros(self.n, dtype=np.int32)
        _check(self._lib.msdp_round_coloring(self._h, C.byref(nc), color.ctypes.data_as(_i32p)))
        return nc.value, color

    def debug_get_tcg_step(self):
        """(eta, Heta) of the last tCG solve (test hook, see msdp_debug_get_tcg_step)."""
        eta, heta = self._empty(), self._empty()
        _check(self._lib.msdp_debug_get_tcg_step(self._h, _dptr(eta), _dptr(heta)))
        return np.ascontiguousarray(eta), np.ascontiguousarray(heta)

    def get_z(self):
        z = np.zeros(self.n)
        _check(self._lib.msdp_get_z(self._h, _dptr(z)))
        return z

    def get_blockmult(self):
        """The multiplier blocks Lambda_i = sym((C Y)_i Y_i') of an onlyunitblockdiag handle (of a posegraph handle: of the d
        rotation rows of every block): an (n, d, d) array."""
        nb = self.n // self.blk if self.blk else 0
        d = max(self.blk - self.efree, 1)                  # the multiplier blocks are of the order of the orthonormal rows
        Lam = np.zeros((max(nb, 1), d, d))
        _check(self._lib.msdp_get_blockmult(self._h, _dptr(Lam)))
        return Lam

    def get_z_all(self):
        z = np.zeros(self.n)
        _check(self._lib.msdp_get_z_all(self._h, _dptr(z)))
        return z

    def linesearch_cost(self, U, alpha):
        v = C.c_double()
        if U is None:
            _check(self._lib.msdp_linesearch_cost(self._h, None, 0.0, C.byref(v)))
        else:
            Ub = self._to_boundary(U)
            _check(self._lib.msdp_linesearch_cost(self._h, _dptr(Ub), float(alpha), C.byref(v)))
        return v.value

    def linesearch_accept(self):
        _check(self._lib.msdp_linesearch_accept(self._h))

    def escape_eigs(self, k, tol=1e-10, maxit=500):
        """(lam, V, lambda_max, steps) of msdp_escape_eigs: the k bottom eigenpairs of S = C - diag(z) at the resident point
        (missing pairs: +inf and a zero vector; escape_info() says how many are real).  V is (n, k), complex on an
        onlyunitdiag_hermitian handle.  Which eigen-solver ran: escape_method().  A Hermitian handle takes the Lanczos path on the
        real view unless set_option("escape_method", 2) asks for the block eigen-solver on a complex panel (single rank,
        n >= 256, k <= 56); maxit is then the budget of filter steps.  An onlyunitblockdiag or posegraph handle takes the Lanczos
        path unless set_option("escape_method", 2) asks for the block eigen-solver on block storage (N >= 256, k <= 64)."""
        lam = np.empty(k)
        V = np.empty((self.n, k), order="F", dtype=np.complex128 if self.hermitian else np.float64)   # complex: (re, im) pairs, column by column
        lmax = C.c_double()
        its = C.c_int32()
        _check(self._lib.msdp_escape_eigs(self._h, k, tol, maxit, _dptr(lam), _dptr(V), C.byref(lmax), C.byref(its)))
        return lam, np.ascontiguousarray(V), lmax.value, its.value

    def escape_eigs_matrix(self, S, k, tol=1e-10, maxit=20000):
        """k bottom eigenpairs and lambda_max of an explicit dense symmetric S (device Lanczos, dense GEMV)."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        lam = np.empty(k)
        V = np.empty((self.n, k), order="F")
        lmax = C.c_double()
        its = C.c_int32()
        _check(self._lib.msdp_escape_eigs_matrix(self._h, _dptr(S), k, tol, maxit, _dptr(lam), _dptr(V), C.byref(lmax),
                                                 C.byref(its)))
        return lam, np.ascontiguousarray(V), lmax.value, its.value

    def escape_info(self):
        """(nvalid, converged, residual) of the last escape_eigs* call: how many returned pairs are real, whether
        every Lanczos run passed a stop test, and the worst relative residual of the runs that did not."""
        nv, cv, res = C.c_int32(), C.c_int32(), C.c_double()
        _check(self._lib.msdp_escape_info(self._h, C.byref(nv), C.byref(cv), C.byref(res)))
        return nv.value, bool(cv.value), res.value

    def set_option(self, name, value):
        """Run-time switch of this handle (see msdp_set_option in include/manisdp_hip.h)."""
        _check(self._lib.msdp_set_option(self._h, name.encode(), int(value)))

    def time_collective(self, which, reps=200):
        """Average stream time (us) of one collective call (msdp_debug_time_collective)."""
        v = C.c_double(0)
        _check(self._lib.msdp_debug_time_collective(self._h, which, reps, C.byref(v)))
        return v.value

    def collective_calls(self):
        """Collective calls issued on this handle's communicator so far (a grouped RCCL launch counts once)."""
        v = C.c_int64(0)
        _check(self._lib.msdp_debug_collective_calls(self._h, C.byref(v)))
        return int(v.value)

    def escape_method(self):
        """Which eigen-solver the last escape call ran: 1 = block Chebyshev-filtered subspace iteration, 0 = Lanczos."""
        v = C.c_int32()
        _check(self._lib.msdp_escape_method(self._h, C.byref(v)))
        return v.value

    def be_step_blk(self, b, lpr, Xin, Xio, f1, cs, f2, prev):
        """One launch of the block eigen-solver's filter step on block storage (msdp_debug_be_step_blk) at the resident point of a
        unit-block-diagonal or pose-graph handle: returns f1 * (S @ Xin) - f1 * cs * Xin - f2 * Xio (prev false: without the last
        term) for (N, b) panels, b = 32 / 64 / 128, with lpr lanes per block.  Xio is not modified."""
        Xin = np.ascontiguousarray(Xin, dtype=np.float64)
        out = np.array(Xio, dtype=np.float64, order="C")
        if Xin.shape != (self.n, int(b)) or out.shape != Xin.shape:
            raise ValueError(f"be_step_blk: panels must be ({self.n}, {int(b)})")
        _check(self._lib.msdp_debug_be_step_blk(self._h, int(b), int(lpr), _dptr(Xin), _dptr(out), float(f1), float(cs), float(f2), 1 if prev else 0))
        return out

    def ritz_stages(self):
        """(device, host, fallback): Rayleigh-Ritz stages of the block eigen-solver on this handle so far whose dense algebra ran
        on the device (option escape_rr = 1), on the host, and on the host after the device kernel handed the stage back."""
        d, hst, f = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self._lib.msdp_debug_ritz_stages(self._h, C.byref(d), C.byref(hst), C.byref(f)))
        return int(d.value), int(hst.value), int(f.value)

    def escape_lower_bound(self):
        """Lower estimate of lambda_min(S) from the last escape call; -inf unless that call was cold-started and
        undeflated (see msdp_escape_lower_bound in include/manisdp_hip.h: an estimate, not a certificate)."""
        v = C.c_double()
        _check(self._lib.msdp_escape_lower_bound(self._h, C.byref(v)))
        return v.value

    def get_kind(self):
        k = C.c_int32()
        _check(self._lib.msdp_get_kind(self._h, C.byref(k)))
        return k.value

    def get_dual_slack_block(self, row0, nb):
        """The nb x nb diagonal block of S that starts at row0 (multiblock: eig(S_i) block by block)."""
        S = np.empty((nb, nb))
        _check(self._lib.msdp_get_dual_slack_block(self._h, int(row0), int(nb), _dptr(S)))
        return S

    def get_dual_slack(self):
        """Dense S (n x n) of the last al_dual call."""
        S = np.empty((self.n, self.n))
        _check(self._lib.msdp_get_dual_slack(self._h, _dptr(S)))
        return S

    # ---- AL bookkeeping on the device (affine handles)
    def block_eigs(self, row0, nblk, k, method=0):
        """eig of the diagonal blocks (row0[b], nblk[b]) of the dual slack of the last al_dual call, on the device (msdp_block_eigs):
        returns (w, V) -- all eigenvalues, block after block and ascending inside a block; V[(rows of block b), c] = eigenvector of
        the block's c-th smallest eigenvalue, c < k.  method: 0 = tridiagonalisation + bisection + inverse iteration (k <= 8), else
        Jacobi; 1 = Jacobi; 2 = the tridiagonal method."""
        r0 = np.ascontiguousarray(row0, dtype=np.int64)
        nb = np.ascontiguousarray(nblk, dtype=np.int64)
        tot = int(nb.sum())
        w = np.empty(tot)
        V = np.empty((tot, max(int(k), 1)))
        _check(self._lib.msdp_block_eigs(self._h, len(nb), r0.ctypes.data_as(_i64p), nb.ctypes.data_as(_i64p), int(k), int(method), _dptr(w), _dptr(V)))
        return w, V[:, :int(k)]

    def block_eigs_large(self, row0, nblk, k):
        """block_eigs for blocks of order up to 1024 (msdp_block_eigs_large: a group of workgroups per block of order > 256, the
        tridiagonal method, k <= 8): the same (w, V).  A block's results do not depend on the other blocks of the call."""
        r0 = np.ascontiguousarray(row0, dtype=np.int64)
        nb = np.ascontiguousarray(nblk, dtype=np.int64)
        tot = int(nb.sum())
        w = np.empty(tot)
        V = np.empty((tot, max(int(k), 1)))
        _check(self._lib.msdp_block_eigs_large(self._h, len(nb), r0.ctypes.data_as(_i64p), nb.ctypes.data_as(_i64p), int(k), _dptr(w), _dptr(V)))
        return w, V[:, :int(k)]

    def block_reshape(self, row0, nblk, p, w, V, theta, strict, delta, alpha, min_facsize, mode):
        """Rank cut and escape widening of all blocks of the resident multiblock factor on the device (msdp_block_reshape;
        ManiSDP_multiblock.m:109-147): ``p`` the blocks' widths, ``w`` / ``V`` their eig(S_i) as block_eigs returns them.  Returns
        (p_out, r_out, nne_out, U) -- U (N, max p_out) in mode 1, else None -- and updates ``self.p``."""
        r0 = np.ascontiguousarray(row0, dtype=np.int64); nb = np.ascontiguousarray(nblk, dtype=np.int64)
        pin = np.ascontiguousarray(p, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float64); V = np.ascontiguousarray(V, dtype=np.float64)
        k = int(V.shape[1]) if V.ndim == 2 else 0
        assert len(r0) == len(nb) == len(pin) and w.shape == (int(nb.sum()),) and (k == 0 or V.shape[0] == w.size)
        out = [np.zeros(max(len(nb), 1), dtype=np.int32) for _ in range(3)]
        # mode 1: room for the widest U the call can produce (the library writes N x max p_out of it)
        U = np.zeros(self.n * (int(pin.max(initial=1)) + int(delta))) if int(mode) == 1 else None
        _check(self._lib.msdp_block_reshape(self._h, len(nb), r0.ctypes.data_as(_i64p), nb.ctypes.data_as(_i64p), pin.ctypes.data_as(_i32p),
                                            _dptr(w), _dptr(V) if k else None, k, float(theta), int(bool(strict)), int(delta), float(alpha),
                                            int(min_facsize), int(mode), *(o.ctypes.data_as(_i32p) for o in out),
                                            _dptr(U) if U is not None else None))
        p_out, r_out, nne_out = (o[:len(nb)] for o in out)
        self.p = int(p_out.max())
        if U is not None:
            U = U[:self.n * self.p].reshape(self.n, self.p).copy()
        return p_out, r_out, nne_out, U

    def block_eigs_large_info(self):
        """(launches, workgroups) of the last block_eigs_large call."""
        a, b = C.c_int32(), C.c_int32()
        _check(self._lib.msdp_block_eigs_large_info(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def al_primal(self, m):
        """obj = c'x and A x (length m) at the resident point, without forming X = YY' on the host."""
        obj = C.c_double()
        Ax = np.empty(m)
        _check(self._lib.msdp_al_primal(self._h, C.byref(obj), _dptr(Ax)))
        return obj.value, Ax

    def al_dual(self, y):
        """Build the dual slack S for the multipliers y on the device; returns z (n values for unitdiag, a scalar for
        unittrace, None for the generic kind).  S stays resident for escape_eigs_dual."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        if self.kind in (KIND_UNITDIAG, KIND_MULTIBLOCK):
            z = np.empty(self.n)
        elif self.kind == KIND_UNITTRACE:
            z = np.empty(1)
        else:
            z = None
        _check(self._lib.msdp_al_dual(self._h, _dptr(y), _dptr(z) if z is not None else None))
        if z is None:
            return None
        return z if self.kind in (KIND_UNITDIAG, KIND_MULTIBLOCK) else float(z[0])

    def escape_eigs_dual(self, k, tol=1e-10, maxit=20000):
        """k bottom eigenpairs and lambda_max of the device-resident S of the last al_dual call."""
        lam = np.empty(k)
        V = np.empty((self.n, k), order="F")
        lmax = C.c_double()
        its = C.c_int32()
        _check(self._lib.msdp_escape_eigs_dual(self._h, k, tol, maxit, _dptr(lam), _dptr(V), C.byref(lmax), C.byref(its)))
        return lam, np.ascontiguousarray(V), lmax.value, its.value

    # ---- multi-GPU
    @staticmethod
    def comm_unique_id():
        buf = (C.c_char * 128)()
        _check(load().msdp_comm_unique_id(C.cast(buf, C.c_void_p)))
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        buf = (C.c_char * 128).from_buffer_copy(uid)
        _check(self._lib.msdp_comm_init(self._h, nranks, rank, C.cast(buf, C.c_void_p)))

    def comm_init_local(self, nranks, rank, group):
        """Member `rank` of an in-process group of `nranks` handles on one GPU (one host thread per handle): the N-rank code
        paths with local stand-ins for the RCCL collectives."""
        _check(self._lib.msdp_comm_init_local(self._h, int(nranks), int(rank), int(group)))

    def comm_init_ipc(self, nranks, rank, name):
        """Member `rank` of a group of `nranks` PROCESSES (ranks on one GPU, or one per GPU with peer access): `name` is a POSIX
        shared-memory name ("/..."), the same on every member, fresh per group (msdp_comm_init_ipc)."""
        _check(self._lib.msdp_comm_init_ipc(self._h, int(nranks), int(rank), name.encode()))

    def local_rows(self):
        a, b = C.c_int64(), C.c_int64()
        _check(self._lib.msdp_local_rows(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def point_snapshot(self):
        _check(self._lib.msdp_point_snapshot(self._h))

    def point_restore(self):
        _check(self._lib.msdp_point_restore(self._h))

    def last_rtr_device_ms(self):
        """Device time of the last rtr() call (HIP events on the library's stream; the fused launch on the fused path)."""
        v = C.c_double()
        _check(self._lib.msdp_debug_last_rtr_device_ms(self._h, C.byref(v)))
        return v.value

    def tcg_path(self):
        """1: persistent single-launch tCG kernel, 0: chunked hipGraph (three kernels per trip)."""
        v = C.c_int32()
        _check(self._lib.msdp_tcg_path(self._h, C.byref(v)))
        return v.value

    def persist_form(self):
        """Trip form of the persistent tCG kernel: 2 one grid reduction per trip, 1 early gather, 0 two reductions, -1 not persistent."""
        v = C.c_int32()
        _check(self._lib.msdp_debug_persist_form(self._h, C.byref(v)))
        if v.value < 0:                                    # the block kinds' kernel (option "block_persist") is a unit of its own
            _check(self._lib.msdp_debug_block_persist_form(self._h, C.byref(v)))
        return v.value

    def fused_own(self):
        """1 where the next fused launch takes the own-column instance of the one-reduction trip (msdp_debug_fused_own), else 0."""
        v = C.c_int32()
        _check(self._lib.msdp_debug_fused_own(self._h, C.byref(v)))
        return v.value

    def fused_plan(self):
        """(G, rw_split) of the next fused launch (msdp_debug_fused_plan): its workgroups (0: no fused launch) and the waves per workgroup
        that compute all three row slots (0: every wave does)."""
        g, s = C.c_int32(), C.c_int32()
        _check(self._lib.msdp_debug_fused_plan(self._h, C.byref(g), C.byref(s)))
        return g.value, s.value

    def trip_form(self):
        """Trip of the chunked tCG at the resident point (msdp_debug_trip_form): 1 the linear-product trip, 2 the two-launch trip,
        3 three launches per trip, 0 a persistent path."""
        v = C.c_int32()
        _check(self._lib.msdp_debug_trip_form(self._h, C.byref(v)))
        return v.value

    def block_persist_plan(self):
        """Plan of the block kinds' persistent tCG at the resident width (msdp_debug_block_persist_plan), as a dict."""
        v = (C.c_int32 * 5)()
        _check(self._lib.msdp_debug_block_persist_plan(self._h, v))
        return dict(zip(("eligible", "lpr", "grid", "slots", "lds"), (int(x) for x in v)))

    def affine_plan(self):
        """What the set-up of a primal affine handle planned and which branch the last Hess-vec / A(.) took, as a dict
        (msdp_debug_affine_plan in include/manisdp_hip.h explains every field)."""
        v = (C.c_int32 * 16)()
        _check(self._lib.msdp_debug_affine_plan(self._h, v))
        return dict(zip(AFFINE_PLAN_FIELDS, v))

    # ---- measurement
    def persist_trace(self, reps=256):
        """Phase stamps of the persistent tCG trip: (array [G, nj, 8] of s_memtime ticks, first traced trip, trip time in ms).
        reps <= 0: the fused launch -- ((stamps of the TR iterations, stamps of the trips of one iteration), 0, call time in ms)."""
        cap = 512 * 64 * 8
        buf = (C.c_uint64 * cap)()
        dims = (C.c_int32 * 3)()
        ms = C.c_double()
        _check(self._lib.msdp_debug_persist_trace(self._h, reps, buf, cap, dims, C.byref(ms)))
        G, nj, j0 = dims[0], dims[1], dims[2]
        a = np.frombuffer(buf, dtype=np.uint64, count=G * nj * 8).reshape(G, nj, 8).astype(np.int64)
        if reps <= 0:
            # the fused launch: stamps of the TR iterations, then the trips of one of them (msdp_pipe.h MSDP_TRACE_KSEL)
            b = np.frombuffer(buf, dtype=np.uint64, count=2 * G * nj * 8)[G * nj * 8:].reshape(G, nj, 8).astype(np.int64)
            return (a, b), j0, ms.value
        return a, j0, ms.value

    def bench_hessvec(self, reps):
        ms, by, fl = C.c_double(), C.c_double(), C.c_double()
        _check(self._lib.msdp_bench_hessvec(self._h, reps, C.byref(ms), C.byref(by), C.byref(fl)))
        return ms.value, by.value, fl.value

    def bench_kernel(self, which, reps):
        ms = C.c_double()
        _check(self._lib.msdp_bench_kernel(self._h, which, reps, C.byref(ms)))
        return ms.value

    def bench_tcg_trip(self, reps):
        ms = C.c_double()
        _check(self._lib.msdp_bench_tcg_trip(self._h, reps, C.byref(ms)))
        return ms.value
