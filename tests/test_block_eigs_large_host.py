"""Host-only checks of the large-block eigen-solver's surface: the header declares msdp_block_eigs_large, the library exports it and
the ctypes table binds it; and solvers._Blocks.spectrum sends blocks of order <= 256 through block_eigs and larger ones through
block_eigs_large, one call each, results merged in block order (a stub handle records the calls)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_large_block_eigs_is_declared_exported_and_bound():
    from manisdp_matlab_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "manisdp_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+msdp_block_eigs_large\s*\(\s*msdp_handle h,\s*int32_t nb,\s*const int64_t\* row0,\s*const int64_t\* nblk,\s*"
                     r"int32_t k,\s*double\* w,\s*double\* V\s*\)\s*;", txt)
    assert re.search(r"#define\s+MSDP_BLOCK_EIGS_LARGE_MAXN\s+1024\b", txt)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "msdp_block_eigs_large") and hasattr(lib, "msdp_block_eigs_large_info")
    restype, argtypes = _lib.SIGNATURES["msdp_block_eigs_large"]
    assert restype is ctypes.c_int and len(argtypes) == 7 and argtypes[4] is ctypes.c_int32
    assert hasattr(_lib.Handle, "block_eigs_large")


class _Stub:
    """Stands in for a handle: eigenvalue r of the whole matrix is r, V[r, c] = 10 r + c; every call is recorded."""

    def __init__(self):
        self.calls = []

    def _answer(self, name, row0, nblk, k, **kw):
        self.calls.append((name, [int(v) for v in row0], [int(v) for v in nblk], int(k), kw))
        rows = np.concatenate([np.arange(r, r + n) for r, n in zip(row0, nblk)]).astype(float)
        return rows.copy(), 10.0 * rows[:, None] + np.arange(int(k))[None, :]

    def block_eigs(self, row0, nblk, k, **kw):
        return self._answer("block_eigs", row0, nblk, k, **kw)

    def block_eigs_large(self, row0, nblk, k):
        return self._answer("block_eigs_large", row0, nblk, k)

    def get_dual_slack_block(self, row0, n):
        self.calls.append(("get_dual_slack_block", int(row0), int(n)))
        return np.diag(np.arange(row0, row0 + n).astype(float))


def _blocks(nset, mode, delta=4):
    from manisdp_matlab_amd import solvers
    h = _Stub()
    return h, solvers._Blocks(h, {"block_eig": mode, "delta": delta}, list(nset), 0, strict_rank=False)


def _in_block_order(geo, dS, vS, delta):
    for i, n in enumerate(geo.nset):
        rows = np.arange(geo.r0[i], geo.r0[i + 1]).astype(float)
        assert np.array_equal(dS[i], rows), i
        assert vS[i].shape[0] == n and np.array_equal(vS[i][:, :delta], 10.0 * rows[:, None] + np.arange(delta)[None, :]), i


def test_spectrum_splits_a_mixed_set_between_the_two_calls():
    h, geo = _blocks([16, 277, 211, 600], "device")
    dinf, ok, (dS, vS) = geo.spectrum(None, None)
    assert h.calls == [("block_eigs", [0, 293], [16, 211], 4, {}), ("block_eigs_large", [16, 504], [277, 600], 4, {})]
    _in_block_order(geo, dS, vS, 4)


def test_spectrum_refuses_an_order_above_1024_on_the_device():
    from manisdp_matlab_amd import _lib
    h, geo = _blocks([16, 1025], "device")
    with pytest.raises(_lib.MsdpError, match="1024"):
        geo.spectrum(None, None)
    h, geo = _blocks([16, 300], "device", delta=9)
    with pytest.raises(_lib.MsdpError, match="delta <= 8"):
        geo.spectrum(None, None)


def test_spectrum_on_the_host_makes_no_device_call():
    h, geo = _blocks([16, 277], "host")
    dinf, ok, (dS, vS) = geo.spectrum(None, None)
    assert [c[0] for c in h.calls] == ["get_dual_slack_block", "get_dual_slack_block"]
    _in_block_order(geo, dS, [np.zeros((n, 4)) + 10.0 * np.arange(geo.r0[i], geo.r0[i + 1])[:, None] + np.arange(4)[None, :] for i, n in enumerate(geo.nset)], 4)


def test_auto_keeps_its_call_for_sixteen_small_blocks():
    nset = [256, 16] * 8
    h, geo = _blocks(nset, "auto")
    dinf, ok, (dS, vS) = geo.spectrum(None, None)
    r0 = np.concatenate([[0], np.cumsum(nset)])[:-1]
    assert h.calls == [("block_eigs", [int(v) for v in r0], nset, 4, {})]
    _in_block_order(geo, dS, vS, 4)
    h, geo = _blocks([16] * 15, "auto")                               # fewer than 16 blocks: the host loop, as before
    geo.spectrum(None, None)
    assert {c[0] for c in h.calls} == {"get_dual_slack_block"}


@pytest.mark.parametrize("nset", [[277] * 16, [1024] * 4, [300] * 100, [16] * 20 + [257]])
def test_auto_keeps_the_host_loop_for_sets_with_blocks_above_256(nset):
    """block_eig = "auto" moves a set to the device only where the device has won a measurement; msdp_block_eigs_large has not been
    timed against the host loop, so every set that contains a block of order above 256 stays on the host."""
    from manisdp_matlab_amd import solvers
    assert not solvers._block_eig_auto(nset)
    h, geo = _blocks(nset, "auto")
    assert not geo.eig_device and not geo.eig_forced
    geo.spectrum(None, None)
    assert {c[0] for c in h.calls} == {"get_dual_slack_block"}
