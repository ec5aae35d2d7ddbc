"""Host-only checks of the surface of the block eigen-solver on the two block kinds (options["escape_method"] of
ManiSDP_onlyunitblockdiag / ManiSDP_posegraph, msdp_debug_be_step_blk, msdp_debug_be_step_blk_instances): the library exports the
step's test entry and _lib binds it, a bad option value is refused before any handle exists, and the (width, lanes) table the GPU
test loops over is the one the library's dispatch is generated from."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from manisdp_matlab_amd import _lib, solvers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_step_entry_points():
    lib = _lib.load()
    for name in ("msdp_debug_be_step_blk", "msdp_debug_be_step_blk_instances"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert callable(_lib.Handle.be_step_blk)
    txt = open(os.path.join(ROOT, "include", "manisdp_hip.h")).read()
    assert "int msdp_debug_be_step_blk(" in txt and "int msdp_debug_be_step_blk_instances(" in txt


def test_step_table_of_the_gpu_test_is_the_librarys():
    from test_gpu_blockeig_blocks import BLK_STEP_INSTANCES
    table = _lib.be_step_blk_instances()
    assert table == BLK_STEP_INSTANCES
    assert len(set(table)) == len(table)
    for width, lpr in table:
        assert width in (32, 64, 128) and width % (2 * lpr) == 0 and 1 <= lpr <= 64


@pytest.mark.parametrize("solver,d,order", [("ManiSDP_onlyunitblockdiag", 2, 2), ("ManiSDP_onlyunitblockdiag", 3, 3),
                                            ("ManiSDP_posegraph", 2, 3), ("ManiSDP_posegraph", 3, 4)])
@pytest.mark.parametrize("bad", [3, -1, "block", 2.0, True, None])
def test_bad_escape_method_is_refused_before_any_handle(solver, d, order, bad, monkeypatch):
    def no_handle(*a, **k):
        raise AssertionError("a handle was built")
    for ctor in ("onlyunitblockdiag", "posegraph"):
        monkeypatch.setattr(_lib.Handle, ctor, staticmethod(no_handle))
    N = 4 * order
    C = sp.csr_matrix(np.ones((N, N)) - np.eye(N))
    with pytest.raises(ValueError, match="escape_method"):
        getattr(solvers, solver)(C, d, {"escape_method": bad}, verbose=False)


@pytest.mark.parametrize("solver", ["ManiSDP_onlyunitblockdiag", "ManiSDP_posegraph"])
def test_escape_method_is_documented_and_no_default(solver):
    assert "escape_method" in getattr(solvers, solver).__doc__
    assert "escape_method" not in solvers.onlyunitblockdiag_defaults(3)
    assert "escape_method" not in solvers.posegraph_defaults(3)
