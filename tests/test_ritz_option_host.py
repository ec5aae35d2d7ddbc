"""Host-only checks of the surface of the device Rayleigh-Ritz stage (options["escape_rr"], msdp_set_option "escape_rr",
msdp_debug_ritz_device): a bad option value is refused before any handle exists, the option is no reference default, the header
documents it, and the kernel-alone entry point refuses the widths it has no instance for without touching a device."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from manisdp_matlab_amd import _lib, solvers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("solver", ["ManiSDP_onlyunitdiag", "ManiSDP_unitdiag", "ManiSDP_unittrace", "ManiSDP"])
def test_bad_escape_rr_option_is_refused_before_any_handle(solver, monkeypatch):
    def no_handle(*a, **k):
        raise AssertionError("a handle was built")
    for ctor in ("onlyunitdiag", "affine", "dense_synthetic"):
        monkeypatch.setattr(_lib.Handle, ctor, staticmethod(no_handle))
    n = 6
    C = sp.csr_matrix(np.ones((n, n)) - np.eye(n))
    if solver == "ManiSDP_onlyunitdiag":
        args = (C,)
    else:
        At = sp.csc_matrix(np.eye(n * n)[:, :1])
        args = (At, np.ones(1), np.zeros(n * n), {"s": n})
    with pytest.raises(ValueError, match="escape_rr"):
        getattr(solvers, solver)(*args, {"escape_rr": "gpu"}, verbose=False)


def test_escape_rr_is_not_a_reference_default():
    assert solvers.DEFAULTS
    for kind, defaults in solvers.DEFAULTS.items():
        assert "escape_rr" not in defaults, kind


def test_header_documents_the_option_and_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "manisdp_hip.h")).read()
    options = txt[:txt.index("int msdp_set_option")]               # the option list is the comment in front of the declaration
    assert re.search(r'\*\s+"escape_rr"\s+0/1', options)
    assert "msdp_debug_ritz_device" in _lib.SIGNATURES and "msdp_debug_ritz_stages" in _lib.SIGNATURES


@pytest.mark.parametrize("b", [16, 128])
def test_kernel_alone_refuses_other_widths(b):
    with pytest.raises(_lib.MsdpError, match=r"error -6: debug_ritz_device: block widths 32 and 64 \(got %d\)" % b):
        _lib.ritz_device(np.eye(b), np.eye(b))
