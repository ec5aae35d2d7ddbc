"""Host-only checks of msdp_block_reshape's surface and of its reference: the restatement in block_reshape_ref.py agrees with the
product's own _Blocks.reshape, takes the rank decisions of the planted cases exactly as an extended-precision evaluation does and
stays within X_DEVIATION of it; the library exports the call; a bad ``block_reshape`` option is refused before any handle exists."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_reshape_ref as R  # noqa: E402

RULES = [dict(theta=1e-2, strict=False), dict(theta=1e-3, strict=True)]          # the primal and the dual kinds' defaults


def _rule(base, **kw):
    out = dict(delta=8, alpha=0.1, min_facsize=2)
    out.update(base)
    out.update(kw)
    return out


def _planted_cases():
    rng = np.random.default_rng(71)
    cases = R.seven_blocks(rng) + list(R.branch_blocks(rng).values()) + R.many_blocks(rng, count=40) + R.wide_uncut_blocks()[2:]
    return cases


def _rel(X, Xref):
    nrm = np.linalg.norm(Xref)
    return float(np.linalg.norm(X - Xref)) / nrm if nrm > 0 else float(np.linalg.norm(X - Xref))


def test_restatement_agrees_with_the_products_host_loop():
    """Random block sets (random orders, widths, kept ranks and eigen-data; the factors are planted so that the two sides, which
    form the Gram matrix by different calls, cannot disagree on a rank) through _Blocks.reshape without a handle and through the
    restatement: same widths, X_i within X_TOL, U_i exact."""
    from manisdp_matlab_amd import solvers
    rng = np.random.default_rng(5)
    for trial in range(6):
        nob = int(rng.integers(0, 4))
        nset = [int(v) for v in rng.integers(1, 30, size=6)]
        p = [int(rng.integers(1, min(n, 9) + 1)) for n in nset]
        for base in RULES:
            for ls in (0, 1):
                o = dict(solvers.DEFAULTS["multiblock"], theta=base["theta"], line_search=ls)
                geo = solvers._Blocks(None, o, nset, nob, strict_rank=base["strict"])
                Yb = [R.planted(n, pi, int(rng.integers(1, pi + 1)), rng) for n, pi in zip(nset, p)]
                eig = [R.eigen_data(n, int(rng.integers(0, 12)), n, rng) for n in nset]
                newY, newU, newp = geo.reshape(Yb, p, None, ([e[0] for e in eig], [e[1] for e in eig]))
                for i, n in enumerate(nset):
                    ref = R.reshape_block(Yb[i], eig[i][0], eig[i][1], **_rule(base, mode=ls, oblique=i < nob))
                    assert ref["p_out"] == newp[i] == newY[i].shape[1], (trial, i)
                    assert _rel(newY[i] @ newY[i].T, ref["X"]) <= R.X_TOL, (trial, i)
                    if ls == 1:
                        assert np.array_equal(newU[i], ref["U"]), (trial, i)


def test_planted_decisions_are_unambiguous_and_the_tolerance_holds():
    """On the planted cases the extended-precision rule alone takes the same decisions as the float64 restatement, every decision is
    a factor 10 from its threshold, and the restatement's X stays within X_DEVIATION of the extended-precision X (the figure
    X_TOL = 10 X_DEVIATION rests on)."""
    worst = 0.0
    for case in _planted_cases():
        for base in RULES:
            for mode in (0, 1):
                for oblique in (False, True):
                    rule = _rule(base, mode=mode, oblique=oblique)
                    a = R.reshape_block(case.Y, case.w, case.V, **rule)
                    b = R.reshape_block(case.Y, case.w, case.V, extended=True, **rule)
                    assert (a["p_out"], a["r"], a["nne"]) == (b["p_out"], b["r"], b["nne"]), (case.n, case.p, rule)
                    if b["e"] is not None and b["e"][0] > 0:
                        assert R.decision_margin(np.asarray(b["e"], dtype=np.float64), base["theta"]) >= 10.0, (case.n, case.p)
                    assert np.array_equal(a["U"], b["U"])
                    worst = max(worst, _rel(a["X"], b["X"]))
    print(f"\nlargest |X - X_ext| / |X_ext|: {worst:.2e} (X_DEVIATION {R.X_DEVIATION:.1e})")
    assert worst <= R.X_DEVIATION


def test_library_exports_block_reshape():
    from manisdp_matlab_amd import _lib
    assert "msdp_block_reshape" in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "msdp_block_reshape")
    restype, argtypes = _lib.SIGNATURES["msdp_block_reshape"]
    assert restype is ctypes.c_int and len(argtypes) == 18


@pytest.mark.parametrize("solver", ["ManiSDP_multiblock", "ManiDSDP_multiblock"])
def test_bad_block_reshape_option_is_refused_before_any_handle(solver, monkeypatch):
    import scipy.sparse as sp
    from manisdp_matlab_amd import _lib, solvers
    made = []
    for name in ("multiblock", "dual_multiblock"):
        monkeypatch.setattr(_lib.Handle, name, classmethod(lambda cls, *a, **k: made.append(1)))
    K = {"s": [2, 2], "nob": 1, "f": 0}
    if solver == "ManiSDP_multiblock":
        args = (sp.csc_matrix(np.ones((8, 1))), np.ones(1), np.ones(8), K)
    else:
        args = (sp.csr_matrix(np.ones((1, 8))), np.ones(1), np.ones(8), K)
    with pytest.raises(ValueError, match="block_reshape"):
        getattr(solvers, solver)(*args, {"block_reshape": "gpu"}, verbose=False)
    assert not made
