"""Host-only checks of the sparse-plus-low-rank cost kind (problems.SparsePlusLowRank, problems.modularity,
msdp_create_onlyunitdiag_csc_lowrank): the NumPy restatement of tests/lowrank_ref.py against the oracle on the dense equivalent
and against brute force, the instances of the GPU tests and the precondition of their exact comparisons, the problem classes,
the solver's argument checks, and the header."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import lowrank_ref
import round_ref
from manisdp_matlab_amd import _lib, problems, solvers
from oracle import manisdp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _relerr(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("storage", lowrank_ref.STORAGES)
@pytest.mark.parametrize("q", lowrank_ref.Q_GRID)
def test_instances_are_what_the_gpu_tests_assume(storage, q):
    for n in lowrank_ref.N_GRID:
        C, Cd = lowrank_ref.instance(storage, n, q)
        assert C.shape == (n, n) and C.q == q and Cd.shape == (n, n)
        width = np.diff(C.Cs.indptr)
        if storage == "grid":
            assert np.all(width == 4)                              # fixed-width storage on the device (rows of <= 8 entries)
        else:
            assert width.max() > 64 and np.count_nonzero(C.Cs.diagonal()) > 0      # CSR, second batch of 64, a stored diagonal
        for arr in (C.Cs.data, C.V, C.s):
            assert np.array_equal(arr * 4, np.round(arr * 4)) and np.abs(arr).max() <= 2
        assert np.array_equal(Cd, Cd.T) and np.array_equal(Cd * 64, np.round(Cd * 64))
        assert np.array_equal(Cd, C.Cs.toarray() + sum(C.s[k] * np.outer(C.V[:, k], C.V[:, k]) for k in range(q)))
        if q > 1:
            assert C.s.min() < 0 < C.s.max()                       # mixed signs


@pytest.mark.parametrize("n,p,q,storage", [(203, 5, 1, "grid"), (203, 17, 3, "hub"), (1031, 2, 8, "grid"), (203, 33, 8, "hub")])
def test_split_form_against_the_oracle_on_the_dense_matrix(n, p, q, storage):
    C, Cd = lowrank_ref.instance(storage, n, q)
    Y, U = lowrank_ref.table_point(n, p), lowrank_ref.table_direction(n, p)
    prob = manisdp_ref._OnlyUnitDiagProblem(Cd, n, p)
    f_ref = prob.cost(Y)
    args = (C.Cs, C.V, C.s)
    assert abs(lowrank_ref.cost(*args, Y) - f_ref) <= 1e-13 * max(1.0, abs(f_ref))
    assert _relerr(lowrank_ref.rgrad(*args, Y), prob.grad(Y)) < 1e-13
    assert _relerr(lowrank_ref.hessvec(*args, Y, U), manisdp_ref.hessvec_onlyunitdiag(Cd, Y, U)) < 1e-13
    assert _relerr(lowrank_ref.hessvec(*args, Y, U), prob.hess(Y, U)) < 1e-13
    assert _relerr(lowrank_ref.get_z(*args, Y), np.sum((Cd @ Y) * Y, axis=1)) < 1e-13
    assert _relerr(C.matvec(U), Cd @ U) < 1e-13 and _relerr(C.matvec(U[:, 0]), Cd @ U[:, 0]) < 1e-13


@pytest.mark.parametrize("n,q,storage", [(203, 1, "grid"), (203, 3, "hub"), (203, 8, "grid"), (203, 8, "hub")])
def test_rounding_restatement_against_the_dense_matrix(n, q, storage):
    """Every entry is a multiple of 1/4 (of 1/64 in the dense equivalent): all sums are exact, so the restatement with the
    low-rank term carried as t_k must give, bit for bit, what round_ref gives on the dense matrix."""
    C, Cd = lowrank_ref.instance(storage, n, q)
    X0 = np.random.default_rng(n + q).choice([-1.0, 1.0], size=(128, n))
    v0 = lowrank_ref.values(C.Cs, C.V, C.s, X0)
    assert np.array_equal(v0, np.einsum("ti,ij,tj->t", X0, Cd, X0))                  # plain x' C x
    assert np.array_equal(v0, round_ref.values(Cd, X0))
    for sweeps in (1, 2, 50):
        X, info = lowrank_ref.one_opt(C.Cs, C.V, C.s, X0, sweeps)
        Xd, infod = round_ref.one_opt(Cd, X0, sweeps)                                # brute force: 1-opt on the dense rows
        assert np.array_equal(X, Xd) and np.array_equal(info, infod), sweeps
    assert np.all(info[1] == 0)
    S = X @ (Cd - np.diag(np.diag(Cd)))
    assert np.all(X * S <= 0)                                                        # no single flip improves
    assert np.all(lowrank_ref.values(C.Cs, C.V, C.s, X) <= v0)
    Y, R = lowrank_ref.table_point(n, 3), round_ref.table_directions(64, 3)
    a, b = lowrank_ref.round_hyperplane(C, Y, R, 50), round_ref.round_hyperplane(Cd, Y, R, 50)
    for k in ("values0", "values", "info", "x", "masks"):
        assert np.array_equal(a[k], b[k]), k
    assert a["best"] == b["best"]


def test_no_dot_of_the_gpu_table_is_near_zero():
    """The GPU tests compare sign bits exactly: every |<Y_i, r_t>| of their table must exceed 1e-10 (tests/test_round_ref_host.py
    has the argument)."""
    smallest = np.inf
    for n in lowrank_ref.N_GRID:
        C, _ = lowrank_ref.instance("grid", n, 1)                   # the points belong to the instances' orders
        for p in lowrank_ref.ROUND_P:
            for T in lowrank_ref.ROUND_T:
                _, D = round_ref.signs(lowrank_ref.table_point(C.shape[0], p), round_ref.table_directions(T, p))
                assert D.shape == (T, C.shape[0])
                smallest = min(smallest, float(np.abs(D).min()))
    print("smallest |dot| over the table: %.3e" % smallest)
    assert smallest > 1e-10


def test_sparse_plus_low_rank_class():
    Cs = lowrank_ref.grid_cs(203)
    V, s = lowrank_ref.lowrank_term(203, 3)
    C = problems.SparsePlusLowRank(Cs, V, s)
    assert C.shape == (203, 203) and C.q == 3
    D = C.toarray()
    assert np.array_equal(D, Cs.toarray() + (V * s) @ V.T)
    back = problems.SparsePlusLowRank(sp.csr_matrix(D - (V * s) @ V.T), V, s)       # round trip through the dense form
    assert np.array_equal(back.toarray(), D) and abs(back.Cs - Cs).max() == 0
    one = problems.SparsePlusLowRank(Cs, V[:, 0], s[0])                              # a vector is one column
    assert one.q == 1 and np.array_equal(one.toarray(), Cs.toarray() + s[0] * np.outer(V[:, 0], V[:, 0]))
    x = np.arange(203.0)
    assert np.allclose(C.matvec(x), D @ x, rtol=1e-13, atol=0) and C.matvec(np.ones((203, 2))).shape == (203, 2)
    for bad in ((Cs, V[:100], s), (Cs, V, s[:2]), (Cs, np.zeros((203, 0)), np.zeros(0)), (sp.csr_matrix((3, 4)), V, s)):
        with pytest.raises(ValueError):
            problems.SparsePlusLowRank(*bad)


def test_modularity_agrees_with_its_definition():
    rng = np.random.default_rng(12)
    A = np.triu((rng.random((12, 12)) < 0.4).astype(float), 1)
    A = A + A.T
    d = A.sum(axis=1)
    two_m = d.sum()
    for gamma in (1.0, 0.5):
        C = problems.modularity(sp.csr_matrix(A), gamma=gamma)
        assert isinstance(C, problems.SparsePlusLowRank) and C.q == 1 and C.shape == (12, 12)
        B = A - gamma * np.outer(d, d) / two_m
        assert np.allclose(C.toarray(), -B, rtol=0, atol=1e-15)
        x = rng.choice([-1.0, 1.0], size=12)
        Q = sum(B[i, j] for i in range(12) for j in range(12) if x[i] == x[j]) / two_m   # Newman's modularity of the labelling
        # with delta(c_i, c_j) = (1 + x_i x_j) / 2:  Q = (sum B + x' B x) / (4m), and sum B = 0 when gamma = 1
        mv = lowrank_ref.modularity_value(sp.csr_matrix(A), x, gamma)
        assert abs(mv - (Q - B.sum() / (2 * two_m))) < 1e-14 and (gamma != 1.0 or abs(mv - Q) < 1e-14)
        assert abs(-(x @ C.toarray() @ x) / (2 * two_m) - mv) < 1e-13
    with pytest.raises(ValueError):
        problems.modularity(sp.csr_matrix((5, 5)))


def _no_handle(monkeypatch):
    def no_handle(*a, **k):
        raise AssertionError("a handle was built")
    for ctor in ("onlyunitdiag", "onlyunitdiag_lowrank", "affine", "dense_synthetic"):
        monkeypatch.setattr(_lib.Handle, ctor, staticmethod(no_handle))


def test_solver_refuses_a_communicator_and_a_wide_term_before_any_handle(monkeypatch):
    _no_handle(monkeypatch)
    Cs = sp.csr_matrix(np.ones((6, 6)) - np.eye(6))
    C = problems.SparsePlusLowRank(Cs, np.ones((6, 2)), [1.0, -1.0])
    with pytest.raises(ValueError, match="comm"):
        solvers.ManiSDP_onlyunitdiag(C, {"comm": ("local", 2, 0, 7)}, verbose=False)
    with pytest.raises(ValueError, match="comm"):
        solvers.ManiSDP_onlyunitdiag(C, {"comm": (2, 0, b"")}, verbose=False)
    wide = problems.SparsePlusLowRank(Cs, np.ones((6, _lib.LOWRANK_MAX + 1)), np.ones(_lib.LOWRANK_MAX + 1))
    with pytest.raises(ValueError, match="q = 9"):
        solvers.ManiSDP_onlyunitdiag(wide, {}, verbose=False)
    with pytest.raises(ValueError, match="round"):
        solvers.ManiSDP_onlyunitdiag(C, {"round": {"trials": 65}}, verbose=False)


def test_a_good_problem_reaches_the_low_rank_constructor(monkeypatch):
    class Built(Exception):
        pass

    def built(Cs, V, s, pcap=32):
        assert sp.issparse(Cs) and V.shape == (6, 2) and s.shape == (2,)
        raise Built()
    monkeypatch.setattr(_lib.Handle, "onlyunitdiag_lowrank", staticmethod(built))
    C = problems.SparsePlusLowRank(sp.csr_matrix(np.ones((6, 6)) - np.eye(6)), np.ones((6, 2)), [1.0, -1.0])
    with pytest.raises(Built):
        solvers.ManiSDP_onlyunitdiag(C, {"round": {"trials": 64}}, verbose=False)
    with pytest.raises(Built):
        solvers.round_unitdiag(C, np.ones((6, 1)), trials=64, sweeps=0)


def test_header_and_binding_declare_the_entry_point():
    txt = open(os.path.join(ROOT, "include", "manisdp_hip.h")).read()
    assert re.search(r"^#define\s+MSDP_LOWRANK_MAX\s+8\b", txt, flags=re.M) and _lib.LOWRANK_MAX == 8
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+msdp_create_onlyunitdiag_csc_lowrank\s*\(\s*int64_t\s+n\s*,", code)
    assert "ManiSDP_onlyunitdiag.m:6" in txt
    assert "msdp_create_onlyunitdiag_csc_lowrank" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["msdp_create_onlyunitdiag_csc_lowrank"][1]) == 9
