"""Host-only checks of the rounding feature (msdp_round_hyperplane, options["round"]): the NumPy restatement in
tests/round_ref.py against brute force on tiny instances, the packing, the precondition under which the GPU tests may compare
sign bits exactly, the option's validation, and the header."""
import itertools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import round_ref
from manisdp_matlab_amd import _lib, solvers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny_cost(n, seed, sparse):
    rng = np.random.default_rng(seed)
    A = rng.integers(-4, 5, size=(n, n)) / 4.0                 # multiples of 1/4: every sum below is exact
    if sparse:
        A = A * (rng.random((n, n)) < 0.4)
    A = np.triu(A) + np.triu(A, 1).T                           # symmetric, the diagonal kept
    return sp.csr_matrix(A) if sparse else A


@pytest.mark.parametrize("n,sparse", [(1, False), (2, True), (5, True), (9, False), (12, True), (12, False)])
def test_reference_against_brute_force(n, sparse):
    C = _tiny_cost(n, 7 + n, sparse)
    Cd = C.toarray() if sparse else C
    rng = np.random.default_rng(n)
    X0 = rng.choice([-1.0, 1.0], size=(128, n))
    v0 = round_ref.values(C, X0)
    for t in range(128):
        assert v0[t] == sum(Cd[i, j] * X0[t, i] * X0[t, j] for i in range(n) for j in range(n))
    X, info = round_ref.one_opt(C, X0, 100)
    assert np.all(info[1] == 0) and np.all(info[0] >= 1)       # every word ended on a sweep without a flip
    v = round_ref.values(C, X)
    assert np.all(v <= v0)                                     # a flip lowers x'Cx by 4 x_i s_i > 0
    S = X @ (Cd - np.diag(np.diag(Cd)))                        # s_i of every trial
    assert np.all(X * S <= 0)                                  # 1-opt: no single flip improves
    allx = np.array(list(itertools.product([-1.0, 1.0], repeat=n)))
    assert v.min() >= round_ref.values(C, allx).min()
    # one sweep at a time gives the same trajectory as the sweeps in one call
    X1, i1 = round_ref.one_opt(C, X0, 1)
    X2, i2 = round_ref.one_opt(C, X0, 2)
    X12, _ = round_ref.one_opt(C, X1, 1)
    assert np.array_equal(X12, X2)                             # (a word that had stopped after one sweep has nothing left to flip)
    assert np.all(i2[0] == np.where(i1[1] > 0, 2, 1))


def test_a_tie_does_not_flip_and_zero_rounds_up():
    C = sp.csr_matrix(np.array([[0.0, 0.25, -0.25], [0.25, 0.0, 0.0], [-0.25, 0.0, 0.0]]))
    X0 = np.tile(np.array([[1.0, 1.0, 1.0]]), (64, 1))         # s_0 = 0: a tie; s_1 = s_2 = +-1/4
    X, info = round_ref.one_opt(C, X0, 5)
    assert np.array_equal(X[0], [1.0, -1.0, 1.0]) and info[0, 0] == 2 and info[1, 0] == 0
    Xs, _ = round_ref.signs(np.array([[0.0], [-0.0], [1.0]]), np.ones((64, 1)))
    assert np.array_equal(Xs[0], [1.0, 1.0, 1.0])


def test_packing_round_trip():
    rng = np.random.default_rng(5)
    X = rng.choice([-1.0, 1.0], size=(192, 67))
    M = round_ref.pack(X)
    assert M.shape == (3, 67) and M.dtype == np.uint64
    assert np.array_equal(round_ref.unpack(M), X)
    for t, i in [(0, 0), (63, 66), (64, 1), (191, 66), (100, 33)]:
        assert bool((int(M[t // 64, i]) >> (t % 64)) & 1) == (X[t, i] < 0)
    X[:] = 1.0
    X[63, 2] = -1.0
    assert int(round_ref.pack(X)[0, 2]) == 1 << 63 and not round_ref.pack(X)[1:].any()


def test_no_dot_of_the_gpu_table_is_near_zero():
    """The GPU tests compare sign bits exactly: every |<Y_i, r_t>| of their table must exceed 1e-10, far above the rounding of
    a p-term dot with |Y_i| = 1 (below 1e-13), so the order of the device's sum cannot change a sign."""
    table = round_ref.table()
    assert len(table) == 4 * 12 + 2 * 6
    smallest = np.inf
    for name, n, p, T in table:
        _, D = round_ref.signs(round_ref.table_point(n, p), round_ref.table_directions(T, p))
        assert D.shape == (T, n)
        smallest = min(smallest, float(np.abs(D).min()))
    print("smallest |dot| over the table: %.3e" % smallest)
    assert smallest > 1e-10


@pytest.mark.parametrize("bad", [{"trials": 65}, {"trials": 0}, {"trials": 8192}, {"trials": 64, "sweeps": -1}, {"trials": "64"},
                                 {"trials": 64, "seed": 1.5}, {"trails": 64}, 256, {"trials": True}])
def test_bad_round_option_is_refused_before_any_handle(bad, monkeypatch):
    def no_handle(*a, **k):
        raise AssertionError("a handle was built")
    for ctor in ("onlyunitdiag", "affine", "dense_synthetic"):
        monkeypatch.setattr(_lib.Handle, ctor, staticmethod(no_handle))
    C = sp.csr_matrix(np.ones((6, 6)) - np.eye(6))
    with pytest.raises(ValueError, match="round"):
        solvers.ManiSDP_onlyunitdiag(C, {"round": bad}, verbose=False)


def test_a_good_round_option_reaches_the_handle(monkeypatch):
    class Built(Exception):
        pass

    def built(*a, **k):
        raise Built()
    monkeypatch.setattr(_lib.Handle, "onlyunitdiag", staticmethod(built))
    C = sp.csr_matrix(np.ones((6, 6)) - np.eye(6))
    with pytest.raises(Built):
        solvers.ManiSDP_onlyunitdiag(C, {"round": {"trials": 128, "sweeps": 0, "seed": 3}}, verbose=False)
    with pytest.raises(ValueError, match="round"):
        solvers.ManiSDP_onlyunitdiag(C, {"round": {"trials": 64}, "comm": (2, 0, b"")}, verbose=False)


def test_round_is_not_a_reference_default():
    assert solvers.DEFAULTS
    for kind, defaults in solvers.DEFAULTS.items():
        assert "round" not in defaults, kind
    assert callable(solvers.round_unitdiag)


def test_header_declares_the_entry_point():
    txt = open(os.path.join(ROOT, "include", "manisdp_hip.h")).read()
    assert re.search(r"^#define\s+MSDP_ROUND_MAX_TRIALS\s+4096\b", txt, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+msdp_round_hyperplane\s*\(\s*msdp_handle\s+h\s*,\s*int32_t\s+trials\s*,\s*const\s+double\s*\*\s*R\s*,", code)
    assert "msdp_round_hyperplane" in _lib.SIGNATURES and _lib.ROUND_MAX_TRIALS == 4096
