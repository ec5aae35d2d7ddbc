"""A recording, scripted stand-in for _lib.Handle and the scenarios that drive the four manifold-only entry points of solvers.py
(ManiSDP_onlyunitdiag with a real and with a complex Hermitian C, ManiSDP_onlyunitblockdiag, ManiSDP_posegraph) through every
branch of their outer loop without the library: shared by tests/test_unitdiag_loops_host.py, which compares record(scenario)
with tests/golden/unitdiag_loop_traces.json entry by entry, exactly.

The fixture was made by running this file as a script (``python tests/unitdiag_loop_fake.py OUT.json``) in a checkout of the last
commit that still had the four loops as separate copies (``git worktree add DIR 0b7c1ee``, this file copied next to that tree's
tests), so it pins what those copies did.  The entries named in INTENDED_CHANGES were recorded again after the loops became one
(``python tests/unitdiag_loop_fake.py tests/golden/unitdiag_loop_traces.json NAME ...``): they are the behaviour that commit
changed on purpose (a handle whose set-up raises is closed; a solve of zero iterations
returns).  It holds our own program's output: call names, digests and printed lines.

The handle answers from a script, not from arithmetic: ``z`` / ``gap`` (the shift of the multipliers and obj - dual per
evaluation), ``rank`` (the numerical rank trustregions() leaves the point with), ``esc`` / ``ver`` (lambda_min of the regular and of
the cold escape calls), ``conv`` (escape_info), ``ndeg`` (degenerate-block counts), ``raises`` (the n-th call of a method raises).
A list that runs out repeats its last entry.  Noise comes from a generator seeded by (method, call count), so an answer does not
depend on what was called in between."""
import hashlib
import json
import os
import re
import sys
import zlib

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "unitdiag_loop_traces.json")
LAM_MAX = 3.0                       # lambda_max of every scripted escape call: dinf = -lambda_min / 4
# scenarios whose entry was recorded after the four loops became one (see the module docstring)
INTENDED_CHANGES = ("real_set_option_raises", "real_comm_join_raises", "herm_set_option_raises", "block_set_option_raises",
                    "real_zero_iterations")


def digest(v):
    """dtype, shape and a hash of the bytes for arrays (sparse ones by their dense form), the plain value for scalars."""
    if sp.issparse(v):
        return "sparse:" + digest(v.toarray())
    if isinstance(v, np.ndarray):
        return f"{v.dtype}{list(v.shape)}:{hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest()[:12]}"
    if isinstance(v, (np.integer, np.bool_)):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    if isinstance(v, bytes):
        return "bytes:" + v.hex()
    if isinstance(v, dict):
        return {str(k): digest(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [digest(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if hasattr(v, "_fields_"):                             # the RtrOpts structure
        return f"{type(v).__name__}:{hashlib.sha1(bytes(v)).hexdigest()[:12]}"
    return type(v).__name__


def _call(name, args, kw):
    """One call as a short string: name(digest, ..., key=digest)."""
    show = lambda v: v if isinstance(v, str) else json.dumps(v)
    return name + "(" + ",".join([show(digest(a)) for a in args] + [f"{k}={show(digest(kw[k]))}" for k in sorted(kw)]) + ")"


def _elide(rows, most, keep):
    """A long list as its length, the hash of all of it and its two ends: the 60-iteration scenarios stay small in the fixture."""
    if len(rows) <= most:
        return rows
    return {"n": len(rows), "sha1": hashlib.sha1(json.dumps(rows).encode()).hexdigest(), "head": rows[:keep], "tail": rows[-keep:]}


def _pick(seq, i):
    return seq[min(i, len(seq) - 1)]


class _Stats:
    def __init__(self, i):
        self.seconds, self.hessvecs, self.cost_evals, self.rejected, self.gradnorm = 0.25, 10 + i, 3 + i, i % 2, 10.0 ** -(i + 1)


class FakeHandle:
    def __init__(self, calls, script, n, dtype=np.float64, blk=0, d=0, efree=0):
        self.calls, self.script, self.n, self.dtype, self.blk, self.d, self.efree = calls, script, n, dtype, blk, d, efree
        self.P = None
        self.count = {}
        self.closed = False

    # ---- the machinery
    def _rec(self, name, *args, **kw):
        from manisdp_matlab_amd import _lib
        self.calls.append(_call(name, args, kw))
        i = self.count[name] = self.count.get(name, 0) + 1
        what = self.script.get("raises", {}).get(name)
        if what is not None and what[0] == i:
            if what[1] == "capacity":
                raise _lib.MsdpError(f"{name}: width exceeds the allocated capacity of the handle")
            raise _lib.MsdpError(f"{name}: {what[1]}")
        return i - 1

    def _rng(self, name, i):
        return np.random.default_rng([zlib.crc32(name.encode()), i])

    def _noise(self, name, i, shape):
        g = self._rng(name, i)
        x = g.standard_normal(shape)
        if self.dtype == np.complex128:
            x = x + 1j * g.standard_normal(shape)
        return x

    # ---- set-up and transfers
    def set_option(self, name, value):
        self._rec("set_option", name, value)
        if self.script.get("set_option_raises") == name:
            from manisdp_matlab_amd import _lib
            raise _lib.MsdpError(f"unknown option {name}")

    def comm_init(self, nranks, rank, uid):
        self._rec("comm_init", nranks, rank, uid)
        if self.script.get("comm_raises"):
            from manisdp_matlab_amd import _lib
            raise _lib.MsdpError("comm_init: no such peer")

    def comm_init_local(self, nranks, rank, group):
        self._rec("comm_init_local", nranks, rank, group)

    def set_point(self, Y):
        self._rec("set_point", Y)
        self.P = np.array(Y, dtype=self.dtype)

    def get_point(self):
        self._rec("get_point")
        return self.P.copy()

    def get_point_all(self):
        self._rec("get_point_all")
        return self.P.copy()

    def close(self):
        self._rec("close")
        self.closed = True

    # ---- per iteration
    def rtr(self, opts):
        i = self._rec("rtr", opts)
        self.P = self.P + 1e-3 * self._noise("rtr", i, self.P.shape)
        r = _pick(self.script.get("rank", [None]), i)
        if r is not None:                                  # numerical rank r: the trailing columns as good as gone
            self.P[:, r:] *= 1e-9
        return _Stats(i)

    def _z(self, name):
        i = self._rec(name)
        return i, _pick(self.script.get("z", [1.0]), self.count.get("rtr", 1) - 1)

    def get_z(self):
        i, shift = self._z("get_z")
        z = shift + 0.1 * self._rng("get_z", i).standard_normal(self.n)
        if self.efree:
            z.reshape(-1, self.blk)[:, self.d:] = 0.0
        self.dual = float(np.sum(z))
        return z

    def get_z_all(self):
        i, shift = self._z("get_z_all")
        return shift + 0.1 * self._rng("get_z_all", i).standard_normal(self.n)

    def get_blockmult(self):
        i, shift = self._z("get_blockmult")
        A = 0.1 * self._rng("get_blockmult", i).standard_normal((self.n // self.blk, self.d, self.d))
        return shift * np.eye(self.d)[None] + 0.5 * (A + A.transpose(0, 2, 1))

    def cost(self):
        self._rec("cost")                                  # obj = 2 cost = dual + the scripted difference
        return 0.5 * (self.dual + _pick(self.script.get("gap", [0.0]), self.count.get("rtr", 1) - 1))

    def linesearch_cost(self, U, alpha):
        i = self._rec("linesearch_cost", U, alpha)
        return _pick(self.script.get("ls", [0.0, 0.0, -1.0]), i)

    def linesearch_accept(self):
        self._rec("linesearch_accept")

    # ---- the escape
    def escape_eigs(self, k, tol=1e-10, maxit=500):
        name = "ver" if k == 1 else "esc"
        i = self._rec("escape_eigs", k, tol=tol, maxit=maxit)
        j = self.count[name] = self.count.get(name, 0) + 1
        lam0 = _pick(self.script.get(name, [1e-12] if k == 1 else [-1.0]), j - 1)
        lam = np.asarray(lam0, dtype=np.float64) if isinstance(lam0, list) else lam0 + 0.25 * abs(lam0) * np.arange(k)
        return lam, self._noise("escape_eigs", i, (self.n, k)), LAM_MAX, 100 + i

    def escape_info(self):
        i = self._rec("escape_info")
        return 1, bool(_pick(self.script.get("conv", [True]), i)), 1e-10

    def escape_method(self):
        self._rec("escape_method")
        return self.script.get("method", 1)

    def ritz_stages(self):
        self._rec("ritz_stages")
        return (2, 1, 0)

    # ---- the factor on the device
    def _gram(self, name):
        self._rec(name)
        return self.P.conj().T @ self.P

    def _rotate(self, name, Q):
        i = self._rec(name, Q)
        nd = _pick(self.script.get("ndeg", {}).get(name, [0]), i)
        if nd == 0:
            self.P = self.P @ Q
        return nd

    def _append(self, name, V, alpha, **kw):
        i = self._rec(name, V, alpha, **kw)
        nd = _pick(self.script.get("ndeg", {}).get(name, [0]), i)
        if nd == 0:
            self.P = np.hstack([self.P, alpha * V])
        return nd

    def factor_gram(self):
        return self._gram("factor_gram")

    def hfactor_gram(self):
        return self._gram("hfactor_gram")

    def blockfactor_gram(self):
        return self._gram("blockfactor_gram")

    def factor_rotate(self, Q):
        self._rotate("factor_rotate", Q)

    def hfactor_rotate(self, Q):
        self._rotate("hfactor_rotate", Q)

    def blockfactor_rotate(self, Q):
        return self._rotate("blockfactor_rotate", Q)

    def factor_append(self, V, alpha, normalize=True):
        self._append("factor_append", V, alpha, normalize=normalize)

    def hfactor_append(self, V, alpha):
        self._append("hfactor_append", V, alpha)

    def blockfactor_append(self, V, alpha):
        return self._append("blockfactor_append", V, alpha)

    # ---- rounding
    def round_hyperplane(self, R, sweeps=0, masks=False):
        self._rec("round_hyperplane", R, sweeps=sweeps)
        g = self._rng("round_hyperplane", 0)
        return {"x": np.sign(g.standard_normal(self.n)).astype(np.int8), "values": g.standard_normal(R.shape[0]), "best": 3,
                "info": {"sweeps": np.arange(R.shape[0] // 64)}}

    def round_phases(self, R, M=0, sweeps=0, phases=False):
        self._rec("round_phases", R, M=M, sweeps=sweeps)
        g = self._rng("round_phases", 0)
        return {"z": np.exp(1j * g.standard_normal(self.n)), "values": g.standard_normal(R.shape[0]), "best": 5,
                "info": {"sweeps": np.arange(R.shape[0] // 64)}, "k": np.arange(self.n) % max(M, 1)}

    def round_blocks(self, W=None):
        i = self._rec("round_blocks")
        g = self._rng("round_blocks", 0)
        nb = self.n // self.blk
        return (g.standard_normal((nb, self.d, self.d)), g.standard_normal((nb, self.d)) if self.efree else None, None,
                _pick(self.script.get("ndeg", {}).get("round_blocks", [0]), i))


# ------------------------------------------------------------------------------------------------------------ the problems
def _sym(n, seed, complex_=False):
    g = np.random.default_rng(seed)
    A = np.triu(g.standard_normal((n, n)) * (g.random((n, n)) < 0.5), 1)
    if complex_:
        A = A + 1j * np.triu(g.standard_normal((n, n)), 1) * (A != 0)
    return sp.csr_matrix(A + A.conj().T)


def _psd(n, seed):
    M = np.random.default_rng(seed).standard_normal((n, n))
    return sp.csr_matrix(M @ M.T)


def _wide_start(N, blk, d, p):
    """A feasible start of width p: the first d columns carry the identity blocks."""
    Y = np.zeros((N // blk, blk, p))
    Y[:, :d, :d] = np.eye(d)
    return Y.reshape(N, p)


def _problem(sc):
    from manisdp_matlab_amd import problems
    kind, d, n = sc["kind"], sc.get("d", 0), sc.get("n", 8)
    what = sc.get("C", "sparse")
    if kind == "herm":
        return _sym(n, 2, complex_=True)
    if kind == "block":
        return _sym(sc.get("N", 3 * d), 3)
    if kind == "pose":
        return _psd(sc.get("N", 3 * (d + 1)), 4)
    if what == "dense":
        return _sym(n, 1).toarray()
    if what == "lowrank":
        g = np.random.default_rng(5)
        return problems.SparsePlusLowRank(_sym(n, 1), g.standard_normal((n, 2)), np.array([0.5, -0.25]))
    if what == "lowrank_wide":
        return problems.SparsePlusLowRank(_sym(n, 1), np.ones((n, 9)), np.ones(9))
    if what == "synthetic":
        return problems.SyntheticDenseC(n, seed=7)
    if what == "complex":
        return _sym(n, 2, complex_=True)
    return _sym(n, 1)


# ----------------------------------------------------------------------------------------------------------- the scenarios
def _sc(name, kind, options=None, **kw):
    script = {k: kw.pop(k) for k in list(kw) if k in ("z", "gap", "rank", "esc", "ver", "conv", "ndeg", "raises", "method", "ls",
                                                     "set_option_raises", "comm_raises")}
    return dict(name=name, kind=kind, options=dict(options or {}), script=script, **kw)


DEV = dict(eig="device")
ROUND = dict(round=dict(trials=64, sweeps=3, seed=1))


def _slow():
    """Sixty regular escape answers: dinf at it = 60 above that at it = 40."""
    return [-1.0 / (1 + i) for i in range(40)] + [-0.01] * 19 + [-0.5]


def _real():
    return [
        _sc("real_host", "real", dict(eig="host"), z=[1.0, 1.0, -50.0], rank=[None, 1, None]),
        _sc("real_host_dense_C", "real", dict(eig="host"), C="dense", z=[1.0, -50.0]),
        _sc("real_host_unconverged", "real", dict(eig="host", AL_maxiter=2), z=[1.0]),
        _sc("real_host_sparse", "real", dict(eig="host_sparse", delta=3), n=12, z=[1.0, 1.0, -50.0]),
        _sc("real_device", "real", DEV, rank=[None, 1, None], esc=[-1.0, -1.0, 1e-12]),
        _sc("real_device_inf_pairs", "real", dict(DEV, delta=3), esc=[[-1.0, -0.5, float("inf")], 1e-12]),
        _sc("real_capacity", "real", DEV, rank=[1, None], esc=[-1.0, -1.0, 1e-12], raises={"factor_append": (1, "capacity")}),
        _sc("real_capacity_second", "real", DEV, esc=[-1.0, -1.0, -1.0, 1e-12], raises={"factor_append": (2, "capacity")}),
        _sc("real_append_error", "real", DEV, raises={"factor_append": (2, "device lost")}),
        _sc("real_rotate_error", "real", DEV, rank=[1, None], raises={"factor_rotate": (1, "device lost")}),
        _sc("real_host_factor_device_eig", "real", dict(DEV, device_factor=False), rank=[None, 1, None],
            esc=[-1.0, -1.0, 1e-12]),
        _sc("real_line_search", "real", dict(eig="host", line_search=1), z=[1.0, 1.0, -50.0], rank=[None, 1, None]),
        _sc("real_line_search_backtracks", "real", dict(eig="host", line_search=1), z=[1.0, -50.0], ls=[0.0, 1.0, 0.5, -1.0]),
        _sc("real_line_search_device_eig", "real", dict(DEV, line_search=1), esc=[-1.0, 1e-12]),
        _sc("real_comm", "real", dict(comm=(2, 0, b"id"), halo_exchange=True, eig="host"), esc=[-1.0, -1.0, 1e-12], rank=[1, None]),
        _sc("real_comm_local_synthetic", "real", dict(comm=("local", 2, 1, 0)), C="synthetic", esc=[-1.0, 1e-12]),
        _sc("real_comm_capacity", "real", dict(comm=(2, 1, b"id")), esc=[-1.0, 1e-12], raises={"factor_append": (1, "capacity")}),
        _sc("real_comm_dense_refused", "real", dict(comm=(2, 0, b"id")), C="dense"),
        _sc("real_comm_lowrank_refused", "real", dict(comm=(2, 0, b"id")), C="lowrank"),
        _sc("real_lowrank_host", "real", dict(eig="host"), C="lowrank", z=[1.0, -50.0]),
        _sc("real_lowrank_device", "real", DEV, C="lowrank", esc=[-1.0, 1e-12]),
        _sc("real_lowrank_device_no_S", "real", dict(DEV, dense_X_max=4), C="lowrank", esc=[-1.0, 1e-12]),
        _sc("real_lowrank_too_wide", "real", C="lowrank_wide"),
        _sc("real_synthetic_host", "real", None, C="synthetic", z=[1.0, -50.0]),
        _sc("real_synthetic_device", "real", DEV, C="synthetic", esc=[-1.0, 1e-12]),
        _sc("real_eig_retry", "real", DEV, conv=[False, True], esc=[-1.0, -1.0, 1e-12]),
        _sc("real_eig_unconverged", "real", dict(DEV, AL_maxiter=2), conv=[False], esc=[1e-12]),
        _sc("real_verify_unconverged", "real", dict(DEV, AL_maxiter=2), conv=[True, False, False, True], esc=[1e-12]),
        _sc("real_verify_missed", "real", DEV, esc=[1e-12, -1.0, 1e-12], ver=[-1.0, 1e-12]),
        _sc("real_verify_missed_delta2", "real", dict(DEV, delta=2), esc=[[1e-12, 1.0], [1e-12, 1.0]], ver=[-1.0, 1e-12]),
        _sc("real_verify_at_maxiter", "real", dict(DEV, AL_maxiter=2), esc=[-1.0], ver=[-0.5]),
        _sc("real_verify_at_maxiter_host_factor", "real", dict(DEV, AL_maxiter=2, device_factor=False), esc=[-1.0], ver=[-0.5]),
        _sc("real_slow", "real", dict(DEV, AL_maxiter=100), esc=_slow(), ver=[-0.25]),
        _sc("real_slow_host_factor", "real", dict(DEV, AL_maxiter=100, device_factor=False, delta=2), esc=_slow(), ver=[-0.25]),
        _sc("real_round", "real", dict(DEV, **ROUND), esc=[-1.0, 1e-12]),
        _sc("real_round_host", "real", dict(eig="host", **ROUND), z=[1.0, -50.0]),
        _sc("real_round_comm_refused", "real", dict(comm=(2, 0, b"id"), **ROUND)),
        _sc("real_round_bad", "real", dict(round=dict(trials=65))),
        _sc("real_passthrough", "real", dict(DEV, escape_method=2, escape_rr="device", device_options={"fused": 0, "wide": 1}),
            method=0, esc=[-1.0, 1e-12]),
        _sc("real_Y0", "real", dict(eig="host", Y0=np.eye(8)[:, :3] + 0.5), z=[1.0, -50.0]),
        _sc("real_bad_escape_rr", "real", dict(escape_rr="gpu")),
        _sc("real_round_phases_refused", "real", dict(round_phases=dict(M=0))),
        _sc("real_hermitian_factor_refused", "real", dict(hermitian_factor="device")),
        _sc("real_hermitian_factor_bad", "real", dict(hermitian_factor="gpu")),
        _sc("real_set_option_raises", "real", dict(DEV, device_options={"nonsense": 1}), set_option_raises="nonsense"),
        _sc("real_comm_join_raises", "real", dict(comm=(2, 0, b"id")), comm_raises=True),
        _sc("real_zero_iterations", "real", dict(AL_maxiter=0)),
    ]


def _herm():
    RP = dict(trials=64, sweeps=2, seed=3)
    return [
        _sc("herm_host", "herm", dict(eig="host"), z=[1.0, 1.0, -50.0], rank=[None, 1, None]),
        _sc("herm_host_factor_device_eig", "herm", DEV, rank=[None, 1, None], esc=[-1.0, -1.0, 1e-12]),
        _sc("herm_device", "herm", dict(DEV, hermitian_factor="device"), rank=[None, 1, None], esc=[-1.0, -1.0, 1e-12]),
        _sc("herm_device_host_eig", "herm", dict(eig="host", hermitian_factor="device"), z=[1.0, 1.0, -50.0], rank=[1, None]),
        _sc("herm_capacity", "herm", dict(DEV, hermitian_factor="device"), rank=[1, None], esc=[-1.0, -1.0, 1e-12],
            raises={"hfactor_append": (1, "capacity")}),
        _sc("herm_append_error", "herm", dict(DEV, hermitian_factor="device"), raises={"hfactor_append": (1, "device lost")}),
        _sc("herm_verify_missed", "herm", dict(DEV, hermitian_factor="device"), esc=[1e-12, -1.0, 1e-12], ver=[-1.0, 1e-12]),
        _sc("herm_eig_unconverged", "herm", dict(DEV, AL_maxiter=2), conv=[False], esc=[1e-12]),
        _sc("herm_device_maxiter", "herm", dict(DEV, hermitian_factor="device", AL_maxiter=2), esc=[-1.0], ver=[-0.5]),
        _sc("herm_round_M0", "herm", dict(DEV, round_phases=dict(RP, M=0)), esc=[-1.0, 1e-12]),
        _sc("herm_round_M4", "herm", dict(DEV, hermitian_factor="device", round_phases=dict(RP, M=4)), esc=[-1.0, 1e-12]),
        _sc("herm_slow_device", "herm", dict(DEV, AL_maxiter=100, hermitian_factor="device"), esc=_slow()),
        _sc("herm_zero_iterations", "herm", dict(AL_maxiter=0)),
        _sc("herm_round_refused", "herm", ROUND),
        _sc("herm_comm_refused", "herm", dict(comm=(2, 0, b"id"))),
        _sc("herm_line_search_refused", "herm", dict(line_search=1)),
        _sc("herm_device_factor_refused", "herm", dict(device_factor=True)),
        _sc("herm_bad_eig", "herm", dict(eig="host_sparse")),
        _sc("herm_bad_hermitian_factor", "herm", dict(hermitian_factor="gpu")),
        _sc("herm_bad_round_phases", "herm", dict(round_phases=dict(M=1))),
        _sc("herm_set_option_raises", "herm", dict(device_options={"nonsense": 1}), set_option_raises="nonsense"),
    ]


def _blocks(kind):
    """The scenarios the two block kinds share; the pose-graph kind converges on z = -50 with gap 0 as the block kind does."""
    k = kind
    BD = dict(DEV, block_factor="device")
    rot, app = "blockfactor_rotate", "blockfactor_append"
    out = []
    for d in (2, 3):
        out += [
            _sc(f"{k}_host_d{d}", k, dict(eig="host"), d=d, z=[1.0, 1.0, 1.0, -50.0], rank=[1, d, None, None]),
            _sc(f"{k}_device_d{d}", k, BD, d=d, rank=[1, d, None, None], esc=[-1.0, -1.0, -1.0, 1e-12]),
            _sc(f"{k}_rotate_degenerate_d{d}", k, BD, d=d, rank=[d, None], esc=[-1.0, -1.0, 1e-12], ndeg={rot: [2, 0]}),
        ]
    d = 2
    out += [
        _sc(f"{k}_host_factor_device_eig", k, DEV, d=d, rank=[None, d, None], esc=[-1.0, -1.0, 1e-12]),
        _sc(f"{k}_device_host_eig", k, dict(eig="host", block_factor="device"), d=d, z=[1.0, 1.0, -50.0], rank=[d, None]),
        _sc(f"{k}_append_degenerate", k, BD, d=d, rank=[d, None], esc=[-1.0, -1.0, 1e-12], ndeg={app: [1, 0]}),
        _sc(f"{k}_append_degenerate_no_cut", k, BD, d=d, esc=[-1.0, -1.0, 1e-12], ndeg={app: [1, 0]}),
        _sc(f"{k}_capacity", k, BD, d=d, rank=[d, None], esc=[-1.0, -1.0, 1e-12], raises={app: (1, "capacity")}),
        _sc(f"{k}_append_error", k, BD, d=d, raises={app: (1, "device lost")}),
        _sc(f"{k}_too_wide_host", k, dict(eig="host", Y0=("wide", 255)), d=d, rank=[1]),
        _sc(f"{k}_too_wide_device", k, dict(BD, Y0=("wide", 255)), d=d, rank=[1]),
        _sc(f"{k}_device_maxiter", k, dict(BD, AL_maxiter=2), d=d, esc=[-1.0], ver=[-0.5]),
        _sc(f"{k}_host_maxiter", k, dict(DEV, AL_maxiter=2), d=d, esc=[-1.0], ver=[-0.5]),
        _sc(f"{k}_verify_missed", k, BD, d=d, esc=[1e-12, -1.0, 1e-12], ver=[-1.0, 1e-12]),
        _sc(f"{k}_eig_retry", k, DEV, d=d, conv=[False, True], esc=[-1.0, -1.0, 1e-12]),
        _sc(f"{k}_eig_unconverged", k, dict(BD, AL_maxiter=2), d=d, conv=[False], esc=[1e-12]),
        _sc(f"{k}_persist", k, dict(DEV, block_persist=True, device_options={"wide": 1}), d=d, esc=[-1.0, 1e-12]),
        _sc(f"{k}_round", k, dict(BD, round_blocks=True), d=d, esc=[-1.0, 1e-12]),
        _sc(f"{k}_round_host_factor", k, dict(eig="host", round_blocks=True), d=d, z=[1.0, -50.0]),
        _sc(f"{k}_round_degenerate", k, dict(BD, round_blocks=True), d=3, esc=[-1.0, 1e-12], ndeg={"round_blocks": [2]}),
        _sc(f"{k}_slow_device", k, dict(BD, AL_maxiter=100), d=d, esc=_slow()),
        _sc(f"{k}_zero_iterations", k, dict(AL_maxiter=0, round_blocks=True), d=d),
        _sc(f"{k}_Y0", k, dict(eig="host", Y0=("wide", 5)), d=3, z=[1.0, -50.0]),
        _sc(f"{k}_bad_d", k, None, d=4),
        _sc(f"{k}_round_refused", k, ROUND, d=d),
        _sc(f"{k}_comm_refused", k, dict(comm=(2, 0, b"id")), d=d),
        _sc(f"{k}_line_search_refused", k, dict(line_search=1), d=d),
        _sc(f"{k}_device_factor_refused", k, dict(device_factor=True), d=d),
        _sc(f"{k}_bad_block_factor", k, dict(block_factor="gpu"), d=d),
        _sc(f"{k}_bad_order", k, None, d=d, N=7),
        _sc(f"{k}_bad_eig", k, dict(eig="host_sparse"), d=d),
        _sc(f"{k}_p0_below_d", k, dict(p0=1), d=d),
        _sc(f"{k}_set_option_raises", k, dict(device_options={"nonsense": 1}), d=d, set_option_raises="nonsense"),
    ]
    return out


def _block_only():
    return [_sc("block_precon_refused", "block", dict(precon="blockjacobi"), d=2)]


def _pose_only():
    BD = dict(DEV, block_factor="device")
    return [
        _sc("pose_rerun_host", "pose", dict(eig="host"), d=2, z=[1.0, -50.0, -50.0, -50.0], gap=[0.5, 0.5, 0.5, 0.0]),
        _sc("pose_rerun_device", "pose", BD, d=2, esc=[-1.0, 1e-12, 1e-12, 1e-12], gap=[0.5, 0.5, 0.5, 0.0]),
        _sc("pose_rerun_host_factor_device_eig", "pose", DEV, d=3, esc=[1e-12, -1.0, 1e-12], gap=[0.5, 0.5, 0.0]),
        _sc("pose_rerun_until_maxiter", "pose", dict(BD, AL_maxiter=3), d=2, esc=[1e-12], gap=[0.5]),
        _sc("pose_gap_below_dinf_above", "pose", BD, d=2, esc=[-1.0, -1.0, 1e-12], gap=[0.0, 0.5, 0.0]),
        _sc("pose_slow_on_gap", "pose", dict(eig="host", AL_maxiter=100), z=[1.0], d=2, esc=[-1e-6], gap=[0.5] * 59 + [2.0]),
        _sc("pose_slow_on_gap_reruns", "pose", dict(BD, AL_maxiter=100), d=2, esc=[1e-12], gap=[0.5] * 59 + [2.0]),
        _sc("pose_precon", "pose", dict(DEV, precon="blockjacobi", block_persist=True), d=2, esc=[-1.0, 1e-12]),
        _sc("pose_precon_raises", "pose", dict(precon="blockjacobi"), d=2, set_option_raises="precon"),
        _sc("pose_bad_precon", "pose", dict(precon="jacobi"), d=2),
    ]


def scenarios():
    return _real() + _herm() + _blocks("block") + _block_only() + _blocks("pose") + _pose_only()


SCENARIOS = {sc["name"]: sc for sc in scenarios()}


# ---------------------------------------------------------------------------------------------------------------- recording
_TIME = re.compile(r"time(:| = )[0-9.]+s")


def _strip_times(data):
    out = {}
    for k, v in data.items():
        if k == "time" or k.endswith("_seconds"):
            continue
        if k == "log":
            v = _elide(digest([row[:-2] + row[-1:] for row in v]), 40, 8)   # (..., time, hessvecs): the time column goes
        out[k] = v
    return digest(out)


def record(sc):
    """Run one scenario against the scripted handle; see the module docstring for what comes back."""
    import pytest
    import scipy.sparse.linalg as spla
    from manisdp_matlab_amd import _lib, solvers
    calls, said, made = [], [], []
    kind, d = sc["kind"], sc.get("d", 0)
    mp = pytest.MonkeyPatch()

    def creator(name, **fixed):
        def create(cls, *a, **kw):
            calls.append(_call("create:" + name, a, kw))
            Cm = a[0]
            n = Cm if name == "dense_synthetic" else Cm.shape[0]
            blk = (a[1] + fixed.get("efree", 0)) if "efree" in fixed else 0
            dtype = np.complex128 if name == "onlyunitdiag_hermitian" else np.float64
            h = FakeHandle(calls, sc["script"], n, dtype=dtype, blk=blk, d=a[1] if blk else 0, efree=fixed.get("efree", 0))
            made.append(h)
            return h
        return classmethod(create)

    for name, fixed in (("onlyunitdiag", {}), ("onlyunitdiag_lowrank", {}), ("onlyunitdiag_hermitian", {}), ("dense_synthetic", {}),
                        ("onlyunitblockdiag", {"efree": 0}), ("posegraph", {"efree": 1})):
        mp.setattr(_lib.Handle, name, creator(name, **fixed))
    def default_opts(**kw):                                # (the real one asks the library for the defaults of the other fields)
        opts = _lib.RtrOpts()
        for k, v in kw.items():
            setattr(opts, k, v)
        return opts

    mp.setattr(_lib, "default_opts", default_opts)
    mp.setattr(solvers, "_say", lambda verbose, msg: said.append(_TIME.sub(r"time\1#s", msg)))
    real_eigsh = spla.eigsh                                # ARPACK draws its own start vector: a fixed one, for equal bytes
    mp.setattr(spla, "eigsh", lambda A, **kw: real_eigsh(A, v0=np.ones(A.shape[0]), **kw))
    o = dict(sc["options"])
    C = _problem(sc)
    if isinstance(o.get("Y0"), tuple):
        o["Y0"] = _wide_start(C.shape[0], d + (kind == "pose"), d, o["Y0"][1])
    try:
        if kind in ("real", "herm"):
            Y, obj, data = solvers.ManiSDP_onlyunitdiag(C, o, verbose=True, rng=np.random.default_rng(11))
        elif kind == "block":
            Y, obj, data = solvers.ManiSDP_onlyunitblockdiag(C, d, o, verbose=True, rng=np.random.default_rng(11))
        else:
            Y, obj, data = solvers.ManiSDP_posegraph(C, d, o, verbose=True, rng=np.random.default_rng(11))
        out = {"calls": _elide(calls, 120, 30), "said": _elide(said, 40, 8), "obj": obj, "data": _strip_times(data), "Y": digest(Y)}
    except Exception as err:                               # a scenario that raises
        out = {"calls": _elide(calls, 120, 30), "said": _elide(said, 40, 8), "raised": type(err).__name__, "message": str(err),
               "handles": len(made), "closed": [h.closed for h in made]}
    finally:
        mp.undo()
    return json.loads(json.dumps(out))


if __name__ == "__main__":                                 # OUT.json [scenario ...]: all scenarios, or the named entries of OUT.json anew
    names = sys.argv[2:] or list(SCENARIOS)
    traces = {}
    if sys.argv[2:]:
        with open(sys.argv[1]) as fh:
            traces = json.load(fh)
    traces.update({name: record(SCENARIOS[name]) for name in names})
    with open(sys.argv[1], "w") as fh:
        json.dump(traces, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{len(names)} of {len(traces)} scenarios recorded")
