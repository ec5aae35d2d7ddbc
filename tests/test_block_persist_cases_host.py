"""CPU conditions on the inputs of tests/test_gpu_block_persist.py and tests/test_gpu_block_persist_instances.py
(tests/block_persist_cases.py): on every case the counts of the NumPy restatement's trustregions() do not change when the start
is perturbed by 1e-14 relative in five random directions, so that the summation order of a device path cannot change them; the
cases reach both families of inner stops and the branches they are there for; and the ledger: the Python restatement of the plan
equals msdp_blockpersist_plan.h, and the cases together reach every instance of k_tcg_persist_blk that a handle can select."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import block_persist_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stable(kind, n, d, p, maxiter, tol=K.TOLGRADNORM, masked=False, **opts):
    _, f0, i0 = K.restatement(kind, n, d, p, maxiter, tol, masked, **opts)
    C = K.masked_matrix(kind, n, d) if masked else K.matrix(kind, n, d)
    Y0 = K.start(kind, n, d, p)
    g = np.random.default_rng(99)
    for _ in range(5):
        _, f1, i1 = K.trustregions(kind, C, K.perturbed(kind, Y0, d, g), d, maxiter, tol, **opts)
        assert K.counts(i1) == K.counts(i0) and i1.numinner == i0.numinner, (kind, n, d, p, K.counts(i0), K.counts(i1))
        assert abs(f1 - f0) <= 1e-11 * abs(f0)
    return i0


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("n,d", K.SHAPES)
def test_sweep_cases_are_stable_under_perturbations_of_the_start(kind, n, d):
    for p in K.widths(d):
        i0 = _stable(kind, n, d, p, K.MAXITER)
        assert i0.iters == K.MAXITER and i0.hessvecs >= K.MAXITER


@pytest.mark.parametrize("case", K.LONG_CASES)
def test_long_cases_are_stable_under_perturbations_of_the_start(case):
    i0 = _stable(*case)
    assert i0.hessvecs >= 30


def test_cases_end_on_both_families_of_inner_stops():
    """A case that ends on the trust-region boundary or negative curvature (stop 1 or 2) and one that ends on the kappa / theta
    test (stop 3 or 4), for either kind."""
    for kind in K.KINDS:
        last = {K.restatement(k, n, d, p)[2].stop_inner[-1] for (k, n, d, p) in K.cases() if k == kind}
        last |= {K.restatement(*c)[2].stop_inner[-1] for c in K.LONG_CASES if c[0] == kind}
        assert last & {1, 2} and last & {3, 4}, (kind, last)


# ------------------------------------------------------------------ two row slots
@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("n,d", sorted(K.TWO_SLOT_SHAPES))
def test_two_slot_sweep_cases_are_stable_under_perturbations_of_the_start(kind, n, d):
    for p in K.TWO_SLOT_SHAPES[(n, d)]:
        i0 = _stable(kind, n, d, p, K.MAXITER)
        assert i0.iters == K.MAXITER and i0.hessvecs >= K.MAXITER


@pytest.mark.parametrize("case", K.LONG_TWO_SLOT_CASES)
def test_long_two_slot_cases_are_stable_under_perturbations_of_the_start(case):
    i0 = _stable(*case[:5])
    assert i0.hessvecs >= 30


def test_long_two_slot_cases_reach_the_instances_they_are_there_for():
    """Two slots in every case, sixteen workgroups in one at least; every HDER instance (pose, d = 3, lpr 2, 4, 8) and, for the
    Stiefel kind, both gather depths of its two-slot kernels; rejected iterations, stop 3 and the inner cap among them."""
    inst = {(c[0],) + K.instance_of(*c[:4], c[5]) for c in K.LONG_TWO_SLOT_CASES}
    assert all(i[4] == 2 for i in inst)
    assert {("pose", 3, 1, lpr, 2) for lpr in (2, 4, 8)} <= inst
    assert {K.gather_depth(i[1] + i[2], 2) for i in inst if i[0] == "stiefel"} == {4, 2}
    assert {K.gather_depth(i[1] + i[2], 2) for i in inst if i[0] == "pose"} == {2, 1}
    assert any(c[5] == 16 and K.plan_of(*c[:4], 16)["grid"] == 16 for c in K.LONG_TWO_SLOT_CASES)
    infos = [K.restatement(*c[:5])[2] for c in K.LONG_TWO_SLOT_CASES]
    assert any(i.rejected for i in infos) and any(3 in i.stop_inner for i in infos) and any(K.MAXINNER in i.numinner for i in infos)


def test_block_rows_leave_every_remainder_of_the_gather_depths():
    """The gathers take 4, 2 or 1 entries of a block row together and clamp the last group: block rows of every length modulo
    the depth occur, in one case per depth at least (gather_depth: 4 for B = 2, 2 for B = 3, 1 for B = 4 on two slots)."""
    for kind, n, d in (("stiefel", 521, 2), ("stiefel", 521, 3), ("pose", 521, 2), ("pose", 1031, 3)):
        B = K.blk(kind, d)
        depth = K.gather_depth(B, 2)
        lengths = K.block_row_lengths(K.matrix(kind, n, d), B)
        assert lengths.min() >= 2 and lengths.max() >= 9, (kind, n, d, lengths.min(), lengths.max())
        for depth in {depth, 4}:                                             # (4: the one-slot kernels of the same case)
            assert set(lengths % depth) == set(range(depth)), (kind, n, d, depth)


# ------------------------------------------------------------------ the step itself
@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("n,d,p", K.STEP_SHAPES)
def test_step_cases_run_their_trips_whatever_the_rounding(kind, n, d, p):
    """The tCG that the device's (eta, Heta) are compared with: trips and stop do not move under the perturbations, and from the
    warm start it runs five trips or more."""
    for warm in (False, True):
        _, _, trips, stop = K.first_step(kind, n, d, p, warm)
        Y0 = K.warm_start(kind, n, d, p) if warm else K.start(kind, n, d, p)
        g = np.random.default_rng(98)
        for _ in range(3):
            _, _, t1, s1 = K.first_step(kind, n, d, p, warm, Y=K.perturbed(kind, Y0, d, g))
            assert (t1, s1) == (trips, stop), (kind, n, d, p, warm, trips, stop, t1, s1)
        assert trips >= (5 if warm else 1), (kind, n, d, p, warm, trips)


# ------------------------------------------------------------------ trust-region options
@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("n,d,p", K.OPTION_SHAPES)
def test_option_cases_are_stable_under_perturbations_of_the_start(kind, n, d, p):
    for o in K.OPTION_SETS:
        _stable(kind, n, d, p, K.OPTION_MAXITER[kind], **o)


def test_option_cases_reach_the_branches_of_the_inner_stop():
    """Stop 3 and stop 4; a tCG as long as mininner > 1; a case with theta != 1 that ends on stop 3 or 4 (the pow branch of the
    kernel decides there)."""
    for kind in K.KINDS:
        stops, at_mininner, pow_stop = set(), False, False
        for (n, d, p) in K.OPTION_SHAPES:
            for o in K.OPTION_SETS:
                info = K.restatement(kind, n, d, p, K.OPTION_MAXITER[kind], **o)[2]
                stops |= set(info.stop_inner)
                at_mininner |= o["mininner"] > 1 and any(nu == o["mininner"] and s in (3, 4) for nu, s in zip(info.numinner, info.stop_inner))
                pow_stop |= o["theta"] != 1.0 and info.stop_inner[-1] in (3, 4)
        assert {3, 4} <= stops and at_mininner and pow_stop, (kind, stops, at_mininner, pow_stop)


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("case", K.FINISHED_CASES)
def test_finished_cases_converge_within_their_budget(case):
    kind, n, d, p, maxiter, tol = case
    i0 = _stable(kind, n, d, p, maxiter, tol)
    assert 0 < i0.iters < maxiter and i0.gradnorm < tol
    # a second call from the end point does nothing
    Y = K.restatement(kind, n, d, p, maxiter, tol)[0]
    _, _, i1 = K.trustregions(kind, K.matrix(kind, n, d), Y, d, maxiter, tol)
    assert i1.iters == 0 and i1.hessvecs == 0


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", K.FEW_BLOCKS)
def test_few_block_cases_are_stable_under_perturbations_of_the_start(kind, n, d):
    for p in (d, 32):
        _stable(kind, n, d, p, K.MAXITER)
        pl = K.plan_of(kind, n, d, p)
        assert pl["grid"] == 8 and pl["slots"] == 1 and n < 2 * pl["grid"]     # chunks of one block or none at the planned grid


@pytest.mark.parametrize("kind", K.KINDS)
def test_cap_too_small_case(kind):
    n, d, p = K.CAP_TOO_SMALL
    assert K.plan_of(kind, n, d, p, 8) is None and n > 16 * K.rstep_of(K.lpr_of(p))
    assert K.plan_of(kind, n, d, p, 0)["slots"] == 1
    _stable(kind, n, d, p, K.MAXITER)


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("n,d,p", K.MASKED_SHAPES)
def test_masked_cases_are_stable_and_have_empty_block_rows(kind, n, d, p):
    B = K.blk(kind, d)
    keep = K.block_mask(n)
    lengths = K.block_row_lengths(K.masked_matrix(kind, n, d), B)
    assert 0.15 * n < np.sum(~keep) < 0.35 * n
    assert np.all(lengths[~keep] == 0) and np.all(lengths[keep] >= 1)
    assert lengths[keep].min() <= 2                                          # neighbours of removed blocks are left with little
    i0 = _stable(kind, n, d, p, K.MAXITER, masked=True)
    assert i0.iters == K.MAXITER and i0.hessvecs >= K.MAXITER


# ------------------------------------------------------------------ the ledger
def _header_plans(tmp_path, queries):
    """The plans of msdp_blockpersist_plan.h for (nb, B, efree, p, cus, cap, wide) queries, through the header's self-test tool."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "block_persist_plan_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "manisdp-matlab_amd", "csrc"),
                    os.path.join(ROOT, "tools", "block_persist_plan_selftest.cpp"), "-o", exe], check=True)
    text = "".join("%d %d %d %d %d %d %d\n" % q for q in queries)
    r = subprocess.run([exe, "--plans"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(queries)
    return rows


def test_python_plan_equals_the_header(tmp_path):
    """plan() of block_persist_cases.py against msdp_blockpersist_plan of the header: on every run of the ledger and on a grid
    of block counts around every slot boundary, all widths 1 .. 34, the four block shapes, three devices, three caps, wide."""
    queries = [(n, K.blk(kind, d), int(kind == "pose"), p, K.CUS, cap, 0) for (kind, n, d, p, cap) in K.gpu_runs()]
    nbs = sorted({v + e for v in (1, 8, 64, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536) for e in (-1, 0, 1)} - {0}
                 | {5, 9, 343, 6150, 20000})
    for (B, ef) in ((2, 0), (3, 0), (3, 1), (4, 1)):
        for cus in (64, 256, 304):
            for cap in (0, 8, 16):
                for p in range(1, 35):
                    queries += [(nb, B, ef, p, cus, cap, wide) for nb in nbs for wide in (0, 1)]
    rows = _header_plans(tmp_path, queries)
    for q, row in zip(queries, rows):
        pl = K.plan(*q[:4], cus=q[4], grid_cap=q[5], wide=q[6])
        mine = (1, pl["lpr"], pl["grid"], pl["slots"], pl["rstep"], pl["lds"]) if pl else (0, 0, 0, 0, 0, 0)
        assert row == mine, (q, row, mine)


def test_ledger_every_reachable_instance_runs_under_a_test():
    """The runs of the device tests reach 36 of the 40 instantiated kernels; the other four, <3, *, 1, *>, cannot be selected
    (D = 3 needs p >= 3, hence lpr >= 2), and no run maps to them."""
    assert len(K.INSTANTIATED) == 40 and len(K.UNREACHABLE) == 4 and K.UNREACHABLE < K.INSTANTIATED
    # nothing reaches them: every admissible width of d = 3, every block count that matters, both caps
    for kind in K.KINDS:
        for p in range(3, 33):
            for n in (1, 343, 4099, 8192, 8193, 16384):
                for cap in (0, 8, 16):
                    assert K.instance_of(kind, n, 3, p, cap) not in K.UNREACHABLE
    reached = {K.instance_of(*run) for run in K.gpu_runs()}
    assert None not in reached
    assert not reached & K.UNREACHABLE
    assert reached == K.INSTANTIATED - K.UNREACHABLE and len(reached) == 36, sorted(K.INSTANTIATED - K.UNREACHABLE - reached)
    # the LDS of the largest instance, <3, 1, 2, 2>, as the header's comment has it
    assert K.lds_of(4, 1, 2, 2) == 151552 and max(K.lds_of(D + EF, EF, l, R) for (D, EF, l, R) in reached) == 151552
    # every two-slot shape takes two slots under the cap and one at the planned grid
    for (kind, n, d, p) in K.two_slot_cases():
        assert K.instance_of(kind, n, d, p, 8)[3] == 2 and K.instance_of(kind, n, d, p, 0)[3] == 1
        assert K.plan_of(kind, n, d, p, 8)["grid"] == 8
