"""Host checks (no GPU) of tests/tr_decisions_ref.py: the restatement with records against oracle.manopt_rtr.trustregions, and the
case table against the coverage tests/test_gpu_tr_decisions.py relies on.  A case that misses a check here is replaced; the cut-off
DECIDED = 1e-9 is not moved.

Per route row (a route through the decision code), the compared prefixes of its cases (T.prefix: the decided prefix, cut where the
reference's own cost stops being reproducible to the device's bound) together must contain the stop codes 1 to 5, the
outcomes accept-double, accept-double_capped, accept-keep, accept-quarter and reject-quarter, and a stop on tolgradnorm at an
iteration 0 < k < MAXITER.

Stop 6 (the model value does not decrease, tCG.m:228) is required of a row only where the reference reaches it decided.  It reaches
it decided in NO row (STOP6_DECIDED_ROWS is empty): only theta1 on the sphere ends a tCG with it (p = 3: iteration 12 under
theta = 2 and iteration 11 under mininner = 5 with theta = 2; p = 6: iteration 12 from Delta0 = Delta_bar), each time two to five
iterations behind the first undecided one (margins 6e-14, 1e-13 and 2e-10: rhoden against 0 next to a stationary point); no
other case of the table reaches it at all.  No input is doctored to force it."""
import functools

import numpy as np
import pytest

import tr_decisions_ref as T

STOP6_DECIDED_ROWS = set()


def _pairs():
    return [(name, opt) for name in T.ALL_CASES for opt in T.OPTION_SETS]


@functools.lru_cache(maxsize=None)
def _oracle(name, opt):
    """oracle.manopt_rtr.trustregions (with the preconditioned tCG of posegraph_precon_ref where the case has a preconditioner)."""
    from oracle import manopt_rtr
    c = T.case(name)
    o = dict(T.options(name, opt))
    maxinner, tol = o.pop("maxinner"), o.pop("tolgradnorm")
    if c.kind == "posegraph_precon":
        import posegraph_precon_ref as P
        return P.trustregions(c.data, np.array(c.Y0), c.par["d"], T.MAXITER, maxinner, tol, **o)
    return manopt_rtr.trustregions(c.problem(), np.array(c.Y0), T.MAXITER, maxinner, tol, **o)


@pytest.mark.parametrize("name", T.ALL_CASES)
def test_restatement_equals_the_oracle(name):
    """Every case under every option set: the same totals, per-iteration inner counts and stop codes, and bit for bit the same
    cost, gradient norm, radius and end point."""
    for opt in T.OPTION_SETS:
        run = T.reference(name, opt)
        x, fx, info = _oracle(name, opt)
        a, b = run.info, info
        what = (name, opt)
        assert (a.iters, a.hessvecs, a.accepted, a.rejected, a.cost_evals) == (b.iters, b.hessvecs, b.accepted, b.rejected, b.cost_evals), what
        assert a.stop_inner == b.stop_inner and a.numinner == b.numinner, what
        assert (a.cost, a.gradnorm, a.Delta, run.fx) == (b.cost, b.gradnorm, b.Delta, fx), what
        assert np.array_equal(run.x, x), what
        assert run.totals() == (b.iters, b.hessvecs, b.accepted, b.rejected, b.stop_inner[-1] if b.stop_inner else 0), what
        assert [r["numinner"] for r in run.records] == b.numinner and [r["stop_inner"] for r in run.records] == b.stop_inner
        if run.records:
            last = run.records[-1]
            assert (last["Delta"], last["cost"], last["gradnorm"]) == (b.Delta, b.cost, b.gradnorm), what


def test_records_follow_the_radius_rule():
    """The action of a record is what its radii say: Delta / 4, 2 Delta, Delta_bar from more than half of it, or unchanged."""
    for name, opt in _pairs():
        run = T.reference(name, opt)
        o = T.options(name, opt)
        bar = o.get("Delta_bar", T.case(name).problem().M.typicaldist())
        prev = o.get("Delta0", bar / 8.0)
        for r in run.records:
            want = {"quarter": prev / 4.0, "double": 2.0 * prev, "double_capped": bar, "keep": prev}[r["action"]]
            assert r["Delta"] == want, (name, opt, r)
            assert r["action"] != "double_capped" or 2.0 * prev > bar, (name, opt, r)
            assert r["action"] != "double" or r["Delta"] <= bar, (name, opt, r)
            prev = r["Delta"]


@functools.lru_cache(maxsize=None)
def _row_coverage(row):
    stops, outcomes, tol_stop = set(), set(), []
    for name in T.row_cases(row):
        for opt in T.OPTION_SETS:
            run = T.reference(name, opt)
            s, o = run.outcomes(T.prefix(name, opt))
            stops |= s
            outcomes |= o
            if T.ends_in_mid_run(name, opt):
                tol_stop.append((name, opt, len(run.records)))
    return stops, outcomes, tol_stop


@pytest.mark.parametrize("row", T.ROWS)
def test_row_reaches_every_outcome_decided(row):
    stops, outcomes, tol_stop = _row_coverage(row)
    print(f"{row}: stop codes {sorted(stops)}, outcomes {sorted(outcomes)}, tolgradnorm stops {tol_stop}")
    for name in T.row_cases(row):
        print(f"  {name}: compared / decided / run " + ", ".join(f"{opt} {T.prefix(name, opt)}/{T.reference(name, opt).decided_prefix()}/{len(T.reference(name, opt).records)}"
                                                                 for opt in T.OPTION_SETS))
    assert T.STOPS_REQUIRED <= stops, (row, T.STOPS_REQUIRED - stops)
    assert T.OUTCOMES_REQUIRED <= outcomes, (row, T.OUTCOMES_REQUIRED - outcomes)
    assert tol_stop, row
    assert (6 in stops) == (row in STOP6_DECIDED_ROWS), (row, "stop 6: the docstring of this file is out of date")


@pytest.mark.parametrize("row", T.ROWS)
def test_every_option_is_under_test_in_every_row(row):
    """mininner, kappa, theta, rho_prime and rho_regularization each change the record sequence of at least one case of the row
    against the set without the option, inside the compared prefix of both."""
    for option, sets in T.OPTIONS_UNDER_TEST.items():
        changed = []
        for name in T.row_cases(row):
            for opt in sets:
                a, b = T.reference(name, opt), T.reference(name, T.OPTION_BASE[opt])
                k = min(T.prefix(name, opt), T.prefix(name, T.OPTION_BASE[opt]))
                if a.sequence(k) != b.sequence(k):
                    changed.append((name, opt))
        print(f"{row}: {option} changes {changed}")
        assert changed, (row, option)


@pytest.mark.parametrize("name", T.ALL_CASES)
def test_case_has_six_decided_iterations(name):
    """Six decided iterations under its default options, at least four of them carried by the reference (T.prefix: the two warm
    preconditioned cases, next to a stationary point, carry four and five; every other case six or more).  The other sets are
    printed (a set that stops on tolgradnorm in mid-run is shorter by design) and compare one iteration at the least."""
    run = T.reference(name, "default")
    print(name, "compared / decided:", {opt: (T.prefix(name, opt), T.reference(name, opt).decided_prefix()) for opt in T.OPTION_SETS})
    assert run.decided_prefix() >= 6, (name, [r["margin"] for r in run.records])
    assert T.prefix(name, "default") >= (4 if ":w" in name else 6), name
    for opt in T.OPTION_SETS:
        assert 1 <= T.prefix(name, opt) <= T.reference(name, opt).decided_prefix(), (name, opt)
    tol = T.reference(name, "tolgrad")
    assert tol.ended == "tolgradnorm" and 0 < len(tol.records) < T.MAXITER, name


def test_every_route_names_a_case_and_every_case_a_route():
    assert set(T.ALL_CASES) == {c for r in T.ROUTES.values() for c in r["cases"]}
    assert len(T.ROWS) == 10
    for r in T.ROUTES.values():
        assert r["cases"] and r["path"] in (0, 1) and (r["path"] == 1) == (r["trip"] == 0)
