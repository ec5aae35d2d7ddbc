"""Every exit of the truncated CG and every outcome of the trust-region update, iteration by iteration, in every route through the decision
code (the routing table ROUTES of tests/tr_decisions_ref.py).

For each (route, case, option set) and each k = 1 ... K, K = tr_decisions_ref.prefix (the decided prefix of the case under the set, cut
where the reference's own cost is no longer reproducible to the bound below): set_point(Y0), one
rtr(maxiter = k) and a comparison with the first k records of the reference.  The differences of successive prefixes are the single
iterations' inner counts, stop codes and decisions; the fused launches run maxiter = k whole, which is their "stop at iteration k"
exit for every k.  Where the reference ends on tolgradnorm in mid-run with everything decided, one more call with the whole budget
must end there too.

Compared: (iters, hessvecs, accepted, rejected, last_stop_inner) equal; Delta equal bit for bit (it only ever takes the values
Delta0 2^m and Delta_bar); cost to 1e-11 and gradient norm to 1e-8 relative, the bounds of tests/test_gpu_fused_early_gather.py.
After every call the route is asserted through tcg_path(), persist_form(), trip_form() and block_persist_plan(): a silent
fall-back to another copy fails.  A handle serves all option sets of its case in turn, and the last test alternates sets call
by call: the options of a call must not outlive it."""
import time

import pytest

import tr_decisions_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _open(lib, route, name, graph):
    h = T.case(name).handle(lib)
    for key, value in T.ROUTES[route]["opts"]:
        h.set_option(key, value)
    if graph is not None:
        h.set_option("graph", graph)
    return h


def _on_route(h, route):
    R = T.ROUTES[route]
    got = (h.tcg_path(), h.trip_form())
    assert got == (R["path"], R["trip"]), (route, got)
    if "form" in R:
        assert h.persist_form() == R["form"], (route, h.persist_form())
    if R.get("block_persist"):
        assert h.block_persist_plan()["eligible"] == 1, (route, h.block_persist_plan())


def _call(lib, h, route, name, opt, k):
    """One rtr(maxiter = k) from the case's start under the option set, held to the reference's first records; returns the relative
    differences of cost and gradient norm."""
    run = T.reference(name, opt)
    rec = run.records[:k]
    h.set_point(T.case(name).Y0)
    st = h.rtr(lib.default_opts(maxiter=k, **T.options(name, opt)))
    _on_route(h, route)
    what = f"{route} {name} {opt} maxiter={k}"
    got = (st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner)
    want = run.totals(k)
    dc = abs(st.cost - rec[-1]["cost"]) / max(1.0, abs(rec[-1]["cost"]))
    dg = abs(st.gradnorm - rec[-1]["gradnorm"]) / max(1.0, rec[-1]["gradnorm"])
    if got != want or st.Delta != rec[-1]["Delta"] or not dc < 1e-11 or not dg < 1e-8:
        print(f"{what}: device {got} Delta {st.Delta!r} / reference {want} Delta {rec[-1]['Delta']!r}, cost {dc:.2e}, gradnorm {dg:.2e}; "
              f"the reference's iterations (inner/stop, accepted, action, margin): "
              + " ".join(f"{r['numinner']}/{r['stop_inner']} {'A' if r['accepted'] else 'R'} {r['action']} {r['margin']:.1e}" for r in rec))
    assert got == want, what
    assert st.Delta == rec[-1]["Delta"], what
    assert dc < 1e-11, what
    assert dg < 1e-8, what
    return dc, dg


def _budgets(name, opt):
    """The prefixes to run: 1 ... K, and the whole budget where the reference ends on tolgradnorm before it, all compared."""
    ks = list(range(1, T.prefix(name, opt) + 1))
    if T.ends_in_mid_run(name, opt):
        ks.append(T.MAXITER)
    return ks


@pytest.mark.parametrize("route,name", [(route, name) for route, R in T.ROUTES.items() for name in R["cases"]])
def test_route_takes_the_reference_decisions_at_every_iteration(lib, route, name):
    t0 = time.perf_counter()
    calls = 0
    for graph in T.ROUTES[route].get("graphs", (None,)):
        h = _open(lib, route, name, graph)
        try:
            for opt in T.OPTION_SETS:
                run = T.reference(name, opt)
                worst = (0.0, 0.0)
                for k in _budgets(name, opt):
                    dc, dg = _call(lib, h, route, name, opt, k)
                    worst = (max(worst[0], dc), max(worst[1], dg))
                    calls += 1
                stops, outcomes = run.outcomes(T.prefix(name, opt))
                print(f"{route} {name} graph={graph} {opt}: {T.prefix(name, opt)} of {len(run.records)} iterations compared, stops {sorted(stops)}, "
                      f"outcomes {sorted(outcomes)}, ended on {run.ended}; cost {worst[0]:.2e}, gradnorm {worst[1]:.2e}")
        finally:
            h.close()
    print(f"{route} {name}: {calls} calls in {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("route", list(T.ROUTES))
def test_options_of_a_call_do_not_outlive_it(lib, route):
    """One handle, the option sets alternating call by call (theta and kappa, Delta_bar and Delta0, mininner, rho_prime, the inner
    cap, the gradient tolerance and the defaults), twice around, each call at the whole decided prefix of its set: the control block
    is filled per call, and a chunk graph captured under one set is replayed under the next."""
    name = T.ROUTES[route]["cases"][0]
    for graph in T.ROUTES[route].get("graphs", (None,)):
        h = _open(lib, route, name, graph)
        try:
            for _ in range(2):
                for opt in ("theta2", "delta_small", "mininner5_theta2", "rho_prime_delta0_bar", "maxinner3", "tolgrad", "rho_reg", "default"):
                    ks = _budgets(name, opt)
                    assert ks, (name, opt)
                    _call(lib, h, route, name, opt, ks[-1])
        finally:
            h.close()
