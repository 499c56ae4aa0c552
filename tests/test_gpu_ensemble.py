"""GPU tests of ensemble evaluation (quantumgatedesign.jl_amd/ensemble.py): ONE coefficient vector over K
variants of a problem -- system Hamiltonian and control-operator scales --, every member on a handle of its own, the weighted
sums formed by ``ensemble_reduce``.  The contract is bitwise: the members' rows are what a handle made for
``Ensemble.member_problem(prob, k)`` returns, and the sums are ``ensemble_reduce`` of those rows.  Every case is a few time
points."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu


def _member_rows(qgd, ens, prob, order, ctrl, target, pcof, cost="Infidelity", gradient=True):
    """every member on a handle made here: (grads [K, n] or None, out3 [K, 3])"""
    G, O = [], []
    for k in range(ens.K):
        dp = qgd.DeviceProblem(ens.member_problem(prob, k), order)
        try:
            dp.set_controls(ctrl); dp.set_target(target); dp.set_cost_type(cost)
            if gradient:
                g, o = dp.discrete_adjoint(pcof)
                G.append(g)
            else:
                o = dp.eval_forward(pcof)
            O.append(np.asarray(o, dtype=np.float64).copy())
        finally:
            dp.close()
    return (np.array(G) if gradient else None), np.array(O)


def _assert_is_the_statement_of_the_members(qgd, ens, prob, order, ctrl, target, pcof, cost="Infidelity"):
    res = qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, ens, order=order, cost_type=cost)
    G, O = _member_rows(qgd, ens, prob, order, ctrl, target, pcof, cost)
    assert np.array_equal(res.member_grads, G) and np.array_equal(res.member_out3, O)
    rg, rc, rgd = qgd.ensemble_reduce(G, O, ens.weights, cost, prob.N_ess_levels)
    grad, c, gd = res
    assert np.array_equal(grad, rg) and c == rc and gd == rgd and np.abs(grad).max() > 0
    fwd = qgd.eval_ensemble(prob, ctrl, pcof, target, ens, order=order, cost_type=cost, gradient=False)
    _, Of = _member_rows(qgd, ens, prob, order, ctrl, target, pcof, cost, gradient=False)
    assert fwd.grad is None and fwd.member_grads is None and np.array_equal(fwd.member_out3, Of)
    _, fc, fgd = qgd.ensemble_reduce(None, Of, ens.weights, cost, prob.N_ess_levels)
    assert (fwd.cost, fwd.guard) == (fc, fgd)
    return res


@pytest.mark.parametrize("cost", ["Infidelity", "Tracking"])
def test_members_are_handles_of_their_own_and_the_sums_the_statement(qgd, cost):
    """cnot2 at 6 steps, order 4, K = 4: the problem's own Hamiltonian; a diagonal detuning shift; a shift plus an antisymmetric
    part; a shift with op_scale = (1.03, 0.97).  Gauss-Legendre-like non-uniform weights, then weights = None."""
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=6, tf=6.0)
    K = 4
    S = np.repeat(prob.system_sym[None], K, axis=0).copy()
    A = np.repeat(prob.system_asym[None], K, axis=0).copy()
    scale = np.ones((K, prob.N_operators))
    for k in range(1, K):
        S[k] += np.diag(np.array([0.0, 0.011, -0.023, 0.017]) * (1.0 + 0.37 * (k - 1)))
    A[2, 0, 1], A[2, 1, 0] = 0.004, -0.004
    scale[3] = (1.03, 0.97)
    for weights in ([0.17, 0.33, 0.33, 0.17], None):
        ens = qgd.Ensemble(S, A, scale, weights)
        res = _assert_is_the_statement_of_the_members(qgd, ens, prob, 4, ctrl, target, pcof, cost)
        assert len({g.tobytes() for g in res.member_grads}) == 4       # (four different members)
    again = qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, ens, order=4, cost_type=cost)      # two calls, the same bits
    assert np.array_equal(again.grad, res.grad) and again[1:] == res[1:] and np.array_equal(again.member_grads, res.member_grads)
    g0 = qgd.discrete_adjoint(prob, ctrl, pcof, target, order=4, cost_type=cost)
    assert np.array_equal(res.member_grads[0], g0)                     # member 0 is the problem itself
    one = qgd.Ensemble(S[:1], A[:1])                                   # K = 1, weight 1.0: the single call
    r1 = qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, one, order=4, cost_type=cost)
    assert np.array_equal(r1.grad, g0)
    qgd.clear_cache()


@pytest.mark.parametrize("N,c,n_ops,order,nsteps,cost", [(4, 4, 2, 6, 5, "Infidelity"), (3, 2, 1, 4, 2, "Tracking"), (4, 3, 3, 8, 9, "Norm"),
                                                         (2, 2, 4, 2, 33, "Infidelity"), (4, 1, 2, 12, 17, "Infidelity"),
                                                         (3, 3, 2, 4, 7, "StateTransfer")])
def test_shapes_guards_and_cost_types(qgd, orc, N, c, n_ops, order, nsteps, cost):
    """The shapes of tests/test_gpu_batch.py::test_shapes_the_path_covers (random dense problems with a diagonal guard projector,
    built as there) and one StateTransfer case; K = 3 members from seeded symmetric / antisymmetric perturbations of size 0.1
    (member 0 unperturbed), non-uniform weights and operator scales.  Rows bitwise against handles made for the members, the
    sums -- the weighted guard penalty among them -- bitwise the statement; member 0 against the oracle at that file's bound,
    1e-10 of the gradient's maximum (StateTransfer, which the oracle does not have: against this library's general kernels at
    the same bound)."""
    prob = qgd.construct_rand_prob(N, n_ops, tf=1.0, nsteps=nsteps, gmres_abstol=1e-15, gmres_reltol=1e-15, scale=0.7)
    prob.u0 = np.asfortranarray(prob.u0[:, :c]); prob.v0 = np.asfortranarray(prob.v0[:, :c]); prob.N_initial_conditions = c
    rng = np.random.default_rng(N * 100 + c)
    W = np.zeros((2 * N, 2 * N))
    wd = rng.random(N) * (rng.random(N) > 0.4)
    W[np.arange(N), np.arange(N)] = wd; W[N + np.arange(N), N + np.arange(N)] = wd
    prob.guard_subspace_projector = W
    ctrl = [qgd.FortranBSplineControl(3, 5, prob.tf) for _ in range(n_ops)]
    pcof = rng.standard_normal(qgd.get_number_of_control_parameters(ctrl))
    target = cases.rand_target(prob)
    if cost == "StateTransfer":
        target = target / np.linalg.norm(target, axis=0)
    r = 0.1 * rng.standard_normal((3, N, N)); r[0] = 0.0
    ens = qgd.Ensemble(prob.system_sym[None] + (r + r.transpose(0, 2, 1)), prob.system_asym[None] + (r - r.transpose(0, 2, 1)),
                       1.0 + 0.05 * rng.standard_normal((3, n_ops)) * np.array([[0.0], [1.0], [1.0]]), [0.3, 0.45, 0.25])
    res = _assert_is_the_statement_of_the_members(qgd, ens, prob, order, ctrl, target, pcof, cost)
    G, O = res.member_grads, res.member_out3
    if cost == "StateTransfer":
        dp = qgd.DeviceProblem(prob, order)
        try:
            dp.set_small_path(False); dp.set_controls(ctrl); dp.set_target(target); dp.set_cost_type(cost)
            g_ref, _ = dp.discrete_adjoint(pcof)
            assert not dp.small_path_taken()
        finally:
            dp.close()
    else:
        orc.set_converged_terminal(True); orc.set_cost_type(cost)
        try:
            g_ref = orc.discrete_adjoint(prob, ctrl, pcof, target, order=order)
        finally:
            orc.set_converged_terminal(False); orc.set_cost_type("Infidelity")
    assert np.abs(G[0] - g_ref).max() <= 1e-10 * np.abs(g_ref).max()
    assert O[0, 2] > 0 or not wd.any()
    assert res.guard > 0 or not wd.any()
    assert len({g.tobytes() for g in G}) == 3
    qgd.clear_cache()


def test_gradient_is_the_gradient_of_cost_plus_guard(qgd):
    """cnot2 at 6 steps, order 4, K = 4 with non-uniform weights: centred differences (dpcof = 1e-5) of the forward-only call's
    cost + guard against grad, at 1e-8 max(1, max|g|)."""
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=6, tf=6.0)
    K = 4
    S = np.repeat(prob.system_sym[None], K, axis=0).copy()
    for k in range(1, K):
        S[k] += np.diag(np.array([0.0, 0.011, -0.023, 0.017]) * (1.0 + 0.37 * (k - 1)))
    scale = np.ones((K, prob.N_operators)); scale[3] = (1.03, 0.97)
    ens = qgd.Ensemble(S, np.repeat(prob.system_asym[None], K, axis=0), scale, [0.1, 0.4, 0.3, 0.2])
    grad = qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, ens, order=4).grad
    J = lambda p: sum(qgd.eval_ensemble(prob, ctrl, p, target, ens, order=4, gradient=False)[1:])
    d, fd = 1e-5, np.zeros(len(pcof))
    for i in range(len(pcof)):
        e = np.zeros(len(pcof)); e[i] = d
        fd[i] = (J(pcof + e) - J(pcof - e)) / (2 * d)
    err = np.abs(fd - grad).max()
    print(f"\nensemble gradient against centred differences: {err:.3e}, max|g| = {np.abs(grad).max():.3e}")
    assert err <= 1e-8 * max(1.0, np.abs(grad).max())
    qgd.clear_cache()


def test_nine_levels(qgd):
    """A problem beyond the small-problem kernels (the one of tests/test_gpu_batch.py::test_loop_route_nine_levels), K = 2."""
    prob = qgd.construct_rand_prob(9, 2, tf=1.0, nsteps=5, gmres_abstol=1e-15, gmres_reltol=1e-15, scale=0.7)
    prob.u0 = np.asfortranarray(prob.u0[:, :2]); prob.v0 = np.asfortranarray(prob.v0[:, :2]); prob.N_initial_conditions = 2
    ctrl = [qgd.FortranBSplineControl(3, 5, prob.tf) for _ in range(2)]
    pcof = np.random.default_rng(9).standard_normal(qgd.get_number_of_control_parameters(ctrl))
    target = cases.rand_target(prob)
    r = 0.1 * np.random.default_rng(10).standard_normal((2, 9, 9))
    ens = qgd.Ensemble(prob.system_sym[None] + (r + r.transpose(0, 2, 1)), prob.system_asym[None] + (r - r.transpose(0, 2, 1)),
                       [[1.0, 1.0], [1.02, 0.98]], [0.4, 0.6])
    _assert_is_the_statement_of_the_members(qgd, ens, prob, 4, ctrl, target, pcof)
    qgd.clear_cache()


def test_optimize_gate_over_an_ensemble(qgd):
    """Rabi pi-pulse over three detunings, 10 iterations: the robust objective descends, its optimum scores a lower mean
    infidelity over the ensemble than the nominal-only optimum of the same start and iterations; ensemble=None is today's call."""
    prob = qgd.construct_rabi_prob(tf=np.pi, nsteps=20)
    control = qgd.GRAPEControl(1, prob.tf)
    target = np.array([[0.0, 1.0], [1.0, 0.0]])
    p0 = np.array([0.45, 0.05])
    deltas, w = (-0.3, 0.0, 0.3), [0.25, 0.5, 0.25]
    ens = qgd.Ensemble(np.stack([np.diag([0.0, d]) for d in deltas]), np.zeros((3, 2, 2)), None, w)
    kw = dict(order=8, ridge_penalty_strength=0, maxIter=10, print_level=0)
    nominal = qgd.optimize_gate(prob, control, p0, target, **kw)
    same = qgd.optimize_gate(prob, control, p0, target, ensemble=None, **kw)
    assert len(same) == len(nominal) and all(np.array_equal(a, b) for a, b in zip(same.pcof, nominal.pcof))
    for f in ("ipopt_obj_value", "infidelity", "guard_penalty", "ridge_penalty"):
        assert np.array_equal(getattr(same, f), getattr(nominal, f)), f
    assert all(np.array_equal(a, b) for a, b in zip(same.grad_pcof, nominal.grad_pcof))
    robust = qgd.optimize_gate(prob, control, p0, target, ensemble=ens, **kw)
    obj = np.asarray(robust.analytic_obj_value)
    assert len(obj) >= 2 and np.all(np.diff(obj) <= 0.0)
    assert np.array_equal(np.asarray(robust.infidelity) + np.asarray(robust.guard_penalty), obj)
    mean = lambda p: qgd.discrete_adjoint_ensemble(prob, control, p, target, ens, order=8)
    at_robust, at_nominal = mean(robust.pcof[-1]), mean(nominal.pcof[-1])
    print(f"\nmean infidelity over the ensemble: robust optimum {at_robust.cost:.6e}, nominal optimum {at_nominal.cost:.6e}; "
          f"nominal infidelity {nominal.infidelity[-1]:.3e}")
    assert at_robust.cost == robust.infidelity[-1]
    assert at_robust.cost < at_nominal.cost
    qgd.clear_cache()
