"""GPU tests of the exact Hessian (qgd_eval_hessian): against the numpy statement (proto_hessian.py),
against differences of the device gradient for every cost type, symmetry, reproducibility, and the refusals."""
import numpy as np
import pytest

import cases
import proto_hessian as ph

pytestmark = pytest.mark.gpu


def _handle(qgd, prob, ctrl, target, order, cost_type="Infidelity"):
    dp = qgd.DeviceProblem(prob, order)
    dp.set_controls(ctrl); dp.set_target(target); dp.set_cost_type(cost_type)
    return dp


def _case(qgd, name):
    if name == "cnot2":
        return cases.cnot2_case(qgd, nsteps=12, tf=12.0)
    if name == "guarded":
        return cases.guarded_case(qgd, nsteps=10, tf=5.0)
    if name == "dense_guard":                     # a non-diagonal guard matrix W: the general guard kernels
        return cases.dense_guard_case(qgd, nsteps=10, tf=5.0)
    prob = qgd.construct_rand_prob(4, 1, tf=1.0, nsteps=10, gmres_abstol=1e-15, gmres_reltol=1e-15)
    ctrl = qgd.FortranBSplineControl(16, 20, prob.tf)
    pcof = np.random.default_rng(3).random(qgd.get_number_of_control_parameters(ctrl))
    return prob, ctrl, pcof, cases.rand_target(prob)


@pytest.mark.parametrize("name,order", [("cnot2", 2), ("cnot2", 4), ("cnot2", 8), ("guarded", 6),
                                        ("dense_guard", 6)])
def test_hessian_matches_numpy_statement(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    H0 = ph.hessian(prob, Gp, Gq, off, pcof, target, order)
    sc = np.abs(H0).max()
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        g_adj, _ = dp.discrete_adjoint(pcof)
        for path in ("dense", "sparse"):
            try:
                dp.set_operator_path(path)
            except qgd._lib.QGDError:
                continue                         # (the problem does not qualify for this operator path)
            grad = np.zeros(len(pcof))
            H = dp.eval_hessian(pcof, grad=grad)
            assert np.abs(H - H0).max() <= 1e-11 * sc, path
            assert np.abs(H - H.T).max() <= 1e-13 * sc
            assert np.abs(grad - g_adj).max() <= 1e-12 * max(1.0, np.abs(g_adj).max())
            assert np.array_equal(H, dp.eval_hessian(pcof))      # bitwise reproducible
    finally:
        dp.close()


@pytest.mark.parametrize("name", ["rand4", "guarded", "dense_guard"])
@pytest.mark.parametrize("cost_type", ["Tracking", "Norm", "Infidelity"])
def test_hessian_matches_gradient_differences(qgd, name, cost_type):
    order = 4
    prob, ctrl, pcof, target = _case(qgd, name)
    dp = _handle(qgd, prob, ctrl, target, order, cost_type)
    try:
        H = dp.eval_hessian(pcof)

        def fd(h):
            n = len(pcof)
            F = np.zeros((n, n))
            for l in range(n):
                e = np.zeros(n); e[l] = h
                F[:, l] = (dp.discrete_adjoint(pcof + e)[0] - dp.discrete_adjoint(pcof - e)[0]) / (2 * h)
            return F
        F = (4 * fd(5e-4) - fd(1e-3)) / 3
        assert np.abs(H - F).max() <= 1e-8 * np.abs(F).max()
        assert np.abs(H - H.T).max() <= 1e-13 * np.abs(H).max()
    finally:
        dp.close()


@pytest.mark.parametrize("nsteps", [20, 550])
def test_hessian_cnot3_directional(qgd, nsteps):
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=nsteps, tf=float(nsteps))
    dp = _handle(qgd, prob, ctrl, target, 8)
    try:
        H = dp.eval_hessian(pcof)
        rng = np.random.default_rng(7)
        sc = np.abs(H).max()
        for _ in range(3):
            v = rng.standard_normal(len(pcof)); v /= np.linalg.norm(v)
            w = rng.standard_normal(len(pcof)); w /= np.linalg.norm(w)

            def dd(h):
                return v @ (dp.discrete_adjoint(pcof + h * w)[0] - dp.discrete_adjoint(pcof - h * w)[0]) / (2 * h)
            ref = (4 * dd(5e-4) - dd(1e-3)) / 3
            assert abs(v @ H @ w - ref) <= 1e-7 * sc
    finally:
        dp.close()


def test_hessian_finite_difference_method(qgd):
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=12, tf=12.0)
    He = qgd.eval_hessian(prob, ctrl, pcof, target, order=4, method="exact")
    Hf = qgd.eval_hessian(prob, ctrl, pcof, target, dpcof=1e-5, order=4, method="finite_difference")
    assert np.abs(He - Hf).max() <= 1e-4 * np.abs(He).max() + 1e-5


def _refused(qgd, dp, pcof, code):
    with pytest.raises(qgd._lib.QGDError) as ei:
        dp.eval_hessian(pcof)
    assert ei.value.code == code


def test_hessian_refusals(qgd):
    L = qgd._lib
    # a windowed grid
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=100, tf=100.0)
    dp = qgd.DeviceProblem(prob, 4)
    dp.set_memory_budget(dp.memory_plan()["window_bytes"] // 3)
    dp.set_controls(ctrl); dp.set_target(target)
    try:
        assert dp.memory_plan()["windows"] > 1
        g0 = dp.discrete_adjoint(pcof)[0]
        _refused(qgd, dp, pcof, L.QGD_ERR_UNSUPPORTED)
        assert np.array_equal(dp.discrete_adjoint(pcof)[0], g0)
    finally:
        dp.close()
    # N > 64
    prob, ctrl, pcof, target = cases.synthetic_case(qgd, nsteps=4)
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        g0 = dp.discrete_adjoint(pcof)[0]
        _refused(qgd, dp, pcof, L.QGD_ERR_UNSUPPORTED)
        assert np.array_equal(dp.discrete_adjoint(pcof)[0], g0)
    finally:
        dp.close()
    # a partitioned handle
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=12, tf=12.0)
    rank = qgd.DeviceBackend(prob, 4, ctrl, target, 0, 2)      # rank 0 of a two-way time partition, controls and target set
    dp = rank.dp
    try:
        _refused(qgd, dp, pcof, L.QGD_ERR_STATE)
        assert "partitioned" in dp.lib.qgd_last_error(dp.h).decode()
    finally:
        dp.close()
    # a control that is not linear in its coefficients
    prob = qgd.construct_rabi_prob(tf=np.pi, nsteps=10)
    sc = cases.SineControl(prob.tf)
    with pytest.raises(NotImplementedError, match="linear"):
        qgd.eval_hessian(prob, sc, np.array([0.3, 1.1, 0.2]), cases.rand_target(prob), order=4)
    # the handle still works after a refusal
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=12, tf=12.0)
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        g0 = dp.discrete_adjoint(pcof)[0]
        with pytest.raises(qgd._lib.QGDError):
            dp.eval_hessian(pcof[:-1])
        assert np.array_equal(dp.discrete_adjoint(pcof)[0], g0)
    finally:
        dp.close()
