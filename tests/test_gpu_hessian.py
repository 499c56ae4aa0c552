"""GPU tests of the exact Hessian (qgd_eval_hessian): against the numpy statement (proto_hessian.py),
against differences of the device gradient for every cost type, symmetry, reproducibility, the refusals, and the buffers
the forced gradient, the Hessian and the Hessian-vector product keep on a handle: that they follow the grid and the control
basis, and that the byte count of a QGD_ERR_MEMORY refusal is the amount that decides it."""
import re

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


def _sensitivities(dp, pcof, V):
    grad_h, grad_v = np.zeros(len(pcof)), np.zeros(len(pcof))
    return (dp.eval_grad_forced(pcof), dp.eval_hessian(pcof, grad=grad_h), grad_h, dp.eval_hessian_vec(pcof, V, grad=grad_v), grad_v)


@pytest.mark.parametrize("name,order", [("cnot2", 4), ("guarded", 6)])
def test_sensitivity_buffers_follow_grid_and_basis(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    ctrl2 = [qgd.CarrierControl(qgd.FortranBSplineControl(2, 6, prob.tf), [0.0, -1.0]) for _ in range(prob.N_operators)]
    pcof2 = 0.05 * (0.5 - np.random.default_rng(6).random(qgd.get_number_of_control_parameters(ctrl2)))
    assert len(pcof2) != len(pcof)
    rng = np.random.default_rng(12)
    V, V2 = rng.standard_normal((len(pcof), 2)), rng.standard_normal((len(pcof2), 2))

    def configure(d, stage):                          # stage 0: as created; 1: the grid allocated anew; 2: another basis
        if stage >= 1:
            d.set_memory_budget(1 << 30)              # (room for one window and for every buffer of the three calls)
        d.set_controls(ctrl2 if stage == 2 else ctrl); d.set_target(target)
        assert d.memory_plan()["windows"] == 1

    dp = qgd.DeviceProblem(prob, order)
    try:
        for stage in range(3):
            if stage != 2:                            # (stage 2 keeps the grid of stage 1)
                configure(dp, stage)
            else:
                dp.set_controls(ctrl2)
            args = (pcof2, V2) if stage == 2 else (pcof, V)
            got = _sensitivities(dp, *args)
            fresh = qgd.DeviceProblem(prob, order)
            try:
                configure(fresh, stage)
                ref = _sensitivities(fresh, *args)
            finally:
                fresh.close()
            for i, (a, b) in enumerate(zip(got, ref)):
                assert np.array_equal(a, b), (stage, i)
    finally:
        dp.close()


@pytest.mark.parametrize("entry", ["eval_hessian", "eval_hessian_vec"])
def test_memory_refusal_reports_the_deciding_byte_count(qgd, entry):
    """cnot3, 20 steps, order 8 (8 initial conditions).  The precondition need > window_bytes holds at this shape for both
    entry points (asserted below): nothing had to be raised."""
    L = qgd._lib
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=20, tf=20.0)
    v = np.random.default_rng(3).standard_normal(len(pcof))

    def call(d):
        return d.eval_hessian(pcof) if entry == "eval_hessian" else d.eval_hessian_vec(pcof, v)

    def run(budget):                                  # (result, None), or (None, the bytes the QGD_ERR_MEMORY refusal names)
        d = qgd.DeviceProblem(prob, 8)
        try:
            window = d.memory_plan()["window_bytes"]
            if budget is not None:
                d.set_memory_budget(window if budget == "window" else budget)
            d.set_controls(ctrl); d.set_target(target)
            assert d.memory_plan()["windows"] == 1
            try:
                return call(d), None, window
            except L.QGDError as e:
                assert e.code == L.QGD_ERR_MEMORY
                return None, int(re.search(r"\((\d+) bytes needed\)", d.lib.qgd_last_error(d.h).decode()).group(1)), window
        finally:
            d.close()

    out, need, window = run("window")
    assert out is None and need is not None
    print(f"{entry}: {need} bytes needed, window {window} bytes")
    assert need > window                              # (else a budget of `need` would not keep the grid in one window)
    ref, _, _ = run(None)
    out, refused, _ = run(need)
    assert refused is None and np.array_equal(out, ref)
    out, refused, _ = run(need - 1)
    assert out is None and refused == need
