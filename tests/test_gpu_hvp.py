"""GPU tests of the exact Hessian-vector product (qgd_eval_hessian_vec): against the numpy statement of
the full Hessian times the vector, against differences of the device gradient for every cost type, against qgd_eval_hessian on
cnot3, reproducibility, the kept setup and its invalidation, interleaving with the other entry points, the memory budget the
full Hessian does not fit, and the refusals.

Bound against the numpy statement: max|hv - H0 v| <= 1e-11 max|H0| |v|_1 (the per-entry 1e-11 max|H0| of
test_gpu_hessian.py carried through a matrix-vector product); the measured figures are in DESIGN.md section 4d."""
import itertools
import re

import numpy as np
import pytest

import cases
import proto_hessian as ph
from test_gpu_hessian import _case, _handle

pytestmark = pytest.mark.gpu


def _paths(qgd, dp):
    for path in ("dense", "sparse"):
        try:
            dp.set_operator_path(path)
        except qgd._lib.QGDError:
            continue                         # (the problem does not qualify for this operator path)
        yield path


@pytest.mark.parametrize("name,order", [("cnot2", 2), ("cnot2", 4), ("cnot2", 8), ("guarded", 6), ("dense_guard", 6)])
def test_hvp_matches_numpy_statement(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    H0 = ph.hessian(prob, Gp, Gq, off, pcof, target, order)
    sc = np.abs(H0).max()
    n = len(pcof)
    unit = np.zeros(n); unit[n // 3] = 1.0
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        g_adj, _ = dp.discrete_adjoint(pcof)
        for path in _paths(qgd, dp):
            for label, v in (("random", np.random.default_rng(11).standard_normal(n)), ("unit", unit)):
                grad = np.zeros(n)
                hv = dp.eval_hessian_vec(pcof, v, grad=grad)
                err, bound = np.abs(hv - H0 @ v).max(), 1e-11 * sc * np.abs(v).sum()
                print(f"{name} order {order} {path} {label}: max|hv - H0 v| = {err:.3e}, bound {bound:.3e}")
                assert err <= bound, (path, label)
                assert np.abs(grad - g_adj).max() <= 1e-12 * max(1.0, np.abs(g_adj).max())
            assert np.all(dp.eval_hessian_vec(pcof, np.zeros(n)) == 0.0)
    finally:
        dp.close()


@pytest.mark.parametrize("name", ["rand4", "guarded", "dense_guard"])
@pytest.mark.parametrize("cost_type", ["Tracking", "Norm", "Infidelity"])
def test_hvp_matches_gradient_differences(qgd, name, cost_type):
    order = 4
    prob, ctrl, pcof, target = _case(qgd, name)
    dp = _handle(qgd, prob, ctrl, target, order, cost_type)
    try:
        rng = np.random.default_rng(5)
        for _ in range(2):
            v = rng.standard_normal(len(pcof)); v /= np.linalg.norm(v)
            hv = dp.eval_hessian_vec(pcof, v)

            def fd(h):
                return (dp.discrete_adjoint(pcof + h * v)[0] - dp.discrete_adjoint(pcof - h * v)[0]) / (2 * h)
            F = (4 * fd(5e-4) - fd(1e-3)) / 3
            err = np.abs(hv - F).max()
            print(f"{name} {cost_type}: max|hv - fd| = {err:.3e}, max|fd| = {np.abs(F).max():.3e}")
            assert err <= 1e-8 * np.abs(F).max()
    finally:
        dp.close()


@pytest.mark.parametrize("nsteps", [20, 550])
def test_hvp_cnot3_against_hessian(qgd, nsteps):
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=nsteps, tf=float(nsteps))
    dp = _handle(qgd, prob, ctrl, target, 8)
    try:
        H = dp.eval_hessian(pcof)
        sc = np.abs(H).max()
        rng = np.random.default_rng(7)
        for _ in range(3):
            v = rng.standard_normal(len(pcof)); v /= np.linalg.norm(v)
            hv = dp.eval_hessian_vec(pcof, v)
            err, bound = np.abs(hv - H @ v).max(), 1e-11 * sc * np.abs(v).sum()
            print(f"cnot3 {nsteps} steps: max|hv - H v| = {err:.3e}, bound {bound:.3e}")
            assert err <= bound

            def dd(h):
                return v @ (dp.discrete_adjoint(pcof + h * v)[0] - dp.discrete_adjoint(pcof - h * v)[0]) / (2 * h)
            ref = (4 * dd(5e-4) - dd(1e-3)) / 3
            assert abs(v @ hv - ref) <= 1e-7 * sc
    finally:
        dp.close()


@pytest.mark.parametrize("name,order", [("cnot2", 4), ("guarded", 6), ("dense_guard", 6)])
def test_hvp_batches_and_reproducibility(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    n = len(pcof)
    V = np.random.default_rng(2).standard_normal((n, 3))
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        for path in _paths(qgd, dp):
            HV = dp.eval_hessian_vec(pcof, V)
            assert HV.shape == (n, 3)
            for j in range(3):
                assert np.array_equal(HV[:, j], dp.eval_hessian_vec(pcof, V[:, j])), (path, j)
            assert np.array_equal(HV, dp.eval_hessian_vec(pcof, V))
        fresh = _handle(qgd, prob, ctrl, target, order)
        try:
            dp.set_operator_path("auto")
            assert np.array_equal(dp.eval_hessian_vec(pcof, V), fresh.eval_hessian_vec(pcof, V))      # a second handle, a cold setup
        finally:
            fresh.close()
    finally:
        dp.close()


_FORWARD_PHASES = ("tables", "build_LR", "inverse", "propagator", "sweep_forward", "sweep_forward2", "front")
_SETUP_PHASES = _FORWARD_PHASES + ("hess_basis", "hess_terms", "forced_basis", "derivs")


def _phases(dp, *args):
    dp.set_timing(1)
    out = dp.eval_hessian_vec(*args)
    names = set(dp.timings())
    dp.set_timing(0)
    return out, names


def test_hvp_setup_is_kept_and_invalidated(qgd):
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    order, n = 6, len(pcof)
    rng = np.random.default_rng(9)
    v1, v2 = rng.standard_normal(n), rng.standard_normal(n)
    pcof2 = pcof * 1.01
    target2 = np.array(target, dtype=complex) * np.exp(0.3j)
    target2[0, 0] *= 0.5
    ctrl2 = [qgd.CarrierControl(qgd.FortranBSplineControl(2, 8, prob.tf), [0.0, -1.0]) for _ in range(2)]

    def fresh(ctrl_=ctrl, target_=target, cost="Infidelity", p=pcof, v=v2):
        f = _handle(qgd, prob, ctrl_, target_, order, cost)
        try:
            return f.eval_hessian_vec(p, v)
        finally:
            f.close()

    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        _, first = _phases(dp, pcof, v1)
        assert "hess_basis" in first and "sweep_forward" in first and "hvp_forcing" in first
        hv2, warm = _phases(dp, pcof, v2)
        assert not (warm & set(_SETUP_PHASES)), warm
        assert "hvp_forcing" in warm and "hvp_adjoint" in warm
        assert np.array_equal(hv2, fresh())
        hv3, other = _phases(dp, pcof2, v2)
        assert "hess_basis" in other and "sweep_forward" in other
        assert np.array_equal(hv3, fresh(p=pcof2))
        # setters in between: the result of a fresh handle, the setup run again
        dp.eval_hessian_vec(pcof, v1)
        dp.set_target(target2)
        hv, names = _phases(dp, pcof, v2)
        assert "hess_basis" in names
        assert np.array_equal(hv, fresh(target_=target2))
        dp.set_cost_type("Tracking")
        hv, names = _phases(dp, pcof, v2)
        assert "hess_basis" in names
        assert np.array_equal(hv, fresh(target_=target2, cost="Tracking"))
        dp.set_cost_type("Infidelity")
        dp.eval_hessian_vec(pcof, v1)
        dp.set_controls(ctrl2)
        hv, names = _phases(dp, pcof, v2)
        assert "hess_basis" in names and "sweep_forward" in names
        assert np.array_equal(hv, fresh(ctrl_=ctrl2, target_=target2))
    finally:
        dp.close()


@pytest.mark.parametrize("name,order", [("cnot2", 4), ("guarded", 6)])
def test_hvp_interleaves_with_other_entry_points(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    n = len(pcof)
    v = np.random.default_rng(4).standard_normal(n)
    calls = {
        "hessian": lambda d: d.eval_hessian(pcof),
        "adjoint": lambda d: d.discrete_adjoint(pcof, history_precomputed=1)[0],
        "hvp": lambda d: d.eval_hessian_vec(pcof, v),
        "forced": lambda d: d.eval_grad_forced(pcof),
    }
    alone = {}
    for key, fn in calls.items():
        d = _handle(qgd, prob, ctrl, target, order)
        try:
            d.eval_forward(pcof)                     # (history_precomputed needs a forward evaluation behind it)
            alone[key] = fn(d)
        finally:
            d.close()
    for perm in itertools.permutations(calls):
        d = _handle(qgd, prob, ctrl, target, order)
        try:
            d.eval_forward(pcof)
            for rep in range(2):
                for key in perm:
                    assert np.array_equal(calls[key](d), alone[key]), (perm, rep, key)
        finally:
            d.close()


def test_hvp_fits_where_the_hessian_does_not(qgd):
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=550, tf=550.0)
    v = np.random.default_rng(3).standard_normal(len(pcof))
    dp = _handle(qgd, prob, ctrl, target, 8)
    try:
        ref = dp.eval_hessian_vec(pcof, v)
        grid = dp.memory_plan()["window_bytes"]
        # what the full Hessian allocates, from its own refusal under a budget that holds the grid and nothing else
        dp.set_memory_budget(grid)
        dp.set_controls(ctrl); dp.set_target(target)
        assert dp.memory_plan()["windows"] == 1
        with pytest.raises(qgd._lib.QGDError) as ei:
            dp.eval_hessian(pcof)
        assert ei.value.code == qgd._lib.QGD_ERR_MEMORY
        need = int(re.search(r"\((\d+) bytes needed\)", dp.lib.qgd_last_error(dp.h).decode()).group(1))
        # section 4c: the sensitivity history alone is nt N 2 n_pcof c doubles (the padded panels take at least that)
        shist = (prob.nsteps + 1) * prob.N_tot_levels * 2 * len(pcof) * prob.N_initial_conditions * 8
        assert need > shist
        budget = max(grid, need - shist)              # room for everything the Hessian needs except its sensitivity history
        assert budget < need
        dp.set_memory_budget(budget)
        dp.set_controls(ctrl); dp.set_target(target)
        assert dp.memory_plan()["windows"] == 1
        with pytest.raises(qgd._lib.QGDError) as ei:
            dp.eval_hessian(pcof)
        assert ei.value.code == qgd._lib.QGD_ERR_MEMORY
        hv = dp.eval_hessian_vec(pcof, v)
        assert np.array_equal(hv, ref)
    finally:
        dp.close()


def _refused(qgd, dp, pcof, v, code):
    with pytest.raises(qgd._lib.QGDError) as ei:
        dp.eval_hessian_vec(pcof, v)
    assert ei.value.code == code


def test_hvp_refusals(qgd):
    L = qgd._lib
    # a windowed grid
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=100, tf=100.0)
    dp = qgd.DeviceProblem(prob, 4)
    dp.set_memory_budget(dp.memory_plan()["window_bytes"] // 3)
    dp.set_controls(ctrl); dp.set_target(target)
    try:
        assert dp.memory_plan()["windows"] > 1
        g0 = dp.discrete_adjoint(pcof)[0]
        _refused(qgd, dp, pcof, np.ones(len(pcof)), L.QGD_ERR_UNSUPPORTED)
        assert np.array_equal(dp.discrete_adjoint(pcof)[0], g0)
    finally:
        dp.close()
    # N > 64
    prob, ctrl, pcof, target = cases.synthetic_case(qgd, nsteps=4)
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        g0 = dp.discrete_adjoint(pcof)[0]
        _refused(qgd, dp, pcof, np.ones(len(pcof)), L.QGD_ERR_UNSUPPORTED)
        assert np.array_equal(dp.discrete_adjoint(pcof)[0], g0)
    finally:
        dp.close()
    # more than 64 basis directions: 5 operators at order 16 (80)
    prob = qgd.construct_rand_prob(4, 5, tf=1.0, nsteps=6)
    ctrl = [qgd.FortranBSplineControl(16, 20, prob.tf) for _ in range(5)]
    pcof = np.random.default_rng(1).random(qgd.get_number_of_control_parameters(ctrl))
    dp = _handle(qgd, prob, ctrl, cases.rand_target(prob), 16)
    try:
        _refused(qgd, dp, pcof, np.ones(len(pcof)), L.QGD_ERR_UNSUPPORTED)
    finally:
        dp.close()
    # a partitioned handle
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=12, tf=12.0)
    rank = qgd.DeviceBackend(prob, 4, ctrl, target, 0, 2)      # rank 0 of a two-way time partition, controls and target set
    dp = rank.dp
    try:
        _refused(qgd, dp, pcof, np.ones(len(pcof)), L.QGD_ERR_STATE)
        assert "partitioned" in dp.lib.qgd_last_error(dp.h).decode()
    finally:
        dp.close()
    # no target, no control basis
    dp = qgd.DeviceProblem(prob, 4)
    try:
        dp.set_controls(ctrl)
        _refused(qgd, dp, pcof, np.ones(len(pcof)), L.QGD_ERR_STATE)
    finally:
        dp.close()
    dp = qgd.DeviceProblem(prob, 4)
    try:
        dp.set_target(target)
        _refused(qgd, dp, pcof, np.ones(len(pcof)), L.QGD_ERR_STATE)
    finally:
        dp.close()
    # a control that is not linear in its coefficients
    rabi = qgd.construct_rabi_prob(tf=np.pi, nsteps=10)
    sc = cases.SineControl(rabi.tf)
    with pytest.raises(NotImplementedError, match="linear"):
        qgd.eval_hessian_vec(rabi, sc, np.array([0.3, 1.1, 0.2]), np.ones(3), cases.rand_target(rabi), order=4)
    # arguments: the C ABI's own checks (NULL pcof, NULL v / hv, n_vec < 1, a pcof of another length)
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        n = len(pcof)
        g0 = dp.discrete_adjoint(pcof)[0]
        p = np.ascontiguousarray(pcof); v = np.ones(n); hv = np.zeros(n)
        f = dp.lib.qgd_eval_hessian_vec
        assert f(dp.h, None, n, v.ctypes.data, 1, hv.ctypes.data, None) == L.QGD_ERR_UNSUPPORTED
        assert f(dp.h, p.ctypes.data, n, None, 1, hv.ctypes.data, None) == L.QGD_ERR_ARGUMENT
        assert f(dp.h, p.ctypes.data, n, v.ctypes.data, 1, None, None) == L.QGD_ERR_ARGUMENT
        assert f(dp.h, p.ctypes.data, n, v.ctypes.data, 0, hv.ctypes.data, None) == L.QGD_ERR_ARGUMENT
        assert f(dp.h, p.ctypes.data, n - 1, v.ctypes.data, 1, hv.ctypes.data, None) == L.QGD_ERR_ARGUMENT
        with pytest.raises(ValueError):
            dp.eval_hessian_vec(pcof, np.ones(n - 1))
        # the handle still works after the refusals
        assert np.array_equal(dp.discrete_adjoint(pcof)[0], g0)
    finally:
        dp.close()


def test_hvp_module_level(qgd):
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=12, tf=12.0)
    V = np.random.default_rng(8).standard_normal((len(pcof), 2))
    H = qgd.eval_hessian(prob, ctrl, pcof, target, order=4)
    HV = qgd.eval_hessian_vec(prob, ctrl, pcof, V, target, order=4)
    assert np.abs(HV - H @ V).max() <= 1e-11 * np.abs(H).max() * np.abs(V).sum(axis=0).max()
