"""GPU tests of cost_type :StateTransfer: J = 1 - (1/c) sum_j |t_j^H psi_j|^2, one overlap per column
where :Infidelity has one global one.  Every evaluation path that forms a terminal condition is compared with routes that do
not share the new kernels' code: the host arithmetic on the device's states (proto_state_transfer.py), eval_pullback with the
host's dJ/dw_N as cotangent, the forced gradient (host terminal part), centred differences.

Bounds (the project's own): two formulations of a gradient 1e-10 max(1, max|ref|) (test_gpu_pullback._bound); a scalar against
host arithmetic 1e-11 max(1, J) (parity tests); centred differences 1e-8 max(1, scale) (test_cost_types_vs_oracle); small path
against general path 1e-12 (include/qgd.h); front against general path and windows / partition against the resident handle
1e-12 max|g| and 1e-12 on the scalars (test_front_cost_types, test_time_partitioned_matches_single_gpu); Hessian against
Richardson-extrapolated differences of the gradient 1e-8 max|F|, symmetry 1e-13 max|H|
(test_hessian_matches_gradient_differences); Hessian-vector product against H v 1e-11 max|H| sum|v|
(test_hvp_cnot3_against_hessian)."""
import ctypes as C

import numpy as np
import pytest

import cases
import proto_state_transfer as pst
from test_gpu_pullback import _bound, _guard_bar

pytestmark = pytest.mark.gpu

ST = "StateTransfer"


def _unit_columns(rng, N, c):
    t = rng.standard_normal((N, c)) + 1j * rng.standard_normal((N, c))
    return t / np.linalg.norm(t, axis=0)[None, :]


def _rand_case(qgd, N, c, nsteps=5, n_ops=2, seed=0):
    """a random dense problem with c of its N columns, short B-spline controls (n_pcof = 2 * 2 * 6 = 24) and unit target columns"""
    prob = qgd.construct_rand_prob(N, n_ops, tf=0.5, nsteps=nsteps, gmres_abstol=1e-15, gmres_reltol=1e-15, scale=1.0 / N)
    prob.u0 = np.asfortranarray(prob.u0[:, :c]); prob.v0 = np.asfortranarray(prob.v0[:, :c]); prob.N_initial_conditions = c
    ctrl = [qgd.FortranBSplineControl(3, 6, prob.tf) for _ in range(n_ops)]
    rng = np.random.default_rng(1000 * N + c + seed)
    pcof = rng.standard_normal(qgd.get_number_of_control_parameters(ctrl))
    return prob, ctrl, pcof, _unit_columns(rng, N, c)


def _case(qgd, name):
    if name == "two_qubit":
        return cases.cnot2_case(qgd) + (4,)
    if name == "guarded":
        return cases.guarded_case(qgd, nsteps=20) + (6,)
    if name == "dense_guard":
        return cases.dense_guard_case(qgd) + (6,)
    if name == "rand12x12":                            # two column groups, the second half full
        return _rand_case(qgd, 12, 12) + (4,)
    if name == "rand21x20":                            # cp = 24: 2 cp = 48 does not divide the workgroup size
        return _rand_case(qgd, 21, 20) + (4,)
    assert name == "three_qubit"
    return cases.cnot3_case(qgd, nsteps=12) + (8,)


def _handle(qgd, prob, ctrl, target, order, cost_type=ST, small=False):
    dp = qgd.DeviceProblem(prob, order)
    dp.set_small_path(small)
    dp.set_controls(ctrl); dp.set_target(target); dp.set_cost_type(cost_type)
    return dp


def _close(got, ref, bound, what):
    err = np.abs(np.asarray(got) - np.asarray(ref)).max()
    print(f"\n{what}: max error {err:.3e}, bound {bound:.3e}")
    assert np.all(np.isfinite(got)), what
    assert err <= bound, what


def _host_cost(dp, pcof, target):
    w = dp.eval_states(pcof)
    return pst.cost(w[:, -1], target), w


def _directional(dp, pcof, d, h=1e-4):
    """Richardson-extrapolated centred difference of the objective eval_forward returns, along d"""
    def J(p):
        o = dp.eval_forward(p)
        return o[0] + o[2]

    def dd(s):
        return (J(pcof + s * d) - J(pcof - s * d)) / (2 * s)
    return (4 * dd(h) - dd(2 * h)) / 3


# -- 1: cost and gradient against independent routes ------------------------------------------------------------------------

def _independent_routes(qgd, name, terminal, monkeypatch):
    if terminal == "kernel":
        monkeypatch.setenv("QGD_PATHS", "terminal_kernel")
    prob, ctrl, pcof, target, order = _case(qgd, name)
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        g, o3 = dp.discrete_adjoint(pcof)
        assert not dp.small_path_taken()
        J, w = _host_cost(dp, pcof, target)
        _close(o3[0], J, 1e-11 * max(1.0, J), f"{name} {terminal}: out3[0] vs host cost of eval_states")
        assert o3[1] == 0.0
        assert np.array_equal(np.asarray(dp.eval_forward(pcof)), np.asarray(o3))
        sb = _guard_bar(prob, w)
        sb[:, -1] += pst.cost_bar(w[:, -1], target)
        _close(g, dp.eval_pullback(pcof, states_bar=sb), _bound(g), f"{name} {terminal}: gradient vs eval_pullback of the host's dJ/dw_N")
        _close(g, dp.eval_grad_forced(pcof), _bound(g), f"{name} {terminal}: gradient vs eval_grad_forced")
        g2, o32 = dp.discrete_adjoint(pcof)
        assert np.array_equal(g, g2) and np.array_equal(o3, o32)
    finally:
        dp.close()
    if len(pcof) <= 50:
        g_fd = qgd.eval_grad_finite_difference(prob, ctrl, pcof, target, order=order, cost_type=ST)
        _close(g, g_fd, 1e-8 * max(1.0, np.abs(g).max()), f"{name} {terminal}: gradient vs eval_grad_finite_difference")
        qgd.clear_cache()


@pytest.mark.parametrize("terminal", ["fused", "kernel"])
@pytest.mark.parametrize("name", ["guarded", "dense_guard", "rand12x12", "rand21x20", "three_qubit"])
def test_cost_and_gradient_against_independent_routes(qgd, monkeypatch, name, terminal):
    _independent_routes(qgd, name, terminal, monkeypatch)


@pytest.mark.parametrize("terminal", ["fused", "kernel"])
def test_cost_and_gradient_cnot2_general_path(qgd, monkeypatch, terminal):
    _independent_routes(qgd, "two_qubit", terminal, monkeypatch)


# -- 2: the small-problem path ----------------------------------------------------------------------------------------------

def _tiny_shape(qgd, N, c, n_ops, order, nsteps):
    """the problems of test_gpu_tiny.py::test_shapes_guards_and_cost_types"""
    prob = qgd.construct_rand_prob(N, n_ops, tf=1.0, nsteps=nsteps, gmres_abstol=1e-15, gmres_reltol=1e-15, scale=0.7)
    prob.u0 = np.asfortranarray(prob.u0[:, :c]); prob.v0 = np.asfortranarray(prob.v0[:, :c]); prob.N_initial_conditions = c
    rng = np.random.default_rng(N * 100 + c)
    W = np.zeros((2 * N, 2 * N))
    wd = rng.random(N) * (rng.random(N) > 0.4)
    W[np.arange(N), np.arange(N)] = wd; W[N + np.arange(N), N + np.arange(N)] = wd
    prob.guard_subspace_projector = W
    ctrl = [qgd.FortranBSplineControl(3, 5, prob.tf) for _ in range(n_ops)]
    pcof = rng.standard_normal(qgd.get_number_of_control_parameters(ctrl))
    return prob, ctrl, pcof, cases.rand_target(prob)


@pytest.mark.parametrize("shape", ["cnot2", (3, 2, 1, 4, 25), (4, 4, 2, 6, 40), (2, 2, 4, 2, 100)])
def test_small_path_against_general_path(qgd, shape):
    if shape == "cnot2":
        prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=6, tf=6.0)
        order = 4
    else:
        prob, ctrl, pcof, target = _tiny_shape(qgd, *shape)
        order = shape[3]
    gen, tiny = _handle(qgd, prob, ctrl, target, order), _handle(qgd, prob, ctrl, target, order, small=True)
    try:
        g0, o0 = gen.discrete_adjoint(pcof)
        g1, o1 = tiny.discrete_adjoint(pcof)
        assert tiny.small_path_taken() and not gen.small_path_taken()
        _close(o1, o0, 1e-12, f"{shape}: scalars, small path vs general path")
        _close(g1, g0, 1e-12 * max(np.abs(g0).max(), 1e-2), f"{shape}: gradient, small path vs general path")
        f1 = tiny.eval_forward(pcof)
        assert tiny.small_path_taken() and np.array_equal(np.asarray(f1), np.asarray(o1))
        J, _ = _host_cost(gen, pcof, target)
        _close(o1[0], J, 1e-11 * max(1.0, J), f"{shape}: small path's cost vs host cost")
    finally:
        gen.close(); tiny.close()


# -- 3: batches --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["side_by_side", "loop"])
def test_batch_equals_single_calls(qgd, route):
    if route == "side_by_side":
        prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=6, tf=6.0)
        order = 4
    else:
        prob, ctrl, pcof, target = cases.guarded_case(qgd, nsteps=10, tf=5.0)
        order = 6
    rng = np.random.default_rng(5)
    P = np.stack([pcof * (1.0 + 0.3 * rng.standard_normal(len(pcof))) for _ in range(5)])
    dp = _handle(qgd, prob, ctrl, target, order, small=(route == "side_by_side"))
    try:
        G, S, status = dp.eval_batch(P)
        assert dp.batch_path_taken() == (route == "side_by_side") and not status.any()
        for k in range(5):
            g, o = dp.discrete_adjoint(P[k])
            assert np.array_equal(G[k], g) and np.array_equal(S[k], o), (route, k)
        _, S2, _ = dp.eval_batch(P, gradient=False)
        assert np.array_equal(S2, S)
    finally:
        dp.close()


# -- 4: the fused front ------------------------------------------------------------------------------------------------------

def test_front_against_general_path(qgd, monkeypatch):
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=550, tf=550.0)
    dp = _handle(qgd, prob, ctrl, target, 8)
    try:
        g, o = dp.discrete_adjoint(pcof)
        assert dp.front_path_taken()
        g2, o2 = dp.discrete_adjoint(pcof)
        assert np.array_equal(g, g2) and np.array_equal(o, o2)
    finally:
        dp.close()
    monkeypatch.setenv("QGD_PATHS", "no_front")
    dn = _handle(qgd, prob, ctrl, target, 8)
    try:
        gn, on = dn.discrete_adjoint(pcof)
        assert not dn.front_path_taken()
    finally:
        dn.close()
    _close(g, gn, 1e-12 * np.abs(gn).max(), "cnot3 550 steps: gradient, front vs general path")
    _close(o, on, 1e-12, "cnot3 550 steps: scalars, front vs general path")


# -- 5: N > 64 ---------------------------------------------------------------------------------------------------------------

def test_large_n_kernels(qgd):
    prob, ctrl, pcof, target = cases.synthetic_case(qgd, N=72, c=4, n_ops=2, nsteps=6, tf=0.3, seed=72)
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        g, o3 = dp.discrete_adjoint(pcof)
        assert dp.intermediate("selection")[0] == 1.0
        J, _ = _host_cost(dp, pcof, target)
        _close(o3[0], J, 1e-11 * max(1.0, J), "N = 72: out3[0] vs host cost")
        _close(g, dp.eval_grad_forced(pcof), _bound(g), "N = 72: gradient vs eval_grad_forced")
        rng = np.random.default_rng(72)
        for k in range(3):
            d = rng.standard_normal(len(pcof)); d /= np.linalg.norm(d)
            _close(g @ d, _directional(dp, pcof, d), 1e-8 * max(1.0, np.abs(g).max()), f"N = 72: directional derivative {k}")
    finally:
        dp.close()


def test_two_launch_terminal(qgd):
    """N = 72 (80 padded rows) and 208 columns: panels of 80 * 416 = 33280 >= 32768 elements take k_terminal_cols_sum +
    k_terminal_y, with two row blocks per column group to add in the last-ticket workgroup"""
    N, c = 72, 208
    prob = qgd.construct_rand_prob(N, 2, tf=0.1, nsteps=2, scale=1.0 / N)
    rng = np.random.default_rng(208)
    psi0 = _unit_columns(rng, N, c)
    prob.u0 = np.asfortranarray(psi0.real); prob.v0 = np.asfortranarray(psi0.imag); prob.N_initial_conditions = c
    ctrl = [qgd.FortranBSplineControl(3, 6, prob.tf) for _ in range(2)]
    pcof = rng.standard_normal(qgd.get_number_of_control_parameters(ctrl))
    target = _unit_columns(rng, N, c)
    dp = _handle(qgd, prob, ctrl, target, 2)
    try:
        assert ((N + 15) // 16 * 16) * 2 * ((c + 7) // 8 * 8) >= 32768
        g, o3 = dp.discrete_adjoint(pcof)
        J, w = _host_cost(dp, pcof, target)
        _close(o3[0], J, 1e-11 * max(1.0, J), "c = 208: out3[0] vs host cost")
        a, b = pst.overlaps(w[:, -1], target)
        _close(dp.column_overlaps(), a - 1j * b, 1e-12, "c = 208: column_overlaps vs host overlaps")
        for k in range(2):
            d = rng.standard_normal(len(pcof)); d /= np.linalg.norm(d)
            _close(g @ d, _directional(dp, pcof, d), 1e-8 * max(1.0, np.abs(g).max()), f"c = 208: directional derivative {k}")
        g2, o32 = dp.discrete_adjoint(pcof)
        assert np.array_equal(g, g2) and np.array_equal(o3, o32)
    finally:
        dp.close()


# -- 6: windowed grids and a time partition ------------------------------------------------------------------------------------

def test_windows_and_time_partition(qgd):
    import torch
    prob, ctrl, pcof, target = cases.guarded_case(qgd, nsteps=30)
    order = 6
    dp = _handle(qgd, prob, ctrl, target, order)
    g_ref, o_ref = dp.discrete_adjoint(pcof)
    dp.close()
    dw = qgd.DeviceProblem(prob, order)
    dw.set_memory_budget(dw.memory_plan()["window_bytes"] // 3)
    dw.set_controls(ctrl); dw.set_target(target); dw.set_cost_type(ST)
    try:
        assert dw.memory_plan()["windows"] >= 2
        g, o = dw.discrete_adjoint(pcof)
        _close(g, g_ref, 1e-12 * np.abs(g_ref).max(), "windowed grid: gradient vs resident handle")
        _close(o, o_ref, 1e-12, "windowed grid: scalars vs resident handle")
        _close(dw.eval_grad_forced(pcof), g_ref, _bound(g_ref), "windowed grid: forced gradient")
        with pytest.raises(qgd._lib.QGDError) as ei:
            dw.column_overlaps()
        assert ei.value.code == qgd._lib.QGD_ERR_UNSUPPORTED
    finally:
        dw.close()
    stream = torch.cuda.current_stream().cuda_stream
    backs = [qgd.DeviceBackend(prob, order, ctrl, target, r, 2, device=0, stream=stream) for r in range(2)]
    try:
        for b in backs:
            b.set_cost_type(ST)
        for g, o in qgd.LocalGroup(backs).discrete_adjoint(pcof):
            _close(g, g_ref, 1e-12 * np.abs(g_ref).max(), "time partition: gradient vs single handle")
            _close(o, o_ref, 1e-12, "time partition: scalars vs single handle")
        with pytest.raises(qgd._lib.QGDError) as ei:
            backs[1].dp.column_overlaps()
        assert ei.value.code == qgd._lib.QGD_ERR_UNSUPPORTED
    finally:
        for b in backs:
            b.close()


# -- 7: Hessian and Hessian-vector products -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,order", [("cnot2", 4), ("guarded", 6)])
def test_hessian_and_hvp(qgd, name, order):
    if name == "cnot2":
        prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=12, tf=12.0)
    else:
        prob, ctrl, pcof, target = cases.guarded_case(qgd, nsteps=10, tf=5.0)
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        n = len(pcof)
        grad = np.zeros(n)
        H = dp.eval_hessian(pcof, grad=grad)
        _close(grad, dp.discrete_adjoint(pcof)[0], _bound(grad), f"{name}: the Hessian call's forced gradient vs discrete_adjoint")

        def fd(h):
            F = np.zeros((n, n))
            for l in range(n):
                e = np.zeros(n); e[l] = h
                F[:, l] = (dp.discrete_adjoint(pcof + e)[0] - dp.discrete_adjoint(pcof - e)[0]) / (2 * h)
            return F
        F = (4 * fd(5e-4) - fd(1e-3)) / 3
        _close(H, F, 1e-8 * np.abs(F).max(), f"{name}: Hessian vs differences of the gradient")
        _close(H, H.T, 1e-13 * np.abs(H).max(), f"{name}: symmetry")
        rng = np.random.default_rng(7)
        for _ in range(2):
            v = rng.standard_normal(n); v /= np.linalg.norm(v)
            _close(dp.eval_hessian_vec(pcof, v), H @ v, 1e-11 * np.abs(H).max() * np.abs(v).sum(), f"{name}: eval_hessian_vec vs H v")
    finally:
        dp.close()


# -- 8: what distinguishes it ---------------------------------------------------------------------------------------------------

def test_column_phases_and_the_one_column_limit(qgd):
    prob, ctrl, pcof, target = cases.guarded_case(qgd, nsteps=20)
    rng = np.random.default_rng(8)
    ph = np.exp(2j * np.pi * rng.random(target.shape[1]))
    t2 = target * ph[None, :]
    dp = _handle(qgd, prob, ctrl, target, 6)
    try:
        g, o = dp.discrete_adjoint(pcof)
        dp.set_target(t2)
        g2, o2 = dp.discrete_adjoint(pcof)
        _close(o2[0], o[0], 1e-12 * max(1.0, abs(o[0])), "column phases: cost")
        _close(g2, g, 1e-12 * max(1.0, np.abs(g).max()), "column phases: gradient")
        dp.set_cost_type("Infidelity")
        gi2, oi2 = dp.discrete_adjoint(pcof)
        dp.set_target(target)
        gi, oi = dp.discrete_adjoint(pcof)
        ness = prob.N_ess_levels
        f = lambda s: 1.0 - (s[0] ** 2 + s[1] ** 2) / ness ** 2
        assert abs(f(oi2) - f(oi)) > 1e-3 and np.abs(gi2 - gi).max() > 1e-3 * np.abs(gi).max()
    finally:
        dp.close()
    # one column, N_ess_levels = 1: the two functionals coincide
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=12, tf=12.0)
    one = prob.copy()
    one.u0 = np.asfortranarray(prob.u0[:, 1:2]); one.v0 = np.asfortranarray(prob.v0[:, 1:2])
    one.N_initial_conditions = 1; one.N_ess_levels = 1
    t1 = target[:, 1:2]
    ds, di = _handle(qgd, one, ctrl, t1, 4), _handle(qgd, one, ctrl, t1, 4, "Infidelity")
    try:
        gs, os_ = ds.discrete_adjoint(pcof)
        gi, oi = di.discrete_adjoint(pcof)
        Ji = 1.0 - (oi[0] ** 2 + oi[1] ** 2)
        _close(os_[0], Ji, 1e-13 * max(abs(Ji), 1.0), "one column: cost vs :Infidelity")
        _close(gs, gi, 1e-13 * np.abs(gi).max(), "one column: gradient vs :Infidelity")
    finally:
        ds.close(); di.close()


# -- 9: the stored sweep and the read-out ---------------------------------------------------------------------------------------

def test_stored_sweep_and_column_overlaps(qgd):
    L = qgd._lib
    prob, ctrl, pcof, target = cases.guarded_case(qgd, nsteps=20)
    fresh = _handle(qgd, prob, ctrl, target, 6)
    dp = _handle(qgd, prob, ctrl, target, 6, "Infidelity")
    try:
        g_new, o_new = fresh.discrete_adjoint(pcof)
        oi = dp.eval_forward(pcof)
        # the read-out works under :Infidelity: the overlaps add up to the global ones
        w = dp.eval_states(pcof)
        a, b = pst.overlaps(w[:, -1], target)
        ov = dp.column_overlaps()
        _close(ov, a - 1j * b, 1e-12, ":Infidelity: column_overlaps vs host overlaps")
        _close([ov.real.sum(), -ov.imag.sum()], [oi[0], oi[1]], 1e-12, ":Infidelity: sum of the column overlaps vs out3")
        dp.eval_forward(pcof)
        dp.set_cost_type(ST)
        g, o = dp.discrete_adjoint(pcof, history_precomputed=True)      # a new terminal condition on the stored sweep, or the sweep again
        assert np.array_equal(g, g_new) and np.array_equal(o, o_new)
        _close(dp.column_overlaps(), a - 1j * b, 1e-12, "column_overlaps vs host overlaps")
        _close(1.0 - dp.column_fidelities().mean(), o[0], 1e-12, "1 - mean(column_fidelities) vs out3[0]")
        # refusals: no stored sweep after a batch, none on a new handle, no target
        dp.eval_batch(np.stack([pcof, 0.5 * pcof]))
        with pytest.raises(L.QGDError) as ei:
            dp.column_overlaps()
        assert ei.value.code == L.QGD_ERR_STATE
        ns = _handle(qgd, prob, ctrl, target, 6)
        nt = qgd.DeviceProblem(prob, 6); nt.set_controls(ctrl)
        try:
            nt.eval_forward(pcof)
            for h in (ns, nt):
                with pytest.raises(L.QGDError) as ei:
                    h.column_overlaps()
                assert ei.value.code == L.QGD_ERR_STATE
        finally:
            ns.close(); nt.close()
    finally:
        fresh.close(); dp.close()
    # after a small-path evaluation the sweep is redone on the general path
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=6, tf=6.0)
    tiny = _handle(qgd, prob, ctrl, target, 4, small=True)
    try:
        g, o = tiny.discrete_adjoint(pcof)
        assert tiny.small_path_taken()
        _close(1.0 - tiny.column_fidelities().mean(), o[0], 1e-12, "small path: 1 - mean(column_fidelities) vs out3[0]")
        assert not tiny.small_path_taken()
    finally:
        tiny.close()


# -- 10: refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals(qgd):
    import torch
    L = qgd._lib
    prob, ctrl, pcof, target = cases.guarded_case(qgd, nsteps=10, tf=5.0)
    dp = _handle(qgd, prob, ctrl, target, 6)
    try:
        g, o = dp.discrete_adjoint(pcof)
        for bad in (4, -1):
            assert dp.lib.qgd_set_cost_type(dp.h, bad) == L.QGD_ERR_ARGUMENT
            g2, o2 = dp.discrete_adjoint(pcof)
            assert np.array_equal(g, g2) and np.array_equal(o, o2)      # still :StateTransfer
        with pytest.raises(ValueError, match="Invalid cost type"):
            dp.set_cost_type("Fidelity")
    finally:
        dp.close()
    stream = torch.cuda.current_stream().cuda_stream
    b = qgd.ColumnBackend(prob, 6, ctrl, target, 0, 1, device=0, stream=stream)
    try:
        g0, o0 = qgd.LocalGroup([b]).discrete_adjoint(pcof)[0]
        scal = b.exchange_buffer(3)[0]
        before = scal.cpu().numpy().copy()
        b.set_cost_type(ST)
        pc = np.ascontiguousarray(pcof)
        assert b.lib.qgd_cols_forward(b.h, pc.ctypes.data_as(C.c_void_p), len(pc)) == L.QGD_ERR_UNSUPPORTED
        assert b.lib.qgd_cols_adjoint(b.h, 1) == L.QGD_ERR_UNSUPPORTED
        with pytest.raises(L.QGDError) as ei:
            qgd.LocalGroup([b]).discrete_adjoint(pcof)
        assert ei.value.code == L.QGD_ERR_UNSUPPORTED
        assert np.array_equal(scal.cpu().numpy(), before)
        b.set_cost_type("Infidelity")
        g1, o1 = qgd.LocalGroup([b]).discrete_adjoint(pcof)[0]
        assert np.array_equal(g0, g1) and np.array_equal(o0, o1)
    finally:
        b.close()


def test_communicator_time_shards_run_and_column_shards_refuse(qgd):
    """The in-library collectives over an RCCL communicator of one rank (test_rccl_world1_reproduces_unpartitioned): a time
    shard evaluates the type, a column shard refuses it in front of the first collective and evaluates as before afterwards."""
    L = qgd._lib
    prob, ctrl, pcof, target = cases.guarded_case(qgd, nsteps=20)
    dp = _handle(qgd, prob, ctrl, target, 6)
    g_ref, o_ref = dp.discrete_adjoint(pcof)
    dp.close()
    ev = qgd.RcclEvaluation(prob, 6, ctrl, target, 0, 1, qgd.comm_unique_id(), shard="time")
    try:
        ev.set_cost_type(ST)
        g, o = ev.discrete_adjoint(pcof)
        _close(g, g_ref, 1e-12 * np.abs(g_ref).max(), "communicator, time shard: gradient vs single handle")
        _close(o, o_ref, 1e-12, "communicator, time shard: scalars vs single handle")
    finally:
        ev.close()
    ev = qgd.RcclEvaluation(prob, 6, ctrl, target, 0, 1, qgd.comm_unique_id(), shard="columns")
    try:
        g0, o0 = ev.discrete_adjoint(pcof)
        ev.set_cost_type(ST)
        for call in (lambda: ev.discrete_adjoint(pcof), lambda: ev.eval_forward(pcof)):
            with pytest.raises(L.QGDError) as ei:
                call()
            assert ei.value.code == L.QGD_ERR_UNSUPPORTED
        ev.set_cost_type("Infidelity")
        g1, o1 = ev.discrete_adjoint(pcof)
        assert np.array_equal(g0, g1) and np.array_equal(o0, o1)
    finally:
        ev.close()


# -- 11: the optimiser ----------------------------------------------------------------------------------------------------------

def test_optimize_gate_with_state_transfer(qgd):
    """The Rabi SWAP problem of test_optimize_gate_rabi_swap (optimization_rabi_osc_SWAP.jl:18-39).  |Omega| = 1/2 swaps the two
    levels up to a phase per column, so the per-column cost reaches 0 there as the infidelity does."""
    prob = qgd.construct_rabi_prob(tf=np.pi, nsteps=20)
    control = qgd.GRAPEControl(1, prob.tf)
    target = np.array([[0.0, 1.0], [1.0, 0.0]])
    p0 = np.array([0.4, 0.1])
    dp = _handle(qgd, prob, control, target, 8)
    try:
        o = dp.eval_forward(p0)
        start = o[0] + o[2]
    finally:
        dp.close()
    hist = qgd.optimize_gate(prob, control, p0, target, order=8, ridge_penalty_strength=0, cost_type=ST, maxIter=30, print_level=0)
    obj = np.asarray(hist.analytic_obj_value)
    print(f"\nRabi SWAP, StateTransfer: start {start:.3e}, history {obj}")
    assert np.all(np.diff(obj) <= 0.0) and obj[0] <= start
    assert obj[-1] <= start / 10
    assert np.array_equal(np.asarray(hist.infidelity) + np.asarray(hist.guard_penalty), obj)
    one = prob.copy()
    one.u0 = np.asfortranarray(prob.u0[:, :1]); one.v0 = np.asfortranarray(prob.v0[:, :1]); one.N_initial_conditions = 1
    h1 = qgd.optimize_gate(one, control, p0, target[:, :1], order=8, ridge_penalty_strength=0, cost_type=ST, maxIter=30, print_level=0)
    assert h1.analytic_obj_value[-1] < 1e-6      # (the bar of test_optimize_gate_rabi_swap)
    with pytest.raises(ValueError, match="Invalid cost type"):
        qgd.optimize_gate(prob, control, p0, target, order=8, cost_type="Fidelity", print_level=0)
    qgd.clear_cache()
