"""GPU tests of the device route of ensemble evaluation (qgd_set_ensemble / qgd_eval_ensemble, DeviceProblem.set_ensemble /
eval_ensemble, ``route=``): the members side by side in one device call, the weighted sums formed on the
device.  Everything is bitwise: a member's row is what a handle made for ``Ensemble.member_problem(prob, k)`` returns, and
``(grad, cost, guard)`` are ``ensemble_reduce`` of those rows.  Every test runs twice (tests/conftest.py): on the library's
defaults, where ``route="auto"`` must take the device, and with the small-problem path switched off on every handle
("general"), where the library refuses and ``auto`` falls back to the loop -- the same bits.  Every case is a few time points."""
import ctypes as C

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _member_rows(qgd, ens, prob, order, ctrl, target, pcof, cost="Infidelity", gradient=True):
    """every member on a handle made here: (grads [K, n] or None, out3 [K, 3])"""
    G, O = [], []
    for k in range(ens.K):
        dp = qgd.DeviceProblem(ens.member_problem(prob, k), order)
        try:
            dp.set_controls(ctrl)
            if target is not None:
                dp.set_target(target)
            dp.set_cost_type(cost)
            if gradient:
                g, o = dp.discrete_adjoint(pcof)
                G.append(g)
            else:
                o = dp.eval_forward(pcof)
            O.append(np.asarray(o, dtype=np.float64).copy())
        finally:
            dp.close()
    return (np.array(G) if gradient else None), np.array(O)


def _handle(qgd, prob, order, ctrl, target, cost="Infidelity", ens=None):
    dp = qgd.DeviceProblem(prob, order)
    dp.set_controls(ctrl)
    if target is not None:
        dp.set_target(target)
    dp.set_cost_type(cost)
    if ens is not None:
        dp.set_ensemble(ens)
    return dp


def _refused_off_the_small_path(qgd, mode, dp, pcof):
    """general mode: the library has no route for a handle whose small-problem path is off -- QGD_ERR_UNSUPPORTED, True"""
    if mode != "general":
        return False
    with pytest.raises(qgd._lib.QGDError) as e:
        dp.eval_ensemble(pcof)
    assert e.value.code == qgd._lib.QGD_ERR_UNSUPPORTED
    return True


def _same(a, b):
    """two EnsembleResults, bit for bit"""
    return (np.array_equal(a.grad, b.grad) if a.grad is not None else b.grad is None) and a[1:] == b[1:] \
        and (np.array_equal(a.member_grads, b.member_grads) if a.member_grads is not None else b.member_grads is None) \
        and np.array_equal(a.member_out3, b.member_out3)


def _cnot2_members(prob, K=4):
    """the members of tests/test_gpu_ensemble.py::test_members_are_handles_of_their_own_and_the_sums_the_statement"""
    S = np.repeat(prob.system_sym[None], K, axis=0).copy()
    A = np.repeat(prob.system_asym[None], K, axis=0).copy()
    scale = np.ones((K, prob.N_operators))
    for k in range(1, K):
        S[k] += np.diag(np.array([0.0, 0.011, -0.023, 0.017]) * (1.0 + 0.37 * (k - 1)))
    A[2, 0, 1], A[2, 1, 0] = 0.004, -0.004
    if K > 3:
        scale[3] = (1.03, 0.97)
    return S, A, scale


def _check_all_routes(qgd, mode, ens, prob, order, ctrl, target, pcof, cost):
    """The three routes against handles made here and the statement; returns (the auto result, G, O)."""
    E = qgd._lib
    want_route = "device" if mode == "default" else "loop"
    G, O = _member_rows(qgd, ens, prob, order, ctrl, target, pcof, cost)
    _, Of = _member_rows(qgd, ens, prob, order, ctrl, target, pcof, cost, gradient=False)
    rg, rc, rgd = qgd.ensemble_reduce(G, O, ens.weights, cost, prob.N_ess_levels)
    _, fc, fgd = qgd.ensemble_reduce(None, Of, ens.weights, cost, prob.N_ess_levels)
    out = None
    for route in ("auto", "device", "loop"):
        kw = dict(order=order, cost_type=cost, route=route)
        if route == "device" and mode == "general":
            with pytest.raises(E.QGDError) as e:
                qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, ens, **kw)
            assert e.value.code == E.QGD_ERR_UNSUPPORTED
            continue
        res = qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, ens, **kw)
        assert res.route == (want_route if route == "auto" else route)
        assert np.array_equal(res.member_grads, G) and np.array_equal(res.member_out3, O)
        assert np.array_equal(res.grad, rg) and res.cost == rc and res.guard == rgd and np.abs(res.grad).max() > 0
        assert _same(qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, ens, **kw), res)      # a second call, the same bits
        fwd = qgd.eval_ensemble(prob, ctrl, pcof, target, ens, gradient=False, **kw)
        assert fwd.route == res.route and fwd.grad is None and fwd.member_grads is None and np.array_equal(fwd.member_out3, Of)
        assert (fwd.cost, fwd.guard) == (fc, fgd)
        out = out or res
    return out, G, O


# -- 1 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", ["Infidelity", "Tracking"])
def test_members_and_sums(qgd, cost, _small_path_mode):
    """cnot2 at 6 steps, order 4, K = 4, non-dyadic weights, then None: rows against handles made here, sums against the
    statement, on every route, twice, with and without the gradient; rows=False returns the same reduced row and no rows."""
    mode = _small_path_mode
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=6, tf=6.0)
    S, A, scale = _cnot2_members(prob)
    for weights in ([0.17, 0.33, 0.33, 0.17], None):
        ens = qgd.Ensemble(S, A, scale, weights)
        res, G, O = _check_all_routes(qgd, mode, ens, prob, 4, ctrl, target, pcof, cost)
        assert len({g.tobytes() for g in G}) == 4                      # (four different members)
        dp = _handle(qgd, prob, 4, ctrl, target, cost, ens)
        if not _refused_off_the_small_path(qgd, mode, dp, pcof):
            g, c, gd, mg, mo, st = dp.eval_ensemble(pcof, rows=False)
            assert mg is None and mo is None and not st.any()
            assert np.array_equal(g, res.grad) and (c, gd) == (res.cost, res.guard)
            g, c, gd, mg, mo, st = dp.eval_ensemble(pcof, gradient=False, rows=False)
            assert g is None and mg is None and mo is None and (c, gd) == (res.cost, res.guard)
            g, c, gd, mg, mo, st = dp.eval_ensemble(pcof)
            assert np.array_equal(mg, G) and np.array_equal(mo, O) and np.array_equal(g, res.grad)
            dp.set_ensemble(ens)                                       # (the same object: skipped)
            assert np.array_equal(dp.eval_ensemble(pcof, rows=False)[0], res.grad)
        dp.close()
    obj = qgd.EnsembleObjective(prob, ctrl, target, ens, 4, cost)      # the optimiser's objective: no rows, the same sums
    g, c, gd = obj(pcof)
    assert np.array_equal(g, res.grad) and (c, gd) == (res.cost, res.guard)
    obj.close()
    qgd.clear_cache()


# -- 2 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,c,n_ops,order,nsteps,cost,family", [
    (4, 4, 2, 6, 5, "Infidelity", "bspline5"), (3, 2, 1, 4, 2, "Tracking", "bspline5"), (4, 3, 3, 8, 9, "Norm", "bspline5"),
    (2, 2, 4, 2, 33, "Infidelity", "bspline5"), (4, 1, 2, 12, 17, "Infidelity", "bspline5"), (3, 3, 2, 4, 7, "StateTransfer", "bspline5"),
    (4, 2, 2, 4, 127, "Infidelity", "bspline5"),       # the longest grid of the path: 128 time points
    (4, 4, 4, 6, 9, "Infidelity", "bspline8"),         # n_pcof = 64 exactly
    (2, 2, 1, 4, 5, "Tracking", "cos1"),               # n_pcof = 1, the smallest a control family gives
])
def test_shapes(qgd, orc, N, c, n_ops, order, nsteps, cost, family, _small_path_mode):
    """The six shapes of tests/test_gpu_ensemble.py::test_shapes_guards_and_cost_types, built as there -- construct_rand_prob(2,
    construct_rand_prob(3 and construct_rand_prob(4 problems with a diagonal guard, 1-4 columns, 1-4 operators, orders 2-12, the
    four cost types, n_ess = 2, 3, 4 (a division by 9 among them) -- and the ends of the path: 3 and 128 time points, 64
    coefficients, one coefficient.  K = 3, non-uniform weights and operator scales: the sums run over generic doubles, so a
    contracted multiply-add in the reduction fails here.  Member 0 against the oracle at 1e-10 of the gradient's maximum (the
    bound of tests/test_gpu_ensemble.py; StateTransfer, as there, and the one-coefficient cosine control, which the oracle does not
    restate either, against this library's general kernels)."""
    prob = qgd.construct_rand_prob(N, n_ops, tf=1.0, nsteps=nsteps, gmres_abstol=1e-15, gmres_reltol=1e-15, scale=0.7)
    prob.u0 = np.asfortranarray(prob.u0[:, :c]); prob.v0 = np.asfortranarray(prob.v0[:, :c]); prob.N_initial_conditions = c
    rng = np.random.default_rng(N * 100 + c)
    W = np.zeros((2 * N, 2 * N))
    wd = rng.random(N) * (rng.random(N) > 0.4)
    W[np.arange(N), np.arange(N)] = wd; W[N + np.arange(N), N + np.arange(N)] = wd
    prob.guard_subspace_projector = W
    ctrl = {"bspline5": lambda: [qgd.FortranBSplineControl(3, 5, prob.tf) for _ in range(n_ops)],
            "bspline8": lambda: [qgd.FortranBSplineControl(3, 8, prob.tf) for _ in range(n_ops)],
            "cos1": lambda: [qgd.SingleSymCosControl(prob.tf, 2.0) for _ in range(n_ops)]}[family]()
    n_pcof = qgd.get_number_of_control_parameters(ctrl)
    assert n_pcof == {"bspline5": 10 * n_ops, "bspline8": 64, "cos1": 1}[family]
    pcof = rng.standard_normal(n_pcof)
    target = cases.rand_target(prob)
    if cost == "StateTransfer":
        target = target / np.linalg.norm(target, axis=0)
    r = 0.1 * rng.standard_normal((3, N, N)); r[0] = 0.0
    ens = qgd.Ensemble(prob.system_sym[None] + (r + r.transpose(0, 2, 1)), prob.system_asym[None] + (r - r.transpose(0, 2, 1)),
                       1.0 + 0.05 * rng.standard_normal((3, n_ops)) * np.array([[0.0], [1.0], [1.0]]), [0.3, 0.45, 0.25])
    res, G, O = _check_all_routes(qgd, _small_path_mode, ens, prob, order, ctrl, target, pcof, cost)
    assert len({g.tobytes() for g in G}) == 3
    assert O[0, 2] > 0 or not wd.any()
    assert res.guard > 0 or not wd.any()
    if cost == "StateTransfer" or family == "cos1":      # (neither has a restatement in the oracle)
        dp = qgd.DeviceProblem(prob, order)
        try:
            dp.set_small_path(False); dp.set_controls(ctrl); dp.set_target(target); dp.set_cost_type(cost)
            g_ref, _ = dp.discrete_adjoint(pcof)
        finally:
            dp.close()
    else:
        orc.set_converged_terminal(True); orc.set_cost_type(cost)
        try:
            g_ref = orc.discrete_adjoint(prob, ctrl, pcof, target, order=order)
        finally:
            orc.set_converged_terminal(False); orc.set_cost_type("Infidelity")
    err = np.abs(res.member_grads[0] - g_ref).max()
    print(f"\nmember 0 against the reference: {err:.3e}, max|g| = {np.abs(g_ref).max():.3e}")
    assert err <= 1e-10 * np.abs(g_ref).max()
    qgd.clear_cache()


# -- 3 -------------------------------------------------------------------------------------------------------------------------

def _five(qgd, weights=(0.1, 0.3, 0.2, 0.25, 0.15)):
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=6, tf=6.0)
    S, A, scale = _cnot2_members(prob, 5)
    scale[4] = (0.98, 1.01)
    return prob, ctrl, pcof, target, qgd.Ensemble(S, A, scale, None if weights is None else list(weights))


def test_chunking(qgd, monkeypatch, _small_path_mode):
    """QGD_BATCH_CHUNK = 2 (read when the handle is made), cnot2, K = 5 -> 2 + 2 + 1: rows and reduced row are the unchunked
    call's bits, with and without the gradient, with and without rows -- the accumulator carried from chunk to chunk and the
    chunks' operator planes and weights addressed in place."""
    prob, ctrl, pcof, target, ens = _five(qgd)
    whole = _handle(qgd, prob, 4, ctrl, target, ens=ens)
    monkeypatch.setenv("QGD_BATCH_CHUNK", "2")
    parts = _handle(qgd, prob, 4, ctrl, target, ens=ens)
    monkeypatch.delenv("QGD_BATCH_CHUNK")
    if not _refused_off_the_small_path(qgd, _small_path_mode, parts, pcof):
        for gradient in (True, False):
            for rows in (True, False):
                w = whole.eval_ensemble(pcof, gradient=gradient, rows=rows)
                p = parts.eval_ensemble(pcof, gradient=gradient, rows=rows)
                for a, b in zip(w, p):
                    assert (a is None and b is None) or np.array_equal(a, b)
        G, O = _member_rows(qgd, ens, prob, 4, ctrl, target, pcof)
        g, c, gd, mg, mo, _ = parts.eval_ensemble(pcof)
        assert np.array_equal(mg, G) and np.array_equal(mo, O)
        rg, rc, rgd = qgd.ensemble_reduce(G, O, ens.weights, "Infidelity", prob.N_ess_levels)
        assert np.array_equal(g, rg) and (c, gd) == (rc, rgd)
    whole.close(); parts.close()


def test_chunks_shrink_to_the_memory_budget(qgd, _small_path_mode):
    """The per-member arrays are the batch's (POOL_BATCH) and count against qgd_set_memory_budget as there
    (tests/test_gpu_batch.py::test_chunks_shrink_to_the_memory_budget).  The budget cannot go below what the resident grid takes,
    so at that budget a chunk holds budget / (bytes per member) members, never one alone: an ensemble of 2 chunks + 1 cnot2
    members takes three passes and gives the bits of the handle without a budget."""
    prob, ctrl, pcof, target, _ = _five(qgd)
    tight = qgd.DeviceProblem(prob, 4)
    budget = tight.memory_plan()["window_bytes"]
    tight.set_memory_budget(budget)
    assert tight.memory_plan()["windows"] == 1
    tight.set_controls(ctrl); tight.set_target(target)
    nt, m, n_ops, n = prob.nsteps + 1, 2, prob.N_operators, len(pcof)
    per = 8 * (nt * ((m + 1) * n_ops * 2 + 4 * 32 + n) + 8 + n + (n + 5)) + 9 * 64
    chunk = budget // per
    assert 1 <= chunk < 500, (budget, per)
    K = 2 * chunk + 1
    shift = np.linspace(-0.02, 0.02, K)[:, None, None] * np.diag(np.arange(prob.N_tot_levels, dtype=float))
    ens = qgd.Ensemble(prob.system_sym[None] + shift, np.repeat(prob.system_asym[None], K, axis=0), None, np.linspace(0.5, 1.5, K) / K)
    tight.set_ensemble(ens)
    whole = _handle(qgd, prob, 4, ctrl, target, ens=ens)
    if not _refused_off_the_small_path(qgd, _small_path_mode, tight, pcof):
        for gradient in (True, False):
            w = whole.eval_ensemble(pcof, gradient=gradient)
            t = tight.eval_ensemble(pcof, gradient=gradient)
            for a, b in zip(w, t):
                assert (a is None and b is None) or np.array_equal(a, b)
        g, c, gd, mg, mo, _ = tight.eval_ensemble(pcof)
        rg, rc, rgd = qgd.ensemble_reduce(mg, mo, ens.weights, "Infidelity", prob.N_ess_levels)
        assert np.array_equal(g, rg) and (c, gd) == (rc, rgd)
    whole.close(); tight.close()


# -- 4 -------------------------------------------------------------------------------------------------------------------------

def test_the_reduction_runs_in_ascending_order(qgd, _small_path_mode):
    """cnot2, K = 5, weights over six orders of magnitude: the reduced gradient is ensemble_reduce of the downloaded rows, and is
    NOT ensemble_reduce of the same rows taken in descending order (the inputs are checked to tell the two apart)."""
    prob, ctrl, pcof, target, ens = _five(qgd, weights=(1.3e-3, 0.71, 1.9e3, 3.7e-2, 23.0))
    dp = _handle(qgd, prob, 4, ctrl, target, ens=ens)
    if not _refused_off_the_small_path(qgd, _small_path_mode, dp, pcof):
        g, c, gd, mg, mo, _ = dp.eval_ensemble(pcof)
        up = qgd.ensemble_reduce(mg, mo, ens.weights, "Infidelity", prob.N_ess_levels)
        down = qgd.ensemble_reduce(mg[::-1], mo[::-1], ens.weights[::-1], "Infidelity", prob.N_ess_levels)
        assert not np.array_equal(up[0], down[0])                      # (the inputs make the order visible)
        assert np.array_equal(g, up[0]) and (c, gd) == up[1:]
        assert not np.array_equal(g, down[0])
    dp.close()


# -- 5 -------------------------------------------------------------------------------------------------------------------------

def test_members_do_not_leak_into_each_other(qgd, _small_path_mode):
    """cnot2 at order 8, K = 4, member 1 with a system Hamiltonian of 1e150 on the diagonal (its Taylor levels overflow): a
    non-finite row of its own, and the other members' rows are bitwise what they are beside a harmless member 1."""
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=6, tf=6.0)
    S, A, scale = _cnot2_members(prob)
    good = qgd.Ensemble(S, A, scale, [0.17, 0.33, 0.33, 0.17])
    Sb = S.copy(); Sb[1] = np.diag(np.full(prob.N_tot_levels, 1e150))
    bad = qgd.Ensemble(Sb, A, scale, [0.17, 0.33, 0.33, 0.17])
    dp = _handle(qgd, prob, 8, ctrl, target, ens=good)
    if not _refused_off_the_small_path(qgd, _small_path_mode, dp, pcof):
        _, _, _, G, O, _ = dp.eval_ensemble(pcof)
        dp.set_ensemble(bad)
        n, K = len(pcof), 4
        grad, out2, mg, mo, st = np.zeros(n), np.zeros(2), np.zeros((K, n)), np.zeros((K, 3)), np.zeros(K, dtype=np.int32)
        rc = dp.lib.qgd_eval_ensemble(dp.h, _vp(np.ascontiguousarray(pcof)), n, 1, _vp(grad), _vp(out2), _vp(mg), _vp(mo), _vp(st))
        assert rc in (qgd._lib.QGD_OK, qgd._lib.QGD_ERR_NUMERIC) and not st[[0, 2, 3]].any()
        assert not (np.isfinite(mg[1]).all() and np.isfinite(mo[1]).all())
        for k in (0, 2, 3):
            assert np.array_equal(mg[k], G[k]) and np.array_equal(mo[k], O[k])
        dp.set_ensemble(good)                                          # and the handle is as usable as before
        _, _, _, G2, O2, _ = dp.eval_ensemble(pcof)
        assert np.array_equal(G2, G) and np.array_equal(O2, O)
    dp.close()


# -- 6 -------------------------------------------------------------------------------------------------------------------------

def test_what_the_call_leaves_and_refuses(qgd, _small_path_mode):
    """cnot2.  No stored sweep afterwards (a history_precomputed call does what it does on a fresh handle, as after a batch);
    every refusal of include/qgd_ensemble.h, each with the handle's next single evaluation unchanged and no output written."""
    mode = _small_path_mode
    E = qgd._lib
    prob, ctrl, pcof, target, ens = _five(qgd)
    pc = np.ascontiguousarray(pcof)
    n, K = len(pcof), ens.K

    def precomputed(dp):
        try:
            g, o = dp.discrete_adjoint(pcof, history_precomputed=True)
            return ("returned", g.tobytes(), np.asarray(o).tobytes())
        except E.QGDError as e:
            return ("refused", e.code)

    fresh = _handle(qgd, prob, 4, ctrl, target)
    want = precomputed(fresh)
    fresh.close()
    dp = _handle(qgd, prob, 4, ctrl, target, ens=ens)
    g0, o0 = dp.discrete_adjoint(pcof)
    grad, out2, mg, mo, st = np.full(n, 7.0), np.full(2, 7.0), np.full((K, n), 7.0), np.full((K, 3), 7.0), np.full(K, 7, dtype=np.int32)
    ev = dp.lib.qgd_eval_ensemble

    def unchanged(h=dp):
        g, o = h.discrete_adjoint(pcof)
        return np.array_equal(g, g0) and np.array_equal(np.asarray(o), np.asarray(o0)) and all((a == 7).all() for a in (grad, out2, mg, mo, st))

    args = lambda **k: [k.get("h", dp.h), k.get("pcof", _vp(pc)), k.get("n", n), k.get("gradient", 1), k.get("grad", _vp(grad)),
                        k.get("out2", _vp(out2)), _vp(mg), _vp(mo), _vp(st)]
    if mode == "default":
        dp.eval_ensemble(pcof)
        assert precomputed(dp) == want                                 # what the call leaves
        dp.eval_ensemble(pcof, gradient=False)
        assert precomputed(dp) == want
        assert unchanged()
    else:
        assert ev(*args()) == E.QGD_ERR_UNSUPPORTED and unchanged()    # the small path switched off
    assert ev(*args(pcof=None)) == E.QGD_ERR_ARGUMENT and unchanged()
    assert ev(*args(out2=None)) == E.QGD_ERR_ARGUMENT and unchanged()
    assert ev(*args(grad=None)) == E.QGD_ERR_ARGUMENT and unchanged()                  # gradient without grad
    assert ev(*args(n=n - 1)) == E.QGD_ERR_ARGUMENT and unchanged()
    assert ev(*args(n=n + 1)) == E.QGD_ERR_ARGUMENT and unchanged()
    # a refused call leaves the stored sweep as it was: history_precomputed still finds the single call's
    g, _ = dp.discrete_adjoint(pcof, history_precomputed=True)
    assert np.array_equal(g, g0)
    ss, sa, so, ao, w = ens.device_arrays(prob)
    se = dp.lib.qgd_set_ensemble
    assert se(dp.h, -1, _vp(ss), _vp(sa), _vp(so), _vp(ao), _vp(w)) == E.QGD_ERR_ARGUMENT
    for hole in range(5):
        a = [_vp(ss), _vp(sa), _vp(so), _vp(ao), _vp(w)]; a[hole] = None
        assert se(dp.h, K, *a) == E.QGD_ERR_ARGUMENT
    if mode == "default":                                              # (a refused setter leaves the ensemble that was set)
        assert np.array_equal(dp.eval_ensemble(pcof, rows=False)[0], qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, ens, order=4, route="loop").grad)
        grad[:] = 7.0; out2[:] = 7.0
    assert se(dp.h, 0, None, None, None, None, None) == E.QGD_OK       # released: no ensemble set
    assert ev(*args()) == E.QGD_ERR_STATE and unchanged()
    dp.close()
    # gradients without a target: QGD_ERR_STATE; a forward-only call needs none
    dp = _handle(qgd, prob, 4, ctrl, None, ens=ens)
    f0 = np.asarray(dp.eval_forward(pcof))
    assert ev(*args(h=dp.h)) == E.QGD_ERR_STATE and np.array_equal(np.asarray(dp.eval_forward(pcof)), f0) and (grad == 7).all()
    if mode == "default":
        _, _, _, _, mo_f, _ = dp.eval_ensemble(pcof, gradient=False)
        assert np.array_equal(mo_f[0], f0)                             # (member 0 is the problem itself)
    dp.close()
    # no control basis, no ensemble: QGD_ERR_STATE
    dp = qgd.DeviceProblem(prob, 4)
    assert ev(*args(h=dp.h)) == E.QGD_ERR_STATE
    E.check(dp.h, se(dp.h, K, _vp(ss), _vp(sa), _vp(so), _vp(ao), _vp(w)))
    assert ev(*args(h=dp.h)) == E.QGD_ERR_STATE and (grad == 7).all() and (mg == 7).all()
    dp.close()
    # a partitioned handle: single-GPU only
    dp = qgd.DeviceProblem(prob, 4)
    E.check(dp.h, dp.lib.qgd_set_partition(dp.h, 0, 2))
    assert ev(*args(h=dp.h)) == E.QGD_ERR_UNSUPPORTED and (grad == 7).all()
    dp.close()
    # event bracketing on: not the small-problem path's
    dp = _handle(qgd, prob, 4, ctrl, target, ens=ens)
    dp.set_timing(1)
    assert ev(*args(h=dp.h)) == E.QGD_ERR_UNSUPPORTED and (grad == 7).all() and (mg == 7).all()
    dp.close()


def test_nine_levels_are_refused_and_auto_takes_the_loop(qgd):
    """N = 9 (the problem of tests/test_gpu_ensemble.py::test_nine_levels): QGD_ERR_UNSUPPORTED from the library, the loop from auto."""
    E = qgd._lib
    prob = qgd.construct_rand_prob(9, 2, tf=1.0, nsteps=5, gmres_abstol=1e-15, gmres_reltol=1e-15, scale=0.7)
    prob.u0 = np.asfortranarray(prob.u0[:, :2]); prob.v0 = np.asfortranarray(prob.v0[:, :2]); prob.N_initial_conditions = 2
    ctrl = [qgd.FortranBSplineControl(3, 5, prob.tf) for _ in range(2)]
    pcof = np.random.default_rng(9).standard_normal(qgd.get_number_of_control_parameters(ctrl))
    target = cases.rand_target(prob)
    r = 0.1 * np.random.default_rng(10).standard_normal((2, 9, 9))
    ens = qgd.Ensemble(prob.system_sym[None] + (r + r.transpose(0, 2, 1)), prob.system_asym[None] + (r - r.transpose(0, 2, 1)),
                       [[1.0, 1.0], [1.02, 0.98]], [0.4, 0.6])
    with pytest.raises(E.QGDError) as e:
        qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, ens, order=4, route="device")
    assert e.value.code == E.QGD_ERR_UNSUPPORTED
    assert qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, ens, order=4).route == "loop"
    qgd.clear_cache()


def test_a_singular_member_is_flagged_and_the_others_are_written(qgd, _small_path_mode):
    """cnot2 at order 2 with dt = 1 and pcof = 0: L = I - (dt / 2) (K_sys - i S_sys), so the antisymmetric slot holding 2 I (the C
    call does not test symmetry) and a zero symmetric part make member 1's step matrix exactly zero.  QGD_ERR_NUMERIC, member_status = (0, 1, 0), the other rows
    bitwise what they are beside a regular member 1, and the next call is clean."""
    E = qgd._lib
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=6, tf=6.0)
    pc = np.zeros(len(pcof))
    S, A, scale = _cnot2_members(prob, 3)
    ens = qgd.Ensemble(S, A, scale, [0.2, 0.5, 0.3])
    dp = _handle(qgd, prob, 2, ctrl, target, ens=ens)
    if not _refused_off_the_small_path(qgd, _small_path_mode, dp, pc):
        _, _, _, G, O, _ = dp.eval_ensemble(pc)
        ss, sa, so, ao, w = ens.device_arrays(prob)
        sa = sa.copy(); sa[1] = 2.0 * np.eye(prob.N_tot_levels)
        ss = ss.copy(); ss[1] = 0.0
        E.check(dp.h, dp.lib.qgd_set_ensemble(dp.h, 3, _vp(ss), _vp(sa), _vp(so), _vp(ao), _vp(w)))
        n, K = len(pc), 3
        grad, out2, mg, mo, st = np.zeros(n), np.zeros(2), np.zeros((K, n)), np.zeros((K, 3)), np.zeros(K, dtype=np.int32)
        rc = dp.lib.qgd_eval_ensemble(dp.h, _vp(pc), n, 1, _vp(grad), _vp(out2), _vp(mg), _vp(mo), _vp(st))
        assert rc == E.QGD_ERR_NUMERIC and st.tolist() == [0, 1, 0]
        for k in (0, 2):
            assert np.array_equal(mg[k], G[k]) and np.array_equal(mo[k], O[k])
        ss, sa, so, ao, w = ens.device_arrays(prob)
        E.check(dp.h, dp.lib.qgd_set_ensemble(dp.h, 3, _vp(ss), _vp(sa), _vp(so), _vp(ao), _vp(w)))
        st[:] = 0
        assert dp.lib.qgd_eval_ensemble(dp.h, _vp(pc), n, 1, _vp(grad), _vp(out2), _vp(mg), _vp(mo), _vp(st)) == E.QGD_OK and not st.any()
        assert np.array_equal(mg, G) and np.array_equal(mo, O)
        g1, o1 = dp.discrete_adjoint(pc)                               # and the single path's status word was not left dirty
        assert np.array_equal(g1, G[0])
    dp.close()


# -- 7 -------------------------------------------------------------------------------------------------------------------------

def test_a_batch_is_unchanged_by_an_ensemble_call_before_it(qgd, _small_path_mode):
    """cnot2: eval_batch(P) on the same handle before and after eval_ensemble, the same bits (the two share POOL_BATCH), and the
    ensemble's after the batch."""
    prob, ctrl, pcof, target, ens = _five(qgd)
    P = 0.05 * np.random.default_rng(11).standard_normal((3, len(pcof)))
    dp = _handle(qgd, prob, 4, ctrl, target, ens=ens)
    G0, S0, _ = dp.eval_batch(P)
    if not _refused_off_the_small_path(qgd, _small_path_mode, dp, pcof):
        first = dp.eval_ensemble(pcof)
        G1, S1, st1 = dp.eval_batch(P)
        assert dp.batch_path_taken() and not st1.any() and np.array_equal(G1, G0) and np.array_equal(S1, S0)
        again = dp.eval_ensemble(pcof)
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
        _, S2, _ = dp.eval_batch(P, gradient=False)
        assert np.array_equal(S2, np.array([np.asarray(dp.eval_forward(p)) for p in P]))
    dp.close()
