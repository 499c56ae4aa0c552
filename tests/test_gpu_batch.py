"""GPU tests of batched evaluation (qgd_eval_batch, DeviceProblem.eval_batch): K coefficient vectors of one
problem in one call.  The contract is bitwise: member k receives what the single call on the same handle returns for pcofs[k].
Small problems (csrc/qgd_k_tiny.hip) run their members side by side -- a member axis on the four launches of that path --,
everything else runs them one after another inside the library.  The path is set per handle, as in tests/test_gpu_tiny.py."""
import ctypes as C

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu


def _handle(qgd, prob, order, ctrl, target, small=True, cost="Infidelity"):
    dp = qgd.DeviceProblem(prob, order)
    dp.set_small_path(small)
    dp.set_controls(ctrl)
    if target is not None:
        dp.set_target(target)
    dp.set_cost_type(cost)
    return dp


def _singles(dp, P, gradient=True):
    if gradient:
        res = [dp.discrete_adjoint(p) for p in P]
        return np.array([g for g, _ in res]), np.array([np.asarray(o) for _, o in res])
    return None, np.array([np.asarray(dp.eval_forward(p)) for p in P])


def _assert_members_equal_singles(dp, P, batched, gradient=True):
    """eval_batch(P) against the single calls on the same handle, bit for bit, and the route it took"""
    g_ref, s_ref = _singles(dp, P, gradient)
    G, S, st = dp.eval_batch(P, gradient=gradient)
    assert dp.batch_path_taken() == batched
    assert S.shape == (len(P), 3) and st.shape == (len(P),) and st.dtype == np.int32 and not st.any()
    assert np.array_equal(S, s_ref)
    if gradient:
        assert G.shape == P.shape and np.array_equal(G, g_ref)
    else:
        assert G is None
    return G, S


@pytest.fixture(scope="module")
def cnot2(qgd):
    """cnot2 at 6 steps, order 4, with five distinct coefficient vectors (shared, never written)"""
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=6, tf=6.0)
    P = 0.05 * np.random.default_rng(11).standard_normal((5, len(pcof)))
    P.setflags(write=False)
    return prob, ctrl, pcof, target, P


# -- 1 -------------------------------------------------------------------------------------------------------------------------

def test_members_equal_single_calls_bitwise(qgd, cnot2):
    prob, ctrl, pcof, target, P = cnot2
    dp = _handle(qgd, prob, 4, ctrl, target)
    dp.discrete_adjoint(P[0])
    assert dp.small_path_taken()
    G, S = _assert_members_equal_singles(dp, P, True)
    _, S0 = _assert_members_equal_singles(dp, P, True, gradient=False)
    G2, S2, _ = dp.eval_batch(P)                                       # the same bits on every run
    assert np.array_equal(G2, G) and np.array_equal(S2, S)
    assert np.abs(G).max() > 0 and len({g.tobytes() for g in G}) == 5      # (five different, non-trivial members)
    _assert_members_equal_singles(dp, P[:1], True)                     # K = 1
    G1, S1, st1 = dp.eval_batch(P[3])                                  # a single vector is a batch of one
    assert G1.shape == (1, P.shape[1]) and np.array_equal(G1[0], G[3]) and np.array_equal(S1[0], S[3])
    twins = np.ascontiguousarray(np.vstack([P[4], P[4]]))              # K = 2, equal members: a member stride of zero would pass K = 1
    Gt, St = _assert_members_equal_singles(dp, twins, True)
    assert np.array_equal(Gt[0], Gt[1]) and np.array_equal(Gt[1], G[4]) and np.array_equal(St[1], S[4])
    # caller's output arrays
    og, os_ = np.full(P.shape, np.nan), np.full((5, 3), np.nan)
    Gr, Sr, _ = dp.eval_batch(P, out_grads=og, out_scalars=os_)
    assert Gr is og and Sr is os_ and np.array_equal(og, G) and np.array_equal(os_, S)
    dp.close()


# -- 2 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,c,n_ops,order,nsteps,cost", [(4, 4, 2, 6, 5, "Infidelity"), (3, 2, 1, 4, 2, "Tracking"), (4, 3, 3, 8, 9, "Norm"),
                                                         (2, 2, 4, 2, 33, "Infidelity"), (4, 1, 2, 12, 17, "Infidelity")])
def test_shapes_the_path_covers(qgd, orc, N, c, n_ops, order, nsteps, cost):
    """Random dense problems with a diagonal guard projector, built like test_shapes_guards_and_cost_types of
    tests/test_gpu_tiny.py: fewer columns than rows, 1-4 control operators, the three cost types, the shortest grid the path takes
    (3 time points), n_pcof = 10, 20, 30 (no multiples of the 16-coefficient tile of the fixed-order sum) and 40.  K = 3, bitwise
    against the single calls; member 0 against the oracle at that file's bound, 1e-10 of the gradient's maximum."""
    prob = qgd.construct_rand_prob(N, n_ops, tf=1.0, nsteps=nsteps, gmres_abstol=1e-15, gmres_reltol=1e-15, scale=0.7)
    prob.u0 = np.asfortranarray(prob.u0[:, :c]); prob.v0 = np.asfortranarray(prob.v0[:, :c]); prob.N_initial_conditions = c
    rng = np.random.default_rng(N * 100 + c)
    W = np.zeros((2 * N, 2 * N))
    wd = rng.random(N) * (rng.random(N) > 0.4)
    W[np.arange(N), np.arange(N)] = wd; W[N + np.arange(N), N + np.arange(N)] = wd
    prob.guard_subspace_projector = W
    ctrl = [qgd.FortranBSplineControl(3, 5, prob.tf) for _ in range(n_ops)]
    n_pcof = qgd.get_number_of_control_parameters(ctrl)
    assert n_pcof == 10 * n_ops
    P = rng.standard_normal((3, n_pcof))
    target = cases.rand_target(prob)
    orc.set_converged_terminal(True); orc.set_cost_type(cost)
    try:
        g_ref = orc.discrete_adjoint(prob, ctrl, P[0], target, order=order)
    finally:
        orc.set_converged_terminal(False); orc.set_cost_type("Infidelity")
    dp = _handle(qgd, prob, order, ctrl, target, cost=cost)
    dp.discrete_adjoint(P[0])
    assert dp.small_path_taken()
    G, S = _assert_members_equal_singles(dp, P, True)
    _assert_members_equal_singles(dp, P, True, gradient=False)
    assert np.abs(G[0] - g_ref).max() <= 1e-10 * np.abs(g_ref).max()
    assert S[0, 2] > 0 or not wd.any()
    dp.close()


# -- 3 -------------------------------------------------------------------------------------------------------------------------

def test_members_do_not_leak_into_each_other(qgd, cnot2):
    """NaN coefficients propagate, as on the single path (test_nan_coefficients_propagate_like_the_general_path): one member of
    NaNs gives a NaN gradient, no error and no singular flag, and leaves its neighbours' bits alone."""
    prob, ctrl, pcof, target, P = cnot2
    dp = _handle(qgd, prob, 4, ctrl, target)
    g_ref, s_ref = _singles(dp, P[:4])
    Q = P[:4].copy(); Q[1] = np.nan
    G, S, st = dp.eval_batch(Q)
    assert dp.batch_path_taken() and not st.any()
    for k in (0, 2, 3):
        assert np.array_equal(G[k], g_ref[k]) and np.array_equal(S[k], s_ref[k])
    assert np.isnan(G[1]).all() and np.isnan(S[1, 0])
    _, Sf, st = dp.eval_batch(Q, gradient=False)
    assert np.isnan(Sf[1, 0]) and np.array_equal(Sf[[0, 2, 3]], np.array([np.asarray(dp.eval_forward(Q[k])) for k in (0, 2, 3)]))
    _assert_members_equal_singles(dp, P[:4], True)                     # and the handle is as usable as before
    dp.close()


# -- 4 -------------------------------------------------------------------------------------------------------------------------

def test_chunking(qgd, cnot2, monkeypatch):
    """QGD_BATCH_CHUNK (read once, when the handle is created): chunks of two members, K = 5 -> 2 + 2 + 1."""
    prob, ctrl, pcof, target, P = cnot2
    whole = _handle(qgd, prob, 4, ctrl, target)
    monkeypatch.setenv("QGD_BATCH_CHUNK", "2")
    parts = _handle(qgd, prob, 4, ctrl, target)
    monkeypatch.delenv("QGD_BATCH_CHUNK")
    for gradient in (True, False):
        Gw, Sw, _ = whole.eval_batch(P, gradient=gradient)
        Gp, Sp, stp = parts.eval_batch(P, gradient=gradient)
        assert whole.batch_path_taken() and parts.batch_path_taken() and not stp.any()
        assert np.array_equal(Sp, Sw) and (not gradient or np.array_equal(Gp, Gw))
    _assert_members_equal_singles(parts, P, True)
    whole.close(); parts.close()


def test_chunks_shrink_to_the_memory_budget(qgd, cnot2):
    """The arrays of a chunk count against qgd_set_memory_budget.  With the budget at what the resident grid itself takes, a chunk
    holds budget / (bytes per member) members -- per member nt ((m+1) n_ops 2 + 4 32 + n_pcof) + 8 doubles, its coefficient and
    result rows and the allocator's 64 bytes for each of the nine buffers -- and 2 chunks + 1 members take
    three passes: the bits of the handle without a budget."""
    prob, ctrl, pcof, target, P = cnot2
    whole = _handle(qgd, prob, 4, ctrl, target)
    tight = qgd.DeviceProblem(prob, 4)
    budget = tight.memory_plan()["window_bytes"]
    tight.set_memory_budget(budget)
    assert tight.memory_plan()["windows"] == 1 and tight.memory_plan()["budget"] == budget
    tight.set_small_path(True); tight.set_controls(ctrl); tight.set_target(target)
    nt, m, n_ops, n = prob.nsteps + 1, 2, prob.N_operators, P.shape[1]
    per = 8 * (nt * ((m + 1) * n_ops * 2 + 4 * 32 + n) + 8 + n + (n + 5)) + 9 * 64
    chunk = budget // per
    assert 1 <= chunk < 500, (budget, per)               # (the budget binds well below the 1024-member limit)
    Q = np.ascontiguousarray(np.resize(P, (2 * chunk + 1, n)) * np.linspace(0.5, 1.5, 2 * chunk + 1)[:, None])
    for gradient in (True, False):
        Gw, Sw, _ = whole.eval_batch(Q, gradient=gradient)
        Gt, St, stt = tight.eval_batch(Q, gradient=gradient)
        assert whole.batch_path_taken() and tight.batch_path_taken() and not stt.any()
        assert np.array_equal(St, Sw) and (not gradient or np.array_equal(Gt, Gw))
    _assert_members_equal_singles(tight, P, True)
    whole.close(); tight.close()


# -- 5 -------------------------------------------------------------------------------------------------------------------------

def test_loop_route_small_path_off(qgd, cnot2):
    prob, ctrl, pcof, target, P = cnot2
    dp = _handle(qgd, prob, 4, ctrl, target, small=False)
    _assert_members_equal_singles(dp, P, False)
    assert not dp.small_path_taken()
    _assert_members_equal_singles(dp, P, False, gradient=False)
    dp.close()


def test_loop_route_nine_levels(qgd):
    prob = qgd.construct_rand_prob(9, 2, tf=1.0, nsteps=5, gmres_abstol=1e-15, gmres_reltol=1e-15, scale=0.7)
    prob.u0 = np.asfortranarray(prob.u0[:, :2]); prob.v0 = np.asfortranarray(prob.v0[:, :2]); prob.N_initial_conditions = 2
    ctrl = [qgd.FortranBSplineControl(3, 5, prob.tf) for _ in range(2)]
    P = np.random.default_rng(9).standard_normal((3, qgd.get_number_of_control_parameters(ctrl)))
    dp = _handle(qgd, prob, 4, ctrl, cases.rand_target(prob))
    _assert_members_equal_singles(dp, P, False)
    _assert_members_equal_singles(dp, P, False, gradient=False)
    dp.close()


# -- 6 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("small", [True, False])
def test_what_a_batch_leaves_on_the_handle(qgd, cnot2, small):
    """No stored sweep: a history_precomputed call after a batch does what it does on a handle that never ran one, on both
    routes; and a single call after a batch has the bits it had before."""
    prob, ctrl, pcof, target, P = cnot2

    def precomputed(dp):
        try:
            g, o = dp.discrete_adjoint(P[0], history_precomputed=True)
            return ("returned", g.tobytes(), np.asarray(o).tobytes())
        except qgd._lib.QGDError as e:
            return ("refused", e.code)

    fresh = _handle(qgd, prob, 4, ctrl, target, small=small)
    want = precomputed(fresh)
    fresh.close()
    dp = _handle(qgd, prob, 4, ctrl, target, small=small)
    g0, o0 = dp.discrete_adjoint(P[1])                                 # (a stored sweep the batch must void)
    f0 = np.asarray(dp.eval_forward(P[1]))
    for gradient in (True, False):
        dp.eval_batch(P, gradient=gradient)
        assert dp.batch_path_taken() == small
        assert precomputed(dp) == want
        dp.eval_batch(P, gradient=gradient)
        g1, o1 = dp.discrete_adjoint(P[1])
        assert np.array_equal(g1, g0) and np.array_equal(np.asarray(o1), np.asarray(o0))
        dp.eval_batch(P, gradient=gradient)
        assert np.array_equal(np.asarray(dp.eval_forward(P[1])), f0)
    dp.close()


# -- 7 -------------------------------------------------------------------------------------------------------------------------

def test_refusals(qgd, cnot2):
    prob, ctrl, pcof, target, P = cnot2
    E = qgd._lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n = P.shape[1]
    Pc = np.ascontiguousarray(P)
    for small in (True, False):
        dp = _handle(qgd, prob, 4, ctrl, target, small=small)
        g0, o0 = dp.discrete_adjoint(P[0])
        G, S, st = np.full((5, n), 7.0), np.full((5, 3), 7.0), np.full(5, 7, dtype=np.int32)

        def unchanged():
            g, o = dp.discrete_adjoint(P[0])
            return np.array_equal(g, g0) and np.array_equal(np.asarray(o), np.asarray(o0)) and (G == 7).all() and (S == 7).all() and (st == 7).all()

        batch = dp.lib.qgd_eval_batch
        assert batch(dp.h, vp(Pc), 5, n - 1, vp(G), vp(S), vp(st)) == E.QGD_ERR_ARGUMENT and unchanged()      # wrong n_pcof
        assert batch(dp.h, vp(Pc), 5, n + 1, vp(G), vp(S), vp(st)) == E.QGD_ERR_ARGUMENT and unchanged()
        assert batch(dp.h, vp(Pc), 0, n, vp(G), vp(S), vp(st)) == E.QGD_ERR_ARGUMENT and unchanged()          # K = 0
        assert batch(dp.h, vp(Pc), -3, n, vp(G), vp(S), vp(st)) == E.QGD_ERR_ARGUMENT and unchanged()
        assert batch(dp.h, None, 5, n, vp(G), vp(S), vp(st)) == E.QGD_ERR_ARGUMENT and unchanged()            # NULL pcofs, out3
        assert batch(dp.h, vp(Pc), 5, n, vp(G), None, vp(st)) == E.QGD_ERR_ARGUMENT and unchanged()
        # a refused call leaves the stored sweep as it was: the single call above stored one, history_precomputed still finds it
        g, _ = dp.discrete_adjoint(P[0], history_precomputed=True)
        assert np.array_equal(g, g0)
        with pytest.raises(ValueError, match="pcofs"):
            dp.eval_batch(P[:, :-1])
        dp.close()
        # gradients without a target: QGD_ERR_STATE; forward-only batches need none
        dp = _handle(qgd, prob, 4, ctrl, None, small=small)
        f0 = np.asarray(dp.eval_forward(P[0]))
        with pytest.raises(E.QGDError) as e:
            dp.eval_batch(P)
        assert e.value.code == E.QGD_ERR_STATE
        assert np.array_equal(np.asarray(dp.eval_forward(P[0])), f0)
        _, S2, _ = dp.eval_batch(P, gradient=False)
        assert np.array_equal(S2[0], f0)
        dp.close()
        # no control basis: QGD_ERR_STATE
        dp = qgd.DeviceProblem(prob, 4); dp.set_small_path(small)
        assert dp.lib.qgd_eval_batch(dp.h, vp(Pc), 5, n, None, vp(S), None) == E.QGD_ERR_STATE and (S == 7).all()
        dp.close()
    # a partitioned handle: the batch is single-GPU
    dp = qgd.DeviceProblem(prob, 4)
    E.check(dp.h, dp.lib.qgd_set_partition(dp.h, 0, 2))
    S = np.full((5, 3), 7.0)
    assert dp.lib.qgd_eval_batch(dp.h, vp(Pc), 5, n, None, vp(S), None) == E.QGD_ERR_UNSUPPORTED and (S == 7).all()
    dp.close()


# -- 8 -------------------------------------------------------------------------------------------------------------------------

def test_eval_grad_finite_difference_is_one_batch_with_the_bits_of_the_loop(qgd, cnot2):
    prob, ctrl, pcof, target, P = cnot2
    d, order = 1e-5, 4
    g_fd = qgd.eval_grad_finite_difference(prob, ctrl, pcof, target, dpcof=d, order=order)
    dp = qgd.device_problem(prob, order)                               # the handle the call above ran on
    dp.set_controls(ctrl); dp.set_target(target)
    assert getattr(dp, "_cost_type", 0) == 0                           # (restored)

    def cost(p):
        a, b, guard = dp.eval_forward(p)
        return (1.0 - (a * a + b * b) / prob.N_ess_levels ** 2) + guard

    want = np.zeros(len(pcof))
    for i in range(len(pcof)):
        e = np.zeros(len(pcof)); e[i] = d
        want[i] = (cost(pcof + e) - cost(pcof - e)) / (2 * d)
    assert np.array_equal(g_fd, want)
    g_adj = qgd.discrete_adjoint(prob, ctrl, pcof, target, order=order)
    scale = np.abs(g_adj).max()
    assert np.abs(g_fd - g_adj).max() <= 3e-9 * max(1.0, scale)        # (the bound of test_forced_gradient_reference_contract)
    # the functional batch calls: rows of single calls
    Gb = qgd.discrete_adjoint_batch(prob, ctrl, P, target, order=order)
    assert Gb.shape == P.shape and np.array_equal(Gb[2], qgd.discrete_adjoint(prob, ctrl, P[2], target, order=order))
    Jb = qgd.eval_objective_batch(prob, ctrl, P, target, order=order)
    assert Jb.shape == (5,) and Jb[2] == cost(P[2])
    qgd.clear_cache()
