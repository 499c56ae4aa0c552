"""GPU tests of qgd_eval_dense_pullback: the pullback of the dense trajectory outputs -- states, level
populations and expectation values of the Hermite interpolant -- to pcof.

Bounds: those of tests/test_gpu_pullback.py.  Against the numpy statement (proto_dense_pullback.py, which
test_dense_pullback_proto.py holds to differences of its own outputs) on the same inputs: 1e-10 max(1, max|g|).  Against
Richardson differences of the device's own eval_dense_* outputs (h = 1e-3 and 5e-4 extrapolated): 1e-8 of the difference
quotient.  The measured figures are in DESIGN.md section 4j."""
import ctypes as C
import re

import numpy as np
import pytest

import cases
import proto_dense_pullback as pdp
import proto_pullback as pb
from test_gpu_hessian import _case, _handle
from test_gpu_hvp import _paths
from test_gpu_pullback import _close, _hermitian

pytestmark = pytest.mark.gpu


def _rand10(qgd):
    """10 levels in 10 columns: Np = 16 with six padding rows, two column groups of which the second holds two columns"""
    prob = qgd.construct_rand_prob(10, 2, tf=0.5, nsteps=6, gmres_abstol=1e-15, gmres_reltol=1e-15)
    ctrl = [qgd.FortranBSplineControl(16, 20, prob.tf) for _ in range(2)]
    pcof = np.random.default_rng(9).random(qgd.get_number_of_control_parameters(ctrl))
    return prob, ctrl, pcof, cases.rand_target(prob)


# name -> (case, order, refine)
SHAPES = {
    "cnot2-o2": (lambda q: _case(q, "cnot2"), 2, 2),                                  # N = 4, Np = 16, c = 4: padded rows and columns
    "cnot2-o8": (lambda q: _case(q, "cnot2"), 8, 3),
    "cnot2-o16": (lambda q: _case(q, "cnot2"), 16, 7),
    "guarded": (lambda q: _case(q, "guarded"), 6, 3),                                 # N = 9
    "rand4": (lambda q: _case(q, "rand4"), 4, 3),                                     # dense operators
    "one-step": (lambda q: cases.cnot2_case(q, nsteps=1, tf=1.0), 4, 3),              # both ends are boundary points
    "cnot3-r2": (lambda q: cases.cnot3_case(q, nsteps=20, tf=20.0), 8, 2),            # N = 64, sparse handle, c = 8
    "cnot3-r7": (lambda q: cases.cnot3_case(q, nsteps=20, tf=20.0), 8, 7),
    "cnot3-o16": (lambda q: cases.cnot3_case(q, nsteps=5, tf=5.0), 16, 2),            # the largest LDS footprint of the sweep kernel
    "rand10": (_rand10, 6, 3),                                                        # c no multiple of 8, N no multiple of 16
}


def _bars(prob, rng, refine, n_obs=3, n_groups=5):
    N, c, slots = prob.N_tot_levels, prob.N_initial_conditions, 1 + prob.nsteps * refine
    return dict(states_bar=rng.standard_normal((2 * N, slots, c)), populations_bar=rng.standard_normal((n_groups, slots, c)),
                level_map=rng.standard_normal((n_groups, N)), expectations_bar=rng.standard_normal((n_obs, slots, c)),
                observables=_hermitian(rng, n_obs, N))


def _proto_names(part):
    names = dict(states_bar="states_bar", populations_bar="pop_bar", level_map="level_map", expectations_bar="expect_bar",
                 observables="observables")
    return {names[k]: v for k, v in part.items()}


# -- 1: the device against the numpy statement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SHAPES))
def test_device_matches_the_statement(qgd, name):
    make, order, refine = SHAPES[name]
    prob, ctrl, pcof, target = make(qgd)
    N, c, slots = prob.N_tot_levels, prob.N_initial_conditions, 1 + prob.nsteps * refine
    rng = np.random.default_rng(17)
    bars = _bars(prob, rng, refine)
    real_obs = _hermitian(rng, 2, N, False)
    parts = {"states": dict(states_bar=bars["states_bar"]),
             "populations with a 5-row map": dict(populations_bar=bars["populations_bar"], level_map=bars["level_map"]),
             "populations without a map": dict(populations_bar=rng.standard_normal((N, slots, c))),
             "expectations, complex observables": dict(expectations_bar=bars["expectations_bar"], observables=bars["observables"]),
             "expectations, real observables": dict(expectations_bar=rng.standard_normal((2, slots, c)), observables=real_obs),
             "all three at once": bars}
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    fwd = pb.forward(prob, Gp, Gq, off, pcof, order)
    refs = {label: pdp.dense_pullback(qgd, prob, Gp, Gq, off, pcof, order, refine, fwd=fwd, **_proto_names(part))
            for label, part in parts.items()}
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        if name.startswith("cnot3"):
            assert N == 64 and dp.operator_path()[0] == "sparse"
        for path in _paths(qgd, dp):
            for label, part in parts.items():
                _close(dp.eval_dense_pullback(refine, pcof, **part), refs[label], f"{name} order {order} refine {refine} {path}: {label}")
    finally:
        dp.close()


# -- 2: differences of the device's own dense outputs ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,order,refine", [("cnot2", 8, 3), ("guarded", 6, 3)])
def test_matches_differences_of_the_dense_outputs(qgd, name, order, refine):
    prob, ctrl, pcof, target = _case(qgd, name)
    rng = np.random.default_rng(5)
    bars = _bars(prob, rng, refine, n_groups=3)
    sb, pbar, lm, eb, obs = (bars[k] for k in ("states_bar", "populations_bar", "level_map", "expectations_bar", "observables"))
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        g = dp.eval_dense_pullback(refine, pcof, **bars)

        def J(p):
            return (np.sum(sb * dp.eval_dense_states(refine, p)) + np.sum(pbar * dp.eval_dense_populations(refine, p, level_map=lm))
                    + np.sum(eb * dp.eval_dense_expectations(refine, obs, p)))
        for _ in range(2):
            d = rng.standard_normal(len(pcof)); d /= np.linalg.norm(d)

            def fd(h):
                return (J(pcof + h * d) - J(pcof - h * d)) / (2 * h)
            F = (4 * fd(5e-4) - fd(1e-3)) / 3
            err = abs(g @ d - F)
            print(f"\n{name} order {order} refine {refine}: |g.d - fd| = {err:.3e}, |fd| = {abs(F):.3e}")
            assert err <= 1e-8 * abs(F)
    finally:
        dp.close()


# -- 3: grid slots and refine = 1 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,order", [("cnot2", 4), ("guarded", 6)])
def test_grid_slots_and_refine_one_are_the_grid_point_pullback(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    refine = 3
    rng = np.random.default_rng(23)
    wide = _bars(prob, rng, refine)
    grid = dict(wide)
    for k in ("states_bar", "populations_bar", "expectations_bar"):
        grid[k] = np.asfortranarray(wide[k][:, ::refine])
        wide[k] = np.zeros_like(wide[k]); wide[k][:, ::refine] = grid[k]
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        ref = dp.eval_pullback(pcof, **grid)
        _close(dp.eval_dense_pullback(refine, pcof, **wide), ref, f"{name}: a cotangent that is zero off the grid slots vs eval_pullback")
        assert np.array_equal(dp.eval_dense_pullback(1, pcof, **grid), ref)
        assert np.array_equal(dp.eval_dense_pullback(1, pcof, history_precomputed=True, **grid), ref)
        dp.set_save_every(3)                           # no part in it, as in eval_dense
        assert np.array_equal(dp.eval_dense_pullback(1, pcof, **grid), ref)
        dp.set_save_every(1)
        moved = dict(grid)                             # slot 0 is ignored
        for k in ("states_bar", "populations_bar", "expectations_bar"):
            moved[k] = grid[k].copy(order="F"); moved[k][:, 0] = 1e3
        assert np.array_equal(dp.eval_dense_pullback(1, pcof, **moved), ref)
        full = _bars(prob, rng, refine)
        g = dp.eval_dense_pullback(refine, pcof, **full)
        for k in ("states_bar", "populations_bar", "expectations_bar"):
            full[k][:, 0] = 1e3
        assert np.array_equal(dp.eval_dense_pullback(refine, pcof, **full), g)
    finally:
        dp.close()


# -- 4: reproducibility and the stored sweep ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cnot2", "guarded"])
def test_reproducible_and_leaves_the_stored_sweep_usable(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    order, refine = 4, 3
    rng = np.random.default_rng(7)
    bars = _bars(prob, rng, refine)
    sb = rng.standard_normal((2 * N, nt, c))
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        g = dp.eval_dense_pullback(refine, pcof, **bars)
        for _ in range(2):
            assert np.array_equal(dp.eval_dense_pullback(refine, pcof, **bars), g)
        assert np.array_equal(dp.eval_dense_pullback(refine, pcof, history_precomputed=True, **bars), g)
        dp.set_timing(1)
        dp.eval_dense_pullback(refine, pcof, history_precomputed=True, **bars)
        names = set(dp.timings())
        dp.set_timing(0)
        assert {"dense_pullback_transpose", "dense_pullback_sweep", "dense_pullback_adjoint"} <= names \
            and not (names & {"sweep_forward", "build_LR", "derivs"}), names
        # another pcof under history_precomputed: the sweep is redone
        fresh = _handle(qgd, prob, ctrl, target, order)
        try:
            assert np.array_equal(dp.eval_dense_pullback(refine, 0.5 * pcof, history_precomputed=True, **bars),
                                  fresh.eval_dense_pullback(refine, 0.5 * pcof, **bars))
        finally:
            fresh.close()
        # the calls around it return the bits they returned before it
        g0, o0 = dp.discrete_adjoint(pcof)
        p0, d0 = dp.eval_pullback(pcof, states_bar=sb), dp.eval_dense_states(refine, pcof)
        assert np.array_equal(dp.eval_dense_pullback(refine, pcof, **bars), g)
        g1, o1 = dp.discrete_adjoint(pcof, history_precomputed=True)
        assert np.array_equal(g1, g0) and np.array_equal(o1, o0)
        assert np.array_equal(dp.eval_dense_pullback(refine, pcof, history_precomputed=True, **bars), g)
        assert np.array_equal(dp.eval_pullback(pcof, states_bar=sb, history_precomputed=True), p0)
        assert np.array_equal(dp.eval_dense_states(refine, pcof, history_precomputed=True), d0)
        assert np.array_equal(dp.eval_dense_pullback(refine, pcof, history_precomputed=True, **bars), g)
        # eval_hessian_vec around it; the product itself is what it is without the pullbacks
        v = rng.standard_normal(len(pcof))
        hv = dp.eval_hessian_vec(pcof, v)
        assert np.array_equal(dp.eval_dense_pullback(refine, pcof, history_precomputed=True, **bars), g)
        assert np.array_equal(dp.eval_hessian_vec(pcof, v), hv)
        assert np.array_equal(dp.eval_dense_pullback(refine, pcof, **bars), g)
        fresh = _handle(qgd, prob, ctrl, target, order)
        try:
            assert np.array_equal(fresh.eval_hessian_vec(pcof, v), hv)
        finally:
            fresh.close()
        # another refine, other upload lengths, and back: the pool is made anew under its key
        other = _bars(prob, rng, 2, n_obs=1)
        assert np.all(np.isfinite(dp.eval_dense_pullback(2, pcof, states_bar=other["states_bar"])))
        assert np.array_equal(dp.eval_dense_pullback(refine, pcof, **bars), g)
        assert np.array_equal(qgd.eval_dense_pullback(prob, ctrl, pcof, order=order, refine=refine, **bars), g)
        qgd.clear_cache()
    finally:
        dp.close()


# -- 5: the memory budget ----------------------------------------------------------------------------------------------------------

def test_a_refused_pool_leaves_the_handle_usable(qgd):
    """Under a budget that holds the grid and the interpolated panels, the planes of enough observables do not fit the call's own
    pool: QGD_ERR_MEMORY before anything is launched."""
    L = qgd._lib
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    N, c, refine = prob.N_tot_levels, prob.N_initial_conditions, 3
    slots = 1 + prob.nsteps * refine
    sb = np.random.default_rng(14).standard_normal((2 * N, slots, c))
    dp = qgd.DeviceProblem(prob, 4)
    window = dp.memory_plan()["window_bytes"]
    dp.set_memory_budget(8 * window)
    dp.set_controls(ctrl); dp.set_target(target)
    try:
        budget = dp.memory_plan()["budget"]
        assert dp.memory_plan()["windows"] == 1 and budget == 8 * window
        g0, o0 = dp.discrete_adjoint(pcof)
        p0 = dp.eval_dense_pullback(refine, pcof, states_bar=sb)
        n_obs = 1 + budget // (8 * N * N)             # real planes [N, N, n_obs] that alone exceed the budget
        obs = np.broadcast_to(np.eye(N), (n_obs, N, N))
        with pytest.raises(L.QGDError) as ei:
            dp.eval_dense_pullback(refine, pcof, expectations_bar=np.ones((n_obs, slots, c)), observables=obs)
        msg = dp.lib.qgd_last_error(dp.h).decode()
        assert ei.value.code == L.QGD_ERR_MEMORY and "qgd_eval_dense_pullback" in msg, msg
        need = int(re.search(r"\((\d+) bytes needed\)", msg).group(1))
        print(f"\nguarded: window {window} bytes, budget {budget}, the refused dense pullback needs {need}")
        assert window < budget < need
        g1, o1 = dp.discrete_adjoint(pcof)
        assert np.array_equal(g1, g0) and np.array_equal(o1, o0)
        assert np.array_equal(dp.eval_dense_pullback(refine, pcof, states_bar=sb), p0)
        fresh = _handle(qgd, prob, ctrl, target, 4)
        try:
            assert np.array_equal(fresh.eval_dense_pullback(refine, pcof, states_bar=sb), p0)
        finally:
            fresh.close()
    finally:
        dp.close()


# -- 6: refusals -------------------------------------------------------------------------------------------------------------------

def _raw(dp, pcof, refine=2, sb=None, pb=None, lm=None, ng=0, eb=None, re=None, im=None, n_obs=0, grad=None, hp=0, n=None):
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    pc = None if pcof is None else np.ascontiguousarray(pcof, dtype=np.float64)
    rc = dp.lib.qgd_eval_dense_pullback(dp.h, vp(pc), (0 if pc is None else len(pc)) if n is None else n, hp, refine, vp(sb), vp(pb),
                                        vp(lm), ng, vp(eb), vp(re), vp(im), n_obs, vp(grad))
    return rc, dp.lib.qgd_last_error(dp.h).decode()


def test_refusals(qgd):
    L = qgd._lib
    A, S, U = L.QGD_ERR_ARGUMENT, L.QGD_ERR_STATE, L.QGD_ERR_UNSUPPORTED
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    N, c, slots = prob.N_tot_levels, prob.N_initial_conditions, 1 + 2 * prob.nsteps
    sb, pbar, eb = np.ones((2 * N, slots, c), order="F"), np.ones((N, slots, c), order="F"), np.ones((1, slots, c), order="F")
    lm, re_ = np.ones((1, N), order="F"), np.asfortranarray(np.eye(N)[:, :, None])
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        dp.discrete_adjoint(pcof)
        g0, o0 = dp.discrete_adjoint(pcof, history_precomputed=True)
        grad = np.full(len(pcof), np.nan)
        for what, kw, code in (("all three cotangents NULL", dict(grad=grad), A),
                               ("NULL grad", dict(sb=sb), A),
                               ("level_map with n_groups < 1", dict(pb=pbar[:1].copy(order="F"), lm=lm, ng=0, grad=grad), A),
                               ("expect_bar without obs_re", dict(eb=eb, n_obs=1, grad=grad), A),
                               ("expect_bar with n_obs < 1", dict(eb=eb, re=re_, n_obs=0, grad=grad), A),
                               ("a pcof of another length", dict(sb=sb, grad=grad, n=len(pcof) - 1), A),
                               ("refine = 0", dict(sb=sb, grad=grad, refine=0), A),
                               ("refine < 0", dict(sb=sb, grad=grad, refine=-2), A),
                               ("1 + nsteps * refine beyond int32", dict(sb=sb, grad=grad, refine=2 ** 28), A)):
            rc, msg = _raw(dp, pcof, **kw)
            assert rc == code and msg, (what, rc, msg)
            assert np.all(np.isnan(grad)), what
            # nothing was launched: the stored sweep and lambda are as the gradient call left them
            g1, o1 = dp.discrete_adjoint(pcof, history_precomputed=True)
            assert np.array_equal(g1, g0) and np.array_equal(o1, o0), what
        rc, msg = _raw(dp, pcof, sb=sb, grad=grad)
        assert rc == L.QGD_OK and np.all(np.isfinite(grad))
        assert np.array_equal(grad, dp.eval_dense_pullback(2, pcof, states_bar=sb))
    finally:
        dp.close()
    # no control basis; history_precomputed on a handle that has evaluated nothing
    dp = qgd.DeviceProblem(prob, 4)
    try:
        grad = np.full(len(pcof), np.nan)
        rc, msg = _raw(dp, pcof, sb=sb, grad=grad)
        assert rc == S and "qgd_set_control_basis" in msg
        dp.set_controls(ctrl)
        rc, msg = _raw(dp, pcof, sb=sb, grad=grad, hp=1)
        assert rc == S and "history_precomputed" in msg and np.all(np.isnan(grad))
        with pytest.raises(qgd._lib.QGDError) as ei:
            dp.eval_dense_pullback(2, pcof, states_bar=sb, history_precomputed=True)
        assert ei.value.code == S
        rc, msg = _raw(dp, pcof, sb=sb, grad=grad)
        assert rc == L.QGD_OK and np.all(np.isfinite(grad))
    finally:
        dp.close()
    # a partitioned handle
    rank = qgd.DeviceBackend(prob, 4, ctrl, target, 0, 2)
    try:
        grad = np.full(len(pcof), np.nan)
        rc, msg = _raw(rank.dp, pcof, sb=sb, grad=grad)
        assert rc == S and "partitioned" in msg and np.all(np.isnan(grad))
    finally:
        rank.dp.close()
    # a windowed grid: a budget small enough for two windows
    prob2, ctrl2, pcof2, target2 = cases.cnot2_case(qgd, nsteps=100, tf=100.0)
    dp = qgd.DeviceProblem(prob2, 4)
    dp.set_memory_budget(dp.memory_plan()["window_bytes"] // 3)
    dp.set_controls(ctrl2); dp.set_target(target2)
    try:
        assert dp.memory_plan()["windows"] >= 2
        g0 = dp.discrete_adjoint(pcof2)[0]
        grad = np.full(len(pcof2), np.nan)
        rc, msg = _raw(dp, pcof2, sb=np.ones((2 * prob2.N_tot_levels, 201, prob2.N_initial_conditions), order="F"), grad=grad)
        assert rc == U and "windows" in msg and np.all(np.isnan(grad))
        assert np.array_equal(dp.discrete_adjoint(pcof2)[0], g0)
    finally:
        dp.close()
    # N > 64: the smallest such case of cases.py
    prob3, ctrl3, pcof3, target3 = cases.synthetic_case(qgd, nsteps=4)
    dp = _handle(qgd, prob3, ctrl3, target3, 4)
    try:
        g0 = dp.discrete_adjoint(pcof3)[0]
        grad = np.full(len(pcof3), np.nan)
        rc, msg = _raw(dp, pcof3, sb=np.ones((2 * prob3.N_tot_levels, 9, prob3.N_initial_conditions), order="F"), grad=grad)
        assert rc == U and "N <= 64" in msg and np.all(np.isnan(grad))
        assert np.array_equal(dp.discrete_adjoint(pcof3)[0], g0)
    finally:
        dp.close()
    # no control operators
    prob4 = qgd.construct_rand_prob(4, 0, tf=0.1, nsteps=6)
    dp = qgd.DeviceProblem(prob4, 4)
    try:
        dp.set_controls([])
        grad = np.zeros(1)
        rc, msg = _raw(dp, None, sb=np.ones((8, 13, prob4.N_initial_conditions), order="F"), grad=grad)
        assert rc == U and "control operators" in msg
    finally:
        dp.close()
