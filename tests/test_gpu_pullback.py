"""GPU tests of qgd_eval_pullback: the pullback of the trajectory outputs -- states, level populations,
expectation values -- to pcof.  Built in stages, each against code that was there before: the states part against
discrete_adjoint's terminal costs and guard penalty, the populations and expectations parts against the states part with the
cotangent formed on the host, all three against differences of the device's own output calls.

Bound where two formulations of the same gradient are compared: the project's 1e-10 max(1, max|g|).  Differences: steps and
bound of test_gpu_hvp.py::test_hvp_matches_gradient_differences (h = 1e-3 and 5e-4 extrapolated, 1e-8 of the difference
quotient).  The measured figures are in DESIGN.md section 4g."""
import ctypes as C

import numpy as np
import pytest

import cases
from test_gpu_hessian import _case, _handle
from test_gpu_hvp import _paths

pytestmark = pytest.mark.gpu


def _bound(g):
    return 1e-10 * max(1.0, np.abs(g).max())


def _close(g, ref, what):
    err, bound = np.abs(g - ref).max(), _bound(ref)
    print(f"\n{what}: max|g - ref| = {err:.3e}, bound {bound:.3e}, max|ref| = {np.abs(ref).max():.3e}")
    assert np.all(np.isfinite(g)), what
    assert err <= bound, what


def _hermitian(rng, n_obs, N, complex_=True):
    a = rng.standard_normal((n_obs, N, N)) + (1j * rng.standard_normal((n_obs, N, N)) if complex_ else 0.0)
    return a + np.conj(np.transpose(a, (0, 2, 1)))


def _host_expect_bar(w, eb, obs):
    """2 sum_j ebar_j [A u - B v; A v + B u] as a cotangent of the states w [2N, slots, c]"""
    N = w.shape[0] // 2
    psi = w[:N] + 1j * w[N:]
    z = 2.0 * np.einsum("jkc,jil,lkc->ikc", eb, np.asarray(obs, dtype=complex), psi)
    return np.asfortranarray(np.concatenate([z.real, z.imag]))


def _trap(nt):
    t = np.ones(nt); t[0] = t[-1] = 0.5
    return t


def _guard_bar(prob, w):
    """(2 dt / tf) trap_n W w_n: the guard penalty's derivative with respect to the states"""
    nt = w.shape[1]
    W = np.asarray(prob.guard_subspace_projector)
    return (2.0 / (nt - 1)) * _trap(nt)[None, :, None] * np.einsum("ij,jkc->ikc", W, w)


# -- 1: the states part against the terminal costs ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cnot2", "rand4"])
@pytest.mark.parametrize("cost_type", ["Tracking", "Norm"])
def test_states_pullback_is_the_terminal_cost_gradient(qgd, name, cost_type):
    prob, ctrl, pcof, target = _case(qgd, name)
    assert not np.any(np.asarray(prob.guard_subspace_projector))
    dp = _handle(qgd, prob, ctrl, target, 4, cost_type)
    try:
        for path in _paths(qgd, dp):
            g_ref = dp.discrete_adjoint(pcof)[0]
            w = dp.eval_states(pcof)
            sb = np.zeros_like(w)
            sb[:, -1] = w[:, -1] - (qgd.complex_to_real(target) if cost_type == "Tracking" else 0.0)
            _close(dp.eval_pullback(pcof, states_bar=sb), g_ref, f"{name} {cost_type} {path}: states pullback vs discrete_adjoint")
    finally:
        dp.close()


# -- 2: the states part against the guard penalty --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["guarded", "dense_guard"])
def test_states_pullback_is_the_guard_gradient(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    dp = _handle(qgd, prob, ctrl, target, 6, "Norm")
    try:
        for path in _paths(qgd, dp):
            g_ref = dp.discrete_adjoint(pcof)[0]
            w = dp.eval_states(pcof)
            sb = _guard_bar(prob, w)
            sb[:, 0] = 1e3                      # the n = 0 rule: whatever slot 0 holds is ignored
            sb[:, -1] += w[:, -1]
            _close(dp.eval_pullback(pcof, states_bar=sb), g_ref, f"{name} Norm {path}: states pullback vs discrete_adjoint with guard")
    finally:
        dp.close()


# -- 3: populations against states ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cnot2", "guarded"])
def test_populations_pullback_against_states(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    rng = np.random.default_rng(21)
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        for path in _paths(qgd, dp):
            w = dp.eval_states(pcof)
            pbar = rng.standard_normal((N, nt, c))
            ref = dp.eval_pullback(pcof, states_bar=2.0 * np.concatenate([pbar, pbar]) * w)
            _close(dp.eval_pullback(pcof, populations_bar=pbar), ref, f"{name} {path}: populations vs states")
            for G in (1, 5):
                lm, pg = rng.standard_normal((G, N)), rng.standard_normal((G, nt, c))
                wl = np.einsum("gl,gkc->lkc", lm, pg)
                ref = dp.eval_pullback(pcof, states_bar=2.0 * np.concatenate([wl, wl]) * w)
                _close(dp.eval_pullback(pcof, populations_bar=pg, level_map=lm), ref, f"{name} {path}: populations with a {G}-row map vs states")
    finally:
        dp.close()


def test_populations_pullback_is_the_diagonal_guard_gradient(qgd):
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    W = np.asarray(prob.guard_subspace_projector)
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    assert not np.any(W - np.diag(np.diag(W))) and np.array_equal(np.diag(W)[:N], np.diag(W)[N:]) and np.any(W)
    dp = _handle(qgd, prob, ctrl, target, 6, "Norm")
    try:
        w = dp.eval_states(pcof)
        ref = dp.eval_pullback(pcof, states_bar=_guard_bar(prob, w))
        pbar = (1.0 / (nt - 1)) * _trap(nt)[None, :, None] * np.diag(W)[:N, None, None] * np.ones((N, nt, c))
        _close(dp.eval_pullback(pcof, populations_bar=pbar), ref, "guarded: populations with (dt/tf) trap W_kk vs the guard part")
        full = dp.discrete_adjoint(pcof)[0]
        sb = np.zeros_like(w); sb[:, -1] = w[:, -1]
        _close(dp.eval_pullback(pcof, populations_bar=pbar, states_bar=sb), full, "guarded: populations + terminal states vs discrete_adjoint")
    finally:
        dp.close()


# -- 4: expectations against states ---------------------------------------------------------------------------------------------

def _expectations_case(qgd, dp, prob, pcof, label, n_obs_list=(1, 5)):
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    rng = np.random.default_rng(31)
    w = dp.eval_states(pcof)
    for n_obs in n_obs_list:
        for kind in ("real", "complex"):
            obs = _hermitian(rng, n_obs, N, kind == "complex")
            eb = rng.standard_normal((n_obs, nt, c))
            ref = dp.eval_pullback(pcof, states_bar=_host_expect_bar(w, eb, obs))
            _close(dp.eval_pullback(pcof, expectations_bar=eb, observables=obs), ref, f"{label}: {n_obs} {kind} observables vs states")
    d, eb = rng.standard_normal(N), rng.standard_normal((1, nt, c))
    _close(dp.eval_pullback(pcof, expectations_bar=eb, observables=np.diag(d)), dp.eval_pullback(pcof, populations_bar=eb, level_map=d[None]),
           f"{label}: a real diagonal observable vs populations with a one-row map")


@pytest.mark.parametrize("name", ["cnot2", "guarded"])      # guarded: N = 9 (no multiple of 4), 4 columns (no multiple of 8)
def test_expectations_pullback_against_states(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    if name == "guarded":
        assert prob.N_tot_levels % 4 and prob.N_initial_conditions % 8
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        for path in _paths(qgd, dp):
            _expectations_case(qgd, dp, prob, pcof, f"{name} {path}")
    finally:
        dp.close()


def test_expectations_pullback_full_tile(qgd):
    """N = 64: cnot3, the sparse path, every row of the 64-row tile"""
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=20, tf=20.0)
    dp = _handle(qgd, prob, ctrl, target, 8)
    try:
        assert prob.N_tot_levels == 64 and dp.operator_path()[0] == "sparse"
        _expectations_case(qgd, dp, prob, pcof, "cnot3 sparse")
    finally:
        dp.close()


def test_expectations_planes_in_lds_and_from_l2_give_the_same_bits(qgd, monkeypatch):
    """120 complex observables at N = 9 exceed the LDS (2 x 120 planes of 1.5 KB in fragment order): the planes are read from
    L2.  The same call with QGD_PATHS=planes_l2 sends a batch that fits down the same route: the bits of the LDS route."""
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    rng = np.random.default_rng(41)
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        w = dp.eval_states(pcof)
        obs, eb = _hermitian(rng, 120, N), rng.standard_normal((120, nt, c))
        _close(dp.eval_pullback(pcof, expectations_bar=eb, observables=obs), dp.eval_pullback(pcof, states_bar=_host_expect_bar(w, eb, obs)),
               "guarded: 120 complex observables (planes from L2) vs states")
        g_lds = dp.eval_pullback(pcof, expectations_bar=eb[:5], observables=obs[:5])
        monkeypatch.setenv("QGD_PATHS", "planes_l2")
        g_l2 = dp.eval_pullback(pcof, expectations_bar=eb[:5], observables=obs[:5])
        monkeypatch.delenv("QGD_PATHS")
        assert np.array_equal(g_lds, g_l2)
    finally:
        dp.close()


# -- 5: differences of the device's own outputs -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rand4", "guarded", "dense_guard"])
def test_pullback_matches_differences_of_the_outputs(qgd, name):
    order = 4
    prob, ctrl, pcof, target = _case(qgd, name)
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    rng = np.random.default_rng(5)
    obs, lm = _hermitian(rng, 3, N), rng.standard_normal((3, N))
    sb, pb, eb = rng.standard_normal((2 * N, nt, c)), rng.standard_normal((3, nt, c)), rng.standard_normal((3, nt, c))
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        g = dp.eval_pullback(pcof, states_bar=sb, populations_bar=pb, level_map=lm, expectations_bar=eb, observables=obs)
        parts = (dp.eval_pullback(pcof, states_bar=sb) + dp.eval_pullback(pcof, populations_bar=pb, level_map=lm)
                 + dp.eval_pullback(pcof, expectations_bar=eb, observables=obs))
        _close(g, parts, f"{name}: the three parts at once vs their sum")

        def J(p):
            return (np.sum(sb * dp.eval_states(p)) + np.sum(pb * dp.eval_populations(p, level_map=lm))
                    + np.sum(eb * dp.eval_expectations(obs, p)))
        for _ in range(2):
            d = rng.standard_normal(len(pcof)); d /= np.linalg.norm(d)

            def fd(h):
                return (J(pcof + h * d) - J(pcof - h * d)) / (2 * h)
            F = (4 * fd(5e-4) - fd(1e-3)) / 3
            err = abs(g @ d - F)
            print(f"\n{name}: |g.d - fd| = {err:.3e}, |fd| = {abs(F):.3e}")
            assert err <= 1e-8 * abs(F)
    finally:
        dp.close()


# -- 6: addressing ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rand4", "guarded"])
def test_save_every_addresses_the_time_points_of_its_slots(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    N, c, S = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps
    assert S % 3
    slots = 1 + S // 3
    rng = np.random.default_rng(6)
    obs, lm = _hermitian(rng, 2, N), rng.standard_normal((2, N))
    bars = dict(states_bar=rng.standard_normal((2 * N, slots, c)), populations_bar=rng.standard_normal((2, slots, c)),
                expectations_bar=rng.standard_normal((2, slots, c)))
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        dp.set_save_every(3)
        g3 = dp.eval_pullback(pcof, level_map=lm, observables=obs, **bars)
        with pytest.raises(ValueError):
            dp.eval_pullback(pcof, states_bar=np.zeros((2 * N, S + 1, c)))
        dp.set_save_every(1)
        wide = {}
        for key, b in bars.items():
            wide[key] = np.zeros((b.shape[0], S + 1, c)); wide[key][:, ::3][:, :slots] = b
        g1 = dp.eval_pullback(pcof, level_map=lm, observables=obs, **wide)
        print(f"\n{name}: save_every 3 vs 1 bitwise equal: {np.array_equal(g3, g1)}")
        _close(g3, g1, f"{name}: save_every = 3 vs the zero-filled save_every = 1 call")
        assert np.abs(g3).max() > 0
    finally:
        dp.close()


# -- 7: reproducibility and the stored sweep ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cnot2", "guarded"])
def test_reproducible_and_leaves_the_stored_sweep_usable(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    rng = np.random.default_rng(7)
    obs, lm = _hermitian(rng, 3, N), rng.standard_normal((2, N))
    bars = dict(states_bar=rng.standard_normal((2 * N, nt, c)), populations_bar=rng.standard_normal((2, nt, c)), level_map=lm,
                expectations_bar=rng.standard_normal((3, nt, c)), observables=obs)
    order = 4
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        g = dp.eval_pullback(pcof, **bars)
        for _ in range(2):
            assert np.array_equal(dp.eval_pullback(pcof, **bars), g)
        assert np.array_equal(dp.eval_pullback(pcof, history_precomputed=True, **bars), g)
        dp.set_timing(1)
        dp.eval_pullback(pcof, history_precomputed=True, **bars)
        names = set(dp.timings())
        dp.set_timing(0)
        assert "pullback_forcing" in names and "pullback_adjoint" in names and not (names & {"sweep_forward", "build_LR", "derivs"}), names
        # another pcof under history_precomputed: the sweep is redone
        fresh = _handle(qgd, prob, ctrl, target, order)
        try:
            assert np.array_equal(dp.eval_pullback(0.5 * pcof, history_precomputed=True, **bars), fresh.eval_pullback(0.5 * pcof, **bars))
        finally:
            fresh.close()
        # discrete_adjoint -> pullback -> discrete_adjoint(history_precomputed): the first gradient's bits; populations and
        # expectations from the stored sweep as before
        g0, o0 = dp.discrete_adjoint(pcof)
        p0, e0 = dp.eval_populations(pcof), dp.eval_expectations(obs, pcof)
        assert np.array_equal(dp.eval_pullback(pcof, **bars), g)
        g1, o1 = dp.discrete_adjoint(pcof, history_precomputed=True)
        assert np.array_equal(g1, g0) and np.array_equal(o1, o0)
        assert np.array_equal(dp.eval_pullback(pcof, history_precomputed=True, **bars), g)
        assert np.array_equal(dp.eval_populations(pcof, history_precomputed=True), p0)
        assert np.array_equal(dp.eval_expectations(obs, pcof, history_precomputed=True), e0)
        # pullback -> eval_hessian_vec -> pullback; the product itself is what it is without pullbacks around it
        v = rng.standard_normal(len(pcof))
        hv = dp.eval_hessian_vec(pcof, v)
        assert np.array_equal(dp.eval_pullback(pcof, history_precomputed=True, **bars), g)
        assert np.array_equal(dp.eval_hessian_vec(pcof, v), hv)
        assert np.array_equal(dp.eval_pullback(pcof, **bars), g)
        fresh = _handle(qgd, prob, ctrl, target, order)
        try:
            assert np.array_equal(fresh.eval_hessian_vec(pcof, v), hv)
        finally:
            fresh.close()
    finally:
        dp.close()


def test_without_a_target_and_with_tables_set_directly(qgd):
    from qgd_amd.controls import control_tables_general
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    order = 4
    rng = np.random.default_rng(8)
    bars = dict(states_bar=rng.standard_normal((2 * N, nt, c)), expectations_bar=rng.standard_normal((2, nt, c)),
                observables=_hermitian(rng, 2, N))
    with_target = _handle(qgd, prob, ctrl, target, order)
    dp = qgd.DeviceProblem(prob, order)
    try:
        dp.set_controls(ctrl)                                # no target on this handle
        g = dp.eval_pullback(pcof, **bars)
        assert np.array_equal(g, with_target.eval_pullback(pcof, **bars))
        # tables set directly, pcof = None: the basis on the handle is the Jacobian
        p, q, _, _ = control_tables_general(ctrl, np.asarray(pcof, float), prob.nsteps, prob.tf, order // 2)
        dp.set_control_tables(p, q)
        _close(dp.eval_pullback(None, **bars), g, "guarded: tables set directly (pcof = None) vs pcof")
        # a control that is not linear in its coefficients goes the same way (tables + Jacobian uploaded by the Python layer)
        gen = qgd.DeviceProblem(prob, order)
        try:
            gen.set_controls([cases.PointwiseOnly(cc) for cc in ctrl])
            _close(gen.eval_pullback(pcof, **bars), g, "guarded: pointwise-protocol controls vs the basis path")
        finally:
            gen.close()
        assert np.array_equal(qgd.eval_pullback(prob, ctrl, pcof, order=order, **bars), g)
        qgd.clear_cache()
    finally:
        dp.close(); with_target.close()


# -- 8: refusals -----------------------------------------------------------------------------------------------------------------

def _raw(dp, pcof, sb=None, pb=None, lm=None, ng=0, eb=None, re=None, im=None, n_obs=0, grad=None, hp=0, n=None):
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    pc = None if pcof is None else np.ascontiguousarray(pcof, dtype=np.float64)
    rc = dp.lib.qgd_eval_pullback(dp.h, vp(pc), (0 if pc is None else len(pc)) if n is None else n, hp, vp(sb), vp(pb), vp(lm), ng,
                                  vp(eb), vp(re), vp(im), n_obs, vp(grad))
    return rc, dp.lib.qgd_last_error(dp.h).decode()


def test_refusals(qgd):
    L = qgd._lib
    A, S, U = L.QGD_ERR_ARGUMENT, L.QGD_ERR_STATE, L.QGD_ERR_UNSUPPORTED
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    sb, pb, eb = np.ones((2 * N, nt, c), order="F"), np.ones((N, nt, c), order="F"), np.ones((1, nt, c), order="F")
    lm, re = np.ones((1, N), order="F"), np.asfortranarray(np.eye(N)[:, :, None])
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        dp.discrete_adjoint(pcof)
        g0, o0 = dp.discrete_adjoint(pcof, history_precomputed=True)
        grad = np.full(len(pcof), np.nan)
        for what, kw, code in (("all three cotangents NULL", dict(grad=grad), A),
                               ("NULL grad", dict(sb=sb), A),
                               ("level_map with n_groups < 1", dict(pb=pb[:1].copy(order="F"), lm=lm, ng=0, grad=grad), A),
                               ("expect_bar without obs_re", dict(eb=eb, n_obs=1, grad=grad), A),
                               ("expect_bar with n_obs < 1", dict(eb=eb, re=re, n_obs=0, grad=grad), A),
                               ("a pcof of another length", dict(sb=sb, grad=grad, n=len(pcof) - 1), A)):
            rc, msg = _raw(dp, pcof, **kw)
            assert rc == code and msg, (what, rc, msg)
            assert np.all(np.isnan(grad)), what
            # nothing was launched: the stored sweep and lambda are as the gradient call left them
            g1, o1 = dp.discrete_adjoint(pcof, history_precomputed=True)
            assert np.array_equal(g1, g0) and np.array_equal(o1, o0), what
        rc, msg = _raw(dp, pcof, sb=sb, grad=grad)
        assert rc == L.QGD_OK and np.all(np.isfinite(grad))
    finally:
        dp.close()
    # history_precomputed on a handle that has evaluated nothing; no control basis
    dp = qgd.DeviceProblem(prob, 4)
    try:
        grad = np.full(len(pcof), np.nan)
        rc, msg = _raw(dp, pcof, sb=sb, grad=grad)
        assert rc == S and "qgd_set_control_basis" in msg
        dp.set_controls(ctrl)
        rc, msg = _raw(dp, pcof, sb=sb, grad=grad, hp=1)
        assert rc == S and "history_precomputed" in msg and np.all(np.isnan(grad))
        with pytest.raises(qgd._lib.QGDError) as ei:
            dp.eval_pullback(pcof, states_bar=sb, history_precomputed=True)
        assert ei.value.code == S
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
        rc, msg = _raw(dp, pcof2, sb=np.ones((2 * prob2.N_tot_levels, 101, prob2.N_initial_conditions), order="F"), grad=grad)
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
        rc, msg = _raw(dp, pcof3, sb=np.ones((2 * prob3.N_tot_levels, 5, prob3.N_initial_conditions), order="F"), grad=grad)
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
        rc, msg = _raw(dp, None, sb=np.ones((8, 7, prob4.N_initial_conditions), order="F"), grad=grad)
        assert rc == U and "control operators" in msg
    finally:
        dp.close()
