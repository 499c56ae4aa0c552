"""GPU tests of qgd_eval_pushforward: J v, the directional derivatives of the trajectory outputs --
states, level populations, expectation values -- along directions v in pcof.  Built in stages, each against code that was there
before: the states tangent against discrete_adjoint's terminal costs and guard penalty, the populations and expectations
tangents against their formulas on the host from eval_states and the states tangent, all three against eval_pullback (duality)
and against differences of the device's own output calls; then what is bitwise: runs, scaling, slot 0, directions side by
side against one by one, chunks, the two routes of the map and the planes, save_every; what the call leaves of the stored
evaluation; the refusals.

Bounds.  Two formulations of one directional derivative <g, v>: the project's 1e-10 max(1, max|g|) of a gradient entry, times
|v|_1 (each entry of g enters with weight v_l).  An output against its formula on the host: 1e-10 max(1, max|ref|).
Differences: h = 1e-3 and 5e-4 extrapolated, 1e-8 of the difference quotient, on the scalar <ybar, output>.  The measured
figures are in DESIGN.md section 4l."""
import ctypes as C

import numpy as np
import pytest

import cases
import qgd_hooks
from test_gpu_hessian import _case, _handle
from test_gpu_hvp import _FORWARD_PHASES, _paths
from test_gpu_pullback import _guard_bar, _hermitian

pytestmark = pytest.mark.gpu


def _dual(jv, gv, g, v, what):
    err, bound = abs(jv - gv), 1e-10 * max(1.0, np.abs(g).max()) * np.abs(v).sum()
    print(f"\n{what}: |<ybar, J v> - <g, v>| = {err:.3e}, bound {bound:.3e}, |<g, v>| = {abs(gv):.3e}")
    assert np.isfinite(jv) and err <= bound, what


def _close(x, ref, what):
    err, bound = np.abs(x - ref).max(), 1e-10 * max(1.0, np.abs(ref).max())
    print(f"\n{what}: max|x - ref| = {err:.3e}, bound {bound:.3e}, max|ref| = {np.abs(ref).max():.3e}")
    assert np.all(np.isfinite(x)) and err <= bound, what


def _directions(rng, pcof, n_vec=None):
    return rng.standard_normal(len(pcof) if n_vec is None else (len(pcof), n_vec))


def _bars(rng, prob, slots, n_obs=3, n_groups=4):
    N, c = prob.N_tot_levels, prob.N_initial_conditions
    return dict(states_bar=rng.standard_normal((2 * N, slots, c)), populations_bar=rng.standard_normal((n_groups, slots, c)),
                level_map=rng.standard_normal((n_groups, N)), expectations_bar=rng.standard_normal((n_obs, slots, c)),
                observables=_hermitian(rng, n_obs, N))


def _all(dp, pcof, v, bars, **kw):
    return dp.eval_pushforward(pcof, v, states=True, level_map=bars["level_map"], observables=bars["observables"], **kw)


KINDS = (("states", "states_bar", ()), ("populations", "populations_bar", ("level_map",)),
         ("expectations", "expectations_bar", ("observables",)))


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


# -- 1: the states tangent against the oracle-pinned gradient -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cnot2", "rand4"])
@pytest.mark.parametrize("cost_type", ["Tracking", "Norm"])
def test_states_tangent_against_the_terminal_cost_gradient(qgd, name, cost_type):
    prob, ctrl, pcof, target = _case(qgd, name)
    assert not np.any(np.asarray(prob.guard_subspace_projector))
    v = _directions(np.random.default_rng(101), pcof)
    dp = _handle(qgd, prob, ctrl, target, 4, cost_type)
    try:
        for path in _paths(qgd, dp):
            g = dp.discrete_adjoint(pcof)[0]
            w = dp.eval_states(pcof)
            cot = np.zeros_like(w)
            cot[:, -1] = w[:, -1] - (qgd.complex_to_real(target) if cost_type == "Tracking" else 0.0)
            sd = dp.eval_pushforward(pcof, v, states=True)["states"]
            assert sd.shape == w.shape
            _dual(np.sum(cot * sd), g @ v, g, v, f"{name} {cost_type} {path}: <dcost/dw, states_dot> vs v . discrete_adjoint")
    finally:
        dp.close()


@pytest.mark.parametrize("name", ["guarded", "dense_guard"])
def test_states_tangent_against_the_guard_gradient(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    v = _directions(np.random.default_rng(102), pcof)
    dp = _handle(qgd, prob, ctrl, target, 6, "Norm")
    try:
        for path in _paths(qgd, dp):
            g = dp.discrete_adjoint(pcof)[0]
            w = dp.eval_states(pcof)
            cot = _guard_bar(prob, w)
            cot[:, -1] += w[:, -1]
            sd = dp.eval_pushforward(pcof, v, states=True)["states"]
            _dual(np.sum(cot * sd), g @ v, g, v, f"{name} Norm {path}: <dcost/dw, states_dot> vs v . discrete_adjoint with guard")
    finally:
        dp.close()


# -- 2: populations and expectations against the states tangent -----------------------------------------------------------------

def _host_tangents(w, sd, level_map=None, observables=None):
    """pop_dot and expect_dot by their formulas from the states w [2N, slots, c] and the states tangent sd [2N, slots, c, n_vec]"""
    N = w.shape[0] // 2
    pop = 2.0 * (w[:N, :, :, None] * sd[:N] + w[N:, :, :, None] * sd[N:])
    if level_map is not None:
        pop = np.einsum("gl,lkcd->gkcd", level_map, pop)
    ex = None
    if observables is not None:
        psi, dpsi = w[:N] + 1j * w[N:], sd[:N] + 1j * sd[N:]
        ex = 2.0 * np.einsum("ikc,jil,lkcd->jkcd", np.conj(psi), np.asarray(observables, dtype=complex), dpsi).real
    return pop, ex


def _outputs_case(qgd, dp, prob, pcof, label):
    N = prob.N_tot_levels
    rng = np.random.default_rng(201)
    V = _directions(rng, pcof, 3)
    w = dp.eval_states(pcof)
    sd = dp.eval_pushforward(pcof, V, states=True)["states"]
    lm, oc, orl = rng.standard_normal((4, N)), _hermitian(rng, 2, N), _hermitian(rng, 1, N, False)
    out = dp.eval_pushforward(pcof, V, populations=True, observables=oc)
    pop, ex = _host_tangents(w, sd, None, oc)
    _close(out["populations"], pop, f"{label}: pop_dot vs 2 (u du + v dv)")
    _close(out["expectations"], ex, f"{label}: expect_dot of 2 complex observables vs 2 Re(psi^H O dpsi)")
    out = dp.eval_pushforward(pcof, V, level_map=lm, observables=orl)
    pop, ex = _host_tangents(w, sd, lm, orl)
    _close(out["populations"], pop, f"{label}: pop_dot with a 4-row map vs the host contraction")
    _close(out["expectations"], ex, f"{label}: expect_dot of 1 real observable vs 2 Re(psi^H O dpsi)")
    assert out["populations"].shape == (4,) + w.shape[1:] + (3,) and out["expectations"].shape == (1,) + w.shape[1:] + (3,)


@pytest.mark.parametrize("name", ["cnot2", "guarded"])      # guarded: N = 9 (no multiple of 4), 4 columns (no multiple of 8)
def test_populations_and_expectations_tangents_against_the_states_tangent(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        for path in _paths(qgd, dp):
            _outputs_case(qgd, dp, prob, pcof, f"{name} {path}")
    finally:
        dp.close()


def test_populations_and_expectations_tangents_full_tile(qgd):
    """N = 64, 8 columns: cnot3, every row of the 64-row tile and every column of the group"""
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=20, tf=20.0)
    dp = _handle(qgd, prob, ctrl, target, 8)
    try:
        assert prob.N_tot_levels == 64 and prob.N_initial_conditions == 8
        _outputs_case(qgd, dp, prob, pcof, "cnot3")
    finally:
        dp.close()


# -- 3: duality with eval_pullback ------------------------------------------------------------------------------------------------

def _duality(qgd, dp, prob, pcof, label, seed=301, pcof_arg="same"):
    rng = np.random.default_rng(seed)
    bars = _bars(rng, prob, dp._slots())
    v = _directions(rng, pcof)
    pc = pcof if pcof_arg == "same" else pcof_arg
    out = _all(dp, pc, v, bars)
    for kind, bar, extra in KINDS:
        part = {bar: bars[bar], **{k: bars[k] for k in extra}}
        g = dp.eval_pullback(pc, **part)
        _dual(np.sum(bars[bar] * out[kind]), g @ v, g, v, f"{label}: {kind}")


@pytest.mark.parametrize("name,order", [("cnot2", 2), ("cnot2", 4), ("cnot2", 8), ("guarded", 6)])
def test_duality_with_the_pullback(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        for path in _paths(qgd, dp):
            _duality(qgd, dp, prob, pcof, f"{name} order {order} {path}")
    finally:
        dp.close()


# -- 4: differences of the device's own output calls -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rand4", "guarded", "dense_guard"])
def test_pushforward_matches_differences_of_the_outputs(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    rng = np.random.default_rng(401)
    bars = _bars(rng, prob, prob.nsteps + 1)
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        def J(p):
            return {"states": np.sum(bars["states_bar"] * dp.eval_states(p)),
                    "populations": np.sum(bars["populations_bar"] * dp.eval_populations(p, level_map=bars["level_map"])),
                    "expectations": np.sum(bars["expectations_bar"] * dp.eval_expectations(bars["observables"], p))}
        for _ in range(2):
            v = _directions(rng, pcof); v /= np.linalg.norm(v)
            out = _all(dp, pcof, v, bars)

            def fd(h):
                a, b = J(pcof + h * v), J(pcof - h * v)
                return {k: (a[k] - b[k]) / (2 * h) for k in a}
            f1, f2 = fd(1e-3), fd(5e-4)
            for kind, bar, _e in KINDS:
                F = (4 * f2[kind] - f1[kind]) / 3
                err = abs(np.sum(bars[bar] * out[kind]) - F)
                print(f"\n{name} {kind}: |<ybar, J v> - fd| = {err:.3e}, |fd| = {abs(F):.3e}, bound {1e-8 * abs(F):.3e}")
                assert err <= 1e-8 * abs(F), kind
    finally:
        dp.close()


# -- 5: what is bitwise -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cnot2", "guarded"])
def test_bitwise_runs_scaling_slot_zero_and_directions_side_by_side(qgd, name, monkeypatch):
    prob, ctrl, pcof, target = _case(qgd, name)
    rng = np.random.default_rng(501)
    bars = _bars(rng, prob, prob.nsteps + 1)
    V = _directions(rng, pcof, 5)
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        one = _all(dp, pcof, V[:, 0], bars)
        assert _same(_all(dp, pcof, V[:, 0], bars), one)
        assert _same(_all(dp, pcof, V[:, 0], bars, history_precomputed=True), one)
        two = _all(dp, pcof, 2.0 * V[:, 0], bars)
        for kind in one:
            assert one[kind].ndim == 3 and np.abs(one[kind]).max() > 0
            assert np.array_equal(two[kind], 2.0 * one[kind]), kind                    # J (2 v) == 2 J v exactly
            assert not one[kind][:, 0].any(), kind                                     # slot 0: exact zeros
        five = _all(dp, pcof, V, bars)
        singles = [_all(dp, pcof, V[:, j], bars) for j in range(5)]
        for kind in five:
            assert five[kind].shape == one[kind].shape + (5,)
            for j in range(5):
                assert np.array_equal(five[kind][..., j], singles[j][kind]), (kind, j)  # side by side == one by one
        # chunks of two directions (2 + 2 + 1), on a handle of its own: the knob is read when the handle is created
        monkeypatch.setenv("QGD_PUSHFORWARD_CHUNK", "2")
        ch = _handle(qgd, prob, ctrl, target, 4)
        monkeypatch.delenv("QGD_PUSHFORWARD_CHUNK")
        try:
            assert _same(_all(ch, pcof, V, bars), five)
            assert _same(_all(ch, pcof, V[:, :3], bars), {k: a[..., :3] for k, a in five.items()})      # 2 + 1: another width last
            assert _same(_all(ch, pcof, V, bars), five)
        finally:
            ch.close()
    finally:
        dp.close()


def test_map_and_planes_in_lds_and_from_l2_give_the_same_bits(qgd, monkeypatch):
    """130 complex observables at N = 9 exceed the LDS (2 x 130 planes of 648 bytes beside the tiles): they are read from L2.
    The same call with QGD_PATHS=planes_l2 sends a set that fits down the same route: the bits of the LDS route."""
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    N = prob.N_tot_levels
    rng = np.random.default_rng(502)
    V = _directions(rng, pcof, 2)
    obs, lm = _hermitian(rng, 130, N), rng.standard_normal((4, N))
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        w = dp.eval_states(pcof)
        sd = dp.eval_pushforward(pcof, V, states=True)["states"]
        big = dp.eval_pushforward(pcof, V, level_map=lm, observables=obs)
        pop, ex = _host_tangents(w, sd, lm, obs)
        _close(big["expectations"], ex, "guarded: 130 complex observables (planes from L2) vs the host formula")
        _close(big["populations"], pop, "guarded: the map beside them (from L2) vs the host contraction")
        lds = dp.eval_pushforward(pcof, V, level_map=lm, observables=obs[:5])
        monkeypatch.setenv("QGD_PATHS", "planes_l2")
        l2 = dp.eval_pushforward(pcof, V, level_map=lm, observables=obs[:5])
        monkeypatch.delenv("QGD_PATHS")
        assert _same(lds, l2)
        assert np.array_equal(lds["expectations"], big["expectations"][:5]) and np.array_equal(lds["populations"], big["populations"])
    finally:
        dp.close()


# -- 6: addressing ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rand4", "guarded"])
def test_save_every_three_is_every_third_slot_bit_for_bit(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    assert prob.nsteps == 10
    rng = np.random.default_rng(601)
    bars = _bars(rng, prob, 4)
    V = _directions(rng, pcof, 2)
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        every = _all(dp, pcof, V, bars)
        dp.set_save_every(3)
        third = _all(dp, pcof, V, bars)
        dp.set_save_every(1)
        for kind in every:
            assert third[kind].shape[1] == 4 and every[kind].shape[1] == 11
            assert np.array_equal(third[kind], every[kind][:, ::3]), kind
            assert np.abs(third[kind][:, 1:]).max() > 0
    finally:
        dp.close()


# -- 7: the stored evaluation ---------------------------------------------------------------------------------------------------

def _timed(dp, call):
    dp.set_timing(1)
    out = call()
    names = set(dp.timings())
    dp.set_timing(0)
    return out, names


@pytest.mark.parametrize("name", ["cnot2", "guarded"])
def test_leaves_the_stored_evaluation_and_the_hvp_setup_usable(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    order = 4
    rng = np.random.default_rng(701)
    bars = _bars(rng, prob, prob.nsteps + 1)
    V, hvv = _directions(rng, pcof, 2), _directions(rng, pcof)
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        g0, o0 = dp.discrete_adjoint(pcof)
        p0 = dp.eval_populations(pcof)
        b0 = dp.eval_pullback(pcof, **bars)
        jv = _all(dp, pcof, V, bars, history_precomputed=True)
        g1, o1 = dp.discrete_adjoint(pcof, history_precomputed=True)
        assert np.array_equal(g1, g0) and np.array_equal(o1, o0)
        assert np.array_equal(dp.eval_populations(pcof, history_precomputed=True), p0)
        assert np.array_equal(dp.eval_pullback(pcof, history_precomputed=True, **bars), b0)
        # a warm Hessian-vector product before and after: the same bits, and its setup is not run again
        hv = dp.eval_hessian_vec(pcof, hvv)
        hv1, warm = _timed(dp, lambda: dp.eval_hessian_vec(pcof, hvv))
        assert np.array_equal(hv1, hv) and "hess_basis" not in warm and not (warm & set(_FORWARD_PHASES)), warm
        jv1, names = _timed(dp, lambda: _all(dp, pcof, V, bars, history_precomputed=True))
        assert _same(jv1, jv)
        assert {"pushforward_direction", "pushforward_sweep", "pushforward_outputs"} <= names, names
        # (the stored sweep has its stage derivatives and, from the product's setup, its forced basis responses: neither is formed again)
        assert not (names & (set(_FORWARD_PHASES) | {"derivs", "forced_basis", "hess_basis", "hvp_adjoint", "pullback_adjoint"})), names
        hv2, after = _timed(dp, lambda: dp.eval_hessian_vec(pcof, hvv))
        assert np.array_equal(hv2, hv) and "hess_basis" not in after and not (after & set(_FORWARD_PHASES)), after
        # another pcof under history_precomputed: the sweep is redone, and the next product redoes its setup
        fresh = _handle(qgd, prob, ctrl, target, order)
        try:
            ref = _all(fresh, 0.5 * pcof, V, bars)
        finally:
            fresh.close()
        other, names = _timed(dp, lambda: _all(dp, 0.5 * pcof, V, bars, history_precomputed=True))
        assert _same(other, ref) and names & set(_FORWARD_PHASES) and {"derivs", "forced_basis"} <= names, names
        hv3, redo = _timed(dp, lambda: dp.eval_hessian_vec(pcof, hvv))
        assert np.array_equal(hv3, hv) and "hess_basis" in redo and redo & set(_FORWARD_PHASES), redo
    finally:
        dp.close()


# -- 8: without a target, and with tables and basis set directly -----------------------------------------------------------------

def test_without_a_target_and_with_tables_set_directly(qgd):
    from qgd_amd.controls import control_tables_general
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    order = 4
    rng = np.random.default_rng(801)
    bars = _bars(rng, prob, prob.nsteps + 1)
    v = _directions(rng, pcof)
    with_target = _handle(qgd, prob, ctrl, target, order)
    dp = qgd.DeviceProblem(prob, order)
    try:
        dp.set_controls(ctrl)                                # no target on this handle
        jv = _all(dp, pcof, v, bars)
        assert _same(jv, _all(with_target, pcof, v, bars))
        _duality(qgd, dp, prob, pcof, "guarded without a target", seed=802)
        # tables set directly, pcof = None: the basis on the handle is the Jacobian
        p, q, _, _ = control_tables_general(ctrl, np.asarray(pcof, float), prob.nsteps, prob.tf, order // 2)
        dp.set_control_tables(p, q)
        none = _all(dp, None, v, bars)
        for kind in jv:
            _close(none[kind], jv[kind], f"guarded: tables set directly (pcof = None) vs pcof, {kind}")
        _duality(qgd, dp, prob, pcof, "guarded with tables set directly (pcof = None)", seed=803, pcof_arg=None)
        # a control that is not linear in its coefficients goes the same way (tables + Jacobian uploaded by the Python layer)
        gen = qgd.DeviceProblem(prob, order)
        try:
            gen.set_controls([cases.PointwiseOnly(cc) for cc in ctrl])
            general = _all(gen, pcof, v, bars)
            for kind in jv:
                _close(general[kind], jv[kind], f"guarded: pointwise-protocol controls vs the basis path, {kind}")
        finally:
            gen.close()
        z = qgd.eval_pushforward(prob, ctrl, pcof, v, order=order)
        assert np.iscomplexobj(z) and np.array_equal(z, qgd.real_to_complex(jv["states"]))
        assert np.array_equal(qgd.eval_pushforward(prob, ctrl, pcof, v, order=order, output="expectations", observables=bars["observables"]),
                              jv["expectations"])
        qgd.clear_cache()
    finally:
        dp.close(); with_target.close()


# -- 9: refusals ----------------------------------------------------------------------------------------------------------------------

def _raw(dp, pcof, v, n_vec=1, sd=None, pd=None, lm=None, ng=0, ed=None, re=None, im=None, n_obs=0, hp=0, n=None):
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    pc = None if pcof is None else np.ascontiguousarray(pcof, dtype=np.float64)
    rc = dp.lib.qgd_eval_pushforward(dp.h, vp(pc), (0 if pc is None else len(pc)) if n is None else n, hp, vp(v), n_vec, vp(sd), vp(pd),
                                     vp(lm), ng, vp(ed), vp(re), vp(im), n_obs)
    return rc, dp.lib.qgd_last_error(dp.h).decode()


def test_refusals(qgd):
    L = qgd._lib
    A, S, U = L.QGD_ERR_ARGUMENT, L.QGD_ERR_STATE, L.QGD_ERR_UNSUPPORTED
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    SENT = -7.25
    fill = lambda rows, slots=nt, cols=c: np.full((rows, slots, cols, 1), SENT, order="F")
    sd, pd, ed = fill(2 * N), fill(N), fill(1)
    untouched = lambda *arrays: all(np.all(a == SENT) for a in arrays)
    lm, re = np.ones((1, N), order="F"), np.asfortranarray(np.eye(N)[:, :, None])
    v = np.ones(len(pcof))
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        dp.discrete_adjoint(pcof)
        g0, o0 = dp.discrete_adjoint(pcof, history_precomputed=True)
        for what, kw, code in (("NULL v", dict(v=None, sd=sd), A),
                               ("n_vec < 1", dict(v=v, n_vec=0, sd=sd), A),
                               ("all three outputs NULL", dict(v=v), A),
                               ("level_map with n_groups < 1", dict(v=v, pd=pd[:1].copy(order="F"), lm=lm, ng=0), A),
                               ("expect_dot without obs_re", dict(v=v, ed=ed, n_obs=1), A),
                               ("expect_dot with n_obs < 1", dict(v=v, ed=ed, re=re, n_obs=0), A),
                               ("a pcof of another length", dict(v=v, sd=sd, n=len(pcof) - 1), A)):
            rc, msg = _raw(dp, pcof, **kw)
            assert rc == code and msg, (what, rc, msg)
            assert untouched(sd, pd, ed), what
            # nothing was launched: the stored sweep and lambda are as the gradient call left them
            g1, o1 = dp.discrete_adjoint(pcof, history_precomputed=True)
            assert np.array_equal(g1, g0) and np.array_equal(o1, o0), what
        rc, msg = _raw(dp, pcof, v=v, sd=sd, pd=pd, ed=ed, re=re, n_obs=1)
        assert rc == L.QGD_OK and not np.any(sd == SENT) and not np.any(pd == SENT) and not np.any(ed == SENT)
        # a dead stream refuses this entry point like every other one (the flag is set by the tests' hook on a healthy handle)
        sd[:] = SENT
        qgd_hooks.stream_dead(dp, True)
        try:
            rc, msg = _raw(dp, pcof, v=v, sd=sd)
            assert rc == L.QGD_ERR_COMM and "leaked" in msg and untouched(sd)
        finally:
            qgd_hooks.stream_dead(dp, False)
        # the memory refusal: a budget that holds the grid, and observable planes that alone exceed it
        window = dp.memory_plan()["window_bytes"]
        n_obs = window // (N * N * 8) + 1
        big_re, big_ed = np.asfortranarray(np.repeat(re, n_obs, axis=2)), fill(n_obs)
        ref = np.zeros_like(big_ed)
        assert _raw(dp, pcof, v=v, ed=ref, re=big_re, n_obs=n_obs)[0] == L.QGD_OK
        dp.set_memory_budget(window)
        dp.set_controls(ctrl); dp.set_target(target)
        assert dp.memory_plan()["windows"] == 1
        g0 = dp.discrete_adjoint(pcof)[0]
        rc, msg = _raw(dp, pcof, v=v, ed=big_ed, re=big_re, n_obs=n_obs)
        assert rc == L.QGD_ERR_MEMORY and "bytes needed" in msg and untouched(big_ed), (rc, msg)
        assert np.array_equal(dp.discrete_adjoint(pcof, history_precomputed=True)[0], g0)
        dp.set_memory_budget(0)
        dp.set_controls(ctrl); dp.set_target(target)
        rc, msg = _raw(dp, pcof, v=v, ed=big_ed, re=big_re, n_obs=n_obs)
        assert rc == L.QGD_OK and np.array_equal(big_ed, ref)
    finally:
        dp.close()
    # history_precomputed on a handle that has evaluated nothing; no control basis
    dp = qgd.DeviceProblem(prob, 4)
    try:
        rc, msg = _raw(dp, pcof, v=v, sd=sd)
        assert rc == S and "qgd_set_control_basis" in msg
        dp.set_controls(ctrl)
        rc, msg = _raw(dp, pcof, v=v, sd=sd, hp=1)
        assert rc == S and "history_precomputed" in msg and untouched(sd)
        with pytest.raises(qgd._lib.QGDError) as ei:
            dp.eval_pushforward(pcof, v, states=True, history_precomputed=True)
        assert ei.value.code == S
    finally:
        dp.close()
    # a partitioned handle
    rank = qgd.DeviceBackend(prob, 4, ctrl, target, 0, 2)
    try:
        rc, msg = _raw(rank.dp, pcof, v=v, sd=sd)
        assert rc == S and "partitioned" in msg and untouched(sd)
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
        sd2 = fill(2 * prob2.N_tot_levels, 101, prob2.N_initial_conditions)
        rc, msg = _raw(dp, pcof2, v=np.ones(len(pcof2)), sd=sd2)
        assert rc == U and "windows" in msg and untouched(sd2)
        assert np.array_equal(dp.discrete_adjoint(pcof2)[0], g0)
    finally:
        dp.close()
    # N > 64: the smallest such case of cases.py
    prob3, ctrl3, pcof3, target3 = cases.synthetic_case(qgd, nsteps=4)
    dp = _handle(qgd, prob3, ctrl3, target3, 4)
    try:
        g0 = dp.discrete_adjoint(pcof3)[0]
        sd3 = fill(2 * prob3.N_tot_levels, 5, prob3.N_initial_conditions)
        rc, msg = _raw(dp, pcof3, v=np.ones(len(pcof3)), sd=sd3)
        assert rc == U and "N <= 64" in msg and untouched(sd3)
        assert np.array_equal(dp.discrete_adjoint(pcof3)[0], g0)
    finally:
        dp.close()
    # no control operators
    prob4 = qgd.construct_rand_prob(4, 0, tf=0.1, nsteps=6)
    dp = qgd.DeviceProblem(prob4, 4)
    try:
        dp.set_controls([])
        sd4 = fill(8, 7, prob4.N_initial_conditions)
        rc, msg = _raw(dp, None, v=np.ones(1), sd=sd4)
        assert rc == U and "control operators" in msg and untouched(sd4)
    finally:
        dp.close()
    # more than 64 basis directions: 5 operators at order 16 (80)
    prob5 = qgd.construct_rand_prob(4, 5, tf=1.0, nsteps=6)
    ctrl5 = [qgd.FortranBSplineControl(16, 20, prob5.tf) for _ in range(5)]
    dp = qgd.DeviceProblem(prob5, 16)
    try:
        dp.set_controls(ctrl5)
        npc = qgd.get_number_of_control_parameters(ctrl5)
        sd5 = fill(8, 7, prob5.N_initial_conditions)
        rc, msg = _raw(dp, np.random.default_rng(1).random(npc), v=np.ones(npc), sd=sd5)
        assert rc == U and "basis directions" in msg and untouched(sd5)
    finally:
        dp.close()
