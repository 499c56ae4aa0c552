"""GPU tests of qgd_eval_dense_pushforward: J v, the directional derivatives of the DENSE trajectory
outputs -- states, level populations and expectation values of the Hermite interpolant -- along directions v in pcof.  Against
the numpy statement (proto_dense_pushforward.py, which test_dense_pushforward_proto.py holds to differences of its own outputs)
at the shapes of test_gpu_dense_pullback.py; against the device's eval_dense_pullback (duality); against differences of the
device's own dense outputs; then what is bitwise: the grid slots and refine = 1 against eval_pushforward, runs, chunks, slot 0;
what the call leaves of the stored evaluation; the refusals.

Bounds, those of test_gpu_pushforward.py.  An output against the statement: 1e-10 max(1, max|ref|) (_close).  Two formulations of
one directional derivative <g, v>: 1e-10 max(1, max|g|) |v|_1 (_dual).  Differences: h = 1e-3 and 5e-4 extrapolated, 1e-8 of the
difference quotient, on the scalar <ybar, output>; the seeds of that test keep the statement's own error against the same
quotient under 1e-9 |fd| (checked with the statement on the CPU: at most 5.1e-11 |fd|).  The measured figures are in DESIGN.md
section 4n."""
import ctypes as C
import re

import numpy as np
import pytest

import cases
import proto_dense_pushforward as pdf
import proto_pushforward as pf
from test_gpu_dense_pullback import SHAPES, _bars
from test_gpu_hessian import _case, _handle
from test_gpu_hvp import _FORWARD_PHASES, _paths
from test_gpu_pullback import _hermitian
from test_gpu_pushforward import KINDS, _close, _dual, _same, _timed

pytestmark = pytest.mark.gpu

N_VEC = 3


def _all(dp, refine, pcof, v, bars, **kw):
    return dp.eval_dense_pushforward(refine, pcof, v, states=True, level_map=bars["level_map"], observables=bars["observables"], **kw)


# -- 1: the device against the numpy statement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SHAPES))
def test_device_matches_the_statement(qgd, name):
    make, order, refine = SHAPES[name]
    prob, ctrl, pcof, target = make(qgd)
    N = prob.N_tot_levels
    rng = np.random.default_rng(41)
    V = rng.standard_normal((len(pcof), N_VEC))
    lm, oc, orl = rng.standard_normal((5, N)), _hermitian(rng, 3, N), _hermitian(rng, 2, N, False)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    pre = pdf.setup(prob, Gp, Gq, off, pcof, target, order)
    terms = [pdf.dense_pushforward(qgd, prob, Gp, Gq, off, pcof, target, order, refine, V[:, j], pre=pre, terms=True)[1] for j in range(N_VEC)]

    def ref(level_map=None, observables=None):
        per = [pf.tangents(t["d"], t["dd"], 1, level_map, observables) for t in terms]
        return [None if per[0][i] is None else np.stack([p[i] for p in per], axis=-1) for i in range(3)]
    S, P, E = ref(lm, oc)
    Pn, Er = ref()[1], ref(None, orl)[2]
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        if name.startswith("cnot3"):
            assert N == 64 and dp.operator_path()[0] == "sparse"
        for path in _paths(qgd, dp):
            label = f"{name} order {order} refine {refine} {path}"
            run = lambda **kw: dp.eval_dense_pushforward(refine, pcof, V, **kw)
            out = run(states=True)
            assert set(out) == {"states"} and out["states"].shape == (2 * N, 1 + prob.nsteps * refine, prob.N_initial_conditions, N_VEC)
            _close(out["states"], S, f"{label}: states alone")
            _close(run(level_map=lm)["populations"], P, f"{label}: populations with a 5-row map")
            _close(run(populations=True)["populations"], Pn, f"{label}: populations without a map")
            _close(run(observables=oc)["expectations"], E, f"{label}: expectations, complex observables")
            _close(run(observables=orl)["expectations"], Er, f"{label}: expectations, real observables")
            out = run(states=True, level_map=lm, observables=oc)
            for kind, r in (("states", S), ("populations", P), ("expectations", E)):
                _close(out[kind], r, f"{label}: all three at once, {kind}")
    finally:
        dp.close()


# -- 2: duality with the device's dense pullback ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,order,refine", [("cnot2", 2, 2), ("cnot2", 4, 3), ("cnot2", 8, 3), ("guarded", 6, 3), ("cnot3-r2", 8, 2)])
def test_duality_with_the_dense_pullback(qgd, name, order, refine):
    prob, ctrl, pcof, target = SHAPES[name][0](qgd) if name in SHAPES else _case(qgd, name)
    rng = np.random.default_rng(43)
    bars = _bars(prob, rng, refine)
    V = rng.standard_normal((len(pcof), N_VEC))
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        for path in _paths(qgd, dp):
            out = _all(dp, refine, pcof, V, bars)
            for kind, bar, extra in KINDS:
                g = dp.eval_dense_pullback(refine, pcof, **{bar: bars[bar], **{k: bars[k] for k in extra}})
                for j in range(N_VEC):
                    _dual(np.sum(bars[bar] * out[kind][..., j]), g @ V[:, j], g, V[:, j], f"{name} order {order} refine {refine} {path}: {kind}, direction {j}")
    finally:
        dp.close()


# -- 3: differences of the device's own dense outputs ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,order,refine", [("cnot2", 8, 3), ("guarded", 6, 3)])
def test_matches_differences_of_the_dense_outputs(qgd, name, order, refine):
    prob, ctrl, pcof, target = _case(qgd, name)
    rng = np.random.default_rng(47)
    bars = _bars(prob, rng, refine, n_groups=3)
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        def J(p):
            return {"states": np.sum(bars["states_bar"] * dp.eval_dense_states(refine, p)),
                    "populations": np.sum(bars["populations_bar"] * dp.eval_dense_populations(refine, p, level_map=bars["level_map"])),
                    "expectations": np.sum(bars["expectations_bar"] * dp.eval_dense_expectations(refine, bars["observables"], p))}
        for _ in range(2):
            v = rng.standard_normal(len(pcof)); v /= np.linalg.norm(v)
            out = _all(dp, refine, pcof, v, bars)

            def fd(h):
                a, b = J(pcof + h * v), J(pcof - h * v)
                return {k: (a[k] - b[k]) / (2 * h) for k in a}
            f1, f2 = fd(1e-3), fd(5e-4)
            for kind, bar, _e in KINDS:
                F = (4 * f2[kind] - f1[kind]) / 3
                err = abs(np.sum(bars[bar] * out[kind]) - F)
                print(f"\n{name} order {order} refine {refine} {kind}: |<ybar, J v> - fd| = {err:.3e}, |fd| = {abs(F):.3e}, bound {1e-8 * abs(F):.3e}")
                assert err <= 1e-8 * abs(F), kind
    finally:
        dp.close()


# -- 4: grid slots and refine = 1 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,order", [("cnot2", 4), ("guarded", 6)])
def test_grid_slots_and_refine_one_are_the_grid_point_pushforward(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    refine = 3
    rng = np.random.default_rng(53)
    bars = _bars(prob, rng, 1)
    V = rng.standard_normal((len(pcof), N_VEC))
    grid_all = lambda **kw: dp.eval_pushforward(pcof, V, states=True, level_map=bars["level_map"], observables=bars["observables"], **kw)
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        grid = grid_all()
        dense = _all(dp, refine, pcof, V, bars)
        assert np.array_equal(dense["states"][:, ::refine], grid["states"]) and np.abs(grid["states"][:, 1:]).max() > 0
        assert np.array_equal(dp.eval_dense_pushforward(refine, pcof, V, states=True)["states"][:, ::refine], grid["states"])
        assert _same(_all(dp, 1, pcof, V, bars), grid)
        assert _same(_all(dp, 1, pcof, V, bars, history_precomputed=True), grid)
        dp.set_save_every(3)                           # no part in it, as in eval_dense
        try:
            assert _same(_all(dp, 1, pcof, V, bars), grid)
            assert _same(_all(dp, refine, pcof, V, bars), dense)
            third = grid_all()
            assert all(np.array_equal(third[k], grid[k][:, ::3]) for k in grid)
        finally:
            dp.set_save_every(1)
    finally:
        dp.close()


# -- 5: what is bitwise -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cnot2", "guarded"])
def test_bitwise_runs_chunks_slot_zero_and_other_calls_in_between(qgd, name, monkeypatch):
    prob, ctrl, pcof, target = _case(qgd, name)
    order, refine = 4, 3
    rng = np.random.default_rng(59)
    bars = _bars(prob, rng, refine)
    V = rng.standard_normal((len(pcof), N_VEC))
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        three = _all(dp, refine, pcof, V, bars)
        assert _same(_all(dp, refine, pcof, V, bars), three)
        assert _same(_all(dp, refine, pcof, V, bars, history_precomputed=True), three)
        singles = [_all(dp, refine, pcof, V[:, j], bars) for j in range(N_VEC)]
        for kind in three:
            assert three[kind].shape[1] == 1 + prob.nsteps * refine and three[kind].shape[-1] == N_VEC
            assert not three[kind][:, 0].any() and np.abs(three[kind][:, 1]).max() > 0, kind      # slot 0: exact zeros
            for j in range(N_VEC):
                assert singles[j][kind].ndim == 3 and np.array_equal(three[kind][..., j], singles[j][kind]), (kind, j)
        # another refine and other output selections in between change nothing
        assert np.all(np.isfinite(dp.eval_dense_pushforward(2, pcof, V[:, :2], populations=True)["populations"]))
        assert np.array_equal(dp.eval_dense_pushforward(refine, pcof, V, observables=bars["observables"][:1])["expectations"],
                              three["expectations"][:1])
        assert np.array_equal(dp.eval_dense_pushforward(refine, pcof, V, states=True)["states"], three["states"])
        assert _same(_all(dp, refine, pcof, V, bars), three)
        # chunks of two directions (2 + 1), on a handle of its own: the knob is read when the handle is created
        monkeypatch.setenv("QGD_PUSHFORWARD_CHUNK", "2")
        ch = _handle(qgd, prob, ctrl, target, order)
        monkeypatch.delenv("QGD_PUSHFORWARD_CHUNK")
        try:
            assert _same(_all(ch, refine, pcof, V, bars), three)
            assert _same(_all(ch, refine, pcof, V[:, :2], bars), {k: a[..., :2] for k, a in three.items()})
            assert _same(_all(ch, refine, pcof, V, bars), three)
        finally:
            ch.close()
        z = qgd.eval_dense_pushforward(prob, ctrl, pcof, V, order=order, refine=refine)
        assert np.iscomplexobj(z) and np.array_equal(z, qgd.real_to_complex(three["states"]))
        qgd.clear_cache()
    finally:
        dp.close()


# -- 6: the neighbours --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cnot2", "guarded"])
def test_leaves_the_stored_evaluation_and_the_hvp_setup_usable(qgd, name):
    prob, ctrl, pcof, target = _case(qgd, name)
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    order, refine = 4, 3
    rng = np.random.default_rng(61)
    bars = _bars(prob, rng, refine)
    sb = rng.standard_normal((2 * N, nt, c))
    V, hvv = rng.standard_normal((len(pcof), 2)), rng.standard_normal(len(pcof))
    dp = _handle(qgd, prob, ctrl, target, order)
    try:
        g0, o0 = dp.discrete_adjoint(pcof)
        b0, d0 = dp.eval_pullback(pcof, states_bar=sb), dp.eval_dense_states(refine, pcof)
        f0 = dp.eval_pushforward(pcof, V, states=True, populations=True)
        jv = _all(dp, refine, pcof, V, bars, history_precomputed=True)
        g1, o1 = dp.discrete_adjoint(pcof, history_precomputed=True)
        assert np.array_equal(g1, g0) and np.array_equal(o1, o0)
        assert np.array_equal(dp.eval_pullback(pcof, states_bar=sb, history_precomputed=True), b0)
        assert np.array_equal(dp.eval_dense_states(refine, pcof, history_precomputed=True), d0)
        assert _same(dp.eval_pushforward(pcof, V, states=True, populations=True, history_precomputed=True), f0)
        assert _same(_all(dp, refine, pcof, V, bars, history_precomputed=True), jv)
        # a warm Hessian-vector product before and after: the same bits, and its setup is not run again
        hv = dp.eval_hessian_vec(pcof, hvv)
        hv1, warm = _timed(dp, lambda: dp.eval_hessian_vec(pcof, hvv))
        assert np.array_equal(hv1, hv) and "hess_basis" not in warm and not (warm & set(_FORWARD_PHASES)), warm
        jv1, names = _timed(dp, lambda: _all(dp, refine, pcof, V, bars, history_precomputed=True))
        assert _same(jv1, jv)
        assert {"pushforward_direction", "pushforward_sweep", "dense_pushforward_derivs", "dense_pushforward_interp",
                "dense_pushforward_outputs"} <= names, names
        # (the stored sweep has its stage derivatives and, from the product's setup, its forced basis responses: neither is formed again)
        assert not (names & (set(_FORWARD_PHASES) | {"derivs", "forced_basis", "hess_basis", "hvp_adjoint", "pullback_adjoint", "pushforward_outputs"})), names
        hv2, after = _timed(dp, lambda: dp.eval_hessian_vec(pcof, hvv))
        assert np.array_equal(hv2, hv) and "hess_basis" not in after and not (after & set(_FORWARD_PHASES)), after
        # another pcof under history_precomputed: the sweep is redone, and the next product redoes its setup
        fresh = _handle(qgd, prob, ctrl, target, order)
        try:
            ref = _all(fresh, refine, 0.5 * pcof, V, bars)
        finally:
            fresh.close()
        other, names = _timed(dp, lambda: _all(dp, refine, 0.5 * pcof, V, bars, history_precomputed=True))
        assert _same(other, ref) and names & set(_FORWARD_PHASES) and {"derivs", "forced_basis"} <= names, names
        hv3, redo = _timed(dp, lambda: dp.eval_hessian_vec(pcof, hvv))
        assert np.array_equal(hv3, hv) and "hess_basis" in redo and redo & set(_FORWARD_PHASES), redo
    finally:
        dp.close()


# -- 7: refusals ----------------------------------------------------------------------------------------------------------------------

def _raw(dp, pcof, v, refine=2, n_vec=1, sd=None, pd=None, lm=None, ng=0, ed=None, re=None, im=None, n_obs=0, hp=0, n=None):
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    pc = None if pcof is None else np.ascontiguousarray(pcof, dtype=np.float64)
    rc = dp.lib.qgd_eval_dense_pushforward(dp.h, vp(pc), (0 if pc is None else len(pc)) if n is None else n, hp, refine, vp(v), n_vec,
                                           vp(sd), vp(pd), vp(lm), ng, vp(ed), vp(re), vp(im), n_obs)
    return rc, dp.lib.qgd_last_error(dp.h).decode()


SENT = -7.25


def _fill(rows, slots, cols):
    return np.full((rows, slots, cols, 1), SENT, order="F")


def _untouched(*arrays):
    return all(np.all(a == SENT) for a in arrays)


def test_refusals(qgd):
    L = qgd._lib
    A, S, U = L.QGD_ERR_ARGUMENT, L.QGD_ERR_STATE, L.QGD_ERR_UNSUPPORTED
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    N, c, slots = prob.N_tot_levels, prob.N_initial_conditions, 1 + 2 * prob.nsteps
    sd, pd, ed = _fill(2 * N, slots, c), _fill(N, slots, c), _fill(1, slots, c)
    lm, re_ = np.ones((1, N), order="F"), np.asfortranarray(np.eye(N)[:, :, None])
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
                               ("expect_dot with n_obs < 1", dict(v=v, ed=ed, re=re_, n_obs=0), A),
                               ("a pcof of another length", dict(v=v, sd=sd, n=len(pcof) - 1), A),
                               ("refine = 0", dict(v=v, sd=sd, refine=0), A),
                               ("refine < 0", dict(v=v, sd=sd, refine=-2), A),
                               ("1 + nsteps * refine beyond int32", dict(v=v, sd=sd, refine=2 ** 28), A)):
            rc, msg = _raw(dp, pcof, **kw)
            assert rc == code and msg, (what, rc, msg)
            assert _untouched(sd, pd, ed), what
            # nothing was launched: the stored sweep and lambda are as the gradient call left them
            g1, o1 = dp.discrete_adjoint(pcof, history_precomputed=True)
            assert np.array_equal(g1, g0) and np.array_equal(o1, o0), what
        rc, msg = _raw(dp, pcof, v=v, sd=sd, pd=pd, ed=ed, re=re_, n_obs=1)
        assert rc == L.QGD_OK and not np.any(sd[:, 1:] == SENT) and not np.any(pd == SENT) and not np.any(ed == SENT)
        assert np.array_equal(sd[..., 0], dp.eval_dense_pushforward(2, pcof, v, states=True)["states"])
    finally:
        dp.close()
    # (refine > 1 with order/2 > 8 is refused as in qgd_eval_dense_pullback; qgd_create admits no order beyond 16, so no handle
    #  reaches that refusal and it has no case here)
    # history_precomputed on a handle that has evaluated nothing; no control basis
    dp = qgd.DeviceProblem(prob, 4)
    try:
        rc, msg = _raw(dp, pcof, v=v, sd=sd)
        assert rc == S and "qgd_set_control_basis" in msg
        dp.set_controls(ctrl)
        sd[:] = SENT
        rc, msg = _raw(dp, pcof, v=v, sd=sd, hp=1)
        assert rc == S and "history_precomputed" in msg and _untouched(sd)
        with pytest.raises(qgd._lib.QGDError) as ei:
            dp.eval_dense_pushforward(2, pcof, v, states=True, history_precomputed=True)
        assert ei.value.code == S
    finally:
        dp.close()
    # a partitioned handle
    rank = qgd.DeviceBackend(prob, 4, ctrl, target, 0, 2)
    try:
        rc, msg = _raw(rank.dp, pcof, v=v, sd=sd)
        assert rc == S and "partitioned" in msg and _untouched(sd)
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
        sd2 = _fill(2 * prob2.N_tot_levels, 201, prob2.N_initial_conditions)
        rc, msg = _raw(dp, pcof2, v=np.ones(len(pcof2)), sd=sd2)
        assert rc == U and "windows" in msg and _untouched(sd2)
        assert np.array_equal(dp.discrete_adjoint(pcof2)[0], g0)
    finally:
        dp.close()
    # N > 64: the smallest such case of cases.py
    prob3, ctrl3, pcof3, target3 = cases.synthetic_case(qgd, nsteps=4)
    dp = _handle(qgd, prob3, ctrl3, target3, 4)
    try:
        g0 = dp.discrete_adjoint(pcof3)[0]
        sd3 = _fill(2 * prob3.N_tot_levels, 9, prob3.N_initial_conditions)
        rc, msg = _raw(dp, pcof3, v=np.ones(len(pcof3)), sd=sd3)
        assert rc == U and "N <= 64" in msg and _untouched(sd3)
        assert np.array_equal(dp.discrete_adjoint(pcof3)[0], g0)
    finally:
        dp.close()
    # no control operators
    prob4 = qgd.construct_rand_prob(4, 0, tf=0.1, nsteps=6)
    dp = qgd.DeviceProblem(prob4, 4)
    try:
        dp.set_controls([])
        sd4 = _fill(8, 13, prob4.N_initial_conditions)
        rc, msg = _raw(dp, None, v=np.ones(1), sd=sd4)
        assert rc == U and "control operators" in msg and _untouched(sd4)
    finally:
        dp.close()
    # more than 64 basis directions: 5 operators at order 16 (80)
    prob5 = qgd.construct_rand_prob(4, 5, tf=1.0, nsteps=6)
    ctrl5 = [qgd.FortranBSplineControl(16, 20, prob5.tf) for _ in range(5)]
    dp = qgd.DeviceProblem(prob5, 16)
    try:
        dp.set_controls(ctrl5)
        npc = qgd.get_number_of_control_parameters(ctrl5)
        sd5 = _fill(8, 13, prob5.N_initial_conditions)
        rc, msg = _raw(dp, np.random.default_rng(1).random(npc), v=np.ones(npc), sd=sd5)
        assert rc == U and "basis directions" in msg and _untouched(sd5)
    finally:
        dp.close()


def test_a_budget_too_small_for_one_direction_leaves_the_handle_usable(qgd):
    """Under a budget that holds the grid and, at this refine, the interpolated state panels (0.8 of it), the call's own buffers of
    ONE direction do not fit: the interpolated tangent panels are as large again and the staged states 2N / (Np 2) of that.
    QGD_ERR_MEMORY before anything is launched, and a smaller refine goes through with the bits of before."""
    L = qgd._lib
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    N, c = prob.N_tot_levels, prob.N_initial_conditions
    v = np.ones(len(pcof))
    dp = qgd.DeviceProblem(prob, 4)
    window = dp.memory_plan()["window_bytes"]
    dp.set_memory_budget(8 * window)
    dp.set_controls(ctrl); dp.set_target(target)
    try:
        budget = dp.memory_plan()["budget"]
        assert dp.memory_plan()["windows"] == 1 and budget == 8 * window
        g0, o0 = dp.discrete_adjoint(pcof)
        p0 = dp.eval_dense_pushforward(3, pcof, v, states=True)["states"]
        Np, cp = 16 * ((N + 15) // 16), 8 * ((c + 7) // 8)
        refine = (budget * 4 // 5) // (8 * prob.nsteps * Np * 2 * cp)      # (1 + nsteps r) Np 2 cp doubles: 0.8 of the budget
        assert refine > 3
        sd = _fill(2 * N, 1 + prob.nsteps * refine, c)
        rc, msg = _raw(dp, pcof, v=v, sd=sd, refine=refine)
        assert rc == L.QGD_ERR_MEMORY and "qgd_eval_dense_pushforward" in msg and "bytes needed" in msg and _untouched(sd), (rc, msg)
        need = int(re.search(r"\((\d+) bytes needed\)", msg).group(1))
        print(f"\nguarded: window {window} bytes, budget {budget}, refine {refine}: the refused call needs {need}")
        assert window < budget < need
        g1, o1 = dp.discrete_adjoint(pcof, history_precomputed=True)
        assert np.array_equal(g1, g0) and np.array_equal(o1, o0)
        assert np.array_equal(dp.eval_dense_pushforward(3, pcof, v, states=True)["states"], p0)
        fresh = _handle(qgd, prob, ctrl, target, 4)
        try:
            assert np.array_equal(fresh.eval_dense_pushforward(3, pcof, v, states=True)["states"], p0)
        finally:
            fresh.close()
    finally:
        dp.close()
