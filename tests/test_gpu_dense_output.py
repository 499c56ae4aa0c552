"""GPU tests of qgd_eval_dense: the Hermite dense output -- states, level populations and expectation
values between the grid points, from the stage derivatives the sweep forms anyway (csrc/qgd_k_interp.hip).

1  Device against the statement.  Reference: hermite_interpolate (numpy, tests/test_dense_output_host.py pins it to polynomials
   and to the oracle) applied to the device's own uv_history of eval_forward on the same handle and pcof.  Elementwise bound,
   derived, not tuned:
       |dev - ref| <= 128 eps sum_j dt^j (|a_j| |w_{n,j}| + |b_j| |w_{n+1,j}|),      eps = 2^-52
   at most 18 terms, each with about (2m+4) eps of weight rounding (two powers, a sum of m+1 terms, three products, on the
   host in C++ and in numpy), one product rounding and the accumulation (fused on the device, not in numpy): <= ~40 eps of
   the absolute sum, with a factor 3 of headroom.  Grid slots: exact equality.
2  Grid slots equal eval_states bitwise; refine = 1 equals eval_states bitwise.
3  Populations and expectation values are those of the interpolated state: numpy applied to the dense states the call itself
   returns, at the bounds tests/test_gpu_populations.py and tests/test_gpu_expectations.py hold the same comparison to.
4  Meaning: the dense output of a 20-step run against the device's own 80-step run.
5  Bookkeeping: reproducibility, the stored sweep, the kept setup of eval_hessian_vec, set_save_every, out3.
6  Windowed grids at the tolerance of tests/test_gpu_memory.py::test_chunked_grid_matches_resident (1e-11 max(1, max|ref|)).
7  Refusals through the raw C ABI."""
import ctypes as C

import numpy as np
import pytest

import cases
from test_gpu_hessian import _handle
from test_gpu_populations import _check_pop, _check_grouped
from test_gpu_expectations import _check as _check_expect

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52

# name -> (case, order, values of refine)
SHAPES = {
    "cnot2-o2": (lambda q: cases.cnot2_case(q, nsteps=12, tf=12.0), 2, (1, 2)),      # N = 4, Np = 16, c = 4: padded rows and columns
    "cnot2-o8": (lambda q: cases.cnot2_case(q, nsteps=12, tf=12.0), 8, (3, 16)),
    "cnot2-o16": (lambda q: cases.cnot2_case(q, nsteps=12, tf=12.0), 16, (2, 7)),
    "guarded": (lambda q: cases.guarded_case(q, nsteps=10, tf=5.0), 6, (1, 3)),
    "cnot3": (lambda q: cases.cnot3_case(q, nsteps=20), 8, (2, 7)),                   # N = 64, c = 8: full panel, sparse path
    "syn72": (lambda q: cases.synthetic_case(q, N=72, c=4, n_ops=1, nsteps=8), 4, (3, 16)),      # Np > 64, partial row block
    "syn100": (lambda q: cases.synthetic_case(q, N=100, c=20, n_ops=2, nsteps=6), 12, (2, 7)),   # three column groups, the last partial
    "one-step": (lambda q: cases.cnot2_case(q, nsteps=1, tf=1.0), 4, (1, 3)),
}


def _open(qgd, name):
    make, order, refines = SHAPES[name]
    prob, ctrl, pcof, target = make(qgd)
    return _handle(qgd, prob, ctrl, target, order), prob, pcof, order, refines


def _uv(dp, pcof):
    hist = np.zeros((2 * dp.N, dp.m + 1, dp.nsteps + 1, dp.c), order="F")
    dp.eval_forward(pcof, uv_history=hist)
    return hist


def _abs_sum(qgd, hist, dt, r):
    """sum_j |a_j| |w_{n,j}| + |b_j| |w_{n+1,j}| at every interior slot [2N, nsteps, r-1, c]"""
    a, b = qgd.hermite_dense_weights(hist.shape[1] - 1, r, dt)
    h = np.abs(hist)
    return np.einsum("sj,ijnc->insc", np.abs(a), h[:, :, :-1]) + np.einsum("sj,ijnc->insc", np.abs(b), h[:, :, 1:])


# -- 1, 2: the device against the statement; grid slots ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SHAPES))
def test_device_matches_the_statement(qgd, name):
    dp, prob, pcof, order, refines = _open(qgd, name)
    try:
        hist = _uv(dp, pcof)
        states = dp.eval_states(pcof)
        assert np.array_equal(states, hist[:, 0])
        dt, nst = prob.tf / prob.nsteps, prob.nsteps
        for r in refines:
            dev = dp.eval_dense_states(r, pcof)
            assert dev.shape == (2 * dp.N, 1 + nst * r, dp.c) and dev.flags.f_contiguous and np.all(np.isfinite(dev))
            assert np.array_equal(dev[:, ::r], states), (name, r)      # grid slots: the bits eval_states returns
            if r == 1:
                continue
            ref = qgd.hermite_interpolate(hist, dt, r)
            inner = lambda x: np.stack([x[:, s::r][:, :nst] for s in range(1, r)], axis=2)      # [2N, nsteps, r-1, c]
            err, bound = np.abs(inner(dev) - inner(ref)), 128 * EPS * _abs_sum(qgd, hist, dt, r)
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))
            print(f"\n{name} order {order} refine {r}: max |dev - ref| / (eps abs sum) = {128 * worst:.2f} (bound 128), max abs {err.max():.2e}")
            assert np.all(err <= bound), (name, r, worst)
    finally:
        dp.close()


# -- 3: populations and expectation values of the interpolant ---------------------------------------------------------------------

@pytest.mark.parametrize("name,r", [("cnot2-o8", 3), ("cnot3", 2), ("syn72", 3)])
def test_populations_and_expectations_of_the_interpolant(qgd, name, r):
    dp, prob, pcof, order, _ = _open(qgd, name)
    N = dp.N
    rng = np.random.default_rng(40 + N)
    try:
        w = dp.eval_dense_states(r, pcof)
        p_ref = w[:N] ** 2 + w[N:] ** 2
        _check_pop(dp.eval_dense_populations(r, pcof), p_ref, f"{name} refine {r}")
        M = rng.standard_normal((5, N))
        _check_grouped(dp.eval_dense_populations(r, pcof, level_map=M), M, p_ref, f"{name} refine {r}")
        sym = rng.standard_normal((N, N))
        a = rng.standard_normal((3, N, N)) + 1j * rng.standard_normal((3, N, N))
        fake = w[:, None]                     # [2N, 1, slots, c]: the dense states in the place of Taylor index 0
        _check_expect(dp.eval_dense_expectations(r, sym + sym.T, pcof), fake, (sym + sym.T)[None], f"{name} refine {r} real")
        herm = a + np.conj(np.transpose(a, (0, 2, 1)))
        _check_expect(dp.eval_dense_expectations(r, herm, pcof), fake, herm, f"{name} refine {r} complex")
    finally:
        dp.close()


# -- 4: meaning ----------------------------------------------------------------------------------------------------------------------

def test_dense_output_against_the_finer_run(qgd):
    """cnot2, order 8: 20 steps with refine = 4 against eval_states of the same problem at 80 steps -- the device is its own fine
    reference.  The interior error is at most twice the grid-slot error of that comparison (the condition of the CPU test)."""
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=20, tf=20.0)
    fine_prob, fine_ctrl, fine_pcof, _ = cases.cnot2_case(qgd, nsteps=80, tf=20.0)
    assert np.array_equal(pcof, fine_pcof)
    dp, fine = _handle(qgd, prob, ctrl, target, 8), _handle(qgd, fine_prob, fine_ctrl, target, 8)
    try:
        err = np.abs(dp.eval_dense_states(4, pcof) - fine.eval_states(pcof)).max(axis=(0, 2))
        grid, interior = err[::4].max(), np.delete(err, np.s_[::4]).max()
        print(f"\ncnot2 order 8, 20 steps, refine 4 against 80 steps: grid slots {grid:.3e}, interior {interior:.3e} (ratio {interior / grid:.3f}, bound 2)")
        assert grid > 0 and interior <= 2.0 * grid
    finally:
        dp.close(); fine.close()


# -- 5: bookkeeping -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cnot2-o8", "cnot3"])
def test_bookkeeping(qgd, name):
    dp, prob, pcof, order, _ = _open(qgd, name)
    r = 4
    try:
        d0 = dp.eval_dense_states(r, pcof)
        o3 = dp.last_scalars.copy()
        assert np.array_equal(dp.eval_dense_states(r, pcof), d0)                               # the same bits on every run
        assert np.array_equal(dp.eval_dense_states(r, pcof, history_precomputed=True), d0)    # and from the stored sweep
        p0 = dp.eval_dense_populations(r, pcof, history_precomputed=True)
        assert np.array_equal(dp.eval_dense_populations(r, pcof), p0)
        # out3 is that of eval_populations
        dp.eval_populations(pcof)
        assert np.array_equal(dp.last_scalars, o3)
        # a history_precomputed gradient / populations call returns the bits it returns without a dense call in between
        dp.eval_forward(pcof)
        g0, s0 = dp.discrete_adjoint(pcof, history_precomputed=True)
        q0 = dp.eval_populations(pcof, history_precomputed=True)
        for fresh in (True, False):
            assert np.array_equal(dp.eval_dense_states(r, pcof, history_precomputed=not fresh), d0)
            g1, s1 = dp.discrete_adjoint(pcof, history_precomputed=True)
            assert np.array_equal(g1, g0) and np.array_equal(s1, s0), fresh
            assert np.array_equal(dp.eval_populations(pcof, history_precomputed=True), q0), fresh
            assert np.array_equal(dp.eval_dense_states(r, pcof, history_precomputed=True), d0)
        # the kept setup of eval_hessian_vec survives a dense call that reuses its sweep
        v = np.random.default_rng(7).standard_normal(len(pcof))
        hv0 = dp.eval_hessian_vec(pcof, v)
        assert np.array_equal(dp.eval_dense_states(r, pcof, history_precomputed=True), d0)
        assert np.array_equal(dp.eval_hessian_vec(pcof, v), hv0)
        # independent of set_save_every
        dp.set_save_every(3)
        try:
            assert np.array_equal(dp.eval_dense_states(r, pcof), d0)
            assert np.array_equal(dp.eval_dense_populations(r, pcof), p0)
            assert np.array_equal(dp.eval_dense_states(1, pcof), d0[:, ::r])
        finally:
            dp.set_save_every(1)
    finally:
        dp.close()


# -- 6: windowed grids -----------------------------------------------------------------------------------------------------------------

def test_windowed_grid_matches_resident(qgd):
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=100, tf=100.0)
    order, r, N = 4, 3, prob.N_tot_levels
    rng = np.random.default_rng(9)
    M = rng.standard_normal((5, N))
    a = rng.standard_normal((2, N, N)) + 1j * rng.standard_normal((2, N, N))
    herm = a + np.conj(np.transpose(a, (0, 2, 1)))
    res = _handle(qgd, prob, ctrl, target, order)
    win = qgd.DeviceProblem(prob, order)
    win.set_memory_budget(win.memory_plan()["window_bytes"] // 3)
    win.set_controls(ctrl); win.set_target(target)
    try:
        assert res.memory_plan()["windows"] == 1 and win.memory_plan()["windows"] >= 2
        pinned = win.pin(np.full((2 * N, 1 + 100 * r, prob.N_initial_conditions), np.nan, order="F"))
        for what, ref, got in (("states", res.eval_dense_states(r, pcof), win.eval_dense_states(r, pcof)),
                               ("states, registered out", res.eval_dense_states(r, pcof), win.eval_dense_states(r, pcof, out=pinned)),
                               ("populations", res.eval_dense_populations(r, pcof, level_map=M), win.eval_dense_populations(r, pcof, level_map=M)),
                               ("expectations", res.eval_dense_expectations(r, herm, pcof), win.eval_dense_expectations(r, herm, pcof))):
            err, tol = np.abs(got - ref).max(), 1e-11 * max(1.0, np.abs(ref).max())
            print(f"\ncnot2 100 steps, {win.memory_plan()['windows']} windows, refine {r}, {what}: max |windowed - resident| = {err:.2e} (bound {tol:.1e})")
            assert got.shape == ref.shape and np.all(np.isfinite(got)) and err <= tol, what
        assert np.array_equal(win.eval_dense_states(r, pcof)[:, ::r], win.eval_states(pcof))      # grid slots of a windowed grid
        assert np.array_equal(win.eval_dense_states(r, pcof), pinned)
        o3 = win.last_scalars.copy()
        win.eval_populations(pcof)
        assert np.array_equal(win.last_scalars, o3)
    finally:
        res.close(); win.close()


# -- 7: refusals -----------------------------------------------------------------------------------------------------------------------

def test_panels_beyond_the_memory_budget_are_refused(qgd):
    """one buffer, no slabs: interpolated panels larger than the budget are QGD_ERR_MEMORY before anything is launched"""
    prob, ctrl, pcof, target = cases.guarded_case(qgd, nsteps=10, tf=5.0)
    dp = qgd.DeviceProblem(prob, 4)
    dp.set_memory_budget(2 * dp.memory_plan()["window_bytes"])
    dp.set_controls(ctrl); dp.set_target(target)
    try:
        assert dp.memory_plan()["windows"] == 1
        d0 = dp.eval_dense_states(3, pcof)
        g0, o0 = dp.discrete_adjoint(pcof, history_precomputed=True)
        r = 1 + 2 * dp.memory_plan()["budget"] // (16 * 2 * 8 * 8 * 10)      # (1 + 10 r) panels of Np = 16, cp = 8 exceed the budget
        out = np.full((2 * dp.N, 1 + 10 * int(r), dp.c), np.nan, order="F")
        rc, msg = _raw(dp, pcof, out, refine=int(r))
        assert rc == qgd._lib.QGD_ERR_MEMORY and "bytes needed" in msg and np.all(np.isnan(out)), (rc, msg)
        g1, o1 = dp.discrete_adjoint(pcof, history_precomputed=True)
        assert np.array_equal(g1, g0) and np.array_equal(o1, o0)
        assert np.array_equal(dp.eval_dense_states(3, pcof), d0)
    finally:
        dp.close()


def _raw(dp, pcof, out, refine=2, kind=0, hp=0, lm=None, ng=0, re=None, im=None, n_obs=0, n=None):
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    pc = None if pcof is None else np.ascontiguousarray(pcof, dtype=np.float64)
    rc = dp.lib.qgd_eval_dense(dp.h, vp(pc), (0 if pc is None else len(pc)) if n is None else n, hp, refine, kind, vp(lm), ng,
                               vp(re), vp(im), n_obs, vp(out), None)
    return rc, dp.lib.qgd_last_error(dp.h).decode()


def test_refusals(qgd):
    L = qgd._lib
    A, S, U = L.QGD_ERR_ARGUMENT, L.QGD_ERR_STATE, L.QGD_ERR_UNSUPPORTED
    prob, ctrl, pcof, target = cases.guarded_case(qgd, nsteps=10, tf=5.0)
    N, c = prob.N_tot_levels, prob.N_initial_conditions
    out = np.full((2 * N, 21, c), np.nan, order="F")
    lm, re = np.ones((1, N), order="F"), np.asfortranarray(np.eye(N)[:, :, None])
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        dp.discrete_adjoint(pcof)
        g0, o0 = dp.discrete_adjoint(pcof, history_precomputed=True)
        for what, kw in (("NULL out", dict(out=None)),
                         ("refine < 1", dict(out=out, refine=0)),
                         ("refine < 1", dict(out=out, refine=-2)),
                         ("1 + nsteps * refine beyond int32", dict(out=out, refine=2 ** 28)),
                         ("unknown kind", dict(out=out, kind=3)),
                         ("unknown kind", dict(out=out, kind=-1)),
                         ("populations with level_map and n_groups < 1", dict(out=out, kind=1, lm=lm, ng=0)),
                         ("expectations without obs_re", dict(out=out, kind=2, n_obs=1)),
                         ("expectations with n_obs < 1", dict(out=out, kind=2, re=re, n_obs=0)),
                         ("a pcof of another length", dict(out=out, n=len(pcof) - 1))):
            rc, msg = _raw(dp, pcof, **kw)
            assert rc == A and msg, (what, rc, msg)
            assert np.all(np.isnan(out)), what
            # nothing was launched: the stored sweep and lambda are as the gradient call left them
            g1, o1 = dp.discrete_adjoint(pcof, history_precomputed=True)
            assert np.array_equal(g1, g0) and np.array_equal(o1, o0), what
        rc, msg = _raw(dp, pcof, out)
        assert rc == L.QGD_OK and np.all(np.isfinite(out))
    finally:
        dp.close()
    # history_precomputed on a handle that has evaluated nothing; pcof without a basis; no tables and no pcof
    dp = qgd.DeviceProblem(prob, 4)
    try:
        out[:] = np.nan
        rc, msg = _raw(dp, pcof, out)
        assert rc == S and "qgd_set_control_basis" in msg and np.all(np.isnan(out))
        dp.set_controls(ctrl)
        rc, msg = _raw(dp, pcof, out, hp=1)
        assert rc == S and "history_precomputed" in msg and np.all(np.isnan(out))
        rc, msg = _raw(dp, None, out)
        assert rc == S and "control tables" in msg and np.all(np.isnan(out))
        with pytest.raises(qgd._lib.QGDError) as ei:
            dp.eval_dense_states(2, pcof, history_precomputed=True)
        assert ei.value.code == S
    finally:
        dp.close()
    # a partitioned handle
    rank = qgd.DeviceBackend(prob, 4, ctrl, target, 0, 2)
    try:
        rc, msg = _raw(rank.dp, pcof, out)
        assert rc == U and "partition" in msg and np.all(np.isnan(out))
    finally:
        rank.dp.close()
