"""GPU tests of the handle's on-demand buffer pools (csrc/qgd_host.h: Pool): the forced gradient's, the Hessian's, the
Hessian-vector product's, the pullback's, the dense output's and the forced forward sweep's.  Each test walks one handle through
changes of a pool's key that the tests of the entry points themselves do not reach -- another refine, other upload lengths,
another grid, a windowed grid, other entry points in between, a refused allocation -- and after every step compares the result
bit for bit with that of a fresh handle configured the same way."""
import re

import numpy as np
import pytest

import cases
from test_gpu_pullback import _hermitian

pytestmark = pytest.mark.gpu

ORDER = 4
CASES = {
    "guarded": lambda q: cases.guarded_case(q, nsteps=10, tf=5.0),      # N = 9, Np = 16: padded panels, the guard's buffers
    "cnot2": lambda q: cases.cnot2_case(q, nsteps=24, tf=24.0),         # 24 steps: more than one scan block
}


class Walk:
    """One handle and how it was configured: `check` runs a call on it and on a fresh handle configured the same way."""

    def __init__(self, qgd, name):
        self.qgd = qgd
        self.prob, self.ctrl, self.pcof, self.target = CASES[name](qgd)
        self.grid = self.budget = None
        self.dp = self._open()

    def _open(self):
        d = self.qgd.DeviceProblem(self.prob, ORDER)
        try:
            if self.grid:
                d.set_nsteps(*self.grid)
            if self.budget:
                d.set_memory_budget(self.budget)
            d.set_controls(self.ctrl); d.set_target(self.target)
        except BaseException:
            d.close()
            raise
        return d

    def set_nsteps(self, nsteps, tf):
        self.grid = (nsteps, tf)
        self.dp.set_nsteps(nsteps, tf)
        self.dp.set_controls(self.ctrl); self.dp.set_target(self.target)

    def set_memory_budget(self, nbytes):
        self.budget = nbytes
        self.dp.set_memory_budget(nbytes)
        self.dp.set_controls(self.ctrl); self.dp.set_target(self.target)

    def check(self, call, what):
        got = call(self.dp)
        fresh = self._open()
        try:
            ref = call(fresh)
        finally:
            fresh.close()
        assert np.all(np.isfinite(got)) and np.array_equal(got, ref), what
        return got

    def close(self):
        self.dp.close()


@pytest.mark.parametrize("name", list(CASES))
def test_dense_pool_follows_refine_and_dt(qgd, name):
    w = Walk(qgd, name)
    dense = lambda r: (lambda d: d.eval_dense_states(r, w.pcof))
    try:
        for r in (3, 5, 3):                           # the weight table and the panels are made anew each time
            w.check(dense(r), f"refine {r}")
        nsteps, tf = w.prob.nsteps, w.prob.tf
        before = w.dp.eval_dense_states(3, w.pcof)
        w.set_nsteps(nsteps, 0.8 * tf)                # the same points: of the key, only dt differs
        after = w.check(dense(3), "refine 3 at another dt")
        assert after.shape == before.shape and not np.array_equal(after, before)
    finally:
        w.close()


@pytest.mark.parametrize("name", list(CASES))
def test_pullback_pool_follows_the_upload_lengths(qgd, name):
    w = Walk(qgd, name)
    N, c, nt = w.prob.N_tot_levels, w.prob.N_initial_conditions, w.prob.nsteps + 1
    rng = np.random.default_rng(11)
    sb, pb, eb = rng.standard_normal((2 * N, nt, c)), rng.standard_normal((2, nt, c)), rng.standard_normal((3, nt, c))
    lm, obs = rng.standard_normal((2, N)), _hermitian(rng, 3, N)
    calls = (("states_bar", lambda d: d.eval_pullback(w.pcof, states_bar=sb)),
             ("states_bar and populations_bar with a level map", lambda d: d.eval_pullback(w.pcof, states_bar=sb, populations_bar=pb, level_map=lm)),
             ("expectations_bar with complex observables", lambda d: d.eval_pullback(w.pcof, expectations_bar=eb, observables=obs)))
    try:
        first = w.check(calls[0][1], calls[0][0])     # nt and n_pcof stay: of the key, only the upload lengths change
        for what, call in calls[1:]:
            w.check(call, what)
        assert np.array_equal(w.check(calls[0][1], "states_bar again"), first)
    finally:
        w.close()


def test_forced_pools_follow_the_grid_and_its_windows(qgd):
    w = Walk(qgd, "cnot2")
    N, c, m = w.prob.N_tot_levels, w.prob.N_initial_conditions, ORDER // 2
    rng = np.random.default_rng(12)

    def forced_forward(ff):
        def call(d):
            hist = np.full((2 * N, m + 1, d.nsteps + 1, c), np.nan, order="F")
            scal = np.ravel(np.asarray(d.eval_forward_forced(w.pcof, ff, hist), dtype=float))
            return np.concatenate([scal, hist.ravel(order="F")])
        return call

    def both(what):
        ff = np.asfortranarray(0.2 * rng.standard_normal((2 * N, m, w.dp.nsteps + 1, c)))
        w.check(forced_forward(ff), f"eval_forward_forced, {what}")
        w.check(lambda d: d.eval_grad_forced(w.pcof), f"eval_grad_forced, {what}")

    try:
        both("the grid of the problem")
        w.set_nsteps(37, w.prob.tf)
        both("37 steps")
        w.set_memory_budget(w.dp.memory_plan()["window_bytes"] // 3)
        assert w.dp.memory_plan()["windows"] >= 2
        both("37 steps in windows")
    finally:
        w.close()


@pytest.mark.parametrize("name", list(CASES))
def test_pools_do_not_disturb_each_other(qgd, name):
    w = Walk(qgd, name)
    N, c, nt = w.prob.N_tot_levels, w.prob.N_initial_conditions, w.prob.nsteps + 1
    rng = np.random.default_rng(13)
    v, sb = rng.standard_normal(len(w.pcof)), rng.standard_normal((2 * N, nt, c))
    calls = (("eval_hessian", lambda d: d.eval_hessian(w.pcof)),
             ("eval_hessian_vec", lambda d: d.eval_hessian_vec(w.pcof, v)),
             ("eval_pullback", lambda d: d.eval_pullback(w.pcof, states_bar=sb)),
             ("eval_dense_states", lambda d: d.eval_dense_states(3, w.pcof)))
    try:
        first = {what: w.check(call, what) for what, call in calls}
        for what, call in reversed(calls):
            assert np.array_equal(call(w.dp), first[what]), f"{what}, in reverse order"
    finally:
        w.close()


def test_a_refused_pool_leaves_the_handle_usable(qgd):
    """tests/test_gpu_dense_output.py::test_panels_beyond_the_memory_budget_are_refused on the pullback: under a budget that holds
    the grid (8 windows' worth: room for the Hessian-vector product's buffers as well) the planes of enough observables do not
    fit.  What the pullback needs is read from the refusal, as test_memory_refusal_reports_the_deciding_byte_count does."""
    L = qgd._lib
    w = Walk(qgd, "guarded")
    N, c, nt = w.prob.N_tot_levels, w.prob.N_initial_conditions, w.prob.nsteps + 1
    rng = np.random.default_rng(14)
    v, sb = rng.standard_normal(len(w.pcof)), rng.standard_normal((2 * N, nt, c))
    try:
        window = w.dp.memory_plan()["window_bytes"]
        w.set_memory_budget(8 * window)
        budget = w.dp.memory_plan()["budget"]
        assert w.dp.memory_plan()["windows"] == 1 and budget == 8 * window
        g0, o0 = w.dp.discrete_adjoint(w.pcof)
        hv0 = w.dp.eval_hessian_vec(w.pcof, v)
        p0 = w.dp.eval_pullback(w.pcof, states_bar=sb)
        n_obs = 1 + budget // (8 * N * N)             # real planes [N, N, n_obs] that alone exceed the budget
        obs = np.broadcast_to(np.eye(N), (n_obs, N, N))
        with pytest.raises(L.QGDError) as ei:
            w.dp.eval_pullback(w.pcof, expectations_bar=np.ones((n_obs, nt, c)), observables=obs)
        msg = w.dp.lib.qgd_last_error(w.dp.h).decode()
        assert ei.value.code == L.QGD_ERR_MEMORY, msg
        need = int(re.search(r"\((\d+) bytes needed\)", msg).group(1))
        print(f"\nguarded: window {window} bytes, budget {budget}, the refused pullback needs {need}")
        assert window < budget < need
        g1, o1 = w.dp.discrete_adjoint(w.pcof)
        assert np.array_equal(g1, g0) and np.array_equal(o1, o0)
        assert np.array_equal(w.dp.eval_hessian_vec(w.pcof, v), hv0)
        assert np.array_equal(w.check(lambda d: d.eval_pullback(w.pcof, states_bar=sb), "the pullback after its refusal"), p0)
    finally:
        w.close()
