"""GPU tests of qgd_eval_expectations: expectation values Re(psi^H O psi) of Hermitian observables
along the sweep, formed on the device from the state panels (csrc/qgd_k_observe.hip, k_expectations).

The yardstick is never the new code: it is the full ``uv_history`` of the existing eval_forward_ / DeviceProblem.eval_forward
on a handle of the same configuration (which the suite pins to the oracle), contracted by numpy.  With w = hist[:, 0] = (u; v)
and O = A + iB:

    ref = u^T A u + v^T A v + v^T B u - u^T B v
    S   = |u|^T|A||u| + |v|^T|A||v| + |v|^T|B||u| + |u|^T|B||v|
    |dev - ref| <= 2 (4N + 2) EPS S,   EPS = 2^-52

Derivation of the bound.  Device and numpy each evaluate two nested inner products of length <= 2N (first (A u, B u) or
(A v, B v): N terms each; then the product with u or v summed over the rows, over the A and the B part and over the u and the
v half: 2N terms twice) plus the products.  The rounding error of such an evaluation, in any order of summation and with or
without fused multiply-adds, is below gamma_{4N+2} S <= (4N + 2) 2^-53 S (Higham, Accuracy and Stability, section 3.1) to
first order.  Two such evaluations differ by at most (4N + 2) EPS S; that is doubled, as the populations tests do.  The bound
uses nothing the device returns.

Against the oracle (setup of test_gpu_parity.py::test_baseline_configs_full_size_vs_oracle[cnot2]): that test allows 5e-11
per state component; sqrt(N) turns it into a 2-norm of the state error, and 2 ||O||_2 ||psi|| with ||psi|| <= 1 is the
derivative of the quadratic form: |dev - ref| <= 2 ||O||_2 sqrt(N) 5e-11.
"""
import ctypes as C

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CASES = ["cnot2", "guarded", "cnot3", "synthetic"]
ORDER = {"cnot2": 8, "guarded": 4, "cnot3": 8, "synthetic": 12}


def _case(qgd, name):
    if name == "cnot2":
        return cases.cnot2_case(qgd) + (ORDER[name],)
    if name == "guarded":
        return cases.guarded_case(qgd) + (ORDER[name],)
    if name == "cnot3":
        return cases.cnot3_case(qgd, nsteps=20) + (ORDER[name],)
    return cases.synthetic_case(qgd) + (ORDER[name],)


def _observables(prob, name):
    """label -> [N, N] matrix: a random complex Hermitian one, a random real symmetric one (NULL obs_im), the identity,
    diag(0 .. N-1) and, for the dispersive problems, their own control operators a_k + a_k^dagger"""
    N = prob.N_tot_levels
    rng = np.random.default_rng(100 + N)
    a = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    b = rng.standard_normal((N, N))
    obs = {"hermitian": a + a.conj().T, "symmetric": b + b.T, "identity": np.eye(N), "number": np.diag(np.arange(N, dtype=float))}
    if name != "synthetic":
        for k, op in enumerate(prob.sym_operators):
            obs[f"control{k}"] = np.array(op, dtype=float)
    return obs


def _uv(qgd, prob, ctrl, pcof, order, save=1):
    hist = np.zeros((prob.real_system_size, 1 + order // 2, 1 + prob.nsteps // save, prob.N_initial_conditions), order="F")
    qgd.eval_forward_(hist, prob, ctrl, pcof, order=order, saveEveryNsteps=save)
    return hist


def _ref(hist, stack):
    """(ref, S) [n_obs, slots, c] of the observables stack [n_obs, N, N] on the states of hist [2N, 1+m, slots, c]"""
    stack = np.asarray(stack)
    if stack.ndim == 2:
        stack = stack[None]
    N = hist.shape[0] // 2
    u, v = hist[:N, 0], hist[N:, 0]
    A, B = np.ascontiguousarray(stack.real), np.ascontiguousarray(stack.imag) if np.iscomplexobj(stack) else np.zeros(stack.shape)

    def form(A, B, u, v, sign):
        Au, Av = np.einsum("oij,jsc->oisc", A, u), np.einsum("oij,jsc->oisc", A, v)
        Bu, Bv = np.einsum("oij,jsc->oisc", B, u), np.einsum("oij,jsc->oisc", B, v)
        return (np.einsum("isc,oisc->osc", u, Au) + np.einsum("isc,oisc->osc", v, Av)
                + np.einsum("isc,oisc->osc", v, Bu) + sign * np.einsum("isc,oisc->osc", u, Bv))

    return form(A, B, u, v, -1.0), form(np.abs(A), np.abs(B), np.abs(u), np.abs(v), 1.0)


def _bound(S, N):
    return 2 * (4 * N + 2) * EPS * S


def _check(dev, hist, stack, what):
    ref, S = _ref(hist, stack)
    N = hist.shape[0] // 2
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    assert dev.flags.f_contiguous and dev.dtype == np.float64, what
    err, bound = np.abs(dev - ref), _bound(S, N)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))
    print(f"\n{what}: expectations max |dev - ref| / bound = {worst:.4f} (N {N}, n_obs {ref.shape[0]}), max abs {err.max():.2e}")
    assert np.all(np.isfinite(dev)), what
    assert np.all(err <= bound), (what, worst)


def _pop_ref(hist):
    N = hist.shape[0] // 2
    u, v = hist[:N, 0], hist[N:, 0]
    return u * u + v * v


def _raw(dp, pcof, re, im, n_obs, out, hp=0):
    """the C ABI directly: planes as given (an explicit all-zero imaginary plane stays one)"""
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    pc = None if pcof is None else np.ascontiguousarray(pcof, dtype=np.float64)
    o3 = np.zeros(3)
    return dp.lib.qgd_eval_expectations(dp.h, vp(pc), 0 if pc is None else len(pc), hp, vp(re), vp(im), n_obs, vp(out), vp(o3))


# -- 1, 2, 3: every kernel branch against uv_history, consistency with eval_populations, determinism ---------------------------

@pytest.mark.parametrize("save", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_expectations_against_uv_history(qgd, name, save):
    prob, ctrl, pcof, target, order = _case(qgd, name)
    N, c = prob.N_tot_levels, prob.N_initial_conditions
    hist = _uv(qgd, prob, ctrl, pcof, order, save)
    obs = _observables(prob, name)
    labels = list(obs)
    stack = np.stack([np.asarray(obs[k], dtype=complex) for k in labels])
    dp = qgd.device_problem(prob, order)
    dp.set_controls(ctrl)
    dp.set_save_every(save)
    try:
        batch = dp.eval_expectations(stack, pcof)                      # imaginary planes present
        o3 = dp.last_scalars.copy()
        o3_ref = np.asarray(dp.eval_forward(pcof))
        assert batch.shape == (len(labels), 1 + prob.nsteps // save, c) and batch.flags.f_contiguous
        _check(batch, hist, stack, f"{name} save {save} batch")
        # (the scalars: a problem with N <= 4 takes the small-problem path for a call without outputs, 1e-12 of the general path)
        assert np.abs(o3 - o3_ref).max() <= 1e-11 * max(1.0, np.abs(o3_ref).max())
        assert np.array_equal(batch, dp.eval_expectations(stack, pcof))                # two calls: the same bits
        # every observable alone (planes in LDS where the batch's did not fit; NULL obs_im for the real ones): what the batch gave
        for j, k in enumerate(labels):
            one = dp.eval_expectations(obs[k], pcof)
            assert one.shape == (1,) + batch.shape[1:]
            if not np.iscomplexobj(obs[k]):
                _check(one, hist, obs[k], f"{name} save {save} {k} alone (real)")
            assert np.array_equal(one[0], batch[j]), (name, k)      # (as values: the determinism test says why, and compares bits)
        real = np.stack([obs[k] for k in labels if not np.iscomplexobj(obs[k])])
        _check(dp.eval_expectations(real, pcof), hist, real, f"{name} save {save} real batch")
        # the identity gives the column sums of eval_populations, diag(d) its contraction with the level map d
        pop = dp.eval_populations(pcof)
        pref = _pop_ref(hist)
        e_id, e_num = batch[labels.index("identity")], batch[labels.index("number")]
        assert np.all(np.abs(e_id - pop.sum(axis=0)) <= _bound(pref.sum(axis=0), N)), name
        d = np.arange(N, dtype=float)
        grouped = dp.eval_populations(pcof, level_map=d[None, :])
        Sd = np.einsum("k,ksc->sc", d, pref)
        assert np.all(np.abs(e_num - grouped[0]) <= _bound(Sd, N) + 2 * (N + 2) * EPS * Sd), name
    finally:
        dp.set_save_every(1)
    # the functional call
    f = qgd.eval_expectations(prob, ctrl, pcof, [obs[k] for k in labels], order=order, saveEveryNsteps=save)
    assert np.array_equal(f, batch)
    qgd.clear_cache()


@pytest.mark.parametrize("name", ["guarded", "synthetic"])
def test_determinism_batches_and_an_explicit_zero_imaginary_plane(qgd, name):
    """A stack of three observables equals three single calls bitwise, with imaginary planes and without: every (observable,
    row block) partial sum is one wave's work whatever else the call holds, and the planes staged in LDS hold the values the
    other path reads from global memory (synthetic: one real observable fits in LDS, three do not).
    A real observable whose imaginary plane is passed explicitly as zeros equals the NULL-obs_im call AS VALUES
    (np.array_equal): every term of the B part is then an exact zero, added to a finite A part it does not change -- only the
    sign of a result that is itself zero could differ, which a bitwise comparison would see and == does not."""
    prob, ctrl, pcof, target, order = _case(qgd, name)
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, 1 + prob.nsteps
    obs = _observables(prob, name)
    rng = np.random.default_rng(7)

    def hermitian():
        a = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        return a + a.conj().T

    bits = lambda x: np.ascontiguousarray(x).view(np.int64)
    dp = qgd.DeviceProblem(prob, order); dp.set_controls(ctrl)
    for three in ([obs["hermitian"], hermitian(), hermitian()], [obs["symmetric"], obs["number"], hermitian().real]):
        batch = dp.eval_expectations(three, pcof)
        assert batch.shape == (3, nt, c) and np.abs(batch).max() > 0
        assert np.array_equal(bits(batch), bits(dp.eval_expectations(three, pcof)))
        for j, o in enumerate(three):
            assert np.array_equal(bits(dp.eval_expectations(o, pcof)[0]), bits(batch[j])), (name, j)
    re = np.asfortranarray(obs["symmetric"][:, :, None])
    null_im, zero_im = np.zeros((1, nt, c), order="F"), np.zeros((1, nt, c), order="F")
    assert _raw(dp, pcof, re, None, 1, null_im) == 0
    assert _raw(dp, pcof, re, np.zeros((N, N, 1), order="F"), 1, zero_im) == 0
    assert np.abs(null_im).max() > 0 and np.array_equal(null_im, zero_im)
    assert np.array_equal(null_im, dp.eval_expectations(obs["symmetric"], pcof))
    dp.close()


# -- 4: the fused front --------------------------------------------------------------------------------------------------------

def test_fused_front(qgd):
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=550, tf=550.0)
    obs = _observables(prob, "cnot3")
    stack = np.stack([np.asarray(o, dtype=complex) for o in obs.values()])
    dp = qgd.DeviceProblem(prob, 8); dp.set_controls(ctrl); dp.set_target(target)
    hist = np.zeros(dp._hist_shape(), order="F")
    dp.eval_forward(pcof, hist)
    assert dp.front_path_taken()
    fresh = dp.eval_expectations(stack, pcof)
    _check(fresh, hist, stack, "front")
    assert dp.front_path_taken()
    stored = dp.eval_expectations(stack, pcof, history_precomputed=True)
    _check(stored, hist, stack, "front, stored sweep")
    _check(dp.eval_expectations(obs["symmetric"], pcof, history_precomputed=True), hist, obs["symmetric"], "front, stored sweep, real")
    dp.set_save_every(3)
    hist3 = np.zeros(dp._hist_shape(3), order="F")
    dp.eval_forward(pcof, hist3)
    _check(dp.eval_expectations(stack, pcof), hist3, stack, "front save 3")
    assert dp.front_path_taken()
    dp.close()


# -- 5: a windowed grid --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("save", [1, 3])
def test_windowed_grid(qgd, save):
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=64, tf=64.0)
    obs = _observables(prob, "cnot3")
    stack = np.stack([np.asarray(o, dtype=complex) for o in obs.values()])
    probe = qgd.DeviceProblem(prob, 8)
    full = probe.memory_plan()["window_bytes"]
    probe.close()
    dp = qgd.DeviceProblem(prob, 8)
    dp.set_memory_budget(int(full / 4 * 1.15))
    dp.set_controls(ctrl); dp.set_target(target)
    assert dp.memory_plan()["windows"] >= 3, dp.memory_plan()
    dp.set_save_every(save)
    hist = np.zeros(dp._hist_shape(save), order="F")
    dp.eval_forward(pcof, hist)
    assert np.abs(hist[:, 0, -1]).max() > 0
    _check(dp.eval_expectations(stack, pcof), hist, stack, f"windowed save {save}")
    _check(dp.eval_expectations(stack, pcof, history_precomputed=True), hist, stack, f"windowed save {save}, history_precomputed")
    _check(dp.eval_expectations(obs["symmetric"], pcof), hist, obs["symmetric"], f"windowed save {save}, real")
    # the windowed sweep stays usable: the gradient from the stored window-boundary states (bound of test_gpu_memory.py)
    g0, _ = dp.discrete_adjoint(pcof)
    dp.eval_expectations(stack, pcof)
    g1, _ = dp.discrete_adjoint(pcof, history_precomputed=True)
    assert np.abs(g1 - g0).max() <= 1e-11 * np.abs(g0).max()
    dp.close()


# -- 6: the stored sweep -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cnot2", "cnot3"])
def test_the_stored_sweep(qgd, name):
    """eval_expectations leaves the sweep record as eval_forward without an output array does: a history_precomputed gradient
    after it has the bits of the one after eval_forward.  history_precomputed with another pcof redoes the sweep."""
    prob, ctrl, pcof, target, order = _case(qgd, name)
    pcof2 = 0.5 * pcof[::-1].copy()
    O = _observables(prob, name)["hermitian"]
    h1, h2 = _uv(qgd, prob, ctrl, pcof, order), _uv(qgd, prob, ctrl, pcof2, order)
    assert np.abs(_ref(h1, O)[0] - _ref(h2, O)[0]).max() > 1e-8
    qgd.clear_cache()

    def handle():
        d = qgd.DeviceProblem(prob, order); d.set_controls(ctrl); d.set_target(target)
        return d

    d = handle(); d.eval_expectations(O, pcof); g_exp, o_exp = d.discrete_adjoint(pcof, history_precomputed=True); d.close()
    d = handle(); d.eval_forward(pcof); g_fwd, o_fwd = d.discrete_adjoint(pcof, history_precomputed=True); d.close()
    assert np.array_equal(g_exp, g_fwd) and np.array_equal(o_exp, o_fwd)
    d = handle()
    o3 = np.asarray(d.eval_forward(pcof))
    _check(d.eval_expectations(O, pcof, history_precomputed=True), h1, O, f"{name} after eval_forward")
    assert np.abs(d.last_scalars - o3).max() <= 1e-11 * max(1.0, np.abs(o3).max())
    d.discrete_adjoint(pcof)
    _check(d.eval_expectations(O, pcof, history_precomputed=True), h1, O, f"{name} after discrete_adjoint")
    _check(d.eval_expectations(O, pcof2, history_precomputed=True), h2, O, f"{name} after another pcof (sweep redone)")
    _check(d.eval_expectations(O, pcof2, history_precomputed=True), h2, O, f"{name} once more (now stored)")
    d.close()


# -- 7: tables set directly, pinned outputs ------------------------------------------------------------------------------------

def test_tables_set_directly_and_a_pinned_output(qgd):
    from qgd_amd.controls import control_tables_general
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=20)
    order = 8
    obs = _observables(prob, "cnot3")
    stack = np.stack([np.asarray(o, dtype=complex) for o in obs.values()])
    hist = _uv(qgd, prob, ctrl, pcof, order)
    qgd.clear_cache()
    p, q, _, _ = control_tables_general(ctrl, np.asarray(pcof, float), prob.nsteps, prob.tf, order // 2)
    dp = qgd.DeviceProblem(prob, order)
    dp.set_control_tables(p, q)
    h2 = np.zeros(hist.shape, order="F")
    dp.eval_forward(None, h2)
    assert np.abs(h2 - hist).max() <= 1e-12
    _check(dp.eval_expectations(stack, None), h2, stack, "tables set directly")
    _check(dp.eval_expectations(obs["symmetric"], None), h2, obs["symmetric"], "tables set directly, real")
    dp.close()
    dp = qgd.DeviceProblem(prob, order); dp.set_controls(ctrl)
    pinned = dp.pin(np.zeros((len(stack), 1 + dp.nsteps, dp.c), order="F"))
    assert dp.eval_expectations(stack, pcof, out=pinned) is pinned
    _check(pinned, hist, stack, "pinned")
    unpinned = dp.eval_expectations(stack, pcof)
    assert np.array_equal(unpinned.view(np.int64), pinned.view(np.int64))
    with pytest.raises(ValueError):
        dp.eval_expectations(stack, pcof, out=np.zeros((len(stack), 1 + dp.nsteps, dp.c + 1), order="F"))
    with pytest.raises(ValueError):
        dp.eval_expectations(stack, pcof, out=np.zeros((len(stack), 1 + dp.nsteps, dp.c)))      # C order
    dp.close()


# -- 8: against the oracle -----------------------------------------------------------------------------------------------------

def test_against_the_oracle_cnot2_full_size(qgd, orc):
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=100, tf=100.0)
    prob.gmres_abstol = prob.gmres_reltol = 1e-15
    orc.set_converged_terminal(True)
    try:
        _, h_ref, _, _, _ = orc.discrete_adjoint(prob, ctrl, pcof, target, order=8, return_all=True)
    finally:
        orc.set_converged_terminal(False)
    N = prob.N_tot_levels
    O = _observables(prob, "cnot2")["hermitian"]
    dev = qgd.eval_expectations(prob, ctrl, pcof, O, order=8)
    ref, _ = _ref(h_ref, O)
    bound = 2 * np.linalg.norm(O, 2) * np.sqrt(N) * 5e-11
    err = np.abs(dev - ref).max()
    print(f"\ncnot2 (100 steps, order 8): expectations vs the oracle's history, max abs {err:.2e} (bound {bound:.2e})")
    assert dev.shape == ref.shape and err <= bound
    qgd.clear_cache()


# -- 9: refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals(qgd):
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=20)
    obs = _observables(prob, "cnot3")
    O = obs["hermitian"]
    hist = _uv(qgd, prob, ctrl, pcof, 8)
    qgd.clear_cache()
    dp = qgd.DeviceProblem(prob, 8); dp.set_controls(ctrl)
    N, nt, c = dp.N, dp.nsteps + 1, dp.c
    re, im = qgd.observable_planes(O, N)
    out = np.zeros((1, nt, c), order="F")
    A, S, U = qgd._lib.QGD_ERR_ARGUMENT, qgd._lib.QGD_ERR_STATE, qgd._lib.QGD_ERR_UNSUPPORTED
    assert _raw(dp, pcof, re, im, 1, out, hp=1) == S                   # a fresh handle has no forward evaluation to reuse
    _check(dp.eval_expectations(O, pcof), hist, O, "after QGD_ERR_STATE")
    assert _raw(dp, pcof, re, im, 1, None) == A                        # NULL output
    _check(dp.eval_expectations(O, pcof), hist, O, "after a NULL output")
    assert _raw(dp, pcof, re, im, 0, out) == A and _raw(dp, pcof, re, im, -3, out) == A      # n_obs < 1
    _check(dp.eval_expectations(O, pcof), hist, O, "after n_obs = 0")
    assert _raw(dp, pcof, None, im, 1, out) == A                       # NULL obs_re
    assert not out.any()
    _check(dp.eval_expectations(O, pcof), hist, O, "after a NULL obs_re")
    # Python: not Hermitian, wrong size -- ValueError before the library is called (the stored scalars are those of the last call)
    dp.last_scalars = None
    for bad in (np.triu(np.ones((N, N))), np.eye(N + 1), 1j * np.eye(N)):
        with pytest.raises(ValueError):
            dp.eval_expectations(bad, pcof)
        with pytest.raises(ValueError):
            qgd.eval_expectations(prob, ctrl, pcof, bad, order=8)
    assert dp.last_scalars is None
    dp.close()
    dp = qgd.DeviceProblem(prob, 8); dp.set_controls(ctrl)
    with pytest.raises(qgd._lib.QGDError) as e:
        dp.eval_expectations(O, pcof, history_precomputed=True)
    assert e.value.code == S
    dp.close()
    qgd.clear_cache()
    # a partitioned handle: the call is single-GPU
    dp = qgd.DeviceProblem(prob, 8)
    qgd._lib.check(dp.h, dp.lib.qgd_set_partition(dp.h, 0, 2))
    assert _raw(dp, pcof, re, im, 1, out) == U
    with pytest.raises(qgd._lib.QGDError) as e:
        dp.eval_expectations(O, pcof)
    assert e.value.code == U
    assert not out.any()
    dp.close()
    # a handle evaluates correctly after the refusal of another configuration of the same problem
    dp = qgd.DeviceProblem(prob, 8); dp.set_controls(ctrl)
    _check(dp.eval_expectations(O, pcof), hist, O, "after QGD_ERR_UNSUPPORTED")
    dp.close()
