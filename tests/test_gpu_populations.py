"""GPU tests of qgd_eval_states / qgd_eval_populations: the state trajectory and the level
populations along the sweep, taken from the device's state panels without the stage derivatives.

The yardstick is always the full ``uv_history`` of the existing eval_forward_ / DeviceProblem.eval_forward on a handle of
the same configuration (which the suite pins to the oracle), never the new code itself:
  states            bitwise (the same panels through the same re-layout kernel)
  populations       |dev - ref| <= 4 eps ref, ref = u*u + v*v by numpy, eps = 2^-52: u*u + v*v and fma(u, u, v*v) are each within
                    2 * 2^-53 relative of the exact sum of two non-negative terms, so they differ by at most 2 eps; twice that
  grouped           |dev - M @ ref| <= 2 (N + 2) eps (|M| @ ref): the bound of a length-N dot product of non-negative data
                    summed in any order, doubled
  against the oracle  1e-10 absolute on the setup of test_gpu_parity.py::test_baseline_configs_full_size_vs_oracle[cnot2]:
                    twice the 5e-11 that test allows for the state history (|psi_k| <= 1, so dp <= 2 |psi_k| dpsi)
"""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CASES = ["cnot2-o2", "cnot2-o4", "cnot2-o8", "guarded", "cnot3", "synthetic"]
SIZES = {"cnot2": (2, 2), "guarded": (3, 3), "cnot3": (4, 4, 4), "synthetic": (4, 25)}


def _case(qgd, name):
    if name.startswith("cnot2"):
        return cases.cnot2_case(qgd) + (int(name[-1]),)
    if name == "guarded":
        return cases.guarded_case(qgd) + (4,)
    if name == "cnot3":
        return cases.cnot3_case(qgd, nsteps=20) + (8,)
    return cases.synthetic_case(qgd) + (12,)


def _uv(qgd, prob, ctrl, pcof, order, save=1, forcing=None):
    hist = np.zeros((prob.real_system_size, 1 + order // 2, 1 + prob.nsteps // save, prob.N_initial_conditions), order="F")
    qgd.eval_forward_(hist, prob, ctrl, pcof, order=order, saveEveryNsteps=save, forcing=forcing)
    return hist


def _pop_ref(hist):
    N = hist.shape[0] // 2
    u, v = hist[:N, 0], hist[N:, 0]
    return u * u + v * v


def _check_pop(dev, ref, what):
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    err = np.abs(dev - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(ref > 0, err / (EPS * ref), np.where(err > 0, np.inf, 0.0)))
    print(f"\n{what}: populations max |dev - ref| / (eps ref) = {worst:.2f} (bound 4), max abs {err.max():.2e}")
    assert np.all(err <= 4 * EPS * ref), (what, worst)


def _check_grouped(dev, M, ref, what):
    N = ref.shape[0]
    want = np.einsum("gk,ksc->gsc", M, ref)
    bound = 2 * (N + 2) * EPS * np.einsum("gk,ksc->gsc", np.abs(M), ref)
    assert dev.shape == want.shape, (what, dev.shape, want.shape)
    err = np.abs(dev - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))
    print(f"\n{what}: grouped max |dev - M ref| / bound = {worst:.3f} (n_groups {M.shape[0]}, N {N})")
    assert np.all(err <= bound), (what, worst)


def _maps(qgd, name, N):
    key = name.split("-")[0]
    maps = {"random5": np.random.default_rng(11).standard_normal((5, N)), "subsystem": qgd.subsystem_population_map(SIZES[key])}
    if N == 100:
        maps["wide"] = np.random.default_rng(12).standard_normal((N + 3, N))      # does not fit in LDS beside the populations
    return maps


@pytest.mark.parametrize("save", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_states_are_a_copy_and_eval_forward_is_unchanged(qgd, name, save):
    prob, ctrl, pcof, target, order = _case(qgd, name)
    hist = _uv(qgd, prob, ctrl, pcof, order, save)
    dp = qgd.device_problem(prob, order)
    dp.set_controls(ctrl)
    dp.set_save_every(save)
    try:
        st = dp.eval_states(pcof)
        o3 = dp.last_scalars.copy()
        o3_ref = dp.eval_forward(pcof)
    finally:
        dp.set_save_every(1)
    assert st.shape == (hist.shape[0],) + hist.shape[2:] and st.flags.f_contiguous
    assert np.array_equal(st, hist[:, 0])
    # (the scalars: a problem with N <= 4 takes the small-problem path for a call without outputs, 1e-12 of the general path)
    assert np.abs(o3 - np.asarray(o3_ref)).max() <= 1e-11 * max(1.0, np.abs(o3_ref).max())
    # the allocating eval_forward takes the state-only route: the same bits as before
    psi = qgd.eval_forward(prob, ctrl, pcof, order=order, saveEveryNsteps=save)
    assert np.array_equal(psi, qgd.real_to_complex(hist[:, 0]))
    qgd.clear_cache()


@pytest.mark.parametrize("name", CASES)
def test_states_with_a_forcing(qgd, name):
    prob, ctrl, pcof, target, order = _case(qgd, name)
    forcing = 0.1 * np.asfortranarray(np.random.default_rng(5).standard_normal(
        (prob.real_system_size, order // 2, 1 + prob.nsteps, prob.N_initial_conditions)))
    for save in (1, 3):
        hist = _uv(qgd, prob, ctrl, pcof, order, save, forcing=forcing)
        dp = qgd.device_problem(prob, order)
        dp.set_controls(ctrl)
        dp.set_save_every(save)
        try:
            st = dp.eval_states(pcof, forcing=forcing)
        finally:
            dp.set_save_every(1)
        assert np.array_equal(st, hist[:, 0]), save
        psi = qgd.eval_forward(prob, ctrl, pcof, order=order, saveEveryNsteps=save, forcing=forcing)
        assert np.array_equal(psi, qgd.real_to_complex(hist[:, 0])), save
    assert np.abs(hist[:, 0] - _uv(qgd, prob, ctrl, pcof, order, 3)[:, 0]).max() > 1e-6      # (the forcing did something)
    qgd.clear_cache()


@pytest.mark.parametrize("save", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_populations(qgd, name, save):
    prob, ctrl, pcof, target, order = _case(qgd, name)
    ref = _pop_ref(_uv(qgd, prob, ctrl, pcof, order, save))
    dev = qgd.eval_populations(prob, ctrl, pcof, order=order, saveEveryNsteps=save)
    _check_pop(dev, ref, f"{name} save {save}")
    assert np.array_equal(dev, qgd.eval_populations(prob, ctrl, pcof, order=order, saveEveryNsteps=save))      # reproducible
    qgd.clear_cache()


@pytest.mark.parametrize("save", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_grouped_populations(qgd, name, save):
    prob, ctrl, pcof, target, order = _case(qgd, name)
    N = prob.N_tot_levels
    ref = _pop_ref(_uv(qgd, prob, ctrl, pcof, order, save))
    total = ref.sum(axis=0)
    for label, M in _maps(qgd, name, N).items():
        dev = qgd.eval_populations(prob, ctrl, pcof, order=order, saveEveryNsteps=save, level_map=M)
        _check_grouped(dev, M, ref, f"{name} save {save} {label}")
        assert np.array_equal(dev, qgd.eval_populations(prob, ctrl, pcof, order=order, saveEveryNsteps=save, level_map=M))
        if label == "subsystem":      # the level populations of every subsystem add up to the norm of the state
            row = 0
            for s in SIZES[name.split("-")[0]]:
                assert np.all(np.abs(dev[row:row + s].sum(axis=0) - total) <= 2 * (N + 2) * EPS * total), (name, label, row)
                row += s
    qgd.clear_cache()


def test_populations_against_the_oracle_cnot2_full_size(qgd, orc):
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=100, tf=100.0)
    prob.gmres_abstol = prob.gmres_reltol = 1e-15
    orc.set_converged_terminal(True)
    try:
        _, h_ref, _, _, _ = orc.discrete_adjoint(prob, ctrl, pcof, target, order=8, return_all=True)
    finally:
        orc.set_converged_terminal(False)
    dev = qgd.eval_populations(prob, ctrl, pcof, order=8)
    err = np.abs(dev - _pop_ref(h_ref)).max()
    print(f"\ncnot2 (100 steps, order 8): populations vs the oracle's u^2 + v^2, max abs {err:.2e} (bound 1e-10)")
    assert err <= 1e-10
    assert np.array_equal(qgd.get_populations(h_ref), _pop_ref(h_ref))
    qgd.clear_cache()


def _all_observables(qgd, dp, pcof, hist, what, sizes=(4, 4, 4), **kw):
    """states, populations and grouped populations of one handle against its own uv_history"""
    ref = _pop_ref(hist)
    assert np.array_equal(dp.eval_states(pcof), hist[:, 0]), what
    _check_pop(dp.eval_populations(pcof, **kw), ref, what)
    for label, M in (("random5", np.random.default_rng(11).standard_normal((5, ref.shape[0]))), ("subsystem", qgd.subsystem_population_map(sizes))):
        _check_grouped(dp.eval_populations(pcof, level_map=M, **kw), M, ref, f"{what} {label}")


def test_fused_front_layout(qgd):
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=550, tf=550.0)
    dp = qgd.DeviceProblem(prob, 8); dp.set_controls(ctrl); dp.set_target(target)
    hist = np.zeros(dp._hist_shape(), order="F")
    dp.eval_forward(pcof, hist)
    assert dp.front_path_taken()
    _all_observables(qgd, dp, pcof, hist, "front")
    assert dp.front_path_taken()
    _all_observables(qgd, dp, pcof, hist, "front, stored sweep", history_precomputed=True)
    dp.set_save_every(3)
    hist3 = np.zeros(dp._hist_shape(3), order="F")
    dp.eval_forward(pcof, hist3)
    _all_observables(qgd, dp, pcof, hist3, "front save 3")
    assert dp.front_path_taken()
    dp.close()


@pytest.mark.parametrize("save", [1, 3])
def test_windowed_grid(qgd, save):
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=64, tf=64.0)
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
    _all_observables(qgd, dp, pcof, hist, f"windowed save {save}")
    _all_observables(qgd, dp, pcof, hist, f"windowed save {save}, history_precomputed", history_precomputed=True)
    # the windowed sweep stays usable: the gradient from the stored window-boundary states (bound of test_gpu_memory.py)
    g0, _ = dp.discrete_adjoint(pcof)
    dp.eval_populations(pcof)
    g1, _ = dp.discrete_adjoint(pcof, history_precomputed=True)
    assert np.abs(g1 - g0).max() <= 1e-11 * np.abs(g0).max()
    # a forcing on the windowed grid
    forcing = 0.1 * np.asfortranarray(np.random.default_rng(5).standard_normal((2 * dp.N, dp.m, 1 + dp.nsteps, dp.c)))
    dp.eval_forward_forced(pcof, forcing, hist)
    assert np.array_equal(dp.eval_states(pcof, forcing=forcing), hist[:, 0])
    dp.close()


@pytest.mark.parametrize("name", ["cnot2-o4", "cnot3"])
def test_history_precomputed_and_the_stored_sweep(qgd, name, monkeypatch):
    """history_precomputed reuses the stored sweep under the rule of discrete_adjoint, and eval_populations leaves the sweep
    as eval_forward does: a history_precomputed gradient after it has the bits of the gradient after eval_forward, and the
    bits of a fresh discrete_adjoint wherever the fresh evaluation forms its terminal condition with the kernel a reusing
    one uses.  On the N = 64 chains a fresh full evaluation fuses the terminal condition into its first adjoint launch
    (qgdk_terminal_can_fuse), which adds the overlaps up in another order: there the library's own eval_forward +
    history_precomputed gradient differs from a fresh one in the last bit (measured on cnot3, 20 steps: 1.65e-16 relative),
    before this feature and after it.  So on cnot3 the bits are compared with the stand-alone terminal kernel selected for
    the fresh evaluation too (QGD_PATHS=terminal_kernel), and on the library's own paths at the 1e-13 that
    tests/test_gpu_front.py allows between a fresh and a reusing gradient."""
    prob, ctrl, pcof, target, order = _case(qgd, name)
    pcof2 = 0.5 * pcof[::-1].copy()
    ref, ref2 = _pop_ref(_uv(qgd, prob, ctrl, pcof, order)), _pop_ref(_uv(qgd, prob, ctrl, pcof2, order))
    assert np.abs(ref - ref2).max() > 1e-8
    qgd.clear_cache()

    def handle():
        d = qgd.DeviceProblem(prob, order); d.set_controls(ctrl); d.set_target(target)
        return d

    dp = handle()
    with pytest.raises(qgd._lib.QGDError) as e:
        dp.eval_populations(pcof, history_precomputed=True)      # nothing to reuse yet
    assert e.value.code == qgd._lib.QGD_ERR_STATE
    o3 = np.asarray(dp.eval_forward(pcof))
    _check_pop(dp.eval_populations(pcof, history_precomputed=True), ref, f"{name} after eval_forward")
    assert np.abs(dp.last_scalars - o3).max() <= 1e-11 * max(1.0, np.abs(o3).max())      # (small-problem path: 1e-12 of the general one)
    dp.discrete_adjoint(pcof)
    _check_pop(dp.eval_populations(pcof, history_precomputed=True), ref, f"{name} after discrete_adjoint")
    _check_pop(dp.eval_populations(pcof2, history_precomputed=True), ref2, f"{name} after another pcof (sweep redone)")
    _check_pop(dp.eval_populations(pcof2, history_precomputed=True), ref2, f"{name} once more (now stored)")
    dp.close()

    def three_gradients():
        d = handle(); g_fresh, o_fresh = d.discrete_adjoint(pcof); d.close()
        d = handle(); d.eval_populations(pcof); g_pop, o_pop = d.discrete_adjoint(pcof, history_precomputed=True); d.close()
        d = handle(); d.eval_forward(pcof); g_fwd, o_fwd = d.discrete_adjoint(pcof, history_precomputed=True); d.close()
        assert np.array_equal(g_pop, g_fwd) and np.array_equal(o_pop, o_fwd)      # the sweep is left as eval_forward leaves it
        print(f"\n{name}: gradient after eval_populations vs fresh, max rel diff {np.abs(g_pop - g_fresh).max() / np.abs(g_fresh).max():.2e}")
        return g_fresh, g_pop

    g_fresh, g_pop = three_gradients()
    if name.startswith("cnot2"):
        assert np.array_equal(g_pop, g_fresh)
    else:
        assert np.abs(g_pop - g_fresh).max() <= 1e-13 * np.abs(g_fresh).max()
        monkeypatch.setenv("QGD_PATHS", "terminal_kernel")
        g_fresh, g_pop = three_gradients()
        assert np.array_equal(g_pop, g_fresh)


def test_tables_set_directly_and_pinned_outputs(qgd):
    from qgd_amd.controls import control_tables_general
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=20)
    order = 8
    hist = _uv(qgd, prob, ctrl, pcof, order)
    ref = _pop_ref(hist)
    qgd.clear_cache()
    # pcof = NULL, the tables set by the caller
    p, q, _, _ = control_tables_general(ctrl, np.asarray(pcof, float), prob.nsteps, prob.tf, order // 2)
    dp = qgd.DeviceProblem(prob, order)
    dp.set_control_tables(p, q)
    h2 = np.zeros(hist.shape, order="F")
    dp.eval_forward(None, h2)
    assert np.abs(h2 - hist).max() <= 1e-12
    assert np.array_equal(dp.eval_states(None), h2[:, 0])
    _check_pop(dp.eval_populations(None), _pop_ref(h2), "tables set directly")
    M = qgd.subsystem_population_map((4, 4, 4))
    _check_grouped(dp.eval_populations(None, level_map=M), M, _pop_ref(h2), "tables set directly, subsystem")
    dp.close()
    # the same through controls that are not linear in pcof (tables uploaded per evaluation, NULL pcof underneath)
    dp = qgd.DeviceProblem(prob, order); dp.set_controls([cases.PointwiseOnly(c) for c in ctrl])
    h3 = np.zeros(hist.shape, order="F")
    dp.eval_forward(pcof, h3)
    assert np.array_equal(dp.eval_states(pcof), h3[:, 0])
    _check_pop(dp.eval_populations(pcof), _pop_ref(h3), "pointwise controls")
    dp.close()
    # registered (pinned) output arrays
    dp = qgd.DeviceProblem(prob, order); dp.set_controls(ctrl)
    st = dp.pin(np.zeros((2 * dp.N, 1 + dp.nsteps, dp.c), order="F"))
    pp = dp.pin(np.zeros((dp.N, 1 + dp.nsteps, dp.c), order="F"))
    pg = dp.pin(np.zeros((M.shape[0], 1 + dp.nsteps, dp.c), order="F"))
    assert dp.eval_states(pcof, out=st) is st and np.array_equal(st, hist[:, 0])
    assert dp.eval_populations(pcof, out=pp) is pp
    _check_pop(pp, ref, "pinned")
    dp.eval_populations(pcof, level_map=M, out=pg)
    _check_grouped(pg, M, ref, "pinned, subsystem")
    unpinned = dp.eval_populations(pcof)
    assert np.array_equal(unpinned, pp)
    dp.close()


def test_refusals(qgd):
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=20)
    dp = qgd.DeviceProblem(prob, 8); dp.set_controls(ctrl)
    N, nt, c = dp.N, dp.nsteps + 1, dp.c
    with pytest.raises(ValueError):
        dp.eval_populations(pcof, out=np.zeros((N, nt, c + 1), order="F"))
    with pytest.raises(ValueError):
        dp.eval_populations(pcof, out=np.zeros((N, nt, c)))                      # C order
    with pytest.raises(ValueError):
        dp.eval_states(pcof, out=np.zeros((N, nt, c), order="F"))
    with pytest.raises(ValueError):
        dp.eval_populations(pcof, level_map=np.zeros((3, N + 1)))                # wrong width
    with pytest.raises(ValueError):
        dp.eval_populations(pcof, level_map=np.zeros((0, N)))                    # no group
    with pytest.raises(ValueError):
        dp.eval_states(pcof, forcing=np.zeros((2 * N, dp.m, nt, c + 1)))
    # the C ABI's own argument errors, raised before anything is launched
    import ctypes as C
    lib, vp = dp.lib, lambda a: a.ctypes.data_as(C.c_void_p)
    pc, out, M, o3 = np.ascontiguousarray(pcof), np.zeros((N, nt, c), order="F"), np.ones((1, N), order="F"), np.zeros(3)
    A = qgd._lib.QGD_ERR_ARGUMENT
    assert lib.qgd_eval_populations(dp.h, vp(pc), len(pc), 0, vp(M), 0, vp(out), vp(o3)) == A        # n_groups = 0 with a map
    assert lib.qgd_eval_populations(dp.h, vp(pc), len(pc), 0, vp(M), -2, vp(out), vp(o3)) == A
    assert lib.qgd_eval_populations(dp.h, vp(pc), len(pc), 0, None, 0, None, vp(o3)) == A            # NULL output
    assert lib.qgd_eval_states(dp.h, vp(pc), len(pc), None, None, vp(o3)) == A
    assert lib.qgd_eval_populations(dp.h, vp(pc), len(pc) - 1, 0, None, 0, vp(out), vp(o3)) == A     # length of pcof
    assert not out.any()
    _check_pop(dp.eval_populations(pcof), _pop_ref(_uv(qgd, prob, ctrl, pcof, 8)), "after the refusals")
    dp.close()
    qgd.clear_cache()
    # a partitioned handle: these calls are single-GPU
    dp = qgd.DeviceProblem(prob, 8)
    qgd._lib.check(dp.h, dp.lib.qgd_set_partition(dp.h, 0, 2))
    assert not dp.observables_supported()
    for call in (lambda: dp.eval_populations(pcof), lambda: dp.eval_states(pcof)):
        with pytest.raises(qgd._lib.QGDError) as e:
            call()
        assert e.value.code == qgd._lib.QGD_ERR_UNSUPPORTED
    dp.close()
