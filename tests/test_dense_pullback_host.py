"""The Python layer of eval_dense_pullback without a device: what DeviceProblem.eval_dense_pullback and the functional
eval_dense_pullback refuse before the library is touched, and that the new names are there."""
import inspect

import numpy as np
import pytest


def test_the_new_names_are_exported(qgd):
    assert "qgd_eval_dense_pullback" in qgd._lib.EXPORTS
    assert callable(qgd.eval_dense_pullback) and callable(qgd.DeviceProblem.eval_dense_pullback)
    sig = inspect.signature(qgd.DeviceProblem.eval_dense_pullback)
    assert list(sig.parameters)[1:] == ["refine", "pcof", "states_bar", "populations_bar", "level_map", "expectations_bar",
                                        "observables", "history_precomputed"]
    sig = inspect.signature(qgd.eval_dense_pullback)
    assert list(sig.parameters)[:5] == ["prob", "controls", "pcof", "order", "refine"]
    assert sig.parameters["order"].default == 2 and sig.parameters["refine"].default == 2


def test_the_functional_form_refuses_before_a_handle_is_made(qgd, monkeypatch):
    prob, _ = qgd.cnot2_problem(nsteps=7, tf=7.0)
    ctrl = [qgd.GeneralBSplineControl(2, 6, prob.tf) for _ in range(prob.N_operators)]
    pcof = np.zeros(qgd.get_number_of_control_parameters(ctrl))
    N, c = prob.N_tot_levels, prob.N_initial_conditions

    def no_handle(*a, **k):
        raise AssertionError("a handle was asked for")
    import sys
    monkeypatch.setattr(sys.modules[qgd.__name__ + ".evolution"], "device_problem", no_handle)
    for refine in (0, 1.5, -1, True):
        with pytest.raises(ValueError, match="refine"):
            qgd.eval_dense_pullback(prob, ctrl, pcof, order=4, refine=refine, states_bar=np.zeros((2 * N, 8, c)))
    with pytest.raises(ValueError, match="at least one"):
        qgd.eval_dense_pullback(prob, ctrl, pcof, refine=3)
    with pytest.raises(ValueError, match="states_bar"):      # 1 + 7 * 3 = 22 slots, not the 8 grid points
        qgd.eval_dense_pullback(prob, ctrl, pcof, refine=3, states_bar=np.zeros((2 * N, 8, c)))
    with pytest.raises(ValueError, match="populations_bar"):
        qgd.eval_dense_pullback(prob, ctrl, pcof, refine=3, populations_bar=np.zeros((N, 21, c)))
    with pytest.raises(ValueError, match="go together"):
        qgd.eval_dense_pullback(prob, ctrl, pcof, refine=3, expectations_bar=np.zeros((1, 22, c)))
    with pytest.raises(ValueError, match="Hermitian"):
        qgd.eval_dense_pullback(prob, ctrl, pcof, refine=3, expectations_bar=np.zeros((1, 22, c)), observables=np.triu(np.ones((N, N))))
    with pytest.raises(AssertionError, match="a handle was asked for"):      # valid arguments get as far as the handle
        qgd.eval_dense_pullback(prob, ctrl, pcof, refine=3, states_bar=np.zeros((2 * N, 22, c)))


def test_handle_method_refuses_before_the_library_is_called(qgd):
    """On an object that has no handle at all, so reaching the C ABI would raise AttributeError."""
    dp = qgd.DeviceProblem.__new__(qgd.DeviceProblem)
    dp.N, dp.c, dp.nsteps, dp.m = 4, 2, 5, 2
    good = np.zeros((8, 16, 2))                            # 1 + 5 * 3 = 16 slots
    for refine in (0, 2.5, -3):
        with pytest.raises(ValueError, match="refine"):
            dp.eval_dense_pullback(refine, states_bar=good)
    with pytest.raises(ValueError, match="at least one"):
        dp.eval_dense_pullback(3)
    with pytest.raises(ValueError, match="states_bar"):
        dp.eval_dense_pullback(3, states_bar=np.zeros((8, 6, 2)))      # the grid's 6 points
    with pytest.raises(ValueError, match="states_bar"):
        dp.eval_dense_pullback(2, states_bar=good)                     # 11 slots at refine = 2
    with pytest.raises(ValueError, match="level_map"):
        dp.eval_dense_pullback(3, populations_bar=np.zeros((3, 16, 2)), level_map=np.ones((3, 5)))
    with pytest.raises(ValueError, match="populations_bar"):
        dp.eval_dense_pullback(3, populations_bar=np.zeros((4, 16, 2)), level_map=np.ones((3, 4)))
    with pytest.raises(ValueError, match="expectations_bar"):
        dp.eval_dense_pullback(3, expectations_bar=np.zeros((2, 16, 2)), observables=np.eye(4))
    with pytest.raises(ValueError, match="Hermitian"):
        dp.eval_dense_pullback(3, expectations_bar=np.zeros((1, 16, 2)), observables=np.triu(np.ones((4, 4))))
    with pytest.raises(AttributeError):                                # valid arguments get as far as the library
        dp.eval_dense_pullback(3, states_bar=good)
