"""Host side of the populations feature: get_populations (the reference's signature, host arithmetic),
subsystem_population_map (its digit order pinned with basis_state) and the argument errors that need no device."""
import itertools

import numpy as np
import pytest


@pytest.mark.parametrize("shape", [(8, 3, 7), (8, 3, 7, 5), (2, 1, 1, 1), (18, 5, 4, 3)])
def test_get_populations_matches_definition(qgd, shape):
    h = np.asfortranarray(np.random.default_rng(3).standard_normal(shape))
    N = shape[0] // 2
    p = qgd.get_populations(h)
    assert p.shape == (N,) + shape[2:]
    assert np.array_equal(p, h[:N, 0] ** 2 + h[N:, 0] ** 2)
    # the derivative axis is dropped: the other Taylor columns do not enter
    h2 = h.copy(); h2[:, 1:] = 7.0
    assert np.array_equal(qgd.get_populations(h2), p)
    # memory order of the input does not matter
    assert np.array_equal(qgd.get_populations(np.ascontiguousarray(h)), p)


@pytest.mark.parametrize("bad", [np.zeros((4, 2)), np.zeros((4, 2, 3, 1, 1)), np.zeros((3, 2, 3)), np.zeros((4, 2, 3), dtype=complex)])
def test_get_populations_refuses_other_arrays(qgd, bad):
    with pytest.raises(ValueError):
        qgd.get_populations(bad)


@pytest.mark.parametrize("sizes", [(2, 2), (4, 4, 4), (3, 2, 4)])
def test_subsystem_population_map_against_basis_states(qgd, sizes):
    M = qgd.subsystem_population_map(sizes)
    N = int(np.prod(sizes))
    assert M.shape == (sum(sizes), N) and M.flags.f_contiguous and M.dtype == np.float64
    assert set(np.unique(M)) == {0.0, 1.0}
    offs = np.concatenate([[0], np.cumsum(sizes)])
    # every level of the full system belongs to exactly one row of every subsystem
    for q in range(len(sizes)):
        assert np.array_equal(M[offs[q]:offs[q + 1]].sum(axis=0), np.ones(N))
    # a product basis state |n0 n1 ...> (problems.basis_state: the digit order of lowering_operators_system) maps to
    # exactly one 1 per subsystem, in the row of that subsystem's level
    for idx in itertools.product(*[range(s) for s in sizes]):
        want = np.zeros(sum(sizes))
        for q, i in enumerate(idx):
            want[offs[q] + i] = 1.0
        assert np.array_equal(M @ qgd.basis_state(sizes, idx), want), (sizes, idx)
    # and agrees with the number operators a'a of lowering_operators_system: <n_q> = sum_l l * P[q, l]
    for q, a in enumerate(qgd.lowering_operators_system(sizes)):
        assert np.allclose(np.arange(sizes[q]) @ M[offs[q]:offs[q + 1]], np.diag(a.T @ a))


@pytest.mark.parametrize("bad", [(), (0, 2), (2, -1)])
def test_subsystem_population_map_refuses_bad_sizes(qgd, bad):
    with pytest.raises(ValueError):
        qgd.subsystem_population_map(bad)


def test_eval_populations_refuses_bad_stride_before_touching_a_device(qgd):
    prob, _ = qgd.cnot2_problem(nsteps=4, tf=4.0)
    ctrl = [qgd.GeneralBSplineControl(2, 4, prob.tf) for _ in range(prob.N_operators)]
    with pytest.raises(ValueError):
        qgd.eval_populations(prob, ctrl, np.zeros(qgd.get_number_of_control_parameters(ctrl)), order=2, saveEveryNsteps=0)


def test_new_entry_points_are_exported(qgd):
    assert {"qgd_eval_states", "qgd_eval_populations"} <= set(qgd._lib.EXPORTS)
    for name in ("get_populations", "eval_populations", "subsystem_population_map"):
        assert callable(getattr(qgd, name))
    for name in ("eval_states", "eval_populations"):
        assert callable(getattr(qgd.DeviceProblem, name))
