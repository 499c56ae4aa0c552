"""The Hermite dense output without a device: the weights, hermite_interpolate -- the written statement
of what qgd_eval_dense computes -- on exact polynomial data and on the oracle's histories, and what the Python layer refuses
before the library is touched.

Accuracy (test 3).  Truth: the oracle at order 12 on a 16 times finer grid, subsampled.  The interpolant of a run must be as
accurate between the grid points as the run is at them: max error over the interior sub-points <= 2 x max error over the grid
points of the same run (measured 0.95 .. 1.17 over orders 2, 4, 8 of both cases; 2 is headroom over the 1.17 worst case), and
below the midpoint error of linear interpolation between the grid values -- at order 8 below a tenth of it (measured factors:
88 .. 102 at order 8; 2.7 and 10.5 at order 4, where only "smaller" is asserted)."""
from math import comb

import numpy as np
import pytest

import cases


# -- 1: the weights ------------------------------------------------------------------------------------------------------------

# A_0(theta) + A_0(1 - theta) = 1 exactly; each of the two non-negative terms is two powers, a sum of up to nine non-negative terms
# and two products, each rounded once: a few units of 2^-53 of a number below 1 -- the 1e-15 the cubic basis is held to
UNITY = 1e-15

def test_m1_is_the_cubic_hermite_basis(qgd):
    dt, r = 0.7, 8
    a, b = qgd.hermite_dense_weights(1, r, dt)
    assert a.shape == b.shape == (r - 1, 2)
    th = np.arange(1, r) / r
    h00, h10 = 2 * th ** 3 - 3 * th ** 2 + 1, th ** 3 - 2 * th ** 2 + th
    h01, h11 = -2 * th ** 3 + 3 * th ** 2, th ** 3 - th ** 2
    for got, want in ((a[:, 0], h00), (a[:, 1], dt * h10), (b[:, 0], h01), (b[:, 1], dt * h11)):
        assert np.abs(got - want).max() <= 1e-15


@pytest.mark.parametrize("m", range(1, 9))
def test_weights_reproduce_polynomials_up_to_degree_2m_plus_1(qgd, m):
    """the exact scaled Taylor data w_j = C(p, j) t^(p-j) of t^p at both ends of one step, theta in {1/7, 1/2, 6/7}"""
    t0, dt = 0.3, 0.8
    a7, b7 = qgd.hermite_dense_weights(m, 7, dt)
    a2, b2 = qgd.hermite_dense_weights(m, 2, dt)
    for theta, a, b in ((1 / 7, a7[0], b7[0]), (1 / 2, a2[0], b2[0]), (6 / 7, a7[5], b7[5])):
        assert a[0] >= 0 and b[0] >= 0 and abs(a[0] + b[0] - 1.0) <= UNITY      # partition of unity: A_0(th) + A_0(1-th) = 1
        for p in range(2 * m + 2):
            wl = np.array([comb(p, j) * t0 ** (p - j) if j <= p else 0.0 for j in range(m + 1)])
            wr = np.array([comb(p, j) * (t0 + dt) ** (p - j) if j <= p else 0.0 for j in range(m + 1)])
            val, want = a @ wl + b @ wr, (t0 + theta * dt) ** p
            assert abs(val - want) <= 1e-12 * max(1.0, abs(want)), (m, theta, p, val, want)


def test_partition_of_unity_on_a_fine_grid(qgd):
    for m in range(1, 9):
        a, b = qgd.hermite_dense_weights(m, 64, 1.3)
        assert np.abs(a[:, 0] + b[:, 0] - 1.0).max() <= UNITY
        assert np.array_equal(a[:, 0], b[::-1, 0])      # A_0(theta) and A_0(1 - theta) mirror each other exactly
        assert np.all(a[:, ::2] >= 0) and np.all(b[:, ::2] >= 0) and np.all(b[:, 1::2] <= 0)


# -- 2: grid slots are copies ----------------------------------------------------------------------------------------------------

def test_grid_slots_are_copied(qgd):
    rng = np.random.default_rng(0)
    h = np.asfortranarray(rng.standard_normal((6, 4, 9, 2)))
    assert np.array_equal(qgd.hermite_interpolate(h, 0.5, 1), h[:, 0])
    out = qgd.hermite_interpolate(h, 0.5, 3)
    assert out.shape == (6, 1 + 8 * 3, 2) and out.flags.f_contiguous
    assert np.array_equal(out[:, ::3], h[:, 0])
    one = qgd.hermite_interpolate(h[:, :, :1], 0.5, 5)      # a single time point: nothing to interpolate
    assert np.array_equal(one, h[:, 0, :1])


# -- 3: accuracy against the oracle ------------------------------------------------------------------------------------------------

FINE, REFINE = 16, 4
_truth = {}


def _problem(qgd, which, nsteps_scale=1):
    if which == "cnot2":
        return cases.cnot2_case(qgd, nsteps=40 * nsteps_scale, tf=40.0)
    return cases.guarded_case(qgd, nsteps=20 * nsteps_scale, tf=15.0)


def _fine_truth(qgd, orc, which):
    """order 12 on the 16 times finer grid, at the times of the dense output (computed once per case, never changed)"""
    if which not in _truth:
        prob, ctrl, pcof, _ = _problem(qgd, which, FINE)
        _truth[which] = orc.eval_forward(prob, ctrl, pcof, order=12)[:, 0, ::FINE // REFINE].copy()
        _truth[which].setflags(write=False)
    return _truth[which]


@pytest.mark.parametrize("which", ["cnot2", "guarded"])
@pytest.mark.parametrize("order", [4, 8])
def test_interpolant_is_as_accurate_as_the_run(qgd, orc, which, order):
    prob, ctrl, pcof, _ = _problem(qgd, which)
    truth = _fine_truth(qgd, orc, which)
    h = orc.eval_forward(prob, ctrl, pcof, order=order)
    dense = qgd.hermite_interpolate(h, prob.tf / prob.nsteps, REFINE)
    assert dense.shape == truth.shape
    err = np.abs(dense - truth).max(axis=(0, 2))
    grid = err[::REFINE].max()
    interior = np.delete(err, np.s_[::REFINE]).max()
    linear = np.abs(0.5 * (h[:, 0, :-1] + h[:, 0, 1:]) - truth[:, REFINE // 2::REFINE]).max()
    print(f"\n{which} order {order}, {prob.nsteps} steps: max error at grid points {grid:.3e}, at interior sub-points {interior:.3e} "
          f"(ratio {interior / grid:.3f}, bound 2), midpoint of linear interpolation {linear:.3e} (factor {linear / interior:.1f})")
    assert interior <= 2.0 * grid
    assert interior < linear
    if order == 8:
        assert interior <= 0.1 * linear


# -- 4: what the Python layer refuses before the library is touched ----------------------------------------------------------------

@pytest.mark.parametrize("refine", [0, -3, 2.5, "2", None, True, np.float64(1.5)])
def test_refine_must_be_a_positive_integer(qgd, refine):
    h = np.zeros((4, 2, 3, 1))
    with pytest.raises(ValueError, match="refine"):
        qgd.hermite_interpolate(h, 1.0, refine)
    with pytest.raises(ValueError, match="refine"):
        qgd.hermite_dense_weights(1, refine, 1.0)
    prob, _ = qgd.cnot2_problem(nsteps=7, tf=7.0)
    with pytest.raises(ValueError, match="refine"):
        qgd.dense_times(prob, refine)


def test_dense_times(qgd):
    prob, _ = qgd.cnot2_problem(nsteps=7, tf=3.5)
    t = qgd.dense_times(prob, 4)
    assert t.shape == (29,) and t[0] == 0.0 and abs(t[-1] - 3.5) <= 1e-15 and np.allclose(np.diff(t), 0.125, rtol=0, atol=1e-15)
    assert np.allclose(qgd.dense_times(prob, 4.0), t)      # an integral float is an integer
    assert np.allclose(t[::4], np.arange(8) * 0.5, rtol=0, atol=1e-15)


def test_history_shape_is_checked(qgd):
    for bad in (np.zeros((4, 2, 3)), np.zeros((4, 1, 3, 1)), np.zeros((4, 2, 3, 1), dtype=complex)):
        with pytest.raises(ValueError, match="uv_history"):
            qgd.hermite_interpolate(bad, 1.0, 2)


def test_the_functional_form_refuses_before_a_handle_is_made(qgd, monkeypatch):
    prob, _ = qgd.cnot2_problem(nsteps=7, tf=7.0)
    ctrl = [qgd.GeneralBSplineControl(2, 6, prob.tf) for _ in range(prob.N_operators)]
    pcof = np.zeros(qgd.get_number_of_control_parameters(ctrl))
    N = prob.N_tot_levels

    def no_handle(*a, **k):
        raise AssertionError("a handle was asked for")
    import sys
    monkeypatch.setattr(sys.modules[qgd.__name__ + ".evolution"], "device_problem", no_handle)
    for refine in (0, 1.5, -1):
        with pytest.raises(ValueError, match="refine"):
            qgd.eval_dense(prob, ctrl, pcof, order=4, refine=refine)
    with pytest.raises(ValueError, match="output"):
        qgd.eval_dense(prob, ctrl, pcof, output="history")
    with pytest.raises(ValueError, match="Hermitian"):
        qgd.eval_dense(prob, ctrl, pcof, output="expectations", observables=np.triu(np.ones((N, N))))
    with pytest.raises(ValueError, match="observables"):
        qgd.eval_dense(prob, ctrl, pcof, output="expectations")
    with pytest.raises(ValueError, match="observables"):
        qgd.eval_dense(prob, ctrl, pcof, output="states", observables=np.eye(N))
    with pytest.raises(ValueError, match="level_map"):
        qgd.eval_dense(prob, ctrl, pcof, output="populations", level_map=np.zeros((2, N + 1)))
    with pytest.raises(ValueError, match="level_map"):
        qgd.eval_dense(prob, ctrl, pcof, output="states", level_map=np.zeros((2, N)))
    with pytest.raises(AssertionError, match="a handle was asked for"):      # valid arguments get as far as the handle
        qgd.eval_dense(prob, ctrl, pcof, order=4, refine=3, output="populations", level_map=np.ones((2, N)))


def test_handle_methods_refuse_before_the_library_is_called(qgd):
    """DeviceProblem.eval_dense_*: refine, the shape of ``out``, the level map and the observables are checked before the C ABI
    is reached -- on an object that has no handle at all, so reaching it would raise AttributeError."""
    dp = qgd.DeviceProblem.__new__(qgd.DeviceProblem)
    dp.N, dp.c, dp.nsteps, dp.m = 4, 2, 5, 2
    for call in (lambda r: dp.eval_dense_states(r), lambda r: dp.eval_dense_populations(r),
                 lambda r: dp.eval_dense_expectations(r, np.eye(4))):
        for refine in (0, 2.5):
            with pytest.raises(ValueError, match="refine"):
                call(refine)
    with pytest.raises(ValueError, match="out"):      # 1 + 5 * 3 = 16 slots
        dp.eval_dense_states(3, out=np.zeros((8, 6, 2), order="F"))
    with pytest.raises(ValueError, match="out"):
        dp.eval_dense_states(3, out=np.zeros((8, 16, 2)))      # C order
    with pytest.raises(ValueError, match="out"):
        dp.eval_dense_populations(3, level_map=np.ones((3, 4)), out=np.zeros((4, 16, 2), order="F"))
    with pytest.raises(ValueError, match="level_map"):
        dp.eval_dense_populations(3, level_map=np.ones((3, 5)))
    with pytest.raises(ValueError, match="Hermitian"):
        dp.eval_dense_expectations(3, np.triu(np.ones((4, 4))))
    with pytest.raises(ValueError, match="out"):
        dp.eval_dense_expectations(3, np.eye(4), out=np.zeros((2, 16, 2), order="F"))
    with pytest.raises(AttributeError):      # valid arguments get as far as the library
        dp.eval_dense_states(3, out=np.zeros((8, 16, 2), order="F"))
