"""Host side of eval_expectations: observable_planes, which validates the caller's observables and splits them into the
planes the library takes (obs_re, obs_im [N, N, n_obs] column-major, obs_im None for real observables).  No device."""
import numpy as np
import pytest


def _hermitian(rng, N):
    a = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    return a + a.conj().T


def _symmetric(rng, N):
    a = rng.standard_normal((N, N))
    return a + a.T


@pytest.mark.parametrize("N", [2, 4, 9])
def test_a_single_matrix_and_a_stack(qgd, N):
    rng = np.random.default_rng(N)
    obs = [_hermitian(rng, N) for _ in range(3)]
    re, im = qgd.observable_planes(obs, N)
    for p in (re, im):
        assert p.shape == (N, N, 3) and p.dtype == np.float64 and p.flags.f_contiguous
    for j, o in enumerate(obs):
        assert np.array_equal(re[:, :, j], o.real) and np.array_equal(im[:, :, j], o.imag)
        r1, i1 = qgd.observable_planes(o, N)                  # one [N, N] matrix: a stack of one
        assert r1.shape == i1.shape == (N, N, 1) and r1.flags.f_contiguous and i1.flags.f_contiguous
        assert np.array_equal(r1[:, :, 0], re[:, :, j]) and np.array_equal(i1[:, :, 0], im[:, :, j])
    r2, i2 = qgd.observable_planes(np.stack(obs), N)          # an [n_obs, N, N] array
    assert np.array_equal(r2, re) and np.array_equal(i2, im)
    r3, i3 = qgd.observable_planes(tuple(obs), N)
    assert np.array_equal(r3, re) and np.array_equal(i3, im)


def test_real_observables_have_no_imaginary_plane(qgd):
    N = 5
    rng = np.random.default_rng(1)
    s = _symmetric(rng, N)
    re, im = qgd.observable_planes(s, N)
    assert im is None and re.shape == (N, N, 1) and re.flags.f_contiguous and np.array_equal(re[:, :, 0], s)
    # a complex dtype whose imaginary parts are all exactly zero is a real observable too
    re2, im2 = qgd.observable_planes(s.astype(complex), N)
    assert im2 is None and np.array_equal(re2, re)
    # integers are numbers
    re3, im3 = qgd.observable_planes(np.diag(np.arange(N)), N)
    assert im3 is None and re3.dtype == np.float64 and np.array_equal(re3[:, :, 0], np.diag(np.arange(N, dtype=float)))
    # one complex matrix in a stack gives the whole stack an imaginary plane, zero where the matrix is real
    h = _hermitian(rng, N)
    re4, im4 = qgd.observable_planes([s, h], N)
    assert im4 is not None and not im4[:, :, 0].any() and np.array_equal(im4[:, :, 1], h.imag)
    assert np.array_equal(re4[:, :, 0], s) and np.array_equal(re4[:, :, 1], h.real)


def test_scipy_sparse_matrices_are_densified(qgd):
    import scipy.sparse as sp
    N = 6
    a = np.diag(np.sqrt(np.arange(1.0, N)), 1)
    x = sp.csc_matrix(a + a.T)
    y = sp.csr_matrix(1j * (a.T - a))
    re, im = qgd.observable_planes(x, N)
    assert im is None and np.array_equal(re[:, :, 0], a + a.T)
    re, im = qgd.observable_planes([x, y], N)
    assert re.shape == im.shape == (N, N, 2)
    assert np.array_equal(re[:, :, 0], a + a.T) and not re[:, :, 1].any()
    assert not im[:, :, 0].any() and np.array_equal(im[:, :, 1], a.T - a)


def test_wrong_shapes_and_dtypes_are_refused(qgd):
    N = 4
    ok = np.eye(N)
    for bad in (np.eye(N + 1), np.zeros((N, N + 1)), np.zeros((2, N + 1, N + 1)), np.zeros(N), np.zeros((0, N, N)), [],
                np.zeros((2, 2, N, N)), [ok, np.eye(N + 1)], np.full((N, N), "a"), np.full((N, N), None, dtype=object),
                np.eye(N, dtype=bool)):
        with pytest.raises(ValueError):
            qgd.observable_planes(bad, N)
    with pytest.raises(ValueError):
        qgd.observable_planes(ok, N + 1)


def test_non_hermitian_matrices_are_refused(qgd):
    N = 4
    rng = np.random.default_rng(2)
    h = _hermitian(rng, N)
    lower = np.tril(np.ones((N, N)), -1)
    for bad in (h + 1e-9 * lower, 1j * np.eye(N), np.triu(np.ones((N, N))), h + 1e-9j * (lower + lower.T)):
        with pytest.raises(ValueError):
            qgd.observable_planes(bad, N)
        with pytest.raises(ValueError):
            qgd.observable_planes([h, bad], N)
    nan = np.eye(N); nan[0, 0] = np.nan
    with pytest.raises(ValueError):
        qgd.observable_planes(nan, N)
    # the rule is max|O - O^H| <= 1e-12 max(1, max|O|): rounding-sized asymmetry passes, relative to a large matrix too
    qgd.observable_planes(h + 1e-14 * lower, N)
    qgd.observable_planes(1e6 * h + 1e-8 * lower, N)
    with pytest.raises(ValueError):
        qgd.observable_planes(1e-6 * h + 1e-11 * lower, N)      # (small matrices are held to the absolute 1e-12)


def test_the_functional_call_refuses_before_touching_a_device(qgd):
    prob, _ = qgd.cnot2_problem(nsteps=4, tf=4.0)
    ctrl = [qgd.GeneralBSplineControl(2, 4, prob.tf) for _ in range(prob.N_operators)]
    pcof = np.zeros(qgd.get_number_of_control_parameters(ctrl))
    with pytest.raises(ValueError):
        qgd.eval_expectations(prob, ctrl, pcof, np.eye(4), order=2, saveEveryNsteps=0)
    with pytest.raises(ValueError):
        qgd.eval_expectations(prob, ctrl, pcof, np.triu(np.ones((4, 4))), order=2)
    with pytest.raises(ValueError):
        qgd.eval_expectations(prob, ctrl, pcof, np.eye(5), order=2)


def test_the_entry_point_is_exported(qgd):
    assert "qgd_eval_expectations" in qgd._lib.EXPORTS
    assert callable(qgd.eval_expectations) and callable(qgd.observable_planes)
    assert callable(qgd.DeviceProblem.eval_expectations)
