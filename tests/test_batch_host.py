"""The host side of batched evaluation without a device: the shape rules of a batch of coefficient
vectors, and the two helpers eval_grad_finite_difference forms its one batch and its difference quotients with."""
import numpy as np
import pytest


# -- batch_pcofs ---------------------------------------------------------------------------------------------------------------

def test_batch_pcofs_returns_c_contiguous_float64_rows(qgd):
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    out = qgd.batch_pcofs(a, 4)
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (3, 4) and np.array_equal(out, a)
    # integers
    out = qgd.batch_pcofs(np.arange(12).reshape(3, 4), 4)
    assert out.dtype == np.float64 and out.flags.c_contiguous and np.array_equal(out, a)
    # Fortran order: the rows must come out as rows
    f = np.asfortranarray(a)
    assert not f.flags.c_contiguous
    out = qgd.batch_pcofs(f, 4)
    assert out.flags.c_contiguous and np.array_equal(out, a) and np.array_equal(out.ravel(), a.ravel())
    # a strided view, nested lists
    assert np.array_equal(qgd.batch_pcofs(np.arange(24.0).reshape(3, 8)[:, ::2], 4), np.arange(24.0).reshape(3, 8)[:, ::2])
    assert qgd.batch_pcofs(np.arange(24.0).reshape(3, 8)[:, ::2], 4).flags.c_contiguous
    assert np.array_equal(qgd.batch_pcofs([[1, 2], [3, 4]], 2), np.array([[1.0, 2.0], [3.0, 4.0]]))
    # float32 widens exactly
    assert np.array_equal(qgd.batch_pcofs(a.astype(np.float32), 4), a)


def test_batch_pcofs_takes_a_single_vector_as_a_batch_of_one(qgd):
    v = np.array([0.5, -1.0, 2.0])
    out = qgd.batch_pcofs(v, 3)
    assert out.shape == (1, 3) and out.flags.c_contiguous and np.array_equal(out[0], v)
    assert qgd.batch_pcofs([1, 2, 3], 3).shape == (1, 3)


@pytest.mark.parametrize("bad", [
    np.zeros((3, 5)),                 # wrong trailing length
    np.zeros(5),                      # a single vector of the wrong length
    np.zeros((0, 4)),                 # an empty batch
    np.zeros(0),
    [],
    np.zeros((2, 3, 4)),              # more than two dimensions
    np.zeros((1, 1, 4)),
    np.zeros((3, 4), dtype=complex),  # complex
    np.zeros(4, dtype=complex),
    [[1j, 0, 0, 0]],
])
def test_batch_pcofs_refusals_name_pcofs(qgd, bad):
    with pytest.raises(ValueError, match="pcofs"):
        qgd.batch_pcofs(bad, 4)


# -- the finite-difference helpers ---------------------------------------------------------------------------------------------

def test_finite_difference_points_are_pcof_plus_minus_dpcof_e_i_in_quotient_order(qgd):
    pcof = np.array([0.3, -0.0, 1e-3, -7.25, 0.0])
    n, d = len(pcof), 1e-5
    P = qgd.finite_difference_points(pcof, d)
    assert P.shape == (2 * n, n) and P.dtype == np.float64 and P.flags.c_contiguous
    for i in range(n):
        e = np.zeros(n); e[i] = d
        # the very expressions of the loop over single evaluations: the same bits, signed zeros included
        assert (P[i].tobytes(), P[n + i].tobytes()) == ((pcof + e).tobytes(), (pcof - e).tobytes())
    # one member per point goes through batch_pcofs unchanged
    assert np.array_equal(qgd.batch_pcofs(P, n), P)
    # the input is left alone
    assert np.array_equal(pcof, np.array([0.3, -0.0, 1e-3, -7.25, 0.0]))


def test_quotient_reproduces_the_centred_difference_on_a_quadratic(qgd):
    """f(x) = 0.5 x^T A x + b^T x: the centred difference is exact up to rounding, its gradient is A x + b."""
    rng = np.random.default_rng(7)
    n, d = 6, 1e-3
    A = rng.standard_normal((n, n)); A = A + A.T
    b, x = rng.standard_normal(n), rng.standard_normal(n)
    f = lambda p: 0.5 * p @ A @ p + b @ p
    costs = np.array([f(p) for p in qgd.finite_difference_points(x, d)])
    g = qgd.finite_difference_quotient(costs, d)
    assert g.shape == (n,)
    # bit for bit the expression of the loop ...
    for i in range(n):
        e = np.zeros(n); e[i] = d
        assert g[i] == (f(x + e) - f(x - e)) / (2 * d)
    # ... and the known gradient: the quotient of a quadratic has no truncation error, its rounding error is that of two
    # values of size |f| <= 40 here (eps * 40 = 9e-15) divided by 2 d = 2e-3: 5e-12, with the sums inside f a few times that
    assert np.abs(costs).max() <= 40
    assert np.abs(g - (A @ x + b)).max() <= 5e-11
