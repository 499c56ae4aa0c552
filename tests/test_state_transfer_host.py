"""cost_type :StateTransfer without a device: the numpy statement (proto_state_transfer.py) against
differences of itself, the invariance that distinguishes the cost from :Infidelity, the Python layer's host arithmetic, and the
places the value 3 is written down (Python table, C header, Julia shim).

Bounds.  Centred differences with h = 1e-6 of a function that is quadratic in w have no truncation error; what is left is
rounding of J (|J| <= 1, unit 1.1e-16) divided by 2h: 1e-10 absolute, against derivatives of order 0.1 .. 1 -- 1e-7 relative is
ample.  The invariances are exact in real arithmetic; a_j^2 + b_j^2 of a column of N <= 5 products is rounded a few units of
2^-53: 1e-14."""
import os
import re

import numpy as np
import pytest

import proto_state_transfer as pst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit_columns(rng, N, c):
    t = rng.standard_normal((N, c)) + 1j * rng.standard_normal((N, c))
    return t / np.linalg.norm(t, axis=0)[None, :]


@pytest.mark.parametrize("N,c", [(3, 2), (5, 5)])
def test_prototype_derivatives_against_differences(N, c):
    rng = np.random.default_rng(10 * N + c)
    target = _unit_columns(rng, N, c)
    w = rng.standard_normal((2 * N, c))
    h = 1e-6
    g = pst.cost_bar(w, target)
    fd = np.zeros_like(w)
    for i in range(2 * N):
        for j in range(c):
            e = np.zeros_like(w); e[i, j] = h
            fd[i, j] = (pst.cost(w + e, target) - pst.cost(w - e, target)) / (2 * h)
    assert np.abs(g - fd).max() <= 1e-7 * np.abs(g).max()
    s = rng.standard_normal((2 * N, c))
    so = pst.second_order(s, target)
    fd2 = (pst.cost_bar(w + h * s, target) - pst.cost_bar(w - h * s, target)) / (2 * h)
    assert np.abs(so - fd2).max() <= 1e-7 * np.abs(so).max()


@pytest.mark.parametrize("N,c", [(3, 2), (5, 5)])
def test_column_phases_leave_the_cost_unchanged(qgd, N, c):
    rng = np.random.default_rng(N + 100 * c)
    target = _unit_columns(rng, N, c)
    psi = _unit_columns(rng, N, c)
    ph = np.exp(2j * np.pi * rng.random(c))
    J0, J1 = pst.cost(psi, target), pst.cost(psi, target * ph[None, :])
    assert abs(J0 - J1) <= 1e-14
    assert abs(pst.cost(target * ph[None, :], target)) <= 1e-14
    # the global overlap of :Infidelity does depend on them
    f0 = qgd.infidelity_real(pst.real(target), pst.real(target), c)
    f1 = qgd.infidelity_real(pst.real(target * ph[None, :]), pst.real(target), c)
    assert abs(f0) <= 1e-14 and f1 > 1e-3


def test_python_host_arithmetic_equals_the_prototype(qgd):
    rng = np.random.default_rng(4)
    N, c = 4, 3
    target, psi = _unit_columns(rng, N, c), _unit_columns(rng, N, c) * 0.9
    J = pst.cost(psi, target)
    assert abs(qgd.state_transfer_infidelity(psi, target) - J) <= 1e-15
    assert abs(qgd.state_transfer_infidelity(pst.real(psi), pst.real(target)) - J) <= 1e-15
    states = np.zeros((2 * N, 3, c), order="F"); states[:, -1] = pst.real(psi)
    assert abs(qgd.state_transfer_infidelity(states, target) - J) <= 1e-15
    hist = np.zeros((2 * N, 2, 3, c), order="F"); hist[:, 0, -1] = pst.real(psi); hist[:, 1, -1] = 7.0
    assert abs(qgd.state_transfer_infidelity(hist, target) - J) <= 1e-15


def test_the_value_three_everywhere(qgd):
    assert qgd.COST_TYPES["StateTransfer"] == 3 and qgd.COST_TYPES[":StateTransfer"] == 3
    assert qgd.COST_TYPES["Infidelity"] == 0 and qgd.COST_TYPES[":Norm"] == 2
    header = open(os.path.join(ROOT, "include", "qgd.h")).read()
    assert re.search(r"^#define\s+QGD_COST_STATE_TRANSFER\s+3\s*$", header, re.M)
    shim = open(os.path.join(ROOT, "julia", "QuantumGateDesignHIP.jl")).read()
    body = shim[shim.index("function set_cost_type!"):]
    body = body[:body.index("\nend")]
    assert re.search(r"cost_type\s*==\s*:StateTransfer\s*\?\s*3\b", body)
