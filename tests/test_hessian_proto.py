"""The numpy statement of the exact Hessian (proto_hessian.py) against Richardson central differences of
proto_propagator's gradient (CPU)."""
import numpy as np
import pytest

import cases
import proto_hessian as ph


CASES = [("cnot2", 2), ("cnot2", 4), ("cnot2", 8), ("guarded", 6), ("dense_guard", 6)]


def _case(qgd, name):
    if name == "cnot2":
        return cases.cnot2_case(qgd, nsteps=12, tf=12.0)
    if name == "rand21x11":                       # N = 21 in two 16-row blocks, 11 columns in two groups, a diagonal guard matrix
        return cases.sensitivity_case(qgd, name)[:4]
    if name == "dense_guard":
        return cases.dense_guard_case(qgd, nsteps=10, tf=5.0)
    return cases.guarded_case(qgd, nsteps=10, tf=5.0)


@pytest.mark.parametrize("name,order", CASES)
def test_proto_hessian_matches_gradient_differences(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    H, t = ph.hessian(prob, Gp, Gq, off, pcof, target, order, terms=True)
    F = ph.grad_fd_hessian(prob, Gp, Gq, off, pcof, target, order)
    sc = np.abs(F).max()
    assert np.abs(H - F).max() <= 1e-9 * sc
    assert np.abs(H - H.T).max() <= 1e-12 * sc
    if order == 2:
        assert np.abs(t["E"]).max() == 0.0
    if order == 4:
        assert np.abs(t["E"]).max() > 1e-3 * sc
