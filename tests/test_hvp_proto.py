"""The numpy statement of the second-order-adjoint Hessian-vector product (proto_hvp.py) against the numpy statement of
the full Hessian (proto_hessian.py) times the vector (CPU).  The cases are those of test_hessian_proto.py; the guarded
ones are also run with the guard projector removed."""
import copy

import numpy as np
import pytest

import proto_hessian as ph
import proto_hvp as pv
from test_hessian_proto import CASES, _case


def _problem(qgd, name, guard):
    prob, ctrl, pcof, target = _case(qgd, name)
    if not guard:
        prob = copy.copy(prob)
        prob.guard_subspace_projector = np.zeros_like(np.asarray(prob.guard_subspace_projector))
    return prob, ctrl, pcof, target


# (cnot2 has no guard levels: "guard" is the problem as it is, "noguard" the two guarded problems without their projector)
PARAMS = [(name, order, True) for name, order in CASES] + [(name, order, False) for name, order in CASES if name != "cnot2"]
PARAMS += [("rand21x11", 4, True), ("rand21x11", 4, False)]      # more than 8 columns, more than 16 levels (cases.sensitivity_case)


@pytest.mark.parametrize("name,order,guard", PARAMS, ids=[f"{n}-{o}-{'guard' if g else 'noguard'}" for n, o, g in PARAMS])
def test_proto_hvp_matches_proto_hessian(qgd, name, order, guard):
    prob, ctrl, pcof, target = _problem(qgd, name, guard)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    H = ph.hessian(prob, Gp, Gq, off, pcof, target, order)
    pre = pv.setup(prob, Gp, Gq, off, pcof, target, order)
    n = len(pcof)
    rng = np.random.default_rng(7)
    unit = np.zeros(n); unit[n // 3] = 1.0
    for v in (rng.standard_normal(n), unit):
        hv = pv.hessian_vec(prob, Gp, Gq, off, pcof, target, order, v, pre=pre)
        err = np.abs(hv - H @ v).max()
        bound = 1e-11 * np.abs(H).max() * np.abs(v).sum()
        print(f"{name} order {order} guard {guard}: max|hv - H v| = {err:.2e} (bound {bound:.2e})")
        assert err <= bound
    assert np.all(pv.hessian_vec(prob, Gp, Gq, off, pcof, target, order, np.zeros(n), pre=pre) == 0.0)
