"""The numpy statement of the dense-output pushforward (proto_dense_pushforward.py) on the CPU: (i) against Richardson central
differences of the statement's own dense outputs (proto_dense_pullback.dense_outputs) along v, (ii) duality with the statement of
the dense-output pullback, (iii) its conventions.

(i) Steps h = 1e-3 and h / 2, extrapolated; bound max|x - fd| <= 1e-9 max|fd| per output, the bound of
test_dense_pullback_proto.py (the reasoning is in test_pullback_proto.py's docstring).  One unit direction.
(ii) |<ybar, J v> - <J^T ybar, v>| <= 1e-10 max(1, max|g|) |v|_1, the project's bound between two formulations of one gradient
(the _dual of test_gpu_pushforward.py), with the cotangents of test_dense_pullback_proto.py from default_rng(13).
The measured figures are in DESIGN.md section 4n."""
import numpy as np
import pytest

import proto_dense_pullback as pdp
import proto_dense_pushforward as pdf
import proto_pushforward as pf
from test_dense_pullback_proto import _cotangents
from test_hessian_proto import _case

CASES = [("cnot2", 2, 2), ("cnot2", 8, 3), ("guarded", 6, 7), ("cnot2", 16, 2), ("rand21x11", 4, 3)]


def _setup(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    return prob, pcof, target, (Gp, Gq, off), pdf.setup(prob, Gp, Gq, off, pcof, target, order)


@pytest.mark.parametrize("name,order,refine", CASES)
def test_statement_matches_differences_of_the_dense_outputs(qgd, name, order, refine):
    prob, pcof, target, G, pre = _setup(qgd, name, order)
    bars = _cotangents(prob, np.random.default_rng(13), refine)
    lm, obs = bars["level_map"], bars["observables"]
    v = np.random.default_rng(29).standard_normal(len(pcof)); v /= np.linalg.norm(v)
    x = pdf.dense_pushforward(qgd, prob, *G, pcof, target, order, refine, v, lm, obs, pre=pre)

    def fd(h):
        a = pdp.dense_outputs(qgd, prob, *G, pcof + h * v, order, refine, lm, obs)
        b = pdp.dense_outputs(qgd, prob, *G, pcof - h * v, order, refine, lm, obs)
        return [(p - q) / (2 * h) for p, q in zip(a, b)]
    f1, f2 = fd(1e-3), fd(5e-4)
    for kind, xi, a1, a2 in zip(("states", "populations", "expectations"), x, f1, f2):
        F = (4 * a2 - a1) / 3
        err, sc = np.abs(xi - F).max(), np.abs(F).max()
        print(f"{name} order {order} refine {refine} {kind}: max|x - fd| = {err:.2e}, max|fd| = {sc:.2e}, ratio {err / sc:.2e}")
        assert xi.shape == F.shape and err <= 1e-9 * sc, kind


@pytest.mark.parametrize("name,order,refine", CASES)
def test_statement_is_dual_to_the_dense_pullback_statement(qgd, name, order, refine):
    prob, pcof, target, G, pre = _setup(qgd, name, order)
    bars = _cotangents(prob, np.random.default_rng(13), refine)
    v = np.zeros(len(pcof)); v[len(pcof) // 2] = 1.0
    S, P, E = pdf.dense_pushforward(qgd, prob, *G, pcof, target, order, refine, v, bars["level_map"], bars["observables"], pre=pre)
    parts = {"states": (S, dict(states_bar=bars["states_bar"])),
             "populations": (P, dict(pop_bar=bars["pop_bar"], level_map=bars["level_map"])),
             "expectations": (E, dict(expect_bar=bars["expect_bar"], observables=bars["observables"]))}
    for kind, (out, part) in parts.items():
        bar = part[[k for k in part if k.endswith("_bar")][0]]
        g = pdp.dense_pullback(qgd, prob, *G, pcof, order, refine, fwd=pre["fwd"], **part)
        jv, gv = np.sum(bar * out), g @ v
        err, bound = abs(jv - gv), 1e-10 * max(1.0, np.abs(g).max()) * np.abs(v).sum()
        print(f"{name} order {order} refine {refine} {kind}: |<ybar, J v> - <g, v>| = {err:.2e}, bound {bound:.2e}, |<g, v>| = {abs(gv):.2e}")
        assert err <= bound, kind


def test_statement_conventions(qgd):
    """Slot 0 is exact zeros; the grid slots of Sdot are proto_pushforward's, and refine = 1 is it everywhere; the dA w term is no
    rounding matter: it exceeds 1e-3 max|Sdot|, and without it the difference check fails."""
    name, order, refine = "cnot2", 4, 3
    prob, pcof, target, G, pre = _setup(qgd, name, order)
    rng = np.random.default_rng(31)
    bars = _cotangents(prob, rng, refine)
    lm, obs = bars["level_map"], bars["observables"]
    v = rng.standard_normal(len(pcof)); v /= np.linalg.norm(v)
    (S, P, E), t = pdf.dense_pushforward(qgd, prob, *G, pcof, target, order, refine, v, lm, obs, pre=pre, terms=True)
    assert not S[:, 0].any() and not P[:, 0].any() and not E[:, 0].any() and S[:, 1:].any()
    grid = pf.pushforward(prob, *G, pcof, target, order, v, 1, lm, obs, pre=pre["pre"])
    assert np.array_equal(S[:, ::refine], grid[0])
    one = pdf.dense_pushforward(qgd, prob, *G, pcof, target, order, 1, v, lm, obs, pre=pre)
    for a, b in zip(one, grid):
        assert np.array_equal(a, b)
    # the dA w term
    S0 = pdf.dense_pushforward(qgd, prob, *G, pcof, target, order, refine, v, lm, obs, pre=pre, explicit=False)[0]
    term = np.abs(S - S0).max()
    print(f"{name} order {order} refine {refine}: max|dA w part of Sdot| = {term:.2e}, max|Sdot| = {np.abs(S).max():.2e}")
    assert term > 1e-3 * np.abs(S).max()
    assert np.array_equal(S0[:, ::refine], S[:, ::refine])      # (it enters between the grid points only)
    a = pdp.dense_outputs(qgd, prob, *G, pcof + 1e-3 * v, order, refine)[0] - pdp.dense_outputs(qgd, prob, *G, pcof - 1e-3 * v, order, refine)[0]
    b = pdp.dense_outputs(qgd, prob, *G, pcof + 5e-4 * v, order, refine)[0] - pdp.dense_outputs(qgd, prob, *G, pcof - 5e-4 * v, order, refine)[0]
    F = (4 * b / 1e-3 - a / 2e-3) / 3
    assert np.abs(S - F).max() <= 1e-9 * np.abs(F).max() < np.abs(S0 - F).max()
