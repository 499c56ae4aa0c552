"""The numpy statement of the pushforward (proto_pushforward.py) on the CPU: (i) against Richardson central differences of the
statement's own forward outputs along v, (ii) duality with the statement of the pullback (proto_pullback.py).

(i) Steps and bound of the project's difference tests (test_gpu_pullback.py section 5): h = 1e-3 and 5e-4 extrapolated, 1e-8
of the difference quotient.  It is applied to the scalar <ybar, output> with a seeded random ybar, so that an element of
the output near zero cannot decide the test.  The outputs are smooth in pcof: the extrapolated truncation error is O(h^4).
(ii) <ybar, J v> and <J^T ybar, v> are two orders of the same sum over time points and basis directions:
|difference| <= 1e-10 max(1, max|J^T ybar|) |v|_1, the project's bound between two formulations of one gradient."""
import numpy as np
import pytest

import proto_pullback as pb
import proto_pushforward as pf
from test_hessian_proto import _case
from test_pullback_proto import _cotangents

CASES = [("cnot2", 2), ("cnot2", 4), ("cnot2", 8), ("guarded", 6), ("rand21x11", 4)]


def _parts(bars):
    return {"states": dict(states_bar=bars["states_bar"]),
            "populations": dict(pop_bar=bars["pop_bar"], level_map=bars["level_map"]),
            "expectations": dict(expect_bar=bars["expect_bar"], observables=bars["observables"])}


def _pairings(bars, S, P, E):
    return {"states": np.sum(bars["states_bar"] * S), "populations": np.sum(bars["pop_bar"] * P),
            "expectations": np.sum(bars["expect_bar"] * E)}


@pytest.mark.parametrize("name,order", CASES)
def test_proto_pushforward_matches_differences_of_the_outputs(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    rng = np.random.default_rng(17)
    bars = _cotangents(qgd, prob, rng, 1)
    v = rng.standard_normal(len(pcof)); v /= np.linalg.norm(v)
    jv = _pairings(bars, *pf.pushforward(prob, Gp, Gq, off, pcof, target, order, v, level_map=bars["level_map"],
                                         observables=bars["observables"]))

    def J(p):
        psi = pb.forward(prob, Gp, Gq, off, p, order)["psi"]
        return _pairings(bars, *pb.outputs(psi, 1, bars["level_map"], bars["observables"]))

    def fd(h):
        a, b = J(pcof + h * v), J(pcof - h * v)
        return {k: (a[k] - b[k]) / (2 * h) for k in a}
    f1, f2 = fd(1e-3), fd(5e-4)
    for kind in jv:
        F = (4 * f2[kind] - f1[kind]) / 3
        err = abs(jv[kind] - F)
        print(f"{name} order {order} {kind}: |<ybar, J v> - fd| = {err:.2e}, |fd| = {abs(F):.2e}, bound {1e-8 * abs(F):.2e}")
        assert err <= 1e-8 * abs(F), kind


@pytest.mark.parametrize("name,order", CASES)
def test_proto_pushforward_is_dual_to_the_proto_pullback(qgd, name, order):
    prob, ctrl, pcof, target = _case(qgd, name)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    rng = np.random.default_rng(19)
    pre = pf.setup(prob, Gp, Gq, off, pcof, target, order)
    fwd = pb.forward(prob, Gp, Gq, off, pcof, order)
    assert np.array_equal(fwd["psi"], pre["ref"]["psi"])
    for save in (1, 5):
        bars = _cotangents(qgd, prob, rng, save)
        v = rng.standard_normal(len(pcof))
        jv = _pairings(bars, *pf.pushforward(prob, Gp, Gq, off, pcof, target, order, v, save, bars["level_map"], bars["observables"],
                                             pre=pre))
        for kind, part in _parts(bars).items():
            g = pb.pullback(prob, Gp, Gq, off, pcof, order, save_every=save, fwd=fwd, **part)
            err, bound = abs(jv[kind] - g @ v), 1e-10 * max(1.0, np.abs(g).max()) * np.abs(v).sum()
            print(f"{name} order {order} save {save} {kind}: |<ybar, J v> - <J^T ybar, v>| = {err:.2e}, bound {bound:.2e}")
            assert err <= bound, kind


def test_proto_pushforward_conventions(qgd):
    """Slot 0 is zero; linear in v; populations without a map; a real diagonal observable is a one-row map; a non-Hermitian
    observable counts with its Hermitian part."""
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    order = 6
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    N = prob.N_tot_levels
    rng = np.random.default_rng(23)
    pre = pf.setup(prob, Gp, Gq, off, pcof, target, order)
    v, w, d = rng.standard_normal(len(pcof)), rng.standard_normal(len(pcof)), rng.standard_normal(N)
    run = lambda vv, **k: pf.pushforward(prob, Gp, Gq, off, pcof, target, order, vv, pre=pre, **k)
    S, P, E = run(v, observables=np.diag(d))
    assert not S[:, 0].any() and not P[:, 0].any() and not E[:, 0].any() and S[:, 1:].any()
    assert np.abs(P - 2 * (S[:N] * pb.outputs(pre["ref"]["psi"])[0][:N] + S[N:] * pb.outputs(pre["ref"]["psi"])[0][N:])).max() <= 1e-15
    assert np.abs(E - run(v, level_map=d[None])[1]).max() <= 1e-13 * np.abs(E).max()
    S2 = run(2.0 * v - 3.0 * w)[0]
    assert np.abs(S2 - (2.0 * S - 3.0 * run(w)[0])).max() <= 1e-13 * np.abs(S2).max()
    O = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    assert np.abs(run(v, observables=O)[2] - run(v, observables=0.5 * (O + O.conj().T))[2]).max() <= 1e-13 * np.abs(O).max()
