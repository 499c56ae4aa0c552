"""The numpy statement of the pullback (proto_pullback.py) against Richardson central differences of its own forward
trajectory contracted with random cotangents (CPU).

Bound: 1e-9 max|F|, the bound the numpy statements of the second-order quantities are held to against differences of the
same kind (test_hessian_proto.py, whose cases test_hvp_proto.py runs on): steps h = 1e-3 and h / 2, extrapolated.  The
objective is smooth in pcof, so the extrapolated truncation error is O(h^4), and the rounding of a difference of two sums of
O(1) terms over 2h = 1e-3 is of the order 1e-13."""
import numpy as np
import pytest

import proto_pullback as pb
from test_hessian_proto import _case


def _cotangents(qgd, prob, rng, save, n_obs=3, n_groups=3, complex_obs=True):
    N, c = prob.N_tot_levels, prob.N_initial_conditions
    slots = 1 + prob.nsteps // save
    obs = rng.standard_normal((n_obs, N, N)) + (1j * rng.standard_normal((n_obs, N, N)) if complex_obs else 0.0)
    obs = obs + np.conj(np.transpose(obs, (0, 2, 1)))
    return dict(states_bar=rng.standard_normal((2 * N, slots, c)), pop_bar=rng.standard_normal((n_groups, slots, c)),
                level_map=rng.standard_normal((n_groups, N)), expect_bar=rng.standard_normal((n_obs, slots, c)), observables=obs)


def _objective(prob, Gp, Gq, off, pcof, order, save, bars):
    psi = pb.forward(prob, Gp, Gq, off, pcof, order)["psi"]
    S, P, E = pb.outputs(psi, save, bars.get("level_map"), bars.get("observables"))
    J = 0.0
    if bars.get("states_bar") is not None:
        J += np.sum(bars["states_bar"] * S)
    if bars.get("pop_bar") is not None:
        J += np.sum(bars["pop_bar"] * P)
    if bars.get("expect_bar") is not None:
        J += np.sum(bars["expect_bar"] * E)
    return J


def _differences(prob, Gp, Gq, off, pcof, order, save, bars, h=1e-3):
    def fd(hh):
        out = np.zeros(len(pcof))
        for l in range(len(pcof)):
            e = np.zeros(len(pcof)); e[l] = hh
            out[l] = (_objective(prob, Gp, Gq, off, pcof + e, order, save, bars)
                      - _objective(prob, Gp, Gq, off, pcof - e, order, save, bars)) / (2 * hh)
        return out
    return (4 * fd(h / 2) - fd(h)) / 3


@pytest.mark.parametrize("name,order,save", [("cnot2", 2, 1), ("cnot2", 4, 1), ("cnot2", 8, 1), ("guarded", 6, 1),
                                             ("cnot2", 4, 5), ("rand21x11", 4, 1), ("rand21x11", 4, 2)])
def test_proto_pullback_matches_differences(qgd, name, order, save):
    prob, ctrl, pcof, _ = _case(qgd, name)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    bars = _cotangents(qgd, prob, np.random.default_rng(13), save)
    parts = {"all": bars,
             "states": dict(states_bar=bars["states_bar"]),
             "populations": dict(pop_bar=bars["pop_bar"], level_map=bars["level_map"]),
             "expectations": dict(expect_bar=bars["expect_bar"], observables=bars["observables"])}
    total = np.zeros(len(pcof))
    for label, part in parts.items():
        g = pb.pullback(prob, Gp, Gq, off, pcof, order, save_every=save, **part)
        F = _differences(prob, Gp, Gq, off, pcof, order, save, part)
        err, sc = np.abs(g - F).max(), np.abs(F).max()
        print(f"{name} order {order} save {save} {label}: max|g - fd| = {err:.2e}, max|fd| = {sc:.2e}")
        assert err <= 1e-9 * sc, label
        if label == "all":
            whole = g
        else:
            total += g
    assert np.abs(total - whole).max() <= 1e-13 * max(1.0, np.abs(whole).max())      # the parts add up


def test_proto_pullback_conventions(qgd):
    """The n = 0 rule, populations without a map, a real diagonal observable as a one-row map, and the guard penalty and the
    :Infidelity terminal cost of proto_propagator.evaluate as cotangents of the states."""
    import proto_propagator as pp
    prob, ctrl, pcof, target = _case(qgd, "guarded")
    order = 6
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    rng = np.random.default_rng(3)
    fwd = pb.forward(prob, Gp, Gq, off, pcof, order)
    run = lambda **k: pb.pullback(prob, Gp, Gq, off, pcof, order, fwd=fwd, **k)
    sb = rng.standard_normal((2 * N, nt, c))
    g = run(states_bar=sb)
    sb0 = sb.copy(); sb0[:, 0] = 7.0
    assert np.array_equal(run(states_bar=sb0), g)
    pbar, d = rng.standard_normal((N, nt, c)), rng.standard_normal(N)
    S, _, _ = pb.outputs(fwd["psi"])
    assert np.abs(run(pop_bar=pbar) - run(states_bar=2 * np.concatenate([pbar, pbar]) * S)).max() <= 1e-13 * np.abs(g).max()
    eb = rng.standard_normal((1, nt, c))
    assert np.abs(run(expect_bar=eb, observables=np.diag(d)) - run(pop_bar=eb, level_map=d[None])).max() <= 1e-13 * np.abs(g).max()
    # the objective of the first-order gradient: guard penalty (trapezoid weights) + terminal infidelity
    ref = pp.evaluate(prob, Gp, Gq, off, pcof, target, order)
    trap = np.ones(nt); trap[0] = trap[-1] = 0.5
    W = np.asarray(prob.guard_subspace_projector)
    cot = (2 * fwd["dt"] / prob.tf) * trap[None, :, None] * np.einsum("ij,jkc->ikc", W, S)
    a, b = ref["overlap"]
    T = np.asarray(target)
    term = -(2 / prob.N_ess_levels ** 2) * (a + 1j * b) * T
    cot[:, -1] += np.concatenate([term.real, term.imag])
    err = np.abs(run(states_bar=cot) - ref["grad"]).max()
    print(f"guard + infidelity as a states cotangent: max|g - grad| = {err:.2e}, max|grad| = {np.abs(ref['grad']).max():.2e}")
    assert err <= 1e-13 * max(1.0, np.abs(ref["grad"]).max())
