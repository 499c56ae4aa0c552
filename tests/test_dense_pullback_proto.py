"""The numpy statement of the dense-output pullback (proto_dense_pullback.py) against Richardson central differences of its
own dense outputs contracted with random cotangents (CPU), and its conventions.

Bound: 1e-9 max|fd|, the bound of test_pullback_proto.py (steps h = 1e-3 and h / 2, extrapolated; the reasoning is in that
file's docstring).  The measured figures are in DESIGN.md section 4j."""
import numpy as np
import pytest

import proto_dense_pullback as pdp
import proto_pullback as pb
from test_hessian_proto import _case


def _cotangents(prob, rng, refine, n_obs=3, n_groups=3):
    N, c = prob.N_tot_levels, prob.N_initial_conditions
    slots = 1 + prob.nsteps * refine
    obs = rng.standard_normal((n_obs, N, N)) + 1j * rng.standard_normal((n_obs, N, N))
    obs = obs + np.conj(np.transpose(obs, (0, 2, 1)))
    return dict(states_bar=rng.standard_normal((2 * N, slots, c)), pop_bar=rng.standard_normal((n_groups, slots, c)),
                level_map=rng.standard_normal((n_groups, N)), expect_bar=rng.standard_normal((n_obs, slots, c)), observables=obs)


def _objective(qgd, prob, Gp, Gq, off, pcof, order, refine, bars):
    S, P, E = pdp.dense_outputs(qgd, prob, Gp, Gq, off, pcof, order, refine, bars.get("level_map"), bars.get("observables"))
    J = 0.0
    if bars.get("states_bar") is not None:
        J += np.sum(bars["states_bar"] * S)
    if bars.get("pop_bar") is not None:
        J += np.sum(bars["pop_bar"] * P)
    if bars.get("expect_bar") is not None:
        J += np.sum(bars["expect_bar"] * E)
    return J


def _differences(qgd, prob, Gp, Gq, off, pcof, order, refine, bars, h=1e-3):
    def fd(hh):
        out = np.zeros(len(pcof))
        for l in range(len(pcof)):
            e = np.zeros(len(pcof)); e[l] = hh
            out[l] = (_objective(qgd, prob, Gp, Gq, off, pcof + e, order, refine, bars)
                      - _objective(qgd, prob, Gp, Gq, off, pcof - e, order, refine, bars)) / (2 * hh)
        return out
    return (4 * fd(h / 2) - fd(h)) / 3


def _parts(bars):
    return {"all": bars,
            "states": dict(states_bar=bars["states_bar"]),
            "populations": dict(pop_bar=bars["pop_bar"], level_map=bars["level_map"]),
            "expectations": dict(expect_bar=bars["expect_bar"], observables=bars["observables"])}


@pytest.mark.parametrize("name,order,refine", [("cnot2", 2, 2), ("cnot2", 4, 3), ("cnot2", 8, 3), ("guarded", 6, 7),
                                               ("cnot2", 16, 2), ("rand21x11", 4, 3)])
def test_proto_dense_pullback_matches_differences(qgd, name, order, refine):
    prob, ctrl, pcof, _ = _case(qgd, name)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    bars = _cotangents(prob, np.random.default_rng(13), refine)
    fwd = pb.forward(prob, Gp, Gq, off, pcof, order)
    total = np.zeros(len(pcof))
    for label, part in _parts(bars).items():
        g, t = pdp.dense_pullback(qgd, prob, Gp, Gq, off, pcof, order, refine, fwd=fwd, terms=True, **part)
        F = _differences(qgd, prob, Gp, Gq, off, pcof, order, refine, part)
        err, sc = np.abs(g - F).max(), np.abs(F).max()
        print(f"{name} order {order} refine {refine} {label}: max|g - fd| = {err:.2e}, max|fd| = {sc:.2e}, "
              f"max|explicit| = {np.abs(t['explicit']).max():.2e}")
        assert err <= 1e-9 * sc, label
        if label == "all":
            whole = g
        else:
            total += g
    assert np.abs(total - whole).max() <= 1e-13 * max(1.0, np.abs(whole).max())      # the parts add up


def test_proto_dense_pullback_conventions(qgd):
    """Slot 0 is ignored; a cotangent that is zero off the grid slots is the grid-point pullback of those slots, and so is
    refine = 1; the explicit part is no rounding matter (without it the difference check above fails)."""
    prob, ctrl, pcof, _ = _case(qgd, "cnot2")
    order, refine = 4, 3
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    rng = np.random.default_rng(13)
    bars = _cotangents(prob, rng, refine)
    fwd = pb.forward(prob, Gp, Gq, off, pcof, order)
    run = lambda r, **k: pdp.dense_pullback(qgd, prob, Gp, Gq, off, pcof, order, r, fwd=fwd, **k)
    g, t = run(refine, terms=True, **bars)
    tol = 1e-13 * max(1.0, np.abs(g).max())
    # slot 0
    moved = {k: (v.copy() if k in ("states_bar", "pop_bar", "expect_bar") else v) for k, v in bars.items()}
    for k in ("states_bar", "pop_bar", "expect_bar"):
        moved[k][:, 0] = 7.0
    assert np.array_equal(run(refine, **moved), g)
    # zero off the grid slots
    grid, wide = {}, {}
    for k, v in bars.items():
        if k in ("states_bar", "pop_bar", "expect_bar"):
            grid[k] = v[:, ::refine].copy()
            wide[k] = np.zeros_like(v); wide[k][:, ::refine] = grid[k]
        else:
            grid[k] = wide[k] = v
    ref = pb.pullback(prob, Gp, Gq, off, pcof, order, fwd=fwd, **grid)
    gw, tw = run(refine, terms=True, **wide)
    assert np.abs(gw - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    assert not np.any(tw["explicit"])
    # refine = 1
    assert np.abs(run(1, **grid) - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    # the explicit part
    ex = np.abs(t["explicit"]).max()
    print(f"cnot2 order 4 refine 3: max|explicit| = {ex:.2e}, max|g| = {np.abs(g).max():.2e}")
    assert ex > 1e-3 * np.abs(g).max()
    assert np.abs(t["implicit"] + t["explicit"] - g).max() <= tol
