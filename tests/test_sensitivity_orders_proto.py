"""What makes the GPU comparisons at orders 10 .. 16 and at 1 .. 8 control operators (test_gpu_sensitivity_shapes.py at
cases.SENSITIVITY_ORDER_SHAPES and at cases.SENSITIVITY_PAST_THE_DIRECTIONS) meaningful, on the CPU.

At high order the top Taylor levels of the control basis can contribute less than the bounds of the GPU tests: with a small
dt |A|, or with controls whose higher time derivatives vanish (a cubic B-spline has none from the fourth on), a kernel that is
wrong in level 6 would pass.  So, for each of the eight problems:

(i)   every level counts: with Gp[k][:, d, :] and Gq[k][:, d, :] zeroed for all operators k, for each d = 0 .. m - 1 in turn,
      proto_hvp.setup's gradient moves by at least 1e-7 max|grad| and its state history by at least 1e-7 absolute -- 1000 times
      the 1e-10 bounds those two are compared at on the device;
(ii)  every operator counts: each operator's block of rows of the reference Hessian has a maximum of at least 1e-6 max|H0|;
(iii) the statements agree with each other: proto_hvp.hessian_vec against proto_hessian.hessian @ v to 1e-13 max|H0| |v|_1 (two
      orders below the device's bound of the product), <ybar, J v> of proto_pushforward against <g, v> of proto_pullback to
      1e-13 max(1, max|g|) |v|_1;
(iv)  at ops4o16 and qutrits27o12 the statement's gradient and state history are tied to the oracle (cases.oracle_pins).

The figures are printed (pytest -s)."""
import types

import numpy as np
import pytest

import cases
import proto_hessian as ph
import proto_hvp as pv
import proto_pullback as pb
import proto_pushforward as pf

NAMES = cases.SENSITIVITY_ORDER_SHAPES + (cases.SENSITIVITY_PAST_THE_DIRECTIONS,)
shapes = pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
PINNED = [NAMES.index("ops4o16"), NAMES.index("qutrits27o12")]
_cache = {}


def _shape(qgd, k):
    if k not in _cache:
        prob, ctrl, pcof, target, order = cases.sensitivity_case(qgd, NAMES[k])
        s = types.SimpleNamespace(name=NAMES[k], prob=prob, ctrl=ctrl, pcof=pcof, target=target, order=order, m=order // 2)
        s.basis = qgd.control_basis(ctrl, prob.nsteps, prob.tf, s.m)
        s.pre = pv.setup(prob, *s.basis, pcof, target, order)
        _cache[k] = s
    return _cache[k]


def _hessian(s):
    if not hasattr(s, "H0"):
        s.H0 = ph.hessian(s.prob, *s.basis, s.pcof, s.target, s.order)
    return s.H0


def test_the_shapes_are_the_stated_ones(qgd):
    """N, columns, order, steps, number of basis directions NB = 2 n_ops m and number of parameters of every problem"""
    want = {"ops8o8": (12, 5, 8, 4, 64, 138), "ops4o16": (20, 9, 16, 3, 64, 74), "ops1o16": (64, 3, 16, 3, 16, 24),
            "ops2o12": (64, 9, 12, 3, 24, 34), "ops5o12": (33, 10, 12, 3, 60, 90), "qutrits27o12": (27, 8, 12, 5, 36, 48),
            "levels543o10": (60, 8, 10, 6, 30, 48), "ops5o14": (10, 3, 14, 3, 70, 90)}
    assert set(want) == set(NAMES)
    for name in NAMES:
        prob, ctrl, pcof, target, order = cases.sensitivity_case(qgd, name)
        got = (prob.N_tot_levels, prob.N_initial_conditions, order, prob.nsteps, 2 * prob.N_operators * (order // 2), len(pcof))
        assert got == want[name], (name, got)
        assert target.shape == got[:2]
        counts = [c.N_coeff for c in ctrl]
        if name.startswith("ops") and len(ctrl) > 1:
            assert len(set(counts)) > 1, (name, counts)      # (an offset taken from another operator does not land on itself)


@shapes
def test_every_level_of_the_control_basis_counts(qgd, k):
    s = _shape(qgd, k)
    Gp, Gq, off = s.basis
    g0, psi0 = s.pre["ref"]["grad"], s.pre["ref"]["psi"]
    gs = np.abs(g0).max()
    for d in range(s.m):
        Gp_d, Gq_d = [g.copy() for g in Gp], [g.copy() for g in Gq]
        for g in Gp_d + Gq_d:
            g[:, d, :] = 0.0
        ref = pv.setup(s.prob, Gp_d, Gq_d, off, s.pcof, s.target, s.order)["ref"]
        dg, dpsi = np.abs(ref["grad"] - g0).max() / gs, np.abs(ref["psi"] - psi0).max()
        print(f"\n{s.name} without level {d}: the gradient moves by {dg:.2e} of max|grad|, the states by {dpsi:.2e}")
        assert dg >= 1e-7 and dpsi >= 1e-7, (s.name, d, dg, dpsi)


@shapes
def test_every_operator_counts(qgd, k):
    s = _shape(qgd, k)
    H0 = _hessian(s)
    off = list(s.basis[2]) + [len(s.pcof)]
    blocks = [np.abs(H0[off[j]:off[j + 1]]).max() for j in range(len(off) - 1)]
    print(f"\n{s.name}: max|H0| of the operators' row blocks, smallest / largest = {min(blocks) / max(blocks):.2e}")
    assert len(blocks) == s.prob.N_operators and off[-1] > off[-2]
    assert min(blocks) >= 1e-6 * np.abs(H0).max(), (s.name, blocks)


@shapes
def test_the_statements_agree_with_each_other(qgd, k):
    s = _shape(qgd, k)
    H0 = _hessian(s)
    prob, N, c, nt = s.prob, s.prob.N_tot_levels, s.prob.N_initial_conditions, s.prob.nsteps + 1
    rng = np.random.default_rng(9000 + k)
    fwd = pb.forward(prob, *s.basis, s.pcof, s.order)
    assert np.array_equal(fwd["psi"], s.pre["ref"]["psi"])
    lm = rng.standard_normal((4, N))
    O = rng.standard_normal((2, N, N)) + 1j * rng.standard_normal((2, N, N))
    O = 0.5 * (O + np.conj(np.transpose(O, (0, 2, 1))))
    bars = {"states": dict(states_bar=rng.standard_normal((2 * N, nt, c))),
            "populations": dict(pop_bar=rng.standard_normal((4, nt, c)), level_map=lm),
            "expectations": dict(expect_bar=rng.standard_normal((2, nt, c)), observables=O)}
    g = {kind: pb.pullback(prob, *s.basis, s.pcof, s.order, fwd=fwd, **part) for kind, part in bars.items()}
    for j in range(2):
        v = rng.standard_normal(len(s.pcof))
        hv, t = pv.hessian_vec(prob, *s.basis, s.pcof, s.target, s.order, v, pre=s.pre, terms=True)
        err, bound = np.abs(hv - H0 @ v).max(), 1e-13 * np.abs(H0).max() * np.abs(v).sum()
        print(f"\n{s.name} direction {j}: max|hessian_vec - hessian @ v| = {err:.2e}, bound {bound:.2e} ({err / (np.abs(H0).max() * np.abs(v).sum()):.1e} of max|H0| |v|_1)")
        assert err <= bound, (s.name, j)
        S, P, E = pf.tangents(s.pre["ref"]["psi"], t["sv"], 1, lm, O)
        jv = {"states": np.sum(bars["states"]["states_bar"] * S), "populations": np.sum(bars["populations"]["pop_bar"] * P),
              "expectations": np.sum(bars["expectations"]["expect_bar"] * E)}
        for kind in jv:
            gv = g[kind] @ v
            err, scale = abs(jv[kind] - gv), max(1.0, np.abs(g[kind]).max()) * np.abs(v).sum()
            print(f"{s.name} direction {j} {kind}: |<ybar, J v> - <g, v>| = {err:.2e}, bound {1e-13 * scale:.2e} ({err / scale:.1e} relative)")
            assert abs(gv) >= 1e-6 * np.abs(g[kind]).max() and err <= 1e-13 * scale, (s.name, j, kind)


@pytest.mark.parametrize("k", PINNED, ids=[NAMES[k] for k in PINNED])
def test_the_statement_is_the_oracles(qgd, orc, k):
    s = _shape(qgd, k)
    assert cases.oracle_pins(orc, s.prob, s.ctrl, s.pcof, s.target, s.order, s.pre["ref"]), "outside the oracle's budget"
