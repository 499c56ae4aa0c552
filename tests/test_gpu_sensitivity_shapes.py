"""GPU tests of the sensitivity entry points -- eval_states / eval_populations / eval_expectations, discrete_adjoint,
eval_grad_forced, eval_hessian, eval_hessian_vec, eval_pullback, eval_pushforward, eval_dense_* and eval_dense_pullback -- at the
shapes their own test files hold constant: more than one column group (ngrp = cp / 8 = 2 and 3), a last group with an odd number
of columns, two and three 16-row blocks (Np = 32 and 48), N = 60 in 64-row tiles, dense operators at Np = 64, sparse operators at
Np = 32, and the fused front with padding rows.  The problems are cases.sensitivity_case's; DESIGN.md section 5 ("Shapes of the
sensitivity tests") lists which shape reaches which branch.

The same tests run at cases.SENSITIVITY_ORDER_SHAPES, where the kernels branch on the order and on the control operators: orders
10 .. 16 (m = 5 .. 8: past the fused front's m <= 4, past launch_gradpoint64_m's m <= 5, the ELL kernels' and the sweep kernels'
last m = 8, 144 KB of LDS in k_forced_basis at Np = 64), 1, 4, 5 and 8 control operators (DISPATCH_NOPS cases 1 and 4, the
generic instantiation) with coefficient counts that differ between the operators, and NB = 2 n_ops m = 64 basis directions, the
last slot of k_hvp_forcing and k_hess_sigma.  Their controls are B-splines under carriers; tests/test_sensitivity_orders_proto.py
asserts on the CPU that every Taylor level of the control basis moves these references by 1000 times the bounds below.  Section 10
is one problem past the 64 directions (NB = 70), section 11 one past the 8 operators.

Every comparison is against a numpy statement of tests/ (proto_propagator, proto_hessian, proto_hvp, proto_pullback,
proto_pushforward, proto_dense_pullback), computed once per shape and shared; the device is compared with itself only where the
claim is that two calls give the same bits.  Direction counts differ from the group counts (3 directions beside 2 groups, 2 beside
3), so a transposed (direction, group) index does not land on itself.

Bounds, those of the files that test each entry point today: Hessian 1e-11 max|H0| (test_gpu_hessian.py); Hessian-vector product
1e-11 max|H0| |v|_1 (test_gpu_hvp.py); outputs, pullback and pushforward 1e-10 max(1, max|ref|) (test_gpu_pullback.py,
test_gpu_pushforward.py); adjoint against forced gradient 1e-12 relative; gradient against the numpy statement 1e-10 relative.
Two numpy formulations of one product (proto_hessian.hessian @ V, proto_hvp.hessian_vec) agree to 4e-15 .. 6.3e-13 of max|H| on
these problems (|v|_1 is 15 .. 40): the references leave more than two orders below the product's bound.  The measured figures of
the device are in DESIGN.md section 5.  Every comparison also requires its reference to be alive:
max|ref| of each block (column group, row block, direction, Hessian row) at least 1e-6 of the whole reference's.

(The tests are parametrised by the shape's index with the name as id, and name no shape in their bodies: tests/conftest.py runs a
test twice when its source or its parameters hold the name of a problem of N <= 4, and one of the names here contains such a
name.)"""
import types

import numpy as np
import pytest

import cases
import proto_dense_pullback as pdp
import proto_hessian as ph
import proto_hvp as pv
import proto_propagator as pp
import proto_pullback as pb
import proto_pushforward as pf
from test_gpu_hessian import _handle
from test_gpu_hvp import _paths
from test_gpu_pullback import _hermitian

pytestmark = pytest.mark.gpu

NAMES = cases.SENSITIVITY_SHAPES + cases.SENSITIVITY_ORDER_SHAPES      # (appended: the indices of the first six stay)
shapes = pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
REFINE = 3
L2_SHAPE = NAMES.index("rand40x20")            # (the route that does not fit in LDS: three groups, three row blocks)
SAVE_SHAPE = NAMES.index("rand21x11")          # (save_every = 2 on 5 steps: slots 0, 2, 4, the odd last column group)
FRONT_SHAPE = NAMES.index("levels543")
ABOVE_THE_FRONT = (NAMES.index("qutrits27o12"), NAMES.index("levels543o10"))      # (the qudit problems at m = 6 and 5: the front has m <= 4)
PAST_THE_DIRECTIONS = cases.SENSITIVITY_PAST_THE_DIRECTIONS
_cache = {}


def _n_vec(c):
    return 2 if (c + 7) // 8 == 3 else 3


def _shape(qgd, k):
    """The problem of shape k with its seeded inputs; what the numpy statements share (forward sweep, setup of the second-order
    sweep) is computed at first use, once, and read only."""
    if k in _cache:
        return _cache[k]
    name, seed = (k, 7100) if isinstance(k, str) else (NAMES[k], 7000 + k)      # (by name: the problem past the direction limit)
    prob, ctrl, pcof, target, order = cases.sensitivity_case(qgd, name)
    N, c, nt = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
    rng = np.random.default_rng(seed)
    s = types.SimpleNamespace(name=name, prob=prob, ctrl=ctrl, pcof=pcof, target=target, order=order, N=N, c=c, nt=nt,
                              n_vec=_n_vec(c), lm=rng.standard_normal((4, N)), oc=_hermitian(rng, 2, N),
                              orl=_hermitian(rng, 1, N, False))
    s.V = rng.standard_normal((len(pcof), s.n_vec))
    s.basis = qgd.control_basis(ctrl, prob.nsteps, prob.tf, order // 2)
    s.fwd = pb.forward(prob, *s.basis, pcof, order)
    _cache[k] = s
    return s


def _second_order(s):
    """proto_hvp.setup (which holds proto_propagator.evaluate as "ref") and proto_hessian.hessian of shape s, once"""
    if not hasattr(s, "pre"):
        s.pre = pv.setup(s.prob, *s.basis, s.pcof, s.target, s.order)
        s.H0 = ph.hessian(s.prob, *s.basis, s.pcof, s.target, s.order)
        rows = np.abs(s.H0).max(axis=1)
        assert rows.min() >= 1e-6 * rows.max(), f"{s.name}: a row of the reference Hessian is negligible"
    return s.pre, s.H0


def _bars(s, slots, seed):
    rng = np.random.default_rng(seed)
    return {"states": dict(states_bar=rng.standard_normal((2 * s.N, slots, s.c))),
            "populations with a 4-row map": dict(populations_bar=rng.standard_normal((4, slots, s.c)), level_map=s.lm),
            "populations without a map": dict(populations_bar=rng.standard_normal((s.N, slots, s.c))),
            "expectations, 2 complex observables": dict(expectations_bar=rng.standard_normal((2, slots, s.c)), observables=s.oc),
            "expectations, 1 real observable": dict(expectations_bar=rng.standard_normal((1, slots, s.c)), observables=s.orl)}


def _together(parts):
    return {**parts["states"], **parts["populations with a 4-row map"], **parts["expectations, 2 complex observables"]}


def _proto(part):
    names = dict(states_bar="states_bar", populations_bar="pop_bar", level_map="level_map", expectations_bar="expect_bar",
                 observables="observables")
    return {names[key]: a for key, a in part.items()}


def _alive(ref, what, first_slot=0):
    """The reference is no vacuous one: an output [rows, slots, c(, directions)] in blocks of 16 rows x 8 columns (x direction)
    -- the kernels' row blocks and column groups --, anything else entry group by entry group along its first axis."""
    ref = np.abs(np.asarray(ref))
    top = ref.max()
    assert top > 0, what
    if ref.ndim >= 3:
        ref = ref[:, first_slot:]
        ref = ref.reshape(ref.shape[:3] + (-1,))
        for r0 in range(0, ref.shape[0], 16):
            for c0 in range(0, ref.shape[2], 8):
                for d in range(ref.shape[3]):
                    low = ref[r0:r0 + 16, :, c0:c0 + 8, d].max()
                    assert low >= 1e-6 * top, f"{what}: rows {r0}.., columns {c0}.., direction {d} of the reference are negligible"
    else:
        low = ref.reshape(ref.shape[0], -1).max(axis=1).min() if ref.ndim == 2 else top
        assert low >= 1e-6 * top, f"{what}: a row of the reference is negligible"


def _close(x, ref, what, first_slot=0):
    """outputs, pullbacks and tangents: 1e-10 max(1, max|ref|)"""
    _alive(ref, what, first_slot)
    x = np.asarray(x)
    assert x.shape == np.shape(ref), (what, x.shape, np.shape(ref))
    err, bound = np.abs(x - ref).max(), 1e-10 * max(1.0, np.abs(ref).max())
    print(f"\n{what}: max|x - ref| = {err:.3e}, bound {bound:.3e}, max|ref| = {np.abs(ref).max():.3e}")
    assert np.all(np.isfinite(x)) and err <= bound, what


def _relative(x, ref, tol, what):
    _alive(ref, what)
    err, bound = np.abs(x - ref).max(), tol * np.abs(ref).max()
    print(f"\n{what}: max|x - ref| = {err:.3e}, bound {bound:.3e}, max|ref| = {np.abs(ref).max():.3e}")
    assert np.all(np.isfinite(x)) and err <= bound, what


def _open(qgd, s):
    return _handle(qgd, s.prob, s.ctrl, s.target, s.order)


def _assert_paths(s, paths):
    """what the shape is there for: dense operators on the random problems, the ELL kernels on the qudit problems"""
    want = ["dense"] if s.name.startswith(("rand", "ops")) else ["dense", "sparse"]
    assert paths == want, (s.name, paths)


# -- 1: forward outputs -------------------------------------------------------------------------------------------------------------

def _forward_outputs(dp, s, label):
    S, P, E = pb.outputs(s.fwd["psi"], 1, None, s.oc)
    _, Pm, Er = pb.outputs(s.fwd["psi"], 1, s.lm, s.orl)
    _close(dp.eval_states(s.pcof), S, f"{label}: eval_states")
    _close(dp.eval_populations(s.pcof), P, f"{label}: eval_populations")
    _close(dp.eval_populations(s.pcof, level_map=s.lm), Pm, f"{label}: eval_populations with a 4-row map")
    _close(dp.eval_expectations(s.oc, s.pcof), E, f"{label}: eval_expectations of 2 complex observables")
    _close(dp.eval_expectations(s.orl, s.pcof), Er, f"{label}: eval_expectations of 1 real observable")


@shapes
def test_forward_outputs(qgd, k, monkeypatch):
    s = _shape(qgd, k)
    dp = _open(qgd, s)
    try:
        paths = []
        for path in _paths(qgd, dp):
            paths.append(path)
            _forward_outputs(dp, s, f"{s.name} {path}")
            assert not dp.front_path_taken()
        _assert_paths(s, paths)
        if k == FRONT_SHAPE:                               # N = 60 in 64-row tiles on the fused front
            assert dp.operator_path()[0] == "sparse"
            monkeypatch.setenv("QGD_PATHS", "front")
            _forward_outputs(dp, s, f"{s.name} front")
            assert dp.front_path_taken()
    finally:
        dp.close()


# -- 2: gradients -------------------------------------------------------------------------------------------------------------------

@shapes
def test_gradients(qgd, k, monkeypatch):
    s = _shape(qgd, k)
    g0 = _second_order(s)[0]["ref"]["grad"]
    dp = _open(qgd, s)
    try:
        for path in _paths(qgd, dp):
            g = dp.discrete_adjoint(s.pcof)[0]
            assert k not in ABOVE_THE_FRONT or not dp.front_path_taken()
            _relative(g, g0, 1e-10, f"{s.name} {path}: discrete_adjoint vs proto_propagator.evaluate")
            _relative(dp.eval_grad_forced(s.pcof), g, 1e-12, f"{s.name} {path}: eval_grad_forced vs discrete_adjoint")
        if k == FRONT_SHAPE:
            monkeypatch.setenv("QGD_PATHS", "front")
            g = dp.discrete_adjoint(s.pcof)[0]
            assert dp.front_path_taken()
            _relative(g, g0, 1e-10, f"{s.name} front: discrete_adjoint vs proto_propagator.evaluate")
    finally:
        dp.close()


# -- 3: Hessian ---------------------------------------------------------------------------------------------------------------------

@shapes
def test_hessian(qgd, k):
    s = _shape(qgd, k)
    _, H0 = _second_order(s)
    sc = np.abs(H0).max()
    dp = _open(qgd, s)
    try:
        for path in _paths(qgd, dp):
            g_adj = dp.discrete_adjoint(s.pcof)[0]
            grad = np.zeros(len(s.pcof))
            H = dp.eval_hessian(s.pcof, grad=grad)
            err, asym = np.abs(H - H0).max(), np.abs(H - H.T).max()
            print(f"\n{s.name} {path}: max|H - H0| = {err:.3e}, bound {1e-11 * sc:.3e}; max|H - H^T| = {asym:.3e}, bound {1e-13 * sc:.3e}")
            assert np.all(np.isfinite(H)) and err <= 1e-11 * sc, path
            assert asym <= 1e-13 * sc, path
            _relative(grad, g_adj, 1e-12, f"{s.name} {path}: eval_hessian's grad vs discrete_adjoint")
            assert np.array_equal(H, dp.eval_hessian(s.pcof)), path
    finally:
        dp.close()


# -- 4: Hessian-vector products -----------------------------------------------------------------------------------------------------

@shapes
def test_hessian_vec(qgd, k):
    s = _shape(qgd, k)
    pre, H0 = _second_order(s)
    sc = np.abs(H0).max()
    ref = np.stack([pv.hessian_vec(s.prob, *s.basis, s.pcof, s.target, s.order, s.V[:, j], pre=pre) for j in range(s.n_vec)], axis=1)
    _alive(ref.T, f"{s.name}: H v of every direction")
    dp = _open(qgd, s)
    try:
        for path in _paths(qgd, dp):
            HV = dp.eval_hessian_vec(s.pcof, s.V)
            assert HV.shape == ref.shape
            for j in range(s.n_vec):
                one = dp.eval_hessian_vec(s.pcof, s.V[:, j])
                bound = 1e-11 * sc * np.abs(s.V[:, j]).sum()
                e1, eb = np.abs(one - ref[:, j]).max(), np.abs(HV[:, j] - ref[:, j]).max()
                print(f"\n{s.name} {path} direction {j}: max|hv - ref| = {e1:.3e} alone, {eb:.3e} in the batch, bound {bound:.3e}")
                assert np.all(np.isfinite(one)) and e1 <= bound and eb <= bound, (path, j)
                assert np.array_equal(HV[:, j], one), (path, j)
    finally:
        dp.close()


# -- 5: pullback --------------------------------------------------------------------------------------------------------------------

def _pullbacks(dp, s, save, label):
    slots = 1 + s.prob.nsteps // save
    parts = _bars(s, slots, 500 + save)
    parts["all three at once"] = _together(parts)
    for what, part in parts.items():
        ref = pb.pullback(s.prob, *s.basis, s.pcof, s.order, save_every=save, fwd=s.fwd, **_proto(part))
        _close(dp.eval_pullback(s.pcof, **part), ref, f"{label}: {what}")


@shapes
def test_pullback(qgd, k):
    s = _shape(qgd, k)
    dp = _open(qgd, s)
    try:
        for path in _paths(qgd, dp):
            _pullbacks(dp, s, 1, f"{s.name} {path}")
        if k == SAVE_SHAPE:
            dp.set_save_every(2)
            assert dp._slots() == 3
            _pullbacks(dp, s, 2, f"{s.name} save_every 2")
    finally:
        dp.close()


# -- 6: pushforward -----------------------------------------------------------------------------------------------------------------

def _tangent_refs(s):
    pre = _second_order(s)[0]
    psi = pre["ref"]["psi"]
    dpsi = [pf.state_tangent(s.prob, *s.basis, s.pcof, s.target, s.order, s.V[:, j], pre=pre) for j in range(s.n_vec)]
    stack = lambda i, **kw: np.stack([pf.tangents(psi, d, 1, **kw)[i] for d in dpsi], axis=-1)
    return dict(states=stack(0), populations=stack(1), expectations=stack(2, observables=s.oc),
                populations_map=stack(1, level_map=s.lm), expectations_real=stack(2, observables=s.orl))


@shapes
def test_pushforward(qgd, k):
    s = _shape(qgd, k)
    ref = _tangent_refs(s)
    parts = _bars(s, s.nt, 600)
    dp = _open(qgd, s)
    try:
        for path in _paths(qgd, dp):
            a = dp.eval_pushforward(s.pcof, s.V, states=True, populations=True, observables=s.oc)
            b = dp.eval_pushforward(s.pcof, s.V, level_map=s.lm, observables=s.orl)
            label = f"{s.name} {path}, {s.n_vec} directions"
            _close(a["states"], ref["states"], f"{label}: states tangent", 1)
            _close(a["populations"], ref["populations"], f"{label}: populations tangent", 1)
            _close(a["expectations"], ref["expectations"], f"{label}: expectations tangent, 2 complex observables", 1)
            _close(b["populations"], ref["populations_map"], f"{label}: populations tangent with a 4-row map", 1)
            _close(b["expectations"], ref["expectations_real"], f"{label}: expectations tangent, 1 real observable", 1)
            for j in range(s.n_vec):                       # side by side == one at a time
                a1 = dp.eval_pushforward(s.pcof, s.V[:, j], states=True, populations=True, observables=s.oc)
                b1 = dp.eval_pushforward(s.pcof, s.V[:, j], level_map=s.lm, observables=s.orl)
                for got, one in ((a, a1), (b, b1)):
                    for kind in got:
                        assert np.array_equal(got[kind][..., j], one[kind]), (path, kind, j)
            # duality with the pullback: <ybar, J v> = <g, v>, the bound of test_gpu_pushforward.py
            for kind, out, bar in (("states", a["states"], parts["states"]),
                                   ("populations", b["populations"], parts["populations with a 4-row map"]),
                                   ("expectations", a["expectations"], parts["expectations, 2 complex observables"])):
                g = dp.eval_pullback(s.pcof, **bar)
                ybar = bar[f"{kind}_bar"]
                for j in range(s.n_vec):
                    jv, gv = np.sum(ybar * out[..., j]), g @ s.V[:, j]
                    err, bound = abs(jv - gv), 1e-10 * max(1.0, np.abs(g).max()) * np.abs(s.V[:, j]).sum()
                    print(f"\n{label} {kind} direction {j}: |<ybar, J v> - <g, v>| = {err:.3e}, bound {bound:.3e}, |<g, v>| = {abs(gv):.3e}")
                    assert abs(gv) >= 1e-6 * np.abs(g).max() and err <= bound, (path, kind, j)
    finally:
        dp.close()


# -- 7: dense output ----------------------------------------------------------------------------------------------------------------

def _dense_refs(qgd, s):
    S, P, E = pdp.dense_outputs(qgd, s.prob, *s.basis, s.pcof, s.order, REFINE, None, s.oc)
    _, Pm, Er = pdp.dense_outputs(qgd, s.prob, *s.basis, s.pcof, s.order, REFINE, s.lm, s.orl)
    parts = _bars(s, 1 + s.prob.nsteps * REFINE, 700)
    parts["all three at once"] = _together(parts)
    refs = {what: pdp.dense_pullback(qgd, s.prob, *s.basis, s.pcof, s.order, REFINE, fwd=s.fwd, **_proto(part))
            for what, part in parts.items()}
    return (S, P, E, Pm, Er), parts, refs


def _dense_outputs_and_pullbacks(dp, s, outputs, parts, refs, label):
    S, P, E, Pm, Er = outputs
    _close(dp.eval_dense_states(REFINE, s.pcof), S, f"{label}: eval_dense_states")
    _close(dp.eval_dense_populations(REFINE, s.pcof), P, f"{label}: eval_dense_populations")
    _close(dp.eval_dense_populations(REFINE, s.pcof, level_map=s.lm), Pm, f"{label}: eval_dense_populations with a 4-row map")
    _close(dp.eval_dense_expectations(REFINE, s.oc, s.pcof), E, f"{label}: eval_dense_expectations of 2 complex observables")
    _close(dp.eval_dense_expectations(REFINE, s.orl, s.pcof), Er, f"{label}: eval_dense_expectations of 1 real observable")
    for what, part in parts.items():
        _close(dp.eval_dense_pullback(REFINE, s.pcof, **part), refs[what], f"{label}: dense pullback, {what}")


@shapes
def test_dense_output_and_its_pullback(qgd, k):
    s = _shape(qgd, k)
    outputs, parts, refs = _dense_refs(qgd, s)
    dp = _open(qgd, s)
    try:
        for path in _paths(qgd, dp):
            _dense_outputs_and_pullbacks(dp, s, outputs, parts, refs, f"{s.name} {path} refine {REFINE}")
    finally:
        dp.close()


# -- 8: the route that does not fit in LDS ----------------------------------------------------------------------------------------

def test_planes_in_lds_and_from_l2_give_the_same_bits(qgd, monkeypatch):
    """Three column groups, three row blocks: the pullback, the pushforward and the expectations with the map and the planes
    staged in LDS, then under QGD_PATHS=planes_l2 read from L2 -- the same bits, and the numpy statement's figures."""
    s = _shape(qgd, L2_SHAPE)
    assert (s.N, s.c) == (40, 20)
    parts = _bars(s, s.nt, 800)
    ref = _tangent_refs(s)
    dp = _open(qgd, s)
    try:
        def calls():
            return (dp.eval_pullback(s.pcof, **_together(parts)),
                    dp.eval_pushforward(s.pcof, s.V, states=True, level_map=s.lm, observables=s.oc),
                    dp.eval_expectations(s.oc, s.pcof))
        g, jv, ex = calls()
        monkeypatch.setenv("QGD_PATHS", "planes_l2")
        g2, jv2, ex2 = calls()
        monkeypatch.delenv("QGD_PATHS")
        assert np.array_equal(g, g2) and np.array_equal(ex, ex2)
        assert set(jv) == set(jv2) == {"states", "populations", "expectations"}
        for kind in jv:
            assert np.array_equal(jv[kind], jv2[kind]), kind
        _close(g2, pb.pullback(s.prob, *s.basis, s.pcof, s.order, fwd=s.fwd, **_proto(_together(parts))), f"{s.name} planes_l2: pullback")
        _close(jv2["populations"], ref["populations_map"], f"{s.name} planes_l2: populations tangent with a 4-row map", 1)
        _close(jv2["expectations"], ref["expectations"], f"{s.name} planes_l2: expectations tangent", 1)
        _close(ex2, pb.outputs(s.fwd["psi"], 1, None, s.oc)[2], f"{s.name} planes_l2: eval_expectations")
    finally:
        dp.close()


# -- 9: one past the limit ----------------------------------------------------------------------------------------------------------

def test_refusals_at_65_levels(qgd):
    """N = 65, one past the 64 rows the sensitivity kernels hold: every entry point that has the limit refuses with
    QGD_ERR_UNSUPPORTED and the handle goes on working (the forced gradient and the dense outputs have kernels for N > 64)."""
    prob, ctrl, pcof, target = cases.synthetic_case(qgd, N=65, c=3, n_ops=2, nsteps=3, tf=0.3)
    N, c, nt = 65, 3, 4
    rng = np.random.default_rng(65)
    v, sb = rng.standard_normal(len(pcof)), rng.standard_normal((2 * N, nt, c))
    dense_sb = rng.standard_normal((2 * N, 1 + 3 * REFINE, c))
    dp = _handle(qgd, prob, ctrl, target, 4)
    try:
        g0 = dp.discrete_adjoint(pcof)[0]
        for what, call in (("eval_hessian", lambda: dp.eval_hessian(pcof)),
                           ("eval_hessian_vec", lambda: dp.eval_hessian_vec(pcof, v)),
                           ("eval_pullback", lambda: dp.eval_pullback(pcof, states_bar=sb)),
                           ("eval_pushforward", lambda: dp.eval_pushforward(pcof, v, states=True)),
                           ("eval_dense_pullback", lambda: dp.eval_dense_pullback(REFINE, pcof, states_bar=dense_sb))):
            with pytest.raises(qgd._lib.QGDError) as ei:
                call()
            assert ei.value.code == qgd._lib.QGD_ERR_UNSUPPORTED, (what, ei.value.code)
            assert dp.lib.qgd_last_error(dp.h).decode(), what
            assert np.array_equal(dp.discrete_adjoint(pcof)[0], g0), what
    finally:
        dp.close()


# -- 10: past the limit of 64 basis directions --------------------------------------------------------------------------------------

def test_past_64_basis_directions(qgd):
    """5 operators at order 14: NB = 2 * 5 * 7 = 70 basis directions.  The entry points that keep one value per direction in 64
    slots (eval_hessian, eval_hessian_vec, eval_pushforward) refuse with QGD_ERR_UNSUPPORTED and leave the handle working; the
    ones without that limit -- both gradients, the pullback, the dense pullback, the forward and dense outputs -- are compared
    with their statements on the same handle, at the bounds of sections 1, 2, 5 and 7."""
    s = _shape(qgd, PAST_THE_DIRECTIONS)
    assert 2 * s.prob.N_operators * (s.order // 2) == 70
    g0 = pp.evaluate(s.prob, *s.basis, s.pcof, s.target, s.order)["grad"]
    dense = _dense_refs(qgd, s)
    dp = _open(qgd, s)
    try:
        first = dp.discrete_adjoint(s.pcof)[0]
        for what, call in (("eval_hessian", lambda: dp.eval_hessian(s.pcof)),
                           ("eval_hessian_vec", lambda: dp.eval_hessian_vec(s.pcof, s.V[:, 0])),
                           ("eval_hessian_vec of a batch", lambda: dp.eval_hessian_vec(s.pcof, s.V)),
                           ("eval_pushforward", lambda: dp.eval_pushforward(s.pcof, s.V, states=True))):
            with pytest.raises(qgd._lib.QGDError) as ei:
                call()
            assert ei.value.code == qgd._lib.QGD_ERR_UNSUPPORTED, (what, ei.value.code)
            assert dp.lib.qgd_last_error(dp.h).decode(), what
            assert np.array_equal(dp.discrete_adjoint(s.pcof)[0], first), what
        paths = []
        for path in _paths(qgd, dp):
            paths.append(path)
            label = f"{s.name} {path}"
            g = dp.discrete_adjoint(s.pcof)[0]
            _relative(g, g0, 1e-10, f"{label}: discrete_adjoint vs proto_propagator.evaluate")
            _relative(dp.eval_grad_forced(s.pcof), g, 1e-12, f"{label}: eval_grad_forced vs discrete_adjoint")
            _forward_outputs(dp, s, label)
            _pullbacks(dp, s, 1, label)
            _dense_outputs_and_pullbacks(dp, s, *dense, f"{label} refine {REFINE}")
        _assert_paths(s, paths)
    finally:
        dp.close()


# -- 11: past the limit of 8 control operators --------------------------------------------------------------------------------------

def test_nine_control_operators_are_refused(qgd):
    """The kernels hold the coefficients of at most 8 control operators (QGD_MAX_OPS_DEV): a ninth is refused when the handle is
    made, 8 are taken."""
    prob = qgd.construct_rand_prob(6, 9, tf=1.0, nsteps=3)
    with pytest.raises(qgd._lib.QGDError) as ei:
        qgd.DeviceProblem(prob, 4)
    assert ei.value.code == qgd._lib.QGD_ERR_UNSUPPORTED
    assert "8 control operators" in str(ei.value)
    qgd.DeviceProblem(qgd.construct_rand_prob(6, 8, tf=1.0, nsteps=3), 4).close()
