"""Ensemble (robust, "risk-neutral") evaluation: ONE coefficient vector over ``K`` variants of a problem that differ in the
system Hamiltonian and, optionally, in a scale factor per control operator, each with a quadrature weight (detuned qubit
frequencies, uncertain couplings, mis-calibrated drive amplitudes).  DESIGN.md section 4m.

  Ensemble(system_sym, system_asym, op_scale=None, weights=None)     the members; from_problems, member_problem
  ensemble_reduce(member_grads, member_out3, weights, cost_type, n_ess)   THE statement of the weighted sums
  eval_ensemble / discrete_adjoint_ensemble(prob, controls, pcof, target, ensemble; order, cost_type, route)

Two routes, the same bits.  ``route="loop"``: every member is evaluated on a handle of its own (``member_problem``), whatever
its size and its controls, and the rows are reduced on the host by ensemble_reduce: a fixed statement, k ascending, every
product and sum rounded on its own.  ``route="device"``: the members run side by side on the handle of the problem itself
(``DeviceProblem.set_ensemble`` / ``eval_ensemble``, qgd_eval_ensemble: small problems with controls linear in pcof), and the
sums are formed on the device, bitwise equal to that statement; an objective then downloads one gradient per evaluation
instead of K.  ``route="auto"`` (the default): the device where the library takes the problem, else the loop.
"""
from __future__ import annotations

import inspect
import weakref

import numpy as np

from . import evolution as _ev
from .controls import as_control_list
from .schrodinger_prob import SchrodingerProb


def _real_array(a, name, ndim):
    a = np.asarray(a)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be real; got dtype {a.dtype}")
    if a.ndim != ndim:
        raise ValueError(f"{name} must have {ndim} dimensions; got shape {a.shape}")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError(f"{name} must be finite")
    return a


class Ensemble:
    """``K`` members: ``system_sym [K, N, N]`` (each exactly symmetric), ``system_asym [K, N, N]`` (each exactly antisymmetric),
    ``op_scale [K, n_ops]`` or None (ones), ``weights [K]`` or None (every weight ``1.0 / K``).  Member ``k`` of a problem is that
    problem with ``system_sym[k]``, ``system_asym[k]`` and the control operators ``op_scale[k, o] * operator_o``."""

    def __init__(self, system_sym, system_asym, op_scale=None, weights=None):
        S = _real_array(system_sym, "system_sym", 3)
        A = _real_array(system_asym, "system_asym", 3)
        if S.shape[0] < 1:
            raise ValueError("system_sym holds no member: an ensemble needs at least one (K >= 1)")
        if S.shape[1] != S.shape[2]:
            raise ValueError(f"system_sym must be [K, N, N]; got shape {S.shape}")
        if A.shape != S.shape:
            raise ValueError(f"system_asym must have the shape {S.shape} of system_sym; got {A.shape}")
        for k in range(S.shape[0]):
            if not np.array_equal(S[k], S[k].T):
                raise ValueError(f"system_sym: member {k} is not symmetric")
            if not np.array_equal(A[k], -A[k].T):
                raise ValueError(f"system_asym: member {k} is not anti-symmetric")
        if op_scale is not None:
            op_scale = _real_array(op_scale, "op_scale", 2)
            if op_scale.shape[0] != S.shape[0]:
                raise ValueError(f"op_scale must be [K = {S.shape[0]}, n_ops]; got shape {op_scale.shape}")
        if weights is not None:
            weights = _real_array(weights, "weights", 1)
            if weights.shape[0] != S.shape[0]:
                raise ValueError(f"weights must have K = {S.shape[0]} entries; got {weights.shape[0]}")
        self.system_sym, self.system_asym, self.op_scale, self.weights = S, A, op_scale, weights
        self._members = {}

    @property
    def K(self):
        return self.system_sym.shape[0]

    @property
    def N(self):
        return self.system_sym.shape[1]

    def __len__(self):
        return self.K

    def effective_weights(self):
        """The weights the reduction uses: the given ones, or ``K`` times the double ``1.0 / K``."""
        return self.weights if self.weights is not None else np.full(self.K, 1.0 / self.K)

    def check_problem(self, prob):
        if prob.N_tot_levels != self.N:
            raise ValueError(f"ensemble: the members have {self.N} levels, the problem {prob.N_tot_levels}")
        if self.op_scale is not None and self.op_scale.shape[1] != prob.N_operators:
            raise ValueError(f"ensemble: op_scale has {self.op_scale.shape[1]} columns for {prob.N_operators} control operators")

    @classmethod
    def from_problems(cls, probs, weights=None):
        """The ensemble of problems that differ in the system Hamiltonian alone (anything else differing is refused)."""
        probs = list(probs)
        if not probs:
            raise ValueError("probs holds no member: an ensemble needs at least one")
        p0 = probs[0]
        for k, p in enumerate(probs[1:], 1):
            for name in ("N_tot_levels", "N_ess_levels", "N_operators", "N_initial_conditions", "tf", "nsteps"):
                if getattr(p, name) != getattr(p0, name):
                    raise ValueError(f"probs: member {k} differs from member 0 in {name}")
            for name in ("u0", "v0", "guard_subspace_projector"):
                if not np.array_equal(getattr(p, name), getattr(p0, name)):
                    raise ValueError(f"probs: member {k} differs from member 0 in {name}")
            for name in ("sym_operators", "asym_operators"):
                if not all(np.array_equal(a, b) for a, b in zip(getattr(p, name), getattr(p0, name))):
                    raise ValueError(f"probs: member {k} differs from member 0 in {name}")
        return cls(np.stack([p.system_sym for p in probs]), np.stack([p.system_asym for p in probs]), None, weights)

    def member_problems(self, prob):
        """``member_problem(prob, k)`` for every ``k``, made once per problem and kept until ``prob`` is garbage-collected,
        changes (operators, initial conditions, guard, grid, essential levels) or ``release_members(prob)`` is called: the
        functional forms evaluate on these, so that the handles ``device_problem`` caches for them are reused."""
        key = id(prob)
        fp = (_ev._fingerprint(prob), prob.tf, prob.nsteps, prob.gmres_abstol, prob.gmres_reltol, prob.preconditioner_type)
        ent = self._members.get(key)
        if ent is None or ent[0]() is not prob or ent[1] != fp:
            self.release_members(prob)
            members = [self.member_problem(prob, k) for k in range(self.K)]
            self._members[key] = (weakref.ref(prob), fp, members)
            weakref.finalize(prob, self._members.pop, key, None)
            return members
        return ent[2]

    def release_members(self, prob):
        """Forget the members made for ``prob`` and close their handles; the cached handles of ``prob`` itself forget this
        ensemble (the device route uploaded it there)."""
        ent = self._members.pop(id(prob), None)
        for mp in (ent[2] if ent else ()):
            _ev.release(mp)
        for key, held in list(_ev._cache.items()):
            if key[0] == id(prob) and held[0]() is prob:
                set_on = getattr(held[1], "_ensemble", None)
                if set_on is not None and set_on[0]() is self:
                    held[1].set_ensemble(None)

    def operator_arrays(self, sym_operators, asym_operators):
        """What qgd_set_ensemble takes for these members of a problem with these control operators, no device involved:
        ``(system_sym [K, N, N], system_asym [K, N, N], sym_ops [K, n_ops, N, N], asym_ops [K, n_ops, N, N], weights [K])``,
        C-contiguous float64 with every matrix stored TRANSPOSED -- the column-major bytes of the matrix itself, as the
        DeviceProblem constructor hands the operators of one problem over (the same ``_f`` conversion).  The control operators are
        ``op_scale[k, o] * operator_o``, one multiply per entry (the arithmetic of member_problem); without ``op_scale`` they are
        taken as they are.  The weights are ``effective_weights()``."""
        K, N, n_ops = self.K, self.N, len(sym_operators)
        if self.op_scale is not None and self.op_scale.shape[1] != n_ops:
            raise ValueError(f"ensemble: op_scale has {self.op_scale.shape[1]} columns for {n_ops} control operators")
        ss = np.ascontiguousarray(np.stack([_ev._f(self.system_sym[k]).T for k in range(K)]))
        sa = np.ascontiguousarray(np.stack([_ev._f(self.system_asym[k]).T for k in range(K)]))
        so, ao = np.zeros((K, max(n_ops, 1), N, N)), np.zeros((K, max(n_ops, 1), N, N))
        for k in range(K):
            for o in range(n_ops):
                sym, asym = sym_operators[o], asym_operators[o]
                if self.op_scale is not None:
                    sym, asym = self.op_scale[k, o] * sym, self.op_scale[k, o] * asym
                so[k, o], ao[k, o] = _ev._f(sym).T, _ev._f(asym).T
        return ss, sa, so, ao, np.ascontiguousarray(self.effective_weights(), dtype=np.float64)

    def device_arrays(self, prob):
        """``operator_arrays`` for the control operators of ``prob``."""
        self.check_problem(prob)
        return self.operator_arrays(prob.sym_operators, prob.asym_operators)

    def member_problem(self, prob, k):
        """A SchrodingerProb copy of ``prob`` carrying member ``k``'s operators: its system Hamiltonian, and the control
        operators times ``op_scale[k, o]`` (one multiply per entry); everything else is ``prob``'s, by value."""
        self.check_problem(prob)
        if not 0 <= k < self.K:
            raise IndexError(f"member {k} of an ensemble of {self.K}")
        s = self.op_scale[k] if self.op_scale is not None else np.ones(prob.N_operators)
        return SchrodingerProb(self.system_sym[k], self.system_asym[k],
                               [s[o] * op for o, op in enumerate(prob.sym_operators)],
                               [s[o] * op for o, op in enumerate(prob.asym_operators)],
                               prob.u0, prob.v0, prob.guard_subspace_projector, prob.tf, prob.nsteps, prob.N_ess_levels,
                               prob.gmres_abstol, prob.gmres_reltol, prob.preconditioner_type)


def ensemble_reduce(member_grads, member_out3, weights, cost_type, n_ess):
    """The weighted sums over the members, as plain loops over ``k`` ascending with every product and every sum rounded on its
    own:

        cost_k  = 1.0 - (a_k*a_k + b_k*b_k) / float(n_ess*n_ess)    for Infidelity, (a_k, b_k) = member_out3[k][0..1]
                = member_out3[k][0]                                 for every other cost type
        guard_k = member_out3[k][2]
        acc = 0.0;  for k = 0 .. K-1:  acc = acc + w_k * x_k        (x = cost, guard, and each gradient entry)

    ``weights`` None: every weight the double ``1.0 / K``.  Returns ``(grad or None, cost, guard)``."""
    code = _ev.COST_TYPES.get(str(cost_type)) if not isinstance(cost_type, (int, np.integer)) else int(cost_type)
    if code is None:
        raise ValueError(f"Invalid cost type: {cost_type}")
    out3 = np.asarray(member_out3, dtype=np.float64).reshape(-1, 3)
    K = out3.shape[0]
    if K < 1:
        raise ValueError("member_out3 holds no member")
    w = np.full(K, 1.0 / K) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (K,):
        raise ValueError(f"weights must have K = {K} entries; got shape {w.shape}")
    G = None
    if member_grads is not None:
        G = np.asarray(member_grads, dtype=np.float64)
        if G.ndim != 2 or G.shape[0] != K:
            raise ValueError(f"member_grads must be [K = {K}, n_pcof]; got shape {G.shape}")
    d = float(int(n_ess) * int(n_ess))
    cost, guard = 0.0, 0.0
    grad = None if G is None else np.zeros(G.shape[1])
    for k in range(K):
        wk = float(w[k])
        a, b = float(out3[k, 0]), float(out3[k, 1])
        ck = 1.0 - (a * a + b * b) / d if code == 0 else a
        cost = cost + wk * ck
        guard = guard + wk * float(out3[k, 2])
        if grad is not None:
            grad = grad + wk * G[k]
    return grad, cost, guard


class EnsembleResult(tuple):
    """What the functional forms return: ``(grad or None, cost, guard)`` as a tuple, plus the members' rows ``member_grads``
    ``[K, n_pcof]`` (or None) and ``member_out3`` ``[K, 3]`` (both None from an evaluation that asked for no rows), and the
    ``route`` that produced them (``"loop"`` or ``"device"``)."""

    def __new__(cls, grad, cost, guard, member_grads, member_out3, *, route="loop"):
        self = super().__new__(cls, (grad, cost, guard))
        self.grad, self.cost, self.guard = grad, cost, guard
        self.member_grads, self.member_out3, self.route = member_grads, member_out3, route
        return self


ROUTES = ("auto", "device", "loop")


def _check_route(route):
    if route not in ROUTES:
        raise ValueError(f"route must be one of {ROUTES}; got {route!r}")


def _evaluate(prob, controls, pcof, target, ensemble, order, cost_type, gradient, route="auto"):
    # every refusal that needs no device comes before a handle is asked for
    _check_route(route)
    if not isinstance(ensemble, Ensemble):
        raise ValueError(f"ensemble must be an Ensemble; got {type(ensemble).__name__}")
    ensemble.check_problem(prob)
    if _ev.COST_TYPES.get(str(cost_type)) is None:
        raise ValueError(f"Invalid cost type: {cost_type}")
    cl = as_control_list(controls)
    if len(cl) != prob.N_operators:
        raise ValueError(f"{len(cl)} controls for {prob.N_operators} control operators")
    n_pcof = int(sum(c.N_coeff for c in cl))
    pc = np.asarray(pcof)
    if pc.dtype.kind not in "fiu":
        raise ValueError(f"pcof must be real; got dtype {pc.dtype}")
    pc = np.ascontiguousarray(pc, dtype=np.float64)
    if pc.shape != (n_pcof,):
        raise ValueError(f"pcof must have shape ({n_pcof},); got {pc.shape}")
    if gradient and target is None:
        raise ValueError("target: a gradient needs one")
    return _loop_members(prob, controls, pc, target, ensemble, order, cost_type, gradient, route=route, rows=True)


_COST_NAMES = {0: "Infidelity", 1: "Tracking", 2: "Norm", 3: "StateTransfer"}


def _device_members(dp, controls, pc, target, ensemble, cost_type, gradient, rows):
    """The members side by side on ``dp``, the handle of the problem itself, with its controls, target and cost type set; the
    handle leaves with the cost type it came with."""
    dp.set_controls(controls)
    if target is not None:
        dp.set_target(target)
    before = _COST_NAMES[getattr(dp, "_cost_type", 0)]
    dp.set_cost_type(cost_type)
    try:
        dp.set_ensemble(ensemble)
        grad, cost, guard, mg, mo, _ = dp.eval_ensemble(pc, gradient=gradient, rows=rows)
    finally:
        dp.set_cost_type(before)
    return EnsembleResult(grad, cost, guard, mg, mo, route="device")


def _loop_members(prob, controls, pc, target, ensemble, order, cost_type, gradient, route="auto", rows=True):
    """The members' evaluation, on the route asked for.

    ``"device"``: side by side on the handle of ``prob`` itself (``_device_members``); ``rows=False`` leaves the members' rows on
    the device.  ``"loop"``: one handle per member, then the statement on the host.  The members' problems are
    ``ensemble.member_problems(prob)``, kept for the lifetime of ``prob``, so their handles stay in ``device_problem``'s cache
    from call to call (a loop of evaluations pays for K handles once); ``release_members`` closes them.  A member's handle
    leaves with the cost type it came with.  The loop always has the rows.  ``"auto"``: the device unless the nominal handle
    forms its control tables on the host (controls that are not linear in pcof) or the library answers QGD_ERR_UNSUPPORTED
    (anything but a small problem on the small-problem path); then the loop."""
    _check_route(route)
    if route == "device" or (route == "auto" and prob.N_tot_levels <= 4):      # (N > 4 is never the device's: no nominal handle is made for it)
        E = _ev._lib
        dp = _ev.device_problem(prob, order)
        dp.set_controls(controls)
        if getattr(dp, "_general", None):
            if route == "device":
                raise E.QGDError(E.QGD_ERR_UNSUPPORTED, "the device route of an ensemble needs controls linear in pcof")
        else:
            try:
                return _device_members(dp, controls, pc, target, ensemble, cost_type, gradient, rows)
            except E.QGDError as e:
                if route == "device" or e.code != E.QGD_ERR_UNSUPPORTED:
                    raise
    K = ensemble.K
    mg = np.zeros((K, len(pc))) if gradient else None
    mo = np.zeros((K, 3))
    for k, mp in enumerate(ensemble.member_problems(prob)):
        dk = _ev.device_problem(mp, order)
        dk.set_controls(controls)
        if target is not None:
            dk.set_target(target)
        before = _COST_NAMES[getattr(dk, "_cost_type", 0)]
        dk.set_cost_type(cost_type)
        try:
            if gradient:
                mg[k], mo[k] = dk.discrete_adjoint(pc)
            else:
                mo[k] = dk.eval_forward(pc)
        finally:
            dk.set_cost_type(before)
    grad, cost, guard = ensemble_reduce(mg, mo, ensemble.weights, _ev.COST_TYPES[str(cost_type)], prob.N_ess_levels)
    return EnsembleResult(grad, cost, guard, mg, mo, route="loop")


class EnsembleObjective:
    """The robust objective of an optimiser: ``obj(pcof) -> (grad, cost, guard)``; ``close()`` closes the members' handles.  It
    asks for no member rows: on the device route one gradient comes back per evaluation, not K."""

    def __init__(self, prob, controls, target, ensemble, order, cost_type, route="auto"):
        _check_route(route)
        if not isinstance(ensemble, Ensemble):
            raise ValueError(f"ensemble must be an Ensemble; got {type(ensemble).__name__}")
        ensemble.check_problem(prob)
        self.prob, self.controls, self.target, self.ensemble = prob, controls, target, ensemble
        self.order, self.cost_type, self.route = order, cost_type, route
        self._members, self._keywords = None, {}

    def __call__(self, pcof):
        pc = np.ascontiguousarray(pcof, dtype=np.float64)
        members = _loop_members      # (the module global at the time of the call: a member evaluation put in its place counts)
        if members is not self._members:
            # one written against the eight positional arguments this function had before it took keywords is called as before
            par = inspect.signature(members).parameters
            takes = any(p.kind is inspect.Parameter.VAR_KEYWORD for p in par.values()) or {"route", "rows"} <= set(par)
            self._members, self._keywords = members, (dict(route=self.route, rows=False) if takes else {})
        res = members(self.prob, self.controls, pc, self.target, self.ensemble, self.order, self.cost_type, True, **self._keywords)
        return res.grad, res.cost, res.guard

    def close(self):
        self.ensemble.release_members(self.prob)


def eval_ensemble(prob, controls, pcof, target, ensemble, order=2, cost_type="Infidelity", gradient=True, route="auto"):
    """One ``pcof`` over the members of ``ensemble``: ``(grad or None, cost, guard)`` with ``cost = sum_k w_k cost_k``,
    ``guard = sum_k w_k guard_k`` and ``grad`` the gradient of their sum (ensemble_reduce is the statement).  The result also
    carries ``member_grads``, ``member_out3`` and the ``route`` it took (``route=``: "auto", "device" or "loop"; the same bits)."""
    return _evaluate(prob, controls, pcof, target, ensemble, order, cost_type, gradient, route)


def discrete_adjoint_ensemble(prob, controls, pcof, target, ensemble, order=2, cost_type="Infidelity", route="auto"):
    """eval_ensemble with the gradient: the robust counterpart of discrete_adjoint."""
    return _evaluate(prob, controls, pcof, target, ensemble, order, cost_type, True, route)
