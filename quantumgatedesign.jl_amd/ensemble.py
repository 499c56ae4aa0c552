"""Ensemble (robust, "risk-neutral") evaluation: ONE coefficient vector over ``K`` variants of a problem that differ in the
system Hamiltonian and, optionally, in a scale factor per control operator, each with a quadrature weight (detuned qubit
frequencies, uncertain couplings, mis-calibrated drive amplitudes).  DESIGN.md section 4m.

  Ensemble(system_sym, system_asym, op_scale=None, weights=None)     the members; from_problems, member_problem
  ensemble_reduce(member_grads, member_out3, weights, cost_type, n_ess)   THE statement of the weighted sums
  eval_ensemble / discrete_adjoint_ensemble(prob, controls, pcof, target, ensemble; order, cost_type)

Every member is evaluated on a handle of its own (``member_problem``), whatever its size and its controls, and the rows are
reduced on the host by ensemble_reduce: a fixed statement, k ascending, every product and sum rounded on its own, so that
a later device-side reduction has a definition to be bitwise equal to.
"""
from __future__ import annotations

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
        """Forget the members made for ``prob`` and close their handles."""
        ent = self._members.pop(id(prob), None)
        for mp in (ent[2] if ent else ()):
            _ev.release(mp)

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
    ``[K, n_pcof]`` (or None) and ``member_out3`` ``[K, 3]``."""

    def __new__(cls, grad, cost, guard, member_grads, member_out3):
        self = super().__new__(cls, (grad, cost, guard))
        self.grad, self.cost, self.guard = grad, cost, guard
        self.member_grads, self.member_out3 = member_grads, member_out3
        return self


def _evaluate(prob, controls, pcof, target, ensemble, order, cost_type, gradient):
    # every refusal that needs no device comes before a handle is asked for
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
    return _loop_members(prob, controls, pc, target, ensemble, order, cost_type, gradient)


_COST_NAMES = {0: "Infidelity", 1: "Tracking", 2: "Norm", 3: "StateTransfer"}


def _loop_members(prob, controls, pc, target, ensemble, order, cost_type, gradient):
    """One handle per member, then the statement on the host.  The members' problems are ``ensemble.member_problems(prob)``,
    kept for the lifetime of ``prob``, so their handles stay in ``device_problem``'s cache from call to call (a loop of
    evaluations pays for K handles once); ``release_members`` closes them.  A member's handle leaves with the cost type it
    came with."""
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
    return EnsembleResult(grad, cost, guard, mg, mo)


class EnsembleObjective:
    """The robust objective of an optimiser: ``obj(pcof) -> (grad, cost, guard)``; ``close()`` closes the members' handles."""

    def __init__(self, prob, controls, target, ensemble, order, cost_type):
        if not isinstance(ensemble, Ensemble):
            raise ValueError(f"ensemble must be an Ensemble; got {type(ensemble).__name__}")
        ensemble.check_problem(prob)
        self.prob, self.controls, self.target, self.ensemble = prob, controls, target, ensemble
        self.order, self.cost_type = order, cost_type

    def __call__(self, pcof):
        pc = np.ascontiguousarray(pcof, dtype=np.float64)
        res = _loop_members(self.prob, self.controls, pc, self.target, self.ensemble, self.order, self.cost_type, True)
        return res.grad, res.cost, res.guard

    def close(self):
        self.ensemble.release_members(self.prob)


def eval_ensemble(prob, controls, pcof, target, ensemble, order=2, cost_type="Infidelity", gradient=True):
    """One ``pcof`` over the members of ``ensemble``: ``(grad or None, cost, guard)`` with ``cost = sum_k w_k cost_k``,
    ``guard = sum_k w_k guard_k`` and ``grad`` the gradient of their sum (ensemble_reduce is the statement).  The result also
    carries ``member_grads`` and ``member_out3``."""
    return _evaluate(prob, controls, pcof, target, ensemble, order, cost_type, gradient)


def discrete_adjoint_ensemble(prob, controls, pcof, target, ensemble, order=2, cost_type="Infidelity"):
    """eval_ensemble with the gradient: the robust counterpart of discrete_adjoint."""
    return _evaluate(prob, controls, pcof, target, ensemble, order, cost_type, True)
