"""numpy statement of the pullback of trajectory outputs to pcof (qgd_eval_pullback), in the notation
of proto_propagator.py / proto_hvp.py.  Test infrastructure only: csrc/qgd_k_pullback.hip is compared with it.

The three outputs along the sweep, slot k holding time point n = k * save_every, w = [u; v] <-> psi = u + iv:

    S[:, k, col] = w_n                                  [2N, n_slots, c]           (eval_states)
    P[g, k, col] = sum_l M[g, l] (u_l^2 + v_l^2)        [n_groups or N, n_slots, c] (eval_populations; M = I without a map)
    E[j, k, col] = Re(psi^H O_j psi),  O_j = A_j + iB_j [n_obs, n_slots, c]        (eval_expectations)

With cotangents Sbar, Pbar, Ebar the derivative of J = <Sbar, S> + <Pbar, P> + <Ebar, E> with respect to w_n is

    f_n = Sbar[:, k, col] + 2 (M^T Pbar[:, k, col]) (.) [u; v] + 2 sum_j Ebar[j, k, col] [A_j u - B_j v; A_j v + B_j u]

at the time points a slot addresses and zero at the others; f_0 is dropped (the initial state does not depend on pcof).
dJ/dpcof = sum_n Re<s_k(n), f_n> is term (B) of proto_hvp.py: the adjoint recursion with forcing F = -f and terminal value
F_N gives mu, and the first-order gradient contraction runs with mu in place of lambda.  No weights are applied: the caller's
cotangent is the whole weight."""
import numpy as np

import proto_propagator as pp


def forward(prob, Gp, Gq, offsets, pcof, order):
    """The forward sweep of proto_propagator.evaluate alone: psi [nt, N, c] and what the adjoint recursion reads."""
    m = order // 2
    N, c, S = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps
    dt = prob.tf / S
    tp, tq = pp.tables(Gp, Gq, offsets, np.asarray(pcof, float), m)
    Ac = pp.assemble(prob, tp, tq, m)
    L, R, _ = pp.build_LR(Ac, m, dt)
    Linv = np.linalg.inv(L)
    P = Linv[1:] @ R[:-1]
    psi = np.zeros((S + 1, N, c), dtype=complex)
    psi[0] = prob.u0 + 1j * prob.v0
    for n in range(S):
        psi[n + 1] = P[n] @ psi[n]
    return dict(m=m, dt=dt, Ac=Ac, Linv=Linv, P=P, psi=psi)


def _observables(observables, N):
    obs = np.asarray(observables)
    return (obs[None] if obs.ndim == 2 else obs).astype(complex).reshape(-1, N, N)


def outputs(psi, save_every=1, level_map=None, observables=None):
    """(S, P, E) of a trajectory psi [nt, N, c], in the layouts of the three entry points; E is None without observables."""
    N = psi.shape[1]
    ps = psi[::save_every]                                         # [n_slots, N, c]
    S = np.concatenate([ps.real, ps.imag], axis=1).transpose(1, 0, 2)
    pop = (np.abs(ps) ** 2).transpose(1, 0, 2)
    P = pop if level_map is None else np.einsum("gl,lkc->gkc", np.asarray(level_map, float), pop)
    E = None
    if observables is not None:
        E = np.einsum("kic,jil,klc->jkc", np.conj(ps), _observables(observables, N), ps).real
    return S, P, E


def cotangent_forcing(psi, save_every=1, states_bar=None, pop_bar=None, level_map=None, expect_bar=None, observables=None):
    """f [nt, N, c] complex (f_u + i f_v): the derivative of <bar, outputs> with respect to every w_n; f_0 = 0."""
    nt, N, c = psi.shape
    f = np.zeros((nt, N, c), dtype=complex)
    idx = np.arange(0, nt, save_every)                             # the time point of every slot
    ps = psi[idx]
    if states_bar is not None:
        sb = np.asarray(states_bar, float)
        f[idx] += (sb[:N] + 1j * sb[N:]).transpose(1, 0, 2)
    if pop_bar is not None:
        pb = np.asarray(pop_bar, float)
        wl = pb if level_map is None else np.einsum("gl,gkc->lkc", np.asarray(level_map, float), pb)
        f[idx] += 2.0 * wl.transpose(1, 0, 2) * ps
    if expect_bar is not None:
        eb = np.asarray(expect_bar, float)
        f[idx] += 2.0 * np.einsum("jkc,jil,klc->kic", eb, _observables(observables, N), ps)
    f[0] = 0.0
    return f


def pullback(prob, Gp, Gq, offsets, pcof, order, save_every=1, states_bar=None, pop_bar=None, level_map=None,
             expect_bar=None, observables=None, fwd=None, terms=False):
    """grad [n_pcof] = sum over the parts given of <bar, d output / d pcof>."""
    if fwd is None:
        fwd = forward(prob, Gp, Gq, offsets, pcof, order)
    P, Linv, psi, S = fwd["P"], fwd["Linv"], fwd["psi"], prob.nsteps
    F = -cotangent_forcing(psi, save_every, states_bar, pop_bar, level_map, expect_bar, observables)
    y = np.zeros_like(F)
    y[-1] = F[-1]
    for n in range(S - 1, 0, -1):
        y[n] = P[n].conj().T @ y[n + 1] + F[n]
    mu = np.zeros_like(y)
    mu[1:] = np.conj(np.transpose(Linv[1:], (0, 2, 1))) @ y[1:]
    grad = pp.gradient_from(prob, Gp, Gq, offsets, pcof, fwd["Ac"], psi, mu, fwd["m"], fwd["dt"])["grad"]
    if terms:
        return grad, dict(F=F, y=y, mu=mu)
    return grad
