"""numpy statement of the exact Hessian of the discrete objective, built on proto_propagator.py.
Test infrastructure only: the device kernels (csrc/qgd_k_hessian.hip) are compared with it term by term.

    H_kl = Phi''[s_k(N), s_l(N)] + Gamma''[s_k, s_l] + Ghat_k(s_l) + Ghat_l(s_k) + E_kl

s_l: forced-sweep sensitivities at every time point; Ghat_k(s): the gradient formula with the state history replaced by s
(same lambda, same reverse-swept seeds g_j); E: the second derivative of the Hermite recursion without d2A (zero at order 2).
:Infidelity plus guard penalty only (proto_propagator's objective)."""
import numpy as np

import proto_propagator as pp


def _bases(prob, m):
    out = []
    for k in range(prob.N_operators):
        for tau, Om in (("p", -1j * prob.sym_operators[k]), ("q", prob.asym_operators[k] + 0j)):
            for d in range(m):
                out.append((k, tau, d, Om))
    return out


def hessian(prob, Gp, Gq, offsets, pcof, target, order, terms=False):
    """H [n_pcof, n_pcof]; terms=True: (H, dict(phi=, guard=, ghat=, E=)) with ghat the non-symmetric Ghat_k(s_l)."""
    m = order // 2
    ref = pp.evaluate(prob, Gp, Gq, offsets, pcof, target, order)
    N, c, S = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps
    dt = prob.tf / S
    nt = S + 1
    Ac, ws, Linv, P, lam, g = ref["Ac"], ref["ws"], ref["Linv"], ref["P"], ref["lam"], ref["g"]
    cj = [pp.coefficient(j, m, m) for j in range(m + 1)]
    bases = _bases(prob, m)
    U = {}
    for (k, tau, d, Om) in bases:      # basis responses of k_forced_basis
        Ub = [np.zeros((nt, N, c), complex)]
        for j in range(m):
            acc = np.zeros((nt, N, c), complex)
            for i in range(j + 1):
                acc += Ac[:, j - i] @ Ub[i]
            if j >= d:
                acc += Om @ ws[j - d]
            Ub.append(acc / (j + 1))
        U[k, tau, d] = Ub
    npc = len(pcof)
    Gb = np.zeros((len(bases), nt, npc))       # table entries G_{b,l}(t_n)
    for bi, (k, tau, d, Om) in enumerate(bases):
        gk = (Gp if tau == "p" else Gq)[k]
        Gb[bi, :, offsets[k]:offsets[k] + gk.shape[2]] = gk[:, d]
    s_hist = np.zeros((npc, nt, N, c), complex)
    for l in range(npc):
        s = np.zeros((N, c), complex)
        for n in range(S):
            r = np.zeros((N, c), complex)
            for bi, (k, tau, d, Om) in enumerate(bases):
                rR = sum(cj[j] * dt ** j * U[k, tau, d][j][n] for j in range(1, m + 1))
                rL = sum(cj[j] * (-dt) ** j * U[k, tau, d][j][n + 1] for j in range(1, m + 1))
                r += Gb[bi, n, l] * rR - Gb[bi, n + 1, l] * rL
            s = P[n] @ s + Linv[n + 1] @ r
            s_hist[l, n + 1] = s
    T = np.asarray(target)
    a = np.array([np.sum(np.conj(T) * s_hist[l, -1]) for l in range(npc)])
    phi = -(2 / prob.N_ess_levels ** 2) * (np.outer(a.real, a.real) + np.outer(a.imag, a.imag))
    W = prob.guard_subspace_projector
    trap = np.ones(nt); trap[0] = trap[-1] = 0.5
    sr = np.concatenate([s_hist.real, s_hist.imag], axis=2)   # [l, nt, 2N, c]
    Ws = np.einsum("ij,lnjc->lnic", W, sr)
    guard = (2 * dt / prob.tf) * np.einsum("n,knic,lnic->kl", trap, sr, Ws)
    ghat = np.zeros((npc, npc))
    for l in range(npc):
        ghat[:, l] = pp.gradient_from(prob, Gp, Gq, offsets, pcof, Ac, s_hist[l], lam, m, dt)["grad"]
    e = np.zeros((nt, len(bases), len(bases)))
    for bi, (k, tau, d, Om) in enumerate(bases):
        for bj, (k2, tau2, d2, Om2) in enumerate(bases):
            for j in range(1, m + 1):
                if j - 1 - d >= 0:
                    e[:, bi, bj] += (1.0 / j) * np.einsum("nic,nic->n", np.conj(Om @ U[k2, tau2, d2][j - 1 - d]), g[j]).real
                if j - 1 - d2 >= 0:
                    e[:, bi, bj] += (1.0 / j) * np.einsum("nic,nic->n", np.conj(Om2 @ U[k, tau, d][j - 1 - d2]), g[j]).real
    E = -np.einsum("bnk,nbc,cnl->kl", Gb, e, Gb)
    H = phi + guard + ghat + ghat.T + E
    if terms:
        return H, dict(phi=phi, guard=guard, ghat=ghat, E=E, s=s_hist)
    return H


def grad_fd_hessian(prob, Gp, Gq, offsets, pcof, target, order, h=1e-3):
    """Richardson-extrapolated central differences (h, h/2) of proto_propagator's gradient."""
    def fd(hh):
        n = len(pcof)
        out = np.zeros((n, n))
        for l in range(n):
            e = np.zeros(n); e[l] = hh
            out[:, l] = (pp.evaluate(prob, Gp, Gq, offsets, pcof + e, target, order)["grad"]
                         - pp.evaluate(prob, Gp, Gq, offsets, pcof - e, target, order)["grad"]) / (2 * hh)
        return out
    return (4 * fd(h / 2) - fd(h)) / 3
