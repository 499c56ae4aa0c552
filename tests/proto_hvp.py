"""numpy statement of the exact Hessian-vector product by a second-order adjoint sweep, in the
notation of proto_propagator.py / proto_hessian.py.  Test infrastructure only: csrc/qgd_k_hvp.hip is compared with it.

With s_v = sum_l v_l s_l (ONE forced sweep, forcing direction gv[n][b] = sum_l G_{b,l}(t_n) v_l), z_b(n) the adjoint of
the homogeneous Taylor recursion applied to the seeds (k_hess_basis' panels) and e_n its half-matrices:

    (H v)_k = - sum_n sum_b G_{b,k}(t_n) ( Re<s_v(n), z_b(n)> + sum_b' e_n[b,b'] gv[n][b'] )          (A)
              + sum_n Re<s_k(n), f_n>                                                                  (B)
    f_n = - sum_b gv[n][b] z_b(n) + (2 dt/tf) trap_n W s_v(n),      f_N += Phi'' s_v(N) = -(2/N_ess^2) <T, s_v(N)> T

(B) is the first-order gradient's shape: the adjoint sweep with terminal condition and forcing -f (the first-order
adjoint runs with -dJ/dpsi), then the gradient contraction against the forward history with mu in place of lambda.
The sensitivities s_l of the individual parameters are never formed.  :Infidelity plus guard penalty (proto_propagator's
objective)."""
import numpy as np

import proto_propagator as pp
from proto_hessian import _bases


def setup(prob, Gp, Gq, offsets, pcof, target, order):
    """Everything that does not depend on v: the forward / adjoint evaluation, the basis responses' step forcings, the
    panels z_b(n), the matrices e_n and the table G_{b,l}(t_n)."""
    m = order // 2
    ref = pp.evaluate(prob, Gp, Gq, offsets, pcof, target, order)
    N, c, S = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps
    dt = prob.tf / S
    nt = S + 1
    Ac, ws, g = ref["Ac"], ref["ws"], ref["g"]
    AcH = np.conj(np.transpose(Ac, (0, 1, 3, 2)))
    cj = [pp.coefficient(j, m, m) for j in range(m + 1)]
    bases = _bases(prob, m)
    NB = len(bases)
    U, rR, rL = [], [], []
    for (k, tau, d, Om) in bases:      # basis responses of k_forced_basis
        Ub = [np.zeros((nt, N, c), complex)]
        for j in range(m):
            acc = np.zeros((nt, N, c), complex)
            for i in range(j + 1):
                acc += Ac[:, j - i] @ Ub[i]
            if j >= d:
                acc += Om @ ws[j - d]
            Ub.append(acc / (j + 1))
        U.append(Ub)
        rR.append(sum(cj[j] * dt ** j * Ub[j] for j in range(1, m + 1)))
        rL.append(sum(cj[j] * (-dt) ** j * Ub[j] for j in range(1, m + 1)))
    Gb = np.zeros((NB, nt, len(pcof)))
    for bi, (k, tau, d, Om) in enumerate(bases):
        gk = (Gp if tau == "p" else Gq)[k]
        Gb[bi, :, offsets[k]:offsets[k] + gk.shape[2]] = gk[:, d]
    # z_b = y_0 of the adjoint recursion: y_i = Omega_b^H g_{i+d+1}/(i+d+1), then y_i += A_{J-1-i}^H y_J / J, J = m-1 .. 1
    Z = np.zeros((NB, nt, N, c), complex)
    for bi, (k, tau, d, Om) in enumerate(bases):
        OmH = np.conj(Om.T)
        y = [(OmH @ g[i + d + 1]) / (i + d + 1) if i + d + 1 <= m else np.zeros((nt, N, c), complex) for i in range(m)]
        for J in range(m - 1, 0, -1):
            for i in range(J):
                y[i] = y[i] + (AcH[:, J - 1 - i] @ y[J]) / J
        Z[bi] = y[0]
    e = np.zeros((nt, NB, NB))
    for bi, (k, tau, d, Om) in enumerate(bases):
        for bj, (k2, tau2, d2, Om2) in enumerate(bases):
            for j in range(1, m + 1):
                if j - 1 - d >= 0:
                    e[:, bi, bj] += (1.0 / j) * np.einsum("nic,nic->n", np.conj(Om @ U[bj][j - 1 - d]), g[j]).real
                if j - 1 - d2 >= 0:
                    e[:, bi, bj] += (1.0 / j) * np.einsum("nic,nic->n", np.conj(Om2 @ U[bi][j - 1 - d2]), g[j]).real
    return dict(ref=ref, m=m, dt=dt, nt=nt, rR=rR, rL=rL, Gb=Gb, Z=Z, e=e)


def hessian_vec(prob, Gp, Gq, offsets, pcof, target, order, v, pre=None, terms=False):
    """H v [n_pcof]; pre: the result of setup() for this pcof (reused between vectors)."""
    if pre is None:
        pre = setup(prob, Gp, Gq, offsets, pcof, target, order)
    ref, m, dt, nt, Gb, Z, e = pre["ref"], pre["m"], pre["dt"], pre["nt"], pre["Gb"], pre["Z"], pre["e"]
    N, c, S = prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps
    P, Linv, Ac, psi = ref["P"], ref["Linv"], ref["Ac"], ref["psi"]
    NB = Gb.shape[0]
    v = np.asarray(v, float)
    gv = np.einsum("bnl,l->nb", Gb, v)
    # one forced sweep with the direction gv
    sv = np.zeros((nt, N, c), complex)
    for n in range(S):
        r = np.zeros((N, c), complex)
        for b in range(NB):
            r += gv[n, b] * pre["rR"][b][n] - gv[n + 1, b] * pre["rL"][b][n + 1]
        sv[n + 1] = P[n] @ sv[n] + Linv[n + 1] @ r
    # (A)
    brk = np.einsum("nic,bnic->nb", np.conj(sv), Z).real + np.einsum("nbc,nc->nb", e, gv)
    partA = -np.einsum("bnk,nb->k", Gb, brk)
    # forcing of the second-order adjoint: F = -f
    W = prob.guard_subspace_projector
    trap = np.ones(nt); trap[0] = trap[-1] = 0.5
    sr = np.concatenate([sv.real, sv.imag], axis=1)
    Ws = np.einsum("ij,njc->nic", W, sr)
    Wc = Ws[:, :N] + 1j * Ws[:, N:]
    F = np.einsum("nb,bnic->nic", gv, Z) - (2 * dt / prob.tf) * trap[:, None, None] * Wc
    T = np.asarray(target)
    ov = np.sum(np.conj(T) * sv[-1])
    F[-1] += (2 / prob.N_ess_levels ** 2) * ov * T
    y = np.zeros((nt, N, c), complex)
    y[-1] = F[-1]
    for n in range(S - 1, 0, -1):
        y[n] = P[n].conj().T @ y[n + 1] + F[n]
    mu = np.zeros_like(y)
    mu[1:] = np.conj(np.transpose(Linv[1:], (0, 2, 1))) @ y[1:]
    partB = pp.gradient_from(prob, Gp, Gq, offsets, pcof, Ac, psi, mu, m, dt)["grad"]
    hv = partA + partB
    if terms:
        return hv, dict(A=partA, B=partB, sv=sv, F=F, mu=mu, gv=gv, brk=brk)
    return hv
