"""numpy statement of the pullback of the DENSE trajectory outputs to pcof (qgd_eval_dense_pullback), on
top of proto_pullback.py.  Test infrastructure only: csrc/qgd_k_dense_pullback.hip is compared with it.

Per time point n, with Ac[n, d] from the tables and w_0 = psi_n (complex form):

    w_j(n) = (1/j) sum_{i<j} Ac[n, j-1-i] w_i(n),  j = 1..m                                     (k_derivs)
    d[n r + s] = sum_j a[s-1, j] w_j(n) + b[s-1, j] w_j(n+1),  s = 1..r-1;   d[n r] = w_0(n)     (k_interp)

The cost is J = <Sbar, S(d)> + <Pbar, P(d)> + <Ebar, E(d)> with the outputs of the interpolated state as eval_dense returns
them.  Its gradient:

    1  G[slot] = cotangent_forcing(d, save_every = 1, ...): dJ/dd, G[0] = 0
    2  transposed interpolation: g_0(n) = G[n r]; g_j(n) += a[s-1, j] G[n r + s], g_j(n+1) += b[s-1, j] G[n r + s]
    3  reverse recursion at every n: j = m..1, i = 0..j-1: g_i += (1/j) Ac[n, j-1-i]^H g_j   (the row i = 0 included)
    4  explicit part -- the stage derivatives depend on pcof through the tables at their own time point:
         sigP[n, k, d] = sum_{j=1..m} sum_{i<j, d=j-1-i} (1/j) Re<-i S_k w_i, g_j>,  sigQ with A_k w_i   (g_j after step 3)
         grad_explicit[off_k + l] = + sum_{n,d} Gp[n, d, l] sigP[n, k, d] + Gq[n, d, l] sigQ[n, k, d]
       (dw_j = (1/j) sum_i (dAc[j-1-i] w_i + Ac[j-1-i] dw_i): the second term is what step 3 transposes, the first term
        contracted with g_j is sigP / sigQ times the basis -- a plain chain rule, so the sign is plus)
    5  implicit part: g_0(n) after step 3 is dJ/dw_0(n), a states cotangent of the grid-point pullback: F = -g_0, F[0]
       dropped, then the adjoint recursion and the first-order contraction of proto_pullback.pullback
    6  grad = grad_implicit + grad_explicit"""
import numpy as np

import proto_propagator as pp
import proto_pullback as pb


def stage_derivatives(Ac, psi, m):
    """[w_0 .. w_m], each [nt, N, c]"""
    ws = [psi]
    for j in range(m):
        acc = np.zeros_like(psi)
        for i in range(j + 1):
            acc += Ac[:, j - i] @ ws[i]
        ws.append(acc / (j + 1))
    return ws


def interpolate(ws, a, b, refine):
    """d [1 + (nt-1) refine, N, c] from the stage derivatives, summed as k_interp does (ascending j, left end before right)"""
    nt = ws[0].shape[0]
    d = np.zeros((1 + (nt - 1) * refine,) + ws[0].shape[1:], dtype=complex)
    d[::refine] = ws[0]
    for s in range(1, refine):
        acc = np.zeros((nt - 1,) + ws[0].shape[1:], dtype=complex)
        for j in range(len(ws)):
            acc = acc + a[s - 1, j] * ws[j][:-1]
            acc = acc + b[s - 1, j] * ws[j][1:]
        d[s::refine] = acc
    return d


def dense_trajectory(qgd, fwd, refine):
    m = fwd["m"]
    a, b = qgd.hermite_dense_weights(m, refine, fwd["dt"]) if refine > 1 else (np.zeros((0, m + 1)),) * 2
    ws = stage_derivatives(fwd["Ac"], fwd["psi"], m)
    return interpolate(ws, a, b, refine), ws, a, b


def dense_outputs(qgd, prob, Gp, Gq, offsets, pcof, order, refine, level_map=None, observables=None):
    """(S, P, E) of the dense output, the layouts of eval_dense_states / _populations / _expectations"""
    fwd = pb.forward(prob, Gp, Gq, offsets, pcof, order)
    d = dense_trajectory(qgd, fwd, refine)[0]
    return pb.outputs(d, 1, level_map, observables)


def dense_pullback(qgd, prob, Gp, Gq, offsets, pcof, order, refine, states_bar=None, pop_bar=None, level_map=None,
                   expect_bar=None, observables=None, fwd=None, terms=False):
    """grad [n_pcof] = sum over the parts given of <bar, d dense output / d pcof>; cotangents [rows, 1 + nsteps refine, c]"""
    if fwd is None:
        fwd = pb.forward(prob, Gp, Gq, offsets, pcof, order)
    m, Ac, psi = fwd["m"], fwd["Ac"], fwd["psi"]
    nt = psi.shape[0]
    d, ws, a, b = dense_trajectory(qgd, fwd, refine)
    G = pb.cotangent_forcing(d, 1, states_bar, pop_bar, level_map, expect_bar, observables)              # step 1
    g = [np.zeros_like(psi) for _ in range(m + 1)]                                                       # step 2
    g[0] = G[::refine].copy()
    for s in range(1, refine):
        Gs = G[s::refine]                                                                                # [nt-1, N, c]
        for j in range(m + 1):
            g[j][:-1] += a[s - 1, j] * Gs
            g[j][1:] += b[s - 1, j] * Gs
    AcH = np.conj(np.transpose(Ac, (0, 1, 3, 2)))                                                        # step 3
    for j in range(m, 0, -1):
        for i in range(j):
            g[i] = g[i] + (1.0 / j) * (AcH[:, j - 1 - i] @ g[j])
    nops = prob.N_operators                                                                              # step 4
    sigP, sigQ = np.zeros((nt, nops, m)), np.zeros((nt, nops, m))
    for k in range(nops):
        Sk, Ak = prob.sym_operators[k], prob.asym_operators[k]
        for j in range(1, m + 1):
            for i in range(j):
                dd = j - 1 - i
                sigP[:, k, dd] += (1.0 / j) * np.einsum("nic,nic->n", np.conj(-1j * (Sk @ ws[i])), g[j]).real
                sigQ[:, k, dd] += (1.0 / j) * np.einsum("nic,nic->n", np.conj(Ak @ ws[i]), g[j]).real
    explicit = np.zeros(len(pcof))
    for k, (gp, gq, off) in enumerate(zip(Gp, Gq, offsets)):
        nl = gp.shape[2]
        explicit[off:off + nl] += np.einsum("ndl,nd->l", gp[:, :m], sigP[:, k]) + np.einsum("ndl,nd->l", gq[:, :m], sigQ[:, k])
    g0 = g[0]                                                                                            # step 5
    sb = np.concatenate([g0.real, g0.imag], axis=1).transpose(1, 0, 2)                                   # [2N, nt, c]
    implicit = pb.pullback(prob, Gp, Gq, offsets, pcof, order, save_every=1, states_bar=sb, fwd=fwd)
    grad = implicit + explicit                                                                           # step 6
    if terms:
        return grad, dict(G=G, g=g, sigP=sigP, sigQ=sigQ, explicit=explicit, implicit=implicit, d=d)
    return grad
