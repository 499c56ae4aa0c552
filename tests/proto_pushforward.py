"""numpy statement of the pushforward of directions in pcof to the trajectory outputs (qgd_eval_pushforward, DESIGN.md section
4l), in the notation of proto_hvp.py / proto_pullback.py.  Test infrastructure only: csrc/qgd_k_pushforward.hip and the forced
scan behind it are compared with it.

s_v = sum_l v_l d psi / d pcof_l at every time point is the forced sweep of proto_hvp.hessian_vec, taken from there as it
stands (its `sv`): s_v(0) = 0, s_v(n+1) = P_n s_v(n) + L_{n+1}^-1 sum_b (gv[n][b] rhoR_b(n) - gv[n+1][b] rhoL_b(n+1)).  With
psi = u + iv and dpsi = s_v = du + i dv, slot k holding time point n = k * save_every, the three tangents are

    Sdot[:, k, col] = [du; dv]                                   [2N, n_slots, c]
    Pdot[g, k, col] = sum_l M[g, l] 2 (u_l du_l + v_l dv_l)      [n_groups or N, n_slots, c]   (M = I without a map)
    Edot[j, k, col] = 2 Re(psi^H H_j dpsi),  H_j = (O_j + O_j^H) / 2        [n_obs, n_slots, c]

the derivatives of proto_pullback.outputs along v; slot 0 is zero."""
import numpy as np

import proto_hvp as hvp
from proto_pullback import _observables


def setup(prob, Gp, Gq, offsets, pcof, target, order):
    """What does not depend on v (proto_hvp.setup: the forward evaluation and the basis responses; the target only enters parts
    of it that the forced sweep does not read)."""
    return hvp.setup(prob, Gp, Gq, offsets, pcof, target, order)


def state_tangent(prob, Gp, Gq, offsets, pcof, target, order, v, pre=None):
    """s_v [nt, N, c] complex, by the forced sweep of proto_hvp.hessian_vec."""
    return hvp.hessian_vec(prob, Gp, Gq, offsets, pcof, target, order, v, pre=pre, terms=True)[1]["sv"]


def tangents(psi, dpsi, save_every=1, level_map=None, observables=None):
    """(Sdot, Pdot, Edot) of a trajectory psi and its tangent dpsi, both [nt, N, c], in the layouts of proto_pullback.outputs;
    Edot is None without observables."""
    N = psi.shape[1]
    ps, ds = psi[::save_every], dpsi[::save_every]
    S = np.concatenate([ds.real, ds.imag], axis=1).transpose(1, 0, 2)
    pop = (2.0 * (ps.real * ds.real + ps.imag * ds.imag)).transpose(1, 0, 2)
    P = pop if level_map is None else np.einsum("gl,lkc->gkc", np.asarray(level_map, float), pop)
    E = None
    if observables is not None:
        O = _observables(observables, N)
        H = 0.5 * (O + np.conj(np.transpose(O, (0, 2, 1))))
        E = 2.0 * np.einsum("kic,jil,klc->jkc", np.conj(ps), H, ds).real
    return S, P, E


def pushforward(prob, Gp, Gq, offsets, pcof, target, order, v, save_every=1, level_map=None, observables=None, pre=None):
    """(Sdot, Pdot, Edot) along one direction v [n_pcof]."""
    if pre is None:
        pre = setup(prob, Gp, Gq, offsets, pcof, target, order)
    dpsi = state_tangent(prob, Gp, Gq, offsets, pcof, target, order, v, pre=pre)
    return tangents(pre["ref"]["psi"], dpsi, save_every, level_map, observables)
