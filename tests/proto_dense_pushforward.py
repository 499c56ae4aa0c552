"""numpy statement of the pushforward of directions in pcof to the DENSE trajectory outputs (qgd_eval_dense_pushforward, DESIGN.md
section 4n), on top of proto_pushforward.py and proto_dense_pullback.py, in their notation.  Test infrastructure only:
csrc/qgd_k_dense_pushforward.hip and the host path around it are compared with it.

Per time point n, with Ac[n, d] from the tables, w_0 = psi_n and the stage derivatives w_j of proto_dense_pullback, and for a
direction v in pcof:

    dw_0(n) = s_v(n)                                                       (the forced sweep of proto_pushforward; s_v(0) = 0)
    dAc[n, d] = sum_o (dq_o^(d) Asym_o - i dp_o^(d) Sym_o)                 (the tables are linear in pcof: the tables of v, no system term)
    dw_j(n) = (1/j) sum_{i<j} [ Ac[n, j-1-i] dw_i(n) + dAc[n, j-1-i] w_i(n) ],  j = 1..m
    dd[n r + s] = sum_j a[s-1, j] dw_j(n) + b[s-1, j] dw_j(n+1),  s = 1..r-1;   dd[n r] = dw_0(n)   (the weights of the dense output)
    Sdot = dd;  Pdot = 2 (u du + v dv);  Edot = 2 Re(d^H H_j dd)                                  (proto_pushforward.tangents on d, dd)

d is the dense state of proto_dense_pullback.dense_trajectory.  The dAc w term is the forward-mode counterpart of the explicit
part of proto_dense_pullback (its step 4): without it the result is wrong by percents."""
import numpy as np

import proto_dense_pullback as pdp
import proto_propagator as pp
import proto_pullback as pb
import proto_pushforward as pf


def operator_tangent(prob, Gp, Gq, offsets, v, m):
    """dAc [nt, m, N, N]: the assembled operators of the tables of v, less the system term"""
    v = np.asarray(v, float)
    return pp.assemble(prob, *pp.tables(Gp, Gq, offsets, v, m), m) - pp.assemble(prob, *pp.tables(Gp, Gq, offsets, np.zeros_like(v), m), m)


def stage_derivative_tangents(Ac, dAc, ws, sv, m, explicit=True):
    """[dw_0 .. dw_m], each [nt, N, c]; per target one sum, i ascending, the Ac dw_i term before the dAc w_i term"""
    dws = [sv]
    for j in range(m):
        acc = np.zeros_like(sv)
        for i in range(j + 1):
            acc = acc + Ac[:, j - i] @ dws[i]
            if explicit:
                acc = acc + dAc[:, j - i] @ ws[i]
        dws.append(acc / (j + 1))
    return dws


def setup(prob, Gp, Gq, offsets, pcof, target, order):
    """What does not depend on v or refine: proto_pushforward.setup and the forward sweep of proto_pullback (the same psi)."""
    return dict(pre=pf.setup(prob, Gp, Gq, offsets, pcof, target, order), fwd=pb.forward(prob, Gp, Gq, offsets, pcof, order))


def dense_pushforward(qgd, prob, Gp, Gq, offsets, pcof, target, order, refine, v, level_map=None, observables=None, pre=None,
                      explicit=True, terms=False):
    """(Sdot, Pdot, Edot) of the dense output along one direction v [n_pcof], slots 1 + nsteps refine, in the layouts of
    proto_pushforward.tangents.  explicit=False drops the dAc w term (to show what it is worth)."""
    if pre is None:
        pre = setup(prob, Gp, Gq, offsets, pcof, target, order)
    fwd = pre["fwd"]
    m = fwd["m"]
    sv = pf.state_tangent(prob, Gp, Gq, offsets, pcof, target, order, v, pre=pre["pre"])
    d, ws, a, b = pdp.dense_trajectory(qgd, fwd, refine)
    dAc = operator_tangent(prob, Gp, Gq, offsets, v, m)
    dws = stage_derivative_tangents(fwd["Ac"], dAc, ws, sv, m, explicit)
    dd = pdp.interpolate(dws, a, b, refine)
    out = pf.tangents(d, dd, 1, level_map, observables)
    if terms:
        return out, dict(d=d, dd=dd, dws=dws, dAc=dAc, sv=sv)
    return out
