"""The numpy statement of cost_type :StateTransfer: the per-column infidelity of the final state,
its derivative with respect to the final state and the second-order terminal term.

Real layout as everywhere in the project: w = [u; v] is [2N, c] with u = Re psi, v = Im psi; R = [r; q] the target the
same way, T = [q; -r].  With a_j = <w_j, R_j>, b_j = <w_j, T_j> (o_j = t_j^H psi_j = a_j - i b_j, infidelity.jl:13-17 column
by column) and c columns:

    J       = 1 - (1/c) sum_j (a_j^2 + b_j^2)
    dJ/dw_j = -(2/c) (a_j R_j + b_j T_j)                       (the terminal condition is y_N = -dJ/dw_N + f_N)
    (d2J/dw2) s, column j = -(2/c) (<s_j, R_j> R_j + <s_j, T_j> T_j)
"""
import numpy as np


def real(x):
    """complex [N, c] -> real [2N, c]; a real array is taken as it is"""
    x = np.asarray(x)
    return np.vstack([x.real, x.imag]).astype(np.float64) if np.iscomplexobj(x) else x.astype(np.float64)


def partner(R):
    """T = [R_im; -R_re]"""
    N = R.shape[0] // 2
    return np.vstack([R[N:], -R[:N]])


def overlaps(w, target):
    """(a_j, b_j) of every column"""
    w, R = real(w), real(target)
    return np.sum(w * R, axis=0), np.sum(w * partner(R), axis=0)


def cost(w, target):
    a, b = overlaps(w, target)
    return 1.0 - np.sum(a * a + b * b) / len(a)


def cost_bar(w, target):
    """dJ/dw, [2N, c]"""
    R = real(target)
    a, b = overlaps(w, R)
    return -(2.0 / len(a)) * (a[None, :] * R + b[None, :] * partner(R))


def second_order(s, target):
    """(d2J/dw2) s, [2N, c]: linear in s, independent of w (J is quadratic in w).  The device's hvp_terminal is its negative,
    +(2/c)(<s_j,R_j> R_j + <s_j,T_j> T_j): the terminal part of the second-order adjoint's right-hand side."""
    R = real(target)
    sR, sT = overlaps(s, R)
    return -(2.0 / len(sR)) * (sR[None, :] * R + sT[None, :] * partner(R))
