"""A Rabi pi-pulse that tolerates detuning: optimize_gate over an ensemble of five detuned copies of the two-level problem,
the detunings at the Gauss-Legendre nodes of [-0.3, 0.3] with their weights (a quadrature of the mean infidelity over a
uniformly distributed detuning).  Printed: what the nominal-only optimum and the ensemble optimum score at every member."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (first: one HIP runtime for the process)
from __graft_entry__ import import_package

qgd = import_package()
prob = qgd.construct_rabi_prob(tf=np.pi, nsteps=100)
controls = qgd.FortranBSplineControl(2, 6, prob.tf)
target = np.array([[0.0, 1.0], [1.0, 0.0]])
n = qgd.get_number_of_control_parameters(controls)
pcof0 = np.concatenate([np.full(n // 2, 0.45), np.full(n - n // 2, 0.05)])

x, w = np.polynomial.legendre.leggauss(5)
deltas = 0.3 * x
ens = qgd.Ensemble(np.stack([np.diag([0.0, d]) for d in deltas]), np.zeros((5, 2, 2)), None, w / 2.0)

kw = dict(order=8, ridge_penalty_strength=0, maxIter=60, print_level=0, pcof_L=-1.5, pcof_U=1.5)
nominal = qgd.optimize_gate(prob, controls, pcof0, target, **kw)
robust = qgd.optimize_gate(prob, controls, pcof0, target, ensemble=ens, **kw)


def member_infidelities(pcof):
    res = qgd.eval_ensemble(prob, controls, pcof, target, ens, order=8, gradient=False)
    a, b = res.member_out3[:, 0], res.member_out3[:, 1]
    return 1.0 - (a * a + b * b) / prob.N_ess_levels ** 2, res.cost


nom, nom_mean = member_infidelities(nominal.pcof[-1])
rob, rob_mean = member_infidelities(robust.pcof[-1])
print("detuning    nominal-only optimum    ensemble optimum")
for d, a, b in zip(deltas, nom, rob):
    print(f"{d:+.4f}      {a:.3e}               {b:.3e}")
print(f"mean        {nom_mean:.3e}               {rob_mean:.3e}")
print(f"outer members: {nom[0]:.3e}, {nom[-1]:.3e} (nominal only)  ->  {rob[0]:.3e}, {rob[-1]:.3e} (ensemble)")
