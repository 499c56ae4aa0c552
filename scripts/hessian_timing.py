"""Full-size cnot3 (550 steps, order 8, 180 parameters): ms per exact Hessian (qgd_eval_hessian) and its phases from
qgd_get_timings, against eval_grad_forced on the same handle."""
import sys, os, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..")); sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
from __graft_entry__ import import_package
qgd = import_package()
import cases
prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=550, tf=550.0)
dp = qgd.DeviceProblem(prob, 8); dp.set_controls(ctrl); dp.set_target(target)
grad = np.zeros(len(pcof))
H = dp.eval_hessian(pcof, grad=grad)
g_for = dp.eval_grad_forced(pcof)
K = 5
t0 = time.time()
for _ in range(K): dp.eval_grad_forced(pcof)
t_for = (time.time() - t0) / K
t0 = time.time()
for _ in range(K): dp.eval_hessian(pcof)
t_hess = (time.time() - t0) / K
print(f"n_pcof {len(pcof)}: Hessian {t_hess * 1e3:.2f} ms, forced gradient {t_for * 1e3:.2f} ms per evaluation; "
      f"grad output vs forced gradient {np.abs(grad - g_for).max() / np.abs(g_for).max():.1e}, "
      f"asymmetry {np.abs(H - H.T).max() / np.abs(H).max():.1e}")
dp.set_timing(1)
dp.eval_hessian(pcof)
print("phases of one Hessian (ms):", {k: round(v, 3) for k, v in dp.timings().items()})
dp.close()
