"""Full-size cnot3 (550 steps, order 8, 180 parameters) on one handle, in one run: ms per Hessian-vector product
(qgd_eval_hessian_vec) (a) at a new pcof (setup + product) and (b) at the same pcof (product only), beside (c) the exact Hessian
and (d) the forced gradient; the phases of (a) and (b) from qgd_get_timings, and the product against eval_hessian(pcof) @ v.
Host clock around calls that end in a device synchronise; the four are timed in alternation, R rounds of K calls each, and the
median over the rounds is reported with the extremes."""
import sys, os, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..")); sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
from __graft_entry__ import import_package
qgd = import_package()
import cases
prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=550, tf=550.0)
dp = qgd.DeviceProblem(prob, 8); dp.set_controls(ctrl); dp.set_target(target)
n = len(pcof)
rng = np.random.default_rng(0)
V = rng.standard_normal((n, 8)); V /= np.linalg.norm(V, axis=0)
H = dp.eval_hessian(pcof)
HV = dp.eval_hessian_vec(pcof, V)
print(f"n_pcof {n}: max|hv - H v| = {np.abs(HV - H @ V).max():.2e} (max|H| = {np.abs(H).max():.2e}, |v|_2 = 1)")
dp.eval_grad_forced(pcof)
K, R = 5, 7


def clock(fn):
    t0 = time.perf_counter()
    for i in range(K): fn(i)
    return (time.perf_counter() - t0) / K * 1e3


shift = [pcof * (1 + 1e-6 * (i + 1)) for i in range(K)]      # new coefficients for every cold call
cold, warm, hess, forced = [], [], [], []
for r in range(R):
    cold.append(clock(lambda i: dp.eval_hessian_vec(shift[i], V[:, r % 8])))
    dp.eval_hessian_vec(pcof, V[:, 0])
    warm.append(clock(lambda i: dp.eval_hessian_vec(pcof, V[:, (r + i) % 8])))
    hess.append(clock(lambda i: dp.eval_hessian(pcof)))
    forced.append(clock(lambda i: dp.eval_grad_forced(pcof)))
for name, t in (("(a) first product at a new pcof", cold), ("(b) further product, same pcof", warm), ("(c) eval_hessian", hess), ("(d) eval_grad_forced", forced)):
    print(f"{name}: median {np.median(t):.3f} ms  (min {min(t):.3f}, max {max(t):.3f}; {R} rounds of {K} calls)")
dp.set_timing(1)
dp.eval_hessian_vec(shift[0], V[:, 1])
print("phases of (a) (ms):", {k: round(v, 3) for k, v in dp.timings().items()})
dp.set_timing(1)
dp.eval_hessian_vec(shift[0], V[:, 2])
print("phases of (b) (ms):", {k: round(v, 3) for k, v in dp.timings().items()})
dp.close()
