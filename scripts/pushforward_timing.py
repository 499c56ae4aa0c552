"""Full-size cnot3 (550 steps, order 8, 180 parameters) on one handle, in one run: ms per pushforward (qgd_eval_pushforward) of
the level populations contracted with a 4-row level map (a small output: what is timed is the sweep and the scan, not the
download) -- (a) a cold call (new pcof: forward sweep + one direction), (b) a warm call with one direction
(history_precomputed), (c) a warm call with 16 directions, (d) a warm call with 180 directions, the full Jacobian -- beside
(e) what a user had before: two eval_populations calls per direction (central differences), and (f) eval_grad_forced, which
runs all 180 parameters through the same scan.  (d') is (d) with the plain populations [64, 551, 8, 180] (406 MB to the host).
The phases of (b) and (d) from qgd_get_timings; duality with eval_pullback as the check that the timed calls compute J v.
Host clock around calls that end in a device synchronise; the calls are timed in alternation, R rounds of K calls each, and the
median over the rounds is reported with the extremes.  QGD_PUSHFORWARD_CHUNK (read when the handle is made) sets how many
directions ride along in one scan."""
import sys, os, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..")); sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
from __graft_entry__ import import_package
qgd = import_package()
import cases
prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=550, tf=550.0)
dp = qgd.DeviceProblem(prob, 8); dp.set_controls(ctrl); dp.set_target(target)
n, N, c, nt = len(pcof), prob.N_tot_levels, prob.N_initial_conditions, prob.nsteps + 1
rng = np.random.default_rng(0)
V = rng.standard_normal((n, 16)); V /= np.linalg.norm(V, axis=0)
I = np.eye(n)
lm = rng.standard_normal((4, N))
ybar = rng.standard_normal((4, nt, c))
jv = dp.eval_pushforward(pcof, I, level_map=lm)["populations"]
g = dp.eval_pullback(pcof, populations_bar=ybar, level_map=lm)
print(f"n_pcof {n}, chunk {os.environ.get('QGD_PUSHFORWARD_CHUNK', 'default')}: max|<ybar, J e_l> - (J^T ybar)_l| = "
      f"{np.abs(np.einsum('gkc,gkcl->l', ybar, jv) - g).max():.2e} (max|J^T ybar| = {np.abs(g).max():.2e})")
dp.eval_grad_forced(pcof)
K, R = 5, 7


def clock(fn, k=K):
    t0 = time.perf_counter()
    for i in range(k): fn(i)
    return (time.perf_counter() - t0) / k * 1e3


shift = [pcof * (1 + 1e-6 * (i + 1)) for i in range(K)]      # new coefficients for every cold call
push = lambda p, v, **kw: dp.eval_pushforward(p, v, level_map=lm, **kw)
cold, one, sixteen, full, plain, fd, forced = [], [], [], [], [], [], []
for r in range(R):
    cold.append(clock(lambda i: push(shift[i], V[:, r % 16])))
    push(pcof, V[:, 0])
    one.append(clock(lambda i: push(pcof, V[:, (r + i) % 16], history_precomputed=True)))
    sixteen.append(clock(lambda i: push(pcof, V, history_precomputed=True)))
    full.append(clock(lambda i: push(pcof, I, history_precomputed=True)))
    plain.append(clock(lambda i: dp.eval_pushforward(pcof, I, populations=True, history_precomputed=True), 1))
    fd.append(clock(lambda i: (dp.eval_populations(pcof + 1e-4 * V[:, i], level_map=lm), dp.eval_populations(pcof - 1e-4 * V[:, i], level_map=lm))))
    forced.append(clock(lambda i: dp.eval_grad_forced(pcof)))
    push(pcof, V[:, 0])
for name, t in (("(a) cold call, one direction", cold), ("(b) warm call, one direction", one), ("(c) warm call, 16 directions", sixteen),
                ("(d) warm call, 180 directions", full), ("(d') the same, plain populations (406 MB out)", plain),
                ("(e) two eval_populations calls (one direction by differences)", fd), ("(f) eval_grad_forced", forced)):
    print(f"{name}: median {np.median(t):.3f} ms  (min {min(t):.3f}, max {max(t):.3f}; {R} rounds)")
print(f"(d) per direction: {np.median(full) / n:.4f} ms; (c) per direction: {np.median(sixteen) / 16:.4f} ms")
dp.set_timing(1)
push(pcof, V[:, 1], history_precomputed=True)
print("phases of (b) (ms):", {k: round(v, 3) for k, v in dp.timings().items()})
dp.set_timing(1)
push(pcof, I, history_precomputed=True)
print("phases of (d) (ms):", {k: round(v, 3) for k, v in dp.timings().items()})
dp.close()
