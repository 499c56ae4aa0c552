"""Full-size cnot3 (550 steps, order 8, 180 parameters) on one handle, in one run: ms per dense pushforward
(qgd_eval_dense_pushforward, refine = 8: 4401 slots) of the level populations contracted with a 4-row level map (a small output:
what is timed is the scan, the tangent of the stage derivatives and the interpolation, not the download) -- (a) a cold call (new
pcof: forward sweep + one direction), (b) a warm call with one direction (history_precomputed), (c) a warm call with 16
directions, (d) a warm call with 180 directions, the full Jacobian -- beside (e) the only route there was before: two
eval_dense_populations calls per direction (central differences), and (f) eval_pushforward at the grid points with the same
directions (one, 16, 180).  The phases of (b), (c) and (d) from qgd_get_timings; duality with eval_dense_pullback as the check
that the timed calls compute J v.  The protocol of scripts/pushforward_timing.py: host clock around calls that end in a device
synchronise, the calls timed in alternation, R rounds of K calls each, median over the rounds with the extremes.
QGD_PUSHFORWARD_CHUNK (read when the handle is made) sets how many directions ride along in one scan."""
import sys, os, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..")); sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
from __graft_entry__ import import_package
qgd = import_package()
import cases
REFINE = 8
prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=550, tf=550.0)
dp = qgd.DeviceProblem(prob, 8); dp.set_controls(ctrl); dp.set_target(target)
n, N, c, slots = len(pcof), prob.N_tot_levels, prob.N_initial_conditions, 1 + prob.nsteps * REFINE
rng = np.random.default_rng(0)
V = rng.standard_normal((n, 16)); V /= np.linalg.norm(V, axis=0)
I = np.eye(n)
lm = rng.standard_normal((4, N))
ybar = rng.standard_normal((4, slots, c))
jv = dp.eval_dense_pushforward(REFINE, pcof, I, level_map=lm)["populations"]
g = dp.eval_dense_pullback(REFINE, pcof, populations_bar=ybar, level_map=lm)
print(f"n_pcof {n}, refine {REFINE}, chunk {os.environ.get('QGD_PUSHFORWARD_CHUNK', 'default')}: max|<ybar, J e_l> - (J^T ybar)_l| = "
      f"{np.abs(np.einsum('gkc,gkcl->l', ybar, jv) - g).max():.2e} (max|J^T ybar| = {np.abs(g).max():.2e})")
del jv
K, R = 5, 7


def clock(fn, k=K):
    t0 = time.perf_counter()
    for i in range(k): fn(i)
    return (time.perf_counter() - t0) / k * 1e3


shift = [pcof * (1 + 1e-6 * (i + 1)) for i in range(K)]      # new coefficients for every cold call
push = lambda p, v, **kw: dp.eval_dense_pushforward(REFINE, p, v, level_map=lm, **kw)
grid = lambda v: dp.eval_pushforward(pcof, v, level_map=lm, history_precomputed=True)
cold, one, sixteen, full, fd, g1, g16, g180 = [], [], [], [], [], [], [], []
for r in range(R):
    cold.append(clock(lambda i: push(shift[i], V[:, r % 16])))
    push(pcof, V[:, 0])
    one.append(clock(lambda i: push(pcof, V[:, (r + i) % 16], history_precomputed=True)))
    sixteen.append(clock(lambda i: push(pcof, V, history_precomputed=True)))
    full.append(clock(lambda i: push(pcof, I, history_precomputed=True), 2))
    g1.append(clock(lambda i: grid(V[:, (r + i) % 16])))
    g16.append(clock(lambda i: grid(V)))
    g180.append(clock(lambda i: grid(I), 2))
    fd.append(clock(lambda i: (dp.eval_dense_populations(REFINE, pcof + 1e-4 * V[:, i], level_map=lm),
                               dp.eval_dense_populations(REFINE, pcof - 1e-4 * V[:, i], level_map=lm))))
    push(pcof, V[:, 0])
for name, t in (("(a) cold call, one direction", cold), ("(b) warm call, one direction", one), ("(c) warm call, 16 directions", sixteen),
                ("(d) warm call, 180 directions", full),
                ("(e) two eval_dense_populations calls (one direction by differences)", fd),
                ("(f) eval_pushforward at the grid points, one direction", g1), ("(f) 16 directions", g16), ("(f) 180 directions", g180)):
    print(f"{name}: median {np.median(t):.3f} ms  (min {min(t):.3f}, max {max(t):.3f}; {R} rounds)")
print(f"per direction: (b) {np.median(one):.4f} ms, (c) {np.median(sixteen) / 16:.4f} ms, (d) {np.median(full) / n:.4f} ms; "
      f"(e) {np.median(fd):.4f} ms: (e) / (b) = {np.median(fd) / np.median(one):.2f}, (e) / (d) per direction = {np.median(fd) * n / np.median(full):.2f}")
for label, v in (("(b)", V[:, 1]), ("(c)", V), ("(d)", I)):
    dp.set_timing(1)
    push(pcof, v, history_precomputed=True)
    print(f"phases of {label} (ms):", {k: round(t, 3) for k, t in dp.timings().items()})
dp.set_timing(0)
dp.close()
