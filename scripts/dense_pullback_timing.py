"""What a pullback of the dense output costs: cnot3 (N = 64, 8 columns, order 8, 550 steps) on one handle, one GPU, refine = 8
(4401 dense points), with an expectations cotangent on the three control operators a_k + a_k^dagger and the drift Hamiltonian
H_d (all real symmetric, the observables of scripts/pullback_timing.py).

  (a) eval_pullback at the grid points                   (551 slots: the yardstick)
  (b) eval_dense_pullback(8)                             (forward sweep on the general path + interpolation + forcing kernel on the
                                                          dense panels + the two kernels of qgd_k_dense_pullback.hip + adjoint sweep)
  (c) the same with history_precomputed                  (the stored sweep reused)

No gate on the numbers: nothing exists to compare a new call with.  Every call ends with a stream synchronisation, so a host
clock around `reps` calls is the call time.  The routes alternate inside a round; the table gives the median over the rounds and
their min .. max.  Also printed: the per-phase device times of (b) and (c) (event bracketing on), and the bytes the two new kernels
move by their algorithm (computed from the shapes) against those times.

    python scripts/dense_pullback_timing.py [--rounds 7] [--reps 50] [--refine 8] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401  (its HIP runtime first, as in tests/conftest.py)
from __graft_entry__ import import_package
import cases


def kernel_bytes(Np, cp, nt, m, refine, n_ops):
    """Bytes the two kernels move by their algorithm (every panel once; the operator planes and tables stay in cache)."""
    panel = Np * 2 * cp * 8
    pts = 1 + (nt - 1) * refine
    transpose = (pts + (nt - 2) * (refine - 1)) * panel + nt * (m + 1) * panel      # G: interior slots once per end; gbar written
    sweep = nt * (m + (m + 1) + 1) * panel + (cp // 8) * nt * n_ops * m * 2 * 8      # w_0..w_{m-1}, gbar read; F, sigma written
    return dict(transpose=transpose, sweep=sweep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--refine", type=int, default=8)
    ap.add_argument("--nsteps", type=int, default=550)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    qgd = import_package()
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=a.nsteps, tf=float(a.nsteps))
    order, r = 8, a.refine
    dp = qgd.DeviceProblem(prob, order)
    dp.set_controls(ctrl); dp.set_target(target)
    nt, c = dp.nsteps + 1, dp.c
    obs = np.stack([np.asarray(o, dtype=float) for o in prob.sym_operators] + [np.asarray(prob.system_sym, dtype=float)])
    rng = np.random.default_rng(0)
    eb = np.asfortranarray(rng.standard_normal((len(obs), nt, c)))
    ebd = np.asfortranarray(rng.standard_normal((len(obs), 1 + dp.nsteps * r, c)))
    routes = {"a_pullback_grid_points": lambda: dp.eval_pullback(pcof, expectations_bar=eb, observables=obs),
              "b_dense_pullback": lambda: dp.eval_dense_pullback(r, pcof, expectations_bar=ebd, observables=obs),
              "c_dense_pullback_history_precomputed": lambda: dp.eval_dense_pullback(r, pcof, expectations_bar=ebd, observables=obs,
                                                                                     history_precomputed=True)}
    for f in routes.values():                      # warm-up: code objects, buffers
        for _ in range(10):
            f()
    g = routes["b_dense_pullback"]()
    same = bool(np.array_equal(g, routes["c_dense_pullback_history_precomputed"]()))
    per = {k: [] for k in routes}
    for _ in range(a.rounds):
        for k, f in routes.items():
            if k.startswith("c_"):
                routes["b_dense_pullback"]()       # (the general path's sweep of this pcof in the buffers)
            t0 = time.perf_counter()
            for _ in range(a.reps):
                f()
            per[k].append((time.perf_counter() - t0) / a.reps * 1e3)
    res = {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in per.items()}
    phases = {}
    for key, hp in (("b", False), ("c", True)):      # (a fresh handle each: qgd_get_timings keeps earlier phases)
        d2 = qgd.DeviceProblem(prob, order); d2.set_controls(ctrl); d2.set_target(target)
        for _ in range(3):
            d2.eval_dense_pullback(r, pcof, expectations_bar=ebd, observables=obs)
        d2.set_timing(1)
        d2.eval_dense_pullback(r, pcof, expectations_bar=ebd, observables=obs, history_precomputed=hp)
        phases[key] = {n: round(float(ms), 4) for n, ms in sorted(d2.timings().items(), key=lambda kv: -kv[1])}
        d2.close()
    Np, cp = 16 * ((dp.N + 15) // 16), 8 * ((c + 7) // 8)
    nbytes = kernel_bytes(Np, cp, nt, order // 2, r, prob.N_operators)
    rates = {k: dict(bytes=nbytes[k], ms=phases["c"].get("dense_pullback_" + k),
                     GB_per_s=(round(nbytes[k] / (phases["c"]["dense_pullback_" + k] * 1e-3) / 1e9, 1)
                               if phases["c"].get("dense_pullback_" + k) else None)) for k in nbytes}
    print(f"cnot3, {dp.nsteps} steps, order {order}, refine {r}, {len(obs)} real observables; {a.rounds} rounds of {a.reps} calls per route (ms per call)")
    for k in sorted(res):
        v = res[k]
        print(f"  {k:38s} median {v['median_ms']:.4f}   min {v['min_ms']:.4f}   max {v['max_ms']:.4f}")
    print(f"  (b) and (c) return the same bits: {same}")
    print(f"  phases of (b) (device ms, event bracketing on): {phases['b']}")
    print(f"  phases of (c): {phases['c']}")
    print(f"  the two new kernels, bytes by the algorithm against the phase time of (c): {rates}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(routes=res, phases=phases, same_bits=same, kernel_bytes=rates), f, indent=1)
    dp.close()


if __name__ == "__main__":
    main()
