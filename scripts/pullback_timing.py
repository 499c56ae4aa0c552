"""What a pullback costs: cnot3 (N = 64, 8 columns, order 8, 550 steps) on one handle, one GPU, with an expectations cotangent
on the three control operators a_k + a_k^dagger and the drift Hamiltonian H_d (all real symmetric).

  (a) discrete_adjoint                                   (the library's own gradient: the yardstick)
  (b) eval_pullback with an expectations cotangent       (forward sweep on the general path + forcing kernel + adjoint sweep)
  (c) the same with history_precomputed                  (the stored sweep reused: forcing kernel + adjoint sweep + gradient)

No gate on the numbers.  The expectation: (b) = (a) + the forcing kernel (+ the stage derivatives (a) may not need, and the
upload of the cotangent).  Every call ends with a stream synchronisation, so a host clock around `reps` calls is the call
time.  The routes alternate inside a round; the table gives the median over the rounds and their min .. max.

    python scripts/pullback_timing.py [--rounds 9] [--reps 100] [--json out.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    qgd = import_package()
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=550, tf=550.0)
    order = 8
    dp = qgd.DeviceProblem(prob, order)
    dp.set_controls(ctrl); dp.set_target(target)
    nt, c = dp.nsteps + 1, dp.c
    obs = np.stack([np.asarray(o, dtype=float) for o in prob.sym_operators] + [np.asarray(prob.system_sym, dtype=float)])
    eb = np.asfortranarray(np.random.default_rng(0).standard_normal((len(obs), nt, c)))
    routes = {"a_discrete_adjoint": lambda: dp.discrete_adjoint(pcof)[0],
              "b_pullback_expectations": lambda: dp.eval_pullback(pcof, expectations_bar=eb, observables=obs),
              "c_pullback_history_precomputed": lambda: dp.eval_pullback(pcof, expectations_bar=eb, observables=obs, history_precomputed=True)}
    for f in routes.values():                      # warm-up: code objects, buffers
        for _ in range(10):
            f()
    g = routes["b_pullback_expectations"]()
    same = bool(np.array_equal(g, routes["c_pullback_history_precomputed"]()))
    per = {k: [] for k in routes}
    for _ in range(a.rounds):
        for k, f in routes.items():
            if k.startswith("c_"):
                routes["b_pullback_expectations"]()      # (the general path's sweep of this pcof in the buffers)
            t0 = time.perf_counter()
            for _ in range(a.reps):
                f()
            per[k].append((time.perf_counter() - t0) / a.reps * 1e3)
    res = {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in per.items()}
    phases = {}
    for key, hp in (("b", False), ("c", True)):      # (a fresh handle each: qgd_get_timings keeps earlier phases)
        d2 = qgd.DeviceProblem(prob, order); d2.set_controls(ctrl); d2.set_target(target)
        d2.eval_pullback(pcof, expectations_bar=eb, observables=obs)
        d2.set_timing(1)
        d2.eval_pullback(pcof, expectations_bar=eb, observables=obs, history_precomputed=hp)
        phases[key] = {n: round(float(ms), 4) for n, ms in sorted(d2.timings().items(), key=lambda kv: -kv[1])}
        d2.close()
    print(f"cnot3, {dp.nsteps} steps, order {order}, {len(obs)} real observables; {a.rounds} rounds of {a.reps} calls per route (ms per call)")
    for k in sorted(res):
        r = res[k]
        print(f"  {k:34s} median {r['median_ms']:.4f}   min {r['min_ms']:.4f}   max {r['max_ms']:.4f}")
    print(f"  (b) and (c) return the same bits: {same}")
    print(f"  phases of (b) (device ms, event bracketing on): {phases['b']}")
    print(f"  phases of (c): {phases['c']}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(routes=res, phases=phases, same_bits=same), f, indent=1)
    dp.close()


if __name__ == "__main__":
    main()
