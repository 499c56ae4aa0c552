"""What the Hermite dense output costs: cnot3 (N = 64, 8 columns, order 8, 550 steps) on one handle, one GPU, refine = 8.

  (a) eval_states                                        (the grid points alone: the yardstick)
  (b) eval_dense_states(refine)                          (forward sweep + stage derivatives + k_interp + 8 times the download)
  (c) the same with history_precomputed                  (the stored sweep reused)
  (d) eval_states at nsteps * refine                     (what the dense output replaces: the sweep on the refined grid;
                                                          --fine-only measures this route alone, e.g. on another checkout)

No gate on the numbers.  Every call ends with a stream synchronisation, so a host clock around `reps` calls is the call time.
The routes alternate inside a round; the table gives the median over the rounds and their min .. max.  The device time of the
interpolation kernel is the `dense_output` phase of qgd_get_timings; its bytes are 2 (m+1) panels read (the right end of a step
is the left end of the next: (m+1) from HBM) and refine written per step.

    python scripts/dense_output_timing.py [--rounds 7] [--reps 30] [--refine 8] [--fine-only] [--json out.json]
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--refine", type=int, default=8)
    ap.add_argument("--nsteps", type=int, default=550)
    ap.add_argument("--fine-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    qgd = import_package()
    order, r = 8, a.refine
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=a.nsteps, tf=float(a.nsteps))
    fprob, fctrl, _, _ = cases.cnot3_case(qgd, nsteps=a.nsteps * r, tf=float(a.nsteps))
    fine = qgd.DeviceProblem(fprob, order)
    fine.set_controls(fctrl); fine.set_target(target)
    routes = {"d_eval_states_refined_grid": lambda: fine.eval_states(pcof)}
    if not a.fine_only:
        dp = qgd.DeviceProblem(prob, order)
        dp.set_controls(ctrl); dp.set_target(target)
        routes = {"a_eval_states": lambda: dp.eval_states(pcof),
                  "b_eval_dense_states": lambda: dp.eval_dense_states(r, pcof),
                  "c_eval_dense_states_history_precomputed": lambda: dp.eval_dense_states(r, pcof, history_precomputed=True),
                  **routes}
    for f in routes.values():                      # warm-up: code objects, buffers
        for _ in range(5):
            f()
    per = {k: [] for k in routes}
    for _ in range(a.rounds):
        for k, f in routes.items():
            t0 = time.perf_counter()
            for _ in range(a.reps):
                f()
            per[k].append((time.perf_counter() - t0) / a.reps * 1e3)
    res = {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in per.items()}
    out = dict(routes=res, nsteps=a.nsteps, refine=r, order=order)
    print(f"cnot3, {a.nsteps} steps, order {order}, refine {r}; {a.rounds} rounds of {a.reps} calls per route (ms per call)")
    for k in sorted(res):
        v = res[k]
        print(f"  {k:42s} median {v['median_ms']:.4f}   min {v['min_ms']:.4f}   max {v['max_ms']:.4f}")
    if not a.fine_only:
        d = routes["b_eval_dense_states"]()
        err = np.abs(d - routes["d_eval_states_refined_grid"]()).max(axis=(0, 2))
        out["against_refined_grid"] = dict(grid=float(err[::r].max()), interior=float(np.delete(err, np.s_[::r]).max()))
        print(f"  dense output against the refined grid's states: max |diff| at grid slots {out['against_refined_grid']['grid']:.3e}, "
              f"between them {out['against_refined_grid']['interior']:.3e}")
        phases = {}
        for key, hp in (("b", False), ("c", True)):      # (a fresh handle each: qgd_get_timings keeps earlier phases)
            d2 = qgd.DeviceProblem(prob, order); d2.set_controls(ctrl); d2.set_target(target)
            d2.eval_dense_states(r, pcof)
            d2.set_timing(1)
            d2.eval_dense_states(r, pcof, history_precomputed=hp)
            phases[key] = {n: round(float(ms), 4) for n, ms in sorted(d2.timings().items(), key=lambda kv: -kv[1])}
            d2.close()
        m, hstep = order // 2, ((dp.N + 15) // 16 * 16) * 2 * ((dp.c + 7) // 8 * 8) * 8      # bytes of one panel [Np][2cp]
        moved = a.nsteps * ((m + 1) + r) * hstep + (m + 1 + 1) * hstep      # HBM bytes: every input panel once, every output panel once
        t = phases["c"].get("dense_output", float("nan"))
        out.update(phases=phases, bytes_moved=moved, gbytes_per_s=moved / (t * 1e-3) / 1e9)
        print(f"  phases of (b) (device ms, event bracketing on): {phases['b']}")
        print(f"  phases of (c): {phases['c']}")
        print(f"  k_interp: {moved / 1e6:.2f} MB in {t:.4f} ms = {out['gbytes_per_s']:.0f} GB/s")
        dp.close()
    fine.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
