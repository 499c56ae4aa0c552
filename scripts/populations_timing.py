"""What the trajectory costs: cnot3 (N = 64, 8 columns, order 8, 550 steps) on one handle, one GPU.

  (a) eval_forward into a pinned full uv_history [128, 5, 551, 8]      (the only route before qgd_eval_states)
  (b) eval_states into a pinned [128, 551, 8]
  (c) eval_populations [64, 551, 8]
  (d) eval_populations with the (4,4,4) subsystem map [12, 551, 8]
  (e) the allocating eval_forward(prob, controls, pcof) of the functional API
  (f) eval_forward without outputs (the evaluation alone)

Every call ends with the library's own stream synchronisation, so a host clock around `reps` calls is the call time.  The
routes alternate inside a round; the table gives the median over the rounds and their min .. max.  A tree without
eval_states (an older checkout) times (a), (e) and (f) only: run this file from both trees in one session for (e).

    python scripts/populations_timing.py [--rounds 9] [--reps 200] [--json out.json]
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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    qgd = import_package()
    prob, ctrl, pcof, target = cases.cnot3_case(qgd, nsteps=550, tf=550.0)
    order = 8
    dp = qgd.device_problem(prob, order)          # (the handle the functional API uses too)
    dp.set_controls(ctrl); dp.set_target(target)
    N, nt, c = dp.N, dp.nsteps + 1, dp.c
    uv = dp.pin(np.zeros((2 * N, dp.m + 1, nt, c), order="F"))
    routes = {"a_uv_history_pinned": lambda: dp.eval_forward(pcof, uv),
              "e_eval_forward_allocating": lambda: qgd.eval_forward(prob, ctrl, pcof, order=order),
              "f_no_outputs": lambda: dp.eval_forward(pcof)}
    bytes_out = {"a_uv_history_pinned": uv.nbytes, "e_eval_forward_allocating": 2 * N * nt * c * 8, "f_no_outputs": 0}
    new = hasattr(dp, "eval_states")
    if new:
        st = dp.pin(np.zeros((2 * N, nt, c), order="F"))
        M = qgd.subsystem_population_map((4, 4, 4))
        pp = dp.pin(np.zeros((N, nt, c), order="F"))
        pg = dp.pin(np.zeros((M.shape[0], nt, c), order="F"))
        routes.update({"b_states_pinned": lambda: dp.eval_states(pcof, out=st),
                       "c_populations": lambda: dp.eval_populations(pcof, out=pp),
                       "d_populations_subsystems": lambda: dp.eval_populations(pcof, level_map=M, out=pg)})
        bytes_out.update({"b_states_pinned": st.nbytes, "c_populations": pp.nbytes, "d_populations_subsystems": pg.nbytes})
    for f in routes.values():                      # warm-up: code objects, staging buffers, pinned mappings
        for _ in range(20):
            f()
    assert dp.front_path_taken()
    per = {k: [] for k in routes}
    for _ in range(a.rounds):
        for k, f in routes.items():
            t0 = time.perf_counter()
            for _ in range(a.reps):
                f()
            per[k].append((time.perf_counter() - t0) / a.reps * 1e3)
    res = {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v), bytes=bytes_out[k]) for k, v in per.items()}
    phases = {}                                    # (a fresh handle each: qgd_get_timings keeps the phases of earlier calls)
    for k in ("a_uv_history_pinned", "c_populations"):
        if k in routes:
            d2 = qgd.DeviceProblem(prob, order); d2.set_controls(ctrl); d2.set_target(target)
            call = (lambda: d2.eval_forward(pcof, uv2)) if k[0] == "a" else (lambda: d2.eval_populations(pcof))
            uv2 = np.zeros(uv.shape, order="F")
            d2.set_timing(1)
            call(); call()
            phases[k] = {n: round(float(ms), 4) for n, ms in sorted(d2.timings().items(), key=lambda kv: -kv[1])}
            d2.close()
    print(f"cnot3, {dp.nsteps} steps, order {order}; {a.rounds} rounds of {a.reps} calls per route (ms per call)")
    for k in sorted(res):
        r = res[k]
        print(f"  {k:28s} median {r['median_ms']:.4f}   min {r['min_ms']:.4f}   max {r['max_ms']:.4f}   {r['bytes'] / 1e6:6.2f} MB out")
    for k, ph in phases.items():
        print(f"  phases of {k} (device ms, event bracketing on): {ph}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(routes=res, phases=phases, new_entry_points=new), f, indent=1)
    qgd.clear_cache()


if __name__ == "__main__":
    main()
