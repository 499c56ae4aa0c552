"""What expectation values cost: cnot3 (N = 64, 8 columns, order 8, 550 steps) on one handle, one GPU, with the three control
operators a_k + a_k^dagger and the drift Hamiltonian H_d as observables (all real symmetric: <H(t)> follows from them by
linearity with the control values).

  (a) eval_states into a pinned [128, 551, 8] + the numpy contraction on the host      (the route without eval_expectations)
  (b) eval_expectations into a pinned [4, 551, 8]
  (c) eval_forward without outputs (the evaluation alone: the floor)

Every call ends with the library's own stream synchronisation, so a host clock around `reps` calls is the call time.  The
routes alternate inside a round; the table gives the median over the rounds and their min .. max.  (a) is also split into
its download and its host contraction.

    python scripts/expectations_timing.py [--rounds 9] [--reps 100] [--json out.json]
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
    N, nt, c = dp.N, dp.nsteps + 1, dp.c
    obs = np.stack([np.asarray(o, dtype=float) for o in prob.sym_operators] + [np.asarray(prob.system_sym, dtype=float)])
    assert not np.any(np.asarray(prob.system_asym)), "H_d of cnot3 is real"
    st = dp.pin(np.zeros((2 * N, nt, c), order="F"))
    ex = dp.pin(np.zeros((len(obs), nt, c), order="F"))

    def contract(states):
        u, v = states[:N], states[N:]
        return np.einsum("isc,oij,jsc->osc", u, obs, u, optimize=True) + np.einsum("isc,oij,jsc->osc", v, obs, v, optimize=True)

    def host_route():
        return contract(dp.eval_states(pcof, out=st))

    routes = {"a_states_pinned_plus_numpy": host_route,
              "a1_states_pinned_alone": lambda: dp.eval_states(pcof, out=st),
              "b_expectations_pinned": lambda: dp.eval_expectations(obs, pcof, out=ex),
              "c_no_outputs": lambda: dp.eval_forward(pcof)}
    bytes_out = {"a_states_pinned_plus_numpy": st.nbytes, "a1_states_pinned_alone": st.nbytes, "b_expectations_pinned": ex.nbytes,
                 "c_no_outputs": 0}
    for f in routes.values():                      # warm-up: code objects, staging buffers, pinned mappings, einsum paths
        for _ in range(10):
            f()
    assert dp.front_path_taken()
    # the two routes agree (the bound of tests/test_gpu_expectations.py)
    host = host_route()
    dev = dp.eval_expectations(obs, pcof, out=ex)
    S = (np.einsum("isc,oij,jsc->osc", np.abs(st[:N]), np.abs(obs), np.abs(st[:N]), optimize=True)
         + np.einsum("isc,oij,jsc->osc", np.abs(st[N:]), np.abs(obs), np.abs(st[N:]), optimize=True))
    ratio = float((np.abs(dev - host) / np.maximum(2 * (4 * N + 2) * 2.0 ** -52 * S, 1e-300)).max())
    per = {k: [] for k in routes}
    for _ in range(a.rounds):
        for k, f in routes.items():
            t0 = time.perf_counter()
            for _ in range(a.reps):
                f()
            per[k].append((time.perf_counter() - t0) / a.reps * 1e3)
    res = {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v), bytes=bytes_out[k]) for k, v in per.items()}
    d2 = qgd.DeviceProblem(prob, order); d2.set_controls(ctrl); d2.set_target(target)      # (a fresh handle: qgd_get_timings keeps earlier phases)
    d2.set_timing(1)
    d2.eval_expectations(obs, pcof); d2.eval_expectations(obs, pcof)
    phases = {n: round(float(ms), 4) for n, ms in sorted(d2.timings().items(), key=lambda kv: -kv[1])}
    d2.close()
    print(f"cnot3, {dp.nsteps} steps, order {order}, {len(obs)} real observables; {a.rounds} rounds of {a.reps} calls per route (ms per call)")
    for k in sorted(res):
        r = res[k]
        print(f"  {k:30s} median {r['median_ms']:.4f}   min {r['min_ms']:.4f}   max {r['max_ms']:.4f}   {r['bytes'] / 1e6:6.2f} MB out")
    print(f"  device vs host contraction: max |diff| / bound = {ratio:.4f}")
    print(f"  phases of eval_expectations (device ms, event bracketing on): {phases}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(routes=res, phases=phases, agreement_over_bound=ratio), f, indent=1)
    dp.close()


if __name__ == "__main__":
    main()
