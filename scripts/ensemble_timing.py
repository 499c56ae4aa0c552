"""What an ensemble evaluation costs: cnot2 at the benchmark shape (order 8, 100 steps), one process, the
protocol of scripts/batch_timing.py.  For K = 1, 4, 16, 64, 256 members (detuned copies of the problem):
  (a) a Python loop over K handles, one per member: DeviceProblem.discrete_adjoint on each, then ensemble_reduce on the host
  (b) discrete_adjoint_ensemble(route=--route), the functional form, which returns the members' rows: on the loop route the same
      loop behind device_problem's cache (controls, target and cost type are looked at on every member of every call), on the
      device route the members side by side on the problem's own handle (qgd_eval_ensemble), K rows downloaded
  (c) EnsembleObjective(route=--route), what an optimiser calls: no rows, one gradient downloaded per call on the device route
The routes alternate inside every round; every call ends in a host wait for its results, so the host clock around `reps`
repetitions is the time of the work.  Reported: median and min..max over the rounds of the time per call.

    timeout 300 python scripts/ensemble_timing.py [--route auto|device|loop] [--rounds 9] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from __graft_entry__ import import_package
import cases

KS = (1, 4, 16, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--route", default="auto", choices=["auto", "device", "loop"], help="route of columns (b) and (c)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("at least 7 rounds")
    if not torch.cuda.is_available():
        sys.exit("ensemble_timing.py measures on the GPU: none found")
    qgd = import_package()
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=100, tf=100.0, amp=1e-2)
    N, Kmax = prob.N_tot_levels, max(KS)
    shift = np.linspace(-0.02, 0.02, Kmax)[:, None, None] * np.diag(np.arange(N, dtype=float))
    full = qgd.Ensemble(prob.system_sym[None] + shift, np.repeat(prob.system_asym[None], Kmax, axis=0))
    singles = []
    for k in range(Kmax):
        h = qgd.DeviceProblem(full.member_problem(prob, k), 8); h.set_controls(ctrl); h.set_target(target); h.set_timing(0)
        singles.append(h)
    n_ess = prob.N_ess_levels

    def loop(K, ens):
        res = [singles[k].discrete_adjoint(pcof) for k in range(K)]
        return qgd.ensemble_reduce(np.array([g for g, _ in res]), np.array([np.asarray(o) for _, o in res]), None, "Infidelity", n_ess)

    def functional(K, ens):
        return qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, ens, order=8, route=args.route)

    def objective(K, ens):
        return objectives[K](pcof)

    def clock(fn, K, ens, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn(K, ens)
        return (time.perf_counter() - t0) / reps

    out, objectives, routes = [], {}, {}
    for K in KS:
        ens = qgd.Ensemble(full.system_sym[:K], full.system_asym[:K])
        g, c, gd = loop(K, ens)                                # what is timed is what the tests compare: the same bits either way
        r = functional(K, ens)
        assert np.array_equal(g, r.grad) and (c, gd) == (r.cost, r.guard)
        objectives[K] = qgd.EnsembleObjective(prob, ctrl, target, ens, 8, "Infidelity", route=args.route)
        go, co, gdo = objective(K, ens)
        assert np.array_equal(g, go) and (c, gd) == (co, gdo)
        routes[K] = r.route
        reps = max(2, 512 // K)
        fns = {"loop": loop, "functional": functional, "objective": objective}
        for fn in fns.values():
            clock(fn, K, ens, 2)
        t = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                t[name].append(clock(fn, K, ens, reps))
        stat = lambda x: [statistics.median(x) * 1e6, min(x) * 1e6, max(x) * 1e6]
        out.append({"K": K, "reps": reps, "rounds": args.rounds, "route": r.route, "loop_us": stat(t["loop"]),
                    "functional_us": stat(t["functional"]), "objective_us": stat(t["objective"])})
        objectives.pop(K).close()
    for h in singles:
        h.close()
    box = torch.cuda.get_device_name(0)
    print(f"cnot2, order 8, 100 steps, {len(pcof)} coefficients; {box}; {args.rounds} rounds, median (min..max) in us")
    print(f"route asked for: {args.route}")
    print("| K | (a) K handles + host reduction, us | (a) per member, us | (b) discrete_adjoint_ensemble, us | (b) per member, us "
          "| (c) EnsembleObjective, us | (c) per member, us | route taken |")
    print("|---|---|---|---|---|---|---|---|")
    for r in out:
        a, b, o = r["loop_us"], r["functional_us"], r["objective_us"]
        print(f"| {r['K']} | {a[0]:.0f} ({a[1]:.0f}..{a[2]:.0f}) | {a[0] / r['K']:.1f} | {b[0]:.0f} ({b[1]:.0f}..{b[2]:.0f}) | {b[0] / r['K']:.1f} "
              f"| {o[0]:.0f} ({o[1]:.0f}..{o[2]:.0f}) | {o[0] / r['K']:.1f} | {r['route']} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": box, "n_pcof": int(len(pcof)), "route": args.route, "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
