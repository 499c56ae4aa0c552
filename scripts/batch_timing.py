"""Batched evaluation against the loop of single calls it replaces: cnot2 at the benchmark shape (order 8,
100 steps), one handle, one process.  For K = 1, 4, 16, 64, 256 members:
  (a) a Python loop of K DeviceProblem.discrete_adjoint calls        (b) one DeviceProblem.eval_batch call
  (c) the same two forward-only (eval_forward / eval_batch(gradient=False))
The routes alternate inside every round; every call ends in a host wait for its results (the single call polls its result
mirror, the batch synchronises the stream), so the host clock around `reps` repetitions is the time of the work.  Reported:
median and min..max over the rounds of the time per call, the time per member, and the ratio (a)/(b).

    timeout 300 python scripts/batch_timing.py [--rounds 9] [--out FILE.json]
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("at least 7 rounds")
    if not torch.cuda.is_available():
        sys.exit("batch_timing.py measures on the GPU: none found")
    qgd = import_package()
    prob, ctrl, pcof, target = cases.cnot2_case(qgd, nsteps=100, tf=100.0, amp=1e-2)
    dp = qgd.DeviceProblem(prob, 8); dp.set_controls(ctrl); dp.set_target(target); dp.set_timing(0)
    rng = np.random.default_rng(0)
    P = np.ascontiguousarray(pcof + 1e-3 * rng.standard_normal((max(KS), len(pcof))))

    def loop(K, gradient):
        if gradient:
            for k in range(K):
                dp.discrete_adjoint(P[k])
        else:
            for k in range(K):
                dp.eval_forward(P[k])

    def batch(K, gradient):
        dp.eval_batch(P[:K], gradient=gradient)

    def clock(fn, K, gradient, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn(K, gradient)
        return (time.perf_counter() - t0) / reps

    # what is timed is what the tests compare: members equal single calls, and the batch takes the side-by-side route
    G, S, st = dp.eval_batch(P[:4])
    assert dp.batch_path_taken() and not st.any()
    for k in range(4):
        g, o = dp.discrete_adjoint(P[k])
        assert dp.small_path_taken() and np.array_equal(g, G[k]) and np.array_equal(np.asarray(o), S[k])
    rows = []
    for K in KS:
        reps = max(2, 512 // K)                          # (a window of a loop: >= 30 ms)
        for gradient in (True, False):                    # warm-up of every shape timed: buffers of this chunk size, code objects
            for fn in (loop, batch):
                clock(fn, K, gradient, 2)
        t = {(r, g): [] for r in ("loop", "batch") for g in (True, False)}
        for _ in range(args.rounds):
            for gradient in (True, False):
                t[("loop", gradient)].append(clock(loop, K, gradient, reps))
                t[("batch", gradient)].append(clock(batch, K, gradient, reps))
        for gradient in (True, False):
            a, b = t[("loop", gradient)], t[("batch", gradient)]
            rows.append({"K": K, "gradient": gradient, "reps": reps, "rounds": args.rounds,
                         "loop_us": [statistics.median(a) * 1e6, min(a) * 1e6, max(a) * 1e6],
                         "batch_us": [statistics.median(b) * 1e6, min(b) * 1e6, max(b) * 1e6],
                         "ratio": statistics.median(a) / statistics.median(b),
                         "ratio_min_max": [min(x / y for x, y in zip(a, b)), max(x / y for x, y in zip(a, b))]})
    dp.close()
    box = torch.cuda.get_device_name(0)
    print(f"cnot2, order 8, 100 steps, {P.shape[1]} coefficients; {box}; {args.rounds} rounds, median (min..max) in us")
    print("| K | call | (a) loop of K single calls, us | (b) one eval_batch call, us | (b) per member, us | (a)/(b) |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        a, b = r["loop_us"], r["batch_us"]
        print(f"| {r['K']} | {'gradient' if r['gradient'] else 'forward'} | {a[0]:.0f} ({a[1]:.0f}..{a[2]:.0f}) | {b[0]:.0f} ({b[1]:.0f}..{b[2]:.0f}) | "
              f"{b[0] / r['K']:.2f} | {r['ratio']:.1f} ({r['ratio_min_max'][0]:.1f}..{r['ratio_min_max'][1]:.1f}) |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": box, "n_pcof": int(P.shape[1]), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
