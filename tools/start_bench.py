#!/usr/bin/env python3
"""Time oc_reset_random (randomised episode starts) in its three uses.

Workload: partial-divider_salad, A = 2, B = 2^20 and 2^16 envs.  Each figure is a window of
back-to-back launches of at least 20 ms between two HIP events; the forms alternate in the same
process, three alternations, the median reported.
  (a) full    : oc_reset_random(state, NULL) against oc_reset at the same B (both write every plane)
  (b) masked  : oc_step(prev -> cur) followed by oc_reset_random(cur, prev) against that oc_step
                alone; prev is a mid-run state (40 steps of oc_gen_actions codes) in which about 1 %
                of the envs, picked at random, carry DONE
  (c) no DONE : oc_reset_random(cur, prev) alone on a prev without a DONE env (one flags load per
                lane, then the block leaves), and alone at 1 % for comparison
Prints one JSON line.

Usage:  python tools/start_bench.py [--out profiles/startdist/start_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-cooking_amd"))

import torch  # noqa: E402

LEVEL, A, STEPS, WINDOW_MS, ROUNDS, DONE_FRAC = "partial-divider_salad", 2, 40, 20.0, 3, 0.01


def window_ms(fn, iters: int) -> float:
    """ms per call over `iters` back-to-back calls between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def timed(fn) -> tuple:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = max(window_ms(fn, 5), 1e-3)
    return fn, max(10, int(WINDOW_MS / per) + 1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--sizes", default="1048576,65536")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("start_bench needs a GPU (no CPU fallback)")
    from gym_cooking_amd import capi
    from gym_cooking_amd.engine import OvercookedBatch, _bound, _ptr
    dev = "cuda:0"
    rows = []
    for B in (int(x) for x in args.sizes.split(",")):
        eb = OvercookedBatch(LEVEL, A, B, max_T=100, device=dev)
        NP, P = eb.layout.num_planes, eb.pitch
        s, s2, act = eb.new_state(), eb.new_state(), eb.new_actions()
        eb.reset_random(s, None, 3, 0, 3)
        for t in range(STEPS):
            eb.gen_actions(act, t, seed=3)
            eb.step(s, s2, act)
            s, s2 = s2, s
        eb.gen_actions(act, STEPS, seed=3)
        prev_none, prev, cur, full = s, s.clone(), s2, eb.new_state()
        torch.manual_seed(5)
        done = torch.rand(B, device=dev) < DONE_FRAC
        prev.view(NP, P)[eb.layout.plane_flags, :B] |= done.to(torch.uint8) * capi.OC_FLAG_DONE
        lanes = int((done.view(-1, 4).any(1)).sum()) if B % 4 == 0 else None
        ex, coll, stats = eb.new_exec(), eb.new_coll(), eb.new_stats()
        step = _bound(eb.lib.oc_step, (eb._h, _ptr(prev), _ptr(cur), _ptr(act), _ptr(ex), _ptr(coll), _ptr(stats),
                                       B, eb._stream()))
        masked = eb.reset_random_launcher(cur, prev, 3, STEPS + 1, 3)
        masked_none = eb.reset_random_launcher(cur, prev_none, 3, STEPS + 1, 3)

        def step_masked():
            step()
            masked()
        runs = {"reset": timed(_bound(eb.lib.oc_reset, (eb._h, _ptr(full), B, eb._stream()))),
                "full": timed(eb.reset_random_launcher(full, None, 3, 0, 3)),
                "step": timed(step), "step_masked": timed(step_masked),
                "masked_1pct": timed(masked), "masked_none": timed(masked_none)}
        ms = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, (fn, iters) in runs.items():
                ms[k].append(window_ms(fn, iters))
        med = {k: statistics.median(v) for k, v in ms.items()}
        rows.append(dict(
            envs=B, done_envs=int(done.sum()), lanes_with_done=lanes,
            ms={k: round(v, 5) for k, v in med.items()}, ms_windows={k: [round(x, 5) for x in v] for k, v in ms.items()},
            launches_per_window={k: v[1] for k, v in runs.items()},
            bytes=dict(reset=NP * P, full=NP * ((B + 3) // 4 * 4),
                       masked_flags_read=B, masked_per_lane_with_done=2 * 4 * NP,
                       step=(2 * NP + 3 * A + 1) * B),
            full_over_reset=round(med["full"] / med["reset"], 3),
            masked_added_over_step=round((med["step_masked"] - med["step"]) / med["step"], 3),
            masked_none_us=round(med["masked_none"] * 1e3, 3), masked_1pct_us=round(med["masked_1pct"] * 1e3, 3)))
    line = json.dumps(dict(bench="oc_reset_random", level=LEVEL, agents=A, device=torch.cuda.get_device_name(0),
                           done_fraction=DONE_FRAC, rows=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
