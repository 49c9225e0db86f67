#!/usr/bin/env python3
"""Time oc_progress (per-subtask counts, completion events, shaped reward) against oc_step at
the same batch size, as time per algorithmic byte.

Workload: partial-divider_salad, A = 2, its all_subtasks, B = 2^20 and 2^16 envs, states taken
mid-episode (40 steps of oc_gen_actions codes), n = 1 (two states) and n = 20 (an oc_step_n
trajectory).  Each figure is a window of back-to-back launches of at least 20 ms between two HIP
events; oc_progress alternates in the same process with oc_step on the same box, three
alternations, the median reported.

Algorithmic bytes per env (computed here from the shapes):
  oc_step      reads the state's NP planes and A action bytes, writes NP planes (no exec / coll)
  oc_progress  reads L = 3A + 2K + 1 planes (item cells, masks, held slots, agent x / y, flags;
               not t) of two states at n = 1, of one state per step (plus one) in the trajectory
               form, and writes S + planes + 4 bytes per step
The ratio reported is (progress time / progress bytes) / (step time / step bytes); the aim was
at most 1.25 at 2^20 envs.  Prints one JSON line.

Usage:  python tools/progress_bench.py [--out profiles/progress/progress_bench.json]
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

LEVEL, A, STEPS, WINDOW_MS, ROUNDS, TRAJ = "partial-divider_salad", 2, 40, 20.0, 3, 20


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
        raise SystemExit("progress_bench needs a GPU (no CPU fallback)")
    from gym_cooking_amd import capi, recipes
    from gym_cooking_amd.engine import OvercookedBatch, _bound, _ptr
    dev = "cuda:0"
    rows = []
    for B in (int(x) for x in args.sizes.split(",")):
        eb = OvercookedBatch(LEVEL, A, B, max_T=100, device=dev)
        subs = capi.progress_subtasks(recipes.all_subtasks(eb.level), eb.level.encoding)
        S, planes = len(subs), capi.event_planes(len(subs))
        s, s2, act = eb.new_state(), eb.new_state(), eb.new_actions()
        eb.reset(s)
        for t in range(STEPS):
            eb.gen_actions(act, t, seed=3)
            eb.step(s, s2, act)
            s, s2 = s2, s
        nb = eb.layout.state_bytes
        acts = eb.new_actions(TRAJ)
        for r in range(TRAJ):
            eb.gen_actions(acts[r], STEPS + r, seed=3)
        traj = torch.empty(TRAJ * nb, dtype=torch.uint8, device=dev)
        eb.step_n(s, traj[(TRAJ - 1) * nb:], acts, TRAJ, traj=traj)
        NP, L = eb.layout.num_planes, 3 * A + 2 * eb.K + 1
        step_bytes = (2 * NP + A) * B
        step_fn = _bound(eb.lib.oc_step, (eb._h, _ptr(s), _ptr(s2), _ptr(act), None, None, None, B, eb._stream()))
        for n in (1, TRAJ):
            c, e, rw = eb.new_progress_buffers(S, n)
            prog_bytes = ((n + 1) * L + n * (S + planes + 4)) * B
            runs = {"progress": timed(eb.progress_launcher(s, traj, subs, None, n, c, e, rw)), "step": timed(step_fn)}
            ms = {k: [] for k in runs}
            for _ in range(ROUNDS):
                for k, (fn, iters) in runs.items():
                    ms[k].append(window_ms(fn, iters))
            med = {k: statistics.median(v) for k, v in ms.items()}
            rows.append(dict(
                envs=B, n=n, subtasks=S, progress_ms=round(med["progress"], 5),
                progress_windows=[round(x, 5) for x in ms["progress"]], launches_per_window=runs["progress"][1],
                progress_bytes=prog_bytes, progress_tb_per_s=round(prog_bytes / med["progress"] / 1e9, 3),
                step_ms=round(med["step"], 5), step_windows=[round(x, 5) for x in ms["step"]],
                step_launches_per_window=runs["step"][1], step_bytes=step_bytes,
                step_tb_per_s=round(step_bytes / med["step"] / 1e9, 3),
                time_per_byte_ratio=round((med["progress"] / prog_bytes) / (med["step"] / step_bytes), 3)))
            del c, e, rw
    line = json.dumps(dict(bench="oc_progress", level=LEVEL, agents=A, device=torch.cuda.get_device_name(0),
                           yardstick="oc_step at the same B, alternating in the same run", rows=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
