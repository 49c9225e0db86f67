#!/usr/bin/env python3
"""Time oc_observe (grid feature planes + legal-move masks) against a write-only pass of the
same output tensor.

Workload: partial-divider_salad, A = 2, B = 2^20 and 2^16 envs, u8 and f16 planes, states taken
mid-episode (40 steps of oc_gen_actions codes).  Each figure is a window of back-to-back
launches of at least 20 ms between two HIP events; oc_observe alternates in the same process
with `tensor.zero_()` on the same output (torch's fill: the floor is not the code under test),
three alternations, the median reported.  Both store policies run: OC_OBS_STORES=plain|nt is
read by oc_create, so each variant has its own handle; OC_OBS_TILE (envs per block at most),
when set, applies to both and is recorded.  Prints one JSON line.

Usage:  python tools/obs_bench.py [--out profiles/obs/obs_bench.json]
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

LEVEL, A, STEPS, WINDOW_MS, ROUNDS = "partial-divider_salad", 2, 40, 20.0, 3


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
        raise SystemExit("obs_bench needs a GPU (no CPU fallback)")
    from gym_cooking_amd.engine import OvercookedBatch
    dev = "cuda:0"
    rows = []
    for B in (int(x) for x in args.sizes.split(",")):
        batches = {}
        for variant in ("plain", "nt"):
            os.environ["OC_OBS_STORES"] = variant
            batches[variant] = OvercookedBatch(LEVEL, A, B, max_T=100, device=dev)
        os.environ.pop("OC_OBS_STORES")
        eb = batches["plain"]
        s, s2, act = eb.new_state(), eb.new_state(), eb.new_actions()
        eb.reset(s)
        for t in range(STEPS):
            eb.gen_actions(act, t, seed=3)
            eb.step(s, s2, act)
            s, s2 = s2, s
        mask = eb.new_action_mask()
        for dtype, name in ((torch.uint8, "u8"), (torch.float16, "f16")):
            obs = eb.new_obs(dtype)
            nbytes = obs.numel() * obs.element_size() + A * B
            runs = {v: timed(batches[v].observe_launcher(s, obs, mask)) for v in ("plain", "nt")}
            runs["zero"] = timed(obs.zero_)
            ms = {k: [] for k in runs}
            for _ in range(ROUNDS):
                for k, (fn, iters) in runs.items():
                    ms[k].append(window_ms(fn, iters))
            med = {k: statistics.median(v) for k, v in ms.items()}
            for v in ("plain", "nt"):
                rows.append(dict(envs=B, dtype=name, stores=v, ms_per_launch=round(med[v], 5),
                                 ms_windows=[round(x, 5) for x in ms[v]], launches_per_window=runs[v][1],
                                 bytes_written=nbytes, state_bytes_read=eb.layout.num_planes * B,
                                 tb_per_s=round(nbytes / med[v] / 1e9, 3),
                                 zero_ms=round(med["zero"], 5), zero_windows=[round(x, 5) for x in ms["zero"]],
                                 zero_tb_per_s=round(obs.numel() * obs.element_size() / med["zero"] / 1e9, 3),
                                 ratio_to_zero=round(med[v] / med["zero"], 3)))
            del obs
    line = json.dumps(dict(bench="oc_observe", level=LEVEL, agents=A, device=torch.cuda.get_device_name(0),
                           floor="torch zero_() of the same output tensor",
                           tile_envs_cap=os.environ.get("OC_OBS_TILE", "default"), rows=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
