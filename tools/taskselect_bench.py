#!/usr/bin/env python3
"""oc_task_select against the routes it replaces: partial-divider_salad, A = 2, the
level's 9 subtasks, M = 1 and M = 2 scripted agents, 2^18 and 2^20 envs whose states and task
states are taken 20 steps into the scripted loop (scripted_actions -> step, random starts).  In one
run, per shape:
  (a) task_select    oc_task_select
  (b) bounds         oc_subtask_bounds on the same M x S configurations
  (c) torch_route    (b) + oc_progress counts + the torch masked-argmin and bookkeeping ops a caller
                     needs today for the same rule
Windows of >= 20 ms of back-to-back launches between HIP events, three alternations, best of each.
Writes profiles/taskselect/taskselect_bench.json.

  python tools/taskselect_bench.py --probe    the 2^20-env, M = 2 shape only: four launches each of
      (a) and (b) and no timing, the workload of a counter pass (rocprofv3 --pmc ... -- python ...)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-cooking_amd"))
from gym_cooking_amd import capi  # noqa: E402
from gym_cooking_amd.envs import OvercookedVecEnv  # noqa: E402


def window(launch, min_ms=20.0):
    """ms per launch over a window of at least min_ms of back-to-back launches."""
    launch()
    torch.cuda.synchronize()
    n = 4
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            launch()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= min_ms:
            return ms / n
        n *= 2


def torch_route(eb, state, rows, agents, tstate, flags):
    """Today's route as one callable: the bounds of the M x S configurations, the counts, and the
    rule in torch ops over its own bookkeeping tensors (incomplete sets as bool [M, S, B])."""
    S, M, B, P = len(rows), len(agents), eb.B, eb.pitch
    EP = capi.event_planes(S)
    cfg = [capi.subtask(r.kind, [a], [r.start_mask[0], r.start_mask[1]], r.goal_mask) for a in agents for r in rows]
    lb = torch.empty((M * S, P), dtype=torch.float32, device=eb.device)
    doable = torch.empty((M * S, P), dtype=torch.uint8, device=eb.device)
    counts = torch.empty((1, S, P), dtype=torch.uint8, device=eb.device)
    bounds = eb.subtask_bounds_launcher(state, cfg, lb, doable)
    progress = eb.progress_launcher(state, state, rows, None, 1, counts, None, None)
    bits = torch.arange(S, device=eb.device)
    inc = ((tstate[:, (bits >> 3).tolist(), :B].long() >> (bits & 7)[None, :, None]) & 1).bool()
    cur0, cnt0 = tstate[:, EP, :B].long(), tstate[:, EP + 1, :B].long()
    real = torch.tensor([r.kind != capi.SUB_NONE for r in rows], device=eb.device)[:, None]
    inf = torch.tensor(float("inf"), device=eb.device)
    commit, distinct = bool(flags & capi.OC_TASK_COMMIT), bool(flags & capi.OC_TASK_DISTINCT)

    def run():
        bounds()
        progress()
        c = counts[0, :, :B].long()
        taken = torch.zeros((S + 1, B), dtype=torch.bool, device=eb.device)
        for m in range(M):
            cur, cnt, im = cur0[m].clone(), cnt0[m].clone(), inc[m].clone()
            has = cur < S
            ci = cur.clamp(max=S - 1)[None]
            done = has & (c.gather(0, ci)[0] > cnt)
            im.scatter_(0, ci, im.gather(0, ci) & ~done[None])
            cur = torch.where(done, S, cur)
            cand = im & real & (doable[m * S:(m + 1) * S, :B] != 0)
            if distinct:
                cand &= ~taken[:S]
            best = torch.where(cand, lb[m * S:(m + 1) * S, :B], inf)
            new = torch.where(cand.any(0), best.argmin(0), S)
            if commit:
                ci = cur.clamp(max=S - 1)[None]
                new = torch.where((cur < S) & cand.gather(0, ci)[0], cur, new)
            take = (new != cur) & (new < S)
            cnt = torch.where(take, c.gather(0, new.clamp(max=S - 1)[None])[0], cnt)
            taken.scatter_(0, new[None], True)
            cur0[m], cnt0[m], inc[m] = new, cnt, im
    return run, len(cfg)


def main():
    level, A = "partial-divider_salad", 2
    out = {"level": level, "A": A, "shapes": []}
    probe = "--probe" in sys.argv[1:]
    for B in ((1 << 20,) if probe else (1 << 18, 1 << 20)):
        for agents in (((0, 1),) if probe else ((1,), (0, 1))):
            env = OvercookedVecEnv(level, A, B, random_starts=capi.OC_START_AGENTS | capi.OC_START_ITEMS, seed=5)
            env.reset()
            others = torch.randint(0, 5, (A * env.P,), dtype=torch.uint8, device=env.batch.device)
            for _ in range(20):  # 20 steps into the scripted loop (an unscripted agent acts at random)
                buf = others.clone()
                acts, _ = env.scripted_actions(agents, out=buf)
                env.step(acts)
                others = torch.randint(0, 5, (A * env.P,), dtype=torch.uint8, device=env.batch.device)
            cur, _ = env.partner_tasks(agents)
            eb, rows, S, M = env.batch, env._sub_rows, len(env._sub_rows), len(agents)
            flags = capi.OC_TASK_COMMIT | capi.OC_TASK_DISTINCT
            saved = env._task.clone()
            ts = saved.clone()
            bound = torch.empty((M, eb.pitch), dtype=torch.float32, device=eb.device)
            info = torch.empty((M, eb.pitch), dtype=torch.uint8, device=eb.device)
            route, ncfg = torch_route(eb, env.state, rows, agents, saved, flags)
            cfg = [capi.subtask(r.kind, [a], [r.start_mask[0], r.start_mask[1]], r.goal_mask) for a in agents for r in rows]
            lb = torch.empty((ncfg, eb.pitch), dtype=torch.float32, device=eb.device)
            doable = torch.empty((ncfg, eb.pitch), dtype=torch.uint8, device=eb.device)
            calls = {
                "task_select": eb.task_select_launcher(env.state, rows, agents, ts, None, flags, bound, info),
                "bounds": eb.subtask_bounds_launcher(env.state, cfg, lb, doable),
                "torch_route": route,
            }
            if probe:
                for k in ("task_select", "bounds"):
                    for _ in range(4):
                        calls[k]()
                torch.cuda.synchronize()
                print("probe done: %d envs, agents %s" % (B, list(agents)))
                return
            rounds = [{k: window(f) for k, f in calls.items()} for _ in range(3)]
            best = {k: min(r[k] for r in rounds) for k in calls}
            EP = capi.event_planes(S)
            incomplete = sum(int(((saved[:, i >> 3, :B] >> (i & 7)) & 1).sum()) for i in range(S)) / (M * B)
            shape = {"B": B, "agents": list(agents), "subtasks": S, "configurations": ncfg,
                     "incomplete_per_agent": incomplete, "following_a_subtask": float((cur < S).float().mean()),
                     "bytes_per_env": {"task_select": 2 * M * (EP + 2) + 5 * M, "bounds": 5 * ncfg},
                     "ms_rounds": rounds, "ms_best": best, "ratio_a_over_b": best["task_select"] / best["bounds"],
                     "ratio_a_over_c": best["task_select"] / best["torch_route"]}
            out["shapes"].append(shape)
            print(json.dumps(shape), flush=True)
            del env, eb, route, calls
            torch.cuda.empty_cache()
    d = os.path.join(ROOT, "profiles", "taskselect")
    os.makedirs(d, exist_ok=True)
    dst = os.environ.get("TASKSELECT_BENCH_OUT", os.path.join(d, "taskselect_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
