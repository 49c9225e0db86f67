#!/usr/bin/env python3
"""oc_team_select against its neighbours: full-divider_salad and partial-divider_salad,
A = 2, the level's 9 subtasks, the pair (0, 1), 2^18 and 2^20 envs whose states and team states are
taken 20 steps into the team loop (team_actions -> step, random starts).  In one run, per shape:
  (a) team_select    oc_team_select
  (b) task_select    oc_task_select with M = 2 (COMMIT | DISTINCT) on the same states, its own task
                     state one call in
  (c) torch_route    what a caller has today for the same rule: oc_subtask_bounds on the 3 x S = 27
                     configurations + oc_progress counts + the torch ops that restate the rule over
                     their own bookkeeping tensors
Windows of >= 20 ms of back-to-back launches between HIP events, three alternations, best of each.
Writes profiles/teamselect/teamselect_bench.json.

  python tools/teamselect_bench.py --probe    the 2^20-env full-divider shape only: four launches
      each of (a) and of oc_subtask_bounds and no timing, the workload of a counter pass
      (rocprofv3 --pmc ... -- python ...)."""
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


def team_configs(rows, pair):
    """The 3 x S configurations of the rule: a0's one-agent rows, a1's, the two-agent rows."""
    cfg = []
    for agents in ([pair[0]], [pair[1]], list(pair)):
        cfg += [capi.subtask(r.kind, agents if r.kind != capi.SUB_NONE else agents[:1], [r.start_mask[0], r.start_mask[1]],
                             r.goal_mask) for r in rows]
    return cfg


def torch_route(eb, state, rows, pair, tstate, flags):
    """Today's route as one callable: the bounds of the 3 x S configurations, the counts, and the rule
    in torch ops over its own bookkeeping tensors (the incomplete set as bool [S, B])."""
    S, B, P = len(rows), eb.B, eb.pitch
    EP = capi.event_planes(S)
    OUT = capi.OC_TEAM_OUT
    cfg = team_configs(rows, pair)
    lb = torch.empty((3 * S, P), dtype=torch.float32, device=eb.device)
    doable = torch.empty((3 * S, P), dtype=torch.uint8, device=eb.device)
    counts = torch.empty((1, S, P), dtype=torch.uint8, device=eb.device)
    bounds = eb.subtask_bounds_launcher(state, cfg, lb, doable)
    progress = eb.progress_launcher(state, state, rows, None, 1, counts, None, None)
    bits = torch.arange(S, device=eb.device)
    st = {"inc": ((tstate[(bits >> 3).tolist(), :B].long() >> (bits & 7)[:, None]) & 1).bool()}
    for q, k in enumerate(("cur0", "cur1", "curJ", "cnt0", "cnt1")):
        st[k] = tstate[EP + q, :B].long()
    real = torch.tensor([r.kind != capi.SUB_NONE for r in rows], device=eb.device)[:, None]
    commit, split_first = bool(flags & capi.OC_TEAM_COMMIT), bool(flags & capi.OC_TEAM_SPLIT_FIRST)

    def at(table, idx, none):
        return torch.where(idx < S, table.gather(0, idx.clamp(max=S - 1)[None])[0], none)

    def top2(C, bound):
        w = torch.where(C, 1.0 / bound.double(), -1.0)
        v1, i1 = w.max(0)
        first = torch.where(v1 >= 0, i1, S)
        w2 = w.scatter(0, i1[None], -1.0)
        v2, i2 = w2.max(0)
        return w, first, torch.where(v2 >= 0, i2, S)

    def run():
        bounds()
        progress()
        c = counts[0, :, :B].long()
        inc, cur0, cur1, curJ, cnt0, cnt1 = (st[k].clone() for k in ("inc", "cur0", "cur1", "curJ", "cnt0", "cnt1"))
        e0, e1, eJ = cur0, cur1, curJ
        joint = curJ < S
        doneJ = joint & (at(c, curJ, 0) > cnt0)
        done0 = ~joint & (cur0 < S) & (at(c, cur0, 0) > cnt0)
        done1 = ~joint & (cur1 < S) & (at(c, cur1, 0) > cnt1)
        for done, cur in ((doneJ, curJ), (done0, cur0), (done1, cur1)):
            ci = cur.clamp(max=S - 1)[None]
            inc.scatter_(0, ci, inc.gather(0, ci) & ~done[None])
        gone = doneJ | done0 | done1
        cur0, cur1, curJ = torch.where(gone, S, cur0), torch.where(gone, S, cur1), torch.where(gone, OUT, curJ)
        opn = inc & real
        C0, C1, CJ = (opn & (doable[q * S:(q + 1) * S, :B] != 0) for q in range(3))
        lb0, lb1, lbJ = (lb[q * S:(q + 1) * S, :B] for q in range(3))
        w0, f0, s0 = top2(C0, lb0)
        w1, f1, s1 = top2(C1, lb1)
        wJ, iJ, _ = top2(CJ, lbJ)
        joint = curJ < S
        keep = torch.where(joint, at(CJ, curJ, False), (cur0 < S) & (cur1 < S) & at(C0, cur0, False) & at(C1, cur1, False))
        keep = keep & ~gone if commit else torch.zeros_like(gone)
        have = (f0 < S) | (f1 < S)
        same = have & (f0 == f1)
        x, y = at(w0, f0, 0.0) + at(w1, s1, 0.0), at(w0, s0, 0.0) + at(w1, f1, 0.0)
        p0, p1 = torch.where(same & ~(x >= y), s0, f0), torch.where(same & (x >= y), s1, f1)
        wS = at(w0, p0, 0.0) + at(w1, p1, 0.0)
        first = have & (p0 < S) & (p1 < S) if split_first else torch.zeros_like(gone)
        take_j = ~first & (iJ < S) & (~have | (at(wJ, iJ, 0.0) >= wS))
        take_s = ~take_j & have
        cur0 = torch.where(keep, cur0, torch.where(take_j, OUT, torch.where(take_s, p0, S)))
        cur1 = torch.where(keep, cur1, torch.where(take_j, OUT, torch.where(take_s, p1, S)))
        curJ = torch.where(keep, curJ, torch.where(take_j, iJ, OUT))
        sw = (cur0 != e0) | (cur1 != e1) | (curJ != eJ)
        joint = curJ < S
        cnt0 = torch.where(sw, torch.where(joint, at(c, curJ, 0), at(c, cur0, 0)), cnt0)
        cnt1 = torch.where(sw, torch.where(joint, 0, at(c, cur1, 0)), cnt1)
        st.update(inc=inc, cur0=cur0, cur1=cur1, curJ=curJ, cnt0=cnt0, cnt1=cnt1)
    return run, cfg


def main():
    A, pair = 2, (0, 1)
    probe = "--probe" in sys.argv[1:]
    out = {"A": A, "pair": list(pair), "shapes": []}
    for level in (("full-divider_salad",) if probe else ("full-divider_salad", "partial-divider_salad")):
        for B in ((1 << 20,) if probe else (1 << 18, 1 << 20)):
            env = OvercookedVecEnv(level, A, B, random_starts=capi.OC_START_AGENTS | capi.OC_START_ITEMS, seed=5)
            env.reset()
            for _ in range(20):  # 20 steps into the team loop
                acts, _ = env.team_actions(pair)
                env.step(acts)
            *_, tinfo = env.team_tasks(pair)
            eb, rows, S = env.batch, env._sub_rows, len(env._sub_rows)
            flags = capi.OC_TEAM_COMMIT
            saved = env._team.clone()
            ts = saved.clone()
            bound = torch.empty((2, eb.pitch), dtype=torch.float32, device=eb.device)
            info = torch.empty(eb.pitch, dtype=torch.uint8, device=eb.device)
            route, cfg = torch_route(eb, env.state, rows, pair, saved, flags)
            lb = torch.empty((len(cfg), eb.pitch), dtype=torch.float32, device=eb.device)
            doable = torch.empty((len(cfg), eb.pitch), dtype=torch.uint8, device=eb.device)
            solo = eb.new_task_state(S, 2)
            sbound = torch.empty((2, eb.pitch), dtype=torch.float32, device=eb.device)
            sinfo = torch.empty((2, eb.pitch), dtype=torch.uint8, device=eb.device)
            sflags = capi.OC_TASK_COMMIT | capi.OC_TASK_DISTINCT
            eb.task_select(env.state, rows, pair, solo, None, sflags | capi.OC_TASK_INIT, sbound, sinfo)
            calls = {
                "team_select": eb.team_select_launcher(env.state, rows, pair, ts, None, flags, bound, info),
                "task_select": eb.task_select_launcher(env.state, rows, pair, solo, None, sflags, sbound, sinfo),
                "torch_route": route,
            }
            if probe:
                bounds = eb.subtask_bounds_launcher(env.state, cfg, lb, doable)
                for f in (calls["team_select"], bounds):
                    for _ in range(4):
                        f()
                torch.cuda.synchronize()
                print("probe done: %s, %d envs" % (level, B))
                return
            rounds = [{k: window(f) for k, f in calls.items()} for _ in range(3)]
            best = {k: min(r[k] for r in rounds) for k in calls}
            EP = capi.event_planes(S)
            incomplete = sum(int(((saved[i >> 3, :B] >> (i & 7)) & 1).sum()) for i in range(S)) / B
            ti = tinfo.long()
            shape = {"level": level, "B": B, "subtasks": S, "configurations": len(cfg), "incomplete_per_env": incomplete,
                     "joint_share": float(((ti & capi.TEAMF_JOINT) != 0).float().mean()),
                     "idle_share": float(((saved[EP + 2, :B] >= S) & (saved[EP, :B] >= S) & (saved[EP + 1, :B] >= S)).float().mean()),
                     "bytes_per_env": {"team_select": 2 * (EP + 5) + 9, "bounds": 5 * len(cfg)},
                     "ms_rounds": rounds, "ms_best": best, "ratio_a_over_b": best["team_select"] / best["task_select"],
                     "ratio_a_over_c": best["team_select"] / best["torch_route"]}
            out["shapes"].append(shape)
            print(json.dumps(shape), flush=True)
            del env, eb, route, calls
            torch.cuda.empty_cache()
    d = os.path.join(ROOT, "profiles", "teamselect")
    os.makedirs(d, exist_ok=True)
    dst = os.environ.get("TEAMSELECT_BENCH_OUT", os.path.join(d, "teamselect_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
