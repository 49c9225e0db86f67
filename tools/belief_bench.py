#!/usr/bin/env python3
"""oc_belief_update against the routes it replaces: partial-divider_salad, A = 2, the
level's 9 subtasks, M = 1 and M = 2 watched agents, 2^18 and 2^20 envs whose states, beliefs and
bstate are taken 20 steps into the scripted loop (scripted_actions -> step -> partner_beliefs, random
starts).  In one run, per shape:
  (a) belief_update  oc_belief_update over the last step, with its events
  (b) policy_probs   oc_nav_policy with `probs` on one hypothesis (subtask 0 of the first watched
                     agent) for the same rows: one view, 5 legality tests, 5 successors, one bound each
  (c) torch_route    today's route per watched agent: S + 1 oc_nav_likelihood launches (one
                     hypothesis each), oc_subtask_bounds for the pruning, and the torch f64 ops of
                     the rule over [S + 1, B]
The launches of a window update the same belief buffers in place again and again: that changes the
values and not the work, except that the first launch prunes and applies the step's events (the live
hypotheses per watched agent before and after the windows are recorded).
Windows of >= 20 ms of back-to-back launches between HIP events, three alternations, best of each.
Writes profiles/belief/belief_bench.json.

  python tools/belief_bench.py --probe    the 2^20-env, M = 2 shape only: four launches each of (a)
      and (b) and no timing, the workload of a counter pass (rocprofv3 --pmc ... -- python ...)."""
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


def torch_route(eb, prev, taken, rows, agents, belief, bstate, beta, nap):
    """Today's route as one callable: per watched agent S + 1 likelihood launches and one bounds
    launch, then the rule (prune, raise test, multiply, normalise, argmax) in torch f64 ops."""
    S, M, B, P = len(rows), len(agents), eb.B, eb.pitch
    HP = capi.belief_planes(S)
    per = []
    for a in agents:
        cfg = [capi.subtask(r.kind, [a], [r.start_mask[0], r.start_mask[1]], r.goal_mask) for r in rows]
        cfg.append(capi.subtask(capi.SUB_NONE, [a], [0, 0], 0))
        lik = torch.empty((S + 1, P), dtype=torch.float64, device=eb.device)
        lfl = torch.empty((S + 1, P), dtype=torch.uint8, device=eb.device)
        lb = torch.empty((S, P), dtype=torch.float32, device=eb.device)
        doable = torch.empty((S, P), dtype=torch.uint8, device=eb.device)
        launches = [eb.nav_likelihood_launcher(prev, taken, [cfg[i]], a, beta, nap, None, lik[i], lfl[i])
                    for i in range(S + 1)]
        launches.append(eb.subtask_bounds_launcher(prev, cfg[:S], lb, doable))
        per.append((launches, lik, lfl, doable))
    bits = torch.arange(S + 1, device=eb.device)
    live0 = ((bstate[:, (HP + (bits >> 3)).tolist(), :B].long() >> (bits & 7)[None, :, None]) & 1).bool()
    bel0 = belief[:, :, :B].clone()

    def run():
        for m in range(M):
            launches, lik, lfl, doable = per[m]
            for f in launches:
                f()
            live, b = live0[m].clone(), bel0[m].clone()
            live[:S] &= doable[:, :B] != 0
            b = torch.where(live, b, 0.0)
            raised = (live[:S] & (lfl[:S, :B] != capi.LIK_OK)).any(0)
            b = torch.where(raised[None] | ~live, b, b * lik[:, :B])
            total = b.sum(0)
            n = live.sum(0)
            b = torch.where(live, torch.where(total == 0, 1.0 / n, b * (1.0 / total)), b)
            best = torch.where(live, b, -1.0).argmax(0)
            live0[m], bel0[m] = live, b
        return best
    return run, M * (S + 2)


def main():
    level, A, beta, nap = "partial-divider_salad", 2, 1.3, 0.5
    out = {"level": level, "A": A, "shapes": []}
    probe = "--probe" in sys.argv[1:]
    for B in ((1 << 20,) if probe else (1 << 18, 1 << 20)):
        for agents in (((0, 1),) if probe else ((1,), (0, 1))):
            env = OvercookedVecEnv(level, A, B, random_starts=capi.OC_START_AGENTS | capi.OC_START_ITEMS, seed=5)
            env.reset()
            env.partner_beliefs(agents)
            for k in range(20):  # 20 steps into the scripted loop (both agents scripted, one or both watched)
                acts, _ = env.scripted_actions((0, 1))
                env.step(acts)
                if k < 19:  # the last step's update is the one measured
                    env.partner_beliefs(agents)
            eb, rows, S, M = env.batch, env._sub_rows, len(env._sub_rows), len(agents)
            HP, EP = capi.belief_planes(S), capi.event_planes(S)
            prev, cur = env._s[env._i ^ 1], env.state
            events = torch.zeros((1, EP, eb.pitch), dtype=torch.uint8, device=eb.device)
            eb.progress(prev, cur, rows, None, 1, None, events, None)
            bel, bst, bmap, info = (t.clone() for t in env._belief)
            live_before = sum(int(((bst[:, HP + (i >> 3), :B] >> (i & 7)) & 1).sum()) for i in range(S + 1)) / (M * B)
            route, nlaunch = torch_route(eb, prev, env.ex, rows, agents, bel, bst, beta, nap)
            table = capi.policy_subtasks([env.subtasks[0]], eb.level.encoding, [agents[0]])
            pacts = eb.new_actions()
            probs = torch.empty((5, eb.pitch), dtype=torch.float64, device=eb.device)
            pfl = torch.empty(eb.pitch, dtype=torch.uint8, device=eb.device)
            calls = {
                "belief_update": eb.belief_update_launcher(prev, env.ex, rows, agents, bel, bst, events, beta, nap, 0,
                                                           bmap, info),
                "policy_probs": eb.nav_policy_launcher(prev, table, pacts, beta, nap,
                                                       capi.OC_POLICY_GREEDY | capi.OC_POLICY_COUNT_STATE, None, 0, 0, 0,
                                                       probs, 5, pfl),
                "torch_route": route,
            }
            if probe:
                for k in ("belief_update", "policy_probs"):
                    for _ in range(4):
                        calls[k]()
                torch.cuda.synchronize()
                print("probe done: %d envs, agents %s" % (B, list(agents)))
                return
            rounds = [{k: window(f) for k, f in calls.items()} for _ in range(3)]
            best = {k: min(r[k] for r in rounds) for k in calls}
            live_after = sum(int(((bst[:, HP + (i >> 3), :B] >> (i & 7)) & 1).sum()) for i in range(S + 1)) / (M * B)
            fl = info[:, :B]
            shape = {"B": B, "agents": list(agents), "subtasks": S, "route_launches": nlaunch,
                     "live_per_agent_before": live_before, "live_per_agent_after": live_after,
                     "info_share": {k: float(((fl & v) != 0).float().mean()) for k, v in
                                    (("updated", capi.BELF_UPDATED), ("pruned", capi.BELF_PRUNED), ("reinit", capi.BELF_REINIT),
                                     ("reset", capi.BELF_RESET), ("raised", capi.BELF_RAISED))},
                     "ms_rounds": rounds, "ms_best": best, "ratio_a_over_b": best["belief_update"] / best["policy_probs"],
                     "ratio_a_over_c": best["belief_update"] / best["torch_route"]}
            out["shapes"].append(shape)
            print(json.dumps(shape), flush=True)
            del env, eb, route, calls
            torch.cuda.empty_cache()
    d = os.path.join(ROOT, "profiles", "belief")
    os.makedirs(d, exist_ok=True)
    dst = os.environ.get("BELIEF_BENCH_OUT", os.path.join(d, "belief_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
