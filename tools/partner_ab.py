#!/usr/bin/env python3
"""A/B of the partner kernels between builds of liboc_engine.so, on one box, the sibling of
tools/bounds_ab.py: oc_nav_policy, oc_task_select, oc_team_select and oc_belief_update on the shape
of their benches (partial-divider_salad, A = 2, the level's 9 subtasks, 2^18 and 2^20 envs whose
states and beliefs are taken 20 steps into the scripted loop with random starts), each build in a
fresh process, alternating.  Per build and size: ms per launch of each call (windows of >= 20 ms of
back-to-back launches between HIP events, best of three) and a digest of every output byte of one
launch of each on the same inputs, so that the builds' outputs can be compared.
  python tools/partner_ab.py --libs A.so A_copy.so B.so [--rounds 3]
Naming one build twice (a copy under another name) gives the spread of a build against itself in
the same run.  Prints one JSON line per (round, lib, size)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(lib):
    sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "gym-cooking_amd")]
    import torch
    from gym_cooking_amd import capi
    capi.load_library(lib)
    from belief_bench import window
    from gym_cooking_amd.envs import OvercookedVecEnv
    level, A, pair, beta, nap = "partial-divider_salad", 2, (0, 1), 1.3, 0.5
    for B in (1 << 18, 1 << 20):
        env = OvercookedVecEnv(level, A, B, random_starts=capi.OC_START_AGENTS | capi.OC_START_ITEMS, seed=5)
        env.reset()
        env.partner_beliefs(pair)
        for k in range(20):
            acts, _ = env.scripted_actions(pair)
            env.step(acts)
            if k < 19:  # the last step's update is the one measured
                env.partner_beliefs(pair)
        eb, rows, S, dev = env.batch, env._sub_rows, len(env._sub_rows), env.batch.device
        P, EP = eb.pitch, capi.event_planes(S)
        prev, cur = env._s[env._i ^ 1], env.state
        events = torch.zeros((1, EP, P), dtype=torch.uint8, device=dev)
        eb.progress(prev, cur, rows, None, 1, None, events, None)
        bel, bst, bmap, binfo = (t.clone() for t in env._belief)
        task, team = eb.new_task_state(S, 2), eb.new_team_state(S)
        tb, ti = torch.zeros((2, P), dtype=torch.float32, device=dev), torch.zeros((2, P), dtype=torch.uint8, device=dev)
        mb, mi = torch.zeros((2, P), dtype=torch.float32, device=dev), torch.zeros(P, dtype=torch.uint8, device=dev)
        tfl, mfl = capi.OC_TASK_COMMIT | capi.OC_TASK_DISTINCT, capi.OC_TEAM_COMMIT
        eb.task_select(cur, rows, pair, task, None, tfl | capi.OC_TASK_INIT, tb, ti)
        eb.team_select(cur, rows, pair, team, None, mfl | capi.OC_TEAM_INIT, mb, mi)
        table = capi.policy_subtasks(env.subtasks, eb.level.encoding, [1])
        alloc = (torch.arange(P, device=dev) % len(table)).to(torch.uint8)
        pact, probs = eb.new_actions(), torch.zeros(5 * P, dtype=torch.float64, device=dev)
        pfl = torch.zeros(P, dtype=torch.uint8, device=dev)
        mode = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE
        calls = {
            "policy": eb.nav_policy_launcher(cur, table, pact, beta, nap, mode, alloc, 0, 1, 0, probs, 5, pfl),
            "task_select": eb.task_select_launcher(cur, rows, pair, task, prev, tfl, tb, ti),
            "team_select": eb.team_select_launcher(cur, rows, pair, team, prev, mfl, mb, mi),
            "belief_update": eb.belief_update_launcher(prev, env.ex, rows, pair, bel, bst, events, beta, nap, 0, bmap, binfo),
        }
        for f in calls.values():  # one launch of each on the same inputs: the digest
            f()
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in (pact, probs, pfl, task, tb, ti, team, mb, mi, bel, bst, bmap, binfo):
            h.update(t.contiguous().cpu().numpy().tobytes())
        rounds = [{k: window(f) for k, f in calls.items()} for _ in range(3)]
        print(json.dumps({"lib": os.path.basename(lib), "B": B, "digest": h.hexdigest()[:16],
                          "ms": {k: min(r[k] for r in rounds) for k in calls}, "ms_rounds": rounds}), flush=True)
        del env, eb, calls
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    for r in range(a.rounds):
        for lib in a.libs:
            out = subprocess.run([sys.executable, __file__, "--child", os.path.abspath(lib)], capture_output=True,
                                 text=True, timeout=300)
            lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
            if out.returncode != 0 or len(lines) != 2:
                print(out.stderr[-2000:], file=sys.stderr)
                return 1
            for x in lines:
                d = json.loads(x)
                d["round"] = r
                print(json.dumps(d), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
