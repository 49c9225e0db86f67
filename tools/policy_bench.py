#!/usr/bin/env python3
"""oc_nav_policy against the grouped oc_nav_likelihood on the same rows: partial-
divider_salad, A = 2, mid-episode states; one-agent tables at 2^18 and 2^20 rows and a joint table
at 2^18; probs NULL and given; windows of >= 20 ms of back-to-back launches between HIP events,
three alternations of the two calls per shape in one run.  Writes
profiles/navpolicy/policy_bench.json."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-cooking_amd"))
from gym_cooking_amd import capi, recipes  # noqa: E402
from gym_cooking_amd.engine import OvercookedBatch  # noqa: E402


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


def main():
    out = {"level": "partial-divider_salad", "A": 2, "shapes": []}
    for B, agents in ((1 << 18, [1]), (1 << 20, [1]), (1 << 18, [0, 1])):
        eb = OvercookedBatch("partial-divider_salad", 2, B, device="cuda:0")
        eb.set_likelihood_form(capi.OC_LIK_FORM_GROUPED)
        s, s2, act = eb.new_state(), eb.new_state(), eb.new_actions()
        eb.reset(s)
        for t in range(20):  # mid-episode states
            eb.gen_actions(act, t, 5)
            eb.step(s, s2, act)
            s, s2 = s2, s
        eb.gen_actions(act, 99, 5)  # the likelihood's taken actions
        table = capi.policy_subtasks(recipes.all_subtasks(eb.level), eb.level.encoding, agents)
        alloc = (torch.arange(eb.pitch, device="cuda:0") % len(table)).to(torch.uint8)
        nc = 25 if len(agents) == 2 else 5
        pact = eb.new_actions()
        probs = torch.empty(nc * eb.pitch, dtype=torch.float64, device="cuda:0")
        flags = torch.empty(eb.pitch, dtype=torch.uint8, device="cuda:0")
        lik, lfl = torch.empty(eb.pitch, dtype=torch.float64, device="cuda:0"), torch.empty_like(flags)
        mode = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE
        calls = {
            "likelihood_grouped": eb.nav_likelihood_launcher(s, act, table, 0, 1.3, 0.5, alloc, lik, lfl),
            "policy_probs_null": eb.nav_policy_launcher(s, table, pact, 1.3, 0.5, mode, alloc, 0, 1, 0, None, nc, flags),
            "policy_probs": eb.nav_policy_launcher(s, table, pact, 1.3, 0.5, mode, alloc, 0, 1, 0, probs, nc, flags),
        }
        rounds = [{k: window(f) for k, f in calls.items()} for _ in range(3)]
        best = {k: min(r[k] for r in rounds) for k in calls}
        ok = int((flags[:B] == capi.POL_OK).sum())
        shape = {"B": B, "agents": agents, "num_cand": nc, "subtasks": len(table), "ok_rows": ok, "ms_rounds": rounds,
                 "ms_best": best, "ratio_probs_null": best["policy_probs_null"] / best["likelihood_grouped"],
                 "ratio_probs": best["policy_probs"] / best["likelihood_grouped"]}
        out["shapes"].append(shape)
        print(json.dumps(shape))
    d = os.path.join(ROOT, "profiles", "navpolicy")
    os.makedirs(d, exist_ok=True)
    dst = os.environ.get("POLICY_BENCH_OUT", os.path.join(d, "policy_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
