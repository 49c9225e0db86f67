#!/usr/bin/env python3
"""Generate tests/golden/belief.npz: Bayesian-delegation belief updates recorded from the
reference, for oc_belief_update's one-agent hypotheses.

Runs ONLY in the build container (the reference is imported with gen_golden.py's stubs).

For goal-directed episodes (GoalPolicy, eps 0.2) on three (level, A) configs, two episodes each, and each of the first
two agents as the watched agent a, a SubtaskAllocDistribution over [(st, (a,))] for st in
env.all_subtasks + [None] (uniform, delegation_planner/utils.py:11-20) is carried through the
episode.  At every step, with obs_tm1 = env.obs_tm1 and actions_tm1 = env.agent_actions, it is
updated with the reference's own pieces in bayes_update's order (bayesian_delegator.py:1026-1072):
    subtask_alloc_is_doable(obs_tm1, ...) -> delete
    prob_nav_actions(obs_tm1, actions_tm1, st, (a,), beta=1.3, no_level_1=True) on a FRESH E2E_BRTDP
        per call (value_init's values, as gen_likelihood.py) -> update
    normalize
with the delegator's agent_name = a and none_action_prob = 0.5.  A step where a prob_nav_actions
call raises (the assert at :672) records `raised` and applies the delete and the normalize only.
No completion events are given, so the priors are never reset.

Usage:  python tests/golden/gen_belief.py
"""
from __future__ import annotations

import contextlib
import copy
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402

CONFIGS = [  # (level, A, seed): two episodes per level
    ("partial-divider_salad", 2, 2101),
    ("partial-divider_salad", 2, 2105),
    ("open-divider_tl", 3, 2202),
    ("open-divider_tl", 3, 2203),
    ("open-divider_salad", 2, 2303),
    ("open-divider_salad", 2, 2304),
]
MAX_T = 40
KIND = {"Chop": 1, "Merge": 2, "Deliver": 3}
BETA, NONE_P = 1.3, 0.5


def main():
    ref = gg.load_reference()
    nav_utils = ref[1]
    from navigation_planner.planners.e2e_brtdp import E2E_BRTDP  # noqa: E402
    from delegation_planner.bayesian_delegator import BayesianDelegator, SubtaskAllocation  # noqa: E402
    from delegation_planner.utils import SubtaskAllocDistribution  # noqa: E402

    def delegator(names, a):
        return BayesianDelegator(agent_name=names[a], all_agent_names=names, model_type="bd",
                                 planner=E2E_BRTDP(alpha=0.01, tau=2, cap=75, main_cap=100), none_action_prob=NONE_P)

    out, nseq = {}, 0
    print("%-24s %2s %5s %5s %6s %6s %6s" % ("level", "a", "steps", "prune", "raised", "single", "hyp-"))
    tot_prune = tot_raised = 0
    for level, A, seed in CONFIGS:
        info = gg.RefEnv(ref, level, 4, 100).level_info()
        env = gg.RefEnv(ref, level, A, 100)
        pol = gg.GoalPolicy(info, A, seed=seed, eps=0.2)
        names = [ag.name for ag in env.env.sim_agents]
        subtasks = list(env.env.all_subtasks) + [None]
        S = len(subtasks) - 1
        kinds, starts, goals = [], [], []
        for st in subtasks[:-1]:
            s_obj, g_obj = nav_utils.get_subtask_obj(st)
            s_obj = s_obj if isinstance(s_obj, list) else [s_obj]
            kinds.append(KIND[type(st).__name__])
            starts.append([gg.content_mask(o) for o in s_obj] + [0] * (2 - len(s_obj)))
            goals.append(gg.content_mask(g_obj))
        watched = list(range(min(A, 2)))
        allocs = {a: [[SubtaskAllocation(subtask=st, subtask_agent_names=(names[a],))] for st in subtasks]
                  for a in watched}
        dist = {a: SubtaskAllocDistribution(allocs[a]) for a in watched}
        rec = {a: dict(agents=[], items=[], t=[], taken=[], live=[], belief=[], raised=[]) for a in watched}
        st = env.canon(0)
        for T in range(MAX_T):
            prev = st
            st, _, _ = env.step(pol.act(st))
            if env.err:
                break
            obs_tm1 = env.env.obs_tm1
            acts = dict(env.env.agent_actions)
            taken = np.full(4, 4, np.uint8)
            for i, n in enumerate(names):
                taken[i] = gg.CODE[tuple(acts[n])]
            for a in watched:
                d = dist[a]
                with contextlib.redirect_stdout(io.StringIO()):
                    for alloc in d.enumerate_subtask_allocs():
                        t0 = alloc[0]
                        if not delegator(names, a).subtask_alloc_is_doable(env=obs_tm1, subtask=t0.subtask,
                                                                           subtask_agent_names=t0.subtask_agent_names):
                            d.delete(alloc)
                    factors, raised = [], 0
                    try:
                        for alloc in d.enumerate_subtask_allocs():
                            t0 = alloc[0]
                            p = delegator(names, a).prob_nav_actions(obs_tm1=copy.copy(obs_tm1), actions_tm1=acts,
                                                                     subtask=t0.subtask,
                                                                     subtask_agent_names=t0.subtask_agent_names,
                                                                     beta=BETA, no_level_1=True)
                            factors.append((alloc, float(p)))
                    except AssertionError:
                        raised = 1
                    # ZeroDivisionError (None with no movable action) is not caught: pick another seed
                    if not raised:
                        for alloc, p in factors:
                            d.update(alloc, p)
                    d.normalize()
                live = np.zeros(S + 1, np.uint8)
                bel = np.zeros(S + 1, np.float64)
                for i, alloc in enumerate(allocs[a]):
                    if tuple(alloc) in d.probs:
                        live[i], bel[i] = 1, d.probs[tuple(alloc)]
                r = rec[a]
                r["agents"].append(prev["agents"].copy())
                r["items"].append(prev["items"].copy())
                r["t"].append(int(prev["t"]))
                r["taken"].append(taken.copy())
                r["live"].append(live)
                r["belief"].append(bel)
                r["raised"].append(raised)
            if st["flags"] & 1:
                break
        for a in watched:
            r, q = rec[a], nseq
            live = np.array(r["live"])
            before = np.vstack([np.ones((1, S + 1), np.uint8), live[:-1]])
            prune = int(((before != 0) & (live == 0)).any(1).sum())
            raised = int(np.sum(r["raised"]))
            print("%-24s %2d %5d %5d %6d %6d %6d" % (level, a, len(live), prune, raised, int((live.sum(1) == 1).sum()),
                                                      int(((before != 0) & (live == 0)).sum())))
            tot_prune, tot_raised = tot_prune + prune, tot_raised + raised
            out.update({"level_%d" % q: np.array(level), "A_%d" % q: np.int32(A), "agent_%d" % q: np.int32(a),
                        "sub_kind_%d" % q: np.array(kinds, np.int32), "sub_start_%d" % q: np.array(starts, np.uint8),
                        "sub_goal_%d" % q: np.array(goals, np.uint8),
                        "st_agents_%d" % q: np.array(r["agents"], np.uint8), "st_items_%d" % q: np.array(r["items"], np.uint8),
                        "st_t_%d" % q: np.array(r["t"], np.int32), "taken_%d" % q: np.array(r["taken"], np.uint8),
                        "live_%d" % q: live, "belief_%d" % q: np.array(r["belief"], np.float64),
                        "raised_%d" % q: np.array(r["raised"], np.uint8)})
            nseq += 1
    print("total: %d pruning steps, %d raised steps" % (tot_prune, tot_raised))
    assert tot_prune >= 20 and tot_raised >= 5, "coverage: pick other seeds"
    path = os.path.join(HERE, "belief.npz")
    np.savez_compressed(path, nseq=np.int32(nseq), beta=BETA, none_action_prob=NONE_P, **out)
    print("wrote %s: %d sequences, %d bytes" % (path, nseq, os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) > 1:  # seeds on the command line, one per config, for picking them
        CONFIGS = [(c[0], c[1], int(s)) for c, s in zip(CONFIGS, sys.argv[1:])]
    main()
