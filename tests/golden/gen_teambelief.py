#!/usr/bin/env python3
"""Generate tests/golden/teambelief.npz: Bayesian-delegation updates of a pair's allocation
posterior recorded from the reference, for oc_team_belief_update.

Runs ONLY in the build container (the reference is imported with gen_golden.py's stubs).

For goal-directed episodes (GoalPolicy, eps 0.2, 40 steps) on five (level, A, seed) configs and both
choices of the self agent in the pair (agent 0, agent 1), a SubtaskAllocDistribution over the pair's
allocations is carried through the episode: the S joint allocations [(t, (a0, a1))] in subtask
order, then the (S + 1) S splits [(ti, (a0,)), (tj, (a1,))] in row-major (i, j), i != j, over
env.all_subtasks + [None].  For A = 2 that hand-built list must equal the reference's own
add_subtasks() enumeration with the joint-None entry (which prune_subtask_allocs deletes first,
bayesian_delegator.py:248) removed.  At every step, with obs_tm1 = env.obs_tm1 and actions_tm1 =
env.agent_actions, the distribution is updated with the reference's own pieces in bayes_update's
order (bayesian_delegator.py:1026-1072):
    subtask_alloc_is_doable(obs_tm1, ...) per member -> delete
    update = sum over the members of len(agents) * prob_nav_actions(obs_tm1, actions_tm1, subtask, agents,
        beta=1.3, no_level_1=True) on a FRESH E2E_BRTDP per call (value_init's values) -> update
    normalize
with the delegator's agent_name = the self agent and none_action_prob = 0.5.  A step where a
prob_nav_actions call raises AssertionError or ZeroDivisionError records `raised` and applies the
delete and the normalize only.  No completion events are given, so the priors are never reset and
the distribution can become empty.

Usage:  python tests/golden/gen_teambelief.py [seed ...]
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

CONFIGS = [  # (level, A, seed); the pair is agents (0, 1)
    ("partial-divider_salad", 2, 2101),
    ("full-divider_salad", 2, 2105),
    ("open-divider_tl", 3, 2202),
    ("open-divider_salad", 2, 2303),
    ("full-divider_tomato", 2, 2401),
]
MAX_T = 40
KIND = {"Chop": 1, "Merge": 2, "Deliver": 3}
BETA, NONE_P = 1.3, 0.5
FLOORS = dict(pruned=20, raised=20, joint=50, split=50, empty=10)
MAX_BYTES = 176337  # the largest fixture committed so far


def main():
    ref = gg.load_reference()
    nav_utils = ref[1]
    from navigation_planner.planners.e2e_brtdp import E2E_BRTDP  # noqa: E402
    from delegation_planner.bayesian_delegator import BayesianDelegator, SubtaskAllocation  # noqa: E402
    from delegation_planner.utils import SubtaskAllocDistribution  # noqa: E402

    def delegator(names, me):
        return BayesianDelegator(agent_name=names[me], all_agent_names=names, model_type="bd",
                                 planner=E2E_BRTDP(alpha=0.01, tau=2, cap=75, main_cap=100), none_action_prob=NONE_P)

    out, nseq = {}, 0
    tot = {k: 0 for k in FLOORS}
    print("%-24s %4s %5s %5s %6s %5s %5s %5s" % ("level", "self", "steps", "prune", "raised", "joint", "split", "empty"))
    for level, A, seed in CONFIGS:
        info = gg.RefEnv(ref, level, 4, 100).level_info()
        for me in (0, 1):
            env = gg.RefEnv(ref, level, A, 100)
            pol = gg.GoalPolicy(info, A, seed=seed, eps=0.2)
            names = [ag.name for ag in env.env.sim_agents]
            a0, a1 = names[0], names[1]
            subtasks = list(env.env.all_subtasks) + [None]
            S = len(subtasks) - 1
            N = S + 1
            kinds, starts, goals = [], [], []
            for st in subtasks[:-1]:
                s_obj, g_obj = nav_utils.get_subtask_obj(st)
                s_obj = s_obj if isinstance(s_obj, list) else [s_obj]
                kinds.append(KIND[type(st).__name__])
                starts.append([gg.content_mask(o) for o in s_obj] + [0] * (2 - len(s_obj)))
                goals.append(gg.content_mask(g_obj))
            hyp = [(t, t) for t in range(S)] + [(i, j) for i in range(N) for j in range(N) if i != j]
            allocs = []
            for i, j in hyp:
                if i == j:
                    allocs.append([SubtaskAllocation(subtask=subtasks[i], subtask_agent_names=(a0, a1))])
                else:
                    allocs.append([SubtaskAllocation(subtask=subtasks[i], subtask_agent_names=(a0,)),
                                   SubtaskAllocation(subtask=subtasks[j], subtask_agent_names=(a1,))])
            if A == 2:  # the reference's own enumeration, without the joint None
                d = delegator(names, me)
                d.incomplete_subtasks = list(env.env.all_subtasks)
                with contextlib.redirect_stdout(io.StringIO()):
                    own = d.add_subtasks().enumerate_subtask_allocs()
                own = [al for al in own if not (len(al) == 1 and al[0].subtask is None)]
                assert own == [tuple(al) for al in allocs], "add_subtasks() enumerates another list"
            with contextlib.redirect_stdout(io.StringIO()):
                dist = SubtaskAllocDistribution(allocs)
            rec = dict(agents=[], items=[], t=[], taken=[], live=[], belief=[], raised=[])
            st = env.canon(0)
            n = {k: 0 for k in FLOORS}
            before = np.ones(len(hyp), bool)
            for T in range(MAX_T):
                prev = st
                st, _, _ = env.step(pol.act(st))
                if env.err:
                    break
                obs_tm1 = env.env.obs_tm1
                acts = dict(env.env.agent_actions)
                taken = np.full(4, 4, np.uint8)
                for i, nm in enumerate(names):
                    taken[i] = gg.CODE[tuple(acts[nm])]
                with contextlib.redirect_stdout(io.StringIO()):
                    for alloc in dist.enumerate_subtask_allocs():
                        for m in alloc:
                            if not delegator(names, me).subtask_alloc_is_doable(
                                    env=obs_tm1, subtask=m.subtask, subtask_agent_names=m.subtask_agent_names):
                                dist.delete(alloc)
                                break
                    factors, raised = [], 0
                    try:
                        for alloc in dist.enumerate_subtask_allocs():
                            update = 0.0
                            for m in alloc:
                                p = delegator(names, me).prob_nav_actions(
                                    obs_tm1=copy.copy(obs_tm1), actions_tm1=acts, subtask=m.subtask,
                                    subtask_agent_names=m.subtask_agent_names, beta=BETA, no_level_1=True)
                                update += len(m.subtask_agent_names) * p
                            factors.append((alloc, float(update)))
                    except (AssertionError, ZeroDivisionError):
                        raised = 1
                    if not raised:
                        for alloc, f in factors:
                            dist.update(alloc, f)
                    dist.normalize()
                live = np.zeros(N * N, np.uint8)
                bel = np.zeros(N * N, np.float64)
                best, bv = None, -1.0
                for h, alloc in zip(hyp, allocs):
                    if tuple(alloc) in dist.probs:
                        live[h[0] * N + h[1]], bel[h[0] * N + h[1]] = 1, dist.probs[tuple(alloc)]
                        if dist.probs[tuple(alloc)] > bv:
                            best, bv = h, dist.probs[tuple(alloc)]
                now = np.array([live[i * N + j] != 0 for i, j in hyp])
                n["pruned"] += int((before & ~now).any())
                n["raised"] += raised
                n["empty"] += int(best is None)
                n["joint"] += int(best is not None and best[0] == best[1])
                n["split"] += int(best is not None and best[0] != best[1])
                before = now
                rec["agents"].append(prev["agents"].copy())
                rec["items"].append(prev["items"].copy())
                rec["t"].append(int(prev["t"]))
                rec["taken"].append(taken.copy())
                rec["live"].append(live)
                rec["belief"].append(bel)
                rec["raised"].append(raised)
                if st["flags"] & 1:
                    break
            print("%-24s %4d %5d %5d %6d %5d %5d %5d" % (level, me, len(rec["live"]), n["pruned"], n["raised"], n["joint"],
                                                         n["split"], n["empty"]))
            for k in tot:
                tot[k] += n[k]
            q = nseq
            out.update({"level_%d" % q: np.array(level), "A_%d" % q: np.int32(A), "pair_%d" % q: np.array([0, 1], np.int32),
                        "self_%d" % q: np.int32(me),
                        "sub_kind_%d" % q: np.array(kinds, np.int32), "sub_start_%d" % q: np.array(starts, np.uint8),
                        "sub_goal_%d" % q: np.array(goals, np.uint8),
                        "st_agents_%d" % q: np.array(rec["agents"], np.uint8),
                        "st_items_%d" % q: np.array(rec["items"], np.uint8),
                        "st_t_%d" % q: np.array(rec["t"], np.int32), "taken_%d" % q: np.array(rec["taken"], np.uint8),
                        "live_%d" % q: np.array(rec["live"]), "belief_%d" % q: np.array(rec["belief"], np.float64),
                        "raised_%d" % q: np.array(rec["raised"], np.uint8)})
            nseq += 1
    print("total:", tot)
    for k, floor in FLOORS.items():
        assert tot[k] >= floor, "coverage of %s: %d < %d: pick other seeds" % (k, tot[k], floor)
    path = os.path.join(HERE, "teambelief.npz")
    np.savez_compressed(path, nseq=np.int32(nseq), beta=BETA, none_action_prob=NONE_P, **out)
    size = os.path.getsize(path)
    print("wrote %s: %d sequences, %d bytes" % (path, nseq, size))
    assert size <= MAX_BYTES, "larger than the largest committed fixture: drop steps"


if __name__ == "__main__":
    if len(sys.argv) > 1:  # seeds on the command line, one per config, for picking them
        CONFIGS = [(c[0], c[1], int(s)) for c, s in zip(CONFIGS, sys.argv[1:])]
    main()
