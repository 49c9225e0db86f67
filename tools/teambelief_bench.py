#!/usr/bin/env python3
"""oc_team_belief_update against the routes beside it: full-divider_salad and
partial-divider_salad, A = 2, the level's 9 subtasks, the pair (0, 1) with self agent 1, 2^18 and 2^20
envs whose states, beliefs and tbstate are taken 20 steps into the team loop (team_actions -> step ->
team_beliefs, random starts).  In one run, per shape:
  (a) team_belief    oc_team_belief_update over the last step, with its events
  (b) belief_m2      oc_belief_update with M = 2 watched agents on the same states (scale, no target:
                     it has no joint rows and 2 (S + 1) beliefs per env against (S + 1)^2 - 1)
  (c) torch_route    today's route: 3 S + 2 oc_nav_likelihood launches (one member row each),
                     oc_subtask_bounds on the 3 S configurations, and the torch f64 ops of the rule
                     over [N, N, B] (`rule`, checked against the host call on CPU tensors: --check)
The launches of a window update the same buffers in place again and again: that changes the values
and not the work, except that the first launch prunes and applies the step's events.
Windows of >= 20 ms of back-to-back launches between HIP events, three alternations, best of each.
Writes profiles/teambelief/teambelief_bench.json.

  python tools/teambelief_bench.py --check   no GPU: `rule` on CPU tensors against
      oc_cpu_team_belief_update over 10 steps of the host team loop at 512 envs.
  python tools/teambelief_bench.py --probe   the 2^20-env full-divider shape only: four launches of
      (a) and no timing, the workload of a counter pass (rocprofv3 --pmc ... -- python ...)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-cooking_amd"))
from gym_cooking_amd import capi  # noqa: E402


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


def set_bits(planes, n):
    """bool [n, B] of the bit set in u8 [planes, B]."""
    i = torch.arange(n, device=planes.device)
    return ((planes[(i >> 3).tolist()].long() >> (i & 7)[:, None]) & 1).bool()


def rule(S, bel, l0, l1, lJ, doable, L, raises, order):
    """Steps 3 to 8 of the rule in torch f64 ops on any device.  bel f64 [N, N, B]; l0, l1 bool
    [S + 1, B], lJ bool [S, B]: the live sets at entry; doable bool [3, S, B]; L f64 [3, S + 1, B]
    (row S of L[0], L[1] the None members); raises bool [3, B]; order: the hypotheses' (i, j) in
    reference order as two index tensors.  Returns (bel', l0', l1', lJ', best index into order, or
    -1 where nothing is live, raised [B], empty [B])."""
    N = S + 1
    eye = torch.eye(N, dtype=torch.bool, device=bel.device)[:, :, None]

    def matrix(a, b, j):
        m = (a[:, None] & b[None]) & ~eye
        d = torch.zeros_like(m)
        d[torch.arange(S), torch.arange(S)] = j
        return m | d

    before = matrix(l0, l1, lJ)
    l0, l1, lJ = l0.clone(), l1.clone(), lJ & doable[2]
    l0[:S] &= doable[0]
    l1[:S] &= doable[1]
    live = matrix(l0, l1, lJ)
    bel = torch.where(before & ~live, 0.0, bel)
    n_live = live.sum((0, 1))
    empty = n_live == 0
    need0 = (live[:S] & ~eye[:S]).any((0, 1))
    need1 = (live[:, :S] & ~eye[:, :S]).any((0, 1))
    raised = ~empty & ((need0 & raises[0]) | (need1 & raises[1]) | (lJ.any(0) & raises[2]))
    fac = L[0][:, None] + L[1][None]
    fac[torch.arange(S), torch.arange(S)] = 2.0 * L[2][:S]
    bel = torch.where(live & ~raised, bel * fac, bel)
    oi, oj = order
    vals = torch.where(live[oi, oj], bel[oi, oj], 0.0)
    total = vals.cumsum(0)[-1]  # the sum in reference order
    r = torch.where(total == 0, 1.0 / n_live, 1.0 / total)
    bel = torch.where(live, torch.where(total == 0, r, bel * r), bel)
    best = torch.where(live[oi, oj], bel[oi, oj], -1.0).argmax(0)
    return bel, l0, l1, lJ, torch.where(empty, -1, best), raised, empty


def order_of(S, device):
    N = S + 1
    hyp = [(t, t) for t in range(S)] + [(i, j) for i in range(N) for j in range(N) if i != j]
    return (torch.tensor([h[0] for h in hyp], device=device), torch.tensor([h[1] for h in hyp], device=device))


def member_rows(rows, pair):
    """The 3 S + 2 member rows in `lik`'s plane order: a0's S rows and None, a1's, the pair's S rows."""
    cfg = lambda ags: [capi.subtask(r.kind, ags, [r.start_mask[0], r.start_mask[1]], r.goal_mask) for r in rows]  # noqa: E731
    none = lambda a: [capi.subtask(capi.SUB_NONE, [a], [0, 0], 0)]  # noqa: E731
    return cfg([pair[0]]) + none(pair[0]) + cfg([pair[1]]) + none(pair[1]) + cfg(list(pair))


def torch_route(eb, prev, taken, rows, pair, me, belief, tbstate, beta, nap):
    """Today's route as one callable: 3 S + 2 likelihood launches, one bounds launch, then `rule`."""
    S, B, P = len(rows), eb.B, eb.pitch
    N = S + 1
    mem = member_rows(rows, pair)
    lik = torch.empty((3 * S + 2, P), dtype=torch.float64, device=eb.device)
    lfl = torch.empty((3 * S + 2, P), dtype=torch.uint8, device=eb.device)
    lb = torch.empty((3 * S, P), dtype=torch.float32, device=eb.device)
    doable = torch.empty((3 * S, P), dtype=torch.uint8, device=eb.device)
    launches = [eb.nav_likelihood_launcher(prev, taken, [mem[i]], me, beta, nap, None, lik[i], lfl[i])
                for i in range(3 * S + 2)]
    launches.append(eb.subtask_bounds_launcher(prev, mem[:S] + mem[N:N + S] + mem[2 * N:], lb, doable))
    _, p0, p1, pJ = capi.team_belief_sets(tbstate, S)
    st = [set_bits(p0[:, :B], N), set_bits(p1[:, :B], N), set_bits(pJ[:, :B], S), belief[:, :B].view(N, N, B).clone()]
    order = order_of(S, eb.device)
    sub = torch.cat([torch.arange(S), N + torch.arange(S), 2 * N + torch.arange(S)]).to(eb.device)

    def run():
        for f in launches:
            f()
        L = torch.zeros((3, N, B), dtype=torch.float64, device=eb.device)
        L[0], L[1], L[2, :S] = lik[:N, :B], lik[N:2 * N, :B], lik[2 * N:, :B]
        raises = (lfl[sub, :B].view(3, S, B) == capi.LIK_RAISES).any(1)
        bel, l0, l1, lJ, best, _, _ = rule(S, st[3], st[0], st[1], st[2], (doable[:, :B] != 0).view(3, S, B), L, raises, order)
        st[:] = [l0, l1, lJ, bel]
        return best
    return run, 3 * S + 3


def check():
    """`rule` on CPU tensors against oc_cpu_team_belief_update: the host call's own likelihoods and
    pruned sets as the rule's inputs, its beliefs, sets, raised, empty and map as the expectation."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import teambelief_ref as tb
    import teamselect_ref as tsr
    level, A, pair, B, me = "full-divider_salad", 2, (0, 1), 512, 1
    _, rec = tb.closed_loop(level, A, pair, B, 10, record_every=1, check=False, selfs=(me,))
    import oc_testlib as tl
    rows = tsr.level_rows(tl.load_level(level))
    S = len(rows)
    N = S + 1
    order = order_of(S, "cpu")
    n = 0
    for prev, taken, events, fl, bel, ts, abel, ats, alik, amap, ainfo in rec[me][1:]:
        upd = (ainfo[:B] & (tb.REINIT | tb.RESET)) == 0
        if not upd.any():
            continue
        sets = [torch.from_numpy(x[:, upd]) for x in tb.unpack(ts, S, B)[1:]]
        after = [torch.from_numpy(x[:, upd]) for x in tb.unpack(ats, S, B)[1:]]
        doable = torch.stack([after[f][:S] | ~sets[f][:S] for f in range(3)])
        mul = torch.from_numpy((ainfo[:B][upd] & tb.UPDATED) != 0)
        L = torch.zeros((3, N, int(upd.sum())), dtype=torch.float64)
        lk = torch.from_numpy(alik[:, :B][:, upd])
        L[0], L[1], L[2, :S] = lk[:N], lk[N:2 * N], lk[2 * N:]
        L = torch.where(mul, L, 0.0)
        raises = torch.from_numpy((ainfo[:B][upd] & tb.RAISED) != 0)[None].expand(3, -1)
        b0 = torch.from_numpy(bel[:, :B][:, upd].reshape(N, N, -1).copy())
        got, l0, l1, lJ, best, raised, empty = rule(S, b0, sets[0], sets[1], sets[2], doable, L, raises, order)
        want = torch.from_numpy(abel[:, :B][:, upd].reshape(N, N, -1).copy())
        live = torch.from_numpy(tb.live_matrix(after[0].numpy().copy(), after[1].numpy().copy(), after[2].numpy().copy(), S))
        err = torch.where(live, (got - want).abs() / want.abs().clamp_min(1e-300), 0.0).max()
        assert err <= 1e-12, err
        assert torch.equal(l0, after[0]) and torch.equal(l1, after[1]) and torch.equal(lJ, after[2])
        assert torch.equal(empty, torch.from_numpy((ainfo[:B][upd] & tb.EMPTY) != 0))
        n += int(upd.sum())
    print("rule matches oc_cpu_team_belief_update on %d env-steps" % n)


def main():
    if "--check" in sys.argv[1:]:
        return check()
    from gym_cooking_amd.envs import OvercookedVecEnv
    A, pair, me, beta, nap = 2, (0, 1), 1, 1.3, 0.5
    out = {"A": A, "pair": list(pair), "self": me, "shapes": []}
    probe = "--probe" in sys.argv[1:]
    for level in (("full-divider_salad",) if probe else ("full-divider_salad", "partial-divider_salad")):
        for B in ((1 << 20,) if probe else (1 << 18, 1 << 20)):
            env = OvercookedVecEnv(level, A, B, random_starts=capi.OC_START_AGENTS | capi.OC_START_ITEMS, seed=5)
            env.reset()
            env.team_beliefs(pair, me)
            env.partner_beliefs(pair)
            for k in range(20):  # 20 steps into the team loop
                acts, _ = env.team_actions(pair)
                env.step(acts)
                if k < 19:  # the last step's update is the one measured
                    env.team_beliefs(pair, me)
                    env.partner_beliefs(pair)
            eb, rows, S = env.batch, env._sub_rows, len(env._sub_rows)
            N, EP = S + 1, capi.event_planes(S)
            prev, cur = env._s[env._i ^ 1], env.state
            events = torch.zeros((1, EP, eb.pitch), dtype=torch.uint8, device=eb.device)
            eb.progress(prev, cur, rows, None, 1, None, events, None)
            bel, tbs, _, tmap, info = (None if t is None else t.clone() for t in env._tbelief)
            lik = torch.zeros((capi.team_lik_planes(S), eb.pitch), dtype=torch.float64, device=eb.device)
            _, p0, p1, pJ = capi.team_belief_sets(tbs, S)
            l0, l1, lJ = set_bits(p0[:, :B], N), set_bits(p1[:, :B], N), set_bits(pJ[:, :B], S)
            live_before = float((lJ.sum(0) + l0.sum(0) * l1.sum(0) - (l0 & l1).sum(0)).float().mean())
            route, nlaunch = torch_route(eb, prev, env.ex, rows, pair, me, bel, tbs, beta, nap)
            b1, s1, m1, i1 = (t.clone() for t in env._belief)
            calls = {
                "team_belief": eb.team_belief_update_launcher(prev, env.ex, rows, pair, me, bel, tbs, events, beta, nap, 0,
                                                              lik, tmap, info),
                "belief_m2": eb.belief_update_launcher(prev, env.ex, rows, pair, b1, s1, events, beta, nap, 0, m1, i1),
                "torch_route": route,
            }
            if probe:
                for _ in range(4):
                    calls["team_belief"]()
                torch.cuda.synchronize()
                print("probe done: %s, %d envs" % (level, B))
                return
            rounds = [{k: window(f) for k, f in calls.items()} for _ in range(3)]
            best = {k: min(r[k] for r in rounds) for k in calls}
            fl = info[:B]
            shape = {"level": level, "B": B, "subtasks": S, "route_launches": nlaunch, "live_hypotheses_before": live_before,
                     "belief_bytes_per_env": 8 * N * N,
                     "info_share": {k: float(((fl & v) != 0).float().mean()) for k, v in
                                    (("updated", capi.TBELF_UPDATED), ("pruned", capi.TBELF_PRUNED),
                                     ("reinit", capi.TBELF_REINIT), ("reset", capi.TBELF_RESET),
                                     ("raised", capi.TBELF_RAISED), ("empty", capi.TBELF_EMPTY), ("joint", capi.TBELF_JOINT))},
                     "ms_rounds": rounds, "ms_best": best, "ratio_a_over_b": best["team_belief"] / best["belief_m2"],
                     "ratio_a_over_c": best["team_belief"] / best["torch_route"]}
            out["shapes"].append(shape)
            print(json.dumps(shape), flush=True)
            del env, eb, route, calls
            torch.cuda.empty_cache()
    d = os.path.join(ROOT, "profiles", "teambelief")
    os.makedirs(d, exist_ok=True)
    dst = os.environ.get("TEAMBELIEF_BENCH_OUT", os.path.join(d, "teambelief_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
