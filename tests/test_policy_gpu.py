"""GPU parity of oc_nav_policy: the device kernel against the host call (oc_cpu_nav_policy, itself
pinned to the oracle and the reference rows by tests/test_policy.py) on the random cases, ragged
sizes, a wide and a u16-distance level; the recorded prob_nav_actions rows; the device likelihood
as a cross-check; and OvercookedVecEnv.partner_actions merged with a learner's actions."""
import numpy as np
import pytest

import oc_testlib as tl
import policy_ref
import test_policy as tp
from gym_cooking_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MODES = [m | c for m in (tp.GREEDY, tp.SAMPLE) for c in (tp.TABLE, tp.STATE)]


def gpu_policy(level, A, B, s, subs, alloc, mode, num_cand=25, step=0, seed=0, env_offset=0, want_probs=True,
               beta=tp.BETA):
    """As test_policy.host_policy, through oc_nav_policy: guard-filled outputs, numpy results."""
    from gym_cooking_amd.engine import OvercookedBatch
    eb = OvercookedBatch(level, A, B, max_T=100, device="cuda:0")
    P = eb.pitch
    act = torch.full((A * P,), 0xEE, dtype=torch.uint8, device="cuda:0")
    probs = torch.full((num_cand * P,), float("nan"), dtype=torch.float64, device="cuda:0") if want_probs else None
    flags = torch.full((P,), 0xA5, dtype=torch.uint8, device="cuda:0")
    a = torch.from_numpy(alloc).cuda() if alloc is not None else None
    eb.nav_policy(torch.from_numpy(s).cuda(), subs, act, beta, tp.NAP, mode, a, step, seed, env_offset, probs, num_cand,
                  flags)
    torch.cuda.synchronize()
    return (act.cpu().numpy().reshape(A, P), None if probs is None else probs.cpu().numpy().reshape(num_cand, P),
            flags.cpu().numpy())


def assert_same(dev, host, B):
    (da, dp, df), (ha, hp, hf) = dev, host
    assert np.array_equal(df, hf), np.argwhere(df != hf)[:5]
    assert np.array_equal(da, ha), np.argwhere(da != ha)[:5]
    assert np.array_equal(np.isnan(dp), np.isnan(hp))  # the guard columns past B, untouched
    np.testing.assert_allclose(dp[:, :B], hp[:, :B], rtol=1e-12, atol=0)


@pytest.mark.parametrize("i", range(len(tp.CASES)))
def test_device_matches_host_random_cases(i):
    ob, s, subs, alloc, nc = tp.case(i)
    for mode in MODES:
        kw = dict(step=7, seed=1234, env_offset=5)
        dev = gpu_policy(ob.level, ob.A, ob.B, s, subs, alloc, mode, nc, **kw)
        host = tp.host_policy(ob.level, ob.A, ob.B, s, subs, alloc, mode, nc, **kw)
        assert (host[2][:ob.B] == capi.POL_OK).sum() > 2000
        assert_same(dev, host, ob.B)


@pytest.mark.parametrize("B", [1, 7, 9, 4097])
def test_device_matches_host_edge_sizes(B):
    import test_rollout_host as th
    ob, s, _, subs, alloc = th.random_rollout_case("open-divider_salad", 2, B, seed=11 + B)
    alloc = alloc.copy()
    alloc[::5] = len(subs) + 3
    for mode in MODES:
        dev = gpu_policy(ob.level, 2, B, s, subs, alloc, mode, 25, step=3, seed=9)
        assert_same(dev, tp.host_policy(ob.level, 2, B, s, subs, alloc, mode, 25, step=3, seed=9), B)
    dev = gpu_policy(ob.level, 2, B, s, subs, alloc, tp.SAMPLE | tp.STATE, 25, step=3, seed=9, want_probs=False)
    host = tp.host_policy(ob.level, 2, B, s, subs, alloc, tp.SAMPLE | tp.STATE, 25, step=3, seed=9, want_probs=False)
    assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[2], host[2])
    # a one-agent table (8-lane groups) writing 25 planes
    single = [capi.subtask(x.kind, [x.agent[0]], list(x.start_mask), x.goal_mask, x.goal_count) for x in subs]
    for nc in (5, 25):
        assert_same(gpu_policy(ob.level, 2, B, s, single, alloc, tp.SAMPLE | tp.STATE, nc, seed=3),
                    tp.host_policy(ob.level, 2, B, s, single, alloc, tp.SAMPLE | tp.STATE, nc, seed=3), B)


@pytest.mark.parametrize("level,A,B", [("levels/wide-17x17_salad.txt", 2, 500), ("levels/maze-31x31_salad.txt", 2, 300)])
def test_wide_and_u16_distance_levels(level, A, B):
    """A wide level (u16 cell ids, distances in device memory) and a maze whose BFS distances need
    u16 entries, against the host call."""
    import test_rollout_host as th
    ob, s, _, subs, alloc = th.random_rollout_case(_path(level), A, B, seed=B)
    for mode in (tp.GREEDY | tp.STATE, tp.SAMPLE | tp.TABLE):
        dev = gpu_policy(ob.level, A, B, s, subs, alloc, mode, 25, step=1, seed=2)
        host = tp.host_policy(ob.level, A, B, s, subs, alloc, mode, 25, step=1, seed=2)
        assert (host[2][:B] == capi.POL_OK).sum() > B // 2
        assert_same(dev, host, B)


def _path(name):
    import os
    return os.path.join(tl.GOLDEN, name)


@pytest.mark.parametrize("cfg", range(4))
def test_recorded_rows_and_device_likelihood(cfg):
    """The recorded prob_nav_actions rows on the device (as test_policy's CPU test), and
    probs[taken] against oc_nav_likelihood with a self agent outside the pair or on one-agent
    configurations (rtol 1e-10)."""
    from gym_cooking_amd.engine import OvercookedBatch
    fx = tl.load_fixture("likelihood.npz")
    compared = crossed = 0
    for self_agent in (0, 1):
        rows = tl.LikelihoodRows(fx, cfg, self_agent)
        for sel, alloc, subs in rows.chunks(capi.MAX_SUBTASKS):
            B = len(sel)
            P = capi.pitch_for(B)
            s, taken = rows.inputs(sel, P)
            a = np.zeros(P, np.uint8)
            a[:B] = alloc
            _, probs, flags = gpu_policy(rows.level, rows.A, B, s, subs, a, tp.GREEDY | tp.TABLE, 25, beta=rows.beta)
            eb = OvercookedBatch(rows.level, rows.A, B, max_T=100, device="cuda:0")
            lv, lf = eb.nav_likelihood(torch.from_numpy(s).cuda(), torch.from_numpy(taken).cuda(), subs, self_agent,
                                       rows.beta, rows.nap, torch.from_numpy(a).cuda())
            lv, lf = lv.cpu().numpy(), lf.cpu().numpy()
            tk = taken.reshape(rows.A, P)
            for r, g in enumerate(sel):
                st = subs[alloc[r]]
                ags = [st.agent[q] for q in range(st.num_agents)]
                t = [min(int(tk[q, r]), 4) for q in ags]
                if st.kind == capi.SUB_NONE and (st.num_agents != 1 or ags[0] != self_agent):
                    continue
                k = t[0] * 5 + t[1] if len(ags) == 2 else t[0]
                if rows.exp_raised[g] or flags[r] != capi.POL_OK:
                    assert rows.exp_raised[g] and (flags[r] == capi.POL_RAISES or probs[k, r] == 0.0
                                                   or st.kind == capi.SUB_NONE), g
                    continue
                v = probs[k, r]
                if st.kind == capi.SUB_NONE and k != 4:
                    v = probs[:4, r].max()
                inside = len(ags) == 2 and self_agent in ags
                if inside:
                    keep = 1 - ags.index(self_agent)
                    v = v / sum(probs[c, r] for c in range(25) if (c // 5, c % 5)[keep] == t[keep])
                elif lf[r] == capi.LIK_OK:
                    assert abs(probs[k, r] - lv[r]) <= 1e-10 * abs(lv[r]) or st.kind == capi.SUB_NONE, (g, probs[k, r], lv[r])
                    crossed += 1
                assert abs(v - rows.exp_value[g]) <= 1e-10 * abs(rows.exp_value[g]), (g, v, rows.exp_value[g])
                compared += 1
    assert compared > 200 and crossed > 100


def test_vecenv_partner_actions_merge_and_step():
    """partner_actions writes only the partner's bytes into a buffer that already holds a learner's
    random actions; the merged planes step bit-equal to the oracle stepping the same planes."""
    from gym_cooking_amd.envs import OvercookedVecEnv
    from oracle import oracle
    B, A = 4096, 2
    env = OvercookedVecEnv("partial-divider_salad", A, B, seed=3)
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(6):  # a few random steps: mid-episode states
        env.step(torch.from_numpy(rng.integers(0, 5, (A, B)).astype(np.uint8)).cuda())
    table = capi.policy_subtasks(env.subtasks, env.batch.level.encoding, [1])
    assert len(table) == len(env.subtasks) > 0
    alloc = torch.from_numpy(rng.integers(0, len(table), env.P).astype(np.uint8)).cuda()
    learner = rng.integers(0, 5, (A, env.P)).astype(np.uint8)
    out = torch.from_numpy(learner.copy()).cuda().reshape(-1)
    acts, flags = env.partner_actions(table, alloc, out=out)
    torch.cuda.synchronize()
    merged = out.cpu().numpy().reshape(A, env.P)
    assert (flags.cpu().numpy() == capi.POL_OK).all()
    assert np.array_equal(merged[0], learner[0]) and np.array_equal(merged[1, B:], learner[1, B:])
    assert (merged[1, :B] <= 4).all() and len(np.unique(merged[1, :B])) >= 3
    assert np.array_equal(acts.cpu().numpy(), merged[:, :B])
    s0 = env.state.cpu().numpy()
    env.step(out)
    torch.cuda.synchronize()
    ob = oracle.OracleBatch(env.batch.level, A, 100, B)
    o1 = ob.new_state()
    ob.step(s0, o1, merged.reshape(-1))
    g1 = env.state.cpu().numpy()
    assert np.array_equal(tl.env_view(g1, A, ob.K, ob.pitch, B), tl.env_view(o1, A, ob.K, ob.pitch, B))
