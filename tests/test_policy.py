"""oc_cpu_nav_policy (the Boltzmann subtask-following action distribution and its draw) on the
host: pinned to the reference through the recorded prob_nav_actions rows of
tests/golden/likelihood.npz, checked against the oracle-built restatement tests/policy_ref.py on
random states x random planner tables in both goal-count modes, on a hand-made raising state, on
ragged batch sizes with guard bytes, and on the statistics and split-invariance of the draw."""
import functools
import os

import numpy as np
import pytest

import oc_testlib as tl
import policy_ref
from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

from oracle import oracle

pytestmark = pytest.mark.skipif(not os.path.isfile(capi.LIB_PATH), reason="liboc_engine.so not built")

BETA, NAP = 1.3, 0.5
SAMPLE, GREEDY = capi.OC_POLICY_SAMPLE, capi.OC_POLICY_GREEDY
TABLE, STATE = capi.OC_POLICY_COUNT_TABLE, capi.OC_POLICY_COUNT_STATE
# (level, A, B, seed, one-agent table) and the issue's floors: OK rows, joint OK rows, goal-reaching rows
CASES = [("open-divider_salad", 2, 3000, 90, False, 2000, 1000, 100),
         ("full-divider_salad", 4, 9000, 41, False, 6000, 1000, 100),
         ("partial-divider_salad", 2, 4000, 87, True, 2500, 0, 100)]


@functools.lru_cache(maxsize=None)
def case(i: int):
    """(ob, state, subtasks, alloc, num_cand) of random case i; shared, never modified."""
    import test_rollout_host as th
    level, A, B, seed, single = CASES[i][:5]
    ob, s, _, subs, alloc = th.random_rollout_case(level, A, B, seed=seed)
    if single:
        subs = [capi.subtask(x.kind, [x.agent[0]], list(x.start_mask), x.goal_mask, x.goal_count) for x in subs]
    return ob, s, subs, alloc, 5 if single else 25


@functools.lru_cache(maxsize=None)
def reference(i: int, count_state: bool):
    ob, s, subs, alloc, _ = case(i)
    return policy_ref.distribution(ob, s, subs, alloc, BETA, NAP, count_state)


def host_policy(level, A, B, s, subs, alloc, mode, num_cand=25, step=0, seed=0, env_offset=0, actions=None,
                want_probs=True, beta=BETA):
    """(actions [A, P], probs [num_cand, P] or None, flags [P]) of oc_cpu_nav_policy; outputs prefilled
    with guard bytes (0xEE actions, 0xA5 flags, NaN-pattern probs)."""
    cs = CpuStepper(level, A, B, nthreads=4)
    P = cs.pitch
    act = np.full(A * P, 0xEE, np.uint8) if actions is None else actions.copy()
    probs = np.full(num_cand * P, np.nan) if want_probs else None
    flags = np.full(P, 0xA5, np.uint8)
    cs.nav_policy(s, subs, act, beta, NAP, mode, alloc, step, seed, env_offset, probs, num_cand, flags)
    return act.reshape(A, P), None if probs is None else probs.reshape(num_cand, P), flags


def check_untouched(act, probs, flags, ref, A, P, B):
    """Nothing outside the contract changed: columns >= B, the other agents' bytes, BADALLOC rows."""
    assert (act[:, B:] == 0xEE).all() and (flags[B:] == 0xA5).all()
    if probs is not None:
        assert np.isnan(probs[:, B:]).all()
    touched = np.zeros((A, B), bool)
    live = ~ref["bad"]
    touched[ref["agent0"][live], np.nonzero(live)[0]] = True
    j = live & ref["joint"]
    touched[ref["agent1"][j], np.nonzero(j)[0]] = True
    assert (act[:, :B][~touched] == 0xEE).all()
    assert (act[:, :B][touched] <= 4).all()


def assert_matches_restatement(ob, s, subs, alloc, nc, ref, count_state):
    """oc_cpu_nav_policy on a case against `ref` (policy_ref.distribution of it in that count
    mode): flags, support, probabilities, the bytes nobody may touch, the GREEDY actions, and the
    SAMPLE draw replayed from the returned probabilities.  Returns the replayed picks (-1 where the
    row is not POL_OK)."""
    A, B, P = ob.A, ob.B, ob.pitch
    ok = ref["flags"] == capi.POL_OK
    cmode = STATE if count_state else TABLE
    act_g, probs, flags = host_policy(ob.level, A, B, s, subs, alloc, GREEDY | cmode, nc)
    assert np.array_equal(flags[:B], ref["flags"]), np.argwhere(flags[:B] != ref["flags"])[:5]
    assert np.array_equal(probs[:, :B] > 0, ref["probs"][:nc] > 0)
    np.testing.assert_allclose(probs[:, :B], ref["probs"][:nc], rtol=1e-12, atol=0)
    assert (probs[:, :B][:, ~ok] == 0).all()
    check_untouched(act_g, probs, flags, ref, A, P, B)
    before = np.full(A * P, 0xEE, np.uint8)
    assert np.array_equal(act_g, policy_ref.expected_actions(ref, ref["greedy"], before, A, P, B))
    # SAMPLE: the replay of the draw from the returned probs and the specified u, exactly
    act_s, probs_s, flags_s = host_policy(ob.level, A, B, s, subs, alloc, SAMPLE | cmode, nc, step=7, seed=1234,
                                          env_offset=5)
    assert np.array_equal(flags_s, flags) and np.array_equal(probs_s[:, :B], probs[:, :B])
    pick = np.full(B, -1)
    for e in np.nonzero(ok)[0]:
        u = policy_ref.draw_u(1234, 5 + int(e), 7, int(ref["agent0"][e]))
        pick[e] = policy_ref.replay_draw(probs_s[:, e], int(ref["ncand"][e]), u)
    assert np.array_equal(act_s, policy_ref.expected_actions(ref, pick, before, A, P, B))
    return pick


@pytest.mark.parametrize("count_state", [False, True])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_random_cases_match_oracle_restatement(i, count_state):
    ob, s, subs, alloc, nc = case(i)
    ref = reference(i, count_state)
    ok = ref["flags"] == capi.POL_OK
    _, _, _, _, _, min_ok, min_joint, min_goal = CASES[i]
    # the conditions of the issue, counted with the oracle alone
    assert ok.sum() >= min_ok and (ok & ref["joint"]).sum() >= min_joint
    assert ((ref["probs"] > 0).sum(0)[ok] >= 2).all()
    if not count_state:
        assert ref["goal_reach"].sum() >= min_goal
    pick = assert_matches_restatement(ob, s, subs, alloc, nc, ref, count_state)
    assert len(np.unique(pick[ok])) >= 4  # the draw spreads over the candidates


def test_count_modes_differ_somewhere():
    """COUNT_STATE is a different goal test from COUNT_TABLE (random goal_count 0..2)."""
    a, b = reference(1, False), reference(1, True)
    both = (a["flags"] == capi.POL_OK) & (b["flags"] == capi.POL_OK)
    assert (np.abs(a["probs"] - b["probs"])[:, both] > 1e-6).any()


def _likelihood_groups():
    fx = tl.load_fixture("likelihood.npz")
    return fx, [(c, sa) for c in range(4) for sa in (0, 1)]


@pytest.mark.parametrize("cfg", range(4))
@pytest.mark.parametrize("self_agent", [0, 1])
def test_recorded_prob_nav_actions_rows(cfg, self_agent):
    """probs[taken] against the reference's recorded prob_nav_actions: equal where the self agent
    is outside a joint pair or the row has one agent; where it is in the pair, probs[taken] over
    the sum of the candidates that keep the other agent's action.  rtol 1e-10 (the two forms
    round beta * Q differently).  None rows use the acting agent as the self agent, so only the
    None rows of the self agent itself compare."""
    fx = tl.load_fixture("likelihood.npz")
    rows = tl.LikelihoodRows(fx, cfg, self_agent)
    assert rows.B > 0
    compared = 0
    for sel, alloc, subs in rows.chunks(capi.MAX_SUBTASKS):
        B = len(sel)
        P = capi.pitch_for(B)
        s, taken = rows.inputs(sel, P)
        taken = taken.reshape(rows.A, P)
        a = np.zeros(P, np.uint8)
        a[:B] = alloc
        _, probs, flags = host_policy(rows.level, rows.A, B, s, subs, a, GREEDY | TABLE, 25, beta=rows.beta)
        for r, g in enumerate(sel):
            st = subs[alloc[r]]
            ags = [st.agent[q] for q in range(st.num_agents)]
            t = [min(int(taken[q, r]), 4) for q in ags]
            if st.kind == capi.SUB_NONE and (st.num_agents != 1 or ags[0] != self_agent):
                continue
            k = t[0] * 5 + t[1] if len(ags) == 2 else t[0]
            if rows.exp_raised[g]:
                # the reference raised: the policy raises too, unless only the taken action was illegal
                assert flags[r] == capi.POL_RAISES or probs[k, r] == 0.0 or st.kind == capi.SUB_NONE, g
                continue
            assert flags[r] == capi.POL_OK, (g, flags[r])
            v = probs[k, r]
            if st.kind == capi.SUB_NONE and k != 4:
                # the reference scores any taken move as one movable action's share, legal or not
                v = probs[:4, r].max()
            if len(ags) == 2 and self_agent in ags:
                keep = 1 - ags.index(self_agent)  # the other agent's action stays
                ks = [c for c in range(25) if (c // 5, c % 5)[keep] == t[keep]]
                v = v / sum(probs[c, r] for c in ks)
            assert abs(v - rows.exp_value[g]) <= 1e-10 * abs(rows.exp_value[g]), (g, v, rows.exp_value[g])
            compared += 1
    assert compared > 100


def test_colocated_removed_agents_raise():
    """A hand-made A = 3 state with agents 1 and 2 on one Floor cell and a one-agent configuration
    of agent 0: the reference raises removing the second agent (OC_ROLL_RAISES in the oracle)."""
    lv = tl.load_level("open-divider_salad")
    ob = oracle.OracleBatch(lv, 3, 100, 1)
    s = ob.new_state()
    ob.reset(s)
    v = tl.planes_view(s, 3, ob.K, ob.pitch)
    v["ax"][2, 0], v["ay"][2, 0] = v["ax"][1, 0], v["ay"][1, 0]
    subs = [capi.subtask(capi.SUB_CHOP, [0], [0x01, 0], 0x11, 0)]
    fl, _ = ob.rollout(s, ob.new_state(), ob.new_actions(), subs, None)
    assert fl[0] == capi.ROLL_RAISES
    act, probs, flags = host_policy(lv, 3, 1, s, subs, None, SAMPLE | STATE, 5)
    assert flags[0] == capi.POL_RAISES and act[0, 0] == 4 and (probs[:, 0] == 0).all()
    assert (act[1:, 0] == 0xEE).all() and (act[:, 1:] == 0xEE).all() and (flags[1:] == 0xA5).all()


@pytest.mark.parametrize("B", [1, 7, 9, 4097])
def test_edges_ragged_sizes_badalloc_and_guards(B):
    import test_rollout_host as th
    ob, s, _, subs, alloc = th.random_rollout_case("open-divider_salad", 2, B, seed=11 + B)
    alloc = alloc.copy()
    alloc[::5] = len(subs) + 3  # BADALLOC rows
    ref = policy_ref.distribution(ob, s, subs, alloc, BETA, NAP, True)
    assert ref["bad"][0]
    for mode in (GREEDY | STATE, SAMPLE | STATE):
        act, probs, flags = host_policy(ob.level, 2, B, s, subs, alloc, mode, 25, step=3, seed=9)
        assert np.array_equal(flags[:B], ref["flags"])
        check_untouched(act, probs, flags, ref, 2, ob.pitch, B)
        np.testing.assert_allclose(probs[:, :B], ref["probs"], rtol=1e-12, atol=0)
        assert (probs[:, :B][:, ref["bad"]] == 0).all()
    # probs NULL: the same actions and flags
    act2, _, flags2 = host_policy(ob.level, 2, B, s, subs, alloc, SAMPLE | STATE, 25, step=3, seed=9, want_probs=False)
    assert np.array_equal(act2, act) and np.array_equal(flags2, flags)
    # a one-agent table in a 25-candidate call: planes 5.. are zero
    single = [capi.subtask(x.kind, [x.agent[0]], list(x.start_mask), x.goal_mask, x.goal_count) for x in subs]
    _, p25, f25 = host_policy(ob.level, 2, B, s, single, alloc, GREEDY | STATE, 25)
    _, p5, f5 = host_policy(ob.level, 2, B, s, single, alloc, GREEDY | STATE, 5)
    assert np.array_equal(f25, f5) and np.array_equal(p25[:5, :B], p5[:, :B]) and (p25[5:, :B] == 0).all()


def test_bad_arguments():
    import test_rollout_host as th
    ob, s, _, subs, alloc = th.random_rollout_case("open-divider_salad", 2, 64, seed=5)
    joint = [capi.subtask(capi.SUB_CHOP, [0, 1], [0x01, 0], 0x11, 0)]
    cs = CpuStepper(ob.level, 2, 64)
    act, fl = np.zeros(2 * cs.pitch, np.uint8), np.zeros(cs.pitch, np.uint8)
    args = lambda table, nc, mode=0: (cs._h, s.ctypes.data, None, capi.subtask_array(table), len(table), BETA, NAP,  # noqa: E731
                                      mode, 0, 0, 0, act.ctypes.data, None, nc, fl.ctypes.data, 64, 1)
    assert cs.lib.oc_cpu_nav_policy(*args(joint, 5)) == capi.OC_EINVAL
    assert b"num_cand 5" in cs.lib.oc_last_error()
    assert cs.lib.oc_cpu_nav_policy(*args(joint, 7)) == capi.OC_EINVAL
    assert cs.lib.oc_cpu_nav_policy(*args(joint, 25, 4)) == capi.OC_EINVAL
    assert cs.lib.oc_cpu_nav_policy(*args(joint, 25)) == 0
    l1 = [capi.subtask(capi.SUB_CHOP, [0], [0x01, 0], 0x11, 0, 1)]
    assert cs.lib.oc_cpu_nav_policy(*args(l1, 5)) == capi.OC_EINVAL
    # the device call refuses a host-only handle
    dev = (cs._h, s.ctypes.data, None, capi.subtask_array(joint), 1, BETA, NAP, 0, 0, 0, 0, act.ctypes.data, None, 25,
           fl.ctypes.data, 64, None)
    assert cs.lib.oc_nav_policy(*dev) == capi.OC_EINVAL and b"host-only handle" in cs.lib.oc_last_error()


def test_sampling_frequencies_and_split_invariance():
    """2^16 copies of one mid-episode state at step 0: every candidate with p >= 0.01 is drawn with
    a frequency within 6 sigma of p; and the bytes depend on (seed, step, gid) only, whatever
    env_offset split of the batch computes them."""
    ob, s, subs, alloc, _ = case(0)
    ref = reference(0, True)
    e = int(np.nonzero((ref["flags"] == capi.POL_OK) & ref["joint"] & ((ref["probs"] >= 0.01).sum(0) >= 4))[0][0])
    N = 1 << 16
    P0, A = ob.pitch, ob.A
    one = s.reshape(-1, P0)[:, e]
    sN = np.repeat(one[:, None], N, 1).reshape(-1).copy()  # pitch == N
    table = [subs[alloc[e]]]
    act, probs, flags = host_policy(ob.level, A, N, sN, table, None, SAMPLE | STATE, 25, step=0, seed=77)
    assert (flags == capi.POL_OK).all()
    p = probs[:, 0]
    np.testing.assert_allclose(p, ref["probs"][:, e], rtol=1e-12, atol=0)
    a0, a1 = table[0].agent[0], table[0].agent[1]
    k = act[a0].astype(np.int64) * 5 + act[a1]
    freq = np.bincount(k, minlength=25) / N
    for c in range(25):
        if p[c] >= 0.01:
            assert abs(freq[c] - p[c]) <= 6 * np.sqrt(p[c] * (1 - p[c]) / N), (c, freq[c], p[c])
    assert (freq[p == 0] == 0).all()
    # the same rows computed as two halves with their env_offset
    H = N // 2
    for off in (0, H):
        half = sN.reshape(-1, N)[:, off:off + H]
        sh = np.zeros((half.shape[0], capi.pitch_for(H)), np.uint8)
        sh[:, :H] = half
        ah, _, _ = host_policy(ob.level, A, H, sh.reshape(-1), table, None, SAMPLE | STATE, 25, step=0, seed=77,
                               env_offset=off, want_probs=False)
        assert np.array_equal(ah[:, :H], act[:, off:off + H])


def test_host_sanitizer_program():
    """tests/policy_host: the host row function under ASan + UBSan in a stand-alone program."""
    import shutil
    import subprocess
    d = os.path.join(tl.ROOT, "tests", "policy_host")
    if not os.path.isfile("/opt/rocm/llvm/bin/clang++") and shutil.which("clang++") is None:
        pytest.skip("no clang++ for the sanitizer build")
    r = subprocess.run(["make", "-s", "-C", d], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "clean" in r.stdout
