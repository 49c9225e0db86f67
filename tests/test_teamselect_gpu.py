"""GPU parity of oc_team_select: the device kernel against the host call (oc_cpu_team_select, itself
pinned to the oracle-built restatement by tests/test_teamselect.py) on identical inputs: recorded
steps of the closed team loop (states and team states recorded on the host and uploaded), ragged
sizes, three and four agents, SPLIT_FIRST, the count encoding, a wide level, the
device-memory-distance builds, the 21-row table, guard columns, NULL outputs and in-place use; the
three cur planes driving oc_nav_policy; one hipGraph of the whole team step; and
OvercookedVecEnv.team_tasks / team_actions."""
import functools

import numpy as np
import pytest

import oc_testlib as tl
import teamselect_ref as mr
import test_teamselect as tt
from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oc_devlib import TeamDev as Dev  # noqa: E402
from oc_devlib import task_assert_same as assert_same  # noqa: E402

C = mr.COMMIT


@functools.lru_cache(maxsize=None)
def recorded(level, A, pair, B, steps, every, flags=C, table=None):
    """The host loop's records (no oracle check here: tests/test_teamselect.py does that)."""
    rows = None if table is None else getattr(tt, table)(level)
    lv = tl.load_level(level)
    rows = mr.level_rows(lv) if rows is None else rows
    _, rec, _ = mr.closed_loop(lv, A, pair, B, steps, flags, rows=rows, record_every=every, check=False)
    return lv, rows, rec


@pytest.mark.parametrize("B", [1, 65, 257, 4097])
def test_device_matches_host_edge_sizes(B):
    level, A, pair, _ = tt.LOOP
    lv, rows, rec = recorded(level, A, pair, B, 13, 12)
    dev = Dev(lv, A, B)
    for s, prev, fl, ts, ts_after, bound, info in rec:
        assert (ts[:, B:] == mr.GUARD_TS).all()
        assert_same(dev.call(s, prev, rows, pair, fl, ts), (ts_after, bound, info))
    s, prev, fl, ts, ts_after, bound, info = rec[1]
    # outputs NULL: the same team state
    for wb, wi in ((False, True), (True, False), (False, False)):
        assert np.array_equal(dev.call(s, prev, rows, pair, fl, ts, wb, wi)[0], ts_after)
    # in place across two consecutive calls, and the initialisation paths
    cs = CpuStepper(lv, A, B, nthreads=4)
    twice = mr.host_call(cs, s, prev, rows, pair, fl, ts_after)
    assert_same(dev.call(s, prev, rows, pair, fl, ts, times=2), twice)
    for flags in (mr.INIT | C, mr.SPLIT_FIRST, 0):
        assert_same(dev.call(s, prev, rows, pair, flags, ts), mr.host_call(cs, s, prev, rows, pair, flags, ts))
        assert_same(dev.call(s, None, rows, pair, flags, ts), mr.host_call(cs, s, None, rows, pair, flags, ts))


def test_recorded_closed_loop_steps():
    """60 steps of the issue's loop at 512 envs, every 6th step: every info bit occurs."""
    level, A, pair, B = tt.LOOP
    lv, rows, rec = recorded(level, A, pair, B, 60, 6)
    dev = Dev(lv, A, B)
    seen = 0
    for s, prev, fl, ts, ts_after, bound, info in rec:
        assert_same(dev.call(s, prev, rows, pair, fl, ts), (ts_after, bound, info))
        seen |= int(np.bitwise_or.reduce(info[:B]))
    assert seen == (mr.COMPLETED0 | mr.COMPLETED1 | mr.SWITCHED | mr.REINIT | mr.JOINT | mr.IDLE), seen


@pytest.mark.parametrize("level,A,pair,B,flags,table", [
    ("full-divider_tl", 3, (0, 2), 257, C, None), ("full-divider_salad", 4, (1, 3), 257, C, None),
    ("partial-divider_salad", 2, (0, 1), 257, C | mr.SPLIT_FIRST, None), ("levels/dup-7x7_tomato2.txt", 2, (0, 1), 257, C, None),
    ("levels/wide-17x17_salad.txt", 2, (0, 1), 129, C, None), ("levels/dense-15x17_salad.txt", 2, (0, 1), 129, C, None),
    ("levels/maze-31x31_salad.txt", 2, (0, 1), 129, C, None), ("full-divider_salad", 2, (0, 1), 257, C, "table21")])
def test_levels_and_tables(level, A, pair, B, flags, table):
    """Three and four agents with a pair that is not (0, 1), SPLIT_FIRST, the count encoding, a
    wide level (u16 cell ids, distances in device memory), a narrow level whose graph is past the
    LDS distance table (the device-memory-distance build of the narrow kernels), a maze whose BFS
    distances need u16 entries, and the 21-row table, against the host call."""
    lv, rows, rec = recorded(level, A, pair, B, 25, 6, flags, table)
    dev = Dev(lv, A, B)
    for s, prev, fl, ts, ts_after, bound, info in rec:
        assert_same(dev.call(s, prev, rows, pair, fl, ts), (ts_after, bound, info))
    EP, S = capi.event_planes(len(rows)), len(rows)
    cur = np.concatenate([r[4][EP:EP + 3, :B] for r in rec])
    assert (cur < S).any()


def test_cur_planes_drive_the_policy_launches():
    """On states with joint and split envs mixed, team_actions writes exactly the pair's bytes:
    every env is OK (or raises) in the launches its allocation names and OC_POL_BADALLOC in the
    others, a learner's bytes for the third agent and every column past B survive, and the team
    state equals the host call's on the downloaded states."""
    from gym_cooking_amd.envs import OvercookedVecEnv
    B, A, pair = 300, 3, (0, 2)
    start = capi.OC_START_AGENTS | capi.OC_START_ITEMS
    env = OvercookedVecEnv("partial-divider_salad", A, B, random_starts=start, seed=11)
    env.reset()
    rows = mr.level_rows(env.batch.level)
    S, P = len(rows), env.P
    EP = capi.event_planes(S)
    cs = CpuStepper(env.batch.level, A, B, nthreads=4)
    rng = np.random.default_rng(1)
    before = np.zeros((capi.team_planes(S), P), np.uint8)
    seen_joint = seen_split = 0
    for t in range(10):
        s = env.state.cpu().numpy()
        prev = env._s[env._i ^ 1].cpu().numpy() if t else None
        learner = rng.integers(0, 5, (A, P)).astype(np.uint8)
        learner[:, B:] = 0x77
        out = torch.from_numpy(learner.copy()).cuda().reshape(-1)
        acts, info = env.team_actions(pair, out=out)
        torch.cuda.synchronize()
        host = mr.host_call(cs, s, prev, rows, pair, C | (mr.INIT if t == 0 else 0), before)
        after = env._team.cpu().numpy()
        assert np.array_equal(after, host[0]), t
        assert np.array_equal(info.cpu().numpy(), host[2][:B]), t
        merged = out.cpu().numpy().reshape(A, P)
        assert np.array_equal(merged[1], learner[1]) and np.array_equal(merged[:, B:], learner[:, B:])
        assert (merged[[0, 2], :B] <= 4).all() and np.array_equal(acts.cpu().numpy(), merged[:, :B])
        cur = after[EP:EP + 3, :B]
        pf = env.team_flags.cpu().numpy()[:, :B]
        for q, size in enumerate((S + 1, S + 1, S)):
            mine = cur[q] < size
            assert np.isin(pf[q][mine], (capi.POL_OK, capi.POL_RAISES)).all(), (t, q)
            assert (pf[q][~mine] == capi.POL_BADALLOC).all(), (t, q)
        joint = cur[2] < S
        assert ((cur[0][joint] == mr.OUT) & (cur[1][joint] == mr.OUT)).all() and (cur[:2, ~joint] <= S).all()
        seen_joint += int(joint.sum())
        seen_split += int((~joint & ((cur[0] < S) | (cur[1] < S))).sum())
        *_, again = env.team_tasks(pair)  # a second call on the same states initialises nothing
        assert not (again.cpu().numpy() & mr.REINIT).any()
        before = env._team.cpu().numpy()
        env.step(acts)
    assert seen_joint > 0 and seen_split > 0


def test_graph_capture_and_replay():
    """team_select, the three policy launches and oc_step as one linear chain on one stream,
    captured in a hipGraph and replayed three times: the bytes of three eager runs."""
    from gym_cooking_amd.engine import OvercookedBatch
    lv, A, B, pair = tl.load_level("full-divider_salad"), 2, 4099, (0, 1)
    eb = OvercookedBatch(lv, A, B, max_T=100, device="cuda:0")
    rows = mr.level_rows(lv)
    S = len(rows)
    EP = capi.event_planes(S)
    tables = mr.policy_tables(rows, pair)
    s0 = eb.new_state()
    eb.reset_random(s0, None, 8, 0, 3)
    ts0 = eb.new_team_state(S)
    eb.team_select(s0, rows, pair, ts0, None, C | mr.INIT)
    s, ts, act = s0.clone(), ts0.clone(), eb.new_actions()
    bound = torch.zeros((2, eb.pitch), dtype=torch.float32, device="cuda:0")
    info = torch.zeros(eb.pitch, dtype=torch.uint8, device="cuda:0")
    pf = torch.zeros((3, eb.pitch), dtype=torch.uint8, device="cuda:0")
    mode = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE

    def run():  # the calls bind the current stream when they are made: inside the capture, the capturing one
        eb.team_select(s, rows, pair, ts, None, C, bound, info)
        for q, (table, ncand) in enumerate(tables):
            eb.nav_policy(s, table, act, 1.3, 0.5, mode, ts[EP + q], 3, 8, 0, None, ncand, pf[q])
        eb.step(s, s, act)

    bufs = (s, ts, act, bound, info, pf)
    init = [b.clone() for b in bufs]
    for _ in range(3):  # outside the capture first (the module load), and the eager result
        run()
    torch.cuda.synchronize()
    eager = [b.clone() for b in bufs]
    assert not torch.equal(eager[0], s0) and bool((eager[4][:B] & mr.JOINT).any())
    graph, cap = torch.cuda.CUDAGraph(), torch.cuda.Stream(device="cuda:0")
    cap.wait_stream(torch.cuda.current_stream("cuda:0"))
    with torch.cuda.graph(graph, stream=cap):
        run()
    torch.cuda.synchronize()
    for b, i in zip(bufs, init):  # the capture ran nothing: restore every buffer and replay
        b.copy_(i)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for b, e in zip(bufs, eager):
        assert torch.equal(b, e)


def test_vecenv_team_surface():
    """OvercookedVecEnv.team_tasks / team_actions over 20 steps at 4,096 envs on full-divider_salad."""
    from gym_cooking_amd.envs import OvercookedVecEnv
    B, pair = 4096, (0, 1)
    env = OvercookedVecEnv("full-divider_salad", 2, B, random_starts=capi.OC_START_AGENTS | capi.OC_START_ITEMS, seed=3)
    env.reset()
    S = len(env.subtasks)
    joint = idle = 0
    for t in range(20):
        acts, info = env.team_actions(pair)
        assert acts.shape == (2, B) and info.shape == (B,)
        i = info.cpu().numpy()
        assert ((i & mr.REINIT) != 0).all() if t == 0 else True
        joint += int(((i & mr.JOINT) != 0).sum())
        idle += int(((i & mr.IDLE) != 0).sum())
        cur0, cur1, curJ, info2 = env.team_tasks(pair)
        assert cur0.shape == cur1.shape == curJ.shape == info2.shape == (B,)
        assert np.array_equal((curJ.cpu().numpy() < S), (info2.cpu().numpy() & mr.JOINT) != 0)
        assert (acts.cpu().numpy() <= 4).all()
        env.step(acts)
    print("joint env-steps %d, idle %d of %d" % (joint, idle, 20 * B))
    assert joint > 0  # the kitchen is played jointly (a one-agent rule idles everywhere)
    assert env.episode_stats().shape == (5,)
    env.reset()
    *_, info = env.team_tasks(pair)
    assert bool(((info & mr.REINIT) != 0).all())
