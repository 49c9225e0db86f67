"""GPU parity of oc_task_select: the device kernel against the host call (oc_cpu_task_select, itself
pinned to the oracle-built restatement by tests/test_taskselect.py) on identical inputs: the
recorded steps of the closed scripted-partner loop, ragged sizes, a wide and a u16-distance level,
the 64-configuration and the 63-subtask tables, guard columns; and OvercookedVecEnv.partner_tasks /
scripted_actions against the host call step by step."""
import functools

import numpy as np
import pytest

import oc_testlib as tl
import taskselect_ref as tr
import test_taskselect as tt
from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oc_devlib import TaskDev as Dev, task_assert_same as assert_same  # noqa: E402

CD = tr.COMMIT | tr.DISTINCT


@functools.lru_cache(maxsize=None)
def recorded(level, A, agents, B, steps, every, table=None):
    """The host loop's records (no oracle check here: tests/test_taskselect.py does that)."""
    rows = None if table is None else getattr(tt, table)(level)
    lv = tl.load_level(level)
    rows = tr.level_rows(lv) if rows is None else rows
    _, rec = tr.closed_loop(lv, A, agents, B, steps, CD, rows=rows, record_every=every, check=False)
    return lv, rows, rec


def test_recorded_closed_loop_steps():
    level, A, agents, B = tt.LOOP
    lv, rows, rec = recorded(level, A, agents, B, 200, 10)
    assert len(rec) == 20
    dev = Dev(lv, A, B)
    seen = 0
    for s, prev, fl, ts, ts_after, bound, info in rec:
        assert_same(dev.call(s, prev, rows, agents, fl, ts), (ts_after, bound, info))
        seen |= int(np.bitwise_or.reduce(info[:, :B].reshape(-1)))
    assert seen == tr.COMPLETED | tr.SWITCHED | tr.REINIT  # every info bit occurs in the records


@pytest.mark.parametrize("B", [1, 7, 9, 65, 257, 4097])
def test_device_matches_host_edge_sizes(B):
    level, A, agents, _ = tt.LOOP
    lv, rows, rec = recorded(level, A, agents, B, 13, 12)
    s, prev, fl, ts, ts_after, bound, info = rec[1]
    assert (ts[:, :, B:] == tr.GUARD_TS).all()
    dev = Dev(lv, A, B)
    assert_same(dev.call(s, prev, rows, agents, fl, ts), (ts_after, bound, info))
    # outputs NULL: the same task state; OC_TASK_INIT over a state_prev
    for wb, wi in ((False, True), (True, False), (False, False)):
        assert np.array_equal(dev.call(s, prev, rows, agents, fl, ts, wb, wi)[0], ts_after)
    cs = CpuStepper(lv, A, B, nthreads=4)
    for flags in (tr.INIT | CD, tr.COMMIT, 0):
        assert_same(dev.call(s, prev, rows, agents, flags, ts), tr.host_call(cs, s, prev, rows, agents, flags, ts))
        assert_same(dev.call(s, None, rows, agents, flags, ts), tr.host_call(cs, s, None, rows, agents, flags, ts))


@pytest.mark.parametrize("level,A,agents,B,table", [
    ("levels/wide-17x17_salad.txt", 2, (0, 1), 500, None), ("levels/maze-31x31_salad.txt", 2, (0, 1), 300, None),
    ("full-divider_salad", 4, (0, 1, 2, 3), 257, "table16"), ("open-divider_salad", 2, (1,), 257, "table63"),
    ("partial-divider_salad", 3, (2, 0), 257, None), ("levels/dup-7x7_tomato2.txt", 2, (0, 1), 257, None)])
def test_levels_and_tables(level, A, agents, B, table):
    """A wide level (u16 cell ids, distances in device memory), a maze whose BFS distances need u16
    entries, the 4 x 16 = 64-configuration table, 63 subtasks, a priority order that is not the
    index order, and the count encoding, against the host call."""
    lv, rows, rec = recorded(level, A, agents, B, 25, 6, table)
    dev = Dev(lv, A, B)
    for s, prev, fl, ts, ts_after, bound, info in rec:
        assert_same(dev.call(s, prev, rows, agents, fl, ts), (ts_after, bound, info))
    cur = rec[-1][4][:, capi.event_planes(len(rows)), :B]
    assert (cur < len(rows)).any()


def test_vecenv_scripted_partners():
    """40 steps of scripted_actions((0, 1)) -> step: after every partner_tasks the downloaded
    (state, state before, task state before) fed to the host call gives the same planes; some env
    delivers (a whole salad takes the two partners 30 to 46 steps from a random start; with seed 27
    the host loop, which makes the same draws, delivers in three envs, first at step 30).  With agents
    (1,) a learner's bytes for agent 0 survive."""
    from gym_cooking_amd.envs import OvercookedVecEnv
    B, A, agents = 300, 2, (0, 1)
    start = capi.OC_START_AGENTS | capi.OC_START_ITEMS
    env = OvercookedVecEnv("open-divider_salad", A, B, random_starts=start, seed=27)
    env.reset()
    rows = tr.level_rows(env.batch.level)
    cs = CpuStepper(env.batch.level, A, B, nthreads=4)
    S, P = len(rows), env.P
    EP = capi.event_planes(S)
    before = np.zeros((2, capi.task_planes(S), P), np.uint8)
    success = 0
    for t in range(40):
        s = env.state.cpu().numpy()
        prev = env._s[env._i ^ 1].cpu().numpy() if t else None
        acts, info = env.scripted_actions(agents)
        torch.cuda.synchronize()
        host = tr.host_call(cs, s, prev, rows, agents, CD | (tr.INIT if t == 0 else 0), before)
        after = env._task.cpu().numpy()
        assert np.array_equal(after, host[0]), t
        assert np.array_equal(info.cpu().numpy(), host[2][:, :B]), t
        cur, _ = env.partner_tasks(agents)  # a second call on the same states changes nothing but SWITCHED / COMPLETED
        assert np.array_equal(cur.cpu().numpy(), after[:, EP, :B])
        assert (acts.cpu().numpy() <= 4).all()
        before = env._task.cpu().numpy()
        _, reward, _, _ = env.step(acts)
        success += int(reward.sum())
    assert success >= 1
    # one scripted agent: the learner's bytes stay
    env = OvercookedVecEnv("open-divider_salad", A, B, random_starts=start, seed=27)
    env.reset()
    learner = np.random.default_rng(1).integers(0, 5, (A, P)).astype(np.uint8)
    out = torch.from_numpy(learner.copy()).cuda().reshape(-1)
    acts, info = env.scripted_actions((1,), out=out)
    torch.cuda.synchronize()
    merged = out.cpu().numpy().reshape(A, P)
    assert np.array_equal(merged[0], learner[0]) and np.array_equal(merged[1, B:], learner[1, B:])
    assert (merged[1, :B] <= 4).all() and np.array_equal(acts.cpu().numpy(), merged[:, :B])
    assert (info.cpu().numpy() & tr.REINIT).all() and info.shape == (1, B)
