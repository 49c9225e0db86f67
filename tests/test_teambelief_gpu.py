"""GPU parity of oc_team_belief_update: the device kernel against the host call
(oc_cpu_team_belief_update, itself pinned to the reference fixture and to the numpy restatement by
tests/test_teambelief.py) on identical inputs: the recorded calls of the closed team loops, ragged
sizes with guard columns, a size past one round of the grid (the launch has at most 8 blocks of 32
lane groups per CU: 65,536 envs per round on 256 CUs), one small loop on every (A >= 2, K, layout)
cell of the planner dispatch grid, INIT with NULL inputs, a captured graph; and
OvercookedVecEnv.team_beliefs / delegate_actions against the batch-level calls."""
import functools

import numpy as np
import pytest

import oc_testlib as tl
import teambelief_ref as tb
import teamselect_ref as tsr
import test_plan_grid as pg
import test_teambelief as tt
from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


class Dev:
    """oc_team_belief_update on guard-filled device buffers, numpy in and out (as teambelief_ref.host_call)."""

    def __init__(self, level, A, B):
        from gym_cooking_amd.engine import OvercookedBatch
        self.eb = OvercookedBatch(level, A, B, max_T=100, device="cuda:0")

    def launcher(self, prev, taken, events, rows, pair, me, flags, bel, ts, want_lik=True, want_map=True, want_info=True):
        P, S = self.eb.pitch, len(rows)
        up = lambda a: None if a is None else torch.from_numpy(a).cuda()  # noqa: E731
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda:0")  # noqa: E731
        dbel, dts = up(bel), up(ts)
        lik = full((capi.team_lik_planes(S), P), tb.GUARD_LIK, torch.float64) if want_lik else None
        amap = full((3, P), tb.GUARD_MAP, torch.uint8) if want_map else None
        info = full((P,), tb.GUARD_INFO, torch.uint8) if want_info else None
        launch = self.eb.team_belief_update_launcher(up(prev), up(taken), rows, pair, me, dbel, dts, up(events), 1.3, 0.5,
                                                     flags, lik, amap, info)
        return launch, (dbel, dts, lik, amap, info)

    def call(self, *args, **kw):
        launch, out = self.launcher(*args, **kw)
        launch()
        torch.cuda.synchronize()
        return tuple(None if t is None else t.cpu().numpy() for t in out)


def assert_same(dev, host, S, B, where=""):
    """tbstate, info and the guard columns byte for byte, beliefs and lik to 1e-12 (exp, fused
    multiply-adds and the order of the normalising sum differ in their last bits), map against the
    device's own beliefs."""
    dbel, dts, dlik, dmap, dinfo = dev
    hbel, hts, hlik, _, hinfo = host
    assert np.array_equal(dts, hts), (where, np.argwhere(dts != hts)[:5])
    if dinfo is not None:
        # OC_TBELF_JOINT says what the map is, and the map is the call's own beliefs' (a joint and a
        # split can be one ulp apart: L0_i + L1_j against 2 LJ_t): that bit against the device's map
        rest = 0xFF & ~tb.JOINT
        assert np.array_equal(dinfo & rest, hinfo & rest), (where, np.argwhere((dinfo & rest) != (hinfo & rest))[:5])
        assert np.array_equal((dinfo[:B] & tb.JOINT) != 0, tb.map_of(dbel, dts, S, B)[2] < S), where
        assert np.array_equal(dinfo[B:], hinfo[B:]), where
    assert tb.close(dbel[:, :B], hbel[:, :B]), (where, np.abs(dbel[:, :B] - hbel[:, :B]).max())
    assert np.array_equal(dbel[:, B:].view(np.uint64), hbel[:, B:].view(np.uint64)), where
    if dlik is not None:
        ran = (hinfo[:B] & tb.UPDATED) != 0
        assert tb.close(dlik[:, :B][:, ran], hlik[:, :B][:, ran]), where
        assert (dlik[:, :B][:, ~ran] == tb.GUARD_LIK).all() and (dlik[:, B:] == tb.GUARD_LIK).all(), where
    if dmap is not None:
        assert np.array_equal(dmap[:, :B], tb.map_of(dbel, dts, S, B)), where
        assert (dmap[:, B:] == tb.GUARD_MAP).all(), where


@functools.lru_cache(maxsize=None)
def recorded(level, A, pair, B, steps, every, selfs=None, max_T=100):
    """The host loop's records (no restatement check here: tests/test_teambelief.py does that)."""
    lv = tl.load_level(level)
    rows = tsr.level_rows(lv)
    _, rec = tb.closed_loop(lv, A, pair, B, steps, record_every=every, check=False, selfs=selfs, max_T=max_T)
    return lv, rows, rec


def replay(dev, rows, pair, rec, B):
    seen = 0
    for me, calls in rec.items():
        for i, (prev, taken, events, fl, bel, ts, *after) in enumerate(calls):
            got = dev.call(prev, taken, events, rows, pair, me, fl, bel, ts)
            assert_same(got, after, len(rows), B, "self %d record %d" % (me, i))
            seen |= int(np.bitwise_or.reduce(after[4][:B]))
    return seen


@pytest.mark.parametrize("name", sorted(tt.LOOPS))
def test_recorded_closed_loop_calls(name):
    level, A, pair, B = tt.LOOPS[name]
    lv, rows, rec = recorded(level, A, pair, B, 120, 10)
    seen = replay(Dev(lv, A, B), rows, pair, rec, B)
    want = tb.UPDATED | tb.REINIT | tb.RESET | tb.RAISED | (tb.JOINT if name == "full" else 0)
    assert seen & want == want, seen


@pytest.mark.parametrize("B", [1, 7, 65, 1031, 16385, 70001])
def test_device_matches_host_edge_sizes(B):
    """70,001: more envs than one round of the grid holds, so lane groups take a second env (the
    grid-stride trip and the reuse of a group's LDS likelihood slots)."""
    level, A, pair, _ = tt.LOOPS["full"]
    lv, rows, rec = recorded(level, A, pair, B, 12, 12, (1,))
    prev, taken, events, fl, bel, ts, *after = rec[1][1]
    S = len(rows)
    assert (ts[:, B:] == tb.GUARD_TS).all() and (bel[:, B:] == tb.GUARD_BELIEF).all()
    dev = Dev(lv, A, B)
    assert_same(dev.call(prev, taken, events, rows, pair, 1, fl, bel, ts), after, S, B)
    for wl, wm, wi in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        assert_same(dev.call(prev, taken, events, rows, pair, 1, fl, bel, ts, wl, wm, wi), after, S, B)  # NULL outputs
    cs = CpuStepper(lv, A, B, nthreads=4)
    assert_same(dev.call(prev, taken, None, rows, pair, 0, fl, bel, ts),
                tb.host_call(cs, prev, taken, None, rows, pair, 0, fl, bel, ts), S, B, "no events, self 0")
    gb, gs = tb.new_buffers(S, cs.pitch)  # INIT over guard values, NULL inputs
    assert_same(dev.call(None, None, None, rows, pair, 1, tb.INIT, gb, gs),
                tb.host_call(cs, None, None, None, rows, pair, 1, tb.INIT, gb, gs), S, B, "init")


@pytest.mark.parametrize("A,K,shape", pg.TEAM_CELLS)
def test_every_dispatch_cell(A, K, shape):
    """One small loop per (A >= 2, K, layout) cell, the pair (0, A - 1), self the last agent."""
    lv, pair = pg.plan_level(K, shape), pg.team_pair(A)
    rows = tsr.level_rows(lv)
    _, rec = tb.closed_loop(lv, A, pair, pg.LOOP_B, pg.LOOP_STEPS, record_every=2, check=False, selfs=(pair[1],),
                            max_T=pg.LOOP_MAX_T)
    assert len(rec[pair[1]]) == pg.LOOP_STEPS // 2 + 1
    seen = replay(Dev(lv, A, pg.LOOP_B), rows, pair, rec, pg.LOOP_B)
    assert seen & tb.REINIT and seen & (tb.UPDATED | tb.RAISED | tb.EMPTY)


def test_graph_capture_and_replay():
    level, A, pair, B = tt.LOOPS["full"]
    lv, rows, rec = recorded(level, A, pair, B, 120, 10)
    prev, taken, events, fl, bel, ts, *after = rec[1][5]
    dev = Dev(lv, A, B)
    _, out = dev.launcher(prev, taken, events, rows, pair, 1, fl, bel, ts)  # the guard-filled buffers
    dprev, dtaken, dev_events = (torch.from_numpy(a).cuda() for a in (prev, taken, events))

    def run():
        dev.eb.team_belief_update(dprev, dtaken, rows, pair, 1, out[0], out[1], dev_events, 1.3, 0.5, fl, out[2], out[3],
                                  out[4])

    run()  # outside the capture first (the kernel's attributes, the module load)
    torch.cuda.synchronize()
    graph, cap = torch.cuda.CUDAGraph(), torch.cuda.Stream(device="cuda:0")
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=cap):
        run()
    torch.cuda.synchronize()
    out[0].copy_(torch.from_numpy(bel))  # the capture ran nothing: restore the inputs and replay once
    out[1].copy_(torch.from_numpy(ts))
    graph.replay()
    torch.cuda.synchronize()
    assert_same(tuple(t.cpu().numpy() for t in out), after, len(rows), B)


def test_vecenv_team_beliefs():
    """15 steps of team_actions((0, 1)) -> step -> team_beliefs((0, 1), 1): the env's buffers equal
    the batch-level calls (oc_progress, then oc_team_belief_update) on copies; a second call on the
    same states changes nothing; another pair or self agent, and reset(), start over."""
    from gym_cooking_amd.envs import OvercookedVecEnv
    B, A, pair = 300, 3, (0, 1)
    start = capi.OC_START_AGENTS | capi.OC_START_ITEMS
    env = OvercookedVecEnv("full-divider_tl", A, B, max_num_timesteps=12, random_starts=start, seed=27)
    env.reset()
    rows = tsr.level_rows(env.batch.level)
    S, P = len(rows), env.P
    N = S + 1
    bel, c0, c1, cJ, info = env.team_beliefs(pair, 1)
    torch.cuda.synchronize()
    assert bel.shape == (N, N, B) and c0.shape == c1.shape == cJ.shape == info.shape == (B,)
    assert (info.cpu().numpy() == tb.REINIT | tb.JOINT).all() and (cJ.cpu().numpy() == 0).all()
    assert env._tbelief[2] is None  # no likelihood buffer is kept
    same = lambda xs, ys: all(torch.equal(a, b) for a, b in zip(xs, ys) if a is not None)  # noqa: E731
    mine = [None if t is None else t.clone() for t in env._tbelief]
    seen = 0
    for t in range(15):
        acts, _ = env.team_actions(pair)
        env.step(acts)
        env.team_beliefs(pair, 1)
        torch.cuda.synchronize()
        prev, cur = env._s[env._i ^ 1], env.state
        _, ev, _ = env.batch.progress(prev, cur, rows, None, 1, None,
                                      torch.zeros((1, capi.event_planes(S), P), dtype=torch.uint8, device="cuda:0"), None)
        env.batch.team_belief_update(prev, env.ex, rows, pair, 1, mine[0], mine[1], ev, map=mine[3], info=mine[4])
        torch.cuda.synchronize()
        assert same(env._tbelief, mine), t
        seen |= int(np.bitwise_or.reduce(mine[4][:B].cpu().numpy()))
        before = [None if x is None else x.clone() for x in env._tbelief]
        env.team_beliefs(pair, 1)  # the same states: nothing changes (the call itself would multiply again)
        torch.cuda.synchronize()
        assert same(env._tbelief, before), t
    assert seen & tb.UPDATED and seen & tb.REINIT  # max_num_timesteps 12: the auto-reset envs start over
    for args in ((pair, 0), ((1, 2), 1)):  # another self agent, another pair
        *_, info = env.team_beliefs(*args)
        torch.cuda.synchronize()
        assert (info.cpu().numpy() & tb.REINIT != 0).all(), args
    env.step(env.team_actions(pair)[0])
    env.reset()
    *_, info = env.team_beliefs((1, 2), 1)
    torch.cuda.synchronize()
    assert (info.cpu().numpy() & tb.REINIT != 0).all()


@pytest.mark.parametrize("level,me,other", [("full-divider_salad", 1, 0), ("partial-divider_salad", 0, 1)])
def test_vecenv_delegate_actions(level, me, other):
    """delegate_actions(me, other) against its hand-composed launches: team_beliefs, oc_nav_policy on
    self's table and cur plane, oc_nav_policy on the two-agent table and curJ into a scratch buffer,
    self's scratch row where the map is joint; the other agent's bytes of `out` survive.  In
    full-divider_salad every one-agent hypothesis is pruned (the own table sees None or OUT only);
    in partial-divider_salad both map kinds occur and self follows subtasks of its own table."""
    from gym_cooking_amd.envs import OvercookedVecEnv
    B, A = 300, 2
    pair = (min(me, other), max(me, other))
    start = capi.OC_START_AGENTS | capi.OC_START_ITEMS
    env = OvercookedVecEnv(level, A, B, max_num_timesteps=30, random_starts=start, seed=5)
    env.reset()
    subs = list(env.subtasks)
    S, P, enc = len(subs), env.P, env.batch.level.encoding
    own = capi.policy_subtasks(subs + [None], enc, [me])
    joint = capi.policy_subtasks(subs, enc, pair)
    mode = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE
    rng = np.random.default_rng(3)
    q = 0 if me == pair[0] else 1  # self's cur plane
    joint_steps = split_steps = own_steps = 0
    for t in range(12):
        out = torch.from_numpy(rng.integers(0, 5, A * P, dtype=np.uint8)).cuda()  # the learner's actions, and junk in self's row
        before = out.clone()
        view, info = env.delegate_actions(me, other, out=out)
        torch.cuda.synchronize()
        cur = env.team_beliefs(pair, me)[1:4]  # the same states: unchanged
        tmap = env._tbelief[3]
        want, scratch = before.clone(), torch.full((A * P,), 4, dtype=torch.uint8, device="cuda:0")
        env.batch.nav_policy(env.state, own, want, mode=mode, alloc=tmap[q], step=env._round, seed=env.seed, num_cand=5)
        env.batch.nav_policy(env.state, joint, scratch, mode=mode, alloc=tmap[2], step=env._round, seed=env.seed, num_cand=25)
        torch.cuda.synchronize()
        isj = (cur[2] < S).cpu().numpy()
        w = want.view(A, P).cpu().numpy()
        w[me, :B] = np.where(isj, scratch.view(A, P)[me, :B].cpu().numpy(), w[me, :B])
        got = out.view(A, P).cpu().numpy()
        assert np.array_equal(got, w), t
        assert np.array_equal(got[other], before.view(A, P)[other].cpu().numpy()), t  # never written
        assert np.array_equal(got[:, B:], before.view(A, P)[:, B:].cpu().numpy()), t
        joint_steps += int(isj.sum())
        split_steps += int((~isj).sum())
        own_steps += int((cur[q] < S).sum())
        env.step(view)
    print(level, "joint", joint_steps, "split", split_steps, "self on a subtask of its own", own_steps)
    assert joint_steps > 0
    if level.startswith("partial"):
        assert split_steps > 0 and own_steps > 0  # both map kinds, and the own table on a real subtask
