"""GPU parity of oc_belief_update: the device kernel against the host call (oc_cpu_belief_update,
itself pinned to the reference fixture and to the numpy restatement by tests/test_belief.py) on
identical inputs: the recorded calls of the closed scripted-partner loop, the level / table / agent
variants, ragged sizes with guard columns, a size past one round of the grid (the launch has at most
8 blocks of 32 lane groups per CU: 65,536 envs per round on 256 CUs), a captured graph; and
OvercookedVecEnv.partner_beliefs against the batch-level calls, with its round bookkeeping."""
import functools

import numpy as np
import pytest

import belief_ref as br
import oc_testlib as tl
import taskselect_ref as tsr
import test_belief as tb
from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oc_devlib import BeliefDev as Dev, belief_assert_same as assert_same  # noqa: E402


@functools.lru_cache(maxsize=None)
def recorded(level, A, agents, scripted, B, steps, every, table=None, events=True):
    """The host loop's records (no restatement check here: tests/test_belief.py does that)."""
    lv = tl.load_level(level)
    rows = tsr.level_rows(lv) if table is None else getattr(tb, table)(level)
    _, rec = br.closed_loop(lv, A, agents, B, steps, rows=rows, use_events=events, record_every=every, check=False,
                            scripted=scripted)
    return lv, rows, rec


def test_recorded_closed_loop_calls():
    level, A, agents, B = tb.LOOP
    lv, rows, rec = recorded(level, A, agents, agents, B, 120, 10)
    assert len(rec) == 13
    dev = Dev(lv, A, B)
    seen = 0
    for i, (prev, taken, events, fl, bel, bs, *after) in enumerate(rec):
        assert_same(dev.call(prev, taken, events, rows, agents, fl, bel, bs), after, len(rows), B, "record %d" % i)
        seen |= int(np.bitwise_or.reduce(after[3][:, :B].reshape(-1)))
    assert seen == br.UPDATED | br.PRUNED | br.REINIT | br.RESET | br.RAISED  # every info bit occurs in the records


@pytest.mark.parametrize("name", sorted(tb.VARIANTS))
def test_variants(name):
    level, A, agents, scripted, B, table, ev = tb.VARIANTS[name]
    lv, rows, rec = recorded(level, A, agents, scripted, B, 40, 8, None if table is None else table.__name__, ev)
    dev = Dev(lv, A, B)
    for i, (prev, taken, events, fl, bel, bs, *after) in enumerate(rec):
        assert_same(dev.call(prev, taken, events, rows, agents, fl, bel, bs), after, len(rows), B, "record %d" % i)


@pytest.mark.parametrize("B", [1, 7, 65, 1031, 16385, 70001])
def test_device_matches_host_edge_sizes(B):
    """70,001: more (env, agent) groups than one round of the grid holds, so lane groups take a
    second env (the grid-stride trip and the reuse of a group's LDS belief slots)."""
    level, A, agents, _ = tb.LOOP
    lv, rows, rec = recorded(level, A, agents, agents, B, 12, 12)
    prev, taken, events, fl, bel, bs, *after = rec[1]
    S = len(rows)
    assert (bs[:, :, B:] == br.GUARD_BS).all() and (bel[:, :, B:] == br.GUARD_BELIEF).all()
    dev = Dev(lv, A, B)
    assert_same(dev.call(prev, taken, events, rows, agents, fl, bel, bs), after, S, B)
    for wm, wi in ((False, True), (True, False), (False, False)):  # map / info NULL: the same state
        got = dev.call(prev, taken, events, rows, agents, fl, bel, bs, wm, wi)
        assert_same(got, after, S, B)
    cs = CpuStepper(lv, A, B, nthreads=4)
    assert_same(dev.call(prev, taken, None, rows, agents, fl, bel, bs),
                br.host_call(cs, prev, taken, None, rows, agents, fl, bel, bs), S, B, "no events")
    gb, gs = br.new_buffers(len(agents), S, cs.pitch)  # INIT over guard values, NULL inputs
    assert_same(dev.call(None, None, None, rows, agents, br.INIT, gb, gs),
                br.host_call(cs, None, None, None, rows, agents, br.INIT, gb, gs), S, B, "init")


def test_graph_capture_and_replay():
    level, A, agents, B = tb.LOOP
    lv, rows, rec = recorded(level, A, agents, agents, B, 120, 10)
    prev, taken, events, fl, bel, bs, *after = rec[5]
    dev = Dev(lv, A, B)
    up = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dprev, dtaken, dev_events = up(prev), up(taken), up(events)
    out = (up(bel), up(bs), torch.zeros((2, dev.eb.pitch), dtype=torch.uint8, device="cuda:0"),
           torch.zeros((2, dev.eb.pitch), dtype=torch.uint8, device="cuda:0"))
    out[2].fill_(br.GUARD_MAP)
    out[3].fill_(br.GUARD_INFO)

    def run():
        dev.eb.belief_update(dprev, dtaken, rows, agents, out[0], out[1], dev_events, 1.3, 0.5, fl, out[2], out[3])

    run()  # outside the capture first (the kernel's attributes, the module load)
    torch.cuda.synchronize()
    graph, cap = torch.cuda.CUDAGraph(), torch.cuda.Stream(device="cuda:0")
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=cap):
        run()
    torch.cuda.synchronize()
    out[0].copy_(up(bel))  # the capture ran nothing: restore the inputs and replay once
    out[1].copy_(up(bs))
    graph.replay()
    torch.cuda.synchronize()
    assert_same(tuple(t.cpu().numpy() for t in out), after, len(rows), B)


def test_vecenv_partner_beliefs():
    """15 steps of scripted_actions((0, 1)) -> step -> partner_beliefs((0, 1)): the env's buffers
    equal the batch-level calls (oc_progress, then oc_belief_update) on downloaded copies; a second
    call on the same states changes nothing; other agents start over."""
    from gym_cooking_amd.envs import OvercookedVecEnv
    B, A, agents = 300, 2, (0, 1)
    start = capi.OC_START_AGENTS | capi.OC_START_ITEMS
    env = OvercookedVecEnv("open-divider_salad", A, B, max_num_timesteps=12, random_starts=start, seed=27)
    env.reset()
    rows = tsr.level_rows(env.batch.level)
    S, P = len(rows), env.P
    bel, amap, info = env.partner_beliefs(agents)
    torch.cuda.synchronize()
    assert bel.shape == (2, S + 1, B) and amap.shape == (2, B) and info.shape == (2, B)
    assert (info.cpu().numpy() == br.REINIT).all() and np.array_equal(bel.cpu().numpy(), np.full((2, S + 1, B), 1 / (S + 1)))
    mine = [t.clone() for t in env._belief]
    seen = 0
    for t in range(15):
        acts, _ = env.scripted_actions(agents)
        env.step(acts)
        bel, amap, info = env.partner_beliefs(agents)
        torch.cuda.synchronize()
        prev, cur = env._s[env._i ^ 1], env.state
        _, ev, _ = env.batch.progress(prev, cur, rows, None, 1, None, torch.zeros((1, capi.event_planes(S), P), dtype=torch.uint8,
                                                                                  device="cuda:0"), None)
        env.batch.belief_update(prev, env.ex, rows, agents, mine[0], mine[1], ev, map=mine[2], info=mine[3])
        torch.cuda.synchronize()
        for a, b in zip(env._belief, mine):
            assert torch.equal(a, b), t
        seen |= int(np.bitwise_or.reduce(info.cpu().numpy().reshape(-1)))
        before = [x.clone() for x in env._belief]
        env.partner_beliefs(agents)  # the same states: nothing changes (the call itself would multiply again)
        torch.cuda.synchronize()
        for a, b in zip(env._belief, before):
            assert torch.equal(a, b), t
    assert seen & br.UPDATED and seen & br.REINIT  # max_num_timesteps 12: the auto-reset envs start over
    _, _, info = env.partner_beliefs((1,))
    torch.cuda.synchronize()
    assert info.shape == (1, B) and (info.cpu().numpy() == br.REINIT).all()
    env.reset()
    _, _, info = env.partner_beliefs((1,))
    torch.cuda.synchronize()
    assert (info.cpu().numpy() == br.REINIT).all()
