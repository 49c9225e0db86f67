"""Every cell of the planner dispatch grid on the GPU: the 36 (A, K, layout) cells, levels and
inputs of tests/test_plan_grid.py through the kernels dispatch_plan instantiates, three tests per
cell at B = 203 (a partial word, lane group, wave and block everywhere):

  * rows: oc_rollout (Level-0 and Level-1 rows), oc_subtask_bounds and oc_nav_likelihood against
    the CPU oracle on the cell's random case.  The likelihood runs for self agents 0 and A - 1 on
    the joint table (32-lane groups) and its one-agent reduction (8-lane groups), in the default
    compacted form and forced to the grouped form, which must agree bit for bit.  On the narrow
    cells one more rollout has one row more than 64 per compute unit, the first size that leaves
    oc_rollout_group_kernel for the row-per-lane oc_rollout_kernel with its tables in LDS;
  * partner: oc_nav_policy (the four modes; 25 and 5 candidate planes), oc_task_select and
    oc_belief_update (the recorded calls of the host loops, all A agents scripted and watched) and,
    with two agents or more, oc_team_select (the recorded calls of the team loop of agents 0 and
    A - 1) against the host twins on the same bytes;
  * starts: oc_reset_random against oc_cpu_reset_random, the whole batch and masked by a state with
    DONE envs, at B = 7 and 203, guard bytes included."""
import numpy as np
import pytest

import belief_ref as br
import oc_testlib as tl
import start_ref as sr
import taskselect_ref as tr
import test_plan_grid as pg
import test_policy as tp
from gym_cooking_amd import capi
from test_plan_grid import B, PLAN_CELLS, plan_level

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oc_devlib as dl  # noqa: E402
import test_bounds_gpu as tbg  # noqa: E402
import test_likelihood_gpu as tlg  # noqa: E402
import test_policy_gpu as tpg  # noqa: E402
import test_rollout_gpu as trg  # noqa: E402
import test_startdist_gpu as tsg  # noqa: E402

BETA, NAP = tp.BETA, tp.NAP


def check_rollout(A, K, shape, size, want):
    """oc_rollout on the cell's case of `size` rows against the oracle's (state_out, flags, bounds)."""
    ob, s, acts, subs, alloc = pg.random_case(A, K, shape, (0, 1), size)
    o_out, o_fl, o_lb = want
    g_out, g_fl, g_lb = trg._gpu_rollout(ob.level, A, size, s, acts, subs, alloc)
    assert np.array_equal(o_fl, g_fl), np.argwhere(o_fl != g_fl)[:5]
    assert np.array_equal(o_lb.view(np.uint32), g_lb.view(np.uint32)), np.argwhere(o_lb != g_lb)[:5]
    v1, v2 = tl.env_view(o_out, A, K, ob.pitch, size), tl.env_view(g_out, A, K, ob.pitch, size)
    assert np.array_equal(v1, v2), np.argwhere(v1 != v2)[:5]


@pytest.mark.parametrize("A,K,shape", PLAN_CELLS)
def test_row_kernels_match_oracle(A, K, shape):
    ref = pg.oracle_rows(A, K, shape)  # tests/test_plan_grid.py checks that it is not degenerate
    check_rollout(A, K, shape, B, ref.rollout)
    if shape == "narrow":  # one row past 64 per CU: oc_rollout_kernel<A, K, false, false>
        big = torch.cuda.get_device_properties(0).multi_processor_count * 64 + 1
        check_rollout(A, K, shape, big, pg.oracle_rollout(A, K, shape, big))
    ob, s, acts, subs, alloc = pg.random_case(A, K, shape, (0, 1))
    lv, subs0 = ob.level, pg.level0(subs)

    o_lb, o_ok = ref.bounds
    g_lb, g_ok = tbg._gpu_bounds(lv, A, B, s, subs0)
    assert np.array_equal(o_lb.view(np.uint32), g_lb.view(np.uint32)), np.argwhere(o_lb != g_lb)[:5]
    assert np.array_equal(o_ok, g_ok), np.argwhere(o_ok != g_ok)[:5]

    for (table, self_agent), (o_v, o_f) in zip(pg.likelihood_calls(A, subs0), ref.lik):
        g_v, g_f = tlg._gpu_lik(lv, A, B, s, acts, table, alloc, self_agent, BETA, NAP)
        assert np.array_equal(o_f, g_f), np.argwhere(o_f != g_f)[:5]
        ok = o_f == capi.LIK_OK
        np.testing.assert_allclose(g_v[ok], o_v[ok], rtol=1e-12, atol=0)
        assert np.all(g_v[~ok] == 0)
        q_v, q_f = tlg._gpu_lik(lv, A, B, s, acts, table, alloc, self_agent, BETA, NAP, form=capi.OC_LIK_FORM_GROUPED)
        assert np.array_equal(q_f, g_f)
        assert np.array_equal(q_v.view(np.uint64), g_v.view(np.uint64))


@pytest.mark.parametrize("A,K,shape", PLAN_CELLS)
def test_partner_kernels_match_host(A, K, shape):
    lv, agents = plan_level(K, shape), pg.scripted(A)
    ob, s, _, subs, alloc = pg.random_case(A, K, shape)
    kw = dict(step=7, seed=1234, env_offset=5)
    for table, ncs in pg.policy_tables(A, subs):
        for nc in ncs:
            for mode in tpg.MODES:
                host = tp.host_policy(lv, A, B, s, table, alloc, mode, nc, **kw)
                tpg.assert_same(tpg.gpu_policy(lv, A, B, s, table, alloc, mode, nc, **kw), host, B)

    rows, LB = tr.level_rows(lv), pg.LOOP_B
    _, rec = pg.task_loop(A, K, shape, False, pg.RECORD_EVERY)
    assert len(rec) == pg.LOOP_STEPS
    dev = dl.TaskDev(lv, A, LB)
    restarted = False
    for st, prev, fl, ts, ts_after, bound, info in rec:
        dl.task_assert_same(dev.call(st, prev, rows, agents, fl, ts), (ts_after, bound, info))
        restarted |= not (fl & tr.INIT) and bool((info[:, :LB] & tr.REINIT).any())
    assert restarted  # some call started envs over from state_prev's DONE flags

    if A >= 2:
        _, rec = pg.team_loop(A, K, shape, False, pg.RECORD_EVERY)
        assert len(rec) == pg.LOOP_STEPS
        dev = dl.TeamDev(lv, A, LB)
        for st, prev, fl, ts, ts_after, bound, info in rec:
            dl.task_assert_same(dev.call(st, prev, rows, pg.team_pair(A), fl, ts), (ts_after, bound, info))

    _, rec = pg.belief_loop(A, K, shape, False, pg.RECORD_EVERY)
    assert len(rec) == pg.LOOP_STEPS + 1
    dev = dl.BeliefDev(lv, A, LB)
    seen = 0
    for i, (prev, taken, events, fl, bel, bs, *after) in enumerate(rec):
        dl.belief_assert_same(dev.call(prev, taken, events, rows, agents, fl, bel, bs), after, len(rows), LB,
                              "record %d" % i)
        seen |= int(np.bitwise_or.reduce(after[3][:, :LB].reshape(-1)))
    want = br.UPDATED | br.PRUNED | br.REINIT | br.RAISED
    assert seen & want == want


@pytest.mark.parametrize("A,K,shape", PLAN_CELLS)
def test_start_kernel_matches_host(A, K, shape):
    from gym_cooking_amd.engine import CpuStepper, OvercookedBatch
    lv = plan_level(K, shape)
    wide = capi.is_wide(lv)
    both = capi.OC_START_AGENTS | capi.OC_START_ITEMS
    for size in pg.START_SIZES:
        eb = OvercookedBatch(lv, A, size, max_T=3, device=tsg.DEV)
        cs = CpuStepper(lv, A, size, max_T=3)
        P = eb.pitch
        assert (eb.K, P) == (K, cs.pitch)
        raw, s = tsg.guarded(eb)
        eb.reset_random(s, None, pg.START_SEED, 0, both, pg.START_OFFSET)
        torch.cuda.synchronize()
        got = tsg.check_guards(raw, eb)
        want = cs.reset_random(np.full(cs.layout.state_bytes, pg.GUARD, np.uint8), None, pg.START_SEED, 0, both,
                               pg.START_OFFSET)
        assert np.array_equal(tl.env_view(got, A, K, P, size), tl.env_view(want, A, K, P, size)), size
        # the kernel writes whole words of four envs: nothing at or past the next multiple of 4 above B
        past = ~sr.env_byte_mask(A, K, wide, P, (size + 3) // 4 * 4)
        assert (got[past] == pg.GUARD).all()
        # masked by the DONE envs of a step's input state: the whole buffer, guard columns included
        prev, state = pg.done_case(A, K, shape, size)
        raw, s = tsg.guarded(eb, state)
        eb.reset_random(s, torch.from_numpy(prev).to(tsg.DEV), pg.START_SEED, 1, both, pg.START_OFFSET)
        torch.cuda.synchronize()
        want = cs.reset_random(state.copy(), prev, pg.START_SEED, 1, both, pg.START_OFFSET)
        got = tsg.check_guards(raw, eb)
        assert np.array_equal(got, want), (size, np.argwhere(got != want)[:5].tolist())
        assert not np.array_equal(want, state)
