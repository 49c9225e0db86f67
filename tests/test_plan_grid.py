"""Every cell of the planner dispatch grid on the host: A = 1..4 agents x K = 4 / 8 / 16 item slots
x the three layouts dispatch_plan tells apart, 36 cells.  The layouts are a narrow kitchen whose
distance table fits LDS (test_dispatch_grid's 12x8, 92 nodes), a narrow one whose graph has more
than 360 nodes so that the planner kernels read the distances from device memory (the 15x17 dense
lattice, 417 nodes) and a wide one (17x16, u16 cell ids).  The host twins go through dispatch_w, so
they see 24 distinct instantiations; the dense cells are their narrow ones on a second level.

Per cell, each host twin against its independent restatement:

  * oc_cpu_task_select inside taskselect_ref.closed_loop, every agent scripted in descending
    order, checked at every step;
  * oc_cpu_team_select inside teamselect_ref.closed_loop for the pair (0, A - 1), on the 27 cells
    with two agents or more, checked at every step;
  * oc_cpu_belief_update inside belief_ref.closed_loop with all A agents watched;
  * oc_cpu_nav_policy on a random case against policy_ref.distribution in both count modes, on
    the joint table (25 candidates) and its one-agent reduction (5); with one agent the table has
    one-agent rows only and runs with 5 and with 25 candidate planes;
  * oc_cpu_reset_random against start_ref: the whole batch, then masked by a state whose DONE
    envs a timed-out step left, at B = 7 and 203.

The narrow grid kitchen has 92 nodes x 96 cells, more than the 8,192 bytes up to which the engine
builds the node-to-square table, so unlike the shipped 7x7 kitchens it has the agent-pair table
only.  That is a path chosen by the level's data, not by a template argument, and the tests of the
larger committed levels cover it; the grid has no fourth shape for it.

tests/test_plan_grid_gpu.py runs the kernels of the same cells on the same inputs."""
import ctypes
import functools
import types

import numpy as np
import pytest

import belief_ref as br
import oc_testlib as tl
import policy_ref
import start_ref as sr
import taskselect_ref as tr
import teamselect_ref as mr
import test_policy as tp
import test_rollout_host as th
from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper
from test_dispatch_grid import dense_level, grid_level

SHAPES = ("narrow", "dense", "wide")
SLOTS = (4, 8, 16)
PLAN_CELLS = [(A, K, shape) for shape in SHAPES for K in SLOTS for A in (1, 2, 3, 4)]
TEAM_CELLS = [cell for cell in PLAN_CELLS if cell[0] >= 2]  # a team needs two agents
LEVELS = [(K, shape) for shape in SHAPES for K in SLOTS]
# random_rollout_case's seed of each cell's random case: row (shape, K), column A = 1..4.  The cells
# count up, except (2, 16, wide): seed 34 draws a table of one row, which has no joint rows
CASE_SEEDS = {
    ("narrow", 4): (1, 2, 3, 4), ("narrow", 8): (5, 6, 7, 8), ("narrow", 16): (9, 10, 11, 12),
    ("dense", 4): (13, 14, 15, 16), ("dense", 8): (17, 18, 19, 20), ("dense", 16): (21, 22, 23, 24),
    ("wide", 4): (25, 26, 27, 28), ("wide", 8): (29, 30, 31, 32), ("wide", 16): (33, 37, 35, 36),
}
B = 203  # ragged against 4, 8, 32, 64 and 256: a partial word, lane group, wave and block
LOOP_B, LOOP_STEPS, LOOP_MAX_T = 48, 16, 12  # the closed loops (seed 7, their default)
# The GPU replay takes every call of the loops, not every fourth: the envs time out at step 12, so
# only the call after it starts envs over from state_prev's DONE flags (a plane whose index depends
# on the cell), and a cell's RAISED rows are few (every fourth call misses them in 12 of the 36 cells).
RECORD_EVERY = 1
START_SIZES = (7, 203)
START_SEED, START_OFFSET = 0xD1B54A32D192ED03, 1 << 33
MAX_GRAPH_NODES_IN_LDS = 360  # ocro::kMaxNodes
GUARD = 0xA5
CD = tr.COMMIT | tr.DISTINCT


def plan_level(K: int, shape: str):
    return dense_level(K) if shape == "dense" else grid_level(K, shape)


def scripted(A: int):
    """Every agent, in descending order: the priority order is not the index order."""
    return tuple(range(A))[::-1]


def graph_nodes(lv) -> int:
    """Nodes of the engine's reachability graph (oc_reachability16 on a host-only handle)."""
    cs = CpuStepper(lv, 1, 1)
    n = ctypes.c_int32()
    capi.check(cs.lib.oc_reachability16(cs._h, ctypes.byref(n), None, 0, None, 0))
    return n.value


@pytest.mark.parametrize("K,shape", LEVELS)
def test_levels_take_the_layout_they_stand_for(K, shape):
    lv = plan_level(K, shape)
    assert capi.item_slots(lv) == K
    assert capi.is_wide(lv) == (shape == "wide")
    if shape != "wide":  # a wide level's distances are in device memory whatever its graph
        assert (graph_nodes(lv) > MAX_GRAPH_NODES_IN_LDS) == (shape == "dense")
    assert len(tr.level_rows(lv)) == 9  # M * S <= 36 configurations for the belief kernel


def task_loop(A: int, K: int, shape: str, check: bool, record_every: int = 0):
    """(Ref with its counters, records) of the scripted-partner loop, every agent scripted."""
    return tr.closed_loop(plan_level(K, shape), A, scripted(A), LOOP_B, LOOP_STEPS, CD, max_T=LOOP_MAX_T,
                          record_every=record_every, check=check)


def team_pair(A: int):
    """The team: the first and the last agent (with 3 or 4 agents the others act at random)."""
    return (0, A - 1)


def team_loop(A: int, K: int, shape: str, check: bool, record_every: int = 0):
    """(Ref with its counters, records) of the team loop of team_pair(A)."""
    ref, rec, _ = mr.closed_loop(plan_level(K, shape), A, team_pair(A), LOOP_B, LOOP_STEPS, mr.COMMIT, max_T=LOOP_MAX_T,
                                 record_every=record_every, check=check)
    return ref, rec


def belief_loop(A: int, K: int, shape: str, check: bool, record_every: int = 0):
    """(Ref with its counters, records) of the loop with the belief update, every agent watched."""
    return br.closed_loop(plan_level(K, shape), A, scripted(A), LOOP_B, LOOP_STEPS, max_T=LOOP_MAX_T,
                          record_every=record_every, check=check)


@functools.lru_cache(maxsize=None)
def task_counts(A: int, K: int, shape: str) -> dict:
    """The restatement's branch counters of the cell's loop, every step checked against it."""
    return dict(task_loop(A, K, shape, True)[0].n)


@functools.lru_cache(maxsize=None)
def team_counts(A: int, K: int, shape: str) -> dict:
    return dict(team_loop(A, K, shape, True)[0].n)


@functools.lru_cache(maxsize=None)
def belief_counts(A: int, K: int, shape: str) -> dict:
    return dict(belief_loop(A, K, shape, True)[0].n)


@pytest.mark.parametrize("A,K,shape", PLAN_CELLS)
def test_task_select_matches_restatement(A, K, shape):
    n = task_counts(A, K, shape)
    assert n["reinit"] >= 2 * LOOP_B  # the INIT call, and every env timing out at step 12 of the 16


@pytest.mark.parametrize("A,K,shape", TEAM_CELLS)
def test_team_select_matches_restatement(A, K, shape):
    n = team_counts(A, K, shape)
    assert n["reinit"] >= 2 * LOOP_B  # the INIT call, and every env timing out at step 12 of the 16
    assert n["split"] >= 1 and n["completed"] >= 1, n


@pytest.mark.parametrize("A,K,shape", PLAN_CELLS)
def test_belief_update_matches_restatement(A, K, shape):
    n = belief_counts(A, K, shape)
    assert min(n["reinit"], n["pruned"], n["raised"], n["updated"]) >= 1, n


@pytest.mark.parametrize("K,shape", LEVELS)
def test_loops_of_a_level_reach_completion_and_reset(K, shape):
    """Over the four A of a level some scripted agent completes a subtask and some watched agent's
    belief is reset by a completion event (single cells with 3 or 4 agents may see neither in 16 steps)."""
    assert sum(task_counts(A, K, shape)["completed"] for A in (1, 2, 3, 4)) >= 1
    assert sum(belief_counts(A, K, shape)["reset"] for A in (1, 2, 3, 4)) >= 1


@pytest.mark.parametrize("K,shape", [level for level in LEVELS if level != (16, "wide")])
def test_team_loops_of_a_level_reach_a_joint_allocation(K, shape):
    """Over the three A of a level some env is played jointly (in 6 of the 27 single cells the pair
    stays split for all 16 steps).  The wide 16-slot level is left out: its 768 env-steps are split
    ones for every pair of every A, with COMMIT and with no flag, at this LOOP_B and LOOP_STEPS; the
    idle branch does not occur in any cell's loop.  tests/test_teamselect.py reaches both."""
    assert sum(team_counts(A, K, shape)["joint"] for A in (2, 3, 4)) >= 1


def level0(subs):
    """The table as Level-0 configurations."""
    return [capi.subtask(x.kind, list(x.agent[:x.num_agents]), list(x.start_mask), x.goal_mask, x.goal_count, 0)
            for x in subs]


def one_agent(subs):
    """The table's one-agent reduction: every row for its first agent alone."""
    return [capi.subtask(x.kind, [x.agent[0]], list(x.start_mask), x.goal_mask, x.goal_count, x.level) for x in subs]


@functools.lru_cache(maxsize=None)
def random_case(A: int, K: int, shape: str, planner_levels=(0,), size: int = B):
    """(ob, state, actions, subtasks, alloc) of the cell's random case; shared, never modified."""
    seed = CASE_SEEDS[shape, K][A - 1]
    return th.random_rollout_case(plan_level(K, shape), A, size, seed, planner_levels=planner_levels)


def policy_tables(A: int, subs):
    """[(table, candidate-plane counts)]: the joint table with 25 and its one-agent reduction with 5;
    with one agent the table itself with 5 and with 25."""
    return [(subs, (25,)), (one_agent(subs), (5,))] if A >= 2 else [(subs, (5, 25))]


@pytest.mark.parametrize("A,K,shape", PLAN_CELLS)
def test_nav_policy_matches_restatement(A, K, shape):
    ob, s, _, subs, alloc = random_case(A, K, shape)
    for table, ncs in policy_tables(A, subs):
        for count_state in (False, True):
            ref = policy_ref.distribution(ob, s, table, alloc, tp.BETA, tp.NAP, count_state)
            ok = ref["flags"] == capi.POL_OK
            # the conditions on the case, counted with the oracle alone
            assert 4 * (ok & ((ref["probs"] > 0).sum(0) >= 2)).sum() >= B
            if A >= 2 and table is subs:
                assert (ok & ref["joint"]).sum() >= 20
            for nc in ncs:
                tp.assert_matches_restatement(ob, s, table, alloc, nc, ref, count_state)


def oracle_rollout(A: int, K: int, shape: str, size: int = B):
    """(state_out, flags, f32 bounds) of the CPU oracle on the cell's case with Level-0 and Level-1 rows."""
    ob, s, acts, subs, alloc = random_case(A, K, shape, (0, 1), size)
    out = ob.new_state()
    fl, lb = ob.rollout(s, out, acts, subs, alloc)
    return out, fl, lb


def likelihood_calls(A: int, subs0):
    """[(table, self agent)]: the joint table and its one-agent reduction, self agents 0 and A - 1."""
    tables = [subs0, one_agent(subs0)] if A >= 2 else [subs0]
    return [(t, a) for t in tables for a in sorted({0, A - 1})]


@functools.lru_cache(maxsize=None)
def oracle_rows(A: int, K: int, shape: str):
    """The CPU oracle on the cell's random case, for the row kernels of the GPU test: the rollout
    (Level-0 and Level-1 rows), and on the table's Level-0 form the subtask bounds and the
    likelihoods of likelihood_calls (values f64 [B], flags u8 [B])."""
    ob, s, acts, subs, alloc = random_case(A, K, shape, (0, 1))
    subs0 = level0(subs)
    return types.SimpleNamespace(
        levels={x.level for x in subs}, rollout=oracle_rollout(A, K, shape), bounds=ob.subtask_bounds(s, subs0),
        lik=[ob.nav_likelihood(s, acts, t, alloc, a, tp.BETA, tp.NAP) for t, a in likelihood_calls(A, subs0)])


@pytest.mark.parametrize("A,K,shape", PLAN_CELLS)
def test_random_case_reaches_the_row_kernels_branches(A, K, shape):
    """What the GPU test compares is not degenerate, counted with the oracle alone: rows of both
    planner levels, legal moves, positive bounds, doable and undoable configurations, and in every
    likelihood call at least 20 rows with a value."""
    ref = oracle_rows(A, K, shape)
    _, fl, lb = ref.rollout
    assert ref.levels == {0, 1}
    assert 4 * ((fl & capi.ROLL_LEGAL) != 0).sum() >= B and (lb > 0).sum() >= 20
    _, doable = ref.bounds
    assert doable.any() and not doable.all()
    assert min(int((f == capi.LIK_OK).sum()) for _, f in ref.lik) >= 20


@functools.lru_cache(maxsize=None)
def done_case(A: int, K: int, shape: str, size: int):
    """(prev, state): the states before and after a step that auto-reset the envs of `prev` that
    carry DONE; shared, never modified.  From random starts whose step counters are set to env % 3, two steps with
    max_T = 3: the first times out the envs at 2 (DONE in `prev`), the second gives `state`, written
    into a buffer of guard bytes."""
    lv = plan_level(K, shape)
    cs = CpuStepper(lv, A, size, max_T=3, nthreads=2)
    P = cs.pitch
    s = cs.reset_random(cs.new_state(), None, START_SEED, 0, 3, START_OFFSET)
    tl.planes_view(s, A, K, P)["t"][:size] = np.arange(size) % 3
    rng = np.random.default_rng(size)
    prev, state = np.zeros_like(s), np.full_like(s, GUARD)
    for src, dst in ((s, prev), (prev, state)):
        act = np.full((A, P), 4, np.uint8)
        act[:, :size] = rng.integers(0, 5, (A, size), dtype=np.uint8)
        cs.step(src, dst, act.reshape(-1))
    done = np.nonzero(prev.reshape(-1, P)[cs.layout.plane_flags, :size] & capi.OC_FLAG_DONE)[0]
    assert 0 < len(done) < size
    return prev, state


@pytest.mark.parametrize("A,K,shape", PLAN_CELLS)
def test_reset_random_matches_restatement(A, K, shape):
    lv = plan_level(K, shape)
    wide = capi.is_wide(lv)
    agent_ok, item_ok = sr.default_masks(lv, A)
    both = capi.OC_START_AGENTS | capi.OC_START_ITEMS
    for size in START_SIZES:
        cs = CpuStepper(lv, A, size, max_T=3, nthreads=2)
        P = cs.pitch
        s = np.full(cs.layout.state_bytes, GUARD, np.uint8)
        cs.reset_random(s, None, START_SEED, 0, both, START_OFFSET)
        exp = sr.expected(lv, A, size, agent_ok, item_ok, START_OFFSET, START_SEED, 0, both)
        got = tl.env_view(s, A, K, P, size)
        assert np.array_equal(got, exp), (size, np.argwhere(got != exp)[:5].tolist())
        assert (s[~sr.env_byte_mask(A, K, wide, P, size)] == GUARD).all(), "a byte past column B was written"
        # masked: only the envs the step auto-reset change, to the start the full call of that round gives
        prev, state = done_case(A, K, shape, size)
        done = np.nonzero(prev.reshape(-1, P)[cs.layout.plane_flags, :size] & capi.OC_FLAG_DONE)[0]
        want = state.copy()
        sr.scatter(want, sr.expected(lv, A, size, agent_ok, item_ok, START_OFFSET, START_SEED, 1, both), done, A, K, wide, P)
        got = cs.reset_random(state.copy(), prev, START_SEED, 1, both, START_OFFSET)
        assert np.array_equal(got, want), (size, np.argwhere(got != want)[:5].tolist())
        assert not np.array_equal(want, state)
