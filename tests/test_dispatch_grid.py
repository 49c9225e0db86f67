"""Every cell of the engine's (A, K, narrow / wide) dispatch grid on the host: A = 1..4 agents,
K = 4 / 8 / 16 item slots (3, 7 and 12 items), a narrow kitchen (12x8 = 96 cells, byte cell ids) and
a wide one (17x16 = 272 cells, u16 ids).  A dispatcher that maps a cell to another cell's template
instantiation reads or writes the wrong planes, so per cell:

  * oc_get_layout against the layout formula written out here;
  * oc_cpu_step against the CPU oracle over random play (states, executed actions, collision
    masks, totals), with max_T = 5 so that episodes time out and auto-reset inside the 12 steps,
    and the columns the batch's last word may and may not write;
  * oc_cpu_observe against tests/obs_ref.py and oc_cpu_progress against tests/progress_ref.py on
    the states of that play.

B = 7: one full word of four envs and one ragged word.  The narrow kitchen is of the common class
(H <= 8, at most 128 cells, no Floor on the border), so its K = 4 cells take the MODE 0 build of the
SWAR step and its K = 8 / 16 cells MODE 1; its 12-item level repeats the foods (counts encoding).
tests/test_dispatch_grid_gpu.py runs the same cells through the kernels."""
import functools
import os
import types

import numpy as np
import pytest

import obs_ref
import oc_testlib as tl
import progress_ref
from gym_cooking_amd import capi, levels, recipes
from gym_cooking_amd.engine import CpuStepper

from oracle import oracle

B, MAX_T, STEPS = 7, 5, 12
ITEMS = {4: "tlp", 8: "tlopppp", 16: "ttlloopppppp"}   # K: the level's items (3, 7, 12)
SHAPES = {"narrow": (12, 8), "wide": (17, 16)}
CELLS = [(A, K, shape) for shape in SHAPES for K in ITEMS for A in (1, 2, 3, 4)]


@functools.lru_cache(maxsize=None)
def grid_level(K: int, shape: str) -> levels.Level:
    """A W x H kitchen with ITEMS[K] on its bottom counter row (the ones past it on the top row),
    Cutboards and the Delivery on the left wall, and the four spawns next to the bottom row."""
    W, H = SHAPES[shape]
    items = ITEMS[K]
    top, bottom = ["-"] * W, ["-"] * W
    for i, ch in enumerate(items):
        row, x = (bottom, 1 + i) if i < W - 2 else (top, 1 + i - (W - 2))
        row[x] = ch
    rows = ["".join(top)] + [("*" if y == 2 else "/") + " " * (W - 2) + "-" for y in range(1, H - 1)] + ["".join(bottom)]
    spawns = "".join("%d %d\n" % (x, H - 2) for x in (1, 3, 5, 7))
    lv = levels.parse_level_text("\n".join(rows) + "\n\nSalad\n\n" + spawns, "grid-%s-%d" % (shape, K))
    assert len(lv.items) == len(items) and capi.item_slots(lv) == K
    assert capi.is_wide(lv) == (shape == "wide") and not lv.edge
    return lv


@functools.lru_cache(maxsize=None)
def dense_level(K: int) -> levels.Level:
    """tests/golden/levels/dense-15x17_salad.txt (255 cells, byte cell ids; its lattice of
    free-standing interior counters makes a 417-node reachability graph) with ITEMS[K] in place of
    its own items, on the bottom counter row from x = 1 (Floor above each).  The planner kernels
    of tests/test_plan_grid.py read such a level's distance table from device memory."""
    with open(os.path.join(tl.GOLDEN, "levels", "dense-15x17_salad.txt")) as f:
        grid, rest = f.read().split("\n\n", 1)
    rows = [r.translate(str.maketrans("tlop", "----")) for r in grid.split("\n")]
    items = ITEMS[K]
    rows[-1] = rows[-1][0] + items + rows[-1][1 + len(items):]
    lv = levels.parse_level_text("\n".join(rows) + "\n\n" + rest, "grid-dense-%d" % K)
    assert len(lv.items) == len(items) and capi.item_slots(lv) == K
    assert (lv.width, lv.height) == (15, 17) and not capi.is_wide(lv) and not lv.edge
    return lv


def expected_layout(A: int, K: int, wide: bool) -> dict:
    """oc_layout of an (A, K) state: A planes each of x, y, hold; K item-cell planes (and K more for
    a wide level's high bytes); K mask planes; the two planes of the u16 t; the flags."""
    hi = K if wide else 0
    np_ = 3 * A + 2 * K + hi + 3
    pitch = capi.OC_PITCH_ALIGN  # B = 7 rounds up to one pitch unit
    return dict(pitch=pitch, state_bytes=np_ * pitch, num_agents=A, num_items=K, plane_agent_x=0, plane_agent_y=A,
                plane_agent_hold=2 * A, plane_item_loc=3 * A, plane_item_loc_hi=3 * A + K if wide else -1,
                plane_item_mask=3 * A + K + hi, plane_t=3 * A + 2 * K + hi, plane_flags=3 * A + 2 * K + hi + 2,
                num_planes=np_, cell_bytes=2 if wide else 1)


def subtask_rows(lv):
    """(oc_subtask rows, [(kind, goal mask)]): the level's recipe subtasks, then a Merge and a
    Deliver row per item mask the level starts with, whose counts are not zero from the first state."""
    rows = capi.progress_subtasks(recipes.all_subtasks(lv), lv.encoding)
    for m in sorted({m for _, m in lv.items}):
        rows += [capi.subtask(capi.SUB_MERGE, [0], [0, 0], m), capi.subtask(capi.SUB_DELIVER, [0], [0, 0], m)]
    return rows, [(r.kind, r.goal_mask) for r in rows]


@functools.lru_cache(maxsize=None)
def oracle_play(A: int, K: int, shape: str):
    """STEPS steps of random play on the CPU oracle (which accepts the level): the start state and
    per step the actions, the state, the executed actions, the collision mask; the window totals."""
    lv = grid_level(K, shape)
    ob = oracle.OracleBatch(lv, A, MAX_T, B)
    assert ob.K == K
    P = ob.pitch
    s, nxt = ob.new_state(), ob.new_state()
    ob.reset(s)
    out = types.SimpleNamespace(level=lv, pitch=P, s0=s.copy(), acts=[], states=[], ex=[], coll=[],
                                totals=np.zeros(capi.OC_NSTATS, np.int64))
    act, ex, coll = ob.new_actions(), np.zeros(A * P, np.uint8), np.zeros(P, np.uint8)
    for t in range(STEPS):
        ob.gen_actions(act, 0, t, 97 * A + K)
        fl_in = tl.planes_view(s, A, K, P)["fl"].copy()
        ob.step(s, nxt, act, ex, coll)
        s, nxt = nxt, s
        out.totals += tl.window_totals(fl_in, s, coll, A, K, P, B)
        out.acts.append(act.copy())
        out.states.append(s.copy())
        out.ex.append(ex.reshape(A, P)[:, :B].copy())
        out.coll.append(coll[:B].copy())
    for a in out.acts + out.states + [out.s0]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("A,K,shape", CELLS)
def test_layout_matches_the_formula(A, K, shape):
    cs = CpuStepper(grid_level(K, shape), A, B, MAX_T)
    got = {name: getattr(cs.layout, name) for name, _ in capi.OcLayout._fields_}
    assert got == expected_layout(A, K, shape == "wide")


@pytest.mark.parametrize("A,K,shape", CELLS)
def test_cpu_step_matches_oracle(A, K, shape):
    ref = oracle_play(A, K, shape)
    cs = CpuStepper(ref.level, A, B, MAX_T, nthreads=2)
    P = cs.pitch
    assert P == ref.pitch
    assert np.array_equal(tl.env_view(cs.new_state(), A, K, P, B), tl.env_view(ref.s0, A, K, P, B))
    s, nxt = ref.s0.copy(), np.zeros_like(ref.s0)
    ex, coll, tot = np.zeros(A * P, np.uint8), np.zeros(P, np.uint8), np.zeros(capi.OC_NSTATS, np.uint64)
    for t in range(STEPS):
        cs.step(s, nxt, ref.acts[t], ex, coll, tot)
        s, nxt = nxt, s
        v, want = tl.env_view(s, A, K, P, B), tl.env_view(ref.states[t], A, K, P, B)
        assert np.array_equal(v, want), (t, np.argwhere(v != want)[:5].tolist())
        assert np.array_equal(ex.reshape(A, P)[:, :B], ref.ex[t]), t
        assert np.array_equal(coll[:B], ref.coll[t]), t
    assert np.array_equal(tot.astype(np.int64), ref.totals), (tot, ref.totals)
    assert ref.totals[0] >= 2 * B  # every env timed out and was reset, twice


@pytest.mark.parametrize("A,K,shape", CELLS)
def test_cpu_step_last_word_columns(A, K, shape):
    """One oc_cpu_step into buffers prefilled with 0xA5: columns 0..6 are the oracle's, and a wide
    level leaves column 7 of every plane (and env 7's two T bytes) as they were."""
    ref = oracle_play(A, K, shape)
    cs = CpuStepper(ref.level, A, B, MAX_T, nthreads=1)
    P, NP = cs.pitch, cs.layout.num_planes
    out, ex, coll = (np.full(n, 0xA5, np.uint8) for n in (NP * P, A * P, P))
    cs.step(ref.s0.copy(), out, ref.acts[0], ex, coll)
    assert np.array_equal(tl.env_view(out, A, K, P, B), tl.env_view(ref.states[0], A, K, P, B))
    assert np.array_equal(ex.reshape(A, P)[:, :B], ref.ex[0]) and np.array_equal(coll[:B], ref.coll[0])
    if shape == "wide":
        planes, pt = out.reshape(NP, P), cs.layout.plane_t
        byte_planes = [p for p in range(NP) if p not in (pt, pt + 1)]
        assert (planes[byte_planes, B] == 0xA5).all()
        assert (out[pt * P + 2 * B:pt * P + 2 * B + 2] == 0xA5).all()
        assert (ex.reshape(A, P)[:, B] == 0xA5).all() and coll[B] == 0xA5


@pytest.mark.parametrize("A,K,shape", CELLS)
def test_cpu_observe_matches_restatement(A, K, shape):
    ref = oracle_play(A, K, shape)
    cs = CpuStepper(ref.level, A, B, MAX_T, nthreads=2)
    lv, P = ref.level, cs.pitch
    for state, view in ((ref.s0, -1), (ref.states[3], A - 1), (ref.states[-1], -1)):
        want_obs, want_mask = obs_ref.observe(lv, A, K, state, P, B, view)
        obs, mask = cs.observe(state, np.uint8, view)
        assert obs.shape == (B, capi.obs_channels(A), lv.height, lv.width) and mask.shape == (A, P)
        assert np.array_equal(obs, want_obs), np.argwhere(obs != want_obs)[:5].tolist()
        assert np.array_equal(mask[:, :B], want_mask) and not mask[:, B:].any()
        obs16, _ = cs.observe(state, np.float16, view, want_mask=False)
        assert obs16.dtype == np.float16 and np.array_equal(obs16, want_obs.astype(np.float16))
    assert want_obs[:, 3:10].any()  # items in sight


@pytest.mark.parametrize("A,K,shape", CELLS)
def test_cpu_progress_matches_restatement(A, K, shape):
    ref = oracle_play(A, K, shape)
    cs = CpuStepper(ref.level, A, B, MAX_T, nthreads=2)
    rows, subs = subtask_rows(ref.level)
    S, P = len(rows), cs.pitch
    w = [0.5 + 0.25 * i for i in range(S)]
    traj = np.concatenate(ref.states)
    want_c, want_e, want_r = progress_ref.progress(ref.level, A, K, ref.s0, traj, P, B, subs, w, STEPS)
    cnt, ev, rew = cs.progress(ref.s0, traj, rows, w, STEPS)
    assert cnt.shape == (STEPS, S, P) and ev.shape == (STEPS, capi.event_planes(S), P) and rew.shape == (STEPS, P)
    assert np.array_equal(cnt[:, :, :B], want_c) and np.array_equal(ev[:, :, :B], want_e)
    assert np.array_equal(rew[:, :B].view(np.uint32), want_r.view(np.uint32))
    assert want_c.any()  # the rows of the level's own item masks count something
