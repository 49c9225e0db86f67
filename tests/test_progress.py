"""oc_cpu_progress (per-subtask object counts, completion events, shaped reward) on the host:
pinned to the reference through tests/golden/progress.npz (gen_progress.py: RealAgent's
def_subtask_completion / is_subtask_complete on replayed transitions), checked against the numpy
restatement tests/progress_ref.py on random play with auto-resets and ragged batch sizes, and
against planner._obj_count."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest

import oc_testlib as tl
import progress_ref
from gym_cooking_amd import capi, planner, recipes
from gym_cooking_amd.engine import CpuStepper

pytestmark = pytest.mark.skipif(not os.path.isfile(capi.LIB_PATH), reason="liboc_engine.so not built")

PAD = 255
PLAY = [("partial-divider_salad", 2), ("partial-divider_salad", 4), ("levels/dup-7x7_tomato2.txt", 2),
        ("levels/many-13x12_full16.txt", 3), ("levels/wide-17x17_salad.txt", 2)]
SIZES = (1, 63, 65, 4099)


@functools.lru_cache(maxsize=None)
def fixture():
    return tl.load_fixture("progress.npz")


def parse_subtask(name: str):
    """recipes.Subtask of a printed reference subtask, "Merge(Tomato, Plate)"."""
    kind, args = name[:-1].split("(")
    return getattr(recipes, kind)(*args.split(", "))


def subtask_rows(level, names=None):
    """(oc_subtask rows, [(kind, goal mask)]) of printed subtask names (default: all_subtasks)."""
    objs = recipes.all_subtasks(level) if names is None else [parse_subtask(n) for n in names]
    rows = capi.progress_subtasks(objs, level.encoding)
    return rows, [(r.kind, r.goal_mask) for r in rows]


class Group:
    """One (fixture, level, A) group of progress.npz: the transitions' two states in the engine
    layout, the subtasks, and the reference's counts and completion flags [S, B]."""

    def __init__(self, g: int):
        fx = fixture()
        sel = np.nonzero(fx["tr_group"] == g)[0]
        self.name = "%s:%s:A%d" % (fx["grp_fixture"][g], fx["grp_level"][g], fx["grp_A"][g])
        self.level = tl.load_level(str(fx["grp_level"][g]))
        self.A = int(fx["grp_A"][g])
        self.K = capi.item_slots(self.level)
        self.B = len(sel)
        self.pitch = capi.pitch_for(self.B)
        assert (self.level.encoding == 1) == bool(fx["grp_counts"][g]), self.name
        self.names = str(fx["grp_subtasks"][g]).split(";")
        self.S = len(self.names)
        self.rows, self.subs = subtask_rows(self.level, self.names)
        fl = capi.layout_planes(self.A, self.K, capi.is_wide(self.level))["flags"]
        for pre in ("p_", "c_"):
            s = tl.state_from_canonical(self.level, self.A, self.K, self.pitch, fx[pre + "agents"][sel],
                                        fx[pre + "items"][sel][:, :max(4, self.K)], fx[pre + "t"][sel])
            s.reshape(-1, self.pitch)[fl, :self.B] = fx[pre + "flags"][sel]
            setattr(self, "prev" if pre == "p_" else "cur", s)
        assert (fx["tr_cnt_cur"][sel][:, self.S:] == PAD).all()
        self.cnt_prev = fx["tr_cnt_prev"][sel][:, :self.S].T
        self.cnt_cur = fx["tr_cnt_cur"][sel][:, :self.S].T
        self.done = fx["tr_done"][sel][:, :self.S].T
        self.events = np.zeros((capi.event_planes(self.S), self.B), np.uint8)
        for i in range(self.S):
            self.events[i >> 3] |= self.done[i] << (i & 7)
        self.c_flags = fx["c_flags"][sel]


@functools.lru_cache(maxsize=None)
def group(g: int) -> Group:
    return Group(g)


def num_groups() -> int:
    return len(fixture()["grp_A"])


def test_fixture_coverage():
    """The classes gen_progress.py asserts, re-read from the committed file."""
    fx = fixture()
    kinds = {"Chop": 0, "Merge": 0, "Deliver": 0}
    on_success = ge2 = wide = k16 = twice = 0
    for g in range(num_groups()):
        G = group(g)
        for i, n in enumerate(G.names):
            kinds[n.split("(")[0]] += int(G.done[i].sum())
            if n.startswith("Deliver"):
                on_success += int((G.done[i] & ((G.c_flags & 2) != 0)).sum())
                twice += int((G.cnt_cur[i] >= 2).sum())
        ge2 += int((G.cnt_cur >= 2).sum())
        wide += capi.is_wide(G.level) * G.B
        k16 += (G.K == 16) * G.B
    assert min(kinds.values()) > 0 and on_success > 0 and ge2 > 0 and wide > 0 and k16 > 0, \
        (kinds, on_success, ge2, wide, k16)
    assert not (fx["p_flags"] & 1).any() and not (fx["c_flags"] & 4).any()
    assert (fx["tr_done"] == 1).any(1).sum() > 500  # every completing transition was kept


def test_restatement_equals_fixture():
    for g in range(num_groups()):
        G = group(g)
        args = (G.level, G.A, G.K)
        assert np.array_equal(progress_ref.counts(*args, G.prev, G.pitch, G.B, G.subs), G.cnt_prev), G.name
        cnt, ev, rew = progress_ref.progress(*args, G.prev, G.cur, G.pitch, G.B, G.subs)
        assert np.array_equal(cnt[0], G.cnt_cur) and np.array_equal(ev[0], G.events), G.name
        assert np.array_equal(rew[0], G.done.sum(0).astype(np.float32)), G.name


def test_cpu_progress_equals_fixture():
    for g in range(num_groups()):
        G = group(g)
        cs = CpuStepper(G.level, G.A, G.B)
        cnt, ev, rew = cs.progress(G.prev, G.cur, G.rows)
        assert cnt.shape == (1, G.S, G.pitch) and ev.shape == (1, capi.event_planes(G.S), G.pitch)
        assert np.array_equal(cnt[0, :, :G.B], G.cnt_cur), G.name
        assert np.array_equal(ev[0, :, :G.B], G.events), G.name
        assert np.array_equal(rew[0, :G.B], G.done.sum(0).astype(np.float32)), G.name
        cnt, ev, _ = cs.progress(G.prev, G.prev, G.rows)  # a state against itself: its counts, no event
        assert np.array_equal(cnt[0, :, :G.B], G.cnt_prev) and not ev.any(), G.name


def test_counts_equal_planner_obj_count():
    """planner._obj_count is the in-repo statement of the count: one Chop, one Merge and one
    Deliver subtask on sampled states of every group."""
    checked = {1: 0, 2: 0, 3: 0}
    for g in range(num_groups()):
        G = group(g)
        exp = types.SimpleNamespace(A=G.A, K=G.K, wide=capi.is_wide(G.level))
        cs = CpuStepper(G.level, G.A, G.B)
        cnt = cs.progress(G.prev, G.cur, G.rows, want=("counts",))[0][0]
        cols = G.cur.reshape(-1, G.pitch)
        picks = {}
        for i, (kind, goal) in enumerate(G.subs):
            picks.setdefault(kind, i)
        for kind, i in picks.items():
            me = types.SimpleNamespace(_kind=kind, _goal_mask=G.subs[i][1])
            for b in list(range(0, G.B, 7)) + list(np.nonzero(G.done[i])[0][:8]):
                assert planner.E2E_BRTDP._obj_count(me, cols[:, b], exp, G.level) == cnt[i, b], (G.name, i, b)
                checked[kind] += 1
    assert min(checked.values()) > 100, checked


@functools.lru_cache(maxsize=None)
def played(level: str, A: int, B: int, steps: int = 45, max_T: int = 30, seed: int = 5):
    """(CpuStepper, start state, trajectory [steps * state_bytes]) of random play; shared by the
    tests below and left unchanged.  An agent repeats its last action with probability 0.7 and
    draws a uniform one otherwise: with independent uniform draws no env of wide-17x17 carries a
    food to a cutting board inside a 30-step episode (0 events in 4099 envs x 60 steps), with
    sticky ones every level of PLAY shows events at seed 5."""
    lv = tl.load_level(level)
    cs = CpuStepper(lv, A, B, max_T=max_T, nthreads=4)
    rng = np.random.default_rng(seed)
    nb = cs.layout.state_bytes
    s0 = cs.new_state()
    traj = np.empty(steps * nb, np.uint8)
    s = s0
    act = rng.integers(0, 5, cs.A * cs.pitch, dtype=np.uint8)
    for r in range(steps):
        out = traj[r * nb:(r + 1) * nb]
        act = np.where(rng.random(act.shape) < 0.7, act, rng.integers(0, 5, act.shape, dtype=np.uint8))
        cs.step(s, out, act)
        s = out
    return cs, s0, traj


def weights_for(S: int):
    return [0.1 * (i + 1) for i in range(S)]  # non-dyadic: the order of the adds shows in the bits


@pytest.mark.parametrize("level,A", PLAY)
@pytest.mark.parametrize("B", SIZES)
def test_random_play_against_restatement(level, A, B):
    cs, s0, traj = played(level, A, B)
    lv, n = cs.level, 45
    rows, subs = subtask_rows(lv)
    w = weights_for(len(rows))
    exp_c, exp_e, exp_r = progress_ref.progress(lv, A, cs.K, s0, traj, cs.pitch, B, subs, w, n)
    fl = capi.layout_planes(A, cs.K, capi.is_wide(lv))["flags"]
    nb = cs.layout.state_bytes
    flags = np.stack([(s0 if r == 0 else traj[(r - 1) * nb:r * nb]).reshape(-1, cs.pitch)[fl, :B] for r in range(n)])
    was_done = (flags & 1) != 0  # [n, B]: prev was DONE, cur is the auto-reset state
    if B == 4099:  # the seed was chosen so that the restatement alone shows both
        assert exp_e.any() and was_done.any()
        assert (exp_r.view(np.uint32) != 0).any()
    assert not exp_e[np.broadcast_to(was_done[:, None, :], exp_e.shape)].any()
    for threads in sorted({1, 1 + B % 8, 8}):
        cs.nthreads = threads
        cnt, ev, rew = cs.progress(s0, traj, rows, w, n)
        assert np.array_equal(cnt[:, :, :B], exp_c), (level, A, B, threads)
        assert np.array_equal(ev[:, :, :B], exp_e), (level, A, B, threads)
        assert np.array_equal(rew[:, :B].view(np.uint32), exp_r.view(np.uint32)), (level, A, B, threads)
        assert not ev[:, :, :B][np.broadcast_to(was_done[:, None, :], exp_e.shape)].any()
        assert not cnt[:, :, B:].any() and not ev[:, :, B:].any() and not rew[:, B:].any()
    # n = 1 calls along the trajectory give the same as the one trajectory call
    for r in (0, 17, 31, n - 1):
        prev = s0 if r == 0 else traj[(r - 1) * nb:r * nb]
        c1, e1, r1 = cs.progress(prev, traj[r * nb:(r + 1) * nb], rows, w)
        assert np.array_equal(c1[0, :, :B], exp_c[r]) and np.array_equal(e1[0, :, :B], exp_e[r])
        assert np.array_equal(r1[0, :B].view(np.uint32), exp_r[r].view(np.uint32))


def raw_progress(cs, prev, states, n, rows, S, weights, counts, events, reward):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return cs.lib.oc_cpu_progress(cs._h, p(prev), p(states), n, None if rows is None else capi.subtask_array(rows),
                                  S, capi.weight_array(weights, S) if weights is not None else None, p(counts),
                                  p(events), p(reward), cs.B, cs.nthreads)


def test_guard_bytes_and_each_output_alone():
    """Nothing past column B of any output plane is written, whichever outputs are asked for,
    and every combination gives the same bits."""
    for B in (1, 63, 65, 4099):
        cs, s0, traj = played("partial-divider_salad", 2, B)
        rows, subs = subtask_rows(cs.level)
        S, n, P = len(rows), 3, cs.pitch
        w = weights_for(S)
        exp_c, exp_e, exp_r = progress_ref.progress(cs.level, 2, cs.K, s0, traj, P, B, subs, w, n)
        for want in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            cnt = np.full((n, S, P), 0xA5, np.uint8) if want[0] else None
            ev = np.full((n, capi.event_planes(S), P), 0xA5, np.uint8) if want[1] else None
            rew = np.full((n, P), 0xA5A5A5A5, np.uint32).view(np.float32) if want[2] else None
            assert raw_progress(cs, s0, traj, n, rows, S, w, cnt, ev, rew) == 0
            if cnt is not None:
                assert np.array_equal(cnt[:, :, :B], exp_c) and (cnt[:, :, B:] == 0xA5).all()
            if ev is not None:
                assert np.array_equal(ev[:, :, :B], exp_e) and (ev[:, :, B:] == 0xA5).all()
            if rew is not None:
                assert np.array_equal(rew[:, :B].view(np.uint32), exp_r.view(np.uint32))
                assert (rew[:, B:].view(np.uint32) == 0xA5A5A5A5).all()


def test_default_weights_count_the_events():
    cs, s0, traj = played("partial-divider_salad", 2, 4099)
    rows, _ = subtask_rows(cs.level)
    _, ev, rew = cs.progress(s0, traj, rows, None, 45)
    pop = np.unpackbits(ev, axis=1).reshape(45, -1, cs.pitch).sum(1)
    assert ev.any() and np.array_equal(rew, pop.astype(np.float32))


def test_bad_arguments_are_refused():
    cs, s0, traj = played("partial-divider_salad", 2, 63)
    rows, _ = subtask_rows(cs.level)
    S, P = len(rows), cs.pitch
    cnt, ev = np.zeros((1, S, P), np.uint8), np.zeros((1, capi.event_planes(S), P), np.uint8)
    rew = np.zeros((1, P), np.float32)
    bad_kind = list(rows)
    bad_kind[0] = capi.subtask(4, [0], [0, 0], 0)
    buf = ctypes.create_string_buffer(256)
    for args, word in (((s0, traj, 0, rows, S, None, cnt, ev, rew), b"n = 0"),
                       ((s0, traj, -3, rows, S, None, cnt, ev, rew), b"n = -3"),
                       ((s0, traj, 1, rows, 0, None, cnt, ev, rew), b"num_subtasks 0"),
                       ((s0, traj, 1, (rows * 65)[:65], capi.MAX_SUBTASKS + 1, None, cnt, ev, rew), b"num_subtasks 65"),
                       ((s0, traj, 1, bad_kind, S, None, cnt, ev, rew), b"kind 4"),
                       ((s0, traj, 1, rows, S, None, None, None, None), b"all NULL"),
                       ((None, traj, 1, rows, S, None, cnt, ev, rew), b"bad argument"),
                       ((s0, traj, 1, None, S, None, cnt, ev, rew), b"bad argument")):
        assert raw_progress(cs, *args) == capi.OC_EINVAL, word
        assert word in cs.lib.oc_last_error(), (word, cs.lib.oc_last_error())
        assert cs.lib.oc_get_last_error(cs._h, buf, len(buf)) > 0 and word in buf.value
    # the device entry point refuses a host-only handle
    rc = cs.lib.oc_progress(cs._h, s0.ctypes.data, traj.ctypes.data, 1, capi.subtask_array(rows), S, None,
                            cnt.ctypes.data, ev.ctypes.data, rew.ctypes.data, cs.B, None)
    assert rc == capi.OC_EINVAL and b"host-only handle" in cs.lib.oc_last_error()


def test_python_surface_agrees_on_the_abi():
    assert capi.OC_ABI_VERSION == 12 and capi.load_library().oc_abi_version() == 12
    assert {"oc_progress", "oc_cpu_progress"} <= set(capi.EXPORTED_SYMBOLS)
    assert [capi.event_planes(n) for n in (1, 8, 9, 64)] == [1, 1, 2, 8]
