"""oc_cpu_team_select (per-env joint or split subtask choice of a scripted pair) on the host, against
the oracle-built numpy restatement tests/teamselect_ref.py: in the closed team loop (team_select ->
three nav_policy launches -> step -> masked reset_random) at every step, on the flag, table, level
and pair variants, on ragged sizes with guard bytes, on the initialisation paths and on bad
arguments; that the feature makes the full-divider kitchen playable where oc_task_select cannot;
and the host row function under ASan + UBSan."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oc_testlib as tl
import teamselect_ref as mr
from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

from oracle import oracle

pytestmark = pytest.mark.skipif(not os.path.isfile(capi.LIB_PATH), reason="liboc_engine.so not built")

INIT, COMMIT, SPLIT_FIRST = mr.INIT, mr.COMMIT, mr.SPLIT_FIRST
LOOP = ("full-divider_salad", 2, (0, 1), 512)  # the closed loop of the issue (and of the GPU test)


@functools.lru_cache(maxsize=None)
def main_loop():
    """The 200-step closed loop, checked at every step; every 10th step recorded.  Shared."""
    level, A, pair, B = LOOP
    return mr.closed_loop(level, A, pair, B, 200, COMMIT, record_every=10)


def test_closed_loop_matches_restatement_and_reaches_every_branch():
    ref, records, totals = main_loop()
    n = ref.n
    print("joint %(joint)d split %(split)d idle %(idle)d completed %(completed)d dropped %(dropped)d reinit %(reinit)d "
          "dropped_full %(dropped_full)d joint_to_split %(joint_to_split)d deliver %(deliver)d same_first %(same_first)d "
          "kept %(kept)d" % n, totals)
    # the first call initialises every env (512 REINIT env-steps): the floor is on the masked ones
    assert n["reinit"] - LOOP[3] >= 100
    for k in ("joint", "split", "completed", "dropped", "joint_to_split"):
        assert n[k] >= 100, (k, n[k])
    assert n["deliver"] >= 1 and n["dropped_full"] >= 1
    assert len(records) == 20
    rows = mr.level_rows(tl.load_level(LOOP[0]))
    assert len(rows) == 9 and rows[8].kind == capi.SUB_DELIVER


def table21(level):
    """The salad's 9 rows, 4 OC_SUB_NONE rows and 8 repeats: ties go to the lowest index."""
    rows = mr.level_rows(tl.load_level(level))
    none = capi.subtask(capi.SUB_NONE, [0], [0, 0], 0)
    return rows[:4] + [none, none] + rows[4:] + [none, none] + rows[:8]


def no_chops(level):
    return [r for r in mr.level_rows(tl.load_level(level)) if r.kind != capi.SUB_CHOP]


VARIANTS = {
    "partial_split_first": ("partial-divider_salad", 2, (0, 1), 256, COMMIT | SPLIT_FIRST, None),
    "partial": ("partial-divider_salad", 2, (0, 1), 256, COMMIT, None),
    "no_commit": ("full-divider_salad", 2, (0, 1), 256, 0, None),
    "pair_02_of_3": ("full-divider_tl", 3, (0, 2), 256, COMMIT, None),
    "enc_counts": ("levels/dup-7x7_tomato2.txt", 2, (0, 1), 256, COMMIT, None),
    "wide": ("levels/wide-17x17_salad.txt", 2, (0, 1), 128, COMMIT, None),
    "s21": ("full-divider_salad", 2, (0, 1), 256, COMMIT, table21),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variants_match_restatement(name):
    level, A, pair, B, flags, table = VARIANTS[name]
    rows = None if table is None else table(level)
    ref, rec, _ = mr.closed_loop(level, A, pair, B, 60, flags, rows=rows, record_every=60)
    n = ref.n
    print(name, n)
    assert n["joint"] + n["split"] > 0  # some env follows an allocation somewhere
    if name == "partial_split_first":
        # at the level's own reset both agents' best one-agent subtask is index 0 (bounds 24 and
        # 14): the "same first" branch of step 5 in every env at the first call
        first, s = mr.Ref(ref.ob, ref.cs, ref.rows, pair), ref.cs.new_state()
        want = first.select(s, None, flags | INIT, rec[0][3])
        mr.assert_equal(mr.host_call(ref.cs, s, None, ref.rows, pair, flags | INIT, rec[0][3]), want, B)
        assert first.n["same_first"] == B
        assert n["joint"] > 0 and n["split"] > 0
    if name == "s21":
        assert len(rows) == capi.OC_TEAM_MAX_SUBTASKS == 21
        S = 21
        cur = rec[0][4][capi.event_planes(S):capi.event_planes(S) + 3, :B]
        assert not np.isin(cur[cur < S], list(range(13, 21))).any()  # a repeat never wins over its original


def test_no_chops_is_idle_everywhere():
    """full-divider_salad at the level's own reset without the two Chop rows: only the Chops are
    jointly doable there, so every env is idle."""
    lv = tl.load_level("full-divider_salad")
    rows = no_chops("full-divider_salad")
    B = 256
    assert len(rows) == 7
    cs = CpuStepper(lv, 2, B, nthreads=4)
    ob = oracle.OracleBatch(lv, 2, 100, B)
    s = cs.new_state()
    ts = np.full((capi.team_planes(len(rows)), cs.pitch), mr.GUARD_TS, np.uint8)
    got = mr.host_call(cs, s, None, rows, (0, 1), COMMIT | INIT, ts)
    mr.assert_equal(got, mr.Ref(ob, cs, rows, (0, 1)).select(s, None, COMMIT | INIT, ts), B)
    assert (got[2][:B] == (mr.IDLE | mr.REINIT)).all()
    EP = capi.event_planes(len(rows))
    assert (got[0][EP:EP + 2, :B] == len(rows)).all() and (got[0][EP + 2, :B] == mr.OUT).all()
    assert (got[1][:, :B] == 0).all()


def test_team_plays_the_full_divider_kitchen():
    """full-divider_tomato, the same seed: with oc_cpu_task_select (COMMIT | DISTINCT) the agents
    idle (no one-agent subtask is doable); with oc_cpu_team_select (COMMIT) they deliver."""
    args = ("full-divider_tomato", 2, (0, 1), 64, 200)
    _, _, solo = mr.closed_loop(*args, 0, check=False, solo=True)
    _, _, team = mr.closed_loop(*args, COMMIT, check=False)
    solo_idle, team_idle = solo["idle"] / solo["env_steps"], team["idle"] / team["env_steps"]
    print("solo idle share %.4f team idle share %.4f solo successes %d team successes %d"
          % (solo_idle, team_idle, solo["successes"], team["successes"]))
    assert solo_idle >= 0.5
    assert team_idle <= 0.1
    assert team["successes"] > solo["successes"]
    assert team["successes"] >= 1


@functools.lru_cache(maxsize=None)
def mid_state(B: int):
    """(cs, ob, rows, state, prev, tstate) 12 steps into the full-divider loop at B envs."""
    level, A, pair, _ = LOOP
    _, rec, _ = mr.closed_loop(level, A, pair, B, 13, COMMIT, record_every=12, check=False)
    s, prev, _, ts, _, _, _ = rec[1]
    lv = tl.load_level(level)
    return CpuStepper(lv, A, B, nthreads=4), oracle.OracleBatch(lv, A, 100, B), mr.level_rows(lv), s, prev, ts


@pytest.mark.parametrize("B", [1, 7, 9, 4097])
def test_ragged_sizes_and_guards(B):
    cs, ob, rows, s, prev, ts = mid_state(B)
    pair = LOOP[2]
    ref = mr.Ref(ob, cs, rows, pair)
    assert (ts[:, B:] == mr.GUARD_TS).all()
    got = mr.host_call(cs, s, prev, rows, pair, COMMIT, ts)
    mr.assert_equal(got, ref.select(s, prev, COMMIT, ts), B)  # guard columns included
    assert (got[0][:, B:] == mr.GUARD_TS).all()
    # bound / info NULL: the same tstate and the same other output
    for wb, wi in ((False, True), (True, False), (False, False)):
        ts2, b2, i2 = mr.host_call(cs, s, prev, rows, pair, COMMIT, ts, want_bound=wb, want_info=wi)
        assert np.array_equal(ts2, got[0])
        assert b2 is None or np.array_equal(b2.view(np.uint32), got[1].view(np.uint32))
        assert i2 is None or np.array_equal(i2, got[2])


def test_zero_envs_is_ok():
    cs, _, rows, s, _, ts = mid_state(7)
    ags = (ctypes.c_uint8 * 2)(0, 1)
    before = ts.copy()
    assert cs.lib.oc_cpu_team_select(cs._h, s.ctypes.data, None, capi.subtask_array(rows), len(rows), ags, COMMIT,
                                     ts.ctypes.data, None, None, 0, 1) == 0
    assert np.array_equal(ts, before)


@pytest.mark.parametrize("path", ["init", "prev", "neither"])
def test_initialisation_paths(path):
    B = 4097
    cs, ob, rows, s, prev, ts = mid_state(B)
    pair = LOOP[2]
    # of the state before, only the flags are read: mark a third of the envs as ended there
    prev = prev.copy()
    done = np.random.default_rng(3).integers(0, 3, B) == 0
    prev.reshape(-1, cs.pitch)[cs.layout.plane_flags, :B] = np.where(done, capi.OC_FLAG_DONE, 0)
    flags = COMMIT | (INIT if path == "init" else 0)
    p = prev if path == "prev" else None
    ref = mr.Ref(ob, cs, rows, pair)
    got = mr.host_call(cs, s, p, rows, pair, flags, ts)
    mr.assert_equal(got, ref.select(s, p, flags, ts), B, path)
    re = (got[2][:B] & mr.REINIT) != 0
    want = np.ones(B, bool) if path == "init" else (done if path == "prev" else np.zeros(B, bool))
    assert (re == want).all()


def test_bad_arguments():
    cs, _, rows, s, _, ts = mid_state(7)
    lib, S = cs.lib, len(rows)
    ts = ts.copy()
    bound = np.zeros(2 * cs.pitch + 1, np.float32)
    sub = capi.subtask_array(rows)
    ags = (ctypes.c_uint8 * 2)(0, 1)
    err = ctypes.create_string_buffer(256)

    def call(h=cs._h, state=s.ctypes.data, subs=sub, nS=S, agents=ags, flags=COMMIT, tstate=ts.ctypes.data, bnd=None,
             fn=None, last=1):
        rc = (fn or lib.oc_cpu_team_select)(h, state, None, subs, nS, agents, flags, tstate, bnd, None, 7, last)
        n = lib.oc_get_last_error(h, err, len(err))
        return rc, (err.value if n > 0 else b"")

    assert call()[0] == 0
    big = capi.subtask_array([rows[i % S] for i in range(22)])
    for kw, text in ((dict(nS=0), b"num_subtasks"), (dict(subs=big, nS=22), b"num_subtasks"),
                     (dict(agents=(ctypes.c_uint8 * 2)(1, 0)), b"ascending"), (dict(agents=(ctypes.c_uint8 * 2)(1, 1)), b"ascending"),
                     (dict(agents=(ctypes.c_uint8 * 2)(0, 2)), b"agent 2"),
                     (dict(flags=8), b"flags"), (dict(flags=-1), b"flags"),
                     (dict(state=None), b"required"), (dict(subs=None), b"required"), (dict(agents=None), b"required"),
                     (dict(tstate=None), b"required"), (dict(bnd=bound.ctypes.data + 2), b"misaligned")):
        rc, msg = call(**kw)
        assert rc == capi.OC_EINVAL and text in msg, (kw, rc, msg)
    bad_kind = capi.subtask_array([capi.subtask(7, [0], [0, 0], 0)])
    assert call(subs=bad_kind, nS=1)[0] == capi.OC_EINVAL
    rc, msg = call(fn=lib.oc_team_select, last=None)  # the device call on a host-only handle
    assert rc == capi.OC_EINVAL and b"host-only handle" in msg
    one = CpuStepper(tl.load_level(LOOP[0]), 1, 7, nthreads=1)  # A = 1: no pair
    s1 = one.new_state()
    rc, msg = call(h=one._h, state=s1.ctypes.data)
    assert rc == capi.OC_EINVAL and b"2 agents" in msg, (rc, msg)


def test_python_surface():
    """capi.team_planes, CpuStepper.team_select and the cur planes as nav_policy's alloc."""
    assert [capi.team_planes(S) for S in (1, 8, 9, 21)] == [6, 6, 7, 8]
    cs, ob, rows, s, prev, ts = mid_state(9)
    pair = LOOP[2]
    want = mr.host_call(cs, s, prev, rows, pair, COMMIT, ts)
    ts2 = ts.copy()
    bound = np.full((2, cs.pitch), np.nan, np.float32)
    info = cs.team_select(s, rows, pair, ts2, prev, bound=bound)
    assert np.array_equal(ts2, want[0]) and np.array_equal(info[:9], want[2][:9])
    assert np.array_equal(bound[:, :9], want[1][:, :9])
    EP, S = capi.event_planes(len(rows)), len(rows)
    cur0, cur1, curJ = ts2[EP:EP + 3, :9]
    joint = curJ < S
    assert ((cur0[joint] == mr.OUT) & (cur1[joint] == mr.OUT)).all()
    assert ((cur0[~joint] <= S) & (cur1[~joint] <= S) & (curJ[~joint] == mr.OUT)).all()
    assert np.array_equal((info[:9] & mr.JOINT) != 0, joint)
    with pytest.raises(ValueError):
        cs.team_select(s, rows, (0, 1, 2), ts2, prev)


def test_host_sanitizer_program():
    """tests/teamselect_host: the host row function under ASan + UBSan in a stand-alone program."""
    import shutil
    import subprocess
    d = os.path.join(tl.ROOT, "tests", "teamselect_host")
    if not os.path.isfile("/opt/rocm/llvm/bin/clang++") and shutil.which("clang++") is None:
        pytest.skip("no clang++ for the sanitizer build")
    r = subprocess.run(["make", "-s", "-C", d], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "clean" in r.stdout
