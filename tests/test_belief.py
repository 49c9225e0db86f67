"""oc_cpu_belief_update (the per-env Bayesian belief over a watched agent's subtask) on the host:
against the reference's own SubtaskAllocDistribution updates (tests/golden/belief.npz), against the
numpy restatement tests/belief_ref.py in the closed scripted-partner loop at every step, on the level,
table and agent variants, on ragged sizes with guard bytes, thread counts, bad arguments; that it
infers the scripted agent's subtask at all; and the host row function under ASan + UBSan."""
import ctypes
import functools
import os

import numpy as np
import pytest

import belief_ref as br
import oc_testlib as tl
import taskselect_ref as tsr
from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

from oracle import oracle

pytestmark = pytest.mark.skipif(not os.path.isfile(capi.LIB_PATH), reason="liboc_engine.so not built")

INIT = br.INIT
LOOP = ("open-divider_salad", 2, (0, 1), 512)  # the closed loop of the issue (and of the GPU test)
GOLDEN = os.path.join(tl.ROOT, "tests", "golden", "belief.npz")


class Shares:
    """on_step hook: how often the inferred map equals the subtask oc_task_select gave the agent,
    at the first step of a commitment and after ten steps of it."""

    def __init__(self, M: int, B: int):
        self.age = np.zeros((M, B), np.int64)
        self.last = np.full((M, B), -1, np.int64)
        self.hit = np.zeros((M, 2), np.int64)
        self.n = np.zeros((M, 2), np.int64)

    def __call__(self, t, cur, amap):
        self.age = np.where(cur == self.last, self.age + 1, 1)
        self.last = cur.astype(np.int64)
        for k, sel in enumerate((self.age == 1, self.age >= 10)):
            self.hit[:, k] += (sel & (amap == cur)).sum(1)
            self.n[:, k] += sel.sum(1)


@functools.lru_cache(maxsize=None)
def main_loop():
    """The 120-step closed loop, checked at every step; every 10th call recorded.  Shared."""
    level, A, agents, B = LOOP
    sh = Shares(len(agents), B)
    ref, records = br.closed_loop(level, A, agents, B, 120, record_every=10, on_step=sh)
    return ref, records, sh


def test_closed_loop_matches_restatement_and_reaches_every_branch():
    ref, records, _ = main_loop()
    n = ref.n
    print("reinit %(reinit)d reset %(reset)d pruned %(pruned)d raised %(raised)d updated %(updated)d "
          "none_map %(none_map)d single %(single)d" % n)
    # the first call initialises every (env, agent): the floor is on the masked ones
    assert n["reinit"] - LOOP[3] * len(LOOP[2]) >= 100
    for k in ("reset", "pruned", "raised", "updated"):
        assert n[k] >= 100, (k, n[k])
    assert n["none_map"] >= 1
    assert len(records) == 13


def test_map_finds_the_scripted_agents_subtask():
    """A sanity check that the belief infers anything: the map equals the subtask oc_task_select
    gave the watched scripted agent in a larger share of env-steps after 10 steps of commitment
    than at its first step, for both agents."""
    _, _, sh = main_loop()
    share = sh.hit / np.maximum(sh.n, 1)
    print("share of env-steps with map == cur, per agent [first step, >= 10 steps]:", share.tolist(), sh.n.tolist())
    assert (sh.n > 0).all()
    for m in range(2):
        assert share[m, 1] > share[m, 0], (m, share[m])


def table_none(level):
    """The salad's 9 rows with OC_SUB_NONE rows inside the table."""
    rows = tsr.level_rows(tl.load_level(level))
    none = capi.subtask(capi.SUB_NONE, [0], [0, 0], 0)
    return rows[:4] + [none, none] + rows[4:] + [none]


def table63(level):
    rows = tsr.level_rows(tl.load_level(level))
    return [rows[i % len(rows)] for i in range(63)]


# level, A, watched, scripted, B, table, events
VARIANTS = {
    "a3_watch_2_0": ("partial-divider_salad", 3, (2, 0), (2, 0), 192, None, True),
    "enc_counts": ("levels/dup-7x7_tomato2.txt", 2, (0, 1), (0, 1), 192, None, True),
    "wide": ("levels/wide-17x17_salad.txt", 2, (0, 1), (0, 1), 128, None, True),
    "k16": ("levels/many-13x12_full16.txt", 2, (1,), (1,), 128, None, True),  # S = 38: one scripted agent's table
    "s63": ("open-divider_salad", 2, (0, 1), (0, 1), 128, table63, True),
    "none_rows": ("open-divider_salad", 2, (0, 1), (0, 1), 192, table_none, True),
    "no_events": ("open-divider_salad", 2, (0, 1), (0, 1), 192, None, False),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variants_match_restatement(name):
    level, A, agents, scripted, B, table, ev = VARIANTS[name]
    rows = None if table is None else table(level)
    ref, _ = br.closed_loop(level, A, agents, B, 40, rows=rows, use_events=ev, scripted=scripted)
    assert ref.n["updated"] > 0
    assert (ref.n["reset"] == 0) == (not ev), ref.n
    if name == "s63":
        assert len(rows) == 63


@functools.lru_cache(maxsize=None)
def mid_call(B: int):
    """(cs, ob, rows, record) of call 12 of the open-divider loop at B envs: record = (prev, taken,
    events, flags, belief before, bstate before, belief, bstate, map, info)."""
    level, A, agents, _ = LOOP
    _, rec = br.closed_loop(level, A, agents, B, 12, record_every=12, check=False)
    lv = tl.load_level(level)
    return CpuStepper(lv, A, B, nthreads=4), oracle.OracleBatch(lv, A, 100, B), tsr.level_rows(lv), rec[1]


@pytest.mark.parametrize("B", [1, 7, 65, 1031])
def test_ragged_sizes_and_guards(B):
    cs, ob, rows, rec = mid_call(B)
    prev, taken, events, fl, bel, bs = rec[:6]
    agents, S = LOOP[2], len(rows)
    assert (bs[:, :, B:] == br.GUARD_BS).all() and (bel[:, :, B:] == br.GUARD_BELIEF).all()
    # the step's inputs end at column B of their last plane
    P = cs.pitch
    taken_t = np.ascontiguousarray(taken[:P + B])
    events_t = np.ascontiguousarray(events.reshape(-1)[:(capi.event_planes(S) - 1) * P + B])
    ref = br.Ref(ob, cs, rows, agents)
    got = br.host_call(cs, prev, taken_t, events_t, rows, agents, fl, bel, bs)
    br.assert_equal(got, ref.update(prev, taken, events, fl, bel, bs), S, B)  # guard columns included
    assert (got[1][:, :, B:] == br.GUARD_BS).all() and (got[0][:, :, B:] == br.GUARD_BELIEF).all()
    for wm, wi in ((False, True), (True, False), (False, False)):  # map / info NULL: the same beliefs
        b2, s2, _, _ = br.host_call(cs, prev, taken, events, rows, agents, fl, bel, bs, want_map=wm, want_info=wi)
        assert np.array_equal(b2.view(np.uint64), got[0].view(np.uint64)) and np.array_equal(s2, got[1])
    # INIT over the guard values: every column below B written, nothing past it
    gb, gs = br.new_buffers(len(agents), S, P)
    ib, isb, imap, iinfo = br.host_call(cs, None, None, None, rows, agents, INIT, gb, gs)
    assert np.array_equal(ib[:, :, :B], np.full((2, S + 1, B), 1.0 / (S + 1))) and (iinfo[:, :B] == br.REINIT).all()
    assert (imap[:, :B] == 0).all()
    assert (ib[:, :, B:] == br.GUARD_BELIEF).all() and (isb[:, :, B:] == br.GUARD_BS).all()


def test_thread_counts_give_identical_bytes():
    B = 4100
    cs, _, rows, rec = mid_call(B)
    prev, taken, events, fl, bel, bs = rec[:6]
    outs = [br.host_call(cs, prev, taken, events, rows, LOOP[2], fl, bel, bs, nthreads=n) for n in (1, 2, 3, 8)]
    for o in outs[1:]:
        assert np.array_equal(o[0].view(np.uint64), outs[0][0].view(np.uint64))
        assert all(np.array_equal(x, y) for x, y in zip(o[1:], outs[0][1:]))


def test_second_call_multiplies_again():
    """Not idempotent by contract: the same step applied twice is two updates."""
    cs, _, rows, rec = mid_call(65)
    prev, taken, _, fl, bel, bs = rec[:6]
    once = br.host_call(cs, prev, taken, None, rows, LOOP[2], fl, bel, bs)
    twice = br.host_call(cs, prev, taken, None, rows, LOOP[2], fl, once[0], once[1])
    assert not np.array_equal(once[0][:, :, :65], twice[0][:, :, :65])
    assert ((twice[3][:, :65] & (br.UPDATED | br.RAISED)) != 0).all()


def test_zero_envs_is_ok():
    cs, _, rows, rec = mid_call(7)
    bel, bs = rec[4].copy(), rec[5].copy()
    ags = (ctypes.c_uint8 * 2)(0, 1)
    assert cs.lib.oc_cpu_belief_update(cs._h, rec[0].ctypes.data, rec[1].ctypes.data, None, capi.subtask_array(rows),
                                       len(rows), ags, 2, 1.3, 0.5, 0, bel.ctypes.data, bs.ctypes.data, None, None, 0,
                                       1) == 0
    assert np.array_equal(bel, rec[4]) and np.array_equal(bs, rec[5])


def test_bad_arguments():
    cs, _, rows, rec = mid_call(7)
    lib, S = cs.lib, len(rows)
    prev, taken = rec[0], rec[1]
    bel, bs = rec[4].copy(), rec[5].copy()
    sub = capi.subtask_array(rows)
    ags = (ctypes.c_uint8 * 4)(0, 1, 0, 0)
    err = ctypes.create_string_buffer(256)

    def call(state=prev.ctypes.data, tk=taken.ctypes.data, subs=sub, nS=S, agents=ags, M=2, beta=1.3, nap=0.5, flags=0,
             belief=None, bstate=bs.ctypes.data, fn=None, last=1):
        belief = bel.ctypes.data if belief is None else belief
        rc = (fn or lib.oc_cpu_belief_update)(cs._h, state, tk, None, subs, nS, agents, M, beta, nap, flags,
                                              belief or None, bstate, None, None, 7, last)
        n = lib.oc_get_last_error(cs._h, err, len(err))
        return rc, (err.value if n > 0 else b"")

    assert call()[0] == 0
    assert call(state=None, tk=None, flags=INIT)[0] == 0  # INIT reads neither
    big = capi.subtask_array([rows[i % S] for i in range(64)])
    for kw, text in ((dict(M=0), b"num_watched"), (dict(M=3), b"num_watched"), (dict(nS=0), b"num_subtasks"),
                     (dict(subs=big, nS=64, M=1), b"num_subtasks"),
                     (dict(agents=(ctypes.c_uint8 * 2)(0, 2)), b"agent 2"), (dict(agents=(ctypes.c_uint8 * 2)(1, 1)), b"twice"),
                     (dict(flags=2), b"flags"), (dict(flags=-1), b"flags"),
                     (dict(state=None), b"required"), (dict(tk=None), b"required"), (dict(subs=None), b"required"),
                     (dict(agents=None), b"required"), (dict(belief=0), b"required"), (dict(bstate=None), b"required"),
                     (dict(nap=1.5), b"none_action_prob"), (dict(nap=-0.1), b"none_action_prob"),
                     (dict(beta=float("nan")), b"beta"),
                     (dict(belief=bel.ctypes.data + 4), b"misaligned"), (dict(state=prev.ctypes.data + 1), b"misaligned")):
        rc, msg = call(**kw)
        assert rc == capi.OC_EINVAL and text in msg, (kw, rc, msg)
    bad_kind = capi.subtask_array([capi.subtask(7, [0], [0, 0], 0)])
    assert call(subs=bad_kind, nS=1)[0] == capi.OC_EINVAL
    assert lib.oc_cpu_belief_update(None, None, None, None, sub, S, ags, 2, 1.3, 0.5, INIT, bel.ctypes.data,
                                    bs.ctypes.data, None, None, 7, 1) == capi.OC_EINVAL
    assert call(last=-1)[0] == capi.OC_EINVAL  # nthreads
    rc = lib.oc_cpu_belief_update(cs._h, prev.ctypes.data, taken.ctypes.data, None, sub, S, ags, 2, 1.3, 0.5, 0,
                                  bel.ctypes.data, bs.ctypes.data, None, None, -1, 1)
    assert rc == capi.OC_EINVAL and lib.oc_get_last_error(cs._h, err, len(err)) > 0 and b"B -1" in err.value
    rc, msg = call(fn=lib.oc_belief_update, last=None)  # the device call on a host-only handle
    assert rc == capi.OC_EINVAL and b"host-only handle" in msg


def test_python_surface():
    """capi.belief_planes, the constants and CpuStepper.new_belief_state / belief_update."""
    assert [capi.belief_planes(S) for S in (1, 7, 8, 9, 63)] == [1, 1, 2, 2, 8]
    assert (capi.OC_BELIEF_INIT, capi.BELF_UPDATED, capi.BELF_PRUNED, capi.BELF_REINIT, capi.BELF_RESET,
            capi.BELF_RAISED) == (1, 1, 2, 4, 8, 16)
    cs, _, rows, rec = mid_call(65)
    prev, taken, events, fl, bel, bs = rec[:6]
    want = br.host_call(cs, prev, taken, events, rows, LOOP[2], fl, bel, bs)
    b2, s2, m2, i2 = cs.new_belief_state(len(rows), 2)
    assert b2.shape == (2, 10, cs.pitch) and s2.shape == (2, 4, cs.pitch) and not b2.any() and not s2.any()
    b2[:], s2[:] = bel, bs
    info = cs.belief_update(prev, taken, rows, LOOP[2], b2, s2, events, map=m2)
    assert info.shape == (2, cs.pitch)
    assert np.array_equal(b2.view(np.uint64), want[0].view(np.uint64)) and np.array_equal(s2, want[1])
    assert np.array_equal(m2[:, :65], want[2][:, :65]) and np.array_equal(info[:, :65], want[3][:, :65])


# ---- the reference's own updates -----------------------------------------------------------------

def golden():
    if not os.path.isfile(GOLDEN):
        pytest.fail("tests/golden/belief.npz is missing (tests/golden/gen_belief.py writes it)")
    return np.load(GOLDEN, allow_pickle=False)


def test_reference_fixture_replayed_from_init():
    """Every sequence of the fixture from its INIT: live and raised exact, beliefs to 1e-12."""
    g = golden()
    nseq = int(g["nseq"])
    pruned = raised = 0
    for q in range(nseq):
        level, A, a = str(g["level_%d" % q]), int(g["A_%d" % q]), int(g["agent_%d" % q])
        lv = tl.load_level(level)
        rows = [capi.subtask(int(k), [a], [int(x) for x in st], int(gm)) for k, st, gm in
                zip(g["sub_kind_%d" % q], g["sub_start_%d" % q], g["sub_goal_%d" % q])]
        S = len(rows)
        taken, live, bel, rz = (g["%s_%d" % (k, q)] for k in ("taken", "live", "belief", "raised"))
        T = len(taken)
        cs = CpuStepper(lv, A, T, nthreads=1)
        P, HP = cs.pitch, capi.belief_planes(S)
        # obs_tm1 of every step, one per column; the belief of the sequence lives in column 0
        obs = tl.state_from_canonical(lv, A, cs.K, P, g["st_agents_%d" % q], g["st_items_%d" % q],
                                      g["st_t_%d" % q]).reshape(-1, P)
        one = CpuStepper(lv, A, 1, nthreads=1)
        b, s = br.new_buffers(1, S, P)
        b, s, _, info = br.host_call(one, None, None, None, rows, (a,), INIT, b, s)
        assert info[0, 0] == br.REINIT
        for t in range(T):
            prev = np.zeros_like(obs)
            prev[:, 0] = obs[:, t]
            tk = np.full((A, P), 4, np.uint8)
            tk[:, 0] = taken[t, :A]
            before = br.bits(s[0, HP:, :1], S + 1)[:, 0]
            b, s, amap, info = br.host_call(one, prev.reshape(-1), tk.reshape(-1), None, rows, (a,), 0, b, s)
            got_live = br.bits(s[0, HP:, :1], S + 1)[:, 0]
            where = (level, a, t)
            assert np.array_equal(got_live, live[t] != 0), (where, got_live, live[t])
            assert bool(info[0, 0] & br.RAISED) == bool(rz[t]), (where, info[0, 0], rz[t])
            assert bool(info[0, 0] & br.PRUNED) == bool((before & ~got_live).any()), where
            got = b[0, :, 0]
            assert (np.abs(got - bel[t]) <= 1e-12 * np.abs(bel[t])).all(), (where, got, bel[t])
            pruned += int((before & ~got_live).any())
            raised += int(rz[t])
    print("fixture: %d sequences, %d pruning steps, %d raised steps" % (nseq, pruned, raised))
    assert pruned >= 20 and raised >= 5


def test_host_sanitizer_program():
    """tests/belief_host: the host row function under ASan + UBSan in a stand-alone program."""
    import shutil
    import subprocess
    d = os.path.join(tl.ROOT, "tests", "belief_host")
    if not os.path.isfile("/opt/rocm/llvm/bin/clang++") and shutil.which("clang++") is None:
        pytest.skip("no clang++ for the sanitizer build")
    r = subprocess.run(["make", "-s", "-C", d], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "clean" in r.stdout
