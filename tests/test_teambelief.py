"""oc_cpu_team_belief_update (the per-env Bayesian belief over a pair's allocation) on the host:
against the reference's own SubtaskAllocDistribution updates over pair allocations
(tests/golden/teambelief.npz), against the numpy restatement tests/teambelief_ref.py in the closed
team loop at every step for both choices of the self agent, on ragged sizes with guard bytes,
thread counts, NULL outputs, bad arguments, and a wide and a K = 16 level."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oc_testlib as tl
import teambelief_ref as tb
import teamselect_ref as tsr
from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

from oracle import oracle

pytestmark = pytest.mark.skipif(not os.path.isfile(capi.LIB_PATH), reason="liboc_engine.so not built")

INIT = tb.INIT
LOOPS = {"full": ("full-divider_salad", 2, (0, 1), 512), "partial": ("partial-divider_salad", 2, (0, 1), 512)}
GOLDEN = os.path.join(tl.ROOT, "tests", "golden", "teambelief.npz")


class Shares:
    """on_step hook: how often the map's kind (joint or split) equals the kind of the allocation
    oc_team_select gave the pair, at the first step of a commitment and after ten steps of it."""

    def __init__(self, selfs, B: int):
        self.age = np.zeros(B, np.int64)
        self.last = np.full((3, B), -1, np.int64)
        self.hit = {a: np.zeros(2, np.int64) for a in selfs}
        self.n = np.zeros(2, np.int64)

    def __call__(self, t, cur, maps):
        S_or_out = cur[2] != capi.OC_TEAM_OUT  # the pair's allocation is joint
        same = (cur == self.last).all(0)
        self.age = np.where(same, self.age + 1, 1)
        self.last = cur.astype(np.int64)
        for k, sel in enumerate((self.age == 1, self.age >= 10)):
            self.n[k] += sel.sum()
            for a, m in maps.items():
                self.hit[a][k] += (sel & ((m[2] != capi.OC_TEAM_OUT) == S_or_out)).sum()


@functools.lru_cache(maxsize=None)
def main_loop(name: str):
    """The 120-step closed loop of one level, both self agents checked at every step; every 10th
    call recorded.  Shared."""
    level, A, pair, B = LOOPS[name]
    sh = Shares(pair, B)
    refs, records = tb.closed_loop(level, A, pair, B, 120, record_every=10, on_step=sh)
    return refs, records, sh


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_closed_loop_matches_restatement(name):
    refs, records, sh = main_loop(name)
    for a, ref in refs.items():
        print(name, "self", a, ref.n)
        assert ref.n["updated"] > 0 and ref.n["reinit"] > LOOPS[name][3]  # the masked restarts too
        assert len(records[a]) == 13
    share = {a: (h / np.maximum(sh.n, 1)).tolist() for a, h in sh.hit.items()}
    print(name, "share of env-steps whose map kind equals team_select's [first step, >= 10 steps]:", share,
          sh.n.tolist())


def test_every_info_bit_occurs():
    """Over the two loops every OC_TBELF_* bit is set somewhere, for each self agent."""
    for a in (0, 1):
        n = {k: sum(main_loop(name)[0][a].n[k] for name in LOOPS) for k in tb.ALL_BITS}
        for k, v in n.items():
            assert v >= 1, (a, k, n)
        assert sum(main_loop(name)[0][a].n["split_map"] for name in LOOPS) >= 1


def short_rows(level):
    return tsr.level_rows(tl.load_level(level))[:capi.OC_TEAM_MAX_SUBTASKS]


def table_none(level):
    """The salad's 9 rows with OC_SUB_NONE rows inside the table."""
    rows = tsr.level_rows(tl.load_level(level))
    none = capi.subtask(capi.SUB_NONE, [0], [0, 0], 0)
    return rows[:4] + [none, none] + rows[4:] + [none]


# level, A, pair, selfs, B, table, events
VARIANTS = {
    "wide": ("levels/wide-17x17_salad.txt", 2, (0, 1), (0,), 96, None, True),
    "k16": ("levels/many-13x12_full16.txt", 2, (0, 1), (1,), 96, short_rows, True),  # the first 21 of its 38 rows
    "pair_02_of_3": ("full-divider_tl", 3, (0, 2), (2,), 128, None, True),
    "none_rows": ("open-divider_salad", 2, (0, 1), (0,), 128, table_none, True),
    "no_events": ("partial-divider_salad", 2, (0, 1), (1,), 128, None, False),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variants_match_restatement(name):
    level, A, pair, selfs, B, table, ev = VARIANTS[name]
    rows = None if table is None else table(level)
    refs, _ = tb.closed_loop(level, A, pair, B, 30, rows=rows, use_events=ev, selfs=selfs)
    for ref in refs.values():
        print(name, ref.n)
        assert ref.n["updated"] > 0
        assert ev or ref.n["reset"] == 0


@functools.lru_cache(maxsize=None)
def mid_call(B: int):
    """(cs, ob, rows, record) of call 12 of the full-divider loop at B envs, self agent 1: record =
    (prev, taken, events, flags, belief before, tbstate before, belief, tbstate, lik, map, info)."""
    level, A, pair, _ = LOOPS["full"]
    _, rec = tb.closed_loop(level, A, pair, B, 12, record_every=12, check=False, selfs=(1,))
    lv = tl.load_level(level)
    return CpuStepper(lv, A, B, nthreads=4), oracle.OracleBatch(lv, A, 100, B), tsr.level_rows(lv), rec[1][1]


@pytest.mark.parametrize("B", [1, 7, 65, 1031])
def test_ragged_sizes_guards_and_null_outputs(B):
    cs, ob, rows, rec = mid_call(B)
    prev, taken, events, fl, bel, ts = rec[:6]
    pair, S, P = LOOPS["full"][2], len(rows), cs.pitch
    assert (ts[:, B:] == tb.GUARD_TS).all() and (bel[:, B:] == tb.GUARD_BELIEF).all()
    # the step's inputs end at column B of their last plane
    taken_t = np.ascontiguousarray(taken[:P + B])
    events_t = np.ascontiguousarray(events.reshape(-1)[:(capi.event_planes(S) - 1) * P + B])
    ref = tb.Ref(ob, cs, rows, pair)
    got = tb.host_call(cs, prev, taken_t, events_t, rows, pair, 1, fl, bel, ts)
    tb.assert_equal(got, ref.update(prev, taken, events, fl, 1, bel, ts), S, B)  # guard columns included
    assert (got[1][:, B:] == tb.GUARD_TS).all() and (got[0][:, B:] == tb.GUARD_BELIEF).all()
    for wl, wm, wi in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        b2, s2 = tb.host_call(cs, prev, taken, events, rows, pair, 1, fl, bel, ts, want_lik=wl, want_map=wm, want_info=wi)[:2]
        assert np.array_equal(b2.view(np.uint64), got[0].view(np.uint64)) and np.array_equal(s2, got[1])
    # INIT over the guard values with NULL inputs: every column below B written, nothing past it
    gb, gs = tb.new_buffers(S, P)
    ib, its, ilik, imap, iinfo = tb.host_call(cs, None, None, None, rows, pair, 1, INIT, gb, gs)
    N, n_live = S + 1, S + (S + 1) * S
    want = np.full((N * N - 1, B), 1.0 / n_live)  # uniform, then step 7's multiply by 1 / (their sum)
    assert tb.close(ib[:-1, :B], want)
    assert (ib[-1] == tb.GUARD_BELIEF).all()  # plane (S, S) is never written
    assert (iinfo[:B] == tb.REINIT | tb.JOINT).all() and (imap[:, :B] == np.array([[tb.OUT], [tb.OUT], [0]])).all()
    assert (ib[:, B:] == tb.GUARD_BELIEF).all() and (its[:, B:] == tb.GUARD_TS).all() and (ilik == tb.GUARD_LIK).all()


def test_thread_counts_give_identical_bytes():
    B = 4100
    cs, _, rows, rec = mid_call(B)
    prev, taken, events, fl, bel, ts = rec[:6]
    outs = [tb.host_call(cs, prev, taken, events, rows, LOOPS["full"][2], 1, fl, bel, ts, nthreads=n) for n in (1, 2, 3, 8)]
    for o in outs[1:]:
        assert np.array_equal(o[0].view(np.uint64), outs[0][0].view(np.uint64))
        assert np.array_equal(o[2].view(np.uint64), outs[0][2].view(np.uint64))
        assert all(np.array_equal(x, y) for x, y in zip(o[1::2], outs[0][1::2])) and np.array_equal(o[4], outs[0][4])


def test_second_call_multiplies_again_and_self_matters():
    cs, _, rows, rec = mid_call(65)
    prev, taken, _, fl, bel, ts = rec[:6]
    pair = LOOPS["full"][2]
    once = tb.host_call(cs, prev, taken, None, rows, pair, 1, fl, bel, ts)
    twice = tb.host_call(cs, prev, taken, None, rows, pair, 1, fl, once[0], once[1])
    assert not np.array_equal(once[0][:, :65], twice[0][:, :65])
    other = tb.host_call(cs, prev, taken, None, rows, pair, 0, fl, bel, ts)
    assert not np.array_equal(once[2][:, :65], other[2][:, :65])  # the joint rows' candidates follow self


def test_zero_envs_is_ok():
    cs, _, rows, rec = mid_call(7)
    bel, ts = rec[4].copy(), rec[5].copy()
    ags = (ctypes.c_uint8 * 2)(0, 1)
    assert cs.lib.oc_cpu_team_belief_update(cs._h, rec[0].ctypes.data, rec[1].ctypes.data, None, capi.subtask_array(rows),
                                            len(rows), ags, 0, 1.3, 0.5, 0, bel.ctypes.data, ts.ctypes.data, None, None,
                                            None, 0, 1) == 0
    assert np.array_equal(bel, rec[4]) and np.array_equal(ts, rec[5])


def test_bad_arguments():
    cs, _, rows, rec = mid_call(7)
    lib, S = cs.lib, len(rows)
    prev, taken = rec[0], rec[1]
    bel, ts = rec[4].copy(), rec[5].copy()
    sub = capi.subtask_array(rows)
    ags = (ctypes.c_uint8 * 2)(0, 1)
    err = ctypes.create_string_buffer(256)

    def call(h=cs._h, state=prev.ctypes.data, tk=taken.ctypes.data, subs=sub, nS=S, agents=ags, me=1, beta=1.3, nap=0.5,
             flags=0, belief=None, tbstate=ts.ctypes.data, lik=None, fn=None, last=1):
        belief = bel.ctypes.data if belief is None else belief
        rc = (fn or lib.oc_cpu_team_belief_update)(h, state, tk, None, subs, nS, agents, me, beta, nap, flags,
                                                   belief or None, tbstate, lik, None, None, 7, last)
        n = lib.oc_get_last_error(h, err, len(err))
        return rc, (err.value if n > 0 else b"")

    assert call()[0] == 0
    assert call(state=None, tk=None, flags=INIT)[0] == 0  # INIT reads neither
    big = capi.subtask_array([rows[i % S] for i in range(22)])
    lik = np.zeros((capi.team_lik_planes(S), cs.pitch))
    for kw, text in ((dict(me=2), b"self_agent"), (dict(me=-1), b"self_agent"),
                     (dict(agents=(ctypes.c_uint8 * 2)(1, 0)), b"not ascending"),
                     (dict(agents=(ctypes.c_uint8 * 2)(1, 1)), b"not ascending"),
                     (dict(agents=(ctypes.c_uint8 * 2)(0, 2), me=0), b"agent 2"),
                     (dict(nS=0), b"num_subtasks"), (dict(subs=big, nS=22), b"num_subtasks"),
                     (dict(flags=2), b"flags"), (dict(flags=-1), b"flags"),
                     (dict(state=None), b"required"), (dict(tk=None), b"required"), (dict(subs=None), b"required"),
                     (dict(agents=None), b"required"), (dict(belief=0), b"required"), (dict(tbstate=None), b"required"),
                     (dict(nap=1.5), b"none_action_prob"), (dict(beta=float("nan")), b"beta"),
                     (dict(belief=bel.ctypes.data + 4), b"misaligned"), (dict(lik=lik.ctypes.data + 4), b"misaligned"),
                     (dict(state=prev.ctypes.data + 1), b"misaligned")):
        rc, msg = call(**kw)
        assert rc == capi.OC_EINVAL and text in msg, (kw, rc, msg)
    assert call(last=-1)[0] == capi.OC_EINVAL  # nthreads
    one = CpuStepper(tl.load_level(LOOPS["full"][0]), 1, 7, nthreads=1)  # A = 1: no pair
    rc, msg = call(h=one._h, state=None, tk=None, flags=INIT)
    assert rc == capi.OC_EINVAL and b"2 agents" in msg
    rc, msg = call(fn=lib.oc_team_belief_update, last=None)  # the device call on a host-only handle
    assert rc == capi.OC_EINVAL and b"host-only handle" in msg


def test_python_surface():
    """capi's helpers and constants, and CpuStepper.new_team_belief_state / team_belief_update."""
    assert [capi.team_belief_planes(S) for S in (1, 7, 8, 9, 21)] == [4, 4, 6, 8, 12]
    assert (capi.OC_TBELIEF_INIT, capi.TBELF_UPDATED, capi.TBELF_PRUNED, capi.TBELF_REINIT, capi.TBELF_RESET,
            capi.TBELF_RAISED, capi.TBELF_EMPTY, capi.TBELF_JOINT) == (1, 1, 2, 4, 8, 16, 32, 64)
    cs, _, rows, rec = mid_call(65)
    prev, taken, events, fl, bel, ts = rec[:6]
    pair, S = LOOPS["full"][2], len(rows)
    want = tb.host_call(cs, prev, taken, events, rows, pair, 1, fl, bel, ts)
    b2, s2, l2, m2, _ = cs.new_team_belief_state(S)
    assert b2.shape == ((S + 1) ** 2, cs.pitch) and s2.shape == (capi.team_belief_planes(S), cs.pitch)
    assert l2.shape == (3 * S + 2, cs.pitch) and m2.shape == (3, cs.pitch) and not b2.any() and not s2.any()
    b2[:], s2[:] = bel, ts
    info = cs.team_belief_update(prev, taken, rows, pair, 1, b2, s2, events, lik=l2, map=m2)
    assert info.shape == (cs.pitch,)
    assert np.array_equal(b2.view(np.uint64), want[0].view(np.uint64)) and np.array_equal(s2, want[1])
    assert np.array_equal(m2[:, :65], want[3][:, :65]) and np.array_equal(info[:65], want[4][:65])


# ---- the reference's own updates -----------------------------------------------------------------

def test_reference_fixture_replayed_from_init():
    """Every sequence of the fixture from its INIT, for both choices of self: live sets, raised and
    empty steps exact, beliefs to 1e-12."""
    if not os.path.isfile(GOLDEN):
        pytest.fail("tests/golden/teambelief.npz is missing (tests/golden/gen_teambelief.py writes it)")
    g = np.load(GOLDEN, allow_pickle=False)
    nseq = int(g["nseq"])
    n = dict(pruned=0, raised=0, joint=0, split=0, empty=0)
    for q in range(nseq):
        level, A = str(g["level_%d" % q]), int(g["A_%d" % q])
        pair, me = tuple(int(a) for a in g["pair_%d" % q]), int(g["self_%d" % q])
        lv = tl.load_level(level)
        rows = [capi.subtask(int(k), [pair[0]], [int(x) for x in st], int(gm)) for k, st, gm in
                zip(g["sub_kind_%d" % q], g["sub_start_%d" % q], g["sub_goal_%d" % q])]
        S = len(rows)
        N = S + 1
        taken, live, bel, rz = (g["%s_%d" % (k, q)] for k in ("taken", "live", "belief", "raised"))
        T = len(taken)
        cs = CpuStepper(lv, A, T, nthreads=1)
        P = cs.pitch
        # obs_tm1 of every step, one per column; the belief of the sequence lives in column 0
        obs = tl.state_from_canonical(lv, A, cs.K, P, g["st_agents_%d" % q], g["st_items_%d" % q],
                                      g["st_t_%d" % q]).reshape(-1, P)
        one = CpuStepper(lv, A, 1, nthreads=1)
        b, s = tb.new_buffers(S, one.pitch)
        b, s, _, amap, info = tb.host_call(one, None, None, None, rows, pair, me, INIT, b, s)
        assert info[0] == tb.REINIT | tb.JOINT
        for t in range(T):
            prev = np.zeros((obs.shape[0], one.pitch), np.uint8)
            prev[:, 0] = obs[:, t]
            tk = np.full((A, one.pitch), 4, np.uint8)
            tk[:, 0] = taken[t, :A]
            before = tb.live_matrix(*tb.unpack(s, S, 1)[1:], S)[:, :, 0]
            b, s, _, amap, info = tb.host_call(one, prev.reshape(-1), tk.reshape(-1), None, rows, pair, me, 0, b, s)
            got_live = tb.live_matrix(*tb.unpack(s, S, 1)[1:], S)[:, :, 0]
            where = (level, me, t)
            assert np.array_equal(got_live, live[t].reshape(N, N) != 0), (where, got_live, live[t])
            assert bool(info[0] & tb.RAISED) == bool(rz[t]), (where, info[0], rz[t])
            assert bool(info[0] & tb.EMPTY) == (not got_live.any()), where
            assert bool(info[0] & tb.PRUNED) == bool((before & ~got_live).any()), where
            got = np.where(got_live, b[:, 0].reshape(N, N), 0.0)
            want = bel[t].reshape(N, N)
            assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (where, got, want)
            n["pruned"] += int((before & ~got_live).any())
            n["raised"] += int(rz[t])
            n["empty"] += int(not got_live.any())
            n["joint"] += int(bool(info[0] & tb.JOINT))
            n["split"] += int(got_live.any() and not info[0] & tb.JOINT)
    print("fixture: %d sequences" % nseq, n)
    assert n["pruned"] >= 20 and n["raised"] >= 20 and n["joint"] >= 50 and n["split"] >= 50 and n["empty"] >= 10
