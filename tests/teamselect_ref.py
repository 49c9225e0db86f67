"""Numpy restatement of oc_team_select (the rule in include/oc_engine.h), built on the CPU oracle's
subtask_bounds over the three row sets (a0's one-agent rows, a1's, the two-agent rows) and
oc_cpu_progress's counts, not on the engine's row function; and the closed team loop the host and
the GPU tests share: team_select -> three nav_policy calls (a0's table on plane cur0, a1's on cur1,
the two-agent table on curJ) -> step -> masked reset_random, on the host, with the host call
checked against the restatement at every step."""
from __future__ import annotations

import ctypes

import numpy as np

import taskselect_ref as tr
from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

from oracle import oracle

INIT, COMMIT, SPLIT_FIRST = capi.OC_TEAM_INIT, capi.OC_TEAM_COMMIT, capi.OC_TEAM_SPLIT_FIRST
COMPLETED0, COMPLETED1, SWITCHED = capi.TEAMF_COMPLETED0, capi.TEAMF_COMPLETED1, capi.TEAMF_SWITCHED
REINIT, JOINT, IDLE = capi.TEAMF_REINIT, capi.TEAMF_JOINT, capi.TEAMF_IDLE
OUT = capi.OC_TEAM_OUT
GUARD_TS, GUARD_INFO = 0xC3, 0xA5

level_rows = tr.level_rows


def config_rows(rows, agents):
    """The S subtask rows as configurations of `agents` (one or two): what the rule evaluates.  A
    None row stays a one-agent row (it is never a candidate)."""
    return [capi.subtask(r.kind, list(agents) if r.kind != capi.SUB_NONE else [agents[0]],
                         [r.start_mask[0], r.start_mask[1]], r.goal_mask) for r in rows]


def policy_tables(rows, pair):
    """oc_nav_policy's three tables for the planes cur0, cur1, curJ and their num_cand."""
    none = lambda a: [capi.subtask(capi.SUB_NONE, [a], [0, 0], 0)]  # noqa: E731
    return ((config_rows(rows, [pair[0]]) + none(pair[0]), 5), (config_rows(rows, [pair[1]]) + none(pair[1]), 5),
            (config_rows(rows, list(pair)), 25))


class Ref:
    """The rule over (OracleBatch, CpuStepper) of one level; counts what happened for the tests."""

    def __init__(self, ob: oracle.OracleBatch, cs: CpuStepper, rows, pair):
        self.ob, self.cs, self.rows, self.pair = ob, cs, rows, (int(pair[0]), int(pair[1]))
        self.S, self.B, self.P = len(rows), ob.B, ob.pitch
        self.EP = capi.event_planes(self.S)
        self.kind = np.array([r.kind for r in rows])
        self.sets = (config_rows(rows, [self.pair[0]]), config_rows(rows, [self.pair[1]]), config_rows(rows, self.pair))
        self.fl_plane = capi.layout_planes(ob.A, ob.K, ob.wide)["flags"]
        self.n = dict(joint=0, split=0, idle=0, completed=0, dropped=0, reinit=0, joint_to_split=0, deliver=0,
                      same_first=0, kept=0, calls=0, dropped_full=0)

    def _top2(self, C, lb):
        """(w f64 [S, B] with -1.0 where not a candidate, first [B], second [B]); argmax takes the
        first of equal maxima: ties to the lowest index."""
        S, e = self.S, np.arange(self.B)
        with np.errstate(divide="ignore"):
            w = np.where(C, 1.0 / lb.astype(np.float64), -1.0)
        first = np.where(C.any(0), w.argmax(0), S)
        C2 = C.copy()
        C2[first[first < S], e[first < S]] = False
        second = np.where(C2.any(0), np.where(C2, w, -1.0).argmax(0), S)
        return w, first, second

    def _at(self, table, idx, none):
        """table[idx[e], e] where idx < S, else `none`."""
        S, e = self.S, np.arange(self.B)
        return np.where(idx < S, table[np.minimum(idx, S - 1), e], none)

    def select(self, state, prev, flags: int, tstate: np.ndarray):
        """(tstate', bound f32 [2, B], info u8 [B]) of one call; `tstate` u8 [TP, P] is not modified."""
        S, B, P, EP = self.S, self.B, self.P, self.EP
        ts = tstate.copy()
        e = np.arange(B)
        init = np.zeros(B, bool)
        if flags & INIT:
            init[:] = True
        elif prev is not None:
            init = (prev.reshape(-1, P)[self.fl_plane, :B] & capi.OC_FLAG_DONE) != 0
        counts = self.cs.progress(state, state, self.rows, want=("counts",))[0][0, :, :B].astype(np.int64)
        (lb0, d0), (lb1, d1), (lbJ, dJ) = (self.ob.subtask_bounds(state, rows) for rows in self.sets)
        inc = np.zeros((S, B), bool)
        for i in range(S):
            inc[i] = (ts[i >> 3, :B] >> (i & 7)) & 1
        cur0, cur1, curJ, cnt0, cnt1 = (ts[EP + q, :B].astype(np.int64) for q in range(5))
        # 1. initialise
        inc[:, init], cur0[init], cur1[init], curJ[init], cnt0[init], cnt1[init] = True, S, S, OUT, 0, 0
        entry = (cur0.copy(), cur1.copy(), curJ.copy())
        # 2. refresh
        joint = curJ < S
        doneJ = joint & (self._at(counts, curJ, 0) > cnt0)
        done0 = ~joint & (cur0 < S) & (self._at(counts, cur0, 0) > cnt0)
        done1 = ~joint & (cur1 < S) & (self._at(counts, cur1, 0) > cnt1)
        for done, cur in ((doneJ, curJ), (done0, cur0), (done1, cur1)):
            inc[cur[done], e[done]] = False
            self.n["deliver"] += int((done & (self._at(self.kind[:, None].repeat(B, 1), cur, 0) == capi.SUB_DELIVER)).sum())
        comp0, comp1 = doneJ | done0, doneJ | done1
        gone = comp0 | comp1
        cur0[gone], cur1[gone], curJ[gone] = S, S, OUT
        # 3. candidates
        opn = inc & (self.kind != capi.SUB_NONE)[:, None]
        C0, C1, CJ = opn & (d0 != 0), opn & (d1 != 0), opn & (dJ != 0)
        w0, f0, s0 = self._top2(C0, lb0)
        w1, f1, s1 = self._top2(C1, lb1)
        wJ, iJ, _ = self._top2(CJ, lbJ)
        # 4. keep
        joint = curJ < S
        full = (cur0 < S) & (cur1 < S)
        still = np.where(joint, self._at(CJ, curJ, False), full & self._at(C0, cur0, False) & self._at(C1, cur1, False))
        keep = still & ~gone if flags & COMMIT else np.zeros(B, bool)
        if flags & COMMIT:
            # a commitment dropped (oc_task_select's `has & ~stays`): after step 2 the allocation names
            # a subtask and step 4 does not keep it; dropped_full: of those, the joint and two-subtask
            # ones, where a member stopped being a candidate (one with a None member is never kept)
            self.n["dropped"] += int(((joint | (cur0 < S) | (cur1 < S)) & ~gone & ~still).sum())
            self.n["dropped_full"] += int(((joint | full) & ~gone & ~still).sum())
        # 5. picks
        have = (f0 < S) | (f1 < S)
        same = have & (f0 == f1)
        x = self._at(w0, f0, 0.0) + self._at(w1, s1, 0.0)
        y = self._at(w0, s0, 0.0) + self._at(w1, f1, 0.0)
        p0 = np.where(same & ~(x >= y), s0, f0)
        p1 = np.where(same & (x >= y), s1, f1)
        wS = self._at(w0, p0, 0.0) + self._at(w1, p1, 0.0)
        wj = self._at(wJ, iJ, 0.0)
        # 6. choose
        has_j = iJ < S
        split_first = bool(flags & SPLIT_FIRST) & have & (p0 < S) & (p1 < S)
        take_j = ~split_first & has_j & (~have | (wj >= wS))
        take_s = ~take_j & have
        idle = ~keep & ~take_j & ~take_s
        n0 = np.where(take_j, OUT, np.where(take_s, p0, S))
        n1 = np.where(take_j, OUT, np.where(take_s, p1, S))
        nJ = np.where(take_j, iJ, OUT)
        cur0, cur1, curJ = np.where(keep, cur0, n0), np.where(keep, cur1, n1), np.where(keep, curJ, nJ)
        # 7. counts and flags
        sw = (cur0 != entry[0]) | (cur1 != entry[1]) | (curJ != entry[2])
        joint = curJ < S
        cnt0 = np.where(sw, np.where(joint, self._at(counts, curJ, 0), self._at(counts, cur0, 0)), cnt0)
        cnt1 = np.where(sw, np.where(joint, 0, self._at(counts, cur1, 0)), cnt1)
        bound = np.zeros((2, B), np.float32)
        bound[0] = np.where(joint, self._at(lbJ, curJ, 0.0), self._at(lb0, cur0, 0.0))
        bound[1] = np.where(joint, self._at(lbJ, curJ, 0.0), self._at(lb1, cur1, 0.0))
        info = (comp0 * COMPLETED0 | comp1 * COMPLETED1 | sw * SWITCHED | init * REINIT | joint * JOINT | idle * IDLE)
        some = ~joint & ((cur0 < S) | (cur1 < S))
        n = self.n
        n["calls"] += B
        n["joint"] += int(joint.sum())
        n["split"] += int(some.sum())
        n["idle"] += int((~joint & ~some).sum())
        n["completed"] += int(gone.sum())
        n["reinit"] += int(init.sum())
        n["kept"] += int(keep.sum())
        n["joint_to_split"] += int(((entry[2] < S) & some).sum())
        n["same_first"] += int((~keep & same).sum())
        ts[:EP, :B] = 0
        for i in range(S):
            ts[i >> 3, :B] |= inc[i].astype(np.uint8) << (i & 7)
        for q, v in enumerate((cur0, cur1, curJ, cnt0, cnt1)):
            ts[EP + q, :B] = v
        return ts, bound, info.astype(np.uint8)


def host_call(cs: CpuStepper, state, prev, rows, pair, flags: int, tstate: np.ndarray, want_bound=True, want_info=True):
    """(tstate', bound [2, P] or None, info [P] or None) of oc_cpu_team_select on a copy of `tstate`;
    bound prefilled with NaN and info with GUARD_INFO."""
    P = cs.pitch
    ts = tstate.copy()
    bound = np.full((2, P), np.nan, np.float32) if want_bound else None
    info = np.full(P, GUARD_INFO, np.uint8) if want_info else None
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    ags = (ctypes.c_uint8 * 2)(int(pair[0]), int(pair[1]))
    capi.check(cs.lib.oc_cpu_team_select(cs._h, p(state), p(prev), capi.subtask_array(rows), len(rows), ags, int(flags),
                                         p(ts), p(bound), p(info), cs.B, cs.nthreads))
    return ts, bound, info


def assert_equal(got, ref, B: int, where=""):
    """The host (or device) call's outputs against the restatement's: the whole tstate (guard
    columns included: the restatement leaves them), bound bit-equal f32, info."""
    ts, bound, info = got
    rts, rbound, rinfo = ref
    assert np.array_equal(ts, rts), (where, np.argwhere(ts != rts)[:5])
    assert np.array_equal(bound[:, :B].view(np.uint32), rbound.view(np.uint32)), (where, np.argwhere(bound[:, :B] != rbound)[:5])
    assert np.array_equal(info[:B], rinfo), (where, np.argwhere(info[:B] != rinfo)[:5])
    assert np.isnan(bound[:, B:]).all() and (info[B:] == GUARD_INFO).all(), where


def closed_loop(level, A: int, pair, B: int, steps: int, flags: int, rows=None, max_T: int = 100, seed: int = 7,
                what: int = capi.OC_START_AGENTS | capi.OC_START_ITEMS, record_every: int = 0, check: bool = True,
                solo: bool = False):
    """The team loop on the host.  At every step the host call is compared with the restatement
    (`check`); agents outside `pair` act uniformly at random, and every env must be OK (or raise) in
    exactly the policy launches its allocation names and OC_POL_BADALLOC in the others.  `solo`: the
    same loop with oc_cpu_task_select (COMMIT | DISTINCT) making the choice, for the comparison of
    the two.  Returns (Ref with its counters, records, totals): every `record_every`-th step's
    (state, prev or None, call flags, tstate before, tstate after, bound, info) as copies; totals =
    dict(idle, env_steps, episodes, successes) of the loop itself."""
    import oc_testlib as tl
    lv = tl.load_level(level) if isinstance(level, str) else level
    rows = level_rows(lv) if rows is None else rows
    cs = CpuStepper(lv, A, B, max_T=max_T, nthreads=4)
    ob = oracle.OracleBatch(lv, A, max_T, B)
    ref = Ref(ob, cs, rows, pair)
    P, S = cs.pitch, len(rows)
    EP = capi.event_planes(S)
    tables = policy_tables(rows, pair)
    fl_plane = cs.layout.plane_flags
    rng = np.random.default_rng(seed)
    s, s2 = cs.new_state(), cs.new_state()
    cs.reset_random(s, None, seed, 0, what)
    ts = np.full((2, capi.task_planes(S), P) if solo else (capi.team_planes(S), P), GUARD_TS, np.uint8)
    prev, records = None, []
    totals = dict(idle=0, env_steps=0, episodes=0, successes=0)
    mode = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE
    for t in range(steps):
        if solo:
            fl = tr.COMMIT | tr.DISTINCT | (tr.INIT if t == 0 else 0)
            got = tr.host_call(cs, s, prev, rows, pair, fl, ts)
            ts = got[0]
            allocs = (ts[0, EP], ts[1, EP], np.full(P, OUT, np.uint8))
        else:
            fl = flags | (INIT if t == 0 else 0)
            got = host_call(cs, s, prev, rows, pair, fl, ts)
            if check:
                assert_equal(got, ref.select(s, prev, fl, ts), B, "step %d" % t)
            if record_every and t % record_every == 0:
                records.append((s.copy(), None if prev is None else prev.copy(), fl, ts.copy(), got[0].copy(), got[1].copy(),
                                got[2].copy()))
            ts = got[0]
            allocs = (ts[EP], ts[EP + 1], ts[EP + 2])
        c0, c1, cJ = (a[:B] for a in allocs)
        totals["idle"] += int(((cJ >= S) & (c0 >= S) & (c1 >= S)).sum())
        totals["env_steps"] += B
        act = np.full((A, P), 4, np.uint8)
        act[:, :B] = rng.integers(0, 5, (A, B), dtype=np.uint8)
        act = act.reshape(-1)
        for q, (table, ncand) in enumerate(tables):
            pf = np.full(P, GUARD_INFO, np.uint8)
            cs.nav_policy(s, table, act, 1.3, 0.5, mode, np.ascontiguousarray(allocs[q]), t, seed, 0, None, ncand, pf)
            mine = allocs[q][:B] < len(table)
            assert ((pf[:B] == capi.POL_OK) | (pf[:B] == capi.POL_RAISES))[mine].all(), (t, q)
            assert (pf[:B][~mine] == capi.POL_BADALLOC).all(), (t, q)
        cs.step(s, s2, act)
        f2 = s2.reshape(-1, P)[fl_plane, :B]
        totals["episodes"] += int(((f2 & capi.OC_FLAG_DONE) != 0).sum())
        totals["successes"] += int(((f2 & capi.OC_FLAG_SUCCESS) != 0).sum())
        cs.reset_random(s2, s, seed, t + 1, what)
        spare = cs.new_state() if prev is None else prev
        prev, s, s2 = s, s2, spare
    return ref, records, totals
