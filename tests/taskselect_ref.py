"""Numpy restatement of oc_task_select (the rule in include/oc_engine.h), built on the CPU oracle's
subtask_bounds (lb_i, doable_i) and oc_cpu_progress's counts (count_i), not on the engine's row
function; and the closed scripted-partner loop the host and the GPU tests share: task_select ->
nav_policy per scripted agent -> step -> masked reset_random, on the host, with the host call
checked against the restatement at every step."""
from __future__ import annotations

import ctypes

import numpy as np

from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

from oracle import oracle

INIT, COMMIT, DISTINCT = capi.OC_TASK_INIT, capi.OC_TASK_COMMIT, capi.OC_TASK_DISTINCT
COMPLETED, SWITCHED, REINIT = capi.TASKF_COMPLETED, capi.TASKF_SWITCHED, capi.TASKF_REINIT
GUARD_TS, GUARD_INFO = 0xC3, 0xA5


def agent_rows(rows, agent: int):
    """The S subtask rows as one-agent configurations of `agent` (what the rule evaluates)."""
    return [capi.subtask(r.kind, [agent], [r.start_mask[0], r.start_mask[1]], r.goal_mask) for r in rows]


def policy_table(rows, agent: int):
    """oc_nav_policy's table for a cur plane: the rows for `agent`, then None at index S."""
    return agent_rows(rows, agent) + [capi.subtask(capi.SUB_NONE, [agent], [0, 0], 0)]


class Ref:
    """The rule over (OracleBatch, CpuStepper) of one level; counts what happened for the tests."""

    def __init__(self, ob: oracle.OracleBatch, cs: CpuStepper, rows, agents):
        self.ob, self.cs, self.rows, self.agents = ob, cs, rows, [int(a) for a in agents]
        self.S, self.M, self.B, self.P = len(rows), len(agents), ob.B, ob.pitch
        self.EP = capi.event_planes(self.S)
        self.kind = np.array([r.kind for r in rows])
        self.per_agent = [agent_rows(rows, a) for a in self.agents]
        self.fl_plane = capi.layout_planes(ob.A, ob.K, ob.wide)["flags"]
        self.n = dict(completed=0, dropped=0, distinct=0, reinit=0, none=0, deliver=0)

    def select(self, state, prev, flags: int, tstate: np.ndarray):
        """(tstate', bound f32 [M, B], info u8 [M, B]) of one call; `tstate` u8 [M, TP, P] is not
        modified."""
        S, M, B, P, EP = self.S, self.M, self.B, self.P, self.EP
        ts = tstate.copy()
        e = np.arange(B)
        init = np.zeros(B, bool)
        if flags & INIT:
            init[:] = True
        elif prev is not None:
            init = (prev.reshape(-1, P)[self.fl_plane, :B] & capi.OC_FLAG_DONE) != 0
        counts = self.cs.progress(state, state, self.rows, want=("counts",))[0][0, :, :B].astype(np.int64)
        bound = np.zeros((M, B), np.float32)
        info = np.zeros((M, B), np.uint8)
        held = []  # DISTINCT: the cur of the earlier agents after their choice
        self.n["reinit"] += int(init.sum())
        for m in range(M):
            lb, doable = self.ob.subtask_bounds(state, self.per_agent[m])
            inc = np.zeros((S, B), bool)
            for i in range(S):
                inc[i] = (ts[m, i >> 3, :B] >> (i & 7)) & 1
            cur = ts[m, EP, :B].astype(np.int64)
            cnt = ts[m, EP + 1, :B].astype(np.int64)
            inc[:, init], cur[init], cnt[init] = True, S, 0
            entry = cur.copy()
            # 2. refresh
            has = cur < S
            done = has & (counts[np.minimum(cur, S - 1), e] > cnt)
            self.n["completed"] += int(done.sum())
            self.n["deliver"] += int((done & (self.kind[np.minimum(cur, S - 1)] == capi.SUB_DELIVER)).sum())
            inc[cur[done], e[done]] = False
            cur[done] = S
            # 3. candidates
            cand = inc & (self.kind != capi.SUB_NONE)[:, None] & (doable != 0)
            if flags & DISTINCT:
                free = cand.copy()
                for c in held:
                    t = c < S
                    cand[c[t], e[t]] = False
                self.n["distinct"] += int((free != cand).any(0).sum())
            # 4. choose
            best = np.where(cand, lb, np.float32(np.inf)).astype(np.float32)
            new = np.where(cand.any(0), best.argmin(0), S)  # argmin: the first of equal minima
            has = cur < S
            stays = has & cand[np.minimum(cur, S - 1), e]
            if flags & COMMIT:
                self.n["dropped"] += int((has & ~stays).sum())
                new = np.where(stays, cur, new)
            take = (new != cur) & (new < S)
            cnt = np.where(take, counts[np.minimum(new, S - 1), e], cnt)
            cur = new
            self.n["none"] += int((cur == S).sum())
            held.append(cur.copy())
            bound[m] = np.where(cur < S, lb[np.minimum(cur, S - 1), e], np.float32(0.0))
            info[m] = (done * COMPLETED) | ((cur != entry) * SWITCHED) | (init * REINIT)
            ts[m, :EP, :B] = 0
            for i in range(S):
                ts[m, i >> 3, :B] |= inc[i].astype(np.uint8) << (i & 7)
            ts[m, EP, :B], ts[m, EP + 1, :B] = cur, cnt
        return ts, bound, info


def host_call(cs: CpuStepper, state, prev, rows, agents, flags: int, tstate: np.ndarray, want_bound=True, want_info=True):
    """(tstate', bound [M, P] or None, info [M, P] or None) of oc_cpu_task_select on a copy of
    `tstate`; bound prefilled with NaN and info with GUARD_INFO."""
    M, P = len(agents), cs.pitch
    ts = tstate.copy()
    bound = np.full((M, P), np.nan, np.float32) if want_bound else None
    info = np.full((M, P), GUARD_INFO, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    ags = (ctypes.c_uint8 * M)(*[int(a) for a in agents])
    capi.check(cs.lib.oc_cpu_task_select(cs._h, p(state), p(prev), capi.subtask_array(rows), len(rows), ags, M, int(flags),
                                         p(ts), p(bound), p(info) if want_info else None, cs.B, cs.nthreads))
    return ts, bound, info if want_info else None


def assert_equal(got, ref, B: int, where=""):
    """The host (or device) call's outputs against the restatement's: the whole tstate (guard
    columns included: the restatement leaves them), bound bit-equal f32, info."""
    ts, bound, info = got
    rts, rbound, rinfo = ref
    assert np.array_equal(ts, rts), (where, np.argwhere(ts != rts)[:5])
    assert np.array_equal(bound[:, :B].view(np.uint32), rbound.view(np.uint32)), (where, np.argwhere(bound[:, :B] != rbound)[:5])
    assert np.array_equal(info[:, :B], rinfo), (where, np.argwhere(info[:, :B] != rinfo)[:5])
    assert np.isnan(bound[:, B:]).all() and (info[:, B:] == GUARD_INFO).all(), where


def level_rows(level):
    """oc_subtask rows of the level's recipes.all_subtasks."""
    from gym_cooking_amd import recipes
    return capi.progress_subtasks(recipes.all_subtasks(level), level.encoding)


def closed_loop(level, A: int, agents, B: int, steps: int, flags: int, rows=None, max_T: int = 100, seed: int = 7,
                what: int = capi.OC_START_AGENTS | capi.OC_START_ITEMS, record_every: int = 0, check: bool = True):
    """The scripted-partner loop on the host.  At every step the host call is compared with the
    restatement (`check`); agents outside `agents` act uniformly at random.  Returns (Ref with its
    counters, records): every `record_every`-th step's (state, prev or None, call flags, tstate
    before, tstate after, bound, info) as copies."""
    import oc_testlib as tl
    lv = tl.load_level(level) if isinstance(level, str) else level
    rows = level_rows(lv) if rows is None else rows
    cs = CpuStepper(lv, A, B, max_T=max_T, nthreads=4)
    ob = oracle.OracleBatch(lv, A, max_T, B)
    ref = Ref(ob, cs, rows, agents)
    P, M, S = cs.pitch, len(agents), len(rows)
    TP, EP = capi.task_planes(S), capi.event_planes(S)
    tables = [policy_table(rows, a) for a in agents]
    rng = np.random.default_rng(seed)
    s, s2 = cs.new_state(), cs.new_state()
    cs.reset_random(s, None, seed, 0, what)
    ts = np.full((M, TP, P), GUARD_TS, np.uint8)
    prev, records = None, []
    mode = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE
    for t in range(steps):
        fl = flags | (INIT if t == 0 else 0)
        got = host_call(cs, s, prev, rows, agents, fl, ts)
        if check:
            assert_equal(got, ref.select(s, prev, fl, ts), B, "step %d" % t)
        if record_every and t % record_every == 0:
            records.append((s.copy(), None if prev is None else prev.copy(), fl, ts.copy(), got[0].copy(), got[1].copy(),
                            got[2].copy()))
        ts = got[0]
        act = np.full((A, P), 4, np.uint8)
        act[:, :B] = rng.integers(0, 5, (A, B), dtype=np.uint8)
        act = act.reshape(-1)
        pf = np.zeros(P, np.uint8)
        for m in range(M):
            cs.nav_policy(s, tables[m], act, 1.3, 0.5, mode, np.ascontiguousarray(ts[m, EP]), t, seed, 0, None, 5, pf)
            assert ((pf[:B] == capi.POL_OK) | (pf[:B] == capi.POL_RAISES)).all()
        cs.step(s, s2, act)
        cs.reset_random(s2, s, seed, t + 1, what)
        spare = cs.new_state() if prev is None else prev
        prev, s, s2 = s, s2, spare
    return ref, records
