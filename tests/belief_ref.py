"""Numpy restatement of oc_belief_update (the rule in include/oc_engine.h), built from code that is
already pinned and not from the engine's row function: oc_cpu_nav_policy's `probs` with
OC_POLICY_COUNT_STATE, one hypothesis per call, for L_i and the raise test; the CPU oracle's
subtask_bounds for doable; oc_cpu_progress for the events; plain f64 numpy in the stated order.  And
the closed scripted-partner loop the host and the GPU tests share: task_select -> nav_policy per
scripted agent -> step -> masked reset_random -> belief_update with events, on the host."""
from __future__ import annotations

import ctypes

import numpy as np

from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

from oracle import oracle

import taskselect_ref as tsr

INIT = capi.OC_BELIEF_INIT
UPDATED, PRUNED, REINIT, RESET, RAISED = (capi.BELF_UPDATED, capi.BELF_PRUNED, capi.BELF_REINIT, capi.BELF_RESET,
                                          capi.BELF_RAISED)
GUARD_BS, GUARD_MAP, GUARD_INFO, GUARD_BELIEF = 0xC3, 0x5A, 0xA5, -7.25
RTOL = 1e-12  # numpy's sums and the libm exp against the row function's


def bits(planes: np.ndarray, n: int) -> np.ndarray:
    """bool [n, B] of the bit set in u8 [planes, B] (bit b of plane c is 8c + b)."""
    return np.array([(planes[i >> 3] >> (i & 7)) & 1 for i in range(n)], bool)


def pack(b: np.ndarray, planes: int) -> np.ndarray:
    out = np.zeros((planes, b.shape[1]), np.uint8)
    for i in range(b.shape[0]):
        out[i >> 3] |= b[i].astype(np.uint8) << (i & 7)
    return out


class Ref:
    """The rule over (OracleBatch, CpuStepper) of one level; counts the branches for the tests."""

    def __init__(self, ob: oracle.OracleBatch, cs: CpuStepper, rows, agents, beta: float = 1.3, nap: float = 0.5):
        self.ob, self.cs, self.rows, self.agents = ob, cs, rows, [int(a) for a in agents]
        self.S, self.M, self.B, self.P = len(rows), len(agents), ob.B, ob.pitch
        self.HP = capi.belief_planes(self.S)
        self.beta, self.nap = beta, nap
        self.kind = np.array([r.kind for r in rows])
        self.per_agent = [tsr.agent_rows(rows, a) for a in self.agents]
        self.fl_plane = capi.layout_planes(ob.A, ob.K, ob.wide)["flags"]
        self.n = dict(reinit=0, reset=0, pruned=0, raised=0, updated=0, none_map=0, single=0)

    def probs(self, prev, row):
        """(p f64 [5, B], flags u8 [B]) of oc_cpu_nav_policy for one configuration on every env."""
        P, B = self.P, self.B
        p = np.zeros((5, P), np.float64)
        pf = np.zeros(P, np.uint8)
        act = np.full(self.ob.A * P, 4, np.uint8)
        self.cs.nav_policy(prev, [row], act, self.beta, self.nap, capi.OC_POLICY_GREEDY | capi.OC_POLICY_COUNT_STATE,
                           None, 0, 0, 0, p, 5, pf)
        return p[:, :B], pf[:B]

    def update(self, prev, taken, events, flags: int, belief: np.ndarray, bstate: np.ndarray):
        """(belief', bstate', map u8 [M, B], info u8 [M, B]) of one call; the inputs (belief f64
        [M, S + 1, P], bstate u8 [M, 2 HP, P]) are not modified.  events: u8 [EP, P] or None."""
        S, M, B, P, HP = self.S, self.M, self.B, self.P, self.HP
        bel, bs = belief.copy(), bstate.copy()
        e = np.arange(B)
        init = np.zeros(B, bool)
        if flags & INIT:
            init[:] = True
        else:
            init = (prev.reshape(-1, P)[self.fl_plane, :B] & capi.OC_FLAG_DONE) != 0
        ev = np.zeros((S + 1, B), bool)
        if events is not None and not flags & INIT:
            ev[:S] = bits(events[:, :B], S)
        fresh = np.append(self.kind != capi.SUB_NONE, True)
        amap = np.zeros((M, B), np.uint8)
        info = np.zeros((M, B), np.uint8)
        for m, a in enumerate(self.agents):
            opn, live = bits(bs[m, :HP, :B], S + 1), bits(bs[m, HP:, :B], S + 1)
            b = bel[m, :, :B].copy()
            opn[:, init] = fresh[:, None]
            reset = ~init & (ev & opn).any(0)
            opn[:, reset] &= ~ev[:, reset]
            uni = init | reset
            live[:, uni] = opn[:, uni]
            with np.errstate(divide="ignore"):
                b[:, uni] = np.where(live[:, uni], 1.0 / live[:, uni].sum(0), 0.0)
            fl = init * REINIT | reset * RESET
            upd = ~uni
            if upd.any():
                t = np.minimum(taken.reshape(-1, P)[a, :B], 4).astype(np.int64)
                _, doable = self.ob.subtask_bounds(prev, self.per_agent[m])
                prune = live[:S] & (doable[:, :B] == 0) & upd
                live[:S] &= ~prune
                b[:S][prune] = 0.0
                fl = fl | prune.any(0) * PRUNED
                any_sub = live[:S].any(0)
                # the raise test: any subtask row of the agent (the Level-0 view and legality do
                # not depend on the subtask); p > 0 exactly on the legal candidates
                p, pf = self.probs(prev, capi.subtask(capi.SUB_CHOP, [a], [1, 0], 0x11))
                raises = upd & any_sub & ((pf != capi.POL_OK) | (p[t, e] == 0.0))
                mul = upd & ~raises
                pn, pfn = self.probs(prev, capi.subtask(capi.SUB_NONE, [a], [0, 0], 0))
                assert (pfn == capi.POL_OK).all()
                for i in range(S + 1):
                    w = mul & live[i]
                    if not w.any():
                        continue
                    if i < S and self.kind[i] != capi.SUB_NONE:
                        pi, pfi = self.probs(prev, self.per_agent[m][i])
                        assert (pfi[w] == capi.POL_OK).all()
                        li = pi[t, e]
                    else:  # p(no-op), or p of each movable action (0 when there is none)
                        li = np.where(t == 4, pn[4], pn[:4].max(0))
                    b[i, w] = b[i, w] * li[w]
                total = np.zeros(B, np.float64)
                for i in range(S + 1):
                    total = np.where(live[i], total + b[i], total)
                n_live = live.sum(0)
                with np.errstate(divide="ignore"):
                    r = np.where(total == 0.0, 1.0 / n_live, 1.0 / total)
                for i in range(S + 1):
                    w = upd & live[i]
                    b[i, w] = np.where(total == 0.0, r, b[i] * r)[w]
                fl = fl | raises * RAISED | mul * UPDATED
                self.n["raised"] += int(raises.sum())
                self.n["updated"] += int(mul.sum())
                self.n["pruned"] += int((prune.any(0)).sum())
            self.n["reinit"] += int(init.sum())
            self.n["reset"] += int(reset.sum())
            best = np.where(live, b, -1.0).argmax(0)  # the first of equal maxima
            self.n["none_map"] += int((best == S).sum())
            self.n["single"] += int((live.sum(0) == 1).sum())
            amap[m], info[m] = best, fl
            bel[m, :, :B] = b
            bs[m, :HP, :B], bs[m, HP:, :B] = pack(opn, HP), pack(live, HP)
        return bel, bs, amap, info


def host_call(cs: CpuStepper, prev, taken, events, rows, agents, flags: int, belief, bstate, beta=1.3, nap=0.5,
              want_map=True, want_info=True, nthreads=None):
    """(belief', bstate', map [M, P] or None, info [M, P] or None) of oc_cpu_belief_update on copies;
    map prefilled with GUARD_MAP and info with GUARD_INFO."""
    M, P = len(agents), cs.pitch
    bel, bs = belief.copy(), bstate.copy()
    amap = np.full((M, P), GUARD_MAP, np.uint8) if want_map else None
    info = np.full((M, P), GUARD_INFO, np.uint8) if want_info else None
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    ags = (ctypes.c_uint8 * M)(*[int(a) for a in agents])
    capi.check(cs.lib.oc_cpu_belief_update(cs._h, p(prev), p(taken), p(events), capi.subtask_array(rows), len(rows), ags,
                                           M, float(beta), float(nap), int(flags), p(bel), p(bs), p(amap), p(info), cs.B,
                                           cs.nthreads if nthreads is None else nthreads))
    return bel, bs, amap, info


def check_map(belief, bstate, amap, S: int, B: int, where=""):
    """map is the lowest live index holding the maximum of the call's own beliefs."""
    HP = capi.belief_planes(S)
    for m in range(belief.shape[0]):
        live = bits(bstate[m, HP:, :B], S + 1)
        want = np.where(live, belief[m, :, :B], -1.0).argmax(0)
        assert np.array_equal(amap[m, :B], want), (where, m, np.argwhere(amap[m, :B] != want)[:5])


def assert_equal(got, ref, S: int, B: int, where=""):
    """A call's outputs against the restatement's: the whole bstate (guard columns included),
    info, beliefs to RTOL, map against the call's own beliefs; guards past column B intact."""
    bel, bs, amap, info = got
    rbel, rbs, _, rinfo = ref
    assert np.array_equal(bs, rbs), (where, np.argwhere(bs != rbs)[:5])
    assert np.array_equal(info[:, :B], rinfo), (where, np.argwhere(info[:, :B] != rinfo)[:5])
    err = np.abs(bel[:, :, :B] - rbel[:, :, :B])
    assert (err <= RTOL * np.abs(rbel[:, :, :B])).all(), (where, err.max())
    assert np.array_equal(bel[:, :, B:], rbel[:, :, B:]), where
    check_map(bel, bs, amap, S, B, where)
    assert (amap[:, B:] == GUARD_MAP).all() and (info[:, B:] == GUARD_INFO).all(), where


def new_buffers(M: int, S: int, P: int):
    """(belief, bstate) filled with guard values: INIT must overwrite every column below B."""
    return (np.full((M, S + 1, P), GUARD_BELIEF, np.float64),
            np.full((M, 2 * capi.belief_planes(S), P), GUARD_BS, np.uint8))


def closed_loop(level, A: int, agents, B: int, steps: int, rows=None, max_T: int = 100, seed: int = 7,
                what: int = capi.OC_START_AGENTS | capi.OC_START_ITEMS, use_events: bool = True, record_every: int = 0,
                check: bool = True, scripted=None, on_step=None, eps: float = 0.1):
    """The scripted-partner loop on the host with the belief update after every step.  The agents
    `scripted` (default: the watched `agents`) follow oc_task_select / oc_nav_policy, except that
    with probability `eps` per env and step they act uniformly at random (as the fixture's
    GoalPolicy does: an action outside get_actions is what makes prob_nav_actions raise); the
    others always act uniformly at random.  At every step the host call is compared with the restatement
    (`check`).  Returns (Ref with its counters, records): every `record_every`-th call's (prev,
    taken, events, call flags, belief before, bstate before, belief, bstate, map, info) as copies
    (call 0 is the INIT call: prev, taken, events None).  on_step(t, cur u8 [Ms, B], map u8 [M, B])
    sees the scripted agents' subtask of the step and the map after it."""
    import oc_testlib as tl
    lv = tl.load_level(level) if isinstance(level, str) else level
    rows = tsr.level_rows(lv) if rows is None else rows
    scripted = list(agents) if scripted is None else list(scripted)
    cs = CpuStepper(lv, A, B, max_T=max_T, nthreads=4)
    ob = oracle.OracleBatch(lv, A, max_T, B)
    ref = Ref(ob, cs, rows, agents)
    P, M, S, Ms = cs.pitch, len(agents), len(rows), len(scripted)
    TP, EP = capi.task_planes(S), capi.event_planes(S)
    task_rows = tsr.level_rows(lv)  # the scripted agents follow the level's own subtasks, whatever table is watched
    tables = [tsr.policy_table(task_rows, a) for a in scripted]
    rng = np.random.default_rng(seed)
    s, s2 = cs.new_state(), cs.new_state()
    cs.reset_random(s, None, seed, 0, what)
    ts = np.full((Ms, TP, P), 0, np.uint8)
    bel, bs = new_buffers(M, S, P)
    records = []

    def call(prev, taken, events, fl, t):
        nonlocal bel, bs
        got = host_call(cs, prev, taken, events, rows, agents, fl, bel, bs)
        if check:
            assert_equal(got, ref.update(prev, taken, events, fl, bel, bs), S, B, "step %d" % t)
        if record_every and t % record_every == 0:
            c = lambda a: None if a is None else a.copy()  # noqa: E731
            records.append((c(prev), c(taken), c(events), fl, bel.copy(), bs.copy(), got[0].copy(), got[1].copy(),
                            got[2].copy(), got[3].copy()))
        bel, bs = got[0], got[1]
        return got[2]

    call(None, None, None, INIT, 0)
    prev = None
    mode = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE
    tflags = capi.OC_TASK_COMMIT | capi.OC_TASK_DISTINCT
    for t in range(steps):
        ts = tsr.host_call(cs, s, prev, task_rows, scripted, tflags | (capi.OC_TASK_INIT if t == 0 else 0), ts)[0]
        act = np.full((A, P), 4, np.uint8)
        act[:, :B] = rng.integers(0, 5, (A, B), dtype=np.uint8)
        rand = act.copy()
        act = act.reshape(-1)
        pf = np.zeros(P, np.uint8)
        for m in range(Ms):
            cs.nav_policy(s, tables[m], act, 1.3, 0.5, mode, np.ascontiguousarray(ts[m, EP]), t, seed, 0, None, 5, pf)
        slip = np.zeros((A, P), bool)
        slip[:, :B] = rng.random((A, B)) < eps
        act = np.where(slip, rand, act.reshape(A, P)).reshape(-1)
        ex = np.full(A * P, 4, np.uint8)
        cs.step(s, s2, act, ex)
        cs.reset_random(s2, s, seed, t + 1, what)
        events = None
        if use_events:
            events = np.ascontiguousarray(cs.progress(s, s2, rows, want=("events",))[1][0])
        amap = call(s, ex, events, 0, t + 1)
        if on_step is not None:
            on_step(t, ts[:, EP, :B].copy(), amap[:, :B].copy())
        spare = cs.new_state() if prev is None else prev
        prev, s, s2 = s, s2, spare
    return ref, records
