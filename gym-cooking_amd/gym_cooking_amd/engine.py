"""OvercookedBatch: B independent kitchens stepped by the HIP engine (torch ROCm buffers).

This is the batched counterpart of ``OvercookedEnvironment.reset/step``
(gym_cooking/envs/overcooked_environment.py:201-306).  All buffers are torch uint8/uint64
tensors on one GPU in the structure-of-arrays layout of include/oc_engine.h; every call is
enqueued on torch's current stream through the C-ABI (liboc_engine.so).  There is no CPU
fallback: without the built library or a GPU the constructor raises.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import capi
from . import levels as _levels


_U64 = (torch.uint64, torch.int64)
_OBS_DTYPES = {torch.uint8: capi.OC_OBS_U8, torch.float16: capi.OC_OBS_F16}


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bound(fn, args):
    """A zero-argument callable issuing fn(*args) and raising on its status: one ctypes call
    per launch (the arguments were validated and converted when it was made)."""
    check = capi.check

    def launch():
        check(fn(*args))
    return launch


class _StartCells:
    """oc_set_start_cells / oc_get_start_cells of a handle (OvercookedBatch and CpuStepper)."""

    def set_start_cells(self, agent_ok=None, item_ok=None) -> None:
        """The start distribution of reset_random: `agent_ok` [A, W*H] (non-zero: agent i may start
        on the Floor cell) and `item_ok` [W*H] (non-zero: an item may start on the Counter cell);
        None is the default (agent i: the Floor cells connected to spawn i; items: the Counters
        with a Floor neighbour).  Not stream-ordered: earlier calls on the handle must have
        completed.  A mask the engine refuses raises with its message."""
        cells = self.level.width * self.level.height

        def mask(m, n):
            if m is None:
                return None
            m = np.ascontiguousarray(np.asarray(m) != 0, dtype=np.uint8).reshape(-1)
            if m.size != n:
                raise ValueError("start mask: %d cells, expected %d" % (m.size, n))
            return m
        a, i = mask(agent_ok, self.A * cells), mask(item_ok, cells)
        capi.check(self.lib.oc_set_start_cells(self._h, None if a is None else a.ctypes.data,
                                               None if i is None else i.ctypes.data))

    def start_cells(self):
        """The effective masks (agent_ok u8 [A, W*H], item_ok u8 [W*H]), defaults included."""
        cells = self.level.width * self.level.height
        a, i = np.zeros((self.A, cells), np.uint8), np.zeros(cells, np.uint8)
        capi.check(self.lib.oc_get_start_cells(self._h, a.ctypes.data, i.ctypes.data))
        return a, i


class OvercookedBatch(_StartCells):
    """B envs of one level on one GPU.

    Args:
        level: builtin level name, level-file path, or :class:`levels.Level`.
        num_agents: A (1..4).
        B: batch size (envs on this device).
        max_T: ``--max-num-timesteps`` (main.py:24; 0 = unlimited).
        device: torch device (``cuda:N``).
    """

    def __init__(self, level, num_agents: int, B: int, max_T: int = 100, device="cuda:0"):
        if isinstance(level, str):
            level = _levels.load_level(level)
        self.level = level
        self.A = num_agents
        self.B = int(B)
        self.max_T = max_T
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("OvercookedBatch runs on the GPU only (no CPU fallback)")
        self.lib = capi.load_library()
        self._desc = capi.level_desc(level, num_agents)
        h = ctypes.c_void_p()
        capi.check(self.lib.oc_create(ctypes.byref(self._desc), num_agents, max_T,
                                      self.device.index or 0, ctypes.byref(h)))
        self._h = h
        lay = capi.OcLayout()
        capi.check(self.lib.oc_get_layout(self._h, self.B, ctypes.byref(lay)))
        self.layout = lay
        self.K = lay.num_items
        self.pitch = lay.pitch
        n = ctypes.c_int64()
        capi.check(self.lib.oc_stats_size(self._h, self.B, ctypes.byref(n)))
        self.stats_bytes = n.value

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and getattr(self, "lib", None) is not None:
            self.lib.oc_destroy(h)
            self._h = None

    # ---- buffers ---------------------------------------------------------------------
    def new_state(self) -> torch.Tensor:
        return torch.empty(self.layout.state_bytes, dtype=torch.uint8, device=self.device)

    def new_actions(self, steps: int = 1) -> torch.Tensor:
        return torch.full((steps, self.A * self.pitch), 4, dtype=torch.uint8, device=self.device).squeeze(0)

    def new_exec(self) -> torch.Tensor:
        return torch.empty(self.A * self.pitch, dtype=torch.uint8, device=self.device)

    def new_coll(self) -> torch.Tensor:
        return torch.empty(self.pitch, dtype=torch.uint8, device=self.device)

    def new_stats(self) -> torch.Tensor:
        """A zeroed statistics buffer.  Besides the partial rows it holds step_n's completion
        counters, which must be zero when a launch with `totals` starts (every completed launch
        leaves them zero): zero it again after a faulted launch, and do not share one buffer
        between concurrent step_n calls on different streams."""
        return torch.zeros(self.stats_bytes // 8, dtype=torch.uint64, device=self.device)

    def new_obs(self, dtype=torch.uint8) -> torch.Tensor:
        """[B, C, H, W] observation planes (oc_observe): torch.uint8 or torch.float16."""
        if dtype not in _OBS_DTYPES:
            raise TypeError("observation dtype %s, expected torch.uint8 or torch.float16" % dtype)
        return torch.empty((self.B, capi.obs_channels(self.A), self.level.height, self.level.width), dtype=dtype,
                           device=self.device)

    def new_action_mask(self) -> torch.Tensor:
        """[A * pitch] u8 legal-move masks (oc_observe): agent a's envs at [a * pitch, a * pitch + B)."""
        return torch.empty(self.A * self.pitch, dtype=torch.uint8, device=self.device)

    def new_progress_buffers(self, num_subtasks: int, n: int = 1):
        """(counts u8 [n, S, pitch], events u8 [n, planes, pitch], reward f32 [n, pitch]) for
        oc_progress over `num_subtasks` subtasks and n steps."""
        P = self.pitch
        return (torch.empty((n, num_subtasks, P), dtype=torch.uint8, device=self.device),
                torch.empty((n, capi.event_planes(num_subtasks), P), dtype=torch.uint8, device=self.device),
                torch.empty((n, P), dtype=torch.float32, device=self.device))

    def planes(self, state: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Named views of a state buffer ([A|K, pitch] u8 planes; t is [pitch] u16)."""
        L, P, A, K = self.layout, self.pitch, self.A, self.K
        s = state.view(L.num_planes, P)
        return dict(
            agent_x=s[L.plane_agent_x:L.plane_agent_x + A], agent_y=s[L.plane_agent_y:L.plane_agent_y + A],
            agent_hold=s[L.plane_agent_hold:L.plane_agent_hold + A],
            item_loc=s[L.plane_item_loc:L.plane_item_loc + K], item_mask=s[L.plane_item_mask:L.plane_item_mask + K],
            t=s[L.plane_t:L.plane_t + 2].reshape(-1).view(torch.int16)[:P], flags=s[L.plane_flags],
        )

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- hot path ----------------------------------------------------------------------
    def reset(self, state: torch.Tensor) -> torch.Tensor:
        """Broadcast the level template (reset(), overcooked_environment.py:201-250)."""
        self._check(state, self.layout.state_bytes)
        capi.check(self.lib.oc_reset(self._h, _ptr(state), self.B, self._stream()))
        return state

    def reset_random(self, state: torch.Tensor, prev: Optional[torch.Tensor] = None, seed: int = 0, round: int = 0,
                     what: int = 3, env_offset: int = 0) -> torch.Tensor:
        """Randomised starts (oc_reset_random): per env the agents on drawn Floor cells
        (what & capi.OC_START_AGENTS) and the level's items on drawn Counter cells
        (what & capi.OC_START_ITEMS), the reset of the level file with its item letters and spawn
        lines moved there.  With `prev` only the envs whose `prev` flags carry DONE are rewritten
        (after step(prev, state): exactly the envs the step auto-reset; `prev` may be `state`).
        The draw depends on (seed, round, env_offset + env) only."""
        self.reset_random_launcher(state, prev, seed, round, what, env_offset)()
        return state

    def reset_random_launcher(self, state: torch.Tensor, prev: Optional[torch.Tensor] = None, seed: int = 0,
                              round: int = 0, what: int = 3, env_offset: int = 0):
        """An oc_reset_random call bound once (see rollout_launcher)."""
        self._check(state, self.layout.state_bytes)
        if prev is not None:
            self._check(prev, self.layout.state_bytes)
        mask = (1 << 64) - 1
        args = (self._h, _ptr(state), _ptr(prev), self.B, int(env_offset), int(seed) & mask, int(round) & mask,
                int(what), self._stream())
        return _bound(self.lib.oc_reset_random, args)

    def step(self, state_in: torch.Tensor, state_out: torch.Tensor, actions: torch.Tensor,
             exec_out: Optional[torch.Tensor] = None, coll: Optional[torch.Tensor] = None,
             stats: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One step of every env (step(), overcooked_environment.py:255-306)."""
        self._check(state_in, self.layout.state_bytes)
        self._check(state_out, self.layout.state_bytes)
        self._check(actions, self.A * self.pitch)
        if exec_out is not None:
            self._check(exec_out, self.A * self.pitch)
        if coll is not None:
            self._check(coll, self.pitch)
        if stats is not None:
            self._check(stats, self.stats_bytes, _U64)
        capi.check(self.lib.oc_step(self._h, _ptr(state_in), _ptr(state_out), _ptr(actions), _ptr(exec_out),
                                    _ptr(coll), _ptr(stats), self.B, self._stream()))
        return state_out

    def step_n(self, state_in: torch.Tensor, state_out: torch.Tensor, actions: torch.Tensor, n: int,
               traj: Optional[torch.Tensor] = None, exec_out: Optional[torch.Tensor] = None,
               coll: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
               totals: Optional[torch.Tensor] = None) -> torch.Tensor:
        """n consecutive steps in one launch (oc_step_n): identical outputs to n step() calls.
        With `totals` (int64 [OC_NSTATS], needs `stats`) the launch also folds the statistics
        into it, as reduce_stats() after it would."""
        self.step_n_launcher(state_in, state_out, actions, n, traj, exec_out, coll, stats, totals)()
        return state_out

    def step_n_launcher(self, state_in: torch.Tensor, state_out: torch.Tensor, actions: torch.Tensor, n: int,
                        traj: Optional[torch.Tensor] = None, exec_out: Optional[torch.Tensor] = None,
                        coll: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
                        totals: Optional[torch.Tensor] = None):
        """Validate the buffers of an oc_step_n call once and return a zero-argument callable
        that issues it (the buffers must stay alive and unchanged in shape): a repeated launch
        then costs one ctypes call, no per-call checks.  The stream is bound here: the callable
        launches on the stream that was current when it was made, whichever is current later."""
        self._check(state_in, self.layout.state_bytes)
        self._check(state_out, self.layout.state_bytes)
        self._check(actions, n * self.A * self.pitch)
        if traj is not None:
            self._check(traj, n * self.layout.state_bytes)
        if exec_out is not None:
            self._check(exec_out, n * self.A * self.pitch)
        if coll is not None:
            self._check(coll, n * self.pitch)
        if stats is not None:
            self._check(stats, self.stats_bytes, _U64)
        if totals is not None:
            if stats is None:
                raise ValueError("totals need the stats buffer")
            self._check(totals, 8 * capi.OC_NSTATS, _U64)
        args = (self._h, _ptr(state_in), _ptr(state_out), _ptr(actions), _ptr(traj), _ptr(exec_out), _ptr(coll),
                _ptr(stats), _ptr(totals), self.B, int(n), self._stream())
        return _bound(self.lib.oc_step_n, args)

    def rollout(self, state_in: torch.Tensor, state_out: torch.Tensor, actions: torch.Tensor, subtasks,
                alloc: Optional[torch.Tensor] = None, flags: Optional[torch.Tensor] = None,
                lower_bound: Optional[torch.Tensor] = None):
        """Navigation-planner rollout rows (oc_rollout): the Level-0 next state of every row
        under its subtask configuration, and (flags u8 [pitch], lower bound f32 [pitch])."""
        flags = torch.empty(self.pitch, dtype=torch.uint8, device=self.device) if flags is None else flags
        lower_bound = (torch.empty(self.pitch, dtype=torch.float32, device=self.device)
                       if lower_bound is None else lower_bound)
        self.rollout_launcher(state_in, state_out, actions, subtasks, alloc, flags, lower_bound)()
        return flags, lower_bound

    def rollout_launcher(self, state_in: torch.Tensor, state_out: torch.Tensor, actions: torch.Tensor, subtasks,
                         alloc: Optional[torch.Tensor], flags: torch.Tensor, lower_bound: torch.Tensor):
        """An oc_rollout call bound once (buffers validated, the subtask table packed): the
        returned callable issues it on the stream current now with one ctypes call."""
        self._check(state_in, self.layout.state_bytes)
        self._check(state_out, self.layout.state_bytes)
        self._check(actions, self.A * self.pitch)
        if alloc is not None:
            self._check(alloc, self.pitch)
        self._check(flags, self.pitch)
        self._check(lower_bound, 4 * self.pitch, (torch.float32,))
        subs = capi.subtask_array(subtasks)
        args = (self._h, _ptr(state_in), _ptr(state_out), _ptr(actions), _ptr(alloc), subs, len(subtasks),
                _ptr(flags), _ptr(lower_bound), self.B, self._stream())
        return _bound(self.lib.oc_rollout, args)

    def nav_likelihood(self, state: torch.Tensor, taken: torch.Tensor, subtasks, self_agent: int,
                       beta: float = 1.3, none_action_prob: float = 0.5, alloc: Optional[torch.Tensor] = None):
        """Bayesian-delegation likelihoods (oc_nav_likelihood): prob_nav_actions of every row's
        allocation given the executed actions `taken` (u8 [A][pitch]); returns
        (likelihood f64 [pitch], flags u8 [pitch])."""
        out = torch.empty(self.pitch, dtype=torch.float64, device=self.device)
        flags = torch.empty(self.pitch, dtype=torch.uint8, device=self.device)
        self.nav_likelihood_launcher(state, taken, subtasks, self_agent, beta, none_action_prob, alloc, out, flags)()
        return out, flags

    def nav_likelihood_launcher(self, state: torch.Tensor, taken: torch.Tensor, subtasks, self_agent: int,
                                beta: float, none_action_prob: float, alloc: Optional[torch.Tensor],
                                out: torch.Tensor, flags: torch.Tensor):
        """An oc_nav_likelihood call bound once (see rollout_launcher)."""
        self._check(state, self.layout.state_bytes)
        self._check(taken, self.A * self.pitch)
        if alloc is not None:
            self._check(alloc, self.pitch)
        self._check(out, 8 * self.pitch, (torch.float64,))
        self._check(flags, self.pitch)
        args = (self._h, _ptr(state), _ptr(taken), _ptr(alloc), capi.subtask_array(subtasks), len(subtasks),
                self_agent, beta, none_action_prob, _ptr(out), _ptr(flags), self.B, self._stream())
        return _bound(self.lib.oc_nav_likelihood, args)

    def nav_policy(self, state: torch.Tensor, subtasks, actions: torch.Tensor, beta: float = 1.3,
                   none_action_prob: float = 0.5, mode: int = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE,
                   alloc: Optional[torch.Tensor] = None, step: int = 0, seed: int = 0, env_offset: int = 0,
                   probs: Optional[torch.Tensor] = None, num_cand: int = 25, flags: Optional[torch.Tensor] = None):
        """Subtask-following actions (oc_nav_policy): for every row the Boltzmann distribution
        p(a) ~ exp(-beta Q(s, a)) of its allocation's subtask agents over get_actions(s), and one
        action from it (mode: capi.OC_POLICY_SAMPLE or OC_POLICY_GREEDY, | OC_POLICY_COUNT_TABLE or
        OC_POLICY_COUNT_STATE) written into the subtask agents' bytes of `actions` (u8 [A][pitch];
        every other byte stays).  `probs` (f64 [num_cand][pitch], num_cand 5 or 25) receives the
        distribution when given.  The draw depends on (seed, step, env_offset + env) only.  Returns
        the flags u8 [pitch] (capi.POL_*)."""
        flags = torch.empty(self.pitch, dtype=torch.uint8, device=self.device) if flags is None else flags
        self.nav_policy_launcher(state, subtasks, actions, beta, none_action_prob, mode, alloc, step, seed, env_offset,
                                 probs, num_cand, flags)()
        return flags

    def nav_policy_launcher(self, state: torch.Tensor, subtasks, actions: torch.Tensor, beta: float,
                            none_action_prob: float, mode: int, alloc: Optional[torch.Tensor], step: int, seed: int,
                            env_offset: int, probs: Optional[torch.Tensor], num_cand: int, flags: torch.Tensor):
        """An oc_nav_policy call bound once (see rollout_launcher)."""
        self._check(state, self.layout.state_bytes)
        self._check(actions, self.A * self.pitch)
        if alloc is not None:
            self._check(alloc, self.pitch)
        if probs is not None:
            self._check(probs, 8 * int(num_cand) * self.pitch, (torch.float64,))
        self._check(flags, self.pitch)
        args = (self._h, _ptr(state), _ptr(alloc), capi.subtask_array(subtasks), len(subtasks), float(beta),
                float(none_action_prob), int(mode), int(env_offset), int(step), int(seed) & ((1 << 64) - 1),
                _ptr(actions), _ptr(probs), int(num_cand), _ptr(flags), self.B, self._stream())
        return _bound(self.lib.oc_nav_policy, args)

    def new_task_state(self, S: int, M: int) -> torch.Tensor:
        """u8 [M, capi.task_planes(S), pitch] task state of M scripted agents over S subtasks
        (oc_task_select), zeroed; the first call on it passes capi.OC_TASK_INIT."""
        return torch.zeros((M, capi.task_planes(S), self.pitch), dtype=torch.uint8, device=self.device)

    def task_select(self, state: torch.Tensor, subtasks, agents, tstate: torch.Tensor,
                    prev: Optional[torch.Tensor] = None, flags: int = capi.OC_TASK_COMMIT | capi.OC_TASK_DISTINCT,
                    bound: Optional[torch.Tensor] = None, info: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-env subtask choice of the scripted agents `agents` (oc_task_select): the reference
        agent's refresh_subtasks over `tstate` (new_task_state; updated in place) and the doable
        incomplete subtask with the smallest lower bound, per agent in the given order.  `subtasks`
        are oc_subtask rows (capi.progress_subtasks; kind, start and goal masks are read).  The cur
        plane tstate[m, capi.event_planes(S)] is nav_policy's `alloc` for agent m's table
        capi.policy_subtasks(subtasks + [None], enc, [agent]).  With `prev` (the state before the
        step that made `state`) the envs that step auto-reset start over; capi.OC_TASK_INIT in
        `flags` starts every env over.  `bound` (f32 [M, pitch]) receives the chosen bounds when
        given.  Returns info u8 [M, pitch] (capi.TASKF_*)."""
        if info is None:
            info = torch.empty((len(agents), self.pitch), dtype=torch.uint8, device=self.device)
        self.task_select_launcher(state, subtasks, agents, tstate, prev, flags, bound, info)()
        return info

    def task_select_launcher(self, state: torch.Tensor, subtasks, agents, tstate: torch.Tensor,
                             prev: Optional[torch.Tensor], flags: int, bound: Optional[torch.Tensor],
                             info: Optional[torch.Tensor]):
        """An oc_task_select call bound once (see rollout_launcher)."""
        S, M = len(subtasks), len(agents)
        self._check(state, self.layout.state_bytes)
        if prev is not None:
            self._check(prev, self.layout.state_bytes)
        self._check(tstate, M * capi.task_planes(S) * self.pitch)
        if bound is not None:
            self._check(bound, 4 * M * self.pitch, (torch.float32,))
        if info is not None:
            self._check(info, M * self.pitch)
        ags = (ctypes.c_uint8 * M)(*[int(a) for a in agents])
        args = (self._h, _ptr(state), _ptr(prev), capi.subtask_array(subtasks), S, ags, M, int(flags), _ptr(tstate),
                _ptr(bound), _ptr(info), self.B, self._stream())
        return _bound(self.lib.oc_task_select, args)

    def new_team_state(self, S: int) -> torch.Tensor:
        """u8 [capi.team_planes(S), pitch] team state of one pair of scripted agents over S subtasks
        (oc_team_select), zeroed; the first call on it passes capi.OC_TEAM_INIT."""
        return torch.zeros((capi.team_planes(S), self.pitch), dtype=torch.uint8, device=self.device)

    def team_select(self, state: torch.Tensor, subtasks, pair, tstate: torch.Tensor,
                    prev: Optional[torch.Tensor] = None, flags: int = capi.OC_TEAM_COMMIT,
                    bound: Optional[torch.Tensor] = None, info: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-env joint or split subtask choice of the scripted pair `pair` = (a0, a1), a0 < a1
        (oc_team_select): the reference agent's refresh_subtasks over `tstate` (new_team_state;
        updated in place), then the heaviest allocation under the spatial prior, the sum of
        1 / lower bound over its members: both agents on one subtask, or each on its own.  With EP =
        capi.event_planes(S) the planes tstate[EP], tstate[EP + 1] and tstate[EP + 2] are
        nav_policy's `alloc` for a0's one-agent table (subtasks + [None]), a1's, and the two-agent
        table; an env outside a table holds capi.OC_TEAM_OUT there and that launch skips it
        (capi.POL_BADALLOC).  `prev`, capi.OC_TEAM_INIT and `bound` (f32 [2, pitch]) as task_select.
        Returns info u8 [pitch] (capi.TEAMF_*)."""
        if info is None:
            info = torch.empty(self.pitch, dtype=torch.uint8, device=self.device)
        self.team_select_launcher(state, subtasks, pair, tstate, prev, flags, bound, info)()
        return info

    def team_select_launcher(self, state: torch.Tensor, subtasks, pair, tstate: torch.Tensor,
                             prev: Optional[torch.Tensor], flags: int, bound: Optional[torch.Tensor],
                             info: Optional[torch.Tensor]):
        """An oc_team_select call bound once (see rollout_launcher)."""
        S = len(subtasks)
        if len(pair) != 2:
            raise ValueError("team_select: a pair of agents, got %r" % (tuple(pair),))
        self._check(state, self.layout.state_bytes)
        if prev is not None:
            self._check(prev, self.layout.state_bytes)
        self._check(tstate, capi.team_planes(S) * self.pitch)
        if bound is not None:
            self._check(bound, 4 * 2 * self.pitch, (torch.float32,))
        if info is not None:
            self._check(info, self.pitch)
        ags = (ctypes.c_uint8 * 2)(*[int(a) for a in pair])
        args = (self._h, _ptr(state), _ptr(prev), capi.subtask_array(subtasks), S, ags, int(flags), _ptr(tstate),
                _ptr(bound), _ptr(info), self.B, self._stream())
        return _bound(self.lib.oc_team_select, args)

    def new_belief_state(self, S: int, M: int):
        """Buffers of oc_belief_update for M watched agents over S subtasks, zeroed: (belief f64
        [M, S + 1, pitch], bstate u8 [M, 2 * capi.belief_planes(S), pitch], map u8 [M, pitch], info
        u8 [M, pitch]).  The first call on them passes capi.OC_BELIEF_INIT."""
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)  # noqa: E731
        return (z((M, S + 1, self.pitch), torch.float64), z((M, 2 * capi.belief_planes(S), self.pitch), torch.uint8),
                z((M, self.pitch), torch.uint8), z((M, self.pitch), torch.uint8))

    def belief_update(self, prev: Optional[torch.Tensor], taken: Optional[torch.Tensor], subtasks, agents,
                      belief: torch.Tensor, bstate: torch.Tensor, events: Optional[torch.Tensor] = None,
                      beta: float = 1.3, none_action_prob: float = 0.5, flags: int = 0,
                      map: Optional[torch.Tensor] = None, info: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The posterior over each watched agent's subtask (oc_belief_update), updated in place over
        one step: `prev` the states the step left, `taken` its executed actions (step's exec_out),
        `events` oc_progress's events of that step (or None: no prior reset).  Hypothesis i < S is
        "the agent alone follows subtasks[i]", hypothesis S is None; `belief`, `bstate`, `map` come
        from new_belief_state.  capi.OC_BELIEF_INIT in `flags` starts every env over (prev, taken
        and events may then be None); the envs whose `prev` flags carry DONE start over by
        themselves.  Not idempotent: every call multiplies the step's likelihoods in.  Returns
        info u8 [M, pitch] (capi.BELF_*)."""
        if info is None:
            info = torch.empty((len(agents), self.pitch), dtype=torch.uint8, device=self.device)
        self.belief_update_launcher(prev, taken, subtasks, agents, belief, bstate, events, beta, none_action_prob,
                                    flags, map, info)()
        return info

    def belief_update_launcher(self, prev: Optional[torch.Tensor], taken: Optional[torch.Tensor], subtasks, agents,
                               belief: torch.Tensor, bstate: torch.Tensor, events: Optional[torch.Tensor], beta: float,
                               none_action_prob: float, flags: int, map: Optional[torch.Tensor],
                               info: Optional[torch.Tensor]):
        """An oc_belief_update call bound once (see rollout_launcher)."""
        S, M = len(subtasks), len(agents)
        if prev is not None:
            self._check(prev, self.layout.state_bytes)
        if taken is not None:
            self._check(taken, self.A * self.pitch)
        if events is not None:
            self._check(events, capi.event_planes(S) * self.pitch)
        self._check(belief, 8 * M * (S + 1) * self.pitch, (torch.float64,))
        self._check(bstate, M * 2 * capi.belief_planes(S) * self.pitch)
        for t in (map, info):
            if t is not None:
                self._check(t, M * self.pitch)
        ags = (ctypes.c_uint8 * M)(*[int(a) for a in agents])
        args = (self._h, _ptr(prev), _ptr(taken), _ptr(events), capi.subtask_array(subtasks), S, ags, M, float(beta),
                float(none_action_prob), int(flags), _ptr(belief), _ptr(bstate), _ptr(map), _ptr(info), self.B,
                self._stream())
        return _bound(self.lib.oc_belief_update, args)

    def new_team_belief_state(self, S: int, lik: bool = True):
        """Buffers of oc_team_belief_update for one pair over S subtasks, zeroed: (belief f64
        [(S + 1)^2, pitch], tbstate u8 [capi.team_belief_planes(S), pitch], lik f64 [3 S + 2, pitch]
        (None with lik=False: the call takes NULL there), map u8 [3, pitch], info u8 [pitch]).  The
        first call on them passes capi.OC_TBELIEF_INIT.  The belief matrix costs (S + 1)^2 * 8 bytes
        per env (839 MB at S = 9 and 2^20 envs)."""
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)  # noqa: E731
        return (z(((S + 1) * (S + 1), self.pitch), torch.float64),
                z((capi.team_belief_planes(S), self.pitch), torch.uint8),
                z((capi.team_lik_planes(S), self.pitch), torch.float64) if lik else None,
                z((3, self.pitch), torch.uint8), z((self.pitch,), torch.uint8))

    def team_belief_update(self, prev: Optional[torch.Tensor], taken: Optional[torch.Tensor], subtasks, pair,
                           self_agent: int, belief: torch.Tensor, tbstate: torch.Tensor,
                           events: Optional[torch.Tensor] = None, beta: float = 1.3, none_action_prob: float = 0.5,
                           flags: int = 0, lik: Optional[torch.Tensor] = None, map: Optional[torch.Tensor] = None,
                           info: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The posterior over the allocation of `pair` = (a0, a1), a0 < a1, as the delegator
        `self_agent` (one of the pair) infers it (oc_team_belief_update), updated in place over one
        step: `prev`, `taken`, `events` as belief_update.  With N = S + 1, plane i * N + j of `belief`
        is the split "a0 on i, a1 on j" (index S = None) for i != j and the joint "both on i" for
        i == j < S.  `map` u8 [3, pitch] gets the most likely allocation as team_select's (cur0, cur1,
        curJ): nav_policy's `alloc` planes.  `lik` f64 [3 S + 2, pitch] gets the step's likelihoods.
        capi.OC_TBELIEF_INIT in `flags` starts every env over; the envs whose `prev` flags carry DONE
        start over by themselves.  Not idempotent.  Returns info u8 [pitch] (capi.TBELF_*)."""
        if info is None:
            info = torch.empty(self.pitch, dtype=torch.uint8, device=self.device)
        self.team_belief_update_launcher(prev, taken, subtasks, pair, self_agent, belief, tbstate, events, beta,
                                         none_action_prob, flags, lik, map, info)()
        return info

    def team_belief_update_launcher(self, prev: Optional[torch.Tensor], taken: Optional[torch.Tensor], subtasks, pair,
                                    self_agent: int, belief: torch.Tensor, tbstate: torch.Tensor,
                                    events: Optional[torch.Tensor], beta: float, none_action_prob: float, flags: int,
                                    lik: Optional[torch.Tensor], map: Optional[torch.Tensor],
                                    info: Optional[torch.Tensor]):
        """An oc_team_belief_update call bound once (see rollout_launcher)."""
        S = len(subtasks)
        if len(pair) != 2:
            raise ValueError("team_belief_update: a pair of agents, got %r" % (tuple(pair),))
        if prev is not None:
            self._check(prev, self.layout.state_bytes)
        if taken is not None:
            self._check(taken, self.A * self.pitch)
        if events is not None:
            self._check(events, capi.event_planes(S) * self.pitch)
        self._check(belief, 8 * (S + 1) * (S + 1) * self.pitch, (torch.float64,))
        self._check(tbstate, capi.team_belief_planes(S) * self.pitch)
        if lik is not None:
            self._check(lik, 8 * capi.team_lik_planes(S) * self.pitch, (torch.float64,))
        if map is not None:
            self._check(map, 3 * self.pitch)
        if info is not None:
            self._check(info, self.pitch)
        ags = (ctypes.c_uint8 * 2)(*[int(a) for a in pair])
        args = (self._h, _ptr(prev), _ptr(taken), _ptr(events), capi.subtask_array(subtasks), S, ags, int(self_agent),
                float(beta), float(none_action_prob), int(flags), _ptr(belief), _ptr(tbstate), _ptr(lik), _ptr(map),
                _ptr(info), self.B, self._stream())
        return _bound(self.lib.oc_team_belief_update, args)

    def subtask_bounds(self, state: torch.Tensor, subtasks, lower_bound: Optional[torch.Tensor] = None,
                       doable: Optional[torch.Tensor] = None):
        """Full-state subtask bounds (oc_subtask_bounds): for every env and configuration,
        get_lower_bound_for_subtask_given_objs and subtask_alloc_is_doable; returns
        (lower bound f32 [S][pitch], doable u8 [S][pitch])."""
        S = len(subtasks)
        if lower_bound is None:
            lower_bound = torch.empty((S, self.pitch), dtype=torch.float32, device=self.device)
        if doable is None:
            doable = torch.empty((S, self.pitch), dtype=torch.uint8, device=self.device)
        self.subtask_bounds_launcher(state, subtasks, lower_bound, doable)()
        return lower_bound, doable

    def subtask_bounds_launcher(self, state: torch.Tensor, subtasks, lower_bound: torch.Tensor,
                                doable: torch.Tensor):
        """An oc_subtask_bounds call bound once (see rollout_launcher)."""
        S = len(subtasks)
        self._check(state, self.layout.state_bytes)
        self._check(lower_bound, 4 * S * self.pitch, (torch.float32,))
        self._check(doable, S * self.pitch)
        args = (self._h, _ptr(state), capi.subtask_array(subtasks), S, _ptr(lower_bound), _ptr(doable), self.B,
                self._stream())
        return _bound(self.lib.oc_subtask_bounds, args)

    def observe(self, state: torch.Tensor, obs: Optional[torch.Tensor] = None,
                action_mask: Optional[torch.Tensor] = None, view_agent: int = -1):
        """Grid observation and legal-move masks of every env (oc_observe): `obs` [B, C, H, W]
        (C = 10 + A: Counter, Cutboard, Delivery, Fresh/Chopped Tomato, Lettuce, Onion, Plate, the
        agents; u8 or float16, taken from the tensor) and `action_mask` u8 [A * pitch] (bit k:
        World.NAV_ACTIONS[k] is in get_single_actions, navigation_planner/utils.py:55-90; bit 4
        always).  With `view_agent` a the agent channels are rotated so that agent a is channel
        10.  Given one output only that one is computed; given neither, both are allocated (u8).
        Returns (obs, action_mask)."""
        if obs is None and action_mask is None:
            obs, action_mask = self.new_obs(), self.new_action_mask()
        self.observe_launcher(state, obs, action_mask, view_agent)()
        return obs, action_mask

    def observe_launcher(self, state: torch.Tensor, obs: Optional[torch.Tensor],
                         action_mask: Optional[torch.Tensor], view_agent: int = -1):
        """An oc_observe call bound once (see rollout_launcher)."""
        self._check(state, self.layout.state_bytes)
        dtype = capi.OC_OBS_U8
        if obs is not None:
            if obs.dtype not in _OBS_DTYPES:
                raise TypeError("observation dtype %s, expected torch.uint8 or torch.float16" % obs.dtype)
            n = self.B * capi.obs_channels(self.A) * self.level.height * self.level.width
            if obs.device != self.device or not obs.is_contiguous() or obs.numel() < n:
                raise ValueError("obs must be contiguous on %s with at least %d elements" % (self.device, n))
            dtype = _OBS_DTYPES[obs.dtype]
        if action_mask is not None:
            self._check(action_mask, self.A * self.pitch)
        args = (self._h, _ptr(state), _ptr(obs), _ptr(action_mask), dtype, int(view_agent), self.B, self._stream())
        return _bound(self.lib.oc_observe, args)

    def progress(self, state_prev: torch.Tensor, states: torch.Tensor, subtasks, weights=None, n: int = 1,
                 counts: Optional[torch.Tensor] = None, events: Optional[torch.Tensor] = None,
                 reward: Optional[torch.Tensor] = None):
        """Subtask progress (oc_progress) of n consecutive states `states` (one state, or an
        oc_step_n trajectory whose state_in is `state_prev`): per step and env the goal-object
        count of every subtask (RealAgent.def_subtask_completion's cur_obj_count), the completion
        events against the state before (is_subtask_complete; bit b of plane c is subtask 8c + b)
        and reward = the sum of `weights` (None: 1.0 each) over the set events.  `subtasks` are
        oc_subtask rows (capi.progress_subtasks makes them from recipe subtasks); only kind and
        goal_mask are read.  Given some outputs only those are computed; given none, all three
        are allocated.  Returns (counts, events, reward)."""
        if counts is None and events is None and reward is None:
            counts, events, reward = self.new_progress_buffers(len(subtasks), n)
        self.progress_launcher(state_prev, states, subtasks, weights, n, counts, events, reward)()
        return counts, events, reward

    def progress_launcher(self, state_prev: torch.Tensor, states: torch.Tensor, subtasks, weights, n: int,
                          counts: Optional[torch.Tensor], events: Optional[torch.Tensor],
                          reward: Optional[torch.Tensor]):
        """An oc_progress call bound once (see rollout_launcher)."""
        S = len(subtasks)
        self._check(state_prev, self.layout.state_bytes)
        self._check(states, n * self.layout.state_bytes)
        if counts is not None:
            self._check(counts, n * S * self.pitch)
        if events is not None:
            self._check(events, n * capi.event_planes(S) * self.pitch)
        if reward is not None:
            self._check(reward, 4 * n * self.pitch, (torch.float32,))
        args = (self._h, _ptr(state_prev), _ptr(states), int(n), capi.subtask_array(subtasks), S,
                capi.weight_array(weights, S), _ptr(counts), _ptr(events), _ptr(reward), self.B, self._stream())
        return _bound(self.lib.oc_progress, args)

    def set_likelihood_form(self, form: int) -> None:
        """oc_set_likelihood_form: capi.OC_LIK_FORM_AUTO (default) or OC_LIK_FORM_GROUPED (the
        grouped likelihood kernel on any level; the same outputs, for its parity test)."""
        capi.check(self.lib.oc_set_likelihood_form(self._h, int(form)))

    def last_error(self) -> str:
        """oc_get_last_error: the message of the last failed call on this handle."""
        buf = ctypes.create_string_buffer(512)
        self.lib.oc_get_last_error(self._h, buf, len(buf))
        return buf.value.decode()

    def reachability(self):
        """The level's static reachability graph (oc_reachability16): (node_of u16 [W*H*5] with
        0xFFFF = not a node, dist u16 [n][n] with 0xFFFF = no path; any level, a maze's BFS
        distances of 255 and more included)."""
        import ctypes
        n = ctypes.c_int32()
        capi.check(self.lib.oc_reachability16(self._h, ctypes.byref(n), None, 0, None, 0))
        cells = self.level.width * self.level.height
        node_of = np.zeros(cells * 5, np.uint16)
        dist = np.zeros((n.value, n.value), np.uint16)
        capi.check(self.lib.oc_reachability16(self._h, ctypes.byref(n), node_of.ctypes.data, node_of.size,
                                              dist.ctypes.data, dist.size))
        return node_of, dist

    def gen_actions(self, actions: torch.Tensor, step: int, seed: int = 0, env_offset: int = 0) -> torch.Tensor:
        self._check(actions, self.A * self.pitch)
        capi.check(self.lib.oc_gen_actions(self._h, _ptr(actions), self.B, env_offset, step, seed, self._stream()))
        return actions

    def checksum(self, state: torch.Tensor) -> torch.Tensor:
        """[1] int64 device checksum of envs [0, B) (include/oc_engine.h oc_state_checksum)."""
        self._check(state, self.layout.state_bytes)
        out = torch.empty(1, dtype=torch.int64, device=self.device)
        capi.check(self.lib.oc_state_checksum(self._h, _ptr(state), self.B, _ptr(out), self._stream()))
        return out

    def reduce_stats(self, stats: torch.Tensor) -> torch.Tensor:
        """[OC_NSTATS] uint64 device totals of a partial-stats buffer."""
        out = torch.empty(capi.OC_NSTATS, dtype=torch.int64, device=self.device)  # u64 sums < 2^63
        capi.check(self.lib.oc_stats_reduce(self._h, _ptr(stats), self.B, _ptr(out), self._stream()))
        return out

    def _check(self, t: torch.Tensor, nbytes: int, dtypes=(torch.uint8,)) -> None:
        """Device, contiguity, size, alignment and element type of a buffer handed to the
        C-ABI (the kernels read raw bytes: an int64 action tensor would pass a size check
        and be read as 8 bytes per code)."""
        if t.dtype not in dtypes:
            raise TypeError("buffer dtype %s, expected %s" % (t.dtype, " or ".join(str(d) for d in dtypes)))
        if t.device != self.device or not t.is_contiguous():
            raise ValueError("buffer must be contiguous on %s" % self.device)
        if t.numel() * t.element_size() < nbytes:
            raise ValueError("buffer too small: %d < %d bytes" % (t.numel() * t.element_size(), nbytes))
        if t.data_ptr() % 16:
            raise ValueError("buffer must be 16-byte aligned")


class CpuStepper(_StartCells):
    """oc_cpu_step: the engine's step on the host, for a caller without a GPU (numpy buffers in
    the oc_step layout).  The same SWAR step as the kernels (its host pass); the GPU path never
    calls it.  `step` mirrors OvercookedBatch.step (overcooked_environment.py:255-306)."""

    def __init__(self, level, num_agents: int, B: int, max_T: int = 100, nthreads: int = 0):
        if isinstance(level, str):
            level = _levels.load_level(level)
        self.level, self.A, self.B, self.max_T, self.nthreads = level, num_agents, int(B), max_T, nthreads
        self.lib = capi.load_library()
        self._desc = capi.level_desc(level, num_agents)
        h = ctypes.c_void_p()
        # a host-only handle: oc_create makes no HIP call (no device query, no device tables)
        capi.check(self.lib.oc_create(ctypes.byref(self._desc), num_agents, max_T, capi.OC_DEVICE_HOST,
                                      ctypes.byref(h)))
        self._h = h
        lay = capi.OcLayout()
        capi.check(self.lib.oc_get_layout(self._h, self.B, ctypes.byref(lay)))
        self.layout, self.K, self.pitch = lay, lay.num_items, lay.pitch

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and getattr(self, "lib", None) is not None:
            self.lib.oc_destroy(h)
            self._h = None

    def new_state(self) -> np.ndarray:
        """The level template in every env (reset(), overcooked_environment.py:201-250), built
        on the host from the level description."""
        A, K, P, L = self.A, self.K, self.pitch, self.layout
        s = np.zeros((L.num_planes, P), np.uint8)
        lv = self.level
        for a in range(A):
            s[a], s[A + a], s[2 * A + a] = lv.spawns[a][0], lv.spawns[a][1], 0xFF
        dead = 0xFFFF if L.cell_bytes == 2 else 0xFF
        for j in range(K):
            c, m = (lv.items[j] if j < len(lv.items) else (dead, 0))
            s[L.plane_item_loc + j], s[L.plane_item_mask + j] = c & 0xFF, m
            if L.cell_bytes == 2:
                s[L.plane_item_loc_hi + j] = c >> 8
        return s.reshape(-1)

    def step(self, state_in: np.ndarray, state_out: np.ndarray, actions: np.ndarray,
             exec_out: Optional[np.ndarray] = None, coll: Optional[np.ndarray] = None,
             totals: Optional[np.ndarray] = None) -> np.ndarray:
        for a, n in ((state_in, self.layout.state_bytes), (state_out, self.layout.state_bytes),
                     (actions, self.A * self.pitch), (exec_out, self.A * self.pitch), (coll, self.pitch)):
            if a is not None and (a.dtype != np.uint8 or not a.flags.c_contiguous or a.nbytes < n):
                raise ValueError("host buffers: contiguous uint8 of at least %d bytes" % n)
        if totals is not None and (totals.dtype not in (np.uint64, np.int64) or totals.size < capi.OC_NSTATS):
            raise ValueError("totals: %d uint64" % capi.OC_NSTATS)
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        capi.check(self.lib.oc_cpu_step(self._h, p(state_in), p(state_out), p(actions), p(exec_out), p(coll),
                                        p(totals), self.B, self.nthreads))
        return state_out

    def reset_random(self, state: np.ndarray, prev: Optional[np.ndarray] = None, seed: int = 0, round: int = 0,
                     what: int = 3, env_offset: int = 0) -> np.ndarray:
        """oc_cpu_reset_random: randomised starts in the host states; mirrors
        OvercookedBatch.reset_random (with `prev`, only its DONE envs are rewritten).  Only columns
        below B are written."""
        for a in (state, prev):
            if a is not None and (a.dtype != np.uint8 or not a.flags.c_contiguous or a.nbytes < self.layout.state_bytes):
                raise ValueError("host buffers: contiguous uint8 of at least %d bytes" % self.layout.state_bytes)
        mask = (1 << 64) - 1
        capi.check(self.lib.oc_cpu_reset_random(self._h, state.ctypes.data, None if prev is None else prev.ctypes.data,
                                                self.B, int(env_offset), int(seed) & mask, int(round) & mask,
                                                int(what), self.nthreads))
        return state

    def observe(self, state: np.ndarray, dtype=np.uint8, view_agent: int = -1, want_mask: bool = True):
        """oc_cpu_observe: the grid observation [B, C, H, W] (np.uint8 or np.float16) and, with
        `want_mask`, the legal-move masks u8 [A, pitch] (columns past B zero) of the host states;
        mirrors OvercookedBatch.observe.  Returns (obs, action_mask or None)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.uint8), np.dtype(np.float16)):
            raise TypeError("observation dtype %s, expected uint8 or float16" % dt)
        if state.dtype != np.uint8 or not state.flags.c_contiguous or state.nbytes < self.layout.state_bytes:
            raise ValueError("host buffers: contiguous uint8 of at least %d bytes" % self.layout.state_bytes)
        obs = np.empty((self.B, capi.obs_channels(self.A), self.level.height, self.level.width), dt)
        mask = np.zeros((self.A, self.pitch), np.uint8) if want_mask else None
        capi.check(self.lib.oc_cpu_observe(self._h, state.ctypes.data, obs.ctypes.data,
                                           None if mask is None else mask.ctypes.data,
                                           capi.OC_OBS_F16 if dt == np.float16 else capi.OC_OBS_U8, int(view_agent),
                                           self.B, self.nthreads))
        return obs, mask

    def nav_policy(self, state: np.ndarray, subtasks, actions: np.ndarray, beta: float = 1.3,
                   none_action_prob: float = 0.5, mode: int = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE,
                   alloc: Optional[np.ndarray] = None, step: int = 0, seed: int = 0, env_offset: int = 0,
                   probs: Optional[np.ndarray] = None, num_cand: int = 25, flags: Optional[np.ndarray] = None):
        """oc_cpu_nav_policy: subtask-following actions in the host buffers; mirrors
        OvercookedBatch.nav_policy.  Only the subtask agents' bytes of `actions` below column B,
        `probs` [num_cand, pitch] and `flags` below column B are written (buffers may end at column
        B of their last plane).  Returns the flags u8 [pitch]."""
        B = self.B
        flags = np.zeros(self.pitch, np.uint8) if flags is None else flags
        for a, n, dt in ((state, self.layout.state_bytes, np.uint8), (actions, (self.A - 1) * self.pitch + B, np.uint8),
                         (alloc, B, np.uint8), (flags, B, np.uint8),
                         (probs, 8 * ((int(num_cand) - 1) * self.pitch + B), np.float64)):
            if a is not None and (a.dtype != dt or not a.flags.c_contiguous or a.nbytes < n):
                raise ValueError("host buffers: contiguous %s of at least %d bytes" % (np.dtype(dt), n))
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        capi.check(self.lib.oc_cpu_nav_policy(self._h, p(state), p(alloc), capi.subtask_array(subtasks), len(subtasks),
                                              float(beta), float(none_action_prob), int(mode), int(env_offset),
                                              int(step), int(seed) & ((1 << 64) - 1), p(actions), p(probs),
                                              int(num_cand), p(flags), B, self.nthreads))
        return flags

    def task_select(self, state: np.ndarray, subtasks, agents, tstate: np.ndarray,
                    prev: Optional[np.ndarray] = None, flags: int = capi.OC_TASK_COMMIT | capi.OC_TASK_DISTINCT,
                    bound: Optional[np.ndarray] = None, info: Optional[np.ndarray] = None) -> np.ndarray:
        """oc_cpu_task_select: the scripted agents' subtask choice in the host buffers; mirrors
        OvercookedBatch.task_select.  `tstate` u8 [M, capi.task_planes(S), pitch] is updated in place,
        `bound` f32 [M, pitch] when given; only columns below B are written (buffers may end at
        column B of their last plane).  Returns info u8 [M, pitch]."""
        S, M, B, P = len(subtasks), len(agents), self.B, self.pitch
        info = np.zeros((M, P), np.uint8) if info is None else info
        for a, n, dt in ((state, self.layout.state_bytes, np.uint8), (prev, self.layout.state_bytes, np.uint8),
                         (tstate, (M * capi.task_planes(S) - 1) * P + B, np.uint8), (info, (M - 1) * P + B, np.uint8),
                         (bound, 4 * ((M - 1) * P + B), np.float32)):
            if a is not None and (a.dtype != dt or not a.flags.c_contiguous or a.nbytes < n):
                raise ValueError("host buffers: contiguous %s of at least %d bytes" % (np.dtype(dt), n))
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        ags = (ctypes.c_uint8 * M)(*[int(a) for a in agents])
        capi.check(self.lib.oc_cpu_task_select(self._h, p(state), p(prev), capi.subtask_array(subtasks), S, ags, M,
                                               int(flags), p(tstate), p(bound), p(info), B, self.nthreads))
        return info

    def team_select(self, state: np.ndarray, subtasks, pair, tstate: np.ndarray, prev: Optional[np.ndarray] = None,
                    flags: int = capi.OC_TEAM_COMMIT, bound: Optional[np.ndarray] = None,
                    info: Optional[np.ndarray] = None) -> np.ndarray:
        """oc_cpu_team_select: the scripted pair's joint or split subtask choice in the host buffers;
        mirrors OvercookedBatch.team_select.  `tstate` u8 [capi.team_planes(S), pitch] is updated in
        place, `bound` f32 [2, pitch] when given; only columns below B are written (buffers may end
        at column B of their last plane).  Returns info u8 [pitch]."""
        S, B, P = len(subtasks), self.B, self.pitch
        if len(pair) != 2:
            raise ValueError("team_select: a pair of agents, got %r" % (tuple(pair),))
        info = np.zeros(P, np.uint8) if info is None else info
        for a, n, dt in ((state, self.layout.state_bytes, np.uint8), (prev, self.layout.state_bytes, np.uint8),
                         (tstate, (capi.team_planes(S) - 1) * P + B, np.uint8), (info, B, np.uint8),
                         (bound, 4 * (P + B), np.float32)):
            if a is not None and (a.dtype != dt or not a.flags.c_contiguous or a.nbytes < n):
                raise ValueError("host buffers: contiguous %s of at least %d bytes" % (np.dtype(dt), n))
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        ags = (ctypes.c_uint8 * 2)(*[int(a) for a in pair])
        capi.check(self.lib.oc_cpu_team_select(self._h, p(state), p(prev), capi.subtask_array(subtasks), S, ags,
                                               int(flags), p(tstate), p(bound), p(info), B, self.nthreads))
        return info

    def new_belief_state(self, S: int, M: int):
        """Host buffers of oc_cpu_belief_update, zeroed; mirrors OvercookedBatch.new_belief_state."""
        P = self.pitch
        return (np.zeros((M, S + 1, P), np.float64), np.zeros((M, 2 * capi.belief_planes(S), P), np.uint8),
                np.zeros((M, P), np.uint8), np.zeros((M, P), np.uint8))

    def belief_update(self, prev: Optional[np.ndarray], taken: Optional[np.ndarray], subtasks, agents,
                      belief: np.ndarray, bstate: np.ndarray, events: Optional[np.ndarray] = None, beta: float = 1.3,
                      none_action_prob: float = 0.5, flags: int = 0, map: Optional[np.ndarray] = None,
                      info: Optional[np.ndarray] = None) -> np.ndarray:
        """oc_cpu_belief_update: the posterior over each watched agent's subtask in the host buffers;
        mirrors OvercookedBatch.belief_update.  `belief` f64 [M, S + 1, pitch] and `bstate` u8
        [M, 2 * capi.belief_planes(S), pitch] are updated in place; only columns below B are written
        (buffers may end at column B of their last plane).  Returns info u8 [M, pitch]."""
        S, M, B, P = len(subtasks), len(agents), self.B, self.pitch
        info = np.zeros((M, P), np.uint8) if info is None else info
        for a, n, dt in ((prev, self.layout.state_bytes, np.uint8), (taken, (self.A - 1) * P + B, np.uint8),
                         (events, (capi.event_planes(S) - 1) * P + B, np.uint8),
                         (belief, 8 * ((M * (S + 1) - 1) * P + B), np.float64),
                         (bstate, (M * 2 * capi.belief_planes(S) - 1) * P + B, np.uint8),
                         (map, (M - 1) * P + B, np.uint8), (info, (M - 1) * P + B, np.uint8)):
            if a is not None and (a.dtype != dt or not a.flags.c_contiguous or a.nbytes < n):
                raise ValueError("host buffers: contiguous %s of at least %d bytes" % (np.dtype(dt), n))
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        ags = (ctypes.c_uint8 * M)(*[int(a) for a in agents])
        capi.check(self.lib.oc_cpu_belief_update(self._h, p(prev), p(taken), p(events), capi.subtask_array(subtasks), S,
                                                 ags, M, float(beta), float(none_action_prob), int(flags), p(belief),
                                                 p(bstate), p(map), p(info), B, self.nthreads))
        return info

    def new_team_belief_state(self, S: int):
        """Host buffers of oc_cpu_team_belief_update, zeroed; mirrors OvercookedBatch.new_team_belief_state."""
        P = self.pitch
        return (np.zeros(((S + 1) * (S + 1), P), np.float64), np.zeros((capi.team_belief_planes(S), P), np.uint8),
                np.zeros((capi.team_lik_planes(S), P), np.float64), np.zeros((3, P), np.uint8), np.zeros(P, np.uint8))

    def team_belief_update(self, prev: Optional[np.ndarray], taken: Optional[np.ndarray], subtasks, pair,
                           self_agent: int, belief: np.ndarray, tbstate: np.ndarray,
                           events: Optional[np.ndarray] = None, beta: float = 1.3, none_action_prob: float = 0.5,
                           flags: int = 0, lik: Optional[np.ndarray] = None, map: Optional[np.ndarray] = None,
                           info: Optional[np.ndarray] = None) -> np.ndarray:
        """oc_cpu_team_belief_update: the posterior over the pair's allocation in the host buffers;
        mirrors OvercookedBatch.team_belief_update.  `belief` f64 [(S + 1)^2, pitch] and `tbstate` u8
        [capi.team_belief_planes(S), pitch] are updated in place; only columns below B are written
        (buffers may end at column B of their last plane).  Returns info u8 [pitch]."""
        S, B, P = len(subtasks), self.B, self.pitch
        if len(pair) != 2:
            raise ValueError("team_belief_update: a pair of agents, got %r" % (tuple(pair),))
        info = np.zeros(P, np.uint8) if info is None else info
        for a, n, dt in ((prev, self.layout.state_bytes, np.uint8), (taken, (self.A - 1) * P + B, np.uint8),
                         (events, (capi.event_planes(S) - 1) * P + B, np.uint8),
                         (belief, 8 * (((S + 1) * (S + 1) - 1) * P + B), np.float64),
                         (tbstate, (capi.team_belief_planes(S) - 1) * P + B, np.uint8),
                         (lik, 8 * ((capi.team_lik_planes(S) - 1) * P + B), np.float64),
                         (map, 2 * P + B, np.uint8), (info, B, np.uint8)):
            if a is not None and (a.dtype != dt or not a.flags.c_contiguous or a.nbytes < n):
                raise ValueError("host buffers: contiguous %s of at least %d bytes" % (np.dtype(dt), n))
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        ags = (ctypes.c_uint8 * 2)(*[int(a) for a in pair])
        capi.check(self.lib.oc_cpu_team_belief_update(self._h, p(prev), p(taken), p(events),
                                                      capi.subtask_array(subtasks), S, ags, int(self_agent), float(beta),
                                                      float(none_action_prob), int(flags), p(belief), p(tbstate),
                                                      p(lik), p(map), p(info), B, self.nthreads))
        return info

    def progress(self, state_prev: np.ndarray, states: np.ndarray, subtasks, weights=None, n: int = 1,
                 want=("counts", "events", "reward")):
        """oc_cpu_progress: (counts u8 [n, S, pitch], events u8 [n, planes, pitch], reward f32
        [n, pitch]) of n consecutive host states against the state before; mirrors
        OvercookedBatch.progress.  Outputs not named in `want` are None; columns past B stay zero."""
        S, P = len(subtasks), self.pitch
        for a, k in ((state_prev, 1), (states, n)):
            if a.dtype != np.uint8 or not a.flags.c_contiguous or a.nbytes < k * self.layout.state_bytes:
                raise ValueError("host buffers: contiguous uint8 of at least %d bytes" % (k * self.layout.state_bytes))
        counts = np.zeros((n, S, P), np.uint8) if "counts" in want else None
        events = np.zeros((n, capi.event_planes(S), P), np.uint8) if "events" in want else None
        reward = np.zeros((n, P), np.float32) if "reward" in want else None
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        capi.check(self.lib.oc_cpu_progress(self._h, state_prev.ctypes.data, states.ctypes.data, int(n),
                                            capi.subtask_array(subtasks), S, capi.weight_array(weights, S),
                                            p(counts), p(events), p(reward), self.B, self.nthreads))
        return counts, events, reward
