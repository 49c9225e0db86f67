"""gym surface of the engine: the reference ``OvercookedEnvironment`` class, drop-in, and a
batched vector env.

``OvercookedEnvironment`` mirrors gym_cooking/envs/overcooked_environment.py (class :37):
the same constructor argument (``arglist`` with ``level``, ``num_agents``,
``max_num_timesteps``, ``seed``, ``model1..4``), ``reset() -> env copy`` (:201-250),
``step(action_dict) -> (obs_env, reward, done, info)`` (:255-306), ``done()`` (:316-363),
``reward()`` (:365-376), ``close()`` (:252), ``get_repr()`` (:50-62), ``is_collision``
(:671-722), and the attributes callers read (``t``, ``sim_agents``, ``world``, ``obs_tm1``,
``agent_actions``, ``collisions``, ``termination_info``, ``successful``, ``filename``).
One env is one batch row of the HIP engine (B = 1); every transition runs on the GPU
through liboc_engine.so, and the host keeps a 17-byte-per-agent-count state copy from
which the object views below are built.

Differences from the reference, by design:
  * stepping after ``done`` continues the episode like the reference (the engine's
    next-step auto-reset is disabled for this single env by clearing DONE on upload);
  * a step that the reference would crash in (two co-located agents both holding,
    ``copy.copy`` at :289 -> world.py:417) raises :class:`CopyCrash`, an ``AttributeError``
    as the reference's is, here after updating the state, as the reference raises after
    ``execute_navigation``;
  * ``world.get_repr()`` keeps an empty group for every object name that existed earlier in
    the episode, as the reference's ``World.objects`` dict does (``remove`` pops from a
    group but never drops it, world.py:304-316, 323-337).  The 17-byte state does not hold
    that history, so the single env tracks the names it has seen since ``reset``; a
    merge's new name always shows in the post-step state (the merged item is held), so
    the set is exact.  ``OvercookedVecEnv`` has no per-env object views.
  * ``info["image_obs"]`` / ``game.get_image_obs()`` come from the oc_render kernel
    (gym_cooking_amd/render.py) when ``with_image_obs`` or ``record`` is set; otherwise
    ``image_obs`` is None (the reference has no ``game`` then and raises in ``step``, :291).
  * ``all_subtasks`` comes from gym_cooking_amd.recipes (the reference's STRIPS
    decomposition; of two Merge orders with the same transition the reference keeps a
    hash-seed-dependent one, this keeps the one it keeps under PYTHONHASHSEED=0).

``OvercookedVecEnv`` is the batched surface (B envs on one GPU, torch tensors in and out).
"""
from __future__ import annotations

import copy as _copy
import functools
import types
from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi
from . import levels as _levels
from . import recipes as _recipes

CollisionRepr = namedtuple("CollisionRepr", "time agent_names agent_locations")   # overcooked_environment.py:34
ObjectRepr = namedtuple("ObjectRepr", "name location is_held")                    # utils/core.py:128
AgentRepr = namedtuple("AgentRepr", "name location holding")                      # utils/agent.py:22
GridSquareRepr = namedtuple("GridSquareRepr", "name location holding")            # utils/core.py:16

FLAG_DONE, FLAG_SUCCESS, FLAG_ERR = 0x01, 0x02, 0x04  # include/oc_engine.h flags plane


class CopyCrash(AttributeError):
    """The reference's crash when ``copy.copy`` meets two co-located agents that both hold an
    item: ``World.get_object_at`` returns None and ``None.name`` raises AttributeError
    (overcooked_environment.py:289 -> :108-113 -> world.py:417).  Callers written against the
    reference catch AttributeError; this is one."""
COLORS = ["blue", "magenta", "yellow", "green"]  # utils/agent.py:25
NAV_ACTIONS = [(0, 1), (0, -1), (-1, 0), (1, 0)]  # utils/world.py:16
_TILE_NAMES = {_levels.TILE_FLOOR: "Floor", _levels.TILE_COUNTER: "Counter",
               _levels.TILE_CUTBOARD: "Cutboard", _levels.TILE_DELIVERY: "Delivery"}


@functools.lru_cache(maxsize=1024)
def _item_names(mask: int, enc: int = _levels.ENC_PRESENCE):
    """(contents, name, full_name) of an item mask in encoding `enc`, as Object.update_names
    builds them: contents sorted by base name (core.py:161-171)."""
    parts = _levels.mask_contents(mask, enc)
    return [p[0] for p in parts], "-".join(p[0] for p in parts), "-".join(p[1] for p in parts)


def item_name(mask: int, enc: int = _levels.ENC_PRESENCE) -> str:
    """The object-group name of an item mask (ItemView.name)."""
    return _item_names(mask, enc)[1]


def action_code(action) -> int:
    """(dx, dy) -> engine action code (World.NAV_ACTIONS order, (0, 0) = no-op)."""
    a = tuple(int(v) for v in action)
    if a not in _levels.ACTION_CODE:
        raise ValueError("not a navigation action: %r" % (action,))
    return _levels.ACTION_CODE[a]


# ---------------------------------------------------------------------------------------
# Host views of one env's state (read-only snapshots of the engine state bytes)
# ---------------------------------------------------------------------------------------
class ItemView:
    """An item slot as the reference ``Object`` (utils/core.py:130-241)."""

    collidable = False
    dynamic = False

    def __init__(self, slot: int, mask: int, location: Tuple[int, int], is_held: bool,
                 enc: int = _levels.ENC_PRESENCE):
        self.slot, self.mask, self.location, self.is_held, self.enc = slot, mask, location, is_held, enc
        contents, self.name, self.full_name = _item_names(mask, enc)
        self.contents = list(contents)

    def get_repr(self):
        return ObjectRepr(name=self.full_name, location=self.location, is_held=self.is_held)

    def contains(self, c_name: str) -> bool:
        return c_name in self.contents

    def needs_chopped(self) -> bool:  # core.py:176-178
        return _levels.needs_chopped(self.mask, self.enc)

    def is_deliverable(self) -> bool:  # core.py:214-219
        return _levels.is_deliverable(self.mask, self.enc)

    def __eq__(self, other):  # core.py:142-146
        return (getattr(other, "name", None) == self.name and getattr(other, "full_name", None) == self.full_name
                and len(getattr(other, "contents", ())) == len(self.contents))

    def __hash__(self):
        return hash((self.slot, self.mask, self.location))

    def __str__(self):
        return self.full_name

    __repr__ = __str__


class GridSquareView:
    """A static tile as the reference ``GridSquare`` (utils/core.py:28-120)."""

    def __init__(self, name: str, location: Tuple[int, int], holding):
        self.name, self.location, self.holding = name, location, holding
        self.collidable = name != "Floor"

    def get_repr(self):
        return GridSquareRepr(name=self.name, location=self.location, holding=self.holding)

    def __eq__(self, other):
        return isinstance(other, GridSquareView) and other.name == self.name

    def __hash__(self):
        return hash((self.name, self.location))


class SimAgentView:
    """An agent as the reference ``SimAgent`` (utils/agent.py:369-423)."""

    def __init__(self, name: str, color: str, location: Tuple[int, int], holding: Optional[ItemView], action=None):
        self.name, self.color, self.location, self.holding, self.action = name, color, location, holding, action

    def get_repr(self):  # agent.py:393-394
        return AgentRepr(name=self.name, location=self.location, holding=self.get_holding())

    def get_holding(self) -> str:  # agent.py:396-399
        return "None" if self.holding is None else self.holding.full_name


class NoPath(Exception):
    """No path between two reachability-graph nodes (networkx raises NetworkXNoPath)."""


class ReachabilityGraph:
    """``World.reachability_graph`` (utils/world.py:67-108) as oc_create builds it: nodes are
    ``(location, approach)``, approach ``(0, 0)`` for a Floor square or the NAV_ACTION from
    which a collidable square is reached; ``shortest_path_length`` reads the all-pairs BFS
    table the kernels use (oc_reachability).  ``to_networkx()`` gives the reference's
    ``nx.Graph`` when networkx is importable."""

    _APPROACH = NAV_ACTIONS + [(0, 0)]

    def __init__(self, width: int, node_of: np.ndarray, dist: np.ndarray):
        self.width = width
        self._id: Dict[tuple, int] = {}
        for key, n in enumerate(node_of.tolist()):
            if n != 0xFFFF:
                c, d = divmod(key, 5)
                self._id[((c % width, c // width), self._APPROACH[d])] = n
        self._dist = dist
        self._nopath = 0xFFFF if dist.dtype == np.uint16 else 0xFF  # oc_reachability16 / oc_reachability

    def nodes(self) -> list:
        return sorted(self._id, key=self._id.get)

    def edges(self) -> list:
        nodes = self.nodes()
        return [(u, v) for i, u in enumerate(nodes) for v in nodes[i + 1:] if self._dist[i, nodes.index(v)] == 1]

    def __contains__(self, node) -> bool:
        return self._key(node) in self._id

    def __len__(self) -> int:
        return len(self._id)

    @staticmethod
    def _key(node):
        (x, y), a = node
        return (int(x), int(y)), (int(a[0]), int(a[1]))

    def shortest_path_length(self, source, target) -> int:
        """nx.shortest_path_length(reachability_graph, source, target); raises NoPath."""
        u, v = self._id.get(self._key(source)), self._id.get(self._key(target))
        if u is None or v is None or self._dist[u, v] == self._nopath:
            raise NoPath("no path between %r and %r" % (source, target))
        return int(self._dist[u, v])

    def to_networkx(self):
        import networkx as nx
        g = nx.Graph()
        g.add_nodes_from(self.nodes())
        g.add_edges_from(self.edges())
        return g


def get_subtask_obj(subtask, enc: int = _levels.ENC_PRESENCE):
    """nav_utils.get_subtask_obj (navigation_planner/utils.py:181-246): (start, goal) objects of
    a subtask (a list of two for Merge; (None, None) for None), compared by contents like the
    reference's Objects."""
    kind, (sa, sb), goal = _recipes.subtask_masks(subtask, enc)
    if kind == 0:
        return None, None
    obj = lambda m: ItemView(-1, m, None, False, enc)  # noqa: E731
    start = [obj(sa), obj(sb)] if kind == 2 else obj(sa)
    return start, obj(goal)


def get_subtask_action_obj(subtask):
    """nav_utils.get_subtask_action_obj (navigation_planner/utils.py:154-177): the static
    square a subtask acts on (Cutboard for Chop, Delivery for Deliver, else None)."""
    if subtask is None:
        return None
    if subtask.name not in ("Chop", "Merge", "Deliver"):
        raise ValueError("Did not recognize subtask {} so could not find the appropriate subtask location"
                         .format(subtask))
    name = {"Chop": "Cutboard", "Deliver": "Delivery"}.get(subtask.name)
    return GridSquareView(name, None, None) if name else None


def _is_merge(subtask) -> bool:
    return subtask is not None and subtask.name == "Merge"


class WorldView:
    """The reference ``World`` queries (utils/world.py:285-436) over one env's state."""

    NAV_ACTIONS = NAV_ACTIONS

    def __init__(self, level: _levels.Level, items: Sequence[ItemView], group_names: Sequence[str] = (),
                 reachability_graph: Optional[ReachabilityGraph] = None):
        self.reachability_graph = reachability_graph
        self.level = level
        self.width, self.height = level.width, level.height
        self.perimeter = 2 * (self.width + self.height)  # overcooked_environment.py:198
        self.items = list(items)
        unheld = {it.location: it for it in self.items if not it.is_held}
        self.objects: Dict[str, list] = {}
        self._squares: Dict[Tuple[int, int], GridSquareView] = {}
        for c, code in enumerate(level.tiles):
            xy = level.xy(c)
            name = _TILE_NAMES[code]
            holding = None
            if name == "Delivery":
                holding = [it for it in self.items if not it.is_held and it.location == xy]
            elif name != "Floor":
                holding = unheld.get(xy)
            gs = GridSquareView(name, xy, holding)
            self._squares[xy] = gs
            self.objects.setdefault(name, []).append(gs)
        for name in group_names:  # emptied groups stay (world.py:304-316)
            self.objects.setdefault(name, [])
        for it in sorted(self.items, key=lambda i: i.slot):
            self.objects.setdefault(it.name, []).append(it)

    def get_object_list(self) -> list:
        out = []
        for v in self.objects.values():
            out += v
        return out

    def get_dynamic_objects(self):  # world.py:322-337 (non-empty groups, see module doc)
        objs = []
        for key in sorted(self.objects):
            if key in ("Counter", "Floor", "Delivery", "Cutboard") or "Supply" in key:
                continue
            objs.append(tuple(o.get_repr() for o in self.objects[key]))
        return tuple(objs)

    get_repr = get_dynamic_objects

    def is_occupied(self, location) -> bool:  # world.py:285-290
        return any(it.location == tuple(location) and not it.is_held for it in self.items)

    def is_collidable(self, location) -> bool:
        return self.get_gridsquare_at(location).collidable

    def get_collidable_object_locations(self) -> list:
        return [o.location for o in self.get_object_list() if o.collidable]

    def get_object_locs(self, obj, is_held: bool) -> list:  # world.py:339-363
        if obj.name not in self.objects:
            return []
        if isinstance(obj, ItemView):
            return [o.location for o in self.objects[obj.name] if obj == o and o.is_held == is_held]
        return [o.location for o in self.objects[obj.name] if obj == o]

    def get_all_object_locs(self, obj) -> list:  # world.py:365-376
        return list(set(self.get_object_locs(obj, True) + self.get_object_locs(obj, False)))

    def get_object_at(self, location, desired_obj, find_held_objects: bool):  # world.py:378-405
        loc = tuple(location)
        objs = [o for o in self.items if o.location == loc and o.is_held is find_held_objects
                and (desired_obj is None or o.name == desired_obj.name)]
        assert len(objs) == 1, "looking for {}, found {} at {}".format(desired_obj, len(objs), location)
        return objs[0]

    def get_gridsquare_at(self, location) -> GridSquareView:  # world.py:407-416
        gs = self._squares.get((int(location[0]), int(location[1])))
        assert gs is not None, "0 gridsquares at {}".format(location)
        return gs

    def inbounds(self, location):  # world.py:432-436
        x, y = location
        return min(max(x, 0), self.width - 1), min(max(y, 0), self.height - 1)

    def get_lower_bound_between(self, subtask, agent_locs, A_locs, B_locs):  # world.py:115-146
        lower_bound = self.perimeter + 1
        for A_loc in A_locs:
            for B_loc in B_locs:
                bound = self.get_lower_bound_between_helper(subtask, tuple(agent_locs), tuple(A_loc), tuple(B_loc))
                if bound < lower_bound:
                    lower_bound = bound
        return lower_bound

    def get_lower_bound_between_helper(self, subtask, agent_locs, A_loc, B_loc):  # world.py:148-264
        g = self.reachability_graph
        if g is None:
            raise RuntimeError("this world view has no reachability graph")
        spl = g.shortest_path_length
        lower_bound = self.perimeter + 1
        A_na = [(0, 0)] if not self.get_gridsquare_at(A_loc).collidable else NAV_ACTIONS
        B_na = [(0, 0)] if not self.get_gridsquare_at(B_loc).collidable else NAV_ACTIONS

        def dist(u, v, default):
            try:
                return spl(u, v)
            except NoPath:
                return default

        for a_na in A_na:
            for b_na in B_na:
                if len(agent_locs) == 1:
                    try:
                        b1 = spl((agent_locs[0], (0, 0)), (A_loc, a_na))
                        b2 = spl((A_loc, a_na), (B_loc, b_na))
                    except NoPath:
                        continue
                    bound = b1 + b2 - 1
                else:
                    b1A = dist((agent_locs[0], (0, 0)), (A_loc, a_na), self.perimeter)
                    b2A = dist((agent_locs[1], (0, 0)), (A_loc, a_na), self.perimeter)
                    b1B = dist((agent_locs[0], (0, 0)), (B_loc, b_na), self.perimeter)
                    b2B = dist((agent_locs[1], (0, 0)), (B_loc, b_na), self.perimeter)
                    mA, mB = min(b1A, b2A), min(b1B, b2B)
                    man = float(abs(A_loc[0] - B_loc[0]) + abs(A_loc[1] - B_loc[1]))  # manhattan_dist
                    if _is_merge(subtask):
                        if (b1A == mA and b1B == mB) or (b2A == mA and b2B == mB):  # check_bound :266-283
                            mA, mB = 2 * mA, 2 * mB
                        bound = max(mA, mB) + (man - 1) / 2
                    else:
                        bound = mA + man - 1
                if bound < lower_bound:
                    lower_bound = bound
        return max(1, lower_bound)


def is_collision(world, agent1_loc, agent2_loc, agent1_action, agent2_action):
    """OvercookedEnvironment.is_collision (overcooked_environment.py:671-722): [execute1,
    execute2] for two agents' (location, action) on `world` (anything with get_gridsquare_at)."""
    execute = [True, True]
    l1, l2, a1, a2 = tuple(agent1_loc), tuple(agent2_loc), tuple(agent1_action), tuple(agent2_action)
    n1 = (l1[0] + a1[0], l1[1] + a1[1])
    if world.get_gridsquare_at(n1).collidable:
        n1 = l1
    n2 = (l2[0] + a2[0], l2[1] + a2[1])
    if world.get_gridsquare_at(n2).collidable:
        n2 = l2
    if n1 == n2:
        if n1 == l1 and a1 != (0, 0):
            execute[1] = False
        elif n2 == l2 and a2 != (0, 0):
            execute[0] = False
        else:
            execute[0] = execute[1] = False
    elif l1 == n2 and l2 == n1:
        execute[0] = execute[1] = False
    return execute


def _decode_items(b, A: int, K: int):
    """(item cells, masks, t, flags, dead cell value) of one env's state bytes: the narrow
    layout (3A + 2K + 3 bytes, byte cells) or the wide one (3A + 3K + 3: the cells' high bytes
    after the low ones, include/oc_engine.h oc_layout)."""
    if len(b) == 3 * A + 3 * K + 3:
        loc = [b[3 * A + j] | (b[3 * A + K + j] << 8) for j in range(K)]
        m0, dead = 3 * A + 2 * K, 0xFFFF
    else:
        loc, m0, dead = b[3 * A:3 * A + K], 3 * A + K, _levels.LOC_DEAD
    return loc, b[m0:m0 + K], b[m0 + K] | (b[m0 + K + 1] << 8), b[m0 + K + 2], dead


def build_views(level: _levels.Level, A: int, K: int, env_bytes: np.ndarray, actions=None, group_names=(),
                reachability_graph: Optional[ReachabilityGraph] = None):
    """(sim_agents, world, t, flags) of one env from its canonical state bytes
    (oc_testlib.env_view order: ax[A] ay[A] ah[A] loc[K] mask[K] t_lo t_hi flags);
    `group_names`: object names whose (possibly empty) groups the world keeps."""
    b = [int(v) for v in env_bytes]
    ax, ay, ah = b[0:A], b[A:2 * A], b[2 * A:3 * A]
    loc, mask, t, flags, dead = _decode_items(b, A, K)
    held = {h: a for a, h in enumerate(ah) if h != _levels.HOLD_NONE}
    items = {}
    for j in range(K):
        if loc[j] == dead:
            continue
        items[j] = ItemView(j, mask[j], level.xy(loc[j]), j in held, level.encoding)
    agents = []
    for a in range(A):
        act = None if actions is None else actions[a]
        agents.append(SimAgentView("agent-%d" % (a + 1), COLORS[a], (ax[a], ay[a]), items.get(ah[a]), act))
    return agents, WorldView(level, list(items.values()), group_names, reachability_graph), t, flags


# ---------------------------------------------------------------------------------------
# Single env: the reference class surface
# ---------------------------------------------------------------------------------------
class OvercookedEnvironment:
    """Drop-in for gym_cooking.envs.OvercookedEnvironment, stepped by the HIP engine."""

    def __init__(self, arglist=None, device="cuda:0", **kwargs):
        if arglist is None:
            arglist = types.SimpleNamespace(level=kwargs.pop("level"), num_agents=kwargs.pop("num_agents"),
                                            max_num_timesteps=kwargs.pop("max_num_timesteps", 100),
                                            seed=kwargs.pop("seed", 1), model1=None, model2=None,
                                            model3=None, model4=None, record=False, with_image_obs=False)
        self.arglist = arglist
        self.t = 0
        self.set_filename()
        self.rep = []
        self.collisions: List[CollisionRepr] = []
        self.termination_info = ""
        self.successful = False
        self._device = device
        self._engine = None
        self._host = None
        self._group_names = frozenset()
        self._step_raises = False
        self._draw = None  # render.DrawOrder: world.objects order for get_image_obs
        self.game = None

    # -- reference bookkeeping ------------------------------------------------------------
    def set_filename(self):  # overcooked_environment.py:116-128
        a = self.arglist
        self.filename = "{}_agents{}_seed{}".format(a.level, a.num_agents, getattr(a, "seed", 1))
        for i in range(1, 5):
            m = getattr(a, "model%d" % i, None)
            if m is not None:
                self.filename += "_model%d-%s" % (i, m)

    def _ensure_engine(self):
        if self._engine is None:
            from .engine import OvercookedBatch  # raises without liboc_engine.so / a GPU
            level = self.arglist.level
            self.level = _levels.load_level(level) if isinstance(level, str) else level
            if self.level.missing:  # reset raises KeyError in make_reachability_graph (world.py:79-86)
                raise KeyError(self.level.reset_key_error())
            # squares past the world width: reset works and every step raises after executing
            # (display -> World.add_object, overcooked_environment.py:283 -> world.py:302)
            self._step_raises = bool(self.level.overflow)
            self._engine = _Single(OvercookedBatch(self.level.within_width(), self.arglist.num_agents, 1,
                                                   max_T=self.arglist.max_num_timesteps, device=self._device))
        return self._engine

    def _refresh(self, actions=None):
        eng = self._engine
        self.sim_agents, self.world, self.t, self._flags = build_views(self.level, eng.A, eng.K, self._host, actions,
                                                                       sorted(self._group_names), eng.reach)
        self._group_names = self._group_names | {it.name for it in self.world.items}

    # -- gym API ----------------------------------------------------------------------------
    def reset(self):  # :201-250
        eng = self._ensure_engine()
        self.agent_actions = {}
        self.rep = []
        self.collisions = []
        self.termination_info = ""
        self.successful = False
        self.recipes = list(self.level.recipes)
        self.all_subtasks = _recipes.all_subtasks(self.level, getattr(self.arglist, "max_num_subtasks", 14))
        self._group_names = frozenset()
        self._host = eng.reset()
        self._refresh()
        from .render import DrawOrder
        self._draw = DrawOrder(self.level, eng.K)
        if getattr(self.arglist, "record", False) or getattr(self.arglist, "with_image_obs", False):
            self.game = _GameImage(self)  # GameImage(filename, world, sim_agents) (:232-240)
        self.obs_tm1 = _copy.copy(self)
        return _copy.copy(self)

    def close(self):  # :252-253
        return

    def step(self, action_dict):  # :255-306
        eng = self._engine
        if eng is None or self._host is None:
            raise RuntimeError("call reset() before step()")
        names = self.get_agent_names()
        codes = [action_code(action_dict[n]) for n in names]
        if eng.A >= 2 and self.level.edge and any(
                self.level.off_grid(a.location[0], a.location[1], codes[names.index(a.name)]) for a in self.sim_agents):
            # an action off the grid: step raises in check_collisions (is_collision looks the
            # unclamped square up, :692-700; world.py:429 asserts).  What the reference has done by
            # then: t += 1 (:257), every sim_agent.action set (:263-264), and a CollisionRepr for
            # each earlier pair (in combinations order) that collided (:731-752)
            self.t += 1
            for a in self.sim_agents:
                a.action = _levels.ACTIONS[codes[names.index(a.name)]]
            for i in range(eng.A):
                for j in range(i + 1, eng.A):
                    ai, aj = self.sim_agents[i], self.sim_agents[j]
                    exec_ = is_collision(self.world, ai.location, aj.location, ai.action, aj.action)  # may raise
                    if not all(exec_):
                        self.collisions.append(CollisionRepr(time=self.t, agent_names=[ai.name, aj.name],
                                                             agent_locations=[ai.location, aj.location]))
            raise AssertionError("off-grid action without a raise")  # unreachable: some pair raised above
        pre = self._host
        new, ex, coll = eng.step(pre, codes)
        t_now = self.t + 1
        # collision log (check_collisions :724-757): pairs in combinations order
        p = 0
        for i in range(eng.A):
            for j in range(i + 1, eng.A):
                if (coll >> p) & 1:
                    self.collisions.append(CollisionRepr(time=t_now, agent_names=[names[i], names[j]],
                                                         agent_locations=[self.sim_agents[i].location,
                                                                          self.sim_agents[j].location]))
                p += 1
        executed = [_levels.ACTIONS[c] for c in ex]
        # obs_tm1: the state before execution, with the post-collision actions (:273)
        self.obs_tm1 = _copy.copy(self)
        self.obs_tm1.t = t_now  # the reference increments t before the copy (:257, :273)
        for a, act in zip(self.obs_tm1.sim_agents, executed):
            a.action = act
        self._host = new
        self._draw.update(_object_planes(pre, eng.A, eng.K), _object_planes(new, eng.A, eng.K))
        self._refresh(executed)
        self.agent_actions = {n: act for n, act in zip(names, executed)}
        if self._step_raises:
            raise IndexError("list assignment index out of range")  # world.py:302
        if self._flags & FLAG_ERR:
            raise CopyCrash("two co-located agents both hold items: the reference crashes in copy.copy "
                            "(overcooked_environment.py:289 -> world.py:417)")
        new_obs = _copy.copy(self)
        image_obs = self.game.get_image_obs() if self.game is not None else None
        done = self.done()
        reward = self.reward()
        info = {"t": self.t, "obs": new_obs, "image_obs": image_obs, "done": done,
                "termination_info": self.termination_info}
        return new_obs, reward, done, info

    def done(self):  # :316-363 (evaluated by the engine; timeout takes precedence)
        mt = self.arglist.max_num_timesteps
        if self.t >= mt and mt:
            self.termination_info = "Terminating because passed {} timesteps".format(mt)
            self.successful = False
            return True
        if self._flags & FLAG_SUCCESS:
            self.termination_info = "Terminating because all deliveries were completed"
            self.successful = True
            return True
        self.termination_info = ""
        self.successful = False
        return False

    def reward(self):  # :365-376
        return 1 if self.successful else 0

    # -- queries the planners use ------------------------------------------------------------
    def get_repr(self):  # :50-62
        return self.world.get_repr() + tuple(a.get_repr() for a in self.sim_agents)

    def __eq__(self, other):
        return isinstance(other, OvercookedEnvironment) and self.get_repr() == other.get_repr()

    def __hash__(self):
        return hash(self.get_repr())

    def __str__(self):
        return "\n".join("".join(c + " " for c in row) for row in self._display_rows())

    def _display_rows(self):
        chars = {"Floor": " ", "Counter": "-", "Cutboard": "/", "Delivery": "*"}
        rows = [[chars[_TILE_NAMES[self.level.tile_at(x, y)]] for x in range(self.world.width)]
                for y in range(self.world.height)]
        for it in self.world.items:
            x, y = it.location
            rows[y][x] = it.full_name[0].lower() if it.full_name else rows[y][x]
        for a in self.sim_agents:
            x, y = a.location
            rows[y][x] = a.name[-1]
        return rows

    def __copy__(self):  # :100-114 -- a snapshot sharing the engine handle
        new = object.__new__(OvercookedEnvironment)
        new.__dict__ = self.__dict__.copy()
        if self._host is not None:
            new._host = self._host.copy()
            new._refresh([a.action for a in self.sim_agents])
        new.collisions = list(self.collisions)
        return new

    def get_agent_names(self) -> List[str]:
        return [a.name for a in self.sim_agents]

    def is_collision(self, agent1_loc, agent2_loc, agent1_action, agent2_action):  # :671-722
        return is_collision(self.world, agent1_loc, agent2_loc, agent1_action, agent2_action)

    def get_AB_locs_given_objs(self, subtask, subtask_agent_names, start_obj, goal_obj, subtask_action_obj):
        """overcooked_environment.py:480-589: (A_locs, B_locs) of a subtask -- un-held start
        objects plus the subtask agents holding one; Cutboard / Delivery squares for Chop /
        Deliver (Deliver drops A locations already on a Delivery)."""
        w = self.world

        def held_by_subtask_agents(obj):
            return [a.location for a in self.sim_agents if a.name in subtask_agent_names and a.holding == obj]

        name = None if subtask is None else subtask.name
        if name == "Chop":
            return (w.get_object_locs(start_obj, is_held=False) + held_by_subtask_agents(start_obj),
                    w.get_all_object_locs(subtask_action_obj))
        if name == "Deliver":
            B_locs = w.get_all_object_locs(subtask_action_obj)
            A_locs = w.get_object_locs(start_obj, is_held=False) + held_by_subtask_agents(start_obj)
            return [a for a in A_locs if a not in B_locs], B_locs
        if name == "Merge":
            return (w.get_object_locs(start_obj[0], is_held=False) + held_by_subtask_agents(start_obj[0]),
                    w.get_object_locs(start_obj[1], is_held=False) + held_by_subtask_agents(start_obj[1]))
        return [], []

    def get_lower_bound_for_subtask_given_objs(self, subtask, subtask_agent_names, start_obj=None, goal_obj=None,
                                               subtask_action_obj=None):
        """overcooked_environment.py:594-664, evaluated by the oc_subtask_bounds kernel on this
        env's state.  The objects are the ones get_subtask_obj / get_subtask_action_obj give for
        `subtask` (the only ones the reference passes); they are implied by it."""
        assert len(subtask_agent_names) <= 2, 'passed in {} agents but can only do 1 or 2'.format(
            len(subtask_agent_names))
        lb, _ = self._subtask_bound(subtask, subtask_agent_names)
        return lb

    def subtask_alloc_is_doable(self, subtask, subtask_agent_names) -> bool:
        """BayesianDelegator.subtask_alloc_is_doable(env, ...) (bayesian_delegator.py:98-156),
        evaluated by the oc_subtask_bounds kernel on this env's state."""
        if subtask is None:
            return True
        _, ok = self._subtask_bound(subtask, subtask_agent_names)
        return ok

    def _subtask_bound(self, subtask, subtask_agent_names):
        names = self.get_agent_names()
        agents = sorted(names.index(n) for n in subtask_agent_names)
        kind, starts, goal = _recipes.subtask_masks(subtask, self.level.encoding)
        lb, ok = self._engine.bounds(self._host, [capi.subtask(kind, agents, list(starts), goal, 0)])
        return float(lb[0]), bool(ok[0])

    def state_bytes(self) -> np.ndarray:
        """The env's state bytes (ax[A] ay[A] ah[A] loc[K] mask[K] t_lo t_hi flags)."""
        return self._host.copy()

    def load_state(self, env_bytes) -> None:
        """Set the env's state from state bytes (same order as :meth:`state_bytes`)."""
        self._ensure_engine()
        b = np.asarray(env_bytes, dtype=np.uint8).copy()
        if b.shape != (self._engine.NP,):
            raise ValueError("expected %d state bytes, got %s" % (self._engine.NP, b.shape))
        self._host = b
        self._group_names = frozenset()
        from .render import DrawOrder
        self._draw = DrawOrder(self.level, self._engine.K)
        self._draw.sync(_object_planes(b, self._engine.A, self._engine.K))
        self._refresh()


def _object_planes(env_bytes: np.ndarray, A: int, K: int) -> Dict[str, np.ndarray]:
    """The held-slot, location and mask planes of one env's state bytes (render.DrawOrder);
    the shim steps a finished env again (it clears DONE), so no auto-reset is implied."""
    if len(env_bytes) == 3 * A + 3 * K + 3:  # wide layout: DrawOrder reads only whether a slot is live
        dead = (env_bytes[3 * A:3 * A + K] == 0xFF) & (env_bytes[3 * A + K:3 * A + 2 * K] == 0xFF)
        return {"ah": env_bytes[2 * A:3 * A], "loc": np.where(dead, 0xFF, 0).astype(np.uint8),
                "mask": env_bytes[3 * A + 2 * K:3 * A + 3 * K]}
    return {"ah": env_bytes[2 * A:3 * A], "loc": env_bytes[3 * A:3 * A + K], "mask": env_bytes[3 * A + K:3 * A + 2 * K]}


class _GameImage:
    """``env.game`` (misc/game/gameimage.py:10-51): ``get_image_obs()`` renders the env's
    current state on the GPU (oc_render_ordered, objects of one square in the reference's
    world.objects order) and returns the reference's u8 [H*80, W*80, 3] array."""

    def __init__(self, env):
        self._env = env
        self._renderer = None
        self._rank = None

    def get_image_obs(self) -> np.ndarray:
        env = self._env
        single = env._engine
        if self._renderer is None:
            from .render import Renderer
            self._renderer = Renderer(single.b)
            self._rank = torch.zeros((single.K, single.P), dtype=torch.uint8, device=single.b.device)
        single._upload(env._host, single.s_in)
        self._rank[:, 0] = torch.from_numpy(env._draw.ranks())
        return self._renderer.render(single.s_in, draw_rank=self._rank)[0].cpu().numpy()


class _Single:
    """One env row of an OvercookedBatch(B=1): host canonical bytes in, host bytes out."""

    def __init__(self, batch):
        self.b = batch
        self.A, self.K, self.P = batch.A, batch.K, batch.pitch
        self.NP = batch.layout.num_planes
        self.s_in, self.s_out = batch.new_state(), batch.new_state()
        self.act, self.ex, self.coll = batch.new_actions(), batch.new_exec(), batch.new_coll()
        self._t = batch.layout.plane_t
        try:
            node_of, dist = batch.reachability()
            self.reach = ReachabilityGraph(batch.level.width, node_of, dist)
        except capi.LevelError:  # graph past the planner tables' envelope: stepping still works
            self.reach = None

    def _download(self, buf) -> np.ndarray:
        host = buf.view(self.NP, self.P)[:, :2].cpu().numpy()  # env 0 of every plane (+ t's high byte)
        out = host[:, 0].copy()
        out[self._t + 1] = host[self._t, 1]  # t is u16 at byte 0..1 of the two t planes' row
        return out

    def _upload(self, env_bytes: np.ndarray, buf):
        rows = np.zeros((self.NP, 2), np.uint8)
        rows[:, 0] = env_bytes
        rows[self._t, 0], rows[self._t, 1] = env_bytes[self._t], env_bytes[self._t + 1]
        rows[self._t + 1, :] = 0
        buf.view(self.NP, self.P)[:, :2].copy_(torch.from_numpy(rows))

    def reset(self) -> np.ndarray:
        self.b.reset(self.s_in)
        return self._download(self.s_in)

    def bounds(self, env_bytes: np.ndarray, subtasks):
        """oc_subtask_bounds of this env: (lb f32 [S], doable u8 [S])."""
        self._upload(env_bytes, self.s_in)
        lb, ok = self.b.subtask_bounds(self.s_in, subtasks)
        return lb[:, 0].cpu().numpy(), ok[:, 0].cpu().numpy()

    def step(self, env_bytes: np.ndarray, codes: Sequence[int]):
        cur = env_bytes.copy()
        cur[-1] &= ~np.uint8(FLAG_DONE)  # no auto-reset for the single env: the reference keeps stepping
        self._upload(cur, self.s_in)
        self.act.view(self.A, self.P)[:, 0].copy_(torch.tensor(list(codes), dtype=torch.uint8))
        self.b.step(self.s_in, self.s_out, self.act, self.ex, self.coll)
        new = self._download(self.s_out)
        ex = self.ex.view(self.A, self.P)[:, 0].cpu().tolist()
        coll = int(self.coll[0].item())
        return new, ex, coll


# ---------------------------------------------------------------------------------------
# Batched vector env
# ---------------------------------------------------------------------------------------
class OvercookedVecEnv:
    """B kitchens on one GPU with the gym vector-env shape of API.

    ``reset()`` returns the state buffer; ``step(actions)`` takes ``uint8 [A, B]`` action
    codes (or ``[A, pitch]``) and returns ``(state, reward[B] int8, done[B] bool, info)``
    where ``info`` holds the executed actions ``[A, B]`` and the collision-pair masks ``[B]``.
    Envs that were done at the input are reset to the level template by the engine in the
    same launch (next-step auto-reset).  All tensors stay on the GPU.

    ``observe(dtype, view_agent)`` returns the grid observation ``[B, C, H, W]`` of the current
    states (``C = 10 + A`` count planes: Counter, Cutboard, Delivery, Fresh/Chopped Tomato,
    Lettuce, Onion, Plate, one per agent; ``uint8`` or ``float16``; with ``view_agent = a`` the
    agent planes are rotated so that agent a is plane 10), and ``action_mask()`` the legal moves
    ``uint8 [A, B]`` (bit k: ``World.NAV_ACTIONS[k]`` is in the reference's
    ``get_single_actions``; bit 4, the no-op, always).  Both reuse their buffers between calls
    (oc_observe); ``render()`` gives the reference's 560x560 image instead, at 1,600 times the bytes.

    ``subtasks`` is ``recipes.all_subtasks(level)`` (the reference env's ``all_subtasks``), and
    ``progress(weights)`` gives, for the last ``step()``, the goal-object count of each of them per
    env (``RealAgent.def_subtask_completion``), the completion events of the step
    (``is_subtask_complete``; bit b of plane c is subtask 8c + b) and a shaped reward, the sum
    of ``weights`` over the events (oc_progress).  It is opt-in: ``step()`` does not compute it.

    ``random_starts`` (``capi.OC_START_AGENTS | capi.OC_START_ITEMS``, default 0: the level's own
    start everywhere, exactly as without the argument) randomises episode starts with ``seed``:
    ``reset()`` draws every env's agents and / or item cells (oc_reset_random, the reset of the level
    file with its item letters and spawn lines moved), and ``step()`` follows its launch with the
    masked call that redraws exactly the envs the step auto-reset, at round = the number of
    ``step()`` calls so far.  ``batch.set_start_cells`` narrows or widens the eligible cells.
    """

    def __init__(self, level, num_agents: int, num_envs: int, max_num_timesteps: int = 100, device="cuda:0",
                 random_starts: int = 0, seed: int = 0):
        from .engine import OvercookedBatch
        self.batch = OvercookedBatch(level, num_agents, num_envs, max_T=max_num_timesteps, device=device)
        self.num_envs, self.A, self.P = num_envs, num_agents, self.batch.pitch
        self._s = [self.batch.new_state(), self.batch.new_state()]
        self._i = 0
        self._act = self.batch.new_actions()
        self.ex, self.coll = self.batch.new_exec(), self.batch.new_coll()
        self.stats = self.batch.new_stats()
        self._fl = self.batch.layout.plane_flags
        self._stepped = False  # progress(): whether the other ping-pong buffer is the state before
        self.random_starts, self.seed = int(random_starts), int(seed)
        self._round = 0  # step() calls so far: the round of the next draw

    @property
    def state(self) -> torch.Tensor:
        return self._s[self._i]

    @property
    def subtasks(self):
        """recipes.all_subtasks(level): the order names the bits of progress()'s events."""
        if getattr(self, "_subtasks", None) is None:
            self._subtasks = _recipes.all_subtasks(self.batch.level)
            self._sub_rows = capi.progress_subtasks(self._subtasks, self.batch.level.encoding)
        return self._subtasks

    def planes(self) -> Dict[str, torch.Tensor]:
        return self.batch.planes(self.state)

    def reset(self) -> torch.Tensor:
        self.batch.reset(self.state)  # the whole pitch: the columns past B hold the template, as always
        if self.random_starts:
            self.batch.reset_random(self.state, None, self.seed, self._round, self.random_starts)
        self._stepped = False
        self._task_round = None  # partner_tasks(): the next call starts every env over
        self._belief_round = None  # partner_beliefs(): likewise
        self._team_round = None  # team_tasks(): likewise
        self._tbelief_round = None  # team_beliefs(): likewise
        return self.state

    def step(self, actions: torch.Tensor):
        B, P = self.num_envs, self.P
        if actions.dtype == torch.uint8 and actions.shape[-1] == P and actions.is_contiguous():
            act = actions.reshape(-1)
        else:  # copy_ converts any integer dtype to the u8 codes the kernel reads
            self._act.view(self.A, P)[:, :B].copy_(actions.reshape(self.A, B))
            act = self._act
        src, dst = self._s[self._i], self._s[self._i ^ 1]
        self.batch.step(src, dst, act, self.ex, self.coll, self.stats)
        self._round += 1
        if self.random_starts:  # the envs this step auto-reset (DONE in src) get a drawn start
            self.batch.reset_random(dst, src, self.seed, self._round, self.random_starts)
        self._i ^= 1
        self._stepped = True
        fl = dst.view(-1, P)[self._fl, :B]
        done = (fl & FLAG_DONE) != 0
        reward = ((fl & FLAG_SUCCESS) != 0).to(torch.int8)
        info = {"exec_actions": self.ex.view(self.A, P)[:, :B], "collisions": self.coll[:B],
                "error": (fl & FLAG_ERR) != 0}
        return dst, reward, done, info

    def render(self, channels: str = "reference", draw_rank: Optional[torch.Tensor] = None) -> torch.Tensor:
        """u8 [B, H*80, W*80, 3] image observations of the current states (oc_render_ordered;
        `draw_rank`: optional u8 [K, pitch] per-slot draw ranks, see render.DrawOrder)."""
        if getattr(self, "_renderer", None) is None:
            from .render import Renderer
            self._renderer = Renderer(self.batch)
        return self._renderer.render(self.state, channels=channels, draw_rank=draw_rank)

    def observe(self, dtype=torch.uint8, view_agent: int = -1) -> torch.Tensor:
        """[B, C, H, W] grid observation of the current states (oc_observe; the class docstring
        lists the planes).  The tensor is this env's buffer for `dtype`, rewritten by the next call."""
        bufs = self.__dict__.setdefault("_obs", {})
        if dtype not in bufs:
            bufs[dtype] = self.batch.new_obs(dtype)
        self.batch.observe(self.state, obs=bufs[dtype], view_agent=view_agent)
        return bufs[dtype]

    def action_mask(self) -> torch.Tensor:
        """u8 [A, B] legal-move masks of the current states (oc_observe): bit k set iff
        World.NAV_ACTIONS[k] is in get_single_actions(env, agent), bit 4 (no-op) always.  A view of
        this env's buffer, rewritten by the next call."""
        if getattr(self, "_mask", None) is None:
            self._mask = self.batch.new_action_mask()
        self.batch.observe(self.state, action_mask=self._mask)
        return self._mask.view(self.A, self.P)[:, :self.num_envs]

    def progress(self, weights=None) -> Dict[str, torch.Tensor]:
        """Subtask progress of the last step() (oc_progress over the two ping-pong buffers):
        {"counts": u8 [S, B], "events": u8 [planes, B], "reward": f32 [B]} for S = len(subtasks).
        Before the first step (and after reset()) the state is compared with itself: no events,
        valid counts.  Views of this env's buffers, rewritten by the next call."""
        S = len(self.subtasks)
        if S == 0:
            raise ValueError("the level's recipes have no subtasks")
        if getattr(self, "_prog", None) is None:
            self._prog = self.batch.new_progress_buffers(S)
        prev = self._s[self._i ^ 1] if self._stepped else self.state
        c, e, r = self._prog
        self.batch.progress(prev, self.state, self._sub_rows, weights, 1, c, e, r)
        B = self.num_envs
        return {"counts": c[0, :, :B], "events": e[0, :, :B], "reward": r[0, :B]}

    def partner_actions(self, table, alloc: Optional[torch.Tensor] = None, beta: float = 1.3,
                        mode: int = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE,
                        out: Optional[torch.Tensor] = None):
        """Scripted-partner actions of the current states (oc_nav_policy): every env's subtask agents
        follow the oc_subtask row `table[alloc[env]]` (capi.policy_subtasks makes the rows; `alloc`
        u8 [pitch], None: row 0) as the reference's Boltzmann-rational agent, p(a) ~ exp(-beta Q).
        Only those agents' bytes of `out` (u8 [A, pitch]; None: this env's buffer) are written, so a
        learner's actions already in it survive; the draw uses the env's seed and the number of
        step() calls so far.  Returns (the [A, B] view of `out`, flags u8 [B] of capi.POL_*)."""
        if out is None:
            if getattr(self, "_partner", None) is None:
                self._partner = self.batch.new_actions()
                self._partner_flags = torch.empty(self.P, dtype=torch.uint8, device=self.batch.device)
            out = self._partner
        if getattr(self, "_partner_flags", None) is None:
            self._partner_flags = torch.empty(self.P, dtype=torch.uint8, device=self.batch.device)
        self.batch.nav_policy(self.state, table, out, beta=beta, mode=mode, alloc=alloc, step=self._round,
                              seed=self.seed, flags=self._partner_flags)
        return out.view(self.A, self.P)[:, :self.num_envs], self._partner_flags[:self.num_envs]

    def partner_tasks(self, agents, commit: bool = True, distinct: bool = True):
        """The subtask each scripted agent of `agents` (indices, in priority order) follows in the
        current states (oc_task_select over ``subtasks``): per env the reference agent's
        refresh_subtasks and then the doable incomplete subtask with the smallest lower bound;
        `commit` keeps the current one while it stays a candidate, `distinct` keeps two scripted
        agents off one subtask.  The task state lives in this env across step(): the first call
        after reset() (or with other agents) starts every env over, a call after a step starts over
        the envs that step auto-reset, and a second call on the same states starts none.  Returns
        (cur u8 [M, B]: the subtask index, len(subtasks) for None; info u8 [M, B] of capi.TASKF_*),
        views of this env's buffers."""
        agents = tuple(int(a) for a in agents)
        S = len(self.subtasks)
        if S == 0:
            raise ValueError("the level's recipes have no subtasks")
        M, EP = len(agents), capi.event_planes(S)
        flags = (capi.OC_TASK_COMMIT if commit else 0) | (capi.OC_TASK_DISTINCT if distinct else 0)
        if getattr(self, "_task_agents", None) != agents:
            self._task_agents = agents
            self._task = self.batch.new_task_state(S, M)
            self._task_info = torch.empty((M, self.P), dtype=torch.uint8, device=self.batch.device)
            self._task_round = None
        prev = None
        if self._task_round is None:
            flags |= capi.OC_TASK_INIT
        elif self._task_round != self._round:  # stepped since: the other buffer is the state before
            prev = self._s[self._i ^ 1]
        self._task_round = self._round
        self.batch.task_select(self.state, self._sub_rows, agents, self._task, prev, flags, None, self._task_info)
        B = self.num_envs
        return self._task[:, EP, :B], self._task_info[:, :B]

    def partner_beliefs(self, agents, beta: float = 1.3, none_action_prob: float = 0.5, use_events: bool = True):
        """What each watched agent of `agents` is doing, inferred from what it did
        (oc_belief_update over ``subtasks``): per env and watched agent the reference's Bayesian
        update of a posterior over "the agent alone follows subtask i" and None, over the last
        step(): hypotheses that are no longer doable leave, the others are multiplied by the
        Boltzmann likelihood (`beta`, `none_action_prob`) of the action the agent executed, and the
        result is normalised.  With `use_events` an oc_progress launch over the same step supplies
        the completion events, after which the priors start over uniform on the open subtasks.  The
        belief lives in this env across step(): the first call after reset() (or with other agents)
        initialises every env, a call after a step updates over that step (only the last one: call
        once per step) and starts over the envs it auto-reset, and a second call on the same states
        changes nothing.  Opt-in: step() does not compute it.  Returns (belief f64 [M, S + 1, B],
        hypothesis S being None; map u8 [M, B], the most likely hypothesis; info u8 [M, B] of
        capi.BELF_*), views of this env's buffers."""
        agents = tuple(int(a) for a in agents)
        S = len(self.subtasks)
        if S == 0:
            raise ValueError("the level's recipes have no subtasks")
        M, B = len(agents), self.num_envs
        if getattr(self, "_belief_agents", None) != agents:
            self._belief_agents = agents
            self._belief = self.batch.new_belief_state(S, M)
            self._belief_events = torch.zeros((1, capi.event_planes(S), self.P), dtype=torch.uint8,
                                              device=self.batch.device)
            self._belief_round = None
        bel, bst, bmap, info = self._belief
        if getattr(self, "_belief_round", None) is None:
            self.batch.belief_update(None, None, self._sub_rows, agents, bel, bst, None, beta, none_action_prob,
                                     capi.OC_BELIEF_INIT, bmap, info)
        elif self._belief_round != self._round:  # stepped since: the other buffer is the state before
            prev, events = self._s[self._i ^ 1], None
            if use_events:
                events = self._belief_events
                self.batch.progress(prev, self.state, self._sub_rows, None, 1, None, events, None)
            self.batch.belief_update(prev, self.ex, self._sub_rows, agents, bel, bst, events, beta, none_action_prob,
                                     0, bmap, info)
        self._belief_round = self._round
        return bel[:, :, :B], bmap[:, :B], info[:, :B]

    def scripted_actions(self, agents, beta: float = 1.3,
                         mode: int = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE,
                         out: Optional[torch.Tensor] = None, commit: bool = True, distinct: bool = True):
        """Actions of scripted partners that drive themselves: partner_tasks(agents) picks each
        agent's subtask per env, then partner_actions runs once per agent with that agent's
        one-agent table (the level's subtasks, then None) and its cur plane as `alloc`.  Only the
        scripted agents' bytes of `out` (u8 [A, pitch]; None: this env's buffer) are written.
        Returns (the [A, B] view of `out`, task info u8 [M, B])."""
        agents = tuple(int(a) for a in agents)
        _, info = self.partner_tasks(agents, commit, distinct)
        tables = self.__dict__.setdefault("_task_tables", {})
        EP = capi.event_planes(len(self.subtasks))
        view = None
        for m, a in enumerate(agents):
            if a not in tables:
                tables[a] = capi.policy_subtasks(list(self.subtasks) + [None], self.batch.level.encoding, [a])
            view, _ = self.partner_actions(tables[a], self._task[m, EP], beta, mode, out)
            out = self._partner if out is None else out
        return view, info

    def team_tasks(self, pair, commit: bool = True, split_first: bool = False):
        """The allocation the scripted pair `pair` = (a0, a1), a0 < a1, follows in the current states
        (oc_team_select over ``subtasks``): per env either both agents on one subtask (joint) or
        each on its own (split), the heaviest under the sum of 1 / lower bound over the members;
        `commit` keeps the current allocation while its members stay candidates, `split_first`
        prefers a split with two subtasks over any joint one.  The team state lives in this env
        across step() with partner_tasks' life cycle: the first call after reset() (or with another
        pair) starts every env over, a call after a step starts over the envs that step auto-reset,
        and a second call on the same states starts none.  Returns (cur0, cur1, curJ u8 [B]: a
        subtask index, len(subtasks) for None, capi.OC_TEAM_OUT where the env is not that plane's;
        info u8 [B] of capi.TEAMF_*), views of this env's buffers."""
        pair = tuple(int(a) for a in pair)
        S = len(self.subtasks)
        if S == 0:
            raise ValueError("the level's recipes have no subtasks")
        EP, B = capi.event_planes(S), self.num_envs
        flags = (capi.OC_TEAM_COMMIT if commit else 0) | (capi.OC_TEAM_SPLIT_FIRST if split_first else 0)
        if getattr(self, "_team_pair", None) != pair:
            self._team_pair = pair
            self._team = self.batch.new_team_state(S)
            self._team_info = torch.empty(self.P, dtype=torch.uint8, device=self.batch.device)
            self._team_round = None
        prev = None
        if self._team_round is None:
            flags |= capi.OC_TEAM_INIT
        elif self._team_round != self._round:  # stepped since: the other buffer is the state before
            prev = self._s[self._i ^ 1]
        self._team_round = self._round
        self.batch.team_select(self.state, self._sub_rows, pair, self._team, prev, flags, None, self._team_info)
        return self._team[EP, :B], self._team[EP + 1, :B], self._team[EP + 2, :B], self._team_info[:B]

    def team_actions(self, pair, beta: float = 1.3,
                     mode: int = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE,
                     out: Optional[torch.Tensor] = None, commit: bool = True, split_first: bool = False):
        """Actions of a scripted pair that drives itself: team_tasks(pair) picks each env's
        allocation, then three oc_nav_policy launches on one stream act on it: a0's one-agent table
        (the level's subtasks, then None) with plane cur0 as `alloc`, a1's with plane cur1, and the
        two-agent table with plane curJ.  An env is written by the launches its allocation names and
        skipped (capi.POL_BADALLOC) by the others; ``team_flags`` u8 [3, pitch] keeps each launch's
        flags.  Only the pair's bytes of `out` (u8 [A, pitch]; None: this env's buffer) are written.
        Returns (the [A, B] view of `out`, team info u8 [B])."""
        pair = tuple(int(a) for a in pair)
        *_, info = self.team_tasks(pair, commit, split_first)
        if out is None:
            if getattr(self, "_partner", None) is None:
                self._partner = self.batch.new_actions()
            out = self._partner
        if getattr(self, "team_flags", None) is None:
            self.team_flags = torch.zeros((3, self.P), dtype=torch.uint8, device=self.batch.device)
        tables = self.__dict__.setdefault("_team_tables", {})
        if pair not in tables:
            enc = self.batch.level.encoding
            tables[pair] = (capi.policy_subtasks(list(self.subtasks) + [None], enc, [pair[0]]),
                            capi.policy_subtasks(list(self.subtasks) + [None], enc, [pair[1]]),
                            capi.policy_subtasks(list(self.subtasks), enc, pair))
        EP = capi.event_planes(len(self.subtasks))
        for q, (table, ncand) in enumerate(zip(tables[pair], (5, 5, 25))):
            self.batch.nav_policy(self.state, table, out, beta=beta, mode=mode, alloc=self._team[EP + q], step=self._round,
                                  seed=self.seed, num_cand=ncand, flags=self.team_flags[q])
        return out.view(self.A, self.P)[:, :self.num_envs], info

    def team_beliefs(self, pair, self_agent: int, beta: float = 1.3, none_action_prob: float = 0.5,
                     use_events: bool = True):
        """What the pair `pair` = (a0, a1), a0 < a1, is doing together, as the delegator `self_agent`
        (a0 or a1) infers it from what both did (oc_team_belief_update over ``subtasks``): per env
        the reference's Bayesian Delegation posterior over "both on subtask t" and "a0 on i, a1 on
        j" (None allowed for one member), updated over the last step() with both executed actions.
        partner_beliefs' life cycle: the first call after reset() (or with another pair or self
        agent) initialises every env, a call after a step updates over that step (only the last one:
        call once per step) and starts over the envs it auto-reset, and a second call on the same
        states changes nothing.  Opt-in: step() does not compute it; the matrix costs
        (S + 1)^2 * 8 bytes per env.  Returns (belief f64 [N, N, B] with N = S + 1: entry (i, j) the
        split for i != j, the joint for i == j < S, index S None, (S, S) unused; cur0, cur1, curJ u8
        [B], the most likely allocation in team_tasks' format; info u8 [B] of capi.TBELF_*), views of
        this env's buffers."""
        pair = tuple(int(a) for a in pair)
        S = len(self.subtasks)
        if S == 0:
            raise ValueError("the level's recipes have no subtasks")
        B, N = self.num_envs, S + 1
        key = (pair, int(self_agent))
        if getattr(self, "_tbelief_key", None) != key:
            self._tbelief_key = key
            self._tbelief = self.batch.new_team_belief_state(S, lik=False)  # the likelihoods are not kept here
            self._tbelief_events = torch.zeros((1, capi.event_planes(S), self.P), dtype=torch.uint8,
                                               device=self.batch.device)
            self._tbelief_round = None
        bel, tbs, _, tmap, info = self._tbelief
        if getattr(self, "_tbelief_round", None) is None:
            self.batch.team_belief_update(None, None, self._sub_rows, pair, self_agent, bel, tbs, None, beta,
                                          none_action_prob, capi.OC_TBELIEF_INIT, None, tmap, info)
        elif self._tbelief_round != self._round:  # stepped since: the other buffer is the state before
            prev, events = self._s[self._i ^ 1], None
            if use_events:
                events = self._tbelief_events
                self.batch.progress(prev, self.state, self._sub_rows, None, 1, None, events, None)
            self.batch.team_belief_update(prev, self.ex, self._sub_rows, pair, self_agent, bel, tbs, events, beta,
                                          none_action_prob, 0, None, tmap, info)
        self._tbelief_round = self._round
        return bel.view(N, N, self.P)[:, :, :B], tmap[0, :B], tmap[1, :B], tmap[2, :B], info[:B]

    def delegate_actions(self, self_agent: int, other: int, beta: float = 1.3,
                         mode: int = capi.OC_POLICY_SAMPLE | capi.OC_POLICY_COUNT_STATE,
                         out: Optional[torch.Tensor] = None, none_action_prob: float = 0.5, use_events: bool = True):
        """Actions of a Bayesian-delegation partner `self_agent` beside the agent `other` (a learner,
        say): team_beliefs infers the pair's allocation from what both did, and the partner plays its
        own member of the most likely one.  Two oc_nav_policy launches: self's one-agent table (the
        level's subtasks, then None) with self's cur plane as `alloc` writes into `out`; the
        two-agent table with plane curJ writes into a private scratch buffer, and self's row of it
        is copied into `out` where the allocation is joint.  Only self's bytes of `out` (u8 [A,
        pitch]; None: this env's buffer) are ever written: the other agent's survive.
        Returns (the [A, B] view of `out`, belief info u8 [B])."""
        me, other = int(self_agent), int(other)
        if me == other:
            raise ValueError("delegate_actions: self_agent and other are one agent")
        pair = (min(me, other), max(me, other))
        _, cur0, cur1, curJ, info = self.team_beliefs(pair, me, beta, none_action_prob, use_events)
        if out is None:
            if getattr(self, "_partner", None) is None:
                self._partner = self.batch.new_actions()
            out = self._partner
        if getattr(self, "_delegate_scratch", None) is None:
            self._delegate_scratch = self.batch.new_actions()
            self.delegate_flags = torch.zeros((2, self.P), dtype=torch.uint8, device=self.batch.device)
        tables = self.__dict__.setdefault("_delegate_tables", {})
        if (me, other) not in tables:
            enc = self.batch.level.encoding
            tables[(me, other)] = (capi.policy_subtasks(list(self.subtasks) + [None], enc, [me]),
                                   capi.policy_subtasks(list(self.subtasks), enc, pair))
        own, joint = tables[(me, other)]
        tmap = self._tbelief[3]
        S = len(self.subtasks)
        self.batch.nav_policy(self.state, own, out, beta=beta, mode=mode, alloc=tmap[0 if me == pair[0] else 1],
                              step=self._round, seed=self.seed, num_cand=5, flags=self.delegate_flags[0])
        self.batch.nav_policy(self.state, joint, self._delegate_scratch, beta=beta, mode=mode, alloc=tmap[2],
                              step=self._round, seed=self.seed, num_cand=25, flags=self.delegate_flags[1])
        B = self.num_envs
        mine, theirs = out.view(self.A, self.P)[me, :B], self._delegate_scratch.view(self.A, self.P)[me, :B]
        torch.where(tmap[2, :B] < S, theirs, mine, out=mine)
        return out.view(self.A, self.P)[:, :self.num_envs], info

    def episode_stats(self) -> torch.Tensor:
        """int64 [episodes, successes, steps, collisions, errors] since construction."""
        return self.batch.reduce_stats(self.stats)


def register(env_id: str = "overcookedEnv-v0") -> bool:
    """Register the shim with gym under the reference's id (gym_cooking/__init__.py:3-6)
    when gym is importable; returns whether it did."""
    try:
        from gym.envs.registration import register as _reg
    except ImportError:
        return False
    _reg(id=env_id, entry_point="gym_cooking_amd.envs:OvercookedEnvironment")
    return True
