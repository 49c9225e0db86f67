"""Numpy restatement of the randomised-start contract (include/oc_engine.h, oc_reset_random): the
default lists, the draws and the skip rule, each written directly from its definition (the "r-th
cell that nobody took" is a cumulative count over the list, not the engine's fixed-point walk),
plus a writer of level text with moved item letters and spawn lines (the reference's load_level,
gym_cooking/envs/overcooked_environment.py:144-193, builds exactly the drawn start from it)."""
from __future__ import annotations

import numpy as np

from gym_cooking_amd import capi, levels

START_AGENTS, START_ITEMS = 1, 2
GOLD, STEPC, TAG = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x53540000
_U = np.uint64


def splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = x + _U(GOLD)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def base_of(B: int, env_offset: int, seed: int, rnd: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        gid = np.arange(B, dtype=np.uint64) + _U(env_offset)
        return _U(seed) ^ (gid * _U(GOLD)) ^ _U((rnd * STEPC) & ((1 << 64) - 1))


def r_of(base: np.ndarray, d: int, n: np.ndarray) -> np.ndarray:
    """r(d, n) = (uint32)(((u(d) >> 32) * n) >> 32), n per env."""
    u = splitmix64(base ^ _U(TAG + d))
    return (((u >> _U(32)) * n.astype(np.uint64)) >> _U(32)).astype(np.int64)


def default_masks(level, A: int):
    """(agent_ok [A, cells], item_ok [cells]) of the defaults: the Floor cells 4-connected through
    Floor to spawn i; the Counter cells with a Floor 4-neighbour."""
    W, H = level.width, level.height
    tiles = np.array(level.tiles).reshape(H, W)

    def nbrs(x, y):
        return [(x + dx, y + dy) for dx, dy in ((0, 1), (0, -1), (-1, 0), (1, 0)) if 0 <= x + dx < W and 0 <= y + dy < H]
    agent_ok = np.zeros((A, W * H), np.uint8)
    for i in range(A):
        seen, todo = {tuple(level.spawns[i])}, [tuple(level.spawns[i])]
        while todo:
            x, y = todo.pop()
            for n in nbrs(x, y):
                if tiles[n[1], n[0]] == levels.TILE_FLOOR and n not in seen:
                    seen.add(n)
                    todo.append(n)
        for x, y in seen:
            agent_ok[i, y * W + x] = 1
    item_ok = np.zeros(W * H, np.uint8)
    for y in range(H):
        for x in range(W):
            if tiles[y, x] == levels.TILE_COUNTER and any(tiles[ny, nx] == levels.TILE_FLOOR for nx, ny in nbrs(x, y)):
                item_ok[y * W + x] = 1
    return agent_ok, item_ok


def _pick(L: np.ndarray, taken: np.ndarray, d: int, base: np.ndarray) -> np.ndarray:
    """Per env the r(d, |L| - m)-th cell of L (ascending) not in that env's `taken` [n, B], m the
    taken cells that are in L."""
    B = len(base)
    free = np.ones((B, len(L)), bool)
    for row in taken:
        free &= L[None, :] != row[:, None]
    nfree = free.sum(1)
    assert (nfree >= 1).all()
    r = r_of(base, d, nfree)
    rank = np.cumsum(free, 1) - 1  # rank of a free cell among the free ones
    hit = free & (rank == r[:, None])
    assert (hit.sum(1) == 1).all()
    return L[hit.argmax(1)]


def draw(agent_ok: np.ndarray, item_ok: np.ndarray, n_items: int, B: int, env_offset: int, seed: int, rnd: int):
    """(agent cells [A, B], item cells [n_items, B]) of envs env_offset .. env_offset + B - 1."""
    base = base_of(B, env_offset, seed, rnd)
    A = agent_ok.shape[0]
    ag = np.zeros((A, B), np.int64)
    for i in range(A):
        ag[i] = _pick(np.nonzero(agent_ok[i])[0], ag[:i], i, base)
    LI = np.nonzero(item_ok)[0]
    it = np.zeros((n_items, B), np.int64)
    for k in range(n_items):
        it[k] = _pick(LI, it[:k], 16 + k, base)
    return ag, it


def template_state(level, A: int, pitch: int) -> np.ndarray:
    """[num_planes, pitch]: the level's own start in every column."""
    K, wide = capi.item_slots(level), capi.is_wide(level)
    P = capi.layout_planes(A, K, wide)
    s = np.zeros((P["num_planes"], pitch), np.uint8)
    for a in range(A):
        s[P["agent_x"] + a], s[P["agent_y"] + a], s[P["agent_hold"] + a] = level.spawns[a][0], level.spawns[a][1], 0xFF
    dead = 0xFFFF if wide else 0xFF
    for j in range(K):
        c, m = level.items[j] if j < len(level.items) else (dead, 0)
        s[P["item_loc"] + j], s[P["item_mask"] + j] = c & 0xFF, m
        if wide:
            s[P["item_loc_hi"] + j] = c >> 8
    return s


def expected(level, A: int, B: int, agent_ok, item_ok, env_offset: int, seed: int, rnd: int, what: int,
             draws=None) -> np.ndarray:
    """[num_planes, B]: the states oc_reset_random gives envs 0 .. B - 1, the two t planes as the
    counter's low and high bytes per env (oc_testlib.env_view's rows).  `draws`: draw()'s result
    for at least B envs, when the caller has it already (it does not depend on `what`)."""
    K, wide = capi.item_slots(level), capi.is_wide(level)
    P = capi.layout_planes(A, K, wide)
    s = template_state(level, A, B)
    ag, it = draws if draws is not None else draw(agent_ok, item_ok, len(level.items), B, env_offset, seed, rnd)
    ag, it = ag[:, :B], it[:, :B]
    if what & START_AGENTS:
        s[P["agent_x"]:P["agent_x"] + A] = ag % level.width
        s[P["agent_y"]:P["agent_y"] + A] = ag // level.width
    if what & START_ITEMS:
        n = len(level.items)
        s[P["item_loc"]:P["item_loc"] + n] = it & 0xFF
        if wide:
            s[P["item_loc_hi"]:P["item_loc_hi"] + n] = it >> 8
    return s


def env_byte_mask(A: int, K: int, wide: bool, pitch: int, B: int, lo: int = 0) -> np.ndarray:
    """bool [num_planes * pitch]: the bytes of a flat state buffer that belong to envs lo .. B - 1
    (the u16 t plane has env e at bytes 2e, 2e + 1 of its two planes)."""
    P = capi.layout_planes(A, K, wide)
    m = np.zeros((P["num_planes"], pitch), bool)
    m[:, lo:B] = True
    m[P["t"]:P["t"] + 2] = False
    m[P["t"]:P["t"] + 2].reshape(-1)[2 * lo:2 * B] = True
    return m.reshape(-1)


def scatter(state: np.ndarray, exp: np.ndarray, envs: np.ndarray, A: int, K: int, wide: bool, pitch: int) -> None:
    """Write columns `envs` of exp ([num_planes, B], expected()'s rows) into a flat state buffer."""
    P = capi.layout_planes(A, K, wide)
    s = state.reshape(P["num_planes"], pitch)
    T = P["t"]
    for p in list(range(T)) + [P["flags"]]:
        s[p, envs] = exp[p, envs]
    t = s[T:T + 2].reshape(-1)
    t[2 * envs], t[2 * envs + 1] = exp[T, envs], exp[T + 1, envs]


_ITEM_CHAR = {"FreshTomato": "t", "FreshLettuce": "l", "FreshOnion": "o", "Plate": "p"}
_TILE_CHAR = {levels.TILE_FLOOR: " ", levels.TILE_COUNTER: "-", levels.TILE_CUTBOARD: "/", levels.TILE_DELIVERY: "*"}


def variant_text(level, A: int, agent_cells, item_cells) -> str:
    """The level file of `level` with item k's letter on item_cells[k] and agent i's spawn line at
    agent_cells[i] (the first A spawn lines; the reference reads one agent per line)."""
    W = level.width
    grid = [_TILE_CHAR[t] for t in level.tiles]
    for (_, mask), c in zip(level.items, item_cells):
        (_, full), = levels.mask_contents(mask, level.encoding)
        assert grid[c] == "-", "item cell %d is not a bare Counter" % c
        grid[c] = _ITEM_CHAR[full]
    rows = ["".join(grid[y * W:(y + 1) * W]) for y in range(level.height)]
    spawns = ["%d %d" % (c % W, c // W) for c in agent_cells[:A]]
    return "\n".join(rows) + "\n\n" + "\n".join(level.recipes) + "\n\n" + "\n".join(spawns) + "\n"
