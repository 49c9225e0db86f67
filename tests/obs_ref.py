"""Numpy restatement of oc_observe over the engine's state layout: the checker for shapes the
observation fixture (tests/golden/obs.npz) does not hold.  Written from the definition in
include/oc_engine.h, not from the kernel, and pinned to the reference by tests/test_observe.py.

  obs[e][c][y][x], C = 10 + A: 0-2 Counter / Cutboard / Delivery squares; 3-8 Fresh / Chopped
    Tomato, Lettuce, Onion and 9 Plate: +1 per content of every live item at its cell (a held
    item's cell is its holder's); 10 + ((i - view) mod A): agent i.
  mask[a][e]: bit k iff World.NAV_ACTIONS[k] is in get_single_actions(env, agent a)
    (navigation_planner/utils.py:55-90), bit 4 always.
"""
from __future__ import annotations

import numpy as np

from gym_cooking_amd import capi

NAV = ((0, 1), (0, -1), (-1, 0), (1, 0))
ENC_COUNTS = 1


def _contents(mask: np.ndarray, counts: bool):
    """[7, ...] per-channel (3..9) content counts of item masks."""
    m = mask.astype(np.int64)
    out = np.zeros((7,) + m.shape, np.int64)
    for f in range(3):
        if counts:  # 2-bit counts; 0x80 marks a single fresh food, every other food is chopped
            n = (m >> (2 * f)) & 3
            fresh = (m & 0x80) != 0
            out[2 * f] = np.where(fresh, n, 0)
            out[2 * f + 1] = np.where(fresh, 0, n)
        else:       # presence bits 0-2, chopped bits 4-6
            has, ch = (m >> f) & 1, (m >> (4 + f)) & 1
            out[2 * f] = has & (1 - ch)
            out[2 * f + 1] = has & ch
    out[6] = ((m & 0x40) != 0) if counts else ((m & 0x08) != 0)
    return out


def _mergeable(a, b, counts: bool):
    u = a | b
    if counts:
        return ((a & b & 0x40) == 0) & ((u & 0x80) == 0)
    return ((a & b & 0x08) == 0) & (((u & 7) & ~(u >> 4)) == 0)


def observe(level, A: int, K: int, state_bytes: np.ndarray, pitch: int, B: int, view_agent: int = -1):
    """(obs u8 [B, 10 + A, H, W], mask u8 [A, B]) of the first B envs of a host state buffer."""
    W, H = level.width, level.height
    HW = W * H
    wide = capi.is_wide(level)
    P = capi.layout_planes(A, K, wide)
    s = state_bytes.reshape(-1, pitch)[:P["num_planes"], :B].astype(np.int64)
    ax, ay, ah = (s[P[k]:P[k] + A] for k in ("agent_x", "agent_y", "agent_hold"))
    il = s[P["item_loc"]:P["item_loc"] + K]
    if wide:
        il = il | (s[P["item_loc_hi"]:P["item_loc_hi"] + K] << 8)
    im = s[P["item_mask"]:P["item_mask"] + K]
    counts = level.encoding == ENC_COUNTS
    tiles = np.asarray(level.tiles, np.int64)
    C = 10 + A
    obs = np.zeros((B, C, HW), np.uint8)
    for cls in (1, 2, 3):
        obs[:, cls - 1, tiles == cls] = 1
    env = np.arange(B)
    cont = _contents(im, counts)  # [7, K, B]
    for j in range(K):
        live = il[j] < HW
        cell = np.where(live, il[j], 0)
        for c in range(7):  # one (env, channel, cell) per env and statement: no repeated index
            obs[env, 3 + c, cell] += np.where(live, cont[c, j], 0).astype(np.uint8)
    rot = max(view_agent, 0)
    for i in range(A):
        obs[env, 10 + (i - rot) % A, ay[i] * W + ax[i]] += 1
    mask = np.full((A, B), 16, np.uint8)
    for a in range(A):
        holding = ah[a] < K
        hm = np.where(holding, np.take_along_axis(im, np.minimum(ah[a], K - 1)[None], 0)[0], 0)
        for k, (dx, dy) in enumerate(NAV):
            nx = np.clip(ax[a] + dx, 0, W - 1)  # World.inbounds
            ny = np.clip(ay[a] + dy, 0, H - 1)
            blocked = np.zeros(B, bool)
            for b in range(A):  # `new_loc not in agent_locs`: the agent's own square too
                blocked |= (ax[b] == nx) & (ay[b] == ny)
            c = ny * W + nx
            t = tiles[c]
            there = il == c[None]                     # [K, B]; a dead slot is no cell
            has = there.any(0)
            o = K - 1 - np.argmax(there[::-1], 0)     # the item on the square (one off Delivery)
            om = np.take_along_axis(im, o[None], 0)[0]
            item_ok = np.where(has, ~holding | _mergeable(hm, om, counts), holding)
            ok = ~blocked & ((t == 0) | (t == 3) | item_ok)
            mask[a] |= (ok.astype(np.uint8) << k)
    return obs.reshape(B, C, H, W), mask
