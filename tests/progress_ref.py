"""Numpy restatement of oc_progress over the engine's state layout: the checker for shapes the
progress fixture (tests/golden/progress.npz) does not hold.  Written from the definition in
include/oc_engine.h, not from the kernel, and pinned to the reference by tests/test_progress.py.

  count_i(s): Chop / Merge: the distinct cells of the live slots whose mask equals the goal mask
    (a held slot's cell is its holder's square); Deliver: the live slots, not held, of that mask
    on a Delivery square (a list: equal dishes on one square count twice); None: 0.
  event i of (prev, cur): prev not DONE and count_i(cur) > count_i(prev); bit i & 7 of plane i >> 3.
  reward: + weights[i] per set event, ascending i, f32 adds from +0.0.
"""
from __future__ import annotations

import numpy as np

from gym_cooking_amd import capi

SUB_NONE, SUB_CHOP, SUB_MERGE, SUB_DELIVER = 0, 1, 2, 3
FLAG_DONE = 1


def _planes(level, A: int, K: int, state: np.ndarray, pitch: int, B: int):
    wide = capi.is_wide(level)
    P = capi.layout_planes(A, K, wide)
    s = state.reshape(-1, pitch)[:P["num_planes"], :B].astype(np.int64)
    ax, ay, ah = (s[P[k]:P[k] + A] for k in ("agent_x", "agent_y", "agent_hold"))
    il = s[P["item_loc"]:P["item_loc"] + K]
    if wide:
        il = il | (s[P["item_loc_hi"]:P["item_loc_hi"] + K] << 8)
    return ax, ay, ah, il, s[P["item_mask"]:P["item_mask"] + K], s[P["flags"]], 0xFFFF if wide else 0xFF


def counts(level, A: int, K: int, state: np.ndarray, pitch: int, B: int, subs) -> np.ndarray:
    """u8 [S, B]: count_i of the first B envs of a host state buffer; subs = [(kind, goal mask)]."""
    ax, ay, ah, il, im, _, dead = _planes(level, A, K, state, pitch, B)
    W = level.width
    tiles = np.asarray(level.tiles, np.int64)
    live = il != dead
    held = np.zeros((K, B), bool)
    cell = il.copy()
    for a in reversed(range(A)):  # the lowest holder wins
        mine = ah[a][None] == np.arange(K)[:, None]
        held |= mine
        cell = np.where(mine, (ay[a] * W + ax[a])[None], cell)
    on_delivery = tiles[np.where(live & (il < len(tiles)), il, 0)] == 3
    out = np.zeros((len(subs), B), np.uint8)
    for i, (kind, goal) in enumerate(subs):
        sel = live & (im == goal)
        if kind == SUB_DELIVER:
            out[i] = (sel & ~held & on_delivery).sum(0)
        elif kind in (SUB_CHOP, SUB_MERGE):
            c = np.sort(np.where(sel, cell, -1), axis=0)  # the distinct cells of the selected slots
            first = np.concatenate([np.ones((1, B), bool), c[1:] != c[:-1]], 0)
            out[i] = ((c >= 0) & first).sum(0)
        else:
            assert kind == SUB_NONE
    return out


def progress(level, A: int, K: int, state_prev: np.ndarray, states: np.ndarray, pitch: int, B: int, subs,
             weights=None, n: int = 1):
    """(counts u8 [n, S, B], events u8 [n, planes, B], reward f32 [n, B])."""
    S = len(subs)
    nb = capi.layout_planes(A, K, capi.is_wide(level))["num_planes"] * pitch
    w = np.ones(S, np.float32) if weights is None else np.asarray(weights, np.float32)
    cnt = np.zeros((n, S, B), np.uint8)
    ev = np.zeros((n, (S + 7) // 8, B), np.uint8)
    rew = np.zeros((n, B), np.float32)
    prev = state_prev
    for r in range(n):
        cur = states[r * nb:(r + 1) * nb]
        cp, cc = counts(level, A, K, prev, pitch, B, subs), counts(level, A, K, cur, pitch, B, subs)
        was_done = (_planes(level, A, K, prev, pitch, B)[5] & FLAG_DONE) != 0
        cnt[r] = cc
        for i in range(S):
            hit = (cc[i] > cp[i]) & ~was_done
            ev[r, i >> 3] |= hit.astype(np.uint8) << (i & 7)
            rew[r] = np.where(hit, rew[r] + w[i], rew[r])  # f32 + f32, in ascending i
        prev = cur
    return cnt, ev, rew
