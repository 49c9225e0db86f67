#!/usr/bin/env python3
"""Generate the observation fixture (oc_observe: grid feature planes and legal-move masks per
env) from the reference itself.

The committed action streams of the five episode fixtures (streams, duplevels, manylevels,
widelevels, edgelevels .npz: `act`, `ep_*`) are replayed through the reference's
OvercookedEnvironment; every replayed state is asserted equal to the committed canonical record,
which guards the replay.  For a deterministic subsample of the states this records
  * the canonical record (t, flags, agents, items) as gen_golden.RefEnv.canon makes it (16 item
    rows, in the mask encoding of the state's fixture);
  * the observation planes [10 + A, H, W] u8, built directly from the reference objects:
      0, 1, 2   Counter, Cutboard, Delivery   GridSquare subclasses in world.objects (core.py:28-120)
      3 .. 8    Fresh/Chopped Tomato, Lettuce, Onion: +1 per content of that full_name of every
      9         Plate                           Object in world.objects at obj.location (core.py:130-305)
      10 + i    sim_agents[i].location
  * get_single_actions(env, agent) of every agent (navigation_planner/utils.py:55-90) as a bit
    mask: bit k = World.NAV_ACTIONS[k] is in the list, bit 4 = (0, 0).
States whose recorded flags carry ERR are left out (only the flag is defined there).

Kept: per (fixture, level, A) group every STRIDE-th state of each episode, and besides them the
first RARE_KEEP states of the whole run that show each coverage class (the table printed at the
end, asserted non-empty): an index rule, no RNG.

Runs ONLY in the build container (the reference is imported with gen_golden.py's stubs).
obs.npz is written with fixed zip timestamps, so a rerun is byte-identical.
Usage:  PYTHONHASHSEED=0 python tests/golden/gen_obs.py
"""
from __future__ import annotations

import io
import os
import shutil
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_duplevels as gd  # noqa: E402
import gen_edgelevels as ge  # noqa: E402
import gen_golden as gg  # noqa: E402
import gen_manylevels as gm  # noqa: E402

# fixture -> (mask encoding of a level name, RefEnv class); streams first (the builtin levels
# load relative to the reference's own directory, the committed ones from a scratch copy)
FIXTURES = ["streams", "duplevels", "manylevels", "widelevels", "edgelevels"]
STRIDE = {"streams": 38, "duplevels": 10, "manylevels": 10, "widelevels": 22, "edgelevels": 6}
RARE_KEEP = 6
MAXK = 16
CHANNEL = {"FreshTomato": 3, "ChoppedTomato": 4, "FreshLettuce": 5, "ChoppedLettuce": 6,
           "FreshOnion": 7, "ChoppedOnion": 8, "Plate": 9}
STATIC = {"Counter": 0, "Cutboard": 1, "Delivery": 2}
CLASSES = (["chan%d" % c for c in range(3, 10)] +
           ["two_in_one_object_counts", "two_objects_one_square", "agent_holding", "success"] +
           ["move%d_%s" % (k, v) for k in range(4) for v in ("legal", "refused")] +
           ["refused_other_agent", "refused_empty_counter", "refused_no_merge",
            "allowed_put_down", "allowed_pick_up", "allowed_merge", "allowed_delivery",
            "edge_clamped_refused"])


def encoding_of(fixture: str, name: str) -> str:
    if fixture == "duplevels":
        return "counts"
    if fixture == "manylevels":
        return gm.LEVELS[name]
    return "presence"


def observe(env, A):
    """(planes [10 + A, H, W] u8, masks [4] u8 (PAD past A), coverage classes) of a reference env."""
    from utils.core import Delivery, Object
    w = env.world
    obs = np.zeros((10 + A, w.height, w.width), np.uint8)
    cls = set()
    per_cell = {}
    for objs in w.objects.values():
        for o in objs:
            x, y = o.location
            if isinstance(o, Object):
                names = [c.full_name for c in o.contents]
                for n in names:
                    obs[CHANNEL[n], y, x] += 1
                    per_cell.setdefault((CHANNEL[n], x, y), set()).add(id(o))
                if len(set(names)) < len(names):
                    cls.add("two_in_one_object_counts")
            elif type(o).__name__ in STATIC:
                obs[STATIC[type(o).__name__], y, x] = 1
            else:
                assert type(o).__name__ == "Floor", type(o).__name__
    if any(len(v) >= 2 for v in per_cell.values()):
        cls.add("two_objects_one_square")
    for c in range(3, 10):
        if obs[c].any():
            cls.add("chan%d" % c)
    locs = [ag.location for ag in env.sim_agents]
    masks = np.full(4, gg.PAD, np.uint8)
    for i, ag in enumerate(env.sim_agents):
        x, y = ag.location
        obs[10 + i, y, x] = 1
        if obs[3:10, y, x].any():  # Floor holds no object of its own: some agent here holds one
            assert any(b.holding is not None for b in env.sim_agents if b.location == ag.location)
            if ag.holding is not None:
                cls.add("agent_holding")
        acts = gg_nav.get_single_actions(env, ag)
        m = 0
        for t in acts:
            m |= 1 << gg.CODE[tuple(t)]
        assert m & 16
        masks[i] = m
        for k in range(4):
            legal = bool(m >> k & 1)
            cls.add("move%d_%s" % (k, "legal" if legal else "refused"))
            raw = (x + gg.NAV[k][0], y + gg.NAV[k][1])
            new = w.inbounds(raw)
            others = [l for j, l in enumerate(locs) if j != i]
            if new in locs:
                assert not legal
                if new in others:
                    cls.add("refused_other_agent")
                elif raw != new:
                    cls.add("edge_clamped_refused")
                continue
            gs = w.get_gridsquare_at(new)
            if not gs.collidable:
                assert legal
            elif isinstance(gs, Delivery):
                assert legal
                cls.add("allowed_delivery")
            elif gs.holding is None:
                cls.add("allowed_put_down" if legal else "refused_empty_counter")
                assert legal == (ag.holding is not None)
            elif ag.holding is None:
                assert legal
                cls.add("allowed_pick_up")
            else:
                cls.add("allowed_merge" if legal else "refused_no_merge")
    return obs, masks, cls


def canon16(st):
    it = np.full((MAXK, 4), gg.PAD, np.uint8)
    it[:st["items"].shape[0]] = st["items"]
    return it


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (a rerun gives the same bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    global gg_nav
    ref = gg.load_reference()
    _, gg_nav, _ = ref
    presence_mask = gg.content_mask
    fx = {}
    for name in FIXTURES:
        with np.load(os.path.join(HERE, name + ".npz")) as z:
            fx[name] = {k: z[k] for k in z.files}
    scratch = tempfile.mkdtemp(prefix="oc_obs_")
    os.makedirs(os.path.join(scratch, "utils", "levels"))
    for f in sorted(os.listdir(os.path.join(HERE, "levels"))):
        shutil.copy(os.path.join(HERE, "levels", f), os.path.join(scratch, "utils", "levels"))

    groups = []            # (fixture, level name as the fixture stores it, A)
    rows = {k: [] for k in ("group", "t", "flags", "agents", "items", "mask")}
    obs_of = {}            # group -> list of planes
    rare = {c: 0 for c in CLASSES}
    seen = {c: 0 for c in CLASSES}
    replayed = 0
    for name in FIXTURES:
        F = fx[name]
        if name != "streams":
            os.chdir(scratch)
        gg.MAXK = F["items"].shape[1]
        Env = ge.EdgeRefEnv if name == "edgelevels" else gg.RefEnv
        order = sorted(range(len(F["ep_T"])), key=lambda e: (int(F["ep_level"][e]), int(F["ep_A"][e]), e))
        for e in order:
            stored = str(F["level_names"][F["ep_level"][e]])
            level = os.path.splitext(os.path.basename(stored))[0]
            A = int(F["ep_A"][e])
            counts = encoding_of(name, level) == "counts"
            gg.content_mask = gd.content_mask_counts if counts else presence_mask
            key = (name, stored, A)
            if key not in groups:
                groups.append(key)
                obs_of[len(groups) - 1] = []
            g = groups.index(key)
            assert (F["ep_start"][e] == gg.PAD).all()
            env = Env(ref, level, A, int(F["ep_maxT"][e]))
            s0, a0, T = int(F["ep_state_off"][e]), int(F["ep_act_off"][e]), int(F["ep_T"][e])
            st = env.canon(0)
            for i in range(T + 1):
                if i > 0:
                    st, _, _ = env.step([int(c) for c in F["act"][a0 + i - 1][:A]])
                o = s0 + i
                assert int(st["t"]) == int(F["t"][o]) and int(st["flags"]) == int(F["flags"][o]), (name, e, i)
                assert np.array_equal(st["agents"], F["agents"][o]) and np.array_equal(st["items"], F["items"][o]), \
                    (name, e, i)
                replayed += 1
                if st["flags"] & 4:
                    continue
                planes, masks, cls = observe(env.env, A)
                assert counts or "two_in_one_object_counts" not in cls
                if st["flags"] & 2:
                    cls.add("success")
                for c in cls:
                    seen[c] += 1
                new_rare = [c for c in sorted(cls) if rare[c] < RARE_KEEP]
                if i % STRIDE[name] != 0 and not new_rare:
                    continue
                for c in cls:
                    rare[c] += 1
                rows["group"].append(g)
                rows["t"].append(int(st["t"]))
                rows["flags"].append(int(st["flags"]))
                rows["agents"].append(st["agents"].copy())
                rows["items"].append(canon16(st))
                rows["mask"].append(masks)
                obs_of[g].append(planes)
    os.chdir(HERE)
    shutil.rmtree(scratch)

    group = np.array(rows["group"], np.int32)
    arrays = dict(
        grp_fixture=np.array([g[0] for g in groups]), grp_level=np.array([g[1] for g in groups]),
        grp_A=np.array([g[2] for g in groups], np.int32),
        grp_counts=np.array([encoding_of(g[0], os.path.splitext(os.path.basename(g[1]))[0]) == "counts"
                             for g in groups], np.uint8),
        st_group=group, st_t=np.array(rows["t"], np.uint16), st_flags=np.array(rows["flags"], np.uint8),
        st_agents=np.stack(rows["agents"]).astype(np.uint8), st_items=np.stack(rows["items"]).astype(np.uint8),
        st_mask=np.stack(rows["mask"]).astype(np.uint8))
    for g in range(len(groups)):
        arrays["obs_%02d" % g] = np.stack(obs_of[g]).astype(np.uint8)
    out = os.path.join(HERE, "obs.npz")
    write_npz(out, arrays)

    print("replayed %d states of %d episodes; kept %d in %d groups; obs.npz %d bytes" % (
        replayed, sum(len(fx[n]["ep_T"]) for n in FIXTURES), len(group), len(groups), os.path.getsize(out)))
    print("%-28s %-30s %2s %6s" % ("fixture", "level", "A", "states"))
    for g, (f, lvl, A) in enumerate(groups):
        n = int((group == g).sum())
        print("%-28s %-30s %2d %6d" % (f, lvl, A, n))
        assert n >= 20, (f, lvl, A, n)
    print("%-28s %8s %8s" % ("coverage class", "seen", "kept"))
    for c in CLASSES:
        print("%-28s %8d %8d" % (c, seen[c], rare[c]))
        assert rare[c] > 0, "no kept state of class " + c
    have = {(f, os.path.splitext(os.path.basename(lvl))[0]) for f, lvl, _ in groups}
    for f in FIXTURES:
        F = fx[f]
        for e in range(len(F["ep_T"])):
            assert (f, str(F["level_names"][F["ep_level"][e]]), int(F["ep_A"][e])) in groups
    assert ("manylevels", "many-13x12_full16") in have and ("manylevels", "many-12x11_onion2") in have
    assert {a for f, _, a in groups if f == "widelevels"} == {1, 2, 3, 4}
    assert os.path.getsize(out) <= 512 * 1024, "obs.npz over 512 KB"
    assert len(group) <= 6500


if __name__ == "__main__":
    main()
