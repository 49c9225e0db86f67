#!/usr/bin/env python3
"""Generate the subtask-progress fixture (oc_progress: per-subtask object counts and completion
events) from the reference's own RealAgent.def_subtask_completion / is_subtask_complete
(gym_cooking/utils/agent.py:286-368).

The committed action streams of the five episode fixtures (streams, duplevels, manylevels,
widelevels, edgelevels .npz: `act`, `ep_*`) are replayed through the reference's
OvercookedEnvironment; every replayed state is asserted equal to the committed canonical record,
which guards the replay.  For every transition (env_{t-1}, env_t) and every subtask of the
reference's own env.all_subtasks a reference RealAgent gets `new_subtask`, runs
def_subtask_completion(env_{t-1}) (its cur_obj_count is recorded), then, after the step,
is_subtask_complete(env_t.world) is recorded, and a second def_subtask_completion(env_t) gives the
count at env_t.  The subtasks are recorded as their printed names ("Chop(Tomato)"); the tests map
them to masks through recipes.subtask_masks.  Transitions whose step raised in the reference (ERR)
are left out (only the flag is defined there).

Kept: every transition on which some subtask completes, and of the others every STRIDE-th per
(fixture, level, A) group, counted in replay order: an index rule, no RNG.  The coverage table
printed at the end is asserted non-empty class by class.

Runs ONLY in the build container (the reference is imported with gen_golden.py's stubs).
progress.npz is written with fixed zip timestamps, so a rerun is byte-identical.
Usage:  PYTHONHASHSEED=0 python tests/golden/gen_progress.py [output path]
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_duplevels as gd  # noqa: E402
import gen_edgelevels as ge  # noqa: E402
import gen_golden as gg  # noqa: E402
import gen_manylevels as gm  # noqa: E402
from gen_obs import FIXTURES, canon16, encoding_of, write_npz  # noqa: E402

STRIDE = 24
SMAX = 64  # subtask columns of the per-transition arrays: OC_MAX_SUBTASKS (PAD past a group's subtasks)
CLASSES = ["chop_event", "merge_event", "deliver_event", "count_ge_2", "deliver_event_on_success",
           "two_equal_objects_one_square", "wide_level", "slots_16", "no_event"]


def make_agents(env, args):
    """One reference RealAgent per subtask of env.all_subtasks, its new_subtask set."""
    from utils.agent import COLORS, RealAgent
    agents = []
    with contextlib.redirect_stdout(io.StringIO()):
        for st in env.all_subtasks:
            ag = RealAgent(arglist=args, name="agent-1", id_color=COLORS[0], recipes=[])
            ag.new_subtask = st
            agents.append(ag)
    return agents


def equal_objects_on_a_square(env) -> bool:
    from utils.core import Object
    seen = set()
    for objs in env.world.objects.values():
        for o in objs:
            if isinstance(o, Object):
                key = (o.full_name, o.location)
                if key in seen:
                    return True
                seen.add(key)
    return False


KEYS = ("group", "p_t", "p_flags", "p_agents", "p_items", "c_t", "c_flags", "c_agents", "c_items",
        "cnt_prev", "cnt_cur", "done")


def replay(name):
    """One episode fixture: (groups, subtask names per group, rows, classes seen, kept, states)."""
    ref = gg.load_reference()
    presence_mask = gg.content_mask
    with np.load(os.path.join(HERE, name + ".npz")) as z:
        F = {k: z[k] for k in z.files}
    scratch = tempfile.mkdtemp(prefix="oc_progress_")
    os.makedirs(os.path.join(scratch, "utils", "levels"))
    for f in sorted(os.listdir(os.path.join(HERE, "levels"))):
        shutil.copy(os.path.join(HERE, "levels", f), os.path.join(scratch, "utils", "levels"))
    if name != "streams":  # the builtin levels load relative to the reference's own directory
        os.chdir(scratch)

    groups, names_of, others = [], {}, {}
    rows = {k: [] for k in KEYS}
    seen = {c: 0 for c in CLASSES}
    kept = {c: 0 for c in CLASSES}
    replayed = 0
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
            others[key] = 0
        g = groups.index(key)
        assert (F["ep_start"][e] == gg.PAD).all()
        env = Env(ref, level, A, int(F["ep_maxT"][e]))
        args = argparse.Namespace(beta=1.3, alpha=0.01, tau=2, cap=75, main_cap=100, **vars(env.args))
        subs = [str(st) for st in env.env.all_subtasks]
        assert names_of.setdefault(g, subs) == subs and 0 < len(subs) <= SMAX, (key, subs)
        # all_subtasks repeats a subtask once per recipe that needs it: one agent per distinct
        # subtask, its results copied to every column of that name
        agents = make_agents(env.env, args)
        first = {}
        for i, n in enumerate(subs):
            first.setdefault(n, i)
        uniq = sorted(first.values())
        col = [uniq.index(first[n]) for n in subs]
        agents = [agents[i] for i in uniq]
        kinds = [type(agents[c].new_subtask).__name__ for c in col]
        w = env.env.world
        wide, slots16 = w.width * w.height > 255, F["items"].shape[1] == 16 and \
            sum(1 for r in F["items"][int(F["ep_state_off"][e])] if r[0] != gg.PAD) > 8
        s0, a0, T = int(F["ep_state_off"][e]), int(F["ep_act_off"][e]), int(F["ep_T"][e])
        st = env.canon(0)
        cnt_cur = None  # the counts def_subtask_completion left at the current state, when it ran there
        for i in range(T + 1):
            prev = st
            if i > 0:
                if cnt_cur is None:
                    for ag in agents:
                        ag.def_subtask_completion(env.env)
                    cnt_cur = [int(ag.cur_obj_count) for ag in agents]
                cnt_prev = cnt_cur  # env_t's second def_subtask_completion is env_t+1's first
                st, _, _ = env.step([int(c) for c in F["act"][a0 + i - 1][:A]])
            o = s0 + i
            assert int(st["t"]) == int(F["t"][o]) and int(st["flags"]) == int(F["flags"][o]), (name, e, i)
            assert np.array_equal(st["agents"], F["agents"][o]) and np.array_equal(st["items"], F["items"][o]), \
                (name, e, i)
            replayed += 1
            if i == 0:
                continue
            if st["flags"] & 4:
                cnt_cur = None
                continue
            assert not prev["flags"] & 1, "a transition out of a DONE state"
            done = [bool(ag.is_subtask_complete(env.env.world)) for ag in agents]
            for ag in agents:
                ag.def_subtask_completion(env.env)
            cnt_cur = [int(ag.cur_obj_count) for ag in agents]
            assert done == [c > p for c, p in zip(cnt_cur, cnt_prev)]
            done_all, prev_all, cur_all = ([v[c] for c in col] for v in (done, cnt_prev, cnt_cur))
            cls = set()
            for k, d in zip(kinds, done_all):
                if d:
                    cls.add({"Chop": "chop_event", "Merge": "merge_event", "Deliver": "deliver_event"}[k])
                    if k == "Deliver" and st["flags"] & 2:
                        cls.add("deliver_event_on_success")
            if max(cur_all) >= 2:
                cls.add("count_ge_2")
            if equal_objects_on_a_square(env.env):
                cls.add("two_equal_objects_one_square")
            if wide:
                cls.add("wide_level")
            if slots16:
                cls.add("slots_16")
            if not any(done_all):
                cls.add("no_event")
            for c in cls:
                seen[c] += 1
            if not any(done_all):
                others[key] += 1
                if (others[key] - 1) % STRIDE != 0:
                    continue
            for c in cls:
                kept[c] += 1
            pad = [gg.PAD] * (SMAX - len(subs))
            rows["group"].append(g)
            for pre, s in (("p_", prev), ("c_", st)):
                rows[pre + "t"].append(int(s["t"]))
                rows[pre + "flags"].append(int(s["flags"]))
                rows[pre + "agents"].append(s["agents"].copy())
                rows[pre + "items"].append(canon16(s))
            rows["cnt_prev"].append(prev_all + pad)
            rows["cnt_cur"].append(cur_all + pad)
            rows["done"].append([int(d) for d in done_all] + pad)
    os.chdir(HERE)
    shutil.rmtree(scratch)
    return groups, names_of, rows, seen, kept, replayed, len(F["ep_T"])


def main():
    # one process per episode fixture (the reference is loaded in each), merged in FIXTURES order
    import multiprocessing as mp
    with mp.get_context("fork").Pool(len(FIXTURES)) as pool:
        parts = pool.map(replay, FIXTURES)
    groups, names_of = [], {}
    rows = {k: [] for k in KEYS}
    seen = {c: 0 for c in CLASSES}
    kept = {c: 0 for c in CLASSES}
    replayed = episodes = 0
    for gs, names, r, sn, kp, n, ne in parts:
        base = len(groups)
        groups += gs
        for g, v in names.items():
            names_of[base + g] = v
        for k in KEYS:
            rows[k] += [base + g for g in r[k]] if k == "group" else r[k]
        for c in CLASSES:
            seen[c] += sn[c]
            kept[c] += kp[c]
        replayed += n
        episodes += ne

    group = np.array(rows["group"], np.int32)
    arrays = dict(
        grp_fixture=np.array([g[0] for g in groups]), grp_level=np.array([g[1] for g in groups]),
        grp_A=np.array([g[2] for g in groups], np.int32),
        grp_counts=np.array([encoding_of(g[0], os.path.splitext(os.path.basename(g[1]))[0]) == "counts"
                             for g in groups], np.uint8),
        grp_subtasks=np.array([";".join(names_of[g]) for g in range(len(groups))]),
        tr_group=group,
        tr_cnt_prev=np.array(rows["cnt_prev"], np.uint8), tr_cnt_cur=np.array(rows["cnt_cur"], np.uint8),
        tr_done=np.array(rows["done"], np.uint8))
    for pre in ("p_", "c_"):
        arrays[pre + "t"] = np.array(rows[pre + "t"], np.uint16)
        arrays[pre + "flags"] = np.array(rows[pre + "flags"], np.uint8)
        arrays[pre + "agents"] = np.stack(rows[pre + "agents"]).astype(np.uint8)
        arrays[pre + "items"] = np.stack(rows[pre + "items"]).astype(np.uint8)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "progress.npz")
    write_npz(out, arrays)

    print("replayed %d states of %d episodes; kept %d transitions in %d groups; progress.npz %d bytes" % (
        replayed, episodes, len(group), len(groups), os.path.getsize(out)))
    print("%-12s %-32s %2s %6s  %s" % ("fixture", "level", "A", "kept", "subtasks"))
    for g, (f, lvl, A) in enumerate(groups):
        print("%-12s %-32s %2d %6d  %s" % (f, lvl, A, int((group == g).sum()), ";".join(names_of[g])))
    print("%-30s %8s %8s" % ("coverage class", "seen", "kept"))
    for c in CLASSES:
        print("%-30s %8d %8d" % (c, seen[c], kept[c]))
        assert kept[c] > 0, "no kept transition of class " + c
    assert os.path.getsize(out) <= 512 * 1024, "progress.npz over 512 KB"


if __name__ == "__main__":
    main()
