"""Device twins of the host calls in tests/taskselect_ref.py, tests/teamselect_ref.py and
tests/belief_ref.py, shared by the GPU tests: oc_task_select, oc_team_select and oc_belief_update on
guard-filled device buffers with numpy in and out, and the comparison of a device call with the
host call on the same bytes."""
import numpy as np
import torch

import belief_ref as br
import taskselect_ref as tr
import teamselect_ref as mr


class TaskDev:
    """oc_task_select on guard-filled device buffers, numpy in and out (as taskselect_ref.host_call)."""

    def __init__(self, level, A, B):
        from gym_cooking_amd.engine import OvercookedBatch
        self.eb = OvercookedBatch(level, A, B, max_T=100, device="cuda:0")

    def call(self, s, prev, rows, agents, flags, ts, want_bound=True, want_info=True):
        M, P = len(agents), self.eb.pitch
        dts = torch.from_numpy(ts).cuda()
        bound = torch.full((M, P), float("nan"), dtype=torch.float32, device="cuda:0") if want_bound else None
        info = torch.full((M, P), tr.GUARD_INFO, dtype=torch.uint8, device="cuda:0") if want_info else None
        launch = self.eb.task_select_launcher(torch.from_numpy(s).cuda(), rows, agents, dts,
                                              None if prev is None else torch.from_numpy(prev).cuda(), flags, bound, info)
        launch()
        torch.cuda.synchronize()
        return (dts.cpu().numpy(), None if bound is None else bound.cpu().numpy(),
                None if info is None else info.cpu().numpy())


def task_assert_same(dev, host):
    """Byte-equal, the guard columns (0xC3 task state, NaN bound, 0xA5 info) included."""
    for d, h in zip(dev, host):
        assert (d is None) == (h is None)
        if d is not None:
            assert np.array_equal(d.view(np.uint8), h.view(np.uint8)), np.argwhere(d.view(np.uint8) != h.view(np.uint8))[:5]


class TeamDev:
    """oc_team_select on guard-filled device buffers, numpy in and out (as teamselect_ref.host_call)."""

    def __init__(self, level, A, B):
        from gym_cooking_amd.engine import OvercookedBatch
        self.eb = OvercookedBatch(level, A, B, max_T=100, device="cuda:0")

    def call(self, s, prev, rows, pair, flags, ts, want_bound=True, want_info=True, times=1):
        P = self.eb.pitch
        dts = torch.from_numpy(ts).cuda()
        bound = torch.full((2, P), float("nan"), dtype=torch.float32, device="cuda:0") if want_bound else None
        info = torch.full((P,), mr.GUARD_INFO, dtype=torch.uint8, device="cuda:0") if want_info else None
        launch = self.eb.team_select_launcher(torch.from_numpy(s).cuda(), rows, pair, dts,
                                              None if prev is None else torch.from_numpy(prev).cuda(), flags, bound, info)
        for _ in range(times):
            launch()
        torch.cuda.synchronize()
        return (dts.cpu().numpy(), None if bound is None else bound.cpu().numpy(),
                None if info is None else info.cpu().numpy())


class BeliefDev:
    """oc_belief_update on guard-filled device buffers, numpy in and out (as belief_ref.host_call)."""

    def __init__(self, level, A, B):
        from gym_cooking_amd.engine import OvercookedBatch
        self.eb = OvercookedBatch(level, A, B, max_T=100, device="cuda:0")

    def launcher(self, prev, taken, events, rows, agents, flags, bel, bs, want_map=True, want_info=True):
        M, P = len(agents), self.eb.pitch
        up = lambda a: None if a is None else torch.from_numpy(a).cuda()  # noqa: E731
        dbel, dbs = up(bel), up(bs)
        amap = torch.full((M, P), br.GUARD_MAP, dtype=torch.uint8, device="cuda:0") if want_map else None
        info = torch.full((M, P), br.GUARD_INFO, dtype=torch.uint8, device="cuda:0") if want_info else None
        launch = self.eb.belief_update_launcher(up(prev), up(taken), rows, agents, dbel, dbs, up(events), 1.3, 0.5, flags,
                                                amap, info)
        return launch, (dbel, dbs, amap, info)

    def call(self, *args, **kw):
        launch, out = self.launcher(*args, **kw)
        launch()
        torch.cuda.synchronize()
        return tuple(None if t is None else t.cpu().numpy() for t in out)


def belief_assert_same(dev, host, S, B, where=""):
    """bstate, info and the guard columns byte for byte, beliefs to 1e-12 (exp and fused
    multiply-adds differ in their last bits), map against the device's own beliefs."""
    dbel, dbs, dmap, dinfo = dev
    hbel, hbs, _, hinfo = host
    assert np.array_equal(dbs, hbs), (where, np.argwhere(dbs != hbs)[:5])
    if dinfo is not None:
        assert np.array_equal(dinfo, hinfo), (where, np.argwhere(dinfo != hinfo)[:5])
    err = np.abs(dbel[:, :, :B] - hbel[:, :, :B])
    assert (err <= br.RTOL * np.abs(hbel[:, :, :B])).all(), (where, err.max())
    assert np.array_equal(dbel[:, :, B:].view(np.uint64), hbel[:, :, B:].view(np.uint64)), where
    if dmap is not None:
        br.check_map(dbel, dbs, dmap, S, B, where)
        assert (dmap[:, B:] == br.GUARD_MAP).all(), where
