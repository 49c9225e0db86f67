"""Every cell of the engine's (A, K, narrow / wide) dispatch grid on the GPU: the 24 cells and
levels of tests/test_dispatch_grid.py at B = 7, each kernel entry point against its host twin on
the same bytes.  Per cell: oc_reset against the host template; six oc_step launches, and the same
six steps as one oc_step_n launch with a trajectory, as one without executed-action and collision
buffers whose state_out is the trajectory's last slot and as one without a trajectory, against
oc_cpu_step; oc_state_checksum against its numpy twin; oc_observe (u8 and f16, with masks) against
oc_cpu_observe; oc_progress against oc_cpu_progress."""
import numpy as np
import pytest

import oc_testlib as tl
from gym_cooking_amd import capi
from test_dispatch_grid import B, CELLS, MAX_T, grid_level, oracle_play, subtask_rows

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 6


def host_steps(cs, s0, acts):
    """N oc_cpu_step steps from s0: per step the state, the executed actions and the collision mask
    (whole buffers), and the totals."""
    A, P = cs.A, cs.pitch
    states, exs, colls, tot = [], [], [], np.zeros(capi.OC_NSTATS, np.uint64)
    s = s0
    for t in range(N):
        nxt, ex, coll = np.zeros_like(s0), np.zeros(A * P, np.uint8), np.zeros(P, np.uint8)
        cs.step(s, nxt, acts[t], ex, coll, tot)
        states.append(nxt)
        exs.append(ex.reshape(A, P)[:, :B])
        colls.append(coll[:B])
        s = nxt
    return states, exs, colls, tot.astype(np.int64)


@pytest.mark.parametrize("A,K,shape", CELLS)
def test_cell_kernels_match_host(A, K, shape):
    from gym_cooking_amd.engine import CpuStepper, OvercookedBatch
    lv = grid_level(K, shape)
    eb = OvercookedBatch(lv, A, B, MAX_T, device=DEV)
    cs = CpuStepper(lv, A, B, MAX_T)
    P, nb = eb.pitch, eb.layout.state_bytes
    assert (eb.K, P, nb) == (K, cs.pitch, cs.layout.state_bytes)
    view = lambda s: tl.env_view(s, A, K, P, B)  # noqa: E731

    s0 = eb.reset(eb.new_state())
    h0 = s0.cpu().numpy()
    assert np.array_equal(view(h0), view(cs.new_state()))

    acts = oracle_play(A, K, shape).acts[:N]
    want_s, want_ex, want_coll, want_tot = host_steps(cs, h0, acts)
    dacts = torch.from_numpy(np.stack(acts)).to(DEV)  # [N, A * P]

    # N oc_step launches, ping-pong
    s, nxt, ex, coll, stats = s0.clone(), eb.new_state(), eb.new_exec(), eb.new_coll(), eb.new_stats()
    for t in range(N):
        eb.step(s, nxt, dacts[t], ex, coll, stats)
        s, nxt = nxt, s
        assert np.array_equal(view(s.cpu().numpy()), view(want_s[t])), t
        assert np.array_equal(ex.cpu().numpy().reshape(A, P)[:, :B], want_ex[t]), t
        assert np.array_equal(coll.cpu().numpy()[:B], want_coll[t]), t
    assert np.array_equal(eb.reduce_stats(stats).cpu().numpy(), want_tot)

    # the same steps as one oc_step_n launch with a trajectory
    out, traj = eb.new_state(), torch.empty(N * nb, dtype=torch.uint8, device=DEV)
    exn = torch.empty(N * A * P, dtype=torch.uint8, device=DEV)
    colln = torch.empty(N * P, dtype=torch.uint8, device=DEV)
    totals = torch.zeros(capi.OC_NSTATS, dtype=torch.int64, device=DEV)
    eb.step_n(s0, out, dacts.reshape(-1), N, traj, exn, colln, eb.new_stats(), totals)
    ht = traj.cpu().numpy()
    for t in range(N):
        assert np.array_equal(view(ht[t * nb:(t + 1) * nb]), view(want_s[t])), t
    assert np.array_equal(view(out.cpu().numpy()), view(want_s[-1]))
    assert np.array_equal(exn.cpu().numpy().reshape(N, A, P)[:, :, :B], np.stack(want_ex))
    assert np.array_equal(colln.cpu().numpy().reshape(N, P)[:, :B], np.stack(want_coll))
    assert np.array_equal(totals.cpu().numpy(), want_tot)

    # absent outputs: no executed-action and no collision buffer, state_out the trajectory's last slot
    # (the launch writes it once, as that slot); then no trajectory at all.  This pins the zero-record
    # descriptors of each layout's own kernel (oc_step_n_kernel, oc_step_wide_kernel)
    traj2 = torch.empty(N * nb, dtype=torch.uint8, device=DEV)
    tot2 = torch.zeros(capi.OC_NSTATS, dtype=torch.int64, device=DEV)
    eb.step_n(s0, traj2[(N - 1) * nb:], dacts.reshape(-1), N, traj2, None, None, eb.new_stats(), tot2)
    ht2 = traj2.cpu().numpy()
    for t in range(N):
        assert np.array_equal(view(ht2[t * nb:(t + 1) * nb]), view(want_s[t])), t
    assert np.array_equal(tot2.cpu().numpy(), want_tot)
    out3 = eb.new_state()
    tot3 = torch.zeros(capi.OC_NSTATS, dtype=torch.int64, device=DEV)
    eb.step_n(s0, out3, dacts.reshape(-1), N, None, None, None, eb.new_stats(), tot3)
    assert np.array_equal(view(out3.cpu().numpy()), view(want_s[-1]))
    assert np.array_equal(tot3.cpu().numpy(), want_tot)

    got = int(eb.checksum(out).cpu().numpy().view(np.uint64)[0])
    assert got == tl.checksum(want_s[-1], A, K, P, B)

    hs = out.cpu().numpy()
    for dtype, npdt in ((torch.uint8, np.uint8), (torch.float16, np.float16)):
        obs, mask = eb.new_obs(dtype), eb.new_action_mask()
        eb.observe(out, obs, mask, view_agent=A - 1)
        want_obs, want_mask = cs.observe(hs, npdt, A - 1)
        assert np.array_equal(obs.cpu().numpy(), want_obs), dtype
        assert np.array_equal(mask.cpu().numpy().reshape(A, P)[:, :B], want_mask[:, :B]), dtype

    rows, _ = subtask_rows(lv)
    w = [0.5 + 0.25 * i for i in range(len(rows))]
    cnt, ev, rew = eb.progress(s0, traj, rows, w, N)
    want_c, want_e, want_r = cs.progress(h0, ht, rows, w, N)
    assert np.array_equal(cnt.cpu().numpy()[:, :, :B], want_c[:, :, :B]) and want_c.any()
    assert np.array_equal(ev.cpu().numpy()[:, :, :B], want_e[:, :, :B])
    assert np.array_equal(rew.cpu().numpy()[:, :B].view(np.uint32), want_r[:, :B].view(np.uint32))
