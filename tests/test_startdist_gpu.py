"""oc_reset_random on the GPU: byte for byte against its host twin oc_cpu_reset_random (which
tests/test_startdist.py pins to the numpy restatement and, through the variant level, to the
reference) in full and masked mode on every layout, with guard bytes around the state and past
the batch's last 4-env word; OvercookedVecEnv(random_starts=...) against a host loop of
CpuStepper.step + reset_random; and one hipGraph capture of oc_step + the masked call."""
import numpy as np
import pytest

import oc_testlib as tl
import start_ref as sr
from gym_cooking_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 0xA5
DONE = capi.OC_FLAG_DONE
CONFIGS = [("partial-divider_salad", 2), ("full-divider_tl", 3), ("full-divider_tl", 4),
           ("levels/many-13x12_full16.txt", 4), ("levels/dup-9x8_tomato2.txt", 2), ("levels/edge-7x6_salad.txt", 2),
           ("levels/wide-17x17_salad.txt", 4)]
SIZES = (5, 259, 4099, 65539)


def _id(cfg):
    return "%s-A%d" % (cfg[0].split("/")[-1].replace(".txt", ""), cfg[1])


def guarded(eb, host_state=None):
    """(raw, state): a state buffer with one guard plane before and after it, filled with the
    guard byte or with `host_state`."""
    P, n = eb.pitch, eb.layout.state_bytes
    raw = torch.full((n + 2 * P,), GUARD, dtype=torch.uint8, device=DEV)
    if host_state is not None:
        raw[P:P + n].copy_(torch.from_numpy(host_state))
    return raw, raw[P:P + n]


def check_guards(raw, eb):
    h = raw.cpu().numpy()
    P = eb.pitch
    assert (h[:P] == GUARD).all() and (h[-P:] == GUARD).all(), "bytes around the state written"
    return h[P:-P]


@pytest.mark.parametrize("config", CONFIGS, ids=_id)
def test_full_mode_equals_cpu_twin(config):
    from gym_cooking_amd.engine import CpuStepper, OvercookedBatch
    lv, A = tl.load_level(config[0]), config[1]
    wide = capi.is_wide(lv)
    for B in SIZES:
        eb = OvercookedBatch(lv, A, B, max_T=30, device=DEV)
        cs = CpuStepper(lv, A, B, max_T=30)
        lim = (B + 3) // 4 * 4
        past = ~sr.env_byte_mask(A, eb.K, wide, eb.pitch, lim)
        for what, seed, off in ((3, 5, 0), (1, 1 << 63, 1 << 33), (2, 7, 12345)):
            raw, s = guarded(eb)
            eb.reset_random(s, None, seed, 9, what, off)
            torch.cuda.synchronize()
            got = check_guards(raw, eb)
            want = cs.reset_random(cs.new_state(), None, seed, 9, what, off)
            assert np.array_equal(tl.env_view(got, A, eb.K, eb.pitch, B), tl.env_view(want, A, cs.K, cs.pitch, B)), \
                (B, what)
            assert (got[past] == GUARD).all(), "a byte at or past the next multiple of 4 above B was written"


@pytest.mark.parametrize("config", CONFIGS, ids=_id)
def test_masked_mode_equals_cpu_twin(config):
    """About 1 % and 100 % DONE envs and none: the whole buffer, untouched envs and everything past
    B included, equals the host twin's on the same bytes; in place too."""
    from gym_cooking_amd.engine import CpuStepper, OvercookedBatch
    lv, A = tl.load_level(config[0]), config[1]
    for B in SIZES:
        eb = OvercookedBatch(lv, A, B, max_T=30, device=DEV)
        cs = CpuStepper(lv, A, B, max_T=30)
        P, NP, fl = eb.pitch, eb.layout.num_planes, eb.layout.plane_flags
        rng = np.random.default_rng(B)
        for frac in (0.01, 1.0, 0.0):
            before = rng.integers(0, 256, NP * P, dtype=np.uint8)
            prev = rng.integers(0, 256, NP * P, dtype=np.uint8)
            pf = prev.reshape(NP, P)[fl]
            pf[:] = (pf & ~np.uint8(DONE)) | (rng.random(P) < frac)
            if frac == 0.01:
                pf[B - 1] |= DONE  # the batch's last env, in a ragged word
            pf[B:] |= DONE  # DONE past B: not envs of the batch
            raw, s = guarded(eb, before)
            dprev = torch.from_numpy(prev).to(DEV)
            eb.reset_random(s, dprev, 21, 4, 3, 77)
            torch.cuda.synchronize()
            got = check_guards(raw, eb)
            want = cs.reset_random(before.copy(), prev, 21, 4, 3, 77)
            assert (frac == 0.0) == np.array_equal(want, before)
            assert np.array_equal(got, want), (B, frac, np.argwhere(got != want)[:5].tolist())
            raw, s = guarded(eb, prev)  # state_prev == state
            eb.reset_random(s, s, 21, 4, 3, 77)
            torch.cuda.synchronize()
            want = prev.copy()
            cs.reset_random(want, want, 21, 4, 3, 77)
            assert np.array_equal(check_guards(raw, eb), want), (B, frac, "in place")


def test_set_start_cells_on_device_handle():
    from gym_cooking_amd.engine import CpuStepper, OvercookedBatch
    lv, A, B = tl.load_level("levels/many-13x12_full16.txt"), 4, 4099
    agent_ok, item_ok = sr.default_masks(lv, A)
    tight = np.zeros_like(item_ok)
    tight[np.nonzero(item_ok)[0][:16]] = 1
    shared = np.zeros_like(agent_ok)
    shared[:, np.nonzero(agent_ok[0])[0][:4]] = 1
    eb, cs = OvercookedBatch(lv, A, B, device=DEV), CpuStepper(lv, A, B)
    for o in (eb, cs):
        o.set_start_cells(shared, tight)
    a, i = eb.start_cells()
    assert np.array_equal(a, shared) and np.array_equal(i, tight)
    raw, s = guarded(eb)
    eb.reset_random(s, None, 3, 0, 3, 0)
    torch.cuda.synchronize()
    want = cs.reset_random(cs.new_state(), None, 3, 0, 3, 0)
    assert np.array_equal(tl.env_view(check_guards(raw, eb), A, eb.K, eb.pitch, B), tl.env_view(want, A, cs.K, cs.pitch, B))
    with pytest.raises(RuntimeError, match="what = 0"):
        eb.reset_random(s, None, 3, 0, 0, 0)
    with pytest.raises(RuntimeError, match="bad argument"):
        eb.reset_random(s, None, 3, 0, 3, -1)


def test_vec_env_random_starts_equals_host_loop():
    """300 steps at B = 4,099 with random starts == CpuStepper.step + reset_random on the host."""
    from gym_cooking_amd.engine import CpuStepper
    from gym_cooking_amd.envs import OvercookedVecEnv
    B, A, seed = 4099, 2, 123
    env = OvercookedVecEnv("partial-divider_salad", A, B, max_num_timesteps=30, device=DEV, random_starts=3, seed=seed)
    cs = CpuStepper("partial-divider_salad", A, B, max_T=30)
    P = cs.pitch
    h, h2 = cs.new_state(), cs.new_state()
    cs.reset_random(h, None, seed, 0, 3)
    assert np.array_equal(tl.env_view(env.reset().cpu().numpy(), A, cs.K, P, B), tl.env_view(h, A, cs.K, P, B))
    assert not np.array_equal(h, cs.new_state())
    gen = torch.Generator(device="cpu").manual_seed(1)
    act = np.full((A, P), 4, np.uint8)
    restarts = 0
    for t in range(300):
        a = torch.randint(0, 5, (A, B), dtype=torch.uint8, generator=gen)
        state, _, _, _ = env.step(a.to(DEV))
        act[:, :B] = a.numpy()
        cs.step(h, h2, act.reshape(-1))
        cs.reset_random(h2, h, seed, t + 1, 3)
        restarts += int((h.reshape(-1, P)[cs.layout.plane_flags, :B] & DONE).sum())
        h, h2 = h2, h
        if t % 10 == 9 or t < 3:
            assert np.array_equal(tl.env_view(state.cpu().numpy(), A, cs.K, P, B), tl.env_view(h, A, cs.K, P, B)), t
    assert restarts > 5 * B


def test_vec_env_default_is_unchanged():
    """random_starts = 0 (the default): state for state what the batch's reset and step give."""
    from gym_cooking_amd.engine import OvercookedBatch
    from gym_cooking_amd.envs import OvercookedVecEnv
    B, A = 4099, 2
    env = OvercookedVecEnv("partial-divider_salad", A, B, max_num_timesteps=20, device=DEV)
    assert env.random_starts == 0
    eb = OvercookedBatch("partial-divider_salad", A, B, max_T=20, device=DEV)
    s, s2, act = eb.new_state(), eb.new_state(), eb.new_actions()
    s.zero_()
    s2.zero_()
    eb.reset(s)
    assert torch.equal(env.reset().view(-1, eb.pitch)[:, :B], s.view(-1, eb.pitch)[:, :B])
    for t in range(50):
        eb.gen_actions(act, t, seed=4)
        eb.step(s, s2, act)
        s, s2 = s2, s
        state, _, _, _ = env.step(act.view(A, eb.pitch))
        assert torch.equal(state.view(-1, eb.pitch)[:, :B], s.view(-1, eb.pitch)[:, :B]), t


def test_hipgraph_capture_of_step_and_masked_restart():
    """One capture of oc_step + masked oc_reset_random replays to the bytes of the direct calls."""
    from gym_cooking_amd.engine import OvercookedBatch
    lv, A, B = tl.load_level("partial-divider_salad"), 2, 4099
    eb = OvercookedBatch(lv, A, B, max_T=6, device=DEV)
    start, act = eb.new_state(), eb.new_actions()
    start.zero_()
    eb.reset_random(start, None, 8, 0, 3)
    s = start.clone()
    for t in range(6):  # to the time-out: every env is DONE in `s`
        eb.gen_actions(act, t, seed=2)
        eb.step(s, s, act)
    assert bool((eb.planes(s)["flags"][:B] & DONE).all())
    eb.gen_actions(act, 6, seed=2)
    direct = torch.zeros_like(s)
    eb.step(s, direct, act)
    eb.reset_random(direct, s, 8, 7, 3)
    torch.cuda.synchronize()
    out = torch.zeros_like(s)
    graph, cap = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=DEV)
    cap.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.graph(graph, stream=cap):
        eb.step(s, out, act)
        eb.reset_random(out, s, 8, 7, 3)
    torch.cuda.synchronize()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, direct)
    tmpl = torch.zeros_like(s)
    eb.step(s, tmpl, act)  # without the masked call: the template everywhere
    torch.cuda.synchronize()
    assert not torch.equal(tmpl, direct)
