"""oc_cpu_observe (grid feature planes + legal-move masks per env) on the host: pinned to the
reference through tests/golden/obs.npz (gen_obs.py: planes built from the reference's objects,
get_single_actions of every agent), and checked against the numpy restatement tests/obs_ref.py
on ragged batch sizes."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oc_testlib as tl
import obs_ref
from gym_cooking_amd import capi
from gym_cooking_amd.engine import CpuStepper

pytestmark = pytest.mark.skipif(not os.path.isfile(capi.LIB_PATH), reason="liboc_engine.so not built")


@functools.lru_cache(maxsize=None)
def fixture():
    return tl.load_fixture("obs.npz")


class Group:
    """One (fixture, level, A) group of obs.npz: its states in the engine layout, the reference's
    planes and masks."""

    def __init__(self, g: int):
        fx = fixture()
        sel = np.nonzero(fx["st_group"] == g)[0]
        self.name = "%s:%s:A%d" % (fx["grp_fixture"][g], fx["grp_level"][g], fx["grp_A"][g])
        self.level = tl.load_level(str(fx["grp_level"][g]))
        self.A = int(fx["grp_A"][g])
        self.K = capi.item_slots(self.level)
        self.B = len(sel)
        self.pitch = capi.pitch_for(self.B)
        assert (self.level.encoding == 1) == bool(fx["grp_counts"][g]), self.name
        self.state = tl.state_from_canonical(self.level, self.A, self.K, self.pitch, fx["st_agents"][sel],
                                             fx["st_items"][sel][:, :max(4, self.K)], fx["st_t"][sel])
        self.obs = fx["obs_%02d" % g]
        self.mask = fx["st_mask"][sel][:, :self.A].T  # [A, B]


@functools.lru_cache(maxsize=None)
def group(g: int) -> Group:
    return Group(g)


def num_groups() -> int:
    return len(fixture()["grp_A"])


def rotated(obs: np.ndarray, A: int, view: int) -> np.ndarray:
    """The planes with agent i at channel 10 + ((i - view) mod A)."""
    out = obs.copy()
    for i in range(A):
        out[:, 10 + (i - view) % A] = obs[:, 10 + i]
    return out


def test_fixture_groups():
    fx = fixture()
    n = num_groups()
    assert n == 59 and all((fx["st_group"] == g).sum() >= 20 for g in range(n))
    assert not (fx["st_flags"] & 4).any()
    for g in range(n):
        assert fx["obs_%02d" % g].shape[1] == 10 + fx["grp_A"][g]


def test_restatement_equals_fixture():
    for g in range(num_groups()):
        G = group(g)
        obs, mask = obs_ref.observe(G.level, G.A, G.K, G.state, G.pitch, G.B)
        assert np.array_equal(obs, G.obs), G.name
        assert np.array_equal(mask, G.mask), G.name
        for v in range(G.A):
            o, m = obs_ref.observe(G.level, G.A, G.K, G.state, G.pitch, G.B, view_agent=v)
            assert np.array_equal(o, rotated(G.obs, G.A, v)) and np.array_equal(m, G.mask), (G.name, v)


def test_cpu_observe_equals_fixture():
    for g in range(num_groups()):
        G = group(g)
        cs = CpuStepper(G.level, G.A, G.B)
        obs, mask = cs.observe(G.state)
        assert obs.dtype == np.uint8 and obs.shape == G.obs.shape
        assert np.array_equal(obs, G.obs), G.name
        assert mask.shape == (G.A, G.pitch) and np.array_equal(mask[:, :G.B], G.mask), G.name
        h, _ = cs.observe(G.state, dtype=np.float16, want_mask=False)
        assert h.dtype == np.float16 and np.array_equal(h.view(np.uint16), G.obs.astype(np.float16).view(np.uint16)), G.name
        v = G.A - 1
        o, m = cs.observe(G.state, view_agent=v)
        assert np.array_equal(o, rotated(G.obs, G.A, v)) and np.array_equal(m[:, :G.B], G.mask), G.name


def stepped_state(cs: CpuStepper, steps: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    s, s2 = cs.new_state(), np.empty(cs.layout.state_bytes, np.uint8)
    for _ in range(steps):
        act = rng.integers(0, 5, cs.A * cs.pitch, dtype=np.uint8)
        cs.step(s, s2, act)
        s, s2 = s2, s
    return s


def raw_observe(cs, state, obs, mask, dtype, view=-1):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return cs.lib.oc_cpu_observe(cs._h, state.ctypes.data, p(obs), p(mask), dtype, view, cs.B, cs.nthreads)


HALF_BITS = np.arange(256).astype(np.float16).view(np.uint16)  # the half of every count a plane can hold


@pytest.mark.parametrize("level,A", [("partial-divider_salad", 2), ("levels/wide-17x17_salad.txt", 2)])
@pytest.mark.parametrize("B", [1, 3, 4097, 70001])
def test_ragged_sizes_against_restatement(level, A, B):
    lv = tl.load_level(level)
    cs = CpuStepper(lv, A, B, nthreads=4)
    state = stepped_state(cs, 200 if B < 70001 else 60, seed=B)
    n = B * capi.obs_channels(A) * lv.width * lv.height
    exp_obs, exp_mask = obs_ref.observe(lv, A, cs.K, state, cs.pitch, B)
    assert exp_obs[:, 3:10].any() and (exp_mask != 31).any()
    lim = (B + 3) // 4 * 4
    for dtype, np_t in ((capi.OC_OBS_U8, np.uint8), (capi.OC_OBS_F16, np.float16)):
        es = np.dtype(np_t).itemsize
        obs = np.full(n * es + 64, 0xA5, np.uint8)
        mask = np.full((A, cs.pitch), 0xA5, np.uint8)
        assert raw_observe(cs, state, obs, mask, dtype) == 0
        got = obs[:n * es].view(np.uint8 if es == 1 else np.uint16).reshape(exp_obs.shape)
        for e in range(0, B, 8192):  # bit for bit (a chunk at a time: the f16 planes are large)
            exp = exp_obs[e:e + 8192]
            assert np.array_equal(got[e:e + 8192], exp if es == 1 else HALF_BITS[exp]), (dtype, e)
        assert (obs[n * es:] == 0xA5).all()
        assert np.array_equal(mask[:, :B], exp_mask) and (mask[:, lim:] == 0xA5).all()


def test_each_output_alone():
    G = group(0)
    cs = CpuStepper(G.level, G.A, G.B)
    obs = np.empty(G.obs.shape, np.uint8)
    assert raw_observe(cs, G.state, obs, None, capi.OC_OBS_U8) == 0 and np.array_equal(obs, G.obs)
    mask = np.zeros((G.A, G.pitch), np.uint8)
    assert raw_observe(cs, G.state, None, mask, capi.OC_OBS_U8) == 0 and np.array_equal(mask[:, :G.B], G.mask)


def test_bad_arguments_are_refused():
    G = group(0)
    cs = CpuStepper(G.level, G.A, G.B)
    obs = np.empty(G.obs.shape, np.uint8)
    mask = np.zeros((G.A, G.pitch), np.uint8)
    buf = ctypes.create_string_buffer(256)
    for args, word in (((None, None, capi.OC_OBS_U8, -1), b"both NULL"), ((obs, mask, 2, -1), b"dtype 2"),
                       ((obs, mask, capi.OC_OBS_U8, G.A), b"view_agent %d" % G.A),
                       ((obs, mask, capi.OC_OBS_U8, -2), b"view_agent -2")):
        assert raw_observe(cs, G.state, *args) == capi.OC_EINVAL
        assert word in cs.lib.oc_last_error()
        assert cs.lib.oc_get_last_error(cs._h, buf, len(buf)) > 0 and word in buf.value
    # the device entry point refuses a host-only handle
    rc = cs.lib.oc_observe(cs._h, G.state.ctypes.data, obs.ctypes.data, mask.ctypes.data, capi.OC_OBS_U8, -1, G.B, None)
    assert rc == capi.OC_EINVAL and b"host-only handle" in cs.lib.oc_last_error()
