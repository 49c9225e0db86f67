// oc_observe.h -- grid feature planes and per-agent legal-move masks of the batched env
// (oc_observe / oc_cpu_observe, include/oc_engine.h).  Included by oc_engine.hip.
//
// Per env the observation is C = 10 + A planes of H x W small counts:
//   0..2   Counter, Cutboard, Delivery squares      (GridSquare subclasses, utils/core.py:28-120)
//   3..8   Fresh/Chopped Tomato, Lettuce, Onion     (+1 per content of every Object, held or not,
//   9      Plate                                      at obj.location; utils/core.py:130-305)
//   10+    agent i at channel 10 + ((i - view) mod A)
// and the action mask is nav_utils.get_single_actions (navigation_planner/utils.py:55-90) on the
// full env: bit k = World.NAV_ACTIONS[k] is in the list, bit 4 (no-op) always.
//
// The decode below (item channels, legal moves) is one set of host/device functions: the kernel
// runs it on a tile of envs staged in LDS, oc_cpu_observe on host memory.
#ifndef OC_OBSERVE_H_
#define OC_OBSERVE_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/oc_engine.h"
#include "oc_layout.h"

#define OC_OH __host__ __device__ inline __attribute__((always_inline))

namespace ocob {

constexpr int kBlock = 256;
constexpr int kMaxTileEnvs = 64;     // envs per block: a power of two, at most kBlock / OC_MAX_AGENTS
constexpr int kLdsBudget = 48 * 1024;  // the default dynamic-LDS limit: no function attribute needed

// Static level data of the observation, by value in the kernel arguments.
struct ObsArgs {
    int32_t W, H, HW;
    int32_t C, CHW;        // channels, elements per env
    int32_t counts;        // item masks in OC_ENC_COUNTS
    int32_t rot;           // view agent (0 for view_agent -1): agent i -> channel 10 + (i - rot) mod A
    int32_t nstatic;       // entries of the static list (non-Floor squares)
    int32_t tile_envs;     // E: envs per block
    int32_t log2_envs;
    int32_t nt;            // non-temporal output stores
    int32_t lds_state, lds_tiles, lds_statics, lds_mask;  // byte offsets of the LDS sections after the tile
    int64_t pitch, B;
};

// The observation channels of one item content mask: add(channel, count) per content kind
// (counts encoding: OC_MC_FRESH marks a single fresh food, every other food is chopped; the
// translation oc_render_kernel's push_item makes).
template <class Add>
OC_OH void item_channels(uint32_t m, bool counts, Add&& add) {
    if (counts) {
        const uint32_t chopped = (m & OC_MC_FRESH) ? 0u : 1u;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            const uint32_t n = (m >> (2 * f)) & 3u;
            if (n != 0u) add(OC_OBS_STATIC + 2 * f + (int)chopped, n);
        }
        if (m & OC_MC_PLATE) add(OC_OBS_STATIC + 6, 1u);
    } else {
#pragma unroll
        for (int f = 0; f < 3; ++f)
            if ((m >> f) & 1u) add(OC_OBS_STATIC + 2 * f + (int)((m >> (OC_M_CHOPPED_SHIFT + f)) & 1u), 1u);
        if (m & OC_M_PLATE) add(OC_OBS_STATIC + 6, 1u);
    }
}

// core.mergeable (utils/core.py:222-241) in the level's mask encoding: at most one plate, every
// food in its last state.
OC_OH bool mergeable(uint32_t a, uint32_t b, bool counts) {
    const uint32_t u = a | b;
    return counts ? !(a & b & OC_MC_PLATE) && !(u & OC_MC_FRESH)
                  : !(a & b & OC_M_PLATE) && ((u & 7u) & ~(u >> OC_M_CHOPPED_SHIFT)) == 0u;
}

using ocly::Planes;  // the observation reads the planes before T (t and flags follow)

// Whether World.NAV_ACTIONS[k] is in get_single_actions of agent a (navigation_planner/
// utils.py:55-90): get(plane) reads this env's byte of a plane, tile(cell) the level's OC_TILE_*
// class.  Every agent's square blocks (the agent's own too: `new_loc not in agent_locs`, which
// matters where inbounds clamps).
template <int A, int K, bool WIDE, class Get, class Tile>
OC_OH bool move_legal(int a, int k, int W, int H, bool counts, Get&& get, Tile&& tile) {
    using PL = Planes<A, K, WIDE>;
    const int x = (int)get(PL::X + a), y = (int)get(PL::Y + a);
    const int dx = k == OC_ACT_LEFT ? -1 : (k == OC_ACT_RIGHT ? 1 : 0);
    const int dy = k == OC_ACT_DOWN ? 1 : (k == OC_ACT_UP ? -1 : 0);
    int nx = x + dx, ny = y + dy;  // World.inbounds (utils/world.py:432-436)
    nx = nx < 0 ? 0 : (nx > W - 1 ? W - 1 : nx);
    ny = ny < 0 ? 0 : (ny > H - 1 ? H - 1 : ny);
    bool blocked = false;
#pragma unroll
    for (int b = 0; b < A; ++b) blocked |= (int)get(PL::X + b) == nx && (int)get(PL::Y + b) == ny;
    const int c = ny * W + nx;
    const int t = (int)tile(c);
    if (blocked) return false;
    if (t == OC_TILE_FLOOR || t == OC_TILE_DELIVERY) return true;
    // a Counter or Cutboard: its object (at most one off Delivery; held ones sit on Floor)
    int o = -1;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int lc = WIDE ? (int)get(PL::LOC + j) | (int)get(PL::LOC_HI + j) << 8 : (int)get(PL::LOC + j);
        if (lc == c) o = j;
    }
    const uint32_t h = get(PL::HOLD + a);
    const bool holding = h < (uint32_t)K;
    if (o < 0) return holding;                                             // put down
    return !holding || mergeable(get(PL::MASK + (int)h), get(PL::MASK + o), counts);  // pick up, merge
}

template <int A, int K, bool WIDE, class Get, class Tile>
OC_OH uint32_t action_mask(int a, int W, int H, bool counts, Get&& get, Tile&& tile) {
    uint32_t bits = 1u << OC_ACT_NOOP;
    for (int k = 0; k < 4; ++k) bits |= move_legal<A, K, WIDE>(a, k, W, H, counts, get, tile) ? 1u << k : 0u;
    return bits;
}

// IEEE half of a small count (exact below 2,048): the host's conversion.
inline uint16_t half_of_count(uint32_t n) {
    if (n == 0u) return 0;
    int e = 31 - __builtin_clz(n);
    return (uint16_t)(((uint32_t)(e + 15) << 10) | ((n << (10 - e)) & 0x3FFu));
}

// oc_cpu_observe's worker: envs [e0, e1) of a host batch, the same decode as the kernel.
template <int A, int K, bool WIDE>
void cpu_observe_range(const ObsArgs& R, const uint8_t* tiles, const uint16_t* statics, const uint8_t* state,
                       void* obs, uint8_t* mask, bool f16, int64_t e0, int64_t e1) {
    using PL = Planes<A, K, WIDE>;
    const int64_t P = R.pitch;
    uint8_t buf[OC_OBS_CHANNELS(OC_MAX_AGENTS) * OC_MAX_CELLS];
    for (int64_t e = e0; e < e1; ++e) {
        auto get = [&](int plane) -> uint32_t { return state[(int64_t)plane * P + e]; };
        if (obs != nullptr) {
            memset(buf, 0, (size_t)R.CHW);
            for (int s = 0; s < R.nstatic; ++s) buf[statics[s]] = 1;
            for (int j = 0; j < K; ++j) {
                const int c = WIDE ? (int)get(PL::LOC + j) | (int)get(PL::LOC_HI + j) << 8 : (int)get(PL::LOC + j);
                if (c >= R.HW) continue;  // a dead slot (0xFF / 0xFFFF) is no cell
                item_channels(get(PL::MASK + j), R.counts != 0,
                              [&](int ch, uint32_t n) { buf[ch * R.HW + c] = (uint8_t)(buf[ch * R.HW + c] + n); });
            }
            for (int a = 0; a < A; ++a) {
                const int x = (int)get(PL::X + a), y = (int)get(PL::Y + a);
                if (x >= R.W || y >= R.H) continue;
                const int ch = OC_OBS_STATIC + OC_OBS_ITEM + (a - R.rot + A) % A;
                buf[ch * R.HW + y * R.W + x] += 1;
            }
            if (f16) {
                uint16_t* o = (uint16_t*)obs + e * R.CHW;
                for (int i = 0; i < R.CHW; ++i) o[i] = half_of_count(buf[i]);
            } else {
                memcpy((uint8_t*)obs + e * R.CHW, buf, (size_t)R.CHW);
            }
        }
        if (mask != nullptr)
            for (int a = 0; a < A; ++a)
                mask[(int64_t)a * P + e] = (uint8_t)action_mask<A, K, WIDE>(a, R.W, R.H, R.counts != 0, get,
                                                                           [&](int c) { return tiles[c]; });
    }
}

#if defined(__HIPCC__)
// A block handles tiles of E consecutive envs: in [B][C][H][W] a tile is one contiguous run of
// E * CHW elements.  The tile is staged as u8 in LDS (zero fill, then the level's static squares
// and the envs' items and agents as LDS adds on the containing word: exact, no count reaches
// 256), and after a barrier the whole block streams it out in 16-byte stores, consecutive lanes
// on consecutive addresses (u8 -> half in registers for OC_OBS_F16).  The tile sits in LDS at the
// byte phase of its output address (pad), so a 16-byte output chunk is one aligned LDS read
// whatever E * CHW and the output pointer are: tiles of a multiple of 16 envs in a 16-byte
// aligned buffer have pad 0 and only full chunks; a smaller tile's (large levels) head and tail
// chunks, and the batch's last one, go out element by element.  Nothing outside the B * CHW
// elements is written.  The action mask comes from the same staged state: thread (env, a)
// evaluates agent a, the bytes meet in LDS and leave four envs per word.
// The grid is persistent (as many blocks as the CUs' LDS holds): a block loads its next tile's
// state words into registers before it streams the current tile out, so no tile waits for
// device memory, and the level's tables are staged in LDS once per block.  (Measured against
// one block per tile: the same time within the noise; kept for the tables.)
template <int A, int K, bool WIDE, bool F16>
__global__ __launch_bounds__(kBlock) void oc_observe_kernel(ObsArgs R, const uint8_t* __restrict__ state,
                                                            const uint8_t* __restrict__ tiles_g,
                                                            const uint16_t* __restrict__ statics_g,
                                                            uint8_t* __restrict__ obs, uint8_t* __restrict__ mask) {
    using PL = Planes<A, K, WIDE>;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) uint8_t obs_lds[];
    constexpr int kEs = F16 ? 2 : 1;          // output element size
    constexpr int kV = 16 / kEs;              // elements (LDS bytes) per 16-byte output chunk
    constexpr int kStage = 4;                 // state words per lane: PL::T * E / 4 <= 60 * 16 words
    const int t = (int)threadIdx.x, E = R.tile_envs, lg = R.log2_envs;
    const int wpe = E >> 2, nw = PL::T * wpe;  // four envs per word (tiles and the pitch are multiples of E)
    const int env = t & (E - 1), part = t >> lg, parts = kBlock >> lg;
    const int64_t ntiles = (R.B + E - 1) >> lg;
    uint32_t* tile32 = (uint32_t*)obs_lds;
    uint8_t* st = obs_lds + R.lds_state;
    uint8_t* tl = obs_lds + R.lds_tiles;
    const uint16_t* statics = (const uint16_t*)(obs_lds + R.lds_statics);
    uint8_t* mk = obs_lds + R.lds_mask;

    uint32_t sw[kStage];
    auto load_state = [&](int64_t tile) {  // a tile's state words into registers
        if (E < 4) return;
#pragma unroll
        for (int r = 0; r < kStage; ++r) {
            const int i = t + r * kBlock, plane = i / wpe, w = i - plane * wpe;
            sw[r] = i < nw ? *(const uint32_t*)(state + (int64_t)plane * R.pitch + tile * E + 4 * w) : 0u;
        }
    };
    int64_t tile = blockIdx.x;
    if (tile < ntiles) load_state(tile);
    // the level's tile classes (at most OC_MAX_CELLS / 4 = kBlock words) and static list, once
    if (t < ((R.HW + 3) >> 2)) ((uint32_t*)tl)[t] = ((const uint32_t*)tiles_g)[t];
    for (int i = t; i < (R.nstatic + 1) >> 1; i += kBlock)
        ((uint32_t*)(obs_lds + R.lds_statics))[i] = ((const uint32_t*)statics_g)[i];

    for (; tile < ntiles; tile += gridDim.x) {
        const int64_t env0 = tile * E;
        const int envs = (int)(R.B - env0 < (int64_t)E ? R.B - env0 : (int64_t)E);  // live envs of the tile
        const int n = envs * R.CHW;                                                 // its elements
        const int64_t o0 = env0 * R.CHW;                                            // its first element
        // the tile's byte phase in LDS = its first element's phase within a 16-byte output chunk
        const int pad = obs != nullptr ? (int)((((uintptr_t)obs + (uint64_t)o0 * kEs) & 15u) / kEs) : 0;
        // zero the tile (16 bytes per lane) and put its state bytes in LDS
        if (obs != nullptr) {
            u32x4* z = (u32x4*)obs_lds;
            const int nz = (pad + E * R.CHW + 15) >> 4;
            for (int i = t; i < nz; i += kBlock) z[i] = u32x4{0u, 0u, 0u, 0u};
        }
        if (t < (A * E + 3) >> 2) ((uint32_t*)mk)[t] = 0x01010101u << OC_ACT_NOOP;  // no-op: always legal
        if (E >= 4) {
#pragma unroll
            for (int r = 0; r < kStage; ++r)
                if (t + r * kBlock < nw) ((uint32_t*)st)[t + r * kBlock] = sw[r];
        } else {
            for (int i = t; i < PL::T * E; i += kBlock) st[i] = state[(int64_t)(i >> lg) * R.pitch + env0 + (i & (E - 1))];
        }
        __syncthreads();
        if (tile + gridDim.x < ntiles) load_state(tile + gridDim.x);  // lands behind this tile's stores

        auto get = [&](int plane) -> uint32_t { return st[plane * E + env]; };
        if (obs != nullptr) {
            auto add = [&](int idx, uint32_t cnt) {  // element idx of the tile += cnt
                idx += pad;
                atomicAdd(&tile32[idx >> 2], cnt << (8 * (idx & 3)));
            };
            // the level's non-Floor squares, every env of the tile
            for (int i = t; i < R.nstatic << lg; i += kBlock) add((i & (E - 1)) * R.CHW + (int)statics[i >> lg], 1u);
            if (env < envs) {
                const int base = env * R.CHW;
                for (int j = part; j < K; j += parts) {
                    const int c = WIDE ? (int)get(PL::LOC + j) | (int)get(PL::LOC_HI + j) << 8 : (int)get(PL::LOC + j);
                    if (c >= R.HW) continue;  // a dead slot (0xFF / 0xFFFF) is no cell
                    item_channels(get(PL::MASK + j), R.counts != 0,
                                  [&](int ch, uint32_t cnt) { add(base + ch * R.HW + c, cnt); });
                }
                if (part < A) {
                    const int x = (int)get(PL::X + part), y = (int)get(PL::Y + part);
                    int ch = part - R.rot;
                    ch += ch < 0 ? A : 0;
                    if (x < R.W && y < R.H) add(base + (OC_OBS_STATIC + OC_OBS_ITEM + ch) * R.HW + y * R.W + x, 1u);
                }
            }
        }
        // the 4 A (agent, move) tests of an env are spread over its `parts` threads, so every wave
        // of the block carries a share; a legal move sets its bit in the env's LDS mask byte
        if (mask != nullptr && env < envs)
            for (int u = part; u < 4 * A; u += parts) {
                const int a = u >> 2, idx = a * E + env;
                if (move_legal<A, K, WIDE>(a, u & 3, R.W, R.H, R.counts != 0, get, [&](int c) { return tl[c]; }))
                    atomicOr(&((uint32_t*)mk)[idx >> 2], (1u << (u & 3)) << (8 * (idx & 3)));
            }
        __syncthreads();

        if (mask != nullptr) {
            if (E >= 4) {  // the batch's last word is completed (no-op only past B)
                for (int i = t; i < A * wpe; i += kBlock) {
                    const int a = i / wpe, w = i - a * wpe;
                    if (4 * w < envs) *(uint32_t*)(mask + (int64_t)a * R.pitch + env0 + 4 * w) = ((const uint32_t*)mk)[i];
                }
            } else if (part < A && env < envs) {
                mask[(int64_t)part * R.pitch + env0 + env] = mk[part * E + env];
            }
        }
        if (obs != nullptr) {
            // stream the tile out: chunk q is LDS bytes [q kV, q kV + kV) = 16 output bytes at base + 16 q
            u32x4* base = (u32x4*)(obs + ((uint64_t)o0 * kEs - (uint64_t)pad * kEs));  // 16-byte aligned
            const int nq = (pad + n + kV - 1) / kV;
            auto chunk = [&](int q) -> u32x4 {
                if constexpr (F16) {
                    // a byte b beside 0x64 is the half 1024 + b; minus 1024 leaves the half of b, exact
                    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                    const u32x2 raw = ((const u32x2*)obs_lds)[q];
                    auto two = [](uint32_t w, uint32_t sel) -> uint32_t {
                        const h2 k = {(_Float16)1024.0f, (_Float16)1024.0f};
                        const h2 p = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, w, sel)) - k;
                        return __builtin_bit_cast(uint32_t, p);
                    };
                    return u32x4{two(raw.x, 0x04010400u), two(raw.x, 0x04030402u), two(raw.y, 0x04010400u),
                                 two(raw.y, 0x04030402u)};
                } else {
                    return ((const u32x4*)obs_lds)[q];
                }
            };
            if (pad == 0 && n % kV == 0) {  // every chunk whole (block-uniform): the main path
                if (R.nt)
                    for (int q = t; q < nq; q += kBlock) __builtin_nontemporal_store(chunk(q), base + q);
                else
                    for (int q = t; q < nq; q += kBlock) base[q] = chunk(q);
            } else {
                for (int q = t; q < nq; q += kBlock) {
                    const int lo = q * kV;
                    const u32x4 v = chunk(q);
                    if (lo >= pad && lo + kV <= pad + n) {
                        base[q] = v;
                    } else {  // a head or tail chunk: only the tile's own elements
                        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int i = 0; i < kV; ++i) {
                            if (lo + i < pad || lo + i >= pad + n) continue;
                            if constexpr (F16) ((uint16_t*)(base + q))[i] = (uint16_t)(w[i >> 1] >> (16 * (i & 1)));
                            else ((uint8_t*)(base + q))[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
                        }
                    }
                }
            }
        }
        __syncthreads();  // the tile and the mask bytes are read: the next tile may overwrite them
    }
}
#endif  // __HIPCC__

}  // namespace ocob

#endif  // OC_OBSERVE_H_
