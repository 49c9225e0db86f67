// oc_startdist.h -- randomised episode starts (oc_reset_random / oc_cpu_reset_random,
// include/oc_engine.h): per env, the agents drawn onto Floor cells and the level's items onto Counter
// cells, which is the state the reference builds when it loads the level file with its item letters
// and spawn lines moved there (load_level, gym_cooking/envs/overcooked_environment.py:144-193).
// Included by oc_engine.hip.
//
// The draw of env gid = env_offset + e (the contract; tests/start_ref.py restates it in numpy):
//   base    = seed ^ gid * 0x9E3779B97F4A7C15 ^ round * 0xC2B2AE3D27D4EB4F
//   u(d)    = splitmix64(base ^ (0x53540000 + d))
//   r(d, n) = (uint32)(((u(d) >> 32) * n) >> 32)
//   agent i : the r(i, |LA_i| - m)-th cell of LA_i, ascending, that no earlier agent occupies, m the
//             earlier agents on a cell of LA_i
//   slot k  : the r(16 + k, |LI| - k)-th cell of LI, ascending, that no earlier slot took (the live
//             template slots are 0 .. items - 1, so slot k has k earlier ones)
// The "r-th free cell" needs no sort and no register array with a run-time index: from idx = r,
// idx = r + #{taken cells of the list at or below L[idx]} until it stops changing.  idx never
// passes the answer, every round but the last moves it past at least one more taken cell, so m
// rounds reach it; the loops over the earlier draws are unrolled over A and K.
//
// Everything here is plain host/device C++ on plane words (four envs per dword, ocio::Chunk): the
// kernel runs it on registers with the tables in LDS, oc_cpu_reset_random on host memory.  A build
// without the HIP compiler (tests/start_host/) defines __host__ / __device__ / __forceinline__
// itself, as for oc_swar.h.
#ifndef OC_STARTDIST_H_
#define OC_STARTDIST_H_

#include <cstdint>
#include <cstring>

#include "../../include/oc_engine.h"
#include "oc_layout.h"
#include "oc_stepio.h"
#include "oc_swar.h"

namespace ocsd {

using ocly::Planes;

constexpr int kBlock = 256;
constexpr uint64_t kDrawTag = 0x53540000ull;  // keeps these draws apart from oc_gen_actions' (agent ids 0..3)

// The call's constants, by value in the kernel arguments.
struct StartArgs {
    int32_t S;        // entries per list and of the x/y table: W * H rounded up to even
    int32_t S2;       // bytes per agent of the agent_ok table: W * H rounded up to 4
    int32_t nI;       // |LI|
    int32_t items;    // live template slots: 0 .. items - 1
    int32_t what;     // OC_START_*
    int32_t masked;   // state_prev given: only its DONE envs restart
    int32_t nA[OC_MAX_AGENTS];  // |LA_i|
    int64_t pitch, B, env_offset;
    uint64_t seed, round;
};

// The handle's start table, one blob: u16 lists[A + 1][S] (LA_0 .. LA_{A-1}, then LI, ascending cell
// ids), u16 xy[S] (x | y << 8 of a cell), u8 ok[A][S2] (agent_ok).
inline int table_bytes(int A, int S, int S2) { return (A + 2) * S * 2 + A * S2; }

struct Tab {
    const uint16_t *L, *xy;
    const uint8_t* ok;
    int S, S2;
};
template <int A>
OC_SW Tab tab_of(const void* base, const StartArgs& R) {
    const uint16_t* p = (const uint16_t*)base;
    return Tab{p, p + (A + 1) * R.S, (const uint8_t*)(p + (A + 2) * R.S), R.S, R.S2};
}

OC_SW uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

OC_SW uint32_t draw(uint64_t base, uint32_t d, uint32_t n) {
    const uint64_t u = splitmix64(base ^ (kDrawTag + d));
    return (uint32_t)(((u >> 32) * (uint64_t)n) >> 32);
}

// One env's draws: ax / ay the agents' squares (what & OC_START_AGENTS), ic the cells of slots
// 0 .. items - 1 (what & OC_START_ITEMS); the other outputs are not written.
template <int A, int K>
OC_SW void draw_env(const StartArgs& R, const Tab& T, uint64_t gid, uint32_t (&ax)[A], uint32_t (&ay)[A],
                    uint32_t (&ic)[K]) {
    const uint64_t base = R.seed ^ (gid * 0x9E3779B97F4A7C15ull) ^ (R.round * 0xC2B2AE3D27D4EB4Full);
    if (R.what & OC_START_AGENTS) {
        uint32_t cell[A];
#pragma unroll
        for (int i = 0; i < A; ++i) {
            const uint16_t* L = T.L + i * T.S;
            const uint8_t* ok = T.ok + i * T.S2;
            uint32_t in[A], m = 0u;  // earlier agents on a cell of LA_i
#pragma unroll
            for (int j = 0; j < i; ++j) {
                in[j] = ok[cell[j]] != 0 ? 1u : 0u;
                m += in[j];
            }
            const uint32_t r = draw(base, (uint32_t)i, (uint32_t)R.nA[i] - m);
            uint32_t idx = r;
#pragma unroll
            for (int t = 0; t < i; ++t) {  // m <= i rounds reach the fixed point
                const uint32_t c = L[idx];
                uint32_t cnt = 0u;
#pragma unroll
                for (int j = 0; j < i; ++j) cnt += in[j] & (cell[j] <= c ? 1u : 0u);
                idx = r + cnt;
            }
            cell[i] = L[idx];
            const uint32_t xy = T.xy[cell[i]];
            ax[i] = xy & 0xFFu;
            ay[i] = xy >> 8;
        }
    }
    if (R.what & OC_START_ITEMS) {
        const uint16_t* L = T.L + A * T.S;
        uint32_t pos[K];  // the slots' positions in LI
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (k < R.items) {
                const uint32_t r = draw(base, 16u + (uint32_t)k, (uint32_t)(R.nI - k));
                uint32_t idx = r;
#pragma unroll 1
                for (int t = 0; t < k; ++t) {
                    uint32_t cnt = 0u;
#pragma unroll
                    for (int j = 0; j < k; ++j) cnt += pos[j] <= idx ? 1u : 0u;
                    if (r + cnt == idx) break;
                    idx = r + cnt;
                }
                pos[k] = idx;
                ic[k] = L[idx];
            }
        }
    }
}

// The start of word g's four envs: the level template, and in the envs of `sel` (bit q: env 4g + q)
// the drawn parts.
template <int A, int K, bool WIDE>
OC_SW void start_chunk(const ocsw::SwarLevel& sw, const StartArgs& R, const Tab& T, int64_t g, uint32_t sel,
                       ocio::Chunk<A, K, WIDE>& c) {
    c = ocio::template_chunk<A, K, WIDE>(sw);
    // each round takes every lane's lowest remaining env, whichever column it is: a wave whose lanes
    // have one restarting env each (masked mode at a few percent) draws once, not four times
#pragma unroll 1
    for (; sel != 0u; sel &= sel - 1u) {
        const int q = __builtin_ctz(sel);
        uint32_t ax[A], ay[A], ic[K];
        draw_env<A, K>(R, T, (uint64_t)(R.env_offset + 4 * g + q), ax, ay, ic);
        const uint32_t sh = 8u * (uint32_t)q, keep = ~(0xFFu << sh);
        if (R.what & OC_START_AGENTS) {
#pragma unroll
            for (int a = 0; a < A; ++a) {
                c.wx[a] = (c.wx[a] & keep) | (ax[a] << sh);
                c.wy[a] = (c.wy[a] & keep) | (ay[a] << sh);
            }
        }
        if (R.what & OC_START_ITEMS) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (k < R.items) {
                    c.wl[k] = (c.wl[k] & keep) | ((ic[k] & 0xFFu) << sh);
                    if constexpr (WIDE) c.wlh[k] = (c.wlh[k] & keep) | ((ic[k] >> 8) << sh);
                }
            }
        }
    }
}

// Masked mode on words: the bytes of `bm` (0xFF per restarting env) of `n` into `o`.
template <int A, int K, bool WIDE>
OC_SW void merge(ocio::Chunk<A, K, WIDE>& o, const ocio::Chunk<A, K, WIDE>& n, uint32_t bm) {
    auto mix = [bm](uint32_t& ow, uint32_t nw) { ow = (ow & ~bm) | (nw & bm); };
#pragma unroll
    for (int a = 0; a < A; ++a) {
        mix(o.wx[a], n.wx[a]);
        mix(o.wy[a], n.wy[a]);
        mix(o.wh[a], n.wh[a]);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        mix(o.wl[j], n.wl[j]);
        if constexpr (WIDE) mix(o.wlh[j], n.wlh[j]);
        mix(o.wm[j], n.wm[j]);
    }
    // the u16 step counts: envs 0, 1 in t0 and 2, 3 in t1; a start has t = 0
    const uint32_t m0 = ((bm & 0xFFu) ? 0xFFFFu : 0u) | ((bm & 0xFF00u) ? 0xFFFF0000u : 0u);
    const uint32_t m1 = ((bm & 0xFF0000u) ? 0xFFFFu : 0u) | ((bm & 0xFF000000u) ? 0xFFFF0000u : 0u);
    o.t0 = (o.t0 & ~m0) | (n.t0 & m0);
    o.t1 = (o.t1 & ~m1) | (n.t1 & m1);
    mix(o.wf, n.wf);
}

// ---- host ------------------------------------------------------------------------------------

// The host store: only the bytes of the envs in `sel` of word g are written, nothing else is touched.
struct HostEnvBytes {
    uint8_t* p;
    int64_t P, g;
    uint32_t sel;
    void st32(int plane, uint32_t v) const {
        for (int q = 0; q < ocio::kEPL; ++q)
            if ((sel >> q) & 1u) p[plane * P + 4 * g + q] = (uint8_t)(v >> (8 * q));
    }
    void st64(int plane, uint32_t lo, uint32_t hi) const {
        for (int q = 0; q < ocio::kEPL; ++q)
            if ((sel >> q) & 1u) {
                const uint32_t v = ((q < 2 ? lo : hi) >> (16 * (q & 1))) & 0xFFFFu;
                p[plane * P + 8 * g + 2 * q] = (uint8_t)v;
                p[plane * P + 8 * g + 2 * q + 1] = (uint8_t)(v >> 8);
            }
    }
};

// oc_cpu_reset_random's worker: words [g0, g1) of a host batch (four envs each, as one lane of the
// kernel).  Only bytes of envs below B are read (the flags of sprev) or written.
template <int A, int K, bool WIDE>
void host_start_range(const ocsw::SwarLevel& sw, const StartArgs& R, const void* table, uint8_t* s,
                      const uint8_t* sprev, int64_t g0, int64_t g1) {
    using PL = Planes<A, K, WIDE>;
    const Tab T = tab_of<A>(table, R);
    for (int64_t g = g0; g < g1; ++g) {
        const int64_t rem = R.B - 4 * g;
        const int ncol = rem >= 4 ? 4 : (int)rem;
        uint32_t sel = 0u;
        for (int q = 0; q < ncol; ++q)
            if (sprev == nullptr || (sprev[PL::F * R.pitch + 4 * g + q] & OC_FLAG_DONE)) sel |= 1u << q;
        if (sel == 0u) continue;
        ocio::Chunk<A, K, WIDE> c;
        start_chunk<A, K, WIDE>(sw, R, T, g, sel, c);
        ocio::store(c, HostEnvBytes{s, R.pitch, g, sel});
    }
}

}  // namespace ocsd

#endif  // OC_STARTDIST_H_
