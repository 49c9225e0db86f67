// oc_progress.h -- per-subtask object counts, completion events and shaped reward of the batched
// env (oc_progress / oc_cpu_progress, include/oc_engine.h).  Included by oc_engine.hip.
//
// count_i(s) of a state s and a subtask i (kind, goal mask) is the reference agent's goal-object
// count, RealAgent.def_subtask_completion (gym_cooking/utils/agent.py:286-368):
//   Chop, Merge   len(world.get_all_object_locs(goal_obj))     utils/world.py:354-387: a
//                 list(set(...)) of locations, held objects at their holder's square
//   Deliver       len of the LIST of goal objects, not held, on any Delivery square (:354-361)
//   None          0
// and event i of a transition (prev, cur) is is_subtask_complete(cur.world) of an agent whose
// def_subtask_completion ran on prev: count_i(cur) > count_i(prev); none when prev was DONE
// (cur is then the auto-reset state).  reward = the weights of the set events, added in
// ascending i from +0.0f with plain f32 adds.
//
// Everything below the kernel is one set of host/device functions on plane words (four envs per
// dword, the byte predicates of oc_swar.h): the kernel runs them on registers, oc_cpu_progress on
// host memory.  A build without the HIP compiler (tests/progress_host/, plain clang++ with
// sanitizers) defines __host__ / __device__ / __forceinline__ itself, as for oc_swar.h, and gets
// the host functions only.
#ifndef OC_PROGRESS_H_
#define OC_PROGRESS_H_

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <cstdint>
#include <cstring>

#include "../../include/oc_engine.h"
#include "oc_layout.h"
#include "oc_swar.h"

namespace ocpg {

constexpr int kBlock = 256;                 // one Delivery-table word per thread
constexpr int kTableBytes = OC_MAX_CELLS;   // h80 per cell id: the cell is a Delivery square

// The call's constants, by value in the kernel arguments (scalar loads, uniform indices).
struct ProgArgs {
    int32_t W;            // grid width (a holder's cell is y * W + x)
    int32_t tile_words;   // words of the level's tile table (W * H bytes rounded up to 4)
    int32_t n, S;         // steps, subtasks
    int32_t planes;       // OC_PROGRESS_EVENT_PLANES(S)
    int64_t pitch, B;
    int64_t state_bytes;  // distance between consecutive states
    uint32_t sub[OC_MAX_SUBTASKS];   // kind << 8 | goal mask
    float weight[OC_MAX_SUBTASKS];
};

using ocly::Planes;

// What the counts read of one state's four envs: per slot the mask word and two h80 words,
//   nd : the slot is live and the first live slot of its (cell, mask) -- among the slots whose
//        mask equals a goal mask these are the distinct cells, whatever the goal mask is, so the
//        "same cell" relation is taken once per env and not once per subtask
//   dl : the slot is live, not held and lies on a Delivery square
// and the env's DONE flag as h80.
template <int K>
struct View {
    uint32_t M[K], nd[K], dl[K];
    uint32_t done80;
};

// h80 per env: cell (lo, or hi << 8 | lo on a wide level) is a Delivery square.  tab holds 0x80
// for Delivery cells and 0 for every other id below kTableBytes (dead narrow cells read 0).
template <bool WIDE>
OC_SW uint32_t on_delivery(const uint8_t* tab, uint32_t lo, uint32_t hi) {
    uint32_t r = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t idx = (lo >> (8 * q)) & 0xFFu;
        if (WIDE) idx = (idx | (((hi >> (8 * q)) & 0xFFu) << 8)) & (uint32_t)(kTableBytes - 1);
        r |= (uint32_t)tab[idx] << (8 * q);
    }
    return r;
}

// The View of a state from its plane words.  LO / HI are updated in place: a held item's cell
// becomes its holder's square (the lowest agent that names the slot; hold values that are no
// slot hold nothing).  HI is read on wide levels only.
template <int A, int K, bool WIDE>
OC_SW void derive(uint32_t W, const uint8_t* tab, const uint32_t (&X)[A], const uint32_t (&Y)[A],
                  const uint32_t (&H)[A], uint32_t (&LO)[K], uint32_t (&HI)[K], const uint32_t (&M)[K], uint32_t F,
                  View<K>& v) {
    using namespace ocsw;
    uint32_t live[K], held[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t dead = WIDE ? zf80(~(LO[j] & HI[j])) : zf80(~LO[j]);  // OC_LOC_DEAD / OC_LOC_DEAD16
        live[j] = dead ^ k80;
        held[j] = 0u;
        v.dl[j] = live[j] & on_delivery<WIDE>(tab, LO[j], HI[j]);
        v.M[j] = M[j];
    }
#pragma unroll
    for (int a = A - 1; a >= 0; --a) {
        uint32_t clo = 0u, chi = 0u;
        if (WIDE) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t c = ((Y[a] >> (8 * q)) & 0xFFu) * W + ((X[a] >> (8 * q)) & 0xFFu);
                clo |= (c & 0xFFu) << (8 * q);
                chi |= ((c >> 8) & 0xFFu) << (8 * q);
            }
        } else {
            clo = Y[a] * W + X[a];  // cells < 255: no carry between envs
        }
        // per-slot select masks, one v_perm each: selector byte = slot index, table byte j = 0xFF;
        // envs that hold no slot get selector 0x0C, a zero byte
        const uint32_t h = H[a];
        const uint32_t valid = full80(zf80(h & (0x01010101u * (uint32_t)(0xFF ^ (K - 1)))));
        uint32_t s_lo = sel(valid, h, 0x0C0C0C0Cu), s_hi = 0x0C0C0C0Cu;
        if constexpr (K == 16) {
            const uint32_t h8 = full80(and3(h << 4, k80, valid));  // index bit 3
            s_hi = sel(h8, h ^ k08, 0x0C0C0C0Cu);
            s_lo = sel(h8, 0x0C0C0C0Cu, s_lo);
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int jj = j & 7;
            const uint32_t lut_lo = jj < 4 ? 0xFFu << (8 * jj) : 0u, lut_hi = jj < 4 ? 0u : 0xFFu << (8 * (jj - 4));
            const uint32_t eh = perm(lut_hi, lut_lo, j < 8 ? s_lo : s_hi);
            LO[j] = sel(eh, clo, LO[j]);
            if (WIDE) HI[j] = sel(eh, chi, HI[j]);
            held[j] |= eh;
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        v.dl[j] = andn(v.dl[j], held[j]);
        uint32_t dup = 0u;  // an earlier live slot of the same cell and mask
#pragma unroll
        for (int i = 0; i < j; ++i) {
            uint32_t x = bop3<OC_LUT((a ^ b) | c)>(LO[j], LO[i], M[j] ^ M[i]);
            if (WIDE) x |= HI[j] ^ HI[i];
            dup |= bop3<OC_LUT(a & !(b | c))>(live[i], (x & k7F) + k7F, x);
        }
        v.nd[j] = andn(live[j], dup);
    }
    v.done80 = (F << 7) & k80;
}

// Per env: how many slots selected by S (h80) carry mask g (replicated); at most K <= 16.
template <int K>
OC_SW uint32_t count4(const uint32_t (&M)[K], const uint32_t (&S)[K], uint32_t g) {
    using namespace ocsw;
    uint32_t c = 0u;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t x = M[j] ^ g;
        c += bop3<OC_LUT(a & !(b | c))>(S[j], (x & k7F) + k7F, x) >> 7;
    }
    return c;
}

template <int K>
OC_SW uint32_t count_of(const View<K>& v, uint32_t sub) {
    const uint32_t kind = sub >> 8, g = (sub & 0xFFu) * 0x01010101u;
    if (kind == OC_SUB_DELIVER) return count4<K>(v.M, v.dl, g);
    if (kind == OC_SUB_NONE) return 0u;
    return count4<K>(v.M, v.nd, g);
}

// One transition of four envs: out.count(i, word), out.events(plane, word) and out.reward(f32[4])
// receive the output words; vmask keeps the envs below B (the others read zero).
template <int K, class Out>
OC_SW void progress_word(const ProgArgs& R, const View<K>& prev, const View<K>& cur, uint32_t vmask, Out&& out) {
    using namespace ocsw;
    float rw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t plane = 0u;
    for (int i = 0; i < R.S; ++i) {
        const uint32_t sub = R.sub[i];
        const uint32_t cp = count_of<K>(prev, sub), cc = count_of<K>(cur, sub);
        // counts are at most 16: (cp | 0x80) - cc keeps bit 7 iff cp >= cc, no borrow between envs
        const uint32_t ev = andn(andn(k80, (cp | k80) - cc), prev.done80) & vmask;
        out.count(i, cc & vmask);
        plane |= ev >> (7 - (i & 7));
        const float w = R.weight[i];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if ((ev >> (8 * q + 7)) & 1u) rw[q] += w;
        if ((i & 7) == 7 || i == R.S - 1) {
            out.events(i >> 3, plane);
            plane = 0u;
        }
    }
    out.reward(rw);
}

// The plane words of lane / word g of a state and their View.
template <int A, int K, bool WIDE>
OC_SW void load_view(const ProgArgs& R, const uint8_t* tab, const uint8_t* s, int64_t g, View<K>& v) {
    using PL = Planes<A, K, WIDE>;
    auto rd = [&](int plane) -> uint32_t {
#if defined(__HIP_DEVICE_COMPILE__)
        return *(const uint32_t*)(s + (int64_t)plane * R.pitch + 4 * g);
#else
        uint32_t w;
        memcpy(&w, s + (int64_t)plane * R.pitch + 4 * g, 4);
        return w;
#endif
    };
    uint32_t X[A], Y[A], H[A], LO[K], HI[K], M[K];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        X[a] = rd(PL::X + a);
        Y[a] = rd(PL::Y + a);
        H[a] = rd(PL::HOLD + a);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        LO[j] = rd(PL::LOC + j);
        HI[j] = WIDE ? rd(PL::LOC_HI + j) : 0u;
        M[j] = rd(PL::MASK + j);
    }
    derive<A, K, WIDE>((uint32_t)R.W, tab, X, Y, H, LO, HI, M, rd(PL::F), v);
}

// The Delivery table of a level from its OC_TILE_* bytes (tiles: tile_words words; ids past
// them read 0).
inline void build_table(const uint8_t* tiles, int tile_words, uint8_t* tab) {
    for (int c = 0; c < kTableBytes; ++c) tab[c] = (c < 4 * tile_words && tiles[c] == OC_TILE_DELIVERY) ? 0x80u : 0u;
}

// oc_cpu_progress's worker: words [g0, g1) of a host batch (four envs each, as one lane of the
// kernel); only columns below B are written.
template <int A, int K, bool WIDE>
void cpu_progress_words(const ProgArgs& R, const uint8_t* tab, const uint8_t* sprev, const uint8_t* states,
                        uint8_t* counts, uint8_t* events, float* reward, int64_t g0, int64_t g1) {
    struct Out {
        const ProgArgs& R;
        uint8_t *pc, *pe;
        float* pr;
        int64_t g;
        int r, ncol;
        void count(int i, uint32_t w) const {
            if (pc != nullptr) memcpy(pc + ((int64_t)r * R.S + i) * R.pitch + 4 * g, &w, (size_t)ncol);
        }
        void events(int c, uint32_t w) const {
            if (pe != nullptr) memcpy(pe + ((int64_t)r * R.planes + c) * R.pitch + 4 * g, &w, (size_t)ncol);
        }
        void reward(const float (&rw)[4]) const {
            if (pr != nullptr) memcpy(pr + (int64_t)r * R.pitch + 4 * g, rw, sizeof(float) * (size_t)ncol);
        }
    };
    for (int64_t g = g0; g < g1; ++g) {
        const int64_t rem = R.B - 4 * g;
        const int ncol = rem >= 4 ? 4 : (int)rem;
        const uint32_t vmask = ncol == 4 ? 0xFFFFFFFFu : (1u << (8 * (uint32_t)ncol)) - 1u;
        View<K> pv, cv;
        load_view<A, K, WIDE>(R, tab, sprev, g, pv);
        for (int r = 0; r < R.n; ++r) {
            load_view<A, K, WIDE>(R, tab, states + (int64_t)r * R.state_bytes, g, cv);
            progress_word<K>(R, pv, cv, vmask, Out{R, counts, events, reward, g, r, ncol});
            pv = cv;
        }
    }
}

#if defined(__HIPCC__)
// A streaming kernel on the state planes: one dword per lane per plane, four envs per lane (a
// wave touches 256 contiguous bytes of a plane, as oc_step), one lane per word of the batch.
// Loaded: the item cells, item masks, held slots, agent x / y and the flags; t is not.  In the
// trajectory form (n > 1) a lane walks the n states and keeps the previous state's View (3 K + 1
// words) in registers, so every state is loaded once.  Both counts of a subtask are taken from the
// two Views inside one loop over the subtasks, whose kind, mask and weight are scalar loads from
// the kernel arguments: nothing is indexed by a lane-varying or loop-varying register index, so
// nothing goes to scratch, however many subtasks the call has.  Outputs leave as dwords (four
// envs of a count or event plane) and the reward as one 16-byte store; the batch's last word
// is completed with zeros, lanes past it store nothing.  All offsets are 64-bit.
template <int A, int K, bool WIDE>
__global__ __launch_bounds__(kBlock) void oc_progress_kernel(ProgArgs R, const uint8_t* __restrict__ tiles_g,
                                                             const uint8_t* sprev, const uint8_t* states,
                                                             uint8_t* __restrict__ counts,
                                                             uint8_t* __restrict__ events,
                                                             float* __restrict__ reward) {
    __shared__ uint32_t tab4[kTableBytes / 4];
    {
        const int t = (int)threadIdx.x;
        const uint32_t w = t < R.tile_words ? ((const uint32_t*)tiles_g)[t] : 0u;
        tab4[t] = ocsw::zf80(w ^ (0x01010101u * OC_TILE_DELIVERY));
    }
    __syncthreads();
    const uint8_t* tab = (const uint8_t*)tab4;
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t rem = R.B - 4 * g;
    if (rem <= 0) return;
    const uint32_t vmask = rem >= 4 ? 0xFFFFFFFFu : (1u << (8 * (uint32_t)rem)) - 1u;
    struct Out {
        const ProgArgs& R;
        uint8_t *pc, *pe;
        float* pr;
        int64_t g;
        int r;
        __device__ void count(int i, uint32_t w) const {
            if (pc != nullptr) *(uint32_t*)(pc + ((int64_t)r * R.S + i) * R.pitch + 4 * g) = w;
        }
        __device__ void events(int c, uint32_t w) const {
            if (pe != nullptr) *(uint32_t*)(pe + ((int64_t)r * R.planes + c) * R.pitch + 4 * g) = w;
        }
        __device__ void reward(const float (&rw)[4]) const {
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            if (pr != nullptr) *(f32x4*)(pr + (int64_t)r * R.pitch + 4 * g) = f32x4{rw[0], rw[1], rw[2], rw[3]};
        }
    };
    View<K> pv, cv;
    load_view<A, K, WIDE>(R, tab, sprev, g, pv);
    for (int r = 0; r < R.n; ++r) {
        load_view<A, K, WIDE>(R, tab, states + (int64_t)r * R.state_bytes, g, cv);
        progress_word<K>(R, pv, cv, vmask, Out{R, counts, events, reward, g, r});
        pv = cv;
    }
}
#endif  // __HIPCC__

}  // namespace ocpg

#endif  // OC_PROGRESS_H_
