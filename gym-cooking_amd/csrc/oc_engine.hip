// oc_engine.hip -- MI355X (gfx950) batched Overcooked step engine + its C-ABI (include/oc_engine.h).
//
// Kernels:
//   oc_step_kernel    one env transition over the batch.  The state is structure-of-arrays byte
//                     planes; a lane owns 4 consecutive envs (one dword per
//                     plane, 256 B per wave-instruction) and steps them as SWAR (oc_swar.h):
//                       pairwise collision resolution  <- check_collisions / is_collision
//                                                         (gym_cooking/envs/overcooked_environment.py:671-762)
//                       sequential per-agent interact  <- execute_navigation + interact
//                                                         (overcooked_environment.py:767-770, utils/interact.py:4-89)
//                       the copy-crash (ERR) condition <- new_obs = copy.copy(self) (:289, :108-113)
//                       done() / reward()              <- overcooked_environment.py:316-376
//                     Tile classes come from a 256-byte LDS table per block; the grid is
//                     persistent and software-pipelined (next chunk's loads before this step).
//   oc_step_n_kernel  n steps per launch with the state in registers; every step's state,
//                     executed actions and collision mask are still written.
//   oc_rollout_kernel navigation-planner rollout rows (oc_rollout.h).
//   oc_bounds_kernel  full-state subtask lower bounds + allocation feasibility (oc_subtask_bounds).
//   oc_render_kernel  image observations.
//   oc_observe_kernel grid feature planes + legal-move masks per env (oc_observe.h).
//   oc_progress_kernel per-subtask object counts, completion events, shaped reward (oc_progress.h).
//   oc_reset_random_kernel randomised episode starts, all envs or the DONE ones (oc_startdist.h).
//   reset / gen_actions / checksum / stats_reduce helpers.
// All of them accumulate nothing on the host; statistics are per-block rows of no-return
// 64-bit atomics reduced by oc_stats_reduce for the all-gather of episode summaries.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/oc_engine.h"
#include "oc_layout.h"
#include "oc_observe.h"
#include "oc_progress.h"
#include "oc_rollout.h"
#include "oc_startdist.h"
#include "oc_stepio.h"
#include "oc_swar.h"

namespace {

using ocly::Planes;  // the state's plane layout (oc_layout.h)
// the step family's chunk, its plane walk, tally and class lookups (oc_stepio.h)
using ocio::Chunk, ocio::kEPL, ocio::NarrowClass, ocio::StepStats, ocio::WideClass;

constexpr int kBlock = 256;  // 4 waves
constexpr int kStepBlock = 128;  // oc_step_kernel: 2 waves
constexpr int kEnvsPerBlock = kBlock * kEPL;

// Kernel argument block: everything static about the level, passed by value (SGPRs).
struct LevelArgs {
    uint32_t cls4[64];    // tile class byte of cell c (ocsw::tile_class) in byte c % 4 of word c / 4;
                          // cells >= W*H (up to 255, 0xFF = dead) read 0; all 0 on a wide level
    int64_t pitch;
    int64_t B;
    ocsw::SwarLevel sw;  // replicated constants / LUTs of the SWAR step
};

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int j) { return (w >> (8 * j)) & 0xFFu; }

// Statistics partial sums, one row of OC_NSTATS uint64 per block.  Wave sum over DPP (VALU
// lane moves, no LDS round trips): an inclusive scan inside each 16-lane row (row_shr 1, 2,
// 4, 8), then row 0's and row 1's totals broadcast into the rows above (row_bcast 15 / 31);
// lane 63 ends with the wave total.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Wave-uniform "some env of the wave": the step's rare-event split (ocsw::step4).
struct WaveAny {
    __device__ __forceinline__ bool operator()(uint32_t v) const { return __ballot(v != 0u) != 0ull; }
};

// Buffer resources of one launch: every plane access is a buffer load/store with the lane's
// 32-bit byte offset in a VGPR and the plane offset (plane * pitch) in an SGPR, so no per-
// access 64-bit address arithmetic is spent on the VALU.
struct Bufs {
    __amdgpu_buffer_rsrc_t sin, sout, act, ex, coll;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, int64_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
template <int CP = 0>
__device__ __forceinline__ uint32_t bld32(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, CP);
}
// Store cache policy (gfx950 CPol bits of the buffer intrinsics): 0 plain, 2 nt, 16 sc1,
// 17 sc0 sc1.  sc1 stores leave no dirty line in the XCD's L2, so the bytes go out to HBM
// while the kernel still computes instead of in the write-back at the kernel boundary (which
// costs about B / 6 TB/s for B dirty bytes, MI355X_MICROARCH.md "boundary").
// oc_step_n, whose trajectory stream is far larger than L2, is faster with nt stores instead
// (tools/stepexp.hip: 4.3 vs 5.2-5.3 us/step at 2^20 envs; sc1 5.3).
constexpr int kCPsc1 = 16, kCPnt = 2;
#ifndef OC_STEP_CP
// oc_step's store policy.  nt measured slower for it (hipGraphs of 20 oc_step launches,
// tools/step_ab.py --per-step, profiles/r04/perstep_nt/: 8.03 vs 8.9-9.5 us/step at A = 2,
// 9.4-9.5 vs 12.0-12.2 at A = 3, same outputs), so oc_step keeps sc1.
#define OC_STEP_CP kCPsc1
#endif
template <int CP = 0>
__device__ __forceinline__ void bst32(__amdgpu_buffer_rsrc_t r, uint32_t v, uint32_t voff, uint32_t soff) {
    __builtin_amdgcn_raw_buffer_store_b32(v, r, (int)voff, (int)soff, CP);
}

// The three step kernels, oc_step_kernel (step_chunk), oc_step_n_kernel and oc_step_wide_kernel,
// keep their own load, store walks, tally, descriptors and statistics flush, written out as they
// were before oc_stepio.h: taking them from shared code (the walks, one descriptor helper, one flush,
// StepStats::add) changed register allocation and schedule although the stores, their order and the
// wait-free loop were the same (oc_step_n_kernel throughout, once with a spill in the loader-wave
// build; four oc_step_kernel builds), and the wide kernel measured 2-3 % slower over them
// (profiles/step_chunk_refactor/).  Their instruction text is equal to the earlier kernels'.  The
// reset kernel and oc_cpu_step use the shared pieces; what must stay in step with them is the plane
// order of ocio::load / ocio::store.
template <int A, int K, bool kActs = true>
__device__ __forceinline__ void load_chunk(Chunk<A, K>& c, const Bufs& b, uint32_t P, uint32_t g) {
    using PL = Planes<A, K, false>;
    const uint32_t vo = g * 4u;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        c.wx[a] = bld32(b.sin, vo, a * P);
        c.wy[a] = bld32(b.sin, vo, (PL::Y + a) * P);
        c.wh[a] = bld32(b.sin, vo, (PL::HOLD + a) * P);
        if (kActs) c.wa[a] = bld32(b.act, vo, a * P);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        c.wl[j] = bld32(b.sin, vo, (PL::LOC + j) * P);
        c.wm[j] = bld32(b.sin, vo, (PL::MASK + j) * P);
    }
    const auto t = __builtin_amdgcn_raw_buffer_load_b64(b.sin, (int)(g * 8u), (int)(PL::T * P), 0);
    c.t0 = t[0];
    c.t1 = t[1];
    c.wf = bld32(b.sin, vo, PL::F * P);
}

// Step the kEPL envs of chunk c (SWAR, oc_swar.h) and store every output plane word of lane g.
template <int A, int K, int CP = 0, int MODE = 1>
__device__ __forceinline__ void step_chunk(const LevelArgs& L, const uint8_t* tbl, Chunk<A, K>& c, const Bufs& b,
                                           bool has_ex, bool has_coll, uint32_t P, uint32_t g, StepStats& st) {
    using PL = Planes<A, K, false>;
    auto cls_of = [tbl](uint32_t cells) -> uint32_t {
        const uint32_t b0 = tbl[cells & 0xFFu], b1 = tbl[(cells >> 8) & 0xFFu], b2 = tbl[(cells >> 16) & 0xFFu],
                       b3 = tbl[cells >> 24];
        return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    };
    const uint32_t f_in = c.wf;
    uint32_t T0 = c.t0, T1 = c.t1, ex[A], cm;
    uint32_t pending = ocsw::at_done80<K, MODE>(L.sw, c.wl);  // a loaded state: the full path once
    const bool full = ocsw::step4<A, K, MODE>(L.sw, c.wx, c.wy, c.wh, c.wl, c.wm, T0, T1, c.wf, c.wa, ex, cm,
                                              cls_of, WaveAny{}, pending);

    // statistics over the valid envs: an episode ended iff DONE is newly set (only on the
    // full path: without a rare event no flag is set)
    const int64_t rem = L.B - (int64_t)g * kEPL;
    const uint32_t vmask = rem >= kEPL ? 0xFFFFFFFFu : (rem <= 0 ? 0u : (1u << (8 * (uint32_t)rem)) - 1u);
    st.coll += __popc(cm & vmask);
    if (full) {
        const uint32_t ended = (c.wf & ~f_in & vmask) & ocsw::k01;  // bit0 per env
        st.eps += __popc(ended);
        st.succ += __popc(c.wf & (ended << 1));
        st.err += __popc(c.wf & (ended << 2));
        const uint32_t efull = (0x80808080u - ended) ^ 0x80808080u;  // 0x01 -> 0xFF per byte, no multiply
        const uint32_t e16a = __builtin_amdgcn_perm(0u, efull, 0x01010000u);  // env 0,1 -> u16 masks
        const uint32_t e16b = __builtin_amdgcn_perm(0u, efull, 0x03030202u);  // env 2,3
        const uint32_t sa = T0 & e16a, sb = T1 & e16b;
        st.steps += (sa & 0xFFFFu) + (sa >> 16) + (sb & 0xFFFFu) + (sb >> 16);
    }

    const uint32_t vo = g * 4u;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        bst32<CP>(b.sout, c.wx[a], vo, a * P);
        bst32<CP>(b.sout, c.wy[a], vo, (PL::Y + a) * P);
        bst32<CP>(b.sout, c.wh[a], vo, (PL::HOLD + a) * P);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        bst32<CP>(b.sout, c.wl[j], vo, (PL::LOC + j) * P);
        bst32<CP>(b.sout, c.wm[j], vo, (PL::MASK + j) * P);
    }
    typedef unsigned int u32x2 __attribute__((__vector_size__(2 * sizeof(unsigned int))));
    const u32x2 tw = {T0, T1};
    __builtin_amdgcn_raw_buffer_store_b64(tw, b.sout, (int)(g * 8u), (int)(PL::T * P), CP);
    bst32<CP>(b.sout, c.wf, vo, PL::F * P);
    if (has_ex) {
#pragma unroll
        for (int a = 0; a < A; ++a) bst32<CP>(b.ex, ex[a], vo, a * P);
    }
    if (has_coll) bst32<CP>(b.coll, cm, vo, 0u);
}

// One step over the batch: one chunk (kEPL envs) per lane, 128-thread blocks, a grid that
// covers the whole batch at once (P / 512 blocks, ~4 waves per SIMD resident at 2^20 envs).
// Each lane issues its chunk's loads first, then the block builds its tile-class table while
// they are in flight.  Measured on MI355X (tools/stepexp.hip, 2^20 envs, hipGraph of 100
// ping-pong steps): 9.1 us/step, against 11.1 for a persistent 2-blocks-per-CU grid with a
// software-pipelined chunk loop (2 chunks per lane at this size: mostly ramp and drain),
// 10.2 with 256-thread blocks, 9.1 with 2 chunks per lane, and 6.5 for the same loads and
// stores with no compute.  Staggering block start times did not help (9.2-9.3).
template <int A, int K, int MODE>
__global__ __launch_bounds__(kStepBlock) void oc_step_kernel(LevelArgs L, const uint8_t* __restrict__ sin,
                                                             uint8_t* __restrict__ sout,
                                                             const uint8_t* __restrict__ actions,
                                                             uint8_t* __restrict__ exec_out,
                                                             uint8_t* __restrict__ coll_out,
                                                             uint64_t* __restrict__ stats, uint32_t stat_rows) {
    const uint32_t P = (uint32_t)L.pitch;  // state <= 2 GiB (checked on the host)
    constexpr int NP = Planes<A, K, false>::NP;
    Bufs b;
    b.sin = make_rsrc(sin, (int64_t)NP * P);
    b.sout = make_rsrc(sout, (int64_t)NP * P);
    b.act = make_rsrc(actions, (int64_t)A * P);
    const bool has_ex = exec_out != nullptr, has_coll = coll_out != nullptr;
    b.ex = make_rsrc(has_ex ? (const void*)exec_out : (const void*)sout, (int64_t)A * P);
    b.coll = make_rsrc(has_coll ? (const void*)coll_out : (const void*)sout, (int64_t)P);
    const uint32_t g = blockIdx.x * (uint32_t)kStepBlock + threadIdx.x;  // grid * kStepBlock == P / kEPL
    Chunk<A, K> c;
    load_chunk<A, K>(c, b, P, g);  // in flight while the block builds its table
    // tile class per cell (bit7 Floor, bit6 Delivery, bit5 Cutboard); cells past the grid read 0.
    // Lane 0 writes the 64 table words from scalar kernel-argument loads (no vector memory
    // access, so nothing waits behind the chunk loads) and the table is published with an
    // LDS-only workgroup fence around the barrier (a plain __syncthreads would also wait for
    // the chunk loads).
    __shared__ uint32_t tbl4[64];
    if (threadIdx.x == 0u) {
#pragma unroll
        for (int i = 0; i < 64; ++i) tbl4[i] = L.cls4[i];
    }
    const uint8_t* tbl = (const uint8_t*)tbl4;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    StepStats st;
    step_chunk<A, K, OC_STEP_CP, MODE>(L, tbl, c, b, has_ex, has_coll, P, g, st);
    if (stats != nullptr) {  // wave sums, then fire-and-forget 64-bit atomics into this block's row
        const uint32_t v[OC_NSTATS] = {wave_sum(st.eps), wave_sum(st.succ), wave_sum(st.steps), wave_sum(st.coll),
                                       wave_sum(st.err)};
        if ((threadIdx.x & 63u) == 0u) {
            unsigned long long* row = (unsigned long long*)stats + (int64_t)(blockIdx.x % stat_rows) * OC_NSTATS;
#pragma unroll
            for (int q = 0; q < OC_NSTATS; ++q)
                if (v[q]) atomicAdd(row + q, (unsigned long long)v[q]);
        }
    }
}

// oc_step_n: n consecutive steps per launch.  Each lane loads its chunk's state once, then
// for every step reads that step's actions (prefetched two steps ahead), steps in registers
// and writes the step's outputs: the full state into traj[r] (when given), the executed
// actions and the collision mask; the state after the last step goes to sout (null when sout
// is the trajectory's last state: that store already wrote it).  Outputs are
// byte-identical to n oc_step launches with ping-pong buffers.
// oc_step_n's completion tickets, after the statistics rows (at a 128-byte boundary, one
// 128-byte line each): [0] counts finished groups, [1 + g] the finished blocks of group g
// (kTicketGroup consecutive blocks).  Every counter is back at zero when a launch ends.
constexpr int kTicketGroup = 32, kTicketStride = 16;  // u64 units
constexpr int64_t kStatRows = 256;  // statistics rows (stats_rows: fewer for small batches)
__host__ __device__ constexpr int64_t ticket_base(int64_t stat_rows) {
    return (stat_rows * OC_NSTATS + kTicketStride - 1) / kTicketStride * kTicketStride;
}

// Loader wave (LW).  A wave that has stores outstanding and consumes a loaded word waits for
// every one of those stores: the compiler emits vmcnt(0) there (loads and stores share the
// counter on gfx950, and it does not take them to complete in order).  With each step's action
// words loaded by the stepping wave, every wave waited at every step for the stores of the step
// before to drain: C3 (3 agents) ran 6.4 us/step, and 5.1 with the action loads taken out of
// the loop (tools/c3_floor.py, profiles/r03/lw/).  With LW, a block has a fifth wave that only
// loads: it fetches the next kLwSteps steps' action words of the block's 256 lanes into one half
// of an LDS ring while the four stepping waves read theirs from the other half, and an
// LDS-only barrier per kLwSteps steps hands the halves over (no vmcnt wait; the stepping waves
// issue no vector load after their state).  Only the loader waits on memory, for loads alone.
// Handing the ring over with per-step LDS flags instead (the loader publishes steps filled,
// each stepping wave the steps it took; a ring of 8 steps, s_sleep polls, no barrier) was
// measured slower: C3 100-step launches 6.28-6.41 us/step against 6.06-6.12 with the barrier,
// four alternating rounds on one box, outputs identical (profiles/r04/lw_flags_ab.jsonl).
#ifndef OC_LW_STEPS
#define OC_LW_STEPS 4
#endif

// Also measured and dropped (round 4, profiles/r04/lw_stagger/): a staggered hand-over, the odd
// stepping waves meeting batch k's barrier between the compute and the stores of step 4k - 1
// (so that at each release the even waves compute while the odd ones store): 6.46-6.51 us/step
// against 6.04-6.07, four alternating rounds on one box, C3 parity tests green on it; and the
// loader's loads as 16-byte loads (16 lanes per 256-byte group, a quarter of the load and LDS
// write instructions): 6.18-6.29 against 6.05-6.12 (profiles/r04/lw_x4/).
constexpr int kLwSteps = OC_LW_STEPS;  // steps per ring half (one barrier per kLwSteps steps)
// A = 3 only: there the stepping waves' drains were a fifth of the time (C3, 100-step launches,
// one box: 6.42 -> 6.07 us/step, outputs identical).  At A <= 2 the step is store-bound and the
// block-wide barrier every kLwSteps steps costs more than the drains (2 agents, 20-step launch:
// 4.60 -> 4.70 us/step; 100-step: 4.20 -> 4.22); A = 4 needs more than 102 VGPRs.
constexpr bool kLoaderWave = true;
template <int A, int K, int MODE>
constexpr bool use_loader_wave() { return kLoaderWave && A == 3 && K == 4; }
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int A, int K, int CP, int LCP, int MODE, bool LW = use_loader_wave<A, K, MODE>()>
__global__ __launch_bounds__(kBlock + (LW ? 64 : 0), LW ? 5 : 1) void oc_step_n_kernel(LevelArgs L, const uint8_t* __restrict__ sin,
                                                           uint8_t* __restrict__ sout,
                                                           const uint8_t* __restrict__ actions,
                                                           uint8_t* __restrict__ traj, uint8_t* __restrict__ exec_out,
                                                           uint8_t* __restrict__ coll_out,
                                                           uint64_t* __restrict__ stats, uint64_t* __restrict__ totals,
                                                           uint32_t stat_rows, int n) {
    __shared__ uint32_t tbl4[64];
    __shared__ uint32_t waves_done;
    __shared__ unsigned long long fold[OC_NSTATS][64 + 8];  // the folding wave's partial sums
    // LW: [half][step of the batch][stepping wave][agent][lane] action words
    __shared__ uint32_t ring[LW ? 2 * kLwSteps * (kBlock / 64) * A * 64 : 1];
    if (threadIdx.x < 64u) tbl4[threadIdx.x] = L.cls4[threadIdx.x];
    if (threadIdx.x == 0u) waves_done = 0u;
    __syncthreads();
    const bool loader = LW && threadIdx.x >= (uint32_t)kBlock;  // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    const uint8_t* tbl = (const uint8_t*)tbl4;
    const uint32_t P = (uint32_t)L.pitch, nlanes = P / kEPL, stride = gridDim.x * (uint32_t)kBlock;
    using PL = Planes<A, K, false>;
    constexpr int NP = PL::NP;
    auto cls_of = [&](uint32_t cells) -> uint32_t {
        const uint32_t b0 = tbl[cells & 0xFFu], b1 = tbl[(cells >> 8) & 0xFFu], b2 = tbl[(cells >> 16) & 0xFFu],
                       b3 = tbl[cells >> 24];
        return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    };
    Bufs b;
    b.sin = make_rsrc(sin, (int64_t)NP * P);
    b.sout = make_rsrc(sout ? (const void*)sout : (const void*)sin, sout ? (int64_t)NP * P : 0);  // null: stores dropped
    b.act = make_rsrc(actions, (int64_t)n * A * P);
    const bool has_tr = traj != nullptr, has_ex = exec_out != nullptr, has_coll = coll_out != nullptr;
    const __amdgpu_buffer_rsrc_t tr = make_rsrc(has_tr ? (const void*)traj : (const void*)sin, has_tr ? (int64_t)n * NP * P : 0);
    b.ex = make_rsrc(has_ex ? (const void*)exec_out : (const void*)sin, has_ex ? (int64_t)n * A * P : 0);
    b.coll = make_rsrc(has_coll ? (const void*)coll_out : (const void*)sin, has_coll ? (int64_t)n * P : 0);
    StepStats st;
    typedef unsigned int u32x2 __attribute__((__vector_size__(2 * sizeof(unsigned int))));
    for (uint32_t gb = blockIdx.x * (uint32_t)kBlock; gb < nlanes; gb += stride) {  // block-uniform
        if (loader) {
            // the action words of steps r0 .. r0 + kLwSteps - 1 (those < n) into ring half h;
            // this wave issues no store, so its waits are for its own loads only
            auto fill = [&](int r0, int h) {
                uint32_t w[kLwSteps][kBlock / 64][A];
#pragma unroll
                for (int q = 0; q < kLwSteps; ++q)
#pragma unroll
                    for (int v = 0; v < kBlock / 64; ++v)
#pragma unroll
                        for (int a = 0; a < A; ++a)
                            w[q][v][a] = r0 + q < n ? bld32<LCP>(b.act, (gb + 64u * v + lane) * 4u,
                                                                 (uint32_t)((r0 + q) * A + a) * P)
                                                    : 0u;
#pragma unroll
                for (int q = 0; q < kLwSteps; ++q)
#pragma unroll
                    for (int v = 0; v < kBlock / 64; ++v)
#pragma unroll
                        for (int a = 0; a < A; ++a)
                            ring[(((h * kLwSteps + q) * (kBlock / 64) + v) * A + a) * 64 + lane] = w[q][v][a];
            };
            fill(0, 0);
            for (int r0 = 0; r0 < n; r0 += kLwSteps) {
                lds_barrier();  // half (r0 / kLwSteps) & 1 is full; the other one has been read
                if (r0 + kLwSteps < n) fill(r0 + kLwSteps, ((r0 / kLwSteps) & 1) ^ 1);
            }
            lds_barrier();  // the chunk's last batch has been read: the next chunk may refill
            continue;
        }
        const uint32_t g = gb + threadIdx.x;
        Chunk<A, K> c;
        load_chunk<A, K, !LW>(c, b, P, g);
        // the state words land before the step loop: waited for at their first use inside the
        // loop, the wait (vmcnt(0) for the last of them) would stay in the loop body and drain
        // every step's stores (an s_waitcnt the compiler's waitcnt pass sees and accounts for)
        if (LW) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt / lgkmcnt untouched
        const uint32_t vo = g * 4u;
        uint32_t T0 = c.t0, T1 = c.t1, nxt[A];
        uint32_t pending = ocsw::at_done80<K, MODE>(L.sw, c.wl);  // the loaded state: the full path once
        const int64_t rem = L.B - (int64_t)g * kEPL;
        const uint32_t vmask = rem >= kEPL ? 0xFFFFFFFFu : (rem <= 0 ? 0u : (1u << (8 * (uint32_t)rem)) - 1u);
        if (!LW) {
#pragma unroll
            for (int a = 0; a < A; ++a) nxt[a] = n > 1 ? bld32<LCP>(b.act, vo, (uint32_t)(A + a) * P) : 0u;
        }
        for (int r = 0; r < n; ++r) {
            uint32_t act[A], ex[A], cm;
            if (LW) {
                const int q = r % kLwSteps;
                if (q == 0) lds_barrier();  // the loader has filled this batch's half
                const int h = (r / kLwSteps) & 1;
#pragma unroll
                for (int a = 0; a < A; ++a)
                    act[a] = ring[(((h * kLwSteps + q) * (kBlock / 64) + (threadIdx.x >> 6)) * A + a) * 64 + lane];
            } else {
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    act[a] = c.wa[a];
                    c.wa[a] = nxt[a];
                }
                if (r + 2 < n) {
#pragma unroll
                    for (int a = 0; a < A; ++a) nxt[a] = bld32<LCP>(b.act, vo, (uint32_t)((r + 2) * A + a) * P);
                }
            }
            const uint32_t f_in = c.wf;
            const bool full = ocsw::step4<A, K, MODE>(L.sw, c.wx, c.wy, c.wh, c.wl, c.wm, T0, T1, c.wf, act, ex,
                                                      cm, cls_of, WaveAny{}, pending);
            st.coll += __popc(cm & vmask);
            if (full) {  // episode ends only on the full path
                const uint32_t ended = (c.wf & ~f_in & vmask) & ocsw::k01;
                st.eps += __popc(ended);
                st.succ += __popc(c.wf & (ended << 1));
                st.err += __popc(c.wf & (ended << 2));
                const uint32_t efull = (0x80808080u - ended) ^ 0x80808080u;  // no multiply
                const uint32_t sa = T0 & __builtin_amdgcn_perm(0u, efull, 0x01010000u);
                const uint32_t sb2 = T1 & __builtin_amdgcn_perm(0u, efull, 0x03030202u);
                st.steps += (sa & 0xFFFFu) + (sa >> 16) + (sb2 & 0xFFFFu) + (sb2 >> 16);
            }
            // Unconditional stores: an absent output's descriptor has num_records 0, so its
            // stores are dropped by the buffer range check.  Guarding them with branches made
            // the waitcnt pass merge a store-free path into the loop back-edge and wait for
            // every store of the step (vmcnt(0)) before taking the next step's action words.
            const uint32_t base = (uint32_t)r * NP * P;
#pragma unroll
            for (int a = 0; a < A; ++a) {
                bst32<CP>(tr, c.wx[a], vo, base + a * P);
                bst32<CP>(tr, c.wy[a], vo, base + (PL::Y + a) * P);
                bst32<CP>(tr, c.wh[a], vo, base + (PL::HOLD + a) * P);
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                bst32<CP>(tr, c.wl[j], vo, base + (PL::LOC + j) * P);
                bst32<CP>(tr, c.wm[j], vo, base + (PL::MASK + j) * P);
            }
            const u32x2 tw = {T0, T1};
            __builtin_amdgcn_raw_buffer_store_b64(tw, tr, (int)(g * 8u), (int)(base + PL::T * P), CP);
            bst32<CP>(tr, c.wf, vo, base + PL::F * P);
#pragma unroll
            for (int a = 0; a < A; ++a) bst32<CP>(b.ex, ex[a], vo, (uint32_t)(r * A + a) * P);
            bst32<CP>(b.coll, cm, vo, (uint32_t)r * P);
        }
        if (LW) lds_barrier();  // pairs with the loader's end-of-chunk barrier
#pragma unroll
        for (int a = 0; a < A; ++a) {
            bst32<CP>(b.sout, c.wx[a], vo, a * P);
            bst32<CP>(b.sout, c.wy[a], vo, (PL::Y + a) * P);
            bst32<CP>(b.sout, c.wh[a], vo, (PL::HOLD + a) * P);
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            bst32<CP>(b.sout, c.wl[j], vo, (PL::LOC + j) * P);
            bst32<CP>(b.sout, c.wm[j], vo, (PL::MASK + j) * P);
        }
        const u32x2 tw = {T0, T1};
        __builtin_amdgcn_raw_buffer_store_b64(tw, b.sout, (int)(g * 8u), (int)(PL::T * P), CP);
        bst32<CP>(b.sout, c.wf, vo, PL::F * P);
    }
    if (loader) return;  // the stepping waves count and fold the statistics
    if (stats != nullptr) {
        const uint32_t v[OC_NSTATS] = {wave_sum(st.eps), wave_sum(st.succ), wave_sum(st.steps), wave_sum(st.coll),
                                       wave_sum(st.err)};
        unsigned long long* const part = (unsigned long long*)stats;
        unsigned long long* const tickets = part + ticket_base(stat_rows);
        uint32_t last = 0u;
        if ((threadIdx.x & 63u) == 0u) {
            unsigned long long* row = part + (int64_t)(blockIdx.x % stat_rows) * OC_NSTATS;
#pragma unroll
            for (int c = 0; c < OC_NSTATS; ++c)
                if (v[c]) atomicAdd(row + c, (unsigned long long)v[c]);
            if (totals != nullptr) {
                // Completion is counted in three levels, so that no counter takes more than
                // kTicketGroup returning atomics (one counter for all 4,096 waves of a 2^20-env
                // launch serialised them at the memory side: ~48 us on a one-step launch).  A
                // wave's adds are performed (vmcnt drained: atomics execute at the memory side,
                // MI355X_MICROARCH.md "Global float atomics") before it counts itself done in
                // LDS; the block's last wave counts the block done in its group, the group's
                // last block counts the group done, and the last group's block folds.
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (atomicAdd(&waves_done, 1u) == (uint32_t)(kBlock / 64) - 1u) {
                    const uint32_t grp = blockIdx.x / (uint32_t)kTicketGroup, ngrp = (gridDim.x + kTicketGroup - 1) / kTicketGroup;
                    const uint32_t gsize = min((uint32_t)kTicketGroup, gridDim.x - grp * (uint32_t)kTicketGroup);
                    unsigned long long* gc = tickets + (int64_t)(1 + grp) * kTicketStride;
                    if ((uint32_t)atomicAdd(gc, 1ull) == gsize - 1u) {
                        atomicExch(gc, 0ull);  // the group's counter ready for the next launch
                        last = (uint32_t)atomicAdd(tickets, 1ull) == ngrp - 1u ? 1u : 0u;
                    }
                }
            }
        }
        if (totals != nullptr && __builtin_amdgcn_readfirstlane((int)last) != 0) {
            // Last wave: fold the partial rows into totals (what oc_stats_reduce does after the
            // launch).  The rows are read with returning atomics, which are served at the memory
            // side, so no XCD's L2 can hand back a stale copy.
            // All of a lane's reads are issued before any is summed (a rolled loop waited for
            // each round's reads before issuing the next), and the 64 lanes' sums are added up
            // in LDS in two rounds of 8 instead of 6 dependent 64-bit shuffle steps per counter.
            const uint32_t lane = threadIdx.x & 63u;
            constexpr int kIt = (int)(kStatRows / 64);
            unsigned long long got[kIt][OC_NSTATS], acc[OC_NSTATS] = {0ull, 0ull, 0ull, 0ull, 0ull};
#pragma unroll
            for (int it = 0; it < kIt; ++it) {  // rows past stat_rows read row 0 again and count 0
                const uint32_t r = lane + 64u * (uint32_t)it, rr = r < stat_rows ? r : 0u;
#pragma unroll
                for (int c = 0; c < OC_NSTATS; ++c) got[it][c] = atomicAdd(part + (int64_t)rr * OC_NSTATS + c, 0ull);
            }
#pragma unroll
            for (int it = 0; it < kIt; ++it)
#pragma unroll
                for (int c = 0; c < OC_NSTATS; ++c)
                    acc[c] += lane + 64u * (uint32_t)it < stat_rows ? got[it][c] : 0ull;
#pragma unroll
            for (int c = 0; c < OC_NSTATS; ++c) fold[c][lane] = acc[c];
            __builtin_amdgcn_wave_barrier();  // LDS is in order within a wave; keep the compiler from moving reads up
            if (lane < 8u * OC_NSTATS) {
                const uint32_t c = lane >> 3, q = lane & 7u;
                unsigned long long v = 0ull;
#pragma unroll
                for (int i = 0; i < 8; ++i) v += fold[c][8u * q + i];
                fold[c][64 + q] = v;
            }
            __builtin_amdgcn_wave_barrier();
            if (lane < (uint32_t)OC_NSTATS) {
                unsigned long long v = 0ull;
#pragma unroll
                for (int i = 0; i < 8; ++i) v += fold[lane][64 + i];
                totals[lane] = v;
            }
            if (lane == 0u) atomicExch(tickets, 0ull);  // ready for the next launch
        }
    }
}

// Planner rollout (oc_rollout): one row per lane, scalar (oc_rollout.h).  Each block stages
// the level's table blob (tile classes, graph nodes, Cutboard / Delivery lists, reachability
// distances: dynamic LDS sized for this level, oc_rollout.h blob_bytes) and the subtask
// configurations in LDS, then walks rows with a grid stride.  Rows are independent;
// byte-plane loads of 64 contiguous bytes per wave instruction.
struct RollArgs {
    ocro::RollLevel L;
    ocro::Sub subs[OC_MAX_SUBTASKS];
    int32_t nsub;
    int32_t blob_words;  // roll.lds_bytes / 4: the whole blob, or (dist_global: a wide level, a narrow
                         // one past kMaxNodes) the tables up to dist_off (distances in device memory)
    int64_t pitch, B;
};

// oc_rollout.h's names of the partner rules' flag values are the documented ones
static_assert(ocro::kTaskCommit == OC_TASK_COMMIT && ocro::kTaskDistinct == OC_TASK_DISTINCT &&
              ocro::kTaskfCompleted == OC_TASKF_COMPLETED && ocro::kTaskfSwitched == OC_TASKF_SWITCHED &&
              ocro::kTaskfReinit == OC_TASKF_REINIT, "oc_rollout.h: task_env's flags");
static_assert(ocro::kTeamCommit == OC_TEAM_COMMIT && ocro::kTeamSplitFirst == OC_TEAM_SPLIT_FIRST &&
              ocro::kTeamOut == OC_TEAM_OUT && ocro::kTeamfCompleted0 == OC_TEAMF_COMPLETED0 &&
              ocro::kTeamfCompleted1 == OC_TEAMF_COMPLETED1 && ocro::kTeamfSwitched == OC_TEAMF_SWITCHED &&
              ocro::kTeamfReinit == OC_TEAMF_REINIT && ocro::kTeamfJoint == OC_TEAMF_JOINT &&
              ocro::kTeamfIdle == OC_TEAMF_IDLE, "oc_rollout.h: team_env's flags");
static_assert(ocro::kBelfUpdated == OC_BELF_UPDATED && ocro::kBelfPruned == OC_BELF_PRUNED &&
              ocro::kBelfReinit == OC_BELF_REINIT && ocro::kBelfReset == OC_BELF_RESET &&
              ocro::kBelfRaised == OC_BELF_RAISED, "oc_rollout.h: belief_env's flags");
static_assert(ocro::kTbelfUpdated == OC_TBELF_UPDATED && ocro::kTbelfPruned == OC_TBELF_PRUNED &&
              ocro::kTbelfReinit == OC_TBELF_REINIT && ocro::kTbelfReset == OC_TBELF_RESET &&
              ocro::kTbelfRaised == OC_TBELF_RAISED && ocro::kTbelfEmpty == OC_TBELF_EMPTY &&
              ocro::kTbelfJoint == OC_TBELF_JOINT && ocro::kTeamMaxSubtasks == OC_TEAM_MAX_SUBTASKS,
              "oc_rollout.h: team_belief_env's flags");

// Stage the level's table blob and the subtask configurations in LDS.
template <int NT = kBlock>
__device__ __forceinline__ void stage_roll_tables(const RollArgs& R, const uint8_t* blob_g, uint32_t* blob_w,
                                                  ocro::Sub* subs) {
    // 16-byte loads (a quarter of the load instructions; round 6), then the last < 4 words
    const int n16 = R.blob_words >> 2;
    for (int i = threadIdx.x; i < n16; i += NT) ((uint4*)blob_w)[i] = ((const uint4*)blob_g)[i];
    for (int i = 4 * n16 + threadIdx.x; i < R.blob_words; i += NT) blob_w[i] = ((const uint32_t*)blob_g)[i];
    constexpr int kSubWords = (int)(sizeof(ocro::Sub) / 4);
    for (int i = threadIdx.x; i < R.nsub * kSubWords; i += NT)
        ((uint32_t*)subs)[i] = ((const uint32_t*)R.subs)[i];
    __syncthreads();
}

template <int A, int K, bool W = false>
__host__ __device__ __forceinline__ ocro::RowT<K, W> load_row(const uint8_t* __restrict__ sin, int64_t P, int64_t e) {
    using PL = Planes<A, K, W>;
    using Row = ocro::RowT<K, W>;
    Row r;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        r.x |= (uint32_t)sin[a * P + e] << (8 * a);
        r.y |= (uint32_t)sin[(PL::Y + a) * P + e] << (8 * a);
        r.h |= (uint32_t)sin[(PL::HOLD + a) * P + e] << (8 * a);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        uint64_t c = sin[(PL::LOC + j) * P + e];
        if (W) c |= (uint64_t)sin[(PL::LOC_HI + j) * P + e] << 8;
        r.loc[j / Row::LPW] |= c << (Row::kLocBits * (j % Row::LPW));
        r.mask[j >> 3] |= (uint64_t)sin[(PL::MASK + j) * P + e] << (8 * (j & 7));
    }
    return r;
}

// The agent-pair table (device memory; L.pair_off), or none: a level without one.
__device__ __forceinline__ const uint32_t* pair_table_of(const RollArgs& R, const uint8_t* blob_g) {
    return R.L.pair_off != 0 ? (const uint32_t*)(blob_g + R.L.pair_off) : nullptr;
}

// A planner kernel's row operations over the staged tables `blob` (LDS) and the level's whole
// blob `blob_g` (device memory).  pair_table: the bounds read the agent-pair table.
template <int A, int K, bool W, bool LEAN, bool GD>
__device__ __forceinline__ ocro::RowOps<A, K, W, LEAN, GD> plan_ops(const RollArgs& R, const uint8_t* blob,
                                                                    const uint8_t* blob_g, bool pair_table) {
    ocro::RowOps<A, K, W, LEAN, GD> ops(R.L, blob, GD ? blob_g + R.L.dist_off : blob + R.L.dist_off);  // distances: LDS (narrow), device memory (wide)
    if (pair_table) ops.PT = pair_table_of(R, blob_g);
    return ops;
}

// An env's partner state starts over: the call says so, or state_prev (where given) shows that the
// env's episode ended.
template <int A, int K, bool W>
__host__ __device__ __forceinline__ bool starts_over(bool init_flag, const uint8_t* sprev, int64_t P, int64_t e) {
    return init_flag || (sprev != nullptr && (sprev[Planes<A, K, W>::F * P + e] & OC_FLAG_DONE) != 0);
}

// the row's agent and item planes (t and flags are the caller's).  NT: non-temporal stores
// (the rollout's outputs: 11.39-11.43 against 11.47-11.55 us per C5 launch; the bounds kernel's
// outputs stored that way were slower, 0.095 against 0.091 ms, profiles/r05/ab/ab_nt_stores.jsonl)
template <int A, int K, bool W = false, bool NT = false>
__device__ __forceinline__ void store_row(uint8_t* __restrict__ sout, int64_t P, int64_t e, const ocro::RowT<K, W>& r) {
    using PL = Planes<A, K, W>;
    auto st = [&](int64_t i, uint32_t v) {
        if constexpr (NT) __builtin_nontemporal_store((uint8_t)v, sout + i);
        else sout[i] = (uint8_t)v;
    };
#pragma unroll
    for (int a = 0; a < A; ++a) {
        st(a * P + e, (uint32_t)r.ax(a));
        st((PL::Y + a) * P + e, (uint32_t)r.ay(a));
        st((PL::HOLD + a) * P + e, (uint32_t)r.ah(a));
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t c = (uint32_t)r.il(j);
        st((PL::LOC + j) * P + e, c);
        if (W) st((PL::LOC_HI + j) * P + e, c >> 8);
        st((PL::MASK + j) * P + e, (uint32_t)r.im(j));
    }
}

#ifndef OC_ROLL_BLOCK
#define OC_ROLL_BLOCK 256
#endif
// The agent-pair table (oc_rollout.h pair_off: the two-agent bound's per-type minima, device
// memory) in the rollout kernels: 2^18 rows 11.35-11.40 -> 10.78-10.83 us, 4,096 rows unchanged;
// in the likelihood kernels 188-192 -> 193-195 us, so off there (profiles/r06/pass_z); the bounds
// kernel always reads it (85 -> 70 us, pass_y).  Every output byte identical.
#ifndef OC_PT_LIK
#define OC_PT_LIK 0
#endif
#ifndef OC_PT_ROLL
#define OC_PT_ROLL 1
#endif
#ifndef OC_ROLL_GROUP
#define OC_ROLL_GROUP 4
#endif
// The rollout kernel's block (one row per lane).  512- and 1,024-lane blocks (fewer blocks to
// dispatch, each staging the tables with more lanes) measured slower at C5: 12.0-12.3 and
// 12.2-12.4 us against 11.6 (profiles/r05/ab/ab_merge_pairs_blocks.jsonl).  One-wave blocks for
// launches under 16 Ki rows (the planner's 4,096-row launches on 64 CUs instead of 16) were
// slower too: 6.79-6.81 against 5.98-5.99 us for 4,096 rows, 11.28-11.37 against 11.32-11.37 at
// 2^18 (profiles/r06/pass_b/ab_roll_small.jsonl, round 6): a block's table staging by one wave
// takes four times as many load rounds, and that staging is on every row's critical path.
constexpr int kRollBlock = OC_ROLL_BLOCK;
template <int A, int K, bool W, bool GD>
__global__ __launch_bounds__(kRollBlock) void oc_rollout_kernel(RollArgs R, const uint8_t* __restrict__ sin,
                                                            uint8_t* __restrict__ sout,
                                                            const uint8_t* __restrict__ act,
                                                            const uint8_t* __restrict__ alloc,
                                                            const uint8_t* __restrict__ blob_g,
                                                            uint8_t* __restrict__ out_flags,
                                                            float* __restrict__ lb) {
    extern __shared__ __attribute__((aligned(16))) uint32_t blob_w[];
    __shared__ ocro::Sub subs[OC_MAX_SUBTASKS];
    const int64_t P = R.pitch;
    using PL = Planes<A, K, W>;
    // A lane's row: its state, t, flags, allocation id and every agent's action (the subtask's
    // agents are known only once the configuration table is in LDS).  The first row's loads are
    // issued before the table staging, so their latency overlaps it (round 6).
    struct In {
        ocro::RowT<K, W> r;
        uint16_t t;
        uint8_t fl;
        int ai;
        uint32_t acts;  // agent a's action in byte a
    };
    auto load_in = [&](int64_t e) {
        In v;
        v.r = load_row<A, K, W>(sin, P, e);
        v.t = ((const uint16_t*)(sin + PL::T * P))[e];
        v.fl = sin[PL::F * P + e];
        v.ai = alloc != nullptr ? alloc[e] : 0;
        v.acts = 0u;
#pragma unroll
        for (int a = 0; a < A; ++a) v.acts |= (uint32_t)act[a * P + e] << (8 * a);
        return v;
    };
    int64_t e = blockIdx.x * (int64_t)kRollBlock + threadIdx.x;
    In in;
    if (e < R.B) in = load_in(e);
    stage_roll_tables<kRollBlock>(R, blob_g, blob_w, subs);
    const uint8_t* blob = (const uint8_t*)blob_w;
    for (bool first = true; e < R.B; e += (int64_t)gridDim.x * kRollBlock, first = false) {
        if (!first) in = load_in(e);
        ocro::RowT<K, W> r = in.r;
        const uint16_t t = in.t;
        const uint8_t fl_in = in.fl;
        const int ai = in.ai;
        float bound = 0.0f;
        int f = OC_ROLL_BADALLOC;  // an alloc id past num_subtasks: the row is copied unchanged
        if (ai < R.nsub) {
            const ocro::Sub& s = subs[ai];
            const int c0 = (in.acts >> (8 * s.agent[0])) & 0xFFu, c1 = s.n == 2 ? (in.acts >> (8 * s.agent[1])) & 0xFFu : ocro::kNoop;
            auto ops = plan_ops<A, K, W, false, GD>(R, blob, blob_g, OC_PT_ROLL);
            f = ops.run(r, s, c0, c1, bound);
        }
        store_row<A, K, W, true>(sout, P, e, r);
        __builtin_nontemporal_store(t, (uint16_t*)(sout + PL::T * P) + e);
        __builtin_nontemporal_store(fl_in, sout + PL::F * P + e);
        __builtin_nontemporal_store((uint8_t)f, out_flags + e);
        __builtin_nontemporal_store(bound, lb + e);
    }
}

// Lane-group rollout rows (round 6), for launches that fit one round of blocks with G lanes per
// row: the planner's own launches (<= 4,096 rows), where the launch lasts as long as its slowest
// wave's row chain.  The G lanes of a group run one row together: every lane builds the Level-0
// view and runs legality, interact and the goal test (one chain), and the lower bound -- the
// longest phase (2.4 of the 8.8 us of a 4,096-row launch, tools/rollx.hip ablations) -- splits
// its approach walks: lane q takes A approach q * 4 / G .. (one-agent rows and the static Chop /
// Deliver side) or B square q & 1 of each Merge pair (two agents, whose per-type minima need both
// sides whole).  The group's minima meet by DPP swaps inside a quad; lane 0 stores.  4,096 rows:
// 8.91 us one row per lane, 7.96 lane pairs, 7.76 lane quads; splitting a two-agent row's
// legality by agent as well, 8.02 / 7.82 (profiles/r06/pass_n/rollx.log).  Narrow levels with LDS
// distances only (every kitchen the reference ships); the others keep one row per lane.
constexpr int kRollGroup = OC_ROLL_GROUP;
template <int G>
__device__ __forceinline__ float group_min(float v) {
    static_assert(G == 2 || G == 4, "lane groups of 2 or 4");
    int o = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
    v = __int_as_float(o) < v ? __int_as_float(o) : v;
    if (G == 4) {
        o = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
        v = __int_as_float(o) < v ? __int_as_float(o) : v;
    }
    return v;
}
template <int G, int A, int K>
struct GroupRowOps : ocro::RowOps<A, K> {
    using Base = ocro::RowOps<A, K>;
    using typename Base::Row;
    using typename Base::Target;
    using Base::L;
    using Base::T;
    static constexpr int NA = 4 / G;  // A approaches per lane when the walk takes four
    int q;                            // this lane's index in its group
    __device__ GroupRowOps(const ocro::RollLevel& l, const uint8_t* blob, int lane) : Base(l, blob), q(lane) {}
    __device__ int approach(bool four, int k) const { return four ? NA * q + k : 0; }

    // Base::helper_static over this lane's A approaches
    __device__ float helper_static(const ocro::Sub& s, int u0, int u1, int Ac, int nb, int side, const uint16_t* man_t) const {
        const float per = (float)L.perimeter;
        float lower = per + 1.0f;
        if (nb == 0) return lower;
        int vAs[4];
        const bool four = ocro::wave_any(this->approaches(Ac, vAs));
        if (s.n == 1) {
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                const int vA = vAs[approach(four, k)];
                const int a1 = this->dn(u0, vA), m = this->dmin(side, vA);
                const float bound = (float)(a1 + m - 1);
                lower = vA != ocro::kNoNode && a1 >= 0 && m >= 0 && bound < lower ? bound : lower;
                if (!four) break;  // wave-uniform: a Floor square's one node
            }
        } else {
            const int man = man_t[Ac];
            float mA = per;
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                const int vA = vAs[approach(four, k)];
                int t;
                const float b1A = (t = this->dn(u0, vA)) < 0 ? per : (float)t;
                const float b2A = (t = this->dn(u1, vA)) < 0 ? per : (float)t;
                const float m2 = b1A < b2A ? b1A : b2A;
                mA = m2 < mA ? m2 : mA;
                if (!four) break;
            }
            const float bound = mA + (float)man - 1.0f;
            if (bound < lower) lower = bound;
        }
        return lower > 1.0f ? lower : 1.0f;
    }
    // Base::helper_n<2>(Ac, {B1, B2}): one agent, this lane's A approaches (the node-to-square
    // table when the level has one); two agents, B square q & 1
    __device__ float helper_pair(const ocro::Sub& s, int u0, int u1, int Ac, int B1, int B2) const {
        if (s.n == 1 && L.sq_off != 0) {
            float lower = (float)L.perimeter + 1.0f;
            int vA[4];
            const bool four = ocro::wave_any(this->approaches(Ac, vA));
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                const int v = vA[approach(four, k)];
                const int a1 = this->dn(u0, v), b1 = this->dsq(v, B1), b2 = this->dsq(v, B2);
                const float x1 = (float)(a1 + b1 - 1), x2 = (float)(a1 + b2 - 1);
                lower = a1 >= 0 && b1 >= 0 && x1 < lower ? x1 : lower;
                lower = a1 >= 0 && b2 >= 0 && x2 < lower ? x2 : lower;
                if (!four) break;
            }
            return lower > 1.0f ? lower : 1.0f;
        }
        const int Bc[1] = {(q & 1) ? B2 : B1};
        return this->template helper_n<1>(s, u0, u1, Ac, Bc);
    }
    // Base::lower_bound with the walks split; the group's min (the clamps are monotone)
    __device__ float lower_bound(const Row& r, const ocro::Sub& s) const {
        const auto br = this->template bound_row<false>(r);
        int u0, u1;
        float pen;
        this->template bound_agents<false>(br, s, u0, u1, pen);
        float lower = (float)L.perimeter + 1.0f;
        if (s.kind == 1 || s.kind == 3) {
            const int nb = s.kind == 1 ? L.ncut : L.ndeliv;
            const int side = s.kind == 1 ? 0 : 1;
            const uint16_t* man_t = (const uint16_t*)(T + L.man_off) + (s.kind == 1 ? 0 : L.man_stride);
            this->template visit_objs<false>(br, r, s.start[0], s.kind == 3, [&](int Ac) {
                const float b = helper_static(s, u0, u1, Ac, nb, side, man_t);
                if (b < lower) lower = b;
            });
        } else if (s.kind == 2) {
            this->template visit_objs<false>(br, r, s.start[0], false, [&](int Ac) {
                this->template visit_obj_pairs<false>(br, r, s.start[1], false, [&](int B1, int B2) {
                    const float b = helper_pair(s, u0, u1, Ac, B1, B2);
                    if (b < lower) lower = b;
                });
            });
        }
        return group_min<G>(lower) + pen;
    }
    // Base::run
    __device__ int run(Row& r, const ocro::Sub& s, int c0, int c1, float& lb) {
        const Row r_in = r;
        if (this->level0(r, s)) {
            r = r_in;
            lb = 0.0f;
            return 8;  // OC_ROLL_RAISES
        }
        if (s.kind == 0) c0 = c1 = ocro::kNoop;
        c0 = c0 > ocro::kNoop ? ocro::kNoop : c0;
        c1 = c1 > ocro::kNoop ? ocro::kNoop : c1;
        const Target g0 = this->target(r, s.agent[0], c0), g1 = s.n == 2 ? this->target(r, s.agent[1], c1) : g0;
        int fl = this->action_legal(r, s, c0, c1, g0, g1) ? 1 : 0;
        this->interact(r, s.agent[0], c0, g0);
        if (s.n == 2) this->interact(r, s.agent[1], c1, g1);
        const bool asserted = s.n == 2 && this->agent_cell(r, s.agent[0]) == this->agent_cell(r, s.agent[1]);
        if (asserted) fl |= 4;
        else if (this->is_goal(r, s)) fl |= 2;
        lb = lower_bound(r, s);
        return fl;
    }
};
// One round of blocks: G * B <= the grid's lanes (oc_rollout checks), so no grid-stride loop.
template <int A, int K>
__global__ __launch_bounds__(kRollBlock) void oc_rollout_group_kernel(RollArgs R, const uint8_t* __restrict__ sin,
                                                                  uint8_t* __restrict__ sout,
                                                                  const uint8_t* __restrict__ act,
                                                                  const uint8_t* __restrict__ alloc,
                                                                  const uint8_t* __restrict__ blob_g,
                                                                  uint8_t* __restrict__ out_flags,
                                                                  float* __restrict__ lb) {
    constexpr int G = kRollGroup;
    extern __shared__ __attribute__((aligned(16))) uint32_t blob_w[];
    __shared__ ocro::Sub subs[OC_MAX_SUBTASKS];
    const int64_t P = R.pitch;
    using PL = Planes<A, K, false>;
    const int q = (int)(threadIdx.x & (G - 1));
    const int64_t e = (blockIdx.x * (int64_t)kRollBlock + threadIdx.x) / G;
    const bool live = e < R.B;  // whole groups: B ends on a group boundary
    ocro::RowT<K> r;
    uint16_t t = 0;
    uint8_t fl_in = 0;
    int ai = 0;
    uint32_t acts = 0;
    if (live) {  // every lane of the group loads the row (the same bytes: one transaction)
        r = load_row<A, K>(sin, P, e);
        t = ((const uint16_t*)(sin + PL::T * P))[e];
        fl_in = sin[PL::F * P + e];
        ai = alloc != nullptr ? alloc[e] : 0;
#pragma unroll
        for (int a = 0; a < A; ++a) acts |= (uint32_t)act[a * P + e] << (8 * a);
    }
    stage_roll_tables<kRollBlock>(R, blob_g, blob_w, subs);
    if (!live) return;
    float bound = 0.0f;
    int f = OC_ROLL_BADALLOC;
    if (ai < R.nsub) {
        const ocro::Sub& s = subs[ai];
        const int c0 = (acts >> (8 * s.agent[0])) & 0xFFu, c1 = s.n == 2 ? (acts >> (8 * s.agent[1])) & 0xFFu : ocro::kNoop;
        GroupRowOps<G, A, K> ops(R.L, (const uint8_t*)blob_w, q);
        if (OC_PT_ROLL) ops.PT = pair_table_of(R, blob_g);
        f = ops.run(r, s, c0, c1, bound);
    }
    if (q == 0) {
        store_row<A, K, false, true>(sout, P, e, r);
        __builtin_nontemporal_store(t, (uint16_t*)(sout + PL::T * P) + e);
        __builtin_nontemporal_store(fl_in, sout + PL::F * P + e);
        __builtin_nontemporal_store((uint8_t)f, out_flags + e);
        __builtin_nontemporal_store(bound, lb + e);
    }
}

// Bayesian-delegation likelihood (oc_nav_likelihood): a group of G lanes per row; candidate
// action k (k = a0 for one subtask agent, a0*5 + a1 for two: the reference's loop order,
// bayesian_delegator.py:676-689) belongs to lane k % G, slot k / G (32 / G slots per lane).  Every
// lane of a group builds the row's Level-0 view, tests its candidates' legality and evaluates
// Q(s, k) with one rollout (interact + goal + lower bound) for each legal candidate and for
// the taken action.  The group then takes Q(s, taken) from the taken action's lane, the max of
// x = beta * (Q(s, taken) - Q(s, k)) over the legal candidates (a butterfly max: order-free),
// exp(x - max) per candidate, and the softmax sum over k in ascending order (every lane adds
// the group's terms in that order, so the sum is the sequential one bit for bit).  A lane
// walking all candidates of its row kept 22 % of the lanes active per VALU instruction
// (profiles/r02/c5_grouped); spreading them over the group leaves the candidates' own path
// differences.  G = 32 (one candidate per lane) when the call's table has a two-agent
// configuration; G = 8 when every configuration has one agent (5 candidates: a 32-lane group
// would idle 27 lanes).  Measured on the C5 rows (profiles/r02/c5_order_probe.json): G = 32
// 0.35 ms configuration-major, 0.55 ms random order, against 0.44 / 1.29 ms with G = 8; a
// one-agent table 0.19 ms with G = 8, 0.41 with G = 32.  The None subtask's closed form runs
// on the group's first lane.
template <int A, int K, int G, bool W, bool GD>
__global__ __launch_bounds__(kBlock) void oc_likelihood_kernel(RollArgs R, const uint8_t* __restrict__ sin,
                                                               const uint8_t* __restrict__ taken_p,
                                                               const uint8_t* __restrict__ alloc,
                                                               const uint8_t* __restrict__ blob_g, int self_agent,
                                                               double beta, double nap, double* __restrict__ out,
                                                               uint8_t* __restrict__ out_flags) {
    extern __shared__ __attribute__((aligned(16))) uint32_t blob_w[];
    __shared__ ocro::Sub subs[OC_MAX_SUBTASKS];
    stage_roll_tables(R, blob_g, blob_w, subs);
    const uint8_t* blob = (const uint8_t*)blob_w;
    const int64_t P = R.pitch;
    constexpr int kLikGroup = G, kLikSlots = 32 / G;  // G x slots >= 25 candidates
    const int lane = (int)(threadIdx.x & (kLikGroup - 1));
    const int64_t ngroups = (int64_t)gridDim.x * (kBlock / kLikGroup);
    for (int64_t e = (int64_t)blockIdx.x * (kBlock / kLikGroup) + threadIdx.x / kLikGroup; e < R.B; e += ngroups) {
        const int ai = alloc != nullptr ? alloc[e] : 0;  // group-uniform from here on
        double v = 0.0;
        int f = OC_LIK_BADALLOC;
        if (ai < R.nsub) {
            const ocro::Sub& s = subs[ai];
            ocro::RowT<K, W> r = load_row<A, K, W>(sin, P, e);
            uint32_t taken = 0;
#pragma unroll
            for (int a = 0; a < A; ++a) taken |= (uint32_t)taken_p[a * P + e] << (8 * a);
            auto ops = plan_ops<A, K, W, true, GD>(R, blob, blob_g, OC_PT_LIK);
            if (s.kind == 0) {
                f = 0;
                if (lane == 0) f = ops.likelihood(r, s, taken, self_agent, beta, nap, v);
            } else if (ops.level0(r, s)) {
                f = OC_LIK_RAISES;  // two removed agents on one square
            } else {
                const bool joint = s.n == 2;
                int t0 = (int)((taken >> (8 * s.agent[0])) & 0xFFu), t1 = ocro::kNoop;
                if (joint) t1 = (int)((taken >> (8 * s.agent[1])) & 0xFFu);
                t0 = t0 > ocro::kNoop ? ocro::kNoop : t0;
                t1 = t1 > ocro::kNoop ? ocro::kNoop : t1;
                const int ncand = joint ? 25 : 5, kt = joint ? t0 * 5 + t1 : t0;
                const int other = joint ? (s.agent[0] == self_agent ? 1 : (s.agent[1] == self_agent ? 0 : -1)) : -1;
                double q[kLikSlots], ex[kLikSlots];
                bool legal[kLikSlots];
                int bad = 0, taken_ok = 0;
                double qt = 0.0;
                // candidate k's legality and Q (one rollout when legal or taken)
                auto eval = [&](int k, double& qj, bool& lg) OC_RL {
                    const int a0 = joint ? k / 5 : k, c1 = joint ? k % 5 : ocro::kNoop;
                    lg = k < ncand && ops.action_legal(r, s, a0, c1);
                    if (other == 0 && a0 != t0) lg = false;
                    if (other == 1 && c1 != t1) lg = false;
                    qj = 0.0;
                    bool ok = true;
                    if (lg || k == kt) ok = ops.q_value(r, s, a0, c1, qj);
                    bad |= (int)(lg && !ok);
                    if (k == kt) {
                        qt = qj;
                        taken_ok = (int)(ok && lg);
                    }
                };
                if constexpr (kLikSlots == 1) {
                    eval(lane, q[0], legal[0]);
                } else {
                    // one rolled loop, one rollout call site (the row code is large); its results
                    // go to the slot registers by static selects (no scratch)
#pragma unroll 1
                    for (int j = 0; j < kLikSlots; ++j) {
                        double qj;
                        bool lg;
                        eval(lane + kLikGroup * j, qj, lg);
#pragma unroll
                        for (int i = 0; i < kLikSlots; ++i)
                            if (i == j) {
                                q[i] = qj;
                                legal[i] = lg;
                            }
                    }
                }
                // Q(s, taken) and its legality from the taken action's lane; the row raises when
                // that rollout or any legal candidate's rollout hits the co-location assert, or
                // when the taken action is not among get_actions
                const double old_q = __shfl(qt, kt % kLikGroup, kLikGroup);
                taken_ok = __shfl(taken_ok, kt % kLikGroup, kLikGroup);
#pragma unroll
                for (int off = 1; off < kLikGroup; off <<= 1) bad |= __shfl_xor(bad, off, kLikGroup);
                if (!taken_ok || bad) {
                    f = OC_LIK_RAISES;
                } else {
                    double m = -1.0e300;
#pragma unroll
                    for (int j = 0; j < kLikSlots; ++j) {
                        q[j] = legal[j] ? beta * (old_q - q[j]) : -1.0e300;  // q now holds x
                        m = q[j] > m ? q[j] : m;
                    }
#pragma unroll
                    for (int off = 1; off < kLikGroup; off <<= 1) {
                        const double o = __shfl_xor(m, off, kLikGroup);
                        m = o > m ? o : m;
                    }
                    double et = 0.0;
#pragma unroll
                    for (int j = 0; j < kLikSlots; ++j) {
                        ex[j] = legal[j] ? exp(q[j] - m) : 0.0;
                        if (lane + kLikGroup * j == kt) et = ex[j];
                    }
                    double S = 0.0;  // ascending k = 8 j + c: the reference's summation order
#pragma unroll
                    for (int j = 0; j < kLikSlots; ++j)
                        for (int c = 0; c < kLikGroup && kLikGroup * j + c < ncand; ++c) S += __shfl(ex[j], c, kLikGroup);
                    v = __shfl(et, kt % kLikGroup, kLikGroup) / S;
                    f = OC_LIK_OK;
                }
            }
        }
        if (lane == 0) {
            out[e] = f == OC_LIK_OK ? v : 0.0;
            out_flags[e] = (uint8_t)f;
        }
    }
}

// Subtask-following actions (oc_nav_policy): the generative side of the likelihood's agent model,
// a sibling of oc_likelihood_kernel.  A group of G lanes per row, candidate k on lane k (G = 8
// when every configuration has one agent: 5 candidates; G = 32 when one has two: 25): every lane
// builds the row's Level-0 view, tests its candidate's legality and evaluates Q(s, k) with one
// rollout when it is legal.  The group takes the min of Q (a butterfly: order-free), w_k =
// exp(beta * (min - Q_k)) per lane, the sum of w in ascending k (every lane adds the group's
// terms in that order: the sequential sum bit for bit) and p_k = w_k / S.  The draw walks the
// p_k in ascending k as shuffles (every lane the same running sum); greedy is the lowest lane
// whose Q is the min.  The None subtask's closed form is evaluated by every lane (four legality
// tests, no rollout).  Lane k stores plane k of probs; the group's first lane stores the flags
// and the subtask agents' action bytes (byte stores: the other agents' bytes stay).
struct PolicyArgs {
    double beta, nap;
    int64_t env_offset, step;
    uint64_t seed;
    int32_t mode, num_cand;
};
template <int A, int K, int G, bool W, bool GD>
__global__ __launch_bounds__(kBlock) void oc_policy_kernel(RollArgs R, PolicyArgs Q, const uint8_t* __restrict__ sin,
                                                           const uint8_t* __restrict__ alloc,
                                                           const uint8_t* __restrict__ blob_g,
                                                           uint8_t* __restrict__ actions, double* __restrict__ probs,
                                                           uint8_t* __restrict__ out_flags) {
    extern __shared__ __attribute__((aligned(16))) uint32_t blob_w[];
    __shared__ ocro::Sub subs[OC_MAX_SUBTASKS];
    stage_roll_tables(R, blob_g, blob_w, subs);
    const uint8_t* blob = (const uint8_t*)blob_w;
    const int64_t P = R.pitch;
    const int lane = (int)(threadIdx.x & (G - 1));
    const int64_t ngroups = (int64_t)gridDim.x * (kBlock / G);
    for (int64_t e = (int64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G; e < R.B; e += ngroups) {
        const int ai = alloc != nullptr ? alloc[e] : 0;  // group-uniform from here on
        int f = OC_POL_BADALLOC;
        double p = 0.0;  // p_k of this lane's candidate
        int pick = 0, ag0 = 0, ag1 = 0;
        bool joint = false;
        if (ai < R.nsub) {
            const ocro::Sub& s = subs[ai];
            ag0 = s.agent[0];
            ag1 = s.agent[1];
            joint = s.n == 2;
            const int ncand = joint ? 25 : 5;
            ocro::RowT<K, W> r = load_row<A, K, W>(sin, P, e);
            auto ops = plan_ops<A, K, W, true, GD>(R, blob, blob_g, OC_PT_LIK);
            bool lg = false;    // this lane's candidate is legal
            bool best = false;  // ... and its Q is the row's min (None: it is the mode)
            f = OC_POL_RAISES;
            if (s.kind == 0) {
                if (!joint) {
                    const uint32_t mv = ops.none_movable(r, ag0);
                    double p0, p1;
                    bool noop_mode;
                    ops.none_probs(__builtin_popcount(mv), Q.beta, Q.nap, p0, p1, noop_mode);
                    lg = lane == ocro::kNoop || (lane < ocro::kNoop && ((mv >> lane) & 1u));
                    p = lane == ocro::kNoop ? p0 : (lg ? p1 : 0.0);
                    best = lg && (lane == ocro::kNoop) == noop_mode;
                    f = OC_POL_OK;
                }
            } else if (!ops.level0(r, s)) {
                const int count = Q.mode & OC_POLICY_COUNT_STATE ? ops.goal_objects(r, s) : (int)s.count;
                const int c0 = joint ? lane / 5 : lane, c1 = joint ? lane % 5 : ocro::kNoop;
                lg = lane < ncand && ops.action_legal(r, s, c0, c1);
                double q = 0.0;
                int bad = 0, any = (int)lg;
                if (lg) bad = (int)!ops.q_value_count(r, s, c0, c1, count, q);
                double m = lg ? q : 1.0e300;
#pragma unroll
                for (int off = 1; off < G; off <<= 1) {
                    bad |= __shfl_xor(bad, off, G);
                    any |= __shfl_xor(any, off, G);
                    const double o = __shfl_xor(m, off, G);
                    m = o < m ? o : m;
                }
                if (any && !bad) {
                    const double w = lg ? exp(Q.beta * (m - q)) : 0.0;
                    double S = 0.0;  // ascending k: the sequential sum
                    for (int c = 0; c < ncand; ++c) S += __shfl(w, c, G);
                    p = w / S;
                    best = lg && q == m;
                    f = OC_POL_OK;
                }
            }
            if (f == OC_POL_OK) {
                if (Q.mode & OC_POLICY_GREEDY) {
                    pick = best ? lane : 31;  // the lowest lane at the min
#pragma unroll
                    for (int off = 1; off < G; off <<= 1) {
                        const int o = __shfl_xor(pick, off, G);
                        pick = o < pick ? o : pick;
                    }
                } else {
                    // the draw on the stored p: running sum in ascending k, the first k past u;
                    // else (rounding) the highest legal k
                    const double u = ocro::policy_u(Q.seed, Q.env_offset + e, Q.step, ag0);
                    double c = 0.0;
                    int hi = 0;
                    pick = -1;
                    for (int k = 0; k < ncand; ++k) {
                        c += __shfl(p, k, G);
                        hi = __shfl((int)lg, k, G) ? k : hi;
                        pick = pick < 0 && u < c ? k : pick;
                    }
                    pick = pick < 0 ? hi : pick;
                }
            } else {
                p = 0.0;
                pick = joint ? 5 * ocro::kNoop + ocro::kNoop : ocro::kNoop;
            }
        }
        if (probs != nullptr)
            for (int k = lane; k < Q.num_cand; k += G) probs[k * P + e] = k == lane ? p : 0.0;
        if (lane == 0) {
            if (f != OC_POL_BADALLOC) {
                actions[ag0 * P + e] = (uint8_t)(joint ? pick / 5 : pick);
                if (joint) actions[ag1 * P + e] = (uint8_t)(pick % 5);
            }
            out_flags[e] = (uint8_t)f;
        }
    }
}

// Full-state subtask bounds (oc_subtask_bounds): one env per lane, the configurations of the
// block's chunk (blockIdx.y of gridDim.y contiguous chunks of the call's table) in turn
// (configurations and tables in LDS).  Output [subtask][pitch], so each store instruction of a
// wave covers 64 consecutive envs of one configuration.  Chunking the table multiplies the
// waves of a launch: the walk is LDS-latency bound and one chunk left 4 waves per SIMD.
// LDS ordering between the lanes of one wave (its LDS operations run in order; this keeps the
// compiler from moving them and waits for the outstanding ones)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

#ifndef OC_LIK_COMPACT
#define OC_LIK_COMPACT 1
#endif
#ifndef OC_LIK_ROUND_SCALE
#define OC_LIK_ROUND_SCALE 2
#endif
// rows a wave takes per round: 16 with 32-lane groups (8 batches of 2), 32 with 8-lane groups
// (OC_LIK_ROUND_SCALE 2; half that: the same at C5 configuration-major, 2-5 % slower in random
// order and on a one-agent table, profiles/r04/lik_compact/lik_ab_rounds.jsonl; twice that: 10-20 %
// slower, lik_ab_rounds4.jsonl)
constexpr int lik_rows_per_round(int G) { return (G == 32 ? 8 : 16) * OC_LIK_ROUND_SCALE; }
// the compacted form's static LDS beyond the subtask table (16,768 B with 32-lane groups)
constexpr int kLikCompactLds = 9 * 1024 * OC_LIK_ROUND_SCALE;
// The likelihood with the wave's rollouts compacted (OC_LIK_COMPACT).  In the grouped form above
// a rollout lane idles when its candidate is illegal and not the taken one, and a 32-lane group
// idles 7 lanes always (27 on a one-agent row of a joint table).  Here a wave takes kNR rows per
// round, in kNB batches of 64 / G rows (a G-lane group per row, as above):
//   1. each group tests its row's candidates' legality and lists the ones that need a rollout
//      (legal, or the taken action) in the wave's LDS item list, (row << 5) | k, by ballot;
//      rows that need none (None subtask, a level0 raise, a bad alloc id) are written here;
//   2. the wave's lanes take the list 64 items at a time: load the item's row, level0, one
//      rollout (q_value), Q(s, k) and its raise bit into the row's LDS slots;
//   3. each group reads its row's Q values back and takes the softmax as above (the same max,
//      exp and ascending sum, so the outputs are bit-identical to the grouped form).
template <int A, int K, int G, bool W, bool GD>
__global__ __launch_bounds__(kBlock) void oc_likelihood_compact_kernel(RollArgs R, const uint8_t* __restrict__ sin,
                                                                       const uint8_t* __restrict__ taken_p,
                                                                       const uint8_t* __restrict__ alloc,
                                                                       const uint8_t* __restrict__ blob_g,
                                                                       int self_agent, double beta, double nap,
                                                                       double* __restrict__ out,
                                                                       uint8_t* __restrict__ out_flags) {
    constexpr int kCand = G == 32 ? 25 : 5;  // candidates a row can have with this table
    constexpr int kSlots = 32 / G;           // candidate k = lane + G * j, j < kSlots
    constexpr int kRPB = 64 / G;             // rows per batch (one group each)
    constexpr int kNR = lik_rows_per_round(G);  // rows per wave per round
    constexpr int kNB = kNR / kRPB;             // batches per round
    constexpr int kWaves = kBlock / 64;
    constexpr uint32_t kNotPending = 0xFFFFu;
    extern __shared__ __attribute__((aligned(16))) uint32_t blob_w[];
    __shared__ ocro::Sub subs[OC_MAX_SUBTASKS];
    __shared__ double lq[kWaves][kNR][kCand];     // Q(s, k)
    __shared__ uint32_t lok[kWaves][kNR];         // bit k: candidate k's rollout did not raise
    __shared__ uint32_t llg[kWaves][kNR];         // bit k: candidate k is legal
    __shared__ uint32_t lrow[kWaves][kNR];        // kt | ncand << 8, or kNotPending
    __shared__ uint16_t items[kWaves][kNR * kCand];
    stage_roll_tables(R, blob_g, blob_w, subs);
    const uint8_t* blob = (const uint8_t*)blob_w;
    const int64_t P = R.pitch;
    const int wv = (int)(threadIdx.x >> 6), wl = (int)(threadIdx.x & 63), lane = wl & (G - 1), grp = wl / G;
    const uint64_t below = (1ull << wl) - 1ull;
    const int64_t stride = (int64_t)gridDim.x * kWaves * kNR;
    for (int64_t base = ((int64_t)blockIdx.x * kWaves + wv) * kNR; base < R.B; base += stride) {
        wave_lds_sync();  // the previous round's phase 3 has read its slots
        // ---- 1: legality, the rollout list ----
        int n = 0;  // wave-uniform
        for (int b = 0; b < kNB; ++b) {
            const int rs = b * kRPB + grp;
            const int64_t e = base + rs;
            bool pending = false;
            int kt = 0, ncand = 0;
            bool need[kSlots], lgs[kSlots];
#pragma unroll
            for (int j = 0; j < kSlots; ++j) need[j] = lgs[j] = false;
            if (e < R.B) {
                const int ai = alloc != nullptr ? alloc[e] : 0;
                int f = OC_LIK_BADALLOC;
                double v = 0.0;
                if (ai < R.nsub) {
                    const ocro::Sub& s = subs[ai];
                    ocro::RowT<K, W> r = load_row<A, K, W>(sin, P, e);
                    uint32_t taken = 0;
#pragma unroll
                    for (int a = 0; a < A; ++a) taken |= (uint32_t)taken_p[a * P + e] << (8 * a);
                    auto ops = plan_ops<A, K, W, true, GD>(R, blob, blob_g, OC_PT_LIK);
                    if (s.kind == 0) {
                        f = 0;
                        if (lane == 0) f = ops.likelihood(r, s, taken, self_agent, beta, nap, v);
                    } else if (ops.level0(r, s)) {
                        f = OC_LIK_RAISES;  // two removed agents on one square
                    } else {
                        const bool joint = s.n == 2;
                        int t0 = (int)((taken >> (8 * s.agent[0])) & 0xFFu), t1 = ocro::kNoop;
                        if (joint) t1 = (int)((taken >> (8 * s.agent[1])) & 0xFFu);
                        t0 = t0 > ocro::kNoop ? ocro::kNoop : t0;
                        t1 = t1 > ocro::kNoop ? ocro::kNoop : t1;
                        ncand = joint ? 25 : 5;
                        kt = joint ? t0 * 5 + t1 : t0;
                        const int other =
                            joint ? (s.agent[0] == self_agent ? 1 : (s.agent[1] == self_agent ? 0 : -1)) : -1;
#pragma unroll
                        for (int j = 0; j < kSlots; ++j) {
                            const int k = lane + G * j;
                            const int a0 = joint ? k / 5 : k, c1 = joint ? k % 5 : ocro::kNoop;
                            bool lg = k < ncand && ops.action_legal(r, s, a0, c1);
                            if (other == 0 && a0 != t0) lg = false;
                            if (other == 1 && c1 != t1) lg = false;
                            lgs[j] = lg;
                            need[j] = lg || k == kt;
                        }
                        pending = true;
                    }
                }
                if (!pending && lane == 0) {
                    out[e] = f == OC_LIK_OK ? v : 0.0;
                    out_flags[e] = (uint8_t)f;
                }
            }
            uint32_t lgm = 0;
#pragma unroll
            for (int j = 0; j < kSlots; ++j) {
                const uint64_t bn = __ballot(need[j]), bl = __ballot(lgs[j]);
                if (need[j]) items[wv][n + __popcll(bn & below)] = (uint16_t)((rs << 5) | (lane + G * j));
                n += __popcll(bn);
                lgm |= (uint32_t)((bl >> (grp * G)) & (G == 32 ? 0xFFFFFFFFull : ((1ull << G) - 1ull))) << (G * j);
            }
            if (lane == 0) {
                llg[wv][rs] = lgm;
                lok[wv][rs] = 0u;
                lrow[wv][rs] = pending ? (uint32_t)kt | ((uint32_t)ncand << 8) : kNotPending;
            }
        }
        wave_lds_sync();
        // ---- 2: the rollouts, 64 at a time ----
        for (int p = 0; p < n; p += 64) {
            if (p + wl < n) {
                const uint32_t it = items[wv][p + wl];
                const int rs = (int)(it >> 5), k = (int)(it & 31u);
                const int64_t e = base + rs;
                const int ai = alloc != nullptr ? alloc[e] : 0;
                const ocro::Sub& s = subs[ai];
                ocro::RowT<K, W> r = load_row<A, K, W>(sin, P, e);
                auto ops = plan_ops<A, K, W, true, GD>(R, blob, blob_g, OC_PT_LIK);
                ops.level0(r, s);
                const bool joint = s.n == 2;
                const int a0 = joint ? k / 5 : k, c1 = joint ? k % 5 : ocro::kNoop;
                double q = 0.0;
                const bool ok = ops.q_value(r, s, a0, c1, q);
                lq[wv][rs][k] = q;
                if (ok) atomicOr(&lok[wv][rs], 1u << k);
            }
        }
        wave_lds_sync();
        // ---- 3: each pending row's softmax (the grouped form's arithmetic) ----
        for (int b = 0; b < kNB; ++b) {
            const int rs = b * kRPB + grp;
            const int64_t e = base + rs;
            const uint32_t rw = lrow[wv][rs];
            if (e >= R.B || rw == kNotPending) continue;  // group-uniform
            const int kt = (int)(rw & 0xFFu), ncand = (int)(rw >> 8);
            const uint32_t lgm = llg[wv][rs], okm = lok[wv][rs];
            int f;
            double v = 0.0;
            if ((lgm & ~okm) != 0u || !((okm & lgm) >> kt & 1u)) {
                f = OC_LIK_RAISES;
            } else {
                const double old_q = lq[wv][rs][kt];
                double q[kSlots], ex[kSlots];
                bool legal[kSlots];
                double m = -1.0e300;
#pragma unroll
                for (int j = 0; j < kSlots; ++j) {
                    const int k = lane + G * j;
                    legal[j] = (lgm >> k) & 1u;
                    q[j] = legal[j] ? beta * (old_q - lq[wv][rs][k < kCand ? k : 0]) : -1.0e300;
                    m = q[j] > m ? q[j] : m;
                }
#pragma unroll
                for (int off = 1; off < G; off <<= 1) {
                    const double o = __shfl_xor(m, off, G);
                    m = o > m ? o : m;
                }
                double et = 0.0;
#pragma unroll
                for (int j = 0; j < kSlots; ++j) {
                    ex[j] = legal[j] ? exp(q[j] - m) : 0.0;
                    if (lane + G * j == kt) et = ex[j];
                }
                double S = 0.0;  // ascending k: the reference's summation order
#pragma unroll
                for (int j = 0; j < kSlots; ++j)
                    for (int c = 0; c < G && G * j + c < ncand; ++c) S += __shfl(ex[j], c, G);
                v = __shfl(et, kt % G, G) / S;
                f = OC_LIK_OK;
            }
            if (lane == 0) {
                out[e] = v;
                out_flags[e] = (uint8_t)f;
            }
        }
    }
}

// One lane per env, every configuration of the block's chunk.  The bound is a min over the
// env's A locations (Chop, Deliver: bound_static per location) or its (A, B) location pairs
// (Merge: helper per pair), whose count depends on where the items are: walked per lane, lanes
// with fewer locations idle while the others finish (0.58 of the lanes active per VALU
// instruction, profiles/r04/c5/pmc_c5.json).  A wave-compacted walk (the wave's (env, location)
// items by a prefix sum, one per lane, folded by LDS atomics) gave the same outputs with 0.70 of
// the lanes active but ran 0.129 ms against 0.118 at C5, where most (env, configuration) pairs
// have 0 or 1 location; it was removed in round 5 (profiles/r04/bounds_compact/).
template <int A, int K, bool W, bool GD>
__global__ __launch_bounds__(kBlock) void oc_bounds_kernel(RollArgs R, const uint8_t* __restrict__ sin,
                                                           const uint8_t* __restrict__ blob_g,
                                                           float* __restrict__ lb, uint8_t* __restrict__ doable) {
    extern __shared__ __attribute__((aligned(16))) uint32_t blob_w[];
    __shared__ ocro::Sub subs[OC_MAX_SUBTASKS];
    stage_roll_tables(R, blob_g, blob_w, subs);
    const uint8_t* blob = (const uint8_t*)blob_w;
    const int64_t P = R.pitch;
    const int i0 = (int)(blockIdx.y * R.nsub / gridDim.y), i1 = (int)((blockIdx.y + 1) * R.nsub / gridDim.y);
    for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < R.B; e += (int64_t)gridDim.x * kBlock) {
        const ocro::RowT<K, W> r = load_row<A, K, W>(sin, P, e);
        auto ops = plan_ops<A, K, W, false, GD>(R, blob, blob_g, true);  // the agent-pair table (device memory)
        const auto br = ops.template bound_row<true>(r);  // the row's agent nodes, slot sets: once for its configurations
        for (int i = i0; i < i1; ++i) {
            float v;
            const bool ok = ops.full_bound(br, r, subs[i], v);
            lb[i * P + e] = v;
            doable[i * P + e] = ok ? 1 : 0;
        }
    }
}

// Per-env subtask choice of scripted agents (oc_task_select), a sibling of oc_bounds_kernel: one
// env per lane, the tables and the M x S one-agent configurations staged as there, bound_row
// built once per env.  Where the bounds kernel evaluates every configuration and writes 5 bytes
// for each, this one walks only the subtasks some lane of the wave still has in its incomplete set
// (ocro::RowOps::task_env) and reads and writes the agents' few task-state planes; every plane
// access of a wave covers 64 consecutive envs of one plane.  The agents of an env run in order on
// its lane (OC_TASK_DISTINCT makes agent m's candidates depend on agent m - 1's choice), so the
// launch is not chunked over configurations.
struct TaskArgs {
    int32_t S, M, flags;
};
template <int A, int K, bool W, bool GD>
__global__ __launch_bounds__(kBlock) void oc_task_kernel(RollArgs R, TaskArgs Q, const uint8_t* __restrict__ sin,
                                                         const uint8_t* __restrict__ sprev,
                                                         const uint8_t* __restrict__ blob_g, uint8_t* __restrict__ ts,
                                                         float* __restrict__ bound, uint8_t* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) uint32_t blob_w[];
    __shared__ ocro::Sub subs[OC_MAX_SUBTASKS];
    stage_roll_tables(R, blob_g, blob_w, subs);
    const uint8_t* blob = (const uint8_t*)blob_w;
    const int64_t P = R.pitch;
    for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < R.B; e += (int64_t)gridDim.x * kBlock) {
        const ocro::RowT<K, W> r = load_row<A, K, W>(sin, P, e);
        const bool init = starts_over<A, K, W>((Q.flags & OC_TASK_INIT) != 0, sprev, P, e);
        auto ops = plan_ops<A, K, W, false, GD>(R, blob, blob_g, false);  // one-agent rows only: no pair table
        ops.task_env(r, subs, Q.S, Q.M, Q.flags, init, ts + e, bound != nullptr ? bound + e : nullptr,
                     info != nullptr ? info + e : nullptr, P);
    }
}

// Joint and split subtask choice of one pair of scripted agents (oc_team_select), a sibling of
// oc_task_kernel: one env per lane, the tables and the 3 x S configurations (a0's one-agent rows,
// a1's, the two-agent rows) staged as there, hold_cells and bound_row once per env, the subtasks
// walked with a wave-uniform index (ocro::RowOps::team_env: a subtask no lane of the wave has open
// costs none of its three bounds).  The rule's state across the walk is scalars, so nothing is
// indexed by the subtask and nothing goes to scratch for it.  Every plane access of a wave covers
// 64 consecutive envs of one plane.  The two-agent bound reads the agent-pair table where the
// level has one, as oc_bounds_kernel does (the same bytes either way).
struct TeamArgs {
    int32_t S, flags;
};
template <int A, int K, bool W, bool GD>
__global__ __launch_bounds__(kBlock) void oc_team_kernel(RollArgs R, TeamArgs Q, const uint8_t* __restrict__ sin,
                                                         const uint8_t* __restrict__ sprev,
                                                         const uint8_t* __restrict__ blob_g, uint8_t* __restrict__ ts,
                                                         float* __restrict__ bound, uint8_t* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) uint32_t blob_w[];
    __shared__ ocro::Sub subs[OC_MAX_SUBTASKS];
    stage_roll_tables(R, blob_g, blob_w, subs);
    const uint8_t* blob = (const uint8_t*)blob_w;
    const int64_t P = R.pitch;
    for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < R.B; e += (int64_t)gridDim.x * kBlock) {
        const ocro::RowT<K, W> r = load_row<A, K, W>(sin, P, e);
        const bool init = starts_over<A, K, W>((Q.flags & OC_TEAM_INIT) != 0, sprev, P, e);
        auto ops = plan_ops<A, K, W, false, GD>(R, blob, blob_g, true);  // the agent-pair table (device memory)
        ops.team_env(r, subs, Q.S, Q.flags, init, ts + e, bound != nullptr ? bound + e : nullptr,
                     info != nullptr ? info + e : nullptr, P);
    }
}

// The posterior over a watched agent's subtask (oc_belief_update), a sibling of oc_policy_kernel:
// a group of 8 lanes per (env, watched agent), the watched agent m = blockIdx.y (the watched agents
// of an env do not depend on each other).  What the S one-agent hypotheses about one agent share
// is built once per env: every lane builds the agent's Level-0 view, lane k < 5 tests candidate
// k's legality and keeps its successor row (target + interact), and lane 5 keeps state_prev's own
// row with the full-state view, so that the doable test of a hypothesis is the same bound call on
// another row.  The hypotheses are then walked with a wave-uniform index over the table in LDS (the
// block writes its watched agent into the staged rows once); one that no group of the wave has
// live is skipped (wave_any).  Per hypothesis the candidate lanes evaluate q_successor (goal
// count, else the lower bound), lane 5 the distance of the doable test, and the group takes
// oc_policy_kernel's butterfly min and ascending-k sum.  A group's S + 1 beliefs sit in LDS between
// their one load and their one store (hypothesis i by lane i % 8: 8 consecutive envs per wave and
// plane); a run-time hypothesis index into registers would put them in scratch.
struct BeliefArgs {
    double beta, nap;
    int32_t S, M, flags;
    uint8_t agents[4];
};
// the kernel's static LDS: the subtask rows and a group's beliefs (17 KB; allow_dyn_lds counts it)
constexpr int kBeliefStaticLds = (int)(OC_MAX_SUBTASKS * sizeof(ocro::Sub)) + (kBlock / 8) * OC_MAX_SUBTASKS * (int)sizeof(double);
template <int A, int K, bool W, bool GD>
__global__ __launch_bounds__(kBlock) void oc_belief_kernel(RollArgs R, BeliefArgs Q, const uint8_t* __restrict__ sprev,
                                                           const uint8_t* __restrict__ taken,
                                                           const uint8_t* __restrict__ events,
                                                           const uint8_t* __restrict__ blob_g, double* __restrict__ belief,
                                                           uint8_t* __restrict__ bstate, uint8_t* __restrict__ map,
                                                           uint8_t* __restrict__ info) {
    constexpr int G = 8;
    extern __shared__ __attribute__((aligned(16))) uint32_t blob_w[];
    __shared__ ocro::Sub subs[OC_MAX_SUBTASKS];
    __shared__ double bl[kBlock / G][OC_MAX_SUBTASKS];  // a group's beliefs, hypothesis i at [i]
    stage_roll_tables(R, blob_g, blob_w, subs);
    const uint8_t* blob = (const uint8_t*)blob_w;
    const int64_t P = R.pitch;
    using Row = ocro::RowT<K, W>;
    const int lane = (int)(threadIdx.x & (G - 1));
    const int S = Q.S, HP = (S + 8) >> 3, EP = (S + 7) >> 3;
    const int m = (int)blockIdx.y, a = Q.agents[m];
    // this block's watched agent into the staged rows; row S (S <= 63): a's Level-0 configuration
    for (int i = threadIdx.x; i <= S; i += kBlock) {
        ocro::Sub d = i < S ? subs[i] : ocro::Sub{};
        d.kind = i < S ? d.kind : 1;
        d.n = 1;
        d.agent[0] = d.agent[1] = (uint8_t)a;
        d.level = 0;
        subs[i] = d;
    }
    __syncthreads();
    const uint64_t subm = (1ull << S) - 1ull, all = subm | 1ull << S;
    double* bel = belief + (int64_t)m * (S + 1) * P;
    uint8_t* bs = bstate + (int64_t)m * 2 * HP * P;
    double* mine = bl[threadIdx.x / G];
    uint64_t real = 1ull << S;  // the hypotheses a fresh distribution holds
    for (int i = 0; i < S; ++i) real |= subs[i].kind != 0 ? 1ull << i : 0ull;
    const int64_t ngroups = (int64_t)gridDim.x * (kBlock / G);
    for (int64_t e = (int64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G; e < R.B; e += ngroups) {
        // group-uniform from here on, except where `lane` is named
        const bool init = starts_over<A, K, W>((Q.flags & OC_BELIEF_INIT) != 0, sprev, P, e);
        uint64_t open = 0ull, live = 0ull, ev = 0ull;
        if (!init) {
            for (int c = 0; c < HP; ++c) {
                open |= (uint64_t)bs[c * P + e] << (8 * c);
                live |= (uint64_t)bs[(HP + c) * P + e] << (8 * c);
            }
            if (events != nullptr)
                for (int c = 0; c < EP; ++c) ev |= (uint64_t)events[c * P + e] << (8 * c);
        }
        open &= all;
        live &= all;
        ev &= subm;
        int fl = 0;
        bool uniform = false;
        if (init) {
            open = real;
            uniform = true;
            fl = OC_BELF_REINIT;
        } else if ((ev & open) != 0ull) {
            open &= ~ev;
            uniform = true;
            fl = OC_BELF_RESET;
        }
        uint64_t dirty;      // the planes this call writes
        double total = 1.0;  // step 6's total; the uniform paths store what they computed (v * 1.0)
        if (uniform) {
            live = open;
            dirty = all;
            const double u = 1.0 / (double)__popcll(live);
            for (int i = lane; i <= S; i += G) mine[i] = (live >> i) & 1ull ? u : 0.0;
        } else {
            dirty = live;
            for (int i = lane; i <= S; i += G) mine[i] = (live >> i) & 1ull ? bel[i * P + e] : 0.0;
            wave_lds_sync();
            const Row r0 = load_row<A, K, W>(sprev, P, e);
            int t = taken[a * P + e];
            t = t > ocro::kNoop ? ocro::kNoop : t;
            auto ops = plan_ops<A, K, W, true, GD>(R, blob, blob_g, false);  // one-agent hypotheses only: no pair table
            using Ops = decltype(ops);
            const uint32_t mv = ops.none_movable(r0, a);  // the None hypothesis' movable actions, full state
            ops.ac = ops.kNoAc;
            Row v = r0;
            const bool raised0 = ops.level0(v, subs[S]);
            const bool lg = lane < 5 && !raised0 && ops.single_legal(v, a, lane);
            const bool rc = raised0 || !__shfl((int)lg, t, G);  // the reference raises (if a subtask stays live)
            // the row this lane bounds: candidate k's successor on lane k, state_prev itself on lane 5
            Row rb = v;
            if (lg && !rc) ops.interact(rb, a, lane);
            if (lane >= 5) {
                rb = r0;
                ops.ac = ops.kNoAc;
            }
            const double cost = lane != ocro::kNoop ? 1.0 + 0.1 : 1.0;
            const bool worker = lane == 5 || (lg && !rc);
            double p0, p1;  // the None closed form
            bool noop_mode;
            ops.none_probs(__builtin_popcount(mv), Q.beta, Q.nap, p0, p1, noop_mode);
            const double ln = t == ocro::kNoop ? p0 : p1;
            total = 0.0;
            for (int i = 0; i < S; ++i) {
                const bool li = ((live >> i) & 1ull) != 0ull;
                if (!ocro::wave_any(li)) continue;  // wave-uniform
                const ocro::Sub& s = subs[i];
                const bool sub = s.kind != 0;
                // lane 5: q_successor's bound-only form on state_prev itself; its `dist` is the
                // doable test's distance (full_bound's, with the same full-state configuration)
                const int count = lane < 5 ? ops.goal_objects(v, s) : Ops::kBoundOnly;
                double q = 0.0;
                float dist = 0.0f;
                if (li && sub && worker) q = ops.q_successor(rb, s, count, cost, dist);
                if (!li) continue;
                const bool doable = !sub || __shfl((int)(dist < (float)R.L.perimeter), 5, G) != 0;
                double bi = 0.0;
                if (!doable) {
                    live &= ~(1ull << i);
                    fl |= OC_BELF_PRUNED;
                } else {
                    bi = mine[i];
                    if (!rc) {
                        double l = ln;
                        if (sub) {
                            double mq = lg ? q : 1.0e300;
#pragma unroll
                            for (int off = 1; off < G; off <<= 1) {
                                const double o = __shfl_xor(mq, off, G);
                                mq = o < mq ? o : mq;
                            }
                            const double w = lg ? exp(Q.beta * (mq - q)) : 0.0;
                            double sum = 0.0;  // ascending k: the sequential sum
                            for (int c = 0; c < 5; ++c) sum += __shfl(w, c, G);
                            l = __shfl(w / sum, t, G);
                        }
                        bi = bi * l;
                    }
                    total += bi;
                }
                if (lane == 0) mine[i] = bi;
            }
            const bool raises = rc && (live & subm) != 0ull;
            fl |= raises ? OC_BELF_RAISED : OC_BELF_UPDATED;
            if ((live >> S) & 1ull) {
                double bn = mine[S];
                if (!raises) bn = bn * ln;
                total += bn;
                if (lane == 0) mine[S] = bn;
            }
        }
        wave_lds_sync();
        // step 6 on this lane's planes, their stores, and the lowest live hypothesis holding the maximum
        const double r = total == 0.0 ? 1.0 / (double)__popcll(live) : 1.0 / total;
        int best = S;
        double bv = -1.0;
        for (int i = lane; i <= S; i += G) {
            double x = mine[i];
            const bool li = ((live >> i) & 1ull) != 0ull;
            if (li) x = total == 0.0 ? r : x * r;
            if ((dirty >> i) & 1ull) bel[i * P + e] = x;
            if (li && x > bv) {
                best = i;
                bv = x;
            }
        }
#pragma unroll
        for (int off = 1; off < G; off <<= 1) {
            const double ov = __shfl_xor(bv, off, G);
            const int oi = __shfl_xor(best, off, G);
            const bool take = ov > bv || (ov == bv && oi < best);
            bv = take ? ov : bv;
            best = take ? oi : best;
        }
        if (lane == 0) {
            for (int c = 0; c < HP; ++c) {
                bs[c * P + e] = (uint8_t)(open >> (8 * c));
                bs[(HP + c) * P + e] = (uint8_t)(live >> (8 * c));
            }
            if (map != nullptr) map[m * P + e] = (uint8_t)best;
            if (info != nullptr) info[m * P + e] = (uint8_t)fl;
        }
        wave_lds_sync();  // the group's slots are free for its next env
    }
}

// The posterior over a pair's allocation (oc_team_belief_update), oc_belief_kernel's shape run over
// three families of members: a0's one-agent rows, a1's, and the pair's two-agent rows
// (oc_team_select's staging of the 3 x S configurations).  A group of 8 lanes per env; per family
// every lane builds the family's Level-0 view, lane k < 5 tests candidate k's legality and keeps
// its successor row (for the pair: self's action k beside the other member's taken action), lane 5
// keeps state_prev's own row with the full-state view for the doable test, and the S rows are
// walked with a wave-uniform index (a row no group of the wave has live is skipped).  The family
// index is a rolled, wave-uniform loop: one copy of the walk per build.  The group's 3 S + 2
// likelihoods sit in LDS in `lik`'s plane order.
// The posterior pass runs in the same kernel, because `lik` may be NULL and the call allocates
// nothing: a second kernel would have no workspace to read the likelihoods and pruned sets from.
// It keeps no hypothesis-indexed registers: row i is a group-uniform loop and lane l takes the
// columns j = l, l + 8, ..; a first sweep reads the beliefs and sums belief * factor, a second one
// reads them again (the same lane, the same planes), scales and stores, and keeps the first maximum
// in reference order by the hypothesis' key.  Each plane access of a wave covers 8 consecutive envs.
struct TBeliefArgs {
    double beta, nap;
    int32_t S, flags;
    uint8_t a0, a1, self, pad;
};
constexpr int kTBeliefLik = 3 * (OC_TEAM_MAX_SUBTASKS + 1);  // a group's likelihood slots (>= 3 S + 2)
// the kernel's static LDS: the subtask rows and the groups' likelihoods (18 KB; allow_dyn_lds counts it)
constexpr int kTBeliefStaticLds = (int)(OC_MAX_SUBTASKS * sizeof(ocro::Sub)) + (kBlock / 8) * kTBeliefLik * (int)sizeof(double);
template <int A, int K, bool W, bool GD>
__global__ __launch_bounds__(kBlock) void oc_team_belief_kernel(RollArgs R, TBeliefArgs Q, const uint8_t* __restrict__ sprev,
                                                                const uint8_t* __restrict__ taken,
                                                                const uint8_t* __restrict__ events,
                                                                const uint8_t* __restrict__ blob_g, double* __restrict__ bel,
                                                                uint8_t* __restrict__ ts, double* __restrict__ lik,
                                                                uint8_t* __restrict__ map, uint8_t* __restrict__ info) {
    constexpr int G = 8;
    extern __shared__ __attribute__((aligned(16))) uint32_t blob_w[];
    __shared__ ocro::Sub subs[OC_MAX_SUBTASKS];
    __shared__ double ll[kBlock / G][kTBeliefLik];  // a group's L0 at [0, N), L1 at [N, 2N), LJ at [2N, 2N + S)
    stage_roll_tables(R, blob_g, blob_w, subs);
    const uint8_t* blob = (const uint8_t*)blob_w;
    const int64_t P = R.pitch;
    using Row = ocro::RowT<K, W>;
    const int lane = (int)(threadIdx.x & (G - 1));
    const int S = Q.S, N = S + 1, HP = (S + 8) >> 3, EP = (S + 7) >> 3;
    const int a0 = Q.a0, a1 = Q.a1;
    const bool self_first = Q.self == Q.a0;
    const uint32_t subm = (1u << S) - 1u, none = 1u << S;
    uint32_t real = 0u;  // the subtasks a fresh distribution holds
    for (int i = 0; i < S; ++i) real |= subs[i].kind != 0 ? 1u << i : 0u;
    double* mine = ll[threadIdx.x / G];
    const int64_t ngroups = (int64_t)gridDim.x * (kBlock / G);
    for (int64_t e = (int64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G; e < R.B; e += ngroups) {
        // group-uniform from here on, except where `lane` is named
        const bool init = starts_over<A, K, W>((Q.flags & OC_TBELIEF_INIT) != 0, sprev, P, e);
        uint32_t open = 0u, l0 = 0u, l1 = 0u, lJ = 0u, ev = 0u;
        if (!init) {
            for (int c = 0; c < EP; ++c) {
                open |= (uint32_t)ts[c * P + e] << (8 * c);
                lJ |= (uint32_t)ts[(EP + 2 * HP + c) * P + e] << (8 * c);
                if (events != nullptr) ev |= (uint32_t)events[c * P + e] << (8 * c);
            }
            for (int c = 0; c < HP; ++c) {
                l0 |= (uint32_t)ts[(EP + c) * P + e] << (8 * c);
                l1 |= (uint32_t)ts[(EP + HP + c) * P + e] << (8 * c);
            }
        }
        open &= real;
        lJ &= real;
        l0 &= real | none;
        l1 &= real | none;
        int fl = 0;
        bool uniform = false;
        if (init) {
            open = real;
            uniform = true;
            fl = OC_TBELF_REINIT;
        } else if ((ev & open) != 0u) {
            open &= ~ev;
            uniform = true;
            fl = OC_TBELF_RESET;
        }
        uint32_t e0 = subm | none, e1 = subm | none, eJ = subm;  // the planes this call writes: the sets at entry
        bool mult = false;  // step 6 runs
        using Ops = ocro::RowOps<A, K, W, true, GD>;
        if (uniform) {
            l0 = l1 = open | none;
            lJ = open;
        } else {
            e0 = l0, e1 = l1, eJ = lJ;
            for (int i = lane; i < 3 * N; i += G) mine[i] = 0.0;
            wave_lds_sync();
            const Row r0 = load_row<A, K, W>(sprev, P, e);
            int t0 = taken[a0 * P + e], t1 = taken[a1 * P + e];
            t0 = t0 > ocro::kNoop ? ocro::kNoop : t0;
            t1 = t1 > ocro::kNoop ? ocro::kNoop : t1;
            Ops ops = plan_ops<A, K, W, true, GD>(R, blob, blob_g, false);  // the bound walk, as the likelihood kernels
            const int n_self = __builtin_popcount(ops.none_movable(r0, Q.self));  // None: the self agent's movable actions
            double p0, p1;
            bool noop_mode;
            ops.none_probs(n_self, Q.beta, Q.nap, p0, p1, noop_mode);
            uint32_t rmask = 0u;  // bit f: family f raises
#pragma unroll 1
            for (int f = 0; f < 3; ++f) {  // a0 alone, a1 alone, the pair: wave-uniform
                uint32_t lf = f == 0 ? l0 : f == 1 ? l1 : lJ;
                if (!ocro::wave_any((lf & subm) != 0u)) continue;
                const ocro::Sub cf = Ops::team_family(f, a0, a1);
                const int tk = f == 0 ? t0 : f == 1 ? t1 : (self_first ? t0 : t1);  // the taken candidate
                ops.ac = ops.kNoAc;
                Row v = r0;
                const bool raised0 = ops.level0(v, cf);
                int c0, c1;
                Ops::team_candidate(f, self_first, lane < 5 ? lane : ocro::kNoop, t0, t1, c0, c1);
                const bool lg = lane < 5 && !raised0 && ops.action_legal(v, cf, c0, c1);
                // the row this lane bounds: candidate k's successor on lane k, state_prev itself on lane 5
                Row rb = v;
                double cost = 1.0;
                int coloc = 0;
                if (lg) coloc = ops.team_successor(rb, cf, c0, c1, cost) ? 0 : 1;
#pragma unroll
                for (int off = 1; off < G; off <<= 1) coloc |= __shfl_xor(coloc, off, G);
                const bool rc = raised0 || !__shfl((int)lg, tk, G) || coloc != 0;  // the family raises
                if (lane >= 5) {
                    rb = r0;
                    ops.ac = ops.kNoAc;
                }
                const bool worker = lane == 5 || (lg && !rc);
#pragma unroll 1
                for (int i = 0; i < S; ++i) {
                    const bool li = ((lf >> i) & 1u) != 0u;
                    if (!ocro::wave_any(li)) continue;  // wave-uniform
                    const ocro::Sub& s = subs[f * S + i];
                    // lane 5: q_successor's bound-only form on state_prev itself; its `dist` is the
                    // doable test's distance (full_bound's, with the same full-state configuration)
                    const int count = lane < 5 ? ops.goal_objects(v, s) : Ops::kBoundOnly;
                    double q = 0.0;
                    float dist = 0.0f;
                    if (li && worker) q = ops.q_successor(rb, s, count, cost, dist);
                    if (!li) continue;
                    if (__shfl((int)(dist < (float)R.L.perimeter), 5, G) == 0) {  // not doable
                        lf &= ~(1u << i);
                        continue;
                    }
                    if (rc) continue;
                    double mq = lg ? q : 1.0e300;
#pragma unroll
                    for (int off = 1; off < G; off <<= 1) {
                        const double o = __shfl_xor(mq, off, G);
                        mq = o < mq ? o : mq;
                    }
                    const double w = lg ? exp(Q.beta * (mq - q)) : 0.0;
                    double sum = 0.0;  // ascending k: the sequential sum
                    for (int c = 0; c < 5; ++c) sum += __shfl(w, c, G);
                    const double l = __shfl(w / sum, tk, G);
                    if (lane == 0) mine[f * N + i] = l;
                }
                if (f == 0) l0 = lf;
                else if (f == 1) l1 = lf;
                else lJ = lf;
                rmask |= rc ? 1u << f : 0u;
            }
            const int n_live = Ops::team_live_count(l0, l1, lJ);
            if (n_live < Ops::team_live_count(e0, e1, eJ)) fl |= OC_TBELF_PRUNED;
            if (n_live == 0) {
                fl |= OC_TBELF_EMPTY;
            } else {
                const bool raised = ((rmask & 1u) && Ops::team_needs(l0, l1, subm)) ||
                                    ((rmask & 2u) && Ops::team_needs(l1, l0, subm)) || ((rmask & 4u) && lJ != 0u);
                mult = !raised;
                fl |= raised ? OC_TBELF_RAISED : OC_TBELF_UPDATED;
                if (lane == 0) {  // (a raising family's members kept their +0.0)
                    mine[S] = t0 == ocro::kNoop ? p0 : p1;
                    mine[N + S] = t1 == ocro::kNoop ? p0 : p1;
                }
            }
        }
        wave_lds_sync();
        // steps 6 to 8: row i group-uniform, this lane's columns j
        const int n_live = Ops::team_live_count(l0, l1, lJ);
        const double u = 1.0 / (double)n_live;
        auto live = [&](int i, int j) {
            return i == j ? i < S && ((lJ >> i) & 1u) != 0u : ((l0 >> i) & 1u) != 0u && ((l1 >> j) & 1u) != 0u;
        };
        auto value = [&](int i, int j) {  // the live hypothesis' belief before step 7
            if (uniform) return u;
            double x = bel[(int64_t)(i * N + j) * P + e];
            if (mult) x = x * (i == j ? 2.0 * mine[2 * N + i] : mine[i] + mine[N + j]);
            return x;
        };
        double total = 0.0;
        for (int i = 0; i < N; ++i)
            for (int j = lane; j < N; j += G)
                if (live(i, j)) total += value(i, j);
#pragma unroll
        for (int off = 1; off < G; off <<= 1) total += __shfl_xor(total, off, G);
        const double r = total == 0.0 ? u : 1.0 / total;
        double bv = -1.0;
        int key = -1;
        for (int i = 0; i < N; ++i)
            for (int j = lane; j < N; j += G) {
                const bool was = i == j ? i < S && ((eJ >> i) & 1u) != 0u : ((e0 >> i) & 1u) != 0u && ((e1 >> j) & 1u) != 0u;
                if (!was) continue;
                double x = 0.0;
                if (live(i, j)) {
                    x = value(i, j);
                    x = total == 0.0 ? r : x * r;
                    const int k = i == j ? i : S + i * N + j;
                    if (x > bv || (x == bv && k < key)) {
                        bv = x;
                        key = k;
                    }
                }
                bel[(int64_t)(i * N + j) * P + e] = x;
            }
#pragma unroll
        for (int off = 1; off < G; off <<= 1) {
            const double ov = __shfl_xor(bv, off, G);
            const int ok = __shfl_xor(key, off, G);
            const bool take = ov > bv || (ov == bv && ok < key);
            bv = take ? ov : bv;
            key = take ? ok : key;
        }
        if (mult && lik != nullptr)
            for (int i = lane; i < 3 * S + 2; i += G) lik[(int64_t)i * P + e] = mine[i];
        if (lane == 0) {
            int m0, m1, mJ;
            Ops::team_map_bytes(key, S, m0, m1, mJ);
            if (mJ < S) fl |= OC_TBELF_JOINT;
            for (int c = 0; c < EP; ++c) {
                ts[c * P + e] = (uint8_t)(open >> (8 * c));
                ts[(EP + 2 * HP + c) * P + e] = (uint8_t)(lJ >> (8 * c));
            }
            for (int c = 0; c < HP; ++c) {
                ts[(EP + c) * P + e] = (uint8_t)(l0 >> (8 * c));
                ts[(EP + HP + c) * P + e] = (uint8_t)(l1 >> (8 * c));
            }
            if (map != nullptr) {
                map[e] = (uint8_t)m0;
                map[P + e] = (uint8_t)m1;
                map[2 * P + e] = (uint8_t)mJ;
            }
            if (info != nullptr) info[e] = (uint8_t)fl;
        }
        wave_lds_sync();  // the group's slots are free for its next env
    }
}

// ---- wide levels (more than 255 cells: u16 cell ids) ----------------------------------------
// A wide level (more than 255 cells, u16 cell ids) is stepped by ocsw::step4w: the SWAR step
// with every cell-valued quantity as two byte words (its low and high bytes, the wide layout's
// two item-cell planes), four envs per lane like oc_step_n_kernel.  Such levels are user kitchens;
// the shipped ones are all narrow.  Its kernel takes no 256-byte narrow class table (LevelArgs::cls4):
// the classes come from the level's tile table in device memory.
struct WideArgs {
    ocsw::SwarLevel sw;  // the SWAR step's constants (step4w reads the wide fields)
    int32_t tile_words;  // the tile table's words (W * H bytes rounded up to 4)
    int64_t pitch, B;
};

// n steps of every env (oc_step: n = 1, no trajectory): the state stays in registers between
// the steps; step r's state goes to traj[r] (when given), its executed actions and collision
// mask to exec_out / coll_out at r * A * pitch / r * pitch; the final state to sout.  Four envs
// per lane, every plane read and written one dword per lane (256 B per wave instruction)
// through buffer resources (an absent output's stores are dropped by its num_records = 0, so
// every store is unconditional), nt stores, the next step's action words loaded before the
// current step runs.
template <int A, int K>
__global__ __launch_bounds__(kBlock) void oc_step_wide_kernel(WideArgs R, const uint8_t* __restrict__ tiles_g,
                                                              const uint8_t* __restrict__ sin, uint8_t* __restrict__ sout,
                                                              const uint8_t* __restrict__ act,
                                                              uint8_t* __restrict__ traj, uint8_t* __restrict__ exec_out,
                                                              uint8_t* __restrict__ coll_out, uint64_t* __restrict__ stats,
                                                              uint32_t stat_rows, int n) {
    // tile class bytes (ocsw::tile_class: Floor 0x80, Counter 0, Cutboard 0x20, Delivery 0x40)
    // of the OC_TILE_* codes, one v_perm per word
    __shared__ uint32_t cls_w[ocro::kMaxCellsWide / 4];
    for (int i = threadIdx.x; i < R.tile_words; i += kBlock)
        cls_w[i] = __builtin_amdgcn_perm(0u, 0x40200080u, ((const uint32_t*)tiles_g)[i]);
    __syncthreads();
    const uint8_t* cls_b = (const uint8_t*)cls_w;
    auto cls_of = [&](const ocsw::Cell2& c) -> uint32_t {  // per env: the class of cell (hi << 8 | lo)
        uint32_t r = 0u;
#pragma unroll
        for (int q = 0; q < kEPL; ++q) {
            const uint32_t idx = __builtin_amdgcn_perm(c.hi >> (8 * q), c.lo >> (8 * q), 0x0C0C0400u) & 0x3FFu;
            r |= (uint32_t)cls_b[idx] << (8 * q);
        }
        return r;
    };
    using PL = Planes<A, K, true>;
    const uint32_t P = (uint32_t)R.pitch;
    const uint32_t nlanes = (uint32_t)((R.B + kEPL - 1) / kEPL);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(sin, (int64_t)PL::NP * P);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(sout ? (const void*)sout : (const void*)sin, sout ? (int64_t)PL::NP * P : 0);
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(act, (int64_t)n * A * P);
    const __amdgpu_buffer_rsrc_t rt = make_rsrc(traj ? (const void*)traj : (const void*)sin, traj ? (int64_t)n * PL::NP * P : 0);
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(exec_out ? (const void*)exec_out : (const void*)sin,
                                                exec_out ? (int64_t)n * A * P : 0);
    const __amdgpu_buffer_rsrc_t rc = make_rsrc(coll_out ? (const void*)coll_out : (const void*)sin,
                                                coll_out ? (int64_t)n * P : 0);
    StepStats st;
    typedef unsigned int u32x2 __attribute__((__vector_size__(2 * sizeof(unsigned int))));
    for (uint32_t g = blockIdx.x * (uint32_t)kBlock + threadIdx.x; g < nlanes; g += gridDim.x * (uint32_t)kBlock) {
        const uint32_t vo = g * 4u;
        uint32_t X[A], Y[A], H[A], LO[K], HI[K], M[K], wa[A], nx[A];
#pragma unroll
        for (int a = 0; a < A; ++a) {
            X[a] = bld32(rs, vo, a * P);
            Y[a] = bld32(rs, vo, (PL::Y + a) * P);
            H[a] = bld32(rs, vo, (PL::HOLD + a) * P);
            wa[a] = bld32(ra, vo, a * P);
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            LO[j] = bld32(rs, vo, (PL::LOC + j) * P);
            HI[j] = bld32(rs, vo, (PL::LOC_HI + j) * P);
            M[j] = bld32(rs, vo, (PL::MASK + j) * P);
        }
        const auto tw0 = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(g * 8u), (int)(PL::T * P), 0);
        uint32_t T0 = tw0[0], T1 = tw0[1], F = bld32(rs, vo, PL::F * P);
        uint32_t pending = ocsw::at_done80w<K>(R.sw, LO, HI);  // the loaded state: the full path once
        const int64_t rem = R.B - (int64_t)g * kEPL;
        const uint32_t vmask = rem >= kEPL ? 0xFFFFFFFFu : (rem <= 0 ? 0u : (1u << (8 * (uint32_t)rem)) - 1u);
        for (int q = 0; q < n; ++q) {
#pragma unroll
            for (int a = 0; a < A; ++a) nx[a] = q + 1 < n ? bld32(ra, vo, (uint32_t)((q + 1) * A + a) * P) : 0u;
            uint32_t EX[A], CM;
            const uint32_t f_in = F;
            const bool full = ocsw::step4w<A, K>(R.sw, X, Y, H, LO, HI, M, T0, T1, F, wa, EX, CM, cls_of, WaveAny{},
                                                 pending);
            st.coll += __popc(CM & vmask);
            if (full) {  // episode ends only on the full path
                const uint32_t ended = (F & ~f_in & vmask) & ocsw::k01;
                st.eps += __popc(ended);
                st.succ += __popc(F & (ended << 1));
                st.err += __popc(F & (ended << 2));
                const uint32_t efull = (0x80808080u - ended) ^ 0x80808080u;
                const uint32_t sa = T0 & __builtin_amdgcn_perm(0u, efull, 0x01010000u);
                const uint32_t sb2 = T1 & __builtin_amdgcn_perm(0u, efull, 0x03030202u);
                st.steps += (sa & 0xFFFFu) + (sa >> 16) + (sb2 & 0xFFFFu) + (sb2 >> 16);
            }
            const uint32_t base = (uint32_t)q * PL::NP * P;
#pragma unroll
            for (int a = 0; a < A; ++a) {
                bst32<kCPnt>(rt, X[a], vo, base + a * P);
                bst32<kCPnt>(rt, Y[a], vo, base + (PL::Y + a) * P);
                bst32<kCPnt>(rt, H[a], vo, base + (PL::HOLD + a) * P);
                bst32<kCPnt>(rx, EX[a], vo, (uint32_t)(q * A + a) * P);
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                bst32<kCPnt>(rt, LO[j], vo, base + (PL::LOC + j) * P);
                bst32<kCPnt>(rt, HI[j], vo, base + (PL::LOC_HI + j) * P);
                bst32<kCPnt>(rt, M[j], vo, base + (PL::MASK + j) * P);
            }
            const u32x2 tv = {T0, T1};
            __builtin_amdgcn_raw_buffer_store_b64(tv, rt, (int)(g * 8u), (int)(base + PL::T * P), kCPnt);
            bst32<kCPnt>(rt, F, vo, base + PL::F * P);
            bst32<kCPnt>(rc, CM, vo, (uint32_t)q * P);
#pragma unroll
            for (int a = 0; a < A; ++a) wa[a] = nx[a];
        }
#pragma unroll
        for (int a = 0; a < A; ++a) {
            bst32<kCPnt>(ro, X[a], vo, a * P);
            bst32<kCPnt>(ro, Y[a], vo, (PL::Y + a) * P);
            bst32<kCPnt>(ro, H[a], vo, (PL::HOLD + a) * P);
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            bst32<kCPnt>(ro, LO[j], vo, (PL::LOC + j) * P);
            bst32<kCPnt>(ro, HI[j], vo, (PL::LOC_HI + j) * P);
            bst32<kCPnt>(ro, M[j], vo, (PL::MASK + j) * P);
        }
        const u32x2 tv = {T0, T1};
        __builtin_amdgcn_raw_buffer_store_b64(tv, ro, (int)(g * 8u), (int)(PL::T * P), kCPnt);
        bst32<kCPnt>(ro, F, vo, PL::F * P);
    }
    if (stats != nullptr) {
        const uint32_t v[OC_NSTATS] = {wave_sum(st.eps), wave_sum(st.succ), wave_sum(st.steps), wave_sum(st.coll),
                                       wave_sum(st.err)};
        if ((threadIdx.x & 63u) == 0u) {
            unsigned long long* row = (unsigned long long*)stats + (int64_t)(blockIdx.x % stat_rows) * OC_NSTATS;
#pragma unroll
            for (int c = 0; c < OC_NSTATS; ++c)
                if (v[c]) atomicAdd(row + c, (unsigned long long)v[c]);
        }
    }
}

// Image observation (oc_render, GameImage.get_image_obs: gym_cooking/misc/game/gameimage.py:31-51,
// Game.on_render / draw_*: game.py:56-186).  Two blocks per (env, cell row), each taking half
// of the row's pixel groups in whole waves.  In each block the first W lanes
// build each cell's ordered draw list in LDS (items not held in slot order or the caller's
// draw rank, then every agent
// in order followed by its held item).  The block then writes the row's tile*W*tile*3 output
// bytes in iterations of 16 pixels per lane (48 output bytes), consecutive lanes on consecutive
// pixels, so a wave's 64 lanes cover 1,024 pixels that span every cell of one to three image
// rows.  A pixel starts from the static level image and blends every sprite of its cell's list
// that covers it; everything is tile-local (every sprite lies inside its cell).  Only the lanes
// over a cell with sprites have blending to do, so the wave does it together: those lanes put
// their 16 pixels in the wave's LDS slice and list themselves, and the wave then blends the
// listed pixels one per lane (16 c / 64 passes for c listed lanes) instead of the listed lanes
// looping over 16 pixels each while the others idle.
struct RenderArgs {
    int32_t W, H, tile;
    int32_t size[OC_RENDER_SIZES], offset[OC_RENDER_SIZES], food_base[OC_RENDER_SIZES];
    int32_t plate_off[2], agent_off[OC_MAX_AGENTS];
    uint32_t chan_map;
    int32_t parts;  // blocks per (env, cell row), each a contiguous run of whole waves of groups
    int32_t counts; // item masks in OC_ENC_COUNTS: translated to the presence masks food_sprite reads
    int64_t pitch;
    uint8_t food_sprite[128];
};
// A render block lists the draws of its cell row (one lane per column, so a row of up to 255
// columns: every width a level may have) in one compact list: a cell row holds every object at
// most once, so it draws at most kRenderMaxDraw sprites (a plate and a food per item, an agent
// and its held item's two), whatever its width.  Round 4's per-column lists (kRenderMaxDraw
// entries for each of 32 or 64 columns) capped the width at 32 (narrow) / 64 (wide) columns.
constexpr int kRenderMaxW = 255, kRenderMaxDraw = 2 * OC_MAX_ITEMS + 3 * OC_MAX_AGENTS;
constexpr int kRenderPx = 16;  // pixels per lane and iteration: 48 output bytes, three 16-byte stores

// SDL 1.2 per-pixel alpha blit of an RGBA source pixel onto an RGB destination pixel
// (BlitNtoNPixelAlpha / ALPHA_BLEND: d = (((s - d) * a + 255) >> 8) + d per channel, a = 0
// skipped).  ((s - d) a + 255 >> 8) + d = (s a + d (256 - a) + 255) >> 8 exactly, and that
// numerator is at most 65,535, so R and B share one 24-bit multiply-add pair in 16-bit fields
// without carries; a = 0 gives (256 d + 255) >> 8 = d, the skipped blit, with no branch.
__device__ __forceinline__ uint32_t sdl_blend(uint32_t d, uint32_t s) {
    const uint32_t a = s >> 24, na = 256u - a;
    const uint32_t rb = __umul24(d & 0xFF00FFu, na) + __umul24(s & 0xFF00FFu, a) + 0xFF00FFu;
    const uint32_t g = __umul24((d >> 8) & 0xFFu, na) + __umul24((s >> 8) & 0xFFu, a) + 0xFFu;
    return ((rb >> 8) & 0xFF00FFu) | (g & 0xFF00u);
}

// floor(n / d) for 0 <= n < 2^22 and 0 < d <= 2^11, from a float reciprocal and one correction
__device__ __forceinline__ int div_small(int n, int d, float rcp) {
    int q = (int)((float)n * rcp);
    const int rem = n - q * d;
    q += rem >= d ? 1 : 0;
    q -= rem < 0 ? 1 : 0;
    return q;
}

template <int A, int K, bool WIDE>
__global__ __launch_bounds__(kBlock) void oc_render_kernel(RenderArgs R, const uint8_t* __restrict__ state,
                                                           const uint8_t* __restrict__ rank,
                                                           const uint32_t* __restrict__ atlas,
                                                           const uint32_t* __restrict__ bg,
                                                           uint8_t* __restrict__ out) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    __shared__ uint32_t dl_off[kRenderMaxDraw];
    __shared__ uint32_t dl_geo[kRenderMaxDraw];    // size | offset << 16
    __shared__ uint16_t col_start[kBlock + 1];     // column c's draws: [col_start[c], col_start[c + 1])
    __shared__ uint32_t wave_tot[kBlock / 64];
    __shared__ u32x4 pix4[kBlock / 64][64 * kRenderPx / 4];
    __shared__ uint32_t work[kBlock / 64][64];  // listed lane | row << 6 | cell column << 16 | (x in cell) / 16 << 24
    const uint32_t part = blockIdx.x % (uint32_t)R.parts, strip = blockIdx.x / (uint32_t)R.parts;
    const int64_t e = strip / (uint32_t)R.H;
    const int ty = (int)(strip % (uint32_t)R.H);
    const int W = R.W, tile = R.tile;
    // planes: a wide level's item cells are u16, low bytes then high bytes, before the masks
    using PL = Planes<A, K, WIDE>;
    // The cell row's draw list: every column lane counts its draws, a block prefix sum places
    // them, and the lanes write them in the same order (draw order within a column).
    const int tx = (int)threadIdx.x, cell = ty * W + tx;
    const uint8_t* s = state + e;
    const int64_t P = R.pitch;
    auto column = [&](bool write, int n) -> int {  // this column's draws from slot n on; returns the end
        uint32_t held = 0u;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const uint32_t h = s[(PL::HOLD + a) * P];
            if (h < (uint32_t)K) held |= 1u << h;
        }
        auto push = [&](int32_t off, int cls) {
            if (write) {
                dl_off[n] = (uint32_t)off;
                dl_geo[n] = (uint32_t)R.size[cls] | ((uint32_t)R.offset[cls] << 16);
            }
            ++n;
        };
        // an item: a plate first, its contents at the container class; else the food itself
        auto push_item = [&](uint32_t m, int cls_plain, int cls_in_plate, int plate) {
            if (R.counts) {  // counts -> presence; two of one food have no sprite (the reference's
                             // draw opens "<full_name>.png", which does not exist: it raises)
                const uint32_t c = m & 0x3Fu, pres = (c & 1u) | ((c >> 1) & 2u) | ((c >> 2) & 4u);
                const uint32_t pl = (m & OC_MC_PLATE) ? OC_M_PLATE : 0u;
                m = (c & 0x2Au) ? pl : pl | pres | ((m & OC_MC_FRESH) ? 0u : pres << OC_M_CHOPPED_SHIFT);
            }
            const uint32_t f = m & ~OC_M_PLATE;
            if (m & OC_M_PLATE) push(R.plate_off[plate], cls_plain);
            const int cls = (m & OC_M_PLATE) ? cls_in_plate : cls_plain;
            if (f != 0u && R.food_sprite[f] != 0xFFu)
                push(R.food_base[cls] + (int32_t)R.food_sprite[f] * R.size[cls] * R.size[cls], cls);
        };
        // Game.on_render: objects not held (draw_object, game.py:138-160), in world.objects order
        // when the caller gives ranks (render.DrawOrder), else in slot order ...
        uint32_t here = 0u;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int c = WIDE ? (int)s[(PL::LOC + j) * P] | (int)s[(PL::LOC_HI + j) * P] << 8 : (int)s[(PL::LOC + j) * P];
            if (c == cell) here |= 1u << j;  // a dead slot (0xFF / 0xFFFF) is no cell
        }
        here &= ~held;
        while (here != 0u) {
            int j = __builtin_ctz(here);
            if (rank != nullptr && (here & (here - 1u)) != 0u) {  // several objects on this square
                uint32_t best = 0xFFFFFFFFu;
                for (uint32_t m = here; m != 0u; m &= m - 1u) {
                    const int k = __builtin_ctz(m);
                    const uint32_t key = ((uint32_t)rank[(int64_t)k * P + e] << 5) | (uint32_t)k;
                    if (key < best) best = key;
                }
                j = (int)(best & 31u);
            }
            here &= ~(1u << j);
            push_item(s[(PL::MASK + j) * P], 0, 1, 0);
        }
        // ... then the agents in order, each with its held object (draw_agent / draw_agent_object, :98-136)
#pragma unroll
        for (int a = 0; a < A; ++a) {
            if ((int)s[(PL::Y + a) * P] * W + (int)s[(PL::X + a) * P] != cell) continue;
            push(R.agent_off[a], 0);
            const uint32_t h = s[(PL::HOLD + a) * P];
            if (h < (uint32_t)K) push_item(s[(PL::MASK + h) * P], 2, 3, 1);
        }
        return n;
    };
    const int cnt = tx < W ? column(false, 0) : 0;
    int incl = cnt;  // inclusive scan over the wave, then over the block's waves
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if ((tx & 63) >= off) incl += o;
    }
    if ((tx & 63) == 63) wave_tot[tx >> 6] = (uint32_t)incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < (tx >> 6); ++w) before += (int)wave_tot[w];
    const int start = before + incl - cnt;
    col_start[tx] = (uint16_t)start;
    if (tx == kBlock - 1) col_start[kBlock] = (uint16_t)(start + cnt);
    if (tx < W) column(true, start);
    __syncthreads();
    const int row_px = W * tile, G = row_px / kRenderPx;  // 16-pixel groups per image row
    // this block's share of the strip's 16-pixel groups: whole waves of them
    const int per_part = (tile * G + 64 * R.parts - 1) / (64 * R.parts) * 64;
    const int i_begin = (int)part * per_part, items = min(tile * G, i_begin + per_part);
    const float rcpG = 1.0f / (float)G, rcpT = 1.0f / (float)tile;
    const int64_t img_bytes = (int64_t)R.H * tile * row_px * 3;
    uint8_t* img = out + e * img_bytes;
    // chan_map -> v_perm selector: output byte c <- pixel byte (chan_map >> 8c), 0x0C = zero
    uint32_t psel = 0x0C000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t ch = (R.chan_map >> (8 * c)) & 0xFFu;
        psel |= (ch >= 3u ? 0x0Cu : ch) << (8 * c);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t* const pix = (uint32_t*)pix4[wave];
    uint8_t* const blk_out = img + (int64_t)ty * tile * row_px * 3;
    for (int base = i_begin; base < items; base += kBlock) {
        const int w0 = base + wave * 64;  // the wave's first group
        const int i = w0 + lane;
        uint32_t p[kRenderPx];
        bool need = false;
        int r = 0, tx = 0, lx0 = 0;
        if (i < items) {
            r = div_small(i, G, rcpG);
            const int py = ty * tile + r, px0 = kRenderPx * (i - r * G);
            tx = div_small(px0, tile, rcpT);  // a group never straddles two cells
            lx0 = px0 - tx * tile;
            const u32x4* bsrc = (const u32x4*)(bg + (int64_t)py * row_px + px0);
#pragma unroll
            for (int q = 0; q < kRenderPx / 4; ++q) {
                const u32x4 v = bsrc[q];
                p[4 * q] = v.x;
                p[4 * q + 1] = v.y;
                p[4 * q + 2] = v.z;
                p[4 * q + 3] = v.w;
            }
            const int d1 = col_start[tx + 1];
            for (int d = col_start[tx]; d < d1; ++d) {
                const uint32_t geo = dl_geo[d];
                const int sz = (int)(geo & 0xFFFFu), o = (int)(geo >> 16);
                need |= (unsigned)(r - o) < (unsigned)sz && lx0 + kRenderPx > o && lx0 < o + sz;
            }
        }
        const uint64_t mask = __ballot(need);
        if (mask != 0ull) {
            if (need) {
#pragma unroll
                for (int q = 0; q < kRenderPx / 4; ++q)
                    pix4[wave][4 * lane + q] = u32x4{p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]};
                const uint32_t slot =
                    __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                work[wave][slot] = (uint32_t)lane | ((uint32_t)r << 6) | ((uint32_t)tx << 16) | ((uint32_t)(lx0 >> 4) << 24);
            }
            __builtin_amdgcn_wave_barrier();  // LDS is in order within a wave; keep the compiler from moving reads up
            const int npx = kRenderPx * __popcll(mask);
            for (int t = lane; t < npx; t += 64) {
                const uint32_t ent = work[wave][t >> 4];
                const int k = t & (kRenderPx - 1), gl = (int)(ent & 63u);
                const int rr = (int)((ent >> 6) & 0x3FFu), ctx = (int)((ent >> 16) & 0xFFu), lx = (int)(ent >> 24) * 16 + k;
                uint32_t dpx = pix[kRenderPx * gl + k];
                const int d1 = col_start[ctx + 1];
                for (int d = col_start[ctx]; d < d1; ++d) {
                    const uint32_t geo = dl_geo[d];
                    const int sz = (int)(geo & 0xFFFFu), o = (int)(geo >> 16);
                    const int dy = rr - o, dx = lx - o;
                    if ((unsigned)dy < (unsigned)sz && (unsigned)dx < (unsigned)sz)
                        dpx = sdl_blend(dpx, atlas[dl_off[d] + dy * sz + dx]);
                }
                pix[kRenderPx * gl + k] = dpx;
            }
            __builtin_amdgcn_wave_barrier();
            if (need) {
#pragma unroll
                for (int q = 0; q < kRenderPx / 4; ++q) {
                    const u32x4 v = pix4[wave][4 * lane + q];
                    p[4 * q] = v.x;
                    p[4 * q + 1] = v.y;
                    p[4 * q + 2] = v.z;
                    p[4 * q + 3] = v.w;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        // The block's output rows are contiguous and group i lands at byte 48 i, so a wave's 64
        // groups are 3 KB contiguous.  Each lane packs its 48 bytes into the wave's LDS slice, and
        // the wave then stores the slice as three fully contiguous 1 KB instructions (16 B per
        // lane) instead of three 16 B-per-lane instructions at a 48 B stride.
        if (i < items) {
            uint32_t w[12];  // 16 pixels -> 48 bytes: per 4 pixels three dwords of packed 3-byte pixels
#pragma unroll
            for (int q = 0; q < kRenderPx / 4; ++q) {
                const uint32_t a0 = __builtin_amdgcn_perm(0u, p[4 * q], psel),
                               a1 = __builtin_amdgcn_perm(0u, p[4 * q + 1], psel),
                               a2 = __builtin_amdgcn_perm(0u, p[4 * q + 2], psel),
                               a3 = __builtin_amdgcn_perm(0u, p[4 * q + 3], psel);
                w[3 * q] = a0 | (a1 << 24);
                w[3 * q + 1] = (a1 >> 8) | (a2 << 16);
                w[3 * q + 2] = (a2 >> 16) | (a3 << 8);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) pix4[wave][3 * lane + q] = u32x4{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
        }
        __builtin_amdgcn_wave_barrier();
        const int nbytes = 48 * (items - w0 < 64 ? (items - w0 > 0 ? items - w0 : 0) : 64);
        u32x4* dst = (u32x4*)(blk_out + (int64_t)w0 * 48);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int off = q * 64 + lane;  // 16-byte units
            if (off * 16 < nbytes) __builtin_nontemporal_store(pix4[wave][off], dst + off);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// reset(): broadcast the level template (overcooked_environment.py:201-250) over the whole pitch,
// one chunk per lane through the shared store walk with 64-bit addresses (no 2 GiB limit here).
struct GlobalWords {
    uint8_t* s;
    int64_t P, g;
    __device__ __forceinline__ uint32_t ld32(int plane) const {
        return *reinterpret_cast<const uint32_t*>(s + plane * P + 4 * g);
    }
    __device__ __forceinline__ void ld64(int plane, uint32_t& lo, uint32_t& hi) const {
        const uint2 v = *reinterpret_cast<const uint2*>(s + plane * P + 8 * g);
        lo = v.x;
        hi = v.y;
    }
    __device__ __forceinline__ void st32(int plane, uint32_t v) const {
        *reinterpret_cast<uint32_t*>(s + plane * P + 4 * g) = v;
    }
    __device__ __forceinline__ void st64(int plane, uint32_t lo, uint32_t hi) const {
        *reinterpret_cast<uint2*>(s + plane * P + 8 * g) = make_uint2(lo, hi);
    }
};
template <int A, int K, bool WIDE>
__global__ __launch_bounds__(kBlock) void oc_reset_kernel(ocsw::SwarLevel sw, int64_t pitch, uint8_t* __restrict__ s) {
    ocio::store(ocio::template_chunk<A, K, WIDE>(sw), GlobalWords{s, pitch, (int64_t)blockIdx.x * kBlock + threadIdx.x});
}

// Randomised starts (oc_startdist.h), one lane per 4-env word as the step.  The handle's lists, the
// x / y table and the agent_ok bytes are staged in LDS once per block ((A + 2) lists of u16 and A
// byte tables: 3.5 KiB at most on a narrow level, 16 KiB on a wide one with four agents).  Full mode
// (sprev null): every lane below B stores its whole chunk, the batch's last word completed with the
// template.  Masked mode: the lane's flags word of sprev is loaded first; a block without a DONE env
// leaves before the staging, a wave without one after it behind a wave-uniform test, a lane without
// one stores nothing, and a lane with some loads its chunk of `s`, merges the restarting envs' bytes
// into it and stores the words back (a lane owns its words; s may be sprev).  The masked call follows
// every step, so its critical path is kept short: the table words are fetched into registers together
// with the flags word (one memory round trip before the block's decision, not two), the chunk of `s`
// is requested before the draws and arrives while they run, and the draws take every lane's lowest
// restarting env per round (ocsd::start_chunk).
template <int A, int K, bool WIDE>
__global__ __launch_bounds__(ocsd::kBlock) void oc_reset_random_kernel(ocsw::SwarLevel sw, ocsd::StartArgs R,
                                                                       const uint32_t* __restrict__ tab_g,
                                                                       int tab_words, uint8_t* s,
                                                                       const uint8_t* sprev) {
    constexpr int NC = WIDE ? OC_MAX_CELLS : 256;
    constexpr int kWords = ((A + 2) * NC * 2 + A * NC) / 4, kPre = (kWords + ocsd::kBlock - 1) / ocsd::kBlock;
    __shared__ uint32_t tab[kWords];
    uint32_t pre[kPre];
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
        const int w = i * ocsd::kBlock + (int)threadIdx.x;
        pre[i] = w < tab_words ? tab_g[w] : 0u;
    }
    const int64_t g = (int64_t)blockIdx.x * ocsd::kBlock + threadIdx.x;
    const int64_t rem = R.B - 4 * g;
    const uint32_t vmask = ocio::valid_mask(R.B, g);
    uint32_t done = 0u;  // 0x01 per restarting env (masked mode)
    if (R.masked) {
        if (rem > 0) done = *reinterpret_cast<const uint32_t*>(sprev + Planes<A, K, WIDE>::F * R.pitch + 4 * g);
        done &= vmask & ocsw::k01 * OC_FLAG_DONE;
        if (!__syncthreads_or(done != 0u)) return;
    }
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
        const int w = i * ocsd::kBlock + (int)threadIdx.x;
        if (w < tab_words) tab[w] = pre[i];
    }
    __syncthreads();
    if (rem <= 0) return;
    uint32_t sel;
    if (R.masked) {
        if (__ballot(done != 0u) == 0ull) return;
        if (done == 0u) return;
        sel = (done & 1u) | ((done >> 7) & 2u) | ((done >> 14) & 4u) | ((done >> 21) & 8u);
    } else {
        sel = rem >= 4 ? 0xFu : (1u << (uint32_t)rem) - 1u;
    }
    const GlobalWords out{s, R.pitch, g};
    Chunk<A, K, WIDE> c, o;
    if (R.masked) ocio::load<false>(o, out, out);
    ocsd::start_chunk<A, K, WIDE>(sw, R, ocsd::tab_of<A>(tab, R), g, sel, c);
    if (R.masked) {
        ocsd::merge(o, c, (done << 8) - done);  // 0x01 -> 0xFF per byte
        ocio::store(o, out);
    } else {
        ocio::store(c, out);
    }
}

// Order-sensitive 64-bit checksum of the state of envs [0, B):
//   sum_e (2e + 1) * sum_p (byte_p(e) + 1) * M_p,   M_p = 0x9E3779B97F4A7C15 * (2p + 1)  (mod 2^64)
// over the byte planes p (the u16 t plane as its low / high byte planes).  It reads the state
// exactly like oc_step does (one dword per plane per lane), so it doubles as the known-byte
// read pass that calibrates the FETCH_SIZE counter for this access pattern.
template <int NP>
__global__ __launch_bounds__(kBlock) void oc_checksum_kernel(const uint8_t* __restrict__ s, int64_t pitch,
                                                             int64_t B,
                                                             unsigned long long* __restrict__ out) {
    constexpr int plane_t = NP - 3;  // t precedes the flags plane (oc_layout)
    const uint32_t g = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const int64_t e0 = (int64_t)g * kEPL;
    uint64_t h[kEPL] = {};
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const uint64_t Mp = 0x9E3779B97F4A7C15ull * (uint64_t)(2 * p + 1);
        if (p == plane_t) {
            const uint2 w = reinterpret_cast<const uint2*>(s + p * pitch)[g];
            const uint64_t Mq = 0x9E3779B97F4A7C15ull * (uint64_t)(2 * p + 3);
#pragma unroll
            for (int q = 0; q < kEPL; ++q) {
                const uint32_t v = ((q < 2 ? w.x : w.y) >> (16 * (q & 1))) & 0xFFFFu;
                h[q] += (uint64_t)((v & 0xFFu) + 1u) * Mp + (uint64_t)((v >> 8) + 1u) * Mq;
            }
        } else if (p != plane_t + 1) {
            const uint32_t w = reinterpret_cast<const uint32_t*>(s + p * pitch)[g];
#pragma unroll
            for (int q = 0; q < kEPL; ++q) h[q] += (uint64_t)(((w >> (8 * q)) & 0xFFu) + 1u) * Mp;
        }
    }
    uint64_t acc = 0;
#pragma unroll
    for (int q = 0; q < kEPL; ++q)
        acc += (e0 + q < B) ? h[q] * (uint64_t)(2 * (e0 + q) + 1) : 0ull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, (unsigned long long)acc);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(kBlock) void oc_gen_actions_kernel(uint8_t* __restrict__ act, int A, int64_t B,
                                                                int64_t pitch, int64_t env_offset,
                                                                uint64_t step, uint64_t seed) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= pitch) return;
    const uint64_t base = seed ^ ((uint64_t)(env_offset + e) * 0x9E3779B97F4A7C15ull) ^
                          (step * 0xC2B2AE3D27D4EB4Full);
    for (int a = 0; a < A; ++a)
        act[a * pitch + e] = e < B ? (uint8_t)(splitmix64(base ^ (uint64_t)a) % 5u) : (uint8_t)OC_ACT_NOOP;
}

__global__ __launch_bounds__(kBlock) void oc_stats_reduce_kernel(const uint64_t* __restrict__ part,
                                                                 int64_t nrows, uint64_t* __restrict__ out) {
    __shared__ uint64_t red[kBlock];
    for (int c = 0; c < OC_NSTATS; ++c) {
        uint64_t s = 0;
        for (int64_t r = threadIdx.x; r < nrows; r += kBlock) s += part[r * OC_NSTATS + c];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int w = kBlock / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[c] = red[0];
        __syncthreads();
    }
}

thread_local std::string g_last_error;
thread_local uint64_t g_err_gen = 0;  // failures on this thread so far (ErrScope compares)

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    ++g_err_gen;
    return code;
}

int hip_check(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(OC_EHIP, "%s: %s", what, hipGetErrorString(e));
    return OC_OK;
}

// Statistics rows: blocks add into row blockIdx % rows (no-return 64-bit atomics); 256 rows
// keep the adds to one address to a few dozen per launch and let one wave fold them.


int64_t pitch_for(int64_t B) {
    int64_t p = (B + OC_PITCH_ALIGN - 1) / OC_PITCH_ALIGN * OC_PITCH_ALIGN;
    return p < OC_PITCH_ALIGN ? OC_PITCH_ALIGN : p;
}

}  // namespace

struct oc_handle {
    oc_level_desc level;
    int32_t A, K, max_T, device;
    int32_t cus;                // compute units of the device (persistent grids: <= 5 blocks per CU)
    LevelArgs args;
    ocro::RollLevel roll;       // planner rollout tables (nnodes < 0: graph too large)
    uint8_t* roll_blob = nullptr;  // device: the level's rollout table blob (oc_rollout.h)
    int32_t roll_blob_bytes = 0;
    std::vector<uint8_t> roll_blob_host;  // the same blob on the host
    // wide levels (more than 255 cells, u16 cell ids): the tile table of oc_step_wide_kernel
    bool wide = false;
    uint8_t* wide_tiles = nullptr;   // device: tile class per cell (W * H rounded up to 4 bytes)
    uint8_t wide_tiles_host[ocro::kMaxCellsWide];
    int32_t lik_form = OC_LIK_FORM_AUTO;  // oc_set_likelihood_form
    // oc_observe: the tile class per cell (W * H rounded up to 4 bytes), then the static list: the
    // element offset (class - 1) * W * H + cell of every non-Floor square, u16 each
    std::vector<uint8_t> obs_tab_host;
    uint8_t* obs_tab = nullptr;      // device copy
    int32_t obs_static_off = 0, obs_nstatic = 0;
    int32_t obs_nt = 0;              // non-temporal output stores (OC_OBS_STORES=nt|plain overrides)
    int32_t obs_tile = ocob::kMaxTileEnvs;  // envs per block at most (OC_OBS_TILE=64|32|16|... overrides)
    // oc_reset_random: the start distribution (oc_startdist.h).  start_ok: agent_ok [A][W*H] then
    // item_ok [W*H], the effective masks; start_tab_host / start_tab: the table blob and its device
    // copy; start_err: why there is no valid distribution (the defaults are too short for the level)
    std::vector<uint8_t> start_ok, start_tab_host;
    uint8_t* start_tab = nullptr;
    ocsd::StartArgs start{};
    int start_rc = OC_OK;
    std::string start_err;
    mutable std::string last_error;       // oc_get_last_error: the last failed call on this handle
};

// An entry point's failure is also recorded on its handle (oc_get_last_error): the scope sees
// whether fail() ran on this thread while the call was in progress.
struct ErrScope {
    const oc_handle* h;
    uint64_t gen;
    explicit ErrScope(const oc_handle* hh) : h(hh), gen(g_err_gen) {}
    ~ErrScope() {
        if (h != nullptr && g_err_gen != gen) h->last_error = g_last_error;
    }
};

// Device entry points refuse a host-only handle (oc_create with OC_DEVICE_HOST).
#define OC_NEED_DEVICE(h_) \
    if ((h_)->device < 0) return fail(OC_EINVAL, "host-only handle (OC_DEVICE_HOST): this entry point needs a device")

// Statistics rows, shared by the blocks of every kernel modulo the row count; oc_step_n's
// completion tickets follow them (ticket_base; zero between launches).
int64_t stats_rows(const oc_handle*, int64_t B) {
    const int64_t need = pitch_for(B) / kEnvsPerBlock;
    return need < kStatRows ? need : kStatRows;
}

// Kernel and worker templates are picked by generic lambdas that take their template arguments as
// tag values.  A lambda returns OC_OK or the failing code, and the dispatcher returns that.
template <int V>
using IntC = std::integral_constant<int, V>;
template <bool V>
using BoolC = std::bool_constant<V>;

// f(IntC<A>, IntC<K>): the supported (agents, item slots) shapes, listed here and nowhere else.
template <class F>
static int dispatch_ak(int A, int K, F&& f) {
    switch (A * 100 + K) {
        case 104: return f(IntC<1>{}, IntC<4>{});
        case 204: return f(IntC<2>{}, IntC<4>{});
        case 304: return f(IntC<3>{}, IntC<4>{});
        case 404: return f(IntC<4>{}, IntC<4>{});
        case 108: return f(IntC<1>{}, IntC<8>{});
        case 208: return f(IntC<2>{}, IntC<8>{});
        case 308: return f(IntC<3>{}, IntC<8>{});
        case 408: return f(IntC<4>{}, IntC<8>{});
        case 116: return f(IntC<1>{}, IntC<16>{});
        case 216: return f(IntC<2>{}, IntC<16>{});
        case 316: return f(IntC<3>{}, IntC<16>{});
        case 416: return f(IntC<4>{}, IntC<16>{});
        default: return fail(OC_EINVAL, "unsupported (A,K)=(%d,%d)", A, K);
    }
}

// f(A, K, BoolC<wide>): narrow (byte cell ids) or wide (u16) states -- render, observe, progress,
// checksum.
template <class F>
static int dispatch_w(const oc_handle* h, F&& f) {
    return dispatch_ak(h->A, h->K, [&](auto a, auto k) {
        return h->wide ? f(a, k, BoolC<true>{}) : f(a, k, BoolC<false>{});
    });
}

// f(A, K, IntC<MODE>), the narrow step: 4-slot levels of the common class (H <= 8, W*H <= 128,
// presence masks: every shipped kitchen) take the MODE 0 build of the SWAR step, everything else
// MODE 1.
template <class F>
static int dispatch_step(const oc_handle* h, F&& f) {
    const ocsw::SwarLevel& sw = h->args.sw;
    const bool common = !sw.tall && !sw.big && !sw.counts && !sw.edge;
    return dispatch_ak(h->A, h->K, [&](auto a, auto k) {
        if constexpr (decltype(k)::value == 4) {
            if (common) return f(a, k, IntC<0>{});
        }
        return f(a, k, IntC<1>{});
    });
}

// f(A, K, BoolC<W>, BoolC<GD>), the planner kernels: narrow (byte cell ids) or wide (u16) rows;
// the distance table in LDS (GD false) or in device memory (GD: every wide level, and a narrow
// level whose graph has more than ocro::kMaxNodes nodes).
template <class F>
static int dispatch_plan(const oc_handle* h, F&& f) {
    return dispatch_ak(h->A, h->K, [&](auto a, auto k) {
        if (h->wide) return f(a, k, BoolC<true>{}, BoolC<true>{});
        if (h->roll.dist_global) return f(a, k, BoolC<false>{}, BoolC<true>{});
        return f(a, k, BoolC<false>{}, BoolC<false>{});
    });
}

// Threads of a host entry point: nthreads (0: the machine's), at most one per min_units of the
// call's units, at least one.
static int64_t host_threads(int32_t nthreads, int64_t units, int64_t min_units) {
    if (nthreads == 0) nthreads = (int32_t)std::thread::hardware_concurrency();
    const int64_t most = (units + min_units - 1) / min_units;
    const int64_t nt = nthreads < most ? nthreads : most;
    return nt < 1 ? 1 : nt;
}

// fn(i) for the ranges i in [0, nt): ranges 1..nt-1 start on workers and range 0 runs on the
// calling thread while they work; ranges whose thread cannot be started run here too.  The first
// failing range's code and message come back through fail().
template <class Fn>
static int run_ranges(int64_t nt, Fn&& fn) {
    std::vector<int> rcs((size_t)nt, OC_OK);
    std::vector<std::string> msgs((size_t)nt);
    auto run = [&](int64_t i) {
        rcs[(size_t)i] = fn(i);
        if (rcs[(size_t)i] != OC_OK) msgs[(size_t)i] = g_last_error;  // thread-local: the range's own
    };
    std::vector<std::thread> pool;
    int64_t started = 1;
    try {
        for (; started < nt; ++started) pool.emplace_back(run, started);
    } catch (const std::exception&) {  // no more threads: the rest of the ranges run here
    }
    run(0);
    for (int64_t i = started; i < nt; ++i) run(i);
    for (auto& t : pool) t.join();
    for (int64_t i = 0; i < nt; ++i)
        if (rcs[(size_t)i] != OC_OK) return fail(rcs[(size_t)i], "%s", msgs[(size_t)i].c_str());
    return OC_OK;
}

// A host entry point's loop: the call's units (envs, or words of four envs) split into one range
// per thread of host_threads(nthreads, units, min_units), fn(A, K, BoolC<wide>, u0, u1) for each.
template <class Fn>
static int host_ranges(const oc_handle* h, int32_t nthreads, int64_t units, int64_t min_units, Fn&& fn) {
    const int64_t nt = host_threads(nthreads, units, min_units);
    return run_ranges(nt, [&](int64_t i) {
        return dispatch_w(h, [&](auto a, auto k, auto w) { return fn(a, k, w, units * i / nt, units * (i + 1) / nt); });
    });
}

// oc_cpu_nav_policy's worker: rows [e0, e1), each the whole-row ocro::RowOps::policy
template <int A, int K, bool W>
static void host_policy_range(const RollArgs& R, const PolicyArgs& Q, const uint8_t* blob, const uint8_t* sin,
                              const uint8_t* alloc, uint8_t* actions, double* probs, uint8_t* out_flags, int64_t e0,
                              int64_t e1) {
    const int64_t P = R.pitch;
    for (int64_t e = e0; e < e1; ++e) {
        const int ai = alloc != nullptr ? alloc[e] : 0;
        double p[25] = {};
        int f = OC_POL_BADALLOC;
        if (ai < R.nsub) {
            const ocro::Sub& s = R.subs[ai];
            ocro::RowOps<A, K, W, true, true> ops(R.L, blob);
            int a0, a1;
            f = ops.policy(load_row<A, K, W>(sin, P, e), s, Q.beta, Q.nap, Q.mode,
                           ocro::policy_u(Q.seed, Q.env_offset + e, Q.step, s.agent[0]), p, a0, a1);
            actions[s.agent[0] * P + e] = (uint8_t)a0;
            if (s.n == 2) actions[s.agent[1] * P + e] = (uint8_t)a1;
        }
        if (probs != nullptr)
            for (int k = 0; k < Q.num_cand; ++k) probs[k * P + e] = p[k];
        out_flags[e] = (uint8_t)f;
    }
}

// One launch of an n-step call: steps [r0, r0 + m) of it.
struct StepLaunch {
    const uint8_t* src;  // the state it starts from
    uint8_t* so;         // where its final state goes; null: its last trajectory slot already holds it
    const uint8_t* ac;   // its steps' actions
    uint8_t *tr, *ex, *cm;  // its steps' trajectory slots, executed actions and collision masks (or null)
    int m;
    bool last;
};

// Splits an n-step call over states of NP planes into equal launches of at most 4,096 steps whose
// buffer offsets (trajectory, actions) stay < 2 GiB, and calls launch(StepLaunch) for each.  With
// a trajectory, a launch's final state is its last trajectory slot: the next launch starts from
// there, and sout is written by the last launch only (and not at all when it is the trajectory's
// last state).  So no launch reads a buffer it also writes.
template <class Launch>
static int split_steps(int64_t NP, int64_t P, int A, const void* sin, void* sout, const uint8_t* act, void* traj,
                       uint8_t* ex, uint8_t* coll, int32_t n, Launch&& launch) {
    if (NP * P >= (1ll << 31)) return fail(OC_EINVAL, "batch too large for one launch (state must be < 2 GiB)");
    int64_t per = ((1ll << 31) - 1) / (NP * P);
    if (per > 4096) per = 4096;
    per = (n + (n + per - 1) / per - 1) / ((n + per - 1) / per);  // equal launches
    const uint8_t* last_slot = traj ? (const uint8_t*)traj + (int64_t)(n - 1) * NP * P : nullptr;
    const bool out_is_last = traj != nullptr && (const uint8_t*)sout == last_slot;
    const uint8_t* src = (const uint8_t*)sin;
    for (int64_t r0 = 0; r0 < n; r0 += per) {
        StepLaunch s;
        s.m = (int)(n - r0 < per ? n - r0 : per);
        s.last = r0 + s.m >= n;
        s.src = src;
        s.so = (traj != nullptr && !s.last) || (out_is_last && s.last) ? nullptr : (uint8_t*)sout;
        s.ac = act + r0 * A * P;
        s.tr = traj ? (uint8_t*)traj + r0 * NP * P : nullptr;
        s.ex = ex ? ex + r0 * A * P : nullptr;
        s.cm = coll ? coll + r0 * P : nullptr;
        if (const int rc = launch(s)) return rc;
        src = traj != nullptr ? s.tr + (int64_t)(s.m - 1) * NP * P : (const uint8_t*)sout;
    }
    return OC_OK;
}

// A level table's device copy, or nullptr (and no HIP error left behind) when there is no device
// to put it on, e.g. a CPU-only build check: the entry points that need the table then refuse.
static uint8_t* upload(int device, const void* src, size_t bytes) {
    uint8_t* d = nullptr;
    if (hipSetDevice(device) == hipSuccess && hipMalloc(&d, bytes) == hipSuccess &&
        hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) == hipSuccess)
        return d;
    (void)hipGetLastError();
    return nullptr;
}

// the node table and the distances, as u8 (oc_reachability) or u16 (oc_reachability16)
static int reachability(const oc_handle* h, int32_t* num_nodes, uint16_t* node_of, int64_t node_of_len, void* dist,
                        int64_t dist_len, int out_bytes) {
    if (h == nullptr || num_nodes == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    if (h->roll.nnodes < 0)
        return fail(OC_ELEVEL, "reachability graph exceeds %d nodes (a level of more than %d cells)", ocro::kMaxNodesWide,
                    ocro::kMaxCellsWide);
    const int n = h->roll.nnodes, cells = h->level.width * h->level.height;
    *num_nodes = n;
    if (node_of != nullptr) {
        if (node_of_len < (int64_t)cells * 5) return fail(OC_EINVAL, "node_of needs %d entries", cells * 5);
        memcpy(node_of, h->roll_blob_host.data() + h->roll.node_off, (size_t)cells * 5 * sizeof(uint16_t));
    }
    if (dist != nullptr) {
        if (dist_len < (int64_t)n * n) return fail(OC_EINVAL, "dist needs %d entries", n * n);
        const uint8_t* src = h->roll_blob_host.data() + h->roll.dist_off;
        const size_t nn = (size_t)n * n;
        if (out_bytes == 1) {
            if (h->roll.dist16)
                return fail(OC_ELEVEL, "a BFS distance of 255 or more: the u8 table cannot hold it (oc_reachability16)");
            memcpy(dist, src, nn);
        } else if (h->roll.dist16) {
            memcpy(dist, src, nn * 2);
        } else {
            for (size_t i = 0; i < nn; ++i) ((uint16_t*)dist)[i] = src[i] == ocro::kNone ? (uint16_t)0xFFFF : src[i];
        }
    }
    return OC_OK;
}

// Wide levels: n steps of oc_step_wide_kernel (oc_step: n = 1), statistics folded by
// oc_stats_reduce when totals are asked for.
static int step_wide(const oc_handle* h, const void* sin, void* sout, const uint8_t* act, void* traj, uint8_t* ex,
                     uint8_t* coll, uint64_t* stats, uint64_t* totals, int64_t B, int32_t n, void* stream) {
    if (h->wide_tiles == nullptr) return fail(OC_EHIP, "level tables not on the device");
    const WideArgs R{h->args.sw, (h->level.width * h->level.height + 3) / 4, pitch_for(B), B};
    // one lane per 4 envs; up to 8 blocks per CU (grid-stride past that)
    const int64_t need = ((B + kEPL - 1) / kEPL + kBlock - 1) / kBlock, cap = (int64_t)h->cus * 8;
    const dim3 grid((unsigned)(need < cap ? need : cap));
    const uint32_t rows = (uint32_t)stats_rows(h, B);
    hipStream_t st = (hipStream_t)stream;
    const int rc = split_steps(ocly::num_planes(h->A, h->K, true), R.pitch, h->A, sin, sout, act, traj, ex, coll, n,
                               [&](const StepLaunch& s) {
        return dispatch_ak(h->A, h->K, [&](auto a, auto k) {
            hipLaunchKernelGGL((oc_step_wide_kernel<a(), k()>), grid, dim3(kBlock), 0, st, R, h->wide_tiles, s.src,
                               s.so, s.ac, s.tr, s.ex, s.cm, stats, rows, s.m);
            return hip_check("oc_step (wide) launch");
        });
    });
    if (rc != OC_OK) return rc;
    return totals != nullptr ? oc_stats_reduce(h, stats, B, totals, stream) : OC_OK;
}

// Shared argument block of oc_rollout / oc_nav_likelihood / oc_subtask_bounds: level tables +
// validated subtasks.  rollout: oc_rollout's call (Level-1 configurations allowed; the
// node-to-square table staged only for launches of one round of blocks, below).
static int roll_args(const oc_handle* h, const oc_subtask* subtasks, int32_t num_subtasks, int64_t B, RollArgs& R,
                     bool rollout = false, bool host = false) {
    for (int i = 0; i < num_subtasks && subtasks != nullptr; ++i)
        if (subtasks[i].level != OC_LEVEL0 && !rollout)
            return fail(OC_EINVAL, "subtask %d: only oc_rollout takes OC_LEVEL1", i);
    if (num_subtasks < 1 || num_subtasks > OC_MAX_SUBTASKS) return fail(OC_EINVAL, "num_subtasks %d", num_subtasks);
    if (h->roll.nnodes < 0)
        return fail(OC_ELEVEL, "reachability graph exceeds %d nodes (a level of more than %d cells)", ocro::kMaxNodesWide,
                    ocro::kMaxCellsWide);
    if (h->roll_blob == nullptr && !host) return fail(OC_EHIP, "rollout tables not on the device");
    R.L = h->roll;
    R.nsub = num_subtasks;
    R.blob_words = h->roll.lds_bytes / 4;  // staged in LDS: the whole blob, or the tables before the distances
    if (R.L.sq_off != 0 && rollout && B > (int64_t)h->cus * kRollBlock) {
        // The node-to-square table (the blob's tail) shortens the one-agent Merge bound from ~3.8
        // to 1.1-2.0 us of a wave.  A rollout launch of one round of blocks (the planner's latency
        // shape) gains (9.03 -> 8.87 us at 4096 rows); past that every rollout block stages 40%
        // more table for one row per lane (11.16-11.34 -> 11.35-11.51 us at 2^18: tools/rollx.hip,
        // profiles/r06/pass_i), so larger rollouts search B's approach nodes as before.  The bounds
        // kernel (many configurations per staged table) gains at every size, 96-97 -> 85 us at C5,
        // and the likelihood kernels are unchanged (profiles/r06/pass_w).
        R.blob_words = R.L.sq_off / 4;
        R.L.sq_off = 0;
    }
    R.pitch = pitch_for(B);
    R.B = B;
    for (int i = 0; i < num_subtasks; ++i) {
        const oc_subtask& s = subtasks[i];
        if (s.kind < OC_SUB_NONE || s.kind > OC_SUB_DELIVER) return fail(OC_EINVAL, "subtask %d kind %d", i, s.kind);
        if (s.num_agents < 1 || s.num_agents > 2) return fail(OC_EINVAL, "subtask %d: %d agents", i, s.num_agents);
        for (int q = 0; q < s.num_agents; ++q)
            if (s.agent[q] >= h->A) return fail(OC_EINVAL, "subtask %d: agent %d", i, s.agent[q]);
        if (s.num_agents == 2 && s.agent[0] >= s.agent[1]) return fail(OC_EINVAL, "subtask %d: agents not ascending", i);
        ocro::Sub& d = R.subs[i];
        d.kind = s.kind;
        d.n = s.num_agents;
        d.agent[0] = s.agent[0];
        d.agent[1] = s.num_agents == 2 ? s.agent[1] : s.agent[0];
        d.start[0] = s.start_mask[0];
        d.start[1] = s.start_mask[1];
        if (s.level > OC_LEVEL1) return fail(OC_EINVAL, "subtask %d: level %d", i, s.level);
        d.goal = s.goal_mask;
        d.count = s.goal_count;
        d.level = s.level;
        d.pad = 0;
    }
    return OC_OK;
}

// The planner kernels stage the level's table blob in dynamic LDS.  Past the 64 KB a launch gets
// by default (graphs of more than ~245 nodes) the kernel must be allowed more, up to the CU's
// 160 KB; the kernel's static LDS counts against the same limit.
constexpr int kLdsPerCu = 160 * 1024;
static_assert((8 * kBlock) % kRollBlock == 0, "oc_rollout's grid: whole rollout blocks per CU");
constexpr int kPlanStaticLds = 16 * 1024;  // an upper bound of a planner kernel's static LDS (the subtask rows)
static int allow_dyn_lds(const void* kernel, int dyn, int static_lds) {
    // static_lds: an upper bound of the kernel's static LDS; together with `dyn` within the default
    // 64 KB nothing needs to be set
    if (dyn + static_lds <= 64 * 1024) return OC_OK;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, kernel) != hipSuccess) return hip_check("hipFuncGetAttributes");
    if ((int64_t)fa.sharedSizeBytes + dyn > kLdsPerCu)
        return fail(OC_ELEVEL, "level tables (%d B) and the kernel's LDS (%d B) exceed %d B", dyn,
                    (int)fa.sharedSizeBytes, kLdsPerCu);
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, dyn) != hipSuccess)
        return hip_check("hipFuncSetAttribute");
    return OC_OK;
}

// One launch of a planner kernel: R's staged tables as its dynamic LDS, R its first argument.
// what: the launch's name in a HIP error's message.
template <class Kernel, class... Args>
static int launch_staged(Kernel kernel, dim3 grid, dim3 block, const RollArgs& R, hipStream_t st, const char* what,
                         int static_lds, Args... args) {
    if (const int rc = allow_dyn_lds((const void*)kernel, R.blob_words * 4, static_lds)) return rc;
    hipLaunchKernelGGL(kernel, grid, block, R.blob_words * 4, st, R, args...);
    return hip_check(what);
}

// Blocks of a launch over B envs, rows_per_block each: one round of blocks, at most blocks_per_cu
// per CU (the kernels stride over the rest).
static unsigned env_grid(const oc_handle* h, int64_t B, int64_t rows_per_block, int64_t blocks_per_cu) {
    const int64_t need = (B + rows_per_block - 1) / rows_per_block, cap = (int64_t)h->cus * blocks_per_cu;
    return (unsigned)(need < cap ? need : cap);
}

// The one- (a1 < 0) or two-agent Level-0 row of a partner entry point's subtask `src`.
static oc_subtask level0_row(const oc_subtask& src, int a0, int a1 = -1) {
    oc_subtask d{};
    d.kind = src.kind;
    d.num_agents = a1 < 0 ? 1 : 2;
    d.agent[0] = (uint8_t)a0;
    if (a1 >= 0) d.agent[1] = (uint8_t)a1;
    d.start_mask[0] = src.start_mask[0];
    d.start_mask[1] = src.start_mask[1];
    d.goal_mask = src.goal_mask;
    d.level = OC_LEVEL0;
    return d;
}

// A partner entry point's agent list: M distinct agents below A.  what: the message's prefix.
static int check_agents(const char* what, const uint8_t* agents, int M, int A) {
    for (int m = 0; m < M; ++m) {
        if (agents[m] >= A) return fail(OC_EINVAL, "%s: agent %d", what, agents[m]);
        for (int q = 0; q < m; ++q)
            if (agents[q] == agents[m]) return fail(OC_EINVAL, "%s: agent %d listed twice", what, agents[m]);
    }
    return OC_OK;
}

// oc_observe / oc_cpu_observe: the arguments both check, and the level's side of ObsArgs
static int observe_args(const oc_handle* h, const void* state, const void* obs, const uint8_t* action_mask,
                        int32_t dtype, int32_t view_agent, int64_t B, ocob::ObsArgs& R) {
    if (state == nullptr || B < 0) return fail(OC_EINVAL, "bad argument");
    if (obs == nullptr && action_mask == nullptr) return fail(OC_EINVAL, "observe: obs and action_mask are both NULL");
    if (dtype != OC_OBS_U8 && dtype != OC_OBS_F16) return fail(OC_EINVAL, "observe: dtype %d (OC_OBS_U8 or OC_OBS_F16)", dtype);
    if (view_agent < -1 || view_agent >= h->A)
        return fail(OC_EINVAL, "observe: view_agent %d outside [-1, %d)", view_agent, h->A);
    if (((uintptr_t)state & 15u) || ((uintptr_t)action_mask & 3u) || (dtype == OC_OBS_F16 && ((uintptr_t)obs & 1u)))
        return fail(OC_EINVAL, "misaligned buffer");
    R = ocob::ObsArgs{};
    R.W = h->level.width;
    R.H = h->level.height;
    R.HW = R.W * R.H;
    R.C = OC_OBS_CHANNELS(h->A);
    R.CHW = R.C * R.HW;
    R.counts = h->level.encoding == OC_ENC_COUNTS;
    R.rot = view_agent < 0 ? 0 : view_agent;
    R.nstatic = h->obs_nstatic;
    R.nt = h->obs_nt;
    R.pitch = pitch_for(B);
    R.B = B;
    return OC_OK;
}

// oc_progress / oc_cpu_progress: the arguments both check, and the call's ProgArgs
static int progress_args(const oc_handle* h, const void* state_prev, const void* states, int32_t n,
                         const oc_subtask* subtasks, int32_t num_subtasks, const float* weights, const uint8_t* counts,
                         const uint8_t* events, const float* reward, int64_t B, ocpg::ProgArgs& R) {
    if (state_prev == nullptr || states == nullptr || subtasks == nullptr || B < 0) return fail(OC_EINVAL, "bad argument");
    if (n < 1) return fail(OC_EINVAL, "progress: n = %d (at least 1)", n);
    if (num_subtasks < 1 || num_subtasks > OC_MAX_SUBTASKS)
        return fail(OC_EINVAL, "progress: num_subtasks %d outside [1, %d]", num_subtasks, OC_MAX_SUBTASKS);
    if (counts == nullptr && events == nullptr && reward == nullptr)
        return fail(OC_EINVAL, "progress: counts, events and reward are all NULL");
    if (((uintptr_t)state_prev & 3u) || ((uintptr_t)states & 3u) || ((uintptr_t)counts & 3u) ||
        ((uintptr_t)events & 3u) || ((uintptr_t)reward & 15u))
        return fail(OC_EINVAL, "misaligned buffer");
    R = ocpg::ProgArgs{};
    for (int i = 0; i < num_subtasks; ++i) {
        const int32_t kind = subtasks[i].kind;
        if (kind != OC_SUB_NONE && kind != OC_SUB_CHOP && kind != OC_SUB_MERGE && kind != OC_SUB_DELIVER)
            return fail(OC_EINVAL, "progress: subtask %d has kind %d", i, kind);
        R.sub[i] = (uint32_t)kind << 8 | subtasks[i].goal_mask;
        R.weight[i] = weights != nullptr ? weights[i] : 1.0f;
    }
    R.W = h->level.width;
    R.tile_words = (h->level.width * h->level.height + 3) / 4;
    R.n = n;
    R.S = num_subtasks;
    R.planes = OC_PROGRESS_EVENT_PLANES(num_subtasks);
    R.pitch = pitch_for(B);
    R.B = B;
    R.state_bytes = (int64_t)ocly::num_planes(h->A, h->K, h->wide) * R.pitch;
    return OC_OK;
}

// The start distribution of oc_set_start_cells(h, agent_ok, item_ok) (NULL: the default lists of
// include/oc_engine.h): checks it and builds the effective masks, the list lengths and the table
// blob (ocsd::table_bytes).  Returns OC_OK, or the code with its message in `err`; the handle is not
// touched.
static int build_start(const oc_handle* h, const uint8_t* agent_ok, const uint8_t* item_ok, std::vector<uint8_t>& ok,
                       std::vector<uint8_t>& tab, ocsd::StartArgs& R, std::string& err) {
    const oc_level_desc& lv = h->level;
    const int W = lv.width, H = lv.height, cells = W * H, A = h->A;
    char msg[256];
    auto refuse = [&](int code) {
        err = msg;
        return code;
    };
    ok.assign((size_t)(A + 1) * cells, 0);
    for (int i = 0; i < A; ++i) {
        uint8_t* m = ok.data() + (size_t)i * cells;
        if (agent_ok != nullptr) {
            for (int c = 0; c < cells; ++c) {
                m[c] = agent_ok[(size_t)i * cells + c] != 0;
                if (m[c] && lv.tiles[c] != OC_TILE_FLOOR) {
                    snprintf(msg, sizeof msg, "start cells: agent %d cell %d (%d,%d) is not Floor", i, c, c % W, c / W);
                    return refuse(OC_EINVAL);
                }
            }
        } else {  // the Floor cells 4-connected through Floor to spawn i
            std::vector<int> todo{lv.spawn_y[i] * W + lv.spawn_x[i]};
            m[todo[0]] = 1;
            while (!todo.empty()) {
                const int c = todo.back(), x = c % W, y = c / W;
                todo.pop_back();
                const int nb[4] = {y + 1 < H ? c + W : -1, y > 0 ? c - W : -1, x > 0 ? c - 1 : -1, x + 1 < W ? c + 1 : -1};
                for (int n : nb)
                    if (n >= 0 && lv.tiles[n] == OC_TILE_FLOOR && !m[n]) {
                        m[n] = 1;
                        todo.push_back(n);
                    }
            }
        }
    }
    uint8_t* mi = ok.data() + (size_t)A * cells;
    for (int c = 0; c < cells; ++c) {
        const int x = c % W, y = c / W;
        if (item_ok != nullptr) {
            mi[c] = item_ok[c] != 0;
            if (mi[c] && lv.tiles[c] != OC_TILE_COUNTER) {
                snprintf(msg, sizeof msg, "start cells: item cell %d (%d,%d) is not a Counter", c, x, y);
                return refuse(OC_EINVAL);
            }
        } else {  // a Counter with a Floor 4-neighbour
            const bool fl = (y + 1 < H && lv.tiles[c + W] == OC_TILE_FLOOR) || (y > 0 && lv.tiles[c - W] == OC_TILE_FLOOR) ||
                            (x > 0 && lv.tiles[c - 1] == OC_TILE_FLOOR) || (x + 1 < W && lv.tiles[c + 1] == OC_TILE_FLOOR);
            mi[c] = lv.tiles[c] == OC_TILE_COUNTER && fl;
        }
    }
    R = ocsd::StartArgs{};
    R.S = (cells + 1) & ~1;
    R.S2 = (cells + 3) & ~3;
    R.items = lv.num_items;
    tab.assign((size_t)ocsd::table_bytes(A, R.S, R.S2), 0);
    uint16_t* L = (uint16_t*)tab.data();
    for (int i = 0; i <= A; ++i) {
        int n = 0;
        for (int c = 0; c < cells; ++c)
            if (ok[(size_t)i * cells + c]) L[i * R.S + n++] = (uint16_t)c;
        if (i < A) {
            R.nA[i] = n;
            if (n < A) {
                snprintf(msg, sizeof msg, "start cells: agent %d has %d cells, fewer than the %d agents", i, n, A);
                return refuse(agent_ok != nullptr ? OC_EINVAL : OC_ELEVEL);
            }
        } else {
            R.nI = n;
            if (n < lv.num_items) {
                snprintf(msg, sizeof msg, "start cells: %d item cells, fewer than the level's %d items", n, lv.num_items);
                return refuse(item_ok != nullptr ? OC_EINVAL : OC_ELEVEL);
            }
        }
    }
    for (int c = 0; c < cells; ++c) L[(A + 1) * R.S + c] = (uint16_t)((c % W) | ((c / W) << 8));
    uint8_t* okb = tab.data() + (size_t)(A + 2) * R.S * 2;
    for (int i = 0; i < A; ++i) memcpy(okb + (size_t)i * R.S2, ok.data() + (size_t)i * cells, (size_t)cells);
    return OC_OK;
}

// oc_reset_random / oc_cpu_reset_random: the arguments both check, and the call's StartArgs
static int start_args(const oc_handle* h, const void* state, int64_t B, int64_t env_offset, uint64_t seed, uint64_t round,
                      int32_t what, bool masked, ocsd::StartArgs& R) {
    if (state == nullptr || B < 0 || env_offset < 0) return fail(OC_EINVAL, "bad argument");
    if (what == 0 || (what & ~(OC_START_AGENTS | OC_START_ITEMS)))
        return fail(OC_EINVAL, "reset_random: what = %d (OC_START_AGENTS | OC_START_ITEMS, not 0)", what);
    if (h->start_rc != OC_OK) return fail(h->start_rc, "%s", h->start_err.c_str());
    R = h->start;
    R.what = what;
    R.masked = masked ? 1 : 0;
    R.pitch = pitch_for(B);
    R.B = B;
    R.env_offset = env_offset;
    R.seed = seed;
    R.round = round;
    return OC_OK;
}

extern "C" {

int oc_abi_version(void) { return OC_ABI_VERSION; }

const char* oc_last_error(void) { return g_last_error.c_str(); }

int oc_get_last_error(const oc_handle* h, char* buf, int64_t size) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    const int64_t n = (int64_t)h->last_error.size();
    if (buf != nullptr && size > 0) {
        const int64_t c = n < size - 1 ? n : size - 1;
        memcpy(buf, h->last_error.data(), (size_t)c);
        buf[c] = '\0';
    }
    return (int)n;
}

int oc_set_likelihood_form(oc_handle* h, int32_t form) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    if (form != OC_LIK_FORM_AUTO && form != OC_LIK_FORM_GROUPED) return fail(OC_EINVAL, "likelihood form %d", form);
    h->lik_form = form;
    return OC_OK;
}

int oc_create(const oc_level_desc* lv, int32_t num_agents, int32_t max_T, int32_t device, oc_handle** out) {
    if (lv == nullptr || out == nullptr) return fail(OC_EINVAL, "null argument");
    const int W = lv->width, H = lv->height;
    if (W < 3 || H < 3 || W > 255 || H > 255 || W * H > OC_MAX_CELLS)
        return fail(OC_ELEVEL, "grid %dx%d: width and height 3..255 and at most %d cells", W, H, OC_MAX_CELLS);
    if (num_agents < 1 || num_agents > OC_MAX_AGENTS) return fail(OC_EINVAL, "num_agents %d", num_agents);
    if (lv->num_spawns < num_agents || lv->num_spawns > OC_MAX_AGENTS) return fail(OC_ELEVEL, "num_spawns %d", lv->num_spawns);
    if (lv->num_items < 0 || lv->num_items > OC_MAX_ITEMS) return fail(OC_ELEVEL, "num_items %d", lv->num_items);
    if (lv->num_goals < 1 || lv->num_goals > OC_MAX_GOALS) return fail(OC_ELEVEL, "num_goals %d", lv->num_goals);
    if (max_T < 0 || max_T > 65535) return fail(OC_EINVAL, "max_T %d", max_T);
    if (device < OC_DEVICE_HOST) return fail(OC_EINVAL, "device %d", device);
    const bool host_only = device == OC_DEVICE_HOST;  // no HIP call at all
    const bool wide = W * H > ocro::kMaxCells;  // u16 cell ids: step4w (oc_step_wide_kernel)
    LevelArgs L{};
    int done_cell = -1;
    for (int c = 0; c < W * H; ++c) {
        const int t = lv->tiles[c];
        if (t < OC_TILE_FLOOR || t > OC_TILE_DELIVERY) return fail(OC_ELEVEL, "tile %d at cell %d", t, c);
        if (!wide) L.cls4[c >> 2] |= (uint32_t)ocsw::tile_class(t) << (8 * (c & 3));
        if (t == OC_TILE_DELIVERY && done_cell < 0) done_cell = c;
    }
    if (done_cell < 0) return fail(OC_ELEVEL, "no Delivery tile");
    if (lv->encoding != OC_ENC_PRESENCE && lv->encoding != OC_ENC_COUNTS)
        return fail(OC_EINVAL, "encoding %d", lv->encoding);
    const bool counts = lv->encoding == OC_ENC_COUNTS;
    uint32_t seen_food = 0;
    int per_food[3] = {0, 0, 0};
    const int K = lv->num_items <= 4 ? 4 : (lv->num_items <= 8 ? 8 : 16);
    uint16_t cell[16];
    uint8_t mask[16], cell8[16];
    for (int j = 0; j < 16; ++j) {
        cell[j] = wide ? (uint16_t)OC_LOC_DEAD16 : (uint16_t)OC_LOC_DEAD;
        mask[j] = 0;
    }
    for (int j = 0; j < lv->num_items; ++j) {
        const int c = lv->item_cell[j], m = lv->item_mask[j];
        if (c >= W * H || lv->tiles[c] == OC_TILE_FLOOR) return fail(OC_ELEVEL, "item %d not on a counter", j);
        if (counts) {  // a level item is one content: a fresh food (Fresh bit + count 1) or a Plate
            const int f = m == (int)(OC_MC_FRESH | OC_MC_TOMATO) ? 0 : m == (int)(OC_MC_FRESH | OC_MC_LETTUCE) ? 1
                          : m == (int)(OC_MC_FRESH | OC_MC_ONION) ? 2 : -1;
            if (f < 0 && m != (int)OC_MC_PLATE) return fail(OC_ELEVEL, "item mask 0x%x (counts encoding)", m);
            if (f >= 0 && ++per_food[f] > OC_MC_MAX_PER_FOOD)
                return fail(OC_ELEVEL, "more than %d of one food type (2-bit counts)", OC_MC_MAX_PER_FOOD);
        } else {
            if (m == 0 || (m & 0x80) || (((m >> OC_M_CHOPPED_SHIFT) & 7) & ~(m & 7)))
                return fail(OC_ELEVEL, "item mask 0x%x", m);
            if (seen_food & m & 7u)
                return fail(OC_ELEVEL, "food type present twice: the level needs OC_ENC_COUNTS");
            seen_food |= m & 7u;
        }
        cell[j] = (uint16_t)c;
        mask[j] = (uint8_t)m;
    }
    for (int j = 0; j < 16; ++j) cell8[j] = (uint8_t)cell[j];
    for (int a = 0; a < num_agents; ++a) {
        const int x = lv->spawn_x[a], y = lv->spawn_y[a];
        if (x >= W || y >= H || lv->tiles[y * W + x] != OC_TILE_FLOOR) return fail(OC_ELEVEL, "spawn %d not on Floor", a);
    }
    ocsw::build_swar_level(L.sw, W, H, done_cell, lv->goal_mask, lv->num_goals, max_T, lv->spawn_x, lv->spawn_y,
                           num_agents, cell8, mask, lv->encoding, lv->tiles);
    if (wide) {  // step4w: u16 cells as low / high byte words (the LUTs, x / y and W - 1 stay bytes)
        L.sw.done_rep = (uint32_t)(done_cell & 0xFF) * 0x01010101u;
        L.sw.done_hi_rep = (uint32_t)(done_cell >> 8) * 0x01010101u;
        for (int j = 0; j < 16; ++j) {
            L.sw.tmpl_l[j] = (uint32_t)(cell[j] & 0xFF) * 0x01010101u;
            L.sw.tmpl_lh[j] = (uint32_t)(cell[j] >> 8) * 0x01010101u;
        }
    }
    oc_handle* h = new oc_handle;
    h->wide = wide;
    memset(h->wide_tiles_host, 0, sizeof h->wide_tiles_host);
    for (int c = 0; c < W * H; ++c) h->wide_tiles_host[c] = lv->tiles[c];
    h->level = *lv;
    h->A = num_agents;
    h->K = K;
    h->max_T = max_T;
    h->device = device;
    h->args = L;
    h->cus = 256;  // MI355X; replaced by the device's own count when there is a device
    if (!host_only) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            h->cus = cus;
        else
            (void)hipGetLastError();
    }
    // planner rollout: the static reachability graph's BFS table (world.py:67-108) and the
    // level's other static tables, one blob per level (oc_rollout.h)
    {
        const int n = ocro::build_roll_level(h->roll, h->roll_blob_host, W, H, lv->tiles, lv->encoding);
        if (n < 0) {
            h->roll.nnodes = -1;
        } else if (!host_only) {
            h->roll_blob_bytes = h->roll.blob_bytes;
            // null: rollout unavailable
            h->roll_blob = upload(device, h->roll_blob_host.data(), (size_t)h->roll_blob_bytes);
        }
    }
    if (h->roll.nnodes >= 0) h->roll_blob_bytes = h->roll.blob_bytes;
    // null: oc_cpu_step only
    if (wide && !host_only) h->wide_tiles = upload(device, h->wide_tiles_host, (size_t)((W * H + 3) & ~3));
    {  // oc_observe's level table
        const int cells = W * H, off = (cells + 3) & ~3;
        std::vector<uint16_t> st;
        for (int c = 0; c < cells; ++c)
            if (lv->tiles[c] != OC_TILE_FLOOR) st.push_back((uint16_t)((lv->tiles[c] - 1) * cells + c));
        h->obs_static_off = off;
        h->obs_nstatic = (int32_t)st.size();
        h->obs_tab_host.assign((size_t)off + 2 * st.size() + 2, 0);
        memcpy(h->obs_tab_host.data(), lv->tiles, (size_t)cells);
        if (!st.empty()) memcpy(h->obs_tab_host.data() + off, st.data(), 2 * st.size());
        if (const char* e = getenv("OC_OBS_STORES")) h->obs_nt = strcmp(e, "nt") == 0 ? 1 : 0;
        if (const char* e = getenv("OC_OBS_TILE")) {  // measurement knob: a power of two up to kMaxTileEnvs
            const int v = atoi(e);
            if (v >= 1 && v <= ocob::kMaxTileEnvs && (v & (v - 1)) == 0) h->obs_tile = v;
        }
        // null: oc_cpu_observe only
        if (!host_only) h->obs_tab = upload(device, h->obs_tab_host.data(), h->obs_tab_host.size());
    }
    // oc_reset_random's default start distribution; a level it does not fit still loads, and the
    // start calls refuse it with the message kept here
    h->start_rc = build_start(h, nullptr, nullptr, h->start_ok, h->start_tab_host, h->start, h->start_err);
    if (h->start_rc == OC_OK && !host_only)  // null: oc_cpu_reset_random only
        h->start_tab = upload(device, h->start_tab_host.data(), h->start_tab_host.size());
    *out = h;
    return OC_OK;
}

int oc_reachability(const oc_handle* h, int32_t* num_nodes, uint16_t* node_of, int64_t node_of_len, uint8_t* dist,
                    int64_t dist_len) {
    return reachability(h, num_nodes, node_of, node_of_len, dist, dist_len, 1);
}

int oc_reachability16(const oc_handle* h, int32_t* num_nodes, uint16_t* node_of, int64_t node_of_len, uint16_t* dist,
                      int64_t dist_len) {
    return reachability(h, num_nodes, node_of, node_of_len, dist, dist_len, 2);
}

int oc_destroy(oc_handle* h) {
    if (h != nullptr && h->roll_blob != nullptr) (void)hipFree(h->roll_blob);
    if (h != nullptr && h->wide_tiles != nullptr) (void)hipFree(h->wide_tiles);
    if (h != nullptr && h->obs_tab != nullptr) (void)hipFree(h->obs_tab);
    if (h != nullptr && h->start_tab != nullptr) (void)hipFree(h->start_tab);
    delete h;
    return OC_OK;
}

int oc_get_layout(const oc_handle* h, int64_t B, oc_layout* out) {
    if (h == nullptr || out == nullptr || B < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    const ocly::Layout l = ocly::layout(h->A, h->K, h->wide);
    out->pitch = pitch_for(B);
    out->num_agents = h->A;
    out->num_items = h->K;
    out->plane_agent_x = l.X;
    out->plane_agent_y = l.Y;
    out->plane_agent_hold = l.HOLD;
    out->plane_item_loc = l.LOC;
    out->plane_item_loc_hi = l.LOC_HI;
    out->cell_bytes = h->wide ? 2 : 1;
    out->plane_item_mask = l.MASK;
    out->plane_t = l.T;
    out->plane_flags = l.F;
    out->num_planes = l.NP;
    out->state_bytes = out->num_planes * out->pitch;
    return OC_OK;
}

int oc_reset(const oc_handle* h, void* state, int64_t B, void* stream) {
    if (h == nullptr || state == nullptr || B < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    if (B == 0) return OC_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t P = pitch_for(B);
    const dim3 grid((unsigned)(P / kEnvsPerBlock));
    return dispatch_w(h, [&](auto a, auto k, auto w) {
        hipLaunchKernelGGL((oc_reset_kernel<a(), k(), w()>), grid, dim3(kBlock), 0, s, h->args.sw, P, (uint8_t*)state);
        return hip_check(h->wide ? "oc_reset (wide) launch" : "oc_reset launch");
    });
}

int oc_step(const oc_handle* h, const void* state_in, void* state_out, const uint8_t* actions,
            uint8_t* exec_actions, uint8_t* coll_mask, uint64_t* stats, int64_t B, void* stream) {
    if (h == nullptr || state_in == nullptr || state_out == nullptr || actions == nullptr || B < 0)
        return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    if (B == 0) return OC_OK;
    if (((uintptr_t)state_in | (uintptr_t)state_out | (uintptr_t)actions | (uintptr_t)exec_actions |
         (uintptr_t)coll_mask) & 15u)
        return fail(OC_EINVAL, "buffers must be 16-byte aligned");
    if (h->wide) return step_wide(h, state_in, state_out, actions, nullptr, exec_actions, coll_mask, stats, nullptr, B, 1, stream);
    LevelArgs L = h->args;
    L.pitch = pitch_for(B);
    L.B = B;
    if ((int64_t)ocly::num_planes(h->A, h->K, false) * L.pitch >= (1ll << 31))
        return fail(OC_EINVAL, "batch too large for one launch (state must be < 2 GiB)");
    const dim3 grid((unsigned)(L.pitch / kEPL / kStepBlock));  // pitch is a multiple of 4096
    const uint32_t rows = (uint32_t)stats_rows(h, B);
    hipStream_t s = (hipStream_t)stream;
    return dispatch_step(h, [&](auto a, auto k, auto mode) {
        hipLaunchKernelGGL((oc_step_kernel<a(), k(), mode()>), grid, dim3(kStepBlock), 0, s, L,
                           (const uint8_t*)state_in, (uint8_t*)state_out, actions, exec_actions, coll_mask, stats, rows);
        return hip_check("oc_step launch");
    });
}

int oc_cpu_step(const oc_handle* h, const void* state_in, void* state_out, const uint8_t* actions,
                uint8_t* exec_actions, uint8_t* coll_mask, uint64_t* totals, int64_t B, int32_t nthreads) {
    if (h == nullptr || state_in == nullptr || state_out == nullptr || actions == nullptr || B < 0 || nthreads < 0)
        return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    if (B == 0) return OC_OK;
    const int64_t P = pitch_for(B), words = (B + kEPL - 1) / kEPL;
    const int64_t nt = host_threads(nthreads, words, 4096);  // >= 4096 words (16 Ki envs) per thread
    std::vector<uint64_t> part((size_t)nt * OC_NSTATS, 0);
    const int rc = run_ranges(nt, [&](int64_t i) {
        const int64_t g0 = words * i / nt, g1 = words * (i + 1) / nt;
        const uint8_t* si = (const uint8_t*)state_in;
        uint8_t* so = (uint8_t*)state_out;
        uint64_t* st = part.data() + i * OC_NSTATS;
        const ocsw::SwarLevel& sw = h->args.sw;
        if (h->wide) {  // the wide SWAR step (step4w), four envs per word as the kernel
            uint8_t cls[ocro::kMaxCellsWide];
            for (int c = 0; c < ocro::kMaxCellsWide; ++c) cls[c] = ocsw::tile_class(h->wide_tiles_host[c]);
            return dispatch_ak(h->A, h->K, [&](auto a, auto k) {
                ocio::host_step_range<1, a(), k(), true>(sw, WideClass{cls}, si, so, actions, exec_actions, coll_mask, B,
                                                         P, g0, g1, st);
                return OC_OK;
            });
        }
        return dispatch_step(h, [&](auto a, auto k, auto mode) {
            ocio::host_step_range<mode(), a(), k(), false>(sw, NarrowClass{(const uint8_t*)h->args.cls4}, si, so, actions,
                                                           exec_actions, coll_mask, B, P, g0, g1, st);
            return OC_OK;
        });
    });
    if (rc == OC_OK && totals != nullptr)
        for (int64_t i = 0; i < nt; ++i)
            for (int c = 0; c < OC_NSTATS; ++c) totals[c] += part[(size_t)(i * OC_NSTATS + c)];
    return rc;
}

int oc_step_n(const oc_handle* h, const void* state_in, void* state_out, const uint8_t* actions, void* traj,
              uint8_t* exec_actions, uint8_t* coll_mask, uint64_t* stats, uint64_t* totals, int64_t B, int32_t n,
              void* stream) {
    if (h == nullptr || state_in == nullptr || state_out == nullptr || actions == nullptr || B < 0 || n < 0)
        return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    if (totals != nullptr && stats == nullptr) return fail(OC_EINVAL, "totals need the stats buffer");
    if (totals != nullptr && (uintptr_t)totals & 7u) return fail(OC_EINVAL, "totals must be 8-byte aligned");
    if (B == 0 || n == 0) return totals != nullptr && B > 0 ? oc_stats_reduce(h, stats, B, totals, stream) : OC_OK;
    if (((uintptr_t)state_in | (uintptr_t)state_out | (uintptr_t)actions | (uintptr_t)traj | (uintptr_t)exec_actions |
         (uintptr_t)coll_mask) & 15u)
        return fail(OC_EINVAL, "buffers must be 16-byte aligned");
    LevelArgs L = h->args;
    L.pitch = pitch_for(B);
    L.B = B;
    const int64_t NP = ocly::num_planes(h->A, h->K, h->wide);
    // state_out may be the trajectory's last state (written once); nothing else may overlap it
    const uint8_t* last_slot = traj ? (const uint8_t*)traj + (int64_t)(n - 1) * NP * L.pitch : nullptr;
    const bool out_is_last = traj != nullptr && (const uint8_t*)state_out == last_slot;
    if (traj != nullptr) {
        const uint8_t *t0 = (const uint8_t*)traj, *t1 = t0 + (int64_t)n * NP * L.pitch;
        auto overlaps = [&](const void* p) {
            const uint8_t* q = (const uint8_t*)p;
            return q + NP * L.pitch > t0 && q < t1;
        };
        if (overlaps(state_in) || (overlaps(state_out) && !out_is_last))
            return fail(OC_EINVAL, "traj must not overlap the state (state_out may be its last state)");
    }
    if (h->wide) return step_wide(h, state_in, state_out, actions, traj, exec_actions, coll_mask, stats, totals, B, n, stream);
    // <= 5 waves per SIMD resident: 5 blocks of 4 waves per CU, or 4 of 5 with the loader wave
    const int64_t need = L.pitch / kEnvsPerBlock;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t rows = (uint32_t)stats_rows(h, B);
    return split_steps(NP, L.pitch, h->A, state_in, state_out, actions, traj, exec_actions, coll_mask, n,
                       [&](const StepLaunch& l) {
        return dispatch_step(h, [&](auto a, auto k, auto mode) {
            constexpr bool kLW = use_loader_wave<a(), k(), mode()>();
            const int64_t cap = (int64_t)h->cus * (kLW ? 4 : 5);
            const dim3 grid((unsigned)(need < cap ? need : cap));
            hipLaunchKernelGGL((oc_step_n_kernel<a(), k(), kCPnt, 0, mode()>), grid, dim3(kBlock + (kLW ? 64 : 0)), 0, s,
                               L, l.src, l.so, l.ac, l.tr, l.ex, l.cm, stats, l.last ? totals : nullptr, rows, l.m);
            return hip_check("oc_step_n launch");
        });
    });
}

int oc_rollout(const oc_handle* h, const void* state_in, void* state_out, const uint8_t* actions,
               const uint8_t* alloc, const oc_subtask* subtasks, int32_t num_subtasks, uint8_t* out_flags,
               float* lower_bound, int64_t B, void* stream) {
    if (h == nullptr || state_in == nullptr || state_out == nullptr || actions == nullptr || subtasks == nullptr ||
        out_flags == nullptr || lower_bound == nullptr || B < 0)
        return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    if (state_in == state_out) return fail(OC_EINVAL, "oc_rollout is out of place");
    if (((uintptr_t)lower_bound & 3u) || ((uintptr_t)state_in & 1u) || ((uintptr_t)state_out & 1u))
        return fail(OC_EINVAL, "misaligned buffer");
    RollArgs R;
    if (const int rc = roll_args(h, subtasks, num_subtasks, B, R, true)) return rc;
    if (B == 0) return OC_OK;
    const dim3 grid(env_grid(h, B, kRollBlock, 8 * kBlock / kRollBlock));
    hipStream_t st = (hipStream_t)stream;
    if (!h->wide && !h->roll.dist_global && B * kRollGroup <= (int64_t)h->cus * kRollBlock) {
        // one round of blocks with a lane group per row (oc_rollout_group_kernel)
        const dim3 ggrid((unsigned)((B * kRollGroup + kRollBlock - 1) / kRollBlock));
        return dispatch_ak(h->A, h->K, [&](auto a, auto k) {
            return launch_staged(oc_rollout_group_kernel<a(), k()>, ggrid, dim3(kRollBlock), R, st, "oc_rollout launch",
                                 kPlanStaticLds, (const uint8_t*)state_in, (uint8_t*)state_out, actions, alloc,
                                 (const uint8_t*)h->roll_blob, out_flags, lower_bound);
        });
    }
    return dispatch_plan(h, [&](auto a, auto k, auto w, auto gd) {
        return launch_staged(oc_rollout_kernel<a(), k(), w(), gd()>, grid, dim3(kRollBlock), R, st, "oc_rollout launch",
                             kPlanStaticLds, (const uint8_t*)state_in, (uint8_t*)state_out, actions, alloc,
                             (const uint8_t*)h->roll_blob, out_flags, lower_bound);
    });
}

int oc_nav_likelihood(const oc_handle* h, const void* state, const uint8_t* taken, const uint8_t* alloc,
                      const oc_subtask* subtasks, int32_t num_subtasks, int32_t self_agent, double beta,
                      double none_action_prob, double* likelihood, uint8_t* out_flags, int64_t B, void* stream) {
    if (h == nullptr || state == nullptr || taken == nullptr || subtasks == nullptr || likelihood == nullptr ||
        out_flags == nullptr || B < 0)
        return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    if (self_agent < 0 || self_agent >= h->A) return fail(OC_EINVAL, "self_agent %d", self_agent);
    if (((uintptr_t)likelihood & 7u) || ((uintptr_t)state & 1u)) return fail(OC_EINVAL, "misaligned buffer");
    RollArgs R;
    if (const int rc = roll_args(h, subtasks, num_subtasks, B, R)) return rc;
    if (B == 0) return OC_OK;
    bool any_joint = false;  // lanes per row: one per candidate with a two-agent configuration
    for (int i = 0; i < num_subtasks; ++i) any_joint |= subtasks[i].num_agents == 2;
    const int64_t G = any_joint ? 32 : 8;
    // grid: up to 16 blocks per CU with 32-lane groups (5 resident per CU: measured 0.35 vs
    // 0.39 ms per 2^18 C5 rows against 8 per CU), 8 per CU with 8-lane groups (3-4 resident)
    // the compacted form's row slots take up to kLikCompactLds more LDS: a level whose tables
    // leave less than that runs the grouped form (same outputs)
    // (oc_set_likelihood_form(h, OC_LIK_FORM_GROUPED) forces the grouped form: the parity test of that path)
    const bool compact = OC_LIK_COMPACT && h->lik_form == OC_LIK_FORM_AUTO &&
                         h->roll.lds_bytes + kLikCompactLds + (int)sizeof(ocro::Sub) * OC_MAX_SUBTASKS <= kLdsPerCu;
    const int64_t rows_per_block = compact ? (kBlock / 64) * lik_rows_per_round((int)G) : kBlock / G;
    const dim3 grid(env_grid(h, B, rows_per_block, any_joint ? 16 : 8));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_plan(h, [&](auto a, auto k, auto w, auto gd) {
        auto go = [&](auto kernel) {
            return launch_staged(kernel, grid, dim3(kBlock), R, st, "oc_nav_likelihood launch", kPlanStaticLds,
                                 (const uint8_t*)state, taken, alloc, (const uint8_t*)h->roll_blob, (int)self_agent, beta,
                                 none_action_prob, likelihood, out_flags);
        };
        if (compact && any_joint) return go(oc_likelihood_compact_kernel<a(), k(), 32, w(), gd()>);
        if (compact) return go(oc_likelihood_compact_kernel<a(), k(), 8, w(), gd()>);
        if (any_joint) return go(oc_likelihood_kernel<a(), k(), 32, w(), gd()>);
        return go(oc_likelihood_kernel<a(), k(), 8, w(), gd()>);
    });
}

// oc_nav_policy / oc_cpu_nav_policy: the arguments both check, and the call's RollArgs / PolicyArgs
static int policy_args(const oc_handle* h, const void* state, const oc_subtask* subtasks, int32_t num_subtasks,
                       double beta, double nap, int32_t mode, int64_t env_offset, int64_t step, uint64_t seed,
                       const uint8_t* actions, const double* probs, int32_t num_cand, const uint8_t* out_flags,
                       int64_t B, bool host, RollArgs& R, PolicyArgs& Q, bool& any_joint) {
    if (state == nullptr || subtasks == nullptr || actions == nullptr || out_flags == nullptr || B < 0 ||
        env_offset < 0 || step < 0)
        return fail(OC_EINVAL, "bad argument");
    if (mode < 0 || mode > (OC_POLICY_GREEDY | OC_POLICY_COUNT_STATE)) return fail(OC_EINVAL, "policy: mode %d", mode);
    if (num_cand != 5 && num_cand != 25) return fail(OC_EINVAL, "policy: num_cand %d (5 or 25)", num_cand);
    if (((uintptr_t)probs & 7u) || ((uintptr_t)state & 1u)) return fail(OC_EINVAL, "misaligned buffer");
    if (const int rc = roll_args(h, subtasks, num_subtasks, B, R, false, host)) return rc;
    any_joint = false;
    for (int i = 0; i < num_subtasks; ++i) any_joint |= subtasks[i].num_agents == 2;
    if (any_joint && num_cand != 25)
        return fail(OC_EINVAL, "policy: num_cand 5 with a two-agent configuration in the table");
    Q.beta = beta;
    Q.nap = nap;
    Q.env_offset = env_offset;
    Q.step = step;
    Q.seed = seed;
    Q.mode = mode;
    Q.num_cand = num_cand;
    return OC_OK;
}

int oc_nav_policy(const oc_handle* h, const void* state, const uint8_t* alloc, const oc_subtask* subtasks,
                  int32_t num_subtasks, double beta, double none_action_prob, int32_t mode, int64_t env_offset,
                  int64_t step, uint64_t seed, uint8_t* actions, double* probs, int32_t num_cand,
                  uint8_t* out_flags, int64_t B, void* stream) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    RollArgs R;
    PolicyArgs Q;
    bool any_joint;
    if (const int rc = policy_args(h, state, subtasks, num_subtasks, beta, none_action_prob, mode, env_offset, step, seed,
                                   actions, probs, num_cand, out_flags, B, false, R, Q, any_joint))
        return rc;
    if (B == 0) return OC_OK;
    // the grouped likelihood's grid: a lane group per row, up to 16 blocks per CU with 32-lane
    // groups, 8 with 8-lane groups
    const int64_t rows_per_block = kBlock / (any_joint ? 32 : 8);
    const dim3 grid(env_grid(h, B, rows_per_block, any_joint ? 16 : 8));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_plan(h, [&](auto a, auto k, auto w, auto gd) {
        auto go = [&](auto kernel) {
            return launch_staged(kernel, grid, dim3(kBlock), R, st, "oc_nav_policy launch", kPlanStaticLds, Q,
                                 (const uint8_t*)state, alloc, (const uint8_t*)h->roll_blob, actions, probs, out_flags);
        };
        if (any_joint) return go(oc_policy_kernel<a(), k(), 32, w(), gd()>);
        return go(oc_policy_kernel<a(), k(), 8, w(), gd()>);
    });
}

int oc_cpu_nav_policy(const oc_handle* h, const void* state, const uint8_t* alloc, const oc_subtask* subtasks,
                      int32_t num_subtasks, double beta, double none_action_prob, int32_t mode, int64_t env_offset,
                      int64_t step, uint64_t seed, uint8_t* actions, double* probs, int32_t num_cand,
                      uint8_t* out_flags, int64_t B, int32_t nthreads) {
    if (h == nullptr || nthreads < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    RollArgs R;
    PolicyArgs Q;
    bool any_joint;
    if (const int rc = policy_args(h, state, subtasks, num_subtasks, beta, none_action_prob, mode, env_offset, step, seed,
                                   actions, probs, num_cand, out_flags, B, true, R, Q, any_joint))
        return rc;
    if (B == 0) return OC_OK;
    const uint8_t* blob = h->roll_blob_host.data();
    // >= 1,024 rows (up to 25 rollouts each) per thread
    return host_ranges(h, nthreads, B, 1024, [&](auto a, auto k, auto w, int64_t e0, int64_t e1) {
        host_policy_range<a(), k(), w()>(R, Q, blob, (const uint8_t*)state, alloc, actions, probs, out_flags, e0, e1);
        return OC_OK;
    });
}

// configuration chunks: enough blocks for this many per CU (round 2's sweep, 0.44 ms kernels:
// 64 best; round 5, 0.09 ms kernels with each block staging the tables: 32 at 0.0916-0.0924 ms
// against 0.0925-0.0938 at 64 and 0.0925-0.0931 at 24, profiles/r05/ab/ab_bounds_chunks.jsonl)
#ifndef OC_BOUNDS_BLOCKS_PER_CU
#define OC_BOUNDS_BLOCKS_PER_CU 32
#endif
int oc_subtask_bounds(const oc_handle* h, const void* state, const oc_subtask* subtasks, int32_t num_subtasks,
                      float* lower_bound, uint8_t* doable, int64_t B, void* stream) {
    if (h == nullptr || state == nullptr || subtasks == nullptr || lower_bound == nullptr || doable == nullptr ||
        B < 0)
        return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    if (((uintptr_t)lower_bound & 3u) || ((uintptr_t)state & 1u)) return fail(OC_EINVAL, "misaligned buffer");
    RollArgs R;
    if (const int rc = roll_args(h, subtasks, num_subtasks, B, R)) return rc;
    if (B == 0) return OC_OK;
    const int64_t bx = env_grid(h, B, kBlock, 8);
    // configuration chunks: enough blocks for OC_BOUNDS_BLOCKS_PER_CU per CU, at most one
    // configuration per chunk (round 2, C5, 2^18 envs x 64 configurations: 0.75 ms unchunked,
    // 0.53 / 0.46 / 0.44 / 0.44 ms at 16 / 32 / 64 / 128 blocks per CU, 0.47 ms at one
    // configuration per block; profiles/r02/bounds_chunk_sweep.log; round 5: see the macro)
    int64_t chunks = ((int64_t)h->cus * OC_BOUNDS_BLOCKS_PER_CU + bx - 1) / bx;
    if (chunks > R.nsub) chunks = R.nsub;
    if (chunks < 1) chunks = 1;
    const dim3 grid((unsigned)bx, (unsigned)chunks);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_plan(h, [&](auto a, auto k, auto w, auto gd) {
        return launch_staged(oc_bounds_kernel<a(), k(), w(), gd()>, grid, dim3(kBlock), R, st, "oc_subtask_bounds launch",
                             kPlanStaticLds, (const uint8_t*)state, (const uint8_t*)h->roll_blob, lower_bound, doable);
    });
}

// oc_task_select / oc_cpu_task_select: the arguments both check, and the call's RollArgs (agent
// m's S one-agent Level-0 configurations at rows m * S ..) and TaskArgs
static int task_args(const oc_handle* h, const void* state, const oc_subtask* subtasks, int32_t num_subtasks,
                     const uint8_t* agents, int32_t num_scripted, int32_t flags, const uint8_t* tstate,
                     const float* bound, int64_t B, bool host, RollArgs& R, TaskArgs& Q) {
    if (state == nullptr || subtasks == nullptr || agents == nullptr || tstate == nullptr)
        return fail(OC_EINVAL, "task_select: state, subtasks, agents and tstate are required");
    if (B < 0) return fail(OC_EINVAL, "task_select: B %lld", (long long)B);
    const int32_t S = num_subtasks, M = num_scripted;
    if (M < 1 || M > h->A) return fail(OC_EINVAL, "task_select: num_scripted %d (1..%d)", M, h->A);
    if (S < 1 || S > 63) return fail(OC_EINVAL, "task_select: num_subtasks %d (1..63)", S);
    if (M * S > OC_MAX_SUBTASKS)
        return fail(OC_EINVAL, "task_select: num_scripted x num_subtasks = %d (at most %d)", M * S, OC_MAX_SUBTASKS);
    if (flags < 0 || flags > (OC_TASK_INIT | OC_TASK_COMMIT | OC_TASK_DISTINCT))
        return fail(OC_EINVAL, "task_select: flags %d", flags);
    if (const int rc = check_agents("task_select", agents, M, h->A)) return rc;
    if (((uintptr_t)bound & 3u) || ((uintptr_t)state & 1u)) return fail(OC_EINVAL, "task_select: misaligned buffer");
    oc_subtask rows[OC_MAX_SUBTASKS];
    for (int m = 0; m < M; ++m)
        for (int i = 0; i < S; ++i) rows[m * S + i] = level0_row(subtasks[i], agents[m]);
    if (const int rc = roll_args(h, rows, M * S, B, R, false, host)) return rc;
    Q.S = S;
    Q.M = M;
    Q.flags = flags;
    return OC_OK;
}

int oc_task_select(const oc_handle* h, const void* state, const void* state_prev, const oc_subtask* subtasks,
                   int32_t num_subtasks, const uint8_t* agents, int32_t num_scripted, int32_t flags, uint8_t* tstate,
                   float* bound, uint8_t* info, int64_t B, void* stream) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    RollArgs R;
    TaskArgs Q;
    if (const int rc = task_args(h, state, subtasks, num_subtasks, agents, num_scripted, flags, tstate, bound, B, false, R, Q))
        return rc;
    if (B == 0) return OC_OK;
    const dim3 grid(env_grid(h, B, kBlock, 8));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_plan(h, [&](auto a, auto k, auto w, auto gd) {
        return launch_staged(oc_task_kernel<a(), k(), w(), gd()>, grid, dim3(kBlock), R, st, "oc_task_select launch",
                             kPlanStaticLds, Q, (const uint8_t*)state, (const uint8_t*)state_prev,
                             (const uint8_t*)h->roll_blob, tstate, bound, info);
    });
}

int oc_cpu_task_select(const oc_handle* h, const void* state, const void* state_prev, const oc_subtask* subtasks,
                       int32_t num_subtasks, const uint8_t* agents, int32_t num_scripted, int32_t flags,
                       uint8_t* tstate, float* bound, uint8_t* info, int64_t B, int32_t nthreads) {
    if (h == nullptr || nthreads < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    RollArgs R;
    TaskArgs Q;
    if (const int rc = task_args(h, state, subtasks, num_subtasks, agents, num_scripted, flags, tstate, bound, B, true, R, Q))
        return rc;
    if (B == 0) return OC_OK;
    const uint8_t* blob = h->roll_blob_host.data();
    const uint8_t *sin = (const uint8_t*)state, *sprev = (const uint8_t*)state_prev;
    // >= 1,024 rows (up to M x S bound walks each) per thread
    return host_ranges(h, nthreads, B, 1024, [&](auto a, auto k, auto w, int64_t e0, int64_t e1) {
        const int64_t P = R.pitch;
        for (int64_t e = e0; e < e1; ++e) {
            const bool init = starts_over<a(), k(), w()>((Q.flags & OC_TASK_INIT) != 0, sprev, P, e);
            ocro::RowOps<a(), k(), w(), false, true> ops(R.L, blob);
            ops.task_env(load_row<a(), k(), w()>(sin, P, e), R.subs, Q.S, Q.M, Q.flags, init, tstate + e,
                         bound != nullptr ? bound + e : nullptr, info != nullptr ? info + e : nullptr, P);
        }
        return OC_OK;
    });
}

// oc_team_select / oc_cpu_team_select: the arguments both check, and the call's RollArgs (a0's S
// one-agent Level-0 configurations at rows 0 .., a1's at S .., the two-agent ones at 2S ..) and
// TeamArgs
static int team_args(const oc_handle* h, const void* state, const oc_subtask* subtasks, int32_t num_subtasks,
                     const uint8_t* agents, int32_t flags, const uint8_t* tstate, const float* bound, int64_t B,
                     bool host, RollArgs& R, TeamArgs& Q) {
    if (state == nullptr || subtasks == nullptr || agents == nullptr || tstate == nullptr)
        return fail(OC_EINVAL, "team_select: state, subtasks, agents and tstate are required");
    if (B < 0) return fail(OC_EINVAL, "team_select: B %lld", (long long)B);
    const int32_t S = num_subtasks;
    if (h->A < 2) return fail(OC_EINVAL, "team_select: a team needs 2 agents, the handle has %d", h->A);
    if (S < 1 || S > OC_TEAM_MAX_SUBTASKS)
        return fail(OC_EINVAL, "team_select: num_subtasks %d (1..%d)", S, OC_TEAM_MAX_SUBTASKS);
    if (flags < 0 || flags > (OC_TEAM_INIT | OC_TEAM_COMMIT | OC_TEAM_SPLIT_FIRST))
        return fail(OC_EINVAL, "team_select: flags %d", flags);
    if (agents[0] >= h->A || agents[1] >= h->A)
        return fail(OC_EINVAL, "team_select: agent %d", agents[0] >= h->A ? agents[0] : agents[1]);
    if (agents[0] >= agents[1]) return fail(OC_EINVAL, "team_select: agents %d, %d not ascending", agents[0], agents[1]);
    if (((uintptr_t)bound & 3u) || ((uintptr_t)state & 1u)) return fail(OC_EINVAL, "team_select: misaligned buffer");
    static_assert(3 * OC_TEAM_MAX_SUBTASKS <= OC_MAX_SUBTASKS, "the three configurations per subtask share the staging");
    oc_subtask rows[OC_MAX_SUBTASKS];
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < S; ++i) {
            const bool two = c == 2 && subtasks[i].kind != OC_SUB_NONE;  // a None row is a one-agent row and never a candidate
            rows[c * S + i] = two ? level0_row(subtasks[i], agents[0], agents[1]) : level0_row(subtasks[i], agents[c == 1 ? 1 : 0]);
        }
    if (const int rc = roll_args(h, rows, 3 * S, B, R, false, host)) return rc;
    Q.S = S;
    Q.flags = flags;
    return OC_OK;
}

int oc_team_select(const oc_handle* h, const void* state, const void* state_prev, const oc_subtask* subtasks,
                   int32_t num_subtasks, const uint8_t* agents, int32_t flags, uint8_t* tstate, float* bound,
                   uint8_t* info, int64_t B, void* stream) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    RollArgs R;
    TeamArgs Q;
    if (const int rc = team_args(h, state, subtasks, num_subtasks, agents, flags, tstate, bound, B, false, R, Q)) return rc;
    if (B == 0) return OC_OK;
    const dim3 grid(env_grid(h, B, kBlock, 8));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_plan(h, [&](auto a, auto k, auto w, auto gd) {
        if constexpr (decltype(a)::value < 2) {
            return fail(OC_EINVAL, "team_select: a team needs 2 agents");
        } else {
            return launch_staged(oc_team_kernel<a(), k(), w(), gd()>, grid, dim3(kBlock), R, st, "oc_team_select launch",
                                 kPlanStaticLds, Q, (const uint8_t*)state, (const uint8_t*)state_prev,
                                 (const uint8_t*)h->roll_blob, tstate, bound, info);
        }
    });
}

int oc_cpu_team_select(const oc_handle* h, const void* state, const void* state_prev, const oc_subtask* subtasks,
                       int32_t num_subtasks, const uint8_t* agents, int32_t flags, uint8_t* tstate, float* bound,
                       uint8_t* info, int64_t B, int32_t nthreads) {
    if (h == nullptr || nthreads < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    RollArgs R;
    TeamArgs Q;
    if (const int rc = team_args(h, state, subtasks, num_subtasks, agents, flags, tstate, bound, B, true, R, Q)) return rc;
    if (B == 0) return OC_OK;
    const uint8_t* blob = h->roll_blob_host.data();
    const uint8_t *sin = (const uint8_t*)state, *sprev = (const uint8_t*)state_prev;
    // >= 1,024 rows (up to 3 x S bound walks each) per thread
    return host_ranges(h, nthreads, B, 1024, [&](auto a, auto k, auto w, int64_t e0, int64_t e1) {
        if constexpr (decltype(a)::value < 2) {
            return fail(OC_EINVAL, "team_select: a team needs 2 agents");
        } else {
            const int64_t P = R.pitch;
            for (int64_t e = e0; e < e1; ++e) {
                const bool init = starts_over<a(), k(), w()>((Q.flags & OC_TEAM_INIT) != 0, sprev, P, e);
                ocro::RowOps<a(), k(), w(), false, true> ops(R.L, blob);
                ops.team_env(load_row<a(), k(), w()>(sin, P, e), R.subs, Q.S, Q.flags, init, tstate + e,
                             bound != nullptr ? bound + e : nullptr, info != nullptr ? info + e : nullptr, P);
            }
            return OC_OK;
        }
    });
}

// oc_belief_update / oc_cpu_belief_update: the arguments both check, and the call's RollArgs (the S
// rows of the table as one-agent Level-0 configurations; the kernels set the watched agent) and
// BeliefArgs
static int belief_args(const oc_handle* h, const void* state_prev, const uint8_t* taken, const oc_subtask* subtasks,
                       int32_t num_subtasks, const uint8_t* agents, int32_t num_watched, double beta, double nap,
                       int32_t flags, const double* belief, const uint8_t* bstate, int64_t B, bool host, RollArgs& R,
                       BeliefArgs& Q) {
    if (subtasks == nullptr || agents == nullptr || belief == nullptr || bstate == nullptr)
        return fail(OC_EINVAL, "belief_update: subtasks, agents, belief and bstate are required");
    if (B < 0) return fail(OC_EINVAL, "belief_update: B %lld", (long long)B);
    const int32_t S = num_subtasks, M = num_watched;
    if (M < 1 || M > h->A) return fail(OC_EINVAL, "belief_update: num_watched %d (1..%d)", M, h->A);
    if (S < 1 || S > 63) return fail(OC_EINVAL, "belief_update: num_subtasks %d (1..63)", S);
    if (flags < 0 || flags > OC_BELIEF_INIT) return fail(OC_EINVAL, "belief_update: flags %d", flags);
    if (!(flags & OC_BELIEF_INIT) && (state_prev == nullptr || taken == nullptr))
        return fail(OC_EINVAL, "belief_update: state_prev and taken are required without OC_BELIEF_INIT");
    if (!(beta == beta) || !(nap >= 0.0 && nap <= 1.0))
        return fail(OC_EINVAL, "belief_update: beta %g, none_action_prob %g", beta, nap);
    if (const int rc = check_agents("belief_update", agents, M, h->A)) return rc;
    if (((uintptr_t)belief & 7u) || ((uintptr_t)state_prev & 1u)) return fail(OC_EINVAL, "belief_update: misaligned buffer");
    oc_subtask rows[OC_MAX_SUBTASKS];
    for (int i = 0; i < S; ++i) rows[i] = level0_row(subtasks[i], 0);
    if (const int rc = roll_args(h, rows, S, B, R, false, host)) return rc;
    Q.beta = beta;
    Q.nap = nap;
    Q.S = S;
    Q.M = M;
    Q.flags = flags;
    for (int m = 0; m < 4; ++m) Q.agents[m] = m < M ? agents[m] : 0;
    return OC_OK;
}

int oc_belief_update(const oc_handle* h, const void* state_prev, const uint8_t* taken, const uint8_t* events,
                     const oc_subtask* subtasks, int32_t num_subtasks, const uint8_t* agents, int32_t num_watched,
                     double beta, double none_action_prob, int32_t flags, double* belief, uint8_t* bstate, uint8_t* map,
                     uint8_t* info, int64_t B, void* stream) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    RollArgs R;
    BeliefArgs Q;
    if (const int rc = belief_args(h, state_prev, taken, subtasks, num_subtasks, agents, num_watched, beta,
                                   none_action_prob, flags, belief, bstate, B, false, R, Q))
        return rc;
    if (B == 0) return OC_OK;
    // oc_nav_policy's grid for 8-lane groups, once per watched agent
    const dim3 grid(env_grid(h, B, kBlock / 8, 8), (unsigned)Q.M);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_plan(h, [&](auto a, auto k, auto w, auto gd) {
        return launch_staged(oc_belief_kernel<a(), k(), w(), gd()>, grid, dim3(kBlock), R, st, "oc_belief_update launch",
                             kBeliefStaticLds, Q, (const uint8_t*)state_prev, taken, events, (const uint8_t*)h->roll_blob,
                             belief, bstate, map, info);
    });
}

int oc_cpu_belief_update(const oc_handle* h, const void* state_prev, const uint8_t* taken, const uint8_t* events,
                         const oc_subtask* subtasks, int32_t num_subtasks, const uint8_t* agents, int32_t num_watched,
                         double beta, double none_action_prob, int32_t flags, double* belief, uint8_t* bstate,
                         uint8_t* map, uint8_t* info, int64_t B, int32_t nthreads) {
    if (h == nullptr || nthreads < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    RollArgs R;
    BeliefArgs Q;
    if (const int rc = belief_args(h, state_prev, taken, subtasks, num_subtasks, agents, num_watched, beta,
                                   none_action_prob, flags, belief, bstate, B, true, R, Q))
        return rc;
    if (B == 0) return OC_OK;
    const uint8_t* blob = h->roll_blob_host.data();
    const uint8_t* sprev = (const uint8_t*)state_prev;
    // >= 1,024 rows (M x S hypotheses each) per thread
    return host_ranges(h, nthreads, B, 1024, [&](auto a, auto k, auto w, int64_t e0, int64_t e1) {
        using Row = ocro::RowT<k(), w()>;
        const int64_t P = R.pitch;
        const int S = Q.S, HP = (S + 8) >> 3, EP = (S + 7) >> 3;
        for (int64_t e = e0; e < e1; ++e) {
            const bool init = starts_over<a(), k(), w()>((Q.flags & OC_BELIEF_INIT) != 0, sprev, P, e);
            uint64_t ev = 0ull;
            if (!init && events != nullptr)
                for (int c = 0; c < EP; ++c) ev |= (uint64_t)events[c * P + e] << (8 * c);
            const Row r0 = init ? Row{} : load_row<a(), k(), w()>(sprev, P, e);
            for (int m = 0; m < Q.M; ++m) {
                const int ag = Q.agents[m];
                ocro::RowOps<a(), k(), w(), true, true> ops(R.L, blob);
                ops.belief_env(r0, R.subs, S, ag, init ? ocro::kNoop : (int)taken[ag * P + e], ev, init, Q.beta, Q.nap,
                               belief + (int64_t)m * (S + 1) * P + e, bstate + (int64_t)m * 2 * HP * P + e,
                               map != nullptr ? map + m * P + e : nullptr, info != nullptr ? info + m * P + e : nullptr,
                               P);
            }
        }
        return OC_OK;
    });
}

// oc_team_belief_update / oc_cpu_team_belief_update: the arguments both check, and the call's
// RollArgs (oc_team_select's staging: a0's S one-agent Level-0 configurations at rows 0 .., a1's at
// S .., the two-agent ones at 2S ..) and TBeliefArgs
static int team_belief_args(const oc_handle* h, const void* state_prev, const uint8_t* taken, const oc_subtask* subtasks,
                            int32_t num_subtasks, const uint8_t* agents, int32_t self_agent, double beta, double nap,
                            int32_t flags, const double* belief, const uint8_t* tbstate, const double* lik, int64_t B,
                            bool host, RollArgs& R, TBeliefArgs& Q) {
    if (subtasks == nullptr || agents == nullptr || belief == nullptr || tbstate == nullptr)
        return fail(OC_EINVAL, "team_belief_update: subtasks, agents, belief and tbstate are required");
    if (B < 0) return fail(OC_EINVAL, "team_belief_update: B %lld", (long long)B);
    const int32_t S = num_subtasks;
    if (h->A < 2) return fail(OC_EINVAL, "team_belief_update: a team needs 2 agents, the handle has %d", h->A);
    if (S < 1 || S > OC_TEAM_MAX_SUBTASKS)
        return fail(OC_EINVAL, "team_belief_update: num_subtasks %d (1..%d)", S, OC_TEAM_MAX_SUBTASKS);
    if (flags < 0 || flags > OC_TBELIEF_INIT) return fail(OC_EINVAL, "team_belief_update: flags %d", flags);
    if (!(flags & OC_TBELIEF_INIT) && (state_prev == nullptr || taken == nullptr))
        return fail(OC_EINVAL, "team_belief_update: state_prev and taken are required without OC_TBELIEF_INIT");
    if (!(beta == beta) || !(nap >= 0.0 && nap <= 1.0))
        return fail(OC_EINVAL, "team_belief_update: beta %g, none_action_prob %g", beta, nap);
    if (agents[0] >= h->A || agents[1] >= h->A)
        return fail(OC_EINVAL, "team_belief_update: agent %d", agents[0] >= h->A ? agents[0] : agents[1]);
    if (agents[0] >= agents[1])
        return fail(OC_EINVAL, "team_belief_update: agents %d, %d not ascending", agents[0], agents[1]);
    if (self_agent != agents[0] && self_agent != agents[1])
        return fail(OC_EINVAL, "team_belief_update: self_agent %d is not in the pair (%d, %d)", self_agent, agents[0],
                    agents[1]);
    if (((uintptr_t)belief & 7u) || ((uintptr_t)lik & 7u) || ((uintptr_t)state_prev & 1u))
        return fail(OC_EINVAL, "team_belief_update: misaligned buffer");
    oc_subtask rows[OC_MAX_SUBTASKS];
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < S; ++i) {
            const bool two = c == 2 && subtasks[i].kind != OC_SUB_NONE;  // a None row is a one-agent row and never a hypothesis
            rows[c * S + i] = two ? level0_row(subtasks[i], agents[0], agents[1]) : level0_row(subtasks[i], agents[c == 1 ? 1 : 0]);
        }
    if (const int rc = roll_args(h, rows, 3 * S, B, R, false, host)) return rc;
    Q.beta = beta;
    Q.nap = nap;
    Q.S = S;
    Q.flags = flags;
    Q.a0 = agents[0];
    Q.a1 = agents[1];
    Q.self = (uint8_t)self_agent;
    Q.pad = 0;
    return OC_OK;
}

int oc_team_belief_update(const oc_handle* h, const void* state_prev, const uint8_t* taken, const uint8_t* events,
                          const oc_subtask* subtasks, int32_t num_subtasks, const uint8_t* agents, int32_t self_agent,
                          double beta, double none_action_prob, int32_t flags, double* belief, uint8_t* tbstate,
                          double* lik, uint8_t* map, uint8_t* info, int64_t B, void* stream) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    RollArgs R;
    TBeliefArgs Q;
    if (const int rc = team_belief_args(h, state_prev, taken, subtasks, num_subtasks, agents, self_agent, beta,
                                        none_action_prob, flags, belief, tbstate, lik, B, false, R, Q))
        return rc;
    if (B == 0) return OC_OK;
    const dim3 grid(env_grid(h, B, kBlock / 8, 8));  // oc_belief_update's grid for 8-lane groups
    hipStream_t st = (hipStream_t)stream;
    return dispatch_plan(h, [&](auto a, auto k, auto w, auto gd) {
        if constexpr (decltype(a)::value < 2) {
            return fail(OC_EINVAL, "team_belief_update: a team needs 2 agents");
        } else {
            return launch_staged(oc_team_belief_kernel<a(), k(), w(), gd()>, grid, dim3(kBlock), R, st,
                                 "oc_team_belief_update launch", kTBeliefStaticLds, Q, (const uint8_t*)state_prev, taken,
                                 events, (const uint8_t*)h->roll_blob, belief, tbstate, lik, map, info);
        }
    });
}

int oc_cpu_team_belief_update(const oc_handle* h, const void* state_prev, const uint8_t* taken, const uint8_t* events,
                              const oc_subtask* subtasks, int32_t num_subtasks, const uint8_t* agents,
                              int32_t self_agent, double beta, double none_action_prob, int32_t flags, double* belief,
                              uint8_t* tbstate, double* lik, uint8_t* map, uint8_t* info, int64_t B, int32_t nthreads) {
    if (h == nullptr || nthreads < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    RollArgs R;
    TBeliefArgs Q;
    if (const int rc = team_belief_args(h, state_prev, taken, subtasks, num_subtasks, agents, self_agent, beta,
                                        none_action_prob, flags, belief, tbstate, lik, B, true, R, Q))
        return rc;
    if (B == 0) return OC_OK;
    const uint8_t* blob = h->roll_blob_host.data();
    const uint8_t* sprev = (const uint8_t*)state_prev;
    // >= 1,024 rows (3 x S members each) per thread
    return host_ranges(h, nthreads, B, 1024, [&](auto a, auto k, auto w, int64_t e0, int64_t e1) {
        if constexpr (decltype(a)::value < 2) {
            return fail(OC_EINVAL, "team_belief_update: a team needs 2 agents");
        } else {
            using Row = ocro::RowT<k(), w()>;
            const int64_t P = R.pitch;
            const int S = Q.S, EP = (S + 7) >> 3;
            for (int64_t e = e0; e < e1; ++e) {
                const bool init = starts_over<a(), k(), w()>((Q.flags & OC_TBELIEF_INIT) != 0, sprev, P, e);
                uint32_t ev = 0u;
                if (!init && events != nullptr)
                    for (int c = 0; c < EP; ++c) ev |= (uint32_t)events[c * P + e] << (8 * c);
                const Row r0 = init ? Row{} : load_row<a(), k(), w()>(sprev, P, e);
                ocro::RowOps<a(), k(), w(), true, true> ops(R.L, blob);
                ops.team_belief_env(r0, R.subs, S, Q.a0, Q.a1, Q.self, init ? ocro::kNoop : (int)taken[Q.a0 * P + e],
                                    init ? ocro::kNoop : (int)taken[Q.a1 * P + e], ev, init, Q.beta, Q.nap, belief + e,
                                    tbstate + e, lik != nullptr ? lik + e : nullptr, map != nullptr ? map + e : nullptr,
                                    info != nullptr ? info + e : nullptr, P);
            }
            return OC_OK;
        }
    });
}

int oc_render(const oc_handle* h, const void* state, const uint32_t* atlas, const uint32_t* background,
              const oc_render_desc* desc, uint8_t* out, int64_t B, void* stream) {
    return oc_render_ordered(h, state, nullptr, atlas, background, desc, out, B, stream);
}

int oc_render_ordered(const oc_handle* h, const void* state, const uint8_t* draw_rank, const uint32_t* atlas,
                      const uint32_t* background, const oc_render_desc* desc, uint8_t* out, int64_t B,
                      void* stream) {
    if (h == nullptr || state == nullptr || atlas == nullptr || background == nullptr || desc == nullptr ||
        out == nullptr || B < 0)
        return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    const int W = h->level.width, H = h->level.height;
    if (W > kRenderMaxW) return fail(OC_ELEVEL, "render: width %d > %d", W, kRenderMaxW);  // oc_create caps it at 255
    if (desc->tile < kRenderPx || desc->tile % kRenderPx != 0 || desc->tile > 1024)
        return fail(OC_EINVAL, "render: tile %d (a multiple of %d)", desc->tile, kRenderPx);
    for (int c = 0; c < OC_RENDER_SIZES; ++c)
        if (desc->size[c] < 0 || desc->offset[c] < 0 || desc->size[c] + desc->offset[c] > desc->tile)
            return fail(OC_EINVAL, "render: size class %d (%d at %d) leaves the %d-px cell", c, desc->size[c],
                        desc->offset[c], desc->tile);
    for (int q = 0; q < 3; ++q)
        if (((desc->chan_map >> (8 * q)) & 0xFFu) > 3u) return fail(OC_EINVAL, "render: chan_map 0x%x", desc->chan_map);
    if (((uintptr_t)atlas | (uintptr_t)background | (uintptr_t)out) & 15u) return fail(OC_EINVAL, "misaligned buffer");
    if (B == 0) return OC_OK;
    if (B * H * 2 > 0x7FFFFFFFll) return fail(OC_EINVAL, "render: batch too large");
    RenderArgs R;
    R.W = W;
    R.H = H;
    R.tile = desc->tile;
    for (int c = 0; c < OC_RENDER_SIZES; ++c) {
        R.size[c] = desc->size[c];
        R.offset[c] = desc->offset[c];
        R.food_base[c] = desc->food_base[c];
    }
    R.plate_off[0] = desc->plate_off[0];
    R.plate_off[1] = desc->plate_off[1];
    for (int a = 0; a < OC_MAX_AGENTS; ++a) R.agent_off[a] = desc->agent_off[a];
    R.chan_map = desc->chan_map;
    R.counts = h->level.encoding == OC_ENC_COUNTS;
    R.pitch = pitch_for(B);
    for (int m = 0; m < 128; ++m) R.food_sprite[m] = desc->food_sprite[m];
    R.parts = 2;  // two blocks per (env, cell row): 0.198 vs 0.214 ms per 1,024 images (3 or 4: 0.211-0.213)
    const dim3 grid((unsigned)(B * H * R.parts));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_w(h, [&](auto a, auto k, auto w) {
        hipLaunchKernelGGL((oc_render_kernel<a(), k(), w()>), grid, dim3(kBlock), 0, st, R, (const uint8_t*)state,
                           draw_rank, atlas, background, out);
        return hip_check("oc_render launch");
    });
}

int oc_observe(const oc_handle* h, const void* state, void* obs, uint8_t* action_mask, int32_t dtype,
               int32_t view_agent, int64_t B, void* stream) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    ocob::ObsArgs R;
    if (const int rc = observe_args(h, state, obs, action_mask, dtype, view_agent, B, R)) return rc;
    if (h->obs_tab == nullptr) return fail(OC_EHIP, "observe: the level table is not on the device");
    if (B == 0) return OC_OK;
    // envs per tile: the largest power of two whose tile and staging fit the LDS budget (a 7x7
    // kitchen: 64; the largest wide levels: 1, every tile then with a head and a tail)
    const int planes = ocly::layout(h->A, h->K, h->wide).T;  // the planes before t
    int E = h->obs_tile, lg = 31 - __builtin_clz((unsigned)h->obs_tile), lds = 0;
    for (;; E >>= 1, --lg) {
        R.lds_state = (E * R.CHW + 16 + 15) & ~15;
        R.lds_tiles = R.lds_state + ((planes * E + 3) & ~3);
        R.lds_statics = R.lds_tiles + ((R.HW + 3) & ~3);
        R.lds_mask = R.lds_statics + ((2 * R.nstatic + 3) & ~3);
        lds = R.lds_mask + ((h->A * E + 3) & ~3);
        if (lds <= ocob::kLdsBudget || E == 1) break;
    }
    if (lds > ocob::kLdsBudget) return fail(OC_ELEVEL, "observe: one env's planes (%d B) exceed the LDS budget", lds);
    R.tile_envs = E;
    R.log2_envs = lg;
    // a persistent grid: the blocks the CUs' LDS holds at once (at most 8 of 4 waves per CU)
    const int64_t tiles = (B + E - 1) / E;
    int per_cu = kLdsPerCu / (lds + 512);
    per_cu = per_cu > 8 ? 8 : per_cu;
    const int64_t resident = (int64_t)h->cus * per_cu;
    const dim3 grid((unsigned)(tiles < resident ? tiles : resident));
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* tab = h->obs_tab;
    const uint16_t* statics = (const uint16_t*)(h->obs_tab + h->obs_static_off);
    return dispatch_w(h, [&](auto a, auto k, auto w) {
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(ocob::kBlock), lds, st, R, (const uint8_t*)state, tab, statics,
                               (uint8_t*)obs, action_mask);
            return hip_check("oc_observe launch");
        };
        return dtype == OC_OBS_F16 ? go(ocob::oc_observe_kernel<a(), k(), w(), true>)
                                   : go(ocob::oc_observe_kernel<a(), k(), w(), false>);
    });
}

int oc_cpu_observe(const oc_handle* h, const void* state, void* obs, uint8_t* action_mask, int32_t dtype,
                   int32_t view_agent, int64_t B, int32_t nthreads) {
    if (h == nullptr || nthreads < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    ocob::ObsArgs R;
    if (const int rc = observe_args(h, state, obs, action_mask, dtype, view_agent, B, R)) return rc;
    if (B == 0) return OC_OK;
    const uint8_t* tab = h->obs_tab_host.data();
    const uint16_t* statics = (const uint16_t*)(tab + h->obs_static_off);
    // >= 16 Ki envs per thread
    return host_ranges(h, nthreads, B, 16384, [&](auto a, auto k, auto w, int64_t e0, int64_t e1) {
        ocob::cpu_observe_range<a(), k(), w()>(R, tab, statics, (const uint8_t*)state, obs, action_mask,
                                               dtype == OC_OBS_F16, e0, e1);
        return OC_OK;
    });
}

int oc_progress(const oc_handle* h, const void* state_prev, const void* states, int32_t n, const oc_subtask* subtasks,
                int32_t num_subtasks, const float* weights, uint8_t* counts, uint8_t* events, float* reward, int64_t B,
                void* stream) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    ocpg::ProgArgs R;
    if (const int rc = progress_args(h, state_prev, states, n, subtasks, num_subtasks, weights, counts, events, reward, B, R))
        return rc;
    if (h->obs_tab == nullptr) return fail(OC_EHIP, "progress: the level table is not on the device");
    if (B == 0) return OC_OK;
    // one lane per word of the batch (four envs), whatever n: a lane walks its envs' n states
    const int64_t lanes = (B + 3) / 4;
    const dim3 grid((unsigned)((lanes + ocpg::kBlock - 1) / ocpg::kBlock));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_w(h, [&](auto a, auto k, auto w) {
        hipLaunchKernelGGL((ocpg::oc_progress_kernel<a(), k(), w()>), grid, dim3(ocpg::kBlock), 0, st, R, h->obs_tab,
                           (const uint8_t*)state_prev, (const uint8_t*)states, counts, events, reward);
        return hip_check("oc_progress launch");
    });
}

int oc_cpu_progress(const oc_handle* h, const void* state_prev, const void* states, int32_t n,
                    const oc_subtask* subtasks, int32_t num_subtasks, const float* weights, uint8_t* counts,
                    uint8_t* events, float* reward, int64_t B, int32_t nthreads) {
    if (h == nullptr || nthreads < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    ocpg::ProgArgs R;
    if (const int rc = progress_args(h, state_prev, states, n, subtasks, num_subtasks, weights, counts, events, reward, B, R))
        return rc;
    if (B == 0) return OC_OK;
    uint8_t tab[ocpg::kTableBytes];
    ocpg::build_table(h->obs_tab_host.data(), R.tile_words, tab);
    const int64_t words = (B + 3) / 4;
    // >= 16 Ki envs per thread: 4,096 words of four (ceil(ceil(B / 4) / 4096) = ceil(B / 16384))
    return host_ranges(h, nthreads, words, 4096, [&](auto a, auto k, auto w, int64_t g0, int64_t g1) {
        ocpg::cpu_progress_words<a(), k(), w()>(R, tab, (const uint8_t*)state_prev, (const uint8_t*)states, counts,
                                                events, reward, g0, g1);
        return OC_OK;
    });
}

int oc_set_start_cells(oc_handle* h, const uint8_t* agent_ok, const uint8_t* item_ok) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    std::vector<uint8_t> ok, tab;
    ocsd::StartArgs R;
    std::string err;
    if (const int rc = build_start(h, agent_ok, item_ok, ok, tab, R, err)) return fail(rc, "%s", err.c_str());
    if (h->start_tab != nullptr) (void)hipFree(h->start_tab);  // waits for the device
    h->start_tab = h->device >= 0 ? upload(h->device, tab.data(), tab.size()) : nullptr;
    h->start_ok.swap(ok);
    h->start_tab_host.swap(tab);
    h->start = R;
    h->start_rc = OC_OK;
    h->start_err.clear();
    return OC_OK;
}

int oc_get_start_cells(const oc_handle* h, uint8_t* agent_ok, uint8_t* item_ok) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    const size_t cells = (size_t)h->level.width * h->level.height, A = (size_t)h->A;
    if (agent_ok != nullptr) memcpy(agent_ok, h->start_ok.data(), A * cells);
    if (item_ok != nullptr) memcpy(item_ok, h->start_ok.data() + A * cells, cells);
    return OC_OK;
}

int oc_reset_random(const oc_handle* h, void* state, const void* state_prev, int64_t B, int64_t env_offset,
                    uint64_t seed, uint64_t round, int32_t what, void* stream) {
    if (h == nullptr) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    ocsd::StartArgs R;
    if (const int rc = start_args(h, state, B, env_offset, seed, round, what, state_prev != nullptr, R)) return rc;
    if (((uintptr_t)state | (uintptr_t)state_prev) & 7u) return fail(OC_EINVAL, "buffers must be 8-byte aligned");
    if (h->start_tab == nullptr) return fail(OC_EHIP, "reset_random: the start table is not on the device");
    if (B == 0) return OC_OK;
    const int64_t lanes = (B + kEPL - 1) / kEPL;  // one lane per word of the batch
    const dim3 grid((unsigned)((lanes + ocsd::kBlock - 1) / ocsd::kBlock));
    const int tab_words = (int)(h->start_tab_host.size() / 4);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_w(h, [&](auto a, auto k, auto w) {
        hipLaunchKernelGGL((oc_reset_random_kernel<a(), k(), w()>), grid, dim3(ocsd::kBlock), 0, st, h->args.sw, R,
                           (const uint32_t*)h->start_tab, tab_words, (uint8_t*)state, (const uint8_t*)state_prev);
        return hip_check("oc_reset_random launch");
    });
}

int oc_cpu_reset_random(const oc_handle* h, void* state, const void* state_prev, int64_t B, int64_t env_offset,
                        uint64_t seed, uint64_t round, int32_t what, int32_t nthreads) {
    if (h == nullptr || nthreads < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    ocsd::StartArgs R;
    if (const int rc = start_args(h, state, B, env_offset, seed, round, what, state_prev != nullptr, R)) return rc;
    if (B == 0) return OC_OK;
    const int64_t words = (B + kEPL - 1) / kEPL;
    // >= 4096 words (16 Ki envs) per thread
    return host_ranges(h, nthreads, words, 4096, [&](auto a, auto k, auto w, int64_t g0, int64_t g1) {
        ocsd::host_start_range<a(), k(), w()>(h->args.sw, R, h->start_tab_host.data(), (uint8_t*)state,
                                              (const uint8_t*)state_prev, g0, g1);
        return OC_OK;
    });
}

int oc_gen_actions(const oc_handle* h, uint8_t* actions, int64_t B, int64_t env_offset, int64_t step,
                   uint64_t seed, void* stream) {
    if (h == nullptr || actions == nullptr || B < 0 || env_offset < 0 || step < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    if (B == 0) return OC_OK;
    const int64_t P = pitch_for(B);
    hipLaunchKernelGGL(oc_gen_actions_kernel, dim3((unsigned)(P / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       actions, h->A, B, P, env_offset, (uint64_t)step, seed);
    return hip_check("oc_gen_actions launch");
}

int oc_state_checksum(const oc_handle* h, const void* state, int64_t B, uint64_t* out, void* stream) {
    if (h == nullptr || state == nullptr || out == nullptr || B < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, sizeof(uint64_t), s) != hipSuccess) return hip_check("oc_state_checksum memset");
    if (B == 0) return OC_OK;
    const int64_t P = pitch_for(B);
    const dim3 grid((unsigned)(P / kEnvsPerBlock));
    return dispatch_w(h, [&](auto a, auto k, auto w) {
        hipLaunchKernelGGL((oc_checksum_kernel<Planes<a(), k(), w()>::NP>), grid, dim3(kBlock), 0, s,
                           (const uint8_t*)state, P, B, (unsigned long long*)out);
        return hip_check("oc_state_checksum launch");
    });
}

int oc_stats_size(const oc_handle* h, int64_t B, int64_t* nbytes) {
    if (h == nullptr || nbytes == nullptr || B < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    const int64_t groups = ((int64_t)h->cus * 5 + kTicketGroup - 1) / kTicketGroup;  // oc_step_n's grid <= 5 blocks per CU
    *nbytes = (ticket_base(stats_rows(h, B)) + (1 + groups) * kTicketStride) * (int64_t)sizeof(uint64_t);
    return OC_OK;
}

int oc_stats_reduce(const oc_handle* h, const uint64_t* stats, int64_t B, uint64_t* totals, void* stream) {
    if (h == nullptr || stats == nullptr || totals == nullptr || B < 0) return fail(OC_EINVAL, "bad argument");
    ErrScope es_(h);
    OC_NEED_DEVICE(h);
    const int64_t rows = stats_rows(h, B);
    hipLaunchKernelGGL(oc_stats_reduce_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, stats, rows, totals);
    return hip_check("oc_stats_reduce launch");
}

}  // extern "C"
