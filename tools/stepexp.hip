// tools/stepexp.hip -- per-step kernel launch-shape experiments (includes the engine TU).
// Build: hipcc -O3 -std=c++20 --offload-arch=gfx950 -o tools/stepexp tools/stepexp.hip
// Workload: partial-divider_salad, 2 agents, B = 2^20, ping-pong state, fresh actions per step,
// stats on: the bench's per_step_launch line.  Every variant's final state is checked against
// the product kernel's.
#include "../gym-cooking_amd/csrc/oc_engine.hip"

#include <algorithm>
#include <vector>

#define CK(x)                                                                                      \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1); } \
    } while (0)

namespace {

// Non-persistent: lane g owns chunks g, g + nl/CH, ...: all CH chunks' loads issued first,
// then each stepped and stored.  BS threads per block.
template <int A, int K, int CH, int BS, int S = 1, int D = 0, bool MEMONLY = false, int CP = 0>
__global__ __launch_bounds__(BS) void step_flat(LevelArgs L, const uint8_t* __restrict__ sin, uint8_t* __restrict__ sout,
                                                const uint8_t* __restrict__ actions, uint8_t* __restrict__ exec_out,
                                                uint8_t* __restrict__ coll_out, uint64_t* __restrict__ stats) {
    const uint32_t P = (uint32_t)L.pitch, nlanes = P / kEPL, span = nlanes / CH;
    constexpr int NP = 3 * A + 2 * K + 3;
    Bufs b;
    b.sin = make_rsrc(sin, (int64_t)NP * P);
    b.sout = make_rsrc(sout, (int64_t)NP * P);
    b.act = make_rsrc(actions, (int64_t)A * P);
    b.ex = make_rsrc(exec_out, (int64_t)A * P);
    b.coll = make_rsrc(coll_out, (int64_t)P);
    const uint32_t g0 = blockIdx.x * (uint32_t)BS + threadIdx.x;
    if (S > 1) {  // cohort stagger: later blocks start loading later
        const uint32_t cohort = blockIdx.x * S / gridDim.x;
        for (uint32_t k = 0; k < cohort * D; ++k) __builtin_amdgcn_s_sleep(1);
    }
    Chunk<A, K> c[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) load_chunk<A, K>(c[i], b, P, g0 + i * span);
    __shared__ uint8_t tbl[256];
    for (int i = threadIdx.x; i < 256; i += BS) tbl[i] = (uint8_t)(L.cls4[i >> 2] >> (8 * (i & 3)));
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    StepStats st;
    if (MEMONLY) {
        constexpr int kPY = A, kPH = 2 * A, kPL = 3 * A, kPM = 3 * A + K, kPT = 3 * A + 2 * K, kPF = kPT + 2;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const uint32_t vo = (g0 + i * span) * 4u;
            for (int a = 0; a < A; ++a) {
                bst32<CP>(b.sout, c[i].wx[a] ^ tbl[a], vo, a * P);
                bst32<CP>(b.sout, c[i].wy[a], vo, (kPY + a) * P);
                bst32<CP>(b.sout, c[i].wh[a], vo, (kPH + a) * P);
                bst32<CP>(b.ex, c[i].wa[a], vo, a * P);
            }
            for (int j = 0; j < K; ++j) {
                bst32<CP>(b.sout, c[i].wl[j], vo, (kPL + j) * P);
                bst32<CP>(b.sout, c[i].wm[j], vo, (kPM + j) * P);
            }
            typedef unsigned int u32x2 __attribute__((__vector_size__(2 * sizeof(unsigned int))));
            const u32x2 tw = {c[i].t0, c[i].t1};
            __builtin_amdgcn_raw_buffer_store_b64(tw, b.sout, (int)((g0 + i * span) * 8u), (int)(kPT * P), CP);
            bst32<CP>(b.sout, c[i].wf, vo, kPF * P);
            bst32<CP>(b.coll, c[i].wf, vo, 0u);
        }
    } else {
#pragma unroll
        for (int i = 0; i < CH; ++i) step_chunk<A, K, CP>(L, tbl, c[i], b, true, true, P, g0 + i * span, st);
    }
    const uint32_t v[OC_NSTATS] = {wave_sum(st.eps), wave_sum(st.succ), wave_sum(st.steps), wave_sum(st.coll),
                                   wave_sum(st.err)};
    if ((threadIdx.x & 63u) == 0u) {
        unsigned long long* row = (unsigned long long*)stats + (int64_t)(blockIdx.x & 1023) * OC_NSTATS;
#pragma unroll
        for (int q = 0; q < OC_NSTATS; ++q)
            if (v[q]) atomicAdd(row + q, (unsigned long long)v[q]);
    }
}

// Wave timeline of one flat step launch: lane 0 of every wave records s_memrealtime (100 MHz)
// at start, when its loads have landed, when its stores are issued and when they are acked.
template <int A, int K, int BS, bool MEMONLY, int CP = 16>
__global__ __launch_bounds__(BS) void step_timeline(LevelArgs L, const uint8_t* __restrict__ sin,
                                                    uint8_t* __restrict__ sout, const uint8_t* __restrict__ actions,
                                                    uint8_t* __restrict__ exec_out, uint8_t* __restrict__ coll_out,
                                                    uint64_t* __restrict__ tl) {
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    const uint32_t P = (uint32_t)L.pitch;
    constexpr int NP = 3 * A + 2 * K + 3;
    Bufs b;
    b.sin = make_rsrc(sin, (int64_t)NP * P);
    b.sout = make_rsrc(sout, (int64_t)NP * P);
    b.act = make_rsrc(actions, (int64_t)A * P);
    b.ex = make_rsrc(exec_out, (int64_t)A * P);
    b.coll = make_rsrc(coll_out, (int64_t)P);
    const uint32_t g = blockIdx.x * (uint32_t)BS + threadIdx.x;
    Chunk<A, K> c;
    load_chunk<A, K>(c, b, P, g);
    __shared__ uint8_t tbl[256];
    for (int i = threadIdx.x; i < 256; i += BS) tbl[i] = (uint8_t)(L.cls4[i >> 2] >> (8 * (i & 3)));
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): every load landed
    const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
    StepStats st;
    if (MEMONLY) {
        constexpr int kPY = A, kPH = 2 * A, kPL = 3 * A, kPM = 3 * A + K, kPT = 3 * A + 2 * K, kPF = kPT + 2;
        const uint32_t vo = g * 4u;
        for (int a = 0; a < A; ++a) {
            bst32<CP>(b.sout, c.wx[a] ^ tbl[a], vo, a * P);
            bst32<CP>(b.sout, c.wy[a], vo, (kPY + a) * P);
            bst32<CP>(b.sout, c.wh[a], vo, (kPH + a) * P);
            bst32<CP>(b.ex, c.wa[a], vo, a * P);
        }
        for (int j = 0; j < K; ++j) {
            bst32<CP>(b.sout, c.wl[j], vo, (kPL + j) * P);
            bst32<CP>(b.sout, c.wm[j], vo, (kPM + j) * P);
        }
        typedef unsigned int u32x2 __attribute__((__vector_size__(2 * sizeof(unsigned int))));
        const u32x2 tw = {c.t0, c.t1};
        __builtin_amdgcn_raw_buffer_store_b64(tw, b.sout, (int)(g * 8u), (int)(kPT * P), CP);
        bst32<CP>(b.sout, c.wf, vo, kPF * P);
        bst32<CP>(b.coll, c.wf, vo, 0u);
    } else {
        step_chunk<A, K, CP>(L, tbl, c, b, true, true, P, g, st);
    }
    const uint64_t t2 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0x0F70);
    const uint64_t t3 = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63u) == 0u) {
        uint64_t* o = tl + (uint64_t)(g >> 6) * 5;
        o[0] = t0; o[1] = t1; o[2] = t2; o[3] = t3;
        o[4] = (uint64_t)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));  // HW_ID
    }
}

}  // namespace

static void timeline_report(const char* name, const std::vector<uint64_t>& t, int nw) {
    uint64_t base = ~0ull;
    for (int w = 0; w < nw; ++w) base = t[w * 5] < base ? t[w * 5] : base;
    std::vector<double> ev[4];
    double dur[3] = {0, 0, 0};
    for (int w = 0; w < nw; ++w) {
        for (int k = 0; k < 4; ++k) ev[k].push_back((t[w * 5 + k] - base) * 0.01);  // us
        for (int k = 0; k < 3; ++k) dur[k] += (t[w * 5 + k + 1] - t[w * 5 + k]) * 0.01;
    }
    printf("%s: %d waves; per-wave mean: load %.2f us, compute+issue %.2f us, store drain %.2f us\n", name, nw,
           dur[0] / nw, dur[1] / nw, dur[2] / nw);
    const char* nm[4] = {"start", "loaded", "issued", "acked"};
    for (int k = 0; k < 4; ++k) {
        std::sort(ev[k].begin(), ev[k].end());
        printf("  %-7s p0 %5.2f p10 %5.2f p25 %5.2f p50 %5.2f p75 %5.2f p90 %5.2f p100 %5.2f\n", nm[k], ev[k][0],
               ev[k][nw / 10], ev[k][nw / 4], ev[k][nw / 2], ev[k][3 * nw / 4], ev[k][9 * nw / 10], ev[k][nw - 1]);
    }
}

int main(int argc, char** argv) {
    const int64_t B = argc > 1 ? atoll(argv[1]) : (1ll << 20);
    const int A = 2, K = 4;
    oc_level_desc lv{};
    const char* rows[7] = {"-----t-", "/  -  l", "/  -  -", "*  -  -", "-  -  -", "-     p", "-----p-"};
    lv.width = 7;
    lv.height = 7;
    int ni = 0;
    for (int y = 0; y < 7; ++y)
        for (int x = 0; x < 7; ++x) {
            const char ch = rows[y][x];
            const int c = y * 7 + x;
            lv.tiles[c] = ch == ' ' ? 0 : ch == '/' ? 2 : ch == '*' ? 3 : 1;
            if (ch == 't' || ch == 'l' || ch == 'p') {
                lv.item_cell[ni] = (uint8_t)c;
                lv.item_mask[ni++] = ch == 't' ? 1 : ch == 'l' ? 2 : 8;
            }
        }
    lv.num_items = ni;
    lv.num_spawns = 4;
    const uint8_t sx[4] = {2, 4, 4, 2}, sy[4] = {1, 1, 4, 4};
    for (int a = 0; a < 4; ++a) { lv.spawn_x[a] = sx[a]; lv.spawn_y[a] = sy[a]; }
    lv.num_goals = 1;
    lv.goal_mask[0] = 0x3B;
    oc_handle* h;
    if (oc_create(&lv, A, 100, 0, &h) != 0) { printf("create: %s\n", oc_last_error()); return 1; }
    oc_layout lay;
    oc_get_layout(h, B, &lay);
    const int64_t P = lay.pitch, NP = lay.num_planes;
    const int R = 100;  // distinct action buffers, one per step of a run
    uint8_t *sa, *sb, *act, *ex, *coll;
    CK(hipMalloc(&sa, NP * P));
    CK(hipMalloc(&sb, NP * P));
    CK(hipMalloc(&act, (int64_t)R * A * P));
    CK(hipMalloc(&ex, A * P));
    CK(hipMalloc(&coll, P));
    uint64_t* stats;
    CK(hipMalloc(&stats, 1 << 20));
    CK(hipMemset(stats, 0, 1 << 20));
    for (int r = 0; r < R; ++r) oc_gen_actions(h, act + (int64_t)r * A * P, B, 0, r, 1, nullptr);
    CK(hipDeviceSynchronize());
    LevelArgs L = h->args;
    L.pitch = P;
    L.B = B;
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const double bytes = 39.0 * B;
    printf("B=%lld  algorithmic %.1f MB/step, %d steps per graph\n", (long long)B, bytes / 1e6, R);
    std::vector<uint8_t> ref(NP * P), got(NP * P);

    // run(step): R ping-pong steps from the reset state, as a hipGraph; returns us/step and
    // leaves the final state in sa (R even)
    auto run = [&](const char* name, auto step_fn) {
        hipGraph_t gr;
        hipGraphExec_t ge;
        CK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
        for (int r = 0; r < R; ++r) step_fn(r & 1 ? sb : sa, r & 1 ? sa : sb, act + (int64_t)r * A * P);
        CK(hipStreamEndCapture(s, &gr));
        CK(hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0));
        float best = 1e30f;
        for (int rep = 0; rep < 6; ++rep) {
            oc_reset(h, sa, B, s);
            CK(hipEventRecord(e0, s));
            CK(hipGraphLaunch(ge, s));
            CK(hipEventRecord(e1, s));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0 && ms < best) best = ms;
        }
        CK(hipMemcpy(got.data(), sa, NP * P, hipMemcpyDeviceToHost));
        const double us = best * 1000.0 / R;
        const bool same = ref.empty() || got == ref;
        printf("%-40s %7.2f us/step  %6.2f TB/s alg  %s\n", name, us, bytes / us / 1e6, same ? "ok" : "MISMATCH");
        CK(hipGraphExecDestroy(ge));
        CK(hipGraphDestroy(gr));
        return us;
    };
    ref.clear();
    run("product oc_step", [&](uint8_t* i, uint8_t* o, uint8_t* a) { oc_step(h, i, o, a, ex, coll, stats, B, s); });
    ref = got;
    const uint32_t nl = (uint32_t)(P / kEPL);
#define FLATX(NAME, CH, BS, ...)                                                                            \
    run(NAME, [&](uint8_t* i, uint8_t* o, uint8_t* a) {                                                       \
        hipLaunchKernelGGL((step_flat<2, 4, CH, BS, __VA_ARGS__>), dim3(nl / CH / BS), dim3(BS), 0, s, L, i, o, a, ex, coll, stats); \
    })
    ref.clear();
    // (oc_step_n launch-shape and cache-policy experiments: tools/stepnexp.hip)
    return 0;
}
