// TEST INFRASTRUCTURE: the host row function of oc_task_select (ocro::RowOps::task_env in
// gym-cooking_amd/csrc/oc_rollout.h, the row of oc_cpu_task_select) in a stand-alone program for
// AddressSanitizer / UBSan: a small kitchen, random state bytes (agents anywhere on the grid, dead
// and shared item cells, hold values that are no slot), random tables of every subtask kind, every
// flag combination, task states as a call leaves them and as a caller may leave them (any cur and
// cnt byte), ragged batch sizes, and buffers that end exactly at the last byte the contract allows
// (column B of the last plane).  Each env is compared with a scalar restatement built from the
// row's own pieces (hold_cells, goal_objects, full_bound) in the order include/oc_engine.h gives.
// The product library never contains this file.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define __device__
#define __host__

#include "../../gym-cooking_amd/csrc/oc_rollout.h"
#include "../../include/oc_engine.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// a 7x6 kitchen: counters around the border and a partial divider, a Cutboard and a Delivery
static const char* kMap[6] = {"#######", "#  #  #", "/  #  *", "#     #", "#  #  #", "#######"};

template <int A, int K>
static ocro::RowT<K> random_row(int W, int H) {
    ocro::RowT<K> r;
    for (int a = 0; a < A; ++a) {
        int x, y;
        do {
            x = 1 + rnd() % (W - 2);
            y = 1 + rnd() % (H - 2);
        } while (kMap[y][x] != ' ');
        r.x |= (uint32_t)x << (8 * a);
        r.y |= (uint32_t)y << (8 * a);
        r.h |= (uint32_t)(rnd() % 3 ? 0xFF : rnd() % (K + 2)) << (8 * a);
    }
    for (int j = 0; j < K; ++j) {
        r.set_loc(j, rnd() % 4 ? rnd() % (W * H) : 0xFF);
        r.set_mask(j, (uint32_t[]){0x01, 0x02, 0x11, 0x08, 0x19, 0x1B}[rnd() % 6]);
    }
    return r;
}

template <int A, int K>
static int run(int64_t B, int S, int M) {
    const int W = 7, H = 6;
    uint8_t tiles[OC_MAX_CELLS] = {};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const char c = kMap[y][x];
            tiles[y * W + x] = c == ' ' ? ocro::kFloor : c == '/' ? ocro::kCutboard : c == '*' ? ocro::kDelivery : ocro::kCounter;
        }
    std::vector<uint8_t> blob;
    ocro::RollLevel L;
    if (ocro::build_roll_level(L, blob, W, H, tiles, 0) < 0) return 1;
    const int64_t P = (B + 4095) / 4096 * 4096;
    const int EP = OC_PROGRESS_EVENT_PLANES(S), TP = OC_TASK_PLANES(S);
    // the table: agent m's rows at m * S, as the entry point lays them out
    std::vector<ocro::Sub> subs((size_t)(M * S));
    uint8_t agents[4] = {0, 1, 2, 3};
    for (int m = 0; m < M; ++m) {  // a random order of distinct agents
        const int q = m + (int)(rnd() % (uint32_t)(A - m));
        const uint8_t t = agents[m];
        agents[m] = agents[q];
        agents[q] = t;
    }
    for (int i = 0; i < S; ++i) {
        ocro::Sub s{};
        s.kind = (int32_t)(rnd() % 4);
        s.n = 1;
        s.start[0] = (uint8_t[]){0x01, 0x11, 0x19}[rnd() % 3];
        s.start[1] = (uint8_t[]){0x08, 0x02, 0x11}[rnd() % 3];
        s.goal = (uint8_t[]){0x11, 0x19, 0x1B}[rnd() % 3];
        for (int m = 0; m < M; ++m) {
            s.agent[0] = s.agent[1] = agents[m];
            subs[(size_t)(m * S + i)] = s;
        }
    }
    // buffers end at column B of their last plane: an access past B is a heap overflow
    const size_t nts = (size_t)((M * TP - 1) * P + B), nmb = (size_t)((M - 1) * P + B);
    uint8_t* ts = (uint8_t*)malloc(nts);
    float* bound = (float*)malloc(nmb * sizeof(float));
    uint8_t* info = (uint8_t*)malloc(nmb);
    int bad = 0;
    for (int64_t e = 0; e < B && !bad; ++e) {
        const int flags = (int)(rnd() % 8);
        const bool init = (flags & OC_TASK_INIT) != 0 || rnd() % 5 == 0;
        const bool nulls = rnd() % 7 == 0;
        const ocro::RowT<K> r = random_row<A, K>(W, H);
        // the env's task state before: a consistent one, now and then any bytes
        uint64_t inc0[4];
        int cur0[4], cnt0[4];
        for (int m = 0; m < M; ++m) {
            inc0[m] = (((uint64_t)rnd() << 32) | rnd()) & ((1ull << S) - 1ull);
            cur0[m] = rnd() % 9 == 0 ? (int)(rnd() % 256) : (int)(rnd() % (uint32_t)(S + 1));
            cnt0[m] = (int)(rnd() % 3);
            uint8_t* tm = ts + (int64_t)m * TP * P + e;
            for (int c = 0; c < EP; ++c) tm[c * P] = (uint8_t)(inc0[m] >> (8 * c));
            tm[EP * P] = (uint8_t)cur0[m];
            tm[(EP + 1) * P] = (uint8_t)cnt0[m];
        }
        ocro::RowOps<A, K, false, false, true> ops(L, blob.data());
        ops.task_env(r, subs.data(), S, M, flags, init, ts + e, nulls ? nullptr : bound + e, nulls ? nullptr : info + e, P);
        // the scalar restatement
        ocro::RowOps<A, K, false, false, true> o2(L, blob.data());
        ocro::RowT<K> rn = r;
        o2.hold_cells(rn);
        int held[4];
        for (int m = 0; m < M && !bad; ++m) {
            const ocro::Sub* sm = subs.data() + m * S;
            uint64_t inc = init ? (1ull << S) - 1ull : inc0[m];
            int cur = init ? S : cur0[m], cnt = init ? 0 : cnt0[m], fl = init ? OC_TASKF_REINIT : 0;
            const int entry = cur;
            if (cur < S && o2.goal_objects(rn, sm[cur]) > cnt) {
                inc &= ~(1ull << cur);
                cur = S;
                fl |= OC_TASKF_COMPLETED;
            }
            int pick = S;
            float best = 0.0f, keep_lb = 0.0f;
            bool keep = false;
            for (int i = 0; i < S; ++i) {
                if (!((inc >> i) & 1ull) || sm[i].kind == OC_SUB_NONE) continue;
                bool other = false;
                for (int q = 0; q < m; ++q) other |= (flags & OC_TASK_DISTINCT) && held[q] == i;
                float lb;
                if (other || !o2.full_bound(rn, sm[i], lb)) continue;
                if (pick == S || lb < best) pick = i, best = lb;
                if (i == cur) keep = true, keep_lb = lb;
            }
            if ((flags & OC_TASK_COMMIT) && keep) pick = cur, best = keep_lb;
            if (pick != cur && pick < S) cnt = o2.goal_objects(rn, sm[pick]);
            cur = pick;
            if (cur != entry) fl |= OC_TASKF_SWITCHED;
            held[m] = cur;
            const uint8_t* tm = ts + (int64_t)m * TP * P + e;
            uint64_t got = 0;
            for (int c = 0; c < EP; ++c) got |= (uint64_t)tm[c * P] << (8 * c);
            const float wb = cur < S ? best : 0.0f;
            if (got != inc || tm[EP * P] != cur || tm[(EP + 1) * P] != cnt)
                bad = printf("A%d K%d S%d e%lld m%d: state %llx %d %d vs %llx %d %d\n", A, K, S, (long long)e, m,
                             (unsigned long long)got, tm[EP * P], tm[(EP + 1) * P], (unsigned long long)inc, cur, cnt);
            if (!nulls && (memcmp(&wb, bound + m * P + e, 4) != 0 || info[m * P + e] != fl))
                bad = printf("A%d K%d S%d e%lld m%d: bound %g info %d vs %g %d\n", A, K, S, (long long)e, m,
                             bound[m * P + e], info[m * P + e], wb, fl);
        }
    }
    free(ts);
    free(bound);
    free(info);
    return bad != 0;
}

int main() {
    int bad = 0;
    for (int64_t B : {1, 7, 9, 300}) {
        bad |= run<1, 4>(B, 9, 1) | run<2, 4>(B, 9, 2) | run<3, 8>(B, 21, 3) | run<4, 16>(B, 16, 4) | run<2, 8>(B, 63, 1);
    }
    printf(bad ? "FAILED\n" : "taskselect_asan: all builds, sizes, tables and flags clean and equal to the scalar restatement\n");
    return bad;
}
