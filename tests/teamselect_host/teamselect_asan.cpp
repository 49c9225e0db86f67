// TEST INFRASTRUCTURE: the host row function of oc_team_select (ocro::RowOps::team_env in
// gym-cooking_amd/csrc/oc_rollout.h, the row of oc_cpu_team_select) in a stand-alone program for
// AddressSanitizer / UBSan: a small kitchen, random state bytes (agents anywhere on the grid, dead
// and shared item cells, hold values that are no slot), random tables of every subtask kind, every
// flag combination, team states as a call leaves them and as a caller may leave them (any cur and
// cnt byte), ragged batch sizes, and buffers that end exactly at the last byte the contract allows
// (column B of the last plane).  Each env is compared with a scalar restatement that keeps the
// weights of all rows in arrays and searches every admissible pair, built from the row's own
// pieces (hold_cells, goal_objects, full_bound) in the order include/oc_engine.h gives.
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
static int run(int64_t B, int S) {
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
    const int EP = OC_PROGRESS_EVENT_PLANES(S), TP = OC_TEAM_PLANES(S);
    // the table as the entry point lays it out: a0's rows, a1's rows, the two-agent rows
    int a0 = (int)(rnd() % (uint32_t)A), a1 = (int)(rnd() % (uint32_t)A);
    if (a0 == a1) a1 = (a0 + 1) % A;
    if (a0 > a1) {
        const int t = a0;
        a0 = a1, a1 = t;
    }
    std::vector<ocro::Sub> subs((size_t)(3 * S));
    for (int i = 0; i < S; ++i) {
        ocro::Sub s{};
        s.kind = (int32_t)(rnd() % 4);
        s.start[0] = (uint8_t[]){0x01, 0x11, 0x19}[rnd() % 3];
        s.start[1] = (uint8_t[]){0x08, 0x02, 0x11}[rnd() % 3];
        s.goal = (uint8_t[]){0x11, 0x19, 0x1B}[rnd() % 3];
        s.n = 1;
        s.agent[0] = s.agent[1] = (uint8_t)a0;
        subs[(size_t)i] = s;
        s.agent[0] = s.agent[1] = (uint8_t)a1;
        subs[(size_t)(S + i)] = s;
        if (s.kind != OC_SUB_NONE) {
            s.n = 2;
            s.agent[0] = (uint8_t)a0;
        }
        subs[(size_t)(2 * S + i)] = s;
    }
    // buffers end at column B of their last plane: an access past B is a heap overflow
    uint8_t* ts = (uint8_t*)malloc((size_t)((TP - 1) * P + B));
    float* bound = (float*)malloc((size_t)(P + B) * sizeof(float));
    uint8_t* info = (uint8_t*)malloc((size_t)B);
    int bad = 0;
    for (int64_t e = 0; e < B && !bad; ++e) {
        const int flags = (int)(rnd() % 8);
        const bool init = (flags & OC_TEAM_INIT) != 0 || rnd() % 5 == 0;
        const bool nulls = rnd() % 7 == 0;
        const ocro::RowT<K> r = random_row<A, K>(W, H);
        // the env's team state before: a consistent one, now and then any bytes
        const uint32_t all = (1u << S) - 1u;
        const uint32_t inc0 = rnd() & all;
        int c0[3], n0[2];
        if (rnd() % 9 == 0) {
            for (int q = 0; q < 3; ++q) c0[q] = (int)(rnd() % 256);
        } else if (rnd() % 2) {
            c0[0] = c0[1] = OC_TEAM_OUT, c0[2] = (int)(rnd() % (uint32_t)S);
        } else {
            c0[0] = (int)(rnd() % (uint32_t)(S + 1)), c0[1] = (int)(rnd() % (uint32_t)(S + 1)), c0[2] = OC_TEAM_OUT;
        }
        n0[0] = (int)(rnd() % 3), n0[1] = (int)(rnd() % 3);
        for (int c = 0; c < EP; ++c) ts[c * P + e] = (uint8_t)(inc0 >> (8 * c));
        for (int q = 0; q < 3; ++q) ts[(EP + q) * P + e] = (uint8_t)c0[q];
        for (int q = 0; q < 2; ++q) ts[(EP + 3 + q) * P + e] = (uint8_t)n0[q];
        ocro::RowOps<A, K, false, false, true> ops(L, blob.data());
        ops.team_env(r, subs.data(), S, flags, init, ts + e, nulls ? nullptr : bound + e, nulls ? nullptr : info + e, P);

        // the scalar restatement: all weights in arrays, every admissible pair searched
        ocro::RowOps<A, K, false, false, true> o2(L, blob.data());
        ocro::RowT<K> rn = r;
        o2.hold_cells(rn);
        uint32_t inc = init ? all : inc0;
        int cur0 = init ? S : c0[0], cur1 = init ? S : c0[1], curJ = init ? OC_TEAM_OUT : c0[2];
        int cnt0 = init ? 0 : n0[0], cnt1 = init ? 0 : n0[1], fl = init ? OC_TEAMF_REINIT : 0;
        const int e0 = cur0, e1 = cur1, eJ = curJ;
        auto count = [&](int i) { return o2.goal_objects(rn, subs[(size_t)i]); };
        if (curJ < S) {
            if (count(curJ) > cnt0) inc &= ~(1u << curJ), fl |= OC_TEAMF_COMPLETED0 | OC_TEAMF_COMPLETED1;
        } else {
            if (cur0 < S && count(cur0) > cnt0) inc &= ~(1u << cur0), fl |= OC_TEAMF_COMPLETED0;
            if (cur1 < S && count(cur1) > cnt1) inc &= ~(1u << cur1), fl |= OC_TEAMF_COMPLETED1;
        }
        const bool dropped = (fl & (OC_TEAMF_COMPLETED0 | OC_TEAMF_COMPLETED1)) != 0;
        if (dropped) cur0 = cur1 = S, curJ = OC_TEAM_OUT;
        bool C[3][OC_TEAM_MAX_SUBTASKS + 1] = {};
        double w[3][OC_TEAM_MAX_SUBTASKS + 1] = {};  // index S: None, +0.0
        float lb[3][OC_TEAM_MAX_SUBTASKS + 1] = {};
        for (int q = 0; q < 3; ++q)
            for (int i = 0; i < S; ++i) {
                if (!((inc >> i) & 1u) || subs[(size_t)i].kind == OC_SUB_NONE) continue;
                float v;
                if (!o2.full_bound(rn, subs[(size_t)(q * S + i)], v)) continue;
                C[q][i] = true, lb[q][i] = v, w[q][i] = 1.0 / (double)v;
            }
        bool keep = false;
        if ((flags & OC_TEAM_COMMIT) && !dropped)
            keep = curJ < S ? C[2][curJ] : cur0 < S && cur1 < S && C[0][cur0] && C[1][cur1];
        if (!keep) {
            // the rule's split pick from whole-array searches, and its sum against the largest sum of
            // an exhaustive search over every admissible (i, j): i != j, None (S) for one member only
            auto first = [&](int q, int skip) {
                int f = S;
                for (int i = 0; i < S; ++i)
                    if (C[q][i] && i != skip && (f == S || w[q][i] > w[q][f])) f = i;
                return f;
            };
            const int f0 = first(0, -1), f1 = first(1, -1);
            int p0 = f0, p1 = f1;
            const bool have = f0 < S || f1 < S;
            if (have && f0 == f1) {
                const int s0 = first(0, f0), s1 = first(1, f1);
                if (w[0][f0] + w[1][s1] >= w[0][s0] + w[1][f1]) p1 = s1;
                else p0 = s0;
            }
            const double wS = w[0][p0] + w[1][p1];
            double most = -1.0;
            for (int i = 0; i <= S; ++i)
                for (int j = 0; j <= S; ++j) {
                    if ((i == S && j == S) || (i < S && !C[0][i]) || (j < S && !C[1][j]) || (i == j)) continue;
                    const double v = w[0][i] + w[1][j];
                    most = v > most ? v : most;
                }
            if (have ? most != wS : most != -1.0)
                bad = printf("A%d K%d S%d e%lld: the pick's sum %g is not the argmax %g\n", A, K, S, (long long)e, wS, most);
            const int iJ = first(2, -1);
            const bool full = p0 < S && p1 < S;
            if ((flags & OC_TEAM_SPLIT_FIRST) && have && full) cur0 = p0, cur1 = p1, curJ = OC_TEAM_OUT;
            else if (iJ < S && (!have || w[2][iJ] >= wS)) cur0 = cur1 = OC_TEAM_OUT, curJ = iJ;
            else if (have) cur0 = p0, cur1 = p1, curJ = OC_TEAM_OUT;
            else cur0 = cur1 = S, curJ = OC_TEAM_OUT, fl |= OC_TEAMF_IDLE;
        }
        if (cur0 != e0 || cur1 != e1 || curJ != eJ) {
            fl |= OC_TEAMF_SWITCHED;
            cnt0 = curJ < S ? count(curJ) : cur0 < S ? count(cur0) : 0;
            cnt1 = curJ >= S && cur1 < S ? count(cur1) : 0;
        }
        if (curJ < S) fl |= OC_TEAMF_JOINT;
        const float wb0 = curJ < S ? lb[2][curJ] : cur0 < S ? lb[0][cur0] : 0.0f;
        const float wb1 = curJ < S ? lb[2][curJ] : cur1 < S ? lb[1][cur1] : 0.0f;
        uint32_t got = 0;
        for (int c = 0; c < EP; ++c) got |= (uint32_t)ts[c * P + e] << (8 * c);
        const uint8_t* t = ts + EP * P + e;
        if (got != inc || t[0] != (uint8_t)cur0 || t[P] != (uint8_t)cur1 || t[2 * P] != (uint8_t)curJ || t[3 * P] != cnt0 ||
            t[4 * P] != cnt1)
            bad = printf("A%d K%d S%d e%lld: state %x %d %d %d %d %d vs %x %d %d %d %d %d\n", A, K, S, (long long)e, got, t[0],
                         t[P], t[2 * P], t[3 * P], t[4 * P], inc, cur0, cur1, curJ, cnt0, cnt1);
        if (!nulls && (memcmp(&wb0, bound + e, 4) != 0 || memcmp(&wb1, bound + P + e, 4) != 0 || info[e] != fl))
            bad = printf("A%d K%d S%d e%lld: bound %g %g info %d vs %g %g %d\n", A, K, S, (long long)e, bound[e], bound[P + e],
                         info[e], wb0, wb1, fl);
    }
    free(ts);
    free(bound);
    free(info);
    return bad != 0;
}

int main() {
    int bad = 0;
    for (int64_t B : {1, 7, 9, 300}) {
        bad |= run<2, 4>(B, 9) | run<3, 4>(B, 1) | run<4, 4>(B, 21) | run<2, 8>(B, 21) | run<3, 8>(B, 8) | run<4, 8>(B, 16) |
               run<2, 16>(B, 17) | run<3, 16>(B, 21) | run<4, 16>(B, 6);
    }
    printf(bad ? "FAILED\n" : "teamselect_asan: all builds, sizes, tables and flags clean and equal to the scalar restatement\n");
    return bad;
}
