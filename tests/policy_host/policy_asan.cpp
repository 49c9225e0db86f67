// TEST INFRASTRUCTURE: the host row function of oc_nav_policy (ocro::RowOps::policy in
// gym-cooking_amd/csrc/oc_rollout.h, the row of oc_cpu_nav_policy) in a stand-alone program for
// AddressSanitizer / UBSan: a small kitchen, random state bytes (agents anywhere on the grid,
// co-located ones included, dead and shared item cells, hold values that are no slot), every
// subtask kind with one and two agents, both choice and both count modes, ragged batch sizes, and
// output buffers that end exactly at the last byte the contract allows (column B of the last
// plane).  Each row is compared with a scalar restatement built from the row's own pieces
// (action_legal, q_value_count, goal_objects) in the order include/oc_engine.h gives.  The
// product library never contains this file.
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
        do {  // agents on Floor squares, now and then on one another
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
static int run(int64_t B) {
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
    // outputs end at column B of their last plane: a write past B is a heap overflow
    uint8_t* actions = (uint8_t*)malloc((size_t)((A - 1) * P + B));
    uint8_t* flags = (uint8_t*)malloc((size_t)B);
    double* probs = (double*)malloc((size_t)(24 * P + B) * sizeof(double));
    memset(actions, 0xEE, (size_t)((A - 1) * P + B));
    int bad = 0;
    for (int64_t e = 0; e < B && !bad; ++e) {
        ocro::Sub s{};
        s.kind = (int32_t)(rnd() % 4);
        s.n = A >= 2 ? 1 + (int32_t)(rnd() % 2) : 1;
        s.agent[0] = (uint8_t)(rnd() % (A - s.n + 1));
        s.agent[1] = s.n == 2 ? (uint8_t)(s.agent[0] + 1 + rnd() % (A - s.agent[0] - 1)) : s.agent[0];
        s.start[0] = 0x01;
        s.start[1] = 0x08;
        s.goal = (uint8_t[]){0x11, 0x19, 0x1B}[rnd() % 3];
        s.count = (uint8_t)(rnd() % 2);
        const int mode = (int)(rnd() % 4);
        const double beta = 1.3, nap = 0.5, u = ocro::policy_u(7, e, 3, s.agent[0]);
        const ocro::RowT<K> r = random_row<A, K>(W, H);
        ocro::RowOps<A, K, false, true, true> ops(L, blob.data());
        double p[25];
        int a0, a1;
        const int f = ops.policy(r, s, beta, nap, mode, u, p, a0, a1);
        // the call's stores
        actions[s.agent[0] * P + e] = (uint8_t)a0;
        if (s.n == 2) actions[s.agent[1] * P + e] = (uint8_t)a1;
        for (int k = 0; k < 25; ++k) probs[k * P + e] = p[k];
        flags[e] = (uint8_t)f;
        // the scalar restatement (subtask rows; the None row's closed form is summed below)
        double sum = 0.0;
        for (int k = 0; k < 25; ++k) sum += p[k];
        if (f == OC_POL_OK && fabs(sum - 1.0) > 1e-12) bad = printf("A%d K%d e%lld: sum %.17g\n", A, K, (long long)e, sum);
        if (f != OC_POL_OK && (sum != 0.0 || a0 != ocro::kNoop || a1 != ocro::kNoop)) bad = printf("A%d K%d e%lld: raising row not empty\n", A, K, (long long)e);
        if (s.kind == 0 || f != OC_POL_OK) continue;
        ocro::RowOps<A, K, false, true, true> o2(L, blob.data());
        ocro::RowT<K> r0 = r;
        if (o2.level0(r0, s)) bad = printf("A%d K%d e%lld: OK on a raising view\n", A, K, (long long)e);
        const int count = mode & 2 ? o2.goal_objects(r0, s) : s.count, nc = s.n == 2 ? 25 : 5;
        double q[25], m = 1e300, S = 0.0;
        bool lg[25];
        for (int k = 0; k < nc; ++k) {
            const int c0 = s.n == 2 ? k / 5 : k, c1 = s.n == 2 ? k % 5 : ocro::kNoop;
            lg[k] = o2.action_legal(r0, s, c0, c1) && o2.q_value_count(r0, s, c0, c1, count, q[k]);
            if (lg[k] && q[k] < m) m = q[k];
        }
        int greedy = -1, pick = -1, hi = -1;
        for (int k = 0; k < nc; ++k)
            if (lg[k]) S += exp(beta * (m - q[k]));
        double c = 0.0;
        for (int k = 0; k < nc; ++k) {
            const double pk = lg[k] ? exp(beta * (m - q[k])) / S : 0.0;
            if (memcmp(&pk, &p[k], 8) != 0) bad = printf("A%d K%d e%lld k%d: p %.17g vs %.17g\n", A, K, (long long)e, k, p[k], pk);
            if (lg[k] && greedy < 0 && q[k] == m) greedy = k;
            c += pk;
            if (pick < 0 && u < c) pick = k;
            if (lg[k]) hi = k;
        }
        const int want = mode & 1 ? greedy : (pick < 0 ? hi : pick), got = s.n == 2 ? a0 * 5 + a1 : a0;
        if (want != got) bad = printf("A%d K%d e%lld mode %d: action %d vs %d\n", A, K, (long long)e, mode, got, want);
    }
    free(actions);
    free(flags);
    free(probs);
    return bad != 0;
}

int main() {
    int bad = 0;
    for (int64_t B : {1, 7, 9, 4097}) {
        bad |= run<1, 4>(B) | run<2, 4>(B) | run<3, 8>(B) | run<4, 16>(B);
    }
    printf(bad ? "FAILED\n" : "policy_asan: all builds, sizes and modes clean and equal to the scalar restatement\n");
    return bad;
}
