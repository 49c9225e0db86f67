// TEST INFRASTRUCTURE: the host functions of gym-cooking_amd/csrc/oc_progress.h (the worker of
// oc_cpu_progress) in a stand-alone program for AddressSanitizer / UBSan: random state bytes
// (every byte value in every plane, so dead cells, hold values that are no slot and cells past
// the grid all occur), every (A, K, narrow / wide) build, ragged batch sizes, and buffers that end
// exactly where the contract says the last byte may be read or written.  Also checks the
// counts against a per-env scalar restatement.  The product library never contains this file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline

#include "../../gym-cooking_amd/csrc/oc_progress.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// count_i of env e, one env at a time (include/oc_engine.h)
template <int A, int K, bool WIDE>
static int scalar_count(const uint8_t* s, int64_t P, int64_t e, int W, const uint8_t* tab, int kind, int goal) {
    using PL = ocly::Planes<A, K, WIDE>;
    if (kind == OC_SUB_NONE) return 0;
    int cells[K], n = 0, cnt = 0;
    for (int j = 0; j < K; ++j) {
        int c = s[(PL::LOC + j) * P + e] | (WIDE ? s[(PL::LOC_HI + j) * P + e] << 8 : 0);
        if (c == (WIDE ? 0xFFFF : 0xFF) || s[(PL::MASK + j) * P + e] != goal) continue;
        int holder = -1;
        for (int a = A - 1; a >= 0; --a)
            if (s[(PL::HOLD + a) * P + e] == j) holder = a;
        if (kind == OC_SUB_DELIVER) {
            cnt += holder < 0 && tab[WIDE ? c & 1023 : c] != 0;
            continue;
        }
        if (holder >= 0) c = (s[(PL::Y + holder) * P + e] * W + s[(PL::X + holder) * P + e]) & (WIDE ? 0xFFFF : 0xFF);
        bool seen = false;
        for (int i = 0; i < n; ++i) seen |= cells[i] == c;
        if (!seen) cells[n++] = c;
    }
    return kind == OC_SUB_DELIVER ? cnt : n;
}

template <int A, int K, bool WIDE>
static int run(int64_t B, int n, int S) {
    using PL = ocly::Planes<A, K, WIDE>;
    const int64_t P = (B + 4095) / 4096 * 4096;
    const int W = WIDE ? 31 : 15, H = WIDE ? 31 : 16, cells = W * H;
    std::vector<uint8_t> tiles((cells + 3) & ~3, 0);
    for (int c = 0; c < cells; ++c) tiles[c] = (uint8_t)(rnd() % 4);
    uint8_t tab[ocpg::kTableBytes];
    ocpg::build_table(tiles.data(), (cells + 3) / 4, tab);
    ocpg::ProgArgs R{};
    R.W = W;
    R.tile_words = (cells + 3) / 4;
    R.n = n;
    R.S = S;
    R.planes = OC_PROGRESS_EVENT_PLANES(S);
    R.pitch = P;
    R.B = B;
    R.state_bytes = (int64_t)PL::NP * P;
    for (int i = 0; i < S; ++i) {
        R.sub[i] = (rnd() % 4) << 8 | (rnd() % 3);  // few masks: matches are common
        R.weight[i] = 0.1f * (float)(i + 1);
    }
    // the states: n + 1 buffers, each ending exactly at its last plane's pitch
    std::vector<std::vector<uint8_t>> st;
    for (int r = 0; r <= n; ++r) {
        st.emplace_back((size_t)R.state_bytes);
        for (auto& b : st.back()) b = (uint8_t)rnd();
        for (int j = 0; j < K; ++j)
            for (int64_t e = 0; e < P; ++e) {
                uint8_t* s = st.back().data();
                s[(PL::MASK + j) * P + e] %= 3;
                if (!WIDE) s[(PL::LOC + j) * P + e] = rnd() % 8 ? (uint8_t)(rnd() % 12) : 0xFF;  // shared squares
                else if (rnd() % 8 == 0) s[(PL::LOC + j) * P + e] = s[(PL::LOC_HI + j) * P + e] = 0xFF;
                else s[(PL::LOC_HI + j) * P + e] &= 3, s[(PL::LOC + j) * P + e] %= 6;
            }
        for (int a = 0; a < A; ++a)
            for (int64_t e = 0; e < P; ++e) {
                uint8_t* s = st.back().data();
                s[(PL::X + a) * P + e] %= W;
                s[(PL::Y + a) * P + e] %= H;
                if (rnd() % 2) s[(PL::HOLD + a) * P + e] %= (K + 2);  // slots, and two values that are none
            }
    }
    std::vector<uint8_t> traj((size_t)R.state_bytes * n);
    for (int r = 0; r < n; ++r) memcpy(traj.data() + (size_t)r * R.state_bytes, st[r + 1].data(), (size_t)R.state_bytes);
    // outputs end at column B of their last plane: a write past B is a heap overflow
    const size_t nc = (size_t)((int64_t)(n * S - 1) * P + B), ne = (size_t)((int64_t)(n * R.planes - 1) * P + B);
    const size_t nr = (size_t)((int64_t)(n - 1) * P + B);
    uint8_t* counts = (uint8_t*)malloc(nc);
    uint8_t* events = (uint8_t*)malloc(ne);
    float* reward = (float*)malloc(nr * sizeof(float));
    memset(counts, 0xA5, nc);
    memset(events, 0xA5, ne);
    ocpg::cpu_progress_words<A, K, WIDE>(R, tab, st[0].data(), traj.data(), counts, events, reward, 0, (B + 3) / 4);
    ocpg::cpu_progress_words<A, K, WIDE>(R, tab, st[0].data(), traj.data(), counts, nullptr, nullptr, 0, (B + 3) / 4);
    ocpg::cpu_progress_words<A, K, WIDE>(R, tab, st[0].data(), traj.data(), nullptr, events, nullptr, 0, (B + 3) / 4);
    ocpg::cpu_progress_words<A, K, WIDE>(R, tab, st[0].data(), traj.data(), nullptr, nullptr, reward, 0, (B + 3) / 4);
    int bad = 0;
    for (int r = 0; r < n && !bad; ++r)
        for (int64_t e = 0; e < B && !bad; ++e) {
            const bool was_done = st[r][PL::F * P + e] & OC_FLAG_DONE;
            float rw = 0.0f;
            for (int i = 0; i < S; ++i) {
                const int kind = (int)(R.sub[i] >> 8), goal = (int)(R.sub[i] & 0xFF);
                const int cp = scalar_count<A, K, WIDE>(st[r].data(), P, e, W, tab, kind, goal);
                const int cc = scalar_count<A, K, WIDE>(st[r + 1].data(), P, e, W, tab, kind, goal);
                const bool ev = !was_done && cc > cp;
                if (ev) rw += R.weight[i];
                const int got_c = counts[((int64_t)r * S + i) * P + e];
                const int got_e = (events[((int64_t)r * R.planes + (i >> 3)) * P + e] >> (i & 7)) & 1;
                if (got_c != cc || got_e != (int)ev) {
                    printf("A%d K%d wide%d B%lld r%d e%lld sub%d kind%d: count %d vs %d, event %d vs %d\n", A, K, (int)WIDE,
                           (long long)B, r, (long long)e, i, kind, got_c, cc, got_e, (int)ev);
                    bad = 1;
                    break;
                }
            }
            if (!bad && memcmp(&rw, &reward[(int64_t)r * P + e], 4) != 0) {
                printf("A%d K%d wide%d B%lld r%d e%lld: reward bits differ\n", A, K, (int)WIDE, (long long)B, r, (long long)e);
                bad = 1;
            }
        }
    free(counts);
    free(events);
    free(reward);
    return bad;
}

template <int K, bool WIDE>
static int run_agents(int64_t B, int n, int S) {
    return run<1, K, WIDE>(B, n, S) | run<2, K, WIDE>(B, n, S) | run<3, K, WIDE>(B, n, S) | run<4, K, WIDE>(B, n, S);
}

int main() {
    int bad = 0;
    const int64_t sizes[] = {1, 2, 3, 4, 5, 63, 4097};
    for (int64_t B : sizes)
        for (int S : {1, 8, 9, 64}) {
            const int n = B > 100 ? 2 : 3;
            bad |= run_agents<4, false>(B, n, S) | run_agents<8, false>(B, n, S) | run_agents<16, false>(B, n, S);
            bad |= run_agents<4, true>(B, n, S) | run_agents<8, true>(B, n, S) | run_agents<16, true>(B, n, S);
        }
    printf(bad ? "FAILED\n" : "progress_asan: all builds, sizes and subtask counts clean and equal to the scalar restatement\n");
    return bad;
}
