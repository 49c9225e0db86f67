// TEST INFRASTRUCTURE: the host row function of oc_belief_update (ocro::RowOps::belief_env in
// gym-cooking_amd/csrc/oc_rollout.h, the row of oc_cpu_belief_update) in a stand-alone program for
// AddressSanitizer / UBSan: a small kitchen, random state bytes (agents anywhere on the floor, dead
// and shared item cells, hold values that are no slot), random tables of every subtask kind, every
// (A, K, wide) build, random taken actions (codes past 4 too) and events, belief states as a call
// leaves them and as a caller may leave them (any open / live bits), ragged batch sizes, and
// buffers that end exactly at the last byte the contract allows (column B of the last plane).  Each
// env is compared with a scalar restatement built from the row's own pieces (full_bound, level0,
// single_legal, interact, goal_objects, lower_bound, none_movable, none_probs) in the order
// include/oc_engine.h gives.  The product library never contains this file.
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

// a 7x6 kitchen: counters around the border and a partial divider, a Cutboard and a Delivery; the
// wide build runs the same kitchen in the middle of a 20x13 one (260 cells: u16 cell ids)
static const char* kMap[6] = {"#######", "#  #  #", "/  #  *", "#     #", "#  #  #", "#######"};

template <int A, int K, bool W>
static ocro::RowT<K, W> random_row(int Wd, int H, const uint8_t* tiles) {
    ocro::RowT<K, W> r;
    for (int a = 0; a < A; ++a) {
        int x, y;
        do {
            x = (int)(rnd() % (uint32_t)Wd);
            y = (int)(rnd() % (uint32_t)H);
        } while (tiles[y * Wd + x] != ocro::kFloor);
        r.x |= (uint32_t)x << (8 * a);
        r.y |= (uint32_t)y << (8 * a);
        r.h |= (uint32_t)(rnd() % 3 ? 0xFF : rnd() % (K + 2)) << (8 * a);
    }
    for (int j = 0; j < K; ++j) {
        r.set_loc(j, rnd() % 4 ? rnd() % (uint32_t)(Wd * H) : (uint32_t)ocro::RowT<K, W>::kDead);
        r.set_mask(j, (uint32_t[]){0x01, 0x02, 0x11, 0x08, 0x19, 0x1B}[rnd() % 6]);
    }
    return r;
}

template <int A, int K, bool W>
static int run(int64_t B, int S, int M) {
    using Row = ocro::RowT<K, W>;
    using Ops = ocro::RowOps<A, K, W, true, true>;
    const int Wd = W ? 20 : 7, H = W ? 13 : 6, ox = W ? 6 : 0, oy = W ? 3 : 0;
    uint8_t tiles[OC_MAX_CELLS] = {};
    for (int c = 0; c < Wd * H; ++c) tiles[c] = ocro::kCounter;
    for (int y = 0; y < 6; ++y)
        for (int x = 0; x < 7; ++x) {
            const char c = kMap[y][x];
            tiles[(y + oy) * Wd + x + ox] = c == ' ' ? ocro::kFloor : c == '/' ? ocro::kCutboard : c == '*' ? ocro::kDelivery : ocro::kCounter;
        }
    std::vector<uint8_t> blob;
    ocro::RollLevel L;
    if (ocro::build_roll_level(L, blob, Wd, H, tiles, 0) < 0) return 1;
    const int64_t P = (B + 4095) / 4096 * 4096;
    const int HP = OC_BELIEF_PLANES(S);
    const uint64_t subm = (1ull << S) - 1ull, all = subm | 1ull << S;
    std::vector<ocro::Sub> subs((size_t)S);
    uint64_t fresh = 1ull << S;
    for (int i = 0; i < S; ++i) {
        ocro::Sub s{};
        s.kind = (int32_t)(rnd() % 4);
        s.n = 1;
        s.start[0] = (uint8_t[]){0x01, 0x11, 0x19}[rnd() % 3];
        s.start[1] = (uint8_t[]){0x08, 0x02, 0x11}[rnd() % 3];
        s.goal = (uint8_t[]){0x11, 0x19, 0x1B}[rnd() % 3];
        subs[(size_t)i] = s;
        if (s.kind != 0) fresh |= 1ull << i;
    }
    // buffers end at column B of their last plane: an access past B is a heap overflow
    const size_t nbel = (size_t)((M * (S + 1) - 1) * P + B), nbs = (size_t)((M * 2 * HP - 1) * P + B);
    const size_t nmb = (size_t)((M - 1) * P + B);
    double* bel = (double*)malloc(nbel * sizeof(double));
    uint8_t* bs = (uint8_t*)malloc(nbs);
    uint8_t* map = (uint8_t*)malloc(nmb);
    uint8_t* info = (uint8_t*)malloc(nmb);
    const double beta = 1.3, nap = 0.5;
    int bad = 0;
    for (int64_t e = 0; e < B && !bad; ++e) {
        const bool init = rnd() % 5 == 0, nulls = rnd() % 7 == 0;
        const Row r = random_row<A, K, W>(Wd, H, tiles);
        const uint64_t ev = rnd() % 3 == 0 ? (((uint64_t)rnd() << 32) | rnd()) & subm & (rnd() % 2 ? ~0ull : 0x11ull) : 0ull;
        for (int m = 0; m < M && !bad; ++m) {
            const int a = (m + (int)(e % A)) % A;  // distinct per m
            const int taken = rnd() % 9 == 0 ? (int)(rnd() % 256) : (int)(rnd() % 5);
            // the belief state before: a consistent one, now and then any bits
            uint64_t open0 = fresh & ((((uint64_t)rnd() << 32) | rnd()) | 1ull << S), live0 = open0 & (((uint64_t)rnd() << 32) | rnd() | 1ull << S);
            if (rnd() % 9 == 0) {
                open0 = (((uint64_t)rnd() << 32) | rnd()) & all;
                live0 = (((uint64_t)rnd() << 32) | rnd()) & all;
            }
            double b0[64];
            double* be = bel + (int64_t)m * (S + 1) * P + e;
            uint8_t* se = bs + (int64_t)m * 2 * HP * P + e;
            for (int i = 0; i <= S; ++i) be[i * P] = b0[i] = (live0 >> i) & 1ull ? (double)(1 + rnd() % 1000) / 4096.0 : 0.0;
            if (rnd() % 11 == 0)
                for (int i = 0; i <= S; ++i) be[i * P] = b0[i] = 0.0;  // the total == 0 branch
            for (int c = 0; c < HP; ++c) {
                se[c * P] = (uint8_t)(open0 >> (8 * c));
                se[(HP + c) * P] = (uint8_t)(live0 >> (8 * c));
            }
            Ops ops(L, blob.data());
            ops.belief_env(r, subs.data(), S, a, taken, ev, init, beta, nap, be, se, nulls ? nullptr : map + m * P + e,
                           nulls ? nullptr : info + m * P + e, P);
            // the scalar restatement
            uint64_t open = open0, live = live0;
            int fl = 0;
            double b[64];
            for (int i = 0; i <= S; ++i) b[i] = b0[i];
            auto row_of = [&](int i) {
                ocro::Sub s = subs[(size_t)i];
                s.agent[0] = s.agent[1] = (uint8_t)a;
                return s;
            };
            if (init || (ev & open) != 0ull) {
                fl = init ? OC_BELF_REINIT : OC_BELF_RESET;
                open = init ? fresh : open & ~ev;
                live = open;
                for (int i = 0; i <= S; ++i) b[i] = (live >> i) & 1ull ? 1.0 / (double)__builtin_popcountll(live) : 0.0;
            } else {
                const int t = taken > 4 ? 4 : taken;
                for (int i = 0; i < S; ++i) {
                    if (!((live >> i) & 1ull)) continue;
                    Ops o(L, blob.data());
                    float lb;
                    if (o.full_bound(r, row_of(i), lb)) continue;
                    live &= ~(1ull << i);
                    b[i] = 0.0;
                    fl |= OC_BELF_PRUNED;
                }
                Ops o(L, blob.data());
                Row v = r;
                ocro::Sub sa = row_of(0);
                sa.kind = 1;
                bool raises = o.level0(v, sa);
                bool legal[5] = {};
                for (int k = 0; k < 5 && !raises; ++k) legal[k] = o.single_legal(v, a, k);
                raises = (live & subm) != 0ull && (raises || !legal[t]);
                if (raises) {
                    fl |= OC_BELF_RAISED;
                } else {
                    fl |= OC_BELF_UPDATED;
                    Ops of(L, blob.data());
                    double p0, p1;
                    bool nm;
                    Ops::none_probs(__builtin_popcount(of.none_movable(r, a)), beta, nap, p0, p1, nm);
                    for (int i = 0; i <= S; ++i) {
                        if (!((live >> i) & 1ull)) continue;
                        double l = t == 4 ? p0 : p1;
                        if (i < S && subs[(size_t)i].kind != 0) {
                            const ocro::Sub s = row_of(i);
                            const int count = o.goal_objects(v, s);
                            double q[5], mq = 1.0e300, sum = 0.0;
                            for (int k = 0; k < 5; ++k) {
                                if (!legal[k]) continue;
                                Row n = v;
                                o.interact(n, a, k);
                                const double cost = k != 4 ? 1.0 + 0.1 : 1.0;
                                q[k] = cost + 1.0 * (o.goal_objects(n, s) > count ? 0.0 : (double)o.lower_bound(n, s) * (1.0 + 0.1) - 1.09);
                                mq = q[k] < mq ? q[k] : mq;
                            }
                            for (int k = 0; k < 5; ++k)
                                if (legal[k]) sum += exp(beta * (mq - q[k]));
                            l = exp(beta * (mq - q[t])) / sum;
                        }
                        b[i] = b[i] * l;
                    }
                }
                double total = 0.0;
                for (int i = 0; i <= S; ++i)
                    if ((live >> i) & 1ull) total += b[i];
                for (int i = 0; i <= S; ++i)
                    if ((live >> i) & 1ull) b[i] = total == 0.0 ? 1.0 / (double)__builtin_popcountll(live) : b[i] * (1.0 / total);
            }
            int best = S;
            double bv = -1.0;
            for (int i = 0; i <= S; ++i)
                if (((live >> i) & 1ull) && b[i] > bv) best = i, bv = b[i];
            uint64_t gopen = 0, glive = 0;
            for (int c = 0; c < HP; ++c) {
                gopen |= (uint64_t)se[c * P] << (8 * c);
                glive |= (uint64_t)se[(HP + c) * P] << (8 * c);
            }
            if (gopen != (open & all) || glive != (live & all))
                bad = printf("A%d K%d W%d S%d e%lld m%d: bstate %llx %llx vs %llx %llx\n", A, K, (int)W, S, (long long)e, m,
                             (unsigned long long)gopen, (unsigned long long)glive, (unsigned long long)open,
                             (unsigned long long)live);
            for (int i = 0; i <= S && !bad; ++i) {
                const double d = fabs(be[i * P] - b[i]);
                if (!(d <= 1e-14 * fabs(b[i])))
                    bad = printf("A%d K%d W%d S%d e%lld m%d i%d: belief %.17g vs %.17g\n", A, K, (int)W, S, (long long)e, m, i,
                                 be[i * P], b[i]);
            }
            if (!nulls && (map[m * P + e] != best || info[m * P + e] != fl))
                bad = printf("A%d K%d W%d S%d e%lld m%d: map %d info %d vs %d %d\n", A, K, (int)W, S, (long long)e, m,
                             map[m * P + e], info[m * P + e], best, fl);
        }
    }
    free(bel);
    free(bs);
    free(map);
    free(info);
    return bad != 0;
}

int main() {
    int bad = 0;
    for (int64_t B : {1, 7, 9, 300}) {
        bad |= run<1, 4, false>(B, 9, 1) | run<2, 4, false>(B, 9, 2) | run<3, 4, false>(B, 7, 3) | run<4, 4, false>(B, 8, 4);
        bad |= run<1, 8, false>(B, 15, 1) | run<2, 8, false>(B, 63, 2) | run<3, 8, false>(B, 21, 3) | run<4, 8, false>(B, 16, 2);
        bad |= run<1, 16, false>(B, 9, 1) | run<2, 16, false>(B, 16, 2) | run<3, 16, false>(B, 5, 2) | run<4, 16, false>(B, 31, 4);
        bad |= run<1, 4, true>(B, 3, 1) | run<2, 4, true>(B, 9, 2) | run<3, 4, true>(B, 9, 3) | run<4, 4, true>(B, 11, 2);
        bad |= run<1, 8, true>(B, 8, 1) | run<2, 8, true>(B, 17, 2) | run<3, 8, true>(B, 16, 3) | run<4, 8, true>(B, 9, 4);
        bad |= run<1, 16, true>(B, 7, 1) | run<2, 16, true>(B, 24, 2) | run<3, 16, true>(B, 9, 1) | run<4, 16, true>(B, 12, 1);
    }
    printf(bad ? "FAILED\n" : "belief_asan: all builds, sizes, tables and states clean and equal to the scalar restatement\n");
    return bad;
}
