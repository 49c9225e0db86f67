// TEST INFRASTRUCTURE: the host step worker of gym-cooking_amd/csrc/oc_stepio.h (oc_cpu_step's
// range function, with the chunk load / store walk and the class lookups it shares with the kernels)
// in a stand-alone program for AddressSanitizer / UBSan.  One narrow and one wide level, every
// agent count, contract-sized buffers (num_planes * pitch bytes, B = 7: one full and one ragged
// word), a few steps with fixed actions; each step is compared with ocsw::step4 / step4w called
// directly on words assembled byte by byte here.  The product library never contains this file.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline

#include "../../gym-cooking_amd/csrc/oc_stepio.h"

static const int64_t B = 7, P = 4096;
static const int STEPS = 4;

struct Level {
    int W, H, done;
    std::vector<uint8_t> tiles;
    uint16_t cell[16];
    uint8_t mask[16], sx[4], sy[4];
};

// Counters on the border (a Delivery and a Cutboard on the left wall), Floor inside, three items
// on the border: a tomato, a lettuce (past cell 255 on the wide level) and a plate.
static Level make_level(int W, int H) {
    Level lv;
    lv.W = W;
    lv.H = H;
    lv.tiles.assign((size_t)W * H, OC_TILE_FLOOR);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (x == 0 || y == 0 || x == W - 1 || y == H - 1) lv.tiles[(size_t)y * W + x] = OC_TILE_COUNTER;
    lv.tiles[(size_t)2 * W] = OC_TILE_DELIVERY;
    lv.tiles[(size_t)3 * W] = OC_TILE_CUTBOARD;
    lv.done = 2 * W;
    for (int j = 0; j < 16; ++j) {
        lv.cell[j] = W * H > 255 ? (uint16_t)OC_LOC_DEAD16 : (uint16_t)OC_LOC_DEAD;
        lv.mask[j] = 0;
    }
    lv.cell[0] = 2;                                // top wall, next to the first spawn
    lv.cell[1] = (uint16_t)((H - 2) * W + W - 1);  // right wall, last inner row
    lv.cell[2] = (uint16_t)((H - 1) * W + 3);      // bottom wall
    lv.mask[0] = 1;
    lv.mask[1] = 2;
    lv.mask[2] = 8;
    for (int a = 0; a < 4; ++a) {
        lv.sx[a] = (uint8_t)(1 + a);
        lv.sy[a] = 1;
    }
    return lv;
}

static uint8_t action(int step, int a, int64_t e) { return (uint8_t)((step * 3 + a * 2 + e) % 5); }

// plane word g assembled from its bytes
static uint32_t word(const std::vector<uint8_t>& s, int plane, int64_t g) {
    uint32_t v = 0;
    for (int q = 0; q < 4; ++q) v |= (uint32_t)s[(size_t)(plane * P + 4 * g + q)] << (8 * q);
    return v;
}
static uint32_t tword(const std::vector<uint8_t>& s, int plane, int64_t g, int half) {
    uint32_t v = 0;
    for (int q = 0; q < 4; ++q) v |= (uint32_t)s[(size_t)(plane * P + 8 * g + 4 * half + q)] << (8 * q);
    return v;
}

template <int A, int K, bool WIDE, int MODE>
static int run(const Level& lv) {
    using PL = ocly::Planes<A, K, WIDE>;
    ocsw::SwarLevel sw;
    uint8_t goal[1] = {0x3B}, cell8[16];
    for (int j = 0; j < 16; ++j) cell8[j] = (uint8_t)lv.cell[j];
    ocsw::build_swar_level(sw, lv.W, lv.H, lv.done, goal, 1, 3, lv.sx, lv.sy, A, cell8, lv.mask, 0, lv.tiles.data());
    if (WIDE) {  // as oc_create: u16 cells as low / high byte words
        sw.done_rep = (uint32_t)(lv.done & 0xFF) * 0x01010101u;
        sw.done_hi_rep = (uint32_t)(lv.done >> 8) * 0x01010101u;
        for (int j = 0; j < 16; ++j) {
            sw.tmpl_l[j] = (uint32_t)(lv.cell[j] & 0xFF) * 0x01010101u;
            sw.tmpl_lh[j] = (uint32_t)(lv.cell[j] >> 8) * 0x01010101u;
        }
    }
    std::vector<uint8_t> cls(1024, 0);
    for (size_t c = 0; c < lv.tiles.size(); ++c) cls[c] = ocsw::tile_class(lv.tiles[c]);
    [[maybe_unused]] auto narrow_cls = [&cls](uint32_t c) {
        uint32_t r = 0;
        for (int q = 0; q < 4; ++q) r |= (uint32_t)cls[(c >> (8 * q)) & 0xFFu] << (8 * q);
        return r;
    };
    [[maybe_unused]] auto wide_cls = [&cls](const ocsw::Cell2& c) {
        uint32_t r = 0;
        for (int q = 0; q < 4; ++q)
            r |= (uint32_t)cls[((((c.hi >> (8 * q)) & 0xFFu) << 8) | ((c.lo >> (8 * q)) & 0xFFu)) & 0x3FFu] << (8 * q);
        return r;
    };

    // the reset state through the shared store walk, whole words
    std::vector<uint8_t> s((size_t)PL::NP * P, 0xEE), nxt((size_t)PL::NP * P), act((size_t)A * P, 0), ex((size_t)A * P),
        coll((size_t)P);
    for (int64_t g = 0; g < 2; ++g) ocio::store(ocio::template_chunk<A, K, WIDE>(sw), ocio::HostWords{s.data(), P, g});
    int bad = 0;
    uint64_t totals[OC_NSTATS] = {}, want_eps = 0;
    for (int step = 0; step < STEPS; ++step) {
        for (int a = 0; a < A; ++a)
            for (int64_t e = 0; e < 8; ++e) act[(size_t)(a * P + e)] = action(step, a, e);
        std::fill(nxt.begin(), nxt.end(), 0xA5);
        std::fill(ex.begin(), ex.end(), 0xA5);
        std::fill(coll.begin(), coll.end(), 0xA5);
        uint64_t st[OC_NSTATS];
        if constexpr (WIDE)
            ocio::host_step_range<MODE, A, K, true>(sw, ocio::WideClass{cls.data()}, s.data(), nxt.data(), act.data(),
                                                    ex.data(), coll.data(), B, P, 0, 2, st);
        else
            ocio::host_step_range<MODE, A, K, false>(sw, ocio::NarrowClass{cls.data()}, s.data(), nxt.data(), act.data(),
                                                     ex.data(), coll.data(), B, P, 0, 2, st);
        for (int c = 0; c < OC_NSTATS; ++c) totals[c] += st[c];
        for (int64_t g = 0; g < 2; ++g) {  // the same step on hand-loaded words
            uint32_t X[A], Y[A], H[A], LL[K], LH[K], M[K], AC[A], EX[A], CM, T0, T1, F, pending;
            for (int a = 0; a < A; ++a) {
                X[a] = word(s, PL::X + a, g);
                Y[a] = word(s, PL::Y + a, g);
                H[a] = word(s, PL::HOLD + a, g);
                AC[a] = word(act, a, g);
            }
            for (int j = 0; j < K; ++j) {
                LL[j] = word(s, PL::LOC + j, g);
                LH[j] = WIDE ? word(s, PL::LOC_HI + j, g) : 0u;
                M[j] = word(s, PL::MASK + j, g);
            }
            T0 = tword(s, PL::T, g, 0);
            T1 = tword(s, PL::T, g, 1);
            F = word(s, PL::F, g);
            const uint32_t f_in = F;
            auto any = [](uint32_t v) { return v != 0u; };
            if constexpr (WIDE) {
                pending = ocsw::at_done80w<K>(sw, LL, LH);
                ocsw::step4w<A, K>(sw, X, Y, H, LL, LH, M, T0, T1, F, AC, EX, CM, wide_cls, any, pending);
            } else {
                pending = ocsw::at_done80<K, MODE>(sw, LL);
                ocsw::step4<A, K, MODE>(sw, X, Y, H, LL, M, T0, T1, F, AC, EX, CM, narrow_cls, any, pending);
            }
            const int ncol = g == 0 ? 4 : 3;  // B = 7
            auto chk = [&](const std::vector<uint8_t>& buf, int plane, uint32_t want, const char* what) {
                for (int q = 0; q < 4; ++q) {
                    const uint8_t got = buf[(size_t)(plane * P + 4 * g + q)];
                    const bool written = q < ncol || !WIDE;  // a narrow level writes whole words
                    const uint8_t w = written ? (uint8_t)(want >> (8 * q)) : (uint8_t)0xA5;
                    if (got != w) {
                        printf("A=%d K=%d wide=%d mode=%d step %d word %d %s plane %d col %d: got %02x want %02x\n", A, K,
                               (int)WIDE, MODE, step, (int)g, what, plane, q, got, w);
                        ++bad;
                    }
                }
            };
            for (int a = 0; a < A; ++a) {
                chk(nxt, PL::X + a, X[a], "x");
                chk(nxt, PL::Y + a, Y[a], "y");
                chk(nxt, PL::HOLD + a, H[a], "hold");
                chk(ex, a, EX[a], "exec");
            }
            for (int j = 0; j < K; ++j) {
                chk(nxt, PL::LOC + j, LL[j], "loc");
                if (WIDE) chk(nxt, PL::LOC_HI + j, LH[j], "loc_hi");
                chk(nxt, PL::MASK + j, M[j], "mask");
            }
            chk(nxt, PL::F, F, "flags");
            chk(coll, 0, CM, "coll");
            for (int q = 0; q < 8; ++q) {  // the u16 step counts: two bytes per env
                const uint8_t got = nxt[(size_t)(PL::T * P + 8 * g + q)];
                const bool written = q < 2 * ncol || !WIDE;
                const uint8_t w = written ? (uint8_t)((q < 4 ? T0 : T1) >> (8 * (q & 3))) : (uint8_t)0xA5;
                if (got != w) {
                    printf("A=%d K=%d wide=%d step %d word %d t byte %d: got %02x want %02x\n", A, K, (int)WIDE, step, (int)g,
                           q, got, w);
                    ++bad;
                }
            }
            for (int q = 0; q < ncol; ++q) want_eps += ((F & ~f_in) >> (8 * q)) & 1u;
        }
        // nothing past the second word
        for (int p = 0; p < PL::NP - 3; ++p)
            if (nxt[(size_t)(p * P + 8)] != 0xA5) ++bad;
        s.swap(nxt);
    }
    if (totals[OC_STAT_EPISODES] != want_eps || want_eps == 0) {  // max_T = 3: every env times out once
        printf("A=%d K=%d wide=%d: episodes %llu, want %llu (> 0)\n", A, K, (int)WIDE,
               (unsigned long long)totals[OC_STAT_EPISODES], (unsigned long long)want_eps);
        ++bad;
    }
    return bad;
}

template <bool WIDE>
static int run_all(const Level& lv) {
    int bad = 0;
    bad += run<1, 4, WIDE, 1>(lv) + run<2, 4, WIDE, 1>(lv) + run<3, 4, WIDE, 1>(lv) + run<4, 4, WIDE, 1>(lv);
    bad += run<2, 8, WIDE, 1>(lv) + run<3, 16, WIDE, 1>(lv);
    if (!WIDE) bad += run<2, 4, false, 0>(lv) + run<3, 4, false, 0>(lv);  // the common-class build
    return bad;
}

int main() {
    const int bad = run_all<false>(make_level(8, 7)) + run_all<true>(make_level(24, 12));
    printf(bad ? "FAILED\n" : "stepio_asan: narrow and wide step ranges clean and equal to step4 / step4w on hand-loaded words\n");
    return bad ? 1 : 0;
}
