// TEST INFRASTRUCTURE: the host functions of gym-cooking_amd/csrc/oc_startdist.h (the worker of
// oc_cpu_reset_random) in a stand-alone program for AddressSanitizer / UBSan: every (A, K, narrow /
// wide) build, ragged batch sizes, full and masked mode, lists from the loosest to the tightest
// (exactly A shared agent cells, exactly as many item cells as items), and state buffers that end
// exactly at the last byte the contract allows to be read or written (column B - 1 of the last
// plane).  Also checks every env against a scalar per-env restatement of the draw.  The product
// library never contains this file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline

#include "../../gym-cooking_amd/csrc/oc_startdist.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static uint64_t mix(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the r-th cell of `list` (ascending) that is not in `taken`, by a plain scan
static int nth_free(const std::vector<int>& list, const std::vector<int>& taken, uint64_t base, int d) {
    int m = 0;
    for (int c : list)
        for (int t : taken) m += c == t;
    const uint64_t u = mix(base ^ (0x53540000ull + (uint64_t)d));
    int r = (int)(uint32_t)(((u >> 32) * (uint64_t)(list.size() - (size_t)m)) >> 32);
    for (int c : list) {
        bool is_taken = false;
        for (int t : taken) is_taken |= c == t;
        if (!is_taken && r-- == 0) return c;
    }
    abort();
}

template <int A, int K, bool WIDE>
static int run(int64_t B, int items, bool tight, int what) {
    using PL = ocly::Planes<A, K, WIDE>;
    const int64_t P = (B + 4095) / 4096 * 4096;
    const int W = WIDE ? 31 : 15, H = WIDE ? 33 : 17, cells = W * H;
    // lists: random subsets, or exactly A shared agent cells and exactly `items` item cells
    std::vector<std::vector<int>> LA(A);
    std::vector<int> LI;
    if (tight) {
        for (int c = 0; c < cells && (int)LA[0].size() < A; ++c)
            if (rnd() % 5 == 0 || cells - c <= A) LA[0].push_back(c);
        for (int i = 1; i < A; ++i) LA[i] = LA[0];
        for (int c = 0; c < cells && (int)LI.size() < items; ++c)
            if (rnd() % 5 == 0 || cells - c <= items) LI.push_back(c);
    } else {
        for (int i = 0; i < A; ++i) {
            for (int c = 0; c < cells; ++c)
                if (rnd() % 3 == 0) LA[i].push_back(c);
            while ((int)LA[i].size() < A) LA[i].push_back(cells - A + (int)LA[i].size());  // ascending: past the random ones
        }
        for (int c = 0; c < cells; ++c)
            if (rnd() % 4 == 0 || c >= cells - items) LI.push_back(c);
    }
    for (int i = 0; i < A; ++i) {  // dedupe the padded tails
        std::vector<int> u;
        for (int c : LA[i])
            if (u.empty() || c > u.back()) u.push_back(c);
        LA[i] = u;
        if ((int)LA[i].size() < A) return 0;  // no valid list this time
    }
    ocsd::StartArgs R{};
    R.S = (cells + 1) & ~1;
    R.S2 = (cells + 3) & ~3;
    R.nI = (int)LI.size();
    R.items = items;
    R.what = what;
    R.pitch = P;
    R.B = B;
    R.env_offset = (int64_t)(rnd() & 0xFFFF) << 20;
    R.seed = ((uint64_t)rnd() << 32) | rnd();
    R.round = rnd();
    // the table ends exactly where table_bytes says
    const size_t tb = (size_t)ocsd::table_bytes(A, R.S, R.S2);
    uint8_t* tab = (uint8_t*)malloc(tb);
    memset(tab, 0, tb);
    uint16_t* L = (uint16_t*)tab;
    for (int i = 0; i < A; ++i) {
        R.nA[i] = (int)LA[i].size();
        for (size_t n = 0; n < LA[i].size(); ++n) L[i * R.S + (int)n] = (uint16_t)LA[i][n];
        for (int c : LA[i]) tab[(size_t)(A + 2) * R.S * 2 + (size_t)i * R.S2 + c] = 1;
    }
    for (size_t n = 0; n < LI.size(); ++n) L[A * R.S + (int)n] = (uint16_t)LI[n];
    for (int c = 0; c < cells; ++c) L[(A + 1) * R.S + c] = (uint16_t)((c % W) | ((c / W) << 8));
    ocsw::SwarLevel sw{};
    for (int a = 0; a < 4; ++a) sw.tmpl_x[a] = 0x01010101u * (uint32_t)(a + 1), sw.tmpl_y[a] = 0x01010101u * (uint32_t)(a + 2);
    for (int j = 0; j < 16; ++j) {
        const uint32_t cell = j < items ? (uint32_t)(7 + j) : (WIDE ? 0xFFFFu : 0xFFu);
        sw.tmpl_l[j] = 0x01010101u * (cell & 0xFFu);
        sw.tmpl_lh[j] = 0x01010101u * (cell >> 8);
        sw.tmpl_m[j] = j < items ? 0x01010101u * (uint32_t)(j + 1) : 0u;
    }
    // buffers end at env B - 1's byte of the last plane (the flags): one byte more is a heap overflow
    const size_t nbytes = (size_t)((int64_t)(PL::NP - 1) * P + B);
    int bad = 0;
    for (int masked = 0; masked < 2 && !bad; ++masked) {
        uint8_t* s = (uint8_t*)malloc(nbytes);
        uint8_t* prev = (uint8_t*)malloc(nbytes);
        for (size_t i = 0; i < nbytes; ++i) s[i] = (uint8_t)rnd(), prev[i] = (uint8_t)rnd();
        std::vector<uint8_t> before(s, s + nbytes);
        R.masked = masked;
        ocsd::host_start_range<A, K, WIDE>(sw, R, tab, s, masked ? prev : nullptr, 0, (B + 3) / 4);
        // the scalar restatement, env by env, into a copy of the old bytes
        std::vector<uint8_t> want(before);
        for (int64_t e = 0; e < B; ++e) {
            if (masked && !(prev[PL::F * P + e] & OC_FLAG_DONE)) continue;
            const uint64_t gid = (uint64_t)(R.env_offset + e);
            const uint64_t base = R.seed ^ (gid * 0x9E3779B97F4A7C15ull) ^ (R.round * 0xC2B2AE3D27D4EB4Full);
            std::vector<int> taken;
            for (int i = 0; i < A; ++i) {
                int x = i + 1, y = i + 2;
                if (what & OC_START_AGENTS) {
                    const int c = nth_free(LA[i], taken, base, i);
                    taken.push_back(c);
                    x = c % W, y = c / W;
                }
                want[(PL::X + i) * P + e] = (uint8_t)x;
                want[(PL::Y + i) * P + e] = (uint8_t)y;
                want[(PL::HOLD + i) * P + e] = OC_HOLD_NONE;
            }
            taken.clear();
            for (int k = 0; k < K; ++k) {
                int c = k < items ? 7 + k : (WIDE ? 0xFFFF : 0xFF);
                if (k < items && (what & OC_START_ITEMS)) {
                    c = nth_free(LI, taken, base, 16 + k);
                    taken.push_back(c);
                }
                want[(PL::LOC + k) * P + e] = (uint8_t)c;
                if (WIDE) want[(PL::LOC_HI + k) * P + e] = (uint8_t)(c >> 8);
                want[(PL::MASK + k) * P + e] = k < items ? (uint8_t)(k + 1) : 0;
            }
            want[PL::T * P + 2 * e] = want[PL::T * P + 2 * e + 1] = 0;
            want[PL::F * P + e] = 0;
        }
        for (size_t i = 0; i < nbytes && !bad; ++i)
            if (s[i] != want[i]) {
                printf("A%d K%d wide%d B%lld items%d tight%d what%d masked%d: plane %lld column %lld: %d vs %d\n", A, K,
                       (int)WIDE, (long long)B, items, (int)tight, what, masked, (long long)(i / P), (long long)(i % P),
                       s[i], want[i]);
                bad = 1;
            }
        free(s);
        free(prev);
    }
    free(tab);
    return bad;
}

template <int K, bool WIDE>
static int run_agents(int64_t B, int items, bool tight, int what) {
    return run<1, K, WIDE>(B, items, tight, what) | run<2, K, WIDE>(B, items, tight, what) |
           run<3, K, WIDE>(B, items, tight, what) | run<4, K, WIDE>(B, items, tight, what);
}

int main() {
    int bad = 0;
    const int64_t sizes[] = {1, 2, 3, 5, 63, 4097};  // every B % 4, one and two pitches
    for (int64_t B : sizes)
        for (int tight = 0; tight < 2; ++tight)
            for (int what = 1; what <= 3; ++what) {
                bad |= run_agents<4, false>(B, 3, tight, what) | run_agents<8, false>(B, 8, tight, what) |
                       run_agents<16, false>(B, 16, tight, what) | run_agents<16, false>(B, 9, tight, what);
                bad |= run_agents<4, true>(B, 4, tight, what) | run_agents<8, true>(B, 5, tight, what) |
                       run_agents<16, true>(B, 16, tight, what);
            }
    printf(bad ? "FAILED\n" : "start_asan: all builds, sizes, modes and lists clean and equal to the scalar restatement\n");
    return bad;
}
