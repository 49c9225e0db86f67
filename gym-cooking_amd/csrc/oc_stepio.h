// oc_stepio.h -- the step family's chunk: one lane's (or one host word's) four envs of a state, its
// load and store walk over the planes of oc_layout.h, the episode tally, the tile-class lookups and
// the host step worker, each defined once for oc_reset_kernel and oc_cpu_step.
// The three step kernels use only the Chunk and StepStats types from here and keep their own walks,
// tally, descriptors and flush in oc_engine.hip, which says why; they follow the same plane order.
//
// Plain host and device C++ over oc_swar.h (the includer provides __host__ / __device__ /
// __forceinline__): a walk reads and writes plane words through an accessor,
//   ld32(plane) / ld64(plane, lo, hi) / st32(plane, v) / st64(plane, lo, hi),
// which on the device is a global pointer (the reset, oc_engine.hip GlobalWords), and on the host
// HostWords below.
#ifndef OC_STEPIO_H_
#define OC_STEPIO_H_

#include <cstdint>
#include <cstring>

#include "../../include/oc_engine.h"
#include "oc_layout.h"
#include "oc_swar.h"

namespace ocio {

using ocly::Planes;

constexpr int kEPL = 4;  // envs per chunk: one dword per byte plane

// kEPL consecutive envs, one dword per byte plane: the agents' x, y, held slot and action, the item
// slots' cell (low byte; wlh the high byte, wide levels only) and mask, the four u16 step counts
// (t0: envs 0 and 1, t1: envs 2 and 3) and the flags.
template <int A, int K, bool WIDE = false>
struct Chunk {
    uint32_t wx[A], wy[A], wh[A], wa[A], wl[K], wlh[WIDE ? K : 1], wm[K];
    uint32_t t0, t1, wf;
};

// The chunk walk, in plane order: X, Y, HOLD per agent; LOC, [LOC_HI], MASK per slot; the 8-byte T
// word; F.  load() also takes agent a's action word from plane a of `acts` (kActs false: not read).
template <bool kActs = true, int A, int K, bool WIDE, class In>
OC_SW void load(Chunk<A, K, WIDE>& c, const In& s, const In& acts) {
    using PL = Planes<A, K, WIDE>;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        c.wx[a] = s.ld32(PL::X + a);
        c.wy[a] = s.ld32(PL::Y + a);
        c.wh[a] = s.ld32(PL::HOLD + a);
        if (kActs) c.wa[a] = acts.ld32(a);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        c.wl[j] = s.ld32(PL::LOC + j);
        if constexpr (WIDE) c.wlh[j] = s.ld32(PL::LOC_HI + j);
        c.wm[j] = s.ld32(PL::MASK + j);
    }
    s.ld64(PL::T, c.t0, c.t1);
    c.wf = s.ld32(PL::F);
}

template <int A, int K, bool WIDE, class Out>
OC_SW void store(const Chunk<A, K, WIDE>& c, const Out& d) {
    using PL = Planes<A, K, WIDE>;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        d.st32(PL::X + a, c.wx[a]);
        d.st32(PL::Y + a, c.wy[a]);
        d.st32(PL::HOLD + a, c.wh[a]);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        d.st32(PL::LOC + j, c.wl[j]);
        if constexpr (WIDE) d.st32(PL::LOC_HI + j, c.wlh[j]);
        d.st32(PL::MASK + j, c.wm[j]);
    }
    d.st64(PL::T, c.t0, c.t1);
    d.st32(PL::F, c.wf);
}

// The level's reset template as a chunk (SwarLevel holds it replicated per byte).
template <int A, int K, bool WIDE>
OC_SW Chunk<A, K, WIDE> template_chunk(const ocsw::SwarLevel& sw) {
    Chunk<A, K, WIDE> c;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        c.wx[a] = sw.tmpl_x[a];
        c.wy[a] = sw.tmpl_y[a];
        c.wh[a] = (uint32_t)OC_HOLD_NONE * ocsw::k01;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        c.wl[j] = sw.tmpl_l[j];
        if constexpr (WIDE) c.wlh[j] = sw.tmpl_lh[j];
        c.wm[j] = sw.tmpl_m[j];
    }
    c.t0 = c.t1 = c.wf = 0u;
    return c;
}

// Tile class byte per env of a word of cell ids.  Narrow: a 256-byte table (cells past the grid
// read 0).  Wide: the cell is hi << 8 | lo, the table has 1,024 entries.
struct NarrowClass {
    const uint8_t* tbl;
    OC_SW uint32_t operator()(uint32_t cells) const {
        const uint32_t b0 = tbl[cells & 0xFFu], b1 = tbl[(cells >> 8) & 0xFFu], b2 = tbl[(cells >> 16) & 0xFFu],
                       b3 = tbl[cells >> 24];
        return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    }
};
struct WideClass {
    const uint8_t* tbl;
    OC_SW uint32_t operator()(const ocsw::Cell2& c) const {
        uint32_t r = 0u;
#pragma unroll
        for (int q = 0; q < kEPL; ++q) {
            const uint32_t idx = ocsw::perm(c.hi >> (8 * q), c.lo >> (8 * q), 0x0C0C0400u) & 0x3FFu;
            r |= (uint32_t)tbl[idx] << (8 * q);
        }
        return r;
    }
};

// One step of the chunk's envs: ocsw::step4<A, K, MODE> (cls_of a NarrowClass) or ocsw::step4w<A, K>
// (a WideClass).  at_done() is the `pending` a freshly loaded chunk starts with.
template <int MODE, int A, int K, bool WIDE>
OC_SW uint32_t at_done(const ocsw::SwarLevel& sw, const Chunk<A, K, WIDE>& c) {
    if constexpr (WIDE) return ocsw::at_done80w<K>(sw, c.wl, c.wlh);
    else return ocsw::at_done80<K, MODE>(sw, c.wl);
}
template <int MODE, int A, int K, bool WIDE, class ClassOf, class AnyOf>
OC_SW bool step(const ocsw::SwarLevel& sw, Chunk<A, K, WIDE>& c, const uint32_t (&act)[A], uint32_t (&ex)[A],
                uint32_t& cm, ClassOf cls_of, AnyOf any_of, uint32_t& pending) {
    if constexpr (WIDE)
        return ocsw::step4w<A, K>(sw, c.wx, c.wy, c.wh, c.wl, c.wlh, c.wm, c.t0, c.t1, c.wf, act, ex, cm, cls_of,
                                  any_of, pending);
    else
        return ocsw::step4<A, K, MODE>(sw, c.wx, c.wy, c.wh, c.wl, c.wm, c.t0, c.t1, c.wf, act, ex, cm, cls_of,
                                       any_of, pending);
}

// Byte mask of chunk g's envs below B: they count in the statistics.
OC_SW uint32_t valid_mask(int64_t B, int64_t g) {
    const int64_t rem = B - g * kEPL;
    return rem >= kEPL ? 0xFFFFFFFFu : (rem <= 0 ? 0u : (1u << (8 * (uint32_t)rem)) - 1u);
}

// Episode counters of the chunks a lane (or a host word) has stepped.
struct StepStats {
    uint32_t eps = 0u, succ = 0u, err = 0u, coll = 0u, steps = 0u;
    // One stepped chunk: `full` as returned by step(), the flags before and after, the step counts
    // and the collision mask after.  An episode ended iff DONE is newly set, which happens only on
    // the full path: without a rare event no flag is set.
    OC_SW void add(bool full, uint32_t f_in, uint32_t F, uint32_t T0, uint32_t T1, uint32_t cm, uint32_t vmask) {
        coll += (uint32_t)__builtin_popcount(cm & vmask);
        if (full) {
            const uint32_t ended = (F & ~f_in & vmask) & ocsw::k01;  // bit0 per env
            eps += (uint32_t)__builtin_popcount(ended);
            succ += (uint32_t)__builtin_popcount(F & (ended << 1));
            err += (uint32_t)__builtin_popcount(F & (ended << 2));
            const uint32_t efull = (0x80808080u - ended) ^ 0x80808080u;  // 0x01 -> 0xFF per byte, no multiply
            const uint32_t e16a = ocsw::perm(0u, efull, 0x01010000u);  // env 0,1 -> u16 masks
            const uint32_t e16b = ocsw::perm(0u, efull, 0x03030202u);  // env 2,3
            const uint32_t sa = T0 & e16a, sb = T1 & e16b;
            steps += (sa & 0xFFFFu) + (sa >> 16) + (sb & 0xFFFFu) + (sb >> 16);
        }
    }
};

// ---- host ------------------------------------------------------------------------------------

// Plane word g of host planes of pitch P.  Loads read whole words; stores write the word's first
// ncol columns (kEPL: the whole word).
struct HostWords {
    uint8_t* p;
    int64_t P, g;
    int ncol = kEPL;
    uint32_t ld32(int plane) const {
        uint32_t v;
        memcpy(&v, p + plane * P + 4 * g, 4);
        return v;
    }
    void ld64(int plane, uint32_t& lo, uint32_t& hi) const {
        memcpy(&lo, p + plane * P + 8 * g, 4);
        memcpy(&hi, p + plane * P + 8 * g + 4, 4);
    }
    void st32(int plane, uint32_t v) const { memcpy(p + plane * P + 4 * g, &v, (size_t)ncol); }
    void st64(int plane, uint32_t lo, uint32_t hi) const {
        const uint32_t t[2] = {lo, hi};
        memcpy(p + plane * P + 8 * g, t, (size_t)(2 * ncol));
    }
};

// oc_cpu_step's worker: words [g0, g1) of the batch (4 envs each, as one lane of the kernels)
// through the host pass of the same step, per-word rare-event split; the range's statistics row
// goes to st.  On the batch's last word a wide level writes only the columns below B (a host
// caller's buffer may be exactly B bytes per plane past the pitch's start); a narrow level writes
// whole words.
template <int MODE, int A, int K, bool WIDE, class ClassOf>
void host_step_range(const ocsw::SwarLevel& sw, ClassOf cls_of, const uint8_t* sin, uint8_t* sout, const uint8_t* act,
                     uint8_t* exo, uint8_t* coll, int64_t B, int64_t P, int64_t g0, int64_t g1, uint64_t* st) {
    uint64_t tot[OC_NSTATS] = {};
    for (int64_t g = g0; g < g1; ++g) {
        Chunk<A, K, WIDE> c;
        load(c, HostWords{const_cast<uint8_t*>(sin), P, g}, HostWords{const_cast<uint8_t*>(act), P, g});
        uint32_t ex[A], cm;
        const uint32_t f_in = c.wf;
        uint32_t pending = at_done<MODE>(sw, c);
        const bool full = step<MODE>(sw, c, c.wa, ex, cm, cls_of, [](uint32_t v) { return v != 0u; }, pending);
        StepStats w;
        w.add(full, f_in, c.wf, c.t0, c.t1, cm, valid_mask(B, g));
        tot[OC_STAT_EPISODES] += w.eps;
        tot[OC_STAT_SUCCESSES] += w.succ;
        tot[OC_STAT_STEPS] += w.steps;
        tot[OC_STAT_COLLISIONS] += w.coll;
        tot[OC_STAT_ERRORS] += w.err;
        const int64_t rem = B - g * kEPL;
        const int ncol = WIDE && rem < kEPL ? (int)rem : kEPL;
        store(c, HostWords{sout, P, g, ncol});
        if (exo != nullptr) {
            for (int a = 0; a < A; ++a) HostWords{exo, P, g, ncol}.st32(a, ex[a]);
        }
        if (coll != nullptr) HostWords{coll, P, g, ncol}.st32(0, cm);
    }
    memcpy(st, tot, sizeof tot);
}

}  // namespace ocio

#endif  // OC_STEPIO_H_
