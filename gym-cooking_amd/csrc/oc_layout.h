// oc_layout.h -- the state's byte-plane layout (oc_layout, include/oc_engine.h), defined once.
//
// A state is NP planes of `pitch` bytes, one byte per env and plane:
//   X, Y, HOLD   A planes each: agent a's x, y and held slot
//   LOC          K planes: item slot j's cell (low byte)
//   LOC_HI       K planes, wide levels (u16 cell ids) only: the cells' high bytes; -1 on a narrow level
//   MASK         K planes: item slot j's content mask
//   T            2 planes: the u16 step counter
//   F            1 plane: the flags
// Plain C++ (constexpr only, no HIP attribute): kernels, the host side and the stand-alone host
// test programs all read the layout from here.
#ifndef OC_LAYOUT_H_
#define OC_LAYOUT_H_

namespace ocly {

// Plane indices of an (A agents, K item slots, narrow / wide) state, named after oc_layout's fields.
struct Layout {
    int X, Y, HOLD, LOC, LOC_HI, MASK, T, F, NP;
};

constexpr Layout layout(int A, int K, bool wide) {
    const int loc = 3 * A, mask = loc + (wide ? 2 : 1) * K, t = mask + K;
    return Layout{0, A, 2 * A, loc, wide ? loc + K : -1, mask, t, t + 2, t + 3};
}

constexpr int num_planes(int A, int K, bool wide) { return layout(A, K, wide).NP; }

// The same indices as compile-time constants.
template <int A, int K, bool WIDE>
struct Planes {
    static constexpr int X = layout(A, K, WIDE).X, Y = layout(A, K, WIDE).Y, HOLD = layout(A, K, WIDE).HOLD;
    static constexpr int LOC = layout(A, K, WIDE).LOC, LOC_HI = layout(A, K, WIDE).LOC_HI;
    static constexpr int MASK = layout(A, K, WIDE).MASK, T = layout(A, K, WIDE).T, F = layout(A, K, WIDE).F;
    static constexpr int NP = layout(A, K, WIDE).NP;
};

static_assert(Planes<2, 4, false>::NP == 17 && Planes<2, 4, false>::MASK == 10 && Planes<2, 4, false>::F == 16,
              "narrow layout: 3A + 2K + 3 planes");
static_assert(Planes<3, 8, true>::NP == num_planes(3, 8, true) && Planes<3, 8, true>::NP == 36 &&
                  Planes<3, 8, true>::LOC_HI == 17 && Planes<3, 8, true>::MASK == 25,
              "wide layout: 3A + 3K + 3 planes");

}  // namespace ocly

#endif  // OC_LAYOUT_H_
