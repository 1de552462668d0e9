// sl_index.h — the index arithmetic of the int8 predict kernel's K loop (gpb_sliced.hip): where in a GP's digit planes each 1-KB
// piece of a stage comes from and how that place moves from one K-step to the next.
// Functions of plain integers, free of HIP, so that a stand-alone program proves them on the host for every geometry before a
// kernel issues one DMA with them (tests/host/sl_index_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SL_HD __host__ __device__ __forceinline__
#else
#define SL_HD inline
#endif

namespace gpb {

constexpr int SL_IDX_BM = 128;                   // rows of a block tile (SL_BM): two 64-row pieces per (plane, k-block) of L^-1

// piece `ch` of a stage: the A_CHUNKS = D x 2 x 2 pieces of L^-1 first, then the D x 2 x WTN of K*^T; inside an operand the order
// is (plane t, k-block q of the step's two, 64-row piece h)
struct SlChunk {
    bool is_a;
    int t, q, h;
};
SL_HD SlChunk sl_chunk(int ch, int depth, int wtn) {
    constexpr int per_a = SL_IDX_BM / 64;
    const int a_chunks = depth * 2 * per_a;
    // (the operand first, so that each branch divides by a constant where depth and wtn are template arguments)
    if (ch < a_chunks) return SlChunk{true, ch / (2 * per_a), (ch / per_a) & 1, ch % per_a};
    const int cb = ch - a_chunks;
    return SlChunk{false, cb / (2 * wtn), (cb / wtn) & 1, cb % wtn};
}

// Closed form: byte offset, from the start of the GP's planes of that operand, of lane 0's granule of piece c in K-step `step`
// (lane l takes the 16 bytes at + 16 l).  plane = bytes of one plane, ld = rows of a k-block (Np128 for L^-1, Wld for K*^T),
// off = the tile's first row (mb) or walker (nb), kb_first = k_begin / 16.
SL_HD int64_t sl_src_offset(const SlChunk& c, int64_t plane, int64_t ld, int64_t off, int64_t kb_first, int64_t step) {
    return c.t * plane + ((kb_first + 2 * step + c.q) * ld + off + 64 * c.h) * 16;
}

// Incremental form: a K-step is two 16-deep k-blocks, so every piece of an operand moves by the same 32 ld bytes per step
SL_HD int64_t sl_src_stride(int64_t ld) { return 32 * ld; }

}  // namespace gpb
