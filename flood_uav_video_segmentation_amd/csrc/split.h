// The split-operand arithmetic, defined once: every fp32 operand x is the exact sum h + m + l of three bf16 terms,
//   h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), each rounded to nearest even (v_cvt_pk_bf16_f32); the residues are exact fp32
// subtractions, and 3 x 8 significant bits with signed residues cover the 24 of fp32.  Exact for every finite |x| <= 3.3895e38 (the
// largest bf16; nothing above 2^-110 is flushed).  Of the nine cross products of two split operands the six of order <= 2^-16 go to
// the bf16 matrix cores (exact products, fp32 accumulation) -- v_mfma_f32_16x16x32_bf16 in the implicit GEMM (conv_igemm.hip: the shape
// that costs the fewest joules per FLOP, profiles/r33_mfma_shape.txt), v_mfma_f32_32x32x16_bf16 in the stem and attention kernels; the
// operand registers are the same for both shapes (eight bf16 of consecutive k per lane):
//   x * w = h h' + (h m' + m h') + (m m' + h l' + l h') + [m l' + l m' + l l' <= 2^-23 |x w|, dropped: below the rounding of one fp32 add]
// +-inf, NaN and finite values beyond the largest bf16: include/floodseg_test.h (fs_test_api::split_bf16x3).
#pragma once
#include "common.h"

namespace fs {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// One level on a pair, in its two halves (conv_igemm.hip pins the packed pair to an MFMA slot between them): the packed bf16 pair
// {x0's term, x1's term}, then x0, x1 -> their residues.
__device__ __forceinline__ unsigned split_round(float x0, float x1) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){x0, x1}, bf16x2));
}
__device__ __forceinline__ void split_residue(unsigned pk, float& x0, float& x1) {
    x0 -= __builtin_bit_cast(float, pk << 16);
    x1 -= __builtin_bit_cast(float, pk & 0xffff0000u);
}
__device__ __forceinline__ unsigned split_level(float& x0, float& x1) {
    const unsigned pk = split_round(x0, x1);
    split_residue(pk, x0, x1);
    return pk;
}

// (x0, x1) -> the three terms of each, packed {x0's term, x1's term}
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = split_level(x0, x1);
    m = split_level(x0, x1);
    l = split_round(x0, x1);
}

// eight values -> t[term] = the term's eight bf16, packed in the values' order (one operand of a 32x32x16 or 16x16x32 bf16 MFMA per term)
__device__ __forceinline__ void split8(const float (&x)[8], u32x4 (&t)[3]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        unsigned h, m, l;
        split_pair(x[2 * e], x[2 * e + 1], h, m, l);
        t[0][e] = h; t[1][e] = m; t[2][e] = l;
    }
}

// one value -> its three terms (the low half of its pair)
__device__ __forceinline__ void split3(float x, unsigned short& h, unsigned short& m, unsigned short& l) {
    unsigned ph, pm, pl;
    split_pair(x, 0.f, ph, pm, pl);
    h = (unsigned short)ph; m = (unsigned short)pm; l = (unsigned short)pl;
}

// The six products as (term of the first operand, term of the second), smallest first so that the small ones are not lost against
// an accumulator that already holds the large one: l h', h l', m m', m h', h m', h h'.
constexpr int SPLIT_PA[6] = {2, 0, 1, 1, 0, 0}, SPLIT_PB[6] = {0, 2, 1, 0, 1, 0};

// 32x32 accumulator of v_mfma_f32_32x32x*: lane (l & 31, h = l >> 5) holds column l & 31; its register e is this row.
__host__ __device__ constexpr int mfma32_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// 16x16 accumulator of v_mfma_f32_16x16x32_bf16 (the implicit GEMM's split loop): lane (n = l & 15, q = l >> 4) holds column n and, in
// register e, the row whose pixels operand lane r = 4 q + e supplied.  conv_igemm.hip gives lane r tile row mfma16_row(r) of the 16-row
// half (bits 2 and 3 of r exchanged): one v_permlane16_swap per register pair then turns two 16-column blocks into the 32x32 layout above.
__host__ __device__ constexpr int mfma16_row(int r) { return (r & 3) | ((r & 4) << 1) | ((r & 8) >> 1); }

// LDS swizzle keys of that loop's fragment reads (one ds_read_b128 = 16 rows x 4 k-blocks): a 128-B pixel row keeps its logical 16-B
// piece c in slot c ^ split_row_key(row), a 64-B filter-plane row its piece c in slot c ^ split_plane_key(row)
// ({0,0,1,1,0,0,1,1,6,6,7,7,6,6,7,7}[row & 15] and {0,2,3,1}[(row >> 2) & 3]: profiles/r04_experiments.txt section 7).
__host__ __device__ constexpr int split_row_key(int row) { return ((row >> 1) & 1) | ((row & 8) ? 6 : 0); }
__host__ __device__ constexpr int split_plane_key(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }

}  // namespace fs
