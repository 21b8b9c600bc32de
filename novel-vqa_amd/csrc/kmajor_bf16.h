// kmajor_bf16.h -- what the kernels that feed v_mfma_f32_16x16x32_bf16 from K-MAJOR operands share: k_wgrad_bf16
// (wgrad_bf16.h), k_wgrad_split (wgrad_split.h), k_wgrad_split2 (wgrad_split2.h) and k_dx0_split (dx0_split.h).  Each piece
// has its ONE definition here; the kernel headers keep what is theirs: tile, pipeline, schedule.
//
// ROUNDING.  f32 -> bf16 is round-to-nearest-even (v_cvt_pk_bf16_f32), four values at a time: wb_pack().  wb_widen() is its
// exact reverse (a bf16 value is the high half of an f32).
//
// THE THREE-WAY SPLIT.  An f32 value is exactly the sum of three bf16 values (3 x 8 significand bits):
//     hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid),      the subtractions exact in f32
// (wb_split4(): four values, packed pieces; wb_split1(): one value -- the same three values).  A product a b is then the sum
// of nine bf16 x bf16 products, each exact in f32; mid lo, lo mid and lo lo lie at or below 2^-24 of the product -- under
// what one f32 rounding of the product loses anyway -- and are dropped.  The other six go into the SAME f32 accumulator,
// smallest first, in the order of WB_TERM_A / WB_TERM_B:
//     lo hi, mid mid, hi lo, mid hi, hi mid, hi hi                     (piece of the A operand x piece of the B operand)
// The order is part of the six-term kernels' definition (bit-reproducible results).  Six MFMAs of K = 32 take 96 matrix-pipe
// cycles where v_mfma_f32_16x16x4_f32 needs 256 for the same K.
// Non-finite operands: x = +-inf or NaN gives NaN pieces, so a non-finite operand still gives a non-finite result (NaN where
// an f32 chain may have said inf); |x| >= 2^127 can round hi to inf.  Neither occurs in a step that is not already lost.
//
// THE K-MAJOR IMAGE AND ITS FRAGMENTS.  With the reduction index the slow one in memory, a lane's MFMA fragment (8
// consecutive k of one column) is a COLUMN of the tile.  The weight-gradient kernels keep [k][128 columns] bf16 images in
// LDS, 256-byte rows, the 16-byte chunk ch of row k at wb_off(k, ch) = 256 k + 16 (ch ^ (((k & 3) << 2) | ((k >> 2) & 3)))
// (layout (b) of cdna_hip_programming.md T10: conflict-free for the reads below), and take fragments out of them with
// ds_read_b64_tr_b16, the hardware transpose read.  One such read covers a 4 (k) x 16 (columns) block per 16-lane group:
// lane 4q + p of the group supplies the address of row q, columns 4p .. 4p+3 and receives column (4q + p) of the 4 rows.
// Lane (li, lh) of the MFMA needs k = 8 lh + j, j = 0 .. 7, of column li: two reads, rows 8 lh + q and 8 lh + q + 4 --
// wb_frag(), given the two addresses (each kernel computes them in its own way).
//
// THE ACCUMULATOR TILE.  A wave owns 64 x 64 outputs as 4 x 4 MFMA tiles; lane (li, lh) holds D[row 4 lh + r][column li] of
// tile (i, j) in acc[i][j][r]: wb_zero_tile(), wb_store_tile().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nvqa {

typedef float wb_f32x4 __attribute__((ext_vector_type(4)));
typedef float wb_f32x2 __attribute__((ext_vector_type(2)));
typedef short wb_s16x4 __attribute__((ext_vector_type(4)));
typedef short wb_s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wb_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wb_bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned wb_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned wb_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) wb_s16x4 *wb_lds_s16x4;

__device__ __forceinline__ unsigned wb_off(int row, int ch) { return 256u * row + 16u * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// four f32 -> two packed bf16 pairs, round to nearest even
__device__ __forceinline__ wb_u32x2 wb_pack(wb_f32x4 v)
{
    const wb_f32x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
    return wb_u32x2{__builtin_bit_cast(unsigned, __builtin_convertvector(lo, wb_bf16x2)),
                    __builtin_bit_cast(unsigned, __builtin_convertvector(hi, wb_bf16x2))};
}
// and back: exact
__device__ __forceinline__ wb_f32x4 wb_widen(wb_u32x2 p)
{
    return wb_f32x4{__builtin_bit_cast(float, p[0] << 16), __builtin_bit_cast(float, p[0] & 0xffff0000u),
                    __builtin_bit_cast(float, p[1] << 16), __builtin_bit_cast(float, p[1] & 0xffff0000u)};
}
// the hi, mid and lo pieces of four values (k_dx0_split's K loop spells the same three steps out, one per MFMA group)
__device__ __forceinline__ void wb_split4(wb_f32x4 v, wb_u32x2 &h, wb_u32x2 &m, wb_u32x2 &l)
{
    h = wb_pack(v);
    v -= wb_widen(h);
    m = wb_pack(v);
    v -= wb_widen(m);
    l = wb_pack(v);
}
// ... and of one value
__device__ __forceinline__ void wb_split1(float w, __bf16 &hi, __bf16 &mid, __bf16 &lo)
{
    hi = (__bf16)w;
    const float r = w - (float)hi;
    mid = (__bf16)r;
    lo = (__bf16)(r - (float)mid);
}

// the six terms of a product, smallest first: piece (0 hi, 1 mid, 2 lo) of the A operand, piece of the B operand
constexpr int WB_TERM_A[6] = {2, 1, 0, 1, 0, 0}, WB_TERM_B[6] = {0, 1, 2, 0, 1, 0};

// the fragment whose two transposed reads start at p0 (rows 8 lh + q) and p1 (rows 8 lh + q + 4)
__device__ __forceinline__ wb_bf16x8 wb_frag(wb_lds_s16x4 p0, wb_lds_s16x4 p1)
{
    const wb_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p0);
    const wb_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p1);
    const wb_s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(wb_bf16x8, v);
}

__device__ __forceinline__ void wb_zero_tile(wb_f32x4 (&acc)[4][4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = wb_f32x4{0.f, 0.f, 0.f, 0.f};
}
// the wave's 64 x 64 outputs from (mw, nw) into out[M][ldo], rows past M and columns past N left alone
__device__ __forceinline__ void wb_store_tile(float *out, int ldo, int M, int N, int mw, int nw, int li, int lh, const wb_f32x4 (&acc)[4][4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = nw + 16 * j + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mw + 16 * i + 4 * lh + r;
                if (m < M && n < N) out[(size_t)m * ldo + n] = acc[i][j][r];
            }
        }
}

} // namespace nvqa
