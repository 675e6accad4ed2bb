// Device helpers shared by the split-operand contraction kernels (egr_nn_gemm_s3.hip: implicit-GEMM / 1-D / batched kernels;
// egr_nn_conv3x3.hip: the input-stationary 3x3 kernels): the exact operand splits (three bf16 terms / two fp16 terms of the
// pre-scaled operand / one fp16 term of it), the partial-product sequences, the LDS slots of operand and halo tiles, and the wave layout of a block tile.
#pragma once
#include "egr_conv.h"
#include "egr_rowmax.h"

namespace egr {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define S3_BK 16

__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {        // RNE; a -> bits 0..15, b -> bits 16..31
    f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// (a, b) -> packed bf16 pairs of the three split terms
__device__ __forceinline__ void split3_pair(float a, float b, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
    p0 = pk_bf16(a, b);
    const float ra = a - __uint_as_float(p0 << 16), rb = b - __uint_as_float(p0 & 0xffff0000u);
    p1 = pk_bf16(ra, rb);
    const float sa = ra - __uint_as_float(p1 << 16), sb = rb - __uint_as_float(p1 & 0xffff0000u);
    p2 = pk_bf16(sa, sb);
}

__device__ __forceinline__ void split3_x8(const float4& u, const float4& v, uint4& q0, uint4& q1, uint4& q2) {
    split3_pair(u.x, u.y, q0.x, q1.x, q2.x);
    split3_pair(u.z, u.w, q0.y, q1.y, q2.y);
    split3_pair(v.x, v.y, q0.z, q1.z, q2.z);
    split3_pair(v.z, v.w, q0.w, q1.w, q2.w);
}

// ---- scheme 1: two fp16 terms of the pre-scaled operand (x s = h0 + h1, h0 = f16(x s), h1 = f16(x s - h0); s a power of two that
// brings the tensor's largest magnitude near 2^12, so every element down to 2^-15 of it keeps 22 significand bits and smaller ones
// an absolute error of 2^-37 of the maximum).  f16 x f16 products are exact in fp32, so  a0 b0 + a0 b1 + a1 b0  carries the fp32
// product up to a1 b1 and the two term roundings (each < 2^-22 |a b|) with HALF the matrix instructions of the bf16 scheme and
// one third fewer LDS operand bytes; fewer accumulator roundings per 16 k (3 instead of 6) make the measured error against
// float64 no larger (tests/test_gpu_split_h2.py).  s is per BATCH ROW and comes from the device: row_amax[b] holds the bits of
// max |x| of row b (left there by the tensor's producer, or by k_absmax_rows), and h2_row_scale turns its exponent into the power
// of two that puts the row's maximum in [2^14, 2^15) -- no host round trip, no history, and a quiet row next to a loud one keeps
// its own 22 bits (csrc/egr_conv.h, csrc/egr_flashsr.cpp).
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split2h_pair(float a, float b, float s, uint32_t& p0, uint32_t& p1) {
    const float as = a * s, bs = b * s;
    const f32x2 v = {as, bs};
    const f16x2 hi = __builtin_convertvector(v, f16x2);                // RNE (v_cvt_pk_f16_f32)
    p0 = __builtin_bit_cast(uint32_t, hi);
    const f32x2 r = {as - (float)hi[0], bs - (float)hi[1]};            // exact
    p1 = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2));
}

__device__ __forceinline__ void split2h_x8(const float4& u, const float4& v, float s, uint4& q0, uint4& q1) {
    split2h_pair(u.x, u.y, s, q0.x, q1.x);
    split2h_pair(u.z, u.w, s, q0.y, q1.y);
    split2h_pair(v.x, v.y, s, q0.z, q1.z);
    split2h_pair(v.z, v.w, s, q0.w, q1.w);
}

// ---- scheme 2: ONE fp16 term of the pre-scaled operand, h0 = f16(x s) with the s of scheme 1 (the row's maximum in [2^14, 2^15):
// nothing overflows, and an element keeps 11 significand bits down to 2^-29 of its row's maximum).  The weight operand is plane 0 of
// the scheme-1 pack, f16(w w_scale); one exact product a0 b0 per 16 k accumulated in fp32.  The result is the fp32-accumulated
// contraction of the ROUNDED operands (each within 2^-12 relative of its fp32 value): a third of scheme 1's matrix instructions and
// half its LDS operand bytes, for previews and batch jobs that do not need fp32-grade results.  Opt-in only (egr_conv_h1,
// EGR_FSR_FAST_F16); scales, epilogue and row maxima are those of scheme 1.
__device__ __forceinline__ uint32_t pk_f16_scaled(float a, float b, float s) {   // RNE (v_cvt_pk_f16_f32); a -> bits 0..15
    const f32x2 v = {a * s, b * s};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
}

__device__ __forceinline__ void split1h_x8(const float4& u, const float4& v, float s, uint4& q0) {
    q0.x = pk_f16_scaled(u.x, u.y, s);
    q0.y = pk_f16_scaled(u.z, u.w, s);
    q0.z = pk_f16_scaled(v.x, v.y, s);
    q0.w = pk_f16_scaled(v.z, v.w, s);
}

// Operand planes (terms of the split) a kernel of scheme SCH keeps per tile, and the planes per 16-k slab of the weight pack it reads
// (scheme 2 reads plane 0 of the two-plane pack of scheme 1: the slab stride stays that pack's).
template <int SCH> __host__ __device__ constexpr int s3_planes() { static_assert(SCH >= 0 && SCH <= 2, "operand scheme"); return SCH == 0 ? 3 : (SCH == 1 ? 2 : 1); }
template <int SCH> __host__ __device__ constexpr int s3_pack_planes() { return SCH == 0 ? 3 : 2; }

// the operand split of scheme SCH into its NP planes q[0..NP)
template <int SCH>
__device__ __forceinline__ void split_x8(const float4& u, const float4& v, float s, uint4 (&q)[3]) {
    if constexpr (SCH == 0) split3_x8(u, v, q[0], q[1], q[2]);
    else if constexpr (SCH == 1) split2h_x8(u, v, s, q[0], q[1]);
    else split1h_x8(u, v, s, q[0]);
}

// <BM, BN> block tile, 4 waves.  256x128: waves 2x2, each 128x64 (TM 4, TN 2; the large-M workhorse: half the split work and
// 0.7x the L2 traffic per MFMA of the 128x128 tile).  128xBN: small-M / thin-Cout layers and split-K.
template <int BM, int BN> struct S3Cfg;
template <> struct S3Cfg<256, 128> { static constexpr int WM = 2, WN = 2, TM = 4, TN = 2; };
template <> struct S3Cfg<128, 256> { static constexpr int WM = 2, WN = 2, TM = 2, TN = 4; };   // Cout >= 256: half the A work per MFMA
template <> struct S3Cfg<128, 128> { static constexpr int WM = 2, WN = 2, TM = 2, TN = 2; };
template <> struct S3Cfg<128, 64> { static constexpr int WM = 2, WN = 2, TM = 2, TN = 1; };
template <> struct S3Cfg<128, 32> { static constexpr int WM = 4, WN = 1, TM = 1, TN = 1; };

__device__ __forceinline__ bf16x8 as_bf(const uint4& v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ f16x8 as_hf(const uint4& v) { return __builtin_bit_cast(f16x8, v); }

template <int TM, int TN>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// ---- partial products.  a[i][q] / b[j][q]: plane q of the wave's 32-row sub-tile i of the first / 32-column sub-tile j of the second
// tile (one uint4 = this lane's 8 k).  One term (plane QA of a times plane QB of b) over TA x TB sub-tiles, accumulated into
// acc[i0 + i][j0 + j].  WFIRST issues mfma(b, a): the weight tile as the first operand, accumulators transposed (conv_epilogue_t).
template <int SCH, bool WFIRST, int QA, int QB, int TA, int TB, int NA, int NB, int TM, int TN>
__device__ __forceinline__ void mma_term(const uint4 (*a)[NA], const uint4 (*b)[NB], f32x16 (&acc)[TM][TN], int i0 = 0, int j0 = 0) {
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            const uint4 &x = WFIRST ? b[j][QB] : a[i][QA], &y = WFIRST ? a[i][QA] : b[j][QB];
            f32x16& c = acc[i0 + i][j0 + j];
            if constexpr (SCH == 0) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(x), as_bf(y), c, 0, 0, 0);
            else c = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_hf(x), as_hf(y), c, 0, 0, 0);
        }
}

// All terms of scheme SCH for one 16-k slab, smallest terms first (the large products then meet a sum that already holds the small
// ones): scheme 0 (2,0) (0,2) (1,1) (1,0) (0,1) (0,0), scheme 1 (1,0) (0,1) (0,0), scheme 2 (0,0).  The order is TERM-outer, sub-tile-inner: an MFMA
// that accumulates into the register block its predecessor wrote waits for that result, so each term runs across all TA x TB
// accumulator blocks before the next term returns to the first of them and consecutive MFMAs are independent.  (All terms of one
// block back to back would be the same sum in the same order per block, with every MFMA waiting for the one before it.)
template <int SCH, bool WFIRST, int TA, int TB, int NA, int NB, int TM, int TN>
__device__ __forceinline__ void mma_terms(const uint4 (*a)[NA], const uint4 (*b)[NB], f32x16 (&acc)[TM][TN], int i0 = 0, int j0 = 0) {
    if constexpr (SCH == 0) {
        mma_term<0, WFIRST, 2, 0, TA, TB>(a, b, acc, i0, j0);
        mma_term<0, WFIRST, 0, 2, TA, TB>(a, b, acc, i0, j0);
        mma_term<0, WFIRST, 1, 1, TA, TB>(a, b, acc, i0, j0);
    }
    if constexpr (SCH != 2) {
        mma_term<SCH, WFIRST, 1, 0, TA, TB>(a, b, acc, i0, j0);
        mma_term<SCH, WFIRST, 0, 1, TA, TB>(a, b, acc, i0, j0);
    }
    mma_term<SCH, WFIRST, 0, 0, TA, TB>(a, b, acc, i0, j0);
}

// ---- LDS slots (uint4 units within one plane).  These two are macros, not functions: an inline function is simplified on its own
// before it is inlined, and that changed the address arithmetic, VGPR counts and spills of the 128 x 256 and the 3x3 instantiations
// (profiles/split_tile_helpers.md); the textual form compiles to what the kernels held before.
// Operand tile [row][2 halves of 8 k]: the half is XOR-ed with bit 3 of the row, which makes the loaders' ds_write_b128 and the MFMA
// operand ds_read_b128 (lane l: row l & 31, half l >> 5) conflict-free at a 32-byte pitch.
#define S3_TILE_SLOT(row, half) ((row) * 2 + ((half) ^ (((row) >> 3) & 1)))
// Halo tile [row][NCH chunks of 8 channels] of the input-stationary kernels, read at a row offset per tap: the chunk is XOR-ed with
// (row / (16 / NCH)) & (NCH - 1) -- conflict-free ds_read_b128 for ANY row offset (brute-forced over all offsets for NCH = 2, 4).
#define S3_HALO_SLOT(NCH, r, ch) ((r) * (NCH) + ((ch) ^ (((r) / (16 / (NCH))) & ((NCH) - 1))))

}  // namespace egr
