// Index arithmetic of the many-pair null test (egr_nullmany_delays in egr_fatllama.hip, egr_nullmany_shift_fir and egr_nullmany_mix in
// egr_glue.hip), kept free of device-only constructs so that the same text compiles for the host: tools/nullmany_host_check.cpp walks it
// under -fsanitize=address,undefined.  As in egr_eval_index.h the host fills one table row per pair / row with these functions (every
// refusal is decided here, from integers alone, before anything is allocated or launched) and the kernels find their row in the ascending
// prefix columns with track_of / tile_of (egr_ragged_index.h).  eval_side_ok and the chunk length are egr_eval_index.h's.  Every grid is flat and equals its work count.
#pragma once

#include "egr_eval_index.h"

namespace egr {

constexpr int NULL_TILE = 256;                       // samples per pack tile and per shift-FIR output tile: one workgroup of 256 threads
constexpr int NULL_CHUNK = EGR_METRICS_CHUNK;        // samples per partial sum of the mix: 16 per thread
constexpr long long NULL_MAX_GROUP_ROWS = 65535;     // rows of one transform group: gridDim.y of the transform passes
constexpr int NULL_MAX_TAPS = 4096;                  // taps of one shift-FIR call: (256 + 2 taps) floats of LDS stay below 64 KiB
constexpr int NULL_SUMS = 8;                         // doubles per chunk and per pair of the mix (seven sums, one spare)

enum NullRefusal { NULL_OK = 0, NULL_SHORT = 1, NULL_BAD_ROW = 2, NULL_OFFSET = 3, NULL_TOTAL = 4, NULL_LENGTH = 5, NULL_MAX_SHIFT = 6,
                   NULL_CHANNELS = 7, NULL_TAPS = 8 };

// the single path's rule (device_ops.xcorr_delay): n = 1; while (n < na + nb) n <<= 1, with na = nb = n_common
EGR_HD long long null_transform_length(long long n_common) {
    long long n = 1;
    while (n < 2 * n_common) n <<= 1;
    return n;
}

// ---- delays.  Caller's row and device row (8 int64): offset of side A in a, its channels, its row stride; the same for side B in b;
// n_common = min(len_a, len_b); max_shift in samples.  All rows of one call share the transform length n.
enum { ND_OFF_A = 0, ND_CA, ND_LD_A, ND_OFF_B, ND_CB, ND_LD_B, ND_N, ND_MS, ND_COLS };

EGR_HD long long delays_tiles(long long n) { return eval_ceil_div(n, NULL_TILE); }

// *tile0: the running total of pack tiles (in: this pair's first, out: the next pair's)
EGR_HD int delays_fill(const long long* in, long long n, long long* tile0, long long* row) {
    const long long nc = in[ND_N];
    if (nc < 1) return NULL_SHORT;
    if (nc > EVAL_MAX_OFF / 4) return NULL_OFFSET;
    if (in[ND_CA] < 1 || in[ND_CA] > 65535 || in[ND_CB] < 1 || in[ND_CB] > 65535 || in[ND_LD_A] < nc || in[ND_LD_B] < nc) return NULL_BAD_ROW;
    if (!eval_side_ok(in[ND_OFF_A], in[ND_CA], in[ND_LD_A], nc) || !eval_side_ok(in[ND_OFF_B], in[ND_CB], in[ND_LD_B], nc)) return NULL_OFFSET;
    if (null_transform_length(nc) != n) return NULL_LENGTH;
    if (in[ND_MS] < 0 || in[ND_MS] >= n / 2 - 1) return NULL_MAX_SHIFT;
    if (delays_tiles(n) > EVAL_MAX_GRID_256 - *tile0) return NULL_TOTAL;
    for (int c = 0; c < ND_COLS; ++c) row[c] = in[c];
    *tile0 += delays_tiles(n);
    return NULL_OK;
}

// flat pack tile -> pair and the tile's first sample (every pair has the same number of tiles)
EGR_HD int delays_tile_of(long long n, long long flat, long long* first) {
    const long long t = delays_tiles(n);
    *first = (flat % t) * NULL_TILE;
    return (int)(flat / t);
}

// ---- shift + FIR.  Caller's row (6 int64): offset of the input row in x, n_in, integer shift, row of the taps table or -1 (no taps),
// offset of the output row in y, n_out.  Device row (8 int64): the six, the first flat output tile, spare.
constexpr int SF_IN_COLS = 6;
enum { SF_IN = 0, SF_N_IN, SF_SHIFT, SF_TAPS, SF_OUT, SF_N_OUT, SF_TILE0, SF_SPARE, SF_COLS };

EGR_HD int shiftfir_fill(const long long* in, long long n_tap_rows, long long* tile0, long long* row) {
    const long long n_in = in[SF_N_IN], n_out = in[SF_N_OUT];
    if (n_in < 1 || n_out < 1) return NULL_SHORT;
    if (n_in > EVAL_MAX_OFF / 4 || n_out > EVAL_MAX_OFF / 4 || in[SF_SHIFT] > EVAL_MAX_OFF / 4 || in[SF_SHIFT] < -(EVAL_MAX_OFF / 4)) return NULL_OFFSET;
    if (!eval_side_ok(in[SF_IN], 1, n_in, n_in) || !eval_side_ok(in[SF_OUT], 1, n_out, n_out)) return NULL_OFFSET;
    if (in[SF_TAPS] < -1 || in[SF_TAPS] >= n_tap_rows) return NULL_TAPS;
    const long long tiles = eval_ceil_div(n_out, NULL_TILE);
    if (tiles > EVAL_MAX_GRID_256 - *tile0) return NULL_TOTAL;
    for (int c = 0; c < SF_IN_COLS; ++c) row[c] = in[c];
    row[SF_TILE0] = *tile0;
    row[SF_SPARE] = 0;
    *tile0 += tiles;
    return NULL_OK;
}

// flat output tile -> row, the tile's first output sample and its length
EGR_HD int shiftfir_tile_of(const long long* tab, int n_rows, long long flat, long long* first, long long* len) {
    return tile_of(tab, n_rows, SF_COLS, SF_TILE0, SF_N_OUT, NULL_TILE, flat, first, len);
}

// ---- mix.  Caller's row (8 int64): offset of the reference in a, its channels, its row stride; the same for the aligned signal in b;
// n = samples per row; offset of the pair's [channels][n] block in each output.  Device row (8 int64): offset a, stride a, offset b,
// stride b, channels, n, output offset, first flat chunk.
constexpr int NM_IN_COLS = 8;
enum { NM_OFF_A = 0, NM_LD_A, NM_OFF_B, NM_LD_B, NM_CH, NM_N, NM_OUT, NM_CHUNK0, NM_COLS };

EGR_HD long long mix_chunks(long long n) { return eval_ceil_div(n, NULL_CHUNK); }

EGR_HD int mix_fill(const long long* in, long long* chunk0, long long* row) {
    const long long n = in[6];
    if (n < 1) return NULL_SHORT;
    if (n > EVAL_MAX_OFF / 65536) return NULL_OFFSET;
    if (in[1] < 1 || in[1] > 65535 || in[4] < 1 || in[4] > 65535 || in[2] < n || in[5] < n) return NULL_BAD_ROW;
    if (in[1] != in[4]) return NULL_CHANNELS;
    if (!eval_side_ok(in[0], in[1], in[2], n) || !eval_side_ok(in[3], in[4], in[5], n) || !eval_side_ok(in[7], in[1], n, n)) return NULL_OFFSET;
    const long long chunks = mix_chunks(n);
    if (chunks > EVAL_MAX_GRID_256 - *chunk0) return NULL_TOTAL;
    row[NM_OFF_A] = in[0]; row[NM_LD_A] = in[2]; row[NM_OFF_B] = in[3]; row[NM_LD_B] = in[5];
    row[NM_CH] = in[1]; row[NM_N] = n; row[NM_OUT] = in[7]; row[NM_CHUNK0] = *chunk0;
    *chunk0 += chunks;
    return NULL_OK;
}

// flat chunk -> pair, the chunk's first sample and its length (no chunk spans two pairs)
EGR_HD int mix_chunk_of(const long long* tab, int n_pairs, long long flat, long long* first, long long* len) {
    return tile_of(tab, n_pairs, NM_COLS, NM_CHUNK0, NM_N, NULL_CHUNK, flat, first, len);
}

#if defined(__HIPCC__)
// mean over channels as numpy's float32 .mean(axis=0): rows added in order, one division.  The mono kernels of egr_glue.hip and the
// pack kernel of egr_nullmany_delays (egr_fatllama.hip) all call it.
__device__ __forceinline__ float mono_mean(const float* __restrict__ x, int C, long long ld, long long i) {
    float m = x[i];
    for (int c = 1; c < C; ++c) m = __fadd_rn(m, x[(size_t)c * ld + i]);
    return C > 1 ? __fdiv_rn(m, (float)C) : m;
}
#endif

}  // namespace egr
