// Index arithmetic of the many-pair metrics and the many-clip loudness meter (egr_metrics_pairs, egr_loudness_tracks in egr_glue.hip),
// kept free of device-only constructs so that the same text compiles for the host: tools/evalmany_host_check.cpp walks it under
// -fsanitize=address,undefined.  The host fills one table row per pair / clip with these functions (every refusal is decided here, from
// integers alone, before anything is allocated or launched); the kernels find their row in the ascending prefix columns with track_of
// (egr_ragged_index.h).
#pragma once

#include "egr_ragged_index.h"

namespace egr {

constexpr int EGR_METRICS_CHUNK = 4096;          // samples per SI-SDR partial sum: one workgroup of 256 threads, 16 samples each
// (the caps of a grid and of an offset are in egr_ragged_index.h)
constexpr long long EVAL_MAX_PAIRS = eval_max_grid(1024);            // 2^22 - 1: k_pair_lsd_reduce has one 1024-thread workgroup per pair
constexpr long long EVAL_MAX_KW_CHUNKS = eval_max_grid(64) * 64;     // thread chunks of k_kweight_mono_tracks: 64 to a workgroup

// frames = 1 + max(0, (n - block) / hop): the frame rule of egr_stft_mag and of the loudness block families
EGR_HD long long eval_frames(long long n, long long block, long long hop) { return 1 + (n > block ? (n - block) / hop : 0); }

enum EvalRefusal { EVAL_OK = 0, EVAL_SHORT = 1, EVAL_BAD_ROW = 2, EVAL_OFFSET = 3, EVAL_TOTAL = 4 };

// ---- pairs.  Caller's row (7 int64): offset of side A in a, its channels, its row stride; the same for side B in b; n = min(len_a, len_b).
constexpr int MP_IN_COLS = 7;
// Device row (12 int64): the caller's seven, then frames, first flat frame, first flat chunk, the two ranks of numpy's linear 95th percentile.
enum { MP_OFF_A = 0, MP_CA, MP_LD_A, MP_OFF_B, MP_CB, MP_LD_B, MP_N, MP_FRAMES, MP_FRAME0, MP_CHUNK0, MP_KLO, MP_KHI, MP_COLS };

EGR_HD long long metrics_chunks(long long n) { return eval_ceil_div(n, EGR_METRICS_CHUNK); }

// side (offset, channels, stride) holding n samples per row: the last float read is offset + (channels - 1) stride + n - 1
EGR_HD bool eval_side_ok(long long off, long long ch, long long ld, long long n) {
    if (off < 0 || off > EVAL_MAX_OFF || ch < 1 || ch > 65535 || ld < n || ld > EVAL_MAX_OFF / 65536) return false;
    return off + (ch - 1) * ld + n <= EVAL_MAX_OFF;
}

// One row of the device table from one caller's row; *frame0 / *chunk0 are the running totals (in: this pair's first, out: the next
// pair's).  Nothing is written on a refusal.
EGR_HD int metrics_fill(const long long* in, int n_fft, int hop, long long* frame0, long long* chunk0, long long* row) {
    const long long n = in[6];
    if (n < 1) return EVAL_SHORT;
    if (n > EVAL_MAX_OFF) return EVAL_OFFSET;
    if (in[1] < 1 || in[1] > 65535 || in[4] < 1 || in[4] > 65535 || in[2] < n || in[5] < n) return EVAL_BAD_ROW;
    if (!eval_side_ok(in[0], in[1], in[2], n) || !eval_side_ok(in[3], in[4], in[5], n)) return EVAL_OFFSET;
    const long long frames = eval_frames(n, n_fft, hop), chunks = metrics_chunks(n);
    if (frames > EVAL_MAX_GRID_256 - *frame0 || chunks > EVAL_MAX_GRID_256 - *chunk0) return EVAL_TOTAL;
    for (int c = 0; c < MP_IN_COLS; ++c) row[c] = in[c];
    row[MP_FRAMES] = frames;
    row[MP_FRAME0] = *frame0;
    row[MP_CHUNK0] = *chunk0;
    const long long lo = (long long)(0.95 * (double)(frames - 1));       // floor: the position is not negative
    row[MP_KLO] = lo;
    row[MP_KHI] = lo + 1 < frames ? lo + 1 : frames - 1;
    *frame0 += frames;
    *chunk0 += chunks;
    return EVAL_OK;
}

// flat frame -> pair and the frame inside the pair; flat chunk -> pair and the chunk's first sample and length inside the pair
EGR_HD int metrics_frame_of(const long long* tab, int n_pairs, long long flat, long long* f) {
    const int p = track_of(tab, n_pairs, MP_COLS, MP_FRAME0, flat);
    *f = flat - tab[(size_t)p * MP_COLS + MP_FRAME0];
    return p;
}
EGR_HD int metrics_chunk_of(const long long* tab, int n_pairs, long long flat, long long* first, long long* len) {
    return tile_of(tab, n_pairs, MP_COLS, MP_CHUNK0, MP_N, EGR_METRICS_CHUNK, flat, first, len);
}

// ---- clips of one (sample rate, channel count) group.  Caller's row (2 int64): offset of the clip's [C][n] block in x, n.
constexpr int LT_IN_COLS = 2;
// Device row (8 int64): the two, offset of the clip's K-weighted mono in the workspace, first flat thread chunk, first flat block of
// either family, first flat 256-sample tile of the oversampled signal, spare.
enum { LT_OFF = 0, LT_N, LT_MONO, LT_CHUNK0, LT_FA0, LT_FB0, LT_TILE0, LT_SPARE, LT_COLS };
constexpr int LT_TILE = 256;

struct LoudTotals { long long mono, chunks, fa, fb, tiles; };

// blk_b = 0: no second family (its column stays a copy of the first, never searched); up = 0: no true peak
EGR_HD int loud_fill(const long long* in, int channels, int L, long long blk_a, long long hop_a, long long blk_b, long long hop_b,
                          int up, LoudTotals* t, long long* row) {
    const long long n = in[1];
    if (n < 1) return EVAL_SHORT;
    if (n > EVAL_MAX_OFF / 64) return EVAL_OFFSET;
    if (!eval_side_ok(in[0], channels, n, n)) return EVAL_OFFSET;
    const long long chunks = eval_ceil_div(n, L), fa = eval_frames(n, blk_a, hop_a), fb = blk_b ? eval_frames(n, blk_b, hop_b) : 0;
    const long long tiles = up ? eval_ceil_div(n * up, LT_TILE) : 0;
    if (chunks > EVAL_MAX_KW_CHUNKS - t->chunks || fa > EVAL_MAX_GRID_256 - t->fa || fb > EVAL_MAX_GRID_256 - t->fb ||
        tiles > EVAL_MAX_GRID_256 - t->tiles ||
        n > EVAL_MAX_OFF - t->mono)
        return EVAL_TOTAL;
    row[LT_OFF] = in[0]; row[LT_N] = n; row[LT_MONO] = t->mono; row[LT_CHUNK0] = t->chunks; row[LT_FA0] = t->fa;
    row[LT_FB0] = blk_b ? t->fb : t->fa; row[LT_TILE0] = up ? t->tiles : t->fa; row[LT_SPARE] = 0;
    t->mono += n; t->chunks += chunks; t->fa += fa; t->fb += fb; t->tiles += tiles;
    return EVAL_OK;
}

// flat index in one of the prefix columns -> clip and the index inside the clip
EGR_HD int loud_item_of(const long long* tab, int n_clips, int col, long long flat, long long* local) {
    const int c = track_of(tab, n_clips, LT_COLS, col, flat);
    *local = flat - tab[(size_t)c * LT_COLS + col];
    return c;
}

}  // namespace egr
