// Index arithmetic of the windowed-sinc resampler (egr_resample_sinc, egr_resample_sinc_tracks in egr_resample_sinc.hip; SPEC.md 4f),
// kept free of device-only constructs so that the same text compiles for the host: tools/sinc_host_check.cpp walks it under
// -fsanitize=address,undefined.  As in egr_eval_index.h every refusal is decided here, from integers alone, before anything is
// allocated or launched, and the many-clip kernels find their track in the ascending output offsets with track_of
// (egr_ragged_index.h, with the grid caps).
//
// Names: o = src / gcd, n = dst / gcd, width = ceil(lpw o / base), L = 2 width + o taps per phase in the full definition,
// run = taps per phase the compact table keeps (the contiguous stretch with |t| < lpw, the same count for every phase, zero filled).
// Output m of a clip is phase p = m % n of frame i = m / n and reads x[i o + first_tap[p] - width + s], s in [0, run), zero outside
// the clip; the table is tap-major, Kt[s n + p].
#pragma once

#include "egr_ragged_index.h"

namespace egr {

constexpr int SINC_TILE = 256;                        // outputs per workgroup: one thread each
// LDS budget of the staged variant: 16 KiB of input per workgroup (the ABI allows at most 64 KiB).  Ten workgroups then share a CU's
// 160 KiB, and a filter whose 256-output span is larger (8000 -> 8001: 16014 floats for 256 x 14 products) re-uses too little of
// what it would stage: it reads x directly.
constexpr int SINC_LDS_FLOATS = 4096;
constexpr long long SINC_MAX_RATE = 1LL << 24;        // o, n: n run and 2 width + o stay far inside int32 / int64
constexpr long long SINC_MAX_WIDTH = 1LL << 28;
constexpr long long SINC_MAX_TABLE_FLOATS = 1LL << 29;    // n * run: 2 GiB of taps
constexpr unsigned SINC_FORCE_DIRECT = 1u;            // flag bit of both C calls (EGR_SINC_FORCE_DIRECT)

enum SincRefusal { SINC_OK = 0, SINC_SHORT = 1, SINC_BAD_RATE = 2, SINC_OFFSET = 3, SINC_TOTAL = 4, SINC_TABLE = 5, SINC_LENGTH = 6,
                   SINC_CHANNELS = 7 };

EGR_HD long long sinc_taps(long long o, long long width) { return 2 * width + o; }

// the filter's integers: rates, width, run inside [1, L], table size
EGR_HD int sinc_filter_check(long long o, long long n, long long width, long long run) {
    if (o < 1 || n < 1 || o > SINC_MAX_RATE || n > SINC_MAX_RATE || width < 1 || width > SINC_MAX_WIDTH) return SINC_BAD_RATE;
    if (run < 1 || run > sinc_taps(o, width)) return SINC_BAD_RATE;
    if (run > SINC_MAX_TABLE_FLOATS / n) return SINC_TABLE;
    return SINC_OK;
}

// ceil(n_in n / o); n_in n stays inside int64 for every n_in the checks below admit
EGR_HD long long sinc_out_len(long long n_in, long long o, long long n) { return (n_in * n + o - 1) / o; }

EGR_HD int sinc_length_check(long long n_in, long long o, long long n) {
    if (o < 1 || n < 1 || o > SINC_MAX_RATE || n > SINC_MAX_RATE) return SINC_BAD_RATE;
    if (n_in < 1) return SINC_SHORT;
    if (n_in > EVAL_MAX_OFF / 65536 || n_in > EVAL_MAX_OFF / n) return SINC_OFFSET;      // channels n_in <= 2^60, n_in n <= 2^60
    return SINC_OK;
}

// the single call: [channels][n_in] -> [channels][n_out], grid (tiles of n_out, channels)
EGR_HD int sinc_single_check(long long channels, long long n_in, long long n_out, long long o, long long n) {
    if (channels < 1 || channels > 65535) return SINC_CHANNELS;
    const int why = sinc_length_check(n_in, o, n);
    if (why != SINC_OK) return why;
    if (n_out != sinc_out_len(n_in, o, n)) return SINC_LENGTH;
    if (eval_ceil_div(n_out, SINC_TILE) > EVAL_MAX_GRID_256) return SINC_TOTAL;
    return SINC_OK;
}

// ---- tracks.  Row (4 int64): offset of the track in x, n_in, offset of its outputs in y, n_out = ceil(n_in n / o); the output
// offsets ascend back to back from 0.  *out0: the running total (in: this track's offset, out: the next track's).  Nothing is written
// on a refusal.
enum { ST_IN = 0, ST_N_IN, ST_OUT, ST_N_OUT, ST_COLS };
constexpr long long SINC_MAX_TOTAL = EVAL_MAX_GRID_256 * SINC_TILE;

EGR_HD int sinc_track_fill(long long in_off, long long n_in, long long o, long long n, long long* out0, long long* row) {
    const int why = sinc_length_check(n_in, o, n);
    if (why != SINC_OK) return why;
    if (in_off < 0 || in_off > EVAL_MAX_OFF) return SINC_OFFSET;
    const long long n_out = sinc_out_len(n_in, o, n);
    if (n_out > SINC_MAX_TOTAL - *out0) return SINC_TOTAL;
    row[ST_IN] = in_off; row[ST_N_IN] = n_in; row[ST_OUT] = *out0; row[ST_N_OUT] = n_out;
    *out0 += n_out;
    return SINC_OK;
}

// what the many-clip call can decide without reading the (device) table
EGR_HD int sinc_tracks_check(long long n_tracks, long long total_out) {
    if (n_tracks < 1 || total_out < 1) return SINC_SHORT;
    if (n_tracks > total_out) return SINC_LENGTH;                       // every track has at least one output
    if (total_out > SINC_MAX_TOTAL) return SINC_TOTAL;
    return SINC_OK;
}

// ---- one output sample
EGR_HD long long sinc_frame_phase(long long m, long long n, int* p) {
    const long long i = m / n;
    *p = (int)(m - i * n);
    return i;
}

// a phase's first tap as the kernels use it: inside [0, L - run], so that no read leaves the L taps of the definition
EGR_HD long long sinc_first_tap(long long f, long long o, long long width, long long run) {
    const long long hi = sinc_taps(o, width) - run;
    return f < 0 ? 0 : (f > hi ? hi : f);
}

// index into x of tap 0 of the run (negative in front of the clip; run - 1 further it may pass the clip's end)
EGR_HD long long sinc_first_in(long long i, long long o, long long width, long long f) { return i * o + f - width; }

// ---- a tile: len <= 256 consecutive outputs of one track from local output m0.  -> floats of x the tile can read, *lo = index into x
// of the first (negative in front of the clip): every tap of every frame the tile touches.
EGR_HD long long sinc_tile_span(long long m0, long long len, long long o, long long n, long long width, long long* lo) {
    const long long i0 = m0 / n, i1 = (m0 + len - 1) / n;
    *lo = i0 * o - width;
    return (i1 - i0) * o + sinc_taps(o, width);
}

// slot of the staged span that holds tap 0 of output m's run (the tile starts at m0)
EGR_HD long long sinc_stage_slot(long long m0, long long i, long long o, long long n, long long f) { return (i - m0 / n) * o + f; }

// the largest span a 256-output tile can have, whatever its alignment: floor((n - 1 + 255) / n) frame steps
EGR_HD long long sinc_max_span(long long o, long long n, long long width) {
    return ((n + SINC_TILE - 2) / n) * o + sinc_taps(o, width);
}

// the variant rule: from (o, n, width) alone, never from a clip's length or from what else is in a call
EGR_HD bool sinc_staged(long long o, long long n, long long width) { return sinc_max_span(o, n, width) <= SINC_LDS_FLOATS; }

// ---- the stretch of a 256-output tile of the flat many-clip grid that belongs to one track.  pos in [tile start, end): the first flat
// output not yet handed out; *t: a track at or before pos's (in: from track_of of the tile start or the last call, out: pos's track).
// -> the flat end of the stretch (> pos); *m0 / *len: its first local output and length inside the track (len 0: a gap in the table).
EGR_HD long long sinc_segment(const long long* __restrict__ tracks, int n_tracks, long long total_out, long long end, long long pos,
                                   int* t, long long* m0, long long* len) {
    while (*t + 1 < n_tracks && tracks[(size_t)(*t + 1) * ST_COLS + ST_OUT] <= pos) ++*t;
    const long long* e = tracks + (size_t)*t * ST_COLS;
    const long long next = *t + 1 < n_tracks ? tracks[(size_t)(*t + 1) * ST_COLS + ST_OUT] : total_out;
    const long long seg_end = next < end ? next : end;
    *m0 = pos - e[ST_OUT];
    const long long left = e[ST_N_OUT] - *m0;
    *len = left < 1 || *m0 < 0 ? 0 : (left < seg_end - pos ? left : seg_end - pos);
    return seg_end;
}

}  // namespace egr
