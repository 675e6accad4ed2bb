// Host walk of csrc/egr_sinc_index.h: the frame / phase split, the staged span and its slots, the variant rule, the track table and the
// per-tile stretches of egr_resample_sinc and egr_resample_sinc_tracks.  Meant to be built with a host compiler under the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/sinc_host_check.cpp -o sinc_host_check
// The staged span of a tile is a heap block of exactly its size and the x of a track a heap block of exactly n_in floats, so a slot
// or a sample outside them is reported.  For every thread of every tile the staged read of every tap must stay inside the span and
// must hold the same x sample (or the same zero) the direct variant reads; every output of every track must be met exactly once and
// in order; the tiles of the flat grid must hand every output of a ragged table (clips of one sample, tracks that start inside a
// tile) to exactly one stretch; the variant rule must follow the span alone; the refusals (lengths below 1, offsets and lengths at
// the edge of int64, tables over the cap, totals past one grid) must come back as codes without any overflow.
// Exit status 0 = all pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../comfyui-egregora-audio-super-resolution_amd/csrc/egr_sinc_index.h"

using namespace egr;

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint32_t urand(uint32_t n) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); fflush(stdout); return 1; } while (0)

struct Filter { long long o, n, width, run; std::vector<int> first_tap; };

// first taps as a design gives them (the stretch follows p o / n) plus values outside [0, L - run] that the kernels must clamp
static Filter make_filter(long long o, long long n, long long width, long long run) {
    Filter F{o, n, width, run, {}};
    const long long L = sinc_taps(o, width);
    for (long long p = 0; p < n; ++p) {
        long long f = p * o / n + (long long)urand(3) - 1;
        if (p % 97 == 5) f = -3;
        if (p % 97 == 6) f = L + 2;
        F.first_tap.push_back((int)f);
    }
    return F;
}

// one clip of n_in samples through the single call's grid: staged tiles against direct reads
static int walk_single(const char* name, const Filter& F, long long n_in) {
    const long long L = sinc_taps(F.o, F.width), n_out = sinc_out_len(n_in, F.o, F.n);
    if (sinc_single_check(1, n_in, n_out, F.o, F.n) != SINC_OK) FAIL("%s: n_in %lld refused", name, n_in);
    float* x = (float*)malloc((size_t)n_in * sizeof(float));
    for (long long k = 0; k < n_in; ++k) x[k] = (float)(k + 1);
    long long met = 0;
    for (long long m0 = 0; m0 < n_out; m0 += SINC_TILE) {
        const long long len = n_out - m0 < SINC_TILE ? n_out - m0 : SINC_TILE;
        long long lo;
        const long long span = sinc_tile_span(m0, len, F.o, F.n, F.width, &lo);
        if (span < L || span > sinc_max_span(F.o, F.n, F.width)) FAIL("%s: tile %lld: span %lld outside [%lld, %lld]", name, m0, span, L, sinc_max_span(F.o, F.n, F.width));
        float* lds = (float*)malloc((size_t)span * sizeof(float));
        for (long long q = 0; q < span; ++q) {
            const long long k = lo + q;
            lds[q] = (k >= 0 && k < n_in) ? x[k] : 0.f;
        }
        for (long long j = 0; j < len; ++j, ++met) {
            const long long m = m0 + j;
            int p;
            const long long i = sinc_frame_phase(m, F.n, &p);
            if (p < 0 || p >= F.n || i * F.n + p != m) FAIL("%s: output %lld -> frame %lld phase %d", name, m, i, p);
            const long long f = sinc_first_tap(F.first_tap[(size_t)p], F.o, F.width, F.run);
            if (f < 0 || f + F.run > L) FAIL("%s: phase %d: first tap %lld with run %lld of %lld", name, p, f, F.run, L);
            const long long slot = sinc_stage_slot(m0, i, F.o, F.n, f), first = sinc_first_in(i, F.o, F.width, f);
            if (slot < 0 || slot + F.run > span || lo + slot != first) FAIL("%s: output %lld: slot %lld of span %lld", name, m, slot, span);
            for (long long s = 0; s < F.run; s += (F.run > 4 && s > 0 && s < F.run - 2 ? F.run - 3 : 1)) {
                const long long k = first + s;
                const float direct = (k >= 0 && k < n_in) ? x[k] : 0.f;
                if (lds[slot + s] != direct) FAIL("%s: output %lld tap %lld: staged %g, direct %g", name, m, s, lds[slot + s], direct);
            }
        }
        free(lds);
    }
    free(x);
    if (met != n_out) FAIL("%s: met %lld of %lld outputs", name, met, n_out);
    return 0;
}

// ragged tracks through the flat grid: every output in exactly one stretch, stretches inside one track and one tile
static int walk_tracks(const char* name, const Filter& F, const std::vector<long long>& n_ins) {
    const int nt = (int)n_ins.size();
    long long* tab = (long long*)malloc((size_t)nt * ST_COLS * sizeof(long long));
    long long total = 0, in_off = 3;
    for (int t = 0; t < nt; ++t) {
        if (sinc_track_fill(in_off, n_ins[t], F.o, F.n, &total, tab + (size_t)t * ST_COLS) != SINC_OK) FAIL("%s: track %d refused", name, t);
        in_off += n_ins[t] + t % 3;
    }
    if (sinc_tracks_check(nt, total) != SINC_OK) FAIL("%s: table refused", name);
    std::vector<unsigned char> seen((size_t)total, 0);
    long long mid_tile_starts = 0, stretches = 0;
    for (int t = 1; t < nt; ++t) mid_tile_starts += tab[(size_t)t * ST_COLS + ST_OUT] % SINC_TILE != 0;
    for (long long base = 0; base < total; base += SINC_TILE) {
        const long long end = base + SINC_TILE < total ? base + SINC_TILE : total;
        int t = track_of(tab, nt, ST_COLS, ST_OUT, base);
        for (long long pos = base; pos < end;) {
            long long m0, len;
            const long long seg_end = sinc_segment(tab, nt, total, end, pos, &t, &m0, &len);
            const long long* e = tab + (size_t)t * ST_COLS;
            if (seg_end <= pos || seg_end > end || len != seg_end - pos || m0 < 0 || m0 + len > e[ST_N_OUT] || e[ST_OUT] + m0 != pos)
                FAIL("%s: tile %lld: stretch [%lld, %lld) -> track %d from %lld, %lld long", name, base, pos, seg_end, t, m0, len);
            long long lo;
            if (sinc_tile_span(m0, len, F.o, F.n, F.width, &lo) > sinc_max_span(F.o, F.n, F.width)) FAIL("%s: stretch span above the rule's", name);
            for (long long j = 0; j < len; ++j) {
                const int lane = (int)(pos - base + j);            // the thread that writes it
                if (lane < 0 || lane >= SINC_TILE || seen[(size_t)(pos + j)]++) FAIL("%s: output %lld met twice or by lane %d", name, pos + j, lane);
            }
            // the direct kernel's per-thread step must land on the same track
            int td = track_of(tab, nt, ST_COLS, ST_OUT, base);
            while (td + 1 < nt && tab[(size_t)(td + 1) * ST_COLS + ST_OUT] <= pos) ++td;
            if (td != t) FAIL("%s: output %lld: direct track %d, staged track %d", name, pos, td, t);
            pos = seg_end;
            ++stretches;
        }
    }
    for (long long i = 0; i < total; ++i)
        if (seen[(size_t)i] != 1) FAIL("%s: output %lld met %d times", name, i, seen[(size_t)i]);
    free(tab);
    printf("%-22s %5d tracks, %lld outputs, %lld stretches, %lld track starts inside a tile ok\n", name, nt, total, stretches, mid_tile_starts);
    return 0;
}

static int check_filter(const char* name, long long o, long long n, long long width, long long run, bool want_staged) {
    if (sinc_filter_check(o, n, width, run) != SINC_OK) FAIL("%s: filter refused", name);
    if (sinc_staged(o, n, width) != want_staged) FAIL("%s: staged %d, want %d (span %lld)", name, (int)sinc_staged(o, n, width), (int)want_staged, sinc_max_span(o, n, width));
    const Filter F = make_filter(o, n, width, run);
    // the rule's span is reached by some alignment and never passed
    long long worst = 0;
    for (long long m0 = 0; m0 < 4 * n + 600; ++m0) {
        long long lo;
        const long long s = sinc_tile_span(m0, SINC_TILE, o, n, width, &lo);
        if (s > worst) worst = s;
    }
    if (worst != sinc_max_span(o, n, width)) FAIL("%s: largest span %lld, rule says %lld", name, worst, sinc_max_span(o, n, width));
    const long long per_tile = eval_ceil_div((long long)SINC_TILE * o, n);            // inputs per 256 outputs
    const long long lens[] = {1, 2, o > 1 ? o - 1 : 1, o, o + 1, per_tile - 1 > 0 ? per_tile - 1 : 1, per_tile, per_tile + 1, 2 * per_tile - 1,
                              2 * per_tile, 2 * per_tile + 1, 3 * per_tile + 7};
    for (long long n_in : lens)
        if (walk_single(name, F, n_in)) return 1;
    std::vector<long long> ragged = {1, per_tile + 1, 1, 1, 2, o, o + 1, 3 * per_tile, 1, per_tile / 2 + 1, 5};
    if (walk_tracks(name, F, ragged)) return 1;
    printf("%-22s o %lld n %lld width %lld run %lld: %s, span %lld floats ok\n", name, o, n, width, run, want_staged ? "staged" : "direct", worst);
    return 0;
}

static int check_refusals() {
    const long long huge = INT64_MAX;
    struct { long long o, n, w, run; int want; } f[] = {
        {147, 160, 68, 136, SINC_OK}, {0, 160, 68, 136, SINC_BAD_RATE}, {147, 0, 68, 136, SINC_BAD_RATE}, {147, -1, 68, 136, SINC_BAD_RATE},
        {147, 160, 0, 1, SINC_BAD_RATE}, {147, 160, 68, 0, SINC_BAD_RATE}, {147, 160, 68, 2 * 68 + 147 + 1, SINC_BAD_RATE},
        {147, 160, 68, 2 * 68 + 147, SINC_OK}, {SINC_MAX_RATE + 1, 1, 68, 2, SINC_BAD_RATE}, {1, SINC_MAX_RATE + 1, 68, 2, SINC_BAD_RATE},
        {1, 1, SINC_MAX_WIDTH + 1, 2, SINC_BAD_RATE}, {huge, huge, huge, huge, SINC_BAD_RATE},
        {SINC_MAX_RATE, SINC_MAX_RATE, 68, 33, SINC_TABLE}, {SINC_MAX_RATE, SINC_MAX_RATE, 68, 32, SINC_OK},
        {1, 1, SINC_MAX_WIDTH, SINC_MAX_TABLE_FLOATS, SINC_OK}, {1, 1, SINC_MAX_WIDTH, SINC_MAX_TABLE_FLOATS + 1, SINC_TABLE},
        {1, 2, SINC_MAX_WIDTH, SINC_MAX_TABLE_FLOATS / 2 + 1, SINC_TABLE},
    };
    for (const auto& c : f)
        if (sinc_filter_check(c.o, c.n, c.w, c.run) != c.want) FAIL("filter refusal (%lld, %lld, %lld, %lld): got %d, want %d", c.o, c.n, c.w, c.run, sinc_filter_check(c.o, c.n, c.w, c.run), c.want);
    const long long cap = SINC_MAX_TOTAL;
    struct { long long ch, n_in, n_out, o, n; int want; } s[] = {
        {2, 100, 109, 147, 160, SINC_OK}, {0, 100, 109, 147, 160, SINC_CHANNELS}, {65536, 100, 109, 147, 160, SINC_CHANNELS},
        {2, 0, 0, 147, 160, SINC_SHORT}, {2, -5, 0, 147, 160, SINC_SHORT}, {2, 100, 108, 147, 160, SINC_LENGTH}, {2, 100, 110, 147, 160, SINC_LENGTH},
        {2, huge, 1, 147, 160, SINC_OFFSET}, {2, (EVAL_MAX_OFF / 65536) + 1, 1, 1, 1, SINC_OFFSET}, {1, EVAL_MAX_OFF / SINC_MAX_RATE + 1, 1, 1, SINC_MAX_RATE, SINC_OFFSET},
        {1, cap, cap, 1, 1, SINC_OK}, {1, cap + 1, cap + 1, 1, 1, SINC_TOTAL}, {1, cap, 2 * cap, 1, 2, SINC_TOTAL}, {1, 100, 100, 0, 1, SINC_BAD_RATE},
    };
    for (const auto& c : s)
        if (sinc_single_check(c.ch, c.n_in, c.n_out, c.o, c.n) != c.want) FAIL("single refusal (%lld, %lld, %lld): got %d, want %d", c.ch, c.n_in, c.n_out, sinc_single_check(c.ch, c.n_in, c.n_out, c.o, c.n), c.want);
    long long row[ST_COLS] = {-1, -1, -1, -1}, out0 = 0;
    struct { long long off, n_in, o, n, out0; int want; } t[] = {
        {0, 100, 147, 160, 0, SINC_OK}, {0, 0, 147, 160, 0, SINC_SHORT}, {-1, 100, 147, 160, 0, SINC_OFFSET}, {huge, 100, 147, 160, 0, SINC_OFFSET},
        {EVAL_MAX_OFF + 1, 100, 147, 160, 0, SINC_OFFSET}, {0, huge, 147, 160, 0, SINC_OFFSET}, {0, 100, 147, 160, cap - 108, SINC_TOTAL},
        {0, 100, 147, 160, cap - 109, SINC_OK}, {0, 100, 147, 0, 0, SINC_BAD_RATE},
    };
    for (const auto& c : t) {
        out0 = c.out0;
        for (long long& v : row) v = -1;
        const int got = sinc_track_fill(c.off, c.n_in, c.o, c.n, &out0, row);
        if (got != c.want) FAIL("track refusal (%lld, %lld): got %d, want %d", c.off, c.n_in, got, c.want);
        if (got != SINC_OK && (out0 != c.out0 || row[0] != -1 || row[3] != -1)) FAIL("track refusal (%lld, %lld) wrote something", c.off, c.n_in);
        if (got == SINC_OK && (row[ST_OUT] != c.out0 || row[ST_N_OUT] != 109 || out0 != c.out0 + 109)) FAIL("track row");
    }
    if (sinc_tracks_check(0, 10) != SINC_SHORT || sinc_tracks_check(1, 0) != SINC_SHORT || sinc_tracks_check(11, 10) != SINC_LENGTH ||
        sinc_tracks_check(1, cap + 1) != SINC_TOTAL || sinc_tracks_check(1, cap) != SINC_OK || sinc_tracks_check(-1, huge) != SINC_SHORT)
        FAIL("tracks check");
    printf("refusals ok\n");
    return 0;
}

int main() {
    if (check_filter("44100 -> 48000 (64)", 147, 160, 68, 136, true)) return 1;
    if (check_filter("48000 -> 44100 (64)", 160, 147, 74, 148, true)) return 1;
    if (check_filter("48000 -> 32000 (64)", 3, 2, 102, 204, true)) return 1;
    if (check_filter("44100 -> 32000 (64)", 441, 320, 94, 187, true)) return 1;
    if (check_filter("44100 -> 16000 (6)", 441, 160, 17, 34, true)) return 1;
    if (check_filter("16000 -> 48000: o = 1", 1, 3, 7, 13, true)) return 1;
    if (check_filter("n above a tile", 8000, 8001, 7, 13, false)) return 1;
    if (check_filter("n of 257", 256, 257, 7, 14, true)) return 1;
    if (check_filter("n = 1: 96 to 1 (64)", 96, 1, 6502, 13006, false)) return 1;
    if (check_filter("n = 1: 4 to 1", 4, 1, 25, 50, true)) return 1;
    if (check_filter("full run", 5, 3, 4, 13, true)) return 1;
    {
        const Filter F = make_filter(147, 160, 68, 136);
        std::vector<long long> n_ins;
        for (int i = 0; i < 1000; ++i) n_ins.push_back(1 + urand(i % 7 == 0 ? 3 : 2000));
        if (walk_tracks("thousand tracks", F, n_ins)) return 1;
    }
    if (check_refusals()) return 1;
    printf("all walks pass\n");
    return 0;
}
