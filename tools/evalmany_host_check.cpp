// Host walk of csrc/egr_eval_index.h: the table rows, prefix columns and flat-index searches of egr_metrics_pairs and egr_loudness_tracks
// over ragged tables.  Meant to be built with a host compiler under the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/evalmany_host_check.cpp -o evalmany_host_check
// The tables are heap blocks of exactly n rows, filled by metrics_fill / loud_fill as the library fills them, so a search that leaves
// them is reported.  Every (pair, frame), (pair, chunk), (clip, thread chunk), (clip, block) and (clip, peak tile) must be met exactly
// once and in the sequential order; a frame past the first must lie inside its pair; the chunks of a pair must tile [0, n) without
// crossing into the next pair.  The refusals (n < 1, bad channels or stride, offsets at the edge of int64, totals past what one grid of
// the consuming kernel's block size can launch: workgroups x threads < 2^32) must come
// back as codes without any overflow.  Tables: the edge lengths of the frame rule and of the chunking, one pair, and 1000 random rows.
// walk_shared walks the two functions of csrc/egr_ragged_index.h that every ragged header builds on: track_of against a linear scan
// (ascending columns of 1, 2, 3 and 1000 rows, row strides 1 and 8, every query from 0 to past the last entry) and tile_of against the
// written-out rule of each of its three callers (metrics chunks, shift-FIR tiles, mix chunks) on rows whose last tile is full, holds
// one sample, or follows a full one by one sample.
// Exit status 0 = all pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../comfyui-egregora-audio-super-resolution_amd/csrc/egr_eval_index.h"
#include "../comfyui-egregora-audio-super-resolution_amd/csrc/egr_null_index.h"

using namespace egr;

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint32_t urand(uint32_t n) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

static int walk_pairs(const char* name, const std::vector<long long>& ns, int n_fft, int hop) {
    const int n = (int)ns.size();
    long long* tab = (long long*)malloc((size_t)n * MP_COLS * sizeof(long long));       // exactly n rows
    long long frames = 0, chunks = 0, off = 0;
    for (int p = 0; p < n; ++p) {
        const long long ca = 1 + p % 3, cb = 1 + (p / 3) % 2, lda = ns[p] + p % 5, ldb = ns[p] + 7 * (p % 2);
        const long long in[MP_IN_COLS] = {off, ca, lda, off + ca * lda, cb, ldb, ns[p]};
        off += ca * lda + cb * ldb;
        if (metrics_fill(in, n_fft, hop, &frames, &chunks, tab + (size_t)p * MP_COLS) != EVAL_OK) FAIL("%s: pair %d refused", name, p);
    }
    long long flat = 0;
    for (int p = 0; p < n; ++p) {
        const long long* e = tab + (size_t)p * MP_COLS;
        const long long fr = e[MP_FRAMES];
        if (fr != 1 + (ns[p] > n_fft ? (ns[p] - n_fft) / hop : 0)) FAIL("%s: pair %d: %lld frames", name, p, fr);
        const long long lo = (long long)(0.95 * (double)(fr - 1));
        if (e[MP_KLO] != lo || e[MP_KHI] != (lo + 1 < fr ? lo + 1 : fr - 1) || e[MP_KLO] < 0 || e[MP_KHI] >= fr) FAIL("%s: pair %d: ranks", name, p);
        for (long long f = 0; f < fr; ++f, ++flat) {
            long long gf;
            const int gp = metrics_frame_of(tab, n, flat, &gf);
            if (gp != p || gf != f) FAIL("%s: frame %lld -> (%d, %lld), want (%d, %lld)", name, flat, gp, gf, p, f);
            if (f > 0 && f * hop + n_fft > ns[p]) FAIL("%s: pair %d frame %lld leaves the pair", name, p, f);
        }
    }
    if (flat != frames) FAIL("%s: walked %lld of %lld frames", name, flat, frames);
    flat = 0;
    for (int p = 0; p < n; ++p) {
        long long covered = 0;
        for (long long c = 0; c < metrics_chunks(ns[p]); ++c, ++flat) {
            long long first, len;
            const int gp = metrics_chunk_of(tab, n, flat, &first, &len);
            if (gp != p || first != covered || len < 1 || len > EGR_METRICS_CHUNK || first + len > ns[p])
                FAIL("%s: chunk %lld -> pair %d [%lld, +%lld), want pair %d from %lld", name, flat, gp, first, len, p, covered);
            covered += len;
        }
        if (covered != ns[p]) FAIL("%s: pair %d: chunks cover %lld of %lld", name, p, covered, ns[p]);
    }
    if (flat != chunks) FAIL("%s: walked %lld of %lld chunks", name, flat, chunks);
    free(tab);
    printf("%-16s %5d pairs, n_fft %4d hop %4d: %lld frames, %lld chunks ok\n", name, n, n_fft, hop, frames, chunks);
    return 0;
}

static int walk_clips(const char* name, const std::vector<long long>& ns, int C, int L, long long blk_a, long long hop_a, long long blk_b,
                      long long hop_b, int up) {
    const int n = (int)ns.size();
    long long* tab = (long long*)malloc((size_t)n * LT_COLS * sizeof(long long));
    LoudTotals t = {0, 0, 0, 0, 0};
    long long off = 0;
    for (int c = 0; c < n; ++c) {
        const long long in[LT_IN_COLS] = {off, ns[c]};
        off += C * ns[c] + c % 3;
        if (loud_fill(in, C, L, blk_a, hop_a, blk_b, hop_b, up, &t, tab + (size_t)c * LT_COLS) != EVAL_OK) FAIL("%s: clip %d refused", name, c);
    }
    struct Col { int col; long long total; const char* what; };
    const Col cols[4] = {{LT_CHUNK0, t.chunks, "thread chunk"}, {LT_FA0, t.fa, "block a"}, {LT_FB0, t.fb, "block b"}, {LT_TILE0, t.tiles, "tile"}};
    for (const Col& k : cols) {
        if (k.total == 0) continue;
        long long flat = 0;
        for (int c = 0; c < n; ++c) {
            const long long nn = ns[c];
            const long long cnt = k.col == LT_CHUNK0 ? (nn + L - 1) / L : k.col == LT_FA0 ? eval_frames(nn, blk_a, hop_a)
                                : k.col == LT_FB0 ? eval_frames(nn, blk_b, hop_b) : (nn * up + LT_TILE - 1) / LT_TILE;
            for (long long j = 0; j < cnt; ++j, ++flat) {
                long long gj;
                const int gc = loud_item_of(tab, n, k.col, flat, &gj);
                if (gc != c || gj != j) FAIL("%s: %s %lld -> (%d, %lld), want (%d, %lld)", name, k.what, flat, gc, gj, c, j);
                if (k.col == LT_CHUNK0 && j * L >= nn) FAIL("%s: clip %d chunk %lld starts past the clip", name, c, j);
                if ((k.col == LT_FA0 || k.col == LT_FB0) && j * (k.col == LT_FA0 ? hop_a : hop_b) >= nn) FAIL("%s: clip %d block %lld is empty", name, c, j);
                if (k.col == LT_TILE0 && j * LT_TILE >= nn * up) FAIL("%s: clip %d tile %lld is empty", name, c, j);
            }
        }
        if (flat != k.total) FAIL("%s: %s: walked %lld of %lld", name, k.what, flat, k.total);
    }
    long long mono = 0;
    for (int c = 0; c < n; ++c) {
        if (tab[(size_t)c * LT_COLS + LT_MONO] != mono) FAIL("%s: clip %d: mono offset", name, c);
        mono += ns[c];
    }
    free(tab);
    printf("%-16s %5d clips x %d ch, L %3d: %lld chunks, %lld + %lld blocks, %lld tiles ok\n", name, n, C, L, t.chunks, t.fa, t.fb, t.tiles);
    return 0;
}

static int refusals() {
    long long row[MP_COLS], f0 = 0, c0 = 0;
    const long long big = INT64_MAX;
    struct Case { const char* why; long long in[MP_IN_COLS]; int want; };
    const Case cases[] = {
        {"n = 0", {0, 1, 10, 0, 1, 10, 0}, EVAL_SHORT},
        {"n < 0", {0, 1, 10, 0, 1, 10, -5}, EVAL_SHORT},
        {"no channels", {0, 0, 10, 0, 1, 10, 10}, EVAL_BAD_ROW},
        {"too many channels", {0, 1, 10, 0, 65536, 10, 10}, EVAL_BAD_ROW},
        {"stride below n", {0, 1, 9, 0, 1, 10, 10}, EVAL_BAD_ROW},
        {"negative offset", {-1, 1, 10, 0, 1, 10, 10}, EVAL_OFFSET},
        {"offset at the edge", {0, 1, 10, big, 2, 10, 10}, EVAL_OFFSET},
        {"stride at the edge", {0, 2, big, 0, 1, 10, 10}, EVAL_OFFSET},
        {"n at the edge", {0, 1, big, 0, 1, big, big}, EVAL_OFFSET},
    };
    for (const Case& c : cases) {
        const int got = metrics_fill(c.in, 512, 64, &f0, &c0, row);
        if (got != c.want || f0 != 0 || c0 != 0) FAIL("refusal '%s': code %d, want %d", c.why, got, c.want);
    }
    const long long ok[MP_IN_COLS] = {0, 1, 100000, 100000, 1, 100000, 100000};
    f0 = EVAL_MAX_GRID_256 - 10; c0 = 0;
    if (metrics_fill(ok, 512, 64, &f0, &c0, row) != EVAL_TOTAL || f0 != EVAL_MAX_GRID_256 - 10) FAIL("refusal 'frame total'");
    f0 = 0; c0 = EVAL_MAX_GRID_256 - 3;
    if (metrics_fill(ok, 512, 64, &f0, &c0, row) != EVAL_TOTAL) FAIL("refusal 'chunk total'");
    f0 = EVAL_MAX_GRID_256 - eval_frames(100000, 512, 64); c0 = 0;
    if (metrics_fill(ok, 512, 64, &f0, &c0, row) != EVAL_OK || f0 != EVAL_MAX_GRID_256) FAIL("the last frame of one grid is refused");
    f0 = EVAL_MAX_GRID_256 - eval_frames(100000, 512, 64) + 1; c0 = 0;
    if (metrics_fill(ok, 512, 64, &f0, &c0, row) != EVAL_TOTAL) FAIL("one frame past one grid is accepted");
    static_assert(EVAL_MAX_GRID_256 == 16777215 && EVAL_MAX_PAIRS == 4194303 && EVAL_MAX_KW_CHUNKS == 64LL * 67108863, "caps follow from 2^32 work-items");
    static_assert((EVAL_MAX_GRID_256 + 1) * 256 > EVAL_MAX_WORK_ITEMS && EVAL_MAX_GRID_256 * 256 <= EVAL_MAX_WORK_ITEMS, "256-thread cap");
    static_assert((EVAL_MAX_PAIRS + 1) * 1024 > EVAL_MAX_WORK_ITEMS && EVAL_MAX_PAIRS * 1024 <= EVAL_MAX_WORK_ITEMS, "1024-thread cap");
    long long lrow[LT_COLS];
    LoudTotals t = {0, 0, 0, 0, 0};
    const long long l0[2] = {0, 0}, l1[2] = {-4, 100}, l2[2] = {big, 100}, l3[2] = {0, big}, l4[2] = {0, 100000};
    if (loud_fill(l0, 2, 22, 3200, 800, 24000, 8000, 4, &t, lrow) != EVAL_SHORT) FAIL("loud refusal n = 0");
    if (loud_fill(l1, 2, 22, 3200, 800, 24000, 8000, 4, &t, lrow) != EVAL_OFFSET) FAIL("loud refusal negative offset");
    if (loud_fill(l2, 2, 22, 3200, 800, 24000, 8000, 4, &t, lrow) != EVAL_OFFSET) FAIL("loud refusal offset at the edge");
    if (loud_fill(l3, 2, 22, 3200, 800, 24000, 8000, 4, &t, lrow) != EVAL_OFFSET) FAIL("loud refusal n at the edge");
    if (loud_fill(l4, 0, 22, 3200, 800, 24000, 8000, 4, &t, lrow) != EVAL_OFFSET) FAIL("loud refusal no channels");
    t.tiles = EVAL_MAX_GRID_256 - 5;
    if (loud_fill(l4, 2, 22, 3200, 800, 24000, 8000, 4, &t, lrow) != EVAL_TOTAL || t.chunks != 0) FAIL("loud refusal tile total");
    t = {0, 0, 0, 0, 0};
    t.tiles = EVAL_MAX_GRID_256 - (100000LL * 4 + LT_TILE - 1) / LT_TILE;
    if (loud_fill(l4, 2, 22, 3200, 800, 24000, 8000, 4, &t, lrow) != EVAL_OK || t.tiles != EVAL_MAX_GRID_256) FAIL("the last tile of one grid is refused");
    t = {0, 0, 0, 0, 0};
    t.fa = EVAL_MAX_GRID_256 - eval_frames(100000, 3200, 800) + 1;
    if (loud_fill(l4, 2, 22, 3200, 800, 24000, 8000, 4, &t, lrow) != EVAL_TOTAL) FAIL("loud refusal block total");
    t = {0, 0, 0, 0, 0};
    t.chunks = EVAL_MAX_KW_CHUNKS - (100000 + 21) / 22 + 1;
    if (loud_fill(l4, 2, 22, 3200, 800, 24000, 8000, 4, &t, lrow) != EVAL_TOTAL) FAIL("loud refusal thread chunk total");
    printf("refusals ok\n");
    return 0;
}

// the search as a scan: the last t with tab[t * stride + col] <= i
static int scan_of(const long long* tab, int n, int stride, int col, long long i) {
    int t = 0;
    for (int k = 1; k < n; ++k)
        if (tab[(size_t)k * stride + col] <= i) t = k;
    return t;
}

static int walk_shared() {
    // track_of: heap tables of exactly n rows; the searched column ascends strictly from 0 (every caller's rows hold at least one tile
    // or sample), the other columns descend so that a read of the wrong column shows
    for (int n : {1, 2, 3, 1000})
        for (int stride : {1, 8}) {
            const int col = stride == 1 ? 0 : 5;
            long long* tab = (long long*)malloc((size_t)n * stride * sizeof(long long));
            long long at = 0;
            for (int t = 0; t < n; ++t) {
                for (int c = 0; c < stride; ++c) tab[(size_t)t * stride + c] = 1000000 - t;
                tab[(size_t)t * stride + col] = at;
                at += 1 + urand(n == 1000 ? 40 : 3);
            }
            for (long long i = 0; i < at + 5; ++i) {
                const int got = track_of(tab, n, stride, col, i), want = scan_of(tab, n, stride, col, i);
                if (got != want) FAIL("track_of: %d rows, stride %d: %lld -> %d, want %d", n, stride, i, got, want);
            }
            free(tab);
        }
    // tile_of against the rule each caller wrote out before it: row by scan, first = (flat - first tile) tile, len = min(left, tile)
    struct Rule { const char* who; int cols, col_first, col_len, tile; };
    const Rule rules[3] = {{"metrics_chunk_of", MP_COLS, MP_CHUNK0, MP_N, EGR_METRICS_CHUNK}, {"shiftfir_tile_of", SF_COLS, SF_TILE0, SF_N_OUT, NULL_TILE},
                           {"mix_chunk_of", NM_COLS, NM_CHUNK0, NM_N, NULL_CHUNK}};
    for (const Rule& r : rules) {
        const long long T = r.tile, lens[] = {T, T + 1, 1, 2 * T, 1, 3 * T + 1, T - 1, T};      // last tiles of T, 1, 1, T, 1, 1, T - 1, T samples
        const int n = (int)(sizeof(lens) / sizeof(lens[0]));
        long long* tab = (long long*)malloc((size_t)n * r.cols * sizeof(long long));
        long long tiles = 0;
        for (int t = 0; t < n; ++t) {
            for (int c = 0; c < r.cols; ++c) tab[(size_t)t * r.cols + c] = -7;
            tab[(size_t)t * r.cols + r.col_first] = tiles;
            tab[(size_t)t * r.cols + r.col_len] = lens[t];
            tiles += (lens[t] + T - 1) / T;
        }
        for (long long flat = 0; flat < tiles; ++flat) {
            const int want = scan_of(tab, n, r.cols, r.col_first, flat);
            const long long* e = tab + (size_t)want * r.cols;
            const long long wfirst = (flat - e[r.col_first]) * T, left = e[r.col_len] - wfirst, wlen = left < T ? left : T;
            long long first = -1, len = -1, f2 = -1, l2 = -1;
            const int got = tile_of(tab, n, r.cols, r.col_first, r.col_len, r.tile, flat, &first, &len);
            const int named = r.cols == MP_COLS && r.col_first == MP_CHUNK0 ? metrics_chunk_of(tab, n, flat, &f2, &l2)
                            : r.col_first == SF_TILE0 ? shiftfir_tile_of(tab, n, flat, &f2, &l2) : mix_chunk_of(tab, n, flat, &f2, &l2);
            if (got != want || first != wfirst || len != wlen || wlen < 1)
                FAIL("tile_of as %s: tile %lld -> row %d [%lld, +%lld), want row %d [%lld, +%lld)", r.who, flat, got, first, len, want, wfirst, wlen);
            if (named != want || f2 != wfirst || l2 != wlen) FAIL("%s: tile %lld -> row %d [%lld, +%lld)", r.who, flat, named, f2, l2);
            const bool last = flat + 1 == tiles || tab[(size_t)(want + 1) * r.cols + r.col_first] == flat + 1;
            if (last ? wfirst + wlen != lens[want] : wlen != T) FAIL("%s: tile %lld of row %d holds %lld samples", r.who, flat, want, wlen);
        }
        free(tab);
    }
    printf("track_of and tile_of ok\n");
    return 0;
}

int main() {
    const long long CH = EGR_METRICS_CHUNK;
    int bad = walk_shared();
    bad |= walk_pairs("frame-rule", {1, 511, 512, 512 + 63, 512 + 64, 512 + 65, 5000}, 512, 64);
    bad |= walk_pairs("chunk-rule", {CH - 1, CH, CH + 1, 2 * CH + 3, 1, 3 * CH}, 512, 64);
    bad |= walk_pairs("single", {60000}, 2048, 512);
    bad |= walk_pairs("n_fft-8192", {8191, 8192, 8192 + 2048 * 2, 3}, 8192, 2048);
    bad |= walk_pairs("hop-1", {700, 513}, 512, 1);
    std::vector<long long> ns;
    for (int i = 0; i < 1000; ++i) ns.push_back(1 + urand(30000));
    bad |= walk_pairs("thousand", ns, 512, 128);
    // loudness: 8 kHz (L = 22 for k = exp(-2 pi 60 / 4000)) and 16 kHz shapes; lengths around a thread chunk, a workgroup's 64 chunks, the blocks
    for (int L : {22, 43}) {
        const long long l = L;
        bad |= walk_clips("around-chunks", {1, l - 1, l, l + 1, 64 * l - 1, 64 * l, 64 * l + 1, 3199, 3200, 3201, 4000, 23999, 24000, 24001, 32000}, 2,
                          L, 3200, 800, 24000, 8000, 4);
    }
    bad |= walk_clips("no-short-term", {1, 100, 6400}, 5, 43, 6400, 1600, 0, 0, 0);
    bad |= walk_clips("peak-only-up1", {1, 255, 256, 257, 9000}, 1, 22, 3200, 800, 0, 0, 1);
    std::vector<long long> cl;
    for (int i = 0; i < 1000; ++i) cl.push_back(1 + urand(50000));
    bad |= walk_clips("thousand", cl, 2, 22, 3200, 800, 24000, 8000, 4);
    bad |= refusals();
    if (bad) return 1;
    printf("all tables pass\n");
    return 0;
}
