// Host walk of csrc/egr_null_index.h: the table rows, prefix columns and flat-index searches of egr_nullmany_delays,
// egr_nullmany_shift_fir and egr_nullmany_mix over ragged tables.  Meant to be built with a host compiler under the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/nullmany_host_check.cpp -o nullmany_host_check
// The tables are heap blocks of exactly n rows, filled by delays_fill / shiftfir_fill / mix_fill as the library fills them, so a search
// that leaves them is reported.  Every (pair, pack tile), (row, output tile) and (pair, chunk) must be met exactly once and in the
// sequential order; the tiles of a row must cover [0, n_out) and the chunks of a pair [0, n) without crossing into the next; the
// LDS window of a tile (its 256 + m - 1 staged samples) must map every (output, tap) term of k_shift_fir to one slot.  The transform
// length must follow the single rule (a total that IS a power of two stays), and the refusals (empty side, stride, max_shift, channel
// mismatch, taps row, offsets at the edge of int64, totals past one grid) must come back as codes without any overflow.
// Exit status 0 = all pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../comfyui-egregora-audio-super-resolution_amd/csrc/egr_null_index.h"

using namespace egr;

static uint64_t g_state = 0x13198A2E03707344ull;
static uint32_t urand(uint32_t n) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); fflush(stdout); return 1; } while (0)

static int check_lengths() {
    const long long want[][2] = {{1, 2}, {2, 4}, {3, 8}, {4, 8}, {5, 16}, {255, 512}, {256, 512}, {257, 1024}, {4096, 8192}, {4097, 16384},
                                 {(1LL << 30), (1LL << 31)}, {(1LL << 30) + 1, (1LL << 32)}};
    for (const auto& w : want)
        if (null_transform_length(w[0]) != w[1]) FAIL("transform length of %lld: %lld, want %lld", w[0], null_transform_length(w[0]), w[1]);
    for (int i = 0; i < 2000; ++i) {
        const long long nc = 1 + urand(1 << 20), n = null_transform_length(nc);
        long long ref = 1;
        while (ref < nc + nc) ref <<= 1;
        if (n != ref || n < 2 * nc || (n > 2 && n / 2 >= 2 * nc)) FAIL("transform length of %lld: %lld", nc, n);
    }
    printf("transform lengths ok\n");
    return 0;
}

static int walk_delays(const char* name, const std::vector<long long>& ncs, long long n) {
    const int np = (int)ncs.size();
    long long* tab = (long long*)malloc((size_t)np * ND_COLS * sizeof(long long));
    long long tiles = 0, off = 0;
    for (int p = 0; p < np; ++p) {
        const long long ca = 1 + p % 3, cb = 1 + (p / 3) % 2, lda = ncs[p] + p % 5, ldb = ncs[p] + 7 * (p % 2);
        const long long in[ND_COLS] = {off, ca, lda, off + ca * lda, cb, ldb, ncs[p], n / 2 - 2};
        off += ca * lda + cb * ldb;
        if (delays_fill(in, n, &tiles, tab + (size_t)p * ND_COLS) != NULL_OK) FAIL("%s: pair %d refused", name, p);
    }
    long long flat = 0;
    for (int p = 0; p < np; ++p) {
        long long covered = 0;
        for (long long t = 0; t < delays_tiles(n); ++t, ++flat) {
            long long first;
            const int gp = delays_tile_of(n, flat, &first);
            if (gp != p || first != covered) FAIL("%s: tile %lld -> pair %d from %lld, want pair %d from %lld", name, flat, gp, first, p, covered);
            covered += NULL_TILE;
        }
        if (covered < n || covered - n >= NULL_TILE) FAIL("%s: pair %d: tiles cover %lld of %lld", name, p, covered, n);
        if (tab[(size_t)p * ND_COLS + ND_N] != ncs[p] || tab[(size_t)p * ND_COLS + ND_MS] != n / 2 - 2) FAIL("%s: pair %d: row", name, p);
    }
    if (flat != tiles) FAIL("%s: walked %lld of %lld tiles", name, flat, tiles);
    free(tab);
    printf("%-16s %5d pairs at n = %lld: %lld pack tiles ok\n", name, np, n, tiles);
    return 0;
}

static int walk_shiftfir(const char* name, const std::vector<long long>& n_ins, const std::vector<long long>& n_outs, int m) {
    const int nr = (int)n_ins.size();
    long long* tab = (long long*)malloc((size_t)nr * SF_COLS * sizeof(long long));
    long long tiles = 0, in_off = 0, out_off = 0;
    for (int r = 0; r < nr; ++r) {
        const long long shift = (long long)urand(64) - 32;
        const long long in[SF_IN_COLS] = {in_off, n_ins[r], shift, r % 4 == 0 ? -1 : r % 3, out_off, n_outs[r]};
        in_off += n_ins[r] + r % 2;
        out_off += n_outs[r];
        if (shiftfir_fill(in, 3, &tiles, tab + (size_t)r * SF_COLS) != NULL_OK) FAIL("%s: row %d refused", name, r);
    }
    std::vector<float> stage((size_t)NULL_TILE + m);          // the LDS window of one tile: exactly 256 + m - 1 slots are legal
    long long flat = 0;
    const int off = (m - 1) / 2;
    for (int r = 0; r < nr; ++r) {
        long long covered = 0;
        const long long nt = eval_ceil_div(n_outs[r], NULL_TILE);
        for (long long t = 0; t < nt; ++t, ++flat) {
            long long first, len;
            const int gr = shiftfir_tile_of(tab, nr, flat, &first, &len);
            if (gr != r || first != covered || len < 1 || len > NULL_TILE || first + len > n_outs[r])
                FAIL("%s: tile %lld -> row %d [%lld, +%lld), want row %d from %lld", name, flat, gr, first, len, r, covered);
            covered += len;
            // every (output, tap) term of the tile lands inside the staged window at the slot the kernel reads
            const long long s0 = first + off - (m - 1);
            for (long long i = first; i < first + len; i += (len > 3 ? len - 1 : 1))
                for (int k = 0; k < m; k += (m > 3 ? m - 1 : 1)) {
                    const long long si = i + off - k, q = (i - first) + m - 1 - k;
                    if (q < 0 || q >= NULL_TILE + m - 1 || s0 + q != si) FAIL("%s: row %d tile %lld: slot %lld for sample %lld", name, r, t, q, si);
                    stage[(size_t)q] = 1.f;
                }
        }
        if (covered != n_outs[r]) FAIL("%s: row %d: tiles cover %lld of %lld", name, r, covered, n_outs[r]);
    }
    if (flat != tiles) FAIL("%s: walked %lld of %lld tiles", name, flat, tiles);
    free(tab);
    printf("%-16s %5d rows, %3d taps: %lld output tiles ok\n", name, nr, m, tiles);
    return 0;
}

static int walk_mix(const char* name, const std::vector<long long>& ns) {
    const int np = (int)ns.size();
    long long* tab = (long long*)malloc((size_t)np * NM_COLS * sizeof(long long));
    long long chunks = 0, off = 0, out = 0;
    for (int p = 0; p < np; ++p) {
        const long long ch = 1 + p % 3, lda = ns[p] + p % 5, ldb = ns[p] + 7 * (p % 2);
        const long long in[NM_IN_COLS] = {off, ch, lda, off + ch * lda, ch, ldb, ns[p], out};
        off += ch * (lda + ldb);
        out += ch * ns[p];
        if (mix_fill(in, &chunks, tab + (size_t)p * NM_COLS) != NULL_OK) FAIL("%s: pair %d refused", name, p);
    }
    long long flat = 0;
    for (int p = 0; p < np; ++p) {
        long long covered = 0;
        for (long long c = 0; c < mix_chunks(ns[p]); ++c, ++flat) {
            long long first, len;
            const int gp = mix_chunk_of(tab, np, flat, &first, &len);
            if (gp != p || first != covered || len < 1 || len > NULL_CHUNK || first + len > ns[p])
                FAIL("%s: chunk %lld -> pair %d [%lld, +%lld), want pair %d from %lld", name, flat, gp, first, len, p, covered);
            covered += len;
        }
        if (covered != ns[p]) FAIL("%s: pair %d: chunks cover %lld of %lld", name, p, covered, ns[p]);
    }
    if (flat != chunks) FAIL("%s: walked %lld of %lld chunks", name, flat, chunks);
    free(tab);
    printf("%-16s %5d pairs: %lld chunks ok\n", name, np, chunks);
    return 0;
}

static int check_refusals() {
    long long row[8], t = 0;
    const long long big = EVAL_MAX_OFF, huge = INT64_MAX;
    struct { long long in[ND_COLS]; long long n; int want; } d[] = {
        {{0, 1, 100, 100, 1, 100, 100, 50}, 256, NULL_OK},
        {{0, 1, 100, 100, 1, 100, 0, 50}, 256, NULL_SHORT},
        {{0, 1, 100, 100, 1, 100, -3, 50}, 256, NULL_SHORT},
        {{0, 1, 99, 100, 1, 100, 100, 50}, 256, NULL_BAD_ROW},
        {{0, 0, 100, 100, 1, 100, 100, 50}, 256, NULL_BAD_ROW},
        {{0, 1, 100, 100, 65536, 100, 100, 50}, 256, NULL_BAD_ROW},
        {{-1, 1, 100, 100, 1, 100, 100, 50}, 256, NULL_OFFSET},
        {{huge, 1, 100, 100, 1, 100, 100, 50}, 256, NULL_OFFSET},
        {{0, 1, huge, 100, 1, 100, 100, 50}, 256, NULL_OFFSET},
        {{0, 1, huge, 0, 1, huge, huge, 50}, 256, NULL_OFFSET},
        {{big, 1, 100, 100, 1, 100, 100, 50}, 256, NULL_OFFSET},
        {{0, 1, 128, 128, 1, 128, 128, 50}, 256, NULL_OK},            // 2 n_common IS the power of two: it stays
        {{0, 1, 129, 129, 1, 129, 129, 50}, 256, NULL_LENGTH},
        {{0, 1, 100, 100, 1, 100, 100, 50}, 512, NULL_LENGTH},
        {{0, 1, 100, 100, 1, 100, 100, 127}, 256, NULL_MAX_SHIFT},
        {{0, 1, 100, 100, 1, 100, 100, 126}, 256, NULL_OK},
        {{0, 1, 100, 100, 1, 100, 100, -1}, 256, NULL_MAX_SHIFT},
        {{0, 1, 100, 100, 1, 100, 100, huge}, 256, NULL_MAX_SHIFT},
    };
    for (const auto& c : d) {
        t = 0;
        if (delays_fill(c.in, c.n, &t, row) != c.want) FAIL("delays refusal: got %d, want %d", delays_fill(c.in, c.n, &t, row), c.want);
    }
    t = EVAL_MAX_GRID_256;
    if (delays_fill(d[0].in, 256, &t, row) != NULL_TOTAL) FAIL("delays: total past one grid not refused");
    t = EVAL_MAX_GRID_256 - 1;
    if (delays_fill(d[0].in, 256, &t, row) != NULL_OK || t != EVAL_MAX_GRID_256) FAIL("delays: the last tile of one grid refused");

    struct { long long in[SF_IN_COLS]; long long taps; int want; } s[] = {
        {{0, 100, 3, -1, 0, 100}, 0, NULL_OK},
        {{0, 100, 3, 0, 0, 100}, 0, NULL_TAPS},
        {{0, 100, 3, 2, 0, 100}, 2, NULL_TAPS},
        {{0, 100, 3, -2, 0, 100}, 2, NULL_TAPS},
        {{0, 0, 3, -1, 0, 100}, 0, NULL_SHORT},
        {{0, 100, 3, -1, 0, 0}, 0, NULL_SHORT},
        {{0, 1, -huge, -1, 0, 1}, 0, NULL_OFFSET},
        {{0, 1, huge, -1, 0, 1}, 0, NULL_OFFSET},
        {{huge, 1, 0, -1, 0, 1}, 0, NULL_OFFSET},
        {{0, 1, 0, -1, -5, 1}, 0, NULL_OFFSET},
        {{0, huge, 0, -1, 0, 1}, 0, NULL_OFFSET},
        {{0, 1, 0, -1, 0, 256 * (EVAL_MAX_GRID_256 + 1)}, 0, NULL_TOTAL},
        {{0, 1, 0, -1, 0, 256 * EVAL_MAX_GRID_256}, 0, NULL_OK},
    };
    for (const auto& c : s) {
        t = 0;
        if (shiftfir_fill(c.in, c.taps, &t, row) != c.want) FAIL("shift_fir refusal: got %d, want %d", shiftfir_fill(c.in, c.taps, &t, row), c.want);
    }
    struct { long long in[NM_IN_COLS]; int want; } m[] = {
        {{0, 2, 100, 200, 2, 100, 100, 0}, NULL_OK},
        {{0, 2, 100, 200, 1, 100, 100, 0}, NULL_CHANNELS},
        {{0, 2, 100, 200, 2, 100, 0, 0}, NULL_SHORT},
        {{0, 2, 99, 200, 2, 100, 100, 0}, NULL_BAD_ROW},
        {{0, 2, 100, 200, 2, 100, 100, -1}, NULL_OFFSET},
        {{0, 2, 100, huge, 2, 100, 100, 0}, NULL_OFFSET},
        {{0, 1, huge, 0, 1, huge, huge, 0}, NULL_OFFSET},
        {{0, 1, 4096 * (EVAL_MAX_GRID_256 + 1), 0, 1, 4096 * (EVAL_MAX_GRID_256 + 1), 4096 * (EVAL_MAX_GRID_256 + 1), 0}, NULL_TOTAL},
        {{0, 1, 4096 * EVAL_MAX_GRID_256, 0, 1, 4096 * EVAL_MAX_GRID_256, 4096 * EVAL_MAX_GRID_256, 0}, NULL_OK},
    };
    for (const auto& c : m) {
        t = 0;
        if (mix_fill(c.in, &t, row) != c.want) FAIL("mix refusal: got %d, want %d", mix_fill(c.in, &t, row), c.want);
    }
    printf("refusals ok\n");
    return 0;
}

int main() {
    if (check_lengths()) return 1;
    if (walk_delays("one pair", {300}, 1024)) return 1;
    if (walk_delays("edges of 512", {129, 130, 200, 255, 256}, 512)) return 1;
    if (walk_delays("short rows", {2, 2}, 4)) return 1;
    {
        std::vector<long long> ncs;
        for (int i = 0; i < 1000; ++i) ncs.push_back(2049 + urand(2048));
        if (walk_delays("thousand pairs", ncs, 8192)) return 1;
    }
    for (int m : {1, 16, 64, 255, NULL_MAX_TAPS}) {
        if (walk_shiftfir("tile edges", {1, 255, 256, 257, 300, 1, 9000}, {255, 256, 257, 1, 511, 513, 300}, m)) return 1;
    }
    {
        std::vector<long long> a, b;
        for (int i = 0; i < 1000; ++i) { a.push_back(1 + urand(5000)); b.push_back(1 + urand(5000)); }
        if (walk_shiftfir("thousand rows", a, b, 64)) return 1;
    }
    if (walk_mix("chunk edges", {1, 4095, 4096, 4097, 8192, 8193, 3})) return 1;
    {
        std::vector<long long> ns;
        for (int i = 0; i < 1000; ++i) ns.push_back(1 + urand(20000));
        if (walk_mix("thousand pairs", ns)) return 1;
    }
    if (check_refusals()) return 1;
    printf("all tables pass\n");
    return 0;
}
