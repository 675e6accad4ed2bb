// Host walk of the many-clip index code of csrc/egr_wpe_index.h (flat workgroup index -> clip and bin; flat frame tile / segment run ->
// clip, channel and place inside the channel) over ragged clip tables.  Meant to be built with a host compiler under the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/wpemany_host_check.cpp -o wpemany_host_check
// The prefix tables are heap blocks of exactly n + 1 entries, built as egr_wpemany_dereverb builds them (longest clip first, C equal
// stretches per clip), so a search that leaves them is reported.  Every (clip, bin) pair, every analysis tile and every synthesis run
// must be visited exactly once, and the flat order must be the sequential one: clip by clip, channel by channel, tile by tile.
// Tables: one-tile tracks, a one-frame clip, frame counts around the tile of 8, a single clip, and 1000 clips.  Exit status 0 = all pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../comfyui-egregora-audio-super-resolution_amd/csrc/egr_wpe_index.h"

using namespace egr;

static uint64_t g_state = 0x13198A2E03707344ull;
static uint32_t urand(uint32_t n) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

struct Table { const char* name; int C, bins, n_fft, hop; std::vector<long long> frames; };

// one prefix table and its walk; per(i) = workgroups one channel of clip i brings
template <class F> static int walk(const char* name, const char* what, const std::vector<long long>& fr, int C, F per) {
    const int n = (int)fr.size();
    long long* off = (long long*)malloc(((size_t)n + 1) * sizeof(long long));        // exactly n + 1 entries
    off[0] = 0;
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + C * per(fr[i]);
    const long long total = off[n];
    std::vector<unsigned char> seen((size_t)total, 0);
    int bad = 0;
    long long flat = 0;
    for (int i = 0; i < n && !bad; ++i)                                               // the sequential definition
        for (int c = 0; c < C && !bad; ++c)
            for (long long l = 0; l < per(fr[i]); ++l, ++flat) {
                int gi, gc;
                long long gl;
                wpe_many_track(off, n, C, flat, &gi, &gc, &gl);
                if (gi != i || gc != c || gl != l) {
                    printf("%s: %s %lld -> (%d, %d, %lld), want (%d, %d, %lld)\n", name, what, flat, gi, gc, gl, i, c, l);
                    bad = 1;
                    break;
                }
                seen[(size_t)(off[gi] + gc * per(fr[gi]) + gl)]++;
            }
    if (!bad && flat != total) { printf("%s: %s: walked %lld of %lld\n", name, what, flat, total); bad = 1; }
    for (long long t = 0; t < total && !bad; ++t)
        if (seen[(size_t)t] != 1) { printf("%s: %s %lld visited %d times\n", name, what, t, (int)seen[(size_t)t]); bad = 1; }
    free(off);
    return bad;
}

static int run(Table t) {
    std::stable_sort(t.frames.begin(), t.frames.end(), [](long long a, long long b) { return a > b; });      // longest first
    const int n = (int)t.frames.size();
    int bad = 0;
    // (clip, bin) pairs of k_wpe_iter_many
    std::vector<unsigned char> seen((size_t)n * t.bins, 0);
    for (long long idx = 0; idx < (long long)n * t.bins; ++idx) {
        int clip, bin;
        wpe_many_pair(idx, t.bins, &clip, &bin);
        if (clip < 0 || clip >= n || bin < 0 || bin >= t.bins || clip != idx / t.bins || bin != idx % t.bins) {
            printf("%s: pair %lld -> (%d, %d)\n", t.name, idx, clip, bin);
            return 1;
        }
        seen[(size_t)clip * t.bins + bin]++;
    }
    for (unsigned char v : seen) bad |= v != 1;
    if (bad) { printf("%s: a (clip, bin) pair is not visited exactly once\n", t.name); return 1; }
    bad |= walk(t.name, "stft tile", t.frames, t.C, [](long long f) { return wpe_stft_tiles(f); });
    bad |= walk(t.name, "istft run", t.frames, t.C, [&](long long f) { return wpe_istft_runs(f, t.n_fft, t.hop); });
    printf("%-14s %5d clips x %d ch, %4d bins: %s\n", t.name, n, t.C, t.bins, bad ? "FAIL" : "ok");
    return bad;
}

int main() {
    std::vector<Table> tabs;
    tabs.push_back({"single", 2, 129, 256, 64, {504}});
    tabs.push_back({"one-frame", 1, 33, 64, 16, {1}});
    tabs.push_back({"one-tile", 3, 33, 64, 16, {8, 8, 1, 8, 5, 8}});
    tabs.push_back({"around-tiles", 1, 33, 64, 16, {1, 3, 4, 7, 8, 9, 63, 64, 65, 1003, 16, 17}});
    tabs.push_back({"half-overlap", 2, 513, 1024, 512, {2, 40, 9, 8, 377}});
    Table big{"thousand", 2, 33, 64, 16, {}};
    for (int i = 0; i < 1000; ++i) big.frames.push_back(1 + urand(300));
    tabs.push_back(big);
    Table wide{"thousand-wide", 64, 513, 1024, 256, {}};
    for (int i = 0; i < 1000; ++i) wide.frames.push_back(1 + urand(40));
    tabs.push_back(wide);
    int bad = 0;
    for (const Table& t : tabs) bad |= run(t);
    if (bad) return 1;
    printf("all tables pass\n");
    return 0;
}
