// Host walk of k_wpe_iter's index and accumulation code (csrc/egr_wpe_index.h) against the sequential definition of SPEC.md WPE-P4.
// Meant to be built with a host compiler under -fsanitize=address,undefined:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/wpe_host_check.cpp -o wpe_host_check
// Every tile is a heap block of exactly the kernel's size, so an index outside it is reported; block ownership is checked to cover
// the needed part of [Ytilde ; Y] diag(inv) Ytilde^H exactly once.  Shapes: the frame counts, channels, taps and delays of the
// cases A-E of tests/wpe_cases.py, an input with fewer frames than K, a two-blocks-per-thread shape, and the wide cases F, H, L
// (32 channels x 2 taps; 40 channels on the 32-frame tile; 64 channels at delay 122, the longest history that fits).  Exit status 0 = all pass.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../comfyui-egregora-audio-super-resolution_amd/csrc/egr_wpe_index.h"

using namespace egr;

static uint64_t g_state = 0x243F6A8885A308D3ull;
static double urand() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0 - 0.5;
}

struct Shape { const char* name; int D, T, taps, delay; };

static int run(const Shape& s) {
    const WpeGeom g = wpe_geom(s.D, s.taps, s.delay);
    const int D = s.D, T = s.T, K = g.K, M = g.M;
    std::vector<wpe_c32> Y((size_t)D * T);
    std::vector<double> inv((size_t)T);
    for (auto& v : Y) { v.x = (float)urand(); v.y = (float)urand(); }
    for (auto& v : inv) v = 1.0 / (0.01 + fabs(urand()));
    auto stacked = [&](int r, int t, double* re, double* im) {      // row r of [Ytilde ; Y] at frame t, from the definition
        int d, tt;
        if (r < K) { const int k = r / D; d = r % D; tt = t - s.delay - k; } else { d = r - K; tt = t; }
        if (tt < 0) { *re = 0; *im = 0; return; }
        *re = Y[(size_t)d * T + tt].x; *im = Y[(size_t)d * T + tt].y;
    };
    // ---- the kernel's walk
    std::vector<double> Ar((size_t)M * K, 0.0), Ai((size_t)M * K, 0.0);
    std::vector<int> owners((size_t)M * K, 0);
    const int NB = (g.nblocks + WPE_THREADS - 1) / WPE_THREADS;
    if (NB > 2) { printf("%s: %d blocks need more than two per thread\n", s.name, g.nblocks); return 1; }
    for (int tid = 0; tid < WPE_THREADS; ++tid)
        for (int n = 0; n < NB; ++n) {
            const int b = tid + n * WPE_THREADS;
            if (b >= g.nblocks) continue;
            int bi, bj;
            wpe_block(g, b, &bi, &bj);
            int rb[4], cb[4];
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * bi + i < M - 1 ? 4 * bi + i : M - 1, c = 4 * bj + i < K - 1 ? 4 * bj + i : K - 1;
                rb[i] = wpe_row_base(g, r);
                cb[i] = wpe_row_base(g, c);
            }
            double ar[16] = {0}, ai[16] = {0};
            for (int t0 = 0; t0 < T; t0 += g.TT) {
                wpe_c32* tile = (wpe_c32*)malloc((size_t)D * g.LDT * sizeof(wpe_c32));     // exact size: the sanitizer sees any overrun
                double* invt = (double*)malloc((size_t)g.TT * sizeof(double));
                for (int e = 0; e < D * g.LDT; ++e) {
                    int d, t;
                    wpe_tile_src(g, e, t0, &d, &t);
                    if (t >= 0 && t < T) tile[e] = Y[(size_t)d * T + t]; else { tile[e].x = 0.f; tile[e].y = 0.f; }
                }
                for (int e = 0; e < g.TT; ++e) invt[e] = t0 + e < T ? inv[t0 + e] : 0.0;
                const int nt = g.TT < T - t0 ? g.TT : T - t0;
                wpe_acc_block(tile, invt, nt, rb, cb, ar, ai);
                free(tile);
                free(invt);
            }
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    const int r = 4 * bi + i, c = 4 * bj + j;
                    if (r < M && c < K) {
                        Ar[(size_t)r * K + c] = ar[i * 4 + j];
                        Ai[(size_t)r * K + c] = ai[i * 4 + j];
                        owners[(size_t)r * K + c]++;
                    }
                }
        }
    // ---- the definition, and the comparison over the needed part (lower triangle of R, all of P^H)
    double err2 = 0.0, ref2 = 0.0;
    int bad_owner = 0;
    for (int r = 0; r < M; ++r)
        for (int c = 0; c < K; ++c) {
            const bool needed = r >= K || c <= r;
            if (owners[(size_t)r * K + c] > 1 || (needed && owners[(size_t)r * K + c] != 1)) ++bad_owner;
            if (!needed) continue;
            double sr = 0.0, si = 0.0;
            for (int t = 0; t < T; ++t) {
                double a, b, cr, ci;
                stacked(r, t, &a, &b);
                stacked(c, t, &cr, &ci);
                sr += inv[t] * (a * cr + b * ci);
                si += inv[t] * (b * cr - a * ci);
            }
            const double dr = sr - Ar[(size_t)r * K + c], di = si - Ai[(size_t)r * K + c];
            err2 += dr * dr + di * di;
            ref2 += sr * sr + si * si;
        }
    // ---- sweep 2: wpe_filter_sum (X = Y - GH Ytilde through the tile, compensated) against the definition in plain double, random GH
    std::vector<wpe_c64> gh((size_t)D * K);
    for (auto& v : gh) { v.x = urand(); v.y = urand(); }
    double xerr = 0.0;
    for (int t0 = 0; t0 < T; t0 += g.TT) {
        wpe_c32* tile = (wpe_c32*)malloc((size_t)D * g.LDT * sizeof(wpe_c32));
        for (int e = 0; e < D * g.LDT; ++e) {
            int d, t;
            wpe_tile_src(g, e, t0, &d, &t);
            if (t >= 0 && t < T) tile[e] = Y[(size_t)d * T + t]; else { tile[e].x = 0.f; tile[e].y = 0.f; }
        }
        const int nt = g.TT < T - t0 ? g.TT : T - t0;
        for (int idx = 0; idx < D * g.TT; ++idx) {
            const int e = idx / g.TT, tl = idx - e * g.TT;
            if (tl >= nt) continue;
            wpe_c64* row = (wpe_c64*)malloc((size_t)K * sizeof(wpe_c64));                   // row e of GH at its exact size
            for (int i = 0; i < K; ++i) row[i] = gh[(size_t)e * K + i];
            double sr, si;
            wpe_filter_sum(g, tile, row, e, tl, &sr, &si);                                  // the kernel's own sweep-2 code
            free(row);
            double wr, wi;
            stacked(K + e, t0 + tl, &wr, &wi);
            for (int r = 0; r < K; ++r) {
                double a, b;
                stacked(r, t0 + tl, &a, &b);
                wr -= gh[(size_t)e * K + r].x * a - gh[(size_t)e * K + r].y * b;
                wi -= gh[(size_t)e * K + r].x * b + gh[(size_t)e * K + r].y * a;
            }
            const double d2 = fabs(wr - sr) + fabs(wi - si);
            if (d2 > xerr) xerr = d2;
        }
        free(tile);
    }
    const double rel = ref2 > 0 ? sqrt(err2 / ref2) : sqrt(err2);
    const bool ok = bad_owner == 0 && rel <= 1e-14 && xerr <= 1e-12;
    printf("%-10s D=%2d T=%4d taps=%2d delay=%2d K=%2d blocks=%3d (x%d)  ownership errors %d  statistics rel %.2e  filter max abs %.2e  %s\n",
           s.name, D, T, s.taps, s.delay, K, g.nblocks, NB, bad_owner, rel, xerr, ok ? "ok" : "FAIL");
    return ok ? 0 : 1;
}

int main() {
    const Shape shapes[] = {
        {"A", 1, 253, 3, 1}, {"B", 3, 503, 5, 2}, {"C", 2, 503, 10, 3}, {"D", 2, 753, 32, 1}, {"E", 2, 337, 10, 3},
        {"frames<K", 1, 8, 10, 3}, {"one-frame", 2, 1, 3, 1}, {"K=15", 5, 130, 3, 16}, {"two-blocks", 64, 70, 1, 1}, {"K=63", 21, 65, 3, 2},
        {"F", 32, 753, 2, 1}, {"H", 40, 503, 1, 1}, {"L", 64, 753, 1, 122},
    };
    int bad = 0;
    for (const Shape& s : shapes) bad += run(s);
    printf(bad ? "FAILED: %d shapes\n" : "all shapes pass\n", bad);
    return bad ? 1 : 0;
}
