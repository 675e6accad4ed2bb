// Index, accumulation and filter code of k_wpe_iter (egr_wpe.hip), kept free of device-only constructs so that the same text compiles for the
// host: tools/wpe_host_check.cpp walks it thread by thread under -fsanitize=address,undefined against the sequential definition.
// The index code of the many-clip kernels (flat index -> clip and bin, flat tile -> track) is at the end; tools/wpemany_host_check.cpp walks it.
//
// One bin's statistics are the lower-left part of  Z diag(inv) Z^H,  Z = [Ytilde (K rows) ; Y (D rows)],  M = K + D rows, K columns:
//   rows r < K, columns c <= r :  R[r][c] = sum_t inv[t] Ytilde_r[t] conj(Ytilde_c[t])          (lower triangle of R)
//   rows K + e, columns c      :  conj(P[c][e]) = sum_t inv[t] Y_e[t] conj(Ytilde_c[t])          (P^H)
// Stacked row i = k D + d is channel d delayed by delay + k frames.  The part is cut into 4 x 4 blocks; thread tid owns blocks
// tid, tid + 256, ... and keeps their 16 complex-double sums in registers over the whole frame sweep.
#pragma once

#include "egr_ragged_index.h"

#if defined(__HIPCC__)
typedef float2 wpe_c32;
typedef double2 wpe_c64;
#else
#include <math.h>
struct wpe_c32 { float x, y; };
struct wpe_c64 { double x, y; };
#endif

namespace egr {

constexpr int WPE_THREADS = 256;
constexpr int WPE_MAX_K = 64;
constexpr int WPE_MAX_HIST = 128;   // delay + taps - 1
constexpr int WPE_FT = 8;           // frames per workgroup of k_wpe_stft: 64-byte store runs
constexpr int WPE_SEG = 8;          // hop-long output segments per workgroup of k_wpe_istft

struct WpeGeom {
    int D, taps, delay;
    int K, M;          // stacked rows, stacked + observed rows
    int H;             // frames of history in front of a tile: delay + taps - 1
    int TT, LDT;       // frames per tile; tile row length H + TT
    int nbk, nbm;      // 4-row blocks covering K and M
    int tri, nblocks;  // blocks in the triangle over the first nbk block rows; all blocks
};

EGR_HD WpeGeom wpe_geom(int D, int taps, int delay) {
    WpeGeom g;
    g.D = D; g.taps = taps; g.delay = delay;
    g.K = D * taps;
    g.M = g.K + D;
    g.H = delay + taps - 1;
    g.TT = D > 32 ? 32 : 64;
    g.LDT = g.H + g.TT;
    g.nbk = (g.K + 3) / 4;
    g.nbm = (g.M + 3) / 4;
    g.tri = g.nbk * (g.nbk + 1) / 2;
    g.nblocks = g.tri + (g.nbm - g.nbk) * g.nbk;
    return g;
}

// block b -> (block row, block column): the triangle row by row, then the full-width block rows below it
EGR_HD void wpe_block(const WpeGeom& g, int b, int* bi, int* bj) {
    if (b < g.tri) {
        int r = 0;
        while ((r + 1) * (r + 2) / 2 <= b) ++r;
        *bi = r;
        *bj = b - r * (r + 1) / 2;
    } else {
        const int q = b - g.tri;
        *bi = g.nbk + q / g.nbk;
        *bj = q % g.nbk;
    }
}

// offset of row r's sample for tile frame 0 inside the tile [D][LDT] (tile column H is the tile's first frame)
EGR_HD int wpe_row_base(const WpeGeom& g, int r) {
    if (r < g.K) {
        const int k = r / g.D, d = r - k * g.D;
        return d * g.LDT + (g.taps - 1 - k);          // H - delay - k
    }
    return (r - g.K) * g.LDT + g.H;
}

// tile element e (0 .. D LDT - 1) of the tile starting at frame t0 -> channel and frame (frame outside [0, T): zero)
EGR_HD void wpe_tile_src(const WpeGeom& g, int e, int t0, int* d, int* t) {
    *d = e / g.LDT;
    *t = t0 - g.H + (e - *d * g.LDT);
}

// one tile's contribution to a 4 x 4 block: acc[i][j] += a_i[t] conj(b_j[t]) inv[t]
EGR_HD void wpe_acc_block(const wpe_c32* tile, const double* invt, int nt, const int (&rb)[4], const int (&cb)[4], double (&ar)[16],
                              double (&ai)[16]) {
    for (int t = 0; t < nt; ++t) {
        const double w = invt[t];
        double axr[4], axi[4], bxr[4], bxi[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const wpe_c32 a = tile[rb[i] + t], b = tile[cb[i] + t];
            axr[i] = (double)a.x; axi[i] = (double)a.y;
            bxr[i] = (double)b.x * w; bxi[i] = (double)b.y * w;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ar[i * 4 + j] += axr[i] * bxr[j] + axi[i] * bxi[j];
                ai[i * 4 + j] += axi[i] * bxr[j] - axr[i] * bxi[j];
            }
    }
}

// s + c += a b with the rounding errors of the product (fma) and of the sum (two-sum) collected in c: the pair carries the running
// sum to about twice the precision of a double.  Contraction is off so that the sum below stays the plain rounded s + p the
// two-sum identity needs.
EGR_HD void wpe_mac2(double a, double b, double& s, double& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p = a * b, pe = fma(a, b, -p);
    const double t = s + p, v = t - s;
    c += ((s - (t - v)) + (p - v)) + pe;
    s = t;
}

// sweep 2 of k_wpe_iter, one output: X[e][t0 + tl] = Y[e][t0 + tl] - sum_i GH[e][i] Ytilde_i[t0 + tl] from the tile [D][LDT]
// (stacked row i = k D + d sits at tile column taps - 1 - k + tl of channel d; Y itself at column H + tl); gh is row e of GH.
// Where the prediction cancels the observation the terms are much larger than X, and the next weights 1 / |X|^2 would carry a
// plain double sum's eps |terms| / |X|; the compensated sum leaves eps |X|.
EGR_HD void wpe_filter_sum(const WpeGeom& g, const wpe_c32* tile, const wpe_c64* gh, int e, int tl, double* xr, double* xi) {
    const wpe_c32 yv = tile[e * g.LDT + g.H + tl];
    double sr = (double)yv.x, si = (double)yv.y, cr = 0.0, ci = 0.0;
    int i = 0;
    for (int k = 0; k < g.taps; ++k)
        for (int d = 0; d < g.D; ++d, ++i) {
            const wpe_c32 z = tile[d * g.LDT + (g.taps - 1 - k) + tl];
            const wpe_c64 c = gh[i];
            wpe_mac2(-c.x, (double)z.x, sr, cr);
            wpe_mac2(c.y, (double)z.y, sr, cr);
            wpe_mac2(-c.x, (double)z.y, si, ci);
            wpe_mac2(-c.y, (double)z.x, si, ci);
        }
    *xr = sr + cr;
    *xi = si + ci;
}

// ---- many clips per launch (egr_wpemany_dereverb; tools/wpemany_host_check.cpp walks this part).  No grid dimension counts clips or
// tracks: k_wpe_iter_many's flat workgroup index is clip * bins + bin, and the analysis and synthesis kernels find their clip in
// a prefix table of tiles (runs): off[i] = first flat tile of clip i, off[n] = all tiles, clip i holding C equal stretches, one per
// channel.  Every clip has at least one tile per channel, so the table ascends strictly.
struct WpeClip {                 // one row of the device table, longest clip first
    long long x_off, y_off;      // the clip's [C][n] input in x and its [C][n_out] output in y, in floats
    long long n, n_out;
    long long ws_off;            // the clip's block of the workspace, in bytes: Y, X, inv[0], inv[1], flags as the single call lays them out
    long long spec_bytes, inv_bytes;
    long long frames;
};

// workgroups one channel of a clip brings to the analysis and to the synthesis grid
EGR_HD long long wpe_stft_tiles(long long frames) { return (frames + WPE_FT - 1) / WPE_FT; }
EGR_HD long long wpe_istft_runs(long long frames, int n_fft, int hop) { return (frames - 1 + n_fft / hop + WPE_SEG - 1) / WPE_SEG; }

EGR_HD void wpe_many_pair(long long idx, int bins, int* clip, int* bin) {
    const long long c = idx / bins;
    *clip = (int)c;
    *bin = (int)(idx - c * bins);
}

// flat tile -> clip, channel and the tile's index inside that channel
EGR_HD void wpe_many_track(const long long* off, int n, int C, long long tile, int* clip, int* c, long long* local) {
    const int i = track_of(off, n, 1, 0, tile);
    const long long r = tile - off[i], per = (off[i + 1] - off[i]) / C;
    const long long ch = r / per;
    *clip = i;
    *c = (int)ch;
    *local = r - ch * per;
}

}  // namespace egr
