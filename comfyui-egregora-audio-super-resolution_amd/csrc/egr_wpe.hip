// WPE dereverberation (SPEC.md 4d): per-bin multi-channel weighted prediction error over STFT frames.
//   k_wpe_stft   periodic-Blackman analysis, spectra stored [bin][channel][frame] so that a bin's frames are contiguous
//   k_wpe_iter   one workgroup per bin and iteration: weighted correlations in registers, Cholesky and the triangular solves in
//                LDS, all in double; then the filter sweep and the next iteration's weights
//   k_wpe_istft  inverse transform, synthesis window and overlap-add as a gather (no atomics)
// Spectra are complex64 in memory; everything between them and the final X is double (SPEC WPE-P6).
// Each kernel's body is a __device__ function that takes the workgroup's place as arguments.  The kernels above pass blockIdx (one clip
// per call); k_wpe_stft_many, k_wpe_iter_many and k_wpe_istft_many look the place up in device tables (egr_wpemany_dereverb: many clips in
// 2 + iterations launches, flat 1-D grids, every clip with the bits of its single call).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "egr_common.h"
#include "egr_fft_device.h"
#include "egr_handle.h"
#include "egr_plan.h"
#include "egr_stft_tables.h"
#include "egr_wpe_index.h"

namespace egr {

// (WPE_FT, WPE_SEG: frames per workgroup of k_wpe_stft, segments per workgroup of k_wpe_istft -- egr_wpe_index.h)
constexpr int WPE_LDS_MAX = 160 * 1024;
constexpr double WPE_PSD_FLOOR = 1e-10, WPE_PIVOT_FLOOR = 1e-13;

// ------------------------------------------------------------------------------------------------------------ analysis
// Workgroup (tile of WPE_FT frames, channel).  Frame t covers samples t hop - (n_fft - hop) + [0, n_fft) of x, zeros outside [0, n).
// (tile, c: the workgroup's place, blockIdx of the single call, a table lookup of the many-clip one)
__device__ __forceinline__ void wpe_stft_tile(const float* __restrict__ x, int C, long long n, int n_fft, int hop, int frames,
                                              const float* __restrict__ win, FftDesc fd, const cplx* __restrict__ tw,
                                              const cplx* __restrict__ wsplit, cplx* __restrict__ Y, long long tile, int c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* buf = (cplx*)smem;                                   // [WPE_FT][Mh]
    const int Mh = n_fft / 2;
    const long long t0 = tile * WPE_FT;
    const long long pad = n_fft - hop;
    const float* xc = x + (size_t)c * n;
    for (int fr = 0; fr < WPE_FT; ++fr) {
        const long long t = t0 + fr;
        for (int e = threadIdx.x; e < Mh; e += blockDim.x) {
            float v[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const long long s = t * hop + 2 * e + h - pad;
                v[h] = (t < frames && s >= 0 && s < n) ? xc[s] * win[2 * e + h] : 0.f;
            }
            buf[fr * Mh + e] = make_float2(v[0], v[1]);
        }
    }
    __syncthreads();
    for (int fr = 0; fr < WPE_FT; ++fr) lds_fft_ip<false, 0, false>(buf + fr * Mh, fd, tw, 1, 0, 1, 0, false);
    for (int idx = threadIdx.x; idx < (Mh + 1) * WPE_FT; idx += blockDim.x) {
        const int k = idx / WPE_FT, fr = idx - k * WPE_FT;
        const long long t = t0 + fr;
        if (t >= frames) continue;
        const cplx* z = buf + fr * Mh;
        const cplx Za = z[k == Mh ? 0 : k];
        const cplx Zb = z[(k == 0 || k == Mh) ? 0 : Mh - k];
        const cplx E = make_float2(0.5f * (Za.x + Zb.x), 0.5f * (Za.y - Zb.y));
        const cplx O = make_float2(0.5f * (Za.y + Zb.y), -0.5f * (Za.x - Zb.x));
        Y[((size_t)k * C + c) * frames + t] = cadd(E, cmul(wsplit[k], O));
    }
}

__global__ __launch_bounds__(256) void k_wpe_stft(const float* __restrict__ x, int C, long long n, int n_fft, int hop, int frames,
                                                   const float* __restrict__ win, FftDesc fd, const cplx* __restrict__ tw,
                                                   const cplx* __restrict__ wsplit, cplx* __restrict__ Y) {
    wpe_stft_tile(x, C, n, n_fft, hop, frames, win, fd, tw, wsplit, Y, (long long)blockIdx.x, (int)blockIdx.y);
}

// Many clips: a flat grid over the frame tiles of every (clip, channel) track; off = the prefix table of tiles (egr_wpe_index.h).
__global__ __launch_bounds__(256) void k_wpe_stft_many(const float* __restrict__ x, const WpeClip* __restrict__ clips,
                                                        const long long* __restrict__ off, int n_clips, int C, int n_fft, int hop,
                                                        const float* __restrict__ win, FftDesc fd, const cplx* __restrict__ tw,
                                                        const cplx* __restrict__ wsplit, char* __restrict__ ws) {
    int i, c;
    long long tile;
    wpe_many_track(off, n_clips, C, (long long)blockIdx.x, &i, &c, &tile);
    const WpeClip q = clips[i];
    wpe_stft_tile(x + q.x_off, C, q.n, n_fft, hop, (int)q.frames, win, fd, tw, wsplit, (cplx*)(ws + q.ws_off), tile, c);
}

// ------------------------------------------------------------------------------------------------------------ synthesis
// Workgroup (run of WPE_SEG hop-long segments of the faded signal, channel): the n_fft / hop + WPE_SEG - 1 frames that touch the run
// are inverse-transformed one after the other, in ascending frame order, and every thread adds its own samples -- the sum order of
// an output sample is fixed, so the result is the same bits on every call.
__device__ __forceinline__ void wpe_istft_run(const cplx* __restrict__ Y, int C, int frames, int n_fft, int hop,
                                              const float* __restrict__ wsyn, FftDesc fd, const cplx* __restrict__ tw,
                                              const cplx* __restrict__ wsplit, float* __restrict__ y, long long n_out, long long run, int c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Mh = n_fft / 2, R = n_fft / hop;
    cplx* buf = (cplx*)smem;                                   // [Mh]
    float* acc = (float*)(buf + Mh);                           // [WPE_SEG hop]
    const long long j0 = run * WPE_SEG;
    const int na = WPE_SEG * hop;
    const float inv_mh = 1.0f / (float)Mh;
    for (int a = threadIdx.x; a < na; a += blockDim.x) acc[a] = 0.f;
    for (long long t = j0 - R + 1; t < j0 + WPE_SEG; ++t) {
        if (t < 0 || t >= frames) continue;                    // the same in every thread
        __syncthreads();
        for (int k = threadIdx.x; k < Mh; k += blockDim.x) {
            cplx Xa = Y[((size_t)k * C + c) * frames + t];
            cplx Xb = Y[((size_t)(Mh - k) * C + c) * frames + t];
            if (k == 0) { Xa.y = 0.f; Xb.y = 0.f; }            // irfft ignores the imaginary parts of bins 0 and n_fft / 2
            const cplx E = make_float2(0.5f * (Xa.x + Xb.x), 0.5f * (Xa.y - Xb.y));
            const cplx Dd = make_float2(0.5f * (Xa.x - Xb.x), 0.5f * (Xa.y + Xb.y));
            const cplx O = cmulc(Dd, wsplit[k]);
            buf[k] = make_float2(E.x - O.y, E.y + O.x);        // Z = E + i O
        }
        __syncthreads();
        lds_fft_ip<false, 0, false>(buf, fd, tw, 1, 0, 1, 0, true);
        const long long shift = (j0 - t) * hop;                // sample i of frame t sits at run offset i - shift
        for (int a = threadIdx.x; a < na; a += blockDim.x) {
            const long long i = a + shift;
            if (i >= 0 && i < n_fft) {
                const cplx z = buf[i >> 1];
                acc[a] += ((i & 1) ? z.y : z.x) * inv_mh * wsyn[i];
            }
        }
    }
    __syncthreads();
    float* yc = y + (size_t)c * n_out;
    for (int a = threadIdx.x; a < na; a += blockDim.x) {
        const long long s = j0 * hop + a - (n_fft - hop);
        if (s >= 0 && s < n_out) yc[s] = acc[a];
    }
}

__global__ __launch_bounds__(256) void k_wpe_istft(const cplx* __restrict__ Y, int C, int frames, int n_fft, int hop,
                                                    const float* __restrict__ wsyn, FftDesc fd, const cplx* __restrict__ tw,
                                                    const cplx* __restrict__ wsplit, float* __restrict__ y, long long n_out) {
    wpe_istft_run(Y, C, frames, n_fft, hop, wsyn, fd, tw, wsplit, y, n_out, (long long)blockIdx.x, (int)blockIdx.y);
}

// Many clips: a flat grid over the segment runs of every track; the spectra read are the clip's X, behind its Y in its block.
__global__ __launch_bounds__(256) void k_wpe_istft_many(const char* __restrict__ ws, const WpeClip* __restrict__ clips,
                                                         const long long* __restrict__ off, int n_clips, int C, int n_fft, int hop,
                                                         const float* __restrict__ wsyn, FftDesc fd, const cplx* __restrict__ tw,
                                                         const cplx* __restrict__ wsplit, float* __restrict__ y) {
    int i, c;
    long long run;
    wpe_many_track(off, n_clips, C, (long long)blockIdx.x, &i, &c, &run);
    const WpeClip q = clips[i];
    wpe_istft_run((const cplx*)(ws + q.ws_off + q.spec_bytes), C, (int)q.frames, n_fft, hop, wsyn, fd, tw, wsplit, y + q.y_off, q.n_out,
                  run, c);
}

// ------------------------------------------------------------------------------------------------------------ one iteration
__device__ __forceinline__ double wpe_block_max(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = WPE_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    const double m = red[0];
    __syncthreads();
    return m;
}

struct WpeLds {
    size_t gh, r, pw, invt, red, ldiag, total;
};
static __host__ __device__ inline WpeLds wpe_lds(const WpeGeom& g) {
    WpeLds l;
    const size_t rbytes = (size_t)g.K * g.K * 16, tbytes = (size_t)g.D * g.LDT * 8;
    l.gh = 0;                                                  // rows K .. M-1 of the factorisation: P^H, then W^H, then G^H
    l.r = (size_t)g.D * g.K * 16;                              // rows 0 .. K-1; the frame tile of both sweeps lives in the same bytes
    l.pw = l.r + (((rbytes > tbytes ? rbytes : tbytes) + 15) & ~(size_t)15);
    l.invt = l.pw + (size_t)g.D * g.TT * 8;
    l.red = l.invt + (size_t)g.TT * 8;
    l.ldiag = l.red + (size_t)WPE_THREADS * 8;
    l.total = l.ldiag + (size_t)WPE_MAX_K * 8;
    return l;
}

// Y: [bins][D][T] complex64.  inv_in: [bins][T] double, or NULL: the weights come from Y itself (first iteration) and are left in
// ws_inv.  X (LAST only): [bins][D][T] complex64.  G: NULL or [bins][K][D] complex double.  inv_out: NULL or [bins][T] double.
// f: the bin (blockIdx.x of the single call; the many-clip call passes its clip's arrays and the bin of its flat index).
template <int NB, bool LAST>
__device__ __forceinline__ void wpe_iter_bin(const cplx* __restrict__ Y, const double* __restrict__ inv_in, int D, int T, int taps,
                                             int delay, cplx* __restrict__ X, double2* __restrict__ G, double* __restrict__ inv_out,
                                             int* __restrict__ flags, double* __restrict__ ws_inv, const size_t f) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const WpeGeom g = wpe_geom(D, taps, delay);
    const WpeLds L = wpe_lds(g);
    const int K = g.K, M = g.M, TT = g.TT, LDT = g.LDT, H = g.H;
    double2* GH = (double2*)(smem + L.gh);
    double2* Rm = (double2*)(smem + L.r);
    cplx* tile = (cplx*)(smem + L.r);
    double* pw = (double*)(smem + L.pw);
    double* invt = (double*)(smem + L.invt);
    double* red = (double*)(smem + L.red);
    double* ldiag = (double*)(smem + L.ldiag);
    const int tid = threadIdx.x;
    const cplx* Yf = Y + f * (size_t)D * T;
    const double* inv = inv_in ? inv_in + f * (size_t)T : ws_inv + f * (size_t)T;

    if (!inv_in) {                                             // p[t] = mean_d |Y[d,t]|^2 ; inv = 1 / max(p, floor * max p)
        double* wi = ws_inv + f * (size_t)T;
        double pm = 0.0;
        for (int t = tid; t < T; t += WPE_THREADS) {
            double p = 0.0;
            for (int d = 0; d < D; ++d) {
                const cplx v = Yf[(size_t)d * T + t];
                p += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
            }
            p /= (double)D;
            wi[t] = p;
            pm = fmax(pm, p);
        }
        pm = wpe_block_max(pm, red);
        for (int t = tid; t < T; t += WPE_THREADS) wi[t] = 1.0 / fmax(wi[t], WPE_PSD_FLOOR * pm);
        __syncthreads();
    }

    // ---- sweep 1: the blocks this thread owns
    double ar[NB][16], ai[NB][16];
    int rb[NB][4], cb[NB][4], r0[NB], c0[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        const int b = tid + n * WPE_THREADS;
        int bi = 0, bj = 0;
        if (b < g.nblocks) wpe_block(g, b, &bi, &bj);
        r0[n] = 4 * bi; c0[n] = 4 * bj;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rb[n][i] = wpe_row_base(g, min(r0[n] + i, M - 1));
            cb[n][i] = wpe_row_base(g, min(c0[n] + i, K - 1));
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) { ar[n][e] = 0.0; ai[n][e] = 0.0; }
    }
    for (int t0 = 0; t0 < T; t0 += TT) {
        __syncthreads();
        for (int e = tid; e < D * LDT; e += WPE_THREADS) {
            int d, t;
            wpe_tile_src(g, e, t0, &d, &t);
            tile[e] = (t >= 0 && t < T) ? Yf[(size_t)d * T + t] : make_float2(0.f, 0.f);
        }
        for (int e = tid; e < TT; e += WPE_THREADS) invt[e] = (t0 + e < T) ? inv[t0 + e] : 0.0;
        __syncthreads();
        const int nt = min(TT, T - t0);
#pragma unroll
        for (int n = 0; n < NB; ++n)
            if (tid + n * WPE_THREADS < g.nblocks) wpe_acc_block(tile, invt, nt, rb[n], cb[n], ar[n], ai[n]);
    }
    __syncthreads();                                           // the tile's bytes become R
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        if (tid + n * WPE_THREADS >= g.nblocks) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = r0[n] + i, c = c0[n] + j;
                if (r < M && c < K) {
                    double2* row = r < K ? Rm + (size_t)r * K : GH + (size_t)(r - K) * K;
                    row[c] = make_double2(ar[n][i * 4 + j], ai[n][i * 4 + j]);
                }
            }
    }
    __syncthreads();

    // ---- Cholesky of R (lower triangle), carried through the P^H rows: they become W^H = (L^-1 P)^H
    double dmax = 0.0;
    if (tid < K) dmax = Rm[(size_t)tid * K + tid].x;
    dmax = wpe_block_max(dmax, red);
    const double thr = WPE_PIVOT_FLOOR * dmax;
    bool fail = false;
    for (int k = 0; k < K; ++k) {
        const double piv = Rm[(size_t)k * K + k].x;            // every thread reads the same value
        if (!(piv > thr)) { fail = true; break; }              // also catches NaN
        const double l = sqrt(piv);
        if (tid == 0) ldiag[k] = l;
        for (int r = k + 1 + tid; r < M; r += WPE_THREADS) {
            double2* row = r < K ? Rm + (size_t)r * K : GH + (size_t)(r - K) * K;
            row[k] = make_double2(row[k].x / l, row[k].y / l);
        }
        __syncthreads();
        const int nr = M - k - 1, nc = K - k - 1;
        for (int idx = tid; idx < nr * nc; idx += WPE_THREADS) {
            const int r = k + 1 + idx / nc, c = k + 1 + idx % nc;
            if (c > r) continue;
            double2* row = r < K ? Rm + (size_t)r * K : GH + (size_t)(r - K) * K;
            const double2 a = row[k], b = Rm[(size_t)c * K + k];
            double2 v = row[c];
            v.x -= a.x * b.x + a.y * b.y;
            v.y -= a.y * b.x - a.x * b.y;
            row[c] = v;
        }
        __syncthreads();
    }
    // ---- back substitution in place: GH[e][k] = conj(G[k][e]),  G = L^-H W
    if (!fail) {
        for (int k = K - 1; k >= 0; --k) {
            const double l = ldiag[k];
            for (int e = tid; e < D; e += WPE_THREADS) {
                double2 v = GH[(size_t)e * K + k];
                GH[(size_t)e * K + k] = make_double2(v.x / l, v.y / l);
            }
            __syncthreads();
            for (int idx = tid; idx < D * k; idx += WPE_THREADS) {
                const int e = idx / k, j = idx - e * k;
                const double2 a = Rm[(size_t)k * K + j], b = GH[(size_t)e * K + k];
                double2 v = GH[(size_t)e * K + j];
                v.x -= a.x * b.x - a.y * b.y;
                v.y -= a.x * b.y + a.y * b.x;
                GH[(size_t)e * K + j] = v;
            }
            __syncthreads();
        }
    }
    if (flags && tid == 0) flags[f] = fail ? 1 : 0;
    if (G) {
        double2* Gf = G + f * (size_t)K * D;
        for (int idx = tid; idx < K * D; idx += WPE_THREADS) {
            const int i = idx / D, e = idx - i * D;
            const double2 v = GH[(size_t)e * K + i];
            Gf[idx] = fail ? make_double2(0.0, 0.0) : make_double2(v.x, -v.y);
        }
    }
    if (!LAST && !inv_out) return;

    // ---- sweep 2: X = Y - G^H Ytilde (a bin whose factorisation stopped keeps X = Y), then the next weights
    double pm = 0.0;
    double* po = inv_out ? inv_out + f * (size_t)T : nullptr;
    for (int t0 = 0; t0 < T; t0 += TT) {
        __syncthreads();
        for (int e = tid; e < D * LDT; e += WPE_THREADS) {
            int d, t;
            wpe_tile_src(g, e, t0, &d, &t);
            tile[e] = (t >= 0 && t < T) ? Yf[(size_t)d * T + t] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        const int nt = min(TT, T - t0);
        for (int idx = tid; idx < D * TT; idx += WPE_THREADS) {
            const int e = idx / TT, tl = idx - e * TT;
            if (tl >= nt) continue;
            const cplx yv = tile[e * LDT + H + tl];
            double sr = (double)yv.x, si = (double)yv.y;
            cplx xo = yv;
            if (!fail) {
                wpe_filter_sum(g, tile, GH + (size_t)e * K, e, tl, &sr, &si);
                xo = make_float2((float)sr, (float)si);
            }
            if (LAST) X[f * (size_t)D * T + (size_t)e * T + t0 + tl] = xo;
            pw[e * TT + tl] = sr * sr + si * si;
        }
        __syncthreads();
        if (po)
            for (int tl = tid; tl < nt; tl += WPE_THREADS) {
                double p = 0.0;
                for (int e = 0; e < D; ++e) p += pw[e * TT + tl];
                p /= (double)D;
                po[t0 + tl] = p;
                pm = fmax(pm, p);
            }
    }
    if (po) {
        pm = wpe_block_max(pm, red);                           // its barriers also order the p stores above before the loads below
        for (int t = tid; t < T; t += WPE_THREADS) po[t] = 1.0 / fmax(po[t], WPE_PSD_FLOOR * pm);
    }
}

template <int NB, bool LAST>
__global__ __launch_bounds__(WPE_THREADS) void k_wpe_iter(const cplx* __restrict__ Y, const double* __restrict__ inv_in, int D, int T,
                                                           int taps, int delay, cplx* __restrict__ X, double2* __restrict__ G,
                                                           double* __restrict__ inv_out, int* __restrict__ flags,
                                                           double* __restrict__ ws_inv) {
    wpe_iter_bin<NB, LAST>(Y, inv_in, D, T, taps, delay, X, G, inv_out, flags, ws_inv, (size_t)blockIdx.x);
}

// Many clips: workgroup clip * bins + bin of a flat grid.  in_sel: -1 (first iteration: the weights come from Y and stay in inv[0]) or
// the inv buffer read; out_sel: -1 (last iteration) or the inv buffer written.  X is written by the LAST instantiation alone.
template <int NB, bool LAST>
__global__ __launch_bounds__(WPE_THREADS) void k_wpe_iter_many(char* __restrict__ ws, const WpeClip* __restrict__ clips, int bins, int D,
                                                                int taps, int delay, int in_sel, int out_sel) {
    int i, f;
    wpe_many_pair((long long)blockIdx.x, bins, &i, &f);
    const WpeClip q = clips[i];
    char* base = ws + q.ws_off;
    double* inv0 = (double*)(base + 2 * q.spec_bytes);
    double* inv1 = (double*)(base + 2 * q.spec_bytes + q.inv_bytes);
    wpe_iter_bin<NB, LAST>((const cplx*)base, in_sel < 0 ? nullptr : (in_sel ? inv1 : inv0), D, (int)q.frames, taps, delay,
                           (cplx*)(base + q.spec_bytes), nullptr, out_sel < 0 ? nullptr : (out_sel ? inv1 : inv0),
                           (int*)(base + 2 * q.spec_bytes + 2 * q.inv_bytes), inv0, (size_t)f);
}

// ------------------------------------------------------------------------------------------------------------ host
struct WpeWindows {
    float *win, *wsyn;
};
static std::mutex g_wpe_mu;
static std::map<std::tuple<int, int, int>, WpeWindows> g_wpe_win;   // (device, n_fft, hop)
static std::map<int, bool> g_wpe_attr;                               // device -> LDS caps raised

static bool wpe_framing_ok(int n_fft, int hop) { return hop >= 1 && n_fft % hop == 0 && n_fft / hop >= 2; }

static int64_t wpe_frames(int64_t n, int n_fft, int hop) {
    const int64_t num = n + n_fft - 2 * (int64_t)hop;
    return (num + hop - 1) / hop + 1;
}

static int wpe_windows(int n_fft, int hop, WpeWindows* out) {
    int dev = 0;
    EGR_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_wpe_mu);
    auto it = g_wpe_win.find(std::make_tuple(dev, n_fft, hop));
    if (it != g_wpe_win.end()) { *out = it->second; return EGR_OK; }
    std::vector<double> w((size_t)n_fft);
    const double two_pi = 6.283185307179586476925286766559;
    for (int i = 0; i < n_fft; ++i)
        w[i] = 0.42 - 0.5 * cos(two_pi * i / n_fft) + 0.08 * cos(2.0 * two_pi * i / n_fft);
    std::vector<float> wa((size_t)n_fft), ws((size_t)n_fft);
    for (int i = 0; i < n_fft; ++i) {
        double s = 0.0;
        for (int j = i % hop; j < n_fft; j += hop) s += w[j] * w[j];
        wa[i] = (float)w[i];
        ws[i] = (float)(w[i] / s);
    }
    WpeWindows t;
    EGR_HIP(hipMalloc((void**)&t.win, (size_t)n_fft * sizeof(float)));
    EGR_HIP(hipMalloc((void**)&t.wsyn, (size_t)n_fft * sizeof(float)));
    EGR_HIP(hipMemcpy(t.win, wa.data(), (size_t)n_fft * sizeof(float), hipMemcpyHostToDevice));
    EGR_HIP(hipMemcpy(t.wsyn, ws.data(), (size_t)n_fft * sizeof(float), hipMemcpyHostToDevice));
    g_wpe_win[std::make_tuple(dev, n_fft, hop)] = t;
    *out = t;
    return EGR_OK;
}

static int wpe_raise_lds() {
    int dev = 0;
    EGR_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_wpe_mu);
    if (g_wpe_attr[dev]) return EGR_OK;
    const void* fns[] = {(const void*)k_wpe_stft, (const void*)k_wpe_istft, (const void*)k_wpe_iter<1, false>,
                         (const void*)k_wpe_iter<1, true>, (const void*)k_wpe_iter<2, false>, (const void*)k_wpe_iter<2, true>,
                         (const void*)k_wpe_stft_many, (const void*)k_wpe_istft_many, (const void*)k_wpe_iter_many<1, false>,
                         (const void*)k_wpe_iter_many<1, true>, (const void*)k_wpe_iter_many<2, false>,
                         (const void*)k_wpe_iter_many<2, true>};
    for (const void* fn : fns) EGR_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, WPE_LDS_MAX));
    g_wpe_attr[dev] = true;
    return EGR_OK;
}

static int wpe_check_framing(int n_fft, int hop, StftTables* t) {
    EGR_CHECK(n_fft >= 4 && (n_fft % 2) == 0 && n_fft <= 4096, EGR_ERR_UNSUPPORTED, "WPE: n_fft=%d must be even and <= 4096", n_fft);
    EGR_CHECK(wpe_framing_ok(n_fft, hop), EGR_ERR_UNSUPPORTED, "WPE: hop=%d must divide n_fft=%d with n_fft / hop >= 2", hop, n_fft);
    int rc = stft_tables(n_fft, t);
    if (rc) return rc;
    for (int s = 0; s < t->fd.nst; ++s)
        EGR_CHECK(t->fd.radix[s] <= 13, EGR_ERR_UNSUPPORTED, "WPE: n_fft=%d: n_fft/2 has a prime factor above 13", n_fft);
    return wpe_raise_lds();
}

// the limits of one iteration (SPEC WPE-P7 and the kernel's own): checked before anything is enqueued
static int wpe_check_iter(int channels, int64_t frames, int taps, int delay, WpeGeom* g, WpeLds* L) {
    EGR_CHECK(channels >= 1 && frames >= 1 && frames < (1LL << 31) - 64 && taps >= 1 && delay >= 1, EGR_ERR_ARG, "bad argument");
    EGR_CHECK((int64_t)channels * taps <= WPE_MAX_K, EGR_ERR_UNSUPPORTED, "WPE: channels * taps = %lld exceeds the limit K <= %d",
              (long long)channels * taps, WPE_MAX_K);
    EGR_CHECK(delay + taps - 1 <= WPE_MAX_HIST, EGR_ERR_UNSUPPORTED, "WPE: delay + taps - 1 = %d exceeds the limit %d", delay + taps - 1,
              WPE_MAX_HIST);
    *g = wpe_geom(channels, taps, delay);
    *L = wpe_lds(*g);
    EGR_CHECK(L->total <= (size_t)WPE_LDS_MAX, EGR_ERR_UNSUPPORTED, "WPE: %zu bytes of LDS needed (limit %d)", L->total, WPE_LDS_MAX);
    return EGR_OK;
}

static size_t wpe_align(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- many clips per call: the plan is host arithmetic alone, so that every refusal comes before anything is allocated
struct WpeManyPlan {
    std::vector<WpeClip> clips;            // longest first: the long workgroups are dispatched first
    std::vector<long long> stft_off, istft_off;
    size_t table_off = 0, table_bytes = 0, total = 0;
    WpeGeom g;
    WpeLds L;
};

// what wpe_check_framing refuses, without its tables: n_fft even, 4 .. 4096, no prime factor of n_fft / 2 above 13
static bool wpe_nfft_ok(int n_fft) {
    if (n_fft < 4 || (n_fft % 2) != 0 || n_fft > 4096) return false;
    int m = n_fft / 2;
    for (int p = 2; p <= 13; ++p)
        while (m % p == 0) m /= p;
    return m == 1;
}

static int wpe_many_plan(const int64_t* tab, int n_clips, int channels, int n_fft, int hop, int taps, int delay, WpeManyPlan* P) {
    EGR_CHECK(tab && n_clips >= 1 && channels >= 1, EGR_ERR_ARG, "WPE: want a table of n_clips >= 1 clips of channels >= 1");
    EGR_CHECK(wpe_nfft_ok(n_fft), EGR_ERR_UNSUPPORTED, "WPE: n_fft=%d must be even, <= 4096, n_fft/2 without a prime factor above 13", n_fft);
    EGR_CHECK(wpe_framing_ok(n_fft, hop), EGR_ERR_UNSUPPORTED, "WPE: hop=%d must divide n_fft=%d with n_fft / hop >= 2", hop, n_fft);
    const long long bins = n_fft / 2 + 1, lim = (1LL << 31) - 4096;
    for (int i = 0; i < n_clips; ++i)
        EGR_CHECK(tab[3 * i] >= 0 && tab[3 * i + 1] >= 1 && tab[3 * i + 2] >= 0, EGR_ERR_ARG, "WPE: clip %d: offsets %lld, %lld, n=%lld", i,
                  (long long)tab[3 * i], (long long)tab[3 * i + 2], (long long)tab[3 * i + 1]);
    int64_t longest = 1;
    for (int i = 0; i < n_clips; ++i) {
        const int64_t n = tab[3 * i + 1];
        EGR_CHECK(n < (1LL << 48) && wpe_frames(n, n_fft, hop) < lim, EGR_ERR_UNSUPPORTED, "WPE: clip %d: n=%lld gives too many frames", i,
                  (long long)n);
        longest = std::max(longest, wpe_frames(n, n_fft, hop));
    }
    int rc = wpe_check_iter(channels, longest, taps, delay, &P->g, &P->L);
    if (rc) return rc;
    EGR_CHECK((long long)n_clips * bins < lim, EGR_ERR_UNSUPPORTED, "WPE: %d clips x %lld bins exceed one grid", n_clips, bins);
    std::vector<int> order((size_t)n_clips);
    for (int i = 0; i < n_clips; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return tab[3 * a + 1] > tab[3 * b + 1]; });
    P->clips.resize((size_t)n_clips);
    P->stft_off.assign((size_t)n_clips + 1, 0);
    P->istft_off.assign((size_t)n_clips + 1, 0);
    size_t off = 0;
    for (int j = 0; j < n_clips; ++j) {
        const int i = order[j];
        WpeClip& q = P->clips[j];
        q.x_off = tab[3 * i];
        q.n = tab[3 * i + 1];
        q.y_off = tab[3 * i + 2];
        q.frames = wpe_frames(q.n, n_fft, hop);
        q.n_out = q.frames * hop - (n_fft - hop);
        q.spec_bytes = (long long)wpe_align((size_t)bins * channels * q.frames * sizeof(float2));
        q.inv_bytes = (long long)wpe_align((size_t)bins * q.frames * sizeof(double));
        q.ws_off = (long long)off;
        off += 2 * (size_t)q.spec_bytes + 2 * (size_t)q.inv_bytes + wpe_align((size_t)bins * sizeof(int));
        EGR_CHECK(off < ((size_t)1 << 60), EGR_ERR_UNSUPPORTED, "WPE: the clips' workspace exceeds 2^60 bytes");
        P->stft_off[j + 1] = P->stft_off[j] + (long long)channels * wpe_stft_tiles(q.frames);
        P->istft_off[j + 1] = P->istft_off[j] + (long long)channels * wpe_istft_runs(q.frames, n_fft, hop);
    }
    EGR_CHECK(P->stft_off[n_clips] < lim && P->istft_off[n_clips] < lim, EGR_ERR_UNSUPPORTED, "WPE: %lld frame tiles exceed one grid",
              P->stft_off[n_clips]);
    P->table_off = off;
    P->table_bytes = (size_t)n_clips * sizeof(WpeClip) + 2 * ((size_t)n_clips + 1) * sizeof(long long);
    P->total = off + wpe_align(P->table_bytes);
    return EGR_OK;
}

}  // namespace egr

using namespace egr;

extern "C" int64_t egr_wpe_frames(int64_t n, int n_fft, int hop) {
    if (n < 1 || n_fft < 2 || !wpe_framing_ok(n_fft, hop)) return 0;
    return wpe_frames(n, n_fft, hop);
}

extern "C" size_t egr_wpe_workspace_bytes(int channels, int64_t n, int n_fft, int hop, int taps) {
    if (channels < 1 || n < 1 || n_fft < 2 || !wpe_framing_ok(n_fft, hop) || taps < 1) return 0;
    const size_t frames = (size_t)wpe_frames(n, n_fft, hop), bins = (size_t)n_fft / 2 + 1;
    return 2 * wpe_align(bins * channels * frames * sizeof(float2)) + 2 * wpe_align(bins * frames * sizeof(double)) +
           wpe_align(bins * sizeof(int));
}

extern "C" int egr_wpe_stft(const float* x, int channels, int64_t n, int n_fft, int hop, void* Y, void* stream) {
    EGR_CHECK(x && Y && channels >= 1 && channels <= 65535 && n >= 1, EGR_ERR_ARG, "bad argument");
    StftTables t;
    int rc = wpe_check_framing(n_fft, hop, &t);
    if (rc) return rc;
    WpeWindows w;
    rc = wpe_windows(n_fft, hop, &w);
    if (rc) return rc;
    const int64_t frames = wpe_frames(n, n_fft, hop);
    EGR_CHECK(frames < (1LL << 31) - WPE_FT, EGR_ERR_UNSUPPORTED, "WPE: %lld frames", (long long)frames);
    const size_t lds = (size_t)WPE_FT * (n_fft / 2) * sizeof(float2);
    hipLaunchKernelGGL(k_wpe_stft, dim3((unsigned)ceil_div(frames, WPE_FT), (unsigned)channels), dim3(256), lds, (hipStream_t)stream, x,
                       channels, (long long)n, n_fft, hop, (int)frames, w.win, t.fd, t.tw, t.wsplit, (cplx*)Y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_wpe_istft(const void* Y, int channels, int64_t frames, int n_fft, int hop, float* y, int64_t n_out, void* stream) {
    EGR_CHECK(Y && y && channels >= 1 && channels <= 65535 && frames >= 1 && frames < (1LL << 31) - 4096, EGR_ERR_ARG, "bad argument");
    StftTables t;
    int rc = wpe_check_framing(n_fft, hop, &t);
    if (rc) return rc;
    EGR_CHECK(n_out == frames * hop - (n_fft - hop) && n_out >= 1, EGR_ERR_ARG, "WPE: n_out=%lld is not frames * hop - (n_fft - hop) = %lld",
              (long long)n_out, (long long)(frames * hop - (n_fft - hop)));
    WpeWindows w;
    rc = wpe_windows(n_fft, hop, &w);
    if (rc) return rc;
    const int64_t segs = frames - 1 + n_fft / hop;
    const size_t lds = (size_t)(n_fft / 2) * sizeof(float2) + (size_t)WPE_SEG * hop * sizeof(float);
    hipLaunchKernelGGL(k_wpe_istft, dim3((unsigned)ceil_div(segs, WPE_SEG), (unsigned)channels), dim3(256), lds, (hipStream_t)stream,
                       (const cplx*)Y, channels, (int)frames, n_fft, hop, w.wsyn, t.fd, t.tw, t.wsplit, y, (long long)n_out);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_wpe_iterate(const void* Y, const double* inv_in, int bins, int channels, int64_t frames, int taps, int delay, void* X,
                               double* G, double* inv_out, int* flags_out, void* ws, size_t ws_bytes, void* stream) {
    EGR_CHECK(Y && bins >= 1 && frames >= 1, EGR_ERR_ARG, "bad argument");
    WpeGeom g;
    WpeLds L;
    int rc = wpe_check_iter(channels, frames, taps, delay, &g, &L);
    if (rc) return rc;
    if (!inv_in)
        EGR_CHECK(ws && ws_bytes >= (size_t)bins * frames * sizeof(double), EGR_ERR_ARG,
                  "WPE: the first iteration needs a workspace of bins * frames * 8 = %zu bytes", (size_t)bins * frames * sizeof(double));
    rc = wpe_raise_lds();
    if (rc) return rc;
    const dim3 grid((unsigned)bins), block(WPE_THREADS);
    const bool two = g.nblocks > WPE_THREADS;
#define EGR_WPE_LAUNCH(NB, LASTV)                                                                                                    \
    hipLaunchKernelGGL((k_wpe_iter<NB, LASTV>), grid, block, L.total, (hipStream_t)stream, (const cplx*)Y, inv_in, channels, (int)frames, \
                       taps, delay, (cplx*)X, (double2*)G, inv_out, flags_out, (double*)ws)
    if (X) { if (two) EGR_WPE_LAUNCH(2, true); else EGR_WPE_LAUNCH(1, true); }
    else   { if (two) EGR_WPE_LAUNCH(2, false); else EGR_WPE_LAUNCH(1, false); }
#undef EGR_WPE_LAUNCH
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_wpe_dereverb(const float* x, int channels, int64_t n, int n_fft, int hop, int taps, int delay, int iterations, float* y,
                                int64_t n_out, void* ws, size_t ws_bytes, void* stream) {
    EGR_CHECK(x && y && ws && channels >= 1 && channels <= 65535 && n >= 1 && iterations >= 1, EGR_ERR_ARG, "bad argument");
    StftTables t;
    int rc = wpe_check_framing(n_fft, hop, &t);
    if (rc) return rc;
    const int64_t frames = wpe_frames(n, n_fft, hop);
    EGR_CHECK(frames < (1LL << 31) - 4096, EGR_ERR_UNSUPPORTED, "WPE: %lld frames", (long long)frames);
    WpeGeom g;
    WpeLds L;
    rc = wpe_check_iter(channels, frames, taps, delay, &g, &L);
    if (rc) return rc;
    EGR_CHECK(n_out == frames * hop - (n_fft - hop), EGR_ERR_ARG, "WPE: n_out=%lld is not frames * hop - (n_fft - hop) = %lld",
              (long long)n_out, (long long)(frames * hop - (n_fft - hop)));
    const size_t need = egr_wpe_workspace_bytes(channels, n, n_fft, hop, taps);
    EGR_CHECK(need > 0 && ws_bytes >= need, EGR_ERR_ARG, "WPE: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const int bins = n_fft / 2 + 1;
    const size_t spec = wpe_align((size_t)bins * channels * frames * sizeof(float2)), invb = wpe_align((size_t)bins * frames * sizeof(double));
    char* base = (char*)ws;
    void* Ys = base;
    void* Xs = base + spec;
    double* inv[2] = {(double*)(base + 2 * spec), (double*)(base + 2 * spec + invb)};
    int* flags = (int*)(base + 2 * spec + 2 * invb);
    rc = egr_wpe_stft(x, channels, n, n_fft, hop, Ys, stream);
    if (rc) return rc;
    for (int it = 0; it < iterations; ++it) {
        const bool last = it == iterations - 1;
        // iteration 0 leaves its own weights in inv[0] (the workspace argument); iteration it writes inv[(it + 1) & 1]
        rc = egr_wpe_iterate(Ys, it == 0 ? nullptr : inv[it & 1], bins, channels, frames, taps, delay, last ? Xs : nullptr, nullptr,
                             last ? nullptr : inv[(it + 1) & 1], flags, inv[0], invb, stream);
        if (rc) return rc;
    }
    return egr_wpe_istft(Xs, channels, frames, n_fft, hop, y, n_out, stream);
}

extern "C" size_t egr_wpemany_workspace_bytes(const int64_t* clips, int n_clips, int channels, int n_fft, int hop, int taps) {
    WpeManyPlan P;
    if (wpe_many_plan(clips, n_clips, channels, n_fft, hop, taps, 1, &P) != EGR_OK) return 0;
    return P.total;
}

extern "C" int egr_wpemany_dereverb(const float* x, const int64_t* clips, int n_clips, int channels, int n_fft, int hop, int taps,
                                    int delay, int iterations, float* y, void* ws, size_t ws_bytes, void* stream) {
    EGR_CHECK(x && y && ws && clips && iterations >= 1, EGR_ERR_ARG, "bad argument");
    WpeManyPlan P;
    int rc = wpe_many_plan(clips, n_clips, channels, n_fft, hop, taps, delay, &P);
    if (rc) return rc;
    EGR_CHECK(ws_bytes >= P.total, EGR_ERR_ARG, "WPE: workspace of %zu bytes, %zu needed", ws_bytes, P.total);
    StftTables t;
    rc = wpe_check_framing(n_fft, hop, &t);
    if (rc) return rc;
    WpeWindows w;
    rc = wpe_windows(n_fft, hop, &w);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    const WpeClip* dclips = (const WpeClip*)(base + P.table_off);
    const long long* dstft = (const long long*)(dclips + n_clips);
    const long long* distft = dstft + n_clips + 1;
    // the three tables go up in one asynchronous copy from pinned memory
    rc = upload_table({{P.clips.data(), (size_t)n_clips * sizeof(WpeClip)},
                       {P.stft_off.data(), ((size_t)n_clips + 1) * sizeof(long long)},
                       {P.istft_off.data(), ((size_t)n_clips + 1) * sizeof(long long)}}, base + P.table_off, st);
    if (rc) return rc;
    const int bins = n_fft / 2 + 1;
    hipLaunchKernelGGL(k_wpe_stft_many, dim3((unsigned)P.stft_off[n_clips]), dim3(256), (size_t)WPE_FT * (n_fft / 2) * sizeof(float2), st, x,
                       dclips, dstft, n_clips, channels, n_fft, hop, w.win, t.fd, t.tw, t.wsplit, base);
    EGR_HIP(hipGetLastError());
    const dim3 grid((unsigned)((long long)n_clips * bins)), block(WPE_THREADS);
    const bool two = P.g.nblocks > WPE_THREADS;
    for (int it = 0; it < iterations; ++it) {
        const bool last = it == iterations - 1;
        // the single call's buffers: iteration 0 leaves its own weights in inv[0]; iteration it reads inv[it & 1], writes inv[(it + 1) & 1]
        const int in_sel = it == 0 ? -1 : (it & 1), out_sel = last ? -1 : ((it + 1) & 1);
#define EGR_WPE_LAUNCH(NB, LASTV)                                                                                                  \
    hipLaunchKernelGGL((k_wpe_iter_many<NB, LASTV>), grid, block, P.L.total, st, base, dclips, bins, channels, taps, delay, in_sel, out_sel)
        if (last) { if (two) EGR_WPE_LAUNCH(2, true); else EGR_WPE_LAUNCH(1, true); }
        else      { if (two) EGR_WPE_LAUNCH(2, false); else EGR_WPE_LAUNCH(1, false); }
#undef EGR_WPE_LAUNCH
        EGR_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_wpe_istft_many, dim3((unsigned)P.istft_off[n_clips]), dim3(256),
                       (size_t)(n_fft / 2) * sizeof(float2) + (size_t)WPE_SEG * hop * sizeof(float), st, (const char*)base, dclips, distft,
                       n_clips, channels, n_fft, hop, w.wsyn, t.fd, t.tw, t.wsplit, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}
