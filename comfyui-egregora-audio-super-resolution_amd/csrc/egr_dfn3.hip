// DeepFilterNet3 forward pass as df.enhance.enhance runs it (SPEC.md "DeepFilterNet3 (UPSTREAM-RECALL)").
//   k_dfn_analysis   : libdf frame_analysis (n_fft - hop samples of frame memory, Vorbis window, DFT summed in double, x wnorm)
//   k_dfn_erb_db     : mean band power over the ERB widths -> 10 log10(p + 1e-10)
//   k_dfn_norm_scan  : the two exponential-mean norms (ERB dB and unit-norm complex bins), sequential over frames per lane, with the
//                      conv_lookahead shift of DfNet.pad_feat folded into the store
//   k_dfn_conv       : direct causal / transposed NHWC convolution with groups, frequency stride, BatchNorm affine, activation and
//                      a residual add (every conv of the encoder, both decoders' pathway / transposed convs)
//   egr_bgemm        : grouped linears (batched over groups) and the GRU input projections of all frames (one GEMM per layer)
//   k_dfn_rows       : bias / ReLU / tanh / residual epilogues of those GEMMs
//   k_dfn_gru        : the recurrence h_t = GRU(W_hh h_{t-1}, proj_t): one workgroup per audio channel, layers one after another
//   k_dfn_assemble   : ERB mask through the inverse map above nb_df, the deep filter (df_order complex taps, df_lookahead) below
//   k_dfn_synth      : libdf frame_synthesis (unnormalised inverse real DFT in double, window); k_dfn_ola: overlap-add + trim
// Work is enqueued on the caller's stream; nothing synchronises (the workspace grows with hipMallocAsync on that stream).
// DeepFilterNet2 (egr_dfn2_*) reuses these kernels and the host path around them; its own kernels follow them.
// Many clips in one ragged pass (egr_dfn*_enhance_tracks): the kernels that look along the frame axis are templates on
// TRK; TRK = false is the uniform [C][nF] form above, TRK = true finds a row's track and its frame within the track in the Tracks
// tables.  The arithmetic is stated once, in the shared body.
#include <math.h>
#include <string.h>

#include <memory>
#include <vector>

#include "egr_handle.h"
#include "egr_ragged_index.h"

namespace egr {
namespace {

constexpr int GRU_THREADS = 1024;
constexpr int GRU_SEG = 16;                                 // lanes that share one gate row (column c = GRU_SEG * k + lane % GRU_SEG)
constexpr int GRU_HMAX = 256;
constexpr int GRU_K = GRU_HMAX / GRU_SEG;                   // 16 columns per (row, lane)
constexpr int GRU_TASKS = 3 * GRU_HMAX * GRU_SEG / GRU_THREADS;     // 12 (row, lane) tasks per thread
constexpr int GRU_NREG = 3 * GRU_K;                         // tasks 0-2 of W_hh in VGPRs (more spills at 128 VGPRs)
constexpr int GRU_NLDS = 2 * GRU_K;                         // tasks 3-4 in LDS (128 KiB)
constexpr int GRU_NGLB = GRU_TASKS * GRU_K - GRU_NREG - GRU_NLDS;   // tasks 5-11 streamed from L2 every step (448 KiB)
constexpr int GRU_PER_THREAD = GRU_TASKS * GRU_K;           // 192
static_assert(GRU_NGLB % GRU_K == 0 && GRU_NGLB > 0, "streamed W_hh part is whole tasks");
constexpr int DFN_LDS_MAX = 152 * 1024;                     // dynamic LDS cap: a gfx950 CU's 160 KiB minus room for static arrays

// ------------------------------------------------------------------------------------------------ tracks
// Device tables of a tracks call.  A track is one channel of one clip; track b's nF_b frames are rows [foff[b], foff[b + 1]) of every
// workspace buffer (R = foff[n] rows in all), its n_b samples sit at xoff[b] of x48 / y and at [soff[b], soff[b + 1]) of the flat index
// over all output samples.  n = 0: not a tracks call.
struct Tracks {
    const int* foff = nullptr;             // [n + 1]
    const int* trk = nullptr;              // [R] the track of a packed row
    const int64_t* xoff = nullptr;         // [n]
    const int64_t* soff = nullptr;         // [n + 1]
    int n = 0;
};

// ------------------------------------------------------------------------------------------------ analysis / features
// Block (f, b) analyses frame f0 + f of channel b into row f of spec [C][nF][Fq] (f0 = 0: the whole file; a segment otherwise).
// TRK: block r analyses packed row r, frame r - foff[b] of its track b (T, nF, f0 unused).
template <bool TRK>
__global__ __launch_bounds__(256) void k_dfn_analysis(const float* __restrict__ x, int64_t T, int nF, int64_t f0, int N, int hop,
                                                       const double2* __restrict__ tw, const float* __restrict__ win, float wnorm,
                                                       float2* __restrict__ spec, Tracks tk) {
    extern __shared__ double sm[];
    double* fr = sm;                       // N windowed samples
    double2* tws = (double2*)(sm + N);     // N twiddles
    const int Fq = N / 2 + 1;
    int f = blockIdx.x, b = blockIdx.y;
    int64_t row = (int64_t)b * nF + f;
    const float* xb = x + (int64_t)b * T;
    if constexpr (TRK) {
        row = blockIdx.x;
        b = tk.trk[row];
        f = (int)row - tk.foff[b];
        xb = x + tk.xoff[b];
        T = tk.soff[b + 1] - tk.soff[b];
        f0 = 0;
    }
    const int64_t s0 = (f0 + f) * hop - (N - hop);
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const int64_t s = s0 + n;
        fr[n] = (s >= 0 && s < T) ? (double)(xb[s] * win[n]) : 0.0;
        tws[n] = tw[n];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < Fq; k += blockDim.x) {
        double re = 0.0, im = 0.0;
        int idx = 0;
        for (int n = 0; n < N; ++n) {
            const double2 w = tws[idx];
            re = fma(fr[n], w.x, re);
            im = fma(-fr[n], w.y, im);
            idx += k;
            if (idx >= N) idx -= N;
        }
        spec[row * Fq + k] = make_float2((float)(re * (double)wnorm), (float)(im * (double)wnorm));
    }
}

__global__ void k_dfn_erb_db(const float2* __restrict__ spec, int64_t rows, int Fq, int E, const int* __restrict__ band_lo,
                             const int* __restrict__ band_w, float* __restrict__ db) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < rows * E; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / E;
        const int e = (int)(i - r * E);
        const float2* s = spec + r * Fq + band_lo[e];
        const int w = band_w[e];
        double p = 0.0;
        for (int j = 0; j < w; ++j) p += (double)s[j].x * s[j].x + (double)s[j].y * s[j].y;
        db[i] = (float)(10.0 * log10(p / w + 1e-10));
    }
}

// lane < E: ERB dB lane (state s0 = linspace(-60, -90)), out (x - s) / 40; lane >= E: complex bin lane - E (state linspace(1e-3, 1e-4)),
// out x / sqrt(s).  Output frame t - la (DfNet.pad_feat); the last la frames are zero.
// The scan reads `cnt` input rows from row src0 of db / spec ([C][nS] rows) and stores input row t at row t + shift of ferb / fspec
// ([C][nD] rows) when that is >= 0; rows [zlo, zhi) of the destination are zeroed.  The whole file: src0 = 0, cnt = nS = nD = nF,
// shift = -la, zlo = max(nF - la, 0), zhi = nF, state null.  A segment continues the lane states in state [C][E + nbdf] (read unless
// `init`, which starts from the linspace values; written back at the end).
// TRK: C tracks; lane (b, l) scans its track's own rows [foff[b], foff[b + 1]) as a whole file of that many frames (shift = -la, the
// zeroed tail the track's last la rows; init, no state).
struct ScanArgs {
    const float* db; const float2* spec; float* ferb; float2* fspec; float* state;
    int C, nS, src0, cnt, nD, shift, zlo, zhi, Fq, E, nbdf, la, init;
    float alpha;
    const int* foff;
};

template <bool TRK>
__global__ void k_dfn_norm_scan(ScanArgs p) {
    const int E = p.E, nbdf = p.nbdf, Fq = p.Fq;
    const int lanes = E + nbdf;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.C * lanes) return;
    const int b = i / lanes, l = i - b * lanes;
    const float a = p.alpha, a1 = 1.f - p.alpha;
    constexpr int U = 16;
    int cnt = p.cnt, zlo = p.zlo, zhi = p.zhi;
    int64_t srow = (int64_t)b * p.nS + p.src0, drow = (int64_t)b * p.nD;      // rows of input 0 in db / spec and of output 0
    if constexpr (TRK) {
        srow = drow = p.foff[b];
        cnt = zhi = p.foff[b + 1] - p.foff[b];
        zlo = cnt - p.la > 0 ? cnt - p.la : 0;
    }
    if (l < E) {
        float s = -60.f + (-90.f + 60.f) * (E > 1 ? (float)l / (float)(E - 1) : 0.f);
        if (!p.init) s = p.state[i];
        const float* src = p.db + srow * E + l;
        float* dst = p.ferb + drow * E + l;
        for (int t0 = 0; t0 < cnt; t0 += U) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = (t0 + u < cnt) ? src[(int64_t)(t0 + u) * E] : 0.f;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u;
                if (t < cnt) {
                    s = v[u] * a1 + s * a;
                    if (t + p.shift >= 0) dst[(int64_t)(t + p.shift) * E] = (v[u] - s) / 40.f;
                }
            }
        }
        for (int t = zlo; t < zhi; ++t) dst[(int64_t)t * E] = 0.f;
        if (p.state) p.state[i] = s;
    } else {
        const int f = l - E;
        float s = 0.001f + (0.0001f - 0.001f) * (nbdf > 1 ? (float)f / (float)(nbdf - 1) : 0.f);
        if (!p.init) s = p.state[i];
        const float2* src = p.spec + srow * Fq + f;
        float2* dst = p.fspec + drow * nbdf + f;
        for (int t0 = 0; t0 < cnt; t0 += U) {
            float2 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = (t0 + u < cnt) ? src[(int64_t)(t0 + u) * Fq] : make_float2(0.f, 0.f);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u;
                if (t < cnt) {
                    s = hypotf(v[u].x, v[u].y) * a1 + s * a;
                    const float r = sqrtf(s);
                    if (t + p.shift >= 0) dst[(int64_t)(t + p.shift) * nbdf] = make_float2(v[u].x / r, v[u].y / r);
                }
            }
        }
        for (int t = zlo; t < zhi; ++t) dst[(int64_t)t * nbdf] = make_float2(0.f, 0.f);
        if (p.state) p.state[i] = s;
    }
}

// ------------------------------------------------------------------------------------------------ convolutions (NHWC: [B][T][F][C])
// t0 is the global frame index of row 0 of x and y (0: the whole file), hist [B][kt - 1][Fin][Cin] the kt - 1 input rows in front of
// row 0 (read only where the global index is >= 0; null with t0 = 0).
// TRK (B = 1, T = R packed rows, t0 = 0, no hist): a row's frame index is the one within its track, so the rows in front of a track's
// frame 0, which are the previous track's, are skipped like the rows in front of a file.
struct ConvArgs {
    const float* x; const float* w; const float* scale; const float* shift; const float* res; float* y; const float* hist;
    int64_t t0;
    int B, T, Fin, Cin, Fout, Cout, groups, kt, kf, fstride, fpad, transposed, act;
    const int* trk; const int* foff;
};

__device__ __forceinline__ float act_fn(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return 1.f / (1.f + expf(-v));
    if (act == 3) return tanhf(v);
    return v;
}

template <bool TRK>
__global__ void k_dfn_conv(ConvArgs p) {
    const int64_t n = (int64_t)p.B * p.T * p.Fout * p.Cout;
    const int cig = p.Cin / p.groups, cog = p.Cout / p.groups;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % p.Cout);
        int64_t r = i / p.Cout;
        const int fo = (int)(r % p.Fout);
        r /= p.Fout;
        int t = (int)(r % p.T);
        const int b = (int)(r / p.T);
        int64_t r0 = (int64_t)b * p.T;             // the row of frame 0
        if constexpr (TRK) {
            r0 = p.foff[p.trk[r]];
            t = (int)(r - r0);
        }
        const int g = co / cog;
        float acc = 0.f;
        if (!p.transposed) {
            const float* wc = p.w + (int64_t)co * cig * p.kt * p.kf;
            for (int it = 0; it < p.kt; ++it) {
                const int ti = t - (p.kt - 1) + it;
                if (p.t0 + ti < 0) continue;
                const float* xr = ti >= 0 ? p.x + (r0 + ti) * p.Fin * p.Cin
                                          : p.hist + ((int64_t)b * (p.kt - 1) + (ti + p.kt - 1)) * p.Fin * p.Cin;
                for (int j = 0; j < p.kf; ++j) {
                    const int fi = fo * p.fstride - p.fpad + j;
                    if (fi < 0 || fi >= p.Fin) continue;
                    const float* xv = xr + ((int64_t)fi * p.Cin + g * cig);
                    const float* wv = wc + it * p.kf + j;
                    for (int c = 0; c < cig; ++c) acc = fmaf(xv[c], wv[(int64_t)c * p.kt * p.kf], acc);
                }
            }
        } else {                                   // kt == 1; weight [Cin][Cout / groups][1][kf]
            const int col = co - g * cog;
            for (int j = 0; j < p.kf; ++j) {
                const int num = fo + p.fpad - j;
                if (num < 0 || num % p.fstride) continue;
                const int fi = num / p.fstride;
                if (fi >= p.Fin) continue;
                const float* xv = p.x + ((r0 + t) * p.Fin + fi) * p.Cin + g * cig;
                for (int c = 0; c < cig; ++c) acc = fmaf(xv[c], p.w[(((int64_t)(g * cig + c)) * cog + col) * p.kf + j], acc);
            }
        }
        float v = p.scale ? fmaf(acc, p.scale[co], p.shift[co]) : acc;
        v = act_fn(v, p.act);
        if (p.res) v += p.res[i];
        p.y[i] = v;
    }
}

// y = act(a (+ bias[col])) (+ res), rows x cols
__global__ void k_dfn_rows(const float* __restrict__ a, const float* __restrict__ bias, const float* __restrict__ res, float* __restrict__ y,
                           int64_t n, int cols, int act) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float v = a[i];
        if (bias) v += bias[i % cols];
        v = act_fn(v, act);
        if (res) v += res[i];
        y[i] = v;
    }
}

// hist [B][P][len] <- the last P rows of (hist | x [B][S][len]): what a consumer of x reads in front of the next segment.  One thread
// owns one column (b, e) and walks its P rows upwards, so the shift by S < P rows reads only rows it has not written yet.
__global__ void k_dfn_hist_push(const float* __restrict__ x, float* hist, int B, int S, int P, int len) {
    const int64_t n = (int64_t)B * len;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / len, e = i - b * len;
        for (int p = 0; p < P; ++p) {
            const int r = p + S - P;
            hist[(b * P + p) * len + e] = r >= 0 ? x[(b * S + r) * len + e] : hist[(b * P + p + S) * len + e];
        }
    }
}

// ------------------------------------------------------------------------------------------------ GRU recurrence
// One workgroup per audio channel runs all nF steps of one layer.  Gate row r (torch order r | z | n, 3H rows) is split over GRU_SEG
// lanes; thread t owns the (row, lane) tasks q = j * 1024 + t, j < 12, row q / 16, lane q % 16, columns 16 k + lane (k < 16).  Its 192
// W_hh values (zero-padded beyond H) sit: tasks 0-2 in VGPRs, 3-4 in LDS, 5-11 in global memory (L2-resident, 448 KiB per step), all
// in thread-minor order so every load is coalesced.  Per step: 16 h values from LDS, 192 FMAs, a 16-lane shuffle sum per task, the
// gate sums to LDS, one barrier, the H gate updates, one barrier.  proj = W_ih x + b_ih of all frames comes from one GEMM beforehand.
// h_in [C][H] is the state in front of step 0 (null: zeros), h_out [C][H] takes the state after the last step (null: not kept); they
// may be the same array.
// TRK: workgroup b runs track b: its rows of proj / out start at packed row foff[b], its step count is foff[b + 1] - foff[b] (nF
// unused).  The two table values are read once, in front of the step loop, and are dead in it.
template <bool TRK>
__global__ __launch_bounds__(GRU_THREADS) void k_dfn_gru(const float* __restrict__ proj, const float* __restrict__ whh_pk,
                                                          const float* __restrict__ bhh, int H, int nF, float* __restrict__ out,
                                                          const float* h_in, float* h_out, const int* __restrict__ foff) {
    __shared__ float wl[GRU_NLDS * GRU_THREADS];
    __shared__ float hs[GRU_HMAX];
    __shared__ float gs[3 * GRU_HMAX];
    const int t = threadIdx.x, lane = t % GRU_SEG, b = blockIdx.x;
    int64_t row0 = (int64_t)b * nF;
    if constexpr (TRK) {
        row0 = foff[b];
        nF = foff[b + 1] - foff[b];
    }
    const float* pb = proj + row0 * 3 * H;
    float* ob = out + row0 * H;
    float wr[GRU_NREG];
#pragma unroll
    for (int e = 0; e < GRU_NREG; ++e) wr[e] = whh_pk[(int64_t)e * GRU_THREADS + t];
    for (int e = 0; e < GRU_NLDS; ++e) wl[e * GRU_THREADS + t] = whh_pk[(int64_t)(GRU_NREG + e) * GRU_THREADS + t];
    const float* wg = whh_pk + (int64_t)(GRU_NREG + GRU_NLDS) * GRU_THREADS + t;
    if (t < GRU_HMAX) hs[t] = (h_in && t < H) ? h_in[(int64_t)b * H + t] : 0.f;
    float br = 0.f, bz = 0.f, bn = 0.f, xr = 0.f, xz = 0.f, xn = 0.f;
    if (t < H) {
        br = bhh[t]; bz = bhh[H + t]; bn = bhh[2 * H + t];
        if (nF > 0) { xr = pb[t]; xz = pb[H + t]; xn = pb[2 * H + t]; }
    }
    __syncthreads();
    for (int s = 0; s < nF; ++s) {
        float nxr = 0.f, nxz = 0.f, nxn = 0.f;
        if (t < H && s + 1 < nF) {                 // next step's projection, in flight during this step
            const float* pn = pb + (int64_t)(s + 1) * 3 * H;
            nxr = pn[t]; nxz = pn[H + t]; nxn = pn[2 * H + t];
        }
        float hv[GRU_K];
#pragma unroll
        for (int k = 0; k < GRU_K; ++k) hv[k] = hs[GRU_SEG * k + lane];
        constexpr int NRES = (GRU_NREG + GRU_NLDS) / GRU_K;      // tasks held in VGPRs / LDS
        float acc[NRES];
#pragma unroll
        for (int j = 0; j < NRES; ++j) acc[j] = 0.f;
#pragma unroll
        for (int e = 0; e < GRU_NREG; ++e) acc[e / GRU_K] = fmaf(wr[e], hv[e % GRU_K], acc[e / GRU_K]);
#pragma unroll 16
        for (int e = 0; e < GRU_NLDS; ++e) {
            const int j = (GRU_NREG + e) / GRU_K;
            acc[j] = fmaf(wl[e * GRU_THREADS + t], hv[e % GRU_K], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < NRES; ++j) {
            float v = acc[j];
#pragma unroll
            for (int o = GRU_SEG / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, GRU_SEG);
            const int row = (j * GRU_THREADS + t) / GRU_SEG;
            if (lane == 0 && row < 3 * H) gs[row] = v;
        }
#pragma unroll 1
        for (int j = NRES; j < GRU_TASKS; ++j) {           // streamed tasks: 16 coalesced loads, dot, 16-lane sum
            const float* wj = wg + (int64_t)(j - NRES) * GRU_K * GRU_THREADS;
            float w[GRU_K];
#pragma unroll
            for (int k = 0; k < GRU_K; ++k) w[k] = wj[(int64_t)k * GRU_THREADS];
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < GRU_K; ++k) v = fmaf(w[k], hv[k], v);
#pragma unroll
            for (int o = GRU_SEG / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, GRU_SEG);
            const int row = (j * GRU_THREADS + t) / GRU_SEG;
            if (lane == 0 && row < 3 * H) gs[row] = v;
        }
        __syncthreads();
        if (t < H) {
            const float r = 1.f / (1.f + expf(-(xr + gs[t] + br)));
            const float z = 1.f / (1.f + expf(-(xz + gs[H + t] + bz)));
            const float nn = tanhf(xn + r * (gs[2 * H + t] + bn));
            const float h = (1.f - z) * nn + z * hs[t];
            hs[t] = h;
            ob[(int64_t)s * H + t] = h;
        }
        xr = nxr; xz = nxz; xn = nxn;
        __syncthreads();
    }
    if (h_out && t < H) h_out[(int64_t)b * H + t] = hs[t];
}

// ------------------------------------------------------------------------------------------------ mask + deep filter, synthesis
// The assemble kernels work on nA frames from global frame asm_lo of a file of nF frames and write out [C][nA][Fq].  spec holds
// [C][nS] rows from global frame spec_lo.  mask, coefs (and alpha) hold [C][S] rows from global frame a; a row in front of a comes from
// the history arrays [C][P][...] (P_m rows of mask, look rows of coefs and alpha), which hold the rows just before a.  The whole file:
// asm_lo = spec_lo = a = 0, nA = nS = S = nF, no history.
// TRK (C = 1, nA = nS = S = R packed rows, asm_lo = spec_lo = a = 0, no history): a row's frame and the file's length nF are those of
// its track, so the deep-filter window stops at the track's last frame and never reads the next track's rows.
struct AsmArgs {
    const float2* spec; const float* mask; const float* coefs; const float* alpha;
    const float* mask_h; const float* coefs_h; const float* alpha_h; const int* band_of; float2* out;
    int64_t nF, asm_lo, spec_lo, a;
    int C, nA, nS, S, P_m, Fq, E, nbdf, order, look;
    const int* trk; const int* foff;
};

// row l of channel b's rows of cur, which start at row cb (l >= 0), or row l + P of hist [C][P][len] (l < 0)
__device__ __forceinline__ const float* lag_row(const float* cur, const float* hist, int64_t cb, int64_t b, int l, int P, int len) {
    return l >= 0 ? cur + (cb + l) * len : hist + (b * P + (l + P)) * len;
}

// What an assemble thread knows of its output row r: t the frame within the file (track), b the channel (track), nF its frames, cb the
// row of frame a in mask / coefs / alpha, sb the row of frame 0 in spec (row of frame ts: sb + ts).
struct AsmRow { int64_t t, b, nF, cb, sb; };

template <bool TRK>
__device__ __forceinline__ AsmRow asm_row(const AsmArgs& p, int64_t r) {
    AsmRow w;
    if constexpr (TRK) {
        w.b = p.trk[r];
        w.cb = w.sb = p.foff[w.b];
        w.t = r - w.cb;
        w.nF = p.foff[w.b + 1] - w.cb;
    } else {
        w.t = p.asm_lo + r % p.nA;
        w.b = r / p.nA;
        w.nF = p.nF;
        w.cb = w.b * p.S;
        w.sb = w.b * p.nS - p.spec_lo;
    }
    return w;
}

template <bool TRK>
__global__ void k_dfn_assemble(AsmArgs p) {
    const int Fq = p.Fq, nbdf = p.nbdf, order = p.order, look = p.look;
    const int64_t n = (int64_t)p.C * p.nA * Fq;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int f = (int)(i % Fq);
        const AsmRow w = asm_row<TRK>(p, i / Fq);
        const int64_t t = w.t, b = w.b;            // global frame, channel
        const int la = (int)(t - p.a);             // row of mask / coefs relative to a
        float2 y;
        if (f < nbdf) {
            const float* c = lag_row(p.coefs, p.coefs_h, w.cb, b, la, look, nbdf * 2 * order) + f * 2 * order;
            float re = 0.f, im = 0.f;
            for (int k = 0; k < order; ++k) {
                const int64_t ts = t - (order - 1 - look) + k;
                if (ts < 0 || ts >= w.nF) continue;
                const float2 s = p.spec[(w.sb + ts) * Fq + f];
                re = fmaf(s.x, c[2 * k], fmaf(-s.y, c[2 * k + 1], re));
                im = fmaf(s.x, c[2 * k + 1], fmaf(s.y, c[2 * k], im));
            }
            y = make_float2(re, im);
        } else {
            const float m = lag_row(p.mask, p.mask_h, w.cb, b, la, p.P_m, p.E)[p.band_of[f]];
            const float2 s = p.spec[(w.sb + t) * Fq + f];
            y = make_float2(s.x * m, s.y * m);
        }
        p.out[i] = y;
    }
}

__global__ __launch_bounds__(256) void k_dfn_synth(const float2* __restrict__ spec, int nF, int N, const double2* __restrict__ tw,
                                                    const float* __restrict__ win, float* __restrict__ frames) {
    extern __shared__ double sm[];
    double2* X = (double2*)sm;                     // N / 2 + 1 bins
    double2* tws = X + (N / 2 + 1);
    const int f = blockIdx.x, b = blockIdx.y, Fq = N / 2 + 1;
    const float2* sp = spec + ((int64_t)b * nF + f) * Fq;
    for (int k = threadIdx.x; k < Fq; k += blockDim.x) X[k] = make_double2(sp[k].x, sp[k].y);
    for (int k = threadIdx.x; k < N; k += blockDim.x) tws[k] = tw[k];
    __syncthreads();
    float* fo = frames + ((int64_t)b * nF + f) * N;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        double acc = 0.0;
        int idx = n;
        for (int k = 1; k < N / 2; ++k) {
            const double2 w = tws[idx];
            acc = fma(X[k].x, w.x, fma(-X[k].y, w.y, acc));
            idx += n;
            if (idx >= N) idx -= N;
        }
        const double v = X[0].x + ((n & 1) ? -X[N / 2].x : X[N / 2].x) + 2.0 * acc;
        fo[n] = (float)(v * (double)win[n]);
    }
}

// Output samples [out_lo, out_lo + cnt) of every channel of y [C][T].  frames [C][nA][N] are the synthesised frames from global frame
// asm_lo of a file of nF frames, hist [C][ov - 1][N] the ov - 1 frames in front of them (the whole file: asm_lo = out_lo = 0, nA = nF,
// cnt = T, no history).
// TRK (C = 1, cnt = the samples of all tracks, asm_lo = out_lo = 0, no history): a flat index over the output samples; thread i finds
// its track b in soff, writes sample i - soff[b] of it at y + xoff[b] and reads the track's own frames, rows foff[b] onwards.
template <bool TRK>
__global__ void k_dfn_ola(const float* __restrict__ frames, const float* __restrict__ hist, int C, int nA, int64_t asm_lo, int64_t nF,
                          int N, int hop, int64_t T, int64_t out_lo, int64_t cnt, float* __restrict__ y, Tracks tk) {
    const int64_t n = (int64_t)C * cnt;
    const int d = N - hop, ov = N / hop;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t b = i / cnt, s = out_lo + (i - b * cnt);
        int64_t fb = b * nA, yb = b * T;           // the row of frame asm_lo in frames, the channel's first sample in y
        if constexpr (TRK) {
            b = track_of((const long long*)tk.soff, tk.n, 1, 0, i);      // egr_ragged_index.h: the largest b < n with soff[b] <= i
            s = i - tk.soff[b];
            fb = tk.foff[b];
            nF = tk.foff[b + 1] - fb;
            yb = tk.xoff[b];
        }
        const int64_t o = s + d;
        const int64_t k = o / hop;
        const int j = (int)(o - k * hop);
        float acc = 0.f;
        for (int m = ov - 1; m >= 0; --m) {
            const int64_t fk = k - m;
            if (fk < 0 || fk >= nF) continue;
            const int64_t lf = fk - asm_lo;
            acc += lf >= 0 ? frames[(fb + lf) * N + m * hop + j] : hist[(b * (ov - 1) + (lf + ov - 1)) * N + m * hop + j];
        }
        y[yb + s] = acc;
    }
}

// ================================================================================================ DeepFilterNet2
// SPEC.md "4c. DeepFilterNet2 (UPSTREAM-RECALL)".  The signal path, the convolutions, the grouped linears without bias
// (GroupedLinearEinsum) and the synthesis are the DeepFilterNet3 kernels above, launched through the same host helpers; what is new:
//   k_dfn2_gru      : one GroupedGRU layer: workgroup (group, audio channel), W_hh block of the group in VGPRs, the P4 shuffle and the
//                     running sum of layer outputs in the store
//   k_dfn2_epi      : bias / activation / P3 output shuffle / residual epilogue of the GroupedLinear GEMMs
//   k_dfn2_alpha    : alpha = sigmoid(Linear(H_df -> 1)(c)) per frame
//   k_dfn2_assemble : ERB mask on every bin, the deep filter on the MASKED bins below nb_df, blended with alpha (P7)
constexpr int G2_HMAX = 128;                // per-group width k_dfn2_gru holds (h = H / G > 128 only for G = 1: the dense k_dfn_gru)

// Thread (j, s) = (threadIdx.x / S, threadIdx.x % S) of workgroup (g, b) owns gate rows j, h + j, 2h + j of group g's W_hh over the
// columns c = s + S k (k < K), 3K weights in VGPRs (zero beyond h), thread-minor in whh_pk so the one-time load is coalesced.  Per
// step: K values of h_{t-1} from LDS (double buffer, zero beyond h), 3K FMAs, an S-lane xor sum of the three gate sums, the update
// (every lane of the row group computes it; lane 0 stores), one barrier.  proj = W_ih x of all frames (egr_bgemm); b_ih is added here.
// Store: layer output at its P4 position (shuffled when `shuffle`), and sum_out = sum_in + it (sum_in null: the first layer).
// TRK: a 1-D grid, workgroup b G + g runs group g of track b over its own rows [foff[b], foff[b + 1]) (nF unused).
template <int K, bool TRK>
__global__ __launch_bounds__(512) void k_dfn2_gru(const float* __restrict__ proj, const float* __restrict__ whh_pk,
                                                   const float* __restrict__ bih, const float* __restrict__ bhh, int G, int h, int S,
                                                   int nF, int shuffle, const float* __restrict__ sum_in, float* __restrict__ out,
                                                   float* __restrict__ sum_out, const float* h_in, float* h_out,
                                                   const int* __restrict__ foff) {
    __shared__ float hs[2][G2_HMAX];
    const int t = threadIdx.x, NT = h * S, j = t / S, s = t - j * S;
    const int g = TRK ? blockIdx.x % G : blockIdx.x, b = TRK ? blockIdx.x / G : blockIdx.y, H = G * h, H3 = 3 * H;
    int64_t row0 = (int64_t)b * nF;
    if constexpr (TRK) {
        row0 = foff[b];
        nF = foff[b + 1] - foff[b];
    }
    const float* pb = proj + row0 * H3 + g * 3 * h;
    const int n = g * h + j;                                   // pre-shuffle output index
    const int pos = shuffle ? (n % G) * h + n / G : n;         // P3: output g' h + j' takes pre-shuffle j' G + g'
    float* ob = out + row0 * H + pos;
    float* sb = sum_out + row0 * H + pos;
    const float* si = sum_in ? sum_in + row0 * H + pos : nullptr;
    float w[3 * K];
    const float* wp = whh_pk + (int64_t)g * 3 * K * NT + t;
#pragma unroll
    for (int e = 0; e < 3 * K; ++e) w[e] = wp[(int64_t)e * NT];
    for (int i = t; i < 2 * G2_HMAX; i += NT) hs[i / G2_HMAX][i % G2_HMAX] = (h_in && i < h) ? h_in[(int64_t)b * H + g * h + i] : 0.f;
    const int rj = g * 3 * h + j;
    const float br = bhh[rj], bz = bhh[rj + h], bn = bhh[rj + 2 * h];
    const float ir = bih[rj], iz = bih[rj + h], in_ = bih[rj + 2 * h];
    float xr = 0.f, xz = 0.f, xn = 0.f, hp = h_in ? h_in[(int64_t)b * H + n] : 0.f;
    if (nF > 0) { xr = pb[j] + ir; xz = pb[h + j] + iz; xn = pb[2 * h + j] + in_; }
    __syncthreads();
    for (int st = 0; st < nF; ++st) {
        float nxr = 0.f, nxz = 0.f, nxn = 0.f;
        if (st + 1 < nF) {                                     // next step's projection, in flight during this step
            const float* pn = pb + (int64_t)(st + 1) * H3;
            nxr = pn[j] + ir; nxz = pn[h + j] + iz; nxn = pn[2 * h + j] + in_;
        }
        const float* hc = hs[st & 1];
        float ar = 0.f, az = 0.f, an = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float hv = hc[s + S * k];
            ar = fmaf(w[k], hv, ar);
            az = fmaf(w[K + k], hv, az);
            an = fmaf(w[2 * K + k], hv, an);
        }
        for (int o = S >> 1; o >= 1; o >>= 1) {
            ar += __shfl_xor(ar, o, S);
            az += __shfl_xor(az, o, S);
            an += __shfl_xor(an, o, S);
        }
        const float r = 1.f / (1.f + expf(-(xr + ar + br)));
        const float z = 1.f / (1.f + expf(-(xz + az + bz)));
        const float nn = tanhf(xn + r * (an + bn));
        hp = (1.f - z) * nn + z * hp;
        if (s == 0) {
            hs[(st + 1) & 1][j] = hp;
            const int64_t o = (int64_t)st * H;
            ob[o] = hp;
            sb[o] = si ? si[o] + hp : hp;
        }
        xr = nxr; xz = nxz; xn = nxn;
        __syncthreads();
    }
    if (h_out && s == 0) h_out[(int64_t)b * H + n] = hp;
}

// y[r][m] = act(a[r][src] + bias[src]) (+ res[r][m]), src = m, or with the P3 shuffle over G groups of width h = cols / G:
// src = (m % h) G + m / h.  y must not alias a when G > 1.
__global__ void k_dfn2_epi(const float* __restrict__ a, const float* __restrict__ bias, const float* __restrict__ res, float* y,
                           int64_t n, int cols, int G, int act) {
    const int h = cols / G;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cols;
        const int m = (int)(i - r * cols);
        const int src = G > 1 ? (m % h) * G + m / h : m;
        float v = a[r * cols + src];
        if (bias) v += bias[src];
        v = act_fn(v, act);
        if (res) v += res[i];
        y[i] = v;
    }
}

__global__ void k_dfn2_alpha(const float* __restrict__ c, const float* __restrict__ w, const float* __restrict__ b, int64_t rows, int H,
                             float* __restrict__ alpha) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const float* cr = c + r * H;
        float acc = 0.f;
        for (int k = 0; k < H; ++k) acc = fmaf(cr[k], w[k], acc);
        alpha[r] = 1.f / (1.f + expf(-(acc + b[0])));
    }
}

// P7: S_m = mask X on every bin; below nb_df Y = alpha DF(S_m) + (1 - alpha) S_m, DF the DFN3-P5 window over the masked frames.
template <bool TRK>
__global__ void k_dfn2_assemble(AsmArgs p) {
    const int Fq = p.Fq, nbdf = p.nbdf, order = p.order, look = p.look, E = p.E;
    const int64_t n = (int64_t)p.C * p.nA * Fq;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int f = (int)(i % Fq);
        const AsmRow w = asm_row<TRK>(p, i / Fq);
        const int64_t t = w.t, b = w.b;            // global frame, channel
        const int la = (int)(t - p.a);             // row of mask / coefs / alpha relative to a
        const int band = p.band_of[f];
        const float m = lag_row(p.mask, p.mask_h, w.cb, b, la, p.P_m, E)[band];
        const float2 s = p.spec[(w.sb + t) * Fq + f];
        const float2 sm = make_float2(s.x * m, s.y * m);
        float2 y = sm;
        if (f < nbdf) {
            const float* c = lag_row(p.coefs, p.coefs_h, w.cb, b, la, look, nbdf * 2 * order) + f * 2 * order;
            float re = 0.f, im = 0.f;
            for (int k = 0; k < order; ++k) {
                const int64_t ts = t - (order - 1 - look) + k;
                if (ts < 0 || ts >= w.nF) continue;
                const float ms = lag_row(p.mask, p.mask_h, w.cb, b, (int)(ts - p.a), p.P_m, E)[band];
                const float2 x = p.spec[(w.sb + ts) * Fq + f];
                const float2 xm = make_float2(x.x * ms, x.y * ms);
                re = fmaf(xm.x, c[2 * k], fmaf(-xm.y, c[2 * k + 1], re));
                im = fmaf(xm.x, c[2 * k + 1], fmaf(xm.y, c[2 * k], im));
            }
            const float a = lag_row(p.alpha, p.alpha_h, w.cb, b, la, look, 1)[0], a1 = 1.f - a;
            y = make_float2(re * a + sm.x * a1, im * a + sm.y * a1);
        }
        p.out[i] = y;
    }
}

// ------------------------------------------------------------------------------------------------ host side: what both models share
// DfnCore is the part of a handle the two models have in common: the signal path (analysis, ERB / dB, norm scan, every convolution,
// synthesis, overlap-add), its tables and weights, the workspace.  Dfn3 and Dfn2 hold one plus their own linears and GRU layers; their
// run() and create() call the stages below and keep only the middle of the network.
inline unsigned grid_for(int64_t n, int bs = 256) {
    int64_t g = (n + bs - 1) / bs;
    if (g > 65536) g = 65536;
    return (unsigned)(g < 1 ? 1 : g);
}
inline int64_t align64(int64_t n) { return (n + 63) & ~63LL; }


struct Conv {                 // one convolution with its (optional) BN affine
    const float* w = nullptr; const float* scale = nullptr; const float* shift = nullptr;
    int cin = 0, cout = 0, groups = 1, kt = 1, kf = 1, transposed = 0;
    // a segmented call only (null / 0 in a one-pass call): the kt - 1 input rows in front of the segment, the segment's first frame
    float* hist = nullptr;
    int64_t t0 = 0;
    // a tracks call only: the row -> track and track -> first row tables (Tracks), for the convolutions that look back in time
    const int* trk = nullptr; const int* foff = nullptr;
};

struct DfnDims {              // the hyper-parameters the shared code reads, from egr_dfn3_config / egr_dfn2_config
    int fft_size, hop_size, nb_erb, nb_df, df_order, df_lookahead, conv_lookahead, conv_ch, kt, kf, kt_inp, kf_inp, convt_kf;
    int df_pathway_kt, path_groups, df_path_groups, emb_hidden_dim, emb_num_layers, df_hidden_dim, df_num_layers;
    float norm_alpha;
    int erb_widths[EGR_DFN3_MAX_ERB];
};

struct Bufs {                 // workspace buffers of the shared path; the models add theirs (Dfn3::X, Dfn2::X)
    float2 *spec, *spec_e, *fspec;
    float *db, *ferb, *e[4], *c0, *c1, *tmp, *emb0, *proj, *gout[EGR_DFN3_MAX_GRU], *dfc, *demb, *pbuf, *dbuf, *mask, *tcoef, *cpt, *cp;
    float *coefs, *frames;
};

struct Rows {                 // rows (channels x frames) of the three kinds of workspace buffers; one-pass: all C * nF
    int64_t net;              // everything the network computes
    int64_t spec;             // spec, db
    int64_t asmr;             // spec_e, frames
};

struct SegState {             // what a segmented call carries besides the GRU states and the convolutions' histories
    float *norm = nullptr, *mask_h = nullptr, *coefs_h = nullptr, *alpha_h = nullptr, *frames_h = nullptr;
};

constexpr int N_HIST_CONV = 9;

struct DfnCore {
    DfnDims d;
    int device = 0, Fq = 0, embd = 0;
    float* dev_w = nullptr;                 // packed weights + repacked W_hh + tables (one allocation)
    const double2* tw = nullptr; const float* win = nullptr; const int* band_lo = nullptr; const int* band_w = nullptr;
    const int* band_of = nullptr;
    float wnorm = 0.f;
    Conv erb0, erb_dw[3], erb_pw[3], df0, df0_pw, df1_dw, df1_pw, path[4], ct_dw[3], ct_pw[3], out0, convp, convp_pw;
    // workspace of the last call
    Workspace ws;
    TableStage stage;                       // tracks calls only
    int lastC = 0, lastF = 0; int64_t lastT = 0;
    bool segmented = false;                 // the last call was a segmented one (its buffers hold the last segment only)
    bool packed = false;                    // the last call was a tracks call (its buffers hold packed rows, not [C][nF])
    SegState sg;
    Tracks tk;                              // a tracks call only (n = 0 otherwise): its tables, which live in the workspace
    Bufs B;
    // GRU layers in the order encoder (1), ERB decoder (emb_num_layers - 1), DF decoder (df_num_layers)
    int ngru() const { return d.emb_num_layers + d.df_num_layers; }
    int gru_width(int g) const { return g < d.emb_num_layers ? d.emb_hidden_dim : d.df_hidden_dim; }
    int64_t frames_of(int64_t n) const { return (n + d.fft_size) / d.hop_size; }
};

struct Take {                 // the workspace allocator: 256-byte slots one after another; base null only measures
    char* base;
    size_t off = 0;
    float* operator()(int64_t nfl) {
        float* p = base ? (float*)(base + off) : nullptr;
        off += ((size_t)nfl * sizeof(float) + 255) & ~(size_t)255;
        return p;
    }
};

void layout_common(const DfnCore& m, const Rows& rows, Take& take, Bufs& b) {
    const int64_t R = rows.net, Rs = rows.spec, Ra = rows.asmr;
    const DfnDims& d = m.d;
    const int ch = d.conv_ch, E = d.nb_erb, nb = d.nb_df, O2 = 2 * d.df_order;
    const int Hm = d.emb_hidden_dim > d.df_hidden_dim ? d.emb_hidden_dim : d.df_hidden_dim;
    const int Fm = E > nb ? E : nb;
    b.spec = (float2*)take(Rs * m.Fq * 2);
    b.spec_e = (float2*)take(Ra * m.Fq * 2);
    b.fspec = (float2*)take(R * nb * 2);
    b.db = take(Rs * E);
    b.ferb = take(R * E);
    b.e[0] = take(R * E * ch);
    b.e[1] = take(R * (E / 2) * ch);
    b.e[2] = take(R * (E / 4) * ch);
    b.e[3] = take(R * (E / 4) * ch);
    b.c0 = take(R * nb * ch);
    b.c1 = take(R * (nb / 2) * ch);
    b.tmp = take(R * Fm * ch);
    b.emb0 = take(R * m.embd);
    b.proj = take(R * 3 * Hm);
    for (int g = 0; g < EGR_DFN3_MAX_GRU; ++g) b.gout[g] = g < m.ngru() ? take(R * m.gru_width(g)) : nullptr;
    b.dfc = take(R * d.df_hidden_dim);
    b.demb = take(R * m.embd);
    b.pbuf = take(R * E * ch);
    b.dbuf = take(R * E * ch);
    b.mask = take(R * E);
    b.tcoef = take(R * nb * O2);
    b.cpt = take(R * nb * O2);
    b.cp = take(R * nb * O2);
    b.coefs = take(R * nb * O2);
    b.frames = take(Ra * d.fft_size);
}

// hist [B][P][len] <- the last P rows of (hist | x [B][S][len])
void hist_push(const float* x, float* hist, int B, int S, int P, int len, hipStream_t st) {
    if (P < 1 || S < 1) return;
    hipLaunchKernelGGL(k_dfn_hist_push, dim3(grid_for((int64_t)B * len)), dim3(256), 0, st, x, hist, B, S, P, len);
}

int conv(const Conv& L, const float* x, float* y, int B, int T, int Fin, int fstride, int act, const float* res, hipStream_t st,
         int* Fout_ret = nullptr) {
    ConvArgs p;
    p.x = x; p.w = L.w; p.scale = L.scale; p.shift = L.shift; p.res = res; p.y = y; p.hist = L.hist; p.t0 = L.t0;
    p.B = B; p.T = T; p.Fin = Fin; p.Cin = L.cin; p.Cout = L.cout; p.groups = L.groups; p.kt = L.kt; p.kf = L.kf; p.fstride = fstride;
    p.transposed = L.transposed; p.act = act;
    p.trk = L.trk; p.foff = L.foff;
    if (L.transposed) {
        p.fpad = L.kf / 2;
        p.Fout = (Fin - 1) * fstride - 2 * p.fpad + (L.kf - 1) + L.kf / 2 + 1;
    } else {
        p.fpad = L.kf / 2;
        p.Fout = (Fin + 2 * p.fpad - L.kf) / fstride + 1;
    }
    if (Fout_ret) *Fout_ret = p.Fout;
    const dim3 grid(grid_for((int64_t)B * T * p.Fout * p.Cout));
    if (L.trk && L.kt > 1) hipLaunchKernelGGL(k_dfn_conv<true>, grid, dim3(256), 0, st, p);        // kt = 1: a row reads its own row only
    else hipLaunchKernelGGL(k_dfn_conv<false>, grid, dim3(256), 0, st, p);
    if (L.hist) hist_push(x, L.hist, B, T, L.kt - 1, Fin * L.cin, st);
    return EGR_OK;
}

// x [rows][G * I] . w [G][I][O / G] -> y [rows][O]
int grouped_linear(const float* x, const float* w, float* y, int64_t rows, int in, int out, int G, hipStream_t st) {
    const int I = in / G, Oh = out / G;
    return egr_bgemm(x, w, y, 1, G, (int)rows, Oh, I, in, Oh, out, 0, I, 0, (int64_t)I * Oh, 0, Oh, 0, 1.f, st);
}

int rows_op(const float* a, const float* bias, const float* res, float* y, int64_t n, int cols, int act, hipStream_t st) {
    hipLaunchKernelGGL(k_dfn_rows, dim3(grid_for(n)), dim3(256), 0, st, a, bias, res, y, n, cols, act);
    return EGR_OK;
}

// ---- run stages, in the order both run()s call them; the models' own launches come between encoder_convs and erb_decoder_convs and
// ---- between erb_decoder_convs and df_pathway_and_coefs, their assemble kernel before synthesis
// Grows the workspace to `need` bytes on `st` and notes the call's shape; the caller lays its buffers out over m.ws afterwards.
int ensure_workspace(DfnCore& m, size_t need, int C, int nF, int64_t T, bool segmented, hipStream_t st, bool packed = false) {
    EGR_TRY(m.ws.grow(need, st));
    m.lastC = C; m.lastF = nF; m.lastT = T;
    m.segmented = segmented;
    m.packed = packed;
    return EGR_OK;
}

// analysis -> ERB dB -> the two norms (with the conv_lookahead shift whenever it is > 0) of the whole file
void features(const DfnCore& m, const float* x, int C, int nF, int64_t T, hipStream_t st) {
    const DfnDims& d = m.d;
    const Bufs& B = m.B;
    const int N = d.fft_size, E = d.nb_erb, nb = d.nb_df, la = d.conv_lookahead;
    const int64_t R = (int64_t)C * nF;
    hipLaunchKernelGGL(k_dfn_analysis<false>, dim3(nF, C), dim3(256), (size_t)N * 24, st, x, T, nF, (int64_t)0, N, d.hop_size, m.tw, m.win,
                       m.wnorm, B.spec, Tracks());
    hipLaunchKernelGGL(k_dfn_erb_db, dim3(grid_for(R * E)), dim3(256), 0, st, B.spec, R, m.Fq, E, m.band_lo, m.band_w, B.db);
    ScanArgs p{B.db, B.spec, B.ferb, B.fspec, nullptr, C, nF, 0, nF, nF, -la, nF - la > 0 ? nF - la : 0, nF, m.Fq, E, nb, la, 1, d.norm_alpha,
               nullptr};
    hipLaunchKernelGGL(k_dfn_norm_scan<false>, dim3((C * (E + nb) + 63) / 64), dim3(64), 0, st, p);
}

// The same over the R packed rows of a tracks call (m.tk): every track is a whole file of its own.
void features_tracks(const DfnCore& m, const float* x, int64_t R, hipStream_t st) {
    const DfnDims& d = m.d;
    const Bufs& B = m.B;
    const int N = d.fft_size, E = d.nb_erb, nb = d.nb_df, la = d.conv_lookahead;
    hipLaunchKernelGGL(k_dfn_analysis<true>, dim3((unsigned)R), dim3(256), (size_t)N * 24, st, x, (int64_t)0, 0, (int64_t)0, N, d.hop_size,
                       m.tw, m.win, m.wnorm, B.spec, m.tk);
    hipLaunchKernelGGL(k_dfn_erb_db, dim3(grid_for(R * E)), dim3(256), 0, st, B.spec, R, m.Fq, E, m.band_lo, m.band_w, B.db);
    ScanArgs p{B.db, B.spec, B.ferb, B.fspec, nullptr, m.tk.n, 0, 0, 0, 0, -la, 0, 0, m.Fq, E, nb, la, 1, d.norm_alpha, m.tk.foff};
    // one lane per (track, band / bin); not a grid-stride kernel (at most 2^18 tracks x 2113 lanes: the index fits an int)
    hipLaunchKernelGGL(k_dfn_norm_scan<true>, dim3((unsigned)(((int64_t)m.tk.n * (E + nb) + 63) / 64)), dim3(64), 0, st, p);
}

struct EncWidths { int F1 = 0, F2 = 0, F3 = 0, Fc = 0; };      // frequency widths of e1, e2, e3 and c1

// ferb -> e[0..3], fspec -> c0, c1
int encoder_convs(const DfnCore& m, const char* who, int C, int nF, EncWidths* w, hipStream_t st) {
    const Bufs& B = m.B;
    const int ch = m.d.conv_ch, E = m.d.nb_erb, nb = m.d.nb_df;
    EGR_TRY(conv(m.erb0, B.ferb, B.e[0], C, nF, E, 1, 1, nullptr, st));
    const int strides[3] = {2, 2, 1};
    int* Fo[3] = {&w->F1, &w->F2, &w->F3};
    int Fi = E;
    for (int i = 0; i < 3; ++i) {
        EGR_TRY(conv(m.erb_dw[i], B.e[i], B.tmp, C, nF, Fi, strides[i], 0, nullptr, st, Fo[i]));
        EGR_TRY(conv(m.erb_pw[i], B.tmp, B.e[i + 1], C, nF, *Fo[i], 1, 1, nullptr, st));
        Fi = *Fo[i];
    }
    EGR_TRY(conv(m.df0, (const float*)B.fspec, B.tmp, C, nF, nb, 1, 0, nullptr, st));
    EGR_TRY(conv(m.df0_pw, B.tmp, B.c0, C, nF, nb, 1, 1, nullptr, st));
    EGR_TRY(conv(m.df1_dw, B.c0, B.tmp, C, nF, nb, 2, 0, nullptr, st, &w->Fc));
    EGR_TRY(conv(m.df1_pw, B.tmp, B.c1, C, nF, w->Fc, 1, 1, nullptr, st));
    EGR_CHECK(w->F3 * ch == m.embd && w->Fc * ch == ch * nb / 2 && w->F1 == E / 2 && w->F2 == E / 4, EGR_ERR_UNSUPPORTED,
              "%s: encoder widths", who);
    return EGR_OK;
}

// demb (the ERB decoder's embedding) and e[3..0] -> mask
int erb_decoder_convs(const DfnCore& m, const char* who, int C, int nF, const EncWidths& w, hipStream_t st) {
    const Bufs& B = m.B;
    const int E = m.d.nb_erb;
    EGR_TRY(conv(m.path[3], B.e[3], B.pbuf, C, nF, w.F3, 1, 1, B.demb, st));
    EGR_TRY(conv(m.ct_dw[0], B.pbuf, B.tmp, C, nF, w.F3, 1, 0, nullptr, st));
    EGR_TRY(conv(m.ct_pw[0], B.tmp, B.dbuf, C, nF, w.F3, 1, 1, nullptr, st));
    for (int i = 0; i < 2; ++i) {             // convt2 (E/4 -> E/2) on conv2p(e2) + d, convt1 (E/2 -> E) on conv1p(e1) + d
        const int Fin = i == 0 ? w.F2 : w.F1, Fwant = i == 0 ? w.F1 : E;
        EGR_TRY(conv(m.path[2 - i], B.e[2 - i], B.pbuf, C, nF, Fin, 1, 1, B.dbuf, st));
        int Fo = 0;
        EGR_TRY(conv(m.ct_dw[1 + i], B.pbuf, B.tmp, C, nF, Fin, 2, 0, nullptr, st, &Fo));
        EGR_CHECK(Fo == Fwant, EGR_ERR_UNSUPPORTED, "%s: transposed conv width %d != %d", who, Fo, Fwant);
        EGR_TRY(conv(m.ct_pw[1 + i], B.tmp, B.dbuf, C, nF, Fo, 1, 1, nullptr, st));
    }
    EGR_TRY(conv(m.path[0], B.e[0], B.pbuf, C, nF, E, 1, 1, B.dbuf, st));
    return conv(m.out0, B.pbuf, B.mask, C, nF, E, 1, 2, nullptr, st);
}

// coefs = tanh(tcoef + bias) + df_convp(c0); tcoef is the model's df_out product, bias null without one
int df_pathway_and_coefs(const DfnCore& m, int C, int nF, const float* bias, hipStream_t st) {
    const Bufs& B = m.B;
    const int nb = m.d.nb_df, O2 = 2 * m.d.df_order;
    EGR_TRY(conv(m.convp, B.c0, B.cpt, C, nF, nb, 1, 0, nullptr, st));
    EGR_TRY(conv(m.convp_pw, B.cpt, B.cp, C, nF, nb, 1, 1, nullptr, st));
    return rows_op(B.tcoef, bias, B.cp, B.coefs, (int64_t)C * nF * nb * O2, nb * O2, 3, st);
}

// spec_e (written by the model's assemble kernel: nA frames from global frame asm_lo of nF) -> y[out_lo, out_lo + cnt).  The whole
// file: nA = nF, asm_lo = out_lo = 0, cnt = T.  A tracks call (m.tk): C = 1, nA = the packed rows, cnt = the samples of all tracks.
int synthesis(const DfnCore& m, int C, int nA, int64_t asm_lo, int64_t nF, int64_t T, int64_t out_lo, int64_t cnt, float* y,
              hipStream_t st) {
    const int N = m.d.fft_size;
    if (nA > 0)
        hipLaunchKernelGGL(k_dfn_synth, dim3(nA, C), dim3(256), (size_t)(m.Fq + N) * 16, st, m.B.spec_e, nA, N, m.tw, m.win, m.B.frames);
    if (cnt > 0 && m.tk.n)
        hipLaunchKernelGGL(k_dfn_ola<true>, dim3(grid_for((int64_t)C * cnt)), dim3(256), 0, st, m.B.frames, m.sg.frames_h, C, nA, asm_lo, nF,
                           N, m.d.hop_size, T, out_lo, cnt, y, m.tk);
    else if (cnt > 0)
        hipLaunchKernelGGL(k_dfn_ola<false>, dim3(grid_for((int64_t)C * cnt)), dim3(256), 0, st, m.B.frames, m.sg.frames_h, C, nA, asm_lo, nF,
                           N, m.d.hop_size, T, out_lo, cnt, y, Tracks());
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

// The arguments of the models' assemble kernels: nA frames from asm_lo; spec holds nS frames from spec_lo, mask / coefs / alpha S
// frames from a (one-pass: everything the whole file from 0; a tracks call: C = 1 and the packed rows as one file from 0).
AsmArgs assemble_args(const DfnCore& m, const float* alpha, int C, int64_t nF, int64_t asm_lo, int nA, int64_t spec_lo, int nS,
                      int64_t a, int S) {
    const DfnDims& d = m.d;
    const Bufs& B = m.B;
    AsmArgs p;
    p.spec = B.spec; p.mask = B.mask; p.coefs = B.coefs; p.alpha = alpha;
    p.mask_h = m.sg.mask_h; p.coefs_h = m.sg.coefs_h; p.alpha_h = m.sg.alpha_h; p.band_of = m.band_of; p.out = B.spec_e;
    p.nF = nF; p.asm_lo = asm_lo; p.spec_lo = spec_lo; p.a = a;
    p.C = C; p.nA = nA; p.nS = nS; p.S = S; p.P_m = d.df_order - 1; p.Fq = m.Fq; p.E = d.nb_erb; p.nbdf = d.nb_df; p.order = d.df_order;
    p.look = d.df_lookahead;
    p.trk = m.tk.trk; p.foff = m.tk.foff;
    return p;
}

// ---- create stages
// The range checks both models make; `who` is the model's prefix in the messages ("egr_dfn3" / "egr_dfn2").
int check_common(const DfnDims& d, const char* who) {
    const int E = d.nb_erb, nb = d.nb_df, ch = d.conv_ch, O2 = 2 * d.df_order;
    EGR_CHECK(d.fft_size > 0 && d.hop_size > 0 && d.fft_size % d.hop_size == 0 && d.fft_size % 2 == 0 && d.fft_size <= 4096, EGR_ERR_UNSUPPORTED,
              "%s: fft_size %d / hop_size %d", who, d.fft_size, d.hop_size);
    EGR_CHECK(E > 0 && E <= EGR_DFN3_MAX_ERB && E % 4 == 0 && nb > 0 && nb % 2 == 0 && nb <= d.fft_size / 2 + 1, EGR_ERR_UNSUPPORTED,
              "%s: nb_erb %d / nb_df %d", who, E, nb);
    EGR_CHECK(d.emb_hidden_dim > 0 && d.emb_hidden_dim <= GRU_HMAX && d.df_hidden_dim > 0 && d.df_hidden_dim <= GRU_HMAX,
              EGR_ERR_UNSUPPORTED, "%s: GRU widths must be <= %d", who, GRU_HMAX);
    EGR_CHECK(d.emb_num_layers >= 2 && d.df_num_layers >= 1 && d.emb_num_layers + d.df_num_layers <= EGR_DFN3_MAX_GRU, EGR_ERR_UNSUPPORTED,
              "%s: GRU layer counts", who);
    EGR_CHECK(d.df_order >= 1 && d.df_lookahead >= 0 && d.df_lookahead < d.df_order && d.conv_lookahead >= 0, EGR_ERR_UNSUPPORTED,
              "%s: df_order / lookaheads", who);
    EGR_CHECK(ch > 0 && d.path_groups > 0 && ch % d.path_groups == 0 && d.df_path_groups > 0 && ch % d.df_path_groups == 0 &&
              O2 % d.df_path_groups == 0, EGR_ERR_UNSUPPORTED, "%s: conv groups", who);
    // a stride-2 transposed conv with padding kf / 2 and output_padding kf / 2 doubles the width only for kf = 3 (torch refuses
    // output_padding >= stride for the wider kernels)
    EGR_CHECK(d.convt_kf == 3, EGR_ERR_UNSUPPORTED, "%s: transposed conv kernel width %d (supported: 3)", who, d.convt_kf);
    EGR_CHECK(d.kf % 2 == 1 && d.kf_inp % 2 == 1 && d.kt >= 1 && d.kt_inp >= 1 && d.df_pathway_kt >= 1, EGR_ERR_UNSUPPORTED,
              "%s: frequency kernels must be odd (same-size padding)", who);
    int wsum = 0;
    for (int e = 0; e < E; ++e) { EGR_CHECK(d.erb_widths[e] > 0, EGR_ERR_ARG, "%s: ERB width %d", who, e); wsum += d.erb_widths[e]; }
    EGR_CHECK(wsum == d.fft_size / 2 + 1, EGR_ERR_ARG, "%s: ERB widths sum %d != %d", who, wsum, d.fft_size / 2 + 1);
    return EGR_OK;
}

void init_core(DfnCore& m, const DfnDims& d, int device) {
    m.d = d;
    m.device = device;
    m.Fq = d.fft_size / 2 + 1;
    m.embd = d.conv_ch * d.nb_erb / 4;
    m.wnorm = 1.f / ((float)d.fft_size * (float)d.fft_size / (float)(2 * d.hop_size));
}

// Walks the packed weights in pack order (dfn_weights.pack_order / dfn2_weights.pack_order): W(k) takes the next k floats and returns
// their offset, cv / bn describe a convolution and the BatchNorm affine behind it.  The three conv stacks are the shared fragments of
// the pack order; the models take their linears and GRUs with W between them.
struct WeightCursor {
    struct ConvSpec { Conv* L; int64_t w, s, t; };
    int64_t pos = 0;                                        // floats consumed so far
    std::vector<ConvSpec> convs;
    int64_t W(int64_t k) { pos += k; return pos - k; }
    void cv(Conv& L, int cin, int cout, int groups, int kt, int kf, int transposed = 0) {
        L.cin = cin; L.cout = cout; L.groups = groups; L.kt = kt; L.kf = kf; L.transposed = transposed;
        convs.push_back({&L, W((int64_t)(transposed ? cin * (cout / groups) : cout * (cin / groups)) * kt * kf), -1, -1});
    }
    void bn(int n) { ConvSpec& s = convs.back(); s.s = W(n); s.t = W(n); }
    void encoder_convs(DfnCore& m) {
        const DfnDims& d = m.d;
        const int ch = d.conv_ch;
        cv(m.erb0, 1, ch, 1, d.kt_inp, d.kf_inp); bn(ch);
        for (int i = 0; i < 3; ++i) { cv(m.erb_dw[i], ch, ch, ch, d.kt, d.kf); cv(m.erb_pw[i], ch, ch, 1, 1, 1); bn(ch); }
        cv(m.df0, 2, ch, 2, d.kt_inp, d.kf_inp); cv(m.df0_pw, ch, ch, 1, 1, 1); bn(ch);
        cv(m.df1_dw, ch, ch, ch, d.kt, d.kf); cv(m.df1_pw, ch, ch, 1, 1, 1); bn(ch);
    }
    void erb_decoder_convs(DfnCore& m) {
        const DfnDims& d = m.d;
        const int ch = d.conv_ch;
        for (int i = 0; i < 3; ++i) {
            cv(m.path[3 - i], ch, ch, d.path_groups, 1, 1); bn(ch);
            if (i == 0) cv(m.ct_dw[0], ch, ch, ch, d.kt, d.kf);
            else cv(m.ct_dw[i], ch, ch, ch, 1, d.convt_kf, 1);
            cv(m.ct_pw[i], ch, ch, 1, 1, 1); bn(ch);
        }
        cv(m.path[0], ch, ch, d.path_groups, 1, 1); bn(ch);
        cv(m.out0, ch, 1, 1, d.kt, d.kf); bn(1);
    }
    void df_pathway_convs(DfnCore& m) {
        const int O2 = 2 * m.d.df_order;
        cv(m.convp, m.d.conv_ch, O2, m.d.df_path_groups, m.d.df_pathway_kt, 1);
        cv(m.convp_pw, O2, O2, 1, 1, 1); bn(O2);
    }
};

constexpr int64_t DENSE_WHH_FLOATS = (int64_t)GRU_PER_THREAD * GRU_THREADS;

// W_hh [3H][H] -> thread-minor (element, thread) order of k_dfn_gru, DENSE_WHH_FLOATS floats
void repack_dense_whh(const float* w, int H, float* dst) {
    for (int t = 0; t < GRU_THREADS; ++t)
        for (int e = 0; e < GRU_PER_THREAD; ++e) {
            const int j = e / GRU_K, k = e % GRU_K;
            const int q = j * GRU_THREADS + t, row = q / GRU_SEG, col = GRU_SEG * k + q % GRU_SEG;
            dst[(int64_t)e * GRU_THREADS + t] = (row < 3 * H && col < H) ? w[(int64_t)row * H + col] : 0.f;
        }
}

// device image: packed weights | repacked W_hh per layer (the model fills [align64(n_floats), o_tw)) | twiddles (double2) | window |
// band tables (band_lo [E], band_w [E], band_of [Fq])
struct Image {
    std::vector<float> host;
    int64_t o_tw = 0, o_win = 0, o_tab = 0;
};

Image build_tables(const DfnDims& d, const float* packed, int64_t n_floats, int64_t o_tw) {
    const int N = d.fft_size, E = d.nb_erb;
    Image im;
    im.o_tw = o_tw;
    im.o_win = o_tw + 4LL * N;
    im.o_tab = im.o_win + N;
    im.host.assign((size_t)(im.o_tab + 2 * E + N / 2 + 1), 0.f);
    memcpy(im.host.data(), packed, sizeof(float) * n_floats);
    double* twd = (double*)(im.host.data() + im.o_tw);
    for (int n = 0; n < N; ++n) {
        twd[2 * n] = cos(2.0 * M_PI * n / N);
        twd[2 * n + 1] = sin(2.0 * M_PI * n / N);
    }
    const int h = N / 2;
    for (int n = 0; n < N; ++n) {
        const double s = sin(0.5 * M_PI * (n + 0.5) / h);
        im.host[im.o_win + n] = (float)sin(0.5 * M_PI * s * s);
    }
    int* tab = (int*)(im.host.data() + im.o_tab);
    int lo = 0;
    for (int e = 0; e < E; ++e) {
        tab[e] = lo;
        tab[E + e] = d.erb_widths[e];
        for (int j = 0; j < d.erb_widths[e]; ++j) tab[2 * E + lo + j] = e;
        lo += d.erb_widths[e];
    }
    return im;
}

// The image onto m.device as m.dev_w, and the dynamic-LDS cap of the analysis / synthesis kernels.  `who` is the create function's
// name.  On failure nothing stays allocated; either way the device that was current is current again.
int upload(DfnCore& m, const char* who, const Image& im) {
    const size_t bytes = sizeof(float) * im.host.size();
    DeviceScope dev(m.device);
    if (!dev.ok || hipMalloc(&m.dev_w, bytes) != hipSuccess || hipMemcpy(m.dev_w, im.host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("%s: device allocation / upload failed on device %d", who, m.device);
        if (m.dev_w) (void)hipFree(m.dev_w);
        m.dev_w = nullptr;
        return EGR_ERR_HIP;
    }
    // the analysis / synthesis DFTs keep a frame and the twiddles in dynamic LDS: 24 N and 16 (1.5 N + 1) bytes, above the 64 KiB
    // default from N = 2732 on.  The attribute is a process-wide cap per kernel, so it is raised to the CU's maximum (as the Fat-Llama
    // plans do), never to this config's need.
    const int N = m.d.fft_size;
    const size_t lds_an = (size_t)N * 24, lds_syn = (size_t)(m.Fq + N) * 16;
    hipError_t ea = hipSuccess;
    if (lds_an > (size_t)DFN_LDS_MAX || lds_syn > (size_t)DFN_LDS_MAX) {
        set_error("%s: fft_size %d needs %zu / %zu bytes of LDS (limit %d)", who, N, lds_an, lds_syn, DFN_LDS_MAX);
        ea = hipErrorInvalidValue;
    }
    if (ea == hipSuccess) ea = hipFuncSetAttribute((const void*)k_dfn_analysis<false>, hipFuncAttributeMaxDynamicSharedMemorySize, DFN_LDS_MAX);
    if (ea == hipSuccess) ea = hipFuncSetAttribute((const void*)k_dfn_analysis<true>, hipFuncAttributeMaxDynamicSharedMemorySize, DFN_LDS_MAX);
    if (ea == hipSuccess) ea = hipFuncSetAttribute((const void*)k_dfn_synth, hipFuncAttributeMaxDynamicSharedMemorySize, DFN_LDS_MAX);
    if (ea != hipSuccess) {
        if (lds_an <= (size_t)DFN_LDS_MAX && lds_syn <= (size_t)DFN_LDS_MAX)
            set_error("%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize) -> %s", who, hipGetErrorString(ea));
        (void)hipFree(m.dev_w);
        m.dev_w = nullptr;
        return EGR_ERR_HIP;
    }
    return EGR_OK;
}

// Points the convolutions and the tables into the uploaded image.
void bind(DfnCore& m, const WeightCursor& wc, const Image& im) {
    float* D = m.dev_w;
    for (const auto& s : wc.convs) {
        s.L->w = D + s.w;
        if (s.s >= 0) { s.L->scale = D + s.s; s.L->shift = D + s.t; }
    }
    m.tw = (const double2*)(D + im.o_tw);
    m.win = D + im.o_win;
    m.band_lo = (const int*)(D + im.o_tab);
    m.band_w = m.band_lo + m.d.nb_erb;
    m.band_of = m.band_lo + 2 * m.d.nb_erb;
}

// ---- entry-point bodies; `who` is the extern "C" function's name
constexpr int64_t MAX_FRAMES = 2147483647LL / 4096;          // frames of one pass (a whole file, or a segment with the rows around it)

// `whole`: a one-pass call, the file's frames are bounded; a segmented call bounds its segments instead (seg_clamp)
int enhance_checks(const DfnCore* m, const char* who, const float* x48, int channels, int64_t n, const float* y, bool whole = true) {
    EGR_CHECK(m && x48 && y && channels >= 1 && channels <= 65535 && n >= 1, EGR_ERR_ARG, "%s: bad argument", who);
    // nF * 4096 fits an int (which also keeps nF below 65535 * 4096)
    EGR_CHECK(!whole || m->frames_of(n) <= MAX_FRAMES, EGR_ERR_UNSUPPORTED, "%s: input too long", who);
    return check_current_device(who, m->device);
}

void destroy(DfnCore& m) {
    DeviceScope dev(m.device);
    m.ws.release();
    m.stage.release();
    if (m.dev_w) (void)hipFree(m.dev_w);
}

static_assert(EGR_DFN2_STAGE_GRU0 == EGR_DFN3_STAGE_GRU0, "one GRU stage range for both models");

// The stages both models keep in the shared buffers (all but EMB), GRU layer g at EGR_DFN3_STAGE_GRU0 + g; false: not one of them.
bool stage_common(const DfnCore& m, int stage, const float** src, int64_t* n) {
    const int64_t R = (int64_t)m.lastC * m.lastF;
    const DfnDims& d = m.d;
    const Bufs& B = m.B;
    switch (stage) {
        case EGR_DFN3_STAGE_SPEC: *src = (const float*)B.spec; *n = R * m.Fq * 2; return true;
        case EGR_DFN3_STAGE_FEAT_ERB: *src = B.ferb; *n = R * d.nb_erb; return true;
        case EGR_DFN3_STAGE_FEAT_SPEC: *src = (const float*)B.fspec; *n = R * d.nb_df * 2; return true;
        case EGR_DFN3_STAGE_E0: *src = B.e[0]; *n = R * d.nb_erb * d.conv_ch; return true;
        case EGR_DFN3_STAGE_E1: *src = B.e[1]; *n = R * (d.nb_erb / 2) * d.conv_ch; return true;
        case EGR_DFN3_STAGE_E2: *src = B.e[2]; *n = R * (d.nb_erb / 4) * d.conv_ch; return true;
        case EGR_DFN3_STAGE_E3: *src = B.e[3]; *n = R * (d.nb_erb / 4) * d.conv_ch; return true;
        case EGR_DFN3_STAGE_C0: *src = B.c0; *n = R * d.nb_df * d.conv_ch; return true;
        case EGR_DFN3_STAGE_MASK: *src = B.mask; *n = R * d.nb_erb; return true;
        case EGR_DFN3_STAGE_COEFS: *src = B.coefs; *n = R * d.nb_df * 2 * d.df_order; return true;
        case EGR_DFN3_STAGE_SPEC_E: *src = (const float*)B.spec_e; *n = R * m.Fq * 2; return true;
    }
    if (stage < EGR_DFN3_STAGE_GRU0 || stage >= EGR_DFN3_STAGE_GRU0 + m.ngru()) return false;
    *src = B.gout[stage - EGR_DFN3_STAGE_GRU0];
    *n = R * m.gru_width(stage - EGR_DFN3_STAGE_GRU0);
    return true;
}

// own(stage, &src, &n) names the model's own stages (it is asked first and leaves src null for every other)
template <class Own>
int stage_copy(const DfnCore& m, const char* who, int stage, float* dst, int64_t capacity, int64_t* count, void* stream, Own own) {
    EGR_CHECK(m.ws.p, EGR_ERR_ARG, "%s: no enhance call yet", who);
    EGR_CHECK(!m.segmented, EGR_ERR_ARG, "%s: the last call was segmented; stages belong to one-pass calls", who);
    EGR_CHECK(!m.packed, EGR_ERR_ARG, "%s: the last call was a tracks call; stages belong to one-pass calls", who);
    const float* src = nullptr;
    int64_t n = 0;
    own(stage, &src, &n);
    EGR_CHECK(src || stage_common(m, stage, &src, &n), EGR_ERR_ARG, "%s: unknown stage %d", who, stage);
    return stage_copy_out(who, src, n, dst, capacity, count, stream);
}

// One recurrence layer alone on zero projections: launch(proj, out, sum, nF) runs it for nF steps on the null stream; a short warm-up
// launch, then the timed one.  sum is room for DeepFilterNet2's running sum when with_sum, else null.
template <class Launch>
int time_gru_harness(const DfnCore* m, const char* who, int layer, int channels, int64_t steps, bool with_sum, double* us_per_step,
                     Launch launch) {
    EGR_CHECK(m && us_per_step && channels >= 1 && channels <= 64 && steps >= 1 && steps <= 10000000, EGR_ERR_ARG, "%s: bad argument", who);
    EGR_CHECK(layer >= 0 && layer < m->ngru(), EGR_ERR_ARG, "%s: layer %d", who, layer);
    const size_t nh = (size_t)channels * steps * m->gru_width(layer);
    float *proj = nullptr, *out = nullptr;
    hipEvent_t e0, e1;
    EGR_HIP(hipMalloc(&proj, sizeof(float) * 3 * nh));
    EGR_HIP(hipMalloc(&out, sizeof(float) * (with_sum ? 2 : 1) * nh));
    float* sum = with_sum ? out + nh : nullptr;
    EGR_HIP(hipMemset(proj, 0, sizeof(float) * 3 * nh));
    EGR_HIP(hipEventCreate(&e0));
    EGR_HIP(hipEventCreate(&e1));
    launch(proj, out, sum, (int)(steps < 64 ? steps : 64));
    EGR_HIP(hipEventRecord(e0, 0));
    launch(proj, out, sum, (int)steps);
    EGR_HIP(hipEventRecord(e1, 0));
    EGR_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    EGR_HIP(hipEventElapsedTime(&ms, e0, e1));
    *us_per_step = 1e3 * ms / (double)steps;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(proj);
    (void)hipFree(out);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

// ------------------------------------------------------------------------------------------------ DeepFilterNet3
struct Gru {
    const float* wih = nullptr; const float* bih = nullptr; const float* bhh = nullptr; float* whh_pk = nullptr;
    int in = 0, H = 0;
    float* hst = nullptr;                   // a segmented call only: the state [C][H] across the cuts
    const int* foff = nullptr; int ntr = 0; // a tracks call only: Tracks::foff and the number of tracks (one workgroup each)
};

// One dense layer over nF steps of C channels, or (foff) over the ntr tracks' own rows; h: the carried state or null.
void launch_gru(const float* proj, const float* whh_pk, const float* bhh, int H, int C, int nF, float* out, float* h, const int* foff,
                int ntr, hipStream_t st) {
    if (foff)
        hipLaunchKernelGGL(k_dfn_gru<true>, dim3(ntr), dim3(GRU_THREADS), 0, st, proj, whh_pk, bhh, H, 0, out, (const float*)nullptr,
                           (float*)nullptr, foff);
    else
        hipLaunchKernelGGL(k_dfn_gru<false>, dim3(C), dim3(GRU_THREADS), 0, st, proj, whh_pk, bhh, H, nF, out, (const float*)h, h,
                           (const int*)nullptr);
}

struct Dfn3 {
    egr_dfn3_config cfg;
    DfnCore core;
    const float *fc_emb = nullptr, *enc_lin_in = nullptr, *enc_lin_out = nullptr, *erb_lin_in = nullptr, *erb_lin_out = nullptr;
    const float *df_lin_in = nullptr, *df_skip = nullptr, *df_out = nullptr;
    std::vector<Gru> grus;
    struct Extra { float *emb, *gx; } X;
};

void layout(const Dfn3& m, const Rows& rows, Take& take, Bufs& B, Dfn3::Extra& X) {
    const int64_t R = rows.net;
    const int Hm = m.cfg.emb_hidden_dim > m.cfg.df_hidden_dim ? m.cfg.emb_hidden_dim : m.cfg.df_hidden_dim;
    layout_common(m.core, rows, take, B);
    X.emb = take(R * m.core.embd);
    X.gx = take(R * Hm);
}

// x [C * nF][in] -> out [C * nF][H] through one GRU layer
int gru_layer(const Gru& g, const float* x, float* proj, float* out, int C, int nF, hipStream_t st) {
    const int64_t R = (int64_t)C * nF;
    EGR_TRY(egr_bgemm(x, g.wih, proj, 1, 1, (int)R, 3 * g.H, g.in, g.in, g.in, 3 * g.H, 0, 0, 0, 0, 0, 0, 1, 1.f, st));
    EGR_TRY(rows_op(proj, g.bih, nullptr, proj, R * 3 * g.H, 3 * g.H, 0, st));
    launch_gru(proj, g.whh_pk, g.bhh, g.H, C, nF, out, g.hst, g.foff, g.ntr, st);
    return EGR_OK;
}

// features (ferb, fspec) -> mask, coefs over nF frames of C channels: the whole file, or one segment; or, with the tables bound
// (bind_tracks), over C = 1 x nF = R packed rows
int network(Dfn3& m, int C, int nF, hipStream_t st) {
    const egr_dfn3_config& c = m.cfg;
    DfnCore& k = m.core;
    const char* who = "egr_dfn3";
    const int64_t R = (int64_t)C * nF;
    const int nb = c.nb_df, O2 = 2 * c.df_order, embd = k.embd;
    Bufs& B = k.B;
    Dfn3::Extra& X = m.X;
    EncWidths w;
    EGR_TRY(encoder_convs(k, who, C, nF, &w, st));
    EGR_TRY(grouped_linear(B.c1, m.fc_emb, B.emb0, R, w.Fc * c.conv_ch, embd, c.enc_lin_groups, st));
    EGR_TRY(rows_op(B.emb0, nullptr, B.e[3], B.emb0, R * embd, embd, 1, st));      // emb = e3 + relu(fc_emb(c1))
    const int He = c.emb_hidden_dim, Hd = c.df_hidden_dim;
    int g = 0;
    EGR_TRY(grouped_linear(B.emb0, m.enc_lin_in, X.gx, R, embd, He, c.lin_groups, st));
    EGR_TRY(rows_op(X.gx, nullptr, nullptr, X.gx, R * He, He, 1, st));
    EGR_TRY(gru_layer(m.grus[g], X.gx, B.proj, B.gout[g], C, nF, st));
    EGR_TRY(grouped_linear(B.gout[g], m.enc_lin_out, X.emb, R, He, embd, c.lin_groups, st));
    EGR_TRY(rows_op(X.emb, nullptr, nullptr, X.emb, R * embd, embd, 1, st));
    ++g;
    // ERB decoder
    EGR_TRY(grouped_linear(X.emb, m.erb_lin_in, X.gx, R, embd, He, c.lin_groups, st));
    EGR_TRY(rows_op(X.gx, nullptr, nullptr, X.gx, R * He, He, 1, st));
    const float* xin = X.gx;
    for (int l = 0; l < c.emb_num_layers - 1; ++l, ++g) {
        EGR_TRY(gru_layer(m.grus[g], xin, B.proj, B.gout[g], C, nF, st));
        xin = B.gout[g];
    }
    EGR_TRY(grouped_linear(xin, m.erb_lin_out, B.demb, R, He, embd, c.lin_groups, st));
    EGR_TRY(rows_op(B.demb, nullptr, nullptr, B.demb, R * embd, embd, 1, st));
    EGR_TRY(erb_decoder_convs(k, who, C, nF, w, st));
    // DF decoder
    EGR_TRY(grouped_linear(X.emb, m.df_lin_in, X.gx, R, embd, Hd, c.lin_groups, st));
    EGR_TRY(rows_op(X.gx, nullptr, nullptr, X.gx, R * Hd, Hd, 1, st));
    xin = X.gx;
    for (int l = 0; l < c.df_num_layers; ++l, ++g) {
        EGR_TRY(gru_layer(m.grus[g], xin, B.proj, B.gout[g], C, nF, st));
        xin = B.gout[g];
    }
    if (m.df_skip) {
        EGR_TRY(grouped_linear(X.emb, m.df_skip, B.dfc, R, embd, Hd, c.lin_groups, st));
        EGR_TRY(rows_op(B.dfc, nullptr, xin, B.dfc, R * Hd, Hd, 0, st));
        xin = B.dfc;
    }
    EGR_TRY(grouped_linear(xin, m.df_out, B.tcoef, R, Hd, nb * O2, c.lin_groups, st));
    return df_pathway_and_coefs(k, C, nF, nullptr, st);                              // tanh(df_out(c)) + df_convp(c0)
}

// mask + deep filter
void assemble(const Dfn3& m, const AsmArgs& p, hipStream_t st) {
    const dim3 grid(grid_for((int64_t)p.C * p.nA * p.Fq));
    if (p.trk) hipLaunchKernelGGL(k_dfn_assemble<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_dfn_assemble<false>, grid, dim3(256), 0, st, p);
}

// ------------------------------------------------------------------------------------------------ DeepFilterNet2
struct GGru {                 // one GroupedGRU layer: G GRUs of width h on input slices of width in / G
    const float* wih = nullptr; const float* bih = nullptr; const float* bhh = nullptr; float* whh_pk = nullptr;
    int in = 0, H = 0, G = 1, h = 0, K = 0, S = 1, shuffle = 0;
    float* hst = nullptr;                   // a segmented call only: the state [C][H] across the cuts, groups in pre-shuffle order
    const int* foff = nullptr; int ntr = 0; // a tracks call only: Tracks::foff and the number of tracks (gru_groups workgroups each)
    bool dense() const { return h > G2_HMAX; }
};

// K (16 or 32 columns per lane) and S (lanes per gate row) of k_dfn2_gru for a group width h <= G2_HMAX
inline void ggru_shape(int h, int* K, int* S) {
    *K = h <= 16 ? 16 : 32;
    *S = 1;
    while (*K * *S < h) *S *= 2;
}

struct Dfn2 {
    egr_dfn2_config cfg;
    DfnCore core;
    const float *fc_emb_w = nullptr, *fc_emb_b = nullptr, *erb_fc_w = nullptr, *erb_fc_b = nullptr;
    const float *df_skip = nullptr, *df_out = nullptr, *df_out_b = nullptr, *fc_a_w = nullptr, *fc_a_b = nullptr;
    std::vector<GGru> grus;
    struct Extra { float *lin, *gsum[EGR_DFN3_MAX_GRU], *alpha; } X;
};

void layout(const Dfn2& m, const Rows& rows, Take& take, Bufs& B, Dfn2::Extra& X) {
    const DfnCore& k = m.core;
    const int64_t R = rows.net;
    const int no = m.cfg.nb_df * 2 * m.cfg.df_order;
    layout_common(k, rows, take, B);
    X.lin = take(R * (k.embd > no ? k.embd : no));
    for (int g = 0; g < EGR_DFN3_MAX_GRU; ++g) X.gsum[g] = g < k.ngru() ? take(R * k.gru_width(g)) : nullptr;
    X.alpha = take(R);
}

int epi(const float* a, const float* bias, const float* res, float* y, int64_t n, int cols, int G, int act, hipStream_t st) {
    hipLaunchKernelGGL(k_dfn2_epi, dim3(grid_for(n)), dim3(256), 0, st, a, bias, res, y, n, cols, G, act);
    return EGR_OK;
}

// GroupedLinear (P3): x [rows][in] . per-group nn.Linear weight [G][out / G][in / G] (torch layout) -> lin, then the epilogue into y
int glinear(const float* x, const float* w, const float* bias, float* lin, float* y, int64_t rows, int in, int out, int G, int shuf,
            int act, const float* res, hipStream_t st) {
    const int I = in / G, Oh = out / G;
    EGR_TRY(egr_bgemm(x, w, lin, 1, G, (int)rows, Oh, I, in, I, out, 0, I, 0, (int64_t)Oh * I, 0, Oh, 1, 1.f, st));
    return epi(lin, bias, res, y, rows * out, out, shuf ? G : 1, act, st);
}

template <int K>
void launch_ggru_k(const GGru& g, const float* proj, const float* sum_in, float* out, float* sum_out, int C, int nF, hipStream_t st) {
    const dim3 block(g.h * g.S);
    if (g.foff)
        hipLaunchKernelGGL((k_dfn2_gru<K, true>), dim3((unsigned)g.G * g.ntr), block, 0, st, proj, g.whh_pk, g.bih, g.bhh, g.G, g.h, g.S, 0,
                           g.shuffle, sum_in, out, sum_out, (const float*)nullptr, (float*)nullptr, g.foff);
    else
        hipLaunchKernelGGL((k_dfn2_gru<K, false>), dim3(g.G, C), block, 0, st, proj, g.whh_pk, g.bih, g.bhh, g.G, g.h, g.S, nF, g.shuffle,
                           sum_in, out, sum_out, (const float*)g.hst, g.hst, (const int*)nullptr);
}

void launch_ggru(const GGru& g, const float* proj, const float* sum_in, float* out, float* sum_out, int C, int nF, hipStream_t st) {
    if (g.K == 16) launch_ggru_k<16>(g, proj, sum_in, out, sum_out, C, nF, st);
    else launch_ggru_k<32>(g, proj, sum_in, out, sum_out, C, nF, st);
}

// x [C * nF][in] -> out (the layer output as passed on) and sum_out (= sum_in + out) [C * nF][H] through one GroupedGRU layer
int ggru_layer(const GGru& g, const float* x, float* proj, const float* sum_in, float* out, float* sum_out, int C, int nF, hipStream_t st) {
    const int64_t R = (int64_t)C * nF;
    const int I = g.in / g.G, h3 = 3 * g.h;
    EGR_TRY(egr_bgemm(x, g.wih, proj, 1, g.G, (int)R, h3, I, g.in, I, 3 * g.H, 0, I, 0, (int64_t)h3 * I, 0, h3, 1, 1.f, st));
    if (g.dense()) {                       // G = 1 and H > 128: a plain nn.GRU layer, no shuffle
        EGR_TRY(rows_op(proj, g.bih, nullptr, proj, R * 3 * g.H, 3 * g.H, 0, st));
        launch_gru(proj, g.whh_pk, g.bhh, g.H, C, nF, out, g.hst, g.foff, g.ntr, st);
        return rows_op(out, nullptr, sum_in, sum_out, R * g.H, g.H, 0, st);
    }
    launch_ggru(g, proj, sum_in, out, sum_out, C, nF, st);
    return EGR_OK;
}

// features (ferb, fspec) -> mask, coefs, alpha over nF frames of C channels: the whole file, or one segment
int network(Dfn2& m, int C, int nF, hipStream_t st) {
    const egr_dfn2_config& c = m.cfg;
    DfnCore& k = m.core;
    const char* who = "egr_dfn2";
    const int64_t R = (int64_t)C * nF;
    const int nb = c.nb_df, O2 = 2 * c.df_order, Hd = c.df_hidden_dim;
    Bufs& B = k.B;
    Dfn2::Extra& X = m.X;
    EncWidths w;
    EGR_TRY(encoder_convs(k, who, C, nF, &w, st));                                    // P2
    // emb0 = e3 + GroupedLinear(c1) (no activation)
    EGR_TRY(glinear(B.c1, m.fc_emb_w, m.fc_emb_b, X.lin, B.emb0, R, w.Fc * c.conv_ch, k.embd, c.lin_groups, c.group_shuffle, 0, B.e[3], st));
    size_t g = 0;
    EGR_TRY(ggru_layer(m.grus[g], B.emb0, B.proj, nullptr, B.gout[g], X.gsum[g], C, nF, st));
    const float* emb = X.gsum[g];
    ++g;
    // ERB decoder (P5)
    const float* xin = emb;
    const float* sum = nullptr;
    for (int l = 0; l < c.emb_num_layers - 1; ++l, ++g) {
        EGR_TRY(ggru_layer(m.grus[g], xin, B.proj, sum, B.gout[g], X.gsum[g], C, nF, st));
        xin = B.gout[g];
        sum = X.gsum[g];
    }
    EGR_TRY(glinear(sum, m.erb_fc_w, m.erb_fc_b, X.lin, B.demb, R, c.emb_hidden_dim, k.embd, c.lin_groups, c.group_shuffle, 1, nullptr, st));
    EGR_TRY(erb_decoder_convs(k, who, C, nF, w, st));
    // DF decoder (P6)
    xin = emb;
    sum = nullptr;
    for (int l = 0; l < c.df_num_layers; ++l, ++g) {
        EGR_TRY(ggru_layer(m.grus[g], xin, B.proj, sum, B.gout[g], X.gsum[g], C, nF, st));
        xin = B.gout[g];
        sum = X.gsum[g];
    }
    if (m.df_skip) {
        EGR_TRY(grouped_linear(emb, m.df_skip, B.dfc, R, c.emb_hidden_dim, Hd, c.lin_groups, st));
        EGR_TRY(rows_op(sum, nullptr, B.dfc, B.dfc, R * Hd, Hd, 0, st));            // c = s + skip(emb)
        sum = B.dfc;
    }
    hipLaunchKernelGGL(k_dfn2_alpha, dim3(grid_for(R)), dim3(256), 0, st, sum, m.fc_a_w, m.fc_a_b, R, Hd, X.alpha);
    if (c.df_output_layer == 1)
        EGR_TRY(egr_bgemm(sum, m.df_out, B.tcoef, 1, 1, (int)R, nb * O2, Hd, Hd, Hd, nb * O2, 0, 0, 0, 0, 0, 0, 1, 1.f, st));
    else
        EGR_TRY(grouped_linear(sum, m.df_out, B.tcoef, R, Hd, nb * O2, c.lin_groups, st));
    return df_pathway_and_coefs(k, C, nF, m.df_out_b, st);                           // tanh(df_out(c)) + df_convp(c0)
}

// mask, then deep filter (P7)
void assemble(const Dfn2& m, const AsmArgs& p, hipStream_t st) {
    const dim3 grid(grid_for((int64_t)p.C * p.nA * p.Fq));
    if (p.trk) hipLaunchKernelGGL(k_dfn2_assemble<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_dfn2_assemble<false>, grid, dim3(256), 0, st, p);
}

inline const float* alpha_of(const Dfn3&) { return nullptr; }
inline const float* alpha_of(const Dfn2& m) { return m.X.alpha; }

// ------------------------------------------------------------------------------------------------ the two ways to run a file
// One pass: every buffer holds the whole file.
template <class M>
size_t workspace_need(const M& m, int C, int nF) {           // measures only: the handle's buffers stay those of the last call
    Bufs B;
    typename M::Extra X;
    Take take{nullptr};
    const int64_t R = (int64_t)C * nF;
    layout(m, Rows{R, R, R}, take, B, X);
    return take.off;
}

// The convolutions with kt > 1 possible, each with the frequency width of its input: the consumers that carry kt - 1 rows.
template <class Core, class ConvT>
void hist_convs(Core& k, ConvT* c[N_HIST_CONV], int fin[N_HIST_CONV]) {
    const int E = k.d.nb_erb, nb = k.d.nb_df;
    ConvT* cs[N_HIST_CONV] = {&k.erb0, &k.df0, &k.erb_dw[0], &k.erb_dw[1], &k.erb_dw[2], &k.df1_dw, &k.ct_dw[0], &k.out0, &k.convp};
    const int fs[N_HIST_CONV] = {E, nb, E, E / 2, E / 4, nb, E / 4, E, nb};
    for (int i = 0; i < N_HIST_CONV; ++i) { c[i] = cs[i]; fin[i] = fs[i]; }
}

// Every call starts from this: no histories, no states, frame 0 first, no track tables.  A one-pass call runs like that.
template <class M>
void unbind(M& m) {
    Conv* c[N_HIST_CONV];
    int fin[N_HIST_CONV];
    hist_convs(m.core, c, fin);
    for (int i = 0; i < N_HIST_CONV; ++i) { c[i]->hist = nullptr; c[i]->t0 = 0; c[i]->trk = c[i]->foff = nullptr; }
    for (auto& g : m.grus) { g.hst = nullptr; g.foff = nullptr; g.ntr = 0; }
    m.core.sg = SegState();
    m.core.tk = Tracks();
}

// A tracks call: the layers that look along the frame axis (the convolutions with kt > 1 possible, the recurrences) get the tables.
template <class M>
void bind_tracks(M& m, const Tracks& tk) {
    Conv* c[N_HIST_CONV];
    int fin[N_HIST_CONV];
    hist_convs(m.core, c, fin);
    for (int i = 0; i < N_HIST_CONV; ++i) { c[i]->trk = tk.trk; c[i]->foff = tk.foff; }
    for (auto& g : m.grus) { g.foff = tk.foff; g.ntr = tk.n; }
    m.core.tk = tk;
}

template <class M>
int run(M& m, const float* x, int C, int64_t T, float* y, hipStream_t st) {
    DfnCore& k = m.core;
    const int nF = (int)k.frames_of(T);
    const int64_t R = (int64_t)C * nF;
    EGR_TRY(ensure_workspace(k, workspace_need(m, C, nF), C, nF, T, false, st));
    Take take{(char*)k.ws.p};
    layout(m, Rows{R, R, R}, take, k.B, m.X);
    unbind(m);
    features(k, x, C, nF, T, st);
    EGR_TRY(network(m, C, nF, st));
    assemble(m, assemble_args(k, alpha_of(m), C, nF, 0, nF, 0, nF, 0, nF), st);
    return synthesis(k, C, nF, 0, nF, T, 0, T, y, st);
}

// Tracks: every buffer holds the tracks' frames back to back, R rows; behind the buffers sit the tables.
struct TrackTable {           // measures of a host table; the image of Tracks is soff [n + 1] | xoff [n] (int64), foff [n + 1] | trk [R] (int)
    int n = 0;
    int64_t R = 0, total = 0;                                // packed rows, samples of all tracks
    int64_t floats() const { return 2 * (2 * (int64_t)n + 1) + (n + 1) + R; }      // the image's size in 4-byte units
};

// Checks a host table [n_tracks][2] = (offset, n) and measures it.  Nothing is allocated.
int track_table(const DfnCore* m, const char* who, const int64_t* tracks, int n_tracks, TrackTable* tt) {
    EGR_CHECK(m && tracks && n_tracks >= 1, EGR_ERR_ARG, "%s: bad argument", who);
    const int64_t n_max = MAX_FRAMES * m->d.hop_size;        // a longer track alone has too many frames
    int64_t R = 0, total = 0;
    for (int b = 0; b < n_tracks; ++b) {
        const int64_t off = tracks[2 * b], n = tracks[2 * b + 1];
        EGR_CHECK(off >= 0 && n >= 1, EGR_ERR_ARG, "%s: track %d: offset %lld, n %lld", who, b, (long long)off, (long long)n);
        EGR_CHECK(n <= n_max, EGR_ERR_UNSUPPORTED, "%s: track %d is too long", who, b);
        R += m->frames_of(n);
        total += n;
        EGR_CHECK(R <= MAX_FRAMES, EGR_ERR_UNSUPPORTED, "%s: the tracks have more than %lld frames together", who, (long long)MAX_FRAMES);
    }
    tt->n = n_tracks;
    tt->R = R;
    tt->total = total;
    return EGR_OK;
}

// The image of a checked table into `image` (tt.floats() 4-byte units).
void fill_tables(const DfnCore& m, const int64_t* tracks, int n_tracks, void* image) {
    int64_t* soff = (int64_t*)image;
    int64_t* xoff = soff + n_tracks + 1;
    int* foff = (int*)(xoff + n_tracks);
    int* trk = foff + n_tracks + 1;
    int64_t s = 0;
    int r = 0;
    for (int b = 0; b < n_tracks; ++b) {
        soff[b] = s;
        xoff[b] = tracks[2 * b];
        foff[b] = r;
        const int nF = (int)m.frames_of(tracks[2 * b + 1]);
        for (int f = 0; f < nF; ++f) trk[r + f] = b;
        s += tracks[2 * b + 1];
        r += nF;
    }
    soff[n_tracks] = s;
    foff[n_tracks] = r;
}

template <class M>
size_t tracks_need(const M& m, const TrackTable& tt, Bufs& B, typename M::Extra& X, char* base, float** table) {
    Take take{base};
    layout(m, Rows{tt.R, tt.R, tt.R}, take, B, X);
    float* t = take(tt.floats());
    if (table) *table = t;
    return take.off;
}

template <class M>
size_t tracks_workspace(const M* m, const char* who, const int64_t* tracks, int n_tracks) {
    TrackTable tt;
    if (track_table(m ? &m->core : nullptr, who, tracks, n_tracks, &tt) != EGR_OK) return 0;
    Bufs B;
    typename M::Extra X;
    return tracks_need(*m, tt, B, X, nullptr, nullptr);
}

template <class M>
int run_tracks(M* mp, const char* who, const float* x, const int64_t* tracks, int n_tracks, float* y, hipStream_t st) {
    EGR_CHECK(mp && x && y, EGR_ERR_ARG, "%s: bad argument", who);
    M& m = *mp;
    DfnCore& k = m.core;
    TrackTable tt;
    EGR_TRY(track_table(&k, who, tracks, n_tracks, &tt));                    // every refusal comes before anything is allocated
    EGR_TRY(check_current_device(who, k.device));
    const size_t table_bytes = sizeof(float) * (size_t)tt.floats();
    EGR_TRY(k.stage.reserve(table_bytes));
    fill_tables(k, tracks, n_tracks, k.stage.p);
    const int R = (int)tt.R;
    {
        Bufs B;
        typename M::Extra X;
        EGR_TRY(ensure_workspace(k, tracks_need(m, tt, B, X, nullptr, nullptr), 1, R, tt.total, false, st, true));
    }
    float* table = nullptr;
    tracks_need(m, tt, k.B, m.X, (char*)k.ws.p, &table);
    EGR_TRY(k.stage.upload(table, table_bytes, st));      // one copy for all tables
    Tracks tk;
    tk.soff = (const int64_t*)table;
    tk.xoff = tk.soff + n_tracks + 1;
    tk.foff = (const int*)(tk.xoff + n_tracks);
    tk.trk = tk.foff + n_tracks + 1;
    tk.n = n_tracks;
    unbind(m);
    bind_tracks(m, tk);
    features_tracks(k, x, R, st);
    int rc = network(m, 1, R, st);
    if (rc == EGR_OK) {
        assemble(m, assemble_args(k, alpha_of(m), 1, R, 0, R, 0, R, 0, R), st);
        rc = synthesis(k, 1, R, 0, R, tt.total, 0, tt.total, y, st);
    }
    unbind(m);                                                               // the tables belong to this call only
    return rc;
}

// Segments: the buffers hold seg_frames network frames (plus the lookahead and deep-filter rows of spec, the lagged
// rows of spec_e / frames); behind them sits what crosses a cut.
struct SegLayout {
    size_t state_off = 0, end = 0;
    SegState sg;
    float* conv_h[N_HIST_CONV];
    float* gru_h[EGR_DFN3_MAX_GRU];
};

// the largest segment whose rows (with the lookahead and deep-filter rows around it) stay within MAX_FRAMES
inline int64_t seg_clamp(const DfnCore& k, int64_t S) {
    const int64_t cap = MAX_FRAMES - k.d.conv_lookahead - k.d.df_order;
    return S < cap ? S : cap;
}

template <class M>
void layout_segments(const M& m, int C, int64_t S, char* base, Bufs& B, typename M::Extra& X, SegLayout& L) {
    const DfnCore& k = m.core;
    const DfnDims& d = k.d;
    const int64_t Cn = C;
    Take take{base};
    layout(m, Rows{Cn * S, Cn * (S + d.conv_lookahead + d.df_order - 1), Cn * (S + d.df_lookahead)}, take, B, X);
    L.state_off = take.off;
    L.sg.norm = take(Cn * (d.nb_erb + d.nb_df));
    const Conv* c[N_HIST_CONV];
    int fin[N_HIST_CONV];
    hist_convs(k, c, fin);
    for (int i = 0; i < N_HIST_CONV; ++i) L.conv_h[i] = c[i]->kt > 1 ? take(Cn * (c[i]->kt - 1) * fin[i] * c[i]->cin) : nullptr;
    for (int g = 0; g < EGR_DFN3_MAX_GRU; ++g) L.gru_h[g] = g < k.ngru() ? take(Cn * k.gru_width(g)) : nullptr;
    L.sg.mask_h = take(Cn * (d.df_order - 1) * d.nb_erb);
    L.sg.coefs_h = take(Cn * d.df_lookahead * d.nb_df * 2 * d.df_order);
    L.sg.alpha_h = take(Cn * d.df_lookahead);
    L.sg.frames_h = take(Cn * (d.fft_size / d.hop_size - 1) * d.fft_size);
    L.end = take.off;
}

template <class M>
size_t segment_need(const M& m, int C, int64_t S) {
    Bufs B;
    typename M::Extra X;
    SegLayout L;
    layout_segments(m, C, seg_clamp(m.core, S), nullptr, B, X, L);
    return L.end;
}

template <class M>
int run_segmented(M& m, const float* x, int C, int64_t T, float* y, int64_t seg_frames, hipStream_t st) {
    DfnCore& k = m.core;
    const DfnDims& d = k.d;
    const Bufs& B = k.B;
    const int64_t S = seg_clamp(k, seg_frames), nF = k.frames_of(T);
    const int N = d.fft_size, E = d.nb_erb, nb = d.nb_df, la = d.conv_lookahead, O2 = 2 * d.df_order;
    EGR_TRY(ensure_workspace(k, segment_need(m, C, S), C, 0, T, true, st));
    SegLayout L;
    layout_segments(m, C, S, (char*)k.ws.p, k.B, m.X, L);
    unbind(m);
    Conv* hc[N_HIST_CONV];
    int fin[N_HIST_CONV];
    hist_convs(k, hc, fin);
    for (int i = 0; i < N_HIST_CONV; ++i) hc[i]->hist = L.conv_h[i];
    for (size_t g = 0; g < m.grus.size(); ++g) m.grus[g].hst = L.gru_h[g];
    k.sg = L.sg;
    // nothing of an earlier call survives: zero states and histories (the norm states start from their linspace values in segment 0)
    EGR_HIP(hipMemsetAsync((char*)k.ws.p + L.state_off, 0, L.end - L.state_off, st));
    int64_t nseg = 0;
    egr_dfn_segment sp;
    EGR_TRY(egr_dfn_segment_plan(N, d.hop_size, la, d.df_order, d.df_lookahead, T, S, 0, nullptr, &nseg));
    for (int64_t j = 0; j < nseg; ++j) {
        EGR_TRY(egr_dfn_segment_plan(N, d.hop_size, la, d.df_order, d.df_lookahead, T, S, j, &sp, nullptr));
        const int Sj = (int)(sp.net_hi - sp.net_lo), nS = (int)(sp.spec_hi - sp.spec_lo);
        const int nA = sp.asm_hi > sp.asm_lo ? (int)(sp.asm_hi - sp.asm_lo) : 0;
        const int64_t Rs = (int64_t)C * nS;
        hipLaunchKernelGGL(k_dfn_analysis<false>, dim3(nS, C), dim3(256), (size_t)N * 24, st, x, T, nS, sp.spec_lo, N, d.hop_size, k.tw,
                           k.win, k.wnorm, B.spec, Tracks());
        hipLaunchKernelGGL(k_dfn_erb_db, dim3(grid_for(Rs * E)), dim3(256), 0, st, B.spec, Rs, k.Fq, E, k.band_lo, k.band_w, B.db);
        // input frames [scan_lo, scan_hi) -> feature rows t - la; the rows >= nF - la of this segment are zero
        int64_t zlo = nF - la - sp.net_lo;
        zlo = zlo < 0 ? 0 : (zlo > Sj ? Sj : zlo);
        ScanArgs sa{B.db, B.spec, B.ferb, B.fspec, k.sg.norm, C, nS, (int)(sp.scan_lo - sp.spec_lo), (int)(sp.scan_hi - sp.scan_lo), Sj,
                    (int)(sp.scan_lo - la - sp.net_lo), (int)zlo, Sj, k.Fq, E, nb, la, j == 0, d.norm_alpha, nullptr};
        hipLaunchKernelGGL(k_dfn_norm_scan<false>, dim3((C * (E + nb) + 63) / 64), dim3(64), 0, st, sa);
        for (int i = 0; i < N_HIST_CONV; ++i) hc[i]->t0 = sp.net_lo;
        EGR_TRY(network(m, C, Sj, st));
        // the assemble step lags the network by df_lookahead frames: its rows in front of net_lo come from the histories
        if (nA > 0) assemble(m, assemble_args(k, alpha_of(m), C, nF, sp.asm_lo, nA, sp.spec_lo, nS, sp.net_lo, Sj), st);
        hist_push(B.mask, k.sg.mask_h, C, Sj, d.df_order - 1, E, st);
        hist_push(B.coefs, k.sg.coefs_h, C, Sj, d.df_lookahead, nb * O2, st);
        if (alpha_of(m)) hist_push(alpha_of(m), k.sg.alpha_h, C, Sj, d.df_lookahead, 1, st);
        EGR_TRY(synthesis(k, C, nA, sp.asm_lo, nF, T, sp.out_lo, sp.out_hi - sp.out_lo, y, st));
        hist_push(B.frames, k.sg.frames_h, C, nA, N / d.hop_size - 1, N, st);
    }
    return EGR_OK;
}

}  // namespace
}  // namespace egr

// ================================================================================================ the segment plan (host only)
// Segment `index` of a file of n samples cut every seg_frames network frames; all ranges are half-open, in frames
// (out: samples).  The non-empty ranges of every kind partition their axis in segment order; a range with hi <= lo is empty.
extern "C" int egr_dfn_segment_plan(int fft_size, int hop_size, int conv_lookahead, int df_order, int df_lookahead, int64_t n,
                                    int64_t seg_frames, int64_t index, egr_dfn_segment* seg, int64_t* n_segments) {
    EGR_CHECK(fft_size > 0 && hop_size > 0 && fft_size % hop_size == 0 && conv_lookahead >= 0 && df_order >= 1 && df_lookahead >= 0 &&
              df_lookahead < df_order && n >= 1 && seg_frames >= 1, EGR_ERR_ARG, "egr_dfn_segment_plan: bad argument");
    const int64_t nF = (n + fft_size) / hop_size, ov = fft_size / hop_size, la = conv_lookahead, look = df_lookahead;
    const int64_t nseg = (nF - 1) / seg_frames + 1;
    if (n_segments) *n_segments = nseg;
    if (!seg) return EGR_OK;
    EGR_CHECK(index >= 0 && index < nseg, EGR_ERR_ARG, "egr_dfn_segment_plan: segment %lld of %lld", (long long)index, (long long)nseg);
    const auto lo0 = [](int64_t v) { return v < 0 ? (int64_t)0 : v; };
    const auto mn = [](int64_t a, int64_t b) { return a < b ? a : b; };
    const bool first = index == 0, last = index == nseg - 1;
    const int64_t a = index * seg_frames, b = last ? nF : a + seg_frames;
    seg->net_lo = a;
    seg->net_hi = b;
    seg->scan_lo = first ? 0 : mn(nF, a + la);              // the norms see input frame t + la for network frame t
    seg->scan_hi = last ? nF : mn(nF, b + la);
    seg->asm_lo = lo0(a - look);                            // mask and deep filter lag the network by df_lookahead frames
    seg->asm_hi = last ? nF : b - look;                     // at or below asm_lo (even negative): nothing to assemble yet
    seg->spec_lo = lo0(seg->asm_lo - (df_order - 1 - look));
    const int64_t win_hi = mn(nF, seg->asm_hi + look);
    seg->spec_hi = seg->scan_hi > win_hi ? seg->scan_hi : win_hi;
    seg->out_lo = first ? 0 : mn(n, lo0(seg->asm_lo - ov + 1) * hop_size);     // samples whose ov frames are all assembled
    seg->out_hi = last ? n : mn(n, lo0(seg->asm_hi - ov + 1) * hop_size);
    return EGR_OK;
}

// ================================================================================================ DeepFilterNet3 entry points
extern "C" int egr_dfn3_create(void** handle, const egr_dfn3_config* cfg, const float* packed, int64_t n_floats, int device) {
    using namespace egr;
    EGR_CHECK(handle && cfg && packed && n_floats > 0, EGR_ERR_ARG, "egr_dfn3_create: null argument");
    EGR_CHECK(cfg->struct_bytes == (int)sizeof(egr_dfn3_config), EGR_ERR_ARG, "egr_dfn3_create: struct_bytes %d != %d",
              cfg->struct_bytes, (int)sizeof(egr_dfn3_config));
    const egr_dfn3_config& c = *cfg;
    DfnDims d{c.fft_size, c.hop_size, c.nb_erb, c.nb_df, c.df_order, c.df_lookahead, c.conv_lookahead, c.conv_ch, c.kt, c.kf, c.kt_inp,
              c.kf_inp, c.convt_kf, c.df_pathway_kt, c.path_groups, c.df_path_groups, c.emb_hidden_dim, c.emb_num_layers, c.df_hidden_dim,
              c.df_num_layers, c.norm_alpha, {}};
    memcpy(d.erb_widths, c.erb_widths, sizeof(d.erb_widths));
    EGR_TRY(check_common(d, "egr_dfn3"));
    EGR_CHECK(c.lin_groups > 0 && c.enc_lin_groups > 0, EGR_ERR_UNSUPPORTED, "egr_dfn3: conv groups");

    std::unique_ptr<Dfn3> m(new Dfn3());
    m->cfg = c;
    DfnCore& k = m->core;
    init_core(k, d, device);
    const int nb = c.nb_df, O2 = 2 * c.df_order, embd = k.embd;
    // packed order: dfn_weights.pack_order
    WeightCursor wc;
    wc.encoder_convs(k);
    const int64_t o_fc = wc.W((int64_t)(c.conv_ch * nb / 2) * embd / c.enc_lin_groups);
    struct GruSpec { int64_t wih, whh, bih, bhh; int H; };
    std::vector<GruSpec> gs;
    auto sq = [&](int in, int H, int layers, int64_t* lin_in) {        // SqueezedGRU: linear_in, then `layers` GRU layers of width H
        *lin_in = wc.W((int64_t)in * H / c.lin_groups);
        for (int l = 0; l < layers; ++l) gs.push_back({wc.W((int64_t)3 * H * H), wc.W((int64_t)3 * H * H), wc.W(3 * H), wc.W(3 * H), H});
    };
    int64_t o_enc_in, o_enc_out, o_erb_in, o_erb_out, o_df_in, o_skip = -1, o_dfout;
    sq(embd, c.emb_hidden_dim, 1, &o_enc_in);
    o_enc_out = wc.W((int64_t)c.emb_hidden_dim * embd / c.lin_groups);
    sq(embd, c.emb_hidden_dim, c.emb_num_layers - 1, &o_erb_in);
    o_erb_out = wc.W((int64_t)c.emb_hidden_dim * embd / c.lin_groups);
    wc.erb_decoder_convs(k);
    sq(embd, c.df_hidden_dim, c.df_num_layers, &o_df_in);
    if (c.df_gru_skip) o_skip = wc.W((int64_t)embd * c.df_hidden_dim / c.lin_groups);
    o_dfout = wc.W((int64_t)c.df_hidden_dim * nb * O2 / c.lin_groups);
    wc.df_pathway_convs(k);
    EGR_CHECK(wc.pos == n_floats, EGR_ERR_ARG, "egr_dfn3_create: packed weights hold %lld floats, the config needs %lld",
              (long long)n_floats, (long long)wc.pos);
    const int64_t o_whh = align64(n_floats);
    Image im = build_tables(d, packed, n_floats, o_whh + (int64_t)gs.size() * DENSE_WHH_FLOATS);
    for (size_t g = 0; g < gs.size(); ++g) repack_dense_whh(packed + gs[g].whh, gs[g].H, im.host.data() + o_whh + g * DENSE_WHH_FLOATS);
    EGR_TRY(upload(k, "egr_dfn3_create", im));
    bind(k, wc, im);
    float* D = k.dev_w;
    m->fc_emb = D + o_fc;
    m->enc_lin_in = D + o_enc_in; m->enc_lin_out = D + o_enc_out;
    m->erb_lin_in = D + o_erb_in; m->erb_lin_out = D + o_erb_out;
    m->df_lin_in = D + o_df_in; m->df_skip = o_skip >= 0 ? D + o_skip : nullptr; m->df_out = D + o_dfout;
    for (size_t g = 0; g < gs.size(); ++g) {
        Gru G;
        G.in = G.H = gs[g].H;
        G.wih = D + gs[g].wih; G.bih = D + gs[g].bih; G.bhh = D + gs[g].bhh; G.whh_pk = D + o_whh + g * DENSE_WHH_FLOATS;
        m->grus.push_back(G);
    }
    *handle = m.release();
    return EGR_OK;
}

extern "C" size_t egr_dfn3_workspace_bytes(void* handle, int channels, int64_t n) {
    if (!handle || channels < 1 || n < 1) return 0;
    const egr::Dfn3* m = (const egr::Dfn3*)handle;
    return egr::workspace_need(*m, channels, (int)m->core.frames_of(n));
}

extern "C" int egr_dfn3_enhance(void* handle, const float* x48, int channels, int64_t n, float* y, void* stream) {
    using namespace egr;
    Dfn3* m = (Dfn3*)handle;
    EGR_TRY(enhance_checks(m ? &m->core : nullptr, "egr_dfn3_enhance", x48, channels, n, y));
    return run(*m, x48, channels, n, y, (hipStream_t)stream);
}

extern "C" int egr_dfn3_enhance_segmented(void* handle, const float* x48, int channels, int64_t n, float* y, int64_t seg_frames,
                                          void* stream) {
    using namespace egr;
    Dfn3* m = (Dfn3*)handle;
    EGR_TRY(enhance_checks(m ? &m->core : nullptr, "egr_dfn3_enhance_segmented", x48, channels, n, y, false));
    EGR_CHECK(seg_frames >= 1, EGR_ERR_ARG, "egr_dfn3_enhance_segmented: seg_frames %lld < 1", (long long)seg_frames);
    return run_segmented(*m, x48, channels, n, y, seg_frames, (hipStream_t)stream);
}

extern "C" size_t egr_dfn3_segment_workspace_bytes(void* handle, int channels, int64_t seg_frames) {
    if (!handle || channels < 1 || seg_frames < 1) return 0;
    return egr::segment_need(*(const egr::Dfn3*)handle, channels, seg_frames);
}

extern "C" int egr_dfn3_enhance_tracks(void* handle, const float* x48, const int64_t* tracks, int n_tracks, float* y, void* stream) {
    return egr::run_tracks((egr::Dfn3*)handle, "egr_dfn3_enhance_tracks", x48, tracks, n_tracks, y, (hipStream_t)stream);
}

extern "C" size_t egr_dfn3_tracks_workspace_bytes(void* handle, const int64_t* tracks, int n_tracks) {
    return egr::tracks_workspace((const egr::Dfn3*)handle, "egr_dfn3_tracks_workspace_bytes", tracks, n_tracks);
}

extern "C" size_t egr_dfn3_workspace_held(void* handle) {
    return handle ? ((const egr::Dfn3*)handle)->core.ws.bytes : 0;
}

extern "C" int egr_dfn3_stage(void* handle, int stage, float* dst, int64_t capacity, int64_t* count, void* stream) {
    using namespace egr;
    EGR_CHECK(handle && count, EGR_ERR_ARG, "egr_dfn3_stage: null argument");
    const Dfn3* m = (const Dfn3*)handle;
    const DfnCore& k = m->core;
    return stage_copy(k, "egr_dfn3_stage", stage, dst, capacity, count, stream, [&](int s, const float** src, int64_t* cnt) {
        if (s == EGR_DFN3_STAGE_EMB) { *src = m->X.emb; *cnt = (int64_t)k.lastC * k.lastF * k.embd; }
    });
}

extern "C" int egr_dfn3_time_gru(void* handle, int layer, int channels, int64_t steps, double* us_per_step) {
    using namespace egr;
    const Dfn3* m = (const Dfn3*)handle;
    return time_gru_harness(m ? &m->core : nullptr, "egr_dfn3_time_gru", layer, channels, steps, false, us_per_step,
                            [&](const float* proj, float* out, float*, int nF) {
        const Gru& g = m->grus[layer];
        launch_gru(proj, g.whh_pk, g.bhh, g.H, channels, nF, out, nullptr, nullptr, 0, 0);
    });
}

extern "C" int egr_dfn3_destroy(void* handle) {
    if (!handle) return EGR_OK;
    egr::Dfn3* m = (egr::Dfn3*)handle;
    egr::destroy(m->core);
    delete m;
    return EGR_OK;
}

// ================================================================================================ DeepFilterNet2 entry points
extern "C" int egr_dfn2_create(void** handle, const egr_dfn2_config* cfg, const float* packed, int64_t n_floats, int device) {
    using namespace egr;
    EGR_CHECK(handle && cfg && packed && n_floats > 0, EGR_ERR_ARG, "egr_dfn2_create: null argument");
    EGR_CHECK(cfg->struct_bytes == (int)sizeof(egr_dfn2_config), EGR_ERR_ARG, "egr_dfn2_create: struct_bytes %d != %d",
              cfg->struct_bytes, (int)sizeof(egr_dfn2_config));
    const egr_dfn2_config& c = *cfg;
    DfnDims d{c.fft_size, c.hop_size, c.nb_erb, c.nb_df, c.df_order, c.df_lookahead, c.conv_lookahead, c.conv_ch, c.kt, c.kf, c.kt_inp,
              c.kf_inp, 3 /* SPEC DFN2-P9: the transposed convs are (1, 3) */, c.df_pathway_kt, c.path_groups, c.df_path_groups,
              c.emb_hidden_dim, c.emb_num_layers, c.df_hidden_dim, c.df_num_layers, c.norm_alpha, {}};
    memcpy(d.erb_widths, c.erb_widths, sizeof(d.erb_widths));
    EGR_TRY(check_common(d, "egr_dfn2"));
    const int ch = c.conv_ch, nb = c.nb_df, O2 = 2 * c.df_order, G = c.gru_groups, Gl = c.lin_groups;
    const int embd = ch * c.nb_erb / 4, He = c.emb_hidden_dim, Hd = c.df_hidden_dim;
    EGR_CHECK(c.conv_lookahead == 0 || c.conv_lookahead >= c.df_lookahead, EGR_ERR_UNSUPPORTED, "egr_dfn2: df_order / lookaheads");
    EGR_CHECK(G > 0 && embd % G == 0 && He % G == 0 && Hd % G == 0, EGR_ERR_UNSUPPORTED, "egr_dfn2: gru_groups %d", G);
    EGR_CHECK(Gl > 0 && (ch * nb / 2) % Gl == 0 && embd % Gl == 0 && He % Gl == 0 && (!c.df_gru_skip || Hd % Gl == 0) &&
              (c.df_output_layer == 1 || (Hd % Gl == 0 && (nb * O2) % Gl == 0)), EGR_ERR_UNSUPPORTED, "egr_dfn2: lin_groups %d", Gl);
    EGR_CHECK((c.df_gru_skip == 0 || c.df_gru_skip == 1) && (c.df_output_layer == 0 || c.df_output_layer == 1) &&
              (c.group_shuffle == 0 || c.group_shuffle == 1), EGR_ERR_UNSUPPORTED, "egr_dfn2: df_gru_skip / df_output_layer / group_shuffle");

    std::unique_ptr<Dfn2> m(new Dfn2());
    m->cfg = c;
    DfnCore& k = m->core;
    init_core(k, d, device);
    // packed order: dfn2_weights.pack_order
    WeightCursor wc;
    wc.encoder_convs(k);
    const int64_t o_fcw = wc.W((int64_t)(ch * nb / 2) * embd / Gl), o_fcb = wc.W(embd);
    struct GruOff { int64_t wih, whh, bih, bhh, pk; };
    std::vector<GruOff> go;                                             // of m->grus[l], until the image is on the device
    auto ggru = [&](int in0, int H, int layers) {                       // GroupedGRU: `layers` layers of G GRUs of width H / G
        for (int l = 0; l < layers; ++l) {
            GGru L;
            L.in = l == 0 ? in0 : H; L.H = H; L.G = G; L.h = H / G;
            L.shuffle = c.group_shuffle && G > 1 && l < layers - 1;
            if (!L.dense()) ggru_shape(L.h, &L.K, &L.S);
            m->grus.push_back(L);
            go.push_back({wc.W((int64_t)3 * H * L.in / G), wc.W((int64_t)3 * H * H / G), wc.W(3 * H), wc.W(3 * H), 0});
        }
    };
    ggru(embd, He, 1);
    ggru(He, He, c.emb_num_layers - 1);
    const int64_t o_erbw = wc.W((int64_t)He * embd / Gl), o_erbb = wc.W(embd);
    wc.erb_decoder_convs(k);
    ggru(He, Hd, c.df_num_layers);
    const int64_t o_skip = c.df_gru_skip ? wc.W((int64_t)He * Hd / Gl) : -1;
    const int64_t o_out = wc.W(c.df_output_layer == 1 ? (int64_t)nb * O2 * Hd : (int64_t)Hd * nb * O2 / Gl);
    const int64_t o_outb = c.df_output_layer == 1 ? wc.W(nb * O2) : -1;
    const int64_t o_aw = wc.W(Hd), o_ab = wc.W(1);
    wc.df_pathway_convs(k);
    EGR_CHECK(wc.pos == n_floats, EGR_ERR_ARG, "egr_dfn2_create: packed weights hold %lld floats, the config needs %lld",
              (long long)n_floats, (long long)wc.pos);
    int64_t o_cur = align64(n_floats);
    for (size_t l = 0; l < go.size(); ++l) {
        const GGru& L = m->grus[l];
        go[l].pk = o_cur;
        o_cur = align64(o_cur + (L.dense() ? DENSE_WHH_FLOATS : (int64_t)G * 3 * L.K * L.h * L.S));
    }
    Image im = build_tables(d, packed, n_floats, o_cur);
    for (size_t l = 0; l < go.size(); ++l) {
        const GGru& L = m->grus[l];
        const float* w = packed + go[l].whh;                    // [G][3h][h]
        float* dst = im.host.data() + go[l].pk;
        if (L.dense()) {                                        // G = 1: k_dfn_gru's order
            repack_dense_whh(w, L.H, dst);
            continue;
        }
        const int h = L.h, K = L.K, S = L.S, NT = h * S;        // k_dfn2_gru's thread-minor order, group after group
        for (int g = 0; g < G; ++g)
            for (int t = 0; t < NT; ++t)
                for (int e = 0; e < 3 * K; ++e) {
                    const int j = t / S, s = t % S, q = e / K, col = s + S * (e % K);
                    dst[((int64_t)g * 3 * K + e) * NT + t] = col < h ? w[((int64_t)g * 3 * h + q * h + j) * h + col] : 0.f;
                }
    }
    EGR_TRY(upload(k, "egr_dfn2_create", im));
    bind(k, wc, im);
    float* D = k.dev_w;
    m->fc_emb_w = D + o_fcw; m->fc_emb_b = D + o_fcb;
    m->erb_fc_w = D + o_erbw; m->erb_fc_b = D + o_erbb;
    m->df_skip = o_skip >= 0 ? D + o_skip : nullptr;
    m->df_out = D + o_out; m->df_out_b = o_outb >= 0 ? D + o_outb : nullptr;
    m->fc_a_w = D + o_aw; m->fc_a_b = D + o_ab;
    for (size_t l = 0; l < go.size(); ++l) {
        GGru& L = m->grus[l];
        L.wih = D + go[l].wih; L.bih = D + go[l].bih; L.bhh = D + go[l].bhh; L.whh_pk = D + go[l].pk;
    }
    *handle = m.release();
    return EGR_OK;
}

extern "C" size_t egr_dfn2_workspace_bytes(void* handle, int channels, int64_t n) {
    if (!handle || channels < 1 || n < 1) return 0;
    const egr::Dfn2* m = (const egr::Dfn2*)handle;
    return egr::workspace_need(*m, channels, (int)m->core.frames_of(n));
}

extern "C" int egr_dfn2_enhance(void* handle, const float* x48, int channels, int64_t n, float* y, void* stream) {
    using namespace egr;
    Dfn2* m = (Dfn2*)handle;
    EGR_TRY(enhance_checks(m ? &m->core : nullptr, "egr_dfn2_enhance", x48, channels, n, y));
    return run(*m, x48, channels, n, y, (hipStream_t)stream);
}

extern "C" int egr_dfn2_enhance_segmented(void* handle, const float* x48, int channels, int64_t n, float* y, int64_t seg_frames,
                                          void* stream) {
    using namespace egr;
    Dfn2* m = (Dfn2*)handle;
    EGR_TRY(enhance_checks(m ? &m->core : nullptr, "egr_dfn2_enhance_segmented", x48, channels, n, y, false));
    EGR_CHECK(seg_frames >= 1, EGR_ERR_ARG, "egr_dfn2_enhance_segmented: seg_frames %lld < 1", (long long)seg_frames);
    return run_segmented(*m, x48, channels, n, y, seg_frames, (hipStream_t)stream);
}

extern "C" size_t egr_dfn2_segment_workspace_bytes(void* handle, int channels, int64_t seg_frames) {
    if (!handle || channels < 1 || seg_frames < 1) return 0;
    return egr::segment_need(*(const egr::Dfn2*)handle, channels, seg_frames);
}

extern "C" int egr_dfn2_enhance_tracks(void* handle, const float* x48, const int64_t* tracks, int n_tracks, float* y, void* stream) {
    return egr::run_tracks((egr::Dfn2*)handle, "egr_dfn2_enhance_tracks", x48, tracks, n_tracks, y, (hipStream_t)stream);
}

extern "C" size_t egr_dfn2_tracks_workspace_bytes(void* handle, const int64_t* tracks, int n_tracks) {
    return egr::tracks_workspace((const egr::Dfn2*)handle, "egr_dfn2_tracks_workspace_bytes", tracks, n_tracks);
}

extern "C" size_t egr_dfn2_workspace_held(void* handle) {
    return handle ? ((const egr::Dfn2*)handle)->core.ws.bytes : 0;
}

extern "C" int egr_dfn2_stage(void* handle, int stage, float* dst, int64_t capacity, int64_t* count, void* stream) {
    using namespace egr;
    EGR_CHECK(handle && count, EGR_ERR_ARG, "egr_dfn2_stage: null argument");
    const Dfn2* m = (const Dfn2*)handle;
    const DfnCore& k = m->core;
    return stage_copy(k, "egr_dfn2_stage", stage, dst, capacity, count, stream, [&](int s, const float** src, int64_t* cnt) {
        const int64_t R = (int64_t)k.lastC * k.lastF;
        if (s == EGR_DFN3_STAGE_EMB) { *src = m->X.gsum[0]; *cnt = R * k.gru_width(0); }
        else if (s == EGR_DFN2_STAGE_ALPHA) { *src = m->X.alpha; *cnt = R; }
        else if (s >= EGR_DFN2_STAGE_SUM0 && s < EGR_DFN2_STAGE_SUM0 + k.ngru()) {
            *src = m->X.gsum[s - EGR_DFN2_STAGE_SUM0];
            *cnt = R * k.gru_width(s - EGR_DFN2_STAGE_SUM0);
        }
    });
}

extern "C" int egr_dfn2_time_gru(void* handle, int layer, int channels, int64_t steps, double* us_per_step) {
    using namespace egr;
    const Dfn2* m = (const Dfn2*)handle;
    return time_gru_harness(m ? &m->core : nullptr, "egr_dfn2_time_gru", layer, channels, steps, true, us_per_step,
                            [&](const float* proj, float* out, float* sum, int nF) {
        const GGru& g = m->grus[layer];
        if (g.dense())
            launch_gru(proj, g.whh_pk, g.bhh, g.H, channels, nF, out, nullptr, nullptr, 0, 0);
        else {
            GGru z = g;                                             // no carried state, no tracks
            z.hst = nullptr;
            z.foff = nullptr;
            launch_ggru(z, proj, nullptr, out, sum, channels, nF, 0);
        }
    });
}

extern "C" int egr_dfn2_destroy(void* handle) {
    if (!handle) return EGR_OK;
    egr::Dfn2* m = (egr::Dfn2*)handle;
    egr::destroy(m->core);
    delete m;
    return EGR_OK;
}
