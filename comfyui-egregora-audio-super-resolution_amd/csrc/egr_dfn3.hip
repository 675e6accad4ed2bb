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
// DeepFilterNet2 (egr_dfn2_*) reuses these kernels; its own ones follow the DeepFilterNet3 entry points below.
#include <math.h>
#include <string.h>

#include <vector>

#include "egr_common.h"

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

// ------------------------------------------------------------------------------------------------ analysis / features
__global__ __launch_bounds__(256) void k_dfn_analysis(const float* __restrict__ x, int64_t T, int nF, int N, int hop,
                                                       const double2* __restrict__ tw, const float* __restrict__ win, float wnorm,
                                                       float2* __restrict__ spec) {
    extern __shared__ double sm[];
    double* fr = sm;                       // N windowed samples
    double2* tws = (double2*)(sm + N);     // N twiddles
    const int f = blockIdx.x, b = blockIdx.y, Fq = N / 2 + 1;
    const float* xb = x + (int64_t)b * T;
    const int64_t s0 = (int64_t)f * hop - (N - hop);
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
        spec[((int64_t)b * nF + f) * Fq + k] = make_float2((float)(re * (double)wnorm), (float)(im * (double)wnorm));
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
__global__ void k_dfn_norm_scan(const float* __restrict__ db, const float2* __restrict__ spec, int C, int nF, int Fq, int E, int nbdf,
                                float alpha, int la, float* __restrict__ ferb, float2* __restrict__ fspec) {
    const int lanes = E + nbdf;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * lanes) return;
    const int b = i / lanes, l = i - b * lanes;
    const float a = alpha, a1 = 1.f - alpha;
    constexpr int U = 16;
    if (l < E) {
        float s = -60.f + (-90.f + 60.f) * (E > 1 ? (float)l / (float)(E - 1) : 0.f);
        const float* src = db + (int64_t)b * nF * E + l;
        float* dst = ferb + (int64_t)b * nF * E + l;
        for (int t0 = 0; t0 < nF; t0 += U) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = (t0 + u < nF) ? src[(int64_t)(t0 + u) * E] : 0.f;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u;
                if (t < nF) {
                    s = v[u] * a1 + s * a;
                    if (t - la >= 0) dst[(int64_t)(t - la) * E] = (v[u] - s) / 40.f;
                }
            }
        }
        for (int t = (nF - la > 0 ? nF - la : 0); t < nF; ++t) dst[(int64_t)t * E] = 0.f;
    } else {
        const int f = l - E;
        float s = 0.001f + (0.0001f - 0.001f) * (nbdf > 1 ? (float)f / (float)(nbdf - 1) : 0.f);
        const float2* src = spec + (int64_t)b * nF * Fq + f;
        float2* dst = fspec + (int64_t)b * nF * nbdf + f;
        for (int t0 = 0; t0 < nF; t0 += U) {
            float2 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = (t0 + u < nF) ? src[(int64_t)(t0 + u) * Fq] : make_float2(0.f, 0.f);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u;
                if (t < nF) {
                    s = hypotf(v[u].x, v[u].y) * a1 + s * a;
                    const float r = sqrtf(s);
                    if (t - la >= 0) dst[(int64_t)(t - la) * nbdf] = make_float2(v[u].x / r, v[u].y / r);
                }
            }
        }
        for (int t = (nF - la > 0 ? nF - la : 0); t < nF; ++t) dst[(int64_t)t * nbdf] = make_float2(0.f, 0.f);
    }
}

// ------------------------------------------------------------------------------------------------ convolutions (NHWC: [B][T][F][C])
struct ConvArgs {
    const float* x; const float* w; const float* scale; const float* shift; const float* res; float* y;
    int B, T, Fin, Cin, Fout, Cout, groups, kt, kf, fstride, fpad, transposed, act;
};

__device__ __forceinline__ float act_fn(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return 1.f / (1.f + expf(-v));
    if (act == 3) return tanhf(v);
    return v;
}

__global__ void k_dfn_conv(ConvArgs p) {
    const int64_t n = (int64_t)p.B * p.T * p.Fout * p.Cout;
    const int cig = p.Cin / p.groups, cog = p.Cout / p.groups;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % p.Cout);
        int64_t r = i / p.Cout;
        const int fo = (int)(r % p.Fout);
        r /= p.Fout;
        const int t = (int)(r % p.T);
        const int b = (int)(r / p.T);
        const int g = co / cog;
        float acc = 0.f;
        if (!p.transposed) {
            const float* wc = p.w + (int64_t)co * cig * p.kt * p.kf;
            for (int it = 0; it < p.kt; ++it) {
                const int ti = t - (p.kt - 1) + it;
                if (ti < 0) continue;
                for (int j = 0; j < p.kf; ++j) {
                    const int fi = fo * p.fstride - p.fpad + j;
                    if (fi < 0 || fi >= p.Fin) continue;
                    const float* xv = p.x + (((int64_t)b * p.T + ti) * p.Fin + fi) * p.Cin + g * cig;
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
                const float* xv = p.x + (((int64_t)b * p.T + t) * p.Fin + fi) * p.Cin + g * cig;
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

// ------------------------------------------------------------------------------------------------ GRU recurrence
// One workgroup per audio channel runs all nF steps of one layer.  Gate row r (torch order r | z | n, 3H rows) is split over GRU_SEG
// lanes; thread t owns the (row, lane) tasks q = j * 1024 + t, j < 12, row q / 16, lane q % 16, columns 16 k + lane (k < 16).  Its 192
// W_hh values (zero-padded beyond H) sit: tasks 0-2 in VGPRs, 3-4 in LDS, 5-11 in global memory (L2-resident, 448 KiB per step), all
// in thread-minor order so every load is coalesced.  Per step: 16 h values from LDS, 192 FMAs, a 16-lane shuffle sum per task, the
// gate sums to LDS, one barrier, the H gate updates, one barrier.  proj = W_ih x + b_ih of all frames comes from one GEMM beforehand.
__global__ __launch_bounds__(GRU_THREADS) void k_dfn_gru(const float* __restrict__ proj, const float* __restrict__ whh_pk,
                                                          const float* __restrict__ bhh, int H, int nF, float* __restrict__ out) {
    __shared__ float wl[GRU_NLDS * GRU_THREADS];
    __shared__ float hs[GRU_HMAX];
    __shared__ float gs[3 * GRU_HMAX];
    const int t = threadIdx.x, lane = t % GRU_SEG, b = blockIdx.x;
    const float* pb = proj + (int64_t)b * nF * 3 * H;
    float* ob = out + (int64_t)b * nF * H;
    float wr[GRU_NREG];
#pragma unroll
    for (int e = 0; e < GRU_NREG; ++e) wr[e] = whh_pk[(int64_t)e * GRU_THREADS + t];
    for (int e = 0; e < GRU_NLDS; ++e) wl[e * GRU_THREADS + t] = whh_pk[(int64_t)(GRU_NREG + e) * GRU_THREADS + t];
    const float* wg = whh_pk + (int64_t)(GRU_NREG + GRU_NLDS) * GRU_THREADS + t;
    if (t < GRU_HMAX) hs[t] = 0.f;
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
}

// ------------------------------------------------------------------------------------------------ mask + deep filter, synthesis
__global__ void k_dfn_assemble(const float2* __restrict__ spec, const float* __restrict__ mask, const float* __restrict__ coefs,
                               const int* __restrict__ band_of, int C, int nF, int Fq, int E, int nbdf, int order, int look,
                               float2* __restrict__ out) {
    const int64_t n = (int64_t)C * nF * Fq;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int f = (int)(i % Fq);
        const int64_t r = i / Fq;                  // b * nF + t
        const int t = (int)(r % nF);
        const int64_t b = r / nF;
        float2 y;
        if (f < nbdf) {
            const float* c = coefs + (r * nbdf + f) * 2 * order;
            float re = 0.f, im = 0.f;
            for (int k = 0; k < order; ++k) {
                const int ts = t - (order - 1 - look) + k;
                if (ts < 0 || ts >= nF) continue;
                const float2 s = spec[(b * nF + ts) * Fq + f];
                re = fmaf(s.x, c[2 * k], fmaf(-s.y, c[2 * k + 1], re));
                im = fmaf(s.x, c[2 * k + 1], fmaf(s.y, c[2 * k], im));
            }
            y = make_float2(re, im);
        } else {
            const float m = mask[r * E + band_of[f]];
            const float2 s = spec[i];
            y = make_float2(s.x * m, s.y * m);
        }
        out[i] = y;
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

__global__ void k_dfn_ola(const float* __restrict__ frames, int C, int nF, int N, int hop, int64_t T, float* __restrict__ y) {
    const int64_t n = (int64_t)C * T;
    const int d = N - hop, ov = N / hop;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / T, s = i - b * T;
        const int64_t o = s + d;
        const int64_t k = o / hop;
        const int j = (int)(o - k * hop);
        float acc = 0.f;
        for (int m = ov - 1; m >= 0; --m) {
            const int64_t fk = k - m;
            if (fk < 0 || fk >= nF) continue;
            acc += frames[(b * nF + fk) * N + m * hop + j];
        }
        y[i] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ host side
inline unsigned grid_for(int64_t n, int bs = 256) {
    int64_t g = (n + bs - 1) / bs;
    if (g > 65536) g = 65536;
    return (unsigned)(g < 1 ? 1 : g);
}

struct Conv {                 // one convolution with its (optional) BN affine
    const float* w = nullptr; const float* scale = nullptr; const float* shift = nullptr;
    int cin = 0, cout = 0, groups = 1, kt = 1, kf = 1, transposed = 0;
};
struct Gru {
    const float* wih = nullptr; const float* bih = nullptr; const float* bhh = nullptr; float* whh_pk = nullptr;
    int in = 0, H = 0;
};

}  // namespace

struct Dfn3 {
    egr_dfn3_config cfg;
    int device = 0, Fq = 0, E4 = 0, embd = 0;
    float* dev_w = nullptr;                 // packed weights + repacked W_hh + tables (one allocation)
    const double2* tw = nullptr; const float* win = nullptr; const int* band_lo = nullptr; const int* band_w = nullptr;
    const int* band_of = nullptr;
    float wnorm = 0.f;
    // layers
    Conv erb0, erb_dw[3], erb_pw[3], df0, df0_pw, df1_dw, df1_pw, path[4], ct_dw[3], ct_pw[3], out0, convp, convp_pw;
    const float *fc_emb = nullptr, *enc_lin_in = nullptr, *enc_lin_out = nullptr, *erb_lin_in = nullptr, *erb_lin_out = nullptr;
    const float *df_lin_in = nullptr, *df_skip = nullptr, *df_out = nullptr;
    std::vector<Gru> grus;                  // enc (1), erb decoder (emb_num_layers - 1), df decoder (df_num_layers)
    // workspace of the last call
    void* ws = nullptr; size_t ws_bytes = 0;
    int lastC = 0, lastF = 0; int64_t lastT = 0;
    struct Bufs {
        float2 *spec, *spec_e, *fspec; float *db, *ferb, *e[4], *c0, *c1, *tmp, *emb0, *emb, *gx, *proj, *gout[EGR_DFN3_MAX_GRU];
        float *demb, *pbuf, *dbuf, *mask, *dfc, *tcoef, *cpt, *cp, *coefs, *frames;
    } B;
};

namespace {

size_t layout(const Dfn3& m, int C, int nF, Dfn3::Bufs* B, char* base) {
    const egr_dfn3_config& c = m.cfg;
    const int64_t R = (int64_t)C * nF;
    const int ch = c.conv_ch, E = c.nb_erb, nb = c.nb_df, O2 = 2 * c.df_order;
    const int Hm = c.emb_hidden_dim > c.df_hidden_dim ? c.emb_hidden_dim : c.df_hidden_dim;
    const int Fm = E > nb ? E : nb;
    size_t off = 0;
    auto take = [&](int64_t nfl) -> float* {
        float* p = base ? (float*)(base + off) : nullptr;
        off += ((size_t)nfl * sizeof(float) + 255) & ~(size_t)255;
        return p;
    };
    Dfn3::Bufs b;
    b.spec = (float2*)take(R * m.Fq * 2);
    b.spec_e = (float2*)take(R * m.Fq * 2);
    b.fspec = (float2*)take(R * nb * 2);
    b.db = take(R * E);
    b.ferb = take(R * E);
    b.e[0] = take(R * E * ch);
    b.e[1] = take(R * (E / 2) * ch);
    b.e[2] = take(R * (E / 4) * ch);
    b.e[3] = take(R * (E / 4) * ch);
    b.c0 = take(R * nb * ch);
    b.c1 = take(R * (nb / 2) * ch);
    b.tmp = take(R * Fm * ch);
    b.emb0 = take(R * m.embd);
    b.emb = take(R * m.embd);
    b.gx = take(R * Hm);
    b.proj = take(R * 3 * Hm);
    for (size_t g = 0; g < EGR_DFN3_MAX_GRU; ++g) b.gout[g] = g < m.grus.size() ? take(R * m.grus[g].H) : nullptr;
    b.demb = take(R * m.embd);
    b.pbuf = take(R * E * ch);
    b.dbuf = take(R * E * ch);
    b.mask = take(R * E);
    b.dfc = take(R * c.df_hidden_dim);
    b.tcoef = take(R * nb * O2);
    b.cpt = take(R * nb * O2);
    b.cp = take(R * nb * O2);
    b.coefs = take(R * nb * O2);
    b.frames = take(R * c.fft_size);
    if (B) *B = b;
    return off;
}

int conv(const Conv& L, const float* x, float* y, int B, int T, int Fin, int fstride, int act, const float* res, hipStream_t st,
         int* Fout_ret = nullptr) {
    ConvArgs p;
    p.x = x; p.w = L.w; p.scale = L.scale; p.shift = L.shift; p.res = res; p.y = y;
    p.B = B; p.T = T; p.Fin = Fin; p.Cin = L.cin; p.Cout = L.cout; p.groups = L.groups; p.kt = L.kt; p.kf = L.kf; p.fstride = fstride;
    p.transposed = L.transposed; p.act = act;
    if (L.transposed) {
        p.fpad = L.kf / 2;
        p.Fout = (Fin - 1) * fstride - 2 * p.fpad + (L.kf - 1) + L.kf / 2 + 1;
    } else {
        p.fpad = L.kf / 2;
        p.Fout = (Fin + 2 * p.fpad - L.kf) / fstride + 1;
    }
    if (Fout_ret) *Fout_ret = p.Fout;
    hipLaunchKernelGGL(k_dfn_conv, dim3(grid_for((int64_t)B * T * p.Fout * p.Cout)), dim3(256), 0, st, p);
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

#define EGR_TRY(x) do { int rc__ = (x); if (rc__ != EGR_OK) return rc__; } while (0)

// x [C * nF][in] -> out [C * nF][H] through one GRU layer
int gru_layer(const Gru& g, const float* x, float* proj, float* out, int C, int nF, hipStream_t st) {
    const int64_t R = (int64_t)C * nF;
    EGR_TRY(egr_bgemm(x, g.wih, proj, 1, 1, (int)R, 3 * g.H, g.in, g.in, g.in, 3 * g.H, 0, 0, 0, 0, 0, 0, 1, 1.f, st));
    EGR_TRY(rows_op(proj, g.bih, nullptr, proj, R * 3 * g.H, 3 * g.H, 0, st));
    hipLaunchKernelGGL(k_dfn_gru, dim3(C), dim3(GRU_THREADS), 0, st, proj, g.whh_pk, g.bhh, g.H, nF, out);
    return EGR_OK;
}

int run(Dfn3& m, const float* x, int C, int64_t T, float* y, hipStream_t st) {
    const egr_dfn3_config& c = m.cfg;
    const int N = c.fft_size, hop = c.hop_size, nF = (int)((T + N) / hop);
    const int64_t R = (int64_t)C * nF;
    const int ch = c.conv_ch, E = c.nb_erb, nb = c.nb_df, O2 = 2 * c.df_order;
    const size_t need = layout(m, C, nF, nullptr, nullptr);
    if (need > m.ws_bytes) {
        if (m.ws) EGR_HIP(hipFreeAsync(m.ws, st));
        m.ws = nullptr;
        m.ws_bytes = 0;
        EGR_HIP(hipMallocAsync(&m.ws, need, st));
        m.ws_bytes = need;
    }
    Dfn3::Bufs& B = m.B;
    layout(m, C, nF, &B, (char*)m.ws);
    m.lastC = C; m.lastF = nF; m.lastT = T;
    // features
    hipLaunchKernelGGL(k_dfn_analysis, dim3(nF, C), dim3(256), (size_t)N * 24, st, x, T, nF, N, hop, m.tw, m.win, m.wnorm, B.spec);
    hipLaunchKernelGGL(k_dfn_erb_db, dim3(grid_for(R * E)), dim3(256), 0, st, B.spec, R, m.Fq, E, m.band_lo, m.band_w, B.db);
    const int la = c.conv_lookahead;
    hipLaunchKernelGGL(k_dfn_norm_scan, dim3((C * (E + nb) + 63) / 64), dim3(64), 0, st, B.db, B.spec, C, nF, m.Fq, E, nb,
                       c.norm_alpha, la, B.ferb, B.fspec);
    // encoder
    int F1 = 0, F2 = 0, F3 = 0, Fc = 0;
    EGR_TRY(conv(m.erb0, B.ferb, B.e[0], C, nF, E, 1, 1, nullptr, st));
    const int strides[3] = {2, 2, 1};
    int Fi = E;
    for (int i = 0; i < 3; ++i) {
        int Fo;
        EGR_TRY(conv(m.erb_dw[i], B.e[i], B.tmp, C, nF, Fi, strides[i], 0, nullptr, st, &Fo));
        EGR_TRY(conv(m.erb_pw[i], B.tmp, B.e[i + 1], C, nF, Fo, 1, 1, nullptr, st));
        Fi = Fo;
        if (i == 0) F1 = Fo; else if (i == 1) F2 = Fo; else F3 = Fo;
    }
    EGR_TRY(conv(m.df0, (const float*)B.fspec, B.tmp, C, nF, nb, 1, 0, nullptr, st));
    EGR_TRY(conv(m.df0_pw, B.tmp, B.c0, C, nF, nb, 1, 1, nullptr, st));
    EGR_TRY(conv(m.df1_dw, B.c0, B.tmp, C, nF, nb, 2, 0, nullptr, st, &Fc));
    EGR_TRY(conv(m.df1_pw, B.tmp, B.c1, C, nF, Fc, 1, 1, nullptr, st));
    EGR_CHECK(F3 * ch == m.embd && Fc * ch == ch * nb / 2 && F1 == E / 2 && F2 == E / 4, EGR_ERR_UNSUPPORTED, "egr_dfn3: encoder widths");
    EGR_TRY(grouped_linear(B.c1, m.fc_emb, B.emb0, R, Fc * ch, m.embd, c.enc_lin_groups, st));
    EGR_TRY(rows_op(B.emb0, nullptr, B.e[3], B.emb0, R * m.embd, m.embd, 1, st));      // emb = e3 + relu(fc_emb(c1))
    const int He = c.emb_hidden_dim, Hd = c.df_hidden_dim;
    int g = 0;
    EGR_TRY(grouped_linear(B.emb0, m.enc_lin_in, B.gx, R, m.embd, He, c.lin_groups, st));
    EGR_TRY(rows_op(B.gx, nullptr, nullptr, B.gx, R * He, He, 1, st));
    EGR_TRY(gru_layer(m.grus[g], B.gx, B.proj, B.gout[g], C, nF, st));
    EGR_TRY(grouped_linear(B.gout[g], m.enc_lin_out, B.emb, R, He, m.embd, c.lin_groups, st));
    EGR_TRY(rows_op(B.emb, nullptr, nullptr, B.emb, R * m.embd, m.embd, 1, st));
    ++g;
    // ERB decoder
    EGR_TRY(grouped_linear(B.emb, m.erb_lin_in, B.gx, R, m.embd, He, c.lin_groups, st));
    EGR_TRY(rows_op(B.gx, nullptr, nullptr, B.gx, R * He, He, 1, st));
    const float* xin = B.gx;
    for (int k = 0; k < c.emb_num_layers - 1; ++k, ++g) {
        EGR_TRY(gru_layer(m.grus[g], xin, B.proj, B.gout[g], C, nF, st));
        xin = B.gout[g];
    }
    EGR_TRY(grouped_linear(xin, m.erb_lin_out, B.demb, R, He, m.embd, c.lin_groups, st));
    EGR_TRY(rows_op(B.demb, nullptr, nullptr, B.demb, R * m.embd, m.embd, 1, st));
    EGR_TRY(conv(m.path[3], B.e[3], B.pbuf, C, nF, F3, 1, 1, B.demb, st));
    EGR_TRY(conv(m.ct_dw[0], B.pbuf, B.tmp, C, nF, F3, 1, 0, nullptr, st));
    EGR_TRY(conv(m.ct_pw[0], B.tmp, B.dbuf, C, nF, F3, 1, 1, nullptr, st));
    for (int i = 0; i < 2; ++i) {             // convt2 (E/4 -> E/2) on conv2p(e2) + d, convt1 (E/2 -> E) on conv1p(e1) + d
        const int Fin = i == 0 ? F2 : F1, Fwant = i == 0 ? F1 : E;
        EGR_TRY(conv(m.path[2 - i], B.e[2 - i], B.pbuf, C, nF, Fin, 1, 1, B.dbuf, st));
        int Fo = 0;
        EGR_TRY(conv(m.ct_dw[1 + i], B.pbuf, B.tmp, C, nF, Fin, 2, 0, nullptr, st, &Fo));
        EGR_CHECK(Fo == Fwant, EGR_ERR_UNSUPPORTED, "egr_dfn3: transposed conv width %d != %d", Fo, Fwant);
        EGR_TRY(conv(m.ct_pw[1 + i], B.tmp, B.dbuf, C, nF, Fo, 1, 1, nullptr, st));
    }
    EGR_TRY(conv(m.path[0], B.e[0], B.pbuf, C, nF, E, 1, 1, B.dbuf, st));
    EGR_TRY(conv(m.out0, B.pbuf, B.mask, C, nF, E, 1, 2, nullptr, st));
    // DF decoder
    EGR_TRY(grouped_linear(B.emb, m.df_lin_in, B.gx, R, m.embd, Hd, c.lin_groups, st));
    EGR_TRY(rows_op(B.gx, nullptr, nullptr, B.gx, R * Hd, Hd, 1, st));
    xin = B.gx;
    for (int k = 0; k < c.df_num_layers; ++k, ++g) {
        EGR_TRY(gru_layer(m.grus[g], xin, B.proj, B.gout[g], C, nF, st));
        xin = B.gout[g];
    }
    if (m.df_skip) {
        EGR_TRY(grouped_linear(B.emb, m.df_skip, B.dfc, R, m.embd, Hd, c.lin_groups, st));
        EGR_TRY(rows_op(B.dfc, nullptr, xin, B.dfc, R * Hd, Hd, 0, st));
        xin = B.dfc;
    }
    EGR_TRY(grouped_linear(xin, m.df_out, B.tcoef, R, Hd, nb * O2, c.lin_groups, st));
    EGR_TRY(conv(m.convp, B.c0, B.cpt, C, nF, nb, 1, 0, nullptr, st));
    EGR_TRY(conv(m.convp_pw, B.cpt, B.cp, C, nF, nb, 1, 1, nullptr, st));
    EGR_TRY(rows_op(B.tcoef, nullptr, B.cp, B.coefs, R * nb * O2, nb * O2, 3, st));      // tanh(df_out(c)) + df_convp(c0)
    // mask + deep filter, synthesis
    hipLaunchKernelGGL(k_dfn_assemble, dim3(grid_for(R * m.Fq)), dim3(256), 0, st, B.spec, B.mask, B.coefs, m.band_of, C, nF, m.Fq, E,
                       nb, c.df_order, c.df_lookahead, B.spec_e);
    hipLaunchKernelGGL(k_dfn_synth, dim3(nF, C), dim3(256), (size_t)(m.Fq + N) * 16, st, B.spec_e, nF, N, m.tw, m.win, B.frames);
    hipLaunchKernelGGL(k_dfn_ola, dim3(grid_for((int64_t)C * T)), dim3(256), 0, st, B.frames, C, nF, N, hop, T, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

}  // namespace
}  // namespace egr

using egr::Dfn3;

extern "C" int egr_dfn3_create(void** handle, const egr_dfn3_config* cfg, const float* packed, int64_t n_floats, int device) {
    using namespace egr;
    EGR_CHECK(handle && cfg && packed && n_floats > 0, EGR_ERR_ARG, "egr_dfn3_create: null argument");
    EGR_CHECK(cfg->struct_bytes == (int)sizeof(egr_dfn3_config), EGR_ERR_ARG, "egr_dfn3_create: struct_bytes %d != %d",
              cfg->struct_bytes, (int)sizeof(egr_dfn3_config));
    const egr_dfn3_config& c = *cfg;
    const int ch = c.conv_ch, E = c.nb_erb, nb = c.nb_df, O2 = 2 * c.df_order;
    const int ngru = 1 + (c.emb_num_layers - 1) + c.df_num_layers;
    EGR_CHECK(c.fft_size > 0 && c.hop_size > 0 && c.fft_size % c.hop_size == 0 && c.fft_size % 2 == 0 && c.fft_size <= 4096, EGR_ERR_UNSUPPORTED,
              "egr_dfn3: fft_size %d / hop_size %d", c.fft_size, c.hop_size);
    EGR_CHECK(E > 0 && E <= EGR_DFN3_MAX_ERB && E % 4 == 0 && nb > 0 && nb % 2 == 0 && nb <= c.fft_size / 2 + 1, EGR_ERR_UNSUPPORTED,
              "egr_dfn3: nb_erb %d / nb_df %d", E, nb);
    EGR_CHECK(c.emb_hidden_dim > 0 && c.emb_hidden_dim <= GRU_HMAX && c.df_hidden_dim > 0 && c.df_hidden_dim <= GRU_HMAX,
              EGR_ERR_UNSUPPORTED, "egr_dfn3: GRU widths must be <= %d", GRU_HMAX);
    EGR_CHECK(c.emb_num_layers >= 2 && c.df_num_layers >= 1 && ngru <= EGR_DFN3_MAX_GRU, EGR_ERR_UNSUPPORTED, "egr_dfn3: GRU layer counts");
    EGR_CHECK(c.df_order >= 1 && c.df_lookahead >= 0 && c.df_lookahead < c.df_order && c.conv_lookahead >= 0, EGR_ERR_UNSUPPORTED,
              "egr_dfn3: df_order / lookaheads");
    EGR_CHECK(ch > 0 && c.lin_groups > 0 && c.enc_lin_groups > 0 && c.path_groups > 0 && ch % c.path_groups == 0 && c.df_path_groups > 0 &&
              ch % c.df_path_groups == 0 && O2 % c.df_path_groups == 0, EGR_ERR_UNSUPPORTED, "egr_dfn3: conv groups");
    // a stride-2 transposed conv with padding kf / 2 and output_padding kf / 2 doubles the width only for kf = 3 (torch refuses
    // output_padding >= stride for the wider kernels)
    EGR_CHECK(c.convt_kf == 3, EGR_ERR_UNSUPPORTED, "egr_dfn3: transposed conv kernel width %d (supported: 3)", c.convt_kf);
    EGR_CHECK(c.kf % 2 == 1 && c.kf_inp % 2 == 1 && c.kt >= 1 && c.kt_inp >= 1 && c.df_pathway_kt >= 1, EGR_ERR_UNSUPPORTED,
              "egr_dfn3: frequency kernels must be odd (same-size padding)");
    int wsum = 0;
    for (int e = 0; e < E; ++e) { EGR_CHECK(c.erb_widths[e] > 0, EGR_ERR_ARG, "egr_dfn3: ERB width %d", e); wsum += c.erb_widths[e]; }
    EGR_CHECK(wsum == c.fft_size / 2 + 1, EGR_ERR_ARG, "egr_dfn3: ERB widths sum %d != %d", wsum, c.fft_size / 2 + 1);

    Dfn3* m = new Dfn3();
    m->cfg = c;
    m->device = device;
    m->Fq = c.fft_size / 2 + 1;
    m->E4 = E / 4;
    m->embd = ch * E / 4;
    // packed order: dfn_weights.pack_order
    int64_t pos = 0;                                        // floats consumed so far
    auto W = [&](int64_t k) { pos += k; return pos - k; };
    struct ConvSpec { Conv* L; int64_t w, s, t; };
    std::vector<ConvSpec> convs;
    auto cv = [&](Conv& L, int cin, int cout, int groups, int kt, int kf, int transposed = 0) {
        L.cin = cin; L.cout = cout; L.groups = groups; L.kt = kt; L.kf = kf; L.transposed = transposed;
        ConvSpec s{&L, W((int64_t)(transposed ? cin * (cout / groups) : cout * (cin / groups)) * kt * kf), -1, -1};
        convs.push_back(s);
    };
    auto bn = [&](int n) { ConvSpec& s = convs.back(); s.s = W(n); s.t = W(n); };
    cv(m->erb0, 1, ch, 1, c.kt_inp, c.kf_inp); bn(ch);
    for (int i = 0; i < 3; ++i) { cv(m->erb_dw[i], ch, ch, ch, c.kt, c.kf); cv(m->erb_pw[i], ch, ch, 1, 1, 1); bn(ch); }
    cv(m->df0, 2, ch, 2, c.kt_inp, c.kf_inp); cv(m->df0_pw, ch, ch, 1, 1, 1); bn(ch);
    cv(m->df1_dw, ch, ch, ch, c.kt, c.kf); cv(m->df1_pw, ch, ch, 1, 1, 1); bn(ch);
    const int64_t o_fc = W((int64_t)(ch * nb / 2) * m->embd / c.enc_lin_groups);
    struct GruSpec { int64_t lin_in = -1, wih, whh, bih, bhh; int in, H; };
    std::vector<GruSpec> gs;
    auto sq = [&](int in, int H, int layers, int64_t* lin_in) {
        *lin_in = W((int64_t)in * H / c.lin_groups);
        for (int k = 0; k < layers; ++k) {
            GruSpec g;
            g.in = H; g.H = H;
            g.wih = W((int64_t)3 * H * H); g.whh = W((int64_t)3 * H * H); g.bih = W(3 * H); g.bhh = W(3 * H);
            gs.push_back(g);
        }
    };
    int64_t o_enc_in, o_enc_out, o_erb_in, o_erb_out, o_df_in, o_skip = -1, o_dfout;
    sq(m->embd, c.emb_hidden_dim, 1, &o_enc_in);
    o_enc_out = W((int64_t)c.emb_hidden_dim * m->embd / c.lin_groups);
    sq(m->embd, c.emb_hidden_dim, c.emb_num_layers - 1, &o_erb_in);
    o_erb_out = W((int64_t)c.emb_hidden_dim * m->embd / c.lin_groups);
    for (int i = 0; i < 3; ++i) {
        cv(m->path[3 - i], ch, ch, c.path_groups, 1, 1); bn(ch);
        if (i == 0) cv(m->ct_dw[0], ch, ch, ch, c.kt, c.kf);
        else cv(m->ct_dw[i], ch, ch, ch, 1, c.convt_kf, 1);
        cv(m->ct_pw[i], ch, ch, 1, 1, 1); bn(ch);
    }
    cv(m->path[0], ch, ch, c.path_groups, 1, 1); bn(ch);
    cv(m->out0, ch, 1, 1, c.kt, c.kf); bn(1);
    sq(m->embd, c.df_hidden_dim, c.df_num_layers, &o_df_in);
    if (c.df_gru_skip) o_skip = W((int64_t)m->embd * c.df_hidden_dim / c.lin_groups);
    o_dfout = W((int64_t)c.df_hidden_dim * nb * O2 / c.lin_groups);
    cv(m->convp, ch, O2, c.df_path_groups, c.df_pathway_kt, 1);
    cv(m->convp_pw, O2, O2, 1, 1, 1); bn(O2);
    if (pos != n_floats) {
        set_error("egr_dfn3_create: packed weights hold %lld floats, the config needs %lld", (long long)n_floats, (long long)pos);
        delete m;
        return EGR_ERR_ARG;
    }
    // device image: packed weights | repacked W_hh per layer | twiddles (double2) | window | band tables
    const int64_t n_whh = (int64_t)GRU_PER_THREAD * GRU_THREADS;
    const int N = c.fft_size;
    const int64_t o_whh = (n_floats + 63) & ~63LL;
    const int64_t o_tw = o_whh + (int64_t)gs.size() * n_whh;
    const int64_t o_win = o_tw + 4LL * N;
    const int64_t o_tab = o_win + N;
    const int64_t total = o_tab + 2 * E + m->Fq;
    std::vector<float> img((size_t)total, 0.f);
    memcpy(img.data(), packed, sizeof(float) * n_floats);
    for (size_t g = 0; g < gs.size(); ++g) {            // W_hh [3H][H] -> thread-minor (element, thread) order of k_dfn_gru
        const int H = gs[g].H;
        const float* w = packed + gs[g].whh;
        float* dst = img.data() + o_whh + g * n_whh;
        for (int t = 0; t < GRU_THREADS; ++t)
            for (int e = 0; e < GRU_PER_THREAD; ++e) {
                const int j = e / GRU_K, k = e % GRU_K;
                const int q = j * GRU_THREADS + t, row = q / GRU_SEG, col = GRU_SEG * k + q % GRU_SEG;
                dst[(int64_t)e * GRU_THREADS + t] = (row < 3 * H && col < H) ? w[(int64_t)row * H + col] : 0.f;
            }
    }
    double* twd = (double*)(img.data() + o_tw);
    for (int n = 0; n < N; ++n) {
        twd[2 * n] = cos(2.0 * M_PI * n / N);
        twd[2 * n + 1] = sin(2.0 * M_PI * n / N);
    }
    const int h = N / 2;
    for (int n = 0; n < N; ++n) {
        const double s = sin(0.5 * M_PI * (n + 0.5) / h);
        img[o_win + n] = (float)sin(0.5 * M_PI * s * s);
    }
    int* tab = (int*)(img.data() + o_tab);
    int lo = 0;
    for (int e = 0; e < E; ++e) {
        tab[e] = lo;
        tab[E + e] = c.erb_widths[e];
        for (int j = 0; j < c.erb_widths[e]; ++j) tab[2 * E + lo + j] = e;
        lo += c.erb_widths[e];
    }
    m->wnorm = 1.f / ((float)N * (float)N / (float)(2 * c.hop_size));
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess ||
        hipMalloc(&m->dev_w, sizeof(float) * total) != hipSuccess ||
        hipMemcpy(m->dev_w, img.data(), sizeof(float) * total, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("egr_dfn3_create: device allocation / upload failed on device %d", device);
        if (m->dev_w) (void)hipFree(m->dev_w);
        (void)hipSetDevice(prev);
        delete m;
        return EGR_ERR_HIP;
    }
    // the analysis / synthesis DFTs keep a frame and the twiddles in dynamic LDS: 24 N and 16 (1.5 N + 1) bytes, above the 64 KiB
    // default from N = 2732 on.  The attribute is a process-wide cap per kernel, so it is raised to the CU's maximum (as the Fat-Llama
    // plans do), never to this config's need.
    const size_t lds_an = (size_t)N * 24, lds_syn = (size_t)(m->Fq + N) * 16;
    hipError_t ea = hipSuccess;
    if (lds_an > (size_t)DFN_LDS_MAX || lds_syn > (size_t)DFN_LDS_MAX) {
        set_error("egr_dfn3_create: fft_size %d needs %zu / %zu bytes of LDS (limit %d)", N, lds_an, lds_syn, DFN_LDS_MAX);
        ea = hipErrorInvalidValue;
    }
    if (ea == hipSuccess) ea = hipFuncSetAttribute((const void*)k_dfn_analysis, hipFuncAttributeMaxDynamicSharedMemorySize, DFN_LDS_MAX);
    if (ea == hipSuccess) ea = hipFuncSetAttribute((const void*)k_dfn_synth, hipFuncAttributeMaxDynamicSharedMemorySize, DFN_LDS_MAX);
    if (ea != hipSuccess) {
        if (lds_an <= (size_t)DFN_LDS_MAX && lds_syn <= (size_t)DFN_LDS_MAX)
            set_error("egr_dfn3_create: hipFuncSetAttribute(MaxDynamicSharedMemorySize) -> %s", hipGetErrorString(ea));
        (void)hipFree(m->dev_w);
        (void)hipSetDevice(prev);
        delete m;
        return EGR_ERR_HIP;
    }
    (void)hipSetDevice(prev);
    float* D = m->dev_w;
    for (auto& s : convs) {
        s.L->w = D + s.w;
        if (s.s >= 0) { s.L->scale = D + s.s; s.L->shift = D + s.t; }
    }
    m->fc_emb = D + o_fc;
    m->enc_lin_in = D + o_enc_in; m->enc_lin_out = D + o_enc_out;
    m->erb_lin_in = D + o_erb_in; m->erb_lin_out = D + o_erb_out;
    m->df_lin_in = D + o_df_in; m->df_skip = o_skip >= 0 ? D + o_skip : nullptr; m->df_out = D + o_dfout;
    for (size_t g = 0; g < gs.size(); ++g) {
        Gru G;
        G.in = gs[g].in; G.H = gs[g].H;
        G.wih = D + gs[g].wih; G.bih = D + gs[g].bih; G.bhh = D + gs[g].bhh; G.whh_pk = D + o_whh + g * n_whh;
        m->grus.push_back(G);
    }
    m->tw = (const double2*)(D + o_tw);
    m->win = D + o_win;
    m->band_lo = (const int*)(D + o_tab);
    m->band_w = (const int*)(D + o_tab) + E;
    m->band_of = (const int*)(D + o_tab) + 2 * E;
    *handle = m;
    return EGR_OK;
}

extern "C" size_t egr_dfn3_workspace_bytes(void* handle, int channels, int64_t n) {
    if (!handle || channels < 1 || n < 1) return 0;
    Dfn3* m = (Dfn3*)handle;
    return egr::layout(*m, channels, (int)((n + m->cfg.fft_size) / m->cfg.hop_size), nullptr, nullptr);
}

extern "C" int egr_dfn3_enhance(void* handle, const float* x48, int channels, int64_t n, float* y, void* stream) {
    using namespace egr;
    EGR_CHECK(handle && x48 && y && channels >= 1 && channels <= 65535 && n >= 1, EGR_ERR_ARG, "egr_dfn3_enhance: bad argument");
    Dfn3* m = (Dfn3*)handle;
    EGR_CHECK((n + m->cfg.fft_size) / m->cfg.hop_size <= 65535LL * 4096, EGR_ERR_UNSUPPORTED, "egr_dfn3_enhance: input too long");
    EGR_CHECK((n + m->cfg.fft_size) / m->cfg.hop_size <= 2147483647LL / 4096, EGR_ERR_UNSUPPORTED, "egr_dfn3_enhance: input too long");
    int cur = -1;
    EGR_HIP(hipGetDevice(&cur));
    EGR_CHECK(cur == m->device, EGR_ERR_ARG, "egr_dfn3_enhance: handle belongs to device %d, current device is %d", m->device, cur);
    return run(*m, x48, channels, n, y, (hipStream_t)stream);
}

extern "C" int egr_dfn3_stage(void* handle, int stage, float* dst, int64_t capacity, int64_t* count, void* stream) {
    using namespace egr;
    EGR_CHECK(handle && count, EGR_ERR_ARG, "egr_dfn3_stage: null argument");
    Dfn3* m = (Dfn3*)handle;
    EGR_CHECK(m->ws, EGR_ERR_ARG, "egr_dfn3_stage: no enhance call yet");
    const int64_t R = (int64_t)m->lastC * m->lastF;
    const egr_dfn3_config& c = m->cfg;
    const Dfn3::Bufs& B = m->B;
    const float* src = nullptr;
    int64_t n = 0;
    switch (stage) {
        case EGR_DFN3_STAGE_SPEC: src = (const float*)B.spec; n = R * m->Fq * 2; break;
        case EGR_DFN3_STAGE_FEAT_ERB: src = B.ferb; n = R * c.nb_erb; break;
        case EGR_DFN3_STAGE_FEAT_SPEC: src = (const float*)B.fspec; n = R * c.nb_df * 2; break;
        case EGR_DFN3_STAGE_E0: src = B.e[0]; n = R * c.nb_erb * c.conv_ch; break;
        case EGR_DFN3_STAGE_E1: src = B.e[1]; n = R * (c.nb_erb / 2) * c.conv_ch; break;
        case EGR_DFN3_STAGE_E2: src = B.e[2]; n = R * (c.nb_erb / 4) * c.conv_ch; break;
        case EGR_DFN3_STAGE_E3: src = B.e[3]; n = R * (c.nb_erb / 4) * c.conv_ch; break;
        case EGR_DFN3_STAGE_C0: src = B.c0; n = R * c.nb_df * c.conv_ch; break;
        case EGR_DFN3_STAGE_EMB: src = B.emb; n = R * m->embd; break;
        case EGR_DFN3_STAGE_MASK: src = B.mask; n = R * c.nb_erb; break;
        case EGR_DFN3_STAGE_COEFS: src = B.coefs; n = R * c.nb_df * 2 * c.df_order; break;
        case EGR_DFN3_STAGE_SPEC_E: src = (const float*)B.spec_e; n = R * m->Fq * 2; break;
        default:
            if (stage >= EGR_DFN3_STAGE_GRU0 && stage < EGR_DFN3_STAGE_GRU0 + (int)m->grus.size()) {
                const int g = stage - EGR_DFN3_STAGE_GRU0;
                src = B.gout[g];
                n = R * m->grus[g].H;
            }
    }
    EGR_CHECK(src, EGR_ERR_ARG, "egr_dfn3_stage: unknown stage %d", stage);
    *count = n;
    if (!dst) return EGR_OK;
    EGR_CHECK(capacity >= n, EGR_ERR_ARG, "egr_dfn3_stage: capacity %lld < %lld", (long long)capacity, (long long)n);
    EGR_HIP(hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return EGR_OK;
}

extern "C" int egr_dfn3_time_gru(void* handle, int layer, int channels, int64_t steps, double* us_per_step) {
    using namespace egr;
    EGR_CHECK(handle && us_per_step && channels >= 1 && channels <= 64 && steps >= 1 && steps <= 10000000, EGR_ERR_ARG,
              "egr_dfn3_time_gru: bad argument");
    Dfn3* m = (Dfn3*)handle;
    EGR_CHECK(layer >= 0 && layer < (int)m->grus.size(), EGR_ERR_ARG, "egr_dfn3_time_gru: layer %d", layer);
    const Gru& g = m->grus[layer];
    float *proj = nullptr, *out = nullptr;
    hipEvent_t e0, e1;
    EGR_HIP(hipMalloc(&proj, sizeof(float) * channels * steps * 3 * g.H));
    EGR_HIP(hipMalloc(&out, sizeof(float) * channels * steps * g.H));
    EGR_HIP(hipMemset(proj, 0, sizeof(float) * channels * steps * 3 * g.H));
    EGR_HIP(hipEventCreate(&e0));
    EGR_HIP(hipEventCreate(&e1));
    hipLaunchKernelGGL(k_dfn_gru, dim3(channels), dim3(GRU_THREADS), 0, 0, proj, g.whh_pk, g.bhh, g.H, (int)(steps < 64 ? steps : 64), out);
    EGR_HIP(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k_dfn_gru, dim3(channels), dim3(GRU_THREADS), 0, 0, proj, g.whh_pk, g.bhh, g.H, (int)steps, out);
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

extern "C" int egr_dfn3_destroy(void* handle) {
    if (!handle) return EGR_OK;
    Dfn3* m = (Dfn3*)handle;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(m->device);
    if (m->ws) {                               // hipMallocAsync memory: returned stream-ordered, then waited for (not a pipeline call)
        (void)hipFreeAsync(m->ws, nullptr);
        (void)hipDeviceSynchronize();
    }
    if (m->dev_w) (void)hipFree(m->dev_w);
    (void)hipSetDevice(prev);
    delete m;
    return EGR_OK;
}

// ================================================================================================ DeepFilterNet2
// SPEC.md "4c. DeepFilterNet2 (UPSTREAM-RECALL)".  The signal path, the convolutions, the grouped linears without bias
// (GroupedLinearEinsum) and the synthesis are the DeepFilterNet3 kernels above, launched through the same host helpers; what is new:
//   k_dfn2_gru      : one GroupedGRU layer: workgroup (group, audio channel), W_hh block of the group in VGPRs, the P4 shuffle and the
//                     running sum of layer outputs in the store
//   k_dfn2_epi      : bias / activation / P3 output shuffle / residual epilogue of the GroupedLinear GEMMs
//   k_dfn2_alpha    : alpha = sigmoid(Linear(H_df -> 1)(c)) per frame
//   k_dfn2_assemble : ERB mask on every bin, the deep filter on the MASKED bins below nb_df, blended with alpha (P7)
namespace egr {
namespace {

constexpr int G2_HMAX = 128;                // per-group width k_dfn2_gru holds (h = H / G > 128 only for G = 1: the dense k_dfn_gru)

// Thread (j, s) = (threadIdx.x / S, threadIdx.x % S) of workgroup (g, b) owns gate rows j, h + j, 2h + j of group g's W_hh over the
// columns c = s + S k (k < K), 3K weights in VGPRs (zero beyond h), thread-minor in whh_pk so the one-time load is coalesced.  Per
// step: K values of h_{t-1} from LDS (double buffer, zero beyond h), 3K FMAs, an S-lane xor sum of the three gate sums, the update
// (every lane of the row group computes it; lane 0 stores), one barrier.  proj = W_ih x of all frames (egr_bgemm); b_ih is added here.
// Store: layer output at its P4 position (shuffled when `shuffle`), and sum_out = sum_in + it (sum_in null: the first layer).
template <int K>
__global__ __launch_bounds__(512) void k_dfn2_gru(const float* __restrict__ proj, const float* __restrict__ whh_pk,
                                                   const float* __restrict__ bih, const float* __restrict__ bhh, int G, int h, int S,
                                                   int nF, int shuffle, const float* __restrict__ sum_in, float* __restrict__ out,
                                                   float* __restrict__ sum_out) {
    __shared__ float hs[2][G2_HMAX];
    const int t = threadIdx.x, NT = h * S, j = t / S, s = t - j * S;
    const int g = blockIdx.x, b = blockIdx.y, H = G * h, H3 = 3 * H;
    const float* pb = proj + (int64_t)b * nF * H3 + g * 3 * h;
    const int n = g * h + j;                                   // pre-shuffle output index
    const int pos = shuffle ? (n % G) * h + n / G : n;         // P3: output g' h + j' takes pre-shuffle j' G + g'
    float* ob = out + (int64_t)b * nF * H + pos;
    float* sb = sum_out + (int64_t)b * nF * H + pos;
    const float* si = sum_in ? sum_in + (int64_t)b * nF * H + pos : nullptr;
    float w[3 * K];
    const float* wp = whh_pk + (int64_t)g * 3 * K * NT + t;
#pragma unroll
    for (int e = 0; e < 3 * K; ++e) w[e] = wp[(int64_t)e * NT];
    for (int i = t; i < 2 * G2_HMAX; i += NT) hs[i / G2_HMAX][i % G2_HMAX] = 0.f;
    const int rj = g * 3 * h + j;
    const float br = bhh[rj], bz = bhh[rj + h], bn = bhh[rj + 2 * h];
    const float ir = bih[rj], iz = bih[rj + h], in_ = bih[rj + 2 * h];
    float xr = 0.f, xz = 0.f, xn = 0.f, hp = 0.f;
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
__global__ void k_dfn2_assemble(const float2* __restrict__ spec, const float* __restrict__ mask, const float* __restrict__ coefs,
                                const float* __restrict__ alpha, const int* __restrict__ band_of, int C, int nF, int Fq, int E, int nbdf,
                                int order, int look, float2* __restrict__ out) {
    const int64_t n = (int64_t)C * nF * Fq;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int f = (int)(i % Fq);
        const int64_t r = i / Fq;                  // b * nF + t
        const int t = (int)(r % nF);
        const int64_t b = r / nF;
        const int band = band_of[f];
        const float m = mask[r * E + band];
        const float2 s = spec[i];
        const float2 sm = make_float2(s.x * m, s.y * m);
        float2 y = sm;
        if (f < nbdf) {
            const float* c = coefs + (r * nbdf + f) * 2 * order;
            float re = 0.f, im = 0.f;
            for (int k = 0; k < order; ++k) {
                const int ts = t - (order - 1 - look) + k;
                if (ts < 0 || ts >= nF) continue;
                const int64_t rs = b * nF + ts;
                const float ms = mask[rs * E + band];
                const float2 x = spec[rs * Fq + f];
                const float2 xm = make_float2(x.x * ms, x.y * ms);
                re = fmaf(xm.x, c[2 * k], fmaf(-xm.y, c[2 * k + 1], re));
                im = fmaf(xm.x, c[2 * k + 1], fmaf(xm.y, c[2 * k], im));
            }
            const float a = alpha[r], a1 = 1.f - a;
            y = make_float2(re * a + sm.x * a1, im * a + sm.y * a1);
        }
        out[i] = y;
    }
}

struct GGru {                 // one GroupedGRU layer: G GRUs of width h on input slices of width in / G
    const float* wih = nullptr; const float* bih = nullptr; const float* bhh = nullptr; float* whh_pk = nullptr;
    int in = 0, H = 0, G = 1, h = 0, K = 0, S = 1, shuffle = 0;
    bool dense() const { return h > G2_HMAX; }
};

// K (16 or 32 columns per lane) and S (lanes per gate row) of k_dfn2_gru for a group width h <= G2_HMAX
inline void ggru_shape(int h, int* K, int* S) {
    *K = h <= 16 ? 16 : 32;
    *S = 1;
    while (*K * *S < h) *S *= 2;
}

}  // namespace

struct Dfn2 {
    egr_dfn2_config cfg;
    int device = 0, Fq = 0, embd = 0;
    float* dev_w = nullptr;
    const double2* tw = nullptr; const float* win = nullptr; const int* band_lo = nullptr; const int* band_w = nullptr;
    const int* band_of = nullptr;
    float wnorm = 0.f;
    Conv erb0, erb_dw[3], erb_pw[3], df0, df0_pw, df1_dw, df1_pw, path[4], ct_dw[3], ct_pw[3], out0, convp, convp_pw;
    const float *fc_emb_w = nullptr, *fc_emb_b = nullptr, *erb_fc_w = nullptr, *erb_fc_b = nullptr;
    const float *df_skip = nullptr, *df_out = nullptr, *df_out_b = nullptr, *fc_a_w = nullptr, *fc_a_b = nullptr;
    std::vector<GGru> grus;                 // enc (1), erb decoder (emb_num_layers - 1), df decoder (df_num_layers)
    void* ws = nullptr; size_t ws_bytes = 0;
    int lastC = 0, lastF = 0; int64_t lastT = 0;
    struct Bufs {
        float2 *spec, *spec_e, *fspec; float *db, *ferb, *e[4], *c0, *c1, *tmp, *lin, *emb0, *proj, *gout[EGR_DFN3_MAX_GRU];
        float *gsum[EGR_DFN3_MAX_GRU], *dfc, *alpha, *demb, *pbuf, *dbuf, *mask, *tcoef, *cpt, *cp, *coefs, *frames;
    } B;
};

namespace {

size_t layout2(const Dfn2& m, int C, int nF, Dfn2::Bufs* B, char* base) {
    const egr_dfn2_config& c = m.cfg;
    const int64_t R = (int64_t)C * nF;
    const int ch = c.conv_ch, E = c.nb_erb, nb = c.nb_df, O2 = 2 * c.df_order;
    const int Hm = c.emb_hidden_dim > c.df_hidden_dim ? c.emb_hidden_dim : c.df_hidden_dim;
    const int Fm = E > nb ? E : nb;
    const int Lm = m.embd > nb * O2 ? m.embd : nb * O2;
    size_t off = 0;
    auto take = [&](int64_t nfl) -> float* {
        float* p = base ? (float*)(base + off) : nullptr;
        off += ((size_t)nfl * sizeof(float) + 255) & ~(size_t)255;
        return p;
    };
    Dfn2::Bufs b;
    b.spec = (float2*)take(R * m.Fq * 2);
    b.spec_e = (float2*)take(R * m.Fq * 2);
    b.fspec = (float2*)take(R * nb * 2);
    b.db = take(R * E);
    b.ferb = take(R * E);
    b.e[0] = take(R * E * ch);
    b.e[1] = take(R * (E / 2) * ch);
    b.e[2] = take(R * (E / 4) * ch);
    b.e[3] = take(R * (E / 4) * ch);
    b.c0 = take(R * nb * ch);
    b.c1 = take(R * (nb / 2) * ch);
    b.tmp = take(R * Fm * ch);
    b.lin = take(R * Lm);
    b.emb0 = take(R * m.embd);
    b.proj = take(R * 3 * Hm);
    for (size_t g = 0; g < EGR_DFN3_MAX_GRU; ++g) b.gout[g] = g < m.grus.size() ? take(R * m.grus[g].H) : nullptr;
    for (size_t g = 0; g < EGR_DFN3_MAX_GRU; ++g) b.gsum[g] = g < m.grus.size() ? take(R * m.grus[g].H) : nullptr;
    b.dfc = take(R * c.df_hidden_dim);
    b.alpha = take(R);
    b.demb = take(R * m.embd);
    b.pbuf = take(R * E * ch);
    b.dbuf = take(R * E * ch);
    b.mask = take(R * E);
    b.tcoef = take(R * nb * O2);
    b.cpt = take(R * nb * O2);
    b.cp = take(R * nb * O2);
    b.coefs = take(R * nb * O2);
    b.frames = take(R * c.fft_size);
    if (B) *B = b;
    return off;
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

void launch_ggru(const GGru& g, const float* proj, const float* sum_in, float* out, float* sum_out, int C, int nF, hipStream_t st) {
    const dim3 grid(g.G, C), block(g.h * g.S);
    if (g.K == 16)
        hipLaunchKernelGGL(k_dfn2_gru<16>, grid, block, 0, st, proj, g.whh_pk, g.bih, g.bhh, g.G, g.h, g.S, nF, g.shuffle, sum_in, out, sum_out);
    else
        hipLaunchKernelGGL(k_dfn2_gru<32>, grid, block, 0, st, proj, g.whh_pk, g.bih, g.bhh, g.G, g.h, g.S, nF, g.shuffle, sum_in, out, sum_out);
}

// x [C * nF][in] -> out (the layer output as passed on) and sum_out (= sum_in + out) [C * nF][H] through one GroupedGRU layer
int ggru_layer(const GGru& g, const float* x, float* proj, const float* sum_in, float* out, float* sum_out, int C, int nF, hipStream_t st) {
    const int64_t R = (int64_t)C * nF;
    const int I = g.in / g.G, h3 = 3 * g.h;
    EGR_TRY(egr_bgemm(x, g.wih, proj, 1, g.G, (int)R, h3, I, g.in, I, 3 * g.H, 0, I, 0, (int64_t)h3 * I, 0, h3, 1, 1.f, st));
    if (g.dense()) {                       // G = 1 and H > 128: a plain nn.GRU layer, no shuffle
        EGR_TRY(rows_op(proj, g.bih, nullptr, proj, R * 3 * g.H, 3 * g.H, 0, st));
        hipLaunchKernelGGL(k_dfn_gru, dim3(C), dim3(GRU_THREADS), 0, st, proj, g.whh_pk, g.bhh, g.H, nF, out);
        return rows_op(out, nullptr, sum_in, sum_out, R * g.H, g.H, 0, st);
    }
    launch_ggru(g, proj, sum_in, out, sum_out, C, nF, st);
    return EGR_OK;
}

int run2(Dfn2& m, const float* x, int C, int64_t T, float* y, hipStream_t st) {
    const egr_dfn2_config& c = m.cfg;
    const int N = c.fft_size, hop = c.hop_size, nF = (int)((T + N) / hop);
    const int64_t R = (int64_t)C * nF;
    const int ch = c.conv_ch, E = c.nb_erb, nb = c.nb_df, O2 = 2 * c.df_order;
    const size_t need = layout2(m, C, nF, nullptr, nullptr);
    if (need > m.ws_bytes) {
        if (m.ws) EGR_HIP(hipFreeAsync(m.ws, st));
        m.ws = nullptr;
        m.ws_bytes = 0;
        EGR_HIP(hipMallocAsync(&m.ws, need, st));
        m.ws_bytes = need;
    }
    Dfn2::Bufs& B = m.B;
    layout2(m, C, nF, &B, (char*)m.ws);
    m.lastC = C; m.lastF = nF; m.lastT = T;
    // features (P1: the conv_lookahead shift whenever it is > 0)
    hipLaunchKernelGGL(k_dfn_analysis, dim3(nF, C), dim3(256), (size_t)N * 24, st, x, T, nF, N, hop, m.tw, m.win, m.wnorm, B.spec);
    hipLaunchKernelGGL(k_dfn_erb_db, dim3(grid_for(R * E)), dim3(256), 0, st, B.spec, R, m.Fq, E, m.band_lo, m.band_w, B.db);
    hipLaunchKernelGGL(k_dfn_norm_scan, dim3((C * (E + nb) + 63) / 64), dim3(64), 0, st, B.db, B.spec, C, nF, m.Fq, E, nb,
                       c.norm_alpha, c.conv_lookahead, B.ferb, B.fspec);
    // encoder (P2)
    int F1 = 0, F2 = 0, F3 = 0, Fc = 0;
    EGR_TRY(conv(m.erb0, B.ferb, B.e[0], C, nF, E, 1, 1, nullptr, st));
    const int strides[3] = {2, 2, 1};
    int Fi = E;
    for (int i = 0; i < 3; ++i) {
        int Fo;
        EGR_TRY(conv(m.erb_dw[i], B.e[i], B.tmp, C, nF, Fi, strides[i], 0, nullptr, st, &Fo));
        EGR_TRY(conv(m.erb_pw[i], B.tmp, B.e[i + 1], C, nF, Fo, 1, 1, nullptr, st));
        Fi = Fo;
        if (i == 0) F1 = Fo; else if (i == 1) F2 = Fo; else F3 = Fo;
    }
    EGR_TRY(conv(m.df0, (const float*)B.fspec, B.tmp, C, nF, nb, 1, 0, nullptr, st));
    EGR_TRY(conv(m.df0_pw, B.tmp, B.c0, C, nF, nb, 1, 1, nullptr, st));
    EGR_TRY(conv(m.df1_dw, B.c0, B.tmp, C, nF, nb, 2, 0, nullptr, st, &Fc));
    EGR_TRY(conv(m.df1_pw, B.tmp, B.c1, C, nF, Fc, 1, 1, nullptr, st));
    EGR_CHECK(F3 * ch == m.embd && Fc * ch == ch * nb / 2 && F1 == E / 2 && F2 == E / 4, EGR_ERR_UNSUPPORTED, "egr_dfn2: encoder widths");
    // emb0 = e3 + GroupedLinear(c1) (no activation)
    EGR_TRY(glinear(B.c1, m.fc_emb_w, m.fc_emb_b, B.lin, B.emb0, R, Fc * ch, m.embd, c.lin_groups, c.group_shuffle, 0, B.e[3], st));
    size_t g = 0;
    EGR_TRY(ggru_layer(m.grus[g], B.emb0, B.proj, nullptr, B.gout[g], B.gsum[g], C, nF, st));
    const float* emb = B.gsum[g];
    ++g;
    // ERB decoder (P5)
    const float* xin = emb;
    const float* sum = nullptr;
    for (int k = 0; k < c.emb_num_layers - 1; ++k, ++g) {
        EGR_TRY(ggru_layer(m.grus[g], xin, B.proj, sum, B.gout[g], B.gsum[g], C, nF, st));
        xin = B.gout[g];
        sum = B.gsum[g];
    }
    EGR_TRY(glinear(sum, m.erb_fc_w, m.erb_fc_b, B.lin, B.demb, R, c.emb_hidden_dim, m.embd, c.lin_groups, c.group_shuffle, 1, nullptr, st));
    EGR_TRY(conv(m.path[3], B.e[3], B.pbuf, C, nF, F3, 1, 1, B.demb, st));
    EGR_TRY(conv(m.ct_dw[0], B.pbuf, B.tmp, C, nF, F3, 1, 0, nullptr, st));
    EGR_TRY(conv(m.ct_pw[0], B.tmp, B.dbuf, C, nF, F3, 1, 1, nullptr, st));
    for (int i = 0; i < 2; ++i) {
        const int Fin = i == 0 ? F2 : F1, Fwant = i == 0 ? F1 : E;
        EGR_TRY(conv(m.path[2 - i], B.e[2 - i], B.pbuf, C, nF, Fin, 1, 1, B.dbuf, st));
        int Fo = 0;
        EGR_TRY(conv(m.ct_dw[1 + i], B.pbuf, B.tmp, C, nF, Fin, 2, 0, nullptr, st, &Fo));
        EGR_CHECK(Fo == Fwant, EGR_ERR_UNSUPPORTED, "egr_dfn2: transposed conv width %d != %d", Fo, Fwant);
        EGR_TRY(conv(m.ct_pw[1 + i], B.tmp, B.dbuf, C, nF, Fo, 1, 1, nullptr, st));
    }
    EGR_TRY(conv(m.path[0], B.e[0], B.pbuf, C, nF, E, 1, 1, B.dbuf, st));
    EGR_TRY(conv(m.out0, B.pbuf, B.mask, C, nF, E, 1, 2, nullptr, st));
    // DF decoder (P6)
    xin = emb;
    sum = nullptr;
    for (int k = 0; k < c.df_num_layers; ++k, ++g) {
        EGR_TRY(ggru_layer(m.grus[g], xin, B.proj, sum, B.gout[g], B.gsum[g], C, nF, st));
        xin = B.gout[g];
        sum = B.gsum[g];
    }
    const int Hd = c.df_hidden_dim;
    if (m.df_skip) {
        EGR_TRY(grouped_linear(emb, m.df_skip, B.dfc, R, c.emb_hidden_dim, Hd, c.lin_groups, st));
        EGR_TRY(rows_op(sum, nullptr, B.dfc, B.dfc, R * Hd, Hd, 0, st));            // c = s + skip(emb)
        sum = B.dfc;
    }
    hipLaunchKernelGGL(k_dfn2_alpha, dim3(grid_for(R)), dim3(256), 0, st, sum, m.fc_a_w, m.fc_a_b, R, Hd, B.alpha);
    if (c.df_output_layer == 1)
        EGR_TRY(egr_bgemm(sum, m.df_out, B.tcoef, 1, 1, (int)R, nb * O2, Hd, Hd, Hd, nb * O2, 0, 0, 0, 0, 0, 0, 1, 1.f, st));
    else
        EGR_TRY(grouped_linear(sum, m.df_out, B.tcoef, R, Hd, nb * O2, c.lin_groups, st));
    EGR_TRY(conv(m.convp, B.c0, B.cpt, C, nF, nb, 1, 0, nullptr, st));
    EGR_TRY(conv(m.convp_pw, B.cpt, B.cp, C, nF, nb, 1, 1, nullptr, st));
    EGR_TRY(rows_op(B.tcoef, m.df_out_b, B.cp, B.coefs, R * nb * O2, nb * O2, 3, st));     // tanh(df_out(c)) + df_convp(c0)
    // mask, then deep filter (P7), synthesis
    hipLaunchKernelGGL(k_dfn2_assemble, dim3(grid_for(R * m.Fq)), dim3(256), 0, st, B.spec, B.mask, B.coefs, B.alpha, m.band_of, C, nF,
                       m.Fq, E, nb, c.df_order, c.df_lookahead, B.spec_e);
    hipLaunchKernelGGL(k_dfn_synth, dim3(nF, C), dim3(256), (size_t)(m.Fq + N) * 16, st, B.spec_e, nF, N, m.tw, m.win, B.frames);
    hipLaunchKernelGGL(k_dfn_ola, dim3(grid_for((int64_t)C * T)), dim3(256), 0, st, B.frames, C, nF, N, hop, T, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

}  // namespace
}  // namespace egr

using egr::Dfn2;

extern "C" int egr_dfn2_create(void** handle, const egr_dfn2_config* cfg, const float* packed, int64_t n_floats, int device) {
    using namespace egr;
    EGR_CHECK(handle && cfg && packed && n_floats > 0, EGR_ERR_ARG, "egr_dfn2_create: null argument");
    EGR_CHECK(cfg->struct_bytes == (int)sizeof(egr_dfn2_config), EGR_ERR_ARG, "egr_dfn2_create: struct_bytes %d != %d",
              cfg->struct_bytes, (int)sizeof(egr_dfn2_config));
    const egr_dfn2_config& c = *cfg;
    const int ch = c.conv_ch, E = c.nb_erb, nb = c.nb_df, O2 = 2 * c.df_order, G = c.gru_groups, Gl = c.lin_groups;
    const int ngru = 1 + (c.emb_num_layers - 1) + c.df_num_layers;
    const int embd = ch * E / 4, He = c.emb_hidden_dim, Hd = c.df_hidden_dim;
    EGR_CHECK(c.fft_size > 0 && c.hop_size > 0 && c.fft_size % c.hop_size == 0 && c.fft_size % 2 == 0 && c.fft_size <= 4096, EGR_ERR_UNSUPPORTED,
              "egr_dfn2: fft_size %d / hop_size %d", c.fft_size, c.hop_size);
    EGR_CHECK(E > 0 && E <= EGR_DFN3_MAX_ERB && E % 4 == 0 && nb > 0 && nb % 2 == 0 && nb <= c.fft_size / 2 + 1, EGR_ERR_UNSUPPORTED,
              "egr_dfn2: nb_erb %d / nb_df %d", E, nb);
    EGR_CHECK(He > 0 && He <= GRU_HMAX && Hd > 0 && Hd <= GRU_HMAX, EGR_ERR_UNSUPPORTED, "egr_dfn2: GRU widths must be <= %d", GRU_HMAX);
    EGR_CHECK(c.emb_num_layers >= 2 && c.df_num_layers >= 1 && ngru <= EGR_DFN3_MAX_GRU, EGR_ERR_UNSUPPORTED, "egr_dfn2: GRU layer counts");
    EGR_CHECK(c.df_order >= 1 && c.df_lookahead >= 0 && c.df_lookahead < c.df_order && c.conv_lookahead >= 0 &&
              (c.conv_lookahead == 0 || c.conv_lookahead >= c.df_lookahead), EGR_ERR_UNSUPPORTED, "egr_dfn2: df_order / lookaheads");
    EGR_CHECK(ch > 0 && c.path_groups > 0 && ch % c.path_groups == 0 && c.df_path_groups > 0 && ch % c.df_path_groups == 0 &&
              O2 % c.df_path_groups == 0, EGR_ERR_UNSUPPORTED, "egr_dfn2: conv groups");
    EGR_CHECK(G > 0 && embd % G == 0 && He % G == 0 && Hd % G == 0, EGR_ERR_UNSUPPORTED, "egr_dfn2: gru_groups %d", G);
    EGR_CHECK(Gl > 0 && (ch * nb / 2) % Gl == 0 && embd % Gl == 0 && He % Gl == 0 && (!c.df_gru_skip || Hd % Gl == 0) &&
              (c.df_output_layer == 1 || (Hd % Gl == 0 && (nb * O2) % Gl == 0)), EGR_ERR_UNSUPPORTED, "egr_dfn2: lin_groups %d", Gl);
    EGR_CHECK((c.df_gru_skip == 0 || c.df_gru_skip == 1) && (c.df_output_layer == 0 || c.df_output_layer == 1) &&
              (c.group_shuffle == 0 || c.group_shuffle == 1), EGR_ERR_UNSUPPORTED, "egr_dfn2: df_gru_skip / df_output_layer / group_shuffle");
    EGR_CHECK(c.kf % 2 == 1 && c.kf_inp % 2 == 1 && c.kt >= 1 && c.kt_inp >= 1 && c.df_pathway_kt >= 1, EGR_ERR_UNSUPPORTED,
              "egr_dfn2: frequency kernels must be odd (same-size padding)");
    int wsum = 0;
    for (int e = 0; e < E; ++e) { EGR_CHECK(c.erb_widths[e] > 0, EGR_ERR_ARG, "egr_dfn2: ERB width %d", e); wsum += c.erb_widths[e]; }
    EGR_CHECK(wsum == c.fft_size / 2 + 1, EGR_ERR_ARG, "egr_dfn2: ERB widths sum %d != %d", wsum, c.fft_size / 2 + 1);

    Dfn2* m = new Dfn2();
    m->cfg = c;
    m->device = device;
    m->Fq = c.fft_size / 2 + 1;
    m->embd = embd;
    // packed order: dfn2_weights.pack_order
    int64_t pos = 0;
    auto W = [&](int64_t k) { pos += k; return pos - k; };
    struct ConvSpec { Conv* L; int64_t w, s, t; };
    std::vector<ConvSpec> convs;
    auto cv = [&](Conv& L, int cin, int cout, int groups, int kt, int kf, int transposed = 0) {
        L.cin = cin; L.cout = cout; L.groups = groups; L.kt = kt; L.kf = kf; L.transposed = transposed;
        ConvSpec s{&L, W((int64_t)(transposed ? cin * (cout / groups) : cout * (cin / groups)) * kt * kf), -1, -1};
        convs.push_back(s);
    };
    auto bn = [&](int n) { ConvSpec& s = convs.back(); s.s = W(n); s.t = W(n); };
    cv(m->erb0, 1, ch, 1, c.kt_inp, c.kf_inp); bn(ch);
    for (int i = 0; i < 3; ++i) { cv(m->erb_dw[i], ch, ch, ch, c.kt, c.kf); cv(m->erb_pw[i], ch, ch, 1, 1, 1); bn(ch); }
    cv(m->df0, 2, ch, 2, c.kt_inp, c.kf_inp); cv(m->df0_pw, ch, ch, 1, 1, 1); bn(ch);
    cv(m->df1_dw, ch, ch, ch, c.kt, c.kf); cv(m->df1_pw, ch, ch, 1, 1, 1); bn(ch);
    const int64_t o_fcw = W((int64_t)(ch * nb / 2) * embd / Gl), o_fcb = W(embd);
    struct GruSpec { int64_t wih, whh, bih, bhh; int in, H; int shuffle; };
    std::vector<GruSpec> gs;
    auto ggru = [&](int in0, int H, int layers) {
        for (int l = 0; l < layers; ++l) {
            GruSpec s;
            s.in = l == 0 ? in0 : H; s.H = H;
            s.shuffle = c.group_shuffle && G > 1 && l < layers - 1;
            s.wih = W((int64_t)3 * H * s.in / G); s.whh = W((int64_t)3 * H * H / G); s.bih = W(3 * H); s.bhh = W(3 * H);
            gs.push_back(s);
        }
    };
    ggru(embd, He, 1);
    ggru(He, He, c.emb_num_layers - 1);
    const int64_t o_erbw = W((int64_t)He * embd / Gl), o_erbb = W(embd);
    for (int i = 0; i < 3; ++i) {
        cv(m->path[3 - i], ch, ch, c.path_groups, 1, 1); bn(ch);
        if (i == 0) cv(m->ct_dw[0], ch, ch, ch, c.kt, c.kf);
        else cv(m->ct_dw[i], ch, ch, ch, 1, 3, 1);                  // SPEC DFN2-P9: the transposed convs are (1, 3)
        cv(m->ct_pw[i], ch, ch, 1, 1, 1); bn(ch);
    }
    cv(m->path[0], ch, ch, c.path_groups, 1, 1); bn(ch);
    cv(m->out0, ch, 1, 1, c.kt, c.kf); bn(1);
    ggru(He, Hd, c.df_num_layers);
    const int64_t o_skip = c.df_gru_skip ? W((int64_t)He * Hd / Gl) : -1;
    const int64_t o_out = W(c.df_output_layer == 1 ? (int64_t)nb * O2 * Hd : (int64_t)Hd * nb * O2 / Gl);
    const int64_t o_outb = c.df_output_layer == 1 ? W(nb * O2) : -1;
    const int64_t o_aw = W(Hd), o_ab = W(1);
    cv(m->convp, ch, O2, c.df_path_groups, c.df_pathway_kt, 1);
    cv(m->convp_pw, O2, O2, 1, 1, 1); bn(O2);
    if (pos != n_floats) {
        set_error("egr_dfn2_create: packed weights hold %lld floats, the config needs %lld", (long long)n_floats, (long long)pos);
        delete m;
        return EGR_ERR_ARG;
    }
    // device image: packed weights | repacked W_hh per layer | twiddles (double2) | window | band tables
    std::vector<int64_t> o_pk(gs.size());
    int64_t o_cur = (n_floats + 63) & ~63LL;
    for (size_t l = 0; l < gs.size(); ++l) {
        o_pk[l] = o_cur;
        const int h = gs[l].H / G;
        int K = 0, S = 1;
        if (h <= G2_HMAX) ggru_shape(h, &K, &S);
        o_cur += h > G2_HMAX ? (int64_t)GRU_PER_THREAD * GRU_THREADS : (int64_t)G * 3 * K * h * S;
        o_cur = (o_cur + 63) & ~63LL;
    }
    const int N = c.fft_size;
    const int64_t o_tw = o_cur;
    const int64_t o_win = o_tw + 4LL * N;
    const int64_t o_tab = o_win + N;
    const int64_t total = o_tab + 2 * E + m->Fq;
    std::vector<float> img((size_t)total, 0.f);
    memcpy(img.data(), packed, sizeof(float) * n_floats);
    for (size_t l = 0; l < gs.size(); ++l) {
        const int H = gs[l].H, h = H / G;
        const float* w = packed + gs[l].whh;                    // [G][3h][h]
        float* dst = img.data() + o_pk[l];
        if (h > G2_HMAX) {                                      // G = 1: k_dfn_gru's thread-minor (element, thread) order
            for (int t = 0; t < GRU_THREADS; ++t)
                for (int e = 0; e < GRU_PER_THREAD; ++e) {
                    const int j = e / GRU_K, k = e % GRU_K;
                    const int q = j * GRU_THREADS + t, row = q / GRU_SEG, col = GRU_SEG * k + q % GRU_SEG;
                    dst[(int64_t)e * GRU_THREADS + t] = (row < 3 * H && col < H) ? w[(int64_t)row * H + col] : 0.f;
                }
            continue;
        }
        int K, S;
        ggru_shape(h, &K, &S);
        const int NT = h * S;
        for (int g = 0; g < G; ++g)
            for (int t = 0; t < NT; ++t)
                for (int e = 0; e < 3 * K; ++e) {
                    const int j = t / S, s = t % S, q = e / K, col = s + S * (e % K);
                    dst[((int64_t)g * 3 * K + e) * NT + t] = col < h ? w[((int64_t)g * 3 * h + q * h + j) * h + col] : 0.f;
                }
    }
    double* twd = (double*)(img.data() + o_tw);
    for (int n = 0; n < N; ++n) {
        twd[2 * n] = cos(2.0 * M_PI * n / N);
        twd[2 * n + 1] = sin(2.0 * M_PI * n / N);
    }
    const int hN = N / 2;
    for (int n = 0; n < N; ++n) {
        const double s = sin(0.5 * M_PI * (n + 0.5) / hN);
        img[o_win + n] = (float)sin(0.5 * M_PI * s * s);
    }
    int* tab = (int*)(img.data() + o_tab);
    int lo = 0;
    for (int e = 0; e < E; ++e) {
        tab[e] = lo;
        tab[E + e] = c.erb_widths[e];
        for (int j = 0; j < c.erb_widths[e]; ++j) tab[2 * E + lo + j] = e;
        lo += c.erb_widths[e];
    }
    m->wnorm = 1.f / ((float)N * (float)N / (float)(2 * c.hop_size));
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess ||
        hipMalloc(&m->dev_w, sizeof(float) * total) != hipSuccess ||
        hipMemcpy(m->dev_w, img.data(), sizeof(float) * total, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("egr_dfn2_create: device allocation / upload failed on device %d", device);
        if (m->dev_w) (void)hipFree(m->dev_w);
        (void)hipSetDevice(prev);
        delete m;
        return EGR_ERR_HIP;
    }
    // the analysis / synthesis kernels are DeepFilterNet3's: the same process-wide dynamic-LDS cap (egr_dfn3_create)
    const size_t lds_an = (size_t)N * 24, lds_syn = (size_t)(m->Fq + N) * 16;
    hipError_t ea = hipSuccess;
    if (lds_an > (size_t)DFN_LDS_MAX || lds_syn > (size_t)DFN_LDS_MAX) {
        set_error("egr_dfn2_create: fft_size %d needs %zu / %zu bytes of LDS (limit %d)", N, lds_an, lds_syn, DFN_LDS_MAX);
        ea = hipErrorInvalidValue;
    }
    if (ea == hipSuccess) ea = hipFuncSetAttribute((const void*)k_dfn_analysis, hipFuncAttributeMaxDynamicSharedMemorySize, DFN_LDS_MAX);
    if (ea == hipSuccess) ea = hipFuncSetAttribute((const void*)k_dfn_synth, hipFuncAttributeMaxDynamicSharedMemorySize, DFN_LDS_MAX);
    if (ea != hipSuccess) {
        if (lds_an <= (size_t)DFN_LDS_MAX && lds_syn <= (size_t)DFN_LDS_MAX)
            set_error("egr_dfn2_create: hipFuncSetAttribute(MaxDynamicSharedMemorySize) -> %s", hipGetErrorString(ea));
        (void)hipFree(m->dev_w);
        (void)hipSetDevice(prev);
        delete m;
        return EGR_ERR_HIP;
    }
    (void)hipSetDevice(prev);
    float* D = m->dev_w;
    for (auto& s : convs) {
        s.L->w = D + s.w;
        if (s.s >= 0) { s.L->scale = D + s.s; s.L->shift = D + s.t; }
    }
    m->fc_emb_w = D + o_fcw; m->fc_emb_b = D + o_fcb;
    m->erb_fc_w = D + o_erbw; m->erb_fc_b = D + o_erbb;
    m->df_skip = o_skip >= 0 ? D + o_skip : nullptr;
    m->df_out = D + o_out; m->df_out_b = o_outb >= 0 ? D + o_outb : nullptr;
    m->fc_a_w = D + o_aw; m->fc_a_b = D + o_ab;
    for (size_t l = 0; l < gs.size(); ++l) {
        GGru L;
        L.in = gs[l].in; L.H = gs[l].H; L.G = G; L.h = L.H / G; L.shuffle = gs[l].shuffle;
        if (!L.dense()) ggru_shape(L.h, &L.K, &L.S);
        L.wih = D + gs[l].wih; L.bih = D + gs[l].bih; L.bhh = D + gs[l].bhh; L.whh_pk = D + o_pk[l];
        m->grus.push_back(L);
    }
    m->tw = (const double2*)(D + o_tw);
    m->win = D + o_win;
    m->band_lo = (const int*)(D + o_tab);
    m->band_w = (const int*)(D + o_tab) + E;
    m->band_of = (const int*)(D + o_tab) + 2 * E;
    *handle = m;
    return EGR_OK;
}

extern "C" size_t egr_dfn2_workspace_bytes(void* handle, int channels, int64_t n) {
    if (!handle || channels < 1 || n < 1) return 0;
    Dfn2* m = (Dfn2*)handle;
    return egr::layout2(*m, channels, (int)((n + m->cfg.fft_size) / m->cfg.hop_size), nullptr, nullptr);
}

extern "C" int egr_dfn2_enhance(void* handle, const float* x48, int channels, int64_t n, float* y, void* stream) {
    using namespace egr;
    EGR_CHECK(handle && x48 && y && channels >= 1 && channels <= 65535 && n >= 1, EGR_ERR_ARG, "egr_dfn2_enhance: bad argument");
    Dfn2* m = (Dfn2*)handle;
    EGR_CHECK((n + m->cfg.fft_size) / m->cfg.hop_size <= 65535LL * 4096, EGR_ERR_UNSUPPORTED, "egr_dfn2_enhance: input too long");
    EGR_CHECK((n + m->cfg.fft_size) / m->cfg.hop_size <= 2147483647LL / 4096, EGR_ERR_UNSUPPORTED, "egr_dfn2_enhance: input too long");
    int cur = -1;
    EGR_HIP(hipGetDevice(&cur));
    EGR_CHECK(cur == m->device, EGR_ERR_ARG, "egr_dfn2_enhance: handle belongs to device %d, current device is %d", m->device, cur);
    return run2(*m, x48, channels, n, y, (hipStream_t)stream);
}

extern "C" int egr_dfn2_stage(void* handle, int stage, float* dst, int64_t capacity, int64_t* count, void* stream) {
    using namespace egr;
    EGR_CHECK(handle && count, EGR_ERR_ARG, "egr_dfn2_stage: null argument");
    Dfn2* m = (Dfn2*)handle;
    EGR_CHECK(m->ws, EGR_ERR_ARG, "egr_dfn2_stage: no enhance call yet");
    const int64_t R = (int64_t)m->lastC * m->lastF;
    const egr_dfn2_config& c = m->cfg;
    const Dfn2::Bufs& B = m->B;
    const float* src = nullptr;
    int64_t n = 0;
    const int ng = (int)m->grus.size();
    switch (stage) {
        case EGR_DFN3_STAGE_SPEC: src = (const float*)B.spec; n = R * m->Fq * 2; break;
        case EGR_DFN3_STAGE_FEAT_ERB: src = B.ferb; n = R * c.nb_erb; break;
        case EGR_DFN3_STAGE_FEAT_SPEC: src = (const float*)B.fspec; n = R * c.nb_df * 2; break;
        case EGR_DFN3_STAGE_E0: src = B.e[0]; n = R * c.nb_erb * c.conv_ch; break;
        case EGR_DFN3_STAGE_E1: src = B.e[1]; n = R * (c.nb_erb / 2) * c.conv_ch; break;
        case EGR_DFN3_STAGE_E2: src = B.e[2]; n = R * (c.nb_erb / 4) * c.conv_ch; break;
        case EGR_DFN3_STAGE_E3: src = B.e[3]; n = R * (c.nb_erb / 4) * c.conv_ch; break;
        case EGR_DFN3_STAGE_C0: src = B.c0; n = R * c.nb_df * c.conv_ch; break;
        case EGR_DFN3_STAGE_EMB: src = B.gsum[0]; n = R * c.emb_hidden_dim; break;
        case EGR_DFN3_STAGE_MASK: src = B.mask; n = R * c.nb_erb; break;
        case EGR_DFN3_STAGE_COEFS: src = B.coefs; n = R * c.nb_df * 2 * c.df_order; break;
        case EGR_DFN3_STAGE_SPEC_E: src = (const float*)B.spec_e; n = R * m->Fq * 2; break;
        case EGR_DFN2_STAGE_ALPHA: src = B.alpha; n = R; break;
        default:
            if (stage >= EGR_DFN2_STAGE_GRU0 && stage < EGR_DFN2_STAGE_GRU0 + ng) {
                const int g = stage - EGR_DFN2_STAGE_GRU0;
                src = B.gout[g];
                n = R * m->grus[g].H;
            } else if (stage >= EGR_DFN2_STAGE_SUM0 && stage < EGR_DFN2_STAGE_SUM0 + ng) {
                const int g = stage - EGR_DFN2_STAGE_SUM0;
                src = B.gsum[g];
                n = R * m->grus[g].H;
            }
    }
    EGR_CHECK(src, EGR_ERR_ARG, "egr_dfn2_stage: unknown stage %d", stage);
    *count = n;
    if (!dst) return EGR_OK;
    EGR_CHECK(capacity >= n, EGR_ERR_ARG, "egr_dfn2_stage: capacity %lld < %lld", (long long)capacity, (long long)n);
    EGR_HIP(hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return EGR_OK;
}

extern "C" int egr_dfn2_time_gru(void* handle, int layer, int channels, int64_t steps, double* us_per_step) {
    using namespace egr;
    EGR_CHECK(handle && us_per_step && channels >= 1 && channels <= 64 && steps >= 1 && steps <= 10000000, EGR_ERR_ARG,
              "egr_dfn2_time_gru: bad argument");
    Dfn2* m = (Dfn2*)handle;
    EGR_CHECK(layer >= 0 && layer < (int)m->grus.size(), EGR_ERR_ARG, "egr_dfn2_time_gru: layer %d", layer);
    const GGru& g = m->grus[layer];
    float *proj = nullptr, *out = nullptr, *sum = nullptr;
    hipEvent_t e0, e1;
    EGR_HIP(hipMalloc(&proj, sizeof(float) * channels * steps * 3 * g.H));
    EGR_HIP(hipMalloc(&out, sizeof(float) * channels * steps * g.H));
    EGR_HIP(hipMalloc(&sum, sizeof(float) * channels * steps * g.H));
    EGR_HIP(hipMemset(proj, 0, sizeof(float) * channels * steps * 3 * g.H));
    EGR_HIP(hipEventCreate(&e0));
    EGR_HIP(hipEventCreate(&e1));
    const int warm = (int)(steps < 64 ? steps : 64);
    for (int rep = 0; rep < 2; ++rep) {                    // a short warm-up launch, then the timed one
        const int nF = rep == 0 ? warm : (int)steps;
        if (rep == 1) EGR_HIP(hipEventRecord(e0, 0));
        if (g.dense())
            hipLaunchKernelGGL(k_dfn_gru, dim3(channels), dim3(GRU_THREADS), 0, 0, proj, g.whh_pk, g.bhh, g.H, nF, out);
        else
            launch_ggru(g, proj, nullptr, out, sum, channels, nF, 0);
    }
    EGR_HIP(hipEventRecord(e1, 0));
    EGR_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    EGR_HIP(hipEventElapsedTime(&ms, e0, e1));
    *us_per_step = 1e3 * ms / (double)steps;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(proj);
    (void)hipFree(out);
    (void)hipFree(sum);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_dfn2_destroy(void* handle) {
    if (!handle) return EGR_OK;
    Dfn2* m = (Dfn2*)handle;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(m->device);
    if (m->ws) {
        (void)hipFreeAsync(m->ws, nullptr);
        (void)hipDeviceSynchronize();
    }
    if (m->dev_w) (void)hipFree(m->dev_w);
    (void)hipSetDevice(prev);
    delete m;
    return EGR_OK;
}
