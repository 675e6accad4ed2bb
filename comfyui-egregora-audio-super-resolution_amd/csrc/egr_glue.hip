// Host-glue arithmetic of the reference moved onto the device: PCM_16 round trip, chunk slice/pad,
// Hann WOLA stitch (as a deterministic gather) and the STFT-magnitude used by the LSD yardstick.
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "egr_common.h"
#include "egr_eval_index.h"
#include "egr_fft_device.h"
#include "egr_handle.h"
#include "egr_null_index.h"
#include "egr_plan.h"
#include "egr_stft_tables.h"

namespace egr {

__global__ __launch_bounds__(256) void k_pcm16(const float* __restrict__ x, float* __restrict__ y, long long n,
                                                float ws, float rd) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        long long q = (long long)rintf(__fmul_rn(x[i], ws));
        q = ((q + 32768) & 65535) - 32768;
        y[i] = __fdiv_rn((float)q, rd);
    }
}

// ---------------------------------------------------------------- chunk slice, WOLA and polyphase resampling: per-sample bodies
// The arithmetic of one output sample is stated once here; the single-clip kernels (k_chunk_gather, k_wola, k_resample_poly) and
// the many-track kernels (k_*_tracks) below only differ in how a thread finds its sample.
__device__ __forceinline__ float chunk_sample(const float* __restrict__ xc, long long total, long long start, long long j) {
    const long long i = start + j;
    return (i < total) ? xc[i] : 0.f;
}

// pr: row of chunk 0 of this channel; consecutive chunks of the channel lie row_stride rows of lp floats apart
__device__ __forceinline__ float wola_sample(const float* __restrict__ pr, long long row_stride, long long nchunks, long long lp,
                                             long long total, long long win, long long hop, const float* __restrict__ window,
                                             long long i) {
    long long k_lo = (i < win) ? 0 : (i - win) / hop + 1;
    long long k_hi = i / hop;
    if (k_hi > nchunks - 1) k_hi = nchunks - 1;
    float acc = 0.f, ws = 0.f;
    for (long long k = k_lo; k <= k_hi; ++k) {
        const long long start = k * hop;
        long long L = total - start;
        if (L > win) L = win;
        if (L > lp) L = lp;
        const long long j = i - start;
        if (j < L) {
            const float w = window[j];
            const float y = pr[(size_t)k * row_stride * lp + j];
            acc = __fadd_rn(acc, __fmul_rn(y, w));
            ws = __fadd_rn(ws, w);
        }
    }
    if (ws == 0.f) ws = 1.f;
    return __fdiv_rn(acc, ws);
}

// Rational-rate polyphase FIR, same definition and float32 accumulation order as scipy.signal.resample_poly
// (upfirdn with zero extension): y[m] = sum_k h[m*down - k*up + half] * x[k], k ascending, unfused mul/add.
__device__ __forceinline__ float resample_sample(const float* __restrict__ xc, long long n_in, int up, int down,
                                                 const float* __restrict__ h, int half, long long m) {
    const long long hl = 2LL * half;
    const long long t = m * down + half;
    long long k_hi = t / up;
    if (k_hi > n_in - 1) k_hi = n_in - 1;
    long long k_lo = t - hl <= 0 ? 0 : (t - hl + up - 1) / up;
    float acc = 0.f;
    for (long long k = k_lo; k <= k_hi; ++k) acc = __fadd_rn(acc, __fmul_rn(xc[k], h[t - k * up]));
    return acc;
}

__global__ __launch_bounds__(256) void k_chunk_gather(const float* __restrict__ x, int C, long long total,
                                                       long long win, long long hop, int chunk_begin,
                                                       float* __restrict__ chunks) {
    const int k = blockIdx.y / C, c = blockIdx.y % C;
    const long long start = (long long)(chunk_begin + k) * hop;
    const float* xc = x + (size_t)c * total;
    float* dst = chunks + ((size_t)k * C + c) * win;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < win;
         j += (long long)gridDim.x * blockDim.x)
        dst[j] = chunk_sample(xc, total, start, j);
}

__global__ __launch_bounds__(256) void k_wola(const float* __restrict__ preds, int nchunks, int C, long long lp,
                                               long long total, long long win, long long hop,
                                               const float* __restrict__ window, float* __restrict__ out) {
    const int c = blockIdx.y;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x)
        out[(size_t)c * total + i] = wola_sample(preds + (size_t)c * lp, C, nchunks, lp, total, win, hop, window, i);
}

__global__ __launch_bounds__(256) void k_resample_poly(const float* __restrict__ x, long long n_in, long long n_out,
                                                        int up, int down, const float* __restrict__ h, int half,
                                                        float* __restrict__ y) {
    const int c = blockIdx.y;
    const float* xc = x + (size_t)c * n_in;
    float* yc = y + (size_t)c * n_out;
    for (long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x; m < n_out;
         m += (long long)gridDim.x * blockDim.x)
        yc[m] = resample_sample(xc, n_in, up, down, h, half, m);
}

// ---------------------------------------------------------------- many tracks per launch (a track = one channel of one clip)
// Work mapping: a FLAT index over the samples the launch writes -- a launch's size is the sum of its tracks' lengths, whatever the
// longest one is, and no grid dimension counts tracks or rows.  A workgroup's 256 consecutive samples mostly belong to one track:
// the group searches the table's ascending output offsets once for its first sample (the same value in every lane), each thread
// then steps forward over the few track starts inside the group's stretch.
// (track_of, the search, is in egr_ragged_index.h: host and device share it)

// rows[r] = (track offset into x, track length, chunk index k); chunks [n_rows][win]
__global__ __launch_bounds__(256) void k_chunk_gather_tracks(const float* __restrict__ x, const long long* __restrict__ rows,
                                                              long long n_rows, long long win, long long hop,
                                                              float* __restrict__ chunks) {
    const long long n = n_rows * win;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long r = i / win, j = i - r * win;
        const long long* e = rows + r * 3;
        chunks[i] = chunk_sample(x + e[0], e[1], e[2] * hop, j);
    }
}

// tracks[t] = (first row, row stride, n_chunks, total, out offset); out offsets ascend back to back from 0 to total_out
__global__ __launch_bounds__(256) void k_wola_tracks(const float* __restrict__ preds, const long long* __restrict__ tracks,
                                                      int n_tracks, long long total_out, long long lp, long long win,
                                                      long long hop, const float* __restrict__ window, float* __restrict__ out) {
    for (long long base = (long long)blockIdx.x * 256; base < total_out; base += (long long)gridDim.x * 256) {
        int t = track_of(tracks, n_tracks, 5, 4, base);
        const long long i = base + threadIdx.x;
        if (i >= total_out) continue;
        while (t + 1 < n_tracks && tracks[(size_t)(t + 1) * 5 + 4] <= i) ++t;
        const long long* e = tracks + (size_t)t * 5;
        const long long m = i - e[4];
        if (m < e[3]) out[i] = wola_sample(preds + (size_t)e[0] * lp, e[1], e[2], lp, e[3], win, hop, window, m);
    }
}

// tracks[t] = (in offset, n_in, out offset, n_out); out offsets ascend back to back from 0 to total_out
__global__ __launch_bounds__(256) void k_resample_poly_tracks(const float* __restrict__ x, const long long* __restrict__ tracks,
                                                               int n_tracks, long long total_out, int up, int down,
                                                               const float* __restrict__ h, int half, float* __restrict__ y) {
    for (long long base = (long long)blockIdx.x * 256; base < total_out; base += (long long)gridDim.x * 256) {
        int t = track_of(tracks, n_tracks, 4, 2, base);
        const long long i = base + threadIdx.x;
        if (i >= total_out) continue;
        while (t + 1 < n_tracks && tracks[(size_t)(t + 1) * 4 + 2] <= i) ++t;
        const long long* e = tracks + (size_t)t * 4;
        const long long m = i - e[2];
        if (m < e[3]) y[i] = resample_sample(x + e[0], e[1], up, down, h, half, m);
    }
}

// One frame of the STFT magnitude, by one workgroup of 256: mono downmix (rows ld apart), window, half-length complex FFT in LDS; the
// transform is left in cur (lds_fft may have swapped cur and alt).  k_stft_mag and k_pair_frames (egr_metrics_pairs) both call it.
__device__ __forceinline__ void stft_frame_fft(const float* __restrict__ x, int C, long long ld, long long n, long long s0, int Mh,
                                               const float* __restrict__ window, const FftDesc& fd, const cplx* __restrict__ tw,
                                               cplx*& cur, cplx*& alt) {
    const float invC = (float)C;
    for (int e = threadIdx.x; e < Mh; e += blockDim.x) {
        float v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long long t = s0 + 2 * e + h;
            float m = 0.f;
            if (t < n) {
                m = x[t];
                if (C > 1) {
                    for (int c = 1; c < C; ++c) m = __fadd_rn(m, x[(size_t)c * ld + t]);
                    m = __fdiv_rn(m, invC);
                }
            }
            v[h] = __fmul_rn(m, window[2 * e + h]);
        }
        cur[e] = make_float2(v[0], v[1]);
    }
    __syncthreads();
    lds_fft<false>(cur, alt, fd, tw, 1, 0, 1, Mh, false);
}

// real split of the half-length transform in cur, |X[k]| for k in [0, Mh]
__device__ __forceinline__ float stft_bin_mag(const cplx* cur, int Mh, const cplx* __restrict__ wsplit, int k) {
    const cplx Za = cur[k == Mh ? 0 : k];
    const cplx Zb = cur[(k == 0 || k == Mh) ? 0 : Mh - k];
    const cplx E = make_float2(0.5f * (Za.x + Zb.x), 0.5f * (Za.y - Zb.y));
    const cplx O = make_float2(0.5f * (Za.y + Zb.y), -0.5f * (Za.x - Zb.x));
    const cplx X = cadd(E, cmul(wsplit[k], O));
    return sqrtf(X.x * X.x + X.y * X.y);
}

// One workgroup per frame: mono downmix, window, half-length complex FFT in LDS, real split, |X|.
__global__ __launch_bounds__(256) void k_stft_mag(const float* __restrict__ x, int C, long long n, int n_fft, int hop,
                                                   const float* __restrict__ window, FftDesc fd,
                                                   const cplx* __restrict__ tw, const cplx* __restrict__ wsplit,
                                                   float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Mh = n_fft / 2;
    cplx* cur = (cplx*)smem;
    cplx* alt = cur + Mh;
    const long long f = blockIdx.x;
    stft_frame_fft(x, C, n, n, f * hop, Mh, window, fd, tw, cur, alt);
    float* o = out + (size_t)f * (Mh + 1);
    for (int k = threadIdx.x; k <= Mh; k += blockDim.x) o[k] = stft_bin_mag(cur, Mh, wsplit, k);
}

static std::mutex g_stft_mu;
static std::map<std::pair<int, int>, StftTables> g_stft;   // (device, n_fft)

int stft_tables(int n_fft, StftTables* out) {
    int dev = 0;
    EGR_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_stft_mu);
    auto it = g_stft.find({dev, n_fft});
    if (it != g_stft.end()) { *out = it->second; return EGR_OK; }
    StftTables t;
    const int Mh = n_fft / 2;
    EGR_CHECK(make_schedule(Mh, &t.fd, 127), EGR_ERR_UNSUPPORTED, "n_fft=%d: n_fft/2 has a prime factor above 127", n_fft);
    std::vector<float2> h;
    make_twiddles(h, Mh, 1, Mh);
    EGR_HIP(hipMalloc((void**)&t.tw, h.size() * sizeof(float2)));
    EGR_HIP(hipMemcpy(t.tw, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice));
    make_twiddles(h, Mh + 1, 1, n_fft);
    EGR_HIP(hipMalloc((void**)&t.wsplit, h.size() * sizeof(float2)));
    EGR_HIP(hipMemcpy(t.wsplit, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice));
    g_stft[{dev, n_fft}] = t;
    *out = t;
    return EGR_OK;
}

// ---------------------------------------------------------------- evaluation metrics (egregora_audio_eval_pack.py:405-429)
// per[f] = sqrt(mean_k (20 log10(A[f][k] + eps) - 20 log10(B[f][k] + eps))^2 + 1e-12), float32 terms like the reference,
// the bin sum in double.  One workgroup per frame.
__device__ __forceinline__ double lsd_bin_term(float a, float b) {
    const float la = 20.0f * log10f(a + 1e-12f), lb = 20.0f * log10f(b + 1e-12f);
    const float d = la - lb;
    return (double)(d * d);
}

__global__ __launch_bounds__(256) void k_lsd_frames(const float* __restrict__ SA, const float* __restrict__ SB, int nb,
                                                     float* __restrict__ per) {
    __shared__ double red[256];
    const size_t f = blockIdx.x;
    const float* a = SA + f * nb;
    const float* b = SB + f * nb;
    double acc = 0.0;
    for (int k = threadIdx.x; k < nb; k += 256) {
        acc += lsd_bin_term(a[k], b[k]);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) per[f] = sqrtf((float)(red[0] / nb) + 1e-12f);
}

__global__ __launch_bounds__(256) void k_sum_f64(const float* __restrict__ v, long long n, double* __restrict__ out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) acc += (double)v[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(out, red[0]);
}

// k-th smallest (0-based) of v[0..n) for two ranks, by 4-pass radix selection on order-preserving keys.  ONE workgroup.
__device__ __forceinline__ unsigned f2key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// the selection, by one workgroup of 1024 threads; k_order_stats2 and k_pair_lsd_reduce (egr_metrics_pairs) both call it
__device__ __forceinline__ void order_stats2_block(const float* __restrict__ v, long long n, long long k0, long long k1,
                                                   float* __restrict__ out2) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix;
    __shared__ long long s_k;
    for (int which = 0; which < 2; ++which) {
        if (threadIdx.x == 0) { s_prefix = 0u; s_k = which ? k1 : k0; }
        __syncthreads();
        for (int pass = 3; pass >= 0; --pass) {
            if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
            __syncthreads();
            const unsigned prefix = s_prefix;
            const unsigned himask = pass == 3 ? 0u : (0xffffffffu << (8 * (pass + 1)));
            for (long long i = threadIdx.x; i < n; i += 1024) {
                const unsigned key = f2key(v[i]);
                if ((key & himask) == (prefix & himask)) atomicAdd(&hist[(key >> (8 * pass)) & 255u], 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                long long k = s_k;
                int bkt = 0;
                for (; bkt < 255; ++bkt) {
                    if (k < (long long)hist[bkt]) break;
                    k -= hist[bkt];
                }
                s_k = k;
                s_prefix = prefix | ((unsigned)bkt << (8 * pass));
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) out2[which] = key2f(s_prefix);
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void k_order_stats2(const float* __restrict__ v, long long n, long long k0, long long k1,
                                                        float* __restrict__ out2) {
    order_stats2_block(v, n, k0, k1, out2);
}

// SI-SDR terms on the mono downmixes (mean over channels in float32, like the reference's .mean(axis=0); sums in double):
//   mode 0: out[0] += <s_hat, s>, out[1] += <s, s>
//   mode 1: alpha = out[0] / (out[1] + 1e-20); out[2] += |alpha s|^2, out[3] += |s_hat - alpha s|^2
__global__ __launch_bounds__(256) void k_sisdr(const float* __restrict__ s, int cs, long long stride_s,
                                                const float* __restrict__ sh, int csh, long long stride_sh, long long n,
                                                int mode, double* __restrict__ out) {
    __shared__ double r0[256], r1[256];
    const double alpha = mode ? out[0] / (out[1] + 1e-20) : 0.0;
    double a0 = 0.0, a1 = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float ms = 0.f, mh = 0.f;
        for (int c = 0; c < cs; ++c) ms += s[c * stride_s + i];
        for (int c = 0; c < csh; ++c) mh += sh[c * stride_sh + i];
        const double x = (double)(ms / (float)cs), y = (double)(mh / (float)csh);
        if (mode == 0) {
            a0 += y * x;
            a1 += x * x;
        } else {
            const double t = alpha * x, e = y - t;
            a0 += t * t;
            a1 += e * e;
        }
    }
    r0[threadIdx.x] = a0;
    r1[threadIdx.x] = a1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { r0[threadIdx.x] += r0[threadIdx.x + o]; r1[threadIdx.x] += r1[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicAdd(out + 2 * mode, r0[0]);
        atomicAdd(out + 2 * mode + 1, r1[0]);
    }
}

// np.interp(linspace(0,1,n_out,False), linspace(0,1,n_in,False), x) per row (Resample Audio (HQ) "linear" mode,
// egregora_audio_eval_pack.py:515-519): position j*n_in/n_out in input samples, clamped to the last sample, double math.
__global__ __launch_bounds__(256) void k_resample_linear(const float* __restrict__ x, long long n_in, long long n_out,
                                                          float* __restrict__ y) {
    const float* xr = x + (size_t)blockIdx.y * n_in;
    float* yr = y + (size_t)blockIdx.y * n_out;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n_out; j += (long long)gridDim.x * 256) {
        const double t = (double)j / (double)n_out;              // linspace(0, 1, n_out, endpoint=False)[j]
        long long i = (long long)(t * (double)n_in);
        if ((double)i / (double)n_in > t) --i;                    // largest i with t_old[i] <= t
        if (i >= n_in - 1) { yr[j] = xr[n_in - 1]; continue; }
        const double t0 = (double)i / (double)n_in, t1 = (double)(i + 1) / (double)n_in;
        const double y0 = xr[i], y1 = xr[i + 1];
        yr[j] = (float)(y0 + (t - t0) * ((y1 - y0) / (t1 - t0)));
    }
}

// ---------------------------------------------------------------- DeepFilterNet stage glue (egregora_audio_enhance_extras.py:548-704)
// rms[c][f] = sqrt(mean(x[c][480 f .. 480 f + 480)^2)) (last frame short), one wave per frame, sum in double.
__global__ __launch_bounds__(64) void k_frame_rms(const float* __restrict__ x, long long T, long long n_frames,
                                                   float* __restrict__ rms) {
    const long long f = blockIdx.x;
    const float* xc = x + (size_t)blockIdx.y * T;
    const long long a = f * 480, b = a + 480 < T ? a + 480 : T;
    double acc = 0.0;
    for (long long i = a + threadIdx.x; i < b; i += 64) acc += (double)xc[i] * (double)xc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (threadIdx.x == 0) rms[(size_t)blockIdx.y * n_frames + f] = (float)sqrt(acc / (double)(b - a));
}

// Per channel (one thread: the smoothing is a recurrence): probs = clip(rms / p95, 0, 1); one-pole smoothing; adaptive strength;
// wet/dry gains.  Every step rounds to float32 exactly where numpy does (no fused multiply-adds), see oracle/dfn_mix.py.
struct DfnP {
    float alpha, oma;      // exp(-10 ms / tau) and 1 - alpha (both already rounded to float32); smooth = 0: no smoothing
    int smooth, mode;      // mode 0 off, 1 more_on_noise, 2 more_on_speech, 3 gate_on_noise
    float s0, a, one_m_s0, thr, s_noise, s_speech;
    int linear;            // 0: equal power (sin / cos of pi/2 * s), 1: linear
    double pos_frac;       // fractional part of 0.95 * (n - 1): numpy's linear percentile between the two order statistics
};
__global__ void k_dfn_gains(const float* __restrict__ rms, const float* __restrict__ ostat2, long long n, DfnP q,
                            float* __restrict__ g_dry, float* __restrict__ g_wet) {
    if (threadIdx.x != 0) return;
    const int c = blockIdx.x;
    const float* r = rms + (size_t)c * n;
    const double lo = ostat2[2 * c], hi = ostat2[2 * c + 1], t = q.pos_frac;
    // numpy _lerp: a + (b - a) t, or b - (b - a)(1 - t) for t >= 0.5 (float32 order statistics, float64 arithmetic)
    double p95 = t >= 0.5 ? hi - (hi - lo) * (1.0 - t) : lo + (hi - lo) * t;
    p95 = (double)(float)p95;                       // np.percentile of a float32 array returns float32
    if (p95 == 0.0) p95 = 1e-6;
    const float p95f = (float)p95;
    float acc = 0.f;
    for (long long i = 0; i < n; ++i) {
        float v = __fdiv_rn(r[i], p95f);
        v = fminf(fmaxf(v, 0.f), 1.f);
        if (q.smooth) {
            if (i == 0) acc = v;
            acc = __fadd_rn(__fmul_rn(q.alpha, acc), __fmul_rn(q.oma, v));
            v = fminf(fmaxf(acc, 0.f), 1.f);
        }
        float s;
        if (q.mode == 1) s = __fadd_rn(q.s0, __fmul_rn(__fmul_rn(q.a, __fsub_rn(1.0f, v)), q.one_m_s0));
        else if (q.mode == 2) s = __fadd_rn(q.s0, __fmul_rn(__fmul_rn(q.a, v), q.one_m_s0));
        else if (q.mode == 3) s = v < q.thr ? q.s_noise : q.s_speech;
        else s = q.s0;
        s = fminf(fmaxf(s, 0.f), 1.f);
        float gd, gw;
        if (q.linear) { gw = s; gd = __fsub_rn(1.0f, s); }
        else {
            const float ang = __fmul_rn(1.57079637f, s);       // float32(0.5 * pi) * s
            gw = sinf(ang);
            gd = cosf(ang);
        }
        g_dry[(size_t)c * n + i] = gd;
        g_wet[(size_t)c * n + i] = gw;
    }
}

// y = clip(g_dry[f] * dry + g_wet[f] * wet, -1, 1) * gain, frame f = i / hop (the last gain repeats); running max |y|
__global__ __launch_bounds__(256) void k_dfn_mix(const float* __restrict__ dry, const float* __restrict__ wet,
                                                  const float* __restrict__ g_dry, const float* __restrict__ g_wet, long long T,
                                                  long long n, int hop, float gain, int use_gain, float* __restrict__ y,
                                                  unsigned* __restrict__ peak) {
    __shared__ float red[4];
    const size_t co = (size_t)blockIdx.y * T, go = (size_t)blockIdx.y * n;
    float mx = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < T; i += (long long)gridDim.x * 256) {
        long long f = i / hop;
        if (f > n - 1) f = n - 1;
        float v = __fadd_rn(__fmul_rn(g_dry[go + f], dry[co + i]), __fmul_rn(g_wet[go + f], wet[co + i]));
        v = fminf(fmaxf(v, -1.f), 1.f);
        if (use_gain) v = __fmul_rn(v, gain);
        y[co + i] = v;
        mx = fmaxf(mx, fabsf(v));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(peak, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// limiter: if (limit && peak > ceiling && peak > 0) y *= float32(ceiling / peak); then clamp to [-1, 1]
__global__ __launch_bounds__(256) void k_dfn_limit(float* __restrict__ y, long long n, const unsigned* __restrict__ peak,
                                                    int limit, double ceiling) {
    const float pk = __uint_as_float(*peak);
    const bool scale = limit && (double)pk > ceiling && pk > 0.f;
    const float sc = scale ? (float)(ceiling / (double)pk) : 1.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float v = y[i];
        if (scale) v = __fmul_rn(v, sc);
        y[i] = fminf(fmaxf(v, -1.f), 1.f);
    }
}

// Delay compensation of the null-test suite (_apply_frac_delay_CN + _pad_or_crop_CN, egregora_null_test_suite.py:203-266):
// s[i] = x[i - shift] inside [0, n_in) else 0; y[i] = sum_k h[k] s[i + (taps-1)/2 - k]  (np.convolve(s, h, "same"); taps = 0:
// y = s); output length n_out (zero beyond n_in).  float32 products summed in order of k.
__global__ __launch_bounds__(256) void k_shift_fir(const float* __restrict__ x, long long n_in, long long shift,
                                                    const float* __restrict__ h, int taps, long long n_out,
                                                    float* __restrict__ y) {
    const float* xr = x + (size_t)blockIdx.y * n_in;
    float* yr = y + (size_t)blockIdx.y * n_out;
    const int off = (taps - 1) / 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_out; i += (long long)gridDim.x * 256) {
        float acc = 0.f;
        if (i < n_in) {
            if (taps <= 0) {
                const long long j = i - shift;
                acc = (j >= 0 && j < n_in) ? xr[j] : 0.f;
            } else {
                for (int k = 0; k < taps; ++k) {
                    const long long si = i + off - k;          // index into the shifted signal
                    const long long j = si - shift;
                    if (si >= 0 && si < n_in && j >= 0 && j < n_in) acc += h[k] * xr[j];
                }
            }
        }
        yr[i] = acc;
    }
}

// ---------------------------------------------------------------- null-test suite levels and sums (egregora_null_test_suite.py:119-165, 420-470)
// K-weighting approximation of the suite's loudness: z = (1-k) x + k z, y = x - z (each product and sum rounded to float32 as numpy's
// scalar loop does), then y[n] += 0.02 (y[n] - y[n-1]).  The recurrence contracts by k per sample, so a thread restarts it W samples
// ahead of its L-sample chunk (k^W < 1e-11: below float32 resolution of the state).
__global__ __launch_bounds__(64) void k_kweight(const float* __restrict__ x, long long n, float a1, float kf, int L, int W,
                                                float* __restrict__ y) {
    const long long s = ((long long)blockIdx.x * 64 + threadIdx.x) * L;
    if (s >= n) return;
    const float* xc = x + (size_t)blockIdx.y * n;
    float* yc = y + (size_t)blockIdx.y * n;
    long long i = s - W - 1;
    if (i < 0) i = 0;
    float z = 0.f, yp = 0.f;
    for (; i < s; ++i) {
        const float xv = xc[i];
        z = __fadd_rn(__fmul_rn(a1, xv), __fmul_rn(kf, z));
        yp = __fsub_rn(xv, z);
    }
    const long long e = s + L < n ? s + L : n;
    for (; i < e; ++i) {
        const float xv = xc[i];
        z = __fadd_rn(__fmul_rn(a1, xv), __fmul_rn(kf, z));
        const float yv = __fsub_rn(xv, z);
        yc[i] = i > 0 ? __fadd_rn(yv, __fmul_rn(0.02f, __fsub_rn(yv, yp))) : yv;
        yp = yv;
    }
}

// (mono_mean, the float32 mean over channels, lives in egr_null_index.h: egr_fatllama.hip forms the same downmix)
__global__ __launch_bounds__(256) void k_mono_mean(const float* __restrict__ x, int C, long long ld, long long n, float* __restrict__ y) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) y[i] = mono_mean(x, C, ld, i);
}

// out[f] = mean(mono[f hop .. f hop + blk)^2) in double (the block is cut at n), one workgroup per block
// block f of one signal, by one workgroup of 256; thread 0 stores.  k_frame_meansq and k_frame_meansq_tracks both call it.
__device__ __forceinline__ void frame_meansq_block(const float* __restrict__ x, int C, long long n, long long blk, long long hop,
                                                   long long f, double* __restrict__ dst) {
    __shared__ double red[256];
    const long long a = f * hop, b = a + blk < n ? a + blk : n;
    double acc = 0.0;
    for (long long i = a + threadIdx.x; i < b; i += 256) {
        const double m = (double)mono_mean(x, C, n, i);
        acc += m * m;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *dst = red[0] / (double)(b - a);
}

__global__ __launch_bounds__(256) void k_frame_meansq(const float* __restrict__ x, int C, long long n, long long blk, long long hop,
                                                      double* __restrict__ out) {
    frame_meansq_block(x, C, n, blk, hop, (long long)blockIdx.x, out + blockIdx.x);
}

// the blocks of every clip's K-weighted mono (one channel), one workgroup per (clip, block) found in prefix column `col`; out is flat
__global__ __launch_bounds__(256) void k_frame_meansq_tracks(const float* __restrict__ mono, const long long* __restrict__ tab, int n_clips,
                                                             int col, long long blk, long long hop, double* __restrict__ out) {
    long long f;
    const long long* e = tab + (size_t)loud_item_of(tab, n_clips, col, (long long)blockIdx.x, &f) * LT_COLS;
    frame_meansq_block(mono + e[LT_MONO], 1, e[LT_N], blk, hop, f, out + blockIdx.x);
}

// ---------------------------------------------------------------- evaluation pack loudness meter (egregora_audio_eval_pack.py:132-214)
// K-weighting of every channel and the channel mean in one pass: mono[i] = mean_c kweight(x[c])[i].  Per channel the arithmetic is
// k_kweight's (same roundings, same order, same restart W samples ahead of the thread's L-sample chunk), the mean is mono_mean's
// (rows added in order, one division).  CT > 0: CT channels advance together with their states in registers (x read once, mono
// written once).  CT = 0: any channel count, one channel after the other, the running sum kept in the thread's own stretch of mono.
// One thread's L-sample chunk starting at s < n; k_kweight_mono and k_kweight_mono_tracks (egr_loudness_tracks) both call it.
template <int CT>
__device__ __forceinline__ void kweight_mono_chunk(const float* __restrict__ x, int C, long long n, float a1, float kf, long long s, int L,
                                                   int W, float* __restrict__ mono) {
    long long i0 = s - W - 1;
    if (i0 < 0) i0 = 0;
    const long long e = s + L < n ? s + L : n;
    if constexpr (CT > 0) {
        float z[CT > 0 ? CT : 1], yp[CT > 0 ? CT : 1];
#pragma unroll
        for (int c = 0; c < CT; ++c) z[c] = yp[c] = 0.f;
        long long i = i0;
        for (; i < s; ++i) {
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const float xv = x[(size_t)c * n + i];
                z[c] = __fadd_rn(__fmul_rn(a1, xv), __fmul_rn(kf, z[c]));
                yp[c] = __fsub_rn(xv, z[c]);
            }
        }
        for (; i < e; ++i) {
            float m = 0.f;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const float xv = x[(size_t)c * n + i];
                z[c] = __fadd_rn(__fmul_rn(a1, xv), __fmul_rn(kf, z[c]));
                const float yv = __fsub_rn(xv, z[c]);
                const float v = i > 0 ? __fadd_rn(yv, __fmul_rn(0.02f, __fsub_rn(yv, yp[c]))) : yv;
                yp[c] = yv;
                m = c ? __fadd_rn(m, v) : v;
            }
            mono[i] = CT > 1 ? __fdiv_rn(m, (float)CT) : m;
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const float* xc = x + (size_t)c * n;
            float z = 0.f, yp = 0.f;
            long long i = i0;
            for (; i < s; ++i) {
                const float xv = xc[i];
                z = __fadd_rn(__fmul_rn(a1, xv), __fmul_rn(kf, z));
                yp = __fsub_rn(xv, z);
            }
            for (; i < e; ++i) {
                const float xv = xc[i];
                z = __fadd_rn(__fmul_rn(a1, xv), __fmul_rn(kf, z));
                const float yv = __fsub_rn(xv, z);
                const float v = i > 0 ? __fadd_rn(yv, __fmul_rn(0.02f, __fsub_rn(yv, yp))) : yv;
                yp = yv;
                float m = c ? __fadd_rn(mono[i], v) : v;
                if (c == C - 1 && C > 1) m = __fdiv_rn(m, (float)C);
                mono[i] = m;
            }
        }
    }
}

template <int CT>
__global__ __launch_bounds__(64) void k_kweight_mono(const float* __restrict__ x, int C, long long n, float a1, float kf, int L, int W,
                                                     float* __restrict__ mono) {
    const long long s = ((long long)blockIdx.x * 64 + threadIdx.x) * L;
    if (s >= n) return;
    kweight_mono_chunk<CT>(x, C, n, a1, kf, s, L, W, mono);
}

// tab: LT_COLS int64 per clip (egr_eval_index.h).  Flat thread index over every clip's chunks: a wave's 64 chunks may belong to
// several clips, each thread looks its own up.
template <int CT>
__global__ __launch_bounds__(64) void k_kweight_mono_tracks(const float* __restrict__ x, const long long* __restrict__ tab, int n_clips,
                                                            long long total_chunks, int C, float a1, float kf, int L, int W,
                                                            float* __restrict__ mono) {
    const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
    if (g >= total_chunks) return;
    long long j;
    const long long* e = tab + (size_t)loud_item_of(tab, n_clips, LT_CHUNK0, g, &j) * LT_COLS;
    kweight_mono_chunk<CT>(x + e[LT_OFF], C, e[LT_N], a1, kf, j * L, L, W, mono + e[LT_MONO]);
}

// *slot (bits of a non-negative float, zeroed by the call) raised to max_m |y[m]|, y = resample_poly(mono_mean(x), up, 1) with
// k_resample_poly's per-output accumulation (down = 1) on the channel mean formed on the fly; the up * n samples are never stored.
// up = 1: y is the channel mean itself (scipy returns a copy, no filter).
// sample m of the oversampled channel mean; k_true_peak and k_true_peak_tracks both call it
__device__ __forceinline__ float true_peak_sample(const float* __restrict__ x, int C, long long n, int up, const float* __restrict__ h,
                                                  int half, long long m) {
    if (up == 1) return mono_mean(x, C, n, m);
    const long long hl = 2LL * half;
    const long long t = m + half;
    long long k_hi = t / up;
    if (k_hi > n - 1) k_hi = n - 1;
    const long long k_lo = t - hl <= 0 ? 0 : (t - hl + up - 1) / up;
    float acc = 0.f;
    for (long long k = k_lo; k <= k_hi; ++k) acc = __fadd_rn(acc, __fmul_rn(mono_mean(x, C, n, k), h[t - k * up]));
    return acc;
}

// the workgroup's maximum (256 threads) raises *slot; an integer maximum of non-negative float bits: any order gives the same value
__device__ __forceinline__ void true_peak_commit(float mx, unsigned* __restrict__ slot) {
    __shared__ float red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(slot, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

__global__ __launch_bounds__(256) void k_true_peak(const float* __restrict__ x, int C, long long n, int up, const float* __restrict__ h,
                                                   int half, unsigned* __restrict__ slot) {
    const long long n_out = n * up;
    float mx = 0.f;
    for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < n_out; m += (long long)gridDim.x * 256)
        mx = fmaxf(mx, fabsf(true_peak_sample(x, C, n, up, h, half, m)));
    true_peak_commit(mx, slot);
}

// one workgroup per 256-sample tile of one clip's oversampled signal; slots[clip] as k_true_peak's slot
__global__ __launch_bounds__(256) void k_true_peak_tracks(const float* __restrict__ x, const long long* __restrict__ tab, int n_clips, int C,
                                                          int up, const float* __restrict__ h, int half, unsigned* __restrict__ slots) {
    long long tile;
    const int c = loud_item_of(tab, n_clips, LT_TILE0, (long long)blockIdx.x, &tile);
    const long long* e = tab + (size_t)c * LT_COLS;
    const long long m = tile * LT_TILE + threadIdx.x;
    float mx = 0.f;
    if (m < e[LT_N] * up) mx = fmaxf(mx, fabsf(true_peak_sample(x + e[LT_OFF], C, e[LT_N], up, h, half, m)));
    true_peak_commit(mx, slots + c);
}

template <int K>
__device__ __forceinline__ void block_add_f64(double (&v)[K], double* __restrict__ out) {
    __shared__ double red[K][4];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x < K) atomicAdd(out + threadIdx.x, red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// sums over the mono downmixes a_m, b_m (b optionally scaled by kf in float32 first): out += {sum a, sum b, sum ab, sum aa, sum bb}
__global__ __launch_bounds__(256) void k_pair_stats(const float* __restrict__ a, int ca, long long lda, const float* __restrict__ b,
                                                    int cb, long long ldb, long long n, float kf, int use_k, double* __restrict__ out) {
    double v[5] = {0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double x = (double)mono_mean(a, ca, lda, i);
        float m = use_k ? __fmul_rn(b[i], kf) : b[i];
        for (int c = 1; c < cb; ++c) m = __fadd_rn(m, use_k ? __fmul_rn(b[(size_t)c * ldb + i], kf) : b[(size_t)c * ldb + i]);
        const double yv = (double)(cb > 1 ? __fdiv_rn(m, (float)cb) : m);
        v[0] += x; v[1] += yv; v[2] += x * yv; v[3] += x * x; v[4] += yv * yv;
    }
    block_add_f64<5>(v, out);
}

// null[c][i] = a[c][i] + sgn * (b[c][i] * kf); out += {sum null_m^2, count(|null| > 1)}
__global__ __launch_bounds__(256) void k_null_mix(const float* __restrict__ a, long long lda, const float* __restrict__ b, long long ldb,
                                                  int C, long long n, float kf, int use_k, float sgn, float* __restrict__ nul,
                                                  double* __restrict__ out) {
    double v[2] = {0, 0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float m = 0.f;
        for (int c = 0; c < C; ++c) {
            float bv = b[(size_t)c * ldb + i];
            if (use_k) bv = __fmul_rn(bv, kf);
            const float d = __fadd_rn(a[(size_t)c * lda + i], sgn * bv);
            nul[(size_t)c * n + i] = d;
            if (fabsf(d) > 1.0f) v[1] += 1.0;
            m = c ? __fadd_rn(m, d) : d;
        }
        if (C > 1) m = __fdiv_rn(m, (float)C);
        v[0] += (double)m * (double)m;
    }
    block_add_f64<2>(v, out);
}

// out += {sum x^2, sum x, sum (-1)^i x, sum y^2, sum y, sum (-1)^i y}: the time-domain side of Parseval for one-sided band energies
__global__ __launch_bounds__(256) void k_band_sums(const float* __restrict__ x, const float* __restrict__ y, long long n,
                                                   double* __restrict__ out) {
    double v[6] = {0, 0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double a = x[i], b = y[i], s = (i & 1) ? -1.0 : 1.0;
        v[0] += a * a; v[1] += a; v[2] += s * a; v[3] += b * b; v[4] += b; v[5] += s * b;
    }
    block_add_f64<6>(v, out);
}

// ---------------------------------------------------------------- many (reference, processed) pairs per call (egr_metrics_pairs)
// tab: MP_COLS int64 per pair (egr_eval_index.h).  Every grid is flat and equals its work count.  No floating-point atomics: a pair's
// eight numbers are sums in a fixed order over that pair's own frames and chunks, whatever else the call holds.
//
// One workgroup per (pair, frame): side A's frame is transformed and its magnitudes kept in registers (at most PF_MAGS per thread,
// n_fft = 8192), then side B's in the same two LDS buffers; per[flat frame] as k_lsd_frames forms it from the two magnitude arrays
// (same bins per thread in the same order, same tree), which here never reach memory.  The tree reuses the transform's LDS.
constexpr int PF_MAGS = (8192 / 2 + 1 + 255) / 256;
__global__ __launch_bounds__(256) void k_pair_frames(const float* __restrict__ a, const float* __restrict__ b, const long long* __restrict__ tab,
                                                     int n_pairs, int n_fft, int hop, const float* __restrict__ window, FftDesc fd,
                                                     const cplx* __restrict__ tw, const cplx* __restrict__ wsplit, float* __restrict__ per) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Mh = n_fft / 2;
    cplx* cur = (cplx*)smem;
    cplx* alt = cur + Mh;
    long long f;
    const long long* e = tab + (size_t)metrics_frame_of(tab, n_pairs, (long long)blockIdx.x, &f) * MP_COLS;
    const long long n = e[MP_N], s0 = f * hop;
    stft_frame_fft(a + e[MP_OFF_A], (int)e[MP_CA], e[MP_LD_A], n, s0, Mh, window, fd, tw, cur, alt);
    float ma[PF_MAGS];
#pragma unroll
    for (int j = 0; j < PF_MAGS; ++j) {
        const int k = threadIdx.x + 256 * j;
        ma[j] = k <= Mh ? stft_bin_mag(cur, Mh, wsplit, k) : 0.f;
    }
    __syncthreads();
    stft_frame_fft(b + e[MP_OFF_B], (int)e[MP_CB], e[MP_LD_B], n, s0, Mh, window, fd, tw, cur, alt);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < PF_MAGS; ++j) {
        const int k = threadIdx.x + 256 * j;
        if (k <= Mh) acc += lsd_bin_term(ma[j], stft_bin_mag(cur, Mh, wsplit, k));
    }
    __syncthreads();
    double* red = (double*)smem;
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) per[blockIdx.x] = sqrtf((float)(red[0] / (Mh + 1)) + 1e-12f);
}

// One workgroup per pair: out8[0] = sum of the pair's per[] in double (thread i takes frames i, i + 1024, ...; a tree), out8[1], out8[2] =
// the order statistics MP_KLO, MP_KHI of per[] (k_order_stats2's selection), out8[3] = frames.
__global__ __launch_bounds__(1024) void k_pair_lsd_reduce(const float* __restrict__ per, const long long* __restrict__ tab,
                                                          double* __restrict__ out8) {
    __shared__ double red[1024];
    __shared__ float o2[2];
    const long long* e = tab + (size_t)blockIdx.x * MP_COLS;
    const float* v = per + e[MP_FRAME0];
    const long long n = e[MP_FRAMES];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n; i += 1024) acc += (double)v[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    order_stats2_block(v, n, e[MP_KLO], e[MP_KHI], o2);
    if (threadIdx.x == 0) {
        double* o = out8 + (size_t)blockIdx.x * 8;
        o[0] = red[0]; o[1] = (double)o2[0]; o[2] = (double)o2[1]; o[3] = (double)n;
    }
}

// One workgroup per chunk of EGR_METRICS_CHUNK samples of one pair (the last chunk of a pair is short; none spans two pairs):
//   MODE 0: part = (<s_hat, s>, <s, s>)       MODE 1: alpha = out8[4] / (out8[5] + 1e-20), part = (|alpha s|^2, |s_hat - alpha s|^2)
// on the mono downmixes (mono_mean), s = side A, s_hat = side B; k_sisdr's terms, summed per chunk.
template <int MODE>
__global__ __launch_bounds__(256) void k_pair_sisdr_part(const float* __restrict__ a, const float* __restrict__ b,
                                                         const long long* __restrict__ tab, int n_pairs, const double* __restrict__ out8,
                                                         double2* __restrict__ part) {
    __shared__ double r0[256], r1[256];
    long long first, len;
    const int p = metrics_chunk_of(tab, n_pairs, (long long)blockIdx.x, &first, &len);
    const long long* e = tab + (size_t)p * MP_COLS;
    const float* s = a + e[MP_OFF_A];
    const float* sh = b + e[MP_OFF_B];
    const int cs = (int)e[MP_CA], csh = (int)e[MP_CB];
    const long long lds = e[MP_LD_A], ldh = e[MP_LD_B];
    const double alpha = MODE ? out8[(size_t)p * 8 + 4] / (out8[(size_t)p * 8 + 5] + 1e-20) : 0.0;
    double a0 = 0.0, a1 = 0.0;
    for (long long i = first + threadIdx.x; i < first + len; i += 256) {
        const double x = (double)mono_mean(s, cs, lds, i), y = (double)mono_mean(sh, csh, ldh, i);
        if (MODE == 0) {
            a0 += y * x;
            a1 += x * x;
        } else {
            const double t = alpha * x, d = y - t;
            a0 += t * t;
            a1 += d * d;
        }
    }
    r0[threadIdx.x] = a0;
    r1[threadIdx.x] = a1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { r0[threadIdx.x] += r0[threadIdx.x + o]; r1[threadIdx.x] += r1[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = make_double2(r0[0], r1[0]);
}

// One workgroup per pair: the pair's chunk sums added in a fixed order (thread i takes chunks i, i + 256, ... ascending; a tree) into
// out8[4 + 2 mode], out8[5 + 2 mode].
__global__ __launch_bounds__(256) void k_pair_sisdr_reduce(const double2* __restrict__ part, const long long* __restrict__ tab, int mode,
                                                           double* __restrict__ out8) {
    __shared__ double r0[256], r1[256];
    const long long* e = tab + (size_t)blockIdx.x * MP_COLS;
    const double2* v = part + e[MP_CHUNK0];
    const long long nc = metrics_chunks(e[MP_N]);
    double a0 = 0.0, a1 = 0.0;
    for (long long i = threadIdx.x; i < nc; i += 256) { a0 += v[i].x; a1 += v[i].y; }
    r0[threadIdx.x] = a0;
    r1[threadIdx.x] = a1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { r0[threadIdx.x] += r0[threadIdx.x + o]; r1[threadIdx.x] += r1[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out8[(size_t)blockIdx.x * 8 + 4 + 2 * mode] = r0[0];
        out8[(size_t)blockIdx.x * 8 + 5 + 2 * mode] = r1[0];
    }
}

// ---------------------------------------------------------------- many pairs through the null test (egr_nullmany_*)
// tab: SF_COLS int64 per (pair, channel) row (egr_null_index.h).  One workgroup per 256-sample output tile of one row; k_shift_fir's
// sums.  The tile's 256 + m - 1 samples of the shifted signal go to LDS once (zero outside [0, n_in) on either index) and the taps
// with them; a zero product added in k_shift_fir's order leaves the accumulator's bits as they are (it starts at +0 and never
// becomes -0), so the result has k_shift_fir's bits.  (A form that read every term from global memory as k_shift_fir does gave the
// same bits 1.5x to 1.85x slower: profiles/null_batch.md.)
__global__ __launch_bounds__(256) void k_shift_fir_rows(const float* __restrict__ x, const long long* __restrict__ tab, int n_rows,
                                                        const float* __restrict__ taps, int m, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    long long first, len;
    const long long* e = tab + (size_t)shiftfir_tile_of(tab, n_rows, (long long)blockIdx.x, &first, &len) * SF_COLS;
    const float* xr = x + e[SF_IN];
    float* yr = y + e[SF_OUT];
    const long long n_in = e[SF_N_IN], shift = e[SF_SHIFT], i = first + threadIdx.x;
    if (e[SF_TAPS] < 0) {          // (the same for the whole workgroup)
        if ((long long)threadIdx.x < len) {
            const long long j = i - shift;
            yr[i] = (i < n_in && j >= 0 && j < n_in) ? xr[j] : 0.f;
        }
        return;
    }
    const float* h = taps + (size_t)e[SF_TAPS] * m;
    const int off = (m - 1) / 2;
    float* S = (float*)smem;
    float* H = S + NULL_TILE + m - 1;
    const long long s0 = first + off - (m - 1);
    for (int q = threadIdx.x; q < NULL_TILE + m - 1; q += 256) {
        const long long si = s0 + q, j = si - shift;
        S[q] = (si >= 0 && si < n_in && j >= 0 && j < n_in) ? xr[j] : 0.f;
    }
    for (int k = threadIdx.x; k < m; k += 256) H[k] = h[k];
    __syncthreads();
    if ((long long)threadIdx.x < len) {
        float acc = 0.f;
        if (i < n_in)
            for (int k = 0; k < m; ++k) acc += H[k] * S[threadIdx.x + m - 1 - k];
        yr[i] = acc;
    }
}

// tab: NM_COLS int64 per pair; prm: {gain g, least-squares k, sign, k in use} per pair.  One workgroup per chunk of NULL_CHUNK samples of
// one pair: matched = fl(aligned g) (egr_eltwise's product), b' = k in use ? fl(matched k) : matched, null = fl(a + sgn b') (k_null_mix);
// part[chunk] = {sum mono(null)^2, count(|null| > 1), sum a, sum b', sum a b', sum a a, sum b' b'} over the mono downmixes in double
// (k_null_mix's and k_pair_stats' terms).  STORE: matched, null and (k in use) b' are written to the pair's [channels][n] blocks.
template <bool STORE>
__global__ __launch_bounds__(256) void k_nullmany_mix(const float* __restrict__ a, const float* __restrict__ b, const long long* __restrict__ tab,
                                                      const float4* __restrict__ prm, int n_pairs, float* __restrict__ matched,
                                                      float* __restrict__ nul, float* __restrict__ scaled, double* __restrict__ part) {
    __shared__ double red[NULL_SUMS - 1][256];
    long long first, len;
    const int p = mix_chunk_of(tab, n_pairs, (long long)blockIdx.x, &first, &len);
    const long long* e = tab + (size_t)p * NM_COLS;
    const float* A = a + e[NM_OFF_A];
    const float* B = b + e[NM_OFF_B];
    const long long lda = e[NM_LD_A], ldb = e[NM_LD_B], n = e[NM_N], o = e[NM_OUT];
    const int C = (int)e[NM_CH];
    const float4 q = prm[p];
    const float g = q.x, kf = q.y, sgn = q.z;
    const bool use_k = q.w != 0.f;
    double v[NULL_SUMS - 1] = {0, 0, 0, 0, 0, 0, 0};
    for (long long i = first + threadIdx.x; i < first + len; i += 256) {
        float mn = 0.f, ma = 0.f, mb = 0.f;
        for (int c = 0; c < C; ++c) {
            const float av = A[(size_t)c * lda + i];
            const float mt = __fmul_rn(B[(size_t)c * ldb + i], g);
            const float bp = use_k ? __fmul_rn(mt, kf) : mt;
            const float d = __fadd_rn(av, sgn * bp);
            if (STORE) {
                const size_t w = (size_t)o + (size_t)c * n + i;
                matched[w] = mt;
                nul[w] = d;
                if (use_k) scaled[w] = bp;
            }
            if (fabsf(d) > 1.0f) v[1] += 1.0;
            mn = c ? __fadd_rn(mn, d) : d;
            ma = c ? __fadd_rn(ma, av) : av;
            mb = c ? __fadd_rn(mb, bp) : bp;
        }
        if (C > 1) { mn = __fdiv_rn(mn, (float)C); ma = __fdiv_rn(ma, (float)C); mb = __fdiv_rn(mb, (float)C); }
        const double dn = mn, x = ma, yv = mb;
        v[0] += dn * dn; v[2] += x; v[3] += yv; v[4] += x * yv; v[5] += x * x; v[6] += yv * yv;
    }
#pragma unroll
    for (int k = 0; k < NULL_SUMS - 1; ++k) red[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < NULL_SUMS - 1; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < NULL_SUMS) part[(size_t)blockIdx.x * NULL_SUMS + threadIdx.x] = threadIdx.x < NULL_SUMS - 1 ? red[threadIdx.x][0] : 0.0;
}

// One workgroup per pair: the pair's chunk sums added in a fixed order (thread i takes chunks i, i + 256, ... ascending; a tree) into
// out8[pair]: k_pair_sisdr_reduce's scheme for the seven sums.
__global__ __launch_bounds__(256) void k_nullmany_reduce(const double* __restrict__ part, const long long* __restrict__ tab,
                                                         double* __restrict__ out8) {
    __shared__ double red[NULL_SUMS - 1][256];
    const long long* e = tab + (size_t)blockIdx.x * NM_COLS;
    const double* v = part + (size_t)e[NM_CHUNK0] * NULL_SUMS;
    const long long nc = mix_chunks(e[NM_N]);
    double acc[NULL_SUMS - 1] = {0, 0, 0, 0, 0, 0, 0};
    for (long long i = threadIdx.x; i < nc; i += 256) {
#pragma unroll
        for (int k = 0; k < NULL_SUMS - 1; ++k) acc[k] += v[(size_t)i * NULL_SUMS + k];
    }
#pragma unroll
    for (int k = 0; k < NULL_SUMS - 1; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < NULL_SUMS - 1; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < NULL_SUMS) out8[(size_t)blockIdx.x * NULL_SUMS + threadIdx.x] = threadIdx.x < NULL_SUMS - 1 ? red[threadIdx.x][0] : 0.0;
}

// The restart rule of the K-weighting kernels, stated once: a thread restarts the recurrence W samples ahead of its L-sample chunk,
// k^W < 6e-12 (below float32 resolution of the state), W at least 64, L = W / 3 rounded up.  egr_kweight, egr_loudness_frames and
// egr_loudness_tracks all take their chunking from here, which is what keeps their results bit-equal.
static inline void kweight_chunking(float k, int* L, int* W) {
    int w = (int)ceil(26.0 / -log((double)k));
    if (w < 64) w = 64;
    *W = w;
    *L = (w + 2) / 3;
}

static inline size_t eval_align(size_t b) { return (b + 255) & ~(size_t)255; }

static const char* eval_why(int r) {
    return r == EVAL_SHORT ? "n < 1" : r == EVAL_BAD_ROW ? "channels outside 1 .. 65535 or a row stride below n"
         : r == EVAL_OFFSET ? "an offset, stride or length is negative or past what the index type holds"
                            : "the running total of frames, chunks, blocks or tiles leaves one grid (workgroups x threads < 2^32)";
}

struct MetricsPlan {
    std::vector<long long> tab;
    long long frames = 0, chunks = 0;
    size_t per_off = 0, part_off = 0, total = 0;
    int launches = 0;
};

// every refusal of egr_metrics_pairs that needs no pointer: host arithmetic only
static int metrics_plan(const int64_t* pairs, int n_pairs, int n_fft, int hop, int flags, MetricsPlan* P) {
    EGR_CHECK(pairs && n_pairs >= 1, EGR_ERR_ARG, "egr_metrics_pairs: no pairs");
    EGR_CHECK(n_pairs <= EVAL_MAX_PAIRS, EGR_ERR_UNSUPPORTED, "egr_metrics_pairs: n_pairs=%d is above %lld, one 1024-thread workgroup per pair",
              n_pairs, EVAL_MAX_PAIRS);
    EGR_CHECK(flags >= 1 && flags <= 3, EGR_ERR_ARG, "egr_metrics_pairs: flags=%d asks for neither LSD (1) nor SI-SDR (2)", flags);
    EGR_CHECK(hop >= 1, EGR_ERR_ARG, "egr_metrics_pairs: hop=%d", hop);
    EGR_CHECK(n_fft >= 2 && (n_fft % 2) == 0 && n_fft <= 8192, EGR_ERR_UNSUPPORTED, "egr_metrics_pairs: n_fft=%d must be even and <= 8192",
              n_fft);
    FftDesc fd;
    EGR_CHECK(make_schedule(n_fft / 2, &fd, 127), EGR_ERR_UNSUPPORTED, "egr_metrics_pairs: n_fft=%d: n_fft/2 has a prime factor above 127",
              n_fft);
    P->tab.assign((size_t)n_pairs * MP_COLS, 0);
    for (int p = 0; p < n_pairs; ++p) {
        const int r = metrics_fill((const long long*)pairs + (size_t)p * MP_IN_COLS, n_fft, hop, &P->frames, &P->chunks,
                                   P->tab.data() + (size_t)p * MP_COLS);
        EGR_CHECK(r == EVAL_OK, r == EVAL_TOTAL ? EGR_ERR_UNSUPPORTED : EGR_ERR_ARG, "egr_metrics_pairs: pair %d: %s", p, eval_why(r));
    }
    P->per_off = eval_align(P->tab.size() * sizeof(long long));
    P->part_off = P->per_off + eval_align((flags & 1) ? (size_t)P->frames * sizeof(float) : 0);
    P->total = P->part_off + eval_align((flags & 2) ? (size_t)P->chunks * sizeof(double2) : 0);
    P->launches = ((flags & 1) ? 2 : 0) + ((flags & 2) ? 4 : 0);
    return EGR_OK;
}

struct LoudPlan {
    std::vector<long long> tab;
    LoudTotals t = {0, 0, 0, 0, 0};
    int L = 0, W = 0;
    size_t mono_off = 0, total = 0;
    int launches = 0;
};

static int loud_plan(const int64_t* clips, int n_clips, int channels, float k, int64_t blk_a, int64_t hop_a, int64_t blk_b, int64_t hop_b,
                     int up, LoudPlan* P) {
    EGR_CHECK(clips && n_clips >= 1, EGR_ERR_ARG, "egr_loudness_tracks: no clips");
    EGR_CHECK(n_clips <= EVAL_MAX_GRID_256, EGR_ERR_UNSUPPORTED, "egr_loudness_tracks: n_clips=%d is above %lld", n_clips, EVAL_MAX_GRID_256);
    EGR_CHECK(channels >= 1 && channels <= 65535 && k > 0.f && k < 1.f, EGR_ERR_ARG, "egr_loudness_tracks: channels=%d, k=%g", channels, k);
    EGR_CHECK(blk_a >= 1 && hop_a >= 1 && blk_b >= 0 && (blk_b == 0 || hop_b >= 1) && up >= 0 && up <= 64, EGR_ERR_ARG,
              "egr_loudness_tracks: bad block family or oversampling factor");
    kweight_chunking(k, &P->L, &P->W);
    P->tab.assign((size_t)n_clips * LT_COLS, 0);
    for (int c = 0; c < n_clips; ++c) {
        const int r = loud_fill((const long long*)clips + (size_t)c * LT_IN_COLS, channels, P->L, blk_a, hop_a, blk_b, hop_b, up, &P->t,
                                P->tab.data() + (size_t)c * LT_COLS);
        EGR_CHECK(r == EVAL_OK, r == EVAL_TOTAL ? EGR_ERR_UNSUPPORTED : EGR_ERR_ARG, "egr_loudness_tracks: clip %d: %s", c, eval_why(r));
    }
    P->mono_off = eval_align(P->tab.size() * sizeof(long long));
    P->total = P->mono_off + eval_align((size_t)P->t.mono * sizeof(float));
    P->launches = 2 + (blk_b ? 1 : 0) + (up ? 1 : 0);
    return EGR_OK;
}

static const char* null_why(int r) {
    return r == NULL_SHORT ? "a length below 1 (an empty side)" : r == NULL_BAD_ROW ? "channels outside 1 .. 65535 or a row stride below n"
         : r == NULL_OFFSET ? "an offset, stride, shift or length is negative or past what the index type holds"
         : r == NULL_CHANNELS ? "operands could not be broadcast together: the two sides differ in channel count"
         : r == NULL_TAPS    ? "its row of the taps table is outside -1 .. n_tap_rows - 1"
                             : "the running total of tiles or chunks leaves one grid (workgroups x threads < 2^32)";
}

struct ShiftFirPlan {
    std::vector<long long> tab;
    long long tiles = 0;
    size_t total = 0;
};

// every refusal of egr_nullmany_shift_fir that needs no pointer: host arithmetic only
static int shiftfir_plan(const int64_t* rows, int n_rows, int n_tap_rows, int taps, ShiftFirPlan* P) {
    EGR_CHECK(rows && n_rows >= 1, EGR_ERR_ARG, "egr_nullmany_shift_fir: no rows");
    EGR_CHECK(n_rows <= EVAL_MAX_GRID_256, EGR_ERR_UNSUPPORTED, "egr_nullmany_shift_fir: n_rows=%d is above %lld", n_rows, EVAL_MAX_GRID_256);
    EGR_CHECK(n_tap_rows >= 0 && taps >= 0 && taps <= NULL_MAX_TAPS && (n_tap_rows == 0 || taps >= 1), EGR_ERR_ARG,
              "egr_nullmany_shift_fir: n_tap_rows=%d, taps=%d (at most %d)", n_tap_rows, taps, NULL_MAX_TAPS);
    P->tab.assign((size_t)n_rows * SF_COLS, 0);
    for (int r = 0; r < n_rows; ++r) {
        const int why = shiftfir_fill((const long long*)rows + (size_t)r * SF_IN_COLS, n_tap_rows, &P->tiles, P->tab.data() + (size_t)r * SF_COLS);
        EGR_CHECK(why == NULL_OK, why == NULL_TOTAL ? EGR_ERR_UNSUPPORTED : EGR_ERR_ARG, "egr_nullmany_shift_fir: row %d: %s", r, null_why(why));
    }
    P->total = eval_align(P->tab.size() * sizeof(long long));
    return EGR_OK;
}

struct MixPlan {
    std::vector<long long> tab;          // the int64 rows, then two int64 per pair holding its four float parameters
    long long chunks = 0;
    size_t prm_off = 0, part_off = 0, total = 0;
};

static int mix_plan(const int64_t* pairs, int n_pairs, MixPlan* P) {
    EGR_CHECK(pairs && n_pairs >= 1, EGR_ERR_ARG, "egr_nullmany_mix: no pairs");
    EGR_CHECK(n_pairs <= EVAL_MAX_GRID_256, EGR_ERR_UNSUPPORTED, "egr_nullmany_mix: n_pairs=%d is above %lld", n_pairs, EVAL_MAX_GRID_256);
    P->prm_off = eval_align((size_t)n_pairs * NM_COLS * sizeof(long long));
    P->tab.assign(P->prm_off / sizeof(long long) + (size_t)n_pairs * 2, 0);
    for (int p = 0; p < n_pairs; ++p) {
        const int why = mix_fill((const long long*)pairs + (size_t)p * NM_IN_COLS, &P->chunks, P->tab.data() + (size_t)p * NM_COLS);
        EGR_CHECK(why == NULL_OK, why == NULL_TOTAL ? EGR_ERR_UNSUPPORTED : EGR_ERR_ARG, "egr_nullmany_mix: pair %d: %s", p, null_why(why));
    }
    P->part_off = eval_align(P->tab.size() * sizeof(long long));
    P->total = P->part_off + eval_align((size_t)P->chunks * NULL_SUMS * sizeof(double));
    return EGR_OK;
}

static inline int grid_for(long long n) {
    long long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace egr

using namespace egr;

extern "C" int egr_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        set_error("hipGetDeviceCount -> %s", hipGetErrorString(e));
        return -EGR_ERR_HIP;
    }
    return n;
}

extern "C" int egr_device_arch(int dev, char* buf, size_t buflen) {
    EGR_CHECK(buf && buflen > 0, EGR_ERR_ARG, "null buffer");
    hipDeviceProp_t prop;
    EGR_HIP(hipGetDeviceProperties(&prop, dev));
    strncpy(buf, prop.gcnArchName, buflen - 1);
    buf[buflen - 1] = 0;
    return EGR_OK;
}

extern "C" int egr_pcm16_roundtrip(const float* x, float* y, int64_t n, float write_scale, float read_div,
                                   void* stream) {
    EGR_CHECK(x && y && n >= 0 && read_div != 0.f, EGR_ERR_ARG, "bad argument");
    if (n == 0) return EGR_OK;
    hipLaunchKernelGGL(k_pcm16, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)n, write_scale,
                       read_div);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_chunk_gather(const float* x, int channels, int64_t total, int64_t win, int64_t hop,
                                int chunk_begin, int n_chunks, float* chunks, void* stream) {
    EGR_CHECK(x && chunks && channels >= 1 && total >= 0 && win >= 1 && hop >= 1 && chunk_begin >= 0 && n_chunks >= 0,
              EGR_ERR_ARG, "bad argument");
    if (n_chunks == 0) return EGR_OK;
    EGR_CHECK((int64_t)n_chunks * channels <= 65535, EGR_ERR_ARG, "too many chunk rows for one launch");
    int gx = grid_for(win);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(k_chunk_gather, dim3(gx, n_chunks * channels), dim3(256), 0, (hipStream_t)stream, x, channels,
                       (long long)total, (long long)win, (long long)hop, chunk_begin, chunks);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_wola_stitch(const float* preds, int n_chunks, int channels, int64_t lp, int64_t total, int64_t win,
                               int64_t hop, const float* window, float* out, void* stream) {
    EGR_CHECK(preds && window && out && n_chunks >= 1 && channels >= 1 && lp >= 1 && total >= 1 && win >= 1 && hop >= 1,
              EGR_ERR_ARG, "bad argument");
    hipLaunchKernelGGL(k_wola, dim3(grid_for(total), channels), dim3(256), 0, (hipStream_t)stream, preds, n_chunks,
                       channels, (long long)lp, (long long)total, (long long)win, (long long)hop, window, out);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_resample_poly(const float* x, int channels, int64_t n_in, int up, int down, const float* h, int half,
                                 float* y, int64_t n_out, void* stream) {
    EGR_CHECK(x && h && y && channels >= 1 && channels <= 65535 && n_in >= 1 && up >= 1 && down >= 1 && half >= 0,
              EGR_ERR_ARG, "bad argument");
    EGR_CHECK(n_out == (n_in * up + down - 1) / down, EGR_ERR_ARG, "n_out must be ceil(n_in*up/down)");
    hipLaunchKernelGGL(k_resample_poly, dim3(grid_for(n_out), channels), dim3(256), 0, (hipStream_t)stream, x,
                       (long long)n_in, (long long)n_out, up, down, h, half, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_chunk_gather_tracks(const float* x, const int64_t* rows, int n_rows, int64_t win, int64_t hop, float* chunks,
                                       void* stream) {
    EGR_CHECK(x && rows && chunks && n_rows >= 0 && win >= 1 && hop >= 1, EGR_ERR_ARG, "bad argument");
    if (n_rows == 0) return EGR_OK;
    hipLaunchKernelGGL(k_chunk_gather_tracks, dim3(grid_for((long long)n_rows * win)), dim3(256), 0, (hipStream_t)stream, x,
                       (const long long*)rows, (long long)n_rows, (long long)win, (long long)hop, chunks);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_wola_tracks(const float* preds, const int64_t* tracks, int n_tracks, int64_t total_out, int64_t lp, int64_t win,
                               int64_t hop, const float* window, float* out, void* stream) {
    EGR_CHECK(preds && tracks && window && out && n_tracks >= 1 && total_out >= 1 && lp >= 1 && win >= 1 && hop >= 1, EGR_ERR_ARG,
              "bad argument");
    hipLaunchKernelGGL(k_wola_tracks, dim3(grid_for(total_out)), dim3(256), 0, (hipStream_t)stream, preds, (const long long*)tracks,
                       n_tracks, (long long)total_out, (long long)lp, (long long)win, (long long)hop, window, out);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_resample_poly_tracks(const float* x, const int64_t* tracks, int n_tracks, int64_t total_out, int up, int down,
                                        const float* h, int half, float* y, void* stream) {
    EGR_CHECK(x && tracks && h && y && n_tracks >= 1 && total_out >= 1 && up >= 1 && down >= 1 && half >= 0, EGR_ERR_ARG,
              "bad argument");
    hipLaunchKernelGGL(k_resample_poly_tracks, dim3(grid_for(total_out)), dim3(256), 0, (hipStream_t)stream, x,
                       (const long long*)tracks, n_tracks, (long long)total_out, up, down, h, half, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_stft_mag(const float* x, int channels, int64_t n, int n_fft, int hop, const float* window,
                            float* out, void* stream) {
    EGR_CHECK(x && window && out && channels >= 1 && n >= 0 && hop >= 1, EGR_ERR_ARG, "bad argument");
    EGR_CHECK(n_fft >= 2 && (n_fft % 2) == 0 && n_fft <= 8192, EGR_ERR_UNSUPPORTED, "n_fft=%d must be even and <= 8192",
              n_fft);
    StftTables t;
    int rc = stft_tables(n_fft, &t);
    if (rc) return rc;
    const int64_t frames = 1 + ((n - n_fft) > 0 ? (n - n_fft) / hop : 0);
    const size_t lds = (size_t)2 * (n_fft / 2) * sizeof(float2);
    hipLaunchKernelGGL(k_stft_mag, dim3((unsigned)frames), dim3(256), lds, (hipStream_t)stream, x, channels,
                       (long long)n, n_fft, hop, window, t.fd, t.tw, t.wsplit, out);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_lsd_frames(const float* SA, const float* SB, int64_t frames, int nb, float* per, void* stream) {
    EGR_CHECK(SA && SB && per && frames >= 1 && frames < (1LL << 31) && nb >= 1, EGR_ERR_ARG, "bad argument");
    hipLaunchKernelGGL(k_lsd_frames, dim3((unsigned)frames), dim3(256), 0, (hipStream_t)stream, SA, SB, nb, per);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_sum_f64(const float* v, int64_t n, double* out, void* stream) {
    EGR_CHECK(v && out && n >= 1, EGR_ERR_ARG, "bad argument");
    EGR_HIP(hipMemsetAsync(out, 0, sizeof(double), (hipStream_t)stream));
    long long nb = (n + 255) / 256;
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(k_sum_f64, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, v, (long long)n, out);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_order_stats2(const float* v, int64_t n, int64_t k_lo, int64_t k_hi, float* out2, void* stream) {
    EGR_CHECK(v && out2 && n >= 1 && k_lo >= 0 && k_lo < n && k_hi >= 0 && k_hi < n, EGR_ERR_ARG, "bad argument");
    hipLaunchKernelGGL(k_order_stats2, dim3(1), dim3(1024), 0, (hipStream_t)stream, v, (long long)n, (long long)k_lo,
                       (long long)k_hi, out2);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_si_sdr_terms(const float* s, int cs, int64_t stride_s, const float* s_hat, int csh, int64_t stride_sh,
                                int64_t n, double* out4, void* stream) {
    EGR_CHECK(s && s_hat && out4 && cs >= 1 && csh >= 1 && n >= 1 && stride_s >= n && stride_sh >= n, EGR_ERR_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    EGR_HIP(hipMemsetAsync(out4, 0, 4 * sizeof(double), st));
    long long nb = (n + 255) / 256;
    if (nb > 1024) nb = 1024;
    for (int mode = 0; mode < 2; ++mode)
        hipLaunchKernelGGL(k_sisdr, dim3((unsigned)nb), dim3(256), 0, st, s, cs, (long long)stride_s, s_hat, csh,
                           (long long)stride_sh, (long long)n, mode, out4);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_resample_linear(const float* x, int channels, int64_t n_in, float* y, int64_t n_out, void* stream) {
    EGR_CHECK(x && y && channels >= 1 && channels <= 65535 && n_in >= 1 && n_out >= 1, EGR_ERR_ARG, "bad argument");
    long long nb = (n_out + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_resample_linear, dim3((unsigned)nb, channels), dim3(256), 0, (hipStream_t)stream, x, (long long)n_in,
                       (long long)n_out, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" size_t egr_dfn_workspace_bytes(int channels, int64_t n48) {
    const int64_t n = (n48 + 479) / 480;
    return (size_t)channels * n * sizeof(float) + (size_t)channels * 2 * sizeof(float) + 64;
}

extern "C" int egr_dfn_vad_gains(const float* dry48, int channels, int64_t n48, double smooth_ms, int mode, double strength,
                                 double amount, double vad_threshold, int linear_curve, void* workspace, float* g_dry,
                                 float* g_wet, void* stream) {
    EGR_CHECK(dry48 && workspace && g_dry && g_wet && channels >= 1 && channels <= 65535 && n48 >= 1, EGR_ERR_ARG, "bad argument");
    EGR_CHECK(mode >= 0 && mode <= 3 && strength >= 0.0 && strength <= 1.0, EGR_ERR_ARG, "bad mode / strength");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (n48 + 479) / 480;
    float* rms = (float*)workspace;
    float* ost = rms + (size_t)channels * n;
    hipLaunchKernelGGL(k_frame_rms, dim3((unsigned)n, channels), dim3(64), 0, st, dry48, (long long)n48, (long long)n, rms);
    const double pos = 0.95 * (double)(n - 1);
    const int64_t lo = (int64_t)pos, hi = lo + 1 < n ? lo + 1 : n - 1;
    for (int c = 0; c < channels; ++c)
        hipLaunchKernelGGL(k_order_stats2, dim3(1), dim3(1024), 0, st, rms + (size_t)c * n, (long long)n, (long long)lo,
                           (long long)hi, ost + 2 * c);
    DfnP q;
    const double s0 = strength, a = amount;          // Python floats in the reference: constants are formed in double
    const double alpha = smooth_ms > 0.0 ? exp(-10.0 / fmax(1e-3, smooth_ms)) : 0.0;
    q.alpha = (float)alpha; q.oma = (float)(1.0 - alpha); q.smooth = smooth_ms > 0.0 ? 1 : 0; q.mode = mode;
    q.s0 = (float)s0; q.a = (float)a; q.one_m_s0 = (float)(1.0 - s0); q.thr = (float)vad_threshold;
    q.s_noise = (float)fmin(fmax(s0 + a * (1.0 - s0), 0.0), 1.0); q.s_speech = (float)fmin(fmax(s0 * (1.0 - a), 0.0), 1.0);
    q.linear = linear_curve ? 1 : 0; q.pos_frac = pos - (double)lo;
    hipLaunchKernelGGL(k_dfn_gains, dim3(channels), dim3(64), 0, st, rms, ost, (long long)n, q, g_dry, g_wet);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_dfn_mix(const float* dry, const float* wet, const float* g_dry, const float* g_wet, int channels, int64_t n,
                           int64_t n_frames, int hop, float post_gain, int use_gain, int limit, double ceiling, float* y,
                           void* peak_ws, void* stream) {
    EGR_CHECK(dry && wet && g_dry && g_wet && y && peak_ws && channels >= 1 && channels <= 65535 && n >= 1 && n_frames >= 1 &&
                  hop >= 1, EGR_ERR_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    EGR_HIP(hipMemsetAsync(peak_ws, 0, sizeof(unsigned), st));
    long long nb = (n + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(k_dfn_mix, dim3((unsigned)nb, channels), dim3(256), 0, st, dry, wet, g_dry, g_wet, (long long)n,
                       (long long)n_frames, hop, post_gain, use_gain, y, (unsigned*)peak_ws);
    const long long tot = (long long)n * channels;
    long long nb2 = (tot + 255) / 256;
    if (nb2 > 4096) nb2 = 4096;
    hipLaunchKernelGGL(k_dfn_limit, dim3((unsigned)nb2), dim3(256), 0, st, y, tot, (const unsigned*)peak_ws, limit, ceiling);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_shift_fir(const float* x, int channels, int64_t n_in, int64_t shift, const float* h, int taps, float* y,
                             int64_t n_out, void* stream) {
    EGR_CHECK(x && y && channels >= 1 && channels <= 65535 && n_in >= 1 && n_out >= 1 && taps >= 0 && (taps == 0 || h),
              EGR_ERR_ARG, "bad argument");
    long long nb = (n_out + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_shift_fir, dim3((unsigned)nb, channels), dim3(256), 0, (hipStream_t)stream, x, (long long)n_in,
                       (long long)shift, h, taps, (long long)n_out, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_kweight(const float* x, int channels, int64_t n, float one_minus_k, float k, float* y, void* stream) {
    EGR_CHECK(x && y && channels >= 1 && channels <= 65535 && n >= 1 && k > 0.f && k < 1.f, EGR_ERR_ARG, "bad argument");
    int L, W;
    kweight_chunking(k, &L, &W);
    const long long chunks = (n + L - 1) / L;
    hipLaunchKernelGGL(k_kweight, dim3((unsigned)((chunks + 63) / 64), channels), dim3(64), 0, (hipStream_t)stream, x, (long long)n,
                       one_minus_k, k, L, W, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_mono_mean(const float* x, int channels, int64_t stride, int64_t n, float* y, void* stream) {
    EGR_CHECK(x && y && channels >= 1 && n >= 1 && stride >= n, EGR_ERR_ARG, "bad argument");
    hipLaunchKernelGGL(k_mono_mean, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, channels, (long long)stride, (long long)n, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_frame_meansq(const float* x, int channels, int64_t n, int64_t block, int64_t hop, int64_t frames, double* out,
                                void* stream) {
    EGR_CHECK(x && out && channels >= 1 && n >= 1 && block >= 1 && hop >= 1 && frames >= 1 && (frames - 1) * hop < n, EGR_ERR_ARG,
              "bad argument");
    hipLaunchKernelGGL(k_frame_meansq, dim3((unsigned)frames), dim3(256), 0, (hipStream_t)stream, x, channels, (long long)n,
                       (long long)block, (long long)hop, out);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_loudness_frames(const float* x, int channels, int64_t n, float one_minus_k, float k, int64_t blk_a, int64_t hop_a,
                                   int64_t frames_a, int64_t blk_b, int64_t hop_b, int64_t frames_b, float* kmono_ws, double* out_a,
                                   double* out_b, void* stream) {
    EGR_CHECK(x && kmono_ws && out_a && channels >= 1 && n >= 1 && k > 0.f && k < 1.f, EGR_ERR_ARG, "bad argument");
    EGR_CHECK(blk_a >= 1 && hop_a >= 1 && frames_a >= 1 && frames_a < (1LL << 31) && (frames_a - 1) * hop_a < n, EGR_ERR_ARG,
              "bad first block family");
    EGR_CHECK(frames_b == 0 || (out_b && blk_b >= 1 && hop_b >= 1 && frames_b >= 1 && frames_b < (1LL << 31) && (frames_b - 1) * hop_b < n),
              EGR_ERR_ARG, "bad second block family");
    hipStream_t st = (hipStream_t)stream;
    int L, W;
    kweight_chunking(k, &L, &W);
    const long long chunks = (n + L - 1) / L;
    const dim3 grid((unsigned)((chunks + 63) / 64));
    const long long nn = (long long)n;
    switch (channels) {
    case 1: hipLaunchKernelGGL(k_kweight_mono<1>, grid, dim3(64), 0, st, x, channels, nn, one_minus_k, k, L, W, kmono_ws); break;
    case 2: hipLaunchKernelGGL(k_kweight_mono<2>, grid, dim3(64), 0, st, x, channels, nn, one_minus_k, k, L, W, kmono_ws); break;
    case 3: hipLaunchKernelGGL(k_kweight_mono<3>, grid, dim3(64), 0, st, x, channels, nn, one_minus_k, k, L, W, kmono_ws); break;
    case 4: hipLaunchKernelGGL(k_kweight_mono<4>, grid, dim3(64), 0, st, x, channels, nn, one_minus_k, k, L, W, kmono_ws); break;
    default: hipLaunchKernelGGL(k_kweight_mono<0>, grid, dim3(64), 0, st, x, channels, nn, one_minus_k, k, L, W, kmono_ws); break;
    }
    hipLaunchKernelGGL(k_frame_meansq, dim3((unsigned)frames_a), dim3(256), 0, st, (const float*)kmono_ws, 1, nn, (long long)blk_a,
                       (long long)hop_a, out_a);
    if (frames_b)
        hipLaunchKernelGGL(k_frame_meansq, dim3((unsigned)frames_b), dim3(256), 0, st, (const float*)kmono_ws, 1, nn, (long long)blk_b,
                           (long long)hop_b, out_b);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_true_peak(const float* x, int channels, int64_t n, int up, const float* h, int half, float* peak_slot, void* stream) {
    EGR_CHECK(x && peak_slot && channels >= 1 && n >= 1 && up >= 1 && half >= 0 && (up == 1 || h), EGR_ERR_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    EGR_HIP(hipMemsetAsync(peak_slot, 0, sizeof(unsigned), st));
    long long nb = ((long long)n * up + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_true_peak, dim3((unsigned)nb), dim3(256), 0, st, x, channels, (long long)n, up, h, half, (unsigned*)peak_slot);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_pair_stats(const float* a, int ca, int64_t stride_a, const float* b, int cb, int64_t stride_b, int64_t n, float k,
                              int use_k, double* out5, void* stream) {
    EGR_CHECK(a && b && out5 && ca >= 1 && cb >= 1 && n >= 1, EGR_ERR_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    EGR_HIP(hipMemsetAsync(out5, 0, 5 * sizeof(double), st));
    hipLaunchKernelGGL(k_pair_stats, dim3(grid_for(n) > 1024 ? 1024 : grid_for(n)), dim3(256), 0, st, a, ca, (long long)stride_a, b, cb,
                       (long long)stride_b, (long long)n, k, use_k, out5);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_null_mix(const float* a, int64_t stride_a, const float* b, int64_t stride_b, int channels, int64_t n, float k,
                            int use_k, int invert_b, float* null_out, double* out2, void* stream) {
    EGR_CHECK(a && b && null_out && out2 && channels >= 1 && n >= 1, EGR_ERR_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    EGR_HIP(hipMemsetAsync(out2, 0, 2 * sizeof(double), st));
    hipLaunchKernelGGL(k_null_mix, dim3(grid_for(n) > 1024 ? 1024 : grid_for(n)), dim3(256), 0, st, a, (long long)stride_a, b,
                       (long long)stride_b, channels, (long long)n, k, use_k, invert_b ? -1.0f : 1.0f, null_out, out2);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_band_sums(const float* x, const float* y, int64_t n, double* out6, void* stream) {
    EGR_CHECK(x && y && out6 && n >= 1, EGR_ERR_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    EGR_HIP(hipMemsetAsync(out6, 0, 6 * sizeof(double), st));
    hipLaunchKernelGGL(k_band_sums, dim3(grid_for(n) > 1024 ? 1024 : grid_for(n)), dim3(256), 0, st, x, y, (long long)n, out6);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" size_t egr_metrics_pairs_workspace_bytes(const int64_t* pairs, int n_pairs, int n_fft, int hop, int flags) {
    MetricsPlan P;
    if (metrics_plan(pairs, n_pairs, n_fft, hop, flags, &P) != EGR_OK) return 0;
    return P.total;
}

extern "C" int egr_metrics_pairs(const float* a, const float* b, const int64_t* pairs, int n_pairs, int n_fft, int hop, int flags,
                                 const float* window, double* out8, float* per_out, void* ws, size_t ws_bytes, int* launches,
                                 void* stream) {
    MetricsPlan P;
    int rc = metrics_plan(pairs, n_pairs, n_fft, hop, flags, &P);
    if (rc) return rc;
    EGR_CHECK(a && b && out8 && ws && ((flags & 1) == 0 || window), EGR_ERR_ARG, "egr_metrics_pairs: null pointer");
    EGR_CHECK(ws_bytes >= P.total, EGR_ERR_ARG, "egr_metrics_pairs: workspace of %zu bytes, %zu needed", ws_bytes, P.total);
    EGR_CHECK(((uintptr_t)ws & 15) == 0 && ((uintptr_t)out8 & 7) == 0, EGR_ERR_ARG,
              "egr_metrics_pairs: the workspace must be 16-byte aligned (int64 table, double2 partial sums), out8 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    const long long* tab = (const long long*)base;
    StftTables t;
    if (flags & 1) {
        rc = stft_tables(n_fft, &t);
        if (rc) return rc;
    }
    rc = upload_table({{P.tab.data(), P.tab.size() * sizeof(long long)}}, base, st);
    if (rc) return rc;
    if (launches) *launches = P.launches;
    if (flags & 1) {
        float* per = per_out ? per_out : (float*)(base + P.per_off);
        size_t lds = (size_t)2 * (n_fft / 2) * sizeof(float2);
        if (lds < 256 * sizeof(double)) lds = 256 * sizeof(double);          // the tree of the bin sums reuses the transform's buffers
        hipLaunchKernelGGL(k_pair_frames, dim3((unsigned)P.frames), dim3(256), lds, st, a, b, tab, n_pairs, n_fft, hop, window, t.fd, t.tw,
                           t.wsplit, per);
        EGR_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_pair_lsd_reduce, dim3((unsigned)n_pairs), dim3(1024), 0, st, (const float*)per, tab, out8);
        EGR_HIP(hipGetLastError());
    }
    if (flags & 2) {
        double2* part = (double2*)(base + P.part_off);
        hipLaunchKernelGGL(k_pair_sisdr_part<0>, dim3((unsigned)P.chunks), dim3(256), 0, st, a, b, tab, n_pairs, (const double*)out8, part);
        EGR_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_pair_sisdr_reduce, dim3((unsigned)n_pairs), dim3(256), 0, st, (const double2*)part, tab, 0, out8);
        EGR_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_pair_sisdr_part<1>, dim3((unsigned)P.chunks), dim3(256), 0, st, a, b, tab, n_pairs, (const double*)out8, part);
        EGR_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_pair_sisdr_reduce, dim3((unsigned)n_pairs), dim3(256), 0, st, (const double2*)part, tab, 1, out8);
    }
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int64_t egr_metrics_pairs_frames(const int64_t* pairs, int n_pairs, int n_fft, int hop) {
    MetricsPlan P;
    if (metrics_plan(pairs, n_pairs, n_fft, hop, 1, &P) != EGR_OK) return 0;
    return P.frames;
}

extern "C" int egr_kweight_chunking(float k, int* chunk, int* restart) {
    EGR_CHECK(chunk && restart && k > 0.f && k < 1.f, EGR_ERR_ARG, "egr_kweight_chunking: k=%g", k);
    kweight_chunking(k, chunk, restart);
    return EGR_OK;
}

extern "C" size_t egr_loudness_tracks_workspace_bytes(const int64_t* clips, int n_clips, int channels, float k, int64_t blk_a, int64_t hop_a,
                                                      int64_t blk_b, int64_t hop_b, int up) {
    LoudPlan P;
    if (loud_plan(clips, n_clips, channels, k, blk_a, hop_a, blk_b, hop_b, up, &P) != EGR_OK) return 0;
    return P.total;
}

extern "C" int egr_loudness_tracks(const float* x, const int64_t* clips, int n_clips, int channels, float one_minus_k, float k, int64_t blk_a,
                                   int64_t hop_a, int64_t blk_b, int64_t hop_b, int up, const float* h, int half, double* out, void* ws,
                                   size_t ws_bytes, int* launches, void* stream) {
    LoudPlan P;
    int rc = loud_plan(clips, n_clips, channels, k, blk_a, hop_a, blk_b, hop_b, up, &P);
    if (rc) return rc;
    EGR_CHECK(x && out && ws && half >= 0 && (up <= 1 || h), EGR_ERR_ARG, "egr_loudness_tracks: null pointer");
    EGR_CHECK(ws_bytes >= P.total, EGR_ERR_ARG, "egr_loudness_tracks: workspace of %zu bytes, %zu needed", ws_bytes, P.total);
    EGR_CHECK(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0, EGR_ERR_ARG,
              "egr_loudness_tracks: the workspace (int64 table) and out (doubles) must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    const long long* tab = (const long long*)base;
    float* mono = (float*)(base + P.mono_off);
    rc = upload_table({{P.tab.data(), P.tab.size() * sizeof(long long)}}, base, st);
    if (rc) return rc;
    if (launches) *launches = P.launches;
    const dim3 grid((unsigned)((P.t.chunks + 63) / 64));
#define EGR_KW_TRACKS(CT) \
    hipLaunchKernelGGL(k_kweight_mono_tracks<CT>, grid, dim3(64), 0, st, x, tab, n_clips, P.t.chunks, channels, one_minus_k, k, P.L, P.W, mono)
    switch (channels) {
    case 1: EGR_KW_TRACKS(1); break;
    case 2: EGR_KW_TRACKS(2); break;
    case 3: EGR_KW_TRACKS(3); break;
    case 4: EGR_KW_TRACKS(4); break;
    default: EGR_KW_TRACKS(0); break;
    }
#undef EGR_KW_TRACKS
    EGR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_frame_meansq_tracks, dim3((unsigned)P.t.fa), dim3(256), 0, st, (const float*)mono, tab, n_clips, (int)LT_FA0,
                       (long long)blk_a, (long long)hop_a, out);
    EGR_HIP(hipGetLastError());
    if (blk_b)
        hipLaunchKernelGGL(k_frame_meansq_tracks, dim3((unsigned)P.t.fb), dim3(256), 0, st, (const float*)mono, tab, n_clips, (int)LT_FB0,
                           (long long)blk_b, (long long)hop_b, out + P.t.fa);
    if (up) {
        unsigned* slots = (unsigned*)(out + P.t.fa + P.t.fb);
        EGR_HIP(hipMemsetAsync(slots, 0, (size_t)n_clips * sizeof(unsigned), st));
        hipLaunchKernelGGL(k_true_peak_tracks, dim3((unsigned)P.t.tiles), dim3(256), 0, st, x, tab, n_clips, channels, up, h, half, slots);
    }
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" size_t egr_nullmany_shift_fir_workspace_bytes(const int64_t* rows, int n_rows, int n_tap_rows, int taps) {
    ShiftFirPlan P;
    if (shiftfir_plan(rows, n_rows, n_tap_rows, taps, &P) != EGR_OK) return 0;
    return P.total;
}

extern "C" int egr_nullmany_shift_fir(const float* x, const int64_t* rows, int n_rows, const float* taps_tab, int n_tap_rows, int taps,
                                      float* y, void* ws, size_t ws_bytes, int* launches, void* stream) {
    ShiftFirPlan P;
    int rc = shiftfir_plan(rows, n_rows, n_tap_rows, taps, &P);
    if (rc) return rc;
    EGR_CHECK(x && y && ws && (n_tap_rows == 0 || taps_tab), EGR_ERR_ARG, "egr_nullmany_shift_fir: null pointer");
    EGR_CHECK(ws_bytes >= P.total, EGR_ERR_ARG, "egr_nullmany_shift_fir: workspace of %zu bytes, %zu needed", ws_bytes, P.total);
    EGR_CHECK(((uintptr_t)ws & 7) == 0, EGR_ERR_ARG, "egr_nullmany_shift_fir: the workspace (int64 table) must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    rc = upload_table({{P.tab.data(), P.tab.size() * sizeof(long long)}}, ws, st);
    if (rc) return rc;
    if (launches) *launches = 1;
    const long long* tab = (const long long*)ws;
    const int m = n_tap_rows ? taps : 0;
    hipLaunchKernelGGL(k_shift_fir_rows, dim3((unsigned)P.tiles), dim3(256), (size_t)(NULL_TILE + 2 * m) * sizeof(float), st, x, tab, n_rows,
                       taps_tab, m, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" size_t egr_nullmany_mix_workspace_bytes(const int64_t* pairs, int n_pairs) {
    MixPlan P;
    if (mix_plan(pairs, n_pairs, &P) != EGR_OK) return 0;
    return P.total;
}

extern "C" int egr_nullmany_mix(const float* a, const float* b, const int64_t* pairs, const float* params, int n_pairs, float* matched,
                                float* null_out, float* scaled, double* out8, void* ws, size_t ws_bytes, int* launches, void* stream) {
    MixPlan P;
    int rc = mix_plan(pairs, n_pairs, &P);
    if (rc) return rc;
    EGR_CHECK(a && b && params && out8 && ws, EGR_ERR_ARG, "egr_nullmany_mix: null pointer");
    const bool store = matched || null_out;
    EGR_CHECK(!store || (matched && null_out), EGR_ERR_ARG, "egr_nullmany_mix: matched and null_out go together (both null: sums only)");
    for (int p = 0; p < n_pairs; ++p) {
        const float* q = params + (size_t)p * 4;
        EGR_CHECK(q[2] == 1.0f || q[2] == -1.0f, EGR_ERR_ARG, "egr_nullmany_mix: pair %d: sign %g is neither 1 nor -1", p, (double)q[2]);
        EGR_CHECK(q[3] == 0.0f || (store && scaled), EGR_ERR_ARG,
                  "egr_nullmany_mix: pair %d: a least-squares factor needs the stored mode and the `scaled` output", p);
    }
    EGR_CHECK(ws_bytes >= P.total, EGR_ERR_ARG, "egr_nullmany_mix: workspace of %zu bytes, %zu needed", ws_bytes, P.total);
    EGR_CHECK(((uintptr_t)ws & 15) == 0 && ((uintptr_t)out8 & 7) == 0, EGR_ERR_ARG,
              "egr_nullmany_mix: the workspace must be 16-byte aligned (int64 table, float4 parameters), out8 8-byte aligned");
    memcpy(P.tab.data() + P.prm_off / sizeof(long long), params, (size_t)n_pairs * 4 * sizeof(float));
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    rc = upload_table({{P.tab.data(), P.tab.size() * sizeof(long long)}}, base, st);
    if (rc) return rc;
    if (launches) *launches = 2;
    const long long* tab = (const long long*)base;
    const float4* prm = (const float4*)(base + P.prm_off);
    double* part = (double*)(base + P.part_off);
    if (store)
        hipLaunchKernelGGL(k_nullmany_mix<true>, dim3((unsigned)P.chunks), dim3(256), 0, st, a, b, tab, prm, n_pairs, matched, null_out, scaled, part);
    else
        hipLaunchKernelGGL(k_nullmany_mix<false>, dim3((unsigned)P.chunks), dim3(256), 0, st, a, b, tab, prm, n_pairs, matched, null_out, scaled, part);
    EGR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_nullmany_reduce, dim3((unsigned)n_pairs), dim3(256), 0, st, (const double*)part, tab, out8);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}
