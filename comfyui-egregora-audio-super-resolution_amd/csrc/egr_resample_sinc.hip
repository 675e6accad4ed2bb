// Windowed-sinc rational-rate resampler with torchaudio.functional.resample's definition (SPEC.md 4f): per-phase taps designed on
// the host in float64 (resample.design_sinc), evaluated here from the compact tap-major table Kt[s n + p] and the per-phase first
// tap.  All index arithmetic and every refusal is in egr_sinc_index.h (host + device, walked by tools/sinc_host_check.cpp).
//
// One output sample is stated once (sinc_sample): the taps of the phase's run in ascending order, one __fmaf_rn per tap in float32.
// The four kernels differ only in how a thread finds its sample and where it reads x from, so a sample has the same bits in the
// staged and the direct variant and in the single and the many-clip call.  Grids are flat and equal the work count (one thread per
// output, no stride loop); no atomics, no inline assembly.  Built without SLP-formed packed arithmetic and without contraction
// (Makefile: NOPK, -ffp-contract=off).
#include "egr_common.h"
#include "egr_sinc_index.h"

namespace egr {

// x as the definition pads it: zero outside [0, n_in)
struct SincGlobalLoad {
    const float* __restrict__ x;
    long long n_in, first;
    __device__ __forceinline__ float operator()(int s) const {
        const long long k = first + s;
        return (k >= 0 && k < n_in) ? x[k] : 0.f;
    }
};

// the tile's span in LDS, zero filled outside the clip when it was staged
struct SincLdsLoad {
    const float* w;
    __device__ __forceinline__ float operator()(int s) const { return w[s]; }
};

// y = sum_s Kt[s n + p] * x_s, s ascending, one fused multiply-add per tap
template <class Load>
__device__ __forceinline__ float sinc_sample(const Load& x, const float* __restrict__ kt, int n, int p, int run) {
    const float* k = kt + p;
    float acc = 0.f;
#pragma unroll 4
    for (int s = 0; s < run; ++s) acc = __fmaf_rn(k[(size_t)s * n], x(s), acc);
    return acc;
}

struct SincFilter {
    int o, n, width, run;
    const float* __restrict__ kt;
    const int* __restrict__ first_tap;
};

__device__ __forceinline__ float sinc_direct_output(const float* __restrict__ x, long long n_in, const SincFilter& F, long long m) {
    int p;
    const long long i = sinc_frame_phase(m, F.n, &p);
    const long long f = sinc_first_tap(F.first_tap[p], F.o, F.width, F.run);
    return sinc_sample(SincGlobalLoad{x, n_in, sinc_first_in(i, F.o, F.width, f)}, F.kt, F.n, p, F.run);
}

// len <= 256 consecutive outputs of one track from local output m0, by the whole workgroup: thread lane0 + j writes output m0 + j.
// The span is copied once (consecutive threads, consecutive floats), then every thread reads its run from it.  Uniform in the
// workgroup: both barriers are met by all 256 threads.
__device__ __forceinline__ void sinc_staged_tile(const float* __restrict__ x, long long n_in, float* __restrict__ y, const SincFilter& F,
                                                 long long m0, int len, int lane0, float* lds) {
    long long lo;
    const int span = (int)sinc_tile_span(m0, len, F.o, F.n, F.width, &lo);
    for (int q = threadIdx.x; q < span; q += SINC_TILE) {
        const long long k = lo + q;
        lds[q] = (k >= 0 && k < n_in) ? x[k] : 0.f;
    }
    __syncthreads();
    const int j = (int)threadIdx.x - lane0;
    if (j >= 0 && j < len) {
        const long long m = m0 + j;
        int p;
        const long long i = sinc_frame_phase(m, F.n, &p);
        const long long f = sinc_first_tap(F.first_tap[p], F.o, F.width, F.run);
        y[m] = sinc_sample(SincLdsLoad{lds + sinc_stage_slot(m0, i, F.o, F.n, f)}, F.kt, F.n, p, F.run);
    }
    __syncthreads();
}

extern __shared__ float sinc_lds[];

// grid (tiles of n_out, channels)
__global__ __launch_bounds__(256) void k_resample_sinc_staged(const float* __restrict__ x, long long n_in, long long n_out, SincFilter F,
                                                               float* __restrict__ y) {
    const long long m0 = (long long)blockIdx.x * SINC_TILE;
    const long long left = n_out - m0;
    sinc_staged_tile(x + (size_t)blockIdx.y * n_in, n_in, y + (size_t)blockIdx.y * n_out, F, m0, left < SINC_TILE ? (int)left : SINC_TILE,
                     0, sinc_lds);
}

__global__ __launch_bounds__(256) void k_resample_sinc_direct(const float* __restrict__ x, long long n_in, long long n_out, SincFilter F,
                                                               float* __restrict__ y) {
    const long long m = (long long)blockIdx.x * SINC_TILE + threadIdx.x;
    if (m < n_out) y[(size_t)blockIdx.y * n_out + m] = sinc_direct_output(x + (size_t)blockIdx.y * n_in, n_in, F, m);
}

// tracks[t] = (in offset, n_in, out offset, n_out); out offsets ascend back to back from 0 to total_out (k_resample_poly_tracks'
// contract).  A tile's 256 flat outputs mostly belong to one track; where track starts fall inside it, the workgroup stages and
// computes one stretch per track, in order.
__global__ __launch_bounds__(256) void k_resample_sinc_staged_tracks(const float* __restrict__ x, const long long* __restrict__ tracks,
                                                                      int n_tracks, long long total_out, SincFilter F,
                                                                      float* __restrict__ y) {
    const long long base = (long long)blockIdx.x * SINC_TILE;
    const long long end = base + SINC_TILE < total_out ? base + SINC_TILE : total_out;
    int t = track_of(tracks, n_tracks, ST_COLS, ST_OUT, base);
    for (long long pos = base; pos < end;) {
        long long m0, len;
        const long long seg_end = sinc_segment(tracks, n_tracks, total_out, end, pos, &t, &m0, &len);
        const long long* e = tracks + (size_t)t * ST_COLS;
        if (len > 0) sinc_staged_tile(x + e[ST_IN], e[ST_N_IN], y + e[ST_OUT], F, m0, (int)len, (int)(pos - base), sinc_lds);
        pos = seg_end;
    }
}

__global__ __launch_bounds__(256) void k_resample_sinc_direct_tracks(const float* __restrict__ x, const long long* __restrict__ tracks,
                                                                      int n_tracks, long long total_out, SincFilter F,
                                                                      float* __restrict__ y) {
    const long long base = (long long)blockIdx.x * SINC_TILE;
    int t = track_of(tracks, n_tracks, ST_COLS, ST_OUT, base);
    const long long i = base + threadIdx.x;
    if (i >= total_out) return;
    while (t + 1 < n_tracks && tracks[(size_t)(t + 1) * ST_COLS + ST_OUT] <= i) ++t;
    const long long* e = tracks + (size_t)t * ST_COLS;
    const long long m = i - e[ST_OUT];
    if (m < e[ST_N_OUT]) y[i] = sinc_direct_output(x + e[ST_IN], e[ST_N_IN], F, m);
}

static const char* sinc_why(int why) {
    switch (why) {
        case SINC_SHORT: return "a length below 1";
        case SINC_BAD_RATE: return "o, n, width or run outside the supported range";
        case SINC_OFFSET: return "a length or offset beyond the 64-bit offset cap";
        case SINC_TOTAL: return "more outputs than one launch holds";
        case SINC_TABLE: return "n * run is above the table cap";
        case SINC_LENGTH: return "n_out is not ceil(n_in * n / o), or more tracks than outputs";
        case SINC_CHANNELS: return "channels outside [1, 65535]";
    }
    return "ok";
}

static int sinc_code(int why) { return (why == SINC_TOTAL || why == SINC_TABLE) ? EGR_ERR_UNSUPPORTED : EGR_ERR_ARG; }

}  // namespace egr

using namespace egr;

extern "C" int egr_resample_sinc(const float* x, int channels, int64_t n_in, int o, int n, int width, int run, const float* table,
                                 const int32_t* first_tap, unsigned flags, float* y, int64_t n_out, void* stream) {
    int why = sinc_filter_check(o, n, width, run);
    EGR_CHECK(why == SINC_OK, sinc_code(why), "egr_resample_sinc: o=%d n=%d width=%d run=%d: %s", o, n, width, run, sinc_why(why));
    why = sinc_single_check(channels, n_in, n_out, o, n);
    EGR_CHECK(why == SINC_OK, sinc_code(why), "egr_resample_sinc: channels=%d n_in=%lld n_out=%lld: %s", channels, (long long)n_in,
              (long long)n_out, sinc_why(why));
    EGR_CHECK((flags & ~SINC_FORCE_DIRECT) == 0, EGR_ERR_ARG, "egr_resample_sinc: unknown flag bits 0x%x", flags);
    EGR_CHECK(x && table && first_tap && y, EGR_ERR_ARG, "egr_resample_sinc: null pointer");
    const SincFilter F{o, n, width, run, table, first_tap};
    const dim3 grid((unsigned)eval_ceil_div(n_out, SINC_TILE), (unsigned)channels);
    if (sinc_staged(o, n, width) && !(flags & SINC_FORCE_DIRECT))
        hipLaunchKernelGGL(k_resample_sinc_staged, grid, dim3(SINC_TILE), (size_t)sinc_max_span(o, n, width) * sizeof(float),
                           (hipStream_t)stream, x, (long long)n_in, (long long)n_out, F, y);
    else
        hipLaunchKernelGGL(k_resample_sinc_direct, grid, dim3(SINC_TILE), 0, (hipStream_t)stream, x, (long long)n_in, (long long)n_out, F, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_resample_sinc_tracks(const float* x, const int64_t* tracks, int n_tracks, int64_t total_out, int o, int n, int width,
                                        int run, const float* table, const int32_t* first_tap, unsigned flags, float* y, void* stream) {
    int why = sinc_filter_check(o, n, width, run);
    EGR_CHECK(why == SINC_OK, sinc_code(why), "egr_resample_sinc_tracks: o=%d n=%d width=%d run=%d: %s", o, n, width, run, sinc_why(why));
    why = sinc_tracks_check(n_tracks, total_out);
    EGR_CHECK(why == SINC_OK, sinc_code(why), "egr_resample_sinc_tracks: n_tracks=%d total_out=%lld: %s", n_tracks, (long long)total_out,
              sinc_why(why));
    EGR_CHECK((flags & ~SINC_FORCE_DIRECT) == 0, EGR_ERR_ARG, "egr_resample_sinc_tracks: unknown flag bits 0x%x", flags);
    EGR_CHECK(x && tracks && table && first_tap && y, EGR_ERR_ARG, "egr_resample_sinc_tracks: null pointer");
    const SincFilter F{o, n, width, run, table, first_tap};
    const dim3 grid((unsigned)eval_ceil_div(total_out, SINC_TILE));
    if (sinc_staged(o, n, width) && !(flags & SINC_FORCE_DIRECT))
        hipLaunchKernelGGL(k_resample_sinc_staged_tracks, grid, dim3(SINC_TILE), (size_t)sinc_max_span(o, n, width) * sizeof(float),
                           (hipStream_t)stream, x, (const long long*)tracks, n_tracks, (long long)total_out, F, y);
    else
        hipLaunchKernelGGL(k_resample_sinc_direct_tracks, grid, dim3(SINC_TILE), 0, (hipStream_t)stream, x, (const long long*)tracks,
                           n_tracks, (long long)total_out, F, y);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}
