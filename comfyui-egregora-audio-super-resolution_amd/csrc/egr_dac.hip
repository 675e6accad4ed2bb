// Descript Audio Codec forward pass on gfx950 (SPEC.md 4e): encoder, residual vector quantiser, decoder.
//
// The handle keeps the weights (weight norm already folded by the host, dac_weights.pack) prepared for the contraction launcher
// (csrc/egr_nn_gemm.hip) by the library's one weight path (egr_weight_prep.h: packed and split on the device at create): every
// convolution with Cin % 16 == 0 runs on two fp16 terms per operand (scheme 1, egr_conv_h2's path), the others on the fp32 MFMA
// kernel.  Workspace, device checks and the stage read are the handles' shared ones (egr_handle.h).  Activations are channels-last
// [rows][L][C]; rows are independent mono signals.  Own kernels:
//   k_dac_snake    x + sin^2(alpha x) / (alpha + 1e-9) per channel, and the row's max |y| for the contraction that reads y
//   k_dac_conv_in  the Cin = 1, k = 7 input convolution of a window at a sample offset of the whole x (zeros outside [0, n): the right
//                  pad to a multiple of the hop, and the true ends)
//   k_dac_conv_out the Cout = 1, k = 7 output convolution with tanh: per input row seven partial dots, then a 7-term gather; stores a
//                  range of the window at its place in the whole y
//   k_dac_vq       all stages of the residual quantiser in one launch; a workgroup keeps the residuals and sums of its frames in LDS
//   k_dac_from_codes  z from integer codes, on k_dac_vq's own out_proj chain (dac_out_proj)
//   k_dac_mask_frames  a many call's decoder input: zero beyond each row's own frames
// The walks run on a window of latent frames (walk_encode_window / walk_decode_window); one pass is the window [0, F), a segmented
// call (egr_dacseg_encode / _decode) runs the windows of egr_dacseg_plan one after the other through one arena and keeps
// only the frames whose dependency cone lies inside their window: exact in exact arithmetic, fp32 round-off here, because the operand
// scales come from each window's own row maxima.
// A many call (egr_dacmany_encode / _decode) is the window [0, pad_frames) over rows of their own lengths: k_dac_snake<true>
// stores +0.0f at and beyond a row's length at its level, k_dac_conv_in<true> reads each row's own [0, n) of a flat x, so every
// convolution sees at a row's end the zero padding the single call gives it; the per-row tables live in the Walk of that call.
// Work is enqueued on the caller's stream; nothing synchronises (the workspace grows with hipMallocAsync on that stream; the launcher's
// split-K scratch is allocated the first time a stream needs it).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "egr_conv.h"
#include "egr_handle.h"

namespace egr {
namespace {

constexpr int DAC_LDS_MAX = 160 * 1024;
constexpr int DAC_LDS_BUDGET = 150 * 1024;
constexpr int DAC_MAX_WIDTH = 2048, DAC_MAX_RATE = 16, DAC_MAX_CODEBOOKS = 32, DAC_MAX_CB_FLOATS = 16384, DAC_MAX_CB_DIM = 64;
constexpr int DAC_AMAX_SLOTS = 8 * 7 + 4;          // snakes of one side (7 per block, one in front of the output convolution) + z

// ------------------------------------------------------------------------------------------------------------------ kernels
// y = x + sin^2(alpha[c] x) * inva[c] over rows of per_row = L * C floats (in place when y == x); row_amax[r * EGR_ROW_AMAX_STRIDE]
// (zeroed by the host) is raised to the row's max |y|.  RAG (a many call): row r holds len[r] valid positions of
// C floats; beyond them y is +0.0f, x is not read there and nothing there raises the row's maximum.  (A position is C floats, so with
// C % 4 == 0 the boundary falls between two float4.)
template <bool RAG>
__global__ __launch_bounds__(256) void k_dac_snake(const float* x, const float* __restrict__ alpha, const float* __restrict__ inva, float* y,
                                                   long long per_row, int C, unsigned* __restrict__ row_amax, const int* __restrict__ len) {
    __shared__ float wmax[4];
    const int r = blockIdx.y;
    const float* xr = x + (size_t)r * per_row;
    float* yr = y + (size_t)r * per_row;
    long long valid = per_row;
    if (RAG) { const long long v = (long long)len[r] * C; valid = v < per_row ? v : per_row; }
    float vm = 0.f;
    if ((C & 3) == 0) {
        for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < per_row; i += (long long)gridDim.x * 1024) {
            if (RAG && i >= valid) { *(float4*)(yr + i) = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
            const int c = (int)(i % C);
            const float4 v = *(const float4*)(xr + i), a = *(const float4*)(alpha + c), q = *(const float4*)(inva + c);
            float4 o;
            float t;
            t = sinf(a.x * v.x); o.x = fmaf(t * t, q.x, v.x);
            t = sinf(a.y * v.y); o.y = fmaf(t * t, q.y, v.y);
            t = sinf(a.z * v.z); o.z = fmaf(t * t, q.z, v.z);
            t = sinf(a.w * v.w); o.w = fmaf(t * t, q.w, v.w);
            *(float4*)(yr + i) = o;
            vm = fmaxf(vm, fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))));
        }
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per_row; i += (long long)gridDim.x * 256) {
            if (RAG && i >= valid) { yr[i] = 0.f; continue; }
            const int c = (int)(i % C);
            const float v = xr[i], t = sinf(alpha[c] * v), o = fmaf(t * t, inva[c], v);
            yr[i] = o;
            vm = fmaxf(vm, fabsf(o));
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) vm = fmaxf(vm, __shfl_xor(vm, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = vm;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned bits = __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
        unsigned* slot = row_amax + (size_t)r * EGR_ROW_AMAX_STRIDE;
        if (bits > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, bits);
    }
}

// y[r][l][c] = b[c] + sum_t w[t][c] x[r][x0 + l + t - 3] for the Lw samples of a window that begins at sample x0 of the whole
// x [rows][n] (rows n apart), read as zero outside [0, n): the right pad to a multiple of the hop, and the true ends of the signal.
// One pass is x0 = 0, Lw = n_pad.  RAG (a many call): row r is the rows[r][1] samples at rows[r][0] of a flat x, each row with its own
// [0, n).
template <bool RAG>
__global__ __launch_bounds__(256) void k_dac_conv_in(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                     float* __restrict__ y, long long n_all, long long x0, long long Lw, int D, long long total,
                                                     const long long* __restrict__ rows) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % D);
        const long long t = i / D, l = t % Lw, r = t / Lw;
        const long long n = RAG ? rows[2 * r + 1] : n_all;
        const float* xr = x + (RAG ? rows[2 * r] : r * n);
        float acc = b[c];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const long long li = x0 + l + k - 3;
            const float xv = (li >= 0 && li < n) ? xr[li] : 0.f;
            acc = fmaf(w[k * D + c], xv, acc);
        }
        y[i] = acc;
    }
}

// z [rows][P][latent] channels-last: frames at or beyond frames[r] of row r become +0.0f (a many call's decoder input: the operand
// scale of the input convolution then comes from the row's own frames, and the convolution sees the zeros of a row that ends there).
__global__ __launch_bounds__(256) void k_dac_mask_frames(float* __restrict__ z, const int* __restrict__ frames, long long P, int latent, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long t = i / latent;
        if (t % P >= frames[t / P]) z[i] = 0.f;
    }
}

// y[r][l] = tanh(b + sum_t sum_c w[t][c] x[r][l + t - 3][c]) over a window x [rows][L][C] (zero outside [0, L)), of which only the
// outputs [o0, o1) are stored: output l goes to sample y0 + l of the whole y (rows ldy apart).  One pass is o0 = 0, o1 = L = ldy,
// y0 = 0.  A workgroup owns 64 outputs of one row; each wave turns input rows into their seven partial dots (lanes stride the
// channels, a fixed butterfly sums them), then 64 threads gather seven partials each.
constexpr int DAC_OUT_TL = 64;
__global__ __launch_bounds__(256) void k_dac_conv_out(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                      float* __restrict__ y, long long L, int C, long long o0, long long o1, long long y0,
                                                      long long ldy) {
    __shared__ float part[DAC_OUT_TL + 6][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = blockIdx.y, l0 = o0 + (long long)blockIdx.x * DAC_OUT_TL;
    for (int j = wave; j < DAC_OUT_TL + 6; j += 4) {
        const long long li = l0 - 3 + j;
        float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (li >= 0 && li < L) {                       // wave-uniform
            const float* xr = x + ((size_t)r * L + li) * C;
            for (int c = lane; c < C; c += 64) {
                const float xv = xr[c];
#pragma unroll
                for (int t = 0; t < 7; ++t) acc[t] = fmaf(w[t * C + c], xv, acc[t]);
            }
#pragma unroll
            for (int t = 0; t < 7; ++t)
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) acc[t] += __shfl_xor(acc[t], o);
        }
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < 7; ++t) part[j][t] = acc[t];
        }
    }
    __syncthreads();
    const int o = threadIdx.x;
    if (o < DAC_OUT_TL && l0 + o < o1 && l0 + o < L) {
        float v = b[0];
#pragma unroll
        for (int t = 0; t < 7; ++t) v += part[o + t][t];
        y[(size_t)r * ldy + y0 + l0 + o] = tanhf(v);
    }
}

// The residual quantiser (DAC-P8).  Frame g = row * F + f of the channels-last input; a workgroup owns TF frames, 32 lanes each: lane
// `sub` of a frame holds channels sub, sub + 32, ... of the frame's residual and sum in LDS (only that lane touches them), the stage's
// pre-normalised codebook is staged in LDS for the search.  Ties go to the lowest index: a lane walks its codes in ascending order and
// keeps the first maximum, the butterfly prefers the lower index on equal similarity.
struct VqP {
    const float* ze; float* z; int* codes; float* rdump;
    const float* in_w;      // [ncb][latent][cd]
    const float* in_b;      // [ncb][cd]
    const float* cbn;       // [ncb][K][cd], rows of unit norm
    const float* cb;        // [ncb][K][cd] as stored
    const float* out_w;     // [ncb][latent][cd]
    const float* out_b;     // [ncb][latent]
    int latent, cd, K, ncb, TF;
    long long total, F;
};

// One channel of a stage's out_proj on a stored codebook row: bias first, then the taps in ascending order.  k_dac_vq and
// k_dac_from_codes both sum the stages' values of this chain in stage order from 0.f, so the same codes give the same bits of z.
template <int CD>
__device__ __forceinline__ float dac_out_proj(const float* __restrict__ wp, const float* __restrict__ crow, float q, int cd) {
    if (CD == 8) {
        const float4 w0 = *(const float4*)wp, w1 = *(const float4*)(wp + 4), c0 = *(const float4*)crow, c1 = *(const float4*)(crow + 4);
        q = fmaf(w0.x, c0.x, q); q = fmaf(w0.y, c0.y, q); q = fmaf(w0.z, c0.z, q); q = fmaf(w0.w, c0.w, q);
        q = fmaf(w1.x, c1.x, q); q = fmaf(w1.y, c1.y, q); q = fmaf(w1.z, c1.z, q); q = fmaf(w1.w, c1.w, q);
    } else {
        for (int j = 0; j < cd; ++j) q = fmaf(wp[j], crow[j], q);
    }
    return q;
}

template <int CD>
__global__ __launch_bounds__(256) void k_dac_vq(const VqP p) {
    extern __shared__ float lds[];
    const int cd = CD ? CD : p.cd, latent = p.latent, K = p.K;
    float* cbs = lds;                                   // [K][cd]
    float* rs = cbs + (size_t)K * cd;                   // [TF][latent]
    float* zs = rs + (size_t)p.TF * latent;             // [TF][latent]
    float* es = zs + (size_t)p.TF * latent;             // [TF][cd] projections
    float* ehs = es + p.TF * cd;                        // [TF][cd] normalised
    int* code_s = (int*)(ehs + p.TF * cd);              // [TF]
    const int tid = threadIdx.x, nthr = blockDim.x, fl = tid >> 5, sub = tid & 31;
    const long long g = (long long)blockIdx.x * p.TF + fl;
    const bool active = g < p.total;
    float* myr = rs + (size_t)fl * latent;
    float* myz = zs + (size_t)fl * latent;
    for (int c = sub; c < latent; c += 32) {
        myr[c] = active ? p.ze[(size_t)g * latent + c] : 0.f;
        myz[c] = 0.f;
    }
    for (int i = 0; i < p.ncb; ++i) {
        __syncthreads();                                // the previous stage's search has left cbs / ehs / code_s
        const float* src = p.cbn + (size_t)i * K * cd;
        for (int t = tid; t < K * cd; t += nthr) cbs[t] = src[t];
        if (p.rdump && active) {
            float* rd = p.rdump + ((size_t)i * p.total + g) * latent;
            for (int c = sub; c < latent; c += 32) rd[c] = myr[c];
        }
        // in_proj: e[j] = b[j] + sum_c W[c][j] r[c], eight outputs a pass
        for (int j0 = 0; j0 < cd; j0 += 8) {
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int c = sub; c < latent; c += 32) {
                const float rv = myr[c];
                const float* wp = p.in_w + ((size_t)i * latent + c) * cd + j0;
                if (CD == 8) {                           // (rows of eight floats: 32-byte aligned)
                    const float4 w0 = *(const float4*)wp, w1 = *(const float4*)(wp + 4);
                    acc[0] = fmaf(w0.x, rv, acc[0]); acc[1] = fmaf(w0.y, rv, acc[1]); acc[2] = fmaf(w0.z, rv, acc[2]); acc[3] = fmaf(w0.w, rv, acc[3]);
                    acc[4] = fmaf(w1.x, rv, acc[4]); acc[5] = fmaf(w1.y, rv, acc[5]); acc[6] = fmaf(w1.z, rv, acc[6]); acc[7] = fmaf(w1.w, rv, acc[7]);
                } else {
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj)
                        if (j0 + jj < cd) acc[jj] = fmaf(wp[jj], rv, acc[jj]);
                }
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
#pragma unroll
                for (int o = 16; o >= 1; o >>= 1) acc[jj] += __shfl_xor(acc[jj], o);
                if (sub == jj && j0 + jj < cd) es[fl * cd + j0 + jj] = acc[jj] + p.in_b[i * cd + j0 + jj];
            }
        }
        __syncthreads();
        float n2 = 0.f;
        for (int j = 0; j < cd; ++j) { const float e = es[fl * cd + j]; n2 = fmaf(e, e, n2); }
        const float inv = 1.0f / fmaxf(sqrtf(n2), 1e-12f);
        for (int j = sub; j < cd; j += 32) ehs[fl * cd + j] = es[fl * cd + j] * inv;
        __syncthreads();
        float best = -INFINITY;
        int bk = 0x7fffffff;
        if (CD == 8) {
            const float4 e0 = *(const float4*)(ehs + fl * 8), e1 = *(const float4*)(ehs + fl * 8 + 4);
            for (int k = sub; k < K; k += 32) {
                const float4 c0 = *(const float4*)(cbs + k * 8), c1 = *(const float4*)(cbs + k * 8 + 4);
                float s = e0.x * c0.x;
                s = fmaf(e0.y, c0.y, s); s = fmaf(e0.z, c0.z, s); s = fmaf(e0.w, c0.w, s);
                s = fmaf(e1.x, c1.x, s); s = fmaf(e1.y, c1.y, s); s = fmaf(e1.z, c1.z, s); s = fmaf(e1.w, c1.w, s);
                if (s > best) { best = s; bk = k; }
            }
        } else {
            for (int k = sub; k < K; k += 32) {
                float s = 0.f;
                for (int j = 0; j < cd; ++j) s = fmaf(ehs[fl * cd + j], cbs[k * cd + j], s);
                if (s > best) { best = s; bk = k; }
            }
        }
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int ok = __shfl_xor(bk, o);
            if (ob > best || (ob == best && ok < bk)) { best = ob; bk = ok; }
        }
        if (sub == 0) code_s[fl] = (bk >= 0 && bk < K) ? bk : 0;       // (no finite similarity: code 0)
        __syncthreads();
        const int code = code_s[fl];
        if (sub == 0 && active) {
            const long long row = g / p.F, f = g % p.F;
            p.codes[((size_t)row * p.ncb + i) * p.F + f] = code;
        }
        // out_proj of the stored codebook row, then z += q, r -= q
        const float* crow = p.cb + ((size_t)i * K + code) * cd;
        for (int c = sub; c < latent; c += 32) {
            const float q = dac_out_proj<CD>(p.out_w + ((size_t)i * latent + c) * cd, crow, p.out_b[(size_t)i * latent + c], cd);
            myz[c] += q;
            myr[c] -= q;
        }
    }
    if (active)
        for (int c = sub; c < latent; c += 32) p.z[(size_t)g * latent + c] = myz[c];
}

size_t vq_lds_bytes(int K, int cd, int latent, int TF) {
    return ((size_t)K * cd + 2 * (size_t)TF * latent + 2 * (size_t)TF * cd) * sizeof(float) + (size_t)TF * sizeof(int);
}

// z[r][c][f] = sum over the stages i, in order, of out_proj_i(codebook_i[codes[r][i][f]])[c] (with bias, from the rows as stored:
// DAC-P8), straight into [rows][latent][frames].  A thread owns one frame and DAC_FC_CH channels of it: the codes are read along f,
// the out_proj rows are wave-uniform.  A code outside [0, K) reads row 0 (the engine refuses such codes; nothing is read outside
// a codebook whatever arrives).
constexpr int DAC_FC_CH = 8;
template <int CD>
__global__ __launch_bounds__(256) void k_dac_from_codes(const VqP p) {
    const int cd = CD ? CD : p.cd, latent = p.latent;
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x, r = blockIdx.z;
    const int c0 = blockIdx.y * DAC_FC_CH;
    if (f >= p.F) return;
    float acc[DAC_FC_CH];
#pragma unroll
    for (int u = 0; u < DAC_FC_CH; ++u) acc[u] = 0.f;
    for (int i = 0; i < p.ncb; ++i) {
        const unsigned code = (unsigned)p.codes[((size_t)r * p.ncb + i) * p.F + f];
        const float* crow = p.cb + ((size_t)i * p.K + (code < (unsigned)p.K ? code : 0u)) * cd;
#pragma unroll
        for (int u = 0; u < DAC_FC_CH; ++u)
            if (c0 + u < latent)                        // block-uniform
                acc[u] += dac_out_proj<CD>(p.out_w + ((size_t)i * latent + c0 + u) * cd, crow, p.out_b[(size_t)i * latent + c0 + u], cd);
    }
#pragma unroll
    for (int u = 0; u < DAC_FC_CH; ++u)
        if (c0 + u < latent) p.z[((size_t)r * latent + c0 + u) * p.F + f] = acc[u];
}

// ------------------------------------------------------------------------------------------------------------------ the handle
struct Conv {                       // one convolution served by the contraction launcher
    int Cin = 0, Cout = 0, K = 1, stride = 1, dil = 1, pad = 0;
    PreparedWeight w;               // two fp16 terms (Cin % 16 == 0), the fp32 pack otherwise
    const float* bias = nullptr;
    size_t o_bias = 0;              // of the bias in the tables, while they are built
};
struct Snake { const float* alpha = nullptr; const float* inva = nullptr; size_t o = 0; int C = 0; };
struct ResUnit { Snake s1, s2; Conv c7, c1; };
struct EncBlock { ResUnit ru[3]; Snake s; Conv down; };
struct DecBlock { Snake s; Conv up; int k = 0, stride = 0, pad = 0, c_out = 0; ResUnit ru[3]; };
struct StageRec { int kind, index; const float* p; int64_t count; };

struct Dac {
    egr_dac_config cfg;
    int device = 0;
    int latent = 0, TF = 8;
    bool keep_vq_inputs = false;     // egr_dac_set_stages: the quantiser also writes the residual entering each stage
    // encoder
    const float* in_w = nullptr; const float* in_b = nullptr; size_t o_in_w = 0, o_in_b = 0;
    std::vector<EncBlock> enc;
    Snake enc_s; Conv enc_out;
    // quantiser
    VqP vq{};
    size_t o_vq[6] = {0, 0, 0, 0, 0, 0};
    // decoder
    Conv dec_in;
    std::vector<DecBlock> dec;
    Snake dec_s;
    const float* out_w = nullptr; const float* out_b = nullptr; size_t o_out_w = 0, o_out_b = 0; int c_last = 0;
    float* d_misc = nullptr;        // biases, snake tables, thin convolutions, quantiser
    float* d_f32 = nullptr;         // fp32 packs of the convolutions the split kernels do not take
    void* d_w2 = nullptr;           // fp16 term packs
    Workspace ws;
    TableStage tables;              // many calls only: the host side of their per-row tables
    std::vector<StageRec> stages;
};

int64_t conv_len(int64_t L, int s) {                 // Conv1d(k = 2 s, stride s, padding ceil(s / 2))
    const int64_t num = L + 2 * ((s + 1) / 2) - 2 * s;
    return num < 0 ? 0 : num / s + 1;
}
int64_t convtr_len(int64_t L, int s) { return (L - 1) * s - 2 * ((s + 1) / 2) + 2 * s; }

int lengths(const egr_dac_config& c, int64_t n, int64_t* n_pad, int64_t* frames, int64_t* n_dec) {
    int64_t hop = 1;
    for (int i = 0; i < c.n_enc; ++i) hop *= c.enc_rates[i];
    const int64_t np = (n + hop - 1) / hop * hop;
    int64_t L = np;
    for (int i = 0; i < c.n_enc; ++i) L = conv_len(L, c.enc_rates[i]);
    const int64_t F = L;
    for (int i = 0; i < c.n_dec; ++i) L = L >= 1 ? convtr_len(L, c.dec_rates[i]) : 0;
    if (n_pad) *n_pad = np;
    if (frames) *frames = F;
    if (n_dec) *n_dec = L;
    return EGR_OK;
}
int64_t decoded_len(const egr_dac_config& c, int64_t frames) {
    int64_t L = frames;
    for (int i = 0; i < c.n_dec; ++i) L = L >= 1 ? convtr_len(L, c.dec_rates[i]) : 0;
    return L;
}

// ---- the segment plan: how far a kept frame's dependency cone reaches, from the layer list itself
struct Reach { int tr, k, s, d, p; };                 // Conv1d (tr = 0) or ConvTranspose1d (tr = 1)
int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

std::vector<Reach> layer_list(const egr_dac_config& c, int kind) {
    std::vector<Reach> v;
    auto units = [&] { for (int d : {1, 3, 9}) { v.push_back({0, 7, 1, d, 3 * d}); v.push_back({0, 1, 1, 1, 0}); } };
    if (kind == EGR_DAC_ENCODE) {
        v.push_back({0, 7, 1, 1, 3});
        for (int i = 0; i < c.n_enc; ++i) { units(); v.push_back({0, 2 * c.enc_rates[i], c.enc_rates[i], 1, (c.enc_rates[i] + 1) / 2}); }
        v.push_back({0, 3, 1, 1, 1});
    } else {
        v.push_back({0, 7, 1, 1, 3});
        for (int i = 0; i < c.n_dec; ++i) { v.push_back({1, 2 * c.dec_rates[i], c.dec_rates[i], 1, (c.dec_rates[i] + 1) / 2}); units(); }
        v.push_back({0, 7, 1, 1, 3});
    }
    return v;
}

// Frames of margin a window needs on the (left, right) of the frames it keeps.  The outputs of kept frame 0 -- the frame itself
// (encode) or its H = prod dec_rates samples (decode) -- are walked back through the layers: a Conv1d output o reads
// o s - p + t d, a ConvTranspose1d output j receives input i where j = i s - p + t (0 <= t < k).  Every rule commutes with a shift
// by whole frames, so frame 0 stands for all.  A value is exact when this cone lies inside the window: whatever the window pads
// with zeros at its cut ends then lies outside the cone.
void seg_margins(const egr_dac_config& c, int kind, int64_t* left, int64_t* right) {
    int64_t hop = 1, lo = 0, hi = 0;
    if (kind == EGR_DAC_ENCODE) for (int i = 0; i < c.n_enc; ++i) hop *= c.enc_rates[i];
    else for (int i = 0; i < c.n_dec; ++i) hop *= c.dec_rates[i];
    if (kind == EGR_DAC_DECODE) hi = hop - 1;
    const std::vector<Reach> v = layer_list(c, kind);
    for (size_t i = v.size(); i-- > 0;) {
        const Reach& r = v[i];
        if (r.tr) { lo = ceil_div(lo + r.p - (r.k - 1), r.s); hi = floor_div(hi + r.p, r.s); }
        else { lo = lo * r.s - r.p; hi = hi * r.s - r.p + (int64_t)(r.k - 1) * r.d; }
    }
    if (kind == EGR_DAC_ENCODE) {                        // samples [lo, hi] around frame 0's [0, hop) -> frames
        *left = std::max<int64_t>(0, ceil_div(-lo, hop));
        *right = std::max<int64_t>(0, ceil_div(hi + 1 - hop, hop));
    } else {
        *left = std::max<int64_t>(0, -lo);
        *right = std::max<int64_t>(0, hi);
    }
}

// Interior windows are widened to a multiple of this many frames: every level with at least 8 samples a frame is then a multiple of
// 128 samples long, which is what k_conv1d_s3 asks of a row (one pass meets it only when the file's length happens to).
constexpr int64_t DAC_SEG_ALIGN = 16;

int64_t seg_window_max(const egr_dac_config& c, int kind, int64_t seg_frames) {
    int64_t l, r;
    seg_margins(c, kind, &l, &r);
    return (seg_frames + l + r + DAC_SEG_ALIGN - 1) / DAC_SEG_ALIGN * DAC_SEG_ALIGN;
}

int check_config(const egr_dac_config* c, const char* who) {
    EGR_CHECK(c && c->struct_bytes == (int)sizeof(egr_dac_config), EGR_ERR_ARG, "%s: bad config (struct_bytes)", who);
    EGR_CHECK(c->n_enc >= 1 && c->n_enc <= EGR_DAC_MAX_RATES && c->n_dec >= 1 && c->n_dec <= EGR_DAC_MAX_RATES, EGR_ERR_UNSUPPORTED,
              "%s: 1 .. %d rates per side (got %d / %d)", who, EGR_DAC_MAX_RATES, c->n_enc, c->n_dec);
    for (int i = 0; i < c->n_enc; ++i)
        EGR_CHECK(c->enc_rates[i] >= 1 && c->enc_rates[i] <= DAC_MAX_RATE, EGR_ERR_UNSUPPORTED, "%s: encoder rate %d outside 1 .. %d", who, c->enc_rates[i], DAC_MAX_RATE);
    for (int i = 0; i < c->n_dec; ++i)
        EGR_CHECK(c->dec_rates[i] >= 1 && c->dec_rates[i] <= DAC_MAX_RATE, EGR_ERR_UNSUPPORTED, "%s: decoder rate %d outside 1 .. %d", who, c->dec_rates[i], DAC_MAX_RATE);
    EGR_CHECK(c->encoder_dim >= 1 && c->decoder_dim >= 1 && c->latent_dim >= 1 && c->n_codebooks >= 1 && c->codebook_size >= 1 && c->codebook_dim >= 1,
              EGR_ERR_ARG, "%s: non-positive dimension", who);
    EGR_CHECK(((long long)c->encoder_dim << c->n_enc) <= DAC_MAX_WIDTH && c->decoder_dim <= DAC_MAX_WIDTH && c->latent_dim <= DAC_MAX_WIDTH, EGR_ERR_UNSUPPORTED,
              "%s: widths up to %d (encoder %lld, decoder %d, latent %d)", who, DAC_MAX_WIDTH, (long long)c->encoder_dim << c->n_enc, c->decoder_dim, c->latent_dim);
    EGR_CHECK(c->decoder_dim % (1 << c->n_dec) == 0, EGR_ERR_UNSUPPORTED, "%s: decoder_dim %d does not halve %d times", who, c->decoder_dim, c->n_dec);
    EGR_CHECK(c->n_codebooks <= DAC_MAX_CODEBOOKS, EGR_ERR_UNSUPPORTED, "%s: n_codebooks %d above %d", who, c->n_codebooks, DAC_MAX_CODEBOOKS);
    EGR_CHECK((long long)c->codebook_size * c->codebook_dim <= DAC_MAX_CB_FLOATS && c->codebook_dim <= DAC_MAX_CB_DIM, EGR_ERR_UNSUPPORTED,
              "%s: codebook_size * codebook_dim = %lld above %d, or codebook_dim %d above %d (a codebook must fit in LDS)", who,
              (long long)c->codebook_size * c->codebook_dim, DAC_MAX_CB_FLOATS, c->codebook_dim, DAC_MAX_CB_DIM);
    return EGR_OK;
}

// ---- building the device images from the packed blob
struct Builder {
    const float* src; int64_t n, pos = 0;
    std::vector<float> misc;
    struct Job { Conv* L; int64_t o_src; int layout, Ci, Co, k; };      // a weight of the blob (torch layout, o_src floats in) to prepare
    std::vector<Job> jobs;
    size_t f32_bytes = 0, w2_bytes = 0, tmp_bytes = 0;   // fp32 packs kept, fp16 term packs, the largest fp32 pack that is only split
    bool ok = true;
    const float* take(int64_t k) {
        if (pos + k > n) { ok = false; return nullptr; }
        const float* p = src + pos; pos += k; return p;
    }
    size_t put(const float* p, int64_t k) {            // into misc, 16-byte aligned
        while (misc.size() % 4) misc.push_back(0.f);
        const size_t o = misc.size();
        misc.insert(misc.end(), p, p + k);
        return o;
    }
    void snake(Snake& s, int C) {
        const float* a = take(C);
        if (!a) return;
        s.C = C;
        s.o = put(a, C);
        std::vector<float> inv(C);
        for (int c = 0; c < C; ++c) inv[c] = (float)(1.0 / ((double)a[c] + 1e-9));
        put(inv.data(), C);                             // 1 / (alpha + 1e-9), at the next 16-byte boundary behind alpha
    }
    // torch Conv1d weight [Co][Ci][k] + bias -> egr_pack_weight's layout 0, K ordered (tap, ci)
    void conv(Conv& L, int Ci, int Co, int k, int stride, int dil, int pad) {
        const float* w = take((int64_t)Co * Ci * k);
        const float* b = take(Co);
        if (!w || !b) return;
        L.Cin = Ci; L.Cout = Co; L.K = k; L.stride = stride; L.dil = dil; L.pad = pad;
        L.o_bias = put(b, Co);
        weight(L, w, 0, k * Ci, Co, Ci, Co, k);
    }
    // torch ConvTranspose1d weight [Ci][Co][k] -> GEMM onto columns n = tap * Co + co
    void convtr(Conv& L, int Ci, int Co, int k) {
        const float* w = take((int64_t)Ci * Co * k);
        const float* b = take(Co);
        if (!w || !b) return;
        L.Cin = Ci; L.Cout = k * Co; L.K = 1;
        L.o_bias = put(b, Co);                          // [Co]: added by the gather, not by the GEMM
        weight(L, w, 1, Ci, k * Co, Ci, Co, k);
    }
    void weight(Conv& L, const float* w, int layout, int K, int N, int Ci, int Co, int k) {
        weight_shape(L.w, K, N);
        if (Ci % 16 == 0) { w2_bytes += L.w.term_bytes(2); tmp_bytes = std::max(tmp_bytes, L.w.pack_bytes()); }
        else f32_bytes += L.w.pack_bytes();
        jobs.push_back({&L, w - src, layout, Ci, Co, k});
    }
};

void res_unit(Builder& B, ResUnit& u, int C, int d) {
    B.snake(u.s1, C);
    B.conv(u.c7, C, C, 7, 1, d, 3 * d);
    B.snake(u.s2, C);
    B.conv(u.c1, C, C, 1, 1, 1, 0);
}

void destroy(Dac* m) {
    {
        DeviceScope dev(m->device);
        m->ws.release();
        m->tables.release();
        if (m->d_misc) (void)hipFree(m->d_misc);
        if (m->d_f32) (void)hipFree(m->d_f32);
        if (m->d_w2) (void)hipFree(m->d_w2);
    }
    delete m;
}

// The tables onto the current device, and the blob's convolution weights through prepare_weight on the null stream: the blob goes up
// as it is (torch layouts); a weight that is split passes through one scratch pack behind it, which leaves with the blob.
int upload(Dac* m, const Builder& B, const float* packed, int64_t n_floats) {
    float* d_tmp = nullptr;                            // [blob][one float: a pack's largest magnitude, 16-byte slot][scratch pack]
    const size_t blob_floats = ((size_t)n_floats + 3) & ~(size_t)3;
    auto fail = [&](const char* what) {
        set_error("egr_dac_create: %s failed on device %d", what, m->device);
        if (d_tmp) (void)hipFree(d_tmp);
        return EGR_ERR_HIP;
    };
    if (hipMalloc((void**)&m->d_misc, std::max<size_t>(16, B.misc.size() * 4)) != hipSuccess) return fail("hipMalloc(tables)");
    if (hipMemcpy(m->d_misc, B.misc.data(), B.misc.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return fail("upload(tables)");
    if (B.f32_bytes && hipMalloc((void**)&m->d_f32, B.f32_bytes) != hipSuccess) return fail("hipMalloc(fp32 packs)");
    if (B.w2_bytes && hipMalloc(&m->d_w2, B.w2_bytes) != hipSuccess) return fail("hipMalloc(fp16 terms)");
    if (hipMalloc((void**)&d_tmp, (blob_floats + 4) * 4 + B.tmp_bytes) != hipSuccess) return fail("hipMalloc(staging)");
    if (hipMemcpy(d_tmp, packed, (size_t)n_floats * 4, hipMemcpyHostToDevice) != hipSuccess) return fail("upload(staging)");
    float* slot = d_tmp + blob_floats;
    char* f32 = (char*)m->d_f32;
    char* w2 = (char*)m->d_w2;
    for (const Builder::Job& j : B.jobs) {
        PreparedWeight& w = j.L->w;
        const bool h2 = j.Ci % 16 == 0;
        if (h2) { w.w = slot + 4; w.w2 = w2; w2 += w.term_bytes(2); }
        else { w.w = (float*)f32; f32 += w.pack_bytes(); }
        const int rc = prepare_weight(d_tmp + j.o_src, j.layout, j.Ci, j.Co, 1, j.k, w, slot, nullptr);
        if (rc) { (void)hipFree(d_tmp); return rc; }
        if (h2) w.w = nullptr;                          // (the scratch pack)
        j.L->bias = m->d_misc + j.L->o_bias;
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail("weight repack");
    (void)hipFree(d_tmp);
    return EGR_OK;
}

// ---- one call: the walk lays the workspace out and (launch) enqueues the kernels
struct Walk {
    Dac& m; hipStream_t st; bool launch; int rows;
    char* base = nullptr; size_t off = 0;
    unsigned* amax_pool = nullptr; int amax_used = 0;
    int rc = EGR_OK;
    bool notes = true;              // a segmented or many call records no stage
    // a many call binds its device tables here; null: every row is whole (one pass, segments)
    const int* lens = nullptr;      // [levels][rows]: the valid positions of each row at each level of the side that runs
    const long long* xrows = nullptr;   // [rows][2]: (offset, n) of each row in the flat x (encode)
    float* take(size_t floats) {
        off = (off + 255) & ~(size_t)255;
        float* p = launch ? (float*)(base + off) : nullptr;
        off += floats * sizeof(float);
        return p;
    }
    unsigned* amax_slot() {
        if (amax_used >= DAC_AMAX_SLOTS) { if (!rc) { set_error("DAC: row maxima pool exhausted"); rc = EGR_ERR_UNSUPPORTED; } return amax_pool; }
        unsigned* p = amax_pool + (size_t)amax_used * rows * EGR_ROW_AMAX_STRIDE;
        ++amax_used;
        return p;
    }
    void note(int kind, int index, const float* p, int64_t count) { if (launch && notes) m.stages.push_back({kind, index, p, count}); }
    bool go() const { return launch && rc == EGR_OK; }
    // y = snake(x) (y may be x); returns the row maxima of y
    const unsigned* snake(const Snake& s, const float* x, float* y, int64_t L, int level) {
        unsigned* slot = amax_slot();
        if (!go()) return slot;
        const long long per_row = (long long)L * s.C;
        long long nb = (per_row / ((s.C & 3) ? 1 : 4) + 255) / 256;
        nb = std::max(1LL, std::min(nb, std::max(1LL, 2048LL / rows)));
        if (lens) hipLaunchKernelGGL(k_dac_snake<true>, dim3((unsigned)nb, (unsigned)rows), dim3(256), 0, st, x, s.alpha, s.inva, y, per_row, s.C, slot, lens + (size_t)level * rows);
        else hipLaunchKernelGGL(k_dac_snake<false>, dim3((unsigned)nb, (unsigned)rows), dim3(256), 0, st, x, s.alpha, s.inva, y, per_row, s.C, slot, (const int*)nullptr);
        return slot;
    }
    void conv(const Conv& c, const float* x, const unsigned* x_amax, float* y, const float* res, const float* bias, int64_t Lin, int64_t Lout) {
        if (!go()) return;
        ConvCall cc;
        cc.x = x; cc.y = y; cc.bias = bias; cc.res = res;
        cc.B = rows; cc.W = (int)Lin; cc.Cin = c.Cin; cc.OW = cc.OWF = (int)Lout; cc.Cout = c.Cout; cc.KW = c.K;
        cc.stride = c.stride; cc.dil = c.dil; cc.pad_l = c.pad;
        set_weight(cc, c.w, x_amax, rows);
        rc = conv_call(cc, st);
    }
};

// scratch rotation: a buffer of S that is none of the given ones
float* other(float* const S[3], const float* a, const float* b = nullptr) {
    for (int i = 0; i < 3; ++i)
        if (S[i] != a && S[i] != b) return S[i];
    return S[0];
}

// x -> snake -> k7 dilated -> snake -> k1 + x, into `out` (or a scratch buffer when out is null); returns where the result is
float* run_res_unit(Walk& w, const ResUnit& u, float* cur, float* const S[3], float* out, int64_t L, int level) {
    float* a = other(S, cur), *b = other(S, cur, a);
    const unsigned* ra = w.snake(u.s1, cur, a, L, level);
    w.conv(u.c7, a, ra, b, nullptr, u.c7.bias, L, L);
    const unsigned* rb = w.snake(u.s2, b, b, L, level);
    float* y = out ? out : a;
    w.conv(u.c1, b, rb, y, cur, u.c1.bias, L, L);
    return y;
}

size_t max_enc_tensor(const Dac& m, int rows, int64_t n_pad) {
    size_t mx = 0;
    int64_t L = n_pad;
    int C = m.cfg.encoder_dim;
    for (int i = 0; i < m.cfg.n_enc; ++i) {
        mx = std::max(mx, (size_t)rows * L * C);
        L = conv_len(L, m.cfg.enc_rates[i]);
        C *= 2;
    }
    return std::max(mx, (size_t)rows * L * C);
}

int launch_vq(Walk& w, const float* ze_cl, float* z_cl, int* codes, int64_t F) {
    Dac& m = w.m;
    const long long total = (long long)w.rows * F;
    float* rdump = m.keep_vq_inputs && w.notes ? w.take((size_t)m.cfg.n_codebooks * total * m.latent) : nullptr;
    if (!w.go()) return w.rc;
    VqP p = m.vq;
    p.ze = ze_cl; p.z = z_cl; p.codes = codes; p.rdump = rdump; p.total = total; p.F = F; p.TF = m.TF;
    const size_t lds = vq_lds_bytes(p.K, p.cd, p.latent, p.TF);
    const unsigned grid = (unsigned)((total + p.TF - 1) / p.TF);
    if (p.cd == 8) hipLaunchKernelGGL(k_dac_vq<8>, dim3(grid), dim3(p.TF * 32), lds, w.st, p);
    else hipLaunchKernelGGL(k_dac_vq<0>, dim3(grid), dim3(p.TF * 32), lds, w.st, p);
    for (int i = 0; rdump && i < m.cfg.n_codebooks; ++i) w.note(EGR_DAC_STAGE_VQ_IN, i, rdump + (size_t)i * total * m.latent, total * m.latent);
    return EGR_OK;
}

// A window of the encoder: `frames` latent frames that begin at sample x0 of the whole x [rows][n]; the kept frames [k0, k1) of
// the window (window-relative) go to frame `at` onwards of the whole-length channels-last ze_all [rows][F][latent].  One pass is
// the window [0, F): x0 = 0, every frame kept, and the last convolution writes ze_all itself.
struct EncWindow { int64_t x0, frames, k0, k1, at, F; };

int walk_encode_window(Walk& w, const float* x, int64_t n, const EncWindow& win, float* ze_all) {
    Dac& m = w.m;
    const egr_dac_config& c = m.cfg;
    int64_t hop = 1;
    for (int i = 0; i < c.n_enc; ++i) hop *= c.enc_rates[i];
    const int64_t Lw = win.frames * hop;
    const int rows = w.rows;
    w.amax_used = 0;
    w.amax_pool = (unsigned*)w.take((size_t)DAC_AMAX_SLOTS * rows * EGR_ROW_AMAX_STRIDE);
    if (w.go()) EGR_HIP(hipMemsetAsync(w.amax_pool, 0, (size_t)DAC_AMAX_SLOTS * rows * EGR_ROW_AMAX_STRIDE * 4, w.st));
    const size_t mx = max_enc_tensor(m, rows, Lw);
    float* S[3] = {w.take(mx), w.take(mx), w.take(mx)};
    int C = c.encoder_dim;
    int64_t L = Lw;
    float* cur = w.take((size_t)rows * L * C);
    if (w.go()) {
        const long long total = (long long)rows * L * C;
        const unsigned nb = (unsigned)std::min<long long>((total + 255) / 256, 8192);
        if (w.xrows) hipLaunchKernelGGL(k_dac_conv_in<true>, dim3(nb), dim3(256), 0, w.st, x, m.in_w, m.in_b, cur, (long long)n, (long long)win.x0, (long long)Lw, C, total, w.xrows);
        else hipLaunchKernelGGL(k_dac_conv_in<false>, dim3(nb), dim3(256), 0, w.st, x, m.in_w, m.in_b, cur, (long long)n, (long long)win.x0, (long long)Lw, C, total, (const long long*)nullptr);
    }
    w.note(EGR_DAC_STAGE_ENC, 0, cur, (int64_t)rows * L * C);
    for (int i = 0; i < c.n_enc; ++i) {
        const EncBlock& b = m.enc[i];
        for (int u = 0; u < 3; ++u) cur = run_res_unit(w, b.ru[u], cur, S, nullptr, L, i);
        float* a = other(S, cur);
        const unsigned* ra = w.snake(b.s, cur, a, L, i);
        const int64_t Lo = conv_len(L, c.enc_rates[i]);
        float* out = w.take((size_t)rows * Lo * C * 2);
        w.conv(b.down, a, ra, out, nullptr, b.down.bias, L, Lo);
        cur = out; L = Lo; C *= 2;
        w.note(EGR_DAC_STAGE_ENC, i + 1, cur, (int64_t)rows * L * C);
    }
    if (L != win.frames) { if (!w.rc) { set_error("DAC: a window of %lld frames encodes to %lld", (long long)win.frames, (long long)L); w.rc = EGR_ERR_UNSUPPORTED; } return w.rc; }
    float* a = other(S, cur);
    const unsigned* ra = w.snake(m.enc_s, cur, a, L, c.n_enc);
    const bool whole = win.k0 == 0 && win.k1 == L && win.at == 0 && L == win.F;
    float* ze = whole ? ze_all : w.take((size_t)rows * L * m.latent);
    w.conv(m.enc_out, a, ra, ze, nullptr, m.enc_out.bias, L, L);
    w.note(EGR_DAC_STAGE_ENC, c.n_enc + 1, ze, (int64_t)rows * L * m.latent);
    if (!whole && w.go())
        EGR_HIP(hipMemcpy2DAsync(ze_all + (size_t)win.at * m.latent, (size_t)win.F * m.latent * 4, ze + (size_t)win.k0 * m.latent, (size_t)L * m.latent * 4,
                                 (size_t)(win.k1 - win.k0) * m.latent * 4, (size_t)rows, hipMemcpyDeviceToDevice, w.st));
    if (w.go()) EGR_HIP(hipGetLastError());
    return w.rc;
}

// quantiser and transposes over the whole-length ze_all [rows][F][latent]
int walk_encode_tail(Walk& w, float* ze_all, int64_t F, float* z, int* codes, float* ze_out) {
    Dac& m = w.m;
    float* z_cl = w.take((size_t)w.rows * F * m.latent);
    { const int rc = launch_vq(w, ze_all, z_cl, codes, F); if (rc) return rc; }
    if (w.go()) { const int rc = egr_transpose_batched(z_cl, z, w.rows, (int)F, m.latent, w.st); if (rc) return rc; }
    if (ze_out && w.go()) { const int rc = egr_transpose_batched(ze_all, ze_out, w.rows, (int)F, m.latent, w.st); if (rc) return rc; }
    if (w.go()) EGR_HIP(hipGetLastError());
    return w.rc;
}

// One pass: the window [0, F), every block output kept for egr_dac_stage.
int walk_encode(Walk& w, const float* x, int64_t n, float* z, int* codes) {
    int64_t F;
    lengths(w.m.cfg, n, nullptr, &F, nullptr);
    float* ze_all = w.take((size_t)w.rows * F * w.m.latent);
    { const int rc = walk_encode_window(w, x, n, EncWindow{0, F, 0, F, 0, F}, ze_all); if (rc) return rc; }
    return walk_encode_tail(w, ze_all, F, z, codes, nullptr);
}

// Segments of seg_frames frames (egr_dacseg_plan), one after the other on the stream through one arena behind the whole-length
// ze_all; the quantiser then runs once over ze_all, in the arena the windows have left.  `sizing`: lay out the largest window a
// segment of seg_frames can have instead (so that the arena depends on rows and seg_frames only), and the quantiser's buffers.
int walk_encode_segmented(Walk& w, const float* x, int64_t n, float* z, int* codes, float* ze_out, int64_t seg_frames, bool sizing) {
    Dac& m = w.m;
    int64_t F, hop = 1;
    lengths(m.cfg, n, nullptr, &F, nullptr);
    for (int i = 0; i < m.cfg.n_enc; ++i) hop *= m.cfg.enc_rates[i];
    float* ze_all = w.take((size_t)w.rows * F * m.latent);
    const size_t arena = w.off;
    size_t top = arena;
    if (sizing) {
        const int64_t Wmax = seg_window_max(m.cfg, EGR_DAC_ENCODE, seg_frames);
        walk_encode_window(w, nullptr, n, EncWindow{0, Wmax, 0, 1, 0, Wmax + 1}, nullptr);
        top = w.off;
    } else {
        int64_t nseg = 0;
        EGR_TRY(egr_dacseg_plan(&m.cfg, EGR_DAC_ENCODE, n, seg_frames, 0, nullptr, &nseg));
        for (int64_t j = 0; j < nseg; ++j) {
            egr_dac_segment sp;
            EGR_TRY(egr_dacseg_plan(&m.cfg, EGR_DAC_ENCODE, n, seg_frames, j, &sp, nullptr));
            w.off = arena;
            const EncWindow win{sp.win_lo * hop, sp.win_hi - sp.win_lo, sp.keep_lo - sp.win_lo, sp.keep_hi - sp.win_lo, sp.keep_lo, F};
            { const int rc = walk_encode_window(w, x, n, win, ze_all); if (rc) return rc; }
            top = std::max(top, w.off);
        }
    }
    w.off = arena;
    { const int rc = walk_encode_tail(w, ze_all, F, z, codes, ze_out); if (rc) return rc; }
    w.off = std::max(top, w.off);
    return w.rc;
}

int walk_quantize(Walk& w, const float* ze, int64_t F, float* z, int* codes) {
    Dac& m = w.m;
    float* ze_cl = w.take((size_t)w.rows * F * m.latent);
    float* z_cl = w.take((size_t)w.rows * F * m.latent);
    if (w.go()) { const int rc = egr_transpose_batched(ze, ze_cl, w.rows, m.latent, (int)F, w.st); if (rc) return rc; }
    { const int rc = launch_vq(w, ze_cl, z_cl, codes, F); if (rc) return rc; }
    if (w.go()) { const int rc = egr_transpose_batched(z_cl, z, w.rows, (int)F, m.latent, w.st); if (rc) return rc; }
    if (w.go()) EGR_HIP(hipGetLastError());
    return w.rc;
}

// A window of the decoder: `frames` latent frames from frame f0 of the whole-length channels-last z_all [rows][F][latent] (or, z_all
// null, the whole z [rows][latent][frames] as given: one pass).  Of the window's samples only [o0, o1) are stored, sample l at
// y0 + l of the whole y (rows ldy apart).
struct DecWindow { int64_t frames; const float* z_all; int64_t f0, F, o0, o1, y0, ldy; };

int walk_decode_window(Walk& w, const float* z, const DecWindow& win, float* y) {
    Dac& m = w.m;
    const egr_dac_config& c = m.cfg;
    const int rows = w.rows;
    const int64_t F = win.frames;
    w.amax_used = 0;
    w.amax_pool = (unsigned*)w.take((size_t)DAC_AMAX_SLOTS * rows * EGR_ROW_AMAX_STRIDE);
    if (w.go()) EGR_HIP(hipMemsetAsync(w.amax_pool, 0, (size_t)DAC_AMAX_SLOTS * rows * EGR_ROW_AMAX_STRIDE * 4, w.st));
    size_t mx = (size_t)rows * F * std::max(m.latent, c.decoder_dim), mxY = 0;
    {
        int64_t L = F;
        int C = c.decoder_dim;
        for (int i = 0; i < c.n_dec; ++i) {
            const int s = c.dec_rates[i];
            mx = std::max(mx, (size_t)rows * L * C);
            mxY = std::max(mxY, (size_t)rows * L * 2 * s * (C / 2));
            L = convtr_len(L, s);
            C /= 2;
            mx = std::max(mx, (size_t)rows * L * C);
        }
    }
    float* S[3] = {w.take(mx), w.take(mx), w.take(mx)};
    float* Y = w.take(mxY);
    int64_t L = F;
    float* z_cl = S[0];
    const unsigned* rz = w.amax_slot();
    if (w.go() && !win.z_all) { const int rc = egr_transpose_batched(z, z_cl, rows, m.latent, (int)F, w.st); if (rc) return rc; }
    if (w.go() && win.z_all)
        EGR_HIP(hipMemcpy2DAsync(z_cl, (size_t)F * m.latent * 4, win.z_all + (size_t)win.f0 * m.latent, (size_t)win.F * m.latent * 4, (size_t)F * m.latent * 4,
                                 (size_t)rows, hipMemcpyDeviceToDevice, w.st));
    if (w.go() && w.lens) {                              // level 0 of a many decode: each row's own frames
        const long long total = (long long)rows * F * m.latent;
        hipLaunchKernelGGL(k_dac_mask_frames, dim3((unsigned)std::min<long long>((total + 255) / 256, 8192)), dim3(256), 0, w.st, z_cl, w.lens, (long long)F, m.latent, total);
    }
    if (w.go()) { const int rc = egr_absmax_rows(z_cl, rows, F * m.latent, 1, 0, (float*)rz, w.st); if (rc) return rc; }
    int C = c.decoder_dim;
    float* cur = w.take((size_t)rows * L * C);
    w.conv(m.dec_in, z_cl, rz, cur, nullptr, m.dec_in.bias, L, L);
    w.note(EGR_DAC_STAGE_DEC, 0, cur, (int64_t)rows * L * C);
    for (int i = 0; i < c.n_dec; ++i) {
        const DecBlock& b = m.dec[i];
        float* a = other(S, cur);
        const unsigned* ra = w.snake(b.s, cur, a, L, i);
        // ConvTranspose1d: a GEMM onto [tap][co] columns of every input sample, gathered by egr_col2im_convtr1d
        if (w.go()) {
            ConvCall cc;
            cc.x = a; cc.y = Y; cc.B = (int)(rows * L); cc.Cin = b.up.Cin; cc.Cout = b.up.Cout;
            set_weight(cc, b.up.w, ra, rows);
            w.rc = conv_call(cc, w.st);
        }
        const int64_t Lo = convtr_len(L, b.stride);
        float* up = other(S, a);
        if (w.go()) w.rc = egr_col2im_convtr1d(Y, b.up.bias, nullptr, up, rows, (int)L, (int)Lo, b.c_out, b.k, b.stride, b.pad, w.st);
        cur = up; L = Lo; C = b.c_out;
        float* out = w.take((size_t)rows * L * C);
        for (int u = 0; u < 3; ++u) cur = run_res_unit(w, b.ru[u], cur, S, u == 2 ? out : nullptr, L, i + 1);
        w.note(EGR_DAC_STAGE_DEC, i + 1, cur, (int64_t)rows * L * C);
    }
    float* a = other(S, cur);
    w.snake(m.dec_s, cur, a, L, c.n_dec);
    const int64_t o0 = std::max<int64_t>(0, win.o0), o1 = std::min(L, win.o1);
    if (w.go() && o1 > o0) {
        hipLaunchKernelGGL(k_dac_conv_out, dim3((unsigned)((o1 - o0 + DAC_OUT_TL - 1) / DAC_OUT_TL), (unsigned)rows), dim3(256), 0, w.st, a, m.out_w, m.out_b, y,
                           (long long)L, C, (long long)o0, (long long)o1, (long long)win.y0, (long long)win.ldy);
        EGR_HIP(hipGetLastError());
    }
    return w.rc;
}

// One pass: the window [0, F), every block output kept for egr_dac_stage.
int walk_decode(Walk& w, const float* z, int64_t F, float* y) {
    const int64_t n_dec = decoded_len(w.m.cfg, F);
    return walk_decode_window(w, z, DecWindow{F, nullptr, 0, F, 0, n_dec, 0, n_dec}, y);
}

// z is transposed once into a whole-length channels-last buffer; every window copies its frame slice out of it.  `sizing` as in
// walk_encode_segmented.
int walk_decode_segmented(Walk& w, const float* z, int64_t F, float* y, int64_t seg_frames, bool sizing) {
    Dac& m = w.m;
    int64_t H = 1;
    for (int i = 0; i < m.cfg.n_dec; ++i) H *= m.cfg.dec_rates[i];
    const int64_t n_dec = decoded_len(m.cfg, F);
    float* z_all = w.take((size_t)w.rows * F * m.latent);
    const size_t arena = w.off;
    size_t top = arena;
    if (sizing) {
        const int64_t Wmax = seg_window_max(m.cfg, EGR_DAC_DECODE, seg_frames);
        walk_decode_window(w, nullptr, DecWindow{Wmax, nullptr, 0, Wmax, 0, 0, 0, 0}, nullptr);
        top = w.off;
    } else {
        if (w.go()) { const int rc = egr_transpose_batched(z, z_all, w.rows, m.latent, (int)F, w.st); if (rc) return rc; }
        int64_t nseg = 0;
        EGR_TRY(egr_dacseg_plan(&m.cfg, EGR_DAC_DECODE, F, seg_frames, 0, nullptr, &nseg));
        for (int64_t j = 0; j < nseg; ++j) {
            egr_dac_segment sp;
            EGR_TRY(egr_dacseg_plan(&m.cfg, EGR_DAC_DECODE, F, seg_frames, j, &sp, nullptr));
            w.off = arena;
            const int64_t base = sp.win_lo * H;                       // the whole-y position of the window's sample 0
            const DecWindow win{sp.win_hi - sp.win_lo, z_all, sp.win_lo, F, sp.out_lo - base, sp.out_hi - base, base, n_dec};
            { const int rc = walk_decode_window(w, nullptr, win, y); if (rc) return rc; }
            top = std::max(top, w.off);
        }
    }
    w.off = top;
    return w.rc;
}

int begin_call(Dac* m, const char* who, int rows, int64_t len) {
    EGR_CHECK(m && rows >= 1 && rows <= 65535 && len >= 1, EGR_ERR_ARG, "%s: bad argument", who);
    return check_current_device(who, m->device);
}

// One call: walk(w) lays the workspace out on a dry Walk (workspace_need), then enqueues the kernels on a launching one over the
// workspace grown to that
template <class F>
size_t workspace_need(Dac& m, int rows, F walk) {
    Walk dry{m, nullptr, false, rows};
    walk(dry);
    return dry.off + 256;
}
template <class F>
int run(Dac& m, int rows, hipStream_t st, F walk) {
    EGR_TRY(m.ws.grow(workspace_need(m, rows, walk), st));
    m.stages.clear();
    Walk w{m, st, true, rows};
    w.base = (char*)m.ws.p;
    return walk(w);
}

}  // namespace
}  // namespace egr

using namespace egr;

extern "C" int egr_dac_lengths(const egr_dac_config* cfg, int64_t n, int64_t* n_padded, int64_t* frames, int64_t* n_decoded) {
    { const int rc = check_config(cfg, "egr_dac_lengths"); if (rc) return rc; }
    EGR_CHECK(n >= 1, EGR_ERR_ARG, "egr_dac_lengths: n < 1");
    return lengths(*cfg, n, n_padded, frames, n_decoded);
}

extern "C" int egr_dac_create(void** handle, const egr_dac_config* cfg, const float* packed, int64_t n_floats, int device) {
    EGR_CHECK(handle && packed, EGR_ERR_ARG, "egr_dac_create: null argument");
    { const int rc = check_config(cfg, "egr_dac_create"); if (rc) return rc; }
    const egr_dac_config& c = *cfg;
    Dac* m = new Dac();
    m->cfg = c;
    m->device = device;
    m->latent = c.latent_dim;
    m->TF = vq_lds_bytes(c.codebook_size, c.codebook_dim, c.latent_dim, 8) <= (size_t)DAC_LDS_BUDGET ? 8 : 4;
    if (vq_lds_bytes(c.codebook_size, c.codebook_dim, c.latent_dim, m->TF) > (size_t)DAC_LDS_BUDGET) {
        set_error("egr_dac_create: the quantiser needs %zu bytes of LDS (limit %d)", vq_lds_bytes(c.codebook_size, c.codebook_dim, c.latent_dim, m->TF), DAC_LDS_BUDGET);
        delete m;
        return EGR_ERR_UNSUPPORTED;
    }
    Builder B{packed, n_floats};
    const int dils[3] = {1, 3, 9};
    // encoder
    {
        const int D = c.encoder_dim;
        const float* w = B.take((int64_t)D * 7);
        const float* b = B.take(D);
        if (w && b) {
            std::vector<float> wt((size_t)7 * D);
            for (int co = 0; co < D; ++co)
                for (int t = 0; t < 7; ++t) wt[(size_t)t * D + co] = w[(size_t)co * 7 + t];
            m->o_in_w = B.put(wt.data(), 7 * D);
            m->o_in_b = B.put(b, D);
        }
        m->enc.resize(c.n_enc);
        int C = D;
        for (int i = 0; i < c.n_enc && B.ok; ++i) {
            const int s = c.enc_rates[i];
            for (int u = 0; u < 3; ++u) res_unit(B, m->enc[i].ru[u], C, dils[u]);
            B.snake(m->enc[i].s, C);
            B.conv(m->enc[i].down, C, 2 * C, 2 * s, s, 1, (s + 1) / 2);
            C *= 2;
        }
        B.snake(m->enc_s, C);
        B.conv(m->enc_out, C, c.latent_dim, 3, 1, 1, 1);
    }
    // quantiser: in_proj transposed to [latent][cd], codebooks as stored and with unit rows (float64)
    {
        const int cd = c.codebook_dim, K = c.codebook_size, lat = c.latent_dim, n = c.n_codebooks;
        std::vector<float> in_w((size_t)n * lat * cd), in_b((size_t)n * cd), cbn((size_t)n * K * cd), cb((size_t)n * K * cd), out_w((size_t)n * lat * cd),
            out_b((size_t)n * lat);
        for (int i = 0; i < n && B.ok; ++i) {
            const float* iw = B.take((int64_t)cd * lat);
            const float* ib = B.take(cd);
            const float* cw = B.take((int64_t)K * cd);
            const float* ow = B.take((int64_t)lat * cd);
            const float* ob = B.take(lat);
            if (!B.ok) break;
            for (int j = 0; j < cd; ++j)
                for (int ch = 0; ch < lat; ++ch) in_w[((size_t)i * lat + ch) * cd + j] = iw[(size_t)j * lat + ch];
            std::copy(ib, ib + cd, in_b.begin() + (size_t)i * cd);
            std::copy(cw, cw + (size_t)K * cd, cb.begin() + (size_t)i * K * cd);
            for (int k = 0; k < K; ++k) {
                double s = 0.0;
                for (int j = 0; j < cd; ++j) s += (double)cw[(size_t)k * cd + j] * cw[(size_t)k * cd + j];
                const double inv = 1.0 / std::max(std::sqrt(s), 1e-12);
                for (int j = 0; j < cd; ++j) cbn[((size_t)i * K + k) * cd + j] = (float)(cw[(size_t)k * cd + j] * inv);
            }
            std::copy(ow, ow + (size_t)lat * cd, out_w.begin() + (size_t)i * lat * cd);
            std::copy(ob, ob + lat, out_b.begin() + (size_t)i * lat);
        }
        m->o_vq[0] = B.put(in_w.data(), in_w.size()); m->o_vq[1] = B.put(in_b.data(), in_b.size()); m->o_vq[2] = B.put(cbn.data(), cbn.size());
        m->o_vq[3] = B.put(cb.data(), cb.size()); m->o_vq[4] = B.put(out_w.data(), out_w.size()); m->o_vq[5] = B.put(out_b.data(), out_b.size());
    }
    // decoder
    {
        int C = c.decoder_dim;
        B.conv(m->dec_in, c.latent_dim, C, 7, 1, 1, 3);
        m->dec.resize(c.n_dec);
        for (int i = 0; i < c.n_dec && B.ok; ++i) {
            DecBlock& d = m->dec[i];
            const int s = c.dec_rates[i];
            d.k = 2 * s; d.stride = s; d.pad = (s + 1) / 2; d.c_out = C / 2;
            B.snake(d.s, C);
            B.convtr(d.up, C, C / 2, 2 * s);
            C /= 2;
            for (int u = 0; u < 3; ++u) res_unit(B, d.ru[u], C, dils[u]);
        }
        B.snake(m->dec_s, C);
        m->c_last = C;
        const float* w = B.take((int64_t)C * 7);
        const float* b = B.take(1);
        if (w && b) {
            std::vector<float> wt((size_t)7 * C);
            for (int ci = 0; ci < C; ++ci)
                for (int t = 0; t < 7; ++t) wt[(size_t)t * C + ci] = w[(size_t)ci * 7 + t];
            m->o_out_w = B.put(wt.data(), 7 * C);
            m->o_out_b = B.put(b, 1);
        }
    }
    if (!B.ok || B.pos != n_floats) {
        set_error("egr_dac_create: the packed weights hold %lld floats, the config describes %s%lld", (long long)n_floats, B.ok ? "" : "more than ",
                  (long long)B.pos);
        delete m;
        return EGR_ERR_ARG;
    }
    int rc = EGR_OK;
    {
        DeviceScope dev(device);
        if (!dev.ok) {
            set_error("egr_dac_create: cannot select device %d", device);
            delete m;
            return EGR_ERR_HIP;
        }
        rc = upload(m, B, packed, n_floats);
        if (rc == EGR_OK) {
            hipError_t e = hipFuncSetAttribute((const void*)k_dac_vq<8>, hipFuncAttributeMaxDynamicSharedMemorySize, DAC_LDS_MAX);
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_dac_vq<0>, hipFuncAttributeMaxDynamicSharedMemorySize, DAC_LDS_MAX);
            if (e != hipSuccess) { set_error("egr_dac_create: hipFuncSetAttribute(MaxDynamicSharedMemorySize) -> %s", hipGetErrorString(e)); rc = EGR_ERR_HIP; }
        }
    }
    if (rc) { destroy(m); return rc; }
    // bind the tables
    const float* D = m->d_misc;
    auto bind_snake = [&](Snake& s) { s.alpha = D + s.o; s.inva = D + ((s.o + s.C + 3) & ~(size_t)3); };
    auto bind_ru = [&](ResUnit& u) { bind_snake(u.s1); bind_snake(u.s2); };
    m->in_w = D + m->o_in_w; m->in_b = D + m->o_in_b;
    for (auto& b : m->enc) { for (auto& u : b.ru) bind_ru(u); bind_snake(b.s); }
    bind_snake(m->enc_s);
    for (auto& b : m->dec) { for (auto& u : b.ru) bind_ru(u); bind_snake(b.s); }
    bind_snake(m->dec_s);
    m->out_w = D + m->o_out_w; m->out_b = D + m->o_out_b;
    m->vq.in_w = D + m->o_vq[0]; m->vq.in_b = D + m->o_vq[1]; m->vq.cbn = D + m->o_vq[2]; m->vq.cb = D + m->o_vq[3];
    m->vq.out_w = D + m->o_vq[4]; m->vq.out_b = D + m->o_vq[5];
    m->vq.latent = c.latent_dim; m->vq.cd = c.codebook_dim; m->vq.K = c.codebook_size; m->vq.ncb = c.n_codebooks;
    *handle = m;
    return EGR_OK;
}

extern "C" int egr_dac_set_stages(void* handle, int enable) {
    EGR_CHECK(handle, EGR_ERR_ARG, "egr_dac_set_stages: null handle");
    ((Dac*)handle)->keep_vq_inputs = enable != 0;
    return EGR_OK;
}

extern "C" int egr_dac_destroy(void* handle) {
    if (handle) destroy((Dac*)handle);
    return EGR_OK;
}

extern "C" size_t egr_dac_workspace_bytes(void* handle, int rows, int64_t n) {
    Dac* m = (Dac*)handle;
    if (!m || rows < 1 || n < 1) return 0;
    int64_t F = 0;
    lengths(m->cfg, n, nullptr, &F, nullptr);
    if (F < 1) return 0;
    return std::max(workspace_need(*m, rows, [&](Walk& w) { return walk_encode(w, nullptr, n, nullptr, nullptr); }),
                    workspace_need(*m, rows, [&](Walk& w) { return walk_decode(w, nullptr, F, nullptr); }));
}

extern "C" int egr_dac_encode(void* handle, const float* x, int rows, int64_t n, float* z, int* codes, void* stream) {
    Dac* m = (Dac*)handle;
    { const int rc = begin_call(m, "egr_dac_encode", rows, n); if (rc) return rc; }
    EGR_CHECK(x && z && codes, EGR_ERR_ARG, "egr_dac_encode: null argument");
    int64_t n_pad, F;
    lengths(m->cfg, n, &n_pad, &F, nullptr);
    EGR_CHECK(F >= 1, EGR_ERR_ARG, "egr_dac_encode: no frames");
    EGR_CHECK((long long)rows * n_pad < (1LL << 31), EGR_ERR_UNSUPPORTED, "egr_dac_encode: rows * padded length = %lld does not index with an int (egr_dacseg_encode takes it)",
              (long long)rows * n_pad);
    return run(*m, rows, (hipStream_t)stream, [&](Walk& w) { return walk_encode(w, x, n, z, codes); });
}

extern "C" int egr_dac_quantize(void* handle, const float* ze, int rows, int64_t frames, float* z, int* codes, void* stream) {
    Dac* m = (Dac*)handle;
    { const int rc = begin_call(m, "egr_dac_quantize", rows, frames); if (rc) return rc; }
    EGR_CHECK(ze && z && codes, EGR_ERR_ARG, "egr_dac_quantize: null argument");
    EGR_CHECK((long long)rows * frames < (1LL << 31) / 32 && frames < (1LL << 31), EGR_ERR_UNSUPPORTED, "egr_dac_quantize: too many frames for one pass");
    return run(*m, rows, (hipStream_t)stream, [&](Walk& w) { return walk_quantize(w, ze, frames, z, codes); });
}

extern "C" int egr_dac_decode(void* handle, const float* z, int rows, int64_t frames, float* y, void* stream) {
    Dac* m = (Dac*)handle;
    { const int rc = begin_call(m, "egr_dac_decode", rows, frames); if (rc) return rc; }
    EGR_CHECK(z && y, EGR_ERR_ARG, "egr_dac_decode: null argument");
    const int64_t n_dec = decoded_len(m->cfg, frames);
    EGR_CHECK(n_dec >= 1, EGR_ERR_ARG, "egr_dac_decode: %lld frames decode to nothing", (long long)frames);
    EGR_CHECK((long long)rows * n_dec < (1LL << 31), EGR_ERR_UNSUPPORTED, "egr_dac_decode: rows * decoded length = %lld does not index with an int (egr_dacseg_decode takes it)",
              (long long)rows * n_dec);
    return run(*m, rows, (hipStream_t)stream, [&](Walk& w) { return walk_decode(w, z, frames, y); });
}

extern "C" int egr_dacseg_plan(const egr_dac_config* cfg, int kind, int64_t length, int64_t seg_frames, int64_t index, egr_dac_segment* seg,
                                    int64_t* n_segments) {
    { const int rc = check_config(cfg, "egr_dacseg_plan"); if (rc) return rc; }
    EGR_CHECK((kind == EGR_DAC_ENCODE || kind == EGR_DAC_DECODE) && length >= 1 && seg_frames >= 1, EGR_ERR_ARG, "egr_dacseg_plan: bad argument");
    const egr_dac_config& c = *cfg;
    for (int i = 0; i < c.n_enc; ++i) EGR_CHECK(c.enc_rates[i] >= 2, EGR_ERR_UNSUPPORTED, "egr_dacseg_plan: an encoder rate of 1 is not cut into segments");
    for (int i = 0; i < c.n_dec; ++i) EGR_CHECK(c.dec_rates[i] >= 2, EGR_ERR_UNSUPPORTED, "egr_dacseg_plan: a decoder rate of 1 is not cut into segments");
    int64_t F = length, n_dec = 0, per = 1;              // per: samples a frame, of x (encode) or of y (decode)
    if (kind == EGR_DAC_ENCODE) {
        lengths(c, length, nullptr, &F, nullptr);
        for (int i = 0; i < c.n_enc; ++i) per *= c.enc_rates[i];
    } else {
        n_dec = decoded_len(c, F);
        for (int i = 0; i < c.n_dec; ++i) per *= c.dec_rates[i];
    }
    EGR_CHECK(F >= 1, EGR_ERR_ARG, "egr_dacseg_plan: no frames");
    const int64_t nseg = (F + seg_frames - 1) / seg_frames;
    if (n_segments) *n_segments = nseg;
    if (!seg) return EGR_OK;
    EGR_CHECK(index >= 0 && index < nseg, EGR_ERR_ARG, "egr_dacseg_plan: segment %lld of %lld", (long long)index, (long long)nseg);
    int64_t ml, mr;
    seg_margins(c, kind, &ml, &mr);
    egr_dac_segment s;
    s.keep_lo = index * seg_frames;
    s.keep_hi = std::min(F, s.keep_lo + seg_frames);
    s.win_lo = std::max<int64_t>(0, s.keep_lo - ml);
    s.win_hi = std::min(F, s.keep_hi + mr);
    int64_t extra = (DAC_SEG_ALIGN - (s.win_hi - s.win_lo) % DAC_SEG_ALIGN) % DAC_SEG_ALIGN;     // widen: left first, then right
    const int64_t tl = std::min(extra, s.win_lo);
    s.win_lo -= tl;
    extra -= tl;
    s.win_hi += std::min(extra, F - s.win_hi);
    if (kind == EGR_DAC_ENCODE) {
        s.in_lo = s.win_lo * per;
        s.in_hi = std::min(length, s.win_hi * per);
        s.out_lo = s.keep_lo;
        s.out_hi = s.keep_hi;
    } else {
        s.in_lo = s.win_lo;
        s.in_hi = s.win_hi;
        s.out_lo = std::min(n_dec, s.keep_lo * per);
        s.out_hi = index == nseg - 1 ? n_dec : std::min(n_dec, s.keep_hi * per);
    }
    *seg = s;
    return EGR_OK;
}

namespace {
// the largest seg_frames whose widest window still indexes with an int (rows * window samples), 0 when none does
int64_t seg_frames_cap(const egr_dac_config& c, int kind, int rows) {
    int64_t per = 1, ml, mr;
    if (kind == EGR_DAC_ENCODE) for (int i = 0; i < c.n_enc; ++i) per *= c.enc_rates[i];
    else for (int i = 0; i < c.n_dec; ++i) per *= c.dec_rates[i];
    seg_margins(c, kind, &ml, &mr);
    return std::max<int64_t>(0, ((1LL << 31) - 1) / ((int64_t)rows * per) - ml - mr - DAC_SEG_ALIGN);
}
int64_t clamp_seg_frames(const egr_dac_config& c, int kind, int rows, int64_t seg_frames, int64_t F) {
    return std::min(std::min(seg_frames, F), seg_frames_cap(c, kind, rows));       // (more than F frames a segment is one window)
}
template <class F>
int run_segmented(Dac& m, int rows, hipStream_t st, F walk) {
    Walk dry{m, nullptr, false, rows};
    dry.notes = false;
    { const int rc = walk(dry, true); if (rc) return rc; }
    EGR_TRY(m.ws.grow(dry.off + 256, st));
    m.stages.clear();                                    // no stage survives a segmented call: egr_dac_stage then refuses
    Walk w{m, st, true, rows};
    w.notes = false;
    w.base = (char*)m.ws.p;
    return walk(w, false);
}
}  // namespace

extern "C" size_t egr_dacseg_workspace_bytes(void* handle, int rows, int64_t seg_frames, int64_t n, int kind) {
    Dac* m = (Dac*)handle;
    if (!m || rows < 1 || rows > 65535 || n < 1 || seg_frames < 1 || (kind != EGR_DAC_ENCODE && kind != EGR_DAC_DECODE)) return 0;
    int64_t F = 0;
    lengths(m->cfg, n, nullptr, &F, nullptr);
    if (F < 1) return 0;
    const int64_t S = std::min(seg_frames, seg_frames_cap(m->cfg, kind, rows));     // (not clamped to F: the arena depends on rows and seg_frames only)
    if (S < 1) return 0;
    Walk dry{*m, nullptr, false, rows};
    dry.notes = false;
    if (kind == EGR_DAC_ENCODE) walk_encode_segmented(dry, nullptr, n, nullptr, nullptr, nullptr, S, true);
    else walk_decode_segmented(dry, nullptr, F, nullptr, S, true);
    return dry.rc ? 0 : dry.off + 256;
}

extern "C" size_t egr_dacseg_workspace_held(void* handle) { return handle ? ((Dac*)handle)->ws.bytes : 0; }

extern "C" int egr_dacseg_encode(void* handle, const float* x, int rows, int64_t n, float* z, int* codes, float* ze_or_null, int64_t seg_frames,
                                        void* stream) {
    Dac* m = (Dac*)handle;
    { const int rc = begin_call(m, "egr_dacseg_encode", rows, n); if (rc) return rc; }
    EGR_CHECK(x && z && codes, EGR_ERR_ARG, "egr_dacseg_encode: null argument");
    EGR_CHECK(seg_frames >= 1, EGR_ERR_ARG, "egr_dacseg_encode: seg_frames < 1");
    int64_t F;
    lengths(m->cfg, n, nullptr, &F, nullptr);
    EGR_CHECK(F >= 1, EGR_ERR_ARG, "egr_dacseg_encode: no frames");
    EGR_CHECK((long long)rows * F < (1LL << 31) / 32, EGR_ERR_UNSUPPORTED, "egr_dacseg_encode: rows * frames = %lld is more than the quantiser indexes",
              (long long)rows * F);
    const int64_t S = clamp_seg_frames(m->cfg, EGR_DAC_ENCODE, rows, seg_frames, F);
    EGR_CHECK(S >= 1, EGR_ERR_UNSUPPORTED, "egr_dacseg_encode: %d rows leave no window that indexes with an int", rows);
    return run_segmented(*m, rows, (hipStream_t)stream, [&](Walk& w, bool sizing) { return walk_encode_segmented(w, x, n, z, codes, ze_or_null, S, sizing); });
}

extern "C" int egr_dacseg_decode(void* handle, const float* z, int rows, int64_t frames, float* y, int64_t seg_frames, void* stream) {
    Dac* m = (Dac*)handle;
    { const int rc = begin_call(m, "egr_dacseg_decode", rows, frames); if (rc) return rc; }
    EGR_CHECK(z && y, EGR_ERR_ARG, "egr_dacseg_decode: null argument");
    EGR_CHECK(seg_frames >= 1, EGR_ERR_ARG, "egr_dacseg_decode: seg_frames < 1");
    const int64_t F = frames, n_dec = decoded_len(m->cfg, F);
    EGR_CHECK(n_dec >= 1, EGR_ERR_ARG, "egr_dacseg_decode: %lld frames decode to nothing", (long long)frames);
    EGR_CHECK(F < (1LL << 31), EGR_ERR_UNSUPPORTED, "egr_dacseg_decode: %lld frames are more than the transpose indexes", (long long)F);
    const int64_t S = clamp_seg_frames(m->cfg, EGR_DAC_DECODE, rows, seg_frames, F);
    EGR_CHECK(S >= 1, EGR_ERR_UNSUPPORTED, "egr_dacseg_decode: %d rows leave no window that indexes with an int", rows);
    return run_segmented(*m, rows, (hipStream_t)stream, [&](Walk& w, bool sizing) { return walk_decode_segmented(w, z, F, y, S, sizing); });
}

extern "C" int egr_dacseg_from_codes(void* handle, const int* codes, int rows, int64_t frames, float* z, void* stream) {
    Dac* m = (Dac*)handle;
    { const int rc = begin_call(m, "egr_dacseg_from_codes", rows, frames); if (rc) return rc; }
    EGR_CHECK(codes && z, EGR_ERR_ARG, "egr_dacseg_from_codes: null argument");
    EGR_CHECK((frames + 255) / 256 < (1LL << 31), EGR_ERR_UNSUPPORTED, "egr_dacseg_from_codes: too many frames");
    VqP p = m->vq;
    p.codes = (int*)codes; p.z = z; p.F = frames; p.total = (long long)rows * frames;
    const dim3 grid((unsigned)((frames + 255) / 256), (unsigned)((m->latent + DAC_FC_CH - 1) / DAC_FC_CH), (unsigned)rows);
    if (p.cd == 8) hipLaunchKernelGGL(k_dac_from_codes<8>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(k_dac_from_codes<0>, grid, dim3(256), 0, (hipStream_t)stream, p);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

// ---- many clips in one padded pass: rows of their own lengths inside tensors of the longest
namespace {
struct ManyShape { int64_t P = 0, L = 0; size_t table_bytes = 0; };      // padded frames, padded samples (x for encode, y for decode)

// every refusal of a many call that depends on (rows, pad_frames, kind) alone
int many_shape(const Dac* m, const char* who, int rows, int64_t pad_frames, int kind, ManyShape* out) {
    EGR_CHECK(m, EGR_ERR_ARG, "%s: null handle", who);
    EGR_CHECK(kind == EGR_DAC_ENCODE || kind == EGR_DAC_DECODE, EGR_ERR_ARG, "%s: kind %d", who, kind);
    EGR_CHECK(rows >= 1 && rows <= 65535, EGR_ERR_ARG, "%s: rows = %d outside 1 .. 65535", who, rows);
    EGR_CHECK(pad_frames >= 1, EGR_ERR_ARG, "%s: pad_frames = %lld < 1", who, (long long)pad_frames);
    EGR_CHECK(pad_frames <= (1LL << 26) / rows, EGR_ERR_UNSUPPORTED, "%s: rows * pad_frames = %lld * %lld is more than the quantiser indexes (2^26)", who,
              (long long)rows, (long long)pad_frames);
    const egr_dac_config& c = m->cfg;
    ManyShape s;
    s.P = pad_frames;
    if (kind == EGR_DAC_ENCODE) {
        s.L = pad_frames;
        for (int i = 0; i < c.n_enc; ++i) s.L *= c.enc_rates[i];
        int64_t F = s.L;
        for (int i = 0; i < c.n_enc; ++i) F = conv_len(F, c.enc_rates[i]);
        EGR_CHECK(F == pad_frames, EGR_ERR_UNSUPPORTED, "%s: pad_frames = %lld frames of samples encode to %lld frames", who, (long long)pad_frames, (long long)F);
        s.table_bytes = (size_t)rows * 2 * sizeof(int64_t) + (size_t)(c.n_enc + 1) * rows * sizeof(int);
    } else {
        s.L = decoded_len(c, pad_frames);
        EGR_CHECK(s.L >= 1, EGR_ERR_ARG, "%s: pad_frames = %lld frames decode to nothing", who, (long long)pad_frames);
        s.table_bytes = (size_t)(c.n_dec + 1) * rows * sizeof(int);
    }
    EGR_CHECK((long long)rows * s.L < (1LL << 31), EGR_ERR_UNSUPPORTED, "%s: rows * padded samples = %lld does not index with an int (pad_frames too large)", who,
              (long long)rows * s.L);
    *out = s;
    return EGR_OK;
}

// The tables go up with one copy from the handle's pinned memory (filled by the caller), then the window [0, P) runs with them bound.
int bind_tables(Walk& w, const ManyShape& s, char** tab) {
    *tab = (char*)w.take((s.table_bytes + 3) / 4);
    if (!w.go()) return w.rc;
    return w.m.tables.upload(*tab, s.table_bytes, w.st);        // one copy for all tables
}

int walk_many_encode(Walk& w, const float* x, const ManyShape& s, float* z, int* codes, float* ze_out) {
    char* tab = nullptr;
    EGR_TRY(bind_tables(w, s, &tab));
    if (w.go()) { w.xrows = (const long long*)tab; w.lens = (const int*)(tab + (size_t)w.rows * 2 * sizeof(int64_t)); }
    float* ze_all = w.take((size_t)w.rows * s.P * w.m.latent);
    { const int rc = walk_encode_window(w, x, 0, EncWindow{0, s.P, 0, s.P, 0, s.P}, ze_all); if (rc) return rc; }
    return walk_encode_tail(w, ze_all, s.P, z, codes, ze_out);
}

int walk_many_decode(Walk& w, const float* z, const ManyShape& s, float* y) {
    char* tab = nullptr;
    EGR_TRY(bind_tables(w, s, &tab));
    if (w.go()) w.lens = (const int*)tab;
    return walk_decode_window(w, z, DecWindow{s.P, nullptr, 0, s.P, 0, s.L, 0, s.L}, y);
}

// as run_segmented: no stage survives; the tables live in the Walk, so the handle carries nothing into the next call
template <class F>
int run_many(Dac& m, int rows, hipStream_t st, F walk) {
    Walk dry{m, nullptr, false, rows};
    dry.notes = false;
    { const int rc = walk(dry); if (rc) return rc; }
    EGR_TRY(m.ws.grow(dry.off + 256, st));
    m.stages.clear();
    Walk w{m, st, true, rows};
    w.notes = false;
    w.base = (char*)m.ws.p;
    return walk(w);
}
}  // namespace

extern "C" size_t egr_dacmany_workspace_bytes(void* handle, int rows, int64_t pad_frames, int kind) {
    Dac* m = (Dac*)handle;
    ManyShape s;
    if (many_shape(m, "egr_dacmany_workspace_bytes", rows, pad_frames, kind, &s)) return 0;
    Walk dry{*m, nullptr, false, rows};
    dry.notes = false;
    if (kind == EGR_DAC_ENCODE) walk_many_encode(dry, nullptr, s, nullptr, nullptr, nullptr);
    else walk_many_decode(dry, nullptr, s, nullptr);
    return dry.rc ? 0 : dry.off + 256;
}

extern "C" int egr_dacmany_encode(void* handle, const float* x_flat, const int64_t* rows_host, int rows, int64_t pad_frames, float* z, int* codes,
                                  float* ze_or_null, void* stream) {
    const char* who = "egr_dacmany_encode";
    Dac* m = (Dac*)handle;
    ManyShape s;
    EGR_TRY(many_shape(m, who, rows, pad_frames, EGR_DAC_ENCODE, &s));
    EGR_CHECK(x_flat && rows_host && z && codes, EGR_ERR_ARG, "%s: null argument", who);
    const egr_dac_config& c = m->cfg;
    for (int r = 0; r < rows; ++r) {
        const int64_t off = rows_host[2 * r], n = rows_host[2 * r + 1];
        EGR_CHECK(off >= 0, EGR_ERR_ARG, "%s: row %d has a negative offset (%lld)", who, r, (long long)off);
        EGR_CHECK(n >= 1, EGR_ERR_ARG, "%s: row %d has n = %lld < 1", who, r, (long long)n);
        int64_t F;
        lengths(c, n, nullptr, &F, nullptr);
        EGR_CHECK(F >= 1 && F <= pad_frames, EGR_ERR_ARG, "%s: pad_frames = %lld is below row %d (n = %lld samples, %lld frames)", who, (long long)pad_frames, r,
                  (long long)n, (long long)F);
    }
    EGR_TRY(check_current_device(who, m->device));
    EGR_TRY(m->tables.reserve(s.table_bytes));
    int64_t* xr = (int64_t*)m->tables.p;
    int* lens = (int*)(xr + (size_t)rows * 2);
    for (int r = 0; r < rows; ++r) {
        xr[2 * r] = rows_host[2 * r];
        xr[2 * r + 1] = rows_host[2 * r + 1];
        int64_t L;
        lengths(c, rows_host[2 * r + 1], &L, nullptr, nullptr);
        for (int i = 0; i <= c.n_enc; ++i) {
            lens[(size_t)i * rows + r] = (int)L;
            if (i < c.n_enc) L = conv_len(L, c.enc_rates[i]);
        }
    }
    return run_many(*m, rows, (hipStream_t)stream, [&](Walk& w) { return walk_many_encode(w, x_flat, s, z, codes, ze_or_null); });
}

extern "C" int egr_dacmany_decode(void* handle, const float* z, const int64_t* frames_host, int rows, int64_t pad_frames, float* y, void* stream) {
    const char* who = "egr_dacmany_decode";
    Dac* m = (Dac*)handle;
    ManyShape s;
    EGR_TRY(many_shape(m, who, rows, pad_frames, EGR_DAC_DECODE, &s));
    EGR_CHECK(z && frames_host && y, EGR_ERR_ARG, "%s: null argument", who);
    const egr_dac_config& c = m->cfg;
    for (int r = 0; r < rows; ++r) {
        EGR_CHECK(frames_host[r] >= 1, EGR_ERR_ARG, "%s: row %d has frames = %lld < 1", who, r, (long long)frames_host[r]);
        EGR_CHECK(frames_host[r] <= pad_frames, EGR_ERR_ARG, "%s: pad_frames = %lld is below row %d (%lld frames)", who, (long long)pad_frames, r,
                  (long long)frames_host[r]);
        EGR_CHECK(decoded_len(c, frames_host[r]) >= 1, EGR_ERR_ARG, "%s: row %d: %lld frames decode to nothing", who, r, (long long)frames_host[r]);
    }
    EGR_TRY(check_current_device(who, m->device));
    EGR_TRY(m->tables.reserve(s.table_bytes));
    int* lens = (int*)m->tables.p;
    for (int r = 0; r < rows; ++r) {
        int64_t L = frames_host[r];
        for (int i = 0; i <= c.n_dec; ++i) {
            lens[(size_t)i * rows + r] = (int)L;
            if (i < c.n_dec) L = convtr_len(L, c.dec_rates[i]);
        }
    }
    return run_many(*m, rows, (hipStream_t)stream, [&](Walk& w) { return walk_many_decode(w, z, s, y); });
}

extern "C" int egr_dac_stage(void* handle, int stage, int index, float* dst, int64_t capacity, int64_t* count, void* stream) {
    Dac* m = (Dac*)handle;
    EGR_CHECK(m && count, EGR_ERR_ARG, "egr_dac_stage: null argument");
    for (const StageRec& s : m->stages)
        if (s.kind == stage && s.index == index) return stage_copy_out("egr_dac_stage", s.p, s.count, dst, capacity, count, stream);
    set_error("egr_dac_stage: the last call left no stage (%d, %d)", stage, index);
    return EGR_ERR_ARG;
}
