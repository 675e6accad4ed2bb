// Fat-Llama iterative spectral enhancer on MI355X (gfx950).
//
// Replaces upstream fat_llama.audio_fattener.feed.upscale as called from the reference at
// egregora_fat_llama_gpu.py:213-224 / egregora_fat_llama_cpu.py:126-134 (see include/egregora_amd.h).
//
// Data layout in HBM (per plan; C channels, N = n_in*factor real samples, M = N/2 = M1*M2):
//   out  [C][N]  float   holds y (the up-rated signal) during the loop, the final result afterwards
//   work [C][M]  float2  the loop state, updated IN PLACE by both loop kernels:
//                          after k_col : A[k1][n2]  (column FFT over n1 done, four-step twiddle applied)
//                          after k_row : B[k1][n2]  (half-spectrum thresholded, row IFFT over k2 done)
// One loop iteration = k_row (FFT_M2 . real-split . threshold . un-split . IFFT_M2 on the row pair
// (k1, M1-k1), all in LDS) followed by k_col (twiddle^-1 . IFFT_M1 . [time domain] . FFT_M1 . twiddle on a
// tile of TC adjacent columns, all in LDS).  Each launch reads 4N and writes 4N bytes per channel; the
// spectrum is never materialised in natural order and nothing is transposed.
// Long inputs add a third factor (state [M1][M2][M3], inner column pass k_col<3>/<4>); lengths without a packed
// plan (odd, large primes) run the chirp-z path further down (k_colz, k_rowconv); egr_spectral_gain reuses the
// passes as a zero-phase filter.  DESIGN.md section 2 has the derivations.
// the register butterflies of this translation unit (packed-real loop kernels) carry their cos / sin constants as two floats: a rounded
// constant is a gain the 800-iteration loop applies in the same direction every iteration (egr_fft_device.h, egr_fatllama_wl.h EGR_WL_HILO)
#ifndef EGR_BFLY_HILO
#define EGR_BFLY_HILO 15
#endif
#include "egr_fatllama_int.h"
#include "egr_null_index.h"

namespace egr {

// MODE 0: first  (y -> time threshold -> FFT -> twiddle -> state)          [outermost pass only]
// MODE 1: middle  (state -> twiddle^-1 -> IFFT -> FFT -> twiddle -> state)  [outermost pass only]
// MODE 2: last    (state -> twiddle^-1 -> IFFT -> out = y + d, peak)        [outermost pass only]
// MODE 3: inverse (state -> twiddle^-1 -> IFFT -> state)                    [inner pass of a 3-level plan]
// MODE 4: forward (state -> FFT -> twiddle -> state)                        [inner pass of a 3-level plan]
// MODE 5: last, plain (state -> twiddle^-1 -> IFFT -> out = d)               [spectral-gain filter]
// thr_rel (MODE 0 only, optional): per-channel max|y| as float bits; the time-domain level becomes thr * max|y| (SPEC.md section 3).
// SCHED 0: run-time radix schedule (any plan).  SCHED 2: L = 625 as 25 x 25 with compile-time stages (egr_fft_device.h).
// The compile-time schedules run IN PLACE (one buffer, two barriers per stage): half the LDS of the ping-pong form, so that
// three 512-thread workgroups share a CU (6 waves per SIMD) and the two channels' kernels are fully resident together.
// rows of the in-place 2304-point schedule are stored with one pad element per 16 (lds_pad): conflict-free first-stage writes
#ifndef EGR_FL_ROW_PAD
#define EGR_FL_ROW_PAD 4
#endif
// radix schedules of the two hot lengths (each a product of up to five radices with a register butterfly)
#ifndef EGR_FL_ROW_RADICES
#define EGR_FL_ROW_RADICES 16, 12, 12
#endif
// column tile of the 625-point schedule: columns per workgroup (64-byte = 8, 32-byte = 4 segments per row) and workgroup size
#ifndef EGR_FL_COL_TC
#define EGR_FL_COL_TC 4
#endif
#ifndef EGR_FL_COL_THREADS
#define EGR_FL_COL_THREADS 512
#endif
#ifndef EGR_FL_COL_RADICES
#define EGR_FL_COL_RADICES 25, 25
#endif
// pad of the chirp-z row kernel's LDS rows (0: dense)
#ifndef EGR_FL_CONV_PAD
#define EGR_FL_CONV_PAD 0
#endif
// rows per workgroup and workgroup size of k_rowconv (in place: rows * L <= 8 * threads)
#ifndef EGR_FL_CONV_ROWS
#define EGR_FL_CONV_ROWS 1
#endif
#ifndef EGR_FL_CONV_THREADS
#define EGR_FL_CONV_THREADS 512
#endif
#ifndef EGR_FL_COL_STW_LDS
#define EGR_FL_COL_STW_LDS 1
#endif
#ifndef EGR_FL_SCHED_WAVES
#define EGR_FL_SCHED_WAVES 6
#endif
template <int SCHED>
__device__ __forceinline__ void col_fft(cplx*& cur, cplx*& alt, const ColP& p, int TC, int lg, bool inverse, const cplx* stw) {
    if (SCHED == 2) lds_fft_sched_inplace<true, 0, 625 * EGR_FL_COL_TC, EGR_FL_COL_THREADS, EGR_FL_COL_RADICES>(cur, p.L, stw, TC, lg, TC, 1, inverse);
    else lds_fft<true>(cur, alt, p.f, p.tw, TC, lg, TC, 1, inverse, p.twd);
}

template <int MODE, int SCHED = 0>
__global__ __launch_bounds__(SCHED ? 512 : 1024, SCHED ? EGR_FL_SCHED_WAVES : 1) void k_col(ColP p, long long M, long long N, float thr, cplx* __restrict__ work,
                                              float* __restrict__ out, unsigned* __restrict__ peak_out,
                                              const unsigned* __restrict__ thr_rel = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    EGR_LDS_CANARY_ARM(smem);
    __shared__ float red[16];
    // XCD-aware tile order: the dispatcher places block b on XCD b%8; give every XCD a contiguous run
    // of column tiles so the two tiles sharing a 128-byte line hit the same L2.
    const int tile = (blockIdx.x & 7) * p.tiles_per_xcd + (blockIdx.x >> 3);
    if (tile >= p.ntiles) return;
    const int ch = blockIdx.y / p.nplanes, plane = blockIdx.y - ch * p.nplanes;
    const int TC = p.TC, lg = p.TClog2, L = p.L, nc = p.ncols;
    const int c0 = tile * TC;
    cplx* cur = (cplx*)EGR_LDS_BASE(smem);
    cplx* alt = cur + (size_t)L * TC;
    const size_t poff = (size_t)plane * L * nc;
    cplx* W = work + (size_t)ch * M + poff;
    float2* Y = (float2*)(out + (size_t)ch * N) + poff;
    const int nel = L * TC;
    if (MODE == 0 && thr_rel) thr *= __uint_as_float(thr_rel[ch]);
    // the 25 x 26 stage-twiddle table of the 25 25 schedule is copied into LDS (5.2 KB): its reads then cost an LDS round trip
    constexpr int col_radices[] = {EGR_FL_COL_RADICES};
    static_assert(!EGR_FL_COL_STW_LDS || (sizeof(col_radices) / sizeof(int) == 2 && col_radices[0] == 25 && col_radices[1] == 25),
                  "the LDS copy of the stage table is sized for the 25 25 schedule");
    __shared__ cplx stw_lds[(SCHED == 2 && EGR_FL_COL_STW_LDS) ? 25 * 26 : 1];
    const cplx* stw = p.stw;
    if (SCHED == 2 && EGR_FL_COL_STW_LDS) {
        for (int e = threadIdx.x; e < 25 * 26; e += blockDim.x) stw_lds[e] = p.stw[e];
        stw = stw_lds;
    }
    EGR_STAMP(p, 0);

    // scheduled mid pass on full tiles: two adjacent columns per thread and step -- 16-byte state loads / stores and LDS accesses,
    // half the memory instructions of the element-wise loops below
    const bool pairwise = MODE == 1 && SCHED == 2 && c0 + TC <= nc;
    if (pairwise) {
        for (int e = 2 * threadIdx.x; e < nel; e += 2 * blockDim.x) {
            const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
            const float4 w2 = *(const float4*)(W + (size_t)i * nc + col);
            const cplx a = cmulc(make_float2(w2.x, w2.y), tw2(p.big, (unsigned)col * (unsigned)i));
            const cplx b = cmulc(make_float2(w2.z, w2.w), tw2(p.big, (unsigned)(col + 1) * (unsigned)i));
            *(float4*)(cur + e) = make_float4(a.x, a.y, b.x, b.y);
        }
    } else
    for (int e = threadIdx.x; e < nel; e += blockDim.x) {
        const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
        cplx v = make_float2(0.f, 0.f);
        if (col < nc) {
            const size_t g = (size_t)i * nc + col;
            if (MODE == 0) {
                const float2 y = Y[g];
                v.x = fabsf(y.x) > thr ? y.x : 0.f;
                v.y = fabsf(y.y) > thr ? y.y : 0.f;
            } else if (MODE == 4) {
                v = W[g];
            } else {
                v = cmulc(W[g], tw2(p.big, (unsigned)col * (unsigned)i));
            }
        }
        cur[e] = v;
    }
    __syncthreads();
    EGR_STAMP(p, 1);
    if (MODE == 1 || MODE == 2 || MODE == 3 || MODE == 5) col_fft<SCHED>(cur, alt, p, TC, lg, true, stw);
    EGR_STAMP(p, 2);
    if (MODE == 5) {
        for (int e = threadIdx.x; e < nel; e += blockDim.x) {
            const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
            if (col < nc) Y[(size_t)i * nc + col] = cur[e];
        }
        return;
    }
    if (MODE == 2) {
        float mx = 0.f;
        for (int e = threadIdx.x; e < nel; e += blockDim.x) {
            const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
            if (col < nc) {
                const size_t g = (size_t)i * nc + col;
                const float2 y = Y[g];
                const cplx d = cur[e];
                const float2 o = make_float2(__fadd_rn(y.x, d.x), __fadd_rn(y.y, d.y));
                Y[g] = o;
                mx = fmaxf(mx, fmaxf(fabsf(o.x), fabsf(o.y)));
            }
        }
        mx = block_max(mx, red);
        if (threadIdx.x == 0) atomic_max_abs(peak_out + ch, mx);
        return;
    }
    if (MODE == 3) {
        for (int e = threadIdx.x; e < nel; e += blockDim.x) {
            const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
            if (col < nc) W[(size_t)i * nc + col] = cur[e];
        }
        return;
    }
    col_fft<SCHED>(cur, alt, p, TC, lg, false, stw);
    EGR_STAMP(p, 3);
    if (pairwise) {
        for (int e = 2 * threadIdx.x; e < nel; e += 2 * blockDim.x) {
            const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
            const float4 v2 = *(const float4*)(cur + e);
            const cplx a = cmul(make_float2(v2.x, v2.y), tw2(p.big, (unsigned)col * (unsigned)i));
            const cplx b = cmul(make_float2(v2.z, v2.w), tw2(p.big, (unsigned)(col + 1) * (unsigned)i));
            *(float4*)(W + (size_t)i * nc + col) = make_float4(a.x, a.y, b.x, b.y);
        }
    } else
    for (int e = threadIdx.x; e < nel; e += blockDim.x) {
        const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
        if (col < nc) W[(size_t)i * nc + col] = cmul(cur[e], tw2(p.big, (unsigned)col * (unsigned)i));
    }
    EGR_STAMP(p, 4);
}

// Row-pair kernel: outer indices oa = pair, ob = R - pair of the in-place state.
// MAXONLY: forward transform + real split only, max_k |X[k]|^2 of the channel -> p.max2_out[ch] (nothing is written back): the
// reduction a threshold RELATIVE to the spectrum's maximum needs before any bin can be judged.
// SCHED 1: L = 2304 as 16 x 16 x 9 with compile-time stages.
template <int SCHED>
__device__ __forceinline__ void row_fft(cplx*& cur, cplx*& alt, const RowP& p, int nrows, int L, bool inverse) {
    if (SCHED == 1) lds_fft_sched_inplace<false, EGR_FL_ROW_PAD, 2304 * 2, 512, EGR_FL_ROW_RADICES>(cur, L, p.stw, nrows, 0, 1, lds_pad<EGR_FL_ROW_PAD>(L), inverse);
    else lds_fft<false>(cur, alt, p.f, p.tw, nrows, 0, 1, L, inverse, p.twd);
}

template <bool MAXONLY, int SCHED = 0>
__global__ __launch_bounds__(SCHED ? 512 : 1024, SCHED ? EGR_FL_SCHED_WAVES : 1) void k_row(RowP p, long long M, cplx* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    EGR_LDS_CANARY_ARM(smem);
    __shared__ float red[16];
    const int L = p.L, R = p.R;
    const int oa = blockIdx.x;
    const int ob = (R - oa) % R;
    const bool self = (oa == ob);
    const int nrows = self ? 1 : 2;
    const int ch = blockIdx.y;
    cplx* cur = (cplx*)EGR_LDS_BASE(smem);
    cplx* alt = cur + 2 * (size_t)L;
    cplx* W = work + (size_t)ch * M;
    const int ra = (oa % p.Ma) * p.Mb + oa / p.Ma;
    const int rbw = (ob % p.Ma) * p.Mb + ob / p.Ma;
    cplx* ga = W + (size_t)ra * L;
    cplx* gb = W + (size_t)rbw * L;

    constexpr int PSH = SCHED == 1 ? EGR_FL_ROW_PAD : 0;      // LDS row layout: element i at lds_pad<PSH>(i)
    const int Lp = lds_pad<PSH>(L);
    // default hook (hard threshold on |X|^2, two distinct rows) of the scheduled kernel: two (k, M-k) pairs per thread and step
    const bool fast2 = SCHED == 1 && !MAXONLY && !self && !p.phat && !p.band && !p.gain && !p.soft && p.max2 == nullptr;
    dcplx wk_next = p.wk[fast2 ? 2 * threadIdx.x : (threadIdx.x < (unsigned)L ? threadIdx.x : 0)];   // first pair twiddle(s) of this thread
    dcplx wk_next1 = p.wk[fast2 ? 2 * threadIdx.x + 1 : 0];
    float max2v = 0.f;                       // the carried spectrum maximum, requested before the transform (an L2 miss: egr_fatllama_wl.h)
    if (!MAXONLY && p.max2) max2v = fl_max2_read(p.max2, ch);
    EGR_STAMP(p, 0);
    if (SCHED == 1) {                     // 16-byte state loads (two elements; a pair never straddles a pad position)
        for (int e = 2 * threadIdx.x; e < L; e += 2 * blockDim.x) {
            const float4 a = *(const float4*)(ga + e);
            cplx* d = cur + lds_pad<PSH>(e);
            d[0] = make_float2(a.x, a.y);
            d[1] = make_float2(a.z, a.w);
            if (!self) {
                const float4 b = *(const float4*)(gb + e);
                d[Lp] = make_float2(b.x, b.y);
                d[Lp + 1] = make_float2(b.z, b.w);
            }
        }
    } else
    for (int e = threadIdx.x; e < L; e += blockDim.x) {
        cur[lds_pad<PSH>(e)] = ga[e];
        if (!self) cur[Lp + lds_pad<PSH>(e)] = gb[e];
    }
    __syncthreads();
    EGR_STAMP(p, 1);
    row_fft<SCHED>(cur, alt, p, nrows, L, false);
    EGR_STAMP(p, 2);

    // real-split, threshold, un-split on the (k, M-k) pairs; Z[o + R*k] sits at row(o)[k]
    const dcplx wa = tw2d(p.wo, (unsigned)oa);
    int cnt, boff;          // partner of row-a element k is row-b element (boff - k) mod L
    cplx* rb;
    if (!self) { cnt = L; boff = L - 1; rb = cur + Lp; }
    else if (oa == 0) { cnt = L / 2 + 1; boff = L; rb = cur; }
    else { cnt = (L + 1) / 2; boff = L - 1; rb = cur; }
    const float sc = p.inv_M;
    const double scd = p.inv_M_d;
    float thr2 = p.thr2, tlev = p.thr;
    if (!MAXONLY && p.max2) {
        tlev = p.thr * sqrtf(max2v);
        thr2 = tlev * tlev;
    }
    if (!MAXONLY && p.max2_zero && blockIdx.x == 0 && threadIdx.x < EGR_FL_MAX_SUB) fl_max2_clear(p.max2_zero, ch, threadIdx.x);
    const bool variant = !MAXONLY && (p.max2 != nullptr || p.soft);
    float mx2 = 0.f;
    if (fast2) {
        // the same arithmetic as the default branch of the loop below, on elements k2, k2 + 1 of row a and their partners
        // L - 1 - k2, L - 2 - k2 of row b: adjacent LDS elements on both sides (a pair never straddles a pad position)
        auto one = [&](const cplx Za, const cplx Zb, const dcplx wkd, cplx& na, cplx& nb) {
            const dcplx Wkd = dcmul(wa, wkd);
            const cplx Wk = make_float2((float)Wkd.x, (float)Wkd.y);
            const cplx E = make_float2(0.5f * (Za.x + Zb.x), 0.5f * (Za.y - Zb.y));
            const cplx O = make_float2(0.5f * (Za.y + Zb.y), -0.5f * (Za.x - Zb.x));
            const cplx WO = cmul(Wk, O);
            cplx Xk = cadd(E, WO), Xm = csub(E, WO);
            if (!(Xk.x * Xk.x + Xk.y * Xk.y > thr2)) Xk = make_float2(0.f, 0.f);
            if (!(Xm.x * Xm.x + Xm.y * Xm.y > thr2)) Xm = make_float2(0.f, 0.f);
            const cplx E2 = make_float2(0.5f * (Xk.x + Xm.x), 0.5f * (Xk.y + Xm.y));
            const cplx H = make_float2(0.5f * (Xk.x - Xm.x), 0.5f * (Xk.y - Xm.y));
            const cplx O2 = cmulc(H, Wk);
            na = make_float2((float)(scd * (double)(E2.x - O2.y)), (float)(scd * (double)(E2.y + O2.x)));
            nb = make_float2((float)(scd * (double)(E2.x + O2.y)), -(float)(scd * (double)(E2.y - O2.x)));
        };
        for (int k2 = 2 * threadIdx.x; k2 < L; k2 += 2 * blockDim.x) {
            const dcplx w0 = wk_next, w1 = wk_next1;
            if (k2 + 2 * (int)blockDim.x < L) { wk_next = p.wk[k2 + 2 * blockDim.x]; wk_next1 = p.wk[k2 + 2 * blockDim.x + 1]; }
            cplx* da = cur + lds_pad<PSH>(k2);
            cplx* db = rb + lds_pad<PSH>(L - 2 - k2);
            const cplx Za0 = da[0], Za1 = da[1], Zb1 = db[0], Zb0 = db[1];
            cplx na0, nb0, na1, nb1;
            one(Za0, Zb0, w0, na0, nb0);
            one(Za1, Zb1, w1, na1, nb1);
            da[0] = na0; da[1] = na1;
            db[1] = nb0; db[0] = nb1;
        }
    } else
    for (int k2 = threadIdx.x; k2 < cnt; k2 += blockDim.x) {
        // the table entry of the NEXT pair is requested before this one is worked on (the first was requested before the
        // forward transform): the 16-byte L2 round trip per pair is off the dependent chain
        const dcplx wk_cur = wk_next;
        if (k2 + (int)blockDim.x < cnt) wk_next = p.wk[k2 + blockDim.x];
        int pb = boff - k2;
        if (pb >= L) pb -= L;
        const bool same = self && (pb == k2);
        const int ia = lds_pad<PSH>(k2), ib = lds_pad<PSH>(pb);
        const cplx Za = cur[ia];
        const cplx Zb = rb[ib];
        const dcplx Wkd = dcmul(wa, wk_cur);
        const cplx Wk = make_float2((float)Wkd.x, (float)Wkd.y);
        // E = (Za + conj Zb)/2 ; O = (Za - conj Zb)/(2i)
        const cplx E = make_float2(0.5f * (Za.x + Zb.x), 0.5f * (Za.y - Zb.y));
        const cplx O = make_float2(0.5f * (Za.y + Zb.y), -0.5f * (Za.x - Zb.x));
        if (p.phat) {
            // two-for-one: A[k] = E, B[k] = O are the spectra of a and b; R = B conj(A) / (|B conj(A)| + 1e-12) is the spectrum
            // of the real GCC-PHAT sequence, so the new state is W[k] = R, W[M-k] = conj(R) (times 1/M for the inverse passes)
            cplx Rk = cmulc(O, E);
            const float inv = sc / (sqrtf(Rk.x * Rk.x + Rk.y * Rk.y) + 1e-12f);
            Rk.x *= inv; Rk.y *= inv;
            cur[ia] = Rk;
            if (!same) rb[ib] = make_float2(Rk.x, -Rk.y);
            continue;
        }
        const cplx WO = cmul(Wk, O);
        cplx Xk = cadd(E, WO);      // X[k]
        cplx Xm = csub(E, WO);      // conj X[M-k]
        if (MAXONLY) {
            mx2 = fmaxf(mx2, fmaxf(Xk.x * Xk.x + Xk.y * Xk.y, Xm.x * Xm.x + Xm.y * Xm.y));
            continue;
        }
        if (variant) {
            const float mk = sqrtf(Xk.x * Xk.x + Xk.y * Xk.y), mm = sqrtf(Xm.x * Xm.x + Xm.y * Xm.y);
            float gk = mk > tlev ? 1.f : 0.f, gm = mm > tlev ? 1.f : 0.f;
            if (p.soft) {
                if (mk > tlev) gk = 1.f - tlev / mk;
                if (mm > tlev) gm = 1.f - tlev / mm;
            }
            Xk.x *= gk; Xk.y *= gk; Xm.x *= gm; Xm.y *= gm;
            mx2 = fmaxf(mx2, fmaxf(Xk.x * Xk.x + Xk.y * Xk.y, Xm.x * Xm.x + Xm.y * Xm.y));      // what the next iteration's spectrum will hold
        } else if (p.band) {
            const long long k = (long long)oa + (long long)R * k2;
            if (k < p.band_lo) Xk = make_float2(0.f, 0.f);
            if (M - k < p.band_lo) Xm = make_float2(0.f, 0.f);
        } else if (p.gain) {
            const long long k = (long long)oa + (long long)R * k2;
            const float* g = p.gain + (size_t)ch * (M + 1);
            const float gk = g[k], gm = g[M - k];
            Xk.x *= gk; Xk.y *= gk; Xm.x *= gm; Xm.y *= gm;
        } else {
            if (!(Xk.x * Xk.x + Xk.y * Xk.y > thr2)) Xk = make_float2(0.f, 0.f);
            if (!(Xm.x * Xm.x + Xm.y * Xm.y > thr2)) Xm = make_float2(0.f, 0.f);
        }
        const cplx E2 = make_float2(0.5f * (Xk.x + Xm.x), 0.5f * (Xk.y + Xm.y));
        const cplx H = make_float2(0.5f * (Xk.x - Xm.x), 0.5f * (Xk.y - Xm.y));
        const cplx O2 = cmulc(H, Wk);
        // Za' = E2 + i*O2 ; Zb' = conj(E2 - i*O2)
        cur[ia] = make_float2((float)(scd * (double)(E2.x - O2.y)), (float)(scd * (double)(E2.y + O2.x)));
        if (!same) rb[ib] = make_float2((float)(scd * (double)(E2.x + O2.y)), -(float)(scd * (double)(E2.y - O2.x)));
    }
    if (MAXONLY) {
        mx2 = block_max(mx2, red);
        if (threadIdx.x == 0) fl_max2_commit(p.max2_out, ch, mx2);
        return;
    }
    if (p.max2_next) {                       // carried maximum: one commit per workgroup, behind the barrier that is there anyway
        mx2 = wave_max(mx2);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx2;
    }
    __syncthreads();
    if (p.max2_next && threadIdx.x == 0) {
        float r = red[0];
        for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = fmaxf(r, red[i]);
        fl_max2_commit(p.max2_next, ch, r);
    }
    EGR_STAMP(p, 3);
    row_fft<SCHED>(cur, alt, p, nrows, L, true);
    EGR_STAMP(p, 4);
    if (SCHED == 1) {
        for (int e = 2 * threadIdx.x; e < L; e += 2 * blockDim.x) {
            const cplx* d = cur + lds_pad<PSH>(e);
            *(float4*)(ga + e) = make_float4(d[0].x, d[0].y, d[1].x, d[1].y);
            if (!self) *(float4*)(gb + e) = make_float4(d[Lp].x, d[Lp].y, d[Lp + 1].x, d[Lp + 1].y);
        }
    } else
    for (int e = threadIdx.x; e < L; e += blockDim.x) {
        ga[e] = cur[lds_pad<PSH>(e)];
        if (!self) gb[e] = cur[Lp + lds_pad<PSH>(e)];
    }
    EGR_STAMP(p, 5);
}

}  // namespace egr
#include "egr_fatllama_wl.h"
namespace egr {

// ------------------------------------------------------------------------------------------------
// Bluestein fallback for lengths the packed real transform cannot take (odd N, large prime factors):
// the exact length-N DFT as a cyclic convolution of length P >= 2N-1 (P smooth):
//   DFT(d)[k] = w[k] * (a (*) b)[k],  a[n] = d[n] w[n],  b[m] = conj(w[m]) for |m| < N,  w[n] = exp(-i pi n^2 / N).
// The convolution runs on the SAME column/row passes with the state holding P complex points:
//   k_colz (outer column pass, hook fused at its natural-order midpoint)  +  k_rowconv (row FFT . x Bhat . row IFFT).
// One loop iteration = spectrum hook (X = w c; threshold; a' = conj(X) w) and time hook (d = Re(w c')/N; a = d w),
// each followed by a convolution: 4 launches over 8P-byte states instead of 2 over 4N-byte ones (slow path).
// ------------------------------------------------------------------------------------------------
// MODE 0: first (y real -> time threshold -> a = d w -> FFT -> twiddle)
// MODE 1: mid   (twiddle^-1 -> IFFT -> hook -> FFT -> twiddle); HOOK 1 = spectrum side, HOOK 2 = time side
// MODE 2: last  (twiddle^-1 -> IFFT -> d = Re(w c)/N -> out = y + d, peak)
// MODE 3: spectrum maximum only (twiddle^-1 -> IFFT -> max |w c|^2 -> cp.max2_out[ch]; nothing written back)
template <int MODE, int HOOK>
__global__ __launch_bounds__(1024) void k_colz(ColP p, ChirpP cp, long long P, float thr, float thr2,
                                               cplx* __restrict__ work, float* __restrict__ out,
                                               unsigned* __restrict__ peak_out, const unsigned* __restrict__ thr_rel = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    EGR_LDS_CANARY_ARM(smem);
    __shared__ float red[16];                 // one slot per wave: up to 1024 threads
    const int tile = (blockIdx.x & 7) * p.tiles_per_xcd + (blockIdx.x >> 3);
    if (tile >= p.ntiles) return;
    const int ch = blockIdx.y;
    const int TC = p.TC, lg = p.TClog2, L = p.L, nc = p.ncols;
    const int c0 = tile * TC;
    cplx* cur = (cplx*)EGR_LDS_BASE(smem);
    cplx* alt = cur + (size_t)L * TC;
    cplx* W = work + (size_t)ch * P;
    float* Y = out + (size_t)ch * cp.N;
    const int nel = L * TC;
    const unsigned long long N = cp.N;
    if (MODE == 0 && thr_rel) thr *= __uint_as_float(thr_rel[ch]);

    for (int e = threadIdx.x; e < nel; e += blockDim.x) {
        const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
        cplx v = make_float2(0.f, 0.f);
        if (col < nc) {
            const unsigned long long n = (unsigned long long)i * nc + col;
            if (MODE == 0) {
                if (n < N) {
                    const float y = Y[n];
                    const float d0 = fabsf(y) > thr ? y : 0.f;
                    const cplx w = chirp(cp, n);
                    v = make_float2(d0 * w.x, d0 * w.y);
                }
            } else {
                v = cmulc(W[n], tw2(p.big, (unsigned)col * (unsigned)i));
            }
        }
        cur[e] = v;
    }
    __syncthreads();
    if (MODE != 0) lds_fft<true>(cur, alt, p.f, p.tw, TC, lg, TC, 1, true, p.twd);
    if (MODE == 3) {
        float mx = 0.f;
        for (int e = threadIdx.x; e < nel; e += blockDim.x) {
            const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
            const unsigned long long n = (unsigned long long)i * nc + col;
            if (col < nc && n < N) {
                const cplx X = cmul(chirp(cp, n), cur[e]);
                mx = fmaxf(mx, X.x * X.x + X.y * X.y);
            }
        }
        mx = block_max(mx, red);
        if (threadIdx.x == 0) fl_max2_commit(cp.max2_out, ch, mx);
        return;
    }
    if (MODE == 1 && HOOK == 1 && cp.max2) {
        thr *= sqrtf(fl_max2_read(cp.max2, ch));
        thr2 = thr * thr;
    }
    if (MODE == 2) {
        float mx = 0.f;
        for (int e = threadIdx.x; e < nel; e += blockDim.x) {
            const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
            const unsigned long long n = (unsigned long long)i * nc + col;
            if (col < nc && n < N) {
                const cplx w = chirp(cp, n);
                const cplx cc = cur[e];
                const float d = (w.x * cc.x - w.y * cc.y) * cp.inv_N;
                const float o = __fadd_rn(Y[n], d);
                Y[n] = o;
                mx = fmaxf(mx, fabsf(o));
            }
        }
        mx = block_max(mx, red);
        if (threadIdx.x == 0) atomic_max_abs(peak_out + ch, mx);
        return;
    }
    if (MODE == 1) {
        for (int e = threadIdx.x; e < nel; e += blockDim.x) {
            const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
            const unsigned long long n = (unsigned long long)i * nc + col;
            cplx v = make_float2(0.f, 0.f);
            if (col < nc && n < N) {
                const cplx w = chirp(cp, n);
                const cplx cc = cur[e];
                if (HOOK == 1) {                 // X = w c ; threshold ; a' = conj(X) w
                    cplx X = cmul(w, cc);
                    if (cp.band) {
                        if ((n < N - n ? n : N - n) < cp.band_lo) X = make_float2(0.f, 0.f);
                    } else if (cp.soft) {
                        const float mg = sqrtf(X.x * X.x + X.y * X.y);
                        const float g = mg > thr ? 1.f - thr / mg : 0.f;
                        X.x *= g; X.y *= g;
                    } else if (!(X.x * X.x + X.y * X.y > thr2)) X = make_float2(0.f, 0.f);
                    v = cmul(make_float2(X.x, -X.y), w);
                } else {                         // d = Re(w c)/N ; a = d w
                    const float d = (w.x * cc.x - w.y * cc.y) * cp.inv_N;
                    v = make_float2(d * w.x, d * w.y);
                }
            }
            cur[e] = v;
        }
        __syncthreads();
    }
    lds_fft<true>(cur, alt, p.f, p.tw, TC, lg, TC, 1, false, p.twd);
    for (int e = threadIdx.x; e < nel; e += blockDim.x) {
        const int c = e & (TC - 1), i = e >> lg, col = c0 + c;
        if (col < nc) W[(size_t)i * nc + col] = cmul(cur[e], tw2(p.big, (unsigned)col * (unsigned)i));
    }
}

// rows r0 = EGR_FL_CONV_ROWS * blockIdx.x (, r0 + 1) of R rows of length L.  CONV: FFT . x bhat[row][k] . IFFT ; else FFT . x scale
// (used once to build bhat itself).
template <bool CONV>
__global__ __launch_bounds__(EGR_FL_CONV_THREADS) void k_rowconv(FftDesc f, int L, int R, const cplx* __restrict__ tw,
                                                  const cplx* __restrict__ bhat, float scale, long long P,
                                                  cplx* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    EGR_LDS_CANARY_ARM(smem);
    const int r0 = EGR_FL_CONV_ROWS * blockIdx.x;
    const int nrows = (r0 + 1 < R && EGR_FL_CONV_ROWS == 2) ? 2 : 1;
    constexpr int PSH = EGR_FL_CONV_PAD;                 // rows in LDS: element i at lds_pad<PSH>(i), stages in place
    const int Lp = lds_pad<PSH>(L);
    cplx* cur = (cplx*)EGR_LDS_BASE(smem);
    cplx* g = work + (size_t)blockIdx.y * P + (size_t)r0 * L;
    // 16-byte accesses (two elements per thread and step) when rows start 16-byte aligned; one row per workgroup then
    const bool pairwise = PSH == 0 && EGR_FL_CONV_ROWS == 1 && (L & 1) == 0;
    if (pairwise) {
        for (int e = 2 * threadIdx.x; e < L; e += 2 * blockDim.x) *(float4*)(cur + e) = *(const float4*)(g + e);
    } else
    for (int e = threadIdx.x; e < nrows * L; e += blockDim.x) {
        const int r = e >= L ? 1 : 0, i = e - r * L;
        cur[r * Lp + lds_pad<PSH>(i)] = g[e];
    }
    __syncthreads();
    lds_fft_ip<false, PSH, false>(cur, f, tw, nrows, 0, 1, Lp, false);
    if (CONV) {
        const cplx* bh = bhat + (size_t)r0 * L;
        if (pairwise) {
            for (int e = 2 * threadIdx.x; e < L; e += 2 * blockDim.x) {
                const float4 c = *(const float4*)(cur + e), b = *(const float4*)(bh + e);
                const cplx u = cmul(make_float2(c.x, c.y), make_float2(b.x, b.y)), v = cmul(make_float2(c.z, c.w), make_float2(b.z, b.w));
                *(float4*)(cur + e) = make_float4(u.x, u.y, v.x, v.y);
            }
        } else
        for (int e = threadIdx.x; e < nrows * L; e += blockDim.x) {
            const int r = e >= L ? 1 : 0, i = e - r * L, a = r * Lp + lds_pad<PSH>(i);
            cur[a] = cmul(cur[a], bh[e]);
        }
        __syncthreads();
        lds_fft_ip<false, PSH, false>(cur, f, tw, nrows, 0, 1, Lp, true);
        if (pairwise) {
            for (int e = 2 * threadIdx.x; e < L; e += 2 * blockDim.x) *(float4*)(g + e) = *(const float4*)(cur + e);
        } else
        for (int e = threadIdx.x; e < nrows * L; e += blockDim.x) {
            const int r = e >= L ? 1 : 0, i = e - r * L;
            g[e] = cur[r * Lp + lds_pad<PSH>(i)];
        }
    } else {
        for (int e = threadIdx.x; e < nrows * L; e += blockDim.x) {
            const int r = e >= L ? 1 : 0, i = e - r * L;
            const cplx c = cur[r * Lp + lds_pad<PSH>(i)];
            g[e] = make_float2(c.x * scale, c.y * scale);
        }
    }
}

// b[j] = conj(w[j]) for j < N, b[P-j] = conj(w[j]) for 0 < j < N, zero elsewhere
__global__ __launch_bounds__(256) void k_chirp_b(ChirpP cp, long long P, cplx* __restrict__ b) {
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < P; j += (long long)gridDim.x * blockDim.x) {
        long long m = -1;
        if ((unsigned long long)j < cp.N) m = j;
        else if ((unsigned long long)(P - j) < cp.N) m = P - j;
        cplx v = make_float2(0.f, 0.f);
        if (m >= 0) {
            const cplx w = chirp(cp, (unsigned long long)m);
            v = make_float2(w.x, -w.y);
        }
        b[j] = v;
    }
}

// x (optionally PCM_16-quantised) -> y = linear up-rate by f, per-channel max|x_q|.
// zero_stuff: y[i*f] = x[i], zeros between (SPEC.md "interp").  peak_y[ch] = max|y| (what a relative time-domain threshold refers to).
// linspace (SPEC.md "interp"): y[j] = interp(j (n_in - 1) / (n_out - 1), arange(n_in), x) -- numpy.interp on the endpoint-inclusive
// grid numpy.linspace(0, n_in - 1, n_out), evaluated like numpy (double: slope * (pos - i) + x[i], last point exactly x[n_in - 1]);
// n_out need not be a multiple of n_in (factor_mode "ratio_then_int").
// One channel row: xc -> yc (n_in f samples; n_out with linspace), the row's peaks into *peak_in / *peak_y.  Shared by k_prepare (the
// rows of one plan) and k_prepare_rows (rows of their own lengths, egr_flmany_enhance).
__device__ __forceinline__ void fl_prepare_row(const float* __restrict__ xc, float* __restrict__ yc, long long n_in, int f, int pcm_in,
                                               int zero_stuff, unsigned* __restrict__ peak_in, unsigned* __restrict__ peak_y, int linspace,
                                               long long n_out, float* red) {
#pragma clang fp contract(off)      // the roundings below are the PCM arithmetic of the reference, written out
    const float ff = (float)f;
    float mx = 0.f, my = 0.f;
    if (linspace) {
        float* yo = yc;
        auto q = [&](float a) -> float {
            if (!pcm_in) return a;
            long long qa = (long long)rintf(__fmul_rn(a, 32767.0f));
            return (float)(((qa + 32768) & 65535) - 32768);
        };
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += (long long)gridDim.x * blockDim.x)
            mx = fmaxf(mx, fabsf(q(xc[i])));
        const double step = n_out > 1 ? (double)(n_in - 1) / (double)(n_out - 1) : 0.0;
        for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n_out; j += (long long)gridDim.x * blockDim.x) {
            float v;
            if (j == n_out - 1 && n_out > 1) {
                v = q(xc[n_in - 1]);
            } else {
                const double pos = (double)j * step;
                long long i0 = (long long)pos;
                if (i0 > n_in - 2) i0 = n_in - 2;
                if (i0 < 0) i0 = 0;
                const double a = (double)q(xc[i0]), b = n_in > 1 ? (double)q(xc[i0 + 1]) : a;
                v = (float)((b - a) * (pos - (double)i0) + a);
            }
            yo[j] = v;
            my = fmaxf(my, fabsf(v));
        }
        mx = block_max(mx, red);
        my = block_max(my, red);
        if (threadIdx.x == 0) {
            atomic_max_abs(peak_in, mx);
            atomic_max_abs(peak_y, my);
        }
        return;
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_in;
         i += (long long)gridDim.x * blockDim.x) {
        float a = xc[i];
        float b = (i + 1 < n_in) ? xc[i + 1] : 0.f;
        if (pcm_in) {
            long long qa = (long long)rintf(__fmul_rn(a, 32767.0f));
            long long qb = (long long)rintf(__fmul_rn(b, 32767.0f));
            qa = ((qa + 32768) & 65535) - 32768;
            qb = ((qb + 32768) & 65535) - 32768;
            a = (float)qa;
            b = (float)qb;
        }
        mx = fmaxf(mx, fabsf(a));
        if (zero_stuff) {
            yc[i * f] = a;
            for (int j = 1; j < f; ++j) yc[i * f + j] = 0.f;
            my = fmaxf(my, fabsf(a));
        } else if (i + 1 < n_in) {
            for (int j = 0; j < f; ++j) {
                const float t = __fdiv_rn((float)j, ff);
                const float u = __fsub_rn(1.0f, t);
                const float v = __fadd_rn(__fmul_rn(u, a), __fmul_rn(t, b));
                yc[i * f + j] = v;
                my = fmaxf(my, fabsf(v));
            }
        } else {
            for (int j = 0; j < f; ++j) yc[i * f + j] = 0.f;   // upstream leaves the last sample's slots zero
        }
    }
    mx = block_max(mx, red);
    my = block_max(my, red);
    if (threadIdx.x == 0) {
        atomic_max_abs(peak_in, mx);
        atomic_max_abs(peak_y, my);
    }
}

__global__ __launch_bounds__(256) void k_prepare(const float* __restrict__ x, float* __restrict__ y, long long n_in,
                                                  int f, int pcm_in, int zero_stuff, unsigned* __restrict__ peak_in,
                                                  unsigned* __restrict__ peak_y, int linspace = 0, long long n_out = 0) {
    __shared__ float red[8];
    const int ch = blockIdx.y;
    fl_prepare_row(x + (size_t)ch * n_in, linspace ? y + (size_t)ch * n_out : y + (size_t)ch * n_in * f, n_in, f, pcm_in, zero_stuff,
                   peak_in + ch, peak_y + ch, linspace, n_out, red);
}

// A channel row of a wave (egr_flmany_*): its own lengths and places in the flat x and y / out buffers, and the channel rows
// [c_lo, c_hi) of its clip (the joint peak of k_finalize_rows).
struct FlRagRow {
    long long x_off, y_off, n_in, n_out;
    int factor, c_lo, c_hi, pad_;
};
// k_prepare for rows of their own lengths: blockIdx.y = channel row; the grid covers the longest row
__global__ __launch_bounds__(256) void k_prepare_rows(const float* __restrict__ x, float* __restrict__ y, const FlRagRow* __restrict__ rows,
                                                       int pcm_in, int zero_stuff, unsigned* __restrict__ peak_in, unsigned* __restrict__ peak_y,
                                                       int linspace) {
    __shared__ float red[8];
    const int ch = blockIdx.y;
    const FlRagRow r = rows[ch];
    fl_prepare_row(x + r.x_off, y + r.y_off, r.n_in, r.factor, pcm_in, zero_stuff, peak_in + ch, peak_y + ch, linspace, r.n_out, red);
}

// max_iter == 0 path: out = y + (|y|>thr ? y : 0), peaks
__global__ __launch_bounds__(256) void k_noiter(float* __restrict__ y, long long N, float thr,
                                                 unsigned* __restrict__ peak_out, const unsigned* __restrict__ thr_rel) {
    __shared__ float red[8];
    const int ch = blockIdx.y;
    if (thr_rel) thr *= __uint_as_float(thr_rel[ch]);
    float* yc = y + (size_t)ch * N;
    float mx = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N;
         i += (long long)gridDim.x * blockDim.x) {
        const float v = yc[i];
        const float o = __fadd_rn(v, fabsf(v) > thr ? v : 0.f);
        yc[i] = o;
        mx = fmaxf(mx, fabsf(o));
    }
    mx = block_max(mx, red);
    if (threadIdx.x == 0) atomic_max_abs(peak_out + ch, mx);
}

// autoscale / normalise / write patch / PCM_16 round trip, all driven by the 2*C peak scalars.
// joint_ext (optional): the peak of channels this plan does NOT hold -- the other ranks' of a channel-parallel run
// (egr_fatllama_joint_peak on every rank, one all-reduce(MAX) of that float, egr_fatllama_finalize): max is exact, so the result is
// the single-plan result bit for bit.  joint_dst (optional, k_joint_peak): where this plan's own joint peak goes; nothing else is done.
// One channel row `ch` (samples oc[0 .. N)) of a signal whose channels are the rows [c_lo, c_hi) of the peak arrays.  Shared by
// k_finalize (c_lo = 0, c_hi = C) and k_finalize_rows.
__device__ __forceinline__ void fl_finalize_row(float* __restrict__ oc, long long N, int c_lo, int c_hi, int ch, unsigned flags,
                                                const unsigned* __restrict__ peak_in, const unsigned* __restrict__ peak_out,
                                                const float* __restrict__ joint_ext, float* __restrict__ joint_dst) {
#pragma clang fp contract(off)      // the roundings below are the PCM arithmetic of the reference, written out
    float s_auto = 1.f;
    float joint = 0.f;
    for (int c = c_lo; c < c_hi; ++c) {
        const float pi = __uint_as_float(peak_in[c]), po = __uint_as_float(peak_out[c]);
        float s = 1.f, m = po;
        if ((flags & EGR_FL_AUTOSCALE) && po > 0.f) {
            s = (float)((double)pi / (double)po);
            m = __fmul_rn(po, s);
        }
        if (c == ch) s_auto = s;
        joint = fmaxf(joint, m);
    }
    if (joint_dst) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *joint_dst = joint;
        return;
    }
    if (joint_ext) joint = fmaxf(joint, *joint_ext);
    const bool do_auto = (flags & EGR_FL_AUTOSCALE) != 0;
    const bool do_norm = (flags & EGR_FL_NORMALIZE) && joint > 0.f;
    float peak_final = do_norm ? 1.0f : joint;
    const bool patch = (flags & EGR_FL_NODE_POST) && peak_final > 1.0f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N;
         i += (long long)gridDim.x * blockDim.x) {
        float v = oc[i];
        if (do_auto) v = __fmul_rn(v, s_auto);
        if (do_norm) v = __fdiv_rn(v, joint);
        if (flags & EGR_FL_NODE_POST) {
            if (patch) v = __fmul_rn(v, 1.0f / 32768.0f);
            long long q = (long long)rintf(__fmul_rn(v, 32767.0f));
            q = ((q + 32768) & 65535) - 32768;
            v = __fmul_rn((float)q, 1.0f / 32768.0f);
        }
        oc[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_finalize(float* __restrict__ out, long long N, int C, unsigned flags,
                                                   const unsigned* __restrict__ peak_in,
                                                   const unsigned* __restrict__ peak_out,
                                                   const float* __restrict__ joint_ext, float* __restrict__ joint_dst) {
    const int ch = blockIdx.y;
    fl_finalize_row(out + (size_t)ch * N, N, 0, C, ch, flags, peak_in, peak_out, joint_ext, joint_dst);
}

// k_finalize for rows of their own lengths: autoscale, the joint peak and the write patch over the channel rows of the row's own clip
__global__ __launch_bounds__(256) void k_finalize_rows(float* __restrict__ out, const FlRagRow* __restrict__ rows, unsigned flags,
                                                        const unsigned* __restrict__ peak_in, const unsigned* __restrict__ peak_out) {
    const int ch = blockIdx.y;
    const FlRagRow r = rows[ch];
    fl_finalize_row(out + r.y_off, r.n_out, r.c_lo, r.c_hi, ch, flags, peak_in, peak_out, nullptr, nullptr);
}

}  // namespace egr

using namespace egr;

// A host table as a device buffer the plan owns; *d: its address.
template <class T> static int upload_bytes(egr_fatllama_plan* p, const void* h, size_t bytes, const T** d) {
    void* ptr = nullptr;
    EGR_HIP(hipMalloc(&ptr, bytes));
    p->tables.emplace_back();
    p->tables.back().p = ptr;
    EGR_HIP(hipMemcpy(ptr, h, bytes, hipMemcpyHostToDevice));
    *d = (const T*)ptr;
    return EGR_OK;
}

int fl_upload(egr_fatllama_plan* p, const std::vector<float2>& h, const cplx** d) { return upload_bytes(p, h.data(), h.size() * sizeof(float2), d); }

int fl_upload_d(egr_fatllama_plan* p, int L, const dcplx** d) { return fl_upload_dtab(p, L, 1, L, d); }

// exp(-2 pi i j num / den), j < count, as a double-precision device table
int fl_upload_dtab(egr_fatllama_plan* p, int64_t count, int64_t num, int64_t den, const dcplx** d) {
    std::vector<double2> h;
    make_twiddles_d(h, count, num, den);
    return upload_bytes(p, h.data(), h.size() * sizeof(double2), d);
}

// butterfly-ordered stage tables of a compile-time schedule (R0, R1, R2; R2 = 1: two stages): for stage s >= 1 with
// Ns = product of the earlier radices, row k < Ns holds W_(Ns R)^(k t), t = 0 .. R-1, padded to an even entry count
int fl_upload_sched_tables(egr_fatllama_plan* p, std::initializer_list<int> radices, const cplx** d) {
    std::vector<float2> h;
    const long double two_pi = 6.283185307179586476925286766559L;
    auto add = [&](int Ns, int R) {
        const int RS = (R + 1) & ~1;
        for (int k = 0; k < Ns; ++k)
            for (int t = 0; t < RS; ++t) {
                const long double ang = t < R ? -two_pi * (long double)((long long)k * t % ((long long)Ns * R)) / (long double)((long long)Ns * R) : 0.0L;
                h.push_back(make_float2((float)cosl(ang), (float)sinl(ang)));
            }
    };
    int ns = 1, s = 0;
    for (int r : radices) {
        if (s > 0 && r > 1) add(ns, r);
        ns *= r;
        ++s;
    }
    return fl_upload(p, h, d);
}

// tables for W_T^r, r < T
int fl_make_tw2(egr_fatllama_plan* p, int64_t T, Tw2* out) {
    int sh = 0;
    while ((1LL << (2 * sh)) < T) ++sh;          // 2^sh >= sqrt(T)
    int rc;
    if ((rc = fl_upload_dtab(p, (T >> sh) + 1, 1LL << sh, T, &out->hi))) return rc;
    if ((rc = fl_upload_dtab(p, 1LL << sh, 1, T, &out->lo))) return rc;
    out->sh = sh;
    return EGR_OK;
}

static void fill_info(const FlSplit& sp, int64_t info[EGR_FL_INFO_LEN]) {
    info[0] = 1;
    info[3] = sp.M1; info[4] = sp.M2; info[5] = sp.TC; info[6] = sp.f1.nst; info[7] = sp.f2.nst;
    for (int i = 0; i < EGR_MAX_STAGES; ++i) { info[8 + i] = sp.f1.radix[i]; info[22 + i] = sp.f2.radix[i]; }
    info[36] = (int64_t)sp.lds_col;
    info[37] = (int64_t)sp.lds_row;
    info[38] = sp.M3;
    info[39] = sp.levels;
}

static bool bluestein_length(int64_t want, FlSplit* sp_out);
static bool pz_length(int64_t D, const FlSwitches& sw, FlSplit* sp_out);
// paired chirp-z kind for N real samples: 1 = even/odd packing (N even, D = N / 2), 2 = channel pairs (N odd, D = N)
static inline int pz_kind_for(int64_t N) { return (N & 1) ? 2 : 1; }
// LDS of k_rowconv: two rows, stages in place
static size_t rowconv_lds(int L) { return EGR_LDS((size_t)EGR_FL_CONV_ROWS * (L + (EGR_FL_CONV_PAD ? L >> EGR_FL_CONV_PAD : 0)) * sizeof(cplx)); }
// blocks of 256 threads striding over n elements of a channel
static int fl_grid(long long n) { return (int)std::min<long long>((n + 255) / 256, 2048); }
// dynamic LDS of the scheduled loop kernels: k_row<., 1> has no ping-pong buffer and pads its two rows by one element per
// 2^EGR_FL_ROW_PAD; k_col<., 2> transforms in place
static size_t row_sched_lds(int L) { return EGR_LDS((size_t)2 * (L + (EGR_FL_ROW_PAD ? L >> EGR_FL_ROW_PAD : 0)) * sizeof(cplx)); }
static size_t col_sched_lds(const egr_fatllama_plan* p) { return EGR_LDS(p->sp.lds_col / 2); }
// workgroup size of the chirp-z loop kernels (their tiles take most of a CU's LDS: one workgroup per CU, so a large one)
static int blue_threads() {
    static const int t = [] { const char* e = getenv("EGR_FL_BLUE_THREADS"); const int v = e ? atoi(e) : 1024; return (v == 256 || v == 512 || v == 1024) ? v : 1024; }();
    return t;
}

static FlSwitches fl_read_switches() {
    auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    FlSwitches s;
    const int streams = num("EGR_FL_STREAMS", s.streams), threads = num("EGR_FL_THREADS", s.threads);
    if (streams == 1 || streams == 2) s.streams = streams;
    if (threads == 256 || threads == 512 || threads == 1024) s.threads = threads;
    s.graph = num("EGR_FL_GRAPH", 1) != 0;
    s.sched = num("EGR_FL_SCHED", 1) != 0;
    s.wl = num("EGR_FL_WL", 1) != 0;
    s.twpow = num("EGR_FL_TWPOW", 1);
    s.m1 = num("EGR_FL_M1", 0);
    s.tc = num("EGR_FL_TC", 0);
    s.legacy_chirpz = num("EGR_FL_LEGACY_CHIRPZ", 0) != 0;
    s.pz_sched = num("EGR_PZ_SCHED", 1) != 0;
    s.pz_colwl = num("EGR_PZ_COLWL", 1) != 0;
    s.pz_pairwl = num("EGR_PZ_PAIRWL", 1) != 0;
    s.pz_rowf = num("EGR_PZ_ROWF", 1) != 0;
    if (const char* e = getenv("EGR_PZ_SPLIT")) {
        int L = 0, nc = 0;
        if (sscanf(e, "%d,%d", &L, &nc) == 2) { s.pz_split_L = L; s.pz_split_nc = nc; }
    }
    return s;
}

static const char* kUnsupported =
    "length %lld unsupported: needs even N whose half factors into 2 or 3 lengths (outer columns <= 2048, inner columns <= 1024, row <= 4096) with "
    "prime factors <= 13";

extern "C" int egr_fatllama_plan_query(int64_t n_in, int factor, int m1_hint, int64_t info[EGR_FL_INFO_LEN]) {
    EGR_CHECK(info != nullptr, EGR_ERR_ARG, "info is null");
    memset(info, 0, sizeof(int64_t) * EGR_FL_INFO_LEN);
    EGR_CHECK(n_in >= 1 && factor >= 1, EGR_ERR_ARG, "n_in=%lld factor=%d out of range", (long long)n_in, factor);
    const int64_t N = n_in * factor;
    FlSplit sp = plan_split(N, m1_hint, 0);
    info[1] = N;
    info[2] = N / 2;
    if (!sp.ok) {
        const int kind = pz_kind_for(N);
        if (N >= 2 && pz_length(kind == 1 ? N / 2 : N, fl_read_switches(), &sp)) {      // paired chirp-z over P = sp.M complex points per state
            fill_info(sp, info);
            info[0] = 2;
            info[2] = sp.M;
            info[40] = kind;
            info[41] = kind == 1 ? N / 2 : N;
            return EGR_OK;
        }
        set_error(kUnsupported, (long long)N);
        return EGR_ERR_UNSUPPORTED;
    }
    fill_info(sp, info);
    return EGR_OK;
}

int fl_drop_graph(egr_fatllama_plan* p) {
    if (!p->gexec) return EGR_OK;
    EGR_HIP(hipDeviceSynchronize());
    EGR_HIP(hipGraphExecDestroy(p->gexec));
    p->gexec = nullptr;
    return EGR_OK;
}

extern "C" int egr_fatllama_plan_destroy(egr_fatllama_plan* p) {
    if (!p) return EGR_OK;
    hipDeviceSynchronize();          // nothing of the plan may still be in flight when its graph, streams and buffers go
    fl_drop_graph(p);
    delete p;
    return EGR_OK;
}

// ---- the launchers of the three kernel families (FlRowPass / FlColPass, egr_fatllama_int.h) ----
static void row_launch(const FlRowPass& e, const egr_fatllama_plan* p, const RowP& R, cplx* work, int nch, hipStream_t st) {
    hipLaunchKernelGGL(e.k, dim3(R.R / 2 + 1, nch), dim3(e.threads), e.lds, st, R, (long long)p->sp.M, work);
}
static void row_launch_wl(const FlRowPass& e, const egr_fatllama_plan* p, const RowP& R, cplx* work, int nch, hipStream_t st) {
    hipLaunchKernelGGL(e.k_wl, dim3(R.R / 2 + 1, nch), dim3(e.threads), e.lds, st, R, p->wl_rt, (long long)p->sp.M, work);
}
static dim3 col_grid(const ColP& A, int nch) { return dim3(8 * A.tiles_per_xcd, nch * A.nplanes); }
static void col_launch(const FlColPass& e, const egr_fatllama_plan* p, const ColP& A, const FlColIO& io, cplx* work, int nch, hipStream_t st) {
    hipLaunchKernelGGL(e.k, col_grid(A, nch), dim3(e.threads), e.lds, st, A, (long long)p->sp.M, (long long)p->sp.N, io.thr, work, io.out, io.peak, io.thr_rel);
}
static void col_launch_wl(const FlColPass& e, const egr_fatllama_plan* p, const ColP& A, const FlColIO&, cplx* work, int nch, hipStream_t st) {
    hipLaunchKernelGGL(e.k_wl, col_grid(A, nch), dim3(e.threads), e.lds, st, A, p->wl_ct, (long long)p->sp.M, work);
}
static void inner_launch_wl(const FlColPass& e, const egr_fatllama_plan* p, const ColP& B, const FlColIO&, cplx* work, int nch, hipStream_t st) {
    hipLaunchKernelGGL(e.k_wlb, col_grid(B, nch), dim3(e.threads), e.lds, st, B, p->wl_it, (long long)p->sp.M, work);
}
static FlRowPass row_pass(FlRowFn k, int threads, size_t lds) { FlRowPass e{}; e.launch = row_launch; e.k = k; e.threads = threads; e.lds = lds; return e; }
static FlRowPass row_pass_wl(WlRowFn k, const WlRowEntry& w) { FlRowPass e{}; e.launch = row_launch_wl; e.k_wl = k; e.threads = w.threads; e.lds = EGR_LDS(w.lds); return e; }
static FlColPass col_pass(FlColFn k, int threads, size_t lds, const ColP* geo) {
    FlColPass e{}; e.launch = col_launch; e.k = k; e.threads = threads; e.lds = lds; e.geo = geo; return e;
}

// The one place that knows which kernel serves which pass of a plan.  `families`: the compile-time schedules and the two-barrier
// kernels serve the passes whose tables build_plan uploaded (the plan's lengths have an instantiation and EGR_FL_SCHED / EGR_FL_WL
// allow it); without them every pass runs the run-time schedule at `threads` threads.
static void fl_select_passes(const egr_fatllama_plan* p, int threads, bool families, FlPasses* ps) {
    const FlSplit& sp = p->sp;
    const int L = p->row.L;
    const size_t lc = EGR_LDS(sp.lds_col), lb = EGR_LDS(sp.lds_colb), lr = EGR_LDS(sp.lds_row);
    // the in-place schedules need one thread per butterfly (288 / 512 row, 200 column butterflies per stage): 512 threads; the
    // column one serves two-level plans only
    const bool sched_ok = families && threads == 512;
    // the two-barrier row kernels: default hook, k_row_wl<.., 1> (level from the iteration's maximum and / or soft shrink), maximum only
    if (const WlRowEntry* w = families && p->wl_rt.t1 ? wl_find(kWlRows, L) : nullptr) {
        ps->row[FL_ROW_DEFAULT] = row_pass_wl(w->fn, *w);
        ps->row[FL_ROW_VARIANT] = row_pass_wl(w->fn_variant, *w);
        ps->row[FL_ROW_MAX] = row_pass_wl(w->fn_max, *w);
    } else {
        const bool rs1 = sched_ok && p->row.stw;
        const size_t lds = rs1 ? row_sched_lds(L) : lr;
        ps->row[FL_ROW_DEFAULT] = ps->row[FL_ROW_VARIANT] = row_pass(rs1 ? k_row<false, 1> : k_row<false>, threads, lds);
        ps->row[FL_ROW_MAX] = row_pass(rs1 ? k_row<true, 1> : k_row<true>, threads, lds);
    }
    const ColP* A = &p->colA;
    const bool cs2 = sched_ok && A->stw && sp.levels == 2;          // (at the scheduled column kernels' own workgroup size)
    const FlColFn outer[2][3] = {{k_col<0>, k_col<1>, k_col<2>}, {k_col<0, 2>, k_col<1, 2>, k_col<2, 2>}};      // [cs2][opening, middle, closing]
    for (int m = 0; m < 3; ++m) ps->col[m] = col_pass(outer[cs2][m], cs2 ? EGR_FL_COL_THREADS : threads, cs2 ? col_sched_lds(p) : lc, A);
    if (const WlColEntry* w = families && p->wl_ct.t3 ? wl_find(kWlCols, A->L) : nullptr) {          // the middle pass only
        FlColPass& e = ps->col[FL_COL_MID];
        e.launch = col_launch_wl; e.k_wl = w->fn; e.threads = w->threads; e.lds = EGR_LDS(w->lds); e.geo = &p->wl_colA;
    }
    ps->inner[FL_INNER_FWD] = col_pass(k_col<4>, threads, lb, &p->colB);
    ps->inner[FL_INNER_INV] = col_pass(k_col<3>, threads, lb, &p->colB);
    if (const WlInnerEntry* w = families && p->wl_it ? wl_find(kWlInner, sp.M2) : nullptr)
        for (int fwd = 0; fwd < 2; ++fwd) {
            FlColPass& e = ps->inner[fwd];
            e.launch = inner_launch_wl; e.k_wlb = fwd ? w->fwd : w->inv; e.threads = w->threads; e.lds = EGR_LDS(w->lds); e.geo = &p->wl_colB;
        }
}

// `c` with the tile geometry of a kernel that takes `tc` columns per workgroup by thread index (a ragged last tile is fine)
static ColP retiled(ColP c, int tc) {
    c.TC = tc; c.TClog2 = 0; c.ntiles = ceil_div(c.ncols, tc); c.tiles_per_xcd = ceil_div(c.ntiles, 8);
    return c;
}

// the kernels of this unit whose dynamic LDS may exceed the 64 KiB default
static const void* const kBigLdsKernels[] = {
    (const void*)k_col<0>, (const void*)k_col<1>, (const void*)k_col<2>, (const void*)k_col<3>, (const void*)k_col<4>, (const void*)k_col<5>,
    (const void*)k_row<false>, (const void*)k_row<true>, (const void*)k_row<false, 1>, (const void*)k_row<true, 1>,
    (const void*)k_col<0, 2>, (const void*)k_col<1, 2>, (const void*)k_col<2, 2>,
    (const void*)k_colz<0, 0>, (const void*)k_colz<1, 1>, (const void*)k_colz<1, 2>, (const void*)k_colz<3, 1>, (const void*)k_colz<2, 0>,
    (const void*)k_rowconv<true>, (const void*)k_rowconv<false>,
};

static int build_plan(egr_fatllama_plan** out, const FlSwitches& sw, int64_t n_in, int channels, int factor, const FlSplit& sp,
                      int64_t bluestein_n = 0, int pz_kind = 0, int64_t n_out = 0) {
    // a failed build goes the way of every plan: egr_fatllama_plan_destroy waits for the device before anything is freed
    std::unique_ptr<egr_fatllama_plan, int (*)(egr_fatllama_plan*)> owner(new egr_fatllama_plan(), egr_fatllama_plan_destroy);
    egr_fatllama_plan* p = owner.get();
    p->n_in = n_in; p->C = channels; p->factor = factor; p->sp = sp;
    p->n_out = n_out > 0 ? n_out : n_in * factor;
    p->bluestein = bluestein_n > 0;
    p->pz_kind = pz_kind;
    p->nstreams = sw.streams;
    p->use_graph = sw.graph;
    hipGetDevice(&p->device);
    const int64_t M = sp.M, N = sp.N;
    std::vector<float2> h;
    // ---- outer column pass A: L = M1, columns = M / M1 ----
    ColP& a = p->colA;
    a.f = sp.f1; a.L = sp.M1; a.ncols = (int)(M / sp.M1); a.nplanes = 1;
    a.TC = sp.TC; a.TClog2 = sp.TClog2; a.ntiles = ceil_div(a.ncols, a.TC); a.tiles_per_xcd = ceil_div(a.ntiles, 8);
    make_twiddles(h, sp.M1, 1, sp.M1);
    EGR_TRY(fl_upload(p, h, &a.tw));
    EGR_TRY(fl_upload_d(p, sp.M1, &a.twd));
    EGR_TRY(fl_make_tw2(p, M, &a.big));
    // ---- inner column pass B (3 levels): per k1 plane, L = M2, columns = M3 ----
    RowP& r = p->row;
    if (sp.levels == 3) {
        ColP& b = p->colB;
        b.f = sp.f2; b.L = sp.M2; b.ncols = sp.M3; b.nplanes = sp.M1;
        b.TC = sp.TCb; b.TClog2 = sp.TCblog2; b.ntiles = ceil_div(b.ncols, b.TC); b.tiles_per_xcd = ceil_div(b.ntiles, 8);
        make_twiddles(h, sp.M2, 1, sp.M2);
        EGR_TRY(fl_upload(p, h, &b.tw));
        EGR_TRY(fl_upload_d(p, sp.M2, &b.twd));
        EGR_TRY(fl_make_tw2(p, (int64_t)sp.M2 * sp.M3, &b.big));
        r.f = sp.f3; r.L = sp.M3; r.R = sp.M1 * sp.M2; r.Ma = sp.M1; r.Mb = sp.M2;
    } else {
        r.f = sp.f2; r.L = sp.M2; r.R = sp.M1; r.Ma = sp.M1; r.Mb = 1;
    }
    make_twiddles(h, r.L, 1, r.L);
    EGR_TRY(fl_upload(p, h, &r.tw));
    EGR_TRY(fl_upload_d(p, r.L, &r.twd));
    EGR_TRY(fl_upload_dtab(p, r.L, 1, 2 * (int64_t)r.L, &r.wk));
    {   // W_N^o for o < R, as hi/lo tables over the range [0, R)
        int sh = 0;
        while ((1LL << (2 * sh)) < r.R) ++sh;
        EGR_TRY(fl_upload_dtab(p, ((int64_t)r.R >> sh) + 1, 1LL << sh, N, &r.wo.hi));
        EGR_TRY(fl_upload_dtab(p, 1LL << sh, 1, N, &r.wo.lo));
        r.wo.sh = sh;
    }
    r.inv_M = (float)(1.0 / (double)M);
    r.inv_M_d = 1.0 / (double)M;
    // stage tables of the compile-time schedules for the hot factor lengths (EGR_FL_SCHED=0: always the run-time schedule)
    if (sw.sched && !p->bluestein && r.L == 2304) EGR_TRY(fl_upload_sched_tables(p, {EGR_FL_ROW_RADICES}, &r.stw));
    if (sw.sched && !p->bluestein && a.L == 625 && a.TC >= 2 && a.TC <= EGR_FL_COL_TC) EGR_TRY(fl_upload_sched_tables(p, {EGR_FL_COL_RADICES}, &a.stw));
    // tables of the two-barrier loop kernels (egr_fatllama_wl.h) where the row / outer column / inner column length has an instantiation;
    // EGR_FL_WL=0 keeps the stage-by-stage kernels
    if (sw.wl && !p->bluestein) {
        auto table = [&](int n, int m, int T, const cplx** d, const cplx** dlo) {          // [n][m]: W_T^(i j), and its low parts
            std::vector<float2> t, tl;
            t.resize((size_t)n * m); tl.resize((size_t)n * m);
            const long double two_pi = 6.283185307179586476925286766559L;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < m; ++j) {
                    const long double ang = -two_pi * (long double)(((long long)i * j) % T) / (long double)T;
                    const long double c = cosl(ang), sn = sinl(ang);
                    const float2 h = make_float2((float)c, (float)sn);
                    t[(size_t)i * m + j] = h;
                    tl[(size_t)i * m + j] = make_float2((float)(c - (long double)h.x), (float)(sn - (long double)h.y));
                }
            const int rc2 = fl_upload(p, t, d);
            return rc2 ? rc2 : fl_upload(p, tl, dlo);
        };
        if (const WlRowEntry* e = wl_find(kWlRows, r.L)) {
            const int qq = e->q * e->q;
            EGR_TRY(table(qq, e->n1, e->L, &p->wl_rt.t1, &p->wl_rt.t1l));
            EGR_TRY(table(e->q, e->q, qq, &p->wl_rt.t2, &p->wl_rt.t2l));
            EGR_TRY(fl_upload_dtab(p, e->q, 1, qq, &p->wl_rt.t2d));
            const long double ang = -3.14159265358979323846264338327950288L / (long double)e->q;         // W_(2Q)
            p->wl_rt.hook_step = make_double2((double)cosl(ang), (double)sinl(ang));
        }
        if (const WlColEntry* e = wl_find(kWlCols, a.L)) {
            EGR_TRY(table(e->r, e->r, e->L, &p->wl_ct.t3, &p->wl_ct.t3l));
            p->wl_colA = retiled(a, e->tc);
        }
        if (const WlInnerEntry* e = sp.levels == 3 ? wl_find(kWlInner, sp.M2) : nullptr) {
            const cplx* itl = nullptr;
            EGR_TRY(table(e->lb, e->la, sp.M2, &p->wl_it, &itl));
            p->wl_colB = retiled(p->colB, e->tcw);
        }
    }
    const int nstates = pz_kind == 2 ? (channels + 1) / 2 : channels;      // a paired chirp-z state of kind 2 carries two channels
    EGR_CHECK(p->d_work.alloc((size_t)nstates * M * sizeof(float2)) && p->d_peaks.alloc(3 * channels * sizeof(unsigned)), EGR_ERR_ALLOC,
              "hipMalloc of the %lld-byte loop state failed", (long long)(channels * M * 8));
    // dynamic LDS above the 64 KiB default needs an explicit opt-in per kernel.  The attribute is a process-wide cap per kernel, so it
    // is always raised to the CU's 160 KiB (a later, smaller plan must not lower it under an earlier plan's needs); what a plan
    // actually requests is checked here.
    EGR_CHECK(pz_kind || (std::max(sp.lds_col, sp.lds_colb) <= (size_t)EGR_LDS_MAX && sp.lds_row <= (size_t)EGR_LDS_MAX), EGR_ERR_UNSUPPORTED,
              "plan needs %zu / %zu bytes of LDS per workgroup (limit %d)", std::max(sp.lds_col, sp.lds_colb), sp.lds_row, EGR_LDS_MAX);
    for (const void* k : kBigLdsKernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, EGR_LDS_MAX);
        EGR_CHECK(e == hipSuccess, EGR_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) -> %s", hipGetErrorString(e));
    }
    fl_select_passes(p, 256, false, &p->single);
    p->single.col[FL_COL_CLOSE].k = k_col<5>;          // a single pass ends plain: out = d, not y + d
    if (p->pz_kind) {
        EGR_TRY(pz_build(p, p->pz_kind, sw));
    } else if (p->bluestein) {
        // chirp tables for W_(2N)^r and bhat = FFT_P(b)/P computed once with the plan's own passes
        ChirpP& c = p->chirp;
        c.N = (unsigned long long)bluestein_n;
        c.inv_N = (float)(1.0 / (double)bluestein_n);
        c.inv_2N_d = 1.0 / (2.0 * (double)bluestein_n);
        EGR_TRY(fl_make_tw2(p, 2 * bluestein_n, &c.w));
        EGR_CHECK(p->d_bhat.alloc((size_t)M * sizeof(float2)), EGR_ERR_ALLOC, "hipMalloc of the %lld-byte chirp spectrum failed", (long long)(M * 8));
        cplx* bhat = p->d_bhat.as<cplx>();
        const FlColIO none{0.f, nullptr, nullptr, nullptr};
        hipLaunchKernelGGL(k_chirp_b, dim3(2048), dim3(256), 0, 0, c, (long long)M, bhat);
        col_pass(k_col<4>, 256, EGR_LDS(sp.lds_col), &a)(p, none, bhat, 1, 0);          // the forward pass over the OUTER columns too
        if (sp.levels == 3) p->single.inner[FL_INNER_FWD](p, none, bhat, 1, 0);
        hipLaunchKernelGGL(k_rowconv<false>, dim3((r.R + EGR_FL_CONV_ROWS - 1) / EGR_FL_CONV_ROWS, 1), dim3(EGR_FL_CONV_THREADS), rowconv_lds(r.L), 0, r.f, r.L, r.R, r.tw,
                           (const cplx*)nullptr, (float)(1.0 / (double)M), (long long)M, bhat);
        EGR_CHECK(hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess, EGR_ERR_HIP, "building the Bluestein chirp spectrum failed");
    }
    // stage twiddles W^2..W^(r-1) by multiplication from one loaded W^1 (default) or all loaded (EGR_FL_TWPOW=0)
    p->colA.f.tw_pow = p->wl_colA.f.tw_pow = p->colB.f.tw_pow = p->row.f.tw_pow = sw.twpow;
    fl_select_passes(p, sw.threads, true, &p->loop);
    *out = owner.release();
    return EGR_OK;
}

// smallest P >= want whose packed plan (M = P) exists; P has only the prime factors 2, 3, 5, 7
static bool bluestein_length(int64_t want, FlSplit* sp_out) {
    // smallest cost, not smallest length: a three-level plan runs ~1.6x the passes of a two-level one per transform
    int64_t best = -1;
    double best_cost = 1e300;
    FlSplit best_sp;
    for (int64_t p7 = 1; p7 <= 8 * want; p7 *= 7)
        for (int64_t p5 = p7; p5 <= 8 * want; p5 *= 5)
            for (int64_t p3 = p5; p3 <= 8 * want; p3 *= 3) {
                int64_t v = p3;
                while (v < want) v *= 2;
                for (int rep = 0; rep < 2; ++rep, v *= 2) {          // v and 2v: the first may not factor into tiles
                    if ((double)v >= best_cost) break;
                    FlSplit sp = plan_split(2 * v, 0, 0, 2048);
                    if (!sp.ok) continue;
                    const double cost = (double)v * (sp.levels == 3 ? 1.6 : 1.0);
                    if (cost < best_cost) { best_cost = cost; best = v; best_sp = sp; }
                    break;
                }
            }
    if (best < 0) return false;
    *sp_out = best_sp;
    return true;
}

// Convolution length and factorisation of a paired chirp-z plan for a length-D complex transform: P = L x nc >= 2 D - 1 with
// nc % 8 == 0 (4-column tiles in mirrored pairs), rows of at most 4096 points (one row per workgroup, stages in place), columns
// of at most 2048; smallest cost, where a plan whose column-tile pair does not fit one in-place call (L > 1024) and a third level
// pay their extra barriers / passes.
static bool pz_length(int64_t D, const FlSwitches& sw, FlSplit* sp_out) {
    const int64_t want = 2 * D - 1;
    const int64_t limit = want < 64 ? 4096 : want + want / 2;
    {   // dev: EGR_PZ_SPLIT="L,nc" forces the factorisation (unset: 0 x 0, shorter than any `want`)
        const int L = sw.pz_split_L, nc = sw.pz_split_nc;
        if ((int64_t)L * nc >= want && nc % 8 == 0) {
            FlSplit sp = plan_split_explicit(2 * (int64_t)L * nc, L, nc, 1, 4);
            if (sp.ok && sp.TC == 4) { *sp_out = sp; return true; }
        }
    }
    std::vector<int64_t> cand;                    // 13-smooth numbers in [want, limit]
    {
        const int primes[6] = {2, 3, 5, 7, 11, 13};
        std::vector<int64_t> cur{1};
        for (int pi = 0; pi < 6; ++pi) {
            std::vector<int64_t> next;
            for (int64_t v : cur)
                for (int64_t x = v; x <= limit; x *= primes[pi]) next.push_back(x);
            cur.swap(next);
        }
        for (int64_t v : cur) if (v >= want && v >= 8) cand.push_back(v);
        std::sort(cand.begin(), cand.end());
    }
    double best_cost = 1e300;
    FlSplit best;
    best.ok = false;
    for (int64_t v : cand) {
        if ((double)v >= best_cost) break;
        // two levels
        double c2 = 1e300;
        int bl = 0;
        for (int64_t L = 1; L <= 2048 && L <= v; ++L) {
            if (v % L) continue;
            const int64_t nc = v / L;
            if (nc % 8) continue;
            const bool sched = nc <= 16384 && sw.pz_sched && pz_sched_has((int)L, (int)nc);       // compile-time schedules on both passes
            if (nc > 4096 && !sched) continue;
            FftDesc f1, f2;
            if (!make_schedule((int)L, &f1) || !make_schedule((int)nc, &f2)) continue;
            double c = (double)v * (1.0 + 0.02 * (f1.nst + f2.nst));
            if (L > 1024) c *= 1.15;
            if (sched) c *= 0.55;
            if (c < c2) { c2 = c; bl = (int)L; }
        }
        if (bl) {
            if (c2 < best_cost) {
                FlSplit sp = plan_split_explicit(2 * v, bl, (int)(v / bl), 1, 4, 16384);
                if (sp.ok && sp.TC == 4) { best_cost = c2; best = sp; }
            }
            continue;
        }
        if (v <= 1024LL * 16384LL) continue;
        FlSplit sp = plan_split(2 * v, 0, 4, 2048);
        if (!sp.ok || sp.levels != 3 || sp.TC != 4 || ((int64_t)sp.M2 * sp.M3) % 8) continue;
        const double c3 = (double)v * 1.6;
        if (c3 < best_cost) { best_cost = c3; best = sp; }
    }
    if (!best.ok) return false;
    *sp_out = best;
    return true;
}

static int create_for_length(egr_fatllama_plan** out, int64_t n_in, int channels, int factor, int64_t N, int m1_hint, int tc_hint) {
    const FlSwitches sw = fl_read_switches();
    if (m1_hint <= 0) m1_hint = sw.m1;
    if (tc_hint <= 0) tc_hint = sw.tc;
    FlSplit sp = plan_split(N, m1_hint, tc_hint);
    // the 625-point column schedule is instantiated for one tile width
    if (tc_hint <= 0 && sp.ok && sp.levels == 2 && sp.M1 == 625 && sp.TC != EGR_FL_COL_TC) sp = plan_split(N, m1_hint, EGR_FL_COL_TC);
    if (!sp.ok) {
        const int kind = pz_kind_for(N);
        const int64_t D = kind == 1 ? N / 2 : N;
        if (N >= 2 && !sw.legacy_chirpz && pz_length(D, sw, &sp)) return build_plan(out, sw, n_in, channels, factor, sp, D, kind, N);
        if (N >= 2 && bluestein_length(2 * N - 1, &sp)) return build_plan(out, sw, n_in, channels, factor, sp, N, 0, N);
        set_error(kUnsupported, (long long)N);
        return EGR_ERR_UNSUPPORTED;
    }
    return build_plan(out, sw, n_in, channels, factor, sp, 0, 0, N);
}

// The preamble of the egr_fatllama_plan_create* entry points: `out` reset, sizes in range (the chirp-z ones need n_in * factor >= 2;
// egr_fatllama_plan_create_n gives its output length instead of a factor).
static int create_check(egr_fatllama_plan** out, int64_t n_in, int channels, int factor, int64_t min_n, const int64_t* n_out = nullptr) {
    EGR_CHECK(out != nullptr, EGR_ERR_ARG, "out is null");
    *out = nullptr;
    if (n_out) {
        EGR_CHECK(n_in >= 1 && *n_out >= n_in && channels >= 1 && channels <= 64, EGR_ERR_ARG,
                  "n_in=%lld n_out=%lld channels=%d out of range", (long long)n_in, (long long)*n_out, channels);
        return EGR_OK;
    }
    EGR_CHECK(n_in >= 1 && factor >= 1 && channels >= 1 && channels <= 64 && n_in * factor >= min_n, EGR_ERR_ARG,
              "n_in=%lld channels=%d factor=%d out of range", (long long)n_in, channels, factor);
    return EGR_OK;
}

extern "C" int egr_fatllama_plan_create(egr_fatllama_plan** out, int64_t n_in, int channels, int factor,
                                        int m1_hint, int tc_hint) {
    if (int rc = create_check(out, n_in, channels, factor, 1)) return rc;
    return create_for_length(out, n_in, channels, factor, n_in * factor, m1_hint, tc_hint);
}

// A plan whose output length is given explicitly (n_out >= n_in, not necessarily a multiple of it): SPEC.md factor_mode
// "ratio_then_int".  egr_fatllama_enhance on such a plan needs EGR_FL_INTERP_LINSPACE (the only up-rating defined for a ratio).
extern "C" int egr_fatllama_plan_create_n(egr_fatllama_plan** out, int64_t n_in, int64_t n_out, int channels) {
    if (int rc = create_check(out, n_in, channels, 0, 0, &n_out)) return rc;
    return create_for_length(out, n_in, channels, 0, n_out, 0, 0);
}

// Force a chirp-z plan on any length (tests, A/B runs): kind 1 = paired, even/odd packing (N even); 2 = paired, channel pairs
// (any N); 3 = the legacy full-complex form (one P >= 2N - 1 state per channel).
extern "C" int egr_fatllama_plan_create_chirpz(egr_fatllama_plan** out, int64_t n_in, int channels, int factor, int kind) {
    if (int rc = create_check(out, n_in, channels, factor, 2)) return rc;
    const int64_t N = n_in * factor;
    if (kind == 0) kind = pz_kind_for(N);
    if (kind == 3) return egr_fatllama_plan_create_bluestein(out, n_in, channels, factor);
    EGR_CHECK(kind == 2 || (kind == 1 && !(N & 1)), EGR_ERR_ARG, "chirp-z kind %d does not fit N=%lld", kind, (long long)N);
    FlSplit sp;
    const int64_t D = kind == 1 ? N / 2 : N;
    const FlSwitches sw = fl_read_switches();
    if (!pz_length(D, sw, &sp)) {
        set_error("no convolution length found for D=%lld", (long long)D);
        return EGR_ERR_UNSUPPORTED;
    }
    return build_plan(out, sw, n_in, channels, factor, sp, D, kind);
}

extern "C" int egr_fatllama_plan_create_bluestein(egr_fatllama_plan** out, int64_t n_in, int channels, int factor) {
    if (int rc = create_check(out, n_in, channels, factor, 2)) return rc;
    const int64_t N = n_in * factor;
    FlSplit sp;
    if (!bluestein_length(2 * N - 1, &sp)) {
        set_error("no convolution length found for N=%lld", (long long)N);
        return EGR_ERR_UNSUPPORTED;
    }
    return build_plan(out, fl_read_switches(), n_in, channels, factor, sp, N);
}

extern "C" int egr_fatllama_plan_create_ex(egr_fatllama_plan** out, int64_t n_in, int channels, int factor, int m1,
                                           int m2, int m3, int tc_hint) {
    if (int rc = create_check(out, n_in, channels, factor, 1)) return rc;
    FlSplit sp = plan_split_explicit(n_in * factor, m1, m2, m3, tc_hint);
    if (!sp.ok) {
        set_error("explicit split %d x %d x %d does not fit N=%lld", m1, m2, m3, (long long)(n_in * factor));
        return EGR_ERR_UNSUPPORTED;
    }
    return build_plan(out, fl_read_switches(), n_in, channels, factor, sp);
}

// dev: one k_row and one k_col<1> launch over the plan's state with per-workgroup phase stamps (100 MHz wall clock);
// prints min / median / max of each phase in microseconds and the launch skew.  Not part of the public header.
extern "C" int egr_fatllama_trace_once(egr_fatllama_plan* p, void* stream) {
    EGR_CHECK(p && !p->bluestein, EGR_ERR_ARG, "packed plan wanted");
    hipStream_t st = (hipStream_t)stream;
    const int C = p->C;
    // through the loop's own selection: the kernels, workgroup sizes and tile geometry an iteration launches
    const FlRowPass& row = p->loop.row[FL_ROW_DEFAULT];
    const FlColPass& mid = p->loop.col[FL_COL_MID];
    ColP A = *mid.geo; RowP R = p->row;
    R.thr2 = 0.36f; R.thr = 0.6f;
    const dim3 gA = col_grid(A, C), grow(R.R / 2 + 1, C);
    const size_t nblk = (size_t)std::max(gA.x * gA.y, grow.x * grow.y);
    DevBuf trbuf;
    EGR_CHECK(trbuf.alloc(nblk * 8 * sizeof(long long)), EGR_ERR_HIP, "hipMalloc of %zu trace stamps failed", nblk * 8);
    long long* tr = trbuf.as<long long>();
    std::vector<long long> h(nblk * 8);
    for (int which = 0; which < 2; ++which) {
        EGR_HIP(hipMemsetAsync(tr, 0, nblk * 8 * sizeof(long long), st));
        R.trace = tr; A.trace = tr;
        for (int rep = 0; rep < 3; ++rep) {          // the last repetition's stamps survive
            if (which == 0) row(p, R, p->work(), C, st);
            else mid.launch(mid, p, A, FlColIO{0.6f, nullptr, nullptr, nullptr}, p->work(), C, st);
        }
        EGR_HIP(hipStreamSynchronize(st));
        EGR_HIP(hipMemcpy(h.data(), tr, nblk * 8 * sizeof(long long), hipMemcpyDeviceToHost));
        const size_t nb = which == 0 ? (size_t)grow.x * grow.y : (size_t)gA.x * gA.y;
        const int nph = which == 0 ? 5 : 4;
        long long t0 = -1, t1 = 0;
        std::vector<std::vector<double>> ph(nph);
        std::vector<double> starts;
        for (size_t b = 0; b < nb; ++b) {
            const long long* s = &h[b * 8];
            if (s[0] == 0) continue;
            if (t0 < 0 || s[0] < t0) t0 = s[0];
            if (s[nph] > t1) t1 = s[nph];
            for (int i = 0; i < nph; ++i) ph[i].push_back((s[i + 1] - s[i]) * 0.01);
            starts.push_back((double)s[0]);
        }
        printf("%s: %zu workgroups stamped, first start -> last end %.2f us\n", which == 0 ? "k_row" : "k_col<1>", starts.size(), (t1 - t0) * 0.01);
        std::sort(starts.begin(), starts.end());
        if (!starts.empty()) printf("   start skew: median %.2f us, max %.2f us after the first\n", (starts[starts.size() / 2] - starts[0]) * 0.01, (starts.back() - starts[0]) * 0.01);
        static const char* rn[5] = {"load", "fwd fft", "hook", "inv fft", "store"};
        static const char* cn[4] = {"load+tw", "inv fft", "fwd fft", "tw+store"};
        for (int i = 0; i < nph; ++i) {
            auto& v = ph[i];
            if (v.empty()) continue;
            std::sort(v.begin(), v.end());
            printf("   %-9s min %.2f  median %.2f  max %.2f us\n", which == 0 ? rn[i] : cn[i], v[0], v[v.size() / 2], v.back());
        }
    }
    return EGR_OK;
}

extern "C" int egr_fatllama_set_profiling(egr_fatllama_plan* p, int enable) {
    EGR_CHECK(p != nullptr, EGR_ERR_ARG, "plan is null");
    p->profiling = enable != 0;
    return EGR_OK;
}

void fl_prof_begin(egr_fatllama_plan* p, int kind, hipStream_t st, size_t* slot) {
    if (!p->profiling) return;
    if (*slot >= p->ev.size()) {
        p->ev.emplace_back();
        p->ev.back().create();
        p->ev_kind.push_back(kind);
    } else {
        p->ev_kind[*slot] = kind;
    }
    hipEventRecord(p->ev[*slot].a, st);
}
void fl_prof_end(egr_fatllama_plan* p, hipStream_t st, size_t* slot) {
    if (!p->profiling) return;
    hipEventRecord(p->ev[*slot].b, st);
    *slot += 1;
}

// k_finalize over `out`, or (out == nullptr) one workgroup that only leaves the joint peak in joint_out
static void launch_finalize(egr_fatllama_plan* p, float* out, unsigned flags, const float* joint_in, float* joint_out, hipStream_t st) {
    const long long Nr = out ? (long long)p->n_out : 0LL;
    hipLaunchKernelGGL(k_finalize, out ? dim3(fl_grid(Nr), p->C) : dim3(1, 1), dim3(out ? 256 : 64), 0, st, out, Nr, p->C, flags, p->peaks(),
                       p->peaks() + p->C, joint_in, joint_out);
}

// Argument and flag checks; clears the peaks and the ring of spectrum maxima of the relative threshold.
static int enhance_begin(FlCall& c, const float* x) {
    egr_fatllama_plan* p = c.p;
    EGR_CHECK(p && x && c.out, EGR_ERR_ARG, "null plan/x/out");
    EGR_CHECK(c.max_iter >= 0, EGR_ERR_ARG, "max_iter=%d < 0", c.max_iter);
    const bool lin = (c.flags & EGR_FL_INTERP_LINSPACE) != 0;
    EGR_CHECK(lin || p->factor >= 1, EGR_ERR_ARG, "a plan with an explicit output length (egr_fatllama_plan_create_n) needs EGR_FL_INTERP_LINSPACE");
    EGR_CHECK(!(lin && (c.flags & EGR_FL_ZERO_STUFF)), EGR_ERR_ARG, "EGR_FL_INTERP_LINSPACE and EGR_FL_ZERO_STUFF exclude each other");
    const int C = p->C;
    c.soft = (c.flags & EGR_FL_THR_SOFT) ? 1 : 0;
    c.relative = (c.flags & EGR_FL_THR_RELATIVE) != 0;
    // EGR_FL_THR_RECOMPUTE: the maximum of every iteration's spectrum from a read-only pass of its own (rounds 1-5) instead of the
    // one the previous iteration's hook carried forward; the two agree to the round-off of one float32 transform pair
    c.recompute = c.relative && (c.flags & EGR_FL_THR_RECOMPUTE) != 0;
    const bool no_init = (c.flags & EGR_FL_NO_INIT_THR) != 0;
    c.thr0 = no_init ? -1.0f : c.thr;
    c.thr0_rel = (c.relative && !no_init) ? p->peaks() + 2 * C : nullptr;
    c.peak_out = p->peaks() + C;
    EGR_HIP(hipMemsetAsync(p->peaks(), 0, 3 * C * sizeof(unsigned), c.st));
    if (c.relative && c.max_iter > 0) {
        // the ring of fl_max2_slot; the legacy chirp-z loop keeps one slot per iteration
        const size_t need = fl_max2_words((p->bluestein && !p->pz) ? (size_t)c.max_iter : (size_t)EGR_FL_MAX_RING, C);
        if (need > p->max2_cap) {
            const int rc = fl_drop_graph(p);      // it recorded the old ring
            if (rc) return rc;
            p->max2_cap = 0;
            EGR_CHECK(p->d_max2.alloc(need * sizeof(unsigned)), EGR_ERR_HIP, "hipMalloc of the %zu-word ring of maxima failed", need);
            p->max2_cap = need;
        }
        EGR_HIP(hipMemsetAsync(p->max2(), 0, need * sizeof(unsigned), c.st));
    }
    return EGR_OK;
}

// x -> y in `out` (PCM rounding, up-rating), peaks of x and y
static void launch_prepare(const FlCall& c, const float* x) {
    egr_fatllama_plan* p = c.p;
    hipLaunchKernelGGL(k_prepare, dim3(fl_grid(p->n_in), p->C), dim3(256), 0, c.st, x, c.out, (long long)p->n_in, p->factor > 0 ? p->factor : 1,
                       (c.flags & EGR_FL_PCM_IN) ? 1 : 0, (c.flags & EGR_FL_ZERO_STUFF) ? 1 : 0, p->peaks(), p->peaks() + 2 * p->C,
                       (c.flags & EGR_FL_INTERP_LINSPACE) ? 1 : 0, (long long)p->n_out);
}

// max_iter == 0: the time-domain threshold alone
static int loop_none(const FlCall& c) {
    const long long Nr = (long long)c.p->n_out;
    hipLaunchKernelGGL(k_noiter, dim3(fl_grid(Nr), c.p->C), dim3(256), 0, c.st, c.out, Nr, c.thr0, c.peak_out, c.thr0_rel);
    return EGR_OK;
}

// The inner column pass on the run-time-schedule kernels at `threads` threads: the chirp-z loops bring workgroup sizes of their own.
static void launch_inner_rt(const egr_fatllama_plan* p, bool forward, int threads, const FlColIO& io, cplx* work, int nstates, hipStream_t st) {
    FlColPass e = p->single.inner[forward];
    e.threads = threads;
    e(p, io, work, nstates, st);
}

// The convolution with the chirp of the legacy chirp-z passes: row FFT, times Bhat, inverse row FFT (inside the inner column pass
// of a three-level plan) over all C states.
static void legacy_conv(egr_fatllama_plan* p, dim3 blk, float thr, float* out, unsigned* pk, hipStream_t st) {
    const bool three = p->sp.levels == 3;
    const RowP& R = p->row;
    const dim3 grc((R.R + EGR_FL_CONV_ROWS - 1) / EGR_FL_CONV_ROWS, p->C);
    const FlColIO io{thr, out, pk, nullptr};
    if (three) launch_inner_rt(p, true, blk.x, io, p->work(), p->C, st);
    hipLaunchKernelGGL(k_rowconv<true>, grc, dim3(EGR_FL_CONV_THREADS), rowconv_lds(R.L), st, R.f, R.L, R.R, R.tw, p->d_bhat.as<const cplx>(), 1.0f,
                       (long long)p->sp.M, p->work());
    if (three) launch_inner_rt(p, false, blk.x, io, p->work(), p->C, st);
}

// The legacy full-complex chirp-z loop: one state of P >= 2N - 1 points per channel, one stream, plain launches.
static int loop_legacy_chirpz(const FlCall& c) {
    egr_fatllama_plan* p = c.p;
    const int C = p->C;
    hipStream_t st = c.st; float* out = c.out; unsigned* peak_out = c.peak_out;
    const float thr = c.thr, thr2 = thr * thr;
    const long long P = p->sp.M;
    const ColP& A = p->colA;
    ChirpP cp = p->chirp;
    cp.soft = c.soft;
    const dim3 gA(8 * A.tiles_per_xcd, C), blk(blue_threads());
    const size_t lc = EGR_LDS(p->sp.lds_col);
    auto conv = [&]() { legacy_conv(p, blk, thr, out, peak_out, st); };
    hipLaunchKernelGGL((k_colz<0, 0>), gA, blk, lc, st, A, cp, P, c.thr0, thr2, p->work(), out, peak_out, c.thr0_rel);
    for (int it = 0; it < c.max_iter; ++it) {
        conv();
        if (c.relative) {                 // this iteration's spectrum maximum first (same pass, no write-back)
            cp.max2_out = p->max2() + fl_max2_words((size_t)it, C);
            hipLaunchKernelGGL((k_colz<3, 1>), gA, blk, lc, st, A, cp, P, thr, thr2, p->work(), out, peak_out, (const unsigned*)nullptr);
            cp.max2 = cp.max2_out;
        }
        hipLaunchKernelGGL((k_colz<1, 1>), gA, blk, lc, st, A, cp, P, thr, thr2, p->work(), out, peak_out);
        conv();
        if (it + 1 < c.max_iter)
            hipLaunchKernelGGL((k_colz<1, 2>), gA, blk, lc, st, A, cp, P, thr, thr2, p->work(), out, peak_out);
    }
    hipLaunchKernelGGL((k_colz<2, 0>), gA, blk, lc, st, A, cp, P, thr, thr2, p->work(), out, peak_out);
    return EGR_OK;
}

// The packed-real loop: two channel groups as concurrent pipelines (fl_run_pipelines), one group's k_row overlapping the
// other's k_col.  Which kernel serves a pass is the plan's choice (p->loop, fl_select_passes).
static int loop_packed(const FlCall& c) {
    egr_fatllama_plan* p = c.p;
    const int C = p->C, max_iter = c.max_iter;
    const long long M = p->sp.M, N = p->sp.N;
    const bool three = p->sp.levels == 3, relative = c.relative, recompute = c.recompute;
    const FlPasses& ps = p->loop;
    RowP R = p->row;
    R.thr2 = c.thr * c.thr;
    R.thr = c.thr;
    R.soft = c.soft;
    const FlRowPass& hook = ps.row[(relative || R.soft != 0) ? FL_ROW_VARIANT : FL_ROW_DEFAULT];
    const int ngroups = (p->nstreams == 2 && C >= 2) ? 2 : 1;
    size_t slot = 0;
    // One group's launches for iterations [it0, it1); `first` adds the opening time-domain pass, `last` the closing one.
    auto run_group = [&](hipStream_t s0, int g, int it0, int it1, bool first, bool last, bool prof) {
        const int c0 = g == 0 ? 0 : C / 2, cn = ngroups == 1 ? C : (g == 0 ? C / 2 : C - C / 2);
        hipStream_t sg = g == 0 ? s0 : p->side.s;
        cplx* wk = p->work() + (size_t)c0 * M;
        const FlColIO io{c.thr, c.out + (size_t)c0 * N, c.peak_out + c0, nullptr};
        auto timed = [&](int kind, const FlColPass& pass) {
            if (prof) fl_prof_begin(p, kind, sg, &slot);
            pass(p, io, wk, cn, sg);
            if (prof) fl_prof_end(p, sg, &slot);
        };
        if (first) {
            ps.col[FL_COL_OPEN](p, FlColIO{c.thr0, io.out, io.peak, c.thr0_rel ? c.thr0_rel + c0 : nullptr}, wk, cn, sg);
            if (three) ps.inner[FL_INNER_FWD](p, io, wk, cn, sg);
        }
        // the spectrum maximum by a pass of its own (forward row transforms + split, no write-back): only the FIRST iteration
        // needs it -- d0 = T0(y) is not the image of a shrunk spectrum -- every later one finds the maximum its predecessor's hook left
        auto max_pass = [&](int it) {
            RowP Rm = R;
            Rm.max2_out = fl_max2_slot(p->max2(), C, it, c0);
            ps.row[FL_ROW_MAX](p, Rm, wk, cn, sg);
        };
        if (first && relative) max_pass(0);
        for (int it = it0; it < it1; ++it) {
            RowP Rg = R;
            if (relative) {
                if (recompute && it > 0) max_pass(it);
                Rg.max2 = fl_max2_slot(p->max2(), C, it, c0);
                Rg.max2_next = recompute ? nullptr : fl_max2_slot(p->max2(), C, it + 1, c0);
                Rg.max2_zero = fl_max2_slot(p->max2(), C, it + 2, c0);
            }
            if (prof) fl_prof_begin(p, 0, sg, &slot);
            hook(p, Rg, wk, cn, sg);
            if (prof) fl_prof_end(p, sg, &slot);
            if (three) timed(2, ps.inner[FL_INNER_INV]);
            if (it + 1 < max_iter) {
                timed(1, ps.col[FL_COL_MID]);
                if (three) timed(2, ps.inner[FL_INNER_FWD]);
            }
        }
        if (last) ps.col[FL_COL_CLOSE](p, io, wk, cn, sg);
    };
    // every iteration is a middle iteration (the maximum pass of the relative threshold belongs to the opening pass);
    // EGR_FL_THR_RECOMPUTE uses plain launches
    return fl_run_pipelines(p, c.st, ngroups, max_iter, 0, !recompute, c.thr, R.soft | (relative ? 2 : 0), run_group);
}

extern "C" int egr_fatllama_enhance(egr_fatllama_plan* p, const float* x, float* out, int max_iter, float thr,
                                    unsigned flags, void* stream) {
    FlCall c{p, out, max_iter, thr, flags, (hipStream_t)stream};
    int rc = enhance_begin(c, x);
    if (rc) return rc;
    launch_prepare(c, x);
    rc = max_iter == 0 ? loop_none(c) : p->pz ? pz_loop(c) : p->bluestein ? loop_legacy_chirpz(c) : loop_packed(c);
    if (rc) return rc;
    if ((flags & (EGR_FL_NORMALIZE | EGR_FL_AUTOSCALE | EGR_FL_NODE_POST)) && !(flags & EGR_FL_DEFER_FINALIZE))
        launch_finalize(p, out, flags, nullptr, nullptr, c.st);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

// Channel-parallel runs (the Fat-Llama path shards over channels only; C = 2 => at most 2 GPUs, nothing is
// exchanged until the joint normalise): every rank runs egr_fatllama_enhance on ITS channels with EGR_FL_DEFER_FINALIZE, asks for its
// joint peak (a device float), the host all-reduces that one float with MAX, and egr_fatllama_finalize applies autoscale / normalise /
// write patch / PCM_16 with the all-reduced value.  `flags` as given to enhance.
extern "C" int egr_fatllama_joint_peak(egr_fatllama_plan* p, unsigned flags, float* joint_dev, void* stream) {
    EGR_CHECK(p && joint_dev, EGR_ERR_ARG, "null plan / joint_dev");
    launch_finalize(p, nullptr, flags, nullptr, joint_dev, (hipStream_t)stream);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

extern "C" int egr_fatllama_finalize(egr_fatllama_plan* p, float* out, unsigned flags, const float* joint_dev, void* stream) {
    EGR_CHECK(p && out, EGR_ERR_ARG, "null plan / out");
    if (!(flags & (EGR_FL_NORMALIZE | EGR_FL_AUTOSCALE | EGR_FL_NODE_POST))) return EGR_OK;
    launch_finalize(p, out, flags, joint_dev, nullptr, (hipStream_t)stream);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

// The second pipeline's stream.  HIP multiplexes streams onto a few hardware queues; a side stream that lands on the caller's
// queue serialises the two channel pipelines, so the host may hand in one it has verified (egr_streams_overlap_us).  The plan
// does not own it.  Drops a captured loop graph (it recorded the previous stream).
extern "C" int egr_fatllama_set_side_stream(egr_fatllama_plan* p, void* stream) {
    EGR_CHECK(p && stream, EGR_ERR_ARG, "null plan / stream");
    if (p->side.s == (hipStream_t)stream) return EGR_OK;
    p->side.borrow((hipStream_t)stream);          // (a stream the plan created goes)
    return fl_drop_graph(p);
}

// Replay of the loop from a captured hipGraph on / off (default on unless EGR_FL_GRAPH=0).  The two ways give identical bits;
// which is faster depends on how the runtime maps the graph's branches onto hardware queues, so the host may time both.
extern "C" int egr_fatllama_set_graph(egr_fatllama_plan* p, int enable) {
    EGR_CHECK(p != nullptr, EGR_ERR_ARG, "plan is null");
    p->use_graph = enable ? 1 : 0;
    return EGR_OK;
}

extern "C" int egr_fatllama_last_peaks(egr_fatllama_plan* p, float* host_pin, float* host_pout, void* stream) {
    EGR_CHECK(p && host_pin && host_pout, EGR_ERR_ARG, "null argument");
    std::vector<unsigned> h(2 * p->C);
    EGR_HIP(hipStreamSynchronize((hipStream_t)stream));
    EGR_HIP(hipMemcpy(h.data(), p->peaks(), h.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (int c = 0; c < p->C; ++c) {
        memcpy(&host_pin[c], &h[c], 4);
        memcpy(&host_pout[c], &h[p->C + c], 4);
    }
    return EGR_OK;
}

extern "C" int egr_fatllama_kernel_times3(egr_fatllama_plan* p, double ms_avg[3], int64_t launches[3]) {
    EGR_CHECK(p && ms_avg && launches, EGR_ERR_ARG, "null argument");
    double sum[3] = {0, 0, 0};
    int64_t cnt[3] = {0, 0, 0};
    EGR_HIP(hipDeviceSynchronize());
    for (size_t i = 0; i < p->ev.size() && i < p->ev_kind.size(); ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p->ev[i].a, p->ev[i].b) != hipSuccess) continue;
        const int k = p->ev_kind[i];
        if (k < 0 || k > 2) continue;
        sum[k] += ms;
        cnt[k] += 1;
    }
    for (int k = 0; k < 3; ++k) { ms_avg[k] = cnt[k] ? sum[k] / cnt[k] : 0.0; launches[k] = cnt[k]; }
    return EGR_OK;
}

// The same averages with the inner column pass (3-level plans) reported together with the outer one.
extern "C" int egr_fatllama_kernel_times(egr_fatllama_plan* p, double* row_ms_avg, double* col_ms_avg,
                                         int64_t* row_launches, int64_t* col_launches) {
    EGR_CHECK(p != nullptr, EGR_ERR_ARG, "plan is null");
    double ms[3];
    int64_t cnt[3];
    if (int rc = egr_fatllama_kernel_times3(p, ms, cnt)) return rc;
    const int64_t ncol = cnt[1] + cnt[2];
    if (row_ms_avg) *row_ms_avg = ms[0];
    if (col_ms_avg) *col_ms_avg = ncol ? (ms[1] * cnt[1] + ms[2] * cnt[2]) / ncol : 0.0;
    if (row_launches) *row_launches = cnt[0];
    if (col_launches) *col_launches = ncol;
    return EGR_OK;
}

// inner column pass of a three-level plan over `nstates` consecutive states (used by the chirp-z loops around their row pass)
void fl_launch_inner(egr_fatllama_plan* p, bool forward, cplx* work, int nstates, hipStream_t st) {
    launch_inner_rt(p, forward, 1024, FlColIO{0.f, nullptr, nullptr, nullptr}, work, nstates, st);
}

// One forward transform, the row pass with the hook `R` selects, one inverse, on the run-time-schedule kernels: src -> dst ([C][N] reals
// each; src is only read, by the MODE 0 pass).
// The passes address state `ch` at work + ch M and its samples at src / dst + ch N and take the number of states from the launch, so
// `rows` states in a caller's `work` ([rows][M] complex) run on a plan of any channel count: its tables depend on the length alone.
static void launch_single_pass_rows(egr_fatllama_plan* p, const RowP& R, const float* src, float* dst, cplx* work, int rows, hipStream_t st) {
    const bool three = p->sp.levels == 3;
    const FlPasses& ps = p->single;
    const FlColIO to_dst{0.f, dst, nullptr, nullptr};
    ps.col[FL_COL_OPEN](p, FlColIO{-1.0f, const_cast<float*>(src), nullptr, nullptr}, work, rows, st);
    if (three) ps.inner[FL_INNER_FWD](p, to_dst, work, rows, st);
    ps.row[FL_ROW_DEFAULT](p, R, work, rows, st);
    if (three) ps.inner[FL_INNER_INV](p, to_dst, work, rows, st);
    ps.col[FL_COL_CLOSE](p, to_dst, work, rows, st);
}
static void launch_single_pass(egr_fatllama_plan* p, const RowP& R, const float* src, float* dst, hipStream_t st) {
    launch_single_pass_rows(p, R, src, dst, p->work(), p->C, st);
}

// y = irfft(rfft(x) * gain): one forward transform, a real per-bin gain, one inverse, on the plan's passes.
extern "C" int egr_spectral_gain(egr_fatllama_plan* p, const float* x, const float* gain, float* y, void* stream) {
    EGR_CHECK(p && x && gain && y, EGR_ERR_ARG, "null argument");
    EGR_CHECK(!p->bluestein && p->factor == 1, EGR_ERR_UNSUPPORTED, "spectral gain needs a packed-real plan with factor 1");
    RowP R = p->row;
    R.gain = gain;
    R.phat = 0;
    launch_single_pass(p, R, x, y, (hipStream_t)stream);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

// y = irfft(rfft(x) * [k >= band_lo]) per channel: the brick-wall high band of x at ITS OWN length (any plan kind, factor 1).
// Serves the null-test suite's _band_energy_hi_db (egregora_null_test_suite.py:192-199): by Parseval the band energies of the
// length-N rfft follow from time-domain sums over x and y (egr_band_sums).
extern "C" int egr_band_filter(egr_fatllama_plan* p, const float* x, int64_t band_lo, float* y, void* stream) {
    EGR_CHECK(p && x && y && band_lo >= 0, EGR_ERR_ARG, "bad argument");
    EGR_CHECK(p->factor == 1, EGR_ERR_UNSUPPORTED, "band filter needs a plan with factor 1");
    hipStream_t st = (hipStream_t)stream;
    if (p->pz) return pz_band_filter(p, x, band_lo, y, st);
    RowP R = p->row;
    R.gain = nullptr; R.phat = 0; R.band = 1; R.band_lo = band_lo;
    if (!p->bluestein) {
        launch_single_pass(p, R, x, y, st);
    } else {
        const int C = p->C;
        const long long P = p->sp.M;
        const ColP& A = p->colA;
        const dim3 gA(8 * A.tiles_per_xcd, C), blk(256);
        const size_t lc = EGR_LDS(p->sp.lds_col);
        float* xs = const_cast<float*>(x);          // read only (MODE 0 pass)
        ChirpP cp = p->chirp;
        cp.band = 1; cp.band_lo = (unsigned long long)band_lo;
        unsigned* pk = p->peaks() + C;
        auto conv = [&]() { legacy_conv(p, blk, 0.f, y, pk, st); };
        hipLaunchKernelGGL((k_colz<0, 0>), gA, blk, lc, st, A, cp, P, -1.0f, 0.f, p->work(), xs, pk);
        conv();
        hipLaunchKernelGGL((k_colz<1, 1>), gA, blk, lc, st, A, cp, P, 0.f, 0.f, p->work(), y, pk);
        conv();
        EGR_HIP(hipMemsetAsync(y, 0, (size_t)C * cp.N * sizeof(float), st));      // the closing pass adds d to what y holds
        hipLaunchKernelGGL((k_colz<2, 0>), gA, blk, lc, st, A, cp, P, 0.f, 0.f, p->work(), y, pk);
    }
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// GCC-PHAT delay estimate on the same transform passes (reference _xcorr_delay, egregora_null_test_suite.py:213-237):
// z = a + i b (zero-padded to n = 2^k >= len(a) + len(b)) is the packed state of a plan for N = 2n "real" samples; the row
// pass's hook turns it into the PHAT-weighted cross-spectrum, the inverse passes return the correlation in the real parts.
namespace egr {

__global__ __launch_bounds__(256) void k_phat_pack(const float* __restrict__ a, long long na, const float* __restrict__ b,
                                                    long long nb, long long n, float2* __restrict__ z) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        z[i] = make_float2(i < na ? a[i] : 0.f, i < nb ? b[i] : 0.f);
}

// cc_c = concat(cc[-(n/2-1):], cc[:n/2+1]), centre = n/2: cc_c[j] = cc[(j + n/2 + 1) mod n].  First maximum of
// cc_c[centre - ms .. centre + ms]; out = {index (int bits), cc_c[idx-1], cc_c[idx], cc_c[idx+1]}.  ONE workgroup of 1024 threads;
// k_phat_peak and k_phat_peak_pairs (egr_nullmany_delays) both call it.
__device__ __forceinline__ void phat_peak_search(const float2* __restrict__ y, long long n, long long ms, float* __restrict__ out4) {
    __shared__ float bv[1024];
    __shared__ long long bi[1024];
    const long long centre = n / 2, sl = centre - ms, cnt = 2 * ms + 1;
    float best = -INFINITY;
    long long besti = sl;
    for (long long t = threadIdx.x; t < cnt; t += 1024) {
        const long long j = sl + t;
        const float v = y[(j + n / 2 + 1) % n].x;
        if (v > best) { best = v; besti = j; }          // ascending t per thread: keeps the first maximum
    }
    bv[threadIdx.x] = best;
    bi[threadIdx.x] = besti;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const float v2 = bv[threadIdx.x + o];
            const long long i2 = bi[threadIdx.x + o];
            if (v2 > bv[threadIdx.x] || (v2 == bv[threadIdx.x] && i2 < bi[threadIdx.x])) { bv[threadIdx.x] = v2; bi[threadIdx.x] = i2; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const long long idx = bi[0];
        out4[0] = __int_as_float((int)(idx - centre));
        const bool inner = idx >= 1 && idx < n - 1;
        out4[1] = inner ? y[(idx - 1 + n / 2 + 1) % n].x : 0.f;
        out4[2] = y[(idx + n / 2 + 1) % n].x;
        out4[3] = inner ? y[(idx + 1 + n / 2 + 1) % n].x : 0.f;
    }
}

__global__ __launch_bounds__(1024) void k_phat_peak(const float2* __restrict__ y, long long n, long long ms,
                                                     float* __restrict__ out4) {
    phat_peak_search(y, n, ms, out4);
}

// ---- many pairs of one transform length (egr_nullmany_delays).  tab: ND_COLS int64 per pair (egr_null_index.h) ----
// One workgroup per 256-sample tile of one pair's row of z: z[pair][i] = (mono a[i], mono b[i]) below the pair's common length, zero
// above; the downmix is mono_mean's (what egr_mono_mean would have stored first).
__global__ __launch_bounds__(256) void k_phat_pack_pairs(const float* __restrict__ a, const float* __restrict__ b,
                                                         const long long* __restrict__ tab, long long n, float2* __restrict__ z) {
    long long first;
    const int p = delays_tile_of(n, (long long)blockIdx.x, &first);
    const long long* e = tab + (size_t)p * ND_COLS;
    const long long i = first + threadIdx.x;
    if (i >= n) return;
    float2 v = make_float2(0.f, 0.f);
    if (i < e[ND_N]) {
        v.x = mono_mean(a + e[ND_OFF_A], (int)e[ND_CA], e[ND_LD_A], i);
        v.y = mono_mean(b + e[ND_OFF_B], (int)e[ND_CB], e[ND_LD_B], i);
    }
    z[(size_t)p * n + i] = v;
}

// one workgroup per pair: k_phat_peak's search on the pair's correlation within its own max_shift
__global__ __launch_bounds__(1024) void k_phat_peak_pairs(const float2* __restrict__ y, const long long* __restrict__ tab, long long n,
                                                           float* __restrict__ out4) {
    phat_peak_search(y + (size_t)blockIdx.x * n, n, tab[(size_t)blockIdx.x * ND_COLS + ND_MS], out4 + (size_t)blockIdx.x * 4);
}

}  // namespace egr

using namespace egr;

// plan: egr_fatllama_plan_create(&plan, 2 n, 1, 1, ...) with n = 2^k >= na + nb; work: 4 n floats of device memory
// (z and the correlation, interleaved pairs); out4 (device, 4 floats): {peak index - n/2 as int bits, y0, y1, y2}.
extern "C" int egr_gcc_phat(egr_fatllama_plan* p, const float* a, int64_t na, const float* b, int64_t nb, int64_t max_shift,
                            float* work, float* out4, void* stream) {
    EGR_CHECK(p && a && b && work && out4 && na >= 1 && nb >= 1, EGR_ERR_ARG, "null / empty argument");
    EGR_CHECK(!p->bluestein && p->factor == 1 && p->C == 1, EGR_ERR_UNSUPPORTED, "GCC-PHAT needs a one-channel packed-real plan");
    const long long n = p->sp.M;
    EGR_CHECK((n & (n - 1)) == 0 && n >= na + nb, EGR_ERR_ARG, "plan length must be 2 n with n = 2^k >= na + nb");
    EGR_CHECK(max_shift >= 0 && max_shift < n / 2 - 1, EGR_ERR_ARG, "max_shift out of range");
    hipStream_t st = (hipStream_t)stream;
    RowP R = p->row;
    R.gain = nullptr;
    R.phat = 1;
    float* z = work;
    float* y = work + 2 * n;
    long long nbk = (n + 255) / 256;
    if (nbk > 4096) nbk = 4096;
    hipLaunchKernelGGL(k_phat_pack, dim3((unsigned)nbk), dim3(256), 0, st, a, (long long)na, b, (long long)nb, n, (float2*)z);
    launch_single_pass(p, R, z, y, st);          // (one channel: the plan's C, checked above)
    hipLaunchKernelGGL(k_phat_peak, dim3(1), dim3(1024), 0, st, (const float2*)y, n, (long long)max_shift, out4);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

// ---- egr_nullmany_delays: egr_gcc_phat for the pairs of one transform length in one pack, one run of the passes, one peak launch ----
namespace {
struct DelaysPlan {
    std::vector<long long> tab;
    long long tiles = 0;
    size_t z_off = 0, y_off = 0, work_off = 0, total = 0;
};
inline size_t nd_align(size_t b) { return (b + 255) & ~(size_t)255; }

// every refusal that needs neither a pointer nor the plan: host arithmetic only
int delays_plan(const int64_t* pairs, int n_pairs, int64_t n, DelaysPlan* P) {
    EGR_CHECK(pairs && n_pairs >= 1, EGR_ERR_ARG, "egr_nullmany_delays: no pairs");
    EGR_CHECK(n >= 4 && (n & (n - 1)) == 0 && n <= (1LL << 40), EGR_ERR_ARG, "egr_nullmany_delays: n=%lld is not a power of two in 4 .. 2^40",
              (long long)n);
    EGR_CHECK(n_pairs <= NULL_MAX_GROUP_ROWS, EGR_ERR_UNSUPPORTED,
              "egr_nullmany_delays: pair %lld: a transform group holds at most %lld rows (gridDim.y of the passes), n_pairs=%d",
              NULL_MAX_GROUP_ROWS, NULL_MAX_GROUP_ROWS, n_pairs);
    P->tab.assign((size_t)n_pairs * ND_COLS, 0);
    for (int p = 0; p < n_pairs; ++p) {
        const int r = delays_fill((const long long*)pairs + (size_t)p * ND_COLS, n, &P->tiles, P->tab.data() + (size_t)p * ND_COLS);
        if (r == NULL_OK) continue;
        const long long* in = (const long long*)pairs + (size_t)p * ND_COLS;
        EGR_CHECK(r != NULL_MAX_SHIFT, EGR_ERR_ARG, "egr_nullmany_delays: pair %d: max_shift out of range (%lld, n = %lld)", p, in[ND_MS], (long long)n);
        EGR_CHECK(r != NULL_LENGTH, EGR_ERR_ARG, "egr_nullmany_delays: pair %d: its common length %lld belongs to the transform length %lld, not %lld",
                  p, in[ND_N], null_transform_length(in[ND_N]), (long long)n);
        EGR_CHECK(false, r == NULL_TOTAL ? EGR_ERR_UNSUPPORTED : EGR_ERR_ARG, "egr_nullmany_delays: pair %d: %s", p,
                  r == NULL_SHORT ? "a common length below 1 (an empty side)" : r == NULL_BAD_ROW ? "channels outside 1 .. 65535 or a row stride below n"
                  : r == NULL_OFFSET ? "an offset, stride or length is negative or past what the index type holds"
                                     : "the running total of pack tiles leaves one grid (workgroups x threads < 2^32)");
    }
    const size_t row = (size_t)n * sizeof(float2);
    P->z_off = nd_align(P->tab.size() * sizeof(long long));
    P->y_off = P->z_off + nd_align((size_t)n_pairs * row);
    P->work_off = P->y_off + nd_align((size_t)n_pairs * row);
    P->total = P->work_off + nd_align((size_t)n_pairs * row);
    return EGR_OK;
}

}  // namespace

extern "C" size_t egr_nullmany_delays_workspace_bytes(const int64_t* pairs, int n_pairs, int64_t n) {
    DelaysPlan P;
    if (delays_plan(pairs, n_pairs, n, &P) != EGR_OK) return 0;
    return P.total;
}

extern "C" int egr_nullmany_delays(egr_fatllama_plan* p, const float* a, const float* b, const int64_t* pairs, int n_pairs, float* out4,
                                   void* ws, size_t ws_bytes, int* launches, void* stream) {
    EGR_CHECK(p != nullptr, EGR_ERR_ARG, "egr_nullmany_delays: null plan");
    EGR_CHECK(!p->bluestein && p->factor == 1 && (p->sp.M & (p->sp.M - 1)) == 0, EGR_ERR_UNSUPPORTED,
              "egr_nullmany_delays needs a packed-real plan for 2 n samples, n a power of two");
    const long long n = p->sp.M;
    DelaysPlan P;
    int rc = delays_plan(pairs, n_pairs, n, &P);
    if (rc) return rc;
    EGR_CHECK(a && b && out4 && ws, EGR_ERR_ARG, "egr_nullmany_delays: null pointer");
    EGR_CHECK(ws_bytes >= P.total, EGR_ERR_ARG, "egr_nullmany_delays: workspace of %zu bytes, %zu needed", ws_bytes, P.total);
    EGR_CHECK(((uintptr_t)ws & 15) == 0, EGR_ERR_ARG, "egr_nullmany_delays: the workspace must be 16-byte aligned (int64 table, complex rows)");
    const long long planes = std::max(p->colA.nplanes, p->sp.levels == 3 ? p->colB.nplanes : 1);
    EGR_CHECK((long long)n_pairs * planes <= NULL_MAX_GROUP_ROWS, EGR_ERR_UNSUPPORTED,
              "egr_nullmany_delays: %d pairs on %lld planes of the plan's column pass exceed gridDim.y", n_pairs, planes);
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    rc = upload_table({{P.tab.data(), P.tab.size() * sizeof(long long)}}, base, st);
    if (rc) return rc;
    const long long* tab = (const long long*)base;
    float* z = (float*)(base + P.z_off);
    float* y = (float*)(base + P.y_off);
    RowP R = p->row;
    R.gain = nullptr;
    R.phat = 1;
    hipLaunchKernelGGL(k_phat_pack_pairs, dim3((unsigned)P.tiles), dim3(256), 0, st, a, b, tab, n, (float2*)z);
    EGR_HIP(hipGetLastError());
    launch_single_pass_rows(p, R, z, y, (cplx*)(base + P.work_off), n_pairs, st);
    EGR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_phat_peak_pairs, dim3((unsigned)n_pairs), dim3(1024), 0, st, (const float2*)y, tab, n, out4);
    EGR_HIP(hipGetLastError());
    if (launches) *launches = 2 + (p->sp.levels == 3 ? 5 : 3);
    return EGR_OK;
}

// ---- EGR_LDS_CANARY (debug builds): guard-band failures since the library was loaded, and a self-test of the guards' placement ----
// ---- waves of clips on one paired chirp-z plan (egr_flmany_*) ----
// Clips whose lengths have no packed plan share the convolution length P of the largest of them (the cyclic convolution is exact for
// any P >= 2 D - 1) and run as states of the same launches; what depends on a clip's own D sits in a row table (PzRowP).
namespace {
struct FlManyClip { int64_t n_in, N; int factor, channels, kind, levels; int64_t D, P_own; int state0, nstates, row0; };
struct FlManyState { int clip, nch, row; int64_t D; PzGeo geo; };
struct FlManyShape {
    std::vector<FlManyClip> clips;
    std::vector<FlManyState> states;
    FlSplit sp{};                 // the wave's plan: pz_length of the largest D
    int kind = 0, rows = 0, gpx = 0, big = -1;      // big: the clip with the largest D
    int bad_clip = -1, reason = 0;
    int64_t bytes = 0, x_total = 0, out_total = 0;
    int distinct = 0;
    bool linspace = false;        // some clip's n_out is not n_in * factor: EGR_FL_INTERP_LINSPACE is required
};
const char* const kFlManyReason[] = {"", "its length has a packed plan", "its chirp-z plan has three levels", "its chirp-z kind differs from clip 0's",
                                     "the wave would exceed 1024 channel rows", "no convolution length for it", "EGR_FL_LEGACY_CHIRPZ is set"};
}  // namespace

// Host only.  rc != EGR_OK: an argument is out of range.  Otherwise shape->bad_clip < 0 says that the clips form one wave.
static int flmany_shape(int n_clips, const int64_t* n_in, const int* factor, const int64_t* n_out, const int* channels, FlManyShape* shape) {
    EGR_CHECK(n_clips >= 1 && n_in && factor && channels, EGR_ERR_ARG, "egr_flmany: %d clips / null array", n_clips);
    const FlSwitches sw = fl_read_switches();
    FlManyShape& w = *shape;
    w.clips.resize((size_t)n_clips);
    auto refuse = [&](int i, int why) { if (w.bad_clip < 0) { w.bad_clip = i; w.reason = why; } };
    int64_t Dmax = 0, rows = 0;
    for (int i = 0; i < n_clips; ++i) {
        FlManyClip& c = w.clips[(size_t)i];
        EGR_CHECK(n_in[i] >= 1 && factor[i] >= 1 && channels[i] >= 1 && (!n_out || n_out[i] == 0 || n_out[i] >= n_in[i]), EGR_ERR_ARG,
                  "egr_flmany: clip %d: n_in=%lld factor=%d channels=%d out of range", i, (long long)n_in[i], factor[i], channels[i]);
        c.n_in = n_in[i]; c.factor = factor[i]; c.channels = channels[i];
        c.N = (n_out && n_out[i] > 0) ? n_out[i] : n_in[i] * factor[i];
        if (c.N != c.n_in * c.factor) { w.linspace = true; c.factor = 1; }
        EGR_CHECK(c.N >= 2, EGR_ERR_ARG, "egr_flmany: clip %d has %lld output samples", i, (long long)c.N);
        rows += c.channels;
        c.kind = 0; c.levels = 0; c.D = 0; c.P_own = 0;
        if (plan_split(c.N, sw.m1, sw.tc).ok) { refuse(i, 1); continue; }
        c.kind = pz_kind_for(c.N);
        c.D = c.kind == 1 ? c.N / 2 : c.N;
        FlSplit sp;
        if (!pz_length(c.D, sw, &sp)) { c.kind = 0; refuse(i, 5); continue; }
        c.P_own = sp.M; c.levels = sp.levels;
        if (sw.legacy_chirpz) refuse(i, 6);
        if (sp.levels != 2) refuse(i, 2);
        if (c.kind != w.clips[0].kind) refuse(i, 3);
        if (c.D > Dmax) { Dmax = c.D; w.big = i; w.sp = sp; }
    }
    w.rows = (int)std::min<int64_t>(rows, 1 << 30);
    if (rows > EGR_FLMANY_MAX_ROWS) refuse(n_clips - 1, 4);
    if (w.bad_clip >= 0) return EGR_OK;
    w.kind = w.clips[0].kind;
    const int nc = (int)(w.sp.M / w.sp.M1);
    std::vector<int64_t> ds;
    int row = 0;
    for (int i = 0; i < n_clips; ++i) {
        FlManyClip& c = w.clips[(size_t)i];
        c.state0 = (int)w.states.size(); c.row0 = row;
        c.nstates = w.kind == 1 ? c.channels : (c.channels + 1) / 2;
        for (int j = 0; j < c.nstates; ++j) {
            FlManyState st;
            st.clip = i; st.D = c.D;
            st.nch = w.kind == 1 ? 1 : std::min(2, c.channels - 2 * j);
            st.row = row + (w.kind == 1 ? j : 2 * j);
            st.geo = pz_row_geometry((unsigned long long)c.D, nc, w.sp.TC);
            w.gpx = std::max(w.gpx, st.geo.g_per_xcd);
            w.states.push_back(st);
        }
        row += c.channels;
        w.x_total += (int64_t)c.channels * c.n_in;
        w.out_total += (int64_t)c.channels * (c.N + (c.N & 1));       // every channel slice starts on an 8-byte boundary (float2 accesses of kind 1)
        ds.push_back(c.D);
    }
    std::sort(ds.begin(), ds.end());
    w.distinct = (int)(std::unique(ds.begin(), ds.end()) - ds.begin());
    const int64_t P = w.sp.M, ns = (int64_t)w.states.size();
    // the states, one chirp spectrum per distinct D, the two double-precision scratch buffers of the build, peaks and tables
    w.bytes = ns * P * 8 + (int64_t)w.distinct * P * 8 + 2 * P * 16 + 3 * 2 * ns * 4 + ns * (int64_t)sizeof(PzRowP) + (int64_t)w.rows * (int64_t)sizeof(FlRagRow);
    return EGR_OK;
}

extern "C" int egr_flmany_query(int n_clips, const int64_t* n_in, const int* factor, const int64_t* n_out, const int* channels, int64_t* info) {
    EGR_CHECK(info != nullptr, EGR_ERR_ARG, "info is null");
    FlManyShape w;
    EGR_TRY(flmany_shape(n_clips, n_in, factor, n_out, channels, &w));
    int64_t total_ch = 0;
    for (const FlManyClip& c : w.clips) total_ch += c.channels;
    memset(info, 0, sizeof(int64_t) * (size_t)(EGR_FLMANY_HEAD + EGR_FLMANY_REC * ((int64_t)n_clips + total_ch)));
    info[0] = w.bad_clip < 0 ? 1 : 0;
    info[6] = w.rows;
    info[10] = w.bad_clip; info[11] = w.reason;
    for (int i = 0; i < n_clips; ++i) {
        const FlManyClip& c = w.clips[(size_t)i];
        int64_t* r = info + EGR_FLMANY_HEAD + EGR_FLMANY_REC * (int64_t)i;
        r[0] = c.kind; r[1] = c.D; r[2] = c.P_own; r[3] = c.levels; r[4] = c.N;
        if (w.bad_clip < 0) { r[5] = c.state0; r[6] = c.nstates; r[7] = c.row0; }
    }
    if (w.bad_clip >= 0) return EGR_OK;
    info[1] = w.kind; info[2] = w.sp.M1; info[3] = w.sp.M / w.sp.M1; info[4] = w.sp.M; info[5] = (int64_t)w.states.size();
    info[7] = w.bytes; info[8] = w.sp.TC; info[9] = w.sp.levels; info[12] = w.gpx; info[13] = w.x_total; info[14] = w.out_total;
    info[15] = w.distinct;
    for (size_t j = 0; j < w.states.size(); ++j) {
        const FlManyState& st = w.states[j];
        int64_t* r = info + EGR_FLMANY_HEAD + EGR_FLMANY_REC * ((int64_t)n_clips + (int64_t)j);
        r[0] = st.clip; r[1] = st.geo.s; r[2] = st.geo.c0; r[3] = st.geo.iDr; r[4] = st.geo.cDr; r[5] = st.geo.G; r[6] = st.D; r[7] = st.nch;
    }
    return EGR_OK;
}

struct egr_flmany {
    egr_fatllama_plan* base = nullptr;      // the plan of the wave's P, kind and state count: kernels, tables, streams, loop graph
    FlManyShape shape;
    std::vector<int64_t> x_off, out_off;    // per channel row, in floats
    egr::DevBuf d_bhat;                     // [distinct D but the largest][P]: the largest D's spectrum is the base plan's own
    egr::DevBuf d_tw;                       // the W_(2D) hi / lo tables of every distinct D
    egr::DevBuf d_rows, d_rag;              // PzRowP per state, FlRagRow per channel row
    int64_t max_n_in = 0, max_n_out = 0;
};

extern "C" int egr_flmany_destroy(egr_flmany* w) {
    if (!w) return EGR_OK;
    egr_fatllama_plan_destroy(w->base);      // (waits for the device: nothing of the wave is in flight when its buffers go)
    delete w;
    return EGR_OK;
}

extern "C" int egr_flmany_create(egr_flmany** out, int n_clips, const int64_t* n_in, const int* factor, const int64_t* n_out, const int* channels) {
    EGR_CHECK(out != nullptr, EGR_ERR_ARG, "out is null");
    *out = nullptr;
    std::unique_ptr<egr_flmany, int (*)(egr_flmany*)> owner(new egr_flmany(), egr_flmany_destroy);
    egr_flmany* w = owner.get();
    FlManyShape& sh = w->shape;
    EGR_TRY(flmany_shape(n_clips, n_in, factor, n_out, channels, &sh));
    EGR_CHECK(sh.bad_clip < 0, EGR_ERR_UNSUPPORTED, "egr_flmany_create: clip %d cannot join the wave: %s", sh.bad_clip, kFlManyReason[sh.reason]);
    const FlSwitches sw = fl_read_switches();
    const int ns = (int)sh.states.size();
    const FlManyClip& big = sh.clips[(size_t)sh.big];
    // the base plan: the largest clip's lengths, one channel per channel row (kind 2: two per state, so that a lone channel keeps its slot)
    const int c_base = sh.kind == 1 ? ns : 2 * ns;
    EGR_TRY(build_plan(&w->base, sw, big.N, c_base, 1, sh.sp, big.D, sh.kind, big.N));
    egr_fatllama_plan* p = w->base;
    EGR_TRY(pz_rows_prepare(p));
    const int64_t P = sh.sp.M;
    // ---- per distinct D: the chirp spectrum (device, double precision, one synchronisation for all) and the W_(2D) tables (one upload) ----
    std::vector<int64_t> ds;
    for (const FlManyClip& c : sh.clips) ds.push_back(c.D);
    std::sort(ds.begin(), ds.end());
    ds.erase(std::unique(ds.begin(), ds.end()), ds.end());
    const size_t nd = ds.size();
    std::vector<double2> tw, part;
    std::vector<size_t> tw_hi(nd), tw_lo(nd);
    std::vector<int> tw_sh(nd);
    for (size_t d = 0; d < nd; ++d) {
        const int64_t T = 2 * ds[d];
        int shb = 0;
        while ((1LL << (2 * shb)) < T) ++shb;          // as fl_make_tw2
        tw_sh[d] = shb;
        tw_hi[d] = tw.size();
        make_twiddles_d(part, (T >> shb) + 1, 1LL << shb, T);
        tw.insert(tw.end(), part.begin(), part.end());
        tw_lo[d] = tw.size();
        make_twiddles_d(part, 1LL << shb, 1, T);
        tw.insert(tw.end(), part.begin(), part.end());
    }
    egr::DevBuf scratch0, scratch1;
    EGR_CHECK(w->d_tw.alloc(tw.size() * sizeof(double2)) && w->d_rows.alloc((size_t)ns * sizeof(PzRowP)) && w->d_rag.alloc((size_t)sh.rows * sizeof(FlRagRow)) &&
              (nd < 2 || (w->d_bhat.alloc((nd - 1) * (size_t)P * sizeof(cplx)) && scratch0.alloc((size_t)P * sizeof(double2)) && scratch1.alloc((size_t)P * sizeof(double2)))),
              EGR_ERR_ALLOC, "egr_flmany_create: hipMalloc of the wave's tables (%zu chirp spectra of %lld points) failed", nd, (long long)P);
    EGR_HIP(hipMemcpy(w->d_tw.p, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice));
    std::vector<const cplx*> bh(nd);
    for (size_t d = 0; d < nd; ++d) {
        if (d + 1 == nd) { bh[d] = pz_plan_bhat(p); continue; }          // the largest D: built by pz_build
        cplx* dst = w->d_bhat.as<cplx>() + d * (size_t)P;
        bh[d] = dst;
        EGR_TRY(pz_bhat_enqueue(p, (unsigned long long)ds[d], scratch0.p, scratch1.p, dst));
    }
    // ---- the row tables ----
    std::vector<FlRagRow> rag((size_t)sh.rows);
    w->x_off.resize((size_t)sh.rows); w->out_off.resize((size_t)sh.rows);
    int64_t xo = 0, yo = 0;
    for (const FlManyClip& c : sh.clips) {
        for (int j = 0; j < c.channels; ++j) {
            FlRagRow& r = rag[(size_t)(c.row0 + j)];
            r.x_off = xo; r.y_off = yo; r.n_in = c.n_in; r.n_out = c.N; r.factor = c.factor; r.c_lo = c.row0; r.c_hi = c.row0 + c.channels; r.pad_ = 0;
            w->x_off[(size_t)(c.row0 + j)] = xo; w->out_off[(size_t)(c.row0 + j)] = yo;
            xo += c.n_in; yo += c.N + (c.N & 1);
        }
        w->max_n_in = std::max(w->max_n_in, c.n_in); w->max_n_out = std::max(w->max_n_out, c.N);
    }
    std::vector<PzRowP> rows((size_t)ns);
    for (int j = 0; j < ns; ++j) {
        const FlManyState& st = sh.states[(size_t)j];
        const size_t d = (size_t)(std::lower_bound(ds.begin(), ds.end(), st.D) - ds.begin());
        PzRowP& r = rows[(size_t)j];
        r.D = (unsigned long long)st.D; r.inv_2D = 1.0 / (2.0 * (double)st.D); r.inv_D = 1.0 / (double)st.D;
        r.w.hi = w->d_tw.as<const dcplx>() + tw_hi[d]; r.w.lo = w->d_tw.as<const dcplx>() + tw_lo[d]; r.w.sh = tw_sh[d];
        r.bhat = bh[d];
        r.N = sh.clips[(size_t)st.clip].N;
        r.ya = rag[(size_t)st.row].y_off;
        r.yb = st.nch == 2 ? rag[(size_t)st.row + 1].y_off : r.ya;
        r.s = st.geo.s; r.odd = st.geo.odd; r.c0 = st.geo.c0; r.iDr = st.geo.iDr; r.cDr = st.geo.cDr; r.G = st.geo.G; r.g_per_xcd = st.geo.g_per_xcd;
        r.cha = st.row;
        r.chb = sh.kind == 1 ? st.row : (st.nch == 2 ? st.row + 1 : -1);
    }
    EGR_HIP(hipMemcpy(w->d_rows.p, rows.data(), rows.size() * sizeof(PzRowP), hipMemcpyHostToDevice));
    EGR_HIP(hipMemcpy(w->d_rag.p, rag.data(), rag.size() * sizeof(FlRagRow), hipMemcpyHostToDevice));
    const hipError_t se = hipDeviceSynchronize();          // the scratch buffers go when this function returns
    EGR_CHECK(se == hipSuccess && hipGetLastError() == hipSuccess, EGR_ERR_HIP, "egr_flmany_create: building the chirp spectra failed: %s", hipGetErrorString(se));
    *out = owner.release();
    return EGR_OK;
}

extern "C" int egr_flmany_layout(egr_flmany* w, int64_t* x_off, int64_t* out_off, int64_t totals[2]) {
    EGR_CHECK(w && x_off && out_off && totals, EGR_ERR_ARG, "egr_flmany_layout: null argument");
    std::copy(w->x_off.begin(), w->x_off.end(), x_off);
    std::copy(w->out_off.begin(), w->out_off.end(), out_off);
    totals[0] = w->shape.x_total; totals[1] = w->shape.out_total;
    return EGR_OK;
}

extern "C" int egr_flmany_enhance(egr_flmany* w, const float* x_flat, float* out_flat, int max_iter, float thr, unsigned flags, void* stream) {
    EGR_CHECK(w && w->base, EGR_ERR_ARG, "egr_flmany_enhance: null wave");
    EGR_CHECK(max_iter >= 1, EGR_ERR_ARG, "egr_flmany_enhance: max_iter=%d < 1", max_iter);
    EGR_CHECK(!(flags & (EGR_FL_THR_RECOMPUTE | EGR_FL_DEFER_FINALIZE)), EGR_ERR_UNSUPPORTED,
              "egr_flmany_enhance: EGR_FL_THR_RECOMPUTE and EGR_FL_DEFER_FINALIZE are not supported on a wave");
    EGR_CHECK(!w->shape.linspace || (flags & EGR_FL_INTERP_LINSPACE), EGR_ERR_ARG, "a wave with an explicit output length needs EGR_FL_INTERP_LINSPACE");
    egr_fatllama_plan* p = w->base;
    FlCall c{p, out_flat, max_iter, thr, flags, (hipStream_t)stream};
    EGR_TRY(enhance_begin(c, x_flat));          // flag checks; clears the peaks and the ring of maxima (both indexed by channel row)
    c.rows = w->d_rows.as<const PzRowP>();
    c.rows_gpx = w->shape.gpx;
    const FlRagRow* rag = w->d_rag.as<const FlRagRow>();
    const int rows = w->shape.rows;
    hipLaunchKernelGGL(k_prepare_rows, dim3(fl_grid(std::max(w->max_n_in, w->max_n_out)), rows), dim3(256), 0, c.st, x_flat, out_flat, rag,
                       (flags & EGR_FL_PCM_IN) ? 1 : 0, (flags & EGR_FL_ZERO_STUFF) ? 1 : 0, p->peaks(), p->peaks() + 2 * p->C,
                       (flags & EGR_FL_INTERP_LINSPACE) ? 1 : 0);
    EGR_TRY(pz_loop(c));
    if (flags & (EGR_FL_NORMALIZE | EGR_FL_AUTOSCALE | EGR_FL_NODE_POST))
        hipLaunchKernelGGL(k_finalize_rows, dim3(fl_grid(w->max_n_out), rows), dim3(256), 0, c.st, out_flat, rag, flags, p->peaks(), p->peaks() + p->C);
    EGR_HIP(hipGetLastError());
    return EGR_OK;
}

namespace egr {
__global__ void k_canary_selftest(int where, int payload_bytes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    EGR_LDS_CANARY_ARM(smem);
    float* cur = (float*)EGR_LDS_BASE(smem);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (where == 1) cur[payload_bytes / 4] = 1.f;          // one element past the payload
        if (where == 2) cur[-1] = 1.f;                         // one element before it
        if (where == 0) cur[payload_bytes / 4 - 1] = 1.f;      // the last payload element: legal
    }
}
}  // namespace egr

static long long canary_read() {
#ifdef EGR_LDS_CANARY
    unsigned v = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(&v, HIP_SYMBOL(egr::g_lds_canary_fail), sizeof(v)) != hipSuccess) return -2;
    return (long long)v;
#else
    return -1;
#endif
}

extern "C" long long egr_lds_canary_failures(void) {
#ifdef EGR_LDS_CANARY
    const long long a = canary_read(), b = pz_canary_failures();
    return (a < 0 || b < 0) ? -2 : a + b;
#else
    return -1;
#endif
}

extern "C" long long egr_lds_canary_selftest(int where) {
#ifdef EGR_LDS_CANARY
    const long long before = canary_read();
    hipLaunchKernelGGL(egr::k_canary_selftest, dim3(1), dim3(64), EGR_LDS(1024), 0, where, 1024);
    const long long after = canary_read();
    return (before < 0 || after < 0) ? -2 : after - before;
#else
    (void)where;
    return -1;
#endif
}
