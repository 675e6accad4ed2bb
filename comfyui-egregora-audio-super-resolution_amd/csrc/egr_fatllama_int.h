// Internal definitions shared by the Fat-Llama translation units (egr_fatllama.hip: packed-real plans, legacy chirp-z;
// egr_fatllama_pz.hip: paired chirp-z for every other length).  Not part of the public header.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <memory>
#include <vector>

#include "egr_common.h"
#include "egr_fft_device.h"
#include "egr_handle.h"
#include "egr_plan.h"

#define EGR_LDS_MAX (152 * 1024)      // dynamic LDS a kernel may ask for: the 160 KiB of a gfx950 CU minus room for its static arrays

// Debug build flag EGR_LDS_CANARY (make CANARY=1): every dynamic LDS region of the Fat-Llama kernels gets a 64-byte guard band in
// front of the payload and one behind it, filled with a sentinel when the kernel starts and checked when it returns (a
// workgroup-local overflow -- a reduction scratch sized for fewer waves, a tile index past its end -- lands in a guard instead
// of silently in a neighbour's data).  The host adds EGR_LDS_GUARD bytes to every dynamic-LDS request (EGR_LDS); the kernel finds
// the end of its region from the dispatch packet (group_segment_size minus its static LDS).  Failures are counted per translation
// unit and read with egr_lds_canary_failures().
#ifdef EGR_LDS_CANARY
#define EGR_LDS_GUARD 128
#define EGR_LDS_HEAD 64
#else
#define EGR_LDS_GUARD 0
#define EGR_LDS_HEAD 0
#endif
#define EGR_LDS(bytes) ((size_t)(bytes) + EGR_LDS_GUARD)
#define EGR_LDS_BASE(smem) ((smem) + EGR_LDS_HEAD)

struct egr_fatllama_plan;

namespace egr {

#ifdef EGR_LDS_CANARY
static __device__ unsigned g_lds_canary_fail;
struct LdsCanary {
    char* head;
    char* tail;
    __device__ __forceinline__ LdsCanary(char* smem) {
        const unsigned total = ((const unsigned*)__builtin_amdgcn_dispatch_ptr())[7];          // group_segment_size
        const unsigned dyn = total - __builtin_amdgcn_groupstaticsize();
        head = smem;
        tail = smem + dyn - 64;
        if (threadIdx.x < 16) {
            ((unsigned*)head)[threadIdx.x] = 0xC0FFEE00u + threadIdx.x;
            ((unsigned*)tail)[threadIdx.x] = 0xC0FFEE00u + threadIdx.x;
        }
    }
    __device__ __forceinline__ ~LdsCanary() {
        __syncthreads();
        if (threadIdx.x < 16 && (((unsigned*)head)[threadIdx.x] != 0xC0FFEE00u + threadIdx.x || ((unsigned*)tail)[threadIdx.x] != 0xC0FFEE00u + threadIdx.x))
            atomicAdd(&g_lds_canary_fail, 1u);
    }
};
#define EGR_LDS_CANARY_ARM(smem) LdsCanary lds_canary__(smem)
#else
#define EGR_LDS_CANARY_ARM(smem) do { } while (0)
#endif

#define EGR_STAMP(P, SLOT) do { if ((P).trace && threadIdx.x == 0) (P).trace[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 8 + (SLOT)] = wall_clock64(); } while (0)

// Twiddle W_T^r for r < T as a product of two table entries: thi[r >> sh] * tlo[r & (2^sh - 1)]
// (tables of ~sqrt(T) entries each, generated in long double).  The tables and the product are DOUBLE precision and the
// result is rounded to float once: every loop iteration multiplies element e by the same W on the way in and conj(W) on
// the way out, so |W|^2 - 1 is a per-element gain that compounds over the iterations -- (1 + eps)^800.  A product of two
// float-rounded factors leaves eps ~ 1.2e-7, the single rounding ~ 4e-8 (what any float32 twiddle table has); measured
// on 800 iterations: rms error vs float64 2.9x -> 1.xx the pocketfft oracle's (tests/test_gpu_fatllama.py).
struct Tw2 {
    const dcplx* hi;
    const dcplx* lo;
    int sh;
};
__device__ __forceinline__ dcplx tw2d(const Tw2& t, unsigned r) {
    return dcmul(t.hi[r >> t.sh], t.lo[r & ((1u << t.sh) - 1u)]);
}
__device__ __forceinline__ cplx tw2(const Tw2& t, unsigned r) {
    const dcplx w = tw2d(t, r);
    return make_float2((float)w.x, (float)w.y);
}

// One strided ("column") pass: `nplanes` matrices [L][ncols] (row-major), transform along L for a tile of TC
// adjacent columns, twiddle W_(L*ncols)^(col*k).
struct ColP {
    FftDesc f;
    int L, ncols, nplanes;
    int TC, TClog2, ntiles, tiles_per_xcd;
    const cplx* tw;        // W_L stage table
    const dcplx* twd;      // the same table in double precision (power-twiddle path)
    const cplx* stw;       // per-stage butterfly-ordered tables of a compile-time schedule (k_col<MODE, SCHED > 0>)
    long long* trace;      // dev: 100 MHz wall-clock stamps per phase, [block][8] (EGR_FL_TRACE)
    Tw2 big;               // W_(L*ncols)^r
};

// The contiguous ("row") pass: R rows of length L; row rho(o) holds Z[o + R*k], o = ka + Ma*kb, rho = ka*Mb + kb.
struct RowP {
    FftDesc f;
    int L, R, Ma, Mb;
    const cplx* tw;        // W_L stage table
    const dcplx* twd;      // the same table in double precision (power-twiddle path)
    const cplx* stw;       // per-stage butterfly-ordered tables of a compile-time schedule (k_row<., SCHED > 0>)
    long long* trace;      // dev: 100 MHz wall-clock stamps per phase, [block][8] (EGR_FL_TRACE)
    Tw2 wo;                // W_N^o, o < R
    const dcplx* wk;       // W_(2L)^k = W_N^(R*k), k < L (double: multiplied with W_N^o in double, rounded once)
    float thr2, inv_M;
    double inv_M_d;        // 1/M in double: the loop's scaling is applied in double and rounded once (a float 1/M is off by up to
                           // 6e-8 relative, the SAME way every iteration -- 5e-5 after 800)
    const float* gain;     // optional [C][M+1] real gain per half-spectrum bin (replaces the threshold)
    int phat;              // 1: the state is z = a + i b of two REAL signals; replace it by the PHAT-weighted cross-spectrum
    long long band_lo;     // > 0: keep half-spectrum bins k >= band_lo, zero the others (replaces the threshold); band = 1 selects it
    int band;
    // threshold variants (SPEC.md section 3).  max2 != nullptr: the level is thr * sqrt(max2[ch]) with max2[ch] = max_k |X[k]|^2 of
    // THIS iteration's spectrum (float bits, written by k_row<true>); soft: X max(0, 1 - t/|X|) instead of X [|X| > t].
    const unsigned* max2;
    unsigned* max2_out;    // k_row<true> only: where the maximum goes
    // carried maximum (round 6): the spectrum the NEXT iteration will see is this iteration's post-shrink spectrum (S keeps the
    // Hermitian symmetry, so fft(real(ifft(S(X)))) = S(X) up to round-off) -- the hook leaves max |S(X)|^2 in max2_next, and
    // clears the ring slot two iterations ahead (max2_zero)
    unsigned* max2_next;
    unsigned* max2_zero;
    float thr;
    int soft;
};

// tables of the two-barrier loop kernels (egr_fatllama_wl.h)
struct WlRowT {
    const cplx* t1;        // [Q^2][N1]: W_L^(n2 k1)
    const cplx* t2;        // [Q][Q]:    W_(Q^2)^(b c)
    const cplx* t1l;       // the low parts of the same tables: t + tl = W to 2^-48 (cmul2)
    const cplx* t2l;
    const dcplx* t2d;      // [Q]: W_(Q^2)^l in double (the ratio of a lane's run over c)
    dcplx hook_step;       // W_(2Q): ratio of the pair twiddles between a lane's consecutive registers
};
struct WlColT {
    const cplx* t3;        // [25][25]: W_625^(b c)
    const cplx* t3l;       // low parts
};

__device__ __forceinline__ void atomic_max_abs(unsigned* slot, float v) {
    // non-negative IEEE floats order like unsigned ints
    atomicMax(slot, __float_as_uint(v));
}

// Slots of the spectrum maxima of the relative threshold: per (ring slot, channel) EGR_FL_MAX_SUB words on lines of their own
// (a line serves about one device-scope atomic per 25 ns, DESIGN.md 4.2b: a workgroup commits to sub-slot blockIdx.x mod 8 and
// the reader takes the maximum of the eight).  All pointers below are the (slot, first channel of the launch) base.
#define EGR_FL_MAX_SUB 8
#define EGR_FL_MAX_LINE 32                                        // words per 128-byte line
#define EGR_FL_MAX_STRIDE (EGR_FL_MAX_SUB * EGR_FL_MAX_LINE)      // words per (slot, channel)
#define EGR_FL_MAX_RING 25                                        // ring slots = iterations of the captured loop graph
__device__ __forceinline__ float fl_max2_read(const unsigned* base, int ch) {
    const unsigned* b = base + (size_t)ch * EGR_FL_MAX_STRIDE;
    unsigned m = b[0];
#pragma unroll
    for (int s = 1; s < EGR_FL_MAX_SUB; ++s) { const unsigned v = b[s * EGR_FL_MAX_LINE]; m = v > m ? v : m; }
    return __uint_as_float(m);                                    // non-negative floats order like unsigned ints
}
__device__ __forceinline__ void fl_max2_commit(unsigned* base, int ch, float v) {
    atomicMax(base + (size_t)ch * EGR_FL_MAX_STRIDE + (blockIdx.x & (EGR_FL_MAX_SUB - 1)) * EGR_FL_MAX_LINE, __float_as_uint(v));
}
// called by threads tid < EGR_FL_MAX_SUB of ONE workgroup per channel
__device__ __forceinline__ void fl_max2_clear(unsigned* base, int ch, int tid) {
    base[(size_t)ch * EGR_FL_MAX_STRIDE + tid * EGR_FL_MAX_LINE] = 0u;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float r = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = fmaxf(r, red[i]);
    __syncthreads();
    return r;
}


struct ChirpP {
    Tw2 w;                   // W_(2N)^r
    unsigned long long N;    // transform length
    float inv_N;
    double inv_2N_d;         // 1 / (2 N) for the remainder estimate of chirp()
    int band;                // 1: the spectrum hook keeps bins min(n, N - n) >= band_lo instead of thresholding
    unsigned long long band_lo;
    int soft;                // 1: soft shrink X max(0, 1 - thr/|X|) instead of the hard threshold
    const unsigned* max2;    // relative threshold: max_k |X[k]|^2 of this iteration per channel (fl_max2_read); level = thr sqrt(.)
    unsigned* max2_out;      // k_colz<3, 1> only: where that maximum goes
};
__device__ __forceinline__ cplx chirp(const ChirpP& c, unsigned long long n) {
    // n^2 mod 2N without the 64-bit division (~150 instructions per element of every hook): n^2 < 2^53 is exact in double, the
    // quotient estimate is off by at most one, two conditional corrections make the remainder exact
    const unsigned long long m = 2ULL * c.N, n2 = n * n;
    unsigned long long r;
    if (n2 < (1ULL << 53)) {
        const unsigned long long q = (unsigned long long)((double)n2 * c.inv_2N_d);
        long long d = (long long)(n2 - q * m);
        if (d < 0) d += (long long)m;
        if (d >= (long long)m) d -= (long long)m;
        r = (unsigned long long)d;
    } else {
        r = n2 % m;
    }
    return tw2(c.w, (unsigned)r);
}


// Ring of the relative threshold's maxima: iteration `it` reads slot it, leaves the next maximum in slot it + 1 and clears slot it + 2
// (mod EGR_FL_MAX_RING); `ch0` is the first channel of the launch.
inline size_t fl_max2_words(size_t nslots, int C) { return nslots * C * EGR_FL_MAX_STRIDE; }
inline unsigned* fl_max2_slot(unsigned* ring, int C, int it, int ch0) {
    return ring + fl_max2_words((size_t)(it % EGR_FL_MAX_RING), C) + (size_t)ch0 * EGR_FL_MAX_STRIDE;
}

// Developer switches (environment), read by fl_read_switches() (egr_fatllama.hip) at the top of every plan build and of egr_fatllama_plan_query: the
// tests and bench.py change them between plan builds of one process.  EGR_FL_BLUE_THREADS alone is read once per process (blue_threads()).
struct FlSwitches {
    int streams = 2;              // EGR_FL_STREAMS: channel groups run as concurrent pipelines (1 or 2)
    bool graph = true;            // EGR_FL_GRAPH=0: plain launches instead of graph replay
    int threads = 512;            // EGR_FL_THREADS: workgroup size of the loop kernels (256, 512, 1024); 16 waves per CU at 2 workgroups
                                  // per CU measured 1.4x over 256
    bool sched = true;            // EGR_FL_SCHED=0: always the run-time schedule
    bool wl = true;               // EGR_FL_WL=0: the stage-by-stage kernels instead of the two-barrier ones (egr_fatllama_wl.h)
    int twpow = 1;                // EGR_FL_TWPOW=0: every stage twiddle loaded instead of W^2..W^(r-1) by multiplication from W^1
    int m1 = 0, tc = 0;           // EGR_FL_M1 / EGR_FL_TC: the planner's hints where the caller gives none
    bool legacy_chirpz = false;   // EGR_FL_LEGACY_CHIRPZ=1: the full-complex chirp-z instead of the paired one
    bool pz_sched = true, pz_colwl = true, pz_pairwl = true, pz_rowf = true;      // EGR_PZ_SCHED / _COLWL / _PAIRWL / _ROWF = 0
    int pz_split_L = 0, pz_split_nc = 0;                                          // EGR_PZ_SPLIT="L,nc" forces the paired factorisation
};

struct PzPlan;                                                   // egr_fatllama_pz.hip
struct PzPlanDelete { void operator()(PzPlan* z) const; };

// Where index 0 of a length-D transform sits inside a convolution of nc columns in tiles of TC, and the mirror geometry of its
// spectrum pass (egr_fatllama_pz.hip): computed by pz_row_geometry for a plan's own D and for every row of a wave.
struct PzGeo { int s, odd, c0, iDr, cDr, G, g_per_xcd; };
PzGeo pz_row_geometry(unsigned long long D, int nc, int TC);

// One state of a wave of clips that share a convolution length P but not the transform length D (egr_flmany_*): what the paired
// chirp-z kernels take from PzP for a plan's single D, per state.  A kernel that is handed a table of these replaces the
// D-dependent fields of its copy of PzP by rows[blockIdx.y] before anything else.
struct PzRowP {
    unsigned long long D;
    double inv_2D, inv_D;
    Tw2 w;                      // W_(2D)^r
    const cplx* bhat;           // FFT_P(b_D) / P in the passes' order
    long long N;                // real samples per channel
    long long ya, yb;           // offsets of the state's channel slices in the flat y / out buffer (yb = ya for a lone channel)
    int s, odd, c0, iDr, cDr, G, g_per_xcd;
    int cha, chb;               // wave-global channel ids (peaks, relative levels, ring of maxima); kind 1: chb = cha; kind 2 without
                                // a second channel: chb = -1
};

// ---- kernel selection of the packed loop ----
// A pass can run on one of three kernel families with different signatures: the run-time schedule (k_row / k_col), the compile-time
// schedule (k_row<., 1> / k_col<., 2>) and the two-barrier kernels (k_row_wl / k_col_wl / k_colb_wl).  fl_select_passes
// (egr_fatllama.hip) picks kernel, workgroup size, dynamic LDS and tile geometry once per plan; a launch is one indirect call.
typedef void (*FlRowFn)(RowP, long long, cplx*);
typedef void (*FlColFn)(ColP, long long, long long, float, cplx*, float*, unsigned*, const unsigned*);
typedef void (*WlRowFn)(RowP, WlRowT, long long, cplx*);
typedef void (*WlColFn)(ColP, WlColT, long long, cplx*);
typedef void (*WlInnerFn)(ColP, const cplx*, long long, cplx*);

// what a column pass takes besides the state (the two-barrier kernels use none of it)
struct FlColIO { float thr; float* out; unsigned* peak; const unsigned* thr_rel; };

// `launch` issues the pass over `nch` consecutive states from `work` with the call's copy of the pass parameters
struct FlRowPass {
    void (*launch)(const FlRowPass&, const egr_fatllama_plan*, const RowP&, cplx* work, int nch, hipStream_t);
    union { FlRowFn k; WlRowFn k_wl; };
    int threads;
    size_t lds;
    void operator()(const egr_fatllama_plan* p, const RowP& R, cplx* work, int nch, hipStream_t st) const { launch(*this, p, R, work, nch, st); }
};
struct FlColPass {
    void (*launch)(const FlColPass&, const egr_fatllama_plan*, const ColP&, const FlColIO&, cplx* work, int nch, hipStream_t);
    union { FlColFn k; WlColFn k_wl; WlInnerFn k_wlb; };
    int threads;
    size_t lds;
    const ColP* geo;       // the plan's ColP with this kernel's tile geometry
    void operator()(const egr_fatllama_plan* p, const FlColIO& io, cplx* work, int nch, hipStream_t st) const { launch(*this, p, *geo, io, work, nch, st); }
};
enum { FL_ROW_DEFAULT, FL_ROW_VARIANT, FL_ROW_MAX };      // hard threshold against an absolute level; relative and / or soft; maximum only
enum { FL_COL_OPEN, FL_COL_MID, FL_COL_CLOSE };
enum { FL_INNER_INV, FL_INNER_FWD };                      // indexed by `forward`
struct FlPasses {
    FlRowPass row[3];
    FlColPass col[3];
    FlColPass inner[2];
};
}  // namespace egr

struct egr_fatllama_plan {
    int64_t n_in = 0;
    int64_t n_out = 0;    // real samples per channel the loop runs on: n_in * factor, or the explicit length of egr_fatllama_plan_create_n (factor 0)
    int C = 0, factor = 0, device = 0;
    egr::FlSplit sp{};
    egr::ColP colA{}, colB{};
    egr::RowP row{};
    std::vector<egr::DevBuf> tables;      // twiddle and schedule tables (fl_upload*)
    bool bluestein = false;   // lengths outside the packed-real plans: chirp-z over P = sp.M complex points
    int pz_kind = 0;          // 0: packed-real plan or the legacy full-complex chirp-z; 1 / 2: paired chirp-z (egr_fatllama_pz.hip)
    std::unique_ptr<egr::PzPlan, egr::PzPlanDelete> pz;
    egr::ChirpP chirp{};
    egr::DevBuf d_bhat;       // FFT_P(b) / P in the passes' transposed layout
    egr::DevBuf d_work;
    egr::DevBuf d_peaks;      // [3*C]: peak_in[C], peak_out[C], peak_y[C]
    egr::DevBuf d_max2;       // [max2_cap]: ring of per-(iteration, channel) max |X|^2 slots of the relative-threshold variant (fl_max2_*)
    size_t max2_cap = 0;
    egr::cplx* work() const { return d_work.as<egr::cplx>(); }
    unsigned* peaks() const { return d_peaks.as<unsigned>(); }
    unsigned* max2() const { return d_max2.as<unsigned>(); }
    bool profiling = false;
    egr::FlPasses loop{};         // the loop's passes: every family the plan's lengths, the switches and `threads` allow
    egr::FlPasses single{};       // run-time-schedule kernels at 256 threads: the single-pass users, the chirp-z paths' inner passes
    egr::ColP wl_colA{}, wl_colB{};      // colA / colB with the tile geometry of k_col_wl / k_colb_wl
    const egr::cplx* wl_it = nullptr;    // [LB][LA]: W_L^(b c) of the inner length
    egr::WlRowT wl_rt{};
    egr::WlColT wl_ct{};
    int nstreams = 2;             // channel groups run as concurrent pipelines (1 or 2)
    egr::Stream side;             // second pipeline's stream (forked from / joined to the caller's stream by events): created by the
                                  // plan, or handed in by egr_fatllama_set_side_stream (then not destroyed with the plan)
    egr::EventPair fork_join;     // a: fork, b: join
    egr::Stream cap;              // private capture stream
    hipGraphExec_t gexec = nullptr;      // EGR_FL_MAX_RING captured loop iterations of all pipelines (fl_run_pipelines)
    float g_thr = 0.f; int g_groups = 0, g_hook_kind = 0;      // what gexec was captured for: threshold, pipelines, hook kind (soft | relative << 1)
    int use_graph = 1;
    std::vector<egr::EventPair> ev;      // (start, stop) per profiled launch, tagged by kind
    std::vector<int> ev_kind;            // 0 = row, 1 = outer column pass, 2 = inner column pass
};

namespace egr {
// one egr_fatllama_enhance call
struct FlCall {
    egr_fatllama_plan* p; float* out; int max_iter; float thr; unsigned flags; hipStream_t st;      // as given
    bool relative, recompute;
    int soft;
    float thr0;                  // time-domain level of the opening pass: thr, thr * max|y| (relative, thr0_rel) or none (-1: every sample kept)
    const unsigned* thr0_rel;
    unsigned* peak_out;
    const PzRowP* rows;          // a wave's row table (device), one entry per state of the plan; nullptr: the plan's own D for every state
    int rows_gpx;                // with rows: the largest g_per_xcd of the table (grid of the spectrum pass)
};
}  // namespace egr


// host helpers defined in egr_fatllama.hip
int fl_upload(egr_fatllama_plan* p, const std::vector<float2>& h, const egr::cplx** d);
int fl_upload_d(egr_fatllama_plan* p, int L, const egr::dcplx** d);                                        // W_L^j in double
int fl_upload_dtab(egr_fatllama_plan* p, int64_t count, int64_t num, int64_t den, const egr::dcplx** d);   // exp(-2 pi i j num / den)
int fl_make_tw2(egr_fatllama_plan* p, int64_t T, egr::Tw2* out);                                           // hi / lo tables of W_T^r
// butterfly-ordered stage tables of a compile-time schedule (stages after the first), egr_fft_device.h lds_fft_sched_inplace
int fl_upload_sched_tables(egr_fatllama_plan* p, std::initializer_list<int> radices, const egr::cplx** d);
void fl_prof_begin(egr_fatllama_plan* p, int kind, hipStream_t st, size_t* slot);
void fl_prof_end(egr_fatllama_plan* p, hipStream_t st, size_t* slot);
// inner column pass of a three-level plan over `nstates` states of the plan (forward: FFT . twiddle, else twiddle^-1 . IFFT)
void fl_launch_inner(egr_fatllama_plan* p, bool forward, egr::cplx* work, int nstates, hipStream_t st);

// Drains the device, then destroys the executable loop graph: it is never destroyed while a launch of it may still be in flight
// (calls return asynchronously).  Rare, millisecond-scale: a re-capture, a grown ring of maxima, a new side stream, the plan's end.
int fl_drop_graph(egr_fatllama_plan* p);

// The two-pipeline driver of the loops between k_prepare and k_finalize (packed: egr_fatllama.hip, paired chirp-z:
// egr_fatllama_pz.hip).  The channels (states) are independent until k_finalize and a loop kernel alone fills barely more than one
// wave of workgroups, so `ngroups` = 2 groups run as concurrent pipelines on the caller's stream and the plan's side stream, forked
// and joined by events.  run_group(s0, g, it0, it1, first, last, prof) issues group g's launches for iterations [it0, it1) on s0
// (g = 0) or the side stream; `first` adds the opening pass, `last` the closing one, `prof` the profiling events.
// Schedule: the opening pass with iterations [0, pre) -- leading ones that differ from a middle iteration --, n_graph replays of CH
// captured iterations, the tail [pre + n_graph CH, max_iter) with the closing pass; without replay the tail runs every iteration.
// A middle iteration is the same launches every time and touches the plan's own state only (never `out`): CH of them, all pipelines,
// are captured once into a hipGraph and replayed (inter-kernel gaps of ~8 us on the streams shrink to the graph's ~1 us).  The
// executable graph is keyed by (threshold, pipelines, hook kind) and survives calls with other buffers; its iterations address the
// ring of carried maxima by iteration mod CH.  `graph_allowed`: the loop's own conditions for replay; profiling runs and
// egr_fatllama_set_graph(0) use plain launches.  A template, not std::function: plain-launch mode issues a few thousand launches
// per call through run_group.
template <class RunGroup>
static inline int fl_run_pipelines(egr_fatllama_plan* p, hipStream_t st, int ngroups, int max_iter, int pre, bool graph_allowed,
                                   float thr, int hook_kind, RunGroup&& run_group) {
    constexpr int CH = 25;
    static_assert(CH == EGR_FL_MAX_RING, "the captured iterations address the ring of maxima by iteration mod CH");
    if (ngroups == 2 && !p->side.s) EGR_HIP(p->side.create());
    if (ngroups == 2 && !p->fork_join.a) EGR_HIP(p->fork_join.create(hipEventDisableTiming));
    // fork: the side stream waits for what s0 holds so far; join: s0 waits for the side stream (one pipeline: nothing to do)
    auto link = [&](hipEvent_t ev, hipStream_t from, hipStream_t to) -> int {
        if (ngroups == 2) { EGR_HIP(hipEventRecord(ev, from)); EGR_HIP(hipStreamWaitEvent(to, ev, 0)); }
        return EGR_OK;
    };
    auto fork = [&](hipStream_t s0) { return link(p->fork_join.a, s0, p->side.s); };
    auto join = [&](hipStream_t s0) { return link(p->fork_join.b, p->side.s, s0); };
    const bool profiling = p->profiling;
    const int n_graph = (graph_allowed && !profiling && p->use_graph && max_iter > 2 * CH) ? (max_iter - 1 - pre) / CH : 0;
    int rc = fork(st);
    if (rc) return rc;
    for (int g = 0; g < ngroups; ++g) run_group(st, g, 0, n_graph > 0 ? pre : 0, true, false, false);
    if (n_graph > 0) {
        rc = join(st);
        if (rc) return rc;
        if (!(p->gexec && p->g_thr == thr && p->g_groups == ngroups && p->g_hook_kind == hook_kind)) {
            rc = fl_drop_graph(p);
            if (rc) return rc;
            hipGraph_t graph = nullptr;
            // captured on a private stream (the caller's may be the legacy default stream, which cannot capture)
            if (!p->cap.s) EGR_HIP(p->cap.create());
            hipStream_t cap = p->cap.s;
            EGR_HIP(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
            rc = fork(cap);
            // max_iter > 2 CH: every one of the iterations [pre, pre + CH) is a "middle" iteration
            if (!rc) for (int g = 0; g < ngroups; ++g) run_group(cap, g, pre, pre + CH, false, false, false);
            if (!rc) rc = join(cap);
            hipError_t ce = hipStreamEndCapture(cap, &graph);
            if (rc || ce != hipSuccess) {          // leave no half-captured state behind: the next call starts from scratch
                if (graph) hipGraphDestroy(graph);
                p->cap.reset();
                if (rc) return rc;
                EGR_HIP(ce);
            }
            hipError_t ie = hipGraphInstantiate(&p->gexec, graph, nullptr, nullptr, 0);
            hipGraphDestroy(graph);
            if (ie != hipSuccess) { p->gexec = nullptr; EGR_HIP(ie); }
            p->g_thr = thr; p->g_groups = ngroups; p->g_hook_kind = hook_kind;
        }
        for (int i = 0; i < n_graph; ++i) EGR_HIP(hipGraphLaunch(p->gexec, st));
        rc = fork(st);
        if (rc) return rc;
    }
    for (int g = 0; g < ngroups; ++g) run_group(st, g, n_graph > 0 ? pre + n_graph * CH : 0, max_iter, false, true, profiling);
    return join(st);
}

// paired chirp-z (egr_fatllama_pz.hip)
int pz_build(egr_fatllama_plan* p, int kind, const egr::FlSwitches& sw);
// a wave's side of a paired chirp-z plan: raises the LDS cap of the row-table kernels; enqueues (default stream, no synchronisation)
// the double-precision build of FFT_P(b_D) / P into `bhat` through two scratch buffers of P double2 each
int pz_rows_prepare(egr_fatllama_plan* p);
const egr::cplx* pz_plan_bhat(const egr_fatllama_plan* p);          // the plan's own chirp spectrum
int pz_bhat_enqueue(const egr_fatllama_plan* p, unsigned long long D, void* scratch0, void* scratch1, egr::cplx* bhat);
long long pz_canary_failures();    // -1 without EGR_LDS_CANARY
bool pz_sched_has(int L, int nc);  // column length L and row length nc both have compile-time schedules (whatever EGR_PZ_SCHED says)
int pz_loop(const egr::FlCall& c);
int pz_band_filter(egr_fatllama_plan* p, const float* x, int64_t band_lo, float* y, hipStream_t st);
