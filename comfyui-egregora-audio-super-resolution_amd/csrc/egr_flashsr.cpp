// FlashSR model handle behind the C ABI:
//   egr_flashsr_create / egr_flashsr_infer / egr_flashsr_destroy stand in for the upstream calls
//   `FlashSR(student_ldm.pth, sr_vocoder.pth, vae.pth)` + `.eval().to(dev)` and `model(x[C,245760], lowpass_input)` that the
//   reference makes at egregora_audio_super_resolution.py:346-359 and :361-369.
// The whole graph walk lives here: layer table (egr_flashsr_config = flashsr_arch.FlashSRConfig) -> weight repacking -> kernel
// launches of the operators in egr_nn_*.hip, with a stream-ordered scratch arena instead of one allocation per operator.
// The host (Python or C) only supplies named fp32 tensors in torch layouts and calls infer on device pointers.
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "egr_arena.h"
#include "egr_conv.h"
#include "egr_handle.h"

extern "C" {
int egr_pack_weight(const float* src, float* dst, int layout, int K, int N, int Ci, int Co, int KH, int KW, void* stream);
int egr_phase_weights(const float* w_oihw, float* dst4, int Co, int Ci, void* stream);
int egr_winograd_pack_u(const float* w_oihw, float* dst, const double* G_dev, int np, int Co, int Ci, void* stream);
}

namespace {

using egr::set_error;
using egr::ConvCall;
using egr::ConvChoice;
using egr::DevBuf;         // egr_handle.h
using egr::EventPair;

enum { ACT_NONE = 0, ACT_SILU = 1, ACT_TANH = 2, ACT_LEAKY = 3, ACT_LOGCLAMP = 4 };
enum { EW_ADD = 0, EW_AXPBY = 1, EW_SILU = 2, EW_SCALE = 3, EW_COPY = 4, EW_ADD_SCALE = 5 };
// the want_ra argument of an operator, by name: its output feeds a split contraction directly, so the producer leaves its row maxima
const bool WANT_RA = true, NO_RA = false;

// ------------------------------------------------------------------------------------------------ device resources
// host time spent in the arenas' hipMalloc calls, in microseconds (EGR_FSR_TRACE=1 prints it per call); forwards on different devices run
// under different per-device locks, so the counter is atomic
static std::atomic<long long> g_arena_malloc_us{0};
static inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the scratch arena (csrc/egr_arena.h) over hipMalloc'ed slabs
struct HipSlabs {
    void* get(size_t bytes) {
        const double t0 = now_ms();
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) p = nullptr;
        g_arena_malloc_us += (long long)((now_ms() - t0) * 1e3);
        return p;
    }
    void put(void* base) { hipFree(base); }
};
typedef egr::Arena<HipSlabs> Arena;

struct Ten {                       // an fp32 activation owned by the arena (move-only)
    Arena* a = nullptr;
    float* p = nullptr;
    size_t bytes = 0;
    int nd = 0;
    int64_t d[4] = {0, 0, 0, 0};
    std::shared_ptr<Ten> part;     // GroupNorm partial sums left by the F(4x4) output transform (egr_winograd4_output_stats)
    int part_tiles = 0;
    // per-batch-row max |x| (bits; a slice of the context's pool, valid until the end of the forward): written by the producer of
    // the tensor or by the first split contraction that reads it (row_amax_of), reused by every later one
    mutable unsigned* rs = nullptr;
    Ten() {}
    Ten(const Ten&) = delete;
    Ten& operator=(const Ten&) = delete;
    Ten(Ten&& o) noexcept { *this = std::move(o); }
    Ten& operator=(Ten&& o) noexcept {
        if (this != &o) {
            release();
            a = o.a; p = o.p; bytes = o.bytes; nd = o.nd; memcpy(d, o.d, sizeof(d)); part = std::move(o.part); part_tiles = o.part_tiles;
            rs = o.rs; o.rs = nullptr;
            o.a = nullptr; o.p = nullptr; o.bytes = 0;
        }
        return *this;
    }
    ~Ten() { release(); }
    void release() { if (a && p) a->put(p, bytes); p = nullptr; a = nullptr; part.reset(); rs = nullptr; }
    int64_t numel() const { int64_t n = 1; for (int i = 0; i < nd; ++i) n *= d[i]; return n; }
    // non-owning view of the same storage (the owner must outlive it); keeps the GroupNorm partials the owner carries
    Ten alias() const { Ten v; v.nd = nd; memcpy(v.d, d, sizeof(d)); v.p = p; v.part = part; v.part_tiles = part_tiles; v.rs = rs; return v; }
    void view(std::initializer_list<int64_t> s) { nd = 0; for (int64_t v : s) d[nd++] = v; }
};

struct Wt : egr::PreparedWeight {  // one entry of the weight store; w may also be a raw tensor (norms, biases, snake parameters)
    int KH = 0, KW = 0, Cin = 0, Cout = 0;   // logical shape of a packed contraction (Cout = GEMM N)
    int64_t zfloats = 0;           // floats per component of a z-stacked Winograd pack
};

struct ProfRec { std::string kind; double flops; EventPair ev; std::string detail; };

}  // namespace

// Everything one in-flight forward owns: its stream, scratch arena and workspaces.  Context 0 runs on the caller's stream; the
// others on the handle's side streams when a pass is split into concurrent row groups (egr_flashsr_infer).  The destructor is the one
// place that releases them; whoever drops a context waits for its work first.
struct FsrCtx {
    hipStream_t st = nullptr;
    bool owns_st = false;                             // a side stream of the handle (context 0 runs on the caller's: not ours to destroy)
    Arena arena;
    DevBuf gn_ws;
    size_t gn_ws_bytes = 0;
    std::map<int, egr_fatllama_plan*> lp_plans;       // input low-pass: spectral-gain plans per row count
    hipEvent_t done = nullptr;
    // per-row operand maxima of the forward in flight (fp16 operand scheme): one R-entry slice per measured tensor, zeroed as a
    // whole when a forward starts
    DevBuf rs_pool;
    size_t rs_cap = 0, rs_used = 0;
    std::vector<DevBuf> rs_retired;                   // pools outgrown in mid-forward: still read by enqueued kernels, freed when the next forward starts
    DevBuf rs_ones;                                   // "maximum 1.0" for every row (operands known to lie in [0, 1]: soft-max outputs); rs_ones_rows entries
    int rs_ones_rows = 0;

    FsrCtx() {}
    explicit FsrCtx(hipStream_t side) : st(side), owns_st(true) { hipEventCreateWithFlags(&done, hipEventDisableTiming); }
    ~FsrCtx() {                                       // (the buffers and the arena's slabs free themselves)
        for (auto& kv : lp_plans) egr_fatllama_plan_destroy(kv.second);
        if (done) hipEventDestroy(done);
        if (owns_st) hipStreamDestroy(st);
    }
    // a forward of R rows on the fp16 operand scheme starts: retired pools go, one zeroed pool sized from the weight count, the ones table
    int begin_rows(int R, int h2_nweights) {
        size_t slices = (size_t)(2 * h2_nweights + 64);
        if (const char* e = getenv("EGR_FSR_RS_POOL_SLICES")) { const int v = atoi(e); if (v >= 1) slices = (size_t)v; }   // test knob: start small, exercise the growth in take_rows
        const size_t need = slices * (size_t)R * EGR_ROW_AMAX_STRIDE;
        if (!rs_retired.empty()) {                     // pools a previous forward outgrew (take_rows): its kernels are done once the stream is
            hipStreamSynchronize(st);
            rs_retired.clear();
        }
        if (rs_cap < need) {
            if (rs_pool.p) { hipStreamSynchronize(st); rs_pool.reset(); rs_cap = 0; }
            if (!rs_pool.alloc(need * sizeof(unsigned))) { set_error("hipMalloc(row maxima pool) failed"); return EGR_ERR_ALLOC; }
            rs_cap = need;
        }
        EGR_HIP(hipMemsetAsync(rs_pool.p, 0, rs_cap * sizeof(unsigned), st));
        rs_used = 0;
        if (rs_ones_rows < R) {
            if (rs_ones.p) { hipStreamSynchronize(st); rs_ones.reset(); }
            const size_t n = (size_t)R * EGR_ROW_AMAX_STRIDE;
            if (!rs_ones.alloc(n * sizeof(unsigned))) { set_error("hipMalloc(row maxima constants) failed"); return EGR_ERR_ALLOC; }
            std::vector<unsigned> ones(n, 0x3f800000u);
            EGR_HIP(hipMemcpy(rs_ones.p, ones.data(), n * sizeof(unsigned), hipMemcpyHostToDevice));
            rs_ones_rows = R;
        }
        return EGR_OK;
    }
    // R-entry slice of the pool of per-row maxima (zero at the start of the forward)
    unsigned* take_rows(int R) {
        if (rs_used + (size_t)R * EGR_ROW_AMAX_STRIDE > rs_cap) {
            // the start-of-forward size is a heuristic over the layer table; a graph that measures more tensors than it allowed for gets a
            // second, larger pool here (zeroed on the forward's stream) instead of a failed call -- the next forward starts at that size
            const size_t grown = std::max(2 * rs_cap, (size_t)64 * R * EGR_ROW_AMAX_STRIDE);
            DevBuf np;
            if (!np.alloc(grown * sizeof(unsigned))) { set_error("FlashSR: hipMalloc(row maxima pool, %zu entries) failed", grown); return nullptr; }
            if (hipMemsetAsync(np.p, 0, grown * sizeof(unsigned), st) != hipSuccess) { set_error("FlashSR: hipMemsetAsync(row maxima pool) failed"); return nullptr; }
            if (rs_pool.p) rs_retired.push_back(std::move(rs_pool));
            rs_pool = std::move(np); rs_cap = grown; rs_used = 0;
        }
        unsigned* p = rs_pool.as<unsigned>() + rs_used;
        rs_used += (size_t)R * EGR_ROW_AMAX_STRIDE;
        return p;
    }
    int gn_scratch(size_t need) {
        if (gn_ws_bytes < need) {
            if (gn_ws.p) { hipStreamSynchronize(st); gn_ws.reset(); gn_ws_bytes = 0; }
            if (!gn_ws.alloc(need + 1024)) { set_error("hipMalloc(GroupNorm workspace) failed"); return EGR_ERR_ALLOC; }
            gn_ws_bytes = need + 1024;
        }
        return EGR_OK;
    }
};

struct egr_flashsr {
    egr_flashsr_config cfg;
    unsigned flags = 0;
    int device = 0;
    std::vector<std::unique_ptr<FsrCtx>> ctxs;        // [0] = the caller's stream
    int max_groups = 2;                              // concurrent row groups per pass (EGREGORA_FLASHSR_STREAMS)
    int min_group_rows = 6;
    hipEvent_t ev_fork = nullptr;
    std::vector<hipStream_t> verified_for;            // caller streams the side streams were checked against
    std::vector<void*> owned;                         // weight allocations
    std::unordered_map<std::string, Wt> W;
    std::vector<std::string> blk_name;                // UNet block table (flashsr_arch.unet_blocks)
    std::vector<int> blk_cin, blk_cout, blk_attn;
    float* window = nullptr; float* filt = nullptr;
    int ldm = 0, lat_h = 0, lat_w = 0;
    float alpha = 0.f, sigma = 0.f;
    DevBuf d_wmax;                                    // one float: weight maxima at pack time
    int rows_per_pass = 32;
    // scratch budget (EGREGORA_FLASHSR_ARENA_GB / egr_flashsr_set_arena_cap; 0 = none): rows per pass are lowered until the arenas
    // of a pass are expected to fit (measured bytes per row once a pass has run, an estimate from the layer table before)
    double arena_cap = 0.0, arena_row_bytes = 0.0;
    int wino_min_ch = 128;
    int profiling = 0;                                // egr_flashsr_set_profiling: 0 off, 1 contraction launches, 2 and the graph's other operator launches
    std::vector<ProfRec> prof;
    // Two-term fp16 operand scheme of egr_flashsr_infer (csrc/egr_nn_gemm_s3.hip, scheme 1).  Every batch row of every split
    // contraction's input is scaled by its own power of two, which the kernel derives from that row's max |x|; the maxima are
    // written on the device by the tensor's producer (Winograd input transforms) or by one k_absmax_rows pass the first time a
    // tensor feeds a split contraction (row_amax_of).  Nothing about the scales passes through the host or survives the call:
    // the result of a row is a function of (weights, that row's input, seed, row id) and of the row count of its forward only
    // through tile choices; no value can leave fp16's range (the scale comes from the row's own maximum), so there is nothing to
    // verify or re-run, and the call is as asynchronous as the bf16 one.
    bool h2 = true;                                   // scheme available (off: EGR_FSR_SPLIT_BF16X3, EGREGORA_FLASHSR_SPLIT=bf16x3, f32 MFMA)
    bool h2_fwd = false;                              // egr_flashsr_forward too runs the fp16 terms (set_split 2 / 4: stage taps for tests)
    // Fast mode (EGR_FSR_FAST_F16, EGREGORA_FLASHSR_SPLIT=f16x1, set_split 3 / 4): the contractions the fp16 scheme serves run on ONE
    // fp16 term per operand (scheme 2: plane 0 of the same packs, the same row maxima and scales, the same graph walk) -- except the
    // fused AMP unit, the thin-end kernels and the attention products, which stay as they are, and the instantiations whose one-term
    // form measured no faster (egr::h1_pays): those launches keep scheme 1.  Reduced precision, opt-in.
    bool h1 = false;
    int h2_nweights = 0;                              // contraction weights that hold fp16 terms
    bool out_amax_on = true;                          // contraction epilogues leave the row maxima of their outputs (EGREGORA_FLASHSR_OUT_AMAX=0: off)
    int direct3x3_max_cout = 128;                     // EGREGORA_FLASHSR_DIRECT3X3_MAX_COUT (0: off): see gn_conv3
    bool fused_amp = true;                            // EGREGORA_FLASHSR_FUSED_AMP=0: the thin AMP units as four launches each
    int64_t h2_calls = 0;

    bool f32_mfma() const { return (flags & EGR_FSR_F32_MFMA) != 0; }
    bool h2_ready() const { return h2 && h2_nweights > 0; }   // egr_flashsr_infer runs the fp16 terms
    bool has(const std::string& k) const { return W.find(k) != W.end(); }
    const Wt* get(const std::string& k) const { auto it = W.find(k); return it == W.end() ? nullptr : &it->second; }
    float* ptr(const std::string& k) const { auto it = W.find(k); return it == W.end() ? nullptr : it->second.w; }
};

namespace {

typedef egr_flashsr M;

// What is true for ONE forward being enqueued.  The operators and stages take it; they read the model through `m` and write only
// through the context, the profile sink and the flop sum named here.
struct Fwd {
    const M& m;
    FsrCtx* cx;                        // its stream, arena, workspaces and row-maxima pool
    hipStream_t st;                    // = cx->st
    int R;                             // batch rows
    bool h2;                           // runs the fp16 operand terms (else three bf16 terms)
    int h_sch;                         // ... two of them per operand (1) or, in the handle's fast mode, one (2)
    std::vector<ProfRec>* prof;        // where timed launches are recorded, up to prof_level (0: nowhere)
    int prof_level;
    double* flops;                     // sum of contraction flops as executed, or null
    Fwd(const M& model, FsrCtx* c, int rows, bool fp16_terms, std::vector<ProfRec>* rec = nullptr, int level = 0, double* flop_sum = nullptr)
        : m(model), cx(c), st(c->st), R(rows), h2(fp16_terms), h_sch(model.h1 ? 2 : 1), prof(rec), prof_level(rec ? level : 0), flops(flop_sum) {}
    void count(double fl) { if (flops) *flops += fl; }
};

int dev_alloc(M* m, size_t bytes, void** out) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    if (hipMalloc(&p, bytes) != hipSuccess) { set_error("FlashSR weights: hipMalloc(%zu) failed", bytes); return EGR_ERR_ALLOC; }
    m->owned.push_back(p);
    *out = p;
    return EGR_OK;
}

int new_ten(Fwd& f, Ten& t, std::initializer_list<int64_t> shape) {
    t.release();
    t.view(shape);
    t.bytes = (size_t)t.numel() * sizeof(float);
    Arena& a = f.cx->arena;
    t.p = (float*)a.get(t.bytes);
    if (!t.p) { set_error("FlashSR scratch arena: hipMalloc(%zu) failed (%zu bytes held)", Arena::round_up(t.bytes), a.total); return EGR_ERR_ALLOC; }
    t.a = &a;
    return EGR_OK;
}

// a fresh arena tensor of x's shape
int new_like(Fwd& f, Ten& y, const Ten& x) {
    EGR_TRY(new_ten(f, y, {x.numel()}));
    y.nd = x.nd; memcpy(y.d, x.d, sizeof(y.d));
    return EGR_OK;
}

// ------------------------------------------------------------------------------------------------ layer table
void build_blocks(M* m) {
    const egr_flashsr_config& c = m->cfg;
    auto is_attn = [&](int ds) { for (int i = 0; i < c.unet_n_attn; ++i) if (c.unet_attn_ds[i] == ds) return 1; return 0; };
    auto add = [&](const std::string& n, int ci, int co, int at) { m->blk_name.push_back(n); m->blk_cin.push_back(ci); m->blk_cout.push_back(co); m->blk_attn.push_back(at); };
    const int mc = c.unet_ch;
    add("in.0.conv_in", 2 * c.z_ch, mc, 0);
    std::vector<int> skip{mc};
    int ch = mc, ds = 1, idx = 1;
    for (int lv = 0; lv < c.unet_levels; ++lv) {
        for (int r = 0; r < c.unet_res; ++r) {
            add("in." + std::to_string(idx) + ".block", ch, mc * c.unet_mult[lv], is_attn(ds));
            ch = mc * c.unet_mult[lv];
            skip.push_back(ch);
            ++idx;
        }
        if (lv != c.unet_levels - 1) {
            add("in." + std::to_string(idx) + ".down", ch, ch, 0);
            skip.push_back(ch);
            ds *= 2;
            ++idx;
        }
    }
    add("mid.0.block", ch, ch, 1);
    add("mid.1.block", ch, ch, 0);
    idx = 0;
    for (int lv = c.unet_levels - 1; lv >= 0; --lv) {
        for (int i = 0; i <= c.unet_res; ++i) {
            const int sc = skip.back(); skip.pop_back();
            add("out." + std::to_string(idx) + ".block", ch + sc, mc * c.unet_mult[lv], is_attn(ds));
            ch = mc * c.unet_mult[lv];
            if (lv != 0 && i == c.unet_res) { add("out." + std::to_string(idx) + ".up", ch, ch, 0); ds /= 2; }
            ++idx;
        }
    }
}

int up_kernel(int r) { return 2 * r + (r % 2); }

// ------------------------------------------------------------------------------------------------ weight packing
// the term packs of the packed w (N and numel set): three bf16 terms, and two fp16 terms of w * 2^k where the scheme is available
int split3(M* m, Wt& w) {
    if (m->f32_mfma() || !w.w) return EGR_OK;
    EGR_TRY(dev_alloc(m, w.term_bytes(3), &w.w3));
    if (m->h2) {
        if (!m->d_wmax.p && !m->d_wmax.alloc(sizeof(float))) { set_error("hipMalloc(weight maximum) failed"); return EGR_ERR_ALLOC; }
        EGR_TRY(dev_alloc(m, w.term_bytes(2), &w.w2));
        ++m->h2_nweights;
    }
    return egr::split_weight(w, m->d_wmax.as<float>(), m->ctxs[0]->st);
}

// src in torch layout on the device; layout as in egr_pack_weight; registers key with logical (KH, KW, Cin, N)
int add_packed(M* m, const std::string& key, const float* src, int layout, int K, int N, int Ci, int Co, int KH, int KW, int logical_kh,
               int logical_kw, int logical_cin) {
    Wt w;
    egr::weight_shape(w, K, N);
    EGR_TRY(dev_alloc(m, w.pack_bytes(), (void**)&w.w));
    EGR_TRY(egr_pack_weight(src, w.w, layout, K, N, Ci, Co, KH, KW, m->ctxs[0]->st));
    w.KH = logical_kh; w.KW = logical_kw; w.Cin = logical_cin; w.Cout = N;
    if (logical_cin % 16 == 0) {
        const bool keep = m->h2;
        if (key == "mel_fb") m->h2 = false;          // spectra span > 90 dB and a log follows: the mel projection keeps three bf16 terms
        const int rc = split3(m, w);
        m->h2 = keep;
        EGR_TRY(rc);
    }
    m->W[key] = w;
    return EGR_OK;
}

int add_weight(M* m, const std::string& key, const egr_tensor_desc& t) {
    const int64_t* s = t.shape;
    if (t.ndim == 4) return add_packed(m, key, t.data, 0, (int)(s[2] * s[3] * s[1]), (int)s[0], (int)s[1], (int)s[0], (int)s[2], (int)s[3], (int)s[2], (int)s[3], (int)s[1]);
    if (key.rfind("voc.ups.", 0) == 0 && t.ndim == 3)       // ConvTranspose1d [Ci][Co][k] -> GEMM [Ci][k*Co]
        return add_packed(m, key, t.data, 1, (int)s[0], (int)(s[2] * s[1]), (int)s[0], (int)s[1], 1, (int)s[2], 1, 1, (int)s[0]);
    if (t.ndim == 3) return add_packed(m, key, t.data, 0, (int)(s[2] * s[1]), (int)s[0], (int)s[1], (int)s[0], 1, (int)s[2], 1, (int)s[2], (int)s[1]);
    return add_packed(m, key, t.data, 0, (int)s[1], (int)s[0], (int)s[1], (int)s[0], 1, 1, 1, 1, (int)s[1]);
}

int add_phases(M* m, const std::string& key, const egr_tensor_desc& t) {
    const int Co = (int)t.shape[0], Ci = (int)t.shape[1];
    DevBuf tmp;
    const size_t n = (size_t)4 * Co * Ci * 4;
    if (!tmp.alloc(n * sizeof(float))) { set_error("hipMalloc(phase weights) failed"); return EGR_ERR_ALLOC; }
    int rc = egr_phase_weights(t.data, tmp.as<float>(), Co, Ci, m->ctxs[0]->st);
    for (int a = 0; a < 2 && rc == EGR_OK; ++a)
        for (int b = 0; b < 2 && rc == EGR_OK; ++b)
            rc = add_packed(m, key + ".ph" + std::to_string(a) + std::to_string(b), tmp.as<float>() + (size_t)(2 * a + b) * Co * Ci * 4, 0, 4 * Ci, Co, Ci, Co, 2, 2, 2, 2, Ci);
    hipStreamSynchronize(m->ctxs[0]->st);          // the packs read tmp: wait before it goes
    return rc;
}

const double kG2[12] = {1.0, 0.0, 0.0, 0.5, 0.5, 0.5, 0.5, -0.5, 0.5, 0.0, 0.0, 1.0};

int add_winograd(M* m, const std::string& key, const egr_tensor_desc& t, const double* G2_dev, const double* G4_dev) {
    const int Co = (int)t.shape[0], Ci = (int)t.shape[1];
    const int64_t zf = (int64_t)((Ci + 15) / 16) * Co * 16;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && (m->flags & EGR_FSR_NO_WINO_F4)) break;
        const int np = pass == 0 ? 4 : 6;
        Wt w;
        w.numel = (int64_t)np * np * zf;
        w.zfloats = zf;
        w.KH = w.KW = 1; w.Cin = w.K = Ci; w.Cout = w.N = Co;
        DevBuf pk;
        if (!pk.alloc((size_t)w.numel * sizeof(float))) { set_error("hipMalloc(Winograd U) failed"); return EGR_ERR_ALLOC; }
        int rc = egr_winograd_pack_u(t.data, pk.as<float>(), pass == 0 ? G2_dev : G4_dev, np, Co, Ci, m->ctxs[0]->st);
        w.w = pk.as<float>();
        if (rc == EGR_OK && Ci % 16 == 0) rc = split3(m, w);
        if (rc != EGR_OK) return rc;
        if (w.w3) {                                         // the fp32 pack is not needed once split
            hipStreamSynchronize(m->ctxs[0]->st);
            w.w = nullptr;
        } else {
            m->owned.push_back(pk.release());
        }
        m->W[key + (pass == 0 ? ".wino" : ".wino4")] = w;
    }
    return EGR_OK;
}

bool contains(const std::string& s, const char* sub) { return s.find(sub) != std::string::npos; }
bool ends_with(const std::string& s, const char* suf) { const size_t n = strlen(suf); return s.size() >= n && s.compare(s.size() - n, n, suf) == 0; }

int pack_all(M* m, const egr_tensor_desc* ts, int n) {
    double g4[18];
    EGR_TRY(egr_winograd4_g(g4));
    double* Gd = nullptr;
    EGR_TRY(dev_alloc(m, 30 * sizeof(double), (void**)&Gd));
    EGR_HIP(hipMemcpyAsync(Gd, kG2, 12 * sizeof(double), hipMemcpyHostToDevice, m->ctxs[0]->st));
    EGR_HIP(hipMemcpyAsync(Gd + 12, g4, 18 * sizeof(double), hipMemcpyHostToDevice, m->ctxs[0]->st));
    const bool thin = !(m->flags & EGR_FSR_NO_THIN_ENDS);
    for (int i = 0; i < n; ++i) {
        const egr_tensor_desc& t = ts[i];
        EGR_CHECK(t.name && t.data && t.ndim >= 0 && t.ndim <= 4, EGR_ERR_ARG, "tensor %d: bad descriptor", i);
        const std::string k = t.name;
        if (k.rfind("const.", 0) == 0) continue;
        if (ends_with(k, ".weight") && t.ndim >= 2) {
            EGR_TRY(add_weight(m, k, t));
            const int64_t* s = t.shape;
            if (contains(k, ".upsample.conv.") || (k.rfind("unet.", 0) == 0 && contains(k, ".up.conv."))) EGR_TRY(add_phases(m, k, t));
            if (thin && t.ndim == 4 && s[2] * s[3] * s[0] <= 32 && s[1] % 16 == 0)       // few outputs: 1x1 contraction onto per-tap products
                EGR_TRY(add_packed(m, k + ".taps", t.data, 2, (int)s[1], (int)(s[2] * s[3] * s[0]), (int)s[1], (int)s[0], (int)s[2], (int)s[3], 1, 1, (int)s[1]));
            if (!(m->flags & EGR_FSR_NO_WINOGRAD) && t.ndim == 4 && s[2] == 3 && s[3] == 3 && std::min(s[0], s[1]) >= m->wino_min_ch &&
                !contains(k, "downsample") && !contains(k, ".down.conv") && !contains(k, "upsample") && !contains(k, ".up.conv"))
                EGR_TRY(add_winograd(m, k, t, Gd, Gd + 12));
        } else {
            Wt w;
            int64_t ne = 1;
            for (int d = 0; d < t.ndim; ++d) ne *= t.shape[d];
            w.numel = ne;
            void* p = nullptr;
            EGR_TRY(dev_alloc(m, (size_t)ne * sizeof(float), &p));
            EGR_HIP(hipMemcpyAsync(p, t.data, (size_t)ne * sizeof(float), hipMemcpyDeviceToDevice, m->ctxs[0]->st));
            w.w = (float*)p;
            m->W[k] = w;
        }
    }
    return EGR_OK;
}

// ------------------------------------------------------------------------------------------------ profiling helpers
struct ProfScope {
    Fwd& f; bool on; EventPair ev;
    explicit ProfScope(Fwd& ff, int level = 1) : f(ff), on(ff.prof_level >= level) {
        if (on) { ev.create(); hipEventRecord(ev.a, f.st); }
    }
    void end(const std::string& kind, double flops, const std::string& detail = std::string()) {
        if (!on) return;
        hipEventRecord(ev.b, f.st);
        f.prof->push_back(ProfRec{kind, flops, std::move(ev), detail});
        on = false;
    }
};

// One timed contraction: `launch(ConvChoice*)` enqueues it between the two events of a profile record, which carries the kernel the
// launcher chose (or `kind`), the flops and `detail`; the flops also go to the forward's sum.
template <class Launch>
int timed(Fwd& f, double flops, const char* detail, Launch&& launch, const char* kind = nullptr) {
    ProfScope ps(f);
    ConvChoice ran;
    EGR_TRY(launch(&ran));
    if (ps.on) ps.end(kind ? kind : egr::conv_choice_name(ran), flops, detail);
    f.count(flops);
    return EGR_OK;
}

// A launch of the graph that is no contraction -- transforms, statistics, norms, gathers, row-maxima passes: at profiling level 2 it
// shows in egr_flashsr_profile under the name of the entry point called (zero flops), so that a test can see which of them a
// creation flag selected; at levels 0 and 1 this is the bare call.
#define OP(fn, ...)                              \
    do {                                         \
        ProfScope ps__(f, 2);                    \
        EGR_TRY(fn(__VA_ARGS__));                    \
        ps__.end(#fn, 0.0);                      \
    } while (0)

// ------------------------------------------------------------------------------------------------ operators
const void* s3_of(const Fwd& f, const Wt* w, int Cin, const float* x) {
    if (f.m.f32_mfma() || !w || Cin % 16 != 0 || (((uintptr_t)x) & 15) != 0) return nullptr;
    return w->w3;
}

// Slice for the row maxima of the fresh tensor y, for a producer that leaves them as it writes y.  y.rs stays null -- the producer
// runs its plain form, and the first split contraction that reads y measures it (row_amax_of) -- outside the fp16 scheme, when the
// producer is switched off, or when y does not split into the forward's rows.
//   sw:   RS_SWITCHED producers are turned off by EGREGORA_FLASHSR_OUT_AMAX=0; RS_ALWAYS ones (snake, the Winograd input transform) are not
//   test: n (y's batch dimension, or its row / element count) must equal R (ROWS_EQUAL) or be a multiple of it (ROWS_DIVIDE)
// (ROWS_EQUAL on the batch dimension B also covers "y's elements split into R rows": numel is a multiple of B)
enum RsSwitch { RS_ALWAYS, RS_SWITCHED };
enum RsRows { ROWS_EQUAL, ROWS_DIVIDE };
int rs_for_output(Fwd& f, Ten& y, RsSwitch sw, RsRows test, int64_t n) {
    if (!f.h2 || (sw == RS_SWITCHED && !f.m.out_amax_on) || (test == ROWS_EQUAL ? n != f.R : n % f.R != 0)) return EGR_OK;
    y.rs = f.cx->take_rows(f.R);
    return y.rs ? EGR_OK : EGR_ERR_ALLOC;
}

// per-batch-row max |x| of a tensor whose leading dimension runs over the R rows of the forward (nz > 1: nz blocks zx floats
// apart, the Winograd V layout); measured once per tensor, reused by every later contraction that reads it
int row_amax_of(Fwd& f, const float* x, int64_t numel, int nz, int64_t zx, unsigned** slot) {
    if (*slot) return EGR_OK;
    EGR_CHECK(numel % f.R == 0, EGR_ERR_ARG, "FlashSR: a tensor of %lld elements does not split into %d batch rows", (long long)numel, f.R);
    unsigned* p = f.cx->take_rows(f.R);
    if (!p) return EGR_ERR_ALLOC;
    OP(egr_absmax_rows, x, f.R, numel / f.R, nz, zx, (float*)p, f.st);
    *slot = p;
    return EGR_OK;
}

// One contraction with the weight `w` (named `key` in errors): completes `c` (the caller filled x, y, geometry and epilogue; zfloats: floats
// per z problem of a stacked pack, 0 otherwise) and launches it -- on the split kernels in the operand scheme of the forward being enqueued,
// or on the fp32 pack when the call cannot be split.  *ran: the kernel the launcher chose (what the profiler reports).
// y_rs (optional): the launch leaves the per-row maxima of y there (fp16 scheme, nz == 1; a fresh slice is taken when *y_rs is null
// -- the four phase launches of an up-sampling convolution share one)
int s3_launch(Fwd& f, const Wt* w, const std::string& key, ConvCall& c, int64_t x_numel, unsigned** x_rs, int64_t zfloats, ConvChoice* ran, unsigned** y_rs = nullptr) {
    const bool split = s3_of(f, w, c.Cin, c.x) != nullptr;
    EGR_CHECK(split || w->w != nullptr, EGR_ERR_ARG, "FlashSR: no fp32 pack for %s", key.c_str());
    const bool use = split && f.h2 && w->w2 && ((int64_t)c.B * c.OH * c.OW) % f.R == 0;
    c.zw = split ? zfloats * (use ? 2 : 3) / 8 : zfloats;
    if (use) {
        EGR_TRY(row_amax_of(f, c.x, c.nz > 1 ? x_numel / c.nz : x_numel, c.nz, c.zx, x_rs));
        if (y_rs && c.nz == 1 && f.m.out_amax_on) {
            if (!*y_rs) *y_rs = f.cx->take_rows(f.R);
            if (!*y_rs) return EGR_ERR_ALLOC;
            c.out_amax = (float*)*y_rs;
        }
    }
    egr::set_weight(c, *w, use ? *x_rs : nullptr, f.R, split, f.h_sch);
    return egr::conv_call(c, f.st, ran, true);
}

// general convolution described by `c`: the caller fills geometry, epilogue and any explicit bias / residual by name; conv() allocates
// y and completes x, y and the full output extent.  Weights by key (key + ".weight"; the bias is key + ".bias" when key_bias and c.bias
// is null) or the explicit entry `wk` (no bias from the key).  want_ra: y feeds another split contraction directly, so the epilogue
// leaves its row maxima.
int conv(Fwd& f, Ten& y, const Ten& x, const std::string& wkey, ConvCall& c, bool want_ra = false, const Wt* wk = nullptr, bool key_bias = true) {
    EGR_TRY(new_ten(f, y, {c.B, c.OH, c.OW, c.Cout}));
    const Wt* w = wk ? wk : f.m.get(wkey + ".weight");
    EGR_CHECK(w != nullptr, EGR_ERR_ARG, "FlashSR: weight %s.weight missing", wkey.c_str());
    if (!c.bias && key_bias && !wk) c.bias = f.m.ptr(wkey + ".bias");
    c.x = x.p; c.y = y.p; c.OHF = c.OH; c.OWF = c.OW;
    char det[160] = "";
    if (f.prof_level >= 1)
        snprintf(det, sizeof(det), "%s B%d %dx%d Cin%d -> %dx%d Cout%d k%dx%d s%d d%d up%d", wkey.c_str(), c.B, c.H, c.W, c.Cin, c.OH, c.OW, c.Cout,
                 c.KH, c.KW, c.stride, c.dil, c.up2);
    return timed(f, 2.0 * c.B * c.OH * c.OW * c.Cout * c.KH * c.KW * c.Cin, det, [&](ConvChoice* ran) {
        return s3_launch(f, w, wkey, c, (int64_t)c.B * c.H * c.W * c.Cin, &x.rs, 0, ran, want_ra ? &y.rs : nullptr);
    });
}

int groupnorm(Fwd& f, Ten& y, const Ten& x, const std::string& key, float eps, bool silu) {
    const int B = (int)x.d[0], Cc = (int)x.d[x.nd - 1];
    const int HW = (int)(x.numel() / ((int64_t)B * Cc));
    const int G = f.m.cfg.gn_groups;
    EGR_TRY(f.cx->gn_scratch(egr_groupnorm_workspace_bytes(B, Cc, G)));
    EGR_TRY(new_like(f, y, x));
    EGR_TRY(rs_for_output(f, y, RS_SWITCHED, ROWS_EQUAL, B));
    OP(egr_groupnorm_nhwc_ra, x.p, f.m.ptr(key + ".weight"), f.m.ptr(key + ".bias"), y.p, B, HW, Cc, G, eps, silu ? 1 : 0, f.cx->gn_ws.p, (float*)y.rs,
       f.st);
    return EGR_OK;
}

int gn_coeff(Fwd& f, Ten& sc, Ten& sh, const Ten& x, const std::string& key, float eps) {
    const int B = (int)x.d[0], Cc = (int)x.d[x.nd - 1];
    const int HW = (int)(x.numel() / ((int64_t)B * Cc));
    const int G = f.m.cfg.gn_groups;
    EGR_TRY(f.cx->gn_scratch(egr_groupnorm_workspace_bytes(B, Cc, G)));
    EGR_TRY(new_ten(f, sc, {B, Cc}));
    EGR_TRY(new_ten(f, sh, {B, Cc}));
    if (x.part) {        // x came out of egr_winograd4_output_stats: reduce its partials instead of re-reading x
        Ten stats;
        EGR_TRY(new_ten(f, stats, {B, G, 4}));            // [B][G][2] doubles
        OP(egr_groupnorm_stats_from_partials, x.part->p, B, x.part_tiles, Cc, G, (double*)stats.p, f.st);
        OP(egr_groupnorm_coeff_from_stats, (const double*)stats.p, f.m.ptr(key + ".weight"), f.m.ptr(key + ".bias"), B, HW, Cc, G, eps, sc.p, sh.p, f.st);
        return EGR_OK;
    }
    OP(egr_groupnorm_coeff, x.p, f.m.ptr(key + ".weight"), f.m.ptr(key + ".bias"), B, HW, Cc, G, eps, f.cx->gn_ws.p, sc.p, sh.p, f.st);
    return EGR_OK;
}

int conv_winograd(Fwd& f, Ten& y, const Ten& x, const std::string& key, int act, const float* res, const float* bias_t, const float* gsc = nullptr,
                  const float* gsh = nullptr, int gsilu = 0) {
    const int B = (int)x.d[0], H = (int)x.d[1], W = (int)x.d[2], Cin = (int)x.d[3];
    const Wt* wb = f.m.get(key + ".weight");
    const int Cout = wb->Cout;
    const bool f4 = f.m.has(key + ".weight.wino4") && H % 4 == 0 && W % 4 == 0;
    const Wt* wz = f.m.get(key + (f4 ? ".weight.wino4" : ".weight.wino"));
    const int nz = f4 ? 36 : 16, ts = f4 ? 4 : 2;
    const int TH = (H + ts - 1) / ts, TW = (W + ts - 1) / ts;
    const int64_t P = (int64_t)B * TH * TW;
    Ten V, Mx;
    EGR_TRY(new_ten(f, V, {nz, P, Cin}));
    // fp16 operand scheme: the F(4x4) input transform leaves the per-row maxima of V as it writes it
    if (f4 && wz && wz->w2 && Cin % 16 == 0) EGR_TRY(rs_for_output(f, V, RS_ALWAYS, ROWS_EQUAL, B));
    if (V.rs) OP(egr_winograd4_input_ra, x.p, gsc, gsh, gsilu, B, H, W, Cin, V.p, (float*)V.rs, f.st);
    else if (f4) OP(egr_winograd4_input, x.p, gsc, gsh, gsilu, B, H, W, Cin, V.p, f.st);
    else OP(egr_winograd_input, x.p, gsc, gsh, gsilu, B, H, W, Cin, V.p, f.st);
    EGR_TRY(new_ten(f, Mx, {nz, P, Cout}));
    ConvCall c;                                        // nz independent [P][Cin] x [Cin][Cout] products
    c.x = V.p; c.y = Mx.p; c.B = (int)P; c.Cin = Cin; c.Cout = Cout; c.nz = nz; c.zx = P * Cin; c.zy = P * Cout;
    EGR_TRY(timed(f, nz * 2.0 * (double)P * Cin * Cout, "", [&](ConvChoice* ran) {
        return s3_launch(f, wz, key + (f4 ? ".weight.wino4" : ".weight.wino"), c, (int64_t)nz * P * Cin, &V.rs, wz->zfloats, ran);
    }));
    V.release();
    EGR_TRY(new_ten(f, y, {B, H, W, Cout}));
    const float* bt = bias_t ? bias_t : f.m.ptr(key + ".bias");
    const int G = f.m.cfg.gn_groups;
    const int silu = act == ACT_SILU ? 1 : 0;
    // fp16 operand scheme: the output transform leaves the per-row maxima of y (it may feed a 1x1 / strided / phase convolution)
    if (f4) EGR_TRY(rs_for_output(f, y, RS_SWITCHED, ROWS_EQUAL, B));
    float* const y_ra = (float*)y.rs;
    if (f4 && !(f.m.flags & EGR_FSR_NO_GN_PARTIALS) && Cout % G == 0 && (Cout / G) % 4 == 0) {
        auto part = std::make_shared<Ten>();
        EGR_TRY(new_ten(f, *part, {P, Cout / 4, 2}));
        OP(egr_winograd4_output_ra, Mx.p, bt, res, y.p, B, H, W, Cout, silu, part->p, y_ra, f.st);
        y.part = part;
        y.part_tiles = TH * TW;
    } else if (f4) {
        OP(egr_winograd4_output_ra, Mx.p, bt, res, y.p, B, H, W, Cout, silu, nullptr, y_ra, f.st);
    } else {
        OP(egr_winograd_output, Mx.p, bt, res, y.p, B, H, W, Cout, silu, f.st);
    }
    return EGR_OK;
}

int conv_up2_phases(Fwd& f, Ten& y, const Ten& x, const std::string& key, int act) {
    const int B = (int)x.d[0], H = (int)x.d[1], W = (int)x.d[2], Cin = (int)x.d[3];
    const int Cout = f.m.get(key + ".weight")->Cout;
    EGR_TRY(new_ten(f, y, {B, 2 * H, 2 * W, Cout}));
    const float* bt = f.m.ptr(key + ".bias");
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const Wt* w = f.m.get(key + ".weight.ph" + std::to_string(a) + std::to_string(b));
            ConvCall c;                               // 2x2 kernel on the low-res input, written to phase (a, b) of the 2H x 2W output
            c.x = x.p; c.bias = bt; c.y = y.p; c.B = B; c.H = c.OH = H; c.W = c.OW = W; c.Cin = Cin; c.Cout = Cout; c.KH = c.KW = 2;
            c.pad_t = 1 - a; c.pad_l = 1 - b; c.act = act; c.osy = c.osx = 2; c.ooy = a; c.oox = b; c.OHF = 2 * H; c.OWF = 2 * W;
            EGR_TRY(timed(f, 2.0 * B * H * W * Cout * 4 * Cin, "", [&](ConvChoice* ran) {
                return s3_launch(f, w, key + ".weight.ph", c, (int64_t)B * H * W * Cin, &x.rs, 0, ran, &y.rs);
            }));
        }
    return EGR_OK;
}

// want_ra reaches only the generic exit; the phase, Winograd, tap-gather and one-input-channel exits track y's row maxima, or not, on their own
int conv3(Fwd& f, Ten& y, const Ten& x, const std::string& key, int stride = 1, int up2 = 0, int act = ACT_NONE, const float* res = nullptr,
          int pad = 1, const float* bias_t = nullptr, bool want_ra = false) {
    const int B = (int)x.d[0], H = (int)x.d[1], W = (int)x.d[2], Cin = (int)x.d[3];
    const Wt* wb = f.m.get(key + ".weight");
    EGR_CHECK(wb != nullptr, EGR_ERR_ARG, "FlashSR: weight %s.weight missing", key.c_str());
    const int Cout = wb->Cout;
    if (up2 && f.m.has(key + ".weight.ph00") && stride == 1 && pad == 1 && !res && !bias_t) return conv_up2_phases(f, y, x, key, act);
    if (f.m.has(key + ".weight.wino") && !up2 && stride == 1 && pad == 1 && (act == ACT_NONE || act == ACT_SILU) && H % 2 == 0 && W % 2 == 0 &&
        Cin % 16 == 0)
        return conv_winograd(f, y, x, key, act, res, bias_t);
    const bool plain = !up2 && stride == 1 && pad == 1 && act == ACT_NONE && !res && !bias_t;
    const bool thin = !(f.m.flags & EGR_FSR_NO_THIN_ENDS);
    const Wt* taps = f.m.get(key + ".weight.taps");
    if (plain && taps && s3_of(f, taps, Cin, x.p)) {
        Ten P;
        ConvCall c;                                   // 1x1 contraction onto the nine per-tap products
        c.B = B; c.H = c.OH = H; c.W = c.OW = W; c.Cin = Cin; c.Cout = 9 * Cout;
        EGR_TRY(conv(f, P, x, key, c, NO_RA, taps));
        EGR_TRY(new_ten(f, y, {B, H, W, Cout}));
        OP(egr_tap_gather, P.p, f.m.ptr(key + ".bias"), y.p, B, H, W, 3, 3, Cout, 1, 1, f.st);
        return EGR_OK;
    }
    if (plain && thin && Cin == 1 && Cout % 4 == 0 && 256 % (Cout / 4) == 0) {
        EGR_TRY(new_ten(f, y, {B, H, W, Cout}));
        OP(egr_conv_cin1, x.p, wb->w, f.m.ptr(key + ".bias"), y.p, B, H, W, Cout, 3, 3, 1, 1, f.st);
        f.count(2.0 * B * H * W * Cout * 9);
        return EGR_OK;
    }
    ConvCall c;                                       // the generic exit: the only one that takes the request for y's row maxima
    c.B = B; c.H = H; c.W = W; c.Cin = Cin; c.OH = (up2 ? 2 * H : H) / stride; c.OW = (up2 ? 2 * W : W) / stride; c.Cout = Cout; c.KH = c.KW = 3;
    c.stride = stride; c.pad_t = c.pad_l = pad; c.up2 = up2; c.act = act; c.bias = bias_t; c.res = res;
    return conv(f, y, x, key, c, want_ra);
}

int conv1x1(Fwd& f, Ten& y, const Ten& x, const std::string& key, const float* res = nullptr, int act = ACT_NONE, bool want_ra = false) {
    ConvCall c;
    c.B = (int)x.d[0]; c.H = c.OH = (int)x.d[1]; c.W = c.OW = (int)x.d[2]; c.Cin = (int)x.d[3]; c.Cout = f.m.get(key + ".weight")->Cout;
    c.act = act; c.res = res;
    return conv(f, y, x, key, c, want_ra);
}

int linear(Fwd& f, Ten& y, const Ten& x2, const std::string& key, const float* res = nullptr, int act = ACT_NONE, bool bias = true,
           bool want_ra = false) {
    const Wt* w = f.m.get(key + ".weight");
    EGR_CHECK(w != nullptr, EGR_ERR_ARG, "FlashSR: weight %s.weight missing", key.c_str());
    ConvCall c;
    c.B = (int)x2.d[0]; c.Cin = (int)x2.d[1]; c.Cout = w->Cout; c.act = act; c.res = res;
    EGR_TRY(conv(f, y, x2, key, c, want_ra, nullptr, bias));
    y.view({c.B, w->Cout});
    return EGR_OK;
}

int conv1d(Fwd& f, Ten& y, const Ten& x, const std::string& key, int k, int stride = 1, int dil = 1, int pad = 0, int act = ACT_NONE,
           const float* res = nullptr, bool want_ra = false) {
    ConvCall c;
    c.B = (int)x.d[0]; c.W = (int)x.d[1]; c.Cin = (int)x.d[2]; c.Cout = f.m.get(key + ".weight")->Cout; c.KW = k;
    c.OW = (c.W + 2 * pad - dil * (k - 1) - 1) / stride + 1; c.stride = stride; c.dil = dil; c.pad_l = pad; c.act = act; c.res = res;
    EGR_TRY(conv(f, y, x, key, c, want_ra));
    y.view({c.B, c.OW, c.Cout});
    return EGR_OK;
}

// conv3x3(silu(groupnorm(x))) with the normalisation fused into the Winograd input transform when the layer takes that path
int gn_conv3(Fwd& f, Ten& y, const Ten& x, const std::string& norm_key, float eps, const std::string& conv_key, const float* res = nullptr,
             const float* bias_t = nullptr) {
    const int H = (int)x.d[1], W = (int)x.d[2], Cin = (int)x.d[3];
    // The big, thin layers (128 output channels on 512 x 256 images) as DIRECT convolutions on the input-stationary kernel with the
    // GroupNorm + SiLU in its loader (fp16 operand scheme only): as an F(4x4) pipeline they are bound by V and M round trips
    // (~19 GB per layer against 3.5 GB of activations), here x is read once and y written once.
    {
        const Wt* wd = f.m.get(conv_key + ".weight");
        const int B = (int)x.d[0];
        if (wd && wd->w2 && f.h2 && f.m.direct3x3_max_cout > 0 && wd->Cout <= f.m.direct3x3_max_cout && wd->KH == 3 &&
            wd->KW == 3 && B == f.R && H % 4 == 0 && W % 32 == 0 && Cin % 32 == 0 && (int64_t)(H / 4) * (W / 32) * B >= 512 &&
            Cin % f.m.cfg.gn_groups == 0 && (((uintptr_t)x.p) & 15) == 0) {
            Ten sc, sh;
            EGR_TRY(gn_coeff(f, sc, sh, x, norm_key, eps));
            EGR_TRY(row_amax_of(f, x.p, x.numel(), 1, 0, &x.rs));
            unsigned* bound = f.cx->take_rows(f.R);
            if (!bound) return EGR_ERR_ALLOC;
            OP(egr_gn_operand_bound, sc.p, sh.p, B, Cin, (const float*)x.rs, (float*)bound, f.st);
            EGR_TRY(new_ten(f, y, {B, H, W, wd->Cout}));
            EGR_TRY(rs_for_output(f, y, RS_SWITCHED, ROWS_EQUAL, B));
            const float* bt = bias_t ? bias_t : f.m.ptr(conv_key + ".bias");
            // GroupNorm partial statistics of y from the epilogue (the next norm then reads 1/32 of y's bytes instead of y)
            void* gpart = nullptr;
            const int G = f.m.cfg.gn_groups;
            if (!(f.m.flags & EGR_FSR_NO_GN_PARTIALS) && wd->Cout % G == 0 && (wd->Cout / G) % 4 == 0) {
                auto part = std::make_shared<Ten>();
                EGR_TRY(new_ten(f, *part, {(int64_t)B * H * W / 32, wd->Cout / 4, 2}));
                gpart = part->p;
                y.part = part;
                y.part_tiles = H * W / 32;
            }
            ConvCall c;
            c.x = x.p; c.bias = bt; c.res = res; c.y = y.p; c.gn_scale = sc.p; c.gn_shift = sh.p; c.gn_silu = 1;
            c.B = B; c.H = c.OH = c.OHF = H; c.W = c.OW = c.OWF = W; c.Cin = Cin; c.Cout = wd->Cout; c.KH = c.KW = 3; c.pad_t = c.pad_l = 1;
            egr::set_weight(c, *wd, bound, B, true, f.h_sch);
            c.out_amax = (float*)y.rs; c.gn_part = gpart;
            return timed(f, 2.0 * B * H * W * (double)wd->Cout * 9 * Cin, conv_key.c_str(), [&](ConvChoice* ran) { return egr::conv_call(c, f.st, ran, true); });
        }
    }
    const bool wino = f.m.has(conv_key + ".weight.wino") && H % 2 == 0 && W % 2 == 0;
    const bool fused_ok = !(f.m.flags & EGR_FSR_NO_FUSE_GN) && Cin % 16 == 0 && Cin % f.m.cfg.gn_groups == 0 && wino;
    if (!fused_ok) {
        Ten h;
        EGR_TRY(groupnorm(f, h, x, norm_key, eps, true));
        return conv3(f, y, h, conv_key, 1, 0, ACT_NONE, res, 1, bias_t);
    }
    Ten sc, sh;
    EGR_TRY(gn_coeff(f, sc, sh, x, norm_key, eps));
    return conv_winograd(f, y, x, conv_key, ACT_NONE, res, bias_t, sc.p, sh.p, 1);
}

int layernorm(Fwd& f, Ten& y, const Ten& x2, const std::string& key) {
    EGR_TRY(new_ten(f, y, {x2.d[0], x2.d[1]}));
    EGR_TRY(rs_for_output(f, y, RS_SWITCHED, ROWS_DIVIDE, x2.d[0]));
    if (!y.rs) OP(egr_layernorm_rows, x2.p, f.m.ptr(key + ".weight"), f.m.ptr(key + ".bias"), y.p, x2.d[0], (int)x2.d[1], 1e-5f, f.st);
    else OP(egr_layernorm_rows_ra, x2.p, f.m.ptr(key + ".weight"), f.m.ptr(key + ".bias"), y.p, x2.d[0], (int)x2.d[1], 1e-5f, f.R, (float*)y.rs, f.st);
    return EGR_OK;
}

int eltwise(Fwd& f, Ten& y, const Ten& a, const float* b, int op, float s0 = 0.f, float s1 = 0.f, bool want_ra = false) {
    EGR_TRY(new_like(f, y, a));
    if (want_ra) EGR_TRY(rs_for_output(f, y, RS_SWITCHED, ROWS_DIVIDE, y.numel()));
    if (!y.rs) OP(egr_eltwise, a.p, b, y.p, a.numel(), op, s0, s1, f.st);
    else OP(egr_eltwise_ra, a.p, b, y.p, a.numel(), op, s0, s1, f.R, (float*)y.rs, f.st);
    return EGR_OK;
}

// q, k, v [B*T][C] -> [B*T][C]: softmax(q k^T / sqrt(d)) v per head
int attention(Fwd& f, Ten& o, const Ten& q, const Ten& k, const Ten& v, int B, int T, int Cc, int heads) {
    const int d = Cc / heads;
    Ten S;
    EGR_TRY(new_ten(f, S, {B, heads, T, T}));
    const bool s3 = !f.m.f32_mfma() && d % 16 == 0 && T % 16 == 0 && Cc % 4 == 0;
    const float sc = (float)pow((double)d, -0.5);
    // fp16 operand scheme: both products on two fp16 terms, every operand scaled per batch row from its own maximum (q / k / v carry
    // theirs from the epilogues of their projections; the soft-max output lies in [0, 1]: a constant)
    const bool h2 = s3 && f.h2 && B == f.R;
    if (h2) {
        EGR_TRY(row_amax_of(f, q.p, q.numel(), 1, 0, &q.rs));
        EGR_TRY(row_amax_of(f, k.p, k.numel(), 1, 0, &k.rs));
        EGR_TRY(row_amax_of(f, v.p, v.numel(), 1, 0, &v.rs));
        EGR_TRY(egr_bgemm_nt_h2(q.p, k.p, S.p, B, heads, T, T, d, Cc, Cc, T, (int64_t)T * Cc, d, (int64_t)T * Cc, d, (int64_t)heads * T * T,
                            (int64_t)T * T, sc, (const float*)q.rs, (const float*)k.rs, nullptr, f.st));
    } else if (s3)
        EGR_TRY(egr_bgemm_nt_s3(q.p, k.p, S.p, B, heads, T, T, d, Cc, Cc, T, (int64_t)T * Cc, d, (int64_t)T * Cc, d, (int64_t)heads * T * T,
                            (int64_t)T * T, sc, f.st));
    else
        EGR_TRY(egr_bgemm(q.p, k.p, S.p, B, heads, T, T, d, Cc, Cc, T, (int64_t)T * Cc, d, (int64_t)T * Cc, d, (int64_t)heads * T * T, (int64_t)T * T, 1,
                      sc, f.st));
    EGR_TRY(egr_softmax_rows(S.p, (int64_t)B * heads * T, T, f.st));
    EGR_TRY(new_ten(f, o, {(int64_t)B * T, Cc}));
    if (s3) {
        Ten vt;
        EGR_TRY(new_ten(f, vt, {B, Cc, T}));
        EGR_TRY(egr_transpose_batched(v.p, vt.p, B, T, Cc, f.st));
        if (h2) {
            EGR_TRY(rs_for_output(f, o, RS_SWITCHED, ROWS_EQUAL, B));   // o feeds the output projection (B == R here, so o splits into the rows)
            EGR_TRY(egr_bgemm_nt_h2(S.p, vt.p, o.p, B, heads, T, d, T, T, T, Cc, (int64_t)heads * T * T, (int64_t)T * T, (int64_t)Cc * T, (int64_t)d * T,
                                (int64_t)T * Cc, d, 1.0f, f.cx->rs_ones.as<float>(), (const float*)v.rs, (float*)o.rs, f.st));
        } else
        EGR_TRY(egr_bgemm_nt_s3(S.p, vt.p, o.p, B, heads, T, d, T, T, T, Cc, (int64_t)heads * T * T, (int64_t)T * T, (int64_t)Cc * T, (int64_t)d * T,
                            (int64_t)T * Cc, d, 1.0f, f.st));
    } else {
        EGR_TRY(egr_bgemm(S.p, v.p, o.p, B, heads, T, d, T, T, Cc, Cc, (int64_t)heads * T * T, (int64_t)T * T, (int64_t)T * Cc, d, (int64_t)T * Cc, d, 0,
                      1.0f, f.st));
    }
    f.count(4.0 * B * heads * (double)T * T * d);
    return EGR_OK;
}

int snake(Fwd& f, Ten& y, const Ten& x, const std::string& akey, const std::string& bkey) {
    EGR_TRY(new_ten(f, y, {x.d[0], x.d[1], x.d[2]}));
    EGR_TRY(rs_for_output(f, y, RS_ALWAYS, ROWS_EQUAL, (int)x.d[0]));   // fp16 operand scheme: y feeds a 1-D convolution; its row maxima ride along
    OP(egr_snake_aa_ra, x.p, f.m.ptr(akey), f.m.ptr(bkey), f.m.filt, y.p, (int)x.d[0], (int)x.d[1], (int)x.d[2], f.m.cfg.aa_taps, (float*)y.rs, f.st);
    return EGR_OK;
}

int concat(Fwd& f, Ten& y, const Ten& a, const Ten& b) {
    const int64_t rows = a.d[0] * a.d[1] * a.d[2];
    EGR_TRY(new_ten(f, y, {a.d[0], a.d[1], a.d[2], a.d[3] + b.d[3]}));
    EGR_TRY(rs_for_output(f, y, RS_SWITCHED, ROWS_EQUAL, (int)a.d[0]));
    if (!y.rs) OP(egr_concat_channels, a.p, b.p, y.p, rows, (int)a.d[3], (int)b.d[3], f.st);
    else OP(egr_concat_channels_ra, a.p, b.p, y.p, rows, (int)a.d[3], (int)b.d[3], f.R, (float*)y.rs, f.st);
    return EGR_OK;
}

// ------------------------------------------------------------------------------------------------ constant sub-graph
// time embedding at t = T-1: silu(MLP(emb)) is shared by all res-blocks; each block's projection is folded into its conv bias
int fold_time_embedding(M* model, const float* emb_dev) {
    const egr_flashsr_config& c = model->cfg;
    Fwd f(*model, model->ctxs[0].get(), 1, false);   // creation: one row on the bf16 terms, context 0, nothing recorded
    Ten emb, t1, t2;
    EGR_TRY(new_ten(f, emb, {1, c.unet_ch}));
    EGR_HIP(hipMemcpyAsync(emb.p, emb_dev, (size_t)c.unet_ch * 4, hipMemcpyDeviceToDevice, f.st));
    EGR_TRY(linear(f, t1, emb, "unet.time_embed.0", nullptr, ACT_SILU));
    EGR_TRY(linear(f, t2, t1, "unet.time_embed.2", nullptr, ACT_SILU));
    for (size_t i = 0; i < f.m.blk_name.size(); ++i) {
        const std::string& name = f.m.blk_name[i];
        if (!ends_with(name, ".block")) continue;
        const std::string base = "unet." + name;
        Ten e;
        EGR_TRY(linear(f, e, t2, base + ".res.emb"));
        const Wt* b = f.m.get(base + ".res.in_conv.bias");
        EGR_CHECK(b != nullptr, EGR_ERR_ARG, "FlashSR: %s.res.in_conv.bias missing", base.c_str());
        Wt bt;
        bt.numel = b->numel;
        void* p = nullptr;
        EGR_TRY(dev_alloc(model, (size_t)b->numel * 4, &p));
        bt.w = (float*)p;
        EGR_TRY(egr_eltwise(b->w, e.p, bt.w, b->numel, EW_ADD, 0.f, 0.f, f.st));
        model->W[base + ".res.in_conv.bias_t"] = bt;
    }
    EGR_HIP(hipStreamSynchronize(f.st));
    return EGR_OK;
}

// ------------------------------------------------------------------------------------------------ stages
int log_mel(Fwd& f, Ten& mel, const float* x, int B, int L) {
    const egr_flashsr_config& c = f.m.cfg;
    const int rpad = (c.n_fft - c.hop) / 2;
    const int t_valid = std::min(c.n_frames, (L + 2 * rpad - c.n_fft) / c.hop + 1);
    Ten mag;
    EGR_TRY(new_ten(f, mag, {B, c.n_frames, f.m.ldm}));
    EGR_TRY(egr_stft_frames(x, B, L, c.n_fft, c.hop, rpad, c.n_frames, t_valid, f.m.ldm, f.m.window, mag.p, f.st));
    mag.view({(int64_t)B * c.n_frames, 1, 1, f.m.ldm});
    ConvCall cc;
    cc.B = B * c.n_frames; cc.Cin = f.m.ldm; cc.Cout = c.n_mels; cc.act = ACT_LOGCLAMP; cc.act_param = c.log_floor;
    EGR_TRY(conv(f, mel, mag, "mel_fb", cc, NO_RA, f.m.get("mel_fb")));
    mel.view({B, c.n_frames, c.n_mels, 1});
    return EGR_OK;
}

// lowpass_input=True: cutoff from the STFT energy, zero-phase 8th-order Chebyshev-I gain applied on the Fat-Llama transform passes
int lowpass(Fwd& f, Ten& y, const float* x, int B, int L) {
    const egr_flashsr_config& c = f.m.cfg;
    const int rpad = (c.n_fft - c.hop) / 2;
    const int T = (L + 2 * rpad - c.n_fft) / c.hop + 1;
    const int nb = c.n_fft / 2 + 1;
    Ten mag, cut, gain;
    EGR_TRY(new_ten(f, mag, {B, T, f.m.ldm}));
    EGR_TRY(egr_stft_frames(x, B, L, c.n_fft, c.hop, rpad, T, T, f.m.ldm, f.m.window, mag.p, f.st));
    EGR_TRY(new_ten(f, cut, {B}));
    const int64_t nbins = L / 2 + 1;
    EGR_TRY(new_ten(f, gain, {B, nbins}));
    EGR_TRY(egr_lowpass_gain(mag.p, B, T, f.m.ldm, nb, 0.985f, (float)c.sr, 8, 0.05f, nbins, (int*)cut.p, gain.p, f.st));
    egr_fatllama_plan*& plan = f.cx->lp_plans[B];
    if (!plan) EGR_TRY(egr_fatllama_plan_create(&plan, L, B, 1, 0, 0));
    EGR_TRY(new_ten(f, y, {B, L}));
    return egr_spectral_gain(plan, x, gain.p, y.p, f.st);
}

int vae_res(Fwd& f, Ten& y, const Ten& x, const std::string& name) {
    Ten h, sc;
    EGR_TRY(gn_conv3(f, h, x, name + ".norm1", 1e-6f, name + ".conv1"));
    const float* scp = x.p;
    if (f.m.has(name + ".nin_shortcut.weight")) { EGR_TRY(conv1x1(f, sc, x, name + ".nin_shortcut")); scp = sc.p; }
    return gn_conv3(f, y, h, name + ".norm2", 1e-6f, name + ".conv2", scp);
}

int vae_attn(Fwd& f, Ten& y, const Ten& x, const std::string& name) {
    const int B = (int)x.d[0], H = (int)x.d[1], W = (int)x.d[2], Cc = (int)x.d[3];
    Ten h, q, k, v, o;
    EGR_TRY(groupnorm(f, h, x, name + ".norm", 1e-6f, false));
    EGR_TRY(conv1x1(f, q, h, name + ".q", nullptr, ACT_NONE, WANT_RA));
    EGR_TRY(conv1x1(f, k, h, name + ".k", nullptr, ACT_NONE, WANT_RA));
    EGR_TRY(conv1x1(f, v, h, name + ".v", nullptr, ACT_NONE, WANT_RA));
    EGR_TRY(attention(f, o, q, k, v, B, H * W, Cc, 1));
    o.view({B, H, W, Cc});
    return conv1x1(f, y, o, name + ".proj_out", x.p, ACT_NONE, WANT_RA);
}

int vae_encode(Fwd& f, Ten& z, const Ten& mel) {
    const egr_flashsr_config& c = f.m.cfg;
    Ten h, t;
    EGR_TRY(conv3(f, h, mel, "vae.encoder.conv_in"));
    for (int lv = 0; lv < c.vae_levels; ++lv) {
        for (int b = 0; b < c.vae_res; ++b) {
            EGR_TRY(vae_res(f, t, h, "vae.encoder.down." + std::to_string(lv) + ".block." + std::to_string(b)));
            h = std::move(t);
        }
        if (lv != c.vae_levels - 1) {
            EGR_TRY(conv3(f, t, h, "vae.encoder.down." + std::to_string(lv) + ".downsample.conv", 2, 0, ACT_NONE, nullptr, 0, nullptr, WANT_RA));
            h = std::move(t);
        }
    }
    EGR_TRY(vae_res(f, t, h, "vae.encoder.mid.block_1")); h = std::move(t);
    EGR_TRY(vae_attn(f, t, h, "vae.encoder.mid.attn_1")); h = std::move(t);
    EGR_TRY(vae_res(f, t, h, "vae.encoder.mid.block_2")); h = std::move(t);
    EGR_TRY(groupnorm(f, t, h, "vae.encoder.norm_out", 1e-6f, true));
    EGR_TRY(conv3(f, h, t, "vae.encoder.conv_out"));
    Ten mom;
    EGR_TRY(conv1x1(f, mom, h, "vae.quant_conv"));
    // the mean half of the moments: channels [0, z_ch) of 2 z_ch
    const int64_t rows = mom.d[0] * mom.d[1] * mom.d[2];
    EGR_TRY(new_ten(f, z, {mom.d[0], mom.d[1], mom.d[2], c.z_ch}));
    EGR_HIP(hipMemcpy2DAsync(z.p, (size_t)c.z_ch * 4, mom.p, (size_t)2 * c.z_ch * 4, (size_t)c.z_ch * 4, (size_t)rows, hipMemcpyDeviceToDevice, f.st));
    return EGR_OK;
}

int vae_decode(Fwd& f, Ten& y, const Ten& z) {
    const egr_flashsr_config& c = f.m.cfg;
    Ten h, t;
    EGR_TRY(conv1x1(f, t, z, "vae.post_quant_conv", nullptr, ACT_NONE, WANT_RA));
    EGR_TRY(conv3(f, h, t, "vae.decoder.conv_in"));
    EGR_TRY(vae_res(f, t, h, "vae.decoder.mid.block_1")); h = std::move(t);
    EGR_TRY(vae_attn(f, t, h, "vae.decoder.mid.attn_1")); h = std::move(t);
    EGR_TRY(vae_res(f, t, h, "vae.decoder.mid.block_2")); h = std::move(t);
    for (int lv = c.vae_levels - 1; lv >= 0; --lv) {
        for (int b = 0; b <= c.vae_res; ++b) {
            EGR_TRY(vae_res(f, t, h, "vae.decoder.up." + std::to_string(lv) + ".block." + std::to_string(b)));
            h = std::move(t);
        }
        if (lv != 0) {
            EGR_TRY(conv3(f, t, h, "vae.decoder.up." + std::to_string(lv) + ".upsample.conv", 1, 1));
            h = std::move(t);
        }
    }
    EGR_TRY(groupnorm(f, t, h, "vae.decoder.norm_out", 1e-6f, true));
    return conv3(f, y, t, "vae.decoder.conv_out");
}

int unet_block(Fwd& f, Ten& y, const Ten& x, const std::string& base, bool has_attn) {
    const egr_flashsr_config& c = f.m.cfg;
    Ten h, sc, r;
    EGR_TRY(gn_conv3(f, h, x, base + ".res.in_norm", 1e-5f, base + ".res.in_conv", nullptr, f.m.ptr(base + ".res.in_conv.bias_t")));
    const float* scp = x.p;
    if (f.m.has(base + ".res.skip.weight")) { EGR_TRY(conv1x1(f, sc, x, base + ".res.skip")); scp = sc.p; }
    EGR_TRY(gn_conv3(f, r, h, base + ".res.out_norm", 1e-5f, base + ".res.out_conv", scp));
    h.release(); sc.release();
    if (!has_attn) { y = std::move(r); return EGR_OK; }
    const int B = (int)r.d[0], H = (int)r.d[1], W = (int)r.d[2], Cc = (int)r.d[3];
    const int T = H * W, heads = Cc / c.head_dim;
    Ten g0, t;
    EGR_TRY(groupnorm(f, g0, r, base + ".st.norm", 1e-6f, false));
    EGR_TRY(conv1x1(f, t, g0, base + ".st.proj_in"));
    g0.release();
    t.view({(int64_t)B * T, Cc});
    for (int a = 1; a <= 2; ++a) {
        const std::string an = base + ".st.attn" + std::to_string(a);
        Ten n_, q, k, v, o, t2;
        EGR_TRY(layernorm(f, n_, t, an + "_ln"));
        // q, k, v feed the attention products: their row maxima ride along
        EGR_TRY(linear(f, q, n_, an + ".to_q", nullptr, ACT_NONE, /*bias*/ false, WANT_RA));
        EGR_TRY(linear(f, k, n_, an + ".to_k", nullptr, ACT_NONE, /*bias*/ false, WANT_RA));
        EGR_TRY(linear(f, v, n_, an + ".to_v", nullptr, ACT_NONE, /*bias*/ false, WANT_RA));
        EGR_TRY(attention(f, o, q, k, v, B, T, Cc, heads));
        EGR_TRY(linear(f, t2, o, an + ".to_out", t.p));
        t = std::move(t2);
    }
    Ten ln, u, g, t3;
    EGR_TRY(layernorm(f, ln, t, base + ".st.ff_ln"));
    EGR_TRY(linear(f, u, ln, base + ".st.ff.geglu"));
    EGR_TRY(new_ten(f, g, {(int64_t)B * T, 4 * Cc}));
    EGR_TRY(rs_for_output(f, g, RS_SWITCHED, ROWS_EQUAL, B));
    if (g.rs) OP(egr_geglu_ra, u.p, g.p, (int64_t)B * T, 4 * Cc, f.R, (float*)g.rs, f.st);
    else OP(egr_geglu, u.p, g.p, (int64_t)B * T, 4 * Cc, f.st);
    EGR_TRY(linear(f, t3, g, base + ".st.ff.out", t.p, ACT_NONE, /*bias*/ true, WANT_RA));
    t3.view({B, H, W, Cc});
    return conv1x1(f, y, t3, base + ".st.proj_out", r.p, ACT_NONE, WANT_RA);
}

int unet(Fwd& f, Ten& out, Ten&& x0) {
    std::vector<Ten> skips;
    Ten h = std::move(x0), t;
    for (size_t i = 0; i < f.m.blk_name.size(); ++i) {
        const std::string& name = f.m.blk_name[i];
        const std::string base = "unet." + name;
        const std::string part = name.substr(0, name.find('.'));
        const std::string kind = name.substr(name.rfind('.') + 1);
        if (kind == "conv_in") {
            EGR_TRY(conv3(f, t, h, base));
            Ten cp = t.alias();                        // the skip stack owns the tensor, h views it
            skips.push_back(std::move(t));
            h = std::move(cp);
        } else if (kind == "down") {
            EGR_TRY(conv3(f, t, h, base + ".conv", 2, 0, ACT_NONE, nullptr, 1, nullptr, WANT_RA));
            Ten cp = t.alias();
            skips.push_back(std::move(t));
            h = std::move(cp);
        } else if (kind == "up") {
            EGR_TRY(conv3(f, t, h, base + ".conv", 1, 1));
            h = std::move(t);
        } else {
            if (part == "out") {
                Ten cat;
                EGR_TRY(concat(f, cat, h, skips.back()));
                skips.pop_back();
                h = std::move(cat);
            }
            EGR_TRY(unet_block(f, t, h, base, f.m.blk_attn[i] != 0));
            if (part == "in") {
                Ten cp = t.alias();
                skips.push_back(std::move(t));
                h = std::move(cp);
            } else {
                h = std::move(t);
            }
        }
    }
    EGR_TRY(groupnorm(f, t, h, "unet.out_norm", 1e-5f, true));
    return conv3(f, out, t, "unet.out_conv");
}

int amp(Fwd& f, Ten& y, Ten&& h, int j) {
    const egr_flashsr_config& c = f.m.cfg;
    Ten acc;
    for (int ki = 0; ki < c.voc_n_kernels; ++ki) {
        const int k = c.voc_kernels[ki];
        Ten x;                                   // aliases h on the first dilation
        const Ten* cur = &h;
        for (int di = 0; di < c.voc_n_dils; ++di) {
            const int d = c.voc_dils[di];
            const std::string b = "voc.amp." + std::to_string(j) + "." + std::to_string(ki) + "." + std::to_string(di);
            Ten xt, xc, xs, xn;
            // the 16- and 32-channel stages (245 760 / 122 880 samples per row): the unit's four launches are pure streaming there -- one fused kernel
            // keeps the L-tile on the CU (csrc/egr_nn_amp.hip); fp16 operand scheme only
            {
                const Wt* w1 = f.m.get(b + ".conv1.weight");
                const Wt* w2 = f.m.get(b + ".conv2.weight");
                const int Cc = (int)cur->d[2];
                if (f.m.fused_amp && f.h2 && w1 && w2 && w1->w2 && w2->w2 && Cc == 16 && w1->Cout == Cc && w2->Cout == Cc && (k & 1) &&
                    k <= 11 && d * (k - 1) / 2 <= 25 && c.aa_taps == 12 && cur->d[1] >= 16) {
                    EGR_TRY(new_ten(f, xn, {cur->d[0], cur->d[1], cur->d[2]}));
                    EGR_TRY(timed(f, 2.0 * 2.0 * (double)cur->d[0] * cur->d[1] * Cc * Cc * k, b.c_str(), [&](ConvChoice*) {
                        return egr_amp_unit_h2(cur->p, xn.p, (int)cur->d[0], (int)cur->d[1], Cc, k, d, f.m.ptr(b + ".alpha1"), f.m.ptr(b + ".beta1"), w1->w2, w1->w_scale,
                                               f.m.ptr(b + ".conv1.bias"), f.m.ptr(b + ".alpha2"), f.m.ptr(b + ".beta2"), w2->w2, w2->w_scale, f.m.ptr(b + ".conv2.bias"),
                                               f.m.filt, c.aa_taps, f.st);
                    }, egr::amp_unit_name()));
                    x = std::move(xn);
                    cur = &x;
                    continue;
                }
            }
            EGR_TRY(snake(f, xt, *cur, b + ".alpha1", b + ".beta1"));
            EGR_TRY(conv1d(f, xc, xt, b + ".conv1", k, 1, d, d * (k - 1) / 2));
            xt.release();
            EGR_TRY(snake(f, xs, xc, b + ".alpha2", b + ".beta2"));
            xc.release();
            EGR_TRY(conv1d(f, xn, xs, b + ".conv2", k, 1, 1, (k - 1) / 2, ACT_NONE, cur->p));
            x = std::move(xn);
            cur = &x;
        }
        if (ki == 0) {
            acc = std::move(x);
        } else if (ki + 1 < c.voc_n_kernels) {
            Ten s;
            EGR_TRY(eltwise(f, s, acc, x.p, EW_ADD));
            acc = std::move(s);
        } else {                                   // last branch: the mean's scale rides on the last add
            return eltwise(f, y, acc, x.p, EW_ADD_SCALE, 1.0f / c.voc_n_kernels, 0.f, WANT_RA);   // feeds the next stage's up-sampling GEMM
        }
    }
    return eltwise(f, y, acc, nullptr, EW_SCALE, 1.0f / c.voc_n_kernels, 0.f, WANT_RA);
}

int vocoder(Fwd& f, Ten& y, const Ten& mel_hat, const float* wave, int B) {
    const egr_flashsr_config& c = f.m.cfg;
    const int T = (int)mel_hat.d[1], Fm = (int)mel_hat.d[2];
    const int n = c.voc_n_rates;
    std::vector<Ten> feats(n);
    {
        Ten e0;                                     // non-owning view of the input rows
        e0.view({B, c.chunk, 1});
        e0.p = const_cast<float*>(wave);
        const Ten* e = &e0;
        for (int i = 0; i < n; ++i) {
            const int r = c.voc_rates[n - 1 - i];
            const bool feeds_next = i + 1 < n;          // the next strided convolution of the encoder reads it
            EGR_TRY(conv1d(f, feats[i], *e, "voc.wave_enc." + std::to_string(i), 2 * r + 1, r, 1, r, ACT_LEAKY, nullptr, feeds_next));
            e = &feats[i];
        }
    }
    Ten mh;                                        // [B][T][Fm] view of mel_hat
    mh.view({B, T, Fm});
    mh.p = mel_hat.p;
    Ten h;
    EGR_TRY(conv1d(f, h, mh, "voc.conv_pre", 7, 1, 1, 3, ACT_NONE, feats[n - 1].p, WANT_RA));
    feats[n - 1].release();
    for (int j = 0; j < n; ++j) {
        const int r = c.voc_rates[j];
        const int kt = up_kernel(r);
        const int Bc = (int)h.d[0], Lin = (int)h.d[1], Ci = (int)h.d[2];
        const Wt* wt = f.m.get("voc.ups." + std::to_string(j) + ".weight");
        const int Co = wt->Cout / kt;
        Ten Y, out, hx;
        hx.view({(int64_t)Bc * Lin, 1, 1, Ci});
        hx.p = h.p;
        hx.rs = h.rs;                                  // (a view: the row maxima of h are its own)
        ConvCall cu;                                   // ConvTranspose1d as a GEMM onto [kt][Co] columns, gathered by col2im below
        cu.B = Bc * Lin; cu.Cin = Ci; cu.Cout = kt * Co;
        EGR_TRY(conv(f, Y, hx, "voc.ups." + std::to_string(j), cu, NO_RA, wt));
        EGR_TRY(new_ten(f, out, {Bc, (int64_t)Lin * r, Co}));
        const float* add = (j <= n - 2) ? feats[n - 2 - j].p : nullptr;
        EGR_TRY(egr_col2im_convtr1d(Y.p, f.m.ptr("voc.ups." + std::to_string(j) + ".bias"), add, out.p, Bc, Lin, Lin * r, Co, kt, r, (kt - r) / 2, f.st));
        Y.release();
        if (j <= n - 2) feats[n - 2 - j].release();
        Ten nx;
        EGR_TRY(amp(f, nx, std::move(out), j));
        h = std::move(nx);
    }
    Ten s;
    EGR_TRY(snake(f, s, h, "voc.post.alpha", "voc.post.beta"));
    EGR_TRY(conv1d(f, y, s, "voc.conv_post", 7, 1, 1, 3, ACT_TANH));
    y.view({B, y.d[1]});
    return EGR_OK;
}

int copy_out(Fwd& f, float* dst, const Ten& t) {
    if (!dst) return EGR_OK;
    EGR_HIP(hipMemcpyAsync(dst, t.p, (size_t)t.numel() * 4, hipMemcpyDeviceToDevice, f.st));
    return EGR_OK;
}

// x [R][chunk], noise [R][h][w][z] (channels-last) -> y [R][chunk]; stages (optional): mel, z_cond, v, z0, mel_hat, y_full
int forward(Fwd& f, const float* x_in, const float* noise, int lowpass_on, float* y_out, float* const* stages) {
    const egr_flashsr_config& c = f.m.cfg;
    const float* x = x_in;
    const int R = f.R;
    if (f.h2) EGR_TRY(f.cx->begin_rows(R, f.m.h2_nweights));   // per-row operand maxima of this forward: one zeroed pool per context
    // EGR_FSR_TRACE=2 (diagnosis of first-call costs): synchronise after every stage and print host / device-complete times
    static const int trace_lv = getenv("EGR_FSR_TRACE") ? atoi(getenv("EGR_FSR_TRACE")) : 0;
    const bool trace2 = trace_lv >= 2;
    const double t_fwd = now_ms();
    auto stage_mark = [&](const char* what) {
        if (trace_lv == 1) fprintf(stderr, "[egr_flashsr forward R=%d] %-10s enqueued at %8.1f ms\n", R, what, now_ms() - t_fwd);
        if (!trace2) return;
        const double t_host = now_ms() - t_fwd;
        hipStreamSynchronize(f.st);
        fprintf(stderr, "[egr_flashsr forward R=%d] %-10s enqueued at %8.1f ms, complete at %8.1f ms (arena hipMalloc so far %.1f ms)\n", R, what, t_host,
                now_ms() - t_fwd, 1e-3 * (double)g_arena_malloc_us.load());
    };
    Ten xl;
    if (lowpass_on) { EGR_TRY(lowpass(f, xl, x_in, R, c.chunk)); x = xl.p; }
    Ten mel, z_c, v, z0, mel_hat, y;
    EGR_TRY(log_mel(f, mel, x, R, c.chunk));
    stage_mark("log_mel");
    EGR_TRY(vae_encode(f, z_c, mel));
    stage_mark("vae_encode");
    {
        Ten nz, cat;                               // non-owning view of the caller's noise
        nz.view({R, f.m.lat_h, f.m.lat_w, c.z_ch});
        nz.p = const_cast<float*>(noise);
        EGR_TRY(concat(f, cat, nz, z_c));
        EGR_TRY(unet(f, v, std::move(cat)));
        EGR_TRY(eltwise(f, z0, nz, v.p, EW_AXPBY, f.m.alpha, -f.m.sigma));
    }
    stage_mark("unet");
    EGR_TRY(vae_decode(f, mel_hat, z0));
    stage_mark("vae_decode");
    EGR_TRY(vocoder(f, y, mel_hat, x, R));
    stage_mark("vocoder");
    if (stages) {
        EGR_TRY(copy_out(f, stages[0], mel)); EGR_TRY(copy_out(f, stages[1], z_c)); EGR_TRY(copy_out(f, stages[2], v));
        EGR_TRY(copy_out(f, stages[3], z0)); EGR_TRY(copy_out(f, stages[4], mel_hat)); EGR_TRY(copy_out(f, stages[5], y));
    }
    const int64_t Ly = y.d[1];
    EGR_CHECK(Ly >= c.chunk, EGR_ERR_UNSUPPORTED, "FlashSR: vocoder output %lld shorter than the chunk %d", (long long)Ly, c.chunk);
    EGR_HIP(hipMemcpy2DAsync(y_out, (size_t)c.chunk * 4, y.p, (size_t)Ly * 4, (size_t)c.chunk * 4, (size_t)R, hipMemcpyDeviceToDevice, f.st));
    return EGR_OK;
}

// ------------------------------------------------------------------------------------------------ one forward at a time per device
// A handle serves ONE caller stream at a time: its contexts' scratch arenas are reused in stream order, so forwards that arrive on
// different streams of one device are chained by an event (whatever streams the host -- ComfyUI nodes, threads -- uses).  Inside
// a call the handle runs up to max_groups row groups concurrently on its own verified side streams (egr_flashsr_infer).
// History: the chain was introduced in round 1 against wrong STFT bins next to a foreign k_conv_s3; that was root-caused in
// round 2 to a gfx950 packed-fp32 op_sel erratum and removed at the source (csrc/Makefile NOPK, tests/test_isa_audit.py,
// DESIGN.md section 4.4a), so the guard is about arena ownership only.  EGR_FSR_NO_STREAM_GUARD=1 removes the chain (probes).
// The lock is PER DEVICE: host threads that drive different GPUs of one process (flashsr_engine.infer_spans_devices) enqueue
// their forwards side by side.
struct ForwardGuard {
    struct Dev { std::mutex fwd; hipStream_t last_st = nullptr; hipEvent_t ev = nullptr; };
    static Dev& of(int device) {
        static std::mutex m;
        static std::map<int, std::unique_ptr<Dev>> devs;
        std::lock_guard<std::mutex> g(m);
        auto& p = devs[device];
        if (!p) p.reset(new Dev());
        return *p;
    }
    Dev& d;
    std::unique_lock<std::mutex> lk;
    hipStream_t st; bool on;
    ForwardGuard(int device, hipStream_t s) : d(of(device)), lk(d.fwd), st(s) {
        static const bool off = getenv("EGR_FSR_NO_STREAM_GUARD") && atoi(getenv("EGR_FSR_NO_STREAM_GUARD")) != 0;
        on = !off;
        if (!on) return;
        if (d.ev && d.last_st != st) hipStreamWaitEvent(st, d.ev, 0);
    }
    ~ForwardGuard() {
        if (!on) return;
        if (!d.ev) hipEventCreateWithFlags(&d.ev, hipEventDisableTiming);
        hipEventRecord(d.ev, st);
        d.last_st = st;
    }
};

const egr_tensor_desc* find(const egr_tensor_desc* ts, int n, const char* name) {
    for (int i = 0; i < n; ++i) if (ts[i].name && strcmp(ts[i].name, name) == 0) return &ts[i];
    return nullptr;
}

}  // namespace

// ==================================================================================================== C ABI
extern "C" int egr_flashsr_default_config(egr_flashsr_config* c) {
    EGR_CHECK(c != nullptr, EGR_ERR_ARG, "config is null");
    memset(c, 0, sizeof(*c));
    c->struct_bytes = (int)sizeof(*c);
    c->sr = 48000; c->chunk = 245760; c->n_fft = 2048; c->hop = 480; c->n_mels = 256; c->n_frames = 512;
    c->fmin = 20.f; c->fmax = 24000.f; c->log_floor = 1e-5f;
    c->vae_ch = 128; c->vae_levels = 4; c->vae_mult[0] = 1; c->vae_mult[1] = 2; c->vae_mult[2] = 4; c->vae_mult[3] = 8; c->vae_res = 2;
    c->z_ch = 16; c->gn_groups = 32;
    c->unet_ch = 128; c->unet_levels = 4; c->unet_mult[0] = 1; c->unet_mult[1] = 2; c->unet_mult[2] = 3; c->unet_mult[3] = 5; c->unet_res = 2;
    c->unet_n_attn = 3; c->unet_attn_ds[0] = 2; c->unet_attn_ds[1] = 4; c->unet_attn_ds[2] = 8; c->head_dim = 32; c->t_steps = 1000;
    c->voc_ch = 512; c->voc_n_rates = 5; const int r[5] = {6, 5, 4, 2, 2}; memcpy(c->voc_rates, r, sizeof(r));
    c->voc_n_kernels = 3; c->voc_kernels[0] = 3; c->voc_kernels[1] = 7; c->voc_kernels[2] = 11;
    c->voc_n_dils = 3; c->voc_dils[0] = 1; c->voc_dils[1] = 3; c->voc_dils[2] = 5; c->aa_taps = 12;
    return EGR_OK;
}

extern "C" int egr_flashsr_destroy(egr_flashsr* m) {
    if (!m) return EGR_OK;
    hipDeviceSynchronize();
    for (void* p : m->owned) hipFree(p);
    if (m->ev_fork) hipEventDestroy(m->ev_fork);
    delete m;                                        // contexts, profile records and the weight maximum release themselves
    return EGR_OK;
}

extern "C" int egr_flashsr_create(egr_flashsr** out, const egr_flashsr_config* cfg, const egr_tensor_desc* tensors, int n_tensors,
                                  unsigned flags, void* stream) {
    EGR_CHECK(out && cfg && tensors && n_tensors > 0, EGR_ERR_ARG, "egr_flashsr_create: null argument");
    *out = nullptr;
    EGR_CHECK(cfg->struct_bytes == (int)sizeof(egr_flashsr_config), EGR_ERR_ARG, "egr_flashsr_config size %d != %d (ABI mismatch)",
              cfg->struct_bytes, (int)sizeof(egr_flashsr_config));
    EGR_CHECK(cfg->vae_levels >= 1 && cfg->vae_levels <= EGR_FSR_MAX && cfg->unet_levels >= 1 && cfg->unet_levels <= EGR_FSR_MAX &&
              cfg->voc_n_rates >= 1 && cfg->voc_n_rates <= EGR_FSR_MAX && cfg->voc_n_kernels >= 1 && cfg->voc_n_kernels <= EGR_FSR_MAX &&
              cfg->voc_n_dils >= 1 && cfg->voc_n_dils <= EGR_FSR_MAX && cfg->unet_n_attn >= 0 && cfg->unet_n_attn <= EGR_FSR_MAX,
              EGR_ERR_ARG, "egr_flashsr_config: level / rate counts out of range");
    EGR_CHECK(!(flags & EGR_FSR_FAST_F16) || !(flags & (EGR_FSR_F32_MFMA | EGR_FSR_SPLIT_BF16X3)), EGR_ERR_ARG,
              "egr_flashsr_create: EGR_FSR_FAST_F16 runs on the fp16 weight terms, which EGR_FSR_F32_MFMA / EGR_FSR_SPLIT_BF16X3 do not keep");
    egr_flashsr* m = new egr_flashsr();
    m->cfg = *cfg;
    m->flags = flags;
    m->ctxs.emplace_back(new FsrCtx());
    m->ctxs[0]->st = (hipStream_t)stream;
    hipGetDevice(&m->device);
    if (const char* e = getenv("EGREGORA_FLASHSR_STREAMS")) { const int g = atoi(e); if (g >= 1 && g <= 4) m->max_groups = g; }
    if (const char* e = getenv("EGREGORA_FLASHSR_WINOGRAD_MIN_CH")) m->wino_min_ch = atoi(e);
    m->h2 = !(flags & (EGR_FSR_F32_MFMA | EGR_FSR_SPLIT_BF16X3));
    if (const char* e = getenv("EGREGORA_FLASHSR_SPLIT")) {
        if (!strcmp(e, "bf16x3")) m->h2 = false;
        else if (!strcmp(e, "f16x1") && m->h2) m->flags |= EGR_FSR_FAST_F16;     // (a handle without fp16 terms cannot run the mode: its flags decide)
    }
    m->h1 = m->h2 && (m->flags & EGR_FSR_FAST_F16) != 0;
    if (const char* e = getenv("EGREGORA_FLASHSR_ROWS")) { const int r = atoi(e); if (r >= 1) m->rows_per_pass = r; }
    if (const char* e = getenv("EGREGORA_FLASHSR_OUT_AMAX")) m->out_amax_on = atoi(e) != 0;
    if (const char* e = getenv("EGREGORA_FLASHSR_DIRECT3X3_MAX_COUT")) m->direct3x3_max_cout = atoi(e);
    if (const char* e = getenv("EGREGORA_FLASHSR_FUSED_AMP")) m->fused_amp = atoi(e) != 0;
    if (const char* e = getenv("EGREGORA_FLASHSR_ARENA_GB")) { const double gb = atof(e); if (gb > 0.0) m->arena_cap = gb * 1e9; }
    build_blocks(m);
    const int down = 1 << (cfg->vae_levels - 1);
    m->lat_h = cfg->n_frames / down; m->lat_w = cfg->n_mels / down;
    const int nb = cfg->n_fft / 2 + 1;
    m->ldm = ((nb + 15) / 16) * 16;
    auto fail = [&](int rc) { egr_flashsr_destroy(m); return rc; };
    int rc = pack_all(m, tensors, n_tensors);
    if (rc) return fail(rc);
    // derived constants travel with the weights (the host computes them exactly as the oracle does): Hann window, mel filterbank,
    // anti-alias FIR, sinusoidal embedding of t = T-1
    const egr_tensor_desc* tw = find(tensors, n_tensors, "const.window");
    const egr_tensor_desc* tf = find(tensors, n_tensors, "const.aa_filter");
    const egr_tensor_desc* tm = find(tensors, n_tensors, "const.mel_fb");
    const egr_tensor_desc* te = find(tensors, n_tensors, "const.time_emb");
    if (!(tw && tf && tm && te)) { set_error("egr_flashsr_create: const.window / const.aa_filter / const.mel_fb / const.time_emb must accompany the weights"); return fail(EGR_ERR_ARG); }
    if (tw->shape[0] != cfg->n_fft || tf->shape[0] != cfg->aa_taps || tm->ndim != 2 || tm->shape[0] != cfg->n_mels || tm->shape[1] != nb ||
        te->shape[te->ndim - 1] != cfg->unet_ch) { set_error("egr_flashsr_create: constant tensor shapes do not match the config"); return fail(EGR_ERR_ARG); }
    void* p = nullptr;
    if ((rc = dev_alloc(m, (size_t)cfg->n_fft * 4, &p))) return fail(rc);
    m->window = (float*)p;
    hipMemcpyAsync(m->window, tw->data, (size_t)cfg->n_fft * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if ((rc = dev_alloc(m, (size_t)cfg->aa_taps * 4, &p))) return fail(rc);
    m->filt = (float*)p;
    hipMemcpyAsync(m->filt, tf->data, (size_t)cfg->aa_taps * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    // mel filterbank [n_mels][nb] as a contraction weight: K = nb (padded to ldm), N = n_mels
    if ((rc = add_packed(m, "mel_fb", tm->data, 0, nb, cfg->n_mels, nb, cfg->n_mels, 1, 1, 1, 1, m->ldm))) return fail(rc);
    {   // cosine schedule at t = T-1 (Nichol & Dhariwal), alpha^2 + sigma^2 = 1
        const double s = 0.008, T = (double)cfg->t_steps, t = T - 1.0;
        auto f = [&](double u) { const double cc = cos((u / T + s) / (1 + s) * M_PI / 2); return cc * cc; };
        double abar = f(t + 1) / f(0);
        abar = abar < 1e-5 ? 1e-5 : (abar > 0.99999 ? 0.99999 : abar);
        m->alpha = (float)sqrt(abar); m->sigma = (float)sqrt(1.0 - abar);
    }
    if ((rc = fold_time_embedding(m, te->data))) return fail(rc);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipGetLastError() != hipSuccess) { set_error("egr_flashsr_create: device work failed"); return fail(EGR_ERR_HIP); }
    *out = m;
    return EGR_OK;
}

extern "C" int egr_flashsr_set_rows_per_pass(egr_flashsr* m, int rows) {
    EGR_CHECK(m && rows >= 1, EGR_ERR_ARG, "bad argument");
    m->rows_per_pass = rows;
    return EGR_OK;
}

extern "C" int egr_flashsr_forward(egr_flashsr* m, const float* x, const float* noise, int rows, int lowpass, float* y, float* const* stages,
                                   void* stream) {
    EGR_CHECK(m && x && noise && y && rows >= 1, EGR_ERR_ARG, "egr_flashsr_forward: null / empty argument");
    ForwardGuard guard(m->device, (hipStream_t)stream);
    m->ctxs[0]->st = (hipStream_t)stream;
    // the introspection walk stays on the three-term kernels (bit-equal to the operator API) unless egr_flashsr_set_split(h, 2) asked
    // for the fp16 operand terms here too (stage taps for the tests)
    Fwd f(*m, m->ctxs[0].get(), rows, m->h2_ready() && m->h2_fwd, &m->prof, m->profiling);
    return forward(f, x, noise, lowpass, y, stages);
}

// x [rows][chunk] -> y [rows][chunk]; rows = chunks x channels ride the batch dimension (reference :366-368) and are processed
// rows_per_pass at a time; the noise of row r is a function of (seed, row_ids[r] or r) only, so results do not depend on how the
// rows are spread over passes or ranks.
extern "C" int egr_streams_overlap_us(void* stream_a, void* stream_b, int spin_us, double* elapsed_us);

// Side streams for concurrent row groups.  HIP multiplexes its streams onto a few hardware queues and two streams on one queue
// run in order, so candidates are CHECKED: two 300 us spin kernels take ~300 us together on different queues, ~600 us on one.
// Verified against the caller's stream and against each other; re-checked when the caller's stream changes.
static int ensure_side_streams(egr_flashsr* m, hipStream_t caller, int want) {
    bool known = false;
    for (hipStream_t s : m->verified_for) known = known || s == caller;
    auto overlaps = [&](hipStream_t a, hipStream_t b) {
        double best = 1e9, us = 0;
        for (int i = 0; i < 2; ++i) { if (egr_streams_overlap_us(a, b, 300, &us) != EGR_OK) return false; best = std::min(best, us); }
        return best < 450.0;
    };
    if (!known) {                                    // drop side contexts that do not overlap with THIS caller stream
        for (size_t i = 1; i < m->ctxs.size();) {
            if (overlaps(caller, m->ctxs[i]->st)) { ++i; continue; }
            hipStreamSynchronize(m->ctxs[i]->st);
            m->ctxs.erase(m->ctxs.begin() + i);
        }
        m->verified_for.assign(1, caller);
    }
    for (int tries = 0; (int)m->ctxs.size() - 1 < want && tries < 12; ++tries) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) break;
        bool ok = overlaps(caller, s);
        for (size_t i = 1; ok && i < m->ctxs.size(); ++i) ok = overlaps(m->ctxs[i]->st, s);
        if (!ok) { hipStreamDestroy(s); continue; }
        m->ctxs.emplace_back(new FsrCtx(s));
    }
    return (int)m->ctxs.size() - 1;
}

// x [rows][chunk] -> y [rows][chunk]; rows = chunks x channels ride the batch dimension (reference :366-368) and are processed
// rows_per_pass at a time; the noise of row r is a function of (seed, row_ids[r] or r) only, so results do not depend on how the
// rows are spread over passes, groups or ranks (beyond fp32 round-off: tile choices follow the row count of a forward).
// A pass of >= 2 * min_group_rows rows is split into up to max_groups contiguous ROW GROUPS that run as concurrent forwards on the
// handle's verified side streams, each with its own scratch arena (fork / join by events around the pass): one group's
// matrix-bound kernels overlap another's HBM-bound ones and fill each other's tails (26 rows: 260 ms in one forward).
// rows of one call; row_ids NULL: implicit ids id_base .. id_base + rows - 1; count_call: the call shows in egr_flashsr_split_info and
// in the profile records (false for the warm-up pass)
static int infer_once(egr_flashsr* m, const float* x, int rows, int lowpass, uint64_t seed, const int64_t* row_ids, int64_t id_base, float* y,
                      void* stream, bool count_call) {
    hipStream_t st0 = (hipStream_t)stream;
    ForwardGuard guard(m->device, st0);                  // everything below touches per-handle state: inside the device's forward lock
    // operand scheme of THIS call's forwards: two fp16 terms with per-row device-side scales (see the h2 fields of the handle), or
    // three bf16 terms.  Either way the call only enqueues work: no read-back, no host synchronisation.
    const bool h2 = m->h2_ready();
    if (h2 && count_call) ++m->h2_calls;
    const int prof_level = count_call ? m->profiling : 0;   // a warm-up pass leaves no profile records behind
    m->ctxs[0]->st = st0;
    const egr_flashsr_config& c = m->cfg;
    const int64_t per_row = (int64_t)m->lat_h * m->lat_w * c.z_ch;
    // scratch budget: fewer rows per pass instead of an allocation failure next to the host's other models
    int rpp = m->rows_per_pass;
    if (m->arena_cap > 0.0) {
        // before any pass has run: ~24 live tensors of the widest activation (n_frames x n_mels x vae_ch) per row, measured 1.5 GB at the full size
        const double est = 24.0 * 4.0 * (double)c.n_frames * c.n_mels * c.vae_ch;
        const double per_row_bytes = m->arena_row_bytes > 0.0 ? m->arena_row_bytes : est;
        rpp = std::max(1, std::min(rpp, (int)(m->arena_cap / per_row_bytes)));
    }
    static const bool trace = getenv("EGR_FSR_TRACE") && atoi(getenv("EGR_FSR_TRACE")) != 0;
    const double t_enter = now_ms(), malloc0 = 1e-3 * (double)g_arena_malloc_us.load();
    double t_side = 0.0;
    int groups_max = prof_level ? 1 : m->max_groups;            // per-kernel timing wants the kernels alone on the chip
    if (groups_max > 1 && std::min(rows, rpp) >= 2 * m->min_group_rows) {
        const double t0 = now_ms();
        groups_max = std::min(m->max_groups, 1 + ensure_side_streams(m, st0, groups_max - 1));   // side contexts of an earlier, wider setting stay idle
        t_side = now_ms() - t0;
    } else {
        groups_max = 1;
    }
    if (groups_max > 1 && !m->ev_fork) EGR_HIP(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
    int rc = EGR_OK;
    // passes of equal size (260 rows at 32 per pass: nine passes of 29 / 28 rows instead of eight of 32 and one of 4)
    const int npass = (rows + rpp - 1) / rpp;
    const int per = (rows + npass - 1) / npass;
    for (int lo = 0; lo < rows && rc == EGR_OK; lo += per) {
        const int n = std::min(per, rows - lo);
        const int G = std::max(1, std::min(groups_max, n / m->min_group_rows));
        if (G > 1) EGR_HIP(hipEventRecord(m->ev_fork, st0));
        int done_rows = 0;
        for (int g = 0; g < G && rc == EGR_OK; ++g) {
            const int ng = (n - done_rows + (G - g) - 1) / (G - g);
            const int glo = lo + done_rows;
            FsrCtx* cx = m->ctxs[g].get();
            if (g > 0) EGR_HIP(hipStreamWaitEvent(cx->st, m->ev_fork, 0));
            Fwd f(*m, cx, ng, h2, &m->prof, prof_level);
            Ten nz;
            rc = new_ten(f, nz, {ng, per_row});
            if (rc == EGR_OK) rc = egr_randn_base(nz.p, per_row, ng, seed, row_ids ? row_ids + glo : nullptr, id_base + glo, f.st);
            if (rc == EGR_OK) rc = forward(f, x + (size_t)glo * c.chunk, nz.p, lowpass, y + (size_t)glo * c.chunk, nullptr);
            if (g > 0) {                                          // join even after an error: nothing may outlive the call unordered
                hipEventRecord(cx->done, cx->st);
                hipStreamWaitEvent(st0, cx->done, 0);
            }
            done_rows += ng;
        }
    }
    if (rc == EGR_OK && per > 0) {                       // what a row of a pass of this size costs in scratch (the arenas never shrink)
        double tot = 0.0;
        for (auto& cx : m->ctxs) tot += (double)cx->arena.total;
        m->arena_row_bytes = std::max(m->arena_row_bytes, tot / std::min(per, rows));
    }
    if (trace) fprintf(stderr, "[egr_flashsr_infer] rows %d: host %.1f ms (side-stream check %.1f, arena hipMalloc %.1f), arenas %.2f GB\n", rows,
                       now_ms() - t_enter, t_side, 1e-3 * (double)g_arena_malloc_us.load() - malloc0, (double)egr_flashsr_scratch_bytes(m) / 1e9);
    return rc;
}

extern "C" int egr_flashsr_infer(egr_flashsr* m, const float* x, int rows, int lowpass, uint64_t seed, const int64_t* row_ids, float* y,
                                 void* stream) {
    EGR_CHECK(m && x && y && rows >= 1, EGR_ERR_ARG, "egr_flashsr_infer: null / empty argument");
    return infer_once(m, x, rows, lowpass, seed, row_ids, 0, y, stream, true);
}

// enabled: egr_flashsr_infer runs the fp16 operand terms on this handle; weights: contraction weights that hold fp16 terms;
// calls: egr_flashsr_infer calls made on the scheme.  (ABI 3 reported a calibration state and re-run count here: the scheme has
// neither any more -- scales are per row and per call, derived on the device.)
extern "C" int egr_flashsr_split_info(egr_flashsr* m, int* enabled, int* weights, int64_t* calls) {
    EGR_CHECK(m != nullptr, EGR_ERR_ARG, "handle is null");
    if (enabled) *enabled = m->h2_ready();
    if (weights) *weights = m->h2_nweights;
    if (calls) *calls = m->h2_calls;
    return EGR_OK;
}

// scheme: 0 = three bf16 terms always, 1 = two fp16 terms with per-row device-side scales in egr_flashsr_infer (needs a handle
// created with the scheme available), 2 = as 1 and egr_flashsr_forward runs the fp16 terms as well (stage taps for tests);
// 3 = one fp16 term (the fast mode) in egr_flashsr_infer, 4 = as 3 and in egr_flashsr_forward.  The fp16 pack serves 1 .. 4: no repacking.
extern "C" int egr_flashsr_set_split(egr_flashsr* m, int scheme) {
    EGR_CHECK(m && scheme >= 0 && scheme <= 4, EGR_ERR_ARG, "bad argument");
    EGR_CHECK(scheme == 0 || m->h2_nweights > 0, EGR_ERR_UNSUPPORTED, "this handle holds no fp16 weight terms");
    m->h2 = scheme >= 1;
    m->h2_fwd = scheme == 2 || scheme == 4;
    m->h1 = scheme >= 3;
    return EGR_OK;
}

// the value egr_flashsr_set_split would have to be given to reach the handle's current state
extern "C" int egr_flashsr_split_scheme(egr_flashsr* m, int* scheme) {
    EGR_CHECK(m && scheme, EGR_ERR_ARG, "null argument");
    *scheme = !m->h2_ready() ? 0 : (m->h1 ? 3 : 1) + (m->h2_fwd ? 1 : 0);
    return EGR_OK;
}

// Scratch budget in bytes for the handle's arenas (0 = none; EGREGORA_FLASHSR_ARENA_GB sets it at creation): egr_flashsr_infer
// lowers its rows per pass until a pass is expected to fit -- slower passes instead of an out-of-memory next to the host's other
// models.  Arenas already allocated are not returned.
extern "C" int egr_flashsr_set_arena_cap(egr_flashsr* m, double bytes) {
    EGR_CHECK(m && bytes >= 0.0, EGR_ERR_ARG, "bad argument");
    m->arena_cap = bytes;
    return EGR_OK;
}

extern "C" int egr_flashsr_warmup(egr_flashsr* m, int rows, void* stream) {
    EGR_CHECK(m && rows >= 1, EGR_ERR_ARG, "bad argument");
    const size_t n = (size_t)rows * m->cfg.chunk;
    DevBuf buf;
    if (!buf.alloc(2 * n * sizeof(float))) { set_error("egr_flashsr_warmup: hipMalloc(%zu) failed", 2 * n * sizeof(float)); return EGR_ERR_ALLOC; }
    float* const x = buf.as<float>();
    int rc = EGR_OK;
    if (hipMemsetAsync(x, 0, n * sizeof(float), (hipStream_t)stream) != hipSuccess) rc = EGR_ERR_HIP;
    if (rc == EGR_OK) rc = infer_once(m, x, rows, 0, 0, nullptr, 0, x + n, stream, false);      // (split_info counts the host's calls, not this one)
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == EGR_OK) { set_error("egr_flashsr_warmup: device work failed"); rc = EGR_ERR_HIP; }
    return rc;                                           // (the buffer goes after the synchronise)
}

extern "C" int egr_flashsr_set_streams(egr_flashsr* m, int max_groups, int min_group_rows) {
    EGR_CHECK(m && max_groups >= 1 && max_groups <= 4 && min_group_rows >= 1, EGR_ERR_ARG, "bad argument");
    m->max_groups = max_groups;
    m->min_group_rows = min_group_rows;
    return EGR_OK;
}

extern "C" int egr_flashsr_set_profiling(egr_flashsr* m, int enable) {
    EGR_CHECK(m != nullptr, EGR_ERR_ARG, "handle is null");
    m->prof.clear();
    m->profiling = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return EGR_OK;
}

// Aggregated HIP-event timing of the MFMA contraction launches since profiling was switched on: entry i of the distinct kernel
// instantiations -> name, launches, flops, milliseconds.  Level 2 adds the graph's other operator launches, each under the name of the
// entry point the walker called (zero flops).  Returns the number of distinct kinds through *count when kind_buf is null.
extern "C" int egr_flashsr_profile(egr_flashsr* m, int index, char* kind_buf, size_t buflen, int64_t* launches, double* flops, double* ms,
                                   int* count) {
    EGR_CHECK(m != nullptr, EGR_ERR_ARG, "handle is null");
    EGR_HIP(hipDeviceSynchronize());
    std::map<std::string, std::tuple<int64_t, double, double>> agg;
    static const bool dump = getenv("EGR_FSR_PROFILE_DUMP") && atoi(getenv("EGR_FSR_PROFILE_DUMP")) != 0;
    for (auto& r : m->prof) {
        float t = 0.f;
        hipEventElapsedTime(&t, r.ev.a, r.ev.b);
        if (dump && count && !kind_buf)              // dev: every timed launch with its layer and shape (once per read-out)
            fprintf(stderr, "[egr_flashsr profile] %-36s %9.3f ms %8.1f GFLOP %7.1f TF/s-eq  %s\n", r.kind.c_str(), t, r.flops / 1e9, t > 0 ? r.flops / t / 1e9 : 0.0,
                    r.detail.c_str());
        auto& e = agg[r.kind];
        std::get<0>(e) += 1; std::get<1>(e) += r.flops; std::get<2>(e) += t;
    }
    if (count) *count = (int)agg.size();
    if (!kind_buf) return EGR_OK;
    EGR_CHECK(index >= 0 && index < (int)agg.size(), EGR_ERR_ARG, "profile index out of range");
    auto it = agg.begin();
    std::advance(it, index);
    snprintf(kind_buf, buflen, "%s", it->first.c_str());
    if (launches) *launches = std::get<0>(it->second);
    if (flops) *flops = std::get<1>(it->second);
    if (ms) *ms = std::get<2>(it->second);
    return EGR_OK;
}

// Dense-contraction flops of one forward over `rows` rows (dry run with counting on; 2 Cin Cout Kh Kw Hout Wout per conv as executed).
extern "C" int egr_flashsr_flop_count(egr_flashsr* m, int rows, double* flops, void* stream) {
    EGR_CHECK(m && flops && rows >= 1, EGR_ERR_ARG, "bad argument");
    ForwardGuard guard(m->device, (hipStream_t)stream);
    m->ctxs[0]->st = (hipStream_t)stream;
    const egr_flashsr_config& c = m->cfg;
    double sum = 0.0;
    Fwd f(*m, m->ctxs[0].get(), rows, false, &m->prof, m->profiling, &sum);   // the bf16 terms, counting
    Ten x, nz, y;
    EGR_TRY(new_ten(f, x, {rows, c.chunk}));
    EGR_TRY(new_ten(f, nz, {rows, (int64_t)m->lat_h * m->lat_w * c.z_ch}));
    EGR_TRY(new_ten(f, y, {rows, c.chunk}));
    EGR_HIP(hipMemsetAsync(x.p, 0, x.bytes, f.st));
    EGR_TRY(egr_randn(nz.p, (int64_t)m->lat_h * m->lat_w * c.z_ch, rows, 0, nullptr, f.st));
    const int rc = forward(f, x.p, nz.p, 0, y.p, nullptr);
    EGR_HIP(hipStreamSynchronize(f.st));
    *flops = sum;
    return rc;
}

extern "C" int64_t egr_flashsr_scratch_bytes(egr_flashsr* m) {
    int64_t t = 0;
    if (m) for (auto& c : m->ctxs) t += (int64_t)c->arena.total;
    return t;
}

// ---------------------------------------------------------------------------------------------------- weight blob files
// "EGRW" container: what `egr_flashsr_create` takes, on disk -- written once by the host that owns checkpoint I/O
// (flashsr_weights.write_blob) and loadable from plain C:
//   char magic[8] = "EGRW0001"; int32 config_bytes; egr_flashsr_config; int32 n_tensors;
//   n x { int32 name_len; char name[name_len]; int32 ndim; int64 shape[4]; int64 offset (bytes from file start); }
//   ... fp32 data, each tensor 64-byte aligned
extern "C" int egr_flashsr_create_from_file(egr_flashsr** out, const char* path, unsigned flags, void* stream) {
    EGR_CHECK(out && path, EGR_ERR_ARG, "null argument");
    *out = nullptr;
    // nothing may throw across the C boundary: allocation failures of the host buffers become EGR_ERR_ALLOC
    try {
        FILE* f = fopen(path, "rb");
        EGR_CHECK(f != nullptr, EGR_ERR_ARG, "cannot open %s", path);
        std::vector<char> buf;
        long sz = -1;
        if (fseek(f, 0, SEEK_END) == 0) sz = ftell(f);
        if (sz <= 16 || fseek(f, 0, SEEK_SET) != 0) {
            fclose(f);
            set_error("%s is not an EGRW0001 weight blob (size %ld)", path, sz);
            return EGR_ERR_ARG;
        }
        buf.resize((size_t)sz);
        const size_t got = fread(buf.data(), 1, (size_t)sz, f);
        fclose(f);
        EGR_CHECK(got == (size_t)sz && memcmp(buf.data(), "EGRW0001", 8) == 0, EGR_ERR_ARG, "%s is not an EGRW0001 weight blob", path);
        size_t pos = 8;
        auto rd = [&](void* dst, size_t n) -> bool { if (n > buf.size() - pos) return false; memcpy(dst, buf.data() + pos, n); pos += n; return true; };
        int32_t cb = 0, nt = 0;
        egr_flashsr_config cfg;
        constexpr int32_t kMaxTensors = 1 << 20;
        bool ok = rd(&cb, 4) && cb == (int32_t)sizeof(cfg) && rd(&cfg, sizeof(cfg)) && rd(&nt, 4) && nt > 0 && nt <= kMaxTensors;
        EGR_CHECK(ok, EGR_ERR_ARG, "%s: header does not match this library's egr_flashsr_config (%d bytes) or tensor count out of range", path, (int)sizeof(cfg));
        std::vector<std::string> names(nt);
        std::vector<egr_tensor_desc> ds(nt);
        std::vector<int64_t> offs(nt);
        std::vector<size_t> bytes(nt);
        size_t total = 0;
        for (int i = 0; i < nt && ok; ++i) {
            int32_t nl = 0, nd = 0;
            ok = rd(&nl, 4) && nl > 0 && nl < 512;
            if (ok) { names[i].resize(nl); ok = rd(&names[i][0], nl); }
            ok = ok && rd(&nd, 4) && nd >= 0 && nd <= 4 && rd(ds[i].shape, 32) && rd(&offs[i], 8);
            if (!ok) break;
            ds[i].ndim = nd;
            // element count without overflow: every extent non-negative, the running product bounded by what the file can hold
            const size_t cap = buf.size() / 4;
            size_t ne = 1;
            for (int d = 0; d < nd && ok; ++d) {
                const int64_t e = ds[i].shape[d];
                ok = e >= 0 && (e == 0 || ne <= cap / (size_t)e);
                if (ok) ne *= (size_t)e;
            }
            ok = ok && offs[i] >= 0 && (size_t)offs[i] <= buf.size() && ne <= (buf.size() - (size_t)offs[i]) / 4;
            bytes[i] = ne * 4;
            total += (bytes[i] + 255) & ~(size_t)255;
        }
        EGR_CHECK(ok, EGR_ERR_ARG, "%s: corrupt tensor index", path);
        DevBuf blob;
        if (!blob.alloc(total + 256)) {
            set_error("hipMalloc of %zu bytes for the weight blob failed", total + 256);
            return EGR_ERR_ALLOC;
        }
        char* const dev = blob.as<char>();
        size_t dpos = 0;
        for (int i = 0; i < nt; ++i) {
            if (bytes[i]) {
                const hipError_t ce = hipMemcpy(dev + dpos, buf.data() + offs[i], bytes[i], hipMemcpyHostToDevice);
                if (ce != hipSuccess) {
                    set_error("hipMemcpy of tensor %s -> %s", names[i].c_str(), hipGetErrorString(ce));
                    return EGR_ERR_HIP;
                }
            }
            ds[i].name = names[i].c_str();
            ds[i].data = (const float*)(dev + dpos);
            dpos += (bytes[i] + 255) & ~(size_t)255;
        }
        return egr_flashsr_create(out, &cfg, ds.data(), nt, flags, stream);   // (synchronises before it returns; the blob goes after)
    } catch (const std::bad_alloc&) {
        set_error("%s: out of host memory while reading the weight blob", path);
        return EGR_ERR_ALLOC;
    } catch (...) {
        set_error("%s: unexpected failure while reading the weight blob", path);
        return EGR_ERR_ARG;
    }
}
