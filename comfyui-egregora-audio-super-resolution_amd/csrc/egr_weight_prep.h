// Contraction weights as the launcher (egr_nn_gemm.hip) reads them, prepared once per model on the device: the one path from a
// torch-layout tensor to the fp32 slab-major pack and its term packs.  The FlashSR handle and the DAC handle both go through it, so
// the layout contract of the launcher has one implementation.  No kernels here (body: egr_flashsr_pack.hip).
#pragma once
#include "egr_common.h"

namespace egr {

// power of two that brings a tensor whose largest magnitude is amax to (2^(e-1), 2^e]; 1 for an empty / non-finite measurement
float h2_scale_for(float amax, int e);

// One prepared weight.  The caller owns the memory: it sets K, N (weight_shape) and the destinations it wants filled before the call
// -- w always, w3 / w2 only for the term packs it asks for -- and may release w once the terms are made.
struct PreparedWeight {
    float* w = nullptr;            // fp32 slab-major pack [ceil(K/16)][N][16] (egr_pack_weight), pack_bytes()
    void* w3 = nullptr;            // three bf16 terms of the pack (egr_split3_pack), term_bytes(3)
    void* w2 = nullptr;            // two fp16 terms of w * w_scale (egr_split2h_pack), term_bytes(2)
    float w_scale = 1.f;           // h2_scale_for(largest magnitude of the pack, 13) when w2 is made
    int K = 0, N = 0;              // the GEMM view [K][N]
    int64_t numel = 0;             // floats of the pack (a stack of z packs: all of them)
    int64_t slabs() const { return numel / ((int64_t)N * 16); }
    size_t pack_bytes() const { return (size_t)numel * sizeof(float); }
    size_t term_bytes(int terms) const { return (size_t)numel * terms * 2; }
};
inline void weight_shape(PreparedWeight& w, int K, int N) { w.K = K; w.N = N; w.numel = (int64_t)((K + 15) / 16) * N * 16; }

// The term packs of a packed weight, on `st`: w3 where a destination is set, then w2 where one is set (the pack's largest magnitude is
// measured into amax_slot, one device float, and read back: the call waits for `st` then).
int split_weight(PreparedWeight& w, float* amax_slot, hipStream_t st);
// src (torch layout on the device; layout and Ci .. KW as egr_pack_weight takes them) -> w.w, then split_weight
int prepare_weight(const float* src, int layout, int Ci, int Co, int KH, int KW, PreparedWeight& w, float* amax_slot, hipStream_t st);

}  // namespace egr
