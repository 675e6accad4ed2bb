// What every ragged (many rows of their own lengths per launch) index header shares: the row search in an ascending prefix column, the
// rule that turns a flat tile into (row, first sample, length), and the grid caps.  Free of device-only constructs so that the same
// text compiles for the host: the host checks under tools/ walk it under -fsanitize=address,undefined (tools/evalmany_host_check.cpp
// walks track_of and tile_of directly).  egr_eval_index.h, egr_null_index.h, egr_sinc_index.h and egr_wpe_index.h build on it.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EGR_HD __host__ __device__ __forceinline__
#else
#include <stddef.h>
#define EGR_HD inline
#endif

namespace egr {

// Every grid equals its work count, and HIP launches no grid with gridDim.x * blockDim.x >= 2^32: a total's cap follows from the block
// size of the kernel that consumes it.  The host refuses a table beyond a cap before anything is copied or launched.
constexpr long long EVAL_MAX_WORK_ITEMS = 4294967295LL;
constexpr long long eval_max_grid(int threads) { return EVAL_MAX_WORK_ITEMS / threads; }
constexpr long long EVAL_MAX_GRID_256 = eval_max_grid(256);          // 2^24 - 1: frames, chunks, blocks, tiles of 256-thread workgroups
constexpr long long EVAL_MAX_OFF = 1LL << 60;    // offsets, strides and lengths in floats: sums of two stay inside int64

EGR_HD long long eval_ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// last t in [0, n) with tab[t * stride + col] <= i; the column ascends and starts at or below i (the callers' start at 0)
EGR_HD int track_of(const long long* __restrict__ tab, int n, int stride, int col, long long i) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[(size_t)mid * stride + col] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// flat tile -> row, the tile's first sample inside the row and its length.  Column col_first holds a row's first flat tile (ascending
// from 0), column col_len its samples; a row has ceil(samples / tile) tiles, so no tile spans two rows and only a row's last is short.
EGR_HD int tile_of(const long long* tab, int n, int cols, int col_first, int col_len, int tile, long long flat, long long* first,
                   long long* len) {
    const int r = track_of(tab, n, cols, col_first, flat);
    const long long* e = tab + (size_t)r * cols;
    *first = (flat - e[col_first]) * tile;
    const long long left = e[col_len] - *first;
    *len = left < tile ? left : tile;
    return r;
}

}  // namespace egr
