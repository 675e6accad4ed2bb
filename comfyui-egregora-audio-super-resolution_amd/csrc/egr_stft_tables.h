// Per-(device, n_fft) tables of the real-input LDS transforms (k_stft_mag, k_stft_frames, k_wpe_stft, k_wpe_istft):
// defined in egr_glue.hip.
#pragma once
#include "egr_fft_device.h"

namespace egr {

struct StftTables {
    FftDesc fd;            // schedule of the half-length complex transform
    cplx *tw, *wsplit;     // W_{n_fft/2}^j, j < n_fft/2 ; W_{n_fft}^k, k <= n_fft/2 (device)
};
// Builds the tables on first use (hipMalloc + a blocking copy, once per device and n_fft).
int stft_tables(int n_fft, StftTables* out);

}  // namespace egr
