// The four-times oversampling interpolation that the true-peak meter (request_levels.hip) and the limiter (request_limit.hip)
// share: its geometry, its 72 taps and the chains of a lane.  Both units include this header, so every table and constant of it is
// written once (include/kokorox_hip.h, "levels": PEAK_TRUE).
#pragma once
#include "kx_common.h"
#include "truepeak_taps.h"

namespace kx {

constexpr int TP_THREADS = 256;
constexpr int TP_BEFORE = TRUEPEAK_NTAPS / 2 - 1, TP_BEHIND = TRUEPEAK_NTAPS / 2;  // j = n - 11 .. n + 12
constexpr int TP_LDS = (int)LEVEL_WINDOW + TP_BEFORE + TP_BEHIND;                    // 4119 floats
constexpr int TP_GROUP = 8;                                                          // samples of a lane in flight
static_assert(LEVEL_WINDOW % (TP_THREADS * TP_GROUP) == 0 && KX_TRUEPEAK_PHASES == 3 && KX_TRUEPEAK_NTAPS == 24, "whole groups, [3][24] taps");
__device__ const uint32_t truepeak_tap_bits[TRUEPEAK_PHASES * TRUEPEAK_NTAPS] = {KX_TRUEPEAK_TAPS_1, KX_TRUEPEAK_TAPS_2, KX_TRUEPEAK_TAPS_3};
// The 24-tap interpolation of TP_GROUP samples of a lane, TP_THREADS apart: sample k reads xp[TP_THREADS k + 0 .. 23], its inputs
// j = n - 11 .. n + 12 ascending, and ts holds the 72 taps as float64.  request_truepeak_kernel and request_limit_kernel share it.
__device__ __forceinline__ void truepeak_chains(const float* __restrict__ xp, const double* __restrict__ ts,
                                                double (&acc)[TRUEPEAK_PHASES][TP_GROUP]) {
#pragma unroll
    for (int f = 0; f < TRUEPEAK_PHASES; ++f)
#pragma unroll
        for (int k = 0; k < TP_GROUP; ++k) acc[f][k] = 0.0;
#pragma unroll 4
    for (int jj = 0; jj < TRUEPEAK_NTAPS; ++jj) {  // j = n - 11 + jj ascending: tap n - j + 12 = 23 - jj
        const double t1 = ts[TRUEPEAK_NTAPS - 1 - jj], t2 = ts[2 * TRUEPEAK_NTAPS - 1 - jj], t3 = ts[3 * TRUEPEAK_NTAPS - 1 - jj];
#pragma unroll
        for (int k = 0; k < TP_GROUP; ++k) {
            const double x = (double)xp[TP_THREADS * k + jj];
            acc[0][k] += t1 * x;
            acc[1][k] += t2 * x;
            acc[2][k] += t3 * x;
        }
    }
}

}  // namespace kx
