// The output stage's units by job (request_*.hip), as request_launch.hip sees them: one function per stage of launch_pack_plan,
// each defined beside its kernels.  A stage decides from the plan which of its kernels run, and launches them on s; the plan's
// tables are in `t` already.  d_y: the resampled streams (null when the plan has none); out: the packed buffer.  Internal: the
// rest of the library goes through kx_common.h (launch_output_plan).
#pragma once
#include "kx_common.h"

namespace kx {

// one launch of `kernel` on s without dynamic LDS, and its check
template <typename... P, typename... A>
inline void launch_checked(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, s, static_cast<P>(args)...);
    KX_HIP(hipGetLastError());
}

// {p, g} of every request, where a measured plan has them in the packed buffer; null for any other plan
inline double* plan_levels(const OutputPlan& plan, char* out) {
    return plan.measured ? reinterpret_cast<double*>(out + plan.levels_off) : nullptr;
}

// request_resample.hip: the resampler (whole streams or pieces) when some request carries a rate code, and the carries of a plan with pieces
void launch_resample_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                           hipStream_t s);
// request_levels.hip: a measured plan's peak pass, meter, true peak and the two gain kernels
void launch_measure_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                          hipStream_t s);
// request_limit.hip: the limiter and its report, of a plan with a limited request
void launch_limit_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                        hipStream_t s);
// request_flac.hip: frames, layout and gather, of a plan with a FLAC request
void launch_flac_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                       hipStream_t s);
// request_adpcm.hip: the blocks of a plan with an ADPCM request
void launch_adpcm_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                        hipStream_t s);
// request_pack.hip: the packer, in the form the plan's flags name, when the plan has a body
void launch_pack_stage(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, char* out,
                       hipStream_t s);

}  // namespace kx
