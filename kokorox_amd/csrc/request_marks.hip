// What the output stage takes from the duration head (gfx950): the token timing marks behind the bodies, and the edge durations
// the host's join plan needs.
#include "kx_common.h"
#include "request_units.h"

namespace kx {

// ---- token timing marks (include/kokorox_hip.h has the definition; host_request.h: MarkRow, build_output_plan) ----------------
// One workgroup of 512 per row: lane t holds the duration of token t (0 at and beyond lens[b]: the front half leaves those
// entries of `dur` unwritten, they are never loaded), an exclusive scan in 64 bits, and lane t stores base + K x scan[t] as one
// 8-byte value, coalesced along t; the lane of the last token stores entry T, the row's end, as well.  The scan is one
// __shfl_up ladder inside each wave64 and ONE exchange of the eight wave totals through LDS (one barrier).
// JOINED (a batch with a joined request): the value is (src_base + clamp(600 x scan - skip, 0, keep)) L / M, written as x K / 600
// -- every term is a multiple of 24 and K of 200, so the division is exact; a plain row (skip 0, keep 600 x its frames) gives
// base + K x scan as before.
constexpr int MARK_THREADS = 512;
template <bool JOINED>
__device__ __forceinline__ void token_marks_body(const int* __restrict__ dur, const int* __restrict__ lens,
                                                 const MarkRow* __restrict__ rows, long long* __restrict__ marks) {
    __shared__ long long wave_total[MARK_THREADS / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const MarkRow mr = rows[b];
    if (mr.first < 0) return;  // (the whole workgroup: its request wants no marks)
    const int T = min(lens[b], MARK_THREADS);
    const long long d = t < T ? (long long)dur[(long)b * 512 + t] : 0;
    const int lane = t & 63, wave = t >> 6;
    long long incl = d;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    long long before = 0;
#pragma unroll
    for (int w = 0; w < MARK_THREADS / 64; ++w) before += w < wave ? wave_total[w] : 0;
    incl += before;
    auto mark = [&](long long scan) -> long long {
        if (!JOINED) return mr.base + mr.K * scan;
        long long u = 600 * scan - mr.skip;
        u = u < 0 ? 0 : (u > mr.keep ? mr.keep : u);
        return (mr.src_base + u) * mr.K / 600;
    };
    if (t < T) {
        marks[mr.first + t] = mark(incl - d);
        if (t == T - 1) marks[mr.first + T] = mark(incl);
    }
}
__global__ __launch_bounds__(MARK_THREADS) void token_marks_kernel(const int* __restrict__ dur, const int* __restrict__ lens,
                                                                   const MarkRow* __restrict__ rows,
                                                                   long long* __restrict__ marks) {
    token_marks_body<false>(dur, lens, rows, marks);
}
__global__ __launch_bounds__(MARK_THREADS) void token_marks_joined_kernel(const int* __restrict__ dur, const int* __restrict__ lens,
                                                                          const MarkRow* __restrict__ rows,
                                                                          long long* __restrict__ marks) {
    token_marks_body<true>(dur, lens, rows, marks);
}
// The marks of a plan (n_marks > 0): its mark rows copied into `t`, then one launch.  dur [B][512], lens [B]: device; marks: the
// marks block (8-byte aligned), n_marks values long.  A joined plan: the rows' skip / keep / src_base matter.
void launch_token_marks(const int* dur, const int* lens, const OutputPlan& plan, const OutputTables& t, void* marks, hipStream_t s) {
    const size_t B = plan.mark.size();
    KX_REQUIRE(dur && lens && t.mark && marks && B >= 1 && (reinterpret_cast<uintptr_t>(marks) & 7) == 0, "marks: bad launch argument");
    KX_HIP(hipMemcpyAsync(t.mark, plan.mark.data(), B * sizeof(MarkRow), hipMemcpyHostToDevice, s));
    launch_checked(plan.joined ? token_marks_joined_kernel : token_marks_kernel, dim3((unsigned)B), dim3(MARK_THREADS), s, dur, lens, t.mark,
                   static_cast<long long*>(marks));
}

// ---- joins: the used durations of every row's first and last token, for the host's join plan ---------------------------------
// edges[b] = {dur[b][0], dur[b][lens[b] - 1]}: eight bytes per row behind the duration head, copied to the host beside the
// frame counts before the forward's one host wait.
__global__ void edge_durations_kernel(const int* __restrict__ dur, const int* __restrict__ lens, int2* __restrict__ edges, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int T = min(max(lens[b], 1), 512);
    edges[b] = make_int2(dur[(long)b * 512], dur[(long)b * 512 + T - 1]);
}
void launch_edge_durations(const int* dur, const int* lens, int* edges, int B, hipStream_t s) {
    KX_REQUIRE(dur && lens && edges && B >= 1 && (reinterpret_cast<uintptr_t>(edges) & 7) == 0, "join: bad launch argument");
    launch_checked(edge_durations_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), s, dur, lens, reinterpret_cast<int2*>(edges), B);
}

}  // namespace kx
