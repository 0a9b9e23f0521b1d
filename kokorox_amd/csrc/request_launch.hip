// The one way the output stage is launched (gfx950), for the model and for the test hook: a plan's tables copied in, then the
// stages of the units by job in their order (request_units.h).  host_request.h has the tables and the planner that fills them
// (build_output_plan).
#include "kx_common.h"
#include "request_units.h"

namespace kx {

// A plan's tables into `t`, each checked against what its kernels will assume: the request table and the prefixes always, the join
// rows of a joined or levelled plan or one with pieces, and the tables of pieces, levels, loudness, the limiter and FLAC where the
// plan has them.
static void copy_plan_tables(const OutputPlan& plan, const OutputTables& t, void* out, hipStream_t s) {
    const size_t R = plan.req.size(), B = plan.join.size();
    KX_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0 && R <= 65535, "pack: unaligned output or too many requests");
    // (a plan with FLAC: the packer's table has those requests emptied; every other kernel reads the fields the two tables share)
    KX_HIP(hipMemcpyAsync(t.req, plan.has_flac() ? plan.pack_req.data() : plan.req.data(), R * sizeof(PackReq), hipMemcpyHostToDevice, s));
    if (plan.has_flac()) {
        KX_REQUIRE(t.frow && t.finfo && plan.flac.size() == R && plan.pack_req.size() == R && (plan.flac_off & 7) == 0 &&
                       plan.flac_off >= plan.blocks_end() && plan.flac_max_frames <= 0x7FFFFFFF &&
                       (plan.flac_slots == 0 || (t.fslot && t.flen && t.foff && (reinterpret_cast<uintptr_t>(t.fslot) & 15) == 0)),
                   "flac: bad launch argument");
        KX_HIP(hipMemcpyAsync(t.frow, plan.flac.data(), R * sizeof(FlacRow), hipMemcpyHostToDevice, s));
    }
    KX_HIP(hipMemcpyAsync(t.cum, plan.cum.data(), (B + 1) * sizeof(long), hipMemcpyHostToDevice, s));
    if (plan.joined || plan.levelled || plan.has_pieces())
        KX_HIP(hipMemcpyAsync(t.join, plan.join.data(), B * sizeof(JoinRow), hipMemcpyHostToDevice, s));
    if (plan.has_pieces()) {  // (the table of the two piece kernels and the carried tails; both always stage through the join table)
        KX_REQUIRE(t.piece && t.join && (t.piece_tail || plan.tail_in.empty()) && plan.piece.size() == R && (plan.carry_off & 7) == 0 &&
                       plan.carry_off >= plan.report_end() && plan.tail_in.size() <= R * (size_t)PIECE_TAIL,
                   "pieces: bad launch argument");
        KX_HIP(hipMemcpyAsync(t.piece, plan.piece.data(), R * sizeof(PieceRow), hipMemcpyHostToDevice, s));
        if (!plan.tail_in.empty())
            KX_HIP(hipMemcpyAsync(t.piece_tail, plan.tail_in.data(), plan.tail_in.size() * sizeof(float), hipMemcpyHostToDevice, s));
    }
    if (plan.measured) {
        KX_REQUIRE(t.level && t.peak && plan.level.size() == R && (plan.levels_off & 7) == 0, "levels: bad launch argument");
        KX_HIP(hipMemcpyAsync(t.level, plan.level.data(), R * sizeof(LevelSpec), hipMemcpyHostToDevice, s));
    }
    const bool loud = !plan.loud.empty();
    if (loud) {
        KX_REQUIRE(t.loud && t.loud_pow && (t.hops || plan.max_hops == 0) && plan.loud.size() == R && plan.loud_off == plan.levels_off + 16 * (long)R,
                   "loudness: bad launch argument");
        KX_HIP(hipMemcpyAsync(t.loud, plan.loud.data(), R * sizeof(LoudSpec), hipMemcpyHostToDevice, s));
        KX_HIP(hipMemcpyAsync(t.loud_pow, loud_powers(), (size_t)4 * LOUD_POWERS * 16 * sizeof(double), hipMemcpyHostToDevice, s));
    }
    if (plan.limited) {
        KX_REQUIRE(t.limit && t.lpart && (t.lim || plan.lim_floats == 0) && loud && plan.limit.size() == R &&
                       plan.limits_off == plan.loud_off + 16 * (long)R,
                   "limiter: bad launch argument");
        KX_HIP(hipMemcpyAsync(t.limit, plan.limit.data(), R * sizeof(LimitRow), hipMemcpyHostToDevice, s));
    }
}

// The bodies of a plan: its tables copied into `t`, then the stages in this order, each of which launches what the plan asks of it
// and nothing where the plan asks nothing.  d_y: plan.y_floats floats (may be null when that is 0); out: 16-byte aligned,
// plan.total_bytes long (plan.end_bytes() with the blocks behind the bodies).
//   1. the resampler, when some request carries a rate code (the piece form in a plan with pieces), and the carries of such a plan;
//   2. a measured plan (OutputPlan::measured): the peak pass, the meter of a plan with loudness, the true peak of a plan with the
//      flag, then the gain kernels: {p, g} of every request at out + plan.levels_off, {I, n_g} of every metered one at
//      out + plan.loud_off;
//   3. a plan with a limited request (OutputPlan::limited): the limiter behind the gains it is driven by, the limited streams into
//      t.lim, and its report, {f64(p), g, I, n_g, r} at out + plan.limits_off;
//   4. a plan with a FLAC request (OutputPlan::has_flac): frames, layout and gather, every region's true size at out + plan.flac_off;
//   5. a plan with an ADPCM request (OutputPlan::adpcm_groups > 0): its blocks, at the same place;
//   6. the packer, when the plan has a body: limited, else levelled (some spec is not the plain one), else joined, else plain.
void launch_pack_plan(const float* audio, long audio_ld, const OutputPlan& plan, const OutputTables& t, float* d_y, void* out,
                      hipStream_t s) {
    if (plan.max_units <= 0 && !plan.measured && !plan.has_flac() && plan.adpcm_groups <= 0 && !plan.has_pieces()) return;
    copy_plan_tables(plan, t, out, s);
    char* o = static_cast<char*>(out);
    launch_resample_stage(audio, audio_ld, plan, t, d_y, o, s);
    if (plan.measured) {
        launch_measure_stage(audio, audio_ld, plan, t, d_y, o, s);
        if (plan.limited) launch_limit_stage(audio, audio_ld, plan, t, d_y, o, s);
    }
    if (plan.has_flac()) launch_flac_stage(audio, audio_ld, plan, t, d_y, o, s);
    if (plan.adpcm_groups > 0) launch_adpcm_stage(audio, audio_ld, plan, t, d_y, o, s);
    launch_pack_stage(audio, audio_ld, plan, t, d_y, o, s);
}

// The output stage of a call whose plan is built, for the model and for the test hook alike: the bodies into d_packed, and the
// marks of the requests that want them in their block behind the bodies (8-aligned), and behind those the levels of a measured
// plan (and behind those the loudness of a plan that has it), so one copy to the host brings them all (the limits of a plan
// with a limited request are the last block).  The order is resampler, peak, loudness, true peak, gain, limiter, packer, marks.
void launch_output_plan(const float* audio, long audio_ld, const int* dur, const int* lens, const OutputPlan& plan,
                        const OutputTables& t, float* d_y, void* d_packed, hipStream_t s) {
    launch_pack_plan(audio, audio_ld, plan, t, d_y, d_packed, s);
    if (plan.n_marks > 0) launch_token_marks(dur, lens, plan, t, static_cast<char*>(d_packed) + plan.marks_off, s);
}

}  // namespace kx
