// Kernel hooks of tests/ (include/kokorox_hip_test.h), the output stage of a call: the packer, the resampler, the meters and the marks
// kernel through build_output_plan and launch_output_plan, the planner and the launcher the model runs.
#include "test_hooks.h"

using namespace kx_test;

extern "C" {

int kx_test_output_plan(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames_in, const int32_t* dur,
                        const int32_t* lens, const int32_t* chunks_per_request, int R, const int32_t* formats, const kx_join* joins,
                        const uint8_t* want, void* out, int64_t out_cap, int64_t* out_bytes, int64_t* out_samples,
                        int64_t* out_marks, int64_t marks_cap, int64_t* out_n_marks, char* err, size_t err_len) {
    return kx_test_output_plan_levelled(device_id, audio, B, audio_ld, frames_in, dur, lens, chunks_per_request, R, formats, joins, want,
                                        out, out_cap, out_bytes, out_samples, out_marks, marks_cap, out_n_marks, nullptr, nullptr, err,
                                        err_len);
}

int kx_test_output_plan_levelled(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames_in,
                                 const int32_t* dur, const int32_t* lens, const int32_t* chunks_per_request, int R,
                                 const int32_t* formats, const kx_join* joins, const uint8_t* want, void* out, int64_t out_cap,
                                 int64_t* out_bytes, int64_t* out_samples, int64_t* out_marks, int64_t marks_cap,
                                 int64_t* out_n_marks, const kx_level* levels, double* out_levels, char* err, size_t err_len) {
    return kx_test_output_plan_loudness(device_id, audio, B, audio_ld, frames_in, dur, lens, chunks_per_request, R, formats, joins, want,
                                        out, out_cap, out_bytes, out_samples, out_marks, marks_cap, out_n_marks, levels, out_levels,
                                        nullptr, nullptr, nullptr, 0, nullptr, err, err_len);
}

int kx_test_output_plan_loudness(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames_in,
                                 const int32_t* dur, const int32_t* lens, const int32_t* chunks_per_request, int R,
                                 const int32_t* formats, const kx_join* joins, const uint8_t* want, void* out, int64_t out_cap,
                                 int64_t* out_bytes, int64_t* out_samples, int64_t* out_marks, int64_t marks_cap,
                                 int64_t* out_n_marks, const kx_level* levels, double* out_levels, const kx_loudness* loudness,
                                 double* out_loudness, double* out_hops, int64_t hops_cap, int64_t* out_n_hops, char* err,
                                 size_t err_len) {
    return kx_test_output_plan_limited(device_id, audio, B, audio_ld, frames_in, dur, lens, chunks_per_request, R, formats, joins, want,
                                       out, out_cap, out_bytes, out_samples, out_marks, marks_cap, out_n_marks, levels, out_levels,
                                       loudness, out_loudness, out_hops, hops_cap, out_n_hops, nullptr, nullptr, err, err_len);
}

int kx_test_output_plan_limited(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames_in,
                                const int32_t* dur, const int32_t* lens, const int32_t* chunks_per_request, int R,
                                const int32_t* formats, const kx_join* joins, const uint8_t* want, void* out, int64_t out_cap,
                                int64_t* out_bytes, int64_t* out_samples, int64_t* out_marks, int64_t marks_cap,
                                int64_t* out_n_marks, const kx_level* levels, double* out_levels, const kx_loudness* loudness,
                                double* out_loudness, double* out_hops, int64_t hops_cap, int64_t* out_n_hops, const kx_limit* limits,
                                double* out_limits, char* err, size_t err_len) {
    return kx_test_output_plan_flac(device_id, audio, B, audio_ld, frames_in, dur, lens, chunks_per_request, R, formats, joins, want, out,
                                    out_cap, out_bytes, out_samples, out_marks, marks_cap, out_n_marks, levels, out_levels, loudness,
                                    out_loudness, out_hops, hops_cap, out_n_hops, limits, out_limits, nullptr, err, err_len);
}

}  // extern "C"

// The one body of the hooks above and of kx_test_output_plan_pieces: the FLAC hook's arguments, and a call's pieces (all three null:
// every request is run whole).
static int output_plan_hook(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames_in, const int32_t* dur,
                            const int32_t* lens, const int32_t* chunks_per_request, int R, const int32_t* formats, const kx_join* joins,
                            const uint8_t* want, void* out, int64_t out_cap, int64_t* out_bytes, int64_t* out_samples,
                            int64_t* out_marks, int64_t marks_cap, int64_t* out_n_marks, const kx_level* levels, double* out_levels,
                            const kx_loudness* loudness, double* out_loudness, double* out_hops, int64_t hops_cap, int64_t* out_n_hops,
                            const kx_limit* limits, double* out_limits, int64_t* out_lengths, const uint32_t* piece_flags,
                            const kx_piece_carry* carry_in, kx_piece_carry* carry_out, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE((piece_flags ? audio && carry_out : !carry_in && !carry_out), "test_output_plan: bad argument");
        KX_REQUIRE(formats && out_bytes && out_samples && out_n_marks && B > 0 && R > 0 && (frames_in ? !dur : dur && lens) &&
                       ((!want && !joins) || dur) && (audio ? out != nullptr : out_cap == 0 && dur) && (levels ? audio && out_levels : !out_levels) &&
                       (loudness ? audio && out_loudness && out_hops && out_n_hops && hops_cap >= 0 : !out_loudness && !out_hops && !out_n_hops) &&
                       (limits ? audio && out_limits : !out_limits),
                   "test_output_plan: bad argument");
        // what the forward would have brought back: the rows' frame counts and the durations of their two edge tokens
        std::vector<int> frames((size_t)B, 0), edges((size_t)2 * B, 0);
        for (int b = 0; b < B; ++b) {
            long f = frames_in ? frames_in[b] : 0;
            if (dur) {
                KX_REQUIRE(lens[b] >= 1 && lens[b] <= 512, "test_output_plan: lens out of range");
                for (int t = 0; t < lens[b]; ++t) {
                    KX_REQUIRE(dur[(size_t)b * 512 + t] >= 0, "test_output_plan: negative duration");
                    f += dur[(size_t)b * 512 + t];
                }
                edges[(size_t)2 * b] = dur[(size_t)b * 512];
                edges[(size_t)2 * b + 1] = dur[(size_t)b * 512 + lens[b] - 1];
            }
            KX_REQUIRE(f >= 0 && f <= 0x7FFFFFFF / 600 && (!audio || 600L * f <= audio_ld), "test_output_plan: a row is shorter than its frames");
            frames[(size_t)b] = (int)f;
        }
        static_assert(sizeof(kx_join) == sizeof(kx::JoinSpec), "kx_join is JoinSpec");
        const kx::JoinSpec* specs = reinterpret_cast<const kx::JoinSpec*>(joins);
        for (int r = 0; joins && r < R; ++r) KX_REQUIRE(kx::join_spec_ok(specs[r]), "infer: bad join");
        static_assert(sizeof(kx_level) == sizeof(kx::LevelSpec), "kx_level is LevelSpec");
        const kx::LevelSpec* lspecs = reinterpret_cast<const kx::LevelSpec*>(levels);
        for (int r = 0; levels && r < R; ++r) KX_REQUIRE(kx::level_spec_ok(lspecs[r]), "infer: bad level");
        // (a loudness spec of mode 0xFFFFFFFF: that request is not metered, as a plain request beside metered ones in a batch)
        static_assert(sizeof(kx_loudness) == sizeof(kx::LoudSpec), "kx_loudness is LoudSpec");
        const kx::LoudSpec* dspecs = reinterpret_cast<const kx::LoudSpec*>(loudness);
        for (int r = 0; loudness && r < R; ++r)
            KX_REQUIRE(dspecs[r].mode == kx::LOUD_NONE || kx::loud_spec_ok(dspecs[r]), "infer: bad loudness");
        // (a limit spec of mode 0xFFFFFFFF: that request is not limited, as a request beside limited ones in a batch)
        static_assert(sizeof(kx_limit) == sizeof(kx::LimitSpec), "kx_limit is LimitSpec");
        const kx::LimitSpec* mspecs = reinterpret_cast<const kx::LimitSpec*>(limits);
        for (int r = 0; limits && r < R; ++r)
            KX_REQUIRE(mspecs[r].mode == kx::LIMIT_NONE || kx::limit_spec_ok(mspecs[r]), "infer: bad limit");
        // the planner and the launcher of Model::infer_host_once
        kx::RequestLayout layout{chunks_per_request, R, formats, R, want, specs, R, lspecs, levels ? R : 0, dspecs, loudness ? R : 0,
                                 mspecs, limits ? R : 0};
        static_assert(sizeof(kx_piece_carry) == sizeof(kx::PieceCarry), "kx_piece_carry is PieceCarry");
        layout.piece_flags = piece_flags;
        layout.carry_in = reinterpret_cast<const kx::PieceCarry*>(carry_in);
        kx::OutputPlan plan;
        kx::build_output_plan(frames.data(), lens, joins ? edges.data() : nullptr, B, layout, plan);
        for (int r = 0; r < R; ++r) {
            out_bytes[r] = plan.req[(size_t)r].out_bytes;
            out_samples[r] = plan.req[(size_t)r].n_samples;
            out_n_marks[r] = plan.count[(size_t)r];
            if (loudness) {
                const bool on = dspecs[r].mode != kx::LOUD_NONE;
                out_n_hops[r] = on ? plan.req[(size_t)r].n_samples / kx::loud_hop(plan.req[(size_t)r].rate) : 0;
            }
        }
        KX_REQUIRE(!loudness || plan.max_hops <= hops_cap, "test_output_plan: hops_cap is too small");
        KX_REQUIRE(plan.n_marks <= marks_cap && (plan.n_marks == 0 || out_marks), "test_output_plan: marks_cap is too small");
        KX_REQUIRE(!audio || plan.total_bytes <= out_cap, "test_output_plan: out_cap is too small");
        if (!audio && plan.n_marks == 0) return;
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        // the partials of the peak pass: poisoned with a large finite value (an entry the launch did not write must not be read), the
        // guard behind them; the true-peak partials likewise
        const size_t n_peak = (size_t)plan.peak_dwords(), n_tpeak = (size_t)plan.truepeak_dwords();
        uint32_t* d_peak = plan.measured ? guarded_bytes<uint32_t>(dm, n_peak, 0x7F) : nullptr;
        uint32_t* d_tpeak = plan.true_peak ? guarded_bytes<uint32_t>(dm, n_tpeak, 0x7F) : nullptr;
        // the hop energies of the meter: poisoned with NaNs (an entry the launch did not write must not be read), the guard behind them
        const size_t n_hop = (size_t)plan.hop_doubles();
        const bool metered = !plan.loud.empty();  // (a plan with a limited request has the meter's tables, whatever the call gave)
        double* d_hops = metered ? guarded_bytes<double>(dm, n_hop, 0xFF) : nullptr;
        // the limiter's partials, poisoned with zeros (the smallest value of their order: an entry the launch did not write must not
        // be read), and the limit buffer, poisoned with NaNs; the guards behind them
        const size_t n_lpart = (size_t)plan.limit_dwords(), n_lim = (size_t)plan.lim_floats;
        uint32_t* d_lpart = plan.limited ? guarded_bytes<uint32_t>(dm, n_lpart, 0x00) : nullptr;
        float* d_lim = plan.limited ? guarded_bytes<float>(dm, n_lim, 0xFF) : nullptr;
        // the encoder's scratch, all sized by the plan's frames: the slots poisoned with ones, the sizes with a large negative value and
        // the offsets with a large one (an entry the launch did not write must not be read), a guard behind each
        const bool flac = plan.has_flac() && audio;
        const size_t n_slot = (size_t)plan.flac_slots;
        uint32_t* d_fslot = flac ? guarded_bytes<uint32_t>(dm, n_slot * (size_t)(kx::FLAC_SLOT / 4), 0xFF) : nullptr;
        int* d_flen = flac ? guarded_bytes<int>(dm, n_slot, 0x80) : nullptr;
        long* d_foff = flac ? guarded_bytes<long>(dm, n_slot, 0x7F) : nullptr;
        // the carried tails of a plan with pieces: a guard behind them (the kernels only read them)
        const bool pieces = plan.has_pieces();
        const size_t n_tail = plan.tail_in.size();
        float* d_tail = pieces ? guarded_bytes<float>(dm, n_tail, 0xFF) : nullptr;
        const kx::OutputTables tables{dm.get<kx::PackReq>((size_t)R), dm.get<long>((size_t)B + 1), dm.get<kx::JoinRow>((size_t)B),
                                      dm.get<kx::MarkRow>((size_t)B), plan.measured ? dm.get<kx::LevelSpec>((size_t)R) : nullptr, d_peak,
                                      metered ? dm.get<kx::LoudSpec>((size_t)R) : nullptr, d_hops,
                                      metered ? dm.get<double>((size_t)4 * kx::LOUD_POWERS * 16) : nullptr, d_tpeak,
                                      plan.limited ? dm.get<kx::LimitRow>((size_t)R) : nullptr, d_lpart, d_lim,
                                      flac ? dm.get<kx::FlacRow>((size_t)R) : nullptr, flac ? dm.get<kx::FlacInfo>((size_t)R) : nullptr,
                                      d_fslot, d_flen, d_foff, pieces ? dm.get<kx::PieceRow>((size_t)R) : nullptr, d_tail};
        const int* d_dur = dur ? dm.up(dur, (size_t)B * 512) : nullptr;
        const int* d_len = dur ? dm.up(lens, (size_t)B) : nullptr;
        // guards: 64 bytes after the last region, after the resampled streams, after the last mark and after the levels, which
        // the kernels must leave alone.  The marks block is moved 64 bytes back for the first of them, the levels block 64 more
        // for the third (the kernels are handed the addresses, still 8-aligned; the offsets themselves are nothing they see).
        // (the loudness block stays right behind the levels: the two count as one here)
        // (and the limits block right behind the loudness)
        const long body = audio ? plan.total_bytes : 0, n_mk = plan.n_marks * 8;
        const long n_lv = plan.measured ? (plan.limited ? 72L : (metered ? 32L : 16L)) * R : 0;
        if (audio) plan.marks_off += GUARD_BYTES;
        if (plan.measured) plan.levels_off += 2 * GUARD_BYTES;
        if (metered) plan.loud_off = plan.levels_off + 16L * R;
        if (plan.limited) plan.limits_off = plan.loud_off + 16L * R;
        const long mk_off = audio ? plan.marks_off : 0, lv_off = plan.measured ? plan.levels_off : mk_off + n_mk;
        // (the lengths block of a plan with FLAC: behind the guard of the last block, a guard of its own behind it)
        const long blocks_end = plan.measured ? lv_off + n_lv : mk_off + n_mk;
        if (flac) plan.flac_off = (blocks_end + GUARD_BYTES + 7) & ~7L;
        // (the carry block of a plan with pieces: behind the guard of the last block, a guard of its own behind it)
        const long carries = (long)sizeof(kx::PieceCarry) * R, before_carry = flac ? plan.flac_off + 8L * R : blocks_end;
        if (pieces) {
            plan.carry_off = (before_carry + GUARD_BYTES + 7) & ~7L;
            for (int r = 0; r < R; ++r) plan.piece[(size_t)r].carry_off = plan.carry_off + (long)sizeof(kx::PieceCarry) * r;
        }
        const long d_out_bytes = (pieces ? plan.carry_off + carries : before_carry) + GUARD_BYTES;
        char* d_out = dm.get<char>((size_t)d_out_bytes);
        KX_HIP(hipMemset(d_out, GUARD_BYTE, (size_t)d_out_bytes));
        float* d_y = audio && plan.y_floats > 0 ? dm.get<float>((size_t)plan.y_floats + GUARD_BYTES / 4) : nullptr;
        if (d_y) KX_HIP(hipMemset(d_y + plan.y_floats, GUARD_BYTE, GUARD_BYTES));
        if (audio) {
            const float* d_audio = dm.up(audio, (size_t)B * (size_t)audio_ld);
            kx::launch_output_plan(d_audio, (long)audio_ld, d_dur, d_len, plan, tables, d_y, d_out, nullptr);
        } else {  // (the marks alone: no audio is read, no body written)
            kx::launch_token_marks(d_dur, d_len, plan, tables, d_out, nullptr);
        }
        KX_HIP(hipDeviceSynchronize());
        if (audio) {
            KX_HIP(hipMemcpy(out, d_out, (size_t)body, hipMemcpyDeviceToHost));
            guard_untouched(d_out + body, "test_output_plan: the kernel wrote past the last region");
            if (flac) {  // the slack of every region is as it was filled, then the regions move together as in Model::infer_host_once
                std::vector<int64_t> lengths((size_t)R);
                KX_HIP(hipMemcpy(lengths.data(), d_out + plan.flac_off, (size_t)R * 8, hipMemcpyDeviceToHost));
                if (out_lengths) std::memcpy(out_lengths, lengths.data(), (size_t)R * 8);
                guard_untouched(d_out + plan.flac_off - GUARD_BYTES, "test_output_plan: a kernel wrote in front of the lengths");
                guard_untouched(d_out + plan.flac_off + 8L * R, "test_output_plan: the kernel wrote past the last length");
                guard_untouched(d_fslot + n_slot * (size_t)(kx::FLAC_SLOT / 4), "test_output_plan: the encoder wrote past its slots");
                guard_untouched(d_flen + n_slot, "test_output_plan: the encoder wrote past its sizes");
                guard_untouched(d_foff + n_slot, "test_output_plan: the layout wrote past its offsets");
                const unsigned char* body_bytes = static_cast<const unsigned char*>(out);
                for (int r = 0; r < R; ++r) {
                    const kx::PackReq& q = plan.req[(size_t)r];
                    KX_REQUIRE(lengths[(size_t)r] >= 0 && lengths[(size_t)r] <= q.out_bytes, "flac: bad length");
                    for (long i = lengths[(size_t)r]; i < q.out_bytes; ++i)
                        if (body_bytes[q.out_off + i] != GUARD_BYTE) throw Error(KX_ERR_STATE, "test_output_plan: a kernel wrote into a region's slack");
                }
                const long closed = kx::close_flac_gaps(static_cast<char*>(out), plan, lengths.data(), out_bytes);
                std::memset(static_cast<char*>(out) + closed, 0, (size_t)(body - closed));  // (what the moves left behind the last body)
            }
            if (d_y) guard_untouched(d_y + plan.y_floats, "test_output_plan: the resampler wrote past the last stream");
        }
        if (pieces) {
            KX_HIP(hipMemcpy(carry_out, d_out + plan.carry_off, (size_t)carries, hipMemcpyDeviceToHost));
            guard_untouched(d_out + plan.carry_off - GUARD_BYTES, "test_output_plan: a kernel wrote in front of the carries");
            guard_untouched(d_out + plan.carry_off + carries, "test_output_plan: the kernel wrote past the last carry");
            guard_untouched(d_tail + n_tail, "test_output_plan: a kernel wrote past the carried tails");
        }
        if (plan.measured) {
            std::vector<double> lv((size_t)n_lv / 8);
            KX_HIP(hipMemcpy(lv.data(), d_out + lv_off, (size_t)n_lv, hipMemcpyDeviceToHost));
            if (out_levels) std::memcpy(out_levels, lv.data(), (size_t)R * 16);
            if (loudness) {
                for (int r = 0; r < R; ++r) {  // {f64(p), g} of the levels block, {I, n_g} of the loudness block
                    std::memcpy(out_loudness + 4 * r, &lv[(size_t)2 * r], 16);
                    std::memcpy(out_loudness + 4 * r + 2, &lv[(size_t)2 * R + 2 * r], 16);
                }
                // [R][hops_cap]: the first out_n_hops[r] entries of row r are the e[k] the meter stored
                for (int r = 0; r < R; ++r)
                    if (out_n_hops[r] > 0)
                        KX_HIP(hipMemcpy(out_hops + (size_t)r * hops_cap, d_hops + (size_t)r * plan.max_hops, (size_t)out_n_hops[r] * 8,
                                         hipMemcpyDeviceToHost));
            }
            if (metered) guard_untouched(d_hops + n_hop, "test_output_plan: the meter wrote past its table");
            if (plan.limited) {  // the rows of the limited requests; the others' are left as the caller gave them
                for (int r = 0; r < R; ++r)
                    if (plan.limit[(size_t)r].off >= 0) std::memcpy(out_limits + 5 * r, &lv[(size_t)4 * R + 5 * r], 40);
                guard_untouched(d_lpart + n_lpart, "test_output_plan: the limiter wrote past its partials");
                guard_untouched(d_lim + n_lim, "test_output_plan: the limiter wrote past the limit buffer");
            }
            guard_untouched(d_out + lv_off - GUARD_BYTES, "test_output_plan: a kernel wrote in front of the levels");
            guard_untouched(d_out + lv_off + n_lv, "test_output_plan: the kernel wrote past the last level");
            guard_untouched(d_peak + n_peak, "test_output_plan: the peak pass wrote past its table");
            if (d_tpeak) guard_untouched(d_tpeak + n_tpeak, "test_output_plan: the true-peak pass wrote past its table");
        }
        if (plan.n_marks == 0) return;
        KX_HIP(hipMemcpy(out_marks, d_out + mk_off, (size_t)n_mk, hipMemcpyDeviceToHost));
        guard_untouched(d_out + mk_off + n_mk, "test_output_plan: the kernel wrote past the last mark");
    });
}

extern "C" {

int kx_test_output_plan_flac(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames_in, const int32_t* dur,
                             const int32_t* lens, const int32_t* chunks_per_request, int R, const int32_t* formats, const kx_join* joins,
                             const uint8_t* want, void* out, int64_t out_cap, int64_t* out_bytes, int64_t* out_samples,
                             int64_t* out_marks, int64_t marks_cap, int64_t* out_n_marks, const kx_level* levels, double* out_levels,
                             const kx_loudness* loudness, double* out_loudness, double* out_hops, int64_t hops_cap, int64_t* out_n_hops,
                             const kx_limit* limits, double* out_limits, int64_t* out_lengths, char* err, size_t err_len) {
    return output_plan_hook(device_id, audio, B, audio_ld, frames_in, dur, lens, chunks_per_request, R, formats, joins, want, out, out_cap,
                            out_bytes, out_samples, out_marks, marks_cap, out_n_marks, levels, out_levels, loudness, out_loudness, out_hops,
                            hops_cap, out_n_hops, limits, out_limits, out_lengths, nullptr, nullptr, nullptr, err, err_len);
}

int kx_test_output_plan_pieces(int device_id, const float* audio, int B, int64_t audio_ld, const int32_t* frames_in, const int32_t* dur,
                               const int32_t* lens, const int32_t* chunks_per_request, int R, const int32_t* formats, const kx_join* joins,
                               const uint8_t* want, void* out, int64_t out_cap, int64_t* out_bytes, int64_t* out_samples,
                               int64_t* out_marks, int64_t marks_cap, int64_t* out_n_marks, const kx_level* levels, double* out_levels,
                               const kx_loudness* loudness, double* out_loudness, const uint32_t* piece_flags,
                               const kx_piece_carry* carry_in, kx_piece_carry* carry_out, char* err, size_t err_len) {
    // (the hop energies of a metered request beside the pieces are not handed out: room for a hop per frame, which is 25 ms)
    long total = 1 + 51L * (B > 0 ? B : 0);  // (and the longest pause behind every row)
    for (int b = 0; b < B && (frames_in || (dur && lens)); ++b) {
        if (frames_in) total += frames_in[b] > 0 ? frames_in[b] : 0;
        else for (int t = 0; t < lens[b] && t < 512; ++t) total += dur[(size_t)b * 512 + t] > 0 ? dur[(size_t)b * 512 + t] : 0;
    }
    std::vector<double> hops(loudness && R > 0 ? (size_t)R * (size_t)total : 0);
    std::vector<int64_t> n_hops(loudness && R > 0 ? (size_t)R : 0);
    return output_plan_hook(device_id, audio, B, audio_ld, frames_in, dur, lens, chunks_per_request, R, formats, joins, want, out, out_cap,
                            out_bytes, out_samples, out_marks, marks_cap, out_n_marks, levels, out_levels, loudness, out_loudness,
                            loudness ? hops.data() : nullptr, loudness ? total : 0, loudness ? n_hops.data() : nullptr, nullptr, nullptr,
                            nullptr, piece_flags, carry_in, carry_out, err, err_len);
}

}  // extern "C"
