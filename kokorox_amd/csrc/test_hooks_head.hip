// Kernel hooks of tests/ (include/kokorox_hip_test.h), the back half's kernels that are no conv: harmonic source, the STFT pair, the
// up-sampling pool.
#include "test_hooks.h"

using namespace kx_test;

namespace {
constexpr int HEAD_MAX_B = 64;        // utterances per hook call
constexpr int HEAD_MAX_F = 64;        // frames per utterance for the STFT hooks (38 400 samples, 7 681 STFT frames)
constexpr int SOURCE_MAX_F = 2048;    // frames per utterance for the source hook (four chunks of its phase kernel)
}  // namespace

extern "C" {

int kx_test_source(int device_id, const float* f0, int B, int F2, const float* lin_w, float lin_b, uint64_t seed,
                   uint64_t utt_base, int noise_off, float* out, char* err, size_t err_len) {
    // every row its full length: the ragged hook with frames[b] = F2 / 2 (nothing of `out` is left as the sentinel)
    if (!(B > 0 && B <= 64 && F2 > 0 && (F2 % 2) == 0))
        return guarded_free(err, err_len, [] { throw Error(KX_ERR_INVALID, "test_source: bad argument"); });
    const std::vector<int32_t> fr((size_t)B, F2 / 2);
    return kx_test_source_ragged(device_id, f0, fr.data(), B, F2 / 2, lin_w, lin_b, seed, utt_base, nullptr, nullptr, noise_off, out, err,
                                 err_len);
}

int kx_test_source_ragged(int device_id, const float* f0, const int32_t* frames, int B, int Fmax, const float* lin_w, float lin_b,
                          uint64_t seed, uint64_t utt_base, const uint64_t* utt_seeds, const uint32_t* utt_index, int noise_off,
                          float* out, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(f0 && frames && lin_w && out && B > 0 && B <= HEAD_MAX_B && Fmax > 0 && Fmax <= SOURCE_MAX_F && (utt_seeds || !utt_index),
                   "test_source_ragged: bad argument");
        check_lens(frames, B, Fmax, "test_source_ragged: frames out of range");
        KX_HIP(hipSetDevice(device_id));
        kx::init_dft_tables();
        DevMem dm;
        // f0 on padded rows: NaN in the padding and in every step >= 2 frames[b]
        const int L2 = 2 * Fmax, f0_ld = pad32(L2);
        const std::vector<float> fp = padded_rows(f0, B, 1, L2, f0_ld, POISON, frames, 2);
        const float* d_f0 = guarded_upload(dm, fp);
        const int* d_fr = dm.up(frames, B);
        const float* d_w = dm.up(lin_w, 9);
        const float* d_b = dm.up(&lin_b, 1);
        const uint64_t* d_seeds = utt_seeds ? dm.up(utt_seeds, B) : nullptr;
        const uint32_t* d_index = utt_index ? dm.up(utt_index, B) : nullptr;
        // the phase workspace [B][9][2 Fmax] as the model sizes it, and the output on rows longer than 600 Fmax
        const size_t n_ph = (size_t)B * 9 * L2;
        float* phase = guarded_buffer(dm, n_ph, POISON);
        const int Ls = 600 * Fmax, har_ld = pad32(Ls) + 32;
        const size_t n_har = (size_t)B * har_ld;
        float* har = guarded_buffer(dm, n_har, SENTINEL);
        kx::launch_source(d_f0, f0_ld, d_fr, B, Fmax, d_w, d_b, seed, utt_base, d_seeds, d_index, noise_off, phase, har, har_ld, nullptr);
        KX_HIP(hipDeviceSynchronize());
        // (samples >= 600 frames[b] go back as they are: the sentinel, if the kernel left them alone)
        unpad_rows(har, (size_t)B, Ls, har_ld, out, "test_source_ragged: source_sample_kernel wrote into the row padding");
        guard_untouched(har + n_har, "test_source_ragged: source_sample_kernel wrote past its tensor");
        guard_untouched(phase + n_ph, "test_source_ragged: source_phase_kernel wrote past its workspace");
        guard_untouched(d_f0 + fp.size(), "test_source_ragged: a kernel wrote behind f0");
    });
}

int kx_test_stft(int device_id, const float* hs, int B, int hs_ld, const int32_t* frames, int Fmax, int variant, float* har, char* err,
                 size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(hs && frames && har && B > 0 && B <= HEAD_MAX_B && Fmax > 0 && Fmax <= HEAD_MAX_F && hs_ld >= 600 * Fmax &&
                       hs_ld <= 600 * Fmax + 4096 && (variant == kx::STFT_ONNX || variant == kx::STFT_TORCH),
                   "test_stft: bad argument");
        check_lens(frames, B, Fmax, "test_stft: frames out of range");
        KX_HIP(hipSetDevice(device_id));
        kx::init_dft_tables();
        DevMem dm;
        // the source rows as the caller strides them: NaN from sample 600 frames[b] on
        const std::vector<float> hp = padded_rows(hs, B, 1, hs_ld, hs_ld, POISON, frames, 600);
        const float* d_hs = guarded_upload(dm, hp);
        const int* d_fr = dm.up(frames, B);
        const int nfmax = 120 * Fmax + 1, ld = pad32(nfmax);
        const size_t n = (size_t)B * 22 * ld;
        float* d_har = guarded_buffer(dm, n, SENTINEL);
        kx::launch_stft(d_hs, hs_ld, d_har, (long)22 * ld, ld, d_fr, B, Fmax, variant, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_har, (size_t)B * 22, nfmax, ld, har, "test_stft: stft_kernel wrote into the row padding");
        guard_untouched(d_har + n, "test_stft: stft_kernel wrote past its tensor");
        guard_untouched(d_hs + hp.size(), "test_stft: stft_kernel wrote behind its input");
    });
}

int kx_test_istft_head(int device_id, const float* cp, int B, const int32_t* frames, int Fmax, int variant, float* spec, float* audio,
                       char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(cp && frames && spec && audio && B > 0 && B <= HEAD_MAX_B && Fmax > 0 && Fmax <= HEAD_MAX_F &&
                       (variant == kx::STFT_ONNX || variant == kx::STFT_TORCH),
                   "test_istft_head: bad argument");
        check_lens(frames, B, Fmax, "test_istft_head: frames out of range");
        KX_HIP(hipSetDevice(device_id));
        kx::init_dft_tables();
        DevMem dm;
        // conv_post's output on the model's padded rows: NaN in the padding and from frame 120 frames[b] + 1 on
        const int nfmax = 120 * Fmax + 1, ld = pad32(nfmax);
        const size_t n = (size_t)B * 22 * ld;
        const float* d_cp = guarded_upload(dm, padded_rows(cp, B, 22, nfmax, ld, POISON, frames, 120, 1));
        const int* d_fr = dm.up(frames, B);
        float* d_spec = guarded_buffer(dm, n, SENTINEL);
        const int Ls = 600 * Fmax, audio_ld = pad32(Ls) + 32;
        const size_t n_a = (size_t)B * audio_ld;
        float* d_audio = guarded_buffer(dm, n_a, SENTINEL);
        kx::launch_istft_head(d_cp, (long)22 * ld, ld, d_spec, d_audio, audio_ld, d_fr, B, Fmax, variant, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_spec, (size_t)B * 22, nfmax, ld, spec, "test_istft_head: istft_spec_kernel wrote into the row padding");
        unpad_rows(d_audio, (size_t)B, Ls, audio_ld, audio, "test_istft_head: istft_ola_kernel wrote into the row padding");
        guard_untouched(d_spec + n, "test_istft_head: istft_spec_kernel wrote past its tensor");
        guard_untouched(d_audio + n_a, "test_istft_head: istft_ola_kernel wrote past its tensor");
        guard_untouched(d_cp + n, "test_istft_head: a kernel wrote behind its input");
    });
}

int kx_test_pool_up2(int device_id, const float* x, int B, int C, int L, const int32_t* lens, const float* norm, int n_bs, const float* w,
                     const float* bias, float slope, float* y, char* err, size_t err_len) {
    return guarded_free(err, err_len, [&] {
        check_device(device_id);
        KX_REQUIRE(x && lens && norm && w && bias && y && B > 0 && B <= HEAD_MAX_B && C > 0 && C <= 1024 && L > 0 && L <= 4096 && n_bs > C &&
                       n_bs <= 2048,
                   "test_pool_up2: bad argument");
        check_lens(lens, B, L, "test_pool_up2: lens out of range");
        KX_HIP(hipSetDevice(device_id));
        DevMem dm;
        // x on the model's padded rows: NaN in the padding and in every column >= lens[b]
        const int x_ld = pad32(L);
        const std::vector<float> xp = padded_rows(x, B, C, L, x_ld, POISON, lens);
        const float* d_x = guarded_upload(dm, xp);
        // the (mean, scale, shift) planes [3][B][n_bs]: an utterance's C values at the front of its n_bs slots, the others NaN
        const std::vector<float> pl = padded_rows(norm, 3 * B, 1, C, n_bs, POISON);
        const float* d_pl = dm.up(pl.data(), pl.size());
        const float* d_w = dm.up(w, (size_t)C * 3);
        const float* d_bias = dm.up(bias, (size_t)C);
        const int* d_len = dm.up(lens, B);
        // y on rows of another stride than x's
        const int y_ld = pad32(2 * L) + 32;
        const size_t n = (size_t)B * C * y_ld;
        float* d_y = guarded_buffer(dm, n, SENTINEL);
        kx::launch_pool_up2(d_x, (long)C * x_ld, x_ld, C, d_pl, d_pl + (size_t)B * n_bs, d_pl + (size_t)2 * B * n_bs, n_bs, slope, d_w, d_bias,
                            d_y, (long)C * y_ld, y_ld, kx::LenMap{d_len, 1, 0}, B, L, nullptr);
        KX_HIP(hipDeviceSynchronize());
        unpad_rows(d_y, (size_t)B * C, 2 * L, y_ld, y, "test_pool_up2: pool_up2_kernel wrote into the row padding");
        guard_untouched(d_y + n, "test_pool_up2: pool_up2_kernel wrote past its tensor");
        guard_untouched(d_x + xp.size(), "test_pool_up2: pool_up2_kernel wrote behind its input");
    });
}

}  // extern "C"
