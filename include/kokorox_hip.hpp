// C++ host-side mirror of the reference's `OrtKoko` (kokorox/src/onn/ort_koko.rs:13-91) over the C ABI
// in kokorox_hip.h.  Header-only; link with -lkokorox_hip.  Same two public operations, same meaning:
//   OrtKoko::new(model_path) -> Result<Self, String>          => HipKoko(model_path) (throws std::runtime_error)
//   OrtKoko::infer(tokens, styles, speed) -> Result<Array,..>  => infer(tokens, styles, speed) -> vector<float>
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "kokorox_hip.h"

namespace kokorox {

// The format word of infer_requests / submit_request: a form, optionally or'ed with an output rate (kokorox_hip.h, KX_PACK_*).
constexpr int PACK_F32_MONO = KX_PACK_F32_MONO, PACK_F32_STEREO = KX_PACK_F32_STEREO, PACK_PCM16_MONO = KX_PACK_PCM16_MONO,
              PACK_WAV_F32 = KX_PACK_WAV_F32, PACK_WAV16_BASE64 = KX_PACK_WAV16_BASE64, PACK_MULAW = KX_PACK_MULAW,
              PACK_ALAW = KX_PACK_ALAW, PACK_FLAC = KX_PACK_FLAC, PACK_ADPCM_WAV = KX_PACK_ADPCM_WAV,
              PACK_WAV16 = KX_PACK_WAV16;
constexpr int PACK_RATE_24000 = KX_PACK_RATE_24000, PACK_RATE_8000 = KX_PACK_RATE_8000, PACK_RATE_16000 = KX_PACK_RATE_16000,
              PACK_RATE_48000 = KX_PACK_RATE_48000;

// The resampler behind a format word's rate code (kx_resample_filter; host only): output rate / 24 000 = L / M and the taps.
struct ResampleFilter {
    int32_t L = 1, M = 1;
    std::vector<float> taps;
};
inline ResampleFilter resample_filter(int format_word) {
    ResampleFilter f;
    int32_t n = 0;
    f.taps.resize(KX_RESAMPLE_MAX_TAPS);
    if (kx_resample_filter(format_word, &f.L, &f.M, &n, f.taps.data(), (int)f.taps.size()) != KX_OK)
        throw std::invalid_argument("resample_filter: unknown output format or sample rate");
    f.taps.resize((size_t)n);
    return f;
}

// True peak ("levels" in kokorox_hip.h): PEAK_TRUE OR-ed into the mode of a kx_level or a KxLoudness makes `peak` bound the true
// peak of the body and the reported peak the true peak; truepeak_filter() = the 72 taps of its interpolator, [3][24], phase 1 first.
constexpr uint32_t PEAK_TRUE = KX_PEAK_TRUE;
inline std::vector<float> truepeak_filter() {
    std::vector<float> taps(72);
    if (kx_truepeak_filter(taps.data(), (int)taps.size()) != KX_OK) throw std::invalid_argument("truepeak_filter: failed");
    return taps;
}

// A request's loudness spec ("loudness" in kokorox_hip.h): {KX_LOUDNESS_MEASURE, 0, 0} measures, {KX_LOUDNESS_NORMALIZE, target_lufs,
// peak} scales the body to the target under a ceiling; and what comes back: the peak, the gain, the integrated loudness in LUFS
// (NaN when undefined) and the number of gated blocks.
using KxLoudness = kx_loudness;
struct LoudnessResult {
    double peak, gain, lufs, gated_blocks;
};

// A call's per-token prosody ("prosody" in kokorox_hip.h): each field empty (neutral) or one row per chunk with a value per token;
// and one token of the report: the mean F0 in Hz over its voiced steps (0 when none), their count, the mean of the N curve, its frames.
struct Prosody {
    std::vector<std::vector<float>> rate;
    std::vector<std::vector<int32_t>> frames;
    std::vector<std::vector<float>> pitch, energy;
};
struct ProsodyToken {
    float f0_hz, voiced_steps, energy, frames;
};

// A fit span and what the GPU chose for it ("fit" in kokorox_hip.h): tokens [begin, end) of request `request`, its chunks laid end
// to end, last exactly `frames` frames of 25 ms; lambda is the factor on the span's weights, 1 / lambda speed-like.
struct FitSpan {
    int32_t request, begin, end, frames;
};
struct FitResult {
    float lambda;
    int32_t n_free, held_frames, excess;
};
static_assert(sizeof(FitSpan) == sizeof(kx_fit_span) && sizeof(FitResult) == sizeof(kx_fit_result), "the layouts of kokorox_hip.h");

// A request run in pieces ("pieces" in kokorox_hip.h): the flag bits, and the carry a piece leaves for the next one.
constexpr uint32_t PIECE_FIRST = KX_PIECE_FIRST, PIECE_LAST = KX_PIECE_LAST;
using PieceCarry = kx_piece_carry;

class HipKoko {
  public:
    explicit HipKoko(const std::string& model_path, int device = 0) {
        char err[512] = {0};
        h_ = kx_create(model_path.c_str(), device, err, sizeof(err));
        if (!h_) throw std::runtime_error(std::string("Failed to create Kokoro TTS model: ") + err);
    }
    // One model per device id from one read of the weight file (kx_create_replicas): what a single-process server
    // hands to kx_dispatcher_create (the reference holds one Arc<OrtKoko>, kokorox-openai/src/lib.rs:370-439).
    static std::vector<HipKoko> replicas(const std::string& model_path, const std::vector<int>& devices) {
        std::vector<kx_model*> hs(devices.size(), nullptr);
        char err[512] = {0};
        if (kx_create_replicas(model_path.c_str(), devices.data(), (int)devices.size(), hs.data(), err, sizeof(err)) != KX_OK)
            throw std::runtime_error(std::string("Failed to create Kokoro TTS model: ") + err);
        std::vector<HipKoko> out;
        out.reserve(hs.size());
        for (kx_model* h : hs) out.push_back(HipKoko(h));
        return out;
    }
    kx_model* handle() const { return h_; }
    HipKoko(const HipKoko&) = delete;
    HipKoko& operator=(const HipKoko&) = delete;
    HipKoko(HipKoko&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~HipKoko() { kx_destroy(h_); }

    // tokens: B rows already wrapped with the 0 pads (koko.rs:1169-1175); styles: B rows of 256 floats.
    // Returns the B waveforms back to back; lens (optional) receives the per-utterance sample counts.
    std::vector<float> infer(const std::vector<std::vector<int64_t>>& tokens,
                             const std::vector<std::vector<float>>& styles, float speed, uint64_t seed = 0,
                             std::vector<int64_t>* lens = nullptr) const {
        if (tokens.empty() || tokens[0].empty()) throw std::invalid_argument("infer: empty token list");
        if (styles.size() != tokens.size()) throw std::invalid_argument("infer: one style row per utterance");
        const int B = (int)tokens.size();
        size_t stride = 0;
        for (const auto& t : tokens) stride = t.size() > stride ? t.size() : stride;
        std::vector<int64_t> ids((size_t)B * stride, 0);
        std::vector<int32_t> tl(B);
        std::vector<float> st((size_t)B * KX_STYLE_DIM);
        for (int b = 0; b < B; ++b) {
            tl[b] = (int32_t)tokens[b].size();
            for (size_t i = 0; i < tokens[b].size(); ++i) ids[(size_t)b * stride + i] = tokens[b][i];
            if (styles[b].size() != KX_STYLE_DIM) throw std::invalid_argument("infer: style rows need 256 floats");
            for (int k = 0; k < KX_STYLE_DIM; ++k) st[(size_t)b * KX_STYLE_DIM + k] = styles[b][k];
        }
        float* out = nullptr;
        std::vector<int64_t> ol(B);
        const int rc = kx_infer(h_, ids.data(), (int64_t)stride, tl.data(), B, st.data(), &speed, 1, seed, 0, &out,
                                ol.data());
        if (rc != KX_OK) {
            char msg[512];
            kx_last_error_copy(h_, msg, sizeof(msg));  // (a copy of our own: other threads may fail on this model meanwhile)
            throw std::runtime_error(std::string("kokorox_hip error: ") + msg);
        }
        int64_t total = 0;
        for (int64_t v : ol) total += v;
        std::vector<float> wav(out, out + total);  // the same owned copy as ort_koko.rs:85
        kx_free_audio(out);
        if (lens) *lens = ol;
        return wav;
    }

    // The chunk loop of TTSKoko::tts_raw_audio (koko.rs:947-1191) as one forward (kx_infer_requests): tokens = the chunks (each
    // 0-wrapped), request r owns chunks_per_request[r] consecutive ones, styles = one row per chunk, format = a format word
    // (a KX_PACK_* form, optionally | KX_PACK_RATE_*) for every request.  Returns each request's body: header of the form, if any, then its chunks' samples in order
    // (KX_PACK_WAV_F32: the HTTP body; KX_PACK_WAV16_BASE64: the WebSocket chunk's base64 text).
    std::vector<std::string> infer_requests(const std::vector<std::vector<int64_t>>& tokens,
                                            const std::vector<int32_t>& chunks_per_request,
                                            const std::vector<std::vector<float>>& styles, float speed, uint64_t seed,
                                            int format) const {
        if (tokens.empty() || styles.size() != tokens.size()) throw std::invalid_argument("infer_requests: one style row per chunk");
        const int B = (int)tokens.size(), R = (int)chunks_per_request.size();
        size_t stride = 1;
        for (const auto& t : tokens) stride = t.size() > stride ? t.size() : stride;
        std::vector<int64_t> ids((size_t)B * stride, 0);
        std::vector<int32_t> tl(B);
        std::vector<float> st((size_t)B * KX_STYLE_DIM);
        for (int b = 0; b < B; ++b) {
            tl[b] = (int32_t)tokens[b].size();
            for (size_t i = 0; i < tokens[b].size(); ++i) ids[(size_t)b * stride + i] = tokens[b][i];
            if (styles[b].size() != KX_STYLE_DIM) throw std::invalid_argument("infer_requests: style rows need 256 floats");
            for (int k = 0; k < KX_STYLE_DIM; ++k) st[(size_t)b * KX_STYLE_DIM + k] = styles[b][k];
        }
        void* out = nullptr;
        std::vector<int64_t> nb(R > 0 ? R : 1), ns(R > 0 ? R : 1);
        const int32_t fmt = format;
        const int rc = kx_infer_requests(h_, ids.data(), (int64_t)stride, tl.data(), B, chunks_per_request.data(), R, st.data(),
                                         nullptr, nullptr, 0, &speed, 1, seed, 0, &fmt, 1, &out, nb.data(), ns.data());
        if (rc != KX_OK) {
            char msg[512];
            kx_last_error_copy(h_, msg, sizeof(msg));
            throw std::runtime_error(std::string("kokorox_hip error: ") + msg);
        }
        std::vector<std::string> bodies;
        const char* p = static_cast<const char*>(out);
        for (int r = 0; r < R; ++r) {
            bodies.emplace_back(p, p + nb[r]);
            p += nb[r];
        }
        kx_free_packed(out);
        return bodies;
    }

    // One piece of ONE request (kx_infer_requests_pieces; "pieces" in kokorox_hip.h): tokens = the piece's chunks, flags = PIECE_FIRST
    // and / or PIECE_LAST, carry = the record the piece before left (ignored with PIECE_FIRST) and, on return, the one this piece
    // leaves.  Returns the piece's payload: the payloads of a request's pieces, end to end, are the body of the request run whole.
    std::string infer_request_piece(const std::vector<std::vector<int64_t>>& tokens, const std::vector<std::vector<float>>& styles,
                                    float speed, uint64_t seed, int format, uint32_t flags, PieceCarry& carry) const {
        if (tokens.empty() || styles.size() != tokens.size()) throw std::invalid_argument("infer_requests: one style row per chunk");
        const int B = (int)tokens.size();
        size_t stride = 1;
        for (const auto& t : tokens) stride = t.size() > stride ? t.size() : stride;
        std::vector<int64_t> ids((size_t)B * stride, 0);
        std::vector<int32_t> tl(B);
        std::vector<float> st((size_t)B * KX_STYLE_DIM);
        for (int b = 0; b < B; ++b) {
            tl[b] = (int32_t)tokens[b].size();
            for (size_t i = 0; i < tokens[b].size(); ++i) ids[(size_t)b * stride + i] = tokens[b][i];
            if (styles[b].size() != KX_STYLE_DIM) throw std::invalid_argument("infer_requests: style rows need 256 floats");
            for (int k = 0; k < KX_STYLE_DIM; ++k) st[(size_t)b * KX_STYLE_DIM + k] = styles[b][k];
        }
        void* out = nullptr;
        int64_t nb = 0, ns = 0;
        const int32_t fmt = format, rows = B;
        PieceCarry next{};
        const int rc = kx_infer_requests_pieces(h_, ids.data(), (int64_t)stride, tl.data(), B, &rows, 1, st.data(), nullptr, nullptr, 0,
                                                &speed, 1, seed, 0, &fmt, 1, &out, &nb, &ns, nullptr, nullptr, nullptr, 0, nullptr, 0,
                                                nullptr, &flags, &carry, &next);
        if (rc != KX_OK) {
            char msg[512];
            kx_last_error_copy(h_, msg, sizeof(msg));
            throw std::runtime_error(std::string("kokorox_hip error: ") + msg);
        }
        std::string body(static_cast<const char*>(out), static_cast<const char*>(out) + nb);
        kx_free_packed(out);
        carry = next;
        return body;
    }

    // infer_requests with the token marks of every request (kx_infer_requests_marks; "token marks" in kokorox_hip.h): marks[r]
    // = per chunk of request r its tokens + 1 sample offsets in the request's stream, at the request's output rate.
    std::vector<std::string> infer_requests_marks(const std::vector<std::vector<int64_t>>& tokens,
                                                  const std::vector<int32_t>& chunks_per_request,
                                                  const std::vector<std::vector<float>>& styles, float speed, uint64_t seed,
                                                  int format, std::vector<std::vector<int64_t>>& marks) const {
        if (tokens.empty() || styles.size() != tokens.size()) throw std::invalid_argument("infer_requests: one style row per chunk");
        const int B = (int)tokens.size(), R = (int)chunks_per_request.size();
        size_t stride = 1;
        for (const auto& t : tokens) stride = t.size() > stride ? t.size() : stride;
        std::vector<int64_t> ids((size_t)B * stride, 0);
        std::vector<int32_t> tl(B);
        std::vector<float> st((size_t)B * KX_STYLE_DIM);
        for (int b = 0; b < B; ++b) {
            tl[b] = (int32_t)tokens[b].size();
            for (size_t i = 0; i < tokens[b].size(); ++i) ids[(size_t)b * stride + i] = tokens[b][i];
            if (styles[b].size() != KX_STYLE_DIM) throw std::invalid_argument("infer_requests: style rows need 256 floats");
            for (int k = 0; k < KX_STYLE_DIM; ++k) st[(size_t)b * KX_STYLE_DIM + k] = styles[b][k];
        }
        void* out = nullptr;
        int64_t* mk = nullptr;
        std::vector<int64_t> nb(R > 0 ? R : 1), ns(R > 0 ? R : 1), nm(R > 0 ? R : 1);
        const int32_t fmt = format;
        const int rc = kx_infer_requests_marks(h_, ids.data(), (int64_t)stride, tl.data(), B, chunks_per_request.data(), R, st.data(),
                                               nullptr, nullptr, 0, &speed, 1, seed, 0, &fmt, 1, &out, nb.data(), ns.data(), &mk,
                                               nm.data());
        if (rc != KX_OK) {
            char msg[512];
            kx_last_error_copy(h_, msg, sizeof(msg));
            throw std::runtime_error(std::string("kokorox_hip error: ") + msg);
        }
        std::vector<std::string> bodies;
        marks.clear();
        const char* p = static_cast<const char*>(out);
        for (int r = 0; r < R; ++r) {  // (the marks live in the buffer of `out`: copied before it is released)
            bodies.emplace_back(p, p + nb[r]);
            p += nb[r];
            marks.emplace_back(mk, mk + nm[r]);
            mk += nm[r];
        }
        kx_free_packed(out);
        return bodies;
    }

    // infer_requests with per-token prosody and its report (kx_infer_requests_prosody; "prosody" in kokorox_hip.h): each field of
    // `prosody` is empty (neutral) or holds one row per chunk with a value per token; no joins, no marks.  report[r] = one
    // ProsodyToken per token of request r, chunk after chunk.
    std::vector<std::string> infer_requests_prosody(const std::vector<std::vector<int64_t>>& tokens,
                                                    const std::vector<int32_t>& chunks_per_request,
                                                    const std::vector<std::vector<float>>& styles, float speed, uint64_t seed,
                                                    int format, const Prosody& prosody,
                                                    std::vector<std::vector<ProsodyToken>>& report) const {
        if (tokens.empty() || styles.size() != tokens.size()) throw std::invalid_argument("infer_requests: one style row per chunk");
        const int B = (int)tokens.size(), R = (int)chunks_per_request.size();
        size_t stride = 1;
        for (const auto& t : tokens) stride = t.size() > stride ? t.size() : stride;
        std::vector<int64_t> ids((size_t)B * stride, 0);
        std::vector<int32_t> tl(B);
        std::vector<float> st((size_t)B * KX_STYLE_DIM);
        for (int b = 0; b < B; ++b) {
            tl[b] = (int32_t)tokens[b].size();
            for (size_t i = 0; i < tokens[b].size(); ++i) ids[(size_t)b * stride + i] = tokens[b][i];
            if (styles[b].size() != KX_STYLE_DIM) throw std::invalid_argument("infer_requests: style rows need 256 floats");
            for (int k = 0; k < KX_STYLE_DIM; ++k) st[(size_t)b * KX_STYLE_DIM + k] = styles[b][k];
        }
        // the four arrays laid out as the ids, neutral where a row is shorter than the stride
        auto rows = [&](const auto& given, auto neutral) {
            std::vector<decltype(neutral)> flat;
            if (given.empty()) return flat;
            if (given.size() != tokens.size()) throw std::invalid_argument("infer_requests_prosody: one row per chunk");
            flat.assign((size_t)B * stride, neutral);
            for (int b = 0; b < B; ++b) {
                if (given[b].size() != tokens[b].size()) throw std::invalid_argument("infer_requests_prosody: one value per token");
                for (size_t i = 0; i < given[b].size(); ++i) flat[(size_t)b * stride + i] = given[b][i];
            }
            return flat;
        };
        const std::vector<float> rate = rows(prosody.rate, 1.0f), pitch = rows(prosody.pitch, 1.0f), energy = rows(prosody.energy, 1.0f);
        const std::vector<int32_t> frames = rows(prosody.frames, (int32_t)0);
        const kx_prosody ps = {rate.empty() ? nullptr : rate.data(), frames.empty() ? nullptr : frames.data(),
                               pitch.empty() ? nullptr : pitch.data(), energy.empty() ? nullptr : energy.data()};
        void* out = nullptr;
        float* rp = nullptr;
        std::vector<int64_t> nb(R > 0 ? R : 1), ns(R > 0 ? R : 1), nr(R > 0 ? R : 1);
        const int32_t fmt = format;
        const int rc = kx_infer_requests_prosody(h_, ids.data(), (int64_t)stride, tl.data(), B, chunks_per_request.data(), R, st.data(),
                                                 nullptr, nullptr, 0, &speed, 1, seed, 0, &fmt, 1, &out, nb.data(), ns.data(), nullptr,
                                                 nullptr, nullptr, 0, &ps, &rp, nr.data());
        if (rc != KX_OK) {
            char msg[512];
            kx_last_error_copy(h_, msg, sizeof(msg));
            throw std::runtime_error(std::string("kokorox_hip error: ") + msg);
        }
        std::vector<std::string> bodies;
        report.clear();
        const char* p = static_cast<const char*>(out);
        for (int r = 0; r < R; ++r) {  // (the report lives in the buffer of `out`: copied before it is released)
            bodies.emplace_back(p, p + nb[r]);
            p += nb[r];
            std::vector<ProsodyToken> tok((size_t)nr[r]);
            for (int64_t i = 0; i < nr[r]; ++i) tok[(size_t)i] = ProsodyToken{rp[4 * i], rp[4 * i + 1], rp[4 * i + 2], rp[4 * i + 3]};
            rp += 4 * nr[r];
            report.push_back(std::move(tok));
        }
        kx_free_packed(out);
        return bodies;
    }

    // infer_requests with fit spans (kx_infer_requests_fitted; "fit" in kokorox_hip.h): `spans` sorted by (request, begin) and
    // disjoint; no prosody arrays, no joins, no marks, no report.  fit[i] = what the GPU chose for spans[i].
    std::vector<std::string> infer_requests_fitted(const std::vector<std::vector<int64_t>>& tokens,
                                                   const std::vector<int32_t>& chunks_per_request,
                                                   const std::vector<std::vector<float>>& styles, float speed, uint64_t seed, int format,
                                                   const std::vector<FitSpan>& spans, std::vector<FitResult>& fit) const {
        if (tokens.empty() || styles.size() != tokens.size()) throw std::invalid_argument("infer_requests: one style row per chunk");
        const int B = (int)tokens.size(), R = (int)chunks_per_request.size();
        size_t stride = 1;
        for (const auto& t : tokens) stride = t.size() > stride ? t.size() : stride;
        std::vector<int64_t> ids((size_t)B * stride, 0);
        std::vector<int32_t> tl(B);
        std::vector<float> st((size_t)B * KX_STYLE_DIM);
        for (int b = 0; b < B; ++b) {
            tl[b] = (int32_t)tokens[b].size();
            for (size_t i = 0; i < tokens[b].size(); ++i) ids[(size_t)b * stride + i] = tokens[b][i];
            if (styles[b].size() != KX_STYLE_DIM) throw std::invalid_argument("infer_requests: style rows need 256 floats");
            for (int k = 0; k < KX_STYLE_DIM; ++k) st[(size_t)b * KX_STYLE_DIM + k] = styles[b][k];
        }
        std::vector<kx_fit_span> sp(spans.size());
        for (size_t i = 0; i < spans.size(); ++i) sp[i] = kx_fit_span{spans[i].request, spans[i].begin, spans[i].end, spans[i].frames};
        std::vector<kx_fit_result> fr(spans.size() ? spans.size() : 1);
        void* out = nullptr;
        std::vector<int64_t> nb(R > 0 ? R : 1), ns(R > 0 ? R : 1);
        const int32_t fmt = format;
        const int rc = kx_infer_requests_fitted(h_, ids.data(), (int64_t)stride, tl.data(), B, chunks_per_request.data(), R, st.data(),
                                                nullptr, nullptr, 0, &speed, 1, seed, 0, &fmt, 1, &out, nb.data(), ns.data(), nullptr,
                                                nullptr, nullptr, 0, nullptr, nullptr, nullptr, sp.empty() ? nullptr : sp.data(),
                                                (int)sp.size(), fr.data());
        if (rc != KX_OK) {
            char msg[512];
            kx_last_error_copy(h_, msg, sizeof(msg));
            throw std::runtime_error(std::string("kokorox_hip error: ") + msg);
        }
        fit.clear();
        for (size_t i = 0; i < spans.size(); ++i) fit.push_back(FitResult{fr[i].lambda, fr[i].n_free, fr[i].held_frames, fr[i].excess});
        std::vector<std::string> bodies;
        const char* p = static_cast<const char*>(out);
        for (int r = 0; r < R; ++r) {
            bodies.emplace_back(p, p + nb[r]);
            p += nb[r];
        }
        kx_free_packed(out);
        return bodies;
    }

    // infer_requests with the integrated loudness of every request measured, and set, on the GPU (kx_infer_requests_loudness;
    // "loudness" in kokorox_hip.h): one spec for every request, no joins, no marks.  loudness[r] = {f64(p), g, I, n_g} of request r.
    std::vector<std::string> infer_requests_loudness(const std::vector<std::vector<int64_t>>& tokens,
                                                     const std::vector<int32_t>& chunks_per_request,
                                                     const std::vector<std::vector<float>>& styles, float speed, uint64_t seed,
                                                     int format, const KxLoudness& spec, std::vector<LoudnessResult>& loudness) const {
        if (tokens.empty() || styles.size() != tokens.size()) throw std::invalid_argument("infer_requests: one style row per chunk");
        const int B = (int)tokens.size(), R = (int)chunks_per_request.size();
        size_t stride = 1;
        for (const auto& t : tokens) stride = t.size() > stride ? t.size() : stride;
        std::vector<int64_t> ids((size_t)B * stride, 0);
        std::vector<int32_t> tl(B);
        std::vector<float> st((size_t)B * KX_STYLE_DIM);
        for (int b = 0; b < B; ++b) {
            tl[b] = (int32_t)tokens[b].size();
            for (size_t i = 0; i < tokens[b].size(); ++i) ids[(size_t)b * stride + i] = tokens[b][i];
            if (styles[b].size() != KX_STYLE_DIM) throw std::invalid_argument("infer_requests: style rows need 256 floats");
            for (int k = 0; k < KX_STYLE_DIM; ++k) st[(size_t)b * KX_STYLE_DIM + k] = styles[b][k];
        }
        void* out = nullptr;
        std::vector<int64_t> nb(R > 0 ? R : 1), ns(R > 0 ? R : 1);
        std::vector<double> ld((size_t)4 * (R > 0 ? R : 1));
        const int32_t fmt = format;
        const int rc = kx_infer_requests_loudness(h_, ids.data(), (int64_t)stride, tl.data(), B, chunks_per_request.data(), R, st.data(),
                                                  nullptr, nullptr, 0, &speed, 1, seed, 0, &fmt, 1, &out, nb.data(), ns.data(), nullptr,
                                                  nullptr, nullptr, 0, &spec, 1, ld.data());
        if (rc != KX_OK) {
            char msg[512];
            kx_last_error_copy(h_, msg, sizeof(msg));
            throw std::runtime_error(std::string("kokorox_hip error: ") + msg);
        }
        std::vector<std::string> bodies;
        loudness.clear();
        const char* p = static_cast<const char*>(out);
        for (int r = 0; r < R; ++r) {
            bodies.emplace_back(p, p + nb[r]);
            p += nb[r];
            loudness.push_back(LoudnessResult{ld[(size_t)4 * r], ld[(size_t)4 * r + 1], ld[(size_t)4 * r + 2], ld[(size_t)4 * r + 3]});
        }
        kx_free_packed(out);
        return bodies;
    }

  private:
    explicit HipKoko(kx_model* adopted) : h_(adopted) {}
    kx_model* h_ = nullptr;
};

// A request of 1 .. max_batch chunks through a dispatcher (kx_dispatcher_submit_request): ids = the chunks back to back, each
// with its own two 0 pads, styles = one 256-float row per chunk; returns the body in the given format word (a KX_PACK_* form, optionally | a rate).
inline std::string submit_request(kx_dispatcher* d, const std::vector<std::vector<int64_t>>& chunks,
                                  const std::vector<float>& styles, float speed, uint64_t seed, int format) {
    std::vector<int64_t> ids;
    std::vector<int32_t> lens;
    for (const auto& c : chunks) {
        ids.insert(ids.end(), c.begin(), c.end());
        lens.push_back((int32_t)c.size());
    }
    if (styles.size() != chunks.size() * KX_STYLE_DIM) throw std::invalid_argument("submit_request: one style row per chunk");
    void* out = nullptr;
    int64_t nb = 0, ns = 0;
    char err[256] = {0};
    if (kx_dispatcher_submit_request(d, ids.data(), lens.data(), (int)lens.size(), styles.data(), nullptr, nullptr, 0, speed, seed,
                                     format, &out, &nb, &ns, err, sizeof(err)) != KX_OK)
        throw std::runtime_error(std::string("kokorox_hip error: ") + err);
    std::string body(static_cast<const char*>(out), (size_t)nb);
    kx_free_packed(out);
    return body;
}

// ... and with the request's token marks (kx_dispatcher_submit_request_marks)
inline std::string submit_request_marks(kx_dispatcher* d, const std::vector<std::vector<int64_t>>& chunks,
                                        const std::vector<float>& styles, float speed, uint64_t seed, int format,
                                        std::vector<int64_t>& marks) {
    std::vector<int64_t> ids;
    std::vector<int32_t> lens;
    for (const auto& c : chunks) {
        ids.insert(ids.end(), c.begin(), c.end());
        lens.push_back((int32_t)c.size());
    }
    if (styles.size() != chunks.size() * KX_STYLE_DIM) throw std::invalid_argument("submit_request: one style row per chunk");
    void* out = nullptr;
    int64_t* mk = nullptr;
    int64_t nb = 0, ns = 0, nm = 0;
    char err[256] = {0};
    if (kx_dispatcher_submit_request_marks(d, ids.data(), lens.data(), (int)lens.size(), styles.data(), nullptr, nullptr, 0, speed,
                                           seed, format, &out, &nb, &ns, &mk, &nm, err, sizeof(err)) != KX_OK)
        throw std::runtime_error(std::string("kokorox_hip error: ") + err);
    std::string body(static_cast<const char*>(out), (size_t)nb);
    marks.assign(mk, mk + nm);  // (inside the allocation of `out`: copied before it is released)
    kx_free_packed(out);
    return body;
}

// ... and with the request's loudness spec (kx_dispatcher_submit_request_loudness; no join, no marks)
inline std::string submit_request_loudness(kx_dispatcher* d, const std::vector<std::vector<int64_t>>& chunks,
                                           const std::vector<float>& styles, float speed, uint64_t seed, int format,
                                           const KxLoudness& spec, LoudnessResult& loudness) {
    std::vector<int64_t> ids;
    std::vector<int32_t> lens;
    for (const auto& c : chunks) {
        ids.insert(ids.end(), c.begin(), c.end());
        lens.push_back((int32_t)c.size());
    }
    if (styles.size() != chunks.size() * KX_STYLE_DIM) throw std::invalid_argument("submit_request: one style row per chunk");
    void* out = nullptr;
    int64_t nb = 0, ns = 0;
    double ld[4] = {0.0, 1.0, 0.0, 0.0};
    char err[256] = {0};
    if (kx_dispatcher_submit_request_loudness(d, ids.data(), lens.data(), (int)lens.size(), styles.data(), nullptr, nullptr, 0, speed,
                                              seed, format, &out, &nb, &ns, nullptr, nullptr, nullptr, &spec, ld, err, sizeof(err)) != KX_OK)
        throw std::runtime_error(std::string("kokorox_hip error: ") + err);
    std::string body(static_cast<const char*>(out), (size_t)nb);
    loudness = LoudnessResult{ld[0], ld[1], ld[2], ld[3]};
    kx_free_packed(out);
    return body;
}

}  // namespace kokorox
