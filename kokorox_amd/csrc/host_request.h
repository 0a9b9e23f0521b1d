// What a call is refused for before it touches the device, and where its output bytes go: the argument checks of the two
// inference entries (Model::infer_host_once, Model::infer_device) and the layout of the compact output.  Plain C++17, no HIP
// header: built with g++ and the sanitizers by the CPU suite (tests/cpp/host_request_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "kx_error.h"

namespace kx {

// general host entry behind kx_infer / kx_infer_voices / kx_infer_packed / kx_infer_requests (Model::infer_host_ex)
struct HostCall {
    const float* styles = nullptr;       // host [B][256], or
    const int32_t* voice_ids = nullptr;  // host [B][max_mix] into the device voice table
    const float* weights = nullptr;      // host [B][max_mix]
    int max_mix = 0;
    const uint64_t* utt_seeds = nullptr;
    int format = 0;                      // 0 f32 mono, 1 f32 stereo, 2 pcm16 mono
    // per-utterance forms (the dispatcher's mixed batches); null = the batch-wide fields above
    const int32_t* kinds = nullptr;      // host [B]: 0 = row of `styles`, 1 = single voice (copy), 2 = mix
    const int32_t* formats = nullptr;    // host [B]
    // requests of several chunks (kx_infer_requests, the dispatcher): rows are chunks, request r owns chunks_per_request[r]
    // consecutive rows and comes out as ONE region (header of its form, then its rows' samples with nothing between them);
    // out_bytes / out_samples of the call then have n_requests entries and `format` / `formats` are not used
    const int32_t* chunks_per_request = nullptr;  // host [n_requests], every entry >= 1, sum = B
    int n_requests = 0;
    const int32_t* req_formats = nullptr;         // host [n_req_formats], values 0..4 (KX_PACK_*)
    int n_req_formats = 0;                        // 1 (shared) or n_requests
    const uint32_t* utt_index = nullptr;          // host [B] beside utt_seeds: row b draws (utt_seeds[b], utt_index[b])

    bool grouped() const { return chunks_per_request != nullptr; }
    bool by_voice() const { return voice_ids != nullptr; }
    int kind_of(int b) const { return kinds ? kinds[b] : (by_voice() ? (max_mix == 1 ? 1 : 2) : 0); }
    int format_of(int b) const { return formats ? formats[b] : format; }
};

// ---- the refusals, side by side.  The two entries word some of them differently (a row longer than the stride, for one):
// each keeps its own text; callers and tests match on them. ----------------------------------------------------------------
// Everything Model::infer_host_once refuses before its first device call, in its order of precedence; *out is cleared once
// the output arguments are known to be there.
void check_host_call(const int64_t* ids, int64_t t_stride, const int32_t* lens, int B, const float* speeds, const HostCall& hc,
                     void** out, const int64_t* out_bytes, const int64_t* out_samples, int n_vocab, int n_voices,
                     bool have_voice_table);
// Everything Model::infer_device refuses before hipSetDevice; returns the longest token count.
int check_device_call(const void* d_ids, int64_t t_stride, const int32_t* lens_host, int B, const void* d_styles,
                      const float* speeds_host, int n_speed);

// ---- the compact output ---------------------------------------------------------------------------------------------------
inline int format_sample_bytes(int form) { return form == 1 ? 8 : (form == 2 ? 2 : 4); }  // forms 0..2

// Utterances back to back, each in its own form 0..2 (`formats` [B], or null: `format` for all)
struct UttLayout {
    std::vector<int> sample_bytes;    // [B]
    std::vector<int64_t> samples;     // [B] 600 x frames
    std::vector<int64_t> bytes;       // [B]
    std::vector<long> off;            // [B] bytes before utterance b
    int64_t total_bytes = 0;
};
void utt_layout(const int* frames, int B, int format, const int* formats, UttLayout& out);

// ---- requests of several chunks, packed as the bytes a server sends (kernels_misc.hip: pack_requests_kernel) ----------
// A request is n_rows consecutive rows of the audio slab; its output is a function of a virtual byte stream: the header of
// its form (if any), then the sample bytes of its rows in order with nothing between them.  Forms 0..2 as launch_pack_audio,
// 3 = 44-byte float WAV header + f32 bit copies, 4 = base64 of a 16-bit WAV file (include/kokorox_hip.h, KX_PACK_*).
struct PackReq {
    int first_row, n_rows, form, pad_;
    long out_off;    // byte offset of the request's region in the compact output (a multiple of 4)
    long out_bytes;  // size of the region (a multiple of 4 in every form)
    long n_samples;  // 600 * the sum of its rows' frames
};
struct PackPlan {
    std::vector<PackReq> req;
    std::vector<long> cum;  // [B + 1] samples of the rows before row b, over the whole batch
    long total_bytes = 0;
    long max_units = 0;     // 16-byte units of the largest region (the launch's grid)
};
long pack_request_bytes(int form, long n_samples);  // throws KX_ERR_INVALID: unknown form, 16-bit WAV past 4 GiB
// Worst case of a batch's compact output before the frame counts are known: R requests, n_samples samples in all, every
// request in the widest of the given forms (the per-request header and the base64 padding do not scale with the samples).
size_t pack_requests_bound(const int* formats, int n_format, int R, size_t n_samples);
// chunks_per_request [R] (null: every row a request of its own, R = B), formats [n_format], n_format = 1 or R
void build_pack_plan(const int* frames, int B, const int* chunks_per_request, int R, const int* formats, int n_format,
                     PackPlan& plan);

// Bytes of the packed buffer of a call of B rows before its forward has run, for n_samples samples in all: the requests' bound
// when the call is grouped, else every sample in the widest form of the batch.
size_t packed_bytes_bound(const HostCall& hc, int B, size_t n_samples);

}  // namespace kx
