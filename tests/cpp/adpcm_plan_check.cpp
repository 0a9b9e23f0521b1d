// CPU driver of the ADPCM WAV and 16-bit WAV forms in the host layout (kokorox_amd/csrc/host_request.cpp: check_format_word,
// pack_request_bytes, adpcm_block_bytes, adpcm_steps, build_output_plan, output_bounds): built with g++ -fsanitize=address,undefined
// together with host_request.cpp by tests/test_adpcm_cpu.py and run as a child process.
//
//   adpcm_plan_check table             "block <rate code> <A> <P>" for the four rate codes, then "steps" and the 89 steps
//   adpcm_plan_check sizes < pairs     per "word n" of the input (n = samples at 24 000 Hz): "<word> <n> <bytes>" or
//                                      "<word> <n> refused <message>"
//   adpcm_plan_check plans < cases     every case "name B R", frames [B], chunks_per_request [R], words [R], printed as
//       case <name>
//       req <r> <form> <rate> <out_off> <out_bytes> <n_samples>
//       sizes <total_bytes> <max_units> <adpcm_groups> <packed bytes of output_bounds>
//     (it judges itself, in every case: the regions lie back to back from 0, every size is a multiple of 4 and the formula's, the
//     packer's grid counts no form-17 region, the encoder's grid is that of the request with most blocks, and output_bounds covers
//     what the plan needs)
//   adpcm_plan_check refusals          one line per case: <name> TAB <code> TAB <message>, or <name> TAB accepted
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_request.h"

namespace {

#define REQUIRE_SAME(cond)                                                      \
    do {                                                                        \
        if (!(cond)) {                                                          \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

const long kBlock[4] = {512, 256, 512, 1024};  // by rate code, written out again: 24 000, 8000, 16 000, 48 000 Hz

bool read_longs(std::vector<long>& v, size_t n) {
    v.assign(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (scanf("%ld", &v[i]) != 1) return false;
    return true;
}

long want_bytes(int form, int rate, long n) {
    const long A = kBlock[rate], P = 2 * A - 7;
    if (form == kx::FORM_ADPCM_WAV) return 60 + A * ((n + P - 1) / P);
    if (form == kx::FORM_WAV16) return (44 + 2 * n + 3) / 4 * 4;
    return -1;
}

bool run_plan_case() {
    char name[64];
    int B, R;
    if (scanf("%63s %d %d", name, &B, &R) != 3) return false;
    std::vector<long> fr, cp, wd;
    if (!read_longs(fr, (size_t)B) || !read_longs(cp, (size_t)R) || !read_longs(wd, (size_t)R)) return false;
    std::vector<int> frames(fr.begin(), fr.end()), cpr(cp.begin(), cp.end()), words(wd.begin(), wd.end());
    kx::RequestLayout lay{};
    lay.chunks_per_request = cpr.data(), lay.R = R, lay.formats = words.data(), lay.n_format = R;
    kx::OutputPlan plan;
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, lay, plan);
    printf("case %s\n", name);
    long off = 0, units = 0, groups = 0;
    for (int r = 0; r < R; ++r) {
        const kx::PackReq& q = plan.req[(size_t)r];
        REQUIRE_SAME(q.out_off == off && q.out_bytes % 4 == 0 && q.form == kx::format_form(words[(size_t)r]) && q.rate == kx::format_rate(words[(size_t)r]));
        const long want = want_bytes(q.form, q.rate, q.n_samples);
        REQUIRE_SAME(want < 0 || q.out_bytes == want);
        REQUIRE_SAME(q.out_bytes == kx::pack_request_bytes(words[(size_t)r], q.src_samples));
        if (q.form == kx::FORM_ADPCM_WAV) {
            const long A = kBlock[q.rate], F = (q.out_bytes - 60) / A, per = 8192 / A, g = (F + per - 1) / per;
            REQUIRE_SAME(kx::adpcm_block_bytes(q.rate) == A && kx::adpcm_block_samples(A) == 2 * A - 7 && kx::adpcm_blocks(q.n_samples, A) == F);
            groups = (g > 1 ? g : 1) > groups ? (g > 1 ? g : 1) : groups;
        } else {
            const long u = ((q.out_off & 15) + q.out_bytes + 15) / 16;
            units = u > units ? u : units;
        }
        off += q.out_bytes;
        printf("req %d %d %d %ld %ld %ld\n", r, q.form, q.rate, q.out_off, q.out_bytes, q.n_samples);
    }
    REQUIRE_SAME(plan.total_bytes == off && plan.max_units == units && plan.adpcm_groups == groups && !plan.has_flac());
    long samples = 0;
    for (int b = 0; b < B; ++b) samples += 600L * frames[(size_t)b];
    const kx::OutputBounds bound = kx::output_bounds(lay, B, (size_t)samples, nullptr);
    REQUIRE_SAME((long)bound.packed_bytes >= plan.end_bytes() && bound.flac_slots == 0);
    // a plan object used again for a call without the form forgets the encoder's grid
    std::vector<int> as_pcm = words;
    for (int& w : as_pcm) w = (w & ~0xFF) | 2;
    lay.formats = as_pcm.data();
    kx::build_output_plan(frames.data(), nullptr, nullptr, B, lay, plan);
    REQUIRE_SAME(plan.adpcm_groups == 0);
    printf("sizes %ld %ld %ld %zu\n", off, units, groups, bound.packed_bytes);
    return true;
}

void refusal(const char* name, int word) {
    try {
        kx::check_format_word(word);
        printf("%s\taccepted\n", name);
    } catch (const kx::Error& e) {
        printf("%s\t%d\t%s\n", name, e.code, e.what());
    }
}

void refusals() {
    char name[64];
    for (int form : {5, 6, 7, 10, 11, 13, 14, 15, 16, 19, 20, 32, 128, 255}) {
        snprintf(name, sizeof name, "form_%d", form);
        refusal(name, form);
    }
    for (int form : {kx::FORM_ADPCM_WAV, kx::FORM_WAV16}) {
        for (int rate = 0; rate < 6; ++rate) {
            snprintf(name, sizeof name, "form_%d_rate_%d", form, rate);
            refusal(name, form | (rate << 8));
        }
        snprintf(name, sizeof name, "form_%d_stray_bit", form);
        refusal(name, form | 0x1000);
        snprintf(name, sizeof name, "form_%d_negative", form);
        refusal(name, (int)(0x80000000u | (unsigned)form));
    }
    // the entries that take the forms 0..2 keep refusing both: a call without chunks_per_request
    const int64_t ids[3] = {0, 5, 0};
    const int32_t lens[1] = {3};
    const float speeds[1] = {1.0f};
    std::vector<float> styles(256, 0.0f);
    void* out = nullptr;
    int64_t bytes[1], samples[1];
    for (int format : {2, kx::FORM_ADPCM_WAV, kx::FORM_WAV16, kx::FORM_ADPCM_WAV | 0x100}) {
        kx::HostCall hc;
        hc.styles = styles.data();
        hc.format = format;
        snprintf(name, sizeof name, "per_utterance_format_%d", format);
        try {
            kx::check_host_call(ids, 3, lens, 1, speeds, hc, &out, bytes, samples, 178, 0, false);
            printf("%s\taccepted\n", name);
        } catch (const kx::Error& e) {
            printf("%s\t%d\t%s\n", name, e.code, e.what());
        }
    }
    // the request entry takes them
    for (int word : {kx::FORM_ADPCM_WAV | 0x100, kx::FORM_WAV16 | 0x300}) {
        const int32_t cpr[1] = {1}, words[1] = {word};
        kx::HostCall hc;
        hc.styles = styles.data();
        hc.chunks_per_request = cpr, hc.n_requests = 1, hc.req_formats = words, hc.n_req_formats = 1;
        snprintf(name, sizeof name, "request_format_%d", word);
        try {
            kx::check_host_call(ids, 3, lens, 1, speeds, hc, &out, bytes, samples, 178, 0, false);
            printf("%s\taccepted\n", name);
        } catch (const kx::Error& e) {
            printf("%s\t%d\t%s\n", name, e.code, e.what());
        }
    }
    try {
        kx::adpcm_block_bytes(4);
        printf("block_rate_4\taccepted\n");
    } catch (const kx::Error& e) {
        printf("block_rate_4\t%d\t%s\n", e.code, e.what());
    }
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "table") {
        for (int c = 0; c < 4; ++c) printf("block %d %ld %ld\n", c, kx::adpcm_block_bytes(c), kx::adpcm_block_samples(kx::adpcm_block_bytes(c)));
        printf("steps");
        for (int i = 0; i < 89; ++i) printf(" %d", kx::adpcm_steps()[i]);
        printf("\n");
    } else if (mode == "sizes") {
        long word, n;
        while (scanf("%ld %ld", &word, &n) == 2) {
            try {
                printf("%ld %ld %ld\n", word, n, kx::pack_request_bytes((int)word, n));
            } catch (const kx::Error& e) {
                printf("%ld %ld refused %s\n", word, n, e.what());
            }
        }
    } else if (mode == "plans") {
        while (run_plan_case()) {
        }
    } else if (mode == "refusals") {
        refusals();
    } else {
        fprintf(stderr, "usage: adpcm_plan_check table|sizes|plans|refusals\n");
        return 2;
    }
    return 0;
}
