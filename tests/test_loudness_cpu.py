"""CPU: loudness -- BS.1770 metering and LUFS normalisation of a request (include/kokorox_hip.h, "loudness").

Layers that need no GPU: the committed K-weighting table against its generator and against the standard's published 48 kHz
coefficients; the numpy definition (kokorox_amd/voices.py: kweight, hop_energies, gated_loudness, integrated_loudness,
loudness_gain, loudness_body) against the 997 Hz anchor of EBU Tech 3341 and against answers worked out by hand
(tests/golden/loudness.json); the host layout (kokorox_amd/csrc/host_request.cpp: build_output_plan with loudness, output_bounds,
check_spec_list, the meter's tables) and the dispatcher's submit-time checks, built with g++ -fsanitize=address,undefined into
tests/cpp/loudness_plan_check.cpp and run as a child process; and the ABI (header, Python table, C++ wrapper, lib.rs).
"""
import json
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from kokorox_amd import voices as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "loudness.json"), encoding="utf-8"))
RATES = {0: 24000, 1: 8000, 2: 16000, 3: 48000}
LM = {0: (1, 1), 1: (1, 3), 2: (2, 3), 3: (2, 1)}
MEASURE, NORMALIZE, NONE = 0, 1, 0xFFFFFFFF
WARMUP = {0: 4096, 1: 1536, 2: 3072, 3: 8192}  # host_request.h: loud_warmup
WINDOW = 4096                                   # host_request.h: LEVEL_WINDOW


# ---- the table -------------------------------------------------------------------------------------------------------------
def test_committed_table_is_what_the_generator_gives():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_kweight_coefs.py"), "--check"])
    assert r.returncode == 0, "kokorox_amd/csrc/kweight_coefs.h differs from tools/gen_kweight_coefs.py"


def test_library_hands_out_the_committed_bits_and_refuses_unknown_words():
    from kokorox_amd import hip_koko as hk
    text = open(os.path.join(ROOT, "kokorox_amd", "csrc", "kweight_coefs.h"), encoding="utf-8").read()
    for code, hz in RATES.items():
        m = re.search(r"#define KX_KWEIGHT_COEFS_%d \\\n((?:.*\\\n)*.*)\n" % hz, text)
        bits = [int(b, 16) for b in re.findall(r"0x([0-9A-F]{16})ull", m.group(1))]
        assert len(bits) == 10
        want = np.array(bits, dtype=np.uint64).view(np.float64)
        for form in (0, 4, 9):
            assert hk.loudness_filter(form | code << 8).tobytes() == want.tobytes()
        assert V.kweight_coefs(hz).tobytes() == want.tobytes()
    for word in (5, 0x400, -1, 0x1000):
        with pytest.raises(hk.KokoroxHipError):
            hk.loudness_filter(word)
    with pytest.raises(ValueError):
        V.kweight_coefs(44100)


def test_the_48_khz_row_is_the_standards_published_coefficients():
    c = V.kweight_coefs(48000)
    published = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, -1.99004745483398, 0.99007225036621]
    assert np.abs(c[[0, 1, 2, 3, 4, 8, 9]] - np.array(published)).max() <= 1e-12
    assert c[5:8].tolist() == [1.0, -2.0, 1.0]


@pytest.mark.parametrize("code", [0, 1, 2, 3], ids=["24000", "8000", "16000", "48000"])
def test_warm_up_covers_the_impulse_response_and_sum_h_is_below_3_35(code):
    """The tail of sum |h| of the cascade beyond the kernel's warm-up is below 1e-15, and sum |h| itself at most 3.35: what the
    tolerances of tests/test_gpu_loudness.py are derived from."""
    x = np.zeros(3 * WARMUP[code], dtype=np.float32)
    x[0] = 1.0
    h = np.abs(V.kweight(x, RATES[code]))
    assert h.sum() <= 3.35 and h[WARMUP[code]:].sum() < 1e-15


# ---- the numpy definition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [0, 1, 2, 3], ids=["24000", "8000", "16000", "48000"])
def test_a_997_hz_sine_measures_its_level_minus_3_01_within_the_meter_tolerance(code):
    """EBU Tech 3341: a 997 Hz sine of amplitude A reads 20 log10(A) - 3.0103 LUFS within +-0.1 LU."""
    rate = RATES[code]
    n = np.arange(3 * rate)
    for A in (1.0, 0.1):
        z = (A * np.sin(2 * np.pi * 997.0 * n / rate)).astype(np.float32)
        I, n_g, margin = V.integrated_loudness(z, rate)
        print(f"{rate} Hz, A = {A}: I = {I}, deviation {I - (20 * np.log10(A) - 3.0103):+.5f} LU")
        assert abs(I - (20 * np.log10(A) - 3.0103)) <= 0.1 and n_g == 27 and margin > 1.0


@pytest.mark.parametrize("case", GOLDEN["gating"], ids=[c["name"] for c in GOLDEN["gating"]])
def test_gating_gives_the_hand_derived_answers(case):
    I, n_g, margin = V.gated_loudness(case["e"], 10 * case["hop"])
    assert n_g == case["n_g"] and margin >= 1e-6
    if case["I"] is None:
        assert np.isnan(I)
    else:
        assert abs(I - case["I"]) <= 1e-12


@pytest.mark.parametrize("case", GOLDEN["gain"], ids=[c["name"] for c in GOLDEN["gain"]])
def test_gain_gives_the_hand_derived_answers(case):
    mode, target, peak = case["spec"]
    g = V.loudness_gain(np.float32(float(case["p"])), float(case["I"]), (mode, float(target), float(peak)))
    assert isinstance(g, float) and abs(g - case["g"]) <= 1e-15 * case["g"]


def test_the_definition_on_a_stream():
    rng = np.random.default_rng(5)
    z = rng.uniform(-0.5, 0.5, 8000 + 333).astype(np.float32)  # ten hops at 8 kHz and a partial one
    e = V.hop_energies(z, 8000)
    assert e.shape == (10,) and e.tobytes() == V.hop_energies(z[:8000], 8000).tobytes()  # the partial hop is ignored, and causal
    I, n_g, margin = V.integrated_loudness(z, 8000)
    assert n_g == 7 and (I, n_g, margin) == V.gated_loudness(e, 8000)
    # non-finite samples are zeros to the meter
    bad = z.copy()
    bad[[3, 900, 7999]] = [np.nan, np.inf, -np.inf]
    zeroed = z.copy()
    zeroed[[3, 900, 7999]] = 0.0
    assert V.hop_energies(bad, 8000).tobytes() == V.hop_energies(zeroed, 8000).tobytes()
    # a gain of 10^(d / 20) moves I by d, and loudness_body is level_stream's product
    g = V.loudness_gain(np.abs(z).max(), I, (NORMALIZE, -23.0, 1.0))
    out = np.frombuffer(V.loudness_body(z, g, 0), dtype="<f4")
    assert out.tobytes() == (np.float64(g) * z.astype(np.float64)).astype(np.float32).tobytes()
    assert abs(V.integrated_loudness(out, 8000)[0] - -23.0) < 1e-6
    assert np.isnan(np.frombuffer(V.loudness_body(bad, g, 0), dtype="<f4")[3])
    short = V.integrated_loudness(z[:2399], 8000)  # two hops and a partial one: no block
    assert np.isnan(short[0]) and short[1:] == (0, float("inf"))


BAD_SPECS = [(2, -23.0, 1.0), (-1, -23.0, 1.0), (1, 1.0, 1.0), (1, -71.0, 1.0), (1, -23.0, 2.0), (1, -23.0, 2.0 ** -16), (1, -23.0, 0.0),
             (0, -23.0, 0.0), (0, 0.0, 0.5), (0, -0.0, 0.0), (1, float("nan"), 1.0), (1, -23.0, float("nan")), (1.5, -23.0, 1.0), (True, -23.0, 1.0)]


def test_mirror_refuses_every_invalid_spec():
    for bad in BAD_SPECS:
        with pytest.raises(ValueError):
            V.loudness_gain(np.float32(0.5), -20.0, bad)
    for ok in ((0, 0.0, 0.0), (1, 0.0, 1.0), (1, -70.0, 2.0 ** -15), None):
        V.loudness_gain(np.float32(0.5), -20.0, ok)


# ---- the host layout (HIP-free, under the sanitizers) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("loudness_plan") / "loudness_plan_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "loudness_plan_check.cpp"), os.path.join(csrc, "host_request.cpp"),
                    "-lpthread", "-o", exe], check=True)

    def run(mode, text=""):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, mode], env=env, input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _bytes_of(word, n):
    return {0: 4 * n, 1: 8 * n, 2: 2 * n, 3: 44 + 4 * n, 4: 4 * ((44 + 2 * n + 2) // 3), 8: n, 9: n}[word & 0xFF]


SPEC_CHOICES = [(MEASURE, 0.0, 0.0), (NORMALIZE, -23.0, 1.0), (NORMALIZE, -16.0, 0.5), (NONE, 0.0, 0.0)]


def test_plan_builder_on_150_random_plans(driver):
    """Rows of 1..60 frames grouped into requests, mixed words, one shared spec or one per request, requests that are not metered
    among them.  The levels block sits where a levelled plan has it, the loudness block right behind it, 16 R bytes each;
    end_bytes is its end; the hop table has R rows of the most hops a metered request has; the bounds hold and the packed bound
    grows by 8 + 32 R.  (The driver itself compares every plan with the one of the same layout without loudness.)"""
    rng = np.random.default_rng(20261021)
    forms, cases, text = (0, 1, 2, 3, 4, 8, 9), {}, ""
    for i in range(150):
        B = int(rng.integers(1, 7))
        frames = [int(rng.integers(1, 61)) for _ in range(B)]
        cpr = []
        while sum(cpr) < B:
            cpr.append(int(rng.integers(1, B - sum(cpr) + 1)))
        R = len(cpr)
        words = [int(rng.choice(forms)) | int(rng.integers(0, 4)) << 8 for _ in range(R)]
        specs = [SPEC_CHOICES[int(rng.integers(0, 3 if i % 4 == 1 else 4))] for _ in range(1 if i % 4 == 1 else R)]
        cases[f"c{i}"] = (frames, cpr, words, specs)
        flat = [f"c{i}", B, R] + frames + cpr + words + [len(specs)] + [v for m, t, p in specs for v in (m, _bits(t), _bits(p))]
        text += " ".join(str(v) for v in flat) + "\n"
    out = driver("plans", text)
    got, cur = {}, None
    for line in out.splitlines():
        kind, *rest = line.split()
        if kind == "case":
            cur = got.setdefault(rest[0], {"req": []})
        elif kind == "req":
            cur["req"].append([int(v) for v in rest[1:]])
        elif kind in ("sizes", "bounds"):
            cur[kind] = [int(v) for v in rest]
        else:
            assert kind == "done" and rest == ["150"], line
    seen_hops, seen_none, seen_all = set(), 0, 0
    for name, (frames, cpr, words, specs) in cases.items():
        g, R = got[name], len(cpr)
        row, off, longest, hops = 0, 0, 0, 0
        for r, n in enumerate(cpr):
            L, M = LM[words[r] >> 8]
            n_out = 600 * sum(frames[row: row + n]) * L // M
            mode, target, peak = specs[r if len(specs) > 1 else 0]
            assert g["req"][r] == [off, _bytes_of(words[r], n_out), n_out, mode, _bits(target), _bits(peak), 1 if mode == NONE else 0], (name, r)
            off += _bytes_of(words[r], n_out)
            longest = max(longest, n_out)
            hops = max(hops, n_out // (RATES[words[r] >> 8] // 10)) if mode != NONE else hops
            row += n
        modes = [specs[r if len(specs) > 1 else 0][0] for r in range(R)]
        total, marks_off, levels_off, loud_off, end, measured, levelled, loud_all, max_hops, hop_doubles, windows = g["sizes"]
        assert (total, marks_off) == (off, (off + 7) & ~7) and levels_off == marks_off and loud_off == levels_off + 16 * R and end == loud_off + 16 * R
        assert measured == 1 and levelled == int(NORMALIZE in modes) and loud_all == int(NONE not in modes)
        assert max_hops == hops and hop_doubles == R * hops and windows == -(-longest // WINDOW)
        packed, hop_bound, peak_bound, packed_without = g["bounds"]
        assert packed >= end and hop_bound >= hop_doubles and peak_bound >= R * windows and packed == packed_without + 8 + 32 * R, name
        seen_hops.add(max_hops)
        seen_none += NONE in modes
        seen_all += bool(loud_all)
    assert len(seen_hops) >= 10 and seen_none >= 20 and seen_all >= 20


def test_refusals_of_the_loudness_arguments(driver):
    got = dict(line.split("\t", 1) for line in driver("refusals").splitlines())
    bad = "1\tinfer: bad loudness"
    names = ["mode_2", "mode_stray_bit", "mode_none", "target_plus_1", "target_minus_71", "peak_2", "peak_small", "peak_0", "mode0_target_set",
             "mode0_peak_set", "mode0_target_minus_0", "target_nan", "peak_nan", "mode0_target_nan", "third_of_three_bad"]
    want = {n: bad for n in names}
    want.update({"null_loudness": "1\tinfer: null loudness argument", "n_loudness_0": "1\tinfer: bad loudness count",
                 "n_loudness_2_of_3": "1\tinfer: bad loudness count", "n_loudness_minus_1": "1\tinfer: bad loudness count",
                 "ok_shared": "accepted", "ok_per_request": "accepted"})
    assert got == want


def test_dispatcher_checks_the_spec_at_submit_and_carries_it_to_the_batch(driver):
    got = dict(line.split("\t", 1) for line in driver("dispatcher").splitlines())
    bad = "1\tdispatcher_submit_request: bad loudness"
    target, half = _bits(-23.0), _bits(0.5)
    assert got == {
        "null_loudness": bad, "mode_2": bad, "target_plus_1": bad, "peak_2": bad, "mode0_target_set": bad, "target_nan": bad, "mode_none": bad,
        "mode_stray_bit": bad, "target_minus_71": bad, "peak_nan": bad,
        "bad_join": "1\tdispatcher_submit_request: bad join",
        "ok_no_join": f"accepted\t1 {target:#x} {half:#x} metered=1 levelled=0 joined=0 pause=0 out=0.25 3 -23.5 7",
        "ok_join": f"accepted\t1 {target:#x} {half:#x} metered=1 levelled=0 joined=1 pause=85 out=0.25 3 -23.5 7",
        "ok_meter_no_out": "accepted\t0 0 0 metered=1 levelled=0 joined=0 pause=0 out=-1 -1 -1 -1",
    }


def test_the_meters_grid_and_transition_powers(driver):
    lines = driver("tables").splitlines()
    assert len(lines) == 4
    for code, line in enumerate(lines):
        f = line.split()
        run, warmup, hop = int(f[3]), int(f[5]), int(f[7])
        assert (int(f[1]), warmup, hop) == (code, WARMUP[code], RATES[code] // 10) and run % 2 == 1
        assert 4 * (warmup + hop) <= 64 * 1024 - 4096  # the staged window leaves room in a workgroup's 64 KB of LDS


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_part_of_the_abi():
    from kokorox_amd import hip_koko as hk
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    test_header = open(os.path.join(ROOT, "include", "kokorox_hip_test.h"), encoding="utf-8").read()
    for name in ("kx_infer_requests_loudness", "kx_dispatcher_submit_request_loudness", "kx_loudness_filter"):
        assert name in hk.ABI_SYMBOLS and re.search(r"^int %s\(" % name, header, re.M), name
        assert name not in test_header
    assert "kx_test_output_plan_loudness" in hk.TEST_ABI_SYMBOLS and "kx_test_output_plan_loudness" not in hk.ABI_SYMBOLS
    assert re.search(r"^int kx_test_output_plan_loudness\(", test_header, re.M) and "kx_test_output_plan_loudness" not in header
    for text in ("infer: null loudness argument", "infer: bad loudness count", "infer: bad loudness", "dispatcher_submit_request: bad loudness"):
        assert '"%s"' % text in header, text
    assert (hk.LOUDNESS_MEASURE, hk.LOUDNESS_NORMALIZE) == (0, 1) == (V.LOUDNESS_MEASURE, V.LOUDNESS_NORMALIZE)
    for name, value in (("KX_LOUDNESS_MEASURE", 0), ("KX_LOUDNESS_NORMALIZE", 1)):
        assert re.search(r"^#define %s\s+%du\b" % (name, value), header, re.M), name
    assert "typedef struct kx_loudness { uint32_t mode; float target_lufs; float peak; } kx_loudness;" in header
    assert hk.LOUDNESS_DTYPE.itemsize == 12 and list(hk.LOUDNESS_DTYPE.names) == ["mode", "target_lufs", "peak"]
    assert hk.LOUDNESS_METER == (0, 0.0, 0.0) == V.LOUDNESS_METER
    ld = hk.loudness_specs((1, -23.0, 0.5), 3)
    assert ld.shape == (3,) and ld.tobytes() == struct.pack("<Iff", 1, -23.0, 0.5) * 3
    with pytest.raises(ValueError):
        hk.loudness_specs([(0, 0.0, 0.0)], 2)
    assert callable(hk.HipKoko.infer_requests_loudness) and callable(hk.loudness_requests)
    # (the struct is 12 bytes for a C compiler as well)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], text=True, capture_output=True,
                       input='#include "kokorox_hip.h"\n#include <cstddef>\nstatic_assert(sizeof(kx_loudness) == 12 && offsetof(kx_loudness, target_lufs) == 4 && '
                             'offsetof(kx_loudness, peak) == 8, "kx_loudness");\n')
    assert r.returncode == 0, r.stderr


def test_cpp_wrapper_and_rust_crate_bind_the_struct_and_both_entries():
    hpp = open(os.path.join(ROOT, "include", "kokorox_hip.hpp"), encoding="utf-8").read()
    for name in ("infer_requests_loudness", "submit_request_loudness", "kx_infer_requests_loudness", "kx_dispatcher_submit_request_loudness"):
        assert re.search(r"\b%s\s*\(" % name, hpp), name
    assert re.search(r"using KxLoudness = kx_loudness;", hpp)
    rs = open(os.path.join(ROOT, "kokorox-hip", "src", "lib.rs"), encoding="utf-8").read()
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct KxLoudness \{(.*?)\}", rs, flags=re.S)
    assert m, "lib.rs lacks a #[repr(C)] KxLoudness"
    assert re.findall(r"pub (\w+): (\w+)", m.group(1)) == [("mode", "u32"), ("target_lufs", "f32"), ("peak", "f32")]
    for name in ("kx_infer_requests_loudness", "kx_dispatcher_submit_request_loudness", "kx_loudness_filter", "infer_requests_loudness",
                 "submit_request_loudness"):
        assert re.search(r"\bfn %s\s*[(<]" % name, rs), name
    for name, value in (("KX_LOUDNESS_MEASURE", 0), ("KX_LOUDNESS_NORMALIZE", 1)):
        assert re.search(r"pub const %s: u32 = %d;" % (name, value), rs), name
