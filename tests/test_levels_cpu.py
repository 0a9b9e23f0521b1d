"""CPU: levels -- a request's gain, peak normalisation and ceiling (include/kokorox_hip.h, "levels").

Three layers, none of which needs a GPU: the numpy definition (kokorox_amd/voices.py: level_gain, level_stream) against answers
worked out by hand (tests/golden/levels.json) and against exact rational arithmetic; the host layout
(kokorox_amd/csrc/host_request.cpp: build_output_plan with levels, output_bounds, check_spec_list) and the dispatcher's
submit-time checks, built with g++ -fsanitize=address,undefined into tests/cpp/level_plan_check.cpp and run as a child process;
and the ABI (header, Python table, lib.rs).
"""
import json
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from kokorox_amd import voices as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "levels.json"), encoding="utf-8"))["cases"]
LM = {0: (1, 1), 1: (1, 3), 2: (2, 3), 3: (2, 1)}
GAIN, NORMALIZE, CEILING = 0, 1, 2
WINDOW = 4096  # host_request.h: LEVEL_WINDOW


def _f32(strings):
    return np.array([float(s) for s in strings], dtype=np.float64).astype(np.float32)


def _level(case):
    mode, gain, peak = case["level"]
    return int(mode), float(np.float32(float(gain))), float(np.float32(float(peak)))


def _same_floats(got, want):
    """Bit equality, except that a NaN must be a NaN where the answer has one."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    assert got[keep].tobytes() == want[keep].tobytes(), (got, want)


# ---- the numpy definition against the hand-derived answers -------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in GOLDEN if "out" in c], ids=[c["name"] for c in GOLDEN if "out" in c])
def test_mirror_gives_the_hand_derived_answers(case):
    z, level = _f32(case["z"]), _level(case)
    p, g = V.level_gain(z, level)
    assert isinstance(p, np.float32) and isinstance(g, float)
    assert p.tobytes() == np.float32(float(case["p"])).tobytes() and g == float(case["g"])
    out = V.level_stream(z, level)
    assert out.dtype == np.float32
    _same_floats(out, _f32(case["out"]))


def test_the_dyadic_cases_of_the_definition_by_hand():
    z = np.array([0.25, -0.5, 0.125], dtype=np.float32)
    assert V.level_gain(z, (NORMALIZE, 1.0, 1.0)) == (np.float32(0.5), 2.0)
    assert V.level_gain(z, (CEILING, 4.0, 0.75)) == (np.float32(0.5), 1.5)
    assert V.level_gain(z, (CEILING, 1.0, 0.75)) == (np.float32(0.5), 1.0)
    assert V.level_gain(z, (GAIN, 0.0, 0.0)) == (np.float32(0.5), 0.0)
    assert V.level_gain(z, None) == (np.float32(0.5), 1.0) and V.level_stream(z, None).tobytes() == z.tobytes()
    assert V.level_stream(z, V.LEVEL_PLAIN).tobytes() == z.tobytes()


def test_non_dyadic_case_equals_exact_rational_arithmetic():
    """g is the correctly rounded float64 of peak / p, a sample the float32 of the correctly rounded float64 of g z: both
    derived here from fractions, which Python rounds to the nearest float64, ties to even."""
    case = next(c for c in GOLDEN if c["name"] == "non_dyadic")
    z, (mode, gain, peak) = _f32(case["z"]), _level(case)
    assert mode == NORMALIZE and len({float(v) for v in z}) == 4  # (the last sample is the float32 just below the peak)
    p = max(Fraction(float(abs(v))) for v in z)
    g = float(Fraction(peak) / p)                                            # one float64 division
    got_p, got_g = V.level_gain(z, (mode, gain, peak))
    assert Fraction(float(got_p)) == p and got_g == g
    assert g != float(np.float32(g))                                         # (the case is not dyadic: g needs its 53 bits)
    want = [np.float32(float(Fraction(g) * Fraction(float(v)))) for v in z]  # one float64 product, one conversion
    out = V.level_stream(z, (mode, gain, peak))
    assert out.tobytes() == np.array(want, dtype=np.float32).tobytes()
    assert float(np.abs(out).max()) == peak


# ---- properties of the definition ------------------------------------------------------------------------------------------
def test_a_normalised_maximum_is_exactly_peak_on_20000_seeded_pairs():
    """f32((f64(peak) / f64(p)) * f64(p)) == peak, and no other sample of the stream passes it: 24 000 seeded (p, peak) pairs
    over the whole range of both, each with smaller samples beside the peak, the float32 just below it among them."""
    rng = np.random.default_rng(20261019)
    n = 24000
    p = (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-40, 40, n)).astype(np.float32)
    peak = np.clip((rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-15, 0, n)).astype(np.float32), np.float32(2.0 ** -15), np.float32(1.0))
    peak[:100], peak[100:200] = np.float32(1.0), np.float32(2.0 ** -15)
    below = np.nextafter(p, np.float32(0), dtype=np.float32)
    others = (p[:, None].astype(np.float64) * rng.uniform(-1.0, 1.0, (n, 5))).astype(np.float32)
    sign = np.where(rng.random(n) < 0.5, np.float32(-1), np.float32(1))
    z = np.concatenate([others[:, :2], (sign * p)[:, None], -sign[:, None] * below[:, None], others[:, 2:]], axis=1).astype(np.float32)
    g = peak.astype(np.float64) / p.astype(np.float64)
    out = (g[:, None] * z.astype(np.float64)).astype(np.float32)
    assert np.array_equal(np.abs(out).max(axis=1), peak)
    assert np.array_equal(np.abs(out[:, 2]), peak) and (np.abs(out) <= peak[:, None]).all()
    for i in range(0, n, 997):  # ... and the mirror agrees with this vectorised form, in mode 1 and in mode 2 with a gain that is too large
        for level in ((NORMALIZE, 1.0, float(peak[i])), (CEILING, 64.0, float(peak[i]))):
            if level[0] == CEILING and 64.0 * float(p[i]) <= float(peak[i]):
                continue
            got_p, got_g = V.level_gain(z[i], level)
            assert got_p == p[i] and got_g == g[i]
            assert V.level_stream(z[i], level).tobytes() == out[i].tobytes()


def test_pcm16_of_a_normalised_stream_never_clamps():
    """With peak < 1 no 16-bit sample is +-32767, the value the clamp gives; with peak == 1 the largest is exactly that."""
    rng = np.random.default_rng(7)
    for peak in (0.25, 0.5, 0.9, 0.999, float(np.nextafter(np.float32(1), np.float32(0))), 1.0):
        for scale in (1e-3, 1.0, 7.5, 1e4):
            z = (rng.standard_normal(4000) * scale).astype(np.float32)
            out = V.level_stream(z, (NORMALIZE, 1.0, peak))
            assert float(np.abs(out).max()) == float(np.float32(peak))
            for word in (2, 4, 8, 9):
                pcm = V.pcm16(out) if word != 2 else np.frombuffer(V.stream_body(out, 2), dtype="<i2")
                assert (int(np.abs(pcm.astype(np.int32)).max()) == 32767) == (peak == 1.0), (peak, scale, word)
            # un-levelled, the streams whose samples pass 1 clip: that is what the ceiling is for
            assert (np.abs(V.pcm16(z).astype(np.int32)).max() == 32767) == bool(np.abs(z).max() >= 1.0)


def test_ceiling_leaves_quiet_streams_alone_and_caps_loud_ones():
    rng = np.random.default_rng(8)
    for scale in (0.01, 0.2, 3.0):
        z = (rng.uniform(-1, 1, 1000) * scale).astype(np.float32)
        p, g = V.level_gain(z, (CEILING, 2.0, 0.5))
        if 2.0 * float(p) > 0.5:
            assert g == 0.5 / float(p) and float(np.abs(V.level_stream(z, (CEILING, 2.0, 0.5))).max()) == 0.5
        else:
            assert g == 2.0 and V.level_stream(z, (CEILING, 2.0, 0.5)).tobytes() == (z * np.float32(2)).tobytes()


BAD_SPECS = [(3, 1.0, 0.0), (-1, 1.0, 0.0), (0, -0.5, 0.0), (0, 65.0, 0.0), (0, float("nan"), 0.0), (2, float("inf"), 0.5), (0, 1.0, 0.5),
             (0, 1.0, -0.0), (0, 1.0, float("nan")), (1, 2.0, 0.5), (1, 0.5, 0.5), (1, 1.0, 0.0), (1, 1.0, 2.0 ** -16), (1, 1.0, 1.0000001),
             (1, 1.0, float("nan")), (2, 1.0, 0.0), (2, 1.0, 2.0), (2, 1.0, float("nan")), (2, float("nan"), 0.5), (2, 1.0, -0.5),
             (1.5, 1.0, 0.5)]


def test_mirror_refuses_every_invalid_spec():
    z = np.array([0.25, -0.5], dtype=np.float32)
    for bad in BAD_SPECS:
        with pytest.raises(ValueError):
            V.level_gain(z, bad)
        with pytest.raises(ValueError):
            V.level_stream(z, bad)
    for ok in ((0, 0.0, 0.0), (0, 64.0, 0.0), (1, 1.0, 1.0), (1, 1.0, 2.0 ** -15), (2, 0.0, 2.0 ** -15), (2, 64.0, 1.0)):
        V.level_gain(z, ok)


def test_levelled_body_is_join_resample_level_form():
    rng = np.random.default_rng(9)
    d = [[2, 1, 3], [1, 2]]
    chunks = [rng.uniform(-0.3, 0.3, 600 * sum(x)).astype(np.float32) for x in d]
    join, level = (7, 10, 85, 1), (NORMALIZE, 1.0, 0.5)
    for word in (0x000, 0x108, 0x204, 0x303):
        y = V.resample_stream(V.join_stream(chunks, d, join), word)
        assert V.levelled_body(chunks, d, word, join, level) == V.stream_body(V.level_stream(y, level), word)
        assert V.levelled_body(chunks, d, word, join, None) == V.joined_body(chunks, d, word, join)
        assert V.levelled_body(chunks, d, word, None, level) == V.stream_body(V.level_stream(V.resample_stream(np.concatenate(chunks), word), level), word)


# ---- the host layout (HIP-free, under the sanitizers) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("level_plan") / "level_plan_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "level_plan_check.cpp"), os.path.join(csrc, "host_request.cpp"),
                    "-lpthread", "-o", exe], check=True)

    def run(mode, text=""):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, mode], env=env, input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _case_text(name, durs, cpr, words, joins, want, levels):
    flat = [name, len(durs), len(cpr)] + [len(d) for d in durs] + [v for d in durs for v in d] + list(cpr) + list(words)
    flat += [0 if joins is None else 1] + [v for j in (joins or [(0, 0, 0, 0)] * len(cpr)) for v in j] + [int(w) for w in want]
    flat += [len(levels)] + [v for m, g, p in levels for v in (m, _bits(g), _bits(p))]
    return " ".join(str(v) for v in flat) + "\n"


def _parse(out):
    cases, cur = {}, None
    for line in out.splitlines():
        kind, *rest = line.split()
        if kind == "case":
            cur = cases.setdefault(rest[0], {"req": [], "sizes": None, "bounds": None})
        elif kind == "req":
            cur["req"].append([int(v) for v in rest[1:]])
        elif kind in ("sizes", "bounds"):
            cur[kind] = [int(v) for v in rest]
        else:
            assert kind == "done", line
    return cases


def _bytes_of(word, n):
    form = word & 0xFF
    return {0: 4 * n, 1: 8 * n, 2: 2 * n, 3: 44 + 4 * n, 4: 4 * ((44 + 2 * n + 2) // 3), 8: n, 9: n}[form]


LEVEL_CHOICES = [(GAIN, 1.0, 0.0), (GAIN, 0.0, 0.0), (GAIN, 2.5, 0.0), (NORMALIZE, 1.0, 1.0), (NORMALIZE, 1.0, 0.5), (CEILING, 4.0, 0.75),
                 (CEILING, 1.0, 2.0 ** -15)]


def test_plan_builder_on_200_random_plans_mixing_words_joins_marks_and_levels(driver):
    """Rows 1..6, lens 1..6, durations 1..9 (a few rows much longer, so that a request has several peak windows), mixed words,
    join specs or none at all, want flags, one shared level spec or one per request, all-plain specs among them.  The levels
    block sits at the marks' end rounded up to 8, is 16 R bytes, end_bytes is its end, the peak table has R rows of the longest
    request's windows, and the three bounds of output_bounds hold; with levels the packed bound is 8 + 16 R larger.  (The driver
    itself compares every plan with the one of the same layout without levels, field for field.)"""
    rng = np.random.default_rng(20261020)
    forms, cases, text = (0, 1, 2, 3, 4, 8, 9), {}, ""
    for i in range(200):
        B = int(rng.integers(1, 7))
        durs = [[int(v) for v in rng.integers(1, 10, int(rng.integers(1, 7)))] for _ in range(B)]
        if i % 5 == 0:
            durs[int(rng.integers(0, B))][0] = int(rng.integers(10, 40))
        cpr = []
        while sum(cpr) < B:
            cpr.append(int(rng.integers(1, B - sum(cpr) + 1)))
        R = len(cpr)
        words = [int(rng.choice(forms)) | int(rng.integers(0, 4)) << 8 for _ in range(R)]
        joins = None if i % 3 == 0 else [(int(rng.integers(0, 8)), int(rng.choice([0, 10, 30, 1000])), int(rng.choice([0, 1, 85, 200, 5000])),
                                          int(rng.choice([0, 1, 12]))) if rng.random() > 0.15 else (0, 0, 0, 0) for _ in range(R)]
        want = [int(rng.integers(0, 2)) for _ in range(R)]
        if i % 7 == 0:
            levels = [LEVEL_CHOICES[0]] * (1 if i % 2 else R)
        else:
            levels = [LEVEL_CHOICES[int(rng.integers(0, len(LEVEL_CHOICES)))] for _ in range(1 if i % 4 == 1 else R)]
        cases[f"c{i}"] = (durs, cpr, words, joins, want, levels)
        text += _case_text(f"c{i}", durs, cpr, words, joins, want, levels)
    got = _parse(driver("plans", text))
    assert len(got) == 200
    seen_windows, seen_plain, seen_gap = set(), 0, 0
    for name, (durs, cpr, words, joins, want, levels) in cases.items():
        g = got[name]
        R = len(cpr)
        row, off, n_marks, longest, y_floats = 0, 0, 0, 0, 0
        for r, n in enumerate(cpr):
            d = durs[row: row + n]
            L, M = LM[words[r] >> 8]
            S = sum(k + gap for _, k, gap, _, _ in V.join_rows(d, joins[r] if joins else None))
            n_out = S * L // M
            nm = sum(len(x) + 1 for x in d) if want[r] else 0
            mode, gain, peak = levels[r if len(levels) > 1 else 0]
            assert g["req"][r] == [off, _bytes_of(words[r], n_out), n_out, nm, mode, _bits(gain), _bits(peak)], (name, r)
            off += _bytes_of(words[r], n_out)
            n_marks += nm
            longest = max(longest, n_out)
            y_floats += n_out if words[r] >> 8 else 0
            row += n
        total, marks_off, nmk, levels_off, end, measured, levelled, windows, dwords = g["sizes"]
        assert (total, marks_off, nmk) == (off, (off + 7) & ~7, n_marks)
        assert levels_off == (marks_off + 8 * n_marks + 7) & ~7 and levels_off % 8 == 0 and end == levels_off + 16 * R
        assert measured == 1 and levelled == int(any(tuple(lv) != LEVEL_CHOICES[0] for lv in levels))
        assert windows == -(-longest // WINDOW) and dwords == R * windows
        packed, y_bound, peak_bound, packed_without = g["bounds"]
        assert packed >= end and y_bound >= y_floats and peak_bound >= dwords and packed == packed_without + 8 + 16 * R, name
        seen_windows.add(windows)
        seen_plain += not levelled
        seen_gap += marks_off != total
    assert len(seen_windows) >= 4 and seen_plain >= 10 and seen_gap >= 20


def test_refusals_of_the_level_arguments(driver):
    got = dict(line.split("\t", 1) for line in driver("refusals").splitlines())
    bad = "1\tinfer: bad level"
    names = ["mode_3", "mode_high_bit", "gain_negative", "gain_65", "gain_nan", "gain_inf", "mode0_peak_set", "mode0_peak_minus_0",
             "mode0_peak_nan", "mode1_gain_2", "mode1_peak_0", "mode1_peak_small", "mode1_peak_above_1", "mode1_peak_nan", "mode2_peak_0",
             "mode2_peak_2", "mode2_peak_nan", "mode2_gain_nan", "mode2_peak_negative", "third_of_three_bad"]
    want = {n: bad for n in names}
    want.update({"null_levels": "1\tinfer: null level argument", "n_level_0": "1\tinfer: bad level count",
                 "n_level_2_of_3": "1\tinfer: bad level count", "n_level_minus_1": "1\tinfer: bad level count",
                 "ok_shared": "accepted", "ok_per_request": "accepted"})
    assert got == want


def test_dispatcher_checks_the_spec_at_submit_and_carries_it_to_the_batch(driver):
    got = dict(line.split("\t", 1) for line in driver("dispatcher").splitlines())
    bad = "1\tdispatcher_submit_request: bad level"
    one, half, three_q, four = _bits(1.0), _bits(0.5), _bits(0.75), _bits(4.0)
    assert got == {
        "null_level": bad, "mode_3": bad, "gain_nan": bad, "peak_2": bad, "mode1_gain_2": bad, "mode0_peak_minus_0": bad,
        "bad_join": "1\tdispatcher_submit_request: bad join",
        "ok_no_join": f"accepted\t1 {one:#x} {half:#x} levelled=1 joined=0 pause=0 out=0.25 3",
        "ok_join": f"accepted\t2 {four:#x} {three_q:#x} levelled=1 joined=1 pause=85 out=0.25 3",
        "ok_plain_no_out": f"accepted\t0 {one:#x} 0 levelled=1 joined=0 pause=0 out=-1 -1",
        "old_entry": f"accepted\t0 {one:#x} 0 levelled=0 joined=1 pause=85",
    }


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_part_of_the_abi():
    from kokorox_amd import hip_koko as hk
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    test_header = open(os.path.join(ROOT, "include", "kokorox_hip_test.h"), encoding="utf-8").read()
    for name in ("kx_infer_requests_levelled", "kx_dispatcher_submit_request_levelled"):
        assert name in hk.ABI_SYMBOLS and re.search(r"^int %s\(" % name, header, re.M), name
        assert name not in test_header
    assert "kx_test_output_plan_levelled" in hk.TEST_ABI_SYMBOLS and "kx_test_output_plan_levelled" not in hk.ABI_SYMBOLS
    assert "kx_test_output_plan" in hk.TEST_ABI_SYMBOLS
    assert re.search(r"^int kx_test_output_plan_levelled\(", test_header, re.M) and "kx_test_output_plan_levelled" not in header
    for text in ("infer: null level argument", "infer: bad level count", "infer: bad level", "dispatcher_submit_request: bad level"):
        assert '"%s"' % text in header, text
    assert (hk.LEVEL_GAIN, hk.LEVEL_NORMALIZE, hk.LEVEL_CEILING) == (0, 1, 2) == (V.LEVEL_GAIN, V.LEVEL_NORMALIZE, V.LEVEL_CEILING)
    for name, value in (("KX_LEVEL_GAIN", 0), ("KX_LEVEL_NORMALIZE", 1), ("KX_LEVEL_CEILING", 2)):
        assert re.search(r"^#define %s\s+%du\b" % (name, value), header, re.M), name
    assert hk.LEVEL_DTYPE.itemsize == 12 and list(hk.LEVEL_DTYPE.names) == ["mode", "gain", "peak"]
    assert hk.LEVEL_PLAIN == (0, 1.0, 0.0) == V.LEVEL_PLAIN
    lv = hk.level_specs((1, 1.0, 0.5), 3)
    assert lv.shape == (3,) and lv.tobytes() == struct.pack("<Iff", 1, 1.0, 0.5) * 3
    assert hk.level_specs([(0, 1.0, 0.0), (2, 4.0, 0.75)]).shape == (2,)
    with pytest.raises(ValueError):
        hk.level_specs([(0, 1.0, 0.0)], 2)
    for fn in ("infer_requests_levelled",):
        assert callable(getattr(hk.HipKoko, fn))
    assert callable(hk.level_requests)


def test_header_restates_the_definition():
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    assert re.search(r"/\* ---- levels", header)
    for phrase in ("typedef struct kx_level { uint32_t mode; float gain; float peak; } kx_level;", "what form 0 in its format word would hold",
                   "after the join,", "after the resampler", "for which z[n] is not a NaN", "p = 0 when there is no such n", "+inf counts",
                   "0 < p < +inf", "g = f64(gain)", "g = f64(peak) / f64(p) if p is usable, else 1.0", "g * f64(p) > f64(peak)",
                   "z'[n] = f32(g * f64(z[n]))", "A NaN stays a", "Marks, out_samples, headers and sizes do not change",
                   "gain is exactly 1.0f in mode 1", "peak is +0.0f in mode 0", "2^-15 <= peak <= 1", "{0, 1.0f, 0.0f}",
                   "f32((f64(peak) / f64(p)) * f64(p)) == peak", "the clamp of the 16-bit forms never engages", "a peak meter"):
        assert phrase in header, phrase


def test_rust_crate_binds_the_struct_and_both_entries():
    rs = open(os.path.join(ROOT, "kokorox-hip", "src", "lib.rs"), encoding="utf-8").read()
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct KxLevel \{(.*?)\}", rs, flags=re.S)
    assert m, "lib.rs lacks a #[repr(C)] KxLevel"
    assert re.findall(r"pub (\w+): (\w+)", m.group(1)) == [("mode", "u32"), ("gain", "f32"), ("peak", "f32")]
    for name in ("kx_infer_requests_levelled", "kx_dispatcher_submit_request_levelled"):
        assert re.search(r"\bfn %s\s*\(" % name, rs), name
    for name, value in (("KX_LEVEL_GAIN", 0), ("KX_LEVEL_NORMALIZE", 1), ("KX_LEVEL_CEILING", 2)):
        assert re.search(r"pub const %s: u32 = %d;" % (name, value), rs), name
