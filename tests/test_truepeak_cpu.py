"""CPU: true peak -- KX_PEAK_TRUE in a level or a loudness spec (include/kokorox_hip.h, "levels", True peak).

Layers that need no GPU: the committed interpolator table against its generator, against the formula recomputed here and against
the ideal fractional delay; the numpy definition (kokorox_amd/voices.py: true_peak, level_gain and loudness_gain with the flag) on
noise, constants, the fs/4 anchors of tests/golden/truepeak.json and non-finite samples; the host layout
(kokorox_amd/csrc/host_request.cpp: the two spec checks, build_output_plan, output_bounds) and the dispatcher's submit-time
checks, built with g++ -fsanitize=address,undefined into tests/cpp/truepeak_plan_check.cpp and run as a child process; and the ABI
(header, Python table, C++ wrapper, lib.rs).
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
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "truepeak.json"), encoding="utf-8"))
TRUE = 0x100
NONE = 0xFFFFFFFF
LM = {0: (1, 1), 1: (1, 3), 2: (2, 3), 3: (2, 1)}
WINDOW = 4096  # host_request.h: LEVEL_WINDOW


def _formula():
    """The 72 taps from the definition, written out once more: float64 throughout, one rounding to float32."""
    i = np.arange(97, dtype=np.float64)
    w = np.sinc((i - 48.0) / 4.0) * np.kaiser(97, 8.0)
    t = np.stack([w[4 * np.arange(24) + phi] for phi in (1, 2, 3)])
    return (t / t.sum(axis=1, keepdims=True)).astype(np.float32)


# ---- the table -------------------------------------------------------------------------------------------------------------
def test_committed_table_is_what_the_generator_gives():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_truepeak_taps.py"), "--check"])
    assert r.returncode == 0, "kokorox_amd/csrc/truepeak_taps.h differs from tools/gen_truepeak_taps.py"


def test_library_hands_out_the_formula_and_refuses_a_short_buffer():
    import ctypes as C

    from kokorox_amd import hip_koko as hk
    want = _formula()
    got = hk.truepeak_filter()
    assert got.dtype == np.float32 and got.shape == (3, 24) and got.tobytes() == want.tobytes()
    assert V.true_peak_taps().tobytes() == want.tobytes()
    text = open(os.path.join(ROOT, "kokorox_amd", "csrc", "truepeak_taps.h"), encoding="utf-8").read()
    bits = [int(b, 16) for b in re.findall(r"0x([0-9A-F]{8})u", text)]
    assert np.array(bits, dtype=np.uint32).tobytes() == want.tobytes()
    lib, buf = hk.load_library(), (C.c_float * 72)()
    assert lib.kx_truepeak_filter(buf, 71) == hk.KX_ERR_INVALID and lib.kx_truepeak_filter(None, 72) == hk.KX_ERR_INVALID
    assert lib.kx_truepeak_filter(buf, 72) == 0 and bytes(buf) == want.tobytes()


def test_every_phase_has_dc_gain_one_and_phase_1_mirrors_phase_3():
    t = V.true_peak_taps()
    assert np.abs(t.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-7
    assert t[0].tobytes() == t[2][::-1].tobytes()


def test_phase_error_against_the_ideal_fractional_delay():
    """u_phi[n] = sum over m of t_phi[m] x[n + 12 - m]: the response to e^(i w n) is sum t_phi[m] e^(i w (12 - m)), the ideal one
    e^(i w phi / 4).  Measured here: 8.1e-5 up to half the Nyquist frequency, 1.35e-3 up to 0.8 of it."""
    t = V.true_peak_taps().astype(np.float64)
    m = np.arange(24)
    for upto, bound in ((0.5, 1e-4), (0.8, 2e-3)):
        w = np.linspace(0.0, upto, 4001) * np.pi
        worst = 0.0
        for phi in (1, 2, 3):
            H = (t[phi - 1][None, :] * np.exp(1j * w[:, None] * (12 - m)[None, :])).sum(axis=1)
            worst = max(worst, float(np.abs(H - np.exp(1j * w * phi / 4)).max()))
        print(f"phase error up to {upto} Nyquist: {worst:.3e}")
        assert worst <= bound


# ---- the numpy definition --------------------------------------------------------------------------------------------------
def _scalar_true_peak(z):
    """The definition one term at a time, for short streams: a Python float accumulator from +0, ascending j."""
    t = V.true_peak_taps()
    z = np.asarray(z, dtype=np.float32)
    N, best = z.shape[0], np.float32(0)
    for v in z:
        if not np.isnan(v):
            best = max(best, np.float32(abs(v)))
    for phi in range(3):
        for n in range(N):
            acc = 0.0
            for j in range(n - 11, n + 13):
                x = float(z[j]) if 0 <= j < N and np.isfinite(z[j]) else 0.0
                acc = acc + float(t[phi, n - j + 12]) * x
            with np.errstate(over="ignore"):
                best = max(best, np.float32(abs(np.float32(acc))))
    return np.float32(best)


def test_mirror_is_the_definition_term_by_term_and_never_below_the_sample_peak():
    rng = np.random.default_rng(20261101)
    for n in (1, 2, 11, 12, 13, 23, 24, 25, 60):
        z = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        assert V.true_peak(z).tobytes() == _scalar_true_peak(z).tobytes(), n
    assert V.true_peak(np.zeros(0, dtype=np.float32)) == 0 and V.true_peak(np.zeros(5, dtype=np.float32)) == 0
    for seed in range(5):
        z = np.random.default_rng(seed).uniform(-1.0, 1.0, 5000).astype(np.float32)
        tp = V.true_peak(z)
        assert tp.dtype == np.float32 and tp >= np.abs(z).max()
    assert V.true_peak(np.random.default_rng(1).uniform(-1.0, 1.0, 5000).astype(np.float32)) > 1.0  # (noise overshoots between samples)


def test_a_constant_stream_reads_the_constant_in_its_interior():
    c = np.float32(0.3)
    t = V.true_peak_taps().astype(np.float64)
    x = np.full(200, c, dtype=np.float32).astype(np.float64)
    for phi in range(3):  # n = 11 .. N - 13: all 24 terms are inside the stream
        u = np.array([np.float32(sum(t[phi, n - j + 12] * x[j] for j in range(n - 11, n + 13))) for n in range(11, 200 - 12)])
        assert np.abs(u.astype(np.float64) - float(c)).max() <= 1e-6
    # (the edges of the burst ring: the stream's tp lies above the constant, by the step response's overshoot and no more)
    assert c < V.true_peak(np.full(200, c, dtype=np.float32)) < np.float32(1.2) * c


@pytest.mark.parametrize("case", GOLDEN["anchors"], ids=[c["name"] for c in GOLDEN["anchors"]])
def test_fs4_anchors_read_inside_the_ebu_window(case):
    n = np.arange(case["samples"])
    z = (case["amplitude"] * np.sin(2 * np.pi * n / 4 + np.deg2rad(case["phase_deg"]))).astype(np.float32)
    tp = V.true_peak(z)
    db = 20 * np.log10(float(tp))
    print(f"{case['name']}: tp = {tp!r}, {db:.4f} dBTP")
    lo, hi = GOLDEN["window_dbtp"]
    assert (lo, hi) == (-6.4, -5.8) and lo <= db <= hi and abs(db - case["dbtp"]) <= 5e-4
    if case["exact_tp"] is not None:
        assert tp.tobytes() == np.float32(case["exact_tp"]).tobytes()


def test_non_finite_samples_and_the_gain_rules():
    rng = np.random.default_rng(7)
    z = rng.uniform(-0.5, 0.5, 300).astype(np.float32)
    gap, zeroed = z.copy(), z.copy()
    gap[[5, 150]] = np.nan
    zeroed[[5, 150]] = 0.0
    assert V.true_peak(gap).tobytes() == V.true_peak(zeroed).tobytes()  # a NaN counts as a gap
    inf = z.copy()
    inf[40] = -np.inf
    assert V.true_peak(inf) == np.float32(np.inf)
    for spec in ((1 | TRUE, 1.0, 0.5), (2 | TRUE, 4.0, 0.5)):
        p, g = V.level_gain(inf, spec)
        assert p == np.float32(np.inf) and g == (1.0 if spec[0] & 3 == 1 else 4.0)
    assert V.loudness_gain(np.float32(np.inf), -30.0, (1 | TRUE, -23.0, 0.5)) == float(np.float64(10.0) ** (np.float64(7.0) / np.float64(20.0)))
    # the rules with tp in place of p
    tp, p = V.true_peak(z), np.abs(z).max()
    assert tp > p
    assert V.level_gain(z, (TRUE, 2.0, 0.0)) == (tp, 2.0) and V.level_gain(z, (0, 2.0, 0.0)) == (p, 2.0)
    assert V.level_gain(z, (1 | TRUE, 1.0, 0.5)) == (tp, float(np.float64(np.float32(0.5)) / np.float64(tp)))
    assert V.level_gain(z, (2 | TRUE, 1.0, 1.0)) == (tp, 1.0) and V.level_gain(z, (2 | TRUE, 8.0, 1.0)) == (tp, float(np.float64(1.0) / np.float64(tp)))
    assert V.loudness_gain(tp, -20.0, (1 | TRUE, -3.0, 0.25)) == float(np.float64(np.float32(0.25)) / np.float64(tp))
    assert V.loudness_gain(tp, -20.0, (TRUE, 0.0, 0.0)) == 1.0


def test_no_sample_of_the_normalised_stream_exceeds_the_peak():
    """g = f64(peak) / f64(tp) with tp >= p: f32(g z) never passes `peak`, so the 16-bit forms cannot clip; and the true peak of the
    result is `peak` up to rounding: 2^-24 relative from tp's own rounding, sum |t| x 2^-24 with sum |t| < 3 from the rounding of
    every z', 2^-24 from the rounding of the interpolated value -- 5 x 2^-24 in all."""
    for seed, peak in ((0, 1.0), (1, 0.5), (2, 2.0 ** -15), (3, 0.7)):
        z = (np.random.default_rng(seed).standard_normal(3000) * 3.0).astype(np.float32)
        out = V.level_stream(z, (1 | TRUE, 1.0, peak))
        assert np.abs(out).max() <= np.float32(peak)
        assert abs(float(V.true_peak(out)) / float(np.float32(peak)) - 1.0) <= 3 * 2.0 ** -24 + 2.0 ** -23
        body = V.levelled_body([z], [[5]], 2, None, (1 | TRUE, 1.0, peak))
        assert body == V.stream_body(out, 2)
    z = (np.random.default_rng(9).standard_normal(3000) * 3.0).astype(np.float32)
    pcm = np.frombuffer(V.levelled_body([z], [[5]], 2, None, (1 | TRUE, 1.0, 1.0)), dtype="<i2")
    assert np.abs(pcm.astype(np.int32)).max() < 32767  # (the largest sample lies below the true peak)


BAD_LEVELS = [(0x200, 1.0, 0.0), (0x301, 1.0, 0.5), (0x103, 1.0, 0.5), (3, 1.0, 0.5), (0x80000000, 1.0, 0.0), (0x00010001, 1.0, 0.5),
              (NONE, 1.0, 0.0), (0x101, 2.0, 0.5), (0x100, 1.0, 0.5), (0x102, 1.0, 2.0)]
BAD_LOUDNESS = [(0x200, 0.0, 0.0), (0x301, -23.0, 0.5), (0x103, -23.0, 0.5), (0x102, -23.0, 0.5), (NONE, 0.0, 0.0), (0x00010001, -23.0, 1.0),
                (0x100, -23.0, 0.0), (0x101, 1.0, 1.0)]


def test_mirror_refuses_what_the_library_refuses():
    z = np.float32([0.25, -0.5])
    for bad in BAD_LEVELS:
        with pytest.raises(ValueError):
            V.level_gain(z, bad)
    for bad in BAD_LOUDNESS:
        with pytest.raises(ValueError):
            V.loudness_gain(np.float32(0.5), -20.0, bad)
    for ok in ((0x100, 2.0, 0.0), (0x101, 1.0, 0.5), (0x102, 2.0, 0.5)):
        V.level_gain(z, ok)
    for ok in ((0x100, 0.0, 0.0), (0x101, -23.0, 0.5)):
        V.loudness_gain(np.float32(0.5), -20.0, ok)


# ---- the host layout (HIP-free, under the sanitizers) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("truepeak_plan") / "truepeak_plan_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "truepeak_plan_check.cpp"), os.path.join(csrc, "host_request.cpp"),
                    "-lpthread", "-o", exe], check=True)

    def run(mode, text=""):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, mode], env=env, input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _hex(v):
    return "0" if v == 0 else f"{v:#x}"  # (printf's %#x)


def test_both_spec_checks_over_every_low_byte_mode_with_and_without_the_flag(driver):
    """Of the 2 x 256 modes of each kind exactly {0, 1, 2} and {0, 1, 2} | 0x100 pass for levels, {0, 1} and {0, 1} | 0x100 for
    loudness, each with the fields of its low byte and with no other set (bit i of the last column: field set i of the driver passed)."""
    got = driver("specs").split("\n")[:-1]
    sets = {"level": {0: 1, 1: 2, 2: 6}, "loudness": {0: 1, 1: 2}}  # (a ceiling takes mode 1's fields as well as its own)
    want = [f"{kind} {_hex(mode | flag)} {sets[kind][mode]}" for flag in (0, TRUE) for mode in (0, 1, 2) for kind in ("level", "loudness")
            if mode in sets[kind]]
    assert got == want


def test_library_hands_out_the_table_in_the_hip_free_unit_too(driver):
    rows = driver("taps").splitlines()
    got = np.array([[int(v, 16) for v in r.split()] for r in rows], dtype=np.uint32)
    assert got.shape == (3, 24) and got.tobytes() == _formula().tobytes()


def test_refusals_keep_todays_texts(driver):
    got = dict(line.split("\t", 1) for line in driver("refusals").splitlines())
    lv, ld = "1\tinfer: bad level", "1\tinfer: bad loudness"
    want = {"level_0x200": lv, "level_0x301": lv, "level_0x103": lv, "level_0x80000000": lv, "level_0x80000001": lv, "level_0x00010001": lv,
            "level_3": lv, "level_none": lv, "level_0x100_ok": "accepted", "level_0x101_ok": "accepted", "level_0x102_ok": "accepted",
            "loudness_0x200": ld, "loudness_0x301": ld, "loudness_0x103": ld, "loudness_0x102": ld, "loudness_none": ld,
            "loudness_0x80000001": ld, "loudness_0x00010001": ld, "loudness_2": ld, "loudness_0x100_ok": "accepted",
            "loudness_0x101_ok": "accepted"}
    assert got == want


LEVEL_CHOICES = [(0, 1.0, 0.0), (0, 2.0, 0.0), (1, 1.0, 0.5), (2, 4.0, 1.0)]
LOUD_CHOICES = [(0, 0.0, 0.0), (1, -23.0, 1.0), (1, -16.0, 0.5)]


def test_plan_builder_on_100_random_plans_with_and_without_flagged_requests(driver):
    """Rows of 1..60 frames grouped into requests, mixed words; every request has a level spec, a loudness spec or neither, and in
    every other plan some of them carry the flag.  true_peak is set exactly when a governing spec has it; the second table has
    the first one's size then and none otherwise; output_bounds sizes it the same way before the forward; every other field is
    what the layout gives without the flag (judged by the driver) and what the parent's layout rules give (recomputed here)."""
    rng = np.random.default_rng(20261102)
    forms, cases, text = (0, 1, 2, 3, 4, 8, 9), {}, ""
    for i in range(100):
        B = int(rng.integers(1, 7))
        frames = [int(rng.integers(1, 61)) for _ in range(B)]
        cpr = []
        while sum(cpr) < B:
            cpr.append(int(rng.integers(1, B - sum(cpr) + 1)))
        R = len(cpr)
        words = [int(rng.choice(forms)) | int(rng.integers(0, 4)) << 8 for _ in range(R)]
        levels, louds = [], []
        for r in range(R):
            kind = int(rng.integers(0, 3)) if i % 5 else 0  # 0: a level spec, 1: metered, 2: plain beside the others
            flag = TRUE if i % 2 == 0 and rng.integers(0, 4) else 0  # (three in four of an even plan's requests)
            if kind == 1:
                m, t, p = LOUD_CHOICES[int(rng.integers(0, 3))]
                levels.append((0, 1.0, 0.0))
                louds.append((m | flag, t, p))
            else:
                m, g, p = LEVEL_CHOICES[int(rng.integers(0, 4))] if kind == 0 else (0, 1.0, 0.0)
                levels.append((m | (flag if kind == 0 else 0), g, p))
                louds.append((NONE, 0.0, 0.0))
        cases[f"c{i}"] = (frames, cpr, words, levels, louds)
        flat = [f"c{i}", B, R] + frames + cpr + words + [v for m, a, b in levels + louds for v in (m, _bits(a), _bits(b))]
        text += " ".join(str(v) for v in flat) + "\n"
    out = driver("plans", text)
    got, cur = {}, None
    for line in out.splitlines():
        kind, *rest = line.split()
        if kind == "case":
            cur = got.setdefault(rest[0], {})
        elif kind in ("sizes", "bounds"):
            cur[kind] = [int(v) for v in rest]
        else:
            assert kind == "done" and rest == ["100"], line
    seen_flagged = seen_plain = seen_loud_flag = 0
    for name, (frames, cpr, words, levels, louds) in cases.items():
        g, R = got[name], len(cpr)
        row, total, longest = 0, 0, 0
        for r, n in enumerate(cpr):
            L, M = LM[words[r] >> 8]
            n_out = 600 * sum(frames[row: row + n]) * L // M
            total += {0: 4 * n_out, 1: 8 * n_out, 2: 2 * n_out, 3: 44 + 4 * n_out, 4: 4 * ((44 + 2 * n_out + 2) // 3), 8: n_out, 9: n_out}[words[r] & 0xFF]
            longest = max(longest, n_out)
            row += n
        metered = [ld[0] != NONE for ld in louds]
        flagged = any((ld[0] if on else lv[0]) & TRUE for lv, ld, on in zip(levels, louds, metered))
        levelled = any(lv != (0, 1.0, 0.0) for lv in levels) or any(on and ld[0] & 0xFF == 1 for ld, on in zip(louds, metered))
        windows = -(-longest // WINDOW)
        levels_off = (total + 7) & ~7
        loud_off = levels_off + 16 * R if any(metered) else 0
        end = (loud_off if any(metered) else levels_off) + 16 * R
        assert g["sizes"] == [int(flagged), R * windows if flagged else 0, R * windows, windows, 1, int(levelled), levels_off, loud_off, end], name
        packed, peak_bound, tp_bound, hop_bound = g["bounds"]
        assert packed >= end and peak_bound >= R * windows and tp_bound == (peak_bound if flagged else 0) and (hop_bound > 0) == any(metered), name
        seen_flagged += flagged
        seen_plain += not flagged
        seen_loud_flag += any(on and ld[0] & TRUE for ld, on in zip(louds, metered))
    assert seen_flagged >= 25 and seen_plain >= 50 and seen_loud_flag >= 10


def test_dispatcher_accepts_a_flagged_spec_at_submit_and_carries_it_to_the_batch(driver):
    got = dict(line.split("\t", 1) for line in driver("dispatcher").splitlines())
    lv, ld = "1\tdispatcher_submit_request: bad level", "1\tdispatcher_submit_request: bad loudness"
    one, two, half, target = _bits(1.0), _bits(2.0), _bits(0.5), _bits(-23.0)
    assert got == {
        "level_norm_tp": f"accepted\tlevel 0x101 {one:#x} {half:#x} loudness 0 0 0 levelled=1 metered=0",
        "level_gain_tp": f"accepted\tlevel 0x100 {two:#x} 0 loudness 0 0 0 levelled=1 metered=0",
        "level_0x200": lv, "level_0x103": lv, "level_0x301": lv, "level_0x101_gain_2": lv,
        "loudness_meter_tp": f"accepted\tlevel 0 {one:#x} 0 loudness 0x100 0 0 levelled=0 metered=1",
        "loudness_norm_tp": f"accepted\tlevel 0 {one:#x} 0 loudness 0x101 {target:#x} {half:#x} levelled=0 metered=1",
        "loudness_0x200": ld, "loudness_0x102": ld, "loudness_0x103": ld, "loudness_none": ld,
    }


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_the_flag_and_the_accessor_are_part_of_the_abi():
    from kokorox_amd import hip_koko as hk
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    test_header = open(os.path.join(ROOT, "include", "kokorox_hip_test.h"), encoding="utf-8").read()
    assert "kx_truepeak_filter" in hk.ABI_SYMBOLS and re.search(r"^int kx_truepeak_filter\(float\* taps, int cap\);", header, re.M)
    assert "kx_truepeak_filter" not in test_header and "kx_truepeak_filter" not in hk.TEST_ABI_SYMBOLS
    assert re.search(r"^#define KX_PEAK_TRUE\s+0x100u\b", header, re.M)
    assert hk.PEAK_TRUE == 0x100 == V.PEAK_TRUE and callable(hk.truepeak_filter) and callable(V.true_peak) and callable(V.true_peak_taps)
    lv = hk.level_specs((hk.LEVEL_NORMALIZE | hk.PEAK_TRUE, 1.0, 0.5), 2)
    assert lv.tobytes() == struct.pack("<Iff", 0x101, 1.0, 0.5) * 2
    ld = hk.loudness_specs((hk.LOUDNESS_NORMALIZE | hk.PEAK_TRUE, -23.0, 0.5), 2)
    assert ld.tobytes() == struct.pack("<Iff", 0x101, -23.0, 0.5) * 2
    hpp = open(os.path.join(ROOT, "include", "kokorox_hip.hpp"), encoding="utf-8").read()
    assert re.search(r"\bkx_truepeak_filter\s*\(", hpp) and re.search(r"\btruepeak_filter\s*\(", hpp) and "KX_PEAK_TRUE" in hpp
    rs = open(os.path.join(ROOT, "kokorox-hip", "src", "lib.rs"), encoding="utf-8").read()
    assert re.search(r"\bfn kx_truepeak_filter\s*\(taps: \*mut f32, cap: c_int\) -> c_int;", rs) and re.search(r"\bfn truepeak_filter\s*\(", rs)
    assert re.search(r"pub const KX_PEAK_TRUE: u32 = 0x100;", rs)
    integration = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    assert "KX_PEAK_TRUE" in integration and "kx_truepeak_filter" in integration
    # (the header still compiles as C++ on its own, and the flag composes with the modes)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], text=True, capture_output=True,
                       input='#include "kokorox_hip.h"\nstatic_assert((KX_LEVEL_CEILING | KX_PEAK_TRUE) == 0x102u && (KX_LOUDNESS_NORMALIZE | KX_PEAK_TRUE) == 0x101u, "");\n')
    assert r.returncode == 0, r.stderr
