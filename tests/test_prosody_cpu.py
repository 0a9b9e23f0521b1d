"""CPU: prosody (include/kokorox_hip.h, "prosody") -- the numpy definitions of kokorox_amd/voices.py against answers written out by
hand, the validity rule and the report block of the packed buffer (kokorox_amd/csrc/host_request.{h,cpp}: prosody_ok,
check_prosody_call, report_rows, build_output_plan, output_bounds) through tests/cpp/prosody_plan_check.cpp, built with
g++ -fsanitize=address,undefined and run as a child process (nothing is loaded into python), and the ABI (header, ctypes, C++
wrapper, lib.rs).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kokorox_amd import voices as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABOVE_10 = np.array([0x41200001], dtype=np.uint32).view(np.float32)[0]


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


# ---- the numpy definitions -------------------------------------------------------------------------------------------------------
def test_semitones_are_float32_powers_of_two():
    assert V.semitones(0) == np.float32(1.0) and V.semitones(12) == np.float32(2.0) and V.semitones(-12) == np.float32(0.5)
    assert V.semitones(7).dtype == np.float32 and V.semitones(7) == np.float32(2.0 ** (7 / 12))
    assert V.prosody_ok(pitch=[V.semitones(24), V.semitones(-24)]) and not V.prosody_ok(pitch=[V.semitones(24.1)])


def test_neutral_arrays_are_the_identity_bit_for_bit():
    rng = np.random.default_rng(1)
    d = rng.integers(1, 6, size=9)
    F = int(d.sum())
    f0 = rng.uniform(-50, 400, size=2 * F).astype(np.float32)
    f0[3] = np.float32(10.0)
    f0[5] = np.float32(np.nan)
    f0[7] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]  # a NaN with a payload: the bits stay
    n = rng.standard_normal(2 * F).astype(np.float32)
    n[2] = np.float32(np.nan)
    one = np.ones(9, np.float32)
    f0s, ns = V.shape_curves(f0, n, d, one, one)
    assert f0s.dtype == ns.dtype == np.float32
    assert (bits(f0s) == bits(f0)).all() and (bits(ns)[np.arange(2 * F) != 2] == bits(n)[np.arange(2 * F) != 2]).all() and np.isnan(ns[2])
    g0, gn = V.shape_curves(f0, n, d)  # (None: not touched at all)
    assert (bits(g0) == bits(f0)).all() and (bits(gn) == bits(n)).all()
    # durations: x / 1.0f is x, frames 0 = as predicted
    s = rng.uniform(0.2, 30, size=40).astype(np.float32)
    plain = V.prosody_durations(s)
    assert (V.prosody_durations(s, rate=np.ones(40, np.float32), frames=np.zeros(40, np.int32)) == plain).all()
    assert plain.dtype == np.int32 and (plain >= 1).all()


def test_durations_by_hand():
    s = np.array([0.2, 2.5, 3.5, 4.4, 7.0, 2.0], np.float32)
    assert V.prosody_durations(s).tolist() == [1, 2, 4, 4, 7, 2]  # (half to even, at least 1)
    rate = np.array([1, 0.5, 2, 4, 0.25, 1], np.float32)
    assert V.prosody_durations(s, rate=rate).tolist() == [1, 5, 2, 1, 28, 2]  # 0.2, 5.0, 1.75, 1.1, 28.0, 2.0
    frames = np.array([0, 50, 0, 1, 0, 0], np.int32)
    assert V.prosody_durations(s, rate=rate, frames=frames).tolist() == [1, 50, 2, 1, 28, 2]
    # the pinned pattern sits between the two: it replaces the prediction, frames replace it
    assert V.prosody_durations(s, rate=rate, frames=frames, pinned=[3, 9]).tolist() == [3, 50, 3, 1, 3, 9]
    # a row cut at idx_ld: the token that crosses the end gets the remainder, the ones behind it 0
    assert V.prosody_durations(s, idx_ld=9).tolist() == [1, 2, 4, 2, 0, 0]
    assert V.prosody_durations(s, frames=[0, 0, 0, 0, 0, 50], idx_ld=20).tolist() == [1, 2, 4, 4, 7, 2]


def test_the_window_clamps_at_both_ends_and_spans_three_tokens():
    # durations 1, 1, 1: six steps, tokens 0 0 1 1 2 2; ratios 1, 2, 4 on a flat voiced curve of 100
    d = [1, 1, 1]
    f0 = np.full(6, 100, np.float32)
    f0s, ns = V.shape_curves(f0, f0, d, pitch=[1, 2, 4], energy=[1, 2, 4])
    # j = 0: taps at cl(-2..2) = 0 0 0 1 2 -> tokens 0 0 0 0 1: (1 + 2 + 3 + 2 + 2) / 9; j = 2: 0 0 1 1 2: (1 + 2 + 6 + 4 + 4) / 9 ...
    want = np.array([10, 12, 17, 23, 30, 34], np.float64) / 9.0
    want32 = (np.float64(100) * want).astype(np.float32)
    assert (bits(f0s) == bits(want32)).all() and (bits(ns) == bits(want32)).all()
    # F = 1: the grid (two steps) is shorter than the window; one token, so its ratio exactly
    f1, n1 = V.shape_curves([100, 200], [1, -1], [1], pitch=[2], energy=[0.5])
    assert f1.tolist() == [200, 400] and n1.tolist() == [0.5, -0.5]


def test_the_voicing_guard():
    d = [2, 2]
    f0 = np.array([5, 10, 10.5, 300, np.nan, -3, 11, 40], np.float32)
    n = np.arange(8, dtype=np.float32)
    f0s, ns = V.shape_curves(f0, n, d, pitch=[0.25, 0.25], energy=[0, 0])
    # not > 10 (5, exactly 10, NaN, -3): as it is; voiced and still voiced (300 -> 75); voiced but at or below 10 after (10.5, 11, 40): the float above 10
    assert (bits(f0s[[0, 1, 4, 5]]) == bits(f0[[0, 1, 4, 5]])).all()
    assert f0s[3] == np.float32(75) and (bits(f0s[[2, 6, 7]]) == bits(ABOVE_10)).all()
    assert ((f0s > 10) == (f0 > 10)).all()  # the decision never flips
    assert (ns == 0).all()
    up, _ = V.shape_curves(f0, n, d, pitch=[4, 4])
    assert (bits(up[[0, 1, 4, 5]]) == bits(f0[[0, 1, 4, 5]])).all() and up[2] == np.float32(42) and up[3] == np.float32(1200)


def test_the_report_by_hand():
    d = [1, 2, 0, 1]
    f0 = np.array([100, 5, 200, 300, 0, 400, 1, 2], np.float32)
    n = np.array([1, 3, 1, 1, 1, 1, 2, np.nan], np.float32)
    rep = V.prosody_report(f0, n, d)
    assert rep.dtype == np.float32 and rep.shape == (4, 4)
    assert rep[0].tolist() == [100, 1, 2, 1]
    assert rep[1].tolist() == [300, 3, 1, 2]
    assert rep[2].tolist() == [0, 0, 0, 0] and not np.signbit(rep[2, 0])  # (no steps at all)
    assert rep[3, 0] == 0 and rep[3, 1] == 0 and np.isnan(rep[3, 2]) and rep[3, 3] == 1  # (none voiced: +0; a NaN in N stays)
    # float64 sums, rounded once: three values whose float32 running sum would round differently
    f = np.array([16777216, 11, 11, 11], np.float32)
    r2 = V.prosody_report(f, np.zeros(4, np.float32), [2])
    assert r2[0, 0] == np.float32((16777216.0 + 33) / 4) and r2[0, 1] == 4
    assert r2[0, 0] != (f[0] + f[1] + f[2] + f[3]) / np.float32(4)


def test_prosody_ok_in_numpy():
    assert V.prosody_ok() and V.prosody_ok(rate=[0.25, 4], frames=[0, 50], pitch=[0.25, 4], energy=[0, 4])
    for bad in (dict(rate=[0.2499]), dict(rate=[4.001]), dict(rate=[np.nan]), dict(frames=[-1]), dict(frames=[51]), dict(pitch=[0.0]),
                dict(pitch=[np.nan]), dict(energy=[-1e-9]), dict(energy=[4.5]), dict(energy=[np.nan]), dict(rate=[np.inf])):
        assert not V.prosody_ok(**bad), bad


# ---- the host rules and layout (HIP-free, under the sanitizers) -------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prosody_plan") / "prosody_plan_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "prosody_plan_check.cpp"), os.path.join(csrc, "host_request.cpp"),
                    "-o", exe], check=True)

    def run(*args):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


def test_prosody_ok_over_the_edges_of_every_range(driver):
    out = driver("rule")
    print(out)
    assert "rule: 42 single values" in out


_FORM_BYTES = {0: (0, 4), 1: (0, 8), 2: (0, 2), 3: (44, 4), 8: (0, 1), 9: (0, 1)}  # form -> (header, bytes per sample)
_RATE_LM = {0: (1, 1), 1: (1, 3), 2: (2, 3), 3: (2, 1)}


def _numpy_layout(lens, frames, cpr, words, marks, reports):
    """The packed buffer of a layout without joins, levels or FLAC, written out: bodies back to back, the marks block 8-aligned
    behind them, the report block 8-aligned behind that (only when some request that wants it has tokens)."""
    row, total, n_marks, n_report = 0, 0, 0, 0
    rep_first, rep_count = [], []
    for r, n in enumerate(cpr):
        L, M = _RATE_LM[words[r] >> 8]
        head, per = _FORM_BYTES[words[r] & 255]
        total += head + per * (600 * int(sum(frames[row: row + n])) * L // M)
        if marks[r]:
            n_marks += int(sum(lens[row: row + n])) + n
        count = 0
        for b in range(row, row + n):
            rep_first.append(n_report + count if reports[r] else -1)
            count += int(lens[b]) if reports[r] else 0
        n_report += count
        rep_count.append(count)
        row += n
    marks_off = (total + 7) & ~7
    fixed_end = marks_off + 8 * n_marks
    report_off = (fixed_end + 7) & ~7 if n_report else 0
    end = report_off + 16 * n_report if n_report else fixed_end
    return [total, marks_off, n_marks, fixed_end, report_off, n_report, end], rep_first, rep_count


def test_150_random_layouts_with_and_without_the_report_block(driver, tmp_path):
    """Mixed groupings, forms, rates, marks and report wishes: the plan's numbers equal the numpy layout; the driver itself checks
    that the plan of a layout nobody asks a report of is the parent's plan field for field, and the packed bound."""
    rng = np.random.default_rng(20251021)
    cases, lines = [], ["150"]
    for c in range(150):
        R = int(rng.integers(1, 6))
        cpr = rng.integers(1, 4, size=R)
        B = int(cpr.sum())
        lens = rng.integers(1, 40, size=B)
        lens[rng.integers(0, B)] = rng.choice([1, 512])
        frames = np.array([int(rng.integers(l, 6 * l + 1)) for l in lens])
        words = [int(rng.choice(list(_FORM_BYTES))) | (int(rng.integers(0, 4)) << 8) for _ in range(R)]
        marks = rng.integers(0, 2, size=R)
        reports = rng.integers(0, 2, size=R) if c % 5 else np.full(R, c % 2)  # (every fifth: all or none)
        cases.append((lens, frames, cpr, words, marks, reports))
        lines.append(f"{B} {R}")
        for arr in (lens, frames, cpr, words, marks, reports):
            lines.append(" ".join(str(int(v)) for v in arr))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = driver("plans", str(path))
    assert "plans: 150 layouts" in out
    got = [ln for ln in out.splitlines() if ln.startswith("case ")]
    assert len(got) == 150
    with_block = 0
    for c, (ln, case) in enumerate(zip(got, cases)):
        head, first, count = ln.split(":", 1)[1].split("|")
        want_head, want_first, want_count = _numpy_layout(*case)
        assert [int(v) for v in head.split()] == want_head, (c, ln)
        assert [int(v) for v in first.split()] == want_first, (c, ln)
        assert [int(v) for v in count.split()] == want_count, (c, ln)
        with_block += want_head[5] > 0
        assert want_head[4] % 8 == 0
    assert 60 < with_block < 150  # both kinds are there


def test_refusals_of_the_prosody_arguments(driver):
    got = dict(line.split("\t", 1) for line in driver("refusals").splitlines())
    assert got == {
        "null_out_report": "1\tinfer: null report argument",
        "null_out_n_report": "1\tinfer: null report argument",
        "report_without_requests": "1\tinfer: reports are for requests (chunks_per_request)",
        "bad_value": "1\tinfer: bad prosody",
        "ok": "accepted",
        "no_report": "accepted",
        "null_prosody": "accepted",
    }


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
ENTRIES = ("kx_infer_prosody", "kx_infer_requests_prosody", "kx_dispatcher_submit_request_prosody")
HOOKS = ("kx_test_prosody_durations", "kx_test_prosody_curves")


def _struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    return [re.findall(r"[A-Za-z_]\w*", d)[-1] for d in body.split(";") if d.strip()]


def test_header_ctypes_wrapper_and_rust_agree():
    from kokorox_amd import hip_koko as hk
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    test_header = open(os.path.join(ROOT, "include", "kokorox_hip_test.h"), encoding="utf-8").read()
    hpp = open(os.path.join(ROOT, "include", "kokorox_hip.hpp"), encoding="utf-8").read()
    rs = open(os.path.join(ROOT, "kokorox-hip", "src", "lib.rs"), encoding="utf-8").read()
    for name in ENTRIES:
        assert name in hk.ABI_SYMBOLS and re.search(r"^int %s\(" % name, header, re.M) and name not in test_header, name
        assert re.search(r"\bfn %s\(" % name, rs), name
    for name in HOOKS:
        assert name in hk.TEST_ABI_SYMBOLS and name not in hk.ABI_SYMBOLS and name not in header, name
        assert re.search(r"^int %s\(" % name, test_header, re.M), name
    # the struct: four pointers in the header's order, everywhere
    fields = _struct_fields(header, "kx_prosody")
    assert fields == ["rate", "frames", "pitch", "energy"]
    assert [n for n, _ in hk.Prosody._fields_] == fields and C.sizeof(hk.Prosody) == 4 * C.sizeof(C.c_void_p)
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct KxProsody \{(.*?)\}", rs, flags=re.S)
    assert m, "lib.rs lacks a #[repr(C)] KxProsody"
    assert re.findall(r"pub (\w+): \*const (\w+)", m.group(1)) == [("rate", "f32"), ("frames", "i32"), ("pitch", "f32"), ("energy", "f32")]
    assert re.search(r"#define KX_PROSODY_MAX_FRAMES 50\b", header) and "pub const KX_PROSODY_MAX_FRAMES: i32 = 50;" in rs
    assert V.PROSODY_MAX_FRAMES == 50
    assert "kx_infer_requests_prosody(" in hpp and "struct Prosody" in hpp and "const kx_prosody ps" in hpp
    # the refusal texts the GPU suite matches are the ones the header promises
    for text in ('"infer: bad prosody"', '"dispatcher_submit_request: bad prosody"', '"infer: null report argument"',
                 '"dispatcher_submit_request: null report argument"'):
        assert text in header, text


def test_header_restates_the_definition():
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    for phrase in ("0.25 <= rate <= 4, 0 <= frames <= 50, 0.25 <= pitch <= 4, 0 <= energy <= 4", "w = (1, 2, 3, 2, 1)", "/ 9.0",
                   "cl(i) = min(max(i, 0), 2 F_b - 1)", "0x41200001", "pred.F0.raw", "N'[j] = f32(f64(N[j]) * e[j])",
                   "pitch = target / measured", "Not offered"):
        assert phrase in header, phrase
