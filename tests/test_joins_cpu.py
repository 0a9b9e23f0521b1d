"""CPU: joins -- a request's chunks trimmed at their pad spans, paused and faded (include/kokorox_hip.h, "joins").

Three layers, none of which needs a GPU: the numpy definition (kokorox_amd/voices.py: join_rows, join_stream, joined_marks)
against answers worked out by hand (tests/golden/joins.json); the host layout (kokorox_amd/csrc/host_request.cpp:
build_output_plan with joins and marks, output_bounds, check_spec_list) and the dispatcher's submit-time checks,
built with g++ -fsanitize=address,undefined into tests/cpp/join_plan_check.cpp and run as a child process, against the golden
answers and against the numpy definition on 200 seeded random cases; and the ABI (header, Python table, lib.rs).
"""
import json
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from kokorox_amd import voices as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "joins.json"), encoding="utf-8"))["cases"]
LM = {0: (1, 1), 1: (1, 3), 2: (2, 3), 3: (2, 1)}
HEAD, TAIL, INNER = 1, 2, 4


def _ramp(frames, seed):
    """Distinct samples per position, away from 0 so that a fade always changes them."""
    n = 600 * frames
    return (1.0 + seed + np.arange(n, dtype=np.float64) / 65536.0).astype(np.float32)


# ---- the numpy definition against the hand-derived answers -------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_mirror_gives_the_hand_derived_answers(case):
    d, join = case["durations"], case["join"]
    assert [len(x) for x in d] == case["lens"]
    assert [list(r) for r in V.join_rows(d, join)] == case["rows"]
    chunks = [_ramp(sum(x), c) for c, x in enumerate(d)]
    s = V.join_stream(chunks, d, join)
    assert s.dtype == np.float32 and s.shape[0] == case["S"] == sum(r[1] + r[2] for r in case["rows"])
    for code, want in case["rates"].items():
        word = int(code) << 8
        L, M = LM[int(code)]
        m = V.joined_marks(d, word, join)
        assert m.dtype == np.int64 and m.tolist() == want["marks"]
        assert int(m[-1]) == want["out_samples"] == case["S"] * L // M
        assert 44 + 4 * want["out_samples"] == want["out_bytes_3"]
        assert 4 * ((44 + 2 * want["out_samples"] + 2) // 3) == want["out_bytes_4"]


def test_worked_example_of_the_first_golden_case():
    """skip_0 = 1200 - 240, cut_0 = 600 - 240 (INNER), row 1 untouched (one token), skip_2 = 1800 - 240, no cut (no TAIL), 2040
    samples of pause; the kept samples are the right ones, the pauses are +0, the fades sit on the trimmed edges only."""
    case = GOLDEN[0]
    d, join = case["durations"], case["join"]
    chunks = [_ramp(sum(x), c) for c, x in enumerate(d)]
    s = V.join_stream(chunks, d, join)
    n = 24
    g = np.array([float(Fraction(2 * i + 1, 2 * n)) for i in range(n)])
    o = 0
    # chunk 0: x[960 .. 3240), faded at both ends
    assert s[o + n: o + 2280 - n].tobytes() == chunks[0][960 + n: 3240 - n].tobytes()
    assert s[o: o + n].tobytes() == (chunks[0][960: 960 + n].astype(np.float64) * g).astype(np.float32).tobytes()
    assert s[o + 2280 - n: o + 2280].tobytes() == (chunks[0][3240 - n: 3240].astype(np.float64) * g[::-1]).astype(np.float32).tobytes()
    o += 2280
    assert s[o: o + 2040].tobytes() == np.zeros(2040, np.float32).tobytes()
    o += 2040
    assert s[o: o + 2400].tobytes() == chunks[1][:2400].tobytes()  # the one-token chunk: whole, no fade
    o += 2400 + 2040
    # chunk 2: x[1560 .. 4200), faded at its head only (the request's tail is not trimmed)
    assert s[o: o + n].tobytes() == (chunks[2][1560: 1560 + n].astype(np.float64) * g).astype(np.float32).tobytes()
    assert s[o + n: o + 2640].tobytes() == chunks[2][1560 + n: 4200].tobytes()
    assert o + 2640 == s.shape[0]


def test_keep_longer_than_the_pad_cuts_nothing_and_still_fades():
    case = GOLDEN[1]
    x = _ramp(4, 0)
    s = V.join_stream([x], case["durations"], case["join"])
    assert s.shape[0] == 2400 and s[48: 2400 - 48].tobytes() == x[48: 2400 - 48].tobytes()
    assert (s[:48] < x[:48]).all() and (s[-48:] < x[-48:]).all()


# ---- properties of the definition ------------------------------------------------------------------------------------------
def _random_request(rng, n_chunks=None):
    n = int(rng.integers(1, 7)) if n_chunks is None else n_chunks
    return [[int(v) for v in rng.integers(1, 10, int(rng.integers(1, 7)))] for _ in range(n)]


def test_all_zero_spec_is_the_concatenation_and_token_marks():
    rng = np.random.default_rng(1)
    for _ in range(20):
        d = _random_request(rng)
        chunks = [_ramp(sum(x), c) for c, x in enumerate(d)]
        s = V.join_stream(chunks, d, (0, 0, 0, 0))
        assert s.tobytes() == np.concatenate(chunks).tobytes()
        for code in LM:
            assert V.joined_marks(d, code << 8, (0, 0, 0, 0)).tolist() == V.token_marks(d, code << 8).tolist()
            assert V.joined_marks(d, code << 8, None).tolist() == V.token_marks(d, code << 8).tolist()


def test_marks_are_multiples_of_24_non_decreasing_and_end_at_the_sample_count():
    rng = np.random.default_rng(2)
    for it in range(60):
        d = _random_request(rng)
        join = (int(rng.integers(0, 8)), int(rng.choice([0, 10, 30, 1000])), int(rng.choice([0, 1, 85, 200, 5000])),
                int(rng.choice([0, 1, 12])))
        rows = V.join_rows(d, join)
        S = sum(k + g for _, k, g, _, _ in rows)
        assert S % 24 == 0 and all(v % 24 == 0 for r in rows for v in r)
        assert all(k >= 600 or len(x) < 3 for x, (_, k, _, _, _) in zip(d, rows))  # (a trimmed row keeps its middle tokens)
        m24 = V.joined_marks(d, 0, join)
        assert (m24 % 24 == 0).all() and (np.diff(m24) >= 0).all() and int(m24[0]) == 0 and int(m24[-1]) == S
        for code, (L, M) in LM.items():
            m = V.joined_marks(d, code << 8, join)
            assert m.tolist() == [int(v) * L // M for v in m24] and all(int(v) * L % M == 0 for v in m24)
            assert int(m[-1]) == S * L // M
            o = 0
            for c, x in enumerate(d):  # the pause is what lies between a chunk's last mark and the next chunk's first
                if c + 1 < len(d):
                    assert int(m[o + len(x) + 1] - m[o + len(x)]) == 24 * join[2] * L // M
                o += len(x) + 1
        if it == 0:
            assert V.join_stream([_ramp(sum(x), c) for c, x in enumerate(d)], d, join).shape[0] == S


def test_fade_gains_match_float64_known_answers():
    """n = 24 and n = 288, i = 0 and i = n - 1: the gain is the correctly rounded float64 of (2 i + 1) / (2 n) (exact rational
    arithmetic here), the sample the correctly rounded float32 of the exact product with it."""
    assert float.fromhex("0x1.5555555555555p-6") == float(Fraction(1, 48))
    assert float.fromhex("0x1.c71c71c71c71cp-10") == float(Fraction(1, 576))
    x = np.float32(0.7310585975646973)
    for fade_ms, n in ((1, 24), (12, 288)):
        chunk = np.full(1800, x, dtype=np.float32)
        s = V.join_stream([chunk], [[1, 1, 1]], (HEAD | TAIL, 1000, 0, fade_ms))
        for i in (0, n - 1):
            gain = float(Fraction(2 * i + 1, 2 * n))                      # one float64 division
            prod = float(Fraction(float(x)) * Fraction(gain))            # one float64 product
            want = np.float32(prod)                                      # one round-to-nearest-even conversion
            assert s[i].tobytes() == want.tobytes() and s[1800 - 1 - i].tobytes() == want.tobytes(), (n, i)
        assert s[n].tobytes() == x.tobytes() and s[1800 - 1 - n].tobytes() == x.tobytes()
    nan = V.join_stream([np.full(1800, np.nan, np.float32)], [[1, 1, 1]], (HEAD, 0, 0, 12))
    assert np.isnan(nan).all()


def test_mirror_refuses_bad_specs():
    for bad in ((8, 0, 0, 0), (1, -1, 0, 0), (1, 1001, 0, 0), (0, 0, 5001, 0), (0, 0, -1, 0), (1, 0, 0, 13), (1, 0, 0, -1)):
        with pytest.raises(ValueError):
            V.join_rows([[1, 1, 1]], bad)
    with pytest.raises(ValueError):
        V.join_stream([np.zeros(599, np.float32)], [[1]], (0, 0, 0, 0))


# ---- the host layout (HIP-free, under the sanitizers) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("join_plan") / "join_plan_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "join_plan_check.cpp"), os.path.join(csrc, "host_request.cpp"),
                    "-lpthread", "-o", exe], check=True)

    def run(mode, text=""):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, mode], env=env, input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


def _case_text(name, durs, cpr, words, joins, want):
    flat = [name, len(durs), len(cpr)] + [len(d) for d in durs] + [v for d in durs for v in d] + list(cpr) + list(words)
    flat += [v for j in joins for v in j] + [int(w) for w in want]
    return " ".join(str(v) for v in flat) + "\n"


def _parse(out):
    cases, cur = {}, None
    for line in out.splitlines():
        kind, *rest = line.split()
        if kind == "case":
            cur = cases.setdefault(rest[0], {"row": [], "req": [], "marks": {}, "sizes": None})
        elif kind == "row":
            cur["row"].append([int(v) for v in rest[1:]])
        elif kind == "req":
            cur["req"].append([int(v) for v in rest[1:]])
        elif kind == "marks":
            cur["marks"][int(rest[0])] = [int(v) for v in rest[1:]]
        elif kind == "sizes":
            cur["sizes"] = [int(v) for v in rest]
    return cases


def _bytes_of(word, n):
    """Bytes of a region of n samples at the output rate in the form of `word` (include/kokorox_hip.h, KX_PACK_*)."""
    form = word & 0xFF
    return {0: 4 * n, 1: 8 * n, 2: 2 * n, 3: 44 + 4 * n, 4: 4 * ((44 + 2 * n + 2) // 3), 8: n, 9: n}[form]


def test_plan_builder_gives_the_hand_derived_answers(driver):
    text = ""
    for case in GOLDEN:
        for code in LM:
            for form in (3, 4):
                text += _case_text(f"{case['name']}.{code}.{form}", case["durations"], [len(case["lens"])], [form | code << 8],
                                   [case["join"]], [1])
    got = _parse(driver("plans", text))
    assert len(got) == len(GOLDEN) * 8
    for case in GOLDEN:
        for code in LM:
            want = case["rates"][str(code)]
            for form in (3, 4):
                g = got[f"{case['name']}.{code}.{form}"]
                assert g["row"] == case["rows"]
                (off, nbytes, n_samples, src, n_marks), = g["req"]
                assert (off, nbytes, n_samples, src) == (0, want[f"out_bytes_{form}"], want["out_samples"], case["S"])
                assert n_marks == sum(case["lens"]) + len(case["lens"]) and g["marks"][0] == want["marks"]
                assert g["sizes"][5] == 1


def test_plan_builder_equals_the_mirror_on_200_random_cases_and_the_bounds_hold(driver):
    """Rows 1..6, lens 1..6, durations 1..9, every flag set, mixed words, specs and want flags (a plain spec among them): the
    rows, every request's sizes and offsets, and the marks equal the numpy definition; the two bounds of
    output_bounds, taken over the un-joined samples plus the pauses, are upper bounds of what the plan lays out."""
    rng = np.random.default_rng(20240611)
    forms, cases, text = (0, 1, 2, 3, 4, 8, 9), {}, ""
    for i in range(200):
        B = int(rng.integers(1, 7))
        durs = _random_request(rng, B)
        cpr = []
        while sum(cpr) < B:
            cpr.append(int(rng.integers(1, B - sum(cpr) + 1)))
        R = len(cpr)
        words = [int(rng.choice(forms)) | int(rng.integers(0, 4)) << 8 for _ in range(R)]
        joins = [(i % 8 if r == 0 else int(rng.integers(0, 8)), int(rng.choice([0, 10, 30, 1000])),
                  int(rng.choice([0, 1, 85, 200, 5000])), int(rng.choice([0, 1, 12]))) if rng.random() > 0.15 else (0, 0, 0, 0)
                 for r in range(R)]
        want = [int(rng.integers(0, 2)) for _ in range(R)]
        cases[f"c{i}"] = (durs, cpr, words, joins, want)
        text += _case_text(f"c{i}", durs, cpr, words, joins, want)
    got = _parse(driver("plans", text))
    assert len(got) == 200
    seen_flags = set()
    for name, (durs, cpr, words, joins, want) in cases.items():
        g = got[name]
        row, off, y_floats = 0, 0, 0
        for r, n in enumerate(cpr):
            d = durs[row: row + n]
            seen_flags.add(joins[r][0])
            assert g["row"][row: row + n] == [list(v) for v in V.join_rows(d, joins[r])], (name, r)
            L, M = LM[words[r] >> 8]
            S = sum(k + gap for _, k, gap, _, _ in V.join_rows(d, joins[r]))
            n_out = S * L // M
            n_marks = sum(len(x) + 1 for x in d) if want[r] else 0
            assert g["req"][r] == [off, _bytes_of(words[r], n_out), n_out, S, n_marks], (name, r)
            assert g["marks"].get(r, []) == (V.joined_marks(d, words[r], joins[r]).tolist() if want[r] else []), (name, r)
            off += _bytes_of(words[r], n_out)
            y_floats += n_out if words[r] >> 8 else 0
            row += n
        total, end, yf, bound, y_bound, any_join = g["sizes"]
        assert total == off and end == ((off + 7) & ~7) + 8 * sum(len(g["marks"][r]) for r in g["marks"]) and yf == y_floats
        assert bound >= end and y_bound >= yf, name
        assert any_join == int(any(j != (0, 0, 0, 0) for j in joins))
    assert seen_flags == set(range(8))


def test_refusals_of_the_join_arguments(driver):
    got = dict(line.split("\t", 1) for line in driver("refusals").splitlines())
    bad = "1\tinfer: bad join"
    assert got == {
        "null_joins": "1\tinfer: null join argument",
        "n_join_0": "1\tinfer: bad join count", "n_join_2_of_3": "1\tinfer: bad join count",
        "flag_bit_8": bad, "keep_minus_1": bad, "keep_1001": bad, "pause_minus_1": bad, "pause_5001": bad, "fade_minus_1": bad,
        "fade_13": bad, "third_of_three_bad": bad,
        "one_marks_pointer_null": "1\tinfer: null marks argument",
        "ok_shared": "accepted", "ok_per_request_with_marks": "accepted",
    }


def test_dispatcher_checks_the_spec_at_submit_and_carries_it_to_the_batch(driver):
    got = dict(line.split("\t", 1) for line in driver("dispatcher").splitlines())
    bad = "1\tdispatcher_submit_request: bad join"
    null_marks = "1\tdispatcher_submit_request: null marks argument"
    assert got == {
        "null_join": bad, "flag_bit_8": bad, "keep_minus_1": bad, "keep_1001": bad, "pause_minus_1": bad, "pause_5001": bad,
        "fade_minus_1": bad, "fade_13": bad,
        "only_out_marks": null_marks, "only_out_n_marks": null_marks,
        "ok_no_marks": "accepted\t5 10 85 1 joined=1 marks=0 n_marks=0",
        "ok_marks": "accepted\t7 1000 5000 12 joined=1 marks=1 n_marks=1",
        "ok_plain_spec": "accepted\t0 0 0 0 joined=0 marks=1 n_marks=1",
    }


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_part_of_the_abi():
    from kokorox_amd import hip_koko as hk
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    test_header = open(os.path.join(ROOT, "include", "kokorox_hip_test.h"), encoding="utf-8").read()
    for name in ("kx_infer_requests_joined", "kx_dispatcher_submit_request_joined"):
        assert name in hk.ABI_SYMBOLS and re.search(r"^int %s\(" % name, header, re.M), name
        assert name not in test_header
    assert "kx_test_output_plan" in hk.TEST_ABI_SYMBOLS and "kx_test_output_plan" not in hk.ABI_SYMBOLS
    assert re.search(r"^int kx_test_output_plan\(", test_header, re.M) and "kx_test_output_plan" not in header
    for text in ("infer: null join argument", "infer: bad join count", "infer: bad join", "infer: null marks argument",
                 "dispatcher_submit_request: bad join", "dispatcher_submit_request: null marks argument"):
        assert '"%s"' % text in header, text
    assert (hk.JOIN_TRIM_HEAD, hk.JOIN_TRIM_TAIL, hk.JOIN_TRIM_INNER) == (1, 2, 4) == (V.JOIN_TRIM_HEAD, V.JOIN_TRIM_TAIL, V.JOIN_TRIM_INNER)
    for name, value in (("KX_JOIN_TRIM_HEAD", 1), ("KX_JOIN_TRIM_TAIL", 2), ("KX_JOIN_TRIM_INNER", 4)):
        assert re.search(r"^#define %s\s+%du\b" % (name, value), header, re.M), name
    assert hk.JOIN_DTYPE.itemsize == 16 and list(hk.JOIN_DTYPE.names) == ["flags", "keep_ms", "pause_ms", "fade_ms"]
    j = hk.join_specs((5, 10, 85, 1), 3)
    assert j.shape == (3,) and j.tobytes() == np.array([5, 10, 85, 1] * 3, dtype="<i4").tobytes()
    assert hk.join_specs([(1, 0, 0, 0), (0, 0, 0, 0)]).shape == (2,)


def test_header_restates_the_definition():
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    for phrase in ("typedef struct kx_join {", "skip = max(0, 600 d[0] - k)", "cut = max(0, 600 d[T-1] - k)", "keep = 600 F - skip - cut",
                   "gap = 24 pause_ms", "f32(f64(x) * (f64(2 i + 1) / f64(2 n)))", "A NaN stays a", "T >= 3",
                   "m_c[t] = (P_c + clamp(u - skip_c, 0, keep_c)) L / M", "S' = sum of (keep + gap)",
                   "A spec of all zeros gives the bytes and marks of kx_infer_requests_marks"):
        assert phrase in header, phrase


def test_rust_crate_binds_the_struct_and_both_entries():
    rs = open(os.path.join(ROOT, "kokorox-hip", "src", "lib.rs"), encoding="utf-8").read()
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct KxJoin \{(.*?)\}", rs, flags=re.S)
    assert m, "lib.rs lacks a #[repr(C)] KxJoin"
    fields = re.findall(r"pub (\w+): (\w+)", m.group(1))
    assert fields == [("flags", "u32"), ("keep_ms", "i32"), ("pause_ms", "i32"), ("fade_ms", "i32")]
    for name in ("kx_infer_requests_joined", "kx_dispatcher_submit_request_joined"):
        assert re.search(r"\bfn %s\s*\(" % name, rs), name
    for name, value in (("KX_JOIN_TRIM_HEAD", 1), ("KX_JOIN_TRIM_TAIL", 2), ("KX_JOIN_TRIM_INNER", 4)):
        assert re.search(r"pub const %s: u32 = %d;" % (name, value), rs), name
