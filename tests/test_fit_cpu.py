"""CPU: fit (include/kokorox_hip.h, "fit") -- the numpy definition voices.fit_durations against answers written out by hand and
against a brute-force walk of the floats around lambda, the host rule and the flat positions (kokorox_amd/csrc/host_request.{h,cpp}:
fit_ok, check_fit_call) through tests/cpp/fit_plan_check.cpp, built with g++ -fsanitize=address,undefined and run as a child
process (nothing is loaded into python), and the ABI (header, ctypes, C++ wrapper, lib.rs).
"""
import os
import re
import subprocess

import numpy as np
import pytest

from kokorox_amd import voices as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = 0x00800000, 0x7F7FFFFF


def f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


# ---- the numpy definition, by hand ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [1, 17, 50])
def test_one_token_takes_exactly_the_target(target):
    for w in (0.3, 1.0, 7.25, 2.0 ** 20, 2.0 ** -20, np.nan):
        d, lam, E = V.fit_durations(np.array([w], np.float32), target)
        assert d.dtype == np.int32 and d.tolist() == [target] and E == 0 and LO <= lam <= HI
        if target == 1:
            assert lam == LO  # (F(smallest lambda) = n already)
        else:  # lambda is the first float at which the token reaches the target
            assert V.fit_counts(V.fit_weights([w]), lam)[0] == target and V.fit_counts(V.fit_weights([w]), lam - 1)[0] == target - 1


def test_equal_weights_and_a_target_that_does_not_divide():
    # five tokens of weight 2, 13 frames: every token steps from 2 to 3 at the same lambda, F jumps from 10 to 15, E = 2, and the two
    # steppers with the highest position keep 2: the extra frames go to the lowest positions
    d, lam, E = V.fit_durations(np.full(5, 2.0, np.float32), 13)
    assert d.tolist() == [3, 3, 3, 2, 2] and E == 2
    # (2 lambda rounds to 3 from 2.5 on, half to even: the first float above 1.25)
    assert f32(lam) == np.nextafter(np.float32(1.25), np.float32(2)) and V.fit_counts(np.full(5, 2.0, np.float32), lam - 1).tolist() == [2] * 5
    # 7 tokens, 8 frames: one token at 2, the lowest position
    d, lam, E = V.fit_durations(np.ones(7, np.float32), 8)
    assert d.tolist() == [2, 1, 1, 1, 1, 1, 1] and E == 6
    # at n and at 50 n nothing is left to the tie rule
    d, lam, E = V.fit_durations(np.ones(7, np.float32), 7)
    assert d.tolist() == [1] * 7 and lam == LO and E == 0
    d, lam, E = V.fit_durations(np.ones(7, np.float32), 350)
    assert d.tolist() == [50] * 7 and E == 0 and f32(lam) == np.float32(49.5)  # (49.5 is even-rounded UP to 50: 49.5 -> 50)


def test_a_held_token_in_the_middle_keeps_its_count():
    w = np.array([2, 2, 9, 2, 2], np.float32)
    held = np.array([0, 0, 6, 0, 0])
    d, lam, E = V.fit_durations(w, 6 + 10, held)
    assert d.tolist() == [3, 3, 6, 2, 2] and E == 2 and int(d.sum()) == 16  # (G = 10 over four tokens of weight 2)
    # the held token's weight is no part of it: another weight there, the same answer
    w2 = w.copy()
    w2[2] = np.float32(np.nan)
    d2, lam2, E2 = V.fit_durations(w2, 16, held)
    assert d2.tolist() == d.tolist() and lam2 == lam and E2 == E
    for bad in (6 + 3, 6 + 201, 5):  # G < n, G > 50 n, G < 0
        with pytest.raises(ValueError):
            V.fit_durations(w, bad, held)
    with pytest.raises(ValueError):
        V.fit_durations(w[:1], 5, [5])  # no free token


def test_weights_are_clamped_and_a_nan_is_one():
    w = V.fit_weights([0.0, -3.0, 2.0 ** -21, 2.0 ** -20, 1.5, 2.0 ** 20, 2.0 ** 21, np.inf, -np.inf, np.nan])
    assert w.dtype == np.float32
    assert w.tolist() == [2.0 ** -20, 2.0 ** -20, 2.0 ** -20, 2.0 ** -20, 1.5, 2.0 ** 20, 2.0 ** 20, 2.0 ** 20, 2.0 ** -20, 1.0]
    assert V.fit_frames(2.4) == 96 and V.fit_frames(0.025) == 1 and V.fit_frames(1.0) == 40


# ---- the numpy definition on random spans ----------------------------------------------------------------------------------------
def _random_span(rng):
    n = int(rng.choice([1, 2, 3, int(rng.integers(1, 60)), int(rng.integers(1, 1301))]))
    kind = rng.integers(0, 4)
    if kind == 0:
        w = np.exp2(rng.uniform(-20, 20, size=n))
    elif kind == 1:
        w = rng.uniform(0.5, 12.0, size=n)  # (what a model gives)
    elif kind == 2:
        w = np.full(n, rng.uniform(0.5, 12.0))  # all equal: everything steps at once
    else:
        w = np.exp2(rng.integers(-20, 21, size=n).astype(np.float64))  # powers of two: many ties
    w = w.astype(np.float32)
    w[rng.random(n) < 0.05] = np.float32(np.nan)
    if n > 3 and rng.random() < 0.3:
        w[rng.integers(0, n)] = np.float32(2.0 ** 20)
        w[rng.integers(0, n)] = np.float32(2.0 ** -20)
    held = None
    if rng.random() < 0.4 and n > 1:
        held = np.where(rng.random(n) < 0.25, rng.integers(1, 51, size=n), 0)
        held[rng.integers(0, n)] = 0  # (a free token is left)
    n_free = n if held is None else int((held < 1).sum())
    phi = 0 if held is None else int(held.sum())
    G = int(rng.choice([n_free, 50 * n_free, int(rng.integers(n_free, 50 * n_free + 1))]))
    return w, phi + G, held, n_free, G


def test_300_random_spans():
    rng = np.random.default_rng(20261021)
    seen_excess = seen_nan = 0
    for case in range(300):
        w, frames, held, n, G = _random_span(rng)
        d, lam, E = V.fit_durations(w, frames, held)
        free = np.ones(w.shape[0], bool) if held is None else held < 1
        wf = V.fit_weights(w)[free]
        seen_nan += bool(np.isnan(w[free]).any())
        # the sum is exactly G, every d is in 1..50, held tokens keep their counts
        assert int(d.sum()) == frames and int(d[free].sum()) == G, case
        assert d[free].min() >= 1 and d[free].max() <= 50, case
        if held is not None:
            assert (d[~free] == held[~free]).all(), case
        # F(lambda-) < G <= F(lambda), and E is the excess
        F_hi = int(V.fit_counts(wf, lam).sum())
        assert G <= F_hi and E == F_hi - G, case
        if lam > LO:
            assert int(V.fit_counts(wf, lam - 1).sum()) < G, case
        else:
            assert E == 0, case
        seen_excess += E > 0
        # brute force around lambda: the first pattern at which F reaches G is lam, and the answer is d(lam) with the LAST E steppers
        # (by position) put back
        near = [u for u in range(max(LO, lam - 3), min(HI, lam + 3) + 1)]
        first = next(u for u in near if int(V.fit_counts(wf, u).sum()) >= G)
        assert first == lam, case
        want = V.fit_counts(wf, lam)
        if E:
            below = V.fit_counts(wf, lam - 1)
            assert ((want - below >= 0) & (want - below <= 1)).all(), case  # (no d moves by more than 1 between neighbours)
            left = E
            for t in range(wf.shape[0] - 1, -1, -1):
                if left and want[t] == below[t] + 1:
                    want[t] = below[t]
                    left -= 1
            assert left == 0, case
        assert (d[free] == want).all(), case
        # monotone in the weights: a larger weight never gets fewer frames, but for the tie rule's one frame at equal d(lambda)
        order = np.argsort(wf, kind="stable")
        dd = V.fit_counts(wf, lam)[order]
        assert (np.diff(dd) >= 0).all(), case
        got = d[free][order]
        assert (np.diff(got) >= -1).all(), case
    assert seen_excess >= 10 and seen_nan > 30  # (ties need equal weights: the all-equal and power-of-two kinds give them)


# ---- the host rule and the flat positions (HIP-free, under the sanitizers) --------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fit_plan") / "fit_plan_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "fit_plan_check.cpp"), os.path.join(csrc, "host_request.cpp"),
                    "-o", exe], check=True)

    def run(*args):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


def _numpy_fit_ok(lens, cpr, held, spans):
    """The rule written out: returns (prefix, flat spans) or None where the call is refused."""
    prefix = np.concatenate([[0], np.cumsum(lens)])
    first_row = np.concatenate([[0], np.cumsum(cpr)])
    flat, last_end = [], 0
    held_flat = np.concatenate([held[b, : lens[b]] for b in range(len(lens))])
    for i, (r, b, e, fr) in enumerate(spans):
        if r < 0 or r >= len(cpr) or b < 0 or b >= e:
            return None
        base = int(prefix[first_row[r]])
        if e > int(prefix[first_row[r + 1]]) - base:
            return None
        if i and base + b < last_end:
            return None
        h = held_flat[base + b: base + e]
        n, phi = int((h < 1).sum()), int(h[h >= 1].sum())
        if n == 0 or fr - phi < n or fr - phi > 50 * n:
            return None
        flat.append((base + b, base + e, fr))
        last_end = base + e
    return prefix.tolist(), flat


def test_150_random_multi_chunk_layouts(driver, tmp_path):
    rng = np.random.default_rng(20261022)
    cases, lines = [], ["150"]
    for c in range(150):
        R = int(rng.integers(1, 5))
        cpr = rng.integers(1, 4, size=R)
        B = int(cpr.sum())
        lens = rng.integers(1, 30, size=B)
        lens[rng.integers(0, B)] = rng.choice([1, 512])
        stride = int(lens.max()) + int(rng.integers(0, 3))
        held = np.where(rng.random((B, stride)) < 0.15, rng.integers(1, 51, size=(B, stride)), 0)
        first_row = np.concatenate([[0], np.cumsum(cpr)])
        tokens = [int(lens[first_row[r]: first_row[r + 1]].sum()) for r in range(R)]
        spans = []
        for r in range(R):
            at = 0
            while at < tokens[r] and rng.random() < 0.7:
                b = at + int(rng.integers(0, 4))
                e = b + 1 + int(rng.integers(0, max(1, tokens[r] - b))) if c % 3 else tokens[r]  # (every third: to the request's end)
                if e > tokens[r] or b >= e:
                    break
                base = int(lens[: first_row[r]].sum())
                h = np.concatenate([held[q, : lens[q]] for q in range(B)])[base + b: base + e]
                n, phi = int((h < 1).sum()), int(h[h >= 1].sum())
                if n == 0:
                    break
                spans.append((r, b, e, phi + int(rng.integers(n, 50 * n + 1))))
                at = e
        if c % 10 == 9 and spans:  # (some broken ones: the driver and numpy must refuse the same cases)
            k = int(rng.integers(0, len(spans)))
            r, b, e, fr = spans[k]
            spans[k] = [(r, b, e, 0), (r, e, b, fr), (R, b, e, fr), (r, b, tokens[r] + 1, fr)][int(rng.integers(0, 4))]
        cases.append((lens, cpr, held, spans))
        lines.append(f"{B} {R} {len(spans)} {stride}")
        lines.append(" ".join(str(int(v)) for v in lens))
        lines.append(" ".join(str(int(v)) for v in cpr))
        lines.append(" ".join(str(int(v)) for v in held.reshape(-1)))
        lines.append(" ".join(str(int(v)) for s in spans for v in s))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = driver("plans", str(path))
    assert "plans: 150 layouts" in out
    got = [ln for ln in out.splitlines() if ln.startswith("case ")]
    assert len(got) == 150
    accepted = crossing = 0
    for c, (ln, case) in enumerate(zip(got, cases)):
        ok, prefix, flat = ln.split(":", 1)[1].split("|")
        want = _numpy_fit_ok(*case)
        if not case[3]:  # (no spans: accepted, nothing planned)
            assert int(ok) == 1 and not prefix.split() and not flat.split(), (c, ln)
            continue
        assert int(ok) == (want is not None), (c, ln)
        if want is None:
            assert not prefix.split() and not flat.split(), (c, ln)
            continue
        accepted += 1
        assert [int(v) for v in prefix.split()] == want[0], (c, ln)
        f = [int(v) for v in flat.split()]
        assert [tuple(f[i: i + 3]) for i in range(0, len(f), 3)] == want[1], (c, ln)
        crossing += any(np.searchsorted(want[0], b, side="right") != np.searchsorted(want[0], e - 1, side="right") for b, e, _ in want[1])
    assert accepted > 80 and crossing > 30  # spans over several chunks are there


def test_every_refusal_of_the_fit(driver):
    got = dict(line.split("\t", 1) for line in driver("refusals").splitlines())
    bad = "1\tinfer: bad fit"
    assert got == {
        "ok": "accepted", "ok_at_50n": "accepted", "ok_second_request": "accepted", "two_sorted": "accepted", "two_touching": "accepted",
        "no_spans": "accepted",
        "request_negative": bad, "request_past_R": bad, "begin_negative": bad, "begin_equals_end": bad, "begin_after_end": bad,
        "end_past_tokens": bad, "end_past_tokens_second": bad, "no_free_token": bad, "below_n": bad, "above_50n": bad, "below_held": bad,
        "unsorted": bad, "overlapping": bad, "unsorted_by_request": bad, "null_spans": bad, "negative_count": bad,
    }


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
ENTRIES = ("kx_infer_requests_fitted", "kx_dispatcher_submit_request_fitted")
HOOKS = ("kx_test_fit_durations",)


def _struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    return [tuple(re.findall(r"[A-Za-z_]\w*", d)[-2:]) for d in body.split(";") if d.strip()]


def _entry_params(header, name):
    decl = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S).group(1)
    return [re.sub(r"\s+", " ", p).strip() for p in decl.split(",")]


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
    # the two structs: four 32-bit fields in the header's order, everywhere
    span = _struct_fields(header, "kx_fit_span")
    result = _struct_fields(header, "kx_fit_result")
    assert span == [("int32_t", "request"), ("int32_t", "begin"), ("int32_t", "end"), ("int32_t", "frames")]
    assert result == [("float", "lambda"), ("int32_t", "n_free"), ("int32_t", "held_frames"), ("int32_t", "excess")]
    np_kind = {"int32_t": np.dtype(np.int32), "float": np.dtype(np.float32)}
    for dt, fields in ((hk.FIT_SPAN_DTYPE, span), (hk.FIT_RESULT_DTYPE, result)):
        assert dt.itemsize == 16 and list(dt.names) == [n for _, n in fields]
        assert [dt.fields[n][0] for _, n in fields] == [np_kind[t] for t, _ in fields] and [dt.fields[n][1] for _, n in fields] == [0, 4, 8, 12]
    rs_kind = {"int32_t": "i32", "float": "f32"}
    for rs_name, fields in (("KxFitSpan", span), ("KxFitResult", result)):
        m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct %s \{(.*?)\}" % rs_name, rs, flags=re.S)
        assert m, "lib.rs lacks a #[repr(C)] " + rs_name
        assert re.findall(r"pub (\w+): (\w+)", m.group(1)) == [(n, rs_kind[t]) for t, n in fields]
    for cpp_name, fields in (("FitSpan", span), ("FitResult", result)):
        m = re.search(r"struct %s \{(.*?)\};" % cpp_name, hpp, flags=re.S)
        assert m and re.findall(r"\b(\w+)[,;]", m.group(1)) == [n for _, n in fields], cpp_name
    assert "kx_infer_requests_fitted(" in hpp and "sizeof(FitSpan) == sizeof(kx_fit_span)" in hpp
    # the two entries: the prosody entries' parameters, then spans, n_spans, out_fit (the dispatcher's err pair stays last)
    tail = ["const kx_fit_span* spans", "int n_spans", "kx_fit_result* out_fit"]
    assert _entry_params(header, "kx_infer_requests_fitted") == _entry_params(header, "kx_infer_requests_prosody") + tail
    pros = _entry_params(header, "kx_dispatcher_submit_request_prosody")
    assert _entry_params(header, "kx_dispatcher_submit_request_fitted") == pros[:-2] + tail + pros[-2:]
    for fn, n_more in (("kx_infer_requests_fitted", "kx_infer_requests_prosody"),
                       ("kx_dispatcher_submit_request_fitted", "kx_dispatcher_submit_request_prosody")):
        count = lambda f: len(re.search(r"\bfn %s\((.*?)\) -> c_int;" % f, rs, flags=re.S).group(1).split(","))
        assert count(fn) == count(n_more) + 3, fn
    # the refusal texts the GPU suite matches are the ones the header promises
    for text in ('"infer: bad fit"', '"dispatcher_submit_request: bad fit"', '"infer: fit with pinned durations"'):
        assert text in re.sub(r"\s*\n \*\s*", " ", header), text


def test_header_restates_the_definition():
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("0x00800000 .. 0x7F7FFFFF", "mid = lo + (hi - lo) / 2", "2^-20 <= s <= 2^20", "a NaN gives 1.0f",
                   "d_t(lambda) = min(max(rintf(f32(w_t * lambda)), 1), 50)", "the E with the highest token position keep d_t(lambda-)",
                   "At lo = 0x00800000, E is 0", "The sum is G exactly", "need not reproduce the un-fitted durations token for token",
                   "A join that trims pads afterwards shortens the body", "pred.dur.weights", "pred.dur.fitted", "Not offered"):
        assert phrase in flat, phrase
