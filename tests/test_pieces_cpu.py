"""CPU: pieces (include/kokorox_hip.h, "pieces") -- a request delivered in several calls whose payloads join byte for byte.

Three layers, none of which needs a GPU: the numpy definition (kokorox_amd/voices.py: piece_ranges, piece_lengths, piece_bodies,
piece_carry) against the definition's own properties and against `levelled_body` of the request run whole; the host layout
(kokorox_amd/csrc/host_request.cpp: build_output_plan with pieces, output_bounds, check_piece_call; host_request.h: piece_refusal)
and the dispatcher's submit-time checks, built with g++ -fsanitize=address,undefined into tests/cpp/piece_plan_check.cpp and run as
a child process, against the numpy definition; and the ABI (header, Python table, C++ wrapper, lib.rs).
"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM = {0: (1, 1, 0), 1: (1, 3, 72), 2: (2, 3, 72), 3: (2, 1, 48)}  # rate code -> (L, M, C): n_taps = 2 C + 1 (resample_taps.h)
FORMS = (0, 1, 2, 3, 8, 9)
SAMPLE_BYTES = {0: 4, 1: 8, 2: 2, 3: 4, 8: 1, 9: 1}
HEAD, TAIL, INNER = 1, 2, 4


def _all_cuts(n):
    """Every way to cut n chunks into consecutive pieces: 2^(n - 1) lists of chunk counts."""
    out = []
    for mask in range(1 << (n - 1)):
        cuts, run = [], 1
        for i in range(n - 1):
            if mask >> i & 1:
                cuts.append(run)
                run = 1
            else:
                run += 1
        out.append(cuts + [run])
    return out


# ---- the numpy definition ---------------------------------------------------------------------------------------------------------
def test_the_table_of_filters_is_the_librarys():
    from kokorox_amd import hip_koko as hk
    for code, (L, M, C) in LM.items():
        l, m, taps = hk.resample_filter(code << 8)
        assert (l, m) == (L, M) and taps.shape[0] == (2 * C + 1 if code else 0)


@pytest.mark.parametrize("code", range(4))
def test_piece_ranges_on_random_splits(code):
    """1. E_k is non-decreasing and a multiple of 4, the last E_k is N, E_k <= F_k with F_k counted from the definition (every
    output whose window lies inside the data), and a one-piece request gives [0, N)."""
    from kokorox_amd import voices as V
    L, M, C = LM[code]
    rng = np.random.default_rng(7100 + code)
    for _ in range(300):
        n = int(rng.integers(1, 9))
        frames = rng.integers(1, 7, size=n)
        cuts = _all_cuts(n)[int(rng.integers(0, 1 << (n - 1)))]
        edges = np.concatenate([[0], np.cumsum(cuts)])
        lengths = [600 * int(frames[a:b].sum()) for a, b in zip(edges[:-1], edges[1:])]
        E = V.piece_ranges(lengths, code << 8)
        N = 600 * int(frames.sum()) * L // M
        assert len(E) == len(cuts) and E[-1] == N and all(e % 4 == 0 for e in E) and all(a <= b for a, b in zip([0] + E[:-1], E))
        A = np.cumsum(lengths)
        for k, e in enumerate(E[:-1]):
            final = [i for i in range(max(0, e - 8), min(N, e + 8)) if i * M + C <= int(A[k]) * L - 1]  # (around E_k: F_k is the count)
            F = final[-1] + 1 if final else 0
            assert e <= F < e + 4 or (code == 0 and e == int(A[k])), (code, lengths, k, e, F)
        assert V.piece_ranges([sum(lengths)], code << 8) == [N]


def test_piece_ranges_hold_nothing_back_at_24_khz_and_refuse_nonsense():
    from kokorox_amd import voices as V
    assert V.piece_ranges([600, 1200, 600], 0x003) == [600, 1800, 2400]
    assert V.piece_ranges([600, 1200, 600], 0x108) == [176, 576, 800]  # (F = 176 and 576: floor((A - 73) / 3) + 1)
    assert V.piece_ranges([24, 24, 600], 0x100) == [0, 0, 216]  # (pieces that emit nothing: 48 samples are inside the first window)
    with pytest.raises(ValueError):
        V.piece_ranges([], 0)
    with pytest.raises(ValueError):
        V.piece_ranges([600], 0x400)
    with pytest.raises(ValueError):
        V.piece_ranges([601], 0x100)


def _request(rng, frames):
    """Chunks of 3 tokens (pad, one token, pad) with these frame counts, the pads 0..2 frames, and noise for samples."""
    dur, chunks = [], []
    for f in frames:
        a = int(rng.integers(0, min(2, f - 1) + 1)) if f > 1 else 0
        b = int(rng.integers(0, min(2, f - 1 - a) + 1)) if f - a > 1 else 0
        dur.append([a, f - a - b, b])
        chunks.append(rng.standard_normal(600 * f).astype(np.float32) * np.float32(0.4))
    return chunks, dur


@pytest.mark.parametrize("code", range(4))
@pytest.mark.parametrize("form", FORMS)
def test_piece_bodies_concatenated_are_the_levelled_body(form, code):
    """2. For every form a piece may have x the four rates, every cut of 4 chunks, plain and joined, with and without a gain."""
    from kokorox_amd import voices as V
    rng = np.random.default_rng(7200 + 16 * form + code)
    chunks, dur = _request(rng, [1, 2, 1, 3])
    word = form | code << 8
    for join in (None, (HEAD | TAIL | INNER, 0, 10, 1)):
        for level in (None, (0, 0.5, 0.0)):
            whole = V.levelled_body(chunks, dur, word, join, level)
            for cuts in _all_cuts(4):
                parts = V.piece_bodies(chunks, dur, word, join, level, cuts)
                assert len(parts) == len(cuts) and b"".join(parts) == whole and all(len(p) % 4 == 0 for p in parts)
                E = V.piece_ranges(V.piece_lengths(dur, join, cuts), word)
                sizes = [SAMPLE_BYTES[form] * (b - a) for a, b in zip([0] + E[:-1], E)]
                sizes[0] += 44 if form == 3 else 0
                assert [len(p) for p in parts] == sizes


def test_piece_bodies_refuse_what_a_piece_cannot_carry():
    from kokorox_amd import voices as V
    rng = np.random.default_rng(5)
    chunks, dur = _request(rng, [1, 1])
    for form in (4, 12, 17, 18):
        with pytest.raises(ValueError, match="sized form"):
            V.piece_bodies(chunks, dur, form, None, None, [1, 1])
    for level in ((1, 1.0, 0.5), (2, 2.0, 0.5), (0x100, 0.5, 0.0)):
        with pytest.raises(ValueError, match="measured level"):
            V.piece_bodies(chunks, dur, 0, None, level, [1, 1])
    with pytest.raises(ValueError):
        V.piece_lengths(dur, None, [1, 2])


@pytest.mark.parametrize("code", range(4))
def test_piece_carry_holds_what_the_outputs_to_come_read(code):
    """The carry after piece k: A_k, E_k, the chunks so far, and a tail that is the end of the joined stream so far; with it and
    the later chunks alone the outputs from E_k on are those of the whole stream (the definition's loop, run on tail ++ rest)."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    L, M, C = LM[code]
    rng = np.random.default_rng(7300 + code)
    chunks, dur = _request(rng, [1, 1, 2, 1])
    join = (HEAD | TAIL | INNER, 0, 10, 1)
    word = code << 8
    x = V.join_stream(chunks, dur, join)
    y = V.resample_stream(x, word)
    for cuts in _all_cuts(4):
        c = V.piece_carry(chunks, dur, word, join, cuts)
        assert c.dtype == hk.PIECE_CARRY_DTYPE and c.shape == (len(cuts),)
        if len(cuts) == 1:
            assert c.tobytes() == bytes(c.nbytes)
            continue
        lengths = V.piece_lengths(dur, join, cuts)
        A, E = np.cumsum(lengths), V.piece_ranges(lengths, word)
        for k in range(len(cuts)):
            n_tail = 0 if code == 0 else min(hk.PIECE_TAIL, int(A[k]))
            assert (int(c[k]["magic"]), int(c[k]["format_word"]), int(c[k]["src_samples"]), int(c[k]["out_samples"]), int(c[k]["n_tail"]),
                    int(c[k]["reserved"])) == (hk.PIECE_MAGIC, word, int(A[k]), E[k], n_tail, sum(cuts[: k + 1]))
            assert c[k]["tail"][:n_tail].tobytes() == x[int(A[k]) - n_tail: int(A[k])].tobytes() and not c[k]["tail"][n_tail:].any()
            if code == 0 or k == len(cuts) - 1:
                continue
            # the outputs still to come read nothing before the tail: zero everything before it and they do not change
            z = x.copy()
            z[: int(A[k]) - n_tail] = 0
            assert V.resample_stream(z, word)[E[k]:].tobytes() == y[E[k]:].tobytes()


# ---- the host layout (HIP-free, under the sanitizers) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("piece_plan") / "piece_plan_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "piece_plan_check.cpp"), os.path.join(csrc, "host_request.cpp"),
                    "-lpthread", "-o", exe], check=True)

    def run(mode, text=""):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, mode], env=env, input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


def _plan_cases():
    """Batches of 1..3 requests, each a piece of a longer request (or one run whole), with what numpy says about them."""
    from kokorox_amd import voices as V
    rng = np.random.default_rng(7400)
    words = [f | c << 8 for f in FORMS for c in range(4)]
    joins = [(0, 0, 0, 0), (HEAD | TAIL | INNER, 0, 10, 1), (INNER, 10, 85, 0), (HEAD | TAIL, 0, 0, 12)]
    cases = []
    for i in range(120):
        R = int(rng.integers(1, 4))
        levelled = int(rng.integers(0, 2))
        reqs, text_rows = [], []
        for r in range(R):
            n = int(rng.integers(1, 6))
            dur = []
            for _ in range(n):
                T = int(rng.integers(1, 5))
                dur.append([int(v) for v in rng.integers(1, 4, size=T)])
            cuts = _all_cuts(n)[int(rng.integers(0, 1 << (n - 1)))]
            k = int(rng.integers(0, len(cuts)))
            word, join = words[int(rng.integers(0, len(words)))], joins[int(rng.integers(0, len(joins)))]
            if len(cuts) == 1:  # (a request run whole may have any form)
                word = [word, 0x104, 0x012][int(rng.integers(0, 3))]
            reqs.append(dict(dur=dur, cuts=cuts, k=k, word=word, join=join, want=int(rng.integers(0, 2))))
        cases.append((f"case{i}", levelled, reqs))
    # pieces that keep nothing, or less than a window: a row whose only token between the pads has no frame, trimmed at both ends
    # (48 samples with keep_ms 1, which its two fades of 1 ms fill), first, in the middle and last, at every rate
    thin = [[1, 1, 1], [1, 0, 1], [2, 1, 1]]
    for code in range(4):
        for k in range(3):
            cases.append((f"thin{code}{k}", k % 2, [dict(dur=thin, cuts=[1, 1, 1], k=k, word=8 | code << 8, join=(7, 0, 0, 0), want=1),
                                                    dict(dur=thin[1:] + thin[:1], cuts=[1, 1, 1], k=k, word=3 | code << 8, join=(7, 1, 0, 1), want=0),
                                                    dict(dur=thin, cuts=[1, 2], k=min(k, 1), word=2 | code << 8, join=(7, 0, 10, 0), want=1)]))
    text = []
    for name, levelled, reqs in cases:
        rows = []
        for q in reqs:
            a = sum(q["cuts"][: q["k"]])
            q["rows"] = q["dur"][a: a + q["cuts"][q["k"]]]
            q["chunks_before"] = a
            rows += q["rows"]
        lengths = [V.piece_lengths(q["dur"], q["join"], q["cuts"]) for q in reqs]
        line = [name, len(rows), len(reqs)] + [len(d) for d in rows] + [v for d in rows for v in d] + [len(q["rows"]) for q in reqs]
        line += [q["word"] for q in reqs] + [v for q in reqs for v in q["join"]] + [q["want"] for q in reqs] + [levelled]
        flags = [(1 if q["k"] == 0 else 0) | (2 if q["k"] == len(q["cuts"]) - 1 else 0) for q in reqs]
        line += flags
        for q, ln in zip(reqs, lengths):
            line += [sum(ln[: q["k"]]), max(q["chunks_before"], 1)]
        text.append(" ".join(str(v) for v in line))
        for q, ln, f in zip(reqs, lengths, flags):
            q["lengths"], q["flags"] = ln, f
    return cases, "\n".join(text) + "\n"


def test_plans_match_numpy(driver):
    """3. Offsets and sizes match numpy, the header appears only in FIRST pieces, the marks are the whole request's; and (inside
    the driver) a call without pieces gives the plan of the same call without flag words, field for field."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    cases, text = _plan_cases()
    out = driver("plans", text).split("\n")
    assert f"done {len(cases)}" in out
    at = 0
    n_pieces = n_empty = 0
    for name, levelled, reqs in cases:
        assert out[at] == f"case {name}", out[at]
        at += 1
        off = y_off = tails = 0
        pieces = any(q["flags"] != 3 for q in reqs)
        carry_off = None
        for r, q in enumerate(reqs):
            L, M, _ = LM[q["word"] >> 8]
            form, k = q["word"] & 0xFF, q["k"]
            E = [0] + V.piece_ranges(q["lengths"], q["word"])
            A = [0] + [int(v) for v in np.cumsum(q["lengths"])]
            n = E[k + 1] - E[k]
            if q["flags"] == 3:
                size = len(V.stream_body(np.zeros(n, np.float32), q["word"]))
                want_form = form
            else:
                size = SAMPLE_BYTES[form] * n + (44 if form == 3 and k == 0 else 0)
                want_form = 0 if form == 3 and k > 0 else form
                n_pieces += 1
                n_empty += n == 0
            marks = V.joined_marks(q["dur"], q["word"], q["join"])
            tok = [len(d) + 1 for d in q["dur"]]
            lo, hi = sum(tok[: q["chunks_before"]]), sum(tok[: q["chunks_before"] + len(q["rows"])])
            n_marks = hi - lo if q["want"] else 0
            rate = q["word"] >> 8
            assert out[at] == f"req {r} {off} {size} {n} {q['lengths'][k]} {want_form} {rate} {y_off if rate else 0} {n_marks}", (name, out[at])
            at += 1
            if pieces:
                f = out[at].split()
                assert f[:2] == ["piece", str(r)]
                emit_lo, emit_hi, src_before, src_end, n_in, n_out, c_off, chunks_end, flags = (int(v) for v in f[2:])
                if q["flags"] == 3:
                    assert (emit_lo, emit_hi, src_before, src_end, n_in, n_out, flags) == (0, n, 0, q["lengths"][0], 0, 0, 3)
                else:
                    want_in = 0 if rate == 0 or k == 0 else min(hk.PIECE_TAIL, A[k])
                    want_out = 0 if rate == 0 else min(hk.PIECE_TAIL, A[k + 1])
                    assert (emit_lo, emit_hi, src_before, src_end, n_in, n_out, flags) == (E[k], E[k + 1], A[k], A[k + 1], want_in, want_out, q["flags"])
                    if k > 0:
                        assert chunks_end == max(q["chunks_before"], 1) + len(q["rows"])
                    tails += n_in
                carry_off = c_off if r == 0 else carry_off
                assert c_off == carry_off + 1056 * r and c_off % 8 == 0
                at += 1
            if n_marks:
                got = [int(v) for v in out[at].split()[2:]]
                assert out[at].startswith(f"marks {r} ") and got == [int(v) for v in marks[lo:hi]], (name, out[at])
                at += 1
            off += size
            y_off += n if rate else 0
        f = out[at].split()
        assert f[0] == "sizes"
        total, end, y_floats, c_off, n_tail, bound, y_bound = (int(v) for v in f[1:])
        assert total == off and y_floats == y_off and n_tail == tails
        if pieces:
            assert c_off == carry_off and end == c_off + 1056 * len(reqs) and c_off >= total
        else:
            assert c_off == 0
        assert end <= bound and y_floats <= y_bound, name
        at += 1
    assert n_pieces >= 100 and n_empty >= 5  # (the four thin middles, and at 8 kHz the first piece of 48 samples)


def test_every_refusal_has_its_text(driver):
    """3. Every refusal of the semantics and of the carry, by the planner and by the entry's check alike, with its text; and what
    must pass passes: every allowed form x rate, a gain, a first piece with a carry that is rubbish, a whole request with anything."""
    lines = [ln.split("\t") for ln in driver("refusals").strip().split("\n")]
    got = {ln[0]: ln[1:] for ln in lines}
    want = {"level_normalize": "a piece cannot carry a measured level", "level_ceiling": "a piece cannot carry a measured level",
            "level_true_peak": "a piece cannot carry a measured level", "loudness": "a piece cannot carry loudness",
            "limiter": "a piece cannot carry a limiter", "form_4": "a piece cannot carry a sized form",
            "form_12": "a piece cannot carry a sized form", "form_17": "a piece cannot carry a sized form",
            "form_18": "a piece cannot carry a sized form", "flags_0_without_carry": "bad piece carry", "flags_4": "bad piece flags",
            "carry_magic": "bad piece carry", "carry_other_word": "bad piece carry", "carry_n_tail_257": "bad piece carry",
            "carry_n_tail_minus_1": "bad piece carry", "carry_n_tail_short": "bad piece carry", "carry_out_samples": "bad piece carry",
            "carry_src_negative": "bad piece carry", "carry_src_odd": "bad piece carry", "carry_no_chunks": "bad piece carry"}
    for who in ("plan_", "entry_"):
        for name, text in want.items():
            assert got[who + name] == ["1", "infer: " + text], (who + name, got[who + name])
        ok = [n for n in got if n.startswith(who + "ok_")]
        assert len(ok) == 6 + 24 and all(got[n] == ["accepted"] for n in ok), [n for n in ok if got[n] != ["accepted"]]
    assert got["entry_null_flags"] == ["1", "infer: null piece argument"] and got["entry_null_carry_out"] == ["1", "infer: null piece argument"]
    assert len(got) == 2 * (len(want) + 30) + 2


def test_dispatcher_checks_a_piece_when_it_is_submitted(driver):
    lines = [ln.split("\t") for ln in driver("dispatcher").strip().split("\n")]
    got = {ln[0]: ln[1:] for ln in lines}
    who = "dispatcher_submit_request: "
    assert got["ok_first"] == ["accepted", "flags=1 base=0 src=0 magic=0 levelled=0 piece=1 next_chunks=2"]
    assert got["ok_first_ignores_carry"] == ["accepted", "flags=1 base=0 src=0 magic=0 levelled=1 piece=1 next_chunks=2"]
    assert got["ok_middle"] == ["accepted", f"flags=0 base=3 src=2400 magic={0x4350584B} levelled=1 piece=1 next_chunks=5"]
    assert got["ok_last"] == ["accepted", f"flags=2 base=3 src=2400 magic={0x4350584B} levelled=0 piece=1 next_chunks=5"]
    assert got["ok_whole"] == ["accepted", "flags=3 base=0 src=0 magic=0 levelled=1 piece=0 next_chunks=2"]
    for name, text in (("null_carry_out", "null piece argument"), ("flags_4", "bad piece flags"), ("middle_without_carry", "bad piece carry"),
                       ("level_normalize", "a piece cannot carry a measured level"), ("bad_level", "bad level"),
                       ("form_12", "a piece cannot carry a sized form"), ("form_4", "a piece cannot carry a sized form"),
                       ("carry_magic", "bad piece carry"), ("carry_other_word", "bad piece carry"), ("carry_n_tail", "bad piece carry")):
        assert got[name] == ["1", who + text], (name, got[name])
    assert len(got) == 15


def test_the_carried_tail_suffices(driver):
    """4. For each rate, over all residues of A_k modulo 4 M (and every A in between), the smallest source index an output still to
    come reads is >= A_k - KX_PIECE_TAIL: the driver asserts it for every A and prints the worst reach, which is the bound
    (2 C + 3 M) / L of the header where a residue attains it, 153 at 8 kHz."""
    from kokorox_amd import hip_koko as hk
    got = [[int(v) for v in ln.split()[1:]] for ln in driver("tail").strip().split("\n")]
    assert [g[0] for g in got] == [1, 2, 3]
    for rate, worst, need, tail in got:
        L, M, C = LM[rate]
        assert tail == hk.PIECE_TAIL == 256 and need == -(-(2 * C + 3 * M) // L) and need - 1 <= worst <= need <= tail
    # the same in numpy, straight from the definition, for the residues alone
    for rate, (L, M, C) in LM.items():
        if rate == 0:
            continue
        for A in range(24 * 40, 24 * 40 + 24 * 4 * M + 1, 24):
            F = (A * L - 1 - C) // M + 1
            E = 4 * (F // 4)
            assert -((C - E * M) // L) >= A - hk.PIECE_TAIL  # ceil((E M - C) / L)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_python_cpp_and_rust_agree_on_pieces():
    from kokorox_amd import hip_koko as hk
    hdr = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    thdr = open(os.path.join(ROOT, "include", "kokorox_hip_test.h"), encoding="utf-8").read()
    hpp = open(os.path.join(ROOT, "include", "kokorox_hip.hpp"), encoding="utf-8").read()
    rs = open(os.path.join(ROOT, "kokorox-hip", "src", "lib.rs"), encoding="utf-8").read()
    for name, value in (("KX_PIECE_FIRST", "1u"), ("KX_PIECE_LAST", "2u"), ("KX_PIECE_TAIL", "256"), ("KX_PIECE_MAGIC", "0x4350584Bu")):
        assert re.search(rf"#define {name}\s+{value}\b", hdr), name
    assert (hk.PIECE_FIRST, hk.PIECE_LAST, hk.PIECE_WHOLE, hk.PIECE_TAIL, hk.PIECE_MAGIC) == (1, 2, 3, 256, 0x4350584B)
    m = re.search(r"typedef struct kx_piece_carry \{(.*?)\} kx_piece_carry;", hdr, flags=re.S)
    fields = re.findall(r"\b(\w+)(?:\[KX_PIECE_TAIL\])?;", m.group(1))
    assert fields == ["magic", "format_word", "src_samples", "out_samples", "n_tail", "reserved", "tail"] == list(hk.PIECE_CARRY_DTYPE.names)
    assert hk.PIECE_CARRY_DTYPE.itemsize == 1056 and hk.PIECE_CARRY_DTYPE.fields["tail"][1] == 32
    m = re.search(r"#\[repr\(C\)\][^{]*pub struct KxPieceCarry \{(.*?)\}", rs, flags=re.S)
    assert m and re.findall(r"pub (\w+):", m.group(1)) == fields
    assert "pub const KX_PIECE_FIRST: u32 = 1;" in rs and "pub const KX_PIECE_LAST: u32 = 2;" in rs and "pub const KX_PIECE_TAIL: usize = 256;" in rs
    for name in ("kx_infer_requests_pieces", "kx_dispatcher_submit_request_piece"):
        assert re.search(rf"\bint {name}\(", hdr) and re.search(rf"\bfn {name}\(", rs) and name in hk.ABI_SYMBOLS
    assert "kx_infer_requests_pieces(" in hpp and "using PieceCarry = kx_piece_carry;" in hpp
    assert re.search(r"\bint kx_test_output_plan_pieces\(", thdr) and "kx_test_output_plan_pieces" in hk.TEST_ABI_SYMBOLS
    for fn in ("infer_requests_pieces",):
        assert hasattr(hk.HipKoko, fn)
    assert hasattr(hk, "RequestStream") and "piece" in hk.Dispatcher.submit_request.__code__.co_varnames
    # the C++ wrapper compiles against the header, and the record has the size the three say
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                       input='#include "kokorox_hip.hpp"\nstatic_assert(sizeof(kokorox::PieceCarry) == 1056 && kokorox::PIECE_FIRST == 1 && '
                             'kokorox::PIECE_LAST == 2, "pieces");\n',
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
