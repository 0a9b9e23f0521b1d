"""CPU: FLAC bodies (include/kokorox_hip.h, "FLAC").  The numpy definition (kokorox_amd/voices.py: flac_body, flac_frame, flac_crc8,
flac_crc16) against a reader written from the format alone (tests/flac_reader.py: it never imports the encoder, verifies both CRCs
of every frame and the STREAMINFO fields) and against a slow brute-force minimum over (o, P, k); the planner, the bounds, the
refusals and the gap closing of the HIP-free host layout, built with g++ -fsanitize=address,undefined into
tests/cpp/flac_plan_check.cpp and run as a child process; and the ABI (header, Python table, lib.rs).
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from kokorox_amd import voices as V

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_reader as FR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RATES = (8000, 16000, 24000, 48000)


# ---- the streams ------------------------------------------------------------------------------------------------------------------
def _golden_streams():
    """The streams of the limiter's fixtures (float32 bit patterns: their inputs z and their limited z2, NaN and infinities among
    them) and the noise fixture, as 16-bit samples."""
    out = {}
    with open(os.path.join(GOLDEN, "limits.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    for c in cases:
        for key in ("z_bits", "z2_bits"):
            out[f"limits.{c['name']}.{key[:-5]}"] = V.pcm16(np.asarray(c[key], dtype=np.uint32).view(np.float32))
    out["limits.all"] = V.pcm16(np.concatenate([np.asarray(c["z_bits"], dtype=np.uint32).view(np.float32) for c in cases] * 3))
    with np.load(os.path.join(GOLDEN, "noise_stream.npz")) as z:
        noise = np.asarray(z["z"], dtype=np.float32).reshape(-1)
    out["noise.z"] = V.pcm16(noise)
    out["noise.quarter"] = V.pcm16(np.resize(noise, 9000) * np.float32(0.25))
    return out


def _streams():
    rng = np.random.default_rng(20260712)
    s = {}
    for n in range(1, 7):
        s[f"short_{n}"] = rng.integers(-2000, 2000, n)
    t = np.arange(10800)
    for N in (15, 16, 17, 4095, 4096, 4097, 8192, 10800):
        s[f"speechlike_{N}"] = (6000 * np.sin(t[:N] * 0.031) + 900 * np.sin(t[:N] * 0.47) + rng.integers(-40, 40, N)).astype(np.int64)
    for c in (0, 1, -32768):
        s[f"equal_{c}"] = np.full(5000, c)
    s["ramp"] = (t[:9000] * 7 - 31000).astype(np.int64)
    s["parabola"] = (t[:360] * (t[:360] - 360)).astype(np.int64)  # an exact quadratic: the second difference is 2, the third 0
    s["sine"] = np.round(30000 * np.sin(t * 0.013)).astype(np.int64)
    s["white_full_scale"] = rng.integers(-32768, 32768, 10800)
    s["alternating"] = np.where(t[:8200] % 2 == 0, 32767, -32767)
    s["alternating_full"] = np.where(t[:4096] % 2 == 0, 32767, -32768)
    s.update(_golden_streams())
    return s


STREAMS = _streams()


def test_the_fixture_streams_are_there():
    assert any(k.startswith("limits.") for k in STREAMS) and any(k.startswith("noise.") for k in STREAMS), sorted(STREAMS)


# ---- the CRCs ---------------------------------------------------------------------------------------------------------------------
def test_crc_check_values():
    assert V.flac_crc8(b"123456789") == 0xF4
    assert V.flac_crc16(b"123456789") == 0xFEE8
    assert V.flac_crc8(b"") == 0 and V.flac_crc16(b"") == 0
    # a CRC that starts at 0 ignores zeros in front, and is linear: what the GPU's per-lane partial CRCs rest on
    a, b = bytes(range(40, 90)), bytes(range(7, 57))
    assert V.flac_crc16(bytes(9) + a) == V.flac_crc16(a)
    assert V.flac_crc16(bytes(x ^ y for x, y in zip(a, b))) == V.flac_crc16(a) ^ V.flac_crc16(b)


# ---- round trips through the independent reader -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_round_trip_at_all_four_rates(name):
    v = np.asarray(STREAMS[name]).astype(np.int64)
    first = None
    for rate in RATES:
        body = V.flac_body(v, rate)
        got = FR.read_flac(body)
        assert got.samples == [int(x) for x in v], (name, rate)
        info = got.info
        assert (info["sample_rate"], info["channels"], info["bits_per_sample"], info["total_samples"]) == (rate, 1, 16, len(v))
        assert info["min_block"] == info["max_block"] == 4096 and info["md5"] == bytes(16)
        sizes = [f.n_bytes for f in got.frames]
        assert (info["min_frame"], info["max_frame"]) == (min(sizes), max(sizes))
        assert info["padding"] == (2 - sum(sizes)) % 4 and body[42] == 0x81
        assert len(got.frames) == -(-len(v) // 4096) and [f.number for f in got.frames] == list(range(len(got.frames)))
        assert len(body) % 4 == 0 and len(body) <= V.flac_bound(len(v)), (name, len(body), V.flac_bound(len(v)))
        assert all(f.n_bytes <= 16 + 2 * f.block_size for f in got.frames)
        # the reader reports the choice flac_frame says it made
        for i, f in enumerate(got.frames):
            kind, o, P, ks = V.flac_frame(v[4096 * i: 4096 * i + 4096], i, rate)[1]
            sub = f.subframes[0]
            assert (sub.kind, sub.order, sub.partition_order, sub.parameters) == (kind, o, P, tuple(ks)), (name, i)
        kinds = [f.subframes[0].kind for f in got.frames]
        first = kinds if first is None else first
        assert kinds == first  # (the rate is in the header alone)
    if name.startswith("equal_"):
        assert set(first) == {"CONSTANT"}
    if name == "white_full_scale":
        assert set(first) == {"VERBATIM"}
    if name == "parabola":  # (order 2 leaves a constant, order 3 zeros: one bit each)
        sub = FR.read_flac(V.flac_body(v, 24000)).frames[0].subframes[0]
        assert (sub.kind, sub.order, sub.parameters) == ("FIXED", 3, (0,))


def test_empty_stream_is_a_header_alone():
    body = V.flac_body(np.zeros(0, dtype=np.int16), 8000)
    assert len(body) == 48 and len(body) <= V.flac_bound(0)
    got = FR.read_flac(body)
    assert got.samples == [] and got.info["min_frame"] == got.info["max_frame"] == 0 and got.info["padding"] == 2


def test_the_reader_rejects_a_damaged_body():
    body = bytearray(V.flac_body(STREAMS["speechlike_4097"], 16000))
    for at in (60, len(body) - 3, 50):  # inside a frame, inside its CRC-16, inside the first frame's header
        bad = bytearray(body)
        bad[at] ^= 0x10
        with pytest.raises(FR.FlacError):
            FR.read_flac(bytes(bad))
    bad = bytearray(body)
    bad[12] ^= 1  # STREAMINFO's smallest frame
    with pytest.raises(FR.FlacError):
        FR.read_flac(bytes(bad))


# ---- the choice against a brute-force minimum -------------------------------------------------------------------------------------
def _brute(v):
    """(bits, o, P, ks) by exhaustive search in plain Python ints, ties as the header orders them."""
    v = [int(x) for x in v]
    n = len(v)
    coefs = ((1,), (1, -1), (1, -2, 1), (1, -3, 3, -1), (1, -4, 6, -4, 1))
    best = None
    for o in range(min(4, n - 1) + 1):
        e = [sum(c * v[i - j] for j, c in enumerate(coefs[o])) for i in range(o, n)]
        u = [2 * x if x >= 0 else -2 * x - 1 for x in e]
        for P in range(7 if n == 4096 else 1):
            size, lo, total, ks = n >> P, 0, 16 * o + 6, []
            for j in range(1 << P):
                hi = lo + size - (o if j == 0 else 0)
                costs = [sum(x >> k for x in u[lo:hi]) + (k + 1) * (hi - lo) for k in range(15)]
                k = min(range(15), key=lambda kk: (costs[kk], kk))
                ks.append(k)
                total += 4 + costs[k]
                lo = hi
            if best is None or (total, o, P) < (best[0], best[1], best[2]):
                best = (total, o, P, tuple(ks))
    return best


def _frame_bits(v, choice):
    kind, o, P, ks = choice
    assert kind == "FIXED"
    return _brute_bits_of(v, o, P, ks)


def _brute_bits_of(v, o, P, ks):
    v = [int(x) for x in v]
    n = len(v)
    coefs = ((1,), (1, -1), (1, -2, 1), (1, -3, 3, -1), (1, -4, 6, -4, 1))
    e = [sum(c * v[i - j] for j, c in enumerate(coefs[o])) for i in range(o, n)]
    u = [2 * x if x >= 0 else -2 * x - 1 for x in e]
    size, lo, total = n >> P, 0, 16 * o + 6
    for j, k in enumerate(ks):
        hi = lo + size - (o if j == 0 else 0)
        total += 4 + sum(x >> k for x in u[lo:hi]) + (k + 1) * (hi - lo)
        lo = hi
    return total


def test_choice_is_the_brute_force_minimum_on_random_frames():
    rng = np.random.default_rng(77)
    n_fixed = 0
    for case in range(240):
        full = case % 8 == 0  # (a full frame searches seven partition orders in plain Python: thirty of them)
        n = 4096 if full else int(rng.integers(2, 700))
        scale = float(rng.choice([3, 40, 700, 9000, 30000]))
        walk = np.cumsum(rng.normal(0, scale / 20, n)) if case % 3 else rng.normal(0, scale, n)
        if case % 5 == 0:  # a change of character inside the frame: partitions pay
            walk[n // 2:] = rng.normal(0, scale * 4, n - n // 2)
        v = np.clip(np.round(walk), -32768, 32767).astype(np.int64)
        if np.all(v == v[0]):
            continue
        frame, choice = V.flac_frame(v, 3, 24000)
        total, o, P, ks = _brute(v)
        if total >= 16 * n:
            assert choice[0] == "VERBATIM", case
            continue
        n_fixed += 1
        assert choice == ("FIXED", o, P, ks), (case, choice, (o, P, ks))
        assert _frame_bits(v, choice) == total
        head = 4 + 1 + (0 if n == 4096 else 2) + 1
        assert len(frame) == head + (8 + total + 7) // 8 + 2, case
    assert n_fixed >= 150


def _bits_table(v):
    """bits(o, P) of every pair the rules consider, from _brute_bits_of with the best parameters found one by one."""
    v = [int(x) for x in v]
    n, out = len(v), {}
    for o in range(min(4, n - 1) + 1):
        for P in range(7 if n == 4096 else 1):
            ks = []
            for j in range(1 << P):  # (partitions are independent: each one's parameter alone)
                costs = [_brute_bits_of(v, o, P, ks + [k] + [0] * ((1 << P) - j - 1)) for k in range(15)]
                ks.append(min(range(15), key=lambda kk: (costs[kk], kk)))
            out[(o, P)] = _brute_bits_of(v, o, P, ks)
    return out


def test_ties_fall_to_the_smaller_order_partition_and_parameter():
    # the parameter: residuals of 1 and 2 and no zero cost the same with k = 0 and k = 1
    u = np.asarray([1, 2, 2, 1, 1, 2, 1, 1] * 8, dtype=np.int64)
    assert sum(int(x) for x in u) + len(u) == sum(int(x) >> 1 for x in u) + 2 * len(u)
    assert V._flac_partitions(u, 0, 64, 0)[0] == [0]
    # the order: three short frames in which orders 1 and 2 cost the same and nothing costs less (judged at P = 0)
    for v in ([0, 1, 1, 1, 0, 0, 0, 1, 3, 6, 9, 11, 13], [-1, -3, -6, -8, -10, -13, -15, -17, -18, -20, -22, -23, -24, -26, -29],
              [-1, -2, -3, -4, -4, -5, -5, -5, -4, -3, -1, 1, 3, 4, 4, 3, 1, -1, -2, -3, -3, -4, -6, -7, -8, -10, -11, -11, -12, -12, -12, -13,
               -13, -12, -11, -9, -8, -8, -8, -7]):
        t = _bits_table(v)
        low = min(t.values())
        assert sorted(k for k, b in t.items() if b == low) == [(1, 0), (2, 0)] and low < 16 * len(v)
        assert V.flac_frame(v, 0, 8000)[1][:3] == ("FIXED", 1, 0)
    # the partition order: zeros, then a half in which 1026 residuals of -2 (u = 3) lie among 1022 zeros -- one partition with k = 0
    # costs what two with k = 0 and k = 1 cost, their second 4-bit parameter included
    v = np.zeros(4096, dtype=np.int64)
    v[2048 + np.round(np.linspace(0, 2047, 1026)).astype(int)] = -2
    table = {}
    for o in range(5):
        e = sum(c * v[o - j: 4096 - j] for j, c in enumerate(((1,), (1, -1), (1, -2, 1), (1, -3, 3, -1), (1, -4, 6, -4, 1))[o]))
        uu = np.where(e >= 0, 2 * e, -2 * e - 1)
        for P in range(7):
            size, lo, bits = 4096 >> P, 0, 16 * o + 6
            for j in range(1 << P):
                hi = lo + size - (o if j == 0 else 0)
                bits += 4 + min(int((uu[lo:hi] >> k).sum()) + (k + 1) * (hi - lo) for k in range(15))
                lo = hi
            table[(o, P)] = bits
    low = min(table.values())
    assert sorted(k for k, b in table.items() if b == low) == [(0, 0), (0, 1)]
    assert V.flac_frame(v, 0, 8000)[1] == ("FIXED", 0, 0, (0,))


# ---- the host layout (HIP-free, under the sanitizers) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flac_plan") / "flac_plan_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "flac_plan_check.cpp"),
                    os.path.join(csrc, "host_request.cpp"), "-lpthread", "-o", exe], check=True)

    def run(mode, text=""):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, mode], env=env, input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


def test_bound_is_the_formula_and_covers_every_body(driver):
    ns = [0, 1, 2, 15, 16, 17, 200, 4095, 4096, 4097, 8192, 10800, 1 << 20, (1 << 31) + 8]
    rows = [tuple(int(x) for x in line.split()) for line in driver("bounds", " ".join(str(n) for n in ns)).splitlines()]
    for (n, bound, frames), want in zip(rows, ns):
        assert n == want and frames == -(-n // 4096)
        assert bound == V.flac_bound(n) == (42 + 7 + sum(16 + 2 * min(4096, n - 4096 * f) for f in range(frames)) + 3) // 4 * 4 if n < 1 << 21 else bound == V.flac_bound(n)
        assert bound % 4 == 0
    for name, v in STREAMS.items():
        assert len(V.flac_body(v, 48000)) <= V.flac_bound(len(v)), name


_LM = {0: (1, 1), 1: (1, 3), 2: (2, 3), 3: (2, 1)}


def _numpy_layout(frames, lens, cpr, words, want, kinds):
    """The plan of a layout without joins, from the header's text: regions, blocks, the packer's grid and the FLAC tables."""
    R, row, off = len(cpr), 0, 0
    reqs, slots, n_marks, units, longest = [], 0, 0, 0, 0
    for r in range(R):
        form, rate = words[r] & 0xFF, words[r] >> 8
        S = 600 * int(sum(frames[row: row + cpr[r]]))
        L, M = _LM[rate]
        n = S * L // M
        size = {0: 4 * n, 1: 8 * n, 2: 2 * n, 3: 44 + 4 * n, 4: 4 * ((44 + 2 * n + 2) // 3), 8: n, 9: n, 12: V.flac_bound(n)}[form]
        flac = form == 12
        reqs.append((r, form, rate, off, size, n, 0 if flac else off, 0 if flac else size, -(-n // 4096) if flac else -1, slots))
        if flac:
            slots += -(-n // 4096)
        else:
            units = max(units, ((off & 15) + size + 15) // 16)
        if want[r]:
            n_marks += int(sum(lens[row: row + cpr[r]])) + cpr[r]
        off += size
        row += cpr[r]
        longest = max(longest, n)
    any_flac = any(q[1] == 12 for q in reqs)
    marks_off = (off + 7) & ~7
    limited, loud = any(k == 3 for k in kinds), any(k in (2, 3) for k in kinds)
    measured = loud or any(k == 1 for k in kinds)
    levels_off = (marks_off + 8 * n_marks + 7) & ~7 if measured else 0
    loud_off = levels_off + 16 * R if loud else 0
    limits_off = loud_off + 16 * R if limited else 0
    end = limits_off + 40 * R if limited else (loud_off + 16 * R if loud else (levels_off + 16 * R if measured else marks_off + 8 * n_marks))
    flac_off = (end + 7) & ~7 if any_flac else 0
    if not any_flac:
        reqs = [q[:8] + (-1, 0) for q in reqs]
    frames_of = [q[8] for q in reqs if q[8] >= 0]
    sizes = (off, units, marks_off, n_marks, levels_off, loud_off, limits_off, flac_off, flac_off + 8 * R if any_flac else end,
             slots, max(frames_of, default=0), max((q[4] for q in reqs if q[1] == 12), default=0))
    return reqs, sizes


def test_random_layouts_against_a_numpy_layout(driver):
    rng = np.random.default_rng(4242)
    cases, text = [], []
    forms = [0, 1, 2, 3, 4, 8, 9, 12, 12, 12]
    for c in range(165):  # 150 that mix form 12 with the others, and 15 without it
        R = int(rng.integers(1, 7))
        cpr = [int(x) for x in rng.integers(1, 4, R)]
        B = sum(cpr)
        frames = [int(x) for x in rng.choice([0, 1, 2, 7, 9, 14, 41], B)]
        lens = [int(x) for x in rng.integers(3, 40, B)]
        words = [int(rng.choice(forms)) | (int(rng.integers(0, 4)) << 8) for _ in range(R)]
        if c >= 150:
            words = [w if w & 0xFF != 12 else (w & ~0xFF) | 3 for w in words]
        elif all(w & 0xFF != 12 for w in words):
            words[int(rng.integers(0, R))] = 12 | (int(rng.integers(0, 4)) << 8)
        want = [int(x) for x in rng.integers(0, 2, R)] if c % 3 else [0] * R
        kinds = [int(x) for x in rng.integers(0, 4, R)] if c % 2 else [0] * R
        cases.append((frames, lens, cpr, words, want, kinds))
        text.append(f"c{c} {B} {R}\n" + " ".join(map(str, frames + lens + cpr + words + want + kinds)))
    out = driver("plans", "\n".join(text) + "\n")
    assert "FAILED" not in out, out[-2000:]
    blocks = out.split("case ")[1:]
    assert len(blocks) == len(cases)
    n_flac = 0
    for block, (frames, lens, cpr, words, want, kinds) in zip(blocks, cases):
        lines = block.splitlines()
        reqs = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("req ")]
        sizes = tuple(int(x) for x in next(ln for ln in lines if ln.startswith("sizes ")).split()[1:])
        bounds = tuple(int(x) for x in next(ln for ln in lines if ln.startswith("bounds ")).split()[1:])
        want_reqs, want_sizes = _numpy_layout(frames, lens, cpr, words, want, kinds)
        assert reqs == want_reqs, lines[0]
        assert sizes == want_sizes, (lines[0], sizes, want_sizes)
        assert all(q[3] % 4 == 0 and q[4] % 4 == 0 for q in reqs) and sizes[7] % 8 == 0
        assert bounds[0] >= sizes[8] and bounds[1] >= sizes[9]
        n_flac += any(w & 0xFF == 12 for w in words)
    assert n_flac == 150


def test_refusals_are_unchanged_and_ten_and_eleven_stay_refused(driver):
    got = dict(line.split("\t", 1) for line in driver("refusals").splitlines())
    for form in (5, 6, 7, 10, 11, 13, 14, 15, 16, 128, 255):
        assert got[f"form_{form}"] == "1\tinfer: unknown output format", form
    for rate in range(4):
        assert got[f"flac_rate_{rate}"] == "accepted"
    for rate in (4, 5):
        assert got[f"flac_rate_{rate}"] == "1\tinfer: unknown output sample rate"
    assert got["flac_stray_bit"] == got["flac_negative"] == "1\tinfer: unknown output format"
    assert got["per_utterance_format_2"] == "accepted"
    assert got["per_utterance_format_12"] == got[f"per_utterance_format_{12 | 0x100}"] == "1\tinfer: unknown output format"
    assert got["request_format_flac_48000"] == "accepted"


def test_gap_closing_on_hand_made_lengths(driver):
    cases = {
        "alone": [(12, 1000, 512)],
        "alone_full": [(12, 1000, 1000)],
        "alone_empty_body": [(12, 52, 48)],
        "first": [(12, 8300, 4100), (2, 2400, 2400), (4, 3260, 3260)],
        "last": [(0, 4800, 4800), (8, 1200, 1200), (12, 21680, 9000)],
        "middle_and_both_ends": [(12, 800, 60), (3, 2444, 2444), (12, 16500, 16496), (9, 600, 600), (12, 2500, 48)],
        "neighbours": [(12, 900, 400), (12, 900, 900), (12, 900, 0), (12, 900, 896)],
        "no_flac": [(2, 2400, 2400), (3, 2444, 2444)],
        "bad_above_its_region": [(12, 1000, 1004)],
        "bad_not_a_multiple_of_four": [(12, 1000, 510)],
        "bad_negative": [(2, 400, 400), (12, 1000, -4)],
        "bad_other_form_shrinks": [(12, 1000, 400), (2, 400, 396)],
    }
    text = "\n".join(f"{name} {len(rows)}\n" + " ".join(f"{a} {b} {c}" for a, b, c in rows) for name, rows in cases.items()) + "\n"
    out = driver("gaps", text)
    assert "FAILED" not in out, out
    got = {ln.split()[1]: ln.split()[2:] for ln in out.splitlines()}
    assert set(got) == set(cases)
    for name, rows in cases.items():
        if name.startswith("bad_"):
            assert got[name] == ["refused", "flac:", "bad", "length"], (name, got[name])
        else:
            lengths = [c for _, _, c in rows]
            assert got[name] == ["total", str(sum(lengths)), "bytes"] + [str(x) for x in lengths], (name, got[name])


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_constant_in_header_python_and_rust():
    from kokorox_amd import hip_koko as hk
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    test_header = open(os.path.join(ROOT, "include", "kokorox_hip_test.h"), encoding="utf-8").read()
    rs = open(os.path.join(ROOT, "kokorox-hip", "src", "lib.rs"), encoding="utf-8").read()
    hpp = open(os.path.join(ROOT, "include", "kokorox_hip.hpp"), encoding="utf-8").read()
    assert re.search(r"^#define KX_PACK_FLAC 12$", header, re.M) and hk.PACK_FLAC == 12 and V.FLAC_BLOCK == 4096
    assert re.search(r"pub const KX_PACK_FLAC: c_int = 12;", rs) and "PACK_FLAC = KX_PACK_FLAC" in hpp
    assert "kx_test_output_plan_flac" in test_header and "kx_test_output_plan_flac" in hk.TEST_ABI_SYMBOLS
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], text=True, capture_output=True,
                       input='#include "kokorox_hip.h"\nstatic_assert(KX_PACK_FLAC == 12 && KX_FLAC_BLOCK == 4096, "");\n')
    assert r.returncode == 0, r.stderr


def test_every_mirror_takes_the_form():
    rng = np.random.default_rng(9)
    x = (0.3 * np.sin(np.arange(1800) * 0.05) + 0.01 * rng.standard_normal(1800)).astype(np.float32)
    x[100] = np.nan
    x[200], x[201] = np.inf, -np.inf
    for word in (12, 12 | 0x100, 12 | 0x200, 12 | 0x300):
        rate = {0: 24000, 1: 8000, 2: 16000, 3: 48000}[word >> 8]
        y = x if word == 12 else x[: 600 * {1: 1, 2: 2, 3: 3}[word >> 8]]  # (stream_body takes the stream at the word's rate)
        body = V.stream_body(y, word)
        got = FR.read_flac(body)
        assert got.info["sample_rate"] == rate and got.samples == [int(s) for s in V.pcm16(y)]
    pcm = V.pcm16(x)
    assert pcm[100] == 0 and pcm[200] == 32767 and pcm[201] == -32767
    chunks, durs = [x[:1200], x[1200:1800]], [[1, 1], [1]]
    assert FR.read_flac(V.levelled_body(chunks, durs, 12, None, (1, 1.0, 0.5))).info["total_samples"] == 1800
    assert FR.read_flac(V.loudness_body(x[:1800], 0.5, 12 | 0x300)).info["sample_rate"] == 48000
    assert FR.read_flac(V.limited_body(chunks, durs, 12, None, (0, 2.0, 0.0, 0.25))).info["total_samples"] == 1800
