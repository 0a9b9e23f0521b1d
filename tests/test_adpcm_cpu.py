"""CPU: IMA ADPCM WAV bodies and 16-bit WAV bodies (include/kokorox_hip.h, "IMA ADPCM"; forms 17 and 18).  The numpy definition
(kokorox_amd/voices.py: adpcm_blocks, adpcm_wav_body, adpcm_wav_decode, wav16_body) against CPython's audioop run block by block from
every block's header state (where the module exists) and against committed answers (tests/golden/adpcm_known_answers.json, where it
does not); the header field by field; the planner, the sizes and the refusals of the HIP-free host layout, built with
g++ -fsanitize=address,undefined into tests/cpp/adpcm_plan_check.cpp and run as a child process; the cost of the block-independent
start index against audioop's sequential encoder; and the ABI (header, Python table, C++ wrapper, lib.rs, the step table's generator).
"""
import base64
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
RATES = (8000, 16000, 24000, 48000)
CODE = {24000: 0, 8000: 1, 16000: 2, 48000: 3}
BLOCK = {8000: 256, 16000: 512, 24000: 512, 48000: 1024}
ADPCM, WAV16, B64 = 17, 18, 4


def _p(rate):
    return 1 + 2 * (BLOCK[rate] - 4)


def _noise():
    with np.load(os.path.join(GOLDEN, "noise_stream.npz")) as z:
        return np.asarray(z["z"], dtype=np.float32).reshape(-1)


def _streams(n):
    """The issue's list as 16-bit samples: ramps, silence, a full-scale square wave (the predictor's clamp, the index pinned at 88),
    16-bit noise; and the noise fixture."""
    rng = np.random.default_rng(1711)
    t = np.arange(n)
    return {
        "ramp_up": np.clip(t * 37 - 32768, -32768, 32767).astype(np.int16),
        "ramp_down": np.clip(32767 - t * 3, -32768, 32767).astype(np.int16),
        "silence": np.zeros(n, dtype=np.int16),
        "square_full_scale": np.where((t // 5) % 2 == 0, 32767, -32767).astype(np.int16),
        "square_every_sample": np.where(t % 2 == 0, 32767, -32768).astype(np.int16),
        "noise_16_bit": rng.integers(-32768, 32768, n).astype(np.int16),
        "noise_quiet": rng.integers(-300, 300, n).astype(np.int16),
        "noise_fixture": V.pcm16(np.resize(_noise(), n) * np.float32(0.25)),
    }


def _padded(v, rate):
    P = _p(rate)
    F = -(-v.shape[0] // P)
    return np.concatenate([v, np.full(F * P - v.shape[0], v[-1], dtype=v.dtype)]).reshape(F, P)


def _swap(b):
    b = np.asarray(b, dtype=np.uint8)
    return ((b >> 4) | (b << 4)).astype(np.uint8)


# ---- the encoder core and the decoder against audioop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 24000, 48000])
def test_blocks_equal_audioop_from_every_header_state(rate):
    """Every block's codes are audioop.lin2adpcm of its samples 1 .. P - 1 from the state (predictor, index) its header holds, with the
    nibbles swapped (audioop puts the earlier sample in the high nibble); the header's predictor is the first sample and its index the
    start rule's (the smallest index whose step reaches the largest of the block's first eight differences); audioop.adpcm2lin from that state is what adpcm_wav_decode returns."""
    audioop = pytest.importorskip("audioop")
    P = _p(rate)
    steps = V.adpcm_steps()
    for name, v in _streams(2 * P + 17).items():
        x = _padded(v, rate)
        blocks = V.adpcm_blocks(v, rate)
        assert blocks.shape == (3, BLOCK[rate]) and blocks.dtype == np.uint8
        decoded, got_rate = V.adpcm_wav_decode(V.adpcm_wav_body(v, rate))
        assert got_rate == rate and decoded.dtype == np.int16 and decoded.shape == v.shape
        for f in range(3):
            pred, i0 = int(x[f, 0]), int(blocks[f, 2])
            d = max(abs(int(x[f, t + 1]) - int(x[f, t])) for t in range(8))
            assert struct.unpack("<h", blocks[f, 0:2].tobytes())[0] == pred and blocks[f, 3] == 0, (name, f)
            assert i0 == next((i for i in range(89) if steps[i] >= d), 88), (name, f)
            code, (last, index) = audioop.lin2adpcm(x[f, 1:].astype("<i2").tobytes(), 2, (pred, i0))
            assert _swap(np.frombuffer(code, dtype=np.uint8)).tobytes() == blocks[f, 4:].tobytes(), (name, f)
            lin, _ = audioop.adpcm2lin(_swap(blocks[f, 4:]).tobytes(), 2, (pred, i0))
            want = np.concatenate([[pred], np.frombuffer(lin, dtype="<i2")])[: v.shape[0] - f * P]
            assert np.array_equal(decoded[f * P: (f + 1) * P], want), (name, f)
            if name == "square_every_sample" and f < 2:  # (a full-scale step every sample: the index ends pinned at its upper clamp)
                assert index == 88 and abs(last) >= 32767 - 4


def test_clamps_are_reached():
    """A full-scale square wave that holds each level for five samples drives the predictor into both ends of the 16-bit range (at
    32767 with the largest step, the code 0 still moves it by step / 8 = 4095: clamped); one that steps every sample starts at index
    88; silence starts at index 0 and every code is 0."""
    d, _ = V.adpcm_wav_decode(V.adpcm_wav_body(_streams(505)["square_full_scale"], 8000))
    assert d.max() == 32767 and d.min() == -32768
    assert V.adpcm_blocks(_streams(505)["square_every_sample"], 8000)[0, 2] == 88  # a difference of 65535 is above every step
    z = V.adpcm_blocks(np.zeros(505, dtype=np.int16), 8000)
    assert not z.any()
    one = V.adpcm_blocks(np.array([-7], dtype=np.int16), 8000)  # a single sample: the predictor, and a block of repeats of it
    assert one.shape == (1, 256) and struct.unpack("<h", one[0, :2].tobytes())[0] == -7 and not one[0, 2:].any()


def test_known_answers():
    """The committed answers (made where audioop exists, and checked against it there by the test above): the check survives a Python
    without the module."""
    with open(os.path.join(GOLDEN, "adpcm_known_answers.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 4 and {c["rate"] for c in cases} >= {8000, 24000, 48000}
    for c in cases:
        v = np.asarray(c["v"], dtype=np.int16)
        body = V.adpcm_wav_body(v, c["rate"])
        assert body.hex() == c["body_hex"], c["name"]
        d, rate = V.adpcm_wav_decode(body)
        assert rate == c["rate"] and [int(s) for s in d] == c["decoded"], c["name"]


# ---- the header ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_header_field_by_field(rate):
    A, P = BLOCK[rate], _p(rate)
    rng = np.random.default_rng(rate)
    for N in (1, P - 1, P, P + 1, 0):
        v = rng.integers(-9000, 9000, N).astype(np.int16)
        body = V.adpcm_wav_body(v, rate)
        F = -(-N // P)
        assert len(body) == 60 + A * F and len(body) % 4 == 0
        assert body[0:4] == b"RIFF" and struct.unpack("<I", body[4:8])[0] == 52 + A * F == len(body) - 8 and body[8:12] == b"WAVE"
        assert body[12:16] == b"fmt " and struct.unpack("<I", body[16:20])[0] == 20
        tag, ch, hz, bps, align, bits, cb, spb = struct.unpack("<HHIIHHHH", body[20:40])
        assert (tag, ch, hz, bps, align, bits, cb, spb) == (0x0011, 1, rate, rate * A // P, A, 4, 2, P)
        assert body[40:44] == b"fact" and struct.unpack("<II", body[44:52]) == (4, N)
        assert body[52:56] == b"data" and struct.unpack("<I", body[56:60])[0] == A * F
        d, got = V.adpcm_wav_decode(body)
        assert got == rate and d.shape == (N,)
        if N:
            assert d[0] == v[0]
            # the tail of the last block repeats v[N - 1]: the body equals that of the stream written out to a whole block
            whole = np.concatenate([v, np.full(F * P - N, v[-1], dtype=np.int16)])
            assert V.adpcm_wav_body(whole, rate)[60:] == body[60:]
    with pytest.raises(ValueError):
        V.adpcm_wav_decode(body[:-1])
    with pytest.raises(ValueError):
        V.adpcm_wav_decode(body[:20] + b"\x01\x00" + body[22:])  # (a PCM tag)


def test_forty_blocks_exactly_at_8_khz():
    """101 frames of 200 samples at 8 kHz are 20 200 = 40 x 505 samples: 40 blocks and no padding."""
    v = _streams(20200)["noise_fixture"]
    body = V.adpcm_wav_body(v, 8000)
    assert len(body) == 60 + 40 * 256 and struct.unpack("<I", body[48:52])[0] == 20200
    assert V.adpcm_wav_body(v[:20199], 8000)[:60] != body[:60] and len(V.adpcm_wav_body(v[:20199], 8000)) == len(body)
    assert len(V.adpcm_wav_body(np.concatenate([v, v[:1]]), 8000)) == len(body) + 256


@pytest.mark.parametrize("rate", RATES)
def test_wav16_is_what_form_4_encodes(rate):
    rng = np.random.default_rng(18)
    for N in (0, 1, 2, 599, 600):
        y = (0.4 * rng.standard_normal(N)).astype(np.float32)
        if N > 10:
            y[3], y[4], y[5], y[6] = np.nan, np.inf, -np.inf, 7.0
        body = V.wav16_body(y, rate)
        assert body == base64.b64decode(V.wav16_base64(y, rate)) and len(body) == 44 + 2 * N
        assert struct.unpack("<I", body[4:8])[0] == 36 + 2 * N and struct.unpack("<I", body[40:44])[0] == 2 * N
        word = WAV16 | CODE[rate] << 8
        region = V.stream_body(y, word)
        assert region == body + bytes(-len(body) % 4) and len(region) % 4 == 0
        assert V.stream_body(y, ADPCM | CODE[rate] << 8) == V.adpcm_wav_body(V.pcm16(y), rate)
        if N > 10:
            assert list(np.frombuffer(body[44:], dtype="<i2")[3:7]) == [0, 32767, -32767, 32767]


# ---- the host layout (HIP-free, under the sanitizers) -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adpcm_plan") / "adpcm_plan_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "adpcm_plan_check.cpp"),
                    os.path.join(csrc, "host_request.cpp"), "-lpthread", "-o", exe], check=True)

    def run(mode, text=""):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, mode], env=env, input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


def test_one_table_for_host_numpy_and_generator(driver):
    out = driver("table").splitlines()
    assert [tuple(int(x) for x in ln.split()[1:]) for ln in out[:4]] == [(c, BLOCK[r], _p(r)) for r, c in sorted(CODE.items(), key=lambda kv: kv[1])]
    steps = [int(x) for x in out[4].split()[1:]]
    assert steps == [int(s) for s in V.adpcm_steps()] and len(steps) == 89 and steps[:4] == [7, 8, 9, 10] and steps[-2:] == [29794, 32767]
    assert V.ADPCM_BLOCK_BYTES == BLOCK and V.ADPCM_INDEX_STEPS == (-1, -1, -1, -1, 2, 4, 6, 8)
    text = open(os.path.join(ROOT, "kokorox_amd", "csrc", "adpcm_steps.h"), encoding="utf-8").read()
    assert f"#define KX_ADPCM_START_DIFFS {V.ADPCM_START_DIFFS}\n" in text and V.ADPCM_START_DIFFS == 8
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_adpcm_steps.py"), "--check"])
    assert r.returncode == 0, "kokorox_amd/csrc/adpcm_steps.h differs from tools/gen_adpcm_steps.py"


def test_region_sizes_and_the_4_gib_refusals(driver):
    """pack_request_bytes for both forms at every rate: the numpy body's size, a multiple of 4; and the refusals at the first sample
    count a 32-bit size field cannot hold.  Form 18: 36 + 2 N > 0xFFFFFFFF from N = 2 147 483 630, as form 4.  Form 17: N itself is
    a field (the fact chunk), and it overflows before the RIFF size 52 + A F does at every block size (A F is about N / 2): the first
    bad N is 2^32."""
    lm = {0: (1, 1), 1: (1, 3), 2: (2, 3), 3: (2, 1)}
    pairs = []
    for code, (L, M) in lm.items():
        for frames in (0, 1, 2, 3, 101, 1000):
            for form in (ADPCM, WAV16):
                pairs.append((form | code << 8, 600 * frames))
    rows = driver("sizes", "\n".join(f"{w} {n}" for w, n in pairs)).splitlines()
    rate_of = {c: r for r, c in CODE.items()}
    for (w, n), line in zip(pairs, rows):
        L, M = lm[w >> 8]
        N = n * L // M
        got = [int(x) for x in line.split()]
        want = len(V.stream_body(np.zeros(N, dtype=np.float32), w)) if N <= 60000 else None
        A, P = BLOCK[rate_of[w >> 8]], _p(rate_of[w >> 8])
        formula = 60 + A * -(-N // P) if w & 0xFF == ADPCM else (44 + 2 * N + 3) // 4 * 4
        assert got == [w, n, formula] and formula % 4 == 0 and want in (None, formula), line
    # the first bad N of each form, and the last good one, at 24 kHz (N = n) and at 8 kHz (N = n / 3)
    edge = {WAV16: 2147483630, B64: 2147483630, ADPCM: 1 << 32}
    asks = [(form | code << 8, (N0 - k) * (3 if code else 1)) for form, N0 in edge.items() for code in (0, 1) for k in (1, 0)]
    rows = driver("sizes", "\n".join(f"{w} {n}" for w, n in asks)).splitlines()
    for (w, n), line in zip(asks, rows):
        N = n // (3 if w >> 8 else 1)
        if N == edge[w & 0xFF]:
            text = "an ADPCM WAV file cannot hold" if w & 0xFF == ADPCM else "a 16-bit WAV file cannot hold that many samples (size field of 32 bits)"
            assert line.startswith(f"{w} {n} refused pack: ") and text in line, line
        else:
            assert "refused" not in line and int(line.split()[2]) % 4 == 0, line
    with pytest.raises(ValueError):
        V.adpcm_wav_body(np.broadcast_to(np.int16(0), (1 << 32,)), 8000)  # (the numpy definition refuses where the host does)


def _region(word, N):
    """Bytes of the region of N samples at the output rate in the form of `word` (include/kokorox_hip.h, KX_PACK_*); the two new forms'
    formulas are checked against the numpy bodies in the test above."""
    form, rate = word & 0xFF, {c: r for r, c in CODE.items()}[word >> 8]
    if form == ADPCM:
        return 60 + BLOCK[rate] * -(-N // _p(rate))
    if form == WAV16:
        return (44 + 2 * N + 3) // 4 * 4
    return {0: 4 * N, 1: 8 * N, 2: 2 * N, 3: 44 + 4 * N, 4: 4 * ((44 + 2 * N + 2) // 3), 8: N, 9: N}[form]


def test_plans_of_every_form_and_rate(driver):
    """One-frame requests of every form x rate, and R = 1 .. 64 requests with the two forms among the others: the driver checks region
    sizes, 4-byte multiples, back-to-back offsets, both grids and the bound of the pre-forward allocation; here the sizes once more
    against the formulas."""
    cases, expect = [], {}
    forms = (0, 1, 2, 3, 4, 8, 9, ADPCM, WAV16)
    for code in range(4):
        words = [f | code << 8 for f in forms]
        cases.append(f"one_frame_{code} {len(words)} {len(words)}\n" + " ".join(["1"] * len(words)) + "\n" + " ".join(["1"] * len(words)) + "\n" +
                     " ".join(str(w) for w in words))
        expect[f"one_frame_{code}"] = (words, [600] * len(words))
    rng = np.random.default_rng(64)
    for R in range(1, 65):
        cpr = [int(c) for c in rng.integers(1, 4, R)]
        frames = [int(f) for f in rng.integers(0, 12, sum(cpr))]
        words = [int(rng.choice((ADPCM, WAV16, ADPCM, 2, 4, 8))) | int(rng.integers(0, 4)) << 8 for _ in range(R)]
        cases.append(f"r_{R} {len(frames)} {R}\n" + " ".join(map(str, frames)) + "\n" + " ".join(map(str, cpr)) + "\n" + " ".join(map(str, words)))
        src, at = [], 0
        for c in cpr:
            src.append(600 * sum(frames[at: at + c]))
            at += c
        expect[f"r_{R}"] = (words, src)
    out = driver("plans", "\n".join(cases) + "\n")
    assert "FAILED" not in out
    blocks = out.split("case ")[1:]
    assert len(blocks) == 4 + 64
    lm = {0: (1, 1), 1: (1, 3), 2: (2, 3), 3: (2, 1)}
    for blk in blocks:
        lines = blk.splitlines()
        words, src = expect[lines[0]]
        off = 0
        for r, (w, n) in enumerate(zip(words, src)):
            L, M = lm[w >> 8]
            N = n * L // M
            got = [int(x) for x in lines[1 + r].split()[1:]]
            size = _region(w, N)
            assert got == [r, w & 0xFF, w >> 8, off, size, N], (lines[0], r)
            off += size
        total, units, groups, bound = (int(x) for x in lines[1 + len(words)].split()[1:])
        assert total == off and bound >= total and (groups >= 1) == any(w & 0xFF == ADPCM for w in words)


def test_refusals_with_their_texts(driver):
    rows = dict(line.split("\t", 1) for line in driver("refusals").splitlines())
    for form in (5, 6, 7, 10, 11, 13, 14, 15, 16, 19, 20, 32, 128, 255):
        assert rows[f"form_{form}"] == "1\tinfer: unknown output format", form
    for form in (ADPCM, WAV16):
        for rate in range(4):
            assert rows[f"form_{form}_rate_{rate}"] == "accepted"
        for rate in (4, 5):
            assert rows[f"form_{form}_rate_{rate}"] == "1\tinfer: unknown output sample rate"
        assert rows[f"form_{form}_stray_bit"] == rows[f"form_{form}_negative"] == "1\tinfer: unknown output format"
    assert rows["per_utterance_format_2"] == "accepted"
    for fmt in (ADPCM, WAV16, ADPCM | 0x100):
        assert rows[f"per_utterance_format_{fmt}"] == "1\tinfer: unknown output format"
    assert rows[f"request_format_{ADPCM | 0x100}"] == rows[f"request_format_{WAV16 | 0x300}"] == "accepted"
    assert rows["block_rate_4"] == "1\tinfer: unknown output sample rate"


# ---- the cost of the block-independent start index ----------------------------------------------------------------------------------------
def _snr(v, d):
    v, d = v.astype(np.float64), d.astype(np.float64)
    return 10 * np.log10((v ** 2).sum() / ((v - d) ** 2).sum())


def _voiced(n, rate):
    """A voiced-like signal: eight harmonics, 1 / k in amplitude, of a 120 Hz fundamental with a slow vibrato, under a syllable-like
    envelope of 1.7 Hz between 0.05 and 0.5 -- the same physical signal at every rate."""
    t = np.arange(n) / rate
    phase = 2 * np.pi * np.cumsum(120 * (1 + 0.1 * np.sin(2 * np.pi * 1.3 * t))) / rate
    x = sum(np.sin(k * phase) / k for k in range(1, 9))
    env = 0.05 + 0.45 * np.abs(np.sin(2 * np.pi * 1.7 * t)) ** 2
    return V.pcm16((0.5 * env * x).astype(np.float32))


@pytest.mark.parametrize("rate", [8000, 24000, 48000])
@pytest.mark.parametrize("signal", ["noise", "voiced"])
def test_start_rule_costs_at_most_1_5_db_against_the_sequential_encoder(signal, rate):
    """SNR of decode(encode(v)) against v, for the blocks of this project (every block from its own start index) and for
    audioop.lin2adpcm over the whole stream (state carried across blocks, from (0, 0)), on 8704 samples: the noise fixture at a quarter
    of full scale, and the voiced-like signal above.  The issue allows the block-independent rule 1.5 dB.

    Measured (block rule / sequential / cost, dB), with the start index from the largest of the block's first EIGHT differences:
        noise   8000 Hz (P =  505)  14.691 / 14.630 / -0.061        voiced   8000 Hz (P =  505)  31.658 / 31.641 / -0.016
        noise  24000 Hz (P = 1017)  14.620 / 14.630 /  0.010        voiced  24000 Hz (P = 1017)  43.498 / 42.974 / -0.524
        noise  48000 Hz (P = 2041)  14.648 / 14.630 / -0.018        voiced  48000 Hz (P = 2041)  50.415 / 50.259 / -0.156
    The rule the issue wrote down, the index from the ONE difference |v[1] - v[0]|, cost 0.074 / 0.052 / -0.027 on the noise and
    2.039 / -0.574 / -0.220 on the voiced signal: outside the bound at 8000 Hz, where a block that begins near an extremum of the
    waveform starts with far too small a step and the samples it takes the index to climb weigh heavily against a steady-state error
    of 31 dB.  This is the condition the issue puts on the definition, so the definition was changed, in the open (DESIGN.md section
    7, "ADPCM and 16-bit WAV"), and signal, bound and reference stayed."""
    audioop = pytest.importorskip("audioop")
    n = 8704
    v = V.pcm16(np.resize(_noise(), n) * np.float32(0.25)) if signal == "noise" else _voiced(n, rate)
    d, _ = V.adpcm_wav_decode(V.adpcm_wav_body(v, rate))
    code, _ = audioop.lin2adpcm(v.astype("<i2").tobytes(), 2, None)
    seq = np.frombuffer(audioop.adpcm2lin(code, 2, None)[0], dtype="<i2")[:n]
    ours, theirs = _snr(v, d), _snr(v, seq)
    print(f"{signal} {rate} Hz: block rule {ours:.3f} dB, sequential {theirs:.3f} dB, cost {theirs - ours:.3f} dB")
    assert theirs - ours <= 1.5


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_constants_agree_everywhere():
    from kokorox_amd import hip_koko as hk
    assert (hk.PACK_ADPCM_WAV, hk.PACK_WAV16, hk.ADPCM_MAX_BLOCK) == (17, 18, 1024)
    hdr = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    for name, val in (("KX_PACK_ADPCM_WAV", 17), ("KX_PACK_WAV16", 18), ("KX_ADPCM_MAX_BLOCK", 1024)):
        assert re.search(rf"^#define {name} {val}$", hdr, flags=re.M), name
    assert re.search(r"\bint kx_adpcm_block\(int format_word, int32_t\* block_bytes, int32_t\* samples_per_block\);", hdr)
    hpp = open(os.path.join(ROOT, "include", "kokorox_hip.hpp"), encoding="utf-8").read()
    assert "PACK_ADPCM_WAV = KX_PACK_ADPCM_WAV" in hpp and "PACK_WAV16 = KX_PACK_WAV16" in hpp
    rs = open(os.path.join(ROOT, "kokorox-hip", "src", "lib.rs"), encoding="utf-8").read()
    for name, val in (("KX_PACK_ADPCM_WAV", 17), ("KX_PACK_WAV16", 18), ("KX_ADPCM_MAX_BLOCK", 1024)):
        assert f"pub const {name}: c_int = {val};" in rs
    assert "fn kx_adpcm_block(format_word: c_int, block_bytes: *mut i32, samples_per_block: *mut i32) -> c_int;" in rs
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], text=True, capture_output=True,
                       input='#include "kokorox_hip.hpp"\nstatic_assert(KX_PACK_ADPCM_WAV == 0x11 && KX_PACK_WAV16 == 18 && kokorox::PACK_ADPCM_WAV == 17 && '
                             'kokorox::PACK_WAV16 == 18 && KX_ADPCM_MAX_BLOCK == 1024, "");\n')
    assert r.returncode == 0, r.stderr


def test_adpcm_block_needs_no_gpu():
    from kokorox_amd import hip_koko as hk
    for rate, code in CODE.items():
        for form in (0, ADPCM, 4):  # (only the rate bits are read)
            assert hk.adpcm_block(form | code << 8) == (BLOCK[rate], _p(rate))
    with pytest.raises(hk.KokoroxHipError):
        hk.adpcm_block(ADPCM | 0x400)
    lib = hk.load_library()
    assert lib.kx_adpcm_block(0x100, None, None) == hk.KX_OK  # (either pointer may be NULL)
