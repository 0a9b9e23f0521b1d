"""CPU: the output-rate resampler and the G.711 forms of the request packer, without a GPU.

The library hands out its one table of taps through kx_resample_filter (host only); the numpy mirrors of kokorox_amd/voices.py
(`resample_stream`, `mulaw_bytes`, `alaw_bytes`) compute with that table, so what the GPU suite compares the kernels with is
checked here first: the taps against their formula, the filters' frequency responses, the mirror on signals whose answer is
known, G.711 against CPython's audioop on all 65 536 inputs, the WAV headers at every rate, and the request plan with format
words (tests/cpp/resample_plan_check.cpp, built with g++ under the address and undefined-behaviour sanitizers).
"""
import base64
import json
import os
import struct
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = {0x100: (8000, 1, 3, 145), 0x200: (16000, 2, 3, 145), 0x300: (48000, 2, 1, 97)}  # word: Hz, L, M, taps
BETA = 10.0


@pytest.fixture(scope="module")
def filters():
    from kokorox_amd import hip_koko as hk
    return {w: hk.resample_filter(w) for w in RATES}


def _formula(L, M):
    Q = max(L, M)
    C = 24 * Q
    N = 2 * C + 1
    i = np.arange(N, dtype=np.float64)
    h = np.sinc((i - C) / Q) * np.kaiser(N, BETA)
    return h * (L / h.sum())


# ---- taps ----------------------------------------------------------------------------------------------------------------
def test_taps_equal_the_formula_within_one_ulp_and_are_symmetric(filters):
    from kokorox_amd import hip_koko as hk
    for w, (hz, L, M, n_taps) in RATES.items():
        gL, gM, h = filters[w]
        assert (gL, gM, h.shape[0], h.dtype) == (L, M, n_taps, np.float32), hz
        want = _formula(L, M)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(h.astype(np.float64) - want) <= ulp), hz
        np.testing.assert_array_equal(h, h[::-1])
        # every form of the word names the same filter; rate code 0 has none
        assert np.array_equal(hk.resample_filter(w | hk.PACK_ALAW)[2], h)
    L0, M0, h0 = hk.resample_filter(hk.PACK_WAV16_BASE64)
    assert (L0, M0, h0.shape) == (1, 1, (0,))
    for bad in (0x400, 0xF00, 0x105, 0x1000, -1):
        with pytest.raises(hk.KokoroxHipError) as e:
            hk.resample_filter(bad)
        assert e.value.code == hk.KX_ERR_INVALID


def test_committed_table_is_what_the_generator_writes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_resample_taps.py"), "--check"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_frequency_response_of_the_float32_taps(filters):
    """On a 20 001-point grid from 0 to the Nyquist frequency of the filter's own rate (24 000 L); Nyq = the smaller Nyquist
    frequency of input and output.  The bounds are the issue's; measured: 1.04e-5 / 1.04e-5 / 1.03e-5 pass-band deviation,
    -100.4 / -100.4 / -100.1 dB stop band, -6.02 dB at Nyq."""
    for w, (hz, L, M, _) in RATES.items():
        h = filters[w][2].astype(np.float64)
        fs = 24000.0 * L
        nyq = min(12000.0, hz / 2.0)
        f = np.linspace(0.0, fs / 2, 20001)
        k = np.arange(h.shape[0])
        H = np.abs(np.exp(-2j * np.pi * np.outer(f / fs, k)) @ h) / L
        dev = np.max(np.abs(H[f <= 0.85 * nyq] - 1.0))
        stop = 20 * np.log10(np.max(H[f >= 1.15 * nyq]))
        at_nyq = 20 * np.log10(np.abs(np.exp(-2j * np.pi * (nyq / fs) * k) @ h) / L)
        phases = [h[p::L].sum() for p in range(L)]
        print(f"{hz} Hz: pass-band deviation {dev:.3e}, stop band {stop:.2f} dB, at Nyquist {at_nyq:.3f} dB, phase sums {phases}")
        assert dev <= 2e-5, hz
        assert stop <= -99.0, hz
        assert abs(at_nyq + 6.0) <= 0.1, hz
        assert all(abs(p - 1.0) <= 2e-6 for p in phases), hz


# ---- the mirror ------------------------------------------------------------------------------------------------------------
def _interior(n_out, L, M, C):
    """Outputs whose whole support lies inside the stream."""
    lo = -(-C // M)
    return slice(lo, n_out - lo)


def test_mirror_of_an_impulse_returns_the_taps(filters):
    from kokorox_amd import voices as V
    for w, (hz, L, M, n_taps) in RATES.items():
        h = filters[w][2]
        C = (n_taps - 1) // 2
        S = 600
        for j0 in (300, 301):
            x = np.zeros(S, dtype=np.float32)
            x[j0] = 1.0
            y = V.resample_stream(x, w)
            assert y.dtype == np.float32 and y.shape == (S * L // M,)
            n = np.arange(y.shape[0])
            idx = n * M - j0 * L + C
            want = np.where((idx >= 0) & (idx < n_taps), h[np.clip(idx, 0, n_taps - 1)], np.float32(0))
            np.testing.assert_array_equal(y, want)
            assert np.count_nonzero(want) >= n_taps // M - 1
    x = np.arange(600, dtype=np.float32)
    assert V.resample_stream(x, 4) is not None and np.array_equal(V.resample_stream(x, 4), x)  # rate code 0: as it is


def test_mirror_on_constants_and_tones(filters):
    from kokorox_amd import voices as V
    S = 2400
    t = np.arange(S, dtype=np.float64) / 24000.0
    for w, (hz, L, M, n_taps) in RATES.items():
        C = (n_taps - 1) // 2
        n_out = S * L // M
        inner = _interior(n_out, L, M, C)
        y = V.resample_stream(np.ones(S, dtype=np.float32), w).astype(np.float64)
        assert np.max(np.abs(y[inner] - 1.0)) <= 2e-6, hz
        # a 1 kHz tone keeps its amplitude: compared with the same tone sampled at the output rate (the filter's delay is C / L
        # input samples = a whole number of taps, which the definition's index n M - j L + C already takes out)
        x = np.sin(2 * np.pi * 1000.0 * t).astype(np.float32)
        y = V.resample_stream(x, w).astype(np.float64)
        want = np.sin(2 * np.pi * 1000.0 * np.arange(n_out) / hz)
        # (x itself is rounded to float32: 6e-8 of the amplitude, far inside the bound)
        assert np.max(np.abs(y[inner] - want[inner])) <= 2e-5, hz
    # 5 kHz lies above 1.15 x the 4 kHz Nyquist frequency of the 8 kHz output: at most 1.2e-5 of it is left
    x = np.sin(2 * np.pi * 5000.0 * t).astype(np.float32)
    y = V.resample_stream(x, 0x100).astype(np.float64)
    assert np.max(np.abs(y[_interior(S // 3, 1, 3, 72)])) <= 1.2e-5


def test_mirror_sums_in_ascending_order_in_float64(filters):
    """The definition written out sample by sample, with python floats (float64), on a short stream with both edges inside the
    filter's support."""
    from kokorox_amd import voices as V
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.3, 1.3, 150).astype(np.float32)
    for w, (hz, L, M, n_taps) in RATES.items():
        h = filters[w][2]
        C = (n_taps - 1) // 2
        y = V.resample_stream(x, w)
        want = np.zeros(y.shape[0], dtype=np.float32)
        for n in range(y.shape[0]):
            acc = 0.0
            for j in range(x.shape[0]):
                i = n * M - j * L + C
                if 0 <= i < n_taps:
                    acc += float(h[i]) * float(x[j])
            want[n] = np.float32(acc)
        np.testing.assert_array_equal(y, want)


# ---- G.711 -----------------------------------------------------------------------------------------------------------------
def test_g711_mirrors_equal_audioop_on_every_16_bit_input():
    from kokorox_amd import voices as V
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        import audioop
    v = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    raw = v.astype("<i2").tobytes()
    np.testing.assert_array_equal(V.mulaw_bytes(v), np.frombuffer(audioop.lin2ulaw(raw, 2), dtype=np.uint8))
    np.testing.assert_array_equal(V.alaw_bytes(v), np.frombuffer(audioop.lin2alaw(raw, 2), dtype=np.uint8))
    assert V.mulaw_bytes(v).dtype == np.uint8 and V.alaw_bytes(v).shape == (65536,)


def test_g711_known_answers_of_the_fixture():
    from kokorox_amd import voices as V
    with open(os.path.join(ROOT, "tests", "golden", "g711_known_answers.json"), encoding="utf-8") as f:
        gold = json.load(f)
    v = np.array(gold["pcm16"], dtype=np.int16)
    assert [f"{b:02X}" for b in V.mulaw_bytes(v)] == gold["mulaw_hex"]
    assert [f"{b:02X}" for b in V.alaw_bytes(v)] == gold["alaw_hex"]


# ---- WAV headers -------------------------------------------------------------------------------------------------------------
def test_wav_headers_carry_the_rate():
    from kokorox_amd import voices as V
    x = np.linspace(-1, 1, 200, dtype=np.float32)
    assert V.wav_f32_body(x) == V.wav_f32_body(x, 24000) and V.wav16_base64(x) == V.wav16_base64(x, 24000)
    for hz in (8000, 16000, 24000, 48000):
        body = V.wav_f32_body(x, hz)
        riff, size, wave, fmt_, n16, tag, ch, rate, brate, align, bits, data, dsize = struct.unpack("<4sI4s4sIHHIIHH4sI", body[:44])
        assert (riff, wave, fmt_, data) == (b"RIFF", b"WAVE", b"fmt ", b"data")
        assert (size, dsize) == (0xFFFFFFFF, 0xFFFFFFFF)  # the reference's placeholders
        assert (n16, tag, ch, rate, brate, align, bits) == (16, 3, 1, hz, hz * 4, 4, 32)
        assert body[44:] == x.tobytes()
        raw = base64.b64decode(V.wav16_base64(x, hz), validate=True)
        riff, size, wave, fmt_, n16, tag, ch, rate, brate, align, bits, data, dsize = struct.unpack("<4sI4s4sIHHIIHH4sI", raw[:44])
        assert (size, dsize) == (36 + 400, 400)
        assert (n16, tag, ch, rate, brate, align, bits) == (16, 1, 1, hz, hz * 2, 2, 16)
        assert raw[44:] == V.pcm16(x).astype("<i2").tobytes()
    # one, two and three frames at 8 kHz: the text ends in no, two and one '='
    for frames, tail in ((1, 0), (2, 2), (3, 1)):
        text = V.wav16_base64(np.zeros(200 * frames, dtype=np.float32), 8000)
        assert len(text) - len(text.rstrip(b"=")) == tail


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def test_request_plan_with_format_words_under_the_sanitizers(tmp_path):
    """Region sizes and offsets for every form x rate with 1, 2 and 3 frames, the packed bound and the intermediate buffer of
    one-frame requests, the refusals (rate codes 4..15, forms 5..7, stray high bits) with their exact messages."""
    exe = str(tmp_path / "resample_plan_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "resample_plan_check.cpp"), os.path.join(csrc, "host_request.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "filters: 145 145 97 taps" in r.stdout
    assert "plans: 84 (rate, form, frames) triples" in r.stdout
    assert "bounds: 224 one-frame batches" in r.stdout
    assert "refusals: 124 words" in r.stdout


def test_python_constants_mirror_the_header():
    from kokorox_amd import hip_koko as hk
    hdr = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    for name in ("MULAW", "ALAW", "RATE_24000", "RATE_8000", "RATE_16000", "RATE_48000"):
        line = next(ln for ln in hdr.splitlines() if ln.startswith(f"#define KX_PACK_{name} "))
        assert int(line.split()[2], 0) == getattr(hk, "PACK_" + name), name
    assert {c: hk.RATE_HZ[c] for c in range(4)} == {0: 24000, 1: 8000, 2: 16000, 3: 48000}
    rs = open(os.path.join(ROOT, "kokorox-hip", "src", "lib.rs"), encoding="utf-8").read()
    for name, val in (("MULAW", "8"), ("ALAW", "9"), ("RATE_8000", "0x100"), ("RATE_16000", "0x200"), ("RATE_48000", "0x300")):
        assert f"pub const KX_PACK_{name}: c_int = {val};" in rs
