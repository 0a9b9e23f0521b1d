"""CPU: the host mirrors of the two bodies the reference's servers send — the float WAV of the HTTP server
(kokorox/src/utils/wav.rs:18-50, kokorox-openai/src/lib.rs:416-425) and the base64 16-bit WAV of the WebSocket server
(`encode_audio`, kokorox-websocket/src/lib.rs:696-736) — against known answers derived by hand (tests/golden/wire_formats.json),
and `tts_request`, the chunk loop as one request, against a fake model."""
import base64
import json
import os
import struct

import numpy as np
import pytest

from kokorox_amd import voices as V

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wire_formats.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLD, encoding="utf-8") as f:
        g = json.load(f)
    g["x"] = np.array([float(s) for s in g["samples"]], dtype=np.float32)
    return g


def test_float_wav_body_matches_the_fixture(gold):
    x = gold["x"].copy()
    x[4] = np.frombuffer(struct.pack("<I", 0x7FC12345), dtype=np.float32)[0]  # a NaN with a payload
    body = V.wav_f32_body(x)
    assert len(body) == 44 + 4 * len(x)
    assert body[:44].hex() == gold["wav_f32_header_hex"]
    assert body[44:] == x.tobytes()  # bit copies: the payload survives
    assert struct.unpack("<I", body[44 + 16: 44 + 20])[0] == 0x7FC12345
    assert V.wav_f32_body([])[:44].hex() == gold["wav_f32_header_hex"]


def test_pcm16_and_base64_match_the_fixture(gold):
    assert V.pcm16(gold["x"]).tolist() == gold["pcm16"]
    text = V.wav16_base64(gold["x"])
    assert isinstance(text, bytes) and text.decode("ascii") == gold["wav16_base64"]
    raw = base64.b64decode(text, validate=True)
    riff, size, wave, fmt_, n16, tag, ch, rate, bps, align, bits, data, n = struct.unpack("<4sI4s4sIHHIIHH4sI", raw[:44])
    assert (riff, wave, fmt_, data) == (b"RIFF", b"WAVE", b"fmt ", b"data")
    assert (size, n16, tag, ch, rate, bps, align, bits, n) == (36 + 24, 16, 1, 1, 24000, 48000, 2, 16, 24)
    assert np.frombuffer(raw[44:], dtype="<i2").tolist() == gold["pcm16"]


def test_rust_cast_semantics_at_the_edges():
    one_up = np.nextafter(np.float32(1), np.float32(2))
    x = np.array([1.0, -1.0, one_up, -one_up, 32766.5 / 32767, -32766.5 / 32767, 1e-45, np.nan, -np.nan], dtype=np.float32)
    assert V.pcm16(x).tolist() == [32767, -32767, 32767, -32767, 32766, -32766, 0, 0, 0]


@pytest.mark.parametrize("n", [600, 1200, 1800, 4200])
def test_text_length_and_single_pad(n):
    rng = np.random.default_rng(n)
    text = V.wav16_base64(rng.uniform(-1.3, 1.3, n).astype(np.float32))
    assert len(text) == 4 * ((44 + 2 * n + 2) // 3)
    assert (44 + 2 * n) % 3 == 2 and text.endswith(b"=") and not text.endswith(b"==")
    assert b"\n" not in text and b"\0" not in text


def test_silence_lengths_of_the_fixture(gold):
    for frames, length in gold["silence_text_length"].items():
        text = V.wav16_base64(np.zeros(600 * int(frames), dtype=np.float32))
        assert len(text) == length and text.decode().endswith(gold["silence_text_tail"])


class _FakeModel:
    def __init__(self):
        self.calls = []

    def infer_requests(self, tokens, chunks_per_request, styles=None, voice_ids=None, weights=None, speeds=(1.0,), seed=0,
                       flags=0, fmt=0):
        self.calls.append(dict(tokens=tokens, cpr=list(chunks_per_request), styles=np.asarray(styles), speeds=list(speeds),
                               seed=seed, fmt=fmt, voice_ids=voice_ids))
        return ["body"]


def test_tts_request_builds_one_request_of_all_chunks():
    rng = np.random.default_rng(3)
    styles = {"af_sky": rng.standard_normal((511, 1, 256)).astype(np.float32),
              "af_nicole": rng.standard_normal((511, 1, 256)).astype(np.float32)}
    m = _FakeModel()
    chunks = [[5, 6, 7], [9], [11, 12, 13, 14, 15]]
    out = V.tts_request(m, styles, "af_sky.4+af_nicole.5", chunks, speed=1.25, initial_silence=2, seed=77, fmt=4)
    assert out == "body" and len(m.calls) == 1
    c = m.calls[0]
    assert c["cpr"] == [3] and c["seed"] == 77 and c["fmt"] == 4 and c["speeds"] == [1.25] and c["voice_ids"] is None
    assert c["tokens"] == [[0, 30, 30] + ch + [0] for ch in chunks]  # koko.rs:1161-1175 per chunk
    want = [V.mix_styles(styles, "af_sky.4+af_nicole.5", len(ch) + 2)[0] for ch in chunks]  # the row of the chunk's own length
    np.testing.assert_array_equal(c["styles"], np.asarray(want, dtype=np.float32))
    with pytest.raises(ValueError, match="empty chunk"):
        V.tts_request(m, styles, "af_sky", [[5], []])
    with pytest.raises(ValueError, match="at least one chunk"):
        V.tts_request(m, styles, "af_sky", [])
    assert len(m.calls) == 1
