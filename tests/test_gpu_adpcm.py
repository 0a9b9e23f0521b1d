"""GPU: IMA ADPCM WAV bodies and 16-bit WAV bodies (include/kokorox_hip.h, "IMA ADPCM"; forms 17 and 18) -- adpcm_blocks_kernel and
the packer's form-18 branch behind the packer's launcher, through the output-plan hook, through kx_infer_requests and through the
dispatcher.

What is compared: a body EQUALS the numpy definition (kokorox_amd/voices.py: adpcm_wav_body, wav16_body, through stream_body and
joined_body) byte for byte; behind the stages this file does not restate (trimmed joins, levels, loudness, the limiter) the request
goes twice into one batch, as form 18 and as form 17, and the ADPCM body must be adpcm_wav_body of the 16-bit samples read back from
the WAV body.  The hook itself fails where a guard behind the last region was touched; a write into a neighbour's region shows as that
neighbour's bytes."""
import base64
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ADPCM, WAV16, B64, MULAW, FLAC, PCM16 = 17, 18, 4, 8, 12, 2
TRUE = 0x100
HEAD, TAIL, INNER = 1, 2, 4
RATES = {0: 24000, 1: 8000, 2: 16000, 3: 48000}
BLOCK = {0: 512, 1: 256, 2: 512, 3: 1024}
LOUD_NONE = (0xFFFFFFFF, 0.0, 0.0)
LIMIT_NONE = (0xFFFFFFFF, 1.0, 0.0, 1.0)
LEVEL_PLAIN = (0, 1.0, 0.0)


def _rows(parts):
    """Rows for the hook from 24 kHz streams of whole frames: up to three tokens whose durations add up to a row's frames, the
    audio poisoned behind each row's samples."""
    B = len(parts)
    frames = [p.shape[0] // 600 for p in parts]
    assert all(p.shape[0] == 600 * f and f >= 1 for p, f in zip(parts, frames))
    dur = np.full((B, 512), -7, dtype=np.int32)
    lens = []
    a = np.empty((B, 600 * max(frames) + 77), dtype=np.float32)
    for b, (p, f) in enumerate(zip(parts, frames)):
        d = [f] if f < 3 else [2, f - 3, 1]
        dur[b, : len(d)] = d
        lens.append(len(d))
        a[b, : p.shape[0]] = p
        a[b, p.shape[0]:] = np.array([1e30, np.inf, -np.inf, np.nan], dtype=np.float32)[(np.arange(a.shape[1] - p.shape[0]) + b) % 4]
    return a, dur, lens


def _speech(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return ((0.3 * np.sin(t * 0.031) + 0.1 * np.sin(t * 0.47)) * (0.2 + 0.8 * np.sin(t * 0.0007) ** 2) + 0.01 * rng.standard_normal(n)).astype(np.float32)


def _same(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} bytes, the definition has {len(want)}"
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"{what}: the first of the differing bytes is {at} of {len(want)}")


def _wav16_samples(region):
    """The 16-bit samples of a form-18 region (its zero padding left out)."""
    assert region[:4] == b"RIFF" and region[36:40] == b"data"
    n = struct.unpack("<I", region[40:44])[0]
    assert len(region) == (44 + n + 3) // 4 * 4 and not any(region[44 + n:])
    return np.frombuffer(region[44: 44 + n], dtype="<i2")


# ---- the hook: bodies against the numpy definition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_hook_one_frame_is_a_single_partial_block(code):
    """One request of one frame: 600 / 200 / 400 / 1200 samples, a single partial block whose tail repeats the last sample; beside it
    the same frame as form 18 and as form 4."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    x = _speech(600, 3 + code)
    words = [ADPCM | code << 8, WAV16 | code << 8, B64 | code << 8]
    a, dur, lens = _rows([x, x, x])
    bodies, samples, _, lengths, _, _, _ = hk.flac_requests(a, dur, lens, [1, 1, 1], words)
    y = V.resample_stream(x, words[0])
    assert samples == [y.shape[0]] * 3 and y.shape[0] == {0: 600, 1: 200, 2: 400, 3: 1200}[code]
    _same(bodies[0], V.adpcm_wav_body(V.pcm16(y), RATES[code]), f"ADPCM at {RATES[code]} Hz")
    assert len(bodies[0]) == 60 + BLOCK[code]
    file = V.wav16_body(y, RATES[code])
    _same(bodies[1], file + bytes(-len(file) % 4), f"WAV16 at {RATES[code]} Hz")
    assert base64.b64decode(bodies[2]) == file  # (form 18 is what form 4 encodes)
    d, rate = V.adpcm_wav_decode(bodies[0])
    assert rate == RATES[code] and d.shape[0] == samples[0] and d[0] == V.pcm16(y)[0]


def test_hook_forty_blocks_exactly_and_more_than_one_group_at_every_rate():
    """101 frames at 8 kHz are 20 200 samples = 40 blocks of 505 with no padding: two workgroups (32 blocks a group).  30 frames at the
    other rates: 18 blocks at 24 kHz and 48 kHz (two and three groups), 12 at 16 kHz; every stream longer than the staging tile."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    long_, short = _speech(600 * 101, 40), _speech(600 * 30, 41)
    parts = [long_, short, short, short, long_]
    words = [ADPCM | 0x100, ADPCM, ADPCM | 0x200, ADPCM | 0x300, WAV16 | 0x100]
    a, dur, lens = _rows(parts)
    bodies, samples, _, _, _, _, _ = hk.flac_requests(a, dur, lens, [1] * 5, words)
    assert samples == [20200, 18000, 12000, 36000, 20200]
    assert len(bodies[0]) == 60 + 40 * 256 and struct.unpack("<I", bodies[0][48:52])[0] == 20200
    for r, (x, w) in enumerate(zip(parts, words)):
        _same(bodies[r], V.stream_body(V.resample_stream(x, w), w), f"request {r}, word {w:#x}")


def test_hook_three_requests_of_one_two_and_three_chunks_in_mixed_forms():
    """Requests of 1, 2 and 3 chunks with a 50 ms pause between chunks, the forms 17, 18, 4, 8 and 12 rotating through the three
    places at mixed rates.  At 24 kHz the blocks end every 1017 samples: inside chunks, across the seams (2400; 1200 and 5400) and
    inside the pauses (2400..3600; 1200..2400 and 5400..6600)."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    frames = [3, 4, 2, 2, 5, 3]
    parts = [_speech(600 * f, 70 + i) for i, f in enumerate(frames)]
    a, dur, lens = _rows(parts)
    cpr = [1, 2, 3]
    join = (0, 0, 50, 0)
    chunks = [parts[0:1], parts[1:3], parts[3:6]]
    durs = [[[int(d) for d in dur[b, : lens[b]]] for b in rows] for rows in ([0], [1, 2], [3, 4, 5])]
    batches = [[ADPCM, WAV16 | 0x100, B64 | 0x300], [FLAC | 0x200, ADPCM, MULAW | 0x100], [WAV16, MULAW, ADPCM], [B64 | 0x100, ADPCM | 0x100, ADPCM | 0x300],
               [ADPCM | 0x200, FLAC, WAV16 | 0x300], [ADPCM | 0x300, ADPCM | 0x200, ADPCM | 0x100]]
    for words in batches:
        bodies, samples, marks, _, _, _, _ = hk.flac_requests(a, dur, lens, cpr, words, joins=[join] * 3, want=[1, 1, 1])
        for r, w in enumerate(words):
            _same(bodies[r], V.joined_body(chunks[r], durs[r], w, join), f"request {r} of {[hex(x) for x in words]}")
            np.testing.assert_array_equal(marks[r], V.joined_marks(durs[r], w, join))
            if w & 0xFF == ADPCM:
                assert V.adpcm_wav_decode(bodies[r])[0].shape[0] == samples[r]
    assert samples[2] == (600 * 10 + 2 * 1200) // 3  # (the last batch: the three-chunk request at 8 kHz, pauses included)


def test_hook_nan_inf_overdrive_silence_and_a_full_scale_square_wave():
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    rng = np.random.default_rng(31)
    n = 3000
    nan = (0.1 * rng.standard_normal(n)).astype(np.float32)
    nan[::7] = np.nan
    infs = (0.1 * rng.standard_normal(n)).astype(np.float32)
    infs[100:140], infs[2000:2100] = np.inf, -np.inf
    loud = (3.0 * rng.standard_normal(n)).astype(np.float32)  # beyond +-1 most of the time
    square = np.where((np.arange(n) // 5) % 2 == 0, 1.0, -1.0).astype(np.float32)
    fast = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    streams = {"nan": nan, "inf": infs, "all_nan": np.full(n, np.nan, dtype=np.float32), "overdrive": loud, "zeros": np.zeros(n, dtype=np.float32),
               "square": square, "square_every_sample": fast}
    parts, words, names = [], [], []
    for name, x in streams.items():
        for w in (ADPCM, WAV16, ADPCM | 0x100, WAV16 | 0x300):
            parts.append(x), words.append(w), names.append(name)
    a, dur, lens = _rows(parts)
    bodies = hk.flac_requests(a, dur, lens, [1] * len(parts), words)[0]
    for r, (x, w, name) in enumerate(zip(parts, words, names)):
        _same(bodies[r], V.stream_body(V.resample_stream(x, w), w), f"{name}, word {w:#x}")
    by = {(n_, w): b for n_, w, b in zip(names, words, bodies)}
    v = _wav16_samples(by["inf", WAV16])
    assert v[100] == 32767 and v[2000] == -32767 and _wav16_samples(by["nan", WAV16])[0] == 0
    assert not any(by["zeros", ADPCM][60:]) and not any(by["all_nan", ADPCM][60:])  # (silence: predictor 0, index 0, codes 0)
    assert by["square_every_sample", ADPCM][62] == 88  # (a difference of 65534 is above every step)
    d = V.adpcm_wav_decode(by["square", ADPCM])[0]
    assert d.max() == 32767 and d.min() == -32768  # (the predictor ran into both clamps)


def test_hook_behind_joins_levels_loudness_and_the_limiter():
    """Every source path of the kernel: plain rows, joined rows, the resampled run, a levelled gain, the limiter's run.  The request is
    in the batch twice, as form 18 and as form 17 with the same specs: the ADPCM body is adpcm_wav_body of the WAV body's samples."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    rng = np.random.default_rng(77)
    trim = (HEAD | TAIL | INNER, 20, 40, 5)
    specs = [("join", trim, 0), ("join", trim, 1), ("level", (1 | TRUE, 1.0, 0.25), 0), ("level", (1 | TRUE, 1.0, 0.25), 3), ("level", (2, 3.0, 0.5), 2),
             ("loud", (1, -20.0, 0.5), 0), ("loud", (1 | TRUE, -20.0, 0.5), 1), ("limit", (0, 3.0, 0.0, 0.25), 0),
             ("limit", (1 | TRUE, 1.0, -14.0, 0.125), 3), ("limit", (0, 3.0, 0.0, 0.25), 1)]
    parts, words, cpr, joins, levels, louds, limits = [], [], [], [], [], [], []
    for i, (kind, spec, code) in enumerate(specs):
        xs = [(0.1 * rng.standard_normal(600 * f)).astype(np.float32) for f in (7, 6)]
        xs[0][rng.integers(0, 4200, 8)] *= 9.0
        for form in (WAV16, ADPCM):
            parts += xs
            cpr.append(2)
            words.append(form | code << 8)
            joins.append(spec if kind == "join" else (0, 0, 0, 0))
            levels.append(spec if kind == "level" else LEVEL_PLAIN)
            louds.append(spec if kind == "loud" else LOUD_NONE)
            limits.append(spec if kind == "limit" else LIMIT_NONE)
    a, dur, lens = _rows(parts)
    bodies, samples, _, _, lv, ld, lm = hk.flac_requests(a, dur, lens, cpr, words, joins=joins, levels=levels, loudness=louds, limits=limits)
    plain = hk.flac_requests(a, dur, lens, cpr, words)[0]
    changed = set()
    for r in range(0, len(words), 2):
        code = words[r] >> 8
        v = _wav16_samples(bodies[r])
        assert samples[r] == samples[r + 1] == v.shape[0]
        _same(bodies[r + 1], V.adpcm_wav_body(v, RATES[code]), f"{specs[r // 2]}")
        # the blocks behind the bodies do not see the form
        assert lv[r].tobytes() == lv[r + 1].tobytes() and ld[r].tobytes() == ld[r + 1].tobytes() and lm[r].tobytes() == lm[r + 1].tobytes()
        if bodies[r + 1] != plain[r + 1]:
            changed.add(specs[r // 2][0])
    assert changed == {"join", "level", "loud", "limit"}  # (every kind of spec did change the samples the encoder saw)


# ---- the model and the dispatcher ---------------------------------------------------------------------------------------------------
def _chunks():
    from oracle import kokoro_ref as R
    return [list(int(v) for v in R.synthetic_inputs(1, k, seed=500 + k)[0]) for k in (9, 10, 11)]


def test_model_dispatcher_and_the_entries_that_refuse_the_forms(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    toks = _chunks()
    rows = [tab[b % 4, len(t) - 2, 0] for b, t in enumerate(toks)]
    hip_model.set_utterance_base(0)
    word = ADPCM | hk.PACK_RATE_8000
    assert (hk.PACK_ADPCM_WAV, hk.PACK_WAV16) == (ADPCM, WAV16)
    # three short chunks as one request: the body decodes to N = out_samples, and it is the definition on form 18's samples
    bodies, samples = hip_model.infer_requests(toks, [3, ], styles=rows, seed=3, fmt=word, with_samples=True)
    wav = hip_model.infer_requests(toks, [3], styles=rows, seed=3, fmt=WAV16 | hk.PACK_RATE_8000)[0]
    b64 = hip_model.infer_requests(toks, [3], styles=rows, seed=3, fmt=B64 | hk.PACK_RATE_8000)[0]
    assert isinstance(bodies[0], bytes) and isinstance(wav, bytes) and wav == base64.b64decode(b64) and len(wav) == 44 + 2 * samples[0]
    d, rate = V.adpcm_wav_decode(bodies[0])
    assert rate == 8000 and d.shape[0] == samples[0] and struct.unpack("<I", bodies[0][48:52])[0] == samples[0]
    _same(bodies[0], V.adpcm_wav_body(np.frombuffer(wav[44:], dtype="<i2"), 8000), "model, form 17 at 8 kHz")
    print(f"model: {len(bodies[0])} ADPCM bytes for {samples[0]} samples, 16-bit WAV {len(wav)}")
    # beside another form in one call, and the marks do not see the form
    both, marks = hip_model.infer_requests_marks(toks, [2, 1], styles=rows, seed=3, fmt=[word, WAV16])
    four, marks4 = hip_model.infer_requests_marks(toks, [2, 1], styles=rows, seed=3, fmt=[B64 | hk.PACK_RATE_8000, B64])
    for m, m4 in zip(marks, marks4):
        np.testing.assert_array_equal(m, m4)
    _same(both[0], V.adpcm_wav_body(np.frombuffer(base64.b64decode(four[0])[44:], dtype="<i2"), 8000), "two chunks beside a WAV request")
    assert both[1] == base64.b64decode(four[1])
    # tts_request: the chunks of one text as one ADPCM body
    body = V.tts_request(hip_model, {"v": tab[0]}, "v", [t[1:-1] for t in toks[:2]], fmt=ADPCM)
    assert V.adpcm_wav_decode(body)[1] == 24000
    # the entries of the forms 0..2 keep refusing both, and the unused numbers stay refused
    for call in (lambda: hip_model.infer_packed(toks[:1], rows[:1], fmt=ADPCM), lambda: hip_model.infer_packed(toks[:1], rows[:1], fmt=WAV16),
                 lambda: hip_model.infer_requests(toks, [2, 1], styles=rows, fmt=16), lambda: hip_model.infer_requests(toks, [2, 1], styles=rows, fmt=19)):
        with pytest.raises(hk.KokoroxHipError, match="unknown output format"):
            call()
    d = hk.Dispatcher([hip_model], max_batch=4, max_wait_us=0)
    try:
        got = d.submit_request(toks, styles=rows, seed=3, fmt=hk.PACK_ADPCM_WAV | hk.PACK_RATE_8000)
        assert type(got) is bytes and got == bodies[0]
        got, m = d.submit_request(toks[:2], styles=rows[:2], seed=3, fmt=word, marks=True)
        assert got == both[0]
        np.testing.assert_array_equal(m, marks[0])
        assert d.submit_request(toks, styles=rows, seed=3, fmt=hk.PACK_WAV16 | hk.PACK_RATE_8000) == wav
        for fmt in (ADPCM, WAV16):
            with pytest.raises(hk.KokoroxHipError, match="bad argument"):
                d.submit_ex(toks[0], style=rows[0], fmt=fmt)
        for bad in (13, 16, 19, ADPCM | 0x400, WAV16 | 0x1000):
            with pytest.raises(hk.KokoroxHipError):
                d.submit_request([toks[0]], styles=[rows[0]], fmt=bad)
    finally:
        d.close()
