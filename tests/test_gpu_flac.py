"""GPU: FLAC bodies (include/kokorox_hip.h, "FLAC") -- flac_frames_kernel, flac_layout_kernel and flac_gather_kernel behind the
packer's launcher, through their test hook, through kx_infer_requests and through the dispatcher.

What is compared, for every FLAC request: its body EQUALS voices.flac_body of the 16-bit samples byte for byte, the length the device
reported is that body's, and the reader of tests/flac_reader.py (written from the format alone) returns exactly the 16-bit samples
form 4 gives for the same request IN THE SAME BATCH (its base64 WAV, decoded).  The hook itself fails where a guard, a poisoned
scratch table or the slack of a region was touched."""
import base64
import json
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_reader as FR  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLAC, PCM16, B64 = 12, 2, 4
TRUE = 0x100
HEAD, TAIL, INNER = 1, 2, 4
RATES = {0: 24000, 1: 8000, 2: 16000, 3: 48000}
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


def _wav16(body):
    """The 16-bit samples of a form 4 body."""
    raw = base64.b64decode(body)
    assert raw[:4] == b"RIFF" and raw[36:40] == b"data"
    return np.frombuffer(raw[44:], dtype="<i2").astype(np.int64)


def _check_flac(body, length, twin, word, what):
    """One FLAC body against the numpy definition and the reader, on the 16-bit samples of its form 4 twin.  Returns the stream."""
    from kokorox_amd import voices as V
    v = _wav16(twin)
    want = V.flac_body(v, RATES[word >> 8])
    assert int(length) == len(body), f"{what}: the device reported {length} bytes, the hook cut {len(body)}"
    assert len(body) == len(want), f"{what}: {len(body)} bytes, the definition has {len(want)}"
    if body != want:
        at = next(i for i in range(len(want)) if body[i] != want[i])
        raise AssertionError(f"{what}: the first of the differing bytes is {at} of {len(want)}")
    got = FR.read_flac(body)
    assert got.samples == [int(x) for x in v], what
    assert got.info["sample_rate"] == RATES[word >> 8] and got.info["total_samples"] == v.shape[0], what
    assert len(body) % 4 == 0 and len(body) <= V.flac_bound(v.shape[0]), what
    return got


def _golden(n):
    """The streams of the limiter's fixtures one behind the other (their NaN and infinities among them) and the noise fixture,
    both repeated up to n samples."""
    with open(os.path.join(GOLDEN, "limits.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    voiced = np.concatenate([np.asarray(c["z_bits"], dtype=np.uint32).view(np.float32) for c in cases])
    with np.load(os.path.join(GOLDEN, "noise_stream.npz")) as z:
        noise = np.asarray(z["z"], dtype=np.float32).reshape(-1)
    return np.resize(voiced, n).astype(np.float32), np.resize(noise, n).astype(np.float32)


def _streams(n):
    """The CPU suite's list, as float streams of n samples at 24 kHz."""
    rng = np.random.default_rng(612)
    t = np.arange(n, dtype=np.float64)
    voiced, noise = _golden(n)
    return {
        "zeros": np.zeros(n, dtype=np.float32),
        "equal": np.full(n, 1.0 / 32767, dtype=np.float32),
        "equal_low": np.full(n, -1.0, dtype=np.float32),
        "ramp": (t / n * 1.9 - 0.95).astype(np.float32),
        "parabola": (((t - n / 2) / (n / 2)) ** 2 * 0.9 - 0.5).astype(np.float32),
        "sine": (0.9 * np.sin(t * 0.013)).astype(np.float32),
        "voiced": voiced,
        "noise": noise,
        "white_full_scale": rng.uniform(-1.0, 1.0, n).astype(np.float32),
        "alternating": np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32),
    }


# ---- the hook ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_hook_one_and_nine_frames_of_every_stream(code):
    """1 and 9 frames of 600 a row: 600 and 5400 samples at 24 kHz, 200 / 1800, 400 / 3600, 1200 / 10800 elsewhere -- a short frame
    alone, and one or two full ones and a short one.  Every stream twice in one launch, as FLAC and as form 4."""
    from kokorox_amd import hip_koko as hk
    parts, words, names = [], [], []
    for frames in (1, 9):
        for name, x in _streams(600 * frames).items():
            for form in (FLAC, B64):
                parts.append(x)
                words.append(form | code << 8)
                names.append(f"{name} x{frames}")
    a, dur, lens = _rows(parts)
    bodies, samples, _, lengths, _, _, _ = hk.flac_requests(a, dur, lens, [1] * len(parts), words)
    kinds = {}
    for r in range(0, len(parts), 2):
        assert samples[r] == samples[r + 1] == parts[r].shape[0] * {0: 3, 1: 1, 2: 2, 3: 6}[code] // 3
        got = _check_flac(bodies[r], lengths[r], bodies[r + 1], words[r], f"{names[r]} at {RATES[code]} Hz")
        assert int(lengths[r + 1]) == len(bodies[r + 1])  # (another form: its region's size)
        kinds[names[r]] = [f.subframes[0].kind for f in got.frames]
        print(names[r], RATES[code], len(bodies[r]), "bytes, PCM16", 2 * samples[r], kinds[names[r]])
    assert set(kinds["zeros x9"]) == {"CONSTANT"}
    assert "FIXED" in kinds["sine x9"] and "FIXED" in kinds["ramp x9"] and "FIXED" in kinds["parabola x1"]
    if code == 0:  # (a constant, and noise over the whole band at full scale, survive only where nothing resamples them)
        assert set(kinds["equal x9"]) == set(kinds["equal_low x1"]) == {"CONSTANT"}
        assert set(kinds["white_full_scale x9"]) == set(kinds["white_full_scale x1"]) == {"VERBATIM"}


def test_hook_exact_lengths_through_a_trimmed_join():
    """N = 4096 exactly, 4088 and 4104 at 8 kHz: 21 frames, the head trimmed down to 12288, 12264 and 12312 samples at 24 kHz (the
    first token lasts two frames: 1200 - 24 keep_ms are cut)."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    rng = np.random.default_rng(8)
    parts, words, joins = [], [], []
    for keep_ms in (37, 36, 38):
        x = (0.2 * np.sin(np.arange(12600) * 0.02) + 0.01 * rng.standard_normal(12600)).astype(np.float32)
        for form in (FLAC, B64):
            parts.append(x)
            words.append(form | 0x100)
            joins.append((HEAD, keep_ms, 0, 4))
    a, dur, lens = _rows(parts)
    bodies, samples, _, lengths, _, _, _ = hk.flac_requests(a, dur, lens, [1] * 6, words, joins=joins)
    assert samples[0::2] == [4096, 4088, 4104]
    for r in range(0, 6, 2):
        got = _check_flac(bodies[r], lengths[r], bodies[r + 1], words[r], f"N {samples[r]}")
        assert [f.block_size for f in got.frames] == ([4096] if samples[r] == 4096 else ([4088] if samples[r] == 4088 else [4096, 8]))
        durs = [[int(d) for d in dur[r, : lens[r]]]]
        assert bodies[r] == V.joined_body([parts[r]], durs, words[r], joins[r])  # (the mirror of the whole request)


def test_hook_nan_inf_and_silence_in_one_batch():
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(31)
    n = 5400
    nan = (0.1 * rng.standard_normal(n)).astype(np.float32)
    nan[::7] = np.nan
    infs = (0.1 * rng.standard_normal(n)).astype(np.float32)
    infs[100:140], infs[4000:4100] = np.inf, -np.inf
    all_nan = np.full(n, np.nan, dtype=np.float32)
    silent = np.zeros(n, dtype=np.float32)
    parts, words = [], []
    for code, x in ((0, nan), (0, infs), (0, all_nan), (0, silent), (3, silent), (1, nan), (3, infs)):
        for form in (FLAC, B64):
            parts.append(x)
            words.append(form | code << 8)
    a, dur, lens = _rows(parts)
    bodies, _, _, lengths, _, _, _ = hk.flac_requests(a, dur, lens, [1] * len(parts), words)
    for r in range(0, len(parts), 2):
        got = _check_flac(bodies[r], lengths[r], bodies[r + 1], words[r], f"request {r}")
        if r in (4, 6, 8):  # NaN -> 0 throughout, and silence at either rate: a dozen bytes a frame
            assert {f.subframes[0].kind for f in got.frames} == {"CONSTANT"} and set(got.samples) == {0}
            assert all(f.n_bytes <= 13 for f in got.frames)
    v = _wav16(bodies[3])
    assert v[100] == 32767 and v[4000] == -32767 and _wav16(bodies[1])[0] == 0


def test_hook_a_pause_between_two_chunks_is_constant_frames_and_marks_do_not_see_the_form():
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(5)
    x0, x1 = (0.2 * rng.standard_normal(3000)).astype(np.float32), (0.2 * rng.standard_normal(2400)).astype(np.float32)
    join = (INNER, 10, 600, 3)  # 14400 zeros between the chunks: frames 1 and 2 of 4096 at 24 kHz lie inside them
    a, dur, lens = _rows([x0, x1, x0, x1, x0, x1])
    words = [FLAC, B64, PCM16]
    res = {}
    for want in (None, [1, 1, 1]):
        res[want is None] = hk.flac_requests(a, dur, lens, [2, 2, 2], words, joins=[join] * 3, want=want)
    bodies, samples, marks, lengths = res[False][:4]
    got = _check_flac(bodies[0], lengths[0], bodies[1], FLAC, "two chunks and a pause")
    kinds = [f.subframes[0].kind for f in got.frames]
    assert kinds.count("CONSTANT") >= 2 and kinds[0] != "CONSTANT" and kinds[-1] != "CONSTANT", kinds
    assert samples[0] == samples[1] == samples[2]
    np.testing.assert_array_equal(marks[0], marks[1])
    np.testing.assert_array_equal(marks[0], marks[2])
    assert marks[0].shape[0] == lens[0] + lens[1] + 2
    assert res[True][0] == bodies and all(m.shape[0] == 0 for m in res[True][2])  # (the bodies do not see the marks either)


def test_hook_levels_loudness_and_limits_run_before_the_encoder():
    """Each kind with and without PEAK_TRUE, at two rates; the twin in form 4 carries the same spec, so the samples the encoder must
    have seen are in the same batch."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(77)
    specs = []
    for flag in (0, TRUE):
        specs += [("level", (0 | flag, 0.5, 0.0)), ("level", (1 | flag, 1.0, 0.25)), ("level", (2 | flag, 3.0, 0.5)),
                  ("loud", (0 | flag, 0.0, 0.0)), ("loud", (1 | flag, -20.0, 0.5)),
                  ("limit", (0 | flag, 3.0, 0.0, 0.25)), ("limit", (1 | flag, 1.0, -14.0, 0.125))]
    parts, words, levels, louds, limits = [], [], [], [], []
    for i, (kind, spec) in enumerate(specs):
        x = (0.1 * rng.standard_normal(5400)).astype(np.float32)
        x[rng.integers(0, 5400, 8)] *= 9.0
        for form in (FLAC, B64):
            parts.append(x)
            words.append(form | (i % 2 * 3) << 8)
            levels.append(spec if kind == "level" else LEVEL_PLAIN)
            louds.append(spec if kind == "loud" else LOUD_NONE)
            limits.append(spec if kind == "limit" else LIMIT_NONE)
    a, dur, lens = _rows(parts)
    bodies, _, _, lengths, lv, ld, lm = hk.flac_requests(a, dur, lens, [1] * len(parts), words, levels=levels, loudness=louds, limits=limits)
    plain = hk.flac_requests(a, dur, lens, [1] * len(parts), words)[0]
    changed = 0
    for r in range(0, len(parts), 2):
        _check_flac(bodies[r], lengths[r], bodies[r + 1], words[r], f"{specs[r // 2]}")
        # the blocks do not see the form: the twin's values are the request's
        assert lv[r].tobytes() == lv[r + 1].tobytes() and ld[r].tobytes() == ld[r + 1].tobytes() and lm[r].tobytes() == lm[r + 1].tobytes()
        changed += bodies[r] != plain[r]
    assert changed >= 10  # (the specs did change the samples: the measuring modes alone leave them)


def test_hook_mixed_batches_flac_in_every_position():
    """FLAC beside forms 0, 3, 4 and 8, in every position: the neighbours' bytes and every block equal those of the same batch with
    form 2 in the FLAC request's place, the FLAC body is the one it has alone, and the bodies are cut back to back by true sizes."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(19)
    xs = [(0.2 * rng.standard_normal(600 * f)).astype(np.float32) * np.float32(np.sin(np.arange(600 * f) * 0.01)) for f in (9, 2, 7, 1, 4)]
    a, dur, lens = _rows(xs)
    others = [0 | 0x100, 3, 4 | 0x300, 8 | 0x200]
    levels = [(1, 1.0, 0.5)] * 5
    want = [1, 0, 1, 1, 0]
    for pos in range(5):
        words = others[:pos] + [FLAC | 0x300] + others[pos:]
        as_pcm = others[:pos] + [PCM16 | 0x300] + others[pos:]
        got = hk.flac_requests(a, dur, lens, [1] * 5, words, levels=levels, want=want)
        ref = hk.flac_requests(a, dur, lens, [1] * 5, as_pcm, levels=levels, want=want)
        for r in range(5):
            if r != pos:
                assert got[0][r] == ref[0][r], (pos, r)
                assert int(got[3][r]) == len(got[0][r])
        assert got[1] == ref[1] and got[4].tobytes() == ref[4].tobytes()
        for m, n in zip(got[2], ref[2]):
            np.testing.assert_array_equal(m, n)
        assert list(ref[3]) == [-1] * 5  # (a batch without the form has no lengths block: the hook left the caller's values)
        alone = hk.flac_requests(a[pos: pos + 1], dur[pos: pos + 1], lens[pos: pos + 1], [1], [FLAC | 0x300], levels=levels[:1])
        assert got[0][pos] == alone[0][0] and int(got[3][pos]) == len(alone[0][0]) == int(alone[3][0]), pos
        twin = hk.flac_requests(a[pos: pos + 1], dur[pos: pos + 1], lens[pos: pos + 1], [1], [B64 | 0x300], levels=levels[:1])[0][0]
        _check_flac(got[0][pos], got[3][pos], twin, FLAC | 0x300, f"position {pos}")
        assert len(got[0][pos]) < len(ref[0][pos])  # (it did compress: noise under a slow envelope)


# ---- the model and the dispatcher ---------------------------------------------------------------------------------------------------
def _chunks():
    from oracle import kokoro_ref as R
    return [list(int(v) for v in R.synthetic_inputs(1, k, seed=500 + k)[0]) for k in (9, 10, 11)]


def test_model_one_request_and_the_entries_that_refuse_the_form(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    toks = _chunks()
    rows = [tab[b % 4, len(t) - 2, 0] for b, t in enumerate(toks)]
    hip_model.set_utterance_base(0)
    for word in (FLAC, FLAC | 0x300):
        bodies, samples = hip_model.infer_requests(toks, [2, 1], styles=rows, seed=3, fmt=[word, B64 | (word & 0xF00)], with_samples=True)
        twins = hip_model.infer_requests(toks, [2, 1], styles=rows, seed=3, fmt=[B64 | (word & 0xF00)] * 2)
        assert isinstance(bodies[0], bytes) and bodies[1] == twins[1]
        got = _check_flac(bodies[0], len(bodies[0]), twins[0], word, f"model, word {word:#x}")
        assert len(got.samples) == samples[0]
        print(f"model word {word:#x}: {len(bodies[0])} bytes for {samples[0]} samples, PCM16 {2 * samples[0]}")
    # with marks, a join and a level in front: the last entry of the family
    bodies, marks, out = hip_model.infer_requests_limited(toks, [3], (0, 2.0, 0.0, 0.5), joins=(INNER, 20, 120, 5), styles=rows, seed=4,
                                                          fmt=FLAC | 0x100, marks=True)
    twin, marks4, out4 = hip_model.infer_requests_limited(toks, [3], (0, 2.0, 0.0, 0.5), joins=(INNER, 20, 120, 5), styles=rows, seed=4,
                                                          fmt=B64 | 0x100, marks=True)
    _check_flac(bodies[0], len(bodies[0]), twin[0], FLAC | 0x100, "limited, joined, marks")
    np.testing.assert_array_equal(marks[0], marks4[0])
    assert out.tobytes() == out4.tobytes()
    # tts_request: the chunks of one text as one FLAC body
    body = V.tts_request(hip_model, {"v": tab[0]}, "v", [t[1:-1] for t in toks[:2]], fmt=FLAC)
    assert FR.read_flac(body).info["sample_rate"] == 24000
    # the entries of the forms 0..2 keep refusing it
    for call in (lambda: hip_model.infer_packed(toks[:1], rows[:1], fmt=FLAC), lambda: hip_model.infer_packed(toks[:1], rows[:1], fmt=10),
                 lambda: hip_model.infer_requests(toks, [2, 1], styles=rows, fmt=11)):
        with pytest.raises(hk.KokoroxHipError, match="unknown output format"):
            call()
    d = hk.Dispatcher([hip_model], max_batch=4, max_wait_us=0)
    try:
        with pytest.raises(hk.KokoroxHipError, match="bad argument"):
            d.submit_ex(toks[0], style=rows[0], fmt=FLAC)
        for bad in (10, 11, FLAC | 0x400):
            with pytest.raises(hk.KokoroxHipError):
                d.submit_request([toks[0]], styles=[rows[0]], fmt=bad)
    finally:
        d.close()


def test_dispatcher_eight_clients_of_mixed_forms_equal_their_solo_runs(hip_model):
    """8 client threads, one request each of 1..3 chunks: FLAC at three rates beside PCM16, float WAV, base64 and mu-law, with and
    without marks and joins; a request's bytes, and so the true length a client is handed, equal the direct call of it alone."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    tab = W.synthetic_voices(4)
    words = [FLAC, 2 | 0x100, FLAC | 0x300, 3, FLAC | 0x100, 4 | 0x200, 8 | 0x100, FLAC | 0x200]
    specs = []
    for i, word in enumerate(words):
        n = 1 + i % 3
        chunks = [list(int(v) for v in R.synthetic_inputs(1, 8 + (5 * i + 3 * c) % 4, seed=1900 + 10 * i + c)[0]) for c in range(n)]
        specs.append(dict(chunks=chunks, styles=[tab[i % 4, len(c) - 2, 0] for c in chunks], fmt=word, seed=8800 + i, marks=i % 2 == 0,
                          join=(INNER, 20, 150, 5) if i % 4 == 2 else None))
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations(None)
    d = hk.Dispatcher([hip_model], max_batch=8, max_wait_us=100000)
    out, errs = [None] * 8, []

    def client(i):
        try:
            s = specs[i]
            out[i] = d.submit_request(s["chunks"], styles=s["styles"], seed=s["seed"], fmt=s["fmt"], marks=s["marks"], join=s["join"])
        except Exception as e:  # pragma: no cover
            errs.append(e)

    try:
        th = [threading.Thread(target=client, args=(i,)) for i in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        st = d.stats()
    finally:
        d.close()
    assert not errs, errs
    for i, s in enumerate(specs):
        n = len(s["chunks"])
        join = s["join"] if s["join"] is not None else (0, 0, 0, 0)
        kw = dict(styles=s["styles"], seed=s["seed"], fmt=s["fmt"])
        if s["marks"]:
            bodies, marks = hip_model.infer_requests_joined(s["chunks"], [n], join, marks=True, **kw)
            np.testing.assert_array_equal(out[i][1], marks[0])
            got = out[i][0]
        else:
            bodies, got = hip_model.infer_requests_joined(s["chunks"], [n], join, **kw), out[i]
        raw = lambda x: x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()  # noqa: E731
        assert raw(got) == raw(bodies[0]) and type(got) is type(bodies[0]), i
        if s["fmt"] & 0xFF == FLAC:
            twin = hip_model.infer_requests_joined(s["chunks"], [n], join, styles=s["styles"], seed=s["seed"], fmt=B64 | (s["fmt"] & 0xF00))[0]
            _check_flac(got, len(got), twin, s["fmt"], f"client {i}")
    assert st["requests"] == 8 and st["batches"] < 8
