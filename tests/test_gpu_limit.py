"""GPU: the limiter (include/kokorox_hip.h, "limiter") -- request_limit_kernel, its report and the limited packer behind the gain
kernels, through their test hook, through kx_infer_requests_limited and through the dispatcher, against the numpy definition of
kokorox_amd/voices.py (limit_stream).

What is compared.  Mode 0 (the drive is a gain): the body's bytes, the marks and the five doubles f64(p), g, I, n_g, r all EQUAL
the mirror's.  Mode 1 (the drive comes from the BS.1770 meter): p, n_g and r are equal; I and g carry the meter's own bounds
(tests/test_gpu_loudness.py: |I - mirror| <= 1e-8 LU, |g - mirror| <= 1e-8 g -- the hop energies are sums of some thousand float64
terms in another order -- and g is equal where the drive cap sets it); everything behind g is then bit-exact: the body and r equal
the mirror's with the drive the GPU reported."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TRUE = 0x100
GAIN, LOUD = 0, 1
NONE = (0xFFFFFFFF, 1.0, 0.0, 1.0)      # the hook only: a request without a limiter
LOUD_NONE = (0xFFFFFFFF, 0.0, 0.0)      # the hook only: a request that is not metered
HEAD, TAIL, INNER = 1, 2, 4
JOIN = (HEAD | TAIL | INNER, 10, 85, 5)
RATES = {0: 24000, 1: 8000, 2: 16000, 3: 48000}
WINDOW = 4096  # host_request.h: LEVEL_WINDOW, the samples of one workgroup of the limiter


def _assert_body(got, want, word, what):
    """Byte equality; in the float forms a NaN must be a NaN where the mirror has one (sign and payload apart)."""
    assert len(got) == len(want), f"{what}: {len(got)} bytes, the mirror has {len(want)}"
    if word & 0xFF in (0, 1, 3):
        head = 44 if word & 0xFF == 3 else 0
        assert got[:head] == want[:head], f"{what}: header"
        g, w = np.frombuffer(got[head:], dtype="<u4"), np.frombuffer(want[head:], dtype="<u4")
        wn = np.isnan(w.view("<f4"))
        np.testing.assert_array_equal(np.isnan(g.view("<f4")), wn, err_msg=what)
        bad = np.flatnonzero((g != w) & ~wn)
        assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} samples differ, the first at {int(bad[0])}"
    else:
        assert got == want, what


def _raw_of(x):
    return x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()


def _check(z, word, spec, out, body, what):
    """One limited request against the mirror on its stream z (at the word's rate), as the module's docstring says.
    Returns the mirror's (z2, p, g, I, n_g, r)."""
    from kokorox_amd import voices as V
    z = np.ascontiguousarray(z, dtype=np.float32)
    want = V.limit_stream(z, spec, word)
    z2, p, g, I, n_g, r = want
    got_p, got_g, got_I, got_ng, got_r = (float(v) for v in out)
    print(f"{what}: p {got_p} g {got_g} I {got_I} n_g {got_ng} r {got_r}; mirror g {g} I {I} r {r}")
    assert got_p == float(p) and got_ng == n_g, what
    if spec[0] & 0xFF == GAIN:
        assert got_g == g and np.isnan(got_I) and got_ng == 0, what
    else:
        if np.isnan(I):
            assert np.isnan(got_I), what
        else:
            assert abs(got_I - I) <= 1e-8, what
        capped = 0 < float(p) < np.inf and g == float(np.float64(4.0) * np.float64(np.float32(spec[3])) / np.float64(p))
        assert (got_g == g) if capped else (abs(got_g - g) <= 1e-8 * g), what
        want = V.limit_stream(z, spec, word, g=got_g)
        z2, r = want[0], want[5]
    assert got_r == r, what
    _assert_body(_raw_of(body), V.stream_body(z2, word), word, what)
    fin = z2[np.isfinite(z2)]
    assert fin.shape[0] == 0 or float(np.abs(fin).max()) <= float(np.float32(spec[3])), what
    return want


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


def _speechlike(rng, n, level=0.1, bursts=6):
    """Noise at `level` with a few short bursts some ten times above it: a crest factor a limiter is for."""
    x = level * rng.standard_normal(n)
    for at in rng.integers(0, n, bursts):
        w = int(rng.integers(1, 90))
        x[at: at + w] *= rng.uniform(4.0, 12.0)
    return x.astype(np.float32)


def _stream(x, word):
    from kokorox_amd import voices as V
    return V.resample_stream(x, word)


# ---- the hook -------------------------------------------------------------------------------------------------------------------
def test_hook_one_and_nine_frames_at_all_rates_and_forms_both_modes_with_and_without_the_flag():
    """1 frame and 9 frames: N = 600 and 5400 at 24 kHz, 200 .. 10800 elsewhere -- one, two and three windows.  All in one launch."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(4100)
    reqs = []
    i = 0
    for code in (0, 1, 2, 3):
        for form in (0, 2, 4, 8):
            for frames in (1, 9):
                flag = TRUE if (i // 2) % 2 else 0
                spec = (GAIN | flag, 2.5, 0.0, 0.5) if i % 2 == 0 else (LOUD | flag, 1.0, -14.0, 0.25)
                reqs.append((_speechlike(rng, 600 * frames), form | code << 8, spec))
                i += 1
    a, dur, lens = _rows([x for x, _, _ in reqs])
    bodies, samples, _, out, _, _ = hk.limit_requests(a, dur, lens, [1] * len(reqs), [w for _, w, _ in reqs], [s for _, _, s in reqs])
    limited = 0
    for r, (x, word, spec) in enumerate(reqs):
        z = _stream(x, word)
        assert samples[r] == z.shape[0]
        want = _check(z, word, spec, out[r], bodies[r], f"request {r} word {word:#x} spec {spec} N {z.shape[0]}")
        limited += want[5] < 1.0
    assert limited >= len(reqs) // 2  # (the inputs do drive the limiter)


def _click_request(N, at, level=0.02):
    at = list(at) if isinstance(at, (list, tuple)) else [at]
    rng = np.random.default_rng(77 + sum(at))
    x = (level * rng.standard_normal(N)).astype(np.float32)
    for p in at:
        x[p] = 0.9 if p % 2 == 0 else -0.9
    return x


@pytest.mark.parametrize("flag", [0, TRUE], ids=["sample", "true_peak"])
def test_hook_peaks_at_window_boundaries_and_stream_ends(flag):
    """A single peak at the window boundary +-1 and +-W, at n = 0 and at n = N - 1, and two peaks closer than W; 24 kHz, so the
    positions are the stream's own (W = 120), N = 5400 and 9000: two and three windows."""
    from kokorox_amd import hip_koko as hk
    W = 120
    cases = [(5400, p) for p in (0, 5399, WINDOW - 1, WINDOW, WINDOW + 1, WINDOW - W, WINDOW + W, WINDOW - W - 1, WINDOW + W + 1, WINDOW - 2 * W,
                                 WINDOW + 2 * W, [WINDOW - 30, WINDOW + 40])]
    cases += [(9000, p) for p in (2 * WINDOW, 2 * WINDOW - 1, 2 * WINDOW - W, [0, 8999], [WINDOW - 1, WINDOW, 2 * WINDOW - 1, 2 * WINDOW])]
    parts = [_click_request(N, at) for N, at in cases]
    spec = (GAIN | flag, 1.0, 0.0, 0.25)
    a, dur, lens = _rows(parts)
    bodies, _, _, out, _, _ = hk.limit_requests(a, dur, lens, [1] * len(cases), [0] * len(cases), [spec] * len(cases))
    for r, (N, at) in enumerate(cases):
        want = _check(parts[r], 0, spec, out[r], bodies[r], f"N {N} peak at {at} flag {flag:#x}")
        assert want[5] < 0.3  # (0.25 / 0.9: the peak is limited, whichever workgroup owns it)


def test_hook_peaks_at_window_boundaries_at_48_khz():
    """The resampled run: a click in the source near output samples 4096 and 8192 (W = 240), N = 10800."""
    from kokorox_amd import hip_koko as hk
    parts = [_click_request(5400, at) for at in (2047, 2048, 2049, 2048 - 120, 2048 + 120, 4096, 4095, [2048, 4096], 0, 5399)]
    specs = [(GAIN | (TRUE if r % 2 else 0), 1.5, 0.0, 0.25) for r in range(len(parts))]
    a, dur, lens = _rows(parts)
    bodies, _, _, out, _, _ = hk.limit_requests(a, dur, lens, [1] * len(parts), [0x300] * len(parts), specs)
    for r, x in enumerate(parts):
        _check(_stream(x, 0x300), 0x300, specs[r], out[r], bodies[r], f"48 kHz request {r}")


def test_hook_a_nan_an_inf_and_a_quiet_request_in_one_batch():
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    rng = np.random.default_rng(4102)
    nan = _speechlike(rng, 5400)
    nan[[0, 700, WINDOW, 5399]] = np.nan
    inf = _speechlike(rng, 5400)
    inf[[3, WINDOW - 1, 5000]] = [np.inf, -np.inf, np.inf]
    quiet = (0.01 * rng.standard_normal(5400)).astype(np.float32)
    parts = [nan, inf, quiet, nan, inf, quiet]
    specs = [(GAIN, 2.0, 0.0, 0.5)] * 3 + [(GAIN | TRUE, 2.0, 0.0, 0.5)] * 3
    a, dur, lens = _rows(parts)
    bodies, _, _, out, _, _ = hk.limit_requests(a, dur, lens, [1] * 6, [0] * 6, specs)
    for r in range(6):
        want = _check(parts[r], 0, specs[r], out[r], bodies[r], f"request {r}")
        z2 = np.frombuffer(bodies[r], dtype="<f4")
        assert np.array_equal(np.isnan(z2), np.isnan(parts[r]))
        assert np.all(np.abs(z2[np.isinf(parts[r])]) == np.float32(0.5))  # (+-inf becomes +-peak)
    for r in (2, 5):  # nothing limited: the levelled stream's bits, r = 1
        assert bodies[r] == V.level_stream(quiet, (0, 2.0, 0.0)).tobytes() and float(out[r][4]) == 1.0


def test_hook_a_join_with_a_pause_and_marks():
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    rng = np.random.default_rng(4103)
    x = _speechlike(rng, 60000, bursts=30)
    parts = [x[:18000], x[18000:45000], x[45000:]]
    a, dur, lens = _rows(parts)
    durs = [[int(v) for v in dur[b, : lens[b]]] for b in range(3)]
    for word, spec in ((0x000, (GAIN | TRUE, 3.0, 0.0, 0.5)), (0x204, (LOUD, 1.0, -12.0, 0.5)), (0x302, (GAIN, 3.0, 0.0, 0.25))):
        bodies, samples, marks, out, _, _ = hk.limit_requests(a, dur, lens, [3], [word], [spec], joins=[JOIN], want=[1])
        z = V.resample_stream(V.join_stream(parts, durs, JOIN), word)
        assert samples == [z.shape[0]]
        want = _check(z, word, spec, out[0], bodies[0], f"joined, word {word:#x} spec {spec}")
        assert want[5] < 1.0
        np.testing.assert_array_equal(marks[0], V.joined_marks(durs, word, JOIN))


def test_hook_plain_levelled_and_metered_requests_beside_a_limited_one_keep_their_bytes():
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(4104)
    parts = [_speechlike(rng, 600 * f) for f in (19, 100, 16, 19, 30)]
    words = [0x104, 0x000, 0x302, 0x003, 0x200]
    levels = [(0, 1.0, 0.0), (0, 1.0, 0.0), (1, 1.0, 0.5), (2 | TRUE, 8.0, 0.75), (0, 1.0, 0.0)]
    louds = [LOUD_NONE, (1, -23.0, 1.0), LOUD_NONE, LOUD_NONE, LOUD_NONE]
    a, dur, lens = _rows(parts)
    want_bodies, want_samples, _, want_ld, _ = hk.loudness_requests(a, dur, lens, [1] * 5, words, louds, levels=levels)
    # (the third spec's drive stays under the cap: its g is the meter's, compared within the meter's bound)
    for spec in ((GAIN, 4.0, 0.0, 0.25), (LOUD | TRUE, 1.0, -10.0, 0.5), (LOUD, 1.0, -30.0, 0.125)):
        limits = [NONE, NONE, NONE, NONE, spec]
        bodies, samples, _, out, out_lv, out_ld = hk.limit_requests(a, dur, lens, [1] * 5, words, limits, levels=levels, loudness=louds)
        assert samples == want_samples
        for r in range(4):
            assert bodies[r] == want_bodies[r] and out_lv[r].tolist() == want_ld[r][:2].tolist() and out[r].tolist() == [-1.0] * 5, r
        assert out_ld[1].tolist() == want_ld[1].tolist()
        _check(_stream(parts[4], 0x200), 0x200, spec, out[4], bodies[4], f"the limited request of the mixed launch, {spec}")
        assert bodies[4] != want_bodies[4]
    # a request alone and beside the others: the same bytes and the same five values
    alone = hk.limit_requests(a[4:], dur[4:], lens[4:], [1], words[4:], [spec])
    assert alone[0][0] == bodies[4] and alone[3][0].tolist() == out[4].tolist()


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _chunks():
    from oracle import kokoro_ref as R
    return [list(int(v) for v in R.synthetic_inputs(1, k, seed=500 + k)[0]) for k in (9, 10, 11)]


def test_model_limited_requests_equal_the_mirror_of_the_unlimited_stream(hip_model):
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    toks = _chunks()
    rows = [tab[b % 4, len(t) - 2, 0] for b, t in enumerate(toks)]
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations([3, 3, 3, 4])
    try:
        kw = dict(styles=rows, speeds=[1.0], seed=23)
        for code, joins, form, cpr in ((0, None, 0, [3]), (3, JOIN, 2, [1, 2]), (1, None, 8, [2, 1]), (2, JOIN, 4, [3])):
            word = form | code << 8
            if joins is None:
                z, zmarks, zsamples = hip_model.infer_requests_marks(toks, cpr, fmt=code << 8, with_samples=True, **kw)
            else:
                z, zmarks, zsamples = hip_model.infer_requests_joined(toks, cpr, joins, fmt=code << 8, marks=True, with_samples=True, **kw)
            peak = float(np.float32(0.5 * max(float(np.abs(s).max()) for s in z)))
            peak = min(max(peak, 2.0 ** -15), 1.0)
            specs = [(GAIN | (TRUE if code else 0), 2.0, 0.0, peak), (LOUD, 1.0, -12.0, peak)][: len(cpr)]
            bodies, marks, out, samples = hip_model.infer_requests_limited(toks, cpr, specs, joins=joins, fmt=word, marks=True,
                                                                           with_samples=True, **kw)
            assert samples == zsamples and out.shape == (len(cpr), 5)
            for r in range(len(cpr)):
                want = _check(z[r], word, specs[r], out[r], bodies[r], f"word {word:#x} joins {joins} request {r}")
                assert want[5] < 1.0
                np.testing.assert_array_equal(marks[r], zmarks[r])
    finally:
        hip_model.set_pinned_durations(None)


def test_tts_request_takes_a_limit(hip_model):
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    styles = {"v": W.synthetic_voices(1)[0]}
    chunks = [[5, 9, 12, 4, 8, 20, 6], [7, 3, 11, 2, 9]]
    hip_model.set_utterance_base(0)
    plain = V.tts_request(hip_model, styles, "v", chunks, seed=4, fmt=0x200)
    peak = float(np.float32(min(max(0.5 * float(np.abs(plain).max()), 2.0 ** -15), 1.0)))
    spec = (GAIN | TRUE, 1.0, 0.0, peak)
    got = V.tts_request(hip_model, styles, "v", chunks, seed=4, fmt=0x200, limit=spec)
    assert got.tobytes() == V.limit_stream(plain, spec, 0x200)[0].tobytes() and float(np.abs(got).max()) <= peak
    assert got.tobytes() != plain.tobytes()


def _raw_call(model, toks, cpr, rows, fmt, specs, n=None, null=False):
    """kx_infer_requests_limited as C callers make it; returns (rc, message, *out after the call)."""
    from kokorox_amd import hip_koko as hk
    ids, lens = model._ids_lens(toks)
    cp = np.ascontiguousarray(cpr, dtype=np.int32)
    st = np.ascontiguousarray(rows, dtype=np.float32)
    sp, fm = np.ones(1, dtype=np.float32), np.array([fmt], dtype=np.int32)
    lm = np.array(specs, dtype=hk.LIMIT_DTYPE)
    out, nb, ns = C.c_void_p(0xDEAD0), np.zeros(len(cpr), np.int64), np.zeros(len(cpr), np.int64)
    rc = model._lib.kx_infer_requests_limited(model._h, hk._ptr(ids), ids.shape[1], hk._ptr(lens), len(toks), hk._ptr(cp), len(cpr), hk._ptr(st),
                                              None, None, 0, hk._ptr(sp), 1, 1, 0, hk._ptr(fm), 1, C.byref(out), hk._ptr(nb), hk._ptr(ns), None,
                                              None, None, 0, None if null else hk._ptr(lm), len(specs) if n is None else n, None)
    if rc == 0:
        assert out.value and out.value != 0xDEAD0, "an accepted call returns a buffer"
        model._lib.kx_free_packed(out)
    else:
        assert out.value is None, "a refused call leaves *out null: nothing to release"
    return rc, model._lib.kx_last_error(model._h).decode() if rc else ""


def test_refusals_and_the_rules_of_out(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    toks = _chunks()
    rows = [tab[b % 4, len(t) - 2, 0] for b, t in enumerate(toks)]
    ok, ok1 = (GAIN, 2.0, 0.0, 0.5), (LOUD | TRUE, 1.0, -16.0, 1.0)
    hip_model.set_pinned_durations([1])
    try:
        call = lambda *a, **k: _raw_call(hip_model, toks, [1, 2], rows, 0, *a, **k)  # noqa: E731
        assert call([ok]) == (0, "") and call([ok, ok1]) == (0, "") and call([(GAIN | TRUE, 0.0, 0.0, 2.0 ** -15)]) == (0, "")
        assert call([ok], null=True) == (1, "infer: null limit argument")
        assert call([ok], n=0) == (1, "infer: bad limit count") and call([ok, ok, ok]) == (1, "infer: bad limit count")
        for bad in ((2, 1.0, 0.0, 0.5), (0x200, 1.0, 0.0, 0.5), (0x80000000, 1.0, 0.0, 0.5), (0, 65.0, 0.0, 0.5), (0, -1.0, 0.0, 0.5),
                    (0, 1.0, -1.0, 0.5), (0, 1.0, -0.0, 0.5), (0, 1.0, 0.0, 2.0), (0, 1.0, 0.0, 2.0 ** -16), (0, 1.0, 0.0, 0.0),
                    (1, 2.0, -16.0, 0.5), (1, 1.0, 1.0, 0.5), (1, 1.0, -71.0, 0.5), (1, 1.0, -16.0, 1.5), (0, float("nan"), 0.0, 0.5),
                    (0, 1.0, 0.0, float("nan")), (1, 1.0, float("nan"), 0.5), NONE):
            assert call([ok, bad]) == (1, "infer: bad limit"), bad
        assert _raw_call(hip_model, toks, [1, 2], rows, 5, [ok]) == (1, "infer: unknown output format")  # (the older refusals speak first)
        # marks live inside the allocation of *out (the wrapper checks alignment and range before it releases the buffer)
        bodies, marks, out = hip_model.infer_requests_limited(toks, [1, 2], ok, styles=rows, seed=1, marks=True)
        assert len(marks) == 2 and marks[0].shape[0] == len(toks[0]) + 1 and out.shape == (2, 5)
        d = hk.Dispatcher([hip_model], max_batch=4, max_wait_us=0)
        try:
            body, five = d.submit_request([toks[0]], styles=[rows[0]], limit=ok)
            assert five.shape == (5,) and np.isnan(five[2])
            for bad in ((2, 1.0, 0.0, 0.5), (0, 1.0, 0.0, 2.0), (1, 2.0, -16.0, 0.5), NONE):
                with pytest.raises(hk.KokoroxHipError, match="dispatcher_submit_request: bad limit"):
                    d.submit_request([toks[0]], styles=[rows[0]], limit=bad)
            with pytest.raises(hk.KokoroxHipError, match="dispatcher_submit_request: bad join"):
                d.submit_request([toks[0]], styles=[rows[0]], limit=ok, join=(8, 0, 0, 0))
        finally:
            d.close()
    finally:
        hip_model.set_pinned_durations(None)


# ---- the dispatcher -------------------------------------------------------------------------------------------------------------
def _request_specs():
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    tab = W.synthetic_voices(4)
    words = [0, 0x108, 0x302, 4, 0x202, 0x109, 3, 0x301]
    joins = [(HEAD | TAIL | INNER, 20, 150, 5), None, (INNER, 0, 85, 12), None]
    kinds = [("limit", (GAIN, 2.0, 0.0, 2.0 ** -6)), ("plain", None), ("level", (1, 1.0, 0.5)), ("limit", (LOUD | TRUE, 1.0, -12.0, 2.0 ** -5)),
             ("loudness", (1, -23.0, 1.0)), ("limit", (GAIN | TRUE, 8.0, 0.0, 2.0 ** -4))]
    specs = []
    for i in range(16):
        n = 1 + i % 3
        chunks = [list(int(v) for v in R.synthetic_inputs(1, 8 + (5 * i + 3 * c) % 4, seed=900 + 10 * i + c)[0]) for c in range(n)]
        voice = dict(styles=[tab[i % 4, len(c) - 2, 0] for c in chunks]) if i % 2 == 0 else dict(voices=i % 4)
        kind, spec = kinds[i % len(kinds)]
        specs.append(dict(chunks=chunks, voice=voice, fmt=words[i % len(words)], seed=9700 + i, speed=1.0 + 0.125 * (i % 2),
                          marks=(i // 3) % 2 == 0, join=joins[i % len(joins)], kind=kind, spec=spec))
    return tab, specs


def _alone(model, s):
    """The request through the direct call with R = 1: (body, marks or None, the entry's values or None)."""
    n = len(s["chunks"])
    v = s["voice"]
    kw = dict(styles=v["styles"]) if "styles" in v else dict(voice_ids=[[v["voices"]]] * n, weights=[[0.0]] * n)
    kw.update(speeds=[s["speed"]], seed=s["seed"], fmt=s["fmt"])
    if s["kind"] == "plain":
        join = s["join"] if s["join"] is not None else (0, 0, 0, 0)
        if s["marks"]:
            bodies, marks = model.infer_requests_joined(s["chunks"], [n], join, marks=True, **kw)
            return bodies[0], marks[0], None
        return model.infer_requests_joined(s["chunks"], [n], join, **kw)[0], None, None
    call = {"limit": model.infer_requests_limited, "loudness": model.infer_requests_loudness, "level": model.infer_requests_levelled}[s["kind"]]
    res = call(s["chunks"], [n], s["spec"], joins=s["join"], marks=s["marks"], **kw)
    return (res[0][0], res[1][0], res[2][0]) if s["marks"] else (res[0][0], None, res[1][0])


def test_dispatcher_eight_clients_of_mixed_kinds_equal_their_solo_runs(hip_model):
    """8 client threads, 16 requests of 1..3 chunks of about ten tokens: limited (both modes, with and without the flag), metered,
    levelled and plain requests, with and without joins and marks, rates and forms mixed; a request's bytes, marks and values equal
    the direct call of the request alone."""
    from kokorox_amd import hip_koko as hk
    tab, specs = _request_specs()
    hip_model.set_voice_table(tab)
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations(None)
    d = hk.Dispatcher([hip_model], max_batch=8, max_wait_us=100000)
    out = [None] * len(specs)
    errs = []

    def client(t):
        try:
            for i in (t, t + 8):
                s = specs[i]
                kind = {s["kind"]: s["spec"]} if s["kind"] != "plain" else {}
                out[i] = d.submit_request(s["chunks"], speed=s["speed"], seed=s["seed"], fmt=s["fmt"], marks=s["marks"], join=s["join"],
                                          **kind, **s["voice"])
        except Exception as e:  # pragma: no cover
            errs.append(e)

    try:
        th = [threading.Thread(target=client, args=(t,)) for t in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        st = d.stats()
    finally:
        d.close()
    assert not errs, errs
    limited = 0
    for i, s in enumerate(specs):
        body, marks, vals = _alone(hip_model, s)
        got = out[i] if isinstance(out[i], tuple) else (out[i],)
        assert _raw_of(got[0]) == _raw_of(body) and type(got[0]) is type(body), i
        if s["marks"]:
            np.testing.assert_array_equal(got[1], marks)
        if vals is not None:
            assert got[-1].tobytes() == np.ascontiguousarray(vals, dtype=np.float64).tobytes(), (i, got[-1], vals)
        if s["kind"] == "limit":
            assert got[-1].shape == (5,)
            limited += float(got[-1][4]) < 1.0
    assert limited >= 4  # (the limiter did act inside the batches)
    assert st["requests"] == len(specs) and st["batches"] < st["requests"]
