"""GPU: loudness (include/kokorox_hip.h, "loudness") -- the BS.1770 meter (request_loudness_kernel), its gating and gain
(request_loudness_gain_kernel) and the levelled packer behind them, through their test hook, through kx_infer_requests_loudness
and through the dispatcher, against the numpy float64 definition of kokorox_amd/voices.py.

Tolerances.  sum |h| of the K-weighting is at most 3.35 at every rate, so float64 rounding and the 1e-15 warm-up tail give errors
near 1e-14 max|x| per weighted sample, far below 1e-9 relative on any block above the absolute gate:
    |e_k - mirror| <= 1e-9 hop max|x|^2,   |I - mirror| <= 1e-8 LU,   |g - mirror| <= 1e-8 g,   n_g equal to the mirror's
(every input has margin >= 1e-6: no block mean lies that close to a gate threshold).  The body is bit-exact: it equals
voices.loudness_body of the stream with the gain the GPU reported."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORMS = [0, 8, 3, 1, 4, 9, 2]
HEAD, TAIL, INNER = 1, 2, 4
MEASURE, NORMALIZE = 0, 1
METER = (MEASURE, 0.0, 0.0)
NONE = (0xFFFFFFFF, 0.0, 0.0)  # the hook only: a request that is not metered
RATES = {0: 24000, 1: 8000, 2: 16000, 3: 48000}
JOIN = (HEAD | TAIL | INNER, 10, 85, 5)


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


def _check(z, word, spec, out, hops, body, what, seen=None):
    """One metered request against the mirror on its stream z (at the word's rate): e[k], I, n_g, p and g within the bounds of
    the module's docstring, the body bit-exact with the GPU's gain.  Returns (I, n_g, g)."""
    from kokorox_amd import voices as V
    rate = RATES[word >> 8]
    hop = rate // 10
    e = V.hop_energies(z, rate)
    assert hops.shape == e.shape == (z.shape[0] // hop,), what
    fin = z[np.isfinite(z)]
    peak_x = float(np.abs(fin).max()) if fin.shape[0] else 0.0
    assert peak_x <= 4.0, what
    dev_e = float(np.abs(hops - e).max()) if e.shape[0] else 0.0
    I, n_g, margin = V.gated_loudness(e, rate)
    assert margin >= 1e-6, f"{what}: a block mean within {margin} of a gate threshold (the input is at fault)"
    p, _ = V.level_gain(z, None)
    g = V.loudness_gain(p, I, spec)
    got_p, got_g, got_I, got_ng = (float(v) for v in out)
    dev_I = 0.0 if np.isnan(I) else abs(got_I - I)
    print(f"{what}: max |e_k - mirror| = {dev_e:.3e} (bound {1e-9 * hop * peak_x ** 2:.3e}), |I - mirror| = {dev_I:.3e}, "
          f"|g - mirror| / g = {abs(got_g - g) / g:.3e}, I = {got_I}, n_g = {got_ng}")
    if seen is not None:
        seen.append((dev_e / (hop * peak_x ** 2) if peak_x else 0.0, dev_I, abs(got_g - g) / g))
    assert dev_e <= 1e-9 * hop * peak_x ** 2, what
    assert got_ng == n_g and float(got_p) == float(p), what
    if np.isnan(I):
        assert np.isnan(got_I) and n_g == 0, what
    else:
        assert dev_I <= 1e-8, what
    assert abs(got_g - g) <= 1e-8 * g, what
    _assert_body(body, V.loudness_body(z, got_g, word), word, what)
    return got_I, got_ng, got_g


# ---- the hook's inputs ---------------------------------------------------------------------------------------------------------
def _signals():
    """name -> (24 kHz samples, a whole number of frames): the contents the issue of the meter names."""
    rng = np.random.default_rng(20270)
    n100 = 60000
    t = np.arange(96000) / 24000.0
    burst = (10.0 ** (-60 / 20) * rng.uniform(-1, 1, n100)).astype(np.float32)
    burst[:12000] = np.sin(2 * np.pi * 100.0 * t[:12000]).astype(np.float32)  # 0.5 s at full scale: its filter tail crosses hops
    gate = np.zeros(96000, dtype=np.float32)                                     # 1 s loud, 2 s at -50 dBFS, 1 s of zeros
    gate[:24000] = 0.5 * rng.uniform(-1, 1, 24000)
    gate[24000:72000] = 10.0 ** (-50 / 20) * rng.uniform(-1, 1, 48000)
    nonfinite = rng.uniform(-0.5, 0.5, n100).astype(np.float32)
    nonfinite[[0, 5, 2399, 2400, 30000, 59999]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
    return {
        "noise15": rng.uniform(-0.5, 0.5, 9000).astype(np.float32), "noise16": rng.uniform(-0.5, 0.5, 9600).astype(np.float32),
        "noise19": rng.uniform(-0.5, 0.5, 11400).astype(np.float32), "noise100": rng.uniform(-0.5, 0.5, n100).astype(np.float32),
        "loud100": rng.uniform(-2.0, 2.0, n100).astype(np.float32), "burst": burst, "gate": gate, "nonfinite": nonfinite,
        "sine": (0.25 * np.sin(2 * np.pi * 997.0 * t[:30000])).astype(np.float32),
    }


def _rows(parts):
    """Rows for the hook from 24 kHz streams: every row three tokens whose durations add up to its frames (dur, lens), the audio
    poisoned behind each row's samples."""
    B = len(parts)
    frames = [p.shape[0] // 600 for p in parts]
    assert all(p.shape[0] == 600 * f and f >= 3 for p, f in zip(parts, frames))
    dur = np.full((B, 512), -7, dtype=np.int32)
    a = np.empty((B, 600 * max(frames) + 77), dtype=np.float32)
    for b, (p, f) in enumerate(zip(parts, frames)):
        dur[b, :3] = [2, f - 3, 1]
        a[b, : p.shape[0]] = p
        a[b, p.shape[0]:] = np.array([1e30, np.inf, -np.inf, np.nan], dtype=np.float32)[(np.arange(a.shape[1] - p.shape[0]) + b) % 4]
    return a, dur, [3] * B


@pytest.fixture(scope="module")
def signals():
    return _signals()


@pytest.fixture(scope="module")
def big_launch(signals):
    """Everything in ONE launch: requests of different rates and lengths side by side, so the meter's grid covers the longest
    and the shorter ones return early; one request of three joined chunks."""
    from kokorox_amd import hip_koko as hk
    s = signals
    reqs = [("noise15", 0x000, METER), ("noise16", 0x003, (NORMALIZE, -23.0, 1.0)), ("noise19", 0x002, (NORMALIZE, -16.0, 1.0)),
            ("noise100", 0x000, (NORMALIZE, -23.0, 1.0)), ("noise100", 0x108, (NORMALIZE, -30.0, 0.5)), ("noise100", 0x204, METER),
            ("noise100", 0x300, (NORMALIZE, -6.0, 0.25)), ("loud100", 0x300, (NORMALIZE, -23.0, 1.0)), ("burst", 0x000, METER),
            ("burst", 0x303, (NORMALIZE, -23.0, 1.0)), ("gate", 0x000, (NORMALIZE, -23.0, 1.0)), ("gate", 0x102, METER),
            ("nonfinite", 0x000, (NORMALIZE, -23.0, 1.0)), ("sine", 0x000, METER), ("sine", 0x100, METER), ("sine", 0x200, METER),
            ("sine", 0x300, METER)]
    parts, cpr, words, specs, joins = [], [], [], [], []
    for name, word, spec in reqs:
        parts.append(s[name])
        cpr.append(1)
        words.append(word)
        specs.append(spec)
        joins.append((0, 0, 0, 0))
    # the joined request: 100 frames as three chunks of 30, 45 and 25, trimmed, paused and faded
    x = s["noise100"]
    parts += [x[:18000], x[18000:45000], x[45000:]]
    cpr.append(3)
    words.append(0x200)
    specs.append((NORMALIZE, -20.0, 1.0))
    joins.append(JOIN)
    a, dur, lens = _rows(parts)
    bodies, samples, _, out, hops = hk.loudness_requests(a, dur, lens, cpr, words, specs, joins=joins)
    return dict(reqs=reqs, parts=parts, dur=dur, lens=lens, bodies=bodies, samples=samples, out=out, hops=hops, specs=specs, words=words)


def _stream(x, word):
    from kokorox_amd import voices as V
    return V.resample_stream(x, word)


def test_hook_one_launch_of_every_shape_content_and_rate(big_launch, signals):
    from kokorox_amd import voices as V
    L = big_launch
    seen, res = [], {}
    for r, (name, word, spec) in enumerate(L["reqs"]):
        z = _stream(signals[name], word)
        assert L["samples"][r] == z.shape[0]
        res[(name, word)] = _check(z, word, spec, L["out"][r], L["hops"][r], L["bodies"][r], f"request {r} {name} word {word:#x} spec {spec}", seen)
    # the shapes: three hops and no block; exactly one block; one block and a partial hop that is ignored
    assert np.isnan(res[("noise15", 0x000)][0]) and res[("noise15", 0x000)][1:] == (0, 1.0) and L["hops"][0].shape == (3,)
    assert res[("noise16", 0x003)][1] == 1 and L["hops"][1].shape == (4,)
    assert res[("noise19", 0x002)][1] == 1 and L["hops"][2].shape == (4,)
    assert L["hops"][3].shape == (25,) and res[("noise100", 0x000)][1] == 22
    # the gate case: the relative gate and the absolute gate each remove blocks (40 hops, 37 blocks)
    e = V.hop_energies(signals["gate"], 24000)
    zj = (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / 9600.0
    n_abs = int((zj > V.LOUDNESS_ABS_GATE).sum())
    assert zj.shape == (37,) and res[("gate", 0x000)][1] < n_abs < 37
    # the ceiling engaged where the target asks for more than the peak allows: the largest |sample| is exactly `peak`
    r = [i for i, q in enumerate(L["reqs"]) if q[:2] == ("noise100", 0x300)][0]
    assert float(np.abs(np.frombuffer(L["bodies"][r], dtype="<f4")).max()) == 0.25 and L["out"][r][1] == 0.25 / L["out"][r][0]
    # the 997 Hz anchor of EBU Tech 3341: 20 log10(A) - 3.0103 within 0.1 LU at every rate
    for code in range(4):
        assert abs(res[("sine", code << 8)][0] - (20 * np.log10(0.25) - 3.0103)) <= 0.1, code
    # a NaN stays a NaN in the body, and the infinities keep p from being usable: g is the loudness gain alone
    r = [i for i, q in enumerate(L["reqs"]) if q[0] == "nonfinite"][0]
    body = np.frombuffer(L["bodies"][r], dtype="<f4")
    assert np.isnan(body[[0, 2400]]).all() and np.isinf(body[[5, 2399, 30000, 59999]]).all() and L["out"][r][0] == np.inf
    # the joined request: the staged stream differs from the rows
    r = len(L["reqs"])
    d = [[int(v) for v in L["dur"][b, :3]] for b in range(r, r + 3)]
    z = _stream(V.join_stream(L["parts"][r:], d, JOIN), 0x200)
    assert z.shape[0] != 40000 and L["samples"][r] == z.shape[0]
    _check(z, 0x200, L["specs"][r], L["out"][r], L["hops"][r], L["bodies"][r], "joined request", seen)
    print("largest deviations of the launch: e_k / (hop max|x|^2) %.3e, I %.3e LU, g %.3e relative" % tuple(max(v[i] for v in seen) for i in range(3)))


def test_hook_body_in_all_seven_forms_at_two_rates(signals):
    from kokorox_amd import hip_koko as hk
    x = signals["noise19"]
    words = [f | code << 8 for code in (0, 1) for f in FORMS]
    specs = [(NORMALIZE, -23.0, 1.0) if i % 2 else (NORMALIZE, -3.0, 0.5) for i in range(len(words))]
    a, dur, lens = _rows([x] * len(words))
    bodies, samples, _, out, hops = hk.loudness_requests(a, dur, lens, [1] * len(words), words, specs)
    for r, word in enumerate(words):
        _check(_stream(x, word), word, specs[r], out[r], hops[r], bodies[r], f"word {word:#x} spec {specs[r]}")
        if specs[r][2] == 0.5:  # (the ceiling case: target -3 LUFS is beyond what a peak of 0.5 allows)
            assert float(out[r][1]) == 0.5 / float(out[r][0])
    assert float(np.abs(np.frombuffer(bodies[0], dtype="<f4")).max()) == 0.5


def test_hook_a_request_alone_and_beside_three_others_gives_the_same_bits(big_launch, signals):
    """Batch-independence: e[k], I, g and the body of a request do not depend on the grid or on which requests are beside it."""
    from kokorox_amd import hip_koko as hk
    L = big_launch
    for r in (3, 6, 9, 11):
        name, word, spec = L["reqs"][r]
        a, dur, lens = _rows([signals[name]])
        bodies, _, _, out, hops = hk.loudness_requests(a, dur, lens, [1], [word], [spec])
        assert hops[0].tobytes() == L["hops"][r].tobytes() and out[0].tobytes() == L["out"][r].tobytes(), (name, word)
        assert bodies[0] == L["bodies"][r], (name, word)
    # ... nor on being first or last among four
    parts = [signals["noise16"], signals["burst"], signals["noise100"], signals["gate"]]
    words, specs = [0x300, 0x000, 0x100, 0x200], [METER, (NORMALIZE, -23.0, 1.0), METER, (NORMALIZE, -18.0, 1.0)]
    fwd = hk.loudness_requests(*_rows(parts), [1] * 4, words, specs)
    rev = hk.loudness_requests(*_rows(parts[::-1]), [1] * 4, words[::-1], specs[::-1])
    for r in range(4):
        assert fwd[0][r] == rev[0][3 - r] and fwd[3][r].tobytes() == rev[3][3 - r].tobytes() and fwd[4][r].tobytes() == rev[4][3 - r].tobytes()


def test_hook_plain_and_levelled_requests_beside_metered_ones_keep_their_bytes(signals):
    from kokorox_amd import hip_koko as hk
    parts = [signals["noise19"], signals["noise100"], signals["noise16"], signals["noise19"]]
    words = [0x104, 0x000, 0x302, 0x003]
    levels = [(0, 1.0, 0.0), (0, 1.0, 0.0), (1, 1.0, 0.5), (2, 8.0, 0.75)]
    a, dur, lens = _rows(parts)
    want_bodies, want_samples, _, want_lv = hk.level_requests(a, dur, lens, [1] * 4, words, levels)
    specs = [NONE, (NORMALIZE, -23.0, 1.0), NONE, NONE]
    bodies, samples, _, out, hops = hk.loudness_requests(a, dur, lens, [1] * 4, words, specs, levels=levels)
    assert samples == want_samples
    for r in (0, 2, 3):
        assert bodies[r] == want_bodies[r] and out[r][:2].tolist() == want_lv[r].tolist() and hops[r].shape == (0,), r
    _check(signals["noise100"], 0x000, specs[1], out[1], hops[1], bodies[1], "the metered request of the mixed launch")
    assert bodies[1] != want_bodies[1]


# ---- the model ------------------------------------------------------------------------------------------------------------
def _chunks():
    from oracle import kokoro_ref as R
    return [list(int(v) for v in R.synthetic_inputs(1, k, seed=500 + k)[0]) for k in (1, 10, 3, 5, 2, 7)]


def _raw_of(x):
    return x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()


def _check_model(z, word, spec, out, body, what):
    """As _check, without the hop energies, which the public entries do not return."""
    from kokorox_amd import voices as V
    z = np.ascontiguousarray(z, dtype=np.float32)
    I, n_g, margin = V.integrated_loudness(z, RATES[word >> 8])
    assert margin >= 1e-6, what
    p, _ = V.level_gain(z, None)
    g = V.loudness_gain(p, I, spec)
    assert float(out[0]) == float(p) and float(out[3]) == n_g, what
    assert (np.isnan(out[2]) and np.isnan(I)) or abs(float(out[2]) - I) <= 1e-8, what
    assert abs(float(out[1]) - g) <= 1e-8 * g, what
    _assert_body(_raw_of(body), V.loudness_body(z, float(out[1]), word), word, what)


def test_model_loudness_requests_equal_the_mirror_of_its_own_form_0_result(hip_model):
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    toks = _chunks()
    rows = [tab[b % 4, len(t) - 2, 0] for b, t in enumerate(toks)]
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations([3, 3, 3, 4])
    cpr = [2, 1, 3]
    specs = [(NORMALIZE, -23.0, 1.0), METER, (NORMALIZE, -1.0, 0.5)]
    try:
        kw = dict(styles=rows, speeds=[1.0], seed=23)
        for code, joins, form in ((0, None, 0), (1, JOIN, 4), (2, None, 8), (3, JOIN, 3), (0, JOIN, 2)):
            word = form | code << 8
            if joins is None:
                z, zmarks, zsamples = hip_model.infer_requests_marks(toks, cpr, fmt=code << 8, with_samples=True, **kw)
            else:
                z, zmarks, zsamples = hip_model.infer_requests_joined(toks, cpr, joins, fmt=code << 8, marks=True, with_samples=True, **kw)
            bodies, marks, out, samples = hip_model.infer_requests_loudness(toks, cpr, specs, joins=joins, fmt=word, marks=True,
                                                                            with_samples=True, **kw)
            assert samples == zsamples and out.shape == (3, 4)
            for r in range(3):
                _check_model(z[r], word, specs[r], out[r], bodies[r], f"word {word:#x} joins {joins} request {r}")
                np.testing.assert_array_equal(marks[r], zmarks[r])
            assert float(out[1][1]) == 1.0 and float(out[2][1]) == 0.5 / float(out[2][0])  # the meter; the ceiling
        # the meter, shared, without marks: the bytes of the call without loudness
        meter, out = hip_model.infer_requests_loudness(toks, cpr, METER, fmt=0x100, **kw)
        z0 = hip_model.infer_requests(toks, cpr, fmt=0x100, **kw)
        for r in range(3):
            assert _raw_of(meter[r]) == _raw_of(z0[r]) and float(out[r][1]) == 1.0
    finally:
        hip_model.set_pinned_durations(None)


def test_tts_request_takes_a_loudness(hip_model):
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    styles = {"v": W.synthetic_voices(1)[0]}
    chunks = [[5, 9, 12, 4, 8, 20, 6], [7, 3, 11, 2, 9]]
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations([3, 3, 3, 4])
    try:
        plain = V.tts_request(hip_model, styles, "v", chunks, seed=4, fmt=0x200)
        got = V.tts_request(hip_model, styles, "v", chunks, seed=4, fmt=0x200, loudness=(NORMALIZE, -23.0, 1.0))
    finally:
        hip_model.set_pinned_durations(None)
    I, n_g, margin = V.integrated_loudness(plain, 16000)
    assert n_g >= 1 and margin >= 1e-6
    I2, _, _ = V.integrated_loudness(got, 16000)
    assert abs(I2 - -23.0) < 1e-3  # (a gain moves every block alike: the gates keep their blocks)


def _raw_call(model, toks, cpr, rows, fmt, specs, n=None, null=False):
    """kx_infer_requests_loudness as C callers make it; returns (rc, message)."""
    from kokorox_amd import hip_koko as hk
    ids, lens = model._ids_lens(toks)
    cp = np.ascontiguousarray(cpr, dtype=np.int32)
    st = np.ascontiguousarray(rows, dtype=np.float32)
    sp, fm = np.ones(1, dtype=np.float32), np.array([fmt], dtype=np.int32)
    ld = np.array(specs, dtype=hk.LOUDNESS_DTYPE)
    out, nb, ns = C.c_void_p(), np.zeros(len(cpr), np.int64), np.zeros(len(cpr), np.int64)
    rc = model._lib.kx_infer_requests_loudness(model._h, hk._ptr(ids), ids.shape[1], hk._ptr(lens), len(toks), hk._ptr(cp), len(cpr), hk._ptr(st),
                                               None, None, 0, hk._ptr(sp), 1, 1, 0, hk._ptr(fm), 1, C.byref(out), hk._ptr(nb), hk._ptr(ns), None,
                                               None, None, 0, None if null else hk._ptr(ld), len(specs) if n is None else n, None)
    if rc == 0:
        model._lib.kx_free_packed(out)
    assert rc != 0 or out.value, "an accepted call returns a buffer"
    return rc, model._lib.kx_last_error(model._h).decode() if rc else ""


def test_refusals(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    toks = _chunks()[:3]
    rows = [tab[b % 4, len(t) - 2, 0] for b, t in enumerate(toks)]
    ok = (NORMALIZE, -23.0, 1.0)
    call = lambda *a, **k: _raw_call(hip_model, toks, [1, 2], rows, 0, *a, **k)  # noqa: E731
    assert call([ok]) == (0, "") and call([ok, METER]) == (0, "")
    assert call([ok], null=True) == (1, "infer: null loudness argument")
    assert call([ok], n=0) == (1, "infer: bad loudness count") and call([ok, ok, ok]) == (1, "infer: bad loudness count")
    for bad in ((2, -23.0, 1.0), (0x80000001, -23.0, 1.0), (1, 1.0, 1.0), (1, -71.0, 1.0), (1, -23.0, 2.0), (0, -23.0, 0.0), (0, 0.0, 0.5),
                (1, float("nan"), 1.0), (1, -23.0, float("nan")), (1, -23.0, 2.0 ** -16), NONE):
        assert call([ok, bad]) == (1, "infer: bad loudness"), bad
    assert _raw_call(hip_model, toks, [1, 2], rows, 5, [ok]) == (1, "infer: unknown output format")  # (the older refusals speak first)
    d = hk.Dispatcher([hip_model], max_batch=4, max_wait_us=0)
    try:
        for bad in ((2, -23.0, 1.0), (1, 1.0, 1.0), (0, 0.0, 0.5), NONE):
            with pytest.raises(hk.KokoroxHipError, match="dispatcher_submit_request: bad loudness"):
                d.submit_request([toks[0]], styles=[rows[0]], loudness=bad)
        with pytest.raises(hk.KokoroxHipError, match="dispatcher_submit_request: bad join"):
            d.submit_request([toks[0]], styles=[rows[0]], loudness=ok, join=(8, 0, 0, 0))
    finally:
        d.close()


# ---- dispatcher ------------------------------------------------------------------------------------------------------------
def _request_specs():
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    tab = W.synthetic_voices(4)
    words = [0, 0x108, 0x303, 4, 0x202, 0x109, 3, 0x301]
    joins = [(HEAD | TAIL | INNER, 20, 150, 5), None, (INNER, 0, 85, 12), None]
    kinds = [("loudness", (NORMALIZE, -23.0, 1.0)), ("plain", None), ("level", (1, 1.0, 0.5)), ("loudness", METER), ("loudness", (NORMALIZE, -2.0, 0.5))]
    specs = []
    for i in range(16):
        n = 1 + i % 3
        chunks = [list(int(v) for v in R.synthetic_inputs(1, 4 + (5 * i + 3 * c) % 8, seed=900 + 10 * i + c)[0]) for c in range(n)]
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
    call = model.infer_requests_loudness if s["kind"] == "loudness" else model.infer_requests_levelled
    res = call(s["chunks"], [n], s["spec"], joins=s["join"], marks=s["marks"], **kw)
    return (res[0][0], res[1][0], res[2][0]) if s["marks"] else (res[0][0], None, res[1][0])


def test_dispatcher_mixed_requests_equal_their_solo_runs(hip_model):
    """8 client threads, 16 requests of 1..3 chunks: metered, levelled and plain, with and without joins and marks, rates and
    forms mixed; body, marks and the entry's values of each equal the direct call of the request alone, bit for bit."""
    from kokorox_amd import hip_koko as hk
    tab, specs = _request_specs()
    hip_model.set_voice_table(tab)
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations([3, 3, 3, 4])
    out, errs = [None] * len(specs), []

    def client(t):
        try:
            for i in (t, t + 8):
                s = specs[i]
                extra = {} if s["kind"] == "plain" else {s["kind"]: s["spec"]}
                out[i] = d.submit_request(s["chunks"], speed=s["speed"], seed=s["seed"], fmt=s["fmt"], marks=s["marks"], join=s["join"],
                                          **extra, **s["voice"])
        except Exception as e:  # pragma: no cover
            errs.append(e)

    try:
        d = hk.Dispatcher([hip_model], max_batch=8, max_wait_us=100000)
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
        defined = 0
        for i, s in enumerate(specs):
            body, marks, values = _alone(hip_model, s)
            got = out[i] if isinstance(out[i], tuple) else (out[i],)
            assert len(got) == 1 + int(s["marks"]) + int(s["kind"] != "plain"), i
            assert _raw_of(got[0]) == _raw_of(body), i
            if s["marks"]:
                np.testing.assert_array_equal(got[1], marks)
            if s["kind"] != "plain":
                assert got[-1].tobytes() == np.asarray(values, dtype=np.float64).tobytes(), (i, got[-1], values)
            if s["kind"] == "loudness":
                defined += int(not np.isnan(got[-1][2]) and got[-1][3] >= 1)
        assert defined >= 6 and st["requests"] == len(specs) and st["batches"] < st["requests"]
    finally:
        hip_model.set_pinned_durations(None)
