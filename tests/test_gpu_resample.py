"""GPU: output sample rates (8, 16, 48 kHz) and the G.711 forms of the request packer -- resample_requests_kernel and
pack_requests_kernel through the kernel's test hook, through kx_infer_requests and through the dispatcher.

Everything is checked by EQUALITY against the numpy mirrors of kokorox_amd/voices.py (`resample_stream`: the definition's
float64 sum in ascending order with the library's own taps; `mulaw_bytes` / `alaw_bytes`; the WAV bodies with their `rate`
argument).  The shapes are those of tests/test_gpu_wire_formats.py, the smallest at which this can go wrong: rows of
600 x [1, 2, 3, 5, 1, 1] samples in a slab of ld 3008 with NaN beyond every row's end; a one-frame request is 200 outputs at
8 kHz, shorter than the filter's support, so both stream edges sit in one window; [2, 1, 3] puts chunk boundaries inside the
support; [6] is 7800 samples -> 15 600 outputs at 48 kHz, several workgroup windows; 1, 2 and 3 frames give all three base64
paddings.  No subnormal and no infinite sample: their handling in the f32 -> f64 conversion is outside the definition."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = [1, 2, 3, 5, 1, 1]
LD = 3008
GROUPINGS = {"six_single": [1] * 6, "two_one_three": [2, 1, 3], "one_of_six": [6]}
FORMS = [0, 1, 2, 3, 4, 8, 9]
RATES = {0x000: (24000, 1, 1), 0x100: (8000, 1, 3), 0x200: (16000, 2, 3), 0x300: (48000, 2, 1)}


def _slab():
    """[6, LD] rows of 600 * FRAMES[b] valid samples, NaN beyond; +-1, +-0, 1 + ulp and 32766.5 / 32767 at 0, 1, 2, 599, 600 and
    the last two positions of every row."""
    rng = np.random.default_rng(4100)
    one_up = np.nextafter(np.float32(1), np.float32(2))
    vals = np.array([1.0, -1.0, 0.0, -0.0, one_up, 32766.5 / 32767, -32766.5 / 32767, -one_up], dtype=np.float32)
    a = np.full((len(FRAMES), LD), np.nan, dtype=np.float32)
    k = 0
    for b, f in enumerate(FRAMES):
        n = 600 * f
        a[b, :n] = rng.uniform(-1.3, 1.3, n).astype(np.float32)
        for pos in (0, 1, 2, 599, 600, n - 2, n - 1):
            if pos < n:
                a[b, pos] = vals[k % len(vals)]
                k += 1
    return a


def _streams(a, cpr):
    first = np.concatenate([[0], np.cumsum(cpr)])
    return [np.concatenate([a[b, : 600 * FRAMES[b]] for b in range(first[r], first[r + 1])]) for r in range(len(cpr))]


def _pcm16_form2(y):
    """Form 2's own conversion: fmax / fmin clamp (a NaN becomes -32767), the product rounded to f32, truncated."""
    c = np.where(np.isnan(y), np.float32(-1.0), np.clip(y, np.float32(-1.0), np.float32(1.0))).astype(np.float32)
    return np.trunc(c * np.float32(32767.0)).astype("<i2")


def _region(y, word):
    """The bytes of a request's region: the form of `word` applied to its stream y at the word's rate."""
    from kokorox_amd import voices as V
    form, hz = word & 0xFF, RATES[word & 0xF00][0]
    if form == 0:
        return y.astype("<f4").tobytes()
    if form == 1:
        return np.stack([y, y], axis=1).astype("<f4").tobytes()
    if form == 2:
        return _pcm16_form2(y).tobytes()
    if form == 3:
        return V.wav_f32_body(y, hz)
    if form == 4:
        return V.wav16_base64(y, hz)
    return (V.mulaw_bytes if form == 8 else V.alaw_bytes)(V.pcm16(y)).tobytes()


@pytest.fixture(scope="module")
def slab():
    return _slab()


@pytest.fixture(scope="module")
def resampled(slab):
    """The mirror's streams, computed once: {(grouping, rate word): [y of request r]}."""
    from kokorox_amd import voices as V
    return {(g, rate): [V.resample_stream(x, rate) for x in _streams(slab, cpr)] for g, cpr in GROUPINGS.items() for rate in RATES}


def _first_difference(got, want):
    n = min(len(got), len(want))
    i = next((j for j in range(n) if got[j] != want[j]), n)
    return f"lengths {len(got)} / {len(want)}, first difference at byte {i}: {got[max(0, i - 8): i + 8]!r} vs {want[max(0, i - 8): i + 8]!r}"


@pytest.mark.parametrize("grouping", sorted(GROUPINGS))
def test_hook_every_rate_and_form_equals_the_mirror(slab, resampled, grouping):
    from kokorox_amd import hip_koko as hk
    cpr = GROUPINGS[grouping]
    R = len(cpr)
    for rate, (hz, L, M) in RATES.items():
        ys = resampled[(grouping, rate)]
        for r, y in enumerate(ys):
            assert y.shape[0] == 600 * sum(FRAMES[sum(cpr[:r]): sum(cpr[: r + 1])]) * L // M
        if rate == 0:
            continue  # (24 kHz alone is tests/test_gpu_wire_formats.py; below it rides in the mixed batch)
        for form in FORMS:
            got = hk.pack_requests(slab, FRAMES, cpr, [form | rate] * R)
            assert len(got) == R
            for r in range(R):
                want = _region(ys[r], form | rate)
                assert got[r] == want, f"{hz} Hz form {form} request {r}: " + _first_difference(got[r], want)
    # one batch that mixes rates and forms, rate code 0 among them
    words = [[0x104, 0x000, 0x308, 0x203, 0x002, 0x109], [0x304, 0x004, 0x208], [0x309]][[6, 3, 1].index(R)]
    for shift in range(R):
        ws = words[shift:] + words[:shift]
        got = hk.pack_requests(slab, FRAMES, cpr, ws)
        for r in range(R):
            want = _region(resampled[(grouping, ws[r] & 0xF00)][r], ws[r])
            assert got[r] == want, f"mixed batch {ws}, request {r}: " + _first_difference(got[r], want)


def test_hook_base64_paddings_and_headers_at_8_khz(slab, resampled):
    """1, 2 and 3 frames at 8 kHz end in no, two and one `=`; the headers carry the rate and the true sizes."""
    import base64
    import struct
    from kokorox_amd import hip_koko as hk
    got = hk.pack_requests(slab, FRAMES, [1] * 6, [0x104] * 6)
    for r, pad in ((0, 0), (1, 2), (2, 1)):
        assert len(got[r]) - len(got[r].rstrip(b"=")) == pad
        raw = base64.b64decode(got[r], validate=True)
        n = 200 * FRAMES[r]
        assert struct.unpack("<I", raw[4:8])[0] == 36 + 2 * n and struct.unpack("<IIHH", raw[24:36]) == (8000, 16000, 2, 16)
        assert struct.unpack("<I", raw[40:44])[0] == 2 * n and len(raw) == 44 + 2 * n
    body = hk.pack_requests(slab, FRAMES, [6], [0x303])[0]
    assert struct.unpack("<IIHH", body[24:36]) == (48000, 192000, 4, 32) and len(body) == 44 + 4 * 15600


def test_hook_a_nan_inside_a_stream_spreads_exactly_as_in_the_mirror(slab):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    a = slab.copy()
    a[0, 595] = np.nan  # five samples before the chunk boundary inside request 0 of [2, 1, 3]: it spreads across the boundary
    cpr = GROUPINGS["two_one_three"]
    streams = _streams(a, cpr)
    for rate, (hz, L, M) in RATES.items():
        if rate == 0:
            continue
        ys = [V.resample_stream(x, rate) for x in streams]
        assert not np.isnan(ys[1]).any() and not np.isnan(ys[2]).any() and 0 < np.isnan(ys[0]).sum() < ys[0].shape[0]
        assert np.isnan(ys[0][601 * L // M + 1])  # (an output that belongs to the second chunk's time)
        got = hk.pack_requests(a, FRAMES, cpr, [0 | rate] * 3)
        for r in range(3):
            g = np.frombuffer(got[r], dtype="<f4")
            nan = np.isnan(ys[r])
            np.testing.assert_array_equal(np.isnan(g), nan)
            np.testing.assert_array_equal(g[~nan], ys[r][~nan])
        # the 16-bit forms keep their own NaN rules on the resampled stream: form 2 -> -32767, form 4 and G.711 -> 0
        for form in (2, 4, 8, 9):
            got = hk.pack_requests(a, FRAMES, cpr, [form | rate] * 3)
            for r in range(3):
                assert got[r] == _region(ys[r], form | rate), (hz, form, r)


# ---- model -----------------------------------------------------------------------------------------------------------
def _chunks():
    from oracle import kokoro_ref as R
    return [list(int(v) for v in R.synthetic_inputs(1, k, seed=500 + k)[0]) for k in (1, 10, 3, 5, 2, 7)]  # 3..12 tokens with the pads


def _decoded(y, word):
    """What infer_requests / submit_request hand out for `word`, from the stream y at the word's rate."""
    form = word & 0xFF
    raw = _region(y, word)
    if form in (3, 4):
        return raw
    dt = {0: np.float32, 1: np.float32, 2: np.int16, 8: np.uint8, 9: np.uint8}[form]
    a = np.frombuffer(raw, dtype=dt)
    return a.reshape(-1, 2) if form == 1 else a


def _same(got, want):
    if isinstance(want, bytes):
        assert isinstance(got, bytes) and got == want
    else:
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)


def test_model_requests_at_every_rate_equal_the_mirror_of_the_24_khz_result(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    names = ["af_sky", "af_nicole", "am_adam", "bf_emma"]
    styles = {n: tab[i] for i, n in enumerate(names)}
    hip_model.set_voice_table(tab)
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations(None)
    toks = _chunks()
    cpr = [1, 2, 3]
    rows = [V.mix_styles(styles, names[b % 4], len(t) - 2)[0] for b, t in enumerate(toks)]
    base, ns0 = hip_model.infer_requests(toks, cpr, styles=rows, speeds=[1.0], seed=21, fmt=0, with_samples=True)
    assert ns0 == [x.shape[0] for x in base] and all(n % 600 == 0 and n > 0 for n in ns0)
    for rate, (hz, L, M) in RATES.items():
        if rate == 0:
            continue
        ys = [V.resample_stream(x, rate) for x in base]
        for fmt in (hk.PACK_PCM16_MONO | rate, hk.PACK_MULAW | rate, [hk.PACK_WAV16_BASE64 | rate, 0, hk.PACK_ALAW | rate]):
            got, ns = hip_model.infer_requests(toks, cpr, styles=rows, speeds=[1.0], seed=21, fmt=fmt, with_samples=True)
            for r in range(3):
                word = fmt[r] if isinstance(fmt, list) else fmt
                if word & 0xF00:
                    assert ns[r] == ns0[r] * L // M == ys[r].shape[0]
                    _same(got[r], _decoded(ys[r], word))
                else:  # a 24 kHz request beside resampled ones: what it has always been
                    assert ns[r] == ns0[r]
                    _same(got[r], base[r])


def test_model_refuses_unknown_words(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    toks = _chunks()[:3]
    rows = [W.synthetic_voices(1)[0, len(t) - 2, 0] for t in toks]
    for fmt, message in ((0x105, "infer: unknown output format"), (0x400, "infer: unknown output sample rate"),
                         ([0, 0xF08], "infer: unknown output sample rate"), (0x1000, "infer: unknown output format"),
                         (0x106, "infer: unknown output format"), (0x207, "infer: unknown output format")):
        with pytest.raises(hk.KokoroxHipError) as e:
            hip_model.infer_requests(toks, [1, 2], styles=rows, fmt=fmt)
        assert e.value.code == hk.KX_ERR_INVALID and message in str(e.value), (fmt, str(e.value))
    for fmt in (0x100, 0x102, 8, 9):  # the old entries keep their three forms
        with pytest.raises(hk.KokoroxHipError) as e:
            hip_model.infer_packed(toks, rows, fmt=fmt)
        assert e.value.code == hk.KX_ERR_INVALID and "unknown output format" in str(e.value)


# ---- dispatcher ------------------------------------------------------------------------------------------------------
WORDS = [0x108, 0x000, 0x204, 0x302, 0x109, 0x004, 0x303, 0x200, 0x002, 0x308, 0x101, 0x209]


def _request_specs():
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    tab = W.synthetic_voices(4)
    specs = []
    for i, word in enumerate(WORDS):
        n = 1 + i % 3
        chunks = [list(int(v) for v in R.synthetic_inputs(1, 1 + (5 * i + 3 * c) % 10, seed=800 + 10 * i + c)[0]) for c in range(n)]
        if i % 2 == 0:
            voice = dict(styles=[tab[i % 4, len(c) - 2, 0] for c in chunks])
        else:
            voice = dict(voices=i % 4)
        specs.append(dict(chunks=chunks, voice=voice, fmt=word, seed=9100 + i))
    return tab, specs


def _alone(model, s):
    n = len(s["chunks"])
    v = s["voice"]
    kw = dict(styles=v["styles"]) if "styles" in v else dict(voice_ids=[[v["voices"]]] * n, weights=[[0.0]] * n)
    return model.infer_requests(s["chunks"], [n], speeds=[1.0], seed=s["seed"], fmt=s["fmt"], **kw)[0]


def test_dispatcher_mixed_rates_and_forms_equal_their_solo_runs(hip_model):
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
            for i in range(t, len(specs), 6):
                out[i] = d.submit_request(specs[i]["chunks"], seed=specs[i]["seed"], fmt=specs[i]["fmt"], **specs[i]["voice"])
        except Exception as e:  # pragma: no cover
            errs.append(e)

    try:
        th = [threading.Thread(target=client, args=(t,)) for t in range(6)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        st = d.stats()
        for fmt, message in ((0x105, "format"), (0x400, "unknown output sample rate"), (0x1004, "format"), (0x107, "format")):
            with pytest.raises(hk.KokoroxHipError) as e:
                d.submit_request(specs[0]["chunks"], fmt=fmt, **specs[0]["voice"])
            assert e.value.code == hk.KX_ERR_INVALID and message in str(e.value), (fmt, str(e.value))
        for fmt in (0x100, 0x102, 8):  # a rate code or a G.711 form on the single-utterance submit
            with pytest.raises(hk.KokoroxHipError) as e:
                d.submit_ex(specs[0]["chunks"][0], style=specs[0]["voice"]["styles"][0], fmt=fmt)
            assert e.value.code == hk.KX_ERR_INVALID
    finally:
        d.close()
    assert not errs, errs
    assert st["requests"] == len(specs)
    for i, s in enumerate(specs):
        _same(out[i], _alone(hip_model, s))
    # a single-row request with a rate code or a G.711 form went through the request packer: its sample count says so
    ns = hip_model.infer_requests(specs[0]["chunks"], [1], styles=specs[0]["voice"]["styles"], seed=specs[0]["seed"], fmt=0,
                                  with_samples=True)[1][0]
    assert specs[0]["fmt"] == 0x108 and out[0].dtype == np.uint8 and out[0].shape[0] * 3 == ns
