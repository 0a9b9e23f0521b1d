"""GPU: prosody (include/kokorox_hip.h, "prosody") -- the duration kernel with a per-token rate and fixed frame counts and the curve
and report kernel through their hooks against the numpy definitions of kokorox_amd/voices.py, the model's taps, durations, marks and
report, the downstream of the shaped curves against the oracle, the dispatcher, and the refusals.  Every comparison is an equality of
bytes unless it says otherwise.
"""
import threading

import numpy as np
import pytest

from kokorox_amd import voices as V

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the durations hook ----------------------------------------------------------------------------------------------------------
LENS = np.array([1, 7, 130], np.int32)  # one token; a few; two waves and a ragged tail
SPEEDS = np.array([0.8, 1.0, 1.3], np.float32)
T = 130
MARGIN = 0.01


def _half_distance(v):
    """|v - the nearest half-integer|, in float64"""
    return np.abs(v - (np.floor(v) + 0.5))


def _make_dur_case():
    """Logits [3,50,130], a rate per token, and the value of every token before rounding in float64 -- with and without the rate --
    and at the slowest rate -- at least 0.01 away from a half-integer, so that expf's last bit decides no case.  Columns are redrawn
    (seeded) until they are twice that far; the tests assert the 0.01 again on what they use."""
    rng = np.random.default_rng(77)
    logits = np.zeros((3, 50, T), np.float32)
    rate = rng.choice(np.array([0.25, 0.5, 0.8, 1.0, 1.0, 1.25, 2.0, 4.0], np.float32), size=(3, T))
    s64 = np.zeros((3, T))
    for b in range(3):
        for t in range(T):
            for _ in range(1000):
                col = (rng.standard_normal(50) * 1.5 - 1.8).astype(np.float32)
                s = (1.0 / (1.0 + np.exp(-col.astype(np.float64)))).sum()
                vals = s / np.float64(SPEEDS[b]) / np.array([1.0, np.float64(rate[b, t]), 0.25])
                if (_half_distance(vals) >= 2 * MARGIN).all():
                    break
            logits[b, :, t] = col
            s64[b, t] = s
    src = rng.standard_normal((3, 2, T)).astype(np.float32)
    return dict(logits=logits, rate=rate, s64=s64, src=src)


@pytest.fixture(scope="module")
def dur_case():
    return _make_dur_case()


def _expected(case, rate=None, frames=None, pinned=None, idx_ld=None):
    """Per row: the used durations by voices.prosody_durations from the float32 s / speed, after the margin has been asserted."""
    out = []
    for b in range(3):
        n = int(LENS[b])
        v = case["s64"][b, :n] / np.float64(SPEEDS[b])
        assert (_half_distance(v) >= MARGIN).all()
        if rate is not None:
            v = v / rate[b, :n].astype(np.float64)
            assert (_half_distance(v) >= MARGIN).all()
        s32 = (case["s64"][b, :n].astype(np.float32) / SPEEDS[b]).astype(np.float32)
        out.append(V.prosody_durations(s32, None if rate is None else rate[b, :n], None if frames is None else frames[b, :n], pinned,
                                       idx_ld=50 * T if idx_ld is None else idx_ld))
    return out


def _check_alignment(got, want, idx_ld, over_want=0):
    from kokorox_amd import hip_koko as hk
    dur, frames, idx, g, over = got
    assert over == over_want
    for b in range(3):
        n, d = int(LENS[b]), want[b]
        np.testing.assert_array_equal(dur[b, :n], d)
        assert (dur[b, n:] == hk.INT_SENTINEL).all()
        F = int(d.sum())
        assert frames[b] == F <= idx_ld
        np.testing.assert_array_equal(idx[b, :F], np.repeat(np.arange(n), d))
        assert (idx[b, F:] == hk.INT_SENTINEL).all()


def _frames_case(rng):
    frames = rng.integers(0, 4, size=(3, T)).astype(np.int32) * rng.integers(0, 2, size=(3, T)).astype(np.int32)
    frames[2, 5], frames[2, 64], frames[2, 129], frames[0, 0] = 50, 1, 50, 0
    return frames


def test_durations_hook_rate_frames_both_and_pinned(dur_case):
    from kokorox_amd import hip_koko as hk
    c = dur_case
    frames = _frames_case(np.random.default_rng(5))
    for kw in (dict(rate=c["rate"]), dict(frames=frames), dict(rate=c["rate"], frames=frames),
               dict(frames=frames, pinned=[3, 9, 2]), dict(rate=c["rate"], pinned=[4])):
        got = hk.prosody_durations(c["logits"], LENS, SPEEDS, c["src"], **kw)
        want = _expected(c, kw.get("rate"), kw.get("frames"), kw.get("pinned"))
        _check_alignment(got, want, 50 * T)
        if "frames" in kw:  # (every override took, whatever stood there before)
            for b in range(3):
                m = frames[b, : LENS[b]] >= 1
                np.testing.assert_array_equal(got[0][b, : LENS[b]][m], frames[b, : LENS[b]][m])
    # the gather behind it reads the new alignment
    dur, fr, idx, g, _ = hk.prosody_durations(c["logits"], LENS, SPEEDS, c["src"], rate=c["rate"])
    for b in range(3):
        np.testing.assert_array_equal(g[b, :, : fr[b]], c["src"][b][:, idx[b, : fr[b]]])
        assert (g[b, :, fr[b]:] == hk.LN_SENTINEL).all()


def test_durations_hook_a_row_that_overflows_is_cut_as_today(dur_case):
    from kokorox_amd import hip_koko as hk
    c = dur_case
    slow = np.ones((3, T), np.float32)
    slow[2] = 0.25
    uncut = int(V.prosody_durations((c["s64"][2].astype(np.float32) / SPEEDS[2]).astype(np.float32), slow[2], idx_ld=10 ** 9).sum())
    idx_ld = uncut - 37  # (row 2 crosses the end inside its last tokens; rows 0 and 1 fit)
    want = _expected(c, slow, idx_ld=idx_ld)
    assert int(want[2].sum()) == idx_ld and (want[2] >= 0).all() and int(want[0].sum()) < idx_ld and int(want[1].sum()) < idx_ld
    got = hk.prosody_durations(c["logits"], LENS, SPEEDS, c["src"], rate=slow, idx_ld=idx_ld, Fcap=idx_ld)
    _check_alignment(got, want, idx_ld, over_want=3)
    # ... and exactly as the plain kernel cuts the same row at the same speed
    plain = hk.alignment(c["logits"], LENS, SPEEDS * np.array([1, 1, 0.25], np.float32), c["src"], idx_ld=idx_ld, Fcap=idx_ld)
    np.testing.assert_array_equal(got[0][2], plain[0][2])
    assert plain[4] == 3


def test_durations_hook_neutral_arrays_equal_the_alignment_hook(dur_case):
    from kokorox_amd import hip_koko as hk
    c = dur_case
    plain = hk.alignment(c["logits"], LENS, SPEEDS, c["src"], pinned=[2, 5])
    for kw in (dict(rate=np.ones((3, T), np.float32)), dict(frames=np.zeros((3, T), np.int32)),
               dict(rate=np.ones((3, T), np.float32), frames=np.zeros((3, T), np.int32))):
        got = hk.prosody_durations(c["logits"], LENS, SPEEDS, c["src"], pinned=[2, 5], **kw)
        for a, b in zip(got[:4], plain[:4]):
            assert a.tobytes() == b.tobytes()
        assert got[4] == plain[4] == 0
    plain = hk.alignment(c["logits"], LENS, SPEEDS, c["src"])
    got = hk.prosody_durations(c["logits"], LENS, SPEEDS, c["src"], rate=np.ones((3, T), np.float32))
    for a, b in zip(got[:4], plain[:4]):
        assert a.tobytes() == b.tobytes()
    _check_alignment(plain, _expected(c), 50 * T)


# ---- 2. the curves hook -------------------------------------------------------------------------------------------------------------
CURVE_DUR = [[1], [1, 1, 1, 2], [2, 1, 1, 1, 4, 0, 7, 1, 1, 3, 16]]  # frames 1, 5, 37; runs of one-frame tokens: a window over three tokens
POISON_PAST = np.float32(777.25)


def _make_curve_case():
    rng = np.random.default_rng(31)
    frames = np.array([sum(d) for d in CURVE_DUR], np.int32)
    lens = np.array([len(d) for d in CURVE_DUR], np.int32)
    Tc, Fcap = int(lens.max()), int(frames.max())
    dur = np.zeros((3, Tc), np.int32)
    idx = np.zeros((3, Fcap), np.int32)
    curves = np.full((3, 2, 2 * Fcap), POISON_PAST, np.float32)
    pitch = rng.choice(np.array([0.25, 0.5, 0.9, 1.0, 1.1, 2.0, 4.0], np.float32), size=(3, Tc))
    energy = rng.choice(np.array([0.0, 0.3, 1.0, 1.7, 4.0], np.float32), size=(3, Tc))
    for b, d in enumerate(CURVE_DUR):
        dur[b, : len(d)] = d
        idx[b, : frames[b]] = np.repeat(np.arange(len(d)), d)
        n = 2 * frames[b]
        curves[b, 0, :n] = rng.uniform(-20, 300, size=n).astype(np.float32)
        curves[b, 1, :n] = rng.standard_normal(n).astype(np.float32)
    # row 2: values on both sides of 10, exactly 10, a NaN, and voiced values whose product falls to 10 or below (tokens 0 and 4 at 0.25)
    pitch[2, 0], pitch[2, 1], pitch[2, 4] = 0.25, 0.25, 0.25
    curves[2, 0, :12] = [9.5, 10.5, 10.0, np.nan, 12.0, 39.0, 10.000001, 250.0, 40.5, 11.0, 9.999999, 30.0]
    curves[2, 1, 20] = np.nan
    curves[1, 0, :4] = [10.0, 10.000001, 5.0, 200.0]
    return dict(frames=frames, lens=lens, dur=dur, idx=idx, curves=curves, pitch=pitch, energy=energy)


@pytest.fixture(scope="module")
def curve_case():
    return _make_curve_case()


def _check_curves(c, shaped, rep, pitch, energy):
    at = 0
    for b, d in enumerate(CURVE_DUR):
        n = 2 * int(c["frames"][b])
        f0s, ns = V.shape_curves(c["curves"][b, 0, :n], c["curves"][b, 1, :n], d, None if pitch is None else pitch[b, : len(d)],
                                 None if energy is None else energy[b, : len(d)])
        assert (bits(shaped[b, 0, :n]) == bits(f0s)).all(), b
        nan_n = np.isnan(ns)
        assert (bits(shaped[b, 1, :n])[~nan_n] == bits(ns)[~nan_n]).all() and np.isnan(shaped[b, 1, :n][nan_n]).all(), b
        assert ((shaped[b, 0, :n] > 10) == (c["curves"][b, 0, :n] > 10)).all()  # the voiced / unvoiced decision never flips
        assert (shaped[b, :, n:] == POISON_PAST).all()  # nothing at or past 2 F_b is written
        if rep is not None:
            want = V.prosody_report(f0s, ns, d)
            got = rep[at: at + len(d)]
            nan_r = np.isnan(want)
            assert (bits(got)[~nan_r] == bits(want)[~nan_r]).all() and np.isnan(got[nan_r]).all(), (b, got, want)
        at += len(d)


def test_curves_hook_against_the_numpy_definition(curve_case):
    from kokorox_amd import hip_koko as hk
    c = curve_case
    # the fixture has what the issue lists: some voiced value really falls to the floor, some step's window spans three tokens
    f0s, _ = V.shape_curves(c["curves"][2, 0, :74], c["curves"][2, 1, :74], CURVE_DUR[2], c["pitch"][2], None)
    assert (bits(f0s) == np.uint32(0x41200001)).sum() >= 2
    for pitch, energy, report in ((c["pitch"], c["energy"], True), (c["pitch"], None, True), (None, c["energy"], True),
                                  (c["pitch"], c["energy"], False), (None, None, True)):
        shaped, rep = hk.prosody_curves(c["curves"], c["frames"], c["lens"], c["idx"], c["dur"], pitch, energy, report=report)
        assert (rep is None) == (not report)
        _check_curves(c, shaped, rep, pitch, energy)
        if pitch is None:
            assert shaped[:, 0].tobytes() == c["curves"][:, 0].tobytes()
        if energy is None:
            assert shaped[:, 1].tobytes() == c["curves"][:, 1].tobytes()
    # neutral ratios: the curves keep their bits, NaN payloads included
    one = np.ones_like(c["pitch"])
    shaped, rep = hk.prosody_curves(c["curves"], c["frames"], c["lens"], c["idx"], c["dur"], one, None, report=True)
    assert shaped.tobytes() == c["curves"].tobytes()
    # a token without frames reports four zeros; the report's frames are the durations
    assert rep[5 + 5].tolist() == [0, 0, 0, 0]
    np.testing.assert_array_equal(rep[:, 3], np.concatenate(CURVE_DUR))


# ---- 3. the model -------------------------------------------------------------------------------------------------------------------
COUNTS = [9, 14, 6]
CPR = [2, 1]


def _model_inputs(seed0=40):
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    toks = [list(R.synthetic_inputs(1, n - 2, seed=seed0 + i)[0]) for i, n in enumerate(COUNTS)]
    voices = W.synthetic_voices(4)
    styles = [voices[i % 4, n - 2, 0] for i, n in enumerate(COUNTS)]
    assert [len(t) for t in toks] == COUNTS
    return toks, styles


def _prosody(rng, counts, with_frames=True):
    rate = [rng.choice([0.5, 1.0, 2.0], size=n).astype(np.float32) for n in counts]
    frames = [rng.integers(1, 7, size=n).astype(np.int32) for n in counts] if with_frames else None
    pitch = [rng.choice([0.7, 1.0, 1.0, 1.3, 2.0], size=n).astype(np.float32) for n in counts]
    energy = [rng.choice([0.0, 0.5, 1.0, 1.5], size=n).astype(np.float32) for n in counts]
    return rate, frames, pitch, energy


def test_model_taps_durations_marks_and_report(hip_model):
    from kokorox_amd import hip_koko as hk
    toks, styles = _model_inputs()
    rate, frames, pitch, energy = _prosody(np.random.default_rng(8), COUNTS)
    hip_model.set_utterance_base(0)
    kw = dict(styles=styles, speeds=[1.1], seed=5)
    JOIN = (7, 20, 50, 2)  # trim head, tail and inner to 20 ms, 50 ms pauses, 2 ms fades
    for word in (0, 0x102):  # f32 at 24 000 Hz, PCM16 at 8000 Hz
        bodies, marks, rep, samples = hip_model.infer_requests_prosody(toks, CPR, (rate, frames, pitch, energy), fmt=word, marks=True,
                                                                       with_samples=True, flags=hk.KX_FLAG_TAPS, **kw)
        # the taps behind the kernel are the numpy shaping of the taps in front of it
        for b, n in enumerate(COUNTS):
            raw0, raw1 = hip_model.tap("pred.F0.raw", b), hip_model.tap("pred.N.raw", b)
            assert raw0.shape == (1, 2 * int(frames[b].sum()))
            f0s, ns = V.shape_curves(raw0[0], raw1[0], frames[b], pitch[b], energy[b])
            assert (bits(hip_model.tap("pred.F0", b)[0]) == bits(f0s)).all() and (bits(hip_model.tap("pred.N", b)[0]) == bits(ns)).all()
            assert (raw0[0] > 10).any() and not (bits(f0s) == bits(raw0[0])).all()  # (something was voiced and something moved)
        per_req = [[frames[0], frames[1]], [frames[2]]]
        for r in range(2):
            np.testing.assert_array_equal(marks[r], V.token_marks(per_req[r], word))
            assert samples[r] == int(marks[r][-1]) == V._RATE_LM[word >> 8][0] * 600 * int(sum(d.sum() for d in per_req[r])) // V._RATE_LM[word >> 8][1]
            np.testing.assert_array_equal(rep[r][:, 3], np.concatenate(per_req[r]))
            # the report is the numpy report of the shaped taps
            rows = range(2) if r == 0 else range(2, 3)
            want = np.concatenate([V.prosody_report(hip_model.tap("pred.F0", b)[0], hip_model.tap("pred.N", b)[0], frames[b]) for b in rows])
            assert (bits(rep[r]) == bits(want)).all()
        # ... and under a join the marks are the joined marks of the same numbers
        _, jmarks, jrep, jsamples = hip_model.infer_requests_prosody(toks, CPR, (rate, frames, pitch, energy), joins=JOIN, fmt=word, marks=True,
                                                                     with_samples=True, **kw)
        for r in range(2):
            np.testing.assert_array_equal(jmarks[r], V.joined_marks(per_req[r], word, JOIN))
            assert jsamples[r] == int(jmarks[r][-1])
            assert (bits(jrep[r]) == bits(rep[r])).all()
    # the used durations of kx_infer_prosody are the frames asked for, and the waveforms have their length
    waves, durs = hip_model.infer_prosody(toks, styles, [1.1], (rate, frames, pitch, energy), seed=5)
    for b in range(3):
        np.testing.assert_array_equal(durs[b], frames[b])
        assert waves[b].shape[0] == 600 * int(frames[b].sum())
    # with a rate alone the durations move the way the rate says (slower is never shorter), and the report's frames follow
    base_w, base_d = hip_model.infer_prosody(toks, styles, [1.1], None, seed=5)
    slow_w, slow_d = hip_model.infer_prosody(toks, styles, [1.1], ([np.full(n, 0.5, np.float32) for n in COUNTS], None, None, None), seed=5)
    for b in range(3):
        assert (slow_d[b] >= base_d[b]).all() and slow_d[b].sum() > base_d[b].sum() and slow_w[b].shape[0] == 600 * int(slow_d[b].sum())


def test_model_neutral_prosody_is_the_call_without_it(hip_model):
    toks, styles = _model_inputs(seed0=60)
    hip_model.set_utterance_base(0)
    kw = dict(styles=styles, speeds=[0.9, 1.0, 1.2], seed=9, fmt=[0x003, 0x202])
    JOIN = (7, 20, 50, 2)
    want_b, want_m = hip_model.infer_requests_joined(toks, CPR, JOIN, marks=True, **kw)
    neutral = ([np.ones(n, np.float32) for n in COUNTS], [np.zeros(n, np.int32) for n in COUNTS], [np.ones(n, np.float32) for n in COUNTS],
               [np.ones(n, np.float32) for n in COUNTS])
    for prosody in (None, neutral, (None, None, neutral[2], None)):
        for report in (False, True):
            got = hip_model.infer_requests_prosody(toks, CPR, prosody, joins=JOIN, marks=True, report=report, **kw)
            for r in range(2):
                assert bytes(got[0][r]) == bytes(want_b[r])
                np.testing.assert_array_equal(got[1][r], want_m[r])
    plain = hip_model.infer_batch(toks, styles, [0.9, 1.0, 1.2], seed=9)
    waves, _ = hip_model.infer_prosody(toks, styles, [0.9, 1.0, 1.2], neutral, seed=9)
    for a, b in zip(plain, waves):
        assert a.tobytes() == b.tobytes()


# ---- 4. downstream of the shaped curves, against the oracle -------------------------------------------------------------------------
def test_both_readers_of_the_curves_take_the_shaped_values(hip_model, oracle):
    """The parity protocol of tests/test_gpu_forward.py with its two edges pinned (the GPU's curves into the oracle's source, the
    GPU's STFT into everything downstream) and that file's tolerance: the harmonic source and F0_conv / N_conv read the SHAPED
    curves, or source and waveform would be those of the raw ones."""
    from test_gpu_forward import TOL_WAVE, _wrapped_diff
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    n = 12
    ids = R.synthetic_inputs(1, n - 2, seed=90)[0]
    style = W.synthetic_voices(4)[1, n - 2, 0]
    rng = np.random.default_rng(12)
    frames = rng.integers(2, 6, size=n).astype(np.int32)
    pitch = rng.choice([0.6, 1.0, 1.5, 2.0], size=n).astype(np.float32)
    energy = rng.choice([0.3, 1.0, 1.8], size=n).astype(np.float32)
    hip_model.set_utterance_base(0)
    (wave,), (dur,) = hip_model.infer_prosody([list(ids)], [style], [1.0], (None, [frames], [pitch], [energy]), seed=2, flags=hk.KX_FLAG_TAPS)
    np.testing.assert_array_equal(dur, frames)
    f0, n_c = hip_model.tap("pred.F0", 0), hip_model.tap("pred.N", 0)[0]
    raw = hip_model.tap("pred.F0.raw", 0)
    assert np.abs(f0 - raw).max() > 1.0 and np.abs(n_c - hip_model.tap("pred.N.raw", 0)[0]).max() > 1e-3  # (the shaping is no rounding matter)
    taps2 = {}
    oracle.forward(ids, style, 1.0, seed=2, utt=0, taps=taps2, pinned_dur=frames, f0_override=f0[0], n_override=n_c)
    assert np.abs(hip_model.tap("gen.har_source", 0) - taps2["gen.har_source"].numpy()).max() < 2e-6
    har = hip_model.tap("gen.har", 0)
    assert _wrapped_diff(har, taps2["gen.har"].numpy()).max() < 2e-3
    audio3, _ = oracle.forward(ids, style, 1.0, seed=2, utt=0, pinned_dur=frames, f0_override=f0[0], n_override=n_c, har_override=har)
    err = float(np.abs(wave - audio3.numpy()).max())
    print(f"conv mode {hip_model.get_conv_mode()}: shaped curves, waveform max|d| {err:.2e}")
    assert err < TOL_WAVE
    # the raw curves give another waveform altogether: the tolerance tells the two apart
    audio_raw, _ = oracle.forward(ids, style, 1.0, seed=2, utt=0, pinned_dur=frames, f0_override=raw[0],
                                  n_override=hip_model.tap("pred.N.raw", 0)[0], har_override=har)
    assert float(np.abs(wave - audio_raw.numpy()).max()) > 10 * TOL_WAVE


# ---- 5. the dispatcher --------------------------------------------------------------------------------------------------------------
def test_dispatcher_prosody_and_plain_requests_share_batches(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    voices = W.synthetic_voices(4)
    rng = np.random.default_rng(3)
    reqs = []
    for i in range(8):
        counts = [7 + i, 5] if i % 3 == 0 else [6 + 2 * i]
        chunks = [list(R.synthetic_inputs(1, n - 2, seed=300 + 10 * i + c)[0]) for c, n in enumerate(counts)]
        rows = [voices[(i + c) % 4, n - 2, 0] for c, n in enumerate(counts)]
        prosody = _prosody(rng, counts, with_frames=i % 4 == 1) if i % 2 == 1 else None
        reqs.append(dict(chunks=chunks, rows=rows, speed=1.0 + 0.1 * (i % 3), seed=500 + i, fmt=(0, 0x102, 3)[i % 3], prosody=prosody,
                         marks=i in (1, 2), join=(7, 20, 30, 1) if i in (3, 4) else None))
    d = hk.Dispatcher([hip_model], max_batch=16, max_wait_us=200000)
    out, errs = [None] * 8, []

    def client(i):
        q = reqs[i]
        try:
            out[i] = d.submit_request(q["chunks"], styles=q["rows"], speed=q["speed"], seed=q["seed"], fmt=q["fmt"], marks=q["marks"],
                                      join=q["join"], prosody=q["prosody"], report=q["prosody"] is not None)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=client, args=(i,)) for i in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    st = d.stats()
    d.close()
    assert not errs, errs
    assert st["requests"] == 8 and st["batches"] < 8 and st["max_batch"] > 1
    hip_model.set_utterance_base(0)
    for i, q in enumerate(reqs):
        kw = dict(styles=q["rows"], speeds=[q["speed"]], seed=q["seed"], fmt=q["fmt"])
        got = out[i] if isinstance(out[i], tuple) else (out[i],)
        if q["prosody"] is not None:
            alone = hip_model.infer_requests_prosody(q["chunks"], [len(q["chunks"])], q["prosody"], joins=q["join"], marks=q["marks"], **kw)
            assert (bits(got[-1]) == bits(alone[-1][0])).all() and got[-1].shape == (sum(len(c) for c in q["chunks"]), 4)
        elif q["join"] is not None:
            alone = (hip_model.infer_requests_joined(q["chunks"], [len(q["chunks"])], q["join"], **kw),)
        elif q["marks"]:
            alone = hip_model.infer_requests_marks(q["chunks"], [len(q["chunks"])], **kw)
        else:
            alone = (hip_model.infer_requests(q["chunks"], [len(q["chunks"])], **kw),)
        assert bytes(got[0]) == bytes(alone[0][0]), i
        if q["marks"]:
            np.testing.assert_array_equal(got[1], alone[1][0])


# ---- 6. the refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(hip_model):
    import ctypes as C
    from kokorox_amd import hip_koko as hk
    toks, styles = _model_inputs()
    kw = dict(styles=styles, speeds=[1.0], seed=1)
    nan = np.float32(np.nan)
    bad_values = [(0, np.float32(0.2499)), (0, np.float32(4.0001)), (0, nan), (0, np.float32(0.0)), (0, np.float32(-1.0)),
                  (1, np.int32(-1)), (1, np.int32(51)),
                  (2, np.float32(0.2499)), (2, np.float32(4.0001)), (2, nan), (2, np.float32(np.inf)),
                  (3, np.float32(-1e-6)), (3, np.float32(4.0001)), (3, nan)]
    for which, v in bad_values:
        arrs = [[np.ones(n, np.float32) for n in COUNTS], [np.zeros(n, np.int32) for n in COUNTS], [np.ones(n, np.float32) for n in COUNTS],
                [np.ones(n, np.float32) for n in COUNTS]]
        arrs[which][2][COUNTS[2] - 1] = v  # the last token of the last row
        given = tuple(a if k == which else None for k, a in enumerate(arrs))
        with pytest.raises(hk.KokoroxHipError) as e:
            hip_model.infer_requests_prosody(toks, CPR, given, **kw)
        assert e.value.code == hk.KX_ERR_INVALID and "infer: bad prosody" in str(e.value), (which, v)
        with pytest.raises(hk.KokoroxHipError) as e:
            hip_model.infer_prosody(toks, styles, [1.0], given)
        assert e.value.code == hk.KX_ERR_INVALID and "infer: bad prosody" in str(e.value), (which, v)
    # the edges themselves are fine
    edge = ([np.full(n, 0.25, np.float32) for n in COUNTS], [np.full(n, 50, np.int32) for n in COUNTS], [np.full(n, 4, np.float32) for n in COUNTS],
            [np.zeros(n, np.float32) for n in COUNTS])
    _, rep = hip_model.infer_requests_prosody(toks, CPR, edge, **kw)
    assert (rep[0][:, 3] == 50).all() and (rep[1][:, 2] == 0).all()
    # the null-pair rule of the report, on the raw entry
    ids, lens = hip_model._ids_lens(toks)
    st = np.ascontiguousarray(np.asarray(styles, np.float32).reshape(3, 256))
    cp, sp, fm = np.array(CPR, np.int32), np.array([1.0], np.float32), np.array([0], np.int32)
    p = hk._ptr
    for give_rep, give_n in ((True, False), (False, True)):
        out, nb, ns = C.c_void_p(), np.zeros(2, np.int64), np.zeros(2, np.int64)
        rp, n_rp = C.c_void_p(), np.zeros(2, np.int64)
        rc = hip_model._lib.kx_infer_requests_prosody(hip_model._h, p(ids), ids.shape[1], p(lens), 3, p(cp), 2, p(st), None, None, 0, p(sp), 1, 1, 0,
                                                      p(fm), 1, C.byref(out), p(nb), p(ns), None, None, None, 0, None,
                                                      C.byref(rp) if give_rep else None, p(n_rp) if give_n else None)
        assert rc == hk.KX_ERR_INVALID and "infer: null report argument" in hip_model.last_error() and not out.value
    # the dispatcher checks a request when it is submitted, with its own texts
    d = hk.Dispatcher([hip_model], max_batch=4, max_wait_us=0)
    try:
        for which, v in bad_values:
            arrs = [[np.ones(n, np.float32) for n in COUNTS[:2]], [np.zeros(n, np.int32) for n in COUNTS[:2]],
                    [np.ones(n, np.float32) for n in COUNTS[:2]], [np.ones(n, np.float32) for n in COUNTS[:2]]]
            arrs[which][1][COUNTS[1] - 1] = v
            given = tuple(a if k == which else None for k, a in enumerate(arrs))
            with pytest.raises(hk.KokoroxHipError) as e:
                d.submit_request(toks[:2], styles=styles[:2], prosody=given, report=True)
            assert e.value.code == hk.KX_ERR_INVALID and "dispatcher_submit_request: bad prosody" in str(e.value), (which, v)
        a = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64) for t in toks[:2]]))
        ln = np.array(COUNTS[:2], np.int32)
        rows = np.ascontiguousarray(np.asarray(styles[:2], np.float32).reshape(-1))
        for give_rep, give_n in ((True, False), (False, True)):
            out, nb, ns, rp, n_rp = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_void_p(), C.c_int64(0)
            err = C.create_string_buffer(256)
            rc = hip_model._lib.kx_dispatcher_submit_request_prosody(d._d, p(a), p(ln), 2, p(rows), None, None, 0, 1.0, 1, 0, C.byref(out),
                                                                     C.byref(nb), C.byref(ns), None, None, None, None,
                                                                     C.byref(rp) if give_rep else None, C.byref(n_rp) if give_n else None, err, len(err))
            assert rc == hk.KX_ERR_INVALID and err.value == b"dispatcher_submit_request: null report argument"
    finally:
        d.close()
