"""GPU: fit (include/kokorox_hip.h, "fit") -- the weights kernel and fit_spans_kernel through their hook against the numpy definition
voices.fit_durations fed with the weights the GPU returned (expf differs between libms, so the weights themselves are compared
with a bound, everything behind them with equalities), then the model: marks, samples, taps, the prosody report, requests without
spans beside fitted ones, the dispatcher, and the refusals.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from kokorox_amd import voices as V

pytestmark = pytest.mark.gpu

T = 130
LO = 0x00800000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the hook ------------------------------------------------------------------------------------------------------------------
# request 0: one row of one token; request 1: three rows of 7 with one span across all three; request 2: four rows of 130 with one
# span of 520 tokens (lanes own several tokens; the span crosses rows and waves); request 3: one row of 40 with two spans and an
# unfitted gap between them (and unfitted tokens in front)
LENS = np.array([1, 7, 7, 7, 130, 130, 130, 130, 40], np.int32)
CPR = np.array([1, 3, 4, 1], np.int32)
SPEEDS = np.array([0.8, 1.0, 1.3, 0.9, 1.0, 1.1, 0.7, 1.2, 1.0], np.float32)
SPANS = [(0, 0, 1), (1, 0, 21), (2, 0, 520), (3, 2, 10), (3, 15, 40)]  # (request, begin, end)
B = len(LENS)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(2026)
    logits = (rng.standard_normal((B, 50, T)) * 1.5 - 1.8).astype(np.float32)
    s64 = (1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).sum(axis=1)  # [B, T]
    rate = rng.choice(np.array([0.25, 0.5, 0.8, 1.0, 1.0, 1.25, 2.0, 4.0], np.float32), size=(B, T))
    src = rng.standard_normal((B, 2, T)).astype(np.float32)
    return dict(logits=logits, s64=s64, rate=rate, src=src)


def _flat(x):
    """[B, >= lens] -> the rows' valid entries back to back"""
    return np.concatenate([x[b, : LENS[b]] for b in range(B)])


def _span_positions(lens, cpr, spans):
    prefix = np.concatenate([[0], np.cumsum(lens)])
    first_row = np.concatenate([[0], np.cumsum(cpr)])
    return [(int(prefix[first_row[s[0]]]) + s[1], int(prefix[first_row[s[0]]]) + s[2]) for s in spans]


def _targets(fixed, how, rng):
    """A target per span of SPANS: n + held, 50 n + held, or something in between."""
    out = []
    held = np.zeros(int(LENS.sum()), np.int64) if fixed is None else _flat(fixed).astype(np.int64)
    for (b, e), s in zip(_span_positions(LENS, CPR, SPANS), SPANS):
        h = held[b:e]
        n, phi = int((h < 1).sum()), int(h[h >= 1].sum())
        G = {"n": n, "50n": 50 * n, "between": int(rng.integers(n + 1, 50 * n)) if n > 0 else 0}[how]
        if how == "between" and s[0] == 2:
            G = 7 * n + 3  # (what a sentence asks for, not half the ceiling)
        out.append((s[0], s[1], s[2], phi + G))
    return out


def _run_and_check(logits, src, spans, rate=None, fixed=None, lens=LENS, cpr=CPR, speeds=SPEEDS, compare_plain=True):
    """The hook on the case, every output against the numpy definition fed with the w it returned; returns (w, fitted, results)."""
    from kokorox_amd import hip_koko as hk
    nb = len(lens)
    dur, frames, idx, g, over, w, fitted, res = hk.fit_durations(logits, lens, speeds, src, spans, chunks_per_request=cpr, rate=rate, frames=fixed)
    assert over == 0
    prefix = np.concatenate([[0], np.cumsum(lens)])
    total = int(prefix[-1])
    flat = lambda x: np.concatenate([x[b, : lens[b]] for b in range(nb)])
    wf, got = flat(w), flat(fitted)
    held = np.zeros(total, np.int64) if fixed is None else flat(np.asarray(fixed)).astype(np.int64)
    held = np.where(held >= 1, held, 0)
    want = held.copy()  # a held token keeps the caller's count, a token outside every span gets 0
    in_span = np.zeros(total, bool)
    assert (wf >= np.float32(2.0 ** -20)).all() and (wf <= np.float32(2.0 ** 20)).all()
    for k, ((b, e), s) in enumerate(zip(_span_positions(lens, cpr, spans), spans)):
        d, lam, E = V.fit_durations(wf[b:e], s[3], held[b:e])
        want[b:e] = d
        in_span[b:e] = True
        assert int(d.sum()) == s[3]
        r = res[k]
        assert bits(r["lambda"]) == lam and r["n_free"] == int((held[b:e] < 1).sum()) and r["held_frames"] == int(held[b:e].sum()) \
            and r["excess"] == E, (k, r, lam, E)
    np.testing.assert_array_equal(got, want)
    for b in range(nb):  # (every entry of the two arrays is written: zeros at and past the row's tokens)
        assert (w[b, lens[b]:] == 0).all() and (fitted[b, lens[b]:] == 0).all()
    # the duration kernel took them: fitted and held tokens last what the array says, and the rows' frames and alignment follow
    used = flat(dur)
    assert (used[want >= 1] == want[want >= 1]).all()
    for b in range(nb):
        n = int(lens[b])
        assert (dur[b, n:] == hk.INT_SENTINEL).all() and frames[b] == int(dur[b, :n].sum())
        np.testing.assert_array_equal(idx[b, : frames[b]], np.repeat(np.arange(n), dur[b, :n]))
    # unfitted tokens: what kx_test_prosody_durations (the alignment hook when the call gives neither array) makes of the same inputs
    if compare_plain:
        if rate is None and fixed is None:
            plain = hk.alignment(logits, lens, speeds, src)[0]
        else:
            plain = hk.prosody_durations(logits, lens, speeds, src, rate=rate, frames=fixed)[0]
        assert (~in_span).any()
        np.testing.assert_array_equal(used[~in_span], flat(plain)[~in_span])
    return w, fitted, res


def test_weights_against_a_float64_sum_of_sigmoids(case):
    """50 float32 additions at half an ulp of at most 2^-18 (the sum is below 50 < 2^6), plus 50 terms at 4 ulp of 1, come to 1.1e-4
    before the two divisions: the bound is 2e-4 / (speed rate)."""
    rng = np.random.default_rng(1)
    for rate in (None, case["rate"]):
        w, _, _ = _run_and_check(case["logits"], case["src"], _targets(None, "between", rng), rate=rate)
        for b in range(B):
            n = int(LENS[b])
            div = np.float64(SPEEDS[b]) * (1.0 if rate is None else rate[b, :n].astype(np.float64))
            err = np.abs(w[b, :n].astype(np.float64) - case["s64"][b, :n] / div)
            assert (err <= 2e-4 / div).all(), (b, float((err * div).max()))


@pytest.mark.parametrize("how", ["n", "50n", "between"])
def test_span_shapes_and_targets(case, how):
    rng = np.random.default_rng(5)
    spans = _targets(None, how, rng)
    _, fitted, res = _run_and_check(case["logits"], case["src"], spans, rate=case["rate"])
    if how == "n":
        assert all(bits(r["lambda"]) == LO and r["excess"] == 0 for r in res)
        assert set(np.unique(fitted).tolist()) == {0, 1}
    if how == "50n":
        assert all(r["excess"] == 0 for r in res) and int(fitted.max()) == 50
    # ... and with held tokens inside the spans (one of them the only token in front of a row boundary), a rate and fixed counts outside
    fixed = (rng.integers(1, 51, size=(B, T)) * (rng.random((B, T)) < 0.2)).astype(np.int32)
    fixed[0, 0] = 0  # (the one-token span keeps its free token)
    fixed[1, 6], fixed[4, 129], fixed[5, 0] = 9, 50, 1
    _run_and_check(case["logits"], case["src"], _targets(fixed, how, rng), rate=case["rate"], fixed=fixed)


@pytest.mark.parametrize("with_held", [False, True])
def test_all_logits_equal_the_tie_rule_decides(case, with_held):
    """Every token has the same weight and steps at the same lambda: E is large, and the extra frames go to the lowest positions."""
    lens = np.array([130, 130, 7], np.int32)
    cpr = np.array([2, 1], np.int32)
    logits = np.zeros((3, 50, T), np.float32)  # 50 sigmoids of 0: s = 25 / speed
    speeds = np.array([1.0], np.float32)
    fixed = None
    if with_held:
        fixed = np.zeros((3, T), np.int32)
        fixed[0, 3], fixed[0, 129], fixed[1, 64], fixed[2, 2] = 4, 50, 1, 17
    held260 = 0 if fixed is None else 55
    n260, n7 = (260, 7) if fixed is None else (257, 6)
    spans = [(0, 0, 260, held260 + 9 * n260 + 101), (1, 0, 7, (17 if with_held else 0) + 3 * n7 + 2)]  # (neither divides)
    _, fitted, res = _run_and_check(logits, case["src"][:3], spans, fixed=fixed, lens=lens, cpr=cpr, speeds=speeds, compare_plain=False)
    assert res[0]["excess"] == n260 - 101 and res[0]["n_free"] == n260 and res[1]["excess"] == n7 - 2
    free = np.concatenate([fitted[0, :130], fitted[1, :130]])
    if fixed is not None:
        free = free[np.concatenate([fixed[0], fixed[1]]) < 1]
    assert free.tolist() == [10] * 101 + [9] * (n260 - 101)  # (the lowest positions have the extra frame)


def test_weights_at_the_clamps_and_nan_logits(case):
    lens = np.array([33, 20, 70], np.int32)
    cpr = np.array([1, 1, 1], np.int32)
    rng = np.random.default_rng(9)
    logits = (rng.standard_normal((3, 50, T)) * 1.5 - 1.8).astype(np.float32)
    logits[0, :, ::2] = -200.0      # exp(200) is infinite in float32: every sigmoid is 0, s = 0, w = 2^-20
    logits[0, 7, 5] = np.nan        # a NaN logit: w = 1
    logits[0, :, 9] = np.nan
    speeds = np.array([1.0, 1e-6, 1.0], np.float32)  # row 1: s = sum / 1e-6 is above 2^20 everywhere
    logits[2, 0, 11] = np.inf       # a sigmoid of exactly 1
    logits[2, 3, 12] = np.nan
    spans = [(0, 0, 33, 33 + 400), (1, 0, 20, 20 + 57), (2, 5, 60, 55 * 6 + 1)]
    w, fitted, res = _run_and_check(logits, case["src"][:3], spans, lens=lens, cpr=cpr, speeds=speeds, compare_plain=False)
    assert (w[0, 0:33:2] == np.float32(2.0 ** -20)).all() and w[0, 5] == 1.0 and w[0, 9] == 1.0 and w[2, 12] == 1.0
    assert (w[1, :20] == np.float32(2.0 ** 20)).all()
    assert (fitted[0, 0:33:2] == 1).all()  # (a weight of 2^-20 beside ordinary ones never gets past one frame)
    # row 1 is all ties at the top clamp: 57 extra frames over 20 tokens, the lowest 17 positions have one more
    assert fitted[1, :20].tolist() == [4] * 17 + [3] * 3 and res[1]["excess"] == 3


# ---- 2. the model -------------------------------------------------------------------------------------------------------------------
COUNTS = [9, 14, 6, 11]
MCPR = [2, 1, 1]
WORDS = (0x000, 0x100, 0x300)  # f32 at 24 000 Hz, at 8000 Hz and at 48 000 Hz


def _model_inputs(seed0=140):
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    toks = [list(R.synthetic_inputs(1, n - 2, seed=seed0 + i)[0]) for i, n in enumerate(COUNTS)]
    voices = W.synthetic_voices(4)
    styles = [voices[i % 4, n - 2, 0] for i, n in enumerate(COUNTS)]
    return toks, styles


def _mark_at(marks_r, chunk_counts, pos):
    """The mark at token position `pos` of a request (0 .. its tokens, the end included): per chunk its tokens + 1 marks."""
    k = 0
    while k + 1 < len(chunk_counts) and pos > chunk_counts[k]:
        pos -= chunk_counts[k]
        k += 1
    return int(marks_r[sum(c + 1 for c in chunk_counts[:k]) + pos])


def _prosody(rng):
    rate = [rng.choice([0.5, 1.0, 2.0], size=n).astype(np.float32) for n in COUNTS]
    frames = [(rng.integers(1, 7, size=n) * (rng.random(n) < 0.25)).astype(np.int32) for n in COUNTS]
    frames[0][4], frames[0][1], frames[1][0], frames[2][:] = 5, 0, 0, 0
    return rate, frames, None, None


# request 0 (23 tokens over two chunks): a span inside chunk 0 and one across the chunk boundary; request 1: the whole request;
# request 2: no span
def _model_spans(frames):
    held = np.concatenate(frames[:2])
    h = lambda b, e: int(held[b:e].sum())
    return [(0, 1, 5, h(1, 5) + 13), (0, 6, 21, h(6, 21) + 77), (1, 0, 6, V.fit_frames(1.0))]


def test_model_marks_samples_taps_and_report(hip_model):
    from kokorox_amd import hip_koko as hk
    toks, styles = _model_inputs()
    prosody = _prosody(np.random.default_rng(21))
    frames = prosody[1]
    spans = _model_spans(frames)
    hip_model.set_utterance_base(0)
    kw = dict(styles=styles, speeds=[1.1], seed=5)
    chunk_counts = [[9, 14], [6], [11]]
    for word in WORDS:
        L, M = V._RATE_LM[word >> 8]
        flags = hk.KX_FLAG_TAPS if word == 0 else 0
        bodies, marks, rep, fit, samples = hip_model.infer_requests_fitted(toks, MCPR, spans, prosody, fmt=word, marks=True, report=True,
                                                                           with_samples=True, flags=flags, **kw)
        for (r, b, e, fr) in spans:
            assert _mark_at(marks[r], chunk_counts[r], e) - _mark_at(marks[r], chunk_counts[r], b) == 600 * fr * L // M, (word, r, b, e)
        assert samples[1] == 600 * V.fit_frames(1.0) * L // M == 24000 * L // M  # a whole-request span: exactly one second
        assert len(bodies[1]) == samples[1]
        if word == 0:
            # the taps are the numpy definition: per span, the durations of voices.fit_durations on the tapped weights
            w = [hip_model.tap("pred.dur.weights", b)[0] for b in range(4)]
            fitted = [hip_model.tap("pred.dur.fitted", b)[0].view(np.int32) for b in range(4)]
            assert [x.shape[0] for x in w] == COUNTS and [x.shape[0] for x in fitted] == COUNTS
            want = [np.where(f >= 1, f, 0).astype(np.int64) for f in frames]
            w0, h0 = np.concatenate(w[:2]), np.concatenate(want[:2])
            d0 = h0.copy()
            for k, (r, b, e, fr) in enumerate(spans[:2]):
                d, lam, E = V.fit_durations(w0[b:e], fr, h0[b:e])
                d0[b:e] = d
                assert bits(fit[k]["lambda"]) == lam and fit[k]["excess"] == E and fit[k]["held_frames"] == int(h0[b:e].sum())
            d1, lam, E = V.fit_durations(w[2], spans[2][3], want[2])
            assert bits(fit[2]["lambda"]) == lam and fit[2]["excess"] == E and fit[2]["n_free"] == 6
            np.testing.assert_array_equal(np.concatenate(fitted[:2]), d0)
            np.testing.assert_array_equal(fitted[2], d1)
            np.testing.assert_array_equal(fitted[3], want[3])  # (a request without spans: the caller's counts, zeros elsewhere)
            # the report's frames column shows the fitted counts wherever something fixed the token
            col0, col1 = rep[0][:, 3].astype(np.int64), rep[1][:, 3].astype(np.int64)
            assert (col0[d0 >= 1] == d0[d0 >= 1]).all() and (col0 >= 1).all()
            np.testing.assert_array_equal(col1, d1)
            tapped = (d0, d1)
        else:  # (the durations do not depend on the output rate)
            assert (rep[0][:, 3].astype(np.int64)[tapped[0] >= 1] == tapped[0][tapped[0] >= 1]).all()
            np.testing.assert_array_equal(rep[1][:, 3].astype(np.int64), tapped[1])


def test_requests_without_spans_keep_their_bytes_and_no_spans_is_the_prosody_call(hip_model):
    toks, styles = _model_inputs(seed0=160)
    prosody = _prosody(np.random.default_rng(22))
    hip_model.set_utterance_base(0)
    kw = dict(styles=styles, speeds=[0.9, 1.0, 1.2, 1.0], seed=9, fmt=[0x003, 0x202, 0x000])
    JOIN = (7, 20, 50, 2)
    for pros in (prosody, None):
        want = hip_model.infer_requests_prosody(toks, MCPR, pros, joins=JOIN, marks=True, report=True, **kw)
        got = hip_model.infer_requests_fitted(toks, MCPR, [], pros, joins=JOIN, marks=True, report=True, **kw)
        assert len(got[3]) == 0
        for r in range(3):  # n_spans == 0: byte for byte
            assert bytes(got[0][r]) == bytes(want[0][r])
            np.testing.assert_array_equal(got[1][r], want[1][r])
            assert (bits(got[2][r]) == bits(want[2][r])).all()
        # a span in request 1 alone: requests 0 and 2 have the bytes of the call without any
        spans = [(1, 1, 5, 31)] if pros is None else [(1, 1, 5, int(prosody[1][2][1:5].sum()) + 31)]
        one = hip_model.infer_requests_fitted(toks, MCPR, spans, pros, joins=JOIN, marks=True, report=True, **kw)
        for r in (0, 2):
            assert bytes(one[0][r]) == bytes(want[0][r])
            np.testing.assert_array_equal(one[1][r], want[1][r])
            assert (bits(one[2][r]) == bits(want[2][r])).all()
        assert int(one[2][1][1:5, 3].sum()) == 31 and bytes(one[0][1]) != bytes(want[0][1])


def test_dispatcher_fitted_and_plain_requests_share_batches(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    voices = W.synthetic_voices(4)
    reqs = []
    for i in range(8):
        counts = [7 + i, 5] if i % 3 == 0 else [6 + 2 * i]
        chunks = [list(R.synthetic_inputs(1, n - 2, seed=700 + 10 * i + c)[0]) for c, n in enumerate(counts)]
        rows = [voices[(i + c) % 4, n - 2, 0] for c, n in enumerate(counts)]
        n = sum(counts)
        fit = None
        if i % 2 == 1:
            fit = [(0, n, 5 * n + 3)]  # the whole request
        elif i % 4 == 0:
            fit = [(1, 4, 10), (5, n - 1, 3 * (n - 6) + 1)]  # two spans, the second over the chunk boundary where there is one
        reqs.append(dict(chunks=chunks, rows=rows, speed=1.0 + 0.1 * (i % 3), seed=900 + i, fmt=(0, 0x102, 3)[i % 3], fit=fit, marks=i in (1, 2),
                         join=(7, 20, 30, 1) if i in (3, 4) else None))
    d = hk.Dispatcher([hip_model], max_batch=16, max_wait_us=200000)
    out, errs = [None] * 8, []

    def client(i):
        q = reqs[i]
        try:
            out[i] = d.submit_request(q["chunks"], styles=q["rows"], speed=q["speed"], seed=q["seed"], fmt=q["fmt"], marks=q["marks"],
                                      join=q["join"], fit=q["fit"])
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
        if q["fit"] is not None:
            alone = hip_model.infer_requests_fitted(q["chunks"], [len(q["chunks"])], [(0,) + f for f in q["fit"]], None, joins=q["join"],
                                                    marks=q["marks"], **kw)
            assert got[-1].tobytes() == alone[-1].tobytes() and len(got[-1]) == len(q["fit"]), i
            if q["join"] is None and len(q["fit"]) == 1:  # (a whole-request span: the body has exactly its frames)
                L, M = V._RATE_LM[q["fmt"] >> 8]
                per = {0: 4, 2: 2}.get(q["fmt"] & 255)
                if per:
                    assert len(bytes(alone[0][0])) == per * (600 * q["fit"][0][2] * L // M), i
        elif q["join"] is not None:
            alone = (hip_model.infer_requests_joined(q["chunks"], [len(q["chunks"])], q["join"], **kw),)
        elif q["marks"]:
            alone = hip_model.infer_requests_marks(q["chunks"], [len(q["chunks"])], **kw)
        else:
            alone = (hip_model.infer_requests(q["chunks"], [len(q["chunks"])], **kw),)
        assert bytes(got[0]) == bytes(alone[0][0]), i
        if q["marks"]:
            np.testing.assert_array_equal(got[1], alone[1][0])


def test_every_refusal_with_its_text(hip_model):
    from kokorox_amd import hip_koko as hk
    toks, styles = _model_inputs()
    kw = dict(styles=styles, speeds=[1.0], seed=1)
    frames = [np.zeros(n, np.int32) for n in COUNTS]
    frames[0][2] = 6  # token 2 of request 0 is held
    prosody = (None, frames, None, None)
    bad = {
        "unsorted": [(0, 5, 8, 9), (0, 0, 2, 4)],
        "overlap": [(0, 0, 6, 6 + 10), (0, 5, 8, 9)],
        "unsorted by request": [(1, 0, 2, 4), (0, 0, 2, 4)],
        "request < 0": [(-1, 0, 2, 4)],
        "request = R": [(3, 0, 2, 4)],
        "begin = end": [(0, 3, 3, 4)],
        "begin > end": [(0, 4, 3, 4)],
        "begin < 0": [(0, -1, 3, 8)],
        "end past the request": [(0, 0, 24, 60)],
        "end past the last request": [(2, 0, 12, 60)],
        "n = 0": [(0, 2, 3, 6)],
        "G < n": [(0, 0, 5, 6 + 3)],
        "G > 50 n": [(0, 0, 5, 6 + 201)],
    }
    hip_model.set_utterance_base(0)
    for name, spans in bad.items():
        with pytest.raises(hk.KokoroxHipError) as e:
            hip_model.infer_requests_fitted(toks, MCPR, spans, prosody, **kw)
        assert e.value.code == hk.KX_ERR_INVALID and "infer: bad fit" in str(e.value), name
    # the edges themselves are fine: G = n and G = 50 n beside a held token, a span that ends where the request ends
    _, fit = hip_model.infer_requests_fitted(toks, MCPR, [(0, 0, 5, 6 + 4), (0, 5, 23, 50 * 18), (2, 10, 11, 50)], prosody, **kw)
    assert [int(f["n_free"]) for f in fit] == [4, 18, 1] and [int(f["held_frames"]) for f in fit] == [6, 0, 0]
    # a null span array with a count, on the raw entry: *out stays null
    ids, lens = hip_model._ids_lens(toks)
    st = np.ascontiguousarray(np.asarray(styles, np.float32).reshape(4, 256))
    cp, sp, fm = np.array(MCPR, np.int32), np.array([1.0], np.float32), np.array([0], np.int32)
    p = hk._ptr
    one = hk.fit_spans([(0, 0, 2, 4)])
    for spans_arg, n in ((None, 1), (p(one), -1)):
        out, nb, ns = C.c_void_p(), np.zeros(3, np.int64), np.zeros(3, np.int64)
        rc = hip_model._lib.kx_infer_requests_fitted(hip_model._h, p(ids), ids.shape[1], p(lens), 4, p(cp), 3, p(st), None, None, 0, p(sp), 1, 1, 0,
                                                     p(fm), 1, C.byref(out), p(nb), p(ns), None, None, None, 0, None, None, None, spans_arg, n, None)
        assert rc == hk.KX_ERR_INVALID and "infer: bad fit" in hip_model.last_error() and not out.value
    # a model with a pinned duration pattern refuses a call that has spans, and only that
    hip_model.set_pinned_durations([3, 2])
    try:
        with pytest.raises(hk.KokoroxHipError) as e:
            hip_model.infer_requests_fitted(toks, MCPR, [(0, 0, 5, 6 + 10)], prosody, **kw)
        assert e.value.code == hk.KX_ERR_INVALID and "infer: fit with pinned durations" in str(e.value)
        hip_model.infer_requests_fitted(toks, MCPR, [], prosody, **kw)
    finally:
        hip_model.set_pinned_durations(None)
    # the dispatcher checks a request when it is submitted, with its own text; `request` must be 0 there
    d = hk.Dispatcher([hip_model], max_batch=4, max_wait_us=0)
    try:
        two = dict(styles=styles[:2], prosody=(None, frames[:2], None, None))
        for name, spans in bad.items():
            if any(s[0] != 0 for s in spans) or name == "end past the last request":
                continue
            with pytest.raises(hk.KokoroxHipError) as e:
                d.submit_request(toks[:2], fit=[s[1:] for s in spans], **two)
            assert e.value.code == hk.KX_ERR_INVALID and "dispatcher_submit_request: bad fit" in str(e.value), name
        a = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64) for t in toks[:2]]))
        ln = np.array(COUNTS[:2], np.int32)
        rows = np.ascontiguousarray(np.asarray(styles[:2], np.float32).reshape(-1))
        for spans_arg, n in ((None, 1), (p(hk.fit_spans([(1, 0, 2, 4)])), 1)):  # a null array with a count; request 1
            out, nb, ns = C.c_void_p(), C.c_int64(0), C.c_int64(0)
            err = C.create_string_buffer(256)
            rc = hip_model._lib.kx_dispatcher_submit_request_fitted(d._d, p(a), p(ln), 2, p(rows), None, None, 0, 1.0, 1, 0, C.byref(out),
                                                                    C.byref(nb), C.byref(ns), None, None, None, None, None, None, spans_arg, n,
                                                                    None, err, len(err))
            assert rc == hk.KX_ERR_INVALID and err.value == b"dispatcher_submit_request: bad fit" and not out.value
        body, fit = d.submit_request(toks[:2], fit=[(0, 23, 6 + 100)], **two)
        assert int(fit[0]["n_free"]) == 22 and body.shape[0] == 600 * 106
    finally:
        d.close()
