"""GPU: true peak (include/kokorox_hip.h, "levels", True peak) -- request_truepeak_kernel and the two gain kernels that join its
table with the sample peaks, through the test hook behind hip_koko.level_requests / loudness_requests, through
kx_infer_requests_levelled / _loudness and through the dispatcher.  Every interpolated value is one float64 chain in a fixed order,
tp a maximum and g one float64 division, so the checks are EQUALITIES against the numpy definition of kokorox_amd/voices.py
(true_peak, level_gain with the flag): on the dword of tp and on g in the level modes.  A loudness normalisation keeps the 1e-8
relative tolerance of tests/test_gpu_loudness.py on g (the meter's I goes through log10 and pow) unless its ceiling engages, in
which case g is peak / tp and equal.

Every row is poisoned behind its 600 x frames samples with FINITE values of 1e30: a non-finite poison would become a zero by the
definition and hide a read past the row."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUE = 0x100
GAIN, NORMALIZE, CEILING = 0, 1, 2
PLAIN = (GAIN, 1.0, 0.0)
METER, NONE = (0, 0.0, 0.0), (0xFFFFFFFF, 0.0, 0.0)
HEAD, TAIL, INNER = 1, 2, 4
RATES = {0: 24000, 1: 8000, 2: 16000, 3: 48000}
WINDOW = 4096  # host_request.h: LEVEL_WINDOW, the samples of a workgroup of the peak pass and of the true-peak pass
POISON = 1e30


def _interpolated(z):
    """|u_phi[n]| of the definition as float32 [3][N]: where the largest interpolated value sits."""
    from kokorox_amd import voices as V
    z = np.ascontiguousarray(z, dtype=np.float32)
    t = V.true_peak_taps().astype(np.float64)
    x = np.concatenate([np.zeros(11), np.where(np.isfinite(z), z, np.float32(0)).astype(np.float64), np.zeros(12)])
    u = np.zeros((3, z.shape[0]), dtype=np.float32)
    with np.errstate(over="ignore"):
        for phi in range(3):
            acc = np.zeros(z.shape[0])
            for k in range(24):
                acc = acc + t[phi, 23 - k] * x[k: k + z.shape[0]]
            u[phi] = np.abs(acc.astype(np.float32))
    return u


def _rows(parts, frames):
    """[B][ld] with row b = parts[b] (600 x frames[b] samples) and finite poison of alternating sign behind it."""
    ld = 600 * max(frames) + 333
    a = np.empty((len(parts), ld), dtype=np.float32)
    for b, (x, f) in enumerate(zip(parts, frames)):
        assert x.shape == (600 * f,)
        a[b, : 600 * f] = x
        a[b, 600 * f:] = np.float32(POISON) * np.where((np.arange(ld - 600 * f) + b) % 2 == 0, np.float32(1), np.float32(-1))
    return a


def _assert_tp(got_p, got_g, z, spec, what):
    """{f64(p), g} of one flagged level request against the mirror on its stream z: the dword of tp and g, both equal."""
    from kokorox_amd import voices as V
    tp, g = V.level_gain(z, spec)
    assert np.float32(got_p).tobytes() == np.float32(tp).tobytes() and float(got_p) == float(tp), f"{what}: tp {got_p!r}, the mirror has {tp!r}"
    assert float(got_g) == g, f"{what}: g {got_g!r}, the mirror has {g!r}"
    return tp, g


def _body(z, g, word):
    from kokorox_amd import voices as V
    return V.loudness_body(z, g, word)  # (f32(g f64(z)) and the form: the same for a level and a loudness)


# ---- 1: one request of two windows, the largest interpolated value wherever a boundary is ---------------------------------------
def _variant(where):
    """4200 samples of noise of |x| <= 0.1 and a shape that puts the largest interpolated value at a chosen place: a pair of equal
    samples (the value half way between them overshoots both), or at the stream's end a run that alternates and grows, whose
    continuation past the last sample overshoots it (zero extension)."""
    z = np.random.default_rng(20261103).uniform(-0.1, 0.1, 4200).astype(np.float32)
    if where == "end":
        k = np.arange(12)
        z[4199 - k] = (0.9 * (-1.0) ** k * 0.8 ** k).astype(np.float32)
        return z, (4199, None)
    n = {"window_boundary": 4095, "start": 0, "mid_window": 2000}[where]
    z[n] = z[n + 1] = 0.9
    return z, (n, 1)  # (u_2[n], the value at n + 1/2)


VARIANTS = ["window_boundary", "start", "end", "mid_window"]
_ALONE = {}


def _alone(where, code):
    """The variant as the only request of a call, form 0 at rate code `code`, normalised to a true peak of 0.5: cached, the
    reference of the batches below."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    if (where, code) not in _ALONE:
        x, at = _variant(where)
        spec = (NORMALIZE | TRUE, 1.0, 0.5)
        bodies, samples, _, lv = hk.level_requests(_rows([x], [7]), None, None, [1], [code << 8], [spec], frames=[7])
        z = V.resample_stream(x, code << 8)
        assert samples == [z.shape[0]]
        _ALONE[(where, code)] = (x, at, z, spec, bodies[0], lv[0].copy())
    return _ALONE[(where, code)]


@pytest.mark.parametrize("where", VARIANTS)
def test_hook_largest_interpolated_value_at_every_boundary_of_a_two_window_request(where):
    x, (n, phase), z, spec, body, lv = _alone(where, 0)
    assert 4200 == z.shape[0] and WINDOW < 4200 < 2 * WINDOW
    u = _interpolated(z)
    phi, at = np.unravel_index(int(np.argmax(u)), u.shape)
    assert at == n and (phase is None or phi == phase) and u[phi, at] > np.abs(z).max(), (where, phi, at)  # (the shape does what it is for)
    tp, g = _assert_tp(lv[0], lv[1], z, spec, where)
    assert tp == u[phi, at] and tp > np.abs(z).max()
    assert body == _body(z, g, 0), where
    out = np.frombuffer(body, dtype="<f4")
    assert np.abs(out).max() < np.float32(0.5)  # (the samples stay below the ceiling their true peak meets)


# ---- 2: a row boundary 8 samples before a window boundary ----------------------------------------------------------------------
@pytest.mark.parametrize("pair_at", [94199, 94207], ids=["across_the_rows", "across_the_windows"])
def test_hook_a_row_ends_eight_samples_before_a_window_does(pair_at):
    """A 157-frame row and a 1-frame row in one request: the rows meet at 94 200, window 23 begins at 94 208.  The pair sits
    across the row boundary (its interpolated value needs the last samples of one row and the first of the next, and the
    workgroup's halo crosses both boundaries) or across the window boundary inside the short row."""
    from kokorox_amd import hip_koko as hk
    assert 157 * 600 == 94200 and 23 * WINDOW == 94208
    rng = np.random.default_rng(20261104)
    x = rng.uniform(-0.1, 0.1, 94800).astype(np.float32)
    x[pair_at] = x[pair_at + 1] = -0.9
    a = _rows([x[:94200], x[94200:]], [157, 1])
    spec = (CEILING | TRUE, 2.0, 0.75)
    bodies, samples, _, lv = hk.level_requests(a, None, None, [2], [0], [spec], frames=[157, 1])
    assert samples == [94800]
    u = _interpolated(x)
    assert np.unravel_index(int(np.argmax(u)), u.shape) == (1, pair_at)
    tp, g = _assert_tp(lv[0][0], lv[0][1], x, spec, f"pair at {pair_at}")
    assert tp > np.float32(0.9) and g == 0.75 / float(tp) and bodies[0] == _body(x, g, 0)


# ---- 3: a joined request whose seam lies 8 samples behind a window boundary ------------------------------------------------------
def test_hook_joined_request_seam_fade_and_pause_begin_eight_samples_past_a_window():
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    join = (TAIL | INNER, 21, 85, 5)
    lens = [3, 3]
    dur = np.full((2, 512), -7, dtype=np.int32)
    dur[0, :3], dur[1, :3] = [2, 4, 1], [1, 3, 2]
    rng = np.random.default_rng(20261105)
    for variant in ("loud_before_the_seam", "loud_in_the_cut", "loud_behind_the_pause"):
        parts = [rng.uniform(-0.1, 0.1, 4200).astype(np.float32), rng.uniform(-0.1, 0.1, 3600).astype(np.float32)]
        if variant == "loud_before_the_seam":
            parts[0][4060:4104] = np.float32(3.0) * np.where(np.arange(44) % 3 == 0, np.float32(-1), np.float32(1))  # (inside the fade of 120)
        elif variant == "loud_in_the_cut":
            parts[0][4104:] = 5.0  # (cut: counts nowhere)
        else:
            parts[1][96 + 130] = parts[1][96 + 131] = 0.9  # (the second chunk's kept samples begin at skip = 600 - 504: behind its fade of 120)
        a = _rows(parts, [7, 6])
        z = V.join_stream(parts, [[2, 4, 1], [1, 3, 2]], join)
        assert z[4103] != 0 and not z[4104: 4104 + 2040].any() and z[4104 + 2040] != 0 and 4104 == WINDOW + 8  # keep, the pause, the next chunk
        spec = (NORMALIZE | TRUE, 1.0, 1.0)
        bodies, samples, _, lv = hk.level_requests(a, dur, lens, [2], [0], [spec], joins=[join])
        assert samples == [z.shape[0]]
        tp, g = _assert_tp(lv[0][0], lv[0][1], z, spec, variant)
        assert tp > np.abs(z).max() and (variant != "loud_in_the_cut" or tp < 0.2) and bodies[0] == _body(z, g, 0), variant


# ---- 4: the y path, beside a request of amplitude 1e30 ------------------------------------------------------------------------
@pytest.mark.parametrize("code", [1, 2, 3], ids=["8000", "16000", "48000"])
def test_hook_resampled_request_reads_nothing_of_the_run_behind_its_own(code):
    """The variants of case 1 at a rate code, each in one batch with a following request of 1e30 throughout (a constant: the
    resampler passes it, where it would filter an alternating one away): the two runs lie back to back in the resampled buffer,
    and a halo read past the first one's end would put 1e30 into its last interpolated values."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    big = np.full(600, POISON, dtype=np.float32)
    zbig = V.resample_stream(big, code << 8)
    for where in VARIANTS:
        x, _, z, spec, body, lv = _alone(where, code)
        _assert_tp(lv[0], lv[1], z, spec, f"{where} alone at rate code {code}")
        assert body == _body(z, float(lv[1]), code << 8)
        a = _rows([x, big], [7, 1])
        bodies, samples, _, both = hk.level_requests(a, None, None, [1, 1], [code << 8] * 2, [spec, (TRUE, 1.0, 0.0)], frames=[7, 1])
        assert samples == [z.shape[0], zbig.shape[0]]
        assert both[0].tobytes() == lv.tobytes() and bodies[0] == body, f"{where} at rate code {code}: beside 1e30"
        _assert_tp(both[1][0], both[1][1], zbig, (TRUE, 1.0, 0.0), "the request of 1e30")
        assert both[1][0] >= 0.99e30  # (the constant comes through the resampler at gain 1 within its ripple)


# ---- 5: flagged and unflagged requests in one batch ----------------------------------------------------------------------------
MIXED_WORDS = [0x000, 0x302, 0x108, 0x204, 0x000, 0x303]


def _mixed_inputs():
    rng = np.random.default_rng(20261106)
    frames = [20] * 6
    # noise, and in its middle a short loud burst of a sine near 0.3 of the request's OUTPUT rate: few samples per period, so the
    # largest value lies between two of them and tp > p at every rate (the largest sample of plain noise is often its true peak)
    tone = {0x000: 7000.0, 0x302: 9000.0, 0x108: 2900.0, 0x204: 5000.0, 0x303: 9000.0}
    n = np.arange(64)
    parts = []
    for s, word in zip((0.3, 0.15, 0.6, 0.3, 0.15, 0.3), MIXED_WORDS):
        x = rng.uniform(-0.3 * s, 0.3 * s, 12000)
        x[6000:6064] += 3.0 * s * np.sin(2 * np.pi * tone[word] * n / 24000.0 + 0.3) * np.hanning(64)
        parts.append(x.astype(np.float32))
    dur = np.full((6, 512), -7, dtype=np.int32)
    dur[:, :3] = [5, 10, 5]
    return _rows(parts, frames), parts, dur, [3] * 6


def test_hook_flagged_and_unflagged_requests_share_a_batch():
    """Flagged level, flagged meter, flagged loudness normalisation (its ceiling engages), unflagged level, unflagged loudness and a
    plain request in one launch.  The unflagged ones give the {p, g}, bodies and marks of the same call with no flag in the batch;
    the flagged ones equal themselves run alone."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    a, parts, dur, lens = _mixed_inputs()
    words = MIXED_WORDS
    levels = [(NORMALIZE | TRUE, 1.0, 0.5), PLAIN, PLAIN, (CEILING, 8.0, 0.75), PLAIN, PLAIN]
    louds = [NONE, (0 | TRUE, 0.0, 0.0), (1 | TRUE, -3.0, 0.25), NONE, (1, -23.0, 1.0), NONE]
    want = [True] * 6
    strip = lambda specs: [(m & ~TRUE if m != 0xFFFFFFFF else m, x, y) for m, x, y in specs]  # noqa: E731
    bodies, samples, marks, out, hops = hk.loudness_requests(a, dur, lens, [1] * 6, words, louds, levels=levels, want=want)
    b0, s0, m0, out0, hops0 = hk.loudness_requests(a, dur, lens, [1] * 6, words, strip(louds), levels=strip(levels), want=want)
    assert samples == s0
    for r in range(6):
        np.testing.assert_array_equal(marks[r], m0[r])
        assert hops[r].tobytes() == hops0[r].tobytes()
        if r in (3, 4, 5):  # unflagged: nothing of them moved
            assert bodies[r] == b0[r] and out[r].tobytes() == out0[r].tobytes(), r
        else:                # flagged: the reported peak grew, the loudness did not move
            assert out[r][0] > out0[r][0] and out[r][2:].tobytes() == out0[r][2:].tobytes(), r
    # the flagged ones against themselves alone, and against the mirror
    for r in (0, 1, 2):
        one = slice(r, r + 1)
        if louds[r] == NONE:
            sb, _, sm, slv = hk.level_requests(a[one], dur[one], lens[one], [1], words[one], levels[one], want=[True])
            assert sb[0] == bodies[r] and slv[0].tobytes() == out[r][:2].tobytes(), r
        else:
            sb, _, sm, sout, shops = hk.loudness_requests(a[one], dur[one], lens[one], [1], words[one], louds[one], want=[True])
            assert sb[0] == bodies[r] and sout[0].tobytes() == out[r].tobytes() and shops[0].tobytes() == hops[r].tobytes(), r
        np.testing.assert_array_equal(sm[0], marks[r])
        z = V.resample_stream(parts[r], words[r])
        tp = V.true_peak(z)
        assert np.float32(out[r][0]).tobytes() == tp.tobytes() and float(out[r][0]) == float(tp), r
        if louds[r] == NONE:
            _assert_tp(out[r][0], out[r][1], z, levels[r], f"request {r}")
        else:
            g = V.loudness_gain(tp, float(out[r][2]), louds[r])
            engaged = louds[r][0] & 1 and g == float(np.float64(np.float32(louds[r][2])) / np.float64(tp))
            assert (float(out[r][1]) == g) if engaged or not louds[r][0] & 1 else (abs(float(out[r][1]) - g) <= 1e-8 * g), r
            assert engaged == (r == 2)
        assert bodies[r] == _body(z, float(out[r][1]), words[r]), r


# ---- 6: non-finite samples in and beside the peak -------------------------------------------------------------------------------
def test_hook_nan_and_infinities_in_and_beside_the_peak():
    from kokorox_amd import hip_koko as hk
    base, _ = _variant("window_boundary")
    cases = {}
    for name, edits in (("nan_in_the_pair", {4096: np.nan}), ("nan_beside_the_pair", {4094: np.nan, 4097: np.nan}),
                        ("inf_far_from_the_pair", {100: np.inf}), ("minus_inf_beside_the_pair", {4097: -np.inf}),
                        ("nan_and_inf", {4095: np.nan, 4096: np.inf}), ("finite_samples_whose_value_between_overflows", {2000: 3e38, 2001: 3e38}),
                        ("nothing_but_nan", None)):
        z = base.copy()
        if edits is None:
            z[:] = np.nan
        else:
            for at, v in edits.items():
                z[at] = v
        cases[name] = z
    names = sorted(cases)
    a = _rows([cases[n] for n in names], [7] * len(names))
    for spec in ((NORMALIZE | TRUE, 1.0, 0.5), (CEILING | TRUE, 3.0, 0.5)):
        bodies, _, _, lv = hk.level_requests(a, None, None, [1] * len(names), [0] * len(names), [spec] * len(names), frames=[7] * len(names))
        for r, n in enumerate(names):
            tp, g = _assert_tp(lv[r][0], lv[r][1], cases[n], spec, f"{n} {spec}")
            want = np.frombuffer(_body(cases[n], g, 0), dtype="<u4")
            got = np.frombuffer(bodies[r], dtype="<u4")
            nan = np.isnan(want.view("<f4"))
            assert np.array_equal(np.isnan(got.view("<f4")), nan) and np.array_equal(got[~nan], want[~nan]), n
            if "inf" in n or "overflows" in n:
                assert tp == np.float32(np.inf) and g == (1.0 if spec[0] & 3 == NORMALIZE else 3.0), n  # unusable
            if n == "finite_samples_whose_value_between_overflows":
                assert np.isfinite(cases[n]).all()
            if n == "nothing_but_nan":
                assert tp == 0 and g == (1.0 if spec[0] & 3 == NORMALIZE else 3.0)


# ---- 7: the bodies ----------------------------------------------------------------------------------------------------------------
def test_hook_bodies_in_the_16_bit_forms_never_clip_under_a_true_peak_of_one():
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    rng = np.random.default_rng(20261107)
    x = rng.uniform(-3.0, 3.0, 4200).astype(np.float32)  # (far outside +-1: the plain 16-bit forms would clip it; bounded: tp > p)
    spec = (NORMALIZE | TRUE, 1.0, 1.0)
    for code in (0, 3):
        z = V.resample_stream(x, code << 8)
        words = [f | code << 8 for f in (0, 2, 4, 8)]
        bodies, _, _, lv = hk.level_requests(_rows([x] * 4, [7] * 4), None, None, [1] * 4, words, [spec] * 4, frames=[7] * 4)
        for r, word in enumerate(words):
            tp, g = _assert_tp(lv[r][0], lv[r][1], z, spec, f"word {word:#x}")
            assert bodies[r] == _body(z, g, word), f"word {word:#x}"
        out = np.frombuffer(bodies[0], dtype="<f4")
        pcm = np.frombuffer(bodies[1], dtype="<i2")
        # no |sample| passes the ceiling its true peak meets, so the clamp never engages; at 24 kHz, where the values between the
        # samples of this noise pass the largest of them, the samples stay well below it (resampled, that sample can be the true peak)
        assert np.abs(out).max() <= 1.0 and tp >= np.abs(z).max() and (code != 0 or (tp > np.abs(z).max() and np.abs(out).max() < 0.7))
        assert np.array_equal(pcm, np.trunc(out * np.float32(32767.0)).astype("<i2")) and np.abs(pcm.astype(np.int32)).max() <= 32767
        assert np.abs(np.frombuffer(V.stream_body(z, 2 | code << 8), dtype="<i2").astype(np.int32)).max() == 32767  # (unlevelled it clips)


# ---- 8: the model ---------------------------------------------------------------------------------------------------------------
def _chunks():
    from oracle import kokoro_ref as R
    return [list(int(v) for v in R.synthetic_inputs(1, k, seed=500 + k)[0]) for k in (1, 10, 3, 5, 2, 7)]


def _raw_of(x):
    return x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()


def test_model_unpinned_levelled_requests_with_the_flag_equal_the_mirror_of_their_plain_result(hip_model):
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    toks = _chunks()
    rows = [tab[b % 4, len(t) - 2, 0] for b, t in enumerate(toks)]
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations(None)
    cpr = [2, 1, 3]
    kw = dict(styles=rows, speeds=[1.0], seed=23)
    specs = [(NORMALIZE | TRUE, 1.0, 0.5), (NORMALIZE, 1.0, 0.5), (CEILING | TRUE, 64.0, 1.0)]
    for code, form, joins in ((0, 0, None), (3, 2, (HEAD | TAIL | INNER, 10, 85, 1)), (1, 8, None)):
        word = form | code << 8
        if joins is None:
            z = hip_model.infer_requests(toks, cpr, fmt=code << 8, **kw)
        else:
            z = hip_model.infer_requests_joined(toks, cpr, joins, fmt=code << 8, **kw)
        bodies, lv = hip_model.infer_requests_levelled(toks, cpr, specs, joins=joins, fmt=word, **kw)
        for r in range(3):
            what = f"word {word:#x} joins {joins} request {r}"
            tp, g = _assert_tp(lv[r][0], lv[r][1], z[r], specs[r], what)
            assert tp >= np.abs(z[r]).max() and (specs[r][0] & TRUE or tp == np.abs(z[r]).max()), what
            assert _raw_of(bodies[r]) == _body(z[r], g, word), what
    # loudness with the flag: p is tp, the ceiling is peak / tp
    spec = (1 | TRUE, -1.0, 0.5)
    z = hip_model.infer_requests(toks, [6], fmt=0, **kw)
    bodies, out = hip_model.infer_requests_loudness(toks, [6], spec, fmt=2, **kw)
    tp = V.true_peak(z[0])
    g = V.loudness_gain(tp, float(out[0][2]), spec)
    engaged = g == float(np.float64(np.float32(0.5)) / np.float64(tp))
    assert np.float32(out[0][0]).tobytes() == tp.tobytes()
    assert (float(out[0][1]) == g) if engaged else (abs(float(out[0][1]) - g) <= 1e-8 * g)
    assert _raw_of(bodies[0]) == _body(z[0], float(out[0][1]), 2)


def test_tts_request_passes_the_flag_through(hip_model):
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    styles = {"v": W.synthetic_voices(1)[0]}
    chunks = [[5, 9, 12], [7, 3]]
    hip_model.set_utterance_base(0)
    plain = V.tts_request(hip_model, styles, "v", chunks, seed=4, fmt=0x200)
    spec = (NORMALIZE | TRUE, 1.0, 0.25)
    got = V.tts_request(hip_model, styles, "v", chunks, seed=4, fmt=0x200, level=spec)
    assert got.tobytes() == V.level_stream(plain, spec).tobytes() and float(np.abs(got).max()) <= 0.25
    assert got.tobytes() != V.level_stream(plain, (NORMALIZE, 1.0, 0.25)).tobytes()  # (the flag reached the GPU)


# ---- 10: the refusals through the real entries ----------------------------------------------------------------------------------
def test_refusals_through_the_model_and_the_dispatcher(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    toks = _chunks()[:3]
    rows = [W.synthetic_voices(1)[0, len(t) - 2, 0] for t in toks]
    kw = dict(styles=rows, speeds=[1.0], seed=5)
    hip_model.set_pinned_durations([1])
    try:
        for ok in ((0x100, 2.0, 0.0), (0x101, 1.0, 0.5), (0x102, 2.0, 0.5)):
            hip_model.infer_requests_levelled(toks, [1, 2], [PLAIN, ok], **kw)
        for ok in ((0x100, 0.0, 0.0), (0x101, -23.0, 0.5)):
            hip_model.infer_requests_loudness(toks, [1, 2], [METER, ok], **kw)
        for bad in ((0x200, 1.0, 0.0), (0x301, 1.0, 0.5), (0x103, 1.0, 0.5), (0x80000100, 1.0, 0.0), (0xFFFFFFFF, 1.0, 0.0), (0x101, 2.0, 0.5),
                    (0x100, 1.0, 0.5)):
            with pytest.raises(hk.KokoroxHipError) as e:
                hip_model.infer_requests_levelled(toks, [1, 2], [PLAIN, bad], **kw)
            assert e.value.code == hk.KX_ERR_INVALID and str(e.value).endswith("infer: bad level"), bad
        for bad in ((0x200, 0.0, 0.0), (0x301, -23.0, 0.5), (0x103, -23.0, 0.5), (0x102, -23.0, 0.5), (0xFFFFFFFF, 0.0, 0.0), (0x100, -23.0, 0.0)):
            with pytest.raises(hk.KokoroxHipError) as e:
                hip_model.infer_requests_loudness(toks, [1, 2], [METER, bad], **kw)
            assert e.value.code == hk.KX_ERR_INVALID and str(e.value).endswith("infer: bad loudness"), bad
        d = hk.Dispatcher([hip_model], max_batch=4, max_wait_us=0)
        try:
            d.submit_request(toks, styles=rows, seed=5, level=(0x101, 1.0, 0.5))
            d.submit_request(toks, styles=rows, seed=5, loudness=(0x100, 0.0, 0.0))
            for bad in ((0x200, 1.0, 0.0), (0x301, 1.0, 0.5), (0x103, 1.0, 0.5), (0xFFFFFFFF, 1.0, 0.0)):
                with pytest.raises(hk.KokoroxHipError) as e:
                    d.submit_request(toks, styles=rows, seed=5, level=bad)
                assert e.value.code == hk.KX_ERR_INVALID and str(e.value).endswith("dispatcher_submit_request: bad level"), bad
            for bad in ((0x200, 0.0, 0.0), (0x301, -23.0, 0.5), (0x103, -23.0, 0.5), (0x102, -23.0, 0.5), (0xFFFFFFFF, 0.0, 0.0)):
                with pytest.raises(hk.KokoroxHipError) as e:
                    d.submit_request(toks, styles=rows, seed=5, loudness=bad)
                assert e.value.code == hk.KX_ERR_INVALID and str(e.value).endswith("dispatcher_submit_request: bad loudness"), bad
        finally:
            d.close()
    finally:
        hip_model.set_pinned_durations(None)


# ---- 9: the dispatcher ----------------------------------------------------------------------------------------------------------
def _request_specs():
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    tab = W.synthetic_voices(4)
    words = [0, 0x108, 0x302, 4, 0x202, 0x109, 3, 0x301]
    joins = [None, (HEAD | TAIL | INNER, 20, 150, 5), None, (INNER, 0, 85, 12)]
    # flagged and unflagged levels and loudness, and plain requests (None, None), mixed in every batch
    kinds = [((NORMALIZE | TRUE, 1.0, 0.5), None), (None, (1 | TRUE, -3.0, 0.25)), ((NORMALIZE, 1.0, 0.5), None), (None, None),
             (None, (0 | TRUE, 0.0, 0.0)), ((CEILING | TRUE, 64.0, 1.0), None), (None, (1, -23.0, 1.0))]
    specs = []
    for i in range(16):
        n = 1 + i % 3
        chunks = [list(int(v) for v in R.synthetic_inputs(1, 1 + (5 * i + 3 * c) % 10, seed=900 + 10 * i + c)[0]) for c in range(n)]
        voice = dict(styles=[tab[i % 4, len(c) - 2, 0] for c in chunks]) if i % 2 == 0 else dict(voices=i % 4)
        level, loudness = kinds[i % len(kinds)]
        specs.append(dict(chunks=chunks, voice=voice, fmt=words[i % len(words)], seed=9700 + i, speed=1.0 + 0.125 * (i % 2),
                          marks=(i // 3) % 2 == 0, join=joins[i % len(joins)], level=level, loudness=loudness))
    return tab, specs


def _solo(model, s):
    """The request through the direct call with R = 1: the tuple Dispatcher.submit_request returns for it."""
    n = len(s["chunks"])
    v = s["voice"]
    kw = dict(styles=v["styles"]) if "styles" in v else dict(voice_ids=[[v["voices"]]] * n, weights=[[0.0]] * n)
    kw.update(speeds=[s["speed"]], seed=s["seed"], fmt=s["fmt"])
    if s["loudness"] is not None:
        res = model.infer_requests_loudness(s["chunks"], [n], s["loudness"], joins=s["join"], marks=s["marks"], **kw)
    elif s["level"] is not None:
        res = model.infer_requests_levelled(s["chunks"], [n], s["level"], joins=s["join"], marks=s["marks"], **kw)
    else:
        res = model.infer_requests_joined(s["chunks"], [n], s["join"] if s["join"] is not None else (0, 0, 0, 0), marks=s["marks"], **kw)
        res = res if s["marks"] else (res,)
    return tuple(part[0] for part in res)


def _dispatcher_scenario(model):
    """8 client threads, 16 requests of 1..3 chunks: flagged and unflagged levels and loudness and plain requests, with and without
    joins and marks, rates and forms mixed; everything a request gets back equals the direct call of the request alone: its tp and
    g do not depend on what it was batched with."""
    from kokorox_amd import hip_koko as hk
    tab, specs = _request_specs()
    model.set_voice_table(tab)
    model.set_utterance_base(0)
    model.set_pinned_durations(None)
    d = hk.Dispatcher([model], max_batch=8, max_wait_us=100000)
    out = [None] * len(specs)
    errs = []

    def client(t):
        try:
            for i in (t, t + 8):
                s = specs[i]
                out[i] = d.submit_request(s["chunks"], speed=s["speed"], seed=s["seed"], fmt=s["fmt"], marks=s["marks"], join=s["join"],
                                          level=s["level"], loudness=s["loudness"], **s["voice"])
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
    grew = 0
    for i, s in enumerate(specs):
        want = _solo(model, s)
        got = out[i] if isinstance(out[i], tuple) else (out[i],)
        assert len(got) == len(want), i
        for g, w in zip(got, want):
            assert _raw_of(g) == _raw_of(w) and type(g) is type(w), i
        spec = s["level"] if s["level"] is not None else s["loudness"]
        if spec is not None and spec[0] & TRUE:  # (the flag reached the batch: the reported peak is above the sample peak)
            unflagged = _solo(model, dict(s, marks=False, **{"level" if s["level"] is not None else "loudness": (spec[0] & ~TRUE,) + spec[1:]}))
            grew += float(got[-1][0]) > float(unflagged[-1][0])
    assert grew >= 6
    assert st["requests"] == len(specs) and st["batches"] < st["requests"]
    return st


def test_dispatcher_flagged_and_unflagged_requests_equal_their_solo_runs(hip_model):
    _dispatcher_scenario(hip_model)


def test_dispatcher_copy_out_path_in_a_fresh_process():
    """KX_PINNED_LIVE_CAP_MB is read once per process: with 0 every request's body and marks are copied out into plain
    allocations; the levels and the loudness travel beside them."""
    env = dict(os.environ, KX_PINNED_LIVE_CAP_MB="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "copy-out scenario passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before libkokorox_hip.so: one shared HIP runtime)
    from kokorox_amd import hip_koko as _hk
    from kokorox_amd import weights as _W
    _m = _hk.HipKoko.new(_W.ensure_synthetic_blob())
    try:
        print("stats", _dispatcher_scenario(_m))
    finally:
        _m.close()
    print("copy-out scenario passed")
