"""GPU: levels (include/kokorox_hip.h, "levels") -- the peak pass, the gain kernel and the levelled packer through their test
hook, through kx_infer_requests_levelled and through the dispatcher.  A peak is a maximum, the gain one float64 division and
every sample one float64 product, so every check is an EQUALITY against the numpy definition of kokorox_amd/voices.py
(level_gain, level_stream behind join_stream and resample_stream, then the form mirrors).  The only latitude is the one
tests/test_gpu_resample.py takes: in the float forms a NaN must be a NaN where the mirror has one, its sign and payload are not
compared."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPINGS = {"six_single": [1] * 6, "two_one_three": [2, 1, 3], "one_of_six": [6]}
FORMS = [0, 8, 3, 1, 4, 9, 2]
HEAD, TAIL, INNER = 1, 2, 4
NO_JOIN = (0, 0, 0, 0)
GAIN, NORMALIZE, CEILING = 0, 1, 2
PLAIN = (GAIN, 1.0, 0.0)
# a gain, a normalisation, a ceiling that engages on the inputs below (their peaks are about 0.3) and one that stays out
SPECS = [(GAIN, 2.5, 0.0), (NORMALIZE, 1.0, 0.5), (CEILING, 8.0, 0.75), (CEILING, 1.5, 1.0)]
LEVEL_WINDOW = 4096  # host_request.h: samples of a request's stream per workgroup of the peak pass


def _firsts(cpr):
    return np.concatenate([[0], np.cumsum(cpr)]).astype(int)


def _assert_body(got, want, word, what):
    """Byte equality; in the float forms a NaN must be a NaN where the mirror has one (sign and payload apart)."""
    assert len(got) == len(want), f"{what}: {len(got)} bytes, the mirror has {len(want)}"
    form = word & 0xFF
    if form in (0, 1, 3):
        head = 44 if form == 3 else 0
        assert got[:head] == want[:head], f"{what}: header"
        g, w = np.frombuffer(got[head:], dtype="<u4"), np.frombuffer(want[head:], dtype="<u4")
        gn, wn = np.isnan(g.view("<f4")), np.isnan(w.view("<f4"))
        np.testing.assert_array_equal(gn, wn, err_msg=what)
        bad = np.flatnonzero((g != w) & ~wn)
        assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} samples differ, the first at {int(bad[0])}: {g[bad[0]]:#x} vs {w[bad[0]]:#x}"
    else:
        i = next((j for j in range(len(got)) if got[j] != want[j]), None)
        assert i is None, f"{what}: first difference at byte {i}: {got[max(0, i - 8): i + 8]!r} vs {want[max(0, i - 8): i + 8]!r}"


def _assert_levels(got, z, level, what):
    """out_levels of one request against the mirror on its stream z: f64(p) and g, both exact."""
    from kokorox_amd import voices as V
    p, g = V.level_gain(z, level)
    assert (float(got[0]), float(got[1])) == (float(p), g), f"{what}: levels {tuple(got)}, the mirror has {(float(p), g)}"
    return p, g


# ---- the peak wherever it sits ------------------------------------------------------------------------------------------------
SPIKE_AT = [0, 9599, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 5000, 9598, 1]


@pytest.fixture(scope="module")
def sweep_inputs():
    """40 single-row requests of 16 frames: noise of |x| <= 0.1 and one sample of +-0.7, at the first and the last sample and on
    both sides of every boundary a lane, a wave, a workgroup's window or a packer window can have; rows poisoned behind their
    9600 samples."""
    rng = np.random.default_rng(20263)
    n = 9600
    a = np.empty((2 * len(SPIKE_AT), n + 333), dtype=np.float32)
    a[:, :n] = rng.uniform(-0.1, 0.1, (a.shape[0], n)).astype(np.float32)
    a[:, n:] = np.array([1e30, np.inf, -1e30, -np.inf], dtype=np.float32)[np.arange(333) % 4]
    for i, at in enumerate(SPIKE_AT):
        a[2 * i, at], a[2 * i + 1, at] = 0.7, -0.7
    return a


@pytest.mark.parametrize("code", [0, 1, 2, 3], ids=["24000", "8000", "16000", "48000"])
def test_hook_peak_position_sweep(sweep_inputs, code):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    a = sweep_inputs
    R = a.shape[0]
    assert 2 * LEVEL_WINDOW < 9600 < 3 * LEVEL_WINDOW  # (three windows of the peak pass at 24 kHz, the last one partial)
    words = [FORMS[r % len(FORMS)] | code << 8 for r in range(R)]
    levels = [[PLAIN, (NORMALIZE, 1.0, 1.0), (CEILING, 4.0, 0.5), (GAIN, 0.5, 0.0)][(r // 2) % 4] for r in range(R)]
    bodies, samples, _, lv = hk.level_requests(a, None, None, [1] * R, words, levels, frames=[16] * R)
    assert lv.shape == (R, 2)
    for r in range(R):
        z = V.resample_stream(a[r, :9600], words[r])
        what = f"row {r} spike at {SPIKE_AT[r // 2]} word {words[r]:#x} level {levels[r]}"
        assert samples[r] == z.shape[0], what
        p, _ = _assert_levels(lv[r], z, levels[r], what)
        if code == 0:
            assert p == np.float32(0.7), what
        _assert_body(bodies[r], V.stream_body(V.level_stream(z, levels[r]), words[r]), words[r], what)


# ---- the hook's inputs: six rows that reach every seam, quiet enough that every spec has something to do ---------------------------
HOOK_LENS = [3, 5, 1, 4, 2, 3]


def _hook_inputs():
    """Durations 2..5 frames per token (rows of 1200 to 15 000 samples, so requests have one to several peak windows), distinct
    samples of |x| <= 0.3, and behind every row's 600 x frames[b] samples 1e30 and +-inf, which must reach nothing."""
    rng = np.random.default_rng(20264)
    dur = np.empty((6, 512), dtype=np.int32)
    dur[:, 0::2] = 2 ** 31 - 1
    dur[:, 1::2] = -7
    for b, n in enumerate(HOOK_LENS):
        dur[b, :n] = rng.integers(2, 6, size=n)
    frames = [int(dur[b, :n].sum()) for b, n in enumerate(HOOK_LENS)]
    ld = 600 * max(frames) + 555
    a = np.empty((6, ld), dtype=np.float32)
    total = 600 * sum(frames)
    values = (-0.3 + 0.6 * (rng.permutation(total) + 0.5) / total).astype(np.float32)
    o = 0
    for b, f in enumerate(frames):
        n = 600 * f
        a[b, :n] = values[o: o + n]
        a[b, n:] = np.array([1e30, np.inf, -np.inf, -1e30], dtype=np.float32)[(np.arange(ld - n) + b) % 4]
        o += n
    return a, dur, frames


@pytest.fixture(scope="module")
def hook_inputs():
    return _hook_inputs()


class _Mirror:
    """The numpy definition, request by request, with the resampled streams computed once per (rows, join, rate)."""

    def __init__(self, audio, dur, lens):
        self.audio, self.dur, self.lens, self.cache = audio, dur, lens, {}

    def durations(self, b0, b1):
        return [[int(v) for v in self.dur[b, : self.lens[b]]] for b in range(b0, b1)]

    def stream(self, b0, b1, join, word):
        from kokorox_amd import voices as V
        key = (b0, b1, tuple(join), word & 0xF00)
        if key not in self.cache:
            d = self.durations(b0, b1)
            x = V.join_stream([self.audio[b, : 600 * sum(d[b - b0])] for b in range(b0, b1)], d, join)
            self.cache[key] = V.resample_stream(x, word & 0xF00)
        return self.cache[key]


def _run_and_compare(mirror, cpr, words, levels, joins=None, want=None):
    """One call of the hook against the mirror: bodies, sample counts, levels, and the marks (which levels must not change)."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    R = len(cpr)
    bodies, samples, marks, lv = hk.level_requests(mirror.audio, mirror.dur, mirror.lens, cpr, words, levels, joins=joins, want=want)
    first = _firsts(cpr)
    out = []
    for r in range(R):
        join = joins[r] if joins is not None else NO_JOIN
        z = mirror.stream(first[r], first[r + 1], join, words[r])
        what = f"grouping {cpr} request {r} word {words[r]:#x} join {join} level {levels[r]}"
        assert samples[r] == z.shape[0], what
        out.append(_assert_levels(lv[r], z, levels[r], what))
        _assert_body(bodies[r], V.stream_body(V.level_stream(z, levels[r]), words[r]), words[r], what)
        if want is not None and want[r]:
            np.testing.assert_array_equal(marks[r], V.joined_marks(mirror.durations(first[r], first[r + 1]), words[r], join), err_msg=what)
        else:
            assert marks[r].shape[0] == 0, what
    return bodies, out


@pytest.fixture(scope="module")
def mirror(hook_inputs):
    a, dur, _ = hook_inputs
    return _Mirror(a, dur, HOOK_LENS)


# ---- what must not count and what must ------------------------------------------------------------------------------------------
def test_hook_what_counts_and_what_does_not(hook_inputs):
    from kokorox_amd import voices as V
    base, dur, frames = hook_inputs
    cpr, trim = [2, 1, 3], (HEAD | TAIL | INNER, 0, 85, 12)
    joins = [trim, NO_JOIN, trim]
    norm = [(NORMALIZE, 1.0, 0.5)] * 3
    for code in range(4):
        words = [0x000 | code << 8, 0x003 | code << 8, 0x002 | code << 8]
        # the poison behind every row (1e30, +-inf) reaches no peak: every p is that of the quiet samples
        _, lv0 = _run_and_compare(_Mirror(base, dur, HOOK_LENS), cpr, words, norm, joins, want=[True, False, True])
        assert all(0.25 < float(p) < 0.6 for p, _ in lv0)  # (about 0.3; the resampler adds its overshoot)
        # a spike inside a cut pad does not count: sample 7 of row 0's lead span, which keep 0 cuts whole
        a = base.copy()
        a[0, 7] = 0.95
        _, lv = _run_and_compare(_Mirror(a, dur, HOOK_LENS), cpr, words, norm, joins)
        assert lv == lv0
        # ... and counts where no join cuts it
        _, lv = _run_and_compare(_Mirror(a, dur, HOOK_LENS), cpr, words, norm)
        if code == 0:
            assert lv[0][0] == np.float32(0.95) and lv[0][0] > lv0[0][0]
        # a spike inside a fade counts at its faded value: sample 5 of row 0's kept segment, gain 11 / 576 of 50
        a = base.copy()
        a[0, 600 * int(dur[0, 0]) + 5] = 50.0
        _, lv = _run_and_compare(_Mirror(a, dur, HOOK_LENS), cpr, words, norm, joins)
        if code == 0:
            assert lv[0][0] == np.float32(np.float64(50.0) * (np.float64(11) / np.float64(576))) and lv[0][0] < 1.0
        # a step of 0.5 over 600 samples as the single-row request: at 24 kHz its peak is 0.5, resampled it overshoots, and p
        # follows the resampled stream
        a = base.copy()
        a[2, : 600 * frames[2]] = 0.0
        a[2, 300:900] = 0.5
        _, lv = _run_and_compare(_Mirror(a, dur, HOOK_LENS), cpr, words, norm, joins)
        assert (lv[1][0] == np.float32(0.5)) if code == 0 else (np.float32(0.52) < lv[1][0] < np.float32(0.6))
        # a NaN is skipped and stays in the output; an +inf makes p unusable: g = 1 when normalising, the gain under a ceiling
        a = base.copy()
        a[3, 600 * int(dur[3, 0]) + 600] = np.nan   # (inside row 3's second token: kept, never faded)
        a[4, 20] = np.inf                            # (a row of two tokens is never trimmed)
        a[1, 600 * int(dur[1, 0]) + 700] = -np.inf
        m = _Mirror(a, dur, HOOK_LENS)
        bodies, lv = _run_and_compare(m, cpr, words, [(NORMALIZE, 1.0, 0.5), (CEILING, 3.0, 0.5), (NORMALIZE, 1.0, 0.5)], joins)
        assert lv[0][0] == np.inf and lv[0][1] == 1.0 and lv[2][0] == np.inf and lv[2][1] == 1.0
        if code == 0:
            z = np.frombuffer(bodies[0], dtype="<f4")
            assert np.isinf(z).sum() == 1 and np.array_equal(z, m.stream(0, 2, trim, 0))
        # a NaN alone: p is that of the other samples
        a = base.copy()
        a[2, 100] = np.nan
        bodies, lv = _run_and_compare(_Mirror(a, dur, HOOK_LENS), cpr, words, norm, joins)
        assert 0.25 < lv[1][0] < 0.6 and lv[1][1] == 0.5 / float(lv[1][0])
        assert np.isnan(np.frombuffer(bodies[1][44:], dtype="<f4")).any()
        # an all-zero request, and one of NaNs only: p = 0, g = 1 (normalise) or the gain (ceiling)
        a = base.copy()
        a[2, : 600 * frames[2]] = 0.0
        a[3:, :] = np.nan
        _, lv = _run_and_compare(_Mirror(a, dur, HOOK_LENS), cpr, words, [norm[0], norm[0], (CEILING, 3.0, 0.5)], joins)
        assert lv[1] == (np.float32(0), 1.0) and lv[2] == (np.float32(0), 3.0)


# ---- every mode, form and rate ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouping", sorted(GROUPINGS))
def test_hook_every_mode_in_all_seven_forms_at_all_four_rates(mirror, grouping):
    """Requests of one, two, three and six rows (one to several windows of the peak pass); the grouping of three is joined.  Every
    one of the four specs meets every form at every rate in every grouping."""
    cpr = GROUPINGS[grouping]
    R = len(cpr)
    joins = [(HEAD | TAIL | INNER, 10, 85, 12)] * R if grouping == "two_one_three" else None
    seen = set()
    for code in range(4):
        for form in FORMS:
            for shift in range(0, len(SPECS), min(R, len(SPECS))):
                levels = [SPECS[(r + shift) % len(SPECS)] for r in range(R)]
                _, lv = _run_and_compare(mirror, cpr, [form | code << 8] * R, levels, joins, want=[form % 2 == 0] * R)
                seen.update((code, form, s) for s in levels)
                for (p, g), s in zip(lv, levels):  # the specs do what they are there for
                    assert 0.25 < p < 0.6 and g == (2.5 if s[0] == GAIN else (0.5 / float(p) if s[0] == NORMALIZE else
                                                                              (0.75 / float(p) if s[1] == 8.0 else 1.5)))
    assert len(seen) == 4 * len(FORMS) * len(SPECS)


def test_hook_plain_requests_beside_levelled_ones_give_the_old_hooks_bytes(hook_inputs, mirror):
    """The same rows through the hooks without levels (pack_requests, join_requests) and through the levelled hook: a plain
    request between two levelled ones, in a plain and in a joined batch, equals the old bytes and marks byte for byte; a batch
    whose specs are all plain equals the old hook's bytes as a whole and still reports every p."""
    from kokorox_amd import hip_koko as hk
    a, dur, frames = hook_inputs
    cpr = [2, 1, 3]
    trim = (HEAD | TAIL | INNER, 10, 85, 12)
    for words in ([0x000, 0x108, 0x303], [0x004, 0x003, 0x202], [0x002, 0x309, 0x001]):
        for joins in (None, [trim, NO_JOIN, trim]):
            if joins is None:
                old = hk.pack_requests(a, frames, cpr, words)
                old_marks = hk.token_marks(dur, HOOK_LENS, cpr, words)
            else:
                old, _, old_marks = hk.join_requests(a, dur, HOOK_LENS, cpr, words, joins, want=[True] * 3)
            for levels in ([PLAIN] * 3, [SPECS[1], PLAIN, SPECS[2]], [PLAIN, SPECS[0], PLAIN], [PLAIN, PLAIN, SPECS[1]]):
                bodies, samples, marks, lv = hk.level_requests(a, dur, HOOK_LENS, cpr, words, levels, joins=joins, want=[True] * 3)
                for r in range(3):
                    np.testing.assert_array_equal(marks[r], old_marks[r])
                    if levels[r] == PLAIN:
                        assert bodies[r] == old[r], (words, joins, levels, r)  # (byte for byte)
                        assert lv[r][1] == 1.0
                    else:
                        assert bodies[r] != old[r], (words, joins, levels, r)
                    assert 0.25 < lv[r][0] < 0.6
    # (and against the mirror, marks included)
    _run_and_compare(mirror, cpr, [0x000, 0x108, 0x303], [PLAIN] * 3, [trim, NO_JOIN, trim], want=[True, True, False])


def test_hook_every_row_a_request_of_its_own_and_one_shared_shape(hook_inputs):
    """chunks_per_request = NULL (the per-utterance layout: R = B) goes through the same plan."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    a, _, frames = hook_inputs
    levels = [SPECS[r % 4] for r in range(6)]
    bodies, samples, _, lv = hk.level_requests(a, None, None, None, [2] * 6, levels, frames=frames)
    for r in range(6):
        z = a[r, : 600 * frames[r]]
        _assert_levels(lv[r], z, levels[r], f"row {r}")
        _assert_body(bodies[r], V.stream_body(V.level_stream(z, levels[r]), 2), 2, f"row {r}")


# ---- the model ------------------------------------------------------------------------------------------------------------
def _chunks():
    """The six chunks of tests/test_gpu_token_marks.py: 3..12 tokens with the pads."""
    from oracle import kokoro_ref as R
    return [list(int(v) for v in R.synthetic_inputs(1, k, seed=500 + k)[0]) for k in (1, 10, 3, 5, 2, 7)]


def _raw_of(x):
    return x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()


MODEL_JOIN = (HEAD | TAIL | INNER, 10, 85, 1)


@pytest.mark.parametrize("pattern", [[3, 3, 3, 4], [2, 5, 1, 1, 3, 7, 2], None], ids=["pinned_3_3_3_4", "pinned_of_seven", "unpinned"])
def test_model_levelled_requests_equal_the_mirror_of_its_own_form_0_result(hip_model, pattern):
    """The model's own f32 body at a rate (form 0, same seed, same utterance base, same joins) is the stream z; the levelled body
    in every form at that rate must equal the form mirror of level_stream(z), out_levels must equal level_gain(z), marks and
    sample counts must be those of the call without levels.  Then a shorter batch on the same model: what the longer one left in
    the peak table must not reach it."""
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    toks = _chunks()
    rows = [tab[b % 4, len(t) - 2, 0] for b, t in enumerate(toks)]
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations(pattern)
    cpr = [2, 1, 3]
    try:
        kw = dict(styles=rows, speeds=[1.0], seed=23)
        for code in range(4):
            for joins in (None, MODEL_JOIN):
                if joins is None:
                    z, zmarks, zsamples = hip_model.infer_requests_marks(toks, cpr, fmt=code << 8, with_samples=True, **kw)
                else:
                    z, zmarks, zsamples = hip_model.infer_requests_joined(toks, cpr, joins, fmt=code << 8, marks=True, with_samples=True, **kw)
                for k, form in enumerate(FORMS if joins is None else [4, 8]):
                    word = form | code << 8
                    levels = [SPECS[(r + k) % len(SPECS)] for r in range(3)]
                    bodies, marks, lv, samples = hip_model.infer_requests_levelled(toks, cpr, levels, joins=joins, fmt=word, marks=True,
                                                                                   with_samples=True, **kw)
                    assert samples == zsamples
                    for r in range(3):
                        what = f"pattern {pattern} word {word:#x} joins {joins} request {r} level {levels[r]}"
                        p, g = _assert_levels(lv[r], z[r], levels[r], what)
                        assert p > 0, what
                        _assert_body(_raw_of(bodies[r]), V.stream_body(V.level_stream(z[r], levels[r]), word), word, what)
                        np.testing.assert_array_equal(marks[r], zmarks[r], err_msg=what)
            # the plain spec, shared, without marks: the bytes of the call without levels, and a peak meter
            meter, lv = hip_model.infer_requests_levelled(toks, cpr, PLAIN, fmt=code << 8, **kw)
            z0 = hip_model.infer_requests(toks, cpr, fmt=code << 8, **kw)
            for r in range(3):
                assert _raw_of(meter[r]) == _raw_of(z0[r])
                assert (float(lv[r][0]), float(lv[r][1])) == (float(np.abs(z0[r]).max()), 1.0)
        # two calls in sequence on one model, the longer batch first
        word = 0x102
        long_toks, long_rows = toks + toks, rows + rows
        hip_model.infer_requests_levelled(long_toks, [6, 6], SPECS[1], styles=long_rows, speeds=[1.0], seed=23, fmt=word)
        short = dict(styles=rows[4:], speeds=[1.0], seed=23)
        bodies, lv = hip_model.infer_requests_levelled(toks[4:], [1, 1], SPECS[1], fmt=word, **short)
        z = hip_model.infer_requests(toks[4:], [1, 1], fmt=0x100, **short)
        for r in range(2):
            _assert_levels(lv[r], z[r], SPECS[1], f"short batch request {r}")
            _assert_body(_raw_of(bodies[r]), V.stream_body(V.level_stream(z[r], SPECS[1]), word), word, f"short batch request {r}")
            assert int(np.abs(bodies[r].astype(np.int32)).max()) == int(np.trunc(np.float32(0.5) * np.float32(32767.0)))
    finally:
        hip_model.set_pinned_durations(None)


def test_tts_request_takes_a_level(hip_model):
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    styles = {"v": W.synthetic_voices(1)[0]}
    chunks = [[5, 9, 12], [7, 3]]
    hip_model.set_utterance_base(0)
    plain = V.tts_request(hip_model, styles, "v", chunks, seed=4, fmt=0x200)
    got = V.tts_request(hip_model, styles, "v", chunks, seed=4, fmt=0x200, level=(NORMALIZE, 1.0, 0.25))
    assert got.tobytes() == V.level_stream(plain, (NORMALIZE, 1.0, 0.25)).tobytes() and float(np.abs(got).max()) == 0.25


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _raw_model_call(model, toks, cpr, rows, fmt, joins, levels, n_join=None, n_level=None, out_marks=True, out_n_marks=True, out_levels=True):
    """kx_infer_requests_levelled as C callers make it; returns (rc, out pointer value, message)."""
    from kokorox_amd import hip_koko as hk
    ids, lens = model._ids_lens(toks)
    cp = np.ascontiguousarray(cpr, dtype=np.int32)
    fm = np.ascontiguousarray(fmt, dtype=np.int32).reshape(-1)
    st = np.ascontiguousarray(rows, dtype=np.float32)
    sp = np.ones(1, dtype=np.float32)
    R = cp.shape[0]
    j = None if joins is None else hk.join_specs(joins)
    lv = None if levels is None else np.array([tuple(v) for v in levels], dtype=hk.LEVEL_DTYPE)
    out, mk = C.c_void_p(0xDEAD0), C.c_void_p()
    nb, ns, nm = np.zeros(max(R, 8), np.int64), np.zeros(max(R, 8), np.int64), np.zeros(max(R, 8), np.int64)
    olv = np.zeros((max(R, 8), 2), np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = model._lib.kx_infer_requests_levelled(model._h, p(ids), ids.shape[1], p(lens), len(toks), p(cp), R, p(st), None, None, 0, p(sp), 1,
                                               5, 0, p(fm), fm.shape[0], C.byref(out), p(nb), p(ns),
                                               C.byref(mk) if out_marks else None, p(nm) if out_n_marks else None,
                                               None if j is None else p(j), (0 if j is None else j.shape[0]) if n_join is None else n_join,
                                               None if lv is None else p(lv), (0 if lv is None else lv.shape[0]) if n_level is None else n_level,
                                               p(olv) if out_levels else None)
    if rc == 0:
        model._lib.kx_free_packed(out)
    return rc, out.value, model.last_error() if rc else ""


BAD_LEVELS = [(3, 1.0, 0.0), (1 << 31, 1.0, 0.0), (0, -0.5, 0.0), (0, 65.0, 0.0), (0, float("nan"), 0.0), (2, float("inf"), 0.5),
              (0, 1.0, 0.5), (0, 1.0, -0.0), (0, 1.0, float("nan")), (1, 2.0, 0.5), (1, 1.0, 0.0), (1, 1.0, 2.0 ** -16), (1, 1.0, 1.0000001),
              (1, 1.0, float("nan")), (2, 1.0, 0.0), (2, 1.0, 2.0), (2, float("nan"), 0.5), (2, 1.0, -0.5)]


def test_refusals(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    toks = _chunks()[:3]
    rows = [W.synthetic_voices(1)[0, len(t) - 2, 0] for t in toks]
    ok, okj = (NORMALIZE, 1.0, 0.5), (HEAD | INNER, 10, 85, 1)
    hip_model.set_pinned_durations([1])
    try:
        call = lambda *a, **k: _raw_model_call(hip_model, toks, [1, 2], rows, *a, **k)  # noqa: E731
        assert call(0, None, [ok])[0] == hk.KX_OK                                                   # no joins, a shared spec
        assert call(0, [okj], [ok, PLAIN])[0] == hk.KX_OK                                           # joins, a spec per request
        assert call(0, None, [ok], out_marks=False, out_n_marks=False, out_levels=False)[0] == hk.KX_OK  # neither marks nor out_levels
        for edge in ((0, 0.0, 0.0), (0, 64.0, 0.0), (1, 1.0, 1.0), (1, 1.0, 2.0 ** -15), (2, 0.0, 2.0 ** -15), (2, 64.0, 1.0)):
            assert call(0, None, [edge])[0] == hk.KX_OK, edge
        rc, out, msg = call(0, None, None, n_level=1)
        assert (rc, msg) == (hk.KX_ERR_INVALID, "infer: null level argument") and not out
        for levels, n_level in (([ok], 0), ([ok, ok, ok], 3), ([ok, ok, ok], -1)):
            rc, out, msg = call(0, None, levels, n_level=n_level)
            assert (rc, msg) == (hk.KX_ERR_INVALID, "infer: bad level count") and not out, n_level
        for bad in BAD_LEVELS:
            for levels in ([bad], [ok, bad]):
                rc, out, msg = call(0, None, levels)
                assert (rc, msg) == (hk.KX_ERR_INVALID, "infer: bad level") and not out, levels
        # everything kx_infer_requests_joined refuses comes first, with its text
        for kw in (dict(out_marks=False), dict(out_n_marks=False)):
            rc, out, msg = call(0, None, None, **kw)
            assert (rc, msg) == (hk.KX_ERR_INVALID, "infer: null marks argument") and not out, kw
        rc, out, msg = call(0, None, None, n_join=1)
        assert (rc, msg) == (hk.KX_ERR_INVALID, "infer: null join argument") and not out
        rc, out, msg = call(0, [okj, okj, okj], None, n_join=3)
        assert (rc, msg) == (hk.KX_ERR_INVALID, "infer: bad join count") and not out
        rc, out, msg = call(0, [(8, 0, 0, 0)], [BAD_LEVELS[0]])
        assert (rc, msg) == (hk.KX_ERR_INVALID, "infer: bad join") and not out
        chunks_text = "infer: chunks_per_request entries must be >= 1 and add up to the batch"
        for cpr, fmt, text in (([1, 2], 5, "infer: unknown output format"), ([1, 2], 0x400, "infer: unknown output sample rate"),
                               ([1, 0, 2], 0, chunks_text), ([2, 2], 0, chunks_text),
                               ([1, 2], [0, 1, 2], "infer: requests need 1 or R output formats")):
            rc, out, msg = _raw_model_call(hip_model, toks, cpr, rows, fmt, None, [BAD_LEVELS[0]])
            assert (rc, msg) == (hk.KX_ERR_INVALID, text) and not out, (cpr, fmt)
            with pytest.raises(hk.KokoroxHipError) as e:
                hip_model.infer_requests_levelled(toks, cpr, ok, styles=rows, fmt=fmt)
            assert e.value.code == hk.KX_ERR_INVALID and str(e.value).endswith(text), (cpr, fmt)
        # the dispatcher's entry
        d = hk.Dispatcher([hip_model], max_batch=4, max_wait_us=0)
        try:
            a = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int64) for t in toks]))
            ln = np.array([len(t) for t in toks], dtype=np.int32)
            st = np.ascontiguousarray(rows, dtype=np.float32)
            p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731

            def raw(level, join=None, fmt=0, marks=True, n_marks=True, want_out=True):
                out, mk, nb, ns, nm = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
                err = C.create_string_buffer(256)
                olv = np.zeros(2, np.float64)
                j = None if join is None else hk.join_specs([join])
                lv = None if level is None else np.array([tuple(level)], dtype=hk.LEVEL_DTYPE)
                rc = d._lib.kx_dispatcher_submit_request_levelled(d._d, p(a), p(ln), 3, p(st), None, None, 0, 1.0, 5, fmt, C.byref(out),
                                                                  C.byref(nb), C.byref(ns), C.byref(mk) if marks else None,
                                                                  C.byref(nm) if n_marks else None, None if j is None else p(j),
                                                                  None if lv is None else p(lv), p(olv) if want_out else None, err, len(err))
                if rc == 0:
                    d._lib.kx_free_packed(out)
                return rc, out.value, err.value.decode()

            assert raw(ok)[0] == hk.KX_OK and raw(ok, join=okj, marks=False, n_marks=False)[0] == hk.KX_OK
            assert raw(PLAIN, want_out=False)[0] == hk.KX_OK
            for bad in [None] + BAD_LEVELS:
                rc, out, msg = raw(bad)
                assert (rc, msg) == (hk.KX_ERR_INVALID, "dispatcher_submit_request: bad level") and not out, bad
            rc, out, msg = raw(ok, join=(8, 0, 0, 0))
            assert (rc, msg) == (hk.KX_ERR_INVALID, "dispatcher_submit_request: bad join") and not out
            for kw in (dict(marks=False), dict(n_marks=False)):
                rc, out, msg = raw(ok, **kw)
                assert (rc, msg) == (hk.KX_ERR_INVALID, "dispatcher_submit_request: null marks argument") and not out
            rc, out, msg = raw(ok, fmt=5)
            assert rc == hk.KX_ERR_INVALID and not out and "format" in msg
        finally:
            d.close()
    finally:
        hip_model.set_pinned_durations(None)


# ---- dispatcher ------------------------------------------------------------------------------------------------------------
def _request_specs():
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    tab = W.synthetic_voices(4)
    words = [0, 0x108, 0x303, 4, 0x202, 0x109, 3, 0x301]
    joins = [(HEAD | TAIL | INNER, 20, 150, 5), None, (INNER, 0, 85, 12), None, NO_JOIN]
    levels = [SPECS[1], None, SPECS[2], PLAIN, None, SPECS[0], SPECS[3]]
    specs = []
    for i in range(16):
        n = 1 + i % 3
        chunks = [list(int(v) for v in R.synthetic_inputs(1, 1 + (5 * i + 3 * c) % 10, seed=900 + 10 * i + c)[0]) for c in range(n)]
        kind = i % 3
        if kind == 0:
            voice = dict(styles=[tab[i % 4, len(c) - 2, 0] for c in chunks])
        elif kind == 1:
            voice = dict(voices=i % 4)
        else:
            voice = dict(voices=[(i % 4, 4.0), ((i + 1) % 4, 5.0)])
        # levelled, joined and plain (None: submitted through the older entries), with and without marks, mixed in every batch
        specs.append(dict(chunks=chunks, voice=voice, fmt=words[i % len(words)], seed=9500 + i, speed=1.0 + 0.125 * (i % 2),
                          marks=(i // 3) % 2 == 0, join=joins[i % len(joins)], level=levels[i % len(levels)]))
    return tab, specs


def _alone(model, s):
    """The request through the direct call with R = 1: (body, marks or None, levels or None)."""
    n = len(s["chunks"])
    v = s["voice"]
    if "styles" in v:
        kw = dict(styles=v["styles"])
    elif isinstance(v["voices"], int):
        kw = dict(voice_ids=[[v["voices"]]] * n, weights=[[0.0]] * n)
    else:
        kw = dict(voice_ids=[[a for a, _ in v["voices"]]] * n, weights=[[w for _, w in v["voices"]]] * n)
    kw.update(speeds=[s["speed"]], seed=s["seed"], fmt=s["fmt"])
    if s["level"] is not None:
        res = model.infer_requests_levelled(s["chunks"], [n], s["level"], joins=s["join"], marks=s["marks"], **kw)
        return (res[0][0], res[1][0], res[2][0]) if s["marks"] else (res[0][0], None, res[1][0])
    join = s["join"] if s["join"] is not None else NO_JOIN
    if s["marks"]:
        bodies, marks = model.infer_requests_joined(s["chunks"], [n], join, marks=True, **kw)
        return bodies[0], marks[0], None
    return model.infer_requests_joined(s["chunks"], [n], join, **kw)[0], None, None


def _same(got, want):
    if isinstance(want, bytes):
        assert isinstance(got, bytes) and got == want
    else:
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _dispatcher_scenario(model):
    """8 client threads, 16 requests of 1..3 chunks: levelled (with and without a join), joined and plain, with and without marks,
    rates and forms mixed, voices by row / id / mix; body, marks and levels of each equal the direct call of the request alone
    (R = 1, its seed, utterance base 0)."""
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
                                          level=s["level"], **s["voice"])
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
    changed = 0
    for i, s in enumerate(specs):
        body, marks, lv = _alone(model, s)
        got = out[i] if isinstance(out[i], tuple) else (out[i],)
        assert len(got) == 1 + int(s["marks"]) + int(s["level"] is not None), i
        _same(got[0], body)
        if s["marks"]:
            np.testing.assert_array_equal(got[1], marks)
        if s["level"] is not None:
            assert got[-1].tolist() == lv.tolist() and lv[0] > 0, i
            if s["level"] != PLAIN:  # (a levelled request is not its plain self: the spec reached the batch)
                changed += _raw_of(_alone(model, dict(s, level=None, marks=False))[0]) != _raw_of(body)
    assert changed >= 6
    assert st["requests"] == len(specs) and st["batches"] < st["requests"]
    return st


def test_dispatcher_levelled_requests_equal_their_solo_runs(hip_model):
    _dispatcher_scenario(hip_model)


def test_dispatcher_copy_out_path_in_a_fresh_process():
    """KX_PINNED_LIVE_CAP_MB is read once per process: with 0 every request's body and marks are copied out into plain
    allocations; the levels travel beside them."""
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
