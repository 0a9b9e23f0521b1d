"""GPU: joins (include/kokorox_hip.h, "joins") -- the joined form of the packer, the resampler and the marks kernel through
their test hook, through kx_infer_requests_joined and through the dispatcher.  Cuts are made at pad spans, which are known
integers, so every check is an EQUALITY against the numpy definition of kokorox_amd/voices.py (join_stream, joined_marks, then
the existing resample_stream and form mirrors).  The only latitude is the one tests/test_gpu_resample.py takes: in the float
forms a NaN must be a NaN where the mirror has one, its sign and payload are not compared."""
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
LM = {0: (1, 1), 1: (1, 3), 2: (2, 3), 3: (2, 1)}
FORMS = [0, 8, 3, 1, 4, 9, 2]
HEAD, TAIL, INNER = 1, 2, 4
PLAIN = (0, 0, 0, 0)
PAUSES, KEEPS, FADES = (0, 1, 85, 200), (0, 10, 30, 1000), (0, 1, 12)
PACK_WINDOW_BYTES, RS_WINDOW = 4096, 1024  # kernels_misc.hip: PACK_THREADS x 16 bytes, RS_WINDOW outputs per workgroup


def _firsts(cpr):
    return np.concatenate([[0], np.cumsum(cpr)]).astype(int)


# ---- the hook's inputs: six rows that reach every seam ----------------------------------------------------------------------
HOOK_LENS = [3, 5, 1, 4, 2, 3]


def _hook_inputs():
    """Durations 1..4 frames per token (rows of 600 to about 7000 samples), a slab whose rows are longer than the longest row
    and poisoned at and past 600 x frames[b], distinct valid samples, and a NaN, a +inf and a -inf where they end up kept, cut
    or inside a fade depending on the spec."""
    rng = np.random.default_rng(20262)
    dur = np.empty((6, 512), dtype=np.int32)
    dur[:, 0::2] = 2 ** 31 - 1  # what lies at or beyond lens[b] must not reach any result
    dur[:, 1::2] = -7
    for b, n in enumerate(HOOK_LENS):
        dur[b, :n] = rng.integers(1, 5, size=n)
    frames = [int(dur[b, :n].sum()) for b, n in enumerate(HOOK_LENS)]
    ld = 600 * max(frames) + 777
    poison = np.array([np.nan, np.inf, 1e30, -np.inf, -1e30], dtype=np.float32)
    a = np.empty((6, ld), dtype=np.float32)
    total = 600 * sum(frames)
    values = (-1.3 + 2.6 * (rng.permutation(total) + 0.5) / total).astype(np.float32)  # every valid sample of the slab is its own value
    assert np.unique(values).shape[0] == total
    o = 0
    for b, f in enumerate(frames):
        n = 600 * f
        a[b, :n] = values[o: o + n]
        a[b, n:] = poison[(np.arange(ld - n) + b) % len(poison)]
        o += n
    lead0, tail1 = 600 * int(dur[0, 0]), 600 * (frames[1] - int(dur[1, 4]))
    a[0, lead0 + 5] = np.nan      # kept under every spec; with keep 0 sample 5 of row 0's kept segment, inside its head fade
    a[0, lead0 + 3] = np.inf
    a[1, tail1 - 2] = -np.inf     # kept under every spec; with keep 0 the last but one kept sample of row 1, inside its tail fade
    a[3, 600 * int(dur[3, 0]) + 300] = np.nan  # the middle of row 3's second token: kept, never faded
    a[0, 7] = np.nan              # inside row 0's lead span: cut when its head is trimmed with keep 0 or 10, kept otherwise
    return a, dur, frames


@pytest.fixture(scope="module")
def hook_inputs():
    return _hook_inputs()


class _Mirror:
    """The numpy definition, request by request, with the resampled streams computed once per (rows, spec, rate)."""

    def __init__(self, audio, dur, lens):
        self.audio, self.dur, self.lens, self.cache = audio, dur, lens, {}

    def durations(self, b0, b1):
        return [[int(v) for v in self.dur[b, : self.lens[b]]] for b in range(b0, b1)]

    def stream(self, b0, b1, join, rate):
        from kokorox_amd import voices as V
        key = (b0, b1, tuple(join), rate)
        if key not in self.cache:
            d = self.durations(b0, b1)
            x = V.join_stream([self.audio[b, : 600 * sum(d[b - b0])] for b in range(b0, b1)], d, join)
            self.cache[key] = V.resample_stream(x, rate)
        return self.cache[key]

    def request(self, b0, b1, word, join):
        """(body bytes, out_samples, marks) of the request of rows b0 .. b1 - 1."""
        from kokorox_amd import voices as V
        y = self.stream(b0, b1, join, word & 0xF00)
        return V.stream_body(y, word), y.shape[0], V.joined_marks(self.durations(b0, b1), word, join)


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


def _run_and_compare(mirror, cpr, words, joins, want=None):
    from kokorox_amd import hip_koko as hk
    R = len(cpr)
    joins = [tuple(j) for j in (joins if len(joins) == R and not isinstance(joins[0], int) else [joins] * R)]
    bodies, samples, marks = hk.join_requests(mirror.audio, mirror.dur, mirror.lens, cpr, words, joins, want=want)
    first = _firsts(cpr)
    for r in range(R):
        body, n, m = mirror.request(first[r], first[r + 1], words[r], joins[r])
        what = f"grouping {cpr} request {r} word {words[r]:#x} join {joins[r]}"
        assert samples[r] == n, what
        _assert_body(bodies[r], body, words[r], what)
        if want is None or not want[r]:
            assert marks[r].shape[0] == 0, what
        else:
            np.testing.assert_array_equal(marks[r], m, err_msg=what)
            assert int(marks[r][-1]) == samples[r] and (np.diff(marks[r]) >= 0).all(), what
    return bodies, samples, marks


def _words(R, shift):
    """Mixed forms and rates over the requests of a batch, rotated by `shift`."""
    cycle = [0x000, 0x108, 0x303, 0x204, 0x002, 0x109, 0x301, 0x200, 0x003, 0x104, 0x308, 0x201]
    return [cycle[(r + shift) % len(cycle)] for r in range(R)]


def _spec_cases():
    """Every (grouping, words, specs) the spec test runs: pause x keep x fade with all three flags, words rotating."""
    cases, k = [], 0
    for g in sorted(GROUPINGS):
        for pause in PAUSES:
            for keep in KEEPS:
                for fade in FADES:
                    cases.append((g, pause, _words(len(GROUPINGS[g]), k), (HEAD | TAIL | INNER, keep, pause, fade)))
                    k += 1
    return cases


@pytest.fixture(scope="module")
def mirror(hook_inputs):
    a, dur, _ = hook_inputs
    return _Mirror(a, dur, HOOK_LENS)


@pytest.mark.parametrize("pause", PAUSES)
@pytest.mark.parametrize("grouping", sorted(GROUPINGS))
def test_hook_every_pause_keep_and_fade_equals_the_mirror(mirror, grouping, pause):
    """24 samples of pause are shorter than any unit, 2040 cross a packer window of 1024 / 2048 / 4096 samples, 4800 are longer
    than every packer window and than the resampler's input window; keep 30 ms is longer than a one-frame pad, keep 1000 ms than
    every pad; bodies, sample counts and marks of every request."""
    n = 0
    for g, p, words, join in _spec_cases():
        if g == grouping and p == pause:
            _run_and_compare(mirror, GROUPINGS[g], words, join, want=[True] * len(words))
            n += 1
    assert n == len(KEEPS) * len(FADES)


def test_hook_every_subset_of_the_flags(mirror):
    cpr = GROUPINGS["two_one_three"]
    seen = set()
    for flags in range(8):
        bodies, samples, _ = _run_and_compare(mirror, cpr, [0x000, 0x108, 0x303], (flags, 10, 85, 1), want=[True, False, True])
        seen.add(tuple(samples))
    # HEAD, TAIL and INNER each change some request's length on these rows (the single-row request has no inner boundary)
    assert len(seen) == 8


def test_hook_all_seven_forms_at_all_four_rates(mirror):
    cpr = GROUPINGS["two_one_three"]
    for code in LM:
        for form in FORMS:
            _run_and_compare(mirror, cpr, [form | code << 8] * 3, (HEAD | TAIL | INNER, 10, 85, 12), want=[form % 2 == 0] * 3)


def test_hook_mixed_words_specs_and_want_flags_in_one_batch(mirror):
    """A plain (all-zero) request between two joined ones, and a batch of six single-row requests each with its own spec."""
    _run_and_compare(mirror, [2, 1, 3], [0x303, 0x000, 0x108], [(HEAD | INNER, 10, 85, 1), PLAIN, (TAIL | INNER, 0, 200, 12)],
                     want=[True, True, False])
    _run_and_compare(mirror, [2, 3, 1], [0x004, 0x202, 0x009], [(INNER, 30, 1, 12), PLAIN, (HEAD | TAIL, 0, 0, 1)], want=[False, True, True])
    specs = [(HEAD, 0, 0, 12), PLAIN, (HEAD | TAIL, 1000, 5000, 1), (TAIL, 10, 85, 0), (HEAD | TAIL | INNER, 0, 200, 12), (HEAD, 30, 0, 1)]
    for shift in (0, 5):
        _run_and_compare(mirror, [1] * 6, _words(6, shift), specs, want=[r % 2 == 0 for r in range(6)])
    _run_and_compare(mirror, [6], [0x108], [(HEAD | TAIL | INNER, 0, 200, 12)], want=[True])


def test_some_case_puts_a_fade_and_a_gap_across_a_window_boundary(hook_inputs):
    """Computed from the layout of the cases test_hook_every_pause_keep_and_fade_equals_the_mirror runs, not assumed: a fade that
    straddles the boundary between two packer workgroups (4096 output bytes each, counted from the 16-byte unit the region
    starts in), a pause that holds the boundary between the inputs of two resampler workgroups (1024 outputs each), and a
    resampler workgroup whose whole input window lies inside a pause: it stages only zeros."""
    from kokorox_amd import voices as V
    _, dur, _ = hook_inputs
    fade_across = gap_across = only_zeros = 0
    for g, pause, words, join in _spec_cases():
        cpr = GROUPINGS[g]
        first, off = _firsts(cpr), 0
        for r in range(len(cpr)):
            d = [[int(v) for v in dur[b, : HOOK_LENS[b]]] for b in range(first[r], first[r + 1])]
            rows = V.join_rows(d, join)
            S = sum(k + gap for _, k, gap, _, _ in rows)
            code, form = words[r] >> 8, words[r] & 0xFF
            L, M = LM[code]
            n_out = S * L // M
            nbytes = {0: 4 * n_out, 1: 8 * n_out, 2: 2 * n_out, 3: 44 + 4 * n_out, 4: 4 * ((44 + 2 * n_out + 2) // 3), 8: n_out, 9: n_out}[form]
            P = 0
            for skip, keep, gap, fh, ft in rows:
                if code == 0 and form != 4:  # sample s of the stream is bytes h + w s .. h + w (s + 1) - 1 of the region
                    h, w = {0: (0, 4), 1: (0, 8), 2: (0, 2), 3: (44, 4), 8: (0, 1), 9: (0, 1)}[form]
                    for f0, f1 in ((P, P + fh), (P + keep - ft, P + keep)):
                        lo_b, hi_b = h + w * f0 + (off & 15), h + w * f1 + (off & 15)  # counted from the region's first unit
                        fade_across += f1 > f0 and (hi_b - 1) // PACK_WINDOW_BYTES > lo_b // PACK_WINDOW_BYTES
                if code and gap:
                    C_, lo, hi = (48 if code == 3 else 72), P + keep, P + keep + gap
                    for n0 in range(0, n_out, RS_WINDOW):
                        n1 = min(n0 + RS_WINDOW, n_out)
                        j_lo, j_hi = max(0, -((C_ - n0 * M) // L)), min(((n1 - 1) * M + C_) // L + 1, S)
                        gap_across += n0 > 0 and lo < j_lo < hi  # this workgroup's first input lies inside the pause
                        only_zeros += lo <= j_lo and j_hi <= hi
                P += keep + gap
            off += nbytes
    print("fades across a packer window:", fade_across, "pauses across a resampler window:", gap_across,
          "resampler workgroups that stage only zeros:", only_zeros)
    assert fade_across > 0 and gap_across > 0 and only_zeros > 0


# ---- the plain path inside a joined batch ------------------------------------------------------------------------------------
def test_plain_requests_give_the_old_hooks_bytes_and_marks_beside_a_joined_one(hook_inputs):
    """The same rows through pack_requests / token_marks and through the new hook: with all-zero specs (the plain kernels), and
    as plain requests in a batch whose other request is joined (the joined kernels with skip = gap = 0), before and behind it."""
    from kokorox_amd import hip_koko as hk
    a, dur, frames = hook_inputs
    cpr = [2, 1, 3]
    for words in ([0x000, 0x108, 0x303], [0x004, 0x003, 0x202], [0x002, 0x309, 0x001]):
        old_bodies = hk.pack_requests(a, frames, cpr, words)
        old_marks = hk.token_marks(dur, HOOK_LENS, cpr, words)
        for specs in ([PLAIN] * 3, [PLAIN, PLAIN, (HEAD | TAIL | INNER, 10, 85, 12)], [(HEAD | TAIL | INNER, 0, 200, 1), PLAIN, PLAIN],
                      [PLAIN, (HEAD | TAIL, 10, 0, 1), PLAIN]):
            bodies, samples, marks = hk.join_requests(a, dur, HOOK_LENS, cpr, words, specs, want=[True] * 3)
            for r in range(3):
                if specs[r] == PLAIN:
                    assert bodies[r] == old_bodies[r], (words, specs, r)  # (byte for byte, NaN payloads included)
                    np.testing.assert_array_equal(marks[r], old_marks[r])
                    assert samples[r] == int(old_marks[r][-1])
                elif r != 1:  # (request 1 is the one-token row, which no spec trims, alone: nothing to pause either)
                    assert bodies[r] != old_bodies[r]
                else:
                    assert bodies[r] == old_bodies[r]


def test_hook_64_bit_arithmetic():
    """Two rows of 512 tokens of 4096 frames each at 48 kHz, marks only, HEAD | TAIL and 5000 ms of pause: the last mark is
    above 2^32."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    dur = np.full((2, 512), 4096, dtype=np.int32)
    join = (HEAD | TAIL, 0, 5000, 12)
    _, samples, (got,) = hk.join_requests(None, dur, [512, 512], [2], [hk.PACK_RATE_48000], [join], want=[True])
    want = V.joined_marks([[4096] * 512] * 2, hk.PACK_RATE_48000, join)
    np.testing.assert_array_equal(got, want)
    # two pads of 4096 frames cut away, 120 000 samples of pause put in, all of it doubled
    assert int(got[-1]) == samples[0] == 2 * (2 * 512 * 4096 * 600 - 2 * 4096 * 600 + 120000) and got[-1] > 2 ** 32
    assert got[0] == got[1] == 0 and got[-1] == got[-2] and int(got[513] - got[512]) == 240000


# ---- the model ------------------------------------------------------------------------------------------------------------
def _chunks():
    """The six chunks of tests/test_gpu_token_marks.py: 3..12 tokens with the pads."""
    from oracle import kokoro_ref as R
    return [list(int(v) for v in R.synthetic_inputs(1, k, seed=500 + k)[0]) for k in (1, 10, 3, 5, 2, 7)]


def _decoded(raw, word):
    form = word & 0xFF
    if form in (3, 4):
        return raw
    dt = {0: np.float32, 1: np.float32, 2: np.int16, 8: np.uint8, 9: np.uint8}[form]
    a = np.frombuffer(raw, dtype=dt)
    return a.reshape(-1, 2) if form == 1 else a


def _raw_of(x):
    return x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()


MODEL_WORDS = [4, 0x108, 0x303, 0x200]
MODEL_SPECS = [(HEAD | TAIL | INNER, 10, 85, 1), (HEAD | INNER, 0, 200, 12), (TAIL, 30, 1, 0), PLAIN, (INNER, 1000, 0, 12),
               (HEAD | TAIL, 0, 0, 1)]


@pytest.mark.parametrize("pattern", [[3, 3, 3, 4], [2, 5, 1, 1, 3, 7, 2], None], ids=["pinned_3_3_3_4", "pinned_of_seven", "unpinned"])
def test_model_joined_requests_equal_the_mirror_of_the_plain_result(hip_model, pattern):
    """The plain f32 24 kHz bodies and marks of infer_requests_marks give every chunk's samples and the durations the forward
    used; the mirrors turn them into the joined bodies and marks of four words, which infer_requests_joined (same seed, same
    utterance base) must equal; the all-zero spec must give the plain bytes; kx_call_times keeps its four milestones."""
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    toks = _chunks()
    lens = [len(t) for t in toks]
    rows = [tab[b % 4, len(t) - 2, 0] for b, t in enumerate(toks)]
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations(pattern)
    try:
        kw = dict(styles=rows, speeds=[1.0], seed=21)
        for cpr in GROUPINGS.values():
            R = len(cpr)
            first = _firsts(cpr)
            plain, pmarks = hip_model.infer_requests_marks(toks, cpr, fmt=0, **kw)
            # every chunk's durations and samples, recovered from the plain result
            dur = np.zeros((6, 512), dtype=np.int32)
            audio_rows = []
            for r in range(R):
                o = 0
                for b in range(first[r], first[r + 1]):
                    m = pmarks[r][o: o + lens[b] + 1]
                    d = np.diff(m) // 600
                    assert (np.diff(m) % 600 == 0).all() and (d >= 1).all()
                    if pattern:
                        assert d.tolist() == [pattern[t % len(pattern)] for t in range(lens[b])]
                    dur[b, : lens[b]] = d
                    audio_rows.append(plain[r][int(m[0]): int(m[-1])])
                    o += lens[b] + 1
            ld = max(x.shape[0] for x in audio_rows)
            audio = np.zeros((6, ld), dtype=np.float32)
            for b, x in enumerate(audio_rows):
                audio[b, : x.shape[0]] = x
            mirror = _Mirror(audio, dur, lens)
            for k, word in enumerate(MODEL_WORDS):
                specs = [MODEL_SPECS[(r + k) % len(MODEL_SPECS)] for r in range(R)]
                bodies, marks, samples = hip_model.infer_requests_joined(toks, cpr, specs, fmt=word, marks=True, with_samples=True, **kw)
                t = hip_model.call_times()
                assert len(t) == 4 and 0 < t[0] <= t[1] <= t[2] <= t[3]
                for r in range(R):
                    body, n, m = mirror.request(first[r], first[r + 1], word, specs[r])
                    what = f"pattern {pattern} grouping {cpr} request {r} word {word:#x} join {specs[r]}"
                    assert samples[r] == n, what
                    _assert_body(_raw_of(bodies[r]), body, word, what)
                    np.testing.assert_array_equal(marks[r], m, err_msg=what)
            # one shared spec, no marks; and the all-zero spec: the plain bytes and marks
            shared = hip_model.infer_requests_joined(toks, cpr, (HEAD | TAIL | INNER, 10, 85, 1), fmt=0x108, **kw)
            for r in range(R):
                _assert_body(_raw_of(shared[r]), mirror.request(first[r], first[r + 1], 0x108, (HEAD | TAIL | INNER, 10, 85, 1))[0], 0x108, "shared")
            zero, zmarks = hip_model.infer_requests_joined(toks, cpr, PLAIN, fmt=0, marks=True, **kw)
            for r in range(R):
                assert _raw_of(zero[r]) == _raw_of(plain[r])
                np.testing.assert_array_equal(zmarks[r], pmarks[r])
    finally:
        hip_model.set_pinned_durations(None)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _raw_model_call(model, toks, cpr, rows, fmt, joins, n_join=None, out_marks=True, out_n_marks=True):
    """kx_infer_requests_joined as C callers make it; returns (rc, out pointer value, message)."""
    from kokorox_amd import hip_koko as hk
    ids, lens = model._ids_lens(toks)
    cp = np.ascontiguousarray(cpr, dtype=np.int32)
    fm = np.ascontiguousarray(fmt, dtype=np.int32).reshape(-1)
    st = np.ascontiguousarray(rows, dtype=np.float32)
    sp = np.ones(1, dtype=np.float32)
    R = cp.shape[0]
    j = None if joins is None else hk.join_specs(joins)
    out, mk = C.c_void_p(0xDEAD0), C.c_void_p()
    nb, ns, nm = np.zeros(max(R, 8), np.int64), np.zeros(max(R, 8), np.int64), np.zeros(max(R, 8), np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = model._lib.kx_infer_requests_joined(model._h, p(ids), ids.shape[1], p(lens), len(toks), p(cp), R, p(st), None, None, 0, p(sp), 1,
                                             5, 0, p(fm), fm.shape[0], C.byref(out), p(nb), p(ns),
                                             C.byref(mk) if out_marks else None, p(nm) if out_n_marks else None,
                                             None if j is None else p(j), (0 if j is None else j.shape[0]) if n_join is None else n_join)
    if rc == 0:
        model._lib.kx_free_packed(out)
    return rc, out.value, model.last_error() if rc else ""


def test_refusals(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    toks = _chunks()[:3]
    rows = [W.synthetic_voices(1)[0, len(t) - 2, 0] for t in toks]
    ok = (HEAD | INNER, 10, 85, 1)
    hip_model.set_pinned_durations([1])
    try:
        assert _raw_model_call(hip_model, toks, [1, 2], rows, 0, [ok])[0] == hk.KX_OK
        assert _raw_model_call(hip_model, toks, [1, 2], rows, 0, [ok, PLAIN])[0] == hk.KX_OK
        assert _raw_model_call(hip_model, toks, [1, 2], rows, 0, [ok], out_marks=False, out_n_marks=False)[0] == hk.KX_OK  # no marks
        for kw in (dict(out_marks=False), dict(out_n_marks=False)):
            rc, out, msg = _raw_model_call(hip_model, toks, [1, 2], rows, 0, [ok], **kw)
            assert (rc, msg) == (hk.KX_ERR_INVALID, "infer: null marks argument") and not out, kw
        rc, out, msg = _raw_model_call(hip_model, toks, [1, 2], rows, 0, None, n_join=1)
        assert (rc, msg) == (hk.KX_ERR_INVALID, "infer: null join argument") and not out
        for joins, n_join in (([ok], 0), ([ok, ok, ok], 3), ([ok, ok, ok], -1)):
            rc, out, msg = _raw_model_call(hip_model, toks, [1, 2], rows, 0, joins, n_join=n_join)
            assert (rc, msg) == (hk.KX_ERR_INVALID, "infer: bad join count") and not out, n_join
        for bad in ((8, 0, 0, 0), (1 << 31, 0, 0, 0), (1, -1, 0, 0), (1, 1001, 0, 0), (0, 0, -1, 0), (0, 0, 5001, 0), (1, 0, 0, -1), (1, 0, 0, 13)):
            for joins in ([bad], [ok, bad]):
                rc, out, msg = _raw_model_call(hip_model, toks, [1, 2], rows, 0, joins)
                assert (rc, msg) == (hk.KX_ERR_INVALID, "infer: bad join") and not out, joins
        # everything kx_infer_requests refuses, with its text, and *out stays null
        chunks_text = "infer: chunks_per_request entries must be >= 1 and add up to the batch"
        for cpr, fmt, text in (([1, 2], 5, "infer: unknown output format"), ([1, 2], [0, 5], "infer: unknown output format"),
                               ([1, 2], -1, "infer: unknown output format"), ([1, 2], 0x400, "infer: unknown output sample rate"),
                               ([1, 2], 0x1000, "infer: unknown output format"),
                               ([1, 0, 2], 0, chunks_text), ([1, 1], 0, chunks_text), ([2, 2], 0, chunks_text), ([3, 1], 0, chunks_text),
                               ([1, 2], [0, 1, 2], "infer: requests need 1 or R output formats")):
            rc, out, msg = _raw_model_call(hip_model, toks, cpr, rows, fmt, [ok])
            assert (rc, msg) == (hk.KX_ERR_INVALID, text) and not out, (cpr, fmt)
            with pytest.raises(hk.KokoroxHipError) as e:
                hip_model.infer_requests_joined(toks, cpr, ok, styles=rows, fmt=fmt)
            assert e.value.code == hk.KX_ERR_INVALID and str(e.value).endswith(text), (cpr, fmt)
        # the dispatcher's entry
        d = hk.Dispatcher([hip_model], max_batch=4, max_wait_us=0)
        try:
            a = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int64) for t in toks]))
            ln = np.array([len(t) for t in toks], dtype=np.int32)
            st = np.ascontiguousarray(rows, dtype=np.float32)
            p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731

            def raw(join, fmt=0, n_chunks=3, marks=True, n_marks=True):
                out, mk, nb, ns, nm = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
                err = C.create_string_buffer(256)
                j = None if join is None else hk.join_specs([join])
                rc = d._lib.kx_dispatcher_submit_request_joined(d._d, p(a), p(ln), n_chunks, p(st), None, None, 0, 1.0, 5, fmt, C.byref(out),
                                                                C.byref(nb), C.byref(ns), C.byref(mk) if marks else None,
                                                                C.byref(nm) if n_marks else None, None if j is None else p(j), err, len(err))
                if rc == 0:
                    d._lib.kx_free_packed(out)
                return rc, out.value, err.value.decode()

            assert raw(ok)[0] == hk.KX_OK and raw(ok, marks=False, n_marks=False)[0] == hk.KX_OK and raw(PLAIN)[0] == hk.KX_OK
            for kw in (dict(marks=False), dict(n_marks=False)):
                rc, out, msg = raw(ok, **kw)
                assert (rc, msg) == (hk.KX_ERR_INVALID, "dispatcher_submit_request: null marks argument") and not out
            for bad in (None, (8, 0, 0, 0), (1 << 31, 0, 0, 0), (1, -1, 0, 0), (1, 1001, 0, 0), (0, 0, -1, 0), (0, 0, 5001, 0), (1, 0, 0, -1),
                        (1, 0, 0, 13)):
                rc, out, msg = raw(bad)
                assert (rc, msg) == (hk.KX_ERR_INVALID, "dispatcher_submit_request: bad join") and not out, bad
            for fmt, n_chunks in ((5, 3), (0x400, 3), (0x1000, 3), (0, 5), (0, 0)):  # ... and what submit_request refuses, with its texts
                rc, out, msg = raw(ok, fmt=fmt, n_chunks=n_chunks)
                with pytest.raises(hk.KokoroxHipError) as e:
                    d.submit_request(toks[:n_chunks] if n_chunks <= 3 else toks + toks[:2], styles=(rows + rows[:2])[: max(n_chunks, 0)], fmt=fmt)
                assert rc == hk.KX_ERR_INVALID and not out and str(e.value).endswith(msg) and msg, (fmt, n_chunks)
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
    joins = [(HEAD | TAIL | INNER, 20, 150, 5), None, (INNER, 0, 85, 12), (HEAD, 10, 0, 1), None, (TAIL | INNER, 30, 200, 0), PLAIN]
    specs = []
    for i in range(16):
        n = 1 + i % 3
        chunks = [list(int(v) for v in R.synthetic_inputs(1, 1 + (5 * i + 3 * c) % 10, seed=800 + 10 * i + c)[0]) for c in range(n)]
        kind = i % 3
        if kind == 0:
            voice = dict(styles=[tab[i % 4, len(c) - 2, 0] for c in chunks])
        elif kind == 1:
            voice = dict(voices=i % 4)
        else:
            voice = dict(voices=[(i % 4, 4.0), ((i + 1) % 4, 5.0)])
        # joined and plain (None: submitted without a spec), with and without marks, at every chunk count, mixed in every batch
        specs.append(dict(chunks=chunks, voice=voice, fmt=words[i % len(words)], seed=9300 + i, speed=1.0 + 0.125 * (i % 2),
                          marks=(i // 3) % 2 == 0, join=joins[i % len(joins)]))
    return tab, specs


def _alone(model, s):
    n = len(s["chunks"])
    v = s["voice"]
    if "styles" in v:
        kw = dict(styles=v["styles"])
    elif isinstance(v["voices"], int):
        kw = dict(voice_ids=[[v["voices"]]] * n, weights=[[0.0]] * n)
    else:
        kw = dict(voice_ids=[[a for a, _ in v["voices"]]] * n, weights=[[w for _, w in v["voices"]]] * n)
    kw.update(speeds=[s["speed"]], seed=s["seed"], fmt=s["fmt"])
    join = s["join"] if s["join"] is not None else PLAIN
    if s["marks"]:
        bodies, marks = model.infer_requests_joined(s["chunks"], [n], join, marks=True, **kw)
        return bodies[0], marks[0]
    return model.infer_requests_joined(s["chunks"], [n], join, **kw)[0], None


def _same(got, want):
    if isinstance(want, bytes):
        assert isinstance(got, bytes) and got == want
    else:
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _dispatcher_scenario(model):
    """8 client threads, 16 requests of 1..3 chunks, joined and plain, with and without marks, rates and forms mixed, voices by
    row / id / mix; each result equals infer_requests_joined of the request alone (R = 1, its seed, utterance base 0)."""
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
                                          **s["voice"])
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
        body, marks = _alone(model, s)
        if s["marks"]:
            _same(out[i][0], body)
            np.testing.assert_array_equal(out[i][1], marks)
            assert out[i][1].shape[0] == sum(len(c) + 1 for c in s["chunks"]) and out[i][1][0] == 0
        else:
            _same(out[i], body)
        if s["join"] not in (None, PLAIN):  # (a joined request is not its plain self: the spec reached the batch)
            kw = dict(s, join=None, marks=False)
            changed += len(_raw_of(_alone(model, kw)[0])) != len(_raw_of(body))
    assert changed > 0
    assert st["requests"] == len(specs) and st["batches"] < st["requests"]
    return st


def test_dispatcher_joined_requests_equal_their_solo_runs(hip_model):
    _dispatcher_scenario(hip_model)


def test_dispatcher_copy_out_path_in_a_fresh_process():
    """KX_PINNED_LIVE_CAP_MB is read once per process: with 0 every request's body and marks are copied out into ONE plain
    allocation, the marks 8-aligned behind the body."""
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
