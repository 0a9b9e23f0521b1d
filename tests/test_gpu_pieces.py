"""GPU: pieces (include/kokorox_hip.h, "pieces") -- a request delivered in several calls -- through the test hook
(kx_test_output_plan_pieces: the model's planner and launcher on host arrays), through kx_infer_requests_pieces and through the
dispatcher.  The invariant is an EQUALITY: the payloads of a request's pieces, laid end to end, are the body of the same request run
whole, every byte, and their marks are its marks; the carry a piece leaves is the numpy definition's, bit for bit
(kokorox_amd/voices.py: piece_bodies, piece_carry, joined_marks).  The audio rows are 1..3 frames of the golden noise stream, so no
sample is special and no NaN needs latitude."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD, TAIL, INNER = 1, 2, 4
FIRST, LAST, WHOLE = 1, 2, 3
GAIN = (0, 0.5, 0.0)
RATES = (0x000, 0x100, 0x200, 0x300)
SAMPLE_BYTES = {0: 4, 1: 8, 2: 2, 3: 4, 8: 1, 9: 1}


def _all_cuts(n):
    """Every way to cut n chunks into consecutive pieces: 2^(n - 1) lists of chunk counts."""
    out = []
    for mask in range(1 << (n - 1)):
        cuts, run = [], 1
        for i in range(n - 1):
            if mask >> i & 1:
                cuts.append(run)
                run = 1
            else:
                run += 1
        out.append(cuts + [run])
    return out


class _Rows:
    """Chunk rows for the hook: durations per token, and a slab whose row c holds 600 x frames[c] samples derived from
    tests/golden/noise_stream.npz and NaN at and past them (what lies beyond a row's frames must not reach any result)."""

    def __init__(self, durations):
        with np.load(os.path.join(ROOT, "tests", "golden", "noise_stream.npz")) as f:
            z = f["z"].astype(np.float32).reshape(-1)
        self.durations = [list(d) for d in durations]
        self.frames = [sum(d) for d in self.durations]
        self.ld = 600 * max(self.frames) + 40
        self.audio = np.full((len(durations), self.ld), np.nan, dtype=np.float32)
        g = 0
        for c, f in enumerate(self.frames):
            i = np.arange(g, g + 600 * f)
            self.audio[c, : 600 * f] = np.float32(0.25) * z[i % z.shape[0]] + np.float32(0.125) * z[(7 * i + i // z.shape[0]) % z.shape[0]]
            g += 600 * f
        self.samples = [self.audio[c, : 600 * f] for c, f in enumerate(self.frames)]

    def slab(self, idx):
        dur = np.full((len(idx), 512), -7, dtype=np.int32)  # (what lies at or beyond lens[b] must not reach any result)
        for b, c in enumerate(idx):
            dur[b, : len(self.durations[c])] = self.durations[c]
        return self.audio[idx], dur, [len(self.durations[c]) for c in idx]


def _run_in_step(rows, requests, levels):
    """Every request of `requests` (dicts: chunks = indices of its rows, cuts, word, join, want) run in pieces, all of them side by
    side: call s of the hook holds piece s of every request that has one, each with the carry its piece s - 1 left.  levels: None
    (the call has no levels) or one spec for every request.  Returns per request (payloads, out_samples, marks, carries)."""
    from kokorox_amd import hip_koko as hk
    out = [([], [], [], []) for _ in requests]
    joined = any(q["join"] is not None for q in requests)
    for s in range(max(len(q["cuts"]) for q in requests)):
        live = [i for i, q in enumerate(requests) if len(q["cuts"]) > s]
        idx, cpr, words, flags, carries, joins, want = [], [], [], [], [], [], []
        for i in live:
            q = requests[i]
            a = sum(q["cuts"][:s])
            idx += q["chunks"][a: a + q["cuts"][s]]
            cpr.append(q["cuts"][s])
            words.append(q["word"])
            flags.append((FIRST if s == 0 else 0) | (LAST if s == len(q["cuts"]) - 1 else 0))
            carries.append(out[i][3][-1] if s else None)
            joins.append(q["join"] if q["join"] is not None else (0, 0, 0, 0))
            want.append(1 if q["want"] else 0)
        audio, dur, lens = rows.slab(idx)
        res, ns, marks, cout, _, _ = hk.piece_requests(audio, dur, lens, cpr, words, flags, carries, joins=joins if joined else None,
                                                       want=want, levels=None if levels is None else [levels] * len(live))
        for r, i in enumerate(live):
            out[i][0].append(res[r])
            out[i][1].append(ns[r])
            out[i][2].append(marks[r])
            out[i][3].append(cout[r].copy())
    return out


class _Mirror:
    """The numpy definition of the whole request, computed once per (chunks, join, rate): its stream at the output rate."""

    def __init__(self, rows):
        self.rows, self.cache = rows, {}

    def stream(self, chunks, join, word):
        from kokorox_amd import voices as V
        key = (tuple(chunks), join, word & 0xF00)
        if key not in self.cache:
            d = [self.rows.durations[c] for c in chunks]
            self.cache[key] = V.resample_stream(V.join_stream([self.rows.samples[c] for c in chunks], d, join), word)
        return self.cache[key]

    def body(self, chunks, join, word, level):
        from kokorox_amd import voices as V
        y = self.stream(chunks, join, word)
        return V.stream_body(y if level is None else V.level_stream(y, level), word)


def _check_pieces(rows, mirror, requests, levels, got, whole_bodies, check_numpy_slices):
    from kokorox_amd import voices as V
    n_empty = 0
    for q, (payloads, ns, marks, carries), whole in zip(requests, got, whole_bodies):
        what = f"word {q['word']:#x} cuts {q['cuts']} join {q['join']} level {levels}"
        d = [rows.durations[c] for c in q["chunks"]]
        assert b"".join(payloads) == whole, what  # every byte of the request run whole on the GPU
        assert whole == mirror.body(q["chunks"], q["join"], q["word"], levels), what
        form = q["word"] & 0xFF
        E = V.piece_ranges(V.piece_lengths(d, q["join"], q["cuts"]), q["word"])
        sizes = [SAMPLE_BYTES[form] * (b - a) for a, b in zip([0] + E[:-1], E)]
        assert ns == [b - a for a, b in zip([0] + E[:-1], E)], what
        sizes[0] += 44 if form == 3 else 0
        assert [len(p) for p in payloads] == sizes, what
        n_empty += sum(1 for p in payloads if len(p) == 0)
        if check_numpy_slices:
            assert payloads == V.piece_bodies([rows.samples[c] for c in q["chunks"]], d, q["word"], q["join"], levels, q["cuts"]), what
        want = V.piece_carry([rows.samples[c] for c in q["chunks"]], d, q["word"], q["join"], q["cuts"])
        for k, c in enumerate(carries):
            assert c.tobytes() == want[k].tobytes(), f"{what}: the carry of piece {k}"
        if q["want"]:
            m = V.joined_marks(d, q["word"], q["join"])
            np.testing.assert_array_equal(np.concatenate(marks), m, err_msg=what)
            assert int(m[-1]) == E[-1], what
        else:
            assert all(mk.shape[0] == 0 for mk in marks), what
    return n_empty


def _whole_bodies(rows, requests, levels):
    """The same requests run whole through kx_test_output_plan_levelled (kx_test_output_plan without levels), in one call."""
    from kokorox_amd import hip_koko as hk
    idx = [c for q in requests for c in q["chunks"]]
    audio, dur, lens = rows.slab(idx)
    cpr, words = [len(q["chunks"]) for q in requests], [q["word"] for q in requests]
    joined = any(q["join"] is not None for q in requests)
    joins = [q["join"] if q["join"] is not None else (0, 0, 0, 0) for q in requests] if joined else None
    if levels is None:  # (all-zero specs: the plain kernels, the plain bytes)
        return hk.join_requests(audio, dur, lens, cpr, words, joins if joined else [(0, 0, 0, 0)] * len(requests))[0]
    return hk.level_requests(audio, dur, lens, cpr, words, [levels] * len(requests), joins=joins)[0]


# ---- 5. every cut of five chunks, four rates, four forms, with and without a gain --------------------------------------------------
PLAIN_ROWS = [[1], [1, 1], [1], [2, 1], [1]]  # frames (1, 2, 1, 3, 1)


@pytest.fixture(scope="module")
def plain_rows():
    rows = _Rows(PLAIN_ROWS)
    assert rows.frames == [1, 2, 1, 3, 1]
    return rows, _Mirror(rows)


@pytest.mark.parametrize("levels", [None, GAIN], ids=["no_level", "gain_half"])
def test_every_cut_of_five_chunks_joins_to_the_whole_body(plain_rows, levels):
    """5. 16 cuts x 4 rates x forms 0, 2, 3, 8: the pieces' payloads joined equal the whole request's body from
    kx_test_output_plan_levelled byte for byte, they equal voices.piece_bodies, and carry_out equals voices.piece_carry bit for
    bit.  All 256 requests run side by side: five calls of the hook, one per piece index."""
    rows, mirror = plain_rows
    requests = [dict(chunks=[0, 1, 2, 3, 4], cuts=cuts, word=form | rate, join=None, want=False)
                for rate in RATES for form in (0, 2, 3, 8) for cuts in _all_cuts(5)]
    got = _run_in_step(rows, requests, levels)
    whole = _whole_bodies(rows, [dict(q, cuts=[5]) for q in requests[::16]], levels)
    _check_pieces(rows, mirror, requests, levels, got, [whole[i // 16] for i in range(len(requests))], check_numpy_slices=True)


def test_a_request_run_whole_through_the_piece_hook_is_the_whole_request(plain_rows):
    """Both flags: planned and launched as ever, the all-zero carry, and any form -- a loudness-normalised FLAC-free mix here."""
    from kokorox_amd import hip_koko as hk
    rows, mirror = plain_rows
    audio, dur, lens = rows.slab([0, 1, 2, 3, 4] * 2)
    words = [0x104, 0x212]
    res, ns, _, cout, lv, _ = hk.piece_requests(audio, dur, lens, [5, 5], words, [WHOLE, WHOLE], None, levels=[(1, 1.0, 0.5), GAIN])
    want = hk.level_requests(audio, dur, lens, [5, 5], words, [(1, 1.0, 0.5), GAIN])
    assert res == want[0] and ns == want[1] and lv.tobytes() == want[3].tobytes()
    assert cout.tobytes() == bytes(cout.nbytes)


# ---- 6. joins: trimmed pads, pauses, fades; pieces that keep nothing, or less than a window ----------------------------------------
# pads at both ends of every chunk.  In the thin rows chunk 2 has no frame between its pads: trimmed at both ends with keep_ms 0 it
# keeps 0 samples (a row that keeps nothing has no room for a fade: those specs have none), with keep_ms 1 it keeps 48, filled by its
# two fades of 1 ms and fewer than the 72 samples either side of an 8 kHz output.  In the full rows every chunk keeps a frame or more.
THIN_ROWS = [[1, 1, 1], [1, 2, 1], [1, 0, 1], [2, 1, 1], [1, 1, 1]]
FULL_ROWS = [[1, 1, 1], [1, 2, 1], [1, 1, 1], [2, 1, 1], [1, 1, 1]]
ALL = HEAD | TAIL | INNER
JOIN_CASES = [("thin", (ALL, 0, 0, 0)), ("thin", (ALL, 0, 10, 0)), ("thin", (ALL, 1, 0, 1)), ("full", (ALL, 0, 0, 1)), ("full", (ALL, 0, 10, 1))]
JOINS = [j for _, j in JOIN_CASES[:3]]


@pytest.fixture(scope="module")
def join_rows():
    rows = _Rows(THIN_ROWS)
    return rows, _Mirror(rows)


@pytest.fixture(scope="module")
def full_rows():
    rows = _Rows(FULL_ROWS)
    return rows, _Mirror(rows)


@pytest.mark.parametrize("which,join", JOIN_CASES, ids=["thin_pause_0", "thin_pause_10ms", "thin_keep_1ms", "fade_pause_0", "fade_pause_10ms"])
def test_joined_pieces_join_to_the_whole_body_and_its_marks(join_rows, full_rows, which, join):
    """6, 7. Every cut of the five chunks x 4 rates in mu-law and float WAV, with a gain, with marks: payloads, carries and marks,
    under TRIM_HEAD | TAIL | INNER with keep_ms 0, pause 0 and 10 ms, fade 1 ms where every chunk keeps samples to fade.  In the
    thin rows chunk 2 is a middle piece of its own in a quarter of the cuts: it keeps 0 samples (keep_ms 0, pause 0: 0 bytes, and
    its carry is the carry before it), 240 zeros (pause 10 ms) or 48 samples (keep_ms 1: its tail is mostly the old tail)."""
    from kokorox_amd import voices as V
    rows, mirror = join_rows if which == "thin" else full_rows
    kept = [keep for _, keep, _, _, _ in V.join_rows(rows.durations, join)]
    assert kept[2] == (600 if which == "full" else (48 if join[1] else 0)) and all(k >= 600 for i, k in enumerate(kept) if i != 2)
    requests = [dict(chunks=[0, 1, 2, 3, 4], cuts=cuts, word=form | rate, join=join, want=True)
                for rate in RATES for form in (8, 3) for cuts in _all_cuts(5)]
    got = _run_in_step(rows, requests, GAIN)
    whole = _whole_bodies(rows, [dict(q, cuts=[5]) for q in requests[::16]], GAIN)
    n_empty = _check_pieces(rows, mirror, requests, GAIN, got, [whole[i // 16] for i in range(len(requests))], check_numpy_slices=False)
    # the middle piece that is chunk 2 alone (cuts [.., 1, ..] with two chunks before it): what it emitted and what it left
    for q, (payloads, ns, _, carries) in zip(requests, got):
        edges = np.cumsum(q["cuts"]).tolist()
        if 2 in edges and 3 in edges:
            k = edges.index(3)
            own = int(carries[k]["src_samples"]) - int(carries[k - 1]["src_samples"])
            assert own == kept[2] + 24 * join[2]
            if own == 0:
                assert len(payloads[k]) == 0 and carries[k]["tail"].tobytes() == carries[k - 1]["tail"].tobytes()
            elif q["word"] >> 8 and own < 256:
                n = int(carries[k]["n_tail"])
                assert n == 256 and carries[k]["tail"][: n - own].tobytes() == carries[k - 1]["tail"][own:n].tobytes()
    assert n_empty >= (32 if which == "thin" and join[1:3] == (0, 0) else 0)


def test_a_first_piece_shorter_than_a_window_emits_nothing_at_8_khz(join_rows):
    """48 kept samples cannot hold the 72 an 8 kHz output needs behind it: a first piece of them is 0 bytes (a float WAV: the header
    alone), its carry holds all 48, and the rest of the request still joins to the whole body."""
    rows, mirror = join_rows
    join = JOINS[2]
    requests = [dict(chunks=[2, 0, 3], cuts=[1, 2], word=w, join=join, want=True) for w in (0x108, 0x103, 0x208)]
    got = _run_in_step(rows, requests, None)
    whole = _whole_bodies(rows, requests, None)
    _check_pieces(rows, mirror, requests, None, got, whole, check_numpy_slices=True)
    assert [len(got[0][0][0]), len(got[1][0][0])] == [0, 44] and len(got[2][0][0]) > 0
    assert int(got[0][3][0]["n_tail"]) == 48 and int(got[0][3][0]["out_samples"]) == 0


# ---- 8. a mixed batch ------------------------------------------------------------------------------------------------------------------
def test_pieces_of_two_requests_beside_a_whole_loudness_request(plain_rows):
    """8. Two requests at different pieces, at different rates, beside one whole loudness-normalised request in one call: each
    result equals the bits it has alone."""
    from kokorox_amd import hip_koko as hk
    rows, _ = plain_rows
    a = dict(chunks=[0, 1, 2, 3, 4], cuts=[2, 1, 2], word=0x108, join=None, want=True)   # its middle piece goes into the batch
    b = dict(chunks=[4, 3, 2, 1, 0], cuts=[1, 2, 2], word=0x303, join=None, want=False)  # its last piece
    alone = _run_in_step(rows, [a], GAIN)[0], _run_in_step(rows, [b], GAIN)[0]
    loud_idx = [0, 1, 2, 3, 4] * 3
    la, ld, ll = rows.slab(loud_idx)
    loud = (1, -20.0, 0.9)
    solo = hk.loudness_requests(la, ld, ll, [15], [0x202], [loud])
    idx = [2] + [1, 0] + loud_idx
    audio, dur, lens = rows.slab(idx)
    none = hk.LOUDNESS_NONE
    res, ns, marks, cout, lv, out_ld = hk.piece_requests(audio, dur, lens, [1, 2, 15], [0x108, 0x303, 0x202], [0, LAST, WHOLE],
                                                         [alone[0][3][0], alone[1][3][1], None], want=[1, 0, 0],
                                                         levels=[GAIN, GAIN, hk.LEVEL_PLAIN], loudness=[none, none, loud])
    assert res[0] == alone[0][0][1] and ns[0] == alone[0][1][1] and cout[0].tobytes() == alone[0][3][1].tobytes()
    np.testing.assert_array_equal(marks[0], alone[0][2][1])
    assert res[1] == alone[1][0][2] and ns[1] == alone[1][1][2] and cout[1].tobytes() == alone[1][3][2].tobytes()
    assert res[2] == solo[0][0] and ns[2] == solo[1][0] and out_ld[2].tobytes() == solo[3][0].tobytes()
    assert cout[2].tobytes() == bytes(cout[2].nbytes)
    assert solo[3][0][1] != 1.0 and lv[0].tolist()[1] == 0.5  # (the loudness spec reached its request, the gain its piece)


# ---- 9. guards -----------------------------------------------------------------------------------------------------------------------
def test_guards_behind_bodies_and_around_the_carry_block_hold(join_rows):
    """9. The hook poisons and checks 64 bytes behind the bodies, behind the resampled streams, in front of and behind the carry
    block and behind the carried tails (KX_ERR_STATE otherwise); here with regions of 0 bytes, whose neighbours' guards are the
    first thing a stray store would hit, at every rate, and without marks or levels so that the carry block follows the bodies."""
    from kokorox_amd import hip_koko as hk
    rows, _ = join_rows
    join = JOINS[0]
    for rate in RATES:
        first = _run_in_step(rows, [dict(chunks=[0, 1, 2], cuts=[2, 1], word=8 | rate, join=join, want=False)], None)[0]
        audio, dur, lens = rows.slab([2, 2])
        res, ns, _, cout, _, _ = hk.piece_requests(audio, dur, lens, [1, 1], [8 | rate, 8 | rate], [0, 0], [first[3][0], first[3][0]],
                                                   joins=[join, join])
        assert res == [b"", b""] and ns == [0, 0]
        for c in cout:  # (a piece that keeps nothing leaves the tail it was given, and counts its chunk)
            assert c["tail"].tobytes() == first[3][0]["tail"].tobytes() and int(c["reserved"]) == 3
            assert (int(c["src_samples"]), int(c["out_samples"])) == (int(first[3][0]["src_samples"]), int(first[3][0]["out_samples"]))


def test_the_hook_refuses_what_a_piece_cannot_carry(plain_rows):
    from kokorox_amd import hip_koko as hk
    rows, _ = plain_rows
    audio, dur, lens = rows.slab([0, 1])
    with pytest.raises(hk.KokoroxHipError, match="infer: a piece cannot carry a sized form"):
        hk.piece_requests(audio, dur, lens, [2], [0x104], [FIRST])
    with pytest.raises(hk.KokoroxHipError, match="infer: a piece cannot carry a measured level"):
        hk.piece_requests(audio, dur, lens, [2], [0x108], [FIRST], levels=[(1, 1.0, 0.5)])
    with pytest.raises(hk.KokoroxHipError, match="infer: bad piece carry"):
        hk.piece_requests(audio, dur, lens, [2], [0x108], [LAST])


# ---- 10, 11. the model and the dispatcher -----------------------------------------------------------------------------------------------
PINNED = [3, 3, 3, 4]
MODEL_JOIN = (HEAD | TAIL | INNER, 10, 85, 1)


def _model_chunks():
    """Two chunks of 6 tokens each, the two pads included."""
    from oracle import kokoro_ref as R
    return [list(int(v) for v in R.synthetic_inputs(1, 4, seed=640 + k)[0]) for k in range(2)]


def _raw_of(x):
    return x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()


@pytest.mark.parametrize("join", [None, MODEL_JOIN], ids=["appended", "joined"])
def test_model_two_pieces_equal_the_request_run_whole(hip_model, join):
    """10. kx_infer_requests_pieces in two calls against kx_infer_requests_levelled in one: the same seed, every row at the utterance
    index it has in the whole request, 8 kHz mu-law, pinned durations; the bytes joined are equal, and so are the marks."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    toks = _model_chunks()
    assert [len(t) for t in toks] == [6, 6]
    tab = W.synthetic_voices(2)
    rows = [tab[b % 2, len(t) - 2, 0] for b, t in enumerate(toks)]
    hip_model.set_pinned_durations(PINNED)
    hip_model.set_utterance_base(0)
    try:
        kw = dict(speeds=[1.0], seed=31, fmt=0x108)
        whole, marks, _ = hip_model.infer_requests_levelled(toks, [2], GAIN, joins=join, styles=rows, marks=True, **kw)
        p0, m0, c0, _ = hip_model.infer_requests_pieces(toks[:1], [1], [FIRST], None, levels=GAIN, joins=join, styles=rows[:1], marks=True, **kw)
        assert int(c0[0]["magic"]) == hk.PIECE_MAGIC and int(c0[0]["reserved"]) == 1 and int(c0[0]["format_word"]) == 0x108
        hip_model.set_utterance_base(1)
        p1, m1, c1, _ = hip_model.infer_requests_pieces(toks[1:], [1], [LAST], c0, levels=GAIN, joins=join, styles=rows[1:], marks=True, **kw)
        hip_model.set_utterance_base(0)
        assert p0[0] + p1[0] == _raw_of(whole[0]) and len(p0[0]) > 0 and len(p1[0]) > 0
        np.testing.assert_array_equal(np.concatenate([m0[0], m1[0]]), marks[0])
        assert int(c1[0]["out_samples"]) == len(_raw_of(whole[0])) and int(c1[0]["reserved"]) == 2
        # the same through the helper that holds the carry, as a float WAV: the header once, then every sample
        wav = hip_model.infer_requests_levelled(toks, [2], GAIN, joins=join, styles=rows, speeds=[1.0], seed=31, fmt=0x303)[0][0]
        stream = hk.RequestStream(hip_model, fmt=0x303, join=join, level=GAIN, seed=31)
        parts = [stream.send(toks[:1], rows[:1]), stream.send(toks[1:], rows[1:], last=True)]
        assert b"".join(parts) == wav and parts[0][:4] == b"RIFF" and stream.closed
        with pytest.raises(ValueError):
            stream.send(toks[:1], rows[:1])
    finally:
        hip_model.set_utterance_base(0)
        hip_model.set_pinned_durations(None)


def test_model_refuses_what_a_piece_cannot_carry(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    toks = _model_chunks()
    rows = [W.synthetic_voices(1)[0, len(t) - 2, 0] for t in toks]
    for kw, text in ((dict(fmt=0x104), "infer: a piece cannot carry a sized form"), (dict(fmt=0x10C), "infer: a piece cannot carry a sized form"),
                     (dict(fmt=0x108, levels=(1, 1.0, 0.5)), "infer: a piece cannot carry a measured level"),
                     (dict(fmt=0x108, levels=(0x100, 0.5, 0.0)), "infer: a piece cannot carry a measured level")):
        with pytest.raises(hk.KokoroxHipError, match=text):
            hip_model.infer_requests_pieces(toks, [2], [FIRST], None, styles=rows, **kw)
    with pytest.raises(hk.KokoroxHipError, match="infer: bad piece carry"):
        hip_model.infer_requests_pieces(toks, [2], [LAST], None, styles=rows, fmt=0x108)
    bad = np.zeros(1, hk.PIECE_CARRY_DTYPE)
    bad["magic"], bad["format_word"], bad["src_samples"], bad["n_tail"], bad["reserved"] = hk.PIECE_MAGIC, 0x108, 2400, 300, 1
    with pytest.raises(hk.KokoroxHipError, match="infer: bad piece carry"):
        hip_model.infer_requests_pieces(toks, [2], [0], bad, styles=rows, fmt=0x108)
    with pytest.raises(hk.KokoroxHipError, match="infer: bad piece flags"):
        hip_model.infer_requests_pieces(toks, [2], [4], None, styles=rows, fmt=0x108)
    # a request run whole through the entry is the request of the levelled entry, and its carry is all zeros
    hip_model.set_utterance_base(0)
    got, cout, _ = hip_model.infer_requests_pieces(toks, [2], [WHOLE], None, levels=(1, 1.0, 0.5), styles=rows, fmt=0x104, seed=3)
    want = hip_model.infer_requests_levelled(toks, [2], (1, 1.0, 0.5), styles=rows, fmt=0x104, seed=3)[0]
    assert got[0] == want[0] and cout.tobytes() == bytes(cout.nbytes)


def test_dispatcher_pieces_of_four_clients_equal_their_requests_run_whole(hip_model):
    """11. Four clients at once, each sending its request of two chunks in two pieces through Dispatcher.submit_request(piece=...):
    different seeds, rates and forms, with and without a join; the bytes joined equal kx_infer_requests_levelled of the request
    alone (R = 1, its seed, utterance base 0), whatever the pieces were batched with.  And one refusal through this entry."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    toks = _model_chunks()
    tab = W.synthetic_voices(4)
    specs = [dict(fmt=0x108, join=None, level=GAIN, seed=71), dict(fmt=0x303, join=MODEL_JOIN, level=None, seed=72),
             dict(fmt=0x002, join=MODEL_JOIN, level=GAIN, seed=73), dict(fmt=0x209, join=None, level=None, seed=74)]
    hip_model.set_pinned_durations(PINNED)
    hip_model.set_utterance_base(0)
    out, errs = [None] * 4, []
    d = hk.Dispatcher([hip_model], max_batch=8, max_wait_us=100000)

    def client(i):
        try:
            s = specs[i]
            rows = [tab[i, len(t) - 2, 0] for t in toks]
            stream = hk.RequestStream(d, fmt=s["fmt"], join=s["join"], level=s["level"], seed=s["seed"], marks=True)
            out[i] = [stream.send(toks[:1], rows[:1]), stream.send(toks[1:], rows[1:], last=True)]
        except Exception as e:  # pragma: no cover
            errs.append(e)

    try:
        th = [threading.Thread(target=client, args=(i,)) for i in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        st = d.stats()
        with pytest.raises(hk.KokoroxHipError, match="dispatcher_submit_request: a piece cannot carry a sized form"):
            d.submit_request(toks[:1], styles=[tab[0, 4, 0]], fmt=0x104, piece=(FIRST, None))
        with pytest.raises(hk.KokoroxHipError, match="dispatcher_submit_request: bad piece carry"):
            d.submit_request(toks[:1], styles=[tab[0, 4, 0]], fmt=0x108, piece=(LAST, None))
    finally:
        d.close()
    try:
        assert not errs, errs
        assert st["requests"] == 8 and st["batches"] < 8  # (pieces of different requests shared batches)
        for i, s in enumerate(specs):
            rows = [tab[i, len(t) - 2, 0] for t in toks]
            kw = dict(styles=rows, speeds=[1.0], seed=s["seed"], fmt=s["fmt"], marks=True)
            level = s["level"] if s["level"] is not None else hk.LEVEL_PLAIN
            whole, marks, _ = hip_model.infer_requests_levelled(toks, [2], level, joins=s["join"], **kw)
            (b0, m0), (b1, m1) = out[i]
            assert b0 + b1 == _raw_of(whole[0]), i
            np.testing.assert_array_equal(np.concatenate([m0, m1]), marks[0])
    finally:
        hip_model.set_pinned_durations(None)
