"""GPU: requests of several chunks with the bodies the reference's servers send packed on the device — the float WAV of the
HTTP server (kokorox-openai/src/lib.rs:416-425) and the base64 16-bit WAV of the WebSocket server (`encode_audio`,
kokorox-websocket/src/lib.rs:696-736) — through the kernel's test hook, through kx_infer_requests and through the dispatcher.
Everything is integer- and byte-exact: every check is an equality against the host mirrors of kokorox_amd/voices.py."""
import base64
import json
import os
import struct
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [1, 2, 3, 5, 1, 1]
LD = 3008
GROUPINGS = {"six_single": [1] * 6, "two_one_three": [2, 1, 3], "one_of_six": [6]}


def _f32_bits(u):
    return np.frombuffer(struct.pack("<I", u), dtype=np.float32)[0]


def _special_values():
    one_up = np.nextafter(np.float32(1), np.float32(2))
    return np.array([_f32_bits(0x7FC12345), np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, one_up, 0.99999, 1e-5, -1e-5, _f32_bits(0x00000123),
                     32766.5 / 32767, -32766.5 / 32767, _f32_bits(0xFFC00001)], dtype=np.float32)


def _slab(rot):
    """[6, LD] rows of 600 * FRAMES[b] valid samples, NaN beyond; the special values at 0, 1, 2, 599, 600 and the last two
    positions of every row, rotated by `rot` so that every value meets every position over the rotations."""
    rng = np.random.default_rng(100 + rot)
    vals = _special_values()
    a = np.full((len(FRAMES), LD), np.nan, dtype=np.float32)
    k = rot
    for b, f in enumerate(FRAMES):
        n = 600 * f
        a[b, :n] = rng.uniform(-1.3, 1.3, n).astype(np.float32)
        for pos in (0, 1, 2, 599, 600, n - 2, n - 1):
            if pos < n:
                a[b, pos] = vals[k % len(vals)]
                k += 1
    return a


def _expect_and_compare(got: bytes, x: np.ndarray, form: int):
    from kokorox_amd import voices as V
    fin = np.isfinite(x)
    if form == 0:
        g = np.frombuffer(got, dtype=np.float32)
        assert g.shape == x.shape
        np.testing.assert_array_equal(g[fin], x[fin])
    elif form == 1:
        g = np.frombuffer(got, dtype=np.float32).reshape(-1, 2)
        assert g.shape[0] == x.shape[0]
        np.testing.assert_array_equal(g[fin, 0], x[fin])  # koko.rs:1239-1246: every sample written twice
        np.testing.assert_array_equal(g[fin, 1], x[fin])
    elif form == 2:
        g = np.frombuffer(got, dtype=np.int16)
        assert g.shape == x.shape
        want = np.trunc(np.clip(x[fin], -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)  # websocket lib.rs:701-704
        np.testing.assert_array_equal(g[fin], want)
    elif form == 3:
        assert got == V.wav_f32_body(x)  # raw bytes: the NaN payloads are covered
    else:
        want = V.wav16_base64(x)
        assert len(got) == len(want) == 4 * ((44 + 2 * x.shape[0] + 2) // 3)
        if got != want:
            i = next(j for j in range(len(want)) if got[j] != want[j])
            raise AssertionError(f"base64 text differs first at character {i} of {len(want)} (group {i // 4}): "
                                 f"{got[max(0, i - 8): i + 8]!r} vs {want[max(0, i - 8): i + 8]!r}")
        assert got.endswith(b"=") and not got.endswith(b"==")


@pytest.mark.parametrize("grouping", sorted(GROUPINGS))
def test_hook_packs_every_form_and_grouping(grouping):
    from kokorox_amd import hip_koko as hk
    cpr = GROUPINGS[grouping]
    R = len(cpr)
    first = np.concatenate([[0], np.cumsum(cpr)])
    for rot in range(0, 15, 3):
        a = _slab(rot)
        streams = [np.concatenate([a[b, : 600 * FRAMES[b]] for b in range(first[r], first[r + 1])]) for r in range(R)]
        for forms in ([0] * R, [1] * R, [2] * R, [3] * R, [4] * R, [(4 - r - rot) % 5 for r in range(R)]):
            got = hk.pack_requests(a, FRAMES, cpr, forms)
            assert len(got) == R
            for r in range(R):
                _expect_and_compare(got[r], streams[r], forms[r])


def test_hook_null_grouping_is_one_request_per_row():
    """chunks_per_request = null is what kx_infer / kx_infer_packed / kx_infer_voices hand to the plan builder: R = B single-row
    requests sharing one form 0..2.  Row 0 of one frame, rows of unequal length (workgroups past a short region exit) and the
    last row, against the numpy mirrors and against the same rows grouped explicitly."""
    from kokorox_amd import hip_koko as hk
    B = len(FRAMES)
    for rot in range(0, 15, 3):
        a = _slab(rot)
        for f in (0, 1, 2):
            got = hk.pack_requests(a, FRAMES, None, [f])
            assert len(got) == B
            for b in range(B):
                _expect_and_compare(got[b], a[b, : 600 * FRAMES[b]], f)
            assert got == hk.pack_requests(a, FRAMES, [1] * B, [f] * B)


def test_hook_known_answer_of_the_fixture():
    from kokorox_amd import hip_koko as hk
    with open(os.path.join(ROOT, "tests", "golden", "wire_formats.json"), encoding="utf-8") as f:
        gold = json.load(f)
    x = np.array([float(s) for s in gold["samples"]], dtype=np.float32)
    a = np.full((1, LD), np.nan, dtype=np.float32)
    a[0, :600] = 0.0
    a[0, :12] = x
    body, text = hk.pack_requests(np.repeat(a, 2, axis=0), [1, 1], [1, 1], [3, 4])
    assert body[:44].hex() == gold["wav_f32_header_hex"] and body[44: 44 + 48] == x.tobytes()
    want = gold["wav16_base64"].encode()
    # the two headers differ in their size fields only (bytes 4..7 and 40..43: groups 1, 2, 13, 14); groups 15..21 are the
    # fixture's samples 0..10 and the low byte of sample 11
    for lo, hi in ((0, 4), (12, 52), (60, 88)):
        assert text[lo:hi] == want[lo:hi], (lo, hi)
    raw = base64.b64decode(text, validate=True)
    assert struct.unpack("<I", raw[4:8])[0] == 36 + 1200 and struct.unpack("<I", raw[40:44])[0] == 1200
    assert np.frombuffer(raw[44: 44 + 24], dtype="<i2").tolist() == gold["pcm16"]
    assert len(text) == gold["silence_text_length"]["1"]


# ---- model -----------------------------------------------------------------------------------------------------------
def _chunks():
    from oracle import kokoro_ref as R
    return [list(int(v) for v in R.synthetic_inputs(1, k, seed=500 + k)[0]) for k in (1, 10, 3, 5, 2, 7)]  # 3..12 tokens with the pads


def _mirror(form, x):
    from kokorox_amd import voices as V
    if form == 0:
        return x
    if form == 1:
        return np.stack([x, x], axis=1)
    if form == 2:
        return np.trunc(np.clip(x, -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)
    return V.wav_f32_body(x) if form == 3 else V.wav16_base64(x)


def _same(got, want):
    if isinstance(want, bytes):
        assert isinstance(got, bytes) and got == want
    else:
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("pinned", [[1, 2], None], ids=["pinned_1_2", "unpinned"])
def test_model_requests_equal_the_mirrors_of_the_same_rows(hip_model, pinned):
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    names = ["af_sky", "af_nicole", "am_adam", "bf_emma"]
    styles = {n: tab[i] for i, n in enumerate(names)}
    hip_model.set_voice_table(tab)
    hip_model.set_utterance_base(0)
    toks = _chunks()
    cpr = [1, 2, 3]
    first = [0, 1, 3, 6]
    rows = [V.mix_styles(styles, names[b % 4], len(t) - 2)[0] for b, t in enumerate(toks)]
    hip_model.set_pinned_durations(pinned)
    try:
        wav = hip_model.infer_batch(toks, rows, [1.0], seed=21)
        streams = [np.concatenate(wav[first[r]: first[r + 1]]) for r in range(3)]
        if pinned:
            assert [w.shape[0] // 600 for w in wav] == [sum(pinned[t % 2] for t in range(len(tk))) for tk in toks]
        for fmt in (0, 1, 2, 3, 4, [4, 3, 2], [1, 4, 0]):
            got = hip_model.infer_requests(toks, cpr, styles=rows, speeds=[1.0], seed=21, fmt=fmt)
            for r in range(3):
                _same(got[r], _mirror(fmt[r] if isinstance(fmt, list) else fmt, streams[r]))
        # voices by id: single voices (row copy) and a mix, looked up on the device per chunk
        vid = [[b % 4] for b in range(6)]
        got = hip_model.infer_requests(toks, cpr, voice_ids=vid, weights=[[0.0]] * 6, speeds=[1.0], seed=21, fmt=[4, 3, 4])
        for r in range(3):
            _same(got[r], _mirror([4, 3, 4][r], streams[r]))
        mix_rows = [V.mix_styles(styles, "af_sky.4+am_adam.5", len(t) - 2)[0] for t in toks]
        mwav = hip_model.infer_batch(toks, mix_rows, [1.0], seed=22)
        got = hip_model.infer_requests(toks, cpr, voice_ids=[[0, 2]] * 6, weights=[[4.0, 5.0]] * 6, speeds=[1.0], seed=22, fmt=4)
        for r in range(3):
            _same(got[r], V.wav16_base64(np.concatenate(mwav[first[r]: first[r + 1]])))
        # R = 1 is the chunk loop: tts_chunks' samples, framed
        inner = [t[1:-1] for t in toks[3:]]
        one = V.tts_chunks(hip_model, styles, "bf_emma", inner, seed=9)
        assert V.tts_request(hip_model, styles, "bf_emma", inner, seed=9, fmt=3) == V.wav_f32_body(one)
        assert V.tts_request(hip_model, styles, "bf_emma", inner, seed=9, fmt=4) == V.wav16_base64(one)
        np.testing.assert_array_equal(V.tts_request(hip_model, styles, "bf_emma", inner, seed=9, fmt=0), one)
    finally:
        hip_model.set_pinned_durations(None)


def test_model_refuses_bad_groupings_and_formats(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    toks = _chunks()[:3]
    rows = [W.synthetic_voices(1)[0, len(t) - 2, 0] for t in toks]
    for cpr, fmt in (([1, 2], 5), ([1, 2], [0, 5]), ([1, 2], -1), ([1, 0, 2], 0), ([1, 1], 0), ([2, 2], 0), ([3, 1], 0), ([1, 2], [0, 1, 2])):
        with pytest.raises(hk.KokoroxHipError) as e:
            hip_model.infer_requests(toks, cpr, styles=rows, fmt=fmt)
        assert e.value.code == hk.KX_ERR_INVALID, (cpr, fmt)
    for fmt in (3, 4):  # the old entries keep their three forms
        with pytest.raises(hk.KokoroxHipError) as e:
            hip_model.infer_packed(toks, rows, fmt=fmt)
        assert e.value.code == hk.KX_ERR_INVALID


# ---- dispatcher ------------------------------------------------------------------------------------------------------
def _request_specs():
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    tab = W.synthetic_voices(4)
    specs = []
    for i in range(16):
        n = 1 + i % 4
        chunks = [list(int(v) for v in R.synthetic_inputs(1, 1 + (5 * i + 3 * c) % 10, seed=700 + 10 * i + c)[0]) for c in range(n)]
        kind = i % 3
        if kind == 0:
            voice = dict(styles=[tab[i % 4, len(c) - 2, 0] for c in chunks])
        elif kind == 1:
            voice = dict(voices=i % 4)
        else:
            voice = dict(voices=[(i % 4, 4.0), ((i + 1) % 4, 5.0)])
        specs.append(dict(chunks=chunks, voice=voice, fmt=i % 5, seed=9000 + i, speed=1.0 + 0.125 * (i % 2)))
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
    return model.infer_requests(s["chunks"], [n], speeds=[s["speed"]], seed=s["seed"], fmt=s["fmt"], **kw)[0]


def _dispatcher_scenario(model):
    """8 client threads, 16 requests of 1..4 chunks in all five forms, voices by row / id / mix; then request 0 again beside
    other traffic.  Returns the dispatcher's stats."""
    from kokorox_amd import hip_koko as hk
    tab, specs = _request_specs()
    model.set_voice_table(tab)
    model.set_utterance_base(0)
    model.set_pinned_durations(None)
    d = hk.Dispatcher([model], max_batch=8, max_wait_us=100000)
    out = [None] * len(specs)
    again = [None] * 4
    errs = []

    def submit(s):
        return d.submit_request(s["chunks"], speed=s["speed"], seed=s["seed"], fmt=s["fmt"], **s["voice"])

    def client(t):
        try:
            for i in (t, t + 8):
                out[i] = submit(specs[i])
        except Exception as e:  # pragma: no cover
            errs.append(e)

    def second_round(t):
        try:
            again[t] = submit(specs[[3, 7, 11, 14][t]])
        except Exception as e:  # pragma: no cover
            errs.append(e)

    try:
        for target, n in ((client, 8), (second_round, 4)):
            th = [threading.Thread(target=target, args=(t,)) for t in range(n)]
            for t in th:
                t.start()
            for t in th:
                t.join(timeout=300)
        st = d.stats()
        with pytest.raises(hk.KokoroxHipError):
            d.submit_request([[0, 5, 0]] * 9, voices=0)  # more chunks than max_batch
        with pytest.raises(hk.KokoroxHipError):
            d.submit_request(specs[0]["chunks"], fmt=5, **specs[0]["voice"])
    finally:
        d.close()
    assert not errs, errs
    for i, s in enumerate(specs):
        _same(out[i], _alone(model, s))
    for t, i in enumerate([3, 7, 11, 14]):  # the same request beside different traffic: the same bytes
        _same(again[t], out[i])
    assert st["requests"] == len(specs) + 4 and st["batches"] < st["requests"]
    # rows: no batch went past max_batch rows, and one held more rows than the largest request has chunks (4), i.e. at least two
    # requests; only four of the requests are single rows, so a batch of five rows or more has more rows than requests
    # (This rests on timing: at least two of the eight threads' first submits must reach the queue within the dispatcher's
    # max_wait_us of 100 ms, which is why that wait is so long here; do not shorten it.  The stats expose no per-batch pair
    # of rows and requests to assert on instead.)
    assert 5 <= st["max_batch"] <= 8, st
    return st


def test_dispatcher_requests_equal_their_solo_runs(hip_model):
    _dispatcher_scenario(hip_model)


def test_dispatcher_single_row_requests_beside_each_other_and_beside_chunks(hip_model):
    """The single-utterance traffic in forms 0, 1, 2 goes through the same packer as every other request: one batch of three
    such requests (submit_ex), then three more (submit_request) beside a two-chunk form-4 request.  Every result equals its
    solo run -- kx_infer_packed for the single rows, kx_infer_requests for the chunks -- byte for byte."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    toks = _chunks()
    rows = [W.synthetic_voices(1)[0, len(t) - 2, 0] for t in toks]
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations(None)
    d = hk.Dispatcher([hip_model], max_batch=8, max_wait_us=100000)
    first, second, errs = [None] * 3, [None] * 4, []

    def one(i):
        try:
            first[i] = d.submit_ex(toks[i], style=rows[i], seed=800 + i, fmt=i)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    def two(i):
        try:
            if i < 3:
                second[i] = d.submit_request([toks[i]], styles=[rows[i]], seed=810 + i, fmt=(i + 1) % 3)
            else:
                second[i] = d.submit_request(toks[3:5], styles=rows[3:5], seed=820, fmt=4)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    try:
        for target, n in ((one, 3), (two, 4)):
            th = [threading.Thread(target=target, args=(i,)) for i in range(n)]
            for t in th:
                t.start()
            for t in th:
                t.join(timeout=300)
        st = d.stats()
    finally:
        d.close()
    assert not errs, errs
    for i in range(3):
        _same(first[i], hip_model.infer_packed([toks[i]], [rows[i]], [1.0], seed=800 + i, fmt=i)[0])
        _same(second[i], hip_model.infer_packed([toks[i]], [rows[i]], [1.0], seed=810 + i, fmt=(i + 1) % 3)[0])
    _same(second[3], hip_model.infer_requests(toks[3:5], [2], styles=rows[3:5], speeds=[1.0], seed=820, fmt=4)[0])
    # (as above, this rests on the threads' submits reaching the queue within max_wait_us of each other)
    assert st["requests"] == 7 and st["batches"] < st["requests"], st


def test_dispatcher_copy_out_path_in_a_fresh_process():
    """KX_PINNED_LIVE_CAP_MB is read once per process: with 0 every batch's regions are copied out into plain allocations,
    one per REQUEST, instead of sharing the page-locked buffer."""
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
