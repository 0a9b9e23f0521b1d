"""GPU: token timing marks (include/kokorox_hip.h, "token marks") -- token_marks_kernel through its test hook, through
kx_infer_requests_marks and through the dispatcher.  The marks are exact integers: every check is an EQUALITY against the numpy
mirror of kokorox_amd/voices.py (token_marks), on durations that are known (the hook's input, a pinned pattern) or that the CPU
oracle predicts (the committed fixtures; the oracle's front half)."""
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
RATES = {0x000: 600, 0x100: 200, 0x200: 400, 0x300: 1200}
FORMS = [0, 8, 3, 1, 4, 9, 2]
INT32_MAX = 2 ** 31 - 1
NULL_MARKS = "infer: null marks argument"
NULL_MARKS_DISPATCHER = "dispatcher_submit_request: null marks argument"


def _firsts(cpr):
    return np.concatenate([[0], np.cumsum(cpr)]).astype(int)


def _expect(dur, lens, cpr, words):
    """The mirror, request by request: token_marks of the rows' VALID durations."""
    from kokorox_amd import voices as V
    first = _firsts(cpr)
    return [V.token_marks([dur[b, : lens[b]] for b in range(first[r], first[r + 1])], words[r]) for r in range(len(cpr))]


def _check_request(m, rows_dur, word):
    """What holds for every request whatever the mirror says: starts at 0, ends at K x its frames, T + 1 marks per chunk,
    strictly increasing inside a chunk (durations are >= 1), the chunk boundary stored twice."""
    K = RATES[word & 0xF00]
    assert m.dtype == np.int64 and m.shape[0] == sum(len(d) + 1 for d in rows_dur)
    assert m[0] == 0 and m[-1] == K * sum(int(np.sum(d, dtype=np.int64)) for d in rows_dur)
    o = 0
    for c, d in enumerate(rows_dur):
        part = m[o: o + len(d) + 1]
        assert (np.diff(part) > 0).all()
        if c:
            assert part[0] == m[o - 1]
        o += len(d) + 1


# ---- the kernel through its hook ------------------------------------------------------------------------------------------
HOOK_LENS = [1, 2, 3, 64, 65, 512]  # one token; the wave boundary on both sides; the full block


def _hook_durations():
    rng = np.random.default_rng(20261)
    dur = np.empty((6, 512), dtype=np.int32)
    dur[:, 0::2] = INT32_MAX  # what lies at or beyond lens[b] must not reach any result
    dur[:, 1::2] = -7
    for b, n in enumerate(HOOK_LENS):
        dur[b, :n] = rng.integers(1, 51, size=n)
        if n < 512:
            dur[b, n] = INT32_MAX if n % 2 == 0 else -7  # (the entry right behind the row, in both flavours over the rows)
    return dur


@pytest.mark.parametrize("rate", sorted(RATES))
@pytest.mark.parametrize("grouping", sorted(GROUPINGS))
def test_hook_equals_the_mirror(grouping, rate):
    from kokorox_amd import hip_koko as hk
    cpr = GROUPINGS[grouping]
    dur = _hook_durations()
    words = [FORMS[(r + rate // 0x100) % len(FORMS)] | rate for r in range(len(cpr))]  # mixed form bits: they must not matter
    got = hk.token_marks(dur, HOOK_LENS, cpr, words)
    want = _expect(dur, HOOK_LENS, cpr, words)
    first = _firsts(cpr)
    assert len(got) == len(cpr)
    for r in range(len(cpr)):
        np.testing.assert_array_equal(got[r], want[r])
        _check_request(got[r], [dur[b, : HOOK_LENS[b]] for b in range(first[r], first[r + 1])], words[r])


@pytest.mark.parametrize("grouping", sorted(GROUPINGS))
def test_hook_mixed_rates_and_want_flags(grouping):
    from kokorox_amd import hip_koko as hk
    cpr = GROUPINGS[grouping]
    R = len(cpr)
    dur = _hook_durations()
    words = [FORMS[r % len(FORMS)] | (0x100 * ((r + 1) % 4)) for r in range(R)]
    for want_flags in ([r % 2 == 0 for r in range(R)], [r % 2 == 1 or R == 1 for r in range(R)], [False] * R):
        got = hk.token_marks(dur, HOOK_LENS, cpr, words, want=want_flags)
        want = _expect(dur, HOOK_LENS, cpr, words)
        for r in range(R):
            np.testing.assert_array_equal(got[r], want[r] if want_flags[r] else np.zeros(0, np.int64))
    if R == 6:  # all four rates were in that batch
        assert {w & 0xF00 for w in words} == set(RATES)


def test_hook_64_bit_arithmetic():
    """Two rows of 512 tokens of 4096 frames each at 48 kHz: the last mark is 2 * 512 * 4096 * 1200 = 5 033 164 800 > 2^32."""
    from kokorox_amd import hip_koko as hk
    dur = np.full((2, 512), 4096, dtype=np.int32)
    got, = hk.token_marks(dur, [512, 512], [2], [hk.PACK_RATE_48000])
    want, = _expect(dur, [512, 512], [2], [hk.PACK_RATE_48000])
    np.testing.assert_array_equal(got, want)
    assert int(got[-1]) == 5033164800 and got[-1] > 2 ** 32 and got[512] == got[513] == 5033164800 // 2


# ---- the model ------------------------------------------------------------------------------------------------------------
def _chunks():
    """The six chunks of tests/test_gpu_wire_formats.py: 3..12 tokens with the pads."""
    from oracle import kokoro_ref as R
    return [list(int(v) for v in R.synthetic_inputs(1, k, seed=500 + k)[0]) for k in (1, 10, 3, 5, 2, 7)]


def _same(got, want):
    if isinstance(want, bytes):
        assert isinstance(got, bytes) and got == want
    else:
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("pattern", [[3, 3, 3, 4], [2, 5, 1, 1, 3, 7, 2]], ids=["pinned_3_3_3_4", "pinned_of_seven"])
def test_model_marks_on_pinned_durations(hip_model, pattern):
    """With a pinned pattern the durations the forward used are known: d[t] = pattern[t % n] in every chunk.  (Seven divides
    none of the token counts 3..12 but 7's own.)  The bodies must be those of infer_requests, byte for byte."""
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    tab = W.synthetic_voices(4)
    toks = _chunks()
    rows = [tab[b % 4, len(t) - 2, 0] for b, t in enumerate(toks)]
    durs = [[pattern[t % len(pattern)] for t in range(len(tk))] for tk in toks]
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations(pattern)
    try:
        for cpr in GROUPINGS.values():
            R = len(cpr)
            first = _firsts(cpr)
            words = [[4, 0x108, 0x303][r % 3] for r in range(R)]
            bodies, marks, samples = hip_model.infer_requests_marks(toks, cpr, styles=rows, speeds=[1.0], seed=21, fmt=words,
                                                                    with_samples=True)
            plain, plain_samples = hip_model.infer_requests(toks, cpr, styles=rows, speeds=[1.0], seed=21, fmt=words, with_samples=True)
            assert samples == plain_samples and len(marks) == R
            for r in range(R):
                d = durs[first[r]: first[r + 1]]
                np.testing.assert_array_equal(marks[r], V.token_marks(d, words[r]))
                _check_request(marks[r], d, words[r])
                assert int(marks[r][-1]) == samples[r]
                _same(bodies[r], plain[r])
    finally:
        hip_model.set_pinned_durations(None)


def test_model_marks_equal_the_fixtures_predicted_durations(hip_model, golden):
    """tests/golden/forward_*.npz carry the oracle's pred_dur of their inputs: per-token equality, 600 x their running sum."""
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations(None)
    for name, g in golden.items():
        bodies, marks, samples = hip_model.infer_requests_marks([list(g["ids"])], [1], styles=[list(g["style"])], speeds=[float(g["speed"])],
                                                                seed=int(g["seed"]), fmt=0, with_samples=True)
        pd = np.asarray(g["pred_dur"], dtype=np.int64)
        want = 600 * np.concatenate([np.zeros(1, np.int64), np.cumsum(pd)])
        print(name, "durations", int(pd.min()), "..", int(pd.max()), "tokens", pd.shape[0])
        np.testing.assert_array_equal(marks[0], want)
        assert int(marks[0][-1]) == samples[0] == bodies[0].shape[0]


@pytest.fixture(scope="module")
def ragged_reference(oracle):
    """The oracle's per-token durations of the ragged inputs of tests/test_gpu_forward.py (token counts 21, 9, 14, seed0 = 10, speed
    1.0): its front half alone (KokoroOracle.forward up to pred_dur), computed once."""
    import torch
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    counts = [21, 9, 14]
    ids = [R.synthetic_inputs(1, n, seed=10 + i)[0] for i, n in enumerate(counts)]
    voices = W.synthetic_voices(4)
    styles = [voices[i % 4, n, 0] for i, n in enumerate(counts)]
    durs = []
    with torch.no_grad():
        for b in range(3):
            taps = {}
            t_ids = torch.as_tensor(np.asarray(ids[b]), dtype=torch.long)
            style = torch.as_tensor(np.asarray(styles[b], dtype=np.float32)).to(oracle.dt)
            d_en = oracle._lin(oracle.albert(t_ids, taps), "bert_encoder")
            d = oracle.duration_encoder(d_en, style[None, 128:], taps)
            x = oracle._lstm(d, "predictor.lstm")
            duration = torch.sigmoid(oracle._lin(x, "predictor.duration_proj.linear_layer")).sum(dim=-1) / 1.0
            durs.append(torch.round(duration).clamp(min=1).long().numpy())
    return ids, styles, durs


def test_model_marks_equal_the_oracles_durations_across_chunks(hip_model, ragged_reference):
    """The three ragged utterances as ONE three-chunk request at 8 kHz: every token's mark against the oracle's durations (the
    existing tests compare only the sum of a row's durations)."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    ids, styles, durs = ragged_reference
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations(None)
    word = hk.PACK_PCM16_MONO | hk.PACK_RATE_8000
    bodies, marks, samples = hip_model.infer_requests_marks([list(x) for x in ids], [3], styles=styles, speeds=[1.0], seed=2, fmt=word,
                                                            with_samples=True)
    print("durations per chunk:", [(int(d.min()), int(d.max())) for d in durs])
    np.testing.assert_array_equal(marks[0], V.token_marks(durs, word))
    _check_request(marks[0], durs, word)
    assert int(marks[0][-1]) == samples[0] == bodies[0].shape[0]


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _raw_model_call(model, toks, cpr, rows, fmt, out_marks=True, out_n_marks=True):
    """kx_infer_requests_marks as C callers make it; returns (rc, out pointer value, message)."""
    ids, lens = model._ids_lens(toks)
    cp = np.ascontiguousarray(cpr, dtype=np.int32)
    fm = np.ascontiguousarray(fmt, dtype=np.int32).reshape(-1)
    st = np.ascontiguousarray(rows, dtype=np.float32)
    sp = np.ones(1, dtype=np.float32)
    R = cp.shape[0]
    out, mk = C.c_void_p(0xDEAD0), C.c_void_p()
    nb, ns, nm = np.zeros(max(R, 8), np.int64), np.zeros(max(R, 8), np.int64), np.zeros(max(R, 8), np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = model._lib.kx_infer_requests_marks(model._h, p(ids), ids.shape[1], p(lens), len(toks), p(cp), R, p(st), None, None, 0, p(sp), 1,
                                            5, 0, p(fm), fm.shape[0], C.byref(out), p(nb), p(ns),
                                            C.byref(mk) if out_marks else None, p(nm) if out_n_marks else None)
    if rc == 0:
        model._lib.kx_free_packed(out)
    return rc, out.value, model.last_error() if rc else ""


def test_refusals(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    toks = _chunks()[:3]
    rows = [W.synthetic_voices(1)[0, len(t) - 2, 0] for t in toks]
    hip_model.set_pinned_durations([1])
    try:
        assert _raw_model_call(hip_model, toks, [1, 2], rows, 0)[0] == hk.KX_OK
        for kw in (dict(out_marks=False), dict(out_n_marks=False), dict(out_marks=False, out_n_marks=False)):
            rc, out, msg = _raw_model_call(hip_model, toks, [1, 2], rows, 0, **kw)
            assert (rc, msg) == (hk.KX_ERR_INVALID, NULL_MARKS) and not out, kw
        # everything kx_infer_requests refuses, with its text, and *out stays null
        chunks_text = "infer: chunks_per_request entries must be >= 1 and add up to the batch"
        for cpr, fmt, text in (([1, 2], 5, "infer: unknown output format"), ([1, 2], [0, 5], "infer: unknown output format"),
                               ([1, 2], -1, "infer: unknown output format"), ([1, 2], 0x400, "infer: unknown output sample rate"),
                               ([1, 0, 2], 0, chunks_text), ([1, 1], 0, chunks_text), ([2, 2], 0, chunks_text), ([3, 1], 0, chunks_text),
                               ([1, 2], [0, 1, 2], "infer: requests need 1 or R output formats")):
            rc, out, msg = _raw_model_call(hip_model, toks, cpr, rows, fmt)
            assert (rc, msg) == (hk.KX_ERR_INVALID, text) and not out, (cpr, fmt)
            with pytest.raises(hk.KokoroxHipError) as e:
                hip_model.infer_requests(toks, cpr, styles=rows, fmt=fmt)
            assert e.value.code == hk.KX_ERR_INVALID and str(e.value).endswith(text), (cpr, fmt)
        # the dispatcher's entry
        d = hk.Dispatcher([hip_model], max_batch=4, max_wait_us=0)
        try:
            a = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int64) for t in toks]))
            ln = np.array([len(t) for t in toks], dtype=np.int32)
            st = np.ascontiguousarray(rows, dtype=np.float32)
            p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731

            def raw(fmt, n_chunks=3, marks=True, n_marks=True):
                out, mk, nb, ns, nm = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
                err = C.create_string_buffer(256)
                rc = d._lib.kx_dispatcher_submit_request_marks(d._d, p(a), p(ln), n_chunks, p(st), None, None, 0, 1.0, 5, fmt, C.byref(out),
                                                               C.byref(nb), C.byref(ns), C.byref(mk) if marks else None,
                                                               C.byref(nm) if n_marks else None, err, len(err))
                if rc == 0:
                    d._lib.kx_free_packed(out)
                return rc, out.value, err.value.decode()

            assert raw(0)[0] == hk.KX_OK
            for kw in (dict(marks=False), dict(n_marks=False)):
                rc, out, msg = raw(0, **kw)
                assert (rc, msg) == (hk.KX_ERR_INVALID, NULL_MARKS_DISPATCHER) and not out
            for fmt, n_chunks in ((5, 3), (0x400, 3), (0, 5), (0, 0)):  # ... and what submit_request refuses, with its texts
                rc, out, msg = raw(fmt, n_chunks=n_chunks)
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
        # marks on for 0, 1, 2 (1, 2 and 3 chunks), off for 3, 4, 5, ...: both kinds at every chunk count, mixed in every batch
        specs.append(dict(chunks=chunks, voice=voice, fmt=words[i % len(words)], seed=9100 + i, speed=1.0 + 0.125 * (i % 2),
                          marks=(i // 3) % 2 == 0))
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
    if s["marks"]:
        bodies, marks = model.infer_requests_marks(s["chunks"], [n], **kw)
        return bodies[0], marks[0]
    return model.infer_requests(s["chunks"], [n], **kw)[0], None


def _dispatcher_scenario(model):
    """8 client threads, 16 requests of 1..3 chunks, with and without marks, rates and forms mixed, voices by row / id / mix.
    (Dispatcher.submit_request itself refuses marks that are not 8-byte aligned behind the body, on both paths.)"""
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
                out[i] = d.submit_request(s["chunks"], speed=s["speed"], seed=s["seed"], fmt=s["fmt"], marks=s["marks"], **s["voice"])
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
    for i, s in enumerate(specs):
        body, marks = _alone(model, s)
        if s["marks"]:
            _same(out[i][0], body)
            np.testing.assert_array_equal(out[i][1], marks)
            assert out[i][1].shape[0] == sum(len(c) + 1 for c in s["chunks"]) and out[i][1][0] == 0
        else:
            _same(out[i], body)
    assert st["requests"] == len(specs) and st["batches"] < st["requests"]
    return st


def test_dispatcher_marks_equal_their_solo_runs(hip_model):
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
