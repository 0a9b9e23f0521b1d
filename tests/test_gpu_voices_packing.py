"""GPU: SURVEY 8f ranks 2 and 3 — style rows looked up / mixed on the device from a resident voice table,
and the reference's output forms packed on the device.  Both must equal their host mirrors bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _setup(hip_model):
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    tab = W.synthetic_voices(5)
    names = ["af_sky", "af_nicole", "am_adam", "bf_emma", "jf_alpha"]
    styles = {n: tab[i] for i, n in enumerate(names)}
    hip_model.set_voice_table(tab)
    hip_model.set_utterance_base(0)
    toks = [list(R.synthetic_inputs(1, k, seed=300 + k)[0]) for k in (12, 20, 9)]
    return names, styles, toks


def test_device_style_mix_equals_host_mixer(hip_model):
    from kokorox_amd import voices as V
    names, styles, toks = _setup(hip_model)
    # utterance 0: "af_sky.4+af_nicole.5"; 1: "bf_emma.7+junk+am_adam.3.5" (middle part skipped); 2: "jf_alpha.10"
    vid = [[0, 1, -1], [3, -1, 2], [4, -1, -1]]
    wts = [[4, 5, 0], [7, 0, 3.5], [10, 0, 0]]
    host_styles = [V.mix_styles(styles, "af_sky.4+af_nicole.5", 12)[0],
                   V.mix_styles(styles, "bf_emma.7+junk+am_adam.3.5", 20)[0],
                   V.mix_styles(styles, "jf_alpha.10+zzz", 9)[0]]
    want = hip_model.infer_batch(toks, host_styles, [1.0], seed=5)
    got = hip_model.infer_voices(toks, vid, wts, [1.0], seed=5)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    # single-voice form: a plain copy of row tokens_len (no x1.0)
    one = hip_model.infer_voices(toks[:1], [[1]], [[0.0]], [1.0], seed=5)[0]
    ref = hip_model.infer([toks[0]], V.mix_styles(styles, "af_nicole", 12), 1.0, seed=5)
    np.testing.assert_array_equal(one, ref)
    from kokorox_amd import hip_koko as hk
    with pytest.raises(hk.KokoroxHipError, match="voice id"):
        hip_model.infer_voices(toks[:1], [[99]], [[1.0]])


def test_packed_outputs_match_reference_conversions(hip_model):
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import voices as V
    names, styles, toks = _setup(hip_model)
    st = [V.mix_styles(styles, "af_sky", len(t) - 2)[0] for t in toks]
    mono = hip_model.infer_batch(toks, st, [1.0], seed=8)
    stereo = hip_model.infer_packed(toks, st, [1.0], seed=8, fmt=hk.PACK_F32_STEREO)
    pcm = hip_model.infer_packed(toks, st, [1.0], seed=8, fmt=hk.PACK_PCM16_MONO)
    for m, s2, p in zip(mono, stereo, pcm):
        assert s2.shape == (m.shape[0], 2) and p.dtype == np.int16
        np.testing.assert_array_equal(s2[:, 0], m)          # koko.rs:1239-1246: sample written twice
        np.testing.assert_array_equal(s2[:, 1], m)
        want = np.trunc(np.clip(m, -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)  # websocket lib.rs:701-704
        np.testing.assert_array_equal(p, want)
    # voices + packing together
    both = hip_model.infer_voices(toks[:1], [[0]], [[0.0]], [1.0], seed=8, fmt=hk.PACK_PCM16_MONO)[0]
    np.testing.assert_array_equal(both, pcm[0])


@pytest.fixture(scope="module")
def pinned_rows(hip_model):
    """Six chunks of 3..12 tokens at pinned durations 1, 2, 1, ..: tokens, style rows, voice ids, the f32 rows of kx_infer for
    B = 6 and for the one utterance of B = 1 (computed once, left unchanged), and the frame counts the pin implies."""
    from kokorox_amd import voices as V
    from kokorox_amd import weights as W
    from oracle import kokoro_ref as R
    tab = W.synthetic_voices(4)
    names = ["af_sky", "af_nicole", "am_adam", "bf_emma"]
    styles = {n: tab[i] for i, n in enumerate(names)}
    toks = [list(int(v) for v in R.synthetic_inputs(1, k, seed=500 + k)[0]) for k in (1, 10, 3, 5, 2, 7)]
    rows = [V.mix_styles(styles, names[b % 4], len(t) - 2)[0] for b, t in enumerate(toks)]
    vid = [[b % 4] for b in range(6)]
    frames = [sum([1, 2][t % 2] for t in range(len(tk))) for tk in toks]
    hip_model.set_voice_table(tab)
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations([1, 2])
    try:
        wav = {6: hip_model.infer_batch(toks, rows, [1.0], seed=31), 1: hip_model.infer_batch(toks[1:2], rows[1:2], [1.0], seed=31)}
    finally:
        hip_model.set_pinned_durations(None)
    for w in wav.values():
        for x in w:
            x.setflags(write=False)
    return dict(tab=tab, toks=toks, rows=rows, vid=vid, frames=frames, wav=wav)


@pytest.mark.parametrize("B", [1, 6])
def test_per_utterance_entries_equal_the_mirrors_at_pinned_durations(hip_model, pinned_rows, B):
    """kx_infer_packed in forms 0, 1, 2 and kx_infer_voices in form 2 against the numpy mirrors of kx_infer's rows, exactly;
    out_samples = 600 x the pinned frames.  For B = 6 in form 2 the returned buffer is the rows back to back: the same regions
    as six single-row requests, and one request of the six chunks is their concatenation."""
    from kokorox_amd import hip_koko as hk
    p = pinned_rows
    sel = slice(0, 6) if B == 6 else slice(1, 2)
    toks, rows, vid, frames, wav = p["toks"][sel], p["rows"][sel], p["vid"][sel], p["frames"][sel], p["wav"][B]
    assert [x.shape[0] for x in wav] == [600 * f for f in frames]
    hip_model.set_voice_table(p["tab"])
    hip_model.set_utterance_base(0)
    hip_model.set_pinned_durations([1, 2])
    try:
        got = {f: hip_model.infer_packed(toks, rows, [1.0], seed=31, fmt=f, with_samples=True) for f in (0, 1, 2)}
        voices = hip_model.infer_voices(toks, vid, [[0.0]] * B, [1.0], seed=31, fmt=hk.PACK_PCM16_MONO, with_samples=True)
        for b, x in enumerate(wav):
            pcm = np.trunc(np.clip(x, -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)  # websocket lib.rs:701-704
            np.testing.assert_array_equal(got[0][0][b], x)
            assert got[1][0][b].dtype == np.float32
            np.testing.assert_array_equal(got[1][0][b], np.stack([x, x], axis=1))  # koko.rs:1239-1246
            for res in (got[2][0][b], voices[0][b]):
                assert res.dtype == np.int16
                np.testing.assert_array_equal(res, pcm)
        for res in (*got.values(), voices):
            assert res[1] == [600 * f for f in frames]
        if B == 6:
            single = hip_model.infer_requests(toks, [1] * 6, styles=rows, speeds=[1.0], seed=31, fmt=2)
            for b in range(6):
                assert single[b].dtype == np.int16
                np.testing.assert_array_equal(single[b], got[2][0][b])
            whole = hip_model.infer_requests(toks, [6], styles=rows, speeds=[1.0], seed=31, fmt=2)[0]
            np.testing.assert_array_equal(whole, np.concatenate(got[2][0]))
    finally:
        hip_model.set_pinned_durations(None)
