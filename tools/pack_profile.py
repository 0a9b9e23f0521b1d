"""Three packed calls of the bench batch (64 x 130 tokens, durations pinned 3,3,3,4 -> 422 frames each) in the mode given on
the command line; an optional second argument is the batch (1 = one utterance).  Modes:
    'p0' / 'p1' / 'p2'   kx_infer_packed in form 0 / 1 / 2, 'i' = kx_infer (form 0): the per-utterance entries, single-row
                         requests of pack_requests_kernel (on trees before the two packers became one: the older kernel);
    '2' / '3' / '4'      kx_infer_requests in that form, every row a request of its own (pack_requests_kernel); a format word
                         with a rate code, written as the header does ('0x108' = G.711 mu-law at 8 kHz, '0x303' = float WAV at
                         48 kHz), adds resample_requests_kernel in front of it;
    a word and 'm'       ('2m') kx_infer_requests_marks in that word, which adds token_marks_kernel behind the packer;
    a word and 'j'       ('2j', '0x108j') kx_infer_requests_joined with marks, the batch as BATCH / 4 requests of 4 chunks, every
                         request with the spec {HEAD | TAIL | INNER, keep 20 ms, pause 150 ms, fade 5 ms}: the joined forms of the
                         three kernels (pack_requests_joined_kernel, resample_requests_joined_kernel, token_marks_joined_kernel);
    a word and 'l'       ('2l', '0x108l') kx_infer_requests_levelled, every row a request of its own normalised to a peak of 0.5:
                         request_peak_kernel and request_gain_kernel between resampler and packer, and pack_requests_levelled_kernel;
    a word and 'd'       ('0x300d') kx_infer_requests_loudness, every row a request of its own normalised to -23 LUFS under a peak of 1:
                         request_peak_kernel, request_loudness_kernel and request_loudness_gain_kernel between resampler and packer, and
                         pack_requests_levelled_kernel (no request_gain_kernel: every slot is the loudness gain kernel's);
    'l' or 'd' and 't'   ('0x300lt', '0lt', '0x300dt') the same call with KX_PEAK_TRUE in every spec: request_truepeak_kernel behind the
                         peak pass (the meter) and before the gain kernel; without the 't' no such kernel may show in the stats;
    a word and 'x' / 'y' ('0x300x', '0y', '0x300xt') kx_infer_requests_limited, every row a request of its own: 'x' driven by a gain
                         of 64 and 'y' to -6 LUFS, both into a peak of 2^-6, so the drive cap holds g p at 4 peak and every stretch
                         within 12 dB of a request's peak is limited: request_limit_kernel and request_limit_report_kernel behind
                         the gain kernels, and pack_requests_limited_kernel; with 't' the limiter follows the true-peak envelope;
    '12' / '0x30c'       kx_infer_requests in form 12 (FLAC; '0x30c' = at 48 kHz), every row a request of its own: flac_frames_kernel,
                         flac_layout_kernel and flac_gather_kernel in the packer's place (pack_requests_kernel does not show: no
                         request has a region for it); prints the bodies' bytes beside the PCM16 bytes of the same samples;
    '17' / '0x111'       kx_infer_requests in form 17 (IMA ADPCM in a WAV file; '0x111' = at 8 kHz), every row a request of its own:
                         adpcm_blocks_kernel in the packer's place (pack_requests_kernel does not show); '18' = the 16-bit WAV file,
                         a branch of pack_requests_kernel;
    a word and 'r'       ('2r') kx_infer_requests_prosody with a rate, a pitch and an energy per token and the report, every row a
                         request of its own: prosody_duration_kernel in duration_kernel's place (the pinned pattern still sets the
                         frames) and prosody_curves_kernel behind the F0 / N predictors;
    a word and 'f'       ('2f') kx_infer_requests_fitted, every row a request of its own with one span over all its 130 tokens fitted
                         to 422 frames (what the pinned pattern gives the other modes; a fit refuses a pinned model, so this mode
                         runs without the pattern): fit_weights_kernel and fit_spans_kernel in front of prosody_duration_kernel;
    a word and 'q'       ('0x108q') kx_infer_requests_pieces, every row a one-chunk piece of a request of its own: the first call the
                         FIRST pieces, the second middle pieces with the carries of the first, the third the LAST pieces:
                         resample_pieces_kernel in the resampler's place and piece_carry_kernel behind it, the packer as ever;
    a word and 'g'       ('2g') the same grouping without joins (kx_infer_requests_marks): the plain kernels on the same batch.
Meant to run under the profiler, one mode per run (kernel trace only, no counters in the same run):
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python tools/pack_profile.py p2
profiles/pack_kernels_stats.txt holds the rows of the kernel_stats.csv files."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa
from kokorox_amd import hip_koko as hk, weights as W
from oracle import kokoro_ref as R
which = sys.argv[1]
flag = hk.PEAK_TRUE if which.endswith("t") and which[-2:-1] in ("l", "d", "x", "y") else 0
which = which[:-1] if flag else which
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
m = hk.HipKoko.new(W.ensure_synthetic_blob())
toks = [list(int(v) for v in R.synthetic_inputs(1, 128, seed=40 + b)[0]) for b in range(B)]
rows = [W.synthetic_voices(1)[0, 128, 0]] * B
if not which.endswith("f"):
    m.set_pinned_durations([3, 3, 3, 4])
for it in range(3):
    if which == "i":
        out = m.infer_batch(toks, rows, [1.0])
    elif which in ("p0", "p1", "p2"):
        out = m.infer_packed(toks, rows, fmt=int(which[1]))
    elif which[-1] in "jg":
        word = int(which[:-1], 0)
        L, M, _ = hk.resample_filter(word)
        if which[-1] == "j":
            join = (hk.JOIN_TRIM_HEAD | hk.JOIN_TRIM_TAIL | hk.JOIN_TRIM_INNER, 20, 150, 5)
            out, marks = m.infer_requests_joined(toks, [4] * (B // 4), join, styles=rows, fmt=word, marks=True)
            # per chunk 422 frames less its two 3-frame pads but for 20 ms of each; three pauses of 150 ms per request
            assert all(int(k[-1]) == (4 * (422 * 600 - 2 * (1800 - 480)) + 3 * 3600) * L // M for k in marks)
        else:
            out, marks = m.infer_requests_marks(toks, [4] * (B // 4), styles=rows, fmt=word)
            assert all(int(k[-1]) == 4 * 422 * 600 * L // M for k in marks)
        assert all(k.shape[0] == 4 * 131 for k in marks)
    elif which.endswith("l"):
        word = int(which[:-1], 0)
        out, lv = m.infer_requests_levelled(toks, [1] * B, (hk.LEVEL_NORMALIZE | flag, 1.0, 0.5), styles=rows, fmt=word)
        assert lv.shape == (B, 2) and (lv[:, 0] > 0).all() and np.array_equal((lv[:, 0] * lv[:, 1]).astype(np.float32), np.full(B, 0.5, np.float32))
    elif which.endswith("d"):
        word = int(which[:-1], 0)
        out, ld = m.infer_requests_loudness(toks, [1] * B, (hk.LOUDNESS_NORMALIZE | flag, -23.0, 1.0), styles=rows, fmt=word)
        assert ld.shape == (B, 4) and (ld[:, 3] >= 1).all() and np.isfinite(ld[:, 2]).all()
        if it == 2:
            print("loudness of the first request: p %.6g g %.6g I %.6f LUFS n_g %d" % tuple(ld[0]))
    elif which[-1] in "xy":
        word = int(which[:-1], 0)
        spec = (hk.LIMIT_GAIN | flag, 64.0, 0.0, 2.0 ** -6) if which[-1] == "x" else (hk.LIMIT_LOUDNESS | flag, 1.0, -6.0, 2.0 ** -6)
        out, lm = m.infer_requests_limited(toks, [1] * B, spec, styles=rows, fmt=word)
        assert lm.shape == (B, 5) and (lm[:, 4] < 1.0).all() and (lm[:, 4] > 0.24).all()
        if it == 2:
            print("limits of the first request: p %.6g g %.6g I %.6f LUFS n_g %d r %.6g" % tuple(lm[0]))
    elif which.endswith("r"):
        word = int(which[:-1], 0)
        rng = np.random.default_rng(it)
        pros = tuple([rng.choice(vals, size=len(t)).astype(np.float32) for t in toks] for vals in ([0.8, 1.0, 1.25], [0.7, 1.0, 1.4], [0.5, 1.0, 1.5]))
        out, rep = m.infer_requests_prosody(toks, [1] * B, (pros[0], None, pros[1], pros[2]), styles=rows, fmt=word)
        assert all(k.shape == (130, 4) and int(k[:, 3].sum()) == 422 for k in rep)
        if it == 2:
            print("report of the first request: mean voiced F0 %.3f Hz over %d steps" % (float((rep[0][:, 0] * rep[0][:, 1]).sum() / max(rep[0][:, 1].sum(), 1)), int(rep[0][:, 1].sum())))
    elif which.endswith("f"):
        word = int(which[:-1], 0)
        out, fit, ns = m.infer_requests_fitted(toks, [1] * B, [(b, 0, len(toks[b]), 422) for b in range(B)], styles=rows, fmt=word, with_samples=True)
        L, M, _ = hk.resample_filter(word)
        assert all(int(k) == 422 * 600 * L // M for k in ns) and all(int(f["n_free"]) == 130 for f in fit)
        if it == 2:
            print("fit of the first request: lambda %.6f, excess %d" % (float(fit[0]["lambda"]), int(fit[0]["excess"])))
    elif which.endswith("q"):
        word = int(which[:-1], 0)
        L, M, _ = hk.resample_filter(word)
        out, carries, ns = m.infer_requests_pieces(toks, [1] * B, [[hk.PIECE_FIRST, 0, hk.PIECE_LAST][it]] * B, carries if it else None,
                                                   styles=rows, fmt=word, with_samples=True)
        assert (carries["src_samples"] == 422 * 600 * (it + 1)).all() and (carries["reserved"] == it + 1).all()
        assert it < 2 or (carries["out_samples"] == 3 * 422 * 600 * L // M).all()
        print("call", it, "samples of the first piece", ns[0], "of", 422 * 600 * L // M, "a chunk")
    elif which.endswith("m"):
        word = int(which[:-1], 0)
        out, marks = m.infer_requests_marks(toks, [1] * B, styles=rows, fmt=word)
        L, M, _ = hk.resample_filter(word)
        assert all(k.shape[0] == 131 and int(k[-1]) == 422 * 600 * L // M for k in marks)
    elif int(which, 0) & 0xFF == hk.PACK_FLAC:
        out, ns = m.infer_requests(toks, [1] * B, styles=rows, fmt=int(which, 0), with_samples=True)
        assert all(o[:4] == b"fLaC" and len(o) % 4 == 0 for o in out)
        if it == 2:
            print("FLAC bytes %d, PCM16 bytes of the same samples %d: ratio %.4f" % (sum(len(o) for o in out), 2 * sum(ns), sum(len(o) for o in out) / (2.0 * sum(ns))))
    elif int(which, 0) & 0xFF == hk.PACK_ADPCM_WAV:
        out, ns = m.infer_requests(toks, [1] * B, styles=rows, fmt=int(which, 0), with_samples=True)
        A, P = hk.adpcm_block(int(which, 0))
        assert all(o[:4] == b"RIFF" and len(o) == 60 + A * -(-n // P) for o, n in zip(out, ns))
        if it == 2:
            print("ADPCM bytes %d, PCM16 bytes of the same samples %d: ratio %.4f" % (sum(len(o) for o in out), 2 * sum(ns), sum(len(o) for o in out) / (2.0 * sum(ns))))
    else:
        out = m.infer_requests(toks, [1] * B, styles=rows, fmt=int(which, 0))
    n = sum(len(o) if isinstance(o, bytes) else o.nbytes for o in out)
print("mode", which + ("t" if flag else ""), "batch", B, "bytes", n, "frames", len(toks[0]))
m.close()
