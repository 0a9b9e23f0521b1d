"""Caller-side producers of the hot path's inputs, mirrored from the reference so that
tests and the harness build `infer` arguments exactly as `TTSKoko` does.

Reference (paths under /root/reference/kokorox/src/tts/):
  * `TTSKoko::mix_styles`   koko.rs:1255-1306  — style row lookup and the "a.4+b.5" blend
  * `TTSKoko::load_voices`  koko.rs:1308-1334  — NPZ -> {name: [511][1][256]}
  * `tokenize_with_variant` tokenize.rs:35-67  — char -> id, unknown chars dropped
  * padding                 koko.rs:1161-1175  — optional id-30 prefix, 0 at both ends
  * chunk loop              koko.rs:947-1191   — one forward per <= 500-token chunk, waveforms appended
  * float WAV body          utils/wav.rs:18-50, kokorox-openai/src/lib.rs:416-425  — `wav_f32_body`
  * base64 16-bit WAV       kokorox-websocket/src/lib.rs:696-736 (`encode_audio`)   — `wav16_base64`
Beyond the reference: `resample_stream`, `mulaw_bytes`, `alaw_bytes` mirror the output rates and the G.711 forms of the
request packer (include/kokorox_hip.h, KX_PACK_RATE_*, KX_PACK_MULAW / KX_PACK_ALAW).
These stay on the host (north_star: "the voice-style mixer ... stay identical"); the GPU
only ever sees ids and one 256-float row per utterance.
"""
from __future__ import annotations

import base64
import os
import re
import struct
from typing import Dict, List, Sequence

import numpy as np

VOICE_ROWS = 511


def load_voices(path: str) -> Dict[str, np.ndarray]:
    """NPZ of per-voice arrays [rows<=511, 1, 256] -> zero-padded [511, 1, 256] float32."""
    out: Dict[str, np.ndarray] = {}
    with np.load(path) as npz:
        for name in npz.files:
            a = np.asarray(npz[name], dtype=np.float32)
            t = np.zeros((VOICE_ROWS, 1, 256), dtype=np.float32)
            r = min(a.shape[0], VOICE_ROWS)
            t[:r, : a.shape[1], : a.shape[2]] = a[:r, :1, :256]
            out[name] = t
    return out


def mix_styles(styles: Dict[str, np.ndarray], style_name: str, tokens_len: int) -> List[List[float]]:
    """[[256 floats]] for `style_name` at row `tokens_len` (token count BEFORE the 0 padding).

    A mix "a.4+b.5" is sum(row * (weight * 0.1)) with NO normalisation; parts without '.' or
    with a non-numeric weight are silently skipped; an unknown voice is an error."""
    if "+" not in style_name:
        if style_name not in styles:
            raise KeyError(f"can not found from styles_map: {style_name}")
        return [np.asarray(styles[style_name][tokens_len][0], dtype=np.float32).tolist()]
    names, portions = [], []
    for part in style_name.split("+"):
        if "." not in part:
            continue
        name, portion = part.split(".", 1)
        try:
            p = np.float32(float(portion))
        except ValueError:
            continue
        if name not in styles:
            raise KeyError(f"Voice '{name}' not found in available voices")
        names.append(name)
        portions.append(np.float32(p * np.float32(0.1)))
    if not names:
        raise ValueError(f"Invalid voice mix format '{style_name}'. Use format: voice1.weight+voice2.weight "
                         "(e.g., jf_alpha.4+am_echo.6)")
    blended = np.zeros(256, dtype=np.float32)
    for name, p in zip(names, portions):
        blended = (blended + np.asarray(styles[name][tokens_len][0], dtype=np.float32) * p).astype(np.float32)
    return [blended.tolist()]


def tokenize(phonemes: str, symbols: Sequence[str]) -> List[int]:
    """char -> index in the symbol table; unknown characters are dropped (tokenize.rs:43-55).

    A symbol that occurs twice (the apostrophe, ids 174 and 176 in the v1.0 table) maps to
    its LAST index here; the reference's HashMap makes that choice order-dependent."""
    table = {c: i for i, c in enumerate(symbols)}
    return [table[c] for c in phonemes if c in table]


def pad_tokens(tokens: Sequence[int], initial_silence: int = 0) -> List[List[int]]:
    """koko.rs:1161-1175: optional id-30 prefix, then 0 at both ends, as a batch of one."""
    t = [30] * int(initial_silence) + list(tokens)
    return [[0] + t + [0]]


def tts_chunks(model, styles: Dict[str, np.ndarray], style_name: str, chunk_tokens: Sequence[Sequence[int]],
               speed: float = 1.0, initial_silence: int = 0, seed: int = 0) -> np.ndarray:
    """Mirror of the chunk loop of `TTSKoko::tts_raw_audio` (koko.rs:947-1191) from the point
    where a chunk has been tokenised: per chunk the optional id-30 prefix, `mix_styles(style, tokens.len())` (the
    style row depends on the chunk's own token count, koko.rs:1165), zero padding at both ends, one forward, and
    the waveforms appended one after the other with no cross-fade (koko.rs:1177-1180).

    The reference runs the chunks one by one through its single `Mutex<Session>`; chunks are independent, so here
    they form ONE batched forward (`model.infer_batch`), which on the GPU gives the same samples as chunk-by-chunk
    calls (utterance b of a batch draws its noise from key (seed, b): tests/test_gpu_forward.py).  An empty chunk
    list gives an empty waveform; an empty chunk is an error, as `OrtKoko::infer` would index past the end
    (ort_koko.rs:56)."""
    toks, rows = [], []
    for ch in chunk_tokens:
        t = [30] * int(initial_silence) + [int(v) for v in ch]
        if not t:
            raise ValueError("tts_chunks: empty chunk")
        rows.append(mix_styles(styles, style_name, len(t))[0])
        toks.append([0] + t + [0])
    if not toks:
        return np.zeros(0, dtype=np.float32)
    outs = model.infer_batch(toks, np.asarray(rows, dtype=np.float32), [float(speed)], seed=seed)
    return np.concatenate([np.asarray(o, dtype=np.float32) for o in outs])


SAMPLE_RATE = 24000


def wav_f32_body(samples, rate: int = SAMPLE_RATE) -> bytes:
    """The HTTP body of kokorox-openai/src/lib.rs:416-425: the 44 bytes of `WavHeader::new(1, 24000, 32).write_header`
    (utils/wav.rs:18-50: IEEE float, both size fields the reference's 0xFFFFFFFF placeholders), then `to_le_bytes` of
    every sample: bit copies, a NaN keeps its payload.  `rate`: the header's sample rate (the samples are taken as given)."""
    s = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 0xFFFFFFFF, b"WAVE", b"fmt ", 16, 3, 1, rate, rate * 4, 4, 32,
                      b"data", 0xFFFFFFFF)
    return hdr + s.astype("<f4", copy=False).tobytes()


def pcm16(samples) -> np.ndarray:
    """`(s.clamp(-1.0, 1.0) * 32767.0) as i16` with Rust's meaning: clamp keeps a NaN and the cast turns it into 0, +-inf
    clamp to +-1, the product is rounded to f32 and then truncated toward zero."""
    s = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    nan = np.isnan(s)
    c = np.clip(np.where(nan, np.float32(0), s), np.float32(-1.0), np.float32(1.0)).astype(np.float32)
    return np.trunc(c * np.float32(32767.0)).astype(np.int16)


def wav16_base64(samples, rate: int = SAMPLE_RATE) -> bytes:
    """The WebSocket chunk of `encode_audio` (kokorox-websocket/src/lib.rs:696-736): standard base64 (`=` padding, no line
    breaks) of a 16-bit mono WAV file at 24 kHz (or `rate`: the header's, the samples are taken as given), header with its
    true sizes, samples through `pcm16`."""
    pcm = pcm16(samples)
    n = 2 * pcm.shape[0]
    if 36 + n > 0xFFFFFFFF:
        raise ValueError("wav16_base64: a 16-bit WAV file cannot hold that many samples")
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + n, b"WAVE", b"fmt ", 16, 1, 1, rate, rate * 2, 2, 16,
                      b"data", n)
    return base64.b64encode(hdr + pcm.astype("<i2", copy=False).tobytes())


def resample_stream(x, word: int) -> np.ndarray:
    """A request's stream at the output rate of a format word, as resample_requests_kernel computes it (include/kokorox_hip.h):
    with (L, M) and the float32 taps h of the word's rate code from the library's table (N = 2 C + 1 of them),
        y[n] = f32(sum over j ascending, 0 <= j < S, 0 <= n M - j L + C < N, of f64(h[n M - j L + C]) * f64(x[j])),
    a float64 accumulator from +0, one addition per term, one rounding at the end.  The products are exact in float64, so
    this loop -- the k-th term of every output at once -- gives the GPU's bits.  Rate code 0 returns the stream as it is."""
    from . import hip_koko as hk
    x32 = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    L, M, h32 = hk.resample_filter(word)
    if h32.shape[0] == 0:
        return x32
    S, N = x32.shape[0], h32.shape[0]
    C = (N - 1) // 2
    if (S * L) % M:
        raise ValueError("resample_stream: the stream's length must give a whole number of output samples")
    h, xd = h32.astype(np.float64), x32.astype(np.float64)
    n = np.arange(S * L // M, dtype=np.int64)
    a = n * M - C
    jl = np.where(a <= 0, 0, (a + L - 1) // L)      # first j with n M - j L + C <= N - 1, inside the stream
    jh = np.minimum((n * M + C) // L, S - 1)        # last j with n M - j L + C >= 0, inside the stream
    acc = np.zeros(n.shape[0], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int((jh - jl).max()) + 1 if n.shape[0] else 0):
            j = jl + k
            live = j <= jh
            jj = np.where(live, j, 0)
            acc = np.where(live, acc + h[np.where(live, n * M - jj * L + C, 0)] * xd[jj], acc)
        return acc.astype(np.float32)


def mulaw_bytes(pcm) -> np.ndarray:
    """G.711 mu-law of 16-bit samples: the 16-bit-input algorithm of CPython's `audioop.lin2ulaw(_, 2)` (form 8)."""
    v = np.asarray(pcm).astype(np.int32).reshape(-1)
    p = v >> 2
    mask = np.where(p < 0, 0x7F, 0xFF)
    p = np.minimum(np.abs(p), 8159) + 33
    seg = np.zeros_like(p)
    for k in range(8):  # the first segment end 0x3F, 0x7F .. 0x1FFF that holds p; 8 = none
        seg += p > (0x40 << k) - 1
    byte = np.where(seg >= 8, 0x7F, (seg << 4) | ((p >> (seg + 1)) & 15)) ^ mask
    return byte.astype(np.uint8)


def alaw_bytes(pcm) -> np.ndarray:
    """G.711 A-law of 16-bit samples: the 16-bit-input algorithm of CPython's `audioop.lin2alaw(_, 2)` (form 9)."""
    v = np.asarray(pcm).astype(np.int32).reshape(-1)
    mask = np.where(v >= 0, 0xD5, 0x55)
    p = np.where(v >= 0, v, -v - 1) >> 3
    seg = np.zeros_like(p)
    for k in range(7):  # the first segment end 0x1F, 0x3F .. 0xFFF that holds p (p <= 0xFFF)
        seg += p > (0x20 << k) - 1
    byte = ((seg << 4) | ((p >> np.where(seg < 2, 1, seg)) & 15)) ^ mask
    return byte.astype(np.uint8)


# ---- FLAC (form 12; include/kokorox_hip.h, "FLAC"): one mono 16-bit stream in fixed blocks of 4096, every choice fixed by rule ----
FLAC_BLOCK = 4096
_FLAC_RATE_NIBBLE = {8000: 0b0100, 16000: 0b0101, 24000: 0b0111, 48000: 0b1010}
_FLAC_FIXED = ((1,), (1, -1), (1, -2, 1), (1, -3, 3, -1), (1, -4, 6, -4, 1))  # e_o = sum over j of c[j] v[i - j]


def flac_crc8(data) -> int:
    """CRC-8 of a frame header: polynomial 0x07, initial value 0, MSB first, no final XOR."""
    c = 0
    for b in bytes(data):
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def _flac_crc16_table():
    t = np.arange(256, dtype=np.uint32) << 8
    for _ in range(8):
        t = np.where(t & 0x8000, (t << 1) ^ 0x8005, t << 1) & 0xFFFF
    return [int(v) for v in t]


_FLAC_CRC16 = _flac_crc16_table()


def flac_crc16(data) -> int:
    """CRC-16 of a whole frame: polynomial 0x8005, initial value 0, MSB first, not reflected, no final XOR."""
    c = 0
    for b in bytes(data):
        c = ((c << 8) & 0xFFFF) ^ _FLAC_CRC16[(c >> 8) ^ b]
    return c


def flac_bound(n_samples: int) -> int:
    """Bytes a body of n_samples samples never exceeds: 42 + 7 + the sum over its frames of 16 + 2 n, rounded up to 4."""
    n, frames = int(n_samples), (int(n_samples) + FLAC_BLOCK - 1) // FLAC_BLOCK
    return (49 + 16 * frames + 2 * n + 3) & ~3


def _flac_number(f: int) -> bytes:
    """The frame number in the format's UTF-8-like coding (up to 36 bits; seven bits in one byte)."""
    if f < 0x80:
        return bytes([f])
    n = 2
    while f >> (5 * n + 1):  # n bytes hold 7 - n + 6 (n - 1) = 5 n + 1 bits
        n += 1
    lead = (0xFF << (8 - n)) & 0xFF
    return bytes([lead | (f >> (6 * (n - 1)))] + [0x80 | ((f >> (6 * k)) & 0x3F) for k in range(n - 2, -1, -1)])


def _flac_fold(e):
    return (e << 1) ^ (e >> 31)  # int64 here: the same value as in int32, |e| < 2^20


def _flac_partitions(u, o, n, P):
    """(ks, bits) of order o at partition order P: u = the folded residuals of samples o .. n - 1."""
    size, ks, bits, lo = n >> P, [], 0, 0
    for j in range(1 << P):
        hi = lo + size - (o if j == 0 else 0)
        part = u[lo:hi]
        cost = [int((part >> k).sum()) + (k + 1) * (hi - lo) for k in range(15)]
        k = int(np.argmin(cost))  # (the first minimum: the smaller k wins a tie)
        ks.append(k)
        bits += 4 + cost[k]
        lo = hi
    return ks, 16 * o + 6 + bits


def flac_frame(v, f: int, rate: int):
    """Frame f of a stream: `v` = its n <= 4096 samples (int16).  Returns (bytes, (type, o, P, ks)) with type "CONSTANT", "FIXED" or
    "VERBATIM" (o, P = 0 and ks = () where the type has none): the subframe include/kokorox_hip.h prescribes -- CONSTANT when all
    samples are equal; else the fixed predictor order o in 0..min(4, n - 1) and the partition order P (0..6 when n = 4096, else 0)
    with the fewest bits, Rice parameters 0..14 per partition by the same rule, ties to the smaller o, then P, then k; VERBATIM
    when that reaches 16 n bits."""
    v = np.asarray(v).astype(np.int64).reshape(-1)
    n = v.shape[0]
    if not 1 <= n <= FLAC_BLOCK or np.any(v < -32768) or np.any(v > 32767):
        raise ValueError("flac_frame: 1..4096 samples of 16 bits")
    head = bytes([0xFF, 0xF8, ((0b1100 if n == FLAC_BLOCK else 0b0111) << 4) | _FLAC_RATE_NIBBLE[int(rate)], 0x08]) + _flac_number(int(f))
    if n != FLAC_BLOCK:
        head += struct.pack(">H", n - 1)
    head += bytes([flac_crc8(head)])
    bits = []  # (value, width) pairs, MSB first

    def put(value, width):
        bits.append((int(value) & ((1 << width) - 1), width))

    choice = ("CONSTANT", 0, 0, ())
    if np.all(v == v[0]):
        put(0x00, 8)
        put(v[0], 16)
    else:
        best = None
        for o in range(min(4, n - 1) + 1):
            e = sum(c * v[o - j: n - j] for j, c in enumerate(_FLAC_FIXED[o]))
            u = _flac_fold(e)
            for P in range(7 if n == FLAC_BLOCK else 1):
                ks, total = _flac_partitions(u, o, n, P)
                if best is None or total < best[0]:
                    best = (total, o, P, ks, u)
        total, o, P, ks, u = best
        if total >= 16 * n:
            choice = ("VERBATIM", 0, 0, ())
            put(0x02, 8)
            for s in v:
                put(s, 16)
        else:
            choice = ("FIXED", o, P, tuple(ks))
            put((8 + o) << 1, 8)
            for s in v[:o]:
                put(s, 16)
            put(0, 2)
            put(P, 4)
            size, lo = n >> P, 0
            for j, k in enumerate(ks):
                hi = lo + size - (o if j == 0 else 0)
                put(k, 4)
                for x in u[lo:hi]:
                    x = int(x)
                    put(0, x >> k)
                    put((1 << k) | (x & ((1 << k) - 1)), k + 1)
                lo = hi
    acc, width = 0, 0
    for value, w in bits:
        acc, width = (acc << w) | value, width + w
    pad = -width % 8
    body = head + ((acc << pad).to_bytes((width + pad) // 8, "big") if width else b"")
    return body + struct.pack(">H", flac_crc16(body)), choice


def flac_body(v_int16, rate: int) -> bytes:
    """Form 12: "fLaC", STREAMINFO (blocks of 4096, the frames' true smallest and largest size, `rate`, 1 channel, 16 bits, N samples,
    no MD5), a PADDING block of (2 - the frames' bytes) mod 4 zeros, marked last, and the frames: a multiple of 4 bytes."""
    v = np.asarray(v_int16).astype(np.int64).reshape(-1)
    N = v.shape[0]
    frames = [flac_frame(v[i: i + FLAC_BLOCK], i // FLAC_BLOCK, rate)[0] for i in range(0, N, FLAC_BLOCK)]
    sizes = [len(fr) for fr in frames]
    lo, hi = (min(sizes), max(sizes)) if sizes else (0, 0)
    info = struct.pack(">HH", FLAC_BLOCK, FLAC_BLOCK) + lo.to_bytes(3, "big") + hi.to_bytes(3, "big")
    info += ((int(rate) << 44) | (0 << 41) | (15 << 36) | N).to_bytes(8, "big") + bytes(16)
    p = (2 - sum(sizes)) % 4
    return b"fLaC" + bytes([0x00, 0, 0, 34]) + info + bytes([0x81, 0, 0, p]) + bytes(p) + b"".join(frames)


# ---- IMA ADPCM in a WAV file and the 16-bit WAV file (forms 17 and 18; include/kokorox_hip.h, "IMA ADPCM") ----------------------
ADPCM_INDEX_STEPS = (-1, -1, -1, -1, 2, 4, 6, 8)
ADPCM_START_DIFFS = 8  # a block's start index looks at its first so many differences (KX_ADPCM_START_DIFFS of adpcm_steps.h)
ADPCM_BLOCK_BYTES = {8000: 256, 16000: 512, 24000: 512, 48000: 1024}  # A by rate; a block holds P = 1 + 2 (A - 4) samples


def adpcm_steps() -> np.ndarray:
    """The 89 steps, from the one table the kernel and the host are compiled with (kokorox_amd/csrc/adpcm_steps.h)."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "adpcm_steps.h"), encoding="utf-8").read()
    body = re.search(r"#define KX_ADPCM_STEPS((?:.*\\\n)*.*)\n", text).group(1)
    steps = np.array([int(v) for v in re.findall(r"\d+", body)], dtype=np.int64)
    if steps.shape[0] != 89:
        raise ValueError("adpcm_steps: adpcm_steps.h does not hold 89 steps")
    return steps


def adpcm_blocks(v_int16, rate: int) -> np.ndarray:
    """The F = ceil(N / P) blocks of form 17 as uint8 [F, A]: every block the int16 predictor (its first sample), the start index
    i0 = the smallest i with STEP[i] >= the largest of |v[t + 1] - v[t]|, t = 0..7, over the block's own samples (88 when none; the
    samples past N repeat v[N - 1]), a zero byte, and the codes of its other P - 1 samples by the standard IMA / DVI step, two a byte, the earlier one
    in the low nibble.  All blocks advance together, one sample per pass: a block depends on nothing outside it."""
    v = np.asarray(v_int16).astype(np.int64).reshape(-1)
    A = ADPCM_BLOCK_BYTES[int(rate)]
    P = 1 + 2 * (A - 4)
    N = v.shape[0]
    F = (N + P - 1) // P
    out = np.zeros((F, A), dtype=np.uint8)
    if F == 0:
        return out
    steps = adpcm_steps()
    x = np.concatenate([v, np.full(F * P - N, v[-1], dtype=np.int64)]).reshape(F, P)
    pred = x[:, 0].copy()
    index = np.minimum(np.searchsorted(steps, np.abs(np.diff(x[:, : ADPCM_START_DIFFS + 1], axis=1)).max(axis=1), side="left"), 88)
    out[:, 0:2] = pred.astype("<i2").view(np.uint8).reshape(F, 2)
    out[:, 2] = index
    table = np.asarray(ADPCM_INDEX_STEPS, dtype=np.int64)
    codes = np.zeros((F, P - 1), dtype=np.int64)
    for t in range(1, P):
        step = steps[index]
        d = x[:, t] - pred
        sign = d < 0
        d = np.abs(d)
        code = np.zeros(F, dtype=np.int64)
        vp = step >> 3
        for bit, shift in ((4, 0), (2, 1), (1, 2)):
            s = step >> shift
            take = d >= s
            code |= np.where(take, bit, 0)
            d = np.where(take, d - s, d)
            vp = np.where(take, vp + s, vp)
        pred = np.clip(np.where(sign, pred - vp, pred + vp), -32768, 32767)
        index = np.clip(index + table[code], 0, 88)
        codes[:, t - 1] = code | np.where(sign, 8, 0)
    out[:, 4:] = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    return out


def adpcm_wav_body(v_int16, rate: int) -> bytes:
    """Form 17: the 60-byte header (RIFF, fmt of 20 bytes with tag 0x11, fact = N, data) and the blocks of `adpcm_blocks`."""
    v = np.asarray(v_int16).reshape(-1)
    A = ADPCM_BLOCK_BYTES[int(rate)]
    P = 1 + 2 * (A - 4)
    N = v.shape[0]
    F = (N + P - 1) // P
    if N > 0xFFFFFFFF or 52 + A * F > 0xFFFFFFFF:
        raise ValueError("adpcm_wav_body: an ADPCM WAV file cannot hold that many samples")
    hdr = struct.pack("<4sI4s4sIHHIIHHHH4sII4sI", b"RIFF", 52 + A * F, b"WAVE", b"fmt ", 20, 0x11, 1, rate, rate * A // P, A, 4, 2, P,
                      b"fact", 4, N, b"data", A * F)
    return hdr + adpcm_blocks(v, rate).tobytes()


def adpcm_wav_decode(body: bytes):
    """(int16 samples, rate) of a form-17 body: the header read field by field, every block decoded from its own header state by
    the standard step (the inverse of `adpcm_blocks`: the decoder follows the encoder's predictor exactly), cut to the N of the
    fact chunk.  Raises ValueError for anything that is not this project's layout."""
    if len(body) < 60:
        raise ValueError("adpcm_wav_decode: shorter than the header")
    (riff, size, wave, fmt_, fmt_size, tag, ch, rate, bps, A, bits, cb, P, fact, fact_size, N, data, n_data) = struct.unpack(
        "<4sI4s4sIHHIIHHHH4sII4sI", body[:60])
    ok = (riff, wave, fmt_, fact, data) == (b"RIFF", b"WAVE", b"fmt ", b"fact", b"data") and (fmt_size, tag, ch, bits, cb, fact_size) == (20, 0x11, 1, 4, 2, 4)
    ok = ok and A >= 8 and P == 1 + 2 * (A - 4) and bps == rate * A // P and n_data % A == 0 and size == 52 + n_data and len(body) == 60 + n_data
    F = n_data // A if ok else 0
    if not ok or F != (N + P - 1) // P:
        raise ValueError("adpcm_wav_decode: not an IMA ADPCM WAV body of this layout")
    blocks = np.frombuffer(body, dtype=np.uint8, offset=60).reshape(F, A).astype(np.int64)
    if F and (blocks[:, 2].max() > 88 or blocks[:, 3].any()):
        raise ValueError("adpcm_wav_decode: bad block header")
    steps = adpcm_steps()
    table = np.asarray(ADPCM_INDEX_STEPS, dtype=np.int64)
    out = np.zeros((F, P), dtype=np.int64)
    pred = blocks[:, 0:2].astype(np.uint8).reshape(-1).view("<i2").astype(np.int64)
    index = blocks[:, 2].copy()
    out[:, 0] = pred
    codes = np.empty((F, P - 1), dtype=np.int64)
    codes[:, 0::2] = blocks[:, 4:] & 15
    codes[:, 1::2] = blocks[:, 4:] >> 4
    for t in range(1, P):
        step = steps[index]
        c = codes[:, t - 1]
        vp = (step >> 3) + np.where(c & 4, step, 0) + np.where(c & 2, step >> 1, 0) + np.where(c & 1, step >> 2, 0)
        pred = np.clip(np.where(c & 8, pred - vp, pred + vp), -32768, 32767)
        index = np.clip(index + table[c & 7], 0, 88)
        out[:, t] = pred
    return out.reshape(-1)[:N].astype(np.int16), int(rate)


def wav16_body(samples, rate: int = SAMPLE_RATE) -> bytes:
    """Form 18, the file itself: the bytes `wav16_base64` encodes -- the 44-byte header with its true sizes and the samples
    through `pcm16`; 44 + 2 N bytes.  (A request's region holds it padded with zero bytes to a multiple of 4: `stream_body`.)"""
    return base64.b64decode(wav16_base64(samples, rate))


_RATE_LM = {0: (1, 1), 1: (1, 3), 2: (2, 3), 3: (2, 1)}  # rate code of a format word -> (L, M): 24 000, 8000, 16 000, 48 000 Hz


def token_marks(durations_per_chunk: Sequence[Sequence[int]], word: int = 0) -> np.ndarray:
    """The token marks of ONE request (the definition of include/kokorox_hip.h, "token marks", in numpy int64):
    `durations_per_chunk[c][t]` = frames the forward used for token t of chunk c (the two 0 pads included), `word` the request's
    format word (only its rate code matters).  With K = 600 L / M, chunk after chunk T_c + 1 values
        m_c[t] = K * (frames of the chunks before c + sum of d_c[t'] for t' < t),   t = 0 .. T_c;
    token t of chunk c occupies the output samples [m_c[t], m_c[t + 1]) of the request's stream, the last value is the
    request's sample count."""
    code = (int(word) >> 8) & 15
    if code not in _RATE_LM or not durations_per_chunk:
        raise ValueError("token_marks: unknown output sample rate, or a request without chunks")
    L, M = _RATE_LM[code]
    K = 600 * L // M
    out, base = [], 0
    for d in durations_per_chunk:
        d = np.asarray(d, dtype=np.int64).reshape(-1)
        if d.shape[0] < 1:
            raise ValueError("token_marks: empty chunk")
        out.append(K * (base + np.concatenate([np.zeros(1, np.int64), np.cumsum(d, dtype=np.int64)])))
        base += int(d.sum())
    return np.concatenate(out).astype(np.int64)


JOIN_TRIM_HEAD, JOIN_TRIM_TAIL, JOIN_TRIM_INNER = 1, 2, 4


def _join_fields(join):
    flags, keep_ms, pause_ms, fade_ms = (int(v) for v in (join if join is not None else (0, 0, 0, 0)))
    if flags & ~7 or not (0 <= keep_ms <= 1000 and 0 <= pause_ms <= 5000 and 0 <= fade_ms <= 12):
        raise ValueError("join: flags 0..7, keep_ms 0..1000, pause_ms 0..5000, fade_ms 0..12")
    return flags, keep_ms, pause_ms, fade_ms


def join_rows(durations_per_chunk: Sequence[Sequence[int]], join):
    """Per chunk of ONE request (skip, keep, gap, fade at the head, fade at the tail) in samples at 24 kHz, by the definition of
    include/kokorox_hip.h, "joins": `join` = (flags, keep_ms, pause_ms, fade_ms).  A head edge is selected when the chunk has at
    least 3 tokens and is the request's first with JOIN_TRIM_HEAD or a later one with JOIN_TRIM_INNER; a tail edge symmetrically
    with JOIN_TRIM_TAIL / JOIN_TRIM_INNER; of a selected pad span at most 24 keep_ms samples stay."""
    flags, keep_ms, pause_ms, fade_ms = _join_fields(join)
    n, rows = len(durations_per_chunk), []
    for c, d in enumerate(durations_per_chunk):
        d = [int(v) for v in np.asarray(d).reshape(-1)]
        if not d:
            raise ValueError("join_rows: empty chunk")
        head = len(d) >= 3 and bool(flags & (JOIN_TRIM_HEAD if c == 0 else JOIN_TRIM_INNER))
        tail = len(d) >= 3 and bool(flags & (JOIN_TRIM_TAIL if c == n - 1 else JOIN_TRIM_INNER))
        skip = max(0, 600 * d[0] - 24 * keep_ms) if head else 0
        cut = max(0, 600 * d[-1] - 24 * keep_ms) if tail else 0
        rows.append((skip, 600 * sum(d) - skip - cut, 0 if c == n - 1 else 24 * pause_ms, 24 * fade_ms if head else 0,
                     24 * fade_ms if tail else 0))
    return rows


def join_stream(chunks_samples, durations_per_chunk: Sequence[Sequence[int]], join) -> np.ndarray:
    """The stream of ONE joined request at 24 kHz, float32: for each chunk in order its kept samples x[skip .. skip + keep) --
    sample i < n of a faded head and sample keep - 1 - i of a faded tail as f32(f64(x) * (f64(2 i + 1) / f64(2 n))) -- then gap
    zeros.  `chunks_samples[c]` = the chunk's samples (at least 600 x its frames; what lies beyond is not used)."""
    parts = []
    for x, d, (skip, keep, gap, fh, ft) in zip(chunks_samples, durations_per_chunk, join_rows(durations_per_chunk, join)):
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        if x.shape[0] < 600 * int(np.sum(np.asarray(d, dtype=np.int64))):
            raise ValueError("join_stream: a chunk is shorter than its frames")
        seg = x[skip: skip + keep].copy()
        with np.errstate(invalid="ignore", over="ignore"):
            if fh:
                g = (2 * np.arange(fh, dtype=np.float64) + 1) / np.float64(2 * fh)
                seg[:fh] = (seg[:fh].astype(np.float64) * g).astype(np.float32)
            if ft:
                g = (2 * np.arange(ft, dtype=np.float64) + 1) / np.float64(2 * ft)
                seg[keep - ft:] = (seg[keep - ft:].astype(np.float64) * g[::-1]).astype(np.float32)
        parts.append(seg)
        parts.append(np.zeros(gap, dtype=np.float32))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)


def joined_marks(durations_per_chunk: Sequence[Sequence[int]], word: int, join) -> np.ndarray:
    """The token marks of ONE joined request in int64: m_c[t] = (P_c + clamp(600 x sum of d_c[t'] for t' < t - skip_c, 0,
    keep_c)) L / M with P_c the kept samples and pauses of the chunks before c.  The all-zero spec gives `token_marks`."""
    code = (int(word) >> 8) & 15
    if code not in _RATE_LM or not durations_per_chunk:
        raise ValueError("joined_marks: unknown output sample rate, or a request without chunks")
    L, M = _RATE_LM[code]
    out, base = [], 0
    for d, (skip, keep, gap, _, _) in zip(durations_per_chunk, join_rows(durations_per_chunk, join)):
        u = 600 * np.concatenate([np.zeros(1, np.int64), np.cumsum(np.asarray(d, dtype=np.int64).reshape(-1), dtype=np.int64)])
        out.append((base + np.clip(u - skip, 0, keep)) * L // M)
        base += keep + gap
    return np.concatenate(out).astype(np.int64)


def joined_body(chunks_samples, durations_per_chunk: Sequence[Sequence[int]], word: int, join) -> bytes:
    """The body of ONE joined request in the format word `word`, as bytes: join_stream, resample_stream, then the form."""
    return stream_body(resample_stream(join_stream(chunks_samples, durations_per_chunk, join), word), word)


LEVEL_GAIN, LEVEL_NORMALIZE, LEVEL_CEILING = 0, 1, 2
LEVEL_PLAIN = (LEVEL_GAIN, 1.0, 0.0)
PEAK_TRUE = 0x100  # OR-ed into a level or loudness mode: the peak is the true peak (include/kokorox_hip.h, "levels")


def true_peak_taps() -> np.ndarray:
    """The 72 taps of the true-peak interpolator as float32 [3][24], phase 1 first, from the library's one table
    (kokorox_amd/csrc/truepeak_taps.h through kx_truepeak_filter)."""
    from . import hip_koko as hk
    return hk.truepeak_filter()


def true_peak(z) -> np.float32:
    """tp of ONE request's stream z, which is at its output rate already, by the definition of include/kokorox_hip.h, "levels":
    x[j] = f64(z[j]) where z[j] is finite, 0 elsewhere and outside the stream; for phi = 1..3,
    u_phi[n] = f32(sum over j = n - 11 .. n + 12 ascending of f64(t_phi[n - j + 12]) x[j]), a float64 accumulator from +0;
    tp = max(p, max |u_phi[n]|) as a float32, with p the sample peak of level_gain.  Vectorised over n, the 24 taps one after
    the other in ascending j: the order of every chain is the GPU's."""
    z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1)
    a = np.abs(z[~np.isnan(z)])
    tp = np.float32(a.max()) if a.shape[0] else np.float32(0)
    N = z.shape[0]
    if N == 0:
        return tp
    taps = true_peak_taps().astype(np.float64)
    x = np.concatenate([np.zeros(11), np.where(np.isfinite(z), z, np.float32(0)).astype(np.float64), np.zeros(12)])
    with np.errstate(over="ignore"):
        for phi in range(3):
            acc = np.zeros(N, dtype=np.float64)
            for k in range(24):  # j = n - 11 + k, tap n - j + 12 = 23 - k
                acc = acc + taps[phi, 23 - k] * x[k: k + N]
            tp = max(tp, np.float32(np.abs(acc.astype(np.float32)).max()))
    return np.float32(tp)


def _level_fields(level):
    """(mode, gain, peak) of a valid level spec (include/kokorox_hip.h, "levels"), gain and peak as float32; None = the plain
    spec.  The mode may carry PEAK_TRUE; the rules follow its low byte.  Every comparison is written so that a NaN fails it."""
    mode, gain, peak = level if level is not None else LEVEL_PLAIN
    with np.errstate(over="ignore", invalid="ignore"):
        gain, peak = np.float32(gain), np.float32(peak)
    ok = isinstance(mode, (int, np.integer)) and not isinstance(mode, bool) and (mode & ~PEAK_TRUE) in (0, 1, 2) and bool(np.float32(0) <= gain <= np.float32(64))
    low = mode & ~PEAK_TRUE if ok else 0
    if ok and low == LEVEL_GAIN:
        ok = peak.tobytes() == np.float32(0).tobytes()  # +0.0f and nothing else
    elif ok:
        ok = (low != LEVEL_NORMALIZE or gain == np.float32(1)) and bool(np.float32(2.0 ** -15) <= peak <= np.float32(1))
    if not ok:
        raise ValueError("level: mode 0..2 (| PEAK_TRUE), gain 0..64 (1 in mode 1), peak +0 in mode 0 and 2^-15..1 in modes 1 and 2")
    return int(mode), gain, peak


def level_gain(z, level):
    """(p, g) of ONE request's stream z, which is at its output rate already, by the definition of include/kokorox_hip.h,
    "levels": p = the largest |z[n]| over the samples that are no NaN as a float32 (+inf counts; 0 when there is none), g the
    float64 gain of `level` = (mode, gain, peak): gain itself (mode 0), peak / p (mode 1, when 0 < p < inf, else 1), or gain
    unless gain * p > peak, then peak / p (mode 2, when 0 < p < inf) -- one float64 division, one float64 product.  A mode
    with PEAK_TRUE: p is true_peak(z), in the rules and in what is returned."""
    mode, gain, peak = _level_fields(level)
    z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1)
    if mode & PEAK_TRUE:
        p = true_peak(z)
    else:
        a = np.abs(z[~np.isnan(z)])
        p = np.float32(a.max()) if a.shape[0] else np.float32(0)
    mode &= ~PEAK_TRUE
    usable = bool(np.float32(0) < p < np.float32(np.inf))
    g = np.float64(gain)
    if mode == LEVEL_NORMALIZE:
        g = np.float64(peak) / np.float64(p) if usable else np.float64(1.0)
    elif mode == LEVEL_CEILING and usable and g * np.float64(p) > np.float64(peak):
        g = np.float64(peak) / np.float64(p)
    return p, float(g)


def level_stream(z, level) -> np.ndarray:
    """The levelled stream z'[n] = f32(g * f64(z[n])) with g of level_gain: one float64 product and one round-to-nearest-even
    conversion per sample; a NaN stays a NaN."""
    z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1)
    _, g = level_gain(z, level)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (np.float64(g) * z.astype(np.float64)).astype(np.float32)


def levelled_body(chunks_samples, durations_per_chunk: Sequence[Sequence[int]], word: int, join, level) -> bytes:
    """The body of ONE levelled request in the format word `word`, as bytes: join_stream (join = None: the chunks appended),
    resample_stream, level_stream, then the form."""
    return stream_body(level_stream(resample_stream(join_stream(chunks_samples, durations_per_chunk, join), word), level), word)


_FORM_SAMPLE_BYTES = {0: 4, 1: 8, 2: 2, 3: 4, 8: 1, 9: 1}  # the forms a piece may have: bytes per sample (form 3: behind 44 header bytes)


def piece_ranges(lengths: Sequence[int], word: int) -> List[int]:
    """E_k of a request run in pieces (the definition of include/kokorox_hip.h, "pieces"): `lengths[k]` = the joined source
    samples at 24 kHz of piece k (600 x its frames where nothing joins the chunks; `piece_lengths` with a join), `word` the request's
    format word (only its rate code matters).  With A_k their running sum, N = A L / M and (L, M, C) the rate's filter, output n is
    final after piece k when n M + C <= A_k L - 1: F_k = clamp(floor((A_k L - 1 - C) / M) + 1, 0, N), E_k = 4 floor(F_k / 4); E_k = A_k
    at rate code 0, and N for the last piece.  Piece k's payload is samples [E_{k-1}, E_k) of the whole body."""
    from . import hip_koko as hk
    code = (int(word) >> 8) & 15
    if code not in _RATE_LM or not len(lengths):
        raise ValueError("piece_ranges: unknown output sample rate, or a request without pieces")
    L, M = _RATE_LM[code]
    A = np.cumsum(np.asarray(lengths, dtype=np.int64))
    if int(np.min(np.asarray(lengths, dtype=np.int64))) < 0 or (int(A[-1]) * L) % M:
        raise ValueError("piece_ranges: negative length, or a stream that gives no whole number of output samples")
    N = int(A[-1]) * L // M
    if code == 0:
        return [int(a) for a in A]
    C = (hk.resample_filter(word)[2].shape[0] - 1) // 2
    out = []
    for k, a in enumerate(int(v) for v in A):
        q = a * L - 1 - C
        F = min(max(q // M + 1, 0), N) if q >= 0 else 0
        out.append(N if k == len(A) - 1 else 4 * (F // 4))
    return out


def piece_lengths(durations_per_chunk: Sequence[Sequence[int]], join, cuts: Sequence[int]) -> List[int]:
    """The joined source samples of every piece of ONE request: `cuts[k]` = chunks of piece k (they add up to the request's chunks).
    A piece's rows have the join rows they have in the whole request (`join_rows`): a piece that is not the last keeps the pause
    behind its final chunk, and every boundary between pieces is an inner boundary."""
    rows = join_rows(durations_per_chunk, join)
    if sum(int(c) for c in cuts) != len(rows) or any(int(c) < 1 for c in cuts):
        raise ValueError("piece_lengths: every piece has a chunk, and the pieces add up to the request")
    out, at = [], 0
    for c in cuts:
        out.append(sum(keep + gap for _, keep, gap, _, _ in rows[at: at + int(c)]))
        at += int(c)
    return out


def piece_bodies(chunks_samples, durations_per_chunk: Sequence[Sequence[int]], word: int, join, level, cuts: Sequence[int]) -> List[bytes]:
    """The payloads of ONE request run in pieces of cuts[k] chunks each, as slices of `levelled_body` of the request run whole (level a
    spec of mode LEVEL_GAIN, or None): piece k is the bytes of samples [E_{k-1}, E_k) in the word's form, behind the form's header in
    piece 0 only.  Laid end to end they are the whole body, every byte."""
    form = int(word) & 0xFF
    if form not in _FORM_SAMPLE_BYTES:
        raise ValueError("piece_bodies: a piece cannot carry a sized form")
    if level is not None and _level_fields(level)[0] != LEVEL_GAIN:
        raise ValueError("piece_bodies: a piece cannot carry a measured level")
    body = levelled_body(chunks_samples, durations_per_chunk, word, join, level)
    E = piece_ranges(piece_lengths(durations_per_chunk, join, cuts), word)
    w, hdr = _FORM_SAMPLE_BYTES[form], 44 if form == 3 else 0
    edges = [0] + [hdr + w * e for e in E]
    assert edges[-1] == len(body)
    return [body[a: b] for a, b in zip(edges[:-1], edges[1:])]


def piece_carry(chunks_samples, durations_per_chunk: Sequence[Sequence[int]], word: int, join, cuts: Sequence[int]) -> np.ndarray:
    """The carry every piece of ONE request leaves, an array of hip_koko.PIECE_CARRY_DTYPE: A_k and E_k, the chunks so far, and the
    last n_tail = min(PIECE_TAIL, A_k) samples of the joined 24 kHz stream so far (n_tail = 0 at rate code 0), zeros behind them.
    A request run whole (one piece) leaves the all-zero record."""
    from . import hip_koko as hk
    out = np.zeros(len(cuts), hk.PIECE_CARRY_DTYPE)
    if len(cuts) == 1:
        return out
    x = join_stream(chunks_samples, durations_per_chunk, join)
    lengths = piece_lengths(durations_per_chunk, join, cuts)
    A, E, code = np.cumsum(lengths), piece_ranges(lengths, word), (int(word) >> 8) & 15
    for k in range(len(cuts)):
        n_tail = 0 if code == 0 else min(hk.PIECE_TAIL, int(A[k]))
        out[k]["magic"], out[k]["format_word"] = hk.PIECE_MAGIC, int(word)
        out[k]["src_samples"], out[k]["out_samples"] = int(A[k]), int(E[k])
        out[k]["n_tail"], out[k]["reserved"] = n_tail, sum(int(c) for c in cuts[: k + 1])
        out[k]["tail"][:n_tail] = x[int(A[k]) - n_tail: int(A[k])]
    return out


LOUDNESS_MEASURE, LOUDNESS_NORMALIZE = 0, 1
LOUDNESS_METER = (LOUDNESS_MEASURE, 0.0, 0.0)
LOUDNESS_ABS_GATE = 10.0 ** ((-70 + 0.691) / 10)  # the absolute gate of BS.1770 as a block energy
_RATE_WORD = {24000: 0x000, 8000: 0x100, 16000: 0x200, 48000: 0x300}


def kweight_coefs(rate: int) -> np.ndarray:
    """The ten float64 K-weighting coefficients at an output rate (24000, 8000, 16000 or 48000 Hz) from the library's one table
    (kokorox_amd/csrc/kweight_coefs.h through kx_loudness_filter): shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2."""
    from . import hip_koko as hk
    if int(rate) not in _RATE_WORD:
        raise ValueError("kweight_coefs: the rate is 24000, 8000, 16000 or 48000")
    return hk.loudness_filter(_RATE_WORD[int(rate)])


def kweight(x, rate: int) -> np.ndarray:
    """The K-weighted stream w of include/kokorox_hip.h, "loudness", in float64: x[n] = f64(z[n]) where z[n] is finite, else 0;
    two biquads in direct form I, shelf first, then high-pass, from zero state, one sample after the other."""
    z = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    xs = np.where(np.isfinite(z), z, np.float32(0)).astype(np.float64).tolist()
    b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = (float(v) for v in kweight_coefs(rate))
    x1 = x2 = v1 = v2 = w1 = w2 = 0.0
    out = [0.0] * len(xs)
    for n, xn in enumerate(xs):
        v = b0 * xn + b1 * x1 + b2 * x2 - a1 * v1 - a2 * v2
        w = c0 * v + c1 * v1 + c2 * v2 - d1 * w1 - d2 * w2
        x2, x1, v2, v1, w2, w1 = x1, xn, v1, v, w1, w
        out[n] = w
    return np.array(out, dtype=np.float64)


def hop_energies(z, rate: int) -> np.ndarray:
    """e[k] = the sum of w[n]^2 over hop k of rate / 10 samples, k < floor(N / hop): a trailing partial hop is ignored."""
    w = kweight(z, rate)
    hop = int(rate) // 10
    H = w.shape[0] // hop
    return (w[: H * hop].reshape(H, hop) ** 2).sum(axis=1) if H else np.zeros(0, dtype=np.float64)


def gated_loudness(e, rate: int):
    """(I, n_g, margin) from the hop energies e: the 400 ms block means z_j = (e[j] + e[j+1] + e[j+2] + e[j+3]) / (4 hop), the
    absolute gate z_j > 10^((-70 + 0.691) / 10), the relative gate z_j > 0.1 m1 with m1 the mean over the absolute gate's blocks,
    I = -0.691 + 10 log10(the mean over the n_g blocks that pass both), NaN when there is no such block.  margin = the smallest
    relative distance |z_j - t| / t of any block to either threshold t (inf when there is no block): an input whose margin is
    large against the rounding of e has the same n_g on every implementation."""
    e = np.asarray(e, dtype=np.float64).reshape(-1)
    hop = int(rate) // 10
    J = e.shape[0] - 3
    if J < 1:
        return float("nan"), 0, float("inf")
    zj = (((e[0:J] + e[1:J + 1]) + e[2:J + 2]) + e[3:J + 3]) / (4.0 * hop)
    margin = float(np.min(np.abs(zj - LOUDNESS_ABS_GATE) / LOUDNESS_ABS_GATE))
    above = zj > LOUDNESS_ABS_GATE
    if not above.any():
        return float("nan"), 0, margin
    floor = 0.1 * (float(zj[above].sum()) / int(above.sum()))
    margin = min(margin, float(np.min(np.abs(zj - floor) / floor)))
    both = above & (zj > floor)
    n_g = int(both.sum())
    if n_g == 0:
        return float("nan"), 0, margin
    return -0.691 + 10.0 * float(np.log10(float(zj[both].sum()) / n_g)), n_g, margin


def integrated_loudness(z, rate: int):
    """(I, n_g, margin) of ONE request's stream z, which is at the output rate `rate` already: gated_loudness of hop_energies."""
    return gated_loudness(hop_energies(z, rate), rate)


def _loudness_fields(loudness):
    """(mode, target_lufs, peak) of a valid loudness spec (include/kokorox_hip.h, "loudness"), the two floats as float32; None =
    the meter.  The mode may carry PEAK_TRUE.  Every comparison is written so that a NaN fails it."""
    mode, target, peak = loudness if loudness is not None else LOUDNESS_METER
    with np.errstate(over="ignore", invalid="ignore"):
        target, peak = np.float32(target), np.float32(peak)
    ok = isinstance(mode, (int, np.integer)) and not isinstance(mode, bool) and (mode & ~PEAK_TRUE) in (0, 1)
    if ok and mode & ~PEAK_TRUE == LOUDNESS_MEASURE:
        ok = target.tobytes() == np.float32(0).tobytes() and peak.tobytes() == np.float32(0).tobytes()
    elif ok:
        ok = bool(np.float32(-70) <= target <= np.float32(0)) and bool(np.float32(2.0 ** -15) <= peak <= np.float32(1))
    if not ok:
        raise ValueError("loudness: mode 0 (| PEAK_TRUE) with target and peak +0, or mode 1 (| PEAK_TRUE) with -70 <= target_lufs <= 0 and 2^-15 <= peak <= 1")
    return int(mode), target, peak


def loudness_gain(p, I, loudness) -> float:
    """The float64 gain of a loudness spec for a stream of peak p (level_gain's) and integrated loudness I: 1 for the meter;
    10^((target - I) / 20) when I is defined, else 1, and then peak / p where p is usable and g p would pass peak.  A mode with
    PEAK_TRUE: the rule is the same and p is the stream's true peak (level_gain with the flag, or true_peak)."""
    mode, target, peak = _loudness_fields(loudness)
    p = np.float32(p)
    g = np.float64(1.0)
    if mode & ~PEAK_TRUE == LOUDNESS_NORMALIZE:
        if not np.isnan(I):
            g = np.float64(10.0) ** ((np.float64(target) - np.float64(I)) / np.float64(20.0))
        if bool(np.float32(0) < p < np.float32(np.inf)) and g * np.float64(p) > np.float64(peak):
            g = np.float64(peak) / np.float64(p)
    return float(g)


def loudness_body(z, g: float, word: int) -> bytes:
    """The body of a request whose stream z (at the word's rate) is scaled by the gain g: z'[n] = f32(g f64(z[n])), one float64
    product and one rounding per sample as in level_stream, then the form of `word`.  (With PEAK_TRUE in the spec g came from the
    true peak: the body is made the same way.)"""
    z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return stream_body((np.float64(g) * z.astype(np.float64)).astype(np.float32), word)


LIMIT_GAIN, LIMIT_LOUDNESS = 0, 1
_WORD_RATE = {0: 24000, 1: 8000, 2: 16000, 3: 48000}  # rate code of a format word -> Hz


def limit_taps(rate: int):
    """(W, h): the limiter's window W = rate / 200 and its 2 W + 1 smoothing weights as float32 at an output rate (24000, 8000,
    16000 or 48000 Hz), from the library's one table (kokorox_amd/csrc/limit_taps.h through kx_limit_filter)."""
    from . import hip_koko as hk
    if int(rate) not in _RATE_WORD:
        raise ValueError("limit_taps: the rate is 24000, 8000, 16000 or 48000")
    return hk.limit_filter(_RATE_WORD[int(rate)])


def _limit_fields(limit):
    """(mode, gain, target_lufs, peak) of a valid limit spec (include/kokorox_hip.h, "limiter"), the three floats as float32.  The
    mode may carry PEAK_TRUE.  Every comparison is written so that a NaN fails it."""
    mode, gain, target, peak = limit
    with np.errstate(over="ignore", invalid="ignore"):
        gain, target, peak = np.float32(gain), np.float32(target), np.float32(peak)
    ok = isinstance(mode, (int, np.integer)) and not isinstance(mode, bool) and (mode & ~PEAK_TRUE) in (0, 1)
    ok = ok and bool(np.float32(2.0 ** -15) <= peak <= np.float32(1))
    if ok and mode & ~PEAK_TRUE == LIMIT_GAIN:
        ok = bool(np.float32(0) <= gain <= np.float32(64)) and target.tobytes() == np.float32(0).tobytes()
    elif ok:
        ok = bool(gain == np.float32(1)) and bool(np.float32(-70) <= target <= np.float32(0))
    if not ok:
        raise ValueError("limit: mode 0 (| PEAK_TRUE) with 0 <= gain <= 64 and target +0, or mode 1 (| PEAK_TRUE) with gain 1 and "
                         "-70 <= target_lufs <= 0; 2^-15 <= peak <= 1")
    return int(mode), gain, target, peak


def limit_curve(z1, peak, word: int, true_peak_flag: bool = False):
    """(s, a) of the driven stream z1 (float32, at the rate of the format word `word`) by the definition of include/kokorox_hip.h,
    "limiter": the envelope a as float32 (|z1|, 0 where z1 is not finite; with true_peak_flag the largest of it and the three
    interpolated values either side), the required gain c, its sliding minimum m over [j - W, j + W] with c = 1 outside the stream,
    and the smoothed gain s as float64: the sum over j = n - W .. n + W ascending of f64(h[j - n + W]) f64(m[j]) from +0, and 1.0
    exactly where every m of the sum is 1.  Vectorised over n, the weights one after the other: the order of every chain is the GPU's."""
    z1 = np.ascontiguousarray(z1, dtype=np.float32).reshape(-1)
    peak = np.float32(peak)
    N = z1.shape[0]
    W, h = limit_taps(_WORD_RATE[(int(word) >> 8) & 15])
    x = np.where(np.isfinite(z1), z1, np.float32(0)).astype(np.float32)
    a = np.abs(x)
    if N == 0:
        return np.zeros(0, dtype=np.float64), a
    if true_peak_flag:
        taps = true_peak_taps().astype(np.float64)
        xp = np.concatenate([np.zeros(11), x.astype(np.float64), np.zeros(12)])
        e = np.zeros(N, dtype=np.float32)
        with np.errstate(over="ignore"):
            for phi in range(3):
                acc = np.zeros(N, dtype=np.float64)
                for k in range(24):  # j = n - 11 + k, tap n - j + 12 = 23 - k
                    acc = acc + taps[phi, 23 - k] * xp[k: k + N]
                e = np.maximum(e, np.abs(acc.astype(np.float32)))
        a = np.maximum(a, np.maximum(e, np.concatenate([np.zeros(1, dtype=np.float32), e[:-1]])))
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        c = np.where(a <= peak, np.float32(1), (np.float64(peak) / a.astype(np.float64)).astype(np.float32)).astype(np.float32)
    cp = np.concatenate([np.ones(2 * W, dtype=np.float32), c, np.ones(2 * W, dtype=np.float32)])
    m = np.lib.stride_tricks.sliding_window_view(cp, 2 * W + 1).min(axis=1)  # m[j], j = -W .. N + W - 1
    ones = np.lib.stride_tricks.sliding_window_view(m, 2 * W + 1).min(axis=1) == np.float32(1)  # every m of sample n's sum is 1
    m64, h64 = m.astype(np.float64), h.astype(np.float64)
    s = np.zeros(N, dtype=np.float64)
    for i in range(2 * W + 1):
        s = s + h64[i] * m64[i: i + N]
    return np.where(ones, np.float64(1.0), s), a


def limit_stream(z, limit, word: int, g=None):
    """(z2, p, g, I, n_g, r) of ONE request's stream z, which is at the rate of `word` already, by the definition of
    include/kokorox_hip.h, "limiter": limit = (mode, gain, target_lufs, peak).  p = the sample peak, or true_peak(z) with
    PEAK_TRUE; g = the drive (mode 0: gain; mode 1: 10^((target - I) / 20) where I is defined, else 1), capped where g p would
    pass 4 peak; z1 = f32(g f64(z)); s of limit_curve; z2 = f32(s f64(z1)) clamped to +-peak; r = the smallest f32(s), 1.0 for an
    empty stream.  I is NaN and n_g 0 in mode 0.  `g` given: that drive is taken as it is (the GPU's, whose meter agrees with this
    one to 1e-8 and not to the bit), everything behind it follows."""
    mode, gain, target, peak = _limit_fields(limit)
    z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1)
    flag = bool(mode & PEAK_TRUE)
    p, _ = level_gain(z, (LEVEL_GAIN | (PEAK_TRUE if flag else 0), 1.0, 0.0))
    I, n_g = float("nan"), 0
    if mode & ~PEAK_TRUE == LIMIT_LOUDNESS:
        I, n_g, _ = integrated_loudness(z, _WORD_RATE[(int(word) >> 8) & 15])
    if g is None:
        g = np.float64(gain)
        if mode & ~PEAK_TRUE == LIMIT_LOUDNESS:
            g = np.float64(10.0) ** ((np.float64(target) - np.float64(I)) / np.float64(20.0)) if not np.isnan(I) else np.float64(1.0)
        cap = np.float64(4.0) * np.float64(peak)
        if bool(np.float32(0) < p < np.float32(np.inf)) and g * np.float64(p) > cap:
            g = cap / np.float64(p)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        z1 = (np.float64(g) * z.astype(np.float64)).astype(np.float32)
        s, _ = limit_curve(z1, peak, word, flag)
        z2 = (s * z1.astype(np.float64)).astype(np.float32)
        z2 = np.where(np.abs(z2) > peak, np.copysign(peak, z2), z2).astype(np.float32)
        r = float(s.astype(np.float32).min()) if s.shape[0] else 1.0
    return z2, p, float(g), float(I), int(n_g), r


def limited_body(chunks_samples, durations_per_chunk: Sequence[Sequence[int]], word: int, join, limit, g=None) -> bytes:
    """The body of ONE limited request in the format word `word`, as bytes: join_stream (join = None: the chunks appended),
    resample_stream, limit_stream, then the form."""
    z = resample_stream(join_stream(chunks_samples, durations_per_chunk, join), word)
    return stream_body(limit_stream(z, limit, word, g)[0], word)


def stream_body(y, word: int) -> bytes:
    """The form of a format word applied to a request's stream `y`, which is at the word's rate already, as bytes."""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
    form, rate = int(word) & 0xFF, {0: 24000, 1: 8000, 2: 16000, 3: 48000}[(int(word) >> 8) & 15]
    if form == 0:
        return y.astype("<f4").tobytes()
    if form == 1:
        return np.repeat(y, 2).astype("<f4").tobytes()
    if form == 2:
        # (form 2 clamps with fmax / fmin, which drop a NaN: -32767 there, include/kokorox_hip.h)
        c = np.where(np.isnan(y), np.float32(-1.0), np.clip(y, np.float32(-1.0), np.float32(1.0))).astype(np.float32)
        return np.trunc(c * np.float32(32767.0)).astype("<i2").tobytes()
    if form == 3:
        return wav_f32_body(y, rate)
    if form == 4:
        return wav16_base64(y, rate)
    if form in (8, 9):
        return (mulaw_bytes if form == 8 else alaw_bytes)(pcm16(y)).tobytes()
    if form == 12:
        return flac_body(pcm16(y), rate)
    if form == 17:
        return adpcm_wav_body(pcm16(y), rate)
    if form == 18:  # (the region: the file and its zero padding to a multiple of 4)
        body = wav16_body(y, rate)
        return body + bytes(-len(body) % 4)
    raise ValueError("stream_body: unknown output format")


def token_spans(marks, chunk_tokens: Sequence[int]):
    """A request's marks as one (start, end) pair of int64 arrays per chunk: token t of chunk c occupies samples
    [start[t], end[t]) of the request's stream.  `chunk_tokens[c]` = tokens of chunk c (its two pads included); chunk c has
    chunk_tokens[c] + 1 marks.  start[0] is where the chunk begins in the body; the first and the last span are the spans of
    the two pad tokens: the chunk's lead-in and tail."""
    m = np.asarray(marks, dtype=np.int64).reshape(-1)
    if m.shape[0] != sum(int(t) + 1 for t in chunk_tokens):
        raise ValueError("token_spans: a request has the sum over its chunks of tokens + 1 marks")
    spans, o = [], 0
    for t in chunk_tokens:
        t = int(t)
        spans.append((m[o: o + t].copy(), m[o + 1: o + t + 1].copy()))
        o += t + 1
    return spans


def word_spans(spans, words: Sequence[Sequence[int]]):
    """(start, end) samples of words given as token index ranges: `spans` = (start, end) arrays of ONE chunk (token_spans),
    `words` = (first token, last token) pairs, both inclusive, indices into the chunk's tokens with the pads counted.  A word
    starts where its first token starts and ends where its last token ends.  (Which tokens make a word is the text
    front-end's knowledge: it stays outside this library.)"""
    start, end = spans
    out = []
    for a, b in words:
        a, b = int(a), int(b)
        if not 0 <= a <= b < len(start):
            raise ValueError("word_spans: token range outside the chunk")
        out.append((int(start[a]), int(end[b])))
    return out


def tts_request(model, styles: Dict[str, np.ndarray], style_name: str, chunk_tokens: Sequence[Sequence[int]],
                speed: float = 1.0, initial_silence: int = 0, seed: int = 0, fmt: int = 0, join=None, level=None, loudness=None,
                limit=None):
    """`tts_chunks` through `model.infer_requests`: the chunks of one text as ONE request of one batched forward, its body
    (header of the form, then the chunks' samples with nothing between them) packed on the GPU.  `fmt` is a format word of
    hip_koko (a PACK_* form, optionally | PACK_RATE_*): 0..2 and 8 / 9 give the samples as an array, 3 (`wav_f32_body`) and 4
    (`wav16_base64`) the bytes a server sends, 12 (`flac_body`) a FLAC stream of the 16-bit samples.  `join` = (flags, keep_ms, pause_ms, fade_ms): the seams shaped on the GPU
    (`model.infer_requests_joined`; trim the pads' silence, pause between sentences, fade the cut edges).  `level` = (mode, gain,
    peak): the level set on the GPU (`model.infer_requests_levelled`; a volume, a peak to normalise to, or a ceiling).
    `loudness` = (mode, target_lufs, peak): the BS.1770 loudness set on the GPU (`model.infer_requests_loudness`).  Either mode
    may carry PEAK_TRUE: `peak` then bounds the true peak of the body, four times oversampled, not its largest sample.
    `limit` = (mode, gain, target_lufs, peak): the body driven by a gain or to a loudness and peak-limited on the GPU
    (`model.infer_requests_limited`): only the neighbourhood of the samples that would pass `peak` is turned down.  An
    empty chunk list and an empty chunk are errors (a request has at least one chunk)."""
    toks, rows = [], []
    for ch in chunk_tokens:
        t = [30] * int(initial_silence) + [int(v) for v in ch]
        if not t:
            raise ValueError("tts_request: empty chunk")
        rows.append(mix_styles(styles, style_name, len(t))[0])
        toks.append([0] + t + [0])
    if not toks:
        raise ValueError("tts_request: a request has at least one chunk")
    if limit is not None:
        if level is not None or loudness is not None:
            raise ValueError("tts_request: a request has a level, a loudness or a limit, not two of them")
        return model.infer_requests_limited(toks, [len(toks)], limit, joins=join, styles=np.asarray(rows, dtype=np.float32),
                                            speeds=[float(speed)], seed=seed, fmt=fmt)[0][0]
    if loudness is not None:
        if level is not None:
            raise ValueError("tts_request: a request has a level or a loudness, not both")
        return model.infer_requests_loudness(toks, [len(toks)], loudness, joins=join, styles=np.asarray(rows, dtype=np.float32),
                                             speeds=[float(speed)], seed=seed, fmt=fmt)[0][0]
    if level is not None:
        return model.infer_requests_levelled(toks, [len(toks)], level, joins=join, styles=np.asarray(rows, dtype=np.float32),
                                             speeds=[float(speed)], seed=seed, fmt=fmt)[0][0]
    if join is not None:
        return model.infer_requests_joined(toks, [len(toks)], join, styles=np.asarray(rows, dtype=np.float32), speeds=[float(speed)],
                                           seed=seed, fmt=fmt)[0]
    return model.infer_requests(toks, [len(toks)], styles=np.asarray(rows, dtype=np.float32), speeds=[float(speed)], seed=seed,
                                fmt=fmt)[0]


# ---- prosody (include/kokorox_hip.h, "prosody"): the numpy form of the per-token controls and of the report -------------------------
PROSODY_MAX_FRAMES = 50
_F0_FLOOR = np.float32(10.0)
_F0_ABOVE_FLOOR = np.array([0x41200001], dtype=np.uint32).view(np.float32)[0]  # the float above 10


def semitones(p) -> np.float32:
    """The pitch ratio of p semitones, float32(2 ** (p / 12)): what a caller puts into `pitch` (the library takes ratios)."""
    return np.float32(2.0 ** (float(p) / 12.0))


def prosody_ok(rate=None, frames=None, pitch=None, energy=None) -> bool:
    """The validity rule of kx_prosody over the given values: 0.25 <= rate <= 4, 0 <= frames <= 50, 0.25 <= pitch <= 4,
    0 <= energy <= 4; a NaN fails every rule; None is neutral."""
    def inside(a, lo, hi):
        a = np.asarray(a, dtype=np.float32)
        return bool(np.all((a >= np.float32(lo)) & (a <= np.float32(hi))))
    ok = rate is None or inside(rate, 0.25, 4)
    ok = ok and (pitch is None or inside(pitch, 0.25, 4))
    ok = ok and (energy is None or inside(energy, 0, 4))
    if frames is not None:
        f = np.asarray(frames, dtype=np.int64)
        ok = ok and bool(np.all((f >= 0) & (f <= PROSODY_MAX_FRAMES)))
    return ok


def prosody_durations(s, rate=None, frames=None, pinned=None, idx_ld=None) -> np.ndarray:
    """The USED durations of one row from its float32 values s[t] = (sum of sigmoids) / speed: divided by rate[t] in float32,
    rounded half to even, at least 1, the model's pinned pattern over it, frames[t] >= 1 over that, and the row cut at idx_ld frames
    (default 50 per token) as the duration kernel cuts it."""
    s = np.asarray(s, dtype=np.float32).reshape(-1)
    T = s.shape[0]
    idx_ld = 50 * T if idx_ld is None else int(idx_ld)
    if rate is not None:
        s = (s / np.asarray(rate, dtype=np.float32).reshape(-1)).astype(np.float32)
    r = np.rint(s)
    d = np.where(~(r >= np.float32(1)), 1, np.where(r > np.float32(idx_ld), idx_ld + 1, np.nan_to_num(r))).astype(np.int64)
    if pinned is not None and len(pinned):
        d = np.asarray(pinned, dtype=np.int64)[np.arange(T) % len(pinned)]
    if frames is not None:
        f = np.asarray(frames, dtype=np.int64).reshape(-1)
        d = np.where(f >= 1, f, d)
    scan = np.cumsum(d)
    return (np.minimum(scan, idx_ld) - np.minimum(scan - d, idx_ld)).astype(np.int32)


FIT_FRAME_SECONDS = 0.025  # a frame: 600 samples at 24 000 Hz


def fit_frames(seconds) -> int:
    """The frame count closest to `seconds` (a frame is 25 ms): what a caller puts into a fit span."""
    return int(round(float(seconds) / FIT_FRAME_SECONDS))


def fit_weights(s) -> np.ndarray:
    """The weights of a fit from the float32 values s[t] before rintf: s inside 2^-20 .. 2^20, clamped to it outside, 1 for a NaN."""
    s = np.asarray(s, dtype=np.float32).reshape(-1)
    lo, hi = np.float32(2.0 ** -20), np.float32(2.0 ** 20)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(s), np.float32(1), np.minimum(np.maximum(s, lo), hi)).astype(np.float32)


def fit_counts(w, lam_bits) -> np.ndarray:
    """d_t(lambda) of the definition for the float32 lambda with the bit pattern lam_bits: min(max(rint(f32(w lambda)), 1), 50)."""
    lam = np.array([lam_bits], dtype=np.uint32).view(np.float32)[0]
    with np.errstate(over="ignore", under="ignore"):
        p = (np.asarray(w, dtype=np.float32) * lam).astype(np.float32)
    return np.minimum(np.maximum(np.rint(p), np.float32(1)), np.float32(50)).astype(np.int64)


def fit_durations(w, frames, held=None):
    """The fit of one span (include/kokorox_hip.h, "fit"): w = the float32 values of its tokens before rintf (clamped here as the
    GPU clamps them), frames = the wanted total, held = None or one count per token, >= 1 where the token is held.  Returns
    (d, lam_bits, excess): the durations of all its tokens (int32; a held token keeps its count), the bit pattern of lambda and E.
    Raises ValueError where the library refuses the span (no free token, G outside n .. 50 n)."""
    w = fit_weights(w)
    h = np.zeros(w.shape[0], dtype=np.int64) if held is None else np.asarray(held, dtype=np.int64).reshape(-1)
    if h.shape[0] != w.shape[0]:
        raise ValueError("fit: one held count per token")
    free = h < 1
    n = int(free.sum())
    G = int(frames) - int(h[~free].sum())
    if n == 0 or G < n or G > 50 * n:
        raise ValueError("fit: bad fit")
    wf = w[free]
    lo, hi = 0x00800000, 0x7F7FFFFF
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if int(fit_counts(wf, mid).sum()) >= G:
            hi = mid
        else:
            lo = mid + 1
    d_hi = fit_counts(wf, lo)
    E = int(d_hi.sum()) - G
    df = d_hi.copy()
    if E > 0:
        d_lo = fit_counts(wf, lo - 1)
        steppers = np.flatnonzero(d_hi == d_lo + 1)
        if steppers.shape[0] < E:
            raise AssertionError("fit: fewer steppers than the excess")
        keep = steppers[steppers.shape[0] - E:]  # (the E with the highest position)
        df[keep] = d_lo[keep]
    d = h.copy()
    d[free] = df
    return d.astype(np.int32), int(lo), E


def _prosody_ratio(rho, step_token) -> np.ndarray:
    """r[j] of the definition: the 5-step triangle over the per-token ratio, clamped to the row, float64 in ascending k."""
    n = step_token.shape[0]
    rho = np.asarray(rho, dtype=np.float32).astype(np.float64)
    j = np.arange(n)
    acc = np.zeros(n, dtype=np.float64)
    for k, w in zip(range(-2, 3), (1.0, 2.0, 3.0, 2.0, 1.0)):
        acc = acc + np.float64(w) * rho[step_token[np.clip(j + k, 0, n - 1)]]
    return acc / np.float64(9.0)


def shape_curves(f0, n, durations, pitch=None, energy=None):
    """One row's F0 and N curves (2 F steps each, F = sum(durations)) shaped by the per-token ratios; None leaves a curve as it is.
    Returns (F0', N') as float32.  Unvoiced steps (not > 10, NaN included) keep their bits; a voiced step stays above 10."""
    f0 = np.asarray(f0, dtype=np.float32).reshape(-1)
    n = np.asarray(n, dtype=np.float32).reshape(-1)
    d = np.asarray(durations, dtype=np.int64).reshape(-1)
    steps = 2 * int(d.sum())
    assert f0.shape[0] == steps and n.shape[0] == steps, "curves: 2 steps per frame"
    step_token = np.repeat(np.arange(d.shape[0]), 2 * d)
    f0s, ns = f0.copy(), n.copy()
    if pitch is not None and steps:
        with np.errstate(invalid="ignore", over="ignore"):
            voiced = f0 > _F0_FLOOR
            v = (f0.astype(np.float64) * _prosody_ratio(pitch, step_token)).astype(np.float32)
            f0s = np.where(voiced, np.where(v > _F0_FLOOR, v, _F0_ABOVE_FLOOR), f0).astype(np.float32)
    if energy is not None and steps:
        with np.errstate(invalid="ignore", over="ignore"):
            ns = (n.astype(np.float64) * _prosody_ratio(energy, step_token)).astype(np.float32)
    return f0s, ns


def prosody_report(f0s, ns, durations) -> np.ndarray:
    """The report of one row, [tokens, 4] float32: the mean of the voiced (> 10) steps of F0' of every token (+0 when none), their
    count, the mean of N' over its steps (+0 when it has none), and its frames.  Float64 sums in ascending order, rounded once."""
    f0s = np.asarray(f0s, dtype=np.float32).reshape(-1)
    ns = np.asarray(ns, dtype=np.float32).reshape(-1)
    d = np.asarray(durations, dtype=np.int64).reshape(-1)
    out = np.zeros((d.shape[0], 4), dtype=np.float32)
    at = 0
    for t, dt in enumerate(d):
        sf, sn, voiced = 0.0, 0.0, 0
        for j in range(2 * at, 2 * (at + int(dt))):
            if f0s[j] > _F0_FLOOR:
                sf += float(f0s[j])
                voiced += 1
            sn += float(ns[j])
        with np.errstate(invalid="ignore", over="ignore"):
            out[t] = (np.float32(sf / voiced) if voiced else 0.0, voiced, np.float32(sn / (2 * int(dt))) if dt else 0.0, dt)
        at += int(dt)
    return out
