"""Time from submission to a request's first bytes, whole against in pieces (include/kokorox_hip.h, "pieces"): a request of 8 chunks
of 130 tokens (durations pinned 3,3,3,4 -> 422 frames a chunk) at 8 kHz mu-law on one model, (a) as one kx_infer_requests call, whose
bytes all come back together, (b) as 8 one-chunk pieces through hip_koko.RequestStream: the first piece's bytes, and the whole
request.  Wall clock around the Python calls, the median of 5 after a warm-up of each shape; prints one line per figure."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa
from kokorox_amd import hip_koko as hk, weights as W
from oracle import kokoro_ref as R

m = hk.HipKoko.new(W.ensure_synthetic_blob())
toks = [list(int(v) for v in R.synthetic_inputs(1, 128, seed=40 + b)[0]) for b in range(8)]
rows = [W.synthetic_voices(1)[0, 128, 0]] * 8
m.set_pinned_durations([3, 3, 3, 4])
word = 0x108
whole, first, pieces = [], [], []
body = parts = None
for it in range(6):
    t0 = time.perf_counter()
    body = m.infer_requests(toks, [8], styles=rows, fmt=word, seed=5)[0]
    t1 = time.perf_counter()
    stream = hk.RequestStream(m, fmt=word, seed=5)
    parts = []
    t2 = time.perf_counter()
    for c in range(8):
        parts.append(stream.send(toks[c: c + 1], rows[c: c + 1], last=c == 7))
        if c == 0:
            t3 = time.perf_counter()
    t4 = time.perf_counter()
    if it:  # (the first round sizes the arenas of both shapes)
        whole.append(t1 - t0), first.append(t3 - t2), pieces.append(t4 - t2)
assert b"".join(parts) == np.ascontiguousarray(body).tobytes()
print("whole request, 8 chunks in one call: %.2f ms to its bytes" % (1e3 * float(np.median(whole))))
print("in 8 pieces: %.2f ms to the first piece's %d bytes, %.2f ms to the last byte" % (1e3 * float(np.median(first)), len(parts[0]), 1e3 * float(np.median(pieces))))
m.close()
