"""Three packed calls of the bench batch (64 x 130 tokens, durations pinned 3,3,3,4 -> 422 frames each) in the form given on
the command line: 'old2' = kx_infer_packed form 2 (pack_audio_kernel), '2' / '3' / '4' = kx_infer_requests in that form, every
row a request of its own (pack_requests_kernel); a format word with a rate code, written as the header does ('0x108' = G.711
mu-law at 8 kHz, '0x303' = float WAV at 48 kHz), adds resample_requests_kernel in front of it; a word followed by 'm' ('2m')
runs kx_infer_requests_marks in that word, which adds token_marks_kernel behind the packer.  Meant to run under the
profiler, one word per run (kernel trace only, no counters in the same run):
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python tools/pack_profile.py 4
profiles/pack_kernels_stats.txt holds the rows of the kernel_stats.csv files."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa
from kokorox_amd import hip_koko as hk, weights as W
from oracle import kokoro_ref as R
which = sys.argv[1]
m = hk.HipKoko.new(W.ensure_synthetic_blob())
B = 64
toks = [list(int(v) for v in R.synthetic_inputs(1, 128, seed=40 + b)[0]) for b in range(B)]
rows = [W.synthetic_voices(1)[0, 128, 0]] * B
m.set_pinned_durations([3, 3, 3, 4])
word = int(which[:-1], 0) if which.endswith("m") else (2 if which == "old2" else int(which, 0))
for it in range(3):
    if which == "old2":
        out = m.infer_packed(toks, rows, fmt=2)
    elif which.endswith("m"):
        out, marks = m.infer_requests_marks(toks, [1] * B, styles=rows, fmt=word)
        L, M, _ = hk.resample_filter(word)
        assert all(k.shape[0] == 131 and int(k[-1]) == 422 * 600 * L // M for k in marks)
    else:
        out = m.infer_requests(toks, [1] * B, styles=rows, fmt=word)
    n = sum(len(o) if isinstance(o, bytes) else o.nbytes for o in out)
print("form", which, "bytes", n, "frames", len(toks[0]))
m.close()
