"""GPU: the token-axis kernels of the forward's front half, each alone through its test hook (include/kokorox_hip_test.h), against
NumPy / torch CPU references in float64 built here: the BiLSTM recurrence on ragged batches (all three forms), the duration head
with the alignment gather, the two embedding gathers with their bad-id word, the style projections and the row fills / copies.

The hooks lay the tensors out as the model does (rows padded to 32 floats, NaN wherever a kernel must not read, a sentinel wherever
it must not write) and check what a caller cannot see themselves; what comes back here still carries the sentinel in every column
past an utterance's length.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = np.float32(-12345.5)
LSTM_NAMES = [n + suf for suf in ("", "_reverse") for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- ragged BiLSTM -----------------------------------------------------------------------------------------------------------
LSTM_TOL = 2e-5  # the bound test_bilstm_two_and_four_workgroups... holds at n_in = 640, L = 47; every L here is <= 67

LSTM_CASES = [
    # lens, n_in, hook options
    pytest.param([1], 640, {}, id="one-step-never-publishes"),
    pytest.param([2, 1, 3, 2], 64, {}, id="one-exchange-both-parities"),
    pytest.param([33, 1, 32, 31, 2, 33, 17, 5], 512, {}, id="16-pairs-groups-full-ld64"),
    pytest.param([7, 40, 1, 23, 32, 33, 2, 16, 39], 640, {}, id="18-pairs-padding-blocks"),
    pytest.param([67, 64, 3], 640, {"inplace": True}, id="inplace-rows-of-the-input"),
    pytest.param([67, 64, 3], 640, {"repeat": 4, "epoch0": 0xFFFD}, id="epoch-wrap"),
]


@functools.lru_cache(maxsize=None)
def _lstm_module(n_in):
    torch.manual_seed(1000 + n_in)
    return torch.nn.LSTM(n_in, 256, 1, batch_first=True, bidirectional=True).double()


def _lstm_reference(m, x, lens):
    """float64, utterance by utterance on its own steps; [B, L, 512] with NaN past lens[b]."""
    ref = np.full((len(lens), x.shape[1], 512), np.nan)
    with torch.no_grad():
        for b, n in enumerate(lens):
            ref[b, :n] = m(torch.from_numpy(x[b:b + 1, :n]).double())[0][0].numpy()
    return ref


def _lstm_forms(fn):
    """fn() under each of the three forms of the recurrence: two and four workgroups, and the streaming fall-back."""
    from kokorox_amd import hip_koko as hk
    tlib = hk.load_test_library()
    out = {}
    try:
        for parts in (2, 4, 1):
            tlib.kx_test_lstm_parts(parts)
            out[parts] = fn()
    finally:
        tlib.kx_test_lstm_parts(0)
    return out


@pytest.mark.parametrize("lens,n_in,opts", LSTM_CASES)
def test_bilstm_ragged_batch(lens, n_in, opts):
    """What Model::lstm asks of the recurrence and kx_test_lstm never did: every utterance its own length (the reverse direction
    starts at ITS last step, the publish / poll guards end at ITS length), padded rows, a batch whose last group of blocks is partly
    padding, the output written into the rows of the input tensor, and one exchange buffer reused across launches and across the
    wrap of its 16-bit epoch.  The three forms agree bit for bit, each is within LSTM_TOL of torch float64 run per utterance,
    nothing past an utterance's length is written, and an utterance's result does not depend on the batch around it."""
    from kokorox_amd import hip_koko as hk
    B, L = len(lens), max(lens)
    m = _lstm_module(n_in)
    ps = [getattr(m, n).detach().float().numpy() for n in LSTM_NAMES]
    rng = np.random.default_rng(sum(lens) * 7 + n_in)
    x = rng.standard_normal((B, L, n_in), dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    ref = _lstm_reference(m, x, lens)
    got = _lstm_forms(lambda: hk.lstm_ragged(x, lens, ps, **opts))
    np.testing.assert_array_equal(_bits(got[2]), _bits(got[4]))
    np.testing.assert_array_equal(_bits(got[2]), _bits(got[1]))
    for parts, y in got.items():
        for b, n in enumerate(lens):
            err = np.abs(y[b, :n] - ref[b, :n]).max()
            print(f"form {parts} utterance {b} len {n}: max |y - ref64| = {err:.3g}")
            assert err <= LSTM_TOL, (parts, b, n, err)
            assert (y[b, n:] == SENT).all(), (parts, b, "a column past the utterance's length was written")
    # the same utterance alone, B = 1 and L = lens[b], in each form
    for b, n in enumerate(lens):
        alone = _lstm_forms(lambda: hk.lstm_ragged(x[b:b + 1, :n], [n], ps, inplace=opts.get("inplace", False)))
        for parts in (2, 4, 1):
            np.testing.assert_array_equal(_bits(alone[parts][0]), _bits(got[parts][b, :n]), err_msg=f"form {parts}, utterance {b}")


# ---- duration head and alignment ---------------------------------------------------------------------------------------------
TIE_MARGIN = 0.01
# The kernel sums 50 float32 sigmoids and divides by the speed; the reference does so in float64.  50 float32 additions of partial
# sums below 64 lose at most 50 x 1.9e-6, expf and the division add a few 1e-5, and at speed 0.5 the result doubles: about 6e-4.
# Every input here keeps every s at least TIE_MARGIN = 0.01 away from a rounding tie, more than ten times that, so the float32
# kernel cannot legitimately round differently from the reference.


def _sig_sum(logits, speeds):
    """float64: s[b, t] = sum of the 50 sigmoids / speed[b]."""
    return (1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).sum(axis=1) / np.asarray(speeds, dtype=np.float64)[:, None]


def _align_inputs(T, speeds, seed):
    """(logits [3,50,T] float32, lens, row speeds): ragged lengths with the longest row not first; where it cannot overflow the
    row, one token with all 50 logits at -12 (its duration clamps to 1) and one with all at +12 (50 / speed frames)."""
    lens = [max(1, T // 2), T, max(1, T - 1)]
    row_speed = [float(speeds[b if len(speeds) > 1 else 0]) for b in range(3)]
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((3, 50, T)) - 3.0).astype(np.float32)
    for b, n in enumerate(lens):
        # (one-token rows: row 0 gets the -12 token, row 1 the +12 one, row 2 neither)
        if n >= 2 or b == 0:
            logits[b, :, 0] = -12.0
        # (a +12 token is 50 / speed frames: at T <= 2 and a speed below 1 it would not fit a row of 50 T beside the others)
        if (n >= 2 or b == 1) and 50.0 / row_speed[b] + 8.0 * (n - 1) <= 50 * T:
            logits[b, :, n - 1] = 12.0
    valid = np.arange(T)[None, :] < np.asarray(lens)[:, None]
    for _ in range(200):
        s = _sig_sum(logits, row_speed)
        near = (np.abs(s - np.floor(s) - 0.5) < TIE_MARGIN) & valid
        if not near.any():
            break
        logits[:, 0, :][near] += np.float32(0.3)
    return logits, lens, row_speed


def _align_reference(logits, lens, row_speed, pinned=None):
    """Durations (round half even, at least 1; a pinned pattern replaces them), frame counts and the repeat_interleave index."""
    s = _sig_sum(logits, row_speed)
    valid = np.arange(logits.shape[2])[None, :] < np.asarray(lens)[:, None]
    assert not ((np.abs(s - np.floor(s) - 0.5) < TIE_MARGIN) & valid).any(), "an input sits on a rounding tie"
    dur, idx = [], []
    for b, n in enumerate(lens):
        d = np.maximum(np.rint(s[b, :n]), 1.0).astype(np.int64)
        if pinned is not None:
            d = np.asarray(pinned, dtype=np.int64)[np.arange(n) % len(pinned)]
        dur.append(d)
        idx.append(np.repeat(np.arange(n), d))
    return dur, idx


def _check_alignment(hk, logits, lens, speeds, pinned, C, dur_ref, idx_ref, seed):
    B, _, T = logits.shape
    idx_ld = 50 * T
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((B, C, T), dtype=np.float32)
    for b, n in enumerate(lens):
        src[b, :, n:] = np.nan
    Fcap = max(len(i) for i in idx_ref) + 3
    dur, frames, idx, g, over = hk.alignment(logits, lens, speeds, src, pinned=pinned, idx_ld=idx_ld, Fcap=Fcap)
    assert over == 0
    for b, n in enumerate(lens):
        F = len(idx_ref[b])
        assert F <= idx_ld
        np.testing.assert_array_equal(dur[b, :n], dur_ref[b], err_msg=f"dur, row {b}")
        assert (dur[b, n:] == hk.INT_SENTINEL).all()
        assert frames[b] == F, (b, frames[b], F)
        np.testing.assert_array_equal(idx[b, :F], idx_ref[b], err_msg=f"idx, row {b}")
        assert (idx[b, F:] == hk.INT_SENTINEL).all()
        np.testing.assert_array_equal(_bits(g[b, :, :F]), _bits(src[b][:, idx_ref[b]]), err_msg=f"gathered, row {b}")
        assert (g[b, :, F:] == SENT).all()


SPEEDS = [pytest.param([2.0], id="speed2"), pytest.param([1.0], id="speed1"), pytest.param([0.5], id="speed0.5"),
          pytest.param([2.0, 1.0, 0.5], id="per-row")]
ALIGN_T = [1, 2, 33, 511, 512]


@pytest.mark.parametrize("speeds", SPEEDS)
@pytest.mark.parametrize("T", ALIGN_T)
def test_duration_and_alignment(T, speeds):
    """duration_kernel and gather_cols_kernel against float64: durations, frame counts and the gather index exactly, the gathered
    columns bit for bit at the two widths the model gathers (640 and 512 rows), nothing written past a row's frames."""
    from kokorox_amd import hip_koko as hk
    logits, lens, row_speed = _align_inputs(T, speeds, seed=T * 10 + len(speeds))
    dur_ref, idx_ref = _align_reference(logits, lens, row_speed)
    if T >= 33:  # (both extreme tokens are in: the -12 one clamps to 1, the +12 one is 50 / speed)
        assert dur_ref[1][0] == 1 and dur_ref[1][-1] == round(50 / row_speed[1])
    for C in (640, 512):
        _check_alignment(hk, logits, lens, speeds, None, C, dur_ref, idx_ref, seed=C + T)


@pytest.mark.parametrize("T,n_pinned", [(33, 3), (512, 3), (33, 512), (512, 512)])
def test_pinned_durations_replace_the_predicted_ones(T, n_pinned):
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(n_pinned + T)
    pinned = [3, 1, 50] if n_pinned == 3 else np.where(rng.random(512) < 0.02, 50, rng.integers(1, 9, size=512)).tolist()
    logits, lens, row_speed = _align_inputs(T, [0.5], seed=T + 1)
    dur_ref, idx_ref = _align_reference(logits, lens, row_speed, pinned=pinned)
    for C in (640, 512):
        _check_alignment(hk, logits, lens, [0.5], pinned, C, dur_ref, idx_ref, seed=C + n_pinned)


def test_alignment_overflow_is_cut_at_the_row_and_reported():
    """A row slowed down beyond its 50 T frames: every token at the largest duration (all logits +12: 50 sigmoids of 0.999994) and
    speed 0.5 is 100 frames per token.  The row is cut at idx_ld -- the crossing token gets the remainder, the ones behind it 0,
    dur holds what was used -- and named in the sticky word; its neighbours are what they are without it, bit for bit; nothing
    is written past a row (the hook's guards and sentinels)."""
    from kokorox_amd import hip_koko as hk
    T, C = 33, 640
    idx_ld = 50 * T
    speeds = [1.0, 0.5, 2.0]
    logits, lens, _ = _align_inputs(T, speeds, seed=5)
    assert lens[1] == T
    logits[1] = 12.0
    rng = np.random.default_rng(6)
    src = rng.standard_normal((3, C, T), dtype=np.float32)
    for b, n in enumerate(lens):
        src[b, :, n:] = np.nan
    dur, frames, idx, g, over = hk.alignment(logits, lens, speeds, src, idx_ld=idx_ld, Fcap=idx_ld)
    assert over == 1 + 1, "the overflow word names row 1"
    assert frames[1] == idx_ld and dur[1, :T].sum() == frames[1]
    want = np.zeros(T, dtype=np.int64)
    want[:16], want[16] = 100, 50  # 16 x 100 + 50 = 1650 = idx_ld
    np.testing.assert_array_equal(dur[1, :T], want)
    assert (np.diff(idx[1]) >= 0).all() and idx[1].min() >= 0 and idx[1].max() < T
    np.testing.assert_array_equal(idx[1], np.repeat(np.arange(T), want))
    np.testing.assert_array_equal(_bits(g[1]), _bits(src[1][:, idx[1]]))
    # rows 0 and 2 against the reference, and against a run without the overflowing row
    keep = [0, 2]
    dur_ref, idx_ref = _align_reference(logits[keep], [lens[b] for b in keep], [speeds[b] for b in keep])
    dur2, frames2, idx2, g2, over2 = hk.alignment(logits[keep], [lens[b] for b in keep], [speeds[b] for b in keep], src[keep],
                                                  idx_ld=idx_ld, Fcap=idx_ld)
    assert over2 == 0
    for j, b in enumerate(keep):
        np.testing.assert_array_equal(dur2[j, :lens[b]], dur_ref[j])
        assert frames2[j] == len(idx_ref[j])
        np.testing.assert_array_equal(dur[b], dur2[j])
        assert frames[b] == frames2[j]
        np.testing.assert_array_equal(idx[b], idx2[j])
        np.testing.assert_array_equal(_bits(g[b]), _bits(g2[j]))
    # two offenders: the word names one of them (the first to get there)
    logits[2] = 12.0
    over3 = hk.alignment(logits, [lens[0], T, T], [1.0, 0.5, 0.25], np.nan_to_num(src), idx_ld=idx_ld, Fcap=idx_ld)[4]
    assert over3 in (2, 3)


# ---- embeddings ----------------------------------------------------------------------------------------------------------------
N_VOCAB = 178


@functools.lru_cache(maxsize=None)
def _embed_tables():
    rng = np.random.default_rng(178)
    return (rng.standard_normal((N_VOCAB, 512), dtype=np.float32), rng.standard_normal((N_VOCAB, 128), dtype=np.float32),
            rng.standard_normal(128, dtype=np.float32), rng.standard_normal((512, 128), dtype=np.float32))


def _embed_reference(ids, lens, T, tables):
    """NumPy float32 indexing; ALBERT in the kernel's association (word + type0) + pos; the sentinel past lens[b]."""
    table, word, type0, pos = tables
    B = len(lens)
    text = np.full((B, 512, T), SENT, dtype=np.float32)
    alb = np.full((B, 128, T), SENT, dtype=np.float32)
    for b, n in enumerate(lens):
        i = np.clip(ids[b, :n], 0, N_VOCAB - 1)
        text[b, :, :n] = table[i].T
        alb[b, :, :n] = ((word[i] + type0[None, :]) + pos[:n]).T
    return text, alb


def _embed_ids(T, lens, stride, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, N_VOCAB, size=(len(lens), stride)).astype(np.int64)
    for b, n in enumerate(lens):
        ids[b, 0], ids[b, n - 1] = (0, N_VOCAB - 1) if b % 2 == 0 else (N_VOCAB - 1, 0)  # both ends of the table, at both ends of a row
    return ids


@pytest.mark.parametrize("T,lens", [(1, [1, 1]), (5, [5, 2, 4]), (130, [130, 1, 97, 129])])
def test_embedding_gathers(T, lens):
    from kokorox_amd import hip_koko as hk
    tables = _embed_tables()
    ids = _embed_ids(T, lens, stride=T + 3, seed=T)
    assert (ids == 0).any() and (ids == N_VOCAB - 1).any()
    text, alb, bad = hk.embed(ids, lens, T, tables[0], tables[1], tables[2], tables[3][:T])
    ref_text, ref_alb = _embed_reference(ids, lens, T, tables)
    assert bad == 0
    np.testing.assert_array_equal(_bits(text), _bits(ref_text))
    np.testing.assert_array_equal(_bits(alb), _bits(ref_alb))


def test_embedding_bad_ids_are_clamped_and_recorded():
    """An id outside the table: both gathers read the nearest row (0 for a negative id, n_vocab - 1 for one too large), and the
    sticky word holds (b << 16 | t) + 1 of an offender -- of THE offender when there is one.  An id past lens[b] is never read."""
    from kokorox_amd import hip_koko as hk
    tables = _embed_tables()
    T, lens = 37, [37, 20, 33]
    base = _embed_ids(T, lens, stride=T + 2, seed=9)
    offenders = {(0, 36): -1, (2, 5): N_VOCAB}

    def run(bad_at):
        ids = base.copy()
        for (b, t), v in bad_at.items():
            ids[b, t] = v
        text, alb, bad = hk.embed(ids, lens, T, tables[0], tables[1], tables[2], tables[3][:T])
        ref_text, ref_alb = _embed_reference(ids, lens, T, tables)  # (the reference clamps as the kernels must)
        np.testing.assert_array_equal(_bits(text), _bits(ref_text))
        np.testing.assert_array_equal(_bits(alb), _bits(ref_alb))
        return bad

    word = lambda b, t: ((b << 16) | t) + 1
    assert run(offenders) in {word(b, t) for b, t in offenders}
    for (b, t), v in offenders.items():
        assert run({(b, t): v}) == word(b, t)
    # out-of-table ids behind an utterance's end, in the row and in the stride padding: not read, not reported
    assert run({(1, 20): -5, (1, 36): 10 ** 12, (2, 33): N_VOCAB, (0, T + 1): -1}) == 0


# ---- style projections ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_style_projections(B):
    """Every AdaIN / AdaLayerNorm projection of a call is one launch over a descriptor list: 128 inputs from one half of the style
    row, outputs back to back.  Bound per output, nothing free in it: a float32 dot product of 128 terms plus the bias, summed in any
    order, is within 129 x 2^-24 x (sum |w_k s_k| + |bias|) of the exact value to first order; twice that covers the higher-order
    terms and the rounding of the products themselves."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(B)
    n_out = [2, 128, 256, 257, 1024, 2180]
    offs = [0, 128, 128, 0, 128, 0]
    styles = rng.standard_normal((B, 256), dtype=np.float32)
    ws = [rng.standard_normal((n, 128), dtype=np.float32) for n in n_out]
    bs = [rng.standard_normal(n, dtype=np.float32) for n in n_out]
    out = hk.style_fc(styles, ws, bs, offs)
    assert out.shape == (B, sum(n_out))
    at = 0
    for w, b, off in zip(ws, bs, offs):
        s = styles[:, off:off + 128].astype(np.float64)
        ref = s @ w.astype(np.float64).T + b.astype(np.float64)[None, :]
        bound = 2 * 129 * 2.0 ** -24 * (np.abs(s) @ np.abs(w.astype(np.float64)).T + np.abs(b.astype(np.float64))[None, :])
        err = np.abs(out[:, at:at + len(b)] - ref)
        print(f"n_out {len(b)} style_off {off}: max err / bound = {(err / bound).max():.3g}")
        assert (err <= bound).all(), (len(b), off, (err / bound).max())
        at += len(b)


# ---- row fills and copies ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,lens,mul,add", [(5, [5, 1, 3], 1, 0), (70, [70, 33, 64], 2, 0), (300, [300, 257, 1], 2, 3), (40, [40, 2, 17], 1, -1)])
def test_row_fills_and_copies(T, lens, mul, add):
    """fill_style_rows_kernel (rows 512..639 of the duration encoder's input = the second half of the style row, over lens[b]
    columns) and copy_rows_kernel (another row stride on each side, lens[b] mul + add columns): exact, and nothing else written."""
    from kokorox_amd import hip_koko as hk
    B, R = len(lens), 66
    rng = np.random.default_rng(T)
    styles = rng.standard_normal((B, 256), dtype=np.float32)
    Ls, Ld = max(lens) * mul + add + 5, max(lens) * mul + add + 40
    src = rng.standard_normal((B, R, Ls), dtype=np.float32)
    fill, cp = hk.rows(styles, lens, T, src, Ld, mul=mul, add=add)
    ref_fill = np.full((B, 640, T), SENT, dtype=np.float32)
    ref_cp = np.full((B, R, Ld), SENT, dtype=np.float32)
    for b, n in enumerate(lens):
        ref_fill[b, 512:, :n] = styles[b, 128:, None]
        ref_cp[b, :, :n * mul + add] = src[b, :, :n * mul + add]
    np.testing.assert_array_equal(_bits(fill), _bits(ref_fill))
    np.testing.assert_array_equal(_bits(cp), _bits(ref_cp))
