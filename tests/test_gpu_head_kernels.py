"""GPU: the back half's kernels that are no conv, each alone through its test hook (include/kokorox_hip_test.h): the harmonic
source across the chunk seams of its phase kernel and under per-utterance noise keys, stft_kernel and the iSTFT head in both
variants of the pair (kx_set_stft_variant), and the up-sampling pool.

The references, the bounds and their derivations are oracle/head_ref.py's; tests/test_head_kernels_cpu.py shows there that a
correct float32 restatement of every kernel passes these very checks and that each wrong one they are written for does not.
The hooks pad the rows as the model does, put NaN wherever a kernel must not read and a sentinel wherever it must not write,
check row padding and guard bytes themselves, and refuse arguments the model could not produce before anything is launched.
Every figure is printed as a fraction of its bound (pytest -s): DESIGN.md section 4 quotes them.
"""
import numpy as np
import pytest
import torch

from oracle import head_ref as H

pytestmark = pytest.mark.gpu

SENT = H.SENT
FRAME_SETS = [pytest.param((1, 3, 5), id="ragged-1-3-5"), pytest.param((3,), id="alone-3-two-blocks")]
VARIANTS = [pytest.param(0, id="onnx"), pytest.param(1, id="torch")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _report(what, got):
    print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in got.items()) + "  (fraction of the bound)")


# ---- harmonic source -------------------------------------------------------------------------------------------------------------
SRC_FRAMES = (513, 60, 1030)  # 1026 steps: the shortest row with a second chunk (of two steps); 2060 steps: three chunks
SRC_TOL = 2e-6                # test_harmonic_source_phase_is_bit_faithful's
_src_refs = {}


def _src_f0():
    rng = np.random.default_rng(3)
    f0 = (rng.standard_normal((3, 2 * max(SRC_FRAMES))) * 150 + 110).astype(np.float32)  # (negative values are in range)
    f0[2, 1000:1060] = 0.0  # an unvoiced stretch across the first chunk seam of the longest row
    f0[0, :40] = 0.0
    return f0


def _src_ref(oracle, b, seed, utt, noise):
    """oracle.source on row b's own f0, computed once per key (1 - 2 s for the long rows)."""
    key = (b, seed, utt, noise)
    if key not in _src_refs:
        f0 = torch.from_numpy(_src_f0()[b, :2 * SRC_FRAMES[b]].copy())
        _src_refs[key] = oracle.source(f0, seed, utt, 1.0 if noise else 0.0, {}).numpy()
    return _src_refs[key]


def _src_weights(oracle):
    return oracle.w["decoder.generator.m_source.l_linear.weight"].numpy(), float(oracle.w["decoder.generator.m_source.l_linear.bias"][0])


@pytest.mark.parametrize("noise", [pytest.param(True, id="noise"), pytest.param(False, id="noise_off")])
def test_source_rows_beyond_one_chunk_match_the_oracle(oracle, noise):
    """Every row of a ragged batch against oracle.source on its own f0: the float64 running sum of source_phase_kernel carried
    over one and over two chunk seams (phases of 1e5 rad: a carry lost or rounded there decorrelates every harmonic behind it)."""
    from kokorox_amd import hip_koko as hk
    lw, lb = _src_weights(oracle)
    y = hk.harmonic_source_ragged(_src_f0(), SRC_FRAMES, lw, lb, seed=7, utt_base=5, noise_off=not noise)
    for b, f in enumerate(SRC_FRAMES):
        d = np.abs(y[b, :600 * f] - _src_ref(oracle, b, 7, 5 + b, noise))
        seam = 300 * H.SRC_CH * ((2 * f - 1) // H.SRC_CH)  # the first sample of the row's last chunk
        print(f"source, {f} frames, noise {noise}: max|d| {d.max():.2e} of {SRC_TOL:.0e}, {d[seam:].max():.2e} in the last chunk")
        assert d.max() < SRC_TOL, (b, f)
        assert np.all(y[b, 600 * f:] == SENT), b


def test_source_batch_invariance_and_per_utterance_keys(oracle):
    from kokorox_amd import hip_koko as hk
    lw, lb = _src_weights(oracle)
    f0 = _src_f0()
    y = hk.harmonic_source_ragged(f0, SRC_FRAMES, lw, lb, seed=7, utt_base=5)
    for b, f in enumerate(SRC_FRAMES):  # alone, under the key it had in the batch: the same bits
        one = hk.harmonic_source_ragged(f0[b:b + 1, :2 * f], [f], lw, lb, seed=7, utt_base=5 + b)
        assert np.array_equal(_bits(one[0]), _bits(y[b, :600 * f])), b
    # the dispatcher's keys: row b draws (utt_seeds[b], utt_index[b]) whatever seed and utt_base say
    seeds, index = [(1 << 33) + 1, 7, 99], [3, 6, 4]
    k = hk.harmonic_source_ragged(f0, SRC_FRAMES, lw, lb, seed=1234, utt_base=77, utt_seeds=seeds, utt_index=index)
    for b, f in enumerate(SRC_FRAMES):
        assert np.abs(k[b, :600 * f] - _src_ref(oracle, b, seeds[b], index[b], True)).max() < SRC_TOL, b
        assert np.all(k[b, 600 * f:] == SENT), b
    assert np.array_equal(_bits(k[1]), _bits(y[1]))  # ((7, 6) is what row 1 drew under (seed 7, utt_base 5))
    # no index beside the seeds: utterance 0 of every seed
    k0 = hk.harmonic_source_ragged(f0, SRC_FRAMES, lw, lb, seed=1234, utt_base=77, utt_seeds=seeds)
    z = hk.harmonic_source_ragged(f0, SRC_FRAMES, lw, lb, seed=1234, utt_base=77, utt_seeds=seeds, utt_index=[0, 0, 0])
    assert np.array_equal(_bits(k0), _bits(z))
    assert np.abs(k0[1, :600 * 60] - _src_ref(oracle, 1, 7, 0, True)).max() < SRC_TOL
    assert not np.array_equal(_bits(k0[1]), _bits(k[1]))


# ---- forward STFT ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "small", "edges"])
@pytest.mark.parametrize("frames", FRAME_SETS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_stft_against_float64_in_the_re_im_domain(variant, frames, kind):
    """mag cos(ph) and mag sin(ph), rebuilt in float64 from what the kernel stored, against the exact transform of the same row:
    well conditioned in every bin, so none is left out.  Rows of 1, 3 and 5 frames in one batch (the replicate padding must clamp
    to the row's own last sample: NaN follows it), 361 STFT frames alone (two blocks); random rows, rows at 1e-3 of that scale,
    and rows whose first and last 15 samples dominate frames 0, 1, nf - 2 and nf - 1."""
    from kokorox_amd import hip_koko as hk
    rows = H.stft_rows(frames, kind, seed=10)
    har = hk.stft(rows, frames, variant)
    worst = {}
    for b, f in enumerate(frames):
        nf = 120 * f + 1
        mag, ph = har[b, :11, :nf], har[b, 11:, :nf]
        assert np.isfinite(mag).all() and np.isfinite(ph).all() and np.abs(ph).max() <= H.PI32, b
        got = H.stft_check(mag, ph, rows[b, :600 * f], variant)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in got.items()}
        assert max(got.values()) <= 1.0, (b, got)
        assert np.all(har[b, :, nf:] == SENT), b
    _report(f"stft variant {variant}, frames {frames}, {kind}", worst)


@pytest.mark.parametrize("variant", VARIANTS)
def test_stft_exact_cases(variant):
    from kokorox_amd import hip_koko as hk
    frames = (1, 3, 5)
    pi_bits = _bits(H.PI32)
    rows = np.zeros((3, 3000), dtype=np.float32)
    har = hk.stft(rows, frames, variant)
    for b, f in enumerate(frames):
        nf = 120 * f + 1
        want = np.sqrt(np.float32(1e-14)) if variant == 0 else np.float32(0)
        assert np.all(har[b, :11, :nf] == want) and np.all(har[b, 11:, :nf] == 0), b
    # a constant negative row: bin 0 sits on the negative real axis with an imaginary part of exactly zero
    har = hk.stft(np.full((3, 3000), -0.75, dtype=np.float32), frames, variant)
    for b, f in enumerate(frames):
        nf = 120 * f + 1
        ph0, ph10 = har[b, 11, :nf], har[b, 21, :nf]
        if variant == 0:
            assert np.all(_bits(ph0) == pi_bits), b
            # bin 10 of a constant row is zero in exact arithmetic (the window sums to zero against (-1)^n): its real part is
            # rounding residue of either sign, its imaginary part an exact zero (the table's sines are), so its phase is 0 or the
            # forced pi, bit for bit, and nothing else
            assert np.all((ph10 == 0) | (_bits(ph10) == pi_bits)), b
            print(f"constant row, {f} frames: bin 10 phase is pi in {int((ph10 != 0).sum())} of {nf} frames, magnitude up to {har[b, 10, :nf].max():.2e}")
        else:
            assert np.all(np.abs(np.abs(ph0.astype(np.float64)) - np.pi) <= H.ULP2 * np.pi), b
    # bin 10 on the negative real axis for certain: x[p] = -0.75 (-1)^p gives re = -7.5 on the even interior frames, +7.5 on the odd
    alt = np.tile((-0.75 * (-1.0) ** np.arange(3000)).astype(np.float32), (3, 1))
    har = hk.stft(alt, frames, variant)
    for b, f in enumerate(frames):
        nf = 120 * f + 1
        ph10 = har[b, 21, :nf]
        if variant == 0:
            assert np.all(_bits(ph10[2:-2:2]) == pi_bits) and np.all(ph10[3:-2:2] == 0), b
        else:
            assert np.all(np.abs(np.abs(ph10[2:-2:2].astype(np.float64)) - np.pi) <= H.ULP2 * np.pi) and np.all(ph10[3:-2:2] == 0), b
        assert np.all(np.abs(har[b, 10, 2:nf - 2].astype(np.float64) - 7.5) <= 7.5 * (H.gamma(21) + 6 * H.U)), b


# ---- iSTFT head ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", FRAME_SETS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_istft_head_against_float64(variant, frames):
    """istft_spec_kernel against float64 exp / sin / cos of the same float32 logits (magnitude logits uniform on [-6, 2], phase
    logits on [-20, 20]); istft_ola_kernel against the float64 inverse of the spectrum the first kernel stored, under the
    arithmetic bound alone.  The first ten samples (frame 0 only behind them), the last hop (cut at frame nf - 1) and the seam of
    the 256-hop blocks at sample 1280 are inside the compared range; a second assertion names them."""
    from kokorox_amd import hip_koko as hk
    cp = H.head_logits(frames, seed=20)
    spec, audio = hk.istft_head(cp, frames, variant)
    worst = {}
    for b, f in enumerate(frames):
        nf, ns = 120 * f + 1, 600 * f
        re, im = spec[b, :11, :nf], spec[b, 11:, :nf]
        got = H.spec_check(re, im, cp[b, :11, :nf], cp[b, 11:, :nf])
        assert max(got.values()) <= 1.0, (b, got)
        got.update(H.istft_check(audio[b, :ns], re, im, variant))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in got.items()}
        assert got["audio"] <= 1.0, (b, got)
        for name in H.istft_edges(nf):
            assert got[name] <= 1.0, (b, name, got)
        assert np.all(spec[b, :, nf:] == SENT) and np.all(audio[b, ns:] == SENT), b
    _report(f"istft head variant {variant}, frames {frames}", worst)


# ---- up-sampling pool ------------------------------------------------------------------------------------------------------------
def test_pool_up2_against_float64():
    """B = 3, C = 5, lens (1, 128, 129): one column has nothing but the right edge (v[m + 1] = 0 at m = L - 1), 129 give 258
    outputs across a block seam; slope 0.2 on pre-activations of both signs; NaN behind every row and in the planes' unused slots."""
    from kokorox_amd import hip_koko as hk
    x, lens, norm, w, bias, slope = H.pool_case()
    y = hk.pool_up2(x, lens, norm, w, bias, slope, n_bs=x.shape[1] + 3)
    for b, L in enumerate(lens):
        got = H.pool_check(y[b, :, :2 * L], x[b, :, :L], norm[0, b], norm[1, b], norm[2, b], w, bias, slope)
        _report(f"pool, {L} columns", got)
        assert got["pool"] <= 1.0, (b, got)
        assert np.all(y[b, :, 2 * L:] == SENT), b


# ---- the hooks refuse what the model could not produce ---------------------------------------------------------------------------
def test_hooks_refuse_arguments_out_of_range():
    """Nothing is launched on a length outside its row: KX_ERR_INVALID (1) before any device work."""
    from kokorox_amd import hip_koko as hk
    x, lens, norm, w, bias, slope = H.pool_case()
    lw = np.zeros(9, dtype=np.float32)
    calls = [
        lambda: hk.stft(np.zeros((2, 600), dtype=np.float32), [1, 0], 0),
        lambda: hk.stft(np.zeros((2, 599), dtype=np.float32), [1, 1], 0),      # rows shorter than 600 Fmax
        lambda: hk.stft(np.zeros((1, 600), dtype=np.float32), [1], 2),         # no such variant
        lambda: hk.stft(np.zeros((1, 600 * 65), dtype=np.float32), [65], 0),   # beyond the hook's size cap
        lambda: hk.istft_head(np.zeros((2, 22, 121), dtype=np.float32), [1, -3], 1),
        lambda: hk.pool_up2(x, (1, 128, 130), norm, w, bias, slope),
        lambda: hk.pool_up2(x, (0, 128, 129), norm, w, bias, slope),
        lambda: hk.pool_up2(x, lens, norm, w, bias, slope, n_bs=x.shape[1]),   # the planes' stride must exceed C
        lambda: hk.harmonic_source_ragged(np.zeros((2, 8), dtype=np.float32), [4, 0], lw, 0.0),
        lambda: hk.harmonic_source_ragged(np.zeros((1, 8), dtype=np.float32), [4], lw, 0.0, utt_index=[1]),  # an index without seeds
    ]
    for i, call in enumerate(calls):
        with pytest.raises(hk.KokoroxHipError) as e:
            call()
        assert e.value.code == 1, i
