"""No GPU: the references, bounds and stand-ins of oracle/head_ref.py, which tests/test_gpu_head_kernels.py holds the harmonic
source, the STFT pair, the iSTFT head and the up-sampling pool against.

Three kinds of assertion.  The float64 references equal the definitions they claim (torch.stft / torch.istft for variant 1, the
oracle's stft / istft for variant 0, the oracle's source for the restated one).  A float32 numpy stand-in of every kernel, same
operation order, passes exactly the check functions the GPU tests call, so the a-priori bounds are not too tight for correct
float32 code.  And every way in which a kernel could be wrong that the GPU tests are there to catch is applied to its stand-in
and must be rejected by the same check: one assertion per mutation.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import head_ref as H
from oracle import kokoro_ref as R

FRAME_SETS = [(1, 3, 5), (3,)]  # the batches of the GPU file: 121, 361 and 601 STFT frames; 361 alone has a second block


def _worst(d):
    return max(d.values())


# ---- the references are the definitions ------------------------------------------------------------------------------------------
def test_forward_reference_is_torch_stft_and_the_oracle():
    x = np.random.default_rng(0).standard_normal(1800)
    re, im, are, aim = H.stft_ref(x)
    w = torch.hann_window(20, periodic=True, dtype=torch.float64)
    st = torch.stft(torch.from_numpy(x), 20, 5, 20, window=w, center=True, pad_mode="replicate", return_complex=True).numpy()
    assert re.shape == (11, 361) and np.abs(re + 1j * im - st).max() < 1e-13
    # the oracle's conv form in float64 carries float32-rounded tables: within u sum |x T| of the exact ones
    for variant, name in ((0, "onnx"), (1, "torch")):
        o = R.KokoroOracle({}, dtype=torch.float64, stft_variant=name)
        har = o.stft(torch.from_numpy(x)).numpy()
        b = H.stft_bounds(x, variant)
        z = har[:11] * np.exp(1j * har[11:])
        assert np.all(np.abs(z.real - b["re"]) <= H.U * are + (b["mag"] - np.hypot(b["re"], b["im"])) + 1e-15)
        assert np.all(np.abs(z.imag - b["im"]) <= H.U * aim + (b["mag"] - np.hypot(b["re"], b["im"])) + 1e-15)
        assert np.all(np.abs(har[:11] - b["mag"]) <= H.U * np.hypot(are, aim) + 1e-15)


def test_inverse_reference_is_torch_istft_and_the_oracle():
    rng = np.random.default_rng(1)
    re, im = rng.standard_normal((11, 361)), rng.standard_normal((11, 361))
    w = torch.hann_window(20, periodic=True, dtype=torch.float64)
    yt = torch.istft(torch.from_numpy(re + 1j * im), 20, 5, 20, window=w, center=True).numpy()
    y1, a1 = H.istft_ref(re, im, 1)
    assert y1.shape == (1800,) and np.abs(y1 - yt).max() < 1e-14
    mag, ph = np.hypot(re, im), np.arctan2(im, re)
    for variant, name in ((0, "onnx"), (1, "torch")):
        o = R.KokoroOracle({}, dtype=torch.float64, stft_variant=name)
        yo = o.istft(torch.from_numpy(mag), torch.from_numpy(ph)).numpy()
        y, a = H.istft_ref(re, im, variant)
        assert np.all(np.abs(y - yo) <= 6 * H.U * a + 1e-15)  # (float32-rounded tables, and in variant 1 a rounded envelope)
    # the two variants differ where they should: the doubled interior bins and the division
    assert np.abs(H.istft_ref(re, im, 0)[0] - y1).max() > 0.1


def test_variant_1_round_trip_is_the_identity():
    x = np.random.default_rng(2).standard_normal(600)
    re, im, _, _ = H.stft_ref(x)
    assert np.abs(H.istft_ref(re, im, 1)[0] - x).max() < 1e-14


def test_pool_reference_is_the_tap_formula():
    rng = np.random.default_rng(3)
    C, L = 4, 9
    x, w = rng.standard_normal((C, L)), rng.standard_normal((C, 3))
    one, zero = np.ones(C), np.zeros(C)
    y, _ = H.pool_ref(x, zero, one, zero, w, zero, 1.0)  # (slope 1, identity affine: v = x)
    assert np.abs(y[:, 0::2] - x * w[:, 1:2]).max() < 1e-15
    nxt = np.concatenate([x[:, 1:], np.zeros((C, 1))], axis=1)
    assert np.abs(y[:, 1::2] - (x * w[:, 2:3] + nxt * w[:, 0:1])).max() < 1e-15


# ---- forward: stand-in and mutations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("frames", FRAME_SETS)
@pytest.mark.parametrize("kind", ["random", "small", "edges"])
def test_forward_stand_in_passes_and_its_mutations_do_not(variant, frames, kind):
    rows = H.stft_rows(frames, kind, seed=10)
    for b, f in enumerate(frames):
        L = 600 * f
        x = rows[b, :L]
        mag, ph = H.stft_f32(rows[b], L, variant)
        got = H.stft_check(mag, ph, x, variant)
        assert _worst(got) <= 1.0, got
        assert np.isfinite(ph).all() and np.abs(ph).max() <= H.PI32
        # the clamp goes to the row stride, not to the row's own last sample
        assert not _worst(H.stft_check(*H.stft_f32(rows[b], L, variant, clamp=rows.shape[1] - 1), x, variant)) <= 1.0
        # ... even when what follows the row is finite data
        nxt = rows[b].copy()
        nxt[L:] = 0.25
        assert not _worst(H.stft_check(*H.stft_f32(nxt, L, variant, clamp=rows.shape[1] - 1), x, variant)) <= 1.0
        # a wrong edge frame
        assert not _worst(H.stft_check(*H.stft_f32(rows[b], L, variant, shift=9), x, variant)) <= 1.0


def test_forward_check_separates_the_variants_on_a_quiet_row():
    """The epsilon under the root is visible to the magnitude check wherever the spectrum is small: a variant-1 magnitude fails
    variant 0's check and the other way round."""
    x = (np.random.default_rng(11).standard_normal(600) * 1e-7).astype(np.float32)
    for variant in (0, 1):
        assert _worst(H.stft_check(*H.stft_f32(x, 600, variant), x, variant)) <= 1.0
        assert not H.stft_check(*H.stft_f32(x, 600, 1 - variant), x, variant)["mag2"] <= 1.0


def test_forward_exact_cases_of_the_stand_in():
    zero = np.zeros(600, dtype=np.float32)
    mag, ph = H.stft_f32(zero, 600, 0)
    assert np.all(mag == np.sqrt(np.float32(1e-14))) and np.all(ph == 0)
    mag, ph = H.stft_f32(zero, 600, 1)
    assert np.all(mag == 0) and np.all(ph == 0)
    neg = np.full(600, -0.75, dtype=np.float32)
    mag, ph = H.stft_f32(neg, 600, 0)
    assert np.all(ph[0].view(np.uint32) == H.PI32.view(np.uint32))
    # bin 10 of a constant row is an exact zero in exact arithmetic (the window sums to zero against (-1)^n): its real part is
    # rounding residue of either sign, its imaginary part an exact zero, its phase 0 or the forced pi and nothing else
    assert np.all((ph[10] == 0) | (ph[10].view(np.uint32) == H.PI32.view(np.uint32)))
    # the forced branch on bin 10 where its sign is determined: x[p] = -(-1)^p gives re = -10 on the even interior frames
    alt = (-0.75 * (-1.0) ** np.arange(600)).astype(np.float32)
    mag, ph = H.stft_f32(alt, 600, 0)
    assert np.all(ph[10, 2:-2:2].view(np.uint32) == H.PI32.view(np.uint32)) and np.all(ph[10, 3:-2:2] == 0)
    mag, ph = H.stft_f32(neg, 600, 1)
    assert np.all(np.abs(np.abs(ph[0].astype(np.float64)) - np.pi) <= H.ULP2 * np.pi)


# ---- iSTFT head: stand-in and mutations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("frames", FRAME_SETS)
def test_inverse_stand_in_passes_and_its_mutations_do_not(variant, frames):
    cp = H.head_logits(frames, seed=20)
    for b, f in enumerate(frames):
        nf = 120 * f + 1
        a, p = cp[b, :11, :nf], cp[b, 11:, :nf]
        re, im = H.spec_f32(a, p)
        assert _worst(H.spec_check(re, im, a, p)) <= 1.0
        assert not _worst(H.spec_check(re, im * np.float32(1 + 2e-6), a, p)) <= 1.0  # (2e-6 of scale is seen)
        got = H.istft_check(H.istft_f32(re, im, variant), re, im, variant)
        assert _worst(got) <= 1.0, got
        bad = lambda **kw: not H.istft_check(H.istft_f32(re, im, variant, **kw), re, im, variant)["audio"] <= 1.0
        if variant == 1:
            assert bad(table_variant=(0, 0))    # without the interior doubling
            assert bad(divide=False)            # without the envelope division
        else:
            assert bad(table_variant=(1, 1))    # variant 0 with the doubled interior bins
            assert bad(divide=True)             # variant 0 with the envelope division
        if nf > 256:
            for drop, name in (("hi", "block seam at sample 1280"), ("lo", "block seam at sample 1280")):
                got = H.istft_check(H.istft_f32(re, im, variant, drop=drop), re, im, variant)
                assert not got["audio"] <= 1.0 and not got[name] <= 1.0
                assert got["first ten samples"] <= 1.0 and got["last hop"] <= 1.0  # (the named edges say which one broke)


def test_imaginary_parts_of_bins_0_and_10_do_not_count():
    """torch.istft ignores the imaginary parts of the two real bins.  Variant 0 sums every bin's sine row, but the sines of bins 0
    and 10 are exact zeros in the exact tables (sin 0, sin pi n), so a kernel that "kept" them with their own coefficients is the
    same kernel: that mutation cannot be told apart by any finite input, and what can be is one that keeps them with coefficients
    that are not zero."""
    cp = H.head_logits((1,), seed=21)[0]
    re, im = H.spec_f32(cp[:11], cp[11:])
    im2 = im.copy()
    im2[[0, 10]] = 1e3
    for variant in (0, 1):
        assert np.array_equal(H.istft_ref(re, im, variant)[0], H.istft_ref(re, im2, variant)[0])
        assert np.array_equal(H.istft_f32(re, im, variant), H.istft_f32(re, im2, variant))
    # a kernel that kept them with a non-zero coefficient (a table of sines at the wrong bins) is rejected
    keep = H.INV[1][1].copy()
    try:
        H.INV[1][1][:, [0, 10]] = H.INV[1][1][:, [1, 9]]
        wrong = H.istft_f32(re, im, 1)
    finally:
        H.INV[1][1][:] = keep
    assert not H.istft_check(wrong, re, im, 1)["audio"] <= 1.0


# ---- pool: stand-in and mutations ------------------------------------------------------------------------------------------------
def test_pool_stand_in_passes_and_its_mutations_do_not():
    x, lens, norm, w, bias, slope = H.pool_case()
    for b, L in enumerate(lens):
        row = np.full((x.shape[1], x.shape[2] + 1), np.nan, dtype=np.float32)
        row[:, :L] = x[b, :, :L]
        args = (x[b, :, :L], norm[0, b], norm[1, b], norm[2, b], w, bias, slope)
        pre = (x[b, :, :L] - norm[0, b][:, None]) * norm[1, b][:, None] + norm[2, b][:, None]
        assert L == 1 or ((pre > 0).any() and (pre < 0).any())
        run = lambda r, **kw: H.pool_f32(r, L, norm[0, b], norm[1, b], norm[2, b], w, bias, slope, **kw)
        assert _worst(H.pool_check(run(row), *args)) <= 1.0
        assert not _worst(H.pool_check(run(row, swap=True), *args)) <= 1.0       # w0 and w2 swapped
        assert not _worst(H.pool_check(run(row, read_past=True), *args)) <= 1.0  # v[m + 1] read at m = L - 1 (NaN behind the row)
        nxt = row.copy()
        nxt[:, L:] = 0.5
        assert not _worst(H.pool_check(run(nxt, read_past=True), *args)) <= 1.0  # ... and finite data behind it


# ---- source: the running sum across chunk seams ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _source_oracle():
    rng = np.random.default_rng(40)
    w = {"decoder.generator.m_source.l_linear.weight": (rng.standard_normal((1, 9)) * 0.3).astype(np.float32),
         "decoder.generator.m_source.l_linear.bias": np.array([0.05], dtype=np.float32)}
    return R.KokoroOracle(w)


def test_source_stand_in_passes_and_its_mutations_do_not():
    """513 frames: 1026 steps, the shortest row with a second chunk.  The restated source with torch.cumsum is the oracle's, bit
    for bit; with the kernel's chunked float64 running sum it stays within the GPU test's 2e-6 of it (it is in fact the same
    bits); a sum that restarts in the second chunk or crosses the seam as a float32 does not."""
    o = _source_oracle()
    rng = np.random.default_rng(41)
    f0 = torch.from_numpy((rng.standard_normal(1026) * 150 + 110).astype(np.float32))
    ref = o.source(f0, 7, 5, 1.0, {}).numpy()
    assert np.array_equal(H.source_with_cumsum(o, f0, 7, 5, 1.0).numpy(), ref)
    err = lambda **kw: np.abs(H.source_with_cumsum(o, f0, 7, 5, 1.0, lambda r: H.cumsum_chunked(r, **kw)).numpy() - ref)
    assert err().max() < 2e-6
    e = err(restart=True)
    assert e[:600 * 512 - 300].max() < 2e-6 and not e.max() < 2e-6   # (the first chunk is untouched: the last two steps break)
    assert not err(carry32=True).max() < 2e-6
