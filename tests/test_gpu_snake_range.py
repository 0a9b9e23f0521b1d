"""GPU: the snake input activation v + sin^2(alpha v) / alpha of the conv kernels, over the two axes along which it is
conditioned: alpha at O(1) activations (1 / alpha multiplies whatever absolute error sin^2 carries) and the size of the
argument alpha v (range reduction; the valid input domain of the hardware trig instructions).

Every conv form is reached through the hooks hk.conv1d / hk.conv1d_full: hook mode 0 (f32: sinf, squared), 1 (f16x3, the
plan's choice), 2 (LDS forms) and 3 (direct-A) -- the polynomial sin_sq of conv_f16x3_common.h and its restatement in
conv_f16x3_da.hip -- and 1 | F8, 3 | F8 (f16f8, the library's default mode, on its two tile widths: the hardware-trig form).
The reference is torch float64 on the float32 inputs widened to double (alpha included, the AdaIN affine in double).
Bounds are the classes the project states for these forms at alpha ~ 1 (tests/test_gpu_kernels.py), unchanged along alpha.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F8 = 0x200  # hook mode bit: the layer carries the 8-bit cross image of its weights (f16f8)
POLY_MODES = (0, 1, 2, 3)
F8_MODES = (1 | F8, 3 | F8)
MODE_NAMES = {0: "f32", 1: "f16x3", 2: "f16x3lds", 3: "f16x3da", 1 | F8: "f16f8/128", 3 | F8: "f16f8/192"}
ALPHAS = [0.01, 0.02, 0.05, 0.2, 1.0, 5.0, 20.0]
# (k, dil, Cin, Cout, L): the smallest shapes at which each f16f8 instantiation runs (11, 7 and 3 taps; Cin = 24: a partial second
# chunk; 128 and 256 rows; L = 517 and 193: more than one column tile on either tile width; 65: one) -- all among _f8_cases() of
# tests/test_gpu_kernels.py.  The first chunk pair of a tile goes through the staging path, later ones through the dealt-out transform.
SHAPES = [(11, 3, 128, 128, 517), (7, 1, 24, 128, 193), (3, 5, 256, 256, 65)]
POLY_MAX = 3e-5             # modes 0 .. 3: test_conv1d_fused_adain_activation's bound
F8_MAX, F8_RMS = 4e-4, 3e-5  # f16f8: test_f16f8_form_against_float64's bounds


def _snake64(x, norm, alpha):
    """float64: AdaIN affine, then the snake (x [B,Cin,L], norm [3,B,Cin], alpha [Cin]: float32 values widened to double)."""
    n = torch.from_numpy(norm).double()
    v = (torch.from_numpy(x).double() - n[0][:, :, None]) * n[1][:, :, None] + n[2][:, :, None]
    a = torch.from_numpy(alpha).double()[None, :, None]
    return v + (1 / a) * torch.sin(a * v) ** 2


class _Case:
    """One ragged conv problem (B = 2, lens = [L, 2L // 3], padded rows, the flat tile list when L % 4 == 1, as
    test_f16f8_form_against_float64 sets them) and its float64 reference, computed once for all modes."""

    def __init__(self, shape, alpha, x, norm, seed):
        k, d, Cin, Cout, L = shape
        rng = np.random.default_rng(seed)
        self.x, self.norm, self.alpha = x, norm, alpha
        self.w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
        self.b = rng.standard_normal(Cout, dtype=np.float32)
        p = (k - 1) // 2 * d
        self.lens = np.array([L, (2 * L) // 3], dtype=np.int32)
        v = _snake64(x, norm, alpha)
        self.ref = np.zeros((2, Cout, L))
        for i in range(2):
            n = int(self.lens[i])
            self.ref[i, :, :n] = F.conv1d(v[i:i + 1, :, :n], torch.from_numpy(self.w).double(), torch.from_numpy(self.b).double(),
                                          padding=p, dilation=d).numpy()[0]
        self.valid = np.broadcast_to(np.arange(L)[None, None, :] < self.lens[:, None, None], self.ref.shape)
        self.scale = max(1.0, float(np.sqrt((self.ref[self.valid] ** 2).mean())))
        self.ref_rms = float(np.sqrt((self.ref[self.valid] ** 2).mean()))
        self.kw = dict(pad=p, dil=d, act=2, alpha=alpha, norm=norm, lens=self.lens, pad_ld=True, flat=(L % 4 == 1))

    def run(self, mode):
        """-> (y, max |err|, rms err) over the valid columns; the columns past lens[b] must be exactly 0."""
        from kokorox_amd import hip_koko as hk
        y = hk.conv1d_full(self.x, self.w, self.b, mode=mode, **self.kw)
        assert np.all(y[~self.valid] == 0.0), MODE_NAMES[mode]
        err = (y - self.ref)[self.valid]
        return y, float(np.abs(err).max()), float(np.sqrt((err ** 2).mean()))


def _inputs(shape, seed):
    """x ~ N(0,1) and AdaIN planes (N(0,1), 1 + 0.2 N(0,1), N(0,1)): v is O(1) whatever alpha is."""
    _, _, Cin, _, L = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, Cin, L), dtype=np.float32)
    norm = rng.standard_normal((3, 2, Cin), dtype=np.float32)
    norm[1] = 1.0 + 0.2 * norm[1]
    return x, norm


def _check_classes(case, tag):
    """Every mode inside its class; both f16f8 tile widths the same bits."""
    ys = {}
    for mode in POLY_MODES + F8_MODES:
        ys[mode], emax, erms = case.run(mode)
        print(f"{tag}, {MODE_NAMES[mode]:>9}: max {emax / case.scale:.2e}, rms {erms / case.scale:.2e} (of scale {case.scale:.3g})")
        if mode in F8_MODES:
            assert emax < F8_MAX * case.scale, (tag, MODE_NAMES[mode], emax / case.scale)
            assert erms < F8_RMS * case.scale, (tag, MODE_NAMES[mode], erms / case.scale)
        else:
            assert emax < POLY_MAX * case.scale, (tag, MODE_NAMES[mode], emax / case.scale)
    if case.ref.shape[1] >= 128:
        np.testing.assert_array_equal(ys[1 | F8], ys[3 | F8])  # whichever path transformed a chunk: the same bits
    return ys


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"k{s[0]}")
def test_shapes_reach_each_f16f8_instantiation_on_both_tile_widths(shape):
    """What SHAPES claims, from the plan the hook launched: the F8 form with this tap count, 128 columns by hook mode 1, 192 by mode 3."""
    from kokorox_amd import hip_koko as hk
    k, d, Cin, Cout, L = shape
    x, norm = _inputs(shape, 5)
    case = _Case(shape, np.ones(Cin, dtype=np.float32), x, norm, 6)
    for mode, bn in ((1 | F8, 128), (3 | F8, 192)):
        out = hk.conv1d_opts(x, case.w, case.b, mode=mode, **case.kw)
        plan = out["plan"]
        assert (plan["form"], plan["kt"], plan["bn"]) == ("DA_F8", k, bn), plan
        np.testing.assert_array_equal(out["y"], case.run(mode)[0])


def _alpha_cases():
    cases = [pytest.param(s, a, id=f"k{s[0]}-a{a:g}") for s in SHAPES for a in ALPHAS]
    return cases + [pytest.param(SHAPES[0], None, id=f"k{SHAPES[0][0]}-loguniform")]


@pytest.mark.parametrize("shape,a", _alpha_cases())
def test_snake_conv_error_is_flat_in_alpha(shape, a):
    """The conv forms' error classes hold at every alpha from 0.01 to 20, the same alpha on every channel (a well-conditioned
    channel cannot dilute a bad one), and per channel log-uniform over that range.

    The hardware cosine's ABSOLUTE error becomes an activation error ~ 1.5e-6 / alpha, whatever v is: at alpha = 0.01 a model of it
    put the f16f8 forms at 9e-5 rms, three times their class."""
    k, d, Cin, Cout, L = shape
    seed = k * 1009 + Cin + (0 if a is None else ALPHAS.index(a) + 1)
    x, norm = _inputs(shape, seed)
    if a is None:
        alpha = np.exp(np.random.default_rng(seed + 1).uniform(np.log(0.01), np.log(20.0), Cin)).astype(np.float32)
    else:
        alpha = np.full(Cin, a, dtype=np.float32)
    _check_classes(_Case(shape, alpha, x, norm, seed + 2), f"k {k}, alpha {'log-uniform' if a is None else a}")


# ---- the activation alone: a float32 restatement of sin_sq / in_act (conv_f16x3_common.h), every fma in float64, rounded once

def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; one rounding to double, one to float."""
    return _f32(a.astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64) + np.asarray(c, dtype=np.float32).astype(np.float64))


def _sin_sq32(t):
    n = np.rint(t * np.float32(0.318309886183790672))
    r = _fma32(n, np.float32(-3.14159274101257324), t)
    r = _fma32(n, np.float32(8.74227765734758578e-08), r)
    z = r * r
    p = _fma32(z, np.float32(-3.6197402550897095e-06), np.float32(1.3928599946666651e-04))
    p = _fma32(z, p, np.float32(-3.1722760759294033e-03))
    p = _fma32(z, p, np.float32(4.4443082064390182e-02))
    p = _fma32(z, p, np.float32(-3.3333304524421692e-01))
    p = _fma32(z, p, np.float32(1.0))
    return z * p


def _snake32(x, norm, alpha):
    """The kernels' own arithmetic in float32: fma(x - mean, scale, shift), then fma(1 / alpha, sin_sq(alpha v), v)."""
    v = _fma32(x - norm[0][:, :, None], norm[1][:, :, None], norm[2][:, :, None])
    al = alpha[None, :, None]
    ial = (np.float32(1.0) / alpha)[None, :, None]
    assert v.dtype == np.float32 and ial.dtype == np.float32
    return _fma32(ial, _sin_sq32(al * v), v)


@pytest.mark.parametrize("a", ALPHAS)
def test_snake_alone_at_float32_resolution(a):
    """An identity centre tap makes the conv's output the activation itself, so the class bounds' two orders of slack are gone: a wrong
    1 / alpha, a dropped low part of pi, or a restatement in the dealt-out transform that drifted from sin_sq would show.

    The bound is derived, not fixed: e_ref is the worst error against float64 of a float32 restatement of the kernels' arithmetic on
    these very inputs; a kernel may be off by 3 e_ref (fma contraction differences between host and device; sinf instead of the
    polynomial in mode 0) + 2^-21 |ref| (the split-f16 product and the output rounding)."""
    from kokorox_amd import hip_koko as hk
    C, L = 128, 300
    x, norm = _inputs((3, 1, C, C, L), 300 + ALPHAS.index(a))
    alpha = np.full(C, a, dtype=np.float32)
    w = np.zeros((C, C, 3), dtype=np.float32)
    w[np.arange(C), np.arange(C), 1] = 1.0
    ref = _snake64(x, norm, alpha).numpy()
    e_ref = float(np.abs(_snake32(x, norm, alpha).astype(np.float64) - ref).max())
    # (the restatement itself is float32 rounding and nothing more: |x - mean| < 8 and |v| < 16 round by at most 4.8e-7 and 9.5e-7,
    # the snake's slope is at most 2, its result rounds once more: 4.4e-6 at the very worst)
    assert 0.0 < e_ref < 5e-6
    bound = 3.0 * e_ref + 2.0 ** -21 * np.abs(ref)
    for mode in POLY_MODES:
        y = hk.conv1d(x, w, None, pad=1, act=2, alpha=alpha, norm=norm, mode=mode)
        err = np.abs(y - ref)
        print(f"alpha {a:g}, {MODE_NAMES[mode]:>8}: e_ref {e_ref:.2e}, kernel max |err| {err.max():.2e}, worst err / bound {(err / bound).max():.2f}")
        assert np.all(err <= bound), (a, MODE_NAMES[mode], float(err.max()), float((err / bound).max()))


# ---- large arguments

BIG = SHAPES[0]


def _big_inputs(sigma, clip, seed):
    """v = sigma x exactly (mean 0, scale sigma, shift 0), x ~ N(0,1) clipped so that |v| <= clip."""
    _, _, Cin, _, L = BIG
    rng = np.random.default_rng(seed)
    x = np.clip(rng.standard_normal((2, Cin, L), dtype=np.float32), -clip / sigma, clip / sigma).astype(np.float32)
    norm = np.zeros((3, 2, Cin), dtype=np.float32)
    norm[1] = sigma
    return x, norm


@pytest.mark.parametrize("a", [5.0, 20.0])
def test_snake_conv_large_arguments_inside_the_trig_domain(a):
    """v ~ N(0, 12^2), clipped to |v| <= 35: at alpha = 20 the argument alpha v reaches 700 rad = 111 turns of sin, 223 of the
    cosine of the doubled angle -- inside +-256 turns, the hardware instructions' input domain, and inside the e4m3 window.  The
    polynomial's two-part reduction runs at n ~ 200, the hardware's own reduction far beyond |t| <= 40, where
    tools/probes/sin_accuracy.hip swept it.  All six modes stay in their classes (times scale, which grows with v)."""
    x, norm = _big_inputs(12.0, 35.0, 1200 + int(a))
    case = _Case(BIG, np.full(BIG[2], a, dtype=np.float32), x, norm, 1300 + int(a))
    assert 0.9 * 35.0 * a < np.abs(a * 12.0 * x).max() <= 35.0 * a + 1e-3
    _check_classes(case, f"|alpha v| <= {35 * a:g}, alpha {a:g}")


def test_snake_conv_arguments_beyond_256_turns():
    """alpha = 20, v ~ N(0, 100^2) clipped to |v| <= 440 (the e4m3 window): |alpha v| up to 8800 rad, 1400 turns.  The polynomial
    forms have no domain (float32 rounding of alpha v costs ~5e-4 rad, 1 / alpha makes that 2.5e-5 on a |v| of order 100) and stay in
    their class.  The f16f8 forms must return finite values within what test_f16f8_form_outside_the_e4m3_window grants that form
    outside its window: relative rms error below 4e-4 + that of the f16x3 form on the same data (a wrong sin^2 costs at most
    1 / alpha = 0.05 on a |v| of order 100)."""
    a = 20.0
    x, norm = _big_inputs(100.0, 440.0, 77)
    case = _Case(BIG, np.full(BIG[2], a, dtype=np.float32), x, norm, 78)
    assert np.abs(a * 100.0 * x).max() > 8000.0
    rel3 = None
    for mode in (1, 2, 3):
        _, emax, erms = case.run(mode)
        print(f"|alpha v| <= 8800, {MODE_NAMES[mode]:>9}: max {emax / case.scale:.2e}, rms {erms / case.scale:.2e} (of scale {case.scale:.3g})")
        assert emax < POLY_MAX * case.scale, (MODE_NAMES[mode], emax / case.scale)
        if mode == 1:
            rel3 = erms / case.ref_rms
    for mode in F8_MODES:
        y, emax, erms = case.run(mode)
        assert np.isfinite(y).all(), MODE_NAMES[mode]
        rel = erms / case.ref_rms
        print(f"|alpha v| <= 8800, {MODE_NAMES[mode]:>9}: max {emax / case.scale:.2e}, rms {erms / case.scale:.2e}, relative rms {rel:.2e} "
              f"(f16x3 form {rel3:.2e})")
        assert rel < 4e-4 + rel3, (MODE_NAMES[mode], rel, rel3)
