"""GPU: the normalisation kernels of kernels_misc.hip that feed the convs, alone, against float64: layernorm_ch_kernel
(kx_test_layernorm), in_stats_kernel and stats_finalize_kernel (kx_test_instance_norm), the fused InstanceNorm statistics of the conv
epilogues carried through stats_finalize_kernel to the planes the next conv reads (conv1d_opts(..., want_norm=gb)), and the chain
conv -> fused statistics -> finalize -> conv.  Every bound is derived from float32 rounding where it is used; run with -s to see
the measured figures."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # unit round-off of float32
F8 = 0x200


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


# ---- channel layer norm ------------------------------------------------------------------------------------------------------

LN_VARIANTS = [  # mode, leaky slope, eps, DC offset in units of the row's spread
    (0, 0.0, 1e-12, 0.0), (1, 0.0, 1e-12, 0.0), (2, 0.0, 1e-5, 0.0), (0, 0.2, 1e-5, 100.0), (1, 0.2, 1e-12, 100.0), (2, 0.2, 1e-5, 100.0),
    (2, 0.0, 1e-12, 100.0), (1, 0.0, 1e-5, 0.0),
]


@pytest.mark.parametrize("T", [1, 15, 16, 17, 130, 512])
@pytest.mark.parametrize("C", [128, 512, 768, 100, 200, 700])  # 100 / 200 / 700: not a multiple of 64, on 2 / 8 / 12 values per thread
def test_layernorm_over_channels(C, T):
    """launch_layernorm_ch on a ragged batch of three, padded rows: plain, affine (ALBERT, eps 1e-12) and adaptive ((1 + g) xhat +
    be, per-utterance planes), with and without the leaky slope, zero-mean columns and columns with a DC offset of 100 x their spread.
    Bound, from float32 rounding of the kernel's two passes: a column's C values are summed over a chain of at most D = CPT + 2
    + 16 <= 30 additions (registers, two shuffles, 16 LDS partials), so the mean is off by <= D U mean|x| and the centred sum of
    squares by <= (D + 2) U relative, i.e. rstd by half that; with the subtraction, the product and the final affine / leaky
    steps (<= 4 U) the normalised value is off by <= (D / 2 + 5) U |xhat| + D U mean|x| rstd, times |gain|, + 2 U |out|:
    a few ulp of the normalised value, plus the DC term (100 x spread: 30 U 100 = 1.8e-4).  Columns past the length and the padding
    are untouched; an utterance's bits do not depend on the batch."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(C * 1000 + T)
    B = 3
    lens = np.array([T, max(1, (2 * T) // 3), max(1, T // 3)], dtype=np.int32)
    D = 30
    worst = 0.0
    for mode, leaky, eps, dc in LN_VARIANTS:
        spread = (0.5 + rng.random((B, 1, T))).astype(np.float32)
        x = (spread * (rng.standard_normal((B, C, T)) + dc * rng.choice([-1.0, 1.0], size=(B, 1, T)))).astype(np.float32)
        g = be = None
        if mode == 1:
            g, be = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
        elif mode == 2:
            g, be = (0.3 * rng.standard_normal((B, C))).astype(np.float32), rng.standard_normal((B, C)).astype(np.float32)
        y = hk.layernorm(x, lens, eps=eps, mode=mode, g=g, be=be, leaky=leaky)
        x64 = x.astype(np.float64)
        m = x64.mean(axis=1, keepdims=True)
        rstd = 1.0 / np.sqrt(x64.var(axis=1, keepdims=True) + eps)
        xhat = (x64 - m) * rstd
        gain, off = 1.0, 0.0
        if mode == 1:
            gain, off = g.astype(np.float64)[None, :, None], be.astype(np.float64)[None, :, None]
        elif mode == 2:
            gain, off = 1.0 + g.astype(np.float64)[:, :, None], be.astype(np.float64)[:, :, None]
        ref = gain * xhat + off
        if leaky:
            ref = np.where(ref > 0, ref, ref * np.float64(np.float32(leaky)))
        tol = np.abs(gain) * ((D / 2 + 5) * U * np.abs(xhat) + D * U * np.abs(x64).mean(axis=1, keepdims=True) * rstd) + 2 * U * np.abs(ref) + 1e-30
        valid = np.broadcast_to(np.arange(T)[None, None, :] < lens[:, None, None], y.shape)
        ratio = float((np.abs(y - ref) / tol)[valid].max())
        worst = max(worst, ratio)
        print(f"layernorm C={C} T={T} mode {mode} leaky {leaky} eps {eps:g} dc {dc:g}: max err {np.abs(y - ref)[valid].max():.2e} "
              f"= {ratio:.3f} of the bound")
        assert ratio < 1.0, (mode, leaky, eps, dc, ratio)
        assert np.all(y[~valid] == hk.LN_SENTINEL), (mode, "columns past the length were written")
        for i in (1, 2):  # an utterance's bits do not depend on the batch
            n = int(lens[i])
            y1 = hk.layernorm(x[i:i + 1, :, :n], lens[i:i + 1], eps=eps, mode=mode, g=g if mode != 2 else g[i:i + 1],
                              be=be if mode != 2 else be[i:i + 1], leaky=leaky)
            np.testing.assert_array_equal(y1[0], y[i, :, :n])


# ---- InstanceNorm statistics -------------------------------------------------------------------------------------------------

RATIOS = (0.0, 3.0, 30.0, 300.0)  # mean / std of a row


def _in_ref(y, lens, gb):
    """float64 InstanceNorm planes of the float32 tensor y [B,C,L] over each utterance's own columns: mean, scale = (1 + gamma)
    rstd (biased variance, eps 1e-5, gamma as the float32 the kernel reads), shift = beta; and the variance."""
    B, C, _ = y.shape
    mean, var = np.zeros((B, C)), np.zeros((B, C))
    for i in range(B):
        v = y[i, :, :int(lens[i])].astype(np.float64)
        mean[i], var[i] = v.mean(axis=1), v.var(axis=1)
    g = (np.float32(1.0) + gb[:, :C]).astype(np.float64)  # (1.0f + g: one float32 rounding, as in the kernels)
    return mean, g / np.sqrt(var + 1e-5), gb[:, C:].astype(np.float64), var


@pytest.mark.parametrize("L", [1, 3, 63, 64, 65, 1023, 5200, 84000])
def test_instance_norm_pass_matches_float64_at_every_mean_to_spread_ratio(L):
    """launch_in_stats (f64 accumulation) alone, leaving its raw sums, and those raw sums (a high and a low float each) through
    launch_stats_finalize, as Model::stats runs the first and the later AdaINs of a tensor: rows with mean / std = 0, 3, 30, 300,
    ragged batch of three, padded rows with NaN padding.  All three must match the float64 planes to float32 rounding whatever
    the ratio: the mean is one rounding of an f64 value (<= U, 2 U allowed), the scale is float32((1 + g)) x float32(rstd) (three
    roundings, 4 U allowed), the raw sums recombine to 2^-48, which the variance's cancellation (1 + ratio^2 = 9e4) leaves at
    3e-10.  The shift is beta itself."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(L)
    B, C = 3, 8
    lens = np.array([L, max(1, (2 * L) // 3), max(1, L // 3)], dtype=np.int32)
    ratio = np.array(RATIOS * 2)
    sigma = (0.5 + rng.random((B, C, 1)))
    x = (sigma * (rng.standard_normal((B, C, L)) + ratio[None, :, None])).astype(np.float32)
    gb = (0.3 * rng.standard_normal((B, 2 * C))).astype(np.float32)
    out = hk.instance_norm(x, lens, gb)
    mean, scale, shift, _ = _in_ref(x, lens, gb)
    np.testing.assert_array_equal(out[0], out[1])  # leaving the raw sums changes nothing
    for route, name in ((0, "in_stats"), (2, "raw sums finalized")):
        em = np.abs(out[route, 0] - mean) / np.maximum(np.abs(mean), 1e-30)
        es = np.abs(out[route, 1] - scale) / np.abs(scale)
        for r in RATIOS:
            sel = ratio == r
            print(f"instance norm L={L} {name}, mean/std {r:g}: mean rel err {em[:, sel].max():.1e}, scale rel err {es[:, sel].max():.1e}")
        assert np.all(np.abs(out[route, 0] - mean) <= 2 * U * np.abs(mean) + 1e-12), name
        assert es.max() <= 4 * U + 3e-9, name
        np.testing.assert_array_equal(out[route, 2], gb[:, C:])


def _slot_envelope(mean, var, n):
    """What n-column float32 partial sums can cost the scale.  A slot adds n values (and, by fma, n squares) in float32, in whatever
    order: each sum is off by <= (n - 1) U sum|terms|; the slots are added in f64.  So S / L is off by <= n U mean|v| <= n U
    sqrt(var + m^2) and Q / L by <= n U (var + m^2), and var = Q / L - m^2 by E = n U (var + m^2) + 2 |m| n U sqrt(var + m^2) <=
    n U (var + m^2) (1 + 2) -- with ratio = |m| / sigma: var' = var (1 +- 3 n U (1 + ratio^2)).  The scale goes like
    (var + eps)^-1/2: relative error <= e / 2 (1 + e) with e = E / (var + 1e-5), + 4 U for the float32 planes; this is
    eps_slot (1 + ratio^2) with eps_slot = 1.5 n U (1.1e-5 for 128-column slots, 5.7e-6 for 64).  Returns (bound, e)."""
    E = 3.0 * n * U * (var + mean * mean)
    e = E / (var + 1e-5)
    return 0.5 * e * (1.0 + e) + 4 * U, e


FUSED_FORMS = [  # name, Cin, Cout, k, dil, act, hook mode, form, stat_cols
    ("f32", 32, 128, 3, 1, 0, 0, "F32", 64),
    ("lds64rows", 32, 64, 3, 1, 0, 1, "LDS", 64),
    ("s16", 32, 128, 11, 1, 2, 3, "DA_S16", 64),
    ("f8", 32, 128, 7, 3, 2, 3 | F8, "DA_F8", 64),
    ("lds", 32, 128, 3, 1, 0, 2, "LDS", 128),
    ("da", 32, 128, 3, 1, 0, 3, "DA", 128),
    ("da_w2", 32, 128, 3, 1, 1, 3, "DA_W2", 128),
]
FUSED_LENS = {1: ("f32", "da"), 3: ("lds64rows", "s16"), 63: ("f8", "lds"), 64: ("da_w2", "f32"), 65: ("s16", "da"),
              1023: tuple(f[0] for f in FUSED_FORMS), 5200: tuple(f[0] for f in FUSED_FORMS), 84000: ("da", "s16", "f32")}


@pytest.mark.parametrize("name,Cin,Cout,k,d,act,mode,form,stat_cols", FUSED_FORMS)
def test_fused_statistics_through_finalize_stay_inside_the_slot_envelope(name, Cin, Cout, k, d, act, mode, form, stat_cols):
    """The conv route to the AdaIN planes: the epilogue's float32 (sum, sum of squares) per statistics slot, added up in f64 by
    stats_finalize_kernel into var = Q / L - m^2.  The conv's bias gives its output rows mean / std ratios of 0, 3, 30 and 300;
    the reference is the float64 InstanceNorm of the float32 tensor the conv stored.  Every slot width the plan takes is reached
    (64 columns: F32, the 64-row LDS-DMA tile, S16, F8; 128: LDS, DA, DA_W2; asserted from the plan), at lengths 1 .. 84000 on a
    ragged batch of three.  Asserted: _slot_envelope (derived from the slot arithmetic, not fitted), wherever it is below 0.5;
    the mean to n U mean|v| + U |m|; a finite, positive scale everywhere.  Printed: the measured relative scale error per ratio."""
    from kokorox_amd import hip_koko as hk
    pad = (k - 1) // 2 * d
    edges = (0.0, 1.0, 3.0, 10.0, 30.0, 100.0, 300.0, np.inf)  # bins of the measured mean / std of rows of >= 63 columns
    worst, first_over = np.zeros(len(edges) - 1), np.inf
    for L, names in FUSED_LENS.items():
        if name not in names:
            continue
        rng = np.random.default_rng(L + Cout + k)
        B = 3
        lens = np.array([L, max(1, (2 * L) // 3), max(1, L // 3)], dtype=np.int32)
        x = rng.standard_normal((B, Cin, L), dtype=np.float32)
        w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
        ratio = np.array(RATIOS * (Cout // 4))
        b = ratio.astype(np.float32)  # (the conv's own output has a spread of about 1)
        alpha = (rng.random(Cin, dtype=np.float32) + 0.5).astype(np.float32)
        norm = np.zeros((3, B, Cin), dtype=np.float32)
        norm[1] = 1.0
        gb = (0.3 * rng.standard_normal((B, 2 * Cout))).astype(np.float32)
        r = hk.conv1d_opts(x, w, b, pad=pad, dil=d, act=act, slope=0.2, alpha=alpha, norm=norm if act else None, lens=lens, pad_ld=True,
                           flat=True, mode=mode, want_norm=gb)
        assert r["plan"]["form"] == form and r["plan"]["stat_cols"] == stat_cols, (L, r["plan"])
        pm, ps, ph = r["norm"].astype(np.float64)
        mean, scale, shift, var = _in_ref(r["y"], lens, gb)
        assert np.isfinite(r["norm"]).all() and np.all(ps / scale > 0), L
        np.testing.assert_array_equal(r["norm"][2], gb[:, Cout:])
        bound, e = _slot_envelope(mean, var, stat_cols)
        es = np.abs(ps - scale) / np.abs(scale)
        checked = e < 0.5
        assert np.all(es[checked] <= bound[checked]), (L, float((es / bound)[checked].max()))
        assert np.all(np.abs(pm - mean) <= stat_cols * U * np.sqrt(var + mean * mean) + U * np.abs(mean) + 1e-12), L
        act_ratio = np.abs(mean) / np.sqrt(np.maximum(var, 1e-30))
        for rr in RATIOS:
            sel = np.broadcast_to(ratio[None, :] == rr, es.shape) & (var > 0)
            if sel.any():
                print(f"fused statistics {name} ({form}, {stat_cols}-column slots) L={L}, bias / std {rr:g} (mean / std up to "
                      f"{act_ratio[sel].max():.0f}): scale rel err {es[sel].max():.2e} (envelope {bound[sel].max():.1e})")
        rows = np.broadcast_to(lens[:, None] >= 63, es.shape)
        for j in range(len(worst)):
            sel = rows & (act_ratio >= edges[j]) & (act_ratio < edges[j + 1])
            if sel.any():
                worst[j] = max(worst[j], float(es[sel].max()))
        if (rows & (es > 1e-4)).any():
            first_over = min(first_over, float(act_ratio[rows & (es > 1e-4)].min()))
    print(f"fused statistics {name} ({form}): worst relative scale error by measured mean / std (rows of >= 63 columns): " +
          ", ".join(f"[{edges[j]:g}, {edges[j + 1]:g}): {worst[j]:.1e}" for j in range(len(worst)) if worst[j] > 0) +
          f"; smallest mean / std with an error above 1e-4: {first_over:.0f}")


def test_conv_statistics_finalize_conv_chain():
    """conv A (64 -> 128, k = 3, fused statistics) -> stats_finalize -> conv B (128 -> 128, k = 7, those planes + snake), ragged, on
    the direct-A forms a generator resblock runs, against float64 conv(snake(instance_norm(conv A))).
    Bound, added up: conv B's own 3e-5 (f16x3 with a fused transform) + what reaches its input, through it.  Its input
    s (yA - m) + beta is off by (1) conv A's 2e-5 times the scale s, (2) the planes' error from _slot_envelope: a relative scale
    error e_s on |s (yA - m)| and a mean error n U mean|yA| times s.  The snake x + sin^2(alpha x) / alpha has slope <= 2.  Conv B
    adds Cin k = 896 such errors with weights of l2 norm ~1 per row: independent errors add in quadrature, six standard deviations
    = 6 |w|_2 (never more than the l1 norm).  tol = 3e-5 + 2 min(|w|_1, 6 |w|_2) max(e_in)."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(77)
    B, Ca, Cb, L = 3, 64, 128, 700
    lens = np.array([L, 517, 129], dtype=np.int32)
    x = rng.standard_normal((B, Ca, L), dtype=np.float32)
    wa = (rng.standard_normal((Cb, Ca, 3), dtype=np.float32) / np.sqrt(Ca * 3)).astype(np.float32)
    ba = rng.standard_normal(Cb, dtype=np.float32)  # (rows with mean / std up to ~3)
    wb = (rng.standard_normal((Cb, Cb, 7), dtype=np.float32) / np.sqrt(Cb * 7)).astype(np.float32)
    bb = rng.standard_normal(Cb, dtype=np.float32)
    gb = (0.3 * rng.standard_normal((B, 2 * Cb))).astype(np.float32)
    alpha = (rng.random(Cb, dtype=np.float32) + 0.5).astype(np.float32)
    # float64 chain
    ref = np.zeros((B, Cb, L))
    e_in = 0.0
    for i in range(B):
        n = int(lens[i])
        ya = F.conv1d(_t(x[i:i + 1, :, :n]), _t(wa), _t(ba), padding=1)
        m, var = ya.mean(dim=2, keepdim=True), ya.var(dim=2, unbiased=False, keepdim=True)
        s = (1.0 + _t(gb[i, :Cb]))[None, :, None] / torch.sqrt(var + 1e-5)
        xin = s * (ya - m) + _t(gb[i, Cb:])[None, :, None]
        a = _t(alpha)[None, :, None]
        ref[i, :, :n] = F.conv1d(xin + torch.sin(a * xin) ** 2 / a, _t(wb), _t(bb), padding=3).numpy()[0]
        mm, vv = m.numpy()[0, :, 0], var.numpy()[0, :, 0]
        e_s, _ = _slot_envelope(mm, vv, 128)
        sn = np.abs(s.numpy()[0, :, 0])
        e_in = max(e_in, float((sn * 2e-5 + e_s * np.abs((s * (ya - m)).numpy()[0]).max(axis=1) + 128 * U * np.sqrt(vv + mm * mm) * sn).max()))
    w1, w2 = np.abs(wb).sum(axis=(1, 2)).max(), np.sqrt((wb.astype(np.float64) ** 2).sum(axis=(1, 2))).max()
    tol = 3e-5 + 2.0 * min(w1, 6.0 * w2) * e_in
    valid = np.arange(L)[None, None, :] < lens[:, None, None]
    for mode, form_a, form_b in ((1, "DA", "DA_S16"), (3, "DA", "DA_S16"), (3 | F8, "DA", "DA_F8"), (2, "LDS", "LDS"), (0, "F32", "F32")):
        ra = hk.conv1d_opts(x, wa, ba, pad=1, lens=lens, pad_ld=True, flat=True, mode=mode & ~F8, want_norm=gb)
        assert ra["plan"]["form"] == form_a and ra["plan"]["stat_cols"] == (64 if mode == 0 else 128), ra["plan"]
        rb = hk.conv1d_opts(ra["y"], wb, bb, pad=3, act=2, alpha=alpha, norm=ra["norm"], lens=lens, pad_ld=True, flat=True, mode=mode)
        assert rb["plan"]["form"] == form_b, rb["plan"]
        bound = tol + (4e-4 if mode & F8 else 0.0)  # (the f16f8 form's own bound on O(1) outputs instead of 3e-5)
        err = np.abs(np.where(valid, rb["y"] - ref, 0.0)).max()
        print(f"chain mode {mode:#x} ({form_a} -> {form_b}): max err {err:.2e} (bound {bound:.2e}, input error allowed {e_in:.1e})")
        assert err < bound, (mode, err, bound)
