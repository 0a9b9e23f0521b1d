"""GPU: the conv launch options the model sets on every forward and no other kernel test reaches, through kx_test_conv
(hip_koko.conv1d_opts), against torch CPU float64: in_up2, the gelu_new epilogue, the merged token axis, time-major stores on the
f16x3 forms, the reduced-precision forms (prec1), the activation pre-scale (act_shift) and the streamed epilogue (epi_stream).

Every case names the ConvForm it is meant to reach and asserts it from the plan the hook launched, so that a later change of
conv_plan.hip cannot quietly move a case to another kernel.  Forms that follow the grid are named for 256 CUs (MI355X).
Bounds: 2e-5 absolute on O(1) outputs, 3e-5 with a fused input transform (tests/test_gpu_kernels.py); others are derived where
they are used.  Run with -s to see the measured figures."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F8 = 0x200     # hook mode bit: the layer carries the 8-bit cross image of its weights
DA_4X1 = 0x400  # the 4 x 1 wave layout on the direct-A conv's 256-column tile too
NO_S16 = 0x800  # no 16x16x32 form
U = 2.0 ** -24  # unit round-off of float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _weights(rng, cout, cin, k):
    return (rng.standard_normal((cout, cin, k), dtype=np.float32) / np.sqrt(cin * k)).astype(np.float32)


def _act_ref(x, act, norm, alpha, slope=0.2):
    """float64 reference of the fused input transform: AdaIN affine, then leaky / snake (x [B,Cin,L] torch f64)."""
    if norm is not None:
        n = _t(norm)
        x = (x - n[0][:, :, None]) * n[1][:, :, None] + n[2][:, :, None]
    if act == 2:
        a = _t(alpha)[None, :, None]
        return x + (1 / a) * torch.sin(a * x) ** 2
    if act == 1:
        return F.leaky_relu(x, slope)
    return x


def _ragged_conv(xt, w, b, lens, pad, dil, up2=False):
    """Each utterance convolved alone over its own (doubled, with up2) length: [B,Cout,Lmax_out] float64, zeros past its end."""
    B, k = xt.shape[0], w.shape[2]
    outs = []
    for i in range(B):
        xi = xt[i:i + 1, :, :int(lens[i])]
        if up2:
            xi = xi.repeat_interleave(2, -1)
        outs.append(F.conv1d(xi, _t(w), None if b is None else _t(b), padding=pad, dilation=dil).numpy()[0])
    ref = np.zeros((B, w.shape[0], max(o.shape[1] for o in outs)))
    for i, o in enumerate(outs):
        ref[i, :, :o.shape[1]] = o
    return ref, np.array([o.shape[1] for o in outs])


# ---- in_up2 ----------------------------------------------------------------------------------------------------------------

UP2_LENS = [(64, 63, 1), (65, 64, 33), (128, 127, 2), (129, 128, 65), (256, 255, 129), (257, 256, 1)]  # 2 L = 128 / 256 / 512 +- 2, and L = 1


@pytest.mark.parametrize("lens", UP2_LENS)
@pytest.mark.parametrize("Cin,Cout,k,act", [(1090, 512, 1, 0), (70, 130, 1, 0), (64, 128, 3, 1)])
def test_in_up2_reads_each_column_twice(Cin, Cout, k, act, lens):
    """The decoder's up-sampling shortcut (Model::adain_resblk: conv1x1 1090 -> 512 over x[p >> 1]), a ragged channel count, and a
    3-tap conv with a fused AdaIN + leaky transform, on a ragged batch of three on padded rows.  Forms: hook mode 0 F32, 2 LDS,
    3 DA (k = 1: run-time taps) / DA_W2 (leaky k = 3 on the 256-column tile), 1 LDS up to 160 columns and DA (128-column tile) past
    them.  Reference: F.conv1d of repeat_interleave(x, 2) per utterance over its own doubled length."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(Cin * 131 + Cout * 17 + k + lens[0] * 7)
    B, L, pad = 3, lens[0], (k - 1) // 2
    lens = np.array(lens, dtype=np.int32)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w, b = _weights(rng, Cout, Cin, k), rng.standard_normal(Cout, dtype=np.float32)
    norm = alpha = None
    if act:
        norm = rng.standard_normal((3, B, Cin), dtype=np.float32)
        norm[1] = 1.0 + 0.2 * norm[1]
    ref, out_lens = _ragged_conv(_act_ref(_t(x), act, norm, alpha), w, b, lens, pad, 1, up2=True)
    assert np.array_equal(out_lens, 2 * lens) and ref.shape[2] == 2 * L
    valid = np.arange(2 * L)[None, None, :] < 2 * lens[:, None, None]
    tol = 3e-5 if act else 2e-5
    forms = {0: "F32", 2: "LDS", 3: "DA_W2" if k == 3 else "DA", 1: "LDS" if 2 * L <= 160 else "DA"}
    got = {}
    for mode in (1, 0, 2, 3) + ((1 | F8,) if k == 3 else ()):
        r = hk.conv1d_opts(x, w, b, pad=pad, act=act, slope=0.2, norm=norm, lens=lens, pad_ld=True, flat=True, mode=mode, in_up2=True)
        y, plan = r["y"], r["plan"]
        assert plan["form"] == forms[mode & 0xff] and not plan["merged"], (mode, plan)
        err = np.abs(np.where(valid, y - ref, 0.0)).max()
        print(f"in_up2 {Cin}->{Cout} k={k} lens={tuple(lens)} mode {mode:#x} {plan['form']} bn={plan['bn']}: max err {err:.2e}")
        assert err < tol, (mode, err)
        assert np.all(np.where(valid, 0.0, y) == 0.0), mode  # columns past 2 * lens[b] are not written
        got[mode] = y
    if k == 3:  # (a leaky conv never takes the f16f8 form: the layer's 8-bit image rides along unused)
        np.testing.assert_array_equal(got[1 | F8], got[1])


# ---- the gelu_new epilogue -------------------------------------------------------------------------------------------------

GELU_CASES = [
    # B, Cin, Cout, lens, {hook mode: (form, vt)}
    (3, 768, 3072, (300, 257, 1), {1: ("DAG", 1), 3: ("DAG", 1), 2: ("LDS", 3), 0: ("F32", 1)}),   # the ALBERT FFN; chip-filling grid
    (2, 128, 768, (40, 33), {1: ("DAGN", 1), 3: ("DAGN", 1), 2: ("LDS", 3), 0: ("F32", 1)}),      # small grid: 128 x 32 tiles
    (3, 200, 256, (129, 128, 5), {1: ("DAGN", 1), 2: ("LDS", 3), 0: ("F32", 1)}),                  # partial 16-channel chunk
    (1, 200, 3072, (2800,), {1: ("DAG", 1), 2: ("LDS", 2)}),                                       # > 2 x 256 tiles: two-chunk virtual taps
]


def _gelu_tol(pre):
    """conv bound x max |gelu'| + the float32 evaluation of gelu_new_f (conv_epilogue.h) at the pre-activation `pre`:
    gelu'(x) peaks at 1.129 (x = 1.41), so the conv's 2e-5 becomes 2.26e-5.  The epilogue then computes
    0.5 x (1 + tanhf(c (x + 0.044715 x^3))) in float32: the argument u carries <= 4 roundings, which tanh' <= 1 scales by
    max |u| tanh'(u) = 0.45 (<= 4 U 0.45); tanhf is within 2 ulp of a value <= 1 (<= 2 U); the sum and the two products add
    <= 3 U of the result, itself <= |x|.  Together <= |x| (0.5 (1.8 U + 2 U) + 3 U) < 5 U |x| = 3e-7 |x|."""
    return 1.13 * 2e-5 + 5 * U * float(np.abs(pre).max())


@pytest.mark.parametrize("B,Cin,Cout,lens,forms", GELU_CASES)
def test_gelu_epilogue_against_float64(B, Cin, Cout, lens, forms):
    """EPI_GELU_NEW on the four kernels that carry it: the direct-A GEMM on a chip-filling grid (DAG) and on a small one (DAGN), the
    LDS-DMA virtual-tap form (hook mode 2, two and three chunks per super-chunk) and the f32 kernel, ragged on padded rows.
    Reference: F.gelu(conv, approximate="tanh") in float64.  Bound: _gelu_tol."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(Cin * 1009 + Cout + lens[0])
    L = lens[0]
    lens = np.array(lens, dtype=np.int32)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w, b = _weights(rng, Cout, Cin, 1), rng.standard_normal(Cout, dtype=np.float32)
    pre, _ = _ragged_conv(_t(x), w, b, lens, 0, 1)
    ref = F.gelu(torch.from_numpy(pre), approximate="tanh").numpy()
    valid = np.arange(L)[None, None, :] < lens[:, None, None]
    tol = _gelu_tol(pre)
    for mode, (form, vt) in forms.items():
        r = hk.conv1d_opts(x, w, b, lens=lens, pad_ld=True, mode=mode, epi=1)
        assert r["plan"]["form"] == form and r["plan"]["vt"] == vt, (mode, r["plan"])
        err = np.abs(np.where(valid, r["y"] - ref, 0.0)).max()
        print(f"gelu {Cin}->{Cout} lens={tuple(lens)} mode {mode} {form} vt={vt}: max err {err:.2e} (bound {tol:.2e})")
        assert err < tol, (mode, err, tol)
        assert np.all(np.where(valid, 0.0, r["y"]) == 0.0), mode


def test_gelu_epilogue_is_refused_where_no_kernel_carries_it():
    """16 input channels are one 16-channel chunk: not a GEMM form (conv_plan.hip wants three), so the f16x3 modes land on a kernel
    without the gelu epilogue and launch_conv must refuse (KX_REQUIRE, before any launch) instead of storing the pre-activation;
    the f32 kernel carries gelu on its 128-row tile only and refuses the 64-row one; on 128 rows it computes it."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(16)
    x = rng.standard_normal((2, 16, 70), dtype=np.float32)
    w, b = _weights(rng, 128, 16, 1), rng.standard_normal(128, dtype=np.float32)
    for mode in (1, 2, 3):
        with pytest.raises(hk.KokoroxHipError, match="gelu"):
            hk.conv1d_opts(x, w, b, mode=mode, epi=1)
    with pytest.raises(hk.KokoroxHipError, match="gelu"):
        hk.conv1d_opts(x, w[:64], b[:64], mode=0, epi=1)
    r = hk.conv1d_opts(x, w, b, mode=0, epi=1)
    pre = F.conv1d(_t(x), _t(w), _t(b)).numpy()
    assert r["plan"]["form"] == "F32"
    assert np.abs(r["y"] - F.gelu(torch.from_numpy(pre), approximate="tanh").numpy()).max() < _gelu_tol(pre)


# ---- the merged token axis -------------------------------------------------------------------------------------------------

MERGE_CASES = [  # B, T, form of hook mode 1 (128 -> 768: six row tiles; 2 x tiles <= 256 CUs: the narrow form)
    (2, 1, "DAGN"), (3, 9, "DAGN"), (8, 31, "DAGN"), (64, 33, "DAGN"), (2, 64, "DAGN"), (3, 130, "DAGN"), (8, 510, "DAG"),
    (64, 512, "DAG"), (3, 512, "DAGN"), (8, 33, "DAGN"),
]


@pytest.mark.parametrize("B,T,form", MERGE_CASES)
def test_merged_token_axis_equals_each_utterance_alone(B, T, form):
    """k = 1 GEMMs with one merged column space for the batch (ConvArgs::merge_T / merge_B: utterance = column / T), as every
    token-axis GEMM of a forward at B > 1 runs: 32- and 128-column tiles straddle the utterance borders at T = 1 .. 512.  Plain,
    + residual, + gelu and time-major, in hook mode 1 (DAG / DAGN) and 2 (LDS virtual taps), rows padded to 32 floats with NaN in
    the input padding.  Each utterance equals its own B = 1 call over its own length (never merged) bit for bit and float64 within
    2e-5 (gelu: _gelu_tol); the hook fails if anything in [T, ld) of a row is touched.  The f32 kernel never merges: control."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(B * 1000 + T)
    Cin, Cout = 128, 768
    lens = rng.integers(1, T + 1, size=B).astype(np.int32)
    lens[0] = T
    lens[-1] = max(1, T // 3)
    x = rng.standard_normal((B, Cin, T), dtype=np.float32)
    w, b = _weights(rng, Cout, Cin, 1), rng.standard_normal(Cout, dtype=np.float32)
    res = rng.standard_normal((B, Cout, T), dtype=np.float32)
    pre, _ = _ragged_conv(_t(x), w, b, lens, 0, 1)
    valid = np.arange(T)[None, None, :] < lens[:, None, None]
    combos = {"plain": (dict(), pre, 2e-5), "resid": (dict(resid=res), pre + res, 2e-5),
              "gelu": (dict(epi=1), F.gelu(torch.from_numpy(pre), approximate="tanh").numpy(), _gelu_tol(pre)),
              "tmajor": (dict(tmajor=True), pre, 2e-5)}
    for mode, want in ((1, form), (2, "LDS"), (0, "F32")):
        for name, (kw, ref, tol) in combos.items():
            if mode == 0 and name != "plain":
                continue
            r = hk.conv1d_opts(x, w, b, lens=lens, pad_ld=True, mode=mode, merged=True, **kw)
            plan = r["plan"]
            assert plan["form"] == want and plan["merged"] == (mode != 0) and (mode == 0 or plan["cols"] == B * T), (mode, name, plan)
            y = r["y"].transpose(0, 2, 1) if name == "tmajor" else r["y"]
            err = np.abs(np.where(valid, y - ref, 0.0)).max()
            print(f"merged B={B} T={T} mode {mode} {plan['form']} {name}: max err {err:.2e}")
            assert err < tol, (mode, name, err)
            for i in range(B):
                n = int(lens[i])
                k1 = {k_: (v[i:i + 1, :, :n] if k_ == "resid" else v) for k_, v in kw.items()}
                r1 = hk.conv1d_opts(x[i:i + 1, :, :n], w, b, lens=lens[i:i + 1], pad_ld=True, mode=mode, merged=True, **k1)
                assert not r1["plan"]["merged"]
                y1 = r1["y"].transpose(0, 2, 1) if name == "tmajor" else r1["y"]
                np.testing.assert_array_equal(y[i, :, :n], y1[0], err_msg=f"utterance {i} of {B}, mode {mode}, {name}")


@pytest.mark.parametrize("why", ["norm", "T>512"])
def test_plan_refuses_to_merge(why):
    """A GEMM with an AdaIN affine on its input, or a token axis longer than 512, keeps one grid slice per utterance whatever
    merge_T offers: the plan says so and the result still matches float64 (norm: the LDS virtual-tap form, 3e-5 with its fused
    transform; T = 513: DAGN)."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(len(why))
    B, Cin, Cout = 3, 128, 256
    T = 513 if why == "T>512" else 33
    lens = np.array([T, T - 1, 7], dtype=np.int32)
    x = rng.standard_normal((B, Cin, T), dtype=np.float32)
    w, b = _weights(rng, Cout, Cin, 1), rng.standard_normal(Cout, dtype=np.float32)
    norm, act = None, 0
    if why == "norm":
        norm = rng.standard_normal((3, B, Cin), dtype=np.float32)
        norm[1] = 1.0 + 0.2 * norm[1]
        act = 1
    ref, _ = _ragged_conv(_act_ref(_t(x), act, norm, None), w, b, lens, 0, 1)
    valid = np.arange(T)[None, None, :] < lens[:, None, None]
    for mode, form in ((1, "LDS" if why == "norm" else "DAGN"), (2, "LDS")):
        r = hk.conv1d_opts(x, w, b, act=act, slope=0.2, norm=norm, lens=lens, pad_ld=True, mode=mode, merged=True)
        assert r["plan"]["form"] == form and not r["plan"]["merged"] and r["plan"]["cols"] == T, r["plan"]
        assert np.abs(np.where(valid, r["y"] - ref, 0.0)).max() < (3e-5 if act else 2e-5), mode
        assert np.all(np.where(valid, 0.0, r["y"]) == 0.0), mode


# ---- time-major stores on the f16x3 forms ------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cin,lens,forms,merged", [
    (640, (1, 40, 700), {1: "DAG", 3: "DAG", 2: "LDS", 0: "F32"}, False),
    (512, (2600,), {1: "DAG", 3: "DAG", 2: "LDS", 0: "F32"}, False),
    (512, (40, 1), {1: "DAGN", 3: "DAGN", 2: "LDS", 0: "F32"}, True),   # a token-axis LSTM at B = 2: merged AND time-major
])
def test_time_major_store_of_the_lstm_input_projection(Cin, lens, forms, merged):
    """The 2048-row input projection of Model::lstm (store = ST_TMAJOR: y [B][frame][2048]) on the kernels a forward runs it on,
    offered merge_T as the model offers it.  Each row of 2048 values ends in a checked margin; rows past an utterance's length
    stay as they were (a merged launch writes all T rows of every utterance: there only the margin is checked)."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(Cin + lens[0])
    B, L, Cout = len(lens), max(lens), 2048
    lens = np.array(lens, dtype=np.int32)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w, b = _weights(rng, Cout, Cin, 1), rng.standard_normal(Cout, dtype=np.float32)
    ref, _ = _ragged_conv(_t(x), w, b, lens, 0, 1)
    valid = np.arange(L)[None, None, :] < lens[:, None, None]
    for mode, form in forms.items():
        r = hk.conv1d_opts(x, w, b, lens=lens, pad_ld=True, mode=mode, merged=True, tmajor=True)
        assert r["plan"]["form"] == form and r["plan"]["merged"] == (merged and mode != 0), (mode, r["plan"])
        assert r["y"].shape == (B, L, Cout)
        y = r["y"].transpose(0, 2, 1)
        err = np.abs(np.where(valid, y - ref, 0.0)).max()
        print(f"tmajor {Cin}->2048 lens={tuple(lens)} mode {mode} {form}: max err {err:.2e}")
        assert err < 2e-5, (mode, err)
        if not r["plan"]["merged"]:
            assert np.all(np.where(valid, 0.0, y) == 0.0), mode


# ---- prec1: one f16 / bf16 MFMA per product ------------------------------------------------------------------------------------

def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64 (the sum's rounding to 53 bits before the one to 24
    matters only in ties that the data do not produce)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def _sin_sq32(t):
    """sin_sq of conv_f16x3_common.h, operation for operation in float32."""
    f = np.float32
    n = np.rint(t * f(0.318309886183790672)).astype(np.float32)
    r = _fma32(n, f(-3.14159274101257324), t)
    r = _fma32(n, f(8.74227765734758578e-08), r)
    z = r * r
    p = _fma32(z, f(-3.6197402550897095e-06), f(1.3928599946666651e-04))
    p = _fma32(z, p, f(-3.1722760759294033e-03))
    p = _fma32(z, p, f(4.4443082064390182e-02))
    p = _fma32(z, p, f(-3.3333304524421692e-01))
    p = _fma32(z, p, f(1.0))
    return z * p


def _transform32(x, act, norm, alpha, slope):
    """The staged value of the direct-A kernels (conv_f16x3_da.hip, emit8: fmaf(x - mean, scale, shift), then in_act) in float32,
    operation for operation, so that the rounding to f16 / bf16 that follows decides as the kernel decides."""
    y = x.astype(np.float32)
    if norm is not None:
        y = _fma32(y - norm[0][:, :, None], norm[1][:, :, None], norm[2][:, :, None])
    if act == 2:
        al = alpha.astype(np.float32)[None, :, None]
        y = _fma32(np.float32(1.0) / al, _sin_sq32(al * y), y)
    elif act == 1:
        y = np.where(y > 0, y, y * np.float32(slope)).astype(np.float32)
    return y


def _bf16_rne(v):
    """Round float32 to bfloat16 as pack_pair (BF) and image_to_bf16_kernel do: u += 0x7fff + ((u >> 16) & 1); u >>= 16."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def _round_operands(xt32, w, prec1):
    """What the reduced-precision kernels multiply, in float64.  Activations: f16(clamp(v, +-65504)) (split_pair's high half), or
    bf16.  Weights: the image holds hi = f16(w 2^ws), lo = f16(w 2^ws - hi) with ws = 12 - exponent(max |w|) clamped to [-8, 24]
    (pick_weight_shift); the f16 form reads hi alone, the bf16 image is bf16(hi + lo)."""
    _, e = np.frexp(np.float32(np.abs(w).max()))
    ws = int(np.clip(12 - int(e), -8, 24))
    v = (w * np.float32(2.0 ** ws)).astype(np.float32)
    hi = v.astype(np.float16)
    if prec1 == 1:
        xq = np.clip(xt32, -65504.0, 65504.0).astype(np.float16).astype(np.float64)
        wq = hi.astype(np.float64)
    else:
        lo = (v - hi.astype(np.float32)).astype(np.float16)
        xq = _bf16_rne(xt32).astype(np.float64)
        wq = _bf16_rne(hi.astype(np.float32) + lo.astype(np.float32)).astype(np.float64)
    return xq, wq * 2.0 ** -ws


P1_CASES = [  # Cin, Cout, k, dil, act, lens (B = 3, ragged, flat tile list; lengths at the 128- / 256-column borders)
    (128, 128, 3, 1, 2, (257, 256, 129)), (128, 128, 7, 3, 2, (385, 255, 128)), (128, 128, 11, 5, 2, (257, 129, 127)),
    (128, 128, 3, 5, 2, (385, 257, 1)), (128, 128, 7, 1, 2, (257, 256, 255)), (128, 128, 11, 3, 2, (513, 384, 129)),
    (256, 256, 3, 3, 2, (257, 255, 129)), (256, 256, 7, 5, 2, (385, 256, 127)), (256, 256, 11, 1, 2, (257, 129, 128)),
    (1090, 1024, 3, 1, 1, (257, 256, 129)),
]


@pytest.mark.parametrize("prec1", [1, 2])
@pytest.mark.parametrize("Cin,Cout,k,d,act,lens", P1_CASES)
def test_reduced_precision_forms_against_rounded_operands(Cin, Cout, k, d, act, lens, prec1):
    """KOKOROX_CONV=f16 / bf16 (conv_f16x3_da_p1.hip): the generator's snake resblock convs and the decoder's leaky 1090 -> 1024
    conv on FORM_DA with p1 (and bf for bf16), on its 128-column tile (hook mode 1) and its 256-column one (mode 3).  The reference
    is the float64 conv of the operands rounded as the kernel rounds them (_transform32, _round_operands), so only the f32
    accumulation is left and the f16x3 bound (3e-5 with the fused transform) applies.  The result is really reduced: it differs
    from the f16x3 result by more than 1e-5 of the output's rms."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(Cin * 31 + k * 7 + d + prec1)
    B, L, pad = 3, lens[0], (k - 1) // 2 * d
    lens = np.array(lens, dtype=np.int32)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w, b = _weights(rng, Cout, Cin, k), rng.standard_normal(Cout, dtype=np.float32)
    norm = rng.standard_normal((3, B, Cin), dtype=np.float32)
    norm[1] = 1.0 + 0.2 * norm[1]
    alpha = (rng.random(Cin, dtype=np.float32) + 0.5).astype(np.float32)
    xq, wq = _round_operands(_transform32(x, act, norm, alpha, 0.2), w, prec1)
    ref, _ = _ragged_conv(torch.from_numpy(xq), wq, b, lens, pad, d)
    valid = np.arange(L)[None, None, :] < lens[:, None, None]
    kw = dict(pad=pad, dil=d, act=act, slope=0.2, alpha=alpha, norm=norm, lens=lens, pad_ld=True, flat=True)
    ys = []
    for mode, bn in ((1, 128), (3, 256)):
        r = hk.conv1d_opts(x, w, b, mode=mode, prec1=prec1, **kw)
        plan = r["plan"]
        assert plan["form"] == "DA" and plan["p1"] == 1 and plan["bf"] == (prec1 == 2) and plan["bn"] == bn and plan["flat_bn"] == bn, plan
        err = np.abs(np.where(valid, r["y"] - ref, 0.0)).max()
        print(f"prec1={prec1} {Cin}->{Cout} k={k} d={d} act={act} mode {mode} bn={bn}: max err vs rounded operands {err:.2e}")
        assert err < 3e-5, (mode, err)
        assert np.all(np.where(valid, 0.0, r["y"]) == 0.0), mode
        ys.append(r["y"])
    np.testing.assert_array_equal(ys[0], ys[1])  # both tile widths: the same bits
    y3 = hk.conv1d_opts(x, w, b, mode=1, **kw)["y"]
    rms = np.sqrt((ref[valid.repeat(Cout, 1)] ** 2).mean())
    diff = np.abs(np.where(valid, ys[0] - y3, 0.0)).max()
    print(f"   differs from f16x3 by {diff:.2e} (output rms {rms:.2f})")
    assert diff > 1e-5 * rms


@pytest.mark.parametrize("prec1", [1, 2])
def test_reduced_precision_polyphase_upsampler(prec1):
    """The generator's first upsampler shape (ConvTranspose1d 256 -> 128, stride 6, as two-tap polyphase GEMM with a fused leaky
    input) on FORM_DA with p1, against conv_transpose1d of the rounded operands in float64."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(60 + prec1)
    B, Cin, Cout, L, s = 2, 256, 128, 300, 6
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cin, Cout, 2 * s), dtype=np.float32) / np.sqrt(Cin * 2)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    xq, wq = _round_operands(_transform32(x, 1, None, None, 0.1), w, prec1)
    ref = F.conv_transpose1d(torch.from_numpy(xq), torch.from_numpy(wq), _t(b), stride=s, padding=s // 2).numpy()
    r = hk.conv1d_opts(x, w, b, act=1, slope=0.1, mode=1, prec1=prec1, up_stride=s)
    assert r["plan"]["form"] == "DA" and r["plan"]["p1"] == 1 and r["plan"]["bf"] == (prec1 == 2), r["plan"]
    err = np.abs(r["y"] - ref).max()
    y3 = hk.conv1d_opts(x, w, b, act=1, slope=0.1, mode=1, up_stride=s)["y"]
    print(f"prec1={prec1} polyphase 256->128 s=6: max err vs rounded operands {err:.2e}, differs from f16x3 by {np.abs(r['y'] - y3).max():.2e}")
    assert r["y"].shape == ref.shape and err < 3e-5
    assert np.abs(r["y"] - y3).max() > 1e-5 * np.sqrt((ref ** 2).mean())


# ---- act_shift -------------------------------------------------------------------------------------------------------------

ACT_SHIFT_MODES = [(1, "DA_S16"), (3, "DA_S16"), (2, "LDS"), (1 | NO_S16, "DA"), (3 | NO_S16, "DA_W2"), (1 | F8, "DA_F8")]


def _act_shift_setup(gain):
    rng = np.random.default_rng(int(gain * 1000) % 9973)
    B, C, L, k, d = 2, 128, 700, 11, 3
    x = rng.standard_normal((B, C, L), dtype=np.float32)
    w = _weights(rng, C, C, k)
    alpha = (rng.random(C, dtype=np.float32) + 0.5).astype(np.float32) / np.float32(max(gain, 1.0))
    norm = np.zeros((3, B, C), dtype=np.float32)
    norm[1] = gain  # the AdaIN scale carries the gain: v = gain * x, then the snake
    ref = F.conv1d(_act_ref(_t(x), 2, norm, alpha), _t(w), None, padding=d * (k - 1) // 2, dilation=d).numpy()
    return x, w, dict(pad=d * (k - 1) // 2, dil=d, act=2, alpha=alpha, norm=norm), ref


def _rel_rms(y, ref):
    return float(np.sqrt(((y - ref) ** 2).mean()) / np.sqrt((ref ** 2).mean()))


@pytest.mark.parametrize("mode,form", ACT_SHIFT_MODES)
def test_act_shift_restores_small_activations(mode, form):
    """kx_set_act_prescale's repair: with the AdaIN scale carrying a gain of 1e-5 (the set-up of
    test_f16f8_form_outside_the_e4m3_window) the low halves of the split fall under f16's range and the conv degrades; with
    x_prescale = 2^12 the operands are back in range and the relative rms error against float64 must be back in the f16x3 class,
    the same as measured at gain 1.  Class bound: a split product keeps 2^-22; four times that (hi / lo rounding of both operands,
    the dropped lo x lo term, f32 accumulation of 1408 terms) = 2^-20 = 9.5e-7.  The f16f8 form: its own 3e-5 at gain 1 (the cross
    terms keep 4 bits); 2^12 x 1e-5 = 0.04 leaves part of the values under the e4m3 window [2^-6, 448], where that form's bound is
    the one-MFMA class, 4e-4 (test_f16f8_form_outside_the_e4m3_window).  Both figures are printed."""
    from kokorox_amd import hip_koko as hk
    bound, bound12 = (3e-5, 4e-4) if mode & F8 else (2.0 ** -20, 2.0 ** -20)
    x, w, kw, ref = _act_shift_setup(1.0)
    r = hk.conv1d_opts(x, w, None, mode=mode, **kw)
    assert r["plan"]["form"] == form, r["plan"]
    rel1 = _rel_rms(r["y"], ref)
    x, w, kw, ref = _act_shift_setup(1e-5)
    rel_small = _rel_rms(hk.conv1d_opts(x, w, None, mode=mode, **kw)["y"], ref)
    r = hk.conv1d_opts(x, w, None, mode=mode, act_shift=12, **kw)
    assert r["plan"]["form"] == form and np.isfinite(r["y"]).all()
    rel12 = _rel_rms(r["y"], ref)
    print(f"act_shift mode {mode:#x} {form}: relative rms error at gain 1: {rel1:.2e}; at gain 1e-5: {rel_small:.2e}, with act_shift 12: {rel12:.2e}")
    assert rel1 < bound and rel12 < bound12, (rel1, rel12)


@pytest.mark.parametrize("mode,form", ACT_SHIFT_MODES)
def test_act_shift_is_harmless_at_gain_one(mode, form):
    """A power-of-two pre-scale moves exponents only: at gain 1, act_shift -4 and +8 (|v| 2^8 stays far below 65504) must not be
    worse than shift 0 by more than the f16x3 bound with a fused transform, 3e-5 absolute (f16f8: its 4e-4 of the output's rms, the
    images' window moves with the scale), and never produce a NaN or an infinity."""
    from kokorox_amd import hip_koko as hk
    x, w, kw, ref = _act_shift_setup(1.0)
    e0 = np.abs(hk.conv1d_opts(x, w, None, mode=mode, **kw)["y"] - ref).max()
    for s in (-4, 8):
        r = hk.conv1d_opts(x, w, None, mode=mode, act_shift=s, **kw)
        assert r["plan"]["form"] == form and np.isfinite(r["y"]).all(), (s, r["plan"])
        e = np.abs(r["y"] - ref).max()
        print(f"act_shift {s:+d} mode {mode:#x} {form}: max err {e:.2e} (shift 0: {e0:.2e})")
        assert e <= e0 + (4e-4 * max(1.0, float(np.sqrt((ref ** 2).mean()))) if mode & F8 else 3e-5), (s, e, e0)


# ---- epi_stream ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,d,mode,form", [(3, 1, 1, "DA_W2"), (11, 3, 1, "DA_S16"), (7, 3, 1 | F8, "DA_F8"), (3, 1, 1 | DA_4X1, "DA")])
def test_streamed_epilogue_gives_the_same_bits(k, d, mode, form):
    """ConvArgs::epi_stream (non-temporal 16-byte stores and residual / running-sum loads of the interior groups: what every
    generator conv runs at batch 64) on chip-filling direct-A launches (4 x 65 column tiles >= 256 workgroups), one per form:
    the streamed launch equals the cached one bit for bit in y and in the fused statistics, for a plain store, + residual,
    + residual + running sum / 3, and with statistics; the 3-tap 2 x 2 form is checked against float64 too."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(k * 100 + d + mode)
    B, C, L, pad = 4, 128, 16500, (k - 1) // 2 * d
    lens = np.array([L, 16400, 16389, 16385], dtype=np.int32)
    x = rng.standard_normal((B, C, L), dtype=np.float32)
    w, b = _weights(rng, C, C, k), rng.standard_normal(C, dtype=np.float32)
    norm = rng.standard_normal((3, B, C), dtype=np.float32)
    norm[1] = 1.0 + 0.2 * norm[1]
    alpha = (rng.random(C, dtype=np.float32) + 0.5).astype(np.float32)
    res = rng.standard_normal((B, C, L), dtype=np.float32)
    run = rng.standard_normal((B, C, L), dtype=np.float32)
    kw = dict(pad=pad, dil=d, act=2, alpha=alpha, norm=norm, lens=lens, pad_ld=True, flat=True, mode=mode)
    combos = {"plain": dict(), "resid": dict(resid=res), "resid+accum/3": dict(resid=res, y_init=run, out_div=3.0),
              "stats": dict(want_stats=True), "resid+stats": dict(resid=res, want_stats=True)}
    for name, c in combos.items():
        r0 = hk.conv1d_opts(x, w, b, **kw, **c)
        r1 = hk.conv1d_opts(x, w, b, epi_stream=True, **kw, **c)
        for r in (r0, r1):
            assert r["plan"]["form"] == form and r["plan"]["bn"] == (192 if "S16" in form or "F8" in form else 256), r["plan"]
        np.testing.assert_array_equal(r1["y"], r0["y"], err_msg=name)
        if "stats" in name:
            np.testing.assert_array_equal(r1["stats"], r0["stats"], err_msg=name)
        if form == "DA_W2" and name == "resid":
            ref, _ = _ragged_conv(_act_ref(_t(x), 2, norm, alpha), w, b, lens, pad, d)
            valid = np.arange(L)[None, None, :] < lens[:, None, None]
            err = np.abs(np.where(valid, r1["y"] - (ref + res), 0.0)).max()
            print(f"epi_stream {form} + residual: max err vs float64 {err:.2e}")
            assert err < 3e-5
            assert np.all(np.where(valid, 0.0, r1["y"]) == 0.0)


# ---- one descriptor behind every wrapper -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_every_plain_wrapper_fills_the_same_descriptor(mode):
    """One plain stride-1 conv through conv1d, conv1d_epilogue, conv1d_full and conv1d_opts: bit-identical y.  The smallest shapes
    suffice: this is about the wrappers' argument mapping onto kx_test_conv_args, not about a kernel."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(40 + mode)
    x = rng.standard_normal((2, 16, 40), dtype=np.float32)
    w, b = _weights(rng, 32, 16, 3), rng.standard_normal(32, dtype=np.float32)
    y = hk.conv1d(x, w, b, pad=1, mode=mode)
    assert y.shape == (2, 32, 40) and np.isfinite(y).all() and np.abs(y).max() > 0.1
    np.testing.assert_array_equal(hk.conv1d_epilogue(x, w, b, pad=1, mode=mode), y)
    np.testing.assert_array_equal(hk.conv1d_full(x, w, b, pad=1, mode=mode), y)
    np.testing.assert_array_equal(hk.conv1d_opts(x, w, b, pad=1, mode=mode)["y"], y)


def test_every_transposed_wrapper_fills_the_same_descriptor():
    """The polyphase transposed conv (stride 6, k = 12, pad = 3, leaky 0.1 on the input) through conv_transpose,
    conv1d(transposed=True) and conv1d_opts(up_stride=6): bit-identical y."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(42)
    x = rng.standard_normal((2, 16, 12), dtype=np.float32)
    w, b = _weights(rng, 16, 16, 12), rng.standard_normal(16, dtype=np.float32)
    y = hk.conv_transpose(x, w, b, stride=6, act=1, slope=0.1)
    assert y.shape == (2, 16, 72) and np.isfinite(y).all() and np.abs(y).max() > 0.1
    np.testing.assert_array_equal(hk.conv1d(x, w, b, stride=6, pad=3, transposed=True, act=1, slope=0.1, mode=1), y)
    np.testing.assert_array_equal(hk.conv1d_opts(x, w, b, act=1, slope=0.1, up_stride=6)["y"], y)
