"""GPU: the weight images every conv, GEMM and transposed conv runs on (kokorox_amd/csrc/conv_call.hip: pack_conv, pack_convT,
add_bf16_image, add_f8_image), byte for byte against oracle/weight_image_ref.py (held to its definitions by
tests/test_weight_images_cpu.py), the edges of the one-shift-per-layer rule, what the pack path refuses, and every conv form along
the SPREAD of a layer's weights: rows 2^-r below the layer's maximum, whose error is relative to themselves because the next
InstanceNorm rescales every channel.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import weight_image_ref as R

pytestmark = pytest.mark.gpu


def _cpu_file():
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_weight_images_cpu.py")
    spec = importlib.util.spec_from_file_location("_weight_image_cases", p)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CPU = _cpu_file()
IMAGES = ("w", "w16", "w16b", "w8x")


def _assert_images_equal(got, ref, tag):
    for k in ("BM", "rows", "n_chunks", "n_chunks16", "K"):
        assert got[k] == ref[k], (tag, k, got[k], ref[k])
    assert got["unscale"] == 2.0 ** -ref["ws"], (tag, got["unscale"], ref["ws"])
    for k in IMAGES:
        assert got[k].size == ref[k].size, (tag, k, got[k].size, ref[k].size)
        bad = np.flatnonzero(got[k] != ref[k])
        assert bad.size == 0, (tag, k, f"{bad.size} bytes differ, the first at {bad[0]}: {got[k][bad[0]]:#x} for {ref[k][bad[0]]:#x}")


# ---- a. the images, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,sources,up_stride", CPU.image_cases(), ids=[c[0] for c in CPU.image_cases()])
def test_images_equal_the_reference_byte_for_byte(cid, sources, up_stride):
    """Every image of the layer equals the reference's bytes (so every padding slot holds +0: the hook pre-fills the images with
    0xC3), the guards behind the images are intact (the hook: KX_ERR_STATE otherwise) and unscale is 2^-ws."""
    from kokorox_amd import hip_koko as hk
    got = hk.weight_images(sources, up_stride=up_stride)
    ref = R.images(sources, up_stride)
    _assert_images_equal(got, ref, cid)
    d = ref["dims"]
    _, _, free = R.unpack_w16(d, got["w16"].view(np.float16))
    assert not got["w16"].view(np.uint16)[free].any(), cid


def test_hook_refuses_sizes_no_layer_has():
    from kokorox_amd import hip_koko as hk
    lib = hk.load_test_library()
    import ctypes as C
    w = np.zeros(4096 * 2, dtype=np.float32)
    for rows, Cin, K in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (4097, 1, 1), (1, 2049, 1), (1, 1, 25)):
        ptrs = (C.c_void_p * 1)(w.ctypes.data)
        rws = np.array([rows], dtype=np.int32)
        meta, un = np.zeros(9, dtype=np.int64), np.zeros(1, dtype=np.float32)
        bufs = [np.zeros(16, dtype=np.uint8) for _ in range(4)]
        outs = (C.c_void_p * 4)(*[b.ctypes.data for b in bufs])
        caps = np.full(4, 16, dtype=np.int64)
        err = C.create_string_buffer(256)
        rc = lib.kx_test_weight_images(0, ptrs, rws.ctypes.data, 1, Cin, K, 0, meta.ctypes.data, un.ctypes.data, outs, caps.ctypes.data, err, len(err))
        assert rc == hk.KX_ERR_INVALID and b"out of range" in err.value, (rows, Cin, K, rc, err.value)


# ---- b. the shift's edges -----------------------------------------------------------------------------------------------------------
def _with_absmax(shape, seed, absmax):
    """A draw whose largest magnitude is exactly `absmax` (float32), every other weight at most half of it."""
    w = CPU.draw(shape, seed) * np.float32(0.5)
    w = (w * np.float32(2.0) ** np.floor(np.log2(float(absmax)))).astype(np.float32)
    w[shape[0] // 2, shape[1] // 3, shape[2] - 1] = -np.float32(absmax)
    assert np.abs(w).max() == np.float32(absmax)
    return w


@pytest.mark.parametrize("e", [-3, 0, 5])
def test_shift_at_a_power_of_two_and_one_ulp_below(e):
    from kokorox_amd import hip_koko as hk
    p2 = np.float32(2.0 ** e)
    for absmax, ws in ((p2, 11 - e), (np.nextafter(p2, np.float32(0)), 12 - e)):
        w = _with_absmax((130, 24, 7), 40 + e, absmax)
        got, ref = hk.weight_images([w]), R.images([w])
        assert ref["ws"] == ws and got["unscale"] == 2.0 ** -ws, (e, absmax, got["unscale"])
        _assert_images_equal(got, ref, (e, float(absmax)))


def test_all_zero_layer():
    """Shift 0, every image zero, and the conv's output is the bias."""
    from kokorox_amd import hip_koko as hk
    w = np.zeros((130, 32, 7), dtype=np.float32)
    got = hk.weight_images([w])
    assert got["unscale"] == 1.0
    for k in IMAGES:
        assert got[k].size and not got[k].any(), k
    rng = np.random.default_rng(3)
    x, b = rng.standard_normal((2, 32, 70), dtype=np.float32), rng.standard_normal(130, dtype=np.float32)
    for mode in (0, 1, 2, 3, 1 | 0x200):
        y = hk.conv1d(x, w, b, pad=3, mode=mode)
        np.testing.assert_array_equal(y, np.broadcast_to(b[None, :, None], y.shape))


def test_upper_clamp_of_the_shift():
    """absmax = 2^-14: 11 + 14 = 25 is clamped to 24, the largest weight lands at 2^10."""
    from kokorox_amd import hip_koko as hk
    w = _with_absmax((130, 24, 7), 50, np.float32(2.0 ** -14))
    got, ref = hk.weight_images([w]), R.images([w])
    assert ref["ws"] == 24 and got["unscale"] == 2.0 ** -24
    _assert_images_equal(got, ref, "2^-14")
    assert np.abs(ref["hi"].astype(np.float32)).max() == 1024.0


def test_lower_clamp_of_the_shift():
    """absmax = 2^21: 11 - 21 = -10 is clamped to -8.  hi is finite (2^13 at most), the 8-bit hi operand of the largest weight is at
    its clamp (2^-4 2^13 = 512 -> 448), and the f16x3 conv is still inside its class against float64 (3e-5 of the output's scale,
    tests/test_gpu_kernels.py): the split itself loses nothing up there, only the 8-bit cross terms do."""
    from kokorox_amd import hip_koko as hk
    w = _with_absmax((128, 32, 7), 51, np.float32(2.0 ** 21))
    got, ref = hk.weight_images([w]), R.images([w])
    assert ref["ws"] == -8 and got["unscale"] == 256.0
    _assert_images_equal(got, ref, "2^21")
    hi = got["w16"].view(np.float16)
    assert np.isfinite(hi).all() and np.abs(hi.astype(np.float32)).max() == 8192.0
    at = R.addr_w8x(ref["dims"], np.array(64), np.array(10), np.array(6), 0)
    assert got["w8x"].size and got["w8x"][int(at)] == 0xfe  # (-448: the weight is -2^21)
    rng = np.random.default_rng(52)
    x, b = rng.standard_normal((2, 32, 140), dtype=np.float32), rng.standard_normal(128, dtype=np.float32)
    ref_y = F.conv1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=3).numpy()
    scale = max(1.0, float(np.sqrt((ref_y ** 2).mean())))
    for mode in (1, 2, 3):
        y = hk.conv1d(x, w, b, pad=3, mode=mode)
        err = float(np.abs(y - ref_y).max())
        print(f"absmax 2^21, mode {mode}: max err {err / scale:.2e} of scale {scale:.3g}")
        assert np.isfinite(y).all() and err < 3e-5 * scale, (mode, err / scale)


# ---- c. what the pack path refuses -----------------------------------------------------------------------------------------------------
BIGGEST = np.float32(65504.0 * 256.0)  # max|w| 2^-8 = 65504: the largest layer the split carries


@pytest.mark.parametrize("what,value,why", [("nan", np.nan, "non-finite"), ("inf", np.inf, "non-finite"), ("-inf", -np.inf, "non-finite"),
                                            ("2^24", 2.0 ** 24, "beyond the split's range"),
                                            ("one ulp past", np.nextafter(BIGGEST, np.float32(np.inf)), "beyond the split's range")])
def test_pack_path_refuses_what_it_cannot_carry(what, value, why):
    """The contract (conv_call.hip): a layer with a NaN or an infinite weight, or with max|w| 2^ws > 65504, is
    refused when it is packed, KX_ERR_INVALID, with a message that says which -- in a plain layer, in the second of two sources, in
    a transposed weight, and through the conv hook, whose layer comes from the same packers."""
    from kokorox_amd import hip_koko as hk
    assert R.carried(np.float32(value)) == why
    w = CPU.draw((130, 24, 7), 60)
    w[77, 5, 2] = value
    clean = CPU.draw((40, 24, 7), 61)
    wt = CPU.draw((17, 5, 12), 62)
    wt[3, 4, 11] = value
    x = np.zeros((1, 24, 20), dtype=np.float32)
    calls = [lambda: hk.weight_images([w]), lambda: hk.weight_images([clean, w]), lambda: hk.weight_images([wt], up_stride=6),
             lambda: hk.conv1d(x, w, None, pad=3, mode=1), lambda: hk.conv1d(x, w, None, pad=3, mode=0)]
    for call in calls:
        with pytest.raises(hk.KokoroxHipError) as ei:
            call()
        assert ei.value.code == hk.KX_ERR_INVALID and why in str(ei.value), str(ei.value)
        with pytest.raises(ValueError, match=why):
            R.images([w])


def test_largest_layer_the_split_carries():
    from kokorox_amd import hip_koko as hk
    w = _with_absmax((130, 24, 7), 63, BIGGEST)
    got, ref = hk.weight_images([w]), R.images([w])
    _assert_images_equal(got, ref, "65504 * 256")
    assert np.abs(got["w16"].view(np.float16).astype(np.float32)).max() == 65504.0


def test_model_load_names_the_tensor_it_refuses(hip_model, blob_path):
    """A NaN in one conv weight of the container: kx_create_from_device_blob fails with the usual load error, "weight blob: ...",
    naming the tensor and the reason; the session's model is unharmed."""
    from kokorox_amd import hip_koko as hk
    from kokorox_amd import weights as W
    name = "decoder.generator.ups.1.weight"
    table, _, _ = W._layout(W.tensor_spec())
    _, shape, off, nbytes = next(t for t in table if t[0] == name)
    a = np.fromfile(blob_path, dtype=np.uint8)
    a[off + 4 * 1001: off + 4 * 1002] = np.frombuffer(np.float32(np.nan).tobytes(), dtype=np.uint8)
    buf = torch.from_numpy(a).cuda()
    with pytest.raises(RuntimeError) as ei:
        hk.HipKoko.from_device_blob(buf.data_ptr(), buf.numel(), 0)
    del buf
    msg = str(ei.value)
    assert "weight blob: bad weights " + name in msg and "non-finite" in msg, msg
    audio = hip_model.infer([[0, 5, 6, 0]], [[0.0] * 256], 1.0)
    assert audio.shape[0] > 0 and audio.shape[0] % 600 == 0


# ---- d. every conv form along the spread of its weights ------------------------------------------------------------------------------
F8 = 0x200
CLASSES = (0, 4, 8, 10, 12, 14, 16, 20)  # class c = row mod 8 holds the class-0 draw's bits times 2^-CLASSES[c]
# (name, hook mode, prec1, the form the plan must return, its tile width or None, the reference's restatement of its arithmetic)
PLAIN_RUNS = [("f32", 0, 0, ("F32",), None, "f32"), ("f16x3", 1, 0, None, None, "f16x3"), ("f16x3lds", 2, 0, ("LDS",), None, "f16x3"),
              ("f16x3da", 3, 0, ("DA", "DA_W2", "DA_S16", "DA_PRE"), None, "f16x3"), ("f16f8/128", 1 | F8, 0, ("DA_F8",), 128, "f16f8"),
              ("f16f8/192", 3 | F8, 0, ("DA_F8",), 192, "f16f8"), ("f16", 3, 1, ("DA",), None, "f16"), ("bf16", 3, 2, ("DA",), None, "bf16")]
# (the reduced-precision forms exist on the direct-A kernel only: hook mode 3 routes these small grids there, as a forward's larger ones go)
UP_RUNS = [r for r in PLAIN_RUNS if not r[1] & F8]
# (taps, Cin, Cout, columns, dilation)
SPREAD_SHAPES = [(7, 128, 128, 193, 3), (3, 256, 256, 65, 1), (11, 64, 256, 130, 1)]
UPSAMPLER = (64, 32, 6, 50)  # Cin, Cout, stride, columns; leaky input


def _rel_rms(y, ref, valid, groups):
    """Relative rms error over the valid columns of each group of rows: rms(y - ref) / rms(ref)."""
    out = []
    for rows in groups:
        e, r = (y - ref)[:, rows][valid[:, rows]], ref[:, rows][valid[:, rows]]
        out.append(float(np.sqrt((e ** 2).mean()) / np.sqrt((r ** 2).mean())))
    return np.array(out)


class _Spread:
    """One conv problem and everything the runs share: the float64 reference, the activation and weight operands of the
    reference's restatements, and their per-group figures (computed once)."""

    def __init__(self, w, x, norm, conv, v64, valid, groups, kw, n_terms):
        self.w, self.x, self.norm, self.valid, self.groups, self.kw = w, x, norm, valid, groups, kw
        self.ref = conv(v64, torch.from_numpy(w).double())
        a, wo = R.act_operands(v64.numpy().astype(np.float32)), R.weight_operands(w)
        tt = lambda d: {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
        a, wo = tt(a), tt(wo)
        self.emu = {f: _rel_rms(R.emulate_conv(f, a, wo, conv).numpy(), self.ref.numpy(), valid, groups) for f in R.FORMS}
        self.ref = self.ref.numpy()
        # float32 accumulation of n_terms products: independent roundings of the partial sums, each at most 2^-24 of a partial
        # sum that random-walks up to the result, are sqrt(n_terms) 2^-24 of it in rms -- with a factor 4
        self.allow = 4.0 * np.sqrt(n_terms) * 2.0 ** -24

    def run(self, name, mode, prec1, forms, bn):
        from kokorox_amd import hip_koko as hk
        r = hk.conv1d_opts(self.x, self.w, None, norm=self.norm, mode=mode, prec1=prec1, **self.kw)
        plan = r["plan"]
        if forms is None:
            assert plan["form"] not in ("F32", "DA_F8") and not plan["p1"], (name, plan)
        else:
            assert plan["form"] in forms and plan["p1"] == (prec1 != 0) and plan["bf"] == (prec1 == 2), (name, plan)
        assert bn is None or plan["bn"] == bn, (name, plan)
        y = r["y"]
        assert np.isfinite(y).all(), name                                  # 1.
        assert np.all(y[~np.broadcast_to(self.valid, y.shape)] == 0.0), name
        return y, _rel_rms(y.astype(np.float64), self.ref, self.valid, self.groups), plan["form"]


def _affine_inputs(Cin, L, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, Cin, L), dtype=np.float32)
    norm = rng.standard_normal((3, 2, Cin), dtype=np.float32)
    norm[1] = 1.0 + 0.2 * norm[1]
    n = torch.from_numpy(norm).double()
    v = (torch.from_numpy(x).double() - n[0][:, :, None]) * n[1][:, :, None] + n[2][:, :, None]
    return rng, x, norm, v


def _plain_problem(shape, w_of, seed):
    """Snake input, alpha in [0.5, 2], a ragged batch of two on padded rows (the flat tile list when L % 4 == 1), bias 0."""
    k, Cin, Cout, L, d = shape
    rng, x, norm, v = _affine_inputs(Cin, L, seed)
    alpha = np.exp2(rng.uniform(-1.0, 1.0, Cin)).astype(np.float32)
    al = torch.from_numpy(alpha).double()[None, :, None]
    v = v + torch.sin(al * v) ** 2 / al
    lens = np.array([L, (2 * L) // 3], dtype=np.int32)
    pad = (k - 1) // 2 * d

    def conv(x64, w64):
        y = torch.zeros((2, w64.shape[0], L), dtype=torch.float64)
        for i in range(2):
            n = int(lens[i])
            y[i, :, :n] = F.conv1d(x64[i:i + 1, :, :n], w64, padding=pad, dilation=d)[0]
        return y
    valid = np.broadcast_to(np.arange(L)[None, None, :] < lens[:, None, None], (2, Cout, L))
    kw = dict(pad=pad, dil=d, act=2, alpha=alpha, lens=lens, pad_ld=True, flat=(L % 4 == 1))
    w = w_of(rng, Cout, Cin, k)
    return _Spread(w, x, norm, conv, v, valid, [np.arange(c, Cout, 8) for c in range(8)], kw, Cin * k)


def _class_weights(rng, Cout, Cin, k):
    """Rows in eight classes 2^-r: exact powers of two on one N(0, 1 / (Cin k)) draw, so a class's weights are class 0's bits
    with another exponent; class 0 holds the layer's maximum."""
    w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    scale = np.exp2(-np.array(CLASSES, dtype=np.float32))[np.arange(Cout) % 8]
    w = (w * scale[:, None, None]).astype(np.float32)
    assert np.abs(w).max() == np.abs(w[0::8]).max()
    return w


def _check_spread(p, runs, tag):
    """The four assertions of the module on every run, and both f16f8 tile widths the same bits.

    2. a class's figure is at most the restatement's figure on the same inputs (operands rounded as the reference rounds them,
       products and sums in float64) plus the allowance for the kernel's float32 accumulation, 4 sqrt(Cin K) 2^-24: independent
       roundings of partial sums, with a factor 4.
    3. and at most the ONE-MFMA restatement's figure plus that allowance ("degrades towards one MFMA, never below it"; for the
       bf16 form the one MFMA is the bf16 one).
    4. for r <= 10 it is within 1.5 x the restatement's figure of class 0 plus the allowance (pick_weight_shift's promise)."""
    ys = {}
    for name, mode, prec1, forms, bn, emu in runs:
        y, fig, form = p.run(name, mode, prec1, forms, bn)
        ys[name] = y
        one = p.emu["bf16" if emu == "bf16" else "f16"]
        for c, r in enumerate(CLASSES):
            print(f"{tag} {name:>9} {form:>6} r={r:2d}: rel rms {fig[c]:.2e}  emulation {p.emu[emu][c]:.2e} (x{fig[c] / max(p.emu[emu][c], 1e-30):.2f})  "
                  f"one MFMA {one[c]:.2e}  allowance {p.allow:.1e}")
        for c, r in enumerate(CLASSES):
            assert fig[c] <= p.emu[emu][c] + p.allow, (tag, name, r, fig[c], p.emu[emu][c])      # 2.
            assert fig[c] <= one[c] + p.allow, (tag, name, r, fig[c], one[c])                  # 3.
            if r <= 10:
                assert fig[c] <= 1.5 * p.emu[emu][0] + p.allow, (tag, name, r, fig[c], p.emu[emu][0])  # 4.
    if "f16f8/128" in ys:
        np.testing.assert_array_equal(ys["f16f8/128"], ys["f16f8/192"])


@pytest.mark.parametrize("shape", SPREAD_SHAPES, ids=lambda s: f"k{s[0]}-{s[1]}to{s[2]}")
def test_conv_forms_along_the_spread_of_the_weights(shape):
    p = _plain_problem(shape, _class_weights, 7000 + shape[0])
    _check_spread(p, PLAIN_RUNS, f"k{shape[0]}")


def test_polyphase_upsampler_along_the_spread_of_the_weights():
    """ConvTranspose1d 64 -> 32, stride 6, 50 columns, leaky input; the class belongs to the output channel."""
    Cin, Cout, s, L = UPSAMPLER
    rng, x, norm, v = _affine_inputs(Cin, L, 7100)
    v = torch.where(v > 0, v, v * 0.1)
    w = (rng.standard_normal((Cin, Cout, 2 * s), dtype=np.float32) / np.sqrt(Cin * 2)).astype(np.float32)
    w = (w * np.exp2(-np.array(CLASSES, dtype=np.float32))[np.arange(Cout) % 8][None, :, None]).astype(np.float32)
    conv = lambda x64, w64: F.conv_transpose1d(x64, w64, stride=s, padding=s // 2)
    Lout = (L - 1) * s - 2 * (s // 2) + 2 * s
    valid = np.ones((2, Cout, Lout), dtype=bool)
    p = _Spread(w, x, norm, conv, v, valid, [np.arange(c, Cout, 8) for c in range(8)], dict(act=1, slope=0.1, up_stride=s), Cin * 2)
    _check_spread(p, UP_RUNS, "ups")


@pytest.mark.parametrize("log2_outlier", [10, 14])
def test_one_outlier_weight_sets_the_shift_for_every_row(log2_outlier):
    """The 7-tap shape, every row at one scale, and w[0, 0, 0] = 2^10, then 2^14, times the largest of the rest: the whole layer
    sits that far below its shift.  At 2^10 every row group keeps the form's class: within 1.5 x the restatement's figure of the
    layer WITHOUT the outlier, plus the allowance.  At 2^14 the figures are finite, at most the restatement's and at most the
    one-MFMA restatement's, each plus the allowance."""
    shape = SPREAD_SHAPES[0]
    plain = lambda rng, Cout, Cin, k: (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    base = _plain_problem(shape, plain, 7200)

    def outlier(rng, Cout, Cin, k):
        w = plain(rng, Cout, Cin, k)
        w[0, 0, 0] = 0.0
        w[0, 0, 0] = np.float32(2.0 ** log2_outlier) * np.abs(w).max()
        return w
    p = _plain_problem(shape, outlier, 7200)
    assert np.array_equal(p.w.ravel()[1:], base.w.ravel()[1:]) and R.weight_operands(p.w)["ws"] == R.weight_operands(base.w)["ws"] - log2_outlier
    ys = {}
    for name, mode, prec1, forms, bn, emu in PLAIN_RUNS:
        y, fig, form = p.run(name, mode, prec1, forms, bn)
        ys[name] = y
        one = p.emu["bf16" if emu == "bf16" else "f16"]
        print(f"outlier 2^{log2_outlier} {name:>9} {form:>6}: rel rms {fig.min():.2e} .. {fig.max():.2e}  emulation {p.emu[emu].max():.2e}  "
              f"without the outlier {base.emu[emu].max():.2e}  one MFMA {one.max():.2e}")
        assert np.all(fig <= p.emu[emu] + p.allow), (name, fig, p.emu[emu])
        assert np.all(fig <= one + p.allow), (name, fig, one)
        if log2_outlier == 10:
            assert np.all(fig <= 1.5 * base.emu[emu] + p.allow), (name, fig, base.emu[emu])
    np.testing.assert_array_equal(ys["f16f8/128"], ys["f16f8/192"])
