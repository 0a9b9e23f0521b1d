"""Float64 references and checks for the generator's ragged conv launches -- strided convs, polyphase transposed convs with a
residual, an output offset and a reflected first column, convs on the 120 f + 1 axis, row-slice views -- shared by
tests/test_conv_ragged_cpu.py and tests/test_gpu_conv_ragged.py, and a float32 stand-in of hip_koko.conv1d_opts that the CPU
file runs the checks against, whole and with one fault at a time.

Every reference is written from the definition, one utterance at a time on its own length: utterance b of a batch with units
lens[b] (the model's frames) stores lin = lens[b] * len_in[0] + len_in[1] input columns and owns lout = lens[b] * len_out[0] +
len_out[1] output columns (+ 1 with up_off); what lies past them is not its data."""
import numpy as np
import torch
import torch.nn.functional as F

SENTINEL = np.float32(-12345.5)  # what the hook leaves in every output column an utterance does not own
U = 2.0 ** -24                   # unit round-off of float32
VIEW_ROWS, VIEW_TOP = 8, 3       # a view sits VIEW_TOP rows below the top of a tensor VIEW_ROWS rows taller


def own_lengths(lens, len_in, len_out):
    """(stored input columns, owned output columns without the offset column) per utterance."""
    lens = np.asarray(lens, dtype=np.int64)
    return lens * len_in[0] + len_in[1], lens * len_out[0] + len_out[1]


def conv_out_len(lin, k, stride=1, pad=0, dil=1, up_stride=0):
    """The conv's own output count on lin input columns: plain (lin + 2 pad - dil (k-1) - 1) / stride + 1, polyphase s lin."""
    return up_stride * lin if up_stride else (lin + 2 * pad - dil * (k - 1) - 1) // stride + 1


def input_transform(x, act=0, slope=0.0, alpha=None, norm=None):
    """The fused input transform on one utterance x [Cin,L] (torch, any float type): AdaIN affine (norm = (mean, scale, shift), each
    [Cin]), then leaky (act 1) or snake (act 2)."""
    if norm is not None:
        x = (x - norm[0][:, None]) * norm[1][:, None] + norm[2][:, None]
    if act == 2:
        a = alpha[:, None]
        return x + (1 / a) * torch.sin(a * x) ** 2
    if act == 1:
        return F.leaky_relu(x, slope)
    return x


def _tt(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def conv_one(xi, w, bias, *, stride=1, pad=0, dil=1, act=0, slope=0.0, alpha=None, norm=None, resid=None, up_stride=0, up_off=False,
             dtype=torch.float64):
    """One utterance by the definition: xi [Cin,lin] -> [Cout, lout (+ 1 with up_off)] as a numpy array of `dtype`.  norm = (mean,
    scale, shift) of this utterance, resid [Cout, lout (+ 1)] its own residual columns."""
    xt = input_transform(_tt(xi, dtype), act, slope, _tt(alpha, dtype), None if norm is None else [_tt(n, dtype) for n in norm])[None]
    if up_stride:
        y = F.conv_transpose1d(xt, _tt(w, dtype), _tt(bias, dtype), stride=up_stride, padding=(w.shape[2] - up_stride) // 2)
        if up_off:  # ReflectionPad1d((1, 0)) of the up-sampled axis
            y = torch.cat([y[..., 1:2], y], dim=-1)
    else:
        y = F.conv1d(xt, _tt(w, dtype), _tt(bias, dtype), stride=stride, padding=pad, dilation=dil)
    y = y[0]
    if resid is not None:
        y = y + _tt(resid, dtype)
    return y.numpy()


def reference(x, w, bias, lens, len_in, len_out, *, resid=None, norm=None, **conv):
    """Float64 reference of a ragged launch: a list of B arrays [Cout, owned columns], each utterance convolved alone over its own
    lin columns (conv = the keywords of conv_one).  norm [3,B,Cin], resid [B,Cout,>= owned columns]."""
    lin, lout = own_lengths(lens, len_in, len_out)
    own = lout + (1 if conv.get("up_off") else 0)
    refs = []
    for b in range(len(lin)):
        r = conv_one(x[b, :, :lin[b]], w, bias, resid=None if resid is None else resid[b, :, :own[b]],
                     norm=None if norm is None else norm[:, b], **conv)
        assert r.shape[1] == own[b], (b, r.shape, own[b])
        refs.append(r)
    return refs


def row_sums(refs):
    """(sum, sum of squares) [B,Cout,2] in float64 of each utterance's rows over its own columns."""
    return np.stack([np.stack([np.asarray(r, dtype=np.float64).sum(axis=1), (np.asarray(r, dtype=np.float64) ** 2).sum(axis=1)], axis=1)
                     for r in refs])


# ---- the checks --------------------------------------------------------------------------------------------------------------

def check_owned(y, refs, bound):
    """Every owned column within `bound` of the reference (a NaN fails).  Returns the worst error."""
    worst = 0.0
    for b, r in enumerate(refs):
        err = np.abs(y[b, :, :r.shape[1]].astype(np.float64) - r)
        assert np.isfinite(err).all(), f"utterance {b}: a NaN or an infinity in its owned columns"
        worst = max(worst, float(err.max()))
        at = np.unravel_index(int(err.argmax()), err.shape)
        assert err.max() < bound, f"utterance {b}: error {err.max():.3e} at (row, column) {at} of {r.shape}, bound {bound:.1e}"
    return worst


def check_untouched(y, refs):
    """The sentinel in every column an utterance does not own."""
    for b, r in enumerate(refs):
        rest = y[b, :, r.shape[1]:]
        assert np.all(rest == SENTINEL), f"utterance {b}: {int((rest != SENTINEL).sum())} value(s) written past its {r.shape[1]} columns"


def check_sums(stats, y, refs, stat_cols):
    """The fused (sum, sum of squares) against the float64 sums of the stored float32 rows over their own columns.  A slot adds
    stat_cols values in float32 in any order, the slots are added in float64 and the result is rounded once (the envelope of
    tests/test_gpu_norm_kernels.py, _slot_envelope, before it is carried to the variance): |S - S64| <= n U sum|v| + U |S64| and
    |Q - Q64| <= (n U + U) Q64.  Returns the worst fraction of the bound."""
    worst = 0.0
    for b, r in enumerate(refs):
        v = y[b, :, :r.shape[1]].astype(np.float64)
        s64, q64, a64 = v.sum(axis=1), (v * v).sum(axis=1), np.abs(v).sum(axis=1)
        bs = stat_cols * U * a64 + U * np.abs(s64) + 1e-30
        bq = (stat_cols + 1) * U * q64 + 1e-30
        fs = np.abs(stats[b, :, 0] - s64) / bs
        fq = np.abs(stats[b, :, 1] - q64) / bq
        assert np.isfinite(stats[b]).all(), f"utterance {b}: statistics not finite"
        assert fs.max() <= 1.0 and fq.max() <= 1.0, f"utterance {b}: sums off by {fs.max():.2f} / {fq.max():.2f} of the slot envelope"
        worst = max(worst, float(fs.max()), float(fq.max()))
    return worst


def slot_envelope(mean, var, n):
    """tests/test_gpu_norm_kernels.py, _slot_envelope: what n-column float32 partial sums can cost the scale (bound, e)."""
    E = 3.0 * n * U * (var + mean * mean)
    e = E / (var + 1e-5)
    return 0.5 * e * (1.0 + e) + 4 * U, e


def check_planes(planes, gb, y, refs, stat_cols):
    """(mean, scale, shift) [3,B,Cout] from the fused sums through the finalize pass, against the float64 InstanceNorm of the stored
    rows over their own columns, asserted as test_fused_statistics_through_finalize_stay_inside_the_slot_envelope asserts them."""
    C = y.shape[1]
    worst = 0.0
    for b, r in enumerate(refs):
        v = y[b, :, :r.shape[1]].astype(np.float64)
        mean, var = v.mean(axis=1), v.var(axis=1)
        scale = (np.float32(1.0) + gb[b, :C]).astype(np.float64) / np.sqrt(var + 1e-5)
        pm, ps = planes[0, b].astype(np.float64), planes[1, b].astype(np.float64)
        assert np.isfinite(planes[:, b]).all() and np.all(ps / scale > 0), f"utterance {b}: planes not finite or of the wrong sign"
        bound, e = slot_envelope(mean, var, stat_cols)
        es = np.abs(ps - scale) / np.abs(scale)
        ok = e < 0.5
        assert np.all(es[ok] <= bound[ok]), f"utterance {b}: scale off by {float((es / bound)[ok].max()):.2f} of the slot envelope"
        assert np.all(np.abs(pm - mean) <= stat_cols * U * np.sqrt(var + mean * mean) + U * np.abs(mean) + 1e-12), f"utterance {b}: mean"
        assert np.array_equal(planes[2, b], gb[b, C:]), f"utterance {b}: shift is not beta"
        if ok.any():
            worst = max(worst, float((es / bound)[ok].max()))
    return worst


# ---- the stand-in ------------------------------------------------------------------------------------------------------------

class StandInStateError(RuntimeError):
    """The stand-in's KX_ERR_STATE: something outside the launch's own rows changed."""


FAULTS = ("neighbour", "lout_max", "reflect_up0", "resid_no_off", "origin_second_tile", "stats_lmax", "view_bs")


def standin_conv1d_opts(x, w, bias=None, pad=0, dil=1, act=0, slope=0.0, alpha=None, norm=None, resid=None, y_init=None,
                        out_mul=1.0, out_div=1.0, want_stats=False, lens=None, pad_ld=False, flat=False, mode=1, device=0, pre=False,
                        in_up2=False, epi=0, merged=False, tmajor=False, prec1=0, act_shift=0, epi_stream=False, want_norm=None,
                        up_stride=0, stride=1, len_in=None, len_out=None, up_off=False, view=False, fault=None):
    """hip_koko.conv1d_opts in float32 torch, for the launches this module is about (length maps given; no in_up2, merged, time-major
    or accumulating store): the same arguments, the same dict back, y at its stored shape with SENTINEL wherever no utterance owns
    it.  fault: one of FAULTS, the stand-in made wrong in the way a kernel could be."""
    assert fault is None or fault in FAULTS
    assert len_in is not None and len_out is not None and lens is not None
    assert not (in_up2 or merged or tmajor or epi or y_init is not None) and out_mul == 1.0 and out_div == 1.0
    x, w = np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32)
    B, Cin, L = x.shape
    k = w.shape[2]
    Cout = w.shape[1] if up_stride else w.shape[0]
    off = 1 if up_off else 0
    lin, lout = own_lengths(lens, len_in, len_out)
    assert lin.max() <= L and np.array_equal(lout, conv_out_len(lin, k, stride, pad, dil, up_stride))
    Ly = conv_out_len(L, k, stride, pad, dil, up_stride) + off
    f32 = torch.float32
    conv = dict(stride=stride, pad=pad, dil=dil, act=act, slope=slope, alpha=alpha, up_stride=up_stride, dtype=f32)

    # the tensors as the launch sees them: (view) row slices of taller ones, foreign input rows NaN, foreign output rows SENTINEL
    vr, vt = (VIEW_ROWS, VIEW_TOP) if view else (0, 0)

    def tall(src, C, width, fill):
        t = np.full((B, C + vr, width), fill, dtype=np.float32)
        if src is not None:
            t[:, vt:vt + C] = src
        return t.reshape(-1)

    def rows_of(flat, b, C, width, wrong_bs):  # utterance b's C rows of a flat tall tensor (a view: writes go through)
        bs = (C if wrong_bs else C + vr) * width
        return flat[b * bs + vt * width: b * bs + (vt + C) * width].reshape(C, width)

    xs = tall(x, Cin, L, np.nan)
    rs = None if resid is None else tall(np.asarray(resid, dtype=np.float32), Cout, Ly, np.nan)
    ys = tall(None, Cout, Ly, SENTINEL)
    wrong_bs = fault == "view_bs" and view
    stats = np.zeros((B, Cout, 2), dtype=np.float32)
    for b in range(B):
        xb = rows_of(xs, b, Cin, L, wrong_bs)
        n, no = int(lin[b]), int(lout[b])
        xi = xb[:, :n]
        nb = None if norm is None else np.asarray(norm, dtype=np.float32)[:, b]
        if fault == "neighbour" and n < L:  # what lies behind the utterance's end is read as if it were its own
            xi = np.concatenate([xi, rows_of(xs, (b + 1) % B, Cin, L, wrong_bs)[:, n:n + k * dil]], axis=1)
        up = conv_one(xi, w, bias, norm=nb, **conv)[:, :no]
        if fault == "origin_second_tile" and not up_stride and no > 128:  # p0 = t0 * stride for the second column tile
            shifted = np.concatenate([xi[:, pad:], np.zeros((Cin, pad), dtype=np.float32)], axis=1)
            up[:, 128:] = conv_one(shifted, w, bias, norm=nb, **conv)[:, 128:no]
        if fault == "lout_max":
            full = conv_one(np.concatenate([xi, np.zeros((Cin, L - n), dtype=np.float32)], axis=1), w, bias, norm=nb, **conv)
            up, no = full, full.shape[1]
        if up_off:
            up = np.concatenate([up[:, 0:1] if fault == "reflect_up0" else up[:, 1:2], up], axis=1)
        if rs is not None:
            rb = rows_of(rs, b, Cout, Ly, wrong_bs)
            if fault == "resid_no_off" and up_off:
                up = up + np.concatenate([rb[:, 0:1], rb[:, :no]], axis=1)
            else:
                up = up + rb[:, :no + off]
        rows_of(ys, b, Cout, Ly, wrong_bs)[:, :no + off] = up
        sv = up.astype(np.float64)
        if fault == "stats_lmax":  # the sums of every column of the launch, whatever lies there
            sv = conv_one(xb, w, bias, norm=nb, **conv).astype(np.float64)
        stats[b, :, 0], stats[b, :, 1] = sv.sum(axis=1), (sv * sv).sum(axis=1)
    y_tall = ys.reshape(B, Cout + vr, Ly)
    if view and not (np.all(y_tall[:, :vt] == SENTINEL) and np.all(y_tall[:, vt + Cout:] == SENTINEL)):
        raise StandInStateError("the stand-in wrote into a foreign row of the output tensor")
    y = y_tall[:, vt:vt + Cout].copy()
    planes = None
    if want_norm is not None:
        gb = np.asarray(want_norm, dtype=np.float32)
        cnt = np.where(fault == "stats_lmax", Ly, lout).astype(np.float64)[:, None]
        mean = stats[:, :, 0] / cnt
        var = np.maximum(stats[:, :, 1] / cnt - mean * mean, 0.0)
        planes = np.stack([mean, (np.float32(1.0) + gb[:, :Cout]) / np.sqrt(var + 1e-5), gb[:, Cout:]]).astype(np.float32)
    plan = {"form": "STANDIN", "stat_cols": 64, "bn": 128, "flat_bn": 0, "merged": 0, "pre": 0}
    return {"y": y, "plan": plan, "stats": stats if want_stats else None, "norm": planes}


# ---- the launches of Model::back_half that both test files run ------------------------------------------------------------------

CASES = {
    # noise_convs.0: 22 -> 256 (and 22 -> 40: a partial row tile), 841 / 121 / 481 input and 140 / 20 / 80 output columns
    "noise0": dict(Cin=22, Cout=256, k=12, stride=6, pad=3, len_in=(120, 1), len_out=(20, 0), units=(7, 1, 4)),
    "noise0_40": dict(Cin=22, Cout=40, k=12, stride=6, pad=3, len_in=(120, 1), len_out=(20, 0), units=(7, 1, 4)),
    # decoder.F0_conv / N_conv: one row of a taller tensor in, one row of a taller tensor out
    "f0": dict(Cin=1, Cout=1, k=3, stride=2, pad=1, len_in=(2, 0), len_out=(1, 0), units=(130, 1, 65), view=True),
    # generator.ups.0 / ups.1: row tiles cut channels (128 / 10, 128 / 6)
    "ups0": dict(Cin=64, Cout=26, up_stride=10, act=1, slope=0.1, resid=True, len_in=(2, 0), len_out=(20, 0), units=(400, 1, 65)),
    "ups1": dict(Cin=48, Cout=52, up_stride=6, act=1, slope=0.1, resid=True, up_off=True, len_in=(20, 0), len_out=(120, 0),
                 units=(40, 1, 7)),
    # the 120 f + 1 axis at stride 1: a stage-1 resblock conv and conv_post
    "res121": dict(Cin=128, Cout=128, k=7, dil=3, pad=9, act=2, norm=True, resid=True, len_in=(120, 1), len_out=(120, 1), units=(5, 1, 2)),
    "post121": dict(Cin=128, Cout=22, k=7, pad=3, act=1, slope=0.01, len_in=(120, 1), len_out=(120, 1), units=(5, 1, 2)),
}


def make_case(name, overrides=None):
    """Inputs of one of CASES: N(0,1) inputs and residual, weights N(0,1) / sqrt(Cin k) (transposed: / sqrt(2 Cin)), a bias.  Returns
    (x, w, bias, kw) with kw the keywords of conv1d_opts (lens, maps, pad_ld and the layer's own)."""
    c = dict(CASES[name], **(overrides or {}))
    rng = np.random.default_rng(sum(name.encode()) * 7 + c["Cout"])
    lens = np.array(c["units"], dtype=np.int32)
    B, Cin, Cout, s = len(lens), c["Cin"], c["Cout"], c.get("up_stride", 0)
    k = 2 * s if s else c["k"]
    lin, lout = own_lengths(lens, c["len_in"], c["len_out"])
    L = int(lin.max())
    off = 1 if c.get("up_off") else 0
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    if s:
        w = (rng.standard_normal((Cin, Cout, k), dtype=np.float32) / np.sqrt(2 * Cin)).astype(np.float32)
    else:
        w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    bias = rng.standard_normal(Cout, dtype=np.float32)
    kw = dict(lens=lens, len_in=c["len_in"], len_out=c["len_out"], pad_ld=True, pad=c.get("pad", 0), dil=c.get("dil", 1),
              act=c.get("act", 0), slope=c.get("slope", 0.0), stride=c.get("stride", 1), up_stride=s, up_off=bool(off),
              view=bool(c.get("view")))
    if c.get("act") == 2:
        kw["alpha"] = (rng.random(Cin, dtype=np.float32) + 0.5).astype(np.float32)
    if c.get("norm"):
        norm = rng.standard_normal((3, B, Cin), dtype=np.float32)
        norm[1] = 1.0 + 0.2 * norm[1]
        kw["norm"] = norm
    if c.get("resid"):
        kw["resid"] = rng.standard_normal((B, Cout, int(lout.max()) + off), dtype=np.float32)
    return x, w, bias, kw


def case_reference(x, w, bias, kw):
    """reference() for the keywords make_case returns."""
    return reference(x, w, bias, kw["lens"], kw["len_in"], kw["len_out"], resid=kw.get("resid"), norm=kw.get("norm"), stride=kw["stride"],
                     pad=kw["pad"], dil=kw["dil"], act=kw["act"], slope=kw["slope"], alpha=kw.get("alpha"), up_stride=kw["up_stride"],
                     up_off=kw["up_off"])


def one_utterance(x, kw, b):
    """Utterance b of a case as its own B = 1 call: (x, kw) cut to its stored columns."""
    lin, lout = own_lengths(kw["lens"], kw["len_in"], kw["len_out"])
    k1 = dict(kw, lens=kw["lens"][b:b + 1])
    if kw.get("norm") is not None:
        k1["norm"] = np.ascontiguousarray(kw["norm"][:, b:b + 1])
    if kw.get("resid") is not None:
        k1["resid"] = np.ascontiguousarray(kw["resid"][b:b + 1, :, :int(lout[b]) + (1 if kw["up_off"] else 0)])
    return np.ascontiguousarray(x[b:b + 1, :, :int(lin[b])]), k1
