"""GPU: the generator's conv launches that only the whole forward used to reach, alone through kx_test_conv (hip_koko.conv1d_opts) with the model's
length maps (hip_koko.conv1d_opts: stride, len_in / len_out, up_off, view): the strided noise_convs.0 with fused statistics, the
1 -> 1 strided F0_conv / N_conv between row slices of taller tensors, the polyphase upsamplers ups.0 / ups.1 ragged on padded rows
with their residual, output offset and reflected column, and the stride-1 convs of the 120 f + 1 axis.  The batches are ragged
(three utterances, the shortest a fraction of one tile); the hook puts NaN behind every utterance's own input and residual columns
and a sentinel into every output column it does not own, and fails if a foreign row, the row padding or a guard behind a buffer
changed.

References, checks and cases: oracle/conv_ragged_ref.py (tests/test_conv_ragged_cpu.py shows what each check catches).  Bounds:
2e-5 absolute against float64 for hook modes 0 .. 3, the bound of test_conv1d_mfma and
test_polyphase_with_residual_offset_and_reflection on the same input scale (a float32 torch conv is at 1e-7 .. 3e-6 on these
shapes); the f16f8 case: the bounds of test_f16f8_form_against_float64.  Every case asserts the ConvForm of the plan the hook
launched (named for 256 CUs).  Run with -s to see the measured figures."""
import numpy as np
import pytest

from oracle import conv_ragged_ref as R

pytestmark = pytest.mark.gpu

F8 = 0x200
BOUND = 2e-5


def _each_alone(hk, x, w, b, kw, y, refs, what, **call):
    """Every utterance equals its own B = 1 call (a tensor of exactly its own columns) bit for bit."""
    for i, ref in enumerate(refs):
        x1, k1 = R.one_utterance(x, kw, i)
        y1 = hk.conv1d_opts(x1, w, b, **k1, **call)["y"]
        assert y1.shape[2] == ref.shape[1], (what, i, y1.shape)
        np.testing.assert_array_equal(y[i, :, :ref.shape[1]], y1[0], err_msg=f"{what}: utterance {i} alone")


# ---- noise_convs.0: strided, ragged, fused statistics ------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,form", [(0, "F32"), (1, "LDS"), (2, "LDS"), (3, "LDS")])
@pytest.mark.parametrize("name", ["noise0", "noise0_40"])
def test_strided_noise_conv_ragged_with_fused_statistics(name, mode, form):
    """22 -> 256 and 22 -> 40 (a partial row tile), k = 12, stride 6, pad 3, maps (120, 1) -> (20, 0), units (7, 1, 4): 140 / 20 / 80
    output columns, so the longest row crosses the 128-column seam (p0 = t0 * stride - pad with t0 > 0) and the shortest is a
    fraction of a tile.  The last column of an utterance reads two taps past its own input: NaN there, zero padding by the
    definition.  A strided conv runs on the LDS form without prefetch (f32 kernel: mode 0), whatever the mode asks for.  Once
    with the raw partial sums and once through the finalize pass: both over the row's own columns."""
    from kokorox_amd import hip_koko as hk
    x, w, b, kw = R.make_case(name)
    refs = R.case_reference(x, w, b, kw)
    gb = (0.3 * np.random.default_rng(5).standard_normal((3, 2 * w.shape[0]))).astype(np.float32)
    r = hk.conv1d_opts(x, w, b, mode=mode, want_stats=True, **kw)
    plan = r["plan"]
    assert plan["form"] == form and plan["pf"] == 0 and plan["stat_cols"] > 0, plan
    err = R.check_owned(r["y"], refs, BOUND)
    R.check_untouched(r["y"], refs)
    fs = R.check_sums(r["stats"], r["y"], refs, plan["stat_cols"])
    rn = hk.conv1d_opts(x, w, b, mode=mode, want_norm=gb, **kw)
    assert rn["plan"] == plan
    np.testing.assert_array_equal(rn["y"], r["y"])
    fp = R.check_planes(rn["norm"], gb, rn["y"], refs, plan["stat_cols"])
    print(f"{name} mode {mode} {plan['form']} bn={plan['bn']} stat_cols={plan['stat_cols']}: max err {err:.2e} = {err / BOUND:.3f} of the "
          f"bound; sums at {fs:.3f}, scale at {fp:.3f} of the slot envelope")
    _each_alone(hk, x, w, b, kw, r["y"], refs, name, mode=mode, want_stats=True)


# ---- F0_conv / N_conv: strided, between row slices of taller tensors -----------------------------------------------------------------

@pytest.mark.parametrize("mode,form", [(0, "F32"), (1, "LDS"), (2, "LDS"), (3, "LDS")])
def test_strided_one_channel_conv_between_row_slices(mode, form):
    """1 -> 1, k = 3, stride 2, pad 1, maps (2, 0) -> (1, 0), units (130, 1, 65), input and output each three rows below the top of a
    tensor eight rows taller (x_bs != Cin x_ld, y_bs != Cout y_ld; the foreign input rows NaN, the foreign output rows checked by
    the hook).  The same bits as on tensors of its own."""
    from kokorox_amd import hip_koko as hk
    x, w, b, kw = R.make_case("f0")
    assert kw["view"]
    refs = R.case_reference(x, w, b, kw)
    r = hk.conv1d_opts(x, w, b, mode=mode, **kw)
    assert r["plan"]["form"] == form, r["plan"]
    err = R.check_owned(r["y"], refs, BOUND)
    R.check_untouched(r["y"], refs)
    print(f"f0 mode {mode} {r['plan']['form']} bn={r['plan']['bn']} under a view: max err {err:.2e} = {err / BOUND:.3f} of the bound")
    np.testing.assert_array_equal(hk.conv1d_opts(x, w, b, mode=mode, **dict(kw, view=False))["y"], r["y"])
    _each_alone(hk, x, w, b, kw, r["y"], refs, "f0", mode=mode)


# ---- ups.0 / ups.1: polyphase, ragged, residual, offset and reflection ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["ups0", "ups1"])
def test_polyphase_upsamplers_ragged_on_padded_rows(name):
    """ups.0 (64 -> 26, s = 10, maps (2, 0) -> (20, 0), units (400, 1, 65)) and ups.1 (48 -> 52, s = 6, maps (20, 0) -> (120, 0), units
    (40, 1, 7), output from column 1 of a tensor 120 f + 1 columns wide, column 0 the reflection), leaky 0.1, the residual added in
    the scatter store.  Per utterance here: the interior / edge decision of the scatter epilogue, ncols = Lin + 1, the flat tile
    list over the input map with one extra column, the tile prefix of a map with mul != 1.  Through the dense grid, the flat tile
    list, the pre-split image and under a view: hook modes 1 and 3, with and without the image, are bit for bit mode 2 (as
    test_polyphase_with_residual_offset_and_reflection holds on dense batches), every utterance is bit for bit its own B = 1 call,
    every row is within 2e-5 of float64 (column 0 of the reflected case and the last s columns of each utterance with it)."""
    from kokorox_amd import hip_koko as hk
    x, w, b, kw = R.make_case(name)
    refs = R.case_reference(x, w, b, kw)
    lin, _ = R.own_lengths(kw["lens"], kw["len_in"], kw["len_out"])
    forms = {0: "F32", 2: "LDS", 1: "DA", 3: "DA"}

    def run(mode, **call):
        r = hk.conv1d_opts(x, w, b, mode=mode, **dict(kw, **call))
        plan = r["plan"]
        assert plan["form"] == ("DA_PRE" if call.get("pre") else forms[mode]), (mode, call, plan)
        # an interior block of the scatter epilogue exists beside the first, the last and the partly valid ones
        assert int(lin.max()) + 1 >= 3 * plan["bn"], plan
        assert (plan["flat_bn"] > 0) == (bool(call.get("flat")) and mode in (1, 3)), (mode, call, plan)
        err = R.check_owned(r["y"], refs, BOUND)
        R.check_untouched(r["y"], refs)
        print(f"{name} mode {mode} {plan['form']} bn={plan['bn']} flat_bn={plan['flat_bn']} {call}: max err {err:.2e} = "
              f"{err / BOUND:.3f} of the bound")
        return r["y"]

    y2 = run(2)
    np.testing.assert_array_equal(run(2, view=True), y2)
    _each_alone(hk, x, w, b, kw, y2, refs, f"{name} mode 2", mode=2)
    for mode in (1, 3):
        for pre in (False, True):
            for call in (dict(), dict(flat=True), dict(view=True), dict(flat=True, view=True)):
                np.testing.assert_array_equal(run(mode, pre=pre, **call), y2, err_msg=f"mode {mode} pre={pre} {call}")
            _each_alone(hk, x, w, b, kw, y2, refs, f"{name} mode {mode} pre={pre}", mode=mode, pre=pre)
    y0 = run(0)
    np.testing.assert_array_equal(run(0, view=True), y0)
    _each_alone(hk, x, w, b, kw, y0, refs, f"{name} mode 0", mode=0)


# ---- the 120 f + 1 axis at stride 1 -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,form", [(1, "DA"), (3, "DA_W2"), (1 | F8, "DA_F8")])
def test_resblock_conv_on_the_120f_plus_1_axis(mode, form):
    """A stage-1 resblock conv: 7 taps, 128 -> 128, dilation 3, snake behind an AdaIN affine, residual, fused statistics, on the maps
    (120, 1) -> (120, 1) (units (5, 1, 2): 601 / 121 / 241 columns -- the hooks' own ragged calls only build {lens, 1, 0}).  The
    flat tile list and the dense grid give the same bits.  f16f8: the bounds of test_f16f8_form_against_float64 (4e-4 absolute,
    3e-5 rms, in units of max(1, output rms)).  Forms: a dilated 7-tap conv is not a 16x16x32 shape in f16x3 (conv_plan.hip,
    s16_shape): the 128-column direct-A tile on this small grid (mode 1), the unrolled 2 x 2 form on 256 columns (mode 3)."""
    from kokorox_amd import hip_koko as hk
    x, w, b, kw = R.make_case("res121")
    refs = R.case_reference(x, w, b, kw)
    r = hk.conv1d_opts(x, w, b, mode=mode, flat=True, want_stats=True, **kw)
    plan = r["plan"]
    assert plan["form"] == form and plan["flat_bn"] == plan["bn"], plan
    if mode & F8:
        conv = R.case_reference(x, w, b, {k_: v for k_, v in kw.items() if k_ != "resid"})
        scale = max(1.0, float(np.sqrt((np.concatenate([c.ravel() for c in conv]) ** 2).mean())))
        err = R.check_owned(r["y"], refs, 4e-4 * scale)
        d = np.concatenate([(r["y"][i, :, :ref.shape[1]] - ref).ravel() for i, ref in enumerate(refs)])
        rms = float(np.sqrt((d ** 2).mean()))
        print(f"res121 mode {mode:#x} {form}: max err {err:.2e} = {err / (4e-4 * scale):.3f} of its bound, rms {rms:.2e} = "
              f"{rms / (3e-5 * scale):.3f} of its bound")
        assert rms < 3e-5 * scale
    else:
        err = R.check_owned(r["y"], refs, BOUND)
        print(f"res121 mode {mode} {form} bn={plan['bn']}: max err {err:.2e} = {err / BOUND:.3f} of the bound")
    R.check_untouched(r["y"], refs)
    fs = R.check_sums(r["stats"], r["y"], refs, plan["stat_cols"])
    print(f"   sums at {fs:.3f} of the slot envelope ({plan['stat_cols']}-column slots)")
    r0 = hk.conv1d_opts(x, w, b, mode=mode, flat=False, want_stats=True, **kw)
    assert r0["plan"]["form"] == form and r0["plan"]["flat_bn"] == 0, r0["plan"]
    np.testing.assert_array_equal(r0["y"], r["y"])
    np.testing.assert_array_equal(r0["stats"], r["stats"])


@pytest.mark.parametrize("mode,form", [(0, "F32"), (1, "LDS"), (2, "LDS"), (3, "LDS")])
def test_conv_post_on_the_120f_plus_1_axis(mode, form):
    """conv_post: 128 -> 22 (the 32-row tile, which only the LDS form and the f32 kernel have), 7 taps, leaky 0.01, on the same maps;
    offered the flat tile list as the model offers it, which this form does not take."""
    from kokorox_amd import hip_koko as hk
    x, w, b, kw = R.make_case("post121")
    refs = R.case_reference(x, w, b, kw)
    ys = []
    for flat in (True, False):
        r = hk.conv1d_opts(x, w, b, mode=mode, flat=flat, **kw)
        assert r["plan"]["form"] == form and r["plan"]["bm"] == 32, r["plan"]
        err = R.check_owned(r["y"], refs, BOUND)
        R.check_untouched(r["y"], refs)
        print(f"post121 mode {mode} {form} bn={r['plan']['bn']} flat_bn={r['plan']['flat_bn']}: max err {err:.2e} = {err / BOUND:.3f} of the bound")
        ys.append(r["y"])
    np.testing.assert_array_equal(ys[0], ys[1])


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def _refused(hk, match, *args, **kw):
    with pytest.raises(hk.KokoroxHipError, match=match) as e:
        hk.conv1d_opts(*args, **kw)
    assert e.value.code == hk.KX_ERR_INVALID


def test_contradictory_maps_and_options_are_refused_before_any_launch():
    """KX_ERR_INVALID for an output map that contradicts the conv's own output count, units that overrun L, an output offset
    without an up-scattering conv; and a strided conv is refused a merged, an in_up2 or a time-major launch (no launch of the
    model is one, and no kernel form is tested for it)."""
    from kokorox_amd import hip_koko as hk
    x, w, b, kw = R.make_case("noise0")
    _refused(hk, "contradicts", x, w, b, **dict(kw, len_out=(20, 1)))
    _refused(hk, "contradicts", x, w, b, **dict(kw, len_out=(19, 0)))
    _refused(hk, "overrun", np.ascontiguousarray(x[:, :, :800]), w, b, **kw)
    _refused(hk, "output offset", x, w, b, **dict(kw, up_off=True))
    xu, wu, bu, ku = R.make_case("ups1")
    _refused(hk, "contradicts", xu, wu, bu, **dict(ku, len_out=(120, 1)))
    _refused(hk, "overrun", np.ascontiguousarray(xu[:, :, :799]), wu, bu, **dict(ku, resid=None))
    for opt in ("merged", "in_up2", "tmajor"):
        _refused(hk, "strided conv", x, w, b, stride=6, pad=3, **{opt: True})
