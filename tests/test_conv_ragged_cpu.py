"""CPU: the references and checks of oracle/conv_ragged_ref.py that tests/test_gpu_conv_ragged.py holds the kernels to.  The
references are held to torch on dense inputs; the float32 stand-in of hip_koko.conv1d_opts passes every check on every case, and
each way a kernel could be subtly wrong on these launches, built into the stand-in, fails the check named for it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_ragged_ref as R

BOUND = 2e-5  # what the GPU file asserts of the f16x3 and f32 forms


def _run(name, fault=None, **over):
    x, w, b, kw = R.make_case(name)
    kw.update(over)
    r = R.standin_conv1d_opts(x, w, b, fault=fault, **kw)
    return r, R.case_reference(x, w, b, kw), kw


@pytest.mark.parametrize("name", ["noise0", "f0", "ups0", "ups1", "res121", "post121"])
def test_references_equal_torch_on_dense_inputs(name):
    """With every utterance at the full length, the per-utterance reference is one batched torch call on the whole tensor."""
    x, w, b, kw = R.make_case(name)
    kw["lens"] = np.full_like(kw["lens"], kw["lens"].max())
    refs = R.case_reference(x, w, b, kw)
    xt = torch.from_numpy(x).double()
    if "norm" in kw:
        n = torch.from_numpy(kw["norm"]).double()
        xt = (xt - n[0][:, :, None]) * n[1][:, :, None] + n[2][:, :, None]
    if kw["act"] == 2:
        a = torch.from_numpy(kw["alpha"]).double()[None, :, None]
        xt = xt + torch.sin(a * xt) ** 2 / a
    elif kw["act"] == 1:
        xt = F.leaky_relu(xt, kw["slope"])
    wt, bt = torch.from_numpy(w).double(), torch.from_numpy(b).double()
    if kw["up_stride"]:
        s = kw["up_stride"]
        y = F.conv_transpose1d(xt, wt, bt, stride=s, padding=s // 2)
        assert y.shape[2] == s * x.shape[2]
        if kw["up_off"]:
            y = F.pad(y, (1, 0), mode="reflect")
    else:
        y = F.conv1d(xt, wt, bt, stride=kw["stride"], padding=kw["pad"], dilation=kw["dil"])
    if "resid" in kw:
        y = y + torch.from_numpy(kw["resid"]).double()
    y = y.numpy()
    lin, lout = R.own_lengths(kw["lens"], kw["len_in"], kw["len_out"])
    assert np.array_equal(lout, R.conv_out_len(lin, w.shape[2], kw["stride"], kw["pad"], kw["dil"], kw["up_stride"]))
    for i, r in enumerate(refs):
        assert r.shape == y[i].shape
        assert np.abs(r - y[i]).max() < 1e-13
    sums = R.row_sums(refs)
    np.testing.assert_allclose(sums[:, :, 0], y.sum(axis=2), rtol=1e-12, atol=1e-10)
    np.testing.assert_allclose(sums[:, :, 1], (y * y).sum(axis=2), rtol=1e-12)


def test_the_models_length_maps_agree_with_the_conv_formulas():
    """The four maps of Model::back_half, for 1 .. 50 frames."""
    f = np.arange(1, 51)
    assert np.array_equal(R.conv_out_len(120 * f + 1, 12, 6, 3), 20 * f)      # noise_convs.0
    assert np.array_equal(R.conv_out_len(2 * f, 3, 2, 1), f)                  # F0_conv / N_conv
    assert np.array_equal(R.conv_out_len(2 * f, 20, up_stride=10), 20 * f)    # ups.0
    assert np.array_equal(R.conv_out_len(20 * f, 12, up_stride=6), 120 * f)   # ups.1
    assert np.array_equal(R.conv_out_len(120 * f + 1, 7, 1, 9, 3), 120 * f + 1)


@pytest.mark.parametrize("name", list(R.CASES))
def test_stand_in_passes_every_check(name):
    gb = None
    if not R.CASES[name].get("up_stride"):
        gb = (0.3 * np.random.default_rng(1).standard_normal((3, 2 * R.CASES[name]["Cout"]))).astype(np.float32)
    r, refs, kw = _run(name, want_stats=gb is not None, want_norm=gb)
    err = R.check_owned(r["y"], refs, BOUND)
    print(f"{name}: float32 stand-in max err {err:.2e}")
    R.check_untouched(r["y"], refs)
    if gb is not None:
        R.check_sums(r["stats"], r["y"], refs, 64)
        R.check_planes(r["norm"], gb, r["y"], refs, 64)
    for view in (False, True):  # and both ways round under a view
        rv, _, _ = _run(name, view=view)
        np.testing.assert_array_equal(rv["y"], r["y"])


def _fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def test_neighbours_data_instead_of_zero_padding_fails_the_value_check():
    for name in ("noise0", "ups0", "ups1", "res121"):
        r, refs, _ = _run(name, fault="neighbour")
        _fails(R.check_owned, r["y"], refs, BOUND)
        R.check_untouched(r["y"], refs)
    # the strided conv's last column alone is wrong, by the two taps past the utterance's end
    r, refs, _ = _run("noise0", fault="neighbour")
    bad = [np.flatnonzero((np.abs(r["y"][i, :, :ref.shape[1]] - ref) >= BOUND).any(axis=0)) for i, ref in enumerate(refs)]
    assert list(bad[1]) == [19] and list(bad[2]) == [79] and len(bad[0]) == 0


def test_longest_rows_output_length_fails_the_untouched_check():
    for name in ("noise0", "f0", "ups0", "ups1", "post121"):
        r, refs, _ = _run(name, fault="lout_max")
        _fails(R.check_untouched, r["y"], refs)
        R.check_owned(r["y"], refs, BOUND)  # (its own columns are right: only the sentinel check sees it)


def test_reflection_from_column_zero_fails_the_value_check():
    r, refs, _ = _run("ups1", fault="reflect_up0")
    _fails(R.check_owned, r["y"], refs, BOUND)
    assert all(np.abs(r["y"][i, :, 1:ref.shape[1]] - ref[:, 1:]).max() < BOUND for i, ref in enumerate(refs))  # column 0 alone


def test_residual_without_the_offset_fails_the_value_check():
    r, refs, _ = _run("ups1", fault="resid_no_off")
    _fails(R.check_owned, r["y"], refs, BOUND)


def test_window_origin_without_pad_at_the_second_tile_fails_the_value_check():
    r, refs, _ = _run("noise0", fault="origin_second_tile")
    _fails(R.check_owned, r["y"], refs, BOUND)
    R.check_owned(r["y"][:, :, :128], [ref[:, :128] for ref in refs], BOUND)  # nothing before the seam, nothing in the shorter rows
    R.check_untouched(r["y"], refs)


def test_statistics_over_the_launchs_columns_fail_the_statistics_checks():
    gb = (0.3 * np.random.default_rng(2).standard_normal((3, 512))).astype(np.float32)
    r, refs, _ = _run("noise0", fault="stats_lmax", want_stats=True, want_norm=gb)
    R.check_owned(r["y"], refs, BOUND)
    _fails(R.check_sums, r["stats"], r["y"], refs, 64)
    _fails(R.check_planes, r["norm"], gb, r["y"], refs, 64)


def test_batch_offset_from_channels_times_row_stride_fails_under_a_view():
    with pytest.raises(R.StandInStateError):
        _run("f0", fault="view_bs")
    x, w, b, kw = R.make_case("ups1", dict(view=True))
    with pytest.raises(R.StandInStateError):
        R.standin_conv1d_opts(x, w, b, fault="view_bs", **kw)
    r, refs, _ = _run("f0", fault="view_bs", view=False)  # without a view C * ld is the batch stride
    R.check_owned(r["y"], refs, BOUND)
