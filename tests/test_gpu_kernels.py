"""GPU: each hand-written kernel, alone, through the C ABI test hooks, against torch CPU in float64.

Both contraction modes are covered: f32 MFMA (a k-ordered fmaf chain, error ~1e-7 * sum|a*b|) and the
f16x3 split MFMA (three f16 MFMAs per step on hi/lo halves, ~2^-22 per product).  2e-5 absolute on
O(1) outputs with K up to 3270 leaves margin for both.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

CONV_CASES = [
    # B, Cin, Cout, L, k, stride, pad, dil
    (2, 16, 32, 70, 3, 1, 1, 1),
    (1, 24, 130, 300, 7, 1, 9, 3),        # Cin/Cout not multiples of the tile, dilation 3
    (2, 128, 128, 517, 11, 1, 25, 5),     # generator stage-1 shape, dilation 5
    (1, 256, 256, 261, 7, 1, 3, 1),       # generator stage-0 shape
    (1, 22, 256, 601, 12, 6, 3, 1),       # noise_convs[0]: stride 6
    (2, 1, 1, 40, 3, 2, 1, 1),            # F0_conv: 1 channel, stride 2
    (1, 640, 50, 33, 1, 1, 0, 1),         # duration projection as k=1 conv
    (1, 1090, 64, 45, 3, 1, 1, 1),        # decoder concat width
    (1, 128, 22, 700, 7, 1, 3, 1),        # conv_post (BM=32 tile)
    (3, 8, 8, 1, 1, 1, 0, 1),             # single column
    (1, 5, 7, 130, 5, 1, 2, 1),           # ragged channel counts, text-encoder kernel
]


MODES = [pytest.param(0, id="f32"), pytest.param(1, id="f16x3"), pytest.param(2, id="f16x3lds"), pytest.param(3, id="f16x3da")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,Cin,Cout,L,k,s,p,d", CONV_CASES)
def test_conv1d_mfma(B, Cin, Cout, L, k, s, p, d, mode):
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(B * 1000 + Cin + L)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    y = hk.conv1d(x, w, b, stride=s, pad=p, dil=d, mode=mode)
    ref = F.conv1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                   stride=s, padding=p, dilation=d).numpy()
    assert y.shape == ref.shape
    assert np.abs(y - ref).max() < 2e-5


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act", [1, 2])
def test_conv1d_fused_adain_activation(act, mode):
    """AdaIN affine + leaky / snake applied while staging the input tile; zero padding comes AFTER."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(act)
    B, Cin, Cout, L, k = 2, 40, 48, 200, 7
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    norm = rng.standard_normal((3, B, Cin), dtype=np.float32)
    alpha = (rng.random(Cin, dtype=np.float32) + 0.5).astype(np.float32)
    y = hk.conv1d(x, w, None, pad=3, act=act, slope=0.2, alpha=alpha, norm=norm, mode=mode)
    n = torch.from_numpy(norm).double()
    xt = (torch.from_numpy(x).double() - n[0][:, :, None]) * n[1][:, :, None] + n[2][:, :, None]
    if act == 2:
        a = torch.from_numpy(alpha).double()[None, :, None]
        xt = xt + (1 / a) * torch.sin(a * xt) ** 2
    else:
        xt = F.leaky_relu(xt, 0.2)
    ref = F.conv1d(xt, torch.from_numpy(w).double(), padding=3).numpy()
    assert np.abs(y - ref).max() < 3e-5


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Cin,Cout,L,s", [(16, 24, 37, 10), (256, 128, 50, 6), (512, 256, 21, 10), (8, 8, 1, 6)])
def test_conv_transpose_polyphase(Cin, Cout, L, s, mode):
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(Cin + L)
    k = 2 * s
    x = rng.standard_normal((2, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cin, Cout, k), dtype=np.float32) / np.sqrt(Cin * 2)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    y = hk.conv1d(x, w, b, stride=s, pad=(k - s) // 2, transposed=True, mode=mode)
    ref = F.conv_transpose1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                             stride=s, padding=(k - s) // 2).numpy()
    assert y.shape == ref.shape
    assert np.abs(y - ref).max() < 2e-5


@pytest.mark.parametrize("L,n_in", [(19, 72), (1, 640), (130, 512)])
def test_bilstm(L, n_in):
    """(the input projection runs on the f32 MFMA kernel in this hook; its time-major store on the f16x3 kernels a forward runs it on:
    tests/test_gpu_conv_options.py, test_time_major_store_of_the_lstm_input_projection)"""
    from kokorox_amd import hip_koko as hk
    torch.manual_seed(L)
    m = torch.nn.LSTM(n_in, 256, 1, batch_first=True, bidirectional=True).double()
    x = torch.randn(2, L, n_in, dtype=torch.float64)
    with torch.no_grad():
        ref = m(x)[0].numpy()
    ps = [getattr(m, n + suf).detach().float().numpy() for suf in ("", "_reverse")
          for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    y = hk.lstm(x.float().numpy(), ps)
    assert np.abs(y - ref).max() < 1e-5


@pytest.mark.gpu
def test_bilstm_two_and_four_workgroups_and_the_streaming_fallback_give_the_same_bits():
    """Round 5: batches that leave CUs idle run the resident-weights recurrence on FOUR workgroups per (utterance, direction)
    (512 threads, all of a lane's weights in registers) instead of two, and a model whose hand-off timed out runs the streaming
    fall-back (one workgroup, most of W_hh from L2 every step).  A lane's arithmetic is the same in all three -- two rows x a K
    quarter, the same order of sums, one shared cell update -- so which one runs may depend on the batch or on the model's
    history without changing a bit: forced to each on the same input, bit for bit, and against the float64 reference."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(5)
    B, L, n_in = 3, 47, 640
    x = rng.standard_normal((B, L, n_in), dtype=np.float32)
    lstm = torch.nn.LSTM(n_in, 256, batch_first=True, bidirectional=True).double()
    ps = [getattr(lstm, n).detach().float().numpy() for n in
          ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse",
           "bias_hh_l0_reverse")]
    tlib = hk.load_test_library()
    try:
        tlib.kx_test_lstm_parts(2)
        y2 = hk.lstm(x, ps)
        tlib.kx_test_lstm_parts(4)
        y4 = hk.lstm(x, ps)
        tlib.kx_test_lstm_parts(1)
        y1 = hk.lstm(x, ps)
    finally:
        tlib.kx_test_lstm_parts(0)
    np.testing.assert_array_equal(y2, y1)
    np.testing.assert_array_equal(y2, y4)
    with torch.no_grad():
        ref = lstm(torch.from_numpy(x).double())[0].numpy()
    assert np.abs(y4 - ref).max() < 2e-5


def test_bilstm_more_pairs_than_cus():
    """The two-CU recurrence at B = 130: 520 workgroups on 256 CUs, so halves wait for partners that are dispatched
    later (blocks are dispatched in order and every poll is bounded); every utterance L steps long (ragged batches:
    tests/test_gpu_front_kernels.py); no sticky error, f64 parity."""
    from kokorox_amd import hip_koko as hk
    torch.manual_seed(130)
    B, L, n_in = 130, 11, 64
    m = torch.nn.LSTM(n_in, 256, 1, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, L, n_in, dtype=torch.float64)
    with torch.no_grad():
        ref = m(x)[0].numpy()
    ps = [getattr(m, n + suf).detach().float().numpy() for suf in ("", "_reverse")
          for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    for _ in range(3):  # (several launches in a row: a stale exchange buffer would show)
        y = hk.lstm(x.float().numpy(), ps)
        assert np.abs(y - ref).max() < 1e-5


@pytest.mark.parametrize("mode,turn", [("partition", "1"), ("whole", "1"), ("whole", "0")])
def test_two_models_run_full_size_forwards_side_by_side(blob_path, mode, turn):
    """Two models on one GPU, each running batch-32 forwards of 128-phoneme utterances from its own thread (tools/
    two_models_side_by_side.py, a process of its own: the switches are read once).  No call may fail and every result must equal
    a quiet run bit for bit, in all three arrangements:
      partition      kx_create_replicas with the device id given twice: two CU-partitioned models (round 5), each confined to
                     half of the CUs -- side by side, never competing for a CU;
      whole, turn 1  two whole-device models: their forwards take turns (Model::DeviceTurn, round 4);
      whole, turn 0  two whole-device models left to run side by side (KX_DEVICE_TURN=0): a recurrence's workgroups, which need a
                     whole CU each, can starve behind the other model's conv workgroups until its partner's bounded poll gives up
                     (round 4 measured a 1 - 2 s stall, KX_ERR_DEVICE and a fall-back whose bits differed).  Round 5: the
                     time-out is 0.2 s, the fall-back gives the same bits and the call is re-run inside the library, so the
                     caller sees neither an error nor a different bit; kx_model_status says what happened."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, KX_DEVICE_TURN=turn)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "two_models_side_by_side.py"), mode, "3"], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(d)
    assert d["ok"] and not d["errors"] and d["wrong"] == 0, d
    if turn == "1":  # (taking turns / partitioned: nothing may even have timed out)
        assert all(st[1] == 0 and st[3] == 0 for st in d["status"]), d


def test_harmonic_source_phase_is_bit_faithful(oracle):
    """The ~1e5 rad phase path must reproduce torch-CPU float32 exactly; only sin/tanh/log ulps remain."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(3)
    F2 = 120
    f0 = (rng.standard_normal((3, F2)) * 150 + 110).astype(np.float32)
    f0[2, :40] = 0.0  # an unvoiced stretch and negative values are both in range
    lw = oracle.w["decoder.generator.m_source.l_linear.weight"].numpy()
    lb = float(oracle.w["decoder.generator.m_source.l_linear.bias"][0])
    y = hk.harmonic_source(f0, lw, lb, seed=7, utt_base=5)
    for b in range(3):
        ref = oracle.source(torch.from_numpy(f0[b]), 7, 5 + b, 1.0, {}).numpy()
        assert np.abs(y[b] - ref).max() < 2e-6, b
    y0 = hk.harmonic_source(f0[:1], lw, lb, seed=7, utt_base=5, noise_off=True)
    ref0 = oracle.source(torch.from_numpy(f0[0]), 7, 5, 0.0, {}).numpy()
    assert np.abs(y0[0] - ref0).max() < 2e-6


# ---- ALBERT self-attention hook (attention_mfma_kernel) vs a float64 softmax -----------------------------------
def _attention_ref(qkv, lens):
    B, _, T = qkv.shape
    out = np.zeros((B, 768, T), dtype=np.float64)
    q64 = qkv.astype(np.float64)
    for b in range(B):
        L = int(lens[b])
        for hd in range(12):
            Q = q64[b, hd * 64:(hd + 1) * 64, :L]            # [64, L]
            K = q64[b, 768 + hd * 64:768 + (hd + 1) * 64, :L]
            V = q64[b, 1536 + hd * 64:1536 + (hd + 1) * 64, :L]
            S = (Q.T @ K) * 0.125                               # [query, key]
            S -= S.max(axis=1, keepdims=True)
            P = np.exp(S)
            P /= P.sum(axis=1, keepdims=True)
            out[b, hd * 64:(hd + 1) * 64, :L] = (P @ V.T).T
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("T,lens", [(1, [1]), (33, [33, 1, 32]), (130, [130, 97, 64, 5]), (300, [300, 257, 31]),
                                     (512, [512, 449])])
def test_attention_matches_float64_softmax(T, lens):
    from kokorox_amd import hip_koko
    rng = np.random.default_rng(1000 + T)
    B = len(lens)
    qkv = rng.standard_normal((B, 2304, T)).astype(np.float32)
    qkv[:, :1536] *= 1.5                                        # sharper softmax than unit-variance scores give
    got = hip_koko.attention(qkv, lens)
    ref = _attention_ref(qkv, lens)
    for b, L in enumerate(lens):
        err = np.abs(got[b, :, :L] - ref[b, :, :L]).max()
        assert err < 2e-5, (b, L, err)
        assert np.all(got[b, :, L:] == 0.0)                     # columns past the utterance are not written


def _sweep_cases(n, seed):
    """Random conv shapes concentrated on tile borders: columns around multiples of 128 / 256, output channels
    around the 32 / 64 / 128-row tiles, every kernel width and dilation the graph uses, with and without the fused
    AdaIN affine + leaky / snake input transform (act 2 with k = 11 and an even number of 16-channel chunks is the
    16x16x32 form of the direct-A kernel: conv_plan.hip, s16_shape)."""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n):
        k = int(rng.choice([1, 2, 3, 5, 7, 11]))
        d = int(rng.choice([1, 3, 5])) if k >= 3 else 1
        base = int(rng.choice([128, 256, 384, 512, 768]))
        L = max(1, base + int(rng.integers(-3, 4)))
        Cout = max(1, int(rng.choice([32, 64, 128, 256])) + int(rng.integers(-5, 6)))
        Cin = int(rng.choice([3, 16, 17, 48, 96, 130]))
        B = int(rng.integers(1, 4))
        pad = (k - 1) * d // 2
        act = int(rng.choice([0, 0, 1, 2]))
        cases.append((B, Cin, Cout, L, k, pad, d, act))
    # the S16 form's own borders (k = 11 snake, Cin 17..32 / 49..64 / whole chunks, rows around the 128-row tile)
    for Cin, Cout, L, d in ((24, 130, 191, 1), (32, 128, 193, 3), (56, 256, 257, 5), (128, 127, 385, 1), (96, 129, 63, 3)):
        cases.append((2, Cin, Cout, L, 11, 5 * d, d, 2))
    return cases


def _act_ref(x, act, norm, alpha, slope=0.2):
    """float64 reference of the fused input transform: AdaIN affine, then leaky / snake (x [B,Cin,L] torch f64)."""
    if act == 0:
        return x
    n = torch.from_numpy(norm).double()
    xt = (x - n[0][:, :, None]) * n[1][:, :, None] + n[2][:, :, None]
    if act == 2:
        a = torch.from_numpy(alpha).double()[None, :, None]
        return xt + (1 / a) * torch.sin(a * xt) ** 2
    return F.leaky_relu(xt, slope)


@pytest.mark.parametrize("B,Cin,Cout,L,k,p,d,act", _sweep_cases(36, seed=2024))
def test_conv1d_tile_border_sweep(B, Cin, Cout, L, k, p, d, act):
    """Both contraction modes must agree with float64 at every tile border (full / edge epilogue forms, the
    128- and 256-column tiles, the small-grid 4x1 tiles, virtual taps for k = 1, the 16x16x32 form's 128- and
    192-column tiles through modes 1 and 3)."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(B * 7919 + Cin * 131 + Cout * 17 + L + k)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    norm = rng.standard_normal((3, B, Cin), dtype=np.float32)
    norm[1] = 1.0 + 0.2 * norm[1]
    alpha = (rng.random(Cin, dtype=np.float32) + 0.5).astype(np.float32)
    kw = dict(act=act, slope=0.2, alpha=alpha, norm=norm) if act else dict()
    ref = F.conv1d(_act_ref(torch.from_numpy(x).double(), act, norm, alpha), torch.from_numpy(w).double(),
                   torch.from_numpy(b).double(), padding=p, dilation=d).numpy()
    tol = 3e-5 if act else 2e-5
    for mode in (1, 0, 2, 3):
        y = hk.conv1d(x, w, b, pad=p, dil=d, mode=mode, **kw)
        assert y.shape == ref.shape
        assert np.abs(y - ref).max() < tol, (mode, np.abs(y - ref).max())


def _s16_border_cases():
    """The 16x16x32 form's predicate (conv_plan.hip, s16_shape: snake, 11 taps, (k-1) dil <= 64, an even
    number >= 2 of 16-channel chunks, 128-row weight tiles) admits partial chunks (Cin 17..32, 49..64), Cout != n 128 and
    any length: every (Cin, Cout) pair of the lists below meets every length once over the three dilations."""
    cins, couts, lens, dils = [24, 32, 56, 128], [22, 128, 130, 256], [1, 63, 65, 191, 193, 257, 517], [1, 3, 5]
    cases, i = [], 0
    for ci in cins:
        for co in couts:
            for L in lens:
                cases.append((ci, co, L, dils[i % 3], bool(i & 1)))
                i += 1
    return cases


@pytest.mark.parametrize("Cin,Cout,L,d,pad_ld", _s16_border_cases())
def test_s16_form_borders_against_float64(Cin, Cout, L, d, pad_ld):
    """act = 2, k = 11 through the full hook (fused transform + every epilogue form the generator uses + ragged lengths +
    the model's padded rows), against torch float64, in hook mode 1 (small grid: the form's 128-column tile) and mode 3
    (its 192-column tile).  Cout = 22 takes a 32-row weight tile, i.e. NOT this form: it rides along as the control."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(Cin * 1000003 + Cout * 1009 + L * 7 + d)
    B, k = 3, 11
    p = 5 * d
    lens = np.array([L, max(1, (2 * L) // 3), max(1, L // 3)], dtype=np.int32)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    norm = rng.standard_normal((3, B, Cin), dtype=np.float32)
    norm[1] = 1.0 + 0.2 * norm[1]
    alpha = (rng.random(Cin, dtype=np.float32) + 0.5).astype(np.float32)
    res = rng.standard_normal((B, Cout, L), dtype=np.float32)
    run = rng.standard_normal((B, Cout, L), dtype=np.float32)
    xt = _act_ref(torch.from_numpy(x).double(), 2, norm, alpha)
    conv = np.zeros((B, Cout, L))
    for i in range(B):  # each utterance is convolved alone over its own length (zero padding at ITS end)
        n = int(lens[i])
        conv[i, :, :n] = F.conv1d(xt[i:i + 1, :, :n], torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                                  padding=p, dilation=d).numpy()[0]
    valid = np.arange(L)[None, None, :] < lens[:, None, None]
    # (every second case through the flat tile list the model uses for batches, the others through the dense grid)
    kw = dict(pad=p, dil=d, act=2, alpha=alpha, norm=norm, lens=lens, pad_ld=pad_ld, flat=(L % 4 == 1))
    mul = float(np.float32(0.70710678))
    for mode in (1, 3):
        # (1) plain store; columns past an utterance's length are not written
        y = hk.conv1d_full(x, w, b, mode=mode, **kw)
        assert np.abs(np.where(valid, y - conv, 0.0)).max() < 3e-5, mode
        assert np.all(np.where(valid, 0.0, y) == 0.0), mode
        # (2) residual + fused statistics (64-column slots in this form), over each utterance's own columns
        y, st = hk.conv1d_full(x, w, b, resid=res, want_stats=True, mode=mode, **kw)
        ref = np.where(valid, conv + res, 0.0)
        assert np.abs(np.where(valid, y - ref, 0.0)).max() < 3e-5, mode
        y64 = np.where(valid, y.astype(np.float64), 0.0)
        assert np.abs(st[..., 0] - y64.sum(axis=2)).max() < 2e-3 * max(1.0, np.sqrt(L) / 10), mode
        assert np.abs(st[..., 1] - (y64 * y64).sum(axis=2)).max() < 1e-5 * max(1.0, (y64 * y64).sum(axis=2).max()), mode
        # (3) residual + accumulate into the running sum, mean over three (the AdaINResBlock1 tail)
        y = hk.conv1d_full(x, w, b, resid=res, y_init=run, out_div=3.0, mode=mode, **kw)
        ref = (conv + res + run) / 3.0
        assert np.abs(np.where(valid, y - ref, 0.0)).max() < 3e-5, mode
        assert np.array_equal(np.where(valid, 0.0, y), np.where(valid, 0.0, run)), mode  # the rest of the running sum stays
        # (4) output scale + statistics
        y, st = hk.conv1d_full(x, w, b, out_mul=mul, want_stats=True, mode=mode, **kw)
        assert np.abs(np.where(valid, y - conv * mul, 0.0)).max() < 3e-5, mode
        y64 = np.where(valid, y.astype(np.float64), 0.0)
        assert np.abs(st[..., 0] - y64.sum(axis=2)).max() < 2e-3 * max(1.0, np.sqrt(L) / 10), mode


@pytest.mark.parametrize("k,d,act,C,L", [(11, 3, 2, 128, 20000), (11, 1, 2, 256, 6000), (7, 5, 2, 128, 20000), (3, 1, 2, 256, 6000),
                                          (3, 1, 1, 1024, 900), (5, 1, 0, 128, 9000), (11, 1, 2, 128, 700)])
def test_flat_tile_list_gives_the_same_bits_as_the_dense_grid(k, d, act, C, L):
    """A ragged batch through the flat list of live tiles (ConvArgs::tile_prefix: what Model::conv hands the direct-A kernels
    when B > 1) against the (longest length) x B grid with early-exit workgroups: same bits in the stored values and in
    the fused statistics, on chip-filling and on small grids, for every unrolled form (S16, W2, leaky k = 3) and the
    run-time form."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(k * 31 + C)
    B = 8
    p = d * (k - 1) // 2
    lens = np.array([L, L // 3, (2 * L) // 3, 1, L - 1, L // 2 + 17, 129, (3 * L) // 4], dtype=np.int32)
    x = rng.standard_normal((B, C, L), dtype=np.float32)
    w = (rng.standard_normal((C, C, k), dtype=np.float32) / np.sqrt(C * k)).astype(np.float32)
    b = rng.standard_normal(C, dtype=np.float32)
    norm = rng.standard_normal((3, B, C), dtype=np.float32)
    norm[1] = 1.0 + 0.2 * norm[1]
    alpha = (rng.random(C, dtype=np.float32) + 0.5).astype(np.float32)
    res = rng.standard_normal((B, C, L), dtype=np.float32)
    kw = dict(pad=p, dil=d, act=act, slope=0.2, lens=lens, pad_ld=True)
    if act:
        kw.update(alpha=alpha, norm=norm)
    for mode in (1, 3):
        y0, s0 = hk.conv1d_full(x, w, b, resid=res, want_stats=True, mode=mode, **kw)
        y1, s1 = hk.conv1d_full(x, w, b, resid=res, want_stats=True, mode=mode, flat=True, **kw)
        np.testing.assert_array_equal(y0, y1)
        np.testing.assert_array_equal(s0, s1)
        assert np.isfinite(y1).all() and np.abs(y1).max() > 0
        run = rng.standard_normal((B, C, L), dtype=np.float32)
        z0 = hk.conv1d_full(x, w, b, resid=res, y_init=run, out_div=3.0, mode=mode, **kw)
        z1 = hk.conv1d_full(x, w, b, resid=res, y_init=run, out_div=3.0, mode=mode, flat=True, **kw)
        np.testing.assert_array_equal(z0, z1)


@pytest.mark.parametrize("k,d,act,Cin,Cout,L", [(3, 1, 1, 1090, 256, 900), (3, 1, 1, 514, 384, 422), (3, 1, 0, 40, 130, 300),
                                               (5, 3, 0, 64, 128, 1300), (2, 1, 1, 100, 128, 517)])
def test_pre_split_image_gives_the_same_bits(k, d, act, Cin, Cout, L):
    """Round 5: layers whose window many row tiles stage read a pre-split image of their input (conv_f16x3_pre.hip: the AdaIN
    affine, activation and f16 hi / lo split done once by an elementwise pass, in the LDS layout) instead of transforming the
    window in every workgroup.  Same bits as the in-kernel transform, stored values and fused statistics, on a ragged batch with
    the model's padded rows (NaN in the padding, NaN in the image wherever the pass does not write), through the flat tile list,
    on both tile widths (mode 1 with this grid: 128 columns; mode 3: 256 columns, the W2 form for k = 3) -- and against float64."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(k * 17 + Cin)
    B = 4
    p = d * (k - 1) // 2
    Lo = L + 2 * p - d * (k - 1)
    lens = np.array([L, max(1, L // 3), L - 1, 131], dtype=np.int32)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    norm = rng.standard_normal((3, B, Cin), dtype=np.float32)
    norm[1] = 1.0 + 0.2 * norm[1]
    res = rng.standard_normal((B, Cout, Lo), dtype=np.float32)
    kw = dict(pad=p, dil=d, act=act, slope=0.2, lens=lens, pad_ld=True)
    if act:
        kw.update(norm=norm)
    for mode in (1, 3):
        for flat in (False, True):
            y0, s0 = hk.conv1d_full(x, w, b, resid=res, want_stats=True, mode=mode, flat=flat, **kw)
            y1, s1 = hk.conv1d_full(x, w, b, resid=res, want_stats=True, mode=mode, flat=flat, pre=True, **kw)
            np.testing.assert_array_equal(y0, y1)
            np.testing.assert_array_equal(s0, s1)
            assert np.isfinite(y1).all() and np.abs(y1).max() > 0
    xt = _act_ref(torch.from_numpy(x).double(), act, norm, None) if act else torch.from_numpy(x).double()
    for i in range(B):
        n = int(lens[i])
        ref = F.conv1d(xt[i:i + 1, :, :n], torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=p, dilation=d).numpy()[0]
        no = n + Lo - L
        assert np.abs(y1[i, :, :no] - (ref + res[i, :, :no])).max() < 3e-5


@pytest.mark.parametrize("B,Cin,Cout,L,s,up_off", [(8, 64, 128, 2100, 6, 1), (8, 48, 256, 1300, 10, 0), (1, 32, 128, 2100, 6, 1),
                                                   (2, 32, 52, 1500, 10, 0)])
def test_polyphase_with_residual_offset_and_reflection(B, Cin, Cout, L, s, up_off):
    """The polyphase transposed convs as Generator.ups runs them -- residual added in the scatter store, the output offset and
    reflected first column of the last upsampler, row tiles that cut channels (128 / 6, 128 / 10), both tile widths (mode 1 at
    B = 1: 128 columns), with and without the pre-split input image -- bit for bit against the LDS-DMA kernel form (mode 2), and
    against float64."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(L + s)
    k = 2 * s
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cin, Cout, k), dtype=np.float32) / np.sqrt(Cin * 2)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    Lout = (L - 1) * s - 2 * ((k - s) // 2) + k
    res = rng.standard_normal((B, Cout, Lout + up_off), dtype=np.float32)
    y2 = hk.conv_transpose(x, w, b, stride=s, resid=res, up_off=up_off, mode=2)
    for mode in (1, 3):
        for pre in (False, True):
            y = hk.conv_transpose(x, w, b, stride=s, resid=res, up_off=up_off, mode=mode, pre=pre)
            np.testing.assert_array_equal(y2, y)
    ref = F.conv_transpose1d(F.leaky_relu(torch.from_numpy(x).double(), 0.1), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                             stride=s, padding=(k - s) // 2)
    if up_off:
        ref = torch.cat([ref[..., 1:2], ref], dim=-1)
    assert np.abs(y - (ref.numpy() + res)).max() < 2e-5


@pytest.mark.parametrize("Cin,Cout,L,s", [(512, 256, 50, 10), (256, 128, 300, 6), (24, 20, 37, 10)])
def test_pre_split_image_polyphase_same_bits(Cin, Cout, L, s):
    """The polyphase transposed convs (run-time-tap form, 20 / 6 row tiles per window in the model) through a pre-split image:
    same bits as the in-kernel transform (leaky 0.1, no norm: what Generator.ups reads), both tile widths, and against float64."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(Cin + L)
    k = 2 * s
    x = rng.standard_normal((3, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cin, Cout, k), dtype=np.float32) / np.sqrt(Cin * 2)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    for mode in (1, 3):
        y0 = hk.conv1d(x, w, b, stride=s, pad=(k - s) // 2, transposed=True, act=1, slope=0.1, mode=mode)
        y1 = hk.conv1d(x, w, b, stride=s, pad=(k - s) // 2, transposed=True, act=1, slope=0.1, mode=mode, pre=True)
        np.testing.assert_array_equal(y0, y1)
    ref = F.conv_transpose1d(F.leaky_relu(torch.from_numpy(x).double(), 0.1), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                             stride=s, padding=(k - s) // 2).numpy()
    assert np.abs(y1 - ref).max() < 2e-5


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,d,act,Cin,Cout,L", [(3, 1, 1, 40, 130, 300), (7, 3, 2, 48, 128, 517), (11, 5, 2, 64, 256, 700),
                                               (5, 1, 0, 130, 64, 129), (3, 5, 2, 128, 128, 1025), (7, 1, 2, 20, 22, 513)])
def test_full_hook_ragged_padded_every_mode(k, d, act, Cin, Cout, L, mode):
    """The ragged / padded-row / fused-transform + epilogue combination on the OTHER kernel forms (f32 MFMA, LDS-DMA,
    direct-A 32x32x16): what the generator's resblocks launch, against float64."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(k * 100 + L)
    B = 3
    p = d * (k - 1) // 2
    lens = np.array([max(1, L // 2), L, max(1, L - 37)], dtype=np.int32)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    norm = rng.standard_normal((3, B, Cin), dtype=np.float32)
    norm[1] = 1.0 + 0.2 * norm[1]
    alpha = (rng.random(Cin, dtype=np.float32) + 0.5).astype(np.float32)
    res = rng.standard_normal((B, Cout, L), dtype=np.float32)
    xt = _act_ref(torch.from_numpy(x).double(), act, norm, alpha)
    conv = np.zeros((B, Cout, L))
    for i in range(B):
        n = int(lens[i])
        conv[i, :, :n] = F.conv1d(xt[i:i + 1, :, :n], torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                                  padding=p, dilation=d).numpy()[0]
    valid = np.arange(L)[None, None, :] < lens[:, None, None]
    kw = dict(pad=p, dil=d, act=act, slope=0.2, lens=lens, pad_ld=True)
    if act:
        kw.update(alpha=alpha, norm=norm)
    y, st = hk.conv1d_full(x, w, b, resid=res, want_stats=True, mode=mode, **kw)
    assert np.abs(np.where(valid, y - (conv + res), 0.0)).max() < 3e-5
    assert np.all(np.where(valid, 0.0, y) == 0.0)
    y64 = np.where(valid, y.astype(np.float64), 0.0)
    assert np.abs(st[..., 0] - y64.sum(axis=2)).max() < 2e-3 * max(1.0, np.sqrt(L) / 10)
    assert np.abs(st[..., 1] - (y64 * y64).sum(axis=2)).max() < 1e-5 * max(1.0, (y64 * y64).sum(axis=2).max())


EPI_CASES = [
    # B, Cin, Cout, L, k, pad, dil
    (2, 48, 128, 700, 7, 3, 1),     # whole 128-row tile, full + edge column tiles (256-wide)
    (1, 32, 130, 300, 3, 1, 1),     # ragged rows: second row tile has 2 rows
    (3, 16, 64, 129, 5, 6, 3),      # BM = 64 tile, dilation
    (2, 128, 128, 1025, 11, 25, 5), # generator shape, 5 column tiles
    (1, 20, 22, 513, 7, 3, 1),      # BM = 32 tile (conv_post rows)
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,Cin,Cout,L,k,p,d", EPI_CASES)
def test_conv1d_epilogue_forms(B, Cin, Cout, L, k, p, d, mode):
    """Residual, residual + accumulate + divide (the AdaINResBlock1 tail: mean over the three kernels), output scale,
    and the fused InstanceNorm partial sums, each against float64."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(Cout * 31 + L)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    conv = F.conv1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                    padding=p, dilation=d).numpy()
    Lout = conv.shape[2]
    res = rng.standard_normal((B, Cout, Lout), dtype=np.float32)
    run = rng.standard_normal((B, Cout, Lout), dtype=np.float32)
    # (1) residual + fused statistics
    y, st = hk.conv1d_epilogue(x, w, b, pad=p, dil=d, resid=res, want_stats=True, mode=mode)
    ref = conv + res.astype(np.float64)
    assert np.abs(y - ref).max() < 2e-5
    y64 = y.astype(np.float64)
    assert np.abs(st[..., 0] - y64.sum(axis=2)).max() < 2e-3 * max(1.0, np.sqrt(Lout) / 10)
    assert np.abs(st[..., 1] - (y64 * y64).sum(axis=2)).max() < 1e-5 * (y64 * y64).sum(axis=2).max()
    # (2) residual + accumulate into a running sum, then the mean over 3
    y2 = hk.conv1d_epilogue(x, w, b, pad=p, dil=d, resid=res, y_init=run, out_div=3.0, mode=mode)
    ref2 = (conv + res.astype(np.float64) + run.astype(np.float64)) / 3.0
    assert np.abs(y2 - ref2).max() < 2e-5
    # (3) plain store with an output scale (the 1 / sqrt(2) of AdainResBlk1d) + statistics
    y3, st3 = hk.conv1d_epilogue(x, w, b, pad=p, dil=d, out_mul=float(np.float32(0.70710678)), want_stats=True, mode=mode)
    assert np.abs(y3 - conv * float(np.float32(0.70710678))).max() < 2e-5
    assert np.abs(st3[..., 0] - y3.astype(np.float64).sum(axis=2)).max() < 2e-3 * max(1.0, np.sqrt(Lout) / 10)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Cin,Cout,L,k,d", [(8, 128, 128, 20000, 11, 1), (4, 256, 256, 6000, 7, 3), (8, 128, 128, 12000, 3, 5)])
def test_direct_a_kernel_is_bit_identical_under_load(B, Cin, Cout, L, k, d):
    """The direct-A kernel (conv_f16x3_da.hip, mode 3) against the LDS-DMA kernel (mode 1), bit for bit, on launches large
    enough to fill the chip: its weight ring is loaded by inline asm with hand-counted waits, and a fragment used before
    it has landed only shows when memory is slow (it did: a register copy ahead of the wait, found on exactly this shape)."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(5 + k)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    alpha = (0.5 + rng.random(Cin)).astype(np.float32)
    norm = rng.standard_normal((B, 3, Cin), dtype=np.float32)
    norm[:, 1] = 1.0 + 0.1 * norm[:, 1]
    p = d * (k - 1) // 2
    for kw in (dict(), dict(act=2, alpha=alpha, norm=norm)):
        y2 = hk.conv1d(x, w, b, pad=p, dil=d, mode=2, **kw)   # LDS-DMA kernel forms only
        y1 = hk.conv1d(x, w, b, pad=p, dil=d, mode=1, **kw)   # what the model launches (direct-A on this grid)
        y3 = hk.conv1d(x, w, b, pad=p, dil=d, mode=3, **kw)   # direct-A forced
        assert np.isfinite(y3).all()
        if k == 11 and kw:
            # snake convs with 11 taps run on v_mfma_f32_16x16x32_f16 (S16 form): one instruction sums 32 products, so the
            # comparison with the 32x32x16 forms is a tolerance (measured 3 - 5e-6 on O(1) outputs); a fragment used before it
            # has landed would show as a far larger error or as a difference between two runs
            assert 0 < np.abs(y2 - y3).max() < 2e-5
            np.testing.assert_array_equal(y1, y3)
            np.testing.assert_array_equal(y3, hk.conv1d(x, w, b, pad=p, dil=d, mode=3, **kw))
            continue
        np.testing.assert_array_equal(y2, y3)
        np.testing.assert_array_equal(y2, y1)
    res = rng.standard_normal(y1.shape, dtype=np.float32)
    o2 = hk.conv1d_epilogue(x, w, b, pad=p, dil=d, resid=res, want_stats=True, mode=2)
    o3 = hk.conv1d_epilogue(x, w, b, pad=p, dil=d, resid=res, want_stats=True, mode=3)
    np.testing.assert_array_equal(o2[0], o3[0])
    np.testing.assert_allclose(o2[1], o3[1], rtol=2e-6, atol=1e-3)  # (the partial sums may be added in another order)


@pytest.mark.gpu
def test_direct_a_4x1_layout_of_the_256_column_tile_by_hook_mode_is_still_bit_identical():
    """The 256-column tile's unrolled forms default to the 2 x 2 wave layout (conv_f16x3_da_w2.hip), which the test above
    exercises; the 4 x 1 forms stay in the library (hook mode bit 0x400: the 4 x 1 layout on the 256-column tile too) as the A/B
    reference and must keep producing the same bits: mode 3 against the LDS-DMA kernel (mode 2) for 7 and 11 taps."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(3)
    for (B, C, L, k, d) in ((4, 128, 16000, 11, 3), (4, 256, 5000, 7, 1)):
        x = rng.standard_normal((B, C, L), dtype=np.float32)
        w = (rng.standard_normal((C, C, k), dtype=np.float32) / np.sqrt(C * k)).astype(np.float32)
        b = rng.standard_normal(C, dtype=np.float32)
        alpha = (0.5 + rng.random(C)).astype(np.float32)
        norm = rng.standard_normal((B, 3, C), dtype=np.float32)
        kw = dict(pad=d * (k - 1) // 2, dil=d, act=2, alpha=alpha, norm=norm)
        y2 = hk.conv1d(x, w, b, mode=2, **kw)
        # (bit 0x800, no 16x16x32 form: the 11-tap case would otherwise take it, which is not bit-identical by construction)
        y3 = hk.conv1d(x, w, b, mode=3 | 0x400 | 0x800, **kw)
        assert np.isfinite(y3).all() and np.array_equal(y2, y3), (k, float(np.abs(y2 - y3).max()))


@pytest.mark.gpu
def test_s16_form_gives_the_same_bits_on_both_of_its_tile_widths():
    """The 16x16x32 form of the 11-tap snake convs runs on a 128-column tile on small grids and on a 192-column tile on
    chip-filling ones; an utterance must come out bit-identical either way (batch invariance): the same utterance alone (98
    tiles of 256 -> small grid) and as member 2 of a batch of eight (chip-filling), against each other and, within the
    tolerance of the K = 32 summation, against the LDS form."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(16)
    B, C, L, k, d = 8, 128, 25000, 11, 3
    x = rng.standard_normal((B, C, L), dtype=np.float32)
    w = (rng.standard_normal((C, C, k), dtype=np.float32) / np.sqrt(C * k)).astype(np.float32)
    b = rng.standard_normal(C, dtype=np.float32)
    alpha = (0.5 + rng.random(C)).astype(np.float32)
    norm = rng.standard_normal((3, B, C), dtype=np.float32)  # (the hook's layout: planes of mean, scale, shift, each [B][C])
    norm[1] = 1.0 + 0.1 * norm[1]
    kw = dict(pad=d * (k - 1) // 2, dil=d, act=2, alpha=alpha)
    y_batch = hk.conv1d(x, w, b, norm=norm, mode=1, **kw)
    y_alone = hk.conv1d(x[2:3], w, b, norm=np.ascontiguousarray(norm[:, 2:3]), mode=1, **kw)
    np.testing.assert_array_equal(y_batch[2:3], y_alone)
    y_lds = hk.conv1d(x[2:3], w, b, norm=np.ascontiguousarray(norm[:, 2:3]), mode=2, **kw)
    assert 0 < np.abs(y_lds - y_alone).max() < 2e-5


F8 = 0x200  # hook mode bit: the layer carries the 8-bit cross image of its weights (f16f8, the library's default mode)


def _f8_cases():
    """The f16f8 kernels (conv_f16x3_da.hip, F8 forms of the 16x16x32 loop: snake, 3, 7 or 11 taps at any dilation with (k-1) dil <= 64,
    an even number >= 2 of 16-channel chunks, 128-row weight tiles): partial chunks, Cout != n 128, lengths around the tile borders."""
    cases, i = [], 0
    for k, dils in ((11, (1, 3, 5)), (7, (1, 3, 5)), (3, (1, 3, 5))):
        for ci, co in ((24, 128), (56, 130), (128, 128), (256, 256)):
            for L in (1, 65, 193, 517):
                cases.append((k, ci, co, L, dils[i % 3], bool(i & 1)))
                i += 1
    return cases


@pytest.mark.parametrize("k,Cin,Cout,L,d,pad_ld", _f8_cases())
def test_f16f8_form_against_float64(k, Cin, Cout, L, d, pad_ld):
    """The f16f8 kernels through the full hook (fused transform with the hardware-cosine snake, every epilogue form the generator
    uses, ragged lengths, padded rows), against torch float64, on both of their tile widths (hook mode 1: small grid, 128 columns;
    mode 3: 192 columns).  Bounds: the cross terms carry 4 significant bits each, so a product keeps ~2^-17: measured 1e-5
    relative rms per output (numpy emulation of the arithmetic: 1.04e-5), against 4e-7 of the f16x3 form."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(k * 7919 + Cin * 1000003 + Cout * 1009 + L * 7 + d)
    B = 3
    p = (k - 1) // 2 * d
    lens = np.array([L, max(1, (2 * L) // 3), max(1, L // 3)], dtype=np.int32)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, k), dtype=np.float32) / np.sqrt(Cin * k)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    norm = rng.standard_normal((3, B, Cin), dtype=np.float32)
    norm[1] = 1.0 + 0.2 * norm[1]
    alpha = (rng.random(Cin, dtype=np.float32) + 0.5).astype(np.float32)
    res = rng.standard_normal((B, Cout, L), dtype=np.float32)
    run = rng.standard_normal((B, Cout, L), dtype=np.float32)
    xt = _act_ref(torch.from_numpy(x).double(), 2, norm, alpha)
    conv = np.zeros((B, Cout, L))
    for i in range(B):
        n = int(lens[i])
        conv[i, :, :n] = F.conv1d(xt[i:i + 1, :, :n], torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                                  padding=p, dilation=d).numpy()[0]
    valid = np.arange(L)[None, None, :] < lens[:, None, None]
    scale = max(1.0, float(np.sqrt((conv[valid.repeat(Cout, 1)] ** 2).mean())))
    kw = dict(pad=p, dil=d, act=2, alpha=alpha, norm=norm, lens=lens, pad_ld=pad_ld, flat=(L % 4 == 1))
    ys = []
    for mode in (1 | F8, 3 | F8):
        y = hk.conv1d_full(x, w, b, mode=mode, **kw)
        err = np.where(valid, y - conv, 0.0)
        assert np.abs(err).max() < 4e-4 * scale, mode
        assert np.sqrt((err ** 2).sum() / valid.sum() / Cout) < 3e-5 * scale, mode
        assert np.all(np.where(valid, 0.0, y) == 0.0), mode
        ys.append(y)
        y, st = hk.conv1d_full(x, w, b, resid=res, want_stats=True, mode=mode, **kw)
        assert np.abs(np.where(valid, y - (conv + res), 0.0)).max() < 4e-4 * scale, mode
        y64 = np.where(valid, y.astype(np.float64), 0.0)
        assert np.abs(st[..., 0] - y64.sum(axis=2)).max() < 2e-3 * max(1.0, np.sqrt(L) / 10), mode
        assert np.abs(st[..., 1] - (y64 * y64).sum(axis=2)).max() < 1e-5 * max(1.0, (y64 * y64).sum(axis=2).max()), mode
        y = hk.conv1d_full(x, w, b, resid=res, y_init=run, out_div=3.0, mode=mode, **kw)
        assert np.abs(np.where(valid, y - (conv + res + run) / 3.0, 0.0)).max() < 4e-4 * scale, mode
        assert np.array_equal(np.where(valid, 0.0, y), np.where(valid, 0.0, run)), mode
    if Cout >= 128:  # (Cout = 130: the second row tile is a 32-row tile of another kernel -- identical in both modes anyway)
        np.testing.assert_array_equal(ys[0], ys[1])  # both tile widths of the form: the same bits
    # really the f16f8 arithmetic (not the f16x3 kernel by a dispatch slip): the f16x3 result differs, by about this form's error
    if Cout % 128 == 0 and L > 60:
        y3 = hk.conv1d_full(x, w, b, mode=1, **kw)
        dd = np.abs(np.where(valid, ys[0] - y3, 0.0)).max()
        assert 1e-6 * scale < dd < 4e-4 * scale


@pytest.mark.parametrize("gain,bound", [(1.0, 3e-5), (300.0, 4e-4), (3000.0, 4e-4), (1e-3, 4e-4), (1e-5, 4e-4)])
def test_f16f8_form_outside_the_e4m3_window(gain, bound):
    """The 8-bit images of the cross terms are exact to 4 bits for |v| in [2^-6, 448] (split_pair_f8).  Outside that window a product
    must degrade towards the one-f16-MFMA class (2.9e-4 relative), never below it, and never to a NaN or an infinity: activations
    300 x and 3000 x larger (the images clamp at +-448; an infinity would poison the block's sum) and 1e3 / 1e5 x smaller (the
    images go subnormal, then to zero).  Relative rms error of the conv output against float64."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(int(gain * 1000) % 9973)
    B, C, L, k, d = 2, 128, 700, 11, 3
    x = rng.standard_normal((B, C, L), dtype=np.float32)
    w = (rng.standard_normal((C, C, k), dtype=np.float32) / np.sqrt(C * k)).astype(np.float32)
    b = np.zeros(C, dtype=np.float32)
    alpha = (rng.random(C, dtype=np.float32) + 0.5).astype(np.float32) / np.float32(max(gain, 1.0))  # (keeps the snake's argument O(1))
    norm = np.zeros((3, B, C), dtype=np.float32)
    norm[1] = gain  # the AdaIN scale carries the gain: v = gain * x, then the snake
    xt = _act_ref(torch.from_numpy(x).double(), 2, norm, alpha)
    ref = F.conv1d(xt, torch.from_numpy(w).double(), None, padding=d * (k - 1) // 2, dilation=d).numpy()
    # (at 1e-5 the f16 hi / lo split itself runs out of exponent -- what tools/real_weights_report.py flags and kx_set_act_prescale
    # repairs; there the f16f8 form must not be worse than the f16x3 form by more than the one-MFMA class)
    y3 = hk.conv1d(x, w, b, norm=norm, pad=d * (k - 1) // 2, dil=d, act=2, alpha=alpha, mode=1)
    rel3 = np.sqrt(((y3 - ref) ** 2).mean()) / np.sqrt((ref ** 2).mean())
    for mode in (1 | F8, 3 | F8):
        y = hk.conv1d(x, w, b, norm=norm, pad=d * (k - 1) // 2, dil=d, act=2, alpha=alpha, mode=mode)
        assert np.isfinite(y).all(), (gain, mode)
        rel = np.sqrt(((y - ref) ** 2).mean()) / np.sqrt((ref ** 2).mean())
        print(f"gain {gain:g}, hook mode {mode:#x}: relative rms error {rel:.2e} (f16x3 form {rel3:.2e})")
        assert rel < bound + rel3, (gain, mode, rel, rel3)


@pytest.mark.parametrize("k,d,C,L", [(11, 3, 128, 25000), (7, 5, 256, 12000), (3, 1, 128, 25000)])
def test_f16f8_form_batch_invariance_and_flat_list(k, d, C, L):
    """An utterance alone (small grid: the 128-column tile) and as a member of a batch of eight (chip-filling: 192 columns) comes out
    bit-identical from the f16f8 kernels, through the dense grid and through the flat tile list of a ragged batch."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(k * 100 + d)
    B = 8
    x = rng.standard_normal((B, C, L), dtype=np.float32)
    w = (rng.standard_normal((C, C, k), dtype=np.float32) / np.sqrt(C * k)).astype(np.float32)
    b = rng.standard_normal(C, dtype=np.float32)
    alpha = (0.5 + rng.random(C)).astype(np.float32)
    norm = rng.standard_normal((3, B, C), dtype=np.float32)
    norm[1] = 1.0 + 0.1 * norm[1]
    kw = dict(pad=d * (k - 1) // 2, dil=d, act=2, alpha=alpha)
    y_batch = hk.conv1d(x, w, b, norm=norm, mode=1 | F8, **kw)
    y_alone = hk.conv1d(x[2:3], w, b, norm=np.ascontiguousarray(norm[:, 2:3]), mode=1 | F8, **kw)
    np.testing.assert_array_equal(y_batch[2:3], y_alone)
    lens = np.array([L, L // 3, (2 * L) // 3, 1, L - 1, L // 2 + 17, 129, (3 * L) // 4], dtype=np.int32)
    res = rng.standard_normal((B, C, L), dtype=np.float32)
    kw2 = dict(kw, norm=norm, lens=lens, pad_ld=True, resid=res, want_stats=True)
    y0, s0 = hk.conv1d_full(x, w, b, mode=1 | F8, **kw2)
    y1, s1 = hk.conv1d_full(x, w, b, mode=1 | F8, flat=True, **kw2)
    np.testing.assert_array_equal(y0, y1)
    np.testing.assert_array_equal(s0, s1)


@pytest.mark.gpu
def test_direct_a_run_time_tap_forms_are_bit_identical_under_load():
    """The forms of the direct-A kernel that the resblock test above does not reach, on chip-filling launches, against the
    LDS-DMA kernel: (a) a polyphase transposed conv (run-time tap count, two taps, scatter store), (b) a one-tap conv with
    fewer than three 16-channel chunks (the ring's third slot is loaded but never consumed when there are fewer than three
    steps), (c) the 128-column tile (NTT = 4) that small grids take."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(77)
    # (a) ConvTranspose1d 256 -> 128, k = 12, stride 6 (generator ups.1) on 8 x 9000 columns
    x = rng.standard_normal((8, 256, 9000), dtype=np.float32)
    wt = (rng.standard_normal((256, 128, 12), dtype=np.float32) / np.sqrt(256 * 2)).astype(np.float32)
    b = rng.standard_normal(128, dtype=np.float32)
    ya = [hk.conv1d(x, wt, b, stride=6, pad=3, transposed=True, act=1, slope=0.1, mode=m) for m in (2, 1, 3)]
    np.testing.assert_array_equal(ya[0], ya[1])
    np.testing.assert_array_equal(ya[0], ya[2])
    # (b) k = 1, 22 -> 128 channels (noise_convs.1: two chunks = two steps) on 8 x 30000 columns, and 40 -> 128 with leaky
    for cin, kw in ((22, dict()), (40, dict(act=1, slope=0.2))):
        x = rng.standard_normal((8, cin, 30000), dtype=np.float32)
        w = (rng.standard_normal((128, cin, 1), dtype=np.float32) / np.sqrt(cin)).astype(np.float32)
        yb = [hk.conv1d(x, w, b, mode=m, **kw) for m in (2, 1, 3)]
        np.testing.assert_array_equal(yb[0], yb[1])
        np.testing.assert_array_equal(yb[0], yb[2])
    # (c) 128-column tiles: a grid under 256 workgroups takes NTT = 4 in mode 1 (B = 1, 128 -> 128, k = 7 on 25000 columns
    # = 98 tiles of 256), several launches back to back
    x = rng.standard_normal((1, 128, 25000), dtype=np.float32)
    w = (rng.standard_normal((128, 128, 7), dtype=np.float32) / np.sqrt(128 * 7)).astype(np.float32)
    alpha = (0.5 + rng.random(128)).astype(np.float32)
    norm = rng.standard_normal((1, 3, 128), dtype=np.float32)
    y2 = hk.conv1d(x, w, b, pad=9, dil=3, act=2, alpha=alpha, norm=norm, mode=2)
    for _ in range(3):
        y1 = hk.conv1d(x, w, b, pad=9, dil=3, act=2, alpha=alpha, norm=norm, mode=1)
        np.testing.assert_array_equal(y2, y1)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Cin,Cout,L", [(4, 768, 2048, 2100), (8, 640, 2048, 130), (3, 1090, 1024, 845), (2, 50, 256, 300),
                                          # small grids (fewer 128 x 128 tiles than CUs): the narrow 128 x 32 form without LDS
                                          (1, 768, 2304, 128), (1, 2048, 768, 100), (2, 640, 512, 70), (1, 128, 768, 33),
                                          (1, 1090, 512, 90)])  # (a partial chunk: stays on the 128 x 128 form)
def test_direct_a_gemm_is_bit_identical_to_virtual_tap_form(B, Cin, Cout, L):
    """k = 1 GEMMs: conv_f16x3_dag.hip (the default: its 128 x 128 form on chip-filling grids, its narrow form on small ones)
    against the virtual-tap LDS-DMA form (test-hook mode 2 keeps it), bit for bit, incl. channel counts that leave a partial
    16-channel chunk and a partial three-chunk super-chunk; and against f64."""
    from kokorox_amd import hip_koko as hk
    rng = np.random.default_rng(Cin)
    x = rng.standard_normal((B, Cin, L), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, 1), dtype=np.float32) / np.sqrt(Cin)).astype(np.float32)
    b = rng.standard_normal(Cout, dtype=np.float32)
    for kw, act in ((dict(), lambda v: v), (dict(act=1, slope=0.2), lambda v: np.where(v > 0, v, 0.2 * v))):
        y1 = hk.conv1d(x, w, b, mode=1, **kw)
        y2 = hk.conv1d(x, w, b, mode=2, **kw)
        np.testing.assert_array_equal(y1, y2)
        ref = np.einsum("oc,bcl->bol", w[:, :, 0].astype(np.float64), act(x.astype(np.float64))) + b[None, :, None]
        assert np.abs(y1 - ref).max() < 2e-5
