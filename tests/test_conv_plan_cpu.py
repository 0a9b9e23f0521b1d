"""The launch plan of the convs (kokorox_amd/csrc/conv_plan.hip), on the host: no GPU.

One pure function decides each conv launch's kernel form, tile, statistics slots, flat tile list and pre-split input.  An
utterance's bits are decided by the MFMA family its layers run on, by whether a layer's input goes through a pre-split image and
by the width of the fused statistics slots; none of these may follow the batch size or the lengths, which only pick among forms
that give the same bits.  Checked here over the conv families of the graph, every precision mode and batches of 1, 8 and 64."""
import itertools

import pytest

from kokorox_amd import hip_koko as hk

ACT_NONE, ACT_LEAKY, ACT_SNAKE = 0, 1, 2
ST_NORMAL, ST_TMAJOR, ST_UPSCATTER = 0, 1, 2
MODES = {"f32": 0, "f16x3": 1, "f16": 4, "bf16": 5, "f16f8": 6}
CUS = 256


def _chunks(cin):
    return (cin + 15) // 16


def _bm(rows):
    return 128 if rows >= 128 else (64 if rows > 32 else 32)


def _layer(rows, cin, k, lengths, dil=1, stride=1, act=ACT_NONE, norm=0, stats=0, store=ST_NORMAL, token_axis=False, p1=False, epi=0,
           in_up2=0):
    return dict(rows=rows, cin=cin, K=k, dil=dil, stride=stride, act=act, norm=norm, stats=stats, store=store, lengths=lengths,
                token_axis=token_axis, p1=p1, epi=epi, in_up2=in_up2)


def _families():
    """name -> layer: the conv families of the graph (lengths: the columns of a launch, shortest to longest utterance)"""
    fam = {
        # k = 1 GEMMs on the token axis (ALBERT, projections; the columns of a batch may be merged) and on the frame axis
        "albert_qkv": _layer(2304, 768, 1, (9, 64, 510), token_axis=True),
        "albert_ffn_gelu": _layer(3072, 768, 1, (9, 64, 510), token_axis=True, epi=1),
        "lstm_input_frames": _layer(2048, 640, 1, (40, 700, 2600), store=ST_TMAJOR),
        "proj_frames": _layer(512, 512, 1, (40, 700, 2600), act=ACT_LEAKY),
        "proj_64_rows": _layer(64, 514, 1, (40, 700, 2600)),
        # the leaky 3-tap predictor convs (AdaIN input, statistics of the output fused) and the 1024-row decoder convs
        "predictor_512": _layer(512, 512, 3, (80, 1400, 5200), act=ACT_LEAKY, norm=1, stats=1),
        "predictor_256": _layer(256, 512, 3, (80, 1400, 5200), act=ACT_LEAKY, norm=1, stats=1),
        "decoder_1024": _layer(1024, 1090, 3, (40, 700, 2600), act=ACT_LEAKY, norm=1, stats=1, p1=True),
        "decoder_1024_up2": _layer(1024, 1090, 3, (80, 1400, 5200), act=ACT_LEAKY, norm=1, stats=1, p1=True, in_up2=1),
        # the polyphase upsamplers (2 taps, scatter store: the columns are the input length + 1)
        "ups_10x": _layer(10 * 256, 512, 2, (81, 1401, 5201), act=ACT_LEAKY, store=ST_UPSCATTER, p1=True),
        "ups_6x": _layer(6 * 128, 256, 2, (801, 14001, 52001), act=ACT_LEAKY, store=ST_UPSCATTER, p1=True),
        # strided convs: the harmonic source's noise convs, and the F0 / N curve's own
        "noise_conv_stride6": _layer(256, 22, 12, (800, 14000, 52000), stride=6),
        "f0_conv_stride2": _layer(1, 1, 3, (80, 1400, 5200), stride=2),
    }
    # the snake convs of the generator's resblocks: 3 / 7 / 11 taps at dilations 1 / 3 / 5, with and without fused statistics
    for rows, k, d, st in itertools.product((256, 128), (3, 7, 11), (1, 3, 5), (0, 1)):
        lens = (800, 14000, 52000) if rows == 256 else (4800, 84000, 312000)
        fam[f"snake_{rows}_k{k}_d{d}_s{st}"] = _layer(rows, rows, k, lens, dil=d, act=ACT_SNAKE, norm=1, stats=st, p1=True)
    return fam


def _launch(lay, mode, B, cols, force=0):
    rows, k = lay["rows"], lay["K"]
    bm, ch = _bm(rows), _chunks(lay["cin"])
    # f16f8: the layers the model gives an 8-bit cross image (Model::set_conv_mode); f16 / bf16: the decoder and generator convs
    f8 = mode == MODES["f16f8"] and lay["store"] != ST_UPSCATTER and bm == 128 and k in (3, 7, 11) and (k != 3 or rows <= 256) and \
        ch >= 2 and ch % 2 == 0
    prec1 = (1 if mode == MODES["f16"] else 2 if mode == MODES["bf16"] else 0) if lay["p1"] else 0
    x_ld = (cols + 31) // 32 * 32
    return dict(mode=mode, prec1=prec1, f8=int(f8), BM=bm, rows=rows, n_chunks16=ch, K=k, dil=lay["dil"], stride=lay["stride"],
                pad=(k - 1) * lay["dil"] // 2, act=lay["act"], in_up2=lay["in_up2"], store=lay["store"], accum=0, epi=lay["epi"],
                norm=lay["norm"], stats=lay["stats"], image=1, merge_T=cols if lay["token_axis"] else 0, x_bs=lay["cin"] * x_ld, x_ld=x_ld,
                B=B, cols=cols, cus=CUS, force=force)


def _family_of(plan):
    """the MFMA family a plan runs on: what decides the bits of its products"""
    return {"F32": "f32", "DA_S16": "16x16x32", "DA_F8": "16x16x32+f8"}.get(plan["form"], "32x32x16")


FAMILIES = _families()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_what_decides_the_bits_does_not_follow_batch_or_length(name, mode):
    lay = FAMILIES[name]
    seen = {}
    for B, cols in itertools.product((1, 8, 64), lay["lengths"]):
        p = hk.conv_plan(**_launch(lay, MODES[mode], B, cols))
        seen[(B, cols)] = (_family_of(p), p["pre"], p["stat_cols"])
        # a flat tile list is laid out for the launch's own tile width
        assert p["flat_bn"] in (0, p["bn"]), (B, cols, p)
        assert p["flat_bn"] == 0 or B > 1, (B, cols, p)
        assert (p["stat_cols"] > 0) == (lay["stats"] == 1), (B, cols, p)
        if p["stat_cols"]:
            assert p["bn"] % p["stat_cols"] == 0 and p["stat_tiles"] == -(-p["cols"] // p["bn"]) * (p["bn"] // p["stat_cols"]), p
        # override 1 (the LDS-DMA forms only): never a direct-A form
        q = hk.conv_plan(**_launch(lay, MODES[mode], B, cols, force=1))
        assert q["form"] in ("F32", "LDS") and q["flat_bn"] == 0, (B, cols, q)
    assert len(set(seen.values())) == 1, seen


def test_the_plan_takes_the_forms_of_each_family():
    """Spot checks of the forms the plan takes (the library's behaviour before the plan existed, read off its dispatch)."""
    fam = FAMILIES

    def plan(name, mode, B, cols, force=0):
        return hk.conv_plan(**_launch(fam[name], MODES[mode], B, cols, force))

    # 11-tap snake convs: the 16x16x32 form (f16f8: its F8 form), 192 columns on big grids, 128 on small ones, 64-column slots
    p = plan("snake_128_k11_d3_s1", "f16x3", 64, 84000)
    assert (p["form"], p["bn"], p["stat_cols"], p["flat_bn"]) == ("DA_S16", 192, 64, 192)
    assert plan("snake_128_k11_d3_s1", "f16x3", 1, 4800)["bn"] == 128
    assert plan("snake_128_k11_d3_s1", "f16f8", 64, 84000)["form"] == "DA_F8"
    # 3-tap snake convs in f16x3 mode: the 2 x 2-wave direct-A form on the 256-column tile, 4 x 1 with override bit FORCE_DA_4X1
    p = plan("snake_256_k3_d1_s0", "f16x3", 64, 14000)
    assert (p["form"], p["kt"], p["bn"]) == ("DA_W2", 3, 256)
    assert plan("snake_256_k3_d1_s0", "f16x3", 64, 14000, force=2 | 4)["form"] == "DA"
    p = plan("snake_128_k11_d3_s0", "f16x3", 8, 84000, force=2 | 4 | 8)
    assert (p["form"], p["kt"], p["bn"]) == ("DA", 11, 256)
    # reduced precision: the 4 x 1 forms (bf16: on the bf16 image)
    p = plan("snake_256_k3_d1_s0", "bf16", 64, 14000)
    assert (p["form"], p["p1"], p["bf"], p["bn"]) == ("DA", 1, 1, 256)
    # the 1024-row decoder convs: a pre-split image in the f16x3 modes; the narrow form without staging on small grids
    assert plan("decoder_1024", "f16x3", 1, 700)["form"] == "DAPN"
    p = plan("decoder_1024", "f16f8", 64, 2600)
    assert (p["form"], p["pre"], p["act"], p["kt"], p["bn"]) == ("DA_PRE", 1, ACT_NONE, 3, 256)
    assert plan("decoder_1024", "f16", 64, 2600)["pre"] == 0
    assert plan("decoder_1024_up2", "f16x3", 64, 5200)["pre"] == 0
    # the polyphase upsamplers: pre-split, run-time taps
    p = plan("ups_10x", "f16x3", 64, 5201)
    assert (p["form"], p["pre"], p["kt"]) == ("DA_PRE", 1, 0)
    # k = 1 GEMMs: merged token-axis columns; the narrow direct-A GEMM on small grids
    p = plan("albert_qkv", "f16x3", 64, 510)
    assert (p["form"], p["merged"], p["cols"]) == ("DAG", 1, 64 * 510)
    assert plan("albert_qkv", "f16x3", 1, 64)["form"] == "DAGN"
    p = plan("albert_qkv", "f16x3", 64, 510, force=1)
    assert (p["form"], p["vt"], p["wm"], p["wn"]) == ("LDS", 2, 2, 2)
    # the strided noise conv: the LDS-DMA form without the prefetching build
    p = plan("noise_conv_stride6", "f16x3", 8, 14000)
    assert (p["form"], p["pf"], p["bn"]) == ("LDS", 0, 256)
    # f32 mode: conv1d_mfma_kernel, 64-column slots
    p = plan("predictor_512", "f32", 8, 1400)
    assert (p["form"], p["bn"], p["stat_cols"]) == ("F32", 128, 64)
