"""CPU: the reference of a conv layer's weight images (oracle/weight_image_ref.py), held to statements that do not come from it.

tests/test_gpu_weight_images.py compares the packers' bytes with this reference, so a reference that shared a mistake with a
packer -- or had one of its own -- must not pass here.  Every check below is a function of the reference module and states one
thing against something independent: torch's float8_e4m3fn and bfloat16, np.concatenate, F.conv_transpose1d, and offsets worked
out by hand from the layout comments of kokorox_amd/csrc/kx_common.h.  test_mutations_are_rejected then breaks the reference in
the ten ways a packer could be wrong and asserts that the check named beside each one fails.

The cases of the GPU file (shapes and draws) live here too, with the properties the draws must have.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import weight_image_ref as R


# ---- the cases of tests/test_gpu_weight_images.py -----------------------------------------------------------------------------------
def draw(shape, seed, lo_exp=-30, hi_exp=0, zeros=True):
    """float32 weights, magnitude log-uniform over 2^lo_exp .. 2^hi_exp, random sign, one in 64 a +0."""
    rng = np.random.default_rng(seed)
    w = np.exp2(rng.uniform(lo_exp, hi_exp, shape)) * rng.choice([-1.0, 1.0], shape)
    if zeros:
        w[rng.random(shape) < 1.0 / 64] = 0.0
    return w.astype(np.float32)


def _pattern(shape, seed, mark):
    """A source of its own value pattern: the draw with the low mantissa bits replaced by `mark`, so the same (row, ci, tap) of
    another source is another number."""
    w = draw(shape, seed, zeros=False)
    return ((w.view(np.uint32) & ~np.uint32(3)) | np.uint32(mark)).view(np.float32)


# (rows, Cin, K): every BM of conv_pick_bm on both sides of its borders (1, 33 | 127, 128, 129, 130, 256); rows that are no
# multiple of BM; Cin that is no multiple of 16 (17, 24, 56, 130, 20) nor of the f32 image's 8 (17, 130, 20); K = 3, 7, 11 on layers
# with an 8-bit image (129 x 20 x 3, 130 x 24 x 7, 128 x 56 x 11: one, two, three tap groups, the last with empty tap slots) and
# layers without (64-row tiles; K = 2, 5; 33 rows)
PLAIN_SHAPES = [(1, 1, 1), (33, 17, 3), (130, 24, 7), (128, 56, 11), (256, 32, 2), (127, 130, 5), (129, 20, 3)]
CONVT_SHAPES = [(17, 5, 6), (32, 20, 10), (16, 128, 6)]  # (Cin, Cout, stride)
WIDE = (128, 56, 11)  # drawn over 2^-8 .. 2^22: the shift at its lower clamp, where the 8-bit operands reach +-448


def image_cases():
    """[(id, sources, up_stride)]"""
    cases = []
    for i, s in enumerate(PLAIN_SHAPES):
        w = draw(s, 100 + i, -8, 22) if s == WIDE else draw(s, 100 + i)
        cases.append(("%dx%dx%d" % s, [w], 0))
    cases.append(("3src-5+64+60x72x1", [_pattern((r, 72, 1), 200 + j, j + 1) for j, r in enumerate((5, 64, 60))], 0))
    cases.append(("2src-1024+1024x72x1", [_pattern((1024, 72, 1), 300 + j, j + 1) for j in range(2)], 0))
    for i, (cin, cout, s) in enumerate(CONVT_SHAPES):
        cases.append(("convT-%dx%dx%d" % (cin, cout, s), [draw((cin, cout, 2 * s), 400 + i)], s))
    return cases


def test_the_cases_cover_what_they_claim():
    refs = {cid: R.images(src, s) for cid, src, s in image_cases()}
    assert {r["BM"] for r in refs.values()} == {32, 64, 128}
    with8 = [cid for cid, r in refs.items() if r["w8x"].size]
    assert {refs[c]["K"] for c in with8} == {3, 7, 11} and len(with8) < len(refs)
    assert any(r["w16b"].size for r in refs.values()) and any(not r["w16b"].size for r in refs.values())
    assert any(r["rows"] % r["BM"] for r in refs.values())
    # every number format meets its subnormal range, a zero and (the 8-bit operands) its clamp somewhere
    f16_sub = lambda h: (np.abs(h.astype(np.float32)) < 2.0 ** -14) & (h != 0)
    assert any(f16_sub(r["hi"]).any() for r in refs.values()) and any(f16_sub(r["lo"]).any() for r in refs.values())
    assert any((r["hi"] == 0).any() for r in refs.values())
    hi8, lo8 = zip(*[R.f8_operands(refs[c]["hi"], refs[c]["lo"]) for c in with8])
    for b in (np.concatenate([a.ravel() for a in hi8]), np.concatenate([a.ravel() for a in lo8])):
        sub = ((b >> 3) & 15 == 0) & (b & 7 != 0)
        assert sub.any() and (b & 0x7f == 0x7e).any() and (b == 0).any()
    bf = np.concatenate([r["w16b"].view(np.uint16) for r in refs.values() if r["w16b"].size])
    assert (((bf >> 7) & 0xff == 0) & (bf & 0x7f != 0)).sum() == 0  # (bf16 has float32's exponent range: no subnormal from an f16 sum)
    wide = refs["%dx%dx%d" % WIDE]
    assert wide["ws"] == -8 and np.isfinite(wide["hi"].astype(np.float32)).all()


# ---- the named checks ---------------------------------------------------------------------------------------------------------------
def check_e4m3_codec(R):
    """The encoder against torch.float8_e4m3fn on every finite f16 value times 2^-4 and times 2^7, clamped as the kernel clamps;
    the decoder on every byte that is no NaN."""
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    h = h[np.isfinite(h)].astype(np.float32)
    for scale in (2.0 ** -4, 2.0 ** 7):
        x = np.clip(h * np.float32(scale), -448.0, 448.0).astype(np.float32)
        want = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        np.testing.assert_array_equal(R.e4m3_encode(x), want)
    b = np.array([i for i in range(256) if i & 0x7f != 0x7f], dtype=np.uint8)
    np.testing.assert_array_equal(R.e4m3_decode(b), torch.from_numpy(b).view(torch.float8_e4m3fn).double().numpy())


def check_bf16_codec(R):
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-140, 120, 200000))).astype(np.float32)
    x[:4] = [0.0, -0.0, 2056.0, 2072.0]  # (ties: to the even neighbour)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(R.bf16_bits(x), want)


def check_shift(R):
    """absmax 2^ws in [2^11, 2^12) between the clamps; at 2^e exactly and one ulp below it; 0; either clamp."""
    f = np.float32
    assert R.weight_shift(f(1.0)) == 11 and R.weight_shift(np.nextafter(f(1.0), f(0.0))) == 12
    assert R.weight_shift(f(2.0 ** -7)) == 18 and R.weight_shift(np.nextafter(f(2.0 ** -7), f(0.0))) == 19
    for e in range(-12, 20):
        for a in (f(2.0 ** e), np.nextafter(f(2.0 ** e), f(0.0)), f(1.37 * 2.0 ** e)):
            assert 2.0 ** 11 <= float(a) * 2.0 ** R.weight_shift(a) < 2.0 ** 12, (e, a)
    assert R.weight_shift(f(0.0)) == 0
    assert R.weight_shift(f(2.0 ** -13)) == 24 and R.weight_shift(f(2.0 ** -14)) == 24 and R.weight_shift(f(1e-30)) == 24
    assert R.weight_shift(f(2.0 ** 19)) == -8 and R.weight_shift(f(2.0 ** 21)) == -8
    assert R.carried(f(2.0 ** 21)) is None and R.carried(f(65504.0 * 256.0)) is None
    assert R.carried(np.nextafter(f(65504.0 * 256.0), f(np.inf))) == "beyond the split's range"
    assert R.carried(f(np.inf)) == "non-finite" and R.carried(f(np.nan)) == "non-finite"


def _single(shape, at, value=1.0 + 2.0 ** -12):
    """A layer with one non-zero weight: 1 + 2^-12 -> shift 11, v = 2048.5, hi = 2048, lo = 0.5."""
    w = np.zeros(shape, dtype=np.float32)
    w[at] = value
    return w


def _nonzero(image, dtype):
    a = image.view(dtype)
    return {int(i): a[i].item() for i in np.flatnonzero(a)}


def check_spots_w(R):
    """f32 image [row tile][chunk of 8][tap][channel in chunk][row in tile]: 130 x 24 x 7 -> BM 128, 3 chunks; weight
    (129, 10, 4) -> tile 1, chunk 1, channel 2, row 1: (((1 * 3 + 1) * 7 + 4) * 8 + 2) * 128 + 1."""
    im = R.images([_single((130, 24, 7), (129, 10, 4))])
    assert (im["BM"], im["n_chunks"]) == (128, 3) and im["w"].size == 4 * 2 * 3 * 7 * 8 * 128
    assert _nonzero(im["w"], np.float32) == {33025: 1.0 + 2.0 ** -12}


def check_spots_w16(R):
    """split image [row tile][chunk of 16][tap][hi | lo][octet][row in tile][channel in octet], in halves.
    33 x 17 x 3 -> BM 64, 2 chunks.  (5, 9, 2): chunk 0, octet 1, channel 1 -> hi ((((0 * 3 + 2) * 2 + 0) * 2 + 1) * 64 + 5) * 8 + 1
    = 4649, lo ((((2) * 2 + 1) * 2 + 1) * 64 + 5) * 8 + 1 = 5673.  (32, 16, 0): chunk 1, octet 0, channel 0 -> hi
    ((((1 * 3 + 0) * 2 + 0) * 2 + 0) * 64 + 32) * 8 = 6400, lo ((((3) * 2 + 1) * 2 + 0) * 64 + 32) * 8 = 7424."""
    for at, hi_at, lo_at in (((5, 9, 2), 4649, 5673), ((32, 16, 0), 6400, 7424)):
        im = R.images([_single((33, 17, 3), at)])
        assert (im["BM"], im["n_chunks16"], im["ws"]) == (64, 2, 11) and im["w16"].size == 2 * 1 * 2 * 3 * 4 * 64 * 8
        assert _nonzero(im["w16"], np.float16) == {hi_at: 2048.0, lo_at: 0.5}, at
        assert im["w16b"].size == 0 and im["w8x"].size == 0


def check_spots_w8x(R):
    """8-bit image [row tile of 128][chunk of 16][tap group][g = octet + 2 pair][slot][row][16 bytes], 130 x 24 x 7 -> 2 chunks,
    2 tap groups.  (129, 13, 6): tile 1, chunk 0, group 1, pair 1, slot 0, octet 1 -> g 3, row 1; channel 5 of the octet is the
    second of dword 2: lo byte 9, hi byte 11: (((((1 * 2 + 0) * 2 + 1) * 4 + 3) * 2 + 0) * 128 + 1) * 16 = 94224.
    (0, 0, 1): group 0, pair 0, slot 1, g 0: ((((0) * 4 + 0) * 2 + 1) * 128 + 0) * 16 = 2048; channel 0: lo byte 0, hi byte 2."""
    for at, lo_at, hi_at in (((129, 13, 6), 94233, 94235), ((0, 0, 1), 2048, 2050)):
        im = R.images([_single((130, 24, 7), at)])
        assert im["w8x"].size == 2 * 2 * 2 * 4 * 2 * 128 * 16
        assert set(_nonzero(im["w8x"], np.uint8)) == {lo_at, hi_at}, at


def check_f8_values(R):
    """hi = 2048 -> 2^-4 hi = 128 = 2^7: exponent field 14, mantissa 0 = 0x70; lo = 0.5 -> 2^7 lo = 64 = 2^6: field 13 = 0x68."""
    im = R.images([_single((130, 24, 7), (0, 0, 1))])
    assert _nonzero(im["w8x"], np.uint8) == {2048: 0x68, 2050: 0x70}
    # the clamp before the conversion: hi = 16384 -> 1024 -> 448 = 0x7e; lo = -6 -> -768 -> -448 = 0xfe
    hi8, lo8 = R.f8_operands(np.array([16384.0], dtype=np.float16), np.array([-6.0], dtype=np.float16))
    assert (int(hi8[0]), int(lo8[0])) == (0x7e, 0xfe)


def _case_arrays():
    return [R.gemm_weights(src, s) for _, src, s in image_cases() if src[0].size < 50000]


def check_unpack(R):
    """unpack(pack(w)): hi + lo == f32(w 2^ws) exactly wherever lo is a normal f16 (weights of 21 significant bits: what is left
    of v after its 11-bit hi then fits lo's 11 bits), to 2^-22 |v| for any weight (lo is within half an ulp of a residual that is
    within half an ulp of hi); every slot that holds no element is +0; the bf16 image of the same layout holds torch's bfloat16
    of hi + lo."""
    for W in _case_arrays():
        W21 = (W.view(np.uint32) & ~np.uint32(7)).view(np.float32)
        for w, exact in ((W21, True), (W, False)):
            im = R.images([w])
            d = im["dims"]
            hi, lo, free = R.unpack_w16(d, im["w16"].view(np.float16))
            assert not im["w16"].view(np.uint16)[free].any() and free.sum() == free.size - 2 * w.size
            v = (w.astype(np.float64) * 2.0 ** im["ws"])
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v)  # (a power of two: no rounding in float32)
            s = hi.astype(np.float64) + lo.astype(np.float64)
            assert np.all(np.abs(s - v) <= 2.0 ** -22 * np.abs(v) + 2.0 ** -25)  # (2^-25: half of f16's subnormal quantum)
            if exact:
                normal = np.abs(lo.astype(np.float64)) >= 2.0 ** -14
                assert normal.any() and np.array_equal(s[normal], v[normal])


def check_bf16_image(R):
    for W in _case_arrays():
        im = R.images([W])
        if not im["w16b"].size:
            continue
        d = im["dims"]
        hi, lo, _ = R.unpack_w16(d, im["w16"].view(np.float16))
        bh, bl, free = R.unpack_w16(d, im["w16b"].view(np.uint16))
        want = torch.from_numpy(hi.astype(np.float32) + lo.astype(np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        np.testing.assert_array_equal(bh, want)
        assert not bl.any() and not im["w16b"].view(np.uint16)[free].any()


def check_addresses(R):
    """Every layout sends the layer's elements to distinct offsets inside its image."""
    for rows, Cin, K in PLAIN_SHAPES + [(192, 64, 2)]:
        d = R.Dims(rows, Cin, K)
        r, c, t = np.meshgrid(np.arange(rows), np.arange(Cin), np.arange(K), indexing="ij")
        a = R.addr_w(d, r, c, t).ravel()
        assert a.min() >= 0 and a.max() < d.w_floats and np.unique(a).size == a.size
        for addr, n in ((R.addr_w16, d.w16_halves), (R.addr_w8x, d.w8x_bytes)):
            a = np.concatenate([addr(d, r, c, t, p).ravel() for p in (0, 1)])
            assert a.min() >= 0 and a.max() < n and np.unique(a).size == a.size


def check_sources(R):
    """Row-concatenated sources are their concatenation."""
    for rows in ((5, 64, 60), (3, 4), (7,)):
        src = [_pattern((r, 6, 2), 50 + j, j + 1) for j, r in enumerate(rows)]
        np.testing.assert_array_equal(R.gemm_weights(src), np.concatenate(src))
        i, r = R.source_of_row(np.arange(sum(rows)), rows)
        assert i[0] == 0 and r[0] == 0 and i[-1] == len(rows) - 1 and r[-1] == rows[-1] - 1


def check_convT_rows(R):
    """GEMM row = co s + p, phase fastest (conv_epilogue.h, ST_UPSCATTER): with s = 6, row 13 is output channel 2, phase 1, and
    holds w[ci][2][1] and w[ci][2][7] (their sum does not depend on which tap is which)."""
    w = draw((4, 5, 12), 9)
    G = R.gemm_weights([w], 6)
    assert G.shape == (30, 4, 2)
    np.testing.assert_array_equal(G[13].astype(np.float64).sum(-1), w[:, 2, 1].astype(np.float64) + w[:, 2, 7])
    np.testing.assert_array_equal(G[29].astype(np.float64).sum(-1), w[:, 4, 5].astype(np.float64) + w[:, 4, 11])


def check_convT_polyphase(R):
    """The two-tap GEMM over q with left padding 1 IS ConvTranspose1d(k = 2 s, stride s, padding s / 2): out[co][s q + p - pad] =
    G[co s + p][.][0] . x[.][q - 1] + G[co s + p][.][1] . x[.][q]."""
    for Cin, Cout, s in ((3, 4, 6), (5, 2, 10), (2, 3, 5)):
        rng = np.random.default_rng(s)
        w = rng.standard_normal((Cin, Cout, 2 * s))
        x = rng.standard_normal((Cin, 9))
        pad, L = s // 2, x.shape[1]
        want = F.conv_transpose1d(torch.from_numpy(x)[None], torch.from_numpy(w), stride=s, padding=pad)[0].numpy()
        w32 = w.astype(np.float32)
        Gd = np.empty((s * Cout, Cin, 2))
        for tap in range(2):  # (the float64 weights in the places the float32 ones go)
            Gd[:, :, tap] = _gather64(R, w, s, tap)
        np.testing.assert_array_equal(R.gemm_weights([w32], s), Gd.astype(np.float32))
        xp = np.concatenate([np.zeros((Cin, 1)), x, np.zeros((Cin, 1))], axis=1)  # x[-1] .. x[L]
        got = np.zeros_like(want)
        for q in range(L + 1):
            col = Gd[:, :, 0] @ xp[:, q] + Gd[:, :, 1] @ xp[:, q + 1]
            for row in range(s * Cout):
                t = s * q + row % s - pad
                if 0 <= t < want.shape[1]:
                    got[row // s, t] += col[row]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def _gather64(R, w, s, tap):
    Cout = w.shape[1]
    row = np.arange(s * Cout)
    co, k = R.convT_element(row, np.full_like(row, tap), Cout, s)
    return w[:, co, k].T


CHECKS = [check_e4m3_codec, check_bf16_codec, check_shift, check_spots_w, check_spots_w16, check_spots_w8x, check_f8_values, check_unpack,
          check_bf16_image, check_addresses, check_sources, check_convT_rows, check_convT_polyphase]


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__)
def test_reference_meets(check):
    check(R)


# ---- the mutations ------------------------------------------------------------------------------------------------------------------
def _mut_planes(m):
    orig = R.addr_w16
    m.setattr(R, "addr_w16", lambda d, row, ci, tap, part: orig(d, row, ci, tap, 1 - part))


def _mut_octets(m):
    orig = R.addr_w16
    m.setattr(R, "addr_w16", lambda d, row, ci, tap, part: orig(d, row, ci ^ 8, tap, part))


def _mut_convT_taps(m):
    orig = R.convT_element
    m.setattr(R, "convT_element", lambda row, tap, Cout, s: orig(row, 1 - tap, Cout, s))


def _mut_convT_rows(m):
    def phase_major(row, tap, Cout, s):
        co, p = row % Cout, row // Cout
        return co, np.where(tap == 0, p + s, p)
    m.setattr(R, "convT_element", phase_major)


def _mut_f8_slot(m):
    orig = R.addr_w8x
    m.setattr(R, "addr_w8x", lambda d, row, ci, tap, part: orig(d, row, ci, tap // 4 * 4 + 2 * (tap % 2) + (tap % 4) // 2, part))


def _mut_f8_scale(m):
    m.setattr(R, "F8_LO_SCALE", 2.0 ** 8)


def _mut_e4m3_trunc(m):
    m.setattr(R, "_round_e4m3", np.floor)


def _mut_bf16_hi(m):
    m.setattr(R, "bf16_source", lambda hi, lo: hi.astype(np.float32))


def _mut_shift(m):
    orig = R.weight_shift

    def one_too_high(absmax):
        ws = orig(absmax)
        exact = float(absmax) > 0 and np.frexp(np.float32(absmax))[0] == 0.5
        return ws + 1 if exact and R.WS_MIN < ws < R.WS_MAX else ws
    m.setattr(R, "weight_shift", one_too_high)


def _mut_source_rows(m):
    orig = R.source_of_row

    def off_by_one(row, src_rows):
        i, r = orig(row, src_rows)
        return i, np.where(i == 1, (r + 1) % np.asarray(src_rows)[i], r)
    m.setattr(R, "source_of_row", off_by_one)


MUTATIONS = [
    ("hi and lo planes exchanged", _mut_planes, check_spots_w16),
    ("the two channel octets of a chunk exchanged", _mut_octets, check_spots_w16),
    ("the transposed conv's taps exchanged, p for p + s", _mut_convT_taps, check_convT_polyphase),
    ("its GEMM row taken as p Cout + co", _mut_convT_rows, check_convT_rows),
    ("the 8-bit image's tap pair and slot exchanged", _mut_f8_slot, check_spots_w8x),
    ("2^7 written as 2^8", _mut_f8_scale, check_f8_values),
    ("e4m3 by truncation", _mut_e4m3_trunc, check_e4m3_codec),
    ("bf16 of hi alone", _mut_bf16_hi, check_bf16_image),
    ("the shift one too high at an exact power of two", _mut_shift, check_shift),
    ("the second source's rows offset by one", _mut_source_rows, check_sources),
]


@pytest.mark.parametrize("what,mutate,check", MUTATIONS, ids=[m[0].replace(" ", "_") for m in MUTATIONS])
def test_mutations_are_rejected(what, mutate, check, monkeypatch):
    check(R)
    mutate(monkeypatch)
    with pytest.raises(AssertionError):
        check(R)
    monkeypatch.undo()
    check(R)
