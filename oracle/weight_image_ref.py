"""NumPy reference of a conv layer's weight images (kokorox_amd/csrc/conv_call.hip: pack_conv, pack_convT, add_bf16_image,
add_f8_image), written from the definitions and from the layout comments of kx_common.h -- every layout below answers "where does
element (row, ci, tap, part) live", the packers' kernels go the other way, from an image position to its element.

  shift     one power of two per layer: max|w| = m 2^e with m in [0.5, 1) (frexp), ws = 12 - e, clamped to [-8, 24], so that
            max|w| 2^ws lies in [2^11, 2^12); ws = 0 for an all-zero layer.  unscale = 2^-ws.
  split     v = f32(w 2^ws); hi = f16(v), lo = f16(v - hi), both round to nearest even.
  bf16      bf16(f32(hi) + f32(lo)), round to nearest even, in the hi slots of the split image's layout, +0 in the lo slots.
  e4m3      OCP FP8 E4M3, finite only: 4 exponent bits (bias 7), 3 mantissa bits, subnormal quantum 2^-9, largest value 448, no
            infinities.  The cross-term operands are e4m3(2^-4 hi) and e4m3(2^7 lo), each clamped to +-448 BEFORE the conversion
            (the conversion itself does not saturate), round to nearest even.
  rows      up to three sources [rows_i][Cin][K] stand for their row-wise concatenation.  A ConvTranspose1d weight [Cin][Cout][2 s]
            is the two-tap polyphase GEMM: row = co s + p (phase fastest), tap 0 = w[ci][co][p + s] (it multiplies x[q - 1]),
            tap 1 = w[ci][co][p] (it multiplies x[q]).

The five layouts, as offsets in units of the image's element:
  w    f32     [row tile of BM][chunk of 8 channels][tap][channel in chunk][row in tile]
  w16  f16     [row tile of BM][chunk of 16 channels][tap][hi | lo][octet of the chunk][row in tile][channel in octet]
  w16b bf16    the layout of w16 (BM = 128 only)
  w8x  bytes   [row tile of 128][chunk of 16][tap group of 4][g = octet + 2 (tap pair)][slot][row in tile][16 bytes]; the slot of
               tap group m, pair g >> 1 holds tap 4 m + 2 (g >> 1) + slot; its 16 bytes are four dwords, dword d =
               [lo(2 d), lo(2 d + 1), hi(2 d), hi(2 d + 1)] of the octet's channels (8-bit operands, lowest byte first)
  and the transposed conv's w / w16 are those of its GEMM, K = 2.
Padding (rows past the layer's in the last tile, channels past Cin in the last chunk, taps >= K in the last tap group) is +0.

The second half restates the conv forms' arithmetic on given operands, products and sums in float64 (emulate_conv).
"""
from __future__ import annotations

import numpy as np

CK, CK16 = 8, 16
WS_MIN, WS_MAX = -8, 24
F8_HI_SCALE, F8_LO_SCALE = 2.0 ** -4, 2.0 ** 7  # the weights' cross-term operands
F8_ACT_LO_SCALE = 2.0 ** 11                     # the activations' residual (split_pair_f8)
E4M3_MAX = 448.0
F16_MAX = 65504.0


# ---- the layer's sizes ------------------------------------------------------------------------------------------------------
def pick_bm(rows: int) -> int:
    """Rows per weight tile: 128 from 128 rows on, 64 above 32, else 32 (conv_pick_bm)."""
    return 128 if rows >= 128 else (64 if rows > 32 else 32)


def f8_layer(BM: int, rows: int, K: int, n_chunks16: int) -> bool:
    """The layers that get an 8-bit image: 128-row tiles, 3 / 7 / 11 taps (3 taps: at most 256 rows), an even number of 16-channel chunks."""
    return BM == 128 and K in (3, 7, 11) and (K != 3 or rows <= 256) and n_chunks16 >= 2 and n_chunks16 % 2 == 0


# ---- shift, split, codecs ---------------------------------------------------------------------------------------------------
def weight_shift(absmax) -> int:
    a = float(np.float32(absmax))
    if not (a > 0.0) or not np.isfinite(a):
        return 0
    _, e = np.frexp(np.float32(a))  # a = m 2^e, m in [0.5, 1)
    return int(min(max(12 - int(e), WS_MIN), WS_MAX))


def carried(absmax, ws=None):
    """The pack path's contract: None if the layer is carried, else why it is refused."""
    a = float(np.float32(absmax))
    if not np.isfinite(a):
        return "non-finite"
    if a * 2.0 ** (weight_shift(a) if ws is None else ws) > F16_MAX:
        return "beyond the split's range"
    return None


def _round_e4m3(x):
    """Round to nearest, ties to even: the one place the e4m3 encoder rounds."""
    return np.rint(x)


def _round_bf16(x):
    return np.rint(x)


def split(w, ws: int):
    """-> (hi, lo) as float16 arrays of w's shape."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = (np.asarray(w, dtype=np.float32) * np.float32(2.0 ** ws)).astype(np.float32)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def e4m3_encode(x):
    """float32 values -> e4m3 bytes, after the clamp to +-448; the sign of a zero is kept."""
    x = np.asarray(x, dtype=np.float32)
    a = np.minimum(np.abs(x.astype(np.float64)), E4M3_MAX)
    _, e = np.frexp(a)                       # a = m 2^e, m in [0.5, 1): the binade is 2^(e - 1)
    ex = np.maximum(e - 1, -6)               # subnormals share the smallest normal binade's quantum
    q = _round_e4m3(a / 2.0 ** (ex - 3))         # in units of the quantum 2^(ex - 3): 8 .. 16 for a normal value, 0 .. 8 below 2^-6
    up = q >= 16                             # rounded up into the next binade
    ex = np.where(up, ex + 1, ex)
    q = np.where(up, 8, q).astype(np.int64)
    normal = q >= 8
    field = np.where(normal, ((ex + 7) << 3) | (q - 8), q)  # subnormal: exponent field 0, mantissa = multiples of 2^-9
    return (np.where(np.signbit(x), 0x80, 0) | field).astype(np.uint8)


def e4m3_decode(b):
    b = np.asarray(b, dtype=np.uint8).astype(np.int64)
    ef, m = (b >> 3) & 15, b & 7
    mag = np.where(ef == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (ef - 10.0))
    return np.where(b & 0x80, -mag, mag)


def bf16_bits(x):
    """float32 values -> bf16 bit patterns (8 significant bits, float32's exponent range), round to nearest even."""
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(x.astype(np.float64))
    _, e = np.frexp(a)
    ex = np.maximum(e - 1, -126)
    r = (_round_bf16(a / 2.0 ** (ex - 7.0)) * 2.0 ** (ex - 7.0)).astype(np.float32)  # (a multiple of the quantum: exact in float32)
    bits = (r.view(np.uint32) >> 16).astype(np.uint16)
    return bits | np.where(np.signbit(x), 0x8000, 0).astype(np.uint16)


def bf16_source(hi, lo):
    """What the bf16 image rounds: hi + lo in float32."""
    return hi.astype(np.float32) + lo.astype(np.float32)


def f8_operands(hi, lo):
    """-> (hi8, lo8): the e4m3 bytes of the cross terms' weight operands."""
    h = np.clip(hi.astype(np.float32) * np.float32(F8_HI_SCALE), -E4M3_MAX, E4M3_MAX)
    l = np.clip(lo.astype(np.float32) * np.float32(F8_LO_SCALE), -E4M3_MAX, E4M3_MAX)
    return e4m3_encode(h), e4m3_encode(l)


# ---- rows -------------------------------------------------------------------------------------------------------------------
def source_of_row(row, src_rows):
    """GEMM row -> (source, row within it) for row-concatenated sources."""
    row = np.asarray(row)
    starts = np.concatenate([[0], np.cumsum(src_rows)])
    i = np.searchsorted(starts, row, side="right") - 1
    return i, row - starts[i]


def convT_element(row, tap, Cout: int, s: int):
    """GEMM (row, tap) of a transposed conv -> (co, k): the weight w[ci][co][k] it holds."""
    co, p = row // s, row % s
    return co, np.where(tap == 0, p + s, p)


def gemm_weights(sources, up_stride: int = 0):
    """The layer as its GEMM sees it: float32 [rows][Cin][K]."""
    src = [np.asarray(a, dtype=np.float32) for a in sources]
    if up_stride:
        w = src[0]  # [Cin][Cout][2 s]
        Cin, Cout, _ = w.shape
        row, tap = np.meshgrid(np.arange(up_stride * Cout), np.arange(2), indexing="ij")
        co, k = convT_element(row, tap, Cout, up_stride)
        return np.ascontiguousarray(w[:, co, k].transpose(1, 0, 2))  # [Cin][rows][2] -> [rows][Cin][2]
    rows = [a.shape[0] for a in src]
    i, r = source_of_row(np.arange(sum(rows)), rows)
    return np.stack([src[int(a)][int(b)] for a, b in zip(i, r)])


# ---- layouts: where element (row, ci, tap, part) lives ------------------------------------------------------------------------
class Dims:
    def __init__(self, rows: int, Cin: int, K: int):
        self.rows, self.Cin, self.K = rows, Cin, K
        self.BM = pick_bm(rows)
        self.tiles = -(-rows // self.BM)
        self.n_chunks = -(-Cin // CK)
        self.n_chunks16 = -(-Cin // CK16)
        self.tiles128 = -(-rows // 128)
        self.groups = -(-K // 4)

    @property
    def w_floats(self):
        return self.tiles * self.n_chunks * self.K * CK * self.BM

    @property
    def w16_halves(self):
        return self.tiles * self.n_chunks16 * self.K * 2 * 2 * self.BM * 8

    @property
    def w8x_bytes(self):
        return self.tiles128 * self.n_chunks16 * self.groups * 4 * 2 * 128 * 16


def addr_w(d: Dims, row, ci, tap):
    """Offset, in floats, of weight (row, ci, tap) in the f32 image."""
    return ((((row // d.BM) * d.n_chunks + ci // CK) * d.K + tap) * CK + ci % CK) * d.BM + row % d.BM


def addr_w16(d: Dims, row, ci, tap, part):
    """Offset, in halves, of part (0 = hi, 1 = lo) of weight (row, ci, tap) in the split-f16 image (and in the bf16 image)."""
    octet, j = (ci % CK16) // 8, ci % 8
    return ((((((row // d.BM) * d.n_chunks16 + ci // CK16) * d.K + tap) * 2 + part) * 2 + octet) * d.BM + row % d.BM) * 8 + j


def addr_w8x(d: Dims, row, ci, tap, part):
    """Offset, in bytes, of the 8-bit operand of part (0 = hi, 1 = lo) of weight (row, ci, tap) in the 8-bit image."""
    octet, j = (ci % CK16) // 8, ci % 8
    group, pair, slot = tap // 4, (tap % 4) // 2, tap % 2
    g = octet + 2 * pair
    byte = 4 * (j // 2) + (j % 2) + (0 if part else 2) * np.ones_like(j)  # dword j // 2 = [lo, lo, hi, hi] of channels 2 d, 2 d + 1
    return ((((((row // 128) * d.n_chunks16 + ci // CK16) * d.groups + group) * 4 + g) * 2 + slot) * 128 + row % 128) * 16 + byte


def _grid(d: Dims):
    return np.meshgrid(np.arange(d.rows), np.arange(d.Cin), np.arange(d.K), indexing="ij")


def pack_w(d: Dims, W):
    out = np.zeros(d.w_floats, dtype=np.float32)
    r, c, t = _grid(d)
    out[addr_w(d, r, c, t)] = W
    return out


def pack_w16(d: Dims, hi, lo, dtype=np.float16):
    out = np.zeros(d.w16_halves, dtype=dtype)
    r, c, t = _grid(d)
    out[addr_w16(d, r, c, t, 0)] = hi
    if lo is not None:
        out[addr_w16(d, r, c, t, 1)] = lo
    return out


def pack_w8x(d: Dims, hi8, lo8):
    out = np.zeros(d.w8x_bytes, dtype=np.uint8)
    r, c, t = _grid(d)
    out[addr_w8x(d, r, c, t, 0)] = hi8
    out[addr_w8x(d, r, c, t, 1)] = lo8
    return out


def unpack_w16(d: Dims, image):
    """-> (hi, lo) [rows][Cin][K] out of a split-f16 image, and a mask of the image's slots that hold no element."""
    image = np.asarray(image)
    r, c, t = _grid(d)
    a0, a1 = addr_w16(d, r, c, t, 0), addr_w16(d, r, c, t, 1)
    free = np.ones(image.shape[0], dtype=bool)
    free[a0] = False
    free[a1] = False
    return image[a0], image[a1], free


def images(sources, up_stride: int = 0):
    """What kx_test_weight_images returns for the same arguments: the sizes, unscale and the raw bytes of the four images (an
    image the layer does not get has length 0).  A layer the pack path refuses raises ValueError with the reason."""
    if isinstance(sources, np.ndarray):
        sources = [sources]
    W = gemm_weights(sources, up_stride)
    d = Dims(*W.shape)
    absmax = np.float32(np.abs(W).max()) if not np.isnan(W).any() else np.float32(np.nan)
    why = carried(absmax)
    if why:
        raise ValueError(why)
    ws = weight_shift(absmax)
    hi, lo = split(W, ws)
    out = {"BM": d.BM, "rows": d.rows, "n_chunks": d.n_chunks, "n_chunks16": d.n_chunks16, "K": d.K, "ws": ws, "unscale": 2.0 ** -ws,
           "hi": hi, "lo": lo, "dims": d}
    out["w"] = pack_w(d, W).view(np.uint8)
    out["w16"] = pack_w16(d, hi, lo).view(np.uint8)
    empty = np.zeros(0, dtype=np.uint8)
    out["w16b"] = pack_w16(d, bf16_bits(bf16_source(hi, lo)), None, np.uint16).view(np.uint8) if d.BM == 128 else empty
    if not up_stride and f8_layer(d.BM, d.rows, d.K, d.n_chunks16):
        out["w8x"] = pack_w8x(d, *f8_operands(hi, lo))
    else:
        out["w8x"] = empty
    return out


# ---- the conv forms' arithmetic, restated -------------------------------------------------------------------------------------
def _f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float64)


def act_operands(v):
    """The activation side of a product, from the float32 value v the kernel splits: a dict of float64 arrays.
    hi, lo: split_pair (clamped to +-65504; hi = f16(v), lo = f16(v - hi)); bf: bf16(v); x8, lo8: split_pair_f8's 8-bit operands
    e4m3(clamp(v, +-448)) and e4m3(clamp(2^11 (v - hi), +-448))."""
    v = np.clip(np.asarray(v, dtype=np.float32), -F16_MAX, F16_MAX)
    hi32 = v.astype(np.float16).astype(np.float32)
    res = v - hi32
    bf = (bf16_bits(v).astype(np.uint32) << 16).view(np.float32)
    x8 = e4m3_decode(e4m3_encode(np.clip(v, -E4M3_MAX, E4M3_MAX)))
    lo8 = e4m3_decode(e4m3_encode(np.clip(res * np.float32(F8_ACT_LO_SCALE), -E4M3_MAX, E4M3_MAX)))
    return {"f32": v.astype(np.float64), "hi": hi32.astype(np.float64), "lo": _f16(res), "bf": bf.astype(np.float64), "x8": x8, "lo8": lo8}


def weight_operands(W):
    """The weights' side, from the float32 GEMM weights [rows][Cin][K] of a whole layer (the shift is the layer's)."""
    W = np.asarray(W, dtype=np.float32)
    ws = weight_shift(np.abs(W).max())
    hi, lo = split(W, ws)
    hi8, lo8 = f8_operands(hi, lo)
    bf = (bf16_bits(bf16_source(hi, lo)).astype(np.uint32) << 16).view(np.float32)
    return {"ws": ws, "f32": W.astype(np.float64) * 2.0 ** ws, "hi": hi.astype(np.float64), "lo": lo.astype(np.float64), "bf": bf.astype(np.float64),
            "hi8": e4m3_decode(hi8) / F8_HI_SCALE, "lo8": e4m3_decode(lo8) / F8_LO_SCALE}


FORMS = ("f32", "f16x3", "f16f8", "f16", "bf16")


def emulate_products(form: str, a: dict, w: dict):
    """The list of (activation operand, weight operand, factor) a form sums per product; lo x lo is dropped as the kernels drop it."""
    if form == "f32":
        return [(a["f32"], w["f32"], 1.0)]
    if form == "f16x3":
        return [(a["hi"], w["hi"], 1.0), (a["hi"], w["lo"], 1.0), (a["lo"], w["hi"], 1.0)]
    if form == "f16f8":  # hi x hi on the f16 MFMA; the cross terms on 8-bit operands
        return [(a["hi"], w["hi"], 1.0), (a["x8"], w["lo8"], 1.0), (a["lo8"], w["hi8"], 1.0 / F8_ACT_LO_SCALE)]
    if form == "f16":
        return [(a["hi"], w["hi"], 1.0)]
    if form == "bf16":
        return [(a["bf"], w["bf"], 1.0)]
    raise ValueError(form)


def emulate_conv(form: str, a: dict, w: dict, conv):
    """A form's result on given operands with every product and sum in float64: conv(x64, w64) -> y64 is the caller's plain conv
    (its padding, dilation, ragged lengths), linear in both arguments; the weight shift is undone at the end, as the kernels do."""
    y = None
    for xa, wb, f in emulate_products(form, a, w):
        t = conv(xa, wb * f)
        y = t if y is None else y + t
    return y * 2.0 ** -w["ws"]
