"""Float64 references, a-priori error bounds and float32 stand-ins for the back half's kernels that are no conv: the harmonic
source's phase chain, the STFT pair in both variants, the iSTFT head and the up-sampling pool (kernels_misc.hip).

Three things per kernel, shared by tests/test_head_kernels_cpu.py (no GPU) and tests/test_gpu_head_kernels.py:
  * a reference written from the definition in vectorised float64 numpy / torch (exact tables, no kernel-shaped indexing);
  * a bound per output element, derived from the operation count and the precision of float32 alone (u = 2^-24; an n-term
    float32 dot product is within gamma(n) sum |terms| of the exact one in any order of summation, with or without fused
    multiply-adds) plus, where a library function is involved, an allowance of 2 ulp per call (the precedent of
    tests/test_gpu_conv_options.py), taken as 2 * 2^-23 |value|.  No figure in here was fitted to what a kernel returns;
  * a float32 numpy stand-in of the kernel with its operation order, which must itself pass the bound -- and whose mutations
    (the ways the kernel could be wrong) must not.  That is the proof that the GPU tests can fail.
"""
import numpy as np
import torch
import torch.nn.functional as F

from .kokoro_ref import dft_tables, gauss_noise, hann_periodic

U = 2.0 ** -24            # unit roundoff of float32
ULP2 = 2 * 2.0 ** -23     # 2 ulp of a float32 result v are at most ULP2 * |v|
PI32 = np.float32(np.pi)  # 3.14159274101257324f: the largest phase the forward kernel may return
EPS_ONNX = 1e-14          # variant 0: the epsilon under the root of the magnitude
SENT = np.float32(-12345.5)


def gamma(n):
    """Higham's gamma_n: the relative error bound of n chained float32 roundings."""
    return n * U / (1.0 - n * U)


def frac(err, bound):
    """max over elements of err / bound (0 / 0 = 0, anything else over 0 = inf; NaN anywhere = inf)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.inf) if np.isnan(f).any() else float(f.max())


# ---- tables (exact: float64, cos / sin exact at the quadrant angles as init_dft_tables has them) ---------------------------------
def _tables():
    c, s = dft_tables(20)
    win = hann_periodic(20)
    n, k = np.arange(20), np.arange(11)
    m = (k[:, None] * n[None, :]) % 20
    fwd_re = win[None] * c[m]            # [11, 20]
    fwd_im = win[None] * (-s[m])
    ck = np.where((k == 0) | (k == 10), 1.0, 2.0)
    inv = {0: ((c[m.T] / 20.0) * win[:, None], (-s[m.T] / 20.0) * win[:, None])}   # [20, 11] each
    im1 = (-ck[None] * s[m.T]) / 20.0 * win[:, None]
    im1[:, 0] = 0.0
    im1[:, 10] = 0.0
    inv[1] = ((ck[None] * c[m.T]) / 20.0 * win[:, None], im1)
    return fwd_re, fwd_im, inv, win * win


FWD_RE, FWD_IM, INV, WIN_SQ = _tables()


# ---- forward STFT ----------------------------------------------------------------------------------------------------------------
def stft_ref(x):
    """x [L] (L a multiple of 5) -> (re, im, are, aim), each [11, L/5 + 1] float64: the windowed 20-point DFT of the centred,
    replicate-padded frames at hop 5 -- torch.stft(x, 20, 5, 20, hann_window(20, periodic=True), center=True,
    pad_mode="replicate"), which both variants share -- and sum |x T| of every sum, which the bounds scale with."""
    x = np.asarray(x, dtype=np.float64)
    xp = np.concatenate([np.full(10, x[0]), x, np.full(10, x[-1])])
    fr = np.lib.stride_tricks.sliding_window_view(xp, 20)[::5]          # [nf, 20]
    return FWD_RE @ fr.T, FWD_IM @ fr.T, np.abs(FWD_RE) @ np.abs(fr.T), np.abs(FWD_IM) @ np.abs(fr.T)


def stft_bounds(x, variant):
    """The reference of stft_kernel on one row and its bounds.  Returns a dict:
      re, im      the exact spectrum; mag = sqrt(re^2 + im^2 [+ 1e-14 in variant 0])
      b_re, b_im  bound on |mag' cos(ph') - re| and |mag' sin(ph') - im| for the kernel's float32 (mag', ph'):
                  gamma(21) sum |x T|  (20 terms and the rounding of the float32 table)
                  + (mag + e2) (6 u + ULP2 pi)  (re^2 + im^2 + eps: three roundings, halved by the root, is 1.5 u; the float32 epsilon
                    another 0.5 u; sqrtf 2 ulp = 4 u.  atan2f 2 ulp of a phase of at most pi turns the vector by ULP2 pi)
                  + (mag - |z|)  (variant 0: the epsilon lengthens the vector)
                  with e2 = the length of the arithmetic bound's vector
      d_mag       bound on |mag' - mag|: e2 + 6 u (mag + e2)   (sqrt(a^2 + eps) is 1-Lipschitz in a)"""
    re, im, are, aim = stft_ref(x)
    e_re, e_im = gamma(21) * are, gamma(21) * aim
    e2 = np.hypot(e_re, e_im)
    z = np.hypot(re, im)
    mag = np.sqrt(re * re + im * im + (EPS_ONNX if variant == 0 else 0.0))
    lib = (mag + e2) * (6 * U + ULP2 * np.pi)
    return {"re": re, "im": im, "mag": mag, "b_re": e_re + lib + (mag - z), "b_im": e_im + lib + (mag - z),
            "d_mag": e2 + 6 * U * (mag + e2)}


def stft_check(mag, ph, x, variant):
    """mag, ph [11, nf] float32 as a kernel returned them for the row x [L] -> the worst error as a fraction of its bound, for
    the real parts, the imaginary parts and the squared magnitudes (rebuilt in float64)."""
    b = stft_bounds(x, variant)
    mag, ph = np.asarray(mag, dtype=np.float64), np.asarray(ph, dtype=np.float64)
    assert mag.shape == b["re"].shape and ph.shape == b["re"].shape
    return {"re": frac(np.abs(mag * np.cos(ph) - b["re"]), b["b_re"]),
            "im": frac(np.abs(mag * np.sin(ph) - b["im"]), b["b_im"]),
            "mag2": frac(np.abs(mag * mag - b["mag"] ** 2), (mag + b["mag"]) * b["d_mag"])}


def stft_f32(row, L, variant, clamp=None, shift=10):
    """Float32 stand-in of stft_kernel on one row of a batch: row [stride] holds L valid samples (whatever follows them is the
    batch's: NaN in the hooks).  Sequential float32 sums over the 20 taps, float32 root and atan2.  Mutations: clamp = the index
    the frames are clamped to (the kernel: L - 1), shift = the centre offset (the kernel: p = 5 f - 10 + n)."""
    row = np.asarray(row, dtype=np.float32)
    nf = L // 5 + 1
    hi = L - 1 if clamp is None else clamp
    idx = np.clip(5 * np.arange(nf)[:, None] - shift + np.arange(20)[None, :], 0, hi)
    X = row[idx]                                                        # [nf, 20]
    tre, tim = FWD_RE.astype(np.float32), FWD_IM.astype(np.float32)
    re = np.zeros((11, nf), dtype=np.float32)
    im = np.zeros((11, nf), dtype=np.float32)
    for n in range(20):                                                 # (over taps, not samples)
        re = re + tre[:, n:n + 1] * X[None, :, n]
        im = im + tim[:, n:n + 1] * X[None, :, n]
    if variant == 0:
        mag = np.sqrt(re * re + im * im + np.float32(1e-14))
        ph = np.where((im == 0) & (re < 0), PI32, np.arctan2(im, re))
    else:
        mag = np.sqrt(re * re + im * im)
        ph = np.arctan2(im, re)
    assert mag.dtype == np.float32 and ph.dtype == np.float32
    return mag, ph


# ---- iSTFT head ------------------------------------------------------------------------------------------------------------------
def spec_bounds(logmag, phl):
    """The reference of istft_spec_kernel on float32 logits: mag = exp(a), re = mag cos(sin(b)), im = mag sin(sin(b)), and the bound
    13 u mag on either: expf 2 ulp (4 u mag); sinf(b) 2 ulp of a value of at most 1 moves the angle by 4 u, the outer function by
    no more; cosf / sinf of the angle 2 ulp (4 u); the product 1 u."""
    a, b = np.asarray(logmag, dtype=np.float64), np.asarray(phl, dtype=np.float64)
    mag, ang = np.exp(a), np.sin(b)
    return mag * np.cos(ang), mag * np.sin(ang), 13 * U * mag


def spec_check(spec_re, spec_im, logmag, phl):
    re, im, bound = spec_bounds(logmag, phl)
    return {"spec_re": frac(np.abs(np.asarray(spec_re, dtype=np.float64) - re), bound),
            "spec_im": frac(np.abs(np.asarray(spec_im, dtype=np.float64) - im), bound)}


def spec_f32(logmag, phl):
    a, b = np.asarray(logmag, dtype=np.float32), np.asarray(phl, dtype=np.float32)
    mag, ang = np.exp(a), np.sin(b)
    return mag * np.cos(ang), mag * np.sin(ang)


def istft_ref(re, im, variant):
    """re, im [11, nf] -> (audio, A), each [5 (nf - 1)] float64.  Variant 1: torch.istft(spec, 20, 5, 20, hann_window(20,
    periodic=True), center=True) -- the one-sided inverse DFT of every frame (interior bins doubled, the imaginary parts of bins 0
    and 10 ignored), windowed, overlap-added, divided by the overlap-added squared window, the centre padding trimmed.  Variant 0:
    the oracle's `istft`: every bin once, real - imag, no division.  A = the same sums over |coefficient * value| (in variant 1
    divided by the envelope as well): what the bound scales with."""
    re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
    nf = re.shape[1]
    cre, cim = INV[variant]
    y = cre @ re + cim @ im                                             # [20, nf]
    a = np.abs(cre) @ np.abs(re) + np.abs(cim) @ np.abs(im)
    total = 5 * (nf - 1) + 20
    out, A, env = np.zeros(total), np.zeros(total), np.zeros(total)
    for n in range(20):                                                 # (over taps, not samples)
        out[n: n + 5 * nf: 5] += y[n]
        A[n: n + 5 * nf: 5] += a[n]
        env[n: n + 5 * nf: 5] += WIN_SQ[n]
    keep = slice(10, 10 + 5 * (nf - 1))  # (the centre padding trimmed; the envelope's one zero lies in front of it)
    if variant == 1:
        return out[keep] / env[keep], A[keep] / env[keep]
    return out[keep], A[keep]


def istft_rel_bound(variant):
    """What istft_ola_kernel may be off by, relative to A: 22 terms per frame (gamma(22) in any order), the rounding of the float32
    table (1), the sum over up to 4 frames (4); variant 1 adds the division (1) and the envelope (a sum of 4 rounded float32
    squares of the window: 4)."""
    return gamma(27) if variant == 0 else gamma(32)


def istft_edges(nf):
    """The samples where istft_ola_kernel can go wrong alone, by name: the first ten reach back only to frame 0, the last hop is cut
    at frame nf - 1, and hop 256 (sample 1280) is the first of a second block with its own staged window (from 361 frames on)."""
    ns = 5 * (nf - 1)
    e = {"first ten samples": np.arange(0, min(10, ns)), "last hop": np.arange(ns - 5, ns)}
    if ns > 1280:
        e["block seam at sample 1280"] = np.arange(1270, min(1290, ns))
    return e


def istft_check(audio, re, im, variant):
    """audio [5 (nf - 1)] float32 as a kernel returned it for the float32 spectrum (re, im) -> the worst error as a fraction of its
    bound, over the whole row and over each named edge."""
    ref, A = istft_ref(re, im, variant)
    err, bound = np.abs(np.asarray(audio, dtype=np.float64) - ref), istft_rel_bound(variant) * A
    out = {"audio": frac(err, bound)}
    for name, idx in istft_edges(np.asarray(re).shape[1]).items():
        out[name] = frac(err[idx], bound[idx])
    return out


def istft_f32(re, im, variant, table_variant=None, divide=None, drop=None):
    """Float32 stand-in of istft_ola_kernel: per sample the frames q + 2 .. q - 1 of its hop q in descending order, the bins in
    ascending order.  Mutations: table_variant = (variant of the real table, variant of the imaginary table) other than the
    kernel's; divide = whether the envelope divides; drop = "hi" / "lo": a staged window one frame short, so that the last hop of a
    256-hop block loses frame q + 2 / the first hop of a later block loses frame q - 1."""
    re, im = np.asarray(re, dtype=np.float32), np.asarray(im, dtype=np.float32)
    nf = re.shape[1]
    ns = 5 * (nf - 1)
    tv = (variant, variant) if table_variant is None else table_variant
    cre, cim = INV[tv[0]][0].astype(np.float32), INV[tv[1]][1].astype(np.float32)
    wsq = WIN_SQ.astype(np.float32)
    j = np.arange(ns)
    q, s5 = j // 5, j % 5
    y = np.zeros(ns, dtype=np.float32)
    env = np.zeros(ns, dtype=np.float32)
    for df in (3, 2, 1, 0):
        f = q - 1 + df
        ok = (f >= 0) & (f <= nf - 1)
        if drop == "hi" and df == 3:
            ok &= (q % 256) != 255
        if drop == "lo" and df == 0:
            ok &= ~((q % 256 == 0) & (q > 0))
        fc = np.clip(f, 0, nf - 1)
        m = 5 * (3 - df) + s5
        acc = np.zeros(ns, dtype=np.float32)
        for k in range(11):
            acc = acc + (cre[m, k] * re[k, fc] + cim[m, k] * im[k, fc])
        y = np.where(ok, y + acc, y)
        env = np.where(ok, env + wsq[m], env)
    assert y.dtype == np.float32 and env.dtype == np.float32
    return y / env if (variant == 1 if divide is None else divide) else y


# ---- up-sampling pool ------------------------------------------------------------------------------------------------------------
def pool_ref(x, mean, scale, shift, w, bias, slope):
    """One utterance: x [C, L], mean / scale / shift / bias [C], w [C, 3], all float32 -> (y, bound), each [C, 2 L] float64:
    F.conv_transpose1d(groups=C, stride=2, padding=1, output_padding=1) of leaky((x - mean) scale + shift) in float64, and
    gamma(7) sum V |w| + u |bias| with V = |x - mean| |scale| + |shift| >= |v| -- a value goes through the subtraction, the
    scaling, the shift, the slope, its tap, the sum of the two taps and the bias: seven roundings; the bias through one."""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    x, mean, scale, shift, w, bias = t(x), t(mean), t(scale), t(shift), t(w), t(bias)
    C = x.shape[0]
    v = F.leaky_relu((x - mean[:, None]) * scale[:, None] + shift[:, None], float(np.float32(slope)))
    kw = dict(stride=2, padding=1, output_padding=1, groups=C)
    y = F.conv_transpose1d(v[None], w.reshape(C, 1, 3), bias, **kw)[0]
    V = (x - mean[:, None]).abs() * scale.abs()[:, None] + shift.abs()[:, None]
    s = F.conv_transpose1d(V[None], w.abs().reshape(C, 1, 3), None, **kw)[0]
    return y.numpy(), (gamma(7) * s + U * bias.abs()[:, None]).numpy()


def pool_check(y, x, mean, scale, shift, w, bias, slope):
    ref, bound = pool_ref(x, mean, scale, shift, w, bias, slope)
    return {"pool": frac(np.abs(np.asarray(y, dtype=np.float64) - ref), bound)}


def pool_f32(row, L, mean, scale, shift, w, bias, slope, swap=False, read_past=False):
    """Float32 stand-in of pool_up2_kernel on one utterance of a batch: row [C, stride] holds L valid columns (NaN behind them in
    the hooks).  Mutations: swap = w0 and w2 exchanged; read_past = v[m + 1] read at m = L - 1 as well."""
    f = np.float32
    row, w = np.asarray(row, dtype=f), np.asarray(w, dtype=f)
    mu, sc, sh, bi = (np.asarray(a, dtype=f)[:, None] for a in (mean, scale, shift, bias))
    v = (row[:, :L + 1] - mu) * sc + sh
    v = np.where(v > 0, v, v * f(slope))
    v0, v1 = v[:, :L], v[:, 1:L + 1].copy()
    if not read_past:
        v1[:, L - 1] = 0
    w0, w1, w2 = (w[:, i:i + 1] for i in ((2, 1, 0) if swap else (0, 1, 2)))
    y = np.empty((row.shape[0], 2 * L), dtype=f)
    y[:, 0::2] = v0 * w1 + bi
    y[:, 1::2] = (v0 * w2 + v1 * w0) + bi
    return y


# ---- harmonic source: the phase chain --------------------------------------------------------------------------------------------
SRC_CH = 1024  # steps per chunk of source_phase_kernel


def cumsum_chunked(rad, restart=False, carry32=False):
    """Float32 stand-in of source_phase_kernel's running sums: rad [1, 9, n] float32 -> [1, 9, n] float32, a float64 sum over the
    steps in order, rounded to float32 per step, carried from one chunk of SRC_CH steps to the next.  Mutations: restart = the sum
    starts at 0 in every chunk; carry32 = it crosses a seam as a float32."""
    r = rad.numpy().astype(np.float64)
    out = np.empty_like(r)
    cs = np.zeros(r.shape[:2] + (1,))
    for base in range(0, r.shape[2], SRC_CH):                           # (over chunks, not steps)
        run = np.cumsum(np.concatenate([cs, r[:, :, base: base + SRC_CH]], axis=2), axis=2)[:, :, 1:]
        out[:, :, base: base + SRC_CH] = run
        cs = run[:, :, -1:]
        if restart:
            cs = np.zeros_like(cs)
        if carry32:
            cs = cs.astype(np.float32).astype(np.float64)
    return torch.from_numpy(out.astype(np.float32))


def source_with_cumsum(oracle, f0_curve, seed, utt, noise_scale, cumsum=None):
    """KokoroOracle.source restated with the running sum as a parameter (None: torch.cumsum, and then the same bits as the
    oracle's own -- tests/test_head_kernels_cpu.py asserts it)."""
    dt = oracle.dt
    f0 = F.interpolate(f0_curve[None, None], scale_factor=300, mode="nearest")[0, 0]
    L = f0.shape[0]
    fn = f0[:, None] * torch.arange(1, 10, dtype=dt)[None, :]
    rad = F.interpolate(((fn / 24000) % 1).T[None], scale_factor=1 / 300, mode="linear")
    run = torch.cumsum(rad, dim=2) if cumsum is None else cumsum(rad)
    phase = F.interpolate(run * 2 * np.pi * 300, scale_factor=300, mode="linear")[0].T
    sines = torch.sin(phase) * 0.1
    uv = (f0 > 10).to(dt)[:, None]
    noise_amp = uv * 0.003 + (1 - uv) * 0.1 / 3
    noise = noise_amp * torch.from_numpy(gauss_noise(seed, utt, L)).to(dt) * noise_scale if noise_scale != 0.0 else torch.zeros_like(sines)
    w = oracle.w
    return torch.tanh(F.linear(sines * uv + noise, w["decoder.generator.m_source.l_linear.weight"],
                               w["decoder.generator.m_source.l_linear.bias"]))[:, 0]


# ---- the inputs both test files draw ---------------------------------------------------------------------------------------------
def stft_rows(frames, kind, seed):
    """The input rows of the forward tests, by kind, padded to the longest with NaN as the hook pads them."""
    rng = np.random.default_rng(seed)
    rows = np.full((len(frames), 600 * max(frames) + 7), np.nan, dtype=np.float32)
    for b, f in enumerate(frames):
        x = rng.standard_normal(600 * f)
        if kind == "small":
            x *= 1e-3
        if kind == "edges":  # the first and last 15 samples large: the replicate padding dominates frames 0, 1, nf - 2, nf - 1
            x[:15] += 40.0 * np.sign(x[:15])
            x[-15:] += 40.0 * np.sign(x[-15:])
        rows[b, :600 * f] = x
    return rows


def head_logits(frames, seed):
    rng = np.random.default_rng(seed)
    nf = 120 * max(frames) + 1
    cp = np.empty((len(frames), 22, nf), dtype=np.float32)
    cp[:, :11] = rng.uniform(-6.0, 2.0, (len(frames), 11, nf))
    cp[:, 11:] = rng.uniform(-20.0, 20.0, (len(frames), 11, nf))
    return cp


def pool_case(seed=30):
    """The pool case of both files: B = 3, C = 5, lens (1, 128, 129); pre-activations of both signs."""
    rng = np.random.default_rng(seed)
    B, C, L = 3, 5, 129
    x = rng.standard_normal((B, C, L)).astype(np.float32) * 2 + 0.5
    norm = np.stack([rng.standard_normal((B, C)) * 0.3 + 0.5, 0.5 + rng.random((B, C)) * 1.5, rng.standard_normal((B, C)) * 0.4]).astype(np.float32)
    norm[1, :, 1] *= -1  # (a negative scale)
    w = rng.standard_normal((C, 3)).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    return x, (1, 128, 129), norm, w, bias, np.float32(0.2)
