"""Host-side mirror of the reference's `OrtKoko` over the kokorox_hip C ABI (ctypes).

Reference interface being mirrored (/root/reference/kokorox/src/onn/ort_koko.rs):
    OrtKoko::new(model_path: String) -> Result<Self, String>                      (l.31-35)
    OrtKoko::infer(&self, tokens: Vec<Vec<i64>>, styles: Vec<Vec<f32>>, speed: f32)
        -> Result<ArrayBase<OwnedRepr<f32>, IxDyn>, Box<dyn Error>>               (l.37-91)
`HipKoko.new` / `HipKoko.infer` keep the names, argument meaning and error behaviour
(load failure and infer failure raise; an empty token list is an error instead of the
reference's index panic at l.56).  There is NO CPU fallback: if libkokorox_hip.so is
missing or no gfx950 device is visible, construction fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libkokorox_hip.so")

PACK_F32_MONO, PACK_F32_STEREO, PACK_PCM16_MONO = 0, 1, 2
PACK_WAV_F32, PACK_WAV16_BASE64 = 3, 4  # the servers' bodies (infer_requests / submit_request only): float WAV, base64 of a 16-bit WAV
PACK_MULAW, PACK_ALAW = 8, 9  # raw G.711, one byte per sample (infer_requests / submit_request only)
PACK_FLAC = 12  # a lossless FLAC body of the 16-bit samples (infer_requests / submit_request only); its size follows from the samples
# (infer_requests / submit_request only) a WAV file of 4-bit IMA ADPCM, the form's number being the WAV tag it carries, and the plain
# 16-bit WAV file that PACK_WAV16_BASE64 encodes, as bytes
PACK_ADPCM_WAV, PACK_WAV16 = 17, 18
ADPCM_MAX_BLOCK = 1024
# the output sample rate, or'ed into the form of infer_requests / submit_request (the format word of include/kokorox_hip.h)
PACK_RATE_24000, PACK_RATE_8000, PACK_RATE_16000, PACK_RATE_48000 = 0x000, 0x100, 0x200, 0x300
RATE_HZ = {0: 24000, 1: 8000, 2: 16000, 3: 48000}  # by rate code (bits 8..11 of the word)
RESAMPLE_MAX_TAPS = 145
# joins (include/kokorox_hip.h, "joins"): a spec is (flags, keep_ms, pause_ms, fade_ms), the layout of kx_join
JOIN_TRIM_HEAD, JOIN_TRIM_TAIL, JOIN_TRIM_INNER = 1, 2, 4
JOIN_DTYPE = np.dtype([("flags", "<u4"), ("keep_ms", "<i4"), ("pause_ms", "<i4"), ("fade_ms", "<i4")])
JOIN_NONE = (0, 0, 0, 0)
# levels (include/kokorox_hip.h, "levels"): a spec is (mode, gain, peak), the layout of kx_level
LEVEL_GAIN, LEVEL_NORMALIZE, LEVEL_CEILING = 0, 1, 2
LEVEL_DTYPE = np.dtype([("mode", "<u4"), ("gain", "<f4"), ("peak", "<f4")])
LEVEL_PLAIN = (LEVEL_GAIN, 1.0, 0.0)
PEAK_TRUE = 0x100  # OR-ed into a level or a loudness mode: p is the true peak tp (KX_PEAK_TRUE)
# pieces (include/kokorox_hip.h, "pieces"): the flag bits of a piece, and the layout of kx_piece_carry
PIECE_FIRST, PIECE_LAST, PIECE_WHOLE = 1, 2, 3
PIECE_TAIL = 256
PIECE_MAGIC = 0x4350584B
PIECE_CARRY_DTYPE = np.dtype([("magic", "<u4"), ("format_word", "<u4"), ("src_samples", "<i8"), ("out_samples", "<i8"), ("n_tail", "<i4"),
                              ("reserved", "<i4"), ("tail", "<f4", (PIECE_TAIL,))])
# loudness (include/kokorox_hip.h, "loudness"): a spec is (mode, target_lufs, peak), the layout of kx_loudness
LOUDNESS_MEASURE, LOUDNESS_NORMALIZE = 0, 1
LOUDNESS_DTYPE = np.dtype([("mode", "<u4"), ("target_lufs", "<f4"), ("peak", "<f4")])
LOUDNESS_METER = (LOUDNESS_MEASURE, 0.0, 0.0)
LOUDNESS_NONE = (0xFFFFFFFF, 0.0, 0.0)  # the test hook only: a request beside metered ones that is not metered
# limiter (include/kokorox_hip.h, "limiter"): a spec is (mode, gain, target_lufs, peak), the layout of kx_limit
LIMIT_GAIN, LIMIT_LOUDNESS = 0, 1
LIMIT_MAX_TAPS = 481
LIMIT_DTYPE = np.dtype([("mode", "<u4"), ("gain", "<f4"), ("target_lufs", "<f4"), ("peak", "<f4")])
LIMIT_NONE = (0xFFFFFFFF, 1.0, 0.0, 1.0)  # the test hook only: a request beside limited ones that has no limiter
KX_OK, KX_ERR_INVALID, KX_ERR_IO, KX_ERR_DEVICE, KX_ERR_STATE = 0, 1, 2, 3, 4  # include/kokorox_hip.h
KX_FLAG_NOISE_OFF = 1
KX_FLAG_TAPS = 2
STYLE_DIM = 256
SAMPLES_PER_FRAME = 600

_lib = None


class KokoroxHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"kokorox_hip error {code}: {msg}")
        self.code = code


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libkokorox_hip.so (built by kokorox_amd.build / __graft_entry__.build())."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    import sys
    p = path or os.environ.get("KX_LIB") or LIB_PATH
    # torch wheels bundle their own libamdhip64; if this library (linked against /opt/rocm's) is loaded first
    # and torch later, the process ends up with two HIP runtimes and torch sees no GPU.  Loading torch first
    # makes both share one runtime.  Processes that never use torch (the C++ host) are unaffected.
    import sys
    if "torch" not in sys.modules and os.environ.get("KX_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.exists(p) and p == LIB_PATH and os.environ.get("KX_NO_AUTOBUILD") != "1":
        # the prebuilt library normally travels with the tree; as a last resort build it here (hipcc, ~2-3 min)
        try:
            from . import build as _build
            _build.build_library(verbose=True)
        except Exception as e:  # fall through to the loud error below
            print(f"kokorox_amd: building libkokorox_hip.so failed: {e}", file=sys.stderr)
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} is missing: build it with `python -m kokorox_amd.build` (hipcc, gfx950). "
            "The HIP path has no CPU fallback.")
    lib = C.CDLL(p)
    vp, i32, i64, u32, u64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_float
    cp, sz = C.c_char_p, C.c_size_t
    sig = {
        "kx_version": (cp, []),
        "kx_init": (i32, [i32, cp, sz]),
        "kx_create": (vp, [cp, i32, cp, sz]),
        "kx_import_onnx": (i32, [cp, cp, cp, sz]),
        "kx_resample_filter": (i32, [i32, vp, vp, vp, vp, i32]),
        "kx_warmup": (i32, [vp, i32, i32, i32]),
        "kx_arena_bytes": (i32, [vp, C.POINTER(i64)]),
        "kx_call_times": (i32, [vp, C.POINTER(C.c_double)]),
        "kx_model_status": (i32, [vp, C.POINTER(i64)]),
        "kx_model_info": (i32, [vp, C.POINTER(i64)]),
        "kx_dispatcher_health": (i32, [vp, vp, i32, C.POINTER(i64), C.POINTER(i64)]),
        "kx_create_from_device_blob": (vp, [vp, sz, i32, cp, sz]),
        "kx_destroy": (None, [vp]),
        "kx_last_error": (cp, [vp]),
        "kx_last_error_copy": (i32, [vp, cp, sz]),
        "kx_create_replicas": (i32, [cp, vp, i32, vp, cp, sz]),
        "kx_replicas_times": (i32, [C.POINTER(C.c_double)]),
        "kx_create_partition": (vp, [cp, i32, i32, i32, cp, sz]),
        "kx_infer": (i32, [vp, vp, i64, vp, i32, vp, vp, i32, u64, u32, C.POINTER(C.POINTER(f32)), vp]),
        "kx_free_audio": (None, [C.POINTER(f32)]),
        "kx_infer_device": (i32, [vp, vp, i64, vp, i32, vp, vp, i32, u64, u32, vp, i64, vp, C.POINTER(i64)]),
        "kx_sync": (i32, [vp]),
        "kx_set_pinned_durations": (i32, [vp, vp, i32]),
        "kx_set_utterance_base": (i32, [vp, u64]),
        "kx_set_lanes": (i32, [vp, i32]),
        "kx_set_conv_mode": (i32, [vp, i32]),
        "kx_get_conv_mode": (i32, [vp]),
        "kx_set_stft_variant": (i32, [vp, i32]),
        "kx_get_stft_variant": (i32, [vp]),
        "kx_profile_enable": (i32, [vp, i32]),
        "kx_profile_read": (i32, [vp, C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "kx_profile_detail": (i32, [vp, vp, i64, C.POINTER(i64)]),
        "kx_profile_aux": (i32, [vp, C.POINTER(i64), C.POINTER(C.c_double)]),
        "kx_diag_enable": (i32, [vp, i32]),
        "kx_diag_count": (i32, [vp, C.POINTER(i64)]),
        "kx_diag_get": (i32, [vp, i64, cp, sz, vp]),
        "kx_set_act_prescale": (i32, [vp, cp, i32]),
        "kx_set_voice_table": (i32, [vp, vp, i32]),
        "kx_infer_voices": (i32, [vp, vp, i64, vp, i32, vp, vp, i32, vp, i32, u64, u32, i32, C.POINTER(vp), vp, vp]),
        "kx_infer_packed": (i32, [vp, vp, i64, vp, i32, vp, vp, i32, u64, u32, i32, C.POINTER(vp), vp, vp]),
        "kx_free_packed": (None, [vp]),
        "kx_infer_requests": (i32, [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, u64, u32, vp, i32, C.POINTER(vp), vp, vp]),
        "kx_dispatcher_submit_request": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, f32, u64, i32, C.POINTER(vp), C.POINTER(i64),
                                               C.POINTER(i64), cp, sz]),
        "kx_infer_requests_marks": (i32, [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, u64, u32, vp, i32, C.POINTER(vp), vp, vp,
                                          C.POINTER(vp), vp]),
        "kx_dispatcher_submit_request_marks": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, f32, u64, i32, C.POINTER(vp), C.POINTER(i64),
                                                     C.POINTER(i64), C.POINTER(vp), C.POINTER(i64), cp, sz]),
        "kx_infer_requests_joined": (i32, [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, u64, u32, vp, i32, C.POINTER(vp), vp, vp,
                                           vp, vp, vp, i32]),
        "kx_dispatcher_submit_request_joined": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, f32, u64, i32, C.POINTER(vp), C.POINTER(i64),
                                                      C.POINTER(i64), vp, vp, vp, cp, sz]),
        "kx_infer_requests_levelled": (i32, [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, u64, u32, vp, i32, C.POINTER(vp), vp, vp,
                                             vp, vp, vp, i32, vp, i32, vp]),
        "kx_dispatcher_submit_request_levelled": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, f32, u64, i32, C.POINTER(vp), C.POINTER(i64),
                                                        C.POINTER(i64), vp, vp, vp, vp, vp, cp, sz]),
        "kx_infer_requests_pieces": (i32, [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, u64, u32, vp, i32, C.POINTER(vp), vp, vp,
                                           vp, vp, vp, i32, vp, i32, vp, vp, vp, vp]),
        "kx_dispatcher_submit_request_piece": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, f32, u64, i32, C.POINTER(vp), C.POINTER(i64),
                                                     C.POINTER(i64), vp, vp, vp, vp, vp, u32, vp, vp, cp, sz]),
        "kx_loudness_filter": (i32, [i32, vp]),
        "kx_truepeak_filter": (i32, [vp, i32]),
        "kx_adpcm_block": (i32, [i32, vp, vp]),
        "kx_infer_requests_loudness": (i32, [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, u64, u32, vp, i32, C.POINTER(vp), vp, vp,
                                             vp, vp, vp, i32, vp, i32, vp]),
        "kx_dispatcher_submit_request_loudness": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, f32, u64, i32, C.POINTER(vp), C.POINTER(i64),
                                                        C.POINTER(i64), vp, vp, vp, vp, vp, cp, sz]),
        "kx_limit_filter": (i32, [i32, vp, vp, i32]),
        "kx_infer_requests_limited": (i32, [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, u64, u32, vp, i32, C.POINTER(vp), vp, vp,
                                            vp, vp, vp, i32, vp, i32, vp]),
        "kx_dispatcher_submit_request_limited": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, f32, u64, i32, C.POINTER(vp), C.POINTER(i64),
                                                       C.POINTER(i64), vp, vp, vp, vp, vp, cp, sz]),
        "kx_infer_prosody": (i32, [vp, vp, i64, vp, i32, vp, vp, i32, u64, u32, C.POINTER(C.POINTER(f32)), vp, vp, vp]),
        "kx_infer_requests_prosody": (i32, [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, u64, u32, vp, i32, C.POINTER(vp), vp, vp,
                                            vp, vp, vp, i32, vp, vp, vp]),
        "kx_dispatcher_submit_request_prosody": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, f32, u64, i32, C.POINTER(vp), C.POINTER(i64),
                                                       C.POINTER(i64), vp, vp, vp, vp, vp, vp, cp, sz]),
        "kx_infer_requests_fitted": (i32, [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, u64, u32, vp, i32, C.POINTER(vp), vp, vp,
                                           vp, vp, vp, i32, vp, vp, vp, vp, i32, vp]),
        "kx_dispatcher_submit_request_fitted": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, f32, u64, i32, C.POINTER(vp), C.POINTER(i64),
                                                      C.POINTER(i64), vp, vp, vp, vp, vp, vp, vp, i32, vp, cp, sz]),
        "kx_dispatcher_create": (vp, [vp, i32, i32, i32, cp, sz]),
        "kx_dispatcher_create_warm": (vp, [vp, i32, i32, i32, i32, i32, cp, sz]),
        "kx_dispatcher_submit": (i32, [vp, vp, i32, vp, f32, u64, C.POINTER(C.POINTER(f32)), C.POINTER(i64), cp, sz]),
        "kx_dispatcher_submit_ex": (i32, [vp, vp, i32, vp, vp, vp, i32, f32, u64, i32, C.POINTER(vp), C.POINTER(i64),
                                          C.POINTER(i64), cp, sz]),
        "kx_dispatcher_stats": (i32, [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
        "kx_dispatcher_model_batches": (i32, [vp, vp, i32]),
        "kx_dispatcher_failures": (i32, [vp, C.POINTER(i64), C.POINTER(i64)]),
        "kx_dispatcher_destroy": (None, [vp]),
        "kx_debug_tap": (i32, [vp, cp, i32, vp, i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here = the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


TEST_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libkokorox_hip_test.so")
_test_lib = None


def _test_signatures():
    """Every hook of include/kokorox_hip_test.h, once: name -> (result, argument types)."""
    vp, i32, i64, u32, u64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_float
    cp, sz = C.c_char_p, C.c_size_t
    return {
        "kx_test_conv": (i32, [vp, cp, sz]),
        "kx_test_lstm": (i32, [i32, vp, i32, i32, i32] + [vp] * 9 + [cp, sz]),
        "kx_test_source": (i32, [i32, vp, i32, i32, vp, f32, u64, u64, i32, vp, cp, sz]),
        "kx_test_attention": (i32, [i32, vp, vp, i32, i32, vp, cp, sz]),
        "kx_test_lstm_fault": (i32, [i32]),
        "kx_test_lstm_parts": (i32, [i32]),
        "kx_test_conv_plan": (i32, [vp, i32, vp, i32, cp, sz]),
        "kx_test_layernorm": (i32, [i32, vp, i32, i32, i32, vp, f32, i32, vp, vp, f32, vp, cp, sz]),
        "kx_test_instance_norm": (i32, [i32, vp, i32, i32, i32, vp, vp, vp, cp, sz]),
        "kx_test_output_plan": (i32, [i32, vp, i32, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, cp, sz]),
        "kx_test_output_plan_levelled": (i32, [i32, vp, i32, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp,
                                               cp, sz]),
        "kx_test_output_plan_loudness": (i32, [i32, vp, i32, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp,
                                               vp, vp, vp, i64, vp, cp, sz]),
        "kx_test_output_plan_limited": (i32, [i32, vp, i32, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp,
                                              vp, vp, vp, i64, vp, vp, vp, cp, sz]),
        "kx_test_output_plan_flac": (i32, [i32, vp, i32, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp,
                                           vp, vp, vp, i64, vp, vp, vp, vp, cp, sz]),
        "kx_test_output_plan_pieces": (i32, [i32, vp, i32, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp,
                                             vp, vp, vp, vp, vp, cp, sz]),
        "kx_test_lstm_ragged": (i32, [i32, vp, vp, i32, i32, i32] + [vp] * 8 + [i32, i32, u32, vp, cp, sz]),
        "kx_test_alignment": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, i32, vp, i32, i32, vp, vp, vp, vp, i32, vp, cp, sz]),
        "kx_test_prosody_durations": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, cp, sz]),
        "kx_test_fit_durations": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, i32, vp, i32, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp,
                                        cp, sz]),
        "kx_test_prosody_curves": (i32, [i32, vp, vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, cp, sz]),
        "kx_test_embed": (i32, [i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, cp, sz]),
        "kx_test_style_fc": (i32, [i32, vp, i32, vp, vp, vp, vp, i32, vp, cp, sz]),
        "kx_test_rows": (i32, [i32, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, cp, sz]),
        "kx_test_source_ragged": (i32, [i32, vp, vp, i32, i32, vp, f32, u64, u64, vp, vp, i32, vp, cp, sz]),
        "kx_test_stft": (i32, [i32, vp, i32, i32, vp, i32, i32, vp, cp, sz]),
        "kx_test_istft_head": (i32, [i32, vp, i32, vp, i32, i32, vp, vp, cp, sz]),
        "kx_test_pool_up2": (i32, [i32, vp, i32, i32, i32, vp, vp, i32, vp, vp, f32, vp, cp, sz]),
        "kx_test_weight_images": (i32, [i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, cp, sz]),
    }


def load_test_library() -> C.CDLL:
    """dlopen libkokorox_hip_test.so: the stand-alone kernel hooks of tests/ (include/kokorox_hip_test.h).  It links against
    libkokorox_hip.so, which is loaded first (same torch-first rule)."""
    global _test_lib
    if _test_lib is not None:
        return _test_lib
    load_library()
    p = os.environ.get("KX_TEST_LIB") or TEST_LIB_PATH
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} is missing: build it with `python -m kokorox_amd.build` (hipcc, gfx950)")
    lib = C.CDLL(p)
    for name, (res, args) in _test_signatures().items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _test_lib = lib
    return lib


TEST_ABI_SYMBOLS = list(_test_signatures())

ABI_SYMBOLS = [
    "kx_version", "kx_init", "kx_create", "kx_import_onnx", "kx_resample_filter", "kx_create_from_device_blob", "kx_create_replicas", "kx_replicas_times", "kx_create_partition", "kx_destroy",
    "kx_last_error", "kx_last_error_copy", "kx_infer",
    "kx_free_audio", "kx_infer_device", "kx_sync", "kx_set_pinned_durations", "kx_warmup", "kx_arena_bytes", "kx_call_times", "kx_model_status", "kx_model_info", "kx_dispatcher_health", "kx_set_utterance_base", "kx_set_lanes",
    "kx_set_conv_mode", "kx_get_conv_mode", "kx_set_stft_variant", "kx_get_stft_variant",
    "kx_profile_enable", "kx_profile_read", "kx_profile_detail", "kx_profile_aux", "kx_diag_enable", "kx_diag_count", "kx_diag_get", "kx_set_act_prescale", "kx_set_voice_table", "kx_infer_voices",
    "kx_infer_packed", "kx_free_packed", "kx_infer_requests", "kx_dispatcher_submit_request", "kx_infer_requests_marks", "kx_dispatcher_submit_request_marks", "kx_infer_requests_joined", "kx_dispatcher_submit_request_joined", "kx_infer_requests_levelled", "kx_dispatcher_submit_request_levelled", "kx_infer_requests_pieces", "kx_dispatcher_submit_request_piece", "kx_loudness_filter", "kx_truepeak_filter", "kx_adpcm_block", "kx_infer_requests_loudness", "kx_dispatcher_submit_request_loudness", "kx_limit_filter", "kx_infer_requests_limited", "kx_dispatcher_submit_request_limited", "kx_infer_prosody", "kx_infer_requests_prosody", "kx_dispatcher_submit_request_prosody", "kx_infer_requests_fitted", "kx_dispatcher_submit_request_fitted", "kx_dispatcher_create", "kx_dispatcher_create_warm", "kx_dispatcher_submit", "kx_dispatcher_submit_ex", "kx_dispatcher_model_batches",
    "kx_dispatcher_stats", "kx_dispatcher_failures", "kx_dispatcher_destroy", "kx_debug_tap",
]


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a) -> Optional[np.ndarray]:
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


class Prosody(C.Structure):
    """kx_prosody (include/kokorox_hip.h, "prosody"): four pointers, each null or [B, t_stride] laid out as the ids."""
    _fields_ = [("rate", C.c_void_p), ("frames", C.c_void_p), ("pitch", C.c_void_p), ("energy", C.c_void_p)]


def prosody_arrays(prosody, lens, stride):
    """`prosody` = (rate, frames, pitch, energy), each None or one sequence per row (its tokens' values), as the [B, stride] arrays
    the library takes -- neutral (1, 0, 1, 1) where a row is shorter than the stride -- and the kx_prosody over them.  Returns
    (struct or None, the arrays): keep the arrays alive for as long as the struct is used."""
    if prosody is None:
        return None, ()
    if len(prosody) != 4:
        raise ValueError("prosody: (rate, frames, pitch, energy), each None or one sequence per row")
    arrs = []
    for k, rows in enumerate(prosody):
        if rows is None:
            arrs.append(None)
            continue
        if len(rows) != len(lens):
            raise ValueError("prosody: one sequence per row")
        a = np.zeros((len(lens), stride), np.int32) if k == 1 else np.ones((len(lens), stride), np.float32)
        for b, row in enumerate(rows):
            if len(row) != int(lens[b]):
                raise ValueError("prosody: one value per token")
            a[b, : len(row)] = np.asarray(row, dtype=a.dtype)
        arrs.append(a)
    return Prosody(*[None if a is None else a.ctypes.data for a in arrs]), tuple(arrs)


# kx_fit_span / kx_fit_result (include/kokorox_hip.h, "fit")
FIT_SPAN_DTYPE = np.dtype([("request", np.int32), ("begin", np.int32), ("end", np.int32), ("frames", np.int32)])
FIT_RESULT_DTYPE = np.dtype([("lambda", np.float32), ("n_free", np.int32), ("held_frames", np.int32), ("excess", np.int32)])


def fit_spans(spans) -> np.ndarray:
    """Fit spans as the array of kx_fit_span the library takes: a list of (request, begin, end, frames), or an array of
    FIT_SPAN_DTYPE already."""
    if isinstance(spans, np.ndarray) and spans.dtype == FIT_SPAN_DTYPE:
        return np.ascontiguousarray(spans).reshape(-1)
    a = np.zeros(len(spans), FIT_SPAN_DTYPE)
    for i, s in enumerate(spans):
        a[i] = tuple(int(v) for v in s)
    return a


def join_specs(joins, n=None) -> np.ndarray:
    """Join specs as the array of kx_join the library takes: one (flags, keep_ms, pause_ms, fade_ms) tuple, a list of them, or
    an array of JOIN_DTYPE already.  n: the count expected (a single tuple is repeated)."""
    if isinstance(joins, np.ndarray) and joins.dtype == JOIN_DTYPE:
        a = np.ascontiguousarray(joins).reshape(-1)
    else:
        j = list(joins)
        if len(j) == 4 and all(isinstance(v, (int, np.integer)) for v in j):
            j = [tuple(j)] * (n if n is not None else 1)
        a = np.array([tuple(int(v) for v in t) for t in j], dtype=JOIN_DTYPE)
    if n is not None and a.shape[0] != n:
        raise ValueError(f"{n} join specs are required")
    return a


def level_specs(levels, n=None) -> np.ndarray:
    """Level specs as the array of kx_level the library takes: one (mode, gain, peak) tuple, a list of them, or an array of
    LEVEL_DTYPE already.  n: the count expected (a single tuple is repeated).  A mode may carry PEAK_TRUE (mode | PEAK_TRUE):
    the peak of that request is then its true peak, four times oversampled on the GPU (voices.true_peak)."""
    if isinstance(levels, np.ndarray) and levels.dtype == LEVEL_DTYPE:
        a = np.ascontiguousarray(levels).reshape(-1)
    else:
        lv = list(levels)
        if lv and not isinstance(lv[0], (tuple, list, np.void)):
            lv = [tuple(lv)] * (n or 1)
        a = np.array([(int(m), float(g), float(p)) for m, g, p in lv], dtype=LEVEL_DTYPE)
    if n is not None and a.shape[0] != n:
        raise ValueError(f"{n} level specs are required")
    return a


def loudness_specs(loudness, n=None) -> np.ndarray:
    """Loudness specs as the array of kx_loudness the library takes: one (mode, target_lufs, peak) tuple, a list of them, or an
    array of LOUDNESS_DTYPE already.  n: the count expected (a single tuple is repeated).  A mode may carry PEAK_TRUE, as in
    level_specs: `peak` is then a true-peak ceiling and the reported p the true peak."""
    if isinstance(loudness, np.ndarray) and loudness.dtype == LOUDNESS_DTYPE:
        a = np.ascontiguousarray(loudness).reshape(-1)
    else:
        ld = list(loudness)
        if ld and not isinstance(ld[0], (tuple, list, np.void)):
            ld = [tuple(ld)] * (n or 1)
        a = np.array([(int(m), float(t), float(p)) for m, t, p in ld], dtype=LOUDNESS_DTYPE)
    if n is not None and a.shape[0] != n:
        raise ValueError(f"{n} loudness specs are required")
    return a


def limit_specs(limits, n=None) -> np.ndarray:
    """Limit specs as the array of kx_limit the library takes: one (mode, gain, target_lufs, peak) tuple, a list of them, or an
    array of LIMIT_DTYPE already.  n: the count expected (a single tuple is repeated).  A mode may carry PEAK_TRUE: the envelope
    the limiter follows is then the four-times oversampled one and the reported p the true peak."""
    if isinstance(limits, np.ndarray) and limits.dtype == LIMIT_DTYPE:
        a = np.ascontiguousarray(limits).reshape(-1)
    else:
        lm = list(limits)
        if lm and not isinstance(lm[0], (tuple, list, np.void)):
            lm = [tuple(lm)] * (n or 1)
        a = np.array([(int(m), float(g), float(t), float(p)) for m, g, t, p in lm], dtype=LIMIT_DTYPE)
    if n is not None and a.shape[0] != n:
        raise ValueError(f"{n} limit specs are required")
    return a


def limit_filter(word: int):
    """(W, taps): the limiter's window W = fs / 200 and its 2 W + 1 smoothing weights as float32 at a format word's rate, from
    the library's one table (kx_limit_filter; host only, no GPU)."""
    W = C.c_int32(0)
    taps = np.zeros(LIMIT_MAX_TAPS, dtype=np.float32)
    rc = load_library().kx_limit_filter(int(word), C.byref(W), _ptr(taps), LIMIT_MAX_TAPS)
    if rc != KX_OK:
        raise KokoroxHipError(rc, "unknown output format or sample rate")
    return int(W.value), taps[: 2 * int(W.value) + 1].copy()


def loudness_filter(word: int) -> np.ndarray:
    """The ten float64 K-weighting coefficients of a format word's rate from the library's one table (kx_loudness_filter; host
    only, no GPU): shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2."""
    out = np.zeros(10, dtype=np.float64)
    rc = load_library().kx_loudness_filter(int(word), _ptr(out))
    if rc != KX_OK:
        raise KokoroxHipError(rc, "unknown output format or sample rate")
    return out


def truepeak_filter() -> np.ndarray:
    """The 72 float32 taps of the true-peak interpolator as [3][24], phase 1 first, from the library's one table
    (kx_truepeak_filter; host only)."""
    out = np.zeros((3, 24), dtype=np.float32)
    rc = load_library().kx_truepeak_filter(_ptr(out), out.size)
    if rc != KX_OK:
        raise KokoroxHipError(rc, "kx_truepeak_filter failed")
    return out


def resample_filter(word: int):
    """(L, M, taps) of a format word's rate code from the library's one table (kx_resample_filter; host only, no GPU): the
    ratio of output to input rate and the float32 taps of the FIR.  Rate code 0 gives (1, 1, no taps)."""
    lib = load_library()
    L, M, n = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    taps = np.zeros(RESAMPLE_MAX_TAPS, dtype=np.float32)
    rc = lib.kx_resample_filter(int(word), C.byref(L), C.byref(M), C.byref(n), _ptr(taps), taps.shape[0])
    if rc != KX_OK:
        raise KokoroxHipError(rc, "unknown output format or sample rate")
    return L.value, M.value, taps[: n.value].copy()


def adpcm_block(word: int = 0):
    """(A, P) of PACK_ADPCM_WAV at the rate of a format word: the bytes of a block and the samples it holds (kx_adpcm_block; host
    only)."""
    a, p = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    rc = load_library().kx_adpcm_block(int(word), _ptr(a), _ptr(p))
    if rc != KX_OK:
        raise KokoroxHipError(rc, "kx_adpcm_block: unknown output sample rate")
    return int(a[0]), int(p[0])


def piece_carries(carries, n) -> np.ndarray:
    """n carries as the array of kx_piece_carry the library takes: None (all zeros: what first pieces are given), one record, a list
    of records (None = zeros), or an array of PIECE_CARRY_DTYPE already."""
    if isinstance(carries, np.ndarray) and carries.dtype == PIECE_CARRY_DTYPE:
        a = np.ascontiguousarray(carries).reshape(-1)
    else:
        a = np.zeros(n, PIECE_CARRY_DTYPE)
        for i, c in enumerate([] if carries is None else carries):
            if c is not None:
                a[i] = np.asarray(c, dtype=PIECE_CARRY_DTYPE).reshape(())
    if a.shape[0] != n:
        raise ValueError(f"{n} piece carries are required")
    return a


def _decode_packed(raw: bytes, fmt: int):
    """A request's region as Python hands it out: samples as an array for forms 0..2 and 8 / 9 (uint8), the body as bytes for
    forms 3, 4, 12 (FLAC), 17 (ADPCM WAV) and 18 (16-bit WAV, its zero padding to a multiple of 4 cut off); at the output rate of
    the word."""
    fmt = int(fmt) & 0xFF
    if fmt == PACK_WAV16:  # (the file is as long as its RIFF size says: 8 + that)
        return raw[: 8 + int.from_bytes(raw[4:8], "little")]
    if fmt in (PACK_WAV_F32, PACK_WAV16_BASE64, PACK_FLAC, PACK_ADPCM_WAV):
        return raw
    if fmt in (PACK_MULAW, PACK_ALAW):
        return np.frombuffer(raw, dtype=np.uint8).copy()
    if fmt == PACK_PCM16_MONO:
        return np.frombuffer(raw, dtype=np.int16).copy()
    a = np.frombuffer(raw, dtype=np.float32).copy()
    return a.reshape(-1, 2) if fmt == PACK_F32_STEREO else a


class HipKoko:
    """MI355X-native stand-in for `OrtKoko` (one instance per GPU, calls serialised)."""

    def __init__(self, model_path: str, device: int = 0, _handle=None):
        self._lib = load_library()
        self.device = device
        if _handle is not None:
            self._h = _handle
            return
        err = C.create_string_buffer(512)
        h = self._lib.kx_create(os.fsencode(model_path), device, err, len(err))
        if not h:
            # reference: `.expect("Failed to create Kokoro TTS model")`, koko.rs:572
            raise RuntimeError(f"Failed to create Kokoro TTS model: {err.value.decode()}")
        self._h = h

    # -- reference-shaped API -------------------------------------------------------------
    @classmethod
    def new(cls, model_path: str, device: int = 0) -> "HipKoko":
        return cls(model_path, device)

    @classmethod
    def from_device_blob(cls, data_ptr: int, n_bytes: int, device: int = 0) -> "HipKoko":
        """Build from a weight blob already in this GPU's memory (after the RCCL broadcast)."""
        lib = load_library()
        err = C.create_string_buffer(512)
        h = lib.kx_create_from_device_blob(C.c_void_p(data_ptr), n_bytes, device, err, len(err))
        if not h:
            raise RuntimeError(f"Failed to create Kokoro TTS model: {err.value.decode()}")
        return cls("", device, _handle=h)

    @classmethod
    def replicas(cls, model_path: str, devices: Sequence[int]) -> List["HipKoko"]:
        """One model per entry of `devices` from ONE read of the weight file: upload to devices[0], device-to-device
        fan-out to the others inside the library (kx_create_replicas).  The list is what `Dispatcher` takes; the
        reference's server is one process holding every GPU (kokorox-openai/src/lib.rs:370-439)."""
        lib = load_library()
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        if dev.ndim != 1 or dev.shape[0] < 1:
            raise ValueError("replicas: at least one device id")
        out = (C.c_void_p * dev.shape[0])()
        err = C.create_string_buffer(512)
        rc = lib.kx_create_replicas(os.fsencode(model_path), _ptr(dev), dev.shape[0], out, err, len(err))
        if rc != 0:
            raise RuntimeError(f"Failed to create Kokoro TTS model: {err.value.decode()}")
        return [cls("", int(d), _handle=out[i]) for i, d in enumerate(dev)]

    @staticmethod
    def replicas_times():
        """ms from the last `replicas` call's entry: [file read (+ conversion), blob resident on every device, models built]."""
        out = (C.c_double * 3)()
        load_library().kx_replicas_times(out)
        return list(out)

    @classmethod
    def partition(cls, model_path: str, device: int, part: int, n_parts: int) -> "HipKoko":
        """A model confined to 1 / n_parts of the device's CUs (kx_create_partition): partitions run side by side on one GPU."""
        lib = load_library()
        err = C.create_string_buffer(512)
        h = lib.kx_create_partition(os.fsencode(model_path), device, part, n_parts, err, len(err))
        if not h:
            raise RuntimeError(f"Failed to create Kokoro TTS model: {err.value.decode()}")
        return cls("", device, _handle=h)

    def last_error(self) -> str:
        """Thread-safe copy of the model's last failure text (kx_last_error_copy)."""
        buf = C.create_string_buffer(512)
        self._lib.kx_last_error_copy(self._h, buf, len(buf))
        return buf.value.decode()

    def infer(self, tokens: Sequence[Sequence[int]], styles: Sequence[Sequence[float]], speed: float,
              seed: int = 0, flags: int = 0):
        """tokens [[...]] (already 0-wrapped, koko.rs:1169-1175), styles [[256 floats]], speed.

        Batch of one returns the waveform as a 1-D float32 array (what koko.rs:1179 flattens);
        a batch of B returns a list of B arrays."""
        if len(tokens) == 0 or len(tokens[0]) == 0:
            raise ValueError("infer: empty token list")
        if len(styles) != len(tokens):
            raise ValueError("infer: one style row per utterance is required")
        outs = self.infer_batch(tokens, styles, [float(speed)], seed=seed, flags=flags)
        return outs[0] if len(outs) == 1 else outs

    # -- batched / instrumented forms -------------------------------------------------------
    def infer_batch(self, tokens, styles, speeds, seed: int = 0, flags: int = 0) -> List[np.ndarray]:
        B = len(tokens)
        lens = np.array([len(t) for t in tokens], dtype=np.int32)
        stride = int(lens.max()) if B else 0
        ids = np.zeros((B, max(stride, 1)), dtype=np.int64)
        for b, t in enumerate(tokens):
            ids[b, : len(t)] = np.asarray(t, dtype=np.int64)
        st = _f32(np.asarray(styles, dtype=np.float32).reshape(B, -1))
        if B and st.shape[1] != STYLE_DIM:
            raise ValueError(f"infer: style rows must have {STYLE_DIM} floats")
        sp = _f32(np.asarray(speeds, dtype=np.float32).reshape(-1))
        out = C.POINTER(C.c_float)()
        out_lens = np.zeros(max(B, 1), dtype=np.int64)
        rc = self._lib.kx_infer(self._h, _ptr(ids), ids.shape[1], _ptr(lens), B, _ptr(st), _ptr(sp), sp.shape[0],
                                seed, flags, C.byref(out), _ptr(out_lens))
        self._check(rc)
        try:
            total = int(out_lens[:B].sum())
            flat = np.ctypeslib.as_array(out, shape=(max(total, 1),))[:total].copy()
        finally:
            self._lib.kx_free_audio(out)
        res, o = [], 0
        for b in range(B):
            res.append(flat[o: o + int(out_lens[b])])
            o += int(out_lens[b])
        return res

    def infer_prosody(self, tokens, styles, speeds, prosody=None, seed: int = 0, flags: int = 0):
        """infer_batch with per-token prosody (kx_infer_prosody; the definition is in include/kokorox_hip.h, "prosody", the numpy form
        voices.prosody_durations / voices.shape_curves): `prosody` = (rate, frames, pitch, energy), each None or one sequence per
        utterance with a value per token; None = no prosody.  Returns (waveforms, durations): the list infer_batch returns and one
        int32 array per utterance, the frames each token was given."""
        ids, lens = self._ids_lens(tokens)
        B = len(tokens)
        st = _f32(np.asarray(styles, dtype=np.float32).reshape(B, STYLE_DIM))
        sp = _f32(np.asarray(speeds, dtype=np.float32).reshape(-1))
        ps, keep = prosody_arrays(prosody, lens, ids.shape[1])
        out = C.POINTER(C.c_float)()
        out_lens = np.zeros(max(B, 1), dtype=np.int64)
        dur = np.zeros(ids.shape, dtype=np.int32)
        rc = self._lib.kx_infer_prosody(self._h, _ptr(ids), ids.shape[1], _ptr(lens), B, _ptr(st), _ptr(sp), sp.shape[0], seed, flags,
                                        C.byref(out), _ptr(out_lens), None if ps is None else C.addressof(ps), _ptr(dur))
        del keep
        self._check(rc)
        try:
            total = int(out_lens[:B].sum())
            flat = np.ctypeslib.as_array(out, shape=(max(total, 1),))[:total].copy()
        finally:
            self._lib.kx_free_audio(out)
        cuts = np.cumsum(out_lens[:B])[:-1]
        return [w.copy() for w in np.split(flat, cuts)], [dur[b, : int(lens[b])].copy() for b in range(B)]

    def infer_requests_prosody(self, tokens, chunks_per_request, prosody=None, joins=None, styles=None, voice_ids=None, weights=None,
                               speeds=(1.0,), seed: int = 0, flags: int = 0, fmt=0, marks: bool = False, report: bool = True,
                               with_samples: bool = False):
        """infer_requests with per-token prosody and its report (kx_infer_requests_prosody): `prosody` as infer_prosody, one sequence
        per chunk; `joins` as infer_requests_joined, or None.  Returns (bodies, report) with report one float32 array [tokens, 4] per
        request = (mean voiced F0, voiced steps, mean N, frames) of every token, chunk after chunk (voices.prosody_report);
        marks=True: (bodies, marks, report); report=False leaves it out.  with_samples: out_samples as a last entry."""
        j = None if joins is None else join_specs(joins)
        res, mk, nsamp, rep = self._infer_requests(tokens, chunks_per_request, styles, voice_ids, weights, speeds, seed, flags, fmt, marks, j,
                                                   prosody=(prosody, report))
        out = (res, mk) if marks else (res,)
        out = out + (rep,) if report else out
        out = out + (nsamp,) if with_samples else out
        return out if len(out) > 1 else out[0]

    def infer_requests_fitted(self, tokens, chunks_per_request, fit, prosody=None, joins=None, styles=None, voice_ids=None, weights=None,
                              speeds=(1.0,), seed: int = 0, flags: int = 0, fmt=0, marks: bool = False, report: bool = False,
                              with_samples: bool = False):
        """infer_requests_prosody with fit spans (kx_infer_requests_fitted; the definition is in include/kokorox_hip.h, "fit", the numpy
        form voices.fit_durations): `fit` = a list of (request, begin, end, frames), sorted by (request, begin) and disjoint; tokens
        [begin, end) of that request, its chunks laid end to end, then last exactly `frames` frames of 25 ms (voices.fit_frames).
        Returns what infer_requests_prosody returns, then the fit results, one FIT_RESULT_DTYPE record per span."""
        j = None if joins is None else join_specs(joins)
        sp = fit_spans(fit)
        fr = np.zeros(max(len(sp), 1), FIT_RESULT_DTYPE)
        res, mk, nsamp, rep = self._infer_requests(tokens, chunks_per_request, styles, voice_ids, weights, speeds, seed, flags, fmt, marks, j,
                                                   prosody=(prosody, report, sp, fr))
        out = (res, mk) if marks else (res,)
        out = out + (rep,) if report else out
        out = out + (fr[: len(sp)],)
        return out + (nsamp,) if with_samples else out

    # -- device voice table, packed output -----------------------------
    def set_voice_table(self, table: np.ndarray):
        """table [n_voices, 511, 1, 256] (or [n, 511, 256]) as built by load_voices / hf_cache.rs:284-309."""
        t = _f32(np.asarray(table, dtype=np.float32).reshape(-1, 511, 256))
        self._check(self._lib.kx_set_voice_table(self._h, _ptr(t), t.shape[0]))

    def _unpack(self, out, nbytes, nsamp, B, fmt):
        total = int(nbytes[:B].sum())
        raw = C.string_at(out, total) if total else b""
        self._lib.kx_free_packed(out)
        res, o = [], 0
        dt = np.int16 if fmt == PACK_PCM16_MONO else np.float32
        for b in range(B):
            a = np.frombuffer(raw, dtype=dt, count=int(nbytes[b]) // np.dtype(dt).itemsize, offset=o).copy()
            res.append(a.reshape(-1, 2) if fmt == PACK_F32_STEREO else a)
            o += int(nbytes[b])
        return res

    def _ids_lens(self, tokens):
        B = len(tokens)
        lens = np.array([len(t) for t in tokens], dtype=np.int32)
        ids = np.zeros((B, max(int(lens.max()), 1)), dtype=np.int64)
        for b, t in enumerate(tokens):
            ids[b, : len(t)] = np.asarray(t, dtype=np.int64)
        return ids, lens

    def infer_voices(self, tokens, voice_ids, weights, speeds=(1.0,), seed: int = 0, flags: int = 0,
                     fmt: int = 0, with_samples: bool = False):
        """Style rows are looked up / mixed on the GPU: voice_ids [B, max_mix] (-1 = unused), weights [B, max_mix]
        (the number after the dot in "af_sky.4+af_nicole.5"); max_mix == 1 is the single-voice copy.  with_samples: also the
        library's own sample count of every utterance (out_samples), as a second list."""
        ids, lens = self._ids_lens(tokens)
        B = len(tokens)
        v = np.ascontiguousarray(np.asarray(voice_ids, dtype=np.int32).reshape(B, -1))
        w = _f32(np.asarray(weights, dtype=np.float32).reshape(B, -1))
        sp = _f32(np.asarray(speeds, dtype=np.float32).reshape(-1))
        out = C.c_void_p()
        nbytes, nsamp = np.zeros(B, np.int64), np.zeros(B, np.int64)
        self._check(self._lib.kx_infer_voices(self._h, _ptr(ids), ids.shape[1], _ptr(lens), B, _ptr(v), _ptr(w),
                                              v.shape[1], _ptr(sp), sp.shape[0], seed, flags, fmt, C.byref(out),
                                              _ptr(nbytes), _ptr(nsamp)))
        res = self._unpack(out, nbytes, nsamp, B, fmt)
        return (res, [int(n) for n in nsamp]) if with_samples else res

    def infer_packed(self, tokens, styles, speeds=(1.0,), seed: int = 0, flags: int = 0, fmt: int = 0, with_samples: bool = False):
        ids, lens = self._ids_lens(tokens)
        B = len(tokens)
        st = _f32(np.asarray(styles, dtype=np.float32).reshape(B, STYLE_DIM))
        sp = _f32(np.asarray(speeds, dtype=np.float32).reshape(-1))
        out = C.c_void_p()
        nbytes, nsamp = np.zeros(B, np.int64), np.zeros(B, np.int64)
        self._check(self._lib.kx_infer_packed(self._h, _ptr(ids), ids.shape[1], _ptr(lens), B, _ptr(st), _ptr(sp),
                                              sp.shape[0], seed, flags, fmt, C.byref(out), _ptr(nbytes), _ptr(nsamp)))
        res = self._unpack(out, nbytes, nsamp, B, fmt)
        return (res, [int(n) for n in nsamp]) if with_samples else res

    def infer_requests(self, tokens, chunks_per_request, styles=None, voice_ids=None, weights=None, speeds=(1.0,), seed: int = 0,
                       flags: int = 0, fmt=0, with_samples: bool = False):
        """Several requests of several chunks in one forward (kx_infer_requests): `tokens` are the B chunks (each 0-wrapped),
        request r owns chunks_per_request[r] consecutive ones.  The voice is per chunk: `styles` [B, 256], or `voice_ids` /
        `weights` [B, max_mix] as infer_voices.  `fmt` = one format word (a PACK_* form, optionally | PACK_RATE_*) for all, or one
        per request.  Returns one entry per request: its chunks' samples back to back, at the word's rate, as an array for forms
        0..2 (float32, [n, 2] float32, int16) and the G.711 forms (uint8), the body as `bytes` for PACK_WAV_F32,
        PACK_WAV16_BASE64, PACK_FLAC (whose size follows from the samples), PACK_ADPCM_WAV and PACK_WAV16.  with_samples: also the library's own sample count of every request (out_samples, at the output
        rate), as a second list."""
        res, _, nsamp, _ = self._infer_requests(tokens, chunks_per_request, styles, voice_ids, weights, speeds, seed, flags, fmt, False)
        return (res, nsamp) if with_samples else res

    def infer_requests_marks(self, tokens, chunks_per_request, styles=None, voice_ids=None, weights=None, speeds=(1.0,),
                             seed: int = 0, flags: int = 0, fmt=0, with_samples: bool = False):
        """infer_requests with the token marks of every request (kx_infer_requests_marks; the definition is in
        include/kokorox_hip.h, the numpy form voices.token_marks).  Returns (bodies, marks): bodies exactly as infer_requests,
        marks one int64 array per request -- per chunk its tokens + 1 sample offsets in the request's stream at the request's
        output rate, the chunks back to back (voices.token_spans splits them).  with_samples: out_samples as a third entry."""
        res, marks, nsamp, _ = self._infer_requests(tokens, chunks_per_request, styles, voice_ids, weights, speeds, seed, flags, fmt, True)
        return (res, marks, nsamp) if with_samples else (res, marks)

    def infer_requests_joined(self, tokens, chunks_per_request, joins, styles=None, voice_ids=None, weights=None, speeds=(1.0,),
                              seed: int = 0, flags: int = 0, fmt=0, marks: bool = False, with_samples: bool = False):
        """infer_requests with the seams of every request shaped on the GPU (kx_infer_requests_joined; the definition is in
        include/kokorox_hip.h, "joins", the numpy form voices.join_stream / voices.joined_marks): `joins` = one spec
        (flags, keep_ms, pause_ms, fade_ms) for all requests, or a list of one per request.  Returns the bodies as
        infer_requests does; marks=True: (bodies, marks) as infer_requests_marks.  with_samples: out_samples as a last entry."""
        j = join_specs(joins)
        res, mk, nsamp, _ = self._infer_requests(tokens, chunks_per_request, styles, voice_ids, weights, speeds, seed, flags, fmt, marks, j)
        out = (res, mk) if marks else (res,)
        out = out + (nsamp,) if with_samples else out
        return out if len(out) > 1 else out[0]

    def infer_requests_levelled(self, tokens, chunks_per_request, levels, joins=None, styles=None, voice_ids=None, weights=None,
                                speeds=(1.0,), seed: int = 0, flags: int = 0, fmt=0, marks: bool = False, with_samples: bool = False):
        """infer_requests with the level of every request set on the GPU (kx_infer_requests_levelled; the definition is in
        include/kokorox_hip.h, "levels", the numpy form voices.level_gain / voices.level_stream): `levels` = one spec
        (mode, gain, peak) for all requests, or a list of one per request; `joins` as infer_requests_joined, or None.  Returns
        (bodies, levels) with levels a float64 array [R, 2] = the peak p and the gain g of every request as the GPU computed
        them; marks=True: (bodies, marks, levels).  with_samples: out_samples as a last entry.  LEVEL_PLAIN is a peak meter."""
        lv = level_specs(levels)
        j = None if joins is None else join_specs(joins)
        res, mk, nsamp, out_lv = self._infer_requests(tokens, chunks_per_request, styles, voice_ids, weights, speeds, seed, flags, fmt, marks,
                                                      j, lv)
        out = (res, mk, out_lv) if marks else (res, out_lv)
        return out + (nsamp,) if with_samples else out

    def infer_requests_loudness(self, tokens, chunks_per_request, loudness, joins=None, styles=None, voice_ids=None, weights=None,
                                speeds=(1.0,), seed: int = 0, flags: int = 0, fmt=0, marks: bool = False, with_samples: bool = False):
        """infer_requests with the integrated loudness of every request measured, and set, on the GPU (kx_infer_requests_loudness;
        the definition is in include/kokorox_hip.h, "loudness", the numpy form voices.integrated_loudness / voices.loudness_gain):
        `loudness` = one spec (mode, target_lufs, peak) for all requests, or a list of one per request; `joins` as
        infer_requests_joined, or None.  Returns (bodies, loudness) with loudness a float64 array [R, 4] = the peak p, the gain g,
        the integrated loudness I in LUFS (NaN when undefined) and the number of gated blocks n_g of every request as the GPU
        computed them; marks=True: (bodies, marks, loudness).  with_samples: out_samples as a last entry.  LOUDNESS_METER measures."""
        ld = loudness_specs(loudness)
        j = None if joins is None else join_specs(joins)
        res, mk, nsamp, out_ld = self._infer_requests(tokens, chunks_per_request, styles, voice_ids, weights, speeds, seed, flags, fmt, marks,
                                                      j, None, ld)
        out = (res, mk, out_ld) if marks else (res, out_ld)
        return out + (nsamp,) if with_samples else out

    def infer_requests_limited(self, tokens, chunks_per_request, limits, joins=None, styles=None, voice_ids=None, weights=None,
                               speeds=(1.0,), seed: int = 0, flags: int = 0, fmt=0, marks: bool = False, with_samples: bool = False):
        """infer_requests with every request driven and peak-limited on the GPU (kx_infer_requests_limited; the definition is in
        include/kokorox_hip.h, "limiter", the numpy form voices.limit_stream): `limits` = one spec (mode, gain, target_lufs, peak)
        for all requests, or a list of one per request; `joins` as infer_requests_joined, or None.  Returns (bodies, limits) with
        limits a float64 array [R, 5] = the peak p, the static gain g, the integrated loudness I (NaN in mode 0 and when undefined),
        the gated blocks n_g and the smallest smoothed gain r of every request as the GPU computed them; marks=True: (bodies,
        marks, limits).  with_samples: out_samples as a last entry."""
        lm = limit_specs(limits)
        j = None if joins is None else join_specs(joins)
        res, mk, nsamp, out_lm = self._infer_requests(tokens, chunks_per_request, styles, voice_ids, weights, speeds, seed, flags, fmt, marks,
                                                      j, None, None, lm)
        out = (res, mk, out_lm) if marks else (res, out_lm)
        return out + (nsamp,) if with_samples else out

    def infer_requests_pieces(self, tokens, chunks_per_request, piece_flags, carries=None, levels=None, joins=None, styles=None,
                              voice_ids=None, weights=None, speeds=(1.0,), seed: int = 0, flags: int = 0, fmt=0, marks: bool = False,
                              with_samples: bool = False):
        """Pieces of requests in one forward (kx_infer_requests_pieces; the definition is in include/kokorox_hip.h, "pieces", the
        numpy form voices.piece_bodies / voices.piece_carry): request r of the call is a piece with the flag word piece_flags[r]
        (PIECE_FIRST, PIECE_LAST, both = a request run whole) and the carry carries[r] that the piece before it left (None, or
        anything for a first piece).  `levels` (mode LEVEL_GAIN for a piece) and `joins` as infer_requests_levelled, or None.
        Returns (payloads, carries): every payload as bytes -- the payloads of a request's pieces, end to end, are the body of the
        request run whole -- and the carries as an array of PIECE_CARRY_DTYPE, one per request, to hand to the next pieces;
        marks=True: (payloads, marks, carries), the marks positions in the whole request's stream.  With levels the result ends
        with the float64 [R, 2] array of p and g; with_samples: out_samples as a last entry.  Row b of the call draws the noise of
        utterance (utterance base + b): a later piece must run at the utterance base of its first row in the whole request
        (set_utterance_base; RequestStream does it)."""
        cpr = np.ascontiguousarray(chunks_per_request, dtype=np.int32).reshape(-1)
        R = cpr.shape[0]
        pf = np.ascontiguousarray(piece_flags, dtype=np.uint32).reshape(-1)
        if pf.shape[0] != R:
            raise ValueError(f"{R} piece flag words are required")
        cin = piece_carries(carries, R)
        cout = np.zeros(R, PIECE_CARRY_DTYPE)
        lv = None if levels is None else level_specs(levels)
        j = None if joins is None else join_specs(joins)
        res, mk, nsamp, out_lv = self._infer_requests(tokens, chunks_per_request, styles, voice_ids, weights, speeds, seed, flags, fmt, marks,
                                                      j, lv, pieces=(pf, cin, cout))
        out = (res, mk, cout) if marks else (res, cout)
        out = out + (out_lv,) if lv is not None else out
        return out + (nsamp,) if with_samples else out

    def _infer_requests(self, tokens, chunks_per_request, styles, voice_ids, weights, speeds, seed, flags, fmt, want_marks, joins=None,
                        levels=None, loudness=None, limits=None, prosody=None, pieces=None):
        """The call behind every infer_requests*: returns (bodies, marks, out_samples, extra) with marks None unless wanted and extra
        the [R, k] values of the level, loudness or limit list, the reports of a call with prosody that wants them, else None."""
        ids, lens = self._ids_lens(tokens)
        B = len(tokens)
        cpr = np.ascontiguousarray(chunks_per_request, dtype=np.int32).reshape(-1)
        R = cpr.shape[0]
        fm = np.ascontiguousarray(fmt, dtype=np.int32).reshape(-1)
        st = v = w = None
        mm = 0
        if styles is not None:
            st = _f32(np.asarray(styles, dtype=np.float32).reshape(B, STYLE_DIM))
        if voice_ids is not None:
            v = np.ascontiguousarray(np.asarray(voice_ids, dtype=np.int32).reshape(B, -1))
            w = _f32(np.asarray(weights, dtype=np.float32).reshape(B, -1))
            mm = v.shape[1]
        sp = _f32(np.asarray(speeds, dtype=np.float32).reshape(-1))
        out = C.c_void_p()
        nbytes, nsamp = np.zeros(max(R, 1), np.int64), np.zeros(max(R, 1), np.int64)
        args = (self._h, _ptr(ids), ids.shape[1], _ptr(lens), B, _ptr(cpr), R, _ptr(st), _ptr(v), _ptr(w), mm, _ptr(sp), sp.shape[0],
                seed, flags, _ptr(fm), fm.shape[0], C.byref(out), _ptr(nbytes), _ptr(nsamp))
        mk, n_mk = C.c_void_p(), np.zeros(max(R, 1), np.int64)
        # what every entry behind kx_infer_requests_marks takes next: the marks pair (both null: no marks), then the joins
        tail = (C.byref(mk) if want_marks else None, _ptr(n_mk) if want_marks else None, _ptr(joins), 0 if joins is None else joins.shape[0])
        # the one spec list that is set picks its entry: (list, entry, float64 values per request that come back)
        spec = next(((s, fn, k) for s, fn, k in ((limits, self._lib.kx_infer_requests_limited, 5), (loudness, self._lib.kx_infer_requests_loudness, 4),
                                                  (levels, self._lib.kx_infer_requests_levelled, 2)) if s is not None), None)
        marks = extra = keep = None
        if pieces is not None:  # (the flag words, the carries before, the carries behind): the levelled entry's list, which may be null
            if levels is not None:
                extra = np.zeros((max(R, 1), 2), np.float64)
            rc = self._lib.kx_infer_requests_pieces(*args, *tail, _ptr(levels), 0 if levels is None else levels.shape[0], _ptr(extra),
                                                    _ptr(pieces[0]), _ptr(pieces[1]), _ptr(pieces[2]))
            extra = None if extra is None else extra[:R]
        elif prosody is not None:  # (prosody, want the report) or, through the fitted entry, (..., the fit spans, their results)
            ps, keep = prosody_arrays(prosody[0], lens, ids.shape[1])
            rp, n_rp = C.c_void_p(), np.zeros(max(R, 1), np.int64)
            ptail = (None if ps is None else C.addressof(ps), C.byref(rp) if prosody[1] else None, _ptr(n_rp) if prosody[1] else None)
            if len(prosody) > 2:  # (..., the spans, their results)
                rc = self._lib.kx_infer_requests_fitted(*args, *tail, *ptail, _ptr(prosody[2]) if len(prosody[2]) else None, len(prosody[2]),
                                                        _ptr(prosody[3]))
            else:
                rc = self._lib.kx_infer_requests_prosody(*args, *tail, *ptail)
        elif spec is not None:
            extra = np.zeros((max(R, 1), spec[2]), np.float64)
            rc = spec[1](*args, *tail, _ptr(spec[0]), spec[0].shape[0], _ptr(extra))
            extra = extra[:R]
        elif joins is not None:
            rc = self._lib.kx_infer_requests_joined(*args, *tail)
        elif want_marks:
            rc = self._lib.kx_infer_requests_marks(*args, *tail[:2])
        else:
            rc = self._lib.kx_infer_requests(*args)
        del keep
        self._check(rc)
        if prosody is not None and prosody[1]:  # (the report lives in the buffer of `out`: read before it is released)
            n_tok = int(n_rp[:R].sum())
            if n_tok and ((rp.value or 0) % 8 != 0 or not (out.value <= (rp.value or 0))):
                self._lib.kx_free_packed(out)
                raise KokoroxHipError(3, "the report is not 8-byte aligned inside the packed buffer")
            flat_r = np.frombuffer(C.string_at(rp, 16 * n_tok) if n_tok else b"", dtype=np.float32).reshape(-1, 4).copy()
            extra = [x.copy() for x in np.split(flat_r, np.cumsum(n_rp[:R])[:-1])]
        total = int(nbytes[:R].sum())
        raw = C.string_at(out, total) if total else b""
        if want_marks:  # (the marks as well)
            if (mk.value or 0) % 8 != 0 or not (out.value <= mk.value):
                self._lib.kx_free_packed(out)
                raise KokoroxHipError(3, "marks are not 8-byte aligned inside the packed buffer")
            flat = np.frombuffer(C.string_at(mk, 8 * int(n_mk[:R].sum())), dtype=np.int64).copy()
            cuts = np.cumsum(n_mk[:R])[:-1]
            marks = [m.copy() for m in np.split(flat, cuts)]
        self._lib.kx_free_packed(out)
        res, o = [], 0
        for r in range(R):
            part = raw[o: o + int(nbytes[r])]
            o += int(nbytes[r])
            res.append(part if pieces is not None else _decode_packed(part, int(fm[r if fm.shape[0] > 1 else 0])))
        return res, marks, [int(v) for v in nsamp[:R]], extra

    def infer_device(self, d_ids: int, t_stride: int, lens_host: np.ndarray, d_styles: int, speeds_host: np.ndarray,
                     d_audio: int, audio_ld: int, d_frames: int, seed: int = 0, flags: int = 0) -> int:
        """Raw device-pointer form (bench.py); returns the audio row length that is needed."""
        lens_host = np.ascontiguousarray(lens_host, dtype=np.int32)
        speeds_host = _f32(speeds_host)
        need = C.c_int64(0)
        rc = self._lib.kx_infer_device(self._h, C.c_void_p(d_ids), t_stride, _ptr(lens_host), lens_host.shape[0],
                                       C.c_void_p(d_styles), _ptr(speeds_host), speeds_host.shape[0], seed, flags,
                                       C.c_void_p(d_audio), audio_ld, C.c_void_p(d_frames), C.byref(need))
        if rc != 0 and need.value > audio_ld:
            return int(need.value)
        self._check(rc)
        return int(need.value)

    def sync(self):
        self._check(self._lib.kx_sync(self._h))

    def set_pinned_durations(self, pattern: Optional[Sequence[int]]):
        if not pattern:
            self._check(self._lib.kx_set_pinned_durations(self._h, None, 0))
            return
        p = np.ascontiguousarray(pattern, dtype=np.int32)
        self._check(self._lib.kx_set_pinned_durations(self._h, _ptr(p), p.shape[0]))

    def warmup(self, B: int, n_tokens: int, frames_per_token: int = 8):
        """Size the arenas / result buffer for B utterances x n_tokens at frames_per_token frames per token (kx_warmup)."""
        self._check(self._lib.kx_warmup(self._h, B, n_tokens, frames_per_token))

    def arena_bytes(self):
        out = (C.c_int64 * 3)()
        self._check(self._lib.kx_arena_bytes(self._h, out))
        return list(out)

    def info(self):
        """kx_model_info as a dict: source variant, whether the arithmetic is the reference's for that file, conv mode, vocabulary,
        voices, CU partition."""
        out = (C.c_int64 * 8)()
        self._check(self._lib.kx_model_info(self._h, out))
        kinds = {0: "kxw container", 1: "onnx fp32", 2: "onnx fp16/bf16 (widened)", 3: "onnx 8-bit quantised (weights de-quantised)",
                 4: "onnx 4-bit quantised (weights de-quantised)", -1: "cached conversion", -2: "device blob"}
        return {"variant": int(out[0]), "variant_name": kinds.get(int(out[0]), "?"), "reference_arithmetic": bool(out[1]), "conv_mode": int(out[2]),
                "n_vocab": int(out[3]), "n_voices": int(out[4]), "cu_partition": int(out[5]), "cu_partitions": int(out[6]), "cus": int(out[7])}

    def status(self):
        """[recurrence in use (0 resident / 1 streaming), hand-off time-outs, clean forwards until the resident forms return, re-run calls]."""
        out = (C.c_int64 * 4)()
        self._check(self._lib.kx_model_status(self._h, out))
        return list(out)

    def call_times(self):
        """Host milestones of the last call in ms from its entry: [front queued, front done (the host wait), back planned, back queued]."""
        out = (C.c_double * 4)()
        self._check(self._lib.kx_call_times(self._h, out))
        return list(out)

    def set_conv_mode(self, mode: int):
        """0 = f32 MFMA, 1 = f16x3 split MFMA, 6 = f16f8 (default: f16x3 with the cross terms of the 7 / 11-tap convs on 8-bit
        MFMAs), 4 / 5 = f16 / bf16 single product (opt-in reduced precision)."""
        self._check(self._lib.kx_set_conv_mode(self._h, mode))

    def get_conv_mode(self) -> int:
        return int(self._lib.kx_get_conv_mode(self._h))

    def set_stft_variant(self, variant: int):
        """0 = the ONNX export's conv-based STFT pair (default), 1 = torch.stft / torch.istft semantics."""
        self._check(self._lib.kx_set_stft_variant(self._h, variant))

    def get_stft_variant(self) -> int:
        return int(self._lib.kx_get_stft_variant(self._h))

    def set_lanes(self, n: int):
        """1 = one stream; 4 = the independent chains of the back half side by side; 0 (default) = 4 up to batch 32,
        else 1.  Bit-identical results for every value."""
        self._check(self._lib.kx_set_lanes(self._h, n))

    def set_utterance_base(self, base: int):
        self._check(self._lib.kx_set_utterance_base(self._h, base))

    def profile_enable(self, on: bool):
        self._check(self._lib.kx_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        n, ms, fl = C.c_int64(0), C.c_double(0), C.c_double(0)
        self._check(self._lib.kx_profile_read(self._h, C.byref(n), C.byref(ms), C.byref(fl)))
        return int(n.value), float(ms.value), float(fl.value)

    def profile_detail(self) -> np.ndarray:
        """[n, 10] rows of the last profile_read: rows, Cin, taps, dil, stride, store, cols, flops, ms, algorithmic bytes."""
        n = C.c_int64(0)
        self._check(self._lib.kx_profile_detail(self._h, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 10), dtype=np.float64)
        self._check(self._lib.kx_profile_detail(self._h, _ptr(out), n.value, C.byref(n)))
        return out[: n.value]

    def profile_aux(self):
        """(launches, bytes) of the unfused InstanceNorm statistics passes since the last call."""
        n, by = C.c_int64(0), C.c_double(0)
        self._check(self._lib.kx_profile_aux(self._h, C.byref(n), C.byref(by)))
        return int(n.value), float(by.value)

    def diag_enable(self, on: bool):
        """Measure every conv input (after its AdaIN affine) during the following calls (real-weights report)."""
        self._check(self._lib.kx_diag_enable(self._h, 1 if on else 0))

    def diag_records(self):
        """[(layer, rows, Cin, taps, pre-scale exponent, absmax, rms, elements)] since diag_enable(True)."""
        n = C.c_int64(0)
        self._check(self._lib.kx_diag_count(self._h, C.byref(n)))
        out = []
        for i in range(n.value):
            name = C.create_string_buffer(128)
            v = np.zeros(7, dtype=np.float64)
            self._check(self._lib.kx_diag_get(self._h, i, name, len(name), _ptr(v)))
            out.append((name.value.decode(), int(v[0]), int(v[1]), int(v[2]), int(v[3]), float(v[4]), float(v[5]), float(v[6])))
        return out

    def set_act_prescale(self, layer: str, log2_scale: int):
        """f16x3: multiply this layer's transformed input by 2**log2_scale before the hi/lo split (undone exactly)."""
        self._check(self._lib.kx_set_act_prescale(self._h, layer.encode(), log2_scale))

    def tap(self, name: str, b: int = 0) -> np.ndarray:
        c, l = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.kx_debug_tap(self._h, name.encode(), b, None, 0, C.byref(c), C.byref(l)))
        out = np.empty((c.value, l.value), dtype=np.float32)
        self._check(self._lib.kx_debug_tap(self._h, name.encode(), b, _ptr(out), out.size, C.byref(c), C.byref(l)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.kx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise KokoroxHipError(rc, self.last_error())


class Dispatcher:
    """Batching front of one or more HipKoko models (one per GPU): the replacement for the reference's
    one-request-at-a-time `Mutex<Session>` (ort_koko.rs:78).  `submit` blocks and is thread-safe."""

    def __init__(self, models: Sequence[HipKoko], max_batch: int = 64, max_wait_us: int = 2000, warm: Optional[Sequence[int]] = None):
        """warm = (tokens, frames per token): one discarded forward of max_batch such utterances on every model first
        (kx_dispatcher_create_warm), so that no request ever pays for an arena growing."""
        self._lib = load_library()
        self._models = list(models)  # keep them alive
        arr = (C.c_void_p * len(self._models))(*[m._h for m in self._models])
        err = C.create_string_buffer(256)
        if warm:
            self._d = self._lib.kx_dispatcher_create_warm(arr, len(self._models), max_batch, max_wait_us, int(warm[0]), int(warm[1]), err, len(err))
        else:
            self._d = self._lib.kx_dispatcher_create(arr, len(self._models), max_batch, max_wait_us, err, len(err))
        if not self._d:
            raise RuntimeError(f"dispatcher: {err.value.decode()}")

    def submit(self, ids: Sequence[int], style: Sequence[float], speed: float = 1.0, seed: int = 0) -> np.ndarray:
        a = np.ascontiguousarray(ids, dtype=np.int64)
        st = _f32(np.asarray(style, dtype=np.float32).reshape(-1))
        if st.shape[0] != STYLE_DIM:
            raise ValueError(f"style row must have {STYLE_DIM} floats")
        out = C.POINTER(C.c_float)()
        n = C.c_int64(0)
        err = C.create_string_buffer(256)
        rc = self._lib.kx_dispatcher_submit(self._d, _ptr(a), a.shape[0], _ptr(st), float(speed), seed, C.byref(out),
                                            C.byref(n), err, len(err))
        if rc != 0:
            raise KokoroxHipError(rc, err.value.decode())
        try:
            return np.ctypeslib.as_array(out, shape=(max(n.value, 1),))[: n.value].copy()
        finally:
            self._lib.kx_free_audio(out)

    def submit_ex(self, ids: Sequence[int], style: Optional[Sequence[float]] = None,
                  voices: Optional[Sequence] = None, speed: float = 1.0, seed: int = 0, fmt: int = 0) -> np.ndarray:
        """The request as the reference's servers make it: `style` = the 256-float row, OR `voices` = one voice id
        (int: single voice, row copy) or [(voice id, weight), ...] (a mix "a.4+b.5", koko.rs:1255-1306) into the
        device voice table of every model; `fmt` = 0 f32 mono, 1 f32 stereo, 2 PCM16.  Returns the packed samples."""
        a = np.ascontiguousarray(ids, dtype=np.int64)
        st = vid = w = None
        n_mix = 0
        if style is not None:
            st = _f32(np.asarray(style, dtype=np.float32).reshape(-1))
            if st.shape[0] != STYLE_DIM:
                raise ValueError(f"style row must have {STYLE_DIM} floats")
        elif isinstance(voices, (int, np.integer)):
            vid, n_mix = np.array([voices], dtype=np.int32), 1
        else:
            vid = np.array([v for v, _ in voices], dtype=np.int32)
            w = np.array([x for _, x in voices], dtype=np.float32)
            n_mix = len(vid)
        out, nb, ns = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        err = C.create_string_buffer(256)
        rc = self._lib.kx_dispatcher_submit_ex(self._d, _ptr(a), a.shape[0], _ptr(st), _ptr(vid), _ptr(w), n_mix,
                                               float(speed), seed, fmt, C.byref(out), C.byref(nb), C.byref(ns), err, len(err))
        if rc != 0:
            raise KokoroxHipError(rc, err.value.decode())
        try:
            raw = C.string_at(out, nb.value)
        finally:
            self._lib.kx_free_audio(C.cast(out, C.POINTER(C.c_float)))
        if fmt == 2:
            return np.frombuffer(raw, dtype=np.int16).copy()
        arr = np.frombuffer(raw, dtype=np.float32).copy()
        return arr.reshape(-1, 2) if fmt == 1 else arr

    def submit_request(self, chunks: Sequence[Sequence[int]], styles=None, voices=None, speed: float = 1.0, seed: int = 0,
                       fmt: int = 0, marks: bool = False, join=None, level=None, loudness=None, limit=None, prosody=None,
                       report: bool = False, fit=None, piece=None):
        """A request of 1 .. max_batch chunks (kx_dispatcher_submit_request): `chunks` = the 0-wrapped id lists; `styles` = one
        256-float row per chunk, OR `voices` as in submit_ex (one voice spec for the request); `fmt` = a format word (a PACK_*
        form, optionally | PACK_RATE_*).  Returns what HipKoko.infer_requests returns for one request: an array (forms 0..2, 8, 9)
        or the body as bytes (3, 4, 12 = FLAC, 17 = ADPCM WAV, 18 = 16-bit WAV).  marks=True (kx_dispatcher_submit_request_marks): returns (body, marks), marks = the
        request's token marks as one int64 array (HipKoko.infer_requests_marks).  join = (flags, keep_ms, pause_ms, fade_ms)
        (kx_dispatcher_submit_request_joined): the request's seams shaped as HipKoko.infer_requests_joined shapes them.
        level = (mode, gain, peak) (kx_dispatcher_submit_request_levelled): the request's level set as
        HipKoko.infer_requests_levelled sets it; the result then ends with a float64 pair, the request's peak p and gain g.
        loudness = (mode, target_lufs, peak) (kx_dispatcher_submit_request_loudness): the request's loudness measured and set as
        HipKoko.infer_requests_loudness does; the result then ends with four float64 values, p, g, I and n_g.
        limit = (mode, gain, target_lufs, peak) (kx_dispatcher_submit_request_limited): the request driven and peak-limited as
        HipKoko.infer_requests_limited does; the result then ends with five float64 values, p, g, I, n_g and r.
        prosody = (rate, frames, pitch, energy), each None or one sequence per chunk (kx_dispatcher_submit_request_prosody), and / or
        report=True: the request shaped as HipKoko.infer_requests_prosody shapes it; with report=True the result ends with the
        request's float32 report [tokens, 4].  Not together with level, loudness or limit.
        fit = [(begin, end, frames), ...] (kx_dispatcher_submit_request_fitted): spans of the request's tokens, chunks laid end to end,
        fitted as HipKoko.infer_requests_fitted fits them; the result then ends with the FIT_RESULT_DTYPE records of the spans.  It goes
        with prosody and report, not with level, loudness or limit.
        piece = (flags, carry) (kx_dispatcher_submit_request_piece; include/kokorox_hip.h, "pieces"): `chunks` are a piece of a request,
        flags = PIECE_FIRST and / or PIECE_LAST, carry = the record the piece before left (None for a first piece).  The body comes
        back as bytes -- the payloads of a request's pieces, end to end, are the body of the request run whole -- and the result ends
        with the carry for the next piece, a PIECE_CARRY_DTYPE record.  It goes with marks, join and a level of mode LEVEL_GAIN."""
        lens = np.array([len(c) for c in chunks], dtype=np.int32)
        a = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.int64).reshape(-1) for c in chunks])
                                 if len(chunks) else np.zeros(0, np.int64))
        st = vid = w = None
        n_mix = 0
        if styles is not None:
            st = _f32(np.asarray(styles, dtype=np.float32).reshape(-1))
            if st.shape[0] != STYLE_DIM * len(chunks):
                raise ValueError(f"one style row of {STYLE_DIM} floats per chunk is required")
        elif voices is None:
            raise ValueError("submit_request: give styles (one row per chunk) or voices")
        elif isinstance(voices, (int, np.integer)):
            vid, n_mix = np.array([voices], dtype=np.int32), 1
        else:
            vid = np.array([v for v, _ in voices], dtype=np.int32)
            w = np.array([x for _, x in voices], dtype=np.float32)
            n_mix = len(vid)
        out, nb, ns = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        err = C.create_string_buffer(256)
        args = (self._d, _ptr(a), _ptr(lens), len(chunks), _ptr(st), _ptr(vid), _ptr(w), n_mix, float(speed), seed, fmt, C.byref(out),
                C.byref(nb), C.byref(ns))
        mk, n_mk = C.c_void_p(), C.c_int64(0)
        if (loudness is not None) + (level is not None) + (limit is not None) > 1:
            raise ValueError("submit_request: a request has a level or a loudness, not both" if limit is None else
                             "submit_request: a request has a level, a loudness or a limit, not two of them")
        if (prosody is not None or report or fit is not None) and (level is not None or loudness is not None or limit is not None):
            raise ValueError("submit_request: prosody does not go with a level, a loudness or a limit")
        rp, n_rp = C.c_void_p(), C.c_int64(0)
        # what every entry behind kx_dispatcher_submit_request_marks takes next: the marks pair (both null: no marks), then the join
        j = None if join is None else join_specs(join, 1)
        tail = (C.byref(mk) if marks else None, C.byref(n_mk) if marks else None, _ptr(j))
        # the one spec that is set picks its entry: (spec, entry, the float64 values that come back)
        spec = next(((make(s, 1), fn, np.zeros(k, np.float64)) for s, make, fn, k in
                     ((limit, limit_specs, self._lib.kx_dispatcher_submit_request_limited, 5),
                      (loudness, loudness_specs, self._lib.kx_dispatcher_submit_request_loudness, 4),
                      (level, level_specs, self._lib.kx_dispatcher_submit_request_levelled, 2)) if s is not None), None)
        if piece is not None and (loudness is not None or limit is not None or prosody is not None or report or fit is not None):
            raise ValueError("submit_request: a piece goes with marks, a join and a level only")
        carry_out = None
        keep = None
        fit_sp = fit_res = None
        if fit is not None:
            fit_sp = fit_spans([(0,) + tuple(f) for f in fit])
            fit_res = np.zeros(max(len(fit_sp), 1), FIT_RESULT_DTYPE)
        if prosody is not None or report or fit is not None:
            flat = None if prosody is None else tuple(None if x is None else [np.concatenate([np.asarray(c).reshape(-1) for c in x])] for x in prosody)
            ps, keep = prosody_arrays(flat, [int(lens.sum())], int(lens.sum()))
            ptail = (None if ps is None else C.addressof(ps), C.byref(rp) if report else None, C.byref(n_rp) if report else None)
            if fit is not None:
                rc = self._lib.kx_dispatcher_submit_request_fitted(*args, *tail, *ptail, _ptr(fit_sp) if len(fit_sp) else None, len(fit_sp),
                                                                   _ptr(fit_res), err, len(err))
            else:
                rc = self._lib.kx_dispatcher_submit_request_prosody(*args, *tail, *ptail, err, len(err))
        elif piece is not None:
            carry_in = None if piece[1] is None else piece_carries([piece[1]], 1)
            carry_out = np.zeros(1, PIECE_CARRY_DTYPE)
            rc = self._lib.kx_dispatcher_submit_request_piece(*args, *tail, None if spec is None else _ptr(spec[0]),
                                                              None if spec is None else _ptr(spec[2]), int(piece[0]), _ptr(carry_in),
                                                              _ptr(carry_out), err, len(err))
        elif spec is not None:
            rc = spec[1](*args, *tail, _ptr(spec[0]), _ptr(spec[2]), err, len(err))
        elif join is not None:
            rc = self._lib.kx_dispatcher_submit_request_joined(*args, *tail, err, len(err))
        elif marks:
            rc = self._lib.kx_dispatcher_submit_request_marks(*args, *tail[:2], err, len(err))
        else:
            rc = self._lib.kx_dispatcher_submit_request(*args, err, len(err))
        del keep
        if rc != 0:
            raise KokoroxHipError(rc, err.value.decode())
        try:
            raw = C.string_at(out, nb.value)
            if marks:  # (inside the allocation of `out`, 8-byte aligned behind the body: read before it is released)
                if (mk.value or 0) % 8 != 0 or (mk.value or 0) < out.value + nb.value:
                    raise KokoroxHipError(3, "marks are not 8-byte aligned behind the body")
                m = np.frombuffer(C.string_at(mk, 8 * n_mk.value), dtype=np.int64).copy()
            if report:  # (inside the allocation of `out` as well)
                if n_rp.value and ((rp.value or 0) % 8 != 0 or (rp.value or 0) < out.value + nb.value):
                    raise KokoroxHipError(3, "the report is not 8-byte aligned behind the body")
                rep_out = np.frombuffer(C.string_at(rp, 16 * n_rp.value) if n_rp.value else b"", dtype=np.float32).reshape(-1, 4).copy()
        finally:
            self._lib.kx_free_packed(out)
        body = raw if piece is not None else _decode_packed(raw, fmt)
        res = (body, m) if marks else (body,)
        res = res + (spec[2],) if spec is not None else res
        res = res + (carry_out[0].copy(),) if piece is not None else res
        res = res + (rep_out,) if report else res
        res = res + (fit_res[: len(fit_sp)],) if fit is not None else res
        return res if len(res) > 1 else res[0]

    def stats(self):
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._lib.kx_dispatcher_stats(self._d, C.byref(a), C.byref(b), C.byref(c))
        per = (C.c_int64 * len(self._models))()
        self._lib.kx_dispatcher_model_batches(self._d, per, len(self._models))
        rp, rt = C.c_int64(0), C.c_int64(0)
        self._lib.kx_dispatcher_failures(self._d, C.byref(rp), C.byref(rt))
        hl = (C.c_int32 * len(self._models))()
        mf, rq = C.c_int64(0), C.c_int64(0)
        self._lib.kx_dispatcher_health(self._d, hl, len(self._models), C.byref(mf), C.byref(rq))
        return {"requests": a.value, "batches": b.value, "max_batch": c.value, "batches_per_model": list(per),
                "replayed_requests": rp.value, "retried_batches": rt.value, "healthy": [int(v) for v in hl],
                "failed_models": mf.value, "requeued_requests": rq.value}

    def close(self):
        if getattr(self, "_d", None):
            self._lib.kx_dispatcher_destroy(self._d)
            self._d = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RequestStream:
    """One request sent in pieces (include/kokorox_hip.h, "pieces"): holds the carry between `send` calls, so that the payloads
    that come back, end to end, are the body of the request run whole -- the header of the form first, every byte.  `backend` is a
    HipKoko or a Dispatcher; fmt, join, level, speed and seed are the request's and stay the same for every piece.  With a HipKoko
    the rows of a later piece run at the utterance base of their place in the whole request (`utterance_base` + the chunks so far),
    and the model's utterance base is put back to `utterance_base` after every call."""

    def __init__(self, backend, fmt: int = PACK_WAV_F32, join=None, level=None, speed: float = 1.0, seed: int = 0, marks: bool = False,
                 utterance_base: int = 0):
        self._be, self._fmt, self._join, self._level, self._speed, self._seed, self._marks = backend, fmt, join, level, speed, seed, marks
        self._base = utterance_base
        self._carry = None
        self._chunks = 0
        self.closed = False

    def send(self, chunks, styles, last: bool = False):
        """The next chunks of the request (0-wrapped id lists) with one style row each; last=True closes the request.  Returns the
        payload as bytes (possibly empty); with marks, (payload, marks) with the marks positions in the whole request's stream."""
        if self.closed:
            raise ValueError("RequestStream: the request has had its last piece")
        flags = (PIECE_FIRST if self._carry is None else 0) | (PIECE_LAST if last else 0)
        if isinstance(self._be, Dispatcher):
            res = self._be.submit_request(chunks, styles=styles, speed=self._speed, seed=self._seed, fmt=self._fmt, marks=self._marks,
                                          join=self._join, level=self._level, piece=(flags, self._carry))
            body, carry = res[0], res[-1]
            mk = res[1] if self._marks else None
        else:
            self._be.set_utterance_base(self._base + self._chunks)
            try:
                res = self._be.infer_requests_pieces(chunks, [len(chunks)], [flags], None if self._carry is None else [self._carry],
                                                     levels=self._level, joins=self._join, styles=styles, speeds=(self._speed,),
                                                     seed=self._seed, fmt=self._fmt, marks=self._marks)
            finally:
                self._be.set_utterance_base(self._base)
            body, carry = res[0][0], res[2 if self._marks else 1][0]
            mk = res[1][0] if self._marks else None
        self._carry = carry
        self._chunks += len(chunks)
        self.closed = last
        return (body, mk) if self._marks else body


# ---- stand-alone kernel hooks (tests) -----------------------------------------------------
def import_onnx(onnx_path: str, out_path: str) -> str:
    """`model.onnx` -> KXHIPW01 container through the LIBRARY's own reader (csrc/onnx_import.cpp; host only, no GPU):
    what kx_create does in memory when it is handed the .onnx path the reference passes (koko.rs:570-573)."""
    lib = load_library()
    err = C.create_string_buffer(2048)
    rc = lib.kx_import_onnx(os.fsencode(onnx_path), os.fsencode(out_path), err, len(err))
    if rc != KX_OK:
        raise KokoroxHipError(rc, err.value.decode(errors="replace"))
    return out_path


def _err_call(fn, *args):
    err = C.create_string_buffer(512)
    rc = fn(*args, err, len(err))
    if rc != 0:
        raise KokoroxHipError(rc, err.value.decode())


CONV_F32, CONV_F16X3, CONV_F16F8 = 0, 1, 6
STFT_ONNX, STFT_TORCH = 0, 1


class ConvArgs(C.Structure):
    """kx_test_conv_args of include/kokorox_hip_test.h, member for member (tests/test_host_cpu.py compares the two)."""
    _fields_ = ([("struct_size", C.c_uint32), ("device_id", C.c_int32)]
                + [(n, C.c_void_p) for n in ("x", "w", "bias", "alpha", "norm", "resid", "lens", "y")]
                + [("y_floats", C.c_int64)]
                + [(n, C.c_void_p) for n in ("stats_out", "norm_gb", "norm_out", "plan_out")]
                + [(n, C.c_int32) for n in ("B", "Cin", "L", "Cout", "k", "stride", "pad", "dil", "up_stride", "act")]
                + [("slope", C.c_float), ("accumulate", C.c_int32), ("out_mul", C.c_float), ("out_div", C.c_float)]
                + [(n, C.c_int32) for n in ("mode", "pad_ld", "flat", "in_up2", "epi", "merged", "tmajor", "prec1", "act_shift",
                                            "epi_stream", "len_mul_in", "len_add_in", "len_mul_out", "len_add_out", "up_off", "view")])


def _conv(x, w, bias=None, stride=1, pad=0, dil=1, up_stride=0, act=0, slope=0.0, alpha=None, norm=None, resid=None, y_init=None,
          out_mul=1.0, out_div=1.0, want_stats=False, lens=None, mode=1, pre=False, want_norm=None, len_in=None, len_out=None,
          device=0, **flags):
    """One descriptor, one call of kx_test_conv: what every conv wrapper below maps its arguments onto.  up_stride = s > 0: the
    polyphase transposed conv (w [Cin,Cout,2 s]) with the pad given; flags: the remaining int fields of ConvArgs by name.
    Returns a dict: y at its stored shape, the plan that ran, stats and norm when asked for."""
    lib = load_test_library()
    x, w = _f32(x), _f32(w)
    B, Cin, L = x.shape
    k = w.shape[2]
    if up_stride:
        Cout = w.shape[1]
        Lout = (L - 1) * up_stride - 2 * pad + k + (1 if flags.get("up_off") else 0)
    else:
        Cout = w.shape[0]
        Lout = ((2 * L if flags.get("in_up2") else L) + 2 * pad - dil * (k - 1) - 1) // stride + 1
    shape = (B, Lout, Cout) if flags.get("tmajor") else (B, Cout, Lout)
    y = np.zeros(shape, dtype=np.float32) if y_init is None else _f32(y_init).copy()
    st = np.zeros((B, Cout, 2), dtype=np.float32) if want_stats else None
    gb = _f32(want_norm)
    assert gb is None or gb.shape == (B, 2 * Cout)
    planes = None if gb is None else np.zeros((3, B, Cout), dtype=np.float32)
    plan = np.zeros(len(CONV_PLAN_FIELDS), dtype=np.int64)
    ptrs = dict(x=x, w=w, bias=_f32(bias), alpha=_f32(alpha), norm=_f32(norm), resid=_f32(resid),
                lens=None if lens is None else np.ascontiguousarray(lens, dtype=np.int32), y=y, stats_out=st, norm_gb=gb,
                norm_out=planes, plan_out=plan)  # (kept alive until the call returns)
    a = ConvArgs(struct_size=C.sizeof(ConvArgs), device_id=device, y_floats=y.size, B=B, Cin=Cin, L=L, Cout=Cout, k=k, stride=stride,
                 pad=pad, dil=dil, up_stride=up_stride, act=act, slope=float(slope), accumulate=0 if y_init is None else 1,
                 out_mul=float(out_mul), out_div=float(out_div), mode=mode | (0x100 if pre else 0), **{n: int(v) for n, v in flags.items()},
                 **{n: _ptr(p) for n, p in ptrs.items()})
    (a.len_mul_in, a.len_add_in), (a.len_mul_out, a.len_add_out) = len_in or (0, 0), len_out or (0, 0)
    _err_call(lib.kx_test_conv, C.byref(a))
    pl = dict(zip(CONV_PLAN_FIELDS, (int(v) for v in plan)))
    pl["form"] = CONV_FORMS[pl["form"]]
    return {"y": y, "plan": pl, "stats": st, "norm": planes}


def conv1d(x, w, bias=None, stride=1, pad=0, dil=1, transposed=False, act=0, slope=0.0, alpha=None, norm=None,
           device=0, mode=None, pre=False):
    """Run the MFMA conv kernel alone: x [B,Cin,L], w [Cout,Cin,k] ([Cin,Cout,k] if transposed).  pre: stage the input
    through a pre-split image (conv_f16x3_pre.hip; direct-A kernels only)."""
    if mode is None:
        mode = CONV_F32 if os.environ.get("KOKOROX_CONV", "") == "f32" else CONV_F16X3
    if transposed:
        return _conv(x, w, bias, up_stride=stride, pad=pad, dil=dil, act=act, slope=slope, alpha=alpha, norm=norm, device=device,
                     mode=mode, pre=pre)["y"]
    return _conv(x, w, bias, stride=stride, pad=pad, dil=dil, act=act, slope=slope, alpha=alpha, norm=norm, device=device, mode=mode,
                 pre=pre)["y"]


# kx::ConvLaunch and kx::ConvPlan (kokorox_amd/csrc/kx_common.h), field by field in declaration order
CONV_LAUNCH_FIELDS = ("mode", "prec1", "f8", "BM", "rows", "n_chunks16", "K", "dil", "stride", "pad", "act", "in_up2", "store", "accum",
                      "epi", "norm", "stats", "image", "merge_T", "x_bs", "x_ld", "B", "cols", "cus", "force")
CONV_PLAN_FIELDS = ("form", "bm", "act", "kt", "wm", "wn", "vt", "pf", "p1", "bf", "bn", "cols", "merged", "pre", "stat_cols",
                    "stat_tiles", "flat_bn")
CONV_FORMS = ("F32", "LDS", "DAG", "DAGN", "DA", "DA_W2", "DA_S16", "DA_F8", "DA_PRE", "DAPN")  # kx::ConvForm


def conv_plan(**launch):
    """The launch plan of one conv (conv_plan.hip) for the kx::ConvLaunch fields given (the others 0), computed on the host: a
    dict of the kx::ConvPlan fields, with "form" as its ConvForm name.  Needs no GPU."""
    lib = load_test_library()
    unknown = set(launch) - set(CONV_LAUNCH_FIELDS)
    assert not unknown, unknown
    src = np.array([int(launch.get(f, 0)) for f in CONV_LAUNCH_FIELDS], dtype=np.int64)
    out = np.zeros(len(CONV_PLAN_FIELDS), dtype=np.int64)
    _err_call(lib.kx_test_conv_plan, _ptr(src), len(src), _ptr(out), len(out))
    plan = dict(zip(CONV_PLAN_FIELDS, (int(v) for v in out)))
    plan["form"] = CONV_FORMS[plan["form"]]
    return plan


def conv_transpose(x, w, bias=None, stride=6, act=1, slope=0.1, resid=None, up_off=0, mode=1, pre=False, device=0):
    """Polyphase transposed conv as Generator.ups runs it: x [B,Cin,L], w [Cin,Cout,2*stride] -> y [B,Cout,Lout + up_off]
    (+ resid; up_off = 1: output from column 1, column 0 = reflection of column 1)."""
    k = np.shape(w)[2]
    assert k == 2 * stride
    return _conv(x, w, bias, up_stride=stride, pad=(k - stride) // 2, act=act, slope=slope, resid=resid, up_off=1 if up_off else 0,
                 mode=mode, pre=pre, device=device)["y"]


def conv1d_epilogue(x, w, bias=None, pad=0, dil=1, resid=None, y_init=None, out_mul=1.0, out_div=1.0, want_stats=False,
                    mode=1, device=0):
    """Stride-1 conv through the epilogue forms: y = (conv + bias + resid [+ y_init]) * out_mul / out_div, and the
    fused per-row (sum, sum of squares) when want_stats.  Returns y or (y, stats[B,Cout,2])."""
    r = _conv(x, w, bias, pad=pad, dil=dil, resid=resid, y_init=y_init, out_mul=out_mul, out_div=out_div, want_stats=want_stats,
              mode=mode, device=device)
    return (r["y"], r["stats"]) if want_stats else r["y"]


def conv1d_full(x, w, bias=None, pad=0, dil=1, act=0, slope=0.0, alpha=None, norm=None, resid=None, y_init=None,
                out_mul=1.0, out_div=1.0, want_stats=False, lens=None, pad_ld=False, flat=False, mode=1, device=0, pre=False):
    """Stride-1 conv with the fused input transform (AdaIN affine + leaky / snake) AND the epilogue forms, on a ragged
    batch (lens[b] valid input columns), with pad_ld on the model's padded rows, with flat through the flat list of live
    tiles the model gives the direct-A kernels.  Returns y or (y, stats[B,Cout,2])."""
    r = _conv(x, w, bias, pad=pad, dil=dil, act=act, slope=slope, alpha=alpha, norm=norm, resid=resid, y_init=y_init, out_mul=out_mul,
              out_div=out_div, want_stats=want_stats, lens=lens, pad_ld=pad_ld, flat=flat, mode=mode, device=device, pre=pre)
    return (r["y"], r["stats"]) if want_stats else r["y"]


def conv1d_opts(x, w, bias=None, pad=0, dil=1, act=0, slope=0.0, alpha=None, norm=None, resid=None, y_init=None,
                out_mul=1.0, out_div=1.0, want_stats=False, lens=None, pad_ld=False, flat=False, mode=1, device=0, pre=False,
                in_up2=False, epi=0, merged=False, tmajor=False, prec1=0, act_shift=0, epi_stream=False, want_norm=None,
                up_stride=0, stride=1, len_in=None, len_out=None, up_off=False, view=False):
    """conv1d_full plus the launch options Model::conv sets (include/kokorox_hip_test.h, kx_test_conv_args): in_up2 (x [B,Cin,L]
    read as 2 L columns), epi (1 = gelu_new), merged (the plan may merge the batch's columns), tmajor (y [B,Lout,Cout]), prec1,
    act_shift, epi_stream, up_stride (s > 0: the polyphase transposed conv instead, w [Cin,Cout,2 s]); want_norm = gb [B,2 Cout]: the fused partial sums finalized into (mean, scale, shift) [3,B,Cout].
    stride (plain convs), len_in / len_out = (mul, add): lens[] are units (the model's frames) and utterance b has lens[b] * mul + add
    input / output columns, up_off (with up_stride: the output starts at column 1, column 0 is its reflection; y and resid are
    [B,Cout,Lout + 1]), view (x, resid and y are row slices of taller tensors).  A call that uses one of these five gets unowned output
    columns back as LN_SENTINEL.
    Returns a dict: y at its stored shape, plan (the ConvPlan that ran, as conv_plan returns it), and stats / norm when asked for."""
    if up_stride:  # (k = 2 s taps, pad = (k - s) / 2, no dilation: pad and dil are not the caller's)
        k = np.shape(w)[2]
        assert k == 2 * up_stride
        pad, dil = (k - up_stride) // 2, 1
    return _conv(x, w, bias, stride=stride, pad=pad, dil=dil, up_stride=up_stride, act=act, slope=slope, alpha=alpha, norm=norm,
                 resid=resid, y_init=y_init, out_mul=out_mul, out_div=out_div, want_stats=want_stats, lens=lens, mode=mode, pre=pre,
                 want_norm=want_norm, len_in=len_in, len_out=len_out, device=device, pad_ld=pad_ld, flat=flat, in_up2=in_up2, epi=epi,
                 merged=merged, tmajor=tmajor, prec1=prec1, act_shift=act_shift, epi_stream=epi_stream, up_off=up_off, view=view)


LN_PLAIN, LN_AFFINE, LN_ADA = 0, 1, 2


def layernorm(x, lens, eps=1e-5, mode=LN_PLAIN, g=None, be=None, leaky=0.0, device=0):
    """Channel layer norm of x [B,C,T] over C (launch_layernorm_ch) on the model's padded rows.  g, be: [C] (LN_AFFINE) or [B,C]
    (LN_ADA: (1 + g) xhat + be).  Columns >= lens[b] come back as LN_SENTINEL."""
    lib = load_test_library()
    x = _f32(x)
    B, C, T = x.shape
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    g, be = _f32(g), _f32(be)
    if mode != LN_PLAIN:
        assert g.shape == be.shape == ((B, C) if mode == LN_ADA else (C,))
    y = np.zeros((B, C, T), dtype=np.float32)
    _err_call(lib.kx_test_layernorm, device, _ptr(x), B, C, T, _ptr(ln), float(eps), mode, _ptr(g), _ptr(be), float(leaky), _ptr(y))
    return y


LN_SENTINEL = np.float32(-12345.5)


def instance_norm(x, lens, gb, device=0):
    """InstanceNorm statistics of x [B,C,L] with gb [B,2 C] (gamma | beta) -> [3 routes, 3, B, C]: (mean, scale, shift) from
    launch_in_stats alone, from launch_in_stats leaving raw sums, and from those raw sums through launch_stats_finalize."""
    lib = load_test_library()
    x, gb = _f32(x), _f32(gb)
    B, C, L = x.shape
    assert gb.shape == (B, 2 * C)
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    out = np.zeros((3, 3, B, C), dtype=np.float32)
    _err_call(lib.kx_test_instance_norm, device, _ptr(x), B, C, L, _ptr(ln), _ptr(gb), _ptr(out))
    return out


def lstm(x, params, device=0):
    """x [B,L,n_in]; params = (w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r) -> [B,L,512]."""
    lib = load_test_library()
    x = _f32(x)
    B, L, n_in = x.shape
    ps = [_f32(p) for p in params]
    y = np.zeros((B, L, 512), dtype=np.float32)
    _err_call(lib.kx_test_lstm, device, _ptr(x), B, L, n_in, *[_ptr(p) for p in ps], _ptr(y))
    return y


def lstm_ragged(x, lens, params, inplace=False, repeat=1, epoch0=0, device=0):
    """lstm() on a ragged batch (kx_test_lstm_ragged): x [B,L,n_in] with utterance b valid for lens[b] steps -> [B,L,512], columns
    >= lens[b] = LN_SENTINEL.  inplace: the output is rows 0..511 of the 640-row input tensor (n_in = 640); repeat launches on one
    exchange buffer whose launch counter starts at epoch0 (two that differ in a bit raise)."""
    lib = load_test_library()
    x = _f32(x)
    B, L, n_in = x.shape
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    assert ln.shape == (B,)
    ps = [_f32(p) for p in params]
    y = np.zeros((B, L, 512), dtype=np.float32)
    _err_call(lib.kx_test_lstm_ragged, device, _ptr(x), _ptr(ln), B, L, n_in, *[_ptr(p) for p in ps], 1 if inplace else 0, repeat,
              epoch0, _ptr(y))
    return y


INT_SENTINEL = np.int32(np.uint32(0xA5A5A5A5).astype(np.int32))  # integer buffers of the hooks start as 0xA5 bytes


def alignment(logits, lens, speeds, src, pinned=None, idx_ld=None, Fcap=None, device=0):
    """Duration head and alignment (kx_test_alignment): logits [B,50,T], lens [B], speeds [1 or B], src [B,C,T], pinned (1..50
    each) or None, rows of idx_ld frames (default 50 T) -> (dur [B,512], frames [B], idx [B,idx_ld], gathered [B,C,Fcap],
    overflow word).  Untouched entries: INT_SENTINEL / LN_SENTINEL."""
    lib = load_test_library()
    logits, src = _f32(logits), _f32(src)
    B, n50, T = logits.shape
    assert n50 == 50 and src.shape[0] == B and src.shape[2] == T
    C_ = src.shape[1]
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    sp = np.ascontiguousarray(speeds, dtype=np.float32).reshape(-1)
    pin = None if pinned is None else np.ascontiguousarray(pinned, dtype=np.int32)
    idx_ld = 50 * T if idx_ld is None else idx_ld
    Fcap = idx_ld if Fcap is None else Fcap
    dur = np.zeros((B, 512), dtype=np.int32)
    frames = np.zeros(B, dtype=np.int32)
    idx = np.zeros((B, idx_ld), dtype=np.int32)
    g = np.zeros((B, C_, Fcap), dtype=np.float32)
    over = np.zeros(1, dtype=np.uint32)
    _err_call(lib.kx_test_alignment, device, _ptr(logits), B, T, _ptr(ln), _ptr(sp), len(sp), _ptr(pin), 0 if pin is None else len(pin),
              _ptr(src), C_, idx_ld, _ptr(dur), _ptr(frames), _ptr(idx), _ptr(g), Fcap, _ptr(over))
    return dur, frames, idx, g, int(over[0])


def prosody_durations(logits, lens, speeds, src, rate=None, frames=None, pinned=None, idx_ld=None, Fcap=None, device=0):
    """`alignment` on the prosody duration kernel (kx_test_prosody_durations): rate / frames [B,T] per token, either may be None (not
    both).  Returns what `alignment` returns."""
    lib = load_test_library()
    logits, src = _f32(logits), _f32(src)
    B, n50, T = logits.shape
    assert n50 == 50 and src.shape[0] == B and src.shape[2] == T
    C_ = src.shape[1]
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    sp = np.ascontiguousarray(speeds, dtype=np.float32).reshape(-1)
    pin = None if pinned is None else np.ascontiguousarray(pinned, dtype=np.int32)
    rt = None if rate is None else np.ascontiguousarray(rate, dtype=np.float32).reshape(B, T)
    fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32).reshape(B, T)
    idx_ld = 50 * T if idx_ld is None else idx_ld
    Fcap = idx_ld if Fcap is None else Fcap
    dur = np.zeros((B, 512), dtype=np.int32)
    n_frames = np.zeros(B, dtype=np.int32)
    idx = np.zeros((B, idx_ld), dtype=np.int32)
    g = np.zeros((B, C_, Fcap), dtype=np.float32)
    over = np.zeros(1, dtype=np.uint32)
    _err_call(lib.kx_test_prosody_durations, device, _ptr(logits), B, T, _ptr(ln), _ptr(sp), len(sp), _ptr(pin), 0 if pin is None else len(pin),
              _ptr(rt), _ptr(fr), _ptr(src), C_, idx_ld, _ptr(dur), _ptr(n_frames), _ptr(idx), _ptr(g), Fcap, _ptr(over))
    return dur, n_frames, idx, g, int(over[0])


def fit_durations(logits, lens, speeds, src, spans, chunks_per_request=None, rate=None, frames=None, idx_ld=None, Fcap=None, device=0):
    """`prosody_durations` with the fit in front of it (kx_test_fit_durations): spans = [(request, begin, end, frames), ...] over the
    requests of chunks_per_request (None: every row a request).  Returns what `alignment` returns, then w [B,512], fitted [B,512]
    and the FIT_RESULT_DTYPE records of the spans."""
    lib = load_test_library()
    logits, src = _f32(logits), _f32(src)
    B, n50, T = logits.shape
    assert n50 == 50 and src.shape[0] == B and src.shape[2] == T
    C_ = src.shape[1]
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    sp = np.ascontiguousarray(speeds, dtype=np.float32).reshape(-1)
    rt = None if rate is None else np.ascontiguousarray(rate, dtype=np.float32).reshape(B, T)
    fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32).reshape(B, T)
    cpr = None if chunks_per_request is None else np.ascontiguousarray(chunks_per_request, dtype=np.int32).reshape(-1)
    fs = fit_spans(spans)
    idx_ld = 50 * T if idx_ld is None else idx_ld
    Fcap = idx_ld if Fcap is None else Fcap
    dur = np.zeros((B, 512), dtype=np.int32)
    n_frames = np.zeros(B, dtype=np.int32)
    idx = np.zeros((B, idx_ld), dtype=np.int32)
    g = np.zeros((B, C_, Fcap), dtype=np.float32)
    over = np.zeros(1, dtype=np.uint32)
    w = np.zeros((B, 512), dtype=np.float32)
    fitted = np.zeros((B, 512), dtype=np.int32)
    res = np.zeros(max(len(fs), 1), FIT_RESULT_DTYPE)
    _err_call(lib.kx_test_fit_durations, device, _ptr(logits), B, T, _ptr(ln), _ptr(sp), len(sp), _ptr(rt), _ptr(fr), _ptr(cpr),
              B if cpr is None else len(cpr), _ptr(fs) if len(fs) else None, len(fs), _ptr(src), C_, idx_ld, _ptr(dur), _ptr(n_frames),
              _ptr(idx), _ptr(g), Fcap, _ptr(over), _ptr(w), _ptr(fitted), _ptr(res))
    return dur, n_frames, idx, g, int(over[0]), w, fitted, res[: len(fs)]


def prosody_curves(curves, frames, lens, idx, dur, pitch=None, energy=None, report=True, device=0):
    """The curve and report kernel (kx_test_prosody_curves): curves [B,2,2 Fcap] (F0, N), frames [B], lens [B], idx [B,idx_ld],
    dur [B,T], pitch / energy [B,T] or None -> (shaped [B,2,2 Fcap], report [sum(lens),4] or None)."""
    lib = load_test_library()
    curves = _f32(curves)
    B, two, n2 = curves.shape
    assert two == 2 and n2 % 2 == 0
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    ix = np.ascontiguousarray(idx, dtype=np.int32)
    du = np.ascontiguousarray(dur, dtype=np.int32)
    T = du.shape[1]
    assert ix.shape[0] == B and du.shape[0] == B
    pt = None if pitch is None else np.ascontiguousarray(pitch, dtype=np.float32).reshape(B, T)
    en = None if energy is None else np.ascontiguousarray(energy, dtype=np.float32).reshape(B, T)
    shaped = np.zeros_like(curves)
    rep = np.zeros((int(ln.sum()), 4), dtype=np.float32) if report else None
    _err_call(lib.kx_test_prosody_curves, device, _ptr(curves), _ptr(fr), B, n2 // 2, _ptr(ln), T, _ptr(ix), ix.shape[1], _ptr(du), _ptr(pt),
              _ptr(en), _ptr(shaped), _ptr(rep))
    return shaped, rep


def embed(ids, lens, T, text_table, word, type0, pos, device=0):
    """Both embedding kernels on ids [B,ids_stride] (kx_test_embed) -> (text [B,512,T], albert [B,128,T], sticky bad-id word)."""
    lib = load_test_library()
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    B, stride = ids.shape
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    text_table, word, type0, pos = _f32(text_table), _f32(word), _f32(type0), _f32(pos)
    n_vocab = text_table.shape[0]
    assert text_table.shape == (n_vocab, 512) and word.shape == (n_vocab, 128) and type0.shape == (128,) and pos.shape == (T, 128)
    out_t = np.zeros((B, 512, T), dtype=np.float32)
    out_a = np.zeros((B, 128, T), dtype=np.float32)
    bad = np.zeros(1, dtype=np.uint32)
    _err_call(lib.kx_test_embed, device, _ptr(ids), B, stride, T, _ptr(ln), _ptr(text_table), _ptr(word), _ptr(type0), _ptr(pos), n_vocab,
              _ptr(out_t), _ptr(out_a), _ptr(bad))
    return out_t, out_a, int(bad[0])


def style_fc(styles, ws, bs, style_offs, device=0):
    """The style projections of a call in one launch (kx_test_style_fc): styles [B,256], descriptor i = (ws[i] [n_out,128], bs[i]
    [n_out], style_offs[i] in (0, 128)) -> [B, sum n_out], descriptor i behind the ones before it."""
    lib = load_test_library()
    styles = _f32(styles)
    B = styles.shape[0]
    n_out = np.array([w.shape[0] for w in ws], dtype=np.int32)
    w = _f32(np.concatenate([np.asarray(w, dtype=np.float32).reshape(-1, 128) for w in ws]))
    b = _f32(np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1) for x in bs]))
    so = np.ascontiguousarray(style_offs, dtype=np.int32)
    out = np.zeros((B, int(n_out.sum())), dtype=np.float32)
    _err_call(lib.kx_test_style_fc, device, _ptr(styles), B, _ptr(w), _ptr(b), _ptr(n_out), _ptr(so), len(n_out), _ptr(out))
    return out


def rows(styles, lens, T, src, Ld, mul=1, add=0, device=0):
    """launch_fill_style_rows and launch_copy_rows (kx_test_rows): styles [B,256], lens [B] -> (fill [B,640,T] with rows 512..639
    = styles[b, 128 + k] over lens[b] columns, copy [B,rows,Ld] = src [B,rows,Ls] over lens[b] mul + add columns); the rest
    LN_SENTINEL."""
    lib = load_test_library()
    styles, src = _f32(styles), _f32(src)
    B, R, Ls = src.shape
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    fill = np.zeros((B, 640, T), dtype=np.float32)
    cp = np.zeros((B, R, Ld), dtype=np.float32)
    _err_call(lib.kx_test_rows, device, _ptr(styles), _ptr(ln), B, T, _ptr(fill), _ptr(src), R, Ls, Ld, mul, add, _ptr(cp))
    return fill, cp


def attention(qkv, lens, device=0):
    """qkv [B,2304,T] (rows Q|K|V, 12 heads x 64 each), lens [B] -> ctx [B,768,T] (ALBERT self-attention)."""
    lib = load_test_library()
    qkv = _f32(qkv)
    B, C, T = qkv.shape
    assert C == 2304
    lens = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    ctx = np.zeros((B, 768, T), dtype=np.float32)
    _err_call(lib.kx_test_attention, device, _ptr(qkv), _ptr(lens), B, T, _ptr(ctx))
    return ctx


def harmonic_source(f0, lin_w, lin_b, seed=0, utt_base=0, noise_off=False, device=0):
    """f0 [B,2F] -> har_source [B,600F]."""
    lib = load_test_library()
    f0 = _f32(f0)
    B, F2 = f0.shape
    lin_w = _f32(np.asarray(lin_w).reshape(-1))
    out = np.zeros((B, 300 * F2), dtype=np.float32)
    _err_call(lib.kx_test_source, device, _ptr(f0), B, F2, _ptr(lin_w), float(lin_b), seed, utt_base,
              1 if noise_off else 0, _ptr(out))
    return out


def harmonic_source_ragged(f0, frames, lin_w, lin_b, seed=0, utt_base=0, utt_seeds=None, utt_index=None, noise_off=False, device=0):
    """f0 [B,2 Fmax], utterance b valid for 2 frames[b] steps -> har_source [B,600 Fmax], LN_SENTINEL from sample 600 frames[b] on
    (kx_test_source_ragged).  utt_seeds / utt_index [B]: the dispatcher's per-utterance noise keys (utt_index None beside
    utt_seeds: utterance 0 of every seed); without utt_seeds row b draws (seed, utt_base + b)."""
    lib = load_test_library()
    f0 = _f32(f0)
    B, F2 = f0.shape
    assert F2 % 2 == 0
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    assert fr.shape == (B,)
    sd = None if utt_seeds is None else np.ascontiguousarray(utt_seeds, dtype=np.uint64)
    ix = None if utt_index is None else np.ascontiguousarray(utt_index, dtype=np.uint32)
    assert (sd is None or sd.shape == (B,)) and (ix is None or ix.shape == (B,))
    lin_w = _f32(np.asarray(lin_w).reshape(-1))
    assert lin_w.shape == (9,)
    out = np.zeros((B, 300 * F2), dtype=np.float32)
    _err_call(lib.kx_test_source_ragged, device, _ptr(f0), _ptr(fr), B, F2 // 2, _ptr(lin_w), float(lin_b), seed, utt_base, _ptr(sd),
              _ptr(ix), 1 if noise_off else 0, _ptr(out))
    return out


def stft(hs, frames, variant, device=0):
    """stft_kernel alone (kx_test_stft): hs [B,hs_ld], utterance b valid for 600 frames[b] samples, hs_ld >= 600 max(frames)
    -> har [B,22,120 Fmax + 1] (magnitudes | phases), LN_SENTINEL from column 120 frames[b] + 1 on."""
    lib = load_test_library()
    hs = _f32(hs)
    B, hs_ld = hs.shape
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    assert fr.shape == (B,)
    Fmax = int(fr.max())
    har = np.zeros((B, 22, 120 * Fmax + 1), dtype=np.float32)
    _err_call(lib.kx_test_stft, device, _ptr(hs), B, hs_ld, _ptr(fr), Fmax, variant, _ptr(har))
    return har


def istft_head(cp, frames, variant, device=0):
    """istft_spec_kernel and istft_ola_kernel (kx_test_istft_head): cp [B,22,120 Fmax + 1] (log-magnitudes | phase logits),
    utterance b valid for 120 frames[b] + 1 columns -> (spec [B,22,120 Fmax + 1] = real | imaginary rows as the first kernel
    stored them, audio [B,600 Fmax]); LN_SENTINEL past an utterance's own length in both."""
    lib = load_test_library()
    cp = _f32(cp)
    B, R, nfmax = cp.shape
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    Fmax = int(fr.max())
    assert R == 22 and nfmax == 120 * Fmax + 1 and fr.shape == (B,)
    spec = np.zeros((B, 22, nfmax), dtype=np.float32)
    audio = np.zeros((B, 600 * Fmax), dtype=np.float32)
    _err_call(lib.kx_test_istft_head, device, _ptr(cp), B, _ptr(fr), Fmax, variant, _ptr(spec), _ptr(audio))
    return spec, audio


def pool_up2(x, lens, norm, w, bias, slope, n_bs=None, device=0):
    """pool_up2_kernel alone (kx_test_pool_up2): x [B,C,L], utterance b valid for lens[b] columns, norm [3,B,C] = (mean, scale,
    shift), w [C,3] (or [C,1,3]), bias [C] -> y [B,C,2 L], LN_SENTINEL from column 2 lens[b] on.  n_bs: the planes' slots per
    utterance (> C; default C + 3)."""
    lib = load_test_library()
    x, norm, bias = _f32(x), _f32(norm), _f32(bias)
    B, C_, L = x.shape
    w = _f32(np.asarray(w, dtype=np.float32).reshape(C_, 3))
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    assert norm.shape == (3, B, C_) and bias.shape == (C_,) and ln.shape == (B,)
    y = np.zeros((B, C_, 2 * L), dtype=np.float32)
    _err_call(lib.kx_test_pool_up2, device, _ptr(x), B, C_, L, _ptr(ln), _ptr(norm), C_ + 3 if n_bs is None else n_bs, _ptr(w), _ptr(bias),
              float(slope), _ptr(y))
    return y


def weight_images(sources, up_stride=0, device=0):
    """The weight images of one layer from the model's packers (kx_test_weight_images): `sources` = one to three float32 arrays
    [rows_i, Cin, K], row-concatenated as the fused layers are, or, with up_stride = s, one transposed-conv weight [Cin, Cout, 2 s].
    Returns a dict: BM, rows, n_chunks, n_chunks16, K, unscale, and the raw bytes (uint8 arrays) of w, w16, w16b and w8x -- length
    0 for an image the layer does not get."""
    lib = load_test_library()
    if isinstance(sources, np.ndarray):
        sources = [sources]
    src = [_f32(a) for a in sources]
    assert all(a.ndim == 3 for a in src)
    if up_stride:
        Cin, rows, K = src[0].shape
        src_rows = [rows]
        rows *= up_stride
    else:
        _, Cin, K = src[0].shape
        assert all(a.shape[1:] == (Cin, K) for a in src)
        src_rows = [a.shape[0] for a in src]
        rows = sum(src_rows)
    # (rows padded to at most 128, channels to 16, taps to groups of 4, at most 4 bytes per weight and image)
    cap = (rows + 127) * (Cin + 15) * (K + 3) * 4
    bufs = [np.zeros(cap, dtype=np.uint8) for _ in range(4)]
    ptrs = (C.c_void_p * len(src))(*[a.ctypes.data for a in src])
    outs = (C.c_void_p * 4)(*[b.ctypes.data for b in bufs])
    caps = np.full(4, cap, dtype=np.int64)
    rws = np.array(src_rows, dtype=np.int32)
    meta = np.zeros(9, dtype=np.int64)
    unscale = np.zeros(1, dtype=np.float32)
    _err_call(lib.kx_test_weight_images, device, ptrs, _ptr(rws), len(src), Cin, K, int(up_stride), _ptr(meta), _ptr(unscale), outs, _ptr(caps))
    out = dict(zip(("BM", "rows", "n_chunks", "n_chunks16", "K"), (int(v) for v in meta[:5])))
    out["unscale"] = float(unscale[0])
    for i, name in enumerate(("w", "w16", "w16b", "w8x")):
        out[name] = bufs[i][: int(meta[5 + i])].copy()
    return out


def _output_plan(audio, frames, dur, lens, chunks_per_request, formats, joins, want, pauses, device, levels=None, loudness=None, limits=None,
                 flac=False):
    """kx_test_output_plan, the one hook of the output stage: the model's planner and launcher on host arrays (None where the
    hook takes a null pointer; include/kokorox_hip_test.h).  Returns (bodies as bytes, out_samples, marks as int64 arrays).
    levels (an array of LEVEL_DTYPE, [R]): kx_test_output_plan_levelled, and a fourth entry, the levels as float64 [R, 2].
    loudness (an array of LOUDNESS_DTYPE, [R]; levels may then be None): kx_test_output_plan_loudness, and the fourth entry is
    the pair (loudness as float64 [R, 4] = p, g, I, n_g; the hop energies e[k] of every request as one float64 array each).
    limits (an array of LIMIT_DTYPE, [R]; levels and loudness may then be None): kx_test_output_plan_limited, and the fourth entry
    is the triple (levels [R, 2] or None, loudness [R, 4] or None, limits as float64 [R, 5] = p, g, I, n_g, r, the rows of the
    requests without a limiter left at -1).
    flac = True: kx_test_output_plan_flac whatever else is given, and the fourth entry is (the lengths block as int64 [R], levels
    [R, 2] or None, loudness [R, 4] or None, limits [R, 5] or None); the bodies are cut by the true sizes."""
    lib = load_test_library()
    B = len(frames if dur is None else lens)
    fm = np.ascontiguousarray(formats, dtype=np.int32)
    cpr = None if chunks_per_request is None else np.ascontiguousarray(chunks_per_request, dtype=np.int32)
    R = B if cpr is None else cpr.shape[0]
    if dur is None:
        fr, ln, n_frames, mcap = np.ascontiguousarray(frames, dtype=np.int32), None, int(np.sum(frames)), 0
        assert fr.shape == (B,)
    else:
        dur = np.ascontiguousarray(dur, dtype=np.int32)
        fr, ln = None, np.ascontiguousarray(lens, dtype=np.int32)
        assert dur.shape == (B, 512)
        n_frames, mcap = int(sum(int(dur[b, : ln[b]].sum()) for b in range(B))), int(ln.sum()) + B
    wt = None if want is None else np.ascontiguousarray(want, dtype=np.uint8)
    assert fm.shape == (R,) and (wt is None or wt.shape == (R,))
    ld, cap = 0, 0
    if audio is not None:
        audio = _f32(audio)
        assert audio.shape[0] == B
        ld = audio.shape[1]
        cap = 16 * (600 * n_frames + pauses) + 64 * R  # (stereo f32 at 48 kHz: 16 bytes per sample of the model)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    mk = np.zeros(max(mcap, 1), dtype=np.int64)
    nb, ns, nm = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    args = (device, _ptr(audio), B, ld, _ptr(fr), _ptr(dur), _ptr(ln), _ptr(cpr), R, _ptr(fm), _ptr(joins), _ptr(wt),
            _ptr(out) if audio is not None else None, cap, _ptr(nb), _ptr(ns), _ptr(mk), mcap, _ptr(nm))
    if flac:
        assert audio is not None
        out_lv = np.zeros((R, 2), dtype=np.float64) if levels is not None else None
        out_ld = np.full((R, 4), -1.0, dtype=np.float64) if loudness is not None else None
        out_lm = np.full((R, 5), -1.0, dtype=np.float64) if limits is not None else None
        hcap = (600 * n_frames + pauses) // 1200 + 1 if loudness is not None else 0
        hops, n_hops = (np.zeros((R, hcap), dtype=np.float64), np.zeros(R, dtype=np.int64)) if loudness is not None else (None, None)
        lengths = np.full(R, -1, dtype=np.int64)
        _err_call(lib.kx_test_output_plan_flac, *args, _ptr(levels), _ptr(out_lv), _ptr(loudness), _ptr(out_ld), _ptr(hops), hcap,
                  _ptr(n_hops), _ptr(limits), _ptr(out_lm), _ptr(lengths))
    elif limits is not None:
        assert limits.dtype == LIMIT_DTYPE and limits.shape == (R,) and (levels is None or (levels.dtype == LEVEL_DTYPE and levels.shape == (R,)))
        assert loudness is None or (loudness.dtype == LOUDNESS_DTYPE and loudness.shape == (R,))
        out_lv = np.zeros((R, 2), dtype=np.float64) if levels is not None else None
        out_ld = np.full((R, 4), -1.0, dtype=np.float64) if loudness is not None else None
        out_lm = np.full((R, 5), -1.0, dtype=np.float64)
        hcap = (600 * n_frames + pauses) // 1200 + 1 if loudness is not None else 0
        hops, n_hops = (np.zeros((R, hcap), dtype=np.float64), np.zeros(R, dtype=np.int64)) if loudness is not None else (None, None)
        _err_call(lib.kx_test_output_plan_limited, *args, _ptr(levels), _ptr(out_lv), _ptr(loudness), _ptr(out_ld), _ptr(hops), hcap,
                  _ptr(n_hops), _ptr(limits), _ptr(out_lm))
    elif loudness is not None:
        assert loudness.dtype == LOUDNESS_DTYPE and loudness.shape == (R,) and (levels is None or (levels.dtype == LEVEL_DTYPE and levels.shape == (R,)))
        out_lv = np.zeros((R, 2), dtype=np.float64)
        out_ld = np.full((R, 4), -1.0, dtype=np.float64)
        hcap = (600 * n_frames + pauses) // 1200 + 1  # (a hop is 100 ms: 2400 samples of the model, 1200 if everything ran at 48 kHz)
        hops, n_hops = np.zeros((R, hcap), dtype=np.float64), np.zeros(R, dtype=np.int64)
        _err_call(lib.kx_test_output_plan_loudness, *args, _ptr(levels), _ptr(out_lv) if levels is not None else None, _ptr(loudness),
                  _ptr(out_ld), _ptr(hops), hcap, _ptr(n_hops))
    elif levels is None:
        _err_call(lib.kx_test_output_plan, *args)
    else:
        assert levels.dtype == LEVEL_DTYPE and levels.shape == (R,)
        out_lv = np.zeros((R, 2), dtype=np.float64)
        _err_call(lib.kx_test_output_plan_levelled, *args, _ptr(levels), _ptr(out_lv))
    raw, res, o = out.tobytes(), [], 0
    for r in range(R):
        res.append(raw[o: o + int(nb[r])] if audio is not None else b"")
        o += int(nb[r])
    marks = [m.copy() for m in np.split(mk[: int(nm.sum())], np.cumsum(nm)[:-1])]
    if flac:
        return res, [int(v) for v in ns], marks, (lengths, out_lv, out_ld, out_lm)
    if limits is not None:
        return res, [int(v) for v in ns], marks, (out_lv, out_ld, out_lm)
    if loudness is not None:
        return res, [int(v) for v in ns], marks, (out_ld, [hops[r, : int(n_hops[r])].copy() for r in range(R)])
    if levels is not None:
        return res, [int(v) for v in ns], marks, out_lv
    return res, [int(v) for v in ns], marks


def pack_requests(audio, frames, chunks_per_request, formats, device=0):
    """The request packer alone: audio [B, audio_ld] with row b valid for 600 * frames[b] samples,
    request r = chunks_per_request[r] consecutive rows in the format word formats[r] (the resampler runs first where a word
    has a rate code).  chunks_per_request = None: every row a request of its own (a null pointer to the planner, as the
    per-utterance entries of the model pass it); one word in `formats` then serves all rows.  Returns the R regions as bytes."""
    fm = np.ascontiguousarray(formats, dtype=np.int32)
    if chunks_per_request is None and fm.shape == (1,):
        fm = np.repeat(fm, len(frames))
    return _output_plan(audio, frames, None, None, chunks_per_request, fm, None, None, 0, device)[0]


def token_marks(dur, lens, chunks_per_request, formats, want=None, device=0):
    """The token marks alone: dur [B, 512] int32 frames per token, row b valid for lens[b] entries,
    request r = chunks_per_request[r] consecutive rows in the format word formats[r]; want [R] = which requests get marks
    (None: all).  Returns one int64 array per request (empty where not wanted): voices.token_marks of the same durations."""
    want = np.ones(len(chunks_per_request), dtype=np.uint8) if want is None else want
    return _output_plan(None, None, dur, lens, chunks_per_request, formats, None, want, 0, device)[2]


def join_requests(audio, dur, lens, chunks_per_request, formats, joins, want=None, device=0):
    """Joined requests alone: audio [B, audio_ld] (None: the marks alone), dur [B, 512] int32 frames per
    token with row b valid for lens[b] entries and 600 * their sum samples of audio, request r = chunks_per_request[r]
    consecutive rows in the format word formats[r] with the join spec joins[r]; want [R] = which requests get marks (None:
    none).  Returns (bodies as bytes, out_samples, marks): voices.join_stream -> resample_stream -> the form mirrors, and
    voices.joined_marks (an empty array where not wanted)."""
    R = len(chunks_per_request)
    j = join_specs(joins, R)
    pauses = sum(24 * int(j["pause_ms"][r]) * (int(chunks_per_request[r]) - 1) for r in range(R))
    return _output_plan(audio, None, dur, lens, chunks_per_request, formats, j, want, pauses, device)


def level_requests(audio, dur, lens, chunks_per_request, formats, levels, joins=None, want=None, frames=None, device=0):
    """Levelled requests alone (kx_test_output_plan_levelled): audio, dur, lens, chunks_per_request, formats, joins and want as
    join_requests takes them (joins = None: the rows appended as they are; dur = lens = None with frames [B]: the frame counts
    given, then neither joins nor marks), levels = one (mode, gain, peak) spec per request.  Returns (bodies as bytes,
    out_samples, marks, levels as float64 [R, 2] = p and g of every request): voices.levelled_body and voices.level_gain."""
    R = len(lens if dur is not None else frames) if chunks_per_request is None else len(chunks_per_request)
    lv = level_specs(levels, R)
    j = None if joins is None else join_specs(joins, R)
    pauses = 0 if j is None else sum(24 * int(j["pause_ms"][r]) * (int(chunks_per_request[r]) - 1) for r in range(R))
    return _output_plan(audio, frames, dur, lens, chunks_per_request, formats, j, want, pauses, device, lv)


def loudness_requests(audio, dur, lens, chunks_per_request, formats, loudness, joins=None, want=None, frames=None, levels=None, device=0):
    """Metered requests alone (kx_test_output_plan_loudness): everything as level_requests takes it, loudness = one (mode,
    target_lufs, peak) spec per request, LOUDNESS_NONE for a request that is not metered (its level spec, if `levels` is given,
    then applies; a metered request's level spec is the plain one).  Returns (bodies as bytes, out_samples, marks, loudness as
    float64 [R, 4] = p, g, I and n_g of every request, the hop energies e[k] of every request): voices.loudness_body,
    voices.integrated_loudness, voices.loudness_gain and voices.hop_energies."""
    R = len(lens if dur is not None else frames) if chunks_per_request is None else len(chunks_per_request)
    ld = loudness_specs(loudness, R)
    lv = None if levels is None else level_specs(levels, R)
    j = None if joins is None else join_specs(joins, R)
    pauses = 0 if j is None else sum(24 * int(j["pause_ms"][r]) * (int(chunks_per_request[r]) - 1) for r in range(R))
    res, ns, marks, (out_ld, hops) = _output_plan(audio, frames, dur, lens, chunks_per_request, formats, j, want, pauses, device, lv, ld)
    return res, ns, marks, out_ld, hops


def limit_requests(audio, dur, lens, chunks_per_request, formats, limits, joins=None, want=None, frames=None, levels=None, loudness=None,
                   device=0):
    """Limited requests alone (kx_test_output_plan_limited): everything as loudness_requests takes it, limits = one (mode, gain,
    target_lufs, peak) spec per request, LIMIT_NONE for a request without a limiter (its level or loudness spec, if given, then
    applies; a limited request's level spec is the plain one and its loudness spec LOUDNESS_NONE).  Returns (bodies as bytes,
    out_samples, marks, limits as float64 [R, 5] = p, g, I, n_g and r of every limited request, levels [R, 2] or None, loudness
    [R, 4] or None): voices.limited_body and voices.limit_stream."""
    R = len(lens if dur is not None else frames) if chunks_per_request is None else len(chunks_per_request)
    lm = limit_specs(limits, R)
    ld = None if loudness is None else loudness_specs(loudness, R)
    lv = None if levels is None else level_specs(levels, R)
    j = None if joins is None else join_specs(joins, R)
    pauses = 0 if j is None else sum(24 * int(j["pause_ms"][r]) * (int(chunks_per_request[r]) - 1) for r in range(R))
    res, ns, marks, (out_lv, out_ld, out_lm) = _output_plan(audio, frames, dur, lens, chunks_per_request, formats, j, want, pauses, device,
                                                            lv, ld, lm)
    return res, ns, marks, out_lm, out_lv, out_ld


def flac_requests(audio, dur, lens, chunks_per_request, formats, joins=None, want=None, frames=None, levels=None, loudness=None,
                  limits=None, device=0):
    """Requests through kx_test_output_plan_flac: everything as limit_requests takes it, every spec list optional, and any mix of
    forms, 12 (FLAC) among them.  Returns (bodies as bytes, cut by their true sizes, out_samples, marks, lengths = the lengths block
    as int64 [R], levels [R, 2] or None, loudness [R, 4] or None, limits [R, 5] or None): voices.flac_body of the 16-bit samples of
    the same request.  The hook itself checks the guards and the poisoned slack of every region."""
    R = len(lens if dur is not None else frames) if chunks_per_request is None else len(chunks_per_request)
    lm = None if limits is None else limit_specs(limits, R)
    ld = None if loudness is None else loudness_specs(loudness, R)
    lv = None if levels is None else level_specs(levels, R)
    j = None if joins is None else join_specs(joins, R)
    pauses = 0 if j is None else sum(24 * int(j["pause_ms"][r]) * (int(chunks_per_request[r]) - 1) for r in range(R))
    res, ns, marks, (lengths, out_lv, out_ld, out_lm) = _output_plan(audio, frames, dur, lens, chunks_per_request, formats, j, want, pauses,
                                                                     device, lv, ld, lm, flac=True)
    return res, ns, marks, lengths, out_lv, out_ld, out_lm


def piece_requests(audio, dur, lens, chunks_per_request, formats, piece_flags, carries=None, joins=None, want=None, levels=None,
                   loudness=None, device=0):
    """Pieces through kx_test_output_plan_pieces: audio, dur, lens, chunks_per_request, formats, joins, want and levels as
    level_requests takes them (levels and joins may be None), piece_flags = one flag word per request (PIECE_WHOLE: run whole),
    carries = what the pieces before left (None = zeros; see piece_carries), loudness = one spec per request or None (LOUDNESS_NONE
    for every piece).  Returns (payloads as bytes, out_samples, marks, carries as an array of PIECE_CARRY_DTYPE, levels [R, 2] or None,
    loudness [R, 4] or None): voices.piece_bodies, voices.joined_marks and voices.piece_carry.  The hook itself checks the guards
    around the carry block and behind the bodies."""
    lib = load_test_library()
    cpr = np.ascontiguousarray(chunks_per_request, dtype=np.int32)
    R, B = cpr.shape[0], len(lens)
    fm = np.ascontiguousarray(formats, dtype=np.int32)
    pf = np.ascontiguousarray(piece_flags, dtype=np.uint32)
    assert fm.shape == (R,) and pf.shape == (R,)
    lv = None if levels is None else level_specs(levels, R)
    ld = None if loudness is None else loudness_specs(loudness, R)
    j = None if joins is None else join_specs(joins, R)
    cin, cout = piece_carries(carries, R), np.zeros(R, PIECE_CARRY_DTYPE)
    audio = _f32(audio)
    dur, ln = np.ascontiguousarray(dur, dtype=np.int32), np.ascontiguousarray(lens, dtype=np.int32)
    assert dur.shape == (B, 512) and audio.shape[0] == B
    n_frames = int(sum(int(dur[b, : ln[b]].sum()) for b in range(B)))
    pauses = 0 if j is None else sum(24 * int(j["pause_ms"][r]) * int(cpr[r]) for r in range(R))
    cap = 16 * (600 * n_frames + pauses) + 1024 * R  # (stereo f32 at 48 kHz; a piece also emits what the ones before held back)
    mcap = int(ln.sum()) + B
    wt = None if want is None else np.ascontiguousarray(want, dtype=np.uint8)
    out, mk = np.zeros(cap, dtype=np.uint8), np.zeros(mcap, dtype=np.int64)
    nb, ns, nm = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    out_lv = None if lv is None else np.zeros((R, 2), dtype=np.float64)
    out_ld = None if ld is None else np.full((R, 4), -1.0, dtype=np.float64)
    _err_call(lib.kx_test_output_plan_pieces, device, _ptr(audio), B, audio.shape[1], None, _ptr(dur), _ptr(ln), _ptr(cpr), R, _ptr(fm),
              _ptr(j), _ptr(wt), _ptr(out), cap, _ptr(nb), _ptr(ns), _ptr(mk), mcap, _ptr(nm), _ptr(lv), _ptr(out_lv), _ptr(ld),
              _ptr(out_ld), _ptr(pf), _ptr(cin), _ptr(cout))
    raw, res, o = out.tobytes(), [], 0
    for r in range(R):
        res.append(raw[o: o + int(nb[r])])
        o += int(nb[r])
    marks = [m.copy() for m in np.split(mk[: int(nm.sum())], np.cumsum(nm)[:-1])]
    return res, [int(v) for v in ns], marks, cout, out_lv, out_ld
