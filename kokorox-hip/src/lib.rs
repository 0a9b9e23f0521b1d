//! `kokorox-hip`: drop-in for `kokorox::onn::ort_koko::OrtKoko` on AMD MI355X (gfx950).
//!
//! The reference runs the Kokoro-82M graph through ONNX Runtime (`ort::Session::run`,
//! kokorox/src/onn/ort_koko.rs:79).  This crate binds `libkokorox_hip.so` (include/kokorox_hip.h), whose forward
//! pass is hand-written CDNA4 HIP, and exposes the same two public operations with the same signatures:
//!
//! ```text
//! OrtKoko::new(model_path: String) -> Result<Self, String>                               ort_koko.rs:31-35
//! OrtKoko::infer(&self, tokens: Vec<Vec<i64>>, styles: Vec<Vec<f32>>, speed: f32)
//!     -> Result<ArrayBase<OwnedRepr<f32>, IxDyn>, Box<dyn Error>>                        ort_koko.rs:37-91
//! ```
//!
//! Change in the reference: `use kokorox_hip::HipKoko as OrtKoko;` at kokorox/src/tts/koko.rs:40,570-573 and
//! `kokorox_hip::init(0)` in place of `init_ort` (koko/src/main.rs:1429).  `model_path` stays what the reference
//! passes: the Hugging Face `onnx/model.onnx` (kokorox/src/utils/hf_cache.rs:128-158; the fp16 / int8 / 4-bit
//! variants of hf_cache.rs:135-144 load too, de-quantised).  The library reads the ONNX initialisers itself (no ONNX
//! Runtime, no protobuf crate); a pre-converted `KXHIPW01` container (`import_onnx` below, or
//! `python -m kokorox_amd.importer`) is recognised by its magic and skips the conversion.
#![allow(clippy::too_many_arguments)]

use ndarray::{ArrayBase, IxDyn, OwnedRepr};
use std::error::Error;
use std::ffi::{c_char, c_int, c_void, CStr, CString};
use std::ptr;

pub const KX_OK: c_int = 0;
pub const KX_STYLE_DIM: usize = 256;
pub const KX_SAMPLES_PER_FRAME: usize = 600;
pub const KX_FLAG_NOISE_OFF: u32 = 1;
pub const KX_PACK_F32_MONO: c_int = 0;
pub const KX_PACK_F32_STEREO: c_int = 1;
pub const KX_PACK_PCM16_MONO: c_int = 2;
/// The HTTP body: 44-byte float WAV header + f32 samples (kokorox-openai/src/lib.rs:416-425); requests only.
pub const KX_PACK_WAV_F32: c_int = 3;
/// The WebSocket chunk: base64 of a 16-bit WAV file (`encode_audio`, kokorox-websocket/src/lib.rs:696-736); requests only.
pub const KX_PACK_WAV16_BASE64: c_int = 4;
/// Raw G.711 mu-law / A-law of the 16-bit sample, one byte per sample, no header; requests only.
pub const KX_PACK_MULAW: c_int = 8;
pub const KX_PACK_ALAW: c_int = 9;
/// FLAC of the 16-bit samples, lossless; the body's size follows from the samples (`kokorox_hip.h`, "FLAC").
pub const KX_PACK_FLAC: c_int = 12;
/// IMA ADPCM in a WAV file, 4 bits per sample, blocks encoded on the GPU (`kokorox_hip.h`, "IMA ADPCM"); the form's number is the
/// WAV format tag it carries.
pub const KX_PACK_ADPCM_WAV: c_int = 17;
/// The largest block of `KX_PACK_ADPCM_WAV`, at 48 000 Hz.
pub const KX_ADPCM_MAX_BLOCK: c_int = 1024;
/// The plain 16-bit WAV file as bytes: what `KX_PACK_WAV16_BASE64` encodes, padded with zeros to a multiple of 4.
pub const KX_PACK_WAV16: c_int = 18;
/// The output sample rate, or'ed into a request's form (bits 8..11 of the format word; 0 = the model's 24 000 Hz).
pub const KX_PACK_RATE_24000: c_int = 0x000;
pub const KX_PACK_RATE_8000: c_int = 0x100;
pub const KX_PACK_RATE_16000: c_int = 0x200;
pub const KX_PACK_RATE_48000: c_int = 0x300;
pub const KX_RESAMPLE_MAX_TAPS: usize = 145;
/// Join flags ("joins" in kokorox_hip.h): trim the request's lead-in, its tail, the pad spans at every boundary between chunks.
pub const KX_JOIN_TRIM_HEAD: u32 = 1;
pub const KX_JOIN_TRIM_TAIL: u32 = 2;
pub const KX_JOIN_TRIM_INNER: u32 = 4;

/// How a request's seams are shaped on the GPU (`kx_join`): of a trimmed pad span at most `keep_ms` stays (0..1000),
/// `pause_ms` of zeros between consecutive chunks (0..5000), a linear fade of `fade_ms` at every trimmed edge (0..12).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct KxJoin {
    pub flags: u32,
    pub keep_ms: i32,
    pub pause_ms: i32,
    pub fade_ms: i32,
}

pub const KX_LEVEL_GAIN: u32 = 0;
pub const KX_LEVEL_NORMALIZE: u32 = 1;
pub const KX_LEVEL_CEILING: u32 = 2;

/// How a request's level is set on the GPU (`kx_level`; "levels" in kokorox_hip.h): mode 0 multiplies by `gain` (0..64, `peak`
/// +0.0), mode 1 scales so that the body's largest |sample| is `peak` (2^-15..1, `gain` 1.0), mode 2 multiplies by `gain` but
/// never lets the largest |sample| exceed `peak`.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct KxLevel {
    pub mode: u32,
    pub gain: f32,
    pub peak: f32,
}

/// A request run in pieces ("pieces" in kokorox_hip.h): the flag bits of a piece, and the record one piece leaves for the next
/// (`kx_piece_carry`, 1056 bytes).  The payloads of a request's pieces, end to end, are the body of the request run whole.
pub const KX_PIECE_FIRST: u32 = 1;
pub const KX_PIECE_LAST: u32 = 2;
pub const KX_PIECE_TAIL: usize = 256;
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct KxPieceCarry {
    pub magic: u32,
    pub format_word: u32,
    pub src_samples: i64,
    pub out_samples: i64,
    pub n_tail: i32,
    pub reserved: i32,
    pub tail: [f32; KX_PIECE_TAIL],
}

impl KxPieceCarry {
    /// What a first piece is given: nothing of it is read.
    pub const EMPTY: KxPieceCarry =
        KxPieceCarry { magic: 0, format_word: 0, src_samples: 0, out_samples: 0, n_tail: 0, reserved: 0, tail: [0.0; KX_PIECE_TAIL] };
}

impl KxLevel {
    /// The plain spec: the samples as they are (through the levelled entries: a peak meter).
    pub const PLAIN: KxLevel = KxLevel { mode: KX_LEVEL_GAIN, gain: 1.0, peak: 0.0 };
}

/// OR-ed into a `KxLevel` or `KxLoudness` mode: `peak` bounds the true peak of the body (four times oversampled), and the
/// reported p is that true peak ("levels" in kokorox_hip.h, True peak).
pub const KX_PEAK_TRUE: u32 = 0x100;

/// The 72 taps of the true-peak interpolator as [3][24], phase 1 first (host only).
pub fn truepeak_filter() -> Result<[[f32; 24]; 3], Box<dyn Error>> {
    let mut t = [[0f32; 24]; 3];
    match unsafe { kx_truepeak_filter(t.as_mut_ptr() as *mut f32, 72) } {
        KX_OK => Ok(t),
        rc => Err(format!("kokorox_hip error {}: kx_truepeak_filter", rc).into()),
    }
}

/// The block of `KX_PACK_ADPCM_WAV` at the rate of a format word: (bytes of a block, samples of a block); host only.
pub fn adpcm_block(format_word: c_int) -> Result<(i32, i32), Box<dyn Error>> {
    let (mut a, mut p) = (0i32, 0i32);
    match unsafe { kx_adpcm_block(format_word, &mut a, &mut p) } {
        KX_OK => Ok((a, p)),
        rc => Err(format!("kokorox_hip error {}: kx_adpcm_block", rc).into()),
    }
}

pub const KX_LOUDNESS_MEASURE: u32 = 0;
pub const KX_LOUDNESS_NORMALIZE: u32 = 1;

/// How a request's loudness is measured and set on the GPU (`kx_loudness`; "loudness" in kokorox_hip.h): mode 0 measures the
/// integrated loudness of ITU-R BS.1770 (`target_lufs` and `peak` +0.0), mode 1 scales the body to `target_lufs` (-70..0) but
/// never lets its largest |sample| exceed `peak` (2^-15..1).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct KxLoudness {
    pub mode: u32,
    pub target_lufs: f32,
    pub peak: f32,
}

impl KxLoudness {
    /// The meter: the samples as they are, their loudness measured.
    pub const METER: KxLoudness = KxLoudness { mode: KX_LOUDNESS_MEASURE, target_lufs: 0.0, peak: 0.0 };
}

/// The ten K-weighting coefficients of a format word's rate: shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2 (host only).
pub fn loudness_filter(format_word: c_int) -> Result<[f64; 10], Box<dyn Error>> {
    let mut c = [0f64; 10];
    match unsafe { kx_loudness_filter(format_word, c.as_mut_ptr()) } {
        KX_OK => Ok(c),
        rc => Err(format!("kokorox_hip error {}: unknown output format or sample rate", rc).into()),
    }
}

pub const KX_LIMIT_GAIN: u32 = 0;
pub const KX_LIMIT_LOUDNESS: u32 = 1;
pub const KX_LIMIT_MAX_TAPS: usize = 481;

/// How a request's body is driven and peak-limited on the GPU (`kx_limit`; "limiter" in kokorox_hip.h): mode 0 drives it by
/// `gain` (0..64, `target_lufs` +0.0), mode 1 to `target_lufs` (-70..0, `gain` exactly 1.0) as `KX_LOUDNESS_NORMALIZE` does; a
/// look-ahead gain of 5 ms either side then keeps every sample at or below `peak` (2^-15..1) by turning down only the
/// neighbourhood of the samples that would pass it.  `KX_PEAK_TRUE` may be OR-ed into the mode: the limiter then follows the
/// four-times oversampled envelope.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct KxLimit {
    pub mode: u32,
    pub gain: f32,
    pub target_lufs: f32,
    pub peak: f32,
}

/// The limiter's window W = fs / 200 and its 2 W + 1 smoothing weights at a format word's rate (host only).
pub fn limit_filter(format_word: c_int) -> Result<(usize, Vec<f32>), Box<dyn Error>> {
    let mut w = 0i32;
    let mut taps = vec![0f32; KX_LIMIT_MAX_TAPS];
    match unsafe { kx_limit_filter(format_word, &mut w, taps.as_mut_ptr(), KX_LIMIT_MAX_TAPS as c_int) } {
        KX_OK => {
            taps.truncate(2 * w as usize + 1);
            Ok((w as usize, taps))
        }
        rc => Err(format!("kokorox_hip error {}: unknown output format or sample rate", rc).into()),
    }
}

pub const KX_PROSODY_MAX_FRAMES: i32 = 50;

/// Per-token prosody of a call (`kx_prosody`; "prosody" in kokorox_hip.h): every pointer is null (neutral) or `[B, t_stride]`
/// laid out as the ids.  `rate` 0.25..4 divides the durations, `frames` 0 (as predicted) or 1..50 fixes them, `pitch` 0.25..4 and
/// `energy` 0..4 are ratios on the F0 and N curves.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct KxProsody {
    pub rate: *const f32,
    pub frames: *const i32,
    pub pitch: *const f32,
    pub energy: *const f32,
}

/// The per-token prosody of a call as the safe wrappers take it: each field empty (neutral) or one vector per row with a value
/// per token.
#[derive(Clone, Debug, Default)]
pub struct Prosody {
    pub rate: Vec<Vec<f32>>,
    pub frames: Vec<Vec<i32>>,
    pub pitch: Vec<Vec<f32>>,
    pub energy: Vec<Vec<f32>>,
}

/// One token of a request's prosody report: the mean F0 in Hz over its voiced steps (0 when none), their count, the mean of the
/// N curve over its steps, and its frames.
pub type ProsodyToken = [f32; 4];

fn prosody_rows<V: Copy>(rows: &[Vec<V>], lens: &[i32], stride: usize, neutral: V) -> Result<Vec<V>, Box<dyn Error>> {
    if rows.is_empty() {
        return Ok(Vec::new());
    }
    if rows.len() != lens.len() || rows.iter().zip(lens).any(|(r, &n)| r.len() != n as usize) {
        return Err("prosody: one value per token of every row is required".into());
    }
    let mut flat = vec![neutral; lens.len() * stride];
    for (b, r) in rows.iter().enumerate() {
        flat[b * stride..b * stride + r.len()].copy_from_slice(r);
    }
    Ok(flat)
}

/// A fit span (`kx_fit_span`; "fit" in kokorox_hip.h): tokens `[begin, end)` of request `request`, its chunks laid end to end,
/// get durations that add up to exactly `frames` frames of 25 ms.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct KxFitSpan {
    pub request: i32,
    pub begin: i32,
    pub end: i32,
    pub frames: i32,
}

/// What the GPU chose for a span (`kx_fit_result`): the factor on its weights (`1 / lambda` is speed-like), its free tokens, the
/// frames of its held tokens and the excess E.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct KxFitResult {
    pub lambda: f32,
    pub n_free: i32,
    pub held_frames: i32,
    pub excess: i32,
}

#[repr(C)]
pub struct KxModel {
    _p: [u8; 0],
}
#[repr(C)]
pub struct KxDispatcher {
    _p: [u8; 0],
}

// One declaration per entry point of include/kokorox_hip.h (test hooks excluded), same order, same arity.
extern "C" {
    fn kx_init(device_id: c_int, err: *mut c_char, err_len: usize) -> c_int;
    fn kx_create(weights_path: *const c_char, device_id: c_int, err: *mut c_char, err_len: usize) -> *mut KxModel;
    fn kx_import_onnx(onnx_path: *const c_char, out_path: *const c_char, err: *mut c_char, err_len: usize) -> c_int;
    fn kx_resample_filter(format_word: c_int, l: *mut i32, m: *mut i32, n_taps: *mut i32, taps: *mut f32, cap: c_int) -> c_int;
    fn kx_loudness_filter(format_word: c_int, out10: *mut f64) -> c_int;
    fn kx_truepeak_filter(taps: *mut f32, cap: c_int) -> c_int;
    fn kx_adpcm_block(format_word: c_int, block_bytes: *mut i32, samples_per_block: *mut i32) -> c_int;
    fn kx_infer_requests_loudness(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int,
                                  chunks_per_request: *const i32, r: c_int, styles: *const f32, voice_ids: *const i32,
                                  weights: *const f32, max_mix: c_int, speeds: *const f32, n_speed: c_int, seed: u64, flags: u32,
                                  formats: *const c_int, n_format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                  out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64, joins: *const KxJoin,
                                  n_join: c_int, loudness: *const KxLoudness, n_loudness: c_int, out_loudness: *mut f64) -> c_int;
    fn kx_dispatcher_submit_request_loudness(d: *mut KxDispatcher, ids: *const i64, chunk_tokens: *const i32, n_chunks: c_int,
                                             styles: *const f32, voice_ids: *const i32, weights: *const f32, n_mix: c_int,
                                             speed: f32, seed: u64, format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                             out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64,
                                             join: *const KxJoin, loudness: *const KxLoudness, out_loudness: *mut f64, err: *mut c_char,
                                             err_len: usize) -> c_int;
    fn kx_limit_filter(format_word: c_int, w: *mut i32, taps: *mut f32, cap: c_int) -> c_int;
    fn kx_infer_requests_limited(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int,
                                 chunks_per_request: *const i32, r: c_int, styles: *const f32, voice_ids: *const i32,
                                 weights: *const f32, max_mix: c_int, speeds: *const f32, n_speed: c_int, seed: u64, flags: u32,
                                 formats: *const c_int, n_format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                 out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64, joins: *const KxJoin,
                                 n_join: c_int, limits: *const KxLimit, n_limit: c_int, out_limits: *mut f64) -> c_int;
    fn kx_dispatcher_submit_request_limited(d: *mut KxDispatcher, ids: *const i64, chunk_tokens: *const i32, n_chunks: c_int,
                                            styles: *const f32, voice_ids: *const i32, weights: *const f32, n_mix: c_int,
                                            speed: f32, seed: u64, format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                            out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64,
                                            join: *const KxJoin, limit: *const KxLimit, out_limit: *mut f64, err: *mut c_char,
                                            err_len: usize) -> c_int;
    fn kx_infer_prosody(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int, styles: *const f32,
                        speeds: *const f32, n_speed: c_int, seed: u64, flags: u32, out: *mut *mut f32, out_lens: *mut i64,
                        prosody: *const KxProsody, out_durations: *mut i32) -> c_int;
    fn kx_infer_requests_prosody(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int,
                                 chunks_per_request: *const i32, r: c_int, styles: *const f32, voice_ids: *const i32,
                                 weights: *const f32, max_mix: c_int, speeds: *const f32, n_speed: c_int, seed: u64, flags: u32,
                                 formats: *const c_int, n_format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                 out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64, joins: *const KxJoin,
                                 n_join: c_int, prosody: *const KxProsody, out_report: *mut *mut f32, out_n_report: *mut i64) -> c_int;
    fn kx_infer_requests_fitted(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int,
                                chunks_per_request: *const i32, r: c_int, styles: *const f32, voice_ids: *const i32,
                                weights: *const f32, max_mix: c_int, speeds: *const f32, n_speed: c_int, seed: u64, flags: u32,
                                formats: *const c_int, n_format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64, joins: *const KxJoin,
                                n_join: c_int, prosody: *const KxProsody, out_report: *mut *mut f32, out_n_report: *mut i64,
                                spans: *const KxFitSpan, n_spans: c_int, out_fit: *mut KxFitResult) -> c_int;
    fn kx_dispatcher_submit_request_fitted(d: *mut KxDispatcher, ids: *const i64, chunk_tokens: *const i32, n_chunks: c_int,
                                           styles: *const f32, voice_ids: *const i32, weights: *const f32, n_mix: c_int,
                                           speed: f32, seed: u64, format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                           out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64,
                                           join: *const KxJoin, prosody: *const KxProsody, out_report: *mut *mut f32,
                                           out_n_report: *mut i64, spans: *const KxFitSpan, n_spans: c_int,
                                           out_fit: *mut KxFitResult, err: *mut c_char, err_len: usize) -> c_int;
    fn kx_dispatcher_submit_request_prosody(d: *mut KxDispatcher, ids: *const i64, chunk_tokens: *const i32, n_chunks: c_int,
                                            styles: *const f32, voice_ids: *const i32, weights: *const f32, n_mix: c_int,
                                            speed: f32, seed: u64, format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                            out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64,
                                            join: *const KxJoin, prosody: *const KxProsody, out_report: *mut *mut f32,
                                            out_n_report: *mut i64, err: *mut c_char, err_len: usize) -> c_int;
    fn kx_create_from_device_blob(d_blob: *const c_void, n_bytes: usize, device_id: c_int, err: *mut c_char,
                                  err_len: usize) -> *mut KxModel;
    fn kx_create_replicas(weights_path: *const c_char, device_ids: *const c_int, n: c_int,
                          out_models: *mut *mut KxModel, err: *mut c_char, err_len: usize) -> c_int;
    fn kx_replicas_times(out3: *mut f64) -> c_int;
    fn kx_create_partition(weights_path: *const c_char, device_id: c_int, part: c_int, n_parts: c_int,
                           err: *mut c_char, err_len: usize) -> *mut KxModel;
    fn kx_destroy(m: *mut KxModel);
    fn kx_last_error(m: *const KxModel) -> *const c_char;
    fn kx_last_error_copy(m: *const KxModel, buf: *mut c_char, buf_len: usize) -> c_int;
    fn kx_infer(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int, styles: *const f32,
                speeds: *const f32, n_speed: c_int, seed: u64, flags: u32, out: *mut *mut f32,
                out_lens: *mut i64) -> c_int;
    fn kx_free_audio(p: *mut f32);
    fn kx_infer_device(m: *mut KxModel, d_ids: *const i64, t_stride: i64, lens_host: *const i32, b: c_int,
                       d_styles: *const f32, speeds_host: *const f32, n_speed: c_int, seed: u64, flags: u32,
                       d_audio: *mut f32, audio_ld: i64, d_frames: *mut i32, need_ld: *mut i64) -> c_int;
    fn kx_sync(m: *mut KxModel) -> c_int;
    fn kx_warmup(m: *mut KxModel, b: c_int, n_tokens: c_int, frames_per_token: c_int) -> c_int;
    fn kx_arena_bytes(m: *mut KxModel, out3: *mut i64) -> c_int;
    fn kx_call_times(m: *mut KxModel, out4: *mut f64) -> c_int;
    fn kx_model_status(m: *mut KxModel, out4: *mut i64) -> c_int;
    fn kx_model_info(m: *mut KxModel, out8: *mut i64) -> c_int;
    fn kx_set_pinned_durations(m: *mut KxModel, pattern: *const i32, n: c_int) -> c_int;
    fn kx_set_conv_mode(m: *mut KxModel, mode: c_int) -> c_int;
    fn kx_get_conv_mode(m: *mut KxModel) -> c_int;
    fn kx_set_stft_variant(m: *mut KxModel, variant: c_int) -> c_int;
    fn kx_get_stft_variant(m: *mut KxModel) -> c_int;
    fn kx_set_utterance_base(m: *mut KxModel, utt_base: u64) -> c_int;
    fn kx_set_lanes(m: *mut KxModel, n_lanes: c_int) -> c_int;
    fn kx_profile_enable(m: *mut KxModel, on: c_int) -> c_int;
    fn kx_profile_read(m: *mut KxModel, launches: *mut i64, total_ms: *mut f64, total_flops: *mut f64) -> c_int;
    fn kx_profile_detail(m: *mut KxModel, out: *mut f64, cap_rows: i64, n_rows: *mut i64) -> c_int;
    fn kx_profile_aux(m: *mut KxModel, stats_launches: *mut i64, stats_bytes: *mut f64) -> c_int;
    fn kx_diag_enable(m: *mut KxModel, on: c_int) -> c_int;
    fn kx_diag_count(m: *mut KxModel, n: *mut i64) -> c_int;
    fn kx_diag_get(m: *mut KxModel, i: i64, name: *mut c_char, name_len: usize, vals7: *mut f64) -> c_int;
    fn kx_set_act_prescale(m: *mut KxModel, conv_name: *const c_char, log2_scale: c_int) -> c_int;
    fn kx_set_voice_table(m: *mut KxModel, table: *const f32, n_voices: c_int) -> c_int;
    fn kx_infer_voices(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int,
                       voice_ids: *const i32, weights: *const f32, max_mix: c_int, speeds: *const f32,
                       n_speed: c_int, seed: u64, flags: u32, format: c_int, out: *mut *mut c_void,
                       out_bytes: *mut i64, out_samples: *mut i64) -> c_int;
    fn kx_infer_packed(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int,
                       styles: *const f32, speeds: *const f32, n_speed: c_int, seed: u64, flags: u32,
                       format: c_int, out: *mut *mut c_void, out_bytes: *mut i64, out_samples: *mut i64) -> c_int;
    fn kx_free_packed(p: *mut c_void);
    fn kx_infer_requests(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int,
                         chunks_per_request: *const i32, r: c_int, styles: *const f32, voice_ids: *const i32,
                         weights: *const f32, max_mix: c_int, speeds: *const f32, n_speed: c_int, seed: u64, flags: u32,
                         formats: *const i32, n_format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                         out_samples: *mut i64) -> c_int;
    fn kx_infer_requests_marks(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int,
                               chunks_per_request: *const i32, r: c_int, styles: *const f32, voice_ids: *const i32,
                               weights: *const f32, max_mix: c_int, speeds: *const f32, n_speed: c_int, seed: u64, flags: u32,
                               formats: *const i32, n_format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                               out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64) -> c_int;
    fn kx_infer_requests_joined(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int,
                                chunks_per_request: *const i32, r: c_int, styles: *const f32, voice_ids: *const i32,
                                weights: *const f32, max_mix: c_int, speeds: *const f32, n_speed: c_int, seed: u64, flags: u32,
                                formats: *const i32, n_format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64, joins: *const KxJoin,
                                n_join: c_int) -> c_int;
    fn kx_infer_requests_levelled(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int,
                                  chunks_per_request: *const i32, r: c_int, styles: *const f32, voice_ids: *const i32,
                                  weights: *const f32, max_mix: c_int, speeds: *const f32, n_speed: c_int, seed: u64, flags: u32,
                                  formats: *const i32, n_format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                  out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64, joins: *const KxJoin,
                                  n_join: c_int, levels: *const KxLevel, n_level: c_int, out_levels: *mut f64) -> c_int;
    fn kx_dispatcher_create(models: *mut *mut KxModel, n_models: c_int, max_batch: c_int, max_wait_us: c_int,
                            err: *mut c_char, err_len: usize) -> *mut KxDispatcher;
    fn kx_dispatcher_create_warm(models: *mut *mut KxModel, n_models: c_int, max_batch: c_int, max_wait_us: c_int,
                                 warm_tokens: c_int, warm_frames_per_token: c_int, err: *mut c_char, err_len: usize) -> *mut KxDispatcher;
    fn kx_dispatcher_submit(d: *mut KxDispatcher, ids: *const i64, n_tokens: c_int, style: *const f32, speed: f32,
                            seed: u64, out: *mut *mut f32, out_len: *mut i64, err: *mut c_char,
                            err_len: usize) -> c_int;
    fn kx_dispatcher_submit_ex(d: *mut KxDispatcher, ids: *const i64, n_tokens: c_int, style: *const f32,
                               voice_ids: *const i32, weights: *const f32, n_mix: c_int, speed: f32, seed: u64,
                               format: c_int, out: *mut *mut c_void, out_bytes: *mut i64, out_samples: *mut i64,
                               err: *mut c_char, err_len: usize) -> c_int;
    fn kx_dispatcher_submit_request(d: *mut KxDispatcher, ids: *const i64, chunk_tokens: *const i32, n_chunks: c_int,
                                    styles: *const f32, voice_ids: *const i32, weights: *const f32, n_mix: c_int,
                                    speed: f32, seed: u64, format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                    out_samples: *mut i64, err: *mut c_char, err_len: usize) -> c_int;
    fn kx_dispatcher_submit_request_marks(d: *mut KxDispatcher, ids: *const i64, chunk_tokens: *const i32, n_chunks: c_int,
                                          styles: *const f32, voice_ids: *const i32, weights: *const f32, n_mix: c_int,
                                          speed: f32, seed: u64, format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                          out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64,
                                          err: *mut c_char, err_len: usize) -> c_int;
    fn kx_dispatcher_submit_request_joined(d: *mut KxDispatcher, ids: *const i64, chunk_tokens: *const i32, n_chunks: c_int,
                                           styles: *const f32, voice_ids: *const i32, weights: *const f32, n_mix: c_int,
                                           speed: f32, seed: u64, format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                           out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64,
                                           join: *const KxJoin, err: *mut c_char, err_len: usize) -> c_int;
    fn kx_dispatcher_submit_request_levelled(d: *mut KxDispatcher, ids: *const i64, chunk_tokens: *const i32, n_chunks: c_int,
                                             styles: *const f32, voice_ids: *const i32, weights: *const f32, n_mix: c_int,
                                             speed: f32, seed: u64, format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                             out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64,
                                             join: *const KxJoin, level: *const KxLevel, out_level: *mut f64, err: *mut c_char,
                                             err_len: usize) -> c_int;
    fn kx_infer_requests_pieces(m: *mut KxModel, ids: *const i64, t_stride: i64, lens: *const i32, b: c_int,
                                chunks_per_request: *const i32, r: c_int, styles: *const f32, voice_ids: *const i32,
                                weights: *const f32, max_mix: c_int, speeds: *const f32, n_speed: c_int, seed: u64, flags: u32,
                                formats: *const i32, n_format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64, joins: *const KxJoin,
                                n_join: c_int, levels: *const KxLevel, n_level: c_int, out_levels: *mut f64,
                                piece_flags: *const u32, carry_in: *const KxPieceCarry, carry_out: *mut KxPieceCarry) -> c_int;
    fn kx_dispatcher_submit_request_piece(d: *mut KxDispatcher, ids: *const i64, chunk_tokens: *const i32, n_chunks: c_int,
                                          styles: *const f32, voice_ids: *const i32, weights: *const f32, n_mix: c_int,
                                          speed: f32, seed: u64, format: c_int, out: *mut *mut c_void, out_bytes: *mut i64,
                                          out_samples: *mut i64, out_marks: *mut *mut i64, out_n_marks: *mut i64,
                                          join: *const KxJoin, level: *const KxLevel, out_level: *mut f64, piece_flags: u32,
                                          carry_in: *const KxPieceCarry, carry_out: *mut KxPieceCarry, err: *mut c_char,
                                          err_len: usize) -> c_int;
    fn kx_dispatcher_stats(d: *mut KxDispatcher, n_requests: *mut i64, n_batches: *mut i64,
                           max_batch_seen: *mut i64) -> c_int;
    fn kx_dispatcher_failures(d: *mut KxDispatcher, n_replayed: *mut i64, n_retried: *mut i64) -> c_int;
    fn kx_dispatcher_model_batches(d: *mut KxDispatcher, per_model: *mut i64, n_models: c_int) -> c_int;
    fn kx_dispatcher_health(d: *mut KxDispatcher, healthy: *mut i32, n_models: c_int, n_model_failures: *mut i64,
                            n_requeued: *mut i64) -> c_int;
    fn kx_dispatcher_destroy(d: *mut KxDispatcher);
    fn kx_version() -> *const c_char;
}

fn cstr_buf(buf: &[c_char]) -> String {
    unsafe { CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned()
}

/// Replaces `init_ort(dylib_path)` (kokorox/src/onn/mod.rs:19-49): checks that `device_id` is a gfx950 part.
pub fn init(device_id: i32) -> Result<(), String> {
    let mut err = vec![0 as c_char; 512];
    match unsafe { kx_init(device_id, err.as_mut_ptr(), err.len()) } {
        KX_OK => Ok(()),
        _ => Err(cstr_buf(&err)),
    }
}

/// Host only: `model.onnx` -> the KXHIPW01 container `HipKoko::new` would build from it in memory (convert once, load
/// faster afterwards).  No reference counterpart: ONNX Runtime parses the file on every start (ort_base.rs:27-33).
pub fn import_onnx(onnx_path: &str, out_path: &str) -> Result<(), String> {
    let a = CString::new(onnx_path).map_err(|e| e.to_string())?;
    let b = CString::new(out_path).map_err(|e| e.to_string())?;
    let mut err = vec![0 as c_char; 1024];
    match unsafe { kx_import_onnx(a.as_ptr(), b.as_ptr(), err.as_mut_ptr(), err.len()) } {
        KX_OK => Ok(()),
        _ => Err(cstr_buf(&err)),
    }
}

/// Host only: `(L, M, taps)` of the resampler behind a format word's rate code, from the library's one table (`L / M` = output
/// rate / 24 000, the float32 taps of the FIR; rate code 0 gives `(1, 1, [])`).  What a host-side check of a resampled body
/// needs: output n is the f32 rounding of the float64 sum, over ascending j, of `taps[n * M - j * L + C] * x[j]`.
pub fn resample_filter(format_word: i32) -> Result<(i32, i32, Vec<f32>), String> {
    let (mut l, mut m, mut n) = (0i32, 0i32, 0i32);
    let mut taps = vec![0f32; KX_RESAMPLE_MAX_TAPS];
    match unsafe { kx_resample_filter(format_word, &mut l, &mut m, &mut n, taps.as_mut_ptr(), taps.len() as c_int) } {
        KX_OK => {
            taps.truncate(n as usize);
            Ok((l, m, taps))
        }
        _ => Err("unknown output format or sample rate".to_string()),
    }
}

pub fn version() -> String {
    unsafe { CStr::from_ptr(kx_version()) }.to_string_lossy().into_owned()
}

/// Drop-in for `kokorox::onn::ort_koko::OrtKoko` (same two public methods, same signatures).
pub struct HipKoko {
    h: *mut KxModel,
}
// Calls on one model are serialised inside the library, exactly as `Mutex<Session>` does (ort_koko.rs:14,17-18,78).
unsafe impl Send for HipKoko {}
unsafe impl Sync for HipKoko {}

impl HipKoko {
    /// `OrtKoko::new` (ort_koko.rs:31-35): load failure is an `Err(String)`; the caller `.expect`s (koko.rs:572).
    /// `model_path` is the `.onnx` the reference passes (koko.rs:570-573) or a pre-converted KXHIPW01 container.
    pub fn new(model_path: String) -> Result<Self, String> {
        Self::on_device(model_path, 0)
    }

    pub fn on_device(model_path: String, device_id: i32) -> Result<Self, String> {
        let p = CString::new(model_path).map_err(|e| e.to_string())?;
        let mut err = vec![0 as c_char; 512];
        let h = unsafe { kx_create(p.as_ptr(), device_id, err.as_mut_ptr(), err.len()) };
        if h.is_null() {
            return Err(cstr_buf(&err));
        }
        Ok(HipKoko { h })
    }

    /// One model per device id from ONE read of the weight file (device-to-device fan-out over xGMI inside the
    /// library).  The result is what `HipKokoDispatcher::new` takes; the reference's server is one process
    /// (kokorox-openai/src/lib.rs:370-439).
    pub fn replicas(model_path: String, device_ids: &[i32]) -> Result<Vec<Self>, String> {
        let p = CString::new(model_path).map_err(|e| e.to_string())?;
        let mut err = vec![0 as c_char; 512];
        let mut hs: Vec<*mut KxModel> = vec![ptr::null_mut(); device_ids.len()];
        let rc = unsafe {
            kx_create_replicas(p.as_ptr(), device_ids.as_ptr(), device_ids.len() as c_int, hs.as_mut_ptr(),
                               err.as_mut_ptr(), err.len())
        };
        if rc != KX_OK {
            return Err(cstr_buf(&err));
        }
        Ok(hs.into_iter().map(|h| HipKoko { h }).collect())
    }

    /// A model confined to CUs `[part, part + 1) x CUs / n_parts` of the device: partitions run their forwards side by side on one
    /// GPU without competing for a CU (`kx_create_replicas` does this for a device id that is named several times).
    pub fn partition(model_path: String, device_id: i32, part: i32, n_parts: i32) -> Result<Self, String> {
        let p = CString::new(model_path).map_err(|e| e.to_string())?;
        let mut err = vec![0 as c_char; 512];
        let h = unsafe { kx_create_partition(p.as_ptr(), device_id, part, n_parts, err.as_mut_ptr(), err.len()) };
        if h.is_null() {
            return Err(cstr_buf(&err));
        }
        Ok(HipKoko { h })
    }

    /// Milestones of the process's last `replicas` call in ms from its entry: file read (+ conversion), blob resident on every
    /// device, every model built.
    pub fn replicas_times() -> [f64; 3] {
        let mut t = [0f64; 3];
        unsafe { kx_replicas_times(t.as_mut_ptr()) };
        t
    }

    /// `[weight-file variant, reference arithmetic (0 for the de-quantised int8 / q4 variants), conv mode, vocabulary rows,
    /// voices, CU partition, partitions, CUs]` (kx_model_info).
    pub fn info(&self) -> Result<[i64; 8], Box<dyn Error>> {
        let mut o = [0i64; 8];
        self.check(unsafe { kx_model_info(self.h, o.as_mut_ptr()) })?;
        Ok(o)
    }

    /// `[recurrence form (0 resident weights / 1 streaming fall-back), hand-off time-outs, clean forwards until the resident forms
    /// return, transparently re-run calls]`: all zero in a healthy deployment (kx_model_status).
    pub fn status(&self) -> Result<[i64; 4], Box<dyn Error>> {
        let mut o = [0i64; 4];
        self.check(unsafe { kx_model_status(self.h, o.as_mut_ptr()) })?;
        Ok(o)
    }

    /// Host-side milestones of the last call in ms from its entry (kx_call_times).
    pub fn call_times(&self) -> Result<[f64; 4], Box<dyn Error>> {
        let mut o = [0f64; 4];
        self.check(unsafe { kx_call_times(self.h, o.as_mut_ptr()) })?;
        Ok(o)
    }

    /// A model from a weight blob that already sits in this GPU's memory (after an RCCL broadcast).
    ///
    /// # Safety
    /// `d_blob` must be a device pointer valid for `n_bytes` on `device_id`.
    pub unsafe fn from_device_blob(d_blob: *const c_void, n_bytes: usize, device_id: i32) -> Result<Self, String> {
        let mut err = vec![0 as c_char; 512];
        let h = kx_create_from_device_blob(d_blob, n_bytes, device_id, err.as_mut_ptr(), err.len());
        if h.is_null() {
            return Err(cstr_buf(&err));
        }
        Ok(HipKoko { h })
    }

    fn last_error(&self) -> String {
        let mut buf = vec![0 as c_char; 512];
        unsafe { kx_last_error_copy(self.h, buf.as_mut_ptr(), buf.len()) };
        let s = cstr_buf(&buf);
        if s.is_empty() {
            // (same text through the pointer form; kept so that both entry points stay bound)
            unsafe { CStr::from_ptr(kx_last_error(self.h)) }.to_string_lossy().into_owned()
        } else {
            s
        }
    }

    fn check(&self, rc: c_int) -> Result<(), Box<dyn Error>> {
        if rc == KX_OK {
            Ok(())
        } else {
            Err(format!("kokorox_hip error {}: {}", rc, self.last_error()).into())
        }
    }

    fn flatten(tokens: &[Vec<i64>]) -> (Vec<i64>, Vec<i32>, usize) {
        let stride = tokens.iter().map(|t| t.len()).max().unwrap_or(0).max(1);
        let lens: Vec<i32> = tokens.iter().map(|t| t.len() as i32).collect();
        let mut ids = vec![0i64; tokens.len() * stride];
        for (i, t) in tokens.iter().enumerate() {
            ids[i * stride..i * stride + t.len()].copy_from_slice(t);
        }
        (ids, lens, stride)
    }

    /// `OrtKoko::infer` (ort_koko.rs:37-91).  B = 1 behaves exactly like the reference call at koko.rs:1177;
    /// B > 1 returns the B waveforms back to back (the chunk loop of koko.rs:947-1191 as one call).
    /// An empty token list is an `Err`, not the index panic of ort_koko.rs:56.
    pub fn infer(&self, tokens: Vec<Vec<i64>>, styles: Vec<Vec<f32>>, speed: f32)
        -> Result<ArrayBase<OwnedRepr<f32>, IxDyn>, Box<dyn Error>> {
        let (wav, _lens) = self.infer_batch(&tokens, &styles, &[speed], 0, 0)?;
        let n = wav.len();
        Ok(ArrayBase::from_shape_vec(IxDyn(&[n]), wav)?)
    }

    /// Batched form with an explicit noise seed; returns (samples back to back, per-utterance sample counts).
    pub fn infer_batch(&self, tokens: &[Vec<i64>], styles: &[Vec<f32>], speeds: &[f32], seed: u64, flags: u32)
        -> Result<(Vec<f32>, Vec<i64>), Box<dyn Error>> {
        if tokens.is_empty() || tokens[0].is_empty() {
            return Err("infer: empty token list".into());
        }
        if styles.len() != tokens.len() || styles.iter().any(|s| s.len() != KX_STYLE_DIM) {
            return Err("infer: one style row of 256 floats per utterance is required".into());
        }
        let b = tokens.len();
        let (ids, lens, stride) = Self::flatten(tokens);
        let st: Vec<f32> = styles.iter().flatten().copied().collect();
        let mut out: *mut f32 = ptr::null_mut();
        let mut out_lens = vec![0i64; b];
        let rc = unsafe {
            kx_infer(self.h, ids.as_ptr(), stride as i64, lens.as_ptr(), b as c_int, st.as_ptr(), speeds.as_ptr(),
                     speeds.len() as c_int, seed, flags, &mut out, out_lens.as_mut_ptr())
        };
        self.check(rc)?;
        let n: usize = out_lens.iter().sum::<i64>() as usize;
        let v = unsafe { std::slice::from_raw_parts(out, n) }.to_vec(); // the same owned copy as ort_koko.rs:85
        unsafe { kx_free_audio(out) };
        Ok((v, out_lens))
    }

    /// Device-resident voice table (`TTSKoko::load_voices` layout, koko.rs:1308-1334): `[n_voices][511][256]`.
    pub fn set_voice_table(&self, table: &[f32], n_voices: usize) -> Result<(), Box<dyn Error>> {
        if table.len() != n_voices * 511 * KX_STYLE_DIM {
            return Err("voice table must hold n_voices * 511 * 256 floats".into());
        }
        self.check(unsafe { kx_set_voice_table(self.h, table.as_ptr(), n_voices as c_int) })
    }

    /// `mix_styles` on the GPU (koko.rs:1255-1306): `(voice id, weight)` pairs per utterance, packed output bytes.
    pub fn infer_voices(&self, tokens: &[Vec<i64>], voice_ids: &[i32], weights: &[f32], max_mix: usize,
                        speeds: &[f32], seed: u64, format: c_int) -> Result<(Vec<u8>, Vec<i64>), Box<dyn Error>> {
        if tokens.is_empty() || voice_ids.len() != tokens.len() * max_mix || weights.len() != voice_ids.len() {
            return Err("infer_voices: B * max_mix voice ids and weights are required".into());
        }
        let b = tokens.len();
        let (ids, lens, stride) = Self::flatten(tokens);
        let mut out: *mut c_void = ptr::null_mut();
        let (mut nbytes, mut nsamp) = (vec![0i64; b], vec![0i64; b]);
        let rc = unsafe {
            kx_infer_voices(self.h, ids.as_ptr(), stride as i64, lens.as_ptr(), b as c_int, voice_ids.as_ptr(),
                            weights.as_ptr(), max_mix as c_int, speeds.as_ptr(), speeds.len() as c_int, seed, 0,
                            format, &mut out, nbytes.as_mut_ptr(), nsamp.as_mut_ptr())
        };
        self.check(rc)?;
        let n: usize = nbytes.iter().sum::<i64>() as usize;
        let v = unsafe { std::slice::from_raw_parts(out as *const u8, n) }.to_vec();
        unsafe { kx_free_packed(out) };
        Ok((v, nbytes))
    }

    /// Explicit style rows, output packed on the GPU: f32 stereo (koko.rs:1239-1246) or PCM16
    /// (kokorox-websocket/src/lib.rs:701-704).
    pub fn infer_packed(&self, tokens: &[Vec<i64>], styles: &[Vec<f32>], speeds: &[f32], seed: u64, format: c_int)
        -> Result<(Vec<u8>, Vec<i64>), Box<dyn Error>> {
        if tokens.is_empty() || styles.len() != tokens.len() {
            return Err("infer_packed: one style row per utterance is required".into());
        }
        let b = tokens.len();
        let (ids, lens, stride) = Self::flatten(tokens);
        let st: Vec<f32> = styles.iter().flatten().copied().collect();
        let mut out: *mut c_void = ptr::null_mut();
        let (mut nbytes, mut nsamp) = (vec![0i64; b], vec![0i64; b]);
        let rc = unsafe {
            kx_infer_packed(self.h, ids.as_ptr(), stride as i64, lens.as_ptr(), b as c_int, st.as_ptr(),
                            speeds.as_ptr(), speeds.len() as c_int, seed, 0, format, &mut out, nbytes.as_mut_ptr(),
                            nsamp.as_mut_ptr())
        };
        self.check(rc)?;
        let n: usize = nbytes.iter().sum::<i64>() as usize;
        let v = unsafe { std::slice::from_raw_parts(out as *const u8, n) }.to_vec();
        unsafe { kx_free_packed(out) };
        Ok((v, nbytes))
    }

    /// The chunk loop of `TTSKoko::tts_raw_audio` (koko.rs:947-1191) as one forward: `tokens` are the chunks, request r owns
    /// `chunks_per_request[r]` consecutive ones, `styles` holds one row per chunk, `formats` one format word (a KX_PACK_* form, optionally | KX_PACK_RATE_*) for
    /// all requests or one per request.  Returns each request's body: header of its form, if any, then its chunks' samples
    /// in order with nothing between them.
    pub fn infer_requests(&self, tokens: &[Vec<i64>], chunks_per_request: &[i32], styles: &[Vec<f32>], speeds: &[f32],
                          seed: u64, formats: &[c_int]) -> Result<Vec<Vec<u8>>, Box<dyn Error>> {
        if tokens.is_empty() || styles.len() != tokens.len() || styles.iter().any(|s| s.len() != KX_STYLE_DIM) {
            return Err("infer_requests: one style row of 256 floats per chunk is required".into());
        }
        let (b, r) = (tokens.len(), chunks_per_request.len());
        let (ids, lens, stride) = Self::flatten(tokens);
        let st: Vec<f32> = styles.iter().flatten().copied().collect();
        let mut out: *mut c_void = ptr::null_mut();
        let (mut nbytes, mut nsamp) = (vec![0i64; r.max(1)], vec![0i64; r.max(1)]);
        let rc = unsafe {
            kx_infer_requests(self.h, ids.as_ptr(), stride as i64, lens.as_ptr(), b as c_int, chunks_per_request.as_ptr(),
                              r as c_int, st.as_ptr(), ptr::null(), ptr::null(), 0, speeds.as_ptr(), speeds.len() as c_int,
                              seed, 0, formats.as_ptr(), formats.len() as c_int, &mut out, nbytes.as_mut_ptr(),
                              nsamp.as_mut_ptr())
        };
        self.check(rc)?;
        let mut bodies = Vec::with_capacity(r);
        let mut at = 0usize;
        for n in nbytes.iter().take(r) {
            bodies.push(unsafe { std::slice::from_raw_parts((out as *const u8).add(at), *n as usize) }.to_vec());
            at += *n as usize;
        }
        unsafe { kx_free_packed(out) };
        Ok(bodies)
    }

    /// `infer_requests` with the token marks of every request ("token marks" in kokorox_hip.h): per request its body and, per
    /// chunk, tokens + 1 sample offsets in the request's stream at the request's output rate, the chunks back to back.
    pub fn infer_requests_marks(&self, tokens: &[Vec<i64>], chunks_per_request: &[i32], styles: &[Vec<f32>], speeds: &[f32],
                                seed: u64, formats: &[c_int]) -> Result<Vec<(Vec<u8>, Vec<i64>)>, Box<dyn Error>> {
        if tokens.is_empty() || styles.len() != tokens.len() || styles.iter().any(|s| s.len() != KX_STYLE_DIM) {
            return Err("infer_requests: one style row of 256 floats per chunk is required".into());
        }
        let (b, r) = (tokens.len(), chunks_per_request.len());
        let (ids, lens, stride) = Self::flatten(tokens);
        let st: Vec<f32> = styles.iter().flatten().copied().collect();
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let (mut nbytes, mut nsamp, mut nmarks) = (vec![0i64; r.max(1)], vec![0i64; r.max(1)], vec![0i64; r.max(1)]);
        let rc = unsafe {
            kx_infer_requests_marks(self.h, ids.as_ptr(), stride as i64, lens.as_ptr(), b as c_int, chunks_per_request.as_ptr(),
                                    r as c_int, st.as_ptr(), ptr::null(), ptr::null(), 0, speeds.as_ptr(), speeds.len() as c_int,
                                    seed, 0, formats.as_ptr(), formats.len() as c_int, &mut out, nbytes.as_mut_ptr(),
                                    nsamp.as_mut_ptr(), &mut mk, nmarks.as_mut_ptr())
        };
        self.check(rc)?;
        let mut res = Vec::with_capacity(r);
        let (mut at, mut mat) = (0usize, 0usize);
        for i in 0..r {
            // (the marks live in the buffer of `out`: copied before it is released)
            let body = unsafe { std::slice::from_raw_parts((out as *const u8).add(at), nbytes[i] as usize) }.to_vec();
            let marks = unsafe { std::slice::from_raw_parts((mk as *const i64).add(mat), nmarks[i] as usize) }.to_vec();
            at += nbytes[i] as usize;
            mat += nmarks[i] as usize;
            res.push((body, marks));
        }
        unsafe { kx_free_packed(out) };
        Ok(res)
    }

    /// `infer_requests_marks` with the seams of every request shaped on the GPU ("joins" in kokorox_hip.h): `joins` holds one
    /// spec for all requests or one per request.
    pub fn infer_requests_joined(&self, tokens: &[Vec<i64>], chunks_per_request: &[i32], styles: &[Vec<f32>], speeds: &[f32],
                                 seed: u64, formats: &[c_int], joins: &[KxJoin]) -> Result<Vec<(Vec<u8>, Vec<i64>)>, Box<dyn Error>> {
        if tokens.is_empty() || styles.len() != tokens.len() || styles.iter().any(|s| s.len() != KX_STYLE_DIM) {
            return Err("infer_requests: one style row of 256 floats per chunk is required".into());
        }
        let (b, r) = (tokens.len(), chunks_per_request.len());
        let (ids, lens, stride) = Self::flatten(tokens);
        let st: Vec<f32> = styles.iter().flatten().copied().collect();
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let (mut nbytes, mut nsamp, mut nmarks) = (vec![0i64; r.max(1)], vec![0i64; r.max(1)], vec![0i64; r.max(1)]);
        let rc = unsafe {
            kx_infer_requests_joined(self.h, ids.as_ptr(), stride as i64, lens.as_ptr(), b as c_int, chunks_per_request.as_ptr(),
                                     r as c_int, st.as_ptr(), ptr::null(), ptr::null(), 0, speeds.as_ptr(), speeds.len() as c_int,
                                     seed, 0, formats.as_ptr(), formats.len() as c_int, &mut out, nbytes.as_mut_ptr(),
                                     nsamp.as_mut_ptr(), &mut mk, nmarks.as_mut_ptr(), joins.as_ptr(), joins.len() as c_int)
        };
        self.check(rc)?;
        let mut res = Vec::with_capacity(r);
        let (mut at, mut mat) = (0usize, 0usize);
        for i in 0..r {
            // (the marks live in the buffer of `out`: copied before it is released)
            let body = unsafe { std::slice::from_raw_parts((out as *const u8).add(at), nbytes[i] as usize) }.to_vec();
            let marks = unsafe { std::slice::from_raw_parts((mk as *const i64).add(mat), nmarks[i] as usize) }.to_vec();
            at += nbytes[i] as usize;
            mat += nmarks[i] as usize;
            res.push((body, marks));
        }
        unsafe { kx_free_packed(out) };
        Ok(res)
    }

    /// `infer_requests_joined` with the level of every request set on the GPU ("levels" in kokorox_hip.h): `levels` holds one
    /// spec for all requests or one per request, `joins` may be empty (no joins).  Per request: body, marks, and (p, g), the
    /// peak of its stream and the gain applied, as the GPU computed them.
    #[allow(clippy::type_complexity)]
    pub fn infer_requests_levelled(&self, tokens: &[Vec<i64>], chunks_per_request: &[i32], styles: &[Vec<f32>], speeds: &[f32],
                                   seed: u64, formats: &[c_int], joins: &[KxJoin], levels: &[KxLevel])
                                   -> Result<Vec<(Vec<u8>, Vec<i64>, (f64, f64))>, Box<dyn Error>> {
        if tokens.is_empty() || styles.len() != tokens.len() || styles.iter().any(|s| s.len() != KX_STYLE_DIM) {
            return Err("infer_requests: one style row of 256 floats per chunk is required".into());
        }
        let (b, r) = (tokens.len(), chunks_per_request.len());
        let (ids, lens, stride) = Self::flatten(tokens);
        let st: Vec<f32> = styles.iter().flatten().copied().collect();
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let (mut nbytes, mut nsamp, mut nmarks) = (vec![0i64; r.max(1)], vec![0i64; r.max(1)], vec![0i64; r.max(1)]);
        let mut lv = vec![0f64; 2 * r.max(1)];
        let rc = unsafe {
            kx_infer_requests_levelled(self.h, ids.as_ptr(), stride as i64, lens.as_ptr(), b as c_int, chunks_per_request.as_ptr(),
                                       r as c_int, st.as_ptr(), ptr::null(), ptr::null(), 0, speeds.as_ptr(), speeds.len() as c_int,
                                       seed, 0, formats.as_ptr(), formats.len() as c_int, &mut out, nbytes.as_mut_ptr(),
                                       nsamp.as_mut_ptr(), &mut mk, nmarks.as_mut_ptr(),
                                       if joins.is_empty() { ptr::null() } else { joins.as_ptr() }, joins.len() as c_int,
                                       levels.as_ptr(), levels.len() as c_int, lv.as_mut_ptr())
        };
        self.check(rc)?;
        let mut res = Vec::with_capacity(r);
        let (mut at, mut mat) = (0usize, 0usize);
        for i in 0..r {
            // (the marks live in the buffer of `out`: copied before it is released)
            let body = unsafe { std::slice::from_raw_parts((out as *const u8).add(at), nbytes[i] as usize) }.to_vec();
            let marks = unsafe { std::slice::from_raw_parts((mk as *const i64).add(mat), nmarks[i] as usize) }.to_vec();
            at += nbytes[i] as usize;
            mat += nmarks[i] as usize;
            res.push((body, marks, (lv[2 * i], lv[2 * i + 1])));
        }
        unsafe { kx_free_packed(out) };
        Ok(res)
    }

    /// `infer_requests_joined` with the integrated loudness of every request measured, and set, on the GPU ("loudness" in
    /// kokorox_hip.h): `loudness` holds one spec for all requests or one per request, `joins` may be empty (no joins).  Per
    /// request: body, marks, and [p, g, I, n_g]: the peak of its stream, the gain applied, its loudness in LUFS (NaN when
    /// undefined) and the number of gated blocks, as the GPU computed them.
    #[allow(clippy::type_complexity)]
    pub fn infer_requests_loudness(&self, tokens: &[Vec<i64>], chunks_per_request: &[i32], styles: &[Vec<f32>], speeds: &[f32],
                                   seed: u64, formats: &[c_int], joins: &[KxJoin], loudness: &[KxLoudness])
                                   -> Result<Vec<(Vec<u8>, Vec<i64>, [f64; 4])>, Box<dyn Error>> {
        if tokens.is_empty() || styles.len() != tokens.len() || styles.iter().any(|s| s.len() != KX_STYLE_DIM) {
            return Err("infer_requests: one style row of 256 floats per chunk is required".into());
        }
        let (b, r) = (tokens.len(), chunks_per_request.len());
        let (ids, lens, stride) = Self::flatten(tokens);
        let st: Vec<f32> = styles.iter().flatten().copied().collect();
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let (mut nbytes, mut nsamp, mut nmarks) = (vec![0i64; r.max(1)], vec![0i64; r.max(1)], vec![0i64; r.max(1)]);
        let mut ld = vec![0f64; 4 * r.max(1)];
        let rc = unsafe {
            kx_infer_requests_loudness(self.h, ids.as_ptr(), stride as i64, lens.as_ptr(), b as c_int, chunks_per_request.as_ptr(),
                                       r as c_int, st.as_ptr(), ptr::null(), ptr::null(), 0, speeds.as_ptr(), speeds.len() as c_int,
                                       seed, 0, formats.as_ptr(), formats.len() as c_int, &mut out, nbytes.as_mut_ptr(),
                                       nsamp.as_mut_ptr(), &mut mk, nmarks.as_mut_ptr(),
                                       if joins.is_empty() { ptr::null() } else { joins.as_ptr() }, joins.len() as c_int,
                                       loudness.as_ptr(), loudness.len() as c_int, ld.as_mut_ptr())
        };
        self.check(rc)?;
        let mut res = Vec::with_capacity(r);
        let (mut at, mut mat) = (0usize, 0usize);
        for i in 0..r {
            // (the marks live in the buffer of `out`: copied before it is released)
            let body = unsafe { std::slice::from_raw_parts((out as *const u8).add(at), nbytes[i] as usize) }.to_vec();
            let marks = unsafe { std::slice::from_raw_parts((mk as *const i64).add(mat), nmarks[i] as usize) }.to_vec();
            at += nbytes[i] as usize;
            mat += nmarks[i] as usize;
            res.push((body, marks, [ld[4 * i], ld[4 * i + 1], ld[4 * i + 2], ld[4 * i + 3]]));
        }
        unsafe { kx_free_packed(out) };
        Ok(res)
    }

    /// `infer_requests_joined` with every request driven and peak-limited on the GPU ("limiter" in kokorox_hip.h): `limits`
    /// holds one spec for all requests or one per request, `joins` may be empty (no joins).  Per request: body, marks, and
    /// [p, g, I, n_g, r]: the peak of its stream, the static gain, its loudness in LUFS and gated blocks (NaN and 0 in mode 0),
    /// and the smallest smoothed gain (1.0 when nothing was limited), as the GPU computed them.
    #[allow(clippy::type_complexity)]
    pub fn infer_requests_limited(&self, tokens: &[Vec<i64>], chunks_per_request: &[i32], styles: &[Vec<f32>], speeds: &[f32],
                                  seed: u64, formats: &[c_int], joins: &[KxJoin], limits: &[KxLimit])
                                  -> Result<Vec<(Vec<u8>, Vec<i64>, [f64; 5])>, Box<dyn Error>> {
        if tokens.is_empty() || styles.len() != tokens.len() || styles.iter().any(|s| s.len() != KX_STYLE_DIM) {
            return Err("infer_requests: one style row of 256 floats per chunk is required".into());
        }
        let (b, r) = (tokens.len(), chunks_per_request.len());
        let (ids, lens, stride) = Self::flatten(tokens);
        let st: Vec<f32> = styles.iter().flatten().copied().collect();
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let (mut nbytes, mut nsamp, mut nmarks) = (vec![0i64; r.max(1)], vec![0i64; r.max(1)], vec![0i64; r.max(1)]);
        let mut lm = vec![0f64; 5 * r.max(1)];
        let rc = unsafe {
            kx_infer_requests_limited(self.h, ids.as_ptr(), stride as i64, lens.as_ptr(), b as c_int, chunks_per_request.as_ptr(),
                                      r as c_int, st.as_ptr(), ptr::null(), ptr::null(), 0, speeds.as_ptr(), speeds.len() as c_int,
                                      seed, 0, formats.as_ptr(), formats.len() as c_int, &mut out, nbytes.as_mut_ptr(),
                                      nsamp.as_mut_ptr(), &mut mk, nmarks.as_mut_ptr(),
                                      if joins.is_empty() { ptr::null() } else { joins.as_ptr() }, joins.len() as c_int,
                                      limits.as_ptr(), limits.len() as c_int, lm.as_mut_ptr())
        };
        self.check(rc)?;
        let mut res = Vec::with_capacity(r);
        let (mut at, mut mat) = (0usize, 0usize);
        for i in 0..r {
            // (the marks live in the buffer of `out`: copied before it is released)
            let body = unsafe { std::slice::from_raw_parts((out as *const u8).add(at), nbytes[i] as usize) }.to_vec();
            let marks = unsafe { std::slice::from_raw_parts((mk as *const i64).add(mat), nmarks[i] as usize) }.to_vec();
            at += nbytes[i] as usize;
            mat += nmarks[i] as usize;
            res.push((body, marks, [lm[5 * i], lm[5 * i + 1], lm[5 * i + 2], lm[5 * i + 3], lm[5 * i + 4]]));
        }
        unsafe { kx_free_packed(out) };
        Ok(res)
    }

    /// `infer_requests_joined` with per-token prosody and its report ("prosody" in kokorox_hip.h): `prosody` holds, per field, no
    /// rows (neutral) or one vector per chunk; `joins` may be empty (no joins).  Per request: body, marks, and the report, one
    /// `ProsodyToken` per token of its chunks.
    #[allow(clippy::type_complexity)]
    pub fn infer_requests_prosody(&self, tokens: &[Vec<i64>], chunks_per_request: &[i32], styles: &[Vec<f32>], speeds: &[f32],
                                  seed: u64, formats: &[c_int], joins: &[KxJoin], prosody: &Prosody)
                                  -> Result<Vec<(Vec<u8>, Vec<i64>, Vec<ProsodyToken>)>, Box<dyn Error>> {
        if tokens.is_empty() || styles.len() != tokens.len() || styles.iter().any(|s| s.len() != KX_STYLE_DIM) {
            return Err("infer_requests: one style row of 256 floats per chunk is required".into());
        }
        let (b, r) = (tokens.len(), chunks_per_request.len());
        let (ids, lens, stride) = Self::flatten(tokens);
        let st: Vec<f32> = styles.iter().flatten().copied().collect();
        let rate = prosody_rows(&prosody.rate, &lens, stride as usize, 1f32)?;
        let frames = prosody_rows(&prosody.frames, &lens, stride as usize, 0i32)?;
        let pitch = prosody_rows(&prosody.pitch, &lens, stride as usize, 1f32)?;
        let energy = prosody_rows(&prosody.energy, &lens, stride as usize, 1f32)?;
        let ps = KxProsody {
            rate: if rate.is_empty() { ptr::null() } else { rate.as_ptr() },
            frames: if frames.is_empty() { ptr::null() } else { frames.as_ptr() },
            pitch: if pitch.is_empty() { ptr::null() } else { pitch.as_ptr() },
            energy: if energy.is_empty() { ptr::null() } else { energy.as_ptr() },
        };
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let mut rp: *mut f32 = ptr::null_mut();
        let (mut nbytes, mut nsamp, mut nmarks) = (vec![0i64; r.max(1)], vec![0i64; r.max(1)], vec![0i64; r.max(1)]);
        let mut nrep = vec![0i64; r.max(1)];
        let rc = unsafe {
            kx_infer_requests_prosody(self.h, ids.as_ptr(), stride as i64, lens.as_ptr(), b as c_int, chunks_per_request.as_ptr(),
                                      r as c_int, st.as_ptr(), ptr::null(), ptr::null(), 0, speeds.as_ptr(), speeds.len() as c_int,
                                      seed, 0, formats.as_ptr(), formats.len() as c_int, &mut out, nbytes.as_mut_ptr(),
                                      nsamp.as_mut_ptr(), &mut mk, nmarks.as_mut_ptr(),
                                      if joins.is_empty() { ptr::null() } else { joins.as_ptr() }, joins.len() as c_int, &ps,
                                      &mut rp, nrep.as_mut_ptr())
        };
        self.check(rc)?;
        let mut res = Vec::with_capacity(r);
        let (mut at, mut mat, mut rat) = (0usize, 0usize, 0usize);
        for i in 0..r {
            // (marks and report live in the buffer of `out`: copied before it is released)
            let body = unsafe { std::slice::from_raw_parts((out as *const u8).add(at), nbytes[i] as usize) }.to_vec();
            let marks = unsafe { std::slice::from_raw_parts((mk as *const i64).add(mat), nmarks[i] as usize) }.to_vec();
            let flat = unsafe { std::slice::from_raw_parts((rp as *const f32).add(4 * rat), 4 * nrep[i] as usize) };
            let report: Vec<ProsodyToken> = flat.chunks_exact(4).map(|c| [c[0], c[1], c[2], c[3]]).collect();
            at += nbytes[i] as usize;
            mat += nmarks[i] as usize;
            rat += nrep[i] as usize;
            res.push((body, marks, report));
        }
        unsafe { kx_free_packed(out) };
        Ok(res)
    }

    /// `infer_requests_prosody` with fit spans ("fit" in kokorox_hip.h): `spans` sorted by (request, begin) and disjoint.  Per
    /// request: body and marks; then one `KxFitResult` per span.
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn infer_requests_fitted(&self, tokens: &[Vec<i64>], chunks_per_request: &[i32], styles: &[Vec<f32>], speeds: &[f32],
                                 seed: u64, formats: &[c_int], joins: &[KxJoin], prosody: &Prosody, spans: &[KxFitSpan])
                                 -> Result<(Vec<(Vec<u8>, Vec<i64>)>, Vec<KxFitResult>), Box<dyn Error>> {
        if tokens.is_empty() || styles.len() != tokens.len() || styles.iter().any(|s| s.len() != KX_STYLE_DIM) {
            return Err("infer_requests: one style row of 256 floats per chunk is required".into());
        }
        let (b, r) = (tokens.len(), chunks_per_request.len());
        let (ids, lens, stride) = Self::flatten(tokens);
        let st: Vec<f32> = styles.iter().flatten().copied().collect();
        let rate = prosody_rows(&prosody.rate, &lens, stride as usize, 1f32)?;
        let frames = prosody_rows(&prosody.frames, &lens, stride as usize, 0i32)?;
        let pitch = prosody_rows(&prosody.pitch, &lens, stride as usize, 1f32)?;
        let energy = prosody_rows(&prosody.energy, &lens, stride as usize, 1f32)?;
        let ps = KxProsody {
            rate: if rate.is_empty() { ptr::null() } else { rate.as_ptr() },
            frames: if frames.is_empty() { ptr::null() } else { frames.as_ptr() },
            pitch: if pitch.is_empty() { ptr::null() } else { pitch.as_ptr() },
            energy: if energy.is_empty() { ptr::null() } else { energy.as_ptr() },
        };
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let (mut nbytes, mut nsamp, mut nmarks) = (vec![0i64; r.max(1)], vec![0i64; r.max(1)], vec![0i64; r.max(1)]);
        let mut fit = vec![KxFitResult::default(); spans.len().max(1)];
        let rc = unsafe {
            kx_infer_requests_fitted(self.h, ids.as_ptr(), stride as i64, lens.as_ptr(), b as c_int, chunks_per_request.as_ptr(),
                                     r as c_int, st.as_ptr(), ptr::null(), ptr::null(), 0, speeds.as_ptr(), speeds.len() as c_int,
                                     seed, 0, formats.as_ptr(), formats.len() as c_int, &mut out, nbytes.as_mut_ptr(),
                                     nsamp.as_mut_ptr(), &mut mk, nmarks.as_mut_ptr(),
                                     if joins.is_empty() { ptr::null() } else { joins.as_ptr() }, joins.len() as c_int, &ps,
                                     ptr::null_mut(), ptr::null_mut(), if spans.is_empty() { ptr::null() } else { spans.as_ptr() },
                                     spans.len() as c_int, fit.as_mut_ptr())
        };
        self.check(rc)?;
        fit.truncate(spans.len());
        let mut res = Vec::with_capacity(r);
        let (mut at, mut mat) = (0usize, 0usize);
        for i in 0..r {
            // (the marks live in the buffer of `out`: copied before it is released)
            let body = unsafe { std::slice::from_raw_parts((out as *const u8).add(at), nbytes[i] as usize) }.to_vec();
            let marks = unsafe { std::slice::from_raw_parts((mk as *const i64).add(mat), nmarks[i] as usize) }.to_vec();
            at += nbytes[i] as usize;
            mat += nmarks[i] as usize;
            res.push((body, marks));
        }
        unsafe { kx_free_packed(out) };
        Ok((res, fit))
    }

    /// Raw device-pointer form (inputs and output stay in HBM).
    ///
    /// # Safety
    /// Every pointer must be device memory of this model's GPU with the extents documented in kokorox_hip.h.
    pub unsafe fn infer_device(&self, d_ids: *const i64, t_stride: i64, lens_host: &[i32], d_styles: *const f32,
                               speeds_host: &[f32], seed: u64, flags: u32, d_audio: *mut f32, audio_ld: i64,
                               d_frames: *mut i32) -> Result<i64, Box<dyn Error>> {
        let mut need: i64 = 0;
        let rc = kx_infer_device(self.h, d_ids, t_stride, lens_host.as_ptr(), lens_host.len() as c_int, d_styles,
                                 speeds_host.as_ptr(), speeds_host.len() as c_int, seed, flags, d_audio, audio_ld,
                                 d_frames, &mut need);
        self.check(rc)?;
        Ok(need)
    }

    pub fn sync(&self) -> Result<(), Box<dyn Error>> {
        self.check(unsafe { kx_sync(self.h) })
    }
    pub fn set_pinned_durations(&self, pattern: &[i32]) -> Result<(), Box<dyn Error>> {
        self.check(unsafe { kx_set_pinned_durations(self.h, pattern.as_ptr(), pattern.len() as c_int) })
    }
    /// For servers: one discarded forward at the largest (batch x length) shape the deployment expects, so that the arenas and
    /// the page-locked result buffer exist before the first request (an arena that grows under load is a second-long outlier).
    pub fn warmup(&self, batch: i32, n_tokens: i32, frames_per_token: i32) -> Result<(), Box<dyn Error>> {
        self.check(unsafe { kx_warmup(self.h, batch, n_tokens, frames_per_token) })
    }
    /// Capacities in bytes of the token-axis, frame-axis and I/O arenas.
    pub fn arena_bytes(&self) -> Result<[i64; 3], Box<dyn Error>> {
        let mut v = [0i64; 3];
        self.check(unsafe { kx_arena_bytes(self.h, v.as_mut_ptr()) })?;
        Ok(v)
    }
    /// Contraction arithmetic: 6 = f16f8 (the default: split f16 products, the cross terms of the 7- / 11-tap convs on 8-bit MFMAs),
    /// 1 = f16x3 (three f16 MFMAs per product), 0 = f32 MFMA, 4 / 5 = one f16 / bf16 MFMA per product (opt-in reduced precision).
    pub fn set_conv_mode(&self, mode: i32) -> Result<(), Box<dyn Error>> {
        self.check(unsafe { kx_set_conv_mode(self.h, mode) })
    }
    pub fn conv_mode(&self) -> i32 {
        unsafe { kx_get_conv_mode(self.h) }
    }
    /// 0 = the ONNX export's conv-based STFT pair (upstream `CustomSTFT`), 1 = `torch.stft/istft` semantics.
    pub fn set_stft_variant(&self, variant: i32) -> Result<(), Box<dyn Error>> {
        self.check(unsafe { kx_set_stft_variant(self.h, variant) })
    }
    pub fn stft_variant(&self) -> i32 {
        unsafe { kx_get_stft_variant(self.h) }
    }
    /// 1 = one stream; 4 = the independent chains of the back half on streams of their own; 0 (default) = by batch size.
    pub fn set_lanes(&self, n: i32) -> Result<(), Box<dyn Error>> {
        self.check(unsafe { kx_set_lanes(self.h, n) })
    }
    pub fn set_utterance_base(&self, base: u64) -> Result<(), Box<dyn Error>> {
        self.check(unsafe { kx_set_utterance_base(self.h, base) })
    }
    /// Real-weights diagnostics: measure every conv input during the following calls.
    pub fn diag_enable(&self, on: bool) -> Result<(), Box<dyn Error>> {
        self.check(unsafe { kx_diag_enable(self.h, on as c_int) })
    }
    /// (layer, [rows, Cin, taps, pre-scale exponent, absmax, rms, elements]) per conv launch since `diag_enable(true)`.
    pub fn diag_records(&self) -> Result<Vec<(String, [f64; 7])>, Box<dyn Error>> {
        let mut n = 0i64;
        self.check(unsafe { kx_diag_count(self.h, &mut n) })?;
        let mut out = Vec::with_capacity(n as usize);
        for i in 0..n {
            let mut name = vec![0 as c_char; 128];
            let mut v = [0f64; 7];
            self.check(unsafe { kx_diag_get(self.h, i, name.as_mut_ptr(), name.len(), v.as_mut_ptr()) })?;
            out.push((cstr_buf(&name), v));
        }
        Ok(out)
    }
    /// f16x3: multiply a layer's transformed input by 2^log2_scale before the hi/lo split (undone exactly).
    pub fn set_act_prescale(&self, layer: &str, log2_scale: i32) -> Result<(), Box<dyn Error>> {
        let c = CString::new(layer)?;
        self.check(unsafe { kx_set_act_prescale(self.h, c.as_ptr(), log2_scale) })
    }
    pub fn profile_enable(&self, on: bool) -> Result<(), Box<dyn Error>> {
        self.check(unsafe { kx_profile_enable(self.h, on as c_int) })
    }
    /// (launches, milliseconds, algorithmic FLOPs) of the dominant kernel family since the last read.
    pub fn profile_read(&self) -> Result<(i64, f64, f64), Box<dyn Error>> {
        let (mut n, mut ms, mut fl) = (0i64, 0f64, 0f64);
        self.check(unsafe { kx_profile_read(self.h, &mut n, &mut ms, &mut fl) })?;
        Ok((n, ms, fl))
    }
    /// (launches, bytes) of the unfused InstanceNorm statistics passes since the last call.
    pub fn profile_aux(&self) -> Result<(i64, f64), Box<dyn Error>> {
        let (mut n, mut by) = (0i64, 0f64);
        self.check(unsafe { kx_profile_aux(self.h, &mut n, &mut by) })?;
        Ok((n, by))
    }
    /// Per-launch rows of the last `profile_read`: [rows, Cin, taps, dil, stride, store, cols, flops, ms, bytes].
    pub fn profile_detail(&self) -> Result<Vec<[f64; 10]>, Box<dyn Error>> {
        let mut n = 0i64;
        self.check(unsafe { kx_profile_detail(self.h, ptr::null_mut(), 0, &mut n) })?;
        let mut rows = vec![[0f64; 10]; n as usize];
        self.check(unsafe { kx_profile_detail(self.h, rows.as_mut_ptr() as *mut f64, n, &mut n) })?;
        Ok(rows)
    }
}

impl Drop for HipKoko {
    fn drop(&mut self) {
        unsafe { kx_destroy(self.h) } // replaces TTSKoko::cleanup's sleep-and-drop (koko.rs:1338-1375)
    }
}

/// How a dispatched request names its voice.
pub enum Voice<'a> {
    Row(&'a [f32]),
    Single(i32),
    Mix(&'a [(i32, f32)]),
}

/// Batching front over one model per GPU: the replacement for the reference's one-request-at-a-time
/// `Mutex<Session>` (ort_koko.rs:78; kokorox-openai/src/lib.rs:370-439, kokorox-websocket/src/lib.rs:657-668).
/// `submit` blocks and may be called from any number of threads (tokio `spawn_blocking` in the servers).
pub struct HipKokoDispatcher {
    d: *mut KxDispatcher,
    _models: Vec<HipKoko>, // kept alive for the dispatcher's lifetime
}
unsafe impl Send for HipKokoDispatcher {}
unsafe impl Sync for HipKokoDispatcher {}

impl HipKokoDispatcher {
    pub fn new(models: Vec<HipKoko>, max_batch: i32, max_wait_us: i32) -> Result<Self, String> {
        let mut hs: Vec<*mut KxModel> = models.iter().map(|m| m.h).collect();
        let mut err = vec![0 as c_char; 256];
        let d = unsafe {
            kx_dispatcher_create(hs.as_mut_ptr(), hs.len() as c_int, max_batch, max_wait_us, err.as_mut_ptr(), err.len())
        };
        if d.is_null() {
            return Err(cstr_buf(&err));
        }
        Ok(HipKokoDispatcher { d, _models: models })
    }

    /// `new`, after one discarded forward of `max_batch` utterances x `warm_tokens` tokens at `warm_frames_per_token` frames per
    /// token on every model: what a server should call, so that no request ever pays for an arena growing.
    pub fn new_warm(models: Vec<HipKoko>, max_batch: i32, max_wait_us: i32, warm_tokens: i32, warm_frames_per_token: i32) -> Result<Self, String> {
        let mut hs: Vec<*mut KxModel> = models.iter().map(|m| m.h).collect();
        let mut err = vec![0 as c_char; 256];
        let d = unsafe {
            kx_dispatcher_create_warm(hs.as_mut_ptr(), hs.len() as c_int, max_batch, max_wait_us, warm_tokens, warm_frames_per_token,
                                      err.as_mut_ptr(), err.len())
        };
        if d.is_null() {
            return Err(cstr_buf(&err));
        }
        Ok(HipKokoDispatcher { d, _models: models })
    }

    /// Per-model health (true = takes work; false = failed a batch with a device error twice in a row and is out), the number of
    /// models marked failed and of requests that went back to the queue for another model.
    pub fn health(&self) -> (Vec<bool>, i64, i64) {
        let n = self._models.len();
        let mut h = vec![0i32; n];
        let (mut f, mut r) = (0i64, 0i64);
        unsafe { kx_dispatcher_health(self.d, h.as_mut_ptr(), n as c_int, &mut f, &mut r) };
        (h.into_iter().map(|v| v != 0).collect(), f, r)
    }

    /// One utterance: `ids` already wrapped with the two 0 pads (koko.rs:1169-1173), `style` = 256 floats.
    /// Bit-identical to `HipKoko::infer` of the same request alone, whatever it was batched with.
    pub fn submit(&self, ids: &[i64], style: &[f32], speed: f32, seed: u64) -> Result<Vec<f32>, Box<dyn Error>> {
        if style.len() != KX_STYLE_DIM {
            return Err("submit: the style row must have 256 floats".into());
        }
        let mut out: *mut f32 = ptr::null_mut();
        let mut n: i64 = 0;
        let mut err = vec![0 as c_char; 256];
        let rc = unsafe {
            kx_dispatcher_submit(self.d, ids.as_ptr(), ids.len() as c_int, style.as_ptr(), speed, seed, &mut out,
                                 &mut n, err.as_mut_ptr(), err.len())
        };
        if rc != KX_OK {
            return Err(format!("kokorox_hip error {}: {}", rc, cstr_buf(&err)).into());
        }
        let v = unsafe { std::slice::from_raw_parts(out, n as usize) }.to_vec();
        unsafe { kx_free_audio(out) };
        Ok(v)
    }

    /// The request as the servers make it (kokorox-openai/src/lib.rs:370-439): the voice by name into the device voice
    /// table -- `Voice::Single(id)` = row copy, `Voice::Mix(&[(id, weight)])` = "a.4+b.5" (koko.rs:1255-1306) -- or as
    /// the 256-float row, and the output form (0 f32 mono, 1 f32 stereo, 2 PCM16).  Returns the packed bytes and the
    /// sample count; bit-identical to the same request run alone.
    pub fn submit_ex(&self, ids: &[i64], voice: Voice, speed: f32, seed: u64, format: i32)
                     -> Result<(Vec<u8>, i64), Box<dyn Error>> {
        let (mut vid, mut w): (Vec<i32>, Vec<f32>) = (Vec::new(), Vec::new());
        let (style_p, vid_p, w_p, n_mix) = match voice {
            Voice::Row(s) => {
                if s.len() != KX_STYLE_DIM {
                    return Err("submit_ex: the style row must have 256 floats".into());
                }
                (s.as_ptr(), ptr::null(), ptr::null(), 0)
            }
            Voice::Single(id) => {
                vid.push(id);
                (ptr::null(), vid.as_ptr(), ptr::null(), 1)
            }
            Voice::Mix(parts) => {
                for (id, p) in parts {
                    vid.push(*id);
                    w.push(*p);
                }
                (ptr::null(), vid.as_ptr(), w.as_ptr(), vid.len() as c_int)
            }
        };
        let mut out: *mut c_void = ptr::null_mut();
        let (mut nb, mut ns) = (0i64, 0i64);
        let mut err = vec![0 as c_char; 256];
        let rc = unsafe {
            kx_dispatcher_submit_ex(self.d, ids.as_ptr(), ids.len() as c_int, style_p, vid_p, w_p, n_mix, speed, seed,
                                    format, &mut out, &mut nb, &mut ns, err.as_mut_ptr(), err.len())
        };
        if rc != KX_OK {
            return Err(format!("kokorox_hip error {}: {}", rc, cstr_buf(&err)).into());
        }
        let v = unsafe { std::slice::from_raw_parts(out as *const u8, nb as usize) }.to_vec();
        unsafe { kx_free_audio(out as *mut f32) };
        Ok((v, ns))
    }

    /// A request of 1 .. max_batch chunks (`chunks`: the 0-wrapped id lists of the chunk loop, koko.rs:947-1191) as rows of one
    /// batched forward; `Voice::Row` carries one 256-float row per chunk, back to back.  Returns the request's body in the given
    /// format word (a KX_PACK_* form, optionally | KX_PACK_RATE_*) and its sample count at that rate; the bytes equal
    /// `HipKoko::infer_requests` of the request alone.
    pub fn submit_request(&self, chunks: &[Vec<i64>], voice: Voice, speed: f32, seed: u64, format: i32)
                          -> Result<(Vec<u8>, i64), Box<dyn Error>> {
        let ids: Vec<i64> = chunks.iter().flatten().copied().collect();
        let lens: Vec<i32> = chunks.iter().map(|c| c.len() as i32).collect();
        let (mut vid, mut w): (Vec<i32>, Vec<f32>) = (Vec::new(), Vec::new());
        let (style_p, vid_p, w_p, n_mix) = match voice {
            Voice::Row(s) => {
                if s.len() != KX_STYLE_DIM * chunks.len() {
                    return Err("submit_request: one style row of 256 floats per chunk is required".into());
                }
                (s.as_ptr(), ptr::null(), ptr::null(), 0)
            }
            Voice::Single(id) => {
                vid.push(id);
                (ptr::null(), vid.as_ptr(), ptr::null(), 1)
            }
            Voice::Mix(parts) => {
                for (id, p) in parts {
                    vid.push(*id);
                    w.push(*p);
                }
                (ptr::null(), vid.as_ptr(), w.as_ptr(), vid.len() as c_int)
            }
        };
        let mut out: *mut c_void = ptr::null_mut();
        let (mut nb, mut ns) = (0i64, 0i64);
        let mut err = vec![0 as c_char; 256];
        let rc = unsafe {
            kx_dispatcher_submit_request(self.d, ids.as_ptr(), lens.as_ptr(), lens.len() as c_int, style_p, vid_p, w_p, n_mix,
                                         speed, seed, format, &mut out, &mut nb, &mut ns, err.as_mut_ptr(), err.len())
        };
        if rc != KX_OK {
            return Err(format!("kokorox_hip error {}: {}", rc, cstr_buf(&err)).into());
        }
        let v = unsafe { std::slice::from_raw_parts(out as *const u8, nb as usize) }.to_vec();
        unsafe { kx_free_packed(out) };
        Ok((v, ns))
    }

    /// `submit_request` with the request's token marks ("token marks" in kokorox_hip.h): body, marks, sample count.
    pub fn submit_request_marks(&self, chunks: &[Vec<i64>], styles: &[f32], speed: f32, seed: u64, format: i32)
                                -> Result<(Vec<u8>, Vec<i64>, i64), Box<dyn Error>> {
        if styles.len() != KX_STYLE_DIM * chunks.len() {
            return Err("submit_request: one style row of 256 floats per chunk is required".into());
        }
        let ids: Vec<i64> = chunks.iter().flatten().copied().collect();
        let lens: Vec<i32> = chunks.iter().map(|c| c.len() as i32).collect();
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let (mut nb, mut ns, mut nm) = (0i64, 0i64, 0i64);
        let mut err = vec![0 as c_char; 256];
        let rc = unsafe {
            kx_dispatcher_submit_request_marks(self.d, ids.as_ptr(), lens.as_ptr(), lens.len() as c_int, styles.as_ptr(), ptr::null(),
                                               ptr::null(), 0, speed, seed, format, &mut out, &mut nb, &mut ns, &mut mk, &mut nm,
                                               err.as_mut_ptr(), err.len())
        };
        if rc != KX_OK {
            return Err(format!("kokorox_hip error {}: {}", rc, cstr_buf(&err)).into());
        }
        let v = unsafe { std::slice::from_raw_parts(out as *const u8, nb as usize) }.to_vec();
        // (inside the allocation of `out`: copied before it is released)
        let marks = unsafe { std::slice::from_raw_parts(mk as *const i64, nm as usize) }.to_vec();
        unsafe { kx_free_packed(out) };
        Ok((v, marks, ns))
    }

    /// `submit_request_marks` with the request's join spec ("joins" in kokorox_hip.h): body, marks, sample count.
    pub fn submit_request_joined(&self, chunks: &[Vec<i64>], styles: &[f32], speed: f32, seed: u64, format: i32, join: KxJoin)
                                 -> Result<(Vec<u8>, Vec<i64>, i64), Box<dyn Error>> {
        if styles.len() != KX_STYLE_DIM * chunks.len() {
            return Err("submit_request: one style row of 256 floats per chunk is required".into());
        }
        let ids: Vec<i64> = chunks.iter().flatten().copied().collect();
        let lens: Vec<i32> = chunks.iter().map(|c| c.len() as i32).collect();
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let (mut nb, mut ns, mut nm) = (0i64, 0i64, 0i64);
        let mut err = vec![0 as c_char; 256];
        let rc = unsafe {
            kx_dispatcher_submit_request_joined(self.d, ids.as_ptr(), lens.as_ptr(), lens.len() as c_int, styles.as_ptr(), ptr::null(),
                                                ptr::null(), 0, speed, seed, format, &mut out, &mut nb, &mut ns, &mut mk, &mut nm,
                                                &join, err.as_mut_ptr(), err.len())
        };
        if rc != KX_OK {
            return Err(format!("kokorox_hip error {}: {}", rc, cstr_buf(&err)).into());
        }
        let v = unsafe { std::slice::from_raw_parts(out as *const u8, nb as usize) }.to_vec();
        // (inside the allocation of `out`: copied before it is released)
        let marks = unsafe { std::slice::from_raw_parts(mk as *const i64, nm as usize) }.to_vec();
        unsafe { kx_free_packed(out) };
        Ok((v, marks, ns))
    }

    /// One piece of a request ("pieces" in kokorox_hip.h): `flags` = KX_PIECE_FIRST and / or KX_PIECE_LAST, `carry` the record the
    /// piece before left (ignored with KX_PIECE_FIRST).  Returns the payload, its sample count and the carry for the next piece.
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn submit_request_piece(&self, chunks: &[Vec<i64>], styles: &[f32], speed: f32, seed: u64, format: i32, join: Option<KxJoin>,
                                flags: u32, carry: &KxPieceCarry) -> Result<(Vec<u8>, i64, KxPieceCarry), Box<dyn Error>> {
        if styles.len() != KX_STYLE_DIM * chunks.len() {
            return Err("submit_request: one style row of 256 floats per chunk is required".into());
        }
        let ids: Vec<i64> = chunks.iter().flatten().copied().collect();
        let lens: Vec<i32> = chunks.iter().map(|c| c.len() as i32).collect();
        let mut out: *mut c_void = ptr::null_mut();
        let (mut nb, mut ns) = (0i64, 0i64);
        let mut next = KxPieceCarry::EMPTY;
        let mut err = vec![0 as c_char; 256];
        let rc = unsafe {
            kx_dispatcher_submit_request_piece(self.d, ids.as_ptr(), lens.as_ptr(), lens.len() as c_int, styles.as_ptr(), ptr::null(),
                                               ptr::null(), 0, speed, seed, format, &mut out, &mut nb, &mut ns, ptr::null_mut(),
                                               ptr::null_mut(), join.as_ref().map_or(ptr::null(), |j| j as *const KxJoin), ptr::null(),
                                               ptr::null_mut(), flags, carry as *const KxPieceCarry, &mut next, err.as_mut_ptr(),
                                               err.len())
        };
        if rc != KX_OK {
            return Err(format!("kokorox_hip error {}: {}", rc, cstr_buf(&err)).into());
        }
        let v = unsafe { std::slice::from_raw_parts(out as *const u8, nb as usize) }.to_vec();
        unsafe { kx_free_packed(out) };
        Ok((v, ns, next))
    }

    /// `submit_request_joined` with the request's level spec ("levels" in kokorox_hip.h; `join` = None: no join): body, marks,
    /// sample count, and (p, g), the peak of the request's stream and the gain applied.
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn submit_request_levelled(&self, chunks: &[Vec<i64>], styles: &[f32], speed: f32, seed: u64, format: i32,
                                   join: Option<KxJoin>, level: KxLevel) -> Result<(Vec<u8>, Vec<i64>, i64, (f64, f64)), Box<dyn Error>> {
        if styles.len() != KX_STYLE_DIM * chunks.len() {
            return Err("submit_request: one style row of 256 floats per chunk is required".into());
        }
        let ids: Vec<i64> = chunks.iter().flatten().copied().collect();
        let lens: Vec<i32> = chunks.iter().map(|c| c.len() as i32).collect();
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let (mut nb, mut ns, mut nm) = (0i64, 0i64, 0i64);
        let mut lv = [0f64; 2];
        let mut err = vec![0 as c_char; 256];
        let rc = unsafe {
            kx_dispatcher_submit_request_levelled(self.d, ids.as_ptr(), lens.as_ptr(), lens.len() as c_int, styles.as_ptr(), ptr::null(),
                                                  ptr::null(), 0, speed, seed, format, &mut out, &mut nb, &mut ns, &mut mk, &mut nm,
                                                  join.as_ref().map_or(ptr::null(), |j| j as *const KxJoin), &level, lv.as_mut_ptr(),
                                                  err.as_mut_ptr(), err.len())
        };
        if rc != KX_OK {
            return Err(format!("kokorox_hip error {}: {}", rc, cstr_buf(&err)).into());
        }
        let v = unsafe { std::slice::from_raw_parts(out as *const u8, nb as usize) }.to_vec();
        // (inside the allocation of `out`: copied before it is released)
        let marks = unsafe { std::slice::from_raw_parts(mk as *const i64, nm as usize) }.to_vec();
        unsafe { kx_free_packed(out) };
        Ok((v, marks, ns, (lv[0], lv[1])))
    }

    /// `submit_request_joined` with the request's loudness spec ("loudness" in kokorox_hip.h; `join` = None: no join): body,
    /// marks, sample count, and [p, g, I, n_g] of the request.
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn submit_request_loudness(&self, chunks: &[Vec<i64>], styles: &[f32], speed: f32, seed: u64, format: i32,
                                   join: Option<KxJoin>, loudness: KxLoudness) -> Result<(Vec<u8>, Vec<i64>, i64, [f64; 4]), Box<dyn Error>> {
        if styles.len() != KX_STYLE_DIM * chunks.len() {
            return Err("submit_request: one style row of 256 floats per chunk is required".into());
        }
        let ids: Vec<i64> = chunks.iter().flatten().copied().collect();
        let lens: Vec<i32> = chunks.iter().map(|c| c.len() as i32).collect();
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let (mut nb, mut ns, mut nm) = (0i64, 0i64, 0i64);
        let mut ld = [0f64; 4];
        let mut err = vec![0 as c_char; 256];
        let rc = unsafe {
            kx_dispatcher_submit_request_loudness(self.d, ids.as_ptr(), lens.as_ptr(), lens.len() as c_int, styles.as_ptr(), ptr::null(),
                                                  ptr::null(), 0, speed, seed, format, &mut out, &mut nb, &mut ns, &mut mk, &mut nm,
                                                  join.as_ref().map_or(ptr::null(), |j| j as *const KxJoin), &loudness, ld.as_mut_ptr(),
                                                  err.as_mut_ptr(), err.len())
        };
        if rc != KX_OK {
            return Err(format!("kokorox_hip error {}: {}", rc, cstr_buf(&err)).into());
        }
        let v = unsafe { std::slice::from_raw_parts(out as *const u8, nb as usize) }.to_vec();
        // (inside the allocation of `out`: copied before it is released)
        let marks = unsafe { std::slice::from_raw_parts(mk as *const i64, nm as usize) }.to_vec();
        unsafe { kx_free_packed(out) };
        Ok((v, marks, ns, ld))
    }

    /// `submit_request_joined` with the request's limit spec ("limiter" in kokorox_hip.h; `join` = None: no join): body, marks,
    /// sample count, and [p, g, I, n_g, r] of the request.
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn submit_request_limited(&self, chunks: &[Vec<i64>], styles: &[f32], speed: f32, seed: u64, format: i32,
                                  join: Option<KxJoin>, limit: KxLimit) -> Result<(Vec<u8>, Vec<i64>, i64, [f64; 5]), Box<dyn Error>> {
        if styles.len() != KX_STYLE_DIM * chunks.len() {
            return Err("submit_request: one style row of 256 floats per chunk is required".into());
        }
        let ids: Vec<i64> = chunks.iter().flatten().copied().collect();
        let lens: Vec<i32> = chunks.iter().map(|c| c.len() as i32).collect();
        let mut out: *mut c_void = ptr::null_mut();
        let mut mk: *mut i64 = ptr::null_mut();
        let (mut nb, mut ns, mut nm) = (0i64, 0i64, 0i64);
        let mut lm = [0f64; 5];
        let mut err = vec![0 as c_char; 256];
        let rc = unsafe {
            kx_dispatcher_submit_request_limited(self.d, ids.as_ptr(), lens.as_ptr(), lens.len() as c_int, styles.as_ptr(), ptr::null(),
                                                 ptr::null(), 0, speed, seed, format, &mut out, &mut nb, &mut ns, &mut mk, &mut nm,
                                                 join.as_ref().map_or(ptr::null(), |j| j as *const KxJoin), &limit, lm.as_mut_ptr(),
                                                 err.as_mut_ptr(), err.len())
        };
        if rc != KX_OK {
            return Err(format!("kokorox_hip error {}: {}", rc, cstr_buf(&err)).into());
        }
        let v = unsafe { std::slice::from_raw_parts(out as *const u8, nb as usize) }.to_vec();
        // (inside the allocation of `out`: copied before it is released)
        let marks = unsafe { std::slice::from_raw_parts(mk as *const i64, nm as usize) }.to_vec();
        unsafe { kx_free_packed(out) };
        Ok((v, marks, ns, lm))
    }

    /// The WebSocket chunk of `encode_audio` (kokorox-websocket/src/lib.rs:696-736) for a request: base64 of its 16-bit WAV
    /// file, encoded on the GPU, as the `String` the server puts into its JSON message.
    pub fn submit_request_base64(&self, chunks: &[Vec<i64>], voice: Voice, speed: f32, seed: u64)
                                 -> Result<String, Box<dyn Error>> {
        let (bytes, _) = self.submit_request(chunks, voice, speed, seed, KX_PACK_WAV16_BASE64)?;
        Ok(String::from_utf8(bytes)?) // (base64 is ASCII: this never fails on what the library returns)
    }

    /// A request as telephony wants it: raw G.711 mu-law bytes at 8 kHz, resampled and encoded on the GPU.
    pub fn submit_request_mulaw_8k(&self, chunks: &[Vec<i64>], voice: Voice, speed: f32, seed: u64) -> Result<Vec<u8>, Box<dyn Error>> {
        let (bytes, _) = self.submit_request(chunks, voice, speed, seed, KX_PACK_MULAW | KX_PACK_RATE_8000)?;
        Ok(bytes)
    }

    /// Batches each model (GPU) has run so far.
    pub fn model_batches(&self) -> Vec<i64> {
        let mut v = vec![0i64; self._models.len()];
        unsafe { kx_dispatcher_model_batches(self.d, v.as_mut_ptr(), v.len() as c_int) };
        v
    }

    /// (requests replayed one by one after an INVALID-class batch failure, batches retried after a DEVICE-class one).
    pub fn failures(&self) -> (i64, i64) {
        let (mut a, mut b) = (0i64, 0i64);
        unsafe { kx_dispatcher_failures(self.d, &mut a, &mut b) };
        (a, b)
    }

    /// (requests, batches, largest batch in rows: a request of n chunks is n rows) so far.
    pub fn stats(&self) -> (i64, i64, i64) {
        let (mut a, mut b, mut c) = (0i64, 0i64, 0i64);
        unsafe { kx_dispatcher_stats(self.d, &mut a, &mut b, &mut c) };
        (a, b, c)
    }
}

impl Drop for HipKokoDispatcher {
    fn drop(&mut self) {
        unsafe { kx_dispatcher_destroy(self.d) } // waits for queued requests; the models drop afterwards
    }
}
