"""ctypes mirror of the reference's Swift surface on top of the C ABI.

The reference's host is Swift (no Swift toolchain exists in this image or on the GPU
box), so this module plays the Swift caller's role for tests and benchmarks, with the
same names, argument meaning and error behaviour:

    generateSpectrogram(audio)        Whisper/Whisper/stft.swift:8-19
    Whisper(...)                      Whisper/Whisper/Whisper.swift:11-21   (init)
    Whisper.encode(audio)             Whisper/Whisper/Whisper.swift:23-31
    Whisper.decode(audioFeatures)     Whisper/Whisper/Whisper.swift:33-40
    Whisper.LANGUAGES                 Whisper/Whisper/Whisper.swift:12

Everything goes through libwhisper_mi355x.so (include/whisper_mi355x.h).  There is no
CPU fallback: if the library is missing, or no gfx950 device is usable, calls raise.
"""
import contextlib
import ctypes
import math
import os
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WM_LIB_PATH") or os.path.join(HERE, "libwhisper_mi355x.so")   # WM_LIB_PATH: A/B builds
# the product objects + the wmdbg_* kernel test hooks (include/whisper_mi355x_debug.h): tests / tools only
DEBUG_LIB_PATH = os.environ.get("WM_DBG_LIB_PATH") or os.path.join(HERE, "libwhisper_mi355x_dbg.so")   # A/B builds (tools/)

WM_OK = 0
WM_I16, WM_F32, WM_F64, WM_BF16 = 0, 1, 2, 3
WM_MEM_HOST, WM_MEM_DEVICE = 0, 1

N_SAMPLES = 16000 * 30  # ContentView.swift:57
N_FRAMES = 3000

_DTYPES = {np.dtype(np.int16): WM_I16, np.dtype(np.float32): WM_F32, np.dtype(np.float64): WM_F64}


class WhisperError(RuntimeError):
    """Plays the role of Swift's `throws` (Whisper.swift:17,23,33)."""

    def __init__(self, status, message):
        super().__init__("wm status %d: %s" % (status, message))
        self.status = status


class wm_dims(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
        "n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# ModelDimensions of the checkpoints named in BASELINE.json / SURVEY.md 8a.
MODEL_DIMS = {
    "tiny.en": dict(n_mels=80, n_audio_ctx=1500, n_audio_state=384, n_audio_head=6, n_audio_layer=4,
                    n_vocab=51864, n_text_ctx=448, n_text_state=384, n_text_head=6, n_text_layer=4),
    "base": dict(n_mels=80, n_audio_ctx=1500, n_audio_state=512, n_audio_head=8, n_audio_layer=6,
                 n_vocab=51865, n_text_ctx=448, n_text_state=512, n_text_head=8, n_text_layer=6),
    "small": dict(n_mels=80, n_audio_ctx=1500, n_audio_state=768, n_audio_head=12, n_audio_layer=12,
                  n_vocab=51865, n_text_ctx=448, n_text_state=768, n_text_head=12, n_text_layer=12),
    "large-v2": dict(n_mels=80, n_audio_ctx=1500, n_audio_state=1280, n_audio_head=20,
                     n_audio_layer=32, n_vocab=51865, n_text_ctx=448, n_text_state=1280,
                     n_text_head=20, n_text_layer=32),
    "large-v3": dict(n_mels=128, n_audio_ctx=1500, n_audio_state=1280, n_audio_head=20,
                     n_audio_layer=32, n_vocab=51866, n_text_ctx=448, n_text_state=1280,
                     n_text_head=20, n_text_layer=32),
}

_lib = None
_dbg_lib = None


def load_debug_library():
    """dlopen libwhisper_mi355x_dbg.so: the same objects as the product plus the wmdbg_* hooks."""
    global _dbg_lib
    if _dbg_lib is None:
        _dbg_lib = load_library(DEBUG_LIB_PATH)
    return _dbg_lib


def load_library(path=None):
    """dlopen the product library.  Fails loudly (no fallback) when it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise WhisperError(-1, "%s not found: run `python __graft_entry__.py build` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback" % p)
    lib = ctypes.CDLL(p)  # RTLD_LOCAL: never interpose another library's symbols
    vp, ip, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    pp = ctypes.POINTER(ctypes.c_void_p)
    lib.generate_spectrogram.argtypes = [vp, vp]
    lib.generate_spectrogram.restype = None
    lib.wm_last_error.restype = ctypes.c_char_p
    sigs = {
        "wm_logmel": [vp, vp, ip, ip, ip, vp, ip, ip],
        "wm_create_frontend": [ip, pp],
        "wm_create": [ctypes.POINTER(wm_dims), ip, pp],
        "wm_clone": [vp, pp],
        "wm_set_tensor": [vp, ctypes.c_char_p, vp, sz],
        "wm_get_tensor": [vp, ctypes.c_char_p, vp, sz],
        "wm_load_weights": [vp, ctypes.c_char_p],
        "wm_init_synthetic": [vp, ctypes.c_uint64],
        "wm_init_synthetic_gain": [vp, ctypes.c_uint64, ctypes.c_float],
        "wm_finalize": [vp],
        "wm_get_dims": [vp, ctypes.POINTER(wm_dims)],
        "wm_encode": [vp, vp, ip, vp, ip],
        "wm_decode_logits": [vp, vp, ip, ip, vp, vp, ip],
        "wm_detect_language": [vp, vp, ip, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, ip],
        "wm_transcribe_greedy": [vp, vp, ip, ip, vp, ip, ip, ctypes.c_int32, vp, vp, ip],
        "wm_transcribe": [vp, vp, ip, ip, vp, ip, ip, ctypes.c_int32, vp, vp, vp, vp, vp, ip],
        "wm_logmel_long": [vp, vp, ip, vp, ip, ip, vp, ip],
        "wm_transcribe_mel": [vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, ip, ctypes.c_int32, vp, vp, vp, vp, vp, ip],
        "wm_transcribe_mel_ragged": [vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, ip, vp, ip, ctypes.c_int32, vp, vp, vp, vp, vp, ip],
        "wm_transcribe_mel_best_of": [vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, ip, vp, ip, ctypes.c_float, ip, ctypes.c_int32, vp,
                                      vp, vp, vp, vp, vp, ip],
        "wm_transcribe_mel_beam": [vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, ip, ip, ip, ctypes.c_float, ip, ctypes.c_int32, vp,
                                   vp, vp, vp, vp, vp, vp, vp, ip],
        "wm_transcribe_mel_speculative": [vp, vp, vp, vp, vp, vp, vp, ip, vp, ip, ip, ip, ctypes.c_int32, vp, vp, vp, vp, vp, vp, ip],
        "wm_rank_candidates": [vp, vp, vp, ip, ip, ip, ctypes.c_int32, ctypes.c_float, vp, vp],
        "wm_set_token_budgets": [vp, vp, ip],
        "wm_set_alignment_heads": [vp, vp, vp, ip],
        "wm_align": [vp, vp, ip, ip, vp, ip, ctypes.c_int32, ctypes.c_int32, vp, vp, ip, vp, ip, ctypes.c_float, vp, vp, ip],
        "wm_align_mel": [vp, vp, vp, vp, vp, vp, ip, vp, ip, ctypes.c_int32, ctypes.c_int32, vp, vp, ip, ip, ctypes.c_float, vp, vp,
                         ip],
        "wm_windows_encode": [vp, vp, vp, vp, vp, vp, ip, ip, pp],
        "wm_windows_count": [vp],
        "wm_transcribe_windows": [vp, vp, vp, ip, vp, ip, vp, ip, vp, ip, ctypes.c_float, ip, ctypes.c_int32, vp, vp, vp, vp, vp,
                                  vp],
        "wm_transcribe_windows_beam": [vp, vp, vp, ip, vp, ip, vp, ip, ip, ip, ctypes.c_float, ip, ctypes.c_int32, vp, vp, vp, vp,
                                       vp, vp, vp, vp],
        "wm_align_windows": [vp, vp, vp, ip, vp, ip, ctypes.c_int32, ctypes.c_int32, vp, vp, ip, ip, ctypes.c_float, vp, vp],
        "wm_windows_detect_language": [vp, vp, vp, ip, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, vp],
        "wm_transcribe_mel_aligned": [vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, ip, vp, ip, ctypes.c_int32, vp, ip, ctypes.c_float,
                                      vp, vp, vp, vp, vp, ip],
        "wm_transcribe_windows_aligned": [vp, vp, vp, ip, vp, ip, vp, ip, vp, ip, ctypes.c_int32, vp, ip, ctypes.c_float, vp, vp,
                                          vp, vp, vp],
        "wm_transcribe_mel_best_of_aligned": [vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, ip, vp, ip, ctypes.c_float, ip, ctypes.c_int32,
                                              vp, ip, ctypes.c_float, vp, vp, vp, vp, vp, vp, ip],
        "wm_transcribe_windows_best_of_aligned": [vp, vp, vp, ip, vp, ip, vp, ip, vp, ip, ctypes.c_float, ip, ctypes.c_int32, vp, ip,
                                                  ctypes.c_float, vp, vp, vp, vp, vp, vp],
        "wm_transcribe_mel_beam_aligned": [vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, ip, ip, ip, ctypes.c_float, ip, ctypes.c_int32, vp,
                                           ip, ctypes.c_float, vp, vp, vp, vp, vp, vp, vp, vp, ip],
        "wm_transcribe_windows_beam_aligned": [vp, vp, vp, ip, vp, ip, vp, ip, ip, ip, ctypes.c_float, ip, ctypes.c_int32, vp, ip,
                                               ctypes.c_float, vp, vp, vp, vp, vp, vp, vp, vp],
        "wm_set_lanes": [vp, ip],
        "wm_dev_malloc": [vp, sz, pp],
        "wm_dev_free": [vp, vp],
        "wm_dev_upload": [vp, vp, vp, sz],
        "wm_dev_download": [vp, vp, vp, sz],
        "wm_sync": [vp],
        "wm_profile_enable": [vp, ip],
        "wm_profile_reset": [vp],
        "wm_profile_json": [vp, ctypes.c_char_p, sz],
        "wm_profile_overhead_us": [vp, vp],
        "wm_last_stage_ms": [vp, vp],
        "wm_vocab_load": [ctypes.c_char_p, pp],
        "wm_vocab_size": [vp],
        "wm_detokenize": [vp, vp, ip, ip, vp, sz, vp],
        "wm_wav_open": [ctypes.c_char_p, pp],
        "wm_wav_num_chunks": [vp],
        "wm_wav_read_chunks": [vp, ip, ip, vp],
        "wm_resample_filter": [ip, vp, sz, vp, vp, vp],
        "wm_resample_16k": [vp, vp, ip, vp, vp, vp, ip, vp, ip],
        "wm_resample_16k_mix": [vp, vp, ip, vp, vp, vp, ip, vp, vp, vp, ip],
        "wm_channel_activity": [vp, vp, vp, ip, vp, ip],
        "wm_vad_energy": [vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, vp, vp, ip],
        "wm_streams_create": [vp, ip, ip, ip, pp],
        "wm_streams_free": [vp, vp],
        "wm_streams_push": [vp, vp, vp, ip, vp, ip],
        "wm_streams_reset": [vp, vp, ip],
        "wm_streams_frames": [vp, vp, vp, vp, vp],
        "wm_streams_window": [vp, vp, ip, vp, vp, vp, vp, vp, ip],
        "wm_vad_segments": [vp, ctypes.c_int64, vp, vp, ip, vp, vp],
        "wm_audio_open": [ctypes.c_char_p, pp],
        "wm_audio_sample_rate": [vp],
        "wm_audio_channels": [vp],
        "wm_audio_bits": [vp],
        "wm_audio_is_float": [vp],
        "wm_audio_read": [vp, ctypes.c_int64, ctypes.c_int64, vp],
        "wm_audio_read_i16": [vp, ctypes.c_int64, ctypes.c_int64, vp],
        "wm_multi_create": [ctypes.POINTER(wm_dims), vp, ip, pp],
        "wm_multi_size": [vp],
        "wm_multi_device_ctx": [vp, ip, pp],
        "wm_multi_transcribe_greedy": [vp, vp, ip, ip, vp, ip, ip, ctypes.c_int32, vp, vp],
        "wm_multi_partition": [ip, ip, ip, vp, vp],
        "wm_multi_pack_tokens": [vp, vp, ip, ip, ip, vp],
        "wm_multi_unpack_tokens": [vp, ip, ip, ip, ip, vp, vp],
    }
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    if hasattr(lib, "wmdbg_streams_set_position"):   # the debug library
        lib.wmdbg_streams_set_position.argtypes = [vp, vp, ip, ctypes.c_int64]
        lib.wmdbg_streams_set_position.restype = ctypes.c_int
        lib.wmdbg_streams_min_capacity.argtypes = [ip]
        lib.wmdbg_streams_min_capacity.restype = ctypes.c_int
    lib.wm_destroy.argtypes = [vp]
    lib.wm_destroy.restype = None
    lib.wm_windows_free.argtypes = [vp]
    lib.wm_windows_free.restype = None
    lib.wm_windows_bytes.argtypes = [vp]
    lib.wm_windows_bytes.restype = sz
    lib.wm_multi_destroy.argtypes = [vp]
    lib.wm_multi_destroy.restype = None
    lib.wm_vocab_free.argtypes = [vp]
    lib.wm_vocab_free.restype = None
    lib.wm_wav_close.argtypes = [vp]
    lib.wm_wav_close.restype = None
    lib.wm_wav_num_samples.argtypes = [vp]
    lib.wm_wav_num_samples.restype = ctypes.c_long
    lib.wm_audio_close.argtypes = [vp]
    lib.wm_audio_close.restype = None
    lib.wm_audio_num_frames.argtypes = [vp]
    lib.wm_audio_num_frames.restype = ctypes.c_int64
    lib.wm_resample_out_len.argtypes = [ctypes.c_int64, ip]
    lib.wm_resample_out_len.restype = ctypes.c_int64
    lib.wm_vad_default_params.argtypes = [vp]
    lib.wm_vad_default_params.restype = None
    if path is None:
        _lib = lib
    return lib


def _check(lib, status):
    if status != WM_OK:
        raise WhisperError(status, lib.wm_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _ptr_or_null(a):
    return None if a is None else _ptr(a)


def generateSpectrogram(audio):
    """stft.swift:8-19.  audio: 480000 doubles -> 240000 doubles ([80][3000] row-major).

    Inserts 200 zeros at the front (stft.swift:10), appends 200 (stft.swift:11), allocates
    the 80*3000 result (stft.swift:12) and calls the C symbol `generate_spectrogram` with
    raw pointers (stft.swift:13-17).  Like the Swift caller, no length check is made by
    the callee; this wrapper checks because Python has no UB to lean on."""
    lib = load_library()
    a = np.asarray(audio, dtype=np.float64)
    if a.shape != (N_SAMPLES,):
        raise ValueError("generateSpectrogram expects %d samples, got %r" % (N_SAMPLES, a.shape))
    buf = np.zeros(N_SAMPLES + 400, dtype=np.float64)
    buf[200:200 + N_SAMPLES] = a
    result = np.zeros(80 * N_FRAMES, dtype=np.float64)
    lib.generate_spectrogram(_ptr(buf), _ptr(result))
    return result


class wm_decode_opts(ctypes.Structure):
    _fields_ = [("temperature", ctypes.c_float), ("seed", ctypes.c_uint64), ("no_speech_token", ctypes.c_int32),
                ("sot_index", ctypes.c_int32)]


MAX_ALTERNATIVES = 16   # WM_MAX_ALTERNATIVES


class wm_alternatives_out(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("rows", ctypes.c_int64), ("max_new", ctypes.c_int32), ("tokens", ctypes.c_void_p),
                ("logprobs", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("entropy", ctypes.c_void_p)]


def alternatives_arg(alternatives, beam_size=None, draft=None):
    """`alternatives=` of the transcribe wrappers as wm_request_alternatives' n: None (no request) or an integer in 1 ..
    MAX_ALTERNATIVES.  ValueError -- before any library call -- for anything else, and together with beam search or a draft
    model (a beam's alternatives need its ancestry; a speculative call verifies the greedy choice alone)."""
    if alternatives is None:
        return None
    n = alternatives
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or not 1 <= n <= MAX_ALTERNATIVES:
        raise ValueError("alternatives: an integer in 1 .. %d (None: no request)" % MAX_ALTERNATIVES)
    if beam_size is not None:
        raise ValueError("alternatives are not served by beam search (beam_size)")
    if draft is not None:
        raise ValueError("alternatives are not served by speculative decoding (draft)")
    return int(n)


def given_arg(given, beam_size=None, draft=None):
    """`given=` of the transcribe wrappers as wm_set_given_tokens' table: None (no table), or one id list per hypothesis row of
    the call (B rows; B * best_of in the order [B][best_of]; an empty list or None: the row decodes freely).  Returns (tokens i32
    [n][stride], lens i32 [n]).  ValueError -- before any library call -- for anything else, and together with beam search or a
    draft model (neither serves a table)."""
    if given is None:
        return None
    if beam_size is not None:
        raise ValueError("given tokens are not served by beam search (beam_size)")
    if draft is not None:
        raise ValueError("given tokens are not served by speculative decoding (draft)")
    try:
        rows = [np.zeros(0, dtype=np.int64) if g is None else np.asarray(g).reshape(-1) for g in given]
    except TypeError:
        raise ValueError("given: one id list per hypothesis row (None: no table)")
    if not rows:
        raise ValueError("given: one id list per hypothesis row (None: no table)")
    for r in rows:
        if r.size and (not np.issubdtype(r.dtype, np.integer) or r.min() < 0 or r.max() > 0x7FFFFFFF):
            raise ValueError("given: token ids are non-negative integers")
    lens = np.array([r.size for r in rows], dtype=np.int32)
    tok = np.zeros((len(rows), max(1, int(lens.max()))), dtype=np.int32)
    for i, r in enumerate(rows):
        tok[i, :r.size] = r
    return tok, lens


class Alternatives:
    """The arrays of one wm_request_alternatives request, filled by the transcribe call that consumes it: tokens i32 / logprobs
    f32 [rows][max_new][n] (-1 / 0 past counts and past a row's length), counts i32 [rows][max_new], entropy f32
    [rows][max_new] (None when not requested), in nats."""

    def __init__(self, n, rows, max_new, entropy=True):
        self.n, self.rows, self.max_new = int(n), int(rows), int(max_new)
        self.tokens = np.full((self.rows, self.max_new, self.n), -1, dtype=np.int32)
        self.logprobs = np.zeros((self.rows, self.max_new, self.n), dtype=np.float32)
        self.counts = np.zeros((self.rows, self.max_new), dtype=np.int32)
        self.entropy = np.zeros((self.rows, self.max_new), dtype=np.float32) if entropy else None

    def attach(self, result, lead=None):
        """The arrays as attributes alt_tokens / alt_logprobs / alt_counts / entropy of `result`, rows reshaped to `lead`"""
        lead = (self.rows,) if lead is None else tuple(lead)
        result.alt_tokens = self.tokens.reshape(lead + (self.max_new, self.n))
        result.alt_logprobs = self.logprobs.reshape(lead + (self.max_new, self.n))
        result.alt_counts = self.counts.reshape(lead + (self.max_new,))
        result.entropy = None if self.entropy is None else self.entropy.reshape(lead + (self.max_new,))
        return result


def token_alternatives(alt_tokens, alt_logprobs, alt_counts):
    """One row's alternatives [max_new][n] as a list per token of (id, logprob) pairs"""
    return [[(int(alt_tokens[i, j]), float(alt_logprobs[i, j])) for j in range(int(alt_counts[i]))]
            for i in range(alt_tokens.shape[0])]


class TranscribeResult:
    """What Context.transcribe returns.  tokens i32 [B][max_new] (padded with eot), lens i32 [B], logprobs f32 [B][max_new]
    (0 past lens), sum_logprob / avg_logprob f64 [B], no_speech_prob f32 [B] (None without a no-speech token).
    sum_logprob adds the log-probs of all lens[b] tokens (the stopping eot included) and avg_logprob = sum / (n_text + 1),
    n_text = tokens before eot -- openai-whisper's DecodingTask.run (its finalize pads with eot).
    With alternatives=n: alt_tokens i32 / alt_logprobs f32 [B][max_new][n], alt_counts i32 and entropy f32 [B][max_new]
    (Alternatives); None when not requested."""
    alt_tokens = alt_logprobs = alt_counts = entropy = None

    def __init__(self, tokens, lens, logprobs, no_speech_prob, eot):
        self.tokens, self.lens, self.logprobs, self.no_speech_prob = tokens, lens, logprobs, no_speech_prob
        B = tokens.shape[0]
        self.sum_logprob = np.array([float(np.sum(logprobs[b, :lens[b]], dtype=np.float64)) for b in range(B)])
        self.n_text = np.array([n_text_tokens(tokens[b, :lens[b]], eot) for b in range(B)], dtype=np.int64)
        self.avg_logprob = self.sum_logprob / (self.n_text + 1)


class SpeculativeResult(TranscribeResult):
    """What Context.transcribe_mel_speculative returns: the TranscribeResult of the plain call, bit for bit, plus `stats`, i32
    [B][4] = (rounds, proposed, accepted, kept) per window (wm_spec_stats)."""

    def __init__(self, tokens, lens, logprobs, no_speech_prob, eot, stats):
        TranscribeResult.__init__(self, tokens, lens, logprobs, no_speech_prob, eot)
        self.stats = stats
        self.rounds, self.proposed, self.accepted, self.kept = (stats[:, i] for i in range(4))


class AlignedResult(TranscribeResult):
    """What Context.transcribe_mel_aligned / transcribe_windows_aligned return: a TranscribeResult plus start_frames i32
    [B][max_new + 1] -- entry k < lens[b] is the first audio frame (20 ms) of generated token k, entry lens[b] is the
    window's n_frames // 2, -1 behind (wm_transcribe_mel_aligned) --, and with capture_matrix=True `matrix`, the cost
    matrices f32 [B][max_new + 1][1500]."""

    def __init__(self, tokens, lens, logprobs, no_speech_prob, eot, start_frames, matrix=None):
        TranscribeResult.__init__(self, tokens, lens, logprobs, no_speech_prob, eot)
        self.start_frames, self.matrix = start_frames, matrix


def decode_alignment_text(tokens, length, start_frames, logprobs, eot, n_text=None):
    """One row of an AlignedResult as the arrays window_word_timestamps / word_timestamps take: (text_tokens [n],
    text_start_frames i32 [n + 1], token_probs f64 [n]).  The text tokens are the generated tokens tokens[:length] with id
    < eot (timestamp tokens and the stopping eot have rows of the alignment but are no text), the first n_text of them when
    n_text is given (a long-form window keeps the tokens of its segments only).  Boundary i < n is the start frame of text
    token i, the final boundary the start frame of the row BEHIND the last text token -- the next generated token's, or
    start_frames[length], the window's end.  token_probs = exp(logprob): the probability under the filtered distribution the
    decode chose from, not wm_align's softmax over the raw text logits.  Without a text token: ([], [start_frames[0]], [])."""
    toks = np.asarray(tokens).reshape(-1)
    sf = np.asarray(start_frames).reshape(-1)
    lp = np.asarray(logprobs, dtype=np.float64).reshape(-1)
    idx = [k for k in range(int(length)) if toks[k] < eot]
    if n_text is not None:
        if n_text > len(idx):
            raise ValueError("decode_alignment_text: the row has %d text tokens, not %d" % (len(idx), n_text))
        idx = idx[:int(n_text)]
    if not idx:
        return [], np.array([int(sf[0])], dtype=np.int32), np.zeros(0, dtype=np.float64)
    bounds = [int(sf[k]) for k in idx] + [int(sf[idx[-1] + 1])]
    return [int(toks[k]) for k in idx], np.array(bounds, dtype=np.int32), np.exp(lp[idx])


class BestOfResult:
    """What Context.transcribe_mel_best_of returns.  tokens i32 [B][N][max_new], lens i32 [B][N], logprobs f32 [B][N][max_new],
    no_speech_prob f32 [B] (candidate 0's; None without a no-speech token), best i32 [B] (wm_rank_candidates) and
    selected: the TranscribeResult of candidate best[b] of every row, with the same indices as its attribute `candidate`.
    With alternatives=n: alt_tokens / alt_logprobs [B][N][max_new][n], alt_counts / entropy [B][N][max_new] of every candidate
    (None when not requested), and `selected` carries the chosen candidate's."""
    alt_tokens = alt_logprobs = alt_counts = entropy = None

    def __init__(self, tokens, lens, logprobs, no_speech_prob, best, eot, alternatives=None):
        self.tokens, self.lens, self.logprobs, self.no_speech_prob, self.best = tokens, lens, logprobs, no_speech_prob, best
        rows = np.arange(tokens.shape[0])
        self.selected = TranscribeResult(np.ascontiguousarray(tokens[rows, best]), np.ascontiguousarray(lens[rows, best]),
                                         np.ascontiguousarray(logprobs[rows, best]), no_speech_prob, eot)
        self.selected.candidate = best
        if alternatives is not None:
            alternatives.attach(self, tokens.shape[:2])
            s = self.selected
            s.alt_tokens, s.alt_logprobs = (np.ascontiguousarray(a[rows, best]) for a in (self.alt_tokens, self.alt_logprobs))
            s.alt_counts = np.ascontiguousarray(self.alt_counts[rows, best])
            s.entropy = None if self.entropy is None else np.ascontiguousarray(self.entropy[rows, best])


MAX_BEAM, MAX_BEAM_HYPS = 8, 16   # WM_MAX_BEAM, WM_MAX_BEAM_HYPS


def beam_max_candidates(beam_size, patience=None):
    """openai-whisper's BeamSearchDecoder: max_candidates = round(beam_size * patience), patience None = 1.0.  Raises
    ValueError where wm_transcribe_mel_beam would reject the pair."""
    if beam_size is None:
        if patience is not None:
            raise ValueError("patience requires beam_size to be given")
        return None
    if int(beam_size) != beam_size or not 1 <= int(beam_size) <= MAX_BEAM:
        raise ValueError("beam_size must be an integer in 1 .. %d" % MAX_BEAM)
    pat = 1.0 if patience is None else float(patience)
    if not pat > 0.0:
        raise ValueError("patience must be positive")
    n = round(int(beam_size) * pat)
    if not 1 <= n <= MAX_BEAM_HYPS:
        raise ValueError("round(beam_size * patience) = %d outside 1 .. %d" % (n, MAX_BEAM_HYPS))
    return int(n)


class BeamResult:
    """What Context.transcribe_mel_beam returns, with S = max(beam_size, max_candidates): tokens i32 [B][S][max_new], lens i32
    [B][S] (a finished hypothesis counts its eot), n_hyp i32 [B], sum_logprob f32 [B][S] (the search's own running sums; -inf
    past n_hyp), logprobs f32 [B][S][max_new], no_speech_prob f32 [B] (beam 0's; None without a no-speech token), best i32 [B]
    and selected: the TranscribeResult of hypothesis best[b] of every row, whose sum_logprob is the search's f32 sum and
    avg_logprob = sum / (n_text + 1), with the same indices as its attribute `hypothesis`."""

    def __init__(self, tokens, lens, n_hyp, sum_logprob, logprobs, no_speech_prob, best, eot):
        self.tokens, self.lens, self.n_hyp, self.sum_logprob = tokens, lens, n_hyp, sum_logprob
        self.logprobs, self.no_speech_prob, self.best = logprobs, no_speech_prob, best
        rows = np.arange(tokens.shape[0])
        self.selected = TranscribeResult(np.ascontiguousarray(tokens[rows, best]), np.ascontiguousarray(lens[rows, best]),
                                         np.ascontiguousarray(logprobs[rows, best]), no_speech_prob, eot)
        self.selected.sum_logprob = sum_logprob[rows, best].astype(np.float64)
        self.selected.avg_logprob = self.selected.sum_logprob / (self.selected.n_text + 1)
        self.selected.hypothesis = best


def rank_candidates(tokens, lens, logprobs, eot, length_penalty=None):
    """wm_rank_candidates (openai-whisper's MaximumLikelihoodRanker; host only): tokens [B][N][max_new], lens [B][N],
    logprobs [B][N][max_new]; length_penalty None is openai-whisper's None.  Returns (best i32 [B], scores f64 [B][N])."""
    lib = load_library()
    tokens = np.ascontiguousarray(tokens, dtype=np.int32)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    logprobs = np.ascontiguousarray(logprobs, dtype=np.float32)
    if tokens.ndim != 3 or lens.shape != tokens.shape[:2] or logprobs.shape != tokens.shape:
        raise ValueError("rank_candidates: tokens / logprobs [B][N][max_new], lens [B][N]")
    B, N, max_new = tokens.shape
    best = np.empty(B, dtype=np.int32)
    scores = np.empty((B, N), dtype=np.float64)
    _check(lib, lib.wm_rank_candidates(_ptr(tokens), _ptr(lens), _ptr(logprobs), B, N, max_new, eot,
                                       float("nan") if length_penalty is None else float(length_penalty), _ptr(best),
                                       _ptr(scores)))
    return best, scores


def score_given(ctx, wset, rows, prompts, texts, eot, append_eot=True, length_penalty=None, alternatives=None, form=None):
    """The log-probs of texts the caller already has (CTranslate2's score_batch; n-best rescoring, "which of these K commands was
    spoken").  wset / rows: a Windows set and its rows (None: all) as for Context.transcribe_windows; prompts: one prompt for all,
    or one per row; texts: per row a list of texts, each a list of token ids.  append_eot: eot is scored behind every text
    (openai-whisper's sum_logprob includes it).  Every text is given whole with a token budget of its length, so nothing is
    decoded beyond it.
    Where every row has the same number K of texts this is ONE transcribe_windows_best_of(best_of=K) call at temperature 0 (a
    given candidate never draws): the K texts of a window share one read of its cross-attention K/V per position; otherwise one
    plain transcribe_windows call with the rows repeated.  Returns a SimpleNamespace: logprobs -- per row a list of f32 arrays,
    one per text --, sum_logprob and avg_logprob (openai-whisper's: sum / (len(text) + 1)) f64 lists of the same shape, `best` i32
    [rows] (the best-of call's ranking: wm_rank_candidates' rule under length_penalty; None on the plain path), `result` (the
    call's own result) and, with alternatives=n, per row and text alt_tokens / alt_logprobs / alt_counts / entropy.
    form: None keeps that choice; "rows" forces the plain call with the rows repeated -- the path Context.set_given_panel serves,
    several positions of every text per decoder step --; "best_of" forces the best-of call and raises ValueError where the rows
    do not all have the same number of texts."""
    if form not in (None, "rows", "best_of"):
        raise ValueError("score_given: form is None, 'rows' or 'best_of'")
    n_alt = alternatives_arg(alternatives)
    idx = list(range(len(wset))) if rows is None else [int(r) for r in np.asarray(rows).reshape(-1)]
    if len(texts) != len(idx) or any(len(t) == 0 for t in texts):
        raise ValueError("score_given: one non-empty list of texts per row")
    tail = [int(eot)] if append_eot else []
    given = [[[int(x) for x in t] + tail for t in ts] for ts in texts]
    if any(len(g) == 0 for gs in given for g in gs):
        raise ValueError("score_given: an empty text needs append_eot")
    max_new = max(len(g) for gs in given for g in gs)
    K = len(given[0])
    same = all(len(gs) == K for gs in given)
    if form == "best_of" and not same:
        raise ValueError("score_given: form='best_of' needs the same number of texts for every row")
    if form == "rows":
        same = False
    pr = prompts
    if not same and not (isinstance(prompts, np.ndarray) and prompts.ndim == 1) and np.ndim(prompts[0]) != 0:
        pr = [prompts[w] for w, gs in enumerate(given) for _ in gs]   # a prompt per row: repeated with the row
    flat = [g for gs in given for g in gs]
    if same:
        r = ctx.transcribe_windows_best_of(wset, idx, pr, max_new, K, eot=eot, temperature=0.0, length_penalty=length_penalty,
                                           budgets=[max(len(g) for g in gs) for gs in given], alternatives=n_alt, given=flat)
        lp = [[r.logprobs[w, k, :len(g)].copy() for k, g in enumerate(gs)] for w, gs in enumerate(given)]
        alt = [[(w, k) for k in range(K)] for w in range(len(idx))]
        best = r.best
    else:
        rep_rows = [idx[w] for w, gs in enumerate(given) for _ in gs]
        r = ctx.transcribe_windows(wset, rep_rows, pr, max_new, eot=eot, budgets=[len(g) for g in flat], alternatives=n_alt,
                                   given=flat)
        at = iter(range(len(flat)))
        alt = [[(next(at),) for _ in gs] for gs in given]
        lp = [[r.logprobs[a[0], :len(g)].copy() for a, g in zip(al, gs)] for al, gs in zip(alt, given)]
        best = None
    out = types.SimpleNamespace(logprobs=lp, best=best, result=r)
    out.sum_logprob = [[float(np.sum(a, dtype=np.float64)) for a in row] for row in lp]
    out.avg_logprob = [[s_ / (len(t) + 1) for s_, t in zip(srow, ts)] for srow, ts in zip(out.sum_logprob, texts)]
    if n_alt:
        for name in ("alt_tokens", "alt_logprobs", "alt_counts", "entropy"):
            a = getattr(r, name)
            setattr(out, name, [[a[i][:len(g)] for i, g in zip(al, gs)] for al, gs in zip(alt, given)])
    return out


def n_text_tokens(toks, eot):
    """generated tokens before the first eot"""
    toks = np.asarray(toks)
    hit = np.flatnonzero(toks == eot) if eot >= 0 else np.array([], dtype=np.int64)
    return int(hit[0]) if hit.size else int(toks.size)


def compression_ratio_text(text):
    """openai-whisper's rule (whisper/utils.py compression_ratio): UTF-8 bytes over their zlib-compressed size."""
    b = text.encode("utf-8")
    return len(b) / len(zlib.compress(b))


def compression_ratio_tokens(tokens, vocab_size):
    """transformers' rule for token ids without a tokenizer (generation_whisper.py _retrieve_compression_ratio): every id as
    int(log2(vocab_size) / 8) + 1 little-endian bytes, over their zlib-compressed size."""
    length = int(math.log2(vocab_size) / 8) + 1
    b = b"".join(int(t).to_bytes(length, "little") for t in np.asarray(tokens).tolist())
    return len(b) / len(zlib.compress(b))


FALLBACK_TEMPERATURES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)


def fallback_seed(seed, k):
    """Sampling seed of temperature step k of transcribe_with_fallback."""
    return (int(seed) + int(k)) & 0xFFFFFFFFFFFFFFFF


def fallback_step_extra(t, best_of=None, length_penalty=None, beam_size=None, patience=None):
    """The keywords the fallback step at temperature t adds to Context.transcribe_mel / transcribe_windows: openai-whisper
    uses beam_size at temperature 0 and best_of above it; {}: the plain call."""
    if beam_size is not None and t == 0:
        return dict(beam_size=beam_size, patience=patience, length_penalty=length_penalty)
    if best_of is not None and t > 0:
        return dict(best_of=best_of, length_penalty=length_penalty)
    return {}


def sampling_rules_args(top_k=None, top_p=None, min_p=None):
    """top_k / top_p / min_p of transcribe_with_fallback and transcribe_long as the arguments of Context.set_sampling_rules:
    None when all three are None (the rules are not touched), else (top_k, top_p, min_p) with a None read as off (0, 1.0, 0.0).
    ValueError -- before any library call -- for top_k < 0 or not an integer, top_p outside (0, 1], min_p outside [0, 1), a NaN."""
    if top_k is None and top_p is None and min_p is None:
        return None
    k = 0 if top_k is None else top_k
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 0 or k > 2 ** 31 - 1:
        raise ValueError("top_k: an integer >= 0 (0: off)")
    p = 1.0 if top_p is None else float(top_p)
    if not (0.0 < p <= 1.0):
        raise ValueError("top_p: a number in (0, 1] (1: off)")
    m = 0.0 if min_p is None else float(min_p)
    if not (0.0 <= m < 1.0):
        raise ValueError("min_p: a number in [0, 1) (0: off)")
    return int(k), p, m


MAX_CST_STATES, MAX_CST_EDGES = 4096, 65536   # WM_MAX_CST_STATES, WM_MAX_CST_EDGES


class Constraint:
    """A token automaton for Context.set_constraint (wm_set_constraint), as that call's flat arrays: edge_beg i32 [S + 1],
    edge_tok / edge_next i32 [E] (tokens strictly ascending within a state; next -1: forbidden), def_next i32 [S] (-1: a text id
    without an explicit edge is forbidden), accept u8 [S] (eot is allowed).  Built by constraint_from_choices / constraint_join,
    or from the arrays of any grammar compiler.  The library validates it; the ids are the caller's tokenizer's."""

    def __init__(self, edge_beg, edge_tok, edge_next, def_next, accept):
        self.edge_beg = np.ascontiguousarray(edge_beg, dtype=np.int32).reshape(-1)
        self.edge_tok = np.ascontiguousarray(edge_tok, dtype=np.int32).reshape(-1)
        self.edge_next = np.ascontiguousarray(edge_next, dtype=np.int32).reshape(-1)
        self.def_next = np.ascontiguousarray(def_next, dtype=np.int32).reshape(-1)
        self.accept = np.ascontiguousarray(accept, dtype=np.uint8).reshape(-1)
        S = self.def_next.size
        if S < 1 or self.edge_beg.size != S + 1 or self.accept.size != S or self.edge_tok.size != self.edge_next.size \
                or int(self.edge_beg[-1]) != self.edge_tok.size:
            raise ValueError("Constraint: edge_beg [S + 1], edge_tok / edge_next [edge_beg[S]], def_next / accept [S], S >= 1")

    @property
    def n_states(self):
        return int(self.def_next.size)

    @property
    def n_edges(self):
        return int(self.edge_tok.size)


def constraint_from_choices(choices, repeat=False):
    """The automaton of a list of token sequences (a trie from state 0): exactly those sequences are allowed, eot where one ends.
    repeat=True: where a sequence ends the next token may also start another one (the ends lead back to the root's edges) --
    digit strings, several commands in a row; the empty output is then allowed too.  A sequence that is a prefix of another is
    fine.  ValueError for an empty list, an empty sequence, a negative id or a trie above MAX_CST_STATES / MAX_CST_EDGES."""
    seqs = [tuple(int(t) for t in c) for c in choices]
    if not seqs or any(len(q) == 0 or min(q) < 0 for q in seqs):
        raise ValueError("constraint_from_choices: a non-empty list of non-empty sequences of ids >= 0")
    kids, accept = [{}], [bool(repeat)]
    for q in seqs:
        s = 0
        for i, t in enumerate(q):
            if repeat and i == len(q) - 1:   # the end of a phrase IS the root: it accepts and continues with any first token
                if kids[s].get(t, 0) != 0:
                    raise ValueError("constraint_from_choices: with repeat, a sequence may not be a prefix of another")
                kids[s][t] = 0
                break
            if kids[s].get(t) == 0 and repeat:
                raise ValueError("constraint_from_choices: with repeat, a sequence may not be a prefix of another")
            if t not in kids[s]:
                kids[s][t] = len(kids)
                kids.append({})
                accept.append(False)
            s = kids[s][t]
        else:
            accept[s] = True
    # the leaves -- accepting, nothing behind them -- are ONE state: 4096 one-token phrases are two states, not 4097
    keep, num, leaf = [], {}, None       # the states that stay, old index -> new index, the shared leaf's new index
    for i, k in enumerate(kids):
        if i > 0 and not k:
            if leaf is None:
                leaf = len(keep)
                keep.append(i)
            num[i] = leaf
        else:
            num[i] = len(keep)
            keep.append(i)
    if len(keep) > MAX_CST_STATES or sum(len(k) for k in kids) > MAX_CST_EDGES:
        raise ValueError("constraint_from_choices: more than %d states or %d edges" % (MAX_CST_STATES, MAX_CST_EDGES))
    beg, tok, nxt = [0], [], []
    for i in keep:
        for t in sorted(kids[i]):
            tok.append(t)
            nxt.append(num[kids[i][t]])
        beg.append(len(tok))
    return Constraint(beg, tok, nxt, [-1] * len(keep), [accept[i] for i in keep])


def constraint_join(automata):
    """Disjoint automata as ONE (states and edges concatenated, targets shifted) and the start state of each: a grammar per
    request in one batched call -- Context.set_constraint(joined), then Context.set_constraint_rows([starts[i] ...]) per call.
    -> (Constraint, starts)."""
    automata = list(automata)
    if not automata or not all(isinstance(a, Constraint) for a in automata):
        raise ValueError("constraint_join: a non-empty list of Constraint")
    beg, tok, nxt, dn, acc, starts = [np.zeros(1, np.int32)], [], [], [], [], []
    s0 = e0 = 0
    for a in automata:
        starts.append(s0)
        beg.append(a.edge_beg[1:] + e0)
        tok.append(a.edge_tok)
        nxt.append(np.where(a.edge_next >= 0, a.edge_next + s0, -1))
        dn.append(np.where(a.def_next >= 0, a.def_next + s0, -1))
        acc.append(a.accept)
        s0 += a.n_states
        e0 += a.n_edges
    if s0 > MAX_CST_STATES or e0 > MAX_CST_EDGES:
        raise ValueError("constraint_join: more than %d states or %d edges" % (MAX_CST_STATES, MAX_CST_EDGES))
    return Constraint(np.concatenate(beg), np.concatenate(tok), np.concatenate(nxt), np.concatenate(dn), np.concatenate(acc)), starts


def constraint_args(constraint, constraint_rows=None, rows=None):
    """constraint / constraint_rows of transcribe_with_fallback and transcribe_long, checked before any library call: None or a
    Constraint; the rows None or one start state in [-1, n_states) per row (`rows`, where known).  -> the rows as a list or None."""
    if constraint is None:
        if constraint_rows is not None:
            raise ValueError("constraint_rows needs a constraint")
        return None
    if not isinstance(constraint, Constraint):
        raise ValueError("constraint: a Constraint (constraint_from_choices, constraint_join) or None")
    if constraint_rows is None:
        return None
    out = [-1 if r is None else int(r) for r in constraint_rows]
    if (rows is not None and len(out) != rows) or any(r < -1 or r >= constraint.n_states for r in out):
        raise ValueError("constraint_rows: one start state in [-1, n_states) per row")
    return out


def transcribe_with_fallback(ctx, pcm, prompt, max_new, eot, temperatures=FALLBACK_TEMPERATURES,
                             compression_ratio_threshold="auto", logprob_threshold=-1.0, no_speech_threshold=0.6,
                             vocab=None, seed=0, no_speech_token=-1, sot_index=0, vocab_size=None, best_of=None,
                             length_penalty=None, beam_size=None, patience=None, top_k=None, top_p=None, min_p=None,
                             alternatives=None, constraint=None, constraint_rows=None):
    """openai-whisper's decode_with_fallback, per chunk, over ctx.transcribe.

    Temperature step k decodes, as ONE batched call, the chunks that still need fallback (step 0: all of them) at
    temperatures[k] with seed fallback_seed(seed, k).  A chunk needs fallback when its compression ratio exceeds
    compression_ratio_threshold or its avg_logprob is below logprob_threshold; it does NOT need it when its
    no_speech_prob exceeds no_speech_threshold (checked last; needs no_speech_token >= 0).  A threshold of None is not
    checked.  A chunk keeps the result of the last call that decoded it.  Compression ratio: with a Vocab,
    openai-whisper's rule on the detokenized text; without one, transformers' token-byte rule.  The default
    compression_ratio_threshold "auto" is each rule's documented threshold: 2.4 with a Vocab, 1.35 without.

    best_of (openai-whisper's best_of; None: one sample): a step with temperature > 0 decodes best_of candidates per chunk
    in ONE wm_transcribe_mel_best_of call -- the chunks' Context.logmel windows at seek 0, the same seed and the same sample
    ids (the index within the call) -- and keeps each chunk's best one under length_penalty (rank_candidates).  The
    temperature-0 step is unchanged.

    top_k / top_p / min_p (all None: the context's sampling rules are not touched): the sampling rules of
    Context.set_sampling_rules are set on the context for the run -- a None of the three reads as off -- and cleared on leaving,
    also on an exception.  They act on the steps above temperature 0 (best_of candidates included); the temperature-0 step
    ignores them.  ValueError before any library call for a bad value (sampling_rules_args).

    beam_size (openai-whisper's beam_size, with patience; None: greedy): the temperature-0 step is ONE wm_transcribe_mel_beam
    call over the chunks' Context.logmel windows and keeps each chunk's best hypothesis under length_penalty; the steps
    above temperature 0 are unchanged.  patience without beam_size is a ValueError.

    alternatives (None; 1 .. MAX_ALTERNATIVES): Context.request_alternatives goes in front of every decode call of the loop,
    and the result gains alt_tokens / alt_logprobs [B][max_new][n], alt_counts / entropy [B][max_new] of each chunk's kept
    attempt.  ValueError before any library call for a value out of range or together with beam_size.

    constraint (None: the context's constraint is not touched; a Constraint): set on the context for the run
    (Context.set_constraint, eot is this call's eot) and cleared on leaving, also on an exception.  constraint_rows (None: every
    chunk starts in state 0): the start state of every chunk, -1 for an unconstrained one; Context.set_constraint_rows goes in
    front of every decode call of the loop with the starts of exactly that call's chunks.  ValueError before any library call
    for a bad value (constraint_args).

    Returns a dict of per-chunk arrays (tokens, lens, logprobs, sum_logprob, avg_logprob, no_speech_prob,
    compression_ratio, temperature, seed, needs_fallback) and `steps`: [(temperature, seed, chunk indices)] per call."""
    pcm = np.asarray(pcm)
    beam_max_candidates(beam_size, patience)
    sampling = sampling_rules_args(top_k, top_p, min_p)
    cst_rows = constraint_args(constraint, constraint_rows, pcm.shape[0])
    alt_kw = {} if alternatives_arg(alternatives, beam_size if beam_size is not None else patience) is None \
        else dict(alternatives=int(alternatives))

    def decode(todo, t, sd):
        extra = fallback_step_extra(t, best_of, length_penalty, beam_size, patience)
        if cst_rows is not None:
            ctx.set_constraint_rows([cst_rows[int(i)] for i in todo])
        if extra:
            n_mels = int(ctx.dims["n_mels"])
            mel = ctx.logmel(pcm[todo], n_mels=n_mels)
            return ctx.transcribe_mel(mel, np.arange(len(todo), dtype=np.int64) * (n_mels * N_FRAMES), N_FRAMES, 0, N_FRAMES,
                                      prompt, max_new, eot=eot, temperature=t, seed=sd, no_speech_token=no_speech_token,
                                      sot_index=sot_index, **extra, **alt_kw)
        return ctx.transcribe(pcm[todo], prompt, max_new, eot=eot, temperature=t, seed=sd,
                              no_speech_token=no_speech_token, sot_index=sot_index, **alt_kw)
    if sampling is not None:
        ctx.set_sampling_rules(*sampling)
    try:
        if constraint is not None:
            ctx.set_constraint(constraint, eot=eot)
        return fallback_decode(decode, pcm.shape[0], int(ctx.dims["n_vocab"]) if vocab_size is None else vocab_size, max_new,
                               eot, temperatures, compression_ratio_threshold, logprob_threshold, no_speech_threshold, vocab,
                               seed)
    finally:
        try:
            if constraint is not None:
                ctx.set_constraint(None)
        finally:
            if sampling is not None:
                ctx.set_sampling_rules()


def needs_fallback(compression_ratio, avg_logprob, no_speech_prob, compression_ratio_threshold, logprob_threshold,
                   no_speech_threshold):
    """The decision rule of the temperature fallback (openai-whisper's decode_with_fallback), stated once for fallback_decode and
    for transcribe_long's deferred rounds: an attempt fails when its compression ratio exceeds compression_ratio_threshold or its
    avg_logprob is below logprob_threshold -- and does not when its no_speech_prob (None: not computed) exceeds
    no_speech_threshold, checked last.  A threshold of None is not checked (compression_ratio_threshold: a number here, 'auto'
    is fallback_decode's to resolve)."""
    nf = False
    if compression_ratio_threshold is not None and compression_ratio > compression_ratio_threshold:
        nf = True
    if logprob_threshold is not None and avg_logprob < logprob_threshold:
        nf = True
    if no_speech_threshold is not None and no_speech_prob is not None and no_speech_prob > no_speech_threshold:
        nf = False
    return nf


def sampling_rows_args(row_temperatures, row_seeds, rows=None):
    """row_temperatures / row_seeds of the transcribe wrappers, checked before any library call: both None (-> None) or one
    value per row each (-> (f32 array, u64 array)); ValueError for one without the other or lengths that differ."""
    if row_temperatures is None and row_seeds is None:
        return None
    if row_temperatures is None or row_seeds is None:
        raise ValueError("row_temperatures and row_seeds: both or neither")
    t = np.ascontiguousarray([float(x) for x in row_temperatures], dtype=np.float32)
    sd = np.ascontiguousarray([int(x) & 0xFFFFFFFFFFFFFFFF for x in row_seeds], dtype=np.uint64)
    if t.size != sd.size or (rows is not None and t.size != rows):
        raise ValueError("row_temperatures and row_seeds: one value per row each")
    return t, sd


def fallback_decode(decode, B, vocab_size, max_new, eot, temperatures=FALLBACK_TEMPERATURES,
                    compression_ratio_threshold="auto", logprob_threshold=-1.0, no_speech_threshold=0.6, vocab=None,
                    seed=0):
    """The decision rule of transcribe_with_fallback over any decode: decode(indices, temperature, seed) returns the
    TranscribeResult of rows `indices` (an int array into 0 .. B - 1).  Same result dict."""
    if isinstance(compression_ratio_threshold, str):
        if compression_ratio_threshold != "auto":
            raise ValueError("compression_ratio_threshold: a number, None (not checked) or 'auto'")
        compression_ratio_threshold = 2.4 if vocab is not None else 1.35
    out = dict(tokens=np.full((B, max_new), eot, dtype=np.int32), lens=np.zeros(B, dtype=np.int32),
               logprobs=np.zeros((B, max_new), dtype=np.float32), sum_logprob=np.zeros(B), avg_logprob=np.zeros(B),
               no_speech_prob=np.full(B, np.nan, dtype=np.float32), compression_ratio=np.zeros(B),
               temperature=np.zeros(B), seed=np.zeros(B, dtype=np.uint64), needs_fallback=np.zeros(B, dtype=bool))
    steps = []
    todo = np.arange(B)
    for k, t in enumerate(temperatures):
        if todo.size == 0:
            break
        sd = fallback_seed(seed, k)
        r = decode(todo, float(t), sd)
        steps.append((float(t), sd, todo.copy()))
        need = np.zeros(todo.size, dtype=bool)
        for i, b in enumerate(todo):
            n_text = int(r.n_text[i])
            text_toks = r.tokens[i, :n_text]
            cr = (compression_ratio_text(vocab.decode(text_toks)) if vocab is not None
                  else compression_ratio_tokens(text_toks, vocab_size))
            nf = needs_fallback(cr, r.avg_logprob[i], None if r.no_speech_prob is None else r.no_speech_prob[i],
                                compression_ratio_threshold, logprob_threshold, no_speech_threshold)
            need[i] = nf
            out["tokens"][b] = r.tokens[i]
            out["lens"][b] = r.lens[i]
            out["logprobs"][b] = r.logprobs[i]
            out["sum_logprob"][b] = r.sum_logprob[i]
            out["avg_logprob"][b] = r.avg_logprob[i]
            if r.no_speech_prob is not None:
                out["no_speech_prob"][b] = r.no_speech_prob[i]
            out["compression_ratio"][b] = cr
            out["temperature"][b] = t
            out["seed"][b] = sd
            out["needs_fallback"][b] = nf
        if getattr(r, "alt_tokens", None) is not None:   # alternatives were requested: the kept attempt's, like everything else
            for key in ("alt_tokens", "alt_logprobs", "alt_counts", "entropy"):
                a = getattr(r, key)
                if a is None:
                    continue
                if key not in out:
                    out[key] = np.full((B,) + a.shape[1:], -1 if key == "alt_tokens" else 0, dtype=a.dtype)
                out[key][todo] = a
        todo = todo[need]
    out["steps"] = steps
    return out


def _pack_recordings(recordings):
    """Recordings (1-D sample arrays) back to back in one array of a supported dtype, plus i64 offsets [R + 1].  All
    int16: int16; otherwise int16 recordings become float32 s / 32768 (exact) and the rest float32 or float64."""
    recs = [np.asarray(r).reshape(-1) for r in recordings]
    for r in recs:
        if r.dtype not in _DTYPES:
            raise ValueError("recording dtype must be int16/float32/float64, got %s" % r.dtype)
    if recs and all(r.dtype == np.int16 for r in recs):
        dt = np.dtype(np.int16)
    else:
        dt = np.dtype(np.float64) if any(r.dtype == np.float64 for r in recs) else np.dtype(np.float32)
        recs = [(r.astype(dt) / dt.type(32768.0)) if r.dtype == np.int16 else r.astype(dt, copy=False) for r in recs]
    offs = np.zeros(len(recs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([r.size for r in recs])
    pcm = np.ascontiguousarray(np.concatenate(recs) if recs else np.zeros(0, dt), dtype=dt)
    return pcm, offs


def resample_out_len(n_frames, sample_rate):
    """wm_resample_out_len: the 16 kHz samples of n_frames frames at sample_rate, ceil(n L / M); ValueError for an
    unsupported rate."""
    n = int(load_library().wm_resample_out_len(int(n_frames), int(sample_rate)))
    if n < 0:
        raise ValueError("unsupported sample rate %r (or a negative length)" % (sample_rate,))
    return n


def resample_filter(sample_rate):
    """wm_resample_filter: (h f32 [2K + 1], L, M, K), the filter wm_resample_16k uses for this input rate."""
    lib = load_library()
    L, M, K = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _check(lib, lib.wm_resample_filter(int(sample_rate), None, 0, ctypes.byref(L), ctypes.byref(M), ctypes.byref(K)))
    h = np.empty(2 * K.value + 1, dtype=np.float32)
    _check(lib, lib.wm_resample_filter(int(sample_rate), _ptr(h), h.size, None, None, None))
    return h, L.value, M.value, K.value


def _pack_interleaved(recordings, sample_rates):
    """Recordings ([n] or [n][C] int16 / float32 arrays, C-contiguous frames) back to back in one interleaved array, plus
    element offsets i64 [R + 1], channel counts and rates i32 [R].  All int16: int16; otherwise int16 recordings become
    float32 s / 32768 (exact: what the kernel computes)."""
    recs = [np.asarray(r) for r in recordings]
    if len(sample_rates) != len(recs):
        raise ValueError("sample_rates: one per recording")
    for r in recs:
        if r.dtype not in (np.dtype(np.int16), np.dtype(np.float32)) or r.ndim not in (1, 2):
            raise ValueError("a recording must be an int16 / float32 array [n] or [n][C], got %s %r" % (r.dtype, r.shape))
    ch = np.array([r.shape[1] if r.ndim == 2 else 1 for r in recs], dtype=np.int32)
    if recs and all(r.dtype == np.int16 for r in recs):
        dt = np.dtype(np.int16)
    else:
        dt = np.dtype(np.float32)
        recs = [(r.astype(np.float32) / np.float32(32768.0)) if r.dtype == np.int16 else r for r in recs]
    offs = np.zeros(len(recs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([r.size for r in recs])
    pcm = np.ascontiguousarray(np.concatenate([r.reshape(-1) for r in recs]) if recs else np.zeros(0, dt), dtype=dt)
    return pcm, offs, ch, np.array([int(x) for x in sample_rates], dtype=np.int32)


# ---- multichannel audio: channel matrices, per-channel activity, the speaker of a span -------------
ACTIVITY_HOP = 160            # WM_ACTIVITY_HOP: samples per activity value, one mel frame


def channel_rows(kind, C):
    """A channel matrix f32 [n_rows][C] for Context.resample_16k_mix.  "split": the identity, one signal per channel;
    "mean": one row of float32(1.0 / C); an int c: the one-hot row of channel c."""
    C = int(C)
    if C < 1:
        raise ValueError("channel_rows: C >= 1")
    if isinstance(kind, str):
        if kind == "split":
            return np.eye(C, dtype=np.float32)
        if kind == "mean":
            return np.full((1, C), np.float32(1.0 / C), dtype=np.float32)
        raise ValueError("channel_rows: 'split', 'mean' or a channel index, got %r" % (kind,))
    if isinstance(kind, bool) or not isinstance(kind, (int, np.integer)) or not 0 <= kind < C:
        raise ValueError("channel_rows: 'split', 'mean' or a channel index 0 .. %d, got %r" % (C - 1, kind))
    row = np.zeros((1, C), dtype=np.float32)
    row[0, int(kind)] = 1.0
    return row


def _channel_ratio(ratio):
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)) or not math.isfinite(ratio) or ratio < 1:
        raise ValueError("channel ratio: a finite number >= 1, got %r" % (ratio,))
    return float(ratio)


def speaker_by_channel(act, start, end, ratio=1.1):
    """whisper.cpp's stereo --diarize rule for C channels.  act [C][F]: the channels' activity per 10 ms frame
    (Context.channel_activity); [start, end): seconds.  The frames [floor(start * 100), ceil(end * 100)), cut to [0, F), are
    summed per channel in f64; best = the first maximal channel; returns best when its sum is > 0 and strictly greater than
    ratio times the largest other sum, else None -- also with fewer than 2 channels, an empty span or a NaN sum.  ratio:
    finite and >= 1 (ValueError)."""
    ratio = _channel_ratio(ratio)
    C = len(act)
    if C < 2:
        return None
    F = min(len(a) for a in act)
    a, b = max(int(math.floor(start * 100.0)), 0), min(int(math.ceil(end * 100.0)), F)
    if a >= b:
        return None
    sums = [float(np.sum(np.asarray(ch[a:b], dtype=np.float64))) for ch in act]
    if any(s != s for s in sums):
        return None
    best = int(np.argmax(sums))   # (the first maximum)
    other = max(s for c, s in enumerate(sums) if c != best)
    return best if sums[best] > 0 and sums[best] > ratio * other else None


def _pack_mix(mix, ch):
    """The matrices of resample_16k_mix -- one [n_rows][C_r] per recording -- as (n_rows i32 [R], the rows back to back f32)."""
    if len(mix) != len(ch):
        raise ValueError("mix: one [n_rows][C] matrix per recording")
    mats = [np.asarray(m, dtype=np.float32) for m in mix]
    for r, m in enumerate(mats):
        if m.ndim != 2 or m.shape[1] != int(ch[r]) or not 1 <= m.shape[0] <= 8:
            raise ValueError("mix: recording %d needs [1 .. 8][%d] weights, got %r" % (r, int(ch[r]), m.shape))
        if not np.all(np.isfinite(m)):
            raise ValueError("mix: recording %d: a weight is not finite" % r)
    rows = np.array([m.shape[0] for m in mats], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in mats]) if mats else np.zeros(0, np.float32), dtype=np.float32)
    return rows, flat


def _channel_counts(recordings):
    """channels of every recording of transcribe_long(channels=...): [n] is one channel, [n][C] are C"""
    counts = []
    for r in recordings:
        shape = np.shape(r)
        if len(shape) not in (1, 2) or (len(shape) == 2 and not 1 <= shape[1] <= 8):
            raise ValueError("channels: a recording must be [n] or [n][C] with 1 .. 8 channels, got %r" % (shape,))
        counts.append(int(shape[1]) if len(shape) == 2 else 1)
    return counts


def _per_channel(value, counts, per_recording):
    """a per-recording list repeated per channel, in (recording, channel) order; anything else as it is"""
    if not per_recording:
        return value
    if len(value) != len(counts):
        raise ValueError("channels='split': a per-recording list has one entry per recording (%d), got %d" % (len(counts), len(value)))
    return [value[r] for r, C in enumerate(counts) for _ in range(C)]


def _split_arguments(counts, language, initial_prompt_tokens, clip_timestamps, recording_bias):
    """transcribe_long(channels='split'): the arguments that are lists per recording, repeated per channel"""
    nested = (list, tuple, np.ndarray)
    ip, ct = initial_prompt_tokens, clip_timestamps
    return (_per_channel(language, counts, language is not None and np.ndim(language) != 0),
            _per_channel(ip, counts, ip is not None and len(ip) > 0 and all(isinstance(x, nested) for x in ip)),
            _per_channel(ct, counts, ct is not None and not np.isscalar(ct) and len(ct) > 0
                         and all(isinstance(x, nested + (str,)) for x in ct)),
            _per_channel(recording_bias, counts, recording_bias is not None))


def _split_results(out, counts):
    """transcribe_long(channels='split'): per recording, `channels` -- its channels' results -- and `segments`, copies of all
    their segments with `channel`, ordered by (start, channel)"""
    res, i = [], 0
    for C in counts:
        chans = out[i:i + C]
        i += C
        segs = [dict(sg, channel=c) for c, ch in enumerate(chans) for sg in ch["segments"]]
        segs.sort(key=lambda sg: (sg["start"], sg["channel"]))   # (stable: a channel's own order stays)
        res.append(dict(channels=chans, segments=segs))
    return res


def _diarize_results(ctx, out, recordings, sample_rates, counts, ratio):
    """transcribe_long(channels='diarize'): ONE wm_resample_16k_mix with identity rows, ONE wm_channel_activity over its device
    output, the split signals freed; then `speaker` on every segment and word"""
    d_sig, offs = ctx.resample_16k_mix(recordings, sample_rates, [channel_rows("split", C) for C in counts], device=True)
    try:
        act = ctx.channel_activity(d_sig, offs, device=True)
    finally:
        ctx.dev_free(d_sig)
    i = 0
    for rec, C in zip(out, counts):
        act_r = act[i:i + C]
        i += C
        for sg in rec["segments"]:
            sg["speaker"] = speaker_by_channel(act_r, sg["start"], sg["end"], ratio)
            for w in sg.get("words", ()):
                w["speaker"] = speaker_by_channel(act_r, w["start"], w["end"], ratio)


# ---- long-form transcription: openai-whisper transcribe()'s seek loop ---------------------------------------------------
HOP_SECONDS = 160 / 16000     # one mel frame
INPUT_STRIDE = 2              # mel frames per encoder output frame (N_FRAMES // n_audio_ctx)
TIME_PRECISION = 0.02         # seconds per timestamp token (INPUT_STRIDE * HOP_LENGTH / SAMPLE_RATE)


def should_skip_window(no_speech_prob, avg_logprob, no_speech_threshold=0.6, logprob_threshold=-1.0):
    """openai-whisper's silence skip: no_speech_prob > no_speech_threshold, unless avg_logprob > logprob_threshold."""
    if no_speech_threshold is None or no_speech_prob is None:
        return False
    skip = no_speech_prob > no_speech_threshold
    if logprob_threshold is not None and avg_logprob > logprob_threshold:
        skip = False
    return bool(skip)


def window_segments(tokens, seek, segment_size, timestamp_begin, eot, result, vocab=None, cleanup=True, alternatives=None):
    """openai-whisper transcribe()'s handling of one decoded window (word_timestamps=False): slicing at consecutive
    timestamps, single_timestamp_ending, the seek update and the clearing of instantaneous / text-less segments.
      tokens : the window's generated tokens without the final eot (openai-whisper DecodingResult.tokens);
      seek, segment_size : the window's first frame and frame count;
      result : dict with temperature, avg_logprob, compression_ratio, no_speech_prob (copied into every segment).
    Returns (segments, next_seek).  A segment is text-less when, with a Vocab, its decoded text is blank, and without one
    when it has no token below eot.  cleanup=False (the word-timestamp path, where openai-whisper clears AFTER the word
    step: clear_empty_segments) leaves the segments as sliced and returns (segments, next_seek, single_timestamp_ending).
    alternatives (None: none): (per token of `tokens` its list of (id, logprob), per token its entropy) -- every segment then
    carries the values of its own tokens as token_alternatives and token_entropy."""
    tokens = [int(t) for t in tokens]
    time_offset = float(seek * HOP_SECONDS)
    segment_duration = segment_size * HOP_SECONDS

    def new_segment(start, end, toks, first=0):
        seg = dict(seek=seek, start=start, end=end, tokens=list(toks), temperature=result["temperature"],
                   avg_logprob=result["avg_logprob"], compression_ratio=result["compression_ratio"],
                   no_speech_prob=result["no_speech_prob"])
        if alternatives is not None:
            seg["token_alternatives"] = list(alternatives[0][first:first + len(toks)])
            seg["token_entropy"] = list(alternatives[1][first:first + len(toks)])
        if vocab is not None:
            seg["text"] = vocab.decode([t for t in toks if t < eot])
        return seg

    is_ts = [t >= timestamp_begin for t in tokens]
    single_timestamp_ending = is_ts[-2:] == [False, True]
    consecutive = [i + 1 for i in range(len(tokens) - 1) if is_ts[i] and is_ts[i + 1]]
    segments = []
    if consecutive:
        slices = list(consecutive)
        if single_timestamp_ending:
            slices.append(len(tokens))
        last_slice = 0
        for cur in slices:
            sl = tokens[last_slice:cur]
            segments.append(new_segment(time_offset + (sl[0] - timestamp_begin) * TIME_PRECISION,
                                        time_offset + (sl[-1] - timestamp_begin) * TIME_PRECISION, sl, last_slice))
            last_slice = cur
        if single_timestamp_ending:
            next_seek = seek + segment_size
        else:
            next_seek = seek + (tokens[last_slice - 1] - timestamp_begin) * INPUT_STRIDE
    else:
        duration = segment_duration
        ts = [t for t in tokens if t >= timestamp_begin]
        if ts and ts[-1] != timestamp_begin:
            duration = (ts[-1] - timestamp_begin) * TIME_PRECISION
        segments.append(new_segment(time_offset, time_offset + duration, tokens))
        next_seek = seek + segment_size
    if not cleanup:
        return segments, next_seek, single_timestamp_ending
    clear_empty_segments(segments, eot, vocab)
    return segments, next_seek


def clear_empty_segments(segments, eot, vocab=None, words=False):
    """The last loop of openai-whisper transcribe() over a window's segments: one with start == end or without text loses
    its tokens and text (and, with words=True, its words)."""
    for seg in segments:
        blank = (seg["text"].strip() == "") if vocab is not None else not any(t < eot for t in seg["tokens"])
        if seg["start"] == seg["end"] or blank:
            seg["tokens"] = []
            if "token_alternatives" in seg:
                seg["token_alternatives"], seg["token_entropy"] = [], []
            if vocab is not None:
                seg["text"] = ""
            if words:
                seg["words"] = []


def conditioned_prompt(all_tokens, prompt_reset_since, sot_sequence, sot_prev, n_text_ctx):
    """The prompt of a window under condition_on_previous_text (openai-whisper transcribe(): prompt =
    all_tokens[prompt_reset_since:], and DecodingTask._get_initial_tokens): [sot_prev] + the last n_text_ctx // 2 - 1
    tokens of that history + sot_sequence, or sot_sequence alone while the history is empty."""
    prev = [int(t) for t in all_tokens[prompt_reset_since:]]
    seq = [int(t) for t in sot_sequence]
    if not prev:
        return seq
    return [int(sot_prev)] + prev[-(n_text_ctx // 2 - 1):] + seq


def conditioned_history(all_tokens, prompt_reset_since, segments, temperature, skipped, prompt_reset_on_temperature=0.5):
    """The history after a window (openai-whisper transcribe()): all_tokens grows by the tokens of the window's segments
    (timestamps included; a cleared segment has none), then the prompt restarts behind them when the window's final
    temperature exceeds prompt_reset_on_temperature.  A skipped window changes nothing.  Returns (all_tokens,
    prompt_reset_since); the list passed in is not modified."""
    if skipped:
        return list(all_tokens), prompt_reset_since
    grown = list(all_tokens) + [int(t) for sg in segments for t in sg["tokens"]]
    if temperature > prompt_reset_on_temperature:
        prompt_reset_since = len(grown)
    return grown, prompt_reset_since


def carried_prompt(initial_prompt, all_tokens, prompt_reset_since, sot_sequence, sot_prev, n_text_ctx):
    """The prompt of a window under condition_on_previous_text with carry_initial_prompt, for a recording with a non-empty
    initial prompt `ip` (all_tokens starts with it): [sot_prev] + ip + the last cap - len(ip) tokens of
    all_tokens[max(len(ip), prompt_reset_since):] + sot_sequence, cap = n_text_ctx // 2 - 1.  This project's rule for
    len(ip) >= cap, where openai-whisper's slice takes a non-positive count: ip[-cap:] and no history."""
    ip = [int(t) for t in initial_prompt]
    cap = n_text_ctx // 2 - 1
    if len(ip) >= cap:
        text = ip[-cap:]
    else:
        text = ip + [int(t) for t in all_tokens[max(len(ip), prompt_reset_since):]][-(cap - len(ip)):]
    return [int(sot_prev)] + text + [int(t) for t in sot_sequence]


def clip_times(clip_timestamps, R):
    """transcribe_long's clip_timestamps as one list of seconds per recording: None, a string of comma-separated seconds
    ("" = none), a flat list or one number (for every recording) or a list of R lists / strings.  Times must be finite,
    >= 0 and non-decreasing (ValueError)."""
    def one(x):
        if isinstance(x, str):
            x = [float(s) for s in x.split(",")] if x.strip() else []
        elif np.isscalar(x):
            x = [x]
        t = [float(v) for v in x]
        if any(not math.isfinite(v) or v < 0 for v in t) or any(b < a for a, b in zip(t, t[1:])):
            raise ValueError("clip_timestamps: finite seconds >= 0 in non-decreasing order")
        return t
    if clip_timestamps is None:
        return [[] for _ in range(R)]
    if (not np.isscalar(clip_timestamps) and len(clip_timestamps) > 0
            and all(isinstance(x, (list, tuple, np.ndarray, str)) for x in clip_timestamps)):
        if len(clip_timestamps) != R:
            raise ValueError("clip_timestamps: one list per recording")
        return [one(x) for x in clip_timestamps]
    t = one(clip_timestamps)
    return [list(t) for _ in range(R)]


def seek_clips(times, content):
    """The clips of one recording of `content` frames from clip_times' seconds, as openai-whisper transcribe() pairs them:
    seek points round(t * 100), `content` appended to an odd count, no time = the one clip [0, content).  This project's
    rules on top: a clip is cut to [0, content) and one that is empty after the cut is dropped.  Returns
    [(first frame, end frame, index of the pair)]."""
    p = [int(round(t * 100)) for t in times]
    if not p:
        p = [0]
    if len(p) % 2:
        p.append(content)
    clips = []
    for k in range(0, len(p), 2):
        a, b = min(p[k], content), min(p[k + 1], content)
        if a < b:
            clips.append((a, b, k // 2))
    return clips


class wm_vad_params(ctypes.Structure):
    _fields_ = [("q_floor", ctypes.c_float), ("q_peak", ctypes.c_float), ("min_range", ctypes.c_float),
                ("on_frac", ctypes.c_float), ("off_frac", ctypes.c_float), ("min_speech", ctypes.c_int32),
                ("min_silence", ctypes.c_int32), ("speech_pad", ctypes.c_int32)]


VAD_SMOOTH = 5             # frames of the moving average transcribe_long(vad=True) asks wm_vad_energy for
MAX_DRAFT_LEN = 7          # WM_MAX_DRAFT_LEN: proposals per round of a speculative call (Context.transcribe_mel_speculative)
MAX_TEACHER_PANEL = 8      # WM_MAX_TEACHER_PANEL: positions per decoder step of a teacher-forced pass (Context.set_teacher_panel)
PARALLEL_CLIPS_TRUE = 56   # parallel_clips=True: the decode-group size of the bench headline


def vad_default_params():
    """wm_vad_default_params as a dict.  Not validated on real speech (include/whisper_mi355x.h)."""
    p = wm_vad_params()
    load_library().wm_vad_default_params(ctypes.byref(p))
    return {k: getattr(p, k) for k, _ in wm_vad_params._fields_}


def vad_segments(y, params=None, stats=False):
    """wm_vad_segments: the speech spans [(start, end)] in frames of one recording's energy track y (f32 [n],
    Context.vad_energy).  params: None (the defaults) or a dict of overrides of wm_vad_params' fields.  stats=True:
    (spans, (floor, peak, thr_on, thr_off))."""
    lib = load_library()
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
    p = wm_vad_params()
    lib.wm_vad_default_params(ctypes.byref(p))
    for k, v in (params or {}).items():
        if k not in dict(wm_vad_params._fields_):
            raise ValueError("vad params: no field %r" % (k,))
        setattr(p, k, v)
    n = ctypes.c_int(0)
    st = np.empty(4, dtype=np.float32)
    _check(lib, lib.wm_vad_segments(_ptr(y), y.size, ctypes.byref(p), None, 0, ctypes.byref(n), None))
    seg = np.empty((max(n.value, 1), 2), dtype=np.int32)
    _check(lib, lib.wm_vad_segments(_ptr(y), y.size, ctypes.byref(p), _ptr(seg), n.value, ctypes.byref(n), _ptr(st)))
    spans = [(int(a), int(b)) for a, b in seg[:n.value]]
    return (spans, tuple(float(v) for v in st)) if stats else spans


def _slaney_mel_to_hz(m):
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return min_log_hz * math.exp(logstep * (m - min_log_mel)) if m >= min_log_mel else f_sp * m


def vad_band(n_mels, f_lo=100.0, f_hi=4000.0):
    """(band_lo, band_hi): the mel bins whose centre frequency -- Slaney scale, 0 .. 8000 Hz, the filterbank of the front
    end -- lies in [f_lo, f_hi].  ValueError when there is none."""
    top = 15.0 + math.log(8000.0 / 1000.0) / (math.log(6.4) / 27.0)   # 8000 Hz in mels
    centres = [_slaney_mel_to_hz(top * (m + 1) / (n_mels + 1)) for m in range(n_mels)]
    inside = [m for m, f in enumerate(centres) if f_lo <= f <= f_hi]
    if not inside:
        raise ValueError("vad_band: no mel bin between %g and %g Hz" % (f_lo, f_hi))
    return inside[0], inside[-1] + 1


def vad_clips(segments, max_frames=N_FRAMES):
    """Speech spans -> the clips transcribe_long decodes, greedy in time: a clip grows over the next span, the silence
    between included, while span end - clip start <= max_frames.  A single span longer than max_frames stays one clip
    (the seek loop walks it).  Returns [(start, end)]."""
    clips = []
    for a, b in segments:
        if clips and b - clips[-1][0] <= max_frames:
            clips[-1][1] = int(b)
        else:
            clips.append([int(a), int(b)])
    return [(a, b) for a, b in clips]


HALLUCINATION_PUNCTUATION = "\"'“¿([{-\"'.。,，!！?？:：”)]}、"   # PREPEND_PUNCTUATIONS + APPEND_PUNCTUATIONS


def word_anomaly_score(word):
    """openai-whisper transcribe()'s word_anomaly_score: 1 for a probability below 0.15, 15 per second short of 0.133 s, and
    the seconds beyond 2 s."""
    d = word["end"] - word["start"]
    score = 0.0
    if word["probability"] < 0.15:
        score += 1.0
    if d < 0.133:
        score += (0.133 - d) * 15
    if d > 2.0:
        score += d - 2.0
    return score


def is_segment_anomaly(segment):
    """openai-whisper transcribe()'s is_segment_anomaly: over the first 8 words that are no substring of
    HALLUCINATION_PUNCTUATION, a score sum of 3 or more, or of the word count less 0.01 or more; False for no segment and
    for one without words."""
    if segment is None or not segment["words"]:
        return False
    words = [w for w in segment["words"] if w["word"] not in HALLUCINATION_PUNCTUATION][:8]
    score = sum(word_anomaly_score(w) for w in words)
    return score >= 3 or score + 0.01 >= len(words)


def hallucination_silence_skip(segments, seek, segment_size, content, threshold, single_timestamp_ending,
                               last_speech_timestamp, next_seek):
    """openai-whisper transcribe()'s hallucination_silence_threshold rules for ONE window, after the word step and before
    the clearing of empty segments.  segments: the window's, with `words`; last_speech_timestamp: the recording's BEFORE
    this window; next_seek: what the window's timestamps gave (window_segments).  Returns (next seek, segments kept, tag):
      the last word's end e behind the window's start, no single timestamp ending: seek to e when more than `threshold`
        of the 30 s window lies behind it, else past the window's frames;
      "leading": the first segment with words is anomalous and starts more than `threshold` into the window -- the seek
        moves by that gap and NO segment is kept;
      "surrounded": an anomalous segment with silence (or the window's edge, or an anomalous neighbour) on both sides --
        the seek goes to its start (at least 1 s on, or to `content` when less than `threshold` of the recording is left
        behind it) and it and the later segments are dropped;
      None otherwise."""
    t0 = seek * HOP_SECONDS
    wend = (seek + N_FRAMES) * HOP_SECONDS
    with_words = [sg for sg in segments if sg["words"]]
    if not single_timestamp_ending and with_words and with_words[-1]["words"][-1]["end"] > t0:
        e = with_words[-1]["words"][-1]["end"]
        next_seek = int(round(e * 100)) if wend - e > threshold else seek + segment_size
    if with_words and is_segment_anomaly(with_words[0]):
        gap = with_words[0]["start"] - t0
        if gap > threshold:
            return seek + int(round(gap * 100)), [], "leading"
    hal_last = last_speech_timestamp
    for si, g in enumerate(segments):
        if not g["words"]:
            continue
        if is_segment_anomaly(g):
            nxt = next((sg for sg in segments[si + 1:] if sg["words"]), None)
            next_start = nxt["words"][0]["start"] if nxt is not None else t0 + segment_size * HOP_SECONDS
            before = g["start"] - hal_last > threshold or g["start"] < threshold or g["start"] - t0 < 2.0
            after = next_start - g["end"] > threshold or is_segment_anomaly(nxt) or wend - g["end"] < 2.0
            if before and after:
                next_seek = int(round(max(t0 + 1, g["start"]) * 100))
                if content * HOP_SECONDS - g["end"] < threshold:
                    next_seek = content
                return next_seek, segments[:si], "surrounded"
        hal_last = g["end"]
    return next_seek, segments, None


# ---- the parts of transcribe_long: options, units, the rows of a round, and the language / clip / word steps ---------------
class _LongOptions(types.SimpleNamespace):
    """transcribe_long's arguments under their names, plus what its checks derive from them.  The checks raise in the order
    they always had: early() before any library call and prompt_head() behind the language step; between them the log-mel
    and the language step check their own arguments (sample_rates; language, lang_first, lang_last)."""

    def early(self, R):
        beam_max_candidates(self.beam_size, self.patience)
        self.alt_kw = {}   # 24.
        if alternatives_arg(self.alternatives, self.beam_size if self.beam_size is not None else self.patience, self.draft) is not None:
            self.alt_kw = dict(alternatives=int(self.alternatives))
        self.rec_ids = list(range(R)) if self.recording_ids is None else [int(i) for i in self.recording_ids]
        if len(self.rec_ids) != R or any(i < 0 or i >= 65536 for i in self.rec_ids):
            raise ValueError("recording_ids: one per recording, each 0 .. 65535")
        self.n_ctx = int(self.ctx.dims["n_text_ctx"])
        self.n_mels = int(self.ctx.dims["n_mels"])
        self.max_new = self.n_ctx // 2
        self.cond = bool(self.condition_on_previous_text)
        if self.cond:
            if self.sot_prev is None:
                raise ValueError("condition_on_previous_text needs sot_prev")
            self.max_new = min(self.n_ctx // 2, self.n_ctx - (self.n_ctx // 2 + 3))
        ip = self.initial_prompt_tokens
        self.per_rec = ip is not None and len(ip) > 0 and all(isinstance(x, (list, tuple, np.ndarray)) for x in ip)
        if self.per_rec and len(ip) != R:
            raise ValueError("initial_prompt_tokens: one list per recording")
        if self.vocab_size is None:
            self.vocab_size = int(self.ctx.dims["n_vocab"])
        if isinstance(self.word_timestamps, str) and self.word_timestamps not in ("decode", "decode_best"):
            raise ValueError("word_timestamps: False, True, 'decode' or 'decode_best'")
        self.words_on = bool(self.word_timestamps)
        self.words_decode = isinstance(self.word_timestamps, str)   # 18.: the alignment comes with the decode
        self.words_best = self.word_timestamps == "decode_best"     # 19.: ... of best_of candidates and beams too
        if self.words_decode and not self.words_best and (self.best_of is not None or self.beam_size is not None):
            raise ValueError("word_timestamps='decode' cannot be combined with best_of or beam_size: that is 'decode_best'")
        if self.words_on and (self.vocab is None or (self.no_timestamps is None and not self.words_decode)):
            raise ValueError("word_timestamps needs vocab and no_timestamps")
        self.clips_on = self.clip_timestamps is not None
        self.times = clip_times(self.clip_timestamps, R)
        self.vad_on = self.vad is not None and self.vad is not False
        if self.vad_on and self.clips_on:
            raise ValueError("vad makes the clips: it cannot be combined with clip_timestamps")
        self.vad_kw = dict(self.vad) if isinstance(self.vad, dict) else {}
        if self.vad_on and set(self.vad_kw) - {"band", "smooth", "params", "max_frames"}:
            raise ValueError("vad: the overrides are band, smooth, params and max_frames")
        self.par = self.parallel_clips is not None
        self.par_n = None   # lanes per round (None: every live unit)
        if self.par:
            self.par_n = PARALLEL_CLIPS_TRUE if self.parallel_clips is True else int(self.parallel_clips)
            if self.parallel_clips is False or self.par_n < 1:
                raise ValueError("parallel_clips: None, True or a lane count >= 1")
            if self.cond:
                raise ValueError("parallel_clips cannot be combined with condition_on_previous_text: the history is serial")
            if self.hallucination_silence_threshold is not None:
                raise ValueError("parallel_clips cannot be combined with hallucination_silence_threshold")
        self.thr = self.hallucination_silence_threshold
        if self.thr is not None:
            self.thr = float(self.thr)
            if not math.isfinite(self.thr) or self.thr < 0:
                raise ValueError("hallucination_silence_threshold: finite seconds >= 0")
            if not self.words_on:
                raise ValueError("hallucination_silence_threshold needs word_timestamps")
        if self.teacher_panel is not None:
            if isinstance(self.teacher_panel, bool) or int(self.teacher_panel) != self.teacher_panel or not 1 <= self.teacher_panel <= MAX_TEACHER_PANEL:
                raise ValueError("teacher_panel: None or a width 1 .. %d" % MAX_TEACHER_PANEL)
        if self.prompt_panel is not None:   # 21.
            if isinstance(self.prompt_panel, bool) or not isinstance(self.prompt_panel, (int, np.integer)) or not 1 <= self.prompt_panel <= MAX_TEACHER_PANEL:
                raise ValueError("prompt_panel: None or a width 1 .. %d" % MAX_TEACHER_PANEL)
        self.prompt_panel_pending = self.prompt_panel is not None   # set on the context in front of the first decode call
        if self.draft is None:
            if self.draft_len is not None:
                raise ValueError("draft_len needs draft")
        else:   # 20.
            self.draft_len = 4 if self.draft_len is None else self.draft_len
            if isinstance(self.draft_len, bool) or int(self.draft_len) != self.draft_len or not 1 <= self.draft_len <= MAX_DRAFT_LEN:
                raise ValueError("draft_len: 1 .. %d" % MAX_DRAFT_LEN)
            for on, what in ((self.cond, "condition_on_previous_text"), (self.best_of is not None, "best_of"),
                             (self.beam_size is not None, "beam_size"), (self.words_decode, "word_timestamps='decode*'"),
                             (bool(self.reuse_encoder), "reuse_encoder"),
                             (self.repetition_penalty is not None or self.no_repeat_ngram_size is not None, "the repetition rules"),
                             (bool(self.sequence_bias) or bool(self.bad_words) or bool(self.boost_phrases), "a sequence bias")):
                if on:
                    raise ValueError("draft (speculative decoding) cannot be combined with %s" % what)
        if self.fallback not in ("lockstep", "deferred"):   # 26.
            raise ValueError("fallback: 'lockstep' or 'deferred'")
        self.deferred = self.fallback == "deferred"
        if self.deferred:
            for on, what in ((self.best_of is not None, "best_of"), (self.beam_size is not None or self.patience is not None, "beam_size"),
                             (self.draft is not None, "draft"), (bool(self.reuse_encoder), "reuse_encoder")):
                if on:
                    raise ValueError("fallback='deferred' cannot be combined with %s" % what)
            if len(self.temperatures) == 0:
                raise ValueError("fallback='deferred' needs at least one temperature")
        self.panel_pending = self.teacher_panel is not None   # set on the context in front of the first alignment call
        if self.prepend_punctuations is None:
            self.prepend_punctuations = PREPEND_PUNCTUATIONS
        if self.append_punctuations is None:
            self.append_punctuations = APPEND_PUNCTUATIONS

    def prompt_head(self):
        """How the rows carry their prompts: head, the tokens in front of [sot, language, task] in a table of one length, or
        ragged -- lists whose lengths may differ --, and sot_kw, which tells a decode call where <|startoftranscript|> is."""
        self.head = []
        if self.initial_prompt_tokens is not None:
            if self.sot_prev is None:
                raise ValueError("initial_prompt_tokens need sot_prev")
            if not self.per_rec:
                self.head = [int(self.sot_prev)] + [int(t) for t in self.initial_prompt_tokens][-(self.n_ctx // 2 - 1):]
        self.ragged = self.cond or self.per_rec
        self.sot_kw = dict(sot_tail=3) if self.ragged else dict(sot_index=len(self.head))


class _Unit:
    """What transcribe_long's rounds advance: a recording with its clip list or, with parallel_clips (lane=True), ONE of its
    clips.  rec .. seed_tokens (the initial prompt) are the recording's; the history (all_tokens, reset_since), the clip
    cursor, the seek, `before` -- (cursor, seek) of the previous window --, last_speech and the result lists its own."""
    __slots__ = ("index", "rec", "rec_id", "mel_off", "T", "content", "lang", "seed_tokens", "carry", "all_tokens",
                 "reset_since", "clips", "cur", "seek", "before", "last_speech", "lane", "segments", "seeks", "windows",
                 "attempt", "tried", "size")

    def __init__(self, index, rec, rec_id, mel_off, T, lang, seed_tokens, carry, clips, lane):
        self.index, self.rec, self.rec_id, self.mel_off, self.T, self.lang = index, rec, rec_id, mel_off, T, lang
        self.content = int(T) - N_FRAMES
        self.seed_tokens, self.carry, self.clips, self.lane = seed_tokens, carry, clips, lane
        self.all_tokens, self.reset_since = list(seed_tokens), 0
        self.cur, self.seek, self.before = 0, clips[0][0] if clips else 0, None
        self.last_speech = clips[0][0] * HOP_SECONDS if lane else 0.0
        self.segments, self.seeks, self.windows = [], [], []
        # fallback="deferred": the open window's next attempt (0: no window is held open), the temperatures it has run, its frames
        self.attempt, self.tried, self.size = 0, [], 0

    def advance(self):
        """the clip cursor before a round: a seek at or past its clip's end moves to the next clip's start; False: none left"""
        while self.cur < len(self.clips) and self.seek >= self.clips[self.cur][1]:
            self.cur += 1
            if self.cur < len(self.clips):
                self.seek = self.clips[self.cur][0]
        if self.cur == len(self.clips):
            return False
        self.seek = max(self.seek, self.clips[self.cur][0])
        return True

    def open_window(self):
        """the frames of the window at the seek, which has grown since the unit's previous window within this clip"""
        if self.before is not None and self.before[0] == self.cur and self.seek <= self.before[1]:
            raise AssertionError("transcribe_long: recording %d stays at seek %d" % (self.index, self.seek))
        self.before = (self.cur, self.seek)
        return min(N_FRAMES, self.content - self.seek, self.clips[self.cur][1] - self.seek)

    def sample_id(self):
        """(window ordinal << 16) | recording id; a lane counts (clip, window within the clip): its noise is its own"""
        n = len(self.windows)
        if self.lane:
            n = (self.clips[0][2] << 4) | min(n, 15)
        return ((n & 0xFFFF) << 16) | self.rec_id

    def prompt(self, o):
        seq = [int(o.sot), self.lang, int(o.task)]
        if not o.ragged:
            return o.head + seq
        if self.carry:
            return carried_prompt(self.seed_tokens, self.all_tokens, self.reset_since, seq, o.sot_prev, o.n_ctx)
        return conditioned_prompt(self.all_tokens, self.reset_since if o.cond else 0, seq, o.sot_prev, o.n_ctx)

    def record_window(self, o, size, prompt, temperatures, skipped, tokens, n_round, kept_by):
        self.seeks.append(self.seek)
        w = dict(seek=self.seek, segment_size=size, temperatures=temperatures, skipped=skipped,
                 tokens=[int(t) for t in tokens], prompt_len=len(prompt), prompt=[int(t) for t in prompt])
        if o.clips_on or o.vad_on or o.par:
            w["clip"] = self.clips[self.cur][2]
        if o.par:
            w["round"] = n_round
        w.update(kept_by)
        self.windows.append(w)

    def commit(self, o, segments, next_seek, temperature):
        """a kept window: the seek, the history of a conditioned run, and the segments"""
        self.seek = next_seek
        if o.cond:
            self.all_tokens, self.reset_since = conditioned_history(self.all_tokens, self.reset_since, segments, temperature,
                                                                    False, o.prompt_reset_on_temperature)
        self.segments += segments

    def deliver(self, out):
        """the unit's lists behind those its recording has already (lanes arrive in clip order); the segments get their ids"""
        for sg in self.segments:
            sg["id"] = len(out["segments"])
            out["segments"].append(sg)
        out["seeks"] += self.seeks
        out["windows"] += self.windows


class _RoundRows:
    """The rows of a round: row i is window [seek, seek + sizes[i]) of units[i], read from the recordings' log-mel on the
    device or, with reuse_encoder, from the Windows set those windows are encoded into ONCE here (close() frees it).
    decode is fallback_decode's `decode` with the step rule of fallback_step_extra; kept_by[row]: `candidate` (with best_of)
    and `hypothesis` (with beam_size), the index the row's last step kept -- 0 after a step of the other kind."""

    def __init__(self, o, d_mel, units, sizes, prompts, sample_ids):
        self.o, self.d_mel, self.units, self.sizes, self.ids = o, d_mel, units, sizes, sample_ids
        self.prompts = prompts if o.ragged else np.array(prompts, dtype=np.int32)
        self.kept_by = [{} for _ in units]
        self.aligned = [None] * len(units)   # word_timestamps="decode": (start_frames, logprobs, lens) of the row's last step
        self.set = o.ctx.encode_windows(*self._mel_windows(range(len(units))), mem=WM_MEM_DEVICE) if o.reuse_encoder else None

    def _mel_windows(self, rows):
        """(a unit's seek is still the window's while the round's calls run)"""
        us = [self.units[i] for i in rows]
        return (self.d_mel, np.array([u.mel_off for u in us]), np.array([u.T for u in us]), [u.seek for u in us],
                [self.sizes[i] for i in rows])

    def decode(self, todo, t, sd, rows=None):
        """rows (fallback="deferred"): (temperatures, seeds) of the ROUND's rows -- the call carries its rows' own"""
        o = self.o
        extra = fallback_step_extra(t, o.best_of, o.length_penalty, o.beam_size, o.patience)
        prompts = [self.prompts[i] for i in todo] if o.ragged else self.prompts[todo]
        if o.rec_tables is not None:   # 22.: the tables of exactly this call's rows (a clip: its recording's)
            o.ctx.set_bias_rows([o.rec_tables[self.units[i].rec] for i in todo])
        kw = dict(eot=o.eot, temperature=t, seed=sd, no_speech_token=o.no_speech_token, sample_ids=[self.ids[i] for i in todo],
                  **o.sot_kw, **extra, **o.alt_kw)
        if rows is not None:   # 26.
            kw.update(row_temperatures=[rows[0][i] for i in todo], row_seeds=[rows[1][i] for i in todo])
        if o.words_decode:   # 18.: every attempt through the aligned entry; the kept one's start frames feed the word step
            r = self._decode_aligned(todo, prompts, kw, extra)
            for k, i in enumerate(todo):
                self.aligned[i] = (r.start_frames[k], r.logprobs[k], int(r.lens[k]), r.tokens[k])
        elif o.draft is not None and t == 0 and not o.ragged:   # 20.: the same tokens, proposed by the draft
            r = o.ctx.transcribe_mel_speculative(o.draft, *self._mel_windows(todo), prompts, o.max_new, o.draft_len, eot=o.eot,
                                                 no_speech_token=o.no_speech_token, mem=WM_MEM_DEVICE, **o.sot_kw)
        elif self.set is not None:   # the same call without the encoder pass
            r = o.ctx.transcribe_windows(self.set, [int(i) for i in todo], prompts, o.max_new, **kw)
        else:
            r = o.ctx.transcribe_mel(*self._mel_windows(todo), prompts, o.max_new, mem=WM_MEM_DEVICE, **kw)
        for k, i in enumerate(todo):
            if o.best_of is not None:
                self.kept_by[i]["candidate"] = int(r.candidate[k]) if "best_of" in extra else 0
            if o.beam_size is not None:
                self.kept_by[i]["hypothesis"] = int(r.hypothesis[k]) if "beam_size" in extra else 0
        return r

    def _decode_aligned(self, todo, prompts, kw, extra):
        """The aligned entry of a fallback step: the plain one or, 19., the beam / best-of one the step's `extra` asks for
        (fallback_step_extra) -- then the TranscribeResult of the hypotheses it chose, with their start_frames."""
        o = self.o
        if self.set is not None:
            rows, tail, kind = (self.set, [int(i) for i in todo], prompts, o.max_new), {}, "windows"
        else:
            rows, tail, kind = (*self._mel_windows(todo), prompts, o.max_new), dict(mem=WM_MEM_DEVICE), "mel"
        if not extra:
            return getattr(o.ctx, "transcribe_%s_aligned" % kind)(*rows, **tail, **kw)
        if "beam_size" in extra:   # beam search decodes at temperature 0: no seed, no sample ids
            kw = {k: v for k, v in kw.items() if k not in ("temperature", "seed", "sample_ids", "beam_size")}
            res = getattr(o.ctx, "transcribe_%s_beam_aligned" % kind)(*rows, extra["beam_size"], **tail, **kw)
            res.selected.hypothesis = res.best
        else:
            kw = {k: v for k, v in kw.items() if k != "best_of"}
            res = getattr(o.ctx, "transcribe_%s_best_of_aligned" % kind)(*rows, extra["best_of"], **tail, **kw)
            res.selected.candidate = res.best
        r = res.selected   # (with alternatives: the chosen candidate's)
        r.start_frames = res.start_frames
        return r

    def align(self, rows, texts, sot_seqs):
        o = self.o
        if o.words_decode:   # no call: the kept attempts' own start frames, cut to the text the segments kept
            out = [decode_alignment_text(self.aligned[i][3], self.aligned[i][2], self.aligned[i][0], self.aligned[i][1], o.eot,
                                         n_text=len(t)) for i, t in zip(rows, texts)]
            for (toks, _, _), t in zip(out, texts):
                if toks != [int(x) for x in t]:
                    raise AssertionError("transcribe_long: a window's segments do not hold a prefix of its text tokens")
            return [sf for _, sf, _ in out], [pr for _, _, pr in out]
        if self.set is not None:
            return o.ctx.align_windows(self.set, rows, texts, sot_seqs, o.no_timestamps, o.eot, medfilt_width=7, qk_scale=1.0)
        return o.ctx.align_mel(*self._mel_windows(rows), texts, sot_seqs, o.no_timestamps, o.eot, medfilt_width=7, qk_scale=1.0,
                               mem=WM_MEM_DEVICE)

    def close(self):
        if self.set is not None:
            self.set.close()


def _long_mel(o, R):
    """1. the log-mel of all recordings on the device: (pointer, element offsets, T)"""
    ctx = o.ctx
    if o.sample_rates is None:
        return ctx.logmel_long(o.recordings, n_mels=o.n_mels, device=True)
    if o.split:   # 27.: the identity matrix of every recording -- one signal per channel, R of them
        d_pcm, pcm_offs = ctx.resample_16k_mix(o.recordings, o.sample_rates, [channel_rows("split", C) for C in o.counts], device=True)
    else:
        if len(o.sample_rates) != R:
            raise ValueError("sample_rates: one per recording")
        d_pcm, pcm_offs = ctx.resample_16k(o.recordings, o.sample_rates, device=True)
    try:
        return ctx.logmel_long_device(d_pcm, np.float32, pcm_offs, n_mels=o.n_mels)
    finally:
        ctx.dev_free(d_pcm)


def _long_languages(o, d_mel, mel_offs, T):
    """2. one language token per recording: as given, or detected on frames [0, 3000) of every recording"""
    ctx, R = o.ctx, len(T)
    if o.language is not None:
        langs = [int(o.language)] * R if np.ndim(o.language) == 0 else [int(x) for x in o.language]
        if len(langs) != R:
            raise ValueError("language: one token id per recording")
        return langs
    if o.lang_first is None or o.lang_last is None:
        raise ValueError("language detection needs lang_first / lang_last")
    if o.reuse_encoder:
        with ctx.encode_windows(d_mel, mel_offs[:R], T, 0, N_FRAMES, mem=WM_MEM_DEVICE) as lid_set:
            idx = np.concatenate([ctx.windows_detect_language(lid_set, np.arange(a, min(a + 128, R)), o.sot, o.lang_first,
                                                              o.lang_last)[0] for a in range(0, R, 128)])
    else:
        win = np.empty((R, o.n_mels, N_FRAMES), dtype=np.float32)
        for r in range(R):
            for c in range(o.n_mels):
                src = ctypes.c_void_p(d_mel.value + 4 * (int(mel_offs[r]) + c * int(T[r])))
                win[r, c] = ctx.download(src, N_FRAMES, np.float32)
        idx, _ = ctx.detect_language_probs(ctx.encode_mel(win), o.sot, o.lang_first, o.lang_last)
    return [int(o.lang_first + i) for i in idx]


def _long_units(o, out, langs, d_mel, mel_offs, T):
    """One unit per recording holding its clips [(first frame, end frame, number)] -- of clip_timestamps (10.) or, with vad,
    from the audio (13.) -- or, with parallel_clips (14.), one unit per clip, in (recording, clip) order."""
    R, ip = len(T), o.initial_prompt_tokens
    content = [int(t) - N_FRAMES for t in T]
    clips = [seek_clips(o.times[r], content[r]) for r in range(R)]
    if o.vad_on:
        kw = o.vad_kw
        ys = o.ctx.vad_energy(d_mel, mel_offs[:R], T, content, kw.get("band") or vad_band(o.n_mels),
                              kw.get("smooth", VAD_SMOOTH), device=True)
        for r in range(R):
            out[r]["vad_segments"] = vad_segments(ys[r], kw.get("params"))
            out[r]["vad_clips"] = vad_clips(out[r]["vad_segments"], kw.get("max_frames", N_FRAMES))
            clips[r] = [(a, b, k) for k, (a, b) in enumerate(out[r]["vad_clips"])]
    units = []
    for r, cl in enumerate(clips):
        out[r]["language"] = langs[r]
        seed = [int(t) for t in (ip[r] if o.per_rec else ip if ip is not None else [])]
        carry = bool(o.carry_initial_prompt) and o.cond and len(seed) > 0
        for own in ([[c] for c in cl] if o.par else [cl]):
            units.append(_Unit(len(units), r, o.rec_ids[r], mel_offs[r], T[r], langs[r], seed, carry, own, o.par))
    return units


def _long_word_step(o, source, live, sizes, kept, res):
    """6. the word step of a round: ONE alignment call over the kept windows that have a text token and at least 2 frames,
    then per window the word rules, the word-driven seek (or 11.), the clearing of empty segments and the commit.
    kept: (row of the round, segments, next seek, single_timestamp_ending) of every kept window."""
    eot = o.eot
    texts = [[t for sg in k[1] for t in sg["tokens"] if t < eot] for k in kept]
    go = [n for n, k in enumerate(kept) if texts[n] and sizes[k[0]] >= 2]
    if go:
        rows = [kept[n][0] for n in go]
        sf, pr = source.align(rows, [texts[n] for n in go], [[int(o.sot), live[i].lang, int(o.task)] for i in rows])
    for n, (i, segs, next_seek, single_ending) in enumerate(kept):
        u = live[i]
        if n in go:
            g = go.index(n)
            code = u.lang - int(o.sot) - 1
            code = Whisper.LANGUAGES[code] if 0 <= code < len(Whisper.LANGUAGES) else None
            window_word_timestamps(o.vocab, segs, sf[g], pr[g], u.seek, eot, u.last_speech, code, o.prepend_punctuations,
                                   o.append_punctuations)
        else:
            for sg in segs:
                sg["words"] = []
        if o.thr is None:
            ends = [sg["words"][-1]["end"] for sg in segs if sg["words"]]
            if ends and not single_ending and ends[-1] > u.seek * HOP_SECONDS:
                next_seek = int(round(ends[-1] * 100))
        else:   # 11. (u.last_speech is still the value before this window; the window is the unit's last record)
            n_segs = len(segs)
            next_seek, segs, tag = hallucination_silence_skip(segs, u.seek, sizes[i], u.content, o.thr, single_ending,
                                                              u.last_speech, next_seek)
            if tag is not None:
                u.windows[-1]["hallucination"] = tag
            if tag == "surrounded":
                u.windows[-1]["dropped_segments"] = n_segs - len(segs)
            if tag == "leading":
                u.seek = next_seek
                continue
        ends = [sg["words"][-1]["end"] for sg in segs if sg["words"]]
        if ends:
            u.last_speech = ends[-1]
        clear_empty_segments(segs, eot, o.vocab, words=True)
        u.commit(o, segs, next_seek, float(res["temperature"][i]))


def long_bias_table(sequence_bias, bad_words, boost_phrases, phrase_boost):
    """transcribe_long's sequence_bias / bad_words / boost_phrases as ONE table for Context.set_sequence_bias: ({token tuple:
    bias} in the order sequence_bias, bad_words, boost_phrases; the tuples whose prefixes are boosted), or None when all three
    are None.  ValueError for a sequence named twice and for boost_phrases without a finite phrase_boost."""
    if sequence_bias is None and bad_words is None and boost_phrases is None:
        return None
    table, boost = {}, []

    def add(seq, bias):
        key = tuple(int(t) for t in seq)
        if key in table:
            raise ValueError("sequence bias: %r is named twice" % (key,))
        table[key] = float(bias)
        return key
    for seq, bias in (sequence_bias or {}).items():
        add(seq, bias)
    for seq in bad_words or ():
        add(seq, -math.inf)
    if boost_phrases:
        if phrase_boost is None or not math.isfinite(float(phrase_boost)):
            raise ValueError("boost_phrases needs a finite phrase_boost")
        for seq in boost_phrases:
            boost.append(add(seq, phrase_boost))
    return table, boost


def long_recording_tables(recording_bias, R):
    """transcribe_long's recording_bias as the tables of Context.set_sequence_bias_tables: (tables [{token tuple: bias}], boosts
    [[token tuple]], table_of_recording [R] with -1 for None).  An entry is None or a dict with any of sequence_bias, bad_words,
    boost_phrases, phrase_boost, turned into a table by long_bias_table (an entry whose three lists are all None reads as None);
    equal tables -- the same entries in the same order with the same boosted keys -- are stored once."""
    entries = list(recording_bias)
    if len(entries) != R:
        raise ValueError("recording_bias: one entry per recording")
    tables, boosts, of, seen = [], [], [], {}
    for e in entries:
        if e is None:
            of.append(-1)
            continue
        if not isinstance(e, dict) or set(e) - {"sequence_bias", "bad_words", "boost_phrases", "phrase_boost"}:
            raise ValueError("recording_bias: an entry is None or a dict of sequence_bias, bad_words, boost_phrases, phrase_boost")
        t = long_bias_table(e.get("sequence_bias"), e.get("bad_words"), e.get("boost_phrases"), e.get("phrase_boost"))
        if t is None:
            of.append(-1)
            continue
        key = (tuple(t[0].items()), tuple(t[1]))
        if key not in seen:
            seen[key] = len(tables)
            tables.append(t[0])
            boosts.append(t[1])
        of.append(seen[key])
    return tables, boosts, of


def transcribe_long(ctx, recordings, *, sot, task, eot, timestamp_begin, no_speech_token, lang_first=None,
                    lang_last=None, language=None, sot_prev=None, initial_prompt_tokens=None, recording_ids=None,
                    temperatures=FALLBACK_TEMPERATURES, compression_ratio_threshold="auto", logprob_threshold=-1.0,
                    no_speech_threshold=0.6, vocab=None, seed=0, vocab_size=None, condition_on_previous_text=False,
                    prompt_reset_on_temperature=0.5, word_timestamps=False, no_timestamps=None,
                    prepend_punctuations=None, append_punctuations=None, best_of=None, length_penalty=None, beam_size=None,
                    patience=None, reuse_encoder=False, sample_rates=None, clip_timestamps=None,
                    hallucination_silence_threshold=None, carry_initial_prompt=False, vad=None, parallel_clips=None,
                    repetition_penalty=None, no_repeat_ngram_size=None, teacher_panel=None, sequence_bias=None, bad_words=None,
                    boost_phrases=None, phrase_boost=None, draft=None, draft_len=None, prompt_panel=None, recording_bias=None,
                    top_k=None, top_p=None, min_p=None, alternatives=None, constraint=None, fallback="lockstep", channels=None,
                    channel_ratio=1.1):
    """openai-whisper transcribe() for recordings of any length, batched across the recordings.
    condition_on_previous_text defaults to False here (openai-whisper: True); see 5.  word_timestamps: see 6.
    clip_timestamps, hallucination_silence_threshold, carry_initial_prompt: see 10 - 12; at their defaults the function
    makes exactly the calls it made before they existed.

    1. One wm_logmel_long call for all recordings, kept on the device; content_frames = T_r - 3000.
       sample_rates (one rate per recording; recordings [n] or [n][C] int16 / float32 at those rates): ONE wm_resample_16k
       call first makes the 16 kHz mono samples on the device (Context.resample_16k) and the log-mel reads that buffer
       where it lies (Context.logmel_long_device) -- no host round trip.  Everything behind the log-mel is as without the
       argument, and equals transcribe_long on the samples downloaded from resample_16k.  None (the default): the
       recordings are 16 kHz mono and the function makes exactly the calls it made before the argument existed.
    2. language None: per recording, openai-whisper's detect_language on mel[:, :3000] (wm_encode + the language-token
       softmax, ids lang_first .. lang_last); otherwise a token id for all recordings or a list of one per recording.
    3. Rounds: every unfinished recording decodes its window mel[:, seek : seek + segment_size], segment_size =
       min(3000, content_frames - seek), prompt [sot_prev, *initial_prompt_tokens[-(n_text_ctx // 2 - 1):]] (when
       given) + [sot, language, task], max_new = n_text_ctx // 2, in ONE wm_transcribe_mel call per fallback step
       (fallback_decode: transcribe_with_fallback's rule and seeds).  Row sample id = (window ordinal << 16) |
       recording id, so a recording's samples depend on itself only; recording ids default to 0 .. R - 1, < 65536.
    4. Per window: should_skip_window, else window_segments.
    5. condition_on_previous_text=True (needs sot_prev): per recording, a window's prompt is conditioned_prompt() of the
       recording's history -- initial_prompt_tokens, then the tokens of every kept window's segments, restarted behind a
       window whose final temperature exceeds prompt_reset_on_temperature (conditioned_history()).  The rows of a round
       then have prompts of different lengths and go out in ONE wm_transcribe_mel_ragged call per fallback step.  max_new
       is min(n_text_ctx // 2, n_text_ctx - (n_text_ctx // 2 + 3)) for every window of such a run (221 at 448): a row's
       budget depends neither on its own prompt nor on the other rows, so batched equals alone.  openai-whisper allows 224
       tokens after a short prompt and 222 after a full one; only a window that fills its whole budget can tell.
    6. word_timestamps=True (needs vocab and no_timestamps, the id of <|notimestamps|>): per round, after the decode, the
       kept windows that have a text token and at least 2 frames go out in ONE wm_align_mel call -- the decode's own mel,
       seek and segment_size, start sequence [sot, language_r, task], median filter 7 -- and window_word_timestamps gives
       every segment its `words` and adjusts its start / end, each recording with its own running last speech timestamp.
       As in openai-whisper, the clearing of instantaneous / text-less segments then runs AFTER the word step, and a
       window that did not end in a single timestamp moves the seek to the end of its last word when that lies behind
       the window's start.  Words are split by spaces unless the language token, counted from sot + 1 in
       Whisper.LANGUAGES, is one of zh / ja / th / lo / my.  This project's rule where openai-whisper defines nothing:
       a window of fewer than 2 frames (no audio frame to align to), like a skipped window or one without a text token,
       gets `words` [] on its segments and the seek of word_timestamps=False.
       prepend_punctuations / append_punctuations: None = openai-whisper's defaults (PREPEND_ / APPEND_PUNCTUATIONS).
    7. best_of (openai-whisper's best_of; None: one sample per window): a fallback step with temperature > 0 decodes best_of
       candidates per window in ONE wm_transcribe_mel_best_of call -- same seeds, same sample ids -- and hands
       fallback_decode each window's best candidate under length_penalty (rank_candidates; None = openai-whisper's None).
       The temperature-0 step is unchanged.  Every window record then has `candidate`, the index its last step kept.
    8. beam_size (openai-whisper's beam_size, with patience; None: greedy): the temperature-0 step of every round is ONE
       wm_transcribe_mel_beam call -- max_candidates = round(beam_size * patience), ranked under length_penalty -- and
       hands fallback_decode each window's best hypothesis (sum_logprob: the search's own f32 sum); the steps above
       temperature 0 are unchanged (openai-whisper uses beam_size at temperature 0 and best_of above it).  Every window
       record then has `hypothesis`, the index that was kept (0 when a later step replaced the beam result).  patience
       without beam_size is a ValueError; with beam_size None the calls made are exactly those without the argument.
    9. reuse_encoder=True: every window is encoded ONCE.  A round makes one wm_windows_encode of its live windows; every
       fallback step decodes the rows it still has to do from that set (wm_transcribe_windows / _beam), the word step aligns
       its kept rows from it (wm_align_windows), and the set is freed before the next round begins, also on an exception.
       Language identification becomes one wm_windows_encode of every recording's frames [0, 3000) plus
       wm_windows_detect_language, without host round trips.  The result equals the reuse_encoder=False run in every field;
       what it costs is the sets' device memory (Windows.nbytes: 246 MB per live recording at large-v2).  The default,
       False, makes exactly the calls this function made before the argument existed.
    10. clip_timestamps (None; a string of comma-separated seconds, "" = none; a flat list of seconds for every recording;
       or a list of R such lists / strings): only these spans of a recording are decoded.  clip_times / seek_clips: seek
       points round(t * 100), the recording's end closes an odd count, no time = the whole recording.  This project's
       rules: times are finite, >= 0 and non-decreasing (ValueError, before any library call), a clip is cut to [0,
       content_frames), a clip that is empty after the cut is dropped, and a recording left without a clip decodes no
       window (segments, seeks, windows [], its language as usual).  Per recording a clip cursor: before a round, a seek
       at or past the clip's end moves to the next clip's start (backwards too: a window's timestamps may point far
       past a short clip), the recording is finished when the clips run out, and the window is segment_size = min(3000,
       content_frames - seek, clip_end - seek) frames -- for the decode, the word step and every seek rule.  Language
       identification still reads frames [0, 3000).  Every window record gains `clip`, the index of its (start, end)
       pair in the times as given (dropped clips keep their number).
    11. hallucination_silence_threshold (seconds, finite and >= 0; needs word_timestamps; else ValueError): per kept
       window, after window_word_timestamps and before the clearing of empty segments, hallucination_silence_skip decides
       the next seek and which segments stay; a "leading" window keeps no segment and changes neither the history nor the
       last speech timestamp, which otherwise follows the segments that remain.  The window record gets `hallucination`
       ("leading" / "surrounded") when a rule fired, and `dropped_segments` with "surrounded".
    12. carry_initial_prompt=True: with condition_on_previous_text and a non-empty initial prompt, every window's prompt is
       carried_prompt() -- the initial prompt stays in front of the history's tail.  This project's rule: an initial
       prompt of n_text_ctx // 2 - 1 tokens or more leaves no room for history, and its last n_text_ctx // 2 - 1 tokens
       are the text.  Without conditioning or without an initial prompt nothing changes.
    13. vad (None; True; or a dict of overrides: band (lo, hi), smooth, params -- wm_vad_params' fields --, max_frames):
       after the log-mel ONE wm_vad_energy call covers all recordings (n_frames = content_frames, band vad_band(n_mels),
       smooth 5), the tracks are downloaded, and per recording vad_segments and vad_clips make its clip list directly in
       frames, (start, end, index) as seek_clips returns it; everything behind is 10.  A recording without contrast is one
       clip (wm_vad_segments' flat rule), one without a span decodes no window.  vad with clip_timestamps is a ValueError.
       The recording's result gains vad_segments and vad_clips.  The defaults are not validated on real speech; any other
       detector's spans can be passed as clip_timestamps instead.
    14. parallel_clips (None; N >= 1; True = 56): the clips of a recording advance in the same round.  Every clip (of 10
       or 13; without either, the recording's one clip) is a LANE with its own seek, "before" record and last speech
       timestamp (which starts at the clip's start time); a round holds one window of each of the first N unfinished lanes
       in (recording, clip) order, and a lane is finished when its seek reaches its clip's end.  The lanes are an index map
       onto the recordings' mel, language, prompt and id.  Row sample id = (((clip << 4) | min(window index within the
       clip, 15)) & 0xFFFF) << 16 | recording id: a lane's noise is its own, so a lane of a parallel run equals the same
       clip run alone (its number kept).  At temperatures=(0.0,) the result equals the sequential clip run.  Per recording
       the segments and windows come in (clip, decode order), ids renumbered; every window record carries `clip` and
       `round`.  ValueError with condition_on_previous_text (history is serial) and with
       hallucination_silence_threshold.  reuse_encoder encodes the round's lanes as one set: N bounds its memory.
    15. repetition_penalty / no_repeat_ngram_size (None, None: off): the repetition rules of Context.set_repetition_rules
       (wm_set_repetition_rules; a None of the two is 1.0 / 0, eot is this call's eot) are set on the context behind the
       log-mel, hold for every decode call of the run -- greedy, sampled, best-of, beam, from windows --, and are cleared
       again when the function leaves, also on an exception.  They act on a row's generated tokens only, so the prompts of
       5 and 12 are never penalised.  With both None the function makes exactly the calls it made before they existed.
    16. teacher_panel (None; 1 .. 8): with word_timestamps, Context.set_teacher_panel(teacher_panel) is called ONCE, in front of
       the run's first alignment call, and stays set on the context: the teacher-forced pass of every alignment then carries
       that many positions per decoder step (wm_set_teacher_panel: a launch policy, the words are the same bit for bit).  A
       value outside 1 .. 8 is a ValueError before any library call.  None makes no call.
    17. sequence_bias / bad_words / boost_phrases (all None: off): ONE table for Context.set_sequence_bias
       (wm_set_sequence_bias, eot is this call's eot) -- sequence_bias {token tuple: bias} as Hugging Face's sequence_bias,
       bad_words [token sequence, ...] with bias -inf (bad_words_ids; CTranslate2's suppress_sequences), boost_phrases [token
       sequence, ...] with bias phrase_boost (a finite float, required with them) and boosted prefixes, so that a phrase is
       helped from its first token on.  A sequence named twice is a ValueError before any library call.  The table is set
       behind the log-mel (behind the repetition rules of 15), holds for every decode call of the run and is cleared again
       when the function leaves, also on an exception.  It acts on a row's generated tokens only.  The ids are the caller's
       tokenizer's: Whisper's " word" and "word" are different ids, and both variants are the caller's to list.  With all
       three None the function makes exactly the calls it made before they existed.
    18. word_timestamps="decode": the words of 6. WITHOUT the alignment call.  Every fallback attempt of a round goes through
       the aligned entry (Context.transcribe_mel_aligned; with reuse_encoder transcribe_windows_aligned: the same tokens bit
       for bit, plus the start frame of every generated token from the decode's own cross-attention queries), and the kept
       attempt's start frames feed window_word_timestamps through decode_alignment_text, cut to the text tokens the window's
       segments kept.  No align_* call is made; the seek to the last word's end, the hallucination rules of 11 and the
       clearing of empty segments run unchanged on the new word times.  The semantic difference from openai-whisper (and
       from word_timestamps=True): the aligned queries are the DECODE's -- its prompt (previous text is no row, but
       [sot, language, task] are), timestamp tokens interleaved with the text -- not those of a clean [sot, language, task,
       <|notimestamps|>, text] pass, and a word's probability is exp(log-prob) under the filtered distribution the decode
       chose from.  The word times therefore differ slightly from 6.'s; the tokens do not.  no_timestamps is not needed;
       teacher_panel has nothing to act on.  Together with best_of or beam_size it is a ValueError before any library call.
       word_timestamps True / False make exactly the calls they made before the mode existed.
    19. word_timestamps="decode_best": 18. for a run with best_of and / or beam_size ("decode" exactly when neither is set).  A
       fallback step that decodes by beam search goes through Context.transcribe_mel_beam_aligned, one that samples best_of
       candidates through transcribe_mel_best_of_aligned (with reuse_encoder the transcribe_windows_* pair), any other through
       18.'s entry; the tokens are those of the plain entries bit for bit, and the start frames are those of the hypothesis
       the step's ranking chose -- the one the window keeps.  For every other value of word_timestamps the calls are unchanged.
    20. draft (None; a Context with a small model of the same vocabulary on the same device) / draft_len (1 .. 7, default 4):
       speculative decoding.  The temperature-0 step of every round whose rows have prompts of one length goes through
       Context.transcribe_mel_speculative -- the draft proposes draft_len tokens at a time, panels of this context verify
       them; the tokens, log-probs and no_speech_prob are those of the plain call bit for bit, so the run's result is the
       same in every field --, every other step and a round of ragged prompts (per-recording initial prompts) through the
       plain entries.  The timestamp rules this function sets on the context are set on the draft too; the suppress lists
       of both are the caller's.  ValueError before any library call: with condition_on_previous_text=True, best_of,
       beam_size, word_timestamps='decode*', reuse_encoder, repetition_penalty / no_repeat_ngram_size, a sequence bias, or
       draft_len without draft.  With draft None the function makes exactly the calls it made before the argument existed.
    21. prompt_panel (None; 1 .. 8): Context.set_prompt_panel(prompt_panel) is called ONCE, in front of the first decode call:
       from then on a decode group steps through the prompt positions whose logits nobody reads that many at a time, without
       the logits product (wm_set_prompt_panel: a launch policy -- every segment is the same bit for bit).  What it is for is
       condition_on_previous_text, whose prompts carry up to n_text_ctx / 2 - 1 tokens of previous text.  The width is not
       restored afterwards.  Best-of, beam-search and speculative steps ignore it.  ValueError before any library call for
       anything but None or an integer 1 .. 8.  With None the function makes exactly the calls it made before the argument
       existed.
    22. recording_bias (None; a list of R entries): 17. PER RECORDING, in the same batched calls.  Entry r is None (no bias) or a
       dict with any of sequence_bias / bad_words / boost_phrases / phrase_boost, which long_bias_table turns into recording
       r's table exactly as 17. does for the run's one table (long_recording_tables; equal tables are stored once).  The tables
       are set ONCE behind the log-mel (Context.set_sequence_bias_tables, eot is this call's eot; behind the repetition rules
       of 15), and in front of EVERY decode call -- every fallback step's rows, from the mel or from a reuse_encoder set, best-of,
       beam and aligned steps alike -- Context.set_bias_rows names the tables of exactly that call's rows; with parallel_clips a
       clip takes its recording's table.  A row then decodes, bit for bit, as the run of its recording alone with its table as
       17.'s.  The tables are cleared again when the function leaves, also on an exception.  Where NO entry has a table
       (all None, or dicts whose three lists are None) the function makes the plain run's calls: nothing is set.
       ValueError before any library call: together with sequence_bias, bad_words or boost_phrases, with draft, for anything
       but one entry per recording, for an unknown key and for what long_bias_table refuses.  With None the function makes
       exactly the calls it made before the argument existed.
    23. top_k / top_p / min_p (all None: off): the sampling rules of Context.set_sampling_rules (wm_set_sampling_rules; a None of
       the three reads as off) are set on the context behind the sequence bias, held for the run and cleared on leaving it, also on
       an exception.  They truncate the distribution of every fallback step above temperature 0 (best_of candidates included);
       the temperature-0 step, beam search and a draft's speculative steps ignore them.  Hugging Face's long-form fallback samples
       under its generation config's top_k = 50.  ValueError before any library call for a bad value (sampling_rules_args).  With
       all three None the function makes exactly the calls it made before the arguments existed.
    24. alternatives (None; 1 .. MAX_ALTERNATIVES): Context.request_alternatives (wm_request_alternatives) goes in front of EVERY
       decode call of every round -- each fallback step's rows, from the mel or from a reuse_encoder set, best-of and aligned
       steps alike --, and the kept attempt's values go into each segment: token_alternatives, per token of the segment's `tokens`
       a list of (id, logprob) -- the n best admissible ids at that position with their log-probs under the filtered
       distribution at temperature 1 --, and token_entropy, per token the entropy of that distribution in nats.  A segment
       cleared as empty loses both with its tokens.  ValueError before any library call for a value out of range and together
       with beam_size or draft (a beam's alternatives need its ancestry; a speculative step verifies the greedy choice alone).
       With None the function makes exactly the calls it made before the argument existed.
    25. constraint (None: off; a Constraint of constraint_from_choices / constraint_join or of the caller's own arrays): the
       automaton of Context.set_constraint (wm_set_constraint, eot is this call's eot) is set on the context behind the sampling
       rules, held for the run and cleared on leaving it, also when a decode raises.  Every window of every recording starts in
       state 0: the text ids of a window form a member of the language (or a prefix of one where the window's tokens run out),
       the timestamps around and between them are the timestamp rules' business.  ValueError before any library call for
       anything but a Constraint and together with draft.  With None the function makes exactly the calls it made before the
       argument existed.
    26. fallback ("lockstep", the default: the rounds of 3.; "deferred"): a window that needs a temperature fallback does not hold
       its round open.  Every round makes ONE decode call whose rows carry their own temperature and seed
       (Context.set_sampling_rows, wm_set_sampling_rows): a unit whose window's attempt k failed fallback_decode's rule
       (needs_fallback) and has a temperature left keeps that window open, does not advance, and is a live unit of the next round
       with attempt k + 1 -- the same window, prompt and sample id at temperatures[k + 1] and fallback_seed(seed, k + 1) -- beside
       the other units' next windows at temperatures[0].  The window's record lists the temperatures it ran, its kept attempt is
       the last one, and the word step runs over the windows a round kept.  Per recording, language, segments, seeks and the
       window records except `round` equal the lockstep run's exactly: a row's bits depend on its own window, prompt, sample id,
       temperature and seed, and the sample id does not depend on the round.  ValueError before any library call for any other
       value and for "deferred" together with best_of, beam_size, draft or reuse_encoder.  With "lockstep" the function makes
       exactly the calls it made before the argument existed.
    27. channels (None; "split"; "diarize") / channel_ratio: multichannel recordings.  Both modes need sample_rates (the
       interleaved path of 1.).  "split": ONE wm_resample_16k_mix call with identity rows (Context.resample_16k_mix) takes the
       place of the wm_resample_16k call, and from the log-mel on every (recording, channel) is a recording of its own, in
       (r, c) order: language, initial_prompt_tokens, clip_timestamps and recording_bias given per recording are repeated per
       channel, recording_ids is one id per channel-recording (default 0 .. sum(C_r) - 1).  The run IS transcribe_long on the
       list of the mono 16 kHz signals resample_16k_mix returns, with the same keywords, and works with every other option.
       The result of recording r is a dict: `channels`, its channels' results as this function returns them, and `segments`,
       copies of all their segments with `channel`, ordered by (start, channel).  "diarize": the decode is the channels=None
       run call for call -- the mean is what the model hears --; behind it ONE wm_resample_16k_mix with identity rows and ONE
       wm_channel_activity over its device output (the split signals are freed at once), and every segment -- with word
       timestamps every word too -- gains speaker = speaker_by_channel(the recording's activity, start, end, channel_ratio): a
       channel index or None; None everywhere for a mono recording.  ValueError before any library call: any other value of
       channels, channels without sample_rates, a channel_ratio that is not finite and >= 1.  With None the function makes
       exactly the calls it made before the arguments existed.
    With vad and parallel_clips at None the function makes exactly the calls it made before they existed.
    A recording's seek strictly grows from one of its windows to the next within a clip (asserted).
    initial_prompt_tokens: one flat list for all recordings, or one list per recording (a list of R lists, empty allowed:
    no prompt).  Without conditioning a recording's list heads every one of its windows; with it, it seeds the history.
    Sets the context's timestamp rules (wm_set_timestamp_rules: timestamp_begin, eot, max initial timestamp 1.0 s);
    suppress lists are the caller's (Context.set_suppress).  Returns per recording a dict: language (token id),
    segments (openai-whisper's keys id seek start end tokens temperature avg_logprob compression_ratio no_speech_prob, plus
    text with a Vocab and words [{word, start, end, probability}] with word_timestamps), text (with a Vocab), seeks (the first frame of every decoded window) and windows (per window:
    seek, segment_size, the fallback steps' temperatures, skipped, prompt_len, prompt)."""
    counts = None   # 27.: the channels of every recording (None: off)
    channel_ratio = _channel_ratio(channel_ratio)
    if channels is not None:
        if channels not in ("split", "diarize"):
            raise ValueError("channels: None, 'split' or 'diarize'")
        if sample_rates is None:
            raise ValueError("channels needs sample_rates: the recordings are interleaved at their own rates")
        if len(sample_rates) != len(recordings):
            raise ValueError("sample_rates: one per recording")
        counts = _channel_counts(recordings)
        if channels == "split":
            language, initial_prompt_tokens, clip_timestamps, recording_bias = _split_arguments(
                counts, language, initial_prompt_tokens, clip_timestamps, recording_bias)
    split = channels == "split"
    o = _LongOptions(**locals())
    R = sum(counts) if split else len(recordings)   # (split: every channel is a recording from the log-mel on)
    o.early(R)
    sampling = sampling_rules_args(top_k, top_p, min_p)   # 23. (None: off)
    constraint_args(constraint)   # 25. (None: off)
    if constraint is not None and draft is not None:
        raise ValueError("draft (speculative decoding) cannot be combined with a constraint")
    bias_table = long_bias_table(sequence_bias, bad_words, boost_phrases, phrase_boost)   # 17. (None: off)
    o.rec_tables = None   # 22.: the table of every recording (None: off)
    if recording_bias is not None:
        if bias_table is not None:
            raise ValueError("recording_bias cannot be combined with sequence_bias, bad_words or boost_phrases: a context has "
                             "one table or a table per row")
        if draft is not None:
            raise ValueError("draft (speculative decoding) cannot be combined with a sequence bias")
        rec_tables, rec_boosts, of_rec = long_recording_tables(recording_bias, R)
        if rec_tables:   # no entry with a table: off (a map needs tables in force, and an all -1 map is the plain run)
            o.rec_tables = of_rec
    ctx.set_timestamp_rules(True, timestamp_begin, eot, int(round(1.0 / TIME_PRECISION)))
    if draft is not None:   # 20.: the draft proposes under the same rules
        draft.set_timestamp_rules(True, timestamp_begin, eot, int(round(1.0 / TIME_PRECISION)))
    out = [dict(language=None, segments=[], seeks=[], windows=[]) for _ in range(R)]
    if R == 0:
        return out
    d_mel, mel_offs, T = _long_mel(o, R)
    source = None   # the rows of the round in progress
    rules = repetition_penalty is not None or no_repeat_ngram_size is not None
    try:
        if rules:   # 15.
            ctx.set_repetition_rules(1.0 if repetition_penalty is None else repetition_penalty,
                                     0 if no_repeat_ngram_size is None else no_repeat_ngram_size, eot)
        if bias_table is not None:   # 17.
            ctx.set_sequence_bias(bias_table[0], bias_table[1], eot=eot)
        if o.rec_tables is not None:   # 22.
            ctx.set_sequence_bias_tables(rec_tables, rec_boosts, eot=eot)
        if sampling is not None:   # 23.
            ctx.set_sampling_rules(*sampling)
        if constraint is not None:   # 25.
            ctx.set_constraint(constraint, eot=eot)
        langs = _long_languages(o, d_mel, mel_offs, T)
        o.prompt_head()
        units = _long_units(o, out, langs, d_mel, mel_offs, T)
        n_round = -1
        # 3. rounds in lockstep
        while True:
            if source is not None:   # the previous round's (reuse_encoder: its set)
                source.close()
                source = None
            live = [u for u in units if u.attempt or u.advance()][:o.par_n]   # (26.: a window held open is not advanced past)
            if not live:
                break
            n_round += 1
            for u in live:
                if not u.attempt:
                    u.size = u.open_window()
            sizes = [u.size for u in live]
            prompts = [u.prompt(o) for u in live]
            # (9. reuse_encoder: the round's windows are encoded once here, for every fallback step and the word step)
            source = _RoundRows(o, d_mel, live, sizes, prompts, [u.sample_id() for u in live])
            if o.prompt_panel_pending:   # 21.
                ctx.set_prompt_panel(int(prompt_panel))
                o.prompt_panel_pending = False
            if o.deferred:   # 26.: ONE call, every row at its own attempt's temperature and seed; the rule is fallback_decode's
                ks = [u.attempt for u in live]
                row_ts = ([float(temperatures[k]) for k in ks], [fallback_seed(seed, k) for k in ks])
                res = fallback_decode(lambda todo, t, sd: source.decode(todo, t, sd, rows=row_ts), len(live), o.vocab_size, o.max_new,
                                      eot, (0.0,), compression_ratio_threshold, logprob_threshold, no_speech_threshold, vocab, seed)
                res["temperature"][:] = row_ts[0]
                res["seed"][:] = row_ts[1]
            else:
                res = fallback_decode(source.decode, len(live), o.vocab_size, o.max_new, eot, temperatures, compression_ratio_threshold,
                                      logprob_threshold, no_speech_threshold, vocab, seed)
            kept = []   # word_timestamps: (row of the round, segments, next seek, single_timestamp_ending) of every kept window
            for i, u in enumerate(live):
                ran = [st[0] for st in res["steps"] if i in st[2]]
                if o.deferred:
                    u.tried.append(row_ts[0][i])
                    if res["needs_fallback"][i] and u.attempt + 1 < len(temperatures):   # the window stays open: the next round
                        u.attempt += 1
                        continue
                    ran, u.tried, u.attempt = u.tried, [], 0
                n_text = n_text_tokens(res["tokens"][i, :res["lens"][i]], eot)
                tokens = res["tokens"][i, :n_text]
                result = {k: float(res[k][i]) for k in ("temperature", "avg_logprob", "compression_ratio", "no_speech_prob")}
                alt_kw = {}   # 24.: the kept attempt's alternatives and entropy of the window's tokens
                if "alt_tokens" in res:
                    alt_kw = dict(alternatives=(token_alternatives(res["alt_tokens"][i, :n_text], res["alt_logprobs"][i, :n_text],
                                                                   res["alt_counts"][i, :n_text]),
                                                [float(h) for h in res["entropy"][i, :n_text]]))
                skip = should_skip_window(result["no_speech_prob"], result["avg_logprob"], no_speech_threshold,
                                          logprob_threshold)
                u.record_window(o, sizes[i], prompts[i], ran, skip, tokens, n_round, source.kept_by[i])
                if skip:
                    u.seek += sizes[i]
                elif o.words_on:
                    kept.append((i,) + window_segments(tokens, u.seek, sizes[i], timestamp_begin, eot, result, vocab,
                                                       cleanup=False, **alt_kw))
                else:
                    u.commit(o, *window_segments(tokens, u.seek, sizes[i], timestamp_begin, eot, result, vocab, **alt_kw),
                             result["temperature"])
            if kept:
                if o.panel_pending and not o.words_decode:   # 16.
                    ctx.set_teacher_panel(int(teacher_panel))
                    o.panel_pending = False
                _long_word_step(o, source, live, sizes, kept, res)
        for u in units:
            u.deliver(out[u.rec])
    finally:
        try:
            if source is not None:
                source.close()
            ctx.dev_free(d_mel)
        finally:
            try:
                try:
                    if constraint is not None:
                        ctx.set_constraint(None)
                finally:
                    if sampling is not None:
                        ctx.set_sampling_rules()
            finally:
                try:
                    if bias_table is not None:
                        ctx.set_sequence_bias(None)
                    if o.rec_tables is not None:
                        ctx.set_sequence_bias_tables(None)
                finally:
                    if rules:
                        ctx.set_repetition_rules(1.0, 0, eot)
    if vocab is not None:
        for rec in out:
            rec["text"] = vocab.decode([t for sg in rec["segments"] for t in sg["tokens"] if t < eot])
    if channels == "diarize":   # 27.
        _diarize_results(ctx, out, recordings, sample_rates, counts, channel_ratio)
    return _split_results(out, counts) if split else out


class Windows:
    """RAII wrapper over wm_windows (Context.encode_windows): the encoded state -- cross-attention K/V -- of W mel windows,
    read by Context.transcribe_windows*, align_windows and windows_detect_language of the context that made it and of its
    clones.  n_frames i32 [W]: the windows' mel frames.  Close it (or leave its `with` block) before the context."""

    def __init__(self, ctx, handle, n_frames):
        self.ctx, self.lib, self.handle, self.n_frames = ctx, ctx.lib, handle, n_frames

    def __len__(self):
        return int(self.lib.wm_windows_count(self.handle))

    @property
    def nbytes(self):
        """device bytes the set holds"""
        return int(self.lib.wm_windows_bytes(self.handle))

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self.lib.wm_windows_free(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def stream_frame_counts(n_samples, capacity_frames):
    """The counters of a live stream that has received n_samples (wm_streams_frames): (final_frames F, avail_frames A,
    first_kept K).  Frame t reads the samples [160 t - 200, 160 t + 200); frame 0's reflected half reads sample 200."""
    n = int(n_samples)
    final = 0 if n < 201 else (n - 200) // 160 + 1
    avail = 0 if n <= 0 else (n + 199) // 160 + 1
    return final, avail, max(0, avail - int(capacity_frames))


class Streams:
    """RAII wrapper over wm_streams: S live audio streams whose appended samples become log-mel frames incrementally on
    the device (push), any window of which is normalised on demand (window).  A front-end-only context is enough.  Close
    it (or leave its `with` block) before the context."""

    def __init__(self, ctx, S, n_mels=80, capacity_frames=3003):
        self.ctx, self.lib = ctx, ctx.lib
        self.S, self.n_mels, self.capacity_frames = int(S), int(n_mels), int(capacity_frames)
        self.handle = ctypes.c_void_p()
        _check(self.lib, self.lib.wm_streams_create(ctx.handle, self.S, self.n_mels, self.capacity_frames,
                                                    ctypes.byref(self.handle)))

    def push(self, pieces):
        """wm_streams_push: pieces[s] = the new samples of stream s (1-D int16 / float32 / float64; one dtype per call) or
        None for nothing.  One launch for all streams."""
        if len(pieces) != self.S:
            raise ValueError("push takes one entry per stream (%d), got %d" % (self.S, len(pieces)))
        arrs = [np.ascontiguousarray(p).reshape(-1) for p in pieces if p is not None and len(p)]
        dtype = arrs[0].dtype if arrs else np.dtype(np.float32)
        if any(a.dtype != dtype for a in arrs) or dtype not in _DTYPES:
            raise ValueError("the pieces of one push share one dtype of int16 / float32 / float64")
        lens = [0 if p is None else len(p) for p in pieces]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        pcm = np.concatenate(arrs) if arrs else np.zeros(1, dtype)
        _check(self.lib, self.lib.wm_streams_push(self.ctx.handle, self.handle, _ptr(pcm), _DTYPES[pcm.dtype], _ptr(offs),
                                                  WM_MEM_HOST))

    def reset(self, s):
        """wm_streams_reset: stream s is empty again."""
        _check(self.lib, self.lib.wm_streams_reset(self.ctx.handle, self.handle, int(s)))

    def frames(self):
        """wm_streams_frames: (samples, final_frames, avail_frames, first_kept), i64 [S] each."""
        out = [np.zeros(self.S, np.int64) for _ in range(4)]
        _check(self.lib, self.lib.wm_streams_frames(self.handle, *[_ptr(o) for o in out]))
        return tuple(out)

    def window(self, rows, device=True):
        """wm_streams_window: rows = (stream, first_frame, n_frames) triples, one launch for all of them.  Returns a list of
        f32 [n_mels][n_frames] arrays with device=False; device=True keeps the blocks on the device, back to back: (pointer,
        out_base i64 [R], n_frames i32 [R]) -- what transcribe_mel takes as (mel, mel_base, mel_len) with seek 0; free the
        pointer with the context's dev_free."""
        rows = [(int(s), int(f), int(n)) for s, f, n in rows]
        R = len(rows)
        stream = np.array([r[0] for r in rows], np.int32)
        first = np.array([r[1] for r in rows], np.int64)
        n = np.array([r[2] for r in rows], np.int32)
        base = np.concatenate([[0], np.cumsum(np.maximum(n, 0).astype(np.int64) * self.n_mels)]).astype(np.int64)
        if not device:
            out = np.empty(max(int(base[-1]), 1), np.float32)
            _check(self.lib, self.lib.wm_streams_window(self.ctx.handle, self.handle, R, _ptr(stream), _ptr(first), _ptr(n),
                                                        _ptr(out), _ptr(base), WM_MEM_HOST))
            return [out[base[r]:base[r + 1]].reshape(self.n_mels, n[r]) for r in range(R)]
        d_out = self.ctx.dev_malloc(max(int(base[-1]), 1) * 4)
        try:
            _check(self.lib, self.lib.wm_streams_window(self.ctx.handle, self.handle, R, _ptr(stream), _ptr(first), _ptr(n),
                                                        d_out, _ptr(base), WM_MEM_DEVICE))
        except Exception:
            self.ctx.dev_free(d_out)
            raise
        return d_out, base[:-1].copy(), n

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self.lib.wm_streams_free(self.ctx.handle, self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Context:
    """Thin RAII wrapper over wm_ctx (front end only unless `dims` is given)."""

    def __init__(self, dims=None, device=0, debug=False):
        self.lib = load_debug_library() if debug else load_library()
        self.handle = ctypes.c_void_p()
        if dims is None:
            _check(self.lib, self.lib.wm_create_frontend(int(device), ctypes.byref(self.handle)))
            self.dims = None
        else:
            d = wm_dims(**dims) if isinstance(dims, dict) else dims
            _check(self.lib, self.lib.wm_create(ctypes.byref(d), int(device), ctypes.byref(self.handle)))
            self.dims = d.as_dict()

    def clone(self):
        """Second context sharing this one's finalised weights (own stream / caches): for overlapping
        independent batches on one GPU from several host threads."""
        c = Context.__new__(Context)
        c.lib = self.lib
        c.handle = ctypes.c_void_p()
        c.dims = dict(self.dims)
        c._parent = self   # keep the weight owner alive
        _check(self.lib, self.lib.wm_clone(self.handle, ctypes.byref(c.handle)))
        return c

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self.lib.wm_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- front end ------------------------------------------------------------------
    def logmel(self, pcm, n_mels=80, out_dtype=np.float32):
        """wm_logmel on host arrays.  pcm: [n][480000] int16 / float32 / float64."""
        pcm = np.ascontiguousarray(pcm)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        if pcm.ndim != 2 or pcm.shape[1] != N_SAMPLES:
            raise ValueError("pcm must be [n_chunks][%d], got %r" % (N_SAMPLES, pcm.shape))
        if pcm.dtype not in _DTYPES:
            raise ValueError("pcm dtype must be int16/float32/float64, got %s" % pcm.dtype)
        n = pcm.shape[0]
        out = np.empty((n, n_mels, N_FRAMES), dtype=out_dtype)
        _check(self.lib, self.lib.wm_logmel(self.handle, _ptr(pcm), _DTYPES[pcm.dtype], n, n_mels,
                                            _ptr(out), _DTYPES[np.dtype(out_dtype)], WM_MEM_HOST))
        return out

    def logmel_long(self, recordings, n_mels=80, device=False):
        """wm_logmel_long: openai-whisper's log_mel_spectrogram(audio, padding=480000) of each recording (1-D int16 /
        float32 / float64 arrays of any length).  Returns a list of f32 [n_mels][T_r] arrays, T_r = (len_r + 480000) //
        160; device=True keeps the result on the device and returns (pointer, element offsets i64 [R + 1], T i32 [R])
        -- free the pointer with dev_free."""
        pcm, offs = _pack_recordings(recordings)
        R = len(offs) - 1
        T = ((np.diff(offs) + N_SAMPLES) // 160).astype(np.int32)
        mel_offs = np.concatenate([[0], np.cumsum(T.astype(np.int64) * n_mels)]).astype(np.int64)
        if not device:
            out = np.empty(max(int(mel_offs[-1]), 1), dtype=np.float32)
            _check(self.lib, self.lib.wm_logmel_long(self.handle, _ptr(pcm), _DTYPES[pcm.dtype], _ptr(offs), R, n_mels,
                                                     _ptr(out), WM_MEM_HOST))
            return [out[mel_offs[r]:mel_offs[r + 1]].reshape(n_mels, T[r]) for r in range(R)]
        d_pcm = self.to_device(pcm) if pcm.nbytes else None
        try:
            return self.logmel_long_device(d_pcm, pcm.dtype, offs, n_mels=n_mels)
        finally:
            if d_pcm is not None:
                self.dev_free(d_pcm)

    def logmel_long_device(self, d_pcm, dtype, sample_offsets, n_mels=80):
        """wm_logmel_long on samples that are on the device already (e.g. resample_16k(..., device=True)'s): d_pcm of
        `dtype` (int16 / float32 / float64), sample_offsets i64 [R + 1].  The caller keeps d_pcm.  Returns (pointer, element
        offsets i64 [R + 1], T i32 [R]) -- free the pointer with dev_free."""
        offs = np.ascontiguousarray(sample_offsets, dtype=np.int64)
        R = len(offs) - 1
        T = ((np.diff(offs) + N_SAMPLES) // 160).astype(np.int32)
        mel_offs = np.concatenate([[0], np.cumsum(T.astype(np.int64) * n_mels)]).astype(np.int64)
        d_out = self.dev_malloc(max(int(mel_offs[-1]), 1) * 4)
        try:
            _check(self.lib, self.lib.wm_logmel_long(self.handle, d_pcm, _DTYPES[np.dtype(dtype)], _ptr(offs), R, n_mels, d_out,
                                                     WM_MEM_DEVICE))
            self.sync()
        except Exception:
            self.dev_free(d_out)
            raise
        return d_out, mel_offs, T

    def resample_16k(self, recordings, sample_rates, device=False):
        """wm_resample_16k: recordings ([n] or [n][C] int16 / float32 arrays) at sample_rates[r] Hz -> 16 kHz mono f32, one
        launch for all of them.  Returns a list of f32 arrays [ceil(n_r L_r / M_r)]; device=True keeps the samples on the
        device and returns (pointer, sample offsets i64 [R + 1]) -- what logmel_long_device reads; free the pointer with
        dev_free."""
        pcm, offs, ch, rates = _pack_interleaved(recordings, sample_rates)
        R = len(ch)
        frames = np.diff(offs) // np.maximum(ch, 1)
        out_offs = np.zeros(R + 1, dtype=np.int64)
        out_offs[1:] = np.cumsum([resample_out_len(int(n), int(sr)) for n, sr in zip(frames, rates)])
        if not device:
            out = np.empty(max(int(out_offs[-1]), 1), dtype=np.float32)
            _check(self.lib, self.lib.wm_resample_16k(self.handle, _ptr(pcm), _DTYPES[pcm.dtype], _ptr(offs), _ptr(ch), _ptr(rates),
                                                      R, _ptr(out), WM_MEM_HOST))
            return [out[out_offs[r]:out_offs[r + 1]] for r in range(R)]
        d_pcm = self.to_device(pcm) if pcm.nbytes else None
        d_out = None
        try:
            d_out = self.dev_malloc(max(int(out_offs[-1]), 1) * 4)
            _check(self.lib, self.lib.wm_resample_16k(self.handle, d_pcm, _DTYPES[pcm.dtype], _ptr(offs), _ptr(ch), _ptr(rates), R,
                                                      d_out, WM_MEM_DEVICE))
            self.sync()
        except Exception:
            if d_out is not None:
                self.dev_free(d_out)
            raise
        finally:
            if d_pcm is not None:
                self.dev_free(d_pcm)
        return d_out, out_offs

    def resample_16k_mix(self, recordings, sample_rates, mix, device=False):
        """wm_resample_16k_mix: resample_16k with a channel matrix.  mix: one [n_rows][C_r] array of finite weights per
        recording (channel_rows makes the usual ones); recording r yields n_rows signals, signal (r, o) the recording mixed
        under row o -- m = w[0] x[0], then fmaf(w[c], x[c], m) in channel order -- and resampled to 16 kHz.  One launch for
        all of them.  Returns per recording a list of f32 arrays; device=True keeps the signals on the device and returns
        (pointer, sample offsets i64 [sum(n_rows) + 1]), the signals in (r, o) order -- what logmel_long_device and
        channel_activity read; free the pointer with dev_free."""
        pcm, offs, ch, rates = _pack_interleaved(recordings, sample_rates)
        rows, flat = _pack_mix(mix, ch)
        R = len(ch)
        frames = np.diff(offs) // np.maximum(ch, 1)
        lens = [resample_out_len(int(n), int(sr)) for n, sr in zip(frames, rates)]
        out_offs = np.zeros(int(rows.sum()) + 1, dtype=np.int64)
        out_offs[1:] = np.cumsum(np.repeat(np.array(lens, dtype=np.int64), rows))
        args = (_DTYPES[pcm.dtype], _ptr(offs), _ptr(ch), _ptr(rates), R, _ptr(rows), _ptr(flat))
        if not device:
            out = np.empty(max(int(out_offs[-1]), 1), dtype=np.float32)
            _check(self.lib, self.lib.wm_resample_16k_mix(self.handle, _ptr(pcm), *args, _ptr(out), WM_MEM_HOST))
            first = np.concatenate([[0], np.cumsum(rows)])
            return [[out[out_offs[s]:out_offs[s + 1]] for s in range(first[r], first[r + 1])] for r in range(R)]
        d_pcm = self.to_device(pcm) if pcm.nbytes else None
        d_out = None
        try:
            d_out = self.dev_malloc(max(int(out_offs[-1]), 1) * 4)
            _check(self.lib, self.lib.wm_resample_16k_mix(self.handle, d_pcm, *args, d_out, WM_MEM_DEVICE))
            self.sync()
        except Exception:
            if d_out is not None:
                self.dev_free(d_out)
            raise
        finally:
            if d_pcm is not None:
                self.dev_free(d_pcm)
        return d_out, out_offs

    def channel_activity(self, signals, offsets=None, device=False):
        """wm_channel_activity: per signal, the f32 sum of |y| over every 160 samples (10 ms, one value per mel frame; the last
        frame may be short).  signals: a list of 16 kHz f32 arrays -- or, with device=True, the device pointer and `offsets`,
        the sample offsets i64 [S + 1], as resample_16k_mix(..., device=True) returns them (computed where the signals lie,
        then downloaded).  Returns a list of f32 [ceil(N_s / 160)] on the host."""
        if device:
            offs = np.ascontiguousarray(offsets, dtype=np.int64)
        else:
            sig = [np.ascontiguousarray(s, dtype=np.float32).reshape(-1) for s in signals]
            offs = np.concatenate([[0], np.cumsum([s.size for s in sig])]).astype(np.int64)
            pcm = np.ascontiguousarray(np.concatenate(sig) if sig else np.zeros(0, np.float32), dtype=np.float32)
        S = len(offs) - 1
        n = -(-np.diff(offs) // ACTIVITY_HOP)
        out_offs = np.concatenate([[0], np.cumsum(np.maximum(n, 0))]).astype(np.int64)
        total = max(int(out_offs[-1]), 1)
        if not device:
            act = np.empty(total, dtype=np.float32)
            _check(self.lib, self.lib.wm_channel_activity(self.handle, _ptr(pcm), _ptr(offs), S, _ptr(act), WM_MEM_HOST))
        else:
            d_act = self.dev_malloc(total * 4)
            try:
                _check(self.lib, self.lib.wm_channel_activity(self.handle, signals, _ptr(offs), S, d_act, WM_MEM_DEVICE))
                act = self.download(d_act, total, np.float32)
            finally:
                self.dev_free(d_act)
        return [act[out_offs[s]:out_offs[s + 1]] for s in range(S)]

    def vad_energy(self, mel, mel_offs, T, n_frames, band, smooth=VAD_SMOOTH, device=False, raw=False, n_mels=None):
        """wm_vad_energy: the smoothed band energy of R recordings' log-mels in one launch.  mel: logmel_long's output --
        a flat f32 array, or with device=True the device pointer; mel_offs i64 [R] and T i32 [R] as logmel_long(...,
        device=True) returns them; n_frames: the frames to do per recording (the content frames T - 3000); band = (lo,
        hi).  Returns a list of f32 [n_frames[r]] on the host (device=True: computed where the mel lies, then
        downloaded); raw=True: (the unsmoothed tracks, the smoothed ones)."""
        base = np.ascontiguousarray(mel_offs, dtype=np.int64)
        R = len(base)
        T = np.ascontiguousarray(T, dtype=np.int32)
        n = np.ascontiguousarray(n_frames, dtype=np.int32)
        if len(T) != R or len(n) != R:
            raise ValueError("vad_energy: mel_offs, T and n_frames have one entry per recording")
        offs = np.concatenate([[0], np.cumsum(np.maximum(n, 0).astype(np.int64))])
        total = max(int(offs[-1]), 1)
        lo, hi = int(band[0]), int(band[1])
        if n_mels is None:   # (a front-end-only context has no dims)
            n_mels = int(self.dims["n_mels"]) if self.dims else 80
        if not device:
            mel = np.ascontiguousarray(mel, dtype=np.float32)
            y = np.empty(total, dtype=np.float32)
            e = np.empty(total, dtype=np.float32) if raw else None
            _check(self.lib, self.lib.wm_vad_energy(self.handle, _ptr(mel), _ptr(base), _ptr(T), _ptr(n), R, n_mels, lo, hi,
                                                    int(smooth), _ptr(e) if raw else None, _ptr(y), WM_MEM_HOST))
        else:
            d_y = self.dev_malloc(total * 4 * (2 if raw else 1))
            try:
                d_e = ctypes.c_void_p(d_y.value + total * 4) if raw else None
                _check(self.lib, self.lib.wm_vad_energy(self.handle, mel, _ptr(base), _ptr(T), _ptr(n), R, n_mels, lo, hi,
                                                        int(smooth), d_e, d_y, WM_MEM_DEVICE))
                both = self.download(d_y, (2 if raw else 1, total), np.float32)
            finally:
                self.dev_free(d_y)
            y, e = both[0], (both[1] if raw else None)
        ys = [y[offs[r]:offs[r + 1]] for r in range(R)]
        return ([e[offs[r]:offs[r + 1]] for r in range(R)], ys) if raw else ys

    # ---- device memory --------------------------------------------------------------
    def dev_malloc(self, nbytes):
        p = ctypes.c_void_p()
        _check(self.lib, self.lib.wm_dev_malloc(self.handle, nbytes, ctypes.byref(p)))
        return p

    def dev_free(self, p):
        _check(self.lib, self.lib.wm_dev_free(self.handle, p))

    def upload(self, p, arr):
        arr = np.ascontiguousarray(arr)
        _check(self.lib, self.lib.wm_dev_upload(self.handle, p, _ptr(arr), arr.nbytes))

    def download(self, p, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        _check(self.lib, self.lib.wm_dev_download(self.handle, _ptr(out), p, out.nbytes))
        return out

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.dev_malloc(arr.nbytes)
        self.upload(p, arr)
        return p

    def sync(self):
        _check(self.lib, self.lib.wm_sync(self.handle))

    # ---- profiling ------------------------------------------------------------------
    def profile_enable(self, on=True):
        _check(self.lib, self.lib.wm_profile_enable(self.handle, 1 if on else 0))

    def profile_reset(self):
        _check(self.lib, self.lib.wm_profile_reset(self.handle))

    def profile(self):
        import json
        buf = ctypes.create_string_buffer(1 << 16)
        _check(self.lib, self.lib.wm_profile_json(self.handle, buf, len(buf)))
        return json.loads(buf.value.decode())

    def profile_overhead_us(self):
        v = ctypes.c_float()
        _check(self.lib, self.lib.wm_profile_overhead_us(self.handle, ctypes.byref(v)))
        return float(v.value)

    def last_stage_ms(self):
        out = np.zeros(3, dtype=np.float32)
        _check(self.lib, self.lib.wm_last_stage_ms(self.handle, _ptr(out)))
        return out

    # ---- weights --------------------------------------------------------------------
    def set_tensor(self, name, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        _check(self.lib, self.lib.wm_set_tensor(self.handle, name.encode(), _ptr(a), a.size))

    def get_tensor(self, name, shape):
        out = np.empty(shape, dtype=np.float32)
        _check(self.lib, self.lib.wm_get_tensor(self.handle, name.encode(), _ptr(out), out.size))
        return out

    def load_state_dict(self, sd):
        for k, v in sd.items():
            self.set_tensor(k, np.asarray(v, dtype=np.float32))

    def load_weights(self, path):
        _check(self.lib, self.lib.wm_load_weights(self.handle, path.encode()))

    def init_synthetic(self, seed, matrix_gain=1.0):
        """wm_init_synthetic / wm_init_synthetic_gain (matrix_gain 4: the `lively` random-init model of the token tests)."""
        if matrix_gain == 1.0:
            _check(self.lib, self.lib.wm_init_synthetic(self.handle, int(seed)))
        else:
            _check(self.lib, self.lib.wm_init_synthetic_gain(self.handle, int(seed), float(matrix_gain)))

    def set_precision(self, f32):
        """Debug library only (Context(..., debug=True)): route wm_encode / wm_decode_logits of this context through the
        all-fp32 debug model path (wmdbg_set_precision, csrc/f32_path.hip) or back to the product kernels."""
        if not hasattr(self.lib, "wmdbg_set_precision"):
            raise WhisperError(-1, "set_precision needs the debug library: Context(dims, debug=True)")
        self.lib.wmdbg_set_precision.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.lib.wmdbg_set_precision.restype = ctypes.c_int
        _check(self.lib, self.lib.wmdbg_set_precision(self.handle, WM_F32 if f32 else WM_BF16))

    def set_spec_script(self, tokens):
        """Debug library only: the proposals of the NEXT transcribe_mel_speculative call on this context come from tokens i32
        [B][max_new] (by generated index) instead of the draft (wmdbg_spec_script); None clears the hook."""
        if not hasattr(self.lib, "wmdbg_spec_script"):
            raise WhisperError(-1, "set_spec_script needs the debug library: Context(dims, debug=True)")
        self.lib.wmdbg_spec_script.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        self.lib.wmdbg_spec_script.restype = ctypes.c_int
        if tokens is None:
            self._spec_script = None
            _check(self.lib, self.lib.wmdbg_spec_script(self.handle, None, 0, 0))
            return
        self._spec_script = np.ascontiguousarray(tokens, dtype=np.int32)   # lives until the call
        B, max_new = self._spec_script.shape
        _check(self.lib, self.lib.wmdbg_spec_script(self.handle, _ptr(self._spec_script), B, max_new))

    def finalize(self):
        _check(self.lib, self.lib.wm_finalize(self.handle))

    # ---- model (host arrays) --------------------------------------------------------
    def encode_mel(self, mel):
        """wm_encode: f32 [B][n_mels][3000] -> f32 [B][n_audio_ctx][d]."""
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        B = mel.shape[0]
        xa = np.empty((B, self.dims["n_audio_ctx"], self.dims["n_audio_state"]), dtype=np.float32)
        _check(self.lib, self.lib.wm_encode(self.handle, _ptr(mel), B, _ptr(xa), WM_MEM_HOST))
        return xa

    def decode_logits(self, tokens, xa):
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        xa = np.ascontiguousarray(xa, dtype=np.float32)
        B, T = tokens.shape
        logits = np.empty((B, T, self.dims["n_vocab"]), dtype=np.float32)
        _check(self.lib, self.lib.wm_decode_logits(self.handle, _ptr(tokens), B, T, _ptr(xa),
                                                   _ptr(logits), WM_MEM_HOST))
        return logits

    def detect_language(self, xa, sot=50258, lang_first=50259, lang_last=50357):
        xa = np.ascontiguousarray(xa, dtype=np.float32)
        B = xa.shape[0]
        idx = np.empty(B, dtype=np.int32)
        _check(self.lib, self.lib.wm_detect_language(self.handle, _ptr(xa), B, sot, lang_first,
                                                     lang_last, _ptr(idx), WM_MEM_HOST))
        return idx

    def detect_language_probs(self, xa, sot=50258, lang_first=50259, lang_last=50357):
        """(lang_idx [B], probs [B][n_lang]): openai-whisper detect_language() -- softmax over the language tokens."""
        xa = np.ascontiguousarray(xa, dtype=np.float32)
        Bn = xa.shape[0]
        idx = np.empty(Bn, dtype=np.int32)
        probs = np.empty((Bn, lang_last - lang_first + 1), dtype=np.float32)
        self.lib.wm_detect_language_probs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int32,
                                                      ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_int]
        _check(self.lib, self.lib.wm_detect_language_probs(self.handle, _ptr(xa), Bn, sot, lang_first, lang_last, _ptr(idx),
                                                           _ptr(probs), WM_MEM_HOST))
        return idx, probs

    def set_suppress(self, suppress=(), suppress_first=()):
        """openai-whisper decode() logit filters for transcribe_greedy: `suppress` ids are never generated
        (SuppressTokens), `suppress_first` ids additionally not as the first generated token (SuppressBlank)."""
        a = np.ascontiguousarray(list(suppress), dtype=np.int32)
        b = np.ascontiguousarray(list(suppress_first), dtype=np.int32)
        self.lib.wm_set_suppress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        _check(self.lib, self.lib.wm_set_suppress(self.handle, _ptr(a) if a.size else None, int(a.size),
                                                  _ptr(b) if b.size else None, int(b.size)))

    def set_timestamp_rules(self, enable, timestamp_begin=0, eot=0, max_initial=-1):
        """openai-whisper ApplyTimestampRules for transcribe_greedy (decoding with timestamps)."""
        self.lib.wm_set_timestamp_rules.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                                                    ctypes.c_int32]
        _check(self.lib, self.lib.wm_set_timestamp_rules(self.handle, 1 if enable else 0, timestamp_begin, eot, max_initial))

    def set_prompt_panel(self, n):
        """wm_set_prompt_panel: positions per decoder step (1 .. MAX_TEACHER_PANEL; 1 = the default) over the prompt positions of
        a transcribe call whose logits nobody reads -- cache-only panel steps, no logits product.  A launch policy: every
        output of every entry is bit-identical for every width.  The plain groups of transcribe_greedy / transcribe /
        transcribe_mel (ragged prompts included) / transcribe_windows and their aligned forms take part; best-of, beam-search
        and speculative calls ignore it.  Inherited by later clones and by the lanes of a call."""
        self.lib.wm_set_prompt_panel.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.lib.wm_set_prompt_panel.restype = ctypes.c_int
        _check(self.lib, self.lib.wm_set_prompt_panel(self.handle, int(n)))

    def set_given_panel(self, n):
        """wm_set_given_panel: generated positions per decoder step (1 .. MAX_TEACHER_PANEL; 1 = the default) over the given tokens
        (given=, set_given_tokens) of a transcribe call.  A launch policy: every output is bit-identical for every width, and
        no call fails because of it.  Served: plain temperature-0 groups with uniform prompts and no alternatives, repetition
        rules, sequence bias or constraint; every other group steps one position at a time.  A context setting, not consumed by
        calls; inherited by later clones and by the lanes of a call."""
        self.lib.wm_set_given_panel.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.lib.wm_set_given_panel.restype = ctypes.c_int
        _check(self.lib, self.lib.wm_set_given_panel(self.handle, int(n)))

    def set_teacher_panel(self, n):
        """wm_set_teacher_panel: positions per decoder step (1 .. MAX_TEACHER_PANEL; 1 = the default) of the teacher-forced passes
        of align / align_mel / align_windows / decode_logits on this context, later clones and the lanes of a call.  A launch
        policy: the results are bit-identical for every width."""
        self.lib.wm_set_teacher_panel.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.lib.wm_set_teacher_panel.restype = ctypes.c_int
        _check(self.lib, self.lib.wm_set_teacher_panel(self.handle, int(n)))

    def set_repetition_rules(self, penalty=1.0, no_repeat_ngram_size=0, eot=0):
        """The repetition rules of every transcribe call on this context (wm_set_repetition_rules): `penalty` (> 0, 1.0 = off)
        scales the logit of every id < eot the row has generated in the call (v > 0 ? v * (1 / penalty) : v * penalty, once
        per id); `no_repeat_ngram_size` n (0 = off, 1 .. 32) bans the ids < eot that would repeat an n-gram of the row's
        generated tokens.  The prompt never counts.  The defaults switch the rules off."""
        self.lib.wm_set_repetition_rules.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int32]
        self.lib.wm_set_repetition_rules.restype = ctypes.c_int
        _check(self.lib, self.lib.wm_set_repetition_rules(self.handle, float(penalty), int(no_repeat_ngram_size), int(eot)))

    def set_sampling_rules(self, top_k=0, top_p=1.0, min_p=0.0):
        """The sampling rules of every transcribe call on this context that samples (wm_set_sampling_rules; temperature > 0):
        the distribution is truncated on the device before the draw -- `top_k` (0 = off) keeps exactly the k best admissible ids
        (ties: the lowest ids), `top_p` (1.0 = off) the shortest prefix of them holding that share of their mass, `min_p` (0.0 =
        off) the ids whose probability is at least min_p times the best one's.  Log-probs stay those of the untruncated filtered
        distribution.  Calls at temperature 0 ignore the rules.  The defaults switch them off."""
        self.lib.wm_set_sampling_rules.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float]
        self.lib.wm_set_sampling_rules.restype = ctypes.c_int
        _check(self.lib, self.lib.wm_set_sampling_rules(self.handle, int(top_k), float(top_p), float(min_p)))

    def set_sequence_bias(self, sequences=None, boost=(), eot=None):
        """The sequence bias of every transcribe call on this context (wm_set_sequence_bias; Hugging Face's sequence_bias,
        with -inf its bad_words_ids): `sequences` {tuple of token ids: bias}, in the dict's order -- the bias (finite or -inf)
        is added to the logit of a sequence's LAST token whenever the row's generated tokens end in its other tokens; the
        prompt never counts.  `boost`: the keys whose proper prefixes are biased too (finite bias), so that a phrase is
        helped from its first token on; prefixes shared by several phrases take the largest bias once.  Only ids < eot
        (default: the vocabulary size) may end a sequence.  The ids are the caller's tokenizer's: Whisper's " word" and
        "word" are different ids, both variants are the caller's to list.  None or {} switches the bias off."""
        fn = self.lib.wm_set_sequence_bias
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int32]
        fn.restype = ctypes.c_int
        eot = int(self.dims["n_vocab"]) if eot is None else int(eot)
        if not sequences:
            _check(self.lib, fn(self.handle, None, None, None, None, 0, eot))
            return
        keys = [tuple(int(t) for t in k) for k in sequences]
        marked = {tuple(int(t) for t in k) for k in boost}
        if not marked <= set(keys):
            raise ValueError("set_sequence_bias: boost names a sequence that is not in the table")
        toks = np.array([t for k in keys for t in k], dtype=np.int32)
        offs = np.zeros(len(keys) + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(k) for k in keys])
        bias = np.array([float(v) for v in sequences.values()], dtype=np.float32)
        flags = np.array([1 if k in marked else 0 for k in keys], dtype=np.uint8)
        _check(self.lib, fn(self.handle, _ptr(toks) if toks.size else None, _ptr(offs), _ptr(bias), _ptr(flags) if marked else None,
                            len(keys), eot))

    def set_sequence_bias_tables(self, tables, boosts=None, eot=None):
        """Row tables (wm_set_sequence_bias_tables): one sequence-bias table PER ROW of a call instead of one per context, so
        that requests with different phrase lists decode in one batched call.  `tables`: a list of {tuple of token ids: bias},
        each as set_sequence_bias takes it (an empty dict: a table without entries); `boosts`: per table the keys whose proper
        prefixes are biased too (None: none).  Replaces the context's single table; set_sequence_bias replaces the tables.
        Every transcribe call on the context then needs set_bias_rows in front of it.  None or [] clears the tables."""
        fn = self.lib.wm_set_sequence_bias_tables
        fn.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_int32]
        fn.restype = ctypes.c_int
        eot = int(self.dims["n_vocab"]) if eot is None else int(eot)
        if not tables:
            _check(self.lib, fn(self.handle, None, None, None, None, None, 0, eot))
            return
        boosts = [()] * len(tables) if boosts is None else list(boosts)
        if len(boosts) != len(tables):
            raise ValueError("set_sequence_bias_tables: boosts has one entry per table")
        keys, bias, flags, toffs = [], [], [], [0]
        for table, boost in zip(tables, boosts):
            own = [tuple(int(t) for t in k) for k in table]
            marked = {tuple(int(t) for t in k) for k in boost or ()}
            if not marked <= set(own):
                raise ValueError("set_sequence_bias_tables: boosts names a sequence that is not in its table")
            keys += own
            bias += [float(v) for v in table.values()]
            flags += [1 if k in marked else 0 for k in own]
            toffs.append(len(keys))
        toks = np.array([t for k in keys for t in k], dtype=np.int32)
        offs = np.zeros(len(keys) + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(k) for k in keys])
        bias = np.array(bias, dtype=np.float32)
        flags = np.array(flags, dtype=np.uint8)
        toffs = np.array(toffs, dtype=np.int32)
        _check(self.lib, fn(self.handle, _ptr(toks) if toks.size else None, _ptr(offs), _ptr(bias) if bias.size else None,
                            _ptr(flags) if flags.any() else None, _ptr(toffs), len(tables), eot))

    def set_bias_rows(self, rows):
        """The table of every row of the NEXT transcribe call (wm_set_bias_rows; len == its B; consumed by it): an index into
        the tables of set_sequence_bias_tables, or -1 (None reads as -1) for a row without a bias.  A best-of window's candidates
        and a beam window's beams use their window's table.  [] drops a pending map."""
        fn = self.lib.wm_set_bias_rows
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        fn.restype = ctypes.c_int
        a = np.ascontiguousarray([-1 if r is None else int(r) for r in rows], dtype=np.int32)
        _check(self.lib, fn(self.handle, _ptr(a) if a.size else None, int(a.size)))

    def set_constraint(self, automaton=None, eot=None):
        """The constraint of every transcribe call on this context (wm_set_constraint): a Constraint -- a token automaton that
        says which text ids (< eot) and whether eot a row may generate next, from the tokens it has generated in the call; ids
        above eot (timestamps, specials) are never banned and do not move the state.  A banned id is treated like a suppressed
        one everywhere; log-probs are those of the constrained distribution.  eot defaults to the vocabulary's last id.  Every
        row starts in state 0 unless set_constraint_rows says otherwise.  None switches the constraint off."""
        fn = self.lib.wm_set_constraint
        fn.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_int32]
        fn.restype = ctypes.c_int
        if automaton is None:
            _check(self.lib, fn(self.handle, None, None, None, None, None, 0, 0))
            return
        if not isinstance(automaton, Constraint):
            raise ValueError("set_constraint: a Constraint (constraint_from_choices, constraint_join) or None")
        eot = int(self.dims["n_vocab"]) - 1 if eot is None else int(eot)
        a = automaton
        _check(self.lib, fn(self.handle, _ptr(a.edge_beg), _ptr(a.edge_tok) if a.n_edges else None,
                            _ptr(a.edge_next) if a.n_edges else None, _ptr(a.def_next), _ptr(a.accept), a.n_states, eot))

    def set_constraint_rows(self, starts):
        """The start state of every row of the NEXT transcribe call (wm_set_constraint_rows; len == its B; consumed by it): a
        state of the automaton of set_constraint, or -1 (None reads as -1) for an unconstrained row.  A best-of window's
        candidates and a beam window's beams take their window's start.  [] drops a pending map."""
        fn = self.lib.wm_set_constraint_rows
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        fn.restype = ctypes.c_int
        a = np.ascontiguousarray([-1 if r is None else int(r) for r in starts], dtype=np.int32)
        _check(self.lib, fn(self.handle, _ptr(a) if a.size else None, int(a.size)))

    def set_sampling_rows(self, temperatures, seeds):
        """Temperature and seed of every row of the NEXT transcribe call (wm_set_sampling_rows; len == its B; consumed by it):
        that call's own temperature and seed are then not read, a row with temperature 0 is an arg-max row.  Served by
        transcribe, transcribe_mel, transcribe_windows and the two aligned wrappers (row_temperatures= / row_seeds=); refused by
        the greedy, best-of, beam-search and speculative entries.  [] and [] (or None and None) drop a pending map."""
        self._put_sampling_rows(*(sampling_rows_args(temperatures, seeds) or sampling_rows_args([], [])))

    def _put_sampling_rows(self, t, sd):
        """wm_set_sampling_rows on checked arrays (sampling_rows_args)"""
        fn = self.lib.wm_set_sampling_rows
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        fn.restype = ctypes.c_int
        _check(self.lib, fn(self.handle, _ptr(t) if t.size else None, _ptr(sd) if sd.size else None, int(t.size)))

    def set_lanes(self, n):
        """Decode groups one transcribe_greedy call keeps in flight (0: default = $WM_LANES or 3; 1: one group per call)."""
        _check(self.lib, self.lib.wm_set_lanes(self.handle, int(n)))

    def set_token_budgets(self, budgets):
        """Per-chunk token budgets of the NEXT transcribe_greedy call (len == its B; consumed by it)."""
        a = np.ascontiguousarray(list(budgets), dtype=np.int32)
        _check(self.lib, self.lib.wm_set_token_budgets(self.handle, _ptr(a) if a.size else None, int(a.size)))

    def request_alternatives(self, n, rows, max_new, entropy=True):
        """Top-n alternatives and entropy per generated token of the NEXT transcribe call on this context
        (wm_request_alternatives; consumed by it whatever happens): `rows` hypotheses (the call's B, or B * best_of) of max_new
        tokens, n in 1 .. MAX_ALTERNATIVES.  Returns the Alternatives whose arrays that call fills; the context keeps them alive
        until the next request.  n None drops a pending request."""
        fn = self.lib.wm_request_alternatives
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        fn.restype = ctypes.c_int
        if n is None:
            _check(self.lib, fn(self.handle, None))
            self._alt_request = None
            return None
        a = Alternatives(n, rows, max_new, entropy)
        req = wm_alternatives_out(a.n, a.rows, a.max_new, _ptr(a.tokens).value, _ptr(a.logprobs).value, _ptr(a.counts).value,
                                  _ptr(a.entropy).value if a.entropy is not None else None)
        self._alt_request = (a, req)
        _check(self.lib, fn(self.handle, ctypes.byref(req)))
        return a

    def set_given_tokens(self, given):
        """Given tokens of the NEXT transcribe call on this context (wm_set_given_tokens; consumed by it whatever happens): one id
        list per hypothesis row of that call (B, or B * best_of in the order [B][best_of]); the row takes them in place of its
        own choices and returns their log-probs, and decodes freely behind them (an empty list: an ordinary row).  None or []
        drops a pending table."""
        if given is None or len(given) == 0:
            self._put_given(None)
        else:
            self._put_given(given_arg(given))

    def _put_given(self, table):
        """wm_set_given_tokens on a checked table (given_arg); None: drop"""
        fn = self.lib.wm_set_given_tokens
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        fn.restype = ctypes.c_int
        if table is None:
            _check(self.lib, fn(self.handle, None, 0, None, 0))
            return
        tok, lens = table
        _check(self.lib, fn(self.handle, _ptr(tok), int(tok.shape[1]), _ptr(lens), int(lens.size)))

    def transcribe_greedy(self, pcm, prompt, max_new, eot=-1, mem=WM_MEM_HOST, pcm_dtype=None, B=None, budgets=None):
        """pcm: host array [B][480000] (int16/float32/float64), or a device pointer
        (c_void_p) with pcm_dtype and B given when mem == WM_MEM_DEVICE.  budgets: per-chunk token budgets
        (wm_set_token_budgets) for this call."""
        if budgets is not None:
            self.set_token_budgets(budgets)
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        if mem == WM_MEM_HOST:
            pcm = np.ascontiguousarray(pcm)
            B = pcm.shape[0]
            pcm_dtype = _DTYPES[pcm.dtype]
            p = _ptr(pcm)
        else:
            p = pcm
        toks = np.empty((B, max_new), dtype=np.int32)
        lens = np.empty(B, dtype=np.int32)
        _check(self.lib, self.lib.wm_transcribe_greedy(self.handle, p, pcm_dtype, B, _ptr(prompt),
                                                       len(prompt), max_new, eot, _ptr(toks),
                                                       _ptr(lens), mem))
        return toks, lens

    def transcribe_raw(self, pcm, prompt, max_new, eot=-1, opts=None, logprobs=True, no_speech=False, budgets=None,
                       alternatives=None, given=None):
        """wm_transcribe on host arrays: opts a wm_decode_opts or None (NULL); logprobs / no_speech request the two
        optional outputs.  Returns (tokens, lens, logprobs or None, no_speech_prob or None) -- and, with alternatives=n, the
        call's Alternatives as a fifth element.  given: the call's given tokens (given_arg), armed right in front of the call."""
        n_alt = alternatives_arg(alternatives)
        g = given_arg(given)
        if budgets is not None:
            self.set_token_budgets(budgets)
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        pcm = np.ascontiguousarray(pcm)
        B = pcm.shape[0]
        toks = np.empty((B, max_new), dtype=np.int32)
        lens = np.empty(B, dtype=np.int32)
        lp = np.empty((B, max_new), dtype=np.float32) if logprobs else None
        ns = np.empty(B, dtype=np.float32) if no_speech else None
        alt = self.request_alternatives(n_alt, B, max_new) if n_alt else None   # (last: nothing can fail between it and the call)
        if g is not None:
            self._put_given(g)
        _check(self.lib, self.lib.wm_transcribe(self.handle, _ptr(pcm), _DTYPES[pcm.dtype], B, _ptr(prompt), len(prompt),
                                                max_new, eot, ctypes.byref(opts) if opts is not None else None,
                                                _ptr(toks), _ptr(lens), _ptr(lp) if lp is not None else None,
                                                _ptr(ns) if ns is not None else None, WM_MEM_HOST))
        return (toks, lens, lp, ns) if alt is None else (toks, lens, lp, ns, alt)

    def transcribe(self, pcm, prompt, max_new, eot=-1, temperature=0.0, seed=0, no_speech_token=-1, sot_index=0,
                   budgets=None, alternatives=None, row_temperatures=None, row_seeds=None, given=None):
        """wm_transcribe: greedy (temperature 0) or sampled decode with per-token log-probs and, with no_speech_token >= 0,
        openai-whisper's no_speech_prob.  alternatives=n: also the n best admissible tokens and the entropy of every generated
        position (request_alternatives).  row_temperatures / row_seeds (both or neither): a temperature and a seed per row
        (set_sampling_rows in front of the call; temperature and seed are then not read).  given: one id list per row that
        the row decodes in place of its own choices, with their log-probs (set_given_tokens).  Returns a TranscribeResult."""
        opts = wm_decode_opts(float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF, int(no_speech_token), int(sot_index))
        with self._rows_map(row_temperatures, row_seeds):
            toks, lens, lp, ns, *alt = self.transcribe_raw(pcm, prompt, max_new, eot, opts, logprobs=True,
                                                           no_speech=no_speech_token >= 0, budgets=budgets, alternatives=alternatives,
                                                           given=given)
        return self._with_alternatives(TranscribeResult(toks, lens, lp, ns, eot), alt)

    @contextlib.contextmanager
    def _rows_map(self, row_temperatures, row_seeds):
        """row_temperatures / row_seeds of a wrapper around its call: the map is set on entry (both None: no library call is
        made at all), and whatever raises between there and the C call -- an argument check in Python -- drops it again, so
        that it cannot stay pending for a later, unrelated call.  (A C call that fails has consumed it; dropping twice is harmless.)"""
        rows = sampling_rows_args(row_temperatures, row_seeds)
        if rows is None:
            yield
            return
        self._put_sampling_rows(*rows)
        try:
            yield
        except BaseException:
            try:
                self.set_sampling_rows([], [])
            except WhisperError:
                pass
            raise

    @staticmethod
    def _with_alternatives(result, alt):
        """`result` with the Alternatives of a raw call's optional fifth element (alt: [] or [Alternatives]) attached"""
        return alt[0].attach(result) if alt else result

    def transcribe_with_fallback(self, pcm, prompt, max_new, eot, temperatures=FALLBACK_TEMPERATURES,
                                 compression_ratio_threshold="auto", logprob_threshold=-1.0, no_speech_threshold=0.6,
                                 vocab=None, seed=0, no_speech_token=-1, sot_index=0, best_of=None, length_penalty=None,
                                 beam_size=None, patience=None, top_k=None, top_p=None, min_p=None, alternatives=None):
        """openai-whisper's temperature fallback (module function transcribe_with_fallback) on this context."""
        return transcribe_with_fallback(self, pcm, prompt, max_new, eot, temperatures, compression_ratio_threshold,
                                        logprob_threshold, no_speech_threshold, vocab, seed, no_speech_token, sot_index,
                                        best_of=best_of, length_penalty=length_penalty, beam_size=beam_size, patience=patience,
                                        top_k=top_k, top_p=top_p, min_p=min_p, alternatives=alternatives)

    def _mel_rows(self, mel, mel_base, mel_len, seek, n_frames, mem):
        """(the arguments that name the B rows of a wm_*_mel* call, each keeping its array alive; B)"""
        mel, mp, base, mlen, sk, nf, B = self._window_arrays(mel, mel_base, mel_len, seek, n_frames, mem)
        return (mp, _ptr(base), _ptr(mlen), _ptr(sk), _ptr(nf)), B

    @staticmethod
    def _window_arrays(mel, mel_base, mel_len, seek, n_frames, mem):
        """The window description of transcribe_mel_raw as a call takes it: (mel kept alive, its pointer, mel_base i64 [B],
        mel_len, seek, n_frames i32 broadcast to [B], B)."""
        base = np.ascontiguousarray(mel_base, dtype=np.int64)
        B = base.size
        mlen, sk, nf = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.int32), (B,)))
                        for x in (mel_len, seek, n_frames))
        if mem == WM_MEM_HOST:
            mel = np.ascontiguousarray(mel, dtype=np.float32)
        return mel, _ptr(mel) if mem == WM_MEM_HOST else mel, base, mlen, sk, nf, B

    @staticmethod
    def _prompt_call_args(B, prompts, opts, sample_ids, prompt_len, sot_tail):
        """The prompt arrays of a B-row wm_transcribe_mel* / wm_transcribe_windows* call: (prompts [B][stride], prompt_len or
        None, opts, sample_ids or None)."""
        plen = None
        if prompt_len is not None:
            plen = np.ascontiguousarray(prompt_len, dtype=np.int32)
        elif not isinstance(prompts, np.ndarray) and len(prompts) > 0 and np.ndim(prompts[0]) == 1 \
                and len({len(p) for p in prompts}) > 1:
            plen = np.array([len(p) for p in prompts], dtype=np.int32)
            padded = np.zeros((len(prompts), int(plen.max())), dtype=np.int32)
            for i, p in enumerate(prompts):
                padded[i, :len(p)] = np.asarray(p, dtype=np.int32)
            prompts = padded
        pr = np.ascontiguousarray(prompts, dtype=np.int32)
        if pr.ndim == 1:
            pr = np.ascontiguousarray(np.broadcast_to(pr, (B, pr.size)))
        if plen is None and sot_tail is not None and opts is not None:
            opts = wm_decode_opts(opts.temperature, opts.seed, opts.no_speech_token, pr.shape[1] - int(sot_tail))
        ids = None if sample_ids is None else np.ascontiguousarray(sample_ids, dtype=np.uint32)
        if plen is not None and plen.shape != (B,):
            raise ValueError("prompt_len: one length per row")
        return pr, plen, opts, ids

    def transcribe_mel_raw(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, eot=-1, opts=None,
                           sample_ids=None, logprobs=True, no_speech=False, mem=WM_MEM_HOST, budgets=None, prompt_len=None,
                           sot_tail=None, alternatives=None, given=None):
        """wm_transcribe_mel: mel is a host f32 array (mem WM_MEM_HOST) or a device pointer (WM_MEM_DEVICE); mel_base i64,
        mel_len / seek / n_frames i32 [B]; prompts [B][n_prompt]; sample_ids u32 [B] or None.  Returns (tokens, lens,
        logprobs or None, no_speech_prob or None).
        Prompts of different lengths -- a list of B lists, or prompts [B][stride] with prompt_len i32 [B] -- go to
        wm_transcribe_mel_ragged with sot_tail (<|startoftranscript|> is the sot_tail-th token from the end of every
        prompt; default 1, opts.sot_index is not read).  A list of lists of ONE length without prompt_len stays
        wm_transcribe_mel; there a sot_tail, when given, replaces opts.sot_index by n_prompt - sot_tail.
        alternatives=n: the call's Alternatives as a fifth element (request_alternatives).  given: the call's given tokens
        (given_arg), armed right in front of the call."""
        n_alt = alternatives_arg(alternatives)
        g = given_arg(given)
        if budgets is not None:
            self.set_token_budgets(budgets)
        head, B = self._mel_rows(mel, mel_base, mel_len, seek, n_frames, mem)
        pr, plen, opts, ids = self._prompt_call_args(B, prompts, opts, sample_ids, prompt_len, sot_tail)
        toks = np.empty((B, max_new), dtype=np.int32)
        lens = np.empty(B, dtype=np.int32)
        lp = np.empty((B, max_new), dtype=np.float32) if logprobs else None
        ns = np.empty(B, dtype=np.float32) if no_speech else None
        rows = (self.handle, *head, B, _ptr(pr), pr.shape[1])
        rest = (_ptr_or_null(ids), max_new, eot, ctypes.byref(opts) if opts is not None else None, _ptr(toks), _ptr(lens),
                _ptr_or_null(lp), _ptr_or_null(ns), mem)
        alt = self.request_alternatives(n_alt, B, max_new) if n_alt else None
        if g is not None:
            self._put_given(g)
        if plen is not None:
            _check(self.lib, self.lib.wm_transcribe_mel_ragged(*rows, _ptr(plen), 1 if sot_tail is None else int(sot_tail), *rest))
        else:
            _check(self.lib, self.lib.wm_transcribe_mel(*rows, *rest))
        return (toks, lens, lp, ns) if alt is None else (toks, lens, lp, ns, alt)

    def transcribe_mel_speculative(self, draft, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, draft_len, eot=-1,
                                   temperature=0.0, no_speech_token=-1, sot_index=0, mem=WM_MEM_HOST, budgets=None):
        """wm_transcribe_mel_speculative: transcribe_mel's uniform-prompt call at temperature 0 whose tokens the Context
        `draft` (same device, same vocabulary; its own suppress lists and timestamp rules set as on this one) proposes
        draft_len at a time and panels of this context verify.  The TranscribeResult is transcribe_mel's bit for bit; the
        returned SpeculativeResult adds the per-window statistics."""
        opts = wm_decode_opts(float(temperature), 0, int(no_speech_token), int(sot_index))
        head, B = self._mel_rows(mel, mel_base, mel_len, seek, n_frames, mem)
        pr, plen, opts, _ = self._prompt_call_args(B, prompts, opts, None, None, None)
        if plen is not None:   # (before the budgets are set: a rejected call leaves none behind)
            raise ValueError("speculative decoding takes prompts of one length")
        if budgets is not None:
            self.set_token_budgets(budgets)
        toks = np.empty((B, max_new), dtype=np.int32)
        lens = np.empty(B, dtype=np.int32)
        lp = np.empty((B, max_new), dtype=np.float32)
        ns = np.empty(B, dtype=np.float32) if no_speech_token >= 0 else None
        stats = np.zeros((B, 4), dtype=np.int32)
        _check(self.lib, self.lib.wm_transcribe_mel_speculative(
            self.handle, draft.handle if draft is not None else None, *head, B, _ptr(pr), pr.shape[1], int(draft_len), max_new, eot,
            ctypes.byref(opts), _ptr(toks), _ptr(lens), _ptr(lp), _ptr_or_null(ns), _ptr(stats), mem))
        return SpeculativeResult(toks, lens, lp, ns, eot, stats)

    def transcribe_mel_best_of(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, best_of, eot=-1, temperature=0.0,
                               seed=0, no_speech_token=-1, sot_index=0, sample_ids=None, mem=WM_MEM_HOST, budgets=None,
                               prompt_len=None, sot_tail=None, length_penalty=None, alternatives=None, given=None):
        """wm_transcribe_mel_best_of: transcribe_mel's arguments (uniform or ragged prompts as in transcribe_mel_raw) with
        best_of sampled candidates per row that share the row's encoder pass and cross-attention cache; length_penalty None
        is openai-whisper's None.  alternatives=n: every candidate's alternatives and entropy.  given: B * best_of id lists in the
        order [B][best_of] (set_given_tokens): a given candidate never draws.  Returns a BestOfResult."""
        return self._best_of_call(self.lib.wm_transcribe_mel_best_of,
                                  lambda: self._mel_rows(mel, mel_base, mel_len, seek, n_frames, mem), (mem,), prompts, max_new,
                                  best_of, eot, temperature, seed, no_speech_token, sot_index, sample_ids, budgets, prompt_len,
                                  sot_tail, length_penalty, alternatives=alternatives, given=given)

    def _best_of_call(self, fn, rows, tail, prompts, max_new, best_of, eot, temperature, seed, no_speech_token, sot_index,
                      sample_ids, budgets, prompt_len, sot_tail, length_penalty, aligned=None, alternatives=None, given=None):
        """wm_transcribe_mel_best_of / wm_transcribe_windows, which differ in the arguments that name the rows -- rows() gives
        (them, B): _mel_rows, _window_rows -- and in the tail (mem).  aligned = (medfilt_width, qk_scale, capture_matrix): fn is
        the aligned counterpart, and the result carries start_frames (and matrix).  alternatives: None or n (every candidate's)."""
        n_alt = alternatives_arg(alternatives)
        g = given_arg(given)   # (the aligned best-of wrappers take none: those entries refuse a table)
        opts = wm_decode_opts(float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF, int(no_speech_token), int(sot_index))
        if budgets is not None:
            self.set_token_budgets(budgets)
        head, B = rows()
        pr, plen, opts, ids = self._prompt_call_args(B, prompts, opts, sample_ids, prompt_len, sot_tail)
        N = int(best_of)
        shape = (B, max(N, 1), max_new)
        toks = np.empty(shape, dtype=np.int32)
        lens = np.empty(shape[:2], dtype=np.int32)
        lp = np.empty(shape, dtype=np.float32)
        ns = np.empty(B, dtype=np.float32) if no_speech_token >= 0 else None
        best = np.empty(B, dtype=np.int32)
        align_in, align_out, start, matrix = self._hyp_aligned_args(aligned, B, max_new)
        alt = self.request_alternatives(n_alt, B * max(N, 1), max_new) if n_alt else None
        if g is not None:
            self._put_given(g)
        _check(self.lib, fn(self.handle, *head, B, _ptr(pr), pr.shape[1], _ptr_or_null(plen),
                            1 if sot_tail is None else int(sot_tail), _ptr_or_null(ids), N,
                            float("nan") if length_penalty is None else float(length_penalty), max_new, eot, ctypes.byref(opts),
                            *align_in, _ptr(toks), _ptr(lens), _ptr(lp), _ptr_or_null(ns), _ptr(best), *align_out, *tail))
        r = BestOfResult(toks, lens, lp, ns, best, eot, alternatives=alt)
        if aligned is not None:
            r.start_frames, r.matrix = start, matrix
        return r

    def _hyp_aligned_args(self, aligned, B, max_new):
        """What an aligned best-of / beam entry takes beyond its plain counterpart: ((medfilt_width, qk_scale) behind opts,
        (start_frame_out,) behind best_out, start_frames i32 [B][max_new + 1], the captured matrix or None); all empty / None for
        the plain entry."""
        if aligned is None:
            return (), (), None, None
        medfilt_width, qk_scale, capture_matrix = aligned
        start = np.empty((B, max_new + 1), dtype=np.int32)
        matrix = self._capture_matrix(B, max_new) if capture_matrix else None
        return (int(medfilt_width), float(qk_scale)), (_ptr(start),), start, matrix

    def transcribe_mel_beam(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, beam_size, eot=-1, patience=None,
                            no_speech_token=-1, sot_index=0, mem=WM_MEM_HOST, budgets=None, prompt_len=None, sot_tail=None,
                            length_penalty=None, max_candidates=None):
        """wm_transcribe_mel_beam: transcribe_mel's arguments (uniform or ragged prompts as in transcribe_mel_raw) decoded by
        beam search with beam_size beams per row that share the row's encoder pass and cross-attention cache; max_candidates
        defaults to openai-whisper's round(beam_size * patience) (patience None = 1.0); length_penalty None is
        openai-whisper's None.  Returns a BeamResult."""
        return self._beam_call(self.lib.wm_transcribe_mel_beam, lambda: self._mel_rows(mel, mel_base, mel_len, seek, n_frames, mem),
                               (mem,), prompts, max_new, beam_size, eot, patience, no_speech_token, sot_index, budgets, prompt_len,
                               sot_tail, length_penalty, max_candidates)

    def _beam_call(self, fn, rows, tail, prompts, max_new, beam_size, eot, patience, no_speech_token, sot_index, budgets,
                   prompt_len, sot_tail, length_penalty, max_candidates, aligned=None):
        """wm_transcribe_mel_beam / wm_transcribe_windows_beam (rows, tail, aligned: as in _best_of_call)"""
        if max_candidates is None:
            max_candidates = beam_max_candidates(beam_size, patience)
        elif patience is not None:
            raise ValueError("give patience or max_candidates, not both")
        opts = wm_decode_opts(0.0, 0, int(no_speech_token), int(sot_index))
        if budgets is not None:
            self.set_token_budgets(budgets)
        head, B = rows()
        pr, plen, opts, _ = self._prompt_call_args(B, prompts, opts, None, prompt_len, sot_tail)
        N, C = int(beam_size), int(max_candidates)
        shape = (B, max(N, C, 1), max_new)
        toks = np.empty(shape, dtype=np.int32)
        lens = np.empty(shape[:2], dtype=np.int32)
        n_hyp = np.empty(B, dtype=np.int32)
        sums = np.empty(shape[:2], dtype=np.float32)
        lp = np.empty(shape, dtype=np.float32)
        ns = np.empty(B, dtype=np.float32) if no_speech_token >= 0 else None
        best = np.empty(B, dtype=np.int32)
        align_in, align_out, start, matrix = self._hyp_aligned_args(aligned, B, max_new)
        _check(self.lib, fn(self.handle, *head, B, _ptr(pr), pr.shape[1], _ptr_or_null(plen),
                            1 if sot_tail is None else int(sot_tail), N, C,
                            float("nan") if length_penalty is None else float(length_penalty), max_new, eot, ctypes.byref(opts),
                            *align_in, _ptr(toks), _ptr(lens), _ptr(n_hyp), _ptr(sums), _ptr(lp), _ptr_or_null(ns), _ptr(best),
                            *align_out, *tail))
        r = BeamResult(toks, lens, n_hyp, sums, lp, ns, best, eot)
        if aligned is not None:
            r.start_frames, r.matrix = start, matrix
        return r

    def transcribe_mel(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, eot=-1, temperature=0.0, seed=0,
                       no_speech_token=-1, sot_index=0, sample_ids=None, mem=WM_MEM_HOST, budgets=None, prompt_len=None,
                       sot_tail=None, best_of=None, length_penalty=None, beam_size=None, patience=None, alternatives=None,
                       row_temperatures=None, row_seeds=None, given=None):
        """wm_transcribe_mel with log-probs (and no_speech_prob with no_speech_token >= 0).  Returns a TranscribeResult.
        row_temperatures / row_seeds (both or neither; not with best_of or beam_size): a temperature and a seed per row
        (set_sampling_rows in front of the call; temperature and seed are then not read).
        alternatives=n: also the n best admissible tokens and the entropy of every generated position (not with beam_size).
        given: one id list per row (B * best_of with best_of) that the row decodes in place of its own choices (set_given_tokens;
        not with beam_size).
        Prompts of different lengths (or prompt_len=) and sot_tail: see transcribe_mel_raw.
        best_of (None: one sample): transcribe_mel_best_of, and the result is its `selected` (with `candidate`).
        beam_size (None: no beam search; with patience): transcribe_mel_beam at temperature 0 -- sample_ids and the seed play
        no part -- and the result is its `selected` (with `hypothesis`)."""
        alternatives_arg(alternatives, beam_size if beam_size is not None else patience)
        given_arg(given, beam_size if beam_size is not None else patience)
        win = (mel, mel_base, mel_len, seek, n_frames, prompts, max_new)
        common = dict(mem=mem, budgets=budgets, prompt_len=prompt_len, sot_tail=sot_tail)
        entry = dict(common, eot=eot, no_speech_token=no_speech_token, sot_index=sot_index, length_penalty=length_penalty)

        self._rows_entry(row_temperatures, row_seeds, best_of, beam_size, patience)

        def plain():
            with self._rows_map(row_temperatures, row_seeds):
                toks, lens, lp, ns, *alt = self.transcribe_mel_raw(
                    *win, eot, wm_decode_opts(float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF, int(no_speech_token), int(sot_index)),
                    sample_ids, logprobs=True, no_speech=no_speech_token >= 0, alternatives=alternatives, given=given, **common)
            return self._with_alternatives(TranscribeResult(toks, lens, lp, ns, eot), alt)
        return self._decode_entry(
            lambda: self.transcribe_mel_beam(*win, beam_size, patience=patience, **entry),
            lambda: self.transcribe_mel_best_of(*win, best_of, temperature=temperature, seed=seed, sample_ids=sample_ids,
                                                alternatives=alternatives, given=given, **entry),
            plain, temperature, best_of, beam_size, patience)

    @staticmethod
    def _rows_entry(row_temperatures, row_seeds, best_of, beam_size, patience):
        """a row map goes with the plain entry alone (checked before any library call)"""
        if sampling_rows_args(row_temperatures, row_seeds) is not None and (best_of is not None or beam_size is not None or
                                                                            patience is not None):
            raise ValueError("row_temperatures / row_seeds cannot be combined with best_of or beam_size")

    @staticmethod
    def _decode_entry(beam, candidates, plain, temperature, best_of, beam_size, patience):
        """transcribe_mel's / transcribe_windows' choice of entry, each a callable; beam search and best-of give `selected`"""
        if beam_size is not None or patience is not None:
            if best_of is not None:
                raise ValueError("beam_size and best_of exclude each other (openai-whisper)")
            if temperature != 0:
                raise ValueError("beam search decodes at temperature 0")
            beam_max_candidates(beam_size, patience)
            return beam().selected
        if best_of is not None:
            return candidates().selected
        return plain()

    # ---- window sets ----------------------------------------------------------------
    def encode_windows(self, mel, mel_base, mel_len, seek, n_frames, mem=WM_MEM_HOST):
        """wm_windows_encode: run the encoder and the cross-K/V projection of the windows ONCE (the window description of
        transcribe_mel_raw) and keep the result on the device.  Returns a Windows; close it before this context."""
        mel, mp, base, mlen, sk, nf, W = self._window_arrays(mel, mel_base, mel_len, seek, n_frames, mem)
        h = ctypes.c_void_p()
        _check(self.lib, self.lib.wm_windows_encode(self.handle, mp, _ptr(base), _ptr(mlen), _ptr(sk), _ptr(nf), W, mem,
                                                    ctypes.byref(h)))
        return Windows(self, h, nf.copy())

    @staticmethod
    def _window_rows(windows, rows):
        """(the arguments that name the B rows of a call that reads a set -- the set, rows i32 [B] or NULL: all --, B)"""
        if rows is None:
            return (windows.handle, None), len(windows)
        r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        return (windows.handle, _ptr(r)), int(r.size)

    def transcribe_windows_best_of(self, windows, rows, prompts, max_new, best_of=1, eot=-1, temperature=0.0, seed=0,
                                   no_speech_token=-1, sot_index=0, sample_ids=None, budgets=None, prompt_len=None,
                                   sot_tail=None, length_penalty=None, alternatives=None, given=None):
        """wm_transcribe_windows: transcribe_mel_best_of with rows of a Windows set (rows None: all of them, in order) in
        place of the mel windows.  Same bits.  Returns a BestOfResult."""
        return self._best_of_call(self.lib.wm_transcribe_windows, lambda: self._window_rows(windows, rows), (), prompts, max_new,
                                  best_of, eot, temperature, seed, no_speech_token, sot_index, sample_ids, budgets, prompt_len,
                                  sot_tail, length_penalty, alternatives=alternatives, given=given)

    def transcribe_windows_beam(self, windows, rows, prompts, max_new, beam_size, eot=-1, patience=None, no_speech_token=-1,
                                sot_index=0, budgets=None, prompt_len=None, sot_tail=None, length_penalty=None,
                                max_candidates=None):
        """wm_transcribe_windows_beam: transcribe_mel_beam with rows of a Windows set.  Same bits.  Returns a BeamResult."""
        return self._beam_call(self.lib.wm_transcribe_windows_beam, lambda: self._window_rows(windows, rows), (), prompts, max_new,
                               beam_size, eot, patience, no_speech_token, sot_index, budgets, prompt_len, sot_tail, length_penalty,
                               max_candidates)

    def transcribe_windows(self, windows, rows, prompts, max_new, eot=-1, temperature=0.0, seed=0, no_speech_token=-1,
                           sot_index=0, sample_ids=None, budgets=None, prompt_len=None, sot_tail=None, best_of=None,
                           length_penalty=None, beam_size=None, patience=None, alternatives=None, row_temperatures=None,
                           row_seeds=None, given=None):
        """transcribe_mel with rows of a Windows set in place of the mel windows: the same bits, no encoder pass.  Returns a
        TranscribeResult (best_of / beam_size: the `selected` one, as transcribe_mel; alternatives=n, given= and row_temperatures /
        row_seeds as there)."""
        alternatives_arg(alternatives, beam_size if beam_size is not None else patience)
        given_arg(given, beam_size if beam_size is not None else patience)
        self._rows_entry(row_temperatures, row_seeds, best_of, beam_size, patience)
        common = dict(eot=eot, no_speech_token=no_speech_token, sot_index=sot_index, budgets=budgets, prompt_len=prompt_len,
                      sot_tail=sot_tail, length_penalty=length_penalty)

        def candidates(n):
            return self.transcribe_windows_best_of(windows, rows, prompts, max_new, n, temperature=temperature, seed=seed,
                                                   sample_ids=sample_ids, alternatives=alternatives, given=given, **common)

        def plain():   # (the set has no entry of its own for one sample: candidate 0 of N = 1)
            with self._rows_map(row_temperatures, row_seeds):
                r = candidates(1)
            t = TranscribeResult(np.ascontiguousarray(r.tokens[:, 0]), np.ascontiguousarray(r.lens[:, 0]),
                                 np.ascontiguousarray(r.logprobs[:, 0]), r.no_speech_prob, eot)
            if r.alt_tokens is not None:
                t.alt_tokens, t.alt_logprobs, t.alt_counts = (np.ascontiguousarray(a[:, 0]) for a in
                                                              (r.alt_tokens, r.alt_logprobs, r.alt_counts))
                t.entropy = None if r.entropy is None else np.ascontiguousarray(r.entropy[:, 0])
            return t
        return self._decode_entry(
            lambda: self.transcribe_windows_beam(windows, rows, prompts, max_new, beam_size, patience=patience, **common),
            lambda: candidates(best_of), plain, temperature, best_of, beam_size, patience)

    def _aligned_call(self, fn, rows, tail, prompts, max_new, eot, temperature, seed, no_speech_token, sot_index, sample_ids,
                      budgets, prompt_len, sot_tail, medfilt_width, qk_scale, capture_matrix, alternatives=None, row_temperatures=None,
                      row_seeds=None, given=None):
        """wm_transcribe_mel_aligned / wm_transcribe_windows_aligned (rows, tail: as in _best_of_call)"""
        n_alt = alternatives_arg(alternatives)
        g = given_arg(given)
        with self._rows_map(row_temperatures, row_seeds):
            opts = wm_decode_opts(float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF, int(no_speech_token), int(sot_index))
            if budgets is not None:
                self.set_token_budgets(budgets)
            head, B = rows()
            pr, plen, opts, ids = self._prompt_call_args(B, prompts, opts, sample_ids, prompt_len, sot_tail)
            toks = np.empty((B, max_new), dtype=np.int32)
            lens = np.empty(B, dtype=np.int32)
            lp = np.empty((B, max_new), dtype=np.float32)
            ns = np.empty(B, dtype=np.float32) if no_speech_token >= 0 else None
            start = np.empty((B, max_new + 1), dtype=np.int32)
            matrix = self._capture_matrix(B, max_new) if capture_matrix else None
            alt = self.request_alternatives(n_alt, B, max_new) if n_alt else None
            if g is not None:
                self._put_given(g)
            _check(self.lib, fn(self.handle, *head, B, _ptr(pr), pr.shape[1], _ptr_or_null(plen),
                                1 if sot_tail is None else int(sot_tail), _ptr_or_null(ids), max_new, eot, ctypes.byref(opts),
                                int(medfilt_width), float(qk_scale), _ptr(toks), _ptr(lens), _ptr(lp), _ptr_or_null(ns), _ptr(start),
                                *tail))
        r = AlignedResult(toks, lens, lp, ns, eot, start, matrix)
        return r if alt is None else alt.attach(r)

    def transcribe_mel_aligned(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, eot=-1, temperature=0.0, seed=0,
                               no_speech_token=-1, sot_index=0, sample_ids=None, mem=WM_MEM_HOST, budgets=None, prompt_len=None,
                               sot_tail=None, medfilt_width=7, qk_scale=1.0, capture_matrix=False, alternatives=None,
                               row_temperatures=None, row_seeds=None, given=None):
        """wm_transcribe_mel_aligned: transcribe_mel (one sample per row; uniform or ragged prompts as in transcribe_mel_raw)
        whose decode also aligns what it generates, from its own cross-attention queries.  Tokens, lens, log-probs and
        no_speech_prob are transcribe_mel's bit for bit.  Returns an AlignedResult (start_frames; decode_alignment_text turns
        a row into word_timestamps' arrays); capture_matrix=True (debug library) also keeps the cost matrices."""
        return self._aligned_call(self.lib.wm_transcribe_mel_aligned,
                                  lambda: self._mel_rows(mel, mel_base, mel_len, seek, n_frames, mem), (mem,), prompts, max_new, eot,
                                  temperature, seed, no_speech_token, sot_index, sample_ids, budgets, prompt_len, sot_tail,
                                  medfilt_width, qk_scale, capture_matrix, alternatives=alternatives,
                                  row_temperatures=row_temperatures, row_seeds=row_seeds, given=given)

    def transcribe_windows_aligned(self, windows, rows, prompts, max_new, eot=-1, temperature=0.0, seed=0, no_speech_token=-1,
                                   sot_index=0, sample_ids=None, budgets=None, prompt_len=None, sot_tail=None, medfilt_width=7,
                                   qk_scale=1.0, capture_matrix=False, alternatives=None, row_temperatures=None, row_seeds=None,
                                   given=None):
        """wm_transcribe_windows_aligned: transcribe_mel_aligned with rows of a Windows set.  Same bits."""
        return self._aligned_call(self.lib.wm_transcribe_windows_aligned, lambda: self._window_rows(windows, rows), (), prompts,
                                  max_new, eot, temperature, seed, no_speech_token, sot_index, sample_ids, budgets, prompt_len,
                                  sot_tail, medfilt_width, qk_scale, capture_matrix, alternatives=alternatives,
                                  row_temperatures=row_temperatures, row_seeds=row_seeds, given=given)

    def transcribe_mel_best_of_aligned(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, best_of, eot=-1,
                                       temperature=0.0, seed=0, no_speech_token=-1, sot_index=0, sample_ids=None, mem=WM_MEM_HOST,
                                       budgets=None, prompt_len=None, sot_tail=None, length_penalty=None, medfilt_width=7,
                                       qk_scale=1.0, capture_matrix=False, alternatives=None):
        """wm_transcribe_mel_best_of_aligned: transcribe_mel_best_of whose decode also aligns, per row, the candidate best[b]
        from its own cross-attention queries.  Every field of the BestOfResult is transcribe_mel_best_of's bit for bit; it also
        carries start_frames i32 [B][max_new + 1] of candidate best[b] (as AlignedResult's; decode_alignment_text takes
        selected.tokens[b], selected.lens[b], start_frames[b], selected.logprobs[b]) and matrix (capture_matrix=True, debug
        library; else None)."""
        return self._best_of_call(self.lib.wm_transcribe_mel_best_of_aligned,
                                  lambda: self._mel_rows(mel, mel_base, mel_len, seek, n_frames, mem), (mem,), prompts, max_new,
                                  best_of, eot, temperature, seed, no_speech_token, sot_index, sample_ids, budgets, prompt_len,
                                  sot_tail, length_penalty, aligned=(medfilt_width, qk_scale, capture_matrix), alternatives=alternatives)

    def transcribe_windows_best_of_aligned(self, windows, rows, prompts, max_new, best_of=1, eot=-1, temperature=0.0, seed=0,
                                           no_speech_token=-1, sot_index=0, sample_ids=None, budgets=None, prompt_len=None,
                                           sot_tail=None, length_penalty=None, medfilt_width=7, qk_scale=1.0,
                                           capture_matrix=False, alternatives=None):
        """wm_transcribe_windows_best_of_aligned: transcribe_mel_best_of_aligned with rows of a Windows set.  Same bits."""
        return self._best_of_call(self.lib.wm_transcribe_windows_best_of_aligned, lambda: self._window_rows(windows, rows), (),
                                  prompts, max_new, best_of, eot, temperature, seed, no_speech_token, sot_index, sample_ids, budgets,
                                  prompt_len, sot_tail, length_penalty, aligned=(medfilt_width, qk_scale, capture_matrix),
                                  alternatives=alternatives)

    def transcribe_mel_beam_aligned(self, mel, mel_base, mel_len, seek, n_frames, prompts, max_new, beam_size, eot=-1, patience=None,
                                    no_speech_token=-1, sot_index=0, mem=WM_MEM_HOST, budgets=None, prompt_len=None, sot_tail=None,
                                    length_penalty=None, max_candidates=None, medfilt_width=7, qk_scale=1.0, capture_matrix=False):
        """wm_transcribe_mel_beam_aligned: transcribe_mel_beam whose decode also aligns, per row, the hypothesis best[b] from the
        search's own cross-attention queries.  Every field of the BeamResult is transcribe_mel_beam's bit for bit; it also
        carries start_frames i32 [B][max_new + 1] of hypothesis best[b] and matrix (as transcribe_mel_best_of_aligned)."""
        return self._beam_call(self.lib.wm_transcribe_mel_beam_aligned,
                               lambda: self._mel_rows(mel, mel_base, mel_len, seek, n_frames, mem), (mem,), prompts, max_new,
                               beam_size, eot, patience, no_speech_token, sot_index, budgets, prompt_len, sot_tail, length_penalty,
                               max_candidates, aligned=(medfilt_width, qk_scale, capture_matrix))

    def transcribe_windows_beam_aligned(self, windows, rows, prompts, max_new, beam_size, eot=-1, patience=None, no_speech_token=-1,
                                        sot_index=0, budgets=None, prompt_len=None, sot_tail=None, length_penalty=None,
                                        max_candidates=None, medfilt_width=7, qk_scale=1.0, capture_matrix=False):
        """wm_transcribe_windows_beam_aligned: transcribe_mel_beam_aligned with rows of a Windows set.  Same bits."""
        return self._beam_call(self.lib.wm_transcribe_windows_beam_aligned, lambda: self._window_rows(windows, rows), (), prompts,
                               max_new, beam_size, eot, patience, no_speech_token, sot_index, budgets, prompt_len, sot_tail,
                               length_penalty, max_candidates, aligned=(medfilt_width, qk_scale, capture_matrix))

    def align_windows(self, windows, rows, text_tokens, sot_seqs, no_timestamps, eot, medfilt_width=7, qk_scale=1.0):
        """wm_align_windows: align_mel with rows of a Windows set (each of at least 2 frames); the alignment covers the set's
        own n_frames of a row.  Returns (start_frames, token_probs) as align."""
        head, B = self._window_rows(windows, rows)
        tt, nt, max_text, start, probs = self._text_table(text_tokens, B, "windows")
        sot = self._sot_table(sot_seqs, B)
        _check(self.lib, self.lib.wm_align_windows(self.handle, *head, B, _ptr(sot), sot.shape[1], int(no_timestamps), int(eot),
                                                   _ptr(tt), _ptr(nt), max_text, int(medfilt_width), float(qk_scale),
                                                   _ptr(start), _ptr(probs)))
        return start, probs

    def windows_detect_language(self, windows, rows=None, sot=50258, lang_first=50259, lang_last=50357):
        """wm_windows_detect_language: detect_language_probs of encode_mel of the rows' zero-padded windows, from the set.
        Returns (lang_idx [B], probs [B][n_lang])."""
        head, B = self._window_rows(windows, rows)
        idx = np.empty(B, dtype=np.int32)
        probs = np.empty((B, lang_last - lang_first + 1), dtype=np.float32)
        _check(self.lib, self.lib.wm_windows_detect_language(self.handle, *head, B, sot, lang_first, lang_last, _ptr(idx),
                                                             _ptr(probs)))
        return idx, probs

    def transcribe_long(self, recordings, **kw):
        """openai-whisper's long-form transcribe() (module function transcribe_long) on this context."""
        return transcribe_long(self, recordings, **kw)

    def set_alignment_heads(self, pairs):
        """wm_set_alignment_heads: the (layer, head) pairs Context.align reads; empty = every head of the last half of the
        decoder layers (openai-whisper's default)."""
        pairs = [(int(l), int(h)) for l, h in pairs]
        ls = np.ascontiguousarray([p[0] for p in pairs], dtype=np.int32)
        hs = np.ascontiguousarray([p[1] for p in pairs], dtype=np.int32)
        _check(self.lib, self.lib.wm_set_alignment_heads(self.handle, _ptr(ls) if ls.size else None,
                                                         _ptr(hs) if hs.size else None, len(pairs)))

    @staticmethod
    def _text_table(text_tokens, B, rows_are):
        """The text tokens of an alignment call over B rows and the outputs they size: (tt i32 [B][max(max_text, 1)] zero
        padded, n_text i32 [B], max_text, start_frames i32 [B][max_text + 1], token_probs f32 [B][max_text])."""
        rows = [list(np.asarray(t).reshape(-1)) for t in text_tokens]
        if len(rows) != B:
            raise ValueError("text_tokens: %d lists for %d %s" % (len(rows), B, rows_are))
        max_text = max([len(r) for r in rows] + [0])
        tt = np.zeros((B, max(max_text, 1)), dtype=np.int32)
        for b, r in enumerate(rows):
            tt[b, :len(r)] = r
        nt = np.ascontiguousarray([len(r) for r in rows], dtype=np.int32)
        return tt, nt, max_text, np.empty((B, max_text + 1), dtype=np.int32), np.empty((B, max_text), dtype=np.float32)

    @staticmethod
    def _sot_table(sot_seqs, B):
        """one start sequence for every row, or B of one length: i32 [B][n]"""
        sot = np.asarray(sot_seqs, dtype=np.int32)
        if sot.ndim == 1:
            sot = np.broadcast_to(sot, (B, sot.size))
        if sot.ndim != 2 or sot.shape[0] != B:
            raise ValueError("sot_seqs: one start sequence, or one per window")
        return np.ascontiguousarray(sot)

    def _capture_matrix(self, B, max_text):
        """Debug library only: the buffer f32 [B][max_text + 1][1500] the NEXT alignment call writes its cost matrix to"""
        if not hasattr(self.lib, "wmdbg_align_capture"):
            raise WhisperError(-1, "capture_matrix needs the debug library: Context(dims, debug=True)")
        matrix = np.empty((B, max_text + 1, 1500), dtype=np.float32)
        self.lib.wmdbg_align_capture.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.lib.wmdbg_align_capture.restype = ctypes.c_int
        _check(self.lib, self.lib.wmdbg_align_capture(self.handle, _ptr(matrix)))
        return matrix

    def align(self, pcm, text_tokens, sot_seq, no_timestamps, eot, n_frames=None, medfilt_width=7, qk_scale=1.0,
              capture_matrix=False):
        """wm_align: word-level timing inputs of every chunk.  pcm [B][480000]; text_tokens: a list of B token lists (or an
        int array [B][n]).  Returns (start_frames i32 [B][max_text + 1], token_probs f32 [B][max_text]), -1 / 0 past each
        chunk's tokens; capture_matrix=True (debug library) also returns the cost matrix f32 [B][max_text + 1][1500]."""
        pcm = np.ascontiguousarray(pcm)
        B = pcm.shape[0]
        tt, nt, max_text, start, probs = self._text_table(text_tokens, B, "chunks")
        sot = np.ascontiguousarray(sot_seq, dtype=np.int32)
        nf = None if n_frames is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_frames, dtype=np.int32), (B,)))
        matrix = self._capture_matrix(B, max_text) if capture_matrix else None
        _check(self.lib, self.lib.wm_align(self.handle, _ptr(pcm), _DTYPES[pcm.dtype], B, _ptr(sot), len(sot),
                                           int(no_timestamps), int(eot), _ptr(tt), _ptr(nt), max_text,
                                           _ptr_or_null(nf), int(medfilt_width), float(qk_scale),
                                           _ptr(start), _ptr(probs), WM_MEM_HOST))
        return (start, probs, matrix) if capture_matrix else (start, probs)

    def align_mel(self, mel, mel_base, mel_len, seek, n_frames, text_tokens, sot_seqs, no_timestamps, eot, medfilt_width=7,
                  qk_scale=1.0, capture_matrix=False, mem=WM_MEM_HOST):
        """wm_align_mel: Context.align on mel windows.  mel, mel_base, mel_len, seek, n_frames, mem: the window description
        of transcribe_mel_raw (n_frames 2 .. 3000: also the audio frames the alignment covers); sot_seqs: one start
        sequence for every row, or B of one length (one per row).  Returns what align returns."""
        mel, mp, base, mlen, sk, nf, B = self._window_arrays(mel, mel_base, mel_len, seek, n_frames, mem)
        tt, nt, max_text, start, probs = self._text_table(text_tokens, B, "windows")
        sot = self._sot_table(sot_seqs, B)
        matrix = self._capture_matrix(B, max_text) if capture_matrix else None
        _check(self.lib, self.lib.wm_align_mel(self.handle, mp, _ptr(base), _ptr(mlen), _ptr(sk), _ptr(nf), B, _ptr(sot),
                                               sot.shape[1], int(no_timestamps), int(eot), _ptr(tt), _ptr(nt), max_text,
                                               int(medfilt_width), float(qk_scale), _ptr(start), _ptr(probs), mem))
        return (start, probs, matrix) if capture_matrix else (start, probs)

    def dtw(self, mats):
        """Debug library only: the DTW kernel of wm_align alone on a list of f32 cost matrices [N][M] (N <= 448,
        M <= 1500).  Returns the start frame of every row of each (wmdbg_dtw)."""
        if not hasattr(self.lib, "wmdbg_dtw"):
            raise WhisperError(-1, "dtw needs the debug library: Context(dims, debug=True)")
        B = len(mats)
        N = np.ascontiguousarray([m.shape[0] for m in mats], dtype=np.int32)
        M = np.ascontiguousarray([m.shape[1] for m in mats], dtype=np.int32)
        nmax, ld = max(int(N.max()), 1), max(int(M.max()), 1)
        x = np.zeros((B, nmax, ld), dtype=np.float32)
        for b, m in enumerate(mats):
            x[b, :m.shape[0], :m.shape[1]] = m
        out = np.empty((B, nmax), dtype=np.int32)
        fn = self.lib.wmdbg_dtw
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                       ctypes.c_void_p]
        fn.restype = ctypes.c_int
        _check(self.lib, fn(self.handle, _ptr(x), B, _ptr(N), _ptr(M), ld, _ptr(out)))
        return [out[b, :N[b]] for b in range(B)]

    def align_matrix(self, q, keys, heads, S, n_text, n_frames, medfilt_width=7, qk_scale=1.0, col_stats=False):
        """Debug library only: the alignment kernels of wm_align alone (wmdbg_align_matrix).  q f32 [B][Tq][J][64], keys f32
        [L][B][H][1500][64], heads: J (layer, head) pairs.  Returns the cost matrix x f32 [B][Tq - S - 1][1500] (the NaN bits
        0x7fc0dead off each chunk's n + 1 rows x n_frames // 2 frames), with col_stats=True also the column statistics
        f32 [B][J][1500][2] (mean, std)."""
        if not hasattr(self.lib, "wmdbg_align_matrix"):
            raise WhisperError(-1, "align_matrix needs the debug library: Context(dims, debug=True)")
        q = np.ascontiguousarray(q, dtype=np.float32)
        keys = np.ascontiguousarray(keys, dtype=np.float32)
        B, Tq, J = q.shape[:3]
        L, H = keys.shape[0], keys.shape[2]
        if q.shape[3] != 64 or keys.shape[1:] != (B, H, 1500, 64) or len(heads) != J:
            raise ValueError("align_matrix: q %s, keys %s, %d heads" % (q.shape, keys.shape, len(heads)))
        hl = np.ascontiguousarray([p[0] for p in heads], dtype=np.int32)
        hh = np.ascontiguousarray([p[1] for p in heads], dtype=np.int32)
        nt = np.ascontiguousarray(np.broadcast_to(np.asarray(n_text, dtype=np.int32), (B,)))
        nf = np.ascontiguousarray(np.broadcast_to(np.asarray(n_frames, dtype=np.int32), (B,)))
        x = np.empty((B, Tq - S - 1, 1500), dtype=np.float32)
        cs = np.empty((B, J, 1500, 2), dtype=np.float32) if col_stats else None
        fn = self.lib.wmdbg_align_matrix
        vp, ip = ctypes.c_void_p, ctypes.c_int
        fn.argtypes = [vp, vp, vp, ip, ip, ip, ip, ip, vp, vp, ip, vp, vp, ip, ctypes.c_float, vp, vp]
        fn.restype = ctypes.c_int
        _check(self.lib, fn(self.handle, _ptr(q), _ptr(keys), L, H, B, Tq, J, _ptr(hl), _ptr(hh), int(S), _ptr(nt), _ptr(nf),
                            int(medfilt_width), float(qk_scale), _ptr(x), _ptr(cs) if col_stats else None))
        return (x, cs) if col_stats else x

    def align_matrix_rows(self, q, keys, heads, S, n_text, n_frames, medfilt_width=7, qk_scale=1.0, tail_rows=0):
        """Debug library only: align_matrix with the row rule of an aligned transcribe group (wmdbg_align_matrix_rows):
        tail_rows decoder rows behind the last matrix row.  0: chunk b has S + n_text[b] + 1 decoder rows and n_text[b] + 1
        matrix rows (-1: none), x f32 [B][Tq - S][1500]; 1: align_matrix."""
        if not hasattr(self.lib, "wmdbg_align_matrix_rows"):
            raise WhisperError(-1, "align_matrix_rows needs the debug library: Context(dims, debug=True)")
        q = np.ascontiguousarray(q, dtype=np.float32)
        keys = np.ascontiguousarray(keys, dtype=np.float32)
        B, Tq, J = q.shape[:3]
        L, H = keys.shape[0], keys.shape[2]
        if q.shape[3] != 64 or keys.shape[1:] != (B, H, 1500, 64) or len(heads) != J:
            raise ValueError("align_matrix_rows: q %s, keys %s, %d heads" % (q.shape, keys.shape, len(heads)))
        hl = np.ascontiguousarray([p[0] for p in heads], dtype=np.int32)
        hh = np.ascontiguousarray([p[1] for p in heads], dtype=np.int32)
        nt = np.ascontiguousarray(np.broadcast_to(np.asarray(n_text, dtype=np.int32), (B,)))
        nf = np.ascontiguousarray(np.broadcast_to(np.asarray(n_frames, dtype=np.int32), (B,)))
        x = np.empty((B, max(Tq - S - int(tail_rows), 1), 1500), dtype=np.float32)
        fn = self.lib.wmdbg_align_matrix_rows
        vp, ip = ctypes.c_void_p, ctypes.c_int
        fn.argtypes = [vp, vp, vp, ip, ip, ip, ip, ip, vp, vp, ip, vp, vp, ip, ctypes.c_float, vp, vp, ip]
        fn.restype = ctypes.c_int
        _check(self.lib, fn(self.handle, _ptr(q), _ptr(keys), L, H, B, Tq, J, _ptr(hl), _ptr(hh), int(S), _ptr(nt), _ptr(nf),
                            int(medfilt_width), float(qk_scale), _ptr(x), None, int(tail_rows)))
        return x

    def align_token_prob(self, logits, tok, eot, V=None):
        """Debug library only: the token-probability kernel of wm_align alone (wmdbg_align_token_prob) on logits rows f32
        [B][ldo] (V <= ldo columns, default ldo): softmax(logits[b][:eot])[tok[b]] f32 [B]."""
        if not hasattr(self.lib, "wmdbg_align_token_prob"):
            raise WhisperError(-1, "align_token_prob needs the debug library: Context(dims, debug=True)")
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        B, ldo = logits.shape
        tok = np.ascontiguousarray(np.broadcast_to(np.asarray(tok, dtype=np.int32), (B,)))
        out = np.empty(B, dtype=np.float32)
        fn = self.lib.wmdbg_align_token_prob
        vp, ip = ctypes.c_void_p, ctypes.c_int
        fn.argtypes = [vp, vp, ip, ip, ip, vp, ip, vp]
        fn.restype = ctypes.c_int
        _check(self.lib, fn(self.handle, _ptr(logits), B, int(ldo if V is None else V), ldo, _ptr(tok), int(eot), _ptr(out)))
        return out

    def sample_noise(self, seed, chunk, gi, n0, count):
        """Debug library only: the Gumbel noise g(n0 .. n0 + count - 1) wm_transcribe's sampling adds, from the device."""
        if not hasattr(self.lib, "wmdbg_sample_noise"):
            raise WhisperError(-1, "sample_noise needs the debug library: Context(dims, debug=True)")
        fn = self.lib.wmdbg_sample_noise
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                       ctypes.c_void_p]
        fn.restype = ctypes.c_int
        g = np.empty(count, dtype=np.float32)
        _check(self.lib, fn(self.handle, int(seed) & 0xFFFFFFFFFFFFFFFF, int(chunk), int(gi), int(n0), int(count), _ptr(g)))
        return g


# openai-whisper's defaults (whisper/transcribe.py): punctuation merged into the following / preceding word
PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
NO_SPACE_LANGUAGES = {"zh", "ja", "th", "lo", "my", "yue"}
FRAMES_PER_SECOND = 50   # audio frames of the encoder output (openai-whisper TOKENS_PER_SECOND)
_EOT = object()          # the <|endoftext|> find_alignment appends to the text tokens


def _split_tokens_on_unicode(decode, tokens):
    """openai-whisper Tokenizer.split_tokens_on_unicode: cut wherever the tokens so far decode to whole characters."""
    decoded_full = decode(tokens)
    words, word_tokens, current, offset = [], [], [], 0
    for t in tokens:
        current.append(t)
        decoded = decode(current)
        if "\ufffd" not in decoded or decoded_full[offset + decoded.index("\ufffd")] == "\ufffd":
            words.append(decoded)
            word_tokens.append(current)
            current = []
            offset += len(decoded)
    return words, word_tokens


def _split_tokens_on_spaces(decode, tokens):
    """openai-whisper Tokenizer.split_tokens_on_spaces: subwords joined until a space, a punctuation mark or a special."""
    import string
    subwords, subword_tokens = _split_tokens_on_unicode(decode, tokens)
    words, word_tokens = [], []
    for sw, st in zip(subwords, subword_tokens):
        if st[0] is _EOT or sw.startswith(" ") or sw.strip() in string.punctuation or not words:
            words.append(sw)
            word_tokens.append(list(st))
        else:
            words[-1] = words[-1] + sw
            word_tokens[-1].extend(st)
    return words, word_tokens


def _merge_punctuations(alignment, prepended, appended):
    """openai-whisper merge_punctuations (whisper/timing.py), in place on dicts with `word` and `tokens`."""
    i, j = len(alignment) - 2, len(alignment) - 1
    while i >= 0:
        prev, foll = alignment[i], alignment[j]
        if prev["word"].startswith(" ") and prev["word"].strip() in prepended:
            foll["word"] = prev["word"] + foll["word"]
            foll["tokens"] = prev["tokens"] + foll["tokens"]
            prev["word"] = ""
            prev["tokens"] = []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(alignment):
        prev, foll = alignment[i], alignment[j]
        if not prev["word"].endswith(" ") and foll["word"] in appended:
            prev["word"] = prev["word"] + foll["word"]
            prev["tokens"] = prev["tokens"] + foll["tokens"]
            foll["word"] = ""
            foll["tokens"] = []
        else:
            i = j
        j += 1


def word_timestamps(vocab, text_tokens, start_frames, token_probs, language=None,
                    prepend_punctuations=PREPEND_PUNCTUATIONS, append_punctuations=APPEND_PUNCTUATIONS):
    """Words of ONE chunk from Context.align's outputs, as openai-whisper's find_alignment + merge_punctuations build them:
    [{word, tokens, start, end, probability}], times in seconds (frame / 50) from the chunk's start.

    The text tokens (plus the <|endoftext|> find_alignment appends) are split into words by split_tokens_on_unicode for
    zh / ja / th / lo / my / yue and by split_tokens_on_spaces otherwise (Vocab.decode gives U+FFFD for a partial UTF-8
    piece).  A word of tokens [a, b) spans [start_frames[a], start_frames[b]) and its probability is the mean of
    token_probs[a:b].  Punctuation is then merged into the neighbouring words (which keep their own times); words left
    empty are dropped.  add_word_timestamps' segment heuristics are not applied here: window_word_timestamps applies them
    to the segments of a long-form window."""
    out = _alignment_words(vocab, text_tokens, start_frames, token_probs, language)
    _merge_punctuations(out, prepend_punctuations, append_punctuations)
    return [w for w in out if w["word"]]


def _alignment_words(vocab, text_tokens, start_frames, token_probs, language):
    """find_alignment's words before punctuation merging (word_timestamps' docstring), zero-length and empty ones kept."""
    toks = [int(t) for t in np.asarray(text_tokens).reshape(-1)]
    n = len(toks)
    if n == 0:
        return []
    start_frames = np.asarray(start_frames)
    token_probs = np.asarray(token_probs, dtype=np.float64)

    def decode(ts):
        ids = [t for t in ts if t is not _EOT]
        text = vocab.decode(ids, skip_special=False) if ids else ""
        return text + ("<|endoftext|>" if ts and ts[-1] is _EOT else "")

    split = _split_tokens_on_unicode if language in NO_SPACE_LANGUAGES else _split_tokens_on_spaces
    words, word_tokens = split(decode, toks + [_EOT])
    if len(word_tokens) <= 1:
        return []
    bounds = np.concatenate([[0], np.cumsum([len(t) for t in word_tokens[:-1]])]).astype(np.int64)
    out = []
    for k in range(len(bounds) - 1):   # the last word is <|endoftext|> (or ends with it): dropped, as by find_alignment
        a, b = int(bounds[k]), int(bounds[k + 1])
        out.append(dict(word=words[k], tokens=[t for t in word_tokens[k] if t is not _EOT],
                        start=float(start_frames[a]) / FRAMES_PER_SECOND, end=float(start_frames[b]) / FRAMES_PER_SECOND,
                        probability=float(np.mean(token_probs[a:b]))))
    return out


SENTENCE_END_MARKS = ".。!！?？"


def window_word_timestamps(vocab, segments, start_frames, token_probs, seek, eot, last_speech_timestamp, language=None,
                           prepend_punctuations=PREPEND_PUNCTUATIONS, append_punctuations=APPEND_PUNCTUATIONS):
    """openai-whisper's add_word_timestamps (whisper/timing.py) for ONE long-form window with at least one segment: the
    words of Context.align_mel's outputs for the window's text tokens -- the tokens < eot of its segments, concatenated --
    dealt out to the segments as `words` [{word, start, end, probability}] in seconds of the recording, with its
    heuristics: word durations capped at twice the window's median (at most 0.7 s) around sentence ends, a long first
    word after a pause pulled to its end, a segment's start / end and its first / last word reconciled.  Edits the
    segments (as window_segments(..., cleanup=False) returns them) in place: words, start, end.  Returns the new
    last_speech_timestamp (the end of the last segment that has words)."""
    per_segment = [[int(t) for t in sg["tokens"] if t < eot] for sg in segments]
    text_tokens = [t for ts in per_segment for t in ts]
    alignment = _alignment_words(vocab, text_tokens, start_frames, token_probs, language)
    durations = np.array([w["end"] - w["start"] for w in alignment], dtype=np.float64)
    durations = durations[durations.nonzero()]
    median = min(0.7, float(np.median(durations))) if len(durations) > 0 else 0.0
    max_duration = median * 2
    if len(durations) > 0:   # a long word at a sentence end is cut at its start side, one behind a sentence end at its end side
        for i in range(1, len(alignment)):
            w = alignment[i]
            if w["end"] - w["start"] > max_duration:
                if _is_sentence_end(w["word"]):
                    w["end"] = w["start"] + max_duration
                elif _is_sentence_end(alignment[i - 1]["word"]):
                    w["start"] = w["end"] - max_duration
    _merge_punctuations(alignment, prepend_punctuations, append_punctuations)
    time_offset = seek * HOP_SECONDS
    word_index = 0
    for sg, toks in zip(segments, per_segment):
        saved = 0
        words = []
        while word_index < len(alignment) and saved < len(toks):
            t = alignment[word_index]
            if t["word"]:
                words.append(dict(word=t["word"], start=round(time_offset + t["start"], 2),
                                  end=round(time_offset + t["end"], 2), probability=t["probability"]))
            saved += len(t["tokens"])
            word_index += 1
        if words:
            # a first word that ends long after the last speech and is itself (or with its follower) too long: a pause
            if words[0]["end"] - last_speech_timestamp > median * 4 and (
                    words[0]["end"] - words[0]["start"] > max_duration
                    or (len(words) > 1 and words[1]["end"] - words[0]["start"] > max_duration * 2)):
                if len(words) > 1 and words[1]["end"] - words[1]["start"] > max_duration:
                    boundary = max(words[1]["end"] / 2, words[1]["end"] - max_duration)
                    words[0]["end"] = words[1]["start"] = boundary
                words[0]["start"] = max(0, words[0]["end"] - max_duration)
            # prefer the segment-level start timestamp if the first word is too long
            if sg["start"] < words[0]["end"] and sg["start"] - 0.5 > words[0]["start"]:
                words[0]["start"] = max(0, min(words[0]["end"] - median, sg["start"]))
            else:
                sg["start"] = words[0]["start"]
            # prefer the segment-level end timestamp if the last word is too long
            if sg["end"] > words[-1]["start"] and sg["end"] + 0.5 < words[-1]["end"]:
                words[-1]["end"] = max(words[-1]["start"] + median, sg["end"])
            else:
                sg["end"] = words[-1]["end"]
            last_speech_timestamp = sg["end"]
        sg["words"] = words
    return last_speech_timestamp


def _is_sentence_end(word):
    return len(word) == 1 and word in SENTENCE_END_MARKS


class Vocab:
    """wm_vocab: GPT-2 byte-level BPE de-tokenizer over a host-supplied vocab.json (ids -> UTF-8 text, no GPU)."""

    def __init__(self, vocab_json_path):
        self.lib = load_library()
        self.handle = ctypes.c_void_p()
        _check(self.lib, self.lib.wm_vocab_load(str(vocab_json_path).encode(), ctypes.byref(self.handle)))

    def __len__(self):
        return int(self.lib.wm_vocab_size(self.handle))

    def decode(self, ids, skip_special=True):
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        need = ctypes.c_size_t()
        _check(self.lib, self.lib.wm_detokenize(self.handle, _ptr(ids), len(ids), 1 if skip_special else 0, None, 0,
                                                ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        _check(self.lib, self.lib.wm_detokenize(self.handle, _ptr(ids), len(ids), 1 if skip_special else 0, buf,
                                                need.value, None))
        return buf.raw[:need.value - 1].decode("utf-8", "replace")

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self.lib.wm_vocab_free(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Wav:
    """wm_wav: 16 kHz mono 16-bit RIFF/WAVE reader + 30 s chunker behind the C ABI (host only)."""

    def __init__(self, path):
        self.lib = load_library()
        self.handle = ctypes.c_void_p()
        _check(self.lib, self.lib.wm_wav_open(str(path).encode(), ctypes.byref(self.handle)))

    @property
    def num_samples(self):
        return int(self.lib.wm_wav_num_samples(self.handle))

    @property
    def num_chunks(self):
        return int(self.lib.wm_wav_num_chunks(self.handle))

    def chunks(self, first=0, n=None):
        n = self.num_chunks - first if n is None else n
        out = np.empty((n, N_SAMPLES), dtype=np.int16)
        _check(self.lib, self.lib.wm_wav_read_chunks(self.handle, int(first), int(n), _ptr(out)))
        return out

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self.lib.wm_wav_close(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Audio:
    """wm_audio: general RIFF/WAVE reader behind the C ABI (host only) -- any rate, 1 .. 8 channels, integer PCM 8 / 16 / 24 /
    32 bits, IEEE float 32 / 64 bits, WAVE_FORMAT_EXTENSIBLE; what Context.resample_16k takes."""

    def __init__(self, path):
        self.lib = load_library()
        self.handle = ctypes.c_void_p()
        _check(self.lib, self.lib.wm_audio_open(str(path).encode(), ctypes.byref(self.handle)))

    @property
    def sample_rate(self):
        return int(self.lib.wm_audio_sample_rate(self.handle))

    @property
    def channels(self):
        return int(self.lib.wm_audio_channels(self.handle))

    @property
    def num_frames(self):
        return int(self.lib.wm_audio_num_frames(self.handle))

    @property
    def bits(self):
        return int(self.lib.wm_audio_bits(self.handle))

    @property
    def is_float(self):
        return bool(self.lib.wm_audio_is_float(self.handle))

    def read(self, first=0, n=None, raw_int16=False):
        """Frames [first, first + n) as f32 [n][channels]; raw_int16=True (16-bit integer files only): the int16 samples."""
        n = self.num_frames - first if n is None else n
        rows = min(max(int(n), 0), self.num_frames)   # (a range outside the recording is the library's to refuse)
        out = np.empty((rows, self.channels), dtype=np.int16 if raw_int16 else np.float32)
        fn = self.lib.wm_audio_read_i16 if raw_int16 else self.lib.wm_audio_read
        _check(self.lib, fn(self.handle, int(first), int(n), _ptr(out)))
        return out

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self.lib.wm_audio_close(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiContext:
    """wm_multi: every listed GPU of the node from ONE process (include/whisper_mi355x.h): weights replicated, chunks
    block-partitioned, one RCCL all-gather of the token streams."""

    def __init__(self, dims, devices=(0,)):
        self.lib = load_library()
        self.handle = ctypes.c_void_p()
        d = wm_dims(**dims) if isinstance(dims, dict) else dims
        devs = np.ascontiguousarray(list(devices), dtype=np.int32)
        _check(self.lib, self.lib.wm_multi_create(ctypes.byref(d), _ptr(devs), len(devs), ctypes.byref(self.handle)))
        self.dims = d.as_dict()
        self.n = int(self.lib.wm_multi_size(self.handle))

    def device_ctx(self, rank):
        """Borrowed Context of one device (owned by the MultiContext: do not close it)."""
        c = Context.__new__(Context)
        c.lib = self.lib
        c.handle = ctypes.c_void_p()
        c.dims = dict(self.dims)
        _check(self.lib, self.lib.wm_multi_device_ctx(self.handle, int(rank), ctypes.byref(c.handle)))
        c.close = lambda: None
        c._owner = self
        return c

    def init_synthetic(self, seed):
        for r in range(self.n):
            c = self.device_ctx(r)
            c.init_synthetic(seed)
            c.finalize()

    def transcribe_greedy(self, pcm, prompt, max_new, eot=-1):
        pcm = np.ascontiguousarray(pcm)
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        Bn = pcm.shape[0]
        toks = np.empty((Bn, max_new), dtype=np.int32)
        lens = np.empty(Bn, dtype=np.int32)
        _check(self.lib, self.lib.wm_multi_transcribe_greedy(self.handle, _ptr(pcm), _DTYPES[pcm.dtype], Bn, _ptr(prompt),
                                                             len(prompt), max_new, eot, _ptr(toks), _ptr(lens)))
        return toks, lens

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self.lib.wm_multi_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Whisper:
    """Mirror of `struct Whisper` (Whisper/Whisper/Whisper.swift:11-41).

    The reference constructs CoreML `decoder` then `encoder` from bundled .mlpackages
    (Whisper.swift:17-21); here construction takes the model dimensions and a weight
    source (state dict, flat weight file, or a synthetic seed) and uploads to HBM."""

    LANGUAGES = ["en", "zh", "de", "es", "ru", "ko", "fr", "ja", "pt", "tr", "pl", "ca", "nl", "ar",
                 "sv", "it", "id", "hi", "fi", "vi", "iw", "uk", "el", "ms", "cs", "ro", "da", "hu",
                 "ta", "no", "th", "ur", "hr", "bg", "lt", "la", "mi", "ml", "cy", "sk", "te", "fa",
                 "lv", "bn", "sr", "az", "sl", "kn", "et", "mk", "br", "eu", "is", "hy", "ne", "mn",
                 "bs", "kk", "sq", "sw", "gl", "mr", "pa", "si", "km", "sn", "yo", "so", "af", "oc",
                 "ka", "be", "tg", "sd", "gu", "am", "yi", "lo", "uz", "fo", "ht", "ps", "tk", "nn",
                 "mt", "sa", "lb", "my", "bo", "tl", "mg", "as", "tt", "haw", "ln", "ha", "ba", "jw",
                 "su"]  # Whisper.swift:12 (99 codes, openai-whisper tokenizer order)

    SOT = 50258          # Whisper.swift:35
    LANG_FIRST = 50259   # Whisper.swift:37
    LANG_LAST = 50357

    def __init__(self, dims="small", state_dict=None, weights_path=None, synthetic_seed=None, device=0):
        d = MODEL_DIMS[dims] if isinstance(dims, str) else dims
        self.ctx = Context(d, device=device)
        if state_dict is not None:
            self.ctx.load_state_dict(state_dict)
        elif weights_path is not None:
            self.ctx.load_weights(weights_path)
        elif synthetic_seed is not None:
            self.ctx.init_synthetic(synthetic_seed)
        else:
            raise ValueError("one of state_dict / weights_path / synthetic_seed is required")
        self.ctx.finalize()

    def encode(self, audio):
        """Whisper.swift:23-31: spectrogram -> f32 [1,80,3000] -> encoder -> [1,1500,d]."""
        spec = generateSpectrogram(audio)                                # :24
        array = spec.astype(np.float32).reshape(1, 80, N_FRAMES)         # :25-28 (f64 -> f32)
        return self.ctx.encode_mel(array)                                # :29

    def decode(self, audioFeatures):
        """Whisper.swift:33-40: one decoder step on SOT, arg-max over the language ids.
        The reference prints the code and returns Void; this returns the code."""
        idx = self.ctx.detect_language(audioFeatures, self.SOT, self.LANG_FIRST, self.LANG_LAST)
        return self.LANGUAGES[int(idx[0])]
