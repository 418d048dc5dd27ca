/*
 * whisper_mi355x.h -- C ABI of libwhisper_mi355x.so, the MI355X (gfx950) drop-in for the
 * two native halves of tanmayb123/OpenAI-Whisper-CoreML's hot path:
 *
 *   boundary #1  the Rust `stft` staticlib          (stft/src/lib.rs:110-122, bridge.h:11)
 *   boundary #2  the CoreML encoder/decoder classes (Whisper/Whisper/Whisper.swift:17-40,
 *                contract fixed by whisper_to_cml.py:10-43)
 *
 * Plain C: pointers, sizes, ints.  No torch / C++ types cross this boundary.  Every
 * function except generate_spectrogram returns an int status (WM_OK == 0) and never
 * aborts or throws across the FFI; wm_last_error() returns the message for the calling
 * thread.  A wm_ctx is not thread-safe; distinct contexts are independent.
 *
 * All pointers are HOST pointers unless the argument is documented "mem-space
 * selectable", in which case `mem` says where it lives (WM_MEM_HOST / WM_MEM_DEVICE).
 */
#ifndef WHISPER_MI355X_H
#define WHISPER_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly the functions declared here are exported. */
#define WM_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------ status codes --- */
enum {
    WM_OK = 0,
    WM_ERR_INVALID = 1,   /* bad argument (null, size, dtype, dims)                     */
    WM_ERR_HIP = 2,       /* a HIP runtime call failed / no gfx950 device               */
    WM_ERR_STATE = 3,     /* call order (weights not finalised, ctx has no model, ...)  */
    WM_ERR_IO = 4,        /* weight file unreadable / malformed                         */
    WM_ERR_NOMEM = 5
};

typedef enum { WM_I16 = 0, WM_F32 = 1, WM_F64 = 2, WM_BF16 = 3 } wm_dtype;
typedef enum { WM_MEM_HOST = 0, WM_MEM_DEVICE = 1 } wm_mem;

/* Model dimensions: the fields of openai-whisper's ModelDimensions, i.e. what
 * whisper.load_model(...) at whisper_to_cml.py:7 fixes for the exported graphs. */
typedef struct wm_dims {
    int32_t n_mels;        /* 80 (128 for large-v3)                                     */
    int32_t n_audio_ctx;   /* 1500                                                      */
    int32_t n_audio_state; /* d                                                         */
    int32_t n_audio_head;
    int32_t n_audio_layer;
    int32_t n_vocab;       /* 51865 (51864 *.en, 51866 large-v3)                        */
    int32_t n_text_ctx;    /* 448                                                       */
    int32_t n_text_state;
    int32_t n_text_head;
    int32_t n_text_layer;
} wm_dims;

typedef struct wm_ctx wm_ctx;

/* ------------------------------------------------------- boundary #1: the front end --- */

/* EXACT replacement for the reference's only native symbol:
 *   Whisper/Whisper/bridge.h:11      void generate_spectrogram(double *, double *);
 *   stft/src/lib.rs:110-122          #[no_mangle] pub extern fn generate_spectrogram(...)
 * arg0: 480400 f64, caller-owned and MUTATED exactly as lib.rs:34-40,113 does (elements
 *       [0,200) and [480200,480400) are overwritten with the reflected samples);
 * arg1: 240000 f64, row-major [80][3000] (lib.rs:116-121).
 * Lengths are implicit, nothing is retained, the symbol is re-entrant.  Runs the f64
 * kernels on device $WM_DEVICE (default 0).  Like the reference (unwrap -> panic ->
 * abort, lib.rs:45,85-87,106) it cannot report an error: on a HIP failure it prints the
 * reason to stderr and abort()s -- there is no CPU fallback. */
WM_API void generate_spectrogram(double *audio, double *output);

/* Batched, typed, error-returning form of the same computation (lib.rs:49-102).
 *   pcm   : [n_chunks][480000] samples, dtype WM_I16 (x = s/32768), WM_F32 or WM_F64;
 *           mem-space selectable.  (No +200 padding: the reflect of lib.rs:34-40 is done
 *           by index arithmetic on device.)
 *   n_mels: 80 (the reference's m80.npy filterbank, bit-exact) or 128 (slaney filters
 *           generated as openai-whisper's mel_128, for large-v3).
 *   out   : [n_chunks][n_mels][3000], dtype WM_F64 (f64 arithmetic end to end: the
 *           ABI-exact path) or WM_F32 (f32 arithmetic: the fast path); mem-space
 *           selectable (same `mem` as pcm). */
WM_API int wm_logmel(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, int n_chunks, int n_mels,
              void *out, wm_dtype out_dtype, wm_mem mem);

/* openai-whisper's log_mel_spectrogram(audio, padding=480000) for R recordings of any length: the front end of its
 * long-form transcribe(), one log-mel over the whole recording.  Recording r's signal is its samples followed by 480000
 * zeros, reflect-padded by 200 samples at both ends (torch.stft center=True, pad_mode="reflect"); then the f32 fast path of
 * wm_logmel frame by frame (periodic Hann 400, hop 160, power, mel, log10(max(., 1e-10))), the same kernel arithmetic;
 * then max(x, gmax_r - 8) with gmax_r over ALL T_r frames of the recording, and (x + 4) / 4.
 *   pcm            : the samples of all recordings back to back, WM_I16 (x = s/32768) / WM_F32 / WM_F64, mem-space
 *                    selectable (with WM_MEM_HOST only pcm[sample_offsets[0] .. sample_offsets[R]) is copied);
 *   sample_offsets : i64 [R + 1] (host), non-decreasing: recording r = pcm[sample_offsets[r] .. sample_offsets[r + 1]),
 *                    0 .. 2^30 samples;  R : 0 .. 65535;
 *   n_mels         : 80 / 128, as wm_logmel;
 *   out            : f32, recording r's [n_mels][T_r] block after those of recordings 0 .. r - 1,
 *                    T_r = (len_r + 480000) / 160 (integer division: torch.stft's center=True frames minus the last, as
 *                    openai-whisper drops it); same `mem` as pcm.
 * Frames [0, 2999) of a 30 s recording see the same samples as wm_logmel's chunk; when the recording's maximum lies
 * there, they are bit-identical to wm_logmel(..., WM_F32). */
WM_API int wm_logmel_long(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, const int64_t *sample_offsets, int R,
                          int n_mels, float *out, wm_mem mem);

/* ---- live audio: a set of S streams whose appended samples become log-mel frames incrementally, on the device (DESIGN.md
 * "Live streams").  A front-end-only context is enough.  Everything is enqueued on the context's stream, so pushes and
 * windows are ordered.  Stream s has received N samples, an absolute i64 count; stream time has no limit.
 *   frame t      : wm_logmel_long's frame t of a recording that begins where the stream began: centred at sample 160 t, it
 *                  reads the samples [160 t - 200, 160 t + 200); an index n < 0 reads sample -n (torch center=True,
 *                  reflect); a sample that has not arrived reads 0 -- no reflect at the live end, which is what
 *                  wm_logmel_long computes for a recording that ends at N, because 480000 zeros follow it.
 *   final_frames : F, the frames whose every sample has arrived, 160 t + 200 <= N (frame 0 reads sample 200: N >= 201); a prefix.
 *   avail_frames : A, the frames that read at least one arrived sample: 0 for N = 0, else (N + 199) / 160 + 1.  Frames
 *                  [F, A) are PROVISIONAL, at most 3; every push recomputes them until they are final.
 *   first_kept   : K = max(0, A - capacity_frames); older frames are gone.
 * The set keeps per stream, on the device: a ring of capacity_frames columns of the RAW values log10(max(mel, 1e-10)), before
 * any normalisation; each frame's maximum over its mel rows; and a carry of the staged f32 samples (at most 399) that frames
 * which are not final still need.  The carry holds values after conversion, and a frame's arithmetic sees its own 400
 * samples alone: a frame does not depend on how the audio was split into pushes, nor on the dtype on either side of a split.
 *
 * wm_streams_create : S 1 .. 65535, n_mels 80 / 128, capacity_frames >= 3003 (a 3000-frame window and the provisional frames
 *                     always fit).  WM_ERR_INVALID otherwise.
 * wm_streams_free   : NULL: no-op; synchronises the context's stream.
 * wm_streams_push   : appends pcm[sample_offsets[s] .. sample_offsets[s + 1]) to stream s, for all S streams at once.
 *     pcm            : WM_I16 (x = s/32768) / WM_F32 / WM_F64, the conversions of the f32 fast path; mem-space selectable
 *                      (with WM_MEM_HOST only pcm[sample_offsets[0] .. sample_offsets[S]) is copied); may be NULL when no
 *                      stream gets a sample;
 *     sample_offsets : i64 [S + 1] (host), >= 0 and non-decreasing; zero samples are legal, at most 2^30 per stream and call.
 *   One launch of the f32 front-end kernel computes, for all streams, every frame that became final and the new provisional
 *   frames; a push that brings more than capacity_frames frames computes only those that stay.  A second, small launch
 *   moves the carries.  A push that fails validation changes nothing.
 * wm_streams_reset  : stream s is empty again (N = 0); the others are untouched.
 * wm_streams_frames : the counters N, F, A, K of every stream, i64 [S] each, any of them NULL.  Host only, no launch.
 * wm_streams_window : row r = frames [first_frame[r], first_frame[r] + n_frames[r]) of stream stream[r]; K <= first,
 *                     first + n <= A, n in 1 .. 3000; R in 1 .. 65535; several rows may name one stream.  The row's block
 *                     [n_mels][n_frames] is written at out + out_base[r] (element offsets, i64 [R], host; >= 0) as
 *                     (max(raw, gmax - 8) + 4) / 4 with gmax the maximum over exactly the row's frames -- the
 *                     normalisation of a recording that is the window, the arithmetic of wm_logmel's second stage.  One
 *                     launch for all rows, no atomics: deterministic.  out: f32, mem-space selectable.  The block is what
 *                     wm_transcribe_mel, wm_windows_encode, wm_align_mel and wm_vad_energy take as `mel` with mel_base =
 *                     out_base, mel_len = n_frames, seek = 0.  For first = 0 it is bit for bit wm_logmel_long's columns
 *                     [0, A) of the samples so far.
 * Errors: WM_ERR_INVALID for the ranges above, decreasing or negative offsets, a row outside [K, A), a stream index outside
 * the set, null pointers; WM_ERR_STATE for a set used with a context on another device. */
typedef struct wm_streams wm_streams;
WM_API int wm_streams_create(wm_ctx *ctx, int S, int n_mels, int capacity_frames, wm_streams **out);
WM_API int wm_streams_free(wm_ctx *ctx, wm_streams *set);
WM_API int wm_streams_push(wm_ctx *ctx, wm_streams *set, const void *pcm, wm_dtype pcm_dtype, const int64_t *sample_offsets,
                           wm_mem mem);
WM_API int wm_streams_reset(wm_ctx *ctx, wm_streams *set, int s);
WM_API int wm_streams_frames(const wm_streams *set, int64_t *samples, int64_t *final_frames, int64_t *avail_frames,
                             int64_t *first_kept);
WM_API int wm_streams_window(wm_ctx *ctx, wm_streams *set, int R, const int32_t *stream, const int64_t *first_frame,
                             const int32_t *n_frames, float *out, const int64_t *out_base, wm_mem mem);

/* --------------------------------------------------------- context / weight loading --- */

/* Front-end-only context (no model): enough for wm_logmel. */
WM_API int wm_create_frontend(int device, wm_ctx **out);

/* Model context with uninitialised weights ( == Whisper.init, Whisper.swift:17-21, minus
 * the load).  Fill with wm_set_tensor / wm_load_weights / wm_init_synthetic, then
 * wm_finalize. */
WM_API int wm_create(const wm_dims *dims, int device, wm_ctx **out);

/* Set one parameter from host f32 data.  Names are openai-whisper state-dict keys, e.g.
 * "encoder.conv1.weight", "encoder.blocks.0.attn.query.weight",
 * "decoder.token_embedding.weight" (SURVEY.md 8f row 2).  n_elems must match. */
WM_API int wm_set_tensor(wm_ctx *ctx, const char *name, const float *data, size_t n_elems);
/* Read a parameter back as f32 (the value the kernels use, i.e. after bf16 rounding for
 * matrix weights). */
WM_API int wm_get_tensor(wm_ctx *ctx, const char *name, float *data, size_t n_elems);
/* Flat weight file written by openai-whisper-coreml_amd/weights.py (format: the docstring of weights.py). */
WM_API int wm_load_weights(wm_ctx *ctx, const char *path);
/* ---- TEST / BENCHMARK WEIGHTS: NOT FOR PRODUCTION USE.  The two generators below exist because no checkpoint can be
 * shipped or downloaded where the tests and bench.py run; a deployment loads real weights (wm_load_weights /
 * wm_set_tensor) and never calls them.  They stay in the product library (not the debug one) for one reason: bench.py's
 * headline must be measured on libwhisper_mi355x.so itself, with weights whose token streams can fail a cross-check. ----
 * Deterministic synthetic weights generated ON DEVICE (hash-based, approx N(0, std^2));
 * identical values to weights.synthetic_state_dict(dims, seed) on the host. */
WM_API int wm_init_synthetic(wm_ctx *ctx, uint64_t seed);
/* The same generator with every weight MATRIX (conv / linear / token embedding; not the positional tables, biases or
 * LayerNorm parameters) multiplied by matrix_gain -- weights.synthetic_state_dict(dims, seed, matrix_gain).  Gain 4 makes a
 * random-init model whose token streams depend on the audio and on the decode history (N(0, 0.02^2) weights give a nearly
 * input-independent one): what the token-level parity tests and bench.py's cross-checks decode.  A power of two keeps the
 * values bf16-exact. */
WM_API int wm_init_synthetic_gain(wm_ctx *ctx, uint64_t seed, float matrix_gain);
/* Freeze weights: fuse QKV, permute conv taps, precompute tables.  Required before any
 * model call. */
WM_API int wm_finalize(wm_ctx *ctx);
/* A second context on the same device that SHARES the (finalised, read-only) weights of `parent`
 * and owns its own HIP stream, activations, KV caches and decode graph.  Independent batches
 * submitted to different contexts from different host threads overlap on the GPU.  Destroy clones
 * before their parent. */
WM_API int wm_clone(wm_ctx *parent, wm_ctx **out);
WM_API void wm_destroy(wm_ctx *ctx);

WM_API const char *wm_last_error(void);
WM_API int wm_get_dims(const wm_ctx *ctx, wm_dims *out);

/* ---------------------------------------------------------- boundary #2: the model --- */

/* == encoderModel.prediction(x_1:).var_1385 (Whisper.swift:29; whisper_to_cml.py:10-23).
 *   mel: f32 [B][n_mels][3000]  ->  xa: f32 [B][n_audio_ctx][n_audio_state].
 * Both mem-space selectable (same `mem`). */
WM_API int wm_encode(wm_ctx *ctx, const float *mel, int B, float *xa, wm_mem mem);

/* == decoderModel.prediction(x_1:xa:).var_2217 (Whisper.swift:36; whisper_to_cml.py:25-43),
 * generalised from T == 1 to a T-token prefix (stateless: offset 0, no cache is kept).
 *   tokens: i32 [B][T];  xa: f32 [B][n_audio_ctx][d];  logits: f32 [B][T][n_vocab]. */
WM_API int wm_decode_logits(wm_ctx *ctx, const int32_t *tokens, int B, int T, const float *xa,
                     float *logits, wm_mem mem);

/* == Whisper.decode (Whisper.swift:33-40): one decoder step on <|startoftranscript|>
 * (id `sot`, 50258 in the reference), arg-max over logits[lang_first .. lang_last]
 * (50259...50357 in the reference), FIRST maximal element wins (Swift max(by:)).
 *   lang_idx: i32 [B], index into Whisper.LANGUAGES. */
WM_API int wm_detect_language(wm_ctx *ctx, const float *xa, int B, int32_t sot, int32_t lang_first,
                       int32_t lang_last, int32_t *lang_idx, wm_mem mem);

/* Same step, additionally returning the language probabilities of openai-whisper's detect_language() [3p]: softmax over
 * the language-token logits only.  probs: f32 [B][lang_last - lang_first + 1], same memory space as xa / lang_idx. */
WM_API int wm_detect_language_probs(wm_ctx *ctx, const float *xa, int B, int32_t sot, int32_t lang_first,
                             int32_t lang_last, int32_t *lang_idx, float *probs, wm_mem mem);

/* New surface asked for by BASELINE.json (not in the reference): front end + encoder +
 * KV-cached greedy decode of B independent 30 s chunks.  Any B >= 1: the call is cut into balanced
 * decode groups (8 .. 128 chunks) that run concurrently on up to $WM_LANES (default 3) weight-sharing
 * lanes inside the context; tokens do not depend on the grouping (bit-level batch invariance).
 *   pcm        : [B][480000], dtype WM_I16 / WM_F32 / WM_F64, mem-space selectable;
 *   prompt     : i32 [n_prompt] initial tokens (e.g. {sot, lang, transcribe, notimestamps});
 *   max_new    : tokens to generate per chunk (<= n_text_ctx - n_prompt);
 *   eot        : stop token; pass -1 to suppress stopping (fixed-length benchmark decode).  With eot >= 0 a chunk that
 *                has produced it leaves the decode (its K/V caches are not read again) and a decode group whose chunks
 *                have all stopped is not decoded any further: the work follows the longest live sequence, the results
 *                are what decoding all max_new positions and truncating would give;
 *   tokens_out : i32 [B][max_new] (host), padded with `eot` after a chunk stops;
 *   lens_out   : i32 [B] (host) generated length per chunk. */
WM_API int wm_transcribe_greedy(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, int B,
                         const int32_t *prompt, int n_prompt, int max_new, int32_t eot,
                         int32_t *tokens_out, int32_t *lens_out, wm_mem mem);

/* Options of wm_transcribe (openai-whisper's DecodingOptions subset that temperature fallback needs). */
typedef struct wm_decode_opts {
    float temperature;         /* 0: arg-max (tokens bit-identical to wm_transcribe_greedy); > 0: sample from
                                  softmax(filtered logits / temperature) */
    uint64_t seed;             /* sampling stream; ignored at temperature 0 */
    int32_t no_speech_token;   /* id of <|nospeech|> (50362 multilingual, 50363 large-v3); -1: not computed */
    int32_t sot_index;         /* index in prompt[] of <|startoftranscript|> (0 unless a previous-text prompt precedes it) */
} wm_decode_opts;

/* wm_transcribe_greedy with decoding options and two optional outputs; the same arguments, policies, grouping, filters
 * (wm_set_suppress, wm_set_timestamp_rules) and token budgets.  opts == NULL is temperature 0, no no-speech token.
 *   token_logprobs_out : f32 [B][max_new] (host, nullable): log-probability of every generated token under the FILTERED
 *                        distribution at temperature 1 -- logit[tok] - logsumexp(allowed logits), "allowed" being what the
 *                        suppress lists (the first-token list at the first generated token), the timestamp rules and, when
 *                        the rules force a timestamp, the admissible timestamps only leave (openai-whisper applies its
 *                        filters before log_softmax and does not divide by T there).  The token that stops a chunk (eot or
 *                        the last one its budget allows) has its value; 0 after it.  -INFINITY when nothing is admissible;
 *   no_speech_prob_out : f32 [B] (host, nullable; needs opts->no_speech_token >= 0): softmax probability of <|nospeech|>
 *                        in the RAW logits at the position of prompt[opts->sot_index] (openai-whisper DecodingTask).
 * Sampling (temperature T > 0) is Gumbel-max inside the fused logits kernel: token = arg-max over the allowed ids of
 * logit(n) * (float)(1 / T) + g(n), g = -log(-log u), u from Philox-4x32-10 with key {seed low, seed high word} and counter
 * {n >> 2, generated index, chunk index within THIS call, 0}, word n & 3 -> u = ((x >> 9) * 2 + 1) * 2^-24.  The
 * timestamp sum rule compares the unperturbed logits.  Results do not depend on the lanes, the grouping or the other
 * chunks of the call.  Invalid: temperature < 0, not finite or so small that
 * (float)(1 / temperature) overflows, sot_index outside [0, n_prompt), no_speech_token outside
 * the vocabulary, no_speech_prob_out without a token. */
WM_API int wm_transcribe(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, int B,
                  const int32_t *prompt, int n_prompt, int max_new, int32_t eot, const wm_decode_opts *opts,
                  int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out, float *no_speech_prob_out,
                  wm_mem mem);

/* wm_transcribe with log-mel windows instead of PCM chunks, and one prompt per row: the decode step of openai-whisper's
 * long-form transcribe(), whose windows start at any frame (`seek`).
 *   mel        : f32, mem-space selectable -- typically wm_logmel_long's output, kept on the device;
 *   mel_base   : i64 [B] (host) element offset in mel of row b's recording block [n_mels][mel_len[b]];
 *   mel_len    : i32 [B] (host) frames T of that block;  seek : i32 [B] (host) first frame, >= 0;
 *   n_frames   : i32 [B] (host) 1 .. 3000 frames, seek + n_frames <= mel_len.  Row b's encoder input is
 *                mel[:, seek : seek + n_frames] zero-padded to 3000 frames (openai-whisper pad_or_trim); the gather is
 *                fused into the encoder's first step.  With WM_MEM_HOST only the B windows are copied;
 *   prompts    : i32 [B][n_prompt] (host), every row its own prompt, all of one length; opts->sot_index applies to all;
 *   sample_ids : u32 [B] (host, nullable): the Philox counter word that wm_transcribe fills with the chunk index within
 *                THIS call is sample_ids[b] instead, so a row's sampling noise depends on its id, not on the other rows
 *                of the call; NULL: the index within the call, exactly as wm_transcribe;
 *   everything else (max_new, eot, opts, outputs, suppress / timestamp rules, token budgets, lanes, grouping, early stop)
 *   exactly as wm_transcribe.  Windows cut at seek 0 with 3000 frames from wm_logmel's output, with every prompt equal and
 *   sample_ids NULL, give wm_transcribe's results bit for bit.  Invalid: n_mels of the model other than the mel's (not
 *   checkable: the caller's duty), mel_len < 1, seek < 0, n_frames outside [1, 3000], seek + n_frames > mel_len,
 *   mel_base < 0, a prompt token outside the vocabulary, and everything wm_transcribe rejects. */
WM_API int wm_transcribe_mel(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                             const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts, int n_prompt,
                             const uint32_t *sample_ids, int max_new, int32_t eot, const wm_decode_opts *opts,
                             int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out, float *no_speech_prob_out,
                             wm_mem mem);

/* wm_transcribe_mel with prompts of DIFFERENT lengths in one call -- what openai-whisper's condition_on_previous_text needs:
 * every window's prompt carries the text its own recording produced so far.
 *   prompts    : i32 [B][prompt_stride] (host): row b's prompt is its first prompt_len[b] entries, the rest is not read;
 *   prompt_len : i32 [B] (host), each 1 .. prompt_stride;
 *   sot_tail   : <|startoftranscript|> is prompts[b][prompt_len[b] - sot_tail] in every row (the same distance from the END
 *                of every prompt: 3 for [..., sot, language, task]); read only when no_speech_prob_out is given.
 *                opts->sot_index is NOT read by this call;
 *   everything else exactly as wm_transcribe_mel.
 * Row b's tokens, length, log-probs and no-speech probability are those of wm_transcribe_mel on row b alone with its own
 * prompt (and sot_index = prompt_len[b] - sot_tail), bit for bit, whatever the other rows, the grouping and the lanes; with
 * all lengths equal the call IS wm_transcribe_mel.  Inside, each decode group right-aligns its rows to its own longest
 * prompt and steps through that many prompt positions.  Invalid: a prompt_len outside
 * [1, prompt_stride], sot_tail outside [1, min prompt_len] when no_speech_prob_out is given, max prompt_len + max_new >
 * n_text_ctx, a token outside the vocabulary among a row's first prompt_len[b], and everything wm_transcribe_mel rejects. */
WM_API int wm_transcribe_mel_ragged(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                    const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts,
                                    int prompt_stride, const int32_t *prompt_len, int sot_tail, const uint32_t *sample_ids,
                                    int max_new, int32_t eot, const wm_decode_opts *opts, int32_t *tokens_out,
                                    int32_t *lens_out, float *token_logprobs_out, float *no_speech_prob_out, wm_mem mem);

/* openai-whisper's best_of: wm_transcribe_mel_ragged (prompt_len given) or wm_transcribe_mel (prompt_len NULL: every prompt is
 * prompt_stride long and opts->sot_index applies) with best_of independently sampled CANDIDATES per window.  The candidates
 * of a window share its encoder pass, its cross-attention K/V cache and every read of that cache.
 *   best_of        : 1 .. WM_MAX_BEST_OF candidates per window;
 *   candidate noise: candidate s of row b is sampled with Philox counter {n >> 2, generated index, id_b, s} -- the fourth word
 *                    is 0 in every other call -- id_b = sample_ids[b], or b when sample_ids is NULL;
 *   length_penalty : NaN (openai-whisper's None) or in [0, 1]: how best_out ranks (wm_rank_candidates);
 *   tokens_out     : i32 [B][best_of][max_new];  lens_out : i32 [B][best_of];
 *   token_logprobs_out : f32 [B][best_of][max_new], nullable (best_out is computed either way);
 *   no_speech_prob_out : f32 [B], nullable: candidate 0's (the raw logits at <|startoftranscript|> do not see the noise);
 *   best_out       : i32 [B], nullable: wm_rank_candidates over each row's candidates.
 * Bit for bit: best_of = 1 is wm_transcribe_mel_ragged / wm_transcribe_mel; candidate 0 of any call is that result; candidate
 * (b, s) depends on row b's window, prompt, id, s, the seed and the temperature only -- not on best_of, the other rows, the
 * grouping or the lanes.  Temperature 0 is allowed (all candidates equal, best_out 0).  Suppress lists and timestamp rules
 * apply per candidate; a token budget (wm_set_token_budgets, B entries) applies to every candidate of its row; early stop is
 * per candidate, and a window whose candidates have all stopped has its cross-K/V cache not read again.
 * Invalid: best_of outside its range, length_penalty neither NaN nor in [0, 1], and
 * everything the ragged / uniform call rejects. */
#define WM_MAX_BEST_OF 8
WM_API int wm_transcribe_mel_best_of(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                     const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts,
                                     int prompt_stride, const int32_t *prompt_len, int sot_tail, const uint32_t *sample_ids,
                                     int best_of, float length_penalty, int max_new, int32_t eot, const wm_decode_opts *opts,
                                     int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out,
                                     float *no_speech_prob_out, int32_t *best_out, wm_mem mem);

/* openai-whisper's MaximumLikelihoodRanker on the host (no GPU, no context): per row the candidate with the highest score.
 *   tokens [B][n_cand][max_new], lens [B][n_cand], token_logprobs [B][n_cand][max_new] as wm_transcribe_mel_best_of returns them;
 *   sum     = f64 sum of token_logprobs[0 .. lens) in index order (the stopping eot included);
 *   n_text  = tokens before the first eot;  penalty = n_text when length_penalty is NaN (1 when n_text is 0: the library's
 *             own rule where openai-whisper divides by zero), else ((5 + n_text) / 6) ** length_penalty;
 *   score   = sum / penalty; the FIRST maximal score wins; -inf is a legal score, all -inf: candidate 0;
 *   best_out [B];  score_out f64 [B][n_cand], nullable.
 * Invalid: null pointers, B or n_cand or max_new < 1, a length outside [0, max_new], length_penalty neither NaN nor in [0, 1]. */
WM_API int wm_rank_candidates(const int32_t *tokens, const int32_t *lens, const float *token_logprobs, int B, int n_cand,
                              int max_new, int32_t eot, float length_penalty, int32_t *best_out, double *score_out);

/* openai-whisper's beam search (BeamSearchDecoder, beam_size / patience): wm_transcribe_mel_ragged (prompt_len given) or
 * wm_transcribe_mel (prompt_len NULL) with beam_size BEAMS per window.  The beams of a window share its encoder pass, its
 * cross-attention K/V cache and every read of that cache, exactly as the candidates of wm_transcribe_mel_best_of do; after
 * every generated token the beams are re-parented on the device.  Per window and generated index:
 *   list      : every live beam's beam_size + 1 most probable tokens under the filtered distribution (suppress lists, timestamp
 *               rules incl. the sum rule -- the filters of the greedy decode), lp = logit - logsumexp(allowed) in f32, best
 *               first (by logit, equal logits: the lower id; -inf is never listed; fewer admissible ids: a shorter list);
 *   candidates: score = f32(sum_of_beam + lp); at the first generated token beam 0 alone contributes (all beams are equal);
 *               walked by descending score (ties: the lower beam, then the earlier list entry).  A candidate ending in eot is
 *               a finished hypothesis, kept while the window has fewer than max_candidates; any other becomes the next beam
 *               0, 1, ... until beam_size are taken.  Slots left empty are DEAD beams (sum -inf, eot padding, no candidates);
 *   a window with max_candidates finished hypotheses leaves the decode: its rows stop, its cross-K/V cache is not read again;
 *   finalize  : when max_new -- or the window's token budget (wm_set_token_budgets, B entries: the window's own max_new) -- is
 *               used up; with fewer than beam_size hypotheses finished, the live beams follow in descending-sum order until
 *               there are beam_size.  Hypothesis order: the finished ones as they finished, then those.
 *   beam_size      : 1 .. WM_MAX_BEAM;  max_candidates : 1 .. WM_MAX_BEAM_HYPS (openai-whisper: round(beam_size * patience));
 *   length_penalty : as wm_rank_candidates;  opts->temperature must be 0 (it plays no part);  eot < 0: nothing ever finishes;
 *   outputs, with S = max(beam_size, max_candidates):
 *   tokens_out i32 [B][S][max_new];  lens_out i32 [B][S] (a finished hypothesis counts its eot);  n_hyp_out i32 [B];
 *   sum_logprobs_out f32 [B][S]: the running f32 sum the search itself used;  token_logprobs_out f32 [B][S][max_new], nullable;
 *   slots past n_hyp: tokens eot, length 0, sum -inf;  no_speech_prob_out f32 [B], nullable: beam 0's;
 *   best_out i32 [B], nullable: the MaximumLikelihoodRanker over sum_logprobs and the tokens before eot, with the penalty
 *   rules of wm_rank_candidates (n_text == 0 counts as 1, the first maximal score wins).
 * Bit for bit: beam_size = 1 with max_candidates = 1 is wm_transcribe_mel / wm_transcribe_mel_ragged at temperature 0 -- tokens,
 * length and log-probs, and the sum is the in-order f32 sum of those log-probs; a window's result depends on its own window,
 * prompt and the beam parameters only, not on the other rows, the grouping or the lanes.
 * Invalid: beam_size or max_candidates outside their ranges, opts->temperature != 0, eot >= n_vocab, a null n_hyp_out or
 * sum_logprobs_out, and everything wm_transcribe_mel_best_of rejects. */
#define WM_MAX_BEAM 8
#define WM_MAX_BEAM_HYPS 16
WM_API int wm_transcribe_mel_beam(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                  const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts, int prompt_stride,
                                  const int32_t *prompt_len, int sot_tail, int beam_size, int max_candidates,
                                  float length_penalty, int max_new, int32_t eot, const wm_decode_opts *opts,
                                  int32_t *tokens_out, int32_t *lens_out, int32_t *n_hyp_out, float *sum_logprobs_out,
                                  float *token_logprobs_out, float *no_speech_prob_out, int32_t *best_out, wm_mem mem);

/* ------------------------------------------------------------- word-level timestamps --- */
/* openai-whisper's find_alignment (whisper/timing.py) on the GPU, for the text tokens a transcription produced (e.g. each
 * chunk's tokens from the temperature step of wm_transcribe that it kept).  Per chunk with text tokens t[0 .. n), all < eot:
 *   1. teacher-forced decoder pass over [*sot_seq, no_timestamps, *t, eot] (T = n_sot + n + 2 rows);
 *   2. per alignment head (layer, head), ascending: softmax over the audio frames [0, M), M = n_frames / 2, of the
 *      cross-attention scores q.k / 8 * qk_scale;  3. z-score per head and frame over the T rows (std with 1 / T);
 *   4. median filter of width medfilt_width along the frames, reflect padding (none when M <= medfilt_width / 2);
 *   5. mean over the heads, rows n_sot .. n_sot + n, negated: the cost matrix x[n + 1][M];
 *   6. dynamic time warping of x in f32 with openai-whisper's CPU cell rule (dtw_cpu; its CUDA path uses another tie order);
 *   7. start_frame_out[b][i], i = 0 .. n: the first audio frame (20 ms each) of row i on the path -- token i spans
 *      [start_frame[i], start_frame[i + 1]), a word of tokens [a, b) spans [start_frame[a], start_frame[b]);
 *   8. token_prob_out[b][i] = softmax(logits[n_sot + i][0 : eot])[t[i]] (raw logits; the word-probability input).
 *   pcm           : [B][480000] samples, host or device memory (mem); everything else is host memory;
 *   text_tokens   : i32 [B][max_text], n_text i32 [B] (0 .. max_text); n_frames i32 [B] mel frames (2 .. 3000), NULL = 3000;
 *   medfilt_width : odd, 1 .. 31 (openai-whisper: 7);  qk_scale finite (openai-whisper: 1.0);
 *   start_frame_out i32 [B][max_text + 1] (-1 past n; a chunk with n = 0 gets only -1), token_prob_out f32 [B][max_text]
 *   (nullable; 0 past n).
 * Every chunk runs its whole path (front end, encoder, cross K/V, teacher-forced pass) on this context's stream, in decode
 * groups of at most 128 chunks.  Results depend only on the chunk's own inputs (bit level).  Invalid: a text token < 0 or
 * >= eot, n_sot + max_text + 2 > n_text_ctx, n_frames outside [2, 3000], an even, non-positive or wider medfilt_width, a
 * qk_scale that is not finite. */
WM_API int wm_align(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, int B, const int32_t *sot_seq, int n_sot,
             int32_t no_timestamps, int32_t eot, const int32_t *text_tokens, const int32_t *n_text, int max_text,
             const int32_t *n_frames, int medfilt_width, float qk_scale, int32_t *start_frame_out, float *token_prob_out,
             wm_mem mem);

/* wm_align on log-mel windows, one start sequence per row: word-level timing inside openai-whisper's long-form seek loop,
 * where a round holds one window of every live recording (each with its own language token) and the text was decoded from
 * the whole-recording log-mel, not from a 30 s chunk's.
 *   mel, mel_base, mel_len, seek, n_frames, mem : the window description of wm_transcribe_mel (typically wm_logmel_long's
 *              output kept on the device; with WM_MEM_HOST only the B windows are copied).  Row b's encoder input is
 *              mel[:, seek : seek + n_frames] zero-padded to 3000 frames, and n_frames[b] is ALSO find_alignment's
 *              num_frames: the cost matrix has M = n_frames[b] / 2 audio frames.  n_frames 2 .. 3000, never NULL;
 *   sot_seqs : i32 [B][n_sot] (host): row b's teacher-forced sequence is [*sot_seqs[b], no_timestamps, *t_b, eot];
 *   everything else (text tokens, alignment heads, median filter, qk_scale, outputs and their -1 / 0 padding, groups of at
 *   most 128 rows, wm_last_stage_ms) exactly as wm_align.
 * Rows cut at seek 0 with 3000 frames from wm_logmel(..., WM_F32)'s output, every row carrying the same start sequence,
 * give wm_align's start_frame_out and token_prob_out bit for bit.  A row's results depend only on its own window, start
 * sequence and text: the same bits alone, among other rows, across decode groups, and for the same frames presented as
 * their own block at seek 0.  Invalid: everything wm_align rejects (n_frames non-null here), mel_len < 1, seek < 0,
 * seek + n_frames > mel_len, mel_base < 0, a null window pointer, a sot_seqs token outside the vocabulary. */
WM_API int wm_align_mel(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                        const int32_t *seek, const int32_t *n_frames, int B, const int32_t *sot_seqs, int n_sot,
                        int32_t no_timestamps, int32_t eot, const int32_t *text_tokens, const int32_t *n_text, int max_text,
                        int medfilt_width, float qk_scale, int32_t *start_frame_out, float *token_prob_out, wm_mem mem);

/* ------------------------------------------------------------- window sets --- */
/* Every call above that takes mel windows runs the encoder and the cross-attention K/V projection of its rows.  A caller that
 * decodes the same window more than once -- openai-whisper's temperature fallback (up to six decodes of a hard window), the
 * word-timestamp pass behind it, language identification on the first 30 s -- encodes it ONCE into a window set and reads the
 * set from then on: everything downstream of the encoder reads a window's cross-attention K/V only. */
typedef struct wm_windows wm_windows;

/* Encode W mel windows ONCE and keep their cross-attention K/V (bf16) on the device.  Window description and `mem` exactly as
 * wm_transcribe_mel (gather fused into the encoder's first step; WM_MEM_HOST copies only the windows).  Runs in decode groups
 * of at most 128 rows on the context's stream; returns when the set is complete.  W >= 1.
 * The set is immutable.  It remembers each window's n_frames, and the weights, dims and device it was made for: the context
 * that made it and every wm_clone of that context or of its parent may read it (the lanes inside a call are such clones), any
 * other context gets WM_ERR_INVALID.  Its store is an allocation of its own -- no call made between the encode and a read
 * disturbs it -- of W * n_text_layer * 2 * 1500 * n_text_state * 2 bytes: 246 MB PER WINDOW at large-v2 (11 MB at tiny), so
 * size sets by the memory you can spare.  A failed allocation is WM_ERR_NOMEM and leaks nothing.  Free the set before the
 * context.  Not supported by the debug library's all-f32 precision path (WM_ERR_STATE).
 * wm_last_stage_ms afterwards: [0] the window copies (WM_MEM_HOST), [1] encoder + cross-K/V projection + the copy into the
 * store, [2] 0. */
WM_API int  wm_windows_encode(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                              const int32_t *seek, const int32_t *n_frames, int W, wm_mem mem, wm_windows **out);
WM_API void wm_windows_free(wm_windows *w);            /* NULL: no-op; may synchronise the device */
WM_API int  wm_windows_count(const wm_windows *w);     /* W; a null set: -1 */
WM_API size_t wm_windows_bytes(const wm_windows *w);   /* device bytes held: W * n_text_layer * 2 * 1500 * n_text_state * 2 */

/* The mel calls over the windows of a set: (w, rows, B) in place of the five mel arguments and `mem`.
 *   rows : i32 [B] (host) indices into the set, any order, repeats allowed; NULL: 0 .. B - 1, and B must be the set's W;
 *   every output is host memory.
 * At the prefill of each decode group the rows' K/V is copied from the set into the lane (one launch) where the mel call
 * runs the encoder.  BIT FOR BIT the result of the corresponding mel call on the same windows, with every other promise of
 * that call: a row depends only on itself, not on the grouping or the lanes; token budgets, suppress lists, timestamp rules,
 * early stop as before.
 *   wm_transcribe_windows      = wm_transcribe_mel_best_of (so best_of = 1 is wm_transcribe_mel_ragged with prompt_len, and
 *                                wm_transcribe_mel with prompt_len NULL);
 *   wm_transcribe_windows_beam = wm_transcribe_mel_beam;
 *   wm_align_windows           = wm_align_mel, find_alignment's num_frames being the set's n_frames of the row (>= 2);
 *   wm_windows_detect_language = wm_encode of the window zero-padded to 3000 frames followed by wm_detect_language_probs
 *                                (probs nullable: wm_detect_language), B <= 128.
 * wm_last_stage_ms after wm_transcribe_windows(_beam) and wm_windows_detect_language: [0] the copy from the set, [1] 0,
 * [2] the decode loop / the decoder step; after wm_align_windows: [0] the copy, [1] and [2] as wm_align.
 * Invalid: a null set, a row outside [0, W), rows NULL with B != W, a set of another model, device or dims,
 * wm_align_windows on a window of fewer than 2 frames, and everything the mel counterpart rejects. */
WM_API int wm_transcribe_windows(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B, const int32_t *prompts,
                                 int prompt_stride, const int32_t *prompt_len, int sot_tail, const uint32_t *sample_ids,
                                 int best_of, float length_penalty, int max_new, int32_t eot, const wm_decode_opts *opts,
                                 int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out, float *no_speech_prob_out,
                                 int32_t *best_out);
WM_API int wm_transcribe_windows_beam(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B, const int32_t *prompts,
                                      int prompt_stride, const int32_t *prompt_len, int sot_tail, int beam_size,
                                      int max_candidates, float length_penalty, int max_new, int32_t eot,
                                      const wm_decode_opts *opts, int32_t *tokens_out, int32_t *lens_out, int32_t *n_hyp_out,
                                      float *sum_logprobs_out, float *token_logprobs_out, float *no_speech_prob_out,
                                      int32_t *best_out);
WM_API int wm_align_windows(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B, const int32_t *sot_seqs, int n_sot,
                            int32_t no_timestamps, int32_t eot, const int32_t *text_tokens, const int32_t *n_text, int max_text,
                            int medfilt_width, float qk_scale, int32_t *start_frame_out, float *token_prob_out);
WM_API int wm_windows_detect_language(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B, int32_t sot,
                                      int32_t lang_first, int32_t lang_last, int32_t *lang_idx, float *probs /* nullable */);

/* ------------------------------------------------------------- word timestamps from the decode's own pass --- */
/* wm_transcribe_mel_ragged (prompt_len NULL: wm_transcribe_mel) that ALSO aligns what it generates, from the cross-attention
 * queries the decode itself formed: no second, teacher-forced pass (wm_align_mel re-runs the decoder over the kept text, which
 * is 93 % of its cost).  This is how Hugging Face's return_token_timestamps works.  Every argument but medfilt_width, qk_scale
 * and start_frame_out is that call's, and tokens_out, lens_out, token_logprobs_out and no_speech_prob_out are BIT FOR BIT
 * that call's for the same arguments -- at any temperature, with suppress lists, timestamp rules, repetition rules, sequence
 * bias, token budgets, early stop and any lane count: the decoder layers with alignment heads form their query in a launch of
 * its own instead of inside the cross-attention launch (the same bits), and nothing else changes.
 * Row b, with a_b the prompt index of <|startoftranscript|> (prompt_len[b] - sot_tail; a uniform call: opts->sot_index, 0
 * without opts), P_b its prompt length, g[0 .. len_b) its generated tokens (a stopping eot included), M_b = n_frames[b] / 2:
 *   1. decoder rows: the inputs u = prompt[a_b .. P_b) ++ g[0 .. len_b - 1), R_b = (P_b - a_b) + len_b - 1 of them -- the last
 *      generated token is never fed; prompt positions in front of <|startoftranscript|> (previous text) are no rows;
 *   2. - 4. of wm_align over these R_b rows and the frames [0, M_b): softmax of q.k / 8 * qk_scale per alignment head
 *      (wm_set_alignment_heads, the same default), z-score per head and frame over the R_b rows (std with 1 / R_b), median
 *      filter of medfilt_width with reflect padding;
 *   5. -mean over the heads of the LAST len_b rows: matrix row k is the decoder position whose OUTPUT was g[k] -- wm_align's
 *      row meaning (the row in front of text token i belongs to token i), except that no row follows the final token
 *      (wm_align teacher-forces eot as an input, a decode never does);
 *   6. wm_align's DTW on [len_b][M_b];
 *   7. start_frame_out[b][k], k < len_b: the first frame of row k on the path; start_frame_out[b][len_b] = M_b; -1 behind.
 *   Degenerate rows: all -1 when len_b == 0 or n_frames[b] < 2 (the row decodes normally); R_b < 2 (one row: the standard
 *   deviation over the rows is zero) gives start_frame_out[b] = 0, M_b, -1 ...
 *   medfilt_width : odd, 1 .. 31;  qk_scale finite;  start_frame_out i32 [B][max_new + 1] (host).
 * The rows are the DECODE's: its prompt, with timestamp tokens interleaved when the timestamp rules are on -- not
 * openai-whisper's clean [sot, lang, task, <|notimestamps|>, text] pass; generated tokens >= eot (timestamps, the stopping
 * eot) have a row and a start frame like any other, and the host drops them (binding.py decode_alignment_text).
 * Token probabilities are NOT a new output: a word's probability on this path is exp(token_logprobs_out) -- the log-prob of
 * the FILTERED distribution the decode sampled from (suppress lists, timestamp rules, repetition rules and bias applied, at
 * temperature 1) -- which differs from wm_align's token_prob_out = softmax(raw logits[0 : eot]).
 * A decode group's capture buffer (R rows x alignment heads x 64 f32 per row of the call) and alignment workspace live in the
 * lane and grow on demand; a group holds as many rows as fit 2 GiB of them (wm_align's rule: large-v2's default 320 heads at
 * max_new 224 behind a 3-token start sequence -> 88 rows), so a call may run in more groups than its plain counterpart --
 * same bits.  A failed allocation is WM_ERR_NOMEM and leaks nothing.  wm_last_stage_ms[2] includes the alignment kernels
 * and the DTW.
 * A row's results depend on the row alone (as wm_transcribe_mel_ragged); scope and inheritance of every setting as there.
 * best_of > 1 and beam search: the four entries below.
 * Invalid: medfilt_width even or outside 1 .. 31, a qk_scale that is not finite, a null start_frame_out, in a ragged call a
 * sot_tail outside [1, the shortest prompt_len] (always read here), and everything the underlying call rejects.  The debug
 * library's all-f32 precision path answers WM_ERR_STATE. */
WM_API int wm_transcribe_mel_aligned(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                     const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts,
                                     int prompt_stride, const int32_t *prompt_len /* nullable */, int sot_tail,
                                     const uint32_t *sample_ids, int max_new, int32_t eot, const wm_decode_opts *opts,
                                     int medfilt_width, float qk_scale, int32_t *tokens_out, int32_t *lens_out,
                                     float *token_logprobs_out, float *no_speech_prob_out,
                                     int32_t *start_frame_out /* [B][max_new + 1] */, wm_mem mem);
/* ... over the windows of a set (wm_transcribe_windows with best_of 1): (w, rows, B) in place of the five mel arguments and
 * `mem`, M_b from the set's n_frames of the row.  Bit for bit wm_transcribe_mel_aligned on the same windows. */
WM_API int wm_transcribe_windows_aligned(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B, const int32_t *prompts,
                                         int prompt_stride, const int32_t *prompt_len /* nullable */, int sot_tail,
                                         const uint32_t *sample_ids, int max_new, int32_t eot, const wm_decode_opts *opts,
                                         int medfilt_width, float qk_scale, int32_t *tokens_out, int32_t *lens_out,
                                         float *token_logprobs_out, float *no_speech_prob_out,
                                         int32_t *start_frame_out /* [B][max_new + 1] */);

/* The aligned counterparts of the best-of and beam calls:
 *   wm_transcribe_mel_best_of_aligned     = wm_transcribe_mel_best_of
 *   wm_transcribe_windows_best_of_aligned = wm_transcribe_windows
 *   wm_transcribe_mel_beam_aligned        = wm_transcribe_mel_beam
 *   wm_transcribe_windows_beam_aligned    = wm_transcribe_windows_beam
 * each with the arguments of its plain counterpart plus medfilt_width, qk_scale and start_frame_out i32 [B][max_new + 1] (as in
 * wm_transcribe_mel_aligned).
 * Decode outputs: every output of the plain counterpart -- tokens, lengths, log-probs, sums, n_hyp, no_speech_prob, best_out --
 * is BIT FOR BIT that call's for the same arguments: at any temperature (best-of), with suppress lists, timestamp rules,
 * repetition rules, sequence bias, token budgets, early stop and any lane count.
 * Alignment output: best_out must not be null (WM_ERR_INVALID).  start_frame_out[b] belongs to the ONE hypothesis h =
 * best_out[b] of window b and follows wm_transcribe_mel_aligned's row rule applied to that hypothesis' own tokens g_h[0 ..
 * len_h): decoder rows prompt[a_b .. P_b) ++ g_h[0 .. len_h - 1), the cost matrix their last len_h rows, the DTW on [len_h][M_b],
 * start_frame_out[b][len_h] = M_b and -1 behind.  Degenerate cases as there: len_h == 0 or n_frames[b] < 2 gives all -1, fewer
 * than 2 decoder rows give 0, M_b.  The other hypotheses of a window get NO alignment: a host that ranks the hypotheses by a rule
 * of its own aligns its choice with wm_align_mel.
 * best_of 1 is wm_transcribe_mel_aligned bit for bit, start frames included, and so is beam_size 1 with max_candidates 1; at
 * temperature 0 a best-of call aligns candidate 0.
 * Every candidate / beam of a window keeps its queries while the decode runs (a beam search re-parents its beams after every
 * token: the rows stay where they were captured and the search records which beam each row continued), so a window counts
 * best_of / beam_size rows, the chosen hypothesis' gathered queries and the window's own statistics and cost matrix towards the
 * 2 GiB a group may hold; groups are made of whole windows.  A window's results depend on the window alone.
 * Invalid: a null best_out, and everything the plain counterpart and wm_transcribe_mel_aligned reject.  The debug library's
 * all-f32 precision path answers WM_ERR_STATE. */
WM_API int wm_transcribe_mel_best_of_aligned(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                             const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts,
                                             int prompt_stride, const int32_t *prompt_len /* nullable */, int sot_tail,
                                             const uint32_t *sample_ids, int best_of, float length_penalty, int max_new,
                                             int32_t eot, const wm_decode_opts *opts, int medfilt_width, float qk_scale,
                                             int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out,
                                             float *no_speech_prob_out, int32_t *best_out,
                                             int32_t *start_frame_out /* [B][max_new + 1] */, wm_mem mem);
WM_API int wm_transcribe_windows_best_of_aligned(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B,
                                                 const int32_t *prompts, int prompt_stride, const int32_t *prompt_len /* nullable */,
                                                 int sot_tail, const uint32_t *sample_ids, int best_of, float length_penalty,
                                                 int max_new, int32_t eot, const wm_decode_opts *opts, int medfilt_width,
                                                 float qk_scale, int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out,
                                                 float *no_speech_prob_out, int32_t *best_out,
                                                 int32_t *start_frame_out /* [B][max_new + 1] */);
WM_API int wm_transcribe_mel_beam_aligned(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                          const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts,
                                          int prompt_stride, const int32_t *prompt_len /* nullable */, int sot_tail, int beam_size,
                                          int max_candidates, float length_penalty, int max_new, int32_t eot,
                                          const wm_decode_opts *opts, int medfilt_width, float qk_scale, int32_t *tokens_out,
                                          int32_t *lens_out, int32_t *n_hyp_out, float *sum_logprobs_out, float *token_logprobs_out,
                                          float *no_speech_prob_out, int32_t *best_out,
                                          int32_t *start_frame_out /* [B][max_new + 1] */, wm_mem mem);
WM_API int wm_transcribe_windows_beam_aligned(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B, const int32_t *prompts,
                                              int prompt_stride, const int32_t *prompt_len /* nullable */, int sot_tail,
                                              int beam_size, int max_candidates, float length_penalty, int max_new, int32_t eot,
                                              const wm_decode_opts *opts, int medfilt_width, float qk_scale, int32_t *tokens_out,
                                              int32_t *lens_out, int32_t *n_hyp_out, float *sum_logprobs_out,
                                              float *token_logprobs_out, float *no_speech_prob_out, int32_t *best_out,
                                              int32_t *start_frame_out /* [B][max_new + 1] */);

/* The alignment heads wm_align, wm_align_mel and the aligned transcribe calls read: n (layer, head) pairs, any order (used ascending).  n = 0 restores the default, every
 * head of the decoder layers n_text_layer / 2 .. n_text_layer - 1 (openai-whisper's default when a checkpoint has no list);
 * a checkpoint's own list (openai-whisper _ALIGNMENT_HEADS, Hugging Face generation_config.alignment_heads) comes from the
 * host.  Out-of-range pairs and duplicates are invalid.  Same inheritance as wm_set_suppress. */
WM_API int wm_set_alignment_heads(wm_ctx *ctx, const int32_t *layers, const int32_t *heads, int n);

/* Positions per decoder step of the TEACHER-FORCED passes: wm_align, wm_align_mel, wm_align_windows and wm_decode_logits
 * (every token of such a pass is known up front).  With width w a step carries w consecutive positions of every window: the
 * pass runs ceil(T / w) steps of up to WM_DEC_MAXB = 128 rows instead of T steps of B rows, streams the decoder weights once
 * per w positions and reads a window's cross-attention K/V once per step for all w of them.
 *   width : 1 .. WM_MAX_TEACHER_PANEL; 1 (the default) enqueues exactly the launches the pass always enqueued.
 * A LAUNCH POLICY, NOT A NUMERICS SWITCH: every output of these calls (start frames, token probabilities, logits) is
 * bit-identical for every width -- a row's arithmetic is the one-position step's, only the rows that share a launch change.
 * The transcribe entries and wm_detect_language* are not affected.  WM_ERR_INVALID: width outside the range.  Same
 * inheritance as wm_set_suppress (later wm_clone's and the lanes of a call take the setting over). */
#define WM_MAX_TEACHER_PANEL 8   /* = WM_MAX_BEST_OF: the widths the shared cross-attention read is built for */
WM_API int wm_set_teacher_panel(wm_ctx *ctx, int width);

/* PROMPT PANELS: positions per decoder step over the PROMPT of a transcribe call (the previous text of a conditioned long-form
 * run above all).  A decode group steps through its prompt one position per step, each with the full logits product, although
 * only the last positions' logits are read.  With width w > 1 the positions [0, P0) in front of the first one the call reads
 * run as teacher-forced panel steps instead -- w consecutive positions of every row per step, the decoder weights streamed
 * once and a window's cross-attention K/V read once per step, NO logits product and no close -- and the group's ordinary steps
 * begin at P0:
 *   P0 = the <|startoftranscript|> position (opts->sot_index; a ragged call: prompt_len - sot_tail of the group's longest
 *        prompt) when the call computes no_speech_prob, else the prompt's last position P - 1; an aligned call caps it at its
 *        first captured position (<|startoftranscript|>).  A ragged group's rows are right-aligned as always; P is its longest.
 *   width : 1 .. WM_MAX_TEACHER_PANEL; 1 (the default) enqueues exactly the launches a call always enqueued, and so does any
 *           width for a group with P0 < 2.  Groups of more rows than 128 / w are cut like the teacher-forced passes.
 * A LAUNCH POLICY, NOT A NUMERICS SWITCH: tokens, lengths, token log-probs, no_speech_prob and start frames are bit-identical
 * for every width.  TAKING PART: the plain groups of wm_transcribe_greedy, wm_transcribe, wm_transcribe_mel,
 * wm_transcribe_mel_ragged, wm_transcribe_windows, wm_transcribe_mel_aligned and wm_transcribe_windows_aligned, under explicit
 * lanes and sub-chip parts too.  IGNORING THE WIDTH (they step through their prompts as always, and do not reject the
 * setting): the best-of and beam-search entries, both models of wm_transcribe_mel_speculative, the all-f32 debug path.  The
 * panel steps run eagerly, not from captured graphs; no graph is dropped by this call.  WM_ERR_INVALID: width outside the
 * range.  Same inheritance as wm_set_suppress. */
WM_API int wm_set_prompt_panel(wm_ctx *ctx, int width);

/* SPECULATIVE DECODING: wm_transcribe_mel on `ctx` (the target) whose tokens a small DRAFT model proposes.  Per round the draft
 * proposes up to draft_len tokens with plain greedy steps, the target checks all of them in ONE panel step (up to draft_len + 1
 * consecutive positions of every window: the weights streamed once, a window's cross-attention K/V read once) and keeps the
 * longest prefix it would have produced itself, plus its own next token.
 * THE CONTRACT: tokens_out, lens_out, token_logprobs_out and no_speech_prob_out are bit for bit those of wm_transcribe_mel on
 * `ctx` with the same arguments -- for every draft, every draft_len and every grouping, with wm_set_suppress lists (the
 * first-token list included), wm_set_timestamp_rules, wm_set_token_budgets, early stop on eot and eot < 0.  A panel row has
 * the one-position step's bits; the draft decides how many rounds a call takes, never what it returns.
 *   draft     : a finalised model context on the same device, with its own weights (a wm_clone of ctx, or a second context with
 *               the same weights, is legal and has every proposal accepted).  Its n_mels, n_vocab, n_text_ctx and n_audio_ctx
 *               must equal the target's.  It runs its own encoder over the same windows.  Its OWN suppress lists and timestamp
 *               rules shape what it proposes -- they affect acceptance, never the result: set them as on the target.  Nothing
 *               else may use the draft context during the call.
 *   draft_len : 1 .. WM_MAX_DRAFT_LEN proposals per round.
 *   stats_out : nullable, [B]: what the draft was worth, per window (wm_spec_stats).
 * The windows of a call are decoded in groups of windows that advance in LOCKSTEP: a round advances a group by the smallest
 * number of tokens any of its live windows could keep, so a group's acceptance is that of its worst window, round by round.
 * The groups run one after the other on ctx's stream; wm_set_lanes is not consulted.
 * NOT OFFERED (each rejected with its own message): a non-zero temperature (WM_ERR_INVALID); repetition rules or a sequence
 * bias set on ctx (WM_ERR_STATE); the all-f32 debug path (WM_ERR_STATE).  There are no ragged-prompt, best-of, beam-search,
 * aligned or window-set forms of this call.  Every other argument and error: wm_transcribe_mel (sample ids play no part at
 * temperature 0). */
#define WM_MAX_DRAFT_LEN 7          /* draft_len + 1 <= WM_MAX_TEACHER_PANEL */
typedef struct wm_spec_stats {
    int32_t rounds;                 /* verify steps the window took part in while live */
    int32_t proposed;               /* draft tokens verified for it */
    int32_t accepted;               /* of those, equal to the target's own choice (the leading run) */
    int32_t kept;                   /* of those, kept after the group's lockstep cut */
} wm_spec_stats;
WM_API int wm_transcribe_mel_speculative(wm_ctx *ctx, wm_ctx *draft, const float *mel, const int64_t *mel_base,
                                         const int32_t *mel_len, const int32_t *seek, const int32_t *n_frames, int B,
                                         const int32_t *prompts, int n_prompt, int draft_len, int max_new, int32_t eot,
                                         const wm_decode_opts *opts, int32_t *tokens_out, int32_t *lens_out,
                                         float *token_logprobs_out /* nullable */, float *no_speech_prob_out /* nullable */,
                                         wm_spec_stats *stats_out /* nullable */, wm_mem mem);

/* Decode groups a wm_transcribe_greedy call on this context keeps in flight.
 *   0 (default): the library's own measured policy -- one group below 32 chunks, two groups (two weight-sharing lanes)
 *                up to 143, three from 144 chunks, never more than $WM_LANES (default 3) at once; for the NARROW models
 *                (decoder width <= 512: tiny, base) the two groups of a 24 .. 128-chunk call (tiny: 32 .. 47) run on two
 *                SUB-CHIP lanes -- streams confined by a CU mask to complementary halves of every XCD's CUs (round 6:
 *                +2 .. +9 % there; a wide model's decode needs all the CUs and is never split this way);
 *   1          : the whole call (up to 128 chunks) is ONE decode group on the context's own stream -- what a host that runs
 *                its own concurrency over wm_clone'd contexts wants (bench.py);
 *   n = 2 .. 8 : n groups in flight whenever the call has 8 chunks for each (groups of ~8 up to 8 n chunks, n balanced
 *                groups of up to 128 beyond): a host that knows its latency / throughput trade-off better than the default.
 * Tokens do not depend on the choice (bit-level batch invariance).
 * EARLY STOP TRADE-OFF (eot >= 0 or wm_set_token_budgets): a decode group runs until its LAST row is finished, so the
 * default's single group below 32 chunks -- measured with fixed-length decodes, where it is the fastest cut -- decodes a
 * 24-chunk call with one straggler for ~0.8 of a full decode, where three groups of 8 (wm_set_lanes(3)) would have
 * spent ~0.6-0.7 (each group stops on its own).  A host whose utterance lengths vary widely and whose calls are 9 .. 31
 * chunks may prefer wm_set_lanes(2) or (3); the default is tuned for throughput at fixed length. */
WM_API int wm_set_lanes(wm_ctx *ctx, int n_lanes);

/* Logit filters of openai-whisper's greedy decode() (whisper/decoding.py SuppressTokens and SuppressBlank; SURVEY.md 8f
 * rank 3), applied inside the fused logits / arg-max kernel of wm_transcribe_greedy:
 *   suppress       : n token ids that are never generated (e.g. the tokenizer's non-speech tokens, sot, translate, ...);
 *   suppress_first : n_first more ids excluded only for the FIRST generated token (SuppressBlank: " " and <|endoftext|>).
 * The lists are copied; n = n_first = 0 clears the filter.  wm_decode_logits / wm_detect_language are unaffected (raw
 * logits).  Contexts made later with wm_clone inherit the filter; existing clones must be set themselves. */
WM_API int wm_set_suppress(wm_ctx *ctx, const int32_t *suppress, int n, const int32_t *suppress_first, int n_first);

/* openai-whisper's ApplyTimestampRules (whisper/decoding.py [3p]) for wm_transcribe_greedy, i.e. decoding WITH
 * timestamps (prompt without <|notimestamps|>): timestamps come in pairs, never decrease, the transcript opens with a
 * timestamp no later than max_initial_timestamp_index (e.g. 50 = 1.0 s; < 0: unlimited), and a timestamp is forced
 * whenever the summed probability of the admissible timestamps exceeds the best admissible text token.
 *   timestamp_begin : id of <|0.00|> (50364; 50365 for large-v3);  eot : <|endoftext|>.
 * Evaluated inside the fused logits / arg-max kernels; combine with wm_set_suppress (which should list <|notimestamps|>).
 * enable = 0 switches the rules off.  Same inheritance as wm_set_suppress. */
WM_API int wm_set_timestamp_rules(wm_ctx *ctx, int enable, int32_t timestamp_begin, int32_t eot,
                           int32_t max_initial_timestamp_index);

/* The repetition rules: repetition_penalty and no_repeat_ngram_size of faster-whisper / CTranslate2 and Hugging Face generate,
 * the remedy for Whisper's repetition loop that needs no second decode.  Both are logit processors over a row's own
 * GENERATED history g[0 .. k) -- the tokens the row has generated in this call, prompt excluded (Hugging Face counts the
 * prompt; here a previous-text prompt would otherwise penalise exactly the words most likely to continue; in a ragged call
 * every row's history starts after its own prompt just the same).  Only ids < eot are ever penalised or banned: timestamps,
 * <|endoftext|> and the specials are left to the timestamp rules and the suppress lists, but ids >= eot still stand in the
 * history and take part in n-gram matching as themselves.
 *   repetition_penalty p (finite, > 0; 1.0 = off): every eligible id t that occurs in g -- once, however often it occurs --
 *     has its logit replaced by v > 0 ? v * inv_p : v * p with inv_p = (float)(1.0 / (double)p): one f32 multiply either way.
 *     (HF / CT2 divide a positive logit by p: the results differ by at most one ulp.)
 *   no_repeat_ngram_size n (0 = off, else 1 .. 32): eligible id t is banned at this position iff there is an i in [0, k - n]
 *     with g[i .. i + n - 1) == g[k - n + 1 .. k) and g[i + n - 1] == t.  Nothing is banned while k < n - 1; n = 1 bans every
 *     eligible id that was already generated.
 * The penalised value replaces the logit before everything the decode does with it (arg-max, the sampling score
 * v / T + Gumbel noise, the log-prob normalisers, the timestamp sum rule, beam lists); a banned id is treated exactly like a
 * suppressed one.  no_speech_prob is read at <|startoftranscript|>, where the history is empty: untouched.  If the bans leave
 * no admissible text token the existing paths apply (a forced timestamp, the fallback token, log-prob -inf).
 * Applies to every transcribe entry (wm_transcribe_greedy, wm_transcribe, _mel, _ragged, _best_of, _beam, wm_transcribe_windows*);
 * wm_decode_logits, wm_detect_language* and wm_align* are teacher-forced and stay raw.  With the rules set a call runs the
 * extended decode (the one behind log-probs and sampling), which at temperature 0 produces wm_transcribe_greedy's tokens bit
 * for bit.  (1.0, 0, any valid eot) switches the rules off.  WM_ERR_INVALID: p not finite or <= 0, n outside [0, 32], eot
 * outside [0, n_vocab].  Same inheritance as wm_set_suppress. */
WM_API int wm_set_repetition_rules(wm_ctx *ctx, float repetition_penalty, int no_repeat_ngram_size, int32_t eot);

/* The sampling rules: top_k, top_p and min_p of Hugging Face generate (CTranslate2 / faster-whisper: sampling_topk,
 * sampling_topp) -- the distribution a sampling call draws from is truncated, on the device, before the draw.  The rules act
 * at every generated position of a row whose call samples (opts->temperature > 0); a call at temperature 0 (wm_transcribe_greedy,
 * beam search and speculative calls among them) ignores them completely and makes the launches it makes without them.
 *   A, the admissible set: exactly the ids the call may draw today -- the suppress lists (the first-token list too), the timestamp
 *     rules (when the sum rule forces a timestamp, A is the admissible timestamps alone), the no-repeat bans, the sequence-bias
 *     bans.  v(n): the logit after the repetition penalty and the sequence bias.
 *   Order: descending value, equal values lower id first.  An id whose value is -INFINITY is never kept.
 *   Masses: m(n) = exp((v(n) - vmax) * inv_T) with inv_T = (float)(1 / T) as the call uses it and vmax the best value in A.
 *   The kept set K is the shortest prefix of A in that order that satisfies every active rule, applied in Hugging Face's
 *     sequence -- temperature, top_k, top_p over what top_k left, min_p -- and never holds fewer than one id:
 *       top_k > 0  : at most top_k ids.  EXACTLY k: Hugging Face keeps every id tied with the k-th, this library the lowest ids
 *                    among the ties.  top_k >= |A| keeps all.
 *       top_p < 1  : with Z_k the mass of the top_k prefix, the shortest prefix whose mass is >= top_p * Z_k.
 *       min_p > 0  : only ids with m(n) >= min_p (a threshold relative to the best id, so the renormalisations do not move it).
 *   Draw: the token is the arg-max over K of fmaf(v(n), inv_T, g(n)) with the Gumbel noise g(n) of the same Philox counters as
 *     without the rules (id quad, generated index, sample id or call index, candidate word): top_k >= |A| reproduces the
 *     untruncated call bit for bit, top_k = 1 the temperature-0 call.
 *   Unchanged: token_logprobs_out stays v[tok] - logsumexp(A) at temperature 1 -- the truncation is NOT part of the normaliser
 *     (openai-whisper's thresholds and the rankers are calibrated on that; Hugging Face reports post-warper scores);
 *     no_speech_prob; the sum rule compares unperturbed values; an empty A takes the existing path (forced timestamp, fallback
 *     token, log-prob -inf).
 *   Determinism: K and the token depend on the row's own values, ids and seed alone -- masses are summed as 64-bit fixed point
 *     (rint(m * 2^40)), never as floats -- not on the group's shape, the lanes, the other rows or the run.
 * Scope: wm_transcribe, _mel, _ragged, _best_of (every candidate of a row gets the same rules and its own noise), the
 * wm_transcribe_windows* counterparts, the *_aligned entries, and wm_multi_* device contexts when set there.  Teacher-forced
 * calls stay raw.  (0, 1.0f, 0.0f) switches the rules off and is the initial state.  WM_ERR_INVALID: top_k < 0, top_p outside
 * (0, 1], min_p outside [0, 1), a NaN.  The all-f32 debug path answers WM_ERR_STATE.  Applied to every lane and copied by later
 * wm_clone's, as wm_set_repetition_rules.  Cost: one launch per generated position and the stored f32 logits row (DESIGN.md
 * section 20). */
WM_API int wm_set_sampling_rules(wm_ctx *ctx, int top_k, float top_p, float min_p);

/* The sequence bias: Hugging Face generate's sequence_bias, and with it bad_words_ids (CTranslate2's suppress_sequences) and
 * phrase boosting (contextual biasing: product names, people, jargon).  A token sequence carries a bias, and the bias is added
 * to the logit of its LAST token whenever the row's history ends in its other tokens.
 *   History: g[0 .. k), the row's GENERATED tokens of this call, exactly as for wm_set_repetition_rules (prompt excluded, a
 *     ragged row counts from its own prompt's end, a beam row has the history of the hypothesis it continues).
 *   Entries: n_seq sequences, sequence i = tokens[seq_offsets[i] .. seq_offsets[i + 1]) with 1 <= length <= WM_MAX_BIAS_SEQ_LEN
 *     and bias[i].  Every token in [0, n_vocab); the LAST token < eot (only text ids are ever biased or banned); ids >= eot may
 *     stand inside a sequence and match as themselves.  bias[i] is finite or -INFINITY.  Two sequences with identical tokens
 *     are invalid.
 *   Match: at a position, entry s[0 .. n) matches a row iff n == 1, or k >= n - 1 and g[k - n + 1 .. k) == s[0 .. n - 1).
 *   Effect: total(t) is an f32 sum that starts at +0.0f and adds the bias of every matching entry whose last token is t, in the
 *     order the entries were given (an implicit entry, below, follows the entry that produced it).  The logit becomes
 *     v[t] + total(t): one f32 add.  A total of -INFINITY is a BAN: the id is treated exactly like a suppressed one.  Fed the
 *     same order this is, bit for bit, Hugging Face's SequenceBiasLogitsProcessor over the generated tokens, and with -INFINITY
 *     its NoBadWordsLogitsProcessor.
 *   Boosted prefixes: boost_prefixes[i] != 0 (the array may be NULL: none) needs a finite bias and adds, for every proper
 *     prefix s[0 .. j), 1 <= j < n, an IMPLICIT entry with the same bias, so that a multi-token phrase is helped from its first
 *     token on.  Implicit entries with identical tokens merge into one that carries the MAXIMUM bias (two phrases that share a
 *     first word boost it once, as a trie would) and stands where the first of them stood; an implicit entry identical to a
 *     given sequence is dropped, and so is a prefix that ends in an id >= eot.  At most WM_MAX_BIAS_ENTRIES entries after the
 *     expansion.
 *   Order: the repetition penalty multiplies first, then the bias is added; the bans of both rules are OR-ed.  The biased value
 *     replaces the logit before everything the decode does with it (arg-max, sampling score, log-prob normalisers, the timestamp
 *     sum rule, the stored f32 row, beam lists).  no_speech_prob is read from the raw logits: single-token entries do not touch
 *     it.
 * Ids are the caller's tokenizer's: Whisper's " word" and "word" are different ids, and both variants are the caller's to list.
 * Scope and inheritance as wm_set_repetition_rules: every transcribe entry, the teacher-forced calls stay raw, the call runs the
 * extended decode, the all-f32 debug path answers WM_ERR_STATE; applied to every lane, copied by later wm_clone's.  n_seq = 0
 * switches it off (the other pointers may then be NULL).  WM_ERR_INVALID -- and the table in force stays -- for a token outside
 * the vocabulary, a last token >= eot, a length of 0 or above 32, offsets that do not start at 0 or decrease, a NaN or +INFINITY
 * bias, a duplicate sequence, -INFINITY with boost_prefixes, more than WM_MAX_BIAS_ENTRIES entries, eot outside [0, n_vocab].
 * Cost, measured: + 6 .. 15 us per decode position with 8 entries (base x 32 rows, large-v2 x 56) -- two
 * state launches and the wider epilogue --, + 12 us / + 27 us with WM_MAX_BIAS_ENTRIES entries that ALL match every row: below
 * the logits launch itself (35 / 82 us), 3.8 % / 0.6 % of a position. */
#define WM_MAX_BIAS_SEQ_LEN 32      /* tokens per sequence (as no_repeat_ngram_size)              */
#define WM_MAX_BIAS_ENTRIES 4096    /* entries after prefix expansion (a full table costs less than the logits launch) */
WM_API int wm_set_sequence_bias(wm_ctx *ctx, const int32_t *tokens, const int32_t *seq_offsets /* [n_seq + 1] */,
                                const float *bias /* [n_seq] */, const uint8_t *boost_prefixes /* [n_seq], nullable */,
                                int n_seq, int32_t eot);

/* Row tables: a sequence-bias table PER ROW of a call, so that requests with different phrase lists (a call's agent roster, a
 * meeting's attendees, a customer's catalogue) decode in ONE batched call instead of one context and one call per table.
 *   Tables: wm_set_sequence_bias_tables gives the context n_tables tables; table t is sequences [table_offsets[t],
 *     table_offsets[t + 1]) of the n_seq = table_offsets[n_tables] sequences, which are given exactly as for
 *     wm_set_sequence_bias.  Every table is checked and expanded ON ITS OWN by that call's rules and limits (32 tokens,
 *     WM_MAX_BIAS_ENTRIES entries after the expansion; duplicates are invalid within a table only); a table may be empty.  At most
 *     WM_MAX_BIAS_TABLES tables and WM_MAX_BIAS_POOL entries after the expansion, all tables together.
 *   Rows: wm_set_bias_rows names the table of every row of the NEXT transcribe call on the context, like wm_set_token_budgets: it
 *     is consumed by that call whatever happens, and n must equal its B.  Row b (a chunk, a window) uses table table_of_row[b];
 *     -1: no bias.  Every candidate of a best-of window and every beam of a beam window uses its window's table.  n = 0 drops a
 *     pending map.  WM_ERR_STATE when the context has no tables; WM_ERR_INVALID for an index outside [-1, n_tables).
 *   A row with table t gives, bit for bit, what the same call gives that row with t as the context's single table: history,
 *     match, the f32 total in table order, bans, boosted prefixes and the order with the repetition rules are
 *     wm_set_sequence_bias's over that table alone.  A row on -1 or on an empty table decodes as with the bias off (the call
 *     still runs the extended decode).
 *   Exclusive with the single table: a successful wm_set_sequence_bias_tables replaces it; wm_set_sequence_bias with n_seq > 0
 *     replaces the tables, with n_seq = 0 it clears both.  n_tables = 0 clears the tables and a pending map (the other pointers
 *     may then be NULL).  Either call drops a pending map.
 *   Scope: every entry the single table serves.  With tables in force a transcribe call WITHOUT a pending map answers
 *     WM_ERR_STATE; a map whose n differs from the call's B, or with an index outside [-1, n_tables), WM_ERR_INVALID.
 *     wm_transcribe_mel_speculative and the all-f32 debug path answer WM_ERR_STATE, as for the single table, and so does
 *     wm_multi_transcribe_greedy on a device context with tables (not built).  The teacher-forced calls stay raw.  Applied to
 *     every lane, copied by later wm_clone's.
 * WM_ERR_INVALID -- and whatever was in force stays -- for anything wm_set_sequence_bias refuses in any table, table_offsets that
 * do not start at 0, decrease or (through seq_offsets) leave the sequences, more than WM_MAX_BIAS_TABLES tables, a pool above
 * WM_MAX_BIAS_POOL entries.
 * Cost, measured: the single table's per position plus 0 .. 2 us -- large-v2 x 56 rows + 13.5 us with
 * 8 entries per row, + 30.8 us with full tables of 4096 entries that all match (single table, same build: + 13.4 / + 29.0); the
 * state launch walks each row's own table instead of the one table, the logits launch and its epilogue are the same. */
#define WM_MAX_BIAS_TABLES 1024     /* tables of one context                                  */
#define WM_MAX_BIAS_POOL   65536    /* entries after prefix expansion, all tables together    */
WM_API int wm_set_sequence_bias_tables(wm_ctx *ctx, const int32_t *tokens, const int32_t *seq_offsets /* [n_seq + 1] */,
                                       const float *bias, const uint8_t *boost_prefixes /* nullable */,
                                       const int32_t *table_offsets /* [n_tables + 1], into the sequences */,
                                       int n_tables, int32_t eot);
WM_API int wm_set_bias_rows(wm_ctx *ctx, const int32_t *table_of_row /* [n], -1 .. n_tables - 1 */, int n);

/* Constrained decoding: an AUTOMATON over token ids says, position by position, which ids a row may generate -- "one of these
 * phrases", "digits only", "`call ` followed by free text" (whisper.cpp's grammars, Hugging Face generate's
 * prefix_allowed_tokens_fn).  A bias tilts the odds and a ban list cannot say "nothing else"; this is the hard rule.
 *   Automaton: S states (1 <= S <= WM_MAX_CST_STATES) and E explicit edges (0 <= E <= WM_MAX_CST_EDGES) as flat arrays:
 *     edge_beg[S + 1] (state s owns edges [edge_beg[s], edge_beg[s + 1]), E = edge_beg[S]), edge_tok[E] (strictly ascending
 *     within a state), edge_next[E], def_next[S], accept[S] (u8), and eot.
 *   Explicit edge (s, t) -> n: t is a text id in [0, eot).  n in [0, S): id t is allowed in state s and leads to n.  n = -1: t is
 *     forbidden in s -- valid only where def_next[s] >= 0 ("anything but").
 *   Default def_next[s]: -1, a text id without an explicit edge is forbidden in s; >= 0, every such id is allowed and leads
 *     there (free-text stretches, wildcards).
 *   Accepting: eot is allowed in state s iff accept[s] != 0.
 *   Ids above eot (timestamps, the specials) are TRANSPARENT: the constraint never bans them and they do not move the state,
 *     delta(s, t) = s; eot itself behaves the same way where it stands in the history as the padding of a finished row.  They stay
 *     the business of the timestamp rules and the suppress lists, so `<|0.00|> turn left <|1.20|>` is the phrase `turn left`.
 *   Dead state -1: reached by a text id the state forbids (possible only through an existing empty-set fallback path); it allows
 *     eot alone and stays dead.
 *   History: g[0 .. k), the tokens the row has generated in this call, exactly as for wm_set_repetition_rules -- the prompt is
 *     excluded, a ragged row counts from the group's longest prompt, a beam row carries the history of the hypothesis it continues.
 *   State of a row at a position: delta folded over g[0 .. k) from the row's start state -- a pure function of the history.
 *   Effect: every id in [0, eot] the state does not allow is BANNED at that position, together with the no-repeat bans and the
 *     sequence-bias bans, and a banned id is treated exactly like a suppressed one everywhere: the arg-max, the Gumbel draw, the
 *     log-prob normaliser, the sum rule of the timestamp rules, the beam lists, the kept set of the sampling rules, the
 *     alternatives.  The stored f32 logit is unchanged (as for a no-repeat ban), token_logprobs_out is the log-prob under the
 *     CONSTRAINED distribution, no_speech_prob is untouched.  An empty admissible set takes the path it always took.  When
 *     max_new or a token budget runs out before an accepting state, the output is a PREFIX of a member of the language.
 *   wm_set_constraint(n_states = 0) switches the constraint off (the initial state; the pointers may be NULL).  Applied to every
 *     lane and copied by later wm_clone's, as wm_set_repetition_rules.  It drops a pending row map.
 *   Rows: wm_set_constraint_rows names the start state of every row of the NEXT transcribe call on the context, like
 *     wm_set_bias_rows: consumed by that call whatever happens, n must equal its B, n = 0 drops a pending map.  Row b starts in
 *     state start_of_row[b]; -1: the row is unconstrained and decodes as with the constraint off.  Every candidate of a best-of
 *     window and every beam of a beam window takes its window's start.  With an automaton in force and no pending map every row
 *     starts in state 0.  One automaton that holds disjoint sub-automata is therefore a grammar per request in one batched call.
 *     WM_ERR_STATE when the context has no automaton; WM_ERR_INVALID for a start outside [-1, S).
 *   Served: wm_transcribe_greedy (the constraint turns the extended decode on, as the repetition rules do), wm_transcribe, _mel,
 *     _mel_ragged, _mel_best_of, _mel_beam, the wm_transcribe_windows* counterparts and the *_aligned entries.  Refused with
 *     WM_ERR_STATE (not built): wm_transcribe_mel_speculative, wm_multi_transcribe_greedy on a device context that has an
 *     automaton, the all-f32 debug path.  The teacher-forced calls stay raw.
 * WM_ERR_INVALID -- and whatever was in force stays -- for: offsets that do not start at 0 or that decrease; edge tokens not
 * strictly ascending within a state; an edge token >= eot; an edge_next or def_next outside [-1, S); an explicit -1 edge in a
 * state whose default is -1; a STUCK state (no allowing edge, no default, not accepting); a count above its limit; eot outside
 * [0, n_vocab).
 * Token ids are the caller's tokenizer's: Whisper's " word" and "word" are different ids, both variants are the caller's to list.
 * Cost: one launch per position that walks the row's history from its start state -- it grows with the
 * history, one dependent lookup per generated text token. */
#define WM_MAX_CST_STATES 4096      /* states of one automaton                                    */
#define WM_MAX_CST_EDGES  65536     /* explicit edges, all states together                        */
WM_API int wm_set_constraint(wm_ctx *ctx, const int32_t *edge_beg /* [n_states + 1] */, const int32_t *edge_tok /* [E] */,
                             const int32_t *edge_next /* [E] */, const int32_t *def_next /* [n_states] */,
                             const uint8_t *accept /* [n_states] */, int n_states, int32_t eot);
WM_API int wm_set_constraint_rows(wm_ctx *ctx, const int32_t *start_of_row /* [n], -1 .. n_states - 1 */, int n);

/* Temperature and seed per ROW: wm_set_sampling_rows names the temperature and the seed of every row of the NEXT transcribe call
 * on the context, like wm_set_bias_rows -- so requests with different temperatures batch into one call, and a long-form window
 * that needs a temperature fallback rides the next round's call beside the other recordings' temperature-0 windows
 * (DESIGN.md section 23).
 *   Life: consumed by that call whatever happens; n must equal its B (WM_ERR_INVALID otherwise); n = 0 drops a pending map.  With
 *     a pending map, opts->temperature and opts->seed of that call are validated as always and not read.  The map is per call:
 *     it applies to the lanes of the call like the other row maps, and wm_clone has nothing to copy.
 *   Row b under (temperature[b], seed[b]): its tokens, length, log-probs and no-speech probability -- and its alternatives,
 *     entropy and the start frames of an aligned entry -- equal, bit for bit, what the same call gives that row when every row
 *     runs at opts->temperature = temperature[b], opts->seed = seed[b].  The Philox counter words are unchanged: id quad,
 *     generated index, sample id or call index, 0.  A row with temperature[b] == 0 is an arg-max row: the temperature-0 call's
 *     bits, its seed is ignored.  The sampling rules (wm_set_sampling_rules) act on the rows whose temperature is > 0 and leave
 *     the others alone.  Results do not depend on the other rows, the grouping or the lanes.
 *   Checked here (on failure the pending map stays dropped): no null pointer when n > 0; every temperature finite and >= 0;
 *     (float)(1.0 / (double)T) finite for every T > 0, the rule of opts->temperature.
 *   Served: wm_transcribe, wm_transcribe_mel, _mel_ragged, wm_transcribe_windows, wm_transcribe_mel_aligned and
 *     wm_transcribe_windows_aligned.  Refused with WM_ERR_STATE (not built; the map is consumed all the same):
 *     wm_transcribe_greedy, the best-of entries, the beam entries and wm_transcribe_mel_speculative (the last two decode at
 *     temperature 0 by definition), wm_multi_transcribe_greedy on a device context with a pending map, the all-f32 debug path.
 * A call without a pending map makes exactly the launches it makes without this entry. */
WM_API int wm_set_sampling_rows(wm_ctx *ctx, const float *temperature /* [n] */, const uint64_t *seed /* [n] */, int n);

/* Per-chunk token budgets for the NEXT wm_transcribe_greedy call on this context (consumed by it; n must equal that
 * call's B): chunk i generates at most budgets[i] tokens (clamped to max_new), lens_out[i] <=
 * budgets[i].  A chunk that has reached its budget -- like one that has emitted `eot` -- LEAVES the decode: its caches are
 * not read again, and once every chunk of a decode group is finished no further position is launched for the group
 * (serving: per-request max_tokens; bench.py: a synthetic early-stop workload).  n = 0 clears. */
WM_API int wm_set_token_budgets(wm_ctx *ctx, const int32_t *budgets, int n);

/* Top-n alternatives and entropy per generated token (OpenAI's `logprobs`, Hugging Face generate's output_scores, CTranslate2's
 * return_scores): what else the model considered at a position, and how peaked its distribution was.  A request applies to the
 * NEXT transcribe call on the context and is consumed by it whatever happens, as wm_set_token_budgets; req == NULL drops a
 * pending request.  The buffers are the caller's and must stay valid until that call returns.  With no request pending every call
 * makes exactly the launches it makes without this entry.
 * At generated index gi of hypothesis row r, gi < lens of that row:
 *   A, the admissible set, and v(id): exactly those of wm_set_sampling_rules -- A is what is left after the suppress lists (the
 *     first-token list too), the timestamp rules (when the sum rule forces a timestamp, A is the admissible timestamps alone),
 *     the no-repeat bans and the sequence-bias bans; v is the stored logit after the repetition penalty and the sequence bias.
 *     An id with v = -INFINITY is not in A.
 *   Order: descending value, equal values lower id first.
 *   tokens[r][gi][j], logprobs[r][gi][j]: the j-th id of A in that order, and v(id) - norm, with norm the normaliser of
 *     token_logprobs_out: log sum over A of exp(v) at temperature 1, truncation (the sampling rules) not part of it -- at any call
 *     temperature and under any sampling rules.  At temperature 0 entry 0 is the generated token, with token_logprobs_out's bits;
 *     at temperature > 0 the drawn token, where it is listed, has token_logprobs_out's bits.
 *   counts[r][gi]: min(n, |A|).  Entries past the count, and every position gi >= lens, are pads: id -1, log-prob 0, count 0,
 *     entropy 0.  The position that stops a row (eot or budget) has its values.
 *   entropy[r][gi]: -sum over A of p log p, p = exp(v - norm), in nats.  The f32 sum runs in a fixed order (each thread of the
 *     row's workgroup adds its ids ascending, then one fixed tree), so a row's bits depend on the row alone -- not on the group's
 *     shape, the lanes, the other rows or the run.  An empty A gives 0.
 * Served: wm_transcribe_greedy (the request turns the extended decode on, as the repetition rules do), wm_transcribe, _mel,
 * _mel_ragged, _mel_best_of (every candidate: rows = B * best_of in the call's hypothesis order [B][best_of]),
 * wm_transcribe_windows, and the *_aligned counterparts of these.  Refused with WM_ERR_STATE, the request consumed:
 * wm_transcribe_mel_beam*, wm_transcribe_windows_beam*, wm_transcribe_mel_speculative, wm_multi_transcribe_greedy (a request
 * pending on a device context) and the all-f32 debug path.  WM_ERR_INVALID: n outside [1, WM_MAX_ALTERNATIVES], null tokens /
 * logprobs, rows or max_new below 1 (answered here); rows / max_new that do not match the call (answered by the call, which
 * still consumes the request).  Teacher-forced calls neither read nor consume a request.  Cost: one launch per position and
 * the stored f32 logits row. */
#define WM_MAX_ALTERNATIVES 16
typedef struct wm_alternatives_out {
    int32_t  n;          /* 1 .. WM_MAX_ALTERNATIVES entries per position                       */
    int64_t  rows;       /* hypotheses of the call the buffers are sized for: B, or B * best_of */
    int32_t  max_new;    /* must equal the call's                                               */
    int32_t *tokens;     /* i32 [rows][max_new][n]  (host)                                      */
    float   *logprobs;   /* f32 [rows][max_new][n]  (host)                                      */
    int32_t *counts;     /* i32 [rows][max_new]     (host, nullable)                            */
    float   *entropy;    /* f32 [rows][max_new]     (host, nullable)                            */
} wm_alternatives_out;
WM_API int wm_request_alternatives(wm_ctx *ctx, const wm_alternatives_out *req /* NULL: drop a pending request */);

/* Given tokens: a row decodes a text the caller already has and returns its log-probs (CTranslate2's score_batch, Hugging Face's
 * compute_transition_scores and forced decoder ids, openai-whisper's `prefix`; n-best rescoring, "which of these K commands was
 * spoken", the log-prob and entropy of a reference transcript, resuming a hypothesis inside a window).  The table is armed for the
 * NEXT transcribe call on the context and is consumed by it whatever happens, as wm_set_token_budgets; n = 0 drops a pending table.
 * Row r is the call's hypothesis row: B rows, or B * best_of in the call's hypothesis order [B][best_of], as
 * wm_request_alternatives counts them.
 * At generated index gi < lens[r] the close takes tokens[r][gi] in place of its own choice; everything else is the call's:
 *   - rule state follows the given token: the timestamp history, the repetition bitmaps, bias and constraint state, budgets, the
 *     eot stop, the embedding of the next position;
 *   - at gi >= lens[r] the row decodes freely; lens[r] = 0 is an ordinary row, so scored and decoded rows batch in one call;
 *   - a caller who wants scoring alone sets budgets equal to lens (wm_set_token_budgets; per row of the CALL: the candidates of a
 *     best-of window share theirs); a caller who wants openai-whisper's `prefix` with log-probs leaves them open.
 * token_logprobs_out[r][gi] at a given position is v(tok) - norm:
 *   - v is the stored logit after the repetition penalty and the sequence bias;
 *   - norm is the normaliser of the decision the row would have made WITHOUT the table (under the timestamp rules: over the
 *     admissible timestamps alone where the sum rule forces one): the normaliser of every other log-prob of the library, at
 *     temperature 1, whatever the call's temperature, seed and sampling rules;
 *   - if the given token is what the plain call chose, the bits are the plain call's;
 *   - if the given token is not admissible -- outside the row's ranges, a text id where the sum rule forces a timestamp,
 *     suppressed, banned, v equal to -INFINITY or NaN -- the log-prob is -INFINITY and the row goes on with the given token;
 *   - a row with NOTHING admissible at a position (every allowed id suppressed) has no normaliser: there the call takes its existing
 *     path (its fallback token, -INFINITY), and the table holds again from the next position.
 * Alternatives of a given position (wm_request_alternatives) list what the model preferred; a given row of a sampling call never
 * draws.  A group of ordinary rows inside a call with a table makes exactly the launches it makes without one.
 * Served: wm_transcribe, _mel, _mel_ragged, _mel_best_of, wm_transcribe_windows and the *_aligned counterparts of the plain
 * entries.  Refused with WM_ERR_STATE, the table consumed: the beam entries, the aligned best-of entries,
 * wm_transcribe_mel_speculative, wm_multi_transcribe_greedy (a table pending on a device context), wm_transcribe_greedy (it has
 * no log-prob output) and the all-f32 debug path.  WM_ERR_INVALID here: a token outside the vocabulary, a lens entry outside
 * [0, stride], null pointers or stride < 1 with n > 0 (the pending table is dropped); from the call, the table still consumed: n
 * other than the call's hypothesis rows, a lens entry above max_new.  Cost: one launch per position of a group that holds a
 * given row, and that group's stored f32 logits row. */
WM_API int wm_set_given_tokens(wm_ctx *ctx, const int32_t *tokens /* i32 [n][stride] */, int stride,
                               const int32_t *lens /* i32 [n], 0 .. stride */, int n);

/* GIVEN PANELS: generated positions per decoder step over the GIVEN tokens of a transcribe call (wm_set_given_tokens).  A given
 * text is known up front, so up to `width` of its positions can share one decoder step -- the weights streamed once, a window's
 * cross-attention K/V read once -- each closed exactly as the one-position step closes it.
 *   width : 1 .. WM_MAX_TEACHER_PANEL; 1 (the default) enqueues exactly the launches a call always enqueued.
 * A context setting like wm_set_prompt_panel: not pending state, calls do not consume it; same inheritance as wm_set_suppress
 * (wm_clone and the lanes of a call take it over).  WM_ERR_INVALID: width outside the range (the old width stays in force).
 * A LAUNCH POLICY, NOT A NUMERICS SWITCH: tokens, lengths, token log-probs and no_speech_prob are bit-identical for every width,
 * and the setting never makes a call fail.  THE RULE, per decode group of G rows with prompt length P:
 *   SERVED GROUPS.  All of: the group holds a given row; it is a plain group (no best-of candidates, no beams) with uniform
 *     prompts, the extended decode on and temperature 0 for every row (no row of a sampling row map samples; the sampling rules
 *     are not read at temperature 0, as in every call); no
 *     alternatives, repetition rules, sequence bias (single table or row tables), constraint or alignment capture; not the
 *     all-f32 debug path and no debug hooks staged by the caller; and w = min(width, 128 / G) >= 2.  Timestamp rules, suppress
 *     masks, budgets and the eot stop may be on or off.  Every other group steps one position at a time, exactly as without the
 *     setting.
 *   FIRST TOKEN.  Generated index 0 is always taken by the ordinary step at position P - 1 (the first-token suppress list,
 *     max_initial_timestamp_index and the <|startoftranscript|> read of no_speech_prob live there; no panel meets them).
 *   PHASE.  Lp = the largest L <= max_new with P + L - 1 < n_text_ctx such that for every row r and every gi in [1, L):
 *     gi < lens[r] or gi >= min(budget[r], max_new) -- at every phase position each row is given, or already finished for a reason
 *     the host knows.  Lp <= 1: no phase.  Otherwise generated indices [1, Lp) run as ceil((Lp - 1) / w) rounds, round at index
 *     g0 of width min(w, Lp - g0), behind the ordinary step at P - 1; the group's ordinary steps (or captured graphs) continue from
 *     position P + Lp - 1.  One round covers the whole group: no slices.
 *   A ROUND at position pos (g0 = pos + 1 - P): the inputs tok[c][g0 + s - 1], s = 1 .. w - 1, are staged at positions pos + s and
 *     the timestamp rules are replayed along them, so that row (c, s) sees the ranges after the tokens up to its own input; one
 *     panel step over G x w rows with the stored f32 row (rows of finished windows are computed and ignored); per row the given
 *     token's admissibility, value and log-prob by the arithmetic of the one-position step (the cases of wm_set_given_tokens apply
 *     unchanged, a forced timestamp included; a row with NOTHING admissible takes the fallback token and -INFINITY as there, and --
 *     the one exception to "the same bits" -- the later rows of that window in the SAME round were computed behind the table's
 *     token, not the fallback); per window the commit -- its tokens and
 *     log-probs up to its first eot (with the eot stop) or the end of its budget, pad and 0 behind, its rule state advanced along the
 *     kept tokens, its done flag; the position advances by the round's width.  Behind the last round the step path's state
 *     (rule state, done flags, the live list, the embedding of position P + Lp - 1) is what the one-position steps leave.
 *   THE ONE EXCEPTION to "the same bits" is the nothing-admissible row named above: the round is not cut at that row.  It needs
 *     every allowed id of a position suppressed (or NaN logits); under the timestamp rules eot stays allowed, so a caller who
 *     does not suppress eot cannot meet it.
 * The rounds run eagerly, not from captured graphs; no graph is dropped by this call. */
WM_API int wm_set_given_panel(wm_ctx *ctx, int width);

/* ------------------------------------------------- all GPUs of the node, one host process --- */
/* the Swift host dlopens ONE library in ONE process; wm_multi drives n GPUs from it.  Weights are
 * replicated (one wm_ctx per device: fetch each with wm_multi_device_ctx and fill it with wm_load_weights /
 * wm_set_tensor / wm_init_synthetic + wm_finalize, exactly as a single context), a call's chunks are cut into contiguous
 * blocks -- rank r owns [r ceil(B/n), min(B, (r+1) ceil(B/n))) -- each block runs its whole path (front end -> encoder
 * -> greedy decode) on its own GPU from its own host thread, and the only exchange is ONE fixed-stride all-gather of
 * int32 [ceil(B/n)][1 + max_new] (length, tokens) per rank over RCCL / xGMI (ncclCommInitAll).  n = 1 is valid.
 *   devices    : n distinct HIP device ordinals;
 *   pcm        : HOST [B][480000] samples; tokens_out i32 [B][max_new], lens_out i32 [B] (host), as wm_transcribe_greedy. */
typedef struct wm_multi wm_multi;
WM_API int wm_multi_create(const wm_dims *dims, const int *devices, int n, wm_multi **out);
WM_API void wm_multi_destroy(wm_multi *m);
WM_API int wm_multi_size(const wm_multi *m);
WM_API int wm_multi_device_ctx(wm_multi *m, int rank, wm_ctx **out);
WM_API int wm_multi_transcribe_greedy(wm_multi *m, const void *pcm, wm_dtype pcm_dtype, int B, const int32_t *prompt,
                               int n_prompt, int max_new, int32_t eot, int32_t *tokens_out, int32_t *lens_out);
/* Host-only pieces of the above (usable without a GPU; also what the CPU tests pin): the block partition, and the
 * fixed-stride payload [per][1 + max_new] = (length, tokens) each rank contributes to the all-gather. */
WM_API int wm_multi_partition(int n_chunks, int world_size, int rank, int *lo, int *hi);
WM_API int wm_multi_pack_tokens(const int32_t *tokens, const int32_t *lens, int n_local, int per, int max_new,
                         int32_t *payload);
WM_API int wm_multi_unpack_tokens(const int32_t *gathered, int world_size, int per, int max_new, int n_chunks,
                           int32_t *tokens_out, int32_t *lens_out);

/* -------------------------------------------------------------- ids -> text (host only) --- */
/* GPT-2 byte-level BPE de-tokenizer for the ids wm_transcribe_greedy returns (the reference prints
 * a language code and has no tokenizer, Whisper.swift:37-39).  vocab_json_path: the tokenizer's vocab.json
 * ({"piece": id, ...}, pieces over GPT-2's byte alphabet) -- supplied by the host, no vocabulary ships with the library.
 * wm_detokenize: UTF-8 text of ids[0..n): ids without a piece (special tokens, timestamps) are skipped
 * (skip_special != 0) or written as <|id|>.  Writes at most cap - 1 bytes + NUL; *needed (nullable) = bytes required
 * including the NUL, so cap = 0 sizes the buffer.  No GPU involved. */
typedef struct wm_vocab wm_vocab;
WM_API int wm_vocab_load(const char *vocab_json_path, wm_vocab **out);
WM_API void wm_vocab_free(wm_vocab *v);
WM_API int wm_vocab_size(const wm_vocab *v);
WM_API int wm_detokenize(const wm_vocab *v, const int32_t *ids, int n, int skip_special, char *buf, size_t cap,
                  size_t *needed);

/* ------------------------------------------------ WAV reader + 30 s chunker (host only) --- */
/* The step BEFORE the path: the reference records 16 kHz mono 16-bit LinearPCM to query.wav
 * (AudioRecorder.swift:56-61), reads it back through AVFoundation (:74-86) and zero-pads / truncates to one 30 s window
 * (ContentView.swift:57-60).  For a dlopen-only host: the same file format in, and the reference's pad rule applied per
 * window, so a recording of any length becomes [n_chunks][480000] int16 (x = s / 32768 inside the front end) for
 * wm_logmel / wm_transcribe_greedy / wm_multi_transcribe_greedy.  Anything but 16 kHz mono 16-bit PCM is WM_ERR_IO. */
typedef struct wm_wav wm_wav;
WM_API int wm_wav_open(const char *path, wm_wav **out);
WM_API void wm_wav_close(wm_wav *w);
WM_API long wm_wav_num_samples(const wm_wav *w);
WM_API int wm_wav_num_chunks(const wm_wav *w);   /* ceil(samples / 480000), at least 1 */
/* windows [first_chunk, first_chunk + n_chunks) -> out int16 [n_chunks][480000], the last window zero-padded */
WM_API int wm_wav_read_chunks(const wm_wav *w, int first_chunk, int n_chunks, int16_t *out);

/* ------------------------------------------------ audio at any sample rate -> 16 kHz mono --- */
/* Everything above takes 16 kHz mono samples.  wm_resample_16k makes them, on the device, from recordings at their own
 * rate and channel count: a polyphase Kaiser-windowed-sinc resampler, defined ONCE, on the host, in
 * f64.  For input rate sr: g = gcd(sr, 16000), L = 16000 / g, M = sr / g, mx = max(L, M), K = WM_RESAMPLE_ZEROS * mx, and
 * for j = -K .. K
 *     c = WM_RESAMPLE_ROLLOFF / (2 mx)
 *     h[j] = L * 2c * sinc(2c j) * I0(WM_RESAMPLE_BETA * sqrt(1 - (j / K)^2)) / I0(WM_RESAMPLE_BETA),  sinc(x) = sin(pi x) / (pi x)
 * rounded once to f32.  Output n of a recording of N frames, n < N_out = ceil(N L / M):
 *     y[n] = sum_k m[k] h[n M - k L],   m = the mono downmix, zero outside [0, N)
 * -- scipy.signal.resample_poly(m, L, M, window=h / L).  Downmix of C channels, per frame: the f32 sum in channel order
 * times (float)(1.0 / C); C == 1: the sample itself.  WM_I16 samples are s / 32768, WM_F32 samples are used as they are.
 * Supported rates: 4000 <= sr <= 192000 with L <= 640 (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200,
 * 96000, 176400, 192000, ...); sr == 16000 is a bypass (downmix only, no filter). */
#define WM_RESAMPLE_ZEROS 32        /* zero-crossing spans of the sinc on each side */
#define WM_RESAMPLE_ROLLOFF 0.9     /* cutoff as a fraction of the lower Nyquist frequency */
#define WM_RESAMPLE_BETA 9.62       /* Kaiser window beta */

/* ceil(n_frames L / M): the 16 kHz samples wm_resample_16k makes of n_frames frames at sample_rate.  Host only.
 * -1: unsupported rate, negative length (or one above 2^40). */
WM_API int64_t wm_resample_out_len(int64_t n_frames, int sample_rate);
/* The f32 filter the kernel uses, h[i] = h[j = i - K], i = 0 .. 2K; *L, *M, *K (each nullable) as above.  Host only, no
 * context.  cap: floats h can hold; cap = 0 only sizes (h is not read).  Invalid: an unsupported rate, 0 < cap < 2K + 1. */
WM_API int wm_resample_filter(int sample_rate, float *h, size_t cap, int *L, int *M, int *K);
/* R recordings, each at its own rate and channel count, to 16 kHz mono f32 in ONE launch.
 *   pcm          : interleaved samples of all recordings back to back, WM_I16 or WM_F32, mem-space selectable (with
 *                  WM_MEM_HOST only pcm[elem_offsets[0] .. elem_offsets[R]) is copied);
 *   elem_offsets : i64 [R + 1] (host), non-decreasing: recording r = pcm[elem_offsets[r] .. elem_offsets[r + 1]), a
 *                  multiple of n_channels[r] elements;  R : 0 .. 65535; empty recordings are legal;
 *   n_channels   : i32 [R] (host), 1 .. 8;  sample_rates : i32 [R] (host);
 *   out          : f32, recording r's wm_resample_out_len(frames_r, sample_rates[r]) samples (at most 2^30) after those of
 *                  recordings 0 .. r - 1 -- the pcm / sample_offsets layout of wm_logmel_long(..., WM_F32, ...); same `mem`.
 * A front-end-only context is enough.  The context builds and uploads a rate's filter on first use and keeps it.
 * A recording's output depends on its own samples, rate and channel count only: bit-identical alone, among other
 * recordings and at any offset (every output is one f32 fma chain over its taps in ascending input order).
 * The call returns when the launch has finished, with WM_MEM_DEVICE too: the per-call tables are pageable host memory, so the
 * stream is synchronised before they go out of scope (as wm_logmel_long does).  At most 2^24 - 1 tiles of 1024 outputs per call
 * (298 hours of output); more is WM_ERR_INVALID.
 * Profile family: "resample".  Invalid: a dtype other than WM_I16 / WM_F32, a length that is no multiple of the channel
 * count, channels outside 1 .. 8, an unsupported rate, decreasing or negative offsets, null pointers with R > 0. */
WM_API int wm_resample_16k(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, const int64_t *elem_offsets,
                           const int32_t *n_channels, const int32_t *sample_rates, int R, float *out, wm_mem mem);

/* ------------------------------------------------ multichannel audio: channel matrix, per-channel activity --- */
/* wm_resample_16k with a CHANNEL MATRIX in place of the mean: recording r yields n_rows[r] output
 * signals, signal (r, o) being the resampling of the recording mixed down under row o of its matrix.  The mixed sample of
 * a frame x[0 .. C - 1] under a row w[0 .. C - 1], stated once:
 *     m = w[0] * x[0]                          (one f32 rounding)
 *     m = fmaf(w[c], x[c], m),  c = 1 .. C-1   (channel order)
 * x is s / 32768 for WM_I16 and the sample itself for WM_F32.  Behind the mix the filter is wm_resample_16k's, unchanged: the
 * same phase tables per rate, ONE f32 fma chain per output over its taps in ascending input order, and at 16000 Hz the
 * bypass, which writes m itself.
 *   pcm, pcm_dtype, elem_offsets, n_channels, sample_rates, R, mem, the supported rates: exactly as wm_resample_16k;
 *   n_rows : i32 [R] (host), 1 .. 8: the output signals of recording r; their sum is at most 65535;
 *   mix    : f32 (host): row o of recording r is n_channels[r] finite weights; the rows lie back to back in (r, o) order;
 *   out    : f32, signal (r, o)'s wm_resample_out_len(frames_r, sample_rates[r]) samples, the signals back to back in (r, o)
 *            order -- the pcm / sample_offsets layout of wm_logmel_long(..., WM_F32, ...) with sum(n_rows) recordings; same `mem`.
 * A signal's bits depend on its own recording, rate and row only: not on the other rows or their order, the other
 * recordings, the offset, the tile or the grid.  A one-hot row c equals wm_resample_16k on channel c as a mono recording
 * (bit for bit behind a filter; at 16000 Hz as values: a -0.0 sample of a recording of two or more channels may come out
 * +0.0), and for WM_I16 stereo the row (0.5, 0.5) equals wm_resample_16k's mean bit for bit.  One launch, one workgroup per
 * (signal, tile of 1024 outputs), each reading the interleaved span of its tile; the tile limit, the return after the launch
 * and the front-end-only context are wm_resample_16k's.  Profile family: "resample_mix".  Invalid: everything wm_resample_16k
 * rejects, n_rows outside 1 .. 8, more than 65535 signals, a weight that is not finite, a null n_rows or mix with R > 0. */
WM_API int wm_resample_16k_mix(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, const int64_t *elem_offsets,
                               const int32_t *n_channels, const int32_t *sample_rates, int R, const int32_t *n_rows,
                               const float *mix, float *out, wm_mem mem);
/* Per-channel activity: the level of S 16 kHz f32 signals (wm_resample_16k_mix's output, where it lies), one value per mel
 * frame of 10 ms.  Signal s = pcm16k[sample_offsets[s] .. sample_offsets[s + 1]) of N_s samples y gets ceil(N_s /
 * WM_ACTIVITY_HOP) values, the signals' values packed back to back in signal order:
 *     act[f] = sum |y[160 f + i]|   over i < 160 with 160 f + i < N_s        (f32)
 * in THIS order, a function of the frame alone:
 *     p[j] = ((|y[160 f + j]| + |y[160 f + 16 + j]|) + ...) + |y[160 f + 144 + j]|    j = 0 .. 15; ten terms, ascending; a term
 *                                                                                    past N_s is +0
 *     q[j] = p[j] + p[j + 8],  r[j] = q[j] + q[j + 4],  t[j] = r[j] + r[j + 2],  act[f] = t[0] + t[1]
 * so a signal's values are bit-identical alone, among other signals and at any offset; a NaN sample makes its frame NaN and
 * no other.  The terms are non-negative: |act - exact| <= 160 * 2^-24 * exact.
 *   pcm16k : f32, mem-space selectable (with WM_MEM_HOST only pcm16k[sample_offsets[0] .. sample_offsets[S]) is copied);
 *   sample_offsets : i64 [S + 1] (host), >= 0 and non-decreasing; S : 0 .. 65535; empty signals are legal (no value);
 *   act_out : f32, same `mem`.
 * A front-end-only context is enough.  One launch, one workgroup per (signal, tile of 64 frames); returns when the launch has
 * finished (per-call tables, as wm_resample_16k); at most 2^24 - 1 tiles per call.  Profile family: "channel_activity".
 * Invalid: negative or decreasing offsets, null pointers with S > 0. */
#define WM_ACTIVITY_HOP 160   /* one value per mel frame: 10 ms */
WM_API int wm_channel_activity(wm_ctx *ctx, const float *pcm16k, const int64_t *sample_offsets, int S, float *act_out, wm_mem mem);

/* ------------------------------------------------ general RIFF/WAVE reader (host only) --- */
/* Beside wm_wav_* (which keeps its strict 16 kHz mono 16-bit rule): any rate, 1 .. 8 channels; integer PCM (format 1) at
 * 8 bits (unsigned, (s - 128) / 128), 16 (s / 2^15), 24 (s / 2^23) and 32 (s / 2^31, computed in double, rounded once);
 * IEEE float (format 3) at 32 and 64 bits (rounded to f32); WAVE_FORMAT_EXTENSIBLE with those sub-formats.  The hardening
 * of wm_wav_open: a truncated or streamed data chunk gives the whole frames that are there, odd chunks are padded, files
 * above 4 GiB and every malformed or inconsistent header (block_align != channels * bits / 8, ...) are WM_ERR_IO. */
typedef struct wm_audio wm_audio;
WM_API int wm_audio_open(const char *path, wm_audio **out);
WM_API void wm_audio_close(wm_audio *w);
WM_API int wm_audio_sample_rate(const wm_audio *w);      /* Hz; a null handle: 0 */
WM_API int wm_audio_channels(const wm_audio *w);         /* 1 .. 8; a null handle: 0 */
WM_API int64_t wm_audio_num_frames(const wm_audio *w);   /* frames (one sample of every channel); a null handle: 0 */
WM_API int wm_audio_bits(const wm_audio *w);             /* bits per sample: 8 / 16 / 24 / 32 / 64; a null handle: 0 */
WM_API int wm_audio_is_float(const wm_audio *w);         /* 1: IEEE float samples, 0: integer PCM */
/* frames [first_frame, first_frame + n_frames) -> out f32 [n_frames][channels] (interleaved).  Invalid: a range outside
 * the recording. */
WM_API int wm_audio_read(const wm_audio *w, int64_t first_frame, int64_t n_frames, float *out);
/* The same frames of a 16-bit integer file as raw int16 (for wm_resample_16k(..., WM_I16, ...): 2 bytes per sample across
 * PCIe).  Invalid: any other format. */
WM_API int wm_audio_read_i16(const wm_audio *w, int64_t first_frame, int64_t n_frames, int16_t *out);

/* ------------------------------------------------ speech-activity detection on the whole-recording log-mel --- */
/* Cutting a long recording at its silences into clips that decode together (binding.transcribe_long(vad=..., parallel_clips=...),
 * DESIGN.md section 13).  wm_vad_energy makes a per-frame energy track on the device from wm_logmel_long's output, where it
 * already lies; wm_vad_segments turns a track into speech spans on the host.  Per recording r and frame t < n_frames[r],
 * with v = the log-mel value ((max(log10 mel, gmax_r - 8) + 4) / 4) and the band rows m in [band_lo, band_hi):
 *     vmax = max_m v[m][t]
 *     s    = sum_m exp2f((v[m][t] - vmax) * (4 log2 10))                      f32, m ascending
 *     e[t] = 4 vmax + log10f(s)                                               log10 of the band's mel power, + 4
 *     y[t] = (sum_{u = max(0, t - h)}^{min(n - 1, t + h)} e[u]) * (1.0f / count),   h = smooth / 2;  f32, u ascending
 * smooth is odd, 1 .. 31; smooth = 1 gives y = e.
 *   mel        : wm_logmel_long's output, mem-space selectable (with WM_MEM_HOST only each recording's band rows are copied);
 *   mel_base   : i64 [R] (host): element of recording r's [n_mels][mel_len[r]] block;  mel_len : i32 [R] (host), >= 1;
 *   n_frames   : i32 [R] (host), 0 .. mel_len[r]: the frames to do -- pass the content frames T_r - 3000, so that the 30 s
 *                of padding never count; 0 writes nothing;  R : 0 .. 65535;
 *   raw_out    : f32, nullable: e;  energy_out : f32: y.  Both packed -- recording r's n_frames[r] values after those of
 *                recordings 0 .. r - 1 -- and in the same `mem` as mel.
 * A front-end-only context is enough.  One launch, one workgroup per (recording, tile of 224 frames); the summation orders are
 * fixed, so a recording's output is bit-identical alone, among other recordings and at any mel_base.  Non-finite mel values
 * propagate.  Returns when the launch has finished (per-call tables, as wm_resample_16k).  At most 2^24 - 1 tiles per call.
 * Profile family: "vad".  Invalid: n_mels not 80 / 128, a band outside 0 <= lo < hi <= n_mels, an even or out-of-range smooth,
 * n_frames outside [0, mel_len], mel_len < 1, mel_base < 0, null pointers with R > 0. */
WM_API int wm_vad_energy(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len, const int32_t *n_frames,
                         int R, int n_mels, int band_lo, int band_hi, int smooth, float *raw_out, float *energy_out, wm_mem mem);
/* The segment rule's parameters.  Defaults (wm_vad_default_params): 0.10, 0.95, 0.6, 0.5, 0.35, 25, 50, 40 -- with smooth 5
 * on the caller's side.  THESE DEFAULTS ARE NOT VALIDATED ON REAL SPEECH: the machines this project is built on hold none;
 * they are set on synthetic bursts over noise (tests/test_vad_cpu.py).  Any other detector's spans can be passed to
 * binding.transcribe_long as clip_timestamps instead. */
typedef struct wm_vad_params {
    float q_floor, q_peak;      /* quantiles of the track that stand for the noise floor and the speech level */
    float min_range;            /* peak - floor below this: no contrast, the whole recording is one segment */
    float on_frac, off_frac;    /* thresholds: floor + frac * (peak - floor); speech begins at >= on, ends below off */
    int32_t min_speech;         /* frames: a shorter span is dropped */
    int32_t min_silence;        /* frames below off that end a span */
    int32_t speech_pad;         /* frames added to every span over both sides: speech_pad / 2 in front, speech_pad / 2 behind */
} wm_vad_params;
WM_API void wm_vad_default_params(wm_vad_params *p);   /* a null p: no-op */
/* Speech spans [start, end) in frames of a track y f32 [n] (wm_vad_energy's energy_out of one recording).  Host only, no
 * context.  All arithmetic in double on the f32 inputs.  s = y sorted; floor = s[(size_t)(q_floor (n - 1))], peak likewise.
 * peak - floor < min_range: the one segment [0, n) (never drop audio when there is no contrast; thresholds NaN).  Otherwise
 * thr_on = floor + on_frac (peak - floor), thr_off likewise, and the scan of Silero VAD's get_speech_timestamps on y: a span
 * opens at the first y >= thr_on; y < thr_off marks a pending end, which any y >= thr_on cancels; the span closes at the
 * pending end once min_silence frames lie behind it and is kept when at least min_speech long; a span open at the end is
 * kept when n - start >= min_speech.  Every span is padded by speech_pad frames over both sides (speech_pad / 2 each, integer
 * division), cut to [0, n), and merged into its
 * predecessor when it begins at or before the predecessor's end.
 *   segments   : i32 [cap][2], nullable with cap = 0;  *n_segments : the count NEEDED (at most cap pairs are written; cap = 0
 *                sizes the buffer);  n = 0: no segment;  stats : f32 [4], nullable: floor, peak, thr_on, thr_off.
 * Invalid: a NaN in y, quantiles outside 0 <= q_floor < q_peak <= 1, fractions outside 0 <= off_frac <= on_frac <= 1 or
 * on_frac = 0, a negative or non-finite min_range, min_silence < 1, a negative min_speech or speech_pad, n above 2^31 - 1,
 * null pointers. */
WM_API int wm_vad_segments(const float *y, int64_t n, const wm_vad_params *p, int32_t *segments, int cap, int *n_segments,
                           float stats[4]);

/* ------------------------------------------------------------ device memory helpers --- */
/* For callers that keep inputs resident in HBM (bench.py; a Swift host would use them to
 * avoid the 5.7 MB/chunk PCIe round trip of the reference ABI). */
WM_API int wm_dev_malloc(wm_ctx *ctx, size_t bytes, void **dptr);
WM_API int wm_dev_free(wm_ctx *ctx, void *dptr);
WM_API int wm_dev_upload(wm_ctx *ctx, void *dptr, const void *host, size_t bytes);
WM_API int wm_dev_download(wm_ctx *ctx, void *host, const void *dptr, size_t bytes);
WM_API int wm_sync(wm_ctx *ctx);

/* -------------------------------------------------------------------- measurement --- */
/* Per-kernel-family HIP-event timing on the context's stream.  When enabled, every launch
 * of a profiled kernel family is bracketed by hipEventRecord on the launch stream; the
 * totals are read back with wm_profile_get (which synchronises). */
WM_API int wm_profile_enable(wm_ctx *ctx, int on);
WM_API int wm_profile_reset(wm_ctx *ctx);
/* Bias (microseconds) of an event-bracketed launch on this stream, calibrated with a kernel that spins
 * for a known time of the device clock: subtract it from a family's mean launch duration. */
WM_API int wm_profile_overhead_us(wm_ctx *ctx, float *us);
/* Writes a JSON object {"family": {"ms": total_ms, "n": launches}, ...} into buf. */
WM_API int wm_profile_json(wm_ctx *ctx, char *buf, size_t buf_bytes);
/* Wall-clock stage split of the last wm_transcribe_greedy call, in ms (HIP events):
 * [0] front end, [1] encoder + cross-KV projection, [2] decode loop.  After wm_align / wm_align_mel: [0] front end (the
 * window copies of a WM_MEM_HOST wm_align_mel call) + encoder + cross-KV projection, [1] teacher-forced pass, [2] alignment
 * kernels + DTW. */
WM_API int wm_last_stage_ms(wm_ctx *ctx, float out3[3]);

#ifdef __cplusplus
}
#endif
#endif /* WHISPER_MI355X_H */
