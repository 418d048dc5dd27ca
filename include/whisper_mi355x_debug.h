/*
 * whisper_mi355x_debug.h -- test hooks exported by libwhisper_mi355x_dbg.so (the product library,
 * libwhisper_mi355x.so, does not contain them).
 *
 * NOT part of the drop-in surface: these let tests/ drive individual HIP kernels (and a
 * few host-side helpers) through the same C ABI conventions, so each kernel can be
 * compared with the oracle in isolation.  All pointers are HOST pointers; the hooks
 * stage through HBM themselves.
 */
#ifndef WHISPER_MI355X_DEBUG_H
#define WHISPER_MI355X_DEBUG_H

#include "whisper_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only: slaney mel filterbank as librosa.filters.mel(sr=16000, n_fft=400, n_mels)
 * builds it (the recipe behind export_m80.py:4's mel_filters.npz); out: [n_mels][201]. */
WM_API int wmdbg_mel_filterbank(int n_mels, float *out);
/* Host-only: the embedded copy of the reference's m80.npy (80*201 f32). */
WM_API int wmdbg_mel80(float *out);

/* ---- single-kernel hooks (GPU).  Matrices are given as f32 and rounded to bf16 inside,
 * exactly as the weights / activations are held in HBM. ---------------------------------- */
/* C[M][N] = A[M][K] . W[N][K]^T (+bias); epi: 6 = f32 out, 0 = bf16 out, 1 = gelu -> bf16,
 * 2 = C += (f32 residual).  K % 64 == 0.  C is f32 on the host in every case. */
WM_API int wmdbg_gemm(wm_ctx *ctx, const float *A, const float *W, const float *bias, float *C, int M, int N,
               int K, int epi);
/* The same kernels with ANY of the seven epilogues and ANY row map, at small shapes: what wm_model_encode_win and
 * wm_model_cross_kv ask of them (both Conv1d layers as implicit GEMMs, the V^T transpose, the cross-K/V scatter).
 *   A row m = the K elements at a_off + (m / a_rpb) * a_bstride + (m % a_rpb) * a_rstride of A f32 [a_elems] (rounded to bf16,
 *     uploaded with zeroed slack behind it); W f32 [N][K]; bias f32 [N] or NULL.
 *   C row m starts at c_off + (m / c_rpb) * c_bstride + (m % c_rpb) * c_rstride of C f32 [c_elems]: the device buffer (bf16 for
 *     epi 0, 1, 4, 5; f32 for 2, 3, 6) widened.  epi 5 (EPI_XKV) ignores the C map: C = [2][batch][n_head][seq][64].
 *   epi 3 (EPI_CONV2_F32): pos f32 [c_rpb][N].  epi 4 (EPI_QKV_ENC): C rows hold the 2 * d_model query | key columns, vt f32
 *     [vt_elems] = the bf16 V^T buffer [batch][n_head][64][seq_pad] widened.
 * Before the launch every bf16 output element holds WMDBG_SENTINEL_BF16 and every f32 one WMDBG_SENTINEL_F32 (NaN bit
 * patterns), except for epi 2 (EPI_RESID_F32), whose C is in / out: what the kernel did not write, or wrote where it should
 * not, shows.  NOTHING is launched unless every address is inside its buffer -- WM_ERR_INVALID otherwise, with the reason in
 * wm_last_error(): every A row inside a_elems + 128 elements (the 256 bytes of slack the product's allocations carry, which
 * conv1 at n_mels = 80 over-reads by 16 elements), the A map a multiple of 8 elements, every C row inside c_elems, C rows
 * disjoint (c_rstride >= N -- 2 * d_model for epi 4 -- and c_bstride >= c_rpb * c_rstride once M > c_rpb), the C map 16-byte
 * aligned when N % 64 == 0 (the staged epilogues), K % 64 == 0; epi 5: M == batch * seq, N == 2 * d_model, d_model == 64 *
 * n_head, c_elems == 2 * batch * n_head * seq * 64; epi 4: M == batch * seq, N == 3 * d_model, d_model == 64 * n_head,
 * seq_pad % 16 == 0, seq_pad >= seq, vt_elems == batch * n_head * 64 * seq_pad. */
typedef struct wmdbg_gemm_map {
    int32_t M, N, K, epi;
    int64_t a_off, a_rpb, a_bstride, a_rstride, a_elems;
    int64_t c_off, c_rpb, c_bstride, c_rstride, c_elems;
    int32_t d_model, n_head, seq, seq_pad, batch, reserved;
    int64_t vt_elems;
} wmdbg_gemm_map;
WM_API int wmdbg_gemm_mapped(wm_ctx *ctx, const wmdbg_gemm_map *map, const float *A, const float *W, const float *bias,
                             const float *pos, float *C, float *vt);
/* For callers that restate the struct (ctypes): out4 = sizeof(wmdbg_gemm_map) and the offsets of a_off, d_model and vt_elems
 * (host only). */
WM_API int wmdbg_gemm_map_layout(int32_t *out4);

/* ---- the product's own encoder-side launches, on a context with finalised weights (so the conv packing of wm_set_tensor is
 * part of what runs).  1 <= B <= 16; C = n_mels, d = n_audio_state, H = n_audio_head. ------------------------------------------ */
/* The stem of wm_model_encode_win (mel re-layout, conv1, conv2) by the function the encoder calls.  mel f32 [B][C][3000], or
 * with wins i64 [B][4] = (base, T, seek, n) per row: row b = frames seek .. seek + n - 1 (n <= 3000, seek + n <= T, zeros
 * after) of the [C][T] block at mel + base; mel then holds max(base + C * T) elements.  Out (bf16 widened / f32): mel_t
 * [B][3002][C], h1p [B][3001][d], x [B][1500][d].  Before the launches the interiors hold the sentinels (mel_t rows 1 .. 3000,
 * h1p rows 1 .. 3000, x); the guard rows -- mel_t rows 0 and 3001, h1p row 0 -- are left as the allocation zeroed them. */
WM_API int wmdbg_encode_stem(wm_ctx *ctx, const float *mel, const int64_t *wins, int B, float *mel_t_out, float *h1p_out,
                             float *x_out);
/* Encoder layer `layer`'s LayerNorm + QKV launch on x f32 [B * 1500][d] uploaded into the model's residual buffer.  Out (bf16
 * widened): xn [B * 1500][d], qk [B * 1500][2 d] (pre-scaled queries | keys), vt [B][H][64][1536].  xn, qk and vt hold
 * WMDBG_SENTINEL_BF16 before the launches; afterwards vt is zeroed, so that its pad columns 1500 .. 1535 are zero again as a
 * later encode expects. */
WM_API int wmdbg_encode_layer_qkv(wm_ctx *ctx, int layer, const float *x, int B, float *xn_out, float *qk_out, float *vt_out);
/* The whole of encoder layer `layer` on x f32 [B * 1500][d]: the LayerNorm + QKV launch as above, then the layer's other five
 * launches by the function the encoder calls (attention, out-projection + residual, LayerNorm, fc1 + GELU, fc2 + residual).
 * Out, each as its launch left it (bf16 widened / f32): att [B * 1500][d], x_mid [B * 1500][d] (the residual stream after the
 * out-projection, copied aside before the LayerNorm), xn2 [B * 1500][d], hid [B * 1500][4 d], x_out [B * 1500][d].  xn, qk
 * with the 64 rows behind it, att and hid hold WMDBG_SENTINEL_BF16 and the copy of x_mid WMDBG_SENTINEL_F32 before the
 * launches; vt is zeroed before them (its pad columns are the attention kernel's contract), the 64 rows behind qk after them. */
WM_API int wmdbg_encode_layer_tail(wm_ctx *ctx, int layer, const float *x, int B, float *att_out, float *x_mid_out,
                                   float *xn2_out, float *hid_out, float *x_out);
/* ln_post by the function the encoder calls, on x f32 [B * 1500][d]: xn [B * 1500][d] (bf16 widened), xa [B * 1500][d] f32; both
 * hold their sentinels before the launch. */
WM_API int wmdbg_encode_post(wm_ctx *ctx, const float *x, int B, float *xn_out, float *xa_out);
/* wm_model_set_xa + wm_model_cross_kv on xa f32 [B][1500][d]: xkv f32 [L][2][B][H][1500][64] (L = n_text_layer; bf16 widened).
 * The model's whole cross-K/V allocation holds WMDBG_SENTINEL_BF16 before the launches; an element behind the B chunks' cache
 * that no longer does is WM_ERR_STATE. */
WM_API int wmdbg_cross_kv(wm_ctx *ctx, const float *xa, int B, float *xkv_out);

/* LayerNorm over the last axis (eps 1e-5): f32 result and the bf16 result widened to f32.  Either output may be null (not
 * both): the kernel is then launched with that output null, as the encoder launches it. */
WM_API int wmdbg_layernorm(wm_ctx *ctx, const float *x, const float *g, const float *b, int rows, int d,
                    float *out_f32, float *out_bf16_as_f32);
/* Non-causal MHA, head_dim 64: q,k,v,out f32 [B][S][H*64]. */
WM_API int wmdbg_enc_attention(wm_ctx *ctx, const float *q, const float *k, const float *v, int B, int H, int S,
                        float *out);
/* The same; flags & 1: the 64 rows behind the last chunk's keys, which the last K tile reads and the kernel masks, hold NaN. */
WM_API int wmdbg_enc_attention_ex(wm_ctx *ctx, const float *q, const float *k, const float *v, int B, int H, int S, int flags,
                           float *out);
/* Decode-step skinny GEMM (the DE_Q epilogue): out[B][N] = (ln_g ? LayerNorm(x) : x) . W[N][K]^T + bias; 1 <= B <= WM_DEC_MAXB
 * (128). */
WM_API int wmdbg_dec_gemv(wm_ctx *ctx, const float *x, const float *ln_g, const float *ln_b, const float *W,
                   const float *bias, float *out, int B, int N, int K);
/* The decoder's residual product (out-projection / fc2): resid[B][N] += x[B][K] . W[N][K]^T + bias, any B <= 128.
 * Also returns the bf16 copy of the updated residual (widened to f32) and its per-row (sum, sum of squares) rebuilt from
 * the per-tile LayerNorm partials the kernel leaves for the next folded GEMV: stats [B][2]. */
WM_API int wmdbg_dec_gemv_resid(wm_ctx *ctx, const float *x, const float *W, const float *bias, float *resid, float *copy_bf16,
                         float *stats, int B, int N, int K);
/* The LayerNorm-folded decode GEMV with any of its layer epilogues at any decode-group size, driven as the decoder drives it:
 * wm_ln_fold on the bf16 weights, then wm_dec_gemv on bf16 activations in WL_TILED order with the producer's K/16 partial
 * statistics of the f32 rows.  epi: 0 = DE_QKV (N = 3 d, d = n_head * 64: q third -> out_f32 [B][d], k / v thirds -> row pos
 * of the caches), 1 = DE_Q (out_f32 [B][N]), 3 = DE_GELU (out_bf16 [B][N], un-tiled and widened; N % 32 == 0).  1 <= B <=
 * WM_DEC_MAXB, K % 64 == 0, K <= 1280; bias nullable.  centre != 0: the activations are bf16(x - mean_b) with mean_in = the
 * rows' f32 means, the statistics still those of the raw x (how the decoder holds its residual stream).  DE_QKV: kcache /
 * vcache f32 [B][n_head][T][64] = the bf16 caches widened, pre-filled with the bf16 bit pattern WMDBG_SENTINEL_BF16 (a NaN);
 * pos in [0, T) is read by the kernel from device memory.  Pointers of outputs an epilogue does not have may be NULL.  Always:
 * mean_out f32 [B] (pre-filled with the NaN bits WMDBG_SENTINEL_F32), and the fold on its own: Wf f32 [pad16(N)][K] (the folded
 * bf16 weights, un-tiled and widened), c1 / c2 f32 [pad16(N)]. */
#define WMDBG_SENTINEL_BF16 0x7fc5u
#define WMDBG_SENTINEL_F32 0x7fc0deadu
WM_API int wmdbg_dec_gemv_ln(wm_ctx *ctx, int epi, const float *x, const float *ln_g, const float *ln_b, const float *W,
                             const float *bias, int B, int N, int K, int centre, int n_head, int T, int pos, float *out_f32,
                             float *out_bf16, float *kcache, float *vcache, float *mean_out, float *Wf, float *c1, float *c2);

/* One decode position's logits launch and its close, as wm_model_decode_step / wm_model_close_step make them: wm_ln_fold of
 * the token embedding, wm_dec_gemv with DE_LOGITS (x_on == 0) or DE_LOGITS_X, then wm_argmax_embed with the arrival counter,
 * on one stream with the position in device memory.  All pointers are host memory; "in/out" fields are read and overwritten.
 * The activations are staged mean-centred (see wmdbg_dec_gemv_ln).  Every per-tile partial buffer (tile maxima, timestamp
 * keys and partials, the X-mode partials) is pre-filled with 0xff bytes, so a partial the close reads must have been written
 * by this position's logits launch. */
typedef struct wmdbg_step {
    /* geometry: B rows (1 .. WM_DEC_MAXB), vocabulary V (>= 16), width K (K % 64 == 0, <= 1280), context n_ctx, decode position
     * pos in [0, n_ctx), n_prompt >= 1 (positions pos + 1 >= n_prompt are generated) */
    int32_t B, V, K, n_ctx, pos, n_prompt;
    const float *x;        /* [B][K] the residual stream in front of the final LayerNorm */
    const float *ln_g, *ln_b;   /* [K] */
    const float *emb;      /* [V][K] token embedding (rounded to bf16): folded copy for the product, plain copy for the embedding */
    const float *bias;     /* [V] or NULL: added to the logits (the model has none; places maxima) */
    const float *pemb;     /* [n_ctx][K] positional embedding */
    int32_t *seq;          /* in/out [n_ctx][B] token history, position-major (a token generated for position n_ctx is not returned here) */
    /* filters: ids suppressed at every position; ids suppressed when mask_first != 0 (this position is the first generated one) */
    const int32_t *suppress, *suppress_first;
    int32_t n_suppress, n_suppress_first, mask_first;
    int32_t arg_first, arg_last;   /* the arg-max range with the timestamp rules off */
    int32_t fallback_tok;          /* the token when nothing is admissible */
    /* timestamp rules: ts_mode 0 = off, 1 = the state wm_ts_init leaves, 2 = rng / hist as given */
    int32_t ts_mode, ts_begin, eot, max_initial;
    int32_t *rng, *hist;   /* [B][4] in (ts_mode 2) / out (ts_mode != 0) */
    /* X mode (log-probs, no-speech, sampling at temperature > 0) */
    int32_t x_on, chunk0, sot_pos, ns_tok;
    float temperature;
    uint64_t seed;
    /* early stop: done in/out [B]; budget [B] or NULL */
    int32_t stop_on, stop_eot, pad_tok;
    int32_t *done;
    const int32_t *budget;
    const int32_t *off;    /* [B] ragged row offsets or NULL */
    /* outputs */
    float *logits;         /* [B][V] the launch's f32 logits */
    int32_t *tok;          /* [B] result + arg_first: the token the close chose */
    int32_t *result;       /* [B] */
    float *logprob;        /* [B] the slot of generated index pos + 1 - n_prompt (X mode; else and for prompt positions the NaN bits WMDBG_SENTINEL_F32) */
    int32_t logprob_written;   /* entries of the whole [n_ctx][B] log-prob buffer that no longer hold the sentinel */
    float *nospeech;       /* [B], pre-filled with WMDBG_SENTINEL_F32 */
    int32_t *live_rows;    /* [B] (stop_on): the list the close rebuilt, -1 where it wrote nothing (entries n_live .. B - 1) */
    int32_t n_live;
    int32_t pos_out;       /* *pos_ptr after the close */
    int32_t arrive_out;    /* the arrival counter after the close (0 between launches) */
    float *x_next;         /* [B][K] the embedded next row, pre-filled with WMDBG_SENTINEL_F32 */
    float *xb_next;        /* [B][K] its bf16 copy, un-tiled and widened (pre-filled with WMDBG_SENTINEL_BF16) */
    float *stats_next;     /* [B][2] (sum, sum of squares) rebuilt from the K/16 statistics parts (buffer pre-filled with WMDBG_SENTINEL_F32) */
    int32_t stats_tail_nonzero;   /* words of parts 1 .. K/16 - 1 of the B rows that are not +0.0 */
} wmdbg_step;
WM_API int wmdbg_decode_close(wm_ctx *ctx, wmdbg_step *io);
/* The THREE closes on one step's partials.  wmdbg_decode_close's launches with x_on, temperature 0, ts_mode 0 or 2 and a
 * generated position; between the DE_LOGITS_X launch and the arg-max close -- before that close moves the rule state and the
 * position -- the beam close's list kernel (wm_beam_topk: B windows of N = 1) and the speculative round's accept + commit
 * (wm_spec_accept: B / w windows of w rows, w dividing B, the rows' ranges the step's rng; token buffer, positions, stop state
 * and statistics are scratch copies) run on the same partials.  Out, per row: the beam list's length, first token and first
 * log-prob (WM_MAX_BEAM + 1 slots per row are not returned: slot 0 only), the beam close's no_speech_prob (pre-filled with
 * WMDBG_SENTINEL_F32; written when sot_pos == pos), the accept kernel's winner and log-prob; the arg-max close's are io's. */
WM_API int wmdbg_decode_close_shared(wm_ctx *ctx, wmdbg_step *io, int w, int32_t *beam_n, int32_t *beam_tok, float *beam_lp,
                                     float *beam_nospeech, int32_t *acc_tok, float *acc_lp);
/* wmdbg_decode_close with the sampling rules on (wm_set_sampling_rules): the truncation launch between the logits launch and
 * the close, for the whole step.  The rules act on a sampling X-mode step (x_on, temperature > 0); with (0, 1, 0), x_on 0 or
 * temperature 0 the launches are wmdbg_decode_close's.  With first-position suppress ids, mask_first must say whether pos is
 * n_prompt - 1. */
WM_API int wmdbg_decode_close_trunc(wm_ctx *ctx, wmdbg_step *io, int top_k, float top_p, float min_p);
/* wmdbg_decode_close / wmdbg_decode_close_trunc with a temperature and a seed per row in force (wm_set_sampling_rows): one decode
 * position -- the logits launch, the truncation launch when the rules are on ((0, 1, 0): no truncation launch) and some row
 * samples, and the close -- with the rows' table handed to the X-mode kernels.  Needs x_on; io->temperature and io->seed are not
 * read; row_T[b] == 0 is an arg-max row.  struct wmdbg_step is unchanged: the row arrays [io->B] are arguments. */
/* wmdbg_decode_close_trunc's step with the given-tokens launch (wm_set_given_tokens, given.hip) last in front of the close: given
 * i32 [B], -1: the row decodes freely; NULL: no such launch.  With (0, 1, 0), or at temperature 0, no truncation launch runs.
 * Needs x_on.  Beside io's outputs: the rows' per-tile keys tilemax_out / key_ts_out u64 [B][n_tiles] (key_ts_out is written
 * under timestamp rules alone) and winner values win_out f32 [B][n_tiles][2] as the launches in front of the close left them,
 * n_tiles = (V + 15) / 16 -- so the rows the kernel must not touch compare byte for byte with the same step at given == NULL.
 * A given id outside [-1, V) answers WM_ERR_INVALID and launches nothing. */
WM_API int wmdbg_decode_close_given(wm_ctx *ctx, wmdbg_step *io, const int32_t *given, int top_k, float top_p, float min_p,
                                    uint64_t *tilemax_out, uint64_t *key_ts_out, float *win_out);
WM_API int wmdbg_decode_close_rows(wm_ctx *ctx, wmdbg_step *io, const float *row_T, const uint64_t *row_seed, int top_k, float top_p,
                                   float min_p);
/* wmdbg_decode_close with the repetition rules on (wm_set_repetition_rules: penalty, ngram, and io->eot as the rules' eot, in
 * [0, V] whatever ts_mode is): wm_repeat_state on the token history in front of a DE_LOGITS_XR launch.  Needs x_on and
 * n_prompt <= n_ctx.  The bitmaps are pre-filled with 0xff bytes.  (1.0, 0) runs the same kernels with empty rules. */
WM_API int wmdbg_decode_close_rep(wm_ctx *ctx, wmdbg_step *io, float penalty, int ngram);
/* The state kernel of the repetition rules alone (repeat.hip): seq i32 [n_ctx][B] (host, position-major; any values), the
 * history of row b = seq[n_prompt .. pos][b].  Out: seen / ban u32 [B][words], words = (pad16(V) + 31) / 32, bit (t & 31) of
 * word t >> 5; both pre-filled with 0xff bytes on the device, so a word the kernel does not write shows. */
WM_API int wmdbg_repeat_state(wm_ctx *ctx, const int32_t *seq, int B, int n_ctx, int pos, int n_prompt, int V, int ngram,
                              int32_t eot, uint32_t *seen_out, uint32_t *ban_out);
/* wmdbg_decode_close_rep with the sequence bias on as well (wm_set_sequence_bias: the table arguments are that call's, io->eot its
 * eot): wm_repeat_state, wm_seqbias_state behind it, then a DE_LOGITS_XB launch -- for n_seq = 0 too (an empty table).  The
 * per-row state is pre-filled with 0xff bytes.  WM_ERR_INVALID for a table wm_set_sequence_bias would refuse. */
WM_API int wmdbg_decode_close_sb(wm_ctx *ctx, wmdbg_step *io, float penalty, int ngram, const int32_t *tokens,
                                 const int32_t *seq_offsets, const float *bias, const uint8_t *boost_prefixes, int n_seq);
/* The state kernel of the sequence bias alone (seqbias.hip) behind wm_repeat_state with empty rules: seq as for
 * wmdbg_repeat_state, the table as for wm_set_sequence_bias with V as the vocabulary.  Out: hit / ban u32 [B][words],
 * words = (pad16(V) + 31) / 32; cnt i32 [B]; id i32 / total f32 [B][WM_MAX_BIAS_ENTRIES], the first cnt[b] of row b written; woff
 * i32 [B][words], the hit bits in the words below each word (the list index of its first hit id) -- everything pre-filled with 0xff bytes on the device, so a word or element the kernels do not write shows. */
WM_API int wmdbg_seqbias_state(wm_ctx *ctx, const int32_t *seq, int B, int n_ctx, int pos, int n_prompt, int V, const int32_t *tokens,
                               const int32_t *seq_offsets, const float *bias, const uint8_t *boost_prefixes, int n_seq, int32_t eot,
                               uint32_t *hit_out, uint32_t *ban_out, int32_t *cnt_out, int32_t *id_out, float *total_out,
                               int32_t *woff_out);
/* Row tables (wm_set_sequence_bias_tables) on the host, no context and no device: the tables as that call takes them with V as the
 * vocabulary, each checked and expanded on its own and concatenated into the pool.  counts_out i32 [3] = tables, groups, entries;
 * the other outputs (each may be NULL: call once for the counts) = tab_grp i32 [tables + 1] (table t is groups [tab_grp[t],
 * tab_grp[t + 1])), grp_id i32 [groups], grp_beg i32 [groups + 1] (absolute into the pool's entries; nothing written for 0
 * tables), ent_len i32 / ent_bias f32 [entries], ent_ctx i32 [entries][31] newest token first.  WM_ERR_INVALID -- and nothing
 * written -- where wm_set_sequence_bias_tables answers it. */
WM_API int wmdbg_sb_expand_tables(const int32_t *tokens, const int32_t *seq_offsets, const float *bias, const uint8_t *boost_prefixes,
                                  const int32_t *table_offsets, int n_tables, int32_t eot, int V, int32_t *counts_out,
                                  int32_t *tab_grp_out, int32_t *grp_id_out, int32_t *grp_beg_out, int32_t *ent_len_out,
                                  float *ent_bias_out, int32_t *ent_ctx_out);
/* The per-row group ranges a decode group uploads under row tables (tx_plan.cpp wm_group_bias_rows; the group-tables dump of
 * wmdbg_group_tables is left as it is): table_of_row i32 [B] of the call (wm_set_bias_rows), the group of windows [b0, b0 + Cg) x N
 * candidates, tab_grp [n_tables + 1] -> rng_out i32 [Cg * N][2] = (first group, end group) of each decoder row; (0, 0) for -1. */
/* wm_group_given (tx_plan.h): the given-tokens table of the group of windows [b0, b0 + Cg) x N of a call whose table is lens
 * i32 [rows] / tokens i32 [rows][stride].  Out: lens_out i32 [Cg * N], tok_out i32 [Cg * N][max(L, 1)] (tok_cap words of room), *L_out
 * = L, the group's longest given text (0: no row of the group is given).  Host only. */
WM_API int wmdbg_group_given(const int32_t *lens, const int32_t *tokens, int stride, int rows, int b0, int Cg, int N, int32_t *lens_out,
                             int32_t *tok_out, int tok_cap, int32_t *L_out);
WM_API int wmdbg_group_bias_rows(const int32_t *table_of_row, int B, const int32_t *tab_grp, int n_tables, int b0, int Cg, int N,
                                 int32_t *rng_out);
/* The state kernel of the row tables alone (seqbias_rows.hip), as wmdbg_seqbias_state: the tables as for
 * wm_set_sequence_bias_tables (n_tables >= 1), table_of_row i32 [B] in [-1, n_tables).  ban_in NULL: behind wm_repeat_state with
 * empty rules, as the product runs it; else u32 [B][words] the ban words as given and NO wm_repeat_state launch -- what the kernel
 * leaves alone shows.  Outputs as wmdbg_seqbias_state's, pre-filled with 0xff bytes. */
WM_API int wmdbg_seqbias_rows_state(wm_ctx *ctx, const int32_t *seq, int B, int n_ctx, int pos, int n_prompt, int V,
                                    const int32_t *tokens, const int32_t *seq_offsets, const float *bias,
                                    const uint8_t *boost_prefixes, const int32_t *table_offsets, int n_tables, int32_t eot,
                                    const int32_t *table_of_row, const uint32_t *ban_in, uint32_t *hit_out, uint32_t *ban_out,
                                    int32_t *cnt_out, int32_t *id_out, float *total_out, int32_t *woff_out);
/* The state kernel of the constraint alone (constraint.hip): seq as for wmdbg_repeat_state; the automaton as for
 * wm_set_constraint with V as the vocabulary (WM_ERR_INVALID where that call answers it; n_states >= 1); starts i32 [B] in
 * [-1, n_states); ban_in u32 [B][words], words = (pad16(V) + 31) / 32: the ban words as given -- NO wm_repeat_state launch, so what
 * the kernel leaves alone shows.  Out: ban_out u32 [B][words]; state_out i32 [B] the state each row reached (-1: dead), pre-filled
 * with 0xfe bytes (0xff bytes would read as the dead state), so a row the kernel does not write reads 0xfefefefe. */
WM_API int wmdbg_constraint_state(wm_ctx *ctx, const int32_t *seq, int B, int n_ctx, int pos, int n_prompt, int V,
                                  const int32_t *edge_beg, const int32_t *edge_tok, const int32_t *edge_next, const int32_t *def_next,
                                  const uint8_t *accept, int n_states, int32_t eot, const int32_t *starts, const uint32_t *ban_in,
                                  uint32_t *ban_out, int32_t *state_out);
/* wmdbg_decode_close_rep with empty rules (1.0, 0) and the constraint on (wm_set_constraint: the automaton arguments are that
 * call's, eot its eot -- the rules' eot stays io->eot; starts i32 [B]): wm_repeat_state, wm_constraint_state behind it, then the
 * DE_LOGITS_XR launch and the close.  WM_ERR_INVALID for an automaton wm_set_constraint would refuse. */
WM_API int wmdbg_decode_close_cst(wm_ctx *ctx, wmdbg_step *io, const int32_t *edge_beg, const int32_t *edge_tok,
                                  const int32_t *edge_next, const int32_t *def_next, const uint8_t *accept, int n_states, int32_t eot,
                                  const int32_t *starts);
/* For callers that restate the struct (ctypes): out4 = sizeof(wmdbg_step) and the offsets of seed, logits and
 * stats_tail_nonzero (host only). */
WM_API int wmdbg_step_layout(int32_t *out4);

/* Single-query attention over a cache: q [B][H*64], k/v [B][H][T][64], keys 0..n_keys-1;
 * out = the bf16 head outputs widened to f32.  nsplit in 1..8. */
WM_API int wmdbg_dec_attention(wm_ctx *ctx, const float *q, const float *k, const float *v, int B, int H, int T,
                        int n_keys, int nsplit, float *out);
/* The decoder's causal self-attention launch at position pos with per-row offsets (ragged decode groups): sequence b
 * attends to the cache rows [min(off[b], pos), pos] of k/v [B][H][T][64]; off i32 [B], each in [0, T).  The cache is used
 * as given (rounded to bf16): rows outside that range may hold anything, NaN included. */
WM_API int wmdbg_dec_self_attention_off(wm_ctx *ctx, const float *q, const float *k, const float *v, int B, int H, int T,
                                        int pos, const int32_t *off, float *out);

/* Every decode-attention launch form alone, driven as the decode step drives it: one call of wm_dec_attention (form 0),
 * wm_dec_attention_cand (1), wm_dec_xattn_fq (2) or wm_dec_self_attention (3) on host data.  All pointers are host memory.
 * rows = B (forms 0, 2, 3) or C * N (form 1: row c * N + s = candidate s of window c); cache entries = B, or C for form 1.
 * Nothing is launched for a geometry the launcher's plan refuses, or when an address would leave a buffer (T outside
 * 1 .. WM_ATT_MAXK, no key or more than T, an offset outside [0, T), a live list that is not ascending rows of the group, a
 * packed field that does not fit): WM_ERR_INVALID with the reason in wm_last_error(), `out` (and mean_out) left at the
 * sentinels, plan[0] = the plan's status. */
typedef struct wmdbg_attn {
    int32_t form;
    int32_t B, C, N, H;        /* B rows, or C windows x N candidates; H heads of 64 */
    int32_t T;                 /* cache rows per (entry, head) pair */
    int32_t n_keys;            /* the constant key count (pos < 0) */
    int32_t nsplit;            /* form 0: workgroups per pair, 1 / 2 / 4 / 8 */
    int32_t pos;               /* >= 0 (forms 0 and 3): uploaded and passed as pos_ptr, keys 0 .. pos (form 0: n_keys = pos + 1 as
                                  well, the cross kernels' row clamp); -1: n_keys keys */
    int32_t n_live;            /* entries of live_rows */
    int32_t short_lived;       /* forms 0 and 1: the shape of a burst that shares the chip */
    int32_t warm_rows, warm_k; /* both non-zero: a [warm_rows][warm_k] bf16 matrix is allocated and passed as the warm-up matrix
                                  (warm_rows % 16 == 0, warm_k % 32 == 0) */
    int32_t K;                 /* form 2: the width of the query projection (= H * 64, <= 1280) */
    const int32_t *off;        /* form 3, with pos >= 0: [B] row offsets, each in [0, T): row b's keys are [min(off[b], pos), pos]; NULL: none.
                                  A row with pos < off[b] has not started: its output is finite, nothing more */
    const int32_t *live_rows;  /* the compact ascending list of the n_live live rows; NULL: every row is live */
    const float *q;            /* forms 0, 1, 3: [rows][H * 64] */
    const float *k, *v;        /* [entries][H][T][64], rounded to bf16; rows outside a pair's key range may hold anything, NaN included */
    /* form 2, the query side as wmdbg_dec_gemv_ln takes it (DE_Q, centre = 1; wm_ln_fold runs first): */
    const float *x;            /* [B][K] */
    const float *ln_g, *ln_b;  /* [K] */
    const float *Wq;           /* [K][K] */
    const float *bias;         /* [K] or NULL */
    /* outputs */
    float *out;                /* [ceil16(rows)][H * 64]: the bf16 head outputs widened; the device buffer is pre-filled with
                                  WMDBG_SENTINEL_BF16, which rows that are not live and the pad rows must still hold */
    float *mean_out;           /* form 2: [B], pre-filled with WMDBG_SENTINEL_F32 */
    int32_t plan[16];          /* the wmdbg_dec_attn_plan output record of the plan the launcher used (same plan function, the
                                  context's CUs, the current wmdbg_set_tuning state) */
} wmdbg_attn;
WM_API int wmdbg_dec_attention_form(wm_ctx *ctx, wmdbg_attn *io);
/* For callers that restate the struct (ctypes): out4 = sizeof(wmdbg_attn) and the offsets of off, out and plan (host only). */
WM_API int wmdbg_attn_layout(int32_t *out4);

/* ---- teacher-forced panels (wm_set_teacher_panel): the panel launches of a step alone, on host data.  A panel is C windows x
 * w consecutive positions pos .. pos + w - 1, row r = c * w + s; 1 <= w <= WM_MAX_TEACHER_PANEL, C * w <= WM_DEC_MAXB. ---- */
/* The self-attention launch of a panel step: q f32 [C * w][H * 64], k / v f32 [C][H][T][64] (rounded to bf16; window c's entry
 * already holds positions 0 .. pos + w - 1), row (c, s) attends to rows [0, pos + s] of entry c.  out f32 [out_rows][H * 64],
 * out_rows a multiple of 16 and >= C * w: the bf16 head outputs widened; the device buffer is pre-filled with the bf16 bit
 * pattern WMDBG_SENTINEL_BF16, which rows >= C * w must still hold. */
WM_API int wmdbg_dec_self_attention_panel(wm_ctx *ctx, const float *q, const float *k, const float *v, int C, int w, int H,
                                          int T, int pos, int out_rows, float *out);
/* wmdbg_dec_gemv_ln's DE_QKV launch (centre = 1) with the panel epilogue: x f32 [C * w][K]; q_out f32 [C * w][N / 3];
 * kcache / vcache f32 [C][n_head][T][64], pre-filled with WMDBG_SENTINEL_BF16: row (c, s) appends at position pos + s of entry c. */
WM_API int wmdbg_dec_qkv_panel(wm_ctx *ctx, const float *x, const float *ln_g, const float *ln_b, const float *W,
                               const float *bias, int C, int w, int N, int K, int n_head, int T, int pos, float *q_out,
                               float *kcache, float *vcache);
/* The panel embedding: emb f32 [V][d] (rounded to bf16), pemb f32 [n_ctx][d], seq i32 [n_ctx][stride] (position-major), the
 * panel's windows are columns c0 .. c0 + C - 1.  Out, per row r: x f32 [C * w][d], xb f32 [C * w][d] (the mean-centred bf16
 * copy widened), stats f32 [C * w][d / 16][2] (the row's LayerNorm partials), mean f32 [C * w].  by_steps != 0: the same rows
 * from the STEP path's launches, position by position over the C windows (wm_dec_embed at position 0, the teacher-forced
 * close wm_argmax_embed afterwards). */
WM_API int wmdbg_dec_embed_panel(wm_ctx *ctx, const float *emb, const float *pemb, int V, int d, int n_ctx, const int32_t *seq,
                                 int stride, int c0, int C, int w, int pos, int by_steps, float *x, float *xb, float *stats,
                                 float *mean);
/* ---- prompt panels (wm_set_prompt_panel): the panel launches of a RAGGED group, and the plan ---- */
/* wmdbg_dec_self_attention_panel with the windows' offsets off i32 [C], each in [0, T): row (c, s) is group position
 * p = pos + s of window c and attends to the rows [min(off[c], p), p] of entry c -- the bits of wmdbg_dec_self_attention_off at
 * position p.  A row with p < off[c] has not started: its output is finite, nothing more.  Cache rows outside a row's range may
 * hold anything, NaN included. */
WM_API int wmdbg_dec_self_attention_panel_off(wm_ctx *ctx, const float *q, const float *k, const float *v, int C, int w, int H,
                                              int T, int pos, const int32_t *off, int out_rows, float *out);
/* wmdbg_dec_embed_panel with the offsets off i32 [C] of the panel's windows, each in [0, n_ctx): the positional row of row
 * (c, s) is max(pos + s - off[c], 0).  by_steps != 0: the step path's launches with the same offsets. */
WM_API int wmdbg_dec_embed_panel_off(wm_ctx *ctx, const float *emb, const float *pemb, int V, int d, int n_ctx, const int32_t *seq,
                                     int stride, int c0, int C, int w, int pos, const int32_t *off, int by_steps, float *x, float *xb,
                                     float *stats, float *mean);
/* The prompt-panel plan of a plain decode group (host only, tx_plan.cpp wm_prompt_panel_plan): G rows (1 .. 128), the width
 * (1 .. 8), P prompt positions (a ragged group: its longest prompt), sot_pos = the <|startoftranscript|> position when
 * no_speech_prob is computed (else -1), acap_base = an aligned group's first captured position (else -1); both < P.
 * out i32 [5] = P0 (the group's first ordinary step), C (windows per slice), w' (positions per panel), slices, panel steps per
 * slice.  No prefill (width 1, or P0 < 2): C = w' = slices = steps = 0.  _batch: n cases, in i32 [n][5] in the argument order,
 * out i32 [n][5]. */
WM_API int wmdbg_prompt_panel_plan(int G, int width, int P, int sot_pos, int acap_base, int32_t *out);
WM_API int wmdbg_prompt_panel_plan_batch(int n, const int32_t *in, int32_t *out);
/* What the context's last decode-group prefill enqueued as prompt panels: out i32 [3] = P0, slices, panel steps (all slices).
 * All 0 when that group ran none (width 1, P0 < 2, a candidate / beam / speculative group). */
WM_API int wmdbg_last_prompt_prefill(wm_ctx *ctx, int32_t *out);
/* ---- given panels (wm_set_given_panel): the plan, and what the last group ran ---- */
/* The given-panel plan of a decode group (host only, tx_plan.cpp wm_given_panel_plan): G rows (1 .. 128), the width (1 .. 8),
 * lens i32 [G] the rows' given tokens, budgets i32 [G] or NULL, max_new, P prompt positions, n_text_ctx, and the group's mode as a
 * bit word: 1 a given row, 2 candidates or beams, 4 ragged prompts, 8 extended decode, 16 sampling row map, 32 sampling rules in
 * force at temperature > 0, 64 alternatives, 128 bias row tables, 256 sequence bias, 512 constraint, 1024 repetition-rule state,
 * 2048 alignment capture, 4096 all-f32 path / debug hooks, 8192 temperature > 0.  out i32 [4] = reason (0: served; else the first
 * test of the rule that failed, in the rule's order: 1 width 1, 2 no table, 3 candidates, 4 ragged, 5 no extended decode, 6 row
 * map, 7 temperature, 8 alternatives, 9 row tables, 10 bias, 11 constraint, 12 repetition rules, 13 capture, 14 f32 / hooks,
 * 15 min(width, 128 / G) < 2, 16 Lp <= 1), w, Lp, rounds.  _batch: n cases of 8 + 2 g_max words each -- G, width, max_new, P,
 * n_text_ctx, bits, budgets given, 0, lens [g_max], budgets [g_max] -- out i32 [n][4]. */
WM_API int wmdbg_given_panel_plan(int G, int width, const int32_t *lens, const int32_t *budgets, int max_new, int P, int n_text_ctx,
                                  uint32_t bits, int32_t *out);
WM_API int wmdbg_given_panel_plan_batch(int n, int g_max, const int32_t *in, int32_t *out);
/* What the context's last decode group ran as given panels: out i32 [4] = first and last generated index of the phase, rounds,
 * width w.  All 0 when that group ran none. */
WM_API int wmdbg_last_given_panel(wm_ctx *ctx, int32_t *out);
/* ... and of the context's lanes (wm_set_lanes): lane 0 is the context itself, lane k >= 1 its k-th clone, which ran the groups the
 * scheduler handed it.  WM_ERR_INVALID for a lane the context does not have. */
WM_API int wmdbg_last_given_panel_lane(wm_ctx *ctx, int lane, int32_t *out);
/* ONE ROUND of a given-panel phase on caller-given state, the kernels of given_panel.hip alone: stage, the hook's own logits
 * launch (final LayerNorm + tied-embedding product with the extended-decode epilogue over the G x w rows x, as
 * wmdbg_decode_close builds it, under the ranges the stage left in the rows' slots), close, commit.  Row c * w + s is window c at
 * position pos + s; pos >= n_prompt, pos + w < n_ctx, and the round's generated indices pos + 1 - n_prompt .. + w - 1 lie below
 * max_new.  R = 128 entries per state buffer whatever G is: every buffer marked in/out goes up whole and comes down whole, so a
 * caller's sentinels show what the kernels left alone.  ts_mode 0 or 2 (rng / hist as given); first / last: the phase's first /
 * last round (first: the committed state is taken from hist / rng [G]; last: hist / rng get the [G] layout back). */
typedef struct {
    int32_t G, w, V, K, n_ctx, pos, n_prompt, max_new, first, last;
    const float *x;             /* [G * w][K] the residual stream in front of the final LayerNorm */
    const float *ln_g, *ln_b;   /* [K] */
    const float *emb;           /* [V][K] token embedding (rounded to bf16) */
    const float *bias;          /* [V] or NULL: added to the logits (places maxima) */
    const int32_t *suppress;    /* ids suppressed at every position */
    int32_t n_suppress, fallback_tok;
    int32_t ts_mode, ts_begin, eot;
    int32_t *hist, *rng;        /* in/out [R][4] the step path's slots: [G] committed in front of the first round, the rows' ranges after */
    int32_t *chist, *crng;      /* in/out [R][4] the side area */
    int32_t stop_on, stop_eot, pad_tok;
    int32_t *done;              /* in/out [R] (stop_on) */
    const int32_t *budget;      /* [G] or NULL */
    int32_t *live_rows;         /* in/out [R] (stop_on) */
    int32_t n_live;             /* in/out (stop_on) */
    const int32_t *glens, *gtok;   /* the group's table: lens [G], tokens [G][stride] */
    int32_t stride;
    int32_t *seq;               /* in/out [n_ctx + 1][G] */
    float *logprob;             /* in/out [max_new][G] */
    int32_t *wtok;              /* in/out [R] the rows' tokens as the close left them */
    float *wlp;                 /* in/out [R] */
    float *logits;              /* out [G * w][V] the launch's f32 rows */
    int32_t pos_out;
} wmdbg_given_panel;
WM_API int wmdbg_given_panel_round(wm_ctx *ctx, wmdbg_given_panel *io);
/* The query capture of an alignment layer in a panel step: dq f32 [C * w][d], the layer's n_heads heads into slots slot0 .. of
 * cap f32 [C][Tq][J][64], pre-filled with the NaN bits WMDBG_SENTINEL_F32 (rows at positions >= Tq are not captured).
 * by_steps != 0: w step launches over the C windows instead. */
WM_API int wmdbg_align_capture_panel(wm_ctx *ctx, const float *dq, int d, int C, int w, int pos, const int32_t *heads,
                                     int n_heads, int slot0, int Tq, int J, int by_steps, float *cap);
/* The token-probability launch of a panel step: logits f32 [C * w][ldo], seq i32 [n_ctx][C] (ids < eot), chunk c has n_text[c]
 * text tokens at positions S .. S + n_text[c] - 1; prob f32 [C][max_text], pre-filled with WMDBG_SENTINEL_F32 -- a row writes
 * only when its own position is one of its chunk's text positions.  by_steps != 0: w step launches instead. */
WM_API int wmdbg_align_token_prob_panel(wm_ctx *ctx, const float *logits, int C, int w, int V, int ldo, const int32_t *seq,
                                        int n_ctx, int pos, int S, int eot, const int32_t *n_text, int max_text, int by_steps,
                                        float *prob);

/* ---- micro-benchmarks: average microseconds per launch over `iters` back-to-back launches
 * that cycle over n_mats weight matrices / n_slices cache slices (defeats L2 / MALL reuse). */
WM_API int wmdbg_bench_dec_gemv(wm_ctx *ctx, int B, int N, int K, int ln, int resid, int n_mats, int iters,
                         int nw_override, float *avg_us);
WM_API int wmdbg_bench_dec_attention(wm_ctx *ctx, int B, int H, int T, int n_keys, int nsplit, int n_slices,
                              int iters, float *avg_us);

/* Dependent-launch floor: average microseconds per trivial kernel, eager vs hipGraph replay. */
WM_API int wmdbg_bench_launch_floor(wm_ctx *ctx, int iters, int grid, float *eager_us, float *graph_us);

/* Wall time (us) of one replay of a captured graph with ONE chain of `iters` spinning kernels vs TWO
 * independent chains: tells whether hipGraph runs parallel branches concurrently on this runtime. */
WM_API int wmdbg_bench_graph_branches(wm_ctx *ctx, int iters, int grid, int us_each, float *one_us, float *two_us);

/* Mean duration (us) of one encoder GEMM launch, C[M][N] = A[M][K] W[N][K]^T, back to back, on encoder-like operands
 * (A ~ N(0,1), W ~ N(0,0.02^2)); launches rotate over n_w copies of W (n_w large: W streams from HBM as in the model). */
WM_API int wmdbg_bench_gemm(wm_ctx *ctx, int M, int N, int K, int epi, int iters, int n_w, float *us);

/* Force the encoder GEMM tile: 64 (64 x 64, 4 waves), 128 (128 x 128, 4 waves), 256 (256 x 256, 8 waves, staggered phases)
 * or 0 = automatic.  Process-wide; used by the parity tests and A/B probes to run every shape through every tile kernel. */
WM_API int wmdbg_set_gemm_tile(int tile);

/* sub-chip lanes (round 6): CU-masked decode groups of a wm_transcribe_greedy call (0: none, 2: two half-chip groups) for a
 * call of B chunks on a model of decoder width n_text_state; the 256-bit CU mask of the CUs [cu_lo, cu_hi) of every XCD */
WM_API int wmdbg_lane_parts(int B, int lanes, int explicit_lanes, int n_text_state);
WM_API int wmdbg_cu_mask(int cu_lo, int cu_hi, uint32_t *mask8);

/* The ALL-FP32 debug model path (BASELINE.md parity gate: "fp32 debug path must match to <= 1e-4 rel-L2"; csrc/f32_path.hip).
 * precision = WM_F32: wm_encode and wm_decode_logits of THIS context run with f32 activations, f32 K/V and f32 accumulation on
 * the very weights the product multiplies (the bf16 values in HBM, in their product layouts) -- separates bugs from rounding.
 * WM_BF16 restores the product kernels.  wm_detect_language / wm_transcribe_greedy are not affected. */
WM_API int wmdbg_set_precision(wm_ctx *ctx, int precision);

/* Launch-shape experiment knobs (csrc/wm_tuning.h, struct WmTuning), by name: "gemv_tn", "gemv_nblk", "gemv_no_ppw2",
 * "prefetch_max_b", "xattn_split_below", "xattn_wgs", "xattn_no_flat", "xattn_lds_pad", "xattn_splits", "gemm_tile",
 * "gemm_gm", "no_early_stop", "xattn_no_deep", "xattn_never_short", "logits_tn", "enc_attn_mfma_sum"; key "reset" restores the product's rules.  Process-wide.  The PRODUCT library has no such
 * entry point and reads no environment variable for launch shapes (rounds 1-3 had WM_GEMV_*, WM_XATTN_*, WM_GEMM_*). */
WM_API int wmdbg_set_tuning(const char *key, int value);
/* The product's group policy as a pure function: decode groups of a wm_transcribe_greedy call of B chunks with `lanes` lanes
 * available; explicit_lanes != 0: the host set the lane count with wm_set_lanes (host only, no GPU). */
WM_API int wmdbg_group_count(int B, int lanes, int explicit_lanes);
/* The prompt table of one decode group of a wm_transcribe_mel_ragged call as a pure function (host only): rows
 * [b0, b0 + Bg) of prompts [.][stride] with lengths prompt_len, right-aligned to the group's own longest prompt P (returned).
 * table_out i32 [P][Bg] (room for stride * Bg), position-major like the device's token buffer; off_out i32 [Bg] = P - len. */
WM_API int wmdbg_right_align(const int32_t *prompts, int stride, const int32_t *prompt_len, int b0, int Bg, int32_t *table_out,
                             int32_t *off_out);

/* The decode groups of a wm_transcribe_mel_best_of call of B windows x N candidates as a pure function (host only): group g
 * holds windows [b0_out[g], b0_out[g] + cg_out[g]) = cg_out[g] * N decoder rows.  Returns the number of groups (room for B
 * entries in both arrays), or -1 on bad arguments. */
WM_API int wmdbg_cand_groups(int B, int N, int lanes, int explicit_lanes, int32_t *b0_out, int32_t *cg_out);
/* The decode step's launch plans as pure functions (host only, no context, no GPU; csrc/dec_launch.h), under the current
 * wmdbg_set_tuning state, for n cases at once; return n, or -1 on bad arguments.
 * wmdbg_dec_attn_plan: in i32 [n][16] = form (0 cross, 1 candidate group, 2 fused query, 3 self, 4 panel), B, C, N (panel: the
 *   width), H, T_stride, n_keys, nsplit, K (fused query), flags (1 device position, 2 partials buffer, 4 row offsets, 8 warm-up
 *   matrix, 16 short_lived, 32 live list -- which no plan reads), pf_rows, pf_k, CUs of the lane, 0, 0, 0;
 *   out i32 [n][16] = status (WM_OK / WM_ERR_INVALID; the rest 0 when refused), variant (DecAttnVariant), spw, grid x, grid y,
 *   block, dynamic LDS bytes, compute workgroups, warm-up tiles, bytes per tile, packA, packB, packC, combine grid (0: none),
 *   [14] (also when refused; B <= 128 and H <= 255 only) = cross: wm_dec_attn_splits(B, H); fused query: wm_dec_xattn_fq_applies(B, H, K, short_lived), 0.
 * wmdbg_dec_gemv_plan: in i32 [n][12] = epilogue (DecEpi), LayerNorm mode, B, N, K, warm-up matrix present, pf_rows, pf_k,
 *   pf_head_major, CUs of the lane, 0, 0;  out i32 [n][20] = status, nw, spw, tn, nblk, ppw, row split, bgroups, n_tiles, n_tg,
 *   n_tg_pad, grid, block, dynamic LDS bytes, warm-up tiles, bytes per tile, pf_head_major, 0, 0, 0. */
WM_API int wmdbg_dec_attn_plan(const int32_t *in, int n, int32_t *out);
WM_API int wmdbg_dec_gemv_plan(const int32_t *in, int n, int32_t *out);
/* The host arithmetic of a transcribe call as pure functions (host only, no context, no GPU; csrc/tx_plan.h), for n cases at
 * once; each returns n, or -1 on bad arguments or a case it refuses.  None reads the wmdbg_set_tuning state.
 * wmdbg_tx_plan: the lane plan.  in i32 [n][12] = B (rows of the call; a candidate call: windows), N (candidates per row), the
 *   lane limit, explicit_lanes, prof_on, no_cu_masks, n_text_state, then the knobs lane_parts, lane_solo_cus, group_chunks, 0, 0;
 *   out i32 [n][8] = L, parts, G, n_lanes, kind (0 the caller's context and its clones, 1 part lanes, 2 the solo lane), the
 *   case's first entry in cut, 0, 0;  cut i32 [cut_cap]: per case b0[0 .. G) then cg[0 .. G), the cases back to back.
 * wmdbg_group_tables: what a decode group uploads.  in i32 [n][256] = B, b0, Cg, N, prompt stride (0: one prompt for all),
 *   ragged, n_prompt (of a uniform call), budgets given, sample ids given, extended decode on, 0 ...; [16] prompt_len [B],
 *   [32] budgets [B], [48] sample_ids [B], [64] prompts [B][stride] (B <= 16, Cg * N <= 16, stride and n_prompt <= 12);
 *   out i32 [n][576] = P, entries of the prompt table, of the offsets, of the budgets, of the id words, 0 ...; [16] the table
 *   [P][Cg * N], [208] offsets, [224] budgets, [240] id words: a candidate group's [2][144], else the rows' sample ids.
 * wmdbg_group_rows_out: the output rows of a finished group.  in i32 [n][320] = B, b0 (first row of the call; a candidate
 *   call: window), Bg (decoder rows), N, max_new (<= 8), eot, budgets given, log-probs wanted, no-speech wanted, 0 ...;
 *   [16] gen [max_new][Bg], [144] log-probs (f32 bits) [max_new][Bg], [272] no-speech (f32 bits) [Bg], [288] budgets [B]
 *   (B * N <= 16);  out i32 [n][288], the caller's fill staying wherever no row is written = [0] tokens [B * N][max_new],
 *   [128] lens [B * N], [144] log-probs (f32 bits), [272] no-speech (f32 bits) [B]. */
WM_API int wmdbg_tx_plan(const int32_t *in, int n, int32_t *out, int32_t *cut, int cut_cap);
/* wmdbg_tx_plan with the plan's optional upper bound on the rows of one group beside each case (max_group_rows i32 [n]; 0:
 * none, and then the case's plan is wmdbg_tx_plan's): an aligned transcribe call's capture budget. */
WM_API int wmdbg_tx_plan_bounded(const int32_t *in, const int32_t *max_group_rows, int n, int32_t *out, int32_t *cut, int cut_cap);
WM_API int wmdbg_group_tables(const int32_t *in, int n, int32_t *out);
WM_API int wmdbg_group_rows_out(const int32_t *in, int n, int32_t *out);
/* Speculative decoding (wm_transcribe_mel_speculative): the pure host rules of tx_plan.cpp, restated in tests/spec_ref.py.
 * wmdbg_spec_groups: the decode groups of B windows at draft length k and preferred group size spec_group (0: the default) into
 *   b0_out / cg_out [<= B]; returns their number (-1: bad arguments).
 * wmdbg_spec_width: the width of the next verify step from the draft length, an upper bound on the device position and the
 *   last position a row may have (0: none).
 * wmdbg_spec_round: one round of G windows whose verify step had w rows each -- accepted / live / eot_at (index of the first
 *   end-of-text among a window's own tokens, -1: none) / left (tokens its budget still allows) i32 [G] -> returns n, the
 *   positions the group advances; live_out i32 [G]; inc_out i32 [G][4] = increments of (rounds, proposed, accepted, kept). */
WM_API int wmdbg_spec_groups(int B, int k, int spec_group, int32_t *b0_out, int32_t *cg_out);
WM_API int wmdbg_spec_width(int k, int bound, int last);
WM_API int wmdbg_spec_round(int G, int w, const int32_t *accepted, const int32_t *live, const int32_t *eot_at, const int32_t *left,
                            int32_t *live_out, int32_t *inc_out);
/* wmdbg_spec_round over n cases of one shape: in i32 [n][4][G] = accepted | live | eot_at | left, out i32 [n][1 + 5 G] = n |
 * live_out [G] | inc [G][4]; returns n (-1: bad arguments). */
WM_API int wmdbg_spec_round_batch(int n, int G, int w, const int32_t *in, int32_t *out);
/* The next-call state of a transcribe call (csrc/tx_pending.h), on the CPU.
 * wmdbg_pending_refusal: who serves which pending item.  pending: bits 1 budgets | 2 bias row map | 4 constraint row map |
 *   8 sampling row map | 16 alternatives; the call: entry 0 plain | 1 mel | 2 ragged | 3 best-of | 4 beam, flags 1 greedy entry |
 *   2 beam | 4 rows of a window set | 8 hypothesis-aligned | 16 speculative | 32 multi | 64 all-f32 path, n_cand.  Alternatives
 *   are judged first; a caller masks `pending` to the items it answers for at that point.  Returns WM_OK (served) or
 *   WM_ERR_STATE (-1: bad arguments) and writes the message ("" when served) to msg_out [msg_cap].
 * wmdbg_pending_take: take() on a value of its own, armed with the items `bits` names, taken, the member armed again with
 *   `again`.  out i32 [6] = bits armed | taken | left behind | the taken value's after the second arm | the member's then | the
 *   taken value's budget (1: the first arm's; 0: none). */
WM_API int wmdbg_pending_refusal(unsigned pending, int entry, unsigned flags, int n_cand, char *msg_out, int msg_cap);
WM_API int wmdbg_pending_take(unsigned bits, unsigned again, int32_t *out);
/* THE ONE-SHOTS' SCOPE (wmdbg_spec_script, wmdbg_align_capture, wmdbg_align_hyp, wmdbg_hyp_slots, wmdbg_beam_trace): each is
 * armed for the NEXT transcribe call on ctx of ANY kind, which takes all of them whatever its outcome and reads the ones that
 * are its own -- so arm one right in front of the call it is meant for: a plain transcribe call in between drops it. */
/* Scoped to the NEXT transcribe call on ctx (above); wm_transcribe_mel_speculative reads it: the proposal for generated
 * index i of row b of that call is tokens[b * max_new + i] (B and max_new must be the call's; ids inside the vocabulary).  The
 * draft model still runs; only what the target is asked to verify changes, so tests and timings fix the acceptance pattern
 * exactly.  tokens is host memory that lives until that call returns; NULL clears the hook. */
WM_API int wmdbg_spec_script(wm_ctx *ctx, const int32_t *tokens, int B, int max_new);
/* The accept and commit launches of one speculative round alone, timestamp rules off: G windows x w rows at position pos (rows
 * at positions pos .. pos + w - 1 <= n_prompt + max_new - 2).  tilemax u64 [G * w][n_tiles] packed (value, ~index) text keys, txt /
 * win f32 [G * w][n_tiles][2] the extended decode's partials -- (max, sum exp) of the tile's allowed ids, raw logit of its winner
 * -- as a verify step's logits launch leaves them; seq i32 [n_ctx][G] (in: the last token at pos, the proposals behind it; out:
 * the kept tokens), done i32 [G] (in / out), budget i32 [G] or NULL.  Out: logprob f32 [max_new][G] (zero where nothing was
 * written), stats i32 [G][4], round i32 [2] = (live windows, position), acc i32 [G], the draft's token buffer i32 [n_ctx][G]
 * (zero but for the token it continues from), pos_out i32 [2] = the target's and the draft's position. */
WM_API int wmdbg_spec_accept(wm_ctx *ctx, int G, int w, int n_tiles, int pos, int n_prompt, int n_ctx, int max_new, int32_t eot,
                             const int32_t *budget, const uint64_t *tilemax, const float *txt, const float *win, int32_t *seq,
                             int32_t *done, float *logprob_out, int32_t *stats_out, int32_t *round_out, int32_t *acc_out,
                             int32_t *draft_seq_out, int32_t *pos_out);
/* The bookkeeping kernels of a speculative round alone (spec.hip), each on caller-given state: which = 0 wm_spec_adopt
 * (spec_adopt_kernel), 1 wm_spec_stage (spec_stage_kernel), 2 wm_spec_commit (spec_commit_kernel WITHOUT the accept launch in
 * front of it: wtok, wlp and acc are the caller's).  G windows x w rows, 1 <= G <= WM_DEC_MAXB, 1 <= w <= 8, G * w <=
 * WM_DEC_MAXB, as the launchers take them; the rules of the target (tts) and of the draft (dts) are on or off independently.
 * Every buffer is host memory that the hook uploads WHOLE before the launch and downloads WHOLE behind it, whichever kernel
 * runs and whether the rules are on: the caller pre-fills what it does not give with a sentinel (the NaN bits
 * WMDBG_SENTINEL_F32 for floats, a fixed negative int) and reads from the buffers what was written and that nothing else was.
 * Per-window arrays have cap >= G rows, per-row arrays cap * w: rows behind the group's must come back untouched.  Nothing is
 * launched when a kernel could leave a buffer (bad geometry, n_prompt >= n_ctx for the adoption, a position outside
 * [n_prompt - 1, n_ctx) for the staging or with pos + w >= n_ctx for the commit, acc[c] outside [0, w)): WM_ERR_INVALID. */
typedef struct wmdbg_spec {
    int32_t which;
    int32_t G, w, cap;
    int32_t n_prompt, n_ctx, max_new, n_vocab;   /* WmSpecDev::max_new and n_vocab (the staging's clamp of proposal ids) */
    int32_t tts_on, dts_on;
    int32_t tts_par[4], dts_par[4];              /* ts_begin, eot, n_vocab, max_initial of WmTsDev */
    int32_t eot, pad_tok;                        /* WmStopDev */
    const int32_t *script;     /* [G][max_new] proposals by generated index, or NULL: the draft's own tokens */
    const int32_t *budget;     /* [cap] or NULL */
    int32_t *tseq, *dseq;      /* [n_ctx][G] the two token buffers */
    int32_t *pos2;             /* [2] the target's and the draft's device position */
    int32_t *tts_hist;         /* [cap][4] */
    int32_t *tts_rng;          /* [cap * w][4]: per window for the adoption, the verify step's per-row slots for the staging */
    int32_t *dts_hist, *dts_rng;                 /* [cap][4] */
    int32_t *chist, *crng, *dchist, *dcrng;      /* [cap][4] the committed states */
    int32_t *wtok;             /* [cap * w] */
    float *wlp;                /* [cap * w] */
    int32_t *acc, *done;       /* [cap] */
    int32_t *stats;            /* [cap][4] */
    int32_t *round;            /* [2] */
    int32_t *n_live;           /* [1] */
    float *logprob;            /* [max_new][G] */
} wmdbg_spec;
WM_API int wmdbg_spec_kernel(wm_ctx *ctx, wmdbg_spec *io);
/* For callers that restate the struct (ctypes): out4 = sizeof(wmdbg_spec) and the offsets of tts_par, script and logprob (host only). */
WM_API int wmdbg_spec_layout(int32_t *out4);
/* The cross-attention launch of a candidate group exactly as the decode step makes it (wm_dec_attention_cand): C windows x N
 * candidates, q f32 [C * N][H * 64] (row c * N + s = candidate s of window c), k / v f32 [C][H][T][64] (rounded to bf16), the
 * first n_keys positions; live_rows: the compact ascending list of the n_live live rows (NULL: every row is live);
 * out f32 [C * N][H * 64] -- rows that are not live are not written by the kernel. */
WM_API int wmdbg_dec_attention_cand(wm_ctx *ctx, const float *q, const float *k, const float *v, int C, int N, int H, int T,
                                    int n_keys, const int32_t *live_rows, int n_live, float *out);
/* The same launch in the shape of a burst that shares the chip with other decode groups (one short-lived 8-wave workgroup per
 * (window, head) pair, merge in LDS, whatever the pair count): same bits. */
WM_API int wmdbg_dec_attention_cand_shared(wm_ctx *ctx, const float *q, const float *k, const float *v, int C, int N, int H,
                                           int T, int n_keys, const int32_t *live_rows, int n_live, float *out);

/* The Gumbel noise wm_transcribe's sampling adds at temperature > 0, computed by the DEVICE code (csrc/philox.h): g(n) of
 * ids n0 .. n0 + count - 1 for chunk `chunk` of a call and generated index gi, into host g[count]. */
WM_API int wmdbg_sample_noise(wm_ctx *ctx, uint64_t seed, int chunk, int gi, int n0, int count, float *g);

/* The DTW kernel of wm_align alone, on host matrices: chunk b is x + b * max(N) * ld, N[b] rows (<= 448) x M[b] frames
 * (<= 1500, <= ld), row stride ld.  start_frame_out i32 [B][max(N)]: the first frame of every row on the path, -1 past N[b]. */
WM_API int wmdbg_dtw(wm_ctx *ctx, const float *x, int B, const int32_t *N, const int32_t *M, int ld, int32_t *start_frame_out);
/* Makes the NEXT wm_align or wm_align_mel call on ctx also return its cost matrix -- AFTER negation, i.e. x = -mean over heads, the matrix
 * the DTW runs on -- into matrix_out f32 [B][max_text + 1][1500] (0 outside each chunk's n + 1 rows x n_frames / 2 frames).
 * The next aligned transcribe call (wm_transcribe_mel_aligned, wm_transcribe_windows_aligned) is served the same way:
 * matrix_out f32 [B][max_new + 1][1500], 0 outside each row's len_b x M_b block.  Whichever comes first takes it: a wm_align
 * call, or a transcribe call of any kind (THE ONE-SHOTS' SCOPE above), which drops it when it is not an aligned one. */
WM_API int wmdbg_align_capture(wm_ctx *ctx, float *matrix_out);
/* The aligned best-of / beam calls (wm_transcribe_mel_best_of_aligned, wm_transcribe_mel_beam_aligned and the window-set
 * pair), each for the NEXT transcribe call on ctx only, read when that call is an aligned one (THE ONE-SHOTS' SCOPE above).
 * wmdbg_align_capture and wmdbg_beam_trace serve them too.
 * wmdbg_align_hyp: the call aligns hypothesis min(h, n_hyp - 1) of every window instead of best_out[b] (best-of: n_hyp =
 * best_of); best_out itself is the ranking's, as always.  For tests only.
 * wmdbg_hyp_slots: the call leaves the slot tables it aligned from in slots_out i32 [B][Tq], Tq = sot_tail + max_new - 1: entry t
 * is the candidate / beam (0 .. N - 1) whose capture slot held capture row t of the aligned hypothesis (zeros with one row per
 * window; entries at or past the hypothesis' own S + len rows are not read by the alignment). */
WM_API int wmdbg_align_hyp(wm_ctx *ctx, int h);
WM_API int wmdbg_hyp_slots(wm_ctx *ctx, int32_t *slots_out);
/* wm_beam_ancestry (csrc/beam.h), the host function an aligned beam group finds a hypothesis' capture slots with, for ONE window:
 * anc i32 [max_new][N] (the source beam of every slot at every close), fin_n finished hypotheses with fin_src / fin_len [fin_n],
 * wsteps closes, the live beams' sums f32 [N] (-inf: dead); h in the window's output order (finished first, then the live beams by
 * descending sum until there are N); S = sot_tail - 1.  Fills slot i32 [Tq] and returns the hypothesis' length, -1 when the window
 * has no hypothesis h, -2 on bad arguments.  Host only. */
WM_API int wmdbg_beam_ancestry(int N, int max_new, const int32_t *anc, int fin_n, const int32_t *fin_src, const int32_t *fin_len,
                               int wsteps, const float *sum, int h, int S, int Tq, int32_t *slot);
/* The gather kernel of an aligned best-of / beam group alone (align.hip), on host data: cap f32 [C * N][Tq][J][64], slot i32
 * [C][Tq] (each in [0, N)), n_rows i32 [C] (each in [0, Tq]); q_sel f32 [C][Tq][J][64] goes to the device as the caller filled
 * it and comes back with q_sel[c][t] = cap[c * N + slot[c][t]][t] for t < n_rows[c], everything else untouched. */
WM_API int wmdbg_align_gather(wm_ctx *ctx, const float *cap, int C, int N, int Tq, int J, const int32_t *slot,
                              const int32_t *n_rows, float *q_sel);
/* The alignment kernels of wm_align alone (column statistics, then the cost matrix) on host data.  q f32 [B][Tq][J][64] (the
 * capture buffer: chunk b's decoder rows 0 .. S + n_text[b] + 1), keys f32 [L][B][H][1500][64] (the cross-attention keys of
 * every decoder layer, chunk and head), alignment heads (hl[j], hh[j]), j < J, in the order the mean adds them.  Row counts as
 * wm_align: n_text[b] in [0, Tq - S - 2] (0: chunk untouched), Tq <= n_text_ctx (448 without a model), n_frames[b] in
 * [2, 3000], medfilt_width odd 1 .. 31.  The keys are rounded to bf16 into a cross-K/V cache [L][2][B][H][1500][64] whose V
 * halves are NaN and whose key frames >= n_frames[b] / 2 hold 32768.  Out: x f32 [B][Tq - S - 1][1500], pre-filled with the
 * NaN bits 0x7fc0dead, of which the kernels overwrite rows [0, n_text[b] + 1) x frames [0, n_frames[b] / 2) of each chunk;
 * optional col_stats f32 [B][J][1500][2] (per frame: mean and std of the probabilities over the S + n + 2 rows). */
WM_API int wmdbg_align_matrix(wm_ctx *ctx, const float *q, const float *keys, int L, int H, int B, int Tq, int J,
                              const int32_t *hl, const int32_t *hh, int S, const int32_t *n_text, const int32_t *n_frames,
                              int medfilt_width, float qk_scale, float *x, float *col_stats);
/* wmdbg_align_matrix with the row rule of an aligned transcribe group (wm_transcribe_mel_aligned): tail_rows = decoder rows
 * behind the last cost-matrix row.  1: wmdbg_align_matrix exactly.  0: chunk b has S + n_text[b] + 1 decoder rows, its matrix
 * is the last n_text[b] + 1 of them, n_text[b] in [-1, Tq - S - 1] with -1 the untouched chunk and 0 a one-row matrix, S >= 0
 * (a chunk of ONE decoder row is invalid: no spread over the rows); x f32 [B][Tq - S][1500]. */
WM_API int wmdbg_align_matrix_rows(wm_ctx *ctx, const float *q, const float *keys, int L, int H, int B, int Tq, int J,
                                   const int32_t *hl, const int32_t *hh, int S, const int32_t *n_text, const int32_t *n_frames,
                                   int medfilt_width, float qk_scale, float *x, float *col_stats, int tail_rows);
/* The token-probability kernel of wm_align alone: prob[b] = softmax(logits[b][0 : eot])[tok[b]] for B host rows of row stride
 * ldo >= V (entries eot .. ldo - 1 are never read), 1 <= eot <= V, 0 <= tok[b] < eot. */
WM_API int wmdbg_align_token_prob(wm_ctx *ctx, const float *logits, int B, int V, int ldo, const int32_t *tok, int eot,
                                  float *prob);

/* Beam search (wm_transcribe_mel_beam).  One selection step of ONE window on host data, by the function the select kernel runs
 * (csrc/beam.h): N beams of which the first n_from contribute (1 at the first generated token), sum f32 [N] (-inf: a dead beam),
 * lists list_n i32 [N] (0 .. WM_MAX_BEAM + 1 entries, best first), list_tok i32 / list_lp f32 [N][WM_MAX_BEAM + 1]; eot < 0:
 * nothing finishes; pad: the token of a dead beam; room: finished hypotheses the window still takes.  Out: *n_next beams taken,
 * src / tok / lp / new_sum [N] (slots >= *n_next: dead -- src = slot, tok = pad, lp 0, sum -inf), *n_fin kept newly finished
 * hypotheses with fin_src / fin_lp / fin_sum [N]. */
WM_API int wmdbg_beam_select(int N, int n_from, int32_t eot, int32_t pad, int room, const float *sum, const int32_t *list_n,
                             const int32_t *list_tok, const float *list_lp, int32_t *n_next, int32_t *src, int32_t *tok,
                             float *lp, float *new_sum, int32_t *n_fin, int32_t *fin_src, float *fin_lp, float *fin_sum);
/* The MaximumLikelihoodRanker's score of one hypothesis, the function behind wm_rank_candidates and
 * wm_transcribe_mel_beam's best_out: sum / n_text (n_text 0 counts as 1) with length_penalty NaN, else
 * sum / ((5 + n_text) / 6) ** length_penalty.  Host only. */
WM_API double wmdbg_rank_score(double sum, int n_text, float length_penalty);
/* Finalize: the live beams (sum > -inf) by descending sum, ties to the lower beam, into order_out [N]; returns their count
 * (-1: bad arguments).  Host only. */
WM_API int wmdbg_beam_fill_order(int N, const float *sum, int32_t *order_out);
/* Makes the NEXT transcribe call on ctx, when it is a beam call (any other drops the hook: THE ONE-SHOTS' SCOPE above), also
 * return, per window, generated index and beam, the beam's list and
 * its running sum BEFORE that step: trace_out f32 [B][max_new][beam_size][2 + 2 * (WM_MAX_BEAM + 1)], each record = entries
 * (i32 bits), sum, WM_MAX_BEAM + 1 token ids (i32 bits), WM_MAX_BEAM + 1 log-probs; zeros where no step ran.  That call
 * launches its positions eagerly. */
WM_API int wmdbg_beam_trace(wm_ctx *ctx, float *trace_out);
/* The per-row list kernel alone.  logits f32 [rows][V] (host), N beams per window (the lists hold N + 1 entries), suppressed
 * ids, rng i32 [rows][4] = (text_lo, text_hi, ts_lo, ts_hi) or NULL (timestamp rules off) with ts_begin.  The per-tile
 * partials the decode step's logits launch would leave are restated on the host (f32, libm expf).  Out: list_n i32 [rows],
 * list_tok i32 / list_lp f32 [rows][WM_MAX_BEAM + 1]. */
WM_API int wmdbg_beam_topk(wm_ctx *ctx, const float *logits, int rows, int V, int N, const int32_t *suppress, int n_suppress,
                           const int32_t *rng, int32_t ts_begin, int32_t *list_n, int32_t *list_tok, float *list_lp);
/* The alternatives kernel (wm_request_alternatives) alone, on host-given logits rows [rows][V] at generated index 0: suppress /
 * rng [rows][4] (nullable: no timestamp rules) / ts_begin as wmdbg_beam_topk, the per-tile partials restated on the host by the
 * same helper -- for n <= WM_MAX_BEAM + 1 the lists are wmdbg_beam_topk's of N = n - 1 bit for bit.  n in [1,
 * WM_MAX_ALTERNATIVES].  In and out: tokens i32 / logprobs f32 [rows][n], counts i32 / entropy f32 [rows] (both nullable) --
 * uploaded as given and downloaded whole, so a sentinel shows what the kernel wrote. */
WM_API int wmdbg_alternatives(wm_ctx *ctx, const float *logits, int rows, int V, int n, const int32_t *suppress, int n_suppress,
                              const int32_t *rng, int32_t ts_begin, int32_t *counts, int32_t *tokens, float *logprobs,
                              float *entropy);
/* The truncation kernel of the sampling rules alone, on host-given logits rows [rows][V] at generated index gi: suppress /
 * rng [rows][4] (nullable: no timestamp rules) / ts_begin as wmdbg_beam_topk, the per-tile partials restated on the host the
 * same way.  temperature > 0, seed and sample_ids [rows] (the rows' Philox counter words) are the call's.  Out, [rows] each:
 * kept_n = |K|, cut_tok = the last kept id, tok = the drawn id (0, -1, -1 where nothing can be kept). */
WM_API int wmdbg_sample_truncate(wm_ctx *ctx, const float *logits, int rows, int V, const int32_t *suppress, int n_suppress,
                                 const int32_t *rng, int32_t ts_begin, float temperature, uint64_t seed, const uint32_t *sample_ids,
                                 int gi, int top_k, float top_p, float min_p, int32_t *kept_n, int32_t *cut_tok, int32_t *tok);
/* The re-parenting kernel alone, in place on host data: cache u16 [L2][rows][H][T][64] (bf16 bits), seq i32 [T][rows] and
 * logprob f32 [T][rows] (position-major), for the close of position pos (rows 0 .. pos of the cache, generated indices
 * 0 .. pos - n_prompt of the histories); src i32 [rows]: the beam (0 .. N - 1) of its window each row continues; wdone i32
 * [rows / N]: 1 = the window has just left the decode (its histories move, its cache does not). */
WM_API int wmdbg_beam_reorder(wm_ctx *ctx, uint16_t *cache, int L2, int rows, int H, int T, int N, int pos, int n_prompt,
                              const int32_t *src, const int32_t *wdone, int32_t *seq, float *logprob);
/* The select kernel alone (beam.hip beam_select_kernel): ONE wm_beam_select_step launch on caller-given state -- the lists are
 * the caller's, no logits and no list kernel in front of it.  A group of C windows x N beams (rows = C * N <= WM_DEC_MAXB) at
 * position pos, generated index gi = pos + 1 - n_prompt.  Every buffer is host memory that the hook uploads WHOLE before the
 * launch and downloads WHOLE behind it, whether the rules, the early stop or the ancestry are on: the caller pre-fills what it
 * does not give with a sentinel (the NaN bits WMDBG_SENTINEL_F32 for floats, a fixed negative int) and reads from the buffers
 * what was written and that nothing else was.  Per-window arrays have cap >= C entries, per-row arrays cap * N: entries behind
 * the group's must come back untouched.  The position-major arrays (seq, logprob, anc) and off have the group's row stride.
 * The embedded next row comes back with the conventions of wmdbg_step: the device buffers are pre-filled with the sentinels by
 * the hook, x_next / xb_next f32 [cap * N][d] (xb_next un-tiled and widened), stats_next [cap * N][2] summed from the d / 16
 * parts, stats_tail_nonzero the words behind part 0 of the GROUP's rows that are not zero bits, mean_next [cap * N].
 * Nothing is launched when the kernel could leave a buffer -- WM_ERR_INVALID with a message: C < 1, N outside 1 ..
 * WM_MAX_BEAM, cap < C, rows > WM_DEC_MAXB; pos outside [n_prompt - 1, n_ctx); gi >= max_new; max_cand outside 1 ..
 * WM_MAX_BEAM_HYPS; fin_n[w] outside 0 .. max_cand; a list_n outside 0 .. N + 1; a listed token, pad or eot outside the
 * vocabulary; a negative off; d that the tiled layout does not take (a multiple of 64, 64 .. 1280). */
typedef struct wmdbg_beam_io {
    int32_t C, N, cap;
    int32_t n_ctx, pos, n_prompt, d, n_vocab;
    int32_t max_cand, max_new, eot, pad;   /* WmBeamPar */
    int32_t ts_on;                         /* timestamp rules: 0 = the kernel gets no hist / rng */
    int32_t ts_par[4];                     /* ts_begin, eot, n_vocab, max_initial of WmTsDev */
    int32_t stop_on;                       /* early stop: 0 = the kernel gets no done / live_rows / n_live */
    const int32_t *budget;     /* [cap] */
    float *sum;                /* [cap * N] in / out */
    int32_t *list_n;           /* [cap * N] */
    int32_t *list_tok;         /* [cap * N][WM_MAX_BEAM + 1] */
    float *list_lp;            /* [cap * N][WM_MAX_BEAM + 1] */
    int32_t *src;              /* [cap * N] */
    int32_t *wdone, *wsteps, *fin_n;       /* [cap] */
    int32_t *fin_len;          /* [cap][WM_MAX_BEAM_HYPS] */
    float *fin_sum;            /* [cap][WM_MAX_BEAM_HYPS] */
    int32_t *fin_src;          /* [cap][WM_MAX_BEAM_HYPS]; handed to the kernel with anc only, as the product does */
    int32_t *fin_tok;          /* [cap][WM_MAX_BEAM_HYPS][n_ctx] */
    float *fin_lp;             /* [cap][WM_MAX_BEAM_HYPS][n_ctx] */
    int32_t *anc;              /* [max_new][rows], or NULL: a group that is not aligned (no anc, no fin_src) */
    int32_t *seq;              /* [n_ctx + 1][rows], as the model's buffer: the close of position n_ctx - 1 writes row n_ctx */
    float *logprob;            /* [max_new][rows] */
    int32_t *hist, *rng;       /* [cap * N][4] */
    int32_t *done, *live_rows; /* [cap * N] */
    int32_t *n_live;           /* [1] */
    const int32_t *off;        /* [rows] or NULL: a ragged group's prompt starts */
    const float *emb;          /* [n_vocab][d], rounded to bf16 and tiled by the hook */
    const float *pemb;         /* [n_ctx][d] */
    float *x_next, *xb_next;   /* [cap * N][d] */
    float *stats_next;         /* [cap * N][2] */
    float *mean_next;          /* [cap * N] */
    int32_t stats_tail_nonzero;
    int32_t pos_out;
} wmdbg_beam_io;
WM_API int wmdbg_beam_step(wm_ctx *ctx, wmdbg_beam_io *io);
/* For callers that restate the struct (ctypes): out4 = sizeof(wmdbg_beam_io) and the offsets of ts_par, budget and x_next (host only). */
WM_API int wmdbg_beam_step_layout(int32_t *out4);
/* The window-set copy kernel alone (xkv_rows.hip), on DEVICE buffers of the caller (16-byte aligned, bf16 bits): group u16
 * [2 * L][group_rows][H][1500][64], a decode group's cross-K/V cache, and store u16 [store_rows][2 * L][H][1500][64], a set's
 * window-major store.  Group row b <-> store row rows[b] (i32 [n_rows], host; every entry in [0, store_rows)), b < n_rows <=
 * group_rows <= 128.  to_store != 0: group -> store (the rows must differ), else store -> group.  Synchronous. */
WM_API int wmdbg_xkv_rows(wm_ctx *ctx, uint16_t *group, int group_rows, uint16_t *store, int64_t store_rows, const int32_t *rows,
                          int n_rows, int L, int H, int to_store);
/* ---- live streams (wm_streams) ---- */
/* An EMPTY stream s (N = 0: new or reset) believes that n_samples >= 0 of silence came before: N = n_samples, its carry is
 * zeros, and no index is reflected because the stream is past its start.  No frame is computed: A reads as F and K as F until
 * the next push, which computes the frames from F on.  Tests 64-bit stream time without pushing 2^33 samples. */
WM_API int wmdbg_streams_set_position(wm_ctx *ctx, wm_streams *set, int s, int64_t n_samples);
/* The smallest capacity_frames wm_streams_create accepts (the product: 3003), 64 .. 3003, so that the ring wrap can be tested on
 * small rings; 0 restores the product's.  Process-wide.  Returns the value in force. */
WM_API int wmdbg_streams_min_capacity(int capacity_frames);

#ifdef __cplusplus
}
#endif
#endif
