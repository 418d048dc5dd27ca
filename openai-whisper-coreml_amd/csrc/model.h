// model.h -- Whisper encoder/decoder state (weights, activations, KV caches) and the
// launch wrappers of the HIP kernels that implement boundary #2
// (Whisper/Whisper/Whisper.swift:17-40; graph contract whisper_to_cml.py:10-43; arithmetic
// = openai-whisper AudioEncoder / TextDecoder).
#pragma once
#include "wm_internal.h"
#include "dec_launch.h"   // DecEpi, WM_DEC_MAXB, the launch plans
#include "tx_pending.h"   // WmPending, WmDebugShots

// ---------------------------------------------------------------- HBM layout ----------
// All matrix weights are bf16 [N][K] row-major (PyTorch Linear layout: K contiguous), so
// both MFMA operands are K-contiguous.  Vectors (biases, LayerNorm, positions) are f32.
struct EncLayerW {
    float *ln1_g, *ln1_b;
    bf16_t *wqkv;  // [3d][d]  rows: query | key | value
    float *bqkv;   // [3d]     (key bias = 0: openai-whisper's key Linear has no bias)
    bf16_t *wo;    // [d][d]
    float *bo;
    float *ln2_g, *ln2_b;
    bf16_t *w1;  // [4d][d]
    float *b1;
    bf16_t *w2;  // [d][4d]
    float *b2;
};
struct DecLayerW {
    float *ln1_g, *ln1_b;
    bf16_t *wqkv;  // [3d][d]
    float *bqkv;
    bf16_t *wo;
    float *bo;
    float *lnx_g, *lnx_b;  // cross_attn_ln
    bf16_t *wxq;           // [d][d]
    float *bxq;
    bf16_t *wxkv;  // [2d][d]  rows: key | value   (applied to the encoder output)
    float *bxkv;   // [2d]     (key half = 0)
    bf16_t *wxo;
    float *bxo;
    float *ln2_g, *ln2_b;
    bf16_t *w1;
    float *b1;
    bf16_t *w2;
    float *b2;
    // LayerNorm-folded copies built by wm_finalize (decode GEMV operands): W' = bf16(W g), c1[n] = sum_k W'[n][k],
    // c2[n] = bias[n] + sum_k beta[k] W[n][k] -- so that LN(x) W^T + b = rstd (x W'^T - mean c1) + c2
    bf16_t *wqkv_f, *wxq_f, *w1_f;
    float *qkv_c1, *qkv_c2, *xq_c1, *xq_c2, *fc1_c1, *fc1_c2;
};

// One registry entry per openai-whisper state-dict key: where its elements live in HBM.
// WL_CONV : [O][C][3] -> [O][Kpad], k = tap*C + c (conv taps made contiguous for the implicit GEMM)
// WL_TILED: [N][K] -> MFMA-fragment-major tiles for the decode GEMV: tile (n/16, k/32) is the
//           1 KiB a wave loads with ONE global_load_dwordx4 (lane = n%16 + 16*((k%32)/8), 8 k
//           per lane), tiles ordered n-tile major, k-step minor -- a wave streams contiguous KiBs.
enum WmLayout { WL_PLAIN = 0, WL_CONV = 1, WL_TILED = 2 };
__host__ __device__ static inline size_t wm_tiled_offset(size_t n, size_t k, size_t K) {
    return (((n >> 4) * (K >> 5) + (k >> 5)) * 64 + (n & 15) + 16 * ((k & 31) >> 3)) * 8 + (k & 7);
}
struct WmTensor {
    std::string name;
    void *ptr = nullptr;  // destination of logical element 0
    bool is_bf16 = false;
    size_t n_elems = 0;
    int layout = WL_PLAIN;
    int conv_c = 0, conv_kpad = 0;
    int kind = 0;  // K_MATRIX..K_SINUSOID of weights.py (synthetic generator)
    bool set = false;
};

// openai-whisper's ApplyTimestampRules (whisper/decoding.py [3p]) evaluated inside the fused logits / arg-max kernels.
// Per sequence the rules reduce to an allowed TEXT range and an allowed TIMESTAMP range of token ids for the next
// position (rng), maintained by the arg-max kernel from a 4-int history (hist), plus one comparison: if the summed
// probability of the allowed timestamps exceeds the best allowed text token, a timestamp is forced -- the logits kernel
// therefore emits, per 16-column tile, the best text key, the best timestamp key and a (max, sum exp) partial of the
// timestamp columns.
struct WmTsDev {
    int *rng;                     // [B][4] text_lo, text_hi, ts_lo, ts_hi for the next position; null = rules off
    int *hist;                    // [B][4] n_sampled, last_is_ts, prev_is_ts, last_ts
    unsigned long long *key_ts;   // [B][n_tiles] best allowed timestamp per tile (tiles >= ts_begin / 16 only)
    float *lse;                   // [B][n_tiles][2] (max, sum exp(v - max)) over the allowed timestamps of the tile
    int ts_begin, eot, n_vocab, max_initial;  // max_initial: index of the largest first timestamp, < 0 = unlimited
};

// wm_transcribe's extended decode (DE_LOGITS_X + the arg-max kernel's X mode): per-token log-probabilities of the filtered
// distribution, openai-whisper's no_speech_prob and Gumbel-max sampling at temperature T > 0.  Everything that changes from
// call to call lives in device memory (WmXPar, written at prefill), so the captured position graphs stay valid.
struct WmXPar {
    unsigned key0, key1;  // the sampling seed (Philox key: low, high word)
    float inv_T;          // (float)(1 / T); sampling on when > 0
    int sample;           // 0: arg-max, 1: Gumbel-max
    int sot_pos;          // decode position of <|startoftranscript|> (no_speech_prob); -1: not computed
    int ns_tok;           // <|nospeech|> id (with sot_pos >= 0)
    int chunk0;           // index within the call of the group's row 0 (Philox counter: call index, not group row)
    int n_prompt;         // generated index gi = pos + 1 - n_prompt
    int ids_on;           // 1: row b's counter word is WmXDev::ids[b] (caller-given sample ids), not chunk0 + b
    int n_cand;           // > 1: a candidate group -- row b's FOURTH counter word is WmXDev::ids[WM_XIDS_CAND + b] (else 0)
    // 1: temperature and seed are per row (wm_set_sampling_rows): inv_T, key0 and key1 above are not read,
    // row b's are wm_x_rows(WmXDev::ids)[b]; `sample` then says "some row of the call samples"
    int rows_on;
};
// a row's own sampling parameters (WmXPar::rows_on): one 16-byte load.  inv_T == 0 (all bits): an arg-max row, its key is not read
struct WmXRow {
    float inv_T;          // (float)(1.0 / (double)T), computed on the host
    unsigned key0, key1;  // the row's seed (Philox key: low, high word)
    unsigned pad;
};
// ... which live BEHIND the two halves of WmXDev::ids, so that WmXDev -- a member of every decode GEMV's argument struct -- keeps its
// size and the kernels that never read the table keep their text: [WM_XIDS_CAND] rows, padded like the ids
constexpr int WM_XIDS_ROWS = 2 * (128 + 16);   // in words of WmXDev::ids (a multiple of 4: the rows are 16-byte aligned)
constexpr int WM_XIDS_WORDS = WM_XIDS_ROWS + 4 * (128 + 16);   // the whole buffer
__host__ __device__ inline const WmXRow *wm_x_rows(const unsigned *ids) { return (const WmXRow *)(ids + WM_XIDS_ROWS); }
constexpr int WM_XIDS_CAND = 128 + 16;   // WmXDev::ids: [WM_DEC_MAXB + 16] sample ids | [WM_DEC_MAXB + 16] candidate words

// wm_transcribe_mel: row b's encoder input = frames seek .. seek + n - 1 of the [n_mels][T] block at mel + base, zeros after
struct WmMelWin {
    long long base;
    int T, seek, n, pad;
};
struct WmXDev {
    const WmXPar *par;    // null: X mode off
    const unsigned *ids;  // [>= WM_DEC_MAXB] per-row Philox counter words, read when par->ids_on (wm_transcribe_mel sample_ids)
                          // (with par->rows_on: WM_XIDS_WORDS words, the rows' WmXRow table at WM_XIDS_ROWS -- wm_x_rows)
    float *txt;           // [B][n_tiles][2] (max, sum exp) over the tile's allowed TEXT ids (raw logits)
    float *win;           // [B][n_tiles][2] raw logit of the tile's winner: text, timestamp
    float *all;           // [B][n_tiles][2] (max, sum exp) over every id -- at pos == sot_pos only
    float *ns_v;          // [B] raw logit of <|nospeech|> at pos == sot_pos
    float *logprob;       // [n_ctx][B] log-prob of generated token gi of row b at [gi * B + b]
    float *nospeech;      // [B]
};

// The repetition rules (wm_set_repetition_rules; repeat.hip): two logit processors over a row's own
// GENERATED history g[0 .. k) = positions n_prompt .. pos of the token buffer (the prompt is excluded).  Only ids < eot are
// ever penalised or banned.  Penalty p: every id that occurs in g, once, v = v > 0 ? v * inv_p : v * p.  No-repeat n-gram n:
// id t is banned iff some i in [0, k - n] has g[i .. i + n - 1) == g[k - n + 1 .. k) and g[i + n - 1] == t.  wm_repeat_state
// REBUILDS both bitmaps from the history in front of every logits launch; the DE_LOGITS_XR epilogue applies them before
// anything else looks at the logit.  What changes from call to call lives in device memory (WmRepPar, written at prefill).
struct WmRepPar {
    float p, inv_p;   // inv_p = (float)(1.0 / (double)p), computed on the host: the penalty is ONE f32 multiply either way
    int n, eot;
};
struct WmRepDev {
    const WmRepPar *par;   // null: the rules are off
    unsigned *seen;        // [rows][words] ids < eot that occur in the row's history
    unsigned *ban;         // [rows][words] ids < eot that would complete a repeated n-gram
    int words;             // (vpad + 31) / 32
};
constexpr int WM_MAX_NGRAM = 32;

// The sampling rules (wm_set_sampling_rules; sample_trunc.hip): top-k, top-p and min-p truncation of a
// sampling row's filtered distribution, applied by one launch between the logits product and the close.  What changes from call
// to call lives in device memory (WmSampPar, written at prefill); (0, 1, 0) is off.
struct WmSampPar {
    int top_k;
    float top_p, min_p;
};

// Given tokens (wm_set_given_tokens; given.hip): one launch per position, last in front of the close, hands
// the close the caller's token for the rows of the table.  The table lives in device memory (written at prefill), so a captured
// position replays for any table.
struct WmGivenPar {
    int stride;       // tokens per row of the table (>= 1)
    const int *lens;  // [rows] given tokens of each row, 0 .. stride (0: the row decodes freely)
    const int *tok;   // [rows][stride]
};

// Top-n alternatives and entropy (wm_request_alternatives; alternatives.hip): one launch per position
// between the logits product and the close lists a row's n best admissible ids with their log-probs and sums its entropy.  n
// and the buffers live in device memory (WmAltPar, written at prefill), so a captured position replays for any request.
struct WmAltPar {
    int n, max_new;   // entries per position; positions the buffers hold
    int *tok;         // [max_new][rows][n] ids, -1 past the count
    float *lp;        // [max_new][rows][n] log-probs, 0 past the count
    int *cnt;         // [max_new][rows]
    float *ent;       // [max_new][rows]
};

// The sequence bias (wm_set_sequence_bias; seqbias.hip): a table of token sequences with a bias each.
// Entry s[0 .. n) matches a row iff n == 1 or the row's generated history g[0 .. k) ends in s[0 .. n - 1); total(t) is the f32
// sum, from +0.0f in table order, of the biases of the matching entries whose last token is t, and the logit becomes
// v[t] + total(t) behind the repetition penalty.  A total of -inf is a ban (OR-ed into WmRepDev::ban).  The table is expanded
// (boosted prefixes), sorted stably by last token and uploaded at set time: entries with the same last token form a GROUP,
// groups ascend by id.  wm_seqbias_state REBUILDS the per-row state from the history in front of every logits launch, behind
// wm_repeat_state; the DE_LOGITS_XB epilogue adds the totals.  What changes from call to call lives in device memory.
struct WmSbPar {
    int n_groups, n_entries;
};
// what the epilogue reads (the LAST member of the GEMV's kernel-argument struct)
struct WmSbEpi {
    unsigned *hit;   // [rows][words] ids with a matching entry at this position (bans included: their total is -inf)
    int *cnt;        // [rows] list length
    int *lid;        // [rows][WM_MAX_BIAS_ENTRIES] the ids of the hit bits, ascending
    float *ltot;     // [rows][WM_MAX_BIAS_ENTRIES] their totals
    int *woff;       // [rows][words] hit bits in the words below: total(t) = ltot[woff[t >> 5] + popcount(hit bits of the word below t)]
    int words;       // (vpad + 31) / 32
};
struct WmSbDev {
    const WmSbPar *par;      // null: the bias is off
    const int *grp_id;       // [WM_MAX_BIAS_ENTRIES] last token of group g, ascending
    const int *grp_beg;      // [WM_MAX_BIAS_ENTRIES + 1] group g = entries [grp_beg[g], grp_beg[g + 1])
    const int *ent_len;      // [WM_MAX_BIAS_ENTRIES] context length n - 1 of entry e (0 .. 31)
    const float *ent_bias;   // [WM_MAX_BIAS_ENTRIES]
    const int *ent_ctx;      // [WM_MAX_BIAS_ENTRIES][WM_SB_CTX] context of entry e, NEWEST token first: s[n - 2], s[n - 3], ...
    WmSbEpi e;
};
constexpr int WM_SB_CTX = WM_MAX_BIAS_SEQ_LEN - 1;
// The expanded table on the host (wm_sb_expand: validation, prefix expansion, merge, stable sort by last token).
struct WmSbTable {
    std::vector<int32_t> grp_id, grp_beg, ent_len, ent_ctx;   // ent_ctx: [n_entries][WM_SB_CTX], newest first, padded with 0
    std::vector<float> ent_bias;
    int n_groups() const { return (int)grp_id.size(); }
    int n_entries() const { return (int)ent_len.size(); }
};
// WM_OK, or WM_ERR_INVALID with the message set; n_seq = 0 gives the empty table.  Pure host code (model_api.cpp).
int wm_sb_expand(const int32_t *tokens, const int32_t *seq_offsets, const float *bias, const uint8_t *boost_prefixes, int n_seq,
                 int32_t eot, int n_vocab, WmSbTable *out);
// Row tables (wm_set_sequence_bias_tables): the expanded tables of a context CONCATENATED in the layout of WmSbDev -- the POOL.
// grp_beg is absolute into the pool's entries (one array of n_groups + 1: a table's last boundary is the next one's first);
// table t is groups [tab_grp[t], tab_grp[t + 1]), each table at most WM_MAX_BIAS_ENTRIES entries, the pool at most
// WM_MAX_BIAS_POOL.  A row of a decode group walks its own table's group range (WmModel::dsb_rng, wm_seqbias_rows_state).
struct WmSbPool {
    WmSbTable t;                    // the pooled arrays (grp_beg: [n_groups + 1], {0} when the pool has no entry)
    std::vector<int32_t> tab_grp;   // [n_tables + 1] (empty: no tables)
    int n_tables() const { return tab_grp.empty() ? 0 : (int)tab_grp.size() - 1; }
};
// wm_sb_expand per table (sequences [table_offsets[t], table_offsets[t + 1])) and the concatenation.  Pure host code.
int wm_sb_expand_tables(const int32_t *tokens, const int32_t *seq_offsets, const float *bias, const uint8_t *boost_prefixes,
                        const int32_t *table_offsets, int n_tables, int n_seq, int32_t eot, int n_vocab, WmSbPool *out);

// The constraint (wm_set_constraint; constraint.hip): an automaton over token ids that says which text ids
// and whether `eot` a row may generate next.  State s allows text id t < eot iff an explicit edge (s, t) has a target >= 0, or no
// explicit edge exists and def_next[s] >= 0; it allows eot iff accept[s].  Ids above eot are never banned and do not move the
// state, nor does eot in the history (the padding of a finished row); a forbidden text id in the history leads to the dead state
// -1, which allows eot alone.  wm_constraint_state REBUILDS a row's state from its generated history g[0 .. k) in front of every
// logits launch, behind wm_repeat_state (and wm_seqbias_state), and ORs the ids of [0, eot] the state does not allow into the ban
// words wm_repeat_state has just rebuilt: everything that tests a ban bit treats them as suppressed.  The walk looks an edge up
// in an open-addressing hash of (state, token) built on the host: one 8-byte load per probe, the table at most half full.
struct WmCstPar {
    int n_states, n_edges, eot;
};
constexpr int WM_CST_TOK_BITS = 20;                          // key = state << 20 | token: eot <= 2^20, states <= 2^12
constexpr int WM_CST_HASH_BITS = 17;                         // 2 * WM_MAX_CST_EDGES slots
constexpr int WM_CST_HASH_SLOTS = 1 << WM_CST_HASH_BITS;
static_assert(WM_CST_HASH_SLOTS >= 2 * WM_MAX_CST_EDGES && WM_MAX_CST_STATES <= (1 << (32 - WM_CST_TOK_BITS)), "constraint hash geometry");
__host__ __device__ inline unsigned wm_cst_key(int state, int tok) { return (unsigned)state << WM_CST_TOK_BITS | (unsigned)tok; }
__host__ __device__ inline unsigned wm_cst_slot(unsigned key) { return (key * 0x9E3779B1u) >> (32 - WM_CST_HASH_BITS); }
struct WmCstDev {
    const WmCstPar *par;    // null: the constraint is off
    const int *edge_beg;    // [WM_MAX_CST_STATES + 1] state s = edges [edge_beg[s], edge_beg[s + 1])
    const int *edge_tok;    // [WM_MAX_CST_EDGES] ascending within a state
    const int *edge_next;   // [WM_MAX_CST_EDGES] target state, or -1: forbidden
    const int *def_next;    // [WM_MAX_CST_STATES] target of a text id without an explicit edge, or -1
    const int *accept;      // [WM_MAX_CST_STATES] 0 / 1
    const int *hash;        // [WM_CST_HASH_SLOTS][2] (key, target); key -1: empty.  Linear probing from wm_cst_slot(key)
    const int *start;       // [rows] start state of each row; -1: the row is unconstrained
};
// The checked automaton on the host with its hash (wm_cst_build: validation and packing).  n_states == 0: off.
struct WmCstTable {
    std::vector<int32_t> edge_beg, edge_tok, edge_next, def_next, accept, hash;
    int32_t eot = 0;
    int n_states() const { return (int)def_next.size(); }
    int n_edges() const { return (int)edge_tok.size(); }
};
// WM_OK, or WM_ERR_INVALID with the message set; n_states = 0 gives the empty table.  Pure host code (constraint_table.cpp).
int wm_cst_build(const int32_t *edge_beg, const int32_t *edge_tok, const int32_t *edge_next, const int32_t *def_next,
                 const uint8_t *accept, int n_states, int32_t eot, int n_vocab, WmCstTable *out);

// Early-stop state of a decode group (device view; done == null: off).  A row is DONE once it has emitted `eot`
// (eot >= 0) or produced budget[b] tokens (budget != null); from then on its tokens are `pad_tok`, it is dropped from
// the compact live list the attention kernels walk, and when the list is empty the host stops launching positions.
struct WmStopDev {
    int *done;          // [B] 0 / 1
    const int *budget;  // [B] tokens a row may generate (null: max_new for all)
    int *live_rows;     // [B] compact, ascending list of the rows that are not done
    int *n_live;        // [1]
    int eot, pad_tok;
};

// Where an embedding goes: the tables and the residual-stream target of the launches that embed a position (wm_dec_embed,
// wm_dec_embed_panel, and the closes wm_argmax_embed and wm_beam_select_step).  x == null (WmEmbedDev{}): a close embeds nothing.
struct WmEmbedDev {
    const bf16_t *emb;   // token embedding [n_vocab][d] bf16, WL_TILED
    const float *pemb;   // positional embedding [n_ctx][d]
    int d;
    float *x;            // [rows][d] f32 residual stream
    bf16_t *xb;          // its mean-centred bf16 copy, WL_TILED
    float *stats_out;    // LayerNorm partial statistics the next layer-0 GEMV expects (nullable)
    float *mean_buf;     // [rows] row means (nullable)
};

// Beam search (wm_transcribe_mel_beam, beam.hip).  A beam group is a candidate group (rows = windows x N, row c * N + k is beam
// k of window c) whose rows are re-parented after every generated token.  What changes from call to call lives in device
// memory (WmBeamPar, the budgets), so the captured positions replay; N and n_prompt are part of the graph key.
struct WmBeamPar {
    int max_cand;   // finished hypotheses after which a window leaves the decode
    int max_new;
    int eot;        // < 0: nothing finishes
    int pad;        // what a dead beam and a window that has left keep emitting: eot, or 0
};
constexpr int WM_BEAM_TRACE = 2 + 2 * (WM_MAX_BEAM + 1);   // debug trace words per (generated index, row): n, sum, tokens, log-probs
struct WmBeamDev {
    const WmBeamPar *par;
    int N, n_ctx;
    const int *budget;   // [windows] tokens a window may generate (<= max_new)
    float *sum;          // [rows] running f32 sum of the beam (-inf: dead)
    int *src;            // [rows] the beam (0 .. N - 1) of its window a row continued at the last close
    int *list_n;         // [rows] entries of the row's list
    int *list_tok;       // [rows][WM_MAX_BEAM + 1]
    float *list_lp;      // [rows][WM_MAX_BEAM + 1]
    int *wdone;          // [windows] 1: the window has left the decode
    int *wsteps;         // [windows] tokens it has generated
    int *fin_n;          // [windows] finished hypotheses
    int *fin_len;        // [windows][WM_MAX_BEAM_HYPS] tokens incl. eot
    float *fin_sum;      // [windows][WM_MAX_BEAM_HYPS]
    int *fin_tok;        // [windows][WM_MAX_BEAM_HYPS][n_ctx]
    float *fin_lp;       // [windows][WM_MAX_BEAM_HYPS][n_ctx]
    float *trace;        // debug library only (else null): [max_new][rows][WM_BEAM_TRACE], the lists and sums BEFORE each step
    // an aligned beam group only (else null): the search's ancestry, which wm_beam_ancestry walks (beam.h)
    int *anc;            // [max_new][rows] the source beam of every row at every close
    int *fin_src;        // [windows][WM_MAX_BEAM_HYPS] the source beam of each finished hypothesis
};

// Word-level timestamps (wm_align, align.hip).  The alignment heads of one decoder layer: n heads (ascending) whose
// captured queries go to slots slot0 .. slot0 + n - 1 of the capture buffer.
struct WmAlignLayer {
    int n = 0, slot0 = 0;
    int head[32] = {};
};
// what the teacher-forced pass of wm_align captures: the layers' alignment-head queries, [B][Tq][J][64] f32
struct WmAlignCap {
    const WmAlignLayer *layer;  // [n_text_layer] (host)
    float *q;
    int Tq, J;
    // >= 0 (an aligned transcribe group): the query of absolute position pos goes to capture row pos - base, positions in front
    // of base and rows at or past Tq are not captured; -1: capture row = position (the teacher-forced passes)
    int base = -1;
};
// the alignment kernels' view of one decode group (device pointers)
struct WmAlignDev {
    const float *q;          // [B][Tq][J][64] captured cross-attention queries (f32)
    const bf16_t *xkv;       // the group's cross-attention K/V cache [L][2][B][H][1500][64]
    const int *hl, *hh;      // [J] alignment heads (layer, head), ascending
    const int *n_text;       // [B] text tokens n of each chunk: decoder rows S + n + 1 + tail, cost-matrix rows n + 1; below n_min = none
    const int *n_frames;     // [B] mel frames; the alignment uses audio frames [0, n_frames / 2)
    float *rowst;            // [B][J][Tq][2] per decoder row: softmax max and 1 / sum (scores in log2 units)
    float *colst;            // [B][J][1500][2] per frame: mean and std of the probabilities over the chunk's rows
    float *x;                // [B][n_ld][1500] cost matrix -mean over heads of the filtered z-scores
    int B, H, Tq, J, S, n_ld;
    float sc;                // 0.125 * qk_scale * log2(e)
    int half;                // medfilt_width / 2
    // The row rule.  tail: decoder rows behind the last cost-matrix row -- 1 for wm_align (the row of the teacher-forced eot),
    // 0 for an aligned transcribe group (a decode never feeds its last token).  n_min: the smallest n_text that is a chunk at
    // all -- 1 for wm_align (n = 0: no text), 0 for an aligned group (n = len - 1: a one-token row is a one-row matrix; absent
    // rows carry -1).
    int tail = 1, n_min = 1;
};

// The mode of ONE decode: everything a captured position bakes into its kernel arguments that the context's weights and
// shapes do not fix.  A default-constructed value is the plain teacher-forced step (wm_decode_logits, language
// identification, wm_align); a transcribe call fills its groups' mode once (transcribe.cpp lane_prefill) and every step,
// eager or captured, is handed that value -- it is also, member by member, the key of the captured graphs (GraphSet).
struct WmDecodeMode {
    bool mask = false;      // the suppress bitmaps apply (wm_set_suppress), the first-token one at position n_prompt - 1
    bool ts = false;        // the timestamp rules apply (wm_set_timestamp_rules, WmTsDev)
    bool x = false;         // extended decode: the X-mode kernels and their WmXDev state
    bool off = false;       // a ragged group: the row offsets WmModel::doff
    bool stop = false;      // early stop: the WmStopDev state ...
    bool budget = false;    // ... with per-row token budgets
    int stop_eot = -1;      // ... and this end-of-text id (< 0: budgets only)
    // The group SHARES the chip with other groups (other lanes of the call, other contexts' calls): its cross-attention
    // is launched as one short-lived workgroup per (sequence, head) pair instead of <= 256 persistent ones.  Alone, the
    // persistent shape streams faster (56 rows: 66.8 vs 70.5 us); next to other groups' kernels the short-lived one lets
    // their workgroups in every ~13 us instead of once per launch: driver command 2076 -> 2100-2134 audio-s/s, default
    // run 2190 -> 2250 (profiles/r04_xattn_short_lived.txt).  A launch shape: same bits.
    bool xattn_shared = false;
    // Candidates per window (wm_transcribe_mel_best_of; 1: none): the group's rows are windows x n_cand, row c * n_cand + s is
    // candidate s of window c, the cross-attention K/V cache holds one entry per WINDOW and is read by
    // wm_dec_attention_cand, once for all live candidates of a window.
    int n_cand = 1;
    // Beam width (wm_transcribe_mel_beam; 0: no beam search): the generating positions close with the beam kernels
    // (wm_model_beam_close) instead of the arg-max; above 1 the rows are a candidate group (n_cand = beam).
    int beam = 0;
    bool rep = false;       // the repetition rules apply (wm_set_repetition_rules, WmRepDev): wm_repeat_state + DE_LOGITS_XR; needs x
    // The sequence bias applies (wm_set_sequence_bias, WmSbDev): wm_seqbias_state behind wm_repeat_state + DE_LOGITS_XB.  A group
    // with sb has rep too -- the bitmaps are wm_repeat_state's, rebuilt with the rules (1.0, 0) when the repetition rules are off.
    bool sb = false;
    // Row tables (wm_set_sequence_bias_tables): the state kernel is wm_seqbias_rows_state over the pool and the group's per-row
    // group ranges instead of wm_seqbias_state over the one table.  Implies sb and rep; the epilogue is the same DE_LOGITS_XB.
    bool sbt = false;
    // The constraint applies (wm_set_constraint, WmCstDev): wm_constraint_state behind wm_repeat_state (and the sequence-bias
    // launch) ORs the ids the rows' automaton states do not allow into the ban words.  Implies rep and x -- the bitmaps are
    // wm_repeat_state's, rebuilt with the rules (1.0, 0) when the repetition rules are off; the epilogue is whatever rep / sb choose.
    bool cst = false;
    // The sampling rules apply (wm_set_sampling_rules on a call with temperature > 0): the logits launch stores the f32 row and
    // wm_sample_truncate runs between it and the close.  Needs x.
    bool trunc = false;
    // A request for alternatives is served (wm_request_alternatives): the logits launch stores the f32 row and wm_alternatives
    // runs between it and the close (in front of wm_sample_truncate).  Needs x.
    bool alt = false;
    // The group holds a row with given tokens (wm_set_given_tokens): the logits launch stores the f32 row and wm_given_tokens runs
    // last in front of the close.  Needs x.  A group of ordinary rows inside a call with a table does not set it.
    bool given = false;
    // Temperature and seed are per row (wm_set_sampling_rows): the X-mode kernels read the rows' table behind WmModel::dx_ids.
    // Needs x.  The table's contents are uploaded at prefill; the key holds the flag, so a group with a table and one without
    // never share a captured graph.
    bool srows = false;
    // Panel width of a teacher-forced pass (wm_set_teacher_panel; 1: none): the step's rows are windows x panel, row c * panel + s
    // is position *dpos + s of window c -- the self-attention cache holds one entry per WINDOW, row (c, s) appends at and reads up
    // to its own position, the cross-attention is the candidate-group launch (wm_model_panel_step).  The teacher-forced entries
    // run eagerly, but a mode is a graph key member by member, so it is compared like the others.
    int panel = 1;
    // An aligned transcribe group (wm_transcribe_mel_aligned): every step captures the alignment heads' queries, so the layers
    // with alignment heads take the unfused cross_attn_ln + query launches (same bits).  What the capture launch bakes in --
    // the buffer, its row count, the head count, the position of capture row 0 -- is part of the key; the head list itself is
    // not: wm_set_alignment_heads drops the captured graphs.
    bool acap = false;
    int acap_base = 0, acap_Tq = 0, acap_J = 0;
    float *acap_q = nullptr;
    bool operator==(const WmDecodeMode &o) const {
        return acap == o.acap && acap_base == o.acap_base && acap_Tq == o.acap_Tq && acap_J == o.acap_J && acap_q == o.acap_q && panel == o.panel && trunc == o.trunc && alt == o.alt && given == o.given && srows == o.srows && rep == o.rep && sb == o.sb && sbt == o.sbt && cst == o.cst && n_cand == o.n_cand && beam == o.beam && mask == o.mask && ts == o.ts && x == o.x && off == o.off && stop == o.stop && budget == o.budget &&
               stop_eot == o.stop_eot && xattn_shared == o.xattn_shared;
    }
};

// A grow-only device buffer: reserve() keeps what it has when that is enough, otherwise waits for the stream, frees and
// reallocates (contents are not kept); a failed allocation leaves {nullptr, 0}.
struct WmDevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int reserve(hipStream_t stream, size_t need);   // model.cpp
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
    }
};

// A captured graph and its executable instance.  Not a destructor-owning type: GraphSet lives in a std::vector that is
// erased from and pushed to, so the owner calls destroy() (wm_model_drop_graphs, the LRU eviction).
struct WmGraph {
    hipGraph_t g = nullptr;
    hipGraphExec_t e = nullptr;
    void destroy() {
        if (e) (void)hipGraphExecDestroy(e);
        if (g) (void)hipGraphDestroy(g);
        e = nullptr; g = nullptr;
    }
};

struct WmModel {
    wm_dims dims;
    bool finalized = false;
    bool shares_weights = false;  // clone: weight pointers alias the parent context's (never freed here)
    int k1pad = 0;  // conv1 GEMM K (3*n_mels rounded up to 64)
    int vpad = 0;   // n_vocab rounded up to 16 (token embedding rows)
    // weights
    bf16_t *conv1_w = nullptr, *conv2_w = nullptr;
    float *conv1_b = nullptr, *conv2_b = nullptr, *enc_pos = nullptr;
    std::vector<EncLayerW> enc;
    float *ln_post_g = nullptr, *ln_post_b = nullptr;
    bf16_t *tok_emb = nullptr;  // [vpad][d]
    float *dec_pos = nullptr;   // [n_text_ctx][d]
    std::vector<DecLayerW> dec;
    float *ln_g = nullptr, *ln_b = nullptr;
    bf16_t *emb_f = nullptr;    // [vpad][d] token embedding with the final LayerNorm's gamma folded in (logits GEMV)
    float *logit_c1 = nullptr, *logit_c2 = nullptr;  // [vpad]
    std::vector<void *> allocs;
    std::vector<WmTensor> tensors;
    std::map<std::string, int> index;
    // activations (sized for `cap_b` chunks)
    int cap_b = 0;
    int cap_rows = 0;         // decoder rows skv holds: min(cap_b, WM_DEC_MAXB), or more for a candidate group (wm_model_reserve_rows)
    bf16_t *mel_t = nullptr;  // [B][3002][n_mels]  time-major, zero rows 0 and 3001
    bf16_t *h1p = nullptr;    // [B][3001][d]       conv1 output, zero row 0
    float *x = nullptr;       // [B*1500][d]        encoder residual stream (f32)
    bf16_t *xn = nullptr;     // [B*1500][d]        LayerNorm output / encoder output (bf16)
    bf16_t *qk = nullptr;     // [B*1500 + 64][2d]  q | k
    bf16_t *vt = nullptr;     // [B][H][64][1536]   v transposed (s contiguous)
    bf16_t *att = nullptr;    // [B*1500][d]
    bf16_t *hid = nullptr;    // [B*1500][4d]
    float *xa_f32 = nullptr;  // [B*1500][d]        ln_post output (API output)
    float *mel_f32 = nullptr; // [B][n_mels][3000]  front-end output kept on device
    bf16_t *xkv = nullptr;    // [L][2][B][H][1500][64]  cross-attention K/V cache
    bf16_t *skv = nullptr;    // [L][2][B][H][n_text_ctx][64] self-attention K/V cache
    // decode-step buffers
    float *dx = nullptr;        // [B][d]    decoder residual stream (f32)
    bf16_t *dxb = nullptr;      // [B][d]    its bf16 copy, MEAN-CENTRED: the A operand of the LayerNorm-folded GEMVs (WL_TILED order)
    float *dmean = nullptr;     // [2][B]    ping-pong: the rows' LayerNorm means = the centring offsets of dxb
    float *dq = nullptr;        // [16][d]   query (self or cross)
    float *dpart = nullptr;     // [16][H][WM_MAXSPLIT][66] attention partials (m, l, o[64])
    float *dstats = nullptr;    // [B/16][d/16][16][2] LayerNorm partial statistics of the residual stream
    bf16_t *datt = nullptr;     // [B][d]    attention head outputs (bf16 A operand of the out-projection; WL_TILED order)
    bf16_t *dhid = nullptr;     // [B][4d]   GELU(fc1) (A operand of fc2; WL_TILED order)
    float *dlogits = nullptr;   // [B][vpad]
    unsigned long long *dargmax = nullptr;  // [16][vpad/16] per-tile packed (value, ~index) maxima
    int *dresult = nullptr;     // [16] arg-max result relative to arg_first
    int *dseq = nullptr;        // [n_text_ctx][16->B] token sequence (prompt, then generated), position-major
    int *dpos = nullptr;        // [1] current decode position (read by every decode kernel)
    // A RAGGED decode group (wm_transcribe_mel_ragged): prompts of different lengths, right-aligned to the longest (P), so
    // that every row generates its first token at position P - 1 and everything about "prompt or generated" stays one
    // scalar per group.  Row b's prompt starts at position doff[b] = P - len_b: its positional embedding and the first key
    // of its causal self-attention count from there (dec_kernels.hip).  Uploaded at prefill like dx_ids.
    int *doff = nullptr;        // [WM_DEC_MAXB]
    int *darrive = nullptr;     // [1] arrival counter of the arg-max workgroups (zero between launches)
    // early stop (wm_transcribe_greedy with eot >= 0 or per-chunk token budgets): see WmStopDev
    int *ddone = nullptr, *dbudget = nullptr, *dlive = nullptr, *dnlive = nullptr;
    int *h_nlive = nullptr;     // pinned host ring: n_live after each burst of positions (the host polls it)
    // What the setters arm for the NEXT transcribe call (and pending.dbg, the debug library's one-shots): ONE value that the call
    // takes whole, in front of its checks (tx_pending.h).  Per call, not per context: wm_clone has nothing to copy.
    WmPending pending;
    // Captured decode steps: one hipGraph of ONE position, and one of WM_BURST consecutive positions (the arg-max kernel
    // advances the device-side position, so consecutive positions do not depend on the host: 1/8 of the graph launches).
    // Everything a capture bakes into its kernel arguments is in the key (the shape and the WmDecodeMode it was captured
    // for, compared member by member); a lane keeps the last few shapes it ran
    // (a server alternating between batch sizes, bench.py's groups of 56 / 48 chunks landing on different lanes from one
    // pass to the next) instead of re-capturing ~2300 launches every time the shape changes (measured: the capture is
    // host work of a few ms that hides behind the lane's own encoder, so this is tidiness, not throughput).
    struct GraphSet {
        int B = 0, n_prompt = 0, cap_b = 0;
        WmDecodeMode mode;   // with xattn_shared false: sharing is the index below
        // [shared]: 0 = the group has the chip to itself, 1 = it shares it (xattn_shared: short-lived cross-attention
        // workgroups); chosen burst by burst from the number of decodes in flight on the device, captured on first use
        int burst[2] = {0, 0};
        WmGraph g1[2], gk[2];   // one position, burst[.] positions
        // a beam group (mode.beam): the graphs above are its PROMPT positions, these its generating ones
        int bburst[2] = {0, 0};
        WmGraph b1[2], bk[2];
        void destroy() {
            for (int i = 0; i < 2; ++i) { g1[i].destroy(); gk[i].destroy(); b1[i].destroy(); bk[i].destroy(); }
        }
        unsigned long stamp = 0;   // last use (LRU eviction)
    };
    // The ONE decoder step of a language-identification call (Whisper.swift:33-40: <|startoftranscript|> -> arg-max over the
    // language ids): ~100 launches of 3-5 us each, i.e. as long on the host (eager: ~3.5 us per launch) as on the GPU --
    // captured once per shape and replayed (round 6: the reference's own flow, device-resident, 2.23 -> see profiles/).
    struct LidGraph {
        int B = 0, cap_b = 0, first = 0, last = 0, logits = 0;
        WmGraph graph;
        void destroy() { graph.destroy(); B = 0; }
    } lid_graph;
    std::vector<int32_t> lid_host;   // host staging of the call's <|startoftranscript|> row (outlives the async upload)
    static constexpr int kMaxGraphSets = 4;
    std::vector<GraphSet> graph_sets;
    unsigned long graph_clock = 0;
    unsigned *dmask = nullptr;   // [2][vpad/32] suppressed-token bitmaps (wm_set_suppress); [1] = first generated token
    bool mask_on = false;
    std::vector<unsigned> mask_host;  // host copy of the every-position bitmap
    // timestamp rules (wm_set_timestamp_rules): per-sequence state and per-tile partials, see WmTsDev
    bool ts_on = false;
    int ts_begin = 0, ts_eot = 0, ts_max_initial = -1;
    int *dts_rng = nullptr, *dts_hist = nullptr;
    unsigned long long *dts_key = nullptr;
    float *dts_lse = nullptr;
    // wm_transcribe's extended decode (WmXDev): per-tile partials, outputs and the group's parameters
    float *dx_txt = nullptr, *dx_win = nullptr, *dx_all = nullptr, *dx_nsv = nullptr;
    float *dx_logprob = nullptr;   // [n_text_ctx][WM_DEC_MAXB]
    float *dx_nospeech = nullptr;  // [WM_DEC_MAXB]
    WmXPar *dx_par = nullptr;
    // repetition rules (wm_set_repetition_rules): the context's setting, and the device state allocated when first set
    bool rep_on = false;
    float rep_p = 1.f;
    int rep_n = 0, rep_eot = 0;
    unsigned *drep_seen = nullptr, *drep_ban = nullptr;   // [WM_DEC_MAXB][(vpad + 31) / 32]
    WmRepPar *drep_par = nullptr;
    // sampling rules (wm_set_sampling_rules): the context's setting and the device block a group's prefill writes
    int samp_k = 0;
    float samp_p = 1.f, samp_minp = 0.f;
    bool samp_on() const { return samp_k > 0 || samp_p < 1.f || samp_minp > 0.f; }
    WmSampPar *dsamp_par = nullptr;
    // alternatives (wm_request_alternatives): the device block a group's prefill writes and the group's output buffers
    // [tok | lp | cnt | ent] (reserved and pad-filled at prefill, grow-only)
    WmAltPar *dalt_par = nullptr;
    WmDevBuf alt_ws;
    // given tokens (wm_set_given_tokens): the device block a group's prefill writes and the group's table [lens | tok] (grow-only)
    WmGivenPar *dgiven_par = nullptr;
    WmDevBuf given_ws;
    int *dgiven_side = nullptr;   // ... and behind the table the side area of a given-panel phase (wm_model_given_panel_dev), set with it
    // sequence bias (wm_set_sequence_bias): the context's expanded table, and the device state allocated at full capacity when
    // first switched on (dsb.par == null before that) -- never moved: the captured graphs hold the addresses
    bool sb_on = false;
    int sb_groups = 0, sb_entries = 0;
    WmSbDev dsb = {};
    // row tables (wm_set_sequence_bias_tables; exclusive with the single table): each table's group range on the host, the pool
    // on the device at full capacity (WM_MAX_BIAS_POOL; dsbt.par stays null, dsbt.e is dsb.e) and the group's per-row
    // (first group, end group) pairs, uploaded at prefill -- allocated once, never moved
    bool sbt_on = false;
    int sbt_groups = 0, sbt_entries = 0;
    std::vector<int32_t> sbt_tab_grp;   // [n_tables + 1]
    WmSbDev dsbt = {};
    int *dsb_rng = nullptr;             // [WM_DEC_MAXB][2]
    // constraint (wm_set_constraint): the automaton's counts, and the device tables allocated at full capacity when first switched
    // on (dcst.par == null before that) -- never moved: the captured graphs hold the addresses; dcst.start is the group's row starts
    bool cst_on = false;
    int cst_states = 0, cst_edges = 0, cst_eot = 0;
    WmCstDev dcst = {};
    // [2][WM_XIDS_CAND] per-row sample ids of the group (WmXPar::ids_on) | candidate words, and behind the two, at WM_XIDS_ROWS,
    // [WM_XIDS_CAND] WmXRow: the rows' (1 / T, seed) of wm_set_sampling_rows (wm_x_rows), uploaded at prefill like the ids
    unsigned *dx_ids = nullptr;
    WmMelWin *dmel_win = nullptr;  // [WM_DEC_MAXB] the group's mel windows (wm_transcribe_mel)
    int *dxkv_rows = nullptr;      // [WM_DEC_MAXB] the group's rows of a window set (wm_transcribe_windows): the gather's row map
    // wm_align: the alignment heads (empty: openai-whisper's default, every head of layers n_text_layer / 2 ..) and the
    // workspace of a call (grown on demand)
    std::vector<int32_t> align_l, align_h;
    WmDevBuf align_ws;
    WmDevBuf acap_ws;   // an aligned transcribe group's capture buffer and alignment workspace (reserved at prefill, grow-only)
    int teacher_panel = 1;   // wm_set_teacher_panel: positions per step of the teacher-forced passes (a launch policy: same bits)
    // wm_set_prompt_panel: positions per step of a transcribe group's prompt prefill (1: none -- every prompt position is an
    // ordinary step; a launch policy: same bits), and what the context's last group prefill enqueued (P0, slices, panel steps;
    // all 0: none ran -- wmdbg_last_prompt_prefill)
    int prompt_panel = 1;
    int last_prefill[3] = {0, 0, 0};
    // wm_set_given_panel: generated positions per step of a served group's given phase (1: none; a launch policy: same bits), and
    // what the context's last group ran (first and last generated index, rounds, width; all 0: no phase -- wmdbg_last_given_panel)
    int given_panel = 1;
    int last_given_panel[4] = {0, 0, 0, 0};
    // wm_transcribe_mel_beam: the group's beam state (WmBeamDev; allocated once at its largest size, so captured graphs keep
    // their addresses) and the device buffer of the debug library's trace capture
    WmDevBuf beam_ws;
    WmDevBuf beam_trace;
    bool beam_trace_on = false;   // the group decoding on this context right now writes its trace
    // wm_transcribe_mel_speculative: the group's state (WmSpecDev) and the pinned ring the host reads a round's (live windows,
    // position) from
    WmDevBuf spec_ws;
    int *h_spec = nullptr;
    WmDevBuf pcm_stage;   // host-pointer staging of a decode group's PCM (wm_transcribe*, wm_align)
    WmDevBuf io_stage;    // staging for host-pointer model calls
};

// An immutable set of encoded windows (wm_windows_encode): the cross-attention K/V of W windows, window-major
// [W][L][2][H][1500][64] bf16 -- one window's 2L slabs are contiguous --, in a device allocation of its own: no lane's
// WmModel::xkv, so nothing a context runs between the encode and a read disturbs it.  A call that reads the set copies the
// rows of each decode group into the lane's xkv (wm_xkv_rows) where the encoder + wm_model_cross_kv would have left them.
struct wm_windows {
    int device = 0;
    wm_dims dims = {};
    const void *weights = nullptr;   // WmModel::tok_emb of the context that made it: every wm_clone of that context aliases it
    int W = 0;
    std::vector<int32_t> n_frames;   // [W] mel frames of each window (find_alignment's num_frames)
    bf16_t *store = nullptr;
    size_t bytes = 0;
};

// model.cpp
int wm_model_create(wm_ctx *ctx, const wm_dims *dims);
void wm_model_destroy(wm_ctx *ctx);
int wm_model_clone(wm_ctx *child, const wm_ctx *parent);
int wm_model_reserve(wm_ctx *ctx, int B);
int wm_model_reserve_rows(wm_ctx *ctx, int rows);   // the self-attention K/V cache alone, for `rows` decoder rows
int wm_model_set_tensor(wm_ctx *ctx, const char *name, const float *data, size_t n);
int wm_model_get_tensor(wm_ctx *ctx, const char *name, float *data, size_t n);
int wm_model_init_synthetic(wm_ctx *ctx, uint64_t seed, float matrix_gain);
int wm_model_finalize(wm_ctx *ctx);
// device-pointer cores
int wm_model_encode_dev(wm_ctx *ctx, const float *d_mel, int B, float *d_xa_out /*nullable*/);
// the same with row b's input the mel window d_win[b] (device, nullable: wm_model_encode_dev)
int wm_model_encode_win(wm_ctx *ctx, const float *d_mel, const WmMelWin *d_win, int B, float *d_xa_out /*nullable*/);
// the four parts of wm_model_encode_win, which the debug library also runs on their own: the stem (mel re-layout, conv1, conv2
// -> m->x), one layer's LayerNorm + QKV launch (m->x -> m->xn, m->qk, m->vt), the rest of the layer (attention, out-projection,
// LayerNorm, fc1, fc2 -> m->x; d_x_mid nullable: a copy of m->x after the out-projection) and ln_post (m->x -> m->xn, xa)
int wm_model_encode_stem(wm_ctx *ctx, const float *d_mel, const WmMelWin *d_win, int B);
int wm_model_encode_layer_qkv(wm_ctx *ctx, int layer, int B);
int wm_model_encode_layer_tail(wm_ctx *ctx, int layer, int B, float *d_x_mid /*nullable*/);
int wm_model_encode_post(wm_ctx *ctx, int B, float *d_xa_out /*nullable*/);
int wm_model_cross_kv(wm_ctx *ctx, int B);                 // from m->xn (bf16 encoder output)
int wm_model_set_xa(wm_ctx *ctx, const float *d_xa, int B);  // f32 xa -> m->xn (bf16)
int wm_model_decode_begin(wm_ctx *ctx, int B);
// One decoder position for all B sequences, position *m->dpos (device memory).  Expects the
// embedded input of that position in m->dx (+ m->dstats): wm_model_embed_first for the first
// position, afterwards produced by wm_model_close_step.  Ends with logits -> per-tile arg-max over
// [arg_first, arg_last] (m->dargmax); want_logits additionally stores f32 logits in m->dlogits.
// cap (wm_align): the layers with alignment heads take the unfused cross_attn_ln + query path and copy those heads' queries
// mode: see WmDecodeMode (mode.x: log-probs, no-speech, sampling -- DE_LOGITS_X and the arg-max kernel's X variant);
// n_prompt is read with mode.mask only: the first-token suppress bitmap applies at decode position n_prompt - 1
int wm_model_decode_step(wm_ctx *ctx, int B, bool want_logits, int arg_first, int arg_last, const WmAlignCap *cap = nullptr,
                         const WmDecodeMode &mode = WmDecodeMode(), int n_prompt = 0);
// the device view of the extended-decode state (par == null when mode.x is false)
WmXDev wm_model_x_dev(const WmModel *m, const WmDecodeMode &mode);
// the device view of the context's timestamp-rule state (rng == null when the rules are off)
WmTsDev wm_model_ts_dev(const WmModel *m);
// the device view of the repetition-rule state (par == null when mode.rep is false)
WmRepDev wm_model_rep_dev(const WmModel *m, const WmDecodeMode &mode);
// (1.0, 0, any eot) switches the rules off; the first enabling call allocates the bitmaps
int wm_model_set_repetition_rules(wm_ctx *ctx, float penalty, int ngram, int32_t eot);
// (0, 1, 0) switches the rules off; validation is the caller's (wm_set_sampling_rules)
int wm_model_set_sampling_rules(wm_ctx *ctx, int top_k, float top_p, float min_p);
// the truncation launch of a generating position of a group with mode.trunc, between wm_model_decode_step (want_logits) and the close
int wm_model_sample_truncate(wm_ctx *ctx, int B, int n_prompt, const WmDecodeMode &mode);
// a group's prefill with mode.alt: reserves alt_ws for rows x max_new x n, pad-fills it and uploads *host_par (which must outlive
// the stream's copy) with the buffers' addresses filled in
int wm_model_alt_begin(wm_ctx *ctx, int rows, int max_new, int n, WmAltPar *host_par);
// the alternatives launch of a position of a group with mode.alt, between wm_model_decode_step (want_logits) and the close
int wm_model_alternatives(wm_ctx *ctx, int B, int n_prompt, const WmDecodeMode &mode);
// a group's prefill with mode.given: uploads the group's table -- lens [rows], tok [rows][stride], host memory that outlives the
// stream's copies -- into given_ws and *host_par, with the addresses filled in, into the context's block
int wm_model_given_begin(wm_ctx *ctx, int rows, int stride, const int32_t *lens, const int32_t *tok, WmGivenPar *host_par);
// the given-tokens launch of a position of a group with mode.given: last in front of the close
int wm_model_given_tokens(wm_ctx *ctx, int B, int n_prompt, const WmDecodeMode &mode);
// the device view of the sequence-bias state (par == null when mode.sb is false)
WmSbDev wm_model_sb_dev(const WmModel *m, const WmDecodeMode &mode);
// an expanded table (empty: off) -> this context's device table; the first non-empty one allocates the state
int wm_model_set_sequence_bias(wm_ctx *ctx, const WmSbTable &t);
// the pooled tables (no tables: off) -> this context's device pool; the first non-empty set allocates it.  Replaces the single
// table, as wm_model_set_sequence_bias replaces the tables.
int wm_model_set_sequence_bias_tables(wm_ctx *ctx, const WmSbPool &p);
// a checked automaton (no states: off) -> this context's device tables; the first non-empty one allocates them
int wm_model_set_constraint(wm_ctx *ctx, const WmCstTable &t);
int wm_model_set_timestamp_rules(wm_ctx *ctx, int enable, int32_t ts_begin, int32_t eot, int32_t max_initial);
int wm_model_set_suppress(wm_ctx *ctx, const int32_t *ids, int n, const int32_t *first_ids, int n_first);
// Speculative decoding (wm_transcribe_mel_speculative, spec.hip): the device view of one decode group of G
// windows on the target context and its draft.  The target's WmTsDev rng slots are per ROW of the verify step (G x w); the
// windows' committed timestamp-rule state lives here, beside the draft's.
struct WmSpecDev {
    int *tseq, *dseq;        // the two token buffers [n_text_ctx][G]
    int *tpos, *dpos;        // the two device positions
    WmTsDev tts, dts;        // the two models' timestamp rules (rng == null: off)
    int *chist, *crng;       // [G][4] the target's committed history and ranges
    int *dchist, *dcrng;     // [G][4] the draft's
    int *wtok;               // [G x w] the rows' winners
    float *wlp;              // [G x w] and their log-probs
    int *acc;                // [G] leading rows whose winner equals the proposal
    int *stats;              // [G][4] wm_spec_stats
    int *round;              // [2] live windows, position after the round (what the host reads behind an event)
    const int *script;       // debug library (wmdbg_spec_script; null in the product): [G][max_new] proposals by generated index
    int max_new, n_vocab;
};
// the verify step: wm_model_decode_step's layer body over G windows x w consecutive positions with the group's own mode (the
// masks, the extended-decode partials, the timestamp rules of the plain step), closed by wm_spec_accept instead of the arg-max
int wm_model_spec_panel_step(wm_ctx *ctx, int G, int w, const WmDecodeMode &mode, int n_prompt);
// the group's state on the target context (allocated on first use) for `draft`
// *script_area: device room for a debug script of the group, [WM_DEC_MAXB][n_text_ctx] ints (WmSpecDev::script stays null)
int wm_model_spec_dev(wm_ctx *ctx, wm_ctx *draft, int max_new, WmSpecDev *out, int **script_area);
int wm_spec_adopt(wm_ctx *draft, const WmSpecDev &sp, int G, int n_prompt);
int wm_spec_stage(wm_ctx *ctx, const WmSpecDev &sp, int G, int w, int n_prompt, int n_ctx);
int wm_spec_accept(wm_ctx *ctx, const unsigned long long *tilemax, int n_tiles, const WmSpecDev &sp, const WmXDev &xd,
                   const WmStopDev &stop, int G, int w, int n_prompt, int n_ctx, int fallback_tok);
// wm_spec_accept = the accept launch, then this one on the same stream
int wm_spec_commit(wm_ctx *ctx, const WmSpecDev &sp, const WmXDev &xd, const WmStopDev &stop, int G, int w, int n_prompt, int n_ctx);
// Prompt panels (wm_set_prompt_panel, tx_plan.h wm_prompt_panel_plan): positions [0, P0) of a plain group of G rows as
// cache-only panel steps at the context's width, then *dpos = P0 and rows 0 .. G - 1 of dx / dxb / dstats / dmean hold the
// embedding of position P0 as the close of step P0 - 1 would have left it.  P0 >= 2 and a width > 1 (the plan says so).
int wm_model_prompt_prefill(wm_ctx *ctx, int G, int P0, const WmDecodeMode &mode);
// Given panels (wm_set_given_panel, tx_plan.h wm_given_panel_plan): generated indices [1, Lp) of a served group of G rows, the
// device position at n_prompt, as rounds of w positions (given_panel.hip); then *dpos = n_prompt + Lp - 1, the stop state, the
// rules' state and rows 0 .. G - 1 of dx / dxb / dstats / dmean are what the plain steps would have left.  Needs the group's
// table uploaded (wm_model_given_begin).
struct WmGivenPanelDev;
int wm_model_given_panel_phase(wm_ctx *ctx, int G, int w, int Lp, int n_prompt, int max_new, const WmDecodeMode &mode);
// the device view of a group's given-panel state (the side area lives behind the table in given_ws)
int wm_model_given_panel_dev(wm_ctx *ctx, int max_new, WmGivenPanelDev *out);
int wm_model_embed_first(wm_ctx *ctx, int B, const WmDecodeMode &mode = WmDecodeMode());
// arg-max reduce + write next token (positions >= n_prompt) + embed next position + advance *dpos
int wm_model_close_step(wm_ctx *ctx, int B, int n_prompt, bool write_seq, int *result, int arg_first,
                        const WmDecodeMode &mode = WmDecodeMode());
// the device view of the early-stop state (done == null when mode.stop is false)
WmStopDev wm_model_stop_dev(const WmModel *m, const WmDecodeMode &mode);
// the embedding tables and the residual-stream target of the context's decoder
WmEmbedDev wm_model_embed_dev(const WmModel *m);
// beam search: the device view of the group's beam state (allocating it on first use), its initial state for `rows` rows in
// `windows` windows (par and budgets [windows] are host memory that outlives the upload), and the close of a generating
// position: per-row lists, per-window selection + next embedding + position advance, re-parenting of the caches
int wm_model_beam_dev(wm_ctx *ctx, const WmDecodeMode &mode, WmBeamDev *out);
int wm_model_beam_begin(wm_ctx *ctx, const WmDecodeMode &mode, int rows, int windows, const WmBeamPar *par, const int32_t *budgets);
int wm_model_beam_close(wm_ctx *ctx, int B, int n_prompt, const WmDecodeMode &mode);
size_t wm_model_beam_state_bytes(const WmModel *m);   // the part of beam_ws in front of fin_tok (what a drain copies whole)
void wm_model_drop_graphs(WmModel *m);
int wm_model_set_pos(wm_ctx *ctx, int pos);
// Teacher-forced PANEL pass (wm_set_teacher_panel).  A panel step is wm_model_decode_step's layer body over C windows x w
// consecutive positions (mode.panel = w, rows c * w + s <-> (window c0 + c, position *dpos + s)): the windows are rows
// c0 .. c0 + C - 1 of a group of G whose token buffer m->dseq is [n_text_ctx][G] and whose caches are [L][2][G][H][.][64].
// Row arithmetic is the step path's, so every output bit is the step path's.
// wm_model_panel_slices: how a group of G windows is cut for a pass of T positions at the context's width -- *C windows per
// slice, *w <= width positions per panel (C * w <= WM_DEC_MAXB; the measured rule: the fewest steps).
void wm_model_panel_slices(int G, int width, int T, int *C, int *w);
// embed positions *dpos .. *dpos + w - 1 of the slice's windows into rows c * w + s of m->dx / dxb / dstats / dmean
int wm_model_panel_embed(wm_ctx *ctx, int G, int c0, int C, int w);
int wm_model_panel_step(wm_ctx *ctx, int G, int c0, int C, int w, bool want_logits, const WmAlignCap *cap);
// *dpos += w and the embedding of the next panel (w_next positions; 0: none) -- what wm_model_close_step does for a step,
// without the arg-max nobody reads in teacher forcing
int wm_model_panel_advance(wm_ctx *ctx, int G, int c0, int C, int w, int w_next);

// ---------------------------------------------------------------- kernel launchers ----
// gemm.hip
enum GemmEpi {
    EPI_BIAS_BF16 = 0,  // C bf16 [.][ldc] = acc + bias
    EPI_GELU_BF16 = 1,  // C bf16 = gelu(acc + bias)
    EPI_RESID_F32 = 2,  // C f32 += acc + bias
    EPI_CONV2_F32 = 3,  // C f32 = gelu(acc + bias) + pos[m % rows_per_batch][n]
    EPI_QKV_ENC = 4,    // n < 2d: C bf16 [m][2d] (query columns n < d multiplied by WM_ENC_QSCALE);  n >= 2d: vt[b][h][e][s]
    EPI_XKV = 5,        // cross K/V cache scatter
    EPI_F32 = 6         // C f32 = acc + bias (debug / generic)
};
// The encoder's queries are stored PRE-SCALED by hd^-1/2 * log2(e) (hd = 64): one f32 multiply in the QKV epilogue before
// its single bf16 rounding, so that the attention kernel's score accumulators are exponents of 2 already (enc_kernels.hip).
#define WM_ENC_QSCALE (0.125f * 1.44269504088896340736f)
// Key position s of a chunk -> its column in the encoder's V^T buffer [b][h][e][seq_pad]: the two middle 4-key groups of
// every 16 keys are swapped, so that the 8 keys one lane of the attention kernel multiplies per MFMA k-step are 16
// contiguous bytes (enc_kernels.hip).
__host__ __device__ static inline unsigned wm_att_vt_pos(unsigned s) { return (s & ~12u) | ((s & 4u) << 1) | ((s & 8u) >> 1); }
struct GemmArgs {
    const bf16_t *A;   // rows addressed as (m / a_rpb) * a_bstride + (m % a_rpb) * a_rstride
    long a_rpb, a_bstride, a_rstride;
    const bf16_t *W;   // [N][K]
    const float *bias; // [N] or null
    void *C;
    long c_rpb, c_bstride, c_rstride;  // same row addressing for C (elements)
    int M, N, K;
    int epi;
    // epilogue extras
    const float *pos;  // EPI_CONV2_F32
    bf16_t *vt;        // EPI_QKV_ENC
    int d_model, n_head, seq, seq_pad, batch;  // EPI_QKV_ENC / EPI_XKV
};
int wm_gemm(wm_ctx *ctx, const GemmArgs &g);

// enc_kernels.hip
int wm_layernorm(wm_ctx *ctx, const float *x, const float *g, const float *b, int rows, int d,
                 bf16_t *out_bf16 /*nullable*/, float *out_f32 /*nullable*/);
// d_win (nullable, device [B]): row b = window d_win[b] of a [n_mels][T] block (wm_transcribe_mel); null: mel [B][n_mels][3000]
int wm_mel_to_time_major(wm_ctx *ctx, const float *mel, int B, int n_mels, bf16_t *mel_t, const WmMelWin *d_win = nullptr);
int wm_f32_to_bf16(wm_ctx *ctx, const float *in, bf16_t *out, size_t n);
int wm_enc_attention(wm_ctx *ctx, const bf16_t *qk, const bf16_t *vt, bf16_t *att, int B, int H,
                     int S, int S_pad, int d);

// dec_kernels.hip
static_assert(WM_MAX_TEACHER_PANEL == 8, "tx_plan.h WM_PANEL_MAX_WIDTH restates it");
static_assert(WM_MAX_TEACHER_PANEL == WM_MAX_BEST_OF, "a panel's cross-attention is dec_xcand_attn_kernel: its instantiated widths");
static_assert(WM_XIDS_CAND == WM_DEC_MAXB + 16, "WmXDev::ids: the candidate words follow the padded sample ids");
static_assert(WM_XIDS_ROWS == 2 * WM_XIDS_CAND && WM_XIDS_ROWS % 4 == 0 && WM_XIDS_WORDS == WM_XIDS_ROWS + 4 * WM_XIDS_CAND && sizeof(WmXRow) == 16,
              "WmXDev::ids: the sampling rows follow the candidate words, 16-byte aligned");
constexpr int WM_NLIVE_RING = 16;  // pinned host slots for the per-burst live-row counts (early stop)
constexpr int WM_MAXSPLIT = 8;  // stream partials of a (sequence, head) pair of the cross-attention (small batches)
// (enum DecEpi: dec_launch.h)
struct DecGemvArgs {
    int epi;
    int B, N, K;
    const bf16_t *W;    // [N (padded to 16)][K] in WL_TILED order; LayerNorm mode: the gamma-folded copy
    const float *c1;    // LayerNorm mode (non-null): column sums of the folded weights, see DecLayerW
    const float *c2;    // [N] bias (LayerNorm mode: + beta fold) or null
    const bf16_t *a;    // [B padded to 16][K] bf16 activations in WL_TILED order (wm_tiled_offset(b, k, K))
    const float *stats_in; // LayerNorm mode: [B/16][K/16][16][2] partial (sum, sum of squares) per row of the f32 residual,
    int stats_parts;       //                 from the producer of the residual (always K/16 parts; unused ones are zero)
    float *stats_out;      // DE_RESID: [B/16][N/16][16][2] partials of the updated residual (may be null)
    // mean-centring of the bf16 residual copy (dec_kernels.hip, DecGemvDev::mean_in): [B] f32 each, nullable.
    // DE_RESID reads the offsets; a LayerNorm-mode launch reads them and writes the rows' new means to mean_out
    // (the OTHER buffer of a ping-pong pair).
    const float *mean_in;
    float *mean_out;
    // outputs
    float *out_f32;        // DE_QKV: q [B][N/3]; DE_Q: [B][ldo]; DE_RESID: residual [B][ldo] (+=); DE_LOGITS: [B][ldo] or null
    bf16_t *out_bf16;      // DE_GELU: [B][ldo]; DE_RESID: bf16 copy of the updated residual (may be null); WL_TILED order
    bf16_t *kcache, *vcache;  // DE_QKV: this layer's [B][H][T][64]
    const int *pos_ptr;       // device-side decode position (DE_QKV appends at *pos_ptr)
    int n_ctx, n_head;
    long ldo;
    unsigned long long *argmax;  // DE_LOGITS: per-tile packed maxima [B][ceil(N/16)] over [arg_first, arg_last]
    int arg_first, arg_last;
    // DE_LOGITS: suppressed-token bitmaps (bit n of word n/32), [2][mask_words]: [0] every position, [1] the position
    // *pos_ptr == mask_first_pos only (first generated token); null = no filter
    const unsigned *mask;
    int mask_words, mask_first_pos;
    WmTsDev ts;  // DE_LOGITS: timestamp rules (ts.rng == null: off)
    WmXDev x;    // DE_LOGITS_X: extended decode (x.par non-null)
    // optional L2 warm-up of the NEXT skinny GEMV's weights ([pf_rows][pf_k] bf16, WL_TILED)
    const bf16_t *pf_ptr;
    int pf_rows, pf_k;
    int pf_head_major;     // the next launch is wm_dec_xattn_fq: (pairs per XCD) place every head's tiles on the XCD(s) that run it
    WmRepDev rep;          // DE_LOGITS_XR / _XB: repetition rules (rep.par non-null)
    WmSbEpi sb;            // DE_LOGITS_XB: sequence bias (sb.hit non-null)
    int panel;             // DE_QKV_P: panel width w (1 .. WM_MAX_TEACHER_PANEL); kcache / vcache are [ceil(B / w)][H][T][64]
};
int wm_dec_gemv(wm_ctx *ctx, const DecGemvArgs &a);
// cross_attn_ln + query projection fused INTO the cross-attention launch (96 .. 256 pairs, alone on the device): qa = the
// DE_Q LayerNorm-mode arguments the separate GEMV would get (out_f32 unused), t = the cross-attention's (kc, vc, att, B, H,
// T_stride, n_keys, live, pf).  Same bits as the two launches.
bool wm_dec_xattn_fq_applies(int B, int H, int K, bool short_lived);
struct DecAttnArgs;
int wm_dec_xattn_fq(wm_ctx *ctx, const DecGemvArgs &qa, const DecAttnArgs &t);
// W' = bf16(W g) (WL_TILED in, WL_TILED out), c1 = row sums of W', c2 = bias + W beta; rows N .. pad16(N) give zeros
int wm_ln_fold(wm_ctx *ctx, const bf16_t *W, const float *g, const float *beta, const float *bias /*nullable*/, int N,
               int K, bf16_t *Wf, float *c1, float *c2);
// x[b] = token_embedding[seq[*pos_ptr][b]] + positional_embedding[*pos_ptr]
// off (device [B], nullable: all 0): the row offsets of a ragged decode group -- row b's positional row is
// max(*pos_ptr - off[b], 0); the same argument of wm_argmax_embed, and of wm_dec_self_attention (keys [min(off[b], pos), pos])
int wm_dec_embed(wm_ctx *ctx, const int *seq, const int *pos_ptr, int B, const WmEmbedDev &e, const int *off);
// Panel embedding: row c * w + s (c < C, s < w) = token seq[(*pos_ptr + s) * seq_stride + c] at positional row *pos_ptr + s.
// Position 0 is embedded with wm_dec_embed's four-wave sums, every later one with the closing kernels' embed_row: the bits of
// the step path's first embedding and of its closes.  pos_add: added to *pos_ptr (the embedding of the NEXT panel).
// off (device [C], nullable): the windows' offsets in a ragged group -- the positional row is max(*pos_ptr + s - off[c], 0)
int wm_dec_embed_panel(wm_ctx *ctx, const int *seq, int seq_stride, const int *pos_ptr, int pos_add, int C, int w, int n_ctx,
                       const WmEmbedDev &e, const int *off = nullptr);
// *pos_ptr += add (one thread)
int wm_dec_pos_add(wm_ctx *ctx, int *pos_ptr, int add);
// Single-query attention over a K/V cache [B][H][T_stride][64] -> bf16 head outputs att[B][H*64] in WL_TILED order.
// Keys 0 .. n-1 with n = *pos_ptr + 1 when pos_ptr != null, else n_keys.  One argument struct for every form; a form reads
// the fields its comment names and ignores the rest (zero them: DecAttnArgs t = {}).
struct DecWarm {           // optional L2 warm-up of the NEXT skinny GEMV's weights by extra workgroups of this launch
    const bf16_t *ptr;     // [rows][k] bf16, WL_TILED; null: none
    int rows, k;
};
struct DecAttnArgs {
    const float *q;        // [rows][H * 64] f32 queries
    const bf16_t *kc, *vc; // K / V cache [B (or C)][H][T_stride][64]
    bf16_t *att;           // [rows][H * 64] bf16 head outputs, WL_TILED
    float *part;           // [rows][H][8][66] f32 stream partials: a split cross launch, a candidate group below 256 pairs
    int B;                 // rows = sequences (cross, fused-query, self)
    int C, N;              // candidate group / panel: C windows x N rows per window (candidates; panel positions w), rows c * N + s
    int H;                 // heads
    int T_stride;          // cache rows per (sequence, head) pair
    int n_keys;            // keys when pos_ptr is null (the cross forms: always)
    const int *pos_ptr;    // self forms: device decode position, keys 0 .. *pos_ptr (a panel row: .. *pos_ptr + s)
    int nsplit;            // cross: workgroups per pair, 1 / 2 / 4 / 8 (wm_dec_attn_splits)
    const int *live;       // early stop: device [WM_DEC_MAXB] compact live rows | [1] their count; null: every row is live
    const int *off;        // self: device [B] row offsets of a ragged decode group (keys [min(off[b], pos), pos]); null: all 0
    DecWarm pf;            // warm-up of the next GEMV's weights
    bool short_lived;      // cross forms: the chip is shared with other decode groups (one short-lived workgroup per pair)
};
int wm_dec_attn_splits(int B, int H);
// The cross-attention (8 streams per pair): q, kc, vc, att, part, B, H, T_stride, n_keys, nsplit, live, pf, short_lived
int wm_dec_attention(wm_ctx *ctx, const DecAttnArgs &t);
// Cross-attention of a candidate group: C windows x N candidates (rows c * N + s of q / att), K/V [C][H][T_stride][64], every
// block of a window's K/V requested once for all its live candidates.  Row bits = wm_dec_attention's over a copy of the cache.
// q, kc, vc, att, part (the flat deal below 256 pairs), C, N, H, T_stride, n_keys, live, pf, short_lived
int wm_dec_attention_cand(wm_ctx *ctx, const DecAttnArgs &t);
// The decoder's causal self-attention (<= 448 cached rows per pair): one 4-wave workgroup per (sequence, head).
// q, kc, vc, att, B, H, T_stride, n_keys, pos_ptr, live, off, pf
int wm_dec_self_attention(wm_ctx *ctx, const DecAttnArgs &t);
// The self-attention of a panel step: B = C * w rows (w = N), the pair (r, h) reads cache entry (r / w, h) of kc / vc [C][H][T_stride][64]
// with *pos_ptr + r % w + 1 keys; query and output are row r.  Row bits = wm_dec_self_attention's at that position.
// q, kc, vc, att, C, N, H, T_stride, pos_ptr, pf
int wm_dec_self_attention_panel(wm_ctx *ctx, const DecAttnArgs &t);
// Close a decode step (one workgroup): reduce the per-tile packed maxima of a DE_LOGITS launch;
// chosen token of row b -> seq[(*pos_ptr + 1) * B + b] when that position is >= n_prompt;
// (token - arg_first) -> result[b]; embed the tokens of position *pos_ptr + 1 into x (+ LayerNorm
// partial statistics) when e.x != null; then *pos_ptr += 1.  seq / pos_ptr / result / e.x may be null.
// arrive: zero-initialised device counter, required above 16 rows (one workgroup per 16 rows; the last one to arrive
// advances the position; null: one workgroup).  fallback_tok: the token taken when nothing is admissible (all suppressed /
// NaN logits).  ts / stop / xd: an empty struct (WmTsDev{} ...) is "off"; off: see wm_dec_embed.
int wm_argmax_embed(wm_ctx *ctx, const unsigned long long *tilemax, int n_tiles, int B, int *seq, int *pos_ptr,
                    int n_prompt, int *result, int arg_first, int n_ctx, const WmEmbedDev &e, const WmTsDev &ts, int *arrive,
                    int fallback_tok, const WmStopDev &stop, const WmXDev &xd, const int *off);
// Gumbel noise g(n) of ids n0 .. n0 + count - 1 as the DE_LOGITS_X epilogue computes it (philox.h), into device memory
int wm_sample_noise(wm_ctx *ctx, uint64_t seed, int chunk, int gi, int n0, int count, float *out);
// start of a decode with early stop: no row done, every row live
int wm_stop_init(wm_ctx *ctx, const WmStopDev &stop, int B);
// initial timestamp-rule state of B sequences (before the first sampled token)
int wm_ts_init(wm_ctx *ctx, const WmTsDev &ts, int B);
int wm_range_softmax(wm_ctx *ctx, const float *logits, long ldo, int B, int first, int n, float *probs);
int wm_fill_synthetic(wm_ctx *ctx, const WmTensor &t, uint32_t seed, int tensor_id, float gain);

// The rows of a group as the kernels between the logits launch and the close see them (stored_row.h): the stored f32 logits
// [rows][ldo] of n_vocab ids and the per-tile partials the DE_LOGITS_X* launch of the same position left (tilemax, xd, ts;
// (n_vocab + 15) / 16 tiles per row), the suppress bitmap (mask, nullable: [2][mask_words], the first generated position's row
// behind the every-position one), the device position, the stop state (done rows are skipped) and the rows' ban bitmaps (ban,
// nullable: [rows][ban_words], WmRepDev::ban -- a banned id is not admissible).  wm_model_stored_rows builds it from a model.
struct WmStoredRows {
    const float *logits;
    long ldo;
    int n_vocab;
    unsigned long long *tilemax;
    int rows;
    WmTsDev ts;
    WmXDev xd;
    const unsigned *mask;
    int mask_words, n_prompt;
    const int *pos_ptr;
    WmStopDev stop;
    const unsigned *ban;
    int ban_words;
};
// what every stored-row entry point requires of it; needs_win: the kernel rewrites the winner values (xd.win)
inline int wm_stored_rows_check(const WmStoredRows &r, const char *who, bool needs_win) {
    WM_REQUIRE(r.rows >= 1 && r.rows <= WM_DEC_MAXB && r.logits && r.tilemax && r.xd.par && r.xd.txt && (!needs_win || r.xd.win) && r.pos_ptr,
               WM_ERR_INVALID, "%s: bad group", who);
    WM_REQUIRE(r.n_vocab >= 1 && r.ldo >= r.n_vocab, WM_ERR_INVALID, "%s: %d ids in rows of %ld", who, r.n_vocab, r.ldo);
    WM_REQUIRE(!r.mask || (long)r.mask_words * 32 >= r.n_vocab, WM_ERR_INVALID, "%s: %d mask words do not cover %d ids", who, r.mask_words,
               r.n_vocab);
    WM_REQUIRE(!r.ban || (long)r.ban_words * 32 >= r.n_vocab, WM_ERR_INVALID, "%s: %d ban words do not cover %d ids", who, r.ban_words,
               r.n_vocab);
    WM_REQUIRE(!r.ts.rng || (r.ts.key_ts && r.ts.lse && r.ts.ts_begin >= 0), WM_ERR_INVALID, "%s: incomplete timestamp-rule state", who);
    return WM_OK;
}
// the shape of a panel round: G windows x w positions are the rows of one step
inline int wm_panel_shape_check(int G, int w, const char *what) {
    WM_REQUIRE(G >= 1 && w >= 1 && w <= WM_MAX_TEACHER_PANEL && G * w <= WM_DEC_MAXB, WM_ERR_INVALID, "%s: %d windows x %d rows", what, G, w);
    return WM_OK;
}

// beam.hip (beam search)
// Per row (grid: rows) the <= N + 1 best admissible tokens of the stored logits with their log-probs under the filtered
// distribution; rows of windows that have left and dead beams get an empty list.  Also no_speech_prob when the position is
// par->sot_pos.  (rows.stop is not read: a beam group's windows leave through bm.wdone.)
int wm_beam_topk(wm_ctx *ctx, const WmStoredRows &rows, const WmBeamDev &bm);
// Per window the selection (beam.h), finished records, the rows' new tokens / sums / sources / timestamp-rule state, the
// early-stop flags and live list, the embedding of the next position and *pos_ptr += 1 (one workgroup).
int wm_beam_select_step(wm_ctx *ctx, int rows, int *seq, int *pos_ptr, int n_prompt, const WmEmbedDev &e, const WmTsDev &ts,
                        const WmStopDev &stop, const WmXDev &xd, const int *off, const WmBeamDev &bm);
// Re-parent what follows a beam, by bm.src within each window, in place: rows [0, *pos_ptr - 1] of every layer's and head's
// self-attention K/V (skv [L2][rows][H][T][64]) and the rows' token / log-prob histories.  Call after wm_beam_select_step.
int wm_beam_reorder(wm_ctx *ctx, bf16_t *skv, int L2, int rows, int H, int T, const int *pos_ptr, int n_prompt, int *seq,
                    float *logprob, const WmBeamDev &bm);

// sample_trunc.hip (sampling rules)
// Per row (grid: rows) of a sampling group at a generated position: the kept set of *par over the row's admissible ids
// (stored_row.h: ranges, mask, ban; `forced` from the partials), the Gumbel-max draw over it with the epilogue's Philox counters,
// and the row's per-tile keys (tilemax, ts.key_ts) and winner values (xd.win) rewritten so that the close picks that id; the
// log-sum-exp partials are left alone.  Rows with stop.done set, prompt positions and arg-max calls are skipped.  dbg
// (nullable, device): [rows][3] kept count, last kept id, drawn id.
int wm_sample_truncate(wm_ctx *ctx, const WmStoredRows &rows, const WmSampPar *par, int *dbg);

// alternatives.hip (top-n alternatives and entropy)
// Per row (grid: rows) at a generated position gi < par->max_new: the par->n best ids of the row's admissible set in descending
// key order (stored_row.h's admissibility, row_list.h's list scan; `forced` and the normaliser from the partials) with log-probs
// value - norm, the count and the entropy, written at [gi][row] of par's buffers (cnt, ent nullable).  Rows with stop.done set
// and prompt positions are skipped.  Reads the partials, writes par's buffers alone.
int wm_alternatives(wm_ctx *ctx, const WmStoredRows &rows, const WmAltPar *par);

// given.hip (given tokens)
// Per row (grid: rows) at a generated position gi < par->lens[row]: the row's per-tile keys (tilemax, ts.key_ts) and the winner
// value of one tile are rewritten so that the close takes par->tok[row][gi], with the log-prob value - norm of the stored
// logits under the row's own `forced` (-inf where the id is not admissible: stored_row.h row_admits).  Rows with stop.done set,
// prompt positions and rows with gi >= lens are not touched.  The log-sum-exp partials are read, never written.
int wm_given_tokens(wm_ctx *ctx, const WmStoredRows &rows, const WmGivenPar *par);

// given_panel.hip (given tokens in panels, wm_set_given_panel)
// A round of a served group of G windows at position pos = *pos_ptr (generated index g0 = pos + 1 - n_prompt) closes w positions per
// window: row c * w + s of the panel step is window c at position pos + s.  The windows' committed timestamp-rule state lives in
// the side area (chist, crng) while the rounds run: the rng slots of WmTsDev are per ROW of the step (G x w).
struct WmGivenPanelDev {
    int *seq;          // the token buffer [n_text_ctx][G]
    int *pos;          // the device position
    WmTsDev ts;        // the timestamp rules (rng == null: off)
    int *chist, *crng; // [G][4] committed history and ranges
    int *wtok;         // [G x w] the rows' tokens as their close chose them
    float *wlp;        // [G x w] and their log-probs
    const WmGivenPar *par;   // the group's table
    int max_new, n_vocab;
};
// STAGE (one workgroup, thread c owns window c): tokens tok[c][g0 + s - 1], s = 1 .. w - 1, go to positions pos + s of the token
// buffer (a row without a token there -- finished by its budget -- gets stop.pad_tok) and the rules' ranges after the tokens up
// to each row's own input go to the rows' rng slots.  first: the committed state is taken from ts.hist / ts.rng [G] first.
int wm_given_panel_stage(wm_ctx *ctx, const WmGivenPanelDev &gp, const WmStopDev &stop, int G, int w, int n_prompt, int n_ctx, bool first);
// CLOSE (one workgroup per window, wave s closes row (c, s)) and COMMIT (one workgroup, thread c owns window c).  The close: per row
// given_tokens_kernel's steps (`forced` from the partials, the admissibility of the one id, the hand-over into the row's keys)
// and then the arg-max close's calls into dec_close.h on what the hand-over left.  The commit: a live window writes its tokens and
// log-probs up to its first eot / the end of its budget and pads behind, advances its committed rule state and its done flag;
// the position advances by w; the live list is rebuilt.  last: ts.hist / ts.rng get the [G] layout of the step path back.
// rows: the G x w rows of the panel step (rows.rows == G * w, rows.ts == gp.ts; no ban rows: a served group has no per-row rule
// state, and never the first generated position: the ordinary step takes it).
int wm_given_panel_close(wm_ctx *ctx, const WmStoredRows &rows, const WmGivenPanelDev &gp, int G, int w, int fallback_tok, bool last);
int wm_given_panel_commit(wm_ctx *ctx, const WmGivenPanelDev &gp, const WmXDev &xd, const WmStopDev &stop, int G, int w, int n_prompt,
                          bool last);

// repeat.hip (repetition rules)
// Rebuild rows 0 .. B - 1 of rep.seen / rep.ban from the generated history of position *pos_ptr: tokens seq[(n_prompt + i) * B + b],
// i < min(*pos_ptr + 1 - n_prompt, n_ctx - n_prompt) (none at a prompt position).  V: ids at or above it set no bit.
int wm_repeat_state(wm_ctx *ctx, const int *seq, const int *pos_ptr, int B, int n_prompt, int n_ctx, int V, const WmRepDev &rep);

// seqbias.hip (sequence bias)
// Rebuild rows 0 .. B - 1 of sb.e (hit bitmap, sorted (id, total) list, count) from the generated history of position *pos_ptr, as
// wm_repeat_state reads it, and OR the banned ids (total -inf) into ban [B][ban_words] -- which a wm_repeat_state launch in front
// of this one has rebuilt.  V: ids at or above it set no bit.
int wm_seqbias_state(wm_ctx *ctx, const int *seq, const int *pos_ptr, int B, int n_prompt, int n_ctx, int V, const WmSbDev &sb,
                     unsigned *ban, int ban_words);
// constraint.hip (constraint)
// The rows' ban words |= the ids of [0, eot] their automaton states do not allow; launched behind wm_repeat_state (and the
// sequence-bias launch) on the same stream.  state_out (nullable, [B]): the state each row reached (-1: dead; a row that wrote
// nothing keeps what it had).
int wm_constraint_state(wm_ctx *ctx, const int *seq, const int *pos_ptr, int B, int n_prompt, int n_ctx, int V, const WmCstDev &cst,
                        unsigned *ban, int ban_words, int *state_out);
// seqbias_rows.hip (row tables)
// The same rebuild with a table per row: `pool` holds the concatenated tables (WmSbPool; pool.par is not read), row b walks groups
// [rng[2 * b], rng[2 * b + 1]) of it -- at most WM_MAX_BIAS_ENTRIES groups; an empty range (no table, an empty table) gives an
// all-zero hit row, cnt 0 and leaves the row's ban words alone.
int wm_seqbias_rows_state(wm_ctx *ctx, const int *seq, const int *pos_ptr, int B, int n_prompt, int n_ctx, int V, const WmSbDev &pool,
                          const int *rng, unsigned *ban, int ban_words);

// xkv_rows.hip (window sets)
// Copy whole windows between a decode group's cross-attention K/V cache, group [L2][group_rows][slab] (slab = H * 1500 * 64
// elements, L2 = 2 * n_text_layer), and a window-major store [.][L2][slab]: group row b <-> store row d_rows[b] (device,
// nullable: row0 + b), b < n_rows <= group_rows.  to_store: group -> store (the rows of d_rows must differ), else store -> group.
int wm_xkv_rows(wm_ctx *ctx, bf16_t *group, long group_rows, bf16_t *store, const int *d_rows, int row0, int n_rows, int L2,
                long slab, bool to_store);

// align.hip (word-level timestamps)
// the alignment heads' queries of decode position *pos_ptr: dq [B][d] -> cap[b][*pos_ptr][L.slot0 + k][64]
// panel > 1: dq holds B = windows x panel rows, row r is position *pos_ptr + r % panel of chunk r / panel
// base >= 0 (panel 1 only): capture row *pos_ptr - base, nothing in front of base (WmAlignCap::base)
int wm_align_capture_q(wm_ctx *ctx, const float *dq, int d, int B, const WmAlignLayer &L, float *cap, int Tq, int J,
                       const int *pos_ptr, int panel = 1, int base = -1);
// position pos = *pos_ptr, i = pos - S in [0, n_text[b]): prob[b][i] = softmax(logits[b][0 : eot])[seq[pos + 1][b]]
// panel > 1: logits holds B = windows x panel rows (row r: position *pos_ptr + r % panel of chunk r / panel; n_text and prob
// per chunk); seq_stride: chunks per position of seq (0: B)
int wm_align_token_prob(wm_ctx *ctx, const float *logits, long ldo, const int *seq, const int *pos_ptr, int B, int S, int eot,
                        const int *n_text, float *prob, int max_text, int panel = 1, int seq_stride = 0);
// scores -> softmax -> z-score -> median filter -> head mean -> a.x (max_n: largest n_text, max_m: largest n_frames / 2)
// Captured queries + statistics + cost matrix of ONE chunk of an alignment group (T decoder rows, J heads, n_ld matrix rows), and
// the chunks a group may hold under the 2 GiB budget of wm_align and of an aligned transcribe call alike
constexpr size_t WM_ALIGN_CAPTURE_BUDGET = (size_t)2 << 30;
inline size_t wm_align_chunk_bytes(size_t T, size_t J, size_t n_ld) { return T * J * (64 * 4 + 8) + J * 1500 * 8 + n_ld * 1500 * 4; }
inline int wm_align_group_rows(size_t T, size_t J, size_t n_ld) {
    const size_t g = WM_ALIGN_CAPTURE_BUDGET / wm_align_chunk_bytes(T, J, n_ld);
    return (int)(g < 1 ? 1 : (g > (size_t)WM_DEC_MAXB ? (size_t)WM_DEC_MAXB : g));
}
// ... of an aligned call with N rows per window (wm_transcribe_mel_best_of_aligned, wm_transcribe_mel_beam_aligned), in WINDOWS:
// a window captures N rows, and above 1 keeps the chosen hypothesis' gathered queries and its slot table beside them; the
// statistics, the cost matrix and the DTW are the window's.  N = 1: wm_align_group_rows.
inline size_t wm_align_window_bytes(size_t T, size_t J, size_t n_ld, size_t N) {
    return wm_align_chunk_bytes(T, J, n_ld) + (N > 1 ? (N * T * J * 64 + T) * 4 : 0);
}
inline int wm_align_group_windows(size_t T, size_t J, size_t n_ld, size_t N) {
    const size_t g = WM_ALIGN_CAPTURE_BUDGET / wm_align_window_bytes(T, J, n_ld, N), c_max = (size_t)WM_DEC_MAXB / N;
    return (int)(g < 1 ? 1 : (g > c_max ? c_max : g));
}
// q_sel[c][t][j][0 .. 64) = cap[c * N + slot[c * Tq + t]][t][j][.] for t < n_rows[c] (cap [C * N][Tq][J][64], q_sel [C][Tq][J][64],
// slot and n_rows on the device; a slot outside [0, N) is clamped): the chosen hypothesis' queries in the layout of a plain
// aligned group of C rows
int wm_align_gather(wm_ctx *ctx, const float *cap, float *q_sel, const int *slot, const int *n_rows, int C, int N, int Tq, int J);
// the alignment heads of a context: wm_set_alignment_heads' list, or openai-whisper's default (every head of the last half of
// the decoder layers), ascending by (layer, head)
void wm_align_heads(const WmModel *m, std::vector<int32_t> *hl, std::vector<int32_t> *hh);
int wm_align_matrix(wm_ctx *ctx, const WmAlignDev &a, int max_n, int max_m);
// trace words a chunk of max_rows rows needs in HBM (when its trace does not fit the DTW kernel's LDS)
size_t wm_dtw_trace_words(int max_rows);
// DTW of x[b] (N[b] x M[b], row stride ld, chunk stride x_bstride) -> start[b][0 .. n_out): the first frame of every row on
// the path, -1 past N[b] (dtw.h).  trace: B * wm_dtw_trace_words(max_rows) words of HBM (used when the LDS is too small).
int wm_dtw(wm_ctx *ctx, const float *x, long x_bstride, int ld, const int *N, const int *M, int B, int max_rows, int max_m,
           unsigned *trace, int *start, int n_out);
