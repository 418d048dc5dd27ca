// model.cpp -- weights registry, HBM buffers and the launch sequences of the encoder
// (openai-whisper AudioEncoder.forward, traced at whisper_to_cml.py:10-23), the
// cross-attention K/V projection, and one KV-cached decoder position
// (TextDecoder.forward, traced at whisper_to_cml.py:25-43).
#include "model.h"
#include "tx_plan.h"   // wm_panel_slices, wm_prompt_panel_plan

#include <math.h>
#include <cmath>
#include <string.h>

static inline bf16_t host_f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}
static inline float host_bf2f(bf16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static int dalloc(WmModel *m, void **p, size_t bytes, hipStream_t s) {
    bytes = (bytes + 255) & ~(size_t)255;
    WM_HIP(hipMalloc(p, bytes + 256));  // + slack: tile loaders may over-read by < 256 B
    WM_HIP(hipMemsetAsync(*p, 0, bytes + 256, s));
    m->allocs.push_back(*p);
    return WM_OK;
}
template <typename T>
static int dalloc_t(WmModel *m, T **p, size_t n, hipStream_t s) {
    return dalloc(m, (void **)p, n * sizeof(T), s);
}

static void reg(WmModel *m, const std::string &name, void *ptr, bool is_bf16, size_t n, int kind,
                int layout = WL_PLAIN, int conv_c = 0, int kpad = 0) {
    WmTensor t;
    t.name = name; t.ptr = ptr; t.is_bf16 = is_bf16; t.n_elems = n; t.kind = kind;
    t.layout = layout; t.conv_c = conv_c; t.conv_kpad = kpad;
    m->index[name] = (int)m->tensors.size();
    m->tensors.push_back(t);
}

static int alloc_decode_buffers(WmModel *m, hipStream_t s) {
    const wm_dims &D = m->dims;
    const int d = D.n_text_state;
    // decode-step buffers (batch <= WM_DEC_MAXB)
    WM_TRY(dalloc_t(m, &m->dx, (size_t)WM_DEC_MAXB * d, s));
    WM_TRY(dalloc_t(m, &m->dxb, (size_t)WM_DEC_MAXB * d, s));
    WM_TRY(dalloc_t(m, &m->dmean, (size_t)2 * WM_DEC_MAXB, s));
    WM_TRY(dalloc_t(m, &m->dq, (size_t)WM_DEC_MAXB * d, s));
    WM_TRY(dalloc_t(m, &m->dpart, (size_t)WM_DEC_MAXB * D.n_text_head * WM_MAXSPLIT * 66, s));
    WM_TRY(dalloc_t(m, &m->datt, (size_t)WM_DEC_MAXB * d, s));
    WM_TRY(dalloc_t(m, &m->dstats, (size_t)(WM_DEC_MAXB / 16) * (d / 16) * 16 * 2, s));
    WM_TRY(dalloc_t(m, &m->dhid, (size_t)WM_DEC_MAXB * 4 * d, s));
    WM_TRY(dalloc_t(m, &m->dlogits, (size_t)WM_DEC_MAXB * m->vpad, s));
    WM_TRY(dalloc_t(m, &m->dargmax, (size_t)WM_DEC_MAXB * (m->vpad / 16), s));
    WM_TRY(dalloc_t(m, &m->dresult, WM_DEC_MAXB, s));
    WM_TRY(dalloc_t(m, &m->dseq, (size_t)WM_DEC_MAXB * (D.n_text_ctx + 1), s));
    WM_TRY(dalloc_t(m, &m->dpos, 4, s));
    WM_TRY(dalloc_t(m, &m->doff, WM_DEC_MAXB, s));
    WM_TRY(dalloc_t(m, &m->darrive, 4, s));
    WM_TRY(dalloc_t(m, &m->ddone, WM_DEC_MAXB, s));
    WM_TRY(dalloc_t(m, &m->dbudget, WM_DEC_MAXB, s));
    WM_TRY(dalloc_t(m, &m->dlive, WM_DEC_MAXB + 4, s));   // [live rows | n_live]: ONE pointer argument for the attention
    m->dnlive = m->dlive + WM_DEC_MAXB;                  // kernels (their first loads need everything in 14 dwords)
    if (!m->h_nlive) WM_HIP(hipHostMalloc((void **)&m->h_nlive, WM_NLIVE_RING * sizeof(int), hipHostMallocDefault));
    WM_TRY(dalloc_t(m, &m->dts_rng, (size_t)WM_DEC_MAXB * 4, s));
    WM_TRY(dalloc_t(m, &m->dts_hist, (size_t)WM_DEC_MAXB * 4, s));
    WM_TRY(dalloc_t(m, &m->dts_key, (size_t)WM_DEC_MAXB * (m->vpad / 16), s));
    WM_TRY(dalloc_t(m, &m->dts_lse, (size_t)WM_DEC_MAXB * (m->vpad / 16) * 2, s));
    const size_t tiles = (size_t)WM_DEC_MAXB * (m->vpad / 16);
    WM_TRY(dalloc_t(m, &m->dx_txt, tiles * 2, s));
    WM_TRY(dalloc_t(m, &m->dx_win, tiles * 2, s));
    WM_TRY(dalloc_t(m, &m->dx_all, tiles * 2, s));
    WM_TRY(dalloc_t(m, &m->dx_nsv, WM_DEC_MAXB, s));
    WM_TRY(dalloc_t(m, &m->dx_logprob, (size_t)D.n_text_ctx * WM_DEC_MAXB, s));
    WM_TRY(dalloc_t(m, &m->dx_nospeech, WM_DEC_MAXB, s));
    WM_TRY(dalloc(m, (void **)&m->dx_par, sizeof(WmXPar), s));
    WM_TRY(dalloc(m, (void **)&m->dsamp_par, sizeof(WmSampPar), s));
    WM_TRY(dalloc(m, (void **)&m->dalt_par, sizeof(WmAltPar), s));
    WM_TRY(dalloc(m, (void **)&m->dgiven_par, sizeof(WmGivenPar), s));
    // (+16: the epilogue's padded 16-row blocks; second half: the rows' candidate words, WM_XIDS_CAND)
    WM_TRY(dalloc_t(m, &m->dx_ids, (size_t)WM_XIDS_WORDS, s));   // (third part: the sampling rows, WM_XIDS_ROWS)
    WM_TRY(dalloc_t(m, &m->dmel_win, (size_t)WM_DEC_MAXB, s));
    WM_TRY(dalloc_t(m, &m->dxkv_rows, (size_t)WM_DEC_MAXB, s));
    WM_TRY(dalloc_t(m, &m->dmask, (size_t)2 * (m->vpad / 32), s));
    WM_HIP(hipMemsetAsync(m->dmask, 0, (size_t)2 * (m->vpad / 32) * 4, s));
    return WM_OK;
}

static int alloc_repetition_state(WmModel *m, hipStream_t s) {
    const size_t words = (size_t)WM_DEC_MAXB * ((m->vpad + 31) / 32);
    WM_TRY(dalloc_t(m, &m->drep_seen, words, s));
    WM_TRY(dalloc_t(m, &m->drep_ban, words, s));
    WM_TRY(dalloc(m, (void **)&m->drep_par, sizeof(WmRepPar), s));
    return WM_OK;
}

// the sequence-bias state at FULL capacity (WM_MAX_BIAS_ENTRIES entries, WM_DEC_MAXB rows), once
static int alloc_seqbias_state(WmModel *m, hipStream_t s) {
    const size_t cap = WM_MAX_BIAS_ENTRIES, words = (size_t)(m->vpad + 31) / 32;
    int *grp_id, *grp_beg, *ent_len, *ent_ctx;
    float *ent_bias;
    WM_TRY(dalloc_t(m, &grp_id, cap, s));
    WM_TRY(dalloc_t(m, &grp_beg, cap + 1, s));
    WM_TRY(dalloc_t(m, &ent_len, cap, s));
    WM_TRY(dalloc_t(m, &ent_bias, cap, s));
    WM_TRY(dalloc_t(m, &ent_ctx, cap * WM_SB_CTX, s));
    WM_TRY(dalloc_t(m, &m->dsb.e.hit, (size_t)WM_DEC_MAXB * words, s));
    WM_TRY(dalloc_t(m, &m->dsb.e.cnt, (size_t)WM_DEC_MAXB, s));
    WM_TRY(dalloc_t(m, &m->dsb.e.lid, (size_t)WM_DEC_MAXB * cap, s));
    WM_TRY(dalloc_t(m, &m->dsb.e.ltot, (size_t)WM_DEC_MAXB * cap, s));
    WM_TRY(dalloc_t(m, &m->dsb.e.woff, (size_t)WM_DEC_MAXB * words, s));
    WmSbPar *par;
    WM_TRY(dalloc(m, (void **)&par, sizeof(WmSbPar), s));
    m->dsb.grp_id = grp_id; m->dsb.grp_beg = grp_beg; m->dsb.ent_len = ent_len; m->dsb.ent_bias = ent_bias; m->dsb.ent_ctx = ent_ctx;
    m->dsb.e.words = (int)words;
    m->dsb.par = par;   // last: non-null = allocated
    return WM_OK;
}

// the pool of the row tables at FULL capacity (WM_MAX_BIAS_POOL entries) and the per-row group ranges, once; the per-row state the
// epilogue reads is the single table's (alloc_seqbias_state)
static int alloc_seqbias_pool(WmModel *m, hipStream_t s) {
    const size_t cap = WM_MAX_BIAS_POOL;
    int *grp_id, *grp_beg, *ent_len, *ent_ctx;
    float *ent_bias;
    WM_TRY(dalloc_t(m, &grp_id, cap, s));
    WM_TRY(dalloc_t(m, &grp_beg, cap + 1, s));
    WM_TRY(dalloc_t(m, &ent_len, cap, s));
    WM_TRY(dalloc_t(m, &ent_bias, cap, s));
    WM_TRY(dalloc_t(m, &ent_ctx, cap * WM_SB_CTX, s));
    WM_TRY(dalloc_t(m, &m->dsb_rng, (size_t)WM_DEC_MAXB * 2, s));
    m->dsbt.ent_len = ent_len; m->dsbt.ent_bias = ent_bias; m->dsbt.ent_ctx = ent_ctx; m->dsbt.grp_beg = grp_beg;
    m->dsbt.e = m->dsb.e;
    m->dsbt.grp_id = grp_id;   // last: non-null = allocated
    return WM_OK;
}

// the constraint's tables at FULL capacity (WM_MAX_CST_STATES states, WM_MAX_CST_EDGES edges, the hash) and the rows' starts, once
static int alloc_constraint_state(WmModel *m, hipStream_t s) {
    int *edge_beg, *edge_tok, *edge_next, *def_next, *accept, *hash, *start;
    WM_TRY(dalloc_t(m, &edge_beg, (size_t)WM_MAX_CST_STATES + 1, s));
    WM_TRY(dalloc_t(m, &edge_tok, (size_t)WM_MAX_CST_EDGES, s));
    WM_TRY(dalloc_t(m, &edge_next, (size_t)WM_MAX_CST_EDGES, s));
    WM_TRY(dalloc_t(m, &def_next, (size_t)WM_MAX_CST_STATES, s));
    WM_TRY(dalloc_t(m, &accept, (size_t)WM_MAX_CST_STATES, s));
    WM_TRY(dalloc_t(m, &hash, (size_t)2 * WM_CST_HASH_SLOTS, s));
    WM_TRY(dalloc_t(m, &start, (size_t)WM_DEC_MAXB, s));
    WmCstPar *par;
    WM_TRY(dalloc(m, (void **)&par, sizeof(WmCstPar), s));
    m->dcst.edge_beg = edge_beg; m->dcst.edge_tok = edge_tok; m->dcst.edge_next = edge_next; m->dcst.def_next = def_next;
    m->dcst.accept = accept; m->dcst.hash = hash; m->dcst.start = start;
    m->dcst.par = par;   // last: non-null = allocated
    return WM_OK;
}

// an automaton's arrays (host or another context's device tables) -> this context's tables
static int upload_constraint(WmModel *m, const WmCstDev &from, int ns, int ne, hipMemcpyKind kind, hipStream_t s) {
    WM_HIP(hipMemcpyAsync((void *)m->dcst.edge_beg, from.edge_beg, (size_t)(ns + 1) * 4, kind, s));
    if (ne) {
        WM_HIP(hipMemcpyAsync((void *)m->dcst.edge_tok, from.edge_tok, (size_t)ne * 4, kind, s));
        WM_HIP(hipMemcpyAsync((void *)m->dcst.edge_next, from.edge_next, (size_t)ne * 4, kind, s));
    }
    WM_HIP(hipMemcpyAsync((void *)m->dcst.def_next, from.def_next, (size_t)ns * 4, kind, s));
    WM_HIP(hipMemcpyAsync((void *)m->dcst.accept, from.accept, (size_t)ns * 4, kind, s));
    WM_HIP(hipMemcpyAsync((void *)m->dcst.hash, from.hash, (size_t)2 * WM_CST_HASH_SLOTS * 4, kind, s));
    return WM_OK;
}

WmStopDev wm_model_stop_dev(const WmModel *m, const WmDecodeMode &mode) {
    WmStopDev t;
    memset(&t, 0, sizeof(t));
    if (!mode.stop) return t;
    t.done = m->ddone; t.budget = mode.budget ? m->dbudget : nullptr; t.live_rows = m->dlive; t.n_live = m->dnlive;
    t.eot = mode.stop_eot;
    t.pad_tok = mode.stop_eot >= 0 ? mode.stop_eot : 0;   // what a finished row keeps embedding: any valid id
    return t;
}

WmEmbedDev wm_model_embed_dev(const WmModel *m) {
    return WmEmbedDev{m->tok_emb, m->dec_pos, m->dims.n_text_state, m->dx, m->dxb, m->dstats, m->dmean};
}

WmXDev wm_model_x_dev(const WmModel *m, const WmDecodeMode &mode) {
    WmXDev t;
    memset(&t, 0, sizeof(t));
    if (!mode.x) return t;
    t.par = m->dx_par; t.txt = m->dx_txt; t.win = m->dx_win; t.all = m->dx_all; t.ns_v = m->dx_nsv;
    t.logprob = m->dx_logprob; t.nospeech = m->dx_nospeech; t.ids = m->dx_ids;
    return t;
}

// ------------------------------------------------------------------ beam search state ----
namespace {
// beam_ws: [WmBeamPar | per-row and per-window state | fin_tok | fin_lp | fin_src | anc], sized for WM_DEC_MAXB rows and as many
// windows (the ancestry record behind everything a plain beam group touches or fetches)
struct BeamLayout {
    size_t par, budget, sum, src, list_n, list_tok, list_lp, wdone, wsteps, fin_n, fin_len, fin_sum, fin_tok, fin_lp, fin_src, anc, end;
    explicit BeamLayout(int n_ctx) {
        size_t o = 0;
        auto take = [&](size_t words) { const size_t at = o; o += (words * 4 + 255) & ~(size_t)255; return at; };
        const size_t R = WM_DEC_MAXB;
        par = take(sizeof(WmBeamPar) / 4); budget = take(R); sum = take(R); src = take(R); list_n = take(R);
        list_tok = take(R * (WM_MAX_BEAM + 1)); list_lp = take(R * (WM_MAX_BEAM + 1));
        wdone = take(R); wsteps = take(R); fin_n = take(R); fin_len = take(R * WM_MAX_BEAM_HYPS); fin_sum = take(R * WM_MAX_BEAM_HYPS);
        fin_tok = take(R * WM_MAX_BEAM_HYPS * n_ctx); fin_lp = take(R * WM_MAX_BEAM_HYPS * n_ctx);
        fin_src = take(R * WM_MAX_BEAM_HYPS); anc = take(R * n_ctx);
        end = o;
    }
};
}  // namespace

size_t wm_model_beam_state_bytes(const WmModel *m) { return BeamLayout(m->dims.n_text_ctx).fin_tok; }

int wm_model_beam_dev(wm_ctx *ctx, const WmDecodeMode &mode, WmBeamDev *out) {
    WmModel *m = ctx->model;
    const BeamLayout L(m->dims.n_text_ctx);
    if (!m->beam_ws.p) {   // (allocated once: the captured graphs hold these addresses)
        WM_TRY(m->beam_ws.reserve(ctx->stream, L.end));
        WM_HIP(hipMemsetAsync(m->beam_ws.p, 0, L.end, ctx->stream));
    }
    char *p = (char *)m->beam_ws.p;
    WmBeamDev d;
    memset(&d, 0, sizeof(d));
    d.par = (const WmBeamPar *)(p + L.par); d.N = mode.beam; d.n_ctx = m->dims.n_text_ctx;
    d.budget = (const int *)(p + L.budget); d.sum = (float *)(p + L.sum); d.src = (int *)(p + L.src);
    d.list_n = (int *)(p + L.list_n); d.list_tok = (int *)(p + L.list_tok); d.list_lp = (float *)(p + L.list_lp);
    d.wdone = (int *)(p + L.wdone); d.wsteps = (int *)(p + L.wsteps); d.fin_n = (int *)(p + L.fin_n);
    d.fin_len = (int *)(p + L.fin_len); d.fin_sum = (float *)(p + L.fin_sum);
    d.fin_tok = (int *)(p + L.fin_tok); d.fin_lp = (float *)(p + L.fin_lp);
    d.trace = m->beam_trace_on ? (float *)m->beam_trace.p : nullptr;   // (the debug library asked for this call's trace)
    if (mode.acap) { d.fin_src = (int *)(p + L.fin_src); d.anc = (int *)(p + L.anc); }   // an aligned group records its ancestry
    *out = d;
    return WM_OK;
}

int wm_model_beam_begin(wm_ctx *ctx, const WmDecodeMode &mode, int rows, int windows, const WmBeamPar *par, const int32_t *budgets) {
    WmModel *m = ctx->model;
    WM_REQUIRE(mode.beam >= 1 && mode.beam <= WM_MAX_BEAM && rows == windows * mode.beam && rows <= WM_DEC_MAXB, WM_ERR_INVALID,
               "beam group: %d rows are not %d windows x %d beams", rows, windows, mode.beam);
    WmBeamDev d;
    WM_TRY(wm_model_beam_dev(ctx, mode, &d));
    const BeamLayout L(m->dims.n_text_ctx);
    char *p = (char *)m->beam_ws.p;
    // sums 0, sources / lists / flags / counts 0: everything between the budgets and the finished records
    WM_HIP(hipMemsetAsync(p + L.sum, 0, L.fin_len - L.sum, ctx->stream));
    WM_HIP(hipMemcpyAsync(p + L.par, par, sizeof(WmBeamPar), hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipMemcpyAsync(p + L.budget, budgets, (size_t)windows * 4, hipMemcpyHostToDevice, ctx->stream));
    return WM_OK;
}

// The group's B rows as the kernels between the logits launch and the close see them (the device views of a mode that is off are
// empty: wm_model_stop_dev, wm_model_x_dev, wm_model_rep_dev).
static WmStoredRows wm_model_stored_rows(const WmModel *m, int B, int n_prompt, const WmDecodeMode &mode) {
    const WmRepDev rp = wm_model_rep_dev(m, mode);
    WmStoredRows r;
    r.logits = m->dlogits; r.ldo = m->vpad; r.n_vocab = m->dims.n_vocab; r.tilemax = m->dargmax; r.rows = B;
    r.ts = mode.ts ? wm_model_ts_dev(m) : WmTsDev{};
    r.xd = wm_model_x_dev(m, mode);
    r.mask = mode.mask ? m->dmask : nullptr; r.mask_words = m->vpad / 32;
    r.n_prompt = n_prompt; r.pos_ptr = m->dpos;
    r.stop = wm_model_stop_dev(m, mode);
    r.ban = rp.par ? rp.ban : nullptr; r.ban_words = rp.words;
    return r;
}

int wm_model_beam_close(wm_ctx *ctx, int B, int n_prompt, const WmDecodeMode &mode) {
    WmModel *m = ctx->model;
    const wm_dims &D = m->dims;
    WmBeamDev bm;
    WM_TRY(wm_model_beam_dev(ctx, mode, &bm));
    const WmStoredRows r = wm_model_stored_rows(m, B, n_prompt, mode);
    WM_REQUIRE(r.xd.par, WM_ERR_STATE, "beam close: the extended decode is off");
    WM_TRY(wm_beam_topk(ctx, r, bm));
    WM_TRY(wm_beam_select_step(ctx, B, m->dseq, m->dpos, n_prompt, wm_model_embed_dev(m), r.ts, r.stop, r.xd, mode.off ? m->doff : nullptr, bm));
    return wm_beam_reorder(ctx, m->skv, D.n_text_layer * 2, B, D.n_text_head, D.n_text_ctx, m->dpos, n_prompt, m->dseq,
                           m->dx_logprob, bm);
}

void wm_model_drop_graphs(WmModel *m) {
    for (WmModel::GraphSet &g : m->graph_sets) g.destroy();
    m->graph_sets.clear();
    m->lid_graph.destroy();
}

WmRepDev wm_model_rep_dev(const WmModel *m, const WmDecodeMode &mode) {
    WmRepDev t;
    memset(&t, 0, sizeof(t));
    if (!mode.rep) return t;
    t.par = m->drep_par; t.seen = m->drep_seen; t.ban = m->drep_ban; t.words = (m->vpad + 31) / 32;
    return t;
}

WmSbDev wm_model_sb_dev(const WmModel *m, const WmDecodeMode &mode) {
    WmSbDev t;
    memset(&t, 0, sizeof(t));
    if (!mode.sb) return t;
    return mode.sbt ? m->dsbt : m->dsb;   // (row tables: the pool; par is null, the rows' ranges are m->dsb_rng)
}

// the bitmaps and the parameter block, once (captured graphs hold these addresses)
static int alloc_repetition_state(WmModel *m, hipStream_t s);

int wm_model_set_sequence_bias(wm_ctx *ctx, const WmSbTable &t) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    const int ng = t.n_groups(), ne = t.n_entries();
    WM_REQUIRE(ne <= WM_MAX_BIAS_ENTRIES && ng <= ne && (int)t.grp_beg.size() == (ne ? ng + 1 : 0) && (int)t.ent_bias.size() == ne &&
                   t.ent_ctx.size() == (size_t)ne * WM_SB_CTX,
               WM_ERR_INVALID, "sequence bias: malformed table");
    if (ne) {
        WM_REQUIRE(!ctx->dbg_hooks, WM_ERR_STATE, "the sequence bias is not supported by the all-f32 precision path");
        WM_REQUIRE(((size_t)3 * ((m->vpad + 31) / 32) + WM_MAX_BIAS_ENTRIES + 512) * 4 <= 64 * 1024 && (m->vpad + 31) / 32 <= 2048, WM_ERR_INVALID,
                   "sequence bias: a vocabulary of %d ids does not fit the state kernel's LDS", m->dims.n_vocab);
        // the bitmaps are wm_repeat_state's: a group with the bias on runs it too (with (1.0, 0) when the repetition rules are off)
        if (!m->drep_par) WM_TRY(alloc_repetition_state(m, ctx->stream));
        if (!m->dsb.par) WM_TRY(alloc_seqbias_state(m, ctx->stream));
        hipStream_t s = ctx->stream;
        WM_HIP(hipMemcpyAsync((void *)m->dsb.grp_id, t.grp_id.data(), (size_t)ng * 4, hipMemcpyHostToDevice, s));
        WM_HIP(hipMemcpyAsync((void *)m->dsb.grp_beg, t.grp_beg.data(), (size_t)(ng + 1) * 4, hipMemcpyHostToDevice, s));
        WM_HIP(hipMemcpyAsync((void *)m->dsb.ent_len, t.ent_len.data(), (size_t)ne * 4, hipMemcpyHostToDevice, s));
        WM_HIP(hipMemcpyAsync((void *)m->dsb.ent_bias, t.ent_bias.data(), (size_t)ne * 4, hipMemcpyHostToDevice, s));
        WM_HIP(hipMemcpyAsync((void *)m->dsb.ent_ctx, t.ent_ctx.data(), (size_t)ne * WM_SB_CTX * 4, hipMemcpyHostToDevice, s));
        WM_HIP(hipStreamSynchronize(s));   // (the table's vectors are the caller's)
    }
    m->sb_on = ne > 0; m->sb_groups = ng; m->sb_entries = ne;
    // exclusive with the row tables: a table replaces them, the empty table clears both
    m->sbt_on = false; m->sbt_groups = m->sbt_entries = 0; m->sbt_tab_grp.clear();
    m->pending.bias_rows.clear();
    return WM_OK;
}

int wm_model_set_constraint(wm_ctx *ctx, const WmCstTable &t) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    const int ns = t.n_states(), ne = t.n_edges();
    WM_REQUIRE(ns <= WM_MAX_CST_STATES && ne <= WM_MAX_CST_EDGES && (int)t.edge_beg.size() == (ns ? ns + 1 : 0) && (int)t.edge_next.size() == ne &&
                   (int)t.accept.size() == ns && t.hash.size() == (ns ? (size_t)2 * WM_CST_HASH_SLOTS : 0),
               WM_ERR_INVALID, "constraint: malformed table");
    if (ns) {
        WM_REQUIRE(!ctx->dbg_hooks, WM_ERR_STATE, "the constraint is not supported by the all-f32 precision path");
        WM_REQUIRE(t.eot >= 0 && t.eot < m->dims.n_vocab, WM_ERR_INVALID, "constraint: eot %d outside [0, %d)", t.eot, m->dims.n_vocab);
        WM_REQUIRE(((size_t)2 * ((m->vpad + 31) / 32) + m->dims.n_text_ctx + 1) * 4 <= 64 * 1024, WM_ERR_INVALID,
                   "constraint: a vocabulary of %d ids does not fit the state kernels' LDS", m->dims.n_vocab);
        // the ban words are wm_repeat_state's: a group with the constraint on runs it too (with (1.0, 0) when the repetition rules are off)
        if (!m->drep_par) WM_TRY(alloc_repetition_state(m, ctx->stream));
        if (!m->dcst.par) WM_TRY(alloc_constraint_state(m, ctx->stream));
        WmCstDev from;
        memset(&from, 0, sizeof(from));
        from.edge_beg = t.edge_beg.data(); from.edge_tok = t.edge_tok.data(); from.edge_next = t.edge_next.data();
        from.def_next = t.def_next.data(); from.accept = t.accept.data(); from.hash = t.hash.data();
        WM_TRY(upload_constraint(m, from, ns, ne, hipMemcpyHostToDevice, ctx->stream));
        WM_HIP(hipStreamSynchronize(ctx->stream));   // (the table's vectors are the caller's)
    }
    m->cst_on = ns > 0; m->cst_states = ns; m->cst_edges = ne; m->cst_eot = ns ? t.eot : 0;
    m->pending.cst_rows.clear();
    return WM_OK;
}

static int upload_seqbias_pool(WmModel *m, const WmSbDev &from, int ng, int ne, hipMemcpyKind kind, hipStream_t s) {
    WM_HIP(hipMemcpyAsync((void *)m->dsbt.grp_beg, from.grp_beg, (size_t)(ng + 1) * 4, kind, s));
    if (ng) WM_HIP(hipMemcpyAsync((void *)m->dsbt.grp_id, from.grp_id, (size_t)ng * 4, kind, s));
    if (ne) {
        WM_HIP(hipMemcpyAsync((void *)m->dsbt.ent_len, from.ent_len, (size_t)ne * 4, kind, s));
        WM_HIP(hipMemcpyAsync((void *)m->dsbt.ent_bias, from.ent_bias, (size_t)ne * 4, kind, s));
        WM_HIP(hipMemcpyAsync((void *)m->dsbt.ent_ctx, from.ent_ctx, (size_t)ne * WM_SB_CTX * 4, kind, s));
    }
    return WM_OK;
}

// One lane's tables.  "A refused call leaves whatever was in force" is about the ARGUMENTS: they are checked and expanded once
// (wm_sb_expand_tables) before any lane is touched.  A device failure in here -- the pool's one allocation, a copy -- on lane k
// leaves the lanes in front with the new pool and the others with the old state, as wm_model_set_sequence_bias does for its
// table; the caller sets the tables again (or clears them) after such a WM_ERR_HIP / WM_ERR_NOMEM.
int wm_model_set_sequence_bias_tables(wm_ctx *ctx, const WmSbPool &p) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    const int nt = p.n_tables(), ng = p.t.n_groups(), ne = p.t.n_entries();
    WM_REQUIRE(nt <= WM_MAX_BIAS_TABLES && ne <= WM_MAX_BIAS_POOL && ng <= ne && (nt == 0 || (int)p.t.grp_beg.size() == ng + 1) &&
                   (int)p.t.ent_bias.size() == ne && p.t.ent_ctx.size() == (size_t)ne * WM_SB_CTX && (nt == 0 || p.tab_grp.back() == ng),
               WM_ERR_INVALID, "sequence bias tables: malformed pool");
    if (nt) {
        WM_REQUIRE(!ctx->dbg_hooks, WM_ERR_STATE, "the sequence bias is not supported by the all-f32 precision path");
        WM_REQUIRE(((size_t)3 * ((m->vpad + 31) / 32) + WM_MAX_BIAS_ENTRIES + 512) * 4 <= 64 * 1024 && (m->vpad + 31) / 32 <= 2048, WM_ERR_INVALID,
                   "sequence bias: a vocabulary of %d ids does not fit the state kernel's LDS", m->dims.n_vocab);
        if (!m->drep_par) WM_TRY(alloc_repetition_state(m, ctx->stream));
        if (!m->dsb.par) WM_TRY(alloc_seqbias_state(m, ctx->stream));
        if (!m->dsbt.grp_id) WM_TRY(alloc_seqbias_pool(m, ctx->stream));
        WmSbDev from;
        memset(&from, 0, sizeof(from));
        from.grp_id = p.t.grp_id.data(); from.grp_beg = p.t.grp_beg.data(); from.ent_len = p.t.ent_len.data();
        from.ent_bias = p.t.ent_bias.data(); from.ent_ctx = p.t.ent_ctx.data();
        WM_TRY(upload_seqbias_pool(m, from, ng, ne, hipMemcpyHostToDevice, ctx->stream));
        WM_HIP(hipStreamSynchronize(ctx->stream));   // (the pool's vectors are the caller's)
        m->sb_on = false; m->sb_groups = m->sb_entries = 0;   // replaces the single table
    }
    m->sbt_on = nt > 0; m->sbt_groups = ng; m->sbt_entries = ne;
    m->sbt_tab_grp = p.tab_grp;
    m->pending.bias_rows.clear();
    return WM_OK;
}

int wm_model_set_repetition_rules(wm_ctx *ctx, float penalty, int ngram, int32_t eot) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    WM_REQUIRE(std::isfinite(penalty) && penalty > 0.f, WM_ERR_INVALID, "repetition rules: the penalty must be finite and > 0 (1.0: off)");
    // (1 / p is the multiplier of a positive logit: it must be a finite f32 as well)
    WM_REQUIRE(std::isfinite((float)(1.0 / (double)penalty)), WM_ERR_INVALID, "repetition rules: penalty %g is too small: 1 / p overflows",
               (double)penalty);
    WM_REQUIRE(ngram >= 0 && ngram <= WM_MAX_NGRAM, WM_ERR_INVALID, "repetition rules: no_repeat_ngram_size %d outside [0, %d]", ngram,
               WM_MAX_NGRAM);
    WM_REQUIRE(eot >= 0 && eot <= m->dims.n_vocab, WM_ERR_INVALID, "repetition rules: eot %d outside [0, %d]", eot, m->dims.n_vocab);
    const bool on = penalty != 1.f || ngram != 0;
    if (on) {
        WM_REQUIRE(!ctx->dbg_hooks, WM_ERR_STATE, "the repetition rules are not supported by the all-f32 precision path");
        WM_REQUIRE(((size_t)2 * ((m->vpad + 31) / 32) + m->dims.n_text_ctx) * 4 <= 64 * 1024, WM_ERR_INVALID,
                   "repetition rules: a vocabulary of %d ids does not fit the state kernel's LDS", m->dims.n_vocab);
        if (!m->drep_par) WM_TRY(alloc_repetition_state(m, ctx->stream));
    }
    m->rep_on = on; m->rep_p = penalty; m->rep_n = ngram; m->rep_eot = eot;
    return WM_OK;
}

int wm_model_set_sampling_rules(wm_ctx *ctx, int top_k, float top_p, float min_p) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    const bool on = top_k > 0 || top_p < 1.f || min_p > 0.f;
    if (on) {
        WM_REQUIRE(!ctx->dbg_hooks, WM_ERR_STATE, "the sampling rules are not supported by the all-f32 precision path");
        WM_REQUIRE(m->dims.n_vocab <= 64 * 2048, WM_ERR_INVALID, "sampling rules: a vocabulary of %d ids does not fit the truncation kernel",
                   m->dims.n_vocab);
    }
    m->samp_k = top_k; m->samp_p = top_p; m->samp_minp = min_p;
    return WM_OK;
}

int wm_model_sample_truncate(wm_ctx *ctx, int B, int n_prompt, const WmDecodeMode &mode) {
    WmModel *m = ctx->model;
    WM_REQUIRE(mode.trunc && mode.x && !mode.beam && mode.panel <= 1, WM_ERR_STATE, "sampling rules: a sampling extended-decode group");
    return wm_sample_truncate(ctx, wm_model_stored_rows(m, B, n_prompt, mode), m->dsamp_par, nullptr);
}

int wm_model_alt_begin(wm_ctx *ctx, int rows, int max_new, int n, WmAltPar *host_par) {
    WmModel *m = ctx->model;
    WM_REQUIRE(rows >= 1 && rows <= WM_DEC_MAXB && max_new >= 1 && n >= 1 && n <= WM_MAX_ALTERNATIVES, WM_ERR_INVALID,
               "alternatives: %d rows x %d positions x %d entries", rows, max_new, n);
    const size_t pos = (size_t)max_new * rows, list = (pos * n * 4 + 255) & ~(size_t)255, one = (pos * 4 + 255) & ~(size_t)255;
    WM_TRY(m->alt_ws.reserve(ctx->stream, 2 * list + 2 * one));
    char *p = (char *)m->alt_ws.p;
    host_par->n = n; host_par->max_new = max_new;
    host_par->tok = (int *)p; host_par->lp = (float *)(p + list);
    host_par->cnt = (int *)(p + 2 * list); host_par->ent = (float *)(p + 2 * list + one);
    // the pads: id -1 (0xff bytes), log-prob 0, count 0, entropy 0 -- what a position no workgroup writes keeps
    WM_HIP(hipMemsetAsync(p, 0xff, list, ctx->stream));
    WM_HIP(hipMemsetAsync(p + list, 0, list + 2 * one, ctx->stream));
    WM_HIP(hipMemcpyAsync(m->dalt_par, host_par, sizeof(WmAltPar), hipMemcpyHostToDevice, ctx->stream));
    return WM_OK;
}

int wm_model_alternatives(wm_ctx *ctx, int B, int n_prompt, const WmDecodeMode &mode) {
    WmModel *m = ctx->model;
    WM_REQUIRE(mode.alt && mode.x && !mode.beam && mode.panel <= 1, WM_ERR_STATE, "alternatives: an extended-decode group without beams");
    return wm_alternatives(ctx, wm_model_stored_rows(m, B, n_prompt, mode), m->dalt_par);
}

int wm_model_given_begin(wm_ctx *ctx, int rows, int stride, const int32_t *lens, const int32_t *tok, WmGivenPar *host_par) {
    WmModel *m = ctx->model;
    WM_REQUIRE(rows >= 1 && rows <= WM_DEC_MAXB && stride >= 1 && lens && tok, WM_ERR_INVALID, "given tokens: %d rows x %d tokens", rows,
               stride);
    const size_t nl = ((size_t)rows * 4 + 255) & ~(size_t)255, nt = (size_t)rows * stride * 4;
    // (behind the table: the side area of a given-panel phase -- committed history and ranges [R][4] each, the rows' tokens and
    // log-probs [R] each)
    const size_t side = (nl + nt + 255) & ~(size_t)255;
    WM_TRY(m->given_ws.reserve(ctx->stream, side + (size_t)WM_DEC_MAXB * 10 * 4));
    char *p = (char *)m->given_ws.p;
    m->dgiven_side = (int *)(p + side);
    host_par->stride = stride; host_par->lens = (const int *)p; host_par->tok = (const int *)(p + nl);
    WM_HIP(hipMemcpyAsync(p, lens, (size_t)rows * 4, hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipMemcpyAsync(p + nl, tok, nt, hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipMemcpyAsync(m->dgiven_par, host_par, sizeof(WmGivenPar), hipMemcpyHostToDevice, ctx->stream));
    return WM_OK;
}

int wm_model_given_tokens(wm_ctx *ctx, int B, int n_prompt, const WmDecodeMode &mode) {
    WmModel *m = ctx->model;
    WM_REQUIRE(mode.given && mode.x && !mode.beam && mode.panel <= 1, WM_ERR_STATE, "given tokens: an extended-decode group without beams");
    return wm_given_tokens(ctx, wm_model_stored_rows(m, B, n_prompt, mode), m->dgiven_par);
}

WmTsDev wm_model_ts_dev(const WmModel *m) {
    WmTsDev t;
    memset(&t, 0, sizeof(t));
    if (!m->ts_on) return t;
    t.rng = m->dts_rng; t.hist = m->dts_hist; t.key_ts = m->dts_key; t.lse = m->dts_lse;
    t.ts_begin = m->ts_begin; t.eot = m->ts_eot; t.n_vocab = m->dims.n_vocab; t.max_initial = m->ts_max_initial;
    return t;
}

int wm_model_set_timestamp_rules(wm_ctx *ctx, int enable, int32_t ts_begin, int32_t eot, int32_t max_initial) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    if (enable) {
        const int V = m->dims.n_vocab;
        WM_REQUIRE(ts_begin > 0 && ts_begin < V && eot >= 0 && eot < ts_begin, WM_ERR_INVALID,
                   "timestamp rules: need 0 <= eot < timestamp_begin < n_vocab (%d)", V);
        // <|endoftext|> is the token of last resort of the rules (an opening timestamp may be followed by it, and it is
        // what the arg-max kernel falls back to when nothing else is admissible): it must not be suppressed
        if (!m->mask_host.empty())
            WM_REQUIRE(!((m->mask_host[eot >> 5] >> (eot & 31)) & 1u), WM_ERR_INVALID,
                       "timestamp rules: <|endoftext|> (%d) is in the suppress list", eot);
        if (m->ts_begin != ts_begin || m->ts_eot != eot || m->ts_max_initial != max_initial) {
            // these ids are baked into the captured decode graphs' kernel arguments: drop the stale captures
            wm_model_drop_graphs(m);
        }
        m->ts_begin = ts_begin; m->ts_eot = eot; m->ts_max_initial = max_initial;
    }
    m->ts_on = enable != 0;
    return WM_OK;
}

// SuppressTokens / SuppressBlank of openai-whisper's decoding.py as two bitmaps over the vocabulary.
int wm_model_set_suppress(wm_ctx *ctx, const int32_t *ids, int n, const int32_t *first_ids, int n_first) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    WM_REQUIRE(n >= 0 && n_first >= 0 && (n == 0 || ids) && (n_first == 0 || first_ids), WM_ERR_INVALID,
               "set_suppress: bad list");
    const int words = m->vpad / 32, V = m->dims.n_vocab;
    std::vector<unsigned> bits((size_t)2 * words, 0u);
    for (int i = 0; i < n; ++i) {
        WM_REQUIRE(ids[i] >= 0 && ids[i] < V, WM_ERR_INVALID, "set_suppress: token %d outside [0, %d)", ids[i], V);
        bits[ids[i] >> 5] |= 1u << (ids[i] & 31);
    }
    for (int i = 0; i < words; ++i) bits[words + i] = bits[i];  // first position: always-list OR first-list
    for (int i = 0; i < n_first; ++i) {
        WM_REQUIRE(first_ids[i] >= 0 && first_ids[i] < V, WM_ERR_INVALID, "set_suppress: token %d outside [0, %d)",
                   first_ids[i], V);
        bits[words + (first_ids[i] >> 5)] |= 1u << (first_ids[i] & 31);
    }
    size_t live0 = 0, live1 = 0;
    for (int t = 0; t < V; ++t) {
        live0 += !((bits[t >> 5] >> (t & 31)) & 1u);
        live1 += !((bits[words + (t >> 5)] >> (t & 31)) & 1u);
    }
    WM_REQUIRE(live0 > 0 && live1 > 0, WM_ERR_INVALID, "set_suppress: every token would be suppressed");
    if (m->ts_on)
        WM_REQUIRE(!((bits[m->ts_eot >> 5] >> (m->ts_eot & 31)) & 1u), WM_ERR_INVALID,
                   "set_suppress: <|endoftext|> (%d) must stay admissible while the timestamp rules are on", m->ts_eot);
    m->mask_host.assign(bits.begin(), bits.begin() + words);   // the every-position list (timestamp-rule validation)
    WM_HIP(hipMemcpyAsync(m->dmask, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    m->mask_on = (n + n_first) > 0;
    return WM_OK;
}

// kinds mirror weights.py: 0 matrix, 1 bias, 2 LN weight, 3 LN bias, 4 sinusoid
int wm_model_create(wm_ctx *ctx, const wm_dims *dims) {
    const wm_dims &D = *dims;
    WM_REQUIRE(D.n_mels == 80 || D.n_mels == 128, WM_ERR_INVALID, "n_mels must be 80 or 128");
    WM_REQUIRE(D.n_audio_ctx == 1500, WM_ERR_INVALID, "n_audio_ctx must be 1500 (30 s chunks)");
    WM_REQUIRE(D.n_audio_state == D.n_text_state, WM_ERR_INVALID, "audio/text widths must match");
    WM_REQUIRE(D.n_audio_state % 64 == 0 && D.n_audio_state <= 1280 && D.n_audio_state >= 64,
               WM_ERR_INVALID, "model width must be a multiple of 64 in [64, 1280]");
    WM_REQUIRE(D.n_audio_head * 64 == D.n_audio_state && D.n_text_head * 64 == D.n_text_state,
               WM_ERR_INVALID, "head_dim must be 64 (Whisper uses 64 at every size)");
    WM_REQUIRE(D.n_text_ctx >= 8 && D.n_text_ctx <= 448 && D.n_vocab >= 16, WM_ERR_INVALID, "bad text dims");
    WM_REQUIRE(D.n_audio_layer >= 1 && D.n_text_layer >= 1, WM_ERR_INVALID, "bad layer counts");
    WM_REQUIRE(wm_dec_gemv_split(D.n_text_state, nullptr) > 0 && wm_dec_gemv_split(4 * D.n_text_state, nullptr) > 0,
               WM_ERR_INVALID, "model width %d: the decode GEMV cannot split K = d / 4d over its waves", D.n_text_state);
    WmModel *m = new WmModel();
    ctx->model = m;
    m->dims = D;
    const int d = D.n_audio_state;
    hipStream_t s = ctx->stream;
    m->k1pad = ((3 * D.n_mels + 63) / 64) * 64;
    m->vpad = ((D.n_vocab + 15) / 16) * 16;

    WM_TRY(dalloc_t(m, &m->conv1_w, (size_t)d * m->k1pad, s));
    WM_TRY(dalloc_t(m, &m->conv1_b, d, s));
    WM_TRY(dalloc_t(m, &m->conv2_w, (size_t)d * 3 * d, s));
    WM_TRY(dalloc_t(m, &m->conv2_b, d, s));
    WM_TRY(dalloc_t(m, &m->enc_pos, (size_t)D.n_audio_ctx * d, s));
    reg(m, "encoder.conv1.weight", m->conv1_w, true, (size_t)d * D.n_mels * 3, 0, WL_CONV, D.n_mels, m->k1pad);
    reg(m, "encoder.conv1.bias", m->conv1_b, false, d, 1);
    reg(m, "encoder.conv2.weight", m->conv2_w, true, (size_t)d * d * 3, 0, WL_CONV, d, 3 * d);
    reg(m, "encoder.conv2.bias", m->conv2_b, false, d, 1);
    reg(m, "encoder.positional_embedding", m->enc_pos, false, (size_t)D.n_audio_ctx * d, 4);

    // lq / lkv / lo: HBM layout of the query, key+value and out matrices (decode GEMV operands are
    // stored fragment-tiled; GEMM operands row-major)
    auto attn_regs = [&](const std::string &p, bf16_t *wq, float *bq, bf16_t *wk, bf16_t *wv, float *bv,
                         bf16_t *wo, float *bo, float *lg, float *lb, const char *a, int lq, int lkv, int lo) {
        const size_t dd = (size_t)d * d;
        reg(m, p + "." + a + ".query.weight", wq, true, dd, 0, lq, 0, d);
        reg(m, p + "." + a + ".query.bias", bq, false, d, 1);
        reg(m, p + "." + a + ".key.weight", wk, true, dd, 0, lkv, 0, d);
        reg(m, p + "." + a + ".value.weight", wv, true, dd, 0, lkv, 0, d);
        reg(m, p + "." + a + ".value.bias", bv, false, d, 1);
        reg(m, p + "." + a + ".out.weight", wo, true, dd, 0, lo, 0, d);
        reg(m, p + "." + a + ".out.bias", bo, false, d, 1);
        reg(m, p + "." + a + "_ln.weight", lg, false, d, 2);
        reg(m, p + "." + a + "_ln.bias", lb, false, d, 3);
    };
    auto mlp_regs = [&](const std::string &p, bf16_t *w1, float *b1, bf16_t *w2, float *b2, float *lg, float *lb,
                        int lay) {
        reg(m, p + ".mlp.0.weight", w1, true, (size_t)4 * d * d, 0, lay, 0, d);
        reg(m, p + ".mlp.0.bias", b1, false, 4 * d, 1);
        reg(m, p + ".mlp.2.weight", w2, true, (size_t)4 * d * d, 0, lay, 0, 4 * d);
        reg(m, p + ".mlp.2.bias", b2, false, d, 1);
        reg(m, p + ".mlp_ln.weight", lg, false, d, 2);
        reg(m, p + ".mlp_ln.bias", lb, false, d, 3);
    };

    m->enc.resize(D.n_audio_layer);
    for (int i = 0; i < D.n_audio_layer; ++i) {
        EncLayerW &L = m->enc[i];
        WM_TRY(dalloc_t(m, &L.ln1_g, d, s)); WM_TRY(dalloc_t(m, &L.ln1_b, d, s));
        WM_TRY(dalloc_t(m, &L.wqkv, (size_t)3 * d * d, s)); WM_TRY(dalloc_t(m, &L.bqkv, 3 * d, s));
        WM_TRY(dalloc_t(m, &L.wo, (size_t)d * d, s)); WM_TRY(dalloc_t(m, &L.bo, d, s));
        WM_TRY(dalloc_t(m, &L.ln2_g, d, s)); WM_TRY(dalloc_t(m, &L.ln2_b, d, s));
        WM_TRY(dalloc_t(m, &L.w1, (size_t)4 * d * d, s)); WM_TRY(dalloc_t(m, &L.b1, 4 * d, s));
        WM_TRY(dalloc_t(m, &L.w2, (size_t)4 * d * d, s)); WM_TRY(dalloc_t(m, &L.b2, d, s));
        const std::string p = "encoder.blocks." + std::to_string(i);
        attn_regs(p, L.wqkv, L.bqkv, L.wqkv + (size_t)d * d, L.wqkv + (size_t)2 * d * d, L.bqkv + 2 * d, L.wo,
                  L.bo, L.ln1_g, L.ln1_b, "attn", WL_PLAIN, WL_PLAIN, WL_PLAIN);
        mlp_regs(p, L.w1, L.b1, L.w2, L.b2, L.ln2_g, L.ln2_b, WL_PLAIN);
    }
    WM_TRY(dalloc_t(m, &m->ln_post_g, d, s)); WM_TRY(dalloc_t(m, &m->ln_post_b, d, s));
    reg(m, "encoder.ln_post.weight", m->ln_post_g, false, d, 2);
    reg(m, "encoder.ln_post.bias", m->ln_post_b, false, d, 3);

    WM_TRY(dalloc_t(m, &m->tok_emb, (size_t)m->vpad * d, s));
    WM_TRY(dalloc_t(m, &m->dec_pos, (size_t)D.n_text_ctx * d, s));
    reg(m, "decoder.token_embedding.weight", m->tok_emb, true, (size_t)D.n_vocab * d, 0, WL_TILED, 0, d);
    reg(m, "decoder.positional_embedding", m->dec_pos, false, (size_t)D.n_text_ctx * d, 0);
    m->dec.resize(D.n_text_layer);
    for (int i = 0; i < D.n_text_layer; ++i) {
        DecLayerW &L = m->dec[i];
        WM_TRY(dalloc_t(m, &L.ln1_g, d, s)); WM_TRY(dalloc_t(m, &L.ln1_b, d, s));
        WM_TRY(dalloc_t(m, &L.wqkv, (size_t)3 * d * d, s)); WM_TRY(dalloc_t(m, &L.bqkv, 3 * d, s));
        WM_TRY(dalloc_t(m, &L.wo, (size_t)d * d, s)); WM_TRY(dalloc_t(m, &L.bo, d, s));
        WM_TRY(dalloc_t(m, &L.lnx_g, d, s)); WM_TRY(dalloc_t(m, &L.lnx_b, d, s));
        WM_TRY(dalloc_t(m, &L.wxq, (size_t)d * d, s)); WM_TRY(dalloc_t(m, &L.bxq, d, s));
        WM_TRY(dalloc_t(m, &L.wxkv, (size_t)2 * d * d, s)); WM_TRY(dalloc_t(m, &L.bxkv, 2 * d, s));
        WM_TRY(dalloc_t(m, &L.wxo, (size_t)d * d, s)); WM_TRY(dalloc_t(m, &L.bxo, d, s));
        WM_TRY(dalloc_t(m, &L.ln2_g, d, s)); WM_TRY(dalloc_t(m, &L.ln2_b, d, s));
        WM_TRY(dalloc_t(m, &L.w1, (size_t)4 * d * d, s)); WM_TRY(dalloc_t(m, &L.b1, 4 * d, s));
        WM_TRY(dalloc_t(m, &L.w2, (size_t)4 * d * d, s)); WM_TRY(dalloc_t(m, &L.b2, d, s));
        // LayerNorm-folded decode operands (filled by wm_finalize)
        WM_TRY(dalloc_t(m, &L.wqkv_f, (size_t)3 * d * d, s)); WM_TRY(dalloc_t(m, &L.wxq_f, (size_t)d * d, s));
        WM_TRY(dalloc_t(m, &L.w1_f, (size_t)4 * d * d, s));
        WM_TRY(dalloc_t(m, &L.qkv_c1, 3 * d, s)); WM_TRY(dalloc_t(m, &L.qkv_c2, 3 * d, s));
        WM_TRY(dalloc_t(m, &L.xq_c1, d, s)); WM_TRY(dalloc_t(m, &L.xq_c2, d, s));
        WM_TRY(dalloc_t(m, &L.fc1_c1, 4 * d, s)); WM_TRY(dalloc_t(m, &L.fc1_c2, 4 * d, s));
        const std::string p = "decoder.blocks." + std::to_string(i);
        attn_regs(p, L.wqkv, L.bqkv, L.wqkv + (size_t)d * d, L.wqkv + (size_t)2 * d * d, L.bqkv + 2 * d, L.wo,
                  L.bo, L.ln1_g, L.ln1_b, "attn", WL_TILED, WL_TILED, WL_TILED);
        // cross-attention key/value matrices feed the big GEMM (row-major); query/out feed the GEMV
        attn_regs(p, L.wxq, L.bxq, L.wxkv, L.wxkv + (size_t)d * d, L.bxkv + d, L.wxo, L.bxo, L.lnx_g, L.lnx_b,
                  "cross_attn", WL_TILED, WL_PLAIN, WL_TILED);
        mlp_regs(p, L.w1, L.b1, L.w2, L.b2, L.ln2_g, L.ln2_b, WL_TILED);
    }
    WM_TRY(dalloc_t(m, &m->ln_g, d, s)); WM_TRY(dalloc_t(m, &m->ln_b, d, s));
    reg(m, "decoder.ln.weight", m->ln_g, false, d, 2);
    reg(m, "decoder.ln.bias", m->ln_b, false, d, 3);
    WM_TRY(dalloc_t(m, &m->emb_f, (size_t)m->vpad * d, s));
    WM_TRY(dalloc_t(m, &m->logit_c1, m->vpad, s)); WM_TRY(dalloc_t(m, &m->logit_c2, m->vpad, s));

    WM_TRY(alloc_decode_buffers(m, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

// A second context on the same device that SHARES the parent's (read-only) weights and owns its
// own stream, activations, KV caches and decode graph: lets independent batches overlap on one GPU
// (the decode chain is latency-bound, so concurrent batches fill the idle HBM bandwidth).
int wm_model_clone(wm_ctx *child, const wm_ctx *parent) {
    const WmModel *pm = parent->model;
    WM_REQUIRE(pm && pm->finalized, WM_ERR_STATE, "clone: the parent's weights must be finalised");
    WmModel *m = new WmModel();
    child->model = m;
    m->dims = pm->dims; m->finalized = true; m->k1pad = pm->k1pad; m->vpad = pm->vpad;
    m->conv1_w = pm->conv1_w; m->conv2_w = pm->conv2_w; m->conv1_b = pm->conv1_b; m->conv2_b = pm->conv2_b;
    m->enc_pos = pm->enc_pos; m->enc = pm->enc; m->ln_post_g = pm->ln_post_g; m->ln_post_b = pm->ln_post_b;
    m->tok_emb = pm->tok_emb; m->dec_pos = pm->dec_pos; m->dec = pm->dec; m->ln_g = pm->ln_g; m->ln_b = pm->ln_b;
    m->emb_f = pm->emb_f; m->logit_c1 = pm->logit_c1; m->logit_c2 = pm->logit_c2;
    m->tensors = pm->tensors; m->index = pm->index;   // registry for wm_get_tensor (pointers alias the parent)
    m->shares_weights = true;
    WM_TRY(alloc_decode_buffers(m, child->stream));
    WM_HIP(hipMemcpyAsync(m->dmask, pm->dmask, (size_t)2 * (m->vpad / 32) * 4, hipMemcpyDeviceToDevice, child->stream));
    m->mask_on = pm->mask_on; m->mask_host = pm->mask_host;
    m->ts_on = pm->ts_on; m->ts_begin = pm->ts_begin; m->ts_eot = pm->ts_eot; m->ts_max_initial = pm->ts_max_initial;
    m->align_l = pm->align_l; m->align_h = pm->align_h;
    m->teacher_panel = pm->teacher_panel;
    m->prompt_panel = pm->prompt_panel;
    m->given_panel = pm->given_panel;
    m->rep_on = pm->rep_on; m->rep_p = pm->rep_p; m->rep_n = pm->rep_n; m->rep_eot = pm->rep_eot;
    m->samp_k = pm->samp_k; m->samp_p = pm->samp_p; m->samp_minp = pm->samp_minp;
    if (m->rep_on || pm->sb_on || pm->sbt_on || pm->cst_on) WM_TRY(alloc_repetition_state(m, child->stream));
    if (pm->cst_on) {   // the parent's automaton
        WM_TRY(alloc_constraint_state(m, child->stream));
        WM_TRY(upload_constraint(m, pm->dcst, pm->cst_states, pm->cst_edges, hipMemcpyDeviceToDevice, child->stream));
        m->cst_on = true; m->cst_states = pm->cst_states; m->cst_edges = pm->cst_edges; m->cst_eot = pm->cst_eot;
    }
    if (pm->sb_on) {   // the parent's device table, as the suppress bitmaps above
        WM_TRY(alloc_seqbias_state(m, child->stream));
        const size_t ng = (size_t)pm->sb_groups, ne = (size_t)pm->sb_entries;
        WM_HIP(hipMemcpyAsync((void *)m->dsb.grp_id, pm->dsb.grp_id, ng * 4, hipMemcpyDeviceToDevice, child->stream));
        WM_HIP(hipMemcpyAsync((void *)m->dsb.grp_beg, pm->dsb.grp_beg, (ng + 1) * 4, hipMemcpyDeviceToDevice, child->stream));
        WM_HIP(hipMemcpyAsync((void *)m->dsb.ent_len, pm->dsb.ent_len, ne * 4, hipMemcpyDeviceToDevice, child->stream));
        WM_HIP(hipMemcpyAsync((void *)m->dsb.ent_bias, pm->dsb.ent_bias, ne * 4, hipMemcpyDeviceToDevice, child->stream));
        WM_HIP(hipMemcpyAsync((void *)m->dsb.ent_ctx, pm->dsb.ent_ctx, ne * WM_SB_CTX * 4, hipMemcpyDeviceToDevice, child->stream));
        m->sb_on = true; m->sb_groups = pm->sb_groups; m->sb_entries = pm->sb_entries;
    }
    if (pm->sbt_on) {   // ... and the parent's pool of row tables
        WM_TRY(alloc_seqbias_state(m, child->stream));
        WM_TRY(alloc_seqbias_pool(m, child->stream));
        WM_TRY(upload_seqbias_pool(m, pm->dsbt, pm->sbt_groups, pm->sbt_entries, hipMemcpyDeviceToDevice, child->stream));
        m->sbt_on = true; m->sbt_groups = pm->sbt_groups; m->sbt_entries = pm->sbt_entries; m->sbt_tab_grp = pm->sbt_tab_grp;
    }
    WM_HIP(hipStreamSynchronize(child->stream));
    return WM_OK;
}

void wm_model_destroy(wm_ctx *ctx) {
    WmModel *m = ctx->model;
    if (!m) return;
    wm_model_drop_graphs(m);
    if (m->h_nlive) (void)hipHostFree(m->h_nlive);
    if (m->h_spec) (void)hipHostFree(m->h_spec);
    m->spec_ws.release();
    for (void *p : m->allocs) (void)hipFree(p);
    for (WmDevBuf *b : {&m->pcm_stage, &m->io_stage, &m->align_ws, &m->acap_ws, &m->beam_ws, &m->beam_trace, &m->alt_ws, &m->given_ws})
        b->release();
    delete m;
    ctx->model = nullptr;
}

// ------------------------------------------------------------------ weights ------------
int wm_model_set_tensor(wm_ctx *ctx, const char *name, const float *data, size_t n) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    WM_REQUIRE(!m->shares_weights, WM_ERR_STATE, "a cloned context shares its parent's weights: set them on the parent");
    WM_REQUIRE(name && data, WM_ERR_INVALID, "null name / data");
    auto it = m->index.find(name);
    WM_REQUIRE(it != m->index.end(), WM_ERR_INVALID, "unknown tensor '%s'", name);
    WmTensor &t = m->tensors[it->second];
    WM_REQUIRE(n == t.n_elems, WM_ERR_INVALID, "tensor '%s': %zu elements given, %zu expected", name, n, t.n_elems);
    if (!t.is_bf16) {
        WM_HIP(hipMemcpy(t.ptr, data, n * sizeof(float), hipMemcpyHostToDevice));
    } else if (t.layout == WL_PLAIN) {
        std::vector<bf16_t> tmp(n);
        for (size_t i = 0; i < n; ++i) tmp[i] = host_f2bf(data[i]);
        WM_HIP(hipMemcpy(t.ptr, tmp.data(), n * sizeof(bf16_t), hipMemcpyHostToDevice));
    } else if (t.layout == WL_TILED) {
        const size_t K = (size_t)t.conv_kpad, N = n / K;
        const size_t Np = (N + 15) / 16 * 16;
        std::vector<bf16_t> tmp(Np * K, 0);
        for (size_t r = 0; r < N; ++r)
            for (size_t k = 0; k < K; ++k) tmp[wm_tiled_offset(r, k, K)] = host_f2bf(data[r * K + k]);
        WM_HIP(hipMemcpy(t.ptr, tmp.data(), tmp.size() * sizeof(bf16_t), hipMemcpyHostToDevice));
    } else {  // WL_CONV: [O][C][3] -> [O][kpad], k = tap*C + c
        const size_t per = (size_t)t.conv_c * 3, O = n / per;
        std::vector<bf16_t> tmp(O * t.conv_kpad, 0);
        for (size_t o = 0; o < O; ++o)
            for (int c = 0; c < t.conv_c; ++c)
                for (int tap = 0; tap < 3; ++tap)
                    tmp[o * t.conv_kpad + (size_t)tap * t.conv_c + c] = host_f2bf(data[o * per + (size_t)c * 3 + tap]);
        WM_HIP(hipMemcpy(t.ptr, tmp.data(), tmp.size() * sizeof(bf16_t), hipMemcpyHostToDevice));
    }
    t.set = true;
    m->finalized = false;
    return WM_OK;
}

int wm_model_get_tensor(wm_ctx *ctx, const char *name, float *data, size_t n) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    WM_REQUIRE(name && data, WM_ERR_INVALID, "null name / data");
    auto it = m->index.find(name);
    WM_REQUIRE(it != m->index.end(), WM_ERR_INVALID, "unknown tensor '%s'", name);
    const WmTensor &t = m->tensors[it->second];
    WM_REQUIRE(n == t.n_elems, WM_ERR_INVALID, "tensor '%s': %zu elements asked, %zu stored", name, n, t.n_elems);
    WM_HIP(hipStreamSynchronize(ctx->stream));
    if (!t.is_bf16) {
        WM_HIP(hipMemcpy(data, t.ptr, n * sizeof(float), hipMemcpyDeviceToHost));
    } else if (t.layout == WL_PLAIN) {
        std::vector<bf16_t> tmp(n);
        WM_HIP(hipMemcpy(tmp.data(), t.ptr, n * sizeof(bf16_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) data[i] = host_bf2f(tmp[i]);
    } else if (t.layout == WL_TILED) {
        const size_t K = (size_t)t.conv_kpad, N = n / K;
        const size_t Np = (N + 15) / 16 * 16;
        std::vector<bf16_t> tmp(Np * K);
        WM_HIP(hipMemcpy(tmp.data(), t.ptr, tmp.size() * sizeof(bf16_t), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < N; ++r)
            for (size_t k = 0; k < K; ++k) data[r * K + k] = host_bf2f(tmp[wm_tiled_offset(r, k, K)]);
    } else {
        const size_t per = (size_t)t.conv_c * 3, O = n / per;
        std::vector<bf16_t> tmp(O * t.conv_kpad);
        WM_HIP(hipMemcpy(tmp.data(), t.ptr, tmp.size() * sizeof(bf16_t), hipMemcpyDeviceToHost));
        for (size_t o = 0; o < O; ++o)
            for (int c = 0; c < t.conv_c; ++c)
                for (int tap = 0; tap < 3; ++tap)
                    data[o * per + (size_t)c * 3 + tap] = host_bf2f(tmp[o * t.conv_kpad + (size_t)tap * t.conv_c + c]);
    }
    return WM_OK;
}

int wm_model_init_synthetic(wm_ctx *ctx, uint64_t seed, float matrix_gain) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    WM_REQUIRE(!m->shares_weights, WM_ERR_STATE, "a cloned context shares its parent's weights");
    const int d = m->dims.n_audio_state;
    for (size_t i = 0; i < m->tensors.size(); ++i) {
        WmTensor &t = m->tensors[i];
        if (t.kind == 4) {  // openai-whisper sinusoids(): fixed encoder positions
            const int L = m->dims.n_audio_ctx, half = d / 2;
            std::vector<float> pe((size_t)L * d);
            const double inc = log(10000.0) / (half - 1);
            for (int p = 0; p < L; ++p)
                for (int j = 0; j < half; ++j) {
                    const double a = (double)p * exp(-inc * j);
                    pe[(size_t)p * d + j] = (float)sin(a);
                    pe[(size_t)p * d + half + j] = (float)cos(a);
                }
            WM_HIP(hipMemcpy(t.ptr, pe.data(), pe.size() * sizeof(float), hipMemcpyHostToDevice));
        } else {
            // matrix_gain scales the MATRICES only (weights.synthetic_state_dict(..., matrix_gain)): not the learned
            // positional table, biases or LayerNorm parameters -- the "lively" recipe of the token-level tests / bench.py
            const bool scaled = t.kind == 0 && t.name.find("positional") == std::string::npos;
            WM_TRY(wm_fill_synthetic(ctx, t, (uint32_t)(seed & 0xffffffffu), (int)i, scaled ? matrix_gain : 1.0f));
        }
        t.set = true;
    }
    WM_HIP(hipStreamSynchronize(ctx->stream));
    m->finalized = false;
    return WM_OK;
}

int wm_model_finalize(wm_ctx *ctx) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    for (const WmTensor &t : m->tensors)
        WM_REQUIRE(t.set, WM_ERR_STATE, "tensor '%s' was never set", t.name.c_str());
    // QKV fusion and conv-tap permutation happen at set time (tensors are written straight into their fused / permuted
    // HBM locations).  What is left: the LayerNorm-folded copies the decode GEMVs multiply (model.h, DecLayerW).
    const int d = m->dims.n_text_state;
    for (DecLayerW &L : m->dec) {
        WM_TRY(wm_ln_fold(ctx, L.wqkv, L.ln1_g, L.ln1_b, L.bqkv, 3 * d, d, L.wqkv_f, L.qkv_c1, L.qkv_c2));
        WM_TRY(wm_ln_fold(ctx, L.wxq, L.lnx_g, L.lnx_b, L.bxq, d, d, L.wxq_f, L.xq_c1, L.xq_c2));
        WM_TRY(wm_ln_fold(ctx, L.w1, L.ln2_g, L.ln2_b, L.b1, 4 * d, d, L.w1_f, L.fc1_c1, L.fc1_c2));
    }
    WM_TRY(wm_ln_fold(ctx, m->tok_emb, m->ln_g, m->ln_b, nullptr, m->dims.n_vocab, d, m->emb_f, m->logit_c1, m->logit_c2));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    m->finalized = true;
    return WM_OK;
}

// ------------------------------------------------------------------ activations --------
int WmDevBuf::reserve(hipStream_t stream, size_t need) {
    if (bytes >= need) return WM_OK;
    WM_HIP(hipStreamSynchronize(stream));
    if (p) WM_HIP(hipFree(p));
    p = nullptr; bytes = 0;
    WM_HIP(hipMalloc(&p, need));
    bytes = need;
    return WM_OK;
}

int wm_model_reserve(wm_ctx *ctx, int B) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m, WM_ERR_STATE, "context has no model");
    if (B <= m->cap_b) return WM_OK;
    WM_HIP(hipStreamSynchronize(ctx->stream));
    void *olds[] = {m->mel_t, m->h1p, m->x, m->xn, m->qk, m->vt, m->att, m->hid, m->xa_f32, m->mel_f32, m->xkv, m->skv};
    for (void *p : olds)
        if (p) {
            (void)hipFree(p);
            for (auto &a : m->allocs)
                if (a == p) a = nullptr;
        }
    const wm_dims &D = m->dims;
    const int d = D.n_audio_state, H = D.n_audio_head;
    const size_t M = (size_t)B * 1500;
    hipStream_t s = ctx->stream;
    WM_TRY(dalloc_t(m, &m->mel_t, (size_t)B * 3002 * D.n_mels, s));
    WM_TRY(dalloc_t(m, &m->h1p, (size_t)B * 3001 * d, s));
    WM_TRY(dalloc_t(m, &m->x, M * d, s));
    WM_TRY(dalloc_t(m, &m->xn, M * d, s));
    WM_TRY(dalloc_t(m, &m->qk, (M + 64) * 2 * d, s));
    WM_TRY(dalloc_t(m, &m->vt, (size_t)B * H * 64 * 1536, s));
    WM_TRY(dalloc_t(m, &m->att, M * d, s));
    WM_TRY(dalloc_t(m, &m->hid, M * 4 * d, s));
    WM_TRY(dalloc_t(m, &m->xa_f32, M * d, s));
    WM_TRY(dalloc_t(m, &m->mel_f32, (size_t)B * D.n_mels * WM_N_FRAMES, s));
    WM_TRY(dalloc_t(m, &m->xkv, (size_t)D.n_text_layer * 2 * B * H * 1500 * 64, s));
    const int Bd = std::max(B < WM_DEC_MAXB ? B : WM_DEC_MAXB, m->cap_rows);   // (cap_rows: wm_model_reserve_rows)
    WM_TRY(dalloc_t(m, &m->skv, (size_t)D.n_text_layer * 2 * Bd * H * D.n_text_ctx * 64, s));
    m->cap_b = B;
    m->cap_rows = Bd;
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

// A candidate group decodes more rows than it encodes windows: the self-attention K/V cache alone grows to `rows` decoder
// rows.  The captured graphs hold its address, so they are dropped with it.
int wm_model_reserve_rows(wm_ctx *ctx, int rows) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m && rows >= 1 && rows <= WM_DEC_MAXB, WM_ERR_INVALID, "decode rows must be 1..%d", WM_DEC_MAXB);
    if (rows <= m->cap_rows) return WM_OK;
    WM_HIP(hipStreamSynchronize(ctx->stream));
    wm_model_drop_graphs(m);
    if (m->skv) {
        (void)hipFree(m->skv);
        for (auto &a : m->allocs)
            if (a == m->skv) a = nullptr;
        m->skv = nullptr;
    }
    const wm_dims &D = m->dims;
    m->cap_rows = 0;
    WM_TRY(dalloc_t(m, &m->skv, (size_t)D.n_text_layer * 2 * rows * D.n_audio_head * D.n_text_ctx * 64, ctx->stream));
    m->cap_rows = rows;
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
}

// ------------------------------------------------------------------ encoder ------------
static GemmArgs plain_gemm(const bf16_t *A, int lda, const bf16_t *W, const float *bias, void *C, int ldc,
                           int M, int N, int K, int epi) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.a_rpb = (long)M + 1; g.a_bstride = 0; g.a_rstride = lda;
    g.W = W; g.bias = bias; g.C = C;
    g.c_rpb = (long)M + 1; g.c_bstride = 0; g.c_rstride = ldc;
    g.M = M; g.N = N; g.K = K; g.epi = epi;
    return g;
}

int wm_model_encode_dev(wm_ctx *ctx, const float *d_mel, int B, float *d_xa_out) {
    return wm_model_encode_win(ctx, d_mel, nullptr, B, d_xa_out);
}

// The stem: mel re-layout, conv1, conv2 (+ positional embedding) -> m->x.  Its own function so that the debug library can run
// exactly these three launches on a loaded model (wmdbg_encode_stem).
int wm_model_encode_stem(wm_ctx *ctx, const float *d_mel, const WmMelWin *d_win, int B) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m && m->finalized, WM_ERR_STATE, "model weights not finalised (wm_finalize)");
    WM_REQUIRE(B >= 1, WM_ERR_INVALID, "B must be >= 1");
    WM_TRY(wm_model_reserve(ctx, B));
    const wm_dims &D = m->dims;
    const int d = D.n_audio_state, S = 1500, C = D.n_mels;
    const int M = B * S;
    // mel [B][C][3000] f32 (or the windows d_win) -> time-major bf16 with zero edge rows (conv padding = 1)
    WM_TRY(wm_mel_to_time_major(ctx, d_mel, B, C, m->mel_t, d_win));
    {   // conv1 (k3, p1) + GELU as an implicit GEMM: window of frame t = mel_t[b][t..t+2][:]
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        g.A = m->mel_t; g.a_rpb = 3000; g.a_bstride = 3002L * C; g.a_rstride = C;
        g.W = m->conv1_w; g.bias = m->conv1_b;
        g.C = m->h1p + d; g.c_rpb = 3000; g.c_bstride = 3001L * d; g.c_rstride = d;
        g.M = B * 3000; g.N = d; g.K = m->k1pad; g.epi = EPI_GELU_BF16;
        WM_TRY(wm_gemm(ctx, g));
    }
    {   // conv2 (k3, s2, p1) + GELU + positional embedding: window of frame s = h1p[b][2s..2s+2][:]
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        g.A = m->h1p; g.a_rpb = S; g.a_bstride = 3001L * d; g.a_rstride = 2L * d;
        g.W = m->conv2_w; g.bias = m->conv2_b;
        g.C = m->x; g.c_rpb = S; g.c_bstride = (long)S * d; g.c_rstride = d;
        g.M = M; g.N = d; g.K = 3 * d; g.epi = EPI_CONV2_F32; g.pos = m->enc_pos;
        WM_TRY(wm_gemm(ctx, g));
    }
    return WM_OK;
}

// One encoder layer's first two launches: LayerNorm of the residual stream m->x into m->xn, then the QKV product (queries
// pre-scaled and keys into m->qk, values transposed into m->vt).  (Also run on its own by wmdbg_encode_layer_qkv.)
int wm_model_encode_layer_qkv(wm_ctx *ctx, int layer, int B) {
    WmModel *m = ctx->model;
    const wm_dims &D = m->dims;
    const int d = D.n_audio_state, H = D.n_audio_head, S = 1500, M = B * S;
    const EncLayerW &L = m->enc[layer];
    WM_TRY(wm_layernorm(ctx, m->x, L.ln1_g, L.ln1_b, M, d, m->xn, nullptr));
    GemmArgs g = plain_gemm(m->xn, d, L.wqkv, L.bqkv, m->qk, 2 * d, M, 3 * d, d, EPI_QKV_ENC);
    g.vt = m->vt; g.d_model = d; g.n_head = H; g.seq = S; g.seq_pad = 1536; g.batch = B;
    return wm_gemm(ctx, g);
}

// The rest of the layer: attention over m->qk / m->vt into m->att, the out-projection onto the residual stream m->x, LayerNorm
// into m->xn, fc1 + GELU into m->hid, fc2 onto m->x.  (Also run on its own by wmdbg_encode_layer_tail, which hands d_x_mid:
// device f32 [B * 1500][d] that receives a copy of the residual stream between the out-projection and the LayerNorm -- the one
// intermediate a later launch of the layer overwrites.  The encoder passes null: no copy.)
int wm_model_encode_layer_tail(wm_ctx *ctx, int layer, int B, float *d_x_mid) {
    WmModel *m = ctx->model;
    const wm_dims &D = m->dims;
    const int d = D.n_audio_state, H = D.n_audio_head, S = 1500, M = B * S;
    const EncLayerW &L = m->enc[layer];
    WM_TRY(wm_enc_attention(ctx, m->qk, m->vt, m->att, B, H, S, 1536, d));
    WM_TRY(wm_gemm(ctx, plain_gemm(m->att, d, L.wo, L.bo, m->x, d, M, d, d, EPI_RESID_F32)));
    if (d_x_mid) WM_HIP(hipMemcpyAsync(d_x_mid, m->x, (size_t)M * d * 4, hipMemcpyDeviceToDevice, ctx->stream));
    WM_TRY(wm_layernorm(ctx, m->x, L.ln2_g, L.ln2_b, M, d, m->xn, nullptr));
    WM_TRY(wm_gemm(ctx, plain_gemm(m->xn, d, L.w1, L.b1, m->hid, 4 * d, M, 4 * d, d, EPI_GELU_BF16)));
    return wm_gemm(ctx, plain_gemm(m->hid, 4 * d, L.w2, L.b2, m->x, d, M, d, 4 * d, EPI_RESID_F32));
}

// ln_post of the residual stream m->x: bf16 into m->xn (the cross-K/V product's operand), f32 into d_xa_out or m->xa_f32.
// (Also run on its own by wmdbg_encode_post.)
int wm_model_encode_post(wm_ctx *ctx, int B, float *d_xa_out) {
    WmModel *m = ctx->model;
    const int d = m->dims.n_audio_state, M = B * 1500;
    return wm_layernorm(ctx, m->x, m->ln_post_g, m->ln_post_b, M, d, m->xn, d_xa_out ? d_xa_out : m->xa_f32);
}

int wm_model_encode_win(wm_ctx *ctx, const float *d_mel, const WmMelWin *d_win, int B, float *d_xa_out) {
    WM_TRY(wm_model_encode_stem(ctx, d_mel, d_win, B));
    const int n_layer = ctx->model->dims.n_audio_layer;
    for (int i = 0; i < n_layer; ++i) {
        WM_TRY(wm_model_encode_layer_qkv(ctx, i, B));
        WM_TRY(wm_model_encode_layer_tail(ctx, i, B, nullptr));
    }
    return wm_model_encode_post(ctx, B, d_xa_out);
}

int wm_model_set_xa(wm_ctx *ctx, const float *d_xa, int B) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m && m->finalized, WM_ERR_STATE, "model weights not finalised (wm_finalize)");
    WM_TRY(wm_model_reserve(ctx, B));
    return wm_f32_to_bf16(ctx, d_xa, m->xn, (size_t)B * 1500 * m->dims.n_audio_state);
}

// Cross-attention K/V of the encoder output, once per chunk (the reference's exported decoder
// recomputes these inside every call -- SURVEY.md 8a row a15; caching them is the point of K9).
int wm_model_cross_kv(wm_ctx *ctx, int B) {
    WmModel *m = ctx->model;
    const wm_dims &D = m->dims;
    const int d = D.n_text_state, H = D.n_text_head, S = 1500, M = B * S;
    for (int l = 0; l < D.n_text_layer; ++l) {
        const DecLayerW &L = m->dec[l];
        GemmArgs g = plain_gemm(m->xn, d, L.wxkv, L.bxkv, m->xkv + (size_t)l * 2 * B * H * S * 64, 0, M, 2 * d, d,
                                EPI_XKV);
        g.d_model = d; g.n_head = H; g.seq = S; g.batch = B;
        WM_TRY(wm_gemm(ctx, g));
    }
    return WM_OK;
}

// ------------------------------------------------------------------ decoder ------------
int wm_model_decode_begin(wm_ctx *ctx, int B) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m && m->finalized, WM_ERR_STATE, "model weights not finalised (wm_finalize)");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB, WM_ERR_INVALID, "decode batch must be 1..%d", WM_DEC_MAXB);
    // the arrival counter of the arg-max workgroups is zero between launches; a decode that was abandoned half way
    // (an error in the middle of a step) must not leave the next one with a stale count
    WM_HIP(hipMemsetAsync(m->darrive, 0, sizeof(int), ctx->stream));
    return WM_OK;
}

int wm_model_set_pos(wm_ctx *ctx, int pos) {
    WmModel *m = ctx->model;
    if (pos == 0) {
        WM_HIP(hipMemsetAsync(m->dpos, 0, sizeof(int), ctx->stream));  // no host operand: stays asynchronous
        return WM_OK;
    }
    WM_HIP(hipMemcpyAsync(m->dpos, &pos, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));  // `pos` is a stack variable
    return WM_OK;
}

// grp / c0 (a panel step only, else 0): the step's windows are rows c0 .. of a group of grp windows whose caches are laid out
// [L][2][grp][H][.][64] -- the per-layer pointers advance by whole windows (wm_model_panel_step)
// cache_only (a prompt-prefill step, wm_model_prompt_prefill): the layers alone -- no logits product; the one panel step that
// admits the row offsets of a ragged group (the offsets of the step's windows: m->doff + c0)
static int decode_step_impl(wm_ctx *ctx, int B, bool want_logits, int arg_first, int arg_last, const WmAlignCap *cap,
                            const WmDecodeMode &mode, int n_prompt, int grp, int c0, bool cache_only = false) {
    WmModel *m = ctx->model;
    const wm_dims &D = m->dims;
    const int d = D.n_text_state, H = D.n_text_head, T = D.n_text_ctx, S = 1500;
    const int PW = mode.panel > 1 ? mode.panel : 1;     // panel step: B = Bx windows x PW positions, one self AND one cross cache entry per window
    const int NC = mode.n_cand > 1 ? mode.n_cand : 1;   // candidate group: B = Bx windows x NC rows, one cross cache per window
    // (mode.x without the repetition rules: the verify step of a speculative group, wm_model_spec_panel_step)
    WM_REQUIRE(PW == 1 || (NC == 1 && !mode.stop && (!mode.off || cache_only) && !(mode.x && mode.rep) && B % PW == 0), WM_ERR_STATE,
               "decode step: a panel is a plain teacher-forced step of windows x width rows");
    const int Bx = B / (NC * PW);
    const int Gx = grp > 0 ? grp : Bx;                  // windows per layer of the cross cache
    const int Gs = grp > 0 ? grp : (PW > 1 ? Bx : B);   // rows per layer of the self cache
    const int ns = wm_dec_attn_splits(B, H);
    const int xns = g_wm_tuning.xattn_splits > 0 ? g_wm_tuning.xattn_splits : ns;   // 0 in the product
    const bool xshort = mode.xattn_shared && !g_wm_tuning.xattn_never_short;
    // mean-centring offsets of the bf16 residual copy: the embedding wrote buffer 0; every LayerNorm-folded GEMV reads
    // the current buffer and leaves the new means in the other one
    int cur = 0;
    auto mean_buf = [&](int i) { return m->dmean + (size_t)i * WM_DEC_MAXB; };
    for (int l = 0; l < D.n_text_layer; ++l) {
        const DecLayerW &L = m->dec[l];
        bf16_t *kc = m->skv + ((size_t)(l * 2 + 0) * Gs + c0) * H * T * 64;
        bf16_t *vc = m->skv + ((size_t)(l * 2 + 1) * Gs + c0) * H * T * 64;
        const bf16_t *xk = m->xkv + ((size_t)(l * 2 + 0) * Gx + c0) * H * S * 64;
        const bf16_t *xv = m->xkv + ((size_t)(l * 2 + 1) * Gx + c0) * H * S * 64;
        // the layer's attentions: what self and cross share here, the rest at their calls
        DecAttnArgs t = {};
        t.q = m->dq; t.att = m->datt; t.H = H; t.live = mode.stop ? m->dlive : nullptr;
        t.B = B; t.C = Bx; t.N = NC * PW;       // a candidate group / a panel: Bx windows x NC * PW rows
        DecGemvArgs a;
        // 1. attn_ln (folded) + fused q|k|v projection; k, v appended to the self-attention cache
        memset(&a, 0, sizeof(a));
        a.epi = DE_QKV; a.B = B; a.N = 3 * d; a.K = d; a.W = L.wqkv_f; a.c1 = L.qkv_c1; a.c2 = L.qkv_c2;
        a.a = m->dxb; a.out_f32 = m->dq; a.kcache = kc; a.vcache = vc;
        a.stats_in = m->dstats;
        a.mean_in = mean_buf(cur); a.mean_out = mean_buf(cur ^ 1); cur ^= 1;
        a.pos_ptr = m->dpos; a.n_ctx = T; a.n_head = H;
        if (PW > 1) { a.epi = DE_QKV_P; a.panel = PW; }   // row (c, s) appends at position pos + s of window c
        WM_TRY(wm_dec_gemv(ctx, a));
        // 2. causal self-attention over positions 0..pos (a panel row: 0 .. pos + s of its window)
        t.kc = kc; t.vc = vc; t.T_stride = T; t.n_keys = 0; t.pos_ptr = m->dpos; t.off = mode.off ? m->doff + c0 : nullptr;
        t.pf = {L.wo, d, d};
        WM_TRY(PW > 1 ? wm_dec_self_attention_panel(ctx, t) : wm_dec_self_attention(ctx, t));
        // 3. out-projection + residual (f32 stream, its bf16 copy, partial statistics)
        memset(&a, 0, sizeof(a));
        a.epi = DE_RESID; a.B = B; a.N = d; a.K = d; a.W = L.wo; a.c2 = L.bo;
        a.a = m->datt; a.out_f32 = m->dx; a.out_bf16 = m->dxb; a.ldo = d; a.stats_out = m->dstats;
        a.mean_in = mean_buf(cur);
        a.pf_ptr = L.wxq_f; a.pf_rows = d; a.pf_k = d;
        // wm_align: a layer with alignment heads leaves its f32 query in m->dq (the two launches: same bits as the fused one)
        const bool cap_l = cap && cap->layer[l].n > 0;
        const bool fuse_q = NC == 1 && PW == 1 && !cap_l && xns == 1 && wm_dec_xattn_fq_applies(B, H, d, xshort);
        a.pf_head_major = fuse_q ? (H * B + 7) / 8 : 0;   // pairs per XCD of the fused consumer
        WM_TRY(wm_dec_gemv(ctx, a));
        // 4. cross_attn_ln (folded) + query projection
        memset(&a, 0, sizeof(a));
        a.epi = DE_Q; a.B = B; a.N = d; a.K = d; a.W = L.wxq_f; a.c1 = L.xq_c1; a.c2 = L.xq_c2;
        a.a = m->dxb; a.out_f32 = m->dq; a.ldo = d;
        a.stats_in = m->dstats;
        a.mean_in = mean_buf(cur); a.mean_out = mean_buf(cur ^ 1); cur ^= 1;
        // the cross-attention over the 1500 cached encoder frames
        t.kc = xk; t.vc = xv; t.T_stride = S; t.n_keys = S; t.pos_ptr = nullptr; t.off = nullptr;
        t.part = m->dpart; t.nsplit = xns; t.short_lived = xshort; t.pf = {L.wxo, d, d};
        if (fuse_q) {
            // 4 + 5 as ONE launch (the latency shape: every pair's workgroup forms its own query, dec_kernels.hip).  Differs from
            // the two launches for FINISHED rows only (early stop): their block's means stay stale, m->dq is not written
            WM_TRY(wm_dec_xattn_fq(ctx, a, t));
        } else {
            WM_TRY(wm_dec_gemv(ctx, a));
            if (cap_l) WM_TRY(wm_align_capture_q(ctx, m->dq, d, B, cap->layer[l], cap->q, cap->Tq, cap->J, m->dpos, PW, cap->base));
            // 5. the cross-attention (a candidate group, a panel: one K/V read per window)
            WM_TRY(NC > 1 || PW > 1 ? wm_dec_attention_cand(ctx, t) : wm_dec_attention(ctx, t));
        }
        // 6. out-projection + residual
        memset(&a, 0, sizeof(a));
        a.epi = DE_RESID; a.B = B; a.N = d; a.K = d; a.W = L.wxo; a.c2 = L.bxo;
        a.a = m->datt; a.out_f32 = m->dx; a.out_bf16 = m->dxb; a.ldo = d; a.stats_out = m->dstats;
        a.mean_in = mean_buf(cur);
        a.pf_ptr = L.w1_f; a.pf_rows = 4 * d; a.pf_k = d;
        WM_TRY(wm_dec_gemv(ctx, a));
        // 7. mlp_ln (folded) + fc1 + GELU
        memset(&a, 0, sizeof(a));
        a.epi = DE_GELU; a.B = B; a.N = 4 * d; a.K = d; a.W = L.w1_f; a.c1 = L.fc1_c1; a.c2 = L.fc1_c2;
        a.a = m->dxb; a.out_bf16 = m->dhid; a.ldo = 4 * d;
        a.stats_in = m->dstats;
        a.mean_in = mean_buf(cur); a.mean_out = mean_buf(cur ^ 1); cur ^= 1;
        a.pf_ptr = L.w2; a.pf_rows = d; a.pf_k = 4 * d;
        WM_TRY(wm_dec_gemv(ctx, a));
        // 8. fc2 + residual
        memset(&a, 0, sizeof(a));
        a.epi = DE_RESID; a.B = B; a.N = d; a.K = 4 * d; a.W = L.w2; a.c2 = L.b2;
        a.a = m->dhid; a.out_f32 = m->dx; a.out_bf16 = m->dxb; a.ldo = d; a.stats_out = m->dstats;
        a.mean_in = mean_buf(cur);
        if (l + 1 < D.n_text_layer) { a.pf_ptr = m->dec[l + 1].wqkv_f; a.pf_rows = 3 * d; a.pf_k = d; }
        WM_TRY(wm_dec_gemv(ctx, a));
    }
    if (cache_only) return WM_OK;   // the positions' k / v are in the self-attention cache: nobody reads their logits
    {   // final LayerNorm (folded) + tied-embedding logits + fused per-tile arg-max
        DecGemvArgs a;
        memset(&a, 0, sizeof(a));
        a.epi = DE_LOGITS; a.B = B; a.N = D.n_vocab; a.K = d; a.W = m->emb_f; a.c1 = m->logit_c1; a.c2 = m->logit_c2;
        a.a = m->dxb; a.stats_in = m->dstats;
        a.mean_in = mean_buf(cur); a.mean_out = mean_buf(cur ^ 1);
        a.out_f32 = want_logits ? m->dlogits : nullptr; a.ldo = m->vpad;
        a.argmax = m->dargmax; a.arg_first = arg_first; a.arg_last = arg_last;
        if (mode.mask) {
            a.mask = m->dmask; a.mask_words = m->vpad / 32; a.mask_first_pos = n_prompt - 1; a.pos_ptr = m->dpos;
        }
        if (mode.ts) a.ts = wm_model_ts_dev(m);
        if (mode.x) {   // extended decode: its own epilogue instantiation, the position always from the device
            a.epi = DE_LOGITS_X; a.x = wm_model_x_dev(m, mode); a.pos_ptr = m->dpos;
        }
        if (mode.rep) {   // repetition rules: the rows' bitmaps rebuilt from their histories, in line in front of the product
            WM_REQUIRE(mode.x, WM_ERR_STATE, "decode step: the repetition rules need the extended decode");
            a.epi = DE_LOGITS_XR; a.rep = wm_model_rep_dev(m, mode);
            WM_TRY(wm_repeat_state(ctx, m->dseq, m->dpos, B, n_prompt, D.n_text_ctx, D.n_vocab, a.rep));
        }
        if (mode.sb) {   // sequence bias: the rows' hit words and totals, behind the bitmaps it ORs its bans into
            WM_REQUIRE(mode.rep, WM_ERR_STATE, "decode step: the sequence bias needs the repetition-rule state");
            const WmSbDev sb = wm_model_sb_dev(m, mode);
            a.epi = DE_LOGITS_XB; a.sb = sb.e;
            if (mode.sbt)   // row tables: each row walks its own table's groups of the pool
                WM_TRY(wm_seqbias_rows_state(ctx, m->dseq, m->dpos, B, n_prompt, D.n_text_ctx, D.n_vocab, sb, m->dsb_rng, a.rep.ban, a.rep.words));
            else
                WM_TRY(wm_seqbias_state(ctx, m->dseq, m->dpos, B, n_prompt, D.n_text_ctx, D.n_vocab, sb, a.rep.ban, a.rep.words));
        }
        if (mode.cst) {   // constraint: the ids the rows' automaton states do not allow, OR-ed into the same ban words
            WM_REQUIRE(mode.rep && m->dcst.par, WM_ERR_STATE, "decode step: the constraint needs the repetition-rule state and its tables");
            WM_TRY(wm_constraint_state(ctx, m->dseq, m->dpos, B, n_prompt, D.n_text_ctx, D.n_vocab, m->dcst, a.rep.ban, a.rep.words, nullptr));
        }
        WM_TRY(wm_dec_gemv(ctx, a));
    }
    return WM_OK;
}

int wm_model_decode_step(wm_ctx *ctx, int B, bool want_logits, int arg_first, int arg_last, const WmAlignCap *cap,
                         const WmDecodeMode &mode, int n_prompt) {
    WM_REQUIRE(mode.panel <= 1, WM_ERR_STATE, "decode step: panels run through wm_model_panel_step");
    return decode_step_impl(ctx, B, want_logits, arg_first, arg_last, cap, mode, n_prompt, 0, 0);
}

// ------------------------------------------------------------------ teacher-forced panels
// How a group of G windows is cut for a pass of T positions at the context's width: slices of C windows x panels of w positions,
// C * w <= 128 rows.  A pass costs (steps) x (a + b * rows) with a -- the weight stream and the launch chain of a step -- the
// larger part (large-v2: 3.3 ms at 64 rows, 4.4 at 120, 5.5 at 128), and steps x rows is the same G x T for every cut: the cut
// with the FEWEST STEPS wins.  So: among the widths w' <= width, slices of floor(128 / w') windows, take the one with the fewest
// slices x ceil(T / w') steps (ties: the wider); its slices are balanced.  Up to 128 / width windows that is the whole group at
// the full width.  Measured, both candidate rules of a larger group (profiles/r18_teacher_panel.txt): 24 windows -- one panel
// narrowed to 5 positions (46 steps) beats slices of 16 at width 8 (58 steps) by 21 - 26 %; 48 windows -- three slices at width 8
// (87 steps) beat one panel narrowed to 2 (115 steps) by 14 %.  Results cannot depend on the cut.
void wm_model_panel_slices(int G, int width, int T, int *C, int *w) {
    const int knob = g_wm_tuning.teacher_panel_cut;   // (probes: 1 = one narrowed panel, 2 = slices at the full width; 0: the rule)
    wm_panel_slices(G, width, T, knob, C, w);   // (stated in tx_plan.cpp: the prompt-panel plan cuts by the same rule)
}

static int panel_check(wm_ctx *ctx, int G, int c0, int C, int w) {
    WmModel *m = ctx->model;
    WM_TRY(wm_panel_shape_check(C, w, "panel"));
    WM_REQUIRE(m && c0 >= 0 && c0 + C <= G && G <= m->cap_b && G <= m->cap_rows, WM_ERR_INVALID,
               "panel: windows [%d, %d) of %d at width %d", c0, c0 + C, G, w);
    return WM_OK;
}

// The mode of a panel step of width w inside a group's call: the group's own, with nothing that stops a row -- the rows of
// frozen windows are computed and ignored, no live list; the round's commit kernel keeps the stop state.
static WmDecodeMode panel_mode(const WmDecodeMode &mode, int w) {
    WmDecodeMode pm = mode;
    pm.panel = w; pm.stop = false; pm.budget = false; pm.stop_eot = -1;
    return pm;
}

int wm_model_panel_embed(wm_ctx *ctx, int G, int c0, int C, int w) {
    WM_TRY(panel_check(ctx, G, c0, C, w));
    WmModel *m = ctx->model;
    return wm_dec_embed_panel(ctx, m->dseq + c0, G, m->dpos, 0, C, w, m->dims.n_text_ctx, wm_model_embed_dev(m));
}

int wm_model_panel_step(wm_ctx *ctx, int G, int c0, int C, int w, bool want_logits, const WmAlignCap *cap) {
    WM_TRY(panel_check(ctx, G, c0, C, w));
    WmDecodeMode mode;
    mode.panel = w;
    WmAlignCap cs;
    if (cap) {   // the slice's chunks start at c0 of the capture buffer [G][Tq][J][64]
        cs = *cap;
        cs.q = cap->q + (size_t)c0 * cap->Tq * cap->J * 64;
    }
    // (w == 1, the last panel of a pass with T mod width == 1: the plain step launches over the slice's windows)
    return decode_step_impl(ctx, C * w, want_logits, 0, ctx->model->dims.n_vocab - 1, cap ? &cs : nullptr, mode, 0, G, c0);
}

int wm_model_panel_advance(wm_ctx *ctx, int G, int c0, int C, int w, int w_next) {
    WM_TRY(panel_check(ctx, G, c0, C, w));
    WmModel *m = ctx->model;
    if (w_next > 0)   // the next panel's embedding reads the position BEFORE it advances (stream order)
        WM_TRY(wm_dec_embed_panel(ctx, m->dseq + c0, G, m->dpos, w, C, w_next, m->dims.n_text_ctx, wm_model_embed_dev(m)));
    return wm_dec_pos_add(ctx, m->dpos, w);
}

// ------------------------------------------------------------------ speculative decoding
int wm_model_spec_panel_step(wm_ctx *ctx, int G, int w, const WmDecodeMode &mode, int n_prompt) {
    WM_TRY(panel_check(ctx, G, 0, G, w));
    WM_REQUIRE(mode.x && !mode.off && !mode.rep && mode.n_cand <= 1 && !mode.beam && !mode.acap, WM_ERR_STATE,
               "speculative verify step: a plain extended-decode group");
    return decode_step_impl(ctx, G * w, false, 0, ctx->model->dims.n_vocab - 1, nullptr, panel_mode(mode, w), n_prompt, G, 0);
}

int wm_model_spec_dev(wm_ctx *ctx, wm_ctx *draft, int max_new, WmSpecDev *out, int **script_area) {
    WmModel *m = ctx->model, *dm = draft->model;
    constexpr size_t R = WM_DEC_MAXB;
    WM_TRY(m->spec_ws.reserve(ctx->stream, (R * 24 + R * (size_t)m->dims.n_text_ctx) * 4));
    if (!m->h_spec) WM_HIP(hipHostMalloc((void **)&m->h_spec, WM_NLIVE_RING * 2 * sizeof(int), hipHostMallocDefault));
    int *p = (int *)m->spec_ws.p;
    WmSpecDev sp;
    memset(&sp, 0, sizeof(sp));
    sp.tseq = m->dseq; sp.dseq = dm->dseq; sp.tpos = m->dpos; sp.dpos = dm->dpos;
    sp.tts = wm_model_ts_dev(m); sp.dts = wm_model_ts_dev(dm);
    sp.chist = p; sp.crng = p + R * 4; sp.dchist = p + R * 8; sp.dcrng = p + R * 12;
    sp.wtok = p + R * 16; sp.wlp = (float *)(p + R * 17); sp.acc = p + R * 18; sp.stats = p + R * 19; sp.round = p + R * 23;
    sp.max_new = max_new; sp.n_vocab = m->dims.n_vocab;
    *script_area = p + R * 24;
    *out = sp;
    return WM_OK;
}

// ------------------------------------------------------------------ prompt panels (wm_set_prompt_panel)
// Positions [0, P0) of a plain decode group of G rows as panel steps that only fill the self-attention cache (tx_plan.h
// wm_prompt_panel_plan): per slice of C windows -- position 0, the panels' embeddings, cache-only steps under a copy of the
// group's mode without anything a close or a logits epilogue would read (the pattern of wm_model_spec_panel_step), the
// position advanced by the panel's width.  Then the device position is P0 and the embedding of position P0 of all G rows is
// written with embed_row's arithmetic into rows 0 .. G - 1 of dx / dxb / dstats / dmean[0]: what the close of step P0 - 1
// leaves, so the group's ordinary steps and captured graphs continue from t = P0.  Expects the prompt table in m->dseq, the
// offsets of a ragged group in m->doff and the cross-K/V of the G windows in m->xkv.
int wm_model_prompt_prefill(wm_ctx *ctx, int G, int P0, const WmDecodeMode &mode) {
    WmModel *m = ctx->model;
    WmPromptPanelPlan pl;
    wm_prompt_panel_plan(G, m->prompt_panel, P0 + 1, P0, -1, g_wm_tuning.teacher_panel_cut, &pl);
    WM_REQUIRE(pl.w >= 1 && pl.P0 == P0 && P0 < m->dims.n_text_ctx, WM_ERR_STATE, "prompt prefill: nothing to run for %d rows up to position %d",
               G, P0);
    WM_REQUIRE(mode.n_cand <= 1 && !mode.beam, WM_ERR_STATE, "prompt prefill: a plain decode group");
    WmDecodeMode pm = panel_mode(mode, pl.w);   // (each step sets its own width below)
    pm.acap = false; pm.acap_base = pm.acap_Tq = pm.acap_J = 0; pm.acap_q = nullptr;
    pm.rep = false; pm.sb = false; pm.sbt = false; pm.cst = false; pm.mask = false; pm.ts = false; pm.x = false;
    const int *off0 = mode.off ? m->doff : nullptr;
    const WmEmbedDev e = wm_model_embed_dev(m);
    const int T = m->dims.n_text_ctx;
    for (int c0 = 0; c0 < G; c0 += pl.C) {
        const int C = std::min(pl.C, G - c0);
        const int *off = off0 ? off0 + c0 : nullptr;
        WM_TRY(panel_check(ctx, G, c0, C, pl.w));
        WM_TRY(wm_model_set_pos(ctx, 0));
        WM_TRY(wm_dec_embed_panel(ctx, m->dseq + c0, G, m->dpos, 0, C, std::min(pl.w, P0), T, e, off));
        for (int t = 0; t < P0; t += pl.w) {
            const int wp = std::min(pl.w, P0 - t), wn = std::min(pl.w, P0 - t - wp);
            pm.panel = wp;
            WM_TRY(decode_step_impl(ctx, C * wp, false, 0, m->dims.n_vocab - 1, nullptr, pm, 0, G, c0, true));
            if (wn > 0) WM_TRY(wm_dec_embed_panel(ctx, m->dseq + c0, G, m->dpos, wp, C, wn, T, e, off));
            WM_TRY(wm_dec_pos_add(ctx, m->dpos, wp));
        }
    }
    // *dpos == P0: the group's rows at that position (one row per window: embed_row, P0 >= 2)
    WM_TRY(wm_dec_embed_panel(ctx, m->dseq, G, m->dpos, 0, G, 1, T, e, off0));
    m->last_prefill[0] = P0; m->last_prefill[1] = pl.slices; m->last_prefill[2] = pl.slices * pl.steps;
    return WM_OK;
}

// ------------------------------------------------------------------ given panels (wm_set_given_panel)
int wm_model_given_panel_dev(wm_ctx *ctx, int max_new, WmGivenPanelDev *out) {
    WmModel *m = ctx->model;
    WM_REQUIRE(m->dgiven_side, WM_ERR_STATE, "given panels: the group has no table (wm_model_given_begin)");
    constexpr size_t R = WM_DEC_MAXB;
    int *p = m->dgiven_side;
    WmGivenPanelDev gp;
    memset(&gp, 0, sizeof(gp));
    gp.seq = m->dseq; gp.pos = m->dpos; gp.ts = wm_model_ts_dev(m);
    gp.chist = p; gp.crng = p + R * 4; gp.wtok = p + R * 8; gp.wlp = (float *)(p + R * 9);
    gp.par = m->dgiven_par; gp.max_new = max_new; gp.n_vocab = m->dims.n_vocab;
    *out = gp;
    return WM_OK;
}

// A round: stage, the panel's embeddings, one step over G x w rows under the group's own mode with the f32 row stored (the pattern
// of wm_model_spec_panel_step: the rows of frozen windows are computed and ignored, no live list), close + commit.  Eager.
int wm_model_given_panel_phase(wm_ctx *ctx, int G, int w, int Lp, int n_prompt, int max_new, const WmDecodeMode &mode) {
    WmModel *m = ctx->model;
    const int T = m->dims.n_text_ctx, V = m->dims.n_vocab;
    WM_TRY(panel_check(ctx, G, 0, G, w));
    WM_REQUIRE(mode.given && mode.x && !mode.off && !mode.rep && !mode.sb && !mode.cst && !mode.alt && !mode.trunc && !mode.srows &&
                   mode.n_cand <= 1 && !mode.beam && !mode.acap,
               WM_ERR_STATE, "given panels: a plain temperature-0 extended-decode group with a table and no per-row rule state");
    WM_REQUIRE(w >= 2 && Lp >= 2 && Lp <= max_new && n_prompt + Lp - 1 < T, WM_ERR_STATE, "given panels: nothing to run for %d rows up to index %d", G, Lp);
    WmGivenPanelDev gp;
    WM_TRY(wm_model_given_panel_dev(ctx, max_new, &gp));
    if (!mode.ts) memset(&gp.ts, 0, sizeof(gp.ts));
    WmStoredRows rows = wm_model_stored_rows(m, G * w, n_prompt, mode);   // (no ban rows: !mode.rep)
    const WmEmbedDev e = wm_model_embed_dev(m);
    int rounds = 0;
    for (int g0 = 1; g0 < Lp; g0 += w, ++rounds) {
        const int wr = std::min(w, Lp - g0);
        const bool last = g0 + wr >= Lp;
        WM_TRY(wm_given_panel_stage(ctx, gp, rows.stop, G, wr, n_prompt, T, g0 == 1));
        WM_TRY(wm_dec_embed_panel(ctx, m->dseq, G, m->dpos, 0, G, wr, T, e));
        WM_TRY(decode_step_impl(ctx, G * wr, true, 0, V - 1, nullptr, panel_mode(mode, wr), n_prompt, G, 0));
        rows.rows = G * wr;
        WM_TRY(wm_given_panel_close(ctx, rows, gp, G, wr, mode.ts ? m->ts_eot : 0, last));
    }
    // *dpos == n_prompt + Lp - 1: the group's rows at that position, as wm_model_prompt_prefill ends
    WM_TRY(wm_dec_embed_panel(ctx, m->dseq, G, m->dpos, 0, G, 1, T, e));
    m->last_given_panel[0] = 1; m->last_given_panel[1] = Lp - 1; m->last_given_panel[2] = rounds; m->last_given_panel[3] = w;
    return WM_OK;
}

int wm_model_embed_first(wm_ctx *ctx, int B, const WmDecodeMode &mode) {
    WmModel *m = ctx->model;
    return wm_dec_embed(ctx, m->dseq, m->dpos, B, wm_model_embed_dev(m), mode.off ? m->doff : nullptr);
}

int wm_model_close_step(wm_ctx *ctx, int B, int n_prompt, bool write_seq, int *result, int arg_first, const WmDecodeMode &mode) {
    WmModel *m = ctx->model;
    // (the device views of a mode that is off are empty: wm_model_stop_dev, wm_model_x_dev)
    return wm_argmax_embed(ctx, m->dargmax, m->vpad / 16, B, write_seq ? m->dseq : nullptr, m->dpos, n_prompt, result, arg_first,
                           m->dims.n_text_ctx, wm_model_embed_dev(m), mode.ts ? wm_model_ts_dev(m) : WmTsDev{}, m->darrive,
                           mode.ts ? m->ts_eot : arg_first, wm_model_stop_dev(m, mode), wm_model_x_dev(m, mode),
                           mode.off ? m->doff : nullptr);
}
