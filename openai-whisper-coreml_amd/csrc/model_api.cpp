// model_api.cpp -- boundary #2 of the C ABI (include/whisper_mi355x.h): weight loading, the
// encoder / decoder entry points that replace the CoreML `encoder` / `decoder` classes
// (Whisper/Whisper/Whisper.swift:17-40), language identification, word-level alignment and window sets.  The transcribe
// calls live in transcribe.cpp.  (The per-kernel test hooks live in debug_hooks.cpp, which is NOT part of the product library.)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "call_src.h"
#include "model.h"

static int io_stage(wm_ctx *ctx, size_t bytes, char **out) {
    WM_TRY(ctx->model->io_stage.reserve(ctx->stream, bytes));
    *out = (char *)ctx->model->io_stage.p;
    return WM_OK;
}

extern "C" int wm_set_tensor(wm_ctx *ctx, const char *name, const float *data, size_t n) try {
    WM_MODEL(ctx);
    (void)m;
    return wm_model_set_tensor(ctx, name, data, n);
} WM_API_CATCH
extern "C" int wm_get_tensor(wm_ctx *ctx, const char *name, float *data, size_t n) try {
    WM_MODEL(ctx);
    (void)m;
    return wm_model_get_tensor(ctx, name, data, n);
} WM_API_CATCH
extern "C" int wm_init_synthetic(wm_ctx *ctx, uint64_t seed) try {
    WM_MODEL(ctx);
    (void)m;
    return wm_model_init_synthetic(ctx, seed, 1.0f);
} WM_API_CATCH
extern "C" int wm_init_synthetic_gain(wm_ctx *ctx, uint64_t seed, float matrix_gain) try {
    WM_MODEL(ctx);
    (void)m;
    WM_REQUIRE(matrix_gain > 0.f && matrix_gain <= 64.f, WM_ERR_INVALID, "init_synthetic_gain: gain must be in (0, 64]");
    return wm_model_init_synthetic(ctx, seed, matrix_gain);
} WM_API_CATCH
extern "C" int wm_finalize(wm_ctx *ctx) try {
    WM_MODEL(ctx);
    (void)m;
    return wm_model_finalize(ctx);
} WM_API_CATCH
extern "C" int wm_set_suppress(wm_ctx *ctx, const int32_t *suppress, int n, const int32_t *suppress_first, int n_first) try {
    WM_MODEL(ctx);
    (void)m;
    return wm_for_each_lane(ctx, true, [&](wm_ctx *c) { return wm_model_set_suppress(c, suppress, n, suppress_first, n_first); });
} WM_API_CATCH
extern "C" int wm_set_timestamp_rules(wm_ctx *ctx, int enable, int32_t timestamp_begin, int32_t eot,
                                      int32_t max_initial_timestamp_index) try {
    WM_MODEL(ctx);
    (void)m;
    return wm_for_each_lane(ctx, true, [&](wm_ctx *c) {
        return wm_model_set_timestamp_rules(c, enable, timestamp_begin, eot, max_initial_timestamp_index);
    });
} WM_API_CATCH
extern "C" int wm_set_repetition_rules(wm_ctx *ctx, float repetition_penalty, int no_repeat_ngram_size, int32_t eot) try {
    WM_MODEL(ctx);
    (void)m;
    return wm_for_each_lane(ctx, true, [&](wm_ctx *c) {
        return wm_model_set_repetition_rules(c, repetition_penalty, no_repeat_ngram_size, eot);
    });
} WM_API_CATCH
extern "C" int wm_set_sampling_rules(wm_ctx *ctx, int top_k, float top_p, float min_p) try {
    WM_MODEL(ctx);
    (void)m;
    WM_REQUIRE(top_k >= 0, WM_ERR_INVALID, "sampling rules: top_k %d is negative (0: off)", top_k);
    WM_REQUIRE(top_p > 0.f && top_p <= 1.f, WM_ERR_INVALID, "sampling rules: top_p must lie in (0, 1] (1: off)");   // (a NaN fails it)
    WM_REQUIRE(min_p >= 0.f && min_p < 1.f, WM_ERR_INVALID, "sampling rules: min_p must lie in [0, 1) (0: off)");
    return wm_for_each_lane(ctx, true, [&](wm_ctx *c) { return wm_model_set_sampling_rules(c, top_k, top_p, min_p); });
} WM_API_CATCH
// The table of wm_set_sequence_bias, checked and expanded: given sequences in order, each followed by its implicit prefix
// entries (shortest first); implicit entries with identical tokens merged into the first of them with the maximum bias, an
// implicit entry identical to a given sequence dropped; then a STABLE sort by last token, so that the entries of one id are a
// contiguous group in table order -- the order of the f32 sum.  Contexts are stored newest token first.
int wm_sb_expand(const int32_t *tokens, const int32_t *seq_offsets, const float *bias, const uint8_t *boost_prefixes, int n_seq,
                 int32_t eot, int n_vocab, WmSbTable *out) {
    *out = WmSbTable();
    WM_REQUIRE(n_seq >= 0, WM_ERR_INVALID, "sequence bias: n_seq %d", n_seq);
    WM_REQUIRE(eot >= 0 && eot <= n_vocab, WM_ERR_INVALID, "sequence bias: eot %d outside [0, %d]", eot, n_vocab);
    if (n_seq == 0) return WM_OK;
    WM_REQUIRE(tokens && seq_offsets && bias, WM_ERR_INVALID, "sequence bias: null pointer");
    WM_REQUIRE(n_seq <= WM_MAX_BIAS_ENTRIES, WM_ERR_INVALID, "sequence bias: %d sequences, at most %d entries", n_seq, WM_MAX_BIAS_ENTRIES);
    WM_REQUIRE(seq_offsets[0] == 0, WM_ERR_INVALID, "sequence bias: seq_offsets[0] must be 0");
    struct Ent { std::vector<int32_t> tok; float bias; bool given; };
    std::vector<Ent> ents;
    std::map<std::vector<int32_t>, int> given, implicit;   // tokens -> index in ents
    for (int i = 0; i < n_seq; ++i) {
        const long n = (long)seq_offsets[i + 1] - seq_offsets[i];
        WM_REQUIRE(n >= 1 && n <= WM_MAX_BIAS_SEQ_LEN, WM_ERR_INVALID, "sequence bias: sequence %d has %ld tokens (1 .. %d)", i, n,
                   WM_MAX_BIAS_SEQ_LEN);
        const int32_t *t = tokens + seq_offsets[i];
        for (long j = 0; j < n; ++j)
            WM_REQUIRE(t[j] >= 0 && t[j] < n_vocab, WM_ERR_INVALID, "sequence bias: token %d of sequence %d outside [0, %d)", t[j], i, n_vocab);
        WM_REQUIRE(t[n - 1] < eot, WM_ERR_INVALID, "sequence bias: sequence %d ends in %d, not a text id (< %d)", i, t[n - 1], eot);
        WM_REQUIRE(!std::isnan(bias[i]) && bias[i] != INFINITY, WM_ERR_INVALID, "sequence bias: the bias of sequence %d must be finite or -inf", i);
        WM_REQUIRE(!(boost_prefixes && boost_prefixes[i]) || std::isfinite(bias[i]), WM_ERR_INVALID,
                   "sequence bias: sequence %d boosts its prefixes, which needs a finite bias", i);
        std::vector<int32_t> key(t, t + n);
        WM_REQUIRE(given.emplace(key, i).second, WM_ERR_INVALID, "sequence bias: sequence %d repeats an earlier one", i);
    }
    for (int i = 0; i < n_seq; ++i) {
        const int32_t *t = tokens + seq_offsets[i];
        const int n = seq_offsets[i + 1] - seq_offsets[i];
        ents.push_back(Ent{std::vector<int32_t>(t, t + n), bias[i], true});
        if (!(boost_prefixes && boost_prefixes[i])) continue;
        for (int j = 1; j < n; ++j) {
            if (t[j - 1] >= eot) continue;   // (a prefix that ends in a special: only text ids are ever biased)
            std::vector<int32_t> key(t, t + j);
            if (given.count(key)) continue;   // the caller has said what that sequence is worth
            auto it = implicit.find(key);
            if (it != implicit.end()) {
                Ent &e = ents[it->second];
                e.bias = bias[i] > e.bias ? bias[i] : e.bias;
                continue;
            }
            implicit.emplace(key, (int)ents.size());
            ents.push_back(Ent{key, bias[i], false});
        }
    }
    WM_REQUIRE((int)ents.size() <= WM_MAX_BIAS_ENTRIES, WM_ERR_INVALID, "sequence bias: %d entries after the prefix expansion, at most %d",
               (int)ents.size(), WM_MAX_BIAS_ENTRIES);
    std::vector<int> order(ents.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ents[a].tok.back() < ents[b].tok.back(); });
    out->ent_ctx.assign(ents.size() * WM_SB_CTX, 0);
    for (size_t k = 0; k < order.size(); ++k) {
        const Ent &e = ents[order[k]];
        const int n = (int)e.tok.size();
        if (out->grp_id.empty() || out->grp_id.back() != e.tok[n - 1]) {
            out->grp_id.push_back(e.tok[n - 1]);
            out->grp_beg.push_back((int32_t)k);
        }
        out->ent_len.push_back(n - 1);
        out->ent_bias.push_back(e.bias);
        for (int j = 0; j < n - 1; ++j) out->ent_ctx[k * WM_SB_CTX + j] = e.tok[n - 2 - j];
    }
    out->grp_beg.push_back((int32_t)ents.size());
    return WM_OK;
}

extern "C" int wm_set_sequence_bias(wm_ctx *ctx, const int32_t *tokens, const int32_t *seq_offsets, const float *bias,
                                    const uint8_t *boost_prefixes, int n_seq, int32_t eot) try {
    WM_MODEL(ctx);
    // checked and expanded ONCE, before any lane is touched: a refused call leaves the table in force where it was
    WmSbTable t;
    WM_TRY(wm_sb_expand(tokens, seq_offsets, bias, boost_prefixes, n_seq, eot, m->dims.n_vocab, &t));
    WM_REQUIRE(t.n_entries() == 0 || !ctx->dbg_hooks, WM_ERR_STATE, "the sequence bias is not supported by the all-f32 precision path");
    return wm_for_each_lane(ctx, true, [&](wm_ctx *c) { return wm_model_set_sequence_bias(c, t); });
} WM_API_CATCH
// The tables of wm_set_sequence_bias_tables: every table checked and expanded on its own (wm_sb_expand), then concatenated --
// grp_beg shifted by the entries in front, so it is absolute into the pool and one array of n_groups + 1 serves all tables.
int wm_sb_expand_tables(const int32_t *tokens, const int32_t *seq_offsets, const float *bias, const uint8_t *boost_prefixes,
                        const int32_t *table_offsets, int n_tables, int n_seq, int32_t eot, int n_vocab, WmSbPool *out) {
    *out = WmSbPool();
    WM_REQUIRE(n_tables >= 0 && n_tables <= WM_MAX_BIAS_TABLES, WM_ERR_INVALID, "sequence bias tables: %d tables (0 .. %d)", n_tables,
               WM_MAX_BIAS_TABLES);
    WM_REQUIRE(eot >= 0 && eot <= n_vocab, WM_ERR_INVALID, "sequence bias: eot %d outside [0, %d]", eot, n_vocab);
    if (n_tables == 0) return WM_OK;
    WM_REQUIRE(table_offsets, WM_ERR_INVALID, "sequence bias tables: null table_offsets");
    WM_REQUIRE(table_offsets[0] == 0 && table_offsets[n_tables] == n_seq, WM_ERR_INVALID,
               "sequence bias tables: table_offsets must run from 0 to the %d sequences", n_seq);
    for (int t = 0; t < n_tables; ++t)
        WM_REQUIRE(table_offsets[t + 1] >= table_offsets[t], WM_ERR_INVALID, "sequence bias tables: table_offsets decrease at table %d", t);
    WM_REQUIRE(n_seq == 0 || (tokens && seq_offsets && bias), WM_ERR_INVALID, "sequence bias: null pointer");
    WM_REQUIRE(n_seq == 0 || seq_offsets[0] == 0, WM_ERR_INVALID, "sequence bias: seq_offsets[0] must be 0");
    WmSbPool p;
    p.tab_grp.push_back(0);
    p.t.grp_beg.push_back(0);
    std::vector<int32_t> offs;
    for (int t = 0; t < n_tables; ++t) {
        const int s0 = table_offsets[t], n = table_offsets[t + 1] - s0;
        WmSbTable one;
        if (n > 0) {   // the table's own offsets from 0, as wm_set_sequence_bias takes them
            WM_REQUIRE(n <= WM_MAX_BIAS_ENTRIES, WM_ERR_INVALID, "sequence bias: table %d has %d sequences, at most %d entries", t, n,
                       WM_MAX_BIAS_ENTRIES);
            offs.resize((size_t)n + 1);
            for (int i = 0; i <= n; ++i) {
                const long o = (long)seq_offsets[s0 + i] - seq_offsets[s0];
                WM_REQUIRE(o >= 0 && o <= (long)WM_MAX_BIAS_ENTRIES * WM_MAX_BIAS_SEQ_LEN, WM_ERR_INVALID,
                           "sequence bias: seq_offsets of table %d decrease or run away", t);
                offs[i] = (int32_t)o;
            }
            WM_TRY(wm_sb_expand(tokens + seq_offsets[s0], offs.data(), bias + s0, boost_prefixes ? boost_prefixes + s0 : nullptr, n, eot,
                                n_vocab, &one));
        }
        const int e0 = p.t.n_entries();
        WM_REQUIRE(e0 + one.n_entries() <= WM_MAX_BIAS_POOL, WM_ERR_INVALID,
                   "sequence bias tables: more than %d entries after the prefix expansion, all tables together", WM_MAX_BIAS_POOL);
        p.t.grp_id.insert(p.t.grp_id.end(), one.grp_id.begin(), one.grp_id.end());
        for (int g = 0; g < one.n_groups(); ++g) p.t.grp_beg.push_back(e0 + one.grp_beg[g + 1]);
        p.t.ent_len.insert(p.t.ent_len.end(), one.ent_len.begin(), one.ent_len.end());
        p.t.ent_bias.insert(p.t.ent_bias.end(), one.ent_bias.begin(), one.ent_bias.end());
        p.t.ent_ctx.insert(p.t.ent_ctx.end(), one.ent_ctx.begin(), one.ent_ctx.end());
        p.tab_grp.push_back(p.t.n_groups());
    }
    *out = std::move(p);
    return WM_OK;
}

extern "C" int wm_set_sequence_bias_tables(wm_ctx *ctx, const int32_t *tokens, const int32_t *seq_offsets, const float *bias,
                                           const uint8_t *boost_prefixes, const int32_t *table_offsets, int n_tables, int32_t eot) try {
    WM_MODEL(ctx);
    // checked and expanded ONCE, before any lane is touched: a refused call leaves whatever was in force
    WM_REQUIRE(n_tables >= 0 && n_tables <= WM_MAX_BIAS_TABLES, WM_ERR_INVALID, "sequence bias tables: %d tables (0 .. %d)", n_tables,
               WM_MAX_BIAS_TABLES);
    WM_REQUIRE(n_tables == 0 || table_offsets, WM_ERR_INVALID, "sequence bias tables: null table_offsets");
    WM_REQUIRE(n_tables == 0 || table_offsets[n_tables] >= 0, WM_ERR_INVALID, "sequence bias tables: table_offsets end below 0");
    WmSbPool p;
    WM_TRY(wm_sb_expand_tables(tokens, seq_offsets, bias, boost_prefixes, table_offsets, n_tables, n_tables ? table_offsets[n_tables] : 0,
                               eot, m->dims.n_vocab, &p));
    WM_REQUIRE(n_tables == 0 || !ctx->dbg_hooks, WM_ERR_STATE, "the sequence bias is not supported by the all-f32 precision path");
    return wm_for_each_lane(ctx, true, [&](wm_ctx *c) { return wm_model_set_sequence_bias_tables(c, p); });
} WM_API_CATCH
// The two i32 row maps of WmModel::pending: a bad list; n == 0 drops the pending map; what must be in force; every value in
// [-1, hi).  A refused call leaves the pending map as it was.
static int set_row_map(std::vector<int32_t> *map, const char *who, const int32_t *v, int n, bool in_force, const char *needs,
                       const char *what, int hi) {
    WM_REQUIRE(n >= 0 && (n == 0 || v), WM_ERR_INVALID, "%s: bad list", who);
    WM_REQUIRE(n == 0 || in_force, WM_ERR_STATE, "%s: the context has no %s", who, needs);
    for (int i = 0; i < n; ++i) WM_REQUIRE(v[i] >= -1 && v[i] < hi, WM_ERR_INVALID, "%s: %s %d of row %d outside [-1, %d)", who, what, v[i], i, hi);
    map->assign(v, v + n);
    return WM_OK;
}
extern "C" int wm_set_bias_rows(wm_ctx *ctx, const int32_t *table_of_row, int n) try {
    WM_MODEL(ctx);
    return set_row_map(&m->pending.bias_rows, "set_bias_rows", table_of_row, n, m->sbt_on,
                       "sequence-bias tables (wm_set_sequence_bias_tables)", "table", (int)m->sbt_tab_grp.size() - 1);
} WM_API_CATCH
extern "C" int wm_set_constraint(wm_ctx *ctx, const int32_t *edge_beg, const int32_t *edge_tok, const int32_t *edge_next,
                                 const int32_t *def_next, const uint8_t *accept, int n_states, int32_t eot) try {
    WM_MODEL(ctx);
    // checked and packed ONCE, before any lane is touched: a refused call leaves the automaton in force where it was
    WmCstTable t;
    WM_TRY(wm_cst_build(edge_beg, edge_tok, edge_next, def_next, accept, n_states, eot, m->dims.n_vocab, &t));
    WM_REQUIRE(t.n_states() == 0 || !ctx->dbg_hooks, WM_ERR_STATE, "the constraint is not supported by the all-f32 precision path");
    return wm_for_each_lane(ctx, true, [&](wm_ctx *c) { return wm_model_set_constraint(c, t); });
} WM_API_CATCH
extern "C" int wm_set_constraint_rows(wm_ctx *ctx, const int32_t *start_of_row, int n) try {
    WM_MODEL(ctx);
    return set_row_map(&m->pending.cst_rows, "set_constraint_rows", start_of_row, n, m->cst_on, "automaton (wm_set_constraint)",
                       "start state", m->cst_states);
} WM_API_CATCH
extern "C" int wm_set_sampling_rows(wm_ctx *ctx, const float *temperature, const uint64_t *seed, int n) try {
    WM_MODEL(ctx);
    m->pending.samp_T.clear(); m->pending.samp_seed.clear();   // whatever happens below, the map that was pending is gone
    WM_REQUIRE(n >= 0 && (n == 0 || (temperature && seed)), WM_ERR_INVALID, "set_sampling_rows: bad list");
    for (int i = 0; i < n; ++i) {
        const float T = temperature[i];
        WM_REQUIRE(std::isfinite(T) && T >= 0.f, WM_ERR_INVALID, "set_sampling_rows: temperature of row %d must be finite and >= 0", i);
        // (1 / T must be a finite f32 too: an infinite scale turns a zero logit's score into NaN)
        WM_REQUIRE(T == 0.f || std::isfinite((float)(1.0 / (double)T)), WM_ERR_INVALID,
                   "set_sampling_rows: temperature %g of row %d is too small: 1 / T overflows", (double)T, i);
    }
    m->pending.samp_T.assign(temperature, temperature + n); m->pending.samp_seed.assign(seed, seed + n);
    return WM_OK;
} WM_API_CATCH
extern "C" int wm_set_teacher_panel(wm_ctx *ctx, int width) try {
    WM_MODEL(ctx);
    (void)m;
    WM_REQUIRE(width >= 1 && width <= WM_MAX_TEACHER_PANEL, WM_ERR_INVALID, "set_teacher_panel: width %d outside [1, %d]", width,
               WM_MAX_TEACHER_PANEL);
    return wm_for_each_lane(ctx, true, [&](wm_ctx *c) { c->model->teacher_panel = width; return (int)WM_OK; });
} WM_API_CATCH
extern "C" int wm_set_prompt_panel(wm_ctx *ctx, int width) try {
    WM_MODEL(ctx);
    (void)m;
    WM_REQUIRE(width >= 1 && width <= WM_MAX_TEACHER_PANEL, WM_ERR_INVALID, "set_prompt_panel: width %d outside [1, %d]", width,
               WM_MAX_TEACHER_PANEL);
    return wm_for_each_lane(ctx, true, [&](wm_ctx *c) { c->model->prompt_panel = width; return (int)WM_OK; });
} WM_API_CATCH
extern "C" int wm_set_given_panel(wm_ctx *ctx, int width) try {
    WM_MODEL(ctx);
    (void)m;
    WM_REQUIRE(width >= 1 && width <= WM_MAX_TEACHER_PANEL, WM_ERR_INVALID, "set_given_panel: width %d outside [1, %d]", width,
               WM_MAX_TEACHER_PANEL);
    return wm_for_each_lane(ctx, true, [&](wm_ctx *c) { c->model->given_panel = width; return (int)WM_OK; });
} WM_API_CATCH
extern "C" int wm_set_lanes(wm_ctx *ctx, int n_lanes) try {
    WM_REQUIRE(ctx, WM_ERR_INVALID, "null context");
    WM_REQUIRE(n_lanes >= 0 && n_lanes <= 8, WM_ERR_INVALID, "set_lanes: 0 (default) .. 8");
    ctx->max_lanes = n_lanes;
    return WM_OK;
} WM_API_CATCH
extern "C" int wm_get_dims(const wm_ctx *ctx, wm_dims *out) try {
    WM_REQUIRE(ctx && out, WM_ERR_INVALID, "null pointer");
    WM_REQUIRE(ctx->model, WM_ERR_STATE, "context has no model");
    *out = ctx->model->dims;
    return WM_OK;
} WM_API_CATCH

// Flat weight file (format: the docstring of openai-whisper-coreml_amd/weights.py).
extern "C" int wm_load_weights(wm_ctx *ctx, const char *path) try {
    WM_MODEL(ctx);
    WM_REQUIRE(path, WM_ERR_INVALID, "null path");
    FILE *f = fopen(path, "rb");
    WM_REQUIRE(f, WM_ERR_IO, "cannot open '%s'", path);
    int st = WM_OK;
    char magic[8];
    int32_t dims[10], count = 0;
    std::vector<float> buf;
    std::vector<char> name;
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "WMI355X1", 8) != 0 || fread(dims, 4, 10, f) != 10 ||
        fread(&count, 4, 1, f) != 1) {
        wm_set_error("'%s' is not a WMI355X1 weight file", path);
        st = WM_ERR_IO;
    }
    if (st == WM_OK && memcmp(dims, &m->dims, sizeof(wm_dims)) != 0) {
        wm_set_error("'%s': model dimensions differ from the context's", path);
        st = WM_ERR_IO;
    }
    if (st == WM_OK && count <= 0) {
        wm_set_error("'%s': tensor count %d", path, count);
        st = WM_ERR_IO;
    }
    for (int i = 0; st == WM_OK && i < count; ++i) {
        int32_t nl = 0;
        int64_t ne = 0;
        if (fread(&nl, 4, 1, f) != 1 || nl <= 0 || nl > 4096) { wm_set_error("'%s': truncated", path); st = WM_ERR_IO; break; }
        name.assign(nl + 1, 0);
        if (fread(name.data(), 1, nl, f) != (size_t)nl || fread(&ne, 8, 1, f) != 1 || ne <= 0) {
            wm_set_error("'%s': truncated", path); st = WM_ERR_IO; break;
        }
        // the element count comes from the file: check it against the registered tensor BEFORE allocating
        auto it = m->index.find(name.data());
        if (it == m->index.end()) { wm_set_error("'%s': unknown tensor '%s'", path, name.data()); st = WM_ERR_IO; break; }
        if ((uint64_t)ne != (uint64_t)m->tensors[it->second].n_elems) {
            wm_set_error("'%s': tensor '%s' has %lld elements, %zu expected", path, name.data(), (long long)ne,
                         m->tensors[it->second].n_elems);
            st = WM_ERR_IO;
            break;
        }
        buf.resize((size_t)ne);
        if (fread(buf.data(), 4, (size_t)ne, f) != (size_t)ne) { wm_set_error("'%s': truncated", path); st = WM_ERR_IO; break; }
        st = wm_model_set_tensor(ctx, name.data(), buf.data(), (size_t)ne);
    }
    fclose(f);
    return st;
} WM_API_CATCH

// ------------------------------------------------------------------ encoder ------------
extern "C" int wm_encode(wm_ctx *ctx, const float *mel, int B, float *xa, wm_mem mem) try {
    WM_MODEL(ctx);
    WM_REQUIRE(mel && xa && B >= 1, WM_ERR_INVALID, "null pointer / B < 1");
    const auto encode_dev = ctx->dbg_hooks ? ctx->dbg_hooks->encode_dev : wm_model_encode_dev;   // null hooks in the product
    if (mem == WM_MEM_DEVICE) return encode_dev(ctx, mel, B, xa);
    const size_t in_b = (size_t)B * m->dims.n_mels * WM_N_FRAMES * 4;
    const size_t out_b = (size_t)B * 1500 * m->dims.n_audio_state * 4;
    char *st;
    WM_TRY(io_stage(ctx, in_b + out_b, &st));
    WM_HIP(hipMemcpyAsync(st, mel, in_b, hipMemcpyHostToDevice, ctx->stream));
    WM_TRY(encode_dev(ctx, (const float *)st, B, (float *)(st + in_b)));
    WM_HIP(hipMemcpyAsync(xa, st + in_b, out_b, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    return WM_OK;
} WM_API_CATCH

// ------------------------------------------------------------------ decoder ------------
// Shared: bring xa (f32 [B][1500][d], host or device) into the bf16 encoder-output buffer
// and build the cross-attention K/V cache.
static int load_xa(wm_ctx *ctx, const float *xa, int B, wm_mem mem) {
    WmModel *m = ctx->model;
    const size_t bytes = (size_t)B * 1500 * m->dims.n_audio_state * 4;
    const float *d_xa = xa;
    if (mem == WM_MEM_HOST) {
        char *st;
        WM_TRY(io_stage(ctx, bytes, &st));
        WM_HIP(hipMemcpyAsync(st, xa, bytes, hipMemcpyHostToDevice, ctx->stream));
        d_xa = (const float *)st;
    }
    WM_TRY(wm_model_set_xa(ctx, d_xa, B));
    return wm_model_cross_kv(ctx, B);
}

// wm_decode_logits at a panel width > 1 (wm_set_teacher_panel): slices of windows, each walking its panels from position 0;
// the logits of row (c, s) of a panel at position t go to out [B][T][V] at [c0 + c][t + s] (strided copies)
static int logits_in_panels(wm_ctx *ctx, int B, int T, int width, float *d_out) {
    WmModel *m = ctx->model;
    const int V = m->dims.n_vocab;
    int Cs = 0, w = 0;
    wm_model_panel_slices(B, width, T, &Cs, &w);
    for (int c0 = 0; c0 < B; c0 += Cs) {
        const int C = std::min(Cs, B - c0);
        if (c0 > 0) WM_TRY(wm_model_set_pos(ctx, 0));
        WM_TRY(wm_model_panel_embed(ctx, B, c0, C, std::min(w, T)));
        for (int t = 0; t < T; t += w) {
            const int wp = std::min(w, T - t);
            WM_TRY(wm_model_panel_step(ctx, B, c0, C, wp, true, nullptr));
            for (int s = 0; s < wp; ++s)
                WM_HIP(hipMemcpy2DAsync(d_out + ((size_t)c0 * T + t + s) * V, (size_t)T * V * 4, m->dlogits + (size_t)s * m->vpad,
                                        (size_t)wp * m->vpad * 4, (size_t)V * 4, C, hipMemcpyDeviceToDevice, ctx->stream));
            if (t + wp < T) WM_TRY(wm_model_panel_advance(ctx, B, c0, C, wp, std::min(w, T - t - wp)));
        }
    }
    return WM_OK;
}

extern "C" int wm_decode_logits(wm_ctx *ctx, const int32_t *tokens, int B, int T, const float *xa,
                                float *logits, wm_mem mem) try {
    WM_MODEL(ctx);
    WM_REQUIRE(tokens && xa && logits, WM_ERR_INVALID, "null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB, WM_ERR_INVALID, "B must be 1..%d", WM_DEC_MAXB);
    WM_REQUIRE(T >= 1 && T <= m->dims.n_text_ctx, WM_ERR_INVALID, "T must be 1..%d", m->dims.n_text_ctx);
    const int V = m->dims.n_vocab;
    // tokens arrive [B][T]; the step kernel wants the B tokens of one position contiguous
    std::vector<int32_t> host_tok((size_t)B * T);
    if (mem == WM_MEM_DEVICE) {
        WM_HIP(hipMemcpy(host_tok.data(), tokens, host_tok.size() * 4, hipMemcpyDeviceToHost));
    } else {
        memcpy(host_tok.data(), tokens, host_tok.size() * 4);
    }
    std::vector<int32_t> tb((size_t)T * B);
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T; ++t) {
            const int32_t tok = host_tok[(size_t)b * T + t];
            WM_REQUIRE(tok >= 0 && tok < V, WM_ERR_INVALID, "token id %d outside [0, %d)", tok, V);
            tb[(size_t)t * B + b] = tok;
        }
    if (ctx->dbg_hooks) {   // debug library only: the all-fp32 path (xa stays f32, no K/V cache, no bf16 anywhere)
        const float *d_xa = xa;
        float *d_out = logits;
        char *st = nullptr;
        const size_t xa_b = (size_t)B * 1500 * m->dims.n_audio_state * 4, out_b = (size_t)B * T * V * 4;
        if (mem == WM_MEM_HOST) {
            WM_TRY(io_stage(ctx, ((xa_b + 255) & ~(size_t)255) + out_b, &st));
            WM_HIP(hipMemcpyAsync(st, xa, xa_b, hipMemcpyHostToDevice, ctx->stream));
            d_xa = (const float *)st;
            d_out = (float *)(st + ((xa_b + 255) & ~(size_t)255));
        }
        WM_TRY(ctx->dbg_hooks->decode_logits_dev(ctx, host_tok.data(), B, T, d_xa, d_out));
        if (mem == WM_MEM_HOST) {
            WM_HIP(hipMemcpyAsync(logits, d_out, out_b, hipMemcpyDeviceToHost, ctx->stream));
            WM_HIP(hipStreamSynchronize(ctx->stream));
        }
        return WM_OK;
    }
    WM_TRY(wm_model_decode_begin(ctx, B));
    WM_TRY(load_xa(ctx, xa, B, mem));
    WM_HIP(hipMemcpyAsync(m->dseq, tb.data(), tb.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));  // fences `tb`
    WM_TRY(wm_model_set_pos(ctx, 0));
    const int width = m->teacher_panel;   // wm_set_teacher_panel: > 1 = the pass in panels (same bits, fewer launches)
    if (width == 1) WM_TRY(wm_model_embed_first(ctx, B));
    float *d_out = logits;
    char *st = nullptr;
    if (mem == WM_MEM_HOST) {
        // io_stage currently holds xa (already consumed into bf16 by load_xa on this stream)
        WM_HIP(hipMalloc((void **)&st, (size_t)B * T * V * 4));
        d_out = (float *)st;
    }
    int rc = WM_OK;
    if (width > 1) rc = logits_in_panels(ctx, B, T, width, d_out);
    else for (int t = 0; t < T && rc == WM_OK; ++t) {
        rc = wm_model_decode_step(ctx, B, true, 0, V - 1);
        if (rc != WM_OK) break;
        // dlogits [B][vpad] -> out [B][T][V], row t
        if (hipMemcpy2DAsync(d_out + (size_t)t * V, (size_t)T * V * 4, m->dlogits, (size_t)m->vpad * 4,
                             (size_t)V * 4, B, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
            wm_set_error("hipMemcpy2DAsync failed");
            rc = WM_ERR_HIP;
            break;
        }
        // teacher forcing: every position < T is "prompt", so the given tokens are kept; this
        // embeds position t+1 and advances the device-side position
        rc = wm_model_close_step(ctx, B, T, true, nullptr, 0);
    }
    if (rc == WM_OK && mem == WM_MEM_HOST) {
        if (hipMemcpyAsync(logits, d_out, (size_t)B * T * V * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
            wm_set_error("hipMemcpyAsync D2H failed");
            rc = WM_ERR_HIP;
        }
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == WM_OK) {
        wm_set_error("stream sync failed: %s", hipGetErrorString(hipGetLastError()));
        rc = WM_ERR_HIP;
    }
    if (st) (void)hipFree(st);
    return rc;
} WM_API_CATCH

static int detect_language_impl(wm_ctx *ctx, const float *xa, int B, int32_t sot, int32_t lang_first, int32_t lang_last,
                                int32_t *lang_idx, float *probs, wm_mem mem, const wm_windows *set = nullptr,
                                const int32_t *rows = nullptr);

extern "C" int wm_detect_language(wm_ctx *ctx, const float *xa, int B, int32_t sot, int32_t lang_first,
                                  int32_t lang_last, int32_t *lang_idx, wm_mem mem) try {
    return detect_language_impl(ctx, xa, B, sot, lang_first, lang_last, lang_idx, nullptr, mem);
} WM_API_CATCH

extern "C" int wm_detect_language_probs(wm_ctx *ctx, const float *xa, int B, int32_t sot, int32_t lang_first,
                                        int32_t lang_last, int32_t *lang_idx, float *probs, wm_mem mem) try {
    WM_REQUIRE(probs != nullptr, WM_ERR_INVALID, "null pointer");
    return detect_language_impl(ctx, xa, B, sot, lang_first, lang_last, lang_idx, probs, mem);
} WM_API_CATCH

// (set: the features are rows of a window set -- wm_windows_detect_language, below the audio-source helpers -- and xa is null)
static int windows_cross_kv(wm_ctx *ctx, const wm_windows *set, const int32_t *rows, int B, std::vector<int32_t> &map);

static int detect_language_impl(wm_ctx *ctx, const float *xa, int B, int32_t sot, int32_t lang_first, int32_t lang_last,
                                int32_t *lang_idx, float *probs, wm_mem mem, const wm_windows *set, const int32_t *rows) {
    WM_MODEL(ctx);
    WM_REQUIRE((xa || set) && lang_idx, WM_ERR_INVALID, "null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB, WM_ERR_INVALID, "B must be 1..%d", WM_DEC_MAXB);
    const int V = m->dims.n_vocab;
    WM_REQUIRE(sot >= 0 && sot < V && lang_first >= 0 && lang_first <= lang_last && lang_last < V, WM_ERR_INVALID,
               "token ids outside the vocabulary (n_vocab = %d)", V);
    WM_TRY(wm_model_decode_begin(ctx, B));
    // (round 6: one stream, no host synchronisation until the result is wanted -- the <|startoftranscript|> row is staged in
    // a buffer that outlives the call, uploaded FIRST, and the features' K/V GEMMs + the decoder step are enqueued behind it)
    m->lid_host.assign(B, sot);  // Whisper.swift:34-35
    WM_HIP(hipMemcpyAsync(m->dseq, m->lid_host.data(), (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
    std::vector<int32_t> map;   // a set's row map, the source of an asynchronous upload: error paths must not outlive it
    WmStreamFence fence{ctx->stream, set != nullptr};
    WmEvents<3> ev;
    if (set) {
        WM_TRY(ev.create());
        WM_HIP(hipEventRecord(ev[0], ctx->stream));
        WM_TRY(windows_cross_kv(ctx, set, rows, B, map));
        WM_HIP(hipEventRecord(ev[1], ctx->stream));
    } else {
        WM_TRY(load_xa(ctx, xa, B, mem));
    }
    WM_TRY(wm_model_set_pos(ctx, 0));
    WM_TRY(wm_model_embed_first(ctx, B));
    auto step = [&]() -> int {
        WM_TRY(wm_model_decode_step(ctx, B, probs != nullptr, lang_first, lang_last));     // :36-37
        // the arg-max alone: no token buffer, no position, nothing embedded, every rule off
        return wm_argmax_embed(ctx, m->dargmax, m->vpad / 16, B, nullptr, nullptr, 0, m->dresult, lang_first, 0, WmEmbedDev{},
                               WmTsDev{}, m->darrive, lang_first, WmStopDev{}, WmXDev{}, nullptr);  // :38
    };
    if (wm_graphs_off() || ctx->prof.on) {
        WM_TRY(step());
    } else {
        WmModel::LidGraph &lg = m->lid_graph;
        const int want = probs != nullptr ? 1 : 0;
        if (!lg.graph.e || lg.B != B || lg.cap_b != m->cap_b || lg.first != lang_first || lg.last != lang_last || lg.logits != want) {
            lg.destroy();
            WM_TRY(wm_capture_graph(ctx->stream, &lg.graph, "the language-identification step", step));
            lg.B = B; lg.cap_b = m->cap_b; lg.first = lang_first; lg.last = lang_last; lg.logits = want;
        }
        WM_HIP(hipGraphLaunch(lg.graph.e, ctx->stream));
    }
    if (probs) {  // openai-whisper detect_language(): softmax over the language-token logits only
        const int n_lang = lang_last - lang_first + 1;
        float *d_probs = probs;
        char *st = nullptr;
        if (mem == WM_MEM_HOST) {
            WM_TRY(io_stage(ctx, (size_t)B * n_lang * 4, &st));
            d_probs = (float *)st;
        }
        WM_TRY(wm_range_softmax(ctx, m->dlogits, m->vpad, B, lang_first, n_lang, d_probs));
        if (mem == WM_MEM_HOST)
            WM_HIP(hipMemcpyAsync(probs, d_probs, (size_t)B * n_lang * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    // (the caller's buffer in device memory: one device-to-device copy behind the step)
    if (set) WM_HIP(hipEventRecord(ev[2], ctx->stream));
    WM_HIP(hipMemcpyAsync(lang_idx, m->dresult, (size_t)B * 4, mem == WM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    if (set) {   // wm_last_stage_ms of a call that read a set: the gather, no encoder stage, the decoder step
        float ms;
        ctx->stage_ms[0] = ctx->stage_ms[1] = ctx->stage_ms[2] = 0.f;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) ctx->stage_ms[0] = ms;
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) ctx->stage_ms[2] = ms;
    }
    return WM_OK;
}

extern "C" int wm_set_token_budgets(wm_ctx *ctx, const int32_t *budgets, int n) try {
    WM_MODEL(ctx);
    WM_REQUIRE(n >= 0 && (n == 0 || budgets), WM_ERR_INVALID, "set_token_budgets: bad list");
    for (int i = 0; i < n; ++i)
        WM_REQUIRE(budgets[i] >= 1, WM_ERR_INVALID, "set_token_budgets: budget %d of chunk %d is < 1", budgets[i], i);
    m->pending.budgets.assign(budgets, budgets + n);
    return WM_OK;
} WM_API_CATCH

extern "C" int wm_request_alternatives(wm_ctx *ctx, const wm_alternatives_out *req) try {
    WM_MODEL(ctx);
    if (!req) { m->pending.alt_on = false; return WM_OK; }   // (drops a pending request)
    WM_REQUIRE(req->n >= 1 && req->n <= WM_MAX_ALTERNATIVES, WM_ERR_INVALID, "request_alternatives: n %d outside [1, %d]", req->n,
               WM_MAX_ALTERNATIVES);
    WM_REQUIRE(req->tokens && req->logprobs, WM_ERR_INVALID, "request_alternatives: null tokens / logprobs");
    WM_REQUIRE(req->rows >= 1 && req->max_new >= 1, WM_ERR_INVALID, "request_alternatives: rows or max_new below 1");
    m->pending.alt = *req; m->pending.alt_on = true;
    return WM_OK;
} WM_API_CATCH

extern "C" int wm_set_given_tokens(wm_ctx *ctx, const int32_t *tokens, int stride, const int32_t *lens, int n) try {
    WM_MODEL(ctx);
    WmPending &p = m->pending;
    p.given_lens.clear(); p.given_tok.clear(); p.given_stride = 0;   // whatever happens below, the table that was pending is gone
    if (n == 0) return WM_OK;
    WM_REQUIRE(n > 0 && stride >= 1 && tokens && lens, WM_ERR_INVALID, "set_given_tokens: bad table");
    for (int r = 0; r < n; ++r) {
        WM_REQUIRE(lens[r] >= 0 && lens[r] <= stride, WM_ERR_INVALID, "set_given_tokens: row %d has %d tokens, outside [0, %d]", r, lens[r],
                   stride);
        for (int i = 0; i < lens[r]; ++i) {
            const int32_t t = tokens[(size_t)r * stride + i];
            WM_REQUIRE(t >= 0 && t < m->dims.n_vocab, WM_ERR_INVALID, "set_given_tokens: row %d token %d: id %d outside the vocabulary", r, i, t);
        }
    }
    p.given_lens.assign(lens, lens + n);
    p.given_tok.assign(tokens, tokens + (size_t)n * stride);
    p.given_stride = stride;
    return WM_OK;
} WM_API_CATCH

// ---------------------------------------------------------------- word-level timestamps
// openai-whisper's find_alignment (whisper/timing.py): a teacher-forced decoder pass that captures the alignment heads'
// cross-attention queries, then the alignment kernels and DTW of align.hip.
extern "C" int wm_set_alignment_heads(wm_ctx *ctx, const int32_t *layers, const int32_t *heads, int n) try {
    WM_MODEL(ctx);
    WM_REQUIRE(n >= 0 && (n == 0 || (layers && heads)), WM_ERR_INVALID, "set_alignment_heads: bad list");
    const int L = m->dims.n_text_layer, H = m->dims.n_text_head;
    std::vector<std::pair<int32_t, int32_t>> v;
    for (int i = 0; i < n; ++i) {
        WM_REQUIRE(layers[i] >= 0 && layers[i] < L && heads[i] >= 0 && heads[i] < H, WM_ERR_INVALID,
                   "set_alignment_heads: (%d, %d) outside %d layers x %d heads", layers[i], heads[i], L, H);
        v.emplace_back(layers[i], heads[i]);
    }
    std::sort(v.begin(), v.end());
    for (size_t i = 1; i < v.size(); ++i)
        WM_REQUIRE(v[i] != v[i - 1], WM_ERR_INVALID, "set_alignment_heads: (%d, %d) listed twice", v[i].first, v[i].second);
    std::vector<int32_t> hl, hh;
    for (auto &p : v) { hl.push_back(p.first); hh.push_back(p.second); }
    // (an aligned transcribe group's captured positions hold the head list in their launches: they are captured afresh)
    return wm_for_each_lane(ctx, true, [&](wm_ctx *c) {
        c->model->align_l = hl; c->model->align_h = hh;
        std::vector<WmModel::GraphSet> &gs = c->model->graph_sets;
        for (size_t i = gs.size(); i-- > 0;)
            if (gs[i].mode.acap) { gs[i].destroy(); gs.erase(gs.begin() + (long)i); }
        return (int)WM_OK;
    });
} WM_API_CATCH

void wm_align_heads(const WmModel *m, std::vector<int32_t> *hl, std::vector<int32_t> *hh) {
    if (!m->align_l.empty()) {
        *hl = m->align_l;
        *hh = m->align_h;
        return;
    }
    hl->clear();
    hh->clear();
    const wm_dims &D = m->dims;   // openai-whisper's default: every head of the last half of the decoder layers
    for (int l = D.n_text_layer / 2; l < D.n_text_layer; ++l)
        for (int h = 0; h < D.n_text_head; ++h) { hl->push_back(l); hh->push_back(h); }
}

namespace {
size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// an align call's encoder input -- PCM chunks (wm_align; n_frames nullable: whole chunks) or mel windows (wm_align_mel) --
// and its start sequences: row b's is sot_seq + b * sot_stride (0: one for all)
struct AlignCall : WmAudioSrc {
    wm_mem mem;
    const int32_t *sot_seq, *text_tokens, *n_text;
    int sot_stride = 0;
    int n_sot, max_text;
    int32_t no_timestamps, eot;
    int half;
    float qk_scale;
    int32_t *start_out;
    float *prob_out, *dbg_matrix;
    std::vector<int32_t> hl, hh;
};

// one decode group: chunks [b0, b0 + Bg) of the call
int align_group(wm_ctx *ctx, const AlignCall &c, int b0, int Bg, const WmEvents<4> &ev) {
    WmModel *m = ctx->model;
    const wm_dims &D = m->dims;
    const int S = c.n_sot, J = (int)c.hl.size(), n_ld = c.max_text + 1, V = D.n_vocab;
    int nmax = 0, mmax = 0;
    for (int b = 0; b < Bg; ++b) {
        nmax = std::max(nmax, (int)c.n_text[b0 + b]);
        mmax = std::max(mmax, (c.n_frames ? (int)c.n_frames[b0 + b] : WM_N_FRAMES) / 2);
    }
    if (nmax == 0) return WM_OK;   // outputs stay -1 / 0
    const int T = S + nmax + 2;
    // workspace
    const size_t o_q = 0, o_row = o_q + align_up((size_t)Bg * T * J * 64 * 4), o_col = o_row + align_up((size_t)Bg * J * T * 8);
    const size_t o_x = o_col + align_up((size_t)Bg * J * 1500 * 8), o_tr = o_x + align_up((size_t)Bg * n_ld * 1500 * 4);
    const size_t o_prob = o_tr + align_up((size_t)Bg * wm_dtw_trace_words(n_ld) * 4);
    const size_t o_start = o_prob + align_up((size_t)Bg * std::max(c.max_text, 1) * 4);
    const size_t o_int = o_start + align_up((size_t)Bg * n_ld * 4), n_int = (size_t)4 * Bg + 2 * J;
    const size_t bytes = o_int + align_up(n_int * 4);
    WM_TRY(m->align_ws.reserve(ctx->stream, bytes));
    char *ws = (char *)m->align_ws.p;
    float *q = (float *)(ws + o_q), *x = (float *)(ws + o_x), *prob = (float *)(ws + o_prob);
    int *start = (int *)(ws + o_start), *ints = (int *)(ws + o_int);
    // host staging (fenced by the synchronisation at the end of the group): n_text, n_frames, DTW rows, DTW frames, heads
    std::vector<int32_t> hint(n_int), seq((size_t)T * Bg);
    std::vector<WmMelWin> win;
    std::vector<int32_t> xrows;
    for (int b = 0; b < Bg; ++b) {
        const int n = c.n_text[b0 + b], nf = c.n_frames ? c.n_frames[b0 + b] : WM_N_FRAMES;
        hint[b] = n;
        hint[Bg + b] = nf;
        hint[2 * Bg + b] = n > 0 ? n + 1 : 0;
        hint[3 * Bg + b] = nf / 2;
        const int32_t *t = c.text_tokens + (size_t)(b0 + b) * c.max_text;
        const int32_t *sot = c.sot_seq + (size_t)(b0 + b) * c.sot_stride;
        for (int p = 0; p < T; ++p) {   // [*sot_seq, no_timestamps, *t, eot, eot ...] (padding after eot: causal, unread)
            const int32_t tok = p < S ? sot[p] : p == S ? c.no_timestamps : p <= S + n ? t[p - S - 1] : c.eot;
            seq[(size_t)p * Bg + b] = tok;
        }
    }
    for (int j = 0; j < J; ++j) { hint[4 * Bg + j] = c.hl[j]; hint[4 * Bg + J + j] = c.hh[j]; }
    WmStreamFence fence{ctx->stream};   // error paths: no copy from seq / hint may outlive them
    // decode state, then the front end -> encoder -> cross K/V of the group
    WM_TRY(wm_model_decode_begin(ctx, Bg));
    WM_HIP(hipMemcpyAsync(m->dseq, seq.data(), seq.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipMemcpyAsync(ints, hint.data(), hint.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(hipMemsetAsync(prob, 0, (size_t)Bg * std::max(c.max_text, 1) * 4, ctx->stream));
    WM_HIP(hipMemsetAsync(x, 0, (size_t)Bg * n_ld * 1500 * 4, ctx->stream));
    WM_TRY(wm_model_set_pos(ctx, 0));
    WM_TRY(wm_model_reserve(ctx, Bg));
    const void *d_pcm;
    WM_TRY(wm_stage_pcm(ctx, c, b0, Bg, c.mem, &d_pcm));
    WM_HIP(hipEventRecord(ev[0], ctx->stream));
    WM_TRY(wm_stage_cross_kv(ctx, c, b0, Bg, c.mem, d_pcm, win, xrows, nullptr));
    WM_HIP(hipEventRecord(ev[1], ctx->stream));
    // teacher-forced pass: every position is prompt, the alignment layers leave their queries in the capture buffer
    std::vector<WmAlignLayer> layers(D.n_text_layer);
    for (int j = 0; j < J; ++j) {
        WmAlignLayer &Ly = layers[c.hl[j]];
        if (Ly.n == 0) Ly.slot0 = j;
        Ly.head[Ly.n++] = c.hh[j];
    }
    const WmAlignCap cap = {layers.data(), q, T, J};
    const int width = m->teacher_panel;   // wm_set_teacher_panel: > 1 = the pass in panels (same bits, ceil(T / w) steps)
    if (width > 1) {
        int Cs = 0, w = 0;
        wm_model_panel_slices(Bg, width, T, &Cs, &w);
        for (int c0 = 0; c0 < Bg; c0 += Cs) {   // a slice walks all its panels, then the next slice starts at position 0
            const int C = std::min(Cs, Bg - c0);
            if (c0 > 0) WM_TRY(wm_model_set_pos(ctx, 0));
            WM_TRY(wm_model_panel_embed(ctx, Bg, c0, C, std::min(w, T)));
            for (int p = 0; p < T; p += w) {
                const int wp = std::min(w, T - p);   // the last panel is narrower: no row ever has a position >= T
                const bool want = p + wp > S && p < S + nmax;   // some row's logits give a token probability
                WM_TRY(wm_model_panel_step(ctx, Bg, c0, C, wp, want, &cap));
                if (want)
                    WM_TRY(wm_align_token_prob(ctx, m->dlogits, m->vpad, m->dseq + c0, m->dpos, C * wp, S, c.eot, ints + c0,
                                               prob + (size_t)c0 * std::max(c.max_text, 1), std::max(c.max_text, 1), wp, Bg));
                if (p + wp < T) WM_TRY(wm_model_panel_advance(ctx, Bg, c0, C, wp, std::min(w, T - p - wp)));
            }
        }
    } else {
        WM_TRY(wm_model_embed_first(ctx, Bg));
        for (int p = 0; p < T; ++p) {
            const bool want = p >= S && p < S + nmax;   // rows whose logits give a token probability
            WM_TRY(wm_model_decode_step(ctx, Bg, want, 0, V - 1, &cap));
            if (want) WM_TRY(wm_align_token_prob(ctx, m->dlogits, m->vpad, m->dseq, m->dpos, Bg, S, c.eot, ints, prob, std::max(c.max_text, 1)));
            if (p + 1 < T) WM_TRY(wm_model_close_step(ctx, Bg, T, true, nullptr, 0));
        }
    }
    WM_HIP(hipEventRecord(ev[2], ctx->stream));
    // alignment kernels and DTW
    WmAlignDev a;
    a.q = q; a.xkv = m->xkv; a.hl = ints + 4 * Bg; a.hh = ints + 4 * Bg + J; a.n_text = ints; a.n_frames = ints + Bg;
    a.rowst = (float *)(ws + o_row); a.colst = (float *)(ws + o_col); a.x = x;
    a.B = Bg; a.H = D.n_text_head; a.Tq = T; a.J = J; a.S = S; a.n_ld = n_ld;
    a.sc = 0.125f * c.qk_scale * 1.44269504088896340736f;
    a.half = c.half;
    WM_TRY(wm_align_matrix(ctx, a, nmax, mmax));
    WM_TRY(wm_dtw(ctx, x, (long)n_ld * 1500, 1500, ints + 2 * Bg, ints + 3 * Bg, Bg, nmax + 1, mmax, (unsigned *)(ws + o_tr),
                  start, n_ld));
    WM_HIP(hipEventRecord(ev[3], ctx->stream));
    WM_HIP(hipMemcpyAsync(c.start_out + (size_t)b0 * n_ld, start, (size_t)Bg * n_ld * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (c.prob_out && c.max_text > 0)
        WM_HIP(hipMemcpyAsync(c.prob_out + (size_t)b0 * c.max_text, prob, (size_t)Bg * c.max_text * 4, hipMemcpyDeviceToHost,
                              ctx->stream));
    if (c.dbg_matrix)
        WM_HIP(hipMemcpyAsync(c.dbg_matrix + (size_t)b0 * n_ld * 1500, x, (size_t)Bg * n_ld * 1500 * 4, hipMemcpyDeviceToHost,
                              ctx->stream));
    WM_HIP(hipStreamSynchronize(ctx->stream));
    wm_add_stage_ms(ev.e, 3, false, ctx->stage_ms);
    return WM_OK;
}
}  // namespace

// wm_align and wm_align_mel behind their own checks of the input source: c carries the source, the start sequences,
// text_tokens, n_text and n_frames
static int align_impl(wm_ctx *ctx, AlignCall &c, int B, int32_t no_timestamps, int32_t eot, int medfilt_width, float qk_scale,
                      int32_t *start_frame_out, float *token_prob_out) {
    WmModel *m = ctx->model;
    const int n_sot = c.n_sot, max_text = c.max_text;
    const int32_t *text_tokens = c.text_tokens, *n_text = c.n_text, *n_frames = c.n_frames;
    const wm_dims &D = m->dims;
    const int V = D.n_vocab;
    WM_REQUIRE(n_sot >= 1 && max_text >= 0 && n_sot + max_text + 2 <= D.n_text_ctx, WM_ERR_INVALID,
               "align: sot_seq (%d) + max_text (%d) + 2 must fit the %d-token context", n_sot, max_text, D.n_text_ctx);
    for (size_t i = 0; i < (size_t)n_sot * (c.sot_stride ? B : 1); ++i)
        WM_REQUIRE(c.sot_seq[i] >= 0 && c.sot_seq[i] < V, WM_ERR_INVALID, "align: sot_seq token %d out of range", c.sot_seq[i]);
    WM_REQUIRE(no_timestamps >= 0 && no_timestamps < V && eot >= 0 && eot < V, WM_ERR_INVALID,
               "align: no_timestamps / eot outside the vocabulary");
    WM_REQUIRE(medfilt_width >= 1 && medfilt_width <= 31 && medfilt_width % 2 == 1, WM_ERR_INVALID,
               "align: medfilt_width %d must be odd, 1 .. 31", medfilt_width);
    WM_REQUIRE(std::isfinite(qk_scale), WM_ERR_INVALID, "align: qk_scale must be finite");
    for (int b = 0; b < B; ++b) {
        WM_REQUIRE(n_text[b] >= 0 && n_text[b] <= max_text, WM_ERR_INVALID, "align: n_text[%d] = %d outside [0, %d]", b,
                   n_text[b], max_text);
        for (int i = 0; i < n_text[b]; ++i) {
            const int32_t t = text_tokens[(size_t)b * max_text + i];
            WM_REQUIRE(t >= 0 && t < eot, WM_ERR_INVALID, "align: text token %d of chunk %d is not a text token (< eot %d)", t,
                       b, eot);
        }
        if (n_frames)
            WM_REQUIRE(n_frames[b] >= 2 && n_frames[b] <= WM_N_FRAMES, WM_ERR_INVALID, "align: n_frames[%d] = %d outside [2, %d]",
                       b, n_frames[b], WM_N_FRAMES);
        if (c.mel) WM_TRY(wm_check_window(c, b, "align: "));
    }
    wm_align_heads(m, &c.hl, &c.hh);
    c.no_timestamps = no_timestamps; c.eot = eot;
    c.half = medfilt_width / 2; c.qk_scale = qk_scale;
    c.start_out = start_frame_out; c.prob_out = token_prob_out;
    const int n_ld = max_text + 1;
    for (size_t i = 0; i < (size_t)B * n_ld; ++i) start_frame_out[i] = -1;
    if (token_prob_out)
        for (size_t i = 0; i < (size_t)B * max_text; ++i) token_prob_out[i] = 0.f;
    if (c.dbg_matrix) memset(c.dbg_matrix, 0, (size_t)B * n_ld * 1500 * 4);
    // decode groups of at most WM_DEC_MAXB chunks, fewer when the captured queries would outgrow the budget
    const int G = wm_align_group_rows((size_t)n_sot + max_text + 2, c.hl.size(), (size_t)n_ld);
    ctx->stage_ms[0] = ctx->stage_ms[1] = ctx->stage_ms[2] = 0.f;
    WmEvents<4> ev;
    WmStreamFence fence{ctx->stream};   // drained before the events go, whatever a group returned
    int rc = ev.create();
    for (int b0 = 0; b0 < B && rc == WM_OK; b0 += G) rc = align_group(ctx, c, b0, std::min(G, B - b0), ev);
    return rc;
}

extern "C" int wm_align(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, int B, const int32_t *sot_seq, int n_sot,
                        int32_t no_timestamps, int32_t eot, const int32_t *text_tokens, const int32_t *n_text, int max_text,
                        const int32_t *n_frames, int medfilt_width, float qk_scale, int32_t *start_frame_out,
                        float *token_prob_out, wm_mem mem) try {
    WM_MODEL(ctx);
    AlignCall c;
    c.dbg_matrix = std::exchange(m->pending.dbg.align_matrix, nullptr);   // the debug library's capture is for this call only
    WM_REQUIRE(m->finalized, WM_ERR_STATE, "model weights not finalised (wm_finalize)");
    WM_REQUIRE(pcm && sot_seq && n_text && start_frame_out && (max_text == 0 || text_tokens), WM_ERR_INVALID, "null pointer");
    WM_REQUIRE(pcm_dtype == WM_I16 || pcm_dtype == WM_F32 || pcm_dtype == WM_F64, WM_ERR_INVALID, "bad pcm dtype");
    WM_REQUIRE(B >= 1, WM_ERR_INVALID, "B < 1");
    c.pcm = pcm; c.pcm_dtype = pcm_dtype; c.mem = mem;
    c.sot_seq = sot_seq; c.text_tokens = text_tokens; c.n_text = n_text; c.n_frames = n_frames;
    c.n_sot = n_sot; c.max_text = max_text;
    return align_impl(ctx, c, B, no_timestamps, eot, medfilt_width, qk_scale, start_frame_out, token_prob_out);
} WM_API_CATCH

// wm_align on mel windows (the window description of wm_transcribe_mel) with one start sequence per row
extern "C" int wm_align_mel(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                            const int32_t *seek, const int32_t *n_frames, int B, const int32_t *sot_seqs, int n_sot,
                            int32_t no_timestamps, int32_t eot, const int32_t *text_tokens, const int32_t *n_text, int max_text,
                            int medfilt_width, float qk_scale, int32_t *start_frame_out, float *token_prob_out,
                            wm_mem mem) try {
    WM_MODEL(ctx);
    AlignCall c;
    c.dbg_matrix = std::exchange(m->pending.dbg.align_matrix, nullptr);   // the debug library's capture is for this call only
    WM_REQUIRE(m->finalized, WM_ERR_STATE, "model weights not finalised (wm_finalize)");
    WM_REQUIRE(mel && mel_base && mel_len && seek && n_frames, WM_ERR_INVALID, "null mel / window pointer");
    WM_REQUIRE(sot_seqs && n_text && start_frame_out && (max_text == 0 || text_tokens), WM_ERR_INVALID, "null pointer");
    WM_REQUIRE(B >= 1, WM_ERR_INVALID, "B < 1");
    c.mel = mel; c.mel_base = mel_base; c.mel_len = mel_len; c.seek = seek; c.mem = mem;
    c.sot_seq = sot_seqs; c.sot_stride = n_sot; c.text_tokens = text_tokens; c.n_text = n_text; c.n_frames = n_frames;
    c.n_sot = n_sot; c.max_text = max_text;
    return align_impl(ctx, c, B, no_timestamps, eot, medfilt_width, qk_scale, start_frame_out, token_prob_out);
} WM_API_CATCH

// ---------------------------------------------------------------- window sets
// wm_windows_encode runs the encoder and the cross-K/V projection of W windows once and keeps the result; the
// wm_*_windows calls are the mel calls with that result copied into the lane (wm_stage_cross_kv) instead of computed.
static int windows_cross_kv(wm_ctx *ctx, const wm_windows *set, const int32_t *rows, int B, std::vector<int32_t> &map) {
    WmAudioSrc a;
    a.windows = true; a.set = set; a.rows = rows;
    WM_TRY(wm_check_set_rows(ctx, a, B, "detect_language: "));
    WM_TRY(wm_model_reserve(ctx, B));
    std::vector<WmMelWin> win;
    return wm_stage_cross_kv(ctx, a, 0, B, WM_MEM_HOST, nullptr, win, map, nullptr);
}

extern "C" int wm_windows_encode(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                 const int32_t *seek, const int32_t *n_frames, int W, wm_mem mem, wm_windows **out) try {
    WM_REQUIRE(out != nullptr, WM_ERR_INVALID, "null out pointer");
    *out = nullptr;
    WM_MODEL(ctx);
    WM_REQUIRE(!ctx->dbg_hooks, WM_ERR_STATE, "window sets are not supported by the all-f32 precision path");
    WM_REQUIRE(m->finalized, WM_ERR_STATE, "model weights not finalised (wm_finalize)");
    WmAudioSrc a;
    a.mel = mel; a.mel_base = mel_base; a.mel_len = mel_len; a.seek = seek; a.n_frames = n_frames;
    WM_TRY(wm_check_src_pointers(a));
    WM_REQUIRE(W >= 1, WM_ERR_INVALID, "W < 1");
    for (int b = 0; b < W; ++b) WM_TRY(wm_check_window(a, b, "windows_encode: "));
    const wm_dims &D = m->dims;
    const long slab = (long)D.n_text_head * 1500 * 64;
    const int L2 = 2 * D.n_text_layer;
    struct Owner {   // nothing leaks on any way out
        wm_windows *w = nullptr;
        ~Owner() { if (w) wm_windows_free(w); }
    } own;
    WmEvents<3> ev;
    own.w = new wm_windows();
    wm_windows *w = own.w;
    w->device = ctx->device; w->dims = D; w->weights = m->tok_emb; w->W = W;
    w->n_frames.assign(n_frames, n_frames + W);
    w->bytes = (size_t)W * L2 * slab * sizeof(bf16_t);
    const hipError_t me = hipMalloc((void **)&w->store, w->bytes);
    if (me != hipSuccess) {
        (void)hipGetLastError();
        w->store = nullptr;
        wm_set_error("windows_encode: no device memory for %d windows (%zu bytes): %s", W, w->bytes, hipGetErrorString(me));
        return me == hipErrorOutOfMemory ? WM_ERR_NOMEM : WM_ERR_HIP;
    }
    WM_TRY(ev.create());
    ctx->stage_ms[0] = ctx->stage_ms[1] = ctx->stage_ms[2] = 0.f;
    std::vector<WmMelWin> win;
    std::vector<int32_t> map;
    WmStreamFence fence{ctx->stream};   // error paths: no copy from win may outlive it
    for (int b0 = 0; b0 < W; b0 += WM_DEC_MAXB) {
        const int Bg = std::min(WM_DEC_MAXB, W - b0);
        WM_TRY(wm_model_reserve(ctx, Bg));
        WM_HIP(hipEventRecord(ev[0], ctx->stream));
        WM_TRY(wm_stage_cross_kv(ctx, a, b0, Bg, mem, nullptr, win, map, ev[1]));
        WM_TRY(wm_xkv_rows(ctx, m->xkv, Bg, w->store, nullptr, b0, Bg, L2, slab, true));
        WM_HIP(hipEventRecord(ev[2], ctx->stream));
        WM_HIP(hipStreamSynchronize(ctx->stream));   // fences win; the next group overwrites m->xkv
        wm_add_stage_ms(ev.e, 2, false, ctx->stage_ms);
    }
    *out = w;
    own.w = nullptr;
    return WM_OK;
} WM_API_CATCH

extern "C" void wm_windows_free(wm_windows *w) {
    if (!w) return;
    if (w->store) {   // a reader may still be in flight on some lane's stream
        (void)hipSetDevice(w->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(w->store);
    }
    delete w;
}

extern "C" int wm_windows_count(const wm_windows *w) { return w ? w->W : -1; }

extern "C" size_t wm_windows_bytes(const wm_windows *w) { return w ? w->bytes : 0; }

// wm_align_mel over the windows of an encoded set: find_alignment's num_frames is the set's n_frames of the row
extern "C" int wm_align_windows(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B, const int32_t *sot_seqs, int n_sot,
                                int32_t no_timestamps, int32_t eot, const int32_t *text_tokens, const int32_t *n_text,
                                int max_text, int medfilt_width, float qk_scale, int32_t *start_frame_out,
                                float *token_prob_out) try {
    WM_MODEL(ctx);
    AlignCall c;
    c.dbg_matrix = std::exchange(m->pending.dbg.align_matrix, nullptr);   // the debug library's capture is for this call only
    WM_REQUIRE(m->finalized, WM_ERR_STATE, "model weights not finalised (wm_finalize)");
    WM_REQUIRE(sot_seqs && n_text && start_frame_out && (max_text == 0 || text_tokens), WM_ERR_INVALID, "null pointer");
    WM_REQUIRE(B >= 1, WM_ERR_INVALID, "B < 1");
    c.windows = true; c.set = w; c.rows = rows; c.mem = WM_MEM_HOST;
    WM_TRY(wm_check_set_rows(ctx, c, B, "align: "));
    std::vector<int32_t> nf(B);
    for (int b = 0; b < B; ++b) nf[b] = w->n_frames[rows ? rows[b] : b];
    c.sot_seq = sot_seqs; c.sot_stride = n_sot; c.text_tokens = text_tokens; c.n_text = n_text; c.n_frames = nf.data();
    c.n_sot = n_sot; c.max_text = max_text;
    return align_impl(ctx, c, B, no_timestamps, eot, medfilt_width, qk_scale, start_frame_out, token_prob_out);
} WM_API_CATCH

// Language identification from the windows of a set: wm_detect_language_probs with the features' cross-K/V copied from the
// set -- the same captured step, the same bits as wm_encode of the zero-padded window followed by that call
extern "C" int wm_windows_detect_language(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B, int32_t sot,
                                          int32_t lang_first, int32_t lang_last, int32_t *lang_idx, float *probs) try {
    WM_REQUIRE(w != nullptr, WM_ERR_INVALID, "null window set");
    return detect_language_impl(ctx, nullptr, B, sot, lang_first, lang_last, lang_idx, probs, WM_MEM_HOST, w, rows);
} WM_API_CATCH
