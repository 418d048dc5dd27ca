// transcribe.cpp -- the transcribe calls of the C ABI (include/whisper_mi355x.h): wm_transcribe_greedy, wm_transcribe,
// wm_transcribe_mel, wm_transcribe_mel_ragged, wm_transcribe_mel_best_of, wm_transcribe_windows, wm_transcribe_mel_beam,
// wm_transcribe_windows_beam, and the aligned entries wm_transcribe_mel_aligned / wm_transcribe_windows_aligned and their
// best-of and beam counterparts wm_transcribe_{mel,windows}_{best_of,beam}_aligned (the decode also captures the alignment
// heads' queries, a group ends with the alignment kernels and the DTW: lane_align; a group of candidates or beams aligns the
// ONE hypothesis of each window that its ranking chose).  Each entry point
// fills one request value (TxCall) and hands it to tx_transcribe: budgets, the entry's own checks, validation (tx_validate),
// the lane plan (tx_plan.h), the lanes (tx_lanes), the scheduler (tx_run: lane_start / lane_advance / lane_fetch /
// lane_finish), the ranking step of a best-of or beam call.  DESIGN.md section 4d.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "beam.h"
#include "call_src.h"
#include "model.h"
#include "tx_plan.h"


// One batch's decode is a chain of ~260 dependent launches per position and is bound by launch latency, not by
// HBM (NOTEBOOK.md section 4), so a call with more chunks than one decode group is spread over LANES: weight-sharing
// clones of the context (wm_clone), each with its own stream, activations, KV caches and decode graphs.  The
// single host thread drives the lanes as a small non-blocking scheduler: a lane takes the next decode group as soon as
// it has finished its previous one, positions are enqueued in BURSTS (one hipGraph of WM_BURST consecutive positions --
// the arg-max kernel advances the device-side position, so consecutive positions do not depend on the host), and with
// early stop on (eot >= 0 or per-chunk token budgets) a lane stays at most two bursts ahead of the GPU and stops
// enqueuing once the device reports that no sequence of its group is live any more.
namespace {
int lane_limit() {
    static const int n = [] {
        const char *e = getenv("WM_LANES");
        const int v = e ? atoi(e) : 3;
        return v < 1 ? 1 : (v > 8 ? 8 : v);
    }();
    return n;
}

int burst_len() {
    static const int n = [] {
        const char *e = getenv("WM_BURST");
        const int v = e ? atoi(e) : 8;
        return v < 1 ? 1 : (v > 32 ? 32 : v);
    }();
    return n;
}

// an aligned group's slice of WmModel::acap_ws, Cg windows of N rows: the capture buffer q [Cg * N][Tq][J][64]; per WINDOW the
// row and column statistics, the cost matrix x [Cg][n_ld][1500], the DTW trace and start frames; the ints n_text | n_frames |
// DTW rows | DTW frames [Cg] each, then the heads' layers | heads [J] each.  N > 1 (candidates, beams) adds the aligned
// hypotheses' gathered queries sel [Cg][Tq][J][64] and, behind the other ints, the gather's rows [Cg] | slot tables [Cg][Tq].
struct AcapWs {
    size_t q = 0, sel = 0, row = 0, col = 0, x = 0, tr = 0, start = 0, ints = 0, bytes = 0;
    int Tq = 0, J = 0, n_ld = 0, n_ints = 0;
};
AcapWs acap_layout(int Cg, int N, int Tq, int J, int n_ld) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    AcapWs w;
    w.Tq = Tq; w.J = J; w.n_ld = n_ld;
    w.sel = w.q + up((size_t)Cg * N * Tq * J * 64 * 4);
    w.row = w.sel + (N > 1 ? up((size_t)Cg * Tq * J * 64 * 4) : 0);
    w.col = w.row + up((size_t)Cg * J * Tq * 8);
    w.x = w.col + up((size_t)Cg * J * 1500 * 8);
    w.tr = w.x + up((size_t)Cg * n_ld * 1500 * 4);
    w.start = w.tr + up((size_t)Cg * wm_dtw_trace_words(n_ld) * 4);
    w.ints = w.start + up((size_t)Cg * n_ld * 4);
    w.n_ints = 4 * Cg + 2 * J + (N > 1 ? Cg + Cg * Tq : 0);
    w.bytes = w.ints + up((size_t)w.n_ints * 4);
    return w;
}

struct LaneJob {
    enum State { IDLE, DECODING, DRAINING, ALIGNING };
    wm_ctx *c = nullptr;
    int b0 = 0, Bg = 0;   // first row of the call (a candidate call: first WINDOW) and decoder rows of the group
    int Cg = 0;           // its encoder rows: Bg, or (candidates) Bg / n_cand windows -- row c * n_cand + s is candidate s of window c
    int P = 0;          // prompt positions of the group (a ragged call: the longest prompt among ITS rows)
    WmDecodeMode mode;  // of the group's decode (xattn_shared: decided burst by burst), filled by lane_prefill
    int gset = -1;      // its graph set in the lane's WmModel::graph_sets (lane_graph)
    State state = IDLE;
    int t = 0;          // decoder positions enqueued so far
    int bursts = 0;     // bursts enqueued so far
    bool stopped = false;   // the device reported zero live rows
    WmEvents<4> ev;                      // prefill begun, input staged, cross-K/V ready, everything enqueued
    WmEvents<WM_NLIVE_RING> burst_ev;    // (early stop) burst i has finished: its live count can be read
    TxGroupTables tab;             // its prompt table, offsets, budgets and sample ids (tx_plan.h)
    std::vector<int32_t> gen;      // its fetched token stream [max_new][Bg]
    WmXPar xpar = {};              // the group's extended-decode parameters (source of an async upload: lives here)
    WmRepPar rpar = {};            // its repetition rules (likewise)
    WmSampPar spar = {};           // its sampling rules (likewise)
    std::vector<WmXRow> samp;      // its rows' temperatures and seeds, padded (wm_set_sampling_rows; likewise)
    WmSbPar sbpar = {};            // its sequence-bias table's counts (likewise)
    WmAltPar apar = {};            // its alternatives request: n and the lane's buffers (likewise)
    WmGivenPar gpar = {};          // its given tokens: the group's table (likewise)
    WmGivenPanelPlan gplan;        // ... and their panel phase (wm_set_given_panel; WM_GP_SERVED: still to run, behind position P - 1)
    WmCstPar cpar = {};            // its constraint automaton's counts (likewise)
    std::vector<int32_t> cstart;   // ... and its rows' start states [Bg] (likewise)
    std::vector<float> lp, ns;     // its log-probs [max_new][Bg] and no-speech probabilities [Bg]
    std::vector<int32_t> atok, acnt;   // its fetched alternatives: ids [max_new][Bg][n], counts [max_new][Bg]
    std::vector<float> alp, aent;      // ... log-probs [max_new][Bg][n], entropy [max_new][Bg]
    std::vector<WmMelWin> win;     // its mel windows (wm_transcribe_mel)
    std::vector<int32_t> xrows;    // its rows of the window set (wm_transcribe_windows)
    // a beam group (wm_transcribe_mel_beam): its parameters and window budgets (sources of async uploads) and what a drain
    // fetches: the state in front of the finished records, the finished tokens / log-probs of its windows, the debug trace
    WmBeamPar bpar = {};
    std::vector<int32_t> bbud, bfin_tok;
    std::vector<char> bstate;
    std::vector<float> bfin_lp, btrace;
    std::vector<int32_t> banc, bfin_src;   // an aligned beam group: the ancestry record [max_new][Bg], [Cg][WM_MAX_BEAM_HYPS]
    // an aligned group: its workspace, the layers' alignment heads (kernel arguments of its steps), the host side of the ints
    // (source of async uploads), the windows that have a matrix, the aligned rows' lengths, the fetched start frames [Cg][n_ld],
    // the tail's two events
    AcapWs aw;
    std::vector<WmAlignLayer> alayers;
    std::vector<int32_t> aints, astart, alen;
    std::vector<char> aok;
    WmEvents<2> tail_ev;
    float stage_sum[3] = {0.f, 0.f, 0.f};
    WmStreamFence fence;   // last member, first to go: nothing in flight outlives the tables, the events or the fetched streams
};

// A transcribe call: its rows (PCM chunks, mel windows or the rows of a window set), their prompts, what decodes them
// (arg-max / sampling, best_of candidates, beams) and where the results go.
struct TxCall : WmCallKind {   // (tx_pending.h: the entry, greedy_entry, n_cand, beam, windows, hyp ...)
    WmAudioSrc src;
    TxPrompts prompts;
    int n_prompt = 0;   // the prompt length of a uniform call (a ragged call: TxCfg::n_prompt, found by validation)
    int max_cand = 0;
    float length_penalty = NAN;   // of the ranking step
    int B = 0, max_new = 0;
    int32_t eot = -1;
    const wm_decode_opts *opts = nullptr;
    int32_t *tokens_out = nullptr, *lens_out = nullptr;   // [B][S][max_new], [B][S]; S = n_cand, a beam call: max(n_cand, max_cand)
    float *logprobs_out = nullptr;    // like tokens_out, nullable
    float *no_speech_out = nullptr;   // [B], nullable
    int32_t *best_out = nullptr;      // [B], nullable: the ranking step's choice
    int32_t *n_hyp = nullptr;   // beam: [B]
    float *sums = nullptr;      // beam: [B][S]
    // wm_transcribe_mel_aligned / wm_transcribe_windows_aligned: word-timestamp alignment from the decode's own queries
    bool aligned = false;
    int medfilt = 0;
    float qk_scale = 1.f;
    int32_t *start_out = nullptr;   // [B][max_new + 1]
    WmDebugShots dbg;   // debug library: the one-shots the call took, a beam call's trace and an aligned call's captures alone
    // hypotheses per window of the outputs: tokens_out [B][S][max_new]
    int out_stride() const { return beam ? std::max(n_cand, max_cand) : n_cand; }
    wm_mem mem = WM_MEM_HOST;
};

struct StopCfg {
    bool on = false;
    int32_t eot = -1;
    const int32_t *budgets = nullptr;  // [B] of the call, already clamped to max_new (null: none)
};

// wm_transcribe's extended decode: off for wm_transcribe_greedy and for a wm_transcribe call that wants neither outputs nor
// sampling (then it IS the greedy decode: same graphs, same kernels)
struct XCfg {
    bool on = false;
    WmXPar par = {};               // chunk0 / n_prompt filled per group
    float *logprobs = nullptr;     // [B][max_new] host, nullable
    float *no_speech = nullptr;    // [B] host, nullable
};

// what validation makes of a call
struct TxCfg {
    int n_prompt = 0;   // the call's longest prompt
    StopCfg stop;
    XCfg xc;
    bool use_graph = false;
    // an aligned call: prompt positions from <|startoftranscript|> to the prompt's end (the same for every row), the
    // alignment heads (ascending), the capture budget's bound on a group's rows (0: none)
    int sot_tail = 0;
    std::vector<int32_t> hl, hh;
    int max_group_rows = 0;
    // What the call took (tx_take), checked: the row maps are [B] of the call where what they map is in force -- bias_rows with
    // row tables; cst_rows with a constraint (empty: every row starts in 0); alt_on: the call's alternatives request.
    const WmPending *pending = &wm_nothing_pending();
    bool samp_rows = false;   // the sampling row map has a sampling row (else opts->temperature and opts->seed hold for every row)
};

// the tokens row `b` of the call may generate
int stop_budget(const StopCfg &stop, int b, int max_new) { return stop.budgets && stop.budgets[b] < max_new ? stop.budgets[b] : max_new; }

// front end -> encoder -> cross K/V -> prompt upload -> first embedding, all enqueued on the lane's stream
int lane_prefill(LaneJob &j, const TxCall &call, const TxCfg &cfg) {
    wm_ctx *c = j.c;
    WmModel *m = c->model;
    const StopCfg &stop = cfg.stop;
    const XCfg &xc = cfg.xc;
    const int Bg = j.Bg, Cg = j.Cg, N = call.n_cand;   // decoder rows, encoder rows (windows), candidates per window
    m->last_prefill[0] = m->last_prefill[1] = m->last_prefill[2] = 0;   // (set again by this group's prompt panels, if it runs any)
    for (int &v : m->last_given_panel) v = 0;                             // (... by its given panels)
    j.gplan = WmGivenPanelPlan();
    // the mode of this group's decode: the lane's own context settings and the call's options, in this one place
    j.mode = WmDecodeMode();
    j.mode.mask = m->mask_on; j.mode.ts = m->ts_on; j.mode.x = xc.on; j.mode.off = call.prompts.len != nullptr;
    j.mode.stop = stop.on; j.mode.budget = stop.on && stop.budgets != nullptr; j.mode.stop_eot = stop.on ? stop.eot : -1;
    j.mode.n_cand = N;
    j.mode.beam = call.beam ? N : 0;
    j.mode.sbt = m->sbt_on;
    j.mode.sb = m->sb_on || m->sbt_on;
    j.mode.cst = m->cst_on;
    // (tx_validate turns the extended decode on with them; the bias and the constraint use the rules' bitmaps)
    j.mode.rep = m->rep_on || j.mode.sb || j.mode.cst;
    j.mode.trunc = m->samp_on() && xc.on && xc.par.sample != 0;   // temperature 0 ignores the sampling rules: today's launches
    const WmPending &pend = *cfg.pending;
    j.mode.srows = xc.on && cfg.samp_rows;   // (a row map: the launch is in the plan when any row of the CALL samples)
    j.mode.alt = pend.alt_on;   // (tx_validate turned the extended decode on with it)
    // given tokens: the group's rows of the call's table, by the hypothesis-row map; a group without a given row is an ordinary one
    int given_L = 0;
    if (!pend.given_lens.empty())
        given_L = wm_group_given(pend.given_lens.data(), pend.given_tok.data(), pend.given_stride, j.b0, Cg, N, &j.tab.glen, &j.tab.gtok);
    j.mode.given = given_L > 0;
    // the group's tables (pure: tx_plan.h), uploaded below: prompt tokens [P][Bg], a ragged call's offsets, budgets, sample ids
    j.P = wm_group_tables(call.prompts, cfg.n_prompt, j.mode.budget ? stop.budgets : nullptr, j.b0, Cg, N, WM_XIDS_CAND, xc.on, &j.tab);
    if (call.aligned) {   // the capture buffer and the alignment workspace, reserved before anything is enqueued
        const int J = (int)cfg.hl.size();
        j.aw = acap_layout(Cg, N, cfg.sot_tail + call.max_new - 1, J, call.max_new + 1);
        WM_TRY(m->acap_ws.reserve(c->stream, j.aw.bytes));
        j.alayers.assign(m->dims.n_text_layer, WmAlignLayer());
        j.aints.assign((size_t)j.aw.n_ints, 0);
        for (int k = 0; k < J; ++k) {
            WmAlignLayer &Ly = j.alayers[cfg.hl[k]];
            if (Ly.n == 0) Ly.slot0 = k;
            Ly.head[Ly.n++] = cfg.hh[k];
            j.aints[4 * Cg + k] = cfg.hl[k];
            j.aints[4 * Cg + J + k] = cfg.hh[k];
        }
        j.mode.acap = true; j.mode.acap_base = j.P - cfg.sot_tail; j.mode.acap_Tq = j.aw.Tq; j.mode.acap_J = J;
        j.mode.acap_q = (float *)((char *)m->acap_ws.p + j.aw.q);
        if (call.dbg.align_matrix) WM_HIP(hipMemsetAsync((char *)m->acap_ws.p + j.aw.x, 0, (size_t)Cg * j.aw.n_ld * 1500 * 4, c->stream));
    }
    const void *d_pcm;
    WM_TRY(wm_stage_pcm(c, call.src, j.b0, Cg, call.mem, &d_pcm));
    // decode state first (prompt tokens, position 0): a pageable H2D copy may wait for the stream to drain, so it is issued
    // while the lane is still idle
    WM_TRY(wm_model_decode_begin(c, Bg));
    if (call.prompts.len) WM_HIP(hipMemcpyAsync(m->doff, j.tab.off.data(), (size_t)Bg * 4, hipMemcpyHostToDevice, c->stream));
    WM_HIP(hipMemcpyAsync(m->dseq, j.tab.pr.data(), j.tab.pr.size() * 4, hipMemcpyHostToDevice, c->stream));
    WM_TRY(wm_model_set_pos(c, 0));
    // early-stop state of this group: done flags, live list, per-row budgets (kernel arguments of the decode graphs)
    if (stop.on) {
        if (j.mode.budget) WM_HIP(hipMemcpyAsync(m->dbudget, j.tab.bud.data(), (size_t)Bg * 4, hipMemcpyHostToDevice, c->stream));
        WM_TRY(wm_stop_init(c, wm_model_stop_dev(m, j.mode), Bg));
    }
    // extended decode: seed, 1/T, the sot position and the group's first call index live in device memory, so the
    // captured graphs replay for any of them
    if (xc.on) {
        j.xpar = xc.par;
        j.xpar.chunk0 = j.b0;
        j.xpar.n_prompt = j.P;
        if (call.prompts.len && xc.no_speech) j.xpar.sot_pos = j.P - call.prompts.sot_tail;   // the same distance from every row's end
        j.xpar.ids_on = (call.prompts.sample_ids || N > 1) ? 1 : 0;
        j.xpar.n_cand = N;
        if (!j.tab.ids.empty()) WM_HIP(hipMemcpyAsync(m->dx_ids, j.tab.ids.data(), j.tab.ids.size() * 4, hipMemcpyHostToDevice, c->stream));
        if (j.mode.srows) {   // the rows' own 1 / T and keys, padded with arg-max rows like the ids (the epilogue's 16-row blocks)
            j.samp.assign(WM_XIDS_CAND, WmXRow{0.f, 0u, 0u, 0u});
            for (int r = 0; r < Bg; ++r) {
                const float T = pend.samp_T[j.b0 + r / N];
                const uint64_t seed = pend.samp_seed[j.b0 + r / N];
                if (T > 0.f) j.samp[r] = WmXRow{(float)(1.0 / (double)T), (unsigned)seed, (unsigned)(seed >> 32), 0u};
            }
            WM_HIP(hipMemcpyAsync((void *)wm_x_rows(m->dx_ids), j.samp.data(), j.samp.size() * sizeof(WmXRow), hipMemcpyHostToDevice, c->stream));
        }
        WM_HIP(hipMemcpyAsync(m->dx_par, &j.xpar, sizeof(WmXPar), hipMemcpyHostToDevice, c->stream));
    }

    // repetition rules: penalty, its reciprocal, n and eot live in device memory too (the graph key holds `rep` alone)
    if (j.mode.rep) {
        WM_REQUIRE(xc.on, WM_ERR_STATE, "the repetition rules need the extended decode");
        j.rpar.p = m->rep_p; j.rpar.inv_p = (float)(1.0 / (double)m->rep_p); j.rpar.n = m->rep_n; j.rpar.eot = m->rep_eot;
        if (!m->rep_on) { j.rpar.p = 1.f; j.rpar.inv_p = 1.f; j.rpar.n = 0; j.rpar.eot = 0; }   // the bias or the constraint alone: empty rules
        WM_HIP(hipMemcpyAsync(m->drep_par, &j.rpar, sizeof(WmRepPar), hipMemcpyHostToDevice, c->stream));
    }
    // sampling rules: top_k, top_p and min_p live in device memory as well (the graph key holds `trunc` alone)
    if (j.mode.trunc) {
        j.spar.top_k = m->samp_k; j.spar.top_p = m->samp_p; j.spar.min_p = m->samp_minp;
        WM_HIP(hipMemcpyAsync(m->dsamp_par, &j.spar, sizeof(WmSampPar), hipMemcpyHostToDevice, c->stream));
    }
    // alternatives: n and the lane's buffers live in device memory too (the graph key holds `alt` alone); the buffers are
    // reserved for this group and pad-filled here, so positions no workgroup writes (finished rows) read as pads
    if (j.mode.alt) {
        WM_REQUIRE(xc.on, WM_ERR_STATE, "alternatives need the extended decode");
        WM_TRY(wm_model_alt_begin(c, Bg, call.max_new, pend.alt.n, &j.apar));
    }
    // given tokens: the group's table lives in device memory as well (the graph key holds `given` alone)
    if (j.mode.given) {
        WM_REQUIRE(xc.on, WM_ERR_STATE, "given tokens need the extended decode");
        WM_TRY(wm_model_given_begin(c, Bg, given_L, j.tab.glen.data(), j.tab.gtok.data(), &j.gpar));
    }
    // sequence bias: the table was uploaded when it was set; its counts go with the group, so a captured graph replays for any table
    if (j.mode.sbt) {   // row tables: the pool was uploaded when it was set; the rows' group ranges go with the group likewise
        WM_REQUIRE(!pend.bias_rows.empty(), WM_ERR_STATE, "sequence-bias tables are in force and the call has no row map (wm_set_bias_rows)");
        wm_group_bias_rows(pend.bias_rows.data(), m->sbt_tab_grp.data(), (int)m->sbt_tab_grp.size() - 1, j.b0, Cg, N, &j.tab.sbr);
        WM_HIP(hipMemcpyAsync(m->dsb_rng, j.tab.sbr.data(), j.tab.sbr.size() * 4, hipMemcpyHostToDevice, c->stream));
    } else if (j.mode.sb) {
        j.sbpar.n_groups = m->sb_groups; j.sbpar.n_entries = m->sb_entries;
        WM_HIP(hipMemcpyAsync((void *)m->dsb.par, &j.sbpar, sizeof(WmSbPar), hipMemcpyHostToDevice, c->stream));
    }
    // constraint: the automaton was uploaded when it was set; its counts and the rows' start states go with the group, so a captured
    // graph replays for any automaton.  Row c * N + s (a candidate, a beam) takes the start of its window.
    if (j.mode.cst) {
        j.cpar.n_states = m->cst_states; j.cpar.n_edges = m->cst_edges; j.cpar.eot = m->cst_eot;
        j.cstart.resize(Bg);
        for (int r = 0; r < Bg; ++r) j.cstart[r] = pend.cst_rows.empty() ? 0 : pend.cst_rows[j.b0 + r / N];
        WM_HIP(hipMemcpyAsync((void *)m->dcst.par, &j.cpar, sizeof(WmCstPar), hipMemcpyHostToDevice, c->stream));
        WM_HIP(hipMemcpyAsync((void *)m->dcst.start, j.cstart.data(), (size_t)Bg * 4, hipMemcpyHostToDevice, c->stream));
    }
    WM_TRY(wm_model_reserve(c, Cg));
    if (N > 1) WM_TRY(wm_model_reserve_rows(c, Bg));
    if (call.beam) {   // beam state: nothing finished, every sum 0; a window's budget is its own max_new
        j.bbud.resize(Cg);
        for (int w = 0; w < Cg; ++w) j.bbud[w] = stop_budget(stop, j.b0 + w, j.bpar.max_new);
        m->beam_trace_on = call.dbg.beam_trace != nullptr;
        if (call.dbg.beam_trace) {
            const size_t bytes = (size_t)j.bpar.max_new * Bg * WM_BEAM_TRACE * 4;
            WM_TRY(m->beam_trace.reserve(c->stream, bytes));
            WM_HIP(hipMemsetAsync(m->beam_trace.p, 0, bytes, c->stream));
        }
        WM_TRY(wm_model_beam_begin(c, j.mode, Bg, Cg, &j.bpar, j.bbud.data()));
    }
    WM_HIP(hipEventRecord(j.ev[0], c->stream));
    // 1. log-mel front end, or the caller's mel windows;  2. encoder + cross-attention K/V  (a window set: 1. the gather)
    WM_TRY(wm_stage_cross_kv(c, call.src, j.b0, Cg, call.mem, d_pcm, j.win, j.xrows, j.ev[1]));

    WM_HIP(hipEventRecord(j.ev[2], c->stream));
    // 3. embedding of the first prompt token (+ the initial timestamp-rule state)
    WM_TRY(wm_model_embed_first(c, Bg, j.mode));
    if (j.mode.ts) WM_TRY(wm_ts_init(c, wm_model_ts_dev(m), Bg));
    return WM_OK;
}

// Prompt panels (wm_set_prompt_panel), enqueued behind the group's prefill and before anyone's first
// burst: the prompt positions whose logits the call does not read -- everything in front of <|startoftranscript|> when
// no_speech_prob is computed, in front of the prompt's last position otherwise, and never an aligned group's captured
// positions -- run as cache-only panel steps, and the group's ordinary steps begin at that position.  Plain groups only: a
// candidate or beam group, a speculative call and the all-f32 precision path step through their prompts as they always did.
int lane_prompt_panels(LaneJob &j, const TxCall &call, const wm_ctx *caller) {
    WmModel *m = j.c->model;
    if (m->prompt_panel <= 1 || call.n_cand != 1 || call.beam || caller->dbg_hooks) return WM_OK;
    WmPromptPanelPlan pl;
    wm_prompt_panel_plan(j.Bg, m->prompt_panel, j.P, j.mode.x ? j.xpar.sot_pos : -1, j.mode.acap ? j.mode.acap_base : -1,
                         g_wm_tuning.teacher_panel_cut, &pl);
    if (pl.w < 1) return WM_OK;
    WM_TRY(wm_model_prompt_prefill(j.c, j.Bg, pl.P0, j.mode));
    j.t = pl.P0;
    return WM_OK;
}

// Given panels (wm_set_given_panel): whether this group runs a phase, decided behind its prefill from the
// group's mode, its rows' given lengths and budgets (tx_plan.h wm_given_panel_plan: pure).  The setting never makes a call fail:
// a group the rule does not serve steps one position at a time.
void lane_given_plan(LaneJob &j, const TxCall &call, const wm_ctx *caller) {
    const WmModel *m = j.c->model;
    const WmDecodeMode &md = j.mode;
    unsigned bits = 0;
    if (md.given) bits |= WM_GPB_GIVEN;
    if (call.n_cand != 1 || call.beam) bits |= WM_GPB_CAND;
    if (md.off) bits |= WM_GPB_OFF;
    if (md.x) bits |= WM_GPB_X;
    if (md.srows) bits |= WM_GPB_SROWS;
    if (md.trunc) bits |= WM_GPB_TRUNC;
    if (md.x && j.xpar.sample) bits |= WM_GPB_SAMPLE;
    if (md.alt) bits |= WM_GPB_ALT;
    if (md.sbt) bits |= WM_GPB_SBT;
    if (md.sb) bits |= WM_GPB_SB;
    if (md.cst) bits |= WM_GPB_CST;
    if (md.rep) bits |= WM_GPB_REP;
    if (md.acap) bits |= WM_GPB_ACAP;
    if (call.f32_path || caller->dbg_hooks) bits |= WM_GPB_F32;
    wm_given_panel_plan(j.Bg, m->given_panel, md.given ? j.tab.glen.data() : nullptr, md.budget ? j.tab.bud.data() : nullptr, call.max_new,
                        j.P, m->dims.n_text_ctx, bits, &j.gplan);
}

// ... and the phase itself, enqueued eagerly behind the ordinary step at position P - 1 (which took generated index 0): generated
// indices [1, Lp) in rounds; the group's ordinary steps or captured graphs continue from position P + Lp - 1.
int lane_given_panels(LaneJob &j, int max_new, const WmDecodeMode &mode) {
    const WmGivenPanelPlan pl = j.gplan;
    j.gplan = WmGivenPanelPlan();   // (runs once)
    WM_TRY(wm_model_given_panel_phase(j.c, j.Bg, pl.w, pl.Lp, j.P, max_new, mode));
    j.t = j.P + pl.Lp - 1;
    return WM_OK;
}

// One decoder position = 8 launches per layer + logits + arg-max/embed (which writes the next token, embeds the
// next position and advances *dpos).  Nothing in it depends on host state, so it is captured ONCE into a
// hipGraph per lane and replayed for every position -- and `burst` consecutive positions are captured as one more graph.
// gen (a beam group's generating positions): the step also stores the f32 logits and the beam kernels close it.
int lane_position(LaneJob &j, const WmDecodeMode &mode, int n_prompt, bool gen) {
    WmAlignCap cap = {j.alayers.data(), mode.acap_q, mode.acap_Tq, mode.acap_J, mode.acap_base};   // an aligned group: every step captures
    WM_TRY(wm_model_decode_step(j.c, j.Bg, gen || mode.trunc || mode.alt || mode.given, 0, j.c->model->dims.n_vocab - 1, mode.acap ? &cap : nullptr, mode, n_prompt));
    if (gen) return wm_model_beam_close(j.c, j.Bg, n_prompt, mode);
    // alternatives: the row's list and entropy from the stored row and the partials as the logits launch left them -- in front of
    // the truncation, which rewrites the per-tile keys.  At a prompt position its workgroups return at once, as the truncation's.
    if (mode.alt) WM_TRY(wm_model_alternatives(j.c, j.Bg, n_prompt, mode));
    // sampling rules: the kept set and its draw, in line between the logits launch (which stored the f32 row) and the close.
    // The graph of a position is one for prompt and generated positions alike (the position lives on the device), so at a
    // prompt position of such a group the row store is wasted and the truncation workgroups return at once (gi < 0): one
    // launch of the floor's cost per prompt position, paid so that no second graph shape exists.
    if (mode.trunc) WM_TRY(wm_model_sample_truncate(j.c, j.Bg, n_prompt, mode));
    // given tokens: last in front of the close, so the alternatives list what the model preferred and a given row overrides a draw.
    // At a prompt position, and for the group's free rows, its workgroups return at once.
    if (mode.given) WM_TRY(wm_model_given_tokens(j.c, j.Bg, n_prompt, mode));
    return wm_model_close_step(j.c, j.Bg, n_prompt, true, nullptr, 0, mode);
}

int capture_positions(LaneJob &j, const WmDecodeMode &mode, int n_prompt, int n_pos, bool gen, WmGraph *out) {
    char what[48];
    snprintf(what, sizeof(what), "the %d-position decode graph", n_pos);
    return wm_capture_graph(j.c->stream, out, what, [&]() -> int {
        for (int i = 0; i < n_pos; ++i) WM_TRY(lane_position(j, mode, n_prompt, gen));
        return WM_OK;
    });
}

// Select (creating it if needed) the graph set of the group's decode shape and mode.  The graphs themselves are captured
// on first use, per sharing mode, by lane_burst.
int lane_graph(LaneJob &j, int n_prompt) {
    WmModel *m = j.c->model;
    int cur = -1;
    for (size_t i = 0; i < m->graph_sets.size(); ++i) {
        const WmModel::GraphSet &g = m->graph_sets[i];
        if (g.B == j.Bg && g.n_prompt == n_prompt && g.cap_b == m->cap_b && g.mode == j.mode) cur = (int)i;
    }
    if (cur < 0) {
        if ((int)m->graph_sets.size() >= WmModel::kMaxGraphSets) {   // evict the least recently used shape
            size_t old = 0;
            for (size_t i = 1; i < m->graph_sets.size(); ++i)
                if (m->graph_sets[i].stamp < m->graph_sets[old].stamp) old = i;
            m->graph_sets[old].destroy();
            m->graph_sets.erase(m->graph_sets.begin() + (long)old);
        }
        WmModel::GraphSet g;
        g.B = j.Bg; g.n_prompt = n_prompt; g.cap_b = m->cap_b; g.mode = j.mode;
        m->graph_sets.push_back(g);
        cur = (int)m->graph_sets.size() - 1;
    }
    j.gset = cur;
    m->graph_sets[cur].stamp = ++m->graph_clock;
    return WM_OK;
}

// a beam group has enqueued everything: fetch its beam state behind the token streams
int beam_fetch(LaneJob &j, int max_new, bool trace) {
    WmModel *m = j.c->model;
    WmBeamDev bm;
    WM_TRY(wm_model_beam_dev(j.c, j.mode, &bm));
    j.lp.resize((size_t)max_new * j.Bg);   // the live beams' log-probs [gi][row], whether or not the caller wants them
    WM_HIP(hipMemcpyAsync(j.lp.data(), m->dx_logprob, j.lp.size() * 4, hipMemcpyDeviceToHost, j.c->stream));
    j.bstate.resize(wm_model_beam_state_bytes(m));
    WM_HIP(hipMemcpyAsync(j.bstate.data(), m->beam_ws.p, j.bstate.size(), hipMemcpyDeviceToHost, j.c->stream));
    const size_t nf = (size_t)j.Cg * WM_MAX_BEAM_HYPS * bm.n_ctx;
    j.bfin_tok.resize(nf);
    j.bfin_lp.resize(nf);
    WM_HIP(hipMemcpyAsync(j.bfin_tok.data(), bm.fin_tok, nf * 4, hipMemcpyDeviceToHost, j.c->stream));
    WM_HIP(hipMemcpyAsync(j.bfin_lp.data(), bm.fin_lp, nf * 4, hipMemcpyDeviceToHost, j.c->stream));
    if (trace) {
        j.btrace.resize((size_t)max_new * j.Bg * WM_BEAM_TRACE);
        WM_HIP(hipMemcpyAsync(j.btrace.data(), m->beam_trace.p, j.btrace.size() * 4, hipMemcpyDeviceToHost, j.c->stream));
    }
    if (bm.anc) {   // an aligned group: the ancestry record lane_align walks
        j.banc.resize((size_t)max_new * j.Bg);
        j.bfin_src.resize((size_t)j.Cg * WM_MAX_BEAM_HYPS);
        WM_HIP(hipMemcpyAsync(j.banc.data(), bm.anc, j.banc.size() * 4, hipMemcpyDeviceToHost, j.c->stream));
        WM_HIP(hipMemcpyAsync(j.bfin_src.data(), bm.fin_src, j.bfin_src.size() * 4, hipMemcpyDeviceToHost, j.c->stream));
    }
    return WM_OK;
}

// ... and, once it has arrived, write the windows' hypotheses: the finished ones in the order they finished, then (fewer
// than N finished) the live beams by descending sum until there are N.  Output stride S = max(N, max_cand) per window.
void beam_drain(const LaneJob &j, const TxCall &call) {
    const int N = call.n_cand, S = std::max(N, call.max_cand), n_ctx = j.c->model->dims.n_text_ctx, max_new = call.max_new;
    const int32_t eot = call.eot;
    int32_t *tokens_out = call.tokens_out, *lens_out = call.lens_out;
    float *logprobs_out = call.logprobs_out, *no_speech_out = call.no_speech_out;
    // the device pointers of the state, as offsets into the fetched copy
    WmBeamDev bm;
    (void)wm_model_beam_dev(j.c, j.mode, &bm);
    const char *dev0 = (const char *)j.c->model->beam_ws.p;
    auto host = [&](const void *dev) { return j.bstate.data() + ((const char *)dev - dev0); };
    const float *sum = (const float *)host(bm.sum), *fin_sum = (const float *)host(bm.fin_sum);
    const int *fin_n = (const int *)host(bm.fin_n), *fin_len = (const int *)host(bm.fin_len), *wsteps = (const int *)host(bm.wsteps);
    for (int w = 0; w < j.Cg; ++w) {
        const int W = j.b0 + w;   // window of the call
        int n_hyp = 0;
        auto put = [&](const int32_t *tok, size_t tok_stride, const float *lp, size_t lp_stride, int len, float s) {
            const size_t o = (size_t)W * S + n_hyp++;
            for (int i = 0; i < max_new; ++i) {
                tokens_out[o * max_new + i] = i < len ? tok[(size_t)i * tok_stride] : eot;
                if (logprobs_out) logprobs_out[o * max_new + i] = i < len ? lp[(size_t)i * lp_stride] : 0.f;
            }
            lens_out[o] = len;
            call.sums[o] = s;
        };
        for (int f = 0; f < fin_n[w]; ++f) {
            const size_t base = ((size_t)w * WM_MAX_BEAM_HYPS + f) * n_ctx;
            put(j.bfin_tok.data() + base, 1, j.bfin_lp.data() + base, 1, fin_len[w * WM_MAX_BEAM_HYPS + f], fin_sum[w * WM_MAX_BEAM_HYPS + f]);
        }
        if (n_hyp < N) {
            int order[WM_MAX_BEAM];
            const int n_live = wm_beam_fill_order(N, sum + (size_t)w * N, order);
            for (int k = 0; k < n_live && n_hyp < N; ++k) {
                const int b = w * N + order[k];
                put(j.gen.data() + b, j.Bg, j.lp.data() + b, j.Bg, wsteps[w], sum[b]);
            }
        }
        call.n_hyp[W] = n_hyp;
        for (int h = n_hyp; h < S; ++h) {   // unused slots
            const size_t o = (size_t)W * S + h;
            for (int i = 0; i < max_new; ++i) {
                tokens_out[o * max_new + i] = eot;
                if (logprobs_out) logprobs_out[o * max_new + i] = 0.f;
            }
            lens_out[o] = 0;
            call.sums[o] = -INFINITY;
        }
        if (no_speech_out) no_speech_out[W] = j.ns[(size_t)w * N];   // beam 0's
        if (call.dbg.beam_trace)     // [gi][row of the group] -> [window of the call][gi][beam]
            for (int gi = 0; gi < max_new; ++gi)
                memcpy(call.dbg.beam_trace + (((size_t)W * max_new + gi) * N) * WM_BEAM_TRACE,
                       j.btrace.data() + ((size_t)gi * j.Bg + (size_t)w * N) * WM_BEAM_TRACE, (size_t)N * WM_BEAM_TRACE * 4);
    }
}

// enqueue the next burst of positions of a lane (<= burst_len(), up to the end of the sequence).  `shared`: other decode
// groups are in flight on the device right now -- this burst's cross-attention launches are the short-lived shape.
int lane_burst(LaneJob &j, int n_prompt, int n_steps, bool use_graph, bool shared) {
    wm_ctx *c = j.c;
    WmModel *m = c->model;
    const int K = burst_len();
    // a beam group: positions 0 .. n_prompt - 2 step through the prompt (the arg-max close), the others generate (the beam
    // close); a burst stays on one side
    const bool gen = j.mode.beam && j.t >= n_prompt - 1;
    const int sh = shared ? 1 : 0;
    WmDecodeMode mode = j.mode;   // what every step of this burst, launched or captured, is handed
    mode.xattn_shared = shared;
    // a group with a given-panel phase to run (never a beam group): a burst ends with the step at position n_prompt - 1, and the
    // phase is the next burst
    const bool phase = j.gplan.reason == WM_GP_SERVED;
    if (phase && j.t == n_prompt) {
        WM_TRY(lane_given_panels(j, n_steps - n_prompt + 1, mode));
    } else {
        const int left = (j.mode.beam && !gen ? n_prompt - 1 : (phase ? n_prompt : n_steps)) - j.t;
        const int k = left < K ? left : K;
        WmModel::GraphSet *g = use_graph ? &m->graph_sets[j.gset] : nullptr;
        WmGraph *g1 = g ? (gen ? g->b1 : g->g1) : nullptr, *gk = g ? (gen ? g->bk : g->gk) : nullptr;
        int *burst = g ? (gen ? g->bburst : g->burst) : nullptr;
        if (use_graph && k == K && K > 1) {
            if (!gk[sh].e || burst[sh] != K) {
                WM_TRY(capture_positions(j, mode, n_prompt, K, gen, &gk[sh]));
                burst[sh] = K;
            }
            WM_HIP(hipGraphLaunch(gk[sh].e, c->stream));
        } else {
            if (use_graph && !g1[sh].e) WM_TRY(capture_positions(j, mode, n_prompt, 1, gen, &g1[sh]));
            for (int i = 0; i < k; ++i) {
                if (use_graph) {
                    WM_HIP(hipGraphLaunch(g1[sh].e, c->stream));
                } else {
                    WM_TRY(lane_position(j, mode, n_prompt, gen));
                }
            }
        }
        j.t += k;
    }
    if (j.mode.stop) {  // the live-row count after this burst, where the host can read it without touching the stream
        const int slot = j.bursts % WM_NLIVE_RING;
        WM_HIP(hipMemcpyAsync(m->h_nlive + slot, m->dnlive, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        WM_HIP(hipEventRecord(j.burst_ev[slot], c->stream));
    }
    ++j.bursts;
    return WM_OK;
}
// ---------------------------------------------------------------- the entries' own checks, validation ----
// The checks of an entry point's own arguments.  They run before the context is looked at: which error wins when several
// apply is part of the ABI (tests/test_transcribe_errors_gpu.py).
int entry_checks(const TxCall &call) {
    const TxPrompts &p = call.prompts;
    switch (call.entry) {
    case TxCall::PLAIN:
        break;
    case TxCall::MEL:
    case TxCall::RAGGED:
        WM_REQUIRE(call.src.mel && call.src.mel_base && call.src.mel_len && call.src.seek && call.src.n_frames, WM_ERR_INVALID,
                   "null mel / window pointer");
        if (call.entry == TxCall::MEL) break;
        WM_REQUIRE(p.len, WM_ERR_INVALID, "null prompt_len");
        WM_REQUIRE(p.stride >= 1, WM_ERR_INVALID, "prompt_stride %d < 1", p.stride);
        break;
    case TxCall::BEST_OF:
    case TxCall::BEAM:
        WM_TRY(wm_check_src_pointers(call.src));
        if (call.beam) WM_REQUIRE(call.n_hyp && call.sums, WM_ERR_INVALID, "null n_hyp_out / sum_logprobs_out");
        WM_REQUIRE(p.stride >= 1, WM_ERR_INVALID, "prompt_stride %d < 1", p.stride);
        if (call.beam) {
            WM_REQUIRE(call.n_cand >= 1 && call.n_cand <= WM_MAX_BEAM, WM_ERR_INVALID, "beam_size %d outside [1, %d]", call.n_cand,
                       WM_MAX_BEAM);
            WM_REQUIRE(call.max_cand >= 1 && call.max_cand <= WM_MAX_BEAM_HYPS, WM_ERR_INVALID, "max_candidates %d outside [1, %d]",
                       call.max_cand, WM_MAX_BEAM_HYPS);
        } else {
            WM_REQUIRE(call.n_cand >= 1 && call.n_cand <= WM_MAX_BEST_OF, WM_ERR_INVALID, "best_of %d outside [1, %d]", call.n_cand,
                       WM_MAX_BEST_OF);
        }
        WM_REQUIRE(std::isnan(call.length_penalty) || (call.length_penalty >= 0.f && call.length_penalty <= 1.f), WM_ERR_INVALID,
                   "length_penalty must be NaN (none) or in [0, 1]");
        WM_REQUIRE(call.B >= 1 && call.max_new >= 1, WM_ERR_INVALID, "B < 1 or max_new < 1");
        break;
    }
    return WM_OK;
}

// What a call takes with it when it begins, in front of every check (tx_pending.h); it learns here whether it runs on the all-f32 path.
WmPending tx_take(wm_ctx *ctx, TxCall &call) {
    call.f32_path = ctx && ctx->dbg_hooks;
    return ctx && ctx->model ? ctx->model->pending.take() : WmPending();
}
int tx_served(unsigned bits, const TxCall &call) {   // does the call serve the pending items `bits` names?
    const char *no = wm_pending_refusal(bits, call);
    WM_REQUIRE(!no, WM_ERR_STATE, "%s", no);
    return WM_OK;
}

// The checks every transcribe call goes through, and what they make of it: the call's longest prompt, the early stop, the
// extended decode.  pending: what the call took (tx_take) -- its budgets are clamped to max_new here, and cfg points into it.
// opts == null with both extra outputs null is the greedy decode exactly.
int tx_validate(wm_ctx *ctx, const TxCall &call, WmPending &pending, TxCfg *cfg) {
    WmModel *m = ctx->model;
    cfg->pending = &pending;
    std::vector<int32_t> &budgets = pending.budgets;
    const wm_alternatives_out *alt = pending.alt_on ? &pending.alt : nullptr;
    const WmAudioSrc &src = call.src;
    const TxPrompts &p = call.prompts;
    const int B = call.B, max_new = call.max_new;
    WM_REQUIRE(m->finalized, WM_ERR_STATE, "model weights not finalised (wm_finalize)");
    WM_REQUIRE((src.pcm || src.mel || src.windows) && p.prompt && call.tokens_out && call.lens_out, WM_ERR_INVALID, "null pointer");
    WM_REQUIRE(src.mel || src.windows || src.pcm_dtype == WM_I16 || src.pcm_dtype == WM_F32 || src.pcm_dtype == WM_F64,
               WM_ERR_INVALID, "bad pcm dtype");
    WM_REQUIRE(B >= 1, WM_ERR_INVALID, "B < 1");
    if (src.mel)
        for (int b = 0; b < B; ++b) WM_TRY(wm_check_window(src, b, ""));
    if (src.windows) WM_TRY(wm_check_set_rows(ctx, src, B, ""));
    const wm_dims &D = m->dims;
    int n_prompt = call.n_prompt;
    if (p.len) {   // ragged: the call's longest prompt
        n_prompt = 0;
        for (int b = 0; b < B; ++b) {
            WM_REQUIRE(p.len[b] >= 1 && p.len[b] <= p.stride, WM_ERR_INVALID, "row %d: prompt_len %d outside [1, %d]", b, p.len[b],
                       p.stride);
            n_prompt = std::max(n_prompt, (int)p.len[b]);
        }
    }
    cfg->n_prompt = n_prompt;
    WM_REQUIRE(n_prompt >= 1 && max_new >= 1 && n_prompt + max_new <= D.n_text_ctx, WM_ERR_INVALID,
               "prompt (%d) + new tokens (%d) must fit the %d-token context", n_prompt, max_new, D.n_text_ctx);
    for (int b = 0; b < (p.stride ? B : 1); ++b)
        for (int i = 0; i < (p.len ? p.len[b] : n_prompt); ++i) {
            const int32_t t = p.prompt[(size_t)b * p.stride + i];
            WM_REQUIRE(t >= 0 && t < D.n_vocab, WM_ERR_INVALID, "prompt token %d out of range", t);
        }
    WM_REQUIRE(call.eot < D.n_vocab, WM_ERR_INVALID, "eot %d outside the vocabulary", call.eot);
    WM_REQUIRE(budgets.empty() || (int)budgets.size() == B, WM_ERR_INVALID,
               "token budgets were set for %d chunks, the call has %d", (int)budgets.size(), B);
    for (auto &b : budgets) b = b > max_new ? max_new : b;
    XCfg &xc = cfg->xc;
    const wm_decode_opts *opts = call.opts;
    const float T = opts ? opts->temperature : 0.f;
    const int32_t ns_tok = opts ? opts->no_speech_token : -1;
    // (a ragged call places <|startoftranscript|> by sot_tail; opts->sot_index is not read)
    const int32_t sot_index = (opts && !p.len) ? opts->sot_index : 0;
    if (p.len && (call.no_speech_out || call.aligned)) {   // (an aligned call always reads sot_tail: its capture starts there)
        const int shortest = *std::min_element(p.len, p.len + B);
        WM_REQUIRE(p.sot_tail >= 1 && p.sot_tail <= shortest, WM_ERR_INVALID, "sot_tail %d outside [1, %d] (the shortest prompt)",
                   p.sot_tail, shortest);
    }
    WM_REQUIRE(std::isfinite(T) && T >= 0.f, WM_ERR_INVALID, "temperature must be finite and >= 0");
    // (1 / T must be a finite f32 too: an infinite scale turns a zero logit's score into NaN)
    WM_REQUIRE(T == 0.f || std::isfinite((float)(1.0 / (double)T)), WM_ERR_INVALID,
               "temperature %g is too small: 1 / T overflows", (double)T);
    WM_REQUIRE(sot_index >= 0 && sot_index < n_prompt, WM_ERR_INVALID, "sot_index %d outside the prompt [0, %d)",
               sot_index, n_prompt);
    WM_REQUIRE(ns_tok >= -1 && ns_tok < D.n_vocab, WM_ERR_INVALID, "no_speech_token %d outside the vocabulary", ns_tok);
    WM_REQUIRE(!call.no_speech_out || ns_tok >= 0, WM_ERR_INVALID, "no_speech_prob_out needs opts->no_speech_token");
    WM_REQUIRE(!call.beam || T == 0.f, WM_ERR_INVALID, "beam search decodes at temperature 0 (got %g)", (double)T);
    // the call's sampling row map (wm_set_sampling_rows checked the values): opts->temperature and opts->seed are validated above
    // and not read below.  A map without a sampling row is the temperature-0 call.
    const std::vector<float> &samp_T = pending.samp_T;
    const bool rows_map = !samp_T.empty();
    bool sampling = T > 0.f;
    if (rows_map) {
        WM_REQUIRE((int)samp_T.size() == B && pending.samp_seed.size() == samp_T.size(), WM_ERR_INVALID,
                   "the sampling row map was set for %d rows, the call has %d", (int)samp_T.size(), B);
        sampling = false;
        for (int b = 0; b < B; ++b) sampling = sampling || samp_T[b] > 0.f;
        cfg->samp_rows = sampling;
    }
    // (the beam close reads the filtered partials; the repetition rules live in the extended epilogue)
    const bool given = !pending.given_lens.empty();   // (a table without a given token changes no launch)
    const bool given_any = std::any_of(pending.given_lens.begin(), pending.given_lens.end(), [](int32_t n) { return n > 0; });
    xc.on = sampling || call.logprobs_out || call.no_speech_out || call.beam || m->rep_on || m->sb_on || m->sbt_on || m->cst_on || alt || given_any;
    if (alt) {   // the call's alternatives request (wm_request_alternatives checked n and the pointers)
        WM_TRY(tx_served(WM_PEND_ALT, call));
        WM_REQUIRE(alt->rows == (int64_t)B * call.n_cand && alt->max_new == max_new, WM_ERR_INVALID,
                   "alternatives were requested for %lld rows x %d tokens, the call has %lld x %d", (long long)alt->rows, alt->max_new,
                   (long long)B * call.n_cand, max_new);
    }
    if (given) {   // the call's given tokens (wm_set_given_tokens checked the ids and the lengths against the stride)
        WM_TRY(tx_served(WM_PEND_GIVEN, call));
        const int64_t rows = (int64_t)B * call.n_cand;
        WM_REQUIRE((int64_t)pending.given_lens.size() == rows, WM_ERR_INVALID, "given tokens were set for %d rows, the call has %lld",
                   (int)pending.given_lens.size(), (long long)rows);
        for (int64_t r = 0; r < rows; ++r)
            WM_REQUIRE(pending.given_lens[r] <= max_new, WM_ERR_INVALID, "row %lld: %d given tokens, the call generates at most %d",
                       (long long)r, pending.given_lens[r], max_new);
    }
    WM_REQUIRE(!m->rep_on || !ctx->dbg_hooks, WM_ERR_STATE, "the repetition rules are not supported by the all-f32 precision path");
    WM_REQUIRE(!(m->sb_on || m->sbt_on) || !ctx->dbg_hooks, WM_ERR_STATE, "the sequence bias is not supported by the all-f32 precision path");
    WM_REQUIRE(!(m->samp_on() && sampling) || !ctx->dbg_hooks, WM_ERR_STATE, "the sampling rules are not supported by the all-f32 precision path");
    // The two row maps' VALUES were checked by their setters against the context's tables / automaton, and whatever replaces those
    // (wm_model_set_sequence_bias, .._tables, wm_model_set_constraint) clears the pending map of the context it changes; wm_clone
    // starts without one.  So a map that arrives here fits what is in force on the CONTEXT: only its length is the call's.
    if (m->sbt_on) {   // row tables: the call's row map (wm_set_bias_rows), one entry per row of the call
        const int n = (int)pending.bias_rows.size();
        WM_REQUIRE(n, WM_ERR_STATE, "sequence-bias tables are in force and the call has no row map (wm_set_bias_rows)");
        WM_REQUIRE(n == B, WM_ERR_INVALID, "the bias row map was set for %d rows, the call has %d", n, B);
    }
    WM_REQUIRE(!m->cst_on || !ctx->dbg_hooks, WM_ERR_STATE, "the constraint is not supported by the all-f32 precision path");
    // the call's start states (wm_set_constraint_rows), one per row of the call; none: every row starts in 0
    WM_REQUIRE(!m->cst_on || pending.cst_rows.empty() || (int)pending.cst_rows.size() == B, WM_ERR_INVALID,
               "the constraint row map was set for %d rows, the call has %d", (int)pending.cst_rows.size(), B);
    xc.logprobs = call.logprobs_out;
    xc.no_speech = call.no_speech_out;
    const uint64_t seed = (opts && !rows_map) ? opts->seed : 0;
    xc.par.key0 = (unsigned)seed;
    xc.par.key1 = (unsigned)(seed >> 32);
    xc.par.sample = sampling ? 1 : 0;
    xc.par.inv_T = (T > 0.f && !rows_map) ? (float)(1.0 / (double)T) : 0.f;
    xc.par.rows_on = cfg->samp_rows ? 1 : 0;  // the rows' own 1 / T and keys: behind WmXDev::ids (lane_prefill)
    xc.par.sot_pos = call.no_speech_out ? sot_index : -1;
    xc.par.ns_tok = ns_tok;
    const bool no_stop = g_wm_tuning.no_early_stop != 0;   // probes only: decode every position, truncate on the host
    cfg->use_graph = !wm_graphs_off() && !ctx->prof.on && !call.dbg.beam_trace;   // (a traced call bakes nothing into graphs)
    cfg->stop.on = !no_stop && (call.eot >= 0 || !budgets.empty());
    cfg->stop.eot = call.eot;
    cfg->stop.budgets = budgets.empty() ? nullptr : budgets.data();
    if (call.aligned) {
        WM_REQUIRE(!ctx->dbg_hooks, WM_ERR_STATE, "aligned transcribe calls are not supported by the all-f32 precision path");
        WM_REQUIRE(call.start_out, WM_ERR_INVALID, "null start_frame_out");
        WM_REQUIRE(call.medfilt >= 1 && call.medfilt <= 31 && call.medfilt % 2 == 1, WM_ERR_INVALID,
                   "medfilt_width %d must be odd, 1 .. 31", call.medfilt);
        WM_REQUIRE(std::isfinite(call.qk_scale), WM_ERR_INVALID, "qk_scale must be finite");
        WM_REQUIRE(call.hyp || (call.n_cand == 1 && !call.beam), WM_ERR_INVALID, "an aligned call decodes one sample per row");
        WM_REQUIRE(!call.hyp || call.best_out, WM_ERR_INVALID, "null best_out: an aligned best-of / beam call aligns the hypothesis it names");
        cfg->sot_tail = p.len ? p.sot_tail : n_prompt - sot_index;
        wm_align_heads(m, &cfg->hl, &cfg->hh);
        // the capture budget's bound, in rows (the plan divides by the rows of a window); none when a full group fits
        const int N = call.n_cand;
        const int windows = wm_align_group_windows((size_t)cfg->sot_tail + max_new - 1, cfg->hl.size(), (size_t)max_new + 1, (size_t)N);
        cfg->max_group_rows = windows < WM_DEC_MAXB / N ? windows * N : 0;
    }
    return WM_OK;
}

// ---------------------------------------------------------------- lanes ----
// The contexts the plan's lanes run on, created on first use: the caller's context and its clones (wm_clone), the CU-masked
// clones of a partition (wm_clone_cus: a slice of the CUs of every XCD), or the solo lane.  *masks_refused: a device / driver
// that refuses CU-masked streams (a partitioned GPU, an older KFD) is not an error -- the caller falls back to the unmasked
// policy, once and for all.
int tx_lanes(wm_ctx *ctx, const WmTxPlan &plan, std::vector<wm_ctx *> *lanes, bool *masks_refused) {
    *masks_refused = false;
    lanes->clear();
    if (plan.kind == WM_LANES_PARTS) {
        const int parts = plan.parts;
        std::vector<wm_ctx *> &pl = ctx->part_lanes[parts - 2];
        while ((int)pl.size() < parts && !*masks_refused) {
            wm_ctx *c = nullptr;
            const int k = (int)pl.size();
            if (wm_clone_cus(ctx, k * 32 / parts, (k + 1) * 32 / parts, &c) != WM_OK) *masks_refused = true;   // 16 + 16, or 10 + 11 + 11 CUs of every XCD
            else pl.push_back(c);
        }
        WM_TRY(wm_ctx_make_current(ctx));
        if (!*masks_refused) lanes->assign(pl.begin(), pl.begin() + parts);
        return WM_OK;
    }
    if (plan.kind == WM_LANES_SOLO) {
        const int solo = g_wm_tuning.lane_solo_cus;   // probes only (0 in the product)
        WM_REQUIRE(solo >= 1 && solo <= 31, WM_ERR_INVALID, "lane_solo_cus: 1 .. 31 CUs per XCD");
        wm_ctx *&c = ctx->solo_lanes[solo];
        if (!c) WM_TRY(wm_clone_cus(ctx, 0, solo, &c));
        lanes->assign(plan.n_lanes, c);
        return WM_OK;
    }
    while ((int)ctx->lanes.size() < plan.n_lanes - 1) {
        wm_ctx *c = nullptr;
        WM_TRY(wm_clone(ctx, &c));
        ctx->lanes.push_back(c);
    }
    lanes->push_back(ctx);
    lanes->insert(lanes->end(), ctx->lanes.begin(), ctx->lanes.begin() + (plan.n_lanes - 1));
    return WM_OK;
}

// ---------------------------------------------------------------- the scheduler ----
// decodes in flight on this device (this call included): other lanes of this call, other contexts' calls
struct ActiveGuard {
    std::atomic<int> &n;
    explicit ActiveGuard(std::atomic<int> &a) : n(a) { n.fetch_add(1, std::memory_order_relaxed); }
    ~ActiveGuard() { n.fetch_sub(1, std::memory_order_relaxed); }
};

struct TxRun {
    wm_ctx *ctx;
    const TxCall &call;
    const TxCfg &cfg;
    const WmTxPlan &plan;
    std::vector<LaneJob> jobs;
    int next_group = 0, groups_done = 0;
    // (a ragged call: a group's prompt positions are its own longest prompt, LaneJob::P)
    int n_steps(const LaneJob &j) const { return j.P + call.max_new - 1; }
    bool decoding(const LaneJob &j) const { return j.state == LaneJob::DECODING && j.t < n_steps(j) && !j.stopped; }
};

// an idle lane takes the next group: prefill, its graph set
int lane_start(TxRun &r, LaneJob &j) {
    const TxCall &call = r.call;
    const int g = r.next_group++;
    j.Cg = r.plan.cg[g];
    j.b0 = r.plan.b0[g];
    j.Bg = j.Cg * call.n_cand;
    j.t = 0; j.bursts = 0; j.stopped = false;
    j.bpar.max_cand = call.max_cand; j.bpar.max_new = call.max_new; j.bpar.eot = call.eot; j.bpar.pad = call.eot >= 0 ? call.eot : 0;
    WM_TRY(lane_prefill(j, call, r.cfg));
    WM_TRY(lane_prompt_panels(j, call, r.ctx));
    lane_given_plan(j, call, r.ctx);
    if (r.cfg.use_graph) WM_TRY(lane_graph(j, j.P));
    j.state = LaneJob::DECODING;
    return WM_OK;
}

enum LaneStep { LANE_WAITS, LANE_MOVED, LANE_ENQUEUED_ALL };

// a decoding lane enqueues its next burst, unless it has to wait for the device or has nothing left to enqueue
int lane_advance(TxRun &r, LaneJob &j, LaneStep *step) {
    *step = LANE_WAITS;
    if (r.cfg.stop.on && j.bursts >= 2 && !j.stopped) {
        // stay at most two bursts ahead of the GPU: burst (bursts - 2) must have finished, and its live count
        // says whether there is anything left to decode
        const int slot = (j.bursts - 2) % WM_NLIVE_RING;
        const hipError_t q = hipEventQuery(j.burst_ev[slot]);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); return WM_OK; }   // "not ready" is not an error to keep
        WM_HIP(q);
        if (j.c->model->h_nlive[slot] == 0) j.stopped = true;
    }
    if (!r.decoding(j)) {   // everything enqueued, or nothing left to decode
        *step = LANE_ENQUEUED_ALL;
        return WM_OK;
    }
    // does this burst share the chip?  other lanes of this call still decoding, or other calls in flight
    int busy = 0;
    for (const LaneJob &o : r.jobs) busy += r.decoding(o);
    // (sub-chip lanes own their CUs: the other lanes of THIS call do not make the chip "shared")
    const bool shared = (busy > 1 && r.plan.kind != WM_LANES_PARTS) ||
                        g_wm_active_decodes[r.ctx->device & 63].load(std::memory_order_relaxed) > 1;
    WM_TRY(lane_burst(j, j.P, r.n_steps(j), r.cfg.use_graph, shared));
    *step = LANE_MOVED;
    return WM_OK;
}

// everything is enqueued: fetch the token streams, the log-probs, the no-speech probabilities, a beam group's state
int lane_fetch(TxRun &r, LaneJob &j) {
    const TxCall &call = r.call;
    const XCfg &xc = r.cfg.xc;
    WmModel *m = j.c->model;
    WM_HIP(hipEventRecord(j.ev[3], j.c->stream));
    j.gen.resize((size_t)call.max_new * j.Bg);  // dseq[P + i][b]
    WM_HIP(hipMemcpyAsync(j.gen.data(), m->dseq + (size_t)j.P * j.Bg, j.gen.size() * 4, hipMemcpyDeviceToHost, j.c->stream));
    if (xc.logprobs && !call.beam) {   // [gi][b], laid out like dseq
        j.lp.resize((size_t)call.max_new * j.Bg);
        WM_HIP(hipMemcpyAsync(j.lp.data(), m->dx_logprob, j.lp.size() * 4, hipMemcpyDeviceToHost, j.c->stream));
    }
    if (xc.no_speech) {
        j.ns.resize(j.Bg);
        WM_HIP(hipMemcpyAsync(j.ns.data(), m->dx_nospeech, j.ns.size() * 4, hipMemcpyDeviceToHost, j.c->stream));
    }
    if (j.mode.alt) {   // [gi][b][n] and [gi][b], as the kernel left them
        const size_t np = (size_t)call.max_new * j.Bg;
        j.atok.resize(np * j.apar.n); j.alp.resize(np * j.apar.n); j.acnt.resize(np); j.aent.resize(np);
        WM_HIP(hipMemcpyAsync(j.atok.data(), j.apar.tok, j.atok.size() * 4, hipMemcpyDeviceToHost, j.c->stream));
        WM_HIP(hipMemcpyAsync(j.alp.data(), j.apar.lp, j.alp.size() * 4, hipMemcpyDeviceToHost, j.c->stream));
        WM_HIP(hipMemcpyAsync(j.acnt.data(), j.apar.cnt, np * 4, hipMemcpyDeviceToHost, j.c->stream));
        WM_HIP(hipMemcpyAsync(j.aent.data(), j.apar.ent, np * 4, hipMemcpyDeviceToHost, j.c->stream));
    }
    if (call.beam) WM_TRY(beam_fetch(j, call.max_new, call.dbg.beam_trace != nullptr));
    j.state = LaneJob::DRAINING;
    return WM_OK;
}

// ---------------------------------------------------------------- the ranking step ----
// The hypothesis of window b a best-of or beam call names in best_out: a best-of call's is wm_rank_candidates' over the
// candidates' log-probs, a beam call's the MaximumLikelihoodRanker's over the search's own sums.  Per window, so that an aligned
// group ranks its windows as soon as their outputs are written (lane_finish) and every other call at its end (tx_rank).
int tx_rank_window(const TxCall &call, int b) {
    const int max_new = call.max_new, S = call.out_stride();
    const size_t r0 = (size_t)b * S;
    if (!call.beam)
        return wm_rank_candidates(call.tokens_out + r0 * max_new, call.lens_out + r0, call.logprobs_out + r0 * max_new, 1, S, max_new,
                                  call.eot, call.length_penalty, call.best_out + b, nullptr);
    int best = 0;
    double best_score = -INFINITY;
    for (int h = 0; h < call.n_hyp[b]; ++h) {
        const size_t r = r0 + h;
        int n_text = 0;
        while (n_text < call.lens_out[r] && call.tokens_out[r * max_new + n_text] != call.eot) ++n_text;
        const double score = wm_rank_score((double)call.sums[r], n_text, call.length_penalty);
        if (score > best_score) { best_score = score; best = h; }   // the first maximal score; all -inf: hypothesis 0
    }
    call.best_out[b] = best;
    return WM_OK;
}

// The tail of an aligned group, enqueued once its rows' lengths are known: matrix row k of a window is the decoder position whose
// output was generated token k, i.e. capture row S + k with S = sot_tail - 1 rows in front (the prompt from
// <|startoftranscript|> on, less the one whose output is token 0); a window's decoder rows are S + len, none behind the last
// matrix row (WmAlignDev::tail 0).  Against the lane's own cross-K/V, on the lane's stream.
// A group of candidates or beams (N rows per window) aligns hypothesis best_out of each window: its capture rows are gathered
// from the slots that held them -- a candidate's own slot; a beam hypothesis' by wm_beam_ancestry over the fetched search
// state -- into the layout of a plain group of Cg rows, which the same two launches then read.
int lane_align(TxRun &r, LaneJob &j) {
    const TxCall &call = r.call;
    wm_ctx *c = j.c;
    WmModel *m = c->model;
    const int Cg = j.Cg, N = call.n_cand, S = r.cfg.sot_tail - 1, n_ld = j.aw.n_ld, J = j.aw.J, Tq = j.aw.Tq;
    char *ws = (char *)m->acap_ws.p;
    int nmax = -1, mmax = 0, rows_max = 0;
    j.aok.assign(Cg, 0);
    j.alen.assign(Cg, 0);
    int32_t *grows = N > 1 ? j.aints.data() + 4 * Cg + 2 * J : nullptr, *slots = N > 1 ? grows + Cg : nullptr;
    // a beam group's fetched state (beam_drain)
    WmBeamDev bm;
    memset(&bm, 0, sizeof(bm));
    if (call.beam && N > 1) WM_TRY(wm_model_beam_dev(c, j.mode, &bm));
    const char *dev0 = (const char *)m->beam_ws.p;
    auto host = [&](const void *dev) { return j.bstate.data() + ((const char *)dev - dev0); };
    for (int w = 0; w < Cg; ++w) {
        const int W = j.b0 + w;   // window of the call
        int h = 0;
        if (call.hyp) {
            h = call.best_out[W];
            if (call.dbg.align_hyp >= 0) h = std::min(call.dbg.align_hyp, (call.beam ? call.n_hyp[W] : N) - 1);
        }
        const int len = call.lens_out[(size_t)W * call.out_stride() + h];
        const int nf = call.src.windows ? call.src.set->n_frames[call.src.rows ? call.src.rows[W] : W] : call.src.n_frames[W];
        const bool ok = len >= 1 && nf >= 2 && S + len >= 2;
        j.aok[w] = ok;
        j.alen[w] = len;
        j.aints[w] = ok ? len - 1 : -1;
        j.aints[Cg + w] = nf;
        j.aints[2 * Cg + w] = ok ? len : 0;
        j.aints[3 * Cg + w] = nf / 2;
        if (ok) { nmax = std::max(nmax, len - 1); mmax = std::max(mmax, nf / 2); rows_max = std::max(rows_max, len); }
        if (N > 1) {
            grows[w] = ok ? S + len : 0;
            int32_t *sl = slots + (size_t)w * Tq;
            std::fill(sl, sl + Tq, call.beam ? 0 : h);   // a candidate keeps its slot
            if (call.beam && h >= 0) {
                const int got = wm_beam_ancestry(N, j.banc.data() + (size_t)w * N, j.Bg, ((const int *)host(bm.fin_n))[w],
                                                 j.bfin_src.data() + (size_t)w * WM_MAX_BEAM_HYPS,
                                                 (const int *)host(bm.fin_len) + (size_t)w * WM_MAX_BEAM_HYPS,
                                                 ((const int *)host(bm.wsteps))[w], (const float *)host(bm.sum) + (size_t)w * N, h, S, Tq, sl);
                WM_REQUIRE(got == len || (got < 0 && len == 0), WM_ERR_STATE, "aligned beam group: window %d, hypothesis %d has %d tokens, its ancestry %d", W, h, len, got);
            }
        }
        if (call.dbg.align_slots)
            for (int t = 0; t < Tq; ++t) call.dbg.align_slots[(size_t)W * Tq + t] = N > 1 ? slots[(size_t)w * Tq + t] : 0;
    }
    WM_HIP(hipEventRecord(j.tail_ev[0], c->stream));
    if (nmax >= 0) {
        int *ints = (int *)(ws + j.aw.ints);
        float *x = (float *)(ws + j.aw.x);
        WM_HIP(hipMemcpyAsync(ints, j.aints.data(), j.aints.size() * 4, hipMemcpyHostToDevice, c->stream));
        WmAlignDev a;
        a.q = j.mode.acap_q;
        if (N > 1) {
            float *sel = (float *)(ws + j.aw.sel);
            WM_TRY(wm_align_gather(c, j.mode.acap_q, sel, ints + 5 * Cg + 2 * J, ints + 4 * Cg + 2 * J, Cg, N, Tq, J));
            a.q = sel;
        }
        a.xkv = m->xkv; a.hl = ints + 4 * Cg; a.hh = ints + 4 * Cg + J; a.n_text = ints; a.n_frames = ints + Cg;
        a.rowst = (float *)(ws + j.aw.row); a.colst = (float *)(ws + j.aw.col); a.x = x;
        a.B = Cg; a.H = m->dims.n_text_head; a.Tq = Tq; a.J = J; a.S = S; a.n_ld = n_ld;
        a.sc = 0.125f * call.qk_scale * 1.44269504088896340736f;
        a.half = call.medfilt / 2;
        a.tail = 0; a.n_min = 0;
        WM_TRY(wm_align_matrix(c, a, nmax, mmax));
        int *start = (int *)(ws + j.aw.start);
        WM_TRY(wm_dtw(c, x, (long)n_ld * 1500, 1500, ints + 2 * Cg, ints + 3 * Cg, Cg, rows_max, mmax, (unsigned *)(ws + j.aw.tr), start, n_ld));
        j.astart.resize((size_t)Cg * n_ld);
        WM_HIP(hipMemcpyAsync(j.astart.data(), start, j.astart.size() * 4, hipMemcpyDeviceToHost, c->stream));
        if (call.dbg.align_matrix)
            WM_HIP(hipMemcpyAsync(call.dbg.align_matrix + (size_t)j.b0 * n_ld * 1500, x, (size_t)Cg * n_ld * 1500 * 4, hipMemcpyDeviceToHost, c->stream));
    }
    WM_HIP(hipEventRecord(j.tail_ev[1], c->stream));
    j.state = LaneJob::ALIGNING;
    return WM_OK;
}

// A draining lane whose stream has drained writes its rows of the call's outputs and adds its stage times.  A decode group
// runs for seconds -- poll instead of spinning in hipStreamSynchronize, so that the host threads of the other lanes / ranks
// (one process per GPU, several contexts each) keep their cores.
int lane_finish(TxRun &r, LaneJob &j, bool *done) {
    const TxCall &call = r.call;
    *done = false;
    const hipError_t q = hipStreamQuery(j.c->stream);
    if (q == hipErrorNotReady) { (void)hipGetLastError(); return WM_OK; }
    WM_HIP(q);
    WM_HIP(hipStreamSynchronize(j.c->stream));
    if (call.beam) {
        j.c->model->beam_trace_on = false;
        beam_drain(j, call);
    } else {
        wm_group_rows_out(j.gen.data(), j.lp.data(), j.ns.data(), r.cfg.stop.budgets, call.eot, call.n_cand, j.b0, j.Bg, call.max_new,
                          call.tokens_out, call.lens_out, r.cfg.xc.logprobs, r.cfg.xc.no_speech);
        if (const wm_alternatives_out *a = r.cfg.pending->alt_on ? &r.cfg.pending->alt : nullptr)   // by the row map and the lengths just written
            wm_group_alt_out(j.atok.data(), j.alp.data(), j.acnt.data(), j.aent.data(), a->n, call.n_cand, j.b0, j.Bg, call.max_new,
                             call.lens_out, a->tokens, a->logprobs, a->counts, a->entropy);
    }
    wm_add_stage_ms(j.ev.e, 3, call.src.windows, j.stage_sum);
    if (call.aligned) {   // the rows' lengths are known now: (candidates, beams) the windows' ranking, the alignment tail, then ALIGNING
        if (call.hyp)
            for (int w = 0; w < j.Cg; ++w) WM_TRY(tx_rank_window(call, j.b0 + w));
        return lane_align(r, j);
    }
    j.state = LaneJob::IDLE;
    ++r.groups_done;
    *done = true;
    return WM_OK;
}

// An aligned group whose tail has drained writes its windows' rows of start_frame_out (of the hypothesis lane_align chose): row
// k < len starts at the first frame of matrix row k on the DTW path, entry len is M, -1 behind; a row without a matrix is all
// -1, or (0, M) when its one decoder row has nothing to be z-scored against.
int lane_align_finish(TxRun &r, LaneJob &j, bool *done) {
    const TxCall &call = r.call;
    *done = false;
    const hipError_t q = hipStreamQuery(j.c->stream);
    if (q == hipErrorNotReady) { (void)hipGetLastError(); return WM_OK; }
    WM_HIP(q);
    WM_HIP(hipStreamSynchronize(j.c->stream));
    const int n_ld = j.aw.n_ld, Cg = j.Cg;
    for (int b = 0; b < Cg; ++b) {
        int32_t *out = call.start_out + (size_t)(j.b0 + b) * n_ld;
        const int len = j.alen[b], nf = j.aints[Cg + b], M = nf / 2;
        for (int k = 0; k < n_ld; ++k) out[k] = -1;
        if (j.aok[b]) {
            for (int k = 0; k < len; ++k) out[k] = j.astart[(size_t)b * n_ld + k];
            out[len] = M;
        } else if (len == 1 && nf >= 2) {   // R = 1: the standard deviation over one row is zero
            out[0] = 0;
            out[1] = M;
        }
    }
    float ms;
    if (hipEventElapsedTime(&ms, j.tail_ev[0], j.tail_ev[1]) == hipSuccess) j.stage_sum[2] += ms;
    j.state = LaneJob::IDLE;
    ++r.groups_done;
    *done = true;
    return WM_OK;
}

// The single host thread drives the lanes round-robin, one step per lane and turn, and sleeps 100 us when nobody moved.  A
// prefill ends the lane's turn, so every lane has its prefill before anyone's first burst.
int tx_run(wm_ctx *ctx, const TxCall &call, const TxCfg &cfg, const WmTxPlan &plan, const std::vector<wm_ctx *> &lanes) {
    TxRun r{ctx, call, cfg, plan, std::vector<LaneJob>(lanes.size())};
    for (size_t l = 0; l < lanes.size(); ++l) {
        LaneJob &j = r.jobs[l];
        j.c = lanes[l];
        j.fence.s = j.c->stream;
        WM_TRY(j.ev.create());
        if (cfg.stop.on) WM_TRY(j.burst_ev.create_untimed());
        if (call.aligned) WM_TRY(j.tail_ev.create());
    }
    ctx->stage_ms[0] = ctx->stage_ms[1] = ctx->stage_ms[2] = 0.f;
    ActiveGuard active_guard(g_wm_active_decodes[ctx->device & 63]);
    while (r.groups_done < plan.G) {
        bool progress = false;
        for (LaneJob &j : r.jobs) {
            WM_TRY(wm_ctx_make_current(j.c));
            if (j.state == LaneJob::IDLE) {
                if (r.next_group >= plan.G) continue;
                WM_TRY(lane_start(r, j));
                progress = true;
            } else if (j.state == LaneJob::DECODING) {
                LaneStep step;
                WM_TRY(lane_advance(r, j, &step));
                if (step == LANE_ENQUEUED_ALL) WM_TRY(lane_fetch(r, j));
                progress |= step != LANE_WAITS;
            } else if (j.state == LaneJob::DRAINING) {
                bool done;
                WM_TRY(lane_finish(r, j, &done));
                progress |= done || j.state == LaneJob::ALIGNING;
            } else {
                bool done;
                WM_TRY(lane_align_finish(r, j, &done));
                progress |= done;
            }
        }
        if (!progress) usleep(100);
    }
    for (const LaneJob &j : r.jobs)   // lanes overlap: the busiest lane per stage
        for (int i = 0; i < 3; ++i)
            if (j.stage_sum[i] > ctx->stage_ms[i]) ctx->stage_ms[i] = j.stage_sum[i];
    return WM_OK;
}

// the ranking step of a best-of or beam call (an aligned one has ranked its windows group by group: lane_finish)
int tx_rank(const TxCall &call) {
    if (!call.best_out || (call.aligned && call.hyp)) return WM_OK;
    for (int b = 0; b < call.B; ++b) WM_TRY(tx_rank_window(call, b));
    return WM_OK;
}

// ---------------------------------------------------------------- the call ----
int tx_transcribe(wm_ctx *ctx, TxCall &call) {
    // whatever was armed for THIS call is consumed by it: a failed check must not leave it armed for a later, unrelated call
    WmPending pending = tx_take(ctx, call);
    call.dbg = pending.dbg;
    if (!call.beam) call.dbg.beam_trace = nullptr;   // (an aligned call's captures are read on its own paths alone)
    WM_TRY(tx_served(pending.bits() & WM_PEND_SAMP_ROWS, call));   // (in front of the entry's own checks; alternatives: tx_validate)
    WM_TRY(entry_checks(call));
    WM_MODEL(ctx);
    std::vector<float> lp_own;   // best_out ranks by the log-probs whether or not the caller wants them
    if (call.entry == TxCall::BEST_OF && call.best_out && !call.logprobs_out) {
        lp_own.resize((size_t)call.B * call.n_cand * call.max_new);
        call.logprobs_out = lp_own.data();
    }
    TxCfg cfg;
    WM_TRY(tx_validate(ctx, call, pending, &cfg));
    // the plan: decode groups and lanes.  A masked clone that cannot be made switches the masks off and asks again.
    WmTxPlanIn pin;
    pin.B = call.B; pin.N = call.n_cand;
    pin.explicit_lanes = ctx->max_lanes > 0;
    pin.lanes = pin.explicit_lanes ? ctx->max_lanes : lane_limit();
    pin.prof_on = ctx->prof.on; pin.no_cu_masks = ctx->no_cu_masks; pin.n_text_state = m->dims.n_text_state;
    pin.max_group_rows = cfg.max_group_rows;   // (an aligned call under its capture budget; else 0: none)
    WmTxPlan plan;
    std::vector<wm_ctx *> lanes;
    bool masks_refused = false;
    wm_tx_plan(pin, g_wm_tuning, &plan);
    WM_TRY(tx_lanes(ctx, plan, &lanes, &masks_refused));
    if (masks_refused) {
        ctx->no_cu_masks = pin.no_cu_masks = true;
        wm_tx_plan(pin, g_wm_tuning, &plan);
        WM_TRY(tx_lanes(ctx, plan, &lanes, &masks_refused));
    }
    if (call.aligned) {   // rows of a group that never ran (an error below) read "no alignment"
        std::fill(call.start_out, call.start_out + (size_t)call.B * (call.max_new + 1), -1);
        if (call.dbg.align_matrix) memset(call.dbg.align_matrix, 0, (size_t)call.B * (call.max_new + 1) * 1500 * 4);
    }
    WM_TRY(tx_run(ctx, call, cfg, plan, lanes));
    return tx_rank(call);
}

// ---------------------------------------------------------------- filling a call ----
void mel_src(TxCall &call, const float *mel, const int64_t *mel_base, const int32_t *mel_len, const int32_t *seek,
             const int32_t *n_frames, wm_mem mem) {
    call.src.mel = mel; call.src.mel_base = mel_base; call.src.mel_len = mel_len; call.src.seek = seek; call.src.n_frames = n_frames;
    call.mem = mem;
}

void set_src(TxCall &call, const wm_windows *w, const int32_t *rows) {
    call.windows = call.src.windows = true; call.src.set = w; call.src.rows = rows;
    call.mem = WM_MEM_HOST;
}

void outputs(TxCall &call, int B, int max_new, int32_t eot, const wm_decode_opts *opts, int32_t *tokens_out, int32_t *lens_out,
             float *logprobs_out, float *no_speech_out) {
    call.B = B; call.max_new = max_new; call.eot = eot; call.opts = opts;
    call.tokens_out = tokens_out; call.lens_out = lens_out; call.logprobs_out = logprobs_out; call.no_speech_out = no_speech_out;
}

// wm_transcribe_mel_ragged / wm_transcribe_mel with best_of candidates per row (TxCall::n_cand): one encoder pass, one
// cross-K/V cache and one read of it per window, best_of decoder rows (lane_prefill, wm_dec_attention_cand)
void best_of(TxCall &call, const int32_t *prompts, int prompt_stride, const int32_t *prompt_len, int sot_tail,
             const uint32_t *sample_ids, int n, float length_penalty, int32_t *best_out) {
    call.entry = TxCall::BEST_OF;
    call.prompts = {prompts, prompt_stride, prompt_len, sot_tail, sample_ids};
    call.n_prompt = prompt_stride;
    call.n_cand = n; call.length_penalty = length_penalty; call.best_out = best_out;
}

// Beam search: the call of wm_transcribe_mel_best_of with the rows of a window as its BEAMS (TxCall::beam) -- the same groups,
// the same prompt phase, one cross-K/V read per window; the generating positions close with the beam kernels (beam.hip)
void beam(TxCall &call, const int32_t *prompts, int prompt_stride, const int32_t *prompt_len, int sot_tail,
          int beam_size, int max_candidates, float length_penalty, int32_t *n_hyp_out, float *sum_logprobs_out, int32_t *best_out) {
    call.entry = TxCall::BEAM;
    call.prompts = {prompts, prompt_stride, prompt_len, sot_tail, nullptr};
    call.n_prompt = prompt_stride;
    call.n_cand = beam_size; call.beam = true; call.max_cand = max_candidates; call.length_penalty = length_penalty;
    call.n_hyp = n_hyp_out; call.sums = sum_logprobs_out; call.best_out = best_out;
}

// the aligned calls: their three arguments
// hyp: a best-of / beam counterpart, which aligns the hypothesis best_out names
void aligned(TxCall &call, int medfilt_width, float qk_scale, int32_t *start_frame_out, bool hyp = false) {
    call.aligned = true; call.medfilt = medfilt_width; call.qk_scale = qk_scale; call.start_out = start_frame_out;
    call.hyp = hyp;
}

// ---------------------------------------------------------------- speculative decoding ----
// wm_transcribe_mel_speculative.  A decode group of G windows lives on TWO contexts: the target (the
// caller's, whose plain call this one reproduces bit for bit) and the draft.  Both prefill and step through the prompt exactly
// as a plain group does and take the first generated token with a plain step; then rounds of [draft: w plain steps | target:
// proposals staged, ONE verify step of G x w rows, accept + commit] until the device reports no live window.  The two streams
// are ordered by events; the host reads a round's (live windows, position) through pinned memory, at most two rounds behind.
struct SpecCall {
    wm_ctx *draft = nullptr;
    int k = 0;                        // draft_len
    wm_spec_stats *stats = nullptr;   // [B] of the call, nullable
};

int spec_checks(wm_ctx *ctx, const SpecCall &sc, const TxCall &call) {
    WM_REQUIRE(sc.draft && sc.draft != ctx, WM_ERR_INVALID, "speculative decoding needs a draft context of its own (a wm_clone will do)");
    WM_REQUIRE(sc.k >= 1 && sc.k <= WM_MAX_DRAFT_LEN, WM_ERR_INVALID, "draft_len %d outside [1, %d]", sc.k, WM_MAX_DRAFT_LEN);
    const float T = call.opts ? call.opts->temperature : 0.f;
    WM_REQUIRE(T == 0.f, WM_ERR_INVALID, "speculative decoding verifies the greedy choice: temperature must be 0 (got %g)", (double)T);
    WmModel *m = ctx->model, *dm = sc.draft->model;
    WM_REQUIRE(!m->rep_on, WM_ERR_STATE, "speculative decoding does not support the repetition rules set on this context");
    WM_REQUIRE(!m->sb_on && !m->sbt_on, WM_ERR_STATE, "speculative decoding does not support the sequence bias set on this context");
    WM_REQUIRE(!m->cst_on, WM_ERR_STATE, "speculative decoding does not support the constraint set on this context");
    WM_REQUIRE(!ctx->dbg_hooks && !sc.draft->dbg_hooks, WM_ERR_STATE, "speculative decoding is not supported by the all-f32 precision path");
    WM_REQUIRE(dm && dm->finalized, WM_ERR_STATE, "the draft's model weights are not finalised (wm_finalize)");
    WM_REQUIRE(sc.draft->device == ctx->device, WM_ERR_INVALID, "the draft context lives on device %d, the target on %d",
               sc.draft->device, ctx->device);
    const wm_dims &a = m->dims, &b = dm->dims;
    WM_REQUIRE(a.n_mels == b.n_mels && a.n_vocab == b.n_vocab && a.n_text_ctx == b.n_text_ctx && a.n_audio_ctx == b.n_audio_ctx,
               WM_ERR_INVALID, "the draft's n_mels / n_vocab / n_text_ctx / n_audio_ctx (%d / %d / %d / %d) differ from the target's (%d / %d / %d / %d)",
               b.n_mels, b.n_vocab, b.n_text_ctx, b.n_audio_ctx, a.n_mels, a.n_vocab, a.n_text_ctx, a.n_audio_ctx);
    WM_REQUIRE(!dm->rep_on && !dm->sb_on && !dm->sbt_on && !dm->cst_on, WM_ERR_STATE,
               "the draft context has repetition rules, a sequence bias or a constraint set");
    return WM_OK;
}

int spec_group(wm_ctx *ctx, const SpecCall &sc, const TxCall &call, const TxCfg &cfg, const TxCfg &dcfg, int b0, int G) {
    wm_ctx *dc = sc.draft;
    WmModel *m = ctx->model, *dm = dc->model;
    const int k = sc.k, n_ctx = m->dims.n_text_ctx, max_new = call.max_new;
    std::vector<int32_t> script, stats;   // (sources / destinations of asynchronous copies: declared before the jobs' fences)
    WmEvents<WM_NLIVE_RING> round_ev;
    WmEvents<2> x_ev;
    LaneJob tj, dj;
    tj.c = ctx; tj.fence.s = ctx->stream;
    dj.c = dc; dj.fence.s = dc->stream;
    WM_TRY(tj.ev.create());
    WM_TRY(dj.ev.create());
    WM_TRY(round_ev.create_untimed());
    WM_TRY(x_ev.create_untimed());
    tj.b0 = dj.b0 = b0; tj.Cg = dj.Cg = tj.Bg = dj.Bg = G;
    WmSpecDev sp;
    int *script_area = nullptr;
    WM_TRY(wm_model_spec_dev(ctx, dc, max_new, &sp, &script_area));
    WM_TRY(lane_prefill(tj, call, cfg));
    WM_TRY(lane_prefill(dj, call, dcfg));
    const int P = tj.P;
    if (const int32_t *s = cfg.pending->dbg.spec_script) {   // debug library: the proposals come from the script (the draft still runs)
        script.assign(s + (size_t)b0 * max_new, s + (size_t)(b0 + G) * max_new);
        WM_HIP(hipMemcpyAsync(script_area, script.data(), script.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        sp.script = script_area;
    }
    // the prompt and the first generated token: plain steps on both models
    for (int i = 0; i < P; ++i) WM_TRY(lane_position(tj, tj.mode, P, false));
    for (int i = 0; i < P; ++i) WM_TRY(lane_position(dj, dj.mode, P, false));
    const WmXDev xd = wm_model_x_dev(m, tj.mode);
    const WmStopDev stop = wm_model_stop_dev(m, tj.mode);
    const int fallback = tj.mode.ts ? m->ts_eot : 0;
    auto draft_embed = [&]() {   // the draft's next step starts from the token the commit left at its position
        return wm_dec_embed_panel(dc, dm->dseq, G, dm->dpos, 0, G, 1, n_ctx, wm_model_embed_dev(dm));
    };
    const int last = P + max_new - 2;   // the last position a row may have: its output is generated token max_new - 1
    int rounds = 0, seen = 0, bound = P;
    bool stopped = false;
    std::vector<int> widths;
    if (max_new > 1) {
        WM_HIP(hipEventRecord(x_ev[1], ctx->stream));
        WM_HIP(hipStreamWaitEvent(dc->stream, x_ev[1], 0));
        WM_TRY(wm_spec_adopt(dc, sp, G, P));
        WM_TRY(draft_embed());
    }
    while (max_new > 1) {
        int w = wm_spec_width(k, bound, last);
        // at most two rounds ahead of the device -- and when the bound on the position leaves no room, what the device says
        while (seen < rounds && (rounds - seen >= 2 || w == 0)) {
            const int slot = seen % WM_NLIVE_RING;
            WM_HIP(hipEventSynchronize(round_ev[slot]));
            if (m->h_spec[slot * 2] == 0) stopped = true;
            bound = m->h_spec[slot * 2 + 1];
            ++seen;
            for (int r = seen; r < rounds; ++r) bound += widths[r];
            w = wm_spec_width(k, bound, last);
        }
        if (stopped || w == 0) break;
        // DRAFT: w plain greedy steps from the target's last token (the last one for its cache alone)
        for (int s = 0; s < w; ++s) WM_TRY(lane_position(dj, dj.mode, P, false));
        WM_HIP(hipEventRecord(x_ev[0], dc->stream));
        WM_HIP(hipStreamWaitEvent(ctx->stream, x_ev[0], 0));
        // VERIFY: the proposals behind the last token, one panel step of G x w rows, then accept + commit
        WM_TRY(wm_spec_stage(ctx, sp, G, w, P, n_ctx));
        WM_TRY(wm_dec_embed_panel(ctx, m->dseq, G, m->dpos, 0, G, w, n_ctx, wm_model_embed_dev(m)));
        WM_TRY(wm_model_spec_panel_step(ctx, G, w, tj.mode, P));
        WM_TRY(wm_spec_accept(ctx, m->dargmax, m->vpad / 16, sp, xd, stop, G, w, P, n_ctx, fallback));
        const int slot = rounds % WM_NLIVE_RING;
        WM_HIP(hipMemcpyAsync(m->h_spec + slot * 2, sp.round, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        WM_HIP(hipEventRecord(round_ev[slot], ctx->stream));
        WM_HIP(hipStreamWaitEvent(dc->stream, round_ev[slot], 0));
        WM_TRY(draft_embed());
        widths.push_back(w);
        bound += w;
        ++rounds;
    }
    // the group's streams, as a plain group fetches them
    WM_HIP(hipEventRecord(tj.ev[3], ctx->stream));
    tj.gen.resize((size_t)max_new * G);
    WM_HIP(hipMemcpyAsync(tj.gen.data(), m->dseq + (size_t)P * G, tj.gen.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (cfg.xc.logprobs) {
        tj.lp.resize((size_t)max_new * G);
        WM_HIP(hipMemcpyAsync(tj.lp.data(), m->dx_logprob, tj.lp.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (cfg.xc.no_speech) {
        tj.ns.resize(G);
        WM_HIP(hipMemcpyAsync(tj.ns.data(), m->dx_nospeech, tj.ns.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (sc.stats && max_new > 1) {
        stats.resize((size_t)G * 4);
        WM_HIP(hipMemcpyAsync(stats.data(), sp.stats, stats.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    WM_HIP(hipStreamSynchronize(ctx->stream));
    WM_HIP(hipStreamSynchronize(dc->stream));
    wm_group_rows_out(tj.gen.data(), tj.lp.data(), tj.ns.data(), cfg.stop.budgets, call.eot, 1, b0, G, max_new, call.tokens_out,
                      call.lens_out, cfg.xc.logprobs, cfg.xc.no_speech);
    if (sc.stats)
        for (int c = 0; c < G; ++c) {
            wm_spec_stats &o = sc.stats[b0 + c];
            o.rounds = o.proposed = o.accepted = o.kept = 0;
            if (!stats.empty()) { o.rounds = stats[c * 4]; o.proposed = stats[c * 4 + 1]; o.accepted = stats[c * 4 + 2]; o.kept = stats[c * 4 + 3]; }
        }
    wm_add_stage_ms(tj.ev.e, 3, false, tj.stage_sum);
    for (int i = 0; i < 3; ++i) ctx->stage_ms[i] += tj.stage_sum[i];
    return WM_OK;
}

int tx_speculative(wm_ctx *ctx, const SpecCall &sc, TxCall &call) {
    WmPending pending = tx_take(ctx, call);   // (alternatives and a sampling row map are refused below: it verifies the greedy choice)
    WM_TRY(entry_checks(call));
    WM_MODEL(ctx);
    WM_TRY(spec_checks(ctx, sc, call));
    WM_TRY(tx_served(pending.bits(), call));
    TxCfg cfg;
    WM_TRY(tx_validate(ctx, call, pending, &cfg));
    const WmDebugShots &dbg = pending.dbg;
    WM_REQUIRE(!dbg.spec_script || (dbg.spec_script_new == call.max_new && dbg.spec_script_rows == call.B), WM_ERR_INVALID,
               "the proposal script was set for %d rows x %d tokens, the call has %d x %d", dbg.spec_script_rows, dbg.spec_script_new, call.B, call.max_new);
    // the accept kernel closes a row from the extended decode's partials and keeps the windows' stop state itself: both on
    // for every speculative call (a plain call without them gives the same tokens: DESIGN.md sections 4, 7)
    cfg.xc.on = true;
    cfg.stop.on = true;
    TxCfg dcfg = cfg;   // the draft: a greedy decode with its own masks and rules, nothing else
    dcfg.xc = XCfg();
    dcfg.stop = StopCfg();
    std::vector<int> b0, cg;
    const int n_groups = wm_spec_groups(call.B, sc.k, g_wm_tuning.spec_group, b0, cg);
    ctx->stage_ms[0] = ctx->stage_ms[1] = ctx->stage_ms[2] = 0.f;
    ActiveGuard active_guard(g_wm_active_decodes[ctx->device & 63]);
    for (int g = 0; g < n_groups; ++g) WM_TRY(spec_group(ctx, sc, call, cfg, dcfg, b0[g], cg[g]));
    return WM_OK;
}
}  // namespace

extern "C" int wm_transcribe_greedy(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, int B,
                                    const int32_t *prompt, int n_prompt, int max_new, int32_t eot,
                                    int32_t *tokens_out, int32_t *lens_out, wm_mem mem) try {
    TxCall call;
    call.src.pcm = pcm; call.src.pcm_dtype = pcm_dtype; call.mem = mem;
    call.prompts.prompt = prompt; call.n_prompt = n_prompt;
    outputs(call, B, max_new, eot, nullptr, tokens_out, lens_out, nullptr, nullptr);
    call.greedy_entry = true;
    return tx_transcribe(ctx, call);
} WM_API_CATCH

extern "C" int wm_transcribe(wm_ctx *ctx, const void *pcm, wm_dtype pcm_dtype, int B, const int32_t *prompt, int n_prompt,
                             int max_new, int32_t eot, const wm_decode_opts *opts, int32_t *tokens_out, int32_t *lens_out,
                             float *token_logprobs_out, float *no_speech_prob_out, wm_mem mem) try {
    TxCall call;
    call.src.pcm = pcm; call.src.pcm_dtype = pcm_dtype; call.mem = mem;
    call.prompts.prompt = prompt; call.n_prompt = n_prompt;
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

extern "C" int wm_transcribe_mel(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                 const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts, int n_prompt,
                                 const uint32_t *sample_ids, int max_new, int32_t eot, const wm_decode_opts *opts,
                                 int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out, float *no_speech_prob_out,
                                 wm_mem mem) try {
    TxCall call;
    call.entry = TxCall::MEL;
    mel_src(call, mel, mel_base, mel_len, seek, n_frames, mem);
    call.prompts = {prompts, n_prompt, nullptr, 0, sample_ids};
    call.n_prompt = n_prompt;
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

// wm_transcribe_mel with prompts of different lengths: every decode group right-aligns its rows to its own longest prompt
// (wm_right_align, WmModel::doff); a row's results are those of wm_transcribe_mel on that row alone with its own prompt
extern "C" int wm_transcribe_mel_ragged(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                        const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts,
                                        int prompt_stride, const int32_t *prompt_len, int sot_tail, const uint32_t *sample_ids,
                                        int max_new, int32_t eot, const wm_decode_opts *opts, int32_t *tokens_out,
                                        int32_t *lens_out, float *token_logprobs_out, float *no_speech_prob_out,
                                        wm_mem mem) try {
    TxCall call;
    call.entry = TxCall::RAGGED;
    mel_src(call, mel, mel_base, mel_len, seek, n_frames, mem);
    call.prompts = {prompts, prompt_stride, prompt_len, sot_tail, sample_ids};
    call.n_prompt = prompt_stride;
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

extern "C" int wm_transcribe_mel_best_of(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                         const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts,
                                         int prompt_stride, const int32_t *prompt_len, int sot_tail, const uint32_t *sample_ids,
                                         int best_of_n, float length_penalty, int max_new, int32_t eot, const wm_decode_opts *opts,
                                         int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out,
                                         float *no_speech_prob_out, int32_t *best_out, wm_mem mem) try {
    TxCall call;
    mel_src(call, mel, mel_base, mel_len, seek, n_frames, mem);
    best_of(call, prompts, prompt_stride, prompt_len, sot_tail, sample_ids, best_of_n, length_penalty, best_out);
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

// wm_transcribe_mel_best_of over the windows of an encoded set: the same call, its cross-K/V copied instead of computed
extern "C" int wm_transcribe_windows(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B, const int32_t *prompts,
                                     int prompt_stride, const int32_t *prompt_len, int sot_tail, const uint32_t *sample_ids,
                                     int best_of_n, float length_penalty, int max_new, int32_t eot, const wm_decode_opts *opts,
                                     int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out,
                                     float *no_speech_prob_out, int32_t *best_out) try {
    TxCall call;
    set_src(call, w, rows);
    best_of(call, prompts, prompt_stride, prompt_len, sot_tail, sample_ids, best_of_n, length_penalty, best_out);
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

extern "C" int wm_transcribe_mel_beam(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                      const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts,
                                      int prompt_stride, const int32_t *prompt_len, int sot_tail, int beam_size, int max_candidates,
                                      float length_penalty, int max_new, int32_t eot, const wm_decode_opts *opts,
                                      int32_t *tokens_out, int32_t *lens_out, int32_t *n_hyp_out, float *sum_logprobs_out,
                                      float *token_logprobs_out, float *no_speech_prob_out, int32_t *best_out, wm_mem mem) try {
    TxCall call;
    mel_src(call, mel, mel_base, mel_len, seek, n_frames, mem);
    beam(call, prompts, prompt_stride, prompt_len, sot_tail, beam_size, max_candidates, length_penalty, n_hyp_out,
         sum_logprobs_out, best_out);
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

extern "C" int wm_transcribe_windows_beam(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B, const int32_t *prompts,
                                          int prompt_stride, const int32_t *prompt_len, int sot_tail, int beam_size,
                                          int max_candidates, float length_penalty, int max_new, int32_t eot,
                                          const wm_decode_opts *opts, int32_t *tokens_out, int32_t *lens_out, int32_t *n_hyp_out,
                                          float *sum_logprobs_out, float *token_logprobs_out, float *no_speech_prob_out,
                                          int32_t *best_out) try {
    TxCall call;
    set_src(call, w, rows);
    beam(call, prompts, prompt_stride, prompt_len, sot_tail, beam_size, max_candidates, length_penalty, n_hyp_out,
         sum_logprobs_out, best_out);
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

// wm_transcribe_mel_ragged (prompt_len null: wm_transcribe_mel) whose decode keeps the alignment heads' cross-attention queries:
// the same tokens, plus the start frame of every generated token (lane_align)
extern "C" int wm_transcribe_mel_aligned(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                         const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts,
                                         int prompt_stride, const int32_t *prompt_len, int sot_tail, const uint32_t *sample_ids,
                                         int max_new, int32_t eot, const wm_decode_opts *opts, int medfilt_width, float qk_scale,
                                         int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out,
                                         float *no_speech_prob_out, int32_t *start_frame_out, wm_mem mem) try {
    TxCall call;
    call.entry = prompt_len ? TxCall::RAGGED : TxCall::MEL;
    mel_src(call, mel, mel_base, mel_len, seek, n_frames, mem);
    call.prompts = {prompts, prompt_stride, prompt_len, prompt_len ? sot_tail : 0, sample_ids};
    call.n_prompt = prompt_stride;
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    aligned(call, medfilt_width, qk_scale, start_frame_out);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

// ... over the windows of an encoded set (wm_transcribe_windows with one sample per row)
extern "C" int wm_transcribe_windows_aligned(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B, const int32_t *prompts,
                                             int prompt_stride, const int32_t *prompt_len, int sot_tail, const uint32_t *sample_ids,
                                             int max_new, int32_t eot, const wm_decode_opts *opts, int medfilt_width,
                                             float qk_scale, int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out,
                                             float *no_speech_prob_out, int32_t *start_frame_out) try {
    TxCall call;
    set_src(call, w, rows);
    best_of(call, prompts, prompt_stride, prompt_len, sot_tail, sample_ids, 1, NAN, nullptr);
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    aligned(call, medfilt_width, qk_scale, start_frame_out);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

// The best-of and beam calls whose decode keeps the alignment heads' queries of every candidate / beam: the same outputs, plus
// the start frames of the ONE hypothesis best_out names (lane_align)
extern "C" int wm_transcribe_mel_best_of_aligned(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                                 const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts,
                                                 int prompt_stride, const int32_t *prompt_len, int sot_tail,
                                                 const uint32_t *sample_ids, int best_of_n, float length_penalty, int max_new,
                                                 int32_t eot, const wm_decode_opts *opts, int medfilt_width, float qk_scale,
                                                 int32_t *tokens_out, int32_t *lens_out, float *token_logprobs_out,
                                                 float *no_speech_prob_out, int32_t *best_out, int32_t *start_frame_out,
                                                 wm_mem mem) try {
    TxCall call;
    mel_src(call, mel, mel_base, mel_len, seek, n_frames, mem);
    best_of(call, prompts, prompt_stride, prompt_len, sot_tail, sample_ids, best_of_n, length_penalty, best_out);
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    aligned(call, medfilt_width, qk_scale, start_frame_out, true);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

extern "C" int wm_transcribe_windows_best_of_aligned(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B,
                                                     const int32_t *prompts, int prompt_stride, const int32_t *prompt_len,
                                                     int sot_tail, const uint32_t *sample_ids, int best_of_n, float length_penalty,
                                                     int max_new, int32_t eot, const wm_decode_opts *opts, int medfilt_width,
                                                     float qk_scale, int32_t *tokens_out, int32_t *lens_out,
                                                     float *token_logprobs_out, float *no_speech_prob_out, int32_t *best_out,
                                                     int32_t *start_frame_out) try {
    TxCall call;
    set_src(call, w, rows);
    best_of(call, prompts, prompt_stride, prompt_len, sot_tail, sample_ids, best_of_n, length_penalty, best_out);
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    aligned(call, medfilt_width, qk_scale, start_frame_out, true);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

extern "C" int wm_transcribe_mel_beam_aligned(wm_ctx *ctx, const float *mel, const int64_t *mel_base, const int32_t *mel_len,
                                              const int32_t *seek, const int32_t *n_frames, int B, const int32_t *prompts,
                                              int prompt_stride, const int32_t *prompt_len, int sot_tail, int beam_size,
                                              int max_candidates, float length_penalty, int max_new, int32_t eot,
                                              const wm_decode_opts *opts, int medfilt_width, float qk_scale, int32_t *tokens_out,
                                              int32_t *lens_out, int32_t *n_hyp_out, float *sum_logprobs_out,
                                              float *token_logprobs_out, float *no_speech_prob_out, int32_t *best_out,
                                              int32_t *start_frame_out, wm_mem mem) try {
    TxCall call;
    mel_src(call, mel, mel_base, mel_len, seek, n_frames, mem);
    beam(call, prompts, prompt_stride, prompt_len, sot_tail, beam_size, max_candidates, length_penalty, n_hyp_out,
         sum_logprobs_out, best_out);
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    aligned(call, medfilt_width, qk_scale, start_frame_out, true);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

extern "C" int wm_transcribe_windows_beam_aligned(wm_ctx *ctx, const wm_windows *w, const int32_t *rows, int B,
                                                  const int32_t *prompts, int prompt_stride, const int32_t *prompt_len, int sot_tail,
                                                  int beam_size, int max_candidates, float length_penalty, int max_new, int32_t eot,
                                                  const wm_decode_opts *opts, int medfilt_width, float qk_scale, int32_t *tokens_out,
                                                  int32_t *lens_out, int32_t *n_hyp_out, float *sum_logprobs_out,
                                                  float *token_logprobs_out, float *no_speech_prob_out, int32_t *best_out,
                                                  int32_t *start_frame_out) try {
    TxCall call;
    set_src(call, w, rows);
    beam(call, prompts, prompt_stride, prompt_len, sot_tail, beam_size, max_candidates, length_penalty, n_hyp_out,
         sum_logprobs_out, best_out);
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    aligned(call, medfilt_width, qk_scale, start_frame_out, true);
    return tx_transcribe(ctx, call);
} WM_API_CATCH

// wm_transcribe_mel whose tokens a draft model proposes and panels of the target verify: the same outputs, bit for bit
extern "C" int wm_transcribe_mel_speculative(wm_ctx *ctx, wm_ctx *draft, const float *mel, const int64_t *mel_base,
                                             const int32_t *mel_len, const int32_t *seek, const int32_t *n_frames, int B,
                                             const int32_t *prompts, int n_prompt, int draft_len, int max_new, int32_t eot,
                                             const wm_decode_opts *opts, int32_t *tokens_out, int32_t *lens_out,
                                             float *token_logprobs_out, float *no_speech_prob_out, wm_spec_stats *stats_out,
                                             wm_mem mem) try {
    TxCall call;
    call.entry = TxCall::MEL; call.speculative = true;
    mel_src(call, mel, mel_base, mel_len, seek, n_frames, mem);
    call.prompts = {prompts, n_prompt, nullptr, 0, nullptr};
    call.n_prompt = n_prompt;
    outputs(call, B, max_new, eot, opts, tokens_out, lens_out, token_logprobs_out, no_speech_prob_out);
    SpecCall sc;
    sc.draft = draft; sc.k = draft_len; sc.stats = stats_out;
    return tx_speculative(ctx, sc, call);
} WM_API_CATCH
