// debug_hooks.cpp -- the wmdbg_* test / micro-benchmark hooks of include/whisper_mi355x_debug.h.
// NOT linked into libwhisper_mi355x.so: build.py links this translation unit, together with the product's objects, into
// libwhisper_mi355x_dbg.so, which only tests/ and tools/ load (kernel-level parity tests against the oracle, probes).
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/whisper_mi355x_debug.h"
#include "beam.h"
#include "model.h"
#include "tx_plan.h"

// ---------------------------------------------------------------- staging, timing and capture: what every hook below goes through
// The only place in this file that allocates or frees device memory, creates or destroys events, streams and graphs, or begins
// and ends a stream capture.  A hook that fails half-way hands back everything it took and leaves the context's stream usable.
namespace {
// Device allocations of one hook call, freed when the hook returns (on an error path too).  Lifetime rule: the pool is
// declared AFTER every host buffer it uploads from or downloads into, so that its hipFree (which waits for the device) runs
// before those buffers die.
struct DevPool {
    std::vector<void *> v;
    DevPool() = default;
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    ~DevPool() {
        for (void *p : v) (void)hipFree(p);
    }
    // bytes of `fill` (a byte value), then the host data when given.  The 512 bytes of slack are a guard band behind
    // host-staged buffers; nothing relies on them: every kernel read of these buffers is clamped to the group's rows and the
    // matrix's tiles (gemv_unit_load), and each buffer is sized for what its kernel may write.
    template <class T>
    int get(T **d, const void *h, size_t bytes, hipStream_t s, int fill = 0) {
        void *p = nullptr;
        WM_HIP(hipMalloc(&p, bytes + 512));
        v.push_back(p);
        *d = static_cast<T *>(p);
        WM_HIP(hipMemsetAsync(p, fill, bytes + 512, s));
        if (h) WM_HIP(hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, s));
        return WM_OK;
    }
};

// ---- bf16 (round to nearest even) and the WL_TILED order
bf16_t f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}
void to_bf16(const float *in, std::vector<bf16_t> &out, size_t n) {
    out.resize(n);
    for (size_t i = 0; i < n; ++i) out[i] = f2bf(in[i]);
}
void from_bf16(const std::vector<bf16_t> &in, float *out) {
    for (size_t i = 0; i < in.size(); ++i) {
        uint32_t u = (uint32_t)in[i] << 16;
        memcpy(&out[i], &u, 4);
    }
}
// [rows][K] f32 -> bf16 in WL_TILED order, rows padded to 16 with zeros
void tile_bf16(const float *m, size_t rows, size_t K, std::vector<bf16_t> &out) {
    const size_t rpad = (rows + 15) / 16 * 16;
    std::vector<float> t(rpad * K, 0.f);
    for (size_t r = 0; r < rows; ++r)
        for (size_t k = 0; k < K; ++k) t[wm_tiled_offset(r, k, K)] = m[r * K + k];
    to_bf16(t.data(), out, t.size());
}
// WL_TILED bf16 [rows][K] -> row-major f32
void untile_bf16(const std::vector<bf16_t> &t, size_t rows, size_t K, float *out) {
    std::vector<bf16_t> lin(rows * K);
    for (size_t r = 0; r < rows; ++r)
        for (size_t k = 0; k < K; ++k) lin[r * K + k] = t[wm_tiled_offset(r, k, K)];
    from_bf16(lin, out);
}
void fill_bf16(std::vector<bf16_t> &v, size_t n) { v.assign(n, (bf16_t)WMDBG_SENTINEL_BF16); }
void fill_f32(std::vector<float> &v, size_t n) {
    const uint32_t u = WMDBG_SENTINEL_F32;
    float f;
    memcpy(&f, &u, 4);
    v.assign(n, f);
}
// device bf16 -> host f32 (widened); synchronous: the stream has drained when it returns
int down_bf16(const void *d, size_t n, float *out, hipStream_t s) {
    std::vector<bf16_t> t(n);
    WM_HIP(hipMemcpyAsync(t.data(), d, n * 2, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    from_bf16(t, out);
    return WM_OK;
}
// device WL_TILED bf16 [rows padded to 16][K] -> host row-major f32 [rows][K]; synchronous.  The attention kernels store their
// head outputs [B][H * 64] this way: the out-projection's tiled A-operand order.
int down_tiled_bf16(const bf16_t *d, size_t rows, size_t K, float *out, hipStream_t s) {
    std::vector<bf16_t> t((rows + 15) / 16 * 16 * K);
    WM_HIP(hipMemcpyAsync(t.data(), d, t.size() * 2, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    untile_bf16(t, rows, K, out);
    return WM_OK;
}

// ---- The decoder's partial row statistics of a [B][K] f32 matrix: per 16-row block (stride 2 K floats) K / 16 parts (part p =
// columns 16 p .. 16 p + 15) of [16 rows][2] = (sum, sum of squares).  The tests compare these on bits: per row, k ascends
// into its part's slot, and the parts ascend when they are summed.
size_t stat_at(int K, size_t b, int part, int c) { return (b >> 4) * (size_t)(2 * K) + ((size_t)part * 16 + (b & 15)) * 2 + c; }
void stats_pack(const float *x, int B, int K, std::vector<float> &st) {
    st.assign((size_t)((B + 15) / 16) * 2 * K, 0.f);
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < K; ++k) {
            const float v = x[(size_t)b * K + k];
            st[stat_at(K, b, k >> 4, 0)] += v;
            st[stat_at(K, b, k >> 4, 1)] += v * v;
        }
}
// (sum, sum of squares) of row b to out2
void stats_sum(const float *st, int K, int b, float *out2) {
    float s1 = 0.f, s2 = 0.f;
    for (int part = 0; part < K / 16; ++part) {
        s1 += st[stat_at(K, b, part, 0)];
        s2 += st[stat_at(K, b, part, 1)];
    }
    out2[0] = s1;
    out2[1] = s2;
}

// The A operand of a LayerNorm-folded GEMV as the decoder holds it: the producer's partial statistics of the raw f32 rows,
// the rows' f32 means, and the bf16 activations in WL_TILED order -- of x - mean when `centre`, else of x (the means are then
// not handed to the kernel).
void stage_ln_rows(const float *x, int B, int K, bool centre, std::vector<bf16_t> &x16, std::vector<float> &st, std::vector<float> &mean) {
    stats_pack(x, B, K, st);
    mean.assign((size_t)B, 0.f);
    std::vector<float> xc((size_t)B * K);
    for (int b = 0; b < B; ++b) {
        float s1 = 0.f;
        for (int k = 0; k < K; ++k) s1 += x[(size_t)b * K + k];
        mean[b] = s1 / (float)K;
        for (int k = 0; k < K; ++k) xc[(size_t)b * K + k] = centre ? x[(size_t)b * K + k] - mean[b] : x[(size_t)b * K + k];
    }
    tile_bf16(xc.data(), (size_t)B, (size_t)K, x16);
}

// ---- timing and capture
// The two events of a timed region, destroyed with the object.
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    int init() {
        WM_HIP(hipEventCreate(&e0));
        WM_HIP(hipEventCreate(&e1));
        return WM_OK;
    }
    int start(hipStream_t s) {
        WM_HIP(hipEventRecord(e0, s));
        return WM_OK;
    }
    // microseconds since start(), once the stream has drained
    int stop_us(hipStream_t s, float *us) {
        WM_HIP(hipEventRecord(e1, s));
        WM_HIP(hipStreamSynchronize(s));
        float ms = 0.f;
        WM_HIP(hipEventElapsedTime(&ms, e0, e1));
        *us = ms * 1e3f;
        return WM_OK;
    }
};

// One captured launch chain of a stream.  A capture it began is always ended -- on an error path too, where the graph is
// discarded -- so the stream stays usable; the graph and its exec are destroyed with the object.
struct GraphRun {
    hipStream_t s;
    bool capturing = false;
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    explicit GraphRun(hipStream_t s_) : s(s_) {}
    GraphRun(const GraphRun &) = delete;
    GraphRun &operator=(const GraphRun &) = delete;
    ~GraphRun() {
        if (capturing) (void)hipStreamEndCapture(s, &g);
        if (ge) (void)hipGraphExecDestroy(ge);
        if (g) (void)hipGraphDestroy(g);
    }
    int begin() {
        WM_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        capturing = true;
        return WM_OK;
    }
    int end() {
        capturing = false;   // a failed end has ended the capture too
        WM_HIP(hipStreamEndCapture(s, &g));
        WM_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        return WM_OK;
    }
    // one warm replay, then the timed one: microseconds of a whole replay
    int replay_us(EventPair &ev, float *us) {
        WM_HIP(hipGraphLaunch(ge, s));
        WM_HIP(hipStreamSynchronize(s));
        WM_TRY(ev.start(s));
        WM_HIP(hipGraphLaunch(ge, s));
        return ev.stop_us(s, us);
    }
};

// A second stream that a capturing stream forks to and joins from: a parallel branch of the captured graph.  Declared before
// the GraphRun whose capture it joins, so that the capture has ended when the stream is destroyed.
struct SideBranch {
    hipStream_t s2 = nullptr;
    hipEvent_t ef = nullptr, ej = nullptr;
    SideBranch() = default;
    SideBranch(const SideBranch &) = delete;
    SideBranch &operator=(const SideBranch &) = delete;
    ~SideBranch() {
        if (ef) (void)hipEventDestroy(ef);
        if (ej) (void)hipEventDestroy(ej);
        if (s2) (void)hipStreamDestroy(s2);
    }
    int init() {
        WM_HIP(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
        WM_HIP(hipEventCreateWithFlags(&ef, hipEventDisableTiming));
        WM_HIP(hipEventCreateWithFlags(&ej, hipEventDisableTiming));
        return WM_OK;
    }
    int fork(hipStream_t s) {
        WM_HIP(hipEventRecord(ef, s));
        WM_HIP(hipStreamWaitEvent(s2, ef, 0));
        return WM_OK;
    }
    int join(hipStream_t s) {
        WM_HIP(hipEventRecord(ej, s2));
        WM_HIP(hipStreamWaitEvent(s, ej, 0));
        return WM_OK;
    }
};
}  // namespace

// ---------------------------------------------------------------- host-only test hooks
int wm_gemm_set_tile_override(int tile);
extern "C" int wmdbg_set_gemm_tile(int tile) { return wm_gemm_set_tile_override(tile); }

// The launch-shape experiment knobs (wm_tuning.h WmTuning): by name, so that tools/ scripts need no struct mirror.
extern "C" int wmdbg_set_tuning(const char *key, int value) {
    WM_REQUIRE(key, WM_ERR_INVALID, "wmdbg_set_tuning: null key");
    struct { const char *name; int *field; } table[] = {
        {"gemv_tn", &g_wm_tuning.gemv_tn}, {"gemv_nblk", &g_wm_tuning.gemv_nblk}, {"gemv_no_ppw2", &g_wm_tuning.gemv_no_ppw2}, {"gemv_ppw2_nblk", &g_wm_tuning.gemv_ppw2_nblk},
        {"prefetch_max_b", &g_wm_tuning.prefetch_max_b}, {"xattn_split_below", &g_wm_tuning.xattn_split_below},
        {"xattn_wgs", &g_wm_tuning.xattn_wgs}, {"xattn_no_flat", &g_wm_tuning.xattn_no_flat},
        {"xattn_lds_pad", &g_wm_tuning.xattn_lds_pad}, {"xattn_splits", &g_wm_tuning.xattn_splits},
        {"gemm_tile", &g_wm_tuning.gemm_tile}, {"gemm128_pipe", &g_wm_tuning.gemm128_pipe}, {"gemm_gm", &g_wm_tuning.gemm_gm}, {"no_early_stop", &g_wm_tuning.no_early_stop},
        {"xattn_no_deep", &g_wm_tuning.xattn_no_deep}, {"xattn_never_short", &g_wm_tuning.xattn_never_short},         {"logits_tn", &g_wm_tuning.logits_tn}, {"enc_attn_mfma_sum", &g_wm_tuning.enc_attn_mfma_sum},
        {"group_chunks", &g_wm_tuning.group_chunks}, {"argmax_rows_per_wg", &g_wm_tuning.argmax_rows_per_wg}, {"xattn_fuse_q", &g_wm_tuning.xattn_fuse_q},
        {"teacher_panel_cut", &g_wm_tuning.teacher_panel_cut}, {"lane_parts", &g_wm_tuning.lane_parts}, {"lane_solo_cus", &g_wm_tuning.lane_solo_cus}, {"spec_group", &g_wm_tuning.spec_group}, {"frontend_per_wave_twiddles", &g_wm_tuning.frontend_per_wave_twiddles},
    };
    if (strcmp(key, "reset") == 0) { g_wm_tuning = WmTuning(); return WM_OK; }
    for (auto &e : table)
        if (strcmp(key, e.name) == 0) { *e.field = value; return WM_OK; }
    wm_set_error("wmdbg_set_tuning: unknown key '%s'", key);
    return WM_ERR_INVALID;
}

extern "C" int wmdbg_group_count(int B, int lanes, int explicit_lanes) { return wm_group_count(B, lanes, explicit_lanes != 0, 0); }
extern "C" int wmdbg_cand_groups(int B, int N, int lanes, int explicit_lanes, int32_t *b0_out, int32_t *cg_out) {
    if (B < 1 || N < 1 || N > WM_MAX_BEST_OF || !b0_out || !cg_out) return -1;
    std::vector<int> b0, cg;
    const int G = wm_cand_groups(B, N, lanes, explicit_lanes != 0, b0, cg);
    for (int g = 0; g < G; ++g) { b0_out[g] = b0[g]; cg_out[g] = cg[g]; }
    return G;
}
extern "C" int wmdbg_dec_attn_plan(const int32_t *in, int n, int32_t *out) {
    if (!in || !out || n < 0) return -1;
    for (int i = 0; i < n; ++i) wm_attn_plan_flat(in + (size_t)i * WM_ATTN_PLAN_IN, g_wm_tuning, out + (size_t)i * WM_ATTN_PLAN_OUT);
    return n;
}
extern "C" int wmdbg_dec_gemv_plan(const int32_t *in, int n, int32_t *out) {
    if (!in || !out || n < 0) return -1;
    for (int i = 0; i < n; ++i) wm_gemv_plan_flat(in + (size_t)i * WM_GEMV_PLAN_IN, g_wm_tuning, out + (size_t)i * WM_GEMV_PLAN_OUT);
    return n;
}
extern "C" int wmdbg_tx_plan(const int32_t *in, int n, int32_t *out, int32_t *cut, int cut_cap) {
    if (!in || !out || !cut || n < 0 || cut_cap < 0) return -1;
    int used = 0;
    for (int i = 0; i < n; ++i) {
        int32_t *o = out + (size_t)i * WM_TX_PLAN_OUT;
        const int k = wm_tx_plan_flat(in + (size_t)i * WM_TX_PLAN_IN, o, cut + used, cut_cap - used);
        if (k < 0) return -1;
        o[5] = used;
        used += k;
    }
    return n;
}
extern "C" int wmdbg_tx_plan_bounded(const int32_t *in, const int32_t *max_group_rows, int n, int32_t *out, int32_t *cut, int cut_cap) {
    if (!in || !max_group_rows || !out || !cut || n < 0 || cut_cap < 0) return -1;
    int used = 0;
    for (int i = 0; i < n; ++i) {
        int32_t *o = out + (size_t)i * WM_TX_PLAN_OUT;
        const int k = wm_tx_plan_flat(in + (size_t)i * WM_TX_PLAN_IN, o, cut + used, cut_cap - used, max_group_rows[i]);
        if (k < 0) return -1;
        o[5] = used;
        used += k;
    }
    return n;
}
extern "C" int wmdbg_group_tables(const int32_t *in, int n, int32_t *out) {
    if (!in || !out || n < 0) return -1;
    for (int i = 0; i < n; ++i)
        if (!wm_group_tables_flat(in + (size_t)i * WM_TX_TAB_IN, WM_XIDS_CAND, out + (size_t)i * WM_TX_TAB_OUT)) return -1;
    return n;
}
// ---- speculative decoding (tx_plan.h): the group cut, the width rule and a round's arithmetic, case by case
extern "C" int wmdbg_spec_groups(int B, int k, int spec_group, int32_t *b0_out, int32_t *cg_out) {
    if (B < 1 || k < 1 || k > WM_MAX_DRAFT_LEN || !b0_out || !cg_out) return -1;
    std::vector<int> b0, cg;
    const int G = wm_spec_groups(B, k, spec_group, b0, cg);
    for (int g = 0; g < G; ++g) { b0_out[g] = b0[g]; cg_out[g] = cg[g]; }
    return G;
}
extern "C" int wmdbg_spec_width(int k, int bound, int last) { return wm_spec_width(k, bound, last); }
extern "C" int wmdbg_spec_round(int G, int w, const int32_t *accepted, const int32_t *live, const int32_t *eot_at, const int32_t *left,
                                int32_t *live_out, int32_t *inc_out) {
    if (G < 1 || w < 1 || !accepted || !live || !eot_at || !left || !live_out || !inc_out) return -1;
    return wm_spec_round(G, w, accepted, live, eot_at, left, live_out, inc_out);
}
// n cases of one shape at once: in i32 [n][4][G] = accepted | live | eot_at | left, out i32 [n][1 + 5 G] = n | live_out [G] | inc [G][4]
extern "C" int wmdbg_spec_round_batch(int n, int G, int w, const int32_t *in, int32_t *out) {
    if (n < 0 || G < 1 || w < 1 || !in || !out) return -1;
    for (int i = 0; i < n; ++i) {
        const int32_t *c = in + (size_t)i * 4 * G;
        int32_t *o = out + (size_t)i * (1 + 5 * G);
        o[0] = wm_spec_round(G, w, c, c + G, c + 2 * G, c + 3 * G, o + 1, o + 1 + G);
    }
    return n;
}
// tx_pending.h on the CPU (documented at include/whisper_mi355x_debug.h): who serves which pending item, and take()
extern "C" int wmdbg_pending_refusal(unsigned pending, int entry, unsigned flags, int n_cand, char *msg_out, int msg_cap) {
    if (entry < WmCallKind::PLAIN || entry > WmCallKind::BEAM || !msg_out || msg_cap < 1) return -1;
    WmCallKind k;
    k.entry = (WmCallKind::Entry)entry; k.n_cand = n_cand; k.greedy_entry = flags & 1; k.beam = flags & 2; k.windows = flags & 4;
    k.hyp = flags & 8; k.speculative = flags & 16; k.multi = flags & 32; k.f32_path = flags & 64;
    const char *no = wm_pending_refusal(pending, k);
    snprintf(msg_out, (size_t)msg_cap, "%s", no ? no : "");
    return no ? WM_ERR_STATE : WM_OK;
}
extern "C" int wmdbg_pending_take(unsigned bits, unsigned again, int32_t *out) {
    if (!out) return -1;
    auto arm = [](WmPending &p, unsigned b, int v) {   // every list one entry of v
        if (b & WM_PEND_BUDGETS) p.budgets.assign(1, v);
        if (b & WM_PEND_BIAS_ROWS) p.bias_rows.assign(1, v);
        if (b & WM_PEND_CST_ROWS) p.cst_rows.assign(1, v);
        if (b & WM_PEND_SAMP_ROWS) { p.samp_T.assign(1, (float)v); p.samp_seed.assign(1, (uint64_t)v); }
        if (b & WM_PEND_ALT) { p.alt_on = true; p.alt.n = v; }
        if (b & WM_PEND_GIVEN) { p.given_lens.assign(1, v); p.given_tok.assign(1, v); p.given_stride = 1; }
    };
    WmPending member;
    arm(member, bits, 1);
    out[0] = (int32_t)member.bits();
    const WmPending taken = member.take();   // (out[0]: before it; [1], [2]: what it returned and what it left)
    out[1] = (int32_t)taken.bits(); out[2] = (int32_t)member.bits();
    arm(member, again, 2);   // (the taken value is its own: it does not see this)
    out[3] = (int32_t)taken.bits(); out[4] = (int32_t)member.bits(); out[5] = taken.budgets.empty() ? 0 : taken.budgets[0];
    return 0;
}
// Scoped to the NEXT transcribe call on ctx, which takes it whatever its outcome; wm_transcribe_mel_speculative reads it: the proposal
// for generated index i of row b of that call is tokens[b * max_new + i].  `tokens` is host memory that lives until the call returns.
extern "C" int wmdbg_spec_script(wm_ctx *ctx, const int32_t *tokens, int B, int max_new) {
    WM_REQUIRE(ctx && ctx->model, WM_ERR_STATE, "wmdbg_spec_script: context has no model");
    WmModel *m = ctx->model;
    WmDebugShots &d = m->pending.dbg;
    d.spec_script = nullptr; d.spec_script_new = d.spec_script_rows = 0;
    if (!tokens) return WM_OK;
    WM_REQUIRE(B >= 1 && max_new >= 1, WM_ERR_INVALID, "wmdbg_spec_script: B < 1 or max_new < 1");
    for (size_t i = 0; i < (size_t)B * max_new; ++i)
        WM_REQUIRE(tokens[i] >= 0 && tokens[i] < m->dims.n_vocab, WM_ERR_INVALID, "wmdbg_spec_script: token %d outside the vocabulary", tokens[i]);
    d.spec_script = tokens; d.spec_script_new = max_new; d.spec_script_rows = B;
    return WM_OK;
}
// The accept + commit launches of a speculative round alone (spec.hip), timestamp rules off: a group of G windows x w rows at
// position pos, staged from the per-tile partials a verify step's logits launch would have left.
extern "C" int wmdbg_spec_accept(wm_ctx *ctx, int G, int w, int n_tiles, int pos, int n_prompt, int n_ctx, int max_new, int32_t eot,
                                 const int32_t *budget, const uint64_t *tilemax, const float *txt, const float *win, int32_t *seq,
                                 int32_t *done, float *logprob_out, int32_t *stats_out, int32_t *round_out, int32_t *acc_out,
                                 int32_t *draft_seq_out, int32_t *pos_out) {
    WM_REQUIRE(ctx && tilemax && txt && win && seq && done && logprob_out && stats_out && round_out && acc_out && draft_seq_out && pos_out,
               WM_ERR_INVALID, "wmdbg_spec_accept: null pointer");
    WM_TRY(wm_panel_shape_check(G, w, "wmdbg_spec_accept"));
    WM_REQUIRE(n_tiles >= 1 && n_prompt >= 1 && max_new >= 1 &&
                   pos >= n_prompt && pos + w < n_ctx && pos + w <= n_prompt + max_new - 1 && n_ctx <= 4096,
               WM_ERR_INVALID, "wmdbg_spec_accept: bad geometry");
    for (int i = 0; i < G * w; ++i)
        for (int t = 0; t < n_tiles; ++t) {
            const uint64_t k = tilemax[(size_t)i * n_tiles + t];
            WM_REQUIRE(k == 0 || (int)((0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)) >> 4) < n_tiles, WM_ERR_INVALID,
                       "wmdbg_spec_accept: a key names an id outside the tiles");
        }
    hipStream_t s = ctx->stream;
    const size_t rows = (size_t)G * w, nt = rows * n_tiles, ns = (size_t)n_ctx * G;
    std::vector<int32_t> zeros((size_t)WM_DEC_MAXB * 4, 0);
    DevPool pool;
    unsigned long long *d_tm;
    float *d_txt, *d_win, *d_lp, *d_wlp;
    int *d_seq, *d_dseq, *d_done, *d_bud = nullptr, *d_pos, *d_wtok, *d_acc, *d_stats, *d_round, *d_nlive;
    WmXPar *d_par;
    WM_TRY(pool.get(&d_tm, tilemax, nt * 8, s));
    WM_TRY(pool.get(&d_txt, txt, nt * 8, s));
    WM_TRY(pool.get(&d_win, win, nt * 8, s));
    WM_TRY(pool.get(&d_lp, nullptr, (size_t)max_new * G * 4, s));
    WM_TRY(pool.get(&d_wlp, nullptr, rows * 4, s));
    WM_TRY(pool.get(&d_seq, seq, ns * 4, s));
    WM_TRY(pool.get(&d_dseq, nullptr, ns * 4, s));
    WM_TRY(pool.get(&d_done, done, (size_t)G * 4, s));
    if (budget) WM_TRY(pool.get(&d_bud, budget, (size_t)G * 4, s));
    const int pos2[2] = {pos, pos + w};   // (the draft has taken its w steps)
    WM_TRY(pool.get(&d_pos, pos2, 8, s));
    WM_TRY(pool.get(&d_wtok, nullptr, rows * 4, s));
    WM_TRY(pool.get(&d_acc, nullptr, (size_t)G * 4, s));
    WM_TRY(pool.get(&d_stats, zeros.data(), (size_t)G * 16, s));
    WM_TRY(pool.get(&d_round, nullptr, 8, s));
    WM_TRY(pool.get(&d_nlive, nullptr, 4, s));
    WM_TRY(pool.get(&d_par, nullptr, sizeof(WmXPar), s));
    WmSpecDev sp;
    memset(&sp, 0, sizeof(sp));
    sp.tseq = d_seq; sp.dseq = d_dseq; sp.tpos = d_pos; sp.dpos = d_pos + 1;
    sp.wtok = d_wtok; sp.wlp = d_wlp; sp.acc = d_acc; sp.stats = d_stats; sp.round = d_round;
    sp.max_new = max_new; sp.n_vocab = n_tiles * 16;
    WmXDev xd;
    memset(&xd, 0, sizeof(xd));
    xd.par = d_par; xd.txt = d_txt; xd.win = d_win; xd.logprob = d_lp;
    WmStopDev st;
    memset(&st, 0, sizeof(st));
    st.done = d_done; st.budget = d_bud; st.n_live = d_nlive; st.eot = eot; st.pad_tok = eot >= 0 ? eot : 0;
    WM_TRY(wm_spec_accept(ctx, d_tm, n_tiles, sp, xd, st, G, w, n_prompt, n_ctx, 0));
    WM_HIP(hipMemcpyAsync(seq, d_seq, ns * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(draft_seq_out, d_dseq, ns * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(done, d_done, (size_t)G * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(logprob_out, d_lp, (size_t)max_new * G * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(stats_out, d_stats, (size_t)G * 16, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(round_out, d_round, 8, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(acc_out, d_acc, (size_t)G * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(pos_out, d_pos, 8, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}
extern "C" int wmdbg_spec_layout(int32_t *out4) {
    if (!out4) return WM_ERR_INVALID;
    out4[0] = (int32_t)sizeof(wmdbg_spec); out4[1] = (int32_t)offsetof(wmdbg_spec, tts_par);
    out4[2] = (int32_t)offsetof(wmdbg_spec, script); out4[3] = (int32_t)offsetof(wmdbg_spec, logprob);
    return WM_OK;
}
// The adoption, the staging or the commit of a speculative round alone (spec.hip) on the caller's state.  Every buffer goes to
// the device whole and comes back whole, so the caller's sentinels show what the kernel left alone.
extern "C" int wmdbg_spec_kernel(wm_ctx *ctx, wmdbg_spec *io) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(io && io->tseq && io->dseq && io->pos2 && io->tts_hist && io->tts_rng && io->dts_hist && io->dts_rng && io->chist &&
                   io->crng && io->dchist && io->dcrng && io->wtok && io->wlp && io->acc && io->done && io->stats && io->round &&
                   io->n_live && io->logprob,
               WM_ERR_INVALID, "wmdbg_spec_kernel: null pointer");
    const int G = io->G, w = io->w, cap = io->cap, n_ctx = io->n_ctx, n_prompt = io->n_prompt, max_new = io->max_new, pos = io->pos2[0];
    WM_REQUIRE(io->which >= 0 && io->which <= 2, WM_ERR_INVALID, "wmdbg_spec_kernel: which %d is not 0 .. 2", io->which);
    WM_TRY(wm_panel_shape_check(G, w, "wmdbg_spec_kernel"));
    WM_REQUIRE(cap >= G && cap <= 2 * WM_DEC_MAXB &&
                   n_prompt >= 1 && n_prompt < n_ctx && n_ctx <= 4096 && max_new >= 1 && max_new <= 4096 && io->n_vocab >= 1,
               WM_ERR_INVALID, "wmdbg_spec_kernel: bad geometry");
    // the positions a kernel addresses the token buffers with: the staging stops at n_ctx by itself, the commit relies on its
    // launcher (the host narrows the last rounds); its reads of wtok go up to row acc[c].  pos = n_prompt - 1: a round whose first
    // token is generated index 0 (the product's first round stands one further: the first token is a plain step's)
    if (io->which == 1) WM_REQUIRE(pos >= n_prompt - 1 && pos < n_ctx, WM_ERR_INVALID, "wmdbg_spec_kernel: position %d outside [n_prompt - 1, n_ctx)", pos);
    if (io->which == 2) {
        WM_REQUIRE(pos >= n_prompt - 1 && pos + w < n_ctx, WM_ERR_INVALID, "wmdbg_spec_kernel: position %d + %d rows leaves the context", pos, w);
        for (int c = 0; c < G; ++c)
            WM_REQUIRE(io->acc[c] >= 0 && io->acc[c] < w, WM_ERR_INVALID, "wmdbg_spec_kernel: acc[%d] = %d outside [0, w)", c, io->acc[c]);
    }
    hipStream_t s = ctx->stream;
    const size_t ns = (size_t)n_ctx * G * 4, win4 = (size_t)cap * 16, rows = (size_t)cap * w;
    DevPool pool;
    // every buffer once: host pointer, bytes, device pointer
    struct Buf { void *h; size_t bytes; void *d; };
    Buf bufs[] = {{io->tseq, ns, nullptr},          {io->dseq, ns, nullptr},        {io->pos2, 8, nullptr},           {io->tts_hist, win4, nullptr},
                  {io->tts_rng, rows * 16, nullptr}, {io->dts_hist, win4, nullptr},  {io->dts_rng, win4, nullptr},     {io->chist, win4, nullptr},
                  {io->crng, win4, nullptr},        {io->dchist, win4, nullptr},    {io->dcrng, win4, nullptr},       {io->wtok, rows * 4, nullptr},
                  {io->wlp, rows * 4, nullptr},     {io->acc, (size_t)cap * 4, nullptr}, {io->done, (size_t)cap * 4, nullptr}, {io->stats, win4, nullptr},
                  {io->round, 8, nullptr},          {io->n_live, 4, nullptr},       {io->logprob, (size_t)max_new * G * 4, nullptr}};
    for (Buf &b : bufs) WM_TRY(pool.get(&b.d, b.h, b.bytes, s));
    int *d_script = nullptr, *d_bud = nullptr;
    if (io->script) WM_TRY(pool.get(&d_script, io->script, (size_t)G * max_new * 4, s));
    if (io->budget) WM_TRY(pool.get(&d_bud, io->budget, (size_t)cap * 4, s));
    auto dev = [&](const void *h) {
        for (const Buf &b : bufs)
            if (b.h == h) return b.d;
        return (void *)nullptr;
    };
    WmSpecDev sp;
    memset(&sp, 0, sizeof(sp));
    sp.tseq = (int *)dev(io->tseq); sp.dseq = (int *)dev(io->dseq);
    sp.tpos = (int *)dev(io->pos2); sp.dpos = sp.tpos + 1;
    sp.tts.rng = io->tts_on ? (int *)dev(io->tts_rng) : nullptr; sp.tts.hist = (int *)dev(io->tts_hist);
    sp.tts.ts_begin = io->tts_par[0]; sp.tts.eot = io->tts_par[1]; sp.tts.n_vocab = io->tts_par[2]; sp.tts.max_initial = io->tts_par[3];
    sp.dts.rng = io->dts_on ? (int *)dev(io->dts_rng) : nullptr; sp.dts.hist = (int *)dev(io->dts_hist);
    sp.dts.ts_begin = io->dts_par[0]; sp.dts.eot = io->dts_par[1]; sp.dts.n_vocab = io->dts_par[2]; sp.dts.max_initial = io->dts_par[3];
    sp.chist = (int *)dev(io->chist); sp.crng = (int *)dev(io->crng); sp.dchist = (int *)dev(io->dchist); sp.dcrng = (int *)dev(io->dcrng);
    sp.wtok = (int *)dev(io->wtok); sp.wlp = (float *)dev(io->wlp); sp.acc = (int *)dev(io->acc);
    sp.stats = (int *)dev(io->stats); sp.round = (int *)dev(io->round);
    sp.script = d_script; sp.max_new = max_new; sp.n_vocab = io->n_vocab;
    if (io->which == 0) {
        WM_TRY(wm_spec_adopt(ctx, sp, G, n_prompt));
    } else if (io->which == 1) {
        WM_TRY(wm_spec_stage(ctx, sp, G, w, n_prompt, n_ctx));
    } else {
        WmXDev xd;
        memset(&xd, 0, sizeof(xd));
        xd.logprob = (float *)dev(io->logprob);
        WmStopDev st;
        memset(&st, 0, sizeof(st));
        st.done = (int *)dev(io->done); st.budget = d_bud; st.n_live = (int *)dev(io->n_live); st.eot = io->eot; st.pad_tok = io->pad_tok;
        WM_TRY(wm_spec_commit(ctx, sp, xd, st, G, w, n_prompt, n_ctx));
    }
    for (const Buf &b : bufs) WM_HIP(hipMemcpyAsync(b.h, b.d, b.bytes, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}
extern "C" int wmdbg_group_rows_out(const int32_t *in, int n, int32_t *out) {
    if (!in || !out || n < 0) return -1;
    for (int i = 0; i < n; ++i)
        if (!wm_group_rows_out_flat(in + (size_t)i * WM_TX_ROWS_IN, out + (size_t)i * WM_TX_ROWS_OUT)) return -1;
    return n;
}
extern "C" int wmdbg_right_align(const int32_t *prompts, int stride, const int32_t *prompt_len, int b0, int Bg,
                                 int32_t *table_out, int32_t *off_out) {
    std::vector<int32_t> table, off;
    const int P = wm_right_align(prompts, stride, prompt_len, b0, Bg, table, off);
    std::copy(table.begin(), table.end(), table_out);
    std::copy(off.begin(), off.end(), off_out);
    return P;
}
extern "C" int wmdbg_lane_parts(int B, int lanes, int explicit_lanes, int n_text_state) {
    return wm_lane_parts(B, lanes, explicit_lanes != 0, n_text_state, 0, g_wm_tuning);
}
extern "C" int wmdbg_cu_mask(int cu_lo, int cu_hi, uint32_t *mask8) { return wm_cu_mask(cu_lo, cu_hi, mask8); }

extern "C" int wmdbg_mel_filterbank(int n_mels, float *out) {
    WM_REQUIRE(out && n_mels > 0 && n_mels <= 256, WM_ERR_INVALID, "bad args");
    std::vector<float> f;
    wm_mel_filterbank(n_mels, f);
    memcpy(out, f.data(), f.size() * sizeof(float));
    return WM_OK;
}
extern "C" int wmdbg_mel80(float *out) {
    WM_REQUIRE(out, WM_ERR_INVALID, "null");
    memcpy(out, wm_mel80_table(), sizeof(float) * 80 * 201);
    return WM_OK;
}

// ------------------------------------------------------------------ per-kernel test hooks
extern "C" int wmdbg_gemm(wm_ctx *ctx, const float *A, const float *W, const float *bias, float *C, int M, int N,
                          int K, int epi) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(epi == EPI_F32 || epi == EPI_BIAS_BF16 || epi == EPI_GELU_BF16 || epi == EPI_RESID_F32, WM_ERR_INVALID,
               "wmdbg_gemm: epilogue %d not exposed", epi);
    std::vector<bf16_t> a16, w16;
    to_bf16(A, a16, (size_t)M * K);
    to_bf16(W, w16, (size_t)N * K);
    const bool f32out = (epi == EPI_F32 || epi == EPI_RESID_F32);
    DevPool pool;
    hipStream_t s = ctx->stream;
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    WM_TRY(pool.get(&g.A, a16.data(), a16.size() * 2, s));
    WM_TRY(pool.get(&g.W, w16.data(), w16.size() * 2, s));
    if (bias) WM_TRY(pool.get(&g.bias, bias, (size_t)N * 4, s));
    WM_TRY(pool.get(&g.C, epi == EPI_RESID_F32 ? C : nullptr, (size_t)M * N * (f32out ? 4 : 2), s));
    g.a_rpb = (long)M + 1; g.a_rstride = K;
    g.c_rpb = (long)M + 1; g.c_rstride = N; g.M = M; g.N = N; g.K = K; g.epi = epi;
    WM_TRY(wm_gemm(ctx, g));
    if (!f32out) return down_bf16(g.C, (size_t)M * N, C, s);
    WM_HIP(hipMemcpyAsync(C, g.C, (size_t)M * N * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

extern "C" int wmdbg_layernorm(wm_ctx *ctx, const float *x, const float *g, const float *b, int rows, int d,
                               float *out_f32, float *out_bf16_as_f32) {
    WM_TRY(wm_ctx_make_current(ctx));
    DevPool pool;
    hipStream_t s = ctx->stream;
    WM_REQUIRE(x && g && b && rows >= 1 && d >= 1 && (out_f32 || out_bf16_as_f32), WM_ERR_INVALID, "wmdbg_layernorm: bad args");
    const float *dx, *dg, *db;
    float *of = nullptr;   // a null host output reaches wm_layernorm as a null output
    bf16_t *ob = nullptr;
    WM_TRY(pool.get(&dx, x, (size_t)rows * d * 4, s));
    WM_TRY(pool.get(&dg, g, (size_t)d * 4, s));
    WM_TRY(pool.get(&db, b, (size_t)d * 4, s));
    if (out_f32) WM_TRY(pool.get(&of, nullptr, (size_t)rows * d * 4, s));
    if (out_bf16_as_f32) WM_TRY(pool.get(&ob, nullptr, (size_t)rows * d * 2, s));
    WM_TRY(wm_layernorm(ctx, dx, dg, db, rows, d, ob, of));
    if (out_f32) WM_HIP(hipMemcpyAsync(out_f32, of, (size_t)rows * d * 4, hipMemcpyDeviceToHost, s));
    if (out_bf16_as_f32) return down_bf16(ob, (size_t)rows * d, out_bf16_as_f32, s);
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

// The sampling noise of wm_transcribe as the device computes it (the DE_LOGITS_X epilogue's philox.h functions).
extern "C" int wmdbg_sample_noise(wm_ctx *ctx, uint64_t seed, int chunk, int gi, int n0, int count, float *g) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(g && count >= 0, WM_ERR_INVALID, "bad args");
    if (count == 0) return WM_OK;
    DevPool pool;
    hipStream_t s = ctx->stream;
    float *dg;
    WM_TRY(pool.get(&dg, nullptr, (size_t)count * 4, s));
    WM_TRY(wm_sample_noise(ctx, seed, chunk, gi, n0, count, dg));
    WM_HIP(hipMemcpyAsync(g, dg, (size_t)count * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

// Encoder attention on host q, k, v given as f32 [B][S][H*64] each (rounded to bf16 inside).
extern "C" int wmdbg_enc_attention(wm_ctx *ctx, const float *q, const float *k, const float *v, int B, int H, int S,
                                   float *out) {
    return wmdbg_enc_attention_ex(ctx, q, k, v, B, H, S, 0, out);
}

// The same; flags & 1: the 64 rows behind the last chunk's in the staged query | key buffer -- what the last chunk's final K
// tile reads behind key S - 1, as the encoder's m->qk has them behind row B * 1500 -- hold NaN instead of zeros.
extern "C" int wmdbg_enc_attention_ex(wm_ctx *ctx, const float *q, const float *k, const float *v, int B, int H, int S,
                                      int flags, float *out) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(q && k && v && out && B >= 1 && H >= 1 && S >= 1 && (flags & ~1) == 0, WM_ERR_INVALID, "wmdbg_enc_attention: bad args");
    const int d = H * 64, S_pad = ((S + 63) / 64) * 64;
    const size_t M = (size_t)B * S;
    std::vector<bf16_t> qk((M + 64) * 2 * d, 0), vt((size_t)B * H * 64 * S_pad, 0);
    if (flags & 1) std::fill(qk.begin() + M * 2 * d, qk.end(), (bf16_t)0x7fc0);
    for (size_t mrow = 0; mrow < M; ++mrow)
        for (int j = 0; j < d; ++j) {
            qk[mrow * 2 * d + j] = f2bf(q[mrow * d + j] * WM_ENC_QSCALE);   // the kernel's contract: pre-scaled queries
            qk[mrow * 2 * d + d + j] = f2bf(k[mrow * d + j]);
        }
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < S; ++s)
            for (int j = 0; j < d; ++j)
                vt[((size_t)(b * H + j / 64) * 64 + j % 64) * S_pad + wm_att_vt_pos((unsigned)s)] = f2bf(v[((size_t)b * S + s) * d + j]);
    DevPool pool;
    hipStream_t st = ctx->stream;
    const bf16_t *dqk, *dvt;
    bf16_t *datt;
    WM_TRY(pool.get(&dqk, qk.data(), qk.size() * 2, st));
    WM_TRY(pool.get(&dvt, vt.data(), vt.size() * 2, st));
    WM_TRY(pool.get(&datt, nullptr, M * d * 2, st));
    WM_TRY(wm_enc_attention(ctx, dqk, dvt, datt, B, H, S, S_pad, d));
    return down_bf16(datt, M * d, out, st);
}

// Skinny decode GEMV: out[B][N] = LN?(x)[B][K] . W[N][K]^T + bias, driven the way the decoder drives it: bf16 activations,
// LayerNorm folded into the weights (W' = bf16(W g), c1, c2 by wm_ln_fold on device) and the row statistics handed over as
// partial sums of the f32 input.
extern "C" int wmdbg_dec_gemv(wm_ctx *ctx, const float *x, const float *ln_g, const float *ln_b, const float *W,
                              const float *bias, float *out, int B, int N, int K) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB, WM_ERR_INVALID, "wmdbg_dec_gemv: B out of range");
    const int Npad = ((N + 15) / 16) * 16;
    std::vector<bf16_t> w16, x16;
    std::vector<float> st, mean;   // (the means are not handed over: the activations are not centred)
    tile_bf16(W, (size_t)N, (size_t)K, w16);
    stage_ln_rows(x, B, K, false, x16, st, mean);
    DevPool pool;
    hipStream_t s = ctx->stream;
    DecGemvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.N = N; a.K = K; a.ldo = N; a.epi = DE_Q; a.pos_ptr = nullptr;
    WM_TRY(pool.get(&a.a, x16.data(), x16.size() * 2, s));
    WM_TRY(pool.get(&a.W, w16.data(), w16.size() * 2, s));
    WM_TRY(pool.get(&a.out_f32, nullptr, (size_t)B * N * 4, s));
    if (bias) WM_TRY(pool.get(&a.c2, bias, (size_t)N * 4, s));
    if (ln_g) {
        const float *dg, *db;
        bf16_t *dWf;
        float *dc1, *dc2;
        WM_TRY(pool.get(&dg, ln_g, (size_t)K * 4, s));
        WM_TRY(pool.get(&db, ln_b, (size_t)K * 4, s));
        WM_TRY(pool.get(&dWf, nullptr, w16.size() * 2, s));
        WM_TRY(pool.get(&dc1, nullptr, (size_t)Npad * 4, s));
        WM_TRY(pool.get(&dc2, nullptr, (size_t)Npad * 4, s));
        WM_TRY(wm_ln_fold(ctx, a.W, dg, db, a.c2, N, K, dWf, dc1, dc2));
        WM_TRY(pool.get(&a.stats_in, st.data(), st.size() * 4, s));
        a.stats_parts = K / 16;
        a.W = dWf; a.c1 = dc1; a.c2 = dc2;
    }
    WM_TRY(wm_dec_gemv(ctx, a));
    WM_HIP(hipMemcpyAsync(out, a.out_f32, (size_t)B * N * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

// The residual product of a decoder layer (DE_RESID: attention out-projection K = d, fc2 K = 4d) at any decode-group size:
// this is the epilogue the two-parts-per-wave kernel serves above 16 rows when K splits over 16 waves (d = 768 / 1024 / 1280).
extern "C" int wmdbg_dec_gemv_resid(wm_ctx *ctx, const float *x, const float *W, const float *bias, float *resid,
                                    float *copy_bf16, float *stats, int B, int N, int K) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && N % 16 == 0, WM_ERR_INVALID, "wmdbg_dec_gemv_resid: B out of range / N % 16");
    const int Bpad = ((B + 15) / 16) * 16;
    std::vector<bf16_t> w16, x16;
    tile_bf16(W, (size_t)N, (size_t)K, w16);
    tile_bf16(x, (size_t)B, (size_t)K, x16);
    std::vector<float> st((size_t)(Bpad / 16) * 2 * N);
    DevPool pool;
    hipStream_t s = ctx->stream;
    DecGemvArgs a;
    memset(&a, 0, sizeof(a));
    a.epi = DE_RESID; a.B = B; a.N = N; a.K = K; a.ldo = N;
    WM_TRY(pool.get(&a.a, x16.data(), x16.size() * 2, s));
    WM_TRY(pool.get(&a.W, w16.data(), w16.size() * 2, s));
    WM_TRY(pool.get(&a.out_f32, resid, (size_t)B * N * 4, s));
    WM_TRY(pool.get(&a.out_bf16, nullptr, (size_t)Bpad * N * 2, s));
    WM_TRY(pool.get(&a.stats_out, nullptr, st.size() * 4, s));
    if (bias) WM_TRY(pool.get(&a.c2, bias, (size_t)N * 4, s));
    WM_TRY(wm_dec_gemv(ctx, a));
    WM_HIP(hipMemcpyAsync(resid, a.out_f32, (size_t)B * N * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(st.data(), a.stats_out, st.size() * 4, hipMemcpyDeviceToHost, s));
    WM_TRY(down_tiled_bf16(a.out_bf16, (size_t)B, (size_t)N, copy_bf16, s));
    for (int b = 0; b < B; ++b) stats_sum(st.data(), N, b, stats + b * 2);   // the N / 16 parts of the updated residual
    return WM_OK;
}

// Single-query attention: q f32 [B][H*64], k/v f32 [B][H][T][64] (rounded to bf16), first
// n_keys positions; `nsplit` (1, 2, 4, 8) workgroups share the 8 streams of a pair; out f32 [B][H*64].
extern "C" int wmdbg_dec_attention(wm_ctx *ctx, const float *q, const float *k, const float *v, int B, int H, int T,
                                   int n_keys, int nsplit, float *out) {
    WM_TRY(wm_ctx_make_current(ctx));
    std::vector<bf16_t> k16, v16;
    to_bf16(k, k16, (size_t)B * H * T * 64);
    to_bf16(v, v16, (size_t)B * H * T * 64);
    DevPool pool;
    hipStream_t s = ctx->stream;
    const float *dq;
    const bf16_t *dk, *dv;
    float *dp;
    bf16_t *datt;
    WM_TRY(pool.get(&dq, q, (size_t)B * H * 64 * 4, s));
    WM_TRY(pool.get(&dk, k16.data(), k16.size() * 2, s));
    WM_TRY(pool.get(&dv, v16.data(), v16.size() * 2, s));
    WM_TRY(pool.get(&dp, nullptr, (size_t)B * H * WM_MAXSPLIT * 66 * 4, s));
    WM_TRY(pool.get(&datt, nullptr, ((size_t)B + 15) / 16 * 16 * H * 64 * 2, s));
    // nsplit == 0 selects the decoder's self-attention kernel (one 4-wave workgroup per pair), nsplit == -1 the
    // cross-attention launch path (8-wave block-streaming kernel, capped grid)
    DecAttnArgs t = {};
    t.q = dq; t.kc = dk; t.vc = dv; t.att = datt; t.part = dp; t.B = B; t.H = H; t.T_stride = T; t.n_keys = n_keys;
    t.nsplit = nsplit < 0 ? 1 : nsplit;
    WM_TRY(nsplit == 0 ? wm_dec_self_attention(ctx, t) : wm_dec_attention(ctx, t));
    return down_tiled_bf16(datt, (size_t)B, (size_t)H * 64, out, s);
}

// The cross-attention launch of a candidate group (wm_transcribe_mel_best_of), as wm_model_decode_step makes it; short_lived:
// the shape of a burst that shares the chip (WmDecodeMode::xattn_shared)
static int dec_attention_cand(wm_ctx *ctx, const float *q, const float *k, const float *v, int C, int N, int H, int T, int n_keys,
                              const int32_t *live_rows, int n_live, float *out, bool short_lived) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(q && k && v && out, WM_ERR_INVALID, "dec_attention_cand: null pointer");
    WM_REQUIRE(N >= 1 && N <= WM_MAX_BEST_OF && C >= 1 && C * N <= WM_DEC_MAXB && H >= 1 && H <= 255 && T >= 1 && n_keys >= 1 &&
                   n_keys <= T,
               WM_ERR_INVALID, "dec_attention_cand: bad geometry");
    const int B = C * N;
    std::vector<int32_t> live((size_t)WM_DEC_MAXB + 4, 0);
    if (live_rows) {
        WM_REQUIRE(n_live >= 0 && n_live <= B, WM_ERR_INVALID, "dec_attention_cand: n_live %d outside [0, %d]", n_live, B);
        for (int i = 0; i < n_live; ++i) {
            WM_REQUIRE(live_rows[i] >= 0 && live_rows[i] < B && (i == 0 || live_rows[i] > live_rows[i - 1]), WM_ERR_INVALID,
                       "dec_attention_cand: the live list must be ascending rows of the group");
            live[i] = live_rows[i];
        }
        live[WM_DEC_MAXB] = n_live;
    }
    std::vector<bf16_t> k16, v16;
    to_bf16(k, k16, (size_t)C * H * T * 64);
    to_bf16(v, v16, (size_t)C * H * T * 64);
    DevPool pool;
    hipStream_t s = ctx->stream;
    const float *dq;
    const bf16_t *dk, *dv;
    float *dp;
    const int *dl;
    bf16_t *datt;
    WM_TRY(pool.get(&dq, q, (size_t)B * H * 64 * 4, s));
    WM_TRY(pool.get(&dk, k16.data(), k16.size() * 2, s));
    WM_TRY(pool.get(&dv, v16.data(), v16.size() * 2, s));
    WM_TRY(pool.get(&dp, nullptr, (size_t)B * H * WM_MAXSPLIT * 66 * 4, s));
    WM_TRY(pool.get(&dl, live.data(), live.size() * 4, s));
    WM_TRY(pool.get(&datt, nullptr, ((size_t)B + 15) / 16 * 16 * H * 64 * 2, s));
    DecAttnArgs t = {};
    t.q = dq; t.kc = dk; t.vc = dv; t.att = datt; t.part = dp; t.C = C; t.N = N; t.H = H; t.T_stride = T; t.n_keys = n_keys;
    t.live = live_rows ? dl : nullptr; t.short_lived = short_lived;
    WM_TRY(wm_dec_attention_cand(ctx, t));
    return down_tiled_bf16(datt, (size_t)B, (size_t)H * 64, out, s);
}

extern "C" int wmdbg_dec_attention_cand(wm_ctx *ctx, const float *q, const float *k, const float *v, int C, int N, int H, int T,
                                        int n_keys, const int32_t *live_rows, int n_live, float *out) {
    return dec_attention_cand(ctx, q, k, v, C, N, H, T, n_keys, live_rows, n_live, out, false);
}
extern "C" int wmdbg_dec_attention_cand_shared(wm_ctx *ctx, const float *q, const float *k, const float *v, int C, int N, int H,
                                               int T, int n_keys, const int32_t *live_rows, int n_live, float *out) {
    return dec_attention_cand(ctx, q, k, v, C, N, H, T, n_keys, live_rows, n_live, out, true);
}

// The production self-attention launch of a ragged decode group: position `pos`, sequence b's keys [min(off[b], pos), pos].
extern "C" int wmdbg_dec_self_attention_off(wm_ctx *ctx, const float *q, const float *k, const float *v, int B, int H, int T,
                                            int pos, const int32_t *off, float *out) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(q && k && v && off && out, WM_ERR_INVALID, "dec_self_attention_off: null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && T >= 1 && pos >= 0 && pos < T, WM_ERR_INVALID, "dec_self_attention_off: bad geometry");
    for (int b = 0; b < B; ++b)
        WM_REQUIRE(off[b] >= 0 && off[b] < T, WM_ERR_INVALID, "dec_self_attention_off: off[%d] = %d outside [0, %d)", b, off[b], T);
    std::vector<bf16_t> k16, v16;
    to_bf16(k, k16, (size_t)B * H * T * 64);
    to_bf16(v, v16, (size_t)B * H * T * 64);
    DevPool pool;
    hipStream_t s = ctx->stream;
    const float *dq;
    const bf16_t *dk, *dv;
    const int *doff, *dpos;
    bf16_t *datt;
    WM_TRY(pool.get(&dq, q, (size_t)B * H * 64 * 4, s));
    WM_TRY(pool.get(&dk, k16.data(), k16.size() * 2, s));
    WM_TRY(pool.get(&dv, v16.data(), v16.size() * 2, s));
    WM_TRY(pool.get(&doff, off, (size_t)B * 4, s));
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&datt, nullptr, ((size_t)B + 15) / 16 * 16 * H * 64 * 2, s));
    DecAttnArgs t = {};
    t.q = dq; t.kc = dk; t.vc = dv; t.att = datt; t.B = B; t.H = H; t.T_stride = T; t.pos_ptr = dpos; t.off = doff;
    WM_TRY(wm_dec_self_attention(ctx, t));
    return down_tiled_bf16(datt, (size_t)B, (size_t)H * 64, out, s);
}

// Every decode-attention form as the decode step drives it (struct wmdbg_attn): one launcher call on staged host data, the
// plan the launcher used beside the outputs.  Nothing is launched for a geometry the plan refuses or for an address that would
// leave a buffer; the caller's output buffers then hold the sentinels.
extern "C" int wmdbg_attn_layout(int32_t *out4) {
    if (!out4) return WM_ERR_INVALID;
    out4[0] = (int32_t)sizeof(wmdbg_attn); out4[1] = (int32_t)offsetof(wmdbg_attn, off);
    out4[2] = (int32_t)offsetof(wmdbg_attn, out); out4[3] = (int32_t)offsetof(wmdbg_attn, plan);
    return WM_OK;
}

extern "C" int wmdbg_dec_attention_form(wm_ctx *ctx, wmdbg_attn *io) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(io && io->out && io->k && io->v, WM_ERR_INVALID, "dec_attention_form: null pointer");
    memset(io->plan, 0, sizeof(io->plan));
    const int form = io->form, H = io->H, T = io->T;
    WM_REQUIRE(form >= 0 && form <= 3, WM_ERR_INVALID, "dec_attention_form: form %d is not 0 .. 3", form);
    const bool cand = form == 1, fq = form == 2, self = form == 3;
    WM_REQUIRE(!cand || (io->C >= 1 && io->N >= 1 && io->N <= WM_MAX_BEST_OF && io->C <= WM_DEC_MAXB), WM_ERR_INVALID,
               "dec_attention_form: %d windows x %d candidates", io->C, io->N);
    const int rows = cand ? io->C * io->N : io->B, entries = cand ? io->C : io->B;
    WM_REQUIRE(rows >= 1 && rows <= WM_DEC_MAXB && H >= 1 && H <= 1024, WM_ERR_INVALID, "dec_attention_form: %d rows x %d heads", rows, H);
    const size_t dd = (size_t)H * 64, rpad = ((size_t)rows + 15) / 16 * 16;
    {   // what a refused call leaves behind: the sentinels
        std::vector<bf16_t> s16;
        fill_bf16(s16, rpad * dd);
        from_bf16(s16, io->out);
        const uint32_t u = WMDBG_SENTINEL_F32;
        for (int b = 0; fq && io->mean_out && b < rows; ++b) memcpy(io->mean_out + b, &u, 4);
    }
    // ---- the plan, from the function the launcher asks (and with the context's CUs)
    const bool has_pos = io->pos >= 0, has_pf = io->warm_rows > 0 && io->warm_k > 0;
    int32_t pin[WM_ATTN_PLAN_IN] = {0};
    pin[0] = form; pin[1] = cand ? 0 : io->B; pin[2] = cand ? io->C : 0; pin[3] = cand ? io->N : 0; pin[4] = H; pin[5] = T;
    pin[6] = io->n_keys; pin[7] = io->nsplit; pin[8] = fq ? io->K : 0;
    pin[9] = (has_pos ? 1 : 0) | (fq || self ? 0 : 2) | (io->off ? 4 : 0) | (has_pf ? 8 : 0) | (io->short_lived ? 16 : 0) | (io->live_rows ? 32 : 0);
    pin[10] = has_pf ? io->warm_rows : 0; pin[11] = has_pf ? io->warm_k : 0; pin[12] = ctx->n_cus;
    wm_attn_plan_flat(pin, g_wm_tuning, io->plan);
    if (io->plan[0] != WM_OK) return WM_ERR_INVALID;   // (the plan function has set the message)
    // ---- every address inside its buffer
    WM_REQUIRE(H <= 255 && T >= 1 && T <= WM_ATT_MAXK, WM_ERR_INVALID, "dec_attention_form: H 1 .. 255, T 1 .. %d", WM_ATT_MAXK);
    WM_REQUIRE(!has_pos || form == 0 || self, WM_ERR_INVALID, "dec_attention_form: form %d takes no device position", form);
    const int nk = has_pos ? io->pos + 1 : io->n_keys;
    WM_REQUIRE(nk >= 1 && nk <= T && io->n_keys >= 0 && io->n_keys <= T, WM_ERR_INVALID, "dec_attention_form: %d keys outside 1 .. T = %d", nk, T);
    // (the cross kernels clamp their loads to row n_keys - 1 whether or not the position comes from device memory)
    WM_REQUIRE(self || (io->n_keys >= 1 && (!has_pos || io->n_keys == nk)), WM_ERR_INVALID,
               "dec_attention_form: a cross form needs n_keys >= 1 keys, and n_keys = pos + 1 with a device position");
    WM_REQUIRE(!io->off || self, WM_ERR_INVALID, "dec_attention_form: row offsets belong to the self-attention");
    WM_REQUIRE(!io->off || has_pos, WM_ERR_INVALID, "dec_attention_form: row offsets need the device position");
    for (int b = 0; io->off && b < rows; ++b)
        WM_REQUIRE(io->off[b] >= 0 && io->off[b] < T, WM_ERR_INVALID, "dec_attention_form: off[%d] = %d outside [0, %d)", b, io->off[b], T);
    WM_REQUIRE(!io->short_lived || form <= 1, WM_ERR_INVALID, "dec_attention_form: short_lived is a cross-attention shape");
    WM_REQUIRE(io->warm_rows >= 0 && io->warm_rows <= 8192 && io->warm_k >= 0 && io->warm_k <= 8192 && io->warm_k % 32 == 0 && io->warm_rows % 16 == 0,
               WM_ERR_INVALID, "dec_attention_form: warm-up matrix of %d x %d", io->warm_rows, io->warm_k);
    std::vector<int32_t> live((size_t)WM_DEC_MAXB + 4, 0);
    if (io->live_rows) {
        WM_REQUIRE(io->n_live >= 0 && io->n_live <= rows, WM_ERR_INVALID, "dec_attention_form: n_live %d outside [0, %d]", io->n_live, rows);
        for (int i = 0; i < io->n_live; ++i) {
            WM_REQUIRE(io->live_rows[i] >= 0 && io->live_rows[i] < rows && (i == 0 || io->live_rows[i] > io->live_rows[i - 1]), WM_ERR_INVALID,
                       "dec_attention_form: the live list must be ascending rows of the group");
            live[i] = io->live_rows[i];
        }
        live[WM_DEC_MAXB] = io->n_live;
    }
    if (fq)
        WM_REQUIRE(io->x && io->ln_g && io->ln_b && io->Wq && io->mean_out && io->K == H * 64 && io->K <= 1280, WM_ERR_INVALID,
                   "dec_attention_form: the fused query needs x, ln_g, ln_b, Wq, mean_out and K = H * 64 <= 1280");
    else
        WM_REQUIRE(io->q, WM_ERR_INVALID, "dec_attention_form: null query");
    // ---- staging
    std::vector<bf16_t> k16, v16, w16, x16, fill;
    std::vector<float> st, mean;
    to_bf16(io->k, k16, (size_t)entries * dd * T);
    to_bf16(io->v, v16, (size_t)entries * dd * T);
    fill_bf16(fill, rpad * dd);
    const std::vector<uint32_t> fill32((size_t)rows, WMDBG_SENTINEL_F32);
    DevPool pool;
    hipStream_t s = ctx->stream;
    const bf16_t *dk, *dv;
    bf16_t *datt;
    WM_TRY(pool.get(&dk, k16.data(), k16.size() * 2, s));
    WM_TRY(pool.get(&dv, v16.data(), v16.size() * 2, s));
    WM_TRY(pool.get(&datt, fill.data(), fill.size() * 2, s));
    DecAttnArgs t = {};
    t.kc = dk; t.vc = dv; t.att = datt; t.H = H; t.T_stride = T; t.n_keys = io->n_keys; t.short_lived = io->short_lived != 0;
    if (cand) { t.C = io->C; t.N = io->N; } else t.B = io->B;
    if (!fq) WM_TRY(pool.get(&t.q, io->q, (size_t)rows * dd * 4, s));
    if (form <= 1) WM_TRY(pool.get(&t.part, nullptr, (size_t)rows * H * WM_MAXSPLIT * 66 * 4, s));
    if (has_pos) WM_TRY(pool.get(&t.pos_ptr, &io->pos, 4, s));
    if (io->off) WM_TRY(pool.get(&t.off, io->off, (size_t)rows * 4, s));
    if (io->live_rows) WM_TRY(pool.get(&t.live, live.data(), live.size() * 4, s));
    if (has_pf) {
        WM_TRY(pool.get(&t.pf.ptr, nullptr, (size_t)io->warm_rows * io->warm_k * 2, s));
        t.pf.rows = io->warm_rows; t.pf.k = io->warm_k;
    }
    float *dmean_out = nullptr;
    switch (form) {
        case 0: t.nsplit = io->nsplit; WM_TRY(wm_dec_attention(ctx, t)); break;
        case 1: WM_TRY(wm_dec_attention_cand(ctx, t)); break;
        case 3: WM_TRY(wm_dec_self_attention(ctx, t)); break;
        default: {   // the query side as wmdbg_dec_gemv_ln stages it (DE_Q, centre = 1), wm_ln_fold first
            const int K = io->K, B = io->B;
            tile_bf16(io->Wq, (size_t)K, (size_t)K, w16);
            stage_ln_rows(io->x, B, K, true, x16, st, mean);
            DecGemvArgs a;
            memset(&a, 0, sizeof(a));
            a.epi = DE_Q; a.B = B; a.N = K; a.K = K; a.stats_parts = K / 16; a.ldo = K;
            const bf16_t *dW;
            bf16_t *dWf;
            float *dc1, *dc2;
            const float *dg, *db, *dbias = nullptr;
            WM_TRY(pool.get(&a.a, x16.data(), x16.size() * 2, s));
            WM_TRY(pool.get(&dW, w16.data(), w16.size() * 2, s));
            WM_TRY(pool.get(&dWf, nullptr, w16.size() * 2, s));
            WM_TRY(pool.get(&dc1, nullptr, (size_t)K * 4, s));
            WM_TRY(pool.get(&dc2, nullptr, (size_t)K * 4, s));
            WM_TRY(pool.get(&dg, io->ln_g, (size_t)K * 4, s));
            WM_TRY(pool.get(&db, io->ln_b, (size_t)K * 4, s));
            if (io->bias) WM_TRY(pool.get(&dbias, io->bias, (size_t)K * 4, s));
            WM_TRY(pool.get(&a.stats_in, st.data(), st.size() * 4, s));
            WM_TRY(pool.get(&a.mean_in, mean.data(), (size_t)B * 4, s));
            WM_TRY(pool.get(&a.mean_out, fill32.data(), (size_t)B * 4, s));
            WM_TRY(wm_ln_fold(ctx, dW, dg, db, dbias, K, K, dWf, dc1, dc2));
            a.W = dWf; a.c1 = dc1; a.c2 = dc2;
            dmean_out = a.mean_out;
            WM_TRY(wm_dec_xattn_fq(ctx, a, t));
        }
    }
    if (dmean_out) WM_HIP(hipMemcpyAsync(io->mean_out, dmean_out, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
    return down_tiled_bf16(datt, rpad, dd, io->out, s);
}

// ------------------------------------------------------------------ micro-benchmarks ------
// Time `iters` back-to-back launches of one decode kernel, cycling over `n_mats` distinct weight
// matrices / cache slices so nothing is served from L2 or MALL.  Returns average microseconds
// per launch (HIP events on the context's stream).

extern "C" int wmdbg_bench_dec_gemv(wm_ctx *ctx, int B, int N, int K, int ln, int resid, int n_mats, int iters,
                                    int nw_override, float *avg_us) {
    (void)nw_override;  // the K split is a function of K alone (wm_dec_gemv_split)
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB, WM_ERR_INVALID, "wmdbg_bench_dec_gemv: B out of range");
    DevPool pool;
    hipStream_t s = ctx->stream;
    const int Npad = ((N + 15) / 16) * 16;
    const bf16_t *dW;
    const float *dc;
    bf16_t *dout16;
    float *dstat;
    DecGemvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.N = N; a.K = K; a.ldo = Npad; a.epi = resid ? DE_RESID : DE_Q;
    WM_TRY(pool.get(&dW, nullptr, (size_t)n_mats * Npad * K * 2, s, 0x3c));
    WM_TRY(pool.get(&a.a, nullptr, (size_t)WM_DEC_MAXB * K * 2, s));
    WM_TRY(pool.get(&dc, nullptr, (size_t)Npad * 4, s));
    WM_TRY(pool.get(&a.out_f32, nullptr, (size_t)WM_DEC_MAXB * Npad * 4, s));
    WM_TRY(pool.get(&dout16, nullptr, (size_t)WM_DEC_MAXB * Npad * 2, s));
    WM_TRY(pool.get(&dstat, nullptr, (size_t)(WM_DEC_MAXB / 16) * 2 * (K > N ? K : N) * 4 + 4096, s));
    a.c2 = dc;
    if (resid) { a.stats_out = dstat; a.out_bf16 = dout16; }
    if (ln) { a.c1 = dc; a.stats_in = dstat; a.stats_parts = K / 16; }
    EventPair ev;
    WM_TRY(ev.init());
    // capture the launch chain once, replay it: per-kernel time = true serialized duration
    GraphRun run(s);
    WM_TRY(run.begin());
    for (int i = 0; i < iters; ++i) {
        a.W = dW + (size_t)(i % n_mats) * Npad * K;
        WM_TRY(wm_dec_gemv(ctx, a));
    }
    WM_TRY(run.end());
    float us = 0.f;
    WM_TRY(run.replay_us(ev, &us));
    *avg_us = us / iters;
    return WM_OK;
}

extern "C" int wmdbg_bench_dec_attention(wm_ctx *ctx, int B, int H, int T, int n_keys, int nsplit, int n_slices,
                                         int iters, float *avg_us) {
    WM_TRY(wm_ctx_make_current(ctx));
    DevPool pool;
    hipStream_t s = ctx->stream;
    const size_t slice = (size_t)B * H * T * 64;
    const bf16_t *dk, *dv;
    const float *dq;
    float *dp;
    bf16_t *datt;
    WM_TRY(pool.get(&dk, nullptr, slice * n_slices * 2, s));
    WM_TRY(pool.get(&dv, nullptr, slice * n_slices * 2, s));
    WM_TRY(pool.get(&dq, nullptr, (size_t)B * H * 64 * 4, s));
    WM_TRY(pool.get(&dp, nullptr, (size_t)B * H * WM_MAXSPLIT * 66 * 4, s));
    WM_TRY(pool.get(&datt, nullptr, ((size_t)B + 15) / 16 * 16 * H * 64 * 2, s));
    EventPair ev;
    WM_TRY(ev.init());
    DecAttnArgs t = {};
    t.q = dq; t.att = datt; t.part = dp; t.B = B; t.H = H; t.T_stride = T; t.n_keys = n_keys; t.nsplit = nsplit;
    for (int pass = 0; pass < 2; ++pass) {   // a warm pass, then the timed one
        if (pass == 1) WM_TRY(ev.start(s));
        for (int i = 0; i < iters; ++i) {
            t.kc = dk + (size_t)(i % n_slices) * slice;
            t.vc = dv + (size_t)(i % n_slices) * slice;
            WM_TRY(wm_dec_attention(ctx, t));
        }
    }
    float us = 0.f;
    WM_TRY(ev.stop_us(s, &us));
    *avg_us = us / iters;
    return WM_OK;
}

int wm_launch_trivial(wm_ctx *ctx, int *p, int grid);
// Dependent-launch floor of this machine: `iters` trivial kernels (each increments one HBM word,
// so they are truly serialised), eager stream launches vs one captured hipGraph replayed.
extern "C" int wmdbg_bench_launch_floor(wm_ctx *ctx, int iters, int grid, float *eager_us, float *graph_us) {
    WM_TRY(wm_ctx_make_current(ctx));
    DevPool pool;
    hipStream_t s = ctx->stream;
    int *d;
    WM_TRY(pool.get(&d, nullptr, 64, s));
    EventPair ev;
    WM_TRY(ev.init());
    float us = 0.f;
    for (int i = 0; i < 20; ++i) WM_TRY(wm_launch_trivial(ctx, d, grid));
    WM_TRY(ev.start(s));
    for (int i = 0; i < iters; ++i) WM_TRY(wm_launch_trivial(ctx, d, grid));
    WM_TRY(ev.stop_us(s, &us));
    *eager_us = us / iters;
    GraphRun run(s);
    WM_TRY(run.begin());
    for (int i = 0; i < iters; ++i) WM_TRY(wm_launch_trivial(ctx, d, grid));
    WM_TRY(run.end());
    WM_TRY(run.replay_us(ev, &us));
    *graph_us = us / iters;
    return WM_OK;
}

// Mean duration (us) of `iters` back-to-back launches of one encoder GEMM shape.  Operands as in the encoder:
// A ~ N(0,1), W ~ N(0, 0.02^2), bias ~ 0.01 N(0,1); the launches rotate over `n_w` weight matrices so that W comes
// from HBM as it does in the 32-layer encoder (n_w = 1: W stays cache-resident).
extern "C" int wmdbg_bench_gemm(wm_ctx *ctx, int M, int N, int K, int epi, int iters, int n_w, float *us) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(epi == EPI_F32 || epi == EPI_BIAS_BF16 || epi == EPI_GELU_BF16 || epi == EPI_RESID_F32, WM_ERR_INVALID,
               "wmdbg_bench_gemm: epilogue %d not exposed", epi);
    WM_REQUIRE(n_w >= 1 && n_w <= 64, WM_ERR_INVALID, "wmdbg_bench_gemm: n_w out of range");
    std::vector<bf16_t> a16((size_t)M * K), w16((size_t)N * K);
    uint32_t x = 12345u;
    auto gauss = [&]() {  // Irwin-Hall(4), unit variance
        float acc = 0.f;
        for (int i = 0; i < 4; ++i) { x = x * 1664525u + 1013904223u; acc += (float)(x >> 8) * (1.0f / 16777216.0f); }
        return (acc - 2.0f) * 1.7320508f;
    };
    for (auto &v : a16) v = f2bf(gauss());
    for (auto &v : w16) v = f2bf(0.02f * gauss());
    std::vector<float> bias(N);
    for (auto &v : bias) v = 0.01f * gauss();
    DevPool pool;
    hipStream_t s = ctx->stream;
    std::vector<const bf16_t *> dW(n_w, nullptr);
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    WM_TRY(pool.get(&g.A, a16.data(), a16.size() * 2, s));
    for (int i = 0; i < n_w; ++i) WM_TRY(pool.get(&dW[i], w16.data(), w16.size() * 2, s));
    WM_TRY(pool.get(&g.bias, bias.data(), (size_t)N * 4, s));
    WM_TRY(pool.get(&g.C, nullptr, (size_t)M * N * 4, s));
    g.a_rpb = (long)M + 1; g.a_rstride = K;
    g.c_rpb = (long)M + 1; g.c_rstride = N; g.M = M; g.N = N; g.K = K; g.epi = epi;
    EventPair ev;
    WM_TRY(ev.init());
    for (int i = 0; i < 3; ++i) { g.W = dW[i % n_w]; WM_TRY(wm_gemm(ctx, g)); }
    WM_TRY(ev.start(s));
    for (int i = 0; i < iters; ++i) { g.W = dW[i % n_w]; WM_TRY(wm_gemm(ctx, g)); }
    float total = 0.f;
    WM_TRY(ev.stop_us(s, &total));
    *us = total / iters;
    return WM_OK;
}

int wm_launch_spin(hipStream_t s, int *p, int grid, int cycles);
// Do two independent branches of a captured hipGraph run concurrently?  Each branch is a chain of
// `iters` kernels that spin ~`us_each` microseconds on `grid` workgroups.  Returns wall time of one
// replay with 1 branch and with 2 branches.
extern "C" int wmdbg_bench_graph_branches(wm_ctx *ctx, int iters, int grid, int us_each, float *one_us, float *two_us) {
    WM_TRY(wm_ctx_make_current(ctx));
    DevPool pool;
    hipStream_t s = ctx->stream;
    SideBranch side;
    WM_TRY(side.init());
    int *d;
    WM_TRY(pool.get(&d, nullptr, 256, s));
    const int cycles = us_each * 100;  // wall_clock64 ticks at 100 MHz
    EventPair ev;
    WM_TRY(ev.init());
    for (int nb = 1; nb <= 2; ++nb) {
        GraphRun run(s);
        WM_TRY(run.begin());
        if (nb == 2) WM_TRY(side.fork(s));
        for (int i = 0; i < iters; ++i) {
            WM_TRY(wm_launch_spin(s, d, grid, cycles));
            if (nb == 2) WM_TRY(wm_launch_spin(side.s2, d + 16, grid, cycles));
        }
        if (nb == 2) WM_TRY(side.join(s));
        WM_TRY(run.end());
        WM_TRY(run.replay_us(ev, nb == 1 ? one_us : two_us));
    }
    return WM_OK;
}

extern "C" int wmdbg_dtw(wm_ctx *ctx, const float *x, int B, const int32_t *N, const int32_t *M, int ld, int32_t *start) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(x && N && M && start && B >= 1 && ld >= 1, WM_ERR_INVALID, "bad args");
    int nmax = 0, mmax = 0;
    for (int b = 0; b < B; ++b) {
        WM_REQUIRE(N[b] >= 0 && N[b] <= 448 && M[b] >= 0 && M[b] <= 1500 && M[b] <= ld, WM_ERR_INVALID, "dtw: bad shape");
        nmax = N[b] > nmax ? N[b] : nmax;
        mmax = M[b] > mmax ? M[b] : mmax;
    }
    if (nmax == 0) return WM_OK;
    DevPool pool;
    hipStream_t s = ctx->stream;
    const float *dx;
    const int *dn, *dm;
    unsigned *dt;
    int *ds;
    WM_TRY(pool.get(&dx, x, (size_t)B * nmax * ld * 4, s));
    WM_TRY(pool.get(&dn, N, (size_t)B * 4, s));
    WM_TRY(pool.get(&dm, M, (size_t)B * 4, s));
    WM_TRY(pool.get(&dt, nullptr, (size_t)B * wm_dtw_trace_words(nmax) * 4, s));
    WM_TRY(pool.get(&ds, nullptr, (size_t)B * nmax * 4, s));
    WM_TRY(wm_dtw(ctx, dx, (long)nmax * ld, ld, dn, dm, B, nmax, mmax, dt, ds, nmax));
    WM_HIP(hipMemcpyAsync(start, ds, (size_t)B * nmax * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

// the one-shots of the NEXT transcribe call on ctx (WmDebugShots, tx_pending.h): the hooks that arm one
template <typename T>
static int arm_shot(wm_ctx *ctx, bool ok, T WmDebugShots::*shot, T v) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(ctx->model && ok, WM_ERR_INVALID, "bad args");
    ctx->model->pending.dbg.*shot = v;
    return WM_OK;
}
extern "C" int wmdbg_align_capture(wm_ctx *ctx, float *matrix_out) { return arm_shot(ctx, matrix_out, &WmDebugShots::align_matrix, matrix_out); }
// ---- the aligned best-of / beam calls (wm_transcribe_mel_beam_aligned) ----
extern "C" int wmdbg_align_hyp(wm_ctx *ctx, int h) { return arm_shot(ctx, h >= 0, &WmDebugShots::align_hyp, h); }
extern "C" int wmdbg_hyp_slots(wm_ctx *ctx, int32_t *slots_out) { return arm_shot(ctx, slots_out, &WmDebugShots::align_slots, slots_out); }
extern "C" int wmdbg_beam_trace(wm_ctx *ctx, float *trace_out) { return arm_shot(ctx, trace_out, &WmDebugShots::beam_trace, trace_out); }

extern "C" int wmdbg_beam_ancestry(int N, int max_new, const int32_t *anc, int fin_n, const int32_t *fin_src, const int32_t *fin_len,
                                   int wsteps, const float *sum, int h, int S, int Tq, int32_t *slot) {
    if (N < 1 || N > WM_MAX_BEAM || max_new < 1 || !anc || !fin_src || !fin_len || !sum || !slot || fin_n < 0 ||
        fin_n > WM_MAX_BEAM_HYPS || wsteps < 0 || wsteps > max_new || S < 0 || Tq < 1)
        return -2;
    for (int i = 0; i < max_new * N; ++i)
        if (anc[i] < 0 || anc[i] >= N) return -2;
    for (int f = 0; f < fin_n; ++f)
        if (fin_src[f] < 0 || fin_src[f] >= N || fin_len[f] < 1 || fin_len[f] > max_new) return -2;
    return wm_beam_ancestry(N, anc, N, fin_n, fin_src, fin_len, wsteps, sum, h, S, Tq, slot);
}

extern "C" int wmdbg_align_gather(wm_ctx *ctx, const float *cap, int C, int N, int Tq, int J, const int32_t *slot,
                                  const int32_t *n_rows, float *q_sel) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(cap && slot && n_rows && q_sel && C >= 1 && N >= 1 && N <= WM_MAX_BEAM && C * N <= WM_DEC_MAXB && Tq >= 1 && Tq <= 448 &&
                   J >= 1, WM_ERR_INVALID, "align_gather: bad args");
    for (int c = 0; c < C; ++c) {
        WM_REQUIRE(n_rows[c] >= 0 && n_rows[c] <= Tq, WM_ERR_INVALID, "align_gather: n_rows[%d] = %d outside [0, %d]", c, n_rows[c], Tq);
        for (int t = 0; t < Tq; ++t)
            WM_REQUIRE(slot[c * Tq + t] >= 0 && slot[c * Tq + t] < N, WM_ERR_INVALID, "align_gather: slot[%d][%d] = %d", c, t, slot[c * Tq + t]);
    }
    const size_t sel_bytes = (size_t)C * Tq * J * 64 * 4;
    DevPool pool;
    hipStream_t s = ctx->stream;
    const float *dcap;
    const int *dslot, *drows;
    float *dsel;
    WM_TRY(pool.get(&dcap, cap, sel_bytes * N, s));
    WM_TRY(pool.get(&dslot, slot, (size_t)C * Tq * 4, s));
    WM_TRY(pool.get(&drows, n_rows, (size_t)C * 4, s));
    WM_TRY(pool.get(&dsel, q_sel, sel_bytes, s));   // the caller's fill stays where nothing is written
    WM_TRY(wm_align_gather(ctx, dcap, dsel, dslot, drows, C, N, Tq, J));
    WM_HIP(hipMemcpyAsync(q_sel, dsel, sel_bytes, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

// tail: decoder rows behind the last cost-matrix row (WmAlignDev::tail, and n_min with it).  1: wm_align's row rule -- chunk b
// has S + n_text[b] + 2 decoder rows, n_text 0 is an untouched chunk; 0: an aligned transcribe group's -- S + n_text[b] + 1
// decoder rows, n_text -1 is the untouched chunk and 0 a one-row matrix.  Either way the matrix has n_text[b] + 1 rows.
static int align_matrix_hook(wm_ctx *ctx, const float *q, const float *keys, int L, int H, int B, int Tq, int J,
                             const int32_t *hl, const int32_t *hh, int S, const int32_t *n_text, const int32_t *n_frames,
                             int medfilt_width, float qk_scale, float *x, float *col_stats, int tail) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(q && keys && hl && hh && n_text && n_frames && x && L >= 1 && H >= 1 && B >= 1 && J >= 1 && S >= (tail ? 1 : 0),
               WM_ERR_INVALID, "bad args");
    const int n_ctx = ctx->model ? ctx->model->dims.n_text_ctx : 448;
    WM_REQUIRE(Tq >= S + 1 + tail && Tq <= n_ctx, WM_ERR_INVALID, "align: Tq = %d outside [S + %d, %d]", Tq, 1 + tail, n_ctx);
    WM_REQUIRE(medfilt_width >= 1 && medfilt_width <= 31 && medfilt_width % 2 == 1, WM_ERR_INVALID,
               "align: medfilt_width %d must be odd, 1 .. 31", medfilt_width);
    WM_REQUIRE(isfinite(qk_scale), WM_ERR_INVALID, "align: qk_scale must be finite");
    for (int j = 0; j < J; ++j)
        WM_REQUIRE(hl[j] >= 0 && hl[j] < L && hh[j] >= 0 && hh[j] < H, WM_ERR_INVALID, "align: head %d outside the model", j);
    int nmax = 0, mmax = 0;
    for (int b = 0; b < B; ++b) {
        WM_REQUIRE(n_text[b] >= tail - 1 && n_text[b] <= Tq - S - 1 - tail, WM_ERR_INVALID, "align: n_text[%d] = %d outside [%d, %d]", b,
                   n_text[b], tail - 1, Tq - S - 1 - tail);
        WM_REQUIRE(tail || n_text[b] < 0 || S + n_text[b] + 1 >= 2, WM_ERR_INVALID, "align: chunk %d has one decoder row (no spread over rows)", b);
        WM_REQUIRE(n_frames[b] >= 2 && n_frames[b] <= WM_N_FRAMES, WM_ERR_INVALID, "align: n_frames[%d] = %d outside [2, %d]",
                   b, n_frames[b], WM_N_FRAMES);
        nmax = n_text[b] > nmax ? n_text[b] : nmax;
        mmax = n_frames[b] / 2 > mmax ? n_frames[b] / 2 : mmax;
    }
    const int n_ld = Tq - S - tail;
    const size_t head = (size_t)1500 * 64;
    // the cross-K/V cache [L][2][B][H][1500][64]: keys rounded as to_bf16 rounds, V halves NaN, frames >= M a large key
    std::vector<bf16_t> kv((size_t)L * 2 * B * H * head, (bf16_t)0x7fc0);
    for (int l = 0; l < L; ++l)
        for (int b = 0; b < B; ++b)
            for (int h = 0; h < H; ++h) {
                const float *src = keys + (((size_t)l * B + b) * H + h) * head;
                bf16_t *dst = kv.data() + (((size_t)l * 2 * B + b) * H + h) * head;
                const size_t live = (size_t)(n_frames[b] / 2) * 64;
                for (size_t i = 0; i < head; ++i) dst[i] = i < live ? f2bf(src[i]) : (bf16_t)0x4700;   // 32768
            }
    std::vector<int32_t> ints((size_t)2 * B + 2 * J);
    for (int b = 0; b < B; ++b) { ints[b] = n_text[b]; ints[B + b] = n_frames[b]; }
    for (int j = 0; j < J; ++j) { ints[2 * B + j] = hl[j]; ints[2 * B + J + j] = hh[j]; }
    const uint32_t sentinel = 0x7fc0deadu;
    std::vector<uint32_t> x0((size_t)B * n_ld * 1500, sentinel);
    DevPool pool;
    hipStream_t s = ctx->stream;
    WmAlignDev a;
    const int *di;
    WM_TRY(pool.get(&a.q, q, (size_t)B * Tq * J * 64 * 4, s));
    WM_TRY(pool.get(&a.xkv, kv.data(), kv.size() * 2, s));
    WM_TRY(pool.get(&di, ints.data(), ints.size() * 4, s));
    WM_TRY(pool.get(&a.rowst, nullptr, (size_t)B * J * Tq * 2 * 4, s));
    WM_TRY(pool.get(&a.colst, nullptr, (size_t)B * J * 1500 * 2 * 4, s));
    WM_TRY(pool.get(&a.x, x0.data(), x0.size() * 4, s));
    a.n_text = di; a.n_frames = di + B; a.hl = di + 2 * B; a.hh = di + 2 * B + J;
    a.B = B; a.H = H; a.Tq = Tq; a.J = J; a.S = S; a.n_ld = n_ld;
    a.sc = 0.125f * qk_scale * 1.44269504088896340736f;   // as wm_align
    a.half = medfilt_width / 2;
    if (!tail) { a.tail = 0; a.n_min = 0; }
    WM_TRY(wm_align_matrix(ctx, a, nmax, mmax));
    WM_HIP(hipMemcpyAsync(x, a.x, x0.size() * 4, hipMemcpyDeviceToHost, s));
    if (col_stats) WM_HIP(hipMemcpyAsync(col_stats, a.colst, (size_t)B * J * 1500 * 2 * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

extern "C" int wmdbg_align_matrix(wm_ctx *ctx, const float *q, const float *keys, int L, int H, int B, int Tq, int J,
                                  const int32_t *hl, const int32_t *hh, int S, const int32_t *n_text, const int32_t *n_frames,
                                  int medfilt_width, float qk_scale, float *x, float *col_stats) {
    return align_matrix_hook(ctx, q, keys, L, H, B, Tq, J, hl, hh, S, n_text, n_frames, medfilt_width, qk_scale, x, col_stats, 1);
}

extern "C" int wmdbg_align_matrix_rows(wm_ctx *ctx, const float *q, const float *keys, int L, int H, int B, int Tq, int J,
                                       const int32_t *hl, const int32_t *hh, int S, const int32_t *n_text, const int32_t *n_frames,
                                       int medfilt_width, float qk_scale, float *x, float *col_stats, int tail_rows) {
    WM_REQUIRE(tail_rows == 0 || tail_rows == 1, WM_ERR_INVALID, "align: tail_rows %d is neither 0 nor 1", tail_rows);
    return align_matrix_hook(ctx, q, keys, L, H, B, Tq, J, hl, hh, S, n_text, n_frames, medfilt_width, qk_scale, x, col_stats, tail_rows);
}

extern "C" int wmdbg_align_token_prob(wm_ctx *ctx, const float *logits, int B, int V, int ldo, const int32_t *tok, int eot,
                                      float *prob) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(logits && tok && prob && B >= 1 && V >= 1 && ldo >= V && eot >= 1 && eot <= V, WM_ERR_INVALID, "bad args");
    for (int b = 0; b < B; ++b)
        WM_REQUIRE(tok[b] >= 0 && tok[b] < eot, WM_ERR_INVALID, "align: token %d of row %d is not below eot %d", tok[b], b, eot);
    // one decode position (pos 0, S = 0) with one text token per row: the token is seq[pos + 1][b]
    std::vector<int32_t> ints((size_t)3 * B + 1, 0);
    for (int b = 0; b < B; ++b) { ints[B + b] = tok[b]; ints[2 * B + b] = 1; }
    DevPool pool;
    hipStream_t s = ctx->stream;
    const float *dl;
    const int *seq;
    float *dp;
    WM_TRY(pool.get(&dl, logits, (size_t)B * ldo * 4, s));
    WM_TRY(pool.get(&seq, ints.data(), ints.size() * 4, s));
    WM_TRY(pool.get(&dp, nullptr, (size_t)B * 4, s));
    const int *n_text = seq + 2 * B, *pos = seq + 3 * B;
    WM_TRY(wm_align_token_prob(ctx, dl, ldo, seq, pos, B, 0, eot, n_text, dp, 1));
    WM_HIP(hipMemcpyAsync(prob, dp, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

// ------------------------------------------------------------------ beam search ----
extern "C" int wmdbg_beam_select(int N, int n_from, int32_t eot, int32_t pad, int room, const float *sum, const int32_t *list_n,
                                 const int32_t *list_tok, const float *list_lp, int32_t *n_next, int32_t *src, int32_t *tok,
                                 float *lp, float *new_sum, int32_t *n_fin, int32_t *fin_src, float *fin_lp, float *fin_sum) {
    WM_REQUIRE(N >= 1 && N <= WM_MAX_BEAM && n_from >= 1 && n_from <= N, WM_ERR_INVALID, "beam_select: N 1..%d, n_from 1..N", WM_MAX_BEAM);
    WM_REQUIRE(sum && list_n && list_tok && list_lp && n_next && src && tok && lp && new_sum && n_fin && fin_src && fin_lp && fin_sum,
               WM_ERR_INVALID, "beam_select: null pointer");
    for (int j = 0; j < N; ++j)
        WM_REQUIRE(list_n[j] >= 0 && list_n[j] <= WM_BEAM_LIST, WM_ERR_INVALID, "beam_select: list_n[%d] = %d", j, list_n[j]);
    WmBeamStep st;
    wm_beam_select(N, n_from, eot, pad, room, sum, list_n, list_tok, list_lp, &st);
    *n_next = st.n_next;
    *n_fin = st.n_fin;
    for (int k = 0; k < N; ++k) { src[k] = st.src[k]; tok[k] = st.tok[k]; lp[k] = st.lp[k]; new_sum[k] = st.sum[k]; }
    for (int f = 0; f < st.n_fin; ++f) { fin_src[f] = st.fin_src[f]; fin_lp[f] = st.fin_lp[f]; fin_sum[f] = st.fin_sum[f]; }
    return WM_OK;
}

extern "C" double wmdbg_rank_score(double sum, int n_text, float length_penalty) { return wm_rank_score(sum, n_text, length_penalty); }

extern "C" int wmdbg_beam_fill_order(int N, const float *sum, int32_t *order_out) {
    if (N < 1 || N > WM_MAX_BEAM || !sum || !order_out) return -1;
    return wm_beam_fill_order(N, sum, order_out);
}

// The partials a DE_LOGITS_X launch leaves for a row, restated on the host: per 16-id tile the best allowed text / timestamp
// key and the (max, sum exp) of the allowed text ids / timestamps.
static unsigned long long host_key(float v, int n) {
    uint32_t u;
    memcpy(&u, &v, 4);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)n);
}

// (wmdbg_beam_topk and wmdbg_sample_truncate stage the same rows)
struct HostPartials {
    int vpad, nt, mw;
    std::vector<unsigned> mask;                  // [2][mw]: the every-position bitmap, then room for the first-position one
    std::vector<float> lg, txt, tsl;             // logits [rows][vpad]; text and timestamp (max, sum exp) [rows][nt][2]
    std::vector<unsigned long long> kt, ks;      // best allowed text / timestamp key [rows][nt]
};
static int host_row_partials(const char *who, const float *logits, int rows, int V, const int32_t *suppress, int n_suppress,
                             const int32_t *rng, HostPartials *out) {
    HostPartials &h = *out;
    const int vpad = (V + 15) / 16 * 16, nt = vpad / 16, mw = (vpad + 31) / 32;
    h.vpad = vpad; h.nt = nt; h.mw = mw;
    std::vector<unsigned> &mask = h.mask;
    mask.assign((size_t)2 * mw, 0u);
    for (int i = 0; i < n_suppress; ++i) {
        WM_REQUIRE(suppress[i] >= 0 && suppress[i] < V, WM_ERR_INVALID, "%s: suppressed id %d", who, suppress[i]);
        mask[suppress[i] >> 5] |= 1u << (suppress[i] & 31);
    }
    std::vector<float> &lg = h.lg, &txt = h.txt, &tsl = h.tsl;
    std::vector<unsigned long long> &kt = h.kt, &ks = h.ks;
    lg.assign((size_t)rows * vpad, 0.f); txt.assign((size_t)rows * nt * 2, 0.f); tsl.assign((size_t)rows * nt * 2, 0.f);
    kt.assign((size_t)rows * nt, 0ull); ks.assign((size_t)rows * nt, 0ull);
    for (int b = 0; b < rows; ++b) {
        memcpy(&lg[(size_t)b * vpad], logits + (size_t)b * V, (size_t)V * 4);
        const int32_t *r = rng ? rng + b * 4 : nullptr;
        for (int t = 0; t < nt; ++t) {
            float mx = -1e30f, mt = -1e30f;
            for (int pass = 0; pass < 2; ++pass) {
                float se = 0.f, st = 0.f;
                for (int n = t * 16; n < t * 16 + 16 && n < V; ++n) {
                    if ((mask[n >> 5] >> (n & 31)) & 1u) continue;
                    const float v = logits[(size_t)b * V + n];
                    const bool in_text = r ? (n >= r[0] && n < r[1]) : true, in_ts = r && n >= r[2] && n < r[3];
                    if (pass == 0) {
                        if (in_text) { mx = std::max(mx, v); kt[(size_t)b * nt + t] = std::max(kt[(size_t)b * nt + t], host_key(v, n)); }
                        if (in_ts) { mt = std::max(mt, v); ks[(size_t)b * nt + t] = std::max(ks[(size_t)b * nt + t], host_key(v, n)); }
                    } else {
                        if (in_text) se += expf(v - mx);
                        if (in_ts) st += expf(v - mt);
                    }
                }
                if (pass == 1) {
                    txt[((size_t)b * nt + t) * 2] = mx; txt[((size_t)b * nt + t) * 2 + 1] = se;
                    tsl[((size_t)b * nt + t) * 2] = mt; tsl[((size_t)b * nt + t) * 2 + 1] = st;
                }
            }
        }
    }
    return WM_OK;
}

extern "C" int wmdbg_beam_topk(wm_ctx *ctx, const float *logits, int rows, int V, int N, const int32_t *suppress, int n_suppress,
                               const int32_t *rng, int32_t ts_begin, int32_t *list_n, int32_t *list_tok, float *list_lp) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(logits && list_n && list_tok && list_lp && rows >= 1 && rows <= WM_DEC_MAXB && V >= 16 && N >= 1 && N <= WM_MAX_BEAM &&
                   rows % N == 0 && n_suppress >= 0 && (n_suppress == 0 || suppress) && (!rng || (ts_begin >= 0 && ts_begin <= V)),
               WM_ERR_INVALID, "beam_topk: bad args");
    HostPartials hp;
    WM_TRY(host_row_partials("beam_topk", logits, rows, V, suppress, n_suppress, rng, &hp));
    const int vpad = hp.vpad, mw = hp.mw;
    const std::vector<unsigned> &mask = hp.mask;
    const std::vector<float> &lg = hp.lg, &txt = hp.txt, &tsl = hp.tsl;
    const std::vector<unsigned long long> &kt = hp.kt, &ks = hp.ks;
    const int L = WM_MAX_BEAM + 1;
    const int32_t ints[2] = {0, 0};   // pos, then the beam parameters are not read by this kernel
    WmXPar xp;
    memset(&xp, 0, sizeof(xp));
    xp.sot_pos = -1;
    DevPool pool;
    hipStream_t s = ctx->stream;
    WmTsDev ts;
    memset(&ts, 0, sizeof(ts));
    WmXDev xd;
    memset(&xd, 0, sizeof(xd));
    WmBeamDev bm;
    memset(&bm, 0, sizeof(bm));
    bm.N = N;
    const float *dlg;
    float *dtsl;
    unsigned long long *dkt;
    unsigned long long *dks;
    const unsigned *dmask;
    const int *dpos;
    WM_TRY(pool.get(&dlg, lg.data(), lg.size() * 4, s));
    WM_TRY(pool.get(&xd.txt, txt.data(), txt.size() * 4, s));
    WM_TRY(pool.get(&dtsl, tsl.data(), tsl.size() * 4, s));
    WM_TRY(pool.get(&dkt, kt.data(), kt.size() * 8, s));
    WM_TRY(pool.get(&dks, ks.data(), ks.size() * 8, s));
    WM_TRY(pool.get(&dmask, mask.data(), mask.size() * 4, s));
    if (rng) {
        WM_TRY(pool.get(&ts.rng, rng, (size_t)rows * 16, s));
        ts.key_ts = dks; ts.lse = dtsl; ts.ts_begin = ts_begin; ts.n_vocab = V;
    }
    WM_TRY(pool.get(&dpos, ints, 8, s));
    WM_TRY(pool.get(&xd.par, &xp, sizeof(xp), s));
    WM_TRY(pool.get(&bm.sum, nullptr, (size_t)rows * 4, s));
    WM_TRY(pool.get(&bm.wdone, nullptr, (size_t)rows * 4, s));
    WM_TRY(pool.get(&bm.list_n, nullptr, (size_t)rows * 4, s));
    WM_TRY(pool.get(&bm.list_tok, nullptr, (size_t)rows * L * 4, s));
    WM_TRY(pool.get(&bm.list_lp, nullptr, (size_t)rows * L * 4, s));
    // n_prompt 2 at position 0: not the first generated token, so the every-position bitmap applies
    WM_TRY(wm_beam_topk(ctx, WmStoredRows{dlg, vpad, V, dkt, rows, ts, xd, dmask, mw, 2, dpos, WmStopDev{}, nullptr, 0}, bm));
    WM_HIP(hipMemcpyAsync(list_n, bm.list_n, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(list_tok, bm.list_tok, (size_t)rows * L * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(list_lp, bm.list_lp, (size_t)rows * L * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

// The alternatives kernel alone on host-given rows at generated index 0 (n_prompt 2, position 1): the partials restated on the
// host as for wmdbg_beam_topk (host_row_partials), so the two kernels see the same normaliser.  The outputs are uploaded as the
// caller filled them and downloaded whole: a sentinel shows what the kernel wrote.
extern "C" int wmdbg_alternatives(wm_ctx *ctx, const float *logits, int rows, int V, int n, const int32_t *suppress, int n_suppress,
                                  const int32_t *rng, int32_t ts_begin, int32_t *counts, int32_t *tokens, float *logprobs,
                                  float *entropy) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(logits && tokens && logprobs && rows >= 1 && rows <= WM_DEC_MAXB && V >= 16 && n >= 1 && n <= WM_MAX_ALTERNATIVES &&
                   n_suppress >= 0 && (n_suppress == 0 || suppress) && (!rng || (ts_begin >= 0 && ts_begin <= V)),
               WM_ERR_INVALID, "alternatives: bad args");
    HostPartials hp;
    WM_TRY(host_row_partials("alternatives", logits, rows, V, suppress, n_suppress, rng, &hp));
    std::copy(hp.mask.begin(), hp.mask.begin() + hp.mw, hp.mask.begin() + hp.mw);   // (gi 0 reads the first-position bitmap)
    const int32_t pos = 1;
    WmXPar xp;
    memset(&xp, 0, sizeof(xp));
    xp.sot_pos = -1; xp.n_prompt = 2;
    DevPool pool;
    hipStream_t s = ctx->stream;
    WmTsDev ts;
    memset(&ts, 0, sizeof(ts));
    WmXDev xd;
    memset(&xd, 0, sizeof(xd));
    WmAltPar ap;
    memset(&ap, 0, sizeof(ap));
    ap.n = n; ap.max_new = 1;
    const float *dlg;
    unsigned long long *dkt;
    const unsigned *dmask;
    const int *dpos;
    const WmAltPar *dpar;
    WM_TRY(pool.get(&dlg, hp.lg.data(), hp.lg.size() * 4, s));
    WM_TRY(pool.get(&xd.txt, hp.txt.data(), hp.txt.size() * 4, s));
    WM_TRY(pool.get(&dkt, hp.kt.data(), hp.kt.size() * 8, s));
    WM_TRY(pool.get(&dmask, hp.mask.data(), hp.mask.size() * 4, s));
    if (rng) {
        WM_TRY(pool.get(&ts.rng, rng, (size_t)rows * 16, s));
        WM_TRY(pool.get(&ts.key_ts, hp.ks.data(), hp.ks.size() * 8, s));
        WM_TRY(pool.get(&ts.lse, hp.tsl.data(), hp.tsl.size() * 4, s));
        ts.ts_begin = ts_begin; ts.n_vocab = V;
    }
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&xd.par, &xp, sizeof(xp), s));
    WM_TRY(pool.get(&ap.tok, tokens, (size_t)rows * n * 4, s));
    WM_TRY(pool.get(&ap.lp, logprobs, (size_t)rows * n * 4, s));
    if (counts) WM_TRY(pool.get(&ap.cnt, counts, (size_t)rows * 4, s));
    if (entropy) WM_TRY(pool.get(&ap.ent, entropy, (size_t)rows * 4, s));
    WM_TRY(pool.get(&dpar, &ap, sizeof(ap), s));
    WM_TRY(wm_alternatives(ctx, WmStoredRows{dlg, hp.vpad, V, dkt, rows, ts, xd, dmask, hp.mw, 2, dpos, WmStopDev{}, nullptr, 0}, dpar));
    WM_HIP(hipMemcpyAsync(tokens, ap.tok, (size_t)rows * n * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(logprobs, ap.lp, (size_t)rows * n * 4, hipMemcpyDeviceToHost, s));
    if (counts) WM_HIP(hipMemcpyAsync(counts, ap.cnt, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
    if (entropy) WM_HIP(hipMemcpyAsync(entropy, ap.ent, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

// The truncation kernel alone on host-given rows at generated index gi (n_prompt 2, position gi + 1): the partials restated on
// the host as for wmdbg_beam_topk, the row's keys and winner values in scratch.
extern "C" int wmdbg_sample_truncate(wm_ctx *ctx, const float *logits, int rows, int V, const int32_t *suppress, int n_suppress,
                                     const int32_t *rng, int32_t ts_begin, float temperature, uint64_t seed, const uint32_t *sample_ids,
                                     int gi, int top_k, float top_p, float min_p, int32_t *kept_n, int32_t *cut_tok, int32_t *tok) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(logits && sample_ids && kept_n && cut_tok && tok && rows >= 1 && rows <= WM_DEC_MAXB && V >= 16 && n_suppress >= 0 &&
                   (n_suppress == 0 || suppress) && (!rng || (ts_begin >= 0 && ts_begin <= V)) && gi >= 0,
               WM_ERR_INVALID, "sample_truncate: bad args");
    WM_REQUIRE(std::isfinite(temperature) && temperature > 0.f && top_k >= 0 && top_p > 0.f && top_p <= 1.f && min_p >= 0.f && min_p < 1.f,
               WM_ERR_INVALID, "sample_truncate: temperature > 0, top_k >= 0, top_p in (0, 1], min_p in [0, 1)");
    HostPartials hp;
    WM_TRY(host_row_partials("sample_truncate", logits, rows, V, suppress, n_suppress, rng, &hp));
    std::copy(hp.mask.begin(), hp.mask.begin() + hp.mw, hp.mask.begin() + hp.mw);   // (gi 0 reads the first-position bitmap)
    const int32_t pos = gi + 1;
    WmXPar xp;
    memset(&xp, 0, sizeof(xp));
    xp.key0 = (unsigned)seed; xp.key1 = (unsigned)(seed >> 32);
    xp.sample = 1; xp.inv_T = (float)(1.0 / (double)temperature);
    xp.sot_pos = -1; xp.n_prompt = 2; xp.ids_on = 1; xp.n_cand = 1;
    const WmSampPar spar = {top_k, top_p, min_p};
    DevPool pool;
    hipStream_t s = ctx->stream;
    WmTsDev ts;
    memset(&ts, 0, sizeof(ts));
    WmXDev xd;
    memset(&xd, 0, sizeof(xd));
    const size_t nt = (size_t)rows * hp.nt;
    const float *dlg;
    unsigned long long *dkt;
    const unsigned *dmask;
    const int *dpos;
    const WmSampPar *dpar;
    int *ddbg;
    WM_TRY(pool.get(&dlg, hp.lg.data(), hp.lg.size() * 4, s));
    WM_TRY(pool.get(&xd.txt, hp.txt.data(), hp.txt.size() * 4, s));
    WM_TRY(pool.get(&xd.win, nullptr, nt * 8, s));
    WM_TRY(pool.get(&xd.ids, sample_ids, (size_t)rows * 4, s));
    WM_TRY(pool.get(&dkt, hp.kt.data(), hp.kt.size() * 8, s));
    WM_TRY(pool.get(&dmask, hp.mask.data(), hp.mask.size() * 4, s));
    if (rng) {
        WM_TRY(pool.get(&ts.rng, rng, (size_t)rows * 16, s));
        WM_TRY(pool.get(&ts.key_ts, hp.ks.data(), hp.ks.size() * 8, s));
        WM_TRY(pool.get(&ts.lse, hp.tsl.data(), hp.tsl.size() * 4, s));
        ts.ts_begin = ts_begin; ts.n_vocab = V;
    }
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&xd.par, &xp, sizeof(xp), s));
    WM_TRY(pool.get(&dpar, &spar, sizeof(spar), s));
    WM_TRY(pool.get(&ddbg, nullptr, (size_t)rows * 12, s, 0xff));
    WM_TRY(wm_sample_truncate(ctx, WmStoredRows{dlg, hp.vpad, V, dkt, rows, ts, xd, dmask, hp.mw, 2, dpos, WmStopDev{}, nullptr, 0}, dpar, ddbg));
    std::vector<int32_t> out((size_t)rows * 3);
    WM_HIP(hipMemcpyAsync(out.data(), ddbg, out.size() * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < rows; ++b) { kept_n[b] = out[b * 3]; cut_tok[b] = out[b * 3 + 1]; tok[b] = out[b * 3 + 2]; }
    return WM_OK;
}

extern "C" int wmdbg_beam_reorder(wm_ctx *ctx, uint16_t *cache, int L2, int rows, int H, int T, int N, int pos, int n_prompt,
                                  const int32_t *src, const int32_t *wdone, int32_t *seq, float *logprob) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(cache && src && wdone && seq && logprob && L2 >= 1 && H >= 1 && T >= 1 && N >= 1 && N <= WM_MAX_BEAM && rows >= 1 &&
                   rows <= WM_DEC_MAXB && rows % N == 0 && pos >= 0 && pos < T && n_prompt >= 1 && n_prompt <= pos + 1,
               WM_ERR_INVALID, "beam_reorder: bad args");
    for (int b = 0; b < rows; ++b) WM_REQUIRE(src[b] >= 0 && src[b] < N, WM_ERR_INVALID, "beam_reorder: src[%d] = %d", b, src[b]);
    const size_t nc = (size_t)L2 * rows * H * T * 64;
    const int after = pos + 1;   // the kernel runs behind the position advance
    DevPool pool;
    hipStream_t s = ctx->stream;
    WmBeamDev bm;
    memset(&bm, 0, sizeof(bm));
    bm.N = N;
    bf16_t *dc;
    int *dseq;
    float *dlp;
    const int *dpos;
    WM_TRY(pool.get(&dc, cache, nc * 2, s));
    WM_TRY(pool.get(&bm.src, src, (size_t)rows * 4, s));
    WM_TRY(pool.get(&bm.wdone, wdone, (size_t)(rows / N) * 4, s));
    WM_TRY(pool.get(&dseq, seq, (size_t)T * rows * 4, s));
    WM_TRY(pool.get(&dlp, logprob, (size_t)T * rows * 4, s));
    WM_TRY(pool.get(&dpos, &after, 4, s));
    WM_TRY(wm_beam_reorder(ctx, dc, L2, rows, H, T, dpos, n_prompt, dseq, dlp, bm));
    WM_HIP(hipMemcpyAsync(cache, dc, nc * 2, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(seq, dseq, (size_t)T * rows * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(logprob, dlp, (size_t)T * rows * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

extern "C" int wmdbg_beam_step_layout(int32_t *out4) {
    if (!out4) return WM_ERR_INVALID;
    out4[0] = (int32_t)sizeof(wmdbg_beam_io); out4[1] = (int32_t)offsetof(wmdbg_beam_io, ts_par);
    out4[2] = (int32_t)offsetof(wmdbg_beam_io, budget); out4[3] = (int32_t)offsetof(wmdbg_beam_io, x_next);
    return WM_OK;
}
// The select kernel alone (beam.hip) on the caller's state.  Every buffer goes to the device whole and comes back whole, so the
// caller's sentinels show what the kernel left alone; nothing is launched when the kernel could leave a buffer.
extern "C" int wmdbg_beam_step(wm_ctx *ctx, wmdbg_beam_io *io) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(io && io->budget && io->sum && io->list_n && io->list_tok && io->list_lp && io->src && io->wdone && io->wsteps &&
                   io->fin_n && io->fin_len && io->fin_sum && io->fin_src && io->fin_tok && io->fin_lp && io->seq && io->logprob &&
                   io->hist && io->rng && io->done && io->live_rows && io->n_live && io->emb && io->pemb && io->x_next &&
                   io->xb_next && io->stats_next && io->mean_next,
               WM_ERR_INVALID, "wmdbg_beam_step: null pointer");
    const int C = io->C, N = io->N, cap = io->cap, n_ctx = io->n_ctx, pos = io->pos, n_prompt = io->n_prompt, d = io->d, V = io->n_vocab;
    WM_REQUIRE(C >= 1 && N >= 1 && N <= WM_MAX_BEAM && cap >= C && cap <= 2 * WM_DEC_MAXB, WM_ERR_INVALID,
               "wmdbg_beam_step: bad group: C %d, N %d (1 .. %d), cap %d", C, N, WM_MAX_BEAM, cap);
    WM_REQUIRE(C * N <= WM_DEC_MAXB, WM_ERR_INVALID, "wmdbg_beam_step: %d rows are more than %d", C * N, WM_DEC_MAXB);
    WM_REQUIRE(n_prompt >= 1 && n_ctx >= 1 && n_ctx <= 4096 && V >= 1 && io->max_new >= 1 && io->max_new <= 4096, WM_ERR_INVALID,
               "wmdbg_beam_step: bad geometry");
    WM_REQUIRE(pos >= n_prompt - 1 && pos < n_ctx, WM_ERR_INVALID, "wmdbg_beam_step: position %d outside [n_prompt - 1, n_ctx)", pos);
    const int gi = pos + 1 - n_prompt, rows = C * N;
    WM_REQUIRE(gi < io->max_new, WM_ERR_INVALID, "wmdbg_beam_step: generated index %d is not below max_new %d", gi, io->max_new);
    WM_REQUIRE(io->max_cand >= 1 && io->max_cand <= WM_MAX_BEAM_HYPS, WM_ERR_INVALID, "wmdbg_beam_step: max_cand %d outside 1 .. %d",
               io->max_cand, WM_MAX_BEAM_HYPS);
    WM_REQUIRE(d >= 64 && d % 64 == 0 && d <= 1280, WM_ERR_INVALID, "wmdbg_beam_step: d %d is not a multiple of 64 in 64 .. 1280", d);
    WM_REQUIRE(io->pad >= 0 && io->pad < V && io->eot < V, WM_ERR_INVALID, "wmdbg_beam_step: pad %d or eot %d outside the vocabulary",
               io->pad, io->eot);
    for (int w = 0; w < C; ++w)
        WM_REQUIRE(io->fin_n[w] >= 0 && io->fin_n[w] <= io->max_cand, WM_ERR_INVALID, "wmdbg_beam_step: fin_n[%d] = %d outside 0 .. max_cand",
                   w, io->fin_n[w]);
    for (int b = 0; b < rows; ++b) {
        WM_REQUIRE(io->list_n[b] >= 0 && io->list_n[b] <= N + 1, WM_ERR_INVALID, "wmdbg_beam_step: list_n[%d] = %d outside 0 .. N + 1", b,
                   io->list_n[b]);
        for (int e = 0; e < io->list_n[b]; ++e) {
            const int t = io->list_tok[b * WM_BEAM_LIST + e];
            WM_REQUIRE(t >= 0 && t < V, WM_ERR_INVALID, "wmdbg_beam_step: list token %d of row %d outside the vocabulary", t, b);
        }
        if (io->off) WM_REQUIRE(io->off[b] >= 0, WM_ERR_INVALID, "wmdbg_beam_step: off[%d] = %d is negative", b, io->off[b]);
    }
    hipStream_t s = ctx->stream;
    const size_t nr = (size_t)cap * N, nh = (size_t)cap * WM_MAX_BEAM_HYPS, rpad = (nr + 15) / 16 * 16, st_words = rpad / 16 * 2 * d;
    std::vector<bf16_t> e16;
    tile_bf16(io->emb, (size_t)V, (size_t)d, e16);
    const std::vector<uint32_t> nan32(std::max(nr * d, st_words), WMDBG_SENTINEL_F32);
    const std::vector<bf16_t> nan16(rpad * d, (bf16_t)WMDBG_SENTINEL_BF16);
    std::vector<float> stn(st_words);
    const WmBeamPar par{io->max_cand, io->max_new, io->eot, io->pad};
    WmXPar xp;
    memset(&xp, 0, sizeof(xp));
    xp.sot_pos = -1; xp.n_prompt = n_prompt; xp.n_cand = N;
    DevPool pool;
    // every in / out buffer once: host pointer, bytes, device pointer
    struct Buf { void *h; size_t bytes; void *d; };
    Buf bufs[] = {{io->sum, nr * 4, nullptr},          {io->list_n, nr * 4, nullptr},       {io->list_tok, nr * WM_BEAM_LIST * 4, nullptr},
                  {io->list_lp, nr * WM_BEAM_LIST * 4, nullptr}, {io->src, nr * 4, nullptr}, {io->wdone, (size_t)cap * 4, nullptr},
                  {io->wsteps, (size_t)cap * 4, nullptr}, {io->fin_n, (size_t)cap * 4, nullptr}, {io->fin_len, nh * 4, nullptr},
                  {io->fin_sum, nh * 4, nullptr},      {io->fin_src, nh * 4, nullptr},      {io->fin_tok, nh * n_ctx * 4, nullptr},
                  {io->fin_lp, nh * n_ctx * 4, nullptr}, {io->seq, (size_t)(n_ctx + 1) * rows * 4, nullptr},
                  {io->logprob, (size_t)io->max_new * rows * 4, nullptr}, {io->hist, nr * 16, nullptr}, {io->rng, nr * 16, nullptr},
                  {io->done, nr * 4, nullptr},         {io->live_rows, nr * 4, nullptr},    {io->n_live, 4, nullptr},
                  {io->anc, io->anc ? (size_t)io->max_new * rows * 4 : 0, nullptr}};
    for (Buf &b : bufs)
        if (b.h) WM_TRY(pool.get(&b.d, b.h, b.bytes, s));
    auto dev = [&](const void *h) {
        for (const Buf &b : bufs)
            if (b.h == h) return b.d;
        return (void *)nullptr;
    };
    const int *d_bud, *d_off = nullptr;
    int *d_pos;
    const bf16_t *d_emb;
    const float *d_pemb;
    float *d_x, *d_st, *d_mean;
    bf16_t *d_xb;
    WM_TRY(pool.get(&d_bud, io->budget, (size_t)cap * 4, s));
    if (io->off) WM_TRY(pool.get(&d_off, io->off, (size_t)rows * 4, s));
    WM_TRY(pool.get(&d_pos, &pos, 4, s));
    WM_TRY(pool.get(&d_emb, e16.data(), e16.size() * 2, s));
    WM_TRY(pool.get(&d_pemb, io->pemb, (size_t)n_ctx * d * 4, s));
    WM_TRY(pool.get(&d_x, nan32.data(), nr * d * 4, s));
    WM_TRY(pool.get(&d_xb, nan16.data(), nan16.size() * 2, s));
    WM_TRY(pool.get(&d_st, nan32.data(), st_words * 4, s));
    WM_TRY(pool.get(&d_mean, nan32.data(), nr * 4, s));
    WmBeamDev bm;
    memset(&bm, 0, sizeof(bm));
    WM_TRY(pool.get(&bm.par, &par, sizeof(par), s));
    bm.N = N; bm.n_ctx = n_ctx; bm.budget = d_bud;
    bm.sum = (float *)dev(io->sum); bm.src = (int *)dev(io->src); bm.list_n = (int *)dev(io->list_n);
    bm.list_tok = (int *)dev(io->list_tok); bm.list_lp = (float *)dev(io->list_lp);
    bm.wdone = (int *)dev(io->wdone); bm.wsteps = (int *)dev(io->wsteps); bm.fin_n = (int *)dev(io->fin_n);
    bm.fin_len = (int *)dev(io->fin_len); bm.fin_sum = (float *)dev(io->fin_sum);
    bm.fin_tok = (int *)dev(io->fin_tok); bm.fin_lp = (float *)dev(io->fin_lp);
    if (io->anc) { bm.anc = (int *)dev(io->anc); bm.fin_src = (int *)dev(io->fin_src); }   // an aligned group (wm_model_beam_dev)
    WmTsDev ts;
    memset(&ts, 0, sizeof(ts));
    if (io->ts_on) {
        ts.hist = (int *)dev(io->hist); ts.rng = (int *)dev(io->rng);
        ts.ts_begin = io->ts_par[0]; ts.eot = io->ts_par[1]; ts.n_vocab = io->ts_par[2]; ts.max_initial = io->ts_par[3];
    }
    WmStopDev sp;
    memset(&sp, 0, sizeof(sp));
    if (io->stop_on) {
        sp.done = (int *)dev(io->done); sp.live_rows = (int *)dev(io->live_rows); sp.n_live = (int *)dev(io->n_live);
        sp.eot = io->eot; sp.pad_tok = io->pad;
    }
    WmXDev xd;
    memset(&xd, 0, sizeof(xd));
    WM_TRY(pool.get(&xd.par, &xp, sizeof(xp), s));
    xd.logprob = (float *)dev(io->logprob);
    WM_TRY(wm_beam_select_step(ctx, rows, (int *)dev(io->seq), d_pos, n_prompt, WmEmbedDev{d_emb, d_pemb, d, d_x, d_xb, d_st, d_mean}, ts, sp,
                               xd, d_off, bm));
    for (const Buf &b : bufs)
        if (b.h) WM_HIP(hipMemcpyAsync(b.h, b.d, b.bytes, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(&io->pos_out, d_pos, 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(io->x_next, d_x, nr * d * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(io->mean_next, d_mean, nr * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(stn.data(), d_st, st_words * 4, hipMemcpyDeviceToHost, s));
    WM_TRY(down_tiled_bf16(d_xb, nr, (size_t)d, io->xb_next, s));   // (synchronises the stream)
    io->stats_tail_nonzero = 0;
    for (size_t b = 0; b < nr; ++b) {   // summed as wmdbg_decode_close sums them; the tail: words behind part 0 that are not zero bits
        stats_sum(stn.data(), d, (int)b, io->stats_next + b * 2);
        for (int part = 1; part < d / 16 && b < (size_t)rows; ++part)
            for (int c = 0; c < 2; ++c) {
                uint32_t u;
                memcpy(&u, &stn[stat_at(d, b, part, c)], 4);
                if (u != 0u) ++io->stats_tail_nonzero;
            }
    }
    return WM_OK;
}

// ------------------------------------------------------------------ window sets: the copy kernel ----
extern "C" int wmdbg_xkv_rows(wm_ctx *ctx, uint16_t *group, int group_rows, uint16_t *store, int64_t store_rows, const int32_t *rows,
                              int n_rows, int L, int H, int to_store) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(group && store && rows && L >= 1 && H >= 1 && n_rows >= 1 && n_rows <= group_rows && group_rows <= WM_DEC_MAXB &&
                   store_rows >= 1, WM_ERR_INVALID, "xkv_rows: bad args");
    for (int b = 0; b < n_rows; ++b) {
        WM_REQUIRE(rows[b] >= 0 && rows[b] < store_rows, WM_ERR_INVALID, "xkv_rows: rows[%d] = %d outside [0, %lld)", b, rows[b],
                   (long long)store_rows);
        for (int o = 0; to_store && o < b; ++o)
            WM_REQUIRE(rows[o] != rows[b], WM_ERR_INVALID, "xkv_rows: store row %d named twice", rows[b]);
    }
    DevPool pool;
    hipStream_t s = ctx->stream;
    const int *drows;
    WM_TRY(pool.get(&drows, rows, (size_t)n_rows * 4, s));
    int rc = wm_xkv_rows(ctx, group, group_rows, store, drows, 0, n_rows, 2 * L, (long)H * 1500 * 64, to_store != 0);
    if (hipStreamSynchronize(s) != hipSuccess && rc == WM_OK) {
        wm_set_error("xkv_rows: %s", hipGetErrorString(hipGetLastError()));
        rc = WM_ERR_HIP;
    }
    return rc;
}

// ------------------------------------------------------------------ the decode step's LN-folded GEMV and its close ----
// panel: 0 = the step epilogues; w >= 1 (DE_QKV only) = the panel epilogue DE_QKV_P, caches [ceil(B / w)][n_head][T][64]
static int dec_gemv_ln_run(wm_ctx *ctx, int epi, const float *x, const float *ln_g, const float *ln_b, const float *W,
                           const float *bias, int B, int N, int K, int centre, int n_head, int T, int pos, int panel, float *out_f32,
                           float *out_bf16, float *kcache, float *vcache, float *mean_out, float *Wf, float *c1, float *c2) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(panel == 0 || (epi == DE_QKV && panel >= 1 && panel <= WM_MAX_TEACHER_PANEL && pos + panel <= T), WM_ERR_INVALID,
               "wmdbg_dec_qkv_panel: width 1 .. %d, pos + width <= T", WM_MAX_TEACHER_PANEL);
    WM_REQUIRE(epi == DE_QKV || epi == DE_Q || epi == DE_GELU, WM_ERR_INVALID, "wmdbg_dec_gemv_ln: epilogue %d not exposed", epi);
    WM_REQUIRE(x && ln_g && ln_b && W && mean_out && Wf && c1 && c2, WM_ERR_INVALID, "wmdbg_dec_gemv_ln: null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && N >= 1 && K >= 64 && K % 64 == 0 && K <= 1280, WM_ERR_INVALID,
               "wmdbg_dec_gemv_ln: B 1 .. %d, N >= 1, K a multiple of 64 up to 1280", WM_DEC_MAXB);
    const int d = N / 3;
    if (epi == DE_QKV)
        WM_REQUIRE(N % 3 == 0 && n_head >= 1 && d == n_head * 64 && T >= 1 && pos >= 0 && pos < T && out_f32 && kcache && vcache,
                   WM_ERR_INVALID, "wmdbg_dec_gemv_ln: DE_QKV needs N = 3 * n_head * 64, pos in [0, T) and its three outputs");
    if (epi == DE_Q) WM_REQUIRE(out_f32, WM_ERR_INVALID, "wmdbg_dec_gemv_ln: DE_Q needs out_f32");
    if (epi == DE_GELU) WM_REQUIRE(N % 32 == 0 && out_bf16, WM_ERR_INVALID, "wmdbg_dec_gemv_ln: DE_GELU needs N %% 32 == 0 and out_bf16");
    const size_t Npad = ((size_t)N + 15) / 16 * 16, Bpad = ((size_t)B + 15) / 16 * 16;
    std::vector<bf16_t> w16, x16;
    std::vector<float> st, mean;
    tile_bf16(W, (size_t)N, (size_t)K, w16);
    stage_ln_rows(x, B, K, centre != 0, x16, st, mean);
    const size_t n_f32 = epi == DE_QKV ? (size_t)B * d : epi == DE_Q ? (size_t)B * N : 0;
    const size_t n_b16 = epi == DE_GELU ? Bpad * N : 0, n_cache = epi == DE_QKV ? (size_t)(panel ? (B + panel - 1) / panel : B) * n_head * T * 64 : 0;
    const std::vector<bf16_t> fill16(std::max(n_b16, n_cache), (bf16_t)WMDBG_SENTINEL_BF16);
    const std::vector<uint32_t> fill32((size_t)B, WMDBG_SENTINEL_F32);
    std::vector<bf16_t> wf16(w16.size()), ob16(n_b16), k16(n_cache), v16(n_cache);
    DevPool pool;
    hipStream_t s = ctx->stream;
    DecGemvArgs a;
    memset(&a, 0, sizeof(a));
    a.epi = epi; a.B = B; a.N = N; a.K = K; a.stats_parts = K / 16; a.ldo = N;
    const bf16_t *dW;
    bf16_t *dWf;
    float *dc1, *dc2;
    const float *dg, *db, *dbias = nullptr, *dmin;
    const int *dpos;
    WM_TRY(pool.get(&a.a, x16.data(), x16.size() * 2, s));
    WM_TRY(pool.get(&dW, w16.data(), w16.size() * 2, s));
    WM_TRY(pool.get(&dWf, nullptr, w16.size() * 2, s));
    WM_TRY(pool.get(&dc1, nullptr, Npad * 4, s));
    WM_TRY(pool.get(&dc2, nullptr, Npad * 4, s));
    WM_TRY(pool.get(&dg, ln_g, (size_t)K * 4, s));
    WM_TRY(pool.get(&db, ln_b, (size_t)K * 4, s));
    if (bias) WM_TRY(pool.get(&dbias, bias, (size_t)N * 4, s));
    WM_TRY(pool.get(&a.stats_in, st.data(), st.size() * 4, s));
    WM_TRY(pool.get(&dmin, mean.data(), (size_t)B * 4, s));
    WM_TRY(pool.get(&a.mean_out, fill32.data(), (size_t)B * 4, s));
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    if (n_f32) WM_TRY(pool.get(&a.out_f32, nullptr, n_f32 * 4, s));
    if (n_b16) WM_TRY(pool.get(&a.out_bf16, fill16.data(), n_b16 * 2, s));
    if (n_cache) {
        WM_TRY(pool.get(&a.kcache, fill16.data(), n_cache * 2, s));
        WM_TRY(pool.get(&a.vcache, fill16.data(), n_cache * 2, s));
    }
    WM_TRY(wm_ln_fold(ctx, dW, dg, db, dbias, N, K, dWf, dc1, dc2));
    a.W = dWf; a.c1 = dc1; a.c2 = dc2;
    a.mean_in = centre ? dmin : nullptr;
    if (epi == DE_QKV) { a.pos_ptr = dpos; a.n_ctx = T; a.n_head = n_head; }
    if (panel) { a.epi = DE_QKV_P; a.panel = panel; }
    WM_TRY(wm_dec_gemv(ctx, a));
    WM_HIP(hipMemcpyAsync(wf16.data(), dWf, wf16.size() * 2, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(c1, dc1, Npad * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(c2, dc2, Npad * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(mean_out, a.mean_out, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    if (n_f32) WM_HIP(hipMemcpyAsync(out_f32, a.out_f32, n_f32 * 4, hipMemcpyDeviceToHost, s));
    if (n_b16) WM_HIP(hipMemcpyAsync(ob16.data(), a.out_bf16, n_b16 * 2, hipMemcpyDeviceToHost, s));
    if (n_cache) {
        WM_HIP(hipMemcpyAsync(k16.data(), a.kcache, n_cache * 2, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(v16.data(), a.vcache, n_cache * 2, hipMemcpyDeviceToHost, s));
    }
    WM_HIP(hipStreamSynchronize(s));
    untile_bf16(wf16, Npad, (size_t)K, Wf);
    if (n_b16) untile_bf16(ob16, (size_t)B, (size_t)N, out_bf16);
    if (n_cache) { from_bf16(k16, kcache); from_bf16(v16, vcache); }
    return WM_OK;
}

extern "C" int wmdbg_dec_gemv_ln(wm_ctx *ctx, int epi, const float *x, const float *ln_g, const float *ln_b, const float *W,
                                 const float *bias, int B, int N, int K, int centre, int n_head, int T, int pos, float *out_f32,
                                 float *out_bf16, float *kcache, float *vcache, float *mean_out, float *Wf, float *c1, float *c2) {
    return dec_gemv_ln_run(ctx, epi, x, ln_g, ln_b, W, bias, B, N, K, centre, n_head, T, pos, 0, out_f32, out_bf16, kcache, vcache,
                           mean_out, Wf, c1, c2);
}

// ------------------------------------------------------------------ teacher-forced panels (wm_set_teacher_panel) ----
extern "C" int wmdbg_dec_qkv_panel(wm_ctx *ctx, const float *x, const float *ln_g, const float *ln_b, const float *W,
                                   const float *bias, int C, int w, int N, int K, int n_head, int T, int pos, float *q_out,
                                   float *kcache, float *vcache) {
    WM_REQUIRE(C >= 1 && w >= 1 && C * w <= WM_DEC_MAXB, WM_ERR_INVALID, "wmdbg_dec_qkv_panel: C x w rows outside 1 .. %d", WM_DEC_MAXB);
    const size_t Npad = ((size_t)(N > 0 ? N : 0) + 15) / 16 * 16;
    std::vector<float> mean((size_t)C * w), Wf(Npad * (size_t)(K > 0 ? K : 0)), c1(Npad), c2(Npad);
    return dec_gemv_ln_run(ctx, DE_QKV, x, ln_g, ln_b, W, bias, C * w, N, K, 1, n_head, T, pos, w, q_out, nullptr, kcache, vcache,
                           mean.data(), Wf.data(), c1.data(), c2.data());
}

// (off: null = the uniform panel launch; else the windows' offsets [C] of a ragged group's prompt panel)
static int dec_self_attention_panel(wm_ctx *ctx, const float *q, const float *k, const float *v, int C, int w, int H, int T, int pos,
                                    const int32_t *off, int out_rows, float *out) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(q && k && v && out, WM_ERR_INVALID, "dec_self_attention_panel: null pointer");
    WM_REQUIRE(C >= 1 && w >= 1 && w <= WM_MAX_TEACHER_PANEL && C * w <= WM_DEC_MAXB && H >= 1 && T >= 1 && pos >= 0 && pos + w <= T &&
                   out_rows >= C * w && out_rows % 16 == 0,
               WM_ERR_INVALID, "dec_self_attention_panel: bad geometry");
    for (int c = 0; off && c < C; ++c)
        WM_REQUIRE(off[c] >= 0 && off[c] < T, WM_ERR_INVALID, "dec_self_attention_panel: off[%d] = %d outside [0, %d)", c, off[c], T);
    const int B = C * w;
    std::vector<bf16_t> k16, v16;
    to_bf16(k, k16, (size_t)C * H * T * 64);
    to_bf16(v, v16, (size_t)C * H * T * 64);
    const size_t dd = (size_t)H * 64;
    const std::vector<bf16_t> fill((size_t)out_rows * dd, (bf16_t)WMDBG_SENTINEL_BF16);
    DevPool pool;
    hipStream_t s = ctx->stream;
    const float *dq;
    const bf16_t *dk, *dv;
    const int *dpos;
    bf16_t *datt;
    WM_TRY(pool.get(&dq, q, (size_t)B * dd * 4, s));
    WM_TRY(pool.get(&dk, k16.data(), k16.size() * 2, s));
    WM_TRY(pool.get(&dv, v16.data(), v16.size() * 2, s));
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&datt, fill.data(), fill.size() * 2, s));
    const int *doff = nullptr;
    if (off) WM_TRY(pool.get(&doff, off, (size_t)C * 4, s));
    DecAttnArgs t = {};
    t.q = dq; t.kc = dk; t.vc = dv; t.att = datt; t.C = C; t.N = w; t.H = H; t.T_stride = T; t.pos_ptr = dpos; t.off = doff;
    WM_TRY(wm_dec_self_attention_panel(ctx, t));
    return down_tiled_bf16(datt, (size_t)out_rows, dd, out, s);
}
extern "C" int wmdbg_dec_self_attention_panel(wm_ctx *ctx, const float *q, const float *k, const float *v, int C, int w, int H,
                                              int T, int pos, int out_rows, float *out) {
    return dec_self_attention_panel(ctx, q, k, v, C, w, H, T, pos, nullptr, out_rows, out);
}
extern "C" int wmdbg_dec_self_attention_panel_off(wm_ctx *ctx, const float *q, const float *k, const float *v, int C, int w, int H,
                                                  int T, int pos, const int32_t *off, int out_rows, float *out) {
    WM_REQUIRE(off, WM_ERR_INVALID, "dec_self_attention_panel_off: null offsets");
    return dec_self_attention_panel(ctx, q, k, v, C, w, H, T, pos, off, out_rows, out);
}

// (off: null = the uniform panel; else the offsets [C] of the panel's windows in a ragged group)
static int dec_embed_panel(wm_ctx *ctx, const float *emb, const float *pemb, int V, int d, int n_ctx, const int32_t *seq, int stride,
                           int c0, int C, int w, int pos, const int32_t *off, int by_steps, float *x, float *xb, float *stats,
                           float *mean) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(emb && pemb && seq && x && xb && stats && mean, WM_ERR_INVALID, "dec_embed_panel: null pointer");
    WM_REQUIRE(V >= 1 && d >= 64 && d % 64 == 0 && C >= 1 && w >= 1 && w <= WM_MAX_TEACHER_PANEL && C * w <= WM_DEC_MAXB && c0 >= 0 &&
                   c0 + C <= stride && pos >= 0 && pos + w <= n_ctx,
               WM_ERR_INVALID, "dec_embed_panel: bad geometry");
    for (size_t i = 0; i < (size_t)n_ctx * stride; ++i) WM_REQUIRE(seq[i] >= 0 && seq[i] < V, WM_ERR_INVALID, "dec_embed_panel: token outside the vocabulary");
    const int B = C * w, Bpad = (B + 15) / 16 * 16, n_tiles = (V + 15) / 16;
    std::vector<bf16_t> e16;
    tile_bf16(emb, (size_t)V, (size_t)d, e16);
    const size_t n_st = (size_t)(Bpad / 16) * (d / 16) * 32;
    std::vector<float> hx((size_t)B * d), hst(n_st), hmean(B);
    std::vector<bf16_t> hxb((size_t)Bpad * d, (bf16_t)0xffffu);
    // the step path's own buffers: the C windows alone
    const int Cpad = (C + 15) / 16 * 16;
    const size_t n_st1 = (size_t)(Cpad / 16) * (d / 16) * 32;
    std::vector<int32_t> seq1;
    std::vector<float> x1, st1, mean1;
    std::vector<bf16_t> xb1;
    DevPool pool;
    hipStream_t s = ctx->stream;
    const bf16_t *de;
    const float *dp;
    const int *dseq;
    int *dpos;
    float *dx, *dst, *dmean;
    bf16_t *dxb;
    WM_TRY(pool.get(&de, e16.data(), e16.size() * 2, s));
    WM_TRY(pool.get(&dp, pemb, (size_t)n_ctx * d * 4, s));
    WM_TRY(pool.get(&dseq, seq, (size_t)n_ctx * stride * 4, s));
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&dx, nullptr, (size_t)B * d * 4, s, 0xff));
    WM_TRY(pool.get(&dxb, nullptr, (size_t)Bpad * d * 2, s, 0xff));
    WM_TRY(pool.get(&dst, nullptr, n_st * 4, s, 0xff));
    WM_TRY(pool.get(&dmean, nullptr, (size_t)B * 4, s, 0xff));
    const int *doff = nullptr;
    if (off) {
        for (int c = 0; c < C; ++c) WM_REQUIRE(off[c] >= 0 && off[c] < n_ctx, WM_ERR_INVALID, "dec_embed_panel: off[%d] = %d outside [0, %d)", c, off[c], n_ctx);
        WM_TRY(pool.get(&doff, off, (size_t)C * 4, s));
    }
    if (!by_steps) {
        WM_TRY(wm_dec_embed_panel(ctx, dseq + c0, stride, dpos, 0, C, w, n_ctx, WmEmbedDev{de, dp, d, dx, dxb, dst, dmean}, doff));
        WM_HIP(hipMemcpyAsync(hx.data(), dx, hx.size() * 4, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(hxb.data(), dxb, hxb.size() * 2, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(hst.data(), dst, hst.size() * 4, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(hmean.data(), dmean, hmean.size() * 4, hipMemcpyDeviceToHost, s));
        WM_HIP(hipStreamSynchronize(s));
    } else {
        // the step path, position by position over the C windows alone: wm_dec_embed for position 0, the teacher-forced close
        // (wm_argmax_embed with every position a prompt position) for the others; row c of step s is row c * w + s of the panel
        seq1.resize((size_t)n_ctx * C);
        for (int t = 0; t < n_ctx; ++t)
            for (int c = 0; c < C; ++c) seq1[(size_t)t * C + c] = seq[(size_t)t * stride + c0 + c];
        x1.resize((size_t)C * d); st1.resize(n_st1); mean1.resize(C); xb1.resize((size_t)Cpad * d);
        int *dseq1, *darr;
        const unsigned long long *dtile;
        float *dx1, *dst1, *dmean1;
        bf16_t *dxb1;
        WM_TRY(pool.get(&dseq1, seq1.data(), seq1.size() * 4, s));
        WM_TRY(pool.get(&dtile, nullptr, (size_t)C * n_tiles * 8, s));
        WM_TRY(pool.get(&darr, nullptr, 4, s));
        WM_TRY(pool.get(&dx1, nullptr, (size_t)C * d * 4, s));
        WM_TRY(pool.get(&dxb1, nullptr, (size_t)Cpad * d * 2, s));
        WM_TRY(pool.get(&dst1, nullptr, n_st1 * 4, s));
        WM_TRY(pool.get(&dmean1, nullptr, (size_t)C * 4, s));
        const WmEmbedDev e1 = {de, dp, d, dx1, dxb1, dst1, dmean1};
        for (int sp = 0; sp < w; ++sp) {
            const int p = pos + sp;
            if (p == 0) {
                WM_HIP(hipMemsetAsync(dpos, 0, 4, s));
                WM_TRY(wm_dec_embed(ctx, dseq1, dpos, C, e1, doff));
            } else {
                const int pm = p - 1;
                WM_HIP(hipMemcpyAsync(dpos, &pm, 4, hipMemcpyHostToDevice, s));
                WM_HIP(hipStreamSynchronize(s));
                WM_TRY(wm_argmax_embed(ctx, dtile, n_tiles, C, dseq1, dpos, n_ctx, nullptr, 0, n_ctx, e1, WmTsDev{}, darr, 0, WmStopDev{},
                                       WmXDev{}, doff));
            }
            WM_HIP(hipMemcpyAsync(x1.data(), dx1, x1.size() * 4, hipMemcpyDeviceToHost, s));
            WM_HIP(hipMemcpyAsync(xb1.data(), dxb1, xb1.size() * 2, hipMemcpyDeviceToHost, s));
            WM_HIP(hipMemcpyAsync(st1.data(), dst1, st1.size() * 4, hipMemcpyDeviceToHost, s));
            WM_HIP(hipMemcpyAsync(mean1.data(), dmean1, mean1.size() * 4, hipMemcpyDeviceToHost, s));
            WM_HIP(hipStreamSynchronize(s));
            for (int c = 0; c < C; ++c) {
                const size_t r = (size_t)c * w + sp;
                memcpy(&hx[r * d], &x1[(size_t)c * d], (size_t)d * 4);
                for (int j = 0; j < d; ++j) hxb[wm_tiled_offset(r, (size_t)j, (size_t)d)] = xb1[wm_tiled_offset((size_t)c, (size_t)j, (size_t)d)];
                for (int pt = 0; pt < d / 16; ++pt)
                    for (int i = 0; i < 2; ++i) hst[stat_at(d, r, pt, i)] = st1[stat_at(d, (size_t)c, pt, i)];
                hmean[r] = mean1[c];
            }
        }
    }
    memcpy(x, hx.data(), hx.size() * 4);
    memcpy(mean, hmean.data(), hmean.size() * 4);
    untile_bf16(hxb, (size_t)B, (size_t)d, xb);
    // statistics [B][d / 16][2]: the parts of row r
    for (size_t r = 0; r < (size_t)B; ++r)
        for (int pt = 0; pt < d / 16; ++pt)
            for (int i = 0; i < 2; ++i) stats[(r * (d / 16) + pt) * 2 + i] = hst[stat_at(d, r, pt, i)];
    return WM_OK;
}
extern "C" int wmdbg_dec_embed_panel(wm_ctx *ctx, const float *emb, const float *pemb, int V, int d, int n_ctx, const int32_t *seq,
                                     int stride, int c0, int C, int w, int pos, int by_steps, float *x, float *xb, float *stats,
                                     float *mean) {
    return dec_embed_panel(ctx, emb, pemb, V, d, n_ctx, seq, stride, c0, C, w, pos, nullptr, by_steps, x, xb, stats, mean);
}
extern "C" int wmdbg_dec_embed_panel_off(wm_ctx *ctx, const float *emb, const float *pemb, int V, int d, int n_ctx, const int32_t *seq,
                                         int stride, int c0, int C, int w, int pos, const int32_t *off, int by_steps, float *x,
                                         float *xb, float *stats, float *mean) {
    WM_REQUIRE(off, WM_ERR_INVALID, "dec_embed_panel_off: null offsets");
    return dec_embed_panel(ctx, emb, pemb, V, d, n_ctx, seq, stride, c0, C, w, pos, off, by_steps, x, xb, stats, mean);
}

// ------------------------------------------------------------------ prompt panels (wm_set_prompt_panel) ----
extern "C" int wmdbg_prompt_panel_plan(int G, int width, int P, int sot_pos, int acap_base, int32_t *out) {
    WM_REQUIRE(out && G >= 1 && G <= WM_DEC_MAXB && width >= 1 && width <= WM_MAX_TEACHER_PANEL && P >= 1 && sot_pos >= -1 && sot_pos < P &&
                   acap_base >= -1 && acap_base < P,
               WM_ERR_INVALID, "wmdbg_prompt_panel_plan: bad arguments");
    WmPromptPanelPlan pl;
    wm_prompt_panel_plan(G, width, P, sot_pos, acap_base, 0, &pl);
    out[0] = pl.P0; out[1] = pl.C; out[2] = pl.w; out[3] = pl.slices; out[4] = pl.steps;
    return WM_OK;
}
extern "C" int wmdbg_prompt_panel_plan_batch(int n, const int32_t *in, int32_t *out) {
    WM_REQUIRE(n >= 0 && (n == 0 || (in && out)), WM_ERR_INVALID, "wmdbg_prompt_panel_plan_batch: bad arguments");
    for (int i = 0; i < n; ++i)
        WM_TRY(wmdbg_prompt_panel_plan(in[5 * (size_t)i], in[5 * (size_t)i + 1], in[5 * (size_t)i + 2], in[5 * (size_t)i + 3], in[5 * (size_t)i + 4],
                                       out + 5 * (size_t)i));
    return WM_OK;
}
extern "C" int wmdbg_last_prompt_prefill(wm_ctx *ctx, int32_t *out) {
    WM_REQUIRE(ctx && ctx->model && out, WM_ERR_INVALID, "wmdbg_last_prompt_prefill: null pointer");
    for (int i = 0; i < 3; ++i) out[i] = ctx->model->last_prefill[i];
    return WM_OK;
}

// ------------------------------------------------------------------ given panels (wm_set_given_panel) ----
extern "C" int wmdbg_given_panel_plan(int G, int width, const int32_t *lens, const int32_t *budgets, int max_new, int P, int n_text_ctx,
                                      uint32_t bits, int32_t *out) {
    WM_REQUIRE(out && lens && G >= 1 && G <= WM_DEC_MAXB && width >= 1 && width <= WM_MAX_TEACHER_PANEL && max_new >= 1 && P >= 1 &&
                   n_text_ctx >= 1,
               WM_ERR_INVALID, "wmdbg_given_panel_plan: bad arguments");
    WmGivenPanelPlan pl;
    wm_given_panel_plan(G, width, lens, budgets, max_new, P, n_text_ctx, bits, &pl);
    out[0] = pl.reason; out[1] = pl.w; out[2] = pl.Lp; out[3] = pl.rounds;
    return WM_OK;
}
extern "C" int wmdbg_given_panel_plan_batch(int n, int g_max, const int32_t *in, int32_t *out) {
    WM_REQUIRE(n >= 0 && g_max >= 1 && g_max <= WM_DEC_MAXB && (n == 0 || (in && out)), WM_ERR_INVALID, "wmdbg_given_panel_plan_batch: bad arguments");
    const size_t stride = 8 + 2 * (size_t)g_max;
    for (int i = 0; i < n; ++i) {
        const int32_t *c = in + stride * (size_t)i;
        WM_REQUIRE(c[0] <= g_max, WM_ERR_INVALID, "wmdbg_given_panel_plan_batch: case %d has %d rows, the table holds %d", i, c[0], g_max);
        WM_TRY(wmdbg_given_panel_plan(c[0], c[1], c + 8, c[6] ? c + 8 + g_max : nullptr, c[2], c[3], c[4], (uint32_t)c[5], out + 4 * (size_t)i));
    }
    return WM_OK;
}
extern "C" int wmdbg_last_given_panel(wm_ctx *ctx, int32_t *out) {
    WM_REQUIRE(ctx && ctx->model && out, WM_ERR_INVALID, "wmdbg_last_given_panel: null pointer");
    for (int i = 0; i < 4; ++i) out[i] = ctx->model->last_given_panel[i];
    return WM_OK;
}
extern "C" int wmdbg_last_given_panel_lane(wm_ctx *ctx, int lane, int32_t *out) {
    WM_REQUIRE(ctx && ctx->model && out, WM_ERR_INVALID, "wmdbg_last_given_panel_lane: null pointer");
    WM_REQUIRE(lane >= 0 && lane <= (int)ctx->lanes.size(), WM_ERR_INVALID, "wmdbg_last_given_panel_lane: lane %d of %d", lane,
               (int)ctx->lanes.size() + 1);
    return wmdbg_last_given_panel(lane == 0 ? ctx : ctx->lanes[(size_t)lane - 1], out);
}

extern "C" int wmdbg_align_capture_panel(wm_ctx *ctx, const float *dq, int d, int C, int w, int pos, const int32_t *heads, int n_heads,
                                         int slot0, int Tq, int J, int by_steps, float *cap) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(dq && heads && cap && d >= 64 && d % 64 == 0 && C >= 1 && w >= 1 && w <= WM_MAX_TEACHER_PANEL && C * w <= WM_DEC_MAXB &&
                   pos >= 0 && n_heads >= 1 && n_heads <= 32 && slot0 >= 0 && slot0 + n_heads <= J && Tq >= 1,
               WM_ERR_INVALID, "align_capture_panel: bad geometry");
    WmAlignLayer L;
    L.n = n_heads; L.slot0 = slot0;
    for (int i = 0; i < n_heads; ++i) {
        WM_REQUIRE(heads[i] >= 0 && heads[i] < d / 64, WM_ERR_INVALID, "align_capture_panel: head %d outside the row", heads[i]);
        L.head[i] = heads[i];
    }
    const int B = C * w;
    const size_t n_cap = (size_t)C * Tq * J * 64;
    const std::vector<uint32_t> fill(n_cap, WMDBG_SENTINEL_F32);
    std::vector<float> q1(by_steps ? (size_t)C * d : 0);   // the step path: one position's rows
    DevPool pool;
    hipStream_t s = ctx->stream;
    const float *dd;
    int *dpos;
    float *dcap;
    WM_TRY(pool.get(&dd, dq, (size_t)B * d * 4, s));
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&dcap, fill.data(), n_cap * 4, s));
    if (!by_steps) {
        WM_TRY(wm_align_capture_q(ctx, dd, d, B, L, dcap, Tq, J, dpos, w));
    } else {
        float *d1;
        WM_TRY(pool.get(&d1, nullptr, q1.size() * 4, s));
        for (int sp = 0; sp < w; ++sp) {
            for (int c = 0; c < C; ++c) memcpy(&q1[(size_t)c * d], dq + ((size_t)c * w + sp) * d, (size_t)d * 4);
            const int p = pos + sp;
            WM_HIP(hipMemcpyAsync(d1, q1.data(), q1.size() * 4, hipMemcpyHostToDevice, s));
            WM_HIP(hipMemcpyAsync(dpos, &p, 4, hipMemcpyHostToDevice, s));
            WM_HIP(hipStreamSynchronize(s));
            WM_TRY(wm_align_capture_q(ctx, d1, d, C, L, dcap, Tq, J, dpos));
        }
    }
    WM_HIP(hipMemcpyAsync(cap, dcap, n_cap * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

extern "C" int wmdbg_align_token_prob_panel(wm_ctx *ctx, const float *logits, int C, int w, int V, int ldo, const int32_t *seq,
                                            int n_ctx, int pos, int S, int eot, const int32_t *n_text, int max_text, int by_steps,
                                            float *prob) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(logits && seq && n_text && prob && C >= 1 && w >= 1 && w <= WM_MAX_TEACHER_PANEL && C * w <= WM_DEC_MAXB && V >= 1 &&
                   ldo >= V && eot >= 1 && eot <= V && pos >= 0 && pos + w < n_ctx && S >= 0 && max_text >= 1,
               WM_ERR_INVALID, "align_token_prob_panel: bad geometry");
    for (int c = 0; c < C; ++c) WM_REQUIRE(n_text[c] >= 0 && n_text[c] <= max_text, WM_ERR_INVALID, "align_token_prob_panel: n_text[%d]", c);
    for (size_t i = 0; i < (size_t)n_ctx * C; ++i) WM_REQUIRE(seq[i] >= 0 && seq[i] < eot, WM_ERR_INVALID, "align_token_prob_panel: token not below eot");
    const int B = C * w;
    const std::vector<uint32_t> fill((size_t)C * max_text, WMDBG_SENTINEL_F32);
    std::vector<float> l1(by_steps ? (size_t)C * ldo : 0);   // the step path: one position's rows
    DevPool pool;
    hipStream_t s = ctx->stream;
    const float *dl;
    const int *dseq, *dn;
    int *dpos;
    float *dp;
    WM_TRY(pool.get(&dl, logits, (size_t)B * ldo * 4, s));
    WM_TRY(pool.get(&dseq, seq, (size_t)n_ctx * C * 4, s));
    WM_TRY(pool.get(&dn, n_text, (size_t)C * 4, s));
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&dp, fill.data(), fill.size() * 4, s));
    if (!by_steps) {
        WM_TRY(wm_align_token_prob(ctx, dl, ldo, dseq, dpos, B, S, eot, dn, dp, max_text, w, C));
    } else {
        float *d1;
        WM_TRY(pool.get(&d1, nullptr, l1.size() * 4, s));
        for (int sp = 0; sp < w; ++sp) {
            for (int c = 0; c < C; ++c) memcpy(&l1[(size_t)c * ldo], logits + ((size_t)c * w + sp) * ldo, (size_t)ldo * 4);
            const int p = pos + sp;
            WM_HIP(hipMemcpyAsync(d1, l1.data(), l1.size() * 4, hipMemcpyHostToDevice, s));
            WM_HIP(hipMemcpyAsync(dpos, &p, 4, hipMemcpyHostToDevice, s));
            WM_HIP(hipStreamSynchronize(s));
            WM_TRY(wm_align_token_prob(ctx, d1, ldo, dseq, dpos, C, S, eot, dn, dp, max_text));
        }
    }
    WM_HIP(hipMemcpyAsync(prob, dp, fill.size() * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

extern "C" int wmdbg_step_layout(int32_t *out4) {
    if (!out4) return WM_ERR_INVALID;
    out4[0] = (int32_t)sizeof(wmdbg_step); out4[1] = (int32_t)offsetof(wmdbg_step, seed);
    out4[2] = (int32_t)offsetof(wmdbg_step, logits); out4[3] = (int32_t)offsetof(wmdbg_step, stats_tail_nonzero);
    return WM_OK;
}

// A sequence-bias table (wm_sb_expand) in device memory as the product lays it out, the per-row state pre-filled with 0xff
// bytes: a word or list element the state kernel leaves alone shows.
static int stage_seqbias(DevPool &pool, hipStream_t s, const WmSbTable &t, int B, int words, WmSbPar *par_host, WmSbDev *out) {
    const size_t cap = WM_MAX_BIAS_ENTRIES;
    const int ng = t.n_groups(), ne = t.n_entries();
    WmSbDev d;
    memset(&d, 0, sizeof(d));
    par_host->n_groups = ng; par_host->n_entries = ne;
    std::vector<int32_t> beg(t.grp_beg);
    if (beg.empty()) beg.push_back(0);
    WM_TRY(pool.get(&d.par, par_host, sizeof(WmSbPar), s));
    WM_TRY(pool.get(&d.grp_id, ng ? t.grp_id.data() : nullptr, std::max<size_t>(ng, 1) * 4, s));
    WM_TRY(pool.get(&d.grp_beg, beg.data(), beg.size() * 4, s));
    WM_TRY(pool.get(&d.ent_len, ne ? t.ent_len.data() : nullptr, std::max<size_t>(ne, 1) * 4, s));
    WM_TRY(pool.get(&d.ent_bias, ne ? t.ent_bias.data() : nullptr, std::max<size_t>(ne, 1) * 4, s));
    WM_TRY(pool.get(&d.ent_ctx, ne ? t.ent_ctx.data() : nullptr, std::max<size_t>(ne, 1) * WM_SB_CTX * 4, s));
    WM_HIP(hipStreamSynchronize(s));   // `beg` leaves scope
    WM_TRY(pool.get(&d.e.hit, nullptr, (size_t)B * words * 4, s, 0xff));
    WM_TRY(pool.get(&d.e.cnt, nullptr, (size_t)B * 4, s, 0xff));
    WM_TRY(pool.get(&d.e.lid, nullptr, (size_t)B * cap * 4, s, 0xff));
    WM_TRY(pool.get(&d.e.ltot, nullptr, (size_t)B * cap * 4, s, 0xff));
    WM_TRY(pool.get(&d.e.woff, nullptr, (size_t)B * words * 4, s, 0xff));
    d.e.words = words;
    *out = d;
    return WM_OK;
}

// A constraint automaton (wm_cst_build) in device memory as the product lays it out, with the rows' starts.
static int stage_constraint(DevPool &pool, hipStream_t s, const WmCstTable &t, const int32_t *starts, int B, WmCstPar *par_host, WmCstDev *out) {
    const int ns = t.n_states(), ne = t.n_edges();
    WmCstDev d;
    memset(&d, 0, sizeof(d));
    par_host->n_states = ns; par_host->n_edges = ne; par_host->eot = t.eot;
    WM_TRY(pool.get(&d.par, par_host, sizeof(WmCstPar), s));
    WM_TRY(pool.get(&d.edge_beg, t.edge_beg.data(), (size_t)(ns + 1) * 4, s));
    WM_TRY(pool.get(&d.edge_tok, ne ? t.edge_tok.data() : nullptr, std::max<size_t>(ne, 1) * 4, s));
    WM_TRY(pool.get(&d.edge_next, ne ? t.edge_next.data() : nullptr, std::max<size_t>(ne, 1) * 4, s));
    WM_TRY(pool.get(&d.def_next, t.def_next.data(), (size_t)ns * 4, s));
    WM_TRY(pool.get(&d.accept, t.accept.data(), (size_t)ns * 4, s));
    WM_TRY(pool.get(&d.hash, t.hash.data(), t.hash.size() * 4, s));
    WM_TRY(pool.get(&d.start, starts, (size_t)B * 4, s));
    *out = d;
    return WM_OK;
}

// wmdbg_decode_close_shared: where the beam and accept closes of the step's partials go (host, [B] each)
struct CloseShared {
    int w;
    int32_t *beam_n, *beam_tok, *acc_tok;
    float *beam_lp, *beam_nospeech, *acc_lp;
};
// The beam list kernel (B windows, N = 1) and the accept + commit of B / w windows x w rows on the partials the logits launch
// `a` left, enqueued in front of the arg-max close.  Everything either one writes is scratch of `pool`: the arg-max close behind
// them reads the step's own state.  The copies to the host are synchronised by the caller.
static int shared_closes_run(wm_ctx *ctx, DevPool &pool, const wmdbg_step *io, const CloseShared &sh, const DecGemvArgs &a,
                             const unsigned *dmask, int mw) {
    const int B = io->B, w = sh.w, G = B / w, n_ctx = io->n_ctx, L = WM_MAX_BEAM + 1;
    hipStream_t s = ctx->stream;
    const std::vector<uint32_t> nan32(B, WMDBG_SENTINEL_F32);
    // beam: live beams with sum 0 in windows that have not left; no_speech_prob into a buffer of its own
    WmBeamDev bm;
    memset(&bm, 0, sizeof(bm));
    bm.N = 1; bm.n_ctx = n_ctx;
    WmXDev bx = a.x;
    WM_TRY(pool.get(&bx.nospeech, nan32.data(), (size_t)B * 4, s));
    WM_HIP(hipStreamSynchronize(s));   // nan32 leaves scope with this function
    WM_TRY(pool.get(&bm.sum, nullptr, (size_t)B * 4, s));
    WM_TRY(pool.get(&bm.wdone, nullptr, (size_t)B * 4, s));
    WM_TRY(pool.get(&bm.list_n, nullptr, (size_t)B * 4, s, 0xff));
    WM_TRY(pool.get(&bm.list_tok, nullptr, (size_t)B * L * 4, s, 0xff));
    WM_TRY(pool.get(&bm.list_lp, nullptr, (size_t)B * L * 4, s, 0xff));
    WM_TRY(wm_beam_topk(ctx, WmStoredRows{a.out_f32, a.ldo, io->V, a.argmax, B, a.ts, bx, a.mask ? dmask : nullptr, mw, io->n_prompt, a.pos_ptr,
                                           WmStopDev{}, nullptr, 0}, bm));
    // accept: the rows' ranges are the step's; the commit launch behind it advances scratch copies only
    WmSpecDev sp;
    memset(&sp, 0, sizeof(sp));
    sp.tts = a.ts; sp.max_new = n_ctx; sp.n_vocab = io->V;
    int *dpos2, *dstate;
    WM_TRY(pool.get(&sp.tseq, nullptr, (size_t)(n_ctx + w + 1) * G * 4, s));
    WM_TRY(pool.get(&sp.dseq, nullptr, (size_t)(n_ctx + w + 1) * G * 4, s));
    const int pos2[2] = {io->pos, io->pos};
    WM_TRY(pool.get(&dpos2, pos2, 8, s));
    WM_HIP(hipStreamSynchronize(s));   // pos2 too
    sp.tpos = dpos2; sp.dpos = dpos2 + 1;
    WM_TRY(pool.get(&dstate, nullptr, ((size_t)G * 21 + 2) * 4, s));   // chist | crng | dchist | dcrng | stats | acc | round
    sp.chist = dstate; sp.crng = dstate + G * 4; sp.dchist = dstate + G * 8; sp.dcrng = dstate + G * 12;
    sp.stats = dstate + G * 16; sp.acc = dstate + G * 20; sp.round = dstate + G * 21;
    WM_TRY(pool.get(&sp.wtok, nullptr, (size_t)B * 4, s, 0xff));
    WM_TRY(pool.get(&sp.wlp, nullptr, (size_t)B * 4, s, 0xff));
    WmXDev ax = a.x;
    WM_TRY(pool.get(&ax.logprob, nullptr, (size_t)n_ctx * G * 4, s));
    WmStopDev st;
    memset(&st, 0, sizeof(st));
    WM_TRY(pool.get(&st.done, nullptr, (size_t)G * 4, s));
    WM_TRY(pool.get(&st.n_live, nullptr, 4, s));
    st.eot = -1;
    WM_TRY(wm_spec_accept(ctx, a.argmax, (io->V + 15) / 16, sp, ax, st, G, w, io->n_prompt, n_ctx, io->fallback_tok));
    WM_HIP(hipMemcpyAsync(sh.beam_n, bm.list_n, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpy2DAsync(sh.beam_tok, 4, bm.list_tok, (size_t)L * 4, 4, B, hipMemcpyDeviceToHost, s));   // slot 0 of every row
    WM_HIP(hipMemcpy2DAsync(sh.beam_lp, 4, bm.list_lp, (size_t)L * 4, 4, B, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(sh.beam_nospeech, bx.nospeech, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(sh.acc_tok, sp.wtok, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(sh.acc_lp, sp.wlp, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    return WM_OK;
}

// rep: the repetition rules (penalty, ngram, io->eot) are on -- wm_repeat_state in front of a DE_LOGITS_XR launch
// sbt (with rep): the sequence bias as well -- wm_seqbias_state behind it and a DE_LOGITS_XB launch, also for an empty table
// sh: the beam and accept closes on the same partials, in front of the arg-max close (wmdbg_decode_close_shared)
// trunc: the sampling rules are on -- wm_sample_truncate between the logits launch and the close (a sampling X-mode step)
// cst (with rep): the constraint as well -- wm_constraint_state behind the other state launches, with the rows' starts
// row_T / row_seed: temperature and seed per row (wm_set_sampling_rows) -- io->temperature and io->seed are not read, the X-mode
// kernels are handed the rows' table
// gv: the given-tokens launch last in front of the close (given == null: no launch), and the row's keys and winner values as
// the launches in front of the close left them
struct CloseGiven {
    const int32_t *given;   // [B], -1: the row decodes freely
    uint64_t *tilemax_out, *key_ts_out;   // [B][n_tiles] (key_ts_out: read with timestamp rules)
    float *win_out;                       // [B][n_tiles][2]
};
static int decode_close_run(wm_ctx *ctx, wmdbg_step *io, bool rep, float penalty, int ngram, const WmSbTable *sbt = nullptr,
                            const CloseShared *sh = nullptr, const WmSampPar *trunc = nullptr, const WmCstTable *cst = nullptr,
                            const int32_t *cst_starts = nullptr, const float *row_T = nullptr, const uint64_t *row_seed = nullptr,
                            const CloseGiven *gv = nullptr) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(io, WM_ERR_INVALID, "wmdbg_decode_close: null");
    if (rep)
        WM_REQUIRE(io->x_on && std::isfinite(penalty) && penalty > 0.f && ngram >= 0 && ngram <= WM_MAX_NGRAM && io->eot >= 0 &&
                       io->eot <= io->V && io->n_prompt <= io->n_ctx,
                   WM_ERR_INVALID, "wmdbg_decode_close_rep: needs x_on, a finite penalty > 0, ngram 0 .. 32 and eot in [0, V]");
    const int B = io->B, V = io->V, K = io->K, n_ctx = io->n_ctx, pos = io->pos, n_prompt = io->n_prompt;
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && V >= 16 && K >= 64 && K % 64 == 0 && K <= 1280 && n_ctx >= 1 && pos >= 0 && pos < n_ctx &&
                   n_prompt >= 1,
               WM_ERR_INVALID, "wmdbg_decode_close: bad geometry");
    WM_REQUIRE(io->x && io->ln_g && io->ln_b && io->emb && io->pemb && io->seq && io->logits && io->tok && io->result && io->logprob &&
                   io->nospeech && io->x_next && io->xb_next && io->stats_next,
               WM_ERR_INVALID, "wmdbg_decode_close: null pointer");
    WM_REQUIRE(io->n_suppress >= 0 && io->n_suppress_first >= 0 && (io->n_suppress == 0 || io->suppress) &&
                   (io->n_suppress_first == 0 || io->suppress_first),
               WM_ERR_INVALID, "wmdbg_decode_close: bad suppress lists");
    WM_REQUIRE(io->arg_first >= 0 && io->arg_first <= io->arg_last && io->arg_last < V && io->fallback_tok >= 0 && io->fallback_tok < V,
               WM_ERR_INVALID, "wmdbg_decode_close: bad arg-max range / fallback token");
    WM_REQUIRE(io->ts_mode >= 0 && io->ts_mode <= 2, WM_ERR_INVALID, "wmdbg_decode_close: ts_mode 0 .. 2");
    if (io->ts_mode)
        WM_REQUIRE(io->rng && io->hist && io->ts_begin > 0 && io->ts_begin < V && io->eot >= 0 && io->eot < io->ts_begin, WM_ERR_INVALID,
                   "wmdbg_decode_close: timestamp rules need rng, hist and 0 <= eot < ts_begin < V");
    if (io->x_on)
        WM_REQUIRE(io->temperature >= 0.f && io->chunk0 >= 0 && (io->sot_pos < 0 || (io->ns_tok >= 0 && io->ns_tok < V)), WM_ERR_INVALID,
                   "wmdbg_decode_close: bad X-mode parameters");
    if (io->stop_on) WM_REQUIRE(io->done && io->live_rows && io->pad_tok >= 0 && io->pad_tok < V, WM_ERR_INVALID, "wmdbg_decode_close: early stop needs done, live_rows and a pad token");
    const int vpad = (V + 15) / 16 * 16, n_tiles = vpad / 16, mw = (vpad + 31) / 32, Bpad = (B + 15) / 16 * 16;
    for (int i = 0; i < n_ctx * B; ++i) WM_REQUIRE(io->seq[i] >= 0 && io->seq[i] < V, WM_ERR_INVALID, "wmdbg_decode_close: seq[%d] outside the vocabulary", i);
    if (io->ts_mode == 2)
        for (int i = 0; i < 4 * B; ++i) WM_REQUIRE(io->rng[i] >= 0 && io->rng[i] <= V, WM_ERR_INVALID, "wmdbg_decode_close: rng[%d] outside [0, V]", i);
    std::vector<unsigned> mask((size_t)2 * mw, 0u);   // [0] every position, [1] = [0] | the first-position list (wm_set_suppress)
    for (int i = 0; i < io->n_suppress; ++i) {
        WM_REQUIRE(io->suppress[i] >= 0 && io->suppress[i] < V, WM_ERR_INVALID, "wmdbg_decode_close: suppressed id %d", io->suppress[i]);
        mask[io->suppress[i] >> 5] |= 1u << (io->suppress[i] & 31);
    }
    for (int i = 0; i < mw; ++i) mask[mw + i] = mask[i];
    for (int i = 0; i < io->n_suppress_first; ++i) {
        WM_REQUIRE(io->suppress_first[i] >= 0 && io->suppress_first[i] < V, WM_ERR_INVALID, "wmdbg_decode_close: suppressed id %d", io->suppress_first[i]);
        mask[mw + (io->suppress_first[i] >> 5)] |= 1u << (io->suppress_first[i] & 31);
    }
    const bool mask_on = io->n_suppress + io->n_suppress_first > 0;
    std::vector<bf16_t> e16, x16;
    std::vector<float> st, mean;
    tile_bf16(io->emb, (size_t)V, (size_t)K, e16);
    stage_ln_rows(io->x, B, K, true, x16, st, mean);
    const size_t nt = (size_t)B * n_tiles, st_words = (size_t)(Bpad / 16) * 2 * K;
    const std::vector<uint32_t> nan32(std::max({(size_t)n_ctx * B, (size_t)B * K, st_words}), WMDBG_SENTINEL_F32);
    const std::vector<bf16_t> nan16((size_t)Bpad * K, (bf16_t)WMDBG_SENTINEL_BF16);
    WmXPar xp;
    memset(&xp, 0, sizeof(xp));
    xp.key0 = (unsigned)io->seed; xp.key1 = (unsigned)(io->seed >> 32);
    xp.sample = io->temperature > 0.f ? 1 : 0;
    xp.inv_T = io->temperature > 0.f ? (float)(1.0 / (double)io->temperature) : 0.f;   // as wm_transcribe fills it
    xp.sot_pos = io->sot_pos; xp.ns_tok = io->ns_tok; xp.chunk0 = io->chunk0; xp.n_prompt = n_prompt; xp.n_cand = 1;
    std::vector<WmXRow> xrows;
    if (row_T) {   // as lane_prefill fills it: behind the (unused) id words, padded with arg-max rows, the scalar fields unused
        WM_REQUIRE(io->x_on && row_seed, WM_ERR_INVALID, "wmdbg_decode_close_rows: needs x_on and both row arrays");
        xrows.assign((size_t)WM_XIDS_WORDS / 4, WmXRow{0.f, 0u, 0u, 0u});
        WmXRow *tab = const_cast<WmXRow *>(wm_x_rows((const unsigned *)xrows.data()));
        xp.key0 = xp.key1 = 0u; xp.inv_T = 0.f; xp.sample = 0; xp.rows_on = 1;
        for (int b = 0; b < B; ++b) {
            WM_REQUIRE(std::isfinite(row_T[b]) && row_T[b] >= 0.f, WM_ERR_INVALID, "wmdbg_decode_close_rows: temperature of row %d", b);
            if (!(row_T[b] > 0.f)) continue;
            tab[b] = WmXRow{(float)(1.0 / (double)row_T[b]), (unsigned)row_seed[b], (unsigned)(row_seed[b] >> 32), 0u};
            xp.sample = 1;
        }
    }
    WmRepPar rpar;
    WmSbPar sbpar;
    WmCstPar cpar;
    const int zero = 0;
    std::vector<float> lg((size_t)B * vpad), lp((size_t)n_ctx * B), stn(st_words);
    DevPool pool;
    hipStream_t s = ctx->stream;
    DecGemvArgs a;
    memset(&a, 0, sizeof(a));
    a.epi = io->x_on ? DE_LOGITS_X : DE_LOGITS; a.B = B; a.N = V; a.K = K; a.stats_parts = K / 16; a.ldo = vpad;
    a.arg_first = io->arg_first; a.arg_last = io->arg_last;
    const bf16_t *dE;
    bf16_t *dEf;
    float *dc1, *dc2;
    const float *dg, *db, *dbias = nullptr, *dpemb;
    WM_TRY(pool.get(&a.a, x16.data(), x16.size() * 2, s));
    WM_TRY(pool.get(&dE, e16.data(), e16.size() * 2, s));
    WM_TRY(pool.get(&dEf, nullptr, e16.size() * 2, s));
    WM_TRY(pool.get(&dc1, nullptr, (size_t)vpad * 4, s));
    WM_TRY(pool.get(&dc2, nullptr, (size_t)vpad * 4, s));
    WM_TRY(pool.get(&dg, io->ln_g, (size_t)K * 4, s));
    WM_TRY(pool.get(&db, io->ln_b, (size_t)K * 4, s));
    if (io->bias) WM_TRY(pool.get(&dbias, io->bias, (size_t)V * 4, s));
    WM_TRY(pool.get(&a.stats_in, st.data(), st.size() * 4, s));
    WM_TRY(pool.get(&a.mean_in, mean.data(), (size_t)B * 4, s));
    WM_TRY(pool.get(&a.mean_out, nullptr, (size_t)B * 4, s));
    WM_TRY(pool.get(&dpemb, io->pemb, (size_t)n_ctx * K * 4, s));
    int *dseq;
    {   // n_ctx + 1 rows, as the model's buffer: the close of the last position writes its token to row n_ctx
        std::vector<int32_t> seq0((size_t)(n_ctx + 1) * B, 0);
        std::copy(io->seq, io->seq + (size_t)n_ctx * B, seq0.begin());
        WM_TRY(pool.get(&dseq, seq0.data(), seq0.size() * 4, s));
        WM_HIP(hipStreamSynchronize(s));   // seq0 leaves scope
    }
    int *dpos, *darr, *dres;
    const unsigned *dmask;
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&darr, &zero, 4, s));
    WM_TRY(pool.get(&a.out_f32, nullptr, (size_t)B * vpad * 4, s));
    WM_TRY(pool.get(&a.argmax, nullptr, nt * 8, s, 0xff));
    WM_TRY(pool.get(&dres, nullptr, (size_t)B * 4, s, 0xff));
    WM_TRY(pool.get(&dmask, mask.data(), mask.size() * 4, s));
    a.pos_ptr = dpos;
    if (mask_on) { a.mask = dmask; a.mask_words = mw; a.mask_first_pos = io->mask_first ? pos : -1; }
    WmTsDev ts;
    memset(&ts, 0, sizeof(ts));
    if (io->ts_mode) {
        WM_TRY(pool.get(&ts.rng, io->ts_mode == 2 ? io->rng : nullptr, (size_t)B * 16, s));
        WM_TRY(pool.get(&ts.hist, io->ts_mode == 2 ? io->hist : nullptr, (size_t)B * 16, s));
        WM_TRY(pool.get(&ts.key_ts, nullptr, nt * 8, s, 0xff));
        WM_TRY(pool.get(&ts.lse, nullptr, nt * 8, s, 0xff));
        ts.ts_begin = io->ts_begin; ts.eot = io->eot; ts.n_vocab = V; ts.max_initial = io->max_initial;
        if (io->ts_mode == 1) WM_TRY(wm_ts_init(ctx, ts, B));
    }
    a.ts = ts;
    WmXDev xd;
    memset(&xd, 0, sizeof(xd));
    float *dns, *dlp;
    WM_TRY(pool.get(&dns, nan32.data(), (size_t)B * 4, s));
    WM_TRY(pool.get(&dlp, nan32.data(), (size_t)n_ctx * B * 4, s));
    if (io->x_on) {
        WM_TRY(pool.get(&xd.par, &xp, sizeof(xp), s));
        WM_TRY(pool.get(&xd.txt, nullptr, nt * 8, s, 0xff));
        WM_TRY(pool.get(&xd.win, nullptr, nt * 8, s, 0xff));
        WM_TRY(pool.get(&xd.all, nullptr, nt * 8, s, 0xff));
        WM_TRY(pool.get(&xd.ns_v, nullptr, (size_t)B * 4, s, 0xff));
        xd.logprob = dlp; xd.nospeech = dns;
        if (row_T) WM_TRY(pool.get(&xd.ids, (const unsigned *)xrows.data(), xrows.size() * sizeof(WmXRow), s));
    }
    a.x = xd;
    WmStopDev sp;
    memset(&sp, 0, sizeof(sp));
    if (io->stop_on) {
        WM_TRY(pool.get(&sp.done, nullptr, (size_t)B * 4, s));
        WM_TRY(pool.get(&sp.live_rows, nullptr, (size_t)B * 4, s));
        WM_TRY(pool.get(&sp.n_live, nullptr, 4, s));
        if (io->budget) WM_TRY(pool.get(&sp.budget, io->budget, (size_t)B * 4, s));
        sp.eot = io->stop_eot; sp.pad_tok = io->pad_tok;
        WM_TRY(wm_stop_init(ctx, sp, B));
        WM_HIP(hipMemcpyAsync(sp.done, io->done, (size_t)B * 4, hipMemcpyHostToDevice, s));   // the flags of the positions before this one
        WM_HIP(hipMemsetAsync(sp.live_rows, 0xff, (size_t)B * 4, s));   // -1: the close rebuilds the list, what it leaves alone shows
    }
    const int *doff = nullptr;
    float *dxn, *dstn, *dmn;
    bf16_t *dxbn;
    if (io->off) WM_TRY(pool.get(&doff, io->off, (size_t)B * 4, s));
    WM_TRY(pool.get(&dxn, nan32.data(), (size_t)B * K * 4, s));
    WM_TRY(pool.get(&dxbn, nan16.data(), nan16.size() * 2, s));
    WM_TRY(pool.get(&dstn, nan32.data(), st_words * 4, s));
    WM_TRY(pool.get(&dmn, nullptr, (size_t)B * 4, s));
    WM_TRY(wm_ln_fold(ctx, dE, dg, db, dbias, V, K, dEf, dc1, dc2));
    a.W = dEf; a.c1 = dc1; a.c2 = dc2;
    if (rep) {   // bitmaps pre-filled with 0xff: every word the epilogue reads must have been rebuilt by this position's launch
        rpar.p = penalty; rpar.inv_p = (float)(1.0 / (double)penalty); rpar.n = ngram; rpar.eot = io->eot;
        WM_TRY(pool.get(&a.rep.seen, nullptr, (size_t)B * mw * 4, s, 0xff));
        WM_TRY(pool.get(&a.rep.ban, nullptr, (size_t)B * mw * 4, s, 0xff));
        WM_TRY(pool.get(&a.rep.par, &rpar, sizeof(rpar), s));
        a.epi = DE_LOGITS_XR;
        a.rep.words = mw;
        WM_TRY(wm_repeat_state(ctx, dseq, dpos, B, n_prompt, n_ctx, V, a.rep));
        if (sbt) {
            WmSbDev sd;
            WM_TRY(stage_seqbias(pool, s, *sbt, B, mw, &sbpar, &sd));
            a.epi = DE_LOGITS_XB;
            a.sb = sd.e;
            WM_TRY(wm_seqbias_state(ctx, dseq, dpos, B, n_prompt, n_ctx, V, sd, a.rep.ban, mw));
        }
        if (cst) {
            WmCstDev cd;
            WM_TRY(stage_constraint(pool, s, *cst, cst_starts, B, &cpar, &cd));
            WM_TRY(wm_constraint_state(ctx, dseq, dpos, B, n_prompt, n_ctx, V, cd, a.rep.ban, mw, nullptr));
        }
    }
    WM_TRY(wm_dec_gemv(ctx, a));
    if (sh) WM_TRY(shared_closes_run(ctx, pool, io, *sh, a, dmask, mw));
    const WmStoredRows stored{a.out_f32, a.ldo, V, a.argmax, B, ts, xd, a.mask ? dmask : nullptr, mw, n_prompt, dpos, sp,
                              rep ? a.rep.ban : nullptr, mw};
    if (trunc) {
        const WmSampPar *dtr;
        WM_TRY(pool.get(&dtr, trunc, sizeof(*trunc), s));
        WM_TRY(wm_sample_truncate(ctx, stored, dtr, nullptr));
    }
    std::vector<int32_t> glen, gtok;
    WmGivenPar gpar;
    if (gv && gv->given) {   // as lane_prefill fills it: the table of a group whose rows are given up to this position
        const int gi = pos + 1 - n_prompt, L = gi + 1 > 1 ? gi + 1 : 1;
        glen.assign(B, 0); gtok.assign((size_t)B * L, 0);
        for (int b = 0; b < B; ++b) {
            if (gv->given[b] < 0) continue;
            glen[b] = L;
            for (int i = 0; i < L; ++i) gtok[(size_t)b * L + i] = gv->given[b];
        }
        int *dgl, *dgt;
        const WmGivenPar *dgp;
        WM_TRY(pool.get(&dgl, glen.data(), glen.size() * 4, s));
        WM_TRY(pool.get(&dgt, gtok.data(), gtok.size() * 4, s));
        gpar.stride = L; gpar.lens = dgl; gpar.tok = dgt;
        WM_TRY(pool.get(&dgp, &gpar, sizeof(gpar), s));
        WM_TRY(wm_given_tokens(ctx, stored, dgp));
    }
    // (ts, sp and xd are empty structs unless ts_mode, stop_on and x_on filled them)
    WM_TRY(wm_argmax_embed(ctx, a.argmax, n_tiles, B, dseq, dpos, n_prompt, dres, io->arg_first, n_ctx,
                           WmEmbedDev{dE, dpemb, K, dxn, dxbn, dstn, dmn}, ts, darr, io->fallback_tok, sp, xd, doff));
    WM_HIP(hipMemcpyAsync(lg.data(), a.out_f32, lg.size() * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(io->result, dres, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(io->seq, dseq, (size_t)n_ctx * B * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(lp.data(), dlp, lp.size() * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(io->nospeech, dns, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(&io->pos_out, dpos, 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(&io->arrive_out, darr, 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(io->x_next, dxn, (size_t)B * K * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(stn.data(), dstn, stn.size() * 4, hipMemcpyDeviceToHost, s));
    if (io->ts_mode) {
        WM_HIP(hipMemcpyAsync(io->rng, ts.rng, (size_t)B * 16, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(io->hist, ts.hist, (size_t)B * 16, hipMemcpyDeviceToHost, s));
    }
    if (gv) {   // (the close reads these and writes none of them)
        WM_HIP(hipMemcpyAsync(gv->tilemax_out, a.argmax, nt * 8, hipMemcpyDeviceToHost, s));
        if (io->ts_mode) WM_HIP(hipMemcpyAsync(gv->key_ts_out, ts.key_ts, nt * 8, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(gv->win_out, xd.win, nt * 8, hipMemcpyDeviceToHost, s));
    }
    io->n_live = -1;
    if (io->stop_on) {
        WM_HIP(hipMemcpyAsync(io->done, sp.done, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(io->live_rows, sp.live_rows, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(&io->n_live, sp.n_live, 4, hipMemcpyDeviceToHost, s));
    }
    WM_TRY(down_tiled_bf16(dxbn, (size_t)B, (size_t)K, io->xb_next, s));
    for (int b = 0; b < B; ++b) {
        memcpy(io->logits + (size_t)b * V, lg.data() + (size_t)b * vpad, (size_t)V * 4);
        io->tok[b] = io->result[b] + io->arg_first;
    }
    const int gi = pos + 1 - n_prompt;
    io->logprob_written = 0;
    for (size_t i = 0; i < lp.size(); ++i) {
        uint32_t u;
        memcpy(&u, &lp[i], 4);
        io->logprob_written += u != WMDBG_SENTINEL_F32;
    }
    memcpy(io->logprob, gi >= 0 ? (const void *)(lp.data() + (size_t)gi * B) : (const void *)nan32.data(), (size_t)B * 4);
    io->stats_tail_nonzero = 0;
    for (int b = 0; b < B; ++b) {   // summed as wmdbg_dec_gemv_resid sums them; the tail: words behind part 0 that are not zero bits
        stats_sum(stn.data(), K, b, io->stats_next + b * 2);
        for (int part = 1; part < K / 16; ++part)
            for (int c = 0; c < 2; ++c) {
                uint32_t u;
                memcpy(&u, &stn[stat_at(K, b, part, c)], 4);
                if (u != 0u) ++io->stats_tail_nonzero;
            }
    }
    return WM_OK;
}

extern "C" int wmdbg_decode_close(wm_ctx *ctx, wmdbg_step *io) { return decode_close_run(ctx, io, false, 1.f, 0); }
extern "C" int wmdbg_decode_close_shared(wm_ctx *ctx, wmdbg_step *io, int w, int32_t *beam_n, int32_t *beam_tok, float *beam_lp,
                                         float *beam_nospeech, int32_t *acc_tok, float *acc_lp) {
    WM_REQUIRE(io && beam_n && beam_tok && beam_lp && beam_nospeech && acc_tok && acc_lp, WM_ERR_INVALID, "wmdbg_decode_close_shared: null");
    WM_REQUIRE(io->x_on && io->temperature == 0.f && (io->ts_mode == 0 || io->ts_mode == 2) && !io->stop_on && io->pos + 1 >= io->n_prompt,
               WM_ERR_INVALID, "wmdbg_decode_close_shared: needs x_on, temperature 0, ts_mode 0 or 2, no early stop and a generated position");
    WM_REQUIRE(w >= 1 && w <= WM_MAX_TEACHER_PANEL && io->B >= 1 && io->B % w == 0, WM_ERR_INVALID,
               "wmdbg_decode_close_shared: the panel width %d does not divide %d rows", w, io->B);
    // (the list kernel takes the first-position bitmap at position n_prompt - 1, the logits launch where mask_first says)
    WM_REQUIRE(io->n_suppress_first == 0 || (io->mask_first != 0) == (io->pos == io->n_prompt - 1), WM_ERR_INVALID,
               "wmdbg_decode_close_shared: mask_first must say whether this is position n_prompt - 1");
    const CloseShared sh = {w, beam_n, beam_tok, acc_tok, beam_lp, beam_nospeech, acc_lp};
    return decode_close_run(ctx, io, false, 1.f, 0, nullptr, &sh);
}
extern "C" int wmdbg_decode_close_trunc(wm_ctx *ctx, wmdbg_step *io, int top_k, float top_p, float min_p) {
    WM_REQUIRE(io, WM_ERR_INVALID, "wmdbg_decode_close_trunc: null");
    WM_REQUIRE(top_k >= 0 && top_p > 0.f && top_p <= 1.f && min_p >= 0.f && min_p < 1.f, WM_ERR_INVALID,
               "wmdbg_decode_close_trunc: top_k >= 0, top_p in (0, 1], min_p in [0, 1)");
    const WmSampPar sp = {top_k, top_p, min_p};
    const bool on = top_k > 0 || top_p < 1.f || min_p > 0.f;
    // as the product: the rules act on a sampling extended-decode step; everywhere else the launches are wmdbg_decode_close's
    if (!on || !io->x_on || !(io->temperature > 0.f)) return decode_close_run(ctx, io, false, 1.f, 0);
    // (the kernel takes the first-position bitmap at position n_prompt - 1, the logits launch where mask_first says)
    WM_REQUIRE(io->n_suppress_first == 0 || (io->mask_first != 0) == (io->pos == io->n_prompt - 1), WM_ERR_INVALID,
               "wmdbg_decode_close_trunc: mask_first must say whether this is position n_prompt - 1");
    return decode_close_run(ctx, io, false, 1.f, 0, nullptr, nullptr, &sp);
}
extern "C" int wmdbg_decode_close_given(wm_ctx *ctx, wmdbg_step *io, const int32_t *given, int top_k, float top_p, float min_p,
                                         uint64_t *tilemax_out, uint64_t *key_ts_out, float *win_out) {
    WM_REQUIRE(io && tilemax_out && key_ts_out && win_out, WM_ERR_INVALID, "wmdbg_decode_close_given: null");
    WM_REQUIRE(top_k >= 0 && top_p > 0.f && top_p <= 1.f && min_p >= 0.f && min_p < 1.f, WM_ERR_INVALID,
               "wmdbg_decode_close_given: top_k >= 0, top_p in (0, 1], min_p in [0, 1)");
    WM_REQUIRE(io->x_on && io->B >= 1 && io->B <= WM_DEC_MAXB, WM_ERR_INVALID, "wmdbg_decode_close_given: needs x_on and 1 .. %d rows", WM_DEC_MAXB);
    if (given)
        for (int b = 0; b < io->B; ++b)
            WM_REQUIRE(given[b] >= -1 && given[b] < io->V, WM_ERR_INVALID, "wmdbg_decode_close_given: row %d: id %d outside [-1, %d)", b,
                       given[b], io->V);
    // (the kernels take the first-position bitmap at position n_prompt - 1, the logits launch where mask_first says)
    WM_REQUIRE(io->n_suppress_first == 0 || (io->mask_first != 0) == (io->pos == io->n_prompt - 1), WM_ERR_INVALID,
               "wmdbg_decode_close_given: mask_first must say whether this is position n_prompt - 1");
    const WmSampPar sp = {top_k, top_p, min_p};
    const bool on = (top_k > 0 || top_p < 1.f || min_p > 0.f) && io->temperature > 0.f;
    const CloseGiven gv = {given, tilemax_out, key_ts_out, win_out};
    return decode_close_run(ctx, io, false, 1.f, 0, nullptr, nullptr, on ? &sp : nullptr, nullptr, nullptr, nullptr, nullptr, &gv);
}
// One round of a given-panel phase on caller-given state (given_panel.hip): stage, the hook's own DE_LOGITS_X launch over the
// G x w rows -- under the ranges the stage left in the rows' slots --, close and commit.  Every state buffer goes up whole (R =
// WM_DEC_MAXB entries, whatever G is) and comes down whole.
extern "C" int wmdbg_given_panel_round(wm_ctx *ctx, wmdbg_given_panel *io) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(io, WM_ERR_INVALID, "wmdbg_given_panel_round: null");
    const int G = io->G, w = io->w, B = G * w, V = io->V, K = io->K, n_ctx = io->n_ctx, pos = io->pos, n_prompt = io->n_prompt;
    constexpr int R = WM_DEC_MAXB;
    WM_REQUIRE(G >= 1 && w >= 1 && w <= WM_MAX_TEACHER_PANEL && B <= R && V >= 16 && K >= 64 && K % 64 == 0 && K <= 1280 && n_ctx >= 2 &&
                   n_prompt >= 1 && pos >= n_prompt && pos + w < n_ctx && io->max_new >= 1 && pos + 1 - n_prompt + w <= io->max_new &&
                   io->stride >= 1,
               WM_ERR_INVALID, "wmdbg_given_panel_round: bad geometry");
    WM_REQUIRE(io->x && io->ln_g && io->ln_b && io->emb && io->seq && io->logprob && io->wtok && io->wlp && io->logits && io->glens &&
                   io->gtok && io->hist && io->rng && io->chist && io->crng && io->done && io->live_rows,
               WM_ERR_INVALID, "wmdbg_given_panel_round: null pointer");
    WM_REQUIRE(io->ts_mode == 0 || io->ts_mode == 2, WM_ERR_INVALID, "wmdbg_given_panel_round: ts_mode 0 or 2");
    if (io->ts_mode)
        WM_REQUIRE(io->ts_begin > 0 && io->ts_begin < V && io->eot >= 0 && io->eot < io->ts_begin, WM_ERR_INVALID,
                   "wmdbg_given_panel_round: timestamp rules need 0 <= eot < ts_begin < V");
    WM_REQUIRE(io->fallback_tok >= 0 && io->fallback_tok < V && io->pad_tok >= 0 && io->pad_tok < V && io->stop_eot < V, WM_ERR_INVALID,
               "wmdbg_given_panel_round: fallback / pad / eot outside the vocabulary");
    WM_REQUIRE(io->n_suppress >= 0 && (io->n_suppress == 0 || io->suppress), WM_ERR_INVALID, "wmdbg_given_panel_round: bad suppress list");
    for (int c = 0; c < G; ++c) {
        WM_REQUIRE(io->glens[c] >= 0 && io->glens[c] <= io->stride, WM_ERR_INVALID, "wmdbg_given_panel_round: lens[%d]", c);
        for (int i = 0; i < io->glens[c]; ++i)
            WM_REQUIRE(io->gtok[(size_t)c * io->stride + i] >= 0 && io->gtok[(size_t)c * io->stride + i] < V, WM_ERR_INVALID,
                       "wmdbg_given_panel_round: given id of window %d outside the vocabulary", c);
    }
    for (int i = 0; i < (n_ctx + 1) * G; ++i)
        WM_REQUIRE(io->seq[i] >= 0 && io->seq[i] < V, WM_ERR_INVALID, "wmdbg_given_panel_round: seq[%d] outside the vocabulary", i);
    if (io->ts_mode)   // (the ranges are compared with ids, never indexed with; the history feeds ts_advance)
        for (int i = 0; i < 4 * R; ++i)
            WM_REQUIRE(io->rng[i] >= 0 && io->rng[i] <= V && io->crng[i] >= 0 && io->crng[i] <= V, WM_ERR_INVALID,
                       "wmdbg_given_panel_round: rng[%d] outside [0, V]", i);
    const int vpad = (V + 15) / 16 * 16, n_tiles = vpad / 16, mw = (vpad + 31) / 32;
    std::vector<unsigned> mask((size_t)2 * mw, 0u);
    for (int i = 0; i < io->n_suppress; ++i) {
        WM_REQUIRE(io->suppress[i] >= 0 && io->suppress[i] < V, WM_ERR_INVALID, "wmdbg_given_panel_round: suppressed id %d", io->suppress[i]);
        mask[io->suppress[i] >> 5] |= 1u << (io->suppress[i] & 31);
    }
    for (int i = 0; i < mw; ++i) mask[mw + i] = mask[i];
    std::vector<bf16_t> e16, x16;
    std::vector<float> st, mean;
    tile_bf16(io->emb, (size_t)V, (size_t)K, e16);
    stage_ln_rows(io->x, B, K, true, x16, st, mean);
    const size_t nt = (size_t)B * n_tiles;
    WmXPar xp;
    memset(&xp, 0, sizeof(xp));
    xp.sot_pos = -1; xp.ns_tok = -1; xp.n_prompt = n_prompt; xp.n_cand = 1;
    DevPool pool;
    hipStream_t s = ctx->stream;
    DecGemvArgs a;
    memset(&a, 0, sizeof(a));
    a.epi = DE_LOGITS_X; a.B = B; a.N = V; a.K = K; a.stats_parts = K / 16; a.ldo = vpad;
    a.arg_first = 0; a.arg_last = V - 1;
    const bf16_t *dE;
    bf16_t *dEf;
    float *dc1, *dc2;
    const float *dg, *db, *dbias = nullptr;
    WM_TRY(pool.get(&a.a, x16.data(), x16.size() * 2, s));
    WM_TRY(pool.get(&dE, e16.data(), e16.size() * 2, s));
    WM_TRY(pool.get(&dEf, nullptr, e16.size() * 2, s));
    WM_TRY(pool.get(&dc1, nullptr, (size_t)vpad * 4, s));
    WM_TRY(pool.get(&dc2, nullptr, (size_t)vpad * 4, s));
    WM_TRY(pool.get(&dg, io->ln_g, (size_t)K * 4, s));
    WM_TRY(pool.get(&db, io->ln_b, (size_t)K * 4, s));
    if (io->bias) WM_TRY(pool.get(&dbias, io->bias, (size_t)V * 4, s));
    WM_TRY(pool.get(&a.stats_in, st.data(), st.size() * 4, s));
    WM_TRY(pool.get(&a.mean_in, mean.data(), (size_t)B * 4, s));
    WM_TRY(pool.get(&a.mean_out, nullptr, (size_t)B * 4, s));
    int *dpos;
    const unsigned *dmask;
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&a.out_f32, nullptr, (size_t)B * vpad * 4, s));
    WM_TRY(pool.get(&a.argmax, nullptr, nt * 8, s, 0xff));
    WM_TRY(pool.get(&dmask, mask.data(), mask.size() * 4, s));
    a.pos_ptr = dpos;
    if (io->n_suppress > 0) { a.mask = dmask; a.mask_words = mw; a.mask_first_pos = -1; }
    WmGivenPanelDev gp;
    memset(&gp, 0, sizeof(gp));
    if (io->ts_mode) {
        WM_TRY(pool.get(&gp.ts.rng, io->rng, (size_t)R * 16, s));
        WM_TRY(pool.get(&gp.ts.hist, io->hist, (size_t)R * 16, s));
        WM_TRY(pool.get(&gp.ts.key_ts, nullptr, nt * 8, s, 0xff));
        WM_TRY(pool.get(&gp.ts.lse, nullptr, nt * 8, s, 0xff));
        gp.ts.ts_begin = io->ts_begin; gp.ts.eot = io->eot; gp.ts.n_vocab = V; gp.ts.max_initial = -1;
    }
    WM_TRY(pool.get(&gp.chist, io->chist, (size_t)R * 16, s));
    WM_TRY(pool.get(&gp.crng, io->crng, (size_t)R * 16, s));
    WM_TRY(pool.get(&gp.wtok, io->wtok, (size_t)R * 4, s));
    WM_TRY(pool.get(&gp.wlp, io->wlp, (size_t)R * 4, s));
    WM_TRY(pool.get(&gp.seq, io->seq, (size_t)(n_ctx + 1) * G * 4, s));
    gp.pos = dpos; gp.max_new = io->max_new; gp.n_vocab = V;
    WmGivenPar gpar;
    int *dgl, *dgt;
    WM_TRY(pool.get(&dgl, io->glens, (size_t)G * 4, s));
    WM_TRY(pool.get(&dgt, io->gtok, (size_t)G * io->stride * 4, s));
    gpar.stride = io->stride; gpar.lens = dgl; gpar.tok = dgt;
    WM_TRY(pool.get(&gp.par, &gpar, sizeof(gpar), s));
    WmXDev xd;
    memset(&xd, 0, sizeof(xd));
    WM_TRY(pool.get(&xd.par, &xp, sizeof(xp), s));
    WM_TRY(pool.get(&xd.txt, nullptr, nt * 8, s, 0xff));
    WM_TRY(pool.get(&xd.win, nullptr, nt * 8, s, 0xff));
    WM_TRY(pool.get(&xd.all, nullptr, nt * 8, s, 0xff));
    WM_TRY(pool.get(&xd.ns_v, nullptr, (size_t)B * 4, s, 0xff));
    WM_TRY(pool.get(&xd.logprob, io->logprob, (size_t)io->max_new * G * 4, s));
    WM_TRY(pool.get(&xd.nospeech, nullptr, (size_t)B * 4, s));
    a.x = xd;
    WmStopDev sp;
    memset(&sp, 0, sizeof(sp));
    sp.pad_tok = io->pad_tok; sp.eot = -1;
    if (io->stop_on) {
        WM_TRY(pool.get(&sp.done, io->done, (size_t)R * 4, s));
        WM_TRY(pool.get(&sp.live_rows, io->live_rows, (size_t)R * 4, s));
        WM_TRY(pool.get(&sp.n_live, &io->n_live, 4, s));
        if (io->budget) WM_TRY(pool.get(&sp.budget, io->budget, (size_t)G * 4, s));
        sp.eot = io->stop_eot;
    }
    WM_TRY(wm_ln_fold(ctx, dE, dg, db, dbias, V, K, dEf, dc1, dc2));
    a.W = dEf; a.c1 = dc1; a.c2 = dc2;
    WM_TRY(wm_given_panel_stage(ctx, gp, sp, G, w, n_prompt, n_ctx, io->first != 0));
    a.ts = gp.ts;   // (the rows' slots as the stage left them)
    WM_TRY(wm_dec_gemv(ctx, a));
    WM_TRY(wm_given_panel_close(ctx, WmStoredRows{a.out_f32, a.ldo, V, a.argmax, B, gp.ts, xd, io->n_suppress > 0 ? dmask : nullptr, mw, n_prompt,
                                                   gp.pos, sp, nullptr, 0}, gp, G, w, io->fallback_tok, io->last != 0));
    std::vector<float> lg((size_t)B * vpad);
    WM_HIP(hipMemcpyAsync(lg.data(), a.out_f32, lg.size() * 4, hipMemcpyDeviceToHost, s));
    if (io->ts_mode) {
        WM_HIP(hipMemcpyAsync(io->rng, gp.ts.rng, (size_t)R * 16, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(io->hist, gp.ts.hist, (size_t)R * 16, hipMemcpyDeviceToHost, s));
    }
    WM_HIP(hipMemcpyAsync(io->chist, gp.chist, (size_t)R * 16, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(io->crng, gp.crng, (size_t)R * 16, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(io->wtok, gp.wtok, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(io->wlp, gp.wlp, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(io->seq, gp.seq, (size_t)(n_ctx + 1) * G * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(io->logprob, xd.logprob, (size_t)io->max_new * G * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(&io->pos_out, dpos, 4, hipMemcpyDeviceToHost, s));
    if (io->stop_on) {
        WM_HIP(hipMemcpyAsync(io->done, sp.done, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(io->live_rows, sp.live_rows, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(&io->n_live, sp.n_live, 4, hipMemcpyDeviceToHost, s));
    }
    WM_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) memcpy(io->logits + (size_t)b * V, lg.data() + (size_t)b * vpad, (size_t)V * 4);
    return WM_OK;
}

extern "C" int wmdbg_decode_close_rows(wm_ctx *ctx, wmdbg_step *io, const float *row_T, const uint64_t *row_seed, int top_k,
                                        float top_p, float min_p) {
    WM_REQUIRE(io && row_T && row_seed, WM_ERR_INVALID, "wmdbg_decode_close_rows: null");
    WM_REQUIRE(top_k >= 0 && top_p > 0.f && top_p <= 1.f && min_p >= 0.f && min_p < 1.f, WM_ERR_INVALID,
               "wmdbg_decode_close_rows: top_k >= 0, top_p in (0, 1], min_p in [0, 1)");
    WM_REQUIRE(io->x_on && io->B >= 1 && io->B <= WM_DEC_MAXB, WM_ERR_INVALID, "wmdbg_decode_close_rows: needs x_on and 1 .. %d rows", WM_DEC_MAXB);
    const WmSampPar sp = {top_k, top_p, min_p};
    bool any = false;
    for (int b = 0; b < io->B; ++b) any = any || row_T[b] > 0.f;
    // as the product: the truncation launch is in the plan when the rules are on and some row samples
    const bool on = (top_k > 0 || top_p < 1.f || min_p > 0.f) && any;
    if (on)
        WM_REQUIRE(io->n_suppress_first == 0 || (io->mask_first != 0) == (io->pos == io->n_prompt - 1), WM_ERR_INVALID,
                   "wmdbg_decode_close_rows: mask_first must say whether this is position n_prompt - 1");
    return decode_close_run(ctx, io, false, 1.f, 0, nullptr, nullptr, on ? &sp : nullptr, nullptr, nullptr, row_T, row_seed);
}
extern "C" int wmdbg_decode_close_rep(wm_ctx *ctx, wmdbg_step *io, float penalty, int ngram) {
    return decode_close_run(ctx, io, true, penalty, ngram);
}

extern "C" int wmdbg_decode_close_sb(wm_ctx *ctx, wmdbg_step *io, float penalty, int ngram, const int32_t *tokens,
                                     const int32_t *seq_offsets, const float *bias, const uint8_t *boost_prefixes, int n_seq) {
    WM_REQUIRE(io, WM_ERR_INVALID, "wmdbg_decode_close_sb: null");
    WmSbTable t;
    WM_TRY(wm_sb_expand(tokens, seq_offsets, bias, boost_prefixes, n_seq, io->eot, io->V, &t));
    return decode_close_run(ctx, io, true, penalty, ngram, &t);
}

extern "C" int wmdbg_seqbias_state(wm_ctx *ctx, const int32_t *seq, int B, int n_ctx, int pos, int n_prompt, int V, const int32_t *tokens,
                                   const int32_t *seq_offsets, const float *bias, const uint8_t *boost_prefixes, int n_seq, int32_t eot,
                                   uint32_t *hit_out, uint32_t *ban_out, int32_t *cnt_out, int32_t *id_out, float *total_out,
                                   int32_t *woff_out) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(seq && hit_out && ban_out && cnt_out && id_out && total_out && woff_out, WM_ERR_INVALID, "wmdbg_seqbias_state: null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && V >= 16 && n_ctx >= 1 && n_ctx <= 448 && pos >= 0 && pos < n_ctx && n_prompt >= 0 &&
                   n_prompt <= n_ctx,
               WM_ERR_INVALID, "wmdbg_seqbias_state: bad geometry");
    WmSbTable t;
    WM_TRY(wm_sb_expand(tokens, seq_offsets, bias, boost_prefixes, n_seq, eot, V, &t));
    const int words = ((V + 15) / 16 * 16 + 31) / 32;
    const size_t cap = WM_MAX_BIAS_ENTRIES;
    WmRepPar rpar;
    rpar.p = 1.f; rpar.inv_p = 1.f; rpar.n = 0; rpar.eot = 0;   // the bitmaps' owner with empty rules, as the product runs it
    WmSbPar sbpar;
    DevPool pool;
    hipStream_t s = ctx->stream;
    const int *dseq, *dpos;
    WmRepDev rd;
    rd.words = words;
    WM_TRY(pool.get(&dseq, seq, (size_t)n_ctx * B * 4, s));
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&rd.par, &rpar, sizeof(rpar), s));
    WM_TRY(pool.get(&rd.seen, nullptr, (size_t)B * words * 4, s, 0xff));
    WM_TRY(pool.get(&rd.ban, nullptr, (size_t)B * words * 4, s, 0xff));
    WmSbDev sd;
    WM_TRY(stage_seqbias(pool, s, t, B, words, &sbpar, &sd));
    WM_TRY(wm_repeat_state(ctx, dseq, dpos, B, n_prompt, n_ctx, V, rd));
    WM_TRY(wm_seqbias_state(ctx, dseq, dpos, B, n_prompt, n_ctx, V, sd, rd.ban, words));
    WM_HIP(hipMemcpyAsync(hit_out, sd.e.hit, (size_t)B * words * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(ban_out, rd.ban, (size_t)B * words * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(cnt_out, sd.e.cnt, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(id_out, sd.e.lid, (size_t)B * cap * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(total_out, sd.e.ltot, (size_t)B * cap * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(woff_out, sd.e.woff, (size_t)B * words * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

extern "C" int wmdbg_decode_close_cst(wm_ctx *ctx, wmdbg_step *io, const int32_t *edge_beg, const int32_t *edge_tok,
                                      const int32_t *edge_next, const int32_t *def_next, const uint8_t *accept, int n_states, int32_t eot,
                                      const int32_t *starts) {
    WM_REQUIRE(io && starts && n_states >= 1, WM_ERR_INVALID, "wmdbg_decode_close_cst: null / no automaton");
    WmCstTable t;
    WM_TRY(wm_cst_build(edge_beg, edge_tok, edge_next, def_next, accept, n_states, eot, io->V, &t));
    for (int b = 0; b < io->B && b < WM_DEC_MAXB; ++b)
        WM_REQUIRE(starts[b] >= -1 && starts[b] < n_states, WM_ERR_INVALID, "wmdbg_decode_close_cst: start of row %d", b);
    return decode_close_run(ctx, io, true, 1.f, 0, nullptr, nullptr, nullptr, &t, starts);
}

extern "C" int wmdbg_constraint_state(wm_ctx *ctx, const int32_t *seq, int B, int n_ctx, int pos, int n_prompt, int V,
                                      const int32_t *edge_beg, const int32_t *edge_tok, const int32_t *edge_next, const int32_t *def_next,
                                      const uint8_t *accept, int n_states, int32_t eot, const int32_t *starts, const uint32_t *ban_in,
                                      uint32_t *ban_out, int32_t *state_out) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(seq && starts && ban_in && ban_out && state_out, WM_ERR_INVALID, "wmdbg_constraint_state: null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && V >= 16 && n_ctx >= 1 && n_ctx <= 448 && pos >= 0 && pos < n_ctx && n_prompt >= 0 &&
                   n_prompt <= n_ctx && n_states >= 1,
               WM_ERR_INVALID, "wmdbg_constraint_state: bad geometry");
    WmCstTable t;
    WM_TRY(wm_cst_build(edge_beg, edge_tok, edge_next, def_next, accept, n_states, eot, V, &t));
    for (int b = 0; b < B; ++b)
        WM_REQUIRE(starts[b] >= -1 && starts[b] < n_states, WM_ERR_INVALID, "wmdbg_constraint_state: start of row %d", b);
    const int words = ((V + 15) / 16 * 16 + 31) / 32;
    WmCstPar cpar;
    DevPool pool;
    hipStream_t s = ctx->stream;
    const int *dseq, *dpos;
    unsigned *dban;
    int *dstate;
    WM_TRY(pool.get(&dseq, seq, (size_t)n_ctx * B * 4, s));
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&dban, ban_in, (size_t)B * words * 4, s));
    WM_TRY(pool.get(&dstate, nullptr, (size_t)B * 4, s, 0xfe));   // (0xff bytes would read -1, the dead state)
    WmCstDev cd;
    WM_TRY(stage_constraint(pool, s, t, starts, B, &cpar, &cd));
    WM_TRY(wm_constraint_state(ctx, dseq, dpos, B, n_prompt, n_ctx, V, cd, dban, words, dstate));
    WM_HIP(hipMemcpyAsync(ban_out, dban, (size_t)B * words * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(state_out, dstate, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

extern "C" int wmdbg_sb_expand_tables(const int32_t *tokens, const int32_t *seq_offsets, const float *bias, const uint8_t *boost_prefixes,
                                      const int32_t *table_offsets, int n_tables, int32_t eot, int V, int32_t *counts_out,
                                      int32_t *tab_grp_out, int32_t *grp_id_out, int32_t *grp_beg_out, int32_t *ent_len_out,
                                      float *ent_bias_out, int32_t *ent_ctx_out) {
    WM_REQUIRE(counts_out && V >= 1, WM_ERR_INVALID, "wmdbg_sb_expand_tables: null counts / V < 1");
    WM_REQUIRE(n_tables <= 0 || n_tables > WM_MAX_BIAS_TABLES || (table_offsets && table_offsets[n_tables] >= 0), WM_ERR_INVALID,
               "wmdbg_sb_expand_tables: bad table_offsets");
    WmSbPool p;
    WM_TRY(wm_sb_expand_tables(tokens, seq_offsets, bias, boost_prefixes, table_offsets, n_tables,
                               n_tables > 0 && n_tables <= WM_MAX_BIAS_TABLES ? table_offsets[n_tables] : 0, eot, V, &p));
    counts_out[0] = p.n_tables(); counts_out[1] = p.t.n_groups(); counts_out[2] = p.t.n_entries();
    if (tab_grp_out) std::copy(p.tab_grp.begin(), p.tab_grp.end(), tab_grp_out);
    if (grp_id_out) std::copy(p.t.grp_id.begin(), p.t.grp_id.end(), grp_id_out);
    if (grp_beg_out) std::copy(p.t.grp_beg.begin(), p.t.grp_beg.end(), grp_beg_out);
    if (ent_len_out) std::copy(p.t.ent_len.begin(), p.t.ent_len.end(), ent_len_out);
    if (ent_bias_out) std::copy(p.t.ent_bias.begin(), p.t.ent_bias.end(), ent_bias_out);
    if (ent_ctx_out) std::copy(p.t.ent_ctx.begin(), p.t.ent_ctx.end(), ent_ctx_out);
    return WM_OK;
}

extern "C" int wmdbg_group_bias_rows(const int32_t *table_of_row, int B, const int32_t *tab_grp, int n_tables, int b0, int Cg, int N,
                                     int32_t *rng_out) {
    WM_REQUIRE(table_of_row && tab_grp && rng_out && B >= 1 && n_tables >= 0 && b0 >= 0 && Cg >= 1 && b0 + Cg <= B && N >= 1 &&
                   Cg * N <= WM_DEC_MAXB,
               WM_ERR_INVALID, "wmdbg_group_bias_rows: bad geometry");
    std::vector<int32_t> r;
    wm_group_bias_rows(table_of_row, tab_grp, n_tables, b0, Cg, N, &r);
    std::copy(r.begin(), r.end(), rng_out);
    return WM_OK;
}

extern "C" int wmdbg_group_given(const int32_t *lens, const int32_t *tokens, int stride, int rows, int b0, int Cg, int N, int32_t *lens_out,
                                  int32_t *tok_out, int tok_cap, int32_t *L_out) {
    WM_REQUIRE(lens && tokens && lens_out && tok_out && L_out && stride >= 1 && rows >= 1 && b0 >= 0 && Cg >= 1 && N >= 1 &&
                   (int64_t)(b0 + Cg) * N <= rows && Cg * N <= WM_DEC_MAXB,
               WM_ERR_INVALID, "wmdbg_group_given: bad geometry");
    for (int r = 0; r < rows; ++r) WM_REQUIRE(lens[r] >= 0 && lens[r] <= stride, WM_ERR_INVALID, "wmdbg_group_given: lens[%d]", r);
    std::vector<int32_t> gl, gt;
    const int L = wm_group_given(lens, tokens, stride, b0, Cg, N, &gl, &gt);
    WM_REQUIRE((int)gt.size() <= tok_cap, WM_ERR_INVALID, "wmdbg_group_given: %d words do not fit %d", (int)gt.size(), tok_cap);
    std::copy(gl.begin(), gl.end(), lens_out);
    std::copy(gt.begin(), gt.end(), tok_out);
    *L_out = L;
    return WM_OK;
}

extern "C" int wmdbg_seqbias_rows_state(wm_ctx *ctx, const int32_t *seq, int B, int n_ctx, int pos, int n_prompt, int V,
                                        const int32_t *tokens, const int32_t *seq_offsets, const float *bias,
                                        const uint8_t *boost_prefixes, const int32_t *table_offsets, int n_tables, int32_t eot,
                                        const int32_t *table_of_row, const uint32_t *ban_in, uint32_t *hit_out, uint32_t *ban_out,
                                        int32_t *cnt_out, int32_t *id_out, float *total_out, int32_t *woff_out) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(seq && table_of_row && hit_out && ban_out && cnt_out && id_out && total_out && woff_out, WM_ERR_INVALID,
               "wmdbg_seqbias_rows_state: null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && V >= 16 && n_ctx >= 1 && n_ctx <= 448 && pos >= 0 && pos < n_ctx && n_prompt >= 0 &&
                   n_prompt <= n_ctx,
               WM_ERR_INVALID, "wmdbg_seqbias_rows_state: bad geometry");
    WM_REQUIRE(n_tables >= 1 && n_tables <= WM_MAX_BIAS_TABLES && table_offsets && table_offsets[n_tables] >= 0, WM_ERR_INVALID,
               "wmdbg_seqbias_rows_state: bad tables");
    WmSbPool p;
    WM_TRY(wm_sb_expand_tables(tokens, seq_offsets, bias, boost_prefixes, table_offsets, n_tables, table_offsets[n_tables], eot, V, &p));
    for (int b = 0; b < B; ++b)
        WM_REQUIRE(table_of_row[b] >= -1 && table_of_row[b] < n_tables, WM_ERR_INVALID, "wmdbg_seqbias_rows_state: table of row %d", b);
    std::vector<int32_t> rng;
    wm_group_bias_rows(table_of_row, p.tab_grp.data(), n_tables, 0, B, 1, &rng);
    const int words = ((V + 15) / 16 * 16 + 31) / 32;
    const size_t cap = WM_MAX_BIAS_ENTRIES;
    const int ng = p.t.n_groups(), ne = p.t.n_entries();
    WmRepPar rpar;
    rpar.p = 1.f; rpar.inv_p = 1.f; rpar.n = 0; rpar.eot = 0;   // the bitmaps' owner with empty rules, as the product runs it
    DevPool pool;
    hipStream_t s = ctx->stream;
    const int *dseq, *dpos, *drng;
    WmRepDev rd;
    rd.words = words;
    WM_TRY(pool.get(&dseq, seq, (size_t)n_ctx * B * 4, s));
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&drng, rng.data(), rng.size() * 4, s));
    WM_TRY(pool.get(&rd.par, &rpar, sizeof(rpar), s));
    WM_TRY(pool.get(&rd.seen, nullptr, (size_t)B * words * 4, s, 0xff));
    if (ban_in) WM_TRY(pool.get(&rd.ban, ban_in, (size_t)B * words * 4, s));
    else WM_TRY(pool.get(&rd.ban, nullptr, (size_t)B * words * 4, s, 0xff));
    // the pool as the product lays it out (the kernel reads groups and entries the ranges name, nothing else)
    WmSbDev d;
    memset(&d, 0, sizeof(d));
    WM_TRY(pool.get(&d.grp_id, ng ? p.t.grp_id.data() : nullptr, std::max<size_t>(ng, 1) * 4, s));
    WM_TRY(pool.get(&d.grp_beg, p.t.grp_beg.data(), p.t.grp_beg.size() * 4, s));
    WM_TRY(pool.get(&d.ent_len, ne ? p.t.ent_len.data() : nullptr, std::max<size_t>(ne, 1) * 4, s));
    WM_TRY(pool.get(&d.ent_bias, ne ? p.t.ent_bias.data() : nullptr, std::max<size_t>(ne, 1) * 4, s));
    WM_TRY(pool.get(&d.ent_ctx, ne ? p.t.ent_ctx.data() : nullptr, std::max<size_t>(ne, 1) * WM_SB_CTX * 4, s));
    WM_TRY(pool.get(&d.e.hit, nullptr, (size_t)B * words * 4, s, 0xff));
    WM_TRY(pool.get(&d.e.cnt, nullptr, (size_t)B * 4, s, 0xff));
    WM_TRY(pool.get(&d.e.lid, nullptr, (size_t)B * cap * 4, s, 0xff));
    WM_TRY(pool.get(&d.e.ltot, nullptr, (size_t)B * cap * 4, s, 0xff));
    WM_TRY(pool.get(&d.e.woff, nullptr, (size_t)B * words * 4, s, 0xff));
    d.e.words = words;
    if (!ban_in) WM_TRY(wm_repeat_state(ctx, dseq, dpos, B, n_prompt, n_ctx, V, rd));
    WM_TRY(wm_seqbias_rows_state(ctx, dseq, dpos, B, n_prompt, n_ctx, V, d, drng, rd.ban, words));
    WM_HIP(hipMemcpyAsync(hit_out, d.e.hit, (size_t)B * words * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(ban_out, rd.ban, (size_t)B * words * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(cnt_out, d.e.cnt, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(id_out, d.e.lid, (size_t)B * cap * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(total_out, d.e.ltot, (size_t)B * cap * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(woff_out, d.e.woff, (size_t)B * words * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

extern "C" int wmdbg_repeat_state(wm_ctx *ctx, const int32_t *seq, int B, int n_ctx, int pos, int n_prompt, int V, int ngram,
                                  int32_t eot, uint32_t *seen_out, uint32_t *ban_out) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(seq && seen_out && ban_out, WM_ERR_INVALID, "wmdbg_repeat_state: null pointer");
    WM_REQUIRE(B >= 1 && B <= WM_DEC_MAXB && V >= 16 && n_ctx >= 1 && n_ctx <= 448 && pos >= 0 && pos < n_ctx && n_prompt >= 0 &&
                   n_prompt <= n_ctx && ngram >= 0 && ngram <= WM_MAX_NGRAM && eot >= 0 && eot <= V,
               WM_ERR_INVALID, "wmdbg_repeat_state: bad geometry");
    const int words = ((V + 15) / 16 * 16 + 31) / 32;
    WmRepPar rpar;
    rpar.p = 1.f; rpar.inv_p = 1.f; rpar.n = ngram; rpar.eot = eot;
    DevPool pool;
    hipStream_t s = ctx->stream;
    const int *dseq, *dpos;
    WmRepDev rd;
    rd.words = words;
    WM_TRY(pool.get(&dseq, seq, (size_t)n_ctx * B * 4, s));
    WM_TRY(pool.get(&dpos, &pos, 4, s));
    WM_TRY(pool.get(&rd.par, &rpar, sizeof(rpar), s));
    WM_TRY(pool.get(&rd.seen, nullptr, (size_t)B * words * 4, s, 0xff));   // 0xff: a word the kernel leaves alone shows
    WM_TRY(pool.get(&rd.ban, nullptr, (size_t)B * words * 4, s, 0xff));
    WM_TRY(wm_repeat_state(ctx, dseq, dpos, B, n_prompt, n_ctx, V, rd));
    WM_HIP(hipMemcpyAsync(seen_out, rd.seen, (size_t)B * words * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipMemcpyAsync(ban_out, rd.ban, (size_t)B * words * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

// ------------------------------------------------------------------ encoder GEMM: any epilogue, any row map -----------------
extern "C" int wmdbg_gemm_map_layout(int32_t *out4) {
    if (!out4) return WM_ERR_INVALID;
    out4[0] = (int32_t)sizeof(wmdbg_gemm_map); out4[1] = (int32_t)offsetof(wmdbg_gemm_map, a_off);
    out4[2] = (int32_t)offsetof(wmdbg_gemm_map, d_model); out4[3] = (int32_t)offsetof(wmdbg_gemm_map, vt_elems);
    return WM_OK;
}

namespace {
constexpr int64_t GEMM_MAP_MAX_ELEMS = (int64_t)1 << 28;   // per buffer: a test hook, not a product path
constexpr int64_t GEMM_MAP_A_SLACK = 128;                  // elements: the 256 bytes of slack behind every dalloc of model.cpp

// Every address the launch may touch, from the arguments alone.  Nothing is launched unless this returns WM_OK.
int gemm_map_check(const wmdbg_gemm_map &g, const float *A, const float *W, const float *pos, const float *C, const float *vt) {
    WM_REQUIRE(A && W && C, WM_ERR_INVALID, "wmdbg_gemm_mapped: null pointer");
    WM_REQUIRE(g.epi >= EPI_BIAS_BF16 && g.epi <= EPI_F32, WM_ERR_INVALID, "wmdbg_gemm_mapped: bad epilogue %d", g.epi);
    WM_REQUIRE(g.M >= 1 && g.M < (1 << 24) && g.N >= 1 && g.N < (1 << 20) && g.K >= 64 && g.K % 64 == 0 && g.K <= (1 << 16),
               WM_ERR_INVALID, "wmdbg_gemm_mapped: bad problem size M=%d N=%d K=%d", g.M, g.N, g.K);
    // ---- A: row m reads [off, off + K) (16-byte DMA pieces: every part of the address is a multiple of 8 elements)
    WM_REQUIRE(g.a_rpb >= 1 && g.a_rpb <= 0x7fffffffLL && g.a_off >= 0 && g.a_bstride >= 0 && g.a_rstride >= 0 && g.a_elems >= 1 &&
                   g.a_elems <= GEMM_MAP_MAX_ELEMS,
               WM_ERR_INVALID, "wmdbg_gemm_mapped: bad A map");
    WM_REQUIRE(g.a_off % 8 == 0 && g.a_bstride % 8 == 0 && g.a_rstride % 8 == 0, WM_ERR_INVALID,
               "wmdbg_gemm_mapped: A map not 16-byte aligned");
    WM_REQUIRE(g.a_bstride <= GEMM_MAP_MAX_ELEMS && g.a_rstride <= GEMM_MAP_MAX_ELEMS, WM_ERR_INVALID, "wmdbg_gemm_mapped: bad A map");
    for (int64_t m = 0; m < g.M; ++m) {
        const int64_t off = g.a_off + (m / g.a_rpb) * g.a_bstride + (m % g.a_rpb) * g.a_rstride;
        WM_REQUIRE(off + g.K <= g.a_elems + GEMM_MAP_A_SLACK, WM_ERR_INVALID,
                   "wmdbg_gemm_mapped: A row %lld reads [%lld, %lld) past a_elems %lld + slack", (long long)m, (long long)off,
                   (long long)(off + g.K), (long long)g.a_elems);
    }
    // ---- the epilogue's own geometry
    if (g.epi == EPI_XKV || g.epi == EPI_QKV_ENC) {
        WM_REQUIRE(g.batch >= 1 && g.seq >= 1 && g.n_head >= 1 && g.d_model == 64 * g.n_head && (int64_t)g.batch * g.seq == g.M,
                   WM_ERR_INVALID, "wmdbg_gemm_mapped: need M == batch * seq and d_model == 64 * n_head");
    }
    if (g.epi == EPI_XKV) {
        WM_REQUIRE(g.N == 2 * g.d_model, WM_ERR_INVALID, "wmdbg_gemm_mapped: EPI_XKV needs N == 2 * d_model");
        WM_REQUIRE(g.c_elems == (int64_t)2 * g.batch * g.n_head * g.seq * 64, WM_ERR_INVALID,
                   "wmdbg_gemm_mapped: EPI_XKV needs c_elems == 2 * batch * n_head * seq * 64");
        WM_REQUIRE(g.c_elems <= GEMM_MAP_MAX_ELEMS, WM_ERR_INVALID, "wmdbg_gemm_mapped: C too large");
        return WM_OK;   // (the scatter does not use the C row map)
    }
    int64_t width = g.N;   // columns of a C row that the epilogue writes
    if (g.epi == EPI_QKV_ENC) {
        WM_REQUIRE(vt, WM_ERR_INVALID, "wmdbg_gemm_mapped: EPI_QKV_ENC needs vt");
        WM_REQUIRE(g.N == 3 * g.d_model, WM_ERR_INVALID, "wmdbg_gemm_mapped: EPI_QKV_ENC needs N == 3 * d_model");
        WM_REQUIRE(g.seq_pad % 16 == 0 && g.seq_pad >= g.seq, WM_ERR_INVALID,
                   "wmdbg_gemm_mapped: EPI_QKV_ENC needs seq_pad %% 16 == 0 and seq_pad >= seq");
        WM_REQUIRE(g.vt_elems == (int64_t)g.batch * g.n_head * 64 * g.seq_pad && g.vt_elems <= GEMM_MAP_MAX_ELEMS, WM_ERR_INVALID,
                   "wmdbg_gemm_mapped: EPI_QKV_ENC needs vt_elems == batch * n_head * 64 * seq_pad");
        width = 2 * g.d_model;
    }
    WM_REQUIRE(g.c_rpb >= 1 && g.c_rpb <= 0x7fffffffLL && g.c_off >= 0 && g.c_bstride >= 0 && g.c_elems >= 1 &&
                   g.c_elems <= GEMM_MAP_MAX_ELEMS && g.c_rstride <= GEMM_MAP_MAX_ELEMS && g.c_bstride <= GEMM_MAP_MAX_ELEMS,
               WM_ERR_INVALID, "wmdbg_gemm_mapped: bad C map");
    WM_REQUIRE(g.c_rstride >= width && (g.M <= g.c_rpb || g.c_bstride >= g.c_rpb * g.c_rstride), WM_ERR_INVALID,
               "wmdbg_gemm_mapped: C rows overlap (c_rstride >= N, c_bstride >= c_rpb * c_rstride)");
    if (g.N % 64 == 0) {   // the staged epilogues store 16 bytes per lane
        const int al = (g.epi == EPI_RESID_F32 || g.epi == EPI_CONV2_F32 || g.epi == EPI_F32) ? 4 : 8;
        WM_REQUIRE(g.c_off % al == 0 && g.c_bstride % al == 0 && g.c_rstride % al == 0, WM_ERR_INVALID,
                   "wmdbg_gemm_mapped: C map not 16-byte aligned");
    }
    for (int64_t m = 0; m < g.M; ++m) {
        const int64_t off = g.c_off + (m / g.c_rpb) * g.c_bstride + (m % g.c_rpb) * g.c_rstride;
        WM_REQUIRE(off + width <= g.c_elems, WM_ERR_INVALID, "wmdbg_gemm_mapped: C row %lld writes [%lld, %lld) past c_elems %lld",
                   (long long)m, (long long)off, (long long)(off + width), (long long)g.c_elems);
    }
    if (g.epi == EPI_CONV2_F32) {
        WM_REQUIRE(pos, WM_ERR_INVALID, "wmdbg_gemm_mapped: EPI_CONV2_F32 needs pos [c_rpb][N]");
        WM_REQUIRE(g.c_rpb * g.N <= GEMM_MAP_MAX_ELEMS, WM_ERR_INVALID, "wmdbg_gemm_mapped: pos too large");
    }
    return WM_OK;
}
}  // namespace

extern "C" int wmdbg_gemm_mapped(wm_ctx *ctx, const wmdbg_gemm_map *map, const float *A, const float *W, const float *bias,
                                 const float *pos, float *C, float *vt) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(map, WM_ERR_INVALID, "wmdbg_gemm_mapped: null map");
    const wmdbg_gemm_map g = *map;
    WM_TRY(gemm_map_check(g, A, W, pos, C, vt));
    const bool f32out = g.epi == EPI_F32 || g.epi == EPI_RESID_F32 || g.epi == EPI_CONV2_F32;
    std::vector<bf16_t> a16, w16, c16, vt16;
    std::vector<float> c32;
    to_bf16(A, a16, (size_t)g.a_elems);
    to_bf16(W, w16, (size_t)g.N * g.K);
    DevPool pool;
    hipStream_t s = ctx->stream;
    GemmArgs ga;
    memset(&ga, 0, sizeof(ga));
    void *dC;   // f32 or bf16 by the epilogue
    WM_TRY(pool.get(&ga.A, a16.data(), a16.size() * 2, s));
    WM_TRY(pool.get(&ga.W, w16.data(), w16.size() * 2, s));
    if (bias) WM_TRY(pool.get(&ga.bias, bias, (size_t)g.N * 4, s));
    if (g.epi == EPI_CONV2_F32) WM_TRY(pool.get(&ga.pos, pos, (size_t)g.c_rpb * g.N * 4, s));
    if (g.epi == EPI_RESID_F32) {
        WM_TRY(pool.get(&dC, C, (size_t)g.c_elems * 4, s));   // in / out
    } else if (f32out) {
        fill_f32(c32, (size_t)g.c_elems);
        WM_TRY(pool.get(&dC, c32.data(), c32.size() * 4, s));
    } else {
        fill_bf16(c16, (size_t)g.c_elems);
        WM_TRY(pool.get(&dC, c16.data(), c16.size() * 2, s));
    }
    if (g.epi == EPI_QKV_ENC) {
        fill_bf16(vt16, (size_t)g.vt_elems);
        WM_TRY(pool.get(&ga.vt, vt16.data(), vt16.size() * 2, s));
    }
    ga.A += g.a_off; ga.a_rpb = (long)g.a_rpb; ga.a_bstride = (long)g.a_bstride; ga.a_rstride = (long)g.a_rstride;
    ga.C = f32out ? (void *)((float *)dC + g.c_off) : (void *)((bf16_t *)dC + g.c_off);
    ga.c_rpb = (long)g.c_rpb; ga.c_bstride = (long)g.c_bstride; ga.c_rstride = (long)g.c_rstride;
    ga.M = g.M; ga.N = g.N; ga.K = g.K; ga.epi = g.epi;
    ga.d_model = g.d_model; ga.n_head = g.n_head; ga.seq = g.seq; ga.seq_pad = g.seq_pad; ga.batch = g.batch;
    if (g.epi == EPI_XKV) { ga.C = dC; ga.c_rpb = (long)g.M + 1; }   // (the scatter ignores the C map; wm_gemm wants c_rpb > 0)
    WM_TRY(wm_gemm(ctx, ga));
    if (f32out) {
        WM_HIP(hipMemcpyAsync(C, dC, (size_t)g.c_elems * 4, hipMemcpyDeviceToHost, s));
        WM_HIP(hipStreamSynchronize(s));
    } else {
        WM_TRY(down_bf16(dC, (size_t)g.c_elems, C, s));
    }
    if (g.epi == EPI_QKV_ENC) WM_TRY(down_bf16(ga.vt, (size_t)g.vt_elems, vt, s));
    return WM_OK;
}

// ------------------------------------------------------------------ the product's own encoder-side launches on a loaded model
namespace {
int model_ready(wm_ctx *ctx, int B, const char *who) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(ctx->model && ctx->model->finalized, WM_ERR_STATE, "%s: model weights not finalised (wm_finalize)", who);
    WM_REQUIRE(B >= 1 && B <= 16, WM_ERR_INVALID, "%s: B must be 1..16", who);
    return wm_model_reserve(ctx, B);
}
}  // namespace

extern "C" int wmdbg_encode_stem(wm_ctx *ctx, const float *mel, const int64_t *wins, int B, float *mel_t_out, float *h1p_out,
                                 float *x_out) {
    WM_REQUIRE(mel && mel_t_out && h1p_out && x_out, WM_ERR_INVALID, "wmdbg_encode_stem: null pointer");
    WM_TRY(model_ready(ctx, B, "wmdbg_encode_stem"));
    WmModel *m = ctx->model;
    const int C = m->dims.n_mels, d = m->dims.n_audio_state;
    size_t mel_elems = (size_t)B * C * WM_N_FRAMES;
    std::vector<WmMelWin> win;
    if (wins) {   // every read of the window kernel: mel[base + c * T + seek + t], c < C, t < n
        mel_elems = 0;
        win.resize(B);
        for (int b = 0; b < B; ++b) {
            const int64_t base = wins[b * 4], T = wins[b * 4 + 1], seek = wins[b * 4 + 2], n = wins[b * 4 + 3];
            WM_REQUIRE(base >= 0 && base <= ((int64_t)1 << 28) && T >= 1 && T <= (1 << 22) && seek >= 0 && n >= 0 && n <= WM_N_FRAMES &&
                           seek + n <= T,
                       WM_ERR_INVALID, "wmdbg_encode_stem: window %d (base %lld, T %lld, seek %lld, n %lld) leaves its block", b,
                       (long long)base, (long long)T, (long long)seek, (long long)n);
            win[b].base = base; win[b].T = (int)T; win[b].seek = (int)seek; win[b].n = (int)n; win[b].pad = 0;
            mel_elems = std::max(mel_elems, (size_t)(base + (int64_t)C * T));
        }
    }
    // sentinels in everything the three launches must write; the guard rows (mel_t rows 0 and 3001, h1p row 0) stay as the
    // allocation left them
    std::vector<bf16_t> s16;
    std::vector<float> s32;
    fill_bf16(s16, (size_t)3000 * std::max(C, d));
    fill_f32(s32, (size_t)B * 1500 * d);
    DevPool pool;
    hipStream_t s = ctx->stream;
    const float *dmel;
    const WmMelWin *dwin = nullptr;
    WM_TRY(pool.get(&dmel, mel, mel_elems * 4, s));
    if (wins) WM_TRY(pool.get(&dwin, win.data(), win.size() * sizeof(WmMelWin), s));
    for (int b = 0; b < B; ++b) {
        WM_HIP(hipMemcpyAsync(m->mel_t + ((size_t)b * 3002 + 1) * C, s16.data(), (size_t)3000 * C * 2, hipMemcpyHostToDevice, s));
        WM_HIP(hipMemcpyAsync(m->h1p + ((size_t)b * 3001 + 1) * d, s16.data(), (size_t)3000 * d * 2, hipMemcpyHostToDevice, s));
    }
    WM_HIP(hipMemcpyAsync(m->x, s32.data(), s32.size() * 4, hipMemcpyHostToDevice, s));
    WM_TRY(wm_model_encode_stem(ctx, dmel, dwin, B));
    WM_TRY(down_bf16(m->mel_t, (size_t)B * 3002 * C, mel_t_out, s));
    WM_TRY(down_bf16(m->h1p, (size_t)B * 3001 * d, h1p_out, s));
    WM_HIP(hipMemcpyAsync(x_out, m->x, (size_t)B * 1500 * d * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return WM_OK;
}

extern "C" int wmdbg_encode_layer_qkv(wm_ctx *ctx, int layer, const float *x, int B, float *xn_out, float *qk_out, float *vt_out) {
    WM_REQUIRE(x && xn_out && qk_out && vt_out, WM_ERR_INVALID, "wmdbg_encode_layer_qkv: null pointer");
    WM_TRY(model_ready(ctx, B, "wmdbg_encode_layer_qkv"));
    WmModel *m = ctx->model;
    WM_REQUIRE(layer >= 0 && layer < m->dims.n_audio_layer, WM_ERR_INVALID, "wmdbg_encode_layer_qkv: layer %d out of range", layer);
    const int d = m->dims.n_audio_state, H = m->dims.n_audio_head;
    const size_t M = (size_t)B * 1500, vt_n = (size_t)B * H * 64 * 1536;
    hipStream_t s = ctx->stream;
    std::vector<bf16_t> s16;
    fill_bf16(s16, std::max(vt_n, M * 2 * d));
    WM_HIP(hipMemcpyAsync(m->x, x, M * d * 4, hipMemcpyHostToDevice, s));
    WM_HIP(hipMemcpyAsync(m->xn, s16.data(), M * d * 2, hipMemcpyHostToDevice, s));
    WM_HIP(hipMemcpyAsync(m->qk, s16.data(), M * 2 * d * 2, hipMemcpyHostToDevice, s));
    WM_HIP(hipMemcpyAsync(m->vt, s16.data(), vt_n * 2, hipMemcpyHostToDevice, s));
    int rc = wm_model_encode_layer_qkv(ctx, layer, B);
    if (rc == WM_OK) rc = down_bf16(m->xn, M * d, xn_out, s);
    if (rc == WM_OK) rc = down_bf16(m->qk, M * 2 * d, qk_out, s);
    if (rc == WM_OK) rc = down_bf16(m->vt, vt_n, vt_out, s);
    // the pad columns 1500 .. 1535 of vt are zero in the product (zeroed at allocation, never written): as a later encode expects
    WM_HIP(hipMemsetAsync(m->vt, 0, vt_n * 2, s));
    WM_HIP(hipStreamSynchronize(s));
    return rc;
}

extern "C" int wmdbg_encode_layer_tail(wm_ctx *ctx, int layer, const float *x, int B, float *att_out, float *x_mid_out,
                                       float *xn2_out, float *hid_out, float *x_out) {
    WM_REQUIRE(x && att_out && x_mid_out && xn2_out && hid_out && x_out, WM_ERR_INVALID, "wmdbg_encode_layer_tail: null pointer");
    WM_TRY(model_ready(ctx, B, "wmdbg_encode_layer_tail"));
    WmModel *m = ctx->model;
    WM_REQUIRE(layer >= 0 && layer < m->dims.n_audio_layer, WM_ERR_INVALID, "wmdbg_encode_layer_tail: layer %d out of range", layer);
    const int d = m->dims.n_audio_state, H = m->dims.n_audio_head;
    const size_t M = (size_t)B * 1500, vt_n = (size_t)B * H * 64 * 1536;
    std::vector<bf16_t> s16;
    std::vector<float> s32;
    fill_bf16(s16, M * 4 * d);
    fill_f32(s32, M * d);
    DevPool pool;
    hipStream_t s = ctx->stream;
    float *dmid;
    WM_TRY(pool.get(&dmid, s32.data(), M * d * 4, s));
    // sentinels in everything the launches must write; vt is zeroed instead: its pad columns 1500 .. 1535 are the attention
    // kernel's contract (zeroed at allocation, never written), and the live columns are all written by the QKV launch
    WM_HIP(hipMemcpyAsync(m->x, x, M * d * 4, hipMemcpyHostToDevice, s));
    WM_HIP(hipMemcpyAsync(m->xn, s16.data(), M * d * 2, hipMemcpyHostToDevice, s));
    WM_HIP(hipMemcpyAsync(m->qk, s16.data(), (M + 64) * 2 * d * 2, hipMemcpyHostToDevice, s));   // and the 64 rows the last K tile over-reads
    WM_HIP(hipMemcpyAsync(m->att, s16.data(), M * d * 2, hipMemcpyHostToDevice, s));
    WM_HIP(hipMemcpyAsync(m->hid, s16.data(), M * 4 * d * 2, hipMemcpyHostToDevice, s));
    WM_HIP(hipMemsetAsync(m->vt, 0, vt_n * 2, s));
    int rc = wm_model_encode_layer_qkv(ctx, layer, B);
    if (rc == WM_OK) rc = wm_model_encode_layer_tail(ctx, layer, B, dmid);
    if (rc == WM_OK) rc = down_bf16(m->att, M * d, att_out, s);
    if (rc == WM_OK) rc = down_bf16(m->xn, M * d, xn2_out, s);
    if (rc == WM_OK) rc = down_bf16(m->hid, M * 4 * d, hid_out, s);
    if (rc == WM_OK) {
        WM_HIP(hipMemcpyAsync(x_mid_out, dmid, M * d * 4, hipMemcpyDeviceToHost, s));
        WM_HIP(hipMemcpyAsync(x_out, m->x, M * d * 4, hipMemcpyDeviceToHost, s));
    }
    WM_HIP(hipMemsetAsync(m->qk + M * 2 * d, 0, (size_t)64 * 2 * d * 2, s));   // the over-read rows as the allocation left them
    WM_HIP(hipStreamSynchronize(s));
    return rc;
}

extern "C" int wmdbg_encode_post(wm_ctx *ctx, const float *x, int B, float *xn_out, float *xa_out) {
    WM_REQUIRE(x && xn_out && xa_out, WM_ERR_INVALID, "wmdbg_encode_post: null pointer");
    WM_TRY(model_ready(ctx, B, "wmdbg_encode_post"));
    WmModel *m = ctx->model;
    const int d = m->dims.n_audio_state;
    const size_t M = (size_t)B * 1500;
    std::vector<bf16_t> s16;
    std::vector<float> s32;
    fill_bf16(s16, M * d);
    fill_f32(s32, M * d);
    hipStream_t s = ctx->stream;
    WM_HIP(hipMemcpyAsync(m->x, x, M * d * 4, hipMemcpyHostToDevice, s));
    WM_HIP(hipMemcpyAsync(m->xn, s16.data(), M * d * 2, hipMemcpyHostToDevice, s));
    WM_HIP(hipMemcpyAsync(m->xa_f32, s32.data(), M * d * 4, hipMemcpyHostToDevice, s));
    int rc = wm_model_encode_post(ctx, B, nullptr);
    if (rc == WM_OK) rc = down_bf16(m->xn, M * d, xn_out, s);
    if (rc == WM_OK) WM_HIP(hipMemcpyAsync(xa_out, m->xa_f32, M * d * 4, hipMemcpyDeviceToHost, s));
    WM_HIP(hipStreamSynchronize(s));
    return rc;
}

extern "C" int wmdbg_cross_kv(wm_ctx *ctx, const float *xa, int B, float *xkv_out) {
    WM_REQUIRE(xa && xkv_out, WM_ERR_INVALID, "wmdbg_cross_kv: null pointer");
    WM_TRY(model_ready(ctx, B, "wmdbg_cross_kv"));
    WmModel *m = ctx->model;
    const wm_dims &D = m->dims;
    WM_REQUIRE(D.n_text_state == D.n_audio_state, WM_ERR_INVALID, "wmdbg_cross_kv: encoder and decoder widths differ");
    const int d = D.n_text_state, H = D.n_text_head;
    const size_t M = (size_t)B * 1500, used = (size_t)D.n_text_layer * 2 * B * H * 1500 * 64,
                 cap = (size_t)D.n_text_layer * 2 * m->cap_b * H * 1500 * 64;   // the whole allocation (wm_model_reserve)
    std::vector<bf16_t> s16, got(cap);
    fill_bf16(s16, cap);
    DevPool pool;
    hipStream_t s = ctx->stream;
    const float *dxa;
    WM_TRY(pool.get(&dxa, xa, M * d * 4, s));
    WM_HIP(hipMemcpyAsync(m->xkv, s16.data(), cap * 2, hipMemcpyHostToDevice, s));
    int rc = wm_model_set_xa(ctx, dxa, B);
    if (rc == WM_OK) rc = wm_model_cross_kv(ctx, B);
    WM_HIP(hipMemcpyAsync(got.data(), m->xkv, cap * 2, hipMemcpyDeviceToHost, s));
    if (cap > used) WM_HIP(hipMemsetAsync(m->xkv + used, 0, (cap - used) * 2, s));
    WM_HIP(hipStreamSynchronize(s));
    WM_TRY(rc);
    size_t disturbed = 0;
    for (size_t i = used; i < cap; ++i) disturbed += got[i] != (bf16_t)WMDBG_SENTINEL_BF16;
    WM_REQUIRE(disturbed == 0, WM_ERR_STATE, "wmdbg_cross_kv: %zu elements behind the %d chunks' cache were written", disturbed, B);
    got.resize(used);
    from_bf16(got, xkv_out);
    return WM_OK;
}

// ---------------------------------------------------------------- live streams (streams.cpp)
#include "streams.h"

extern "C" int wmdbg_streams_set_position(wm_ctx *ctx, wm_streams *st, int s, int64_t n_samples) {
    WM_TRY(wm_ctx_make_current(ctx));
    WM_REQUIRE(st != nullptr, WM_ERR_INVALID, "wmdbg_streams_set_position: null set");
    WM_REQUIRE(st->device == ctx->device, WM_ERR_STATE, "wmdbg_streams_set_position: the set lives on another device");
    WM_REQUIRE(s >= 0 && s < st->S, WM_ERR_INVALID, "wmdbg_streams_set_position: stream %d outside 0 .. %d", s, st->S - 1);
    WM_REQUIRE(n_samples >= 0, WM_ERR_INVALID, "wmdbg_streams_set_position: negative position");
    WM_REQUIRE(st->n[s] == 0, WM_ERR_STATE, "wmdbg_streams_set_position: stream %d is not empty", s);
    WM_HIP(hipMemsetAsync(st->carry + (size_t)s * WM_STREAM_CARRY, 0, sizeof(float) * WM_STREAM_CARRY, ctx->stream));
    st->n[s] = n_samples;
    st->floor[s] = wm_stream_final(n_samples);
    st->reflect[s] = n_samples == 0;
    st->stale[s] = n_samples > 0;
    return WM_OK;
}

extern "C" int wmdbg_streams_min_capacity(int capacity_frames) {
    if (capacity_frames == 0) g_wm_stream_min_capacity = WM_STREAM_MIN_CAPACITY;
    else if (capacity_frames >= WM_STREAM_FPB && capacity_frames <= WM_STREAM_MIN_CAPACITY) g_wm_stream_min_capacity = capacity_frames;
    return g_wm_stream_min_capacity;
}
