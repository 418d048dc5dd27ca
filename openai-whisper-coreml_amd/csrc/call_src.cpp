// call_src.cpp -- the checks and stagers of a call's audio source (call_src.h): PCM chunks, mel windows, or the rows of an
// encoded window set.  Shared by the transcribe calls (transcribe.cpp) and by alignment and window sets (model_api.cpp).
#include "call_src.h"

#include <string.h>

static size_t pcm_elem(wm_dtype t) { return t == WM_I16 ? 2 : t == WM_F32 ? 4 : 8; }

// row b of a mel source: its window lies inside its block (`who` prefixes the message; align bounds n_frames tighter itself)
int wm_check_window(const WmAudioSrc &a, int b, const char *who) {
    WM_REQUIRE(a.mel_base[b] >= 0 && a.mel_len[b] >= 1 && a.seek[b] >= 0 && a.n_frames[b] >= 1 &&
                   a.n_frames[b] <= WM_N_FRAMES && (int64_t)a.seek[b] + a.n_frames[b] <= a.mel_len[b],
               WM_ERR_INVALID, "%srow %d: window (base %lld, T %d, seek %d, n_frames %d) invalid", who, b,
               (long long)a.mel_base[b], a.mel_len[b], a.seek[b], a.n_frames[b]);
    return WM_OK;
}

// the pointers of a window source: the five of a mel call, or the set
int wm_check_src_pointers(const WmAudioSrc &a) {
    if (a.windows) {
        WM_REQUIRE(a.set != nullptr, WM_ERR_INVALID, "null window set");
        return WM_OK;
    }
    WM_REQUIRE(a.mel && a.mel_base && a.mel_len && a.seek && a.n_frames, WM_ERR_INVALID, "null mel / window pointer");
    return WM_OK;
}

// a set may be read by the context that made it and by every context that shares that one's weights
int wm_check_set_owner(const wm_ctx *ctx, const wm_windows *w) {
    const WmModel *m = ctx->model;
    WM_REQUIRE(!ctx->dbg_hooks, WM_ERR_STATE, "window sets are not supported by the all-f32 precision path");
    WM_REQUIRE(w->device == ctx->device && w->weights == (const void *)m->tok_emb && memcmp(&w->dims, &m->dims, sizeof(wm_dims)) == 0,
               WM_ERR_INVALID, "the window set was made for another model, device or dims");
    return WM_OK;
}

// the B rows of a call that reads a set: every one a window of the set, made for this context's weights
int wm_check_set_rows(const wm_ctx *ctx, const WmAudioSrc &a, int B, const char *who) {
    WM_REQUIRE(a.set != nullptr, WM_ERR_INVALID, "%snull window set", who);
    WM_TRY(wm_check_set_owner(ctx, a.set));
    const int W = a.set->W;
    WM_REQUIRE(a.rows || B == W, WM_ERR_INVALID, "%srows is NULL: B (%d) must be the set's %d windows", who, B, W);
    for (int b = 0; a.rows && b < B; ++b)
        WM_REQUIRE(a.rows[b] >= 0 && a.rows[b] < W, WM_ERR_INVALID, "%srow %d: window %d outside the set's [0, %d)", who, b, a.rows[b], W);
    return WM_OK;
}

// *d_pcm = the PCM of rows [b0, b0 + Bg) in device memory: the caller's, or (host memory) uploaded into m->pcm_stage.
// Null for a mel source and for a window set.
int wm_stage_pcm(wm_ctx *c, const WmAudioSrc &a, int b0, int Bg, wm_mem mem, const void **d_pcm) {
    WmModel *m = c->model;
    *d_pcm = nullptr;
    if (a.mel || a.windows) return WM_OK;
    const size_t row = WM_N_SAMPLES * pcm_elem(a.pcm_dtype);
    *d_pcm = (const char *)a.pcm + (size_t)b0 * row;
    if (mem != WM_MEM_HOST) return WM_OK;
    WM_TRY(m->pcm_stage.reserve(c->stream, (size_t)Bg * row));
    WM_HIP(hipMemcpyAsync(m->pcm_stage.p, *d_pcm, (size_t)Bg * row, hipMemcpyHostToDevice, c->stream));
    *d_pcm = m->pcm_stage.p;
    return WM_OK;
}

// The encoder input (enc_mel, enc_win) of rows [b0, b0 + Bg), to be called after wm_model_reserve.  PCM: the log-mel front
// end (f32 fast path) of d_pcm into m->mel_f32, output stays in HBM, no windows.  Mel windows: the table `win` -- the
// CALLER's, it is the source of an asynchronous upload -- in m->dmel_win, gathered by the encoder's first step from the
// caller's device memory; with host memory only the windows are copied, into the front end's buffer.
int wm_stage_mel(wm_ctx *c, const WmAudioSrc &a, int b0, int Bg, wm_mem mem, const void *d_pcm, std::vector<WmMelWin> &win,
              const float **enc_mel, const WmMelWin **enc_win) {
    WmModel *m = c->model;
    const int C = m->dims.n_mels;
    *enc_mel = m->mel_f32;
    *enc_win = nullptr;
    if (!a.mel) return wm_frontend_run(&c->fe, &c->prof, c->stream, d_pcm, a.pcm_dtype, Bg, C, m->mel_f32, WM_F32);
    win.resize(Bg);
    for (int b = 0; b < Bg; ++b) {
        const int r = b0 + b;
        WmMelWin &w = win[b];
        w.T = a.mel_len[r]; w.seek = a.seek[r]; w.n = a.n_frames[r]; w.pad = 0;
        w.base = a.mel_base[r];
        if (mem == WM_MEM_HOST) {
            WM_HIP(hipMemcpy2DAsync(m->mel_f32 + (size_t)b * C * WM_N_FRAMES, WM_N_FRAMES * sizeof(float),
                                    a.mel + w.base + w.seek, (size_t)w.T * sizeof(float), (size_t)w.n * sizeof(float),
                                    C, hipMemcpyHostToDevice, c->stream));
            w.base = (long long)b * C * WM_N_FRAMES; w.T = WM_N_FRAMES; w.seek = 0;
        }
    }
    WM_HIP(hipMemcpyAsync(m->dmel_win, win.data(), (size_t)Bg * sizeof(WmMelWin), hipMemcpyHostToDevice, c->stream));
    if (mem != WM_MEM_HOST) *enc_mel = a.mel;
    *enc_win = m->dmel_win;
    return WM_OK;
}

// The cross-attention K/V of rows [b0, b0 + Bg) of a call in m->xkv ([L][2][Bg][H][1500][64]), to be called after
// wm_model_reserve.  PCM / mel windows: stage_mel, `staged` recorded, the encoder, wm_model_cross_kv.  A window set: the
// rows' slabs copied from the set's store in one launch -- `map` is the CALLER's, the source of the asynchronous upload of
// the row map --, then `staged`: there is no encoder stage.
int wm_stage_cross_kv(wm_ctx *c, const WmAudioSrc &a, int b0, int Bg, wm_mem mem, const void *d_pcm, std::vector<WmMelWin> &win,
                   std::vector<int32_t> &map, hipEvent_t staged) {
    WmModel *m = c->model;
    if (a.windows) {
        const wm_dims &D = m->dims;
        map.resize(Bg);
        for (int b = 0; b < Bg; ++b) map[b] = a.rows ? a.rows[b0 + b] : b0 + b;
        WM_HIP(hipMemcpyAsync(m->dxkv_rows, map.data(), (size_t)Bg * 4, hipMemcpyHostToDevice, c->stream));
        WM_TRY(wm_xkv_rows(c, m->xkv, Bg, a.set->store, m->dxkv_rows, 0, Bg, 2 * D.n_text_layer, (long)D.n_text_head * 1500 * 64,
                           false));
        if (staged) WM_HIP(hipEventRecord(staged, c->stream));
        return WM_OK;
    }
    const float *enc_mel;
    const WmMelWin *enc_win;
    WM_TRY(wm_stage_mel(c, a, b0, Bg, mem, d_pcm, win, &enc_mel, &enc_win));
    if (staged) WM_HIP(hipEventRecord(staged, c->stream));
    WM_TRY(wm_model_encode_win(c, enc_mel, enc_win, Bg, nullptr));
    return wm_model_cross_kv(c, Bg);
}
