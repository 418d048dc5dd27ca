// beam.h -- the selection rule of one beam-search step (wm_transcribe_mel_beam), host and device: the select kernel of
// beam.hip and the debug library's wmdbg_beam_select (which the CPU tests compare with a numpy restatement) run the same code.
//
// openai-whisper's BeamSearchDecoder.update (whisper/decoding.py) for ONE window with N beams.  Every live beam j brings its
// running sum (f32) and its list: its <= N + 1 best admissible tokens with their log-probs, best first.  A candidate's score
// is f32(sum_j + lp).  The candidates are walked in score order -- ties: the lower beam, then the earlier list entry, which
// is what Python's stable sort of the (beam-major) candidate list gives.  Because a list is sorted and an f32 add is
// monotone, a beam's candidates are already in score order, so the walk is an N-way merge of the lists' heads.  A candidate
// whose token is `eot` is a newly finished hypothesis; any other becomes the next beam 0, 1, ... until N are taken, where the
// walk stops.  Slots that stay empty are DEAD beams: sum -inf, token `pad`, source = the slot itself; a dead beam brings no
// candidates.  Of the newly finished hypotheses the first `room` (in walk order) are kept.
#pragma once
#include <math.h>

#include "../../include/whisper_mi355x.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WM_BEAM_FN __host__ __device__ static inline
#else
#define WM_BEAM_FN static inline
#endif

#define WM_BEAM_LIST (WM_MAX_BEAM + 1)   // list entries per beam

struct WmBeamStep {
    // the next beams: slot k continues beam src[k] with token tok[k] (log-prob lp[k]), running sum sum[k]; n_next taken
    int n_next;
    int src[WM_MAX_BEAM], tok[WM_MAX_BEAM];
    float lp[WM_MAX_BEAM], sum[WM_MAX_BEAM];
    // the newly finished hypotheses that are kept: beam fin_src[f] followed by eot (log-prob fin_lp[f]), sum fin_sum[f]
    int n_fin;
    int fin_src[WM_MAX_BEAM];
    float fin_lp[WM_MAX_BEAM], fin_sum[WM_MAX_BEAM];
};

// n_from: the beams that contribute (1 at the first generated token, where all beams are equal; else N).
// sum [N], list_n [N], list_tok / list_lp [N][WM_BEAM_LIST].  eot < 0: nothing finishes.  room: finished hypotheses the
// window still takes (<= 0: none).
WM_BEAM_FN void wm_beam_select(int N, int n_from, int eot, int pad, int room, const float *sum, const int *list_n,
                               const int *list_tok, const float *list_lp, WmBeamStep *o) {
    int ptr[WM_MAX_BEAM];
    for (int j = 0; j < WM_MAX_BEAM; ++j) ptr[j] = 0;
    o->n_next = 0;
    o->n_fin = 0;
    while (o->n_next < N) {
        int bj = -1;
        float bs = 0.f;
        for (int j = 0; j < n_from; ++j) {
            if (sum[j] == -INFINITY || ptr[j] >= list_n[j]) continue;   // dead, or its list is used up
            const float s = sum[j] + list_lp[j * WM_BEAM_LIST + ptr[j]];
            if (bj < 0 || s > bs) { bj = j; bs = s; }
        }
        if (bj < 0) break;
        const int e = bj * WM_BEAM_LIST + ptr[bj];
        ++ptr[bj];
        if (eot >= 0 && list_tok[e] == eot) {
            if (o->n_fin < room) {
                o->fin_src[o->n_fin] = bj; o->fin_lp[o->n_fin] = list_lp[e]; o->fin_sum[o->n_fin] = bs;
                ++o->n_fin;
            }
        } else {
            const int k = o->n_next++;
            o->src[k] = bj; o->tok[k] = list_tok[e]; o->lp[k] = list_lp[e]; o->sum[k] = bs;
        }
    }
    for (int k = o->n_next; k < N; ++k) {
        o->src[k] = k; o->tok[k] = pad; o->lp[k] = 0.f; o->sum[k] = -INFINITY;
    }
}

// Finalize: the live beams (sum > -inf) in descending-sum order, ties to the lower beam; order_out [N], returns their count.
WM_BEAM_FN int wm_beam_fill_order(int N, const float *sum, int *order_out) {
    int n = 0;
    for (int j = 0; j < N; ++j) {
        if (sum[j] == -INFINITY) continue;
        int p = n++;
        while (p > 0 && sum[order_out[p - 1]] < sum[j]) { order_out[p] = order_out[p - 1]; --p; }
        order_out[p] = j;
    }
    return n;
}

// Where the capture rows of ONE hypothesis of a window lie (an aligned beam group, wm_transcribe_mel_beam_aligned).  The rows
// of the group keep their capture slots while the search re-parents its beams, and records its ancestry: anc[gi * anc_stride
// + k] is the beam that slot k continued at close gi (WmBeamStep::src; `anc` points at the window's beam 0), fin_src[f] the
// beam finished hypothesis f continued.  h indexes the window's hypotheses in their output order: the fin_n finished ones as
// they finished, then the live beams by descending sum until there are N.  S = sot_tail - 1 capture rows lie in front of the
// one whose output is generated token 0.  With slot_after[gi] the beam that holds the hypothesis after close gi, capture row
// S + 1 + gi (the step that is fed token gi) lies in slot_after[gi], and slot_after[gi - 1] = anc[gi][slot_after[gi]]; a
// live beam k of wsteps tokens starts the walk at slot_after[wsteps - 1] = k, a finished hypothesis of len tokens (its eot
// counted) at slot_after[len - 2] = fin_src; rows 0 .. S -- the prompt, where all beams are equal -- take the slot the walk
// ends in.  Rows behind the hypothesis' own take the slot the walk starts in (no alignment reads them).  Fills slot [Tq] and
// returns the hypothesis' length, or -1 when the window has no hypothesis h.  Pure.
WM_BEAM_FN int wm_beam_ancestry(int N, const int *anc, int anc_stride, int fin_n, const int *fin_src, const int *fin_len, int wsteps,
                                const float *sum, int h, int S, int Tq, int *slot) {
    int k, gi, len;
    if (h < 0) return -1;
    if (h < fin_n) {
        k = fin_src[h]; len = fin_len[h]; gi = len - 2;
    } else {
        int order[WM_MAX_BEAM];
        const int n_live = wm_beam_fill_order(N, sum, order);
        if (h >= N || h - fin_n >= n_live) return -1;
        k = order[h - fin_n]; len = wsteps; gi = len - 1;
    }
    for (int t = S + 1 + gi; t < Tq; ++t)
        if (t >= 0) slot[t] = k;
    for (; gi >= 0; --gi) {
        if (S + 1 + gi < Tq) slot[S + 1 + gi] = k;
        k = anc[gi * anc_stride + k];
    }
    for (int t = 0; t <= S && t < Tq; ++t) slot[t] = k;
    return len;
}
