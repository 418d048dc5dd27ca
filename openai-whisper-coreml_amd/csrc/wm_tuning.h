// wm_tuning.h -- the launch-shape experiment knobs (see wm_internal.h); plain C++, no HIP headers, so that the pure launch
// plans of dec_launch.cpp can be built and tested on their own.
#pragma once
struct WmTuning {
    int gemv_tn = 0;              // force tiles per workgroup of the wide decode GEMVs (1, 2, 4)
    int gemv_nblk = 0;            // 1: one batch block per workgroup also above 16 rows
    int gemv_ppw2_nblk = 0;       // probes: 1 / 2 = force one / two batch blocks per workgroup in the two-parts-per-wave K = 4d residual product (0: the rule)
    int gemv_no_ppw2 = 0;         // 1: K = 4d residual product as 16-wave workgroups (no two-parts-per-wave kernel)
    int prefetch_max_b = 16;      // L2 warm-up workgroups up to this decode-group size (0: never)
    int xattn_split_below = 96;   // (sequence, head) pairs below which the cross-attention streams are dealt flat
    int xattn_wgs = 256;          // workgroup cap of the cross-attention
    int xattn_no_flat = 0;        // 1: split launches as (pair, split) grids instead of the flat deal
    int xattn_lds_pad = 84 * 1024;  // dynamic LDS reserved per cross-attention workgroup (one per CU chip-wide); 0: off
    int xattn_splits = 0;         // force the split count of the cross-attention (1, 2, 4, 8)
    int gemm_tile = 0;            // force the encoder GEMM tile (128 / 256)
    int gemm_gm = 4;              // grouped tile order of the encoder GEMM
    int gemm128_pipe = 0;         // PROBE: the 128 x 128 tile's 3-stage pipeline kernel: 0 = the rule (grids <= 2 rounds of the chip), 1 = never, 2 = always
    int no_early_stop = 0;        // 1: decode every position and truncate on the host (the round-2 behaviour)
    int logits_tn = 0;            // 1 / 2: tiles per workgroup of the logits product at <= 16 rows (product: 4)
    int enc_attn_mfma_sum = 0;    // 1: encoder attention row sums by a ones-operand MFMA instead of f32 VALU adds
    int xattn_never_short = 0;    // 1: persistent cross-attention workgroups also when the chip is shared (rounds 2-3)
    int xattn_no_deep = 0;        // 1: the flat (few-pair) cross-attention walks its blocks one round trip at a time
    int xattn_fuse_q = 1;         // 96 .. 256 pairs, alone: query projection fused into the cross-attention launch (0: two launches)
    int argmax_rows_per_wg = 0;   // PROBE: rows per workgroup of the step-closing arg-max (0 = the product's rule: 1, or 16 for <= 16 rows with early stop)
    int group_chunks = 0;         // preferred decode-group size of a wm_transcribe_greedy call (product rule: tx_plan.cpp)
    int frontend_per_wave_twiddles = 0;   // 1: the f32 front end's round-1-5 stage-1 kernel (every wave fetches its own twiddles from L2)
    int lane_parts = 0;           // sub-chip lanes: 0 = the product's rule, 1 = never, 2 / 3 = that many CU-masked groups whenever the call has >= 2 chunks per part
    int teacher_panel_cut = 0;    // PROBE: how a teacher-forced group of more windows than fit a full-width panel is cut: 1 = ONE panel narrowed to floor(128 / windows) positions, 2 = slices at the full width (0 = the rule, the fewest steps: model.cpp wm_model_panel_slices)
    int spec_group = 0;           // windows per decode group of a speculative call (0 = the measured default, the whole call: tx_plan.cpp wm_spec_groups); always <= 128 / (draft_len + 1)
    int lane_solo_cus = 0;        // PROBE: n in 1 .. 31 = run the call's decode groups one after the other on ONE lane confined to the first n CUs of every XCD
};
