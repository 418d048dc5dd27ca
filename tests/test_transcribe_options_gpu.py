"""GPU tests of wm_transcribe (include/whisper_mi355x.h): per-token log-probabilities of the filtered distribution,
openai-whisper's no_speech_prob and temperature sampling (Gumbel-max with Philox-4x32-10 noise) inside the fused logits /
arg-max kernels, and Context.transcribe_with_fallback on top of them.  Oracle: oracle/whisper_ref.py, teacher-forced on
the GPU's own token history; the sampling noise is restated in numpy (tests/test_transcribe_options_cpu.py)."""
import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from test_model_gpu import (_lively_on_device, _oracle_weights, _perturb_ln_on_device,
                            _scaled_margin, lively, tones)  # noqa: F401  (lively: module fixture)
from test_transcribe_options_cpu import gumbel_np

pytestmark = pytest.mark.gpu

TS, EOT, MAXI = 900, 890, 20          # the lively model's tiny vocabulary (1024): timestamps 900 .. 1023
PROMPT = [10, 21, 5]
SPECIALS = list(range(EOT + 1, TS))


def _rules(ctx, on=True):
    if on:
        ctx.set_suppress(SPECIALS, [EOT])
        ctx.set_timestamp_rules(True, TS, EOT, MAXI)
    else:
        ctx.set_timestamp_rules(False)
        ctx.set_suppress([], [])


def _filtered_rows(ref_rows, hist, prompt_len, suppress, suppress_first, ts):
    """openai-whisper's filters on teacher-forced logit rows: per generated index i -> (row, forced, gap, unforced row)"""
    out = []
    for i in range(len(hist)):
        row = torch.as_tensor(ref_rows[prompt_len - 1 + i]).clone().double()
        row[suppress] = float("-inf")
        if i == 0:
            row[suppress_first] = float("-inf")
        forced, gap = False, float("inf")
        alt = row.clone()
        if ts is not None:
            forced, gap = R.timestamp_filter(row, [int(t) for t in hist[:i]], *ts)
            R.timestamp_filter(alt, [int(t) for t in hist[:i]], *ts, sum_rule=False)
            if not forced:      # the other branch of the sum rule: timestamps only
                alt[:ts[0]] = float("-inf")
        out.append((row, forced, gap, alt))
    return out


def test_greedy_is_unchanged_with_and_without_the_extra_outputs(lively, pkg):
    """opts == NULL and temperature 0: tokens and lens bit-identical to wm_transcribe_greedy, with and without the two
    outputs, under suppress lists + timestamp rules + budgets, and plain."""
    B = pkg.binding
    dims, _, _, ctx = lively
    pcm = tones(6)
    budgets = [24, 5, 17, 24, 1, 9]
    for rules in (False, True):
        _rules(ctx, rules)
        try:
            for eot, bud in ((-1, None), (EOT, budgets)):
                want_t, want_l = ctx.transcribe_greedy(pcm, PROMPT, 24, eot=eot, budgets=bud)
                for opts in (None, B.wm_decode_opts(0.0, 5, -1, 0), B.wm_decode_opts(0.0, 9, 1000, 1)):
                    for lp, ns in ((False, False), (True, False), (True, True)):
                        if ns and (opts is None or opts.no_speech_token < 0):
                            continue
                        t, l, _, _ = ctx.transcribe_raw(pcm, PROMPT, 24, eot, opts, logprobs=lp, no_speech=ns, budgets=bud)
                        assert np.array_equal(t, want_t) and np.array_equal(l, want_l), (rules, eot, lp, ns)
        finally:
            _rules(ctx, False)
    with pytest.raises(B.WhisperError):
        ctx.transcribe_raw(pcm[:1], PROMPT, 4, -1, B.wm_decode_opts(-1.0, 0, -1, 0))
    with pytest.raises(B.WhisperError):
        ctx.transcribe_raw(pcm[:1], PROMPT, 4, -1, B.wm_decode_opts(float("nan"), 0, -1, 0))
    with pytest.raises(B.WhisperError):   # 1 / T overflows f32
        ctx.transcribe_raw(pcm[:1], PROMPT, 4, -1, B.wm_decode_opts(1e-39, 0, -1, 0))
    with pytest.raises(B.WhisperError):
        ctx.transcribe_raw(pcm[:1], PROMPT, 4, -1, B.wm_decode_opts(0.0, 0, 5, 3), no_speech=True)   # sot outside the prompt
    with pytest.raises(B.WhisperError):
        ctx.transcribe_raw(pcm[:1], PROMPT, 4, -1, B.wm_decode_opts(0.0, 0, 1024, 0), no_speech=True)
    with pytest.raises(B.WhisperError):
        ctx.transcribe_raw(pcm[:1], PROMPT, 4, -1, B.wm_decode_opts(0.0, 0, -1, 0), no_speech=True)


def test_logprobs_and_no_speech_against_the_oracle_and_the_gpus_own_logits(lively, pkg):
    dims, _, sd, ctx = lively
    pcm = tones(4)
    mel = ctx.logmel(pcm, out_dtype=np.float32)
    xa = ctx.encode_mel(mel)
    NEW = 20
    worst_o = worst_own = worst_ns = 0.0
    for rules in (False, True):
        _rules(ctx, rules)
        try:
            for sot_index, prompt in ((0, PROMPT), (1, [7] + PROMPT)):
                r = ctx.transcribe(pcm, prompt, NEW, temperature=0.0, no_speech_token=1000, sot_index=sot_index)
                want_t, _ = ctx.transcribe_greedy(pcm, prompt, NEW)
                assert np.array_equal(r.tokens, want_t)
                seqs = np.concatenate([np.tile(prompt, (4, 1)), r.tokens], axis=1)[:, :-1]
                own = ctx.decode_logits(seqs, xa)
                for b in range(4):
                    ref = R.decode_logits(sd, dims, seqs[b:b + 1], xa[b:b + 1])[0].numpy()
                    ts = (TS, EOT, MAXI) if rules else None
                    sup = SPECIALS if rules else []
                    sup1 = [EOT] if rules else []
                    rows_o = _filtered_rows(ref, r.tokens[b], len(prompt), sup, sup1, ts)
                    rows_g = _filtered_rows(own[b], r.tokens[b], len(prompt), sup, sup1, ts)
                    for i in range(NEW):
                        tok = int(r.tokens[b, i])
                        rg = rows_g[i][0]
                        # the GPU's own filtered logits pick the GPU's token (a finding if not: do not loosen the gate)
                        assert int(torch.argmax(rg)) == tok, (rules, b, i)
                        d_own = abs(float(torch.log_softmax(rg, 0)[tok]) - float(r.logprobs[b, i]))
                        worst_own = max(worst_own, d_own)
                        assert d_own <= 1e-4, (rules, b, i, d_own)
                        row, forced, gap, alt = rows_o[i]
                        mg = _scaled_margin(ref[len(prompt) - 1 + i])
                        cands = [row] + ([alt] if abs(gap) < mg else [])   # sum-rule near-tie: either allowed set
                        d = min(abs(float(torch.log_softmax(c, 0)[tok]) - float(r.logprobs[b, i])) for c in cands)
                        worst_o = max(worst_o, d / (2 * mg))
                        assert d <= 2 * mg, (rules, b, i, d, mg)
                    # no_speech_prob: softmax of the RAW logits at the <|startoftranscript|> position
                    raw = torch.as_tensor(ref[sot_index]).double()
                    want_ns = float(torch.softmax(raw, 0)[1000])
                    own_ns = float(torch.softmax(torch.as_tensor(own[b, sot_index]).double(), 0)[1000])
                    assert abs(own_ns - float(r.no_speech_prob[b])) <= 1e-5 * max(1.0, own_ns * 10)
                    mg = _scaled_margin(ref[sot_index])
                    rel = abs(np.log(max(float(r.no_speech_prob[b]), 1e-30)) - np.log(want_ns))
                    worst_ns = max(worst_ns, rel / (2 * mg))
                    assert rel <= 2 * mg, (b, rel, mg)
                    assert np.all(r.logprobs[b] <= 1e-6)
        finally:
            _rules(ctx, False)
    print("log-prob vs oracle: worst |d| / (2 margin) = %.3f; vs own logits: %.2e; no-speech log-ratio / gate %.3f"
          % (worst_o, worst_own, worst_ns))


def test_production_vocabulary_greedy_logprobs_and_no_speech(pkg):
    """large-v2 vocabulary (51 865 ids, 3 242 tiles; timestamps from 50 364), d = 1280, two layers, 8 rows."""
    dims = dict(pkg.binding.MODEL_DIMS["large-v2"], n_audio_layer=2, n_text_layer=2)
    V = dims["n_vocab"]
    EOT2, SOT, TS2, NS, NEW = 50257, 50258, 50364, 50362, 10
    ctx = pkg.binding.Context(dims)
    try:
        ctx.init_synthetic(29)
        _perturb_ln_on_device(ctx, dims, seed=6)
        _lively_on_device(ctx, dims)
        ctx.finalize()
        sd = _oracle_weights(ctx, dims)
        pcm = tones(8)
        mel = ctx.logmel(pcm, n_mels=dims["n_mels"], out_dtype=np.float32)
        xa = ctx.encode_mel(mel)
        ctx.set_suppress([SOT, TS2 - 1, V - 1], [220, EOT2])
        ctx.set_timestamp_rules(True, TS2, EOT2, 50)
        for sot_index, prompt in ((0, [SOT, SOT + 1, SOT + 101]), (1, [400, SOT, SOT + 1, SOT + 101])):
            want_t, want_l = ctx.transcribe_greedy(pcm, prompt, NEW)
            r = ctx.transcribe(pcm, prompt, NEW, temperature=0.0, no_speech_token=NS, sot_index=sot_index)
            assert np.array_equal(r.tokens, want_t) and np.array_equal(r.lens, want_l)
            t0, l0, _, _ = ctx.transcribe_raw(pcm, prompt, NEW, -1, None, logprobs=False)
            assert np.array_equal(t0, want_t)
            worst = 0.0
            for b in range(0, 8, 3):
                seq = np.concatenate([prompt, r.tokens[b]])[None, :-1]
                ref = R.decode_logits(sd, dims, seq, xa[b:b + 1])[0].numpy()
                rows = _filtered_rows(ref, r.tokens[b], len(prompt), [SOT, TS2 - 1, V - 1], [220, EOT2], (TS2, EOT2, 50))
                for i in range(NEW):
                    row, forced, gap, alt = rows[i]
                    mg = _scaled_margin(ref[len(prompt) - 1 + i])
                    cands = [row] + ([alt] if abs(gap) < mg else [])
                    tok = int(r.tokens[b, i])
                    d = min(abs(float(torch.log_softmax(c, 0)[tok]) - float(r.logprobs[b, i])) for c in cands)
                    worst = max(worst, d / (2 * mg))
                    assert d <= 2 * mg, (b, i, d, mg)
                want_ns = float(torch.softmax(torch.as_tensor(ref[sot_index]).double(), 0)[NS])
                rel = abs(np.log(max(float(r.no_speech_prob[b]), 1e-30)) - np.log(want_ns))
                assert rel <= 2 * _scaled_margin(ref[sot_index]), (b, rel)
            print("large-v2 vocabulary, sot_index %d: log-prob worst |d| / (2 margin) = %.3f" % (sot_index, worst))
            # sampling at the production vocabulary: every choice is the arg-max of the perturbed oracle row
            rs = ctx.transcribe(pcm, prompt, NEW, temperature=1.0, seed=77)
            for b in range(0, 8, 4):
                seq = np.concatenate([prompt, rs.tokens[b]])[None, :-1]
                ref = R.decode_logits(sd, dims, seq, xa[b:b + 1])[0].numpy()
                rows = _filtered_rows(ref, rs.tokens[b], len(prompt), [SOT, TS2 - 1, V - 1], [220, EOT2], (TS2, EOT2, 50))
                for i in range(NEW):
                    _check_sampled(rows[i], ref[len(prompt) - 1 + i], int(rs.tokens[b, i]), 1.0,
                                   gumbel_np(77, b, i, np.arange(V)))
    finally:
        ctx.set_timestamp_rules(False)
        ctx.set_suppress([], [])
        ctx.close()


def _check_sampled(filtered, ref_row, tok, inv_T, g):
    row, forced, gap, alt = filtered
    mg = _scaled_margin(ref_row) * inv_T
    ok = False
    for c in [row] + ([alt] if abs(gap) < _scaled_margin(ref_row) else []):
        sc = c.numpy() * inv_T + g
        if np.isfinite(sc[tok]) and sc.max() - sc[tok] <= mg:
            ok = True
    assert ok, (tok, int(np.argmax(row.numpy() * inv_T + g)))


def test_sampling_follows_the_oracle_and_the_numpy_noise(lively, pkg):
    dims, _, sd, ctx = lively
    dbg = pkg.binding.Context(debug=True)
    try:
        worst = 0.0
        for seed, chunk, gi, n0, cnt in ((0, 0, 0, 0, 1024), (2 ** 40 + 7, 37, 400, 50000, 1866), (2 ** 64 - 1, 127, 3, 1, 333)):
            g = dbg.sample_noise(seed, chunk, gi, n0, cnt)
            want = gumbel_np(seed, chunk, gi, np.arange(n0, n0 + cnt))
            err = np.abs(g - want) / np.maximum(1.0, np.abs(want))
            worst = max(worst, float(err.max()))
            assert np.all(np.isfinite(g)) and err.max() <= 1e-5, err.max()
        print("device Gumbel noise vs numpy f64: worst relative error %.2e" % worst)
    finally:
        dbg.close()
    pcm = tones(4)
    xa = ctx.encode_mel(ctx.logmel(pcm, out_dtype=np.float32))
    NEW = 20
    for rules in (False, True):
        _rules(ctx, rules)
        try:
            for T in (0.5, 1.0):
                r = ctx.transcribe(pcm, PROMPT, NEW, temperature=T, seed=1234)
                inv_T = float(np.float32(1.0 / T))
                for b in range(4):
                    seq = np.concatenate([PROMPT, r.tokens[b]])[None, :-1]
                    ref = R.decode_logits(sd, dims, seq, xa[b:b + 1])[0].numpy()
                    rows = _filtered_rows(ref, r.tokens[b], len(PROMPT), SPECIALS if rules else [], [EOT] if rules else [],
                                          (TS, EOT, MAXI) if rules else None)
                    for i in range(NEW):
                        _check_sampled(rows[i], ref[len(PROMPT) - 1 + i], int(r.tokens[b, i]), inv_T,
                                       gumbel_np(1234, b, i, np.arange(dims["n_vocab"])))
                    # the log-prob is still the temperature-1 filtered one
                    for i in range(NEW):
                        row, forced, gap, alt = rows[i]
                        mg = _scaled_margin(ref[len(PROMPT) - 1 + i])
                        tok = int(r.tokens[b, i])
                        d = min(abs(float(torch.log_softmax(c, 0)[tok]) - float(r.logprobs[b, i]))
                                for c in [row] + ([alt] if abs(gap) < mg else []))
                        assert d <= 2 * mg, (rules, T, b, i, d)
        finally:
            _rules(ctx, False)


def test_sampling_is_deterministic_and_batch_invariant(lively, pkg):
    """Same seed: same results; another seed: other rows.  Identical across wm_set_lanes(1), (3) and the default --
    40 chunks of the tiny model run on two sub-chip lanes by default -- and for a chunk alone vs inside a larger call at
    the same call index."""
    dims, _, _, ctx = lively
    pcm = tones(40)
    _rules(ctx, True)
    try:
        def run(**kw):
            r = ctx.transcribe(pcm, PROMPT, 16, eot=EOT, temperature=1.0, seed=99, no_speech_token=1000, **kw)
            return r.tokens, r.lens, r.logprobs, r.no_speech_prob
        base = run()
        again = run()
        assert all(np.array_equal(a, b) for a, b in zip(base, again))
        r2 = ctx.transcribe(pcm, PROMPT, 16, eot=EOT, temperature=1.0, seed=100, no_speech_token=1000)
        assert (r2.tokens != base[0]).any(axis=1).sum() >= 10
        assert np.array_equal(r2.no_speech_prob, base[3])          # seed-independent
        for lanes in (1, 3):
            ctx.set_lanes(lanes)
            try:
                got = run()
            finally:
                ctx.set_lanes(0)
            assert all(np.array_equal(a, b) for a, b in zip(base, got)), lanes
        one = ctx.transcribe(pcm[:1], PROMPT, 16, eot=EOT, temperature=1.0, seed=99, no_speech_token=1000)
        assert np.array_equal(one.tokens[0], base[0][0]) and np.array_equal(one.logprobs[0], base[2][0])
        assert one.no_speech_prob[0] == base[3][0]
        sub = ctx.transcribe(pcm[:5], PROMPT, 16, eot=EOT, temperature=1.0, seed=99)
        assert np.array_equal(sub.tokens, base[0][:5]) and np.array_equal(sub.logprobs, base[2][:5])
    finally:
        _rules(ctx, False)


def test_first_token_distribution_matches_softmax_over_T(lively, pkg):
    """4 096 draws of the first generated token (one recording at 128 call indices x 32 seeds, T = 2) against the
    oracle's softmax(logits / 2): chi-square over the categories with >= 10 expected draws (+ the rest), p > 1e-4."""
    from scipy import stats
    dims, _, sd, ctx = lively
    pcm = np.repeat(tones(1, start=2), 128, axis=0)
    xa = ctx.encode_mel(ctx.logmel(pcm[:1], out_dtype=np.float32))
    counts = np.zeros(dims["n_vocab"], np.int64)
    for s in range(32):
        r = ctx.transcribe(pcm, PROMPT, 1, temperature=2.0, seed=1000 + s)
        counts += np.bincount(r.tokens[:, 0], minlength=dims["n_vocab"])
    ref = R.decode_logits(sd, dims, np.array([PROMPT]), xa)[0, -1].double()
    p = torch.softmax(ref / 2.0, 0).numpy()
    n = counts.sum()
    assert n == 4096
    top = np.where(p * n >= 10)[0]
    assert top.size >= 5, top.size
    obs = np.append(counts[top], n - counts[top].sum())
    exp = np.append(p[top] * n, n * (1 - p[top].sum()))
    keep = exp > 0
    chi2 = float((((obs - exp) ** 2) / exp)[keep].sum())
    pv = float(stats.chi2.sf(chi2, keep.sum() - 1))
    print("first-token distribution: %d categories, chi2 %.1f, p = %.3g" % (keep.sum(), chi2, pv))
    assert pv > 1e-4


def test_early_stop_zeroes_logprobs_and_matches_a_full_decode(lively, pkg):
    dims, _, _, ctx = lively
    pcm = tones(7)
    NEW = 32
    for T in (0.0, 1.0):
        full = ctx.transcribe(pcm, PROMPT, NEW, eot=-1, temperature=T, seed=5)
        vals, cnt = np.unique(full.tokens[:, 2:], return_counts=True)
        eot = int(vals[np.argmax(cnt)])
        budgets = [32, 3, 40, 1, 17, 9, 25]
        r = ctx.transcribe(pcm, PROMPT, NEW, eot=eot, temperature=T, seed=5, budgets=budgets)
        for b in range(7):
            ln = min(NEW, budgets[b])
            hit = np.nonzero(full.tokens[b, :ln] == eot)[0]
            ln = int(hit[0]) + 1 if hit.size else ln
            assert r.lens[b] == ln, (T, b)
            assert np.array_equal(r.tokens[b, :ln], full.tokens[b, :ln])
            assert np.array_equal(r.logprobs[b, :ln], full.logprobs[b, :ln])
            assert not r.logprobs[b, ln:].any()
            assert r.sum_logprob[b] == pytest.approx(float(np.sum(full.logprobs[b, :ln], dtype=np.float64)), abs=0)


def test_fallback_steps_equal_direct_calls_on_the_same_subsets(lively, pkg):
    dims, _, _, ctx = lively
    pcm = tones(6)
    NEW = 16
    base = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT)
    thr = float(np.median(base.avg_logprob))          # about half the chunks fall back at step 0
    out = ctx.transcribe_with_fallback(pcm, PROMPT, NEW, EOT, temperatures=(0.0, 0.5, 1.0), logprob_threshold=thr,
                                       compression_ratio_threshold=None, seed=11)
    steps = out["steps"]
    assert len(steps) >= 2 and steps[0][2].size == 6 and 0 < steps[1][2].size < 6
    final = {}
    for t, s, idx in steps:
        d = ctx.transcribe(pcm[idx], PROMPT, NEW, eot=EOT, temperature=t, seed=s)
        for k, b in enumerate(idx):
            final[int(b)] = (d.tokens[k], t, s)
    for b in range(6):
        tok, t, s = final[b]
        assert np.array_equal(out["tokens"][b], tok) and out["temperature"][b] == t and out["seed"][b] == s
