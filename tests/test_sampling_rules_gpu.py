"""GPU tests of the sampling rules (wm_set_sampling_rules: top_k, top_p, min_p) through the transcribe
entries, on the `lively` tiny model of test_model_gpu.py (V = 1024) and the two-layer large-v2-vocabulary context of
test_transcribe_options_gpu.py.

Invariants first (bit for bit): top_k = 1 is the temperature-0 call, top_k above the vocabulary the rules-off sampled call,
rules off after on the fresh context.  Then the project's own-logits standard (test_repetition_gpu.py): the GPU's tokens are
teacher-forced through ctx.decode_logits, the existing filters and restatements are applied to those rows, and every token must
lie in tests/sampling_ref.py's kept set of its row and be the arg-max of v / T + Gumbel noise over it; the log-prob stays the
untruncated filtered one."""
import ctypes

import numpy as np
import pytest
import torch

import repeat_ref as RR
import sampling_ref as S
import seqbias_ref as SB
from test_model_gpu import _lively_on_device, _perturb_ln_on_device, lively, tones  # noqa: F401  (lively: module fixture)
from test_transcribe_options_cpu import gumbel_np
from test_transcribe_options_gpu import EOT, MAXI, SPECIALS, TS, _filtered_rows, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
PROMPT = [10, 21, 5]
NEW = 24
# The own-logits tests sample at T = 0.5 with a nucleus of 0.3: the lively model's rows are flat (logit rms 0.9: at T = 1 every
# id holds about 1e-3 of the mass), and a cut that falls among such ids is inside the 1e-4 slack by construction.  Measured on the
# CPU, on the oracle's rows of this model along a sampled history of 4 x 24 positions -- positions inside the slack of 96:
#   T = 1:   (0, 0.9, 0) 39   (0, 0.5, 0) 7   (0, 0.3, 0) 5   (50, 0.9, 0.05) 12   (0, 1, 0.1) 4
#   T = 0.5: (0, 0.9, 0) 46   (0, 0.5, 0) 6   (0, 0.3, 0) 1   (50, 0.9, 0.05) 4    (0, 1, 0.1) 0    (8, 1, 0) 0
# so the wide nucleus (0.9) is left to the kernel tests' rows and the first-token distribution below, where the cap does not bind.
T_OWN = 0.5
RULE_SETS = [(8, 1.0, 0.0), (0, 0.3, 0.0), (0, 1.0, 0.1), (50, 0.9, 0.05)]


def same(*arrays):
    arrays = [np.ascontiguousarray(x) for x in arrays]
    a = arrays[0]
    return all(x.dtype == a.dtype and x.shape == a.shape and np.array_equal(x.view(np.uint8), a.view(np.uint8)) for x in arrays[1:])


def same_result(a, b):
    return same(a.tokens, b.tokens) and same(a.lens, b.lens) and same(a.logprobs, b.logprobs)


@pytest.fixture(scope="module")
def world(lively, pkg):
    dims, sd_np, sd, ctx = lively
    w = dict(dims=dims, sd_np=sd_np, ctx=ctx, b=pkg.binding, pcm=tones(8), V=dims["n_vocab"])
    w["mel"] = ctx.logmel(w["pcm"], out_dtype=np.float32)
    w["mel_args"] = (w["mel"].reshape(-1), np.arange(8, dtype=np.int64) * 80 * 3000, 3000, 0, 3000)
    w["xa"] = ctx.encode_mel(w["mel"])
    yield w
    ctx.set_sampling_rules()
    ctx.set_repetition_rules()
    ctx.set_sequence_bias(None)
    _rules(ctx, False)


def fresh(w):
    c = w["b"].Context(w["dims"])
    c.load_state_dict(w["sd_np"])
    c.finalize()
    return c


# ------------------------------------------------------------------------------------------------------- invariants
@pytest.mark.parametrize("ts_on", [False, True])
def test_top_k_one_is_the_temperature_zero_call(world, ts_on):
    """top_k = 1 at T = 0.5 and 1: tokens, lens and log-probs of the T = 0 call bit for bit -- plain, with eot and with budgets."""
    ctx, pcm = world["ctx"], world["pcm"]
    budgets = [24, 5, 17, 24, 1, 9, 12, 3]
    _rules(ctx, ts_on)
    try:
        for kw in (dict(), dict(eot=EOT), dict(eot=EOT, budgets=budgets), dict(no_speech_token=1000)):
            ctx.set_sampling_rules()
            want = ctx.transcribe(pcm, PROMPT, NEW, temperature=0.0, **kw)
            ctx.set_sampling_rules(1)
            for T in (0.5, 1.0):
                got = ctx.transcribe(pcm, PROMPT, NEW, temperature=T, seed=31, **kw)
                assert same_result(got, want), (ts_on, kw, T)
            ctx.set_sampling_rules(0, 1e-6)          # (a nucleus that only ever holds the best id)
            assert same_result(ctx.transcribe(pcm, PROMPT, NEW, temperature=1.0, seed=31, **kw), want), (ts_on, kw)
    finally:
        ctx.set_sampling_rules()
        _rules(ctx, False)


def test_top_k_above_the_vocabulary_is_the_rules_off_sampled_call(world):
    """top_k = V + 7 keeps everything: every sampling entry returns the rules-off call's bits -- the second-stage draw reproduces
    the fused one -- and differs from it under (8, 1, 0)."""
    ctx, pcm, mel_args, V = world["ctx"], world["pcm"], world["mel_args"], world["V"]
    ragged = [[10, 21, 5], [7, 9, 10, 21, 5], [5, 5, 5, 5, 5, 5, 10, 21, 5], [4, 8, 10, 21, 5]] * 2
    _rules(ctx, True)

    def entries():
        out = {}
        out["transcribe"] = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, temperature=0.8, seed=11, no_speech_token=1000)
        out["mel"] = ctx.transcribe_mel(*mel_args, PROMPT, NEW, eot=EOT, temperature=0.8, seed=11)
        out["ragged"] = ctx.transcribe_mel(*mel_args, ragged, NEW, eot=EOT, sot_tail=3, temperature=0.8, seed=5)
        out["best_of"] = ctx.transcribe_mel_best_of(*mel_args, PROMPT, NEW, 3, eot=EOT, temperature=0.8, seed=11)
        with ctx.encode_windows(*mel_args) as ws:
            out["windows"] = ctx.transcribe_windows(ws, None, PROMPT, NEW, eot=EOT, temperature=0.8, seed=11)
        out["aligned"] = ctx.transcribe_mel_aligned(*mel_args, PROMPT, NEW, eot=EOT, temperature=0.8, seed=11)
        return out
    try:
        ctx.set_sampling_rules()
        off = entries()
        ctx.set_sampling_rules(V + 7)
        on = entries()
        for name in off:
            assert same_result(on[name], off[name]), name
        assert same(on["aligned"].start_frames, off["aligned"].start_frames)
        assert same(on["transcribe"].no_speech_prob, off["transcribe"].no_speech_prob)
        ctx.set_sampling_rules(8)
        cut = entries()
        for name in off:
            assert not same(cut[name].tokens, off[name].tokens), name
        assert same_result(cut["mel"], cut["windows"]) and same_result(cut["mel"], cut["aligned"])
        assert same(cut["transcribe"].no_speech_prob, off["transcribe"].no_speech_prob)          # no_speech_prob is unchanged
    finally:
        ctx.set_sampling_rules()
        _rules(ctx, False)


def test_rules_off_after_on_and_temperature_zero(world):
    """One context's captured graphs: a call under (8, 0.9, 0), then other values (the parameters live in device memory), then
    rules off -- each equals a fresh context's result, and a later clone inherits the rules.  T = 0 with the rules set equals
    T = 0 without, greedy and beam entries included."""
    ctx, pcm, mel_args = world["ctx"], world["pcm"], world["mel_args"]
    try:
        ctx.set_sampling_rules()
        g0 = ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=EOT)
        t0 = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT)
        b0 = ctx.transcribe_mel_beam(*mel_args, PROMPT, NEW, 3, eot=EOT)
        got = []
        settings = ((8, 0.9, 0.0), (3, 1.0, 0.0), (0, 1.0, 0.3), (0, 1.0, 0.0))
        for st in settings:
            ctx.set_sampling_rules(*st)
            got.append(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, temperature=1.0, seed=4))
            g = ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=EOT)
            assert same(g[0], g0[0]) and same(g[1], g0[1]) and same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT), t0)
            bm = ctx.transcribe_mel_beam(*mel_args, PROMPT, NEW, 3, eot=EOT)
            assert same(bm.tokens, b0.tokens) and same(bm.lens, b0.lens)
        assert not same(got[0].tokens, got[1].tokens) and not same(got[0].tokens, got[3].tokens)
        for st, r in zip(settings, got):
            c = fresh(world)
            try:
                c.set_sampling_rules(*st)
                assert same_result(c.transcribe(pcm, PROMPT, NEW, eot=EOT, temperature=1.0, seed=4), r), st
                k = c.clone()
                try:
                    assert same_result(k.transcribe(pcm, PROMPT, NEW, eot=EOT, temperature=1.0, seed=4), r), st
                finally:
                    k.close()
            finally:
                c.close()
    finally:
        ctx.set_sampling_rules()


# ------------------------------------------------------------------------------------------------------- own logits
def check_own_logits(ctx, xa, r, rule, T, seed, ts_on, V, row_rules=None, sample_ids=None):
    """Every generated token of result r against the kept set of the context's own teacher-forced, filtered logits row.
    row_rules(row, hist) -> (row, banned): the repetition / sequence-bias restatements.  Returns (positions, inside the slack)."""
    inv_T = float(np.float32(1.0 / T))
    B = r.tokens.shape[0]
    seqs = np.concatenate([np.tile(PROMPT, (B, 1)), r.tokens], axis=1)[:, :-1]
    own = ctx.decode_logits(seqs, xa[:B])
    n_pos = n_near = 0
    for b in range(B):
        rows = np.array(own[b], dtype=np.float32, copy=True)
        if row_rules is not None:
            for i in range(NEW):
                row, banned = row_rules(rows[len(PROMPT) - 1 + i], r.tokens[b, :i])
                row[banned] = -np.inf
                rows[len(PROMPT) - 1 + i] = row
        filt = _filtered_rows(rows, r.tokens[b], len(PROMPT), SPECIALS if ts_on else [], [EOT] if ts_on else [],
                              (TS, EOT, MAXI) if ts_on else None)
        for i in range(NEW):
            tok = int(r.tokens[b, i])
            v = rows[len(PROMPT) - 1 + i]
            g = gumbel_np(seed, b if sample_ids is None else int(sample_ids[b]), i, np.arange(V))
            ok, near = False, False
            cands = [filt[i][0]] + ([filt[i][3]] if abs(filt[i][2]) < 1e-3 else [])      # a sum-rule near-tie: either allowed set
            for rg in cands:
                d = S.kept_detail(v, torch.isfinite(rg).numpy(), inv_T, *rule)
                fine = False
                for c in ([d.count] if d.slack > S.TOL else sorted(d.accept)):      # inside the slack: any acceptable count
                    keep = d.ids[:c]
                    if tok not in keep:
                        continue
                    sc = v[keep].astype(np.float64) * inv_T + g[keep]
                    at, best = int(np.flatnonzero(keep == tok)[0]), int(np.argmax(sc))
                    fine = fine or sc[best] - sc[at] <= 1e-4 * max(1.0, abs(g[keep][at]), abs(g[keep][best]))
                if fine:
                    ok, near = True, d.slack <= S.TOL
                    # the log-prob is still the untruncated filtered one
                    lp = float(torch.log_softmax(rg, 0)[tok])
                    assert abs(lp - float(r.logprobs[b, i])) <= 1e-4, (rule, ts_on, b, i, lp, float(r.logprobs[b, i]))
                    break
            assert ok, (rule, T, ts_on, b, i, tok)
            n_pos += 1
            n_near += near
    return n_pos, n_near


@pytest.mark.parametrize("ts_on", [False, True])
@pytest.mark.parametrize("rule", RULE_SETS)
def test_every_token_lies_in_the_kept_set_of_the_gpus_own_logits(world, rule, ts_on):
    ctx, pcm, xa, V = world["ctx"], world["pcm"][:4], world["xa"], world["V"]
    _rules(ctx, ts_on)
    try:
        ctx.set_sampling_rules()
        plain = ctx.transcribe(pcm, PROMPT, NEW, temperature=T_OWN, seed=1234)
        ctx.set_sampling_rules(*rule)
        r = ctx.transcribe(pcm, PROMPT, NEW, temperature=T_OWN, seed=1234)
        n_pos, n_near = check_own_logits(ctx, xa, r, rule, T_OWN, 1234, ts_on, V)
        print("rule %s ts %s: %d positions, %d inside the slack; rows changed %d of 4"
              % (rule, ts_on, n_pos, n_near, sum(not same(r.tokens[b], plain.tokens[b]) for b in range(4))))
        assert n_near <= 0.10 * n_pos, (n_near, n_pos)
        assert not same(r.tokens, plain.tokens)            # the rules had something to act on
    finally:
        ctx.set_sampling_rules()
        _rules(ctx, False)


def test_the_kept_set_is_taken_over_the_penalised_and_biased_rows(world):
    """Repetition rules (1.3, 3) and a small sequence-bias table on: the same standard on the penalised, biased rows."""
    ctx, pcm, xa, V = world["ctx"], world["pcm"][:4], world["xa"], world["V"]
    _rules(ctx, True)
    try:
        ctx.set_repetition_rules(1.3, 3, EOT)
        first = ctx.transcribe(pcm, PROMPT, NEW, temperature=T_OWN, seed=8)
        table = {(int(first.tokens[0, 1]),): -np.inf, (int(first.tokens[1, 2]), int(first.tokens[1, 3])): -np.inf, (17,): 1.5, (33, 34): 2.0}
        table = {k: v for k, v in table.items() if k[-1] < EOT}
        ctx.set_sequence_bias(table, eot=EOT)
        ref = SB.expand(list(table), list(table.values()), eot=EOT, V=V)

        def row_rules(row, hist):
            row, banned = RR.apply_rules(row, hist, 1.3, 3, EOT)
            row, sbanned = SB.apply_bias(row, ref, hist)
            return row, banned | sbanned
        for rule in RULE_SETS:
            ctx.set_sampling_rules(*rule)
            r = ctx.transcribe(pcm, PROMPT, NEW, temperature=T_OWN, seed=8)
            n_pos, n_near = check_own_logits(ctx, xa, r, rule, T_OWN, 8, True, V, row_rules)
            print("rule %s on the penalised, biased rows: %d positions, %d inside the slack" % (rule, n_pos, n_near))
            assert n_near <= 0.10 * n_pos, (rule, n_near, n_pos)
            for b in range(4):
                assert RR.repeated_ngrams(r.tokens[b], 3, EOT) == 0
                for s, bias in table.items():
                    assert bias != -np.inf or not SB.contains(r.tokens[b], s), (b, s)
    finally:
        ctx.set_sampling_rules()
        ctx.set_sequence_bias(None)
        ctx.set_repetition_rules()
        _rules(ctx, False)


def test_production_vocabulary(pkg):
    """large-v2 vocabulary (51 865 ids, 3 242 tiles; timestamps from 50 364), d = 1280, two layers, 8 rows: top_k = 1 is the
    greedy call, top_k = V + 7 the sampled call, and (50, 0.9, 0.05) passes the own-logits standard."""
    dims = dict(pkg.binding.MODEL_DIMS["large-v2"], n_audio_layer=2, n_text_layer=2)
    V = dims["n_vocab"]
    EOT2, SOT, TS2, N = 50257, 50258, 50364, 10
    prompt = [SOT, SOT + 1, SOT + 101]
    ctx = pkg.binding.Context(dims)
    try:
        ctx.init_synthetic(29)
        _perturb_ln_on_device(ctx, dims, seed=6)
        _lively_on_device(ctx, dims)
        ctx.finalize()
        pcm = tones(8)
        xa = ctx.encode_mel(ctx.logmel(pcm, n_mels=dims["n_mels"], out_dtype=np.float32))
        sup, sup1 = [SOT, TS2 - 1, V - 1], [220, EOT2]
        ctx.set_suppress(sup, sup1)
        ctx.set_timestamp_rules(True, TS2, EOT2, 50)
        greedy = ctx.transcribe(pcm, prompt, N, temperature=0.0)
        plain = ctx.transcribe(pcm, prompt, N, temperature=T_OWN, seed=77)
        ctx.set_sampling_rules(1)
        assert same_result(ctx.transcribe(pcm, prompt, N, temperature=T_OWN, seed=77), greedy)
        ctx.set_sampling_rules(V + 7)
        assert same_result(ctx.transcribe(pcm, prompt, N, temperature=T_OWN, seed=77), plain)
        rule = (50, 0.9, 0.05)
        inv_T = float(np.float32(1.0 / T_OWN))
        ctx.set_sampling_rules(*rule)
        r = ctx.transcribe(pcm, prompt, N, temperature=T_OWN, seed=77)
        assert not same(r.tokens, plain.tokens)
        n_pos = n_near = 0
        for b in (0, 5):
            seq = np.concatenate([prompt, r.tokens[b]])[None, :-1]
            own = np.array(ctx.decode_logits(seq, xa[b:b + 1])[0], dtype=np.float32)
            filt = _filtered_rows(own, r.tokens[b], len(prompt), sup, sup1, (TS2, EOT2, 50))
            for i in range(N):
                tok, v = int(r.tokens[b, i]), own[len(prompt) - 1 + i]
                assert abs(filt[i][2]) > 1e-3
                d = S.kept_detail(v, torch.isfinite(filt[i][0]).numpy(), inv_T, *rule)
                keep = d.ids[:max(d.accept) if d.slack <= S.TOL else d.count]
                assert tok in keep, (b, i, tok)
                if d.slack > S.TOL:
                    g = gumbel_np(77, b, i, keep)
                    sc = v[keep].astype(np.float64) * inv_T + g
                    at, best = int(np.flatnonzero(keep == tok)[0]), int(np.argmax(sc))
                    assert sc[best] - sc[at] <= 1e-4 * max(1.0, abs(g[at]), abs(g[best])), (b, i)
                lp = float(torch.log_softmax(filt[i][0], 0)[tok])
                assert abs(lp - float(r.logprobs[b, i])) <= 1e-4, (b, i)
                n_pos += 1
                n_near += d.slack <= S.TOL
        print("large-v2 vocabulary, rule %s: %d positions, %d inside the slack" % (rule, n_pos, n_near))
        assert n_near <= 0.10 * n_pos, (n_near, n_pos)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------- batch invariance
def test_lanes_a_row_alone_and_best_of_candidate_zero(world):
    """Under (8, 0.9, 0): 40 rows on one lane, three lanes and the default lanes return the same bits; a row alone is the row
    among others; candidate 0 of a best-of call is the plain call, and the candidates differ."""
    ctx, mel_args = world["ctx"], world["mel_args"]
    pcm = tones(40)
    _rules(ctx, True)
    try:
        ctx.set_sampling_rules(8, 0.9, 0.0)

        def run(p=pcm):
            return ctx.transcribe(p, PROMPT, 16, eot=EOT, temperature=1.0, seed=99)
        base = run()
        assert same_result(run(), base)
        for lanes in (1, 3):
            ctx.set_lanes(lanes)
            try:
                assert same_result(run(), base), lanes
            finally:
                ctx.set_lanes(0)
        one = run(pcm[:1])
        assert same(one.tokens[0], base.tokens[0]) and same(one.logprobs[0], base.logprobs[0])
        sub = run(pcm[:5])
        assert same(sub.tokens, base.tokens[:5]) and same(sub.logprobs, base.logprobs[:5])
        mel = ctx.transcribe_mel(*mel_args, PROMPT, 16, eot=EOT, temperature=1.0, seed=99)
        bo = ctx.transcribe_mel_best_of(*mel_args, PROMPT, 16, 3, eot=EOT, temperature=1.0, seed=99)
        assert same(bo.tokens[:, 0], mel.tokens) and same(bo.logprobs[:, 0], mel.logprobs) and same(bo.lens[:, 0], mel.lens)
        assert (bo.tokens[:, 1] != bo.tokens[:, 0]).any() and (bo.tokens[:, 2] != bo.tokens[:, 1]).any()
    finally:
        ctx.set_sampling_rules()
        _rules(ctx, False)


# ------------------------------------------------------------------------------------------------------- distribution
@pytest.mark.parametrize("rule", [(8, 1.0, 0.0), (0, 0.9, 0.0)])
def test_first_token_distribution_is_the_renormalised_truncated_softmax(world, rule):
    """4 096 draws of the first generated token (one recording at 128 call indices x 32 seeds, T = 2): none outside the kept set
    of the context's own logits row, and chi-square against softmax(v / 2) renormalised over it, p > 1e-4 (the recipe of
    test_first_token_distribution_matches_softmax_over_T)."""
    from scipy import stats
    ctx, V = world["ctx"], world["V"]
    pcm = np.repeat(tones(1, start=2), 128, axis=0)
    xa = ctx.encode_mel(ctx.logmel(pcm[:1], out_dtype=np.float32))
    own = np.array(ctx.decode_logits(np.array([PROMPT]), xa)[0, -1], dtype=np.float32)
    inv_T = float(np.float32(0.5))
    d = S.kept_detail(own, np.ones(V, bool), inv_T, *rule)
    counts = np.zeros(V, np.int64)
    try:
        ctx.set_sampling_rules(*rule)
        for s in range(32):
            r = ctx.transcribe(pcm, PROMPT, 1, temperature=2.0, seed=1000 + s)
            counts += np.bincount(r.tokens[:, 0], minlength=V)
    finally:
        ctx.set_sampling_rules()
    n = counts.sum()
    assert n == 4096
    hi = max(d.accept) if d.slack <= S.TOL else d.count
    assert counts[d.ids[:hi]].sum() == n, "a draw outside the kept set"
    keep = d.ids[:d.count]
    p = d.m[:d.count] / d.m[:d.count].sum()
    top = np.where(p * n >= 10)[0]
    assert top.size >= 3, top.size
    obs = np.append(counts[keep[top]], n - counts[keep[top]].sum())
    exp = np.append(p[top] * n, n * (1 - p[top].sum()))
    ok = exp > 1e-9
    chi2 = float((((obs - exp) ** 2) / np.where(ok, exp, 1.0))[ok].sum())
    pv = float(stats.chi2.sf(chi2, ok.sum() - 1))
    print("rule %s: %d kept ids, %d categories, chi2 %.1f, p = %.3g" % (rule, d.count, ok.sum(), chi2, pv))
    assert pv > 1e-4


# ------------------------------------------------------------------------------------------------------- errors
def test_invalid_arguments_and_the_f32_debug_path(world):
    """WM_ERR_INVALID for top_k < 0, top_p outside (0, 1], min_p outside [0, 1) and NaNs, and the rules in force survive a refused
    call; the debug library's all-f32 precision path answers WM_ERR_STATE."""
    ctx, b, pcm = world["ctx"], world["b"], world["pcm"]
    fn = ctx.lib.wm_set_sampling_rules
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    nan = float("nan")
    try:
        ctx.set_sampling_rules(4, 0.9, 0.0)
        want = ctx.transcribe(pcm, PROMPT, 12, temperature=1.0, seed=2)
        for k, p, mp in ((-1, 1.0, 0.0), (0, 0.0, 0.0), (0, -0.5, 0.0), (0, 1.0001, 0.0), (0, nan, 0.0), (0, 1.0, -0.1), (0, 1.0, 1.0),
                         (0, 1.0, nan), (5, float("inf"), 0.0), (5, 0.5, float("inf"))):
            assert fn(ctx.handle, k, p, mp) == WM_ERR_INVALID, (k, p, mp)
            with pytest.raises(b.WhisperError) as e:
                ctx.set_sampling_rules(k, p, mp)
            assert e.value.status == WM_ERR_INVALID
        assert same_result(ctx.transcribe(pcm, PROMPT, 12, temperature=1.0, seed=2), want)
        for k, p, mp in ((2 ** 31 - 1, 1.0, 0.0), (0, 1e-30, 0.0), (1, 1.0, 0.999), (0, 1.0, 0.0)):
            assert fn(ctx.handle, k, p, mp) == 0, (k, p, mp)
    finally:
        ctx.set_sampling_rules()
    dbg = b.Context(world["dims"], debug=True)
    try:
        dbg.load_state_dict(world["sd_np"])
        dbg.finalize()
        dbg.set_sampling_rules(4)
        dbg.set_precision(True)
        with pytest.raises(b.WhisperError) as e:
            dbg.transcribe(pcm[:1], PROMPT, 4, temperature=1.0)
        assert e.value.status == WM_ERR_STATE
        with pytest.raises(b.WhisperError) as e:
            dbg.set_sampling_rules(0, 0.5)
        assert e.value.status == WM_ERR_STATE
        dbg.set_sampling_rules()                         # switching them off is always allowed
        dbg.set_precision(False)
        dbg.set_sampling_rules(1)
        assert same(dbg.transcribe(pcm[:1], PROMPT, 4, temperature=1.0).tokens, dbg.transcribe(pcm[:1], PROMPT, 4).tokens)
    finally:
        dbg.close()
