"""GPU tests of best-of-N sampling: wm_transcribe_mel_best_of (best_of candidates per window over one encoder pass, one
cross-attention K/V cache and one read of it), its ranking output, and best_of in binding.transcribe_long.  The yardsticks
are the EXISTING calls -- wm_transcribe_mel / wm_transcribe_mel_ragged give candidate 0 bit for bit -- and, for the
candidates s >= 1, the oracle with the numpy noise restated with the candidate word (tests/test_best_of_cpu.py).  All on the
lively synthetic model; every equality is bit-level."""
import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from test_best_of_cpu import gumbel_cand_np, rank_np
from test_longform_gpu import _kw, _long_recs, prod  # noqa: F401  (prod: fixture)
from test_model_gpu import _scaled_margin, lively, tones  # noqa: F401  (lively: fixture)
from test_ragged_prompts_gpu import NS_TOK, _prompts, _ragged, _same
from test_transcribe_options_gpu import EOT, MAXI, PROMPT, SPECIALS, TS, _check_sampled, _filtered_rows, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID = 1   # include/whisper_mi355x.h
NEW = 16


@pytest.fixture(scope="module")
def mel10(lively):
    """Ten distinct windows; a call of any size points its rows at them (mel_base repeats)."""
    _, _, _, ctx = lively
    return ctx.logmel(tones(10), out_dtype=np.float32)


def _base(n):
    return (np.arange(n, dtype=np.int64) % 10) * 240000


def _ids(n):
    return (np.arange(n, dtype=np.uint32) * 7 + 3) | np.uint32(2 << 16)


def _bo(ctx, mel, base, prompts, T, N, new=NEW, eot=EOT, ids=None, budgets=None, sot_tail=None, sot_index=0, seed=77, pen=None,
        ns=True):
    """wm_transcribe_mel_best_of: uniform prompts (2-d array, sot_index) or ragged ones (a list of lists, sot_tail)"""
    return ctx.transcribe_mel_best_of(mel, base, 3000, 0, 3000, prompts, new, N, eot=eot, temperature=T, seed=seed,
                                      no_speech_token=NS_TOK if ns else -1, sot_index=sot_index, sample_ids=ids, budgets=budgets,
                                      sot_tail=sot_tail, length_penalty=pen)


def _cand(r, s):
    return [r.tokens[:, s], r.lens[:, s], r.logprobs[:, s], r.no_speech_prob]


def _uniform_prompts(n, n_prompt=3, seed=3):
    return np.array(_prompts([n_prompt] * n, seed=seed), dtype=np.int32)


RAGGED_LENS = [3, 40, 1, 17, 2, 4, 9, 33, 5, 3, 21, 6]


# ---------------------------------------------------------------- 1. best_of = 1 is the plain call
@pytest.mark.parametrize("T", [0.0, 1.0])
def test_best_of_1_is_the_uniform_and_the_ragged_call(lively, pkg, mel10, T):
    _, _, _, ctx = lively
    b = pkg.binding
    _rules(ctx)
    try:
        n = 6
        base, ids = _base(n), _ids(n)
        budgets = [16, 5, 12, 1, 9, 16]
        prompts = _uniform_prompts(n, 4)
        opts = b.wm_decode_opts(T, 77, NS_TOK, 1)
        want = ctx.transcribe_mel_raw(mel10, base, 3000, 0, 3000, prompts, NEW, EOT, opts, sample_ids=ids, no_speech=True,
                                      budgets=budgets)
        got = _bo(ctx, mel10, base, prompts, T, 1, ids=ids, budgets=budgets, sot_index=1)
        assert got.tokens.shape == (n, 1, NEW) and np.all(got.best == 0)
        _same(_cand(got, 0), want, "uniform")
        # without sample ids: the row's index in the call
        want0 = ctx.transcribe_mel_raw(mel10, base, 3000, 0, 3000, prompts, NEW, EOT, opts, no_speech=True)
        _same(_cand(_bo(ctx, mel10, base, prompts, T, 1, sot_index=1), 0), want0, "uniform, no ids")
        rag = _prompts(RAGGED_LENS[:n], seed=5)
        want = _ragged(ctx, b, mel10, base, rag, T, new=NEW, eot=EOT, ids=ids, budgets=budgets, sot_tail=1)
        got = _bo(ctx, mel10, base, rag, T, 1, ids=ids, budgets=budgets, sot_tail=1)
        _same(_cand(got, 0), want, "ragged")
    finally:
        _rules(ctx, False)


# ---------------------------------------------------------------- 2. candidate 0 is today's stream
@pytest.mark.parametrize("T", [0.0, 1.0])
def test_candidate_0_of_a_best_of_5_call_is_the_best_of_1_result(lively, pkg, mel10, T):
    _, _, _, ctx = lively
    _rules(ctx)
    try:
        n = 12
        base, ids = _base(n), _ids(n)
        for prompts, kw in ((_uniform_prompts(n), dict(sot_index=0)), (_prompts(RAGGED_LENS, seed=5), dict(sot_tail=1))):
            one = _bo(ctx, mel10, base, prompts, T, 1, ids=ids, **kw)
            five = _bo(ctx, mel10, base, prompts, T, 5, ids=ids, **kw)
            assert five.tokens.shape == (n, 5, NEW)
            _same(_cand(five, 0), _cand(one, 0), "candidate 0, %s" % sorted(kw))
            if T == 0.0:   # temperature 0 is allowed: all candidates equal, best 0
                for s in range(1, 5):
                    _same(_cand(five, s), _cand(five, 0), "T = 0, candidate %d" % s)
                assert np.all(five.best == 0)
    finally:
        _rules(ctx, False)


# ---------------------------------------------------------------- 3. invariance
def test_a_candidate_depends_on_its_own_row_only(lively, pkg, mel10):
    _, _, _, ctx = lively
    _rules(ctx)
    try:
        n, T = 12, 1.0
        base, ids = _base(40), _ids(40)
        lens40 = (RAGGED_LENS * 4)[:40]
        for prompts40, kw in ((_uniform_prompts(40), dict(sot_index=0)), (_prompts(lens40, seed=5), dict(sot_tail=1))):
            prompts = prompts40[:n]
            ref = _bo(ctx, mel10, base[:n], prompts, T, 5, ids=ids[:n], **kw)
            # row b alone
            for r in (0, 5, 11):
                alone = _bo(ctx, mel10, base[r:r + 1], prompts[r:r + 1], T, 5, ids=ids[r:r + 1], **kw)
                for s in range(5):
                    _same([x[r:r + 1] for x in _cand(ref, s)], _cand(alone, s), "row %d alone, candidate %d" % (r, s))
            # best_of = 8: candidates s < 5 are the same
            eight = _bo(ctx, mel10, base[:n], prompts, T, 8, ids=ids[:n], **kw)
            for s in range(5):
                _same(_cand(eight, s), _cand(ref, s), "best_of 8, candidate %d" % s)
            # 40 windows = 200 rows: several decode groups, on 1 lane, 3 lanes and the default
            try:
                for lanes in (1, 3, 0):
                    ctx.set_lanes(lanes)
                    big = _bo(ctx, mel10, base, prompts40, T, 5, ids=ids, **kw)
                    for s in range(5):
                        _same([x[:n] for x in _cand(big, s)], _cand(ref, s), "40 windows, lanes %d, candidate %d" % (lanes, s))
                    for r in (17, 39):   # rows of the later groups, against the row alone
                        alone = _bo(ctx, mel10, base[r:r + 1], prompts40[r:r + 1], T, 5, ids=ids[r:r + 1], **kw)
                        for s in (0, 4):
                            _same([x[r:r + 1] for x in _cand(big, s)], _cand(alone, s), "row %d of 40, lanes %d" % (r, lanes))
            finally:
                ctx.set_lanes(0)
    finally:
        _rules(ctx, False)


# ---------------------------------------------------------------- 4. the candidates follow the oracle and the numpy noise
def test_candidates_follow_the_oracle_and_the_numpy_noise(lively, pkg):
    """test_sampling_follows_the_oracle_and_the_numpy_noise for the candidates s >= 1: every choice is the arg-max of the
    oracle's filtered row / T plus the Gumbel noise of counter {n >> 2, gi, id_b, s}, and every returned log-prob is the
    oracle's within 2 x _scaled_margin (the same rules, imported)."""
    dims, _, sd, ctx = lively
    pcm = tones(4)
    mel = ctx.logmel(pcm, out_dtype=np.float32)
    xa = ctx.encode_mel(mel)
    base = np.arange(4, dtype=np.int64) * 240000
    prompts = np.tile(np.array(PROMPT, np.int32), (4, 1))
    new, seed, differ = 20, 1234, 0
    for rules in (False, True):
        _rules(ctx, rules)
        try:
            for T, ids in ((0.5, None), (1.0, np.array([9, (5 << 16) | 2, 70000, 1], np.uint32))):
                r = _bo(ctx, mel, base, prompts, T, 3, new=new, eot=-1, ids=ids, seed=seed, ns=False)
                inv_T = float(np.float32(1.0 / T))
                for b in range(4):
                    idb = b if ids is None else int(ids[b])
                    for s in (1, 2):
                        toks = r.tokens[b, s]
                        differ += int(not np.array_equal(toks, r.tokens[b, 0]))
                        seq = np.concatenate([PROMPT, toks])[None, :-1]
                        ref = R.decode_logits(sd, dims, seq, xa[b:b + 1])[0].numpy()
                        rows = _filtered_rows(ref, toks, len(PROMPT), SPECIALS if rules else [], [EOT] if rules else [],
                                              (TS, EOT, MAXI) if rules else None)
                        for i in range(new):
                            _check_sampled(rows[i], ref[len(PROMPT) - 1 + i], int(toks[i]), inv_T,
                                           gumbel_cand_np(seed, idb, s, i, np.arange(dims["n_vocab"])))
                        # the candidate's log-probs (what best_out ranks by) are the temperature-1 filtered ones of the oracle
                        for i in range(new):
                            row, forced, gap, alt = rows[i]
                            mg = _scaled_margin(ref[len(PROMPT) - 1 + i])
                            tok = int(toks[i])
                            d = min(abs(float(torch.log_softmax(c, 0)[tok]) - float(r.logprobs[b, s, i]))
                                    for c in [row] + ([alt] if abs(gap) < mg else []))
                            assert d <= 2 * mg, (rules, T, b, s, i, d)
        finally:
            _rules(ctx, False)
    assert differ >= 1   # across all windows, a candidate s >= 1 differs from candidate 0


# ---------------------------------------------------------------- 5. early stop per candidate
def test_early_stop_is_per_candidate_and_equals_a_full_decode(lively, pkg, mel10):
    dims, sd_np, _, _ = lively
    b = pkg.binding
    dbg = b.Context(dims, debug=True)     # the debug library: its own tuning knobs (no_early_stop)
    try:
        dbg.load_state_dict(sd_np)
        dbg.finalize()
        _rules(dbg)
        import ctypes
        dbg.lib.wmdbg_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_int]
        n, T, new = 7, 1.0, 32
        base, ids = _base(n), _ids(n)
        prompts = _uniform_prompts(n)
        free = _bo(dbg, mel10, base, prompts, T, 5, new=new, eot=-1, ids=ids, seed=5)
        vals, cnt = np.unique(free.tokens[:, :, 2:], return_counts=True)
        eot = int(vals[np.argmax(cnt)])      # a frequent token plays eot: candidates stop at different lengths
        budgets = [32, 3, 40, 1, 17, 9, 25]
        got = _bo(dbg, mel10, base, prompts, T, 5, new=new, eot=eot, ids=ids, seed=5, budgets=budgets)
        assert dbg.lib.wmdbg_set_tuning(b"no_early_stop", 1) == 0
        try:
            full = _bo(dbg, mel10, base, prompts, T, 5, new=new, eot=eot, ids=ids, seed=5, budgets=budgets)
        finally:
            dbg.lib.wmdbg_set_tuning(b"no_early_stop", 0)
        for s in range(5):
            _same(_cand(got, s), _cand(full, s), "candidate %d against no_early_stop" % s)
        assert any(len(set(int(x) for x in got.lens[w])) > 1 for w in range(n))    # one window, different lengths
        for w in range(n):
            for s in range(5):
                ln = int(got.lens[w, s])
                assert 1 <= ln <= min(new, budgets[w])
                assert np.all(got.tokens[w, s, ln:] == eot) and not got.logprobs[w, s, ln:].any()
                assert ln == min(new, budgets[w]) or got.tokens[w, s, ln - 1] == eot
                # up to its length a candidate is the free-running decode (the budget and eot only cut it)
                assert np.array_equal(got.tokens[w, s, :ln], free.tokens[w, s, :ln])
    finally:
        _rules(dbg, False)
        dbg.close()


# ---------------------------------------------------------------- 6. ranking and outputs
def test_best_is_the_numpy_ranker_on_the_returned_candidates(lively, pkg, mel10):
    _, _, _, ctx = lively
    _rules(ctx)
    try:
        n = 12
        base, ids = _base(n), _ids(n)
        prompts = _uniform_prompts(n)
        seen = set()
        for pen in (None, 0.0, 0.6, 1.0):
            r = _bo(ctx, mel10, base, prompts, 1.0, 5, ids=ids, pen=pen)
            want, _ = rank_np(r.tokens, r.lens, r.logprobs, EOT, pen)
            assert np.array_equal(r.best, want), pen
            seen |= set(int(x) for x in r.best)
            rows = np.arange(n)
            sel = r.selected
            assert np.array_equal(sel.tokens, r.tokens[rows, r.best]) and np.array_equal(sel.lens, r.lens[rows, r.best])
            assert np.array_equal(sel.logprobs, r.logprobs[rows, r.best]) and np.array_equal(sel.candidate, r.best)
            assert np.array_equal(sel.no_speech_prob, r.no_speech_prob)
            # Context.transcribe_mel(best_of=) forwards: the selected rows
            fw = ctx.transcribe_mel(mel10, base, 3000, 0, 3000, prompts, NEW, eot=EOT, temperature=1.0, seed=77,
                                    no_speech_token=NS_TOK, sample_ids=ids, best_of=5, length_penalty=pen)
            assert np.array_equal(fw.tokens, sel.tokens) and np.array_equal(fw.logprobs, sel.logprobs)
            assert np.array_equal(fw.candidate, r.best)
        assert len(seen) > 1     # not always candidate 0
        r0 = _bo(ctx, mel10, base, prompts, 0.0, 5, ids=ids)
        assert np.all(r0.best == 0) and all(np.array_equal(r0.tokens[:, s], r0.tokens[:, 0]) for s in range(5))
        # best_out without the log-prob output: the library ranks by its own copy
        import ctypes
        bnd = pkg.binding
        toks = np.empty((n, 5, NEW), np.int32)
        lens = np.empty((n, 5), np.int32)
        best = np.empty(n, np.int32)
        opts = bnd.wm_decode_opts(1.0, 77, -1, 0)
        mlen = np.full(n, 3000, np.int32)
        sk = np.zeros(n, np.int32)
        P = bnd._ptr
        st = ctx.lib.wm_transcribe_mel_best_of(ctx.handle, P(mel10), P(base), P(mlen), P(sk), P(mlen), n, P(prompts), 3, None, 0,
                                               P(ids), 5, float("nan"), NEW, EOT, ctypes.byref(opts), P(toks), P(lens), None,
                                               None, P(best), bnd.WM_MEM_HOST)
        assert st == 0, ctx.lib.wm_last_error()
        ref = _bo(ctx, mel10, base, prompts, 1.0, 5, ids=ids)
        assert np.array_equal(toks, ref.tokens) and np.array_equal(best, ref.best)
    finally:
        _rules(ctx, False)


# ---------------------------------------------------------------- 7. the candidates share the encoder and the cross cache
def test_encoder_and_cross_kv_run_once_per_window(lively, pkg, mel10):
    dims, _, _, ctx = lively
    n, new = 4, 6
    base, ids = _base(n), _ids(n)
    prompts = _uniform_prompts(n)
    profs = {}
    for N in (1, 5):
        ctx.profile_reset()
        ctx.profile_enable(True)
        try:
            _bo(ctx, mel10, base, prompts, 1.0, N, new=new, eot=-1, ids=ids, ns=False)
            profs[N] = ctx.profile()
        finally:
            ctx.profile_enable(False)
    for fam in ("mel_time_major", "gemm_gelu_bf16", "gemm_conv2_f32", "gemm_qkv_enc", "enc_attention", "gemm_resid_f32",
                "layernorm", "gemm_xkv"):
        assert profs[5][fam]["n"] == profs[1][fam]["n"] > 0, fam
    assert profs[1]["gemm_xkv"]["n"] == dims["n_text_layer"]
    positions = prompts.shape[1] + new - 1
    assert profs[5]["dec_attn_cross_cand"]["n"] == dims["n_text_layer"] * positions   # once per layer and position
    assert "dec_attn_cross_cand" not in profs[1]
    assert "dec_attn_cross" not in profs[5] and "dec_attn_cross_fq" not in profs[5]


# ---------------------------------------------------------------- 8. invalid arguments
def test_invalid_arguments_are_rejected_with_a_message(lively, pkg, mel10):
    _, _, _, ctx = lively
    b = pkg.binding
    base = _base(2)
    prompts = _uniform_prompts(2)

    def bad(**kw):
        args = dict(T=1.0, N=5, prompts=prompts)
        args.update(kw)
        with pytest.raises(b.WhisperError) as e:
            _bo(ctx, mel10, base, args.pop("prompts"), args.pop("T"), args.pop("N"), **args)
        assert e.value.status == WM_ERR_INVALID and len(str(e.value)) > len("wm status 1: "), kw
        return str(e.value)

    assert "best_of" in bad(N=0)
    assert "best_of" in bad(N=9)
    assert "best_of" in bad(N=-1)
    for pen in (-0.1, 1.5, float("inf"), float("-inf")):
        assert "length_penalty" in bad(pen=pen)
    bad(T=-1.0)
    bad(T=float("nan"))
    bad(sot_index=3)                                            # outside the prompt (uniform call)
    bad(new=448)                                                # prompt + new tokens beyond the context
    bad(budgets=[4, 4, 4])                                      # budgets for another row count
    bad(prompts=np.array([[1, 2, 5000], [1, 2, 3]], np.int32))  # a token outside the vocabulary
    bad(prompts=[[1, 2, 3], [4]], sot_tail=2)                   # ragged: sot_tail beyond the shortest prompt
    with pytest.raises(b.WhisperError):                        # ragged: a prompt length of 0
        ctx.transcribe_mel_best_of(mel10, base, 3000, 0, 3000, prompts, 4, 5, temperature=1.0,
                                   prompt_len=np.array([3, 0], np.int32), sot_tail=1)
    with pytest.raises(b.WhisperError):                        # a window outside its block
        ctx.transcribe_mel_best_of(mel10, base, 3000, 10, 3000, prompts, 4, 5, temperature=1.0)
    # budgets armed for a rejected call do not leak into the next one
    with pytest.raises(b.WhisperError):
        _bo(ctx, mel10, base, prompts, 1.0, 9, budgets=[1, 1])
    ok = _bo(ctx, mel10, base, prompts, 1.0, 2, eot=-1, new=4)
    assert np.all(ok.lens == 4)


# ---------------------------------------------------------------- 9. transcribe_long(best_of=5)
def test_transcribe_long_best_of(prod, pkg):
    b = pkg.binding
    recs = _long_recs()[:3]
    ids = [7, 300, 65535]
    # (a) the synthetic model fails the default log-prob threshold on every window, so the windows whose kept step is
    # temperature 0 are those of a run without that threshold: there best_of changes nothing but the new key
    nofb = dict(logprob_threshold=None, compression_ratio_threshold=None)
    plain = prod.transcribe_long(recs, recording_ids=ids, **_kw(**nofb))
    got = prod.transcribe_long(recs, recording_ids=ids, best_of=5, **_kw(**nofb))
    compared = 0
    for o, p in zip(got, plain):
        assert len(o["windows"]) == len(p["windows"]) and o["segments"] == p["segments"] and o["seeks"] == p["seeks"]
        for w, pw in zip(o["windows"], p["windows"]):
            assert w["temperatures"] == [0.0] and w["candidate"] == 0 and "candidate" not in pw
            assert {k: v for k, v in w.items() if k != "candidate"} == pw
            compared += 1
    assert compared >= 6
    # (b) every window falls back: the later steps are direct best-of calls on the same subsets (checked while the
    # recordings' log-mel is still on the device)
    calls, checked = [], []
    real = prod.transcribe_mel

    def spy(*a, **kw):
        r = real(*a, **kw)
        calls.append(kw)
        if "best_of" in kw and len(checked) < 6:
            kw2 = {k: v for k, v in kw.items() if k not in ("best_of", "length_penalty")}
            d = prod.transcribe_mel_best_of(*a[:7], 5, length_penalty=0.5, **kw2)
            assert np.array_equal(d.selected.tokens, r.tokens) and np.array_equal(d.selected.logprobs, r.logprobs)
            assert np.array_equal(d.selected.lens, r.lens) and np.array_equal(d.best, r.candidate)
            want, _ = rank_np(d.tokens, d.lens, d.logprobs, kw["eot"], 0.5)
            assert np.array_equal(d.best, want)
            # and candidate 0 is the call without candidates
            one = real(*a, **kw2)
            assert np.array_equal(d.tokens[:, 0], one.tokens) and np.array_equal(d.logprobs[:, 0], one.logprobs)
            checked.append(len(r.lens))
        return r
    prod.transcribe_mel = spy
    try:
        forced = prod.transcribe_long(recs, recording_ids=ids, best_of=5, length_penalty=0.5,
                                      temperatures=(0.0, 0.4, 0.8), **_kw(logprob_threshold=0.0))
    finally:
        del prod.transcribe_mel
    sampled = [c for c in calls if c["temperature"] > 0]
    assert len(checked) >= 2 and sampled and all(c["best_of"] == 5 and c["length_penalty"] == 0.5 for c in sampled)
    assert all("best_of" not in c for c in calls if c["temperature"] == 0)
    kept = [w for o in forced for w in o["windows"]]
    assert all(0 <= w["candidate"] < 5 for w in kept) and any(w["candidate"] > 0 for w in kept)
    assert all(w["temperatures"][-1] > 0 for w in kept)
