"""GPU tests of beam-search decoding: wm_transcribe_mel_beam (beam_size beams per window over one encoder pass, one
cross-attention K/V cache and one read of it; beams re-parented on the device after every token) and beam_size in
binding.transcribe_long.  The yardsticks: the EXISTING greedy calls (a beam of width 1 is the greedy decode bit for bit), the
numpy restatement of the decoder in tests/test_beam_cpu.py driven by the lists the device saw (the debug library's
wmdbg_beam_trace), and the oracle teacher-forced on every traced beam prefix.  All on the lively synthetic model; every
equality is bit-level."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from test_beam_cpu import BeamWindowNp, best_np
from test_longform_gpu import _kw, _long_recs, prod  # noqa: F401  (prod: fixture)
from test_longform_words_gpu import _words_kw, prod_vocab  # noqa: F401  (prod_vocab: fixture)
from test_model_gpu import _scaled_margin, lively, tones  # noqa: F401  (lively: fixture)
from test_ragged_prompts_gpu import NS_TOK, _prompts, _ragged, _same
from test_transcribe_options_gpu import EOT, MAXI, PROMPT, SPECIALS, TS, _filtered_rows, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID = 1   # include/whisper_mi355x.h
NEW = 16
LIST = 9             # WM_MAX_BEAM + 1
RAGGED_LENS = [3, 40, 1, 17, 2, 4, 9, 33, 5, 3, 21, 6]
f32 = np.float32


@pytest.fixture(scope="module")
def mel10(lively):
    """Ten distinct windows; a call of any size points its rows at them (mel_base repeats)."""
    _, _, _, ctx = lively
    return ctx.logmel(tones(10), out_dtype=np.float32)


@pytest.fixture(scope="module")
def dbg(lively, pkg):
    """The lively model on the debug library: the trace capture and the no_early_stop knob."""
    dims, sd_np, _, _ = lively
    c = pkg.binding.Context(dims, debug=True)
    c.load_state_dict(sd_np)
    c.finalize()
    c.lib.wmdbg_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_int]
    c.lib.wmdbg_beam_trace.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    yield c
    c.close()


def _base(n):
    return (np.arange(n, dtype=np.int64) % 10) * 240000


def _uniform_prompts(n, n_prompt=3, seed=3):
    return np.array(_prompts([n_prompt] * n, seed=seed), dtype=np.int32)


def _beam(ctx, mel, base, prompts, N, new=NEW, eot=EOT, cand=None, patience=None, budgets=None, sot_tail=None, sot_index=0, pen=None,
          ns=True):
    """wm_transcribe_mel_beam: uniform prompts (2-d array, sot_index) or ragged ones (a list of lists, sot_tail)"""
    return ctx.transcribe_mel_beam(mel, base, 3000, 0, 3000, prompts, new, N, eot=eot, patience=patience, max_candidates=cand,
                                   no_speech_token=NS_TOK if ns else -1, sot_index=sot_index, budgets=budgets, sot_tail=sot_tail,
                                   length_penalty=pen)


def _all(r):
    return [r.tokens, r.lens, r.logprobs, r.no_speech_prob, r.n_hyp, r.sum_logprob.view(np.uint32), r.best]


def _same_beam(a, b, what, rows_a=slice(None), rows_b=slice(None)):
    for k, (x, y) in enumerate(zip(_all(a), _all(b))):
        if x is None or y is None:      # (no no-speech token: no no-speech probabilities)
            assert x is None and y is None, what
            continue
        assert np.array_equal(x[rows_a], y[rows_b]), (what, ("tokens", "lens", "logprobs", "no_speech", "n_hyp", "sums", "best")[k])


def _f32_sum(lp):
    s = f32(0)
    for v in lp:
        s = f32(s + f32(v))
    return s


def _traced(dbg, *a, **kw):
    """_beam on the debug context with the trace of the call: (result, n [B][new][N], sum, tok [..][LIST], lp [..][LIST])"""
    B_, new, N = len(a[1]), kw.get("new", NEW), a[3]
    tr = np.full((B_, new, N, 2 + 2 * LIST), np.nan, f32)
    assert dbg.lib.wmdbg_beam_trace(dbg.handle, tr.ctypes.data_as(ctypes.c_void_p)) == 0
    r = _beam(dbg, *a, **kw)
    assert not np.isnan(tr[..., :2]).any()
    return r, tr[..., 0].view(np.int32), tr[..., 1], tr[..., 2:2 + LIST].view(np.int32), tr[..., 2 + LIST:]


def _replay(r, trace, w, N, cand, eot, budget):
    """BeamWindowNp of window w driven by the traced lists; checks the sums before every step on the way"""
    n, sums, tok, lp = trace
    win = BeamWindowNp(N, cand, eot, budget)
    while not win.done:
        gi = win.gi
        assert np.array_equal(np.asarray(win.sums, f32).view(np.uint32), sums[w, gi].view(np.uint32)), (w, gi)
        lists = []
        for j in range(N):
            k = int(n[w, gi, j])
            if win.sums[j] == -np.inf:
                assert k == 0, (w, gi, j)       # a dead beam has no list
            lists.append([(int(tok[w, gi, j, e]), f32(lp[w, gi, j, e])) for e in range(k)])
        win.step(lists)
    return win


def _check_replay(r, trace, N, cand, eot, new, budgets=None, pen=None):
    S = max(N, cand)
    assert r.tokens.shape[1:] == (S, new) and r.sum_logprob.shape[1] == S
    wins = []
    for w in range(r.tokens.shape[0]):
        budget = new if budgets is None else min(new, budgets[w])
        win = _replay(r, trace, w, N, cand, eot, budget)
        hyps = win.hypotheses()
        assert r.n_hyp[w] == len(hyps), w
        for h, (toks, lps, s) in enumerate(hyps):
            assert r.lens[w, h] == len(toks) and list(r.tokens[w, h, :len(toks)]) == toks, (w, h)
            assert np.array_equal(r.logprobs[w, h, :len(toks)].view(np.uint32), np.asarray(lps, f32).view(np.uint32)), (w, h)
            assert f32(r.sum_logprob[w, h]).tobytes() == f32(s).tobytes(), (w, h)
            # the returned log-probs sum, in order and in f32, to the returned sum
            assert _f32_sum(r.logprobs[w, h, :len(toks)]).tobytes() == f32(s).tobytes(), (w, h)
        pad = eot       # (eot < 0: the padding is that value)
        for h in range(S):      # padding behind every hypothesis, empty slots behind the last
            ln = int(r.lens[w, h])
            assert np.all(r.tokens[w, h, ln:] == pad) and not r.logprobs[w, h, ln:].any()
            if h >= len(hyps):
                assert ln == 0 and r.sum_logprob[w, h] == -np.inf
        assert r.best[w] == best_np(hyps, eot, pen), w
        wins.append(win)
    return wins


# ---------------------------------------------------------------- 1. beam 1 is greedy, bit for bit
@pytest.mark.parametrize("hit", [False, True])
def test_beam_1_is_the_greedy_decode(lively, pkg, mel10, hit):
    _, _, _, ctx = lively
    b = pkg.binding
    _rules(ctx)
    try:
        n = 6
        base = _base(n)
        budgets = [16, 5, 12, 1, 9, 16]
        prompts = _uniform_prompts(n, 4)
        opts = b.wm_decode_opts(0.0, 0, NS_TOK, 1)
        eot = EOT
        if hit:   # a frequent token of the free decode plays eot: rows stop at different lengths
            free = ctx.transcribe_mel_raw(mel10, base, 3000, 0, 3000, prompts, NEW, -1, opts, no_speech=True)
            vals, cnt = np.unique(free[0][:, 2:], return_counts=True)
            eot = int(vals[np.argmax(cnt)])
        for bud in (budgets, None):
            want = ctx.transcribe_mel_raw(mel10, base, 3000, 0, 3000, prompts, NEW, eot, opts, no_speech=True, budgets=bud)
            got = _beam(ctx, mel10, base, prompts, 1, eot=eot, cand=1, budgets=bud, sot_index=1)
            assert got.tokens.shape == (n, 1, NEW) and np.all(got.best == 0) and np.all(got.n_hyp == 1)
            _same([got.tokens[:, 0], got.lens[:, 0], got.logprobs[:, 0], got.no_speech_prob], want, "uniform")
            if hit:
                assert any(want[0][r, want[1][r] - 1] == eot for r in range(n)) and len(set(int(x) for x in want[1])) > 1
            for r in range(n):
                assert _f32_sum(want[2][r, :want[1][r]]).tobytes() == f32(got.sum_logprob[r, 0]).tobytes(), r
            rag = _prompts(RAGGED_LENS[:n], seed=5)
            want = _ragged(ctx, b, mel10, base, rag, 0.0, new=NEW, eot=eot, budgets=bud, sot_tail=1)
            got = _beam(ctx, mel10, base, rag, 1, eot=eot, cand=1, budgets=bud, sot_tail=1)
            _same([got.tokens[:, 0], got.lens[:, 0], got.logprobs[:, 0], got.no_speech_prob], want, "ragged")
        # rules off
        _rules(ctx, False)
        want = ctx.transcribe_mel_raw(mel10, base, 3000, 0, 3000, prompts, NEW, eot, opts, no_speech=True)
        got = _beam(ctx, mel10, base, prompts, 1, eot=eot, cand=1, sot_index=1)
        _same([got.tokens[:, 0], got.lens[:, 0], got.logprobs[:, 0], got.no_speech_prob], want, "rules off")
    finally:
        _rules(ctx, False)


# ---------------------------------------------------------------- 2. invariance
def test_a_window_depends_on_itself_only(lively, pkg, mel10):
    _, _, _, ctx = lively
    _rules(ctx)
    try:
        n = 12
        base = _base(40)
        lens40 = (RAGGED_LENS * 4)[:40]
        for prompts40, kw in ((_uniform_prompts(40), dict(sot_index=0)), (_prompts(lens40, seed=5), dict(sot_tail=1))):
            prompts = prompts40[:n]
            ref = _beam(ctx, mel10, base[:n], prompts, 5, **kw)
            for r in (0, 5, 11):    # a window alone
                alone = _beam(ctx, mel10, base[r:r + 1], prompts[r:r + 1], 5, **kw)
                _same_beam(ref, alone, "window %d alone" % r, slice(r, r + 1))
            # the same window repeated
            rep = _beam(ctx, mel10, np.repeat(base[3:4], 4), [prompts[3]] * 4 if isinstance(prompts, list) else np.repeat(prompts[3:4], 4, 0),
                        5, **kw)
            for k in range(4):
                _same_beam(ref, rep, "window 3 repeated", slice(3, 4), slice(k, k + 1))
            # 40 windows = 200 rows: several decode groups, on 1 lane, 3 lanes and the default
            try:
                for lanes in (1, 3, 0):
                    ctx.set_lanes(lanes)
                    big = _beam(ctx, mel10, base, prompts40, 5, **kw)
                    _same_beam(big, ref, "40 windows, lanes %d" % lanes, slice(0, n))
                    for r in (17, 39):
                        alone = _beam(ctx, mel10, base[r:r + 1], prompts40[r:r + 1], 5, **kw)
                        _same_beam(big, alone, "window %d of 40, lanes %d" % (r, lanes), slice(r, r + 1))
            finally:
                ctx.set_lanes(0)
    finally:
        _rules(ctx, False)


# ---------------------------------------------------------------- 3. exact replay, 5. the search really forks
@pytest.mark.parametrize("rules", [False, True])
def test_exact_replay_of_the_traced_lists_and_real_forks(lively, dbg, mel10, rules):
    _, _, _, ctx = lively
    _rules(dbg, rules)
    _rules(ctx, rules)
    try:
        n, N = 4, 5
        base = _base(n)
        prompts = np.tile(np.array(PROMPT, np.int32), (n, 1))
        r, *trace = _traced(dbg, mel10, base, prompts, N, eot=-1, ns=False)
        wins = _check_replay(r, trace, N, N, -1, NEW)
        # the traced (eager) call is the product's call, bit for bit
        _same_beam(r, _beam(ctx, mel10, base, prompts, N, eot=-1, ns=False), "debug trace vs product")
        greedy = _beam(ctx, mel10, base, prompts, 1, eot=-1, cand=1, ns=False)
        differs = 0
        for w, win in enumerate(wins):
            forks = [s for s in win.srcs[1:] if len(set(s)) < N]
            moved = [s for s in win.srcs[1:] if s != list(range(N))]
            assert forks and moved, (w, win.srcs)
            differs += int(not np.array_equal(r.tokens[w, r.best[w]], greedy.tokens[w, 0]))
        assert differs >= 1
        # with a length penalty and patience: max_candidates above the beam width, budgets, eot in play
        free = r.tokens[:, :, 2:]
        vals, cnt = np.unique(free, return_counts=True)
        eot = int(vals[np.argmax(cnt)])
        budgets = [16, 7, 12, 3]
        for cand, pen in ((8, 0.6), (2, None), (5, 1.0)):
            r2, *trace2 = _traced(dbg, mel10, base, prompts, N, eot=eot, cand=cand, budgets=budgets, pen=pen, ns=False)
            _check_replay(r2, trace2, N, cand, eot, NEW, budgets=budgets, pen=pen)
    finally:
        _rules(dbg, False)
        _rules(ctx, False)


# ---------------------------------------------------------------- 4. the lists against the oracle (proves the cache reorder)
@pytest.mark.parametrize("rules", [False, True])
def test_lists_follow_the_oracle_on_every_traced_prefix(lively, dbg, rules):
    dims, _, sd, _ = lively
    pcm = tones(4)
    mel = dbg.logmel(pcm, out_dtype=np.float32)
    xa = dbg.encode_mel(mel)
    base = np.arange(4, dtype=np.int64) * 240000
    prompts = np.tile(np.array(PROMPT, np.int32), (4, 1))
    N, new, P = 5, NEW, len(PROMPT)
    _rules(dbg, rules)
    try:
        r, n, sums, tok, lp = _traced(dbg, mel, base, prompts, N, new=new, eot=-1, ns=False)
        wins = _check_replay(r, (n, sums, tok, lp), N, N, -1, new)
        checked = worst = 0
        for w in range(4):
            # the beams' prefixes before every step, from the replay: hist[gi][j]
            win = BeamWindowNp(N, N, -1, new)
            for gi in range(new):
                live = [j for j in range(N) if win.sums[j] != -np.inf and (gi > 0 or j == 0)]
                seqs = np.array([PROMPT + win.toks[j] for j in live], np.int64)
                ref = R.decode_logits(sd, dims, seqs, np.repeat(xa[w:w + 1], len(live), 0)).numpy()
                for q, j in enumerate(live):
                    row, forced, gap, alt = _filtered_rows(ref[q], win.toks[j] + [0], P, SPECIALS if rules else [],
                                                           [EOT] if rules else [], (TS, EOT, MAXI) if rules else None)[gi]
                    mg = _scaled_margin(ref[q][P - 1 + gi])
                    k = int(n[w, gi, j])
                    assert k == N + 1, (w, gi, j, k)          # (this vocabulary always has N + 1 admissible ids)
                    ltok, llp = tok[w, gi, j, :k], lp[w, gi, j, :k]
                    assert np.all(np.diff(llp) <= 0) and len(set(int(t) for t in ltok)) == k
                    ok = False
                    for c in [row] + ([alt] if abs(gap) < mg else []):
                        lsm = torch.log_softmax(c, 0).numpy()
                        d = np.abs(lsm[ltok] - llp.astype(np.float64))
                        rest = np.delete(lsm, ltok)
                        if np.all(np.isfinite(lsm[ltok])) and d.max() <= 2 * mg and rest.max() - float(llp[-1]) <= 2 * mg:
                            ok = True
                            worst = max(worst, float(d.max() / mg))
                    assert ok, (rules, w, gi, j)
                    checked += 1
                win.step([[(int(tok[w, gi, j, e]), f32(lp[w, gi, j, e])) for e in range(int(n[w, gi, j]))] for j in range(N)])
        assert checked == 4 * (1 + (new - 1) * N)     # no traced (index, live beam) is left out
        print("beam lists vs oracle: %d lists, worst |d lp| = %.3f margins" % (checked, worst))
    finally:
        _rules(dbg, False)


# ---------------------------------------------------------------- 6. finishing
def test_windows_finish_at_different_positions_and_equal_a_full_decode(lively, dbg, mel10):
    _rules(dbg)
    try:
        n, N, new = 7, 5, 24
        base = _base(n)
        prompts = _uniform_prompts(n)
        free = _beam(dbg, mel10, base, prompts, N, new=new, eot=-1)
        assert np.all(free.n_hyp == N) and np.all(free.lens == new)
        vals, cnt = np.unique(free.tokens[:, :, 2:], return_counts=True)
        eot = int(vals[np.argmax(cnt)])      # a frequent token plays eot
        budgets = [24, 3, 40, 1, 17, 9, 24]
        for cand in (5, 8, 2):
            S = max(N, cand)
            got, *trace = _traced(dbg, mel10, base, prompts, N, new=new, eot=eot, cand=cand, budgets=budgets)
            wins = _check_replay(got, trace, N, cand, eot, new, budgets=budgets)
            assert got.tokens.shape == (n, S, new)
            plain = _beam(dbg, mel10, base, prompts, N, new=new, eot=eot, cand=cand, budgets=budgets)
            _same_beam(got, plain, "traced vs captured positions, max_candidates %d" % cand)
            assert dbg.lib.wmdbg_set_tuning(b"no_early_stop", 1) == 0
            try:
                full = _beam(dbg, mel10, base, prompts, N, new=new, eot=eot, cand=cand, budgets=budgets)
            finally:
                dbg.lib.wmdbg_set_tuning(b"no_early_stop", 0)
            _same_beam(got, full, "against no_early_stop, max_candidates %d" % cand)
            steps = [win.gi for win in wins]
            complete = [w for w, win in enumerate(wins) if len(win.finished) >= cand]
            if cand <= 5:
                assert len(complete) >= 2 and len({steps[w] for w in complete}) > 1, (cand, steps)   # complete at different positions
            for w, win in enumerate(wins):
                assert steps[w] <= min(new, budgets[w])
                nf = len(win.finished)
                assert got.n_hyp[w] == (nf if nf >= N else min(N, nf + sum(1 for s in win.sums if s != -np.inf)))
                for h in range(nf):     # a finished hypothesis ends in eot, which its length counts
                    assert got.tokens[w, h, got.lens[w, h] - 1] == eot and eot not in got.tokens[w, h, :got.lens[w, h] - 1]
                for h in range(nf, got.n_hyp[w]):   # a fill-up: the window's token count, no eot
                    assert got.lens[w, h] == steps[w] and eot not in got.tokens[w, h, :steps[w]]
    finally:
        _rules(dbg, False)


# ---------------------------------------------------------------- 7. the beams share the encoder and the cross cache
def test_profile_families(lively, pkg, mel10):
    dims, _, _, ctx = lively
    n, new = 4, 6
    base = _base(n)
    prompts = _uniform_prompts(n)
    profs = {}
    for N in (1, 5):
        ctx.profile_reset()
        ctx.profile_enable(True)
        try:
            _beam(ctx, mel10, base, prompts, N, new=new, eot=-1, cand=N, ns=False)
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
    for fam in ("beam_topk", "beam_select", "beam_reorder"):      # once per generated position
        assert profs[5][fam]["n"] == new, (fam, profs[5][fam])
    assert profs[1]["beam_topk"]["n"] == new and profs[1]["beam_select"]["n"] == new
    assert profs[5]["argmax_embed"]["n"] == prompts.shape[1] - 1    # the prompt positions close with the arg-max


# ---------------------------------------------------------------- 8. invalid arguments
def test_invalid_arguments_are_rejected_with_a_message(lively, pkg, mel10):
    _, _, _, ctx = lively
    b = pkg.binding
    base = _base(2)
    prompts = _uniform_prompts(2)

    def bad(**kw):
        args = dict(N=5, prompts=prompts)
        args.update(kw)
        with pytest.raises(b.WhisperError) as e:
            _beam(ctx, mel10, base, args.pop("prompts"), args.pop("N"), **args)
        assert e.value.status == WM_ERR_INVALID and len(str(e.value)) > len("wm status 1: "), kw
        return str(e.value)

    assert "beam_size" in bad(N=0, cand=1)
    assert "beam_size" in bad(N=9, cand=9)
    assert "max_candidates" in bad(cand=0)
    assert "max_candidates" in bad(cand=17)
    for pen in (-0.1, 1.5, float("inf")):
        assert "length_penalty" in bad(pen=pen)
    assert "vocabulary" in bad(eot=1024)
    bad(sot_index=3)                                            # outside the prompt (uniform call)
    bad(new=448)                                                # prompt + new tokens beyond the context
    bad(budgets=[4, 4, 4])                                      # budgets for another row count
    bad(prompts=np.array([[1, 2, 5000], [1, 2, 3]], np.int32))  # a token outside the vocabulary
    bad(prompts=[[1, 2, 3], [4]], sot_tail=2)                   # ragged: sot_tail beyond the shortest prompt
    with pytest.raises(b.WhisperError):                        # a window outside its block
        ctx.transcribe_mel_beam(mel10, base, 3000, 10, 3000, prompts, 4, 5)
    # temperature plays no part: anything but 0 is invalid
    toks = np.empty((2, 5, 4), np.int32)
    lens = np.empty((2, 5), np.int32)
    nh = np.empty(2, np.int32)
    sums = np.empty((2, 5), np.float32)
    mlen = np.full(2, 3000, np.int32)
    sk = np.zeros(2, np.int32)
    P = b._ptr
    for T, ok in ((0.5, False), (0.0, True)):
        opts = b.wm_decode_opts(T, 0, -1, 0)
        st = ctx.lib.wm_transcribe_mel_beam(ctx.handle, P(mel10), P(base), P(mlen), P(sk), P(mlen), 2, P(prompts), 3, None, 0, 5, 5,
                                            float("nan"), 4, -1, ctypes.byref(opts), P(toks), P(lens), P(nh), P(sums), None, None,
                                            None, b.WM_MEM_HOST)
        assert (st == 0) == ok, ctx.lib.wm_last_error()
        if not ok:
            assert st == WM_ERR_INVALID and b"temperature" in ctx.lib.wm_last_error()
    assert np.all(nh == 5) and np.all(lens == 4)
    # the binding's own checks
    with pytest.raises(ValueError):
        ctx.transcribe_mel(mel10, base, 3000, 0, 3000, prompts, 4, patience=2.0)
    with pytest.raises(ValueError):
        ctx.transcribe_mel(mel10, base, 3000, 0, 3000, prompts, 4, beam_size=5, temperature=0.5)
    # budgets armed for a rejected call do not leak into the next one
    with pytest.raises(b.WhisperError):
        _beam(ctx, mel10, base, prompts, 9, cand=9, budgets=[1, 1])
    ok = _beam(ctx, mel10, base, prompts, 2, eot=-1, new=4)
    assert np.all(ok.lens == 4) and np.all(ok.n_hyp == 2)
    # Context.transcribe_mel(beam_size=) forwards: the selected rows, the search's own sums
    r = _beam(ctx, mel10, base, prompts, 5, patience=1.6, pen=0.4)
    assert r.tokens.shape[1] == 8
    fw = ctx.transcribe_mel(mel10, base, 3000, 0, 3000, prompts, NEW, eot=EOT, no_speech_token=NS_TOK, beam_size=5, patience=1.6,
                            length_penalty=0.4)
    rows = np.arange(2)
    assert np.array_equal(fw.tokens, r.tokens[rows, r.best]) and np.array_equal(fw.logprobs, r.logprobs[rows, r.best])
    assert np.array_equal(fw.hypothesis, r.best) and np.array_equal(fw.sum_logprob, r.sum_logprob[rows, r.best].astype(np.float64))
    assert np.array_equal(fw.avg_logprob, fw.sum_logprob / (fw.n_text + 1))


# ---------------------------------------------------------------- 9. transcribe_long(beam_size=5)
def test_transcribe_long_beam(prod, pkg, prod_vocab):
    recs = _long_recs()[:3]
    ids = [7, 300, 65535]
    nofb = dict(logprob_threshold=None, compression_ratio_threshold=None)
    calls, checked = [], []
    real = prod.transcribe_mel

    def spy(*a, **kw):
        r = real(*a, **kw)
        calls.append(kw)
        if "beam_size" in kw and len(checked) < 6:   # a direct beam call on the same subset
            kw2 = {k: v for k, v in kw.items() if k not in ("beam_size", "patience", "length_penalty", "temperature", "seed", "sample_ids")}
            d = prod.transcribe_mel_beam(*a[:7], 5, patience=kw["patience"], length_penalty=kw["length_penalty"], **kw2)
            assert np.array_equal(d.selected.tokens, r.tokens) and np.array_equal(d.selected.logprobs, r.logprobs)
            assert np.array_equal(d.selected.lens, r.lens) and np.array_equal(d.best, r.hypothesis)
            assert np.array_equal(d.selected.sum_logprob, r.sum_logprob)
            checked.append(len(r.lens))
        return r
    prod.transcribe_mel = spy
    try:
        got = prod.transcribe_long(recs, recording_ids=ids, beam_size=5, patience=1.4, length_penalty=0.5, **_kw(**nofb))
    finally:
        del prod.transcribe_mel
    assert len(checked) >= 2 and all(c["temperature"] == 0 and c["beam_size"] == 5 and c["patience"] == 1.4 for c in calls)
    kept = [w for o in got for w in o["windows"]]
    assert len(kept) >= 6 and all(w["temperatures"] == [0.0] and 0 <= w["hypothesis"] < 7 for w in kept)
    for o in got:       # the segments are built from the kept hypothesis
        for w in o["windows"]:
            if not w["skipped"]:
                seg_toks = [t for sg in o["segments"] if sg["seek"] == w["seek"] for t in sg["tokens"]]
                assert seg_toks and all(t in w["tokens"] for t in seg_toks)
    # beam search changes what the recordings decode to (else the test shows nothing)
    plain = prod.transcribe_long(recs, recording_ids=ids, **_kw(**nofb))
    assert any(w["tokens"] != pw["tokens"] for o, p in zip(got, plain) for w, pw in zip(o["windows"], p["windows"]))
    # fallback above temperature 0 keeps its best_of calls; word timestamps still run
    calls.clear()
    prod.transcribe_mel = lambda *a, **kw: (calls.append(kw), real(*a, **kw))[1]
    try:
        forced = prod.transcribe_long(recs[:2], recording_ids=ids[:2], beam_size=5, best_of=3, temperatures=(0.0, 0.4),
                                      **_kw(logprob_threshold=0.0))
    finally:
        del prod.transcribe_mel
    assert all(("beam_size" in c) == (c["temperature"] == 0) and ("best_of" in c) == (c["temperature"] > 0) for c in calls)
    assert any(c["temperature"] > 0 for c in calls) and all("hypothesis" in w and "candidate" in w for o in forced for w in o["windows"])
    # word timestamps run on the kept hypotheses
    worded = prod.transcribe_long(recs[:2], recording_ids=ids[:2], beam_size=5, **_words_kw(prod_vocab, **nofb))
    segs = [sg for o in worded for sg in o["segments"]]
    assert segs and all("words" in sg for sg in segs) and any(sg["words"] for sg in segs)
