"""GPU tests of the top-n alternatives and the entropy per generated token (wm_request_alternatives)
through the transcribe entries, on the `lively` tiny model of test_model_gpu.py (V = 1024) with the fixtures of
tests/test_sampling_rules_gpu.py.  B <= 5, max_new <= 16.

A request must change nothing else (bit for bit), its first entry must be the decode's own token and log-prob at temperature 0,
a row's values must not depend on the group, and the ids must pass the project's own-logits standard (test_repetition_gpu.py,
test_sampling_rules_gpu.py): the GPU's tokens are teacher-forced through ctx.decode_logits, openai-whisper's filters are applied
to those rows, and the list is compared with tests/alt_ref.py on them.  Own-logits tolerances: the teacher-forced pass and the
decode step agree to 1e-4 in a log-prob (the gate of those files), so the j-th listed id must hold a value within 1e-4 of the
j-th best admissible value (exact ids wherever the values are further apart), its log-prob lies within 1e-4 and the entropy
within 2e-4 * max(1, H)."""
import ctypes

import numpy as np
import pytest
import torch

import alt_ref as A
from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)
from test_sampling_rules_gpu import PROMPT, fresh, same, same_result, world  # noqa: F401  (world: module fixture)
from test_transcribe_options_gpu import EOT, MAXI, SPECIALS, TS, _filtered_rows, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
B, NEW, N_ALT = 5, 12, 5
RAGGED = [[10, 21, 5], [7, 9, 10, 21, 5], [5, 5, 5, 5, 5, 5, 10, 21, 5], [4, 8, 10, 21, 5], [10, 21, 5]]


def mel_args(w, rows=B):
    return (w["mel"][:rows].reshape(-1), np.arange(rows, dtype=np.int64) * 80 * 3000, 3000, 0, 3000)


def entries(w, alternatives, T, seed=11):
    """Every served kind of entry once, on the first B rows: plain, mel, ragged prompts, best-of 3, a window set, aligned"""
    ctx, ma = w["ctx"], mel_args(w)
    kw = dict(eot=EOT, temperature=T, seed=seed, alternatives=alternatives)
    out = {}
    out["transcribe"] = ctx.transcribe(w["pcm"][:B], PROMPT, NEW, no_speech_token=1000, **kw)
    out["mel"] = ctx.transcribe_mel(*ma, PROMPT, NEW, **kw)
    out["ragged"] = ctx.transcribe_mel(*ma, RAGGED, NEW, sot_tail=3, **kw)
    out["best_of"] = ctx.transcribe_mel_best_of(*ma, PROMPT, NEW, 3, **kw)
    with ctx.encode_windows(*mel_args(w, 8)) as ws:
        out["windows"] = ctx.transcribe_windows(ws, [6, 1, 3, 0, 2], PROMPT, NEW, **kw)
    out["aligned"] = ctx.transcribe_mel_aligned(*ma, PROMPT, NEW, **kw)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_result(r, T, name):
    """What every result with alternatives must satisfy on its own: shapes, pads, order, and the link to the decode's token"""
    toks, lens, lp = r.tokens.reshape(-1, NEW), r.lens.reshape(-1), r.logprobs.reshape(-1, NEW)
    at, al = r.alt_tokens.reshape(-1, NEW, N_ALT), r.alt_logprobs.reshape(-1, NEW, N_ALT)
    ac, en = r.alt_counts.reshape(-1, NEW), r.entropy.reshape(-1, NEW)
    hits = 0
    for b in range(toks.shape[0]):
        n = int(lens[b])
        assert np.all(at[b, n:] == -1) and np.all(bits(al[b, n:]) == 0) and np.all(ac[b, n:] == 0) and np.all(bits(en[b, n:]) == 0)
        for i in range(n):
            c = int(ac[b, i])
            assert 1 <= c <= N_ALT, (name, b, i, c)       # the position that stops a row has its values too
            assert np.all(at[b, i, c:] == -1) and np.all(bits(al[b, i, c:]) == 0)
            assert np.all(at[b, i, :c] >= 0) and np.all(np.diff(al[b, i, :c]) <= 0) and np.all(al[b, i, :c] <= 1e-6)
            assert len(set(at[b, i, :c].tolist())) == c
            assert en[b, i] >= 0 and np.isfinite(en[b, i])
            if T == 0:
                assert at[b, i, 0] == toks[b, i] and bits(al[b, i, 0]) == bits(lp[b, i]), (name, b, i)
            where = np.flatnonzero(at[b, i, :c] == toks[b, i])
            if where.size:       # the drawn token, where it is listed, has the decode's own log-prob bits
                assert bits(al[b, i, where[0]]) == bits(lp[b, i]), (name, b, i)
                hits += 1
    return hits


def same_alternatives(a, b, rows=slice(None)):
    return (same(a.alt_tokens[rows], b.alt_tokens[rows]) and same(a.alt_logprobs[rows], b.alt_logprobs[rows])
            and same(a.alt_counts[rows], b.alt_counts[rows]) and same(a.entropy[rows], b.entropy[rows]))


class Config:
    """One setting of the context's other rules around a block of calls"""

    def __init__(self, ctx, kind):
        self.ctx, self.kind = ctx, kind

    def __enter__(self):
        _rules(self.ctx, True)
        if self.kind == "sampling":
            self.ctx.set_sampling_rules(8, 0.9, 0.0)
        if self.kind == "rep_bias":
            self.ctx.set_repetition_rules(1.3, 3, EOT)
            self.ctx.set_sequence_bias({(17,): 1.5, (33, 34): 2.0, (40,): -np.inf}, eot=EOT)

    def __exit__(self, *exc):
        self.ctx.set_sampling_rules()
        self.ctx.set_sequence_bias(None)
        self.ctx.set_repetition_rules()
        _rules(self.ctx, False)


@pytest.mark.parametrize("kind", ["plain", "sampling", "rep_bias"])
@pytest.mark.parametrize("T", [0.0, 0.7])
def test_a_request_changes_nothing_else_and_lists_the_decodes_own_token(world, T, kind):
    """Every served entry with a request returns the tokens, lens, log-probs, no_speech_prob (and start frames) of the same call
    without one, bit for bit; and the lists are consistent with them."""
    with Config(world["ctx"], kind):
        off = entries(world, None, T)
        on = entries(world, N_ALT, T)
        for name in off:
            assert off[name].alt_tokens is None and off[name].entropy is None
            assert same_result(on[name], off[name]), (name, T, kind)
            hits = check_result(on[name], T, name)
            assert hits >= (on[name].lens.sum() if T == 0 else 1), name
        assert same(on["transcribe"].no_speech_prob, off["transcribe"].no_speech_prob)
        assert same(on["aligned"].start_frames, off["aligned"].start_frames)
        assert same(on["best_of"].best, off["best_of"].best)
        # the entries that decode the same rows list the same alternatives; best-of candidate 0 is the plain call
        assert same_alternatives(on["mel"], on["aligned"])
        bo = on["best_of"]
        for a, b_ in ((bo.alt_tokens[:, 0], on["mel"].alt_tokens), (bo.alt_logprobs[:, 0], on["mel"].alt_logprobs),
                      (bo.alt_counts[:, 0], on["mel"].alt_counts), (bo.entropy[:, 0], on["mel"].entropy)):
            assert same(a, b_)
        rows = np.arange(B)
        assert same(bo.selected.alt_tokens, bo.alt_tokens[rows, bo.best]) and same(bo.selected.entropy, bo.entropy[rows, bo.best])
        if T > 0:
            assert (bo.alt_tokens[:, 1] != bo.alt_tokens[:, 0]).any()       # the candidates' histories differ, so do their lists


def test_greedy_entry_budgets_and_the_request_is_consumed(world):
    """wm_transcribe_greedy serves a request (it turns the extended decode on); a budget-stopped row has values at its last
    token and pads behind; the next call writes nothing into the old buffers."""
    ctx, pcm = world["ctx"], world["pcm"][:B]
    budgets = [12, 5, 1, 9, 12]
    with Config(ctx, "plain"):
        want_t, want_l = ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=EOT, budgets=budgets)
        ref = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, budgets=budgets, alternatives=N_ALT)
        alt = ctx.request_alternatives(N_ALT, B, NEW)
        got_t, got_l = ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=EOT, budgets=budgets)
        assert same(got_t, want_t) and same(got_l, want_l) and same(ref.tokens, want_t)
        assert same(alt.tokens, ref.alt_tokens) and same(alt.logprobs, ref.alt_logprobs) and same(alt.entropy, ref.entropy)
        assert list(got_l) == [min(b_, int(n)) for b_, n in zip(budgets, got_l)] and got_l[2] == 1
        for b in range(B):
            n = int(got_l[b])
            assert alt.counts[b, n - 1] >= 1 and alt.tokens[b, n - 1, 0] == got_t[b, n - 1]
            assert np.all(alt.counts[b, n:] == 0) and np.all(alt.tokens[b, n:] == -1)
        # consumed: a second call -- other tokens -- leaves the old buffers alone
        keep = [a.copy() for a in (alt.tokens, alt.logprobs, alt.counts, alt.entropy)]
        other = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, temperature=1.0, seed=3)
        assert not same(other.tokens, want_t) and other.alt_tokens is None
        for a, k in zip((alt.tokens, alt.logprobs, alt.counts, alt.entropy), keep):
            assert same(a, k)
        # entropy not requested: the other three are the same
        a2 = ctx.request_alternatives(N_ALT, B, NEW, entropy=False)
        ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=EOT, budgets=budgets)
        assert a2.entropy is None and same(a2.tokens, alt.tokens) and same(a2.logprobs, alt.logprobs) and same(a2.counts, alt.counts)
        # a dropped request is not served
        a3 = ctx.request_alternatives(N_ALT, B, NEW)
        assert ctx.request_alternatives(None, 0, 0) is None
        ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=EOT)
        assert np.all(a3.tokens == -1) and np.all(a3.counts == 0)


def test_a_row_alone_is_the_row_among_others_across_groups_and_lanes(world):
    """The same bits for a row alone, a subset, one lane, two and three lanes (the call's rows cut into as many decode groups),
    and for n = 16 and n = 5 (the first five entries)."""
    ctx, pcm = world["ctx"], world["pcm"][:B]
    with Config(ctx, "sampling"):
        def run(p=pcm, n=N_ALT):
            return ctx.transcribe(p, PROMPT, NEW, eot=EOT, temperature=1.0, seed=99, alternatives=n)
        base = run()
        for lanes in (1, 2, 3):
            ctx.set_lanes(lanes)
            try:
                r = run()
                assert same_result(r, base) and same_alternatives(r, base), lanes
            finally:
                ctx.set_lanes(0)
        for idx in (slice(0, 1), slice(0, 3)):
            r = run(pcm[idx])
            assert same(r.tokens, base.tokens[idx]) and same(r.lens, base.lens[idx]) and same(r.logprobs, base.logprobs[idx])
            assert same(r.alt_tokens, base.alt_tokens[idx]) and same(r.alt_logprobs, base.alt_logprobs[idx])
            assert same(r.alt_counts, base.alt_counts[idx]) and same(r.entropy, base.entropy[idx])
        wide = run(n=16)
        assert same(wide.alt_tokens[..., :N_ALT], base.alt_tokens) and same(wide.alt_logprobs[..., :N_ALT], base.alt_logprobs)
        assert same(wide.entropy, base.entropy) and same(np.minimum(wide.alt_counts, N_ALT), base.alt_counts)
        clone = fresh(world)       # a fresh context: nothing depends on what the context ran before
        try:
            _rules(clone, True)
            clone.set_sampling_rules(8, 0.9, 0.0)
            r = clone.transcribe(pcm, PROMPT, NEW, eot=EOT, temperature=1.0, seed=99, alternatives=N_ALT)
            assert same_result(r, base) and same_alternatives(r, base)
        finally:
            clone.close()


def own_logits_check(ctx, xa, r, ts_on):
    """The own-logits standard for result r (uniform PROMPT): returns (positions checked, largest log-prob / entropy error)"""
    rows_n = r.tokens.shape[0]
    seqs = np.concatenate([np.tile(PROMPT, (rows_n, 1)), r.tokens], axis=1)[:, :-1]
    own = ctx.decode_logits(seqs, xa[:rows_n])
    n_pos, e_lp, e_h = 0, 0.0, 0.0
    for b in range(rows_n):
        rows = np.array(own[b], dtype=np.float32, copy=True)
        filt = _filtered_rows(rows, r.tokens[b], len(PROMPT), SPECIALS if ts_on else [], [EOT] if ts_on else [],
                              (TS, EOT, MAXI) if ts_on else None)
        for i in range(int(r.lens[b])):
            if abs(filt[i][2]) < 1e-3:       # a sum-rule near-tie: either allowed set is right; not restated here
                continue
            row = filt[i][0].numpy()         # f64, -inf outside the admissible set
            ref = A.alternatives_np(row, N_ALT)
            c = int(r.alt_counts[b, i])
            assert c == ref.count, (b, i, c, ref.count)
            for j in range(c):
                tok = int(r.alt_tokens[b, i, j])
                assert np.isfinite(row[tok]), (b, i, j, tok)                          # admissible
                assert abs(row[tok] - row[ref.ids[j]]) <= 1e-4, (b, i, j, tok, int(ref.ids[j]))
                lp = float(torch.log_softmax(filt[i][0], 0)[tok])
                e_lp = max(e_lp, abs(lp - float(r.alt_logprobs[b, i, j])))
            e_h = max(e_h, abs(ref.entropy - float(r.entropy[b, i])) / max(1.0, ref.entropy))
            n_pos += 1
    return n_pos, e_lp, e_h


@pytest.mark.parametrize("ts_on", [False, True])
@pytest.mark.parametrize("T", [0.0, 0.7])
def test_lists_against_the_gpus_own_logits(world, T, ts_on):
    ctx, xa = world["ctx"], world["xa"]
    _rules(ctx, ts_on)
    try:
        r = ctx.transcribe(world["pcm"][:4], PROMPT, NEW, eot=EOT if ts_on else -1, temperature=T, seed=1234, alternatives=N_ALT)
        n_pos, e_lp, e_h = own_logits_check(ctx, xa, r, ts_on)
        print("T %s ts %s: %d positions, max |dlogprob| %.3g, max |dH| / max(1, H) %.3g" % (T, ts_on, n_pos, e_lp, e_h))
        assert n_pos >= 0.9 * int(r.lens.sum())
        assert e_lp <= 1e-4 and e_h <= 2e-4
    finally:
        _rules(ctx, False)


def test_refused_entries_answer_state_and_leave_nothing_pending(world, pkg):
    """Beam search (mel and windows, plain and aligned), speculative decoding, wm_multi_transcribe_greedy and the all-f32 debug
    path answer WM_ERR_STATE with the request consumed: the next plain call is clean."""
    ctx, b, pcm, ma = world["ctx"], world["b"], world["pcm"][:B], mel_args(world)
    want = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT)

    def refused(call, c=ctx, status=WM_ERR_STATE):
        alt = c.request_alternatives(3, B, NEW)
        with pytest.raises(b.WhisperError) as e:
            call()
        assert e.value.status == status, e.value
        assert np.all(alt.tokens == -1) and np.all(alt.counts == 0)
        return alt

    def clean(alt):
        got = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT)
        assert same_result(got, want) and got.alt_tokens is None
        assert np.all(alt.tokens == -1) and np.all(alt.counts == 0)       # the refused request was consumed, not served late

    clean(refused(lambda: ctx.transcribe_mel_beam(*ma, PROMPT, NEW, 1, eot=EOT)))
    clean(refused(lambda: ctx.transcribe_mel_beam(*ma, PROMPT, NEW, 3, eot=EOT)))
    clean(refused(lambda: ctx.transcribe_mel_beam_aligned(*ma, PROMPT, NEW, 2, eot=EOT)))
    with ctx.encode_windows(*ma) as ws:
        clean(refused(lambda: ctx.transcribe_windows_beam(ws, None, PROMPT, NEW, 2, eot=EOT)))
        clean(refused(lambda: ctx.transcribe_windows_beam_aligned(ws, None, PROMPT, NEW, 2, eot=EOT)))
    draft = fresh(world)
    try:
        clean(refused(lambda: ctx.transcribe_mel_speculative(draft, *ma, PROMPT, NEW, 3, eot=EOT)))
    finally:
        draft.close()
    dbg = b.Context(world["dims"], debug=True)
    try:
        dbg.load_state_dict(world["sd_np"])
        dbg.finalize()
        dbg.set_precision(True)
        refused(lambda: dbg.transcribe(pcm, PROMPT, NEW, eot=EOT), c=dbg)
        assert dbg.transcribe(pcm[:1], PROMPT, 2).alt_tokens is None           # the f32 path without a request still runs
        dbg.set_precision(False)
        r = dbg.transcribe(pcm, PROMPT, NEW, eot=EOT, alternatives=3)         # ... and the debug library's product path serves one
        assert same_result(r, dbg.transcribe(pcm, PROMPT, NEW, eot=EOT)) and np.all(r.alt_tokens[:, 0, 0] == r.tokens[:, 0])
    finally:
        dbg.close()
    from oracle import whisper_ref as R_
    multi = b.MultiContext(dict(R_.TINY_DIMS), devices=[0])
    try:
        multi.init_synthetic(11)
        prompt = [10, 21, 5, 7]
        t0, l0 = multi.transcribe_greedy(pcm, prompt, 6)
        dc = multi.device_ctx(0)
        alt = dc.request_alternatives(3, B, 6)
        with pytest.raises(b.WhisperError) as e:
            multi.transcribe_greedy(pcm, prompt, 6)
        assert e.value.status == WM_ERR_STATE
        t1, l1 = multi.transcribe_greedy(pcm, prompt, 6)                     # consumed: the next call is the plain one
        assert same(t1, t0) and same(l1, l0) and np.all(alt.tokens == -1)
    finally:
        multi.close()
    # the Python wrappers refuse the combination before any library call
    with pytest.raises(ValueError):
        ctx.transcribe_mel(*ma, PROMPT, NEW, beam_size=2, alternatives=3)
    clean(b.Alternatives(3, B, NEW))


def test_invalid_arguments(world):
    """WM_ERR_INVALID from wm_request_alternatives for n outside 1 .. 16, null tokens / logprobs, rows or max_new below 1; from
    the CALL for rows / max_new that do not match it -- and that call still consumes the request."""
    ctx, b, pcm = world["ctx"], world["b"], world["pcm"][:B]
    fn = ctx.lib.wm_request_alternatives
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    a = b.Alternatives(4, B, NEW)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p).value

    def req(n=4, rows=B, max_new=NEW, tokens=True, logprobs=True, counts=True, entropy=True):
        return b.wm_alternatives_out(n, rows, max_new, p(a.tokens) if tokens else None, p(a.logprobs) if logprobs else None,
                                     p(a.counts) if counts else None, p(a.entropy) if entropy else None)
    want = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT)
    for bad in (req(n=0), req(n=17), req(n=-3), req(tokens=False), req(logprobs=False), req(rows=0), req(max_new=0)):
        assert fn(ctx.handle, ctypes.byref(bad)) == WM_ERR_INVALID
    assert same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT), want) and np.all(a.tokens == -1)     # nothing was left pending
    for mismatch in (req(rows=B + 1), req(rows=B - 1), req(max_new=NEW + 1), req(max_new=NEW - 1)):
        assert fn(ctx.handle, ctypes.byref(mismatch)) == 0
        with pytest.raises(b.WhisperError) as e:
            ctx.transcribe(pcm, PROMPT, NEW, eot=EOT)
        assert e.value.status == WM_ERR_INVALID
        assert same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT), want) and np.all(a.tokens == -1)   # consumed by the refused call
    # best-of: rows = B * best_of
    assert fn(ctx.handle, ctypes.byref(req(rows=B))) == 0
    with pytest.raises(b.WhisperError) as e:
        ctx.transcribe_mel_best_of(*mel_args(world), PROMPT, NEW, 3, eot=EOT, temperature=0.5)
    assert e.value.status == WM_ERR_INVALID
    # counts and entropy are optional; n = 1 and n = 16 are the ends of the range
    ok = req(counts=False, entropy=False)
    assert fn(ctx.handle, ctypes.byref(ok)) == 0
    assert same_result(ctx.transcribe(pcm, PROMPT, NEW, eot=EOT), want)
    assert np.all(a.tokens[:, 0, 0] == want.tokens[:, 0]) and np.all(a.counts == 0)
    for n in (1, 16):
        r = ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, alternatives=n)
        assert same_result(r, want) and r.alt_tokens.shape == (B, NEW, n) and np.all(r.alt_tokens[:, 0, 0] == want.tokens[:, 0])
    for bad in (0, 17, -1, 2.5, True, "3"):
        with pytest.raises(ValueError):
            ctx.transcribe(pcm, PROMPT, NEW, eot=EOT, alternatives=bad)
