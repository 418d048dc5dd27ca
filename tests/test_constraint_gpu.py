"""GPU tests of constrained decoding (wm_set_constraint / wm_set_constraint_rows) through the transcribe
entries, on the `lively` tiny model of test_model_gpu.py and tones(4), as test_seqbias_gpu.py.

Membership is checked exactly.  The numeric standard is the project's own-logits one: the GPU's tokens are teacher-forced through
ctx.decode_logits, the numpy restatements (tests/constraint_ref.py, repeat_ref.py, seqbias_ref.py) are applied to those rows, and
the arg-max must be the GPU's token at every position, the log-prob its log-softmax within 1e-4.  Under sampling with the
sampling rules the drawn token is the arg-max of the PERTURBED scores over the kept set, not of the logits: there it must be an
id the restatement allows with the log-prob -- the filtered distribution's at temperature 1, truncation not part of it -- within
the same 1e-4, and the draw itself is held to section 20's standard (test_sampling_rules_gpu.check_own_logits) with the
constraint's bans as the row rule."""
import ctypes

import numpy as np
import pytest
import torch

import constraint_ref as CR
import repeat_ref as RR
import seqbias_ref as SB
from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)
from test_repetition_gpu import PROMPT, STOP, fresh, same
from test_transcribe_options_gpu import EOT, MAXI, SPECIALS, TS, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
NEW = 12
RAGGED = [[1, 2, 3], [7, 9, 1, 2, 3], [5, 5, 5, 5, 5, 5, 1, 2, 3], [4, 8, 1, 2, 3]]
# eight choices of 2 .. 6 text ids (all below EOT = 890, so they serve the calls with eot STOP = 1000 and with eot EOT alike);
# two share a first token, one is a prefix of another
CHOICES = [(17, 402), (17, 88, 3), (250, 31, 32, 33), (64, 63), (64, 63, 700, 701, 702, 5), (811, 9, 9), (300, 301), (5, 6, 7, 8, 9)]


@pytest.fixture(scope="module")
def world(lively, pkg):
    dims, sd_np, sd, ctx = lively
    w = dict(dims=dims, sd_np=sd_np, ctx=ctx, b=pkg.binding, pcm=tones(4), V=dims["n_vocab"])
    w["mel"] = ctx.logmel(w["pcm"], out_dtype=np.float32)
    w["mel_args"] = (w["mel"].reshape(-1), np.arange(4, dtype=np.int64) * 80 * 3000, 3000, 0, 3000)
    w["xa"] = ctx.encode_mel(w["mel"])
    w["list"] = pkg.binding.constraint_from_choices(CHOICES)
    yield w
    ctx.set_constraint(None)
    ctx.set_sequence_bias(None)
    ctx.set_repetition_rules()
    ctx.set_sampling_rules()
    _rules(ctx, False)


def above(ctx, V=1024):
    """The ids above eot = STOP are transparent to the constraint -- never banned, the suppress lists' business: the calls with
    eot = STOP suppress them, as a deployment suppresses the specials it does not want."""
    ctx.set_suppress(list(range(STOP + 1, V)), [])


def rows_of(tokens, lens):
    t, l = np.asarray(tokens), np.asarray(lens)
    return [[int(x) for x in t[i][:l[i]]] for i in np.ndindex(l.shape)]


def assert_members(tokens, lens, eot, tag, choices=CHOICES):
    for r in rows_of(tokens, lens):
        assert r and r[-1] == eot and tuple(r[:-1]) in choices, (tag, r)


def test_every_entry_generates_a_member_followed_by_eot(world):
    """Greedy, wm_transcribe at T = 0 and 1, _mel, ragged prompts, every candidate of best-of 3, every finished hypothesis of beam
    4, a window set, an aligned entry: each row is exactly a member of the list, then eot."""
    ctx, pcm, mel_args = world["ctx"], world["pcm"], world["mel_args"]
    above(ctx)
    ctx.set_constraint(world["list"], eot=STOP)
    try:
        g = ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
        assert_members(*g, STOP, "greedy")
        for T in (0.0, 1.0):
            r = ctx.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=T, seed=11)
            assert_members(r.tokens, r.lens, STOP, "transcribe T=%g" % T)
            if T == 0.0:
                assert same(r.tokens, g[0]) and same(r.lens, g[1])
            m = ctx.transcribe_mel(*mel_args, PROMPT, NEW, eot=STOP, temperature=T, seed=11)
            assert_members(m.tokens, m.lens, STOP, "mel T=%g" % T)
            rg = ctx.transcribe_mel(*mel_args, RAGGED, NEW, eot=STOP, sot_tail=3, temperature=T, seed=5)
            assert_members(rg.tokens, rg.lens, STOP, "ragged T=%g" % T)
        bo = ctx.transcribe_mel_best_of(*mel_args, PROMPT, NEW, 3, eot=STOP, temperature=1.0, seed=11)
        assert_members(bo.tokens, bo.lens, STOP, "best_of")
        assert len({tuple(r) for r in rows_of(bo.tokens, bo.lens)}) > 1          # the candidates do differ
        bm = ctx.transcribe_mel_beam(*mel_args, PROMPT, NEW, 4, eot=STOP)
        assert np.all(bm.n_hyp >= 1)
        for b in range(4):
            assert_members(bm.tokens[b, :bm.n_hyp[b]], bm.lens[b, :bm.n_hyp[b]], STOP, "beam")
        with ctx.encode_windows(*mel_args) as ws:
            wr = ctx.transcribe_windows(ws, None, PROMPT, NEW, eot=STOP, temperature=1.0, seed=11)
            assert same(wr.tokens, m.tokens) and same(wr.lens, m.lens)
            wa = ctx.transcribe_windows_aligned(ws, None, PROMPT, NEW, eot=STOP)
            assert_members(wa.tokens, wa.lens, STOP, "windows aligned")
        al = ctx.transcribe_mel_aligned(*mel_args, PROMPT, NEW, eot=STOP)
        assert_members(al.tokens, al.lens, STOP, "aligned")
        assert same(al.tokens, g[0]) and same(al.lens, g[1])
    finally:
        ctx.set_constraint(None)


def test_timestamp_rules_stay_in_charge_of_the_timestamps(world):
    """Timestamp rules on: ids above eot are transparent -- the text ids between the timestamps form a member (a prefix of one
    where max_new runs out first), and every row still starts with its forced first timestamp."""
    ctx, pcm = world["ctx"], world["pcm"]
    _rules(ctx, True)
    ctx.set_constraint(world["list"], eot=EOT)
    try:
        r = ctx.transcribe(pcm, PROMPT, 24, eot=EOT)
        full = 0
        for row in rows_of(r.tokens, r.lens):
            text = tuple(t for t in row if t < EOT)
            assert row[0] >= TS, row                                  # the first token is forced to a timestamp and the call decodes
            assert all(t >= TS or t < EOT or t == EOT for t in row)
            if row[-1] == EOT:
                assert text in CHOICES, row
                full += 1
            else:
                assert any(c[:len(text)] == text for c in CHOICES), row
        assert full >= 1
    finally:
        ctx.set_constraint(None)
        _rules(ctx, False)


def own_rows(world, tokens, prompt=PROMPT):
    seqs = np.concatenate([np.tile(prompt, (tokens.shape[0], 1)), tokens], axis=1)[:, :-1]
    return world["ctx"].decode_logits(seqs, world["xa"])


@pytest.mark.parametrize("kind", ["constraint", "constraint + (1.3, 3) + bias", "constraint + (50, 0.9, 0) at T = 0.5"])
def test_the_gpus_own_logits_under_the_constraint(world, kind):
    """The own-logits standard at every position of every row (module docstring) under a REPEATING list, so that rows run to
    max_new: the constraint alone; with the repetition rules (1.3, 3) and a bias table beside it (order: penalty, bias, the bans
    of all three OR-ed); with the sampling rules (50, 0.9, 0) at T = 0.5.  Where the three bans leave a position no id at all, the
    existing empty-set path takes over and the row is checked up to there (counted: most positions are checked)."""
    ctx, pcm, V = world["ctx"], world["pcm"], world["V"]
    pairs = [(17, 402), (250, 31), (64, 63), (811, 9), (300, 301), (5, 6), (90, 91), (120, 7)]
    auto = world["b"].constraint_from_choices(pairs, repeat=True)
    ref = CR.of_binding(auto, STOP)
    p, n = (1.3, 3) if "1.3" in kind else (1.0, 0)
    table = {(17,): 2.0, (402, 250): -float("inf"), (63, 5): 1.5} if "bias" in kind else {}
    T = 0.5 if "T = 0.5" in kind else 0.0
    new = 24
    try:
        above(ctx)
        ctx.set_constraint(auto, eot=STOP)
        ctx.set_repetition_rules(p, n, STOP)
        ctx.set_sequence_bias(table or None, eot=STOP)
        if T > 0:
            ctx.set_sampling_rules(50, 0.9, 0.0)
        sref = SB.expand(list(table), list(table.values()), eot=STOP, V=V) if table else None
        r = ctx.transcribe(pcm, PROMPT, new, eot=STOP, temperature=T, seed=21)
        own = own_rows(world, r.tokens)
        checked, worst = 0, 0.0
        for b in range(4):
            for i in range(int(r.lens[b])):
                hist = r.tokens[b, :i]
                row, banned = RR.apply_rules(np.array(own[b][len(PROMPT) - 1 + i], np.float32), hist, p, n, STOP)
                if sref is not None:
                    row, sbanned = SB.apply_bias(row, sref, hist)
                    banned = banned | sbanned
                banned = banned | CR.banned_mask(ref, 0, hist, V)
                banned[STOP + 1:] = True                                   # the suppress list
                if banned.all() or not np.isfinite(row[~banned]).any():
                    break
                tok = int(r.tokens[b, i])
                assert not banned[tok], (kind, b, i, tok)
                rg = torch.as_tensor(row).double()
                rg[torch.as_tensor(banned)] = float("-inf")
                if T == 0.0:
                    assert int(torch.argmax(rg)) == tok, (kind, b, i, tok, int(torch.argmax(rg)))
                d = abs(float(torch.log_softmax(rg, 0)[tok]) - float(r.logprobs[b, i]))
                worst = max(worst, d)
                assert d <= 1e-4, (kind, b, i, d)
                checked += 1
        print("%s: %d positions checked, worst |log-prob - own log-softmax| %.2e" % (kind, checked, worst))
        assert checked >= 3 * new
        if T > 0:
            # ... and the draw itself, by section 20's standard (test_sampling_rules_gpu.check_own_logits: the token is the arg-max
            # of value / T + Gumbel noise over the KEPT set of the filtered row), with the constraint's bans as the row rule
            import test_sampling_rules_gpu as SR

            def row_rules(row, hist):
                banned = CR.banned_mask(ref, 0, hist, V)
                banned[STOP + 1:] = True
                return row, banned
            rs = ctx.transcribe(pcm, SR.PROMPT, SR.NEW, temperature=T, seed=21)         # (no eot: every position is generated)
            n_pos, n_near = SR.check_own_logits(ctx, world["xa"], rs, (50, 0.9, 0.0), T, 21, False, V, row_rules=row_rules)
            print("the draw: %d positions, %d inside the slack" % (n_pos, n_near))
            assert n_pos == 4 * SR.NEW and n_near <= 0.10 * n_pos
    finally:
        ctx.set_sampling_rules()
        ctx.set_sequence_bias(None)
        ctx.set_repetition_rules()
        ctx.set_constraint(None)


def test_a_single_choice_is_certain(world):
    ctx, pcm = world["ctx"], world["pcm"]
    above(ctx)
    ctx.set_constraint(world["b"].constraint_from_choices([CHOICES[4]]), eot=STOP)
    try:
        for r in (ctx.transcribe(pcm, PROMPT, NEW, eot=STOP), ctx.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=1.0, seed=3)):
            for b in range(4):
                assert rows_of(r.tokens, r.lens)[b] == list(CHOICES[4]) + [STOP]
                assert np.all(np.abs(r.logprobs[b, :r.lens[b]]) <= 1e-6)
    finally:
        ctx.set_constraint(None)


def test_off_is_off_and_the_all_allowing_automaton_is_the_plain_call(world):
    """Never set and set-then-cleared equal a fresh context; one accepting state with def_next = 0 equals the plain call bit for
    bit: tokens, lengths, log-probs, no_speech_prob (eot = STOP: the model's ids above it stay free as well)."""
    pcm, b = world["pcm"], world["b"]
    c = fresh(world)
    try:
        g0 = c.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
        r0 = c.transcribe(pcm, PROMPT, NEW, eot=STOP, no_speech_token=5)
        s0 = c.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=0.8, seed=3)
        c.set_constraint(world["list"], eot=STOP)
        assert not same(c.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)[0], g0[0])
        for setup in (lambda: c.set_constraint(None), lambda: c.set_constraint(b.Constraint([0, 0], [], [], [0], [1]), eot=STOP)):
            setup()
            g = c.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
            r = c.transcribe(pcm, PROMPT, NEW, eot=STOP, no_speech_token=5)
            s = c.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=0.8, seed=3)
            assert same(g0[0], g[0]) and same(g0[1], g[1])
            assert same(r0.tokens, r.tokens) and same(r0.lens, r.lens) and same(r0.logprobs, r.logprobs) and same(r0.no_speech_prob, r.no_speech_prob)
            assert same(s0.tokens, s.tokens) and same(s0.logprobs, s.logprobs)
    finally:
        c.close()


def test_rows_lanes_starts_and_two_automata_in_turn(world):
    """A row alone equals the row among others; one lane equals three.  Per-row starts over a joined automaton: a row equals the
    same row under its sub-automaton as the only one, a row on -1 the unconstrained call's row.  Two automata in turn on one
    context's captured graphs equal fresh contexts."""
    ctx, pcm, b = world["ctx"], world["pcm"], world["b"]
    parts = [b.constraint_from_choices(CHOICES[:3]), b.constraint_from_choices(CHOICES[3:6], repeat=False),
             b.constraint_from_choices([(90, 91), (120, 7)], repeat=True)]
    joined, starts = b.constraint_join(parts)
    kw = dict(eot=STOP, temperature=0.7, seed=9)
    try:
        above(ctx)
        plain = ctx.transcribe(pcm, PROMPT, NEW, **kw)
        ctx.set_constraint(world["list"], eot=STOP)
        together = ctx.transcribe(pcm, PROMPT, NEW, **kw)
        m = world["mel_args"]
        all4 = ctx.transcribe_mel(*m, PROMPT, NEW, eot=STOP)              # (temperature 0: a row does not depend on its place)
        for i in range(4):
            alone = ctx.transcribe_mel(m[0], m[1][i:i + 1], *m[2:], PROMPT, NEW, eot=STOP)
            assert same(alone.tokens[0], all4.tokens[i]) and same(alone.logprobs[0], all4.logprobs[i]), i
        ctx.set_lanes(1)
        one = ctx.transcribe(pcm, PROMPT, NEW, **kw)
        ctx.set_lanes(3)
        three = ctx.transcribe(pcm, PROMPT, NEW, **kw)
        ctx.set_lanes(0)
        assert same(one.tokens, together.tokens, three.tokens) and same(one.logprobs, together.logprobs, three.logprobs)
        # per-row starts
        ctx.set_constraint(joined, eot=STOP)
        rows = [starts[2], -1, starts[0], starts[1]]
        ctx.set_constraint_rows(rows)
        mixed = ctx.transcribe(pcm, PROMPT, NEW, **kw)
        assert same(mixed.tokens[1], plain.tokens[1]) and same(mixed.logprobs[1], plain.logprobs[1])
        for i, part in ((0, 2), (2, 0), (3, 1)):
            ctx.set_constraint(parts[part], eot=STOP)
            only = ctx.transcribe(pcm, PROMPT, NEW, **kw)
            assert same(only.tokens[i], mixed.tokens[i]) and same(only.logprobs[i], mixed.logprobs[i]), i
        # the map was consumed: the next call starts every row in state 0 of the joined automaton = parts[0]
        ctx.set_constraint(joined, eot=STOP)
        again = ctx.transcribe(pcm, PROMPT, NEW, **kw)
        assert_members(again.tokens, again.lens, STOP, "state 0", CHOICES[:3])
        # two automata in turn on this context's graphs against fresh contexts
        for auto in (parts[2], world["list"], parts[2]):
            ctx.set_constraint(auto, eot=STOP)
            got = ctx.transcribe(pcm, PROMPT, NEW, **kw)
            c = fresh(world)
            try:
                above(c)
                c.set_constraint(auto, eot=STOP)
                want = c.transcribe(pcm, PROMPT, NEW, **kw)
            finally:
                c.close()
            assert same(got.tokens, want.tokens) and same(got.lens, want.lens) and same(got.logprobs, want.logprobs)
    finally:
        ctx.set_lanes(0)
        ctx.set_constraint(None)


def test_alternatives_list_only_allowed_ids(world):
    ctx, pcm = world["ctx"], world["pcm"]
    ref = CR.of_binding(world["list"], STOP)
    above(ctx)
    ctx.set_constraint(world["list"], eot=STOP)
    try:
        r = ctx.transcribe(pcm, PROMPT, NEW, eot=STOP, alternatives=8)
        for b in range(4):
            for i in range(int(r.lens[b])):
                ok = CR.allowed(ref, CR.fold(ref, 0, r.tokens[b, :i]))
                n = int(r.alt_counts[b, i])
                assert n == min(8, int(ok.sum())) and all(ok[t] for t in r.alt_tokens[b, i, :n]), (b, i)
                assert int(r.alt_tokens[b, i, 0]) == int(r.tokens[b, i])
    finally:
        ctx.set_constraint(None)


def test_refused_entries_and_invalid_arguments(world):
    """wm_transcribe_mel_speculative and the all-f32 debug path answer WM_ERR_STATE; every invalid table is WM_ERR_INVALID and
    leaves the automaton in force; the row map needs an automaton, the call's B and states in [-1, S)."""
    ctx, b, pcm, mel_args, V = world["ctx"], world["b"], world["pcm"], world["mel_args"], world["V"]
    fn = ctx.lib.wm_set_constraint
    fn.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_int32]
    fn.restype = ctypes.c_int

    def call(beg, tok, nxt, dn, acc, eot=STOP, S=None):
        arrs = [np.ascontiguousarray(x, dt) for x, dt in ((beg, np.int32), (tok, np.int32), (nxt, np.int32), (dn, np.int32), (acc, np.uint8))]
        return fn(ctx.handle, *[a.ctypes.data_as(ctypes.c_void_p) for a in arrs], len(dn) if S is None else S, eot)
    good = ([0, 3, 4, 4], [31, 32, 999, 7], [-1, -1, -1, 2], [1, -1, -1], [0, 0, 1])
    try:
        above(ctx)
        with pytest.raises(b.WhisperError) as e:
            ctx.set_constraint_rows([0, 0, 0, 0])                         # no automaton
        assert e.value.status == WM_ERR_STATE
        ctx.set_constraint(world["list"], eot=STOP)
        want = ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
        for bad in (([1, 3, 4, 4],) + good[1:], ([0, 3, 2, 4],) + good[1:], good[:1] + ([32, 31, 999, 7],) + good[2:],
                    good[:1] + ([31, 32, 1000, 7],) + good[2:], good[:2] + ([-1, -1, -1, 3],) + good[3:], good[:2] + ([-2, -1, -1, 2],) + good[3:],
                    good[:3] + ([3, -1, -1],) + good[4:], good[:3] + ([1, -2, -1],) + good[4:], good[:2] + ([-1, -1, -1, -1],) + good[3:],
                    good[:4] + ([0, 0, 0],)):
            assert call(*bad) == WM_ERR_INVALID, bad
        assert call(*good, eot=V) == WM_ERR_INVALID and call(*good, eot=-1) == WM_ERR_INVALID
        assert call(*good, S=4097) == WM_ERR_INVALID and call(*good, S=-1) == WM_ERR_INVALID
        wide = ([0] + [65537] * 1, np.zeros(65537), np.zeros(65537), [0], [1])   # 65537 edges (refused before a token is read)
        assert call(*wide) == WM_ERR_INVALID
        assert same(ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)[0], want[0])   # the automaton in force stayed
        for rows in ([0, 0, 0, world["list"].n_states], [0, -2, 0, 0]):
            with pytest.raises(b.WhisperError) as e:
                ctx.set_constraint_rows(rows)
            assert e.value.status == WM_ERR_INVALID
        ctx.set_constraint_rows([0, 0, 0])                                 # not the call's B: refused by the call, and consumed
        with pytest.raises(b.WhisperError) as e:
            ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)
        assert e.value.status == WM_ERR_INVALID
        assert same(ctx.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)[0], want[0])
        draft = ctx.clone()
        try:
            draft.set_constraint(None)
            with pytest.raises(b.WhisperError) as e:
                ctx.transcribe_mel_speculative(draft, *mel_args, PROMPT, NEW, 4, eot=STOP)
            assert e.value.status == WM_ERR_STATE
            draft.set_constraint(world["list"], eot=STOP)                 # ... and an automaton on the draft alone
            ctx.set_constraint(None)
            with pytest.raises(b.WhisperError) as e:
                ctx.transcribe_mel_speculative(draft, *mel_args, PROMPT, NEW, 4, eot=STOP)
            assert e.value.status == WM_ERR_STATE
        finally:
            draft.close()
        ctx.set_constraint(world["list"], eot=STOP)
        cl = ctx.clone()                                                   # a later clone takes the automaton along
        try:
            assert same(cl.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP)[0], want[0])
        finally:
            cl.close()
    finally:
        ctx.set_constraint(None)
    dbg = b.Context(world["dims"], debug=True)
    try:
        dbg.load_state_dict(world["sd_np"])
        dbg.finalize()
        dbg.set_constraint(world["list"], eot=STOP)
        dbg.set_precision(True)
        with pytest.raises(b.WhisperError) as e:
            dbg.transcribe_greedy(pcm[:1], PROMPT, 4, eot=STOP)
        assert e.value.status == WM_ERR_STATE
        with pytest.raises(b.WhisperError) as e:
            dbg.set_constraint(world["list"], eot=STOP)
        assert e.value.status == WM_ERR_STATE
        dbg.set_constraint(None)                                           # switching it off is always allowed
        dbg.set_precision(False)
    finally:
        dbg.close()


def test_the_multi_device_entry_refuses_an_automaton(world, pkg):
    """wm_multi_transcribe_greedy with an automaton on a device context answers WM_ERR_STATE (not built) before anything runs;
    with the constraint cleared the same call gives what it gave before."""
    from oracle import whisper_ref as R_
    b = pkg.binding
    mc = b.MultiContext(dict(R_.TINY_DIMS), devices=[0])
    try:
        mc.init_synthetic(11)
        pcm, prompt = tones(2), [10, 21, 5, 7]
        want = mc.transcribe_greedy(pcm, prompt, 6)
        one = mc.device_ctx(0)
        one.set_constraint(world["list"], eot=STOP)
        with pytest.raises(b.WhisperError) as e:
            mc.transcribe_greedy(pcm, prompt, 6)
        assert e.value.status == WM_ERR_STATE
        one.set_constraint(None)
        got = mc.transcribe_greedy(pcm, prompt, 6)
        assert same(got[0], want[0]) and same(got[1], want[1])
    finally:
        mc.close()
