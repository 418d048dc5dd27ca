"""GPU tests of given panels (wm_set_given_panel) through the transcribe entries, on the `lively` tiny model
of test_model_gpu.py (V = 1024) with the fixtures tests/test_given_gpu.py imports.  B = 5, 12 tokens.

The width is a launch policy: every comparison of library outputs is on raw bits against the SAME call at width 1 (and, for a
replay, against the call without a table).  wmdbg_last_given_panel says what the context's last group ran -- first and last
generated index, rounds, width -- and is compared with the plan of tests/given_panel_ref.py, so a silent fall-back to one
position per step fails these tests."""
import ctypes

import numpy as np
import pytest
import torch

import given_panel_ref as R
from test_alternatives_gpu import B, NEW, RAGGED, mel_args
from test_constraint_gpu import CHOICES, above
from test_given_gpu import given_of, other_texts
from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)
from test_repetition_gpu import STOP
from test_sampling_rules_gpu import PROMPT, same, same_result, world  # noqa: F401  (world: module fixture)
from test_transcribe_options_gpu import EOT, MAXI, SPECIALS, TS, _filtered_rows, _rules

pytestmark = pytest.mark.gpu

IP = ctypes.POINTER(ctypes.c_int32)
WIDTHS = (2, 3, 8)
WINDOW_ROWS = [6, 1, 3, 0, 2]
P = len(PROMPT)
BITS = R.B_GIVEN | R.B_X


@pytest.fixture(scope="module")
def dbg(world):
    """the lively model on the debug library (the accessor lives there); width 1 between tests"""
    c = world["b"].Context(world["dims"], debug=True)
    c.load_state_dict(world["sd_np"])
    c.finalize()
    c.lib.wmdbg_last_given_panel_lane.argtypes = [ctypes.c_void_p, ctypes.c_int, IP]
    c.lib.wmdbg_last_given_panel_lane.restype = ctypes.c_int
    yield c
    c.close()


def last(ctx, lane=0):
    """what the context's (lane >= 1: its lane's) last group ran"""
    out = np.full(4, -1, np.int32)
    assert ctx.lib.wmdbg_last_given_panel_lane(ctx.handle, lane, out.ctypes.data_as(IP)) == 0
    return out.tolist()


def planned(world, G, width, lens, budgets, max_new=NEW, bits=BITS, n_prompt=P):
    reason, w, Lp, rounds = R.plan(G, width, [int(x) for x in lens], None if budgets is None else [min(int(x), max_new) for x in budgets],
                                   max_new, n_prompt, world["dims"]["n_text_ctx"], bits)
    return [1, Lp - 1, rounds, w] if reason == R.SERVED else [0, 0, 0, 0]


def fields(r):
    out = [r.tokens, r.lens, r.logprobs]
    if getattr(r, "no_speech_prob", None) is not None:
        out.append(r.no_speech_prob)
    return out


def same_fields(a, b_, what):
    fa, fb = fields(a), fields(b_)
    assert len(fa) == len(fb), what
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert same(x, y), (what, i)


def at_widths(ctx, call, expect, what, widths=WIDTHS):
    """call() at width 1, then at every width: the same bits, and the accessor says what expect(width) plans"""
    ctx.set_given_panel(1)
    want = call()
    assert last(ctx) == [0, 0, 0, 0], what
    try:
        for w in widths:
            ctx.set_given_panel(w)
            same_fields(call(), want, "%s, width %d" % (what, w))
            assert last(ctx) == expect(w), (what, w, last(ctx), expect(w))
    finally:
        ctx.set_given_panel(1)
    return want


def entry_calls(ctx, world, ws, eot):
    ma = mel_args(world)
    return {
        "transcribe": lambda **kw: ctx.transcribe(world["pcm"][:B], PROMPT, NEW, eot=eot, no_speech_token=1000, **kw),
        "mel": lambda **kw: ctx.transcribe_mel(*ma, PROMPT, NEW, eot=eot, **kw),
        "windows": lambda **kw: ctx.transcribe_windows(ws, WINDOW_ROWS, PROMPT, NEW, eot=eot, **kw),
    }


@pytest.mark.parametrize("rules", [False, True], ids=["rules_off", "rules_on"])
def test_replay_at_every_width_is_the_call_without_a_table(world, dbg, rules):
    """The tokens of a temperature-0 call given back with budgets equal to the lengths (what a scoring caller passes), through
    transcribe, transcribe_mel and transcribe_windows at widths 2, 3 and 8: tokens, lens, log-probs and no_speech_prob of the
    width-1 call and of the call without a table.  Then without the early stop: every row given to the end, no budgets."""
    _rules(dbg, rules)
    try:
        with dbg.encode_windows(*mel_args(world, 8)) as ws:
            for eot in (EOT, -1):
                for name, call in entry_calls(dbg, world, ws, eot).items():
                    off = call()
                    table, lens = given_of(off.tokens, off.lens), off.lens.tolist()
                    bud = lens if eot >= 0 else None
                    assert eot >= 0 or lens == [NEW] * B
                    want = at_widths(dbg, lambda: call(given=table, budgets=bud), lambda w: planned(world, B, w, lens, bud),
                                     "%s eot %d" % (name, eot))
                    same_fields(want, off, name)
                    assert planned(world, B, 8, lens, bud)[2] >= 1, (name, lens)
    finally:
        _rules(dbg, False)


LENGTHS = [12, 7, 3, 12, 1]


def own_logits_check(ctx, xa, r, ts_on):
    """test_given_gpu.py's own-logits standard over the rows' own lengths: (finite compared, -inf seen, worst |d|)"""
    toks = np.where(np.arange(NEW)[None, :] < r.lens[:, None], r.tokens, EOT).astype(np.int32)
    seqs = np.concatenate([np.tile(PROMPT, (B, 1)), toks], axis=1)[:, :-1]
    own = ctx.decode_logits(seqs, xa[:B])
    n_fin = n_inf = 0
    worst = 0.0
    for b in range(B):
        rows = np.array(own[b], dtype=np.float32, copy=True)
        filt = _filtered_rows(rows, toks[b], P, SPECIALS if ts_on else [], [EOT] if ts_on else [], (TS, EOT, MAXI) if ts_on else None)
        for i in range(int(r.lens[b])):
            if abs(filt[i][2]) < 1e-3:       # a sum-rule near-tie: either allowed set is right; not restated here
                continue
            row, tok = filt[i][0], int(r.tokens[b, i])
            got = float(r.logprobs[b, i])
            if not torch.isfinite(row).any():
                continue
            if row[tok] == float("-inf"):
                assert got == -np.inf, (b, i, tok, got)
                n_inf += 1
            else:
                want = float(torch.log_softmax(row, 0)[tok])
                assert np.isfinite(got), (b, i, tok, got, want)
                worst = max(worst, abs(got - want))
                n_fin += 1
    return n_fin, n_inf, worst


def test_other_texts_of_lengths_12_7_3_12_1(world, dbg):
    """Texts the model would not choose, budgets equal to the lengths, under the rules: width 8 is width 1 bit for bit, the
    log-probs pass the own-logits standard at 1e-4 with -inf exactly where the filters leave the id out.  Rows 0 and 3 are the
    plain call's own tokens, which hold a timestamp the rules force at a panel row s >= 1 (an opening timestamp's partner)."""
    pcm = world["pcm"][:B]
    _rules(dbg, True)
    try:
        plain = dbg.transcribe(pcm, PROMPT, NEW)                                   # (no early stop: 12 tokens a row)
        gen = plain.tokens
        texts = other_texts(True)
        texts[0], texts[3] = gen[0].tolist(), gen[3].tolist()
        texts = [t[:n] for t, n in zip(texts, LENGTHS)]
        call = lambda: dbg.transcribe(pcm, PROMPT, NEW, eot=EOT, given=texts, budgets=LENGTHS)
        r = at_widths(dbg, call, lambda w: planned(world, B, w, LENGTHS, LENGTHS), "other texts", widths=(8,))
        assert planned(world, B, 8, LENGTHS, LENGTHS) == [1, 11, 2, 8]
        # generated token i >= 1 is row (i - 1) % 8 of its round
        forced = [(b, i) for b in (0, 3) for i in range(2, int(r.lens[b]))
                  if gen[b, i - 1] >= TS and gen[b, i - 2] < TS and (gen[b, i] >= TS or gen[b, i] == EOT) and (i - 1) % 8 >= 1]
        assert forced, gen[[0, 3]]
        for b in range(B):
            n = int(r.lens[b])
            assert r.tokens[b, :n].tolist() == texts[b][:n] and (n == LENGTHS[b] or texts[b][n - 1] == EOT)
        n_fin, n_inf, worst = own_logits_check(dbg, world["xa"], r, True)
        print("other texts: %d finite log-probs (max |d| %.3g), %d at -inf, forced at %s" % (n_fin, worst, n_inf, forced))
        assert worst <= 1e-4 and n_fin >= 12 and n_inf >= 1
    finally:
        _rules(dbg, False)


def test_a_text_with_eot_in_the_middle_stops_its_row(world, dbg):
    pcm = world["pcm"][:B]
    off = dbg.transcribe(pcm, PROMPT, NEW)
    table = given_of(off.tokens, off.lens)
    table[2][5] = EOT
    call = lambda: dbg.transcribe(pcm, PROMPT, NEW, eot=EOT, given=table, budgets=[NEW] * B)
    r = at_widths(dbg, call, lambda w: planned(world, B, w, [NEW] * B, [NEW] * B), "eot in the middle")
    ends = [t.index(EOT) + 1 if EOT in t else NEW for t in table]
    assert ends[2] <= 6 and r.lens.tolist() == ends and r.tokens[2, :ends[2]].tolist() == table[2][:ends[2]]
    for b in (0, 1, 3, 4):
        n = ends[b]
        assert r.tokens[b, :n].tolist() == table[b][:n] and same(np.ascontiguousarray(r.logprobs[b, :n]), np.ascontiguousarray(off.logprobs[b, :n]))
    n = min(ends[2], 5)
    assert same(np.ascontiguousarray(r.logprobs[2, :n]), np.ascontiguousarray(off.logprobs[2, :n]))


def test_a_prefix_then_free_decode(world, dbg):
    """lens 4 for every row, budgets 12: the phase covers [1, 4) and the free tokens behind it are the width-1 call's -- the
    restored stop state, rule state and embedding."""
    g = np.random.default_rng(8)
    for rules in (False, True):
        _rules(dbg, rules)
        try:
            pre = [[int(x) for x in g.integers(0, EOT, 4)] for _ in range(B)]
            call = lambda: dbg.transcribe_mel(*mel_args(world), PROMPT, NEW, eot=EOT, given=pre, budgets=[NEW] * B)
            r = at_widths(dbg, call, lambda w: planned(world, B, w, [4] * B, [NEW] * B), "prefix, rules %s" % rules)
            assert planned(world, B, 3, [4] * B, [NEW] * B) == [1, 3, 1, 3]
            assert r.tokens[:, :4].tolist() == pre and int(r.lens.min()) > 4
        finally:
            _rules(dbg, False)


def test_a_group_with_one_free_row_runs_no_round(world, dbg):
    pcm = world["pcm"][:B]
    off = dbg.transcribe(pcm, PROMPT, NEW)
    table = given_of(off.tokens, off.lens)
    table[3] = []
    at_widths(dbg, lambda: dbg.transcribe(pcm, PROMPT, NEW, given=table), lambda w: [0, 0, 0, 0], "a free row")


def test_unserved_configurations_run_no_round_and_the_same_bits(world, dbg):
    """Repetition rules, a sequence bias, a constraint, alternatives, temperature 0.7, ragged prompts, best-of: 0 rounds, the bits
    of width 1, no error."""
    b, pcm, ma = world["b"], world["pcm"][:B], mel_args(world)
    off = dbg.transcribe(pcm, PROMPT, NEW)
    table = given_of(off.tokens, off.lens)
    none = lambda w: [0, 0, 0, 0]

    def alt_fields(r):
        return fields(r) + [r.alt_tokens, r.alt_logprobs]
    try:
        dbg.set_repetition_rules(1.3, 3, EOT)
        at_widths(dbg, lambda: dbg.transcribe(pcm, PROMPT, NEW, eot=EOT, given=table), none, "repetition rules", widths=(8,))
        dbg.set_repetition_rules()
        dbg.set_sequence_bias({(17,): 1.5, (33, 34): 2.0, (40,): -np.inf}, eot=EOT)
        at_widths(dbg, lambda: dbg.transcribe(pcm, PROMPT, NEW, eot=EOT, given=table), none, "sequence bias", widths=(8,))
        dbg.set_sequence_bias(None)
        above(dbg)
        dbg.set_constraint(b.constraint_from_choices(CHOICES), eot=STOP)
        at_widths(dbg, lambda: dbg.transcribe(pcm, PROMPT, NEW, eot=STOP, given=table), none, "constraint", widths=(8,))
        dbg.set_constraint(None)
        _rules(dbg, False)
        want = dbg.transcribe(pcm, PROMPT, NEW, given=table, alternatives=3)
        dbg.set_given_panel(8)
        got = dbg.transcribe(pcm, PROMPT, NEW, given=table, alternatives=3)
        assert last(dbg) == [0, 0, 0, 0] and all(same(x, y) for x, y in zip(alt_fields(got), alt_fields(want)))
        dbg.set_given_panel(1)
        at_widths(dbg, lambda: dbg.transcribe(pcm, PROMPT, NEW, given=table, temperature=0.7, seed=11), none, "temperature", widths=(8,))
        at_widths(dbg, lambda: dbg.transcribe_mel(*ma, RAGGED, NEW, sot_tail=3, given=table), none, "ragged prompts", widths=(8,))
        at_widths(dbg, lambda: dbg.transcribe_mel_best_of(*ma, PROMPT, NEW, 3, given=[t for t in table for _ in range(3)]), none,
                  "best-of", widths=(8,))
    finally:
        dbg.set_constraint(None)
        dbg.set_sequence_bias(None)
        dbg.set_repetition_rules()
        _rules(dbg, False)
        dbg.set_given_panel(1)


def test_grouping_lanes_and_clones(world, dbg):
    """B = 5 alone against rows as subsets and permutations; two lanes; a clone that inherits the width."""
    pcm = world["pcm"][:B]
    _rules(dbg, True)
    try:
        texts = [t[:n] for t, n in zip(other_texts(True), LENGTHS)]
        dbg.set_given_panel(1)
        base = dbg.transcribe(pcm, PROMPT, NEW, eot=EOT, given=texts, budgets=LENGTHS)
        dbg.set_given_panel(8)
        for idx in ([0], [3, 0], [4, 3, 2, 1, 0], [1, 2, 3], [2, 0, 4, 1, 3]):
            sub = [texts[i] for i in idx]
            r = dbg.transcribe(pcm[idx], PROMPT, NEW, eot=EOT, given=sub, budgets=[LENGTHS[i] for i in idx])
            assert last(dbg) == planned(world, len(idx), 8, [LENGTHS[i] for i in idx], [LENGTHS[i] for i in idx]), idx
            assert same(r.tokens, base.tokens[idx]) and same(r.lens, base.lens[idx]) and same(r.logprobs, base.logprobs[idx]), idx
        # two lanes: 12 rows are two decode groups of 6, one per lane; each lane says what ITS group ran
        idx = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1]
        lens12 = [LENGTHS[i] for i in idx]
        dbg.set_lanes(2)
        try:
            r = dbg.transcribe(pcm[idx], PROMPT, NEW, eot=EOT, given=[texts[i] for i in idx], budgets=lens12)
            ran = sorted(last(dbg, lane) for lane in (0, 1))
        finally:
            dbg.set_lanes(0)
        assert same(r.tokens, base.tokens[idx]) and same(r.lens, base.lens[idx]) and same(r.logprobs, base.logprobs[idx])
        assert ran == sorted(planned(world, 6, 8, lens12[g:g + 6], lens12[g:g + 6]) for g in (0, 6)) and ran[0][2] >= 1, ran
        clone = dbg.clone()
        try:
            _rules(clone, True)
            assert same_result(clone.transcribe(pcm, PROMPT, NEW, eot=EOT, given=texts, budgets=LENGTHS), base)
            assert last(clone) == [1, 11, 2, 8]                                   # the width came with the clone
        finally:
            clone.close()
    finally:
        dbg.set_given_panel(1)
        _rules(dbg, False)


def test_with_prompt_panels_and_a_plain_call_after_the_phase(world, dbg):
    pcm = world["pcm"][:B]
    long_prompt = PROMPT + [int(x) for x in np.random.default_rng(4).integers(0, EOT, 9)]
    plain = dbg.transcribe(pcm, PROMPT, NEW, eot=EOT)
    off = dbg.transcribe(pcm, long_prompt, NEW)
    table = given_of(off.tokens, off.lens)
    try:
        dbg.set_prompt_panel(8)
        dbg.set_given_panel(8)
        r = dbg.transcribe(pcm, long_prompt, NEW, given=table)
        assert last(dbg) == planned(world, B, 8, [NEW] * B, None, n_prompt=len(long_prompt)) and last(dbg)[2] == 2
        same_fields(r, off, "both panels")
        # a plain call on the same context: its usual bits (graph sets, ts slots)
        same_fields(dbg.transcribe(pcm, PROMPT, NEW, eot=EOT), plain, "after the phase")
        _rules(dbg, True)
        ruled = dbg.transcribe(pcm, PROMPT, NEW, eot=EOT)
        dbg.transcribe(pcm, PROMPT, NEW, eot=EOT, given=given_of(ruled.tokens, ruled.lens), budgets=ruled.lens.tolist())
        same_fields(dbg.transcribe(pcm, PROMPT, NEW, eot=EOT), ruled, "after the phase, rules")
    finally:
        _rules(dbg, False)
        dbg.set_prompt_panel(1)
        dbg.set_given_panel(1)


def test_score_given_rows_at_width_8(world, dbg):
    b = world["b"]
    g = np.random.default_rng(21)
    texts = [[[int(x) for x in g.integers(0, EOT, n)] for n in lens] for lens in ((3, 7, 5), (6, 6, 2), (1, 4, 9), (8, 3, 3))]
    rows = [5, 0, 2, 7]
    with dbg.encode_windows(*mel_args(world, 8)) as ws:
        dbg.set_given_panel(1)
        one = b.score_given(dbg, ws, rows, PROMPT, texts, EOT, length_penalty=0.6, form="rows")
        try:
            dbg.set_given_panel(8)
            wide = b.score_given(dbg, ws, rows, PROMPT, texts, EOT, length_penalty=0.6, form="rows")
            flat = [len(t) + 1 for ts in texts for t in ts]
            assert last(dbg) == planned(world, 12, 8, flat, flat, max_new=10) and last(dbg)[2] >= 1
        finally:
            dbg.set_given_panel(1)
        best_of = b.score_given(dbg, ws, rows, PROMPT, texts, EOT, length_penalty=0.6, form="best_of")
    assert wide.best is None and same_result(wide.result, one.result)
    for w_ in range(4):
        for k in range(3):
            assert same(wide.logprobs[w_][k], one.logprobs[w_][k]) and same(wide.logprobs[w_][k], best_of.logprobs[w_][k])
    res = wide.result
    S = res.tokens.shape[-1]
    best, _ = b.rank_candidates(res.tokens.reshape(4, 3, S), res.lens.reshape(4, 3), res.logprobs.reshape(4, 3, S), EOT, 0.6)
    assert same(np.asarray(best, np.int32), np.asarray(best_of.best, np.int32))


def test_invalid_widths_leave_the_old_width_in_force(world, dbg):
    b, pcm = world["b"], world["pcm"][:B]
    off = dbg.transcribe(pcm, PROMPT, NEW)
    table = given_of(off.tokens, off.lens)
    try:
        dbg.set_given_panel(3)
        for bad in (0, 9, -1):
            with pytest.raises(b.WhisperError) as e:
                dbg.set_given_panel(bad)
            assert e.value.status == 1 and "set_given_panel: width %d outside [1, 8]" % bad in str(e.value)
        same_fields(dbg.transcribe(pcm, PROMPT, NEW, given=table), off, "width 3")
        assert last(dbg) == [1, 11, 4, 3]
    finally:
        dbg.set_given_panel(1)
