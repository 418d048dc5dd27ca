"""GPU tests of the row tables (wm_set_sequence_bias_tables / wm_set_bias_rows) through every transcribe
entry the single table serves, on the `lively` tiny model of test_model_gpu.py and tones(9).

The standard is the single table itself: a row with table t must give, BIT FOR BIT, what the same call gives that row with t as
the context's one table (wm_set_sequence_bias), and a row without a table what the call gives with the bias off.  No tolerance
appears anywhere.  Every call runs 9 rows on 3 lanes -- two decode groups at least, so a group's first row is not row 0 of the
call -- with four tables (one of them empty) and a row on -1."""
import numpy as np
import pytest

import seqbias_ref as SB
from test_longform_gpu import EOT2, _kw, _long_recs, _strip, prod  # noqa: F401  (prod: module fixture)
from test_model_gpu import lively, tones  # noqa: F401  (lively: module fixture)
from test_repetition_gpu import NEW, PROMPT, STOP, fresh, same
from test_seqbias_gpu import ngrams_of

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
INF = float("inf")
R = 9
MAP = [0, 1, 2, -1, 0, 1, 2, 3, 0]     # table of row b: three tables with entries, the empty table 3, and no table
RAGGED = [[1, 2, 3], [7, 9, 1, 2, 3], [5, 5, 5, 5, 5, 5, 1, 2, 3], [4, 8, 1, 2, 3], [1, 2, 3], [6, 1, 2, 3], [9, 9, 9, 1, 2, 3], [1, 2, 3],
          [2, 2, 1, 2, 3]]


@pytest.fixture(scope="module")
def world(lively, pkg):
    dims, sd_np, sd, ctx = lively
    w = dict(dims=dims, sd_np=sd_np, ctx=ctx, b=pkg.binding, pcm=tones(R))
    w["mel"] = ctx.logmel(w["pcm"], out_dtype=np.float32)
    w["mel_args"] = (w["mel"].reshape(-1), np.arange(R, dtype=np.int64) * 80 * 3000, 3000, 0, 3000)
    ctx.set_sequence_bias(None)
    ctx.set_repetition_rules()
    w["plain"] = ctx.transcribe_greedy(w["pcm"], PROMPT, NEW, eot=STOP)
    w["tables"], w["boosts"] = make_tables(w["plain"])
    yield w
    ctx.set_lanes(0)
    ctx.set_sequence_bias(None)
    ctx.set_repetition_rules()


def make_tables(plain):
    """Table t bans the most frequent 2-gram and 3-gram of the plain decode of every row MAP sends to it (so it changes exactly
    those rows for certain, and the other tables' bans mean nothing to them); table 1 also lifts a single id, table 2 holds a
    boosted phrase made of ids row 2 generates; table 3 is empty."""
    toks, lens = plain
    tables = [dict(), dict(), dict(), dict()]
    for b, t in enumerate(MAP):
        if t in (0, 1, 2):
            for n in (2, 3):
                seq = ngrams_of(toks[b][:lens[b]], n, STOP).most_common(1)[0][0]
                tables[t].setdefault(seq, -INF)
    first = [int(x) for x in toks[:, 0]]
    tables[1][((first[1] + 55) % (STOP - 1),)] = 3.0
    phrase = tuple(int(x) for x in toks[2, 4:7])
    boosts = [[], [], [], []]
    if phrase[-1] < STOP and phrase not in tables[2]:
        tables[2][phrase] = 6.0
        boosts[2] = [phrase]
    return tables, boosts


def fields(r):
    """the arrays of a result that every row must reproduce, by name (rows first)"""
    if isinstance(r, tuple):
        return dict(tokens=r[0], lens=r[1])
    out = dict(tokens=r.tokens, lens=r.lens, logprobs=r.logprobs)
    for k in ("no_speech_prob", "best", "start_frames"):
        if getattr(r, k, None) is not None:
            out[k] = getattr(r, k)
    if hasattr(r, "n_hyp"):       # a beam result: the hypotheses that exist, their sums
        out["n_hyp"] = r.n_hyp
        out["sum_logprob"] = r.sum_logprob
    return out


PER_HYP = ("tokens", "lens", "logprobs", "sum_logprob")


def row_of(f, b):
    """row b of every field; of a beam result the first n_hyp[b] hypotheses only (the rest is never written)"""
    n = int(f["n_hyp"][b]) if "n_hyp" in f else None
    return {k: np.ascontiguousarray(v[b][:n] if n is not None and k in PER_HYP else v[b]) for k, v in f.items()}


def rows_equal(got, b, want, wb, keys=None):
    g, w = row_of(got, b), row_of(want, wb)
    for k in keys or g:
        if not same(g[k], w[k]):
            return k
    return None


def entries(w):
    pcm, m = w["pcm"], w["mel_args"]
    kw = dict(eot=STOP, no_speech_token=5)

    def windows(c):
        with c.encode_windows(*m) as ws:
            return c.transcribe_windows(ws, None, PROMPT, NEW, temperature=0.8, seed=3, **kw)
    return {
        "greedy": lambda c: c.transcribe_greedy(pcm, PROMPT, NEW, eot=STOP),
        "transcribe T=0": lambda c: c.transcribe(pcm, PROMPT, NEW, **kw),
        "transcribe T=0.8": lambda c: c.transcribe(pcm, PROMPT, NEW, temperature=0.8, seed=11, **kw),
        "mel T=0.8": lambda c: c.transcribe_mel(*m, PROMPT, NEW, temperature=0.8, seed=7, **kw),
        "ragged": lambda c: c.transcribe_mel(*m, RAGGED, NEW, sot_tail=3, temperature=0.8, seed=5, **kw),
        "best_of 3": lambda c: c.transcribe_mel_best_of(*m, PROMPT, NEW, 3, temperature=0.8, seed=11, **kw),
        "beam 3": lambda c: c.transcribe_mel_beam(*m, PROMPT, NEW, 3, **kw),
        "windows": windows,
        "aligned": lambda c: c.transcribe_mel_aligned(*m, PROMPT, NEW, **kw),
    }


def singles(w, run):
    """the call under each table as THE table of the context, and with the bias off: {table index or -1: fields}"""
    ctx = w["ctx"]
    out = {}
    for t in (0, 1, 2):                                    # (table 3 is empty: as THE table it is the bias off)
        ctx.set_sequence_bias(w["tables"][t], boost=w["boosts"][t], eot=STOP)
        out[t] = fields(run(ctx))
    ctx.set_sequence_bias(None)
    out[-1] = fields(run(ctx))
    return out


ENTRY_NAMES = ["greedy", "transcribe T=0", "transcribe T=0.8", "mel T=0.8", "ragged", "best_of 3", "beam 3", "windows", "aligned"]


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_a_row_equals_the_single_table_call_with_its_table(world, name):
    """Every served entry: 9 rows on 3 lanes under the map; row b's tokens, lengths, log-probs, no_speech_prob and, where the entry
    has them, candidates, hypotheses, sums, ranking and start frames equal the single-table call's row b under table MAP[b], bit
    for bit; the row on -1 and the row on the empty table equal the call with the bias off.  The tables act: at temperature 0 every
    row with a non-empty table differs from the bias-off call, and in every entry at least one does (printed: how many)."""
    ctx = world["ctx"]
    run = entries(world)[name]
    ctx.set_lanes(3)
    try:
        want = singles(world, run)
        ctx.set_sequence_bias_tables(world["tables"], world["boosts"], eot=STOP)
        ctx.set_bias_rows(MAP)
        got = fields(run(ctx))
        changed = []
        for b, t in enumerate(MAP):
            # (the greedy entry with the bias off runs without the extended decode: the same tokens and lengths)
            ref = want[t if t in (0, 1, 2) else -1]
            assert rows_equal(got, b, ref, b) is None, (name, b, t, rows_equal(got, b, ref, b))
            if t in (0, 1, 2):
                changed.append(rows_equal(got, b, want[-1], b) is not None)
        # the tables act: at temperature 0 a row cannot keep the plain decode's tokens -- they hold an n-gram its table bans
        if name in ("greedy", "transcribe T=0"):
            assert all(rows_equal(got, b, want[-1], b, ["tokens"]) == "tokens" for b, t in enumerate(MAP) if t in (0, 1, 2))
        assert any(changed), name
        print("%s: %d of %d rows with a table differ from the bias-off call" % (name, sum(changed), len(changed)))
    finally:
        ctx.set_lanes(0)
        ctx.set_sequence_bias(None)


def test_row_alone_lanes_and_a_call_of_130_rows(world):
    """A row decoded alone under its table equals the row among others; one lane equals three; and a call of 130 rows -- more
    than one decode group can hold, with a map that follows no group boundary -- gives every row what the 9-row single-table
    calls gave its recording under its table (temperature 0: a row does not depend on its place in the call)."""
    ctx, pcm, m = world["ctx"], world["pcm"], world["mel_args"]
    run = lambda c: c.transcribe_mel(*m, PROMPT, NEW, eot=STOP)       # noqa: E731
    try:
        ctx.set_lanes(3)
        want = singles(world, run)
        ctx.set_sequence_bias_tables(world["tables"], world["boosts"], eot=STOP)
        ctx.set_bias_rows(MAP)
        got = fields(run(ctx))
        for b in (0, 3, 6, 7):
            ctx.set_bias_rows([MAP[b]])
            one = fields(ctx.transcribe_mel(m[0], m[1][b:b + 1], *m[2:], PROMPT, NEW, eot=STOP))
            assert rows_equal(one, 0, got, b) is None, b
        res = []
        for lanes in (1, 3):
            ctx.set_lanes(lanes)
            ctx.set_bias_rows(MAP)
            res.append(fields(ctx.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=0.8, seed=9)))
        assert all(same(res[0][k], res[1][k]) for k in res[0])
        ctx.set_lanes(0)
        B = 130
        src = [b % R for b in range(B)]                               # the 9 mel windows over and over: no copy, their offsets
        big_map = [(b // R * 2 + b) % 5 - 1 for b in range(B)]        # -1 .. 3; a recording meets every table
        assert {(s, t) for s, t in zip(src, big_map)} == {(s, t) for s in range(R) for t in range(-1, 4)} and B > 128
        ctx.set_bias_rows(big_map)
        big = fields(ctx.transcribe_mel(m[0], m[1][src], *m[2:], PROMPT, NEW, eot=STOP))
        for b in range(B):
            ref = want[big_map[b] if big_map[b] in (0, 1, 2) else -1]
            assert rows_equal(big, b, ref, src[b]) is None, (b, src[b], big_map[b])
    finally:
        ctx.set_lanes(0)
        ctx.set_sequence_bias(None)


def test_maps_and_table_sets_replay_the_same_graphs(world):
    """Two maps and two table sets in turn on ONE context -- the later calls replay the graphs the first captured: the pool and
    the rows' ranges live in device memory -- each equal a fresh context's result, and a clone's made behind the set."""
    ctx, pcm = world["ctx"], world["pcm"]
    A = (world["tables"], world["boosts"])
    Bset = ([world["tables"][2], world["tables"][0], {}, world["tables"][1]], [world["boosts"][2], [], [], []])
    map2 = [3, 3, 0, 1, -1, 2, 2, 0, 1]
    plan = [(A, MAP), (A, map2), (Bset, MAP), (Bset, map2)]
    try:
        ctx.set_lanes(3)
        got = []
        for (tables, boosts), rows in plan:
            ctx.set_sequence_bias_tables(tables, boosts, eot=STOP)
            ctx.set_bias_rows(rows)
            got.append(fields(ctx.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=0.8, seed=4)))
        assert not same(got[0]["tokens"], got[1]["tokens"]) and not same(got[0]["tokens"], got[2]["tokens"])
        for ((tables, boosts), rows), g in zip(plan, got):
            c = fresh(world)
            try:
                c.set_lanes(3)
                c.set_sequence_bias_tables(tables, boosts, eot=STOP)
                c.set_bias_rows(rows)
                f = fields(c.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=0.8, seed=4))
                assert all(same(f[k], g[k]) for k in g)
                k = c.clone()
                try:
                    k.set_lanes(3)
                    k.set_bias_rows(rows)
                    f = fields(k.transcribe(pcm, PROMPT, NEW, eot=STOP, temperature=0.8, seed=4))
                    assert all(same(f[x], g[x]) for x in g)
                finally:
                    k.close()
            finally:
                c.close()
    finally:
        ctx.set_lanes(0)
        ctx.set_sequence_bias(None)


def status_of(b, fn):
    with pytest.raises(b.WhisperError) as e:
        fn()
    return e.value.status


def test_refusals_exclusivity_and_what_stays_in_force(world):
    """Every refusal with its status; a refused set call leaves what was in force; the exclusivity with wm_set_sequence_bias."""
    ctx, b, pcm, m = world["ctx"], world["b"], world["pcm"], world["mel_args"]
    V = world["dims"]["n_vocab"]
    tables, boosts = world["tables"], world["boosts"]
    greedy = lambda c=ctx: c.transcribe_greedy(pcm, PROMPT, 12, eot=STOP)     # noqa: E731
    try:
        plain = greedy()
        # no tables: a map has nothing to index
        assert status_of(b, lambda: ctx.set_bias_rows(MAP)) == WM_ERR_STATE
        ctx.set_bias_rows([])
        ctx.set_sequence_bias_tables(tables, boosts, eot=STOP)
        assert status_of(b, greedy) == WM_ERR_STATE                               # tables in force, no map
        ctx.set_bias_rows(MAP)
        want = greedy()
        assert not same(want[0], plain[0])
        assert status_of(b, greedy) == WM_ERR_STATE                               # the map was consumed
        ctx.set_bias_rows(MAP[:8])
        assert status_of(b, greedy) == WM_ERR_INVALID                             # n != B ...
        assert status_of(b, greedy) == WM_ERR_STATE                               # ... and that call consumed it too
        assert status_of(b, lambda: ctx.set_bias_rows([0] * 8 + [4])) == WM_ERR_INVALID   # outside [-1, n_tables)
        assert status_of(b, lambda: ctx.set_bias_rows([0] * 8 + [-2])) == WM_ERR_INVALID
        ctx.set_bias_rows(MAP)
        ctx.set_bias_rows([])                                                     # n = 0 drops a pending map
        assert status_of(b, greedy) == WM_ERR_STATE
        # refused table sets: what wm_set_sequence_bias refuses, in any table; the limits; each leaves the tables in force
        singles_ = {(i,): 0.5 for i in range(900)}
        for bad in ([{(V,): 1.0}], [tables[0], {(1, STOP): 1.0}], [{(1,): float("nan")}, tables[1]], [{}, {(1, 2): -INF}],
                    [{(1,): 1.0}] * 1025):
            bo = [[(1, 2)] if t == {(1, 2): -INF} else [] for t in bad]
            assert status_of(b, lambda: ctx.set_sequence_bias_tables(bad, bo, eot=STOP)) == WM_ERR_INVALID, len(bad)
        assert status_of(b, lambda: ctx.set_sequence_bias_tables([singles_] * 73, eot=STOP)) == WM_ERR_INVALID     # 65700 entries
        assert status_of(b, lambda: ctx.set_sequence_bias_tables(tables, boosts, eot=V + 1)) == WM_ERR_INVALID
        assert status_of(b, lambda: ctx.set_sequence_bias({(1, STOP): 1.0}, eot=STOP)) == WM_ERR_INVALID
        ctx.set_bias_rows(MAP)
        again = greedy()
        assert same(again[0], want[0]) and same(again[1], want[1])
        # the speculative entry answers WM_ERR_STATE, as for the single table
        draft = fresh(world)
        try:
            ctx.set_bias_rows(MAP)
            assert status_of(b, lambda: ctx.transcribe_mel_speculative(draft, *m, PROMPT, 8, 3, eot=STOP)) == WM_ERR_STATE
            assert status_of(b, greedy) == WM_ERR_STATE                           # (it consumed the map)
        finally:
            draft.close()
        # exclusivity: the single table replaces the tables (no map needed, its own result) ...
        ctx.set_sequence_bias(tables[0], eot=STOP)
        one = greedy()
        assert status_of(b, lambda: ctx.set_bias_rows(MAP)) == WM_ERR_STATE
        c = fresh(world)
        try:
            c.set_sequence_bias(tables[0], eot=STOP)
            ref = greedy(c)
            assert same(one[0], ref[0]) and same(one[1], ref[1]) and not same(one[0], want[0])
        finally:
            c.close()
        # ... the tables replace the single table ...
        ctx.set_sequence_bias_tables(tables, boosts, eot=STOP)
        assert status_of(b, greedy) == WM_ERR_STATE
        ctx.set_bias_rows([-1] * R)
        off = greedy()
        assert same(off[0], plain[0]) and same(off[1], plain[1])                  # nobody has a table: table 0 is not in force
        # ... n_tables = 0 clears the tables and a pending map, and leaves a single table alone
        ctx.set_bias_rows(MAP)
        ctx.set_sequence_bias_tables(None)
        assert same(greedy()[0], plain[0])
        ctx.set_sequence_bias(tables[0], eot=STOP)
        ctx.set_sequence_bias_tables([])
        assert same(greedy()[0], one[0])
        # ... and wm_set_sequence_bias with n_seq = 0 clears both
        ctx.set_sequence_bias_tables(tables, boosts, eot=STOP)
        ctx.set_sequence_bias(None)
        assert same(greedy()[0], plain[0])
    finally:
        ctx.set_sequence_bias(None)
    dbg = b.Context(world["dims"], debug=True)
    try:
        dbg.load_state_dict(world["sd_np"])
        dbg.finalize()
        dbg.set_sequence_bias_tables(tables, boosts, eot=STOP)
        dbg.set_bias_rows(MAP[:1])
        dbg.set_precision(True)
        assert status_of(b, lambda: dbg.transcribe_greedy(pcm[:1], PROMPT, 4, eot=STOP)) == WM_ERR_STATE
        assert status_of(b, lambda: dbg.set_sequence_bias_tables(tables, boosts, eot=STOP)) == WM_ERR_STATE
        dbg.set_sequence_bias_tables(None)                                        # switching them off is always allowed
        dbg.set_precision(False)
        dbg.set_sequence_bias_tables(tables, boosts, eot=STOP)
        dbg.set_bias_rows([0])
        r = dbg.transcribe_greedy(pcm[:1], PROMPT, NEW, eot=STOP)
        assert not any(SB.contains(r[0][0][:r[1][0]], s) for s, v in tables[0].items() if v == -INF)
    finally:
        dbg.close()


def test_the_multi_device_entry_refuses_row_tables(pkg):
    """wm_multi_transcribe_greedy with tables on a device context answers WM_ERR_STATE (a row map per device's slice of the call
    is not built) before anything runs; with the tables cleared the same call gives what it gave before."""
    from oracle import whisper_ref as R_
    b = pkg.binding
    mc = b.MultiContext(dict(R_.TINY_DIMS), devices=[0])
    try:
        mc.init_synthetic(11)
        pcm, prompt = tones(2), [10, 21, 5, 7]
        want = mc.transcribe_greedy(pcm, prompt, 6)
        one = mc.device_ctx(0)
        one.set_sequence_bias_tables([{(1, 2): -INF}, {}])
        assert status_of(b, lambda: mc.transcribe_greedy(pcm, prompt, 6)) == WM_ERR_STATE
        one.set_bias_rows([0, 1])                                                  # a pending map does not change the answer
        assert status_of(b, lambda: mc.transcribe_greedy(pcm, prompt, 6)) == WM_ERR_STATE
        one.set_sequence_bias_tables(None)
        got = mc.transcribe_greedy(pcm, prompt, 6)
        assert same(got[0], want[0]) and same(got[1], want[1])
    finally:
        mc.close()


def test_transcribe_long_recording_bias_on_the_library(prod):
    """binding.transcribe_long(recording_bias=) against the real library (the CPU file checks its call log on a fake that refuses
    nothing): every recording of the batched run equals the run of that recording ALONE with its table as the global one
    (sequence_bias / bad_words of 17.); a recording on None equals the plain run's; and entries that give no table at all --
    all None, all empty dicts -- make the plain run (a row map on a context without tables would be WM_ERR_STATE)."""
    ctx = prod
    try:
        recs = _long_recs()
        recs = [recs[0], recs[1][:20 * 16000], recs[2][:35 * 16000]]
        ids, kw = [7, 300, 65535], _kw(no_speech_threshold=None)          # (no window is skipped as silence)
        plain = ctx.transcribe_long(recs, recording_ids=ids, **kw)

        def text(o):
            """the distinct text tokens of the recording's plain decode, in order of appearance"""
            t = [int(x) for w in o["windows"] for x in w["tokens"] if x < EOT2]
            print("plain decode: %d windows, text tokens %s" % (len(o["windows"]), t[:12]))
            assert len(set(t)) >= 2
            return list(dict.fromkeys(t))
        # a table that bans a token the plain decode holds changes that recording for certain
        t0, t2 = text(plain[0]), text(plain[2])
        bias = [dict(bad_words=[[t0[0]], [t0[1], t0[0]]]), None, dict(sequence_bias={(t2[0],): -INF, (t2[0], t2[1]): 1.5})]
        got = ctx.transcribe_long(recs, recording_ids=ids, recording_bias=bias, **kw)
        for r in range(3):
            alone = ctx.transcribe_long([recs[r]], recording_ids=[ids[r]], **dict(kw, **(bias[r] or {})))[0]
            assert _strip(alone) == _strip(got[r]), r
        assert _strip(got[1]) == _strip(plain[1]) and _strip(got[0]) != _strip(plain[0]) and _strip(got[2]) != _strip(plain[2])
        for none in ([None] * 3, [{}] * 3, [None, dict(phrase_boost=2.0), {}]):
            assert ctx.transcribe_long(recs, recording_ids=ids, recording_bias=none, **kw) == plain
    finally:
        ctx.set_sequence_bias(None)
