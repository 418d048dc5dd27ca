"""GPU tests of decode-pass word timestamps for best-of and beam-search hypotheses: wm_transcribe_{mel,windows}_{best_of,beam}_aligned
(every candidate / beam of a window keeps its alignment-head queries, the search records its ancestry, and each group ends by
gathering the chosen hypothesis' queries and running the alignment kernels and the DTW over them) and
transcribe_long(word_timestamps="decode_best") on top.  Yardsticks: the EXISTING plain best-of / beam calls for every decode
output (bit for bit), wm_transcribe_mel_aligned for one row per window, the traced beam sums (wmdbg_beam_trace) for the slot
tables, tests/test_align_gpu.py's fp32 oracle forward with the numpy post-processing of tests/test_align_cpu.py for the cost
matrix, numpy's DTW on the GPU's own matrix for the start frames."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import whisper_ref as R
from test_align_cpu import start_frames
from test_align_gpu import GATE_TINY, dbg, default_heads, oracle_forward  # noqa: F401  (dbg: module fixture)
from test_beam_gpu import LIST, _all, _f32_sum, mel10  # noqa: F401  (mel10: module fixture)
from test_decode_align_gpu import NEW, NO_TS, NS_TOK, SOT_SEQ, _Logged, _aligned, _bits, _ragged_prompts, _window_xa, decode_matrix, mel3  # noqa: F401
from test_longform_gpu import EOT2, NS, SOT, TSB, _kw, _long_recs, prod  # noqa: F401  (prod: fixture)
from test_longform_words_gpu import prod_vocab  # noqa: F401  (fixture)
from test_model_gpu import lively  # noqa: F401  (lively: module fixture)
from test_transcribe_options_gpu import EOT, PROMPT, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
f32 = np.float32
MEASURED = {}
IDS3 = np.array([(3 << 16) | 17, 5, 70000], dtype=np.uint32)


@pytest.fixture(scope="module", autouse=True)
def _write_measured():
    yield
    out = os.environ.get("WM_MEASURED_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "hyp_align_measured.json"), "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(v))


@pytest.fixture(scope="module")
def ctx(dbg):
    c = dbg[2]
    c.lib.wmdbg_beam_trace.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    c.lib.wmdbg_hyp_slots.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    c.lib.wmdbg_align_hyp.argtypes = [ctypes.c_void_p, ctypes.c_int]
    c.lib.wmdbg_align_gather.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return c


def _base(n, mod=3):
    return (np.arange(n, dtype=np.int64) % mod) * 240000


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _best_of(ctx, aligned, mel, base, prompts, N, n_frames=3000, T=0.7, seed=77, ids=None, new=NEW, eot=EOT, **kw):
    fn = ctx.transcribe_mel_best_of_aligned if aligned else ctx.transcribe_mel_best_of
    return fn(mel, base, 3000, 0, n_frames, prompts, new, N, eot=eot, temperature=T, seed=seed, no_speech_token=NS_TOK, sample_ids=ids,
              **kw)


def _beam(ctx, aligned, mel, base, prompts, N, cand, n_frames=3000, new=NEW, eot=EOT, ns=True, **kw):
    fn = ctx.transcribe_mel_beam_aligned if aligned else ctx.transcribe_mel_beam
    return fn(mel, base, 3000, 0, n_frames, prompts, new, N, eot=eot, max_candidates=cand, no_speech_token=NS_TOK if ns else -1, **kw)


def _all_best_of(r):
    return [r.tokens, r.lens, _bits(r.logprobs), _bits(r.no_speech_prob), r.best]


def _all_beam(r):
    return [x if x is None or x.dtype != np.float32 else _bits(x) for x in _all(r)]


def _same_outputs(got, want, fields, what, rows_g=slice(None), rows_w=slice(None)):
    for k, (x, y) in enumerate(zip(fields(got), fields(want))):
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            assert np.array_equal(x[rows_g], y[rows_w]), (what, k)


def _path_ok(r, sel, M=1500):
    """the start frames of every window are a monotone path over the chosen hypothesis' tokens that ends at M"""
    for b in range(len(sel.lens)):
        n, sf = int(sel.lens[b]), r.start_frames[b]
        assert n >= 1 and sf[n] == M and np.all(sf[n + 1:] == -1) and np.all(np.diff(sf[:n + 1]) >= 0) and sf[0] >= 0, (b, sf)


# ---------------------------------------------------------------- 1. the decode outputs are the plain call's bits
FAMILIES = {"best_of3": ("best_of", 3, None), "beam1": ("beam", 1, 1), "beam2": ("beam", 2, 5), "beam5": ("beam", 5, 8)}
CASES_1 = {"uniform": dict(), "ragged-budgets": dict(ragged=True, budgets=[1, 7, 24]), "rules": dict(rules=True)}


def _family_call(ctx, family, aligned, mel, base, prompts, **kw):
    kind, N, cand = FAMILIES[family]
    if kind == "best_of":
        return _best_of(ctx, aligned, mel, base, prompts, N, ids=IDS3[:len(base)], **kw), _all_best_of
    return _beam(ctx, aligned, mel, base, prompts, N, cand, **kw), _all_beam


@pytest.mark.parametrize("case", sorted(CASES_1))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_decode_outputs_are_the_plain_counterpart_s_bits(ctx, mel3, family, case):
    c = dict(CASES_1[case])
    ragged, rules = c.pop("ragged", False), c.pop("rules", False)
    prompts = _ragged_prompts() if ragged else np.array([SOT_SEQ] * 3, dtype=np.int32)
    if ragged:
        c["sot_tail"] = 3
    if rules:   # timestamp rules + suppress lists + no_repeat_ngram_size 3 + one banned sequence
        _rules(ctx)
        ctx.set_repetition_rules(1.0, 3, EOT)
        first = _aligned(ctx, mel3, _base(3), prompts)
        t0 = [int(t) for t in first.tokens[0, :first.lens[0]]]
        i = next(k for k in range(1, len(t0)) if t0[k] < EOT)
        ctx.set_sequence_bias({(t0[i - 1], t0[i]): float("-inf")}, eot=EOT)
    try:
        want, fields = _family_call(ctx, family, False, mel3, _base(3), prompts, **c)
        got, _ = _family_call(ctx, family, True, mel3, _base(3), prompts, **c)
        _same_outputs(got, want, fields, (family, case))
        _path_ok(got, got.selected)
        if ragged:
            assert int(got.selected.lens[0]) == 1 and 1 <= int(got.selected.lens[1]) <= 7
        if rules:
            assert (want.tokens >= 900).any()     # timestamps occur
        if case == "uniform":     # window set = mel
            with ctx.encode_windows(mel3, _base(3), 3000, 0, 3000) as ws:
                kind, N, cand = FAMILIES[family]
                if kind == "best_of":
                    a = (ws, None, prompts, NEW, N)
                    kw = dict(eot=EOT, temperature=0.7, seed=77, no_speech_token=NS_TOK, sample_ids=IDS3)
                    plain, from_set = ctx.transcribe_windows_best_of(*a, **kw), ctx.transcribe_windows_best_of_aligned(*a, **kw)
                else:
                    a = (ws, None, prompts, NEW, N)
                    kw = dict(eot=EOT, max_candidates=cand, no_speech_token=NS_TOK)
                    plain, from_set = ctx.transcribe_windows_beam(*a, **kw), ctx.transcribe_windows_beam_aligned(*a, **kw)
            _same_outputs(from_set, plain, fields, (family, "windows vs plain windows"))
            _same_outputs(from_set, got, fields, (family, "windows vs mel"))
            assert np.array_equal(from_set.start_frames, got.start_frames)
    finally:
        if rules:
            ctx.set_sequence_bias(None)
            ctx.set_repetition_rules(1.0, 0, EOT)
            _rules(ctx, False)


# ---------------------------------------------------------------- 2. one row per window is the plain aligned call
def test_one_row_per_window_is_the_aligned_call_and_candidate_0_is_too(ctx, mel3):
    prompts = _ragged_prompts()
    kw = dict(sot_tail=3, budgets=[24, 7, 24])
    one = _aligned(ctx, mel3, _base(3), prompts, T=0.7, ids=IDS3, **kw)
    got = _best_of(ctx, True, mel3, _base(3), prompts, 1, ids=IDS3, **kw)
    assert np.array_equal(got.start_frames, one.start_frames) and np.all(got.best == 0)
    assert np.array_equal(got.tokens[:, 0], one.tokens) and np.array_equal(_bits(got.logprobs[:, 0]), _bits(one.logprobs))
    greedy = _aligned(ctx, mel3, _base(3), prompts, **kw)
    got = _beam(ctx, True, mel3, _base(3), prompts, 1, 1, **kw)
    assert np.array_equal(got.start_frames, greedy.start_frames) and np.all(got.best == 0)
    assert np.array_equal(got.tokens[:, 0], greedy.tokens) and np.array_equal(_bits(got.logprobs[:, 0]), _bits(greedy.logprobs))
    # candidate 0 of a best-of call is the one-sample call with the same sample ids
    assert ctx.lib.wmdbg_align_hyp(ctx.handle, 0) == 0
    got = _best_of(ctx, True, mel3, _base(3), prompts, 3, ids=IDS3, **kw)
    assert np.array_equal(got.tokens[:, 0], one.tokens) and np.array_equal(got.start_frames, one.start_frames)
    # ... and at temperature 0 the call aligns candidate 0 by itself (the hook was for one call)
    got = _best_of(ctx, True, mel3, _base(3), prompts, 3, T=0.0, ids=IDS3, **kw)
    assert np.all(got.best == 0) and np.array_equal(got.start_frames, greedy.start_frames)


# ---------------------------------------------------------------- 3. the gather kernel alone
@pytest.mark.parametrize("N", [2, 5, 8])
def test_gather_kernel_copies_the_named_slots_and_nothing_else(ctx, N):
    rng = np.random.default_rng(N)
    C, Tq, J = 3, 9, 5     # a row of 5 * 256 B: more than one 16-byte unit per thread of a wave, no multiple of the block
    cap = rng.standard_normal((C * N, Tq, J, 64)).astype(f32)
    tables = {"constant": np.repeat(rng.integers(0, N, size=(C, 1)), Tq, 1), "alternating": (np.arange(C * Tq).reshape(C, Tq) % 2) * (N - 1),
              "random": rng.integers(0, N, size=(C, Tq))}
    for name, slot in tables.items():
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        for rows in ([1, 2, Tq], [Tq, 0, 1], [2, Tq, Tq]):
            n_rows = np.array(rows, dtype=np.int32)
            sel = np.full((C, Tq, J, 64), -7.5, dtype=f32)
            assert ctx.lib.wmdbg_align_gather(ctx.handle, _vp(cap), C, N, Tq, J, _vp(slot), _vp(n_rows), _vp(sel)) == 0
            for c in range(C):
                for t in range(Tq):
                    want = cap[c * N + slot[c, t], t] if t < rows[c] else np.full((J, 64), -7.5, f32)
                    assert np.array_equal(_bits(sel[c, t]), _bits(want)), (name, rows, c, t)
    bad = np.full((C, Tq), N, dtype=np.int32)
    assert ctx.lib.wmdbg_align_gather(ctx.handle, _vp(cap), C, N, Tq, J, _vp(bad), _vp(n_rows), _vp(sel)) == WM_ERR_INVALID


# ---------------------------------------------------------------- 4. the ancestry on a real search
def _traced_aligned(ctx, h, mel, base, prompts, N, cand, new, **kw):
    """the aligned beam call that aligns hypothesis h, with its trace and slot tables: (result, sums [B][new][N], slots [B][Tq])"""
    Bn, Tq = len(base), len(prompts[0]) + new - 1
    tr = np.full((Bn, new, N, 2 + 2 * LIST), np.nan, f32)
    slots = np.full((Bn, Tq), -1, dtype=np.int32)
    assert ctx.lib.wmdbg_beam_trace(ctx.handle, _vp(tr)) == 0
    assert ctx.lib.wmdbg_hyp_slots(ctx.handle, _vp(slots)) == 0
    assert ctx.lib.wmdbg_align_hyp(ctx.handle, h) == 0
    r = _beam(ctx, True, mel, base, prompts, N, cand, new=new, ns=False, **kw)
    return r, tr[..., 1], slots


@pytest.mark.parametrize("rules", [False, True])
def test_slot_tables_name_the_beam_that_carried_the_hypothesis(ctx, mel10, rules):
    """test_beam_gpu.py's fork inputs.  At every generated step the slot the table names held, before the next step, a running
    sum equal to the in-order f32 sum of the hypothesis' own log-prob prefix."""
    _rules(ctx, rules)
    try:
        n, N, new, S = 4, 5, 16, len(PROMPT) - 1
        base = _base(n, 10)
        prompts = np.tile(np.array(PROMPT, np.int32), (n, 1))
        free = _beam(ctx, False, mel10, base, prompts, N, N, new=new, eot=-1, ns=False)
        vals, cnt = np.unique(free.tokens[:, :, 2:], return_counts=True)
        eot = int(vals[np.argmax(cnt)])     # a frequent token plays eot
        steps = skipped = 0
        seen = dict(moved_twice=0, finished=0, live=0)
        for e, cand, kw in ((-1, N, {}), (eot, 8, dict(budgets=[16, 7, 12, 3], length_penalty=0.6))):
            plain = _beam(ctx, False, mel10, base, prompts, N, cand, new=new, eot=e, ns=False, **kw)
            for h in range(max(N, cand)):
                r, sums, slots = _traced_aligned(ctx, h, mel10, base, prompts, N, cand, new, eot=e, **kw)
                _same_outputs(r, plain, _all_beam, ("traced aligned vs plain", h))
                for w in range(n):
                    hh = min(h, int(r.n_hyp[w]) - 1)
                    ln = int(r.lens[w, hh])
                    lp = r.logprobs[w, hh]
                    sl = slots[w]
                    assert ((sl >= 0) & (sl < N)).all() and (sl[:S + 1] == sl[0]).all()
                    sf = r.start_frames[w]
                    assert sf[ln] == 1500 and np.all(sf[ln + 1:] == -1) and np.all(np.diff(sf[:ln + 1]) >= 0)
                    finished = e >= 0 and r.tokens[w, hh, ln - 1] == e
                    seen["finished" if finished else "live"] += 1
                    seen["moved_twice"] += int(np.count_nonzero(np.diff(sl[S + 1:S + ln])) >= 2)
                    for g in range(ln - 1):     # capture row S + 1 + g: the step that is fed token g
                        steps += 1
                        before_next = sums[w, g + 1]
                        live = before_next[before_next != -np.inf]
                        if len(set(live.view(np.uint32).tolist())) < len(live):
                            skipped += 1     # two live beams carry one sum: the step proves nothing
                            continue
                        want = _f32_sum(lp[:g + 1])
                        assert f32(before_next[sl[S + 1 + g]]).tobytes() == f32(want).tobytes(), (rules, e, h, w, g)
        print("slot tables: %d steps, %d skipped for equal sums; %s" % (steps, skipped, seen))
        assert steps > 0 and skipped <= 0.05 * steps
        assert seen["moved_twice"] >= 1 and seen["finished"] >= 1 and seen["live"] >= 1, seen
    finally:
        _rules(ctx, False)


# ---------------------------------------------------------------- 5. the cost matrix of the chosen hypothesis against the oracle
def _check_matrix(ctx, sd, dims, mel, r, prompts, key):
    """Per window: rel-L2 of the captured matrix against the fp32 oracle forward over the chosen hypothesis' own rows (gate
    GATE_TINY), its extent, and numpy's DTW on the GPU's matrix."""
    heads = default_heads(dims)
    sel = r.selected
    for b in range(len(prompts)):
        n, M = int(sel.lens[b]), 1500
        sf, mat = r.start_frames[b], r.matrix[b]
        assert n >= 2, (key, b)
        seq = [int(t) for t in prompts[b]] + [int(t) for t in sel.tokens[b, :n - 1]]     # the last generated token is never fed
        _, qk = oracle_forward(sd, dims, seq, _window_xa(ctx, mel[b], 3000))
        want = decode_matrix(np.stack([qk[l, h] for l, h in heads]), 3000, 7, 1.0, n)
        got = mat[:n, :M]
        assert np.all(mat[n:] == 0), (key, b)
        e = R.rel_l2(got, want)
        _note(key, e)
        print("hypothesis alignment %s window %d (hypothesis %d, len %d): rel-L2 %.5f (gate %.3f)" % (key, b, r.best[b], n, e, GATE_TINY))
        assert e <= GATE_TINY, (key, b, e)
        assert sf[:n].tolist() == start_frames(got).tolist(), (key, b)     # exact, on the GPU's own matrix
        assert sf[n] == M and np.all(sf[n + 1:] == -1), (key, b)
        _note(key + "_frame_median", np.median(np.abs(start_frames(want) - sf[:n])))


def test_cost_matrix_of_the_chosen_beam_hypothesis_against_the_oracle(dbg, ctx, mel3):
    """Measured on an MI355X: see DESIGN.md section 17."""
    dims, sd, _ = dbg
    prompts = np.array([SOT_SEQ + [NO_TS]] * 3, dtype=np.int32)
    r = _beam(ctx, True, mel3, _base(3), prompts, 5, 5, eot=-1, capture_matrix=True)
    _check_matrix(ctx, sd, dims, mel3, r, prompts, "beam5")


def test_cost_matrix_of_a_chosen_candidate_that_is_not_candidate_0_against_the_oracle(dbg, ctx, mel3):
    dims, sd, _ = dbg
    prompts = np.array([SOT_SEQ + [NO_TS]] * 3, dtype=np.int32)
    for seed in (77, 78, 79, 80, 81, 82):     # the first seed whose ranking prefers another candidate somewhere
        r = _best_of(ctx, True, mel3, _base(3), prompts, 3, seed=seed, ids=IDS3, eot=-1, capture_matrix=True)
        if (r.best != 0).any():
            break
    assert (r.best != 0).any(), r.best
    _check_matrix(ctx, sd, dims, mel3, r, prompts, "best_of3")


# ---------------------------------------------------------------- 6. invariance and robustness
@pytest.mark.parametrize("family", ["best_of", "beam"])
def test_a_window_depends_on_itself_only(ctx, mel10, family):
    prompts17 = _ragged_prompts(lens=[3, 5, 9, 4, 3, 7, 12, 3, 6, 5, 3, 8, 4, 3, 9, 5, 3], seed=9)
    ids17 = (np.arange(17, dtype=np.uint32) * 65537 + 11).astype(np.uint32)

    def call(rows, **kw):
        p, base = [prompts17[i] for i in rows], _base(17, 10)[list(rows)]
        if family == "best_of":
            return _best_of(ctx, True, mel10, base, p, 3, ids=ids17[list(rows)], sot_tail=3, **kw)
        return _beam(ctx, True, mel10, base, p, 3, 3, sot_tail=3, **kw)

    fields = _all_best_of if family == "best_of" else _all_beam
    ref = call(range(12))
    _path_ok(ref, ref.selected)
    for w in (0, 5, 11):
        alone = call([w])
        _same_outputs(alone, ref, fields, ("alone", w), slice(None), slice(w, w + 1))
        assert np.array_equal(alone.start_frames[0], ref.start_frames[w]), w
    try:
        for lanes in (1, 3):     # 17 windows x 3 rows
            ctx.set_lanes(lanes)
            many = call(range(17))
            _same_outputs(many, ref, fields, ("17 windows", lanes), slice(0, 12))
            assert np.array_equal(many.start_frames[:12], ref.start_frames), lanes
    finally:
        ctx.set_lanes(0)


@pytest.mark.parametrize("family", ["best_of", "beam"])
def test_degenerate_windows(ctx, mel3, family):
    prompts = np.array([SOT_SEQ] * 3, dtype=np.int32)

    def call(**kw):
        if family == "best_of":
            return _best_of(ctx, True, mel3, _base(3), prompts, 3, ids=IDS3, **kw)
        return _beam(ctx, True, mel3, _base(3), prompts, 2, 5, **kw)

    r = call(budgets=[1, 24, 3])
    s = r.selected
    assert int(s.lens[0]) == 1 and r.start_frames[0, 0] >= 0 and r.start_frames[0, 1] == 1500 and np.all(r.start_frames[0, 2:] == -1)
    assert 1 <= int(s.lens[2]) <= 3 and r.start_frames[2, int(s.lens[2])] == 1500
    # one generated token behind a prompt that ENDS in <|startoftranscript|>: one decoder row, nothing to z-score against
    r = call(n_frames=[3000, 1234, 3000], sot_index=2, budgets=[1, 1, 2])
    for k, M in ((0, 1500), (1, 617)):
        assert int(r.selected.lens[k]) == 1 and r.start_frames[k].tolist() == [0, M] + [-1] * (NEW - 1), k
    n2 = int(r.selected.lens[2])
    assert r.start_frames[2, n2] == 1500 and np.all(r.start_frames[2, :n2] >= 0)
    # a window of one frame decodes normally and has no audio frame to align to
    r = call(n_frames=[1, 3000, 1])
    assert int(r.selected.lens[0]) >= 1 and np.all(r.start_frames[0] == -1) and np.all(r.start_frames[2] == -1)
    assert r.start_frames[1, int(r.selected.lens[1])] == 1500


def test_invalid_arguments_and_the_context_still_works(ctx, pkg, mel3):
    b = pkg.binding
    prompts = np.array([SOT_SEQ] * 3, dtype=np.int32)
    ragged = _ragged_prompts()
    good_c = _best_of(ctx, True, mel3, _base(3), prompts, 3, ids=IDS3)
    good_b = _beam(ctx, True, mel3, _base(3), prompts, 2, 5)
    bad = [dict(medfilt_width=6), dict(medfilt_width=0), dict(medfilt_width=33), dict(qk_scale=float("nan")), dict(qk_scale=float("inf")),
           dict(prompts=ragged, sot_tail=0), dict(prompts=ragged, sot_tail=4), dict(new=0), dict(new=446),
           dict(prompts=np.array([[10, 21, 1024]] * 3)), dict(n_frames=3001), dict(sot_index=3), dict(budgets=[1, 2]),
           dict(length_penalty=1.5)]
    for kw in bad:
        for call in (lambda p, **k: _best_of(ctx, True, mel3, _base(3), p, 3, ids=IDS3, **k),
                     lambda p, **k: _beam(ctx, True, mel3, _base(3), p, 2, 5, **k)):
            a = dict(prompts=prompts)
            a.update(kw)
            with pytest.raises(b.WhisperError) as e:
                call(a.pop("prompts"), **a)
            assert e.value.status == WM_ERR_INVALID and str(e.value), kw
    for kw, call in ((dict(T=-1.0), _best_of), (dict(), _best_of), (dict(), _beam)):     # the counts of the families' own
        for n in (0, 9):
            with pytest.raises(b.WhisperError) as e:
                if call is _best_of:
                    _best_of(ctx, True, mel3, _base(3), prompts, 3 if kw else n, ids=IDS3, **kw)
                else:
                    _beam(ctx, True, mel3, _base(3), prompts, n, 5)
            assert e.value.status == WM_ERR_INVALID
    with pytest.raises(b.WhisperError) as e:
        _beam(ctx, True, mel3, _base(3), prompts, 2, 17)
    assert e.value.status == WM_ERR_INVALID
    # null best_out and null start_frame_out, through the raw symbols
    base, full, zero = _base(3), np.full(3, 3000, np.int32), np.zeros(3, np.int32)
    toks, lens, lp = np.zeros((3, 3, NEW), np.int32), np.zeros((3, 3), np.int32), np.zeros((3, 3, NEW), f32)
    best, start = np.zeros(3, np.int32), np.zeros((3, NEW + 1), np.int32)
    opts = b.wm_decode_opts(0.7, 77, NS_TOK, 0)
    head = [b._ptr(mel3), b._ptr(base), b._ptr(full), b._ptr(zero), b._ptr(full), 3, b._ptr(prompts), 3, None, 0]
    args = head + [b._ptr(IDS3), 3, float("nan"), NEW, EOT, ctypes.byref(opts), 7, 1.0, b._ptr(toks), b._ptr(lens), b._ptr(lp), None,
                   b._ptr(best), b._ptr(start), b.WM_MEM_HOST]
    assert ctx.lib.wm_transcribe_mel_best_of_aligned(ctx.handle, *args) == 0
    assert np.array_equal(toks, good_c.tokens) and np.array_equal(start, good_c.start_frames) and np.array_equal(best, good_c.best)
    for i, word in ((22, b"best_out"), (23, b"start_frame_out")):
        null = list(args)
        null[i] = None
        assert ctx.lib.wm_transcribe_mel_best_of_aligned(ctx.handle, *null) == WM_ERR_INVALID and word in ctx.lib.wm_last_error()
    S = 5
    toks, lens, lp = np.zeros((3, S, NEW), np.int32), np.zeros((3, S), np.int32), np.zeros((3, S, NEW), f32)
    n_hyp, sums = np.zeros(3, np.int32), np.zeros((3, S), f32)
    opts = b.wm_decode_opts(0.0, 0, NS_TOK, 0)
    args = head + [2, 5, float("nan"), NEW, EOT, ctypes.byref(opts), 7, 1.0, b._ptr(toks), b._ptr(lens), b._ptr(n_hyp), b._ptr(sums),
                   b._ptr(lp), None, b._ptr(best), b._ptr(start), b.WM_MEM_HOST]
    assert ctx.lib.wm_transcribe_mel_beam_aligned(ctx.handle, *args) == 0
    assert np.array_equal(toks, good_b.tokens) and np.array_equal(start, good_b.start_frames) and np.array_equal(best, good_b.best)
    for i, word in ((24, b"best_out"), (25, b"start_frame_out")):
        null = list(args)
        null[i] = None
        assert ctx.lib.wm_transcribe_mel_beam_aligned(ctx.handle, *null) == WM_ERR_INVALID and word in ctx.lib.wm_last_error()
    # the all-f32 debug precision path
    ctx.set_precision(True)
    try:
        for call in (lambda: _best_of(ctx, True, mel3, _base(3), prompts, 3, ids=IDS3), lambda: _beam(ctx, True, mel3, _base(3), prompts, 2, 5)):
            with pytest.raises(b.WhisperError) as e:
                call()
            assert e.value.status == WM_ERR_STATE
    finally:
        ctx.set_precision(False)
    again = _beam(ctx, True, mel3, _base(3), prompts, 2, 5)
    _same_outputs(again, good_b, _all_beam, "after the errors")
    assert np.array_equal(again.start_frames, good_b.start_frames)
    again = _best_of(ctx, True, mel3, _base(3), prompts, 3, ids=IDS3)
    assert np.array_equal(again.start_frames, good_c.start_frames) and np.array_equal(again.tokens, good_c.tokens)


# ---------------------------------------------------------------- 7. transcribe_long(word_timestamps="decode_best")
def test_transcribe_long_words_from_the_beam_search(prod, pkg, prod_vocab):
    B = pkg.binding
    recs = _long_recs()[:2]
    kw = _kw(vocab=prod_vocab, word_timestamps="decode_best", beam_size=2, temperatures=(0.0,))
    log = _Logged(prod)
    got = B.transcribe_long(log, recs, recording_ids=[7, 300], **kw)
    assert not [n for n in log.names if n.startswith("align")], log.names
    assert "transcribe_mel_beam_aligned" in log.names and "transcribe_mel" not in log.names and "transcribe_mel_aligned" not in log.names
    # the first window of a recording is that of the run without words (later ones start where the last word ended)
    plain = B.transcribe_long(prod, recs, recording_ids=[7, 300], **_kw(beam_size=2, temperatures=(0.0,)))
    for o, p in zip(got, plain):
        assert o["windows"][0]["tokens"] == p["windows"][0]["tokens"] and o["windows"][0]["hypothesis"] == p["windows"][0]["hypothesis"]
    log2 = _Logged(prod)
    again = B.transcribe_long(log2, recs, recording_ids=[7, 300], reuse_encoder=True, **kw)
    assert again == got
    assert not [n for n in log2.names if n.startswith("align")] and "transcribe_windows_beam_aligned" in log2.names
    n_words = 0
    for o, x in zip(got, recs):
        mel = prod.logmel_long([x])[0]
        lang = B.Whisper.LANGUAGES[o["language"] - SOT - 1]
        last_speech = 0.0
        for w in o["windows"]:
            seek, size = w["seek"], w["segment_size"]
            mine = [s for s in o["segments"] if s["seek"] == seek]
            if w["skipped"]:
                assert mine == []
                continue
            res = prod.transcribe_mel_beam_aligned(mel, [0], mel.shape[1], seek, size, [w["prompt"]], 32, 2, eot=EOT2, no_speech_token=NS)
            r = res.selected
            n = int(r.lens[0])
            assert int(res.best[0]) == w["hypothesis"]
            assert [int(t) for t in r.tokens[0, :n] if t != EOT2] == w["tokens"]
            result = {k: mine[0][k] if mine else 0.0 for k in ("temperature", "avg_logprob", "compression_ratio", "no_speech_prob")}
            segs, _, _ = B.window_segments(w["tokens"], seek, size, TSB, EOT2, result, prod_vocab, cleanup=False)
            text = [t for s in segs for t in s["tokens"] if t < EOT2]
            if text and size >= 2:
                toks, sf, pr = B.decode_alignment_text(r.tokens[0], n, res.start_frames[0], r.logprobs[0], EOT2, n_text=len(text))
                assert toks == text
                B.window_word_timestamps(prod_vocab, segs, sf, pr, seek, EOT2, last_speech, lang)
                ends = [s["words"][-1]["end"] for s in segs if s["words"]]
                if ends:
                    last_speech = ends[-1]
            else:
                for s in segs:
                    s["words"] = []
            B.clear_empty_segments(segs, EOT2, prod_vocab, words=True)
            assert len(mine) == len(segs)
            for s, m in zip(segs, mine):
                n_words += len(s["words"])
                assert (m["start"], m["end"], m["words"], m["tokens"]) == (s["start"], s["end"], s["words"], s["tokens"]), seek
    assert n_words > 0
