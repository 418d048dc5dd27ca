"""GPU tests of ragged prompts: wm_transcribe_mel_ragged (rows of one decode group whose prompts differ in length, right-
aligned inside the group), the self-attention launch with per-row offsets on its own, and condition_on_previous_text in
binding.transcribe_long.  The yardstick of every ragged result is the EXISTING wm_transcribe_mel on that row alone with
the row's own uniform-length prompt; the oracle checks reuse test_model_gpu's helpers and margins."""
import ctypes

import numpy as np
import pytest
import torch

from test_kernels_gpu import P, bf
from test_longform_gpu import SOT, SOT_PREV, TASK, _kw, _long_recs, _strip, prod  # noqa: F401  (prod: fixture)
from test_model_gpu import (_check_policy_choices, _lively_on_device, _perturb_ln_on_device, lively,  # noqa: F401
                            tones)
from test_ragged_prompts_cpu import expected_prompts
from test_transcribe_options_gpu import EOT, MAXI, SPECIALS, TS, _rules

pytestmark = pytest.mark.gpu

WM_ERR_INVALID = 1   # include/whisper_mi355x.h
NS_TOK = 899
NEW = 24
N_CTX = 448
LENS = [3, N_CTX - NEW, 1, 17, 2, 4]   # not sorted; the longest fills the context with NEW


def _prompts(lens, seed=0, vocab=EOT):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(0, vocab, size=n)] for n in lens]


@pytest.fixture(scope="module")
def mel10(lively):
    """Ten distinct windows; a call of any size points its rows at them (mel_base repeats)."""
    _, _, _, ctx = lively
    return ctx.logmel(tones(10), out_dtype=np.float32)


def _base(n):
    return (np.arange(n, dtype=np.int64) % 10) * 240000


def _same(a, b, what=""):
    for k, (x, y) in enumerate(zip(a, b)):
        if x is None or y is None:
            assert x is None and y is None, (what, k)
        else:
            assert np.array_equal(x, y), (what, ("tokens", "lens", "logprobs", "no_speech")[k])


def _ragged(ctx, b, mel, base, prompts, T, new=NEW, eot=-1, ids=None, budgets=None, sot_tail=None, seed=77, mem=None):
    opts = b.wm_decode_opts(T, seed, NS_TOK if sot_tail else -1, 0)
    return ctx.transcribe_mel_raw(mel, base, 3000, 0, 3000, prompts, new, eot, opts, sample_ids=ids, logprobs=True,
                                  no_speech=bool(sot_tail), budgets=budgets, sot_tail=sot_tail,
                                  mem=b.WM_MEM_HOST if mem is None else mem)


def _alone(ctx, b, mel, base, prompts, r, T, new=NEW, eot=-1, ids=None, budgets=None, sot_tail=None, seed=77):
    """Row r through wm_transcribe_mel: one row, its own prompt, its own sample id, sot_index counted from the front."""
    opts = b.wm_decode_opts(T, seed, NS_TOK if sot_tail else -1, len(prompts[r]) - sot_tail if sot_tail else 0)
    return ctx.transcribe_mel_raw(mel, base[r:r + 1], 3000, 0, 3000, np.array([prompts[r]], dtype=np.int32), new, eot, opts,
                                  sample_ids=None if ids is None else ids[r:r + 1], logprobs=True, no_speech=bool(sot_tail),
                                  budgets=None if budgets is None else [budgets[r]])


def _check_rows(ctx, b, mel, base, prompts, got, rows, T, **kw):
    for r in rows:
        one = _alone(ctx, b, mel, base, prompts, r, T, **kw)
        _same([None if x is None else x[r:r + 1] for x in got], one, "row %d (prompt of %d)" % (r, len(prompts[r])))


# ---------------------------------------------------------------- 1. equal lengths
@pytest.mark.parametrize("T", [0.0, 0.7])
def test_equal_lengths_are_wm_transcribe_mel(lively, pkg, mel10, T):
    _, _, _, ctx = lively
    b = pkg.binding
    _rules(ctx)
    try:
        n = 6
        base = _base(n)
        for n_prompt, sot_index in ((3, 0), (4, 1)):
            prompts = np.array(_prompts([n_prompt] * n, seed=3), dtype=np.int32)
            opts = b.wm_decode_opts(T, 77, NS_TOK, sot_index)
            want = ctx.transcribe_mel_raw(mel10, base, 3000, 0, 3000, prompts, NEW, EOT, opts, no_speech=True)
            plen = np.full(n, n_prompt, dtype=np.int32)
            opts_r = b.wm_decode_opts(T, 77, NS_TOK, 99)   # sot_index is not read by the ragged call
            got = ctx.transcribe_mel_raw(mel10, base, 3000, 0, 3000, prompts, NEW, EOT, opts_r, no_speech=True,
                                         prompt_len=plen, sot_tail=n_prompt - sot_index)
            _same(got, want, "host mel")
            # a wider stride with the same lengths: the entries past prompt_len are not read
            wide = np.full((n, n_prompt + 5), 1 << 20, dtype=np.int32)
            wide[:, :n_prompt] = prompts
            _same(ctx.transcribe_mel_raw(mel10, base, 3000, 0, 3000, wide, NEW, EOT, opts_r, no_speech=True,
                                         prompt_len=plen, sot_tail=n_prompt - sot_index), want, "wide stride")
            d = ctx.to_device(mel10)
            try:
                got_d = ctx.transcribe_mel_raw(d, base, 3000, 0, 3000, prompts, NEW, EOT, opts_r, no_speech=True,
                                               prompt_len=plen, sot_tail=n_prompt - sot_index, mem=b.WM_MEM_DEVICE)
            finally:
                ctx.dev_free(d)
            _same(got_d, want, "device mel")
    finally:
        _rules(ctx, False)


# ---------------------------------------------------------------- 2. a ragged batch is each row alone
@pytest.mark.parametrize("T", [0.0, 0.9])
@pytest.mark.parametrize("mode", ["fixed", "eot", "budgets"])
def test_a_ragged_batch_is_each_row_alone(lively, pkg, mel10, T, mode):
    _, _, _, ctx = lively
    b = pkg.binding
    _rules(ctx)
    try:
        n = len(LENS)
        base = _base(n)
        prompts = _prompts(LENS, seed=5)
        ids = np.array([(3 << 16) | 17, 5, 1 << 16, 0xFFFF, 9, 70000], dtype=np.uint32)
        kw = dict(ids=ids, sot_tail=1)
        if mode != "fixed":
            kw["eot"] = EOT
        if mode == "budgets":
            kw["budgets"] = [24, 5, 17, 1, 9, 24]
        got = _ragged(ctx, b, mel10, base, prompts, T, **kw)
        _check_rows(ctx, b, mel10, base, prompts, got, range(n), T, **kw)
        if mode == "budgets":
            assert len({int(x) for x in got[1]}) > 1 and all(int(x) <= bud for x, bud in zip(got[1], kw["budgets"]))
        if mode == "fixed":
            # <|startoftranscript|> third from the end, over prompts of at least three tokens
            lens3 = [5, 3, 17, 9]
            p3 = _prompts(lens3, seed=6)
            got3 = _ragged(ctx, b, mel10, base[:4], p3, T, ids=ids[:4], sot_tail=3)
            _check_rows(ctx, b, mel10, base[:4], p3, got3, range(4), T, ids=ids[:4], sot_tail=3)
            # and without the no-speech output
            got0 = _ragged(ctx, b, mel10, base, prompts, T, ids=ids)
            _same(got0[:3], got[:3], "without no_speech")
    finally:
        _rules(ctx, False)


# ---------------------------------------------------------------- 3. every launch shape
def _mixed_lens(n, seed, longest):
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(1, longest, size=n)]
    lens[n // 3] = longest
    return lens


@pytest.mark.parametrize("T", [0.0, 0.9])
def test_ragged_rows_at_17_and_130_rows_and_under_explicit_lanes(lively, pkg, mel10, T):
    _, _, _, ctx = lively
    b = pkg.binding
    _rules(ctx)
    try:
        # 17 rows: two arg-max workgroups, the arrival counter
        lens = _mixed_lens(17, 1, 40)
        prompts = _prompts(lens, seed=7)
        ids = np.arange(17, dtype=np.uint32) * 3 + 1
        got = _ragged(ctx, b, mel10, _base(17), prompts, T, new=12, eot=EOT, ids=ids, sot_tail=1)
        _check_rows(ctx, b, mel10, _base(17), prompts, got, (0, 5, 16, lens.index(40)), T, new=12, eot=EOT, ids=ids, sot_tail=1)
        # 130 rows: two decode groups of 65 whose longest prompts differ (30 in the first, 50 in the second)
        lens = _mixed_lens(65, 2, 30) + _mixed_lens(65, 3, 50)
        prompts = _prompts(lens, seed=8)
        ids = np.arange(130, dtype=np.uint32) + 1000
        got = _ragged(ctx, b, mel10, _base(130), prompts, T, new=10, eot=EOT, ids=ids, sot_tail=1)
        rows = (0, 64, 65, 129, lens.index(30), 65 + lens[65:].index(50))
        _check_rows(ctx, b, mel10, _base(130), prompts, got, rows, T, new=10, eot=EOT, ids=ids, sot_tail=1)
        # explicit lanes: groups of ~8 on 1, 2 and 3 lanes -- the same bits as the library's own grouping
        lens = _mixed_lens(40, 4, 33)
        prompts = _prompts(lens, seed=9)
        ids = np.arange(40, dtype=np.uint32) + 7
        want = _ragged(ctx, b, mel10, _base(40), prompts, T, new=10, eot=EOT, ids=ids, sot_tail=1)
        _check_rows(ctx, b, mel10, _base(40), prompts, want, (0, 9, 39, lens.index(33)), T, new=10, eot=EOT, ids=ids, sot_tail=1)
        try:
            for lanes in (1, 2, 3):
                ctx.set_lanes(lanes)
                _same(_ragged(ctx, b, mel10, _base(40), prompts, T, new=10, eot=EOT, ids=ids, sot_tail=1), want,
                      "set_lanes(%d)" % lanes)
        finally:
            ctx.set_lanes(0)
    finally:
        _rules(ctx, False)


def _synthetic_ctx(pkg, dims, seed):
    ctx = pkg.binding.Context(dims)
    ctx.init_synthetic(seed)
    _perturb_ln_on_device(ctx, dims, seed=seed + 1)
    _lively_on_device(ctx, dims)
    ctx.finalize()
    return ctx


@pytest.mark.parametrize("shape", ["base width, 24 rows: sub-chip parts", "d = 1280, 2 layers"])
def test_ragged_rows_at_base_width_and_at_a_wide_geometry(pkg, shape):
    from oracle import whisper_ref as R
    b = pkg.binding
    if shape.startswith("base"):
        dims = dict(R.TINY_DIMS, n_audio_state=512, n_audio_head=8, n_text_state=512, n_text_head=8)
        n, vocab = 24, 1024
    else:
        dims = dict(b.MODEL_DIMS["large-v2"], n_audio_layer=2, n_text_layer=2)
        n, vocab = 9, 51865
    ctx = _synthetic_ctx(pkg, dims, 31)
    try:
        mel = ctx.logmel(tones(6), out_dtype=np.float32)
        base = (np.arange(n, dtype=np.int64) % 6) * (dims["n_mels"] * 3000)
        lens = _mixed_lens(n, 5, 21)
        prompts = _prompts(lens, seed=10, vocab=vocab - 200)
        ids = np.arange(n, dtype=np.uint32) + 3
        eot = vocab - 150
        ctx.set_suppress(list(range(eot + 1, eot + 10)), [eot])
        ctx.set_timestamp_rules(True, vocab - 100, eot, 20)
        for T in (0.0, 0.9):
            opts = b.wm_decode_opts(T, 5, eot + 3, 0)
            got = ctx.transcribe_mel_raw(mel, base, 3000, 0, 3000, prompts, 10, eot, opts, sample_ids=ids, no_speech=True,
                                         sot_tail=1)
            for r in (0, 7, n - 1, lens.index(21)):
                o = b.wm_decode_opts(T, 5, eot + 3, lens[r] - 1)
                one = ctx.transcribe_mel_raw(mel, base[r:r + 1], 3000, 0, 3000, np.array([prompts[r]], np.int32), 10, eot, o,
                                             sample_ids=ids[r:r + 1], no_speech=True)
                _same([x[r:r + 1] for x in got], one, "%s, T %g, row %d" % (shape, T, r))
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4. the self-attention launch on its own
@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    vp, ip = ctypes.c_void_p, ctypes.c_int
    c.lib.wmdbg_dec_attention.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, vp]
    c.lib.wmdbg_dec_self_attention_off.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, vp, vp]
    yield c
    c.close()


def _self_attn_off(dbg, q, k, v, pos, off):
    Bn, H, T = k.shape[:3]
    out = np.full((Bn, H * 64), np.nan, np.float32)
    off = np.ascontiguousarray(off, dtype=np.int32)
    st = dbg.lib.wmdbg_dec_self_attention_off(dbg.handle, P(q), P(k), P(v), Bn, H, T, pos, P(off), P(out))
    assert st == 0, dbg.lib.wm_last_error()
    return out


@pytest.mark.parametrize("pos", [0, 36, 127, 128, 226, 447])
def test_self_attention_with_row_offsets(dbg, pos):
    T = 448
    for Bn, H in ((2, 2), (2, 3), (1, 3), (3, 2), (32, 20)):
        rng = np.random.default_rng(1000 * pos + 10 * Bn + H)
        cand = [0, 1, 7, 8, 9, 63, pos - 1, pos, pos + 5]
        cand = [o for o in cand if 0 <= o < T]
        off = np.array([cand[(b + pos + H) % len(cand)] for b in range(Bn)], dtype=np.int32)
        q = rng.standard_normal((Bn, H * 64)).astype(np.float32)
        k = bf(rng.standard_normal((Bn, H, T, 64)))
        v = bf(rng.standard_normal((Bn, H, T, 64)) + np.linspace(-1, 1, 64))
        clean_k, clean_v = k.copy(), v.copy()
        first = np.minimum(off, pos)            # a row that has not started attends to its current row alone
        for b in range(Bn):                     # poison everything in front of the row's keys and behind the position
            k[b, :, :first[b]] = 1e3
            v[b, :, :first[b]] = np.nan
            k[b, :, pos + 1:] = 1e3
            v[b, :, pos + 1:] = np.nan
        out = _self_attn_off(dbg, q, k, v, pos, off)
        assert np.isfinite(out).all(), (Bn, H, off.tolist())
        started = [b for b in range(Bn) if off[b] <= pos]
        # (b) the f64 softmax over keys [off_b, pos], the gate of test_kernels_gpu.test_decode_attention
        for b in started:
            tq = torch.from_numpy(q[b]).double().view(H, 1, 64)
            tk = torch.from_numpy(clean_k[b, :, off[b]:pos + 1]).double()
            tv = torch.from_numpy(clean_v[b, :, off[b]:pos + 1]).double()
            ref = (torch.softmax(tq @ tk.transpose(-1, -2) / 8.0, dim=-1) @ tv).reshape(H * 64).numpy()
            assert np.abs(out[b] - ref).max() <= 2 ** -8 * max(1.0, np.abs(ref).max()), (Bn, H, b, int(off[b]))
        # (a) bit-identical to the row's keys at the front of a fresh cache with offset 0 (rows of one offset per call)
        for o in sorted({int(off[b]) for b in started}):
            rows = [b for b in started if off[b] == o]
            n = pos + 1 - o
            k2 = np.full((len(rows), H, T, 64), 1e3, np.float32)
            v2 = np.full((len(rows), H, T, 64), np.nan, np.float32)
            k2[:, :, :n] = clean_k[rows][:, :, o:pos + 1]
            v2[:, :, :n] = clean_v[rows][:, :, o:pos + 1]
            front = _self_attn_off(dbg, np.ascontiguousarray(q[rows]), k2, v2, pos - o, np.zeros(len(rows), np.int32))
            assert np.array_equal(front, out[rows]), (Bn, H, o)
        # (c) offsets all 0: the launch every uniform group has always had
        k0, v0 = clean_k.copy(), clean_v.copy()
        k0[:, :, pos + 1:] = 1e3
        v0[:, :, pos + 1:] = np.nan
        zero = _self_attn_off(dbg, q, k0, v0, pos, np.zeros(Bn, np.int32))
        want = np.zeros((Bn, H * 64), np.float32)
        assert dbg.lib.wmdbg_dec_attention(dbg.handle, P(q), P(k0), P(v0), Bn, H, T, pos + 1, 0, P(want)) == 0
        assert np.array_equal(zero, want), (Bn, H)


def test_ragged_results_do_not_depend_on_what_the_caches_held(lively, pkg, mel10):
    """The ragged batch twice on one context; in between a uniform call whose prompts are the same rows padded on the LEFT
    with other tokens, so that the self-K/V rows in front of every offset and the token buffer hold other contents."""
    _, _, _, ctx = lively
    b = pkg.binding
    _rules(ctx)
    try:
        n = len(LENS)
        prompts = _prompts(LENS, seed=5)
        ids = np.arange(n, dtype=np.uint32) + 40
        for T in (0.0, 0.9):
            first = _ragged(ctx, b, mel10, _base(n), prompts, T, eot=EOT, ids=ids, sot_tail=1)
            pad = _prompts([max(LENS)] * n, seed=99)
            padded = np.array([pad[r][:max(LENS) - len(prompts[r])] + prompts[r] for r in range(n)], dtype=np.int32)
            ctx.transcribe_mel_raw(mel10, _base(n), 3000, 0, 3000, padded, NEW, EOT, b.wm_decode_opts(T, 1, NS_TOK, 0),
                                   sample_ids=ids, no_speech=True)
            second = _ragged(ctx, b, mel10, _base(n), prompts, T, eot=EOT, ids=ids, sot_tail=1)
            _same(second, first, "T %g" % T)
    finally:
        _rules(ctx, False)


# ---------------------------------------------------------------- 5. oracle
def test_ragged_rows_follow_the_oracle(lively, pkg, mel10):
    dims, _, sd, ctx = lively
    b = pkg.binding
    _rules(ctx)
    try:
        lens = [6, 1, 17]
        prompts = _prompts(lens, seed=11)
        got = _ragged(ctx, b, mel10, _base(3), prompts, 0.0, new=16)
        xa = ctx.encode_mel(mel10[:3])
        for r in range(3):
            _check_policy_choices(sd, dims, xa[r:r + 1], np.array(prompts[r]), got[0][r:r + 1], SPECIALS, [EOT], TS, EOT, MAXI)
    finally:
        _rules(ctx, False)


# ---------------------------------------------------------------- 6. argument checks
def test_ragged_call_rejects_invalid_arguments(lively, pkg, mel10):
    _, _, _, ctx = lively
    b = pkg.binding
    base = _base(2)
    good = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], dtype=np.int32)

    def call(prompts=good, plen=(4, 2), sot_tail=1, new=4, no_speech=False, opts=None, **kw):
        return ctx.transcribe_mel_raw(mel10, kw.get("base", base), kw.get("mel_len", 3000), kw.get("seek", 0),
                                      kw.get("n_frames", 3000), prompts, new, EOT,
                                      opts if opts is not None else b.wm_decode_opts(0.0, 0, NS_TOK, 0), no_speech=no_speech,
                                      prompt_len=np.array(plen, dtype=np.int32), sot_tail=sot_tail)
    bad_tok = good.copy()
    bad_tok[1, 1] = 1 << 20
    unread = good.copy()
    unread[1, 2:] = 1 << 20     # past prompt_len[1] = 2: not looked at
    cases = [dict(plen=(0, 2)), dict(plen=(4, 5)), dict(plen=(4, -1)),
             dict(sot_tail=0, no_speech=True), dict(sot_tail=3, no_speech=True), dict(sot_tail=-1, no_speech=True),
             dict(new=N_CTX - 3), dict(prompts=bad_tok),
             dict(seek=-1), dict(n_frames=3001), dict(mel_len=0), dict(new=0),
             dict(opts=b.wm_decode_opts(-1.0, 0, NS_TOK, 0)), dict(opts=b.wm_decode_opts(0.0, 0, -1, 0), no_speech=True)]
    for kw in cases:
        with pytest.raises(b.WhisperError) as e:
            call(**kw)
        assert e.value.status == WM_ERR_INVALID and str(e.value), kw
        ok = call(prompts=unread)     # the context is usable afterwards
        assert ok[0].shape == (2, 4)
    # what is NOT an error: sot_tail out of range without the no-speech output, the longest prompt filling the context
    call(sot_tail=0)
    call(sot_tail=9)
    call(new=N_CTX - 4)
    assert np.array_equal(call(prompts=unread)[0], call()[0])


# ---------------------------------------------------------------- 7. long form
def _conditioned(prod, recs, ids, seeds, **extra):
    return prod.transcribe_long(recs, recording_ids=ids, condition_on_previous_text=True, sot_prev=SOT_PREV,
                                initial_prompt_tokens=seeds, **_kw(**extra))


@pytest.mark.parametrize("run", ["no fallback", "forced, no reset", "forced, reset at 0.5"])
def test_conditioned_long_form_batched_equals_alone_and_follows_the_rule(prod, run):
    n_ctx = 64
    recs = _long_recs()
    ids = [7, 300, 65535, 0]
    rng = np.random.default_rng(21)
    seeds = [[int(t) for t in rng.integers(0, 50000, size=n)] for n in (0, 2, 5, n_ctx)]
    extra = {"no fallback": dict(logprob_threshold=None, compression_ratio_threshold=None),
             "forced, no reset": dict(logprob_threshold=0.0, prompt_reset_on_temperature=2.0),
             "forced, reset at 0.5": dict(logprob_threshold=0.0)}[run]
    reset_above = extra.get("prompt_reset_on_temperature", 0.5)
    got = _conditioned(prod, recs, ids, seeds, **extra)
    for r, x in enumerate(recs):
        alone = _conditioned(prod, [x], [ids[r]], [seeds[r]], **extra)[0]
        assert _strip(alone) == _strip(got[r]), "recording %d" % r
        assert [w["prompt_len"] for w in alone["windows"]] == [w["prompt_len"] for w in got[r]["windows"]]
    cap = n_ctx // 2 + 3
    # a round whose rows have at least three different prompt lengths, and a prompt at the cap
    n_rounds = max(len(o["windows"]) for o in got)
    per_round = [{o["windows"][i]["prompt_len"] for o in got if i < len(o["windows"])} for i in range(n_rounds)]
    assert [w["prompt_len"] for w in (o["windows"][0] for o in got)] == [3, 6, 9, cap]
    assert any(len(s) >= 3 for s in per_round) and any(cap in s for s in per_round)
    # every window's prompt is what the literal rule gives from the earlier windows' records
    for r, o in enumerate(got):
        lang = o["language"]
        want = expected_prompts(o["windows"], o["segments"], seeds[r], [SOT, lang, TASK], SOT_PREV, n_ctx, reset_above)
        assert [w["prompt"] for w in o["windows"]] == want, (run, r)
        assert all(w["prompt_len"] == len(w["prompt"]) <= cap for w in o["windows"])
    if run == "no fallback":
        assert all(w["temperatures"] == [0.0] for o in got for w in o["windows"])
        fed = False
        for o in got:
            for i in range(1, len(o["windows"])):
                prev_w, w = o["windows"][i - 1], o["windows"][i]
                made = [t for s in o["segments"] if s["seek"] == prev_w["seek"] for t in s["tokens"]]
                body = w["prompt"][1:-3]
                if w["prompt_len"] > 3 and made and body[-len(made):] == made[-len(body):]:
                    fed = True
        assert fed, "no window was conditioned on the tokens of the window before it"
    else:
        assert any(t > 0 for o in got for w in o["windows"] for t in w["temperatures"])
    if run == "forced, reset at 0.5":
        reset = False
        for o in got:
            for i in range(1, len(o["windows"])):
                prev_w, w = o["windows"][i - 1], o["windows"][i]
                if not prev_w["skipped"] and prev_w["temperatures"][-1] > 0.5:
                    assert w["prompt_len"] == 3 and w["prompt"] == [SOT, o["language"], TASK]
                if w["prompt_len"] == 3 and any(p["prompt_len"] > 3 for p in o["windows"][:i]):
                    reset = True
        assert reset, "no prompt went back to three tokens after a longer one"


def test_per_recording_initial_prompts_without_conditioning(prod):
    recs = _long_recs()[:3]
    seeds = [[], [400, 401], [402, 403, 404, 405, 406]]
    got = prod.transcribe_long(recs, sot_prev=SOT_PREV, initial_prompt_tokens=seeds, language=[50259, 50260, 50261], **_kw())
    for r, o in enumerate(got):
        head = ([SOT_PREV] + seeds[r]) if seeds[r] else []
        assert all(w["prompt"] == head + [SOT, 50259 + r, TASK] for w in o["windows"])
        # a recording with the flat list of today's interface: the same windows
        if seeds[r]:
            flat = prod.transcribe_long([recs[r]], sot_prev=SOT_PREV, initial_prompt_tokens=seeds[r], language=50259 + r,
                                        recording_ids=[r], **_kw())[0]
            assert _strip(flat) == _strip(o)
