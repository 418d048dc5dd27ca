"""Kernel-level tests of the per-row temperature and seed (wm_set_sampling_rows) through
wmdbg_decode_close_rows: one decode position -- the DE_LOGITS_X launch, the truncation launch when the rules are on, the close --
with the rows' table in force.  Every case is compared BIT FOR BIT, row by row, with wmdbg_decode_close (or _trunc) on the SAME
rows at that row's scalar (T, seed): the row keeps its index in the call, so its Philox counter words are the same.  The outputs
compared are the tokens, the result words, the log-probs, the stored logits and no_speech_prob."""
import ctypes
import types

import numpy as np
import pytest

from test_decode_step_kernels_gpu import GEOMS, Step, bits, dbg, pool_rows, run_step, sum_rule_inputs, world  # noqa: F401  (dbg: fixture)

pytestmark = pytest.mark.gpu

vp, ip = ctypes.c_void_p, ctypes.c_int
SEED = 2 ** 40 + 7
OFF = (0, 1.0, 0.0)
GEOM_NAMES = ["small64", "production"]
assert set(GEOM_NAMES) <= set(GEOMS)


def stand_in(dbg, close):
    return types.SimpleNamespace(handle=dbg.handle, lib=types.SimpleNamespace(wmdbg_decode_close=close, wm_last_error=dbg.lib.wm_last_error))


def run_rows(dbg, w, rows, Ts, seeds, rule=OFF, **kw):
    """run_step with wmdbg_decode_close_rows in the place of wmdbg_decode_close (xm: the step's X-mode fields without T / seed)"""
    fn = dbg.lib.wmdbg_decode_close_rows
    fn.argtypes = [vp, ctypes.POINTER(Step), vp, vp, ip, ctypes.c_float, ctypes.c_float]
    t = np.ascontiguousarray(Ts, dtype=np.float32)
    sd = np.ascontiguousarray([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64)
    assert t.size == sd.size == len(rows)

    def close(handle, step):
        return fn(handle, step, t.ctypes.data_as(vp), sd.ctypes.data_as(vp), rule[0], rule[1], rule[2])
    return run_step(stand_in(dbg, close), w, rows, **kw)


def run_scalar(dbg, w, rows, T, seed, rule=OFF, xm=None, **kw):
    """the call that exists today: wmdbg_decode_close, or wmdbg_decode_close_trunc under a rule"""
    xm = dict(xm or {}, T=float(np.float32(T)), seed=int(seed))
    if rule == OFF:
        return run_step(dbg, w, rows, xm=xm, **kw)
    fn = dbg.lib.wmdbg_decode_close_trunc
    fn.argtypes = [vp, ctypes.POINTER(Step), ip, ctypes.c_float, ctypes.c_float]
    return run_step(stand_in(dbg, lambda h, s: fn(h, s, rule[0], rule[1], rule[2])), w, rows, xm=xm, **kw)


def check_rows(dbg, w, rows, Ts, seeds, rule=OFF, xm=None, **kw):
    """the per-row call against one scalar call per distinct (T, seed); a temperature-0 row against the T = 0 call (any seed)"""
    got = run_rows(dbg, w, rows, Ts, seeds, rule, xm=dict(xm or {}), **kw)
    keys = {}
    for b, (T, sd) in enumerate(zip(Ts, seeds)):
        keys.setdefault((float(T), int(sd) if T > 0 else 0), []).append(b)
    for (T, sd), bs in keys.items():
        want = run_scalar(dbg, w, rows, T, sd, rule, xm=xm, **kw)
        for b in bs:
            what = (T, sd, b)
            assert got.tok[b] == want.tok[b] and got.result[b] == want.result[b], what
            assert bits(got.logprob)[b] == bits(want.logprob)[b], what
            assert bits(got.nospeech)[b] == bits(want.nospeech)[b], what
            assert np.array_equal(bits(got.logits[b]), bits(want.logits[b])), what
            assert np.array_equal(got.seq[:, b], want.seq[:, b]), what
            assert np.array_equal(bits(got.x_next[b]), bits(want.x_next[b])), what
        assert got.logprob_written == want.logprob_written
        if got.done is not None:
            assert np.array_equal(got.done[bs], want.done[bs])
    return got


def patterns(B):
    """name -> (temperatures, seeds) of B rows"""
    quad = [0.0, 0.7, 0.0, 1.3]
    p = {
        "all_zero": ([0.0] * B, [SEED + b for b in range(B)]),
        "one_pair": ([0.7] * B, [SEED] * B),
        "mixed_quad": ([quad[b % 4] for b in range(B)], [SEED + (b % 4) for b in range(B)]),
        "low_words": ([0.9] * B, [SEED + (b % 3) for b in range(B)]),
        "high_words": ([0.9] * B, [SEED + ((b % 3) << 32) for b in range(B)]),
    }
    if B > 16:
        p["row_16_alone"] = ([0.8 if b == 16 else 0.0 for b in range(B)], [SEED] * B)
    return p


def group(B):
    """(rows, early stop) of a row count: 40 rows run with early stop and some rows already done"""
    rows = pool_rows(B, 11)
    if B < 40:
        return rows, None
    done = np.zeros(B, np.int32)
    done[[0, 17, 39]] = 1
    return rows, dict(done=done, eot=3, pad=3)


@pytest.mark.parametrize("B", [1, 5, 17, 40])
@pytest.mark.parametrize("geom", GEOM_NAMES)
def test_a_generated_position_row_by_row(dbg, geom, B):
    w = world(geom)
    rows, stop = group(B)
    sampled = 0
    for name, (Ts, seeds) in patterns(B).items():
        got = check_rows(dbg, w, rows, Ts, seeds, pos=5, n_prompt=3, n_ctx=16, arg_first=1, arg_last=w.V - 2, fallback=w.eot, stop=stop)
        if name == "all_zero":   # ... which is also the X-mode arg-max call of today
            want = run_step(dbg, w, rows, xm=dict(T=0.0), pos=5, n_prompt=3, n_ctx=16, arg_first=1, arg_last=w.V - 2, fallback=w.eot,
                            stop=stop)
            assert np.array_equal(got.tok, want.tok) and np.array_equal(bits(got.logprob), bits(want.logprob))
            zero = got
        else:
            sampled += int(np.sum(got.tok != zero.tok))
    assert sampled > 0 or B == 1   # (the sampling rows did draw: not every pattern returns the arg-max)


@pytest.mark.parametrize("geom", GEOM_NAMES)
def test_prompt_and_sot_positions(dbg, geom):
    """A prompt position (gi < 0): nothing samples, the token comes from the prompt.  The <|startoftranscript|> position:
    no_speech_prob is the scalar call's (check_rows compares its bits), at a prompt position and at a generated one."""
    w = world(geom)
    B = 17
    rows, _ = group(B)
    Ts, seeds = patterns(B)["mixed_quad"]
    seq = (np.arange(16 * B, dtype=np.int32).reshape(16, B) * 13 + 50) % w.V
    got = check_rows(dbg, w, rows, Ts, seeds, pos=1, n_prompt=4, n_ctx=16, seq=seq, xm=dict(sot_pos=1, ns_tok=33), fallback=2)
    assert got.logprob_written == 0 and np.array_equal(got.seq, seq)
    zero = run_step(dbg, w, rows, pos=1, n_prompt=4, n_ctx=16, seq=seq, xm=dict(T=0.0, sot_pos=1, ns_tok=33), fallback=2)
    assert np.array_equal(bits(got.nospeech), bits(zero.nospeech))
    got = check_rows(dbg, w, rows, Ts, seeds, pos=3, n_prompt=4, n_ctx=16, xm=dict(sot_pos=3, ns_tok=33), fallback=2)
    zero = run_step(dbg, w, rows, pos=3, n_prompt=4, n_ctx=16, xm=dict(T=0.0, sot_pos=3, ns_tok=33), fallback=2)
    assert np.array_equal(bits(got.nospeech), bits(zero.nospeech)) and got.logprob_written == B


@pytest.mark.parametrize("B", [5, 40])
@pytest.mark.parametrize("geom", GEOM_NAMES)
def test_under_the_timestamp_rules(dbg, geom, B):
    """the sum-rule rows of sum_rule_inputs: forced or not is decided on the raw logits, per row, whatever the row's temperature"""
    w = world(geom)
    rows, bias, rng, _ = sum_rule_inputs(w, B)
    _, stop = group(B)
    ts = dict(mode=2, rng=rng, hist=np.tile([3, 0, 0, -1], (B, 1)))
    for name in ("mixed_quad", "low_words"):
        Ts, seeds = patterns(B)[name]
        check_rows(dbg, w, rows, Ts, seeds, pos=6, n_prompt=3, n_ctx=16, bias=bias, ts=ts, fallback=w.eot, stop=stop)


@pytest.mark.parametrize("rule", [(5, 1.0, 0.0), (0, 0.9, 0.05)])
@pytest.mark.parametrize("geom", GEOM_NAMES)
def test_with_the_truncation_rules(dbg, geom, rule):
    """the truncation launch reads the row's own flag, 1 / T and key; a temperature-0 row is untouched by it: the rules-off
    arg-max call's bits"""
    w = world(geom)
    for B in (5, 17):
        rows, _ = group(B)
        rs, bias, rng, _ = sum_rule_inputs(w, B)
        for use_ts in (False, True):
            kw = dict(pos=4, n_prompt=3, n_ctx=16, fallback=w.eot)
            if use_ts:
                kw.update(bias=bias, ts=dict(mode=2, rng=rng, hist=np.tile([3, 0, 0, -1], (B, 1))))
            r = rs if use_ts else rows
            for name in ("mixed_quad", "high_words", "all_zero"):
                Ts, seeds = patterns(B)[name]
                got = check_rows(dbg, w, r, Ts, seeds, rule, **kw)
                plain = run_step(dbg, w, r, xm=dict(T=0.0), **kw)
                for b in range(B):
                    if Ts[b] == 0:
                        assert got.tok[b] == plain.tok[b] and bits(got.logprob)[b] == bits(plain.logprob)[b]
