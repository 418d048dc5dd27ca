"""wm_set_teacher_panel end to end: the teacher-forced entries (wm_align, wm_align_mel, wm_align_windows, wm_decode_logits)
at panel widths 2 .. 8 against width 1, on the raw bits -- the width is a launch policy, not a numerics switch -- plus the
setter's checks, its inheritance by wm_clone, the launches a pass records, and transcribe_long(teacher_panel=...).
Model: tiny.en geometry, device-generated synthetic weights with the `lively` matrix gain."""
import ctypes

import numpy as np
import pytest

from test_longform_gpu import _kw, _long_recs, prod  # noqa: F401  (prod: fixture)
from test_longform_words_gpu import _strip_words, _words_kw, prod_vocab  # noqa: F401  (prod_vocab: fixture)
from test_model_gpu import tones

pytestmark = pytest.mark.gpu

EOT, NO_TS, SOT = 50256, 50362, 50257
S = 3   # start sequence [sot, language-like, task-like]
HEADS = [(1, 0), (1, 3), (3, 2), (3, 5)]   # two alignment layers of the four
WM_ERR_INVALID = 1


@pytest.fixture(scope="module")
def tiny(pkg):
    dims = dict(pkg.binding.MODEL_DIMS["tiny.en"])
    ctx = pkg.binding.Context(dims, debug=True)
    ctx.init_synthetic(23, matrix_gain=4.0)
    ctx.finalize()
    ctx.set_alignment_heads(HEADS)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def mel3(tiny):
    return tiny.logmel(tones(3), out_dtype=np.float32)   # [3][80][3000]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, i)


def _at_width(ctx, w, fn):
    ctx.set_teacher_panel(w)
    try:
        return fn()
    finally:
        ctx.set_teacher_panel(1)


def _windows(Bn, nmax, seed):
    """Bn windows over the three chunks at different seeks and lengths, texts of different lengths (the longest nmax; a 0
    where there is room), one start sequence per row"""
    rng = np.random.default_rng(seed)
    base = (np.arange(Bn) % 3).astype(np.int64) * 80 * 3000
    seek = [int(v) for v in rng.integers(0, 1500, size=Bn)]
    nf = [int(min(3000 - s, v)) for s, v in zip(seek, rng.integers(2, 3001, size=Bn))]
    seek[0], nf[0] = 0, 3000
    lens = [int(v) for v in rng.integers(0, nmax + 1, size=Bn)]
    lens[0] = nmax
    if Bn > 1:
        lens[1] = 0
    if Bn > 2:
        lens[Bn - 1] = 1
    texts = [[int(t) for t in rng.integers(0, EOT, size=n)] for n in lens]
    sots = [[SOT, 100 + b, 7] for b in range(Bn)]
    return base, seek, nf, texts, sots


# T = S + nmax + 2: nmax 11, 12, 16 -> T = 16, 17, 21, i.e. T mod 8 = 0, 1, 5
# More windows than fit a full-width panel (128 / 8 = 16): the cut with the fewest steps.  17 windows run as ONE panel narrowed to 7
# positions, 48 windows at T = 21 as three slices of 16 at width 8 (test_the_cut_of_a_large_group below pins both).
@pytest.mark.parametrize("Bn,nmax", [(1, 11), (1, 12), (1, 16), (3, 11), (3, 12), (3, 16), (17, 11), (17, 12), (17, 16), (48, 16)])
def test_align_mel_is_bit_identical_at_every_width(tiny, mel3, Bn, nmax):
    base, seek, nf, texts, sots = _windows(Bn, nmax, 10 * Bn + nmax)

    def run():
        return tiny.align_mel(mel3, base, 3000, seek, nf, texts, sots, NO_TS, EOT, capture_matrix=True)

    want = run()
    assert np.any(want[0] >= 0) and np.any(want[1] > 0) and np.any(want[2] != 0)
    if Bn > 1:
        assert np.all(want[0][1] == -1) and np.all(want[1][1] == 0)   # the row without text
    for w in (2, 3, 8):
        _same(_at_width(tiny, w, run), want, "width %d" % w)
    _same(run(), want, "width 1 again")


def test_align_pcm_and_align_windows_at_width_8(tiny, mel3):
    pcm = tones(2)
    rng = np.random.default_rng(3)
    texts = [[int(t) for t in rng.integers(0, EOT, size=n)] for n in (9, 4)]

    def run_pcm():
        return tiny.align(pcm, texts, [SOT, 101, 7], NO_TS, EOT, n_frames=[3000, 1700], capture_matrix=True)

    _same(_at_width(tiny, 8, run_pcm), run_pcm(), "wm_align")
    base, seek, nf, texts, sots = _windows(5, 13, 77)
    with tiny.encode_windows(mel3, base, 3000, seek, nf) as ws:
        rows = [4, 0, 2, 3]

        def run_set():
            return tiny.align_windows(ws, rows, [texts[r] for r in rows], [sots[r] for r in rows], NO_TS, EOT)

        want = run_set()
        _same(_at_width(tiny, 8, run_set), want, "wm_align_windows")
    _same(want, tiny.align_mel(mel3, base[rows], 3000, [seek[r] for r in rows], [nf[r] for r in rows], [texts[r] for r in rows],
                               [sots[r] for r in rows], NO_TS, EOT), "the set against the mel")


@pytest.mark.parametrize("T", [13, 1])
def test_decode_logits_is_bit_identical_at_width_8(tiny, mel3, T):
    xa = tiny.encode_mel(mel3)
    tokens = np.random.default_rng(T).integers(0, EOT, size=(3, T)).astype(np.int32)
    want = tiny.decode_logits(tokens, xa)
    assert want.shape == (3, T, tiny.dims["n_vocab"]) and np.isfinite(want).all()
    for w in (8, 5):
        got = _at_width(tiny, w, lambda: tiny.decode_logits(tokens, xa))
        assert np.array_equal(_bits(got), _bits(want)), w


def test_the_setter_checks_its_width(tiny):
    lib = tiny.lib
    lib.wm_set_teacher_panel.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.wm_set_teacher_panel.restype = ctypes.c_int
    for bad in (0, 9, -1):
        assert lib.wm_set_teacher_panel(tiny.handle, bad) == WM_ERR_INVALID
        assert b"teacher_panel" in lib.wm_last_error() and str(bad).encode() in lib.wm_last_error()
    for good in (8, 1):
        assert lib.wm_set_teacher_panel(tiny.handle, good) == 0


def _families(ctx, fn):
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = fn()
        return out, ctx.profile()
    finally:
        ctx.profile_enable(False)


def test_a_clone_inherits_the_width(tiny, mel3):
    base, seek, nf, texts, sots = _windows(3, 16, 5)

    def run(c):
        return lambda: c.align_mel(mel3, base, 3000, seek, nf, texts, sots, NO_TS, EOT)

    want = run(tiny)()
    before = tiny.clone()
    tiny.set_teacher_panel(8)
    try:
        after = tiny.clone()
    finally:
        tiny.set_teacher_panel(1)
    try:
        got_b, prof_b = _families(before, run(before))
        got_a, prof_a = _families(after, run(after))
        _same(got_b, want, "clone made before the call")
        _same(got_a, want, "clone made after the call")
        assert "dec_attn_cross_cand" in prof_a and "dec_embed_panel" in prof_a
        assert "dec_attn_cross_cand" not in prof_b and "dec_embed_panel" not in prof_b
    finally:
        before.close()
        after.close()


def test_a_pass_of_21_positions_at_width_8_is_3_steps(tiny, mel3):
    """T = S + 16 + 2 = 21 positions: 21 self-attention launches per layer at width 1, ceil(21 / 8) = 3 at width 8"""
    base, seek, nf, texts, sots = _windows(3, 16, 9)
    L = tiny.dims["n_text_layer"]

    def run():
        return tiny.align_mel(mel3, base, 3000, seek, nf, texts, sots, NO_TS, EOT)

    want, prof1 = _families(tiny, run)
    got, prof8 = _at_width(tiny, 8, lambda: _families(tiny, run))
    _same(got, want, "width 8")
    assert prof1["dec_attn_self"]["n"] == 21 * L
    assert prof8["dec_attn_self"]["n"] == 3 * L
    assert prof8["dec_gemv_ln_qkv"]["n"] == 3 * L and prof8["dec_gemv_ln_logits"]["n"] == 3
    assert prof8["dec_attn_cross_cand"]["n"] == 3 * L and "dec_attn_cross_cand" not in prof1


@pytest.mark.parametrize("Bn,steps", [(17, 3), (48, 9)])
def test_the_cut_of_a_large_group(tiny, mel3, Bn, steps):
    """T = 21 at width 8: 17 windows = one panel of width 7 (3 steps), 48 windows = 3 slices of 16 x 3 panels (9 steps)"""
    base, seek, nf, texts, sots = _windows(Bn, 16, Bn)
    L = tiny.dims["n_text_layer"]
    _, prof = _at_width(tiny, 8, lambda: _families(tiny, lambda: tiny.align_mel(mel3, base, 3000, seek, nf, texts, sots, NO_TS, EOT)))
    assert prof["dec_attn_self"]["n"] == steps * L and prof["dec_attn_cross_cand"]["n"] == steps * L
    assert prof["dec_embed_panel"]["n"] == steps


def test_transcribe_long_words_do_not_depend_on_the_width(prod, prod_vocab):
    recs = _long_recs()[:2]
    want = prod.transcribe_long(recs, **_words_kw(prod_vocab))
    try:
        got = prod.transcribe_long(recs, teacher_panel=8, **_words_kw(prod_vocab))
    finally:
        prod.set_teacher_panel(1)
    assert any(s.get("words") for o in want for s in o["segments"])
    for a, b in zip(got, want):
        assert _strip_words(a) == _strip_words(b)
