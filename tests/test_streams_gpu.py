"""GPU tests of live streams (include/whisper_mi355x.h wm_streams_*, csrc/streams.cpp / streams.hip and the stream rule of
csrc/frontend.hip's f32 stage-1 kernel) on a front-end-only context: a stream's frames do not depend on how its audio was
split into pushes or on the dtype of a piece, bit for bit; window (0, A) is wm_logmel_long's columns of the audio so far, bit
for bit, and within the f32 front end's 1e-4 of the f64 restatement (tests/stream_ref.py); streams of a set are independent;
windows that start later and the ring wrap; 64-bit stream time; extents and argument checks."""
import ctypes
import os

import numpy as np
import pytest

import stream_ref as SR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

WM_ERR_INVALID, WM_ERR_STATE = 1, 3   # include/whisper_mi355x.h
PIECES = (1, 159, 160, 161, 399, 400, 401, 10479, 10480, 10481, 0)   # 10 480 samples: a workgroup's span
DTYPES = (np.int16, np.float32, np.float64)
N_SIG = 50001


@pytest.fixture(scope="module")
def fe(pkg):
    ctx = pkg.binding.Context(debug=True)
    yield ctx
    ctx.lib.wmdbg_streams_min_capacity(0)
    ctx.close()


@pytest.fixture(scope="module")
def filters(pkg):
    lib = pkg.binding.load_debug_library()
    f128 = np.zeros((128, 201), np.float32)
    assert lib.wmdbg_mel_filterbank(128, f128.ctypes.data_as(ctypes.c_void_p)) == 0
    return {80: np.load(os.path.join(GOLDEN, "m80.npy")).reshape(80, 201), 128: f128}


def _signal(n, seed=0, burst=None):
    """int16 samples: every dtype of a piece then holds exactly the same values"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.25 * np.sin(t * 0.031) * (1 + 0.5 * np.cos(t * 7e-4)) + 0.01 * rng.standard_normal(n)
    if burst is not None:
        x[burst[0]:burst[1]] += 0.6 * np.sin(t[burst[0]:burst[1]] * 0.4)
    return np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)


def _as(q, dtype):
    return q if dtype == np.int16 else (q.astype(np.float64) / 32768.0).astype(dtype)


def _cuts(n, order):
    """piece boundaries of n samples: PIECES cycled in the given order until the signal is used up"""
    out, at, i = [], 0, 0
    while at < n:
        k = min(PIECES[order[i % len(order)]], n - at)
        out.append((at, at + k))
        at += k
        i += 1
    return out


def _counters(streams, pkg, want_n):
    n, F, A, K = streams.frames()
    for s, N in enumerate(want_n):
        assert (int(F[s]), int(A[s]), int(K[s])) == pkg.binding.stream_frame_counts(N, streams.capacity_frames) == \
            SR.counts(N, streams.capacity_frames)
        assert int(n[s]) == N
    return A


_LONG = {}


def _long(fe, q, N, n_mels):
    """wm_logmel_long of the first N samples, columns [0, A): computed once per (signal, N, n_mels), never modified"""
    key = (q.ctypes.data, N, n_mels)
    if key not in _LONG:
        A = SR.counts(N, 1 << 40)[1]
        m = fe.logmel_long([_as(q[:N], np.float32)], n_mels=n_mels)[0][:, :A].copy()
        m.setflags(write=False)
        _LONG[key] = m
    return _LONG[key]


@pytest.fixture(scope="module")
def sig():
    return _signal(N_SIG, seed=1)


@pytest.mark.parametrize("n_mels", [80, 128])
def test_split_invariance_bit_for_bit(fe, pkg, sig, filters, n_mels):
    b = pkg.binding
    orders = (list(range(len(PIECES))), list(range(len(PIECES)))[::-1], [7, 10, 0, 4, 9, 2, 5, 1, 8, 3, 6], None)
    final = []
    for oi, order in enumerate(orders):
        cuts = [(0, N_SIG)] if order is None else _cuts(N_SIG, order)
        with b.Streams(fe, 1, n_mels=n_mels) as st:
            for pi, (a, z) in enumerate(cuts):
                st.push([_as(sig[a:z], DTYPES[(pi + oi) % 3])])
                A = int(_counters(st, pkg, [z])[0])
                if A:
                    got = st.window([(0, 0, A)], device=False)[0]
                    assert np.array_equal(got, _long(fe, sig, z, n_mels)), "order %d, %d samples" % (oi, z)
            final.append(got)
    assert all(np.array_equal(final[0], f) for f in final[1:])
    A = SR.counts(N_SIG, 1 << 40)[1]
    want = SR.window(SR.raw_frames(sig.astype(np.float64) / 32768.0, filters[n_mels]), 0, A)
    err = float(np.abs(final[0] - want).max())
    assert err <= 1e-4, "max|err| against the f64 restatement %g" % err


@pytest.mark.parametrize("n", [1, 41, 121, 200, 201, 359, 360])
def test_short_starts(fe, pkg, sig, filters, n):
    """Frame 0 is final only at 201 samples, and its reflection reaches past the samples that have arrived before that."""
    b = pkg.binding
    outs = []
    for split in ((n,), (1, n - 1), (n // 2, 0, n - n // 2)):
        with b.Streams(fe, 1) as st:
            at = 0
            for i, k in enumerate(split):
                st.push([_as(sig[at:at + k], DTYPES[i % 3])])
                at += k
            A = int(_counters(st, pkg, [n])[0])
            outs.append(st.window([(0, 0, A)], device=False)[0])
    assert all(np.array_equal(outs[0], o) for o in outs[1:])
    assert np.array_equal(outs[0], _long(fe, sig, n, 80))
    want = SR.window(SR.raw_frames(sig[:n].astype(np.float64) / 32768.0, filters[80]), 0, outs[0].shape[1])
    assert np.abs(outs[0] - want).max() <= 1e-4


def test_streams_are_independent(fe, pkg):
    b = pkg.binding
    sigs = [_signal(20000 + 777 * s, seed=10 + s) for s in range(3)]
    plans = [[3000, 0, 161, 9000, 7839], [1, 10480, 0, 5000, 5296], [0, 400, 12000, 0, 9154]]
    assert [sum(p) for p in plans] == [len(q) for q in sigs]

    def run(which):
        outs = {}
        with b.Streams(fe, len(which)) as st:
            at = [0] * 3
            for step in range(5):
                pieces = []
                for s in which:
                    k = plans[s][step]
                    pieces.append(_as(sigs[s][at[s]:at[s] + k], np.float32) if k else None)
                    at[s] += k
                st.push(pieces)
            A = _counters(st, pkg, [len(sigs[s]) for s in which])
            wins = st.window([(i, 0, int(A[i])) for i in range(len(which))], device=False)
            for i, s in enumerate(which):
                outs[s] = wins[i]
            if len(which) == 3:
                st.reset(1)
                n, F, A2, K = st.frames()
                assert (int(n[1]), int(F[1]), int(A2[1]), int(K[1])) == (0, 0, 0, 0) and int(A2[0]) == int(A[0])
                again = st.window([(0, 0, int(A[0])), (2, 0, int(A[2]))], device=False)
                assert np.array_equal(again[0], outs[0]) and np.array_equal(again[1], outs[2])
                st.push([None, _as(sigs[1][:5000], np.int16), None])     # the reset stream starts over, reflected start included
                assert np.array_equal(st.window([(1, 0, 33)], device=False)[0],
                                      fe.logmel_long([_as(sigs[1][:5000], np.float32)])[0][:, :33])
        return outs
    together = run([0, 1, 2])
    for s in range(3):
        assert np.array_equal(run([s])[s], together[s])


def test_later_windows_and_the_ring_wrap(fe, pkg, filters):
    """A ring of 256 columns holds the last 256 frames of 3 x 256 frames' worth of audio.  The loud burst lies in the last 200
    frames: a window over them has the recording's maximum and equals wm_logmel_long's columns bit for bit; a quiet window
    elsewhere is normalised by its own maximum."""
    b = pkg.binding
    CAP = 256
    n = 3 * CAP * 160
    q = _signal(n, seed=20, burst=(n - 150 * 160, n - 100 * 160))
    raw = SR.raw_frames(q.astype(np.float64) / 32768.0, filters[80])
    A = raw.shape[1]
    assert A == SR.counts(n, CAP)[1] and np.argmax(raw.max(axis=0)) >= A - 200
    assert fe.lib.wmdbg_streams_min_capacity(CAP) == CAP
    try:
        outs = []
        for pieces in ([n], [10481, 1, 30000, 399, 161, 50000, n - 91042]):
            with b.Streams(fe, 1, capacity_frames=CAP) as st:
                at = 0
                for i, k in enumerate(pieces):
                    st.push([_as(q[at:at + k], DTYPES[i % 3])])
                    at += k
                assert int(_counters(st, pkg, [n])[0]) == A
                K = A - CAP
                loud, quiet = (0, A - 200, 200), (0, K + 3, 40)
                both = st.window([loud, quiet], device=False)
                one = [st.window([loud], device=False)[0], st.window([quiet], device=False)[0]]
                assert np.array_equal(both[0], one[0]) and np.array_equal(both[1], one[1])
                outs.append(both)
                for bad in ((0, K - 1, 10), (0, A - 9, 10)):
                    with pytest.raises(b.WhisperError):
                        st.window([bad], device=False)
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    finally:
        fe.lib.wmdbg_streams_min_capacity(0)
    long_ = fe.logmel_long([_as(q, np.float32)])[0]
    assert np.array_equal(outs[0][0], long_[:, A - 200:A])
    assert np.abs(outs[0][0] - SR.window(raw, A - 200, 200)).max() <= 1e-4
    assert np.abs(outs[0][1] - SR.window(raw, A - CAP + 3, 40)).max() <= 1e-4
    # the quiet window's own maximum is lower by far more than the 1e-4 gate: normalising it by the recording's would show
    assert raw[:, A - CAP + 3:A - CAP + 43].max() < raw.max() - 0.01


@pytest.mark.parametrize("near, far", [(1632, (1 << 33) + 1600), (1600, (1 << 33) + 1728)])
def test_64_bit_positions(fe, pkg, filters, near, far):
    """A stream placed at 2^33 + 1600 samples gives, from the first frame centred on a pushed sample on, the bits of a stream
    placed at a small position.  2^33 = 32 (mod 160), so the frame grid of 2^33 + 1600 has the phase of position 1632, not of
    1600: the pair (1632, 2^33 + 1600) keeps that position, the pair (1600, 2^33 + 1728) a whole number of hops, where the f64
    restatement of a placed stream applies as well."""
    b = pkg.binding
    assert (far - near) % 160 == 0 and far > 1 << 33
    q = _signal(20001, seed=30)
    outs = []
    for pos in (near, far):
        with b.Streams(fe, 1) as st:
            assert fe.lib.wmdbg_streams_set_position(fe.handle, st.handle, 0, pos) == 0
            F0 = b.stream_frame_counts(pos, st.capacity_frames)[0]
            st.push([_as(q[:7000], np.int16)])
            st.push([_as(q[7000:], np.float64)])
            n, F, A, K = st.frames()
            assert int(n[0]) == pos + q.size
            assert (int(F[0]), int(A[0])) == b.stream_frame_counts(pos + q.size, st.capacity_frames)[:2] and int(K[0]) == F0
            first = -(-pos // 160)     # the first frame centred on a pushed sample
            outs.append(st.window([(0, first, int(A[0]) - first)], device=False)[0])
            with pytest.raises(b.WhisperError):
                st.window([(0, F0 - 1, 10)], device=False)
    assert outs[0].shape == outs[1].shape and np.array_equal(outs[0], outs[1])
    if near % 160 == 0:
        raw = SR.raw_frames(q.astype(np.float64) / 32768.0, filters[80], n_frames=outs[0].shape[1], from_start=False)
        assert np.abs(outs[0] - SR.window(raw, 0, raw.shape[1])).max() <= 1e-4


def test_extents_and_errors(fe, pkg):
    b, lib = pkg.binding, fe.lib
    q = _signal(30000, seed=40)
    x = _as(q, np.float32)
    h = ctypes.c_void_p()
    for S, n_mels, cap in ((0, 80, 3003), (65536, 80, 3003), (1, 64, 3003), (1, 80, 3002)):
        assert lib.wm_streams_create(fe.handle, S, n_mels, cap, ctypes.byref(h)) == WM_ERR_INVALID and not h.value
    assert lib.wm_streams_create(fe.handle, 1, 80, 3003, None) == WM_ERR_INVALID
    with b.Streams(fe, 2) as st:
        st.push([x[:20000], x[:9000]])
        before = [a.copy() for a in st.frames()]
        A = [int(a) for a in before[2]]
        ref = st.window([(0, 0, A[0]), (1, 0, A[1])], device=False)

        def off(*v):
            return b._ptr(np.array(v, dtype=np.int64))
        i32 = lambda *v: b._ptr(np.array(v, dtype=np.int32))   # noqa: E731
        out = np.zeros(80 * 3000, np.float32)
        push_bad = [
            lib.wm_streams_push(fe.handle, st.handle, b._ptr(x), b.WM_F32, off(0, 10, 5), b.WM_MEM_HOST),      # decreasing
            lib.wm_streams_push(fe.handle, st.handle, b._ptr(x), b.WM_F32, off(-1, 4, 8), b.WM_MEM_HOST),      # negative
            lib.wm_streams_push(fe.handle, st.handle, b._ptr(x), b.WM_F32, off(0, 4, (1 << 30) + 5), b.WM_MEM_HOST),
            lib.wm_streams_push(fe.handle, st.handle, None, b.WM_F32, off(0, 4, 8), b.WM_MEM_HOST),            # null pcm
            lib.wm_streams_push(fe.handle, st.handle, b._ptr(x), b.WM_F32, None, b.WM_MEM_HOST),               # null offsets
            lib.wm_streams_push(fe.handle, st.handle, b._ptr(x), b.WM_BF16, off(0, 4, 8), b.WM_MEM_HOST),      # dtype
            lib.wm_streams_push(fe.handle, None, b._ptr(x), b.WM_F32, off(0, 4, 8), b.WM_MEM_HOST),            # null set
        ]
        assert push_bad == [WM_ERR_INVALID] * len(push_bad)
        win_bad = [
            lib.wm_streams_window(fe.handle, st.handle, 1, i32(2), off(0), i32(10), b._ptr(out), off(0), b.WM_MEM_HOST),    # stream
            lib.wm_streams_window(fe.handle, st.handle, 1, i32(-1), off(0), i32(10), b._ptr(out), off(0), b.WM_MEM_HOST),
            lib.wm_streams_window(fe.handle, st.handle, 1, i32(0), off(0), i32(0), b._ptr(out), off(0), b.WM_MEM_HOST),     # n
            lib.wm_streams_window(fe.handle, st.handle, 1, i32(0), off(0), i32(3001), b._ptr(out), off(0), b.WM_MEM_HOST),
            lib.wm_streams_window(fe.handle, st.handle, 1, i32(0), off(-1), i32(10), b._ptr(out), off(0), b.WM_MEM_HOST),   # below K
            lib.wm_streams_window(fe.handle, st.handle, 1, i32(1), off(A[1] - 9), i32(10), b._ptr(out), off(0), b.WM_MEM_HOST),   # past A
            lib.wm_streams_window(fe.handle, st.handle, 0, i32(0), off(0), i32(10), b._ptr(out), off(0), b.WM_MEM_HOST),    # R
            lib.wm_streams_window(fe.handle, st.handle, 1, None, off(0), i32(10), b._ptr(out), off(0), b.WM_MEM_HOST),
            lib.wm_streams_window(fe.handle, st.handle, 1, i32(0), off(0), i32(10), None, off(0), b.WM_MEM_HOST),
            lib.wm_streams_window(fe.handle, st.handle, 1, i32(0), off(0), i32(10), b._ptr(out), None, b.WM_MEM_HOST),
        ]
        assert win_bad == [WM_ERR_INVALID] * len(win_bad)
        assert lib.wm_streams_reset(fe.handle, st.handle, 2) == WM_ERR_INVALID
        assert lib.wm_streams_reset(fe.handle, st.handle, -1) == WM_ERR_INVALID
        assert lib.wm_streams_frames(None, None, None, None, None) == WM_ERR_INVALID
        assert not np.any(out)
        assert all(np.array_equal(a, c) for a, c in zip(before, st.frames()))
        again = st.window([(0, 0, A[0]), (1, 0, A[1])], device=False)
        assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])
        # a push on the device, and canaries around every block of a device window
        d_pcm = fe.to_device(x)
        CAN = 1024
        rows = [(0, 5, 100), (1, 0, A[1]), (0, A[0] - 37, 37)]
        sizes = [80 * r[2] for r in rows]
        base = np.cumsum([CAN] + [s + CAN for s in sizes[:-1]]).astype(np.int64)
        buf = np.full(int(base[-1]) + sizes[-1] + CAN, 12345.0, np.float32)
        d_out = fe.to_device(buf)
        try:
            assert lib.wm_streams_push(fe.handle, st.handle, d_pcm, b.WM_F32, off(20000, 30000, 30000), b.WM_MEM_DEVICE) == 0
            assert [int(v) for v in st.frames()[0]] == [30000, 9000]
            assert lib.wm_streams_window(fe.handle, st.handle, 3, i32(*[r[0] for r in rows]), off(*[r[1] for r in rows]),
                                         i32(*[r[2] for r in rows]), d_out, b._ptr(base), b.WM_MEM_DEVICE) == 0
            got = fe.download(d_out, buf.shape, np.float32)
        finally:
            fe.dev_free(d_pcm)
            fe.dev_free(d_out)
        host = st.window(rows, device=False)
        keep = np.ones(buf.size, bool)
        for r in range(3):
            blk = slice(int(base[r]), int(base[r]) + sizes[r])
            keep[blk] = False
            assert np.array_equal(got[blk].reshape(80, rows[r][2]), host[r])
        assert np.all(got[keep] == 12345.0)
        with b.Streams(fe, 1) as whole:
            whole.push([x])
            assert np.array_equal(whole.window([(0, 5, 100)], device=False)[0], host[0])


def test_a_set_is_bound_to_its_device(fe, pkg):
    """WM_ERR_STATE needs a context on another device; with one device the rule is checked where it can be: a set keeps
    working with a second context on the same device."""
    b = pkg.binding
    x = _as(_signal(5000, seed=50), np.float32)
    other = b.Context(debug=True)
    try:
        with b.Streams(fe, 1) as st:
            st.push([x])
            want = st.window([(0, 0, 33)], device=False)[0]
            offs = np.array([0, 0], np.int64)
            assert fe.lib.wm_streams_push(other.handle, st.handle, None, b.WM_F32, b._ptr(offs), b.WM_MEM_HOST) == 0
            assert np.array_equal(st.window([(0, 0, 33)], device=False)[0], want)
            try:
                far = b.Context(device=1, debug=True)
            except b.WhisperError:
                far = None   # one visible device
            if far is not None:
                try:
                    assert fe.lib.wm_streams_push(far.handle, st.handle, None, b.WM_F32, b._ptr(offs), b.WM_MEM_HOST) == WM_ERR_STATE
                    assert fe.lib.wm_streams_reset(far.handle, st.handle, 0) == WM_ERR_STATE
                finally:
                    far.close()
                fe.sync()   # (makes this context's device current again)
                assert np.array_equal(st.window([(0, 0, 33)], device=False)[0], want)
    finally:
        other.close()
