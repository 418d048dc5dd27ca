"""The row tables (wm_set_sequence_bias_tables / wm_set_bias_rows) without a device: the pooled layout of
the host expansion (wmdbg_sb_expand_tables) and a group's per-row ranges (wmdbg_group_bias_rows) against the restatement in
tests/seqbias_rows_ref.py, the limits, what is refused, the wrappers' packing on a stand-in library, and transcribe_long's
recording_bias on the recording fake of tests/test_longform_calls_cpu.py.  (What a refused call leaves in force on a context, and
the exclusivity with wm_set_sequence_bias, need a context and so a device: tests/test_seqbias_rows_gpu.py.)"""
import ctypes
import importlib

import numpy as np
import pytest

import seqbias_ref as SB
import seqbias_rows_ref as SR
from test_decode_align_cpu import AlignedCtx
from test_longform_calls_cpu import SECONDS, cases, make_vocab, run_case, canon
from test_longform_clips_cpu import _rec

B = importlib.import_module("openai-whisper-coreml_amd.binding")
INF = float("inf")
WM_ERR_INVALID = 1
vp, ip = ctypes.c_void_p, ctypes.c_int
V, EOT = 51865, 50257


@pytest.fixture(scope="module")
def dbg(pkg):
    lib = pkg.binding.load_debug_library()
    lib.wmdbg_sb_expand_tables.argtypes = [vp] * 5 + [ip, ctypes.c_int32, ip] + [vp] * 7
    lib.wmdbg_sb_expand_tables.restype = ip
    lib.wmdbg_group_bias_rows.argtypes = [vp, ip, vp, ip, ip, ip, ip, vp]
    lib.wmdbg_group_bias_rows.restype = ip
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


FILL = -77


def expand_call(dbg, tables, eot=EOT, vocab=V, toffs=None, n_tables=None, offs=None):
    """(status, counts, dict of the pooled arrays cut to the counts, the raw buffers) of wmdbg_sb_expand_tables"""
    toks, o, bs, fl, to = SR.pack_tables(tables)
    o = o if offs is None else np.array(offs, np.int32)
    to = to if toffs is None else np.array(toffs, np.int32)
    nt = len(tables) if n_tables is None else n_tables
    cap = SR.MAX_POOL + 2
    counts = np.full(3, FILL, np.int32)
    buf = dict(tab_grp=np.full(max(len(to), 2), FILL, np.int32), grp_id=np.full(cap, FILL, np.int32), grp_beg=np.full(cap, FILL, np.int32),
               ent_len=np.full(cap, FILL, np.int32), ent_bias=np.full(cap, FILL, np.float32),
               ent_ctx=np.full((cap, SR.CTX), FILL, np.int32))
    rc = dbg.wmdbg_sb_expand_tables(_p(toks) if toks.size else None, _p(o), _p(bs) if bs.size else None, _p(fl), _p(to), nt, eot, vocab,
                                    _p(counts), *[_p(buf[k]) for k in ("tab_grp", "grp_id", "grp_beg", "ent_len", "ent_bias", "ent_ctx")])
    got = None
    if rc == 0:
        t, g, e = (int(x) for x in counts)
        got = dict(tab_grp=buf["tab_grp"][:t + 1], grp_id=buf["grp_id"][:g], grp_beg=buf["grp_beg"][:g + 1], ent_len=buf["ent_len"][:e],
                   ent_bias=buf["ent_bias"][:e], ent_ctx=buf["ent_ctx"][:e])
    return rc, counts, got, buf


def same_pool(got, want):
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), k


def full_table(shift=0):
    """exactly 4096 entries after the expansion: 1024 boosted 4-token phrases with distinct first tokens"""
    seqs = [(1000 + 4 * i + shift, 7, 8, 9 + (i % 5)) for i in range(1024)]
    return seqs, [1.0 + (i % 7) for i in range(1024)], [True] * 1024


TABLES = dict(
    empty=([], [], None),
    one=([(5, 6)], [1.5], None),
    shared=([(10, 11, 12), (10, 13), (10, 11, 14, 15), (12,)], [2.0, 3.0, 1.0, -INF], [True, True, True, False]),   # shared first words
    ids=([(3, 9), (4, 9), (9,), (1, 2, 3, 4, 5), (EOT + 1, 9)], [0.5, -INF, 0.25, 1e8, -2.0], None),              # one last token, in order
    long=([tuple(range(100, 132)), tuple(range(100, 131))], [1.0, 2.0], [True, False]),                          # 32 tokens, boosted
)


@pytest.mark.parametrize("names", [["one"], ["empty"], ["empty", "empty"], ["empty", "one", "empty", "shared"],
                                   ["shared", "shared", "ids"], ["ids", "long", "one", "empty"], ["full", "one", "full", "empty"]])
def test_the_pooled_layout_is_the_tables_expanded_one_by_one(dbg, names):
    """wmdbg_sb_expand_tables == seqbias_ref.expand per table, each sorted stably by last token, concatenated, grp_beg absolute,
    with every table's group range: empty tables (first, last, adjacent), one entry, boosted phrases with shared first words,
    the same table twice (duplicates are invalid WITHIN a table only) and a table at exactly 4096 entries."""
    tables = [full_table(i) if n == "full" else TABLES[n] for i, n in enumerate(names)]
    expanded = SR.expand_tables(tables, eot=EOT, V=V)
    if "full" in names:
        assert [len(t) for t, n in zip(expanded, names) if n == "full"] == [SB.MAX_ENTRIES] * names.count("full")
    want = SR.pool(expanded)
    rc, counts, got, buf = expand_call(dbg, tables)
    assert rc == 0
    assert counts.tolist() == [len(names), want["grp_id"].size, sum(len(t) for t in expanded)]
    same_pool(got, want)
    assert np.all(buf["grp_id"][want["grp_id"].size:] == FILL) and np.all(buf["ent_len"][want["ent_len"].size:] == FILL)
    # the ranges: table t's groups hold exactly its entries, in its own single-table layout shifted by the entries in front
    e0 = 0
    for t, ex in enumerate(expanded):
        g0, g1 = want["tab_grp"][t], want["tab_grp"][t + 1]
        alone = SR.pool([ex])
        assert g1 - g0 == alone["grp_id"].size and np.array_equal(got["grp_id"][g0:g1], alone["grp_id"])
        if g1 > g0:
            assert np.array_equal(got["grp_beg"][g0:g1 + 1] - e0, alone["grp_beg"])
        e0 += len(ex)


def test_the_pool_limit(dbg):
    """65536 entries (16 tables x 4096) are accepted, one more is WM_ERR_INVALID; 1024 tables are accepted, 1025 are not"""
    singles = ([(i,) for i in range(4096)], [0.5] * 4096, None)
    rc, counts, got, _ = expand_call(dbg, [singles] * 16)
    assert rc == 0 and counts.tolist() == [16, 65536, 65536] and got["tab_grp"].tolist() == [4096 * t for t in range(17)]
    assert got["grp_beg"].tolist() == list(range(65537))
    rc, counts, _, _ = expand_call(dbg, [singles] * 16 + [TABLES["one"]])
    assert rc == WM_ERR_INVALID and np.all(counts == FILL)
    rc, counts, _, _ = expand_call(dbg, [TABLES["one"]] + [singles] * 16)
    assert rc == WM_ERR_INVALID
    rc, counts, got, _ = expand_call(dbg, [TABLES["one"]] * SR.MAX_TABLES)
    assert rc == 0 and counts.tolist() == [1024, 1024, 1024]
    rc, counts, _, _ = expand_call(dbg, [TABLES["one"]] * (SR.MAX_TABLES + 1))
    assert rc == WM_ERR_INVALID


def test_what_is_refused_writes_nothing(dbg):
    """WM_ERR_INVALID, with every output as it was, for what wm_set_sequence_bias refuses in ANY table and for bad offsets"""
    ok = TABLES["shared"]
    bad_tables = [
        ([(V,)], [1.0], None), ([(1, EOT)], [1.0], None), ([(1,), ()], [1.0, 1.0], None), ([tuple([1] * 33)], [1.0], None),
        ([(1,)], [float("nan")], None), ([(1,)], [INF], None), ([(1, 2), (3,), (1, 2)], [1.0, 1.0, 2.0], None),
        ([(1, 2)], [-INF], [True]),
        ([(i % 1000, i // 1000 + 1) for i in range(4097)], [1.0] * 4097, None),                               # 4097 given
        ([(a, 10 + c, d) for a in range(10) for c in range(20) for d in range(20)], [1.0] * 4000, [True] * 4000),   # 4210 expanded
    ]
    for bad in bad_tables:
        for tables in ([bad], [ok, bad], [bad, ok], [TABLES["empty"], ok, bad, TABLES["one"]]):
            with pytest.raises(SB.Invalid):
                SR.expand_tables(tables, eot=EOT, V=V)
            rc, counts, _, buf = expand_call(dbg, tables)
            assert rc == WM_ERR_INVALID, (bad[0][:3], len(tables))
            assert np.all(counts == FILL) and all(np.all(a == FILL) for a in buf.values())
    two = [TABLES["one"], TABLES["ids"]]
    assert expand_call(dbg, two)[0] == 0
    for kw in (dict(toffs=[1, 1, 6]), dict(toffs=[0, 3, 1]), dict(toffs=[0, -1, 6]), dict(n_tables=-1), dict(eot=-1), dict(eot=V + 1),
               dict(offs=[1, 2, 4, 6, 7, 12, 14]), dict(offs=[0, 2, 1, 6, 7, 12, 14])):
        assert expand_call(dbg, two, **kw)[0] == WM_ERR_INVALID, kw
    # the same sequence in two tables is fine; n_tables = 0 is the empty pool
    assert expand_call(dbg, [TABLES["one"], TABLES["one"]])[0] == 0
    rc, counts, got, _ = expand_call(dbg, [])
    assert rc == 0 and counts.tolist() == [0, 0, 0]


def test_a_groups_row_ranges(dbg):
    """wmdbg_group_bias_rows: decoder row b of the group of windows [b0, b0 + Cg) x N takes the range of table_of_row[b0 + b / N]"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        nt = int(rng.integers(1, 9))
        tab_grp = np.concatenate([[0], np.cumsum(rng.integers(0, 50, nt))]).astype(np.int32)
        Bc = int(rng.integers(1, 140))
        N = int(rng.integers(1, 6))
        Cg = int(rng.integers(1, min(Bc, 128 // N) + 1))
        b0 = int(rng.integers(0, Bc - Cg + 1))
        rows = rng.integers(-1, nt, Bc).astype(np.int32)
        out = np.full((Cg * N, 2), FILL, np.int32)
        assert dbg.wmdbg_group_bias_rows(_p(rows), Bc, _p(tab_grp), nt, b0, Cg, N, _p(out)) == 0
        assert np.array_equal(out, SR.row_ranges(rows, tab_grp, b0, Cg, N)), (nt, Bc, N, Cg, b0)
    rows = np.zeros(4, np.int32)
    out = np.zeros((8, 2), np.int32)
    assert dbg.wmdbg_group_bias_rows(_p(rows), 4, _p(tab_grp), nt, 2, 3, 1, _p(out)) == WM_ERR_INVALID     # the group leaves the call


# ---------------------------------------------------------------- the wrappers' packing
class StandIn:
    """records what the two calls are handed (arrays copied out of the pointers)"""

    def __init__(self, status=0):
        self.calls, self.status = [], status

        def read(p, ct, count):
            return None if p is None else list(ctypes.cast(p, ctypes.POINTER(ct))[:count])

        def tables(handle, toks, offs, bias, flags, toffs, n_tables, eot):
            to = read(toffs, ctypes.c_int32, n_tables + 1)
            n = to[-1] if to else 0
            o = read(offs, ctypes.c_int32, n + 1)
            self.calls.append(("tables", handle, read(toks, ctypes.c_int32, o[-1] if o else 0), o, read(bias, ctypes.c_float, n),
                               read(flags, ctypes.c_uint8, n), to, n_tables, eot))
            return self.status

        def rows(handle, p, n):
            self.calls.append(("rows", handle, read(p, ctypes.c_int32, n), n))
            return self.status
        self.wm_set_sequence_bias_tables, self.wm_set_bias_rows = tables, rows

    def wm_last_error(self):
        return b"stand-in"


def _ctx(lib):
    c = object.__new__(B.Context)
    c.lib, c.handle, c.dims = lib, ctypes.c_void_p(0x1234), dict(n_vocab=51865)
    return c


def test_the_wrappers_pack_the_tables_and_the_rows():
    lib = StandIn()
    c = _ctx(lib)
    c.set_sequence_bias_tables([{(5, 6, 7): 2.0, (np.int64(9),): -INF}, {}, {(1, 2): 0.5, (5, 6, 7): 1.0}],
                               boosts=[[(5, 6, 7)], None, [(1, 2)]], eot=50257)
    c.set_sequence_bias_tables([{(3,): 1.5}])
    c.set_sequence_bias_tables(None)
    c.set_sequence_bias_tables([], eot=7)
    c.set_sequence_bias_tables([{}, {}])
    c.set_bias_rows([2, -1, None, np.int64(0)])
    c.set_bias_rows([])
    assert lib.calls[0][2:] == ([5, 6, 7, 9, 1, 2, 5, 6, 7], [0, 3, 4, 6, 9], [2.0, -INF, 0.5, 1.0], [1, 0, 1, 0], [0, 2, 2, 4], 3, 50257)
    assert lib.calls[1][2:] == ([3], [0, 1], [1.5], None, [0, 1], 1, 51865)
    assert lib.calls[2][2:] == (None, None, None, None, None, 0, 51865) and lib.calls[3][2:] == (None, None, None, None, None, 0, 7)
    assert lib.calls[4][2:] == (None, [0], None, None, [0, 0, 0], 2, 51865)
    assert lib.calls[5][2:] == ([2, -1, -1, 0], 4) and lib.calls[6][2:] == (None, 0)
    assert all(a[1] is c.handle and all(type(x) is int for x in a[-2:]) for a in lib.calls[:5])
    assert lib.wm_set_sequence_bias_tables.argtypes == [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_int32]
    assert lib.wm_set_bias_rows.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    assert lib.wm_set_sequence_bias_tables.restype is ctypes.c_int and lib.wm_set_bias_rows.restype is ctypes.c_int
    # the packing is the restatement's
    toks, offs, bs, fl, toffs = SR.pack_tables([([(5, 6, 7), (9,)], [2.0, -INF], [True, False]), ([], [], None),
                                                ([(1, 2), (5, 6, 7)], [0.5, 1.0], [True, False])])
    assert (toks.tolist(), offs.tolist(), bs.tolist(), fl.tolist(), toffs.tolist()) == lib.calls[0][2:7]
    for bad in (dict(tables=[{(1, 2): 1.0}], boosts=[[(1, 3)]]), dict(tables=[{(1, 2): 1.0}, {(1, 3): 1.0}], boosts=[[(1, 3)], []]),
                dict(tables=[{(1,): 1.0}], boosts=[[], []])):
        with pytest.raises(ValueError):
            c.set_sequence_bias_tables(**bad)
    for fn in (lambda k: k.set_sequence_bias_tables([{(1,): 1.0}]), lambda k: k.set_bias_rows([0])):
        with pytest.raises(B.WhisperError):
            fn(_ctx(StandIn(status=1)))


# ---------------------------------------------------------------- transcribe_long(recording_bias=) on the recording fake
class RowsCtx(AlignedCtx):
    def set_sequence_bias_tables(self, tables=None, boosts=None, eot=None):
        self.calls.append(["set_sequence_bias_tables", None if tables is None else [[[list(k), v] for k, v in t.items()] for t in tables],
                           None if boosts is None else [[list(k) for k in b] for b in boosts], eot])

    def set_bias_rows(self, rows):
        self.calls.append(["set_bias_rows", [int(r) for r in rows]])

    def set_sequence_bias(self, *a, **kw):
        self._log("set_sequence_bias", a, kw)


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    v = make_vocab(tmp_path_factory.mktemp("vocab"))
    yield v
    v.close()


def _run(case, **extra):
    ctx = RowsCtx(case["script"], **case.get("ctx", {}))
    recs = case["recs"] if "recs" in case else [_rec(s) for s in SECONDS]
    got = dict(calls=ctx.calls)
    try:
        got["out"] = canon(B.transcribe_long(ctx, recs, **dict(case["kw"], **extra)))
    except (ValueError, RuntimeError) as e:
        got["error"] = [type(e).__name__, str(e)]
    return got


DECODES = ("transcribe_mel", "transcribe_windows", "transcribe_mel_aligned", "transcribe_windows_aligned")
BIAS = [dict(bad_words=[[4, 5], [6]]), None, dict(sequence_bias={(1, 2): 0.5}, boost_phrases=[[7, 8, 9]], phrase_boost=2.0)]
WANT_TABLES = [[[[4, 5], -INF], [[6], -INF]], [[[1, 2], 0.5], [[7, 8, 9], 2.0]]]
WANT_BOOSTS = [[], [[7, 8, 9]]]
CASES = ["defaults", "cond", "best_of", "beam", "beam_best_of_cond", "reuse", "reuse_words", "reuse_best_of", "reuse_beam", "words",
         "clips_per_recording", "parallel_2_clips", "parallel_true_clips", "parallel_3_words_ids", "parallel_1_reuse_best_of",
         "parallel_2_vad_words_reuse", "vad_true", "decode_raises_in_a_reuse_round", "decode_raises_in_the_first_round",
         "decode_raises_without_reuse", "words_decode", "words_decode_reuse"]


def _case(vocab, name):
    c = cases(vocab)
    if name.startswith("words_decode"):
        base = c["words"]
        kw = {k: v for k, v in base["kw"].items() if k != "no_timestamps"}
        return dict(base, kw=dict(kw, word_timestamps="decode", reuse_encoder=name.endswith("reuse")))
    return c[name]


@pytest.mark.parametrize("name", CASES)
def test_transcribe_long_maps_every_decode_call(vocab, name):
    """With recording_bias the call log is the plain run's plus ONE set_sequence_bias_tables behind the log-mel and in front of
    the first decode, ONE set_bias_rows directly in front of EVERY decode call -- plain, from a reuse_encoder set, best-of and
    beam steps, the aligned entries; every fallback step's subset of the rows -- whose entries are the tables of exactly that
    call's rows (a row's recording is the low 16 bits of its sample id; with parallel_clips a clip takes its recording's
    table), and ONE clear at the very end, also when a decode raises.  The results are the plain run's (the fake does not read
    the tables).  With recording_bias=None the log is the plain run's, call for call."""
    case = _case(vocab, name)
    plain = _run(case)
    if not name.startswith("words_decode"):
        assert canon(plain["calls"]) == run_case(case)["calls"]
    none = _run(case, recording_bias=None)
    assert none["calls"] == plain["calls"]
    got = _run(case, recording_bias=BIAS)
    assert ("error" in got) == ("error" in plain) == name.startswith("decode_raises")
    if "error" in plain:
        assert got["error"] == plain["error"]
    else:
        assert got["out"] == plain["out"]
    calls = got["calls"]
    names = [c[0] for c in calls]
    eot = case["kw"]["eot"]
    sets = [i for i, n in enumerate(names) if n == "set_sequence_bias_tables"]
    assert len(sets) == 2 and sets[1] == len(calls) - 1, names
    assert calls[sets[0]] == ["set_sequence_bias_tables", WANT_TABLES, WANT_BOOSTS, eot]
    assert calls[sets[1]] == ["set_sequence_bias_tables", None, None, None]
    mel = max(i for i, n in enumerate(names) if n in ("logmel_long", "logmel_long_device"))
    first_use = min(i for i, n in enumerate(names) if n.startswith(("transcribe_", "encode_windows", "windows_detect", "set_bias_rows")))
    assert mel < sets[0] < first_use
    rest = [c for c in calls if c[0] not in ("set_sequence_bias_tables", "set_bias_rows")]
    assert rest == plain["calls"] and "set_sequence_bias" not in names
    rec_ids = list(case["kw"].get("recording_ids", range(3)))
    table_of = [0, -1, 1]
    n_maps, sizes = 0, set()
    for i, c in enumerate(calls):
        if c[0] in DECODES:
            assert calls[i - 1][0] == "set_bias_rows", (i, names[max(0, i - 3):i + 1])
            sids = dict((k, v) for k, v in c[2])["sample_ids"]
            assert calls[i - 1][1] == [table_of[rec_ids.index(int(s) & 0xFFFF)] for s in sids], (i, c[0])
            n_maps += 1
            sizes.add(len(sids))
        if c[0] == "set_bias_rows":
            assert calls[i + 1][0] in DECODES
    assert names.count("set_bias_rows") == n_maps >= 1
    if name in ("defaults", "reuse", "words"):
        assert len(sizes) > 1                        # a fallback step decoded a subset of the round's rows
    if name.startswith("words_decode"):
        assert any(n.endswith("_aligned") for n in names) and not any(n in ("transcribe_mel", "transcribe_windows") for n in names)


@pytest.mark.parametrize("name", ["defaults", "reuse_best_of", "parallel_2_clips", "decode_raises_without_reuse"])
@pytest.mark.parametrize("bias", [[None, None, None], [{}, {}, {}], [None, dict(phrase_boost=2.0), {}]])
def test_no_entry_with_a_table_is_the_plain_run(vocab, name, bias):
    """Entries that are all None, or dicts whose three lists are None, give no table: the library refuses a row map on a context
    without tables, so NEITHER call is made and the log is the plain run's, call for call."""
    case = _case(vocab, name)
    plain, got = _run(case), _run(case, recording_bias=bias)
    assert got == plain
    assert not any(c[0] in ("set_sequence_bias_tables", "set_bias_rows") for c in got["calls"])


def test_equal_entries_share_a_table_and_the_errors(vocab):
    f = B.long_recording_tables
    a = dict(bad_words=[[4, 5]], boost_phrases=[(7, 8)], phrase_boost=1.0)
    assert f([a, None, dict(a), dict(sequence_bias={(4, 5): -INF}, boost_phrases=[[7, 8]], phrase_boost=1.0), dict(bad_words=[[4, 5]])], 5) == \
        ([{(4, 5): -INF, (7, 8): 1.0}, {(4, 5): -INF}], [[(7, 8)], []], [0, -1, 0, 0, 1])
    assert f([None, dict(), dict(phrase_boost=2.0)], 3) == ([], [], [-1, -1, -1])
    assert f([dict(bad_words=[])], 1) == ([{}], [[]], [0])                   # an empty table is a table
    # the order of the entries is part of a table: the f32 sum follows it
    assert f([dict(sequence_bias={(1,): 1.0, (2, 1): 2.0}), dict(sequence_bias={(2, 1): 2.0, (1,): 1.0})], 2)[2] == [0, 1]
    for bad, n in (([None], 2), ([dict(bad_word=[[1]])], 1), ([[(1, 2)]], 1), ([dict(boost_phrases=[[1, 2]])], 1),
                   ([dict(bad_words=[[1]], sequence_bias={(1,): 1.0})], 1)):
        with pytest.raises(ValueError):
            f(bad, n)
    case = cases(vocab)["defaults"]
    for extra in (dict(sequence_bias={(1,): 1.0}), dict(bad_words=[[1]]), dict(boost_phrases=[[1, 2]], phrase_boost=1.0),
                  dict(draft=object())):
        got = _run(case, recording_bias=BIAS, **extra)
        assert got["error"][0] == "ValueError" and got["calls"] == [], extra
    got = _run(case, recording_bias=BIAS[:2])
    assert got["error"][0] == "ValueError" and got["calls"] == []
