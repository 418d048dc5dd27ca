"""Kernel-level GPU tests of the row tables (wm_set_sequence_bias_tables): the state kernel alone
(wm_seqbias_rows_state through wmdbg_seqbias_rows_state) compared EXACTLY -- no tolerance anywhere -- with the numpy restatement
of each row's own table (tests/seqbias_ref.py) and with the single-table kernel (wmdbg_seqbias_state) run with that table.

The tables, histories and row checks are those of test_seqbias_kernel_gpu.py: the pool here holds its tables of 0, 1, 7, 7 and
4096 entries (sequence lengths 1 .. 32) side by side."""
import ctypes
import functools

import numpy as np
import pytest

import repeat_ref as RR
import seqbias_ref as SB
import seqbias_rows_ref as SR
import test_seqbias_kernel_gpu as SK
from test_decode_step_kernels_gpu import P, bits, err_msg

pytestmark = pytest.mark.gpu

vp, ip = ctypes.c_void_p, ctypes.c_int
CAP, EOTS = SK.CAP, SK.EOTS
NAMES = ["empty", "one", "seven", "deep", "ctx7"]          # table t of the pool: 0, 1, 7, 4096 and 7 entries


@pytest.fixture(scope="module")
def dbg(pkg):
    c = pkg.binding.Context(debug=True)
    c.lib.wmdbg_seqbias_state.argtypes = [vp, vp] + [ip] * 5 + [vp] * 4 + [ip, ctypes.c_int32] + [vp] * 6
    c.lib.wmdbg_seqbias_rows_state.argtypes = [vp, vp] + [ip] * 5 + [vp] * 5 + [ip, ctypes.c_int32] + [vp] * 8
    yield c
    c.close()


def table(V, name):
    return ([], []) if name == "empty" else SK.table(V, name)


@functools.lru_cache(maxsize=None)
def want_state(V, name, h, k):
    """what the single-table restatement leaves for history h[:k] under the named table; no table (None): nothing"""
    if name is None or name == "empty":
        return SB.state([], SK.hist(V, h, k), V)
    return SK.want_state(V, name, h, k)


def rows_call(dbg, seq, pos, n_prompt, V, names, rows, ban_in=None):
    """wmdbg_seqbias_rows_state with the named tables as the pool and `rows` (indices into names, -1) as the row map"""
    n_ctx, B = seq.shape
    words = RR.words_of(V)
    tabs = [table(V, n) + (None,) for n in names]
    toks, offs, bs, fl, toffs = SR.pack_tables(tabs)
    hit, ban = np.zeros((B, words), np.uint32), np.zeros((B, words), np.uint32)
    cnt, ids, tot = np.zeros(B, np.int32), np.zeros((B, CAP), np.int32), np.zeros((B, CAP), np.float32)
    woff = np.zeros((B, words), np.int32)
    rows = np.ascontiguousarray(rows, np.int32)
    rc = dbg.lib.wmdbg_seqbias_rows_state(dbg.handle, P(np.ascontiguousarray(seq, np.int32)), B, n_ctx, pos, n_prompt, V, P(toks), P(offs),
                                          P(bs), P(fl), P(toffs), len(names), EOTS[V], P(rows),
                                          None if ban_in is None else P(np.ascontiguousarray(ban_in, np.uint32)), P(hit), P(ban), P(cnt),
                                          P(ids), P(tot), P(woff))
    assert rc == 0, err_msg(dbg)
    return hit, ban, cnt, ids, tot, woff


def row_maps(B):
    """every row on another table (as far as there are tables), two rows on one table, rows without a table"""
    n = len(NAMES)
    a = [(b + 1) % n for b in range(B)]                     # consecutive rows on different tables; B = 5: every table once
    b_ = [3 if b % 4 < 2 else (-1 if b % 4 == 2 else 2) for b in range(B)]   # rows 0 and 1 on `deep`, then -1, then `seven`
    c = [-1 if b % 3 == 0 else b % n for b in range(B)]
    return [a, b_, c] if B > 1 else [[3], [-1], [0], [2]]


@pytest.mark.parametrize("V", [1024, 51865])
@pytest.mark.parametrize("B", [1, 5, 128])
def test_rows_state_kernel_is_the_single_table_kernel_per_row(dbg, B, V):
    """Every row's hit, ban and offset words, its count and every list element equal the restatement of the ROW'S table, and
    equal, bit for bit, the single-table hook run with that table on the same histories -- for every row map of row_maps, at k
    in {434, 31, 1, 0} generated tokens in that order on one context (a shorter history after a longer one: a stale word or list
    element would show, and so would one the kernel does not write -- the hooks pre-fill with 0xff)."""
    hs = [(b * 3 + B) % 8 for b in range(B)]
    for k in (434, 31, 1, 0):
        seq = SK.seq_for(V, hs, k)
        single = {}
        for rows in row_maps(B):
            got = rows_call(dbg, seq, k, 1, V, NAMES, rows)
            for b in range(B):
                name = None if rows[b] < 0 else NAMES[rows[b]]
                SK.check_row(got, b, want_state(V, name, hs[b], k), (k, rows[b], b, hs[b]))
                if name is None:
                    continue
                if name not in single:                      # the existing kernel with this table as THE table, all rows
                    s_, b_ = table(V, name)
                    single[name] = (SK.state_call(dbg, seq, k, 1, V, s_, b_) if s_ else
                                    empty_single(dbg, seq, k, V))
                one = single[name]
                n = int(got[2][b])
                assert n == int(one[2][b]), (k, name, b)
                for i in (0, 1, 5):                         # hit, ban, woff words
                    assert np.array_equal(got[i][b], one[i][b]), (k, name, b, i)
                assert np.array_equal(got[3][b, :n], one[3][b, :n]) and np.array_equal(bits(got[4][b, :n]), bits(one[4][b, :n])), (k, name, b)


def empty_single(dbg, seq, pos, V):
    n_ctx, B = seq.shape
    words = RR.words_of(V)
    out = (np.zeros((B, words), np.uint32), np.zeros((B, words), np.uint32), np.zeros(B, np.int32), np.zeros((B, CAP), np.int32),
           np.zeros((B, CAP), np.float32), np.zeros((B, words), np.int32))
    rc = dbg.lib.wmdbg_seqbias_state(dbg.handle, P(np.ascontiguousarray(seq, np.int32)), B, n_ctx, pos, 1, V, None, None, None, None, 0, EOTS[V],
                                     *[P(a) for a in out])
    assert rc == 0, err_msg(dbg)
    return out


@pytest.mark.parametrize("V", [1024, 51865])
def test_a_row_without_a_table_leaves_its_ban_words_alone(dbg, V):
    """The ban words are pre-filled with a pattern and NO wm_repeat_state runs: a row on -1 or on the empty table keeps every
    word as it was (and gets an all-zero hit row, count 0); a row with a table keeps the pattern OR-ed with its table's bans --
    nothing else.  A hot row that matches all 4096 entries of `deep` sits next to a row that matches nothing of `ctx7`."""
    B, k = 6, 434
    hs = [0, 2, 0, 1, 2, 0]                                 # hot, random, hot, cold, random, hot
    rows = [3, 4, -1, 0, -1, 2]                             # deep, ctx7, none, empty, none, seven
    words = RR.words_of(V)
    rng = np.random.default_rng(V)
    pattern = rng.integers(0, 2 ** 32, (B, words), dtype=np.uint64).astype(np.uint32)
    got = rows_call(dbg, SK.seq_for(V, hs, k), k, 1, V, NAMES, rows, ban_in=pattern)
    hit, ban, cnt, ids, tot, woff = got
    for b in range(B):
        name = None if rows[b] < 0 else NAMES[rows[b]]
        wh, wb, wi, wt, wo = want_state(V, name, hs[b], k)
        assert np.array_equal(hit[b], wh) and np.array_equal(woff[b], wo) and cnt[b] == wi.size, b
        assert np.array_equal(ban[b], pattern[b] | wb), b
        assert np.array_equal(ids[b, :wi.size], wi) and np.array_equal(bits(tot[b, :wi.size]), bits(wt)), b
        assert np.all(ids[b, wi.size:] == -1), b
        if name in (None, "empty"):
            assert not hit[b].any() and not woff[b].any() and cnt[b] == 0 and np.array_equal(ban[b], pattern[b]), b
    # conditions on the inputs: the hot row matches every entry of its table, its neighbour none of its own
    deep = SB.expand(*SK.table(V, "deep"), eot=EOTS[V], V=V)
    assert len(deep) == CAP and all(SB.matches(s, SK.hist(V, 0, k)) for s, _ in deep) and cnt[0] == 128
    assert cnt[1] == 0 and not hit[1].any() and want_state(V, "seven", 0, k)[1].any()


def test_a_table_of_4096_groups_behind_another_table(dbg):
    """`wide` at 51 865 ids has 4096 distinct last tokens, so 4096 GROUPS (`deep` has 128): behind `seven` in the pool its rows
    walk g = g0 + gl with g0 = 5 and gl up to 4095 -- four rounds of the 1024 lanes in the match pass and in the list pass --,
    and the hot row's list fills all 4096 places.  Every row against the restatement of its table and, bit for bit, against the
    single-table hook; the tables on either side (`seven` in front, `one` behind) must not leak into it."""
    V, k = 51865, 434
    names, rows, hs = ["seven", "wide", "one"], [1, 0, 1, -1, 2, 1], [0, 0, 2, 0, 0, 1]
    seq = SK.seq_for(V, hs, k)
    got = rows_call(dbg, seq, k, 1, V, names, rows)
    single = {n: SK.state_call(dbg, seq, k, 1, V, *SK.table(V, n)) for n in names}
    for b, r in enumerate(rows):
        name = None if r < 0 else names[r]
        SK.check_row(got, b, want_state(V, name, hs[b], k), (b, name))
        if name is None:
            continue
        one, n = single[name], int(got[2][b])
        assert n == int(one[2][b])
        for i in (0, 1, 5):
            assert np.array_equal(got[i][b], one[i][b]), (b, name, i)
        assert np.array_equal(got[3][b, :n], one[3][b, :n]) and np.array_equal(bits(got[4][b, :n]), bits(one[4][b, :n])), (b, name)
    # conditions on the inputs: 4096 groups behind 5 of `seven`, every one of them in the hot row's list, fewer in the others'
    pool = SR.pool(SR.expand_tables([SK.table(V, n) + (None,) for n in names], eot=EOTS[V], V=V))
    assert pool["tab_grp"].tolist()[:3] == [0, 5, 5 + CAP]
    assert got[2][0] == CAP and 1024 < got[2][2] < CAP and 1024 < got[2][5] < CAP


def test_the_hook_refuses_a_bad_map_or_table(dbg):
    V, B = 1024, 2
    seq = SK.seq_for(V, [0, 1], 5)
    words = RR.words_of(V)
    out = [np.zeros((B, words), np.uint32), np.zeros((B, words), np.uint32), np.zeros(B, np.int32), np.zeros((B, CAP), np.int32),
           np.zeros((B, CAP), np.float32), np.zeros((B, words), np.int32)]
    toks, offs, bs, fl, toffs = SR.pack_tables([([(1, 2)], [1.0], None), ([(3,)], [2.0], None)])

    def call(rows, toffs_=toffs, n_tables=2):
        rows = np.array(rows, np.int32)
        return dbg.lib.wmdbg_seqbias_rows_state(dbg.handle, P(seq), B, seq.shape[0], 5, 1, V, P(toks), P(offs), P(bs), None, P(toffs_),
                                                n_tables, EOTS[V], P(rows), None, *[P(a) for a in out])
    assert call([0, 1]) == 0 and call([-1, -1]) == 0
    assert call([0, 2]) == 1 and call([-2, 0]) == 1                                   # WM_ERR_INVALID: outside [-1, n_tables)
    assert call([0, 1], np.array([0, 2, 1], np.int32)) == 1                           # table_offsets that decrease
    assert call([0, -1], np.array([0, 2, 2], np.int32)) == 0                          # both sequences in table 0, table 1 empty
    assert call([0, 0], np.array([1, 1, 2], np.int32)) == 1                           # ... that do not start at 0
