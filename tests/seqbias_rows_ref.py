"""numpy restatement of the row tables (wm_set_sequence_bias_tables / wm_set_bias_rows), on top of
tests/seqbias_ref.py: a context holds a LIST of tables, every table is checked and expanded on its own, and a row of a call uses
the table its row map names (-1: none) exactly as the single table of seqbias_ref.

The pooled layout the library uploads: the expanded tables, each sorted STABLY by last token (entries with one last token form a
group in table order, groups ascend by id), concatenated; grp_beg is absolute into the pool's entries and one array of
n_groups + 1 serves all tables; table t is groups [tab_grp[t], tab_grp[t + 1])."""
import numpy as np

import seqbias_ref as SB

MAX_TABLES, MAX_POOL, CTX = 1024, 65536, SB.MAX_LEN - 1


def expand_tables(tables, *, eot, V):
    """tables: [(seqs, biases, boost or None)] -> the expanded tables in table order; Invalid as the library answers it"""
    if len(tables) > MAX_TABLES:
        raise SB.Invalid("%d tables" % len(tables))
    out = [SB.expand(s, b, f, eot=eot, V=V) for s, b, f in tables]
    if sum(len(t) for t in out) > MAX_POOL:
        raise SB.Invalid("pool")
    return out


def pool(expanded):
    """The pooled arrays of expanded tables: dict(tab_grp, grp_id, grp_beg, ent_len, ent_bias, ent_ctx [entries][31])"""
    tab_grp, grp_id, grp_beg, ent_len, ent_bias, ent_ctx = [0], [], [0], [], [], []
    for t in expanded:
        last = None                                                       # a table's first entry always opens a group
        for s, b in sorted(t, key=lambda e: e[0][-1]):                    # stable: table order within an id
            if s[-1] != last:
                if last is not None:
                    grp_beg.append(len(ent_len))                          # the end of the group before = the start of this one
                grp_id.append(s[-1])
                last = s[-1]
            ent_len.append(len(s) - 1)
            ent_bias.append(b)
            ent_ctx.append(list(reversed(s[:-1])) + [0] * (CTX - len(s) + 1))
        if last is not None:
            grp_beg.append(len(ent_len))                                  # ... and of the table's last group = the next table's start
        tab_grp.append(len(grp_id))
    return dict(tab_grp=np.array(tab_grp, np.int32), grp_id=np.array(grp_id, np.int32), grp_beg=np.array(grp_beg, np.int32),
                ent_len=np.array(ent_len, np.int32), ent_bias=np.array(ent_bias, np.float32),
                ent_ctx=np.array(ent_ctx, np.int32).reshape(-1, CTX))


def pack_tables(tables):
    """The arrays of the C call: SB.pack of all sequences back to back, plus table_offsets i32 [n_tables + 1]"""
    seqs = [s for t in tables for s in t[0]]
    bias = [b for t in tables for b in t[1]]
    any_boost = any(t[2] is not None for t in tables)
    boost = [f for t in tables for f in (t[2] if t[2] is not None else [False] * len(t[0]))] if any_boost else None
    toks, offs, bs, fl = SB.pack(seqs, bias, boost)
    toffs = np.zeros(len(tables) + 1, np.int32)
    toffs[1:] = np.cumsum([len(t[0]) for t in tables])
    return toks, offs, bs, fl, toffs


def row_ranges(table_of_row, tab_grp, b0, Cg, N):
    """[Cg * N][2] (first group, end group) of the decoder rows of the group of windows [b0, b0 + Cg) x N candidates"""
    out = np.zeros((Cg * N, 2), np.int32)
    for b in range(Cg * N):
        t = int(table_of_row[b0 + b // N])
        if t >= 0:
            out[b] = (tab_grp[t], tab_grp[t + 1])
    return out
