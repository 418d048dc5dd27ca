// constraint_table.cpp -- the constraint's automaton on the host (wm_set_constraint): the checks of the
// header, and the packing wm_constraint_state walks -- the flat arrays as given (accept widened to a word per state) and an
// open-addressing hash of the explicit edges, key = state << 20 | token, linear probing, WM_CST_HASH_SLOTS slots for at most
// WM_MAX_CST_EDGES edges: the table is at most half full whatever the automaton.  Pure host code: nothing here touches the device.
#include "model.h"

int wm_cst_build(const int32_t *edge_beg, const int32_t *edge_tok, const int32_t *edge_next, const int32_t *def_next,
                 const uint8_t *accept, int n_states, int32_t eot, int n_vocab, WmCstTable *out) {
    *out = WmCstTable();
    WM_REQUIRE(n_states >= 0 && n_states <= WM_MAX_CST_STATES, WM_ERR_INVALID, "constraint: %d states (0 .. %d)", n_states, WM_MAX_CST_STATES);
    if (n_states == 0) return WM_OK;
    WM_REQUIRE(eot >= 0 && eot < n_vocab, WM_ERR_INVALID, "constraint: eot %d outside [0, %d)", eot, n_vocab);
    // (strictly below: no key is the empty slot's -1)
    WM_REQUIRE(eot < (1 << WM_CST_TOK_BITS), WM_ERR_INVALID, "constraint: eot %d does not fit the edge keys' %d token bits", eot, WM_CST_TOK_BITS);
    WM_REQUIRE(edge_beg && def_next && accept, WM_ERR_INVALID, "constraint: null pointer");
    WM_REQUIRE(edge_beg[0] == 0, WM_ERR_INVALID, "constraint: edge_beg[0] must be 0");
    for (int s = 0; s < n_states; ++s) {
        WM_REQUIRE(edge_beg[s + 1] >= edge_beg[s], WM_ERR_INVALID, "constraint: edge_beg decreases at state %d", s);
        WM_REQUIRE(edge_beg[s + 1] <= WM_MAX_CST_EDGES, WM_ERR_INVALID, "constraint: more than %d edges", WM_MAX_CST_EDGES);
    }
    const int E = edge_beg[n_states];
    WM_REQUIRE(E == 0 || (edge_tok && edge_next), WM_ERR_INVALID, "constraint: null pointer");
    for (int s = 0; s < n_states; ++s) {
        WM_REQUIRE(def_next[s] >= -1 && def_next[s] < n_states, WM_ERR_INVALID, "constraint: def_next %d of state %d outside [-1, %d)",
                   def_next[s], s, n_states);
        bool allows = def_next[s] >= 0;
        for (int e = edge_beg[s]; e < edge_beg[s + 1]; ++e) {
            WM_REQUIRE(edge_tok[e] >= 0 && edge_tok[e] < eot, WM_ERR_INVALID, "constraint: edge token %d of state %d is not a text id (< %d)",
                       edge_tok[e], s, eot);
            WM_REQUIRE(e == edge_beg[s] || edge_tok[e] > edge_tok[e - 1], WM_ERR_INVALID,
                       "constraint: the edge tokens of state %d are not strictly ascending", s);
            WM_REQUIRE(edge_next[e] >= -1 && edge_next[e] < n_states, WM_ERR_INVALID, "constraint: edge target %d of state %d outside [-1, %d)",
                       edge_next[e], s, n_states);
            WM_REQUIRE(edge_next[e] >= 0 || def_next[s] >= 0, WM_ERR_INVALID,
                       "constraint: state %d forbids id %d explicitly, which needs a default (def_next >= 0)", s, edge_tok[e]);
            allows = allows || edge_next[e] >= 0;
        }
        WM_REQUIRE(allows || accept[s], WM_ERR_INVALID, "constraint: state %d is stuck: no allowing edge, no default and not accepting", s);
    }
    WmCstTable t;
    t.eot = eot;
    t.edge_beg.assign(edge_beg, edge_beg + n_states + 1);
    if (E) {
        t.edge_tok.assign(edge_tok, edge_tok + E);
        t.edge_next.assign(edge_next, edge_next + E);
    }
    t.def_next.assign(def_next, def_next + n_states);
    t.accept.resize(n_states);
    for (int s = 0; s < n_states; ++s) t.accept[s] = accept[s] ? 1 : 0;
    t.hash.assign((size_t)2 * WM_CST_HASH_SLOTS, -1);
    for (int s = 0; s < n_states; ++s)
        for (int e = edge_beg[s]; e < edge_beg[s + 1]; ++e) {
            const unsigned key = wm_cst_key(s, edge_tok[e]);
            unsigned at = wm_cst_slot(key);
            while (t.hash[2 * (size_t)at] != -1) at = (at + 1) & (WM_CST_HASH_SLOTS - 1);   // (E <= half the slots: an empty one exists)
            t.hash[2 * (size_t)at] = (int32_t)key;
            t.hash[2 * (size_t)at + 1] = edge_next[e];
        }
    *out = std::move(t);
    return WM_OK;
}
