// constraint_sanitize_main.cpp -- a stand-alone driver of the constraint's host side (wm_cst_build, csrc/constraint_table.cpp:
// validation of an automaton and the packing of its (state, token) hash) over valid, malformed and random tables, for a
// host-sanitizer build.  CPU only: it links csrc/constraint_table.cpp alone (no HIP call is made) and needs no GPU and no
// preloaded runtime:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I include -I openai-whisper-coreml_amd/csrc -Xarch_host \
//         -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -x hip tools/constraint_sanitize_main.cpp \
//         openai-whisper-coreml_amd/csrc/constraint_table.cpp -o /tmp/constraint_sanitize && /tmp/constraint_sanitize
//
// Every table must come back with a status; a table that is accepted must be found again, edge by edge, through the hash the
// way the kernel probes it.  The sanitizers turn any out-of-bounds access or overflow into a failure.  Prints the counts, exits 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "model.h"

void wm_set_error(const char *, ...) {}   // constraint_table.cpp's only dependency on the rest of the library

namespace {
struct Table {
    std::vector<int32_t> beg, tok, nxt, dn;
    std::vector<uint8_t> acc;
    int32_t eot;
};

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 11);
}

// a random VALID automaton: every state has a default or accepts, tokens ascending
Table random_valid(int S, int max_fan, int eot) {
    Table t;
    t.eot = eot;
    t.beg.push_back(0);
    for (int s = 0; s < S; ++s) {
        const bool def = rnd() % 3 == 0;
        t.dn.push_back(def ? (int32_t)(rnd() % S) : -1);
        t.acc.push_back(def ? rnd() % 2 : 1);
        int fan = rnd() % (max_fan + 1), tokv = -1;
        for (int e = 0; e < fan; ++e) {
            tokv += 1 + rnd() % 5;
            if (tokv >= eot) break;
            t.tok.push_back(tokv);
            t.nxt.push_back(def && rnd() % 4 == 0 ? -1 : (int32_t)(rnd() % S));
        }
        t.beg.push_back((int32_t)t.tok.size());
    }
    return t;
}

int build(const Table &t, int n_vocab, WmCstTable *out) {
    return wm_cst_build(t.beg.data(), t.tok.empty() ? nullptr : t.tok.data(), t.nxt.empty() ? nullptr : t.nxt.data(), t.dn.data(),
                        t.acc.data(), (int)t.dn.size(), t.eot, n_vocab, out);
}

// the kernel's probe
int lookup(const WmCstTable &c, int s, int t) {
    const unsigned key = wm_cst_key(s, t);
    unsigned at = wm_cst_slot(key);
    for (int probe = 0; probe < WM_CST_HASH_SLOTS; ++probe) {
        if ((unsigned)c.hash[2 * (size_t)at] == key) return c.hash[2 * (size_t)at + 1];
        if (c.hash[2 * (size_t)at] == -1) return c.def_next[s];
        at = (at + 1) & (WM_CST_HASH_SLOTS - 1);
    }
    return -2;
}
}  // namespace

int main() {
    int ok = 0, refused = 0;
    const int V = 51865, eot = 50257;
    for (int round = 0; round < 40; ++round) {
        const int S = 1 + rnd() % (round < 30 ? 200 : WM_MAX_CST_STATES), fan = round < 30 ? 40 : 15;
        Table t = random_valid(S, fan, eot);
        WmCstTable c;
        if (build(t, V, &c) != WM_OK) { fprintf(stderr, "a valid table was refused (round %d)\n", round); return 1; }
        ++ok;
        for (int s = 0; s < S; ++s) {
            for (int e = t.beg[s]; e < t.beg[s + 1]; ++e)
                if (lookup(c, s, t.tok[e]) != t.nxt[e]) { fprintf(stderr, "edge (%d, %d) lost in the hash\n", s, t.tok[e]); return 1; }
            const int miss = (int)(rnd() % eot);   // a token without an explicit edge takes the default
            bool has = false;
            for (int e = t.beg[s]; e < t.beg[s + 1]; ++e) has = has || t.tok[e] == miss;
            if (!has && lookup(c, s, miss) != t.dn[s]) { fprintf(stderr, "default of state %d lost\n", s); return 1; }
        }
        // one field of it damaged at a time: each must be refused, none may be read out of bounds
        for (int kind = 0; kind < 9; ++kind) {
            Table b = t;
            const int s = (int)(rnd() % S);
            switch (kind) {
            case 0: b.beg[0] = 1; break;
            case 1: if (S < 2) continue; b.beg[1 + rnd() % (S - 1)] = -5; break;
            case 2: b.beg[S] = WM_MAX_CST_EDGES + 1; break;
            case 3: b.dn[s] = S; break;
            case 4: b.dn[s] = -2; break;
            case 5: if (b.tok.empty()) continue; b.tok[rnd() % b.tok.size()] = eot; break;
            case 6: if (b.nxt.empty()) continue; b.nxt[rnd() % b.nxt.size()] = S + 3; break;
            case 7: b.eot = V; break;
            case 8: b.eot = -1; break;
            }
            WmCstTable d;
            if (build(b, V, &d) != WM_ERR_INVALID) { fprintf(stderr, "a damaged table (kind %d) was accepted\n", kind); return 1; }
            ++refused;
        }
    }
    {   // the limits: the largest automaton, all edges on one state and spread over all states
        Table t;
        t.eot = 1 << 19;
        t.beg.push_back(0);
        for (int e = 0; e < WM_MAX_CST_EDGES; ++e) { t.tok.push_back(e * 7); t.nxt.push_back(e % WM_MAX_CST_STATES); }
        t.beg.push_back(WM_MAX_CST_EDGES);
        for (int s = 1; s < WM_MAX_CST_STATES; ++s) t.beg.push_back(WM_MAX_CST_EDGES);
        t.dn.assign(WM_MAX_CST_STATES, -1);
        t.acc.assign(WM_MAX_CST_STATES, 1);
        WmCstTable c;
        if (build(t, 1 << 20, &c) != WM_OK) { fprintf(stderr, "the largest table was refused\n"); return 1; }
        for (int e = 0; e < WM_MAX_CST_EDGES; ++e)
            if (lookup(c, 0, t.tok[e]) != t.nxt[e]) { fprintf(stderr, "edge %d of the largest table lost\n", e); return 1; }
        ++ok;
        t.dn.push_back(-1); t.acc.push_back(1); t.beg.push_back(WM_MAX_CST_EDGES);   // one state too many
        if (build(t, 1 << 20, &c) != WM_ERR_INVALID) { fprintf(stderr, "4097 states were accepted\n"); return 1; }
        ++refused;
    }
    WmCstTable off;
    if (wm_cst_build(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, V, &off) != WM_OK || off.n_states() != 0) return 1;
    printf("constraint tables: %d accepted and found again through the hash, %d refused\n", ok, refused);
    return 0;
}
