// given_panel_sanitize_main.cpp -- a stand-alone driver of the given-panel plan (wm_given_panel_plan, csrc/tx_plan.cpp: which
// decode groups wm_set_given_panel serves, and the phase's width, length and rounds) over the product of
// tests/test_given_panel_cpu.py and seeded large groups, for a host-sanitizer build.  CPU only: it links csrc/tx_plan.cpp alone
// (no HIP call is made) and needs no GPU and no preloaded runtime:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I include -I openai-whisper-coreml_amd/csrc -Xarch_host \
//         -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -x hip tools/given_panel_sanitize_main.cpp \
//         openai-whisper-coreml_amd/csrc/tx_plan.cpp -o /tmp/given_panel_sanitize && /tmp/given_panel_sanitize
//
// Every plan is compared with the definition, tried candidate by candidate: Lp is the largest L <= max_new with
// P + L - 1 < n_text_ctx such that every row is given or finished at every index of [1, L).  The arrays are sized exactly, so the
// sanitizers turn any read past a group's rows into a failure.  Prints the counts, exits 0.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "tx_plan.h"

namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 11);
}

const unsigned kServed = WM_GPB_GIVEN | WM_GPB_X;

int phase_by_definition(int G, const int32_t *lens, const int32_t *bud, int max_new, int P, int n_ctx) {
    int L = 0;
    for (int cand = 1; cand <= std::min(max_new, n_ctx - P); ++cand) {
        bool ok = true;
        for (int r = 0; r < G && ok; ++r) {
            const int fin = bud ? std::min(bud[r], max_new) : max_new;
            for (int gi = 1; gi < cand && ok; ++gi) ok = gi < lens[r] || gi >= fin;
        }
        if (ok) L = cand;
    }
    return L;
}

long g_served = 0, g_unserved = 0;
bool check(int G, int width, const std::vector<int32_t> &lens, const std::vector<int32_t> *bud, int max_new, int P, int n_ctx,
           unsigned bits) {
    WmGivenPanelPlan pl;
    wm_given_panel_plan(G, width, lens.data(), bud ? bud->data() : nullptr, max_new, P, n_ctx, bits, &pl);
    if (pl.reason < 0 || pl.reason >= WM_GP_REASONS) return false;
    if (bits != kServed || width <= 1) {
        if (pl.reason == WM_GP_SERVED) return false;
        ++g_unserved;
        return pl.rounds == 0;
    }
    const int w = std::min(std::min(width, WM_PANEL_MAX_WIDTH), WM_DEC_MAXB / G);
    if (w < 2) { ++g_unserved; return pl.reason == WM_GP_NARROW && pl.rounds == 0; }
    const int L = phase_by_definition(G, lens.data(), bud ? bud->data() : nullptr, max_new, P, n_ctx);
    if (pl.w != w || pl.Lp != L) return false;
    if (L <= 1) { ++g_unserved; return pl.reason == WM_GP_NO_PHASE && pl.rounds == 0; }
    ++g_served;
    return pl.reason == WM_GP_SERVED && pl.rounds == (L - 1 + w - 1) / w && w * G <= WM_DEC_MAXB;
}
}  // namespace

int main() {
    // the product: G <= 3, lens 0 .. 5, budgets 1 .. 5 (and none), max_new <= 5, width <= 4, a roomy and a short context
    for (int G = 1; G <= 3; ++G) {
        int n_l = 1, n_b = 1;
        for (int i = 0; i < G; ++i) { n_l *= 6; n_b *= 5; }
        for (int li = 0; li < n_l; ++li)
            for (int bi = -1; bi < n_b; ++bi) {
                std::vector<int32_t> lens(G), bud(G);
                for (int r = 0, a = li, c = bi < 0 ? 0 : bi; r < G; ++r, a /= 6, c /= 5) { lens[r] = a % 6; bud[r] = 1 + c % 5; }
                for (int max_new = 1; max_new <= 5; ++max_new)
                    for (int width = 1; width <= 4; ++width)
                        for (int n_ctx : {64, 6})
                            if (!check(G, width, lens, bi < 0 ? nullptr : &bud, max_new, 3, n_ctx, kServed)) {
                                fprintf(stderr, "plan differs: G %d lens %d budgets %d max_new %d width %d n_ctx %d\n", G, li, bi, max_new, width, n_ctx);
                                return 1;
                            }
            }
    }
    // seeded groups up to 128 rows and width 8, every mode bit
    for (int i = 0; i < 20000; ++i) {
        const int G = 1 + rnd() % 128, width = 1 + rnd() % 8, max_new = 1 + rnd() % 40, P = 1 + rnd() % 20;
        const int n_ctx = rnd() % 5 == 0 ? P + 1 + (int)(rnd() % 12) : 448;
        std::vector<int32_t> lens(G), bud(G);
        const bool full = rnd() % 2;
        for (int r = 0; r < G; ++r) { lens[r] = full ? max_new : (int)(rnd() % (max_new + 1)); bud[r] = 1 + rnd() % 40; }
        unsigned bits = kServed;
        if (rnd() % 3 == 0) bits ^= 1u << (rnd() % 14);
        if (!check(G, width, lens, rnd() % 2 ? &bud : nullptr, max_new, P, n_ctx, bits)) {
            fprintf(stderr, "plan differs: seeded case %d (G %d width %d max_new %d bits %x)\n", i, G, width, max_new, bits);
            return 1;
        }
    }
    printf("given-panel plans: %ld served, %ld not served, all as the definition says\n", g_served, g_unserved);
    return 0;
}
