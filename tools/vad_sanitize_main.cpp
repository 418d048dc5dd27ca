// vad_sanitize_main.cpp -- a stand-alone driver of wm_vad_segments (csrc/vad_segments.cpp) for a host-sanitizer build.  CPU
// only: it links csrc/vad_segments.cpp alone (no HIP call is made) and needs no GPU and no preloaded runtime:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I include -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all -x hip tools/vad_sanitize_main.cpp \
//         openai-whisper-coreml_amd/csrc/vad_segments.cpp -o /tmp/vad_sanitize && /tmp/vad_sanitize
//
// Tracks and buffers are heap blocks of exactly the size the call is told, so that the sanitizers turn any byte read or
// written past them into a failure; every call must come back with a status, and every valid call's spans must be ordered,
// disjoint and inside [0, n).  Prints the number of calls and exits 0.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "whisper_mi355x.h"

void wm_set_error(const char *, ...) {}   // vad_segments.cpp's only dependency on the rest of the library

namespace {
int fail(const char *what, long call) {
    fprintf(stderr, "vad_sanitize: %s (call %ld)\n", what, call);
    return 1;
}
}  // namespace

int main() {
    std::mt19937_64 rng(12345);
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    auto pick = [&](int a, int b) { return (int)std::uniform_int_distribution<int>(a, b)(rng); };
    long calls = 0, valid = 0, invalid = 0;
    for (int it = 0; it < 20000; ++it) {
        const int64_t n = it % 7 == 0 ? pick(0, 3) : pick(0, 700);
        // exactly n floats on the heap
        float *y = (float *)malloc(n ? (size_t)n * sizeof(float) : 1);
        double level = 0.0;
        bool high = false;
        for (int64_t t = 0; t < n; ++t) {
            if (pick(0, 40) == 0) high = !high;
            level = it % 3 == 0 ? level + uni(-0.3, 0.3) : (high ? 5.0 : 0.0) + uni(-0.4, 0.4);
            y[t] = (float)level;
        }
        if (n && it % 11 == 0) y[pick(0, (int)n - 1)] = it % 22 == 0 ? INFINITY : -INFINITY;
        const bool nan = n && it % 13 == 0;
        if (nan) y[pick(0, (int)n - 1)] = NAN;
        wm_vad_params p;
        wm_vad_default_params(&p);
        bool bad = false;
        if (it % 2) {
            p.q_floor = (float)uni(0.0, 0.5);
            p.q_peak = (float)uni(0.5, 1.0);
            p.min_range = (float)uni(0.0, 3.0);
            p.on_frac = (float)uni(0.01, 1.0);
            p.off_frac = p.on_frac * (float)uni(0.0, 1.0);
            p.min_speech = pick(0, 60);
            p.min_silence = pick(1, 80);
            p.speech_pad = pick(0, 100);
            if (p.q_floor >= p.q_peak) bad = true;
        }
        if (it % 17 == 0) {   // one field out of its range
            bad = true;
            switch (pick(0, 7)) {
                case 0: p.q_floor = -0.5f; break;
                case 1: p.q_peak = 1.5f; break;
                case 2: p.min_range = it % 34 ? -1.f : NAN; break;
                case 3: p.on_frac = 0.f; p.off_frac = 0.f; break;
                case 4: p.off_frac = p.on_frac + 0.1f; break;
                case 5: p.min_silence = 0; break;
                case 6: p.min_speech = -1; break;
                default: p.speech_pad = INT32_MIN; break;
            }
        }
        int need = -1;
        int st = wm_vad_segments(y, n, &p, nullptr, 0, &need, nullptr);   // the sizing call
        ++calls;
        if (bad || nan) {
            if (st != WM_ERR_INVALID) return fail("an invalid call was accepted", calls);
            ++invalid;
            free(y);
            continue;
        }
        if (st != WM_OK || need < 0) return fail("a valid call was rejected", calls);
        // exactly `cap` pairs on the heap: the count needed, one fewer, or one
        const int cap = it % 5 == 0 ? (need > 0 ? need - 1 : 0) : (it % 5 == 1 ? 1 : need);
        int32_t *seg = (int32_t *)malloc(cap ? (size_t)cap * 2 * sizeof(int32_t) : 1);
        float *stats = (float *)malloc(4 * sizeof(float));
        int got = -1;
        st = wm_vad_segments(y, n, &p, cap ? seg : nullptr, cap, &got, it % 4 ? stats : nullptr);
        ++calls;
        if (st != WM_OK || got != need) return fail("the second call disagrees with the sizing call", calls);
        int64_t last = -1;
        for (int k = 0; k < (cap < got ? cap : got); ++k) {
            if (!(seg[2 * k] > last || (k == 0 && seg[0] == 0)) || seg[2 * k] >= seg[2 * k + 1] || seg[2 * k + 1] > n)
                return fail("spans out of order or outside [0, n)", calls);
            last = seg[2 * k + 1];
        }
        ++valid;
        free(stats);
        free(seg);
        free(y);
    }
    // null pointers and sizes that cannot be
    wm_vad_params p;
    wm_vad_default_params(&p);
    wm_vad_default_params(nullptr);
    float one = 1.f;
    int n_seg = 0;
    int32_t pair[2];
    if (wm_vad_segments(nullptr, 5, &p, pair, 1, &n_seg, nullptr) != WM_ERR_INVALID) return fail("null track", calls);
    if (wm_vad_segments(&one, 1, nullptr, pair, 1, &n_seg, nullptr) != WM_ERR_INVALID) return fail("null params", calls);
    if (wm_vad_segments(&one, 1, &p, nullptr, 1, &n_seg, nullptr) != WM_ERR_INVALID) return fail("null segments", calls);
    if (wm_vad_segments(&one, 1, &p, pair, 1, nullptr, nullptr) != WM_ERR_INVALID) return fail("null count", calls);
    if (wm_vad_segments(&one, -1, &p, pair, 1, &n_seg, nullptr) != WM_ERR_INVALID) return fail("negative n", calls);
    if (wm_vad_segments(&one, (int64_t)1 << 40, &p, pair, 1, &n_seg, nullptr) != WM_ERR_INVALID) return fail("huge n", calls);
    if (wm_vad_segments(&one, 1, &p, pair, -1, &n_seg, nullptr) != WM_ERR_INVALID) return fail("negative cap", calls);
    if (wm_vad_segments(&one, 1, &p, pair, 1, &n_seg, nullptr) != WM_OK || n_seg != 1 || pair[0] != 0 || pair[1] != 1)
        return fail("one frame is one flat segment", calls);
    printf("vad_sanitize: %ld calls (%ld valid pairs of calls, %ld rejected), no finding\n", calls + 8, valid, invalid);
    return 0;
}
