// vad_segments.cpp -- speech segments from a smoothed energy track (wm_vad_energy's energy_out): host only, no context,
// no GPU.  Adaptive thresholds from two quantiles of the track, then the hysteresis scan of Silero
// VAD's get_speech_timestamps on the track, padding and merging.  All arithmetic in double on the f32 inputs.
#include <math.h>

#include <algorithm>
#include <vector>

#include "wm_internal.h"

extern "C" void wm_vad_default_params(wm_vad_params *p) {
    if (!p) return;
    p->q_floor = 0.10f;
    p->q_peak = 0.95f;
    p->min_range = 0.6f;
    p->on_frac = 0.5f;
    p->off_frac = 0.35f;
    p->min_speech = 25;
    p->min_silence = 50;
    p->speech_pad = 40;
}

extern "C" int wm_vad_segments(const float *y, int64_t n, const wm_vad_params *p, int32_t *segments, int cap, int *n_segments,
                               float stats[4]) try {
    WM_REQUIRE(p && n_segments, WM_ERR_INVALID, "vad_segments: null params / n_segments");
    WM_REQUIRE(n >= 0 && n <= INT32_MAX, WM_ERR_INVALID, "vad_segments: n must be 0 .. 2^31 - 1, got %lld", (long long)n);
    WM_REQUIRE(cap >= 0 && (cap == 0 || segments), WM_ERR_INVALID, "vad_segments: cap %d with null segments", cap);
    WM_REQUIRE(n == 0 || y, WM_ERR_INVALID, "vad_segments: null track");
    WM_REQUIRE(p->q_floor >= 0.f && p->q_floor < p->q_peak && p->q_peak <= 1.f, WM_ERR_INVALID,
               "vad_segments: quantiles must be 0 <= q_floor < q_peak <= 1");
    WM_REQUIRE(p->off_frac >= 0.f && p->off_frac <= p->on_frac && p->on_frac <= 1.f && p->on_frac > 0.f, WM_ERR_INVALID,
               "vad_segments: fractions must be 0 <= off_frac <= on_frac <= 1, on_frac > 0");
    WM_REQUIRE(std::isfinite(p->min_range) && p->min_range >= 0.f, WM_ERR_INVALID, "vad_segments: min_range must be finite and >= 0");
    WM_REQUIRE(p->min_silence >= 1 && p->min_speech >= 0 && p->speech_pad >= 0, WM_ERR_INVALID,
               "vad_segments: min_silence >= 1, min_speech >= 0, speech_pad >= 0");
    for (int64_t t = 0; t < n; ++t) WM_REQUIRE(!std::isnan(y[t]), WM_ERR_INVALID, "vad_segments: NaN at frame %lld", (long long)t);
    *n_segments = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = NAN;
    if (n == 0) return WM_OK;
    std::vector<float> s(y, y + n);
    std::sort(s.begin(), s.end());
    const double floor_ = (double)s[(size_t)((double)p->q_floor * (double)(n - 1))];
    const double peak = (double)s[(size_t)((double)p->q_peak * (double)(n - 1))];
    if (stats) {
        stats[0] = (float)floor_;
        stats[1] = (float)peak;
    }
    std::vector<std::pair<int64_t, int64_t>> seg;
    if (peak - floor_ < (double)p->min_range) {   // no contrast: never drop audio
        seg.emplace_back(0, n);
    } else {
        const double thr_on = floor_ + (double)p->on_frac * (peak - floor_), thr_off = floor_ + (double)p->off_frac * (peak - floor_);
        if (stats) {
            stats[2] = (float)thr_on;
            stats[3] = (float)thr_off;
        }
        std::vector<std::pair<int64_t, int64_t>> raw;
        bool trig = false;
        int64_t pend = -1, start = 0;
        for (int64_t t = 0; t < n; ++t) {
            const double v = (double)y[t];
            if (v >= thr_on) pend = -1;
            if (!trig && v >= thr_on) {
                trig = true;
                start = t;
            } else if (trig && v < thr_off) {
                if (pend < 0) pend = t;
                if (t + 1 - pend >= p->min_silence) {
                    if (pend - start >= p->min_speech) raw.emplace_back(start, pend);
                    trig = false;
                    pend = -1;
                }
            }
        }
        if (trig && n - start >= p->min_speech) raw.emplace_back(start, n);
        const int64_t pad = p->speech_pad / 2;   // speech_pad frames over both sides
        for (auto &g : raw) {
            const int64_t a = std::max<int64_t>(0, g.first - pad), b = std::min<int64_t>(n, g.second + pad);
            if (!seg.empty() && a <= seg.back().second) seg.back().second = std::max(seg.back().second, b);
            else seg.emplace_back(a, b);
        }
    }
    *n_segments = (int)seg.size();
    for (size_t k = 0; k < seg.size() && k < (size_t)cap; ++k) {
        segments[2 * k] = (int32_t)seg[k].first;
        segments[2 * k + 1] = (int32_t)seg[k].second;
    }
    return WM_OK;
} WM_API_CATCH
