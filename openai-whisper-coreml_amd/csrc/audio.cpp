// audio.cpp -- the step immediately BEFORE the hot path, behind the C ABI: a 16 kHz mono 16-bit
// RIFF/WAVE file in, independent 30 s windows out.  Host only, no GPU.
//
// The reference records 16 kHz mono LinearPCM to `query.wav` (Whisper/Whisper/AudioRecorder.swift:56-61), reads it back
// through AVFoundation (:74-86) and pads / truncates to ONE 30 s window (Whisper/Whisper/ContentView.swift:57-60).  A
// dlopen-only host has no AVFoundation: these functions give it the same input path, and apply the reference's pad rule
// per window so that a recording of any length becomes the list of chunks wm_transcribe_greedy shards over.
// (openai-whisper-coreml_amd/audio.py is the Python twin; tests pin one against the other.)
#include <stdio.h>
#include <string.h>

#include <vector>

#include "wm_internal.h"

struct wm_wav {
    std::vector<unsigned char> raw;  // the file image (kept as read: ONE copy of the recording, whatever its size)
    size_t data_off = 0;             // first byte of the data chunk
    size_t n_samples = 0;
};

namespace {
uint32_t rd32(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint16_t rd16(const unsigned char *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
constexpr size_t kMaxWavBytes = (size_t)1 << 32;  // 4 GiB: > 37 h of 16 kHz int16; RIFF cannot describe more anyway
}  // namespace

extern "C" int wm_wav_open(const char *path, wm_wav **out) try {
    WM_REQUIRE(path && out, WM_ERR_INVALID, "wav_open: null pointer");
    *out = nullptr;
    FILE *f = fopen(path, "rb");
    WM_REQUIRE(f, WM_ERR_IO, "cannot open '%s'", path);
    std::vector<unsigned char> buf;
    {
        unsigned char tmp[1 << 16];
        size_t n;
        while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) {
            if (buf.size() + n > kMaxWavBytes) { fclose(f); wm_set_error("'%s': larger than 4 GiB", path); return WM_ERR_IO; }
            buf.insert(buf.end(), tmp, tmp + n);
        }
    }
    fclose(f);
    WM_REQUIRE(buf.size() >= 12 && memcmp(buf.data(), "RIFF", 4) == 0 && memcmp(buf.data() + 8, "WAVE", 4) == 0, WM_ERR_IO,
               "'%s' is not a RIFF/WAVE file", path);
    bool have_fmt = false;
    size_t pos = 12, data_off = 0, data_len = 0;
    while (pos + 8 <= buf.size()) {
        const unsigned char *h = buf.data() + pos;
        size_t len = rd32(h + 4);
        const size_t body = pos + 8;
        if (memcmp(h, "fmt ", 4) == 0) {
            WM_REQUIRE(len >= 16 && body + 16 <= buf.size(), WM_ERR_IO, "'%s': truncated fmt chunk", path);
            const unsigned char *p = buf.data() + body;
            unsigned fmt = rd16(p);
            const unsigned ch = rd16(p + 2), rate = rd32(p + 4), bits = rd16(p + 14);
            if (fmt == 0xFFFE && len >= 26 && body + 26 <= buf.size()) fmt = rd16(p + 24);  // WAVE_FORMAT_EXTENSIBLE: sub-format
            WM_REQUIRE(fmt == 1 && ch == 1 && rate == 16000 && bits == 16, WM_ERR_IO,
                       "'%s': expected 16 kHz mono 16-bit PCM, got format %u, %u Hz, %u ch, %u-bit", path, fmt, rate, ch, bits);
            have_fmt = true;
        } else if (memcmp(h, "data", 4) == 0) {
            if (len == 0xFFFFFFFFu || body + len > buf.size()) len = buf.size() - body;  // streamed / truncated: what is there
            data_off = body;
            data_len = len;
            break;
        }
        pos = body + len + (len & 1);  // chunks are word-aligned
    }
    WM_REQUIRE(have_fmt, WM_ERR_IO, "'%s': no fmt chunk before the data", path);
    WM_REQUIRE(data_off != 0, WM_ERR_IO, "'%s': no data chunk", path);
    wm_wav *w = new wm_wav();
    w->raw.swap(buf);   // no second copy: samples are decoded (little endian -> host int16) window by window on read
    w->data_off = data_off;
    w->n_samples = data_len / 2;
    *out = w;
    return WM_OK;
} WM_API_CATCH

extern "C" void wm_wav_close(wm_wav *w) { delete w; }

extern "C" long wm_wav_num_samples(const wm_wav *w) { return w ? (long)w->n_samples : 0; }

// ceil(n / 480000), at least one window (an empty recording is one silent chunk -- sharding.chunk_pcm's rule)
extern "C" int wm_wav_num_chunks(const wm_wav *w) {
    if (!w) return 0;
    const size_t n = w->n_samples;
    return n == 0 ? 1 : (int)((n + WM_N_SAMPLES - 1) / WM_N_SAMPLES);
}

extern "C" int wm_wav_read_chunks(const wm_wav *w, int first_chunk, int n_chunks, int16_t *out) try {
    WM_REQUIRE(w && out && first_chunk >= 0 && n_chunks >= 0 && first_chunk + (long)n_chunks <= wm_wav_num_chunks(w),
               WM_ERR_INVALID, "wav_read_chunks: windows [%d, %d) outside the recording's %d", first_chunk,
               first_chunk + n_chunks, wm_wav_num_chunks(w));
    const size_t n = w->n_samples;
    for (int c = 0; c < n_chunks; ++c) {
        const size_t lo = (size_t)(first_chunk + c) * WM_N_SAMPLES;
        const size_t have = lo < n ? (n - lo < (size_t)WM_N_SAMPLES ? n - lo : (size_t)WM_N_SAMPLES) : 0;
        int16_t *dst = out + (size_t)c * WM_N_SAMPLES;
        const unsigned char *src = w->raw.data() + w->data_off + 2 * lo;
        for (size_t i = 0; i < have; ++i) dst[i] = (int16_t)rd16(src + 2 * i);   // little endian, whatever the host
        memset(dst + have, 0, ((size_t)WM_N_SAMPLES - have) * sizeof(int16_t));  // ContentView.swift:57-60: zero-pad
    }
    return WM_OK;
} WM_API_CATCH

// ---------------------------------------------------------------- general reader (wm_audio_*) ----------
// Any rate, 1 .. 8 channels, integer PCM 8 / 16 / 24 / 32 bits, IEEE float 32 / 64 bits, plain or WAVE_FORMAT_EXTENSIBLE:
// what wm_resample_16k takes.  The same parse and the same hardening as wm_wav_open; samples are decoded on read.
struct wm_audio {
    std::vector<unsigned char> raw;  // the file image
    size_t data_off = 0;
    uint64_t n_frames = 0;
    unsigned rate = 0, channels = 0, bits = 0;
    bool is_float = false;
};

namespace {
constexpr unsigned kMaxAudioChannels = 8;

int read_file(const char *path, std::vector<unsigned char> &buf) {
    FILE *f = fopen(path, "rb");
    WM_REQUIRE(f, WM_ERR_IO, "cannot open '%s'", path);
    unsigned char tmp[1 << 16];
    size_t n;
    while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) {
        if (buf.size() + n > kMaxWavBytes) { fclose(f); wm_set_error("'%s': larger than 4 GiB", path); return WM_ERR_IO; }
        buf.insert(buf.end(), tmp, tmp + n);
    }
    fclose(f);
    return WM_OK;
}

// one sample at p -> f32
inline float audio_sample(const unsigned char *p, unsigned bits, bool is_float) {
    if (is_float) {
        if (bits == 32) { uint32_t u = rd32(p); float v; memcpy(&v, &u, 4); return v; }
        uint64_t u = (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32);
        double d; memcpy(&d, &u, 8);
        if (d != d) return __builtin_nanf("");                                // (a cast of a NaN or an out-of-range double is
        if (d > 3.4028234663852886e38) return __builtin_inff();              //  undefined behaviour in C++: saturate)
        if (d < -3.4028234663852886e38) return -__builtin_inff();
        return (float)d;
    }
    switch (bits) {
        case 8: return (float)((int)p[0] - 128) * (1.0f / 128.0f);
        case 16: return (float)(int16_t)rd16(p) * (1.0f / 32768.0f);
        case 24: {
            int32_t v = (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
            if (v & 0x800000) v -= 0x1000000;
            return (float)v * (1.0f / 8388608.0f);   // |v| < 2^24: exact
        }
        default: return (float)((double)(int32_t)rd32(p) / 2147483648.0);   // 32: in double, rounded once
    }
}
}  // namespace

extern "C" int wm_audio_open(const char *path, wm_audio **out) try {
    WM_REQUIRE(path && out, WM_ERR_INVALID, "audio_open: null pointer");
    *out = nullptr;
    std::vector<unsigned char> buf;
    WM_TRY(read_file(path, buf));
    WM_REQUIRE(buf.size() >= 12 && memcmp(buf.data(), "RIFF", 4) == 0 && memcmp(buf.data() + 8, "WAVE", 4) == 0, WM_ERR_IO,
               "'%s' is not a RIFF/WAVE file", path);
    bool have_fmt = false, is_float = false;
    unsigned ch = 0, rate = 0, bits = 0;
    size_t pos = 12, data_off = 0, data_len = 0;
    while (pos + 8 <= buf.size()) {
        const unsigned char *h = buf.data() + pos;
        size_t len = rd32(h + 4);
        const size_t body = pos + 8;
        if (memcmp(h, "fmt ", 4) == 0) {
            WM_REQUIRE(len >= 16 && body + 16 <= buf.size(), WM_ERR_IO, "'%s': truncated fmt chunk", path);
            const unsigned char *p = buf.data() + body;
            unsigned fmt = rd16(p);
            const unsigned align = rd16(p + 12);
            ch = rd16(p + 2), rate = rd32(p + 4), bits = rd16(p + 14);
            if (fmt == 0xFFFE) {   // WAVE_FORMAT_EXTENSIBLE: the sub-format's first two bytes are the format tag
                WM_REQUIRE(len >= 26 && body + 26 <= buf.size(), WM_ERR_IO, "'%s': truncated extensible fmt chunk", path);
                fmt = rd16(p + 24);
            }
            WM_REQUIRE(fmt == 1 || fmt == 3, WM_ERR_IO, "'%s': format %u is neither integer PCM (1) nor IEEE float (3)", path, fmt);
            is_float = fmt == 3;
            WM_REQUIRE(ch >= 1 && ch <= kMaxAudioChannels, WM_ERR_IO, "'%s': %u channels (1 .. %u)", path, ch, kMaxAudioChannels);
            WM_REQUIRE(rate >= 1 && rate <= 0x7FFFFFFFu, WM_ERR_IO, "'%s': sample rate %u", path, rate);
            WM_REQUIRE(is_float ? (bits == 32 || bits == 64) : (bits == 8 || bits == 16 || bits == 24 || bits == 32), WM_ERR_IO,
                       "'%s': %u-bit %s samples are not supported", path, bits, is_float ? "float" : "integer");
            WM_REQUIRE(align == ch * (bits / 8), WM_ERR_IO, "'%s': block align %u, but %u channels of %u bits", path, align, ch, bits);
            have_fmt = true;
        } else if (memcmp(h, "data", 4) == 0) {
            if (len == 0xFFFFFFFFu || len > buf.size() - body) len = buf.size() - body;  // streamed / truncated: what is there
            data_off = body;
            data_len = len;
            break;
        }
        if (len > buf.size() - body) break;   // a chunk that runs past the file: nothing behind it
        pos = body + len + (len & 1);         // chunks are word-aligned
    }
    WM_REQUIRE(have_fmt, WM_ERR_IO, "'%s': no fmt chunk before the data", path);
    WM_REQUIRE(data_off != 0, WM_ERR_IO, "'%s': no data chunk", path);
    wm_audio *w = new wm_audio();
    w->raw.swap(buf);
    w->data_off = data_off;
    w->n_frames = data_len / ((size_t)ch * (bits / 8));   // whole frames only; <= 2^32, so frames * channels cannot overflow
    w->rate = rate;
    w->channels = ch;
    w->bits = bits;
    w->is_float = is_float;
    *out = w;
    return WM_OK;
} WM_API_CATCH

extern "C" void wm_audio_close(wm_audio *w) { delete w; }
extern "C" int wm_audio_sample_rate(const wm_audio *w) { return w ? (int)w->rate : 0; }
extern "C" int wm_audio_channels(const wm_audio *w) { return w ? (int)w->channels : 0; }
extern "C" int64_t wm_audio_num_frames(const wm_audio *w) { return w ? (int64_t)w->n_frames : 0; }
extern "C" int wm_audio_bits(const wm_audio *w) { return w ? (int)w->bits : 0; }
extern "C" int wm_audio_is_float(const wm_audio *w) { return w && w->is_float ? 1 : 0; }

namespace {
int audio_range(const wm_audio *w, int64_t first, int64_t n, const void *out, const char *what) {
    WM_REQUIRE(w && first >= 0 && n >= 0 && (uint64_t)first <= w->n_frames && (uint64_t)n <= w->n_frames - (uint64_t)first,
               WM_ERR_INVALID, "%s: frames [%lld, %lld + %lld) outside the recording's %lld", what, (long long)first,
               (long long)first, (long long)n, w ? (long long)w->n_frames : 0LL);
    WM_REQUIRE(out || n == 0, WM_ERR_INVALID, "%s: null output", what);
    return WM_OK;
}
}  // namespace

extern "C" int wm_audio_read(const wm_audio *w, int64_t first_frame, int64_t n_frames, float *out) try {
    WM_TRY(audio_range(w, first_frame, n_frames, out, "audio_read"));
    const size_t bytes = w->bits / 8, n = (size_t)n_frames * w->channels;
    const unsigned char *src = w->raw.data() + w->data_off + (size_t)first_frame * w->channels * bytes;
    for (size_t i = 0; i < n; ++i) out[i] = audio_sample(src + i * bytes, w->bits, w->is_float);
    return WM_OK;
} WM_API_CATCH

extern "C" int wm_audio_read_i16(const wm_audio *w, int64_t first_frame, int64_t n_frames, int16_t *out) try {
    WM_TRY(audio_range(w, first_frame, n_frames, out, "audio_read_i16"));
    WM_REQUIRE(!w->is_float && w->bits == 16, WM_ERR_INVALID, "audio_read_i16: the file holds %u-bit %s samples", w->bits,
               w->is_float ? "float" : "integer");
    const size_t n = (size_t)n_frames * w->channels;
    const unsigned char *src = w->raw.data() + w->data_off + (size_t)first_frame * w->channels * 2;
    for (size_t i = 0; i < n; ++i) out[i] = (int16_t)rd16(src + 2 * i);
    return WM_OK;
} WM_API_CATCH
