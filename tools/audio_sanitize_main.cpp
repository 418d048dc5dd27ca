// audio_sanitize_main.cpp -- a stand-alone driver of the general WAV reader (wm_audio_open / wm_audio_read, csrc/audio.cpp)
// over malformed files, for a host-sanitizer build.  CPU only: it links csrc/audio.cpp alone (no HIP call is made) and
// needs no GPU and no preloaded runtime:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I include -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all -x hip tools/audio_sanitize_main.cpp \
//         openai-whisper-coreml_amd/csrc/audio.cpp -o /tmp/audio_sanitize && /tmp/audio_sanitize
//
// Every case must come back with a status; the sanitizers turn any out-of-bounds byte or overflow into a failure.
// Prints the number of files tried and exits 0.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "whisper_mi355x.h"

void wm_set_error(const char *, ...) {}   // audio.cpp's only dependency on the rest of the library

namespace {
typedef std::vector<unsigned char> Bytes;
void put16(Bytes &b, unsigned v) { b.push_back(v & 255); b.push_back((v >> 8) & 255); }
void put32(Bytes &b, uint32_t v) { put16(b, v & 0xffff); put16(b, v >> 16); }
void puts4(Bytes &b, const char *s) { b.insert(b.end(), s, s + 4); }

Bytes riff(unsigned tag, unsigned ch, uint32_t rate, unsigned bits, unsigned align, int sub, size_t n_data, uint32_t data_len,
           bool junk) {
    Bytes b;
    puts4(b, "RIFF"); put32(b, 0); puts4(b, "WAVE");
    puts4(b, "fmt "); put32(b, sub >= 0 ? 40 : 16);
    put16(b, tag); put16(b, ch); put32(b, rate); put32(b, rate * align); put16(b, align); put16(b, bits);
    if (sub >= 0) {
        put16(b, 22); put16(b, bits); put32(b, 0); put16(b, (unsigned)sub);
        for (int i = 0; i < 14; ++i) b.push_back((unsigned char)i);
    }
    if (junk) { puts4(b, "junk"); put32(b, 5); for (int i = 0; i < 6; ++i) b.push_back('x'); }
    puts4(b, "data"); put32(b, data_len);
    for (size_t i = 0; i < n_data; ++i) b.push_back((unsigned char)(i * 37 + 11));
    return b;
}

int g_files = 0, g_opened = 0;

void try_file(const std::string &path, const Bytes &b) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { perror("fopen"); exit(2); }
    if (!b.empty()) fwrite(b.data(), 1, b.size(), f);
    fclose(f);
    ++g_files;
    wm_audio *a = nullptr;
    if (wm_audio_open(path.c_str(), &a) != WM_OK) {
        if (a) { fprintf(stderr, "a failed open handed out a handle\n"); exit(1); }
        return;
    }
    ++g_opened;
    const int64_t n = wm_audio_num_frames(a);
    const int c = wm_audio_channels(a);
    std::vector<float> out((size_t)n * c + 1);       // exactly sized: one float too many is ASan's to catch
    std::vector<int16_t> o16((size_t)n * c + 1);
    if (wm_audio_read(a, 0, n, out.data()) != WM_OK) { fprintf(stderr, "a full read failed\n"); exit(1); }
    (void)wm_audio_read_i16(a, 0, n, o16.data());
    if (n > 1 && wm_audio_read(a, n / 2, n - n / 2, out.data()) != WM_OK) { fprintf(stderr, "a partial read failed\n"); exit(1); }
    if (wm_audio_read(a, n, 1, out.data()) == WM_OK || wm_audio_read(a, -1, 1, out.data()) == WM_OK ||
        wm_audio_read(a, 1, INT64_MAX, out.data()) == WM_OK || wm_audio_read(a, INT64_MAX, INT64_MAX, out.data()) == WM_OK) {
        fprintf(stderr, "an out-of-range read was accepted\n");
        exit(1);
    }
    wm_audio_close(a);
}
}  // namespace

int main() {
    char dir[] = "/tmp/wm_audio_sanXXXXXX";
    if (!mkdtemp(dir)) { perror("mkdtemp"); return 2; }
    const std::string path = std::string(dir) + "/case.wav";
    const unsigned tags[] = {0, 1, 2, 3, 0xFFFE}, chans[] = {0, 1, 2, 3, 8, 9, 65535}, bitses[] = {0, 8, 12, 16, 24, 32, 64, 65528};
    const uint32_t rates[] = {0, 8000, 44100, 0xFFFFFFFFu}, lens[] = {0, 1, 7, 333, 0x7FFFFFFFu, 0xFFFFFFFFu};
    // every header combination, honest and dishonest block aligns, data lengths that lie
    for (unsigned tag : tags)
        for (unsigned ch : chans)
            for (unsigned bits : bitses)
                for (int k = 0; k < 6; ++k) {
                    const unsigned align = (k & 1) ? 1 : (ch * (bits / 8)) & 0xffff;
                    const int sub = tag == 0xFFFE ? (k % 3 == 0 ? 1 : k % 3 == 1 ? 3 : 9) : -1;
                    try_file(path, riff(tag, ch, rates[(ch + bits + k) % 4], bits, align, sub, 333, lens[k], k & 2));
                }
    // every truncation of a well-formed extensible file, and every single-byte corruption of its header
    const Bytes good = riff(0xFFFE, 2, 48000, 24, 6, 1, 120, 120, true);
    for (size_t cut = 0; cut <= good.size(); ++cut) try_file(path, Bytes(good.begin(), good.begin() + cut));
    for (size_t pos = 0; pos < good.size() - 120; ++pos)
        for (unsigned v : {0u, 1u, 0x7Fu, 0x80u, 0xFFu}) {
            Bytes b = good;
            b[pos] = (unsigned char)v;
            try_file(path, b);
        }
    // float files with non-finite and out-of-range doubles
    Bytes f64 = riff(3, 1, 22050, 64, 8, -1, 0, 64, false);
    const double vals[] = {1e300, -1e300, 0.0 / 1.0, __builtin_nan(""), __builtin_inf(), -__builtin_inf(), 3.5e38, 1e-320};
    for (double d : vals) { unsigned char raw[8]; memcpy(raw, &d, 8); f64.insert(f64.end(), raw, raw + 8); }
    try_file(path, f64);
    // null arguments
    wm_audio *a = nullptr;
    if (wm_audio_open(nullptr, &a) == WM_OK || wm_audio_open(path.c_str(), nullptr) == WM_OK || wm_audio_read(nullptr, 0, 0, nullptr) == WM_OK) return 1;
    wm_audio_close(nullptr);
    unlink(path.c_str());
    rmdir(dir);
    printf("audio_sanitize: %d files tried, %d opened, no finding\n", g_files, g_opened);
    return 0;
}
