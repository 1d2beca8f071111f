// wav_max_main.cpp — TEST INFRASTRUCTURE: a stand-alone program (its own main, host code only) over the library's wav reader
// (csrc/ss_wavio.hpp), built by tests/test_rir16_loader_args.py with -fsanitize=address,undefined.  It writes three tiny float32
// stereo wav files (and names a fourth that does not exist) into the directory given as argv[1], reads them through
// sswav::read_many with and without the maxima, and compares rows, statuses and maxima with what it wrote.  Prints "ok" and returns
// 0, or says what differs and returns 1.  Never part of the product, never loaded into Python.
#include "../sound-spaces_amd/csrc/ss_wavio.hpp"

#include <cmath>
#include <cstdio>
#include <string>

static bool write_wav(const std::string& path, const std::vector<float>& frames) {      // frames: (L, R) pairs
    const uint32_t bytes = static_cast<uint32_t>(frames.size() * 4);
    unsigned char h[44];
    auto put32 = [&](int at, uint32_t v) { for (int i = 0; i < 4; ++i) h[at + i] = static_cast<unsigned char>(v >> (8 * i)); };
    auto put16 = [&](int at, uint32_t v) { h[at] = static_cast<unsigned char>(v); h[at + 1] = static_cast<unsigned char>(v >> 8); };
    std::memcpy(h, "RIFF", 4); put32(4, 36 + bytes); std::memcpy(h + 8, "WAVEfmt ", 8); put32(16, 16);
    put16(20, 3); put16(22, 2); put32(24, 16000); put32(28, 16000 * 8); put16(32, 8); put16(34, 32);
    std::memcpy(h + 36, "data", 4); put32(40, bytes);
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    bool ok = std::fwrite(h, 1, 44, f) == 44 && (frames.empty() || std::fwrite(frames.data(), 4, frames.size(), f) == frames.size());
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: wav_max_main <dir>\n"); return 2; }
    const std::string dir = argv[1];
    // a: 700 frames (past the reader's first 4-KiB read), peak of ear 0 on the LAST frame; b: 5 frames, ear 1 silent; c: no frames
    std::vector<std::vector<float>> data(3);
    for (int j = 0; j < 700; ++j) { data[0].push_back(0.25f * std::sin(0.37f * j)); data[0].push_back(-0.5f * std::cos(0.11f * j)); }
    data[0][2 * 699] = -3.5f;
    data[1] = {0.125f, 0.f, -0.75f, 0.f, 0.5f, 0.f, 0.f, 0.f, 0x1p-20f, 0.f};
    std::vector<std::string> paths = {dir + "/a.wav", dir + "/b.wav", dir + "/c.wav", dir + "/missing.wav"};
    for (int i = 0; i < 3; ++i)
        if (!write_wav(paths[i], data[i])) { std::fprintf(stderr, "cannot write %s\n", paths[i].c_str()); return 2; }
    const int n = 4, cap = 704;
    const char* cp[4];
    for (int i = 0; i < n; ++i) cp[i] = paths[i].c_str();
    int bad = 0;
    for (int keep : {-1, 699, 3}) {
        for (int threads : {1, 3}) {
            std::vector<float> rows(static_cast<size_t>(n) * 2 * cap, 7.f), plain(rows), mx(2 * n, -1.f);
            std::vector<int> kept(n), frames(n), status(n), kept0(n), frames0(n), status0(n);
            sswav::read_many(cp, n, rows.data(), 2LL * cap, cap, keep, false, kept.data(), frames.data(), status.data(), threads, mx.data());
            sswav::read_many(cp, n, plain.data(), 2LL * cap, cap, keep, false, kept0.data(), frames0.data(), status0.data(), threads);
            if (rows != plain || kept != kept0 || frames != frames0 || status != status0) { std::fprintf(stderr, "keep %d: rows differ\n", keep); ++bad; }
            const int want_status[4] = {sswav::kOk, sswav::kOk, sswav::kEmpty, sswav::kMissing};
            for (int i = 0; i < n; ++i) {
                float ml = 0.f, mr = 0.f;
                if (i < 2) {
                    const int fr = static_cast<int>(data[i].size() / 2), k = keep >= 0 && keep < fr ? keep : fr;
                    for (int j = 0; j < k; ++j) { ml = std::fmax(ml, std::fabs(data[i][2 * j])); mr = std::fmax(mr, std::fabs(data[i][2 * j + 1])); }
                    if (kept[i] != k || std::memcmp(rows.data() + static_cast<size_t>(i) * 2 * cap, data[i].data(), static_cast<size_t>(k) * 8) != 0) {
                        std::fprintf(stderr, "keep %d file %d: samples differ\n", keep, i); ++bad;
                    }
                }
                if (status[i] != want_status[i] || mx[2 * i] != ml || mx[2 * i + 1] != mr) {
                    std::fprintf(stderr, "keep %d file %d: status %d maxima %g %g, expected %d %g %g\n", keep, i, status[i], mx[2 * i], mx[2 * i + 1],
                                 want_status[i], ml, mr);
                    ++bad;
                }
            }
            if (keep == -1 && mx[0] != 3.5f) { std::fprintf(stderr, "the last frame's peak was not counted\n"); ++bad; }
            if (keep == 699 && mx[0] >= 3.5f) { std::fprintf(stderr, "a frame behind keep was counted\n"); ++bad; }
        }
    }
    if (bad) return 1;
    std::puts("ok");
    return 0;
}
