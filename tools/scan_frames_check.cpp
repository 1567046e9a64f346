// scan_frames_check -- the host scan of raw frame streams (flacenc::scan_raw_frames, csrc/host/flac_stream.cpp) with
// FLACGPU_SCAN_SPECULATIVE, run stand-alone under AddressSanitizer and UndefinedBehaviorSanitizer: every read of the
// extent walker (csrc/kernels/frame_extent.h) must stay inside the input it was given.  No device, no Python.
//
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover -Iinclude -Iflac-codec_amd/csrc/host \
//       tools/scan_frames_check.cpp flac-codec_amd/csrc/host/flac_stream.cpp flac-codec_amd/csrc/host/checksums.cpp \
//       -o scan_frames_check
//   scan_frames_check INPUTS
//
// INPUTS holds the inputs back to back, each a 32-bit little-endian length and that many bytes
// (tests/test_scan_frames_speculative.py writes it).  Every input is scanned whole, with and without the flag, and then
// truncated at every length that is a multiple of 7, each time from a heap block of exactly that size, so that one byte
// read past the end is reported.  Prints the number of inputs, of scans, and of frames kept in the whole inputs without
// and with the flag; exit status 0 when everything ran, 2 on a malformed file or a scan that loses a frame under the flag.
// The inputs are shared out among up to eight threads: a scan touches nothing but its own input.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "flac_stream.h"

static size_t scan(const uint8_t *src, size_t len, uint32_t flags) {
    uint8_t *exact = static_cast<uint8_t *>(malloc(len ? len : 1));   // no slack behind the input
    if (!exact) abort();
    memcpy(exact, src, len);
    std::vector<flacgpu_frame_record> frames;
    flacgpu_raw_stream sum{};
    flacenc::scan_raw_frames(exact, len, flags, frames, sum);
    free(exact);
    if (sum.frames != frames.size()) abort();
    return frames.size();
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s INPUTS\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<uint8_t> all;
    uint8_t buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + got);
    fclose(f);
    std::vector<std::pair<size_t, size_t>> inputs;   // (first byte, length)
    for (size_t at = 0; at < all.size();) {
        if (all.size() - at < 4) return 2;
        const size_t len = (size_t)all[at] | (size_t)all[at + 1] << 8 | (size_t)all[at + 2] << 16 | (size_t)all[at + 3] << 24;
        at += 4;
        if (all.size() - at < len) return 2;
        inputs.emplace_back(at, len);
        at += len;
    }
    std::atomic<size_t> next{0}, scans{0}, plain{0}, spec{0}, lost{0};
    auto work = [&] {
        for (size_t i; (i = next++) < inputs.size();) {
            const uint8_t *d = all.data() + inputs[i].first;
            const size_t len = inputs[i].second;
            const size_t a = scan(d, len, 0), b = scan(d, len, FLACGPU_SCAN_SPECULATIVE);
            if (b < a) lost++;
            plain += a;
            spec += b;
            scans += 2;
            for (size_t cut = 0; cut < len; cut += 7, scans++) scan(d, cut, FLACGPU_SCAN_SPECULATIVE);
        }
    };
    std::vector<std::thread> pool;
    const unsigned hw = std::thread::hardware_concurrency();
    for (unsigned t = 1; t < (hw < 8 ? hw : 8u); t++) pool.emplace_back(work);
    work();
    for (std::thread &t : pool) t.join();
    printf("inputs %zu scans %zu frames %zu speculative %zu\n", inputs.size(), scans.load(), plain.load(), spec.load());
    return lost ? 2 : 0;
}
