// frame_analysis_fuzz_main.cpp -- a stand-alone program around flacgpu_analyze_frame_host for the address and
// undefined-behaviour sanitizers (TEST INFRASTRUCTURE ONLY; built and run by tests/test_frame_analysis_host.py as a
// child process, together with csrc/host/frame_analysis.cpp, flac_stream.cpp and checksums.cpp; no device code).
// Input file: frames, each a little-endian uint32 length, a uint32 STREAMINFO sample size, then the bytes.  Every frame
// is analysed whole, at every truncation and under `flips` single-bit flips (a fixed generator), with rows and
// without.  Every buffer is a heap block of exactly the size the frame needs -- the rows are sized for the intact
// frame, so a flip that enlarges the block size must be refused as too small -- so that a store outside them is the
// sanitizer's to report.  Exit status 0: every call returned FLACGPU_OK or FLACGPU_ERR_BUFFER_TOO_SMALL.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "flacenc_gpu.h"

static int run(const uint8_t *frame, size_t len, uint32_t bps, size_t rows_cap, bool expect_ok) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[len ? len : 1]);   // exactly len bytes: a read behind them is reported
    if (len) memcpy(copy.get(), frame, len);
    std::unique_ptr<flacgpu_frame_analysis> fa(new flacgpu_frame_analysis);
    std::unique_ptr<flacgpu_subframe_plan[]> subs(new flacgpu_subframe_plan[FLACGPU_MAX_CHANNELS]);
    std::unique_ptr<int64_t[]> rows(new int64_t[rows_cap ? rows_cap : 1]);
    for (int with_rows = 0; with_rows < 2; with_rows++) {
        const int rc = flacgpu_analyze_frame_host(len ? copy.get() : nullptr, len, bps, fa.get(), subs.get(),
                                                  with_rows ? rows.get() : nullptr, with_rows ? rows_cap : 0);
        if (rc != FLACGPU_OK && rc != FLACGPU_ERR_BUFFER_TOO_SMALL) return 1;
        if (expect_ok && (rc != FLACGPU_OK || fa->status != 0)) return 2;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) return 64;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 65;
    const long flips = strtol(argv[2], nullptr, 10);
    uint32_t head[2];
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    size_t calls = 0;
    while (fread(head, 4, 2, f) == 2) {
        std::vector<uint8_t> frame(head[0]);
        if (fread(frame.data(), 1, frame.size(), f) != frame.size()) return 66;
        // the intact frame tells how large its rows are
        flacgpu_frame_analysis fa;
        flacgpu_subframe_plan subs[FLACGPU_MAX_CHANNELS];
        if (flacgpu_analyze_frame_host(frame.data(), frame.size(), head[1], &fa, subs, nullptr, 0) || fa.status) return 67;
        const size_t rows_cap = (size_t)fa.plan.channels * ((fa.block_size + 3u) & ~3u);
        if (int rc = run(frame.data(), frame.size(), head[1], rows_cap, true)) return 10 + rc;
        for (size_t cut = 0; cut < frame.size(); cut++, calls++)
            if (int rc = run(frame.data(), cut, head[1], rows_cap, false)) return 20 + rc;
        for (long k = 0; k < flips; k++, calls++) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            const size_t bit = (size_t)((seed >> 20) % (8 * frame.size()));
            frame[bit >> 3] ^= (uint8_t)(0x80u >> (bit & 7));
            const int rc = run(frame.data(), frame.size(), head[1], rows_cap, false);
            frame[bit >> 3] ^= (uint8_t)(0x80u >> (bit & 7));
            if (rc) return 30 + rc;
        }
    }
    fclose(f);
    printf("%zu damaged frames analysed\n", calls);
    return 0;
}
