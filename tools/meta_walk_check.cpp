// meta_walk_check -- the metadata walk the batch decoder runs on streams in device memory (meta_walk,
// csrc/kernels/meta_walk.h; the host build, which flacenc::parse_metadata is made of), run stand-alone under
// AddressSanitizer and UndefinedBehaviorSanitizer: every read must stay inside the input it was given.  No device, no
// Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover -Iinclude -Iflac-codec_amd/csrc/host \
//       tools/meta_walk_check.cpp flac-codec_amd/csrc/host/flac_stream.cpp flac-codec_amd/csrc/host/checksums.cpp \
//       -o meta_walk_check
//   meta_walk_check INPUTS
//
// INPUTS holds the inputs back to back, each a 32-bit little-endian length and that many bytes
// (tests/test_device_input_abi.py writes it).  Every input is walked from a heap block of exactly its size, so that one
// byte read past the end is reported.  Prints the number of inputs, how many were accepted, and the sum of their
// frames_at; exit status 0 when everything ran, 2 on a malformed file or a walk whose answer is impossible (frames_at
// past the end, an accepted stream without a STREAMINFO).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flac_stream.h"

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
    size_t inputs = 0, accepted = 0, sum = 0;
    for (size_t at = 0; at < all.size();) {
        if (all.size() - at < 4) return 2;
        const size_t len = (size_t)all[at] | (size_t)all[at + 1] << 8 | (size_t)all[at + 2] << 16 | (size_t)all[at + 3] << 24;
        at += 4;
        if (all.size() - at < len) return 2;
        uint8_t *exact = static_cast<uint8_t *>(malloc(len ? len : 1));   // no slack behind the input
        if (!exact) abort();
        memcpy(exact, all.data() + at, len);
        MetaRecord rec;
        meta_walk(exact, len, rec);
        flacgpu_stream_info info;
        uint32_t min_frame = 0;
        size_t frames_at = 0;
        const char *why = flacenc::metadata_of_record(rec, &info, &min_frame, &frames_at);
        flacgpu_stream_info info2;
        uint32_t min_frame2 = 0;
        size_t frames_at2 = 0;
        const char *why2 = flacenc::parse_metadata(exact, len, &info2, &min_frame2, &frames_at2);
        free(exact);
        if (!why != !why2 || memcmp(&info, &info2, sizeof info) != 0 || min_frame != min_frame2 || frames_at != frames_at2) return 2;
        if (!why && (frames_at > len || !(rec.status & META_HAVE_SI) || rec.frames_at != frames_at)) return 2;
        inputs++;
        accepted += !why;
        sum += frames_at;
        at += len;
    }
    printf("inputs %zu accepted %zu frames_at %zu\n", inputs, accepted, sum);
    return 0;
}
