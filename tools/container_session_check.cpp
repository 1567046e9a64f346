// container_session_check -- the host side of a container session (DESIGN.md 4b "Container sessions"), run stand-alone
// under AddressSanitizer and UndefinedBehaviorSanitizer: the resumable metadata walk (csrc/kernels/meta_feed_rule.h
// through flacgpu_meta_feed_host) and the host container session (flacgpu_session_host_open_container,
// csrc/host/session_rule.cpp).  No device, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       -Iflac-codec_amd/csrc/host -Iflac-codec_amd/csrc tools/container_session_check.cpp \
//       flac-codec_amd/csrc/host/session_rule.cpp flac-codec_amd/csrc/host/flac_stream.cpp \
//       flac-codec_amd/csrc/host/checksums.cpp -o container_session_check
//   python tools/container_session_check_inputs.py INPUTS   (the tests' own streams, fixed by their seeds)
//   container_session_check INPUTS
//
// INPUTS holds .flac streams (whole, damaged, truncated, refused) back to back, each a 32-bit little-endian length and
// that many bytes.  Every stream goes through the walk and through a host session in chunks of 1, 7, 64 and 333 bytes,
// each chunk a heap block of exactly its size, so that a read of one byte outside a chunk is reported.  The walk must
// give what the one-shot decoders' parse_metadata gives for the whole stream (flacgpu_meta_walk_host's answer); the
// session's frames must be those of their scan_frames (flacgpu_scan_stream_host's answer), whatever the chunking.  Exit status 0 when everything agreed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flac_stream.h"
#include "flacenc_gpu.h"

namespace {
constexpr uint32_t kW = 1u << 22;   // the largest max_frame_bytes: no frame of the inputs is longer

// data[at, at + n) in a heap block of exactly n bytes (one byte when n is 0: never read)
struct Exact {
    uint8_t *p;
    Exact(const uint8_t *data, size_t n) : p(static_cast<uint8_t *>(malloc(n ? n : 1))) {
        if (!p) abort();
        memcpy(p, data, n);
    }
    ~Exact() { free(p); }
};

bool same_info(const flacgpu_stream_info &a, const flacgpu_stream_info &b) { return !memcmp(&a, &b, sizeof a); }

bool check_walk(const uint8_t *data, size_t len, size_t step) {
    flacgpu_stream_info want{}, got{};
    uint32_t want_mf = 0, got_mf = 0;
    uint64_t want_at = 0, got_at = 0;
    size_t pos = 0;
    const int want_rc = flacenc::parse_metadata(data, len, &want, &want_mf, &pos) ? FLACGPU_ERR_INVALID_ARG : FLACGPU_OK;
    if (!want_rc) want_at = pos;
    flacgpu_meta_feed st;
    flacgpu_meta_feed_init_host(&st);
    uint64_t used = 0;
    for (size_t at = 0; at < len; at += step) {
        const size_t n = len - at < step ? len - at : step;
        Exact chunk(data + at, n);
        size_t took = 0;
        if (flacgpu_meta_feed_host(&st, chunk.p, n, &took) || took > n) return false;
        used += took;
    }
    const int got_rc = flacgpu_meta_feed_result_host(&st, len, &got, &got_mf, &got_at);
    if (got_rc != want_rc || !same_info(got, want) || got_mf != want_mf || got_at != want_at) return false;
    return want_rc != 0 || used == want_at;
}

struct Run {
    std::vector<flacgpu_frame_record> records;
    flacgpu_raw_stream raw{};
};

bool run_session(const uint8_t *data, size_t len, size_t step, Run &out) {
    flacgpu_session_host *s = nullptr;
    if (flacgpu_session_host_open_container(1, kW, &s)) return false;
    std::vector<flacgpu_frame_record> recs(len / 8 + 16);
    for (size_t at = 0; at < len; at += step) {
        const size_t n = len - at < step ? len - at : step;
        Exact chunk(data + at, n);
        const uint8_t *ptr = chunk.p;
        uint64_t total = 0, held = 0;
        if (flacgpu_session_host_feed(s, &ptr, &n, nullptr, recs.data(), recs.size(), &out.raw, &held, &total) ||
            held > kW + 15)
            return false;
        out.records.insert(out.records.end(), recs.begin(), recs.begin() + total);
    }
    uint64_t total = 0;
    if (flacgpu_session_host_finish(s, recs.data(), recs.size(), &out.raw, &total)) return false;
    out.records.insert(out.records.end(), recs.begin(), recs.begin() + total);
    flacgpu_session_host_close(s);
    return true;
}

// the session's frames against the one-shot scan of the whole stream
bool check_session(const uint8_t *data, size_t len, size_t step, size_t *frames) {
    Run run;
    if (!run_session(data, len, step, run)) return false;
    flacgpu_stream_info info{};
    uint32_t min_frame = 0;
    size_t pos = 0;
    if (flacenc::parse_metadata(data, len, &info, &min_frame, &pos))   // refused: every byte is skipped
        return run.records.empty() && !run.raw.uniform && run.raw.skipped_bytes == len;
    flacenc::FrameScan scan;   // the one-shot decoders' scan of the whole stream
    if (pos < len) flacenc::scan_frames(data, len, pos, min_frame, &info, scan);
    const std::vector<uint64_t> &off = scan.off;
    const std::vector<uint32_t> &size = scan.n;
    const uint32_t n = (uint32_t)size.size();
    if (run.records.size() != n || run.raw.frames != n || !run.raw.uniform || run.raw.gaps != info.bad_frames) return false;
    for (uint32_t k = 0; k < n; k++)
        if (run.records[k].byte_offset != off[k] || run.records[k].block_size != size[k]) return false;
    *frames += n;
    return true;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: container_session_check INPUTS\n");
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
    size_t inputs = 0, frames = 0;
    for (size_t at = 0; at < all.size(); inputs++) {
        if (all.size() - at < 4) return 2;
        const size_t len = (size_t)all[at] | (size_t)all[at + 1] << 8 | (size_t)all[at + 2] << 16 | (size_t)all[at + 3] << 24;
        at += 4;
        if (all.size() - at < len) return 2;
        Exact whole(all.data() + at, len);
        for (size_t step : {1, 7, 64, 333}) {
            if (!check_walk(whole.p, len, step)) {
                fprintf(stderr, "input %zu: the walk in chunks of %zu differs\n", inputs, step);
                return 1;
            }
            size_t fr = 0;
            if (!check_session(whole.p, len, step, &fr)) {
                fprintf(stderr, "input %zu: the session in chunks of %zu differs\n", inputs, step);
                return 1;
            }
            if (step == 1) frames += fr;
        }
        at += len;
    }
    printf("inputs %zu frames %zu\n", inputs, frames);
    return 0;
}
