// session_check -- the two host-side pieces of a decoder session (DESIGN.md 4b "Decoder sessions"), run stand-alone under
// AddressSanitizer and UndefinedBehaviorSanitizer: the per-group rule that builds a slot from a held tail and a chunk
// (csrc/kernels/session_slots_rule.h, its host pass) and the host session (flacgpu_session_host_*,
// csrc/host/session_rule.cpp).  No device, no Python.
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Iflac-codec_amd/csrc/host -Iflac-codec_amd/csrc tools/session_check.cpp \
//       flac-codec_amd/csrc/host/session_rule.cpp flac-codec_amd/csrc/host/flac_stream.cpp \
//       flac-codec_amd/csrc/host/checksums.cpp -o session_check
//   python tools/session_check_inputs.py INPUTS      (the 30 streams of the recorded run, fixed by the tests' seeds)
//   session_check [INPUTS]
//
// Part 1 needs no input: tail length 0..49 x tail source residue 0..15 x chunk source residue 0..15 x chunk length
// 0..49, and tails and chunks around 64 bytes and 16 KiB; every source is a heap block that ENDS with the source (and a
// second time one with slack behind it), so that a read of one byte outside it is reported; every group is compared
// with the concatenation.  Part 2: INPUTS holds raw frame streams back to back, each a 32-bit little-endian length and
// that many bytes; every stream goes through a host session in chunks of 1, 7, 64 and 333 bytes, each chunk a heap
// block of exactly its size, and the records must not depend on the chunking.  Exit status 0 when everything agreed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flacenc_gpu.h"
#include "kernels/session_slots_rule.h"

namespace {
// n bytes at address residue `res` modulo 16 that end with their heap block (at_end) or have slack behind them
struct Source {
    uint8_t *block = nullptr, *p = nullptr;
    Source(size_t n, uint32_t res, bool at_end, uint32_t seed) {
        // a 16-byte aligned block of res + n bytes ends with the source; with slack behind it the aligned groups the
        // rule touches behind the source are the block's too, and only the bytes in front of p are not the source's
        void *mem = nullptr;
        if (posix_memalign(&mem, 16, res + n + (at_end ? 0 : 48) + (res + n ? 0 : 1))) abort();
        block = static_cast<uint8_t *>(mem);
        p = block + res;
        for (size_t i = 0; i < n; i++) p[i] = (uint8_t)((i * 7 + seed) % 251 + 1);
    }
    ~Source() { free(block); }
};

bool check_slot(size_t tl, uint32_t tres, size_t cl, uint32_t cres, bool at_end) {
    Source tail(tl, tres, at_end, 3), chunk(cl, cres, at_end, 5);
    if (((uintptr_t)tail.p & 15u) != tres || ((uintptr_t)chunk.p & 15u) != cres) return false;
    const SessionSrc src{(uint64_t)(uintptr_t)tail.p, tl, (uint64_t)(uintptr_t)chunk.p, cl};
    const size_t span = (tl + cl + 64 + 63) & ~(size_t)63;
    for (size_t rel = 0; rel < span; rel += 16) {
        const uint4 v = session_group(src, rel);
        uint8_t got[16], want[16];
        memcpy(got, &v, 16);
        for (size_t j = 0; j < 16; j++) {
            const size_t k = rel + j;
            want[j] = k < tl ? tail.p[k] : k < tl + cl ? chunk.p[k - tl] : 0;
        }
        if (memcmp(got, want, 16) != 0) return false;
    }
    return true;
}

struct Feed {
    std::vector<flacgpu_frame_record> records;
    flacgpu_raw_stream raw{};
};

bool run_session(const uint8_t *data, size_t len, size_t step, Feed &out) {
    flacgpu_session_host *s = nullptr;
    if (flacgpu_session_host_open(1, 4096, &s)) return false;
    std::vector<flacgpu_frame_record> recs(len / 4 + 16);
    for (size_t at = 0; at <= len; at += step) {
        const bool last = at + step > len;
        const size_t n = last ? len - at : step;
        uint8_t *exact = static_cast<uint8_t *>(malloc(n ? n : 1));   // no slack behind the chunk
        if (!exact) abort();
        memcpy(exact, data + at, n);
        const uint8_t *ptr = exact;
        uint64_t total = 0, held = 0;
        const int rc = flacgpu_session_host_feed(s, &ptr, &n, nullptr, recs.data(), recs.size(), &out.raw, &held, &total);
        free(exact);
        if (rc || held > 4096 + 15) return false;
        out.records.insert(out.records.end(), recs.begin(), recs.begin() + total);
    }
    uint64_t total = 0;
    if (flacgpu_session_host_finish(s, recs.data(), recs.size(), &out.raw, &total)) return false;
    out.records.insert(out.records.end(), recs.begin(), recs.begin() + total);
    flacgpu_session_host_close(s);
    return true;
}
}  // namespace

int main(int argc, char **argv) {
    size_t slots = 0;
    for (int at_end = 0; at_end < 2; at_end++) {
        for (uint32_t tres = 0; tres < 16; tres++)
            for (uint32_t cres = 0; cres < 16; cres++)
                for (size_t tl = 0; tl < 50; tl++)
                    for (size_t cl = 0; cl < 50; cl++, slots++)
                        if (!check_slot(tl, tres, cl, cres, at_end)) {
                            fprintf(stderr, "slot: tail %zu @%u, chunk %zu @%u\n", tl, tres, cl, cres);
                            return 1;
                        }
        for (size_t tl : {63, 64, 65, 16383, 16384, 16385})
            for (size_t cl : {1, 63, 64, 65, 16400}) {
                if (!check_slot(tl, 13, cl, 7, at_end)) return 1;
                slots++;
            }
    }
    size_t inputs = 0, frames = 0;
    if (argc == 2) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) {
            perror(argv[1]);
            return 2;
        }
        std::vector<uint8_t> all;
        uint8_t buf[1 << 16];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + got);
        fclose(f);
        for (size_t at = 0; at < all.size(); inputs++) {
            if (all.size() - at < 4) return 2;
            const size_t len = (size_t)all[at] | (size_t)all[at + 1] << 8 | (size_t)all[at + 2] << 16 | (size_t)all[at + 3] << 24;
            at += 4;
            if (all.size() - at < len) return 2;
            Feed first;
            for (size_t step : {1, 7, 64, 333}) {
                Feed f2;
                if (!run_session(all.data() + at, len, step, step == 1 ? first : f2)) return 1;
                const Feed &g = step == 1 ? first : f2;
                if (g.records.size() != first.records.size() || g.raw.skipped_bytes != first.raw.skipped_bytes ||
                    g.raw.gaps != first.raw.gaps || g.raw.frames != first.raw.frames)
                    return 1;
                for (size_t k = 0; k < g.records.size(); k++)
                    if (g.records[k].byte_offset != first.records[k].byte_offset || g.records[k].bytes != first.records[k].bytes)
                        return 1;
            }
            frames += first.records.size();
            at += len;
        }
    }
    printf("slots %zu inputs %zu frames %zu\n", slots, inputs, frames);
    return 0;
}
