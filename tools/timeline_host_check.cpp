// timeline_host_check.cpp -- the timeline rule (host/flac_stream.cpp timeline_of_records) in a program of its own, for a
// sanitizer run of the host code without a GPU and without Python in the process:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iflac-codec_amd/csrc/host \
//       tools/timeline_host_check.cpp flac-codec_amd/csrc/host/flac_stream.cpp flac-codec_amd/csrc/host/checksums.cpp -o check
//   ./check < records.txt
// records.txt is tests/_timeline.dump's text: per stream a line with the record count n, then n lines of the 13 fields
// of flacgpu_frame_record.  Prints one line per stream -- rc placed dropped concealed gaps first_sample timeline_samples
// gap_samples concealed_samples -- and per record `at flags`, which the caller compares with the model's.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "flac_stream.h"

int main() {
    size_t n = 0, streams = 0;
    while (scanf("%zu", &n) == 1) {
        std::vector<flacgpu_frame_record> recs(n);
        for (flacgpu_frame_record &r : recs)
            if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %u %u %u %u %u %u %u %u %u %u", &r.byte_offset, &r.number,
                      &r.out_offset, &r.stream, &r.bytes, &r.block_size, &r.sample_rate, &r.channels, &r.bits_per_sample,
                      &r.assignment, &r.blocking, &r.status, &r.reserved) != 13)
                return 2;
        // exactly n entries on the heap: a write past the end is the sanitizer's to find
        std::vector<flacgpu_timeline_frame> frames(n);
        flacgpu_timeline_result res;
        flacenc::timeline_of_records(recs.data(), n, frames.data(), res);
        printf("%d %u %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", res.rc, res.placed, res.dropped,
               res.concealed, res.gaps, res.first_sample, res.timeline_samples, res.gap_samples, res.concealed_samples);
        for (const flacgpu_timeline_frame &f : frames) printf("%" PRIu64 " %u\n", f.at, f.flags);
        streams++;
    }
    fprintf(stderr, "%zu streams\n", streams);
    return 0;
}
