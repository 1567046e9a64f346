// stream_ledger_main.cpp -- StreamLedger (flac-codec_amd/csrc/host/stream_ledger.h) as a stand-alone program, for a build
// with -fsanitize=address,undefined from host/stream_ledger.cpp ALONE (tests/test_stream_ledger_host.py): that it links
// without the rest of the host driver and without HIP is part of the check.
//   usage: stream_ledger_main cases.txt     one case per line, one result line per case ("-" stands for an absent string,
//                                           other strings are hex):
//   header  block rate bps ch has_total total padding seek_mode seek_value vendor n_tags tag.. md5 last_len n_cuts cut.. size..
//           open, the frames fed cut[0], cut[1], ... at a time (sizes in stream order, the stream's last frame last_len
//           samples long), close -> "rc header-in-hex"
//   admit   block total n_runs {n_frames last_len}..
//           open with that total, every run through admit / frames (10 bytes a frame) / overrun
//           -> per run "usable deferred error samples_written seek_points", separated by "|"
//   verdict known total written                      -> "rc"
//   sizes   size..    frames of these sizes          -> "min_frame max_frame"
#include <stdint.h>
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "stream_ledger.h"

using namespace flacenc_host;

static std::string unhex(const std::string &h) {
    std::string s;
    if (h == "-") return s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back(static_cast<char>(std::stoi(h.substr(i, 2), nullptr, 16)));
    return s;
}

static flacenc_options options_of(uint32_t block) {
    flacenc_options o{};
    o.block_size = block;
    o.max_partition_order = 5;
    o.max_lpc_order = 8;
    return o;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: stream_ledger_main cases.txt\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string kind;
        if (!(ls >> kind)) continue;
        if (kind == "header") {
            uint32_t block, rate, bps, ch, has_total, n_tags, last_len, n_cuts;
            uint64_t total;
            int64_t padding;
            std::string vendor_hex, md5_hex;
            ls >> block >> rate >> bps >> ch >> has_total >> total;
            flacenc_options o = options_of(block);
            ls >> padding >> o.seektable_mode >> o.seektable_value >> vendor_hex >> n_tags;
            o.padding = padding;
            const std::string vendor = unhex(vendor_hex);
            std::vector<std::string> tags(n_tags);
            std::vector<const char *> tag_ptrs;
            for (auto &t : tags) {
                std::string h;
                ls >> h;
                t = unhex(h);
                tag_ptrs.push_back(t.c_str());
            }
            o.vendor_string = vendor_hex == "-" ? nullptr : vendor.c_str();
            o.comment_fields = tag_ptrs.data();
            o.n_comment_fields = n_tags;
            ls >> md5_hex >> last_len >> n_cuts;
            std::vector<uint64_t> cuts(n_cuts);
            for (auto &c : cuts) ls >> c;
            std::vector<uint32_t> sizes;
            for (uint32_t s; ls >> s;) sizes.push_back(s);
            const std::string md5 = unhex(md5_hex);
            StreamLedger led;
            std::vector<uint8_t> header;
            int rc = led.open(o, rate, bps, ch, has_total != 0, total, header);
            size_t at = 0;
            for (uint64_t c : cuts) {
                if (rc) break;
                const uint32_t *run = sizes.data() + at;   // exactly c sizes are read from here
                at += c;
                led.frames(c, at == sizes.size() ? last_len : block, [&](uint64_t k) { return run[k]; });
                led.frame_number += c;
            }
            if (!rc && (at != sizes.size() || md5.size() != 16)) {
                fprintf(stderr, "the cuts do not add up to the frames, or no MD5\n");
                return 1;
            }
            if (!rc) rc = led.close(reinterpret_cast<const uint8_t *>(md5.data()), header);
            std::cout << rc << " ";
            for (uint8_t b : header) printf("%02x", b);
            fflush(stdout);
            std::cout << "\n";
        } else if (kind == "admit") {
            uint32_t block, n_runs;
            uint64_t total;
            ls >> block >> total >> n_runs;
            StreamLedger led;
            std::vector<uint8_t> header;
            if (led.open(options_of(block), 44100, 16, 2, true, total, header)) return 1;
            for (uint32_t r = 0; r < n_runs; r++) {
                uint32_t n_frames, last_len;
                ls >> n_frames >> last_len;
                const StreamLedger::Admit a = led.admit(led.samples_written, n_frames, last_len);
                if (a.usable && !a.error) {
                    led.frames(a.usable, a.usable == n_frames ? last_len : block, [](uint64_t) { return 10u; });
                    led.frame_number += a.usable;
                }
                if (a.deferred && !a.error) led.overrun(n_frames, a.usable, last_len);
                std::cout << (r ? " | " : "") << a.usable << " " << a.deferred << " " << a.error << " " << led.samples_written
                          << " " << led.seekpoints.size();
            }
            std::cout << "\n";
        } else if (kind == "verdict") {
            uint64_t known, total, written;
            ls >> known >> total >> written;
            std::cout << totals_verdict(known != 0, total, written) << "\n";
        } else if (kind == "sizes") {
            std::vector<uint32_t> sizes;
            for (uint32_t s; ls >> s;) sizes.push_back(s);
            StreamLedger led;
            std::vector<uint8_t> header;
            if (led.open(options_of(16), 44100, 16, 2, false, 0, header)) return 1;
            led.frames(sizes.size(), 16, [&](uint64_t k) { return sizes[k]; });
            std::cout << led.si.min_frame << " " << led.si.max_frame << "\n";
        } else {
            fprintf(stderr, "unknown case: %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
