// ragged_plan_check.cpp -- flacenc_ragged::plan (flac-codec_amd/csrc/host/ragged_plan.h) as a stand-alone program, for a
// build with -fsanitize=address,undefined (tests/test_ragged_plan_host.py).  Every table lives in a heap allocation of
// EXACTLY the size the interface promises -- samples[n], window_of[n], distinct[n_distinct of the accepted plan, found by a
// first pass without tables] -- so a read or write one element past any of them is reported.
//   usage: ragged_plan_check rows.txt      rows: block_size max_partition_order n len_0 .. len_{n-1}
//   prints per row: rc n_distinct pool_doubles | window_of ... | distinct ...      (a refused row: rc and the error text)
#include <stdint.h>
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "ragged_plan.h"

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: ragged_plan_check rows.txt\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        uint32_t block = 0, po = 0, n = 0;
        if (!(ls >> block >> po >> n)) continue;
        std::unique_ptr<uint32_t[]> samples(new uint32_t[n]);   // (n == 0: an allocation of no elements)
        for (uint32_t i = 0; i < n; i++) ls >> samples[i];
        std::string err;
        uint32_t nd = 0;
        uint64_t pool = 0;
        // first pass: no tables at all -- every out pointer may be null
        int rc = flacenc_ragged::plan(block, po, samples.get(), n, nullptr, nullptr, &nd, &pool, &err);
        if (rc) {
            // a refused batch writes nothing: the tables below would be touched at [0] if it did
            std::unique_ptr<uint32_t[]> none(new uint32_t[0]);
            uint32_t nd2 = 77;
            uint64_t pool2 = 77;
            const int rc2 = flacenc_ragged::plan(block, po, samples.get(), n, none.get(), none.get(), &nd2, &pool2, nullptr);
            if (rc2 != rc || nd2 != 77 || pool2 != 77) {
                fprintf(stderr, "a refused batch changed its outputs\n");
                return 1;
            }
            std::cout << rc << " " << err << "\n";
            continue;
        }
        std::unique_ptr<uint32_t[]> window_of(new uint32_t[n]), distinct(new uint32_t[nd]);
        uint32_t nd3 = 0;
        uint64_t pool3 = 0;
        rc = flacenc_ragged::plan(block, po, samples.get(), n, window_of.get(), distinct.get(), &nd3, &pool3, &err);
        if (rc || nd3 != nd || pool3 != pool) {
            fprintf(stderr, "the two passes disagree\n");
            return 1;
        }
        std::cout << rc << " " << nd << " " << pool << " |";
        for (uint32_t i = 0; i < n; i++) std::cout << " " << window_of[i];
        std::cout << " |";
        for (uint32_t i = 0; i < nd; i++) std::cout << " " << distinct[i];
        std::cout << "\n";
    }
    return 0;
}
