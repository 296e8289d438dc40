// combo_regions_driver.cpp -- runs the reference's kaori::CombinatorialBarcodesSingleEnd<256, V> over a FASTQ file for the
// number of variable regions V = the number of pools given (1 to 8), and prints the combinations it counted.  Built and run by
// tools/gen_combo_regions_golden.py only (the reference's headers are read in place with -I); no test and no build step
// uses it.
//   usage: combo_regions_driver <fastq> <template> <strand 0|1|2> <mismatches> <use_first 0|1> <pool file>
//          pool file: one barcode per line, a line ">" before every pool
//   output: "ok <total> <K>" and K lines "<index 0> ... <index V-1> <count>" in the handler's sorted order, or
//           "error <what()>" (exit status 0 either way; 2 on bad usage)
#include <stdexcept>
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kaori/kaori.hpp"
#include "kaori/handlers/CombinatorialBarcodesSingleEnd.hpp"
#include "byteme/SomeFileReader.hpp"

template<size_t V>
static void count(const char* fastq, const std::string& tmpl, int strand, const std::vector<std::vector<std::string> >& lines, int mm, bool first) {
    std::vector<kaori::BarcodePool> pools;
    for (const auto& p : lines) pools.emplace_back(p);
    typename kaori::CombinatorialBarcodesSingleEnd<256, V>::Options opt;
    opt.strand = strand == 0 ? kaori::SearchStrand::FORWARD : strand == 1 ? kaori::SearchStrand::REVERSE : kaori::SearchStrand::BOTH;
    opt.max_mismatches = mm;
    opt.use_first = first;
    kaori::CombinatorialBarcodesSingleEnd<256, V> handler(tmpl.c_str(), tmpl.size(), pools, opt);
    byteme::SomeFileReader reader(fastq);
    kaori::process_single_end_data(&reader, handler, 1);
    handler.sort();
    const std::vector<std::array<int, V> >& found = handler.get_combinations();
    std::vector<size_t> starts;
    for (size_t i = 0; i < found.size(); ++i) {
        if (i == 0 || found[i] != found[i - 1]) starts.push_back(i);
    }
    std::cout << "ok " << handler.get_total() << ' ' << starts.size() << '\n';
    for (size_t s = 0; s < starts.size(); ++s) {
        for (int x : found[starts[s]]) std::cout << x << ' ';
        std::cout << (s + 1 < starts.size() ? starts[s + 1] : found.size()) - starts[s] << '\n';
    }
    std::cout.flush();
}

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s fastq template strand mismatches use_first poolfile\n", argv[0]);
        return 2;
    }
    try {
        const std::string tmpl(argv[2]);
        const int strand = std::atoi(argv[3]), mm = std::atoi(argv[4]);
        const bool first = std::atoi(argv[5]) != 0;
        std::vector<std::vector<std::string> > lines;
        std::ifstream in(argv[6]);
        for (std::string s; std::getline(in, s);) {
            if (s == ">") lines.emplace_back();
            else if (!lines.empty()) lines.back().push_back(s);
        }
        if (tmpl.size() > 256) throw std::runtime_error("lacking compile-time support for constant regions longer than 256 bp");
        switch (lines.size()) {
        case 1: count<1>(argv[1], tmpl, strand, lines, mm, first); break;
        case 2: count<2>(argv[1], tmpl, strand, lines, mm, first); break;
        case 3: count<3>(argv[1], tmpl, strand, lines, mm, first); break;
        case 4: count<4>(argv[1], tmpl, strand, lines, mm, first); break;
        case 5: count<5>(argv[1], tmpl, strand, lines, mm, first); break;
        case 6: count<6>(argv[1], tmpl, strand, lines, mm, first); break;
        case 7: count<7>(argv[1], tmpl, strand, lines, mm, first); break;
        case 8: count<8>(argv[1], tmpl, strand, lines, mm, first); break;
        default: std::fprintf(stderr, "1 to 8 pools\n"); return 2;
        }
    } catch (std::exception& e) {
        std::cout << "error " << e.what() << std::endl;
    }
    return 0;
}
