// assign_driver.cpp -- runs the reference's kaori::SimpleSingleMatch (search_first or search_best) on every line of a reads
// file and prints the State it leaves.  Built and run by tools/gen_assign_golden.py only (the reference's headers are read
// in place with -I); no test and no build step uses it.
//   usage: assign_driver <reads file, one read per line> <template> <strand 0|1|2> <mismatches> <use_first 0|1> <pool file, one barcode per line>
//   output: per read "index position mismatches variable_mismatches reverse", or "-1 -1 -1 -1 -1" when the search returns
//           false (the fields of State are stale then, not results); "error <what()>" alone when the constructor throws
//           (exit status 0 either way; 2 on bad usage)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "kaori/kaori.hpp"
#include "kaori/SimpleSingleMatch.hpp"

template<size_t N>
static void assign(const std::vector<std::string>& reads, const std::string& tmpl, int strand, const kaori::BarcodePool& pool, int mm, bool first) {
    typename kaori::SimpleSingleMatch<N>::Options opt;
    opt.strand = strand == 0 ? kaori::SearchStrand::FORWARD : strand == 1 ? kaori::SearchStrand::REVERSE : kaori::SearchStrand::BOTH;
    opt.max_mismatches = mm;
    opt.duplicates = kaori::DuplicateAction::ERROR;
    kaori::SimpleSingleMatch<N> matcher(tmpl.c_str(), tmpl.size(), pool, opt);
    auto state = matcher.initialize();
    for (const std::string& r : reads) {
        const bool found = first ? matcher.search_first(r.c_str(), r.size(), state) : matcher.search_best(r.c_str(), r.size(), state);
        if (found) {
            std::cout << state.index << ' ' << state.position << ' ' << state.mismatches << ' ' << state.variable_mismatches << ' '
                      << (state.reverse ? 1 : 0) << '\n';
        } else {
            std::cout << "-1 -1 -1 -1 -1\n";
        }
    }
}

static std::vector<std::string> lines_of(const char* path) {
    std::vector<std::string> lines;
    std::ifstream in(path);
    if (!in) throw std::runtime_error(std::string("cannot open ") + path);
    for (std::string s; std::getline(in, s);) lines.push_back(s);
    return lines;
}

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s reads template strand mismatches use_first poolfile\n", argv[0]);
        return 2;
    }
    try {
        const std::vector<std::string> reads = lines_of(argv[1]);
        const std::string tmpl(argv[2]);
        const int strand = std::atoi(argv[3]), mm = std::atoi(argv[4]);
        const bool first = std::atoi(argv[5]) != 0;
        const std::vector<std::string> barcodes = lines_of(argv[6]);
        kaori::BarcodePool pool(barcodes);
        if (tmpl.size() <= 32) assign<32>(reads, tmpl, strand, pool, mm, first);
        else if (tmpl.size() <= 64) assign<64>(reads, tmpl, strand, pool, mm, first);
        else if (tmpl.size() <= 128) assign<128>(reads, tmpl, strand, pool, mm, first);
        else if (tmpl.size() <= 256) assign<256>(reads, tmpl, strand, pool, mm, first);
        else throw std::runtime_error("lacking compile-time support for constant regions longer than 256 bp");
    } catch (std::exception& e) {
        std::cout << "error " << e.what() << std::endl;
    }
    return 0;
}
