// single_paired_driver.cpp -- runs the reference's kaori::SingleBarcodePairedEnd over two FASTQ files and prints what it
// counted.  Built and run by tools/gen_single_paired_golden.py only (the reference's headers are read in place with -I);
// no test and no build step uses it.
//   usage: single_paired_driver <fastq1> <fastq2> <template> <strand 0|1|2> <mismatches> <use_first 0|1> <pool file, one barcode per line>
//   output: "ok <total> <count 0> <count 1> ..." or "error <what()>" (exit status 0 either way; 2 on bad usage)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "kaori/kaori.hpp"
#include "kaori/handlers/SingleBarcodePairedEnd.hpp"
#include "byteme/SomeFileReader.hpp"

template<size_t N>
static void count(const char* f1, const char* f2, const std::string& tmpl, int strand, const kaori::BarcodePool& pool, int mm, bool first) {
    typename kaori::SingleBarcodePairedEnd<N>::Options opt;
    opt.strand = strand == 0 ? kaori::SearchStrand::FORWARD : strand == 1 ? kaori::SearchStrand::REVERSE : kaori::SearchStrand::BOTH;
    opt.max_mismatches = mm;
    opt.use_first = first;
    kaori::SingleBarcodePairedEnd<N> handler(tmpl.c_str(), tmpl.size(), pool, opt);
    byteme::SomeFileReader r1(f1), r2(f2);
    kaori::process_paired_end_data(&r1, &r2, handler, 1);
    std::cout << "ok " << handler.get_total();
    for (int c : handler.get_counts()) std::cout << ' ' << c;
    std::cout << std::endl;
}

int main(int argc, char** argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s fastq1 fastq2 template strand mismatches use_first poolfile\n", argv[0]);
        return 2;
    }
    try {
        const std::string tmpl(argv[3]);
        const int strand = std::atoi(argv[4]), mm = std::atoi(argv[5]);
        const bool first = std::atoi(argv[6]) != 0;
        std::vector<std::string> lines;
        std::ifstream in(argv[7]);
        for (std::string s; std::getline(in, s);) lines.push_back(s);
        kaori::BarcodePool pool(lines);
        if (tmpl.size() <= 32) count<32>(argv[1], argv[2], tmpl, strand, pool, mm, first);
        else if (tmpl.size() <= 64) count<64>(argv[1], argv[2], tmpl, strand, pool, mm, first);
        else if (tmpl.size() <= 128) count<128>(argv[1], argv[2], tmpl, strand, pool, mm, first);
        else if (tmpl.size() <= 256) count<256>(argv[1], argv[2], tmpl, strand, pool, mm, first);
        else throw std::runtime_error("lacking compile-time support for constant regions longer than 256 bp");
    } catch (std::exception& e) {
        std::cout << "error " << e.what() << std::endl;
    }
    return 0;
}
