// shim/scg_shim.cpp -- the Rcpp glue a screenCounter maintainer drops into src/ in place of the bodies of
// src/count_single_barcodes.cpp, src/count_combo_barcodes_single.cpp, src/count_dual_barcodes.cpp,
// src/count_combo_barcodes_paired.cpp, src/count_dual_barcodes_single_end.cpp, src/count_random_barcodes.cpp and
// src/match_barcodes.cpp of the reference.  The exported signatures are the reference's own
// (src/RcppExports.cpp:136-145: arity 7 / 7 / 14 / 13 / 8 / 6 / 4), so R/RcppExports.R and every R/*.R file stay
// unchanged.  Each function: borrow the CHARSXP pointers, call the C ABI of include/scg.h, turn a non-zero
// return into Rcpp::stop (what END_RCPP does with the reference's std::runtime_error).
//
// R is not present in this repository's build image, so the file is compiled only for syntax there, against
// the type-level stand-in tests/fake_rcpp/Rcpp.h (tests/test_shim.py); with the real Rcpp it builds as part
// of the package: PKG_CPPFLAGS=-I<repo>/include, PKG_LIBS=-L<repo>/screencounter_amd -lscg.
#include "Rcpp.h"
#include "scg.h"
#include <algorithm>
#include <string>
#include <vector>

namespace {
// R CHARSXPs are NUL-terminated; libscg checks "all the same length" itself (src/utils.cpp:5-23).
std::vector<const char*> borrow(const Rcpp::CharacterVector& x) {
    std::vector<const char*> p(x.size());
    for (R_xlen_t i = 0; i < x.size(); ++i) p[i] = CHAR(STRING_ELT(x, i));
    return p;
}
void check(int rc, const char* err) { if (rc != SCG_OK) Rcpp::stop(err); }

// Combinations as libscg hands them out (malloc'd: 2 x K indices, column-major and 0-based, sorted by (first, second); K
// frequencies) -> what R gets.
Rcpp::IntegerMatrix combination_indices(const int32_t* idx, int64_t k, int rows = 2) {     // (rows: the variable regions, where not 2)
    Rcpp::IntegerMatrix m(rows, k);
    std::copy(idx, idx + rows * k, m.begin());
    return m;
}
Rcpp::IntegerVector combination_counts(const int32_t* freq, int64_t k) { return Rcpp::IntegerVector(freq, freq + k); }

// The (indices, frequencies, K) outputs of a one-file entry.  Released when this goes out of scope: after the copies are
// made, and also when an allocation on the R side throws before that.
struct Combinations {
    int32_t *idx = nullptr, *freq = nullptr;
    int64_t k = 0;
    Combinations() {}
    Combinations(const Combinations&) = delete;
    Combinations& operator=(const Combinations&) = delete;
    ~Combinations() { scg_free(idx); scg_free(freq); }
    Rcpp::IntegerMatrix indices() const { return combination_indices(idx, k); }
    Rcpp::IntegerVector counts() const { return combination_counts(freq, k); }
    Rcpp::List both() const { return Rcpp::List::create(indices(), counts()); }
};

// The same per file, in the arrays of n_files entries a many-files entry fills: file f's 2 x K_f matrix of indices and its
// K_f frequencies.  All of them are released when this goes out of scope, also when an allocation on the R side throws
// half-way through the files.
struct PerFileCombinations {
    std::vector<int32_t*> idx, freq;
    std::vector<int64_t> k;
    explicit PerFileCombinations(size_t n_files) : idx(n_files, nullptr), freq(n_files, nullptr), k(n_files, 0) {}
    PerFileCombinations(const PerFileCombinations&) = delete;
    PerFileCombinations& operator=(const PerFileCombinations&) = delete;
    ~PerFileCombinations() { for (size_t f = 0; f < idx.size(); ++f) { scg_free(idx[f]); scg_free(freq[f]); } }
    Rcpp::IntegerMatrix indices(R_xlen_t f) const { return combination_indices(idx[f], k[f]); }
    Rcpp::IntegerVector counts(R_xlen_t f) const { return combination_counts(freq[f], k[f]); }
    Rcpp::List both(R_xlen_t f) const { return Rcpp::List::create(indices(f), counts(f)); }
};
}

//[[Rcpp::export(rng=false)]]
Rcpp::List count_single_barcodes(std::string path, std::string constant, int strand, Rcpp::CharacterVector pool,
                                 int mismatches, bool use_first, int nthreads) {
    auto p = borrow(pool);
    Rcpp::IntegerVector counts(pool.size());
    int total = 0;
    char err[1024];
    check(scg_count_single_barcodes(path.c_str(), constant.c_str(), strand, p.data(), (int32_t)p.size(),
                                    mismatches, use_first, nthreads, counts.begin(), &total, err, sizeof(err)), err);
    return Rcpp::List::create(counts, total);          // same shape as src/count_single_barcodes.cpp:49
}

//[[Rcpp::export(rng=false)]]
Rcpp::List count_combo_barcodes_single(std::string path, std::string constant, int strand, Rcpp::List pool,
                                       int mismatches, bool use_first, int nthreads) {
    if (pool.size() != 2) Rcpp::stop("currently expecting only 2 variable regions for single-end combinatorial barcodes");
    Rcpp::CharacterVector c0(pool[0]), c1(pool[1]);
    auto p0 = borrow(c0), p1 = borrow(c1);
    Combinations found; int total = 0;
    char err[1024];
    check(scg_count_combo_barcodes_single(path.c_str(), constant.c_str(), strand, p0.data(), (int32_t)p0.size(),
                                          p1.data(), (int32_t)p1.size(), mismatches, use_first, nthreads,
                                          &found.idx, &found.freq, &found.k, &total, err, sizeof(err)), err);
    return Rcpp::List::create(found.indices(), found.counts(), Rcpp::IntegerVector::create(total));   // src/count_combo_barcodes_single.cpp:32-36
}

//[[Rcpp::export(rng=false)]]
Rcpp::List count_dual_barcodes(std::string path1, std::string constant1, bool reverse1, int mismatches1, Rcpp::CharacterVector pool1,
                               std::string path2, std::string constant2, bool reverse2, int mismatches2, Rcpp::CharacterVector pool2,
                               bool randomized, bool use_first, bool diagnostics, int nthreads) {
    if (pool1.size() != pool2.size()) Rcpp::stop("both barcode pools should be of the same length");
    auto p1 = borrow(pool1), p2 = borrow(pool2);
    Rcpp::IntegerVector counts(pool1.size());
    int total = 0;
    char err[1024];
    if (diagnostics) {                                  // include.invalid=TRUE: 5-list of src/count_dual_barcodes.cpp:64-70
        Combinations invalid; int b1 = 0, b2 = 0;
        check(scg_count_dual_barcodes_diagnostics(path1.c_str(), constant1.c_str(), reverse1, mismatches1, p1.data(),
                                                  path2.c_str(), constant2.c_str(), reverse2, mismatches2, p2.data(), (int32_t)p1.size(),
                                                  randomized, use_first, nthreads, counts.begin(), &invalid.idx, &invalid.freq, &invalid.k,
                                                  &total, &b1, &b2, err, sizeof(err)), err);
        return Rcpp::List::create(counts, invalid.both(), Rcpp::IntegerVector::create(total),
                                  Rcpp::IntegerVector::create(b1), Rcpp::IntegerVector::create(b2));
    }
    check(scg_count_dual_barcodes(path1.c_str(), constant1.c_str(), reverse1, mismatches1, p1.data(),
                                  path2.c_str(), constant2.c_str(), reverse2, mismatches2, p2.data(), (int32_t)p1.size(),
                                  randomized, use_first, diagnostics, nthreads, counts.begin(), &total, err, sizeof(err)), err);
    return Rcpp::List::create(counts, Rcpp::IntegerVector::create(total));            // src/count_dual_barcodes.cpp:47-50
}

//[[Rcpp::export(rng=false)]]
Rcpp::List count_random_barcodes(std::string path, std::string constant, int strand, int mismatches, bool use_first, int nthreads) {
    char* seqs = nullptr; int32_t* freq = nullptr; int64_t k = 0; int32_t len = 0; int total = 0;
    char err[1024];
    check(scg_count_random_barcodes(path.c_str(), constant.c_str(), strand, mismatches, use_first, nthreads,
                                    &seqs, &freq, &k, &len, &total, err, sizeof(err)), err);
    Rcpp::CharacterVector sequences(k);
    for (int64_t i = 0; i < k; ++i) sequences[i] = std::string(seqs + i * (len + 1), len);
    Rcpp::IntegerVector frequencies(freq, freq + k);
    scg_free(seqs); scg_free(freq);
    return Rcpp::List::create(Rcpp::List::create(sequences, frequencies), total);           // src/count_random_barcodes.cpp:61
}

//[[Rcpp::export(rng=false)]]
Rcpp::List count_dual_barcodes_single_end(std::string path, std::string constant, Rcpp::List pools, int strand, int mismatches,
                                          bool use_first, bool diagnostics, int nthreads) {
    std::vector<std::vector<const char*> > cols;           // one pool per variable region
    std::vector<const char* const*> rows;
    std::vector<int32_t> sizes;
    for (R_xlen_t p = 0; p < pools.size(); ++p) {
        cols.push_back(borrow(Rcpp::CharacterVector(pools[p])));
        sizes.push_back((int32_t)cols.back().size());
    }
    for (auto& c : cols) rows.push_back(c.data());
    Rcpp::IntegerVector counts(sizes.empty() ? 0 : sizes[0]);
    int total = 0;
    char err[1024];
    if (diagnostics) {                                  // 3-list of src/count_dual_barcodes_single_end.cpp:44-48
        Combinations invalid;
        check(scg_count_dual_barcodes_single_end_diagnostics(path.c_str(), constant.c_str(), rows.data(), sizes.data(), (int32_t)rows.size(),
                                                             strand, mismatches, use_first, nthreads, counts.begin(),
                                                             &invalid.idx, &invalid.freq, &invalid.k, &total, err, sizeof(err)), err);
        return Rcpp::List::create(counts, invalid.both(), Rcpp::IntegerVector::create(total));
    }
    check(scg_count_dual_barcodes_single_end(path.c_str(), constant.c_str(), rows.data(), sizes.data(), (int32_t)rows.size(),
                                             strand, mismatches, use_first, diagnostics, nthreads, counts.begin(), &total, err, sizeof(err)), err);
    return Rcpp::List::create(counts, Rcpp::IntegerVector::create(total));     // src/count_dual_barcodes_single_end.cpp:31-34
}

//[[Rcpp::export(rng=false)]]
Rcpp::List count_combo_barcodes_paired(std::string path1, std::string constant1, bool reverse1, int mismatches1, Rcpp::CharacterVector pool1,
                                       std::string path2, std::string constant2, bool reverse2, int mismatches2, Rcpp::CharacterVector pool2,
                                       bool randomized, bool use_first, int nthreads) {
    auto p1 = borrow(pool1), p2 = borrow(pool2);
    Combinations found; int total = 0, b1 = 0, b2 = 0;
    char err[1024];
    check(scg_count_combo_barcodes_paired(path1.c_str(), constant1.c_str(), reverse1, mismatches1, p1.data(), (int32_t)p1.size(),
                                          path2.c_str(), constant2.c_str(), reverse2, mismatches2, p2.data(), (int32_t)p2.size(),
                                          randomized, use_first, nthreads, &found.idx, &found.freq, &found.k, &total, &b1, &b2,
                                          err, sizeof(err)), err);
    return Rcpp::List::create(found.indices(), found.counts(), Rcpp::IntegerVector::create(total),   // src/count_combo_barcodes_paired.cpp:47-54
                              Rcpp::IntegerVector::create(b1), Rcpp::IntegerVector::create(b2));
}

//[[Rcpp::export(rng=false)]]
Rcpp::List match_barcodes(Rcpp::CharacterVector sequences, Rcpp::CharacterVector choices, int substitutions, bool reverse) {
    auto s = borrow(sequences), c = borrow(choices);
    Rcpp::IntegerVector id(sequences.size()), mm(sequences.size());
    char err[1024];
    check(scg_match_barcodes(s.data(), (int32_t)s.size(), c.data(), (int32_t)c.size(), substitutions, reverse,
                             id.begin(), mm.begin(), err, sizeof(err)), err);
    for (R_xlen_t i = 0; i < id.size(); ++i) {          // 0-based / -1  ->  1-based / NA (src/match_barcodes.cpp:24-31)
        if (id[i] < 0) { id[i] = NA_INTEGER; mm[i] = NA_INTEGER; } else { id[i] += 1; }
    }
    return Rcpp::List::create(id, mm);
}

// ---------------------------------------------------------------------------------------------------------------
// Many files in one native call: optional additions for the matrixOf* functions.  With these eight exported, e.g.
// matrixOfSingleBarcodes (R/countSingleBarcodes.R:112-126) replaces its
//     out <- bplapply(files, FUN=countSingleBarcodes, ..., BPPARAM=BPPARAM)
// by one call whose result it unpacks into the same per-file list; libscg schedules the files over the GPUs itself
// (one file at a time per device, library compiled once), so no BiocParallel worker processes are needed.  The same
// goes for matrixOfDualBarcodes (with and without include.invalid), matrixOfDualBarcodesSingleEnd (likewise),
// matrixOfPairedComboBarcodes and matrixOfRandomBarcodes: INTEGRATION.md lists which wrapper reaches which export.
// ---------------------------------------------------------------------------------------------------------------

//[[Rcpp::export(rng=false)]]
Rcpp::List count_single_barcodes_files(Rcpp::CharacterVector paths, std::string constant, int strand, Rcpp::CharacterVector pool,
                                       int mismatches, bool use_first, int nthreads) {
    auto f = borrow(paths), p = borrow(pool);
    Rcpp::IntegerMatrix counts((int)pool.size(), paths.size());     // column f = file f
    Rcpp::IntegerVector totals(paths.size());
    char err[1024];
    check(scg_count_single_barcodes_files(f.data(), (int32_t)f.size(), constant.c_str(), strand, p.data(), (int32_t)p.size(),
                                          mismatches, use_first, nthreads, counts.begin(), totals.begin(), err, sizeof(err)), err);
    return Rcpp::List::create(counts, totals);
}

// kaori::SingleBarcodePairedEnd (handlers/SingleBarcodePairedEnd.hpp:93-124): no R/ wrapper in the reference; INTEGRATION.md has the .Call.
//[[Rcpp::export(rng=false)]]
Rcpp::List count_single_barcodes_paired(std::string path1, std::string path2, std::string constant, int strand, Rcpp::CharacterVector pool,
                                        int mismatches, bool use_first, int nthreads) {
    auto p = borrow(pool);
    Rcpp::IntegerVector counts(pool.size());
    int total = 0;
    char err[1024];
    check(scg_count_single_barcodes_paired(path1.c_str(), path2.c_str(), constant.c_str(), strand, p.data(), (int32_t)p.size(),
                                           mismatches, use_first, nthreads, counts.begin(), &total, err, sizeof(err)), err);
    return Rcpp::List::create(counts, total);
}

//[[Rcpp::export(rng=false)]]
Rcpp::List count_single_barcodes_paired_files(Rcpp::CharacterVector paths1, Rcpp::CharacterVector paths2, std::string constant, int strand,
                                              Rcpp::CharacterVector pool, int mismatches, bool use_first, int nthreads) {
    if (paths1.size() != paths2.size()) Rcpp::stop("'paths1' and 'paths2' should be of the same length");
    auto f1 = borrow(paths1), f2 = borrow(paths2), p = borrow(pool);
    Rcpp::IntegerMatrix counts((int)pool.size(), paths1.size());    // column f = file f
    Rcpp::IntegerVector totals(paths1.size());
    char err[1024];
    check(scg_count_single_barcodes_paired_files(f1.data(), f2.data(), (int32_t)f1.size(), constant.c_str(), strand, p.data(), (int32_t)p.size(),
                                                 mismatches, use_first, nthreads, counts.begin(), totals.begin(), err, sizeof(err)), err);
    return Rcpp::List::create(counts, totals);
}

//[[Rcpp::export(rng=false)]]
Rcpp::List count_combo_barcodes_single_files(Rcpp::CharacterVector paths, std::string constant, int strand, Rcpp::List pool,
                                             int mismatches, bool use_first, int nthreads) {
    if (pool.size() != 2) Rcpp::stop("currently expecting only 2 variable regions for single-end combinatorial barcodes");
    Rcpp::CharacterVector c0(pool[0]), c1(pool[1]);
    auto f = borrow(paths), p0 = borrow(c0), p1 = borrow(c1);
    PerFileCombinations found(f.size());
    Rcpp::IntegerVector totals(paths.size());
    char err[1024];
    check(scg_count_combo_barcodes_single_files(f.data(), (int32_t)f.size(), constant.c_str(), strand, p0.data(), (int32_t)p0.size(),
                                                p1.data(), (int32_t)p1.size(), mismatches, use_first, nthreads,
                                                found.idx.data(), found.freq.data(), found.k.data(), totals.begin(), err, sizeof(err)), err);
    Rcpp::List out(paths.size());                        // one count_combo_barcodes_single() result per file
    for (R_xlen_t i = 0; i < paths.size(); ++i) {
        out[i] = Rcpp::List::create(found.indices(i), found.counts(i), Rcpp::IntegerVector::create(totals[i]));
    }
    return out;
}

//[[Rcpp::export(rng=false)]]
Rcpp::List count_dual_barcodes_files(Rcpp::CharacterVector paths1, std::string constant1, bool reverse1, int mismatches1, Rcpp::CharacterVector pool1,
                                     Rcpp::CharacterVector paths2, std::string constant2, bool reverse2, int mismatches2, Rcpp::CharacterVector pool2,
                                     bool randomized, bool use_first, int nthreads) {
    if (pool1.size() != pool2.size()) Rcpp::stop("both barcode pools should be of the same length");
    if (paths1.size() != paths2.size()) Rcpp::stop("'paths1' and 'paths2' should be of the same length");
    auto f1 = borrow(paths1), f2 = borrow(paths2), p1 = borrow(pool1), p2 = borrow(pool2);
    Rcpp::IntegerMatrix counts((int)pool1.size(), paths1.size());
    Rcpp::IntegerVector totals(paths1.size());
    char err[1024];
    check(scg_count_dual_barcodes_files(f1.data(), constant1.c_str(), reverse1, mismatches1, p1.data(),
                                        f2.data(), constant2.c_str(), reverse2, mismatches2, p2.data(), (int32_t)p1.size(), (int32_t)f1.size(),
                                        randomized, use_first, nthreads, counts.begin(), totals.begin(), err, sizeof(err)), err);
    return Rcpp::List::create(counts, totals);
}

namespace {
// A list of pools (one per variable region) as the rows libscg takes.
struct PoolRows {
    std::vector<std::vector<const char*> > cols;
    std::vector<const char* const*> rows;
    std::vector<int32_t> sizes;
    explicit PoolRows(const Rcpp::List& pools) {
        for (R_xlen_t p = 0; p < pools.size(); ++p) {
            cols.push_back(borrow(Rcpp::CharacterVector(pools[p])));
            sizes.push_back((int32_t)cols.back().size());
        }
        for (auto& c : cols) rows.push_back(c.data());
    }
};
}

// matrixOfDualBarcodes(include.invalid=TRUE): List(counts matrix, per-file List(indices, frequencies), totals,
// barcode-1-only, barcode-2-only) -- per file what count_dual_barcodes(diagnostics=TRUE) returns.
//[[Rcpp::export(rng=false)]]
Rcpp::List count_dual_barcodes_diagnostics_files(Rcpp::CharacterVector paths1, std::string constant1, bool reverse1, int mismatches1,
                                                 Rcpp::CharacterVector pool1,
                                                 Rcpp::CharacterVector paths2, std::string constant2, bool reverse2, int mismatches2,
                                                 Rcpp::CharacterVector pool2, bool randomized, bool use_first, int nthreads) {
    if (pool1.size() != pool2.size()) Rcpp::stop("both barcode pools should be of the same length");
    if (paths1.size() != paths2.size()) Rcpp::stop("'paths1' and 'paths2' should be of the same length");
    auto f1 = borrow(paths1), f2 = borrow(paths2), p1 = borrow(pool1), p2 = borrow(pool2);
    PerFileCombinations found(f1.size());
    Rcpp::IntegerMatrix counts((int)pool1.size(), paths1.size());
    Rcpp::IntegerVector totals(paths1.size()), b1(paths1.size()), b2(paths1.size());
    char err[1024];
    check(scg_count_dual_barcodes_diagnostics_files(f1.data(), constant1.c_str(), reverse1, mismatches1, p1.data(),
                                                    f2.data(), constant2.c_str(), reverse2, mismatches2, p2.data(), (int32_t)p1.size(),
                                                    (int32_t)f1.size(), randomized, use_first, nthreads, counts.begin(),
                                                    found.idx.data(), found.freq.data(), found.k.data(), totals.begin(), b1.begin(), b2.begin(),
                                                    err, sizeof(err)), err);
    Rcpp::List invalid(paths1.size());
    for (R_xlen_t i = 0; i < paths1.size(); ++i) invalid[i] = found.both(i);
    return Rcpp::List::create(counts, invalid, totals, b1, b2);
}

// matrixOfDualBarcodesSingleEnd: List(counts matrix, totals).
//[[Rcpp::export(rng=false)]]
Rcpp::List count_dual_barcodes_single_end_files(Rcpp::CharacterVector paths, std::string constant, Rcpp::List pools, int strand,
                                                int mismatches, bool use_first, int nthreads) {
    auto f = borrow(paths);
    PoolRows p(pools);
    Rcpp::IntegerMatrix counts(p.sizes.empty() ? 0 : p.sizes[0], paths.size());
    Rcpp::IntegerVector totals(paths.size());
    char err[1024];
    check(scg_count_dual_barcodes_single_end_files(f.data(), (int32_t)f.size(), constant.c_str(), p.rows.data(), p.sizes.data(),
                                                   (int32_t)p.rows.size(), strand, mismatches, use_first, nthreads,
                                                   counts.begin(), totals.begin(), err, sizeof(err)), err);
    return Rcpp::List::create(counts, totals);
}

// matrixOfDualBarcodesSingleEnd(include.invalid=TRUE): List(counts matrix, per-file List(indices, frequencies), totals).
//[[Rcpp::export(rng=false)]]
Rcpp::List count_dual_barcodes_single_end_diagnostics_files(Rcpp::CharacterVector paths, std::string constant, Rcpp::List pools, int strand,
                                                            int mismatches, bool use_first, int nthreads) {
    auto f = borrow(paths);
    PoolRows p(pools);
    PerFileCombinations found(f.size());
    Rcpp::IntegerMatrix counts(p.sizes.empty() ? 0 : p.sizes[0], paths.size());
    Rcpp::IntegerVector totals(paths.size());
    char err[1024];
    check(scg_count_dual_barcodes_single_end_diagnostics_files(f.data(), (int32_t)f.size(), constant.c_str(), p.rows.data(), p.sizes.data(),
                                                               (int32_t)p.rows.size(), strand, mismatches, use_first, nthreads,
                                                               counts.begin(), found.idx.data(), found.freq.data(), found.k.data(), totals.begin(),
                                                               err, sizeof(err)), err);
    Rcpp::List invalid(paths.size());
    for (R_xlen_t i = 0; i < paths.size(); ++i) invalid[i] = found.both(i);
    return Rcpp::List::create(counts, invalid, totals);
}

// matrixOfPairedComboBarcodes: one count_combo_barcodes_paired() result per pair of files.
//[[Rcpp::export(rng=false)]]
Rcpp::List count_combo_barcodes_paired_files(Rcpp::CharacterVector paths1, std::string constant1, bool reverse1, int mismatches1,
                                             Rcpp::CharacterVector pool1,
                                             Rcpp::CharacterVector paths2, std::string constant2, bool reverse2, int mismatches2,
                                             Rcpp::CharacterVector pool2, bool randomized, bool use_first, int nthreads) {
    if (paths1.size() != paths2.size()) Rcpp::stop("'paths1' and 'paths2' should be of the same length");
    auto f1 = borrow(paths1), f2 = borrow(paths2), p1 = borrow(pool1), p2 = borrow(pool2);
    PerFileCombinations found(f1.size());
    Rcpp::IntegerVector totals(paths1.size()), b1(paths1.size()), b2(paths1.size());
    char err[1024];
    check(scg_count_combo_barcodes_paired_files(f1.data(), constant1.c_str(), reverse1, mismatches1, p1.data(), (int32_t)p1.size(),
                                                f2.data(), constant2.c_str(), reverse2, mismatches2, p2.data(), (int32_t)p2.size(),
                                                (int32_t)f1.size(), randomized, use_first, nthreads,
                                                found.idx.data(), found.freq.data(), found.k.data(), totals.begin(), b1.begin(), b2.begin(),
                                                err, sizeof(err)), err);
    Rcpp::List out(paths1.size());
    for (R_xlen_t i = 0; i < paths1.size(); ++i) {
        out[i] = Rcpp::List::create(found.indices(i), found.counts(i), Rcpp::IntegerVector::create(totals[i]),
                                    Rcpp::IntegerVector::create(b1[i]), Rcpp::IntegerVector::create(b2[i]));
    }
    return out;
}

// matrixOfRandomBarcodes (R/countRandomBarcodes.R:84-104): List(sequences, counts matrix, totals) -- the rows are the sorted
// union of the files' sequences, column f what count_random_barcodes() counts in file f, zero where it found none.
//[[Rcpp::export(rng=false)]]
Rcpp::List count_random_barcodes_files(Rcpp::CharacterVector paths, std::string constant, int strand, int mismatches, bool use_first,
                                       int nthreads) {
    auto f = borrow(paths);
    char* seqs = nullptr; int64_t* col_ptr = nullptr; int32_t *rows = nullptr, *freq = nullptr; int64_t k = 0; int32_t len = 0;
    Rcpp::IntegerVector totals(paths.size());
    char err[1024];
    check(scg_count_random_barcodes_files(f.data(), (int32_t)f.size(), constant.c_str(), strand, mismatches, use_first, nthreads,
                                          &seqs, &k, &len, &col_ptr, &rows, &freq, totals.begin(), err, sizeof(err)), err);
    // (the arrays are released below also when an allocation on the R side throws)
    struct Release { void *a, *b, *c, *d; ~Release() { scg_free(a); scg_free(b); scg_free(c); scg_free(d); } } release{seqs, col_ptr, rows, freq};
    Rcpp::CharacterVector sequences(k);
    for (int64_t i = 0; i < k; ++i) sequences[i] = std::string(seqs + i * (len + 1), len);
    Rcpp::IntegerMatrix counts((int)k, paths.size());               // zero-filled; column f = file f
    for (R_xlen_t c = 0; c < paths.size(); ++c) {
        int* column = counts.column_begin(c);
        for (int64_t j = col_ptr[c]; j < col_ptr[c + 1]; ++j) column[rows[j]] = freq[j];
    }
    return Rcpp::List::create(sequences, counts, totals);
}

namespace {
// The combination matrix as libscg hands it out (include/scg.h, "Combination counts of many files as one matrix"): the
// union's 2 x K indices and the files' columns in compressed form.  Released when this goes out of scope.
struct CombinationMatrix {
    int32_t *idx = nullptr, *rows = nullptr, *freq = nullptr;
    int64_t* col_ptr = nullptr;
    int64_t k = 0;
    CombinationMatrix() {}
    CombinationMatrix(const CombinationMatrix&) = delete;
    CombinationMatrix& operator=(const CombinationMatrix&) = delete;
    ~CombinationMatrix() { scg_free(idx); scg_free(rows); scg_free(freq); scg_free(col_ptr); }
    Rcpp::IntegerMatrix indices() const { return combination_indices(idx, k); }
    // K x n_files, zero-filled; column f = file f: the out.counts of R/combineComboCounts.R:45-54
    Rcpp::IntegerMatrix counts(R_xlen_t n_files) const {
        Rcpp::IntegerMatrix m((int)k, n_files);
        for (R_xlen_t c = 0; c < n_files; ++c) {
            int* column = m.column_begin(c);
            for (int64_t j = col_ptr[c]; j < col_ptr[c + 1]; ++j) column[rows[j]] = freq[j];
        }
        return m;
    }
};
}

// matrixOfComboBarcodes after its combineComboCounts: List(indices 2 x K, counts K x n_files, totals).  Rows are sorted by
// (first index, second index); with indices=FALSE the R wrapper reorders them by the barcode strings.
//[[Rcpp::export(rng=false)]]
Rcpp::List count_combo_barcodes_single_matrix(Rcpp::CharacterVector paths, std::string constant, int strand, Rcpp::List pool,
                                              int mismatches, bool use_first, int nthreads) {
    if (pool.size() != 2) Rcpp::stop("currently expecting only 2 variable regions for single-end combinatorial barcodes");
    Rcpp::CharacterVector c0(pool[0]), c1(pool[1]);
    auto f = borrow(paths), p0 = borrow(c0), p1 = borrow(c1);
    CombinationMatrix found;
    Rcpp::IntegerVector totals(paths.size());
    char err[1024];
    check(scg_count_combo_barcodes_single_matrix(f.data(), (int32_t)f.size(), constant.c_str(), strand, p0.data(), (int32_t)p0.size(),
                                                 p1.data(), (int32_t)p1.size(), mismatches, use_first, nthreads,
                                                 &found.idx, &found.k, &found.col_ptr, &found.rows, &found.freq, totals.begin(), err, sizeof(err)), err);
    return Rcpp::List::create(found.indices(), found.counts(paths.size()), totals);
}

// matrixOfPairedComboBarcodes after its combineComboCounts: List(indices, counts, totals, barcode-1-only, barcode-2-only).
//[[Rcpp::export(rng=false)]]
Rcpp::List count_combo_barcodes_paired_matrix(Rcpp::CharacterVector paths1, std::string constant1, bool reverse1, int mismatches1,
                                              Rcpp::CharacterVector pool1,
                                              Rcpp::CharacterVector paths2, std::string constant2, bool reverse2, int mismatches2,
                                              Rcpp::CharacterVector pool2, bool randomized, bool use_first, int nthreads) {
    if (paths1.size() != paths2.size()) Rcpp::stop("'paths1' and 'paths2' should be of the same length");
    auto f1 = borrow(paths1), f2 = borrow(paths2), p1 = borrow(pool1), p2 = borrow(pool2);
    CombinationMatrix found;
    Rcpp::IntegerVector totals(paths1.size()), b1(paths1.size()), b2(paths1.size());
    char err[1024];
    check(scg_count_combo_barcodes_paired_matrix(f1.data(), constant1.c_str(), reverse1, mismatches1, p1.data(), (int32_t)p1.size(),
                                                 f2.data(), constant2.c_str(), reverse2, mismatches2, p2.data(), (int32_t)p2.size(),
                                                 (int32_t)f1.size(), randomized, use_first, nthreads,
                                                 &found.idx, &found.k, &found.col_ptr, &found.rows, &found.freq,
                                                 totals.begin(), b1.begin(), b2.begin(), err, sizeof(err)), err);
    return Rcpp::List::create(found.indices(), found.counts(paths1.size()), totals, b1, b2);
}

// combineComboCounts (R/combineComboCounts.R:31-57) for lists R already holds, in the form its own first step gives them:
// the DataFrames bound together -- `first` and `second` (0-based indices) and `counts` of all of them back to back -- and
// `sizes`, the number of rows of each.  List(indices 2 x K, counts K x length(sizes)).
//[[Rcpp::export(rng=false)]]
Rcpp::List combine_combinations(Rcpp::IntegerVector first, Rcpp::IntegerVector second, Rcpp::IntegerVector counts, Rcpp::IntegerVector sizes) {
    if (first.size() != second.size() || first.size() != counts.size()) Rcpp::stop("'first', 'second' and 'counts' should be of the same length");
    const R_xlen_t n_files = sizes.size();
    std::vector<int32_t> pairs(2 * (size_t)first.size() + 2);
    for (R_xlen_t i = 0; i < first.size(); ++i) { pairs[2 * i] = first[i]; pairs[2 * i + 1] = second[i]; }
    std::vector<const int32_t*> idx(n_files + 1), freq(n_files + 1);
    std::vector<int64_t> k(n_files + 1);
    R_xlen_t at = 0;
    for (R_xlen_t f = 0; f < n_files; ++f) {
        if (sizes[f] < 0 || sizes[f] > first.size() - at) Rcpp::stop("'sizes' should add up to the number of combinations");
        idx[f] = pairs.data() + 2 * at; freq[f] = counts.begin() + at; k[f] = sizes[f];
        at += sizes[f];
    }
    if (at != first.size()) Rcpp::stop("'sizes' should add up to the number of combinations");
    CombinationMatrix found;
    char err[1024];
    check(scg_combine_combinations(idx.data(), freq.data(), k.data(), (int32_t)n_files,
                                   &found.idx, &found.k, &found.col_ptr, &found.rows, &found.freq, err, sizeof(err)), err);
    return Rcpp::List::create(found.indices(), found.counts(n_files));
}

// Combinations over any number of variable regions (kaori::CombinatorialBarcodesSingleEnd<N, V> for V = length(pool), 1 to
// 8): count_combo_barcodes_single's arguments and result shape, the matrix of indices having one row per region.
//[[Rcpp::export(rng=false)]]
Rcpp::List count_combo_barcodes_regions(std::string path, std::string constant, int strand, Rcpp::List pool,
                                        int mismatches, bool use_first, int nthreads) {
    PoolRows pools(pool);
    Combinations found; int total = 0;
    char err[1024];
    check(scg_count_combo_barcodes_regions(path.c_str(), constant.c_str(), strand, pools.rows.data(), pools.sizes.data(), (int32_t)pools.rows.size(),
                                           mismatches, use_first, nthreads, &found.idx, &found.freq, &found.k, &total, err, sizeof(err)), err);
    return Rcpp::List::create(combination_indices(found.idx, found.k, (int)pools.rows.size()), found.counts(), Rcpp::IntegerVector::create(total));
}

//[[Rcpp::export(rng=false)]]
Rcpp::List count_combo_barcodes_regions_files(Rcpp::CharacterVector paths, std::string constant, int strand, Rcpp::List pool,
                                              int mismatches, bool use_first, int nthreads) {
    PoolRows pools(pool);
    auto f = borrow(paths);
    PerFileCombinations found(f.size());
    Rcpp::IntegerVector totals(paths.size());
    char err[1024];
    check(scg_count_combo_barcodes_regions_files(f.data(), (int32_t)f.size(), constant.c_str(), strand, pools.rows.data(), pools.sizes.data(),
                                                 (int32_t)pools.rows.size(), mismatches, use_first, nthreads,
                                                 found.idx.data(), found.freq.data(), found.k.data(), totals.begin(), err, sizeof(err)), err);
    Rcpp::List out(paths.size());                        // one count_combo_barcodes_regions() result per file
    for (R_xlen_t i = 0; i < paths.size(); ++i) {
        out[i] = Rcpp::List::create(combination_indices(found.idx[i], found.k[i], (int)pools.rows.size()), found.counts(i),
                                    Rcpp::IntegerVector::create(totals[i]));
    }
    return out;
}
