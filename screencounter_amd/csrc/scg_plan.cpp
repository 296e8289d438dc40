// scg_plan.cpp -- plans: host compilation of the templates and libraries (every argument check of the reference's
// constructors lives here, each once), the kernel arguments built from a plan (one builder per struct), the combination
// streams of the sparse mode, and the launch of one batch.
//
// Host-side counterpart of the handler construction in the reference's Rcpp glue (src/count_single_barcodes.cpp,
// src/count_combo_barcodes_single.cpp, src/count_dual_barcodes.cpp, src/count_dual_barcodes_single_end.cpp).
#include "scg_internal.hpp"

namespace scgapi {
using scg::key_class;

// Big keys have the byte-wise general kernels only, whatever scg::staged_takes says of the batch.
bool general_only(const scg_plan* P) {
    if (P->kind == scg_plan::COMBO_REGIONS) return P->rtab[0].view.wide == 2;      // (all pools share one key class)
    return P->tab[0].view.wide == 2 || (P->kind == scg_plan::DUAL_SE_DIAG && P->tab_combined.view.wide == 2);
}

// 256 MB of int32 cells: beyond that, combinations are sorted and run-length encoded.  $SCG_DENSE_CELLS moves the limit (the
// tests run every combination case both ways).
int64_t dense_cells() { return scg::env().dense_cells; }

ScgReads make_reads(const char* d_seqs, const uint32_t* d_offsets, int32_t fixed_len, int32_t max_len) {
    ScgReads r;
    r.seqs = reinterpret_cast<const uint8_t*>(d_seqs);
    r.offsets = d_offsets;
    r.fixed_len = d_offsets ? 0 : fixed_len;
    r.max_len = d_offsets ? max_len : fixed_len;
#ifdef SCG_ABLATE
    // measurement builds only (make EXTRA=-DSCG_ABLATE OUT=...): the product library has no such switch
    r.ablate = scg::env().ablate;
#else
    r.ablate = 0;
#endif
    return r;
}

void check_reads_args(const char* d_seqs, const uint32_t* d_offsets, int32_t fixed_len, int64_t n) {
    if (n < 0) throw Error(SCG_ERR_INVALID, "negative read count");
    if (n > 0 && !d_seqs && !(d_offsets == nullptr && fixed_len == 0)) throw Error(SCG_ERR_INVALID, "null read buffer");
    if (!d_offsets && fixed_len < 0) throw Error(SCG_ERR_INVALID, "negative fixed read length");
}

// ---- host compilation of the plan kinds (all reference argument checks live here) ----

// SimpleSingleMatch.hpp:75-83: one variable region, as long as the pool's sequences.
void check_single_match(const scg::HostTemplate& ht, int plen) {
    if (ht.t.nreg != 1) throw Error(SCG_ERR_INVALID, "expected one variable region in the constant template");
    if (ht.t.flen[0] != plen) {
        throw Error(SCG_ERR_INVALID, "length of barcode_pool sequences (" + std::to_string(plen) +
                    ") should be the same as the barcode_pool region (" + std::to_string(ht.t.flen[0]) + ")");
    }
}

// CombinatorialBarcodesSingleEnd.hpp:86-93, DualBarcodesSingleEnd.hpp:80-87: variable region r against its pool's sequences.
void check_region_length(const ScgTemplate& t, int r, int plen) {
    if (t.flen[r] != plen) {
        throw Error(SCG_ERR_INVALID, "length of variable region " + std::to_string(r + 1) + " (" + std::to_string(t.flen[r]) +
                    ") should be the same as its sequences (" + std::to_string(plen) + ")");
    }
}

// The uid indexes of two pools whose sequences meet as pairs (both mates, or both regions of include.invalid=TRUE), into
// P->htab[0..1], both in the wider key class of the two.
struct UidIndexes {
    std::vector<std::vector<int32_t> > exp[2];   // barcode -> the uids of its sequences
    std::vector<uint64_t> keys[2];               // class 0: uid -> key, for the pair table
    size_t n_uid[2] = {0, 0};

    UidIndexes(scg_plan* P, const char* const* pool0, int32_t n0, int len0, int mm0, const char* const* pool1, int32_t n1, int len1, int mm1) {
        const int cls = std::max(key_class(len0), key_class(len1));
        P->htab[0] = scg::build_uid_index(pool0, n0, len0, mm0, cls, exp[0], keys[0]);
        P->htab[1] = scg::build_uid_index(pool1, n1, len1, mm1, cls, exp[1], keys[1]);
        for (int side = 0; side < 2; ++side) n_uid[side] = static_cast<size_t>(P->htab[side].n_entries);
    }
    // uid -> index of the first barcode that contains the sequence
    std::vector<int32_t> first(int side) const {
        std::vector<int32_t> f(n_uid[side], -1);
        for (size_t i = 0; i < exp[side].size(); ++i) {
            for (int32_t u : exp[side][i]) if (f[u] < 0) f[u] = static_cast<int32_t>(i);
        }
        return f;
    }
    // The counters of a diagnostics plan: [n_pool valid][2][n_uid0 x n_uid1], the grid only below the dense limit.
    void diagnostics_grid(scg_plan* P, int32_t n_pool) const {
        P->first1 = first(0);
        P->first2 = first(1);
        const int64_t cells = static_cast<int64_t>(n_uid[0]) * static_cast<int64_t>(n_uid[1]);
        P->sparse = cells > dense_cells();
        P->n_counters = static_cast<int64_t>(n_pool) + 2 + (P->sparse ? 0 : cells);
    }
};

std::unique_ptr<scg_plan> compile_single(const char* constant, int strand, const char* const* pool, int32_t n_pool,
                                         int mismatches, int use_first) {
    if (!constant || (n_pool > 0 && !pool) || n_pool < 0) throw Error(SCG_ERR_INVALID, "null argument");
    std::unique_ptr<scg_plan> P(new scg_plan);
    P->kind = scg_plan::SINGLE;
    int plen = scg::pool_length(pool, n_pool);                 // src/utils.cpp:15-17
    P->ht1 = scg::parse_template(constant, strand);            // src/count_single_barcodes.cpp:37-47, ScanTemplate.hpp:53-95
    check_single_match(P->ht1, plen);
    if (mismatches < 0) throw Error(SCG_ERR_INVALID, "negative number of mismatches");
    // BarcodeSearch.hpp:23-60; barcodes of 33..64 bases take the wide (2 x 64-bit plane) index and kernels, longer ones the big
    P->htab[0] = scg::build_index(pool, n_pool, plen, mismatches, key_class(plen));
    P->scan1 = scg::build_scan(P->ht1.t, mismatches);
    P->n_pool[0] = n_pool;
    P->n_counters = n_pool;
    P->max_mm1 = mismatches;
    P->use_first = use_first != 0;
    P->simple_match = true;
    return P;
}

// kaori::SingleBarcodePairedEnd (handlers/SingleBarcodePairedEnd.hpp:41-58): the template, pool and checks of the
// single-end handler; the pairs go through launch_batch_paired.
std::unique_ptr<scg_plan> compile_single_paired(const char* constant, int strand, const char* const* pool, int32_t n_pool,
                                                int mismatches, int use_first) {
    std::unique_ptr<scg_plan> P = compile_single(constant, strand, pool, n_pool, mismatches, use_first);
    P->kind = scg_plan::SINGLE_PAIRED;
    return P;
}

// countDualBarcodesSingleEnd (kaori::DualBarcodesSingleEnd, handlers/DualBarcodesSingleEnd.hpp:66-123): one read
// holds every variable region; pools[r][c] over r spells valid combination c, and the concatenation of a window's
// regions is matched against the concatenated library with one shared mismatch budget.  Same kernels as the single
// barcode with a wide key assembled from several regions.
std::unique_ptr<scg_plan> compile_dual_single_end(const char* constant, int strand, const char* const* const* pools, const int32_t* n_pools,
                                                  int32_t n_regions, int mismatches, int use_first) {
    if (!constant || n_regions < 0 || (n_regions > 0 && (!pools || !n_pools))) throw Error(SCG_ERR_INVALID, "null argument");
    std::unique_ptr<scg_plan> P(new scg_plan);
    P->kind = scg_plan::SINGLE;
    std::vector<int> plen(n_regions);
    for (int r = 0; r < n_regions; ++r) {
        if (n_pools[r] < 0 || (n_pools[r] > 0 && !pools[r])) throw Error(SCG_ERR_INVALID, "null argument");
        plen[r] = scg::pool_length(pools[r], n_pools[r]);         // src/utils.cpp:15-17 (format_pointers per pool)
    }
    P->ht1 = scg::parse_template(constant, strand);
    const ScgTemplate& t = P->ht1.t;
    if (t.nreg != n_regions) throw Error(SCG_ERR_INVALID, "length of 'barcode_pools' should equal the number of variable regions");   // :76-78
    if (n_regions < 1 || n_regions > SCG_MAX_REGIONS) {
        throw Error(SCG_ERR_UNSUPPORTED, "this engine counts dual barcodes in single-end reads with 1 to " + std::to_string(SCG_MAX_REGIONS) +
                    " variable regions (got " + std::to_string(n_regions) + ")");
    }
    int total = 0;
    for (int r = 0; r < n_regions; ++r) {                         // :80-87
        check_region_length(t, r, plen[r]);
        total += plen[r];
    }
    const int32_t n_choices = n_pools[0];
    for (int r = 1; r < n_regions; ++r) {                         // :89-97
        if (n_pools[r] != n_choices) throw Error(SCG_ERR_INVALID, "all entries of 'barcode_pools' should have the same length");
    }
    if (mismatches < 0) throw Error(SCG_ERR_INVALID, "negative number of mismatches");
    std::vector<std::string> combined(n_choices);                // :100-109
    std::vector<const char*> ptrs(n_choices);
    for (int32_t c = 0; c < n_choices; ++c) {
        for (int r = 0; r < n_regions; ++r) combined[c].append(pools[r][c], plen[r]);
        ptrs[c] = combined[c].c_str();
    }
    P->htab[0] = scg::build_index(ptrs.data(), n_choices, total, mismatches, std::max(1, key_class(total)));     // duplicates => error (:111-113)
    P->scan1 = scg::build_scan(t, mismatches);
    P->n_pool[0] = n_choices;
    P->n_counters = n_choices;
    P->max_mm1 = mismatches;
    P->use_first = use_first != 0;
    return P;
}

std::unique_ptr<scg_plan> compile_combo(const char* constant, int strand,
                                        const char* const* pool0, int32_t n0, const char* const* pool1, int32_t n1,
                                        int mismatches, int use_first) {
    if (!constant || (n0 > 0 && !pool0) || (n1 > 0 && !pool1) || n0 < 0 || n1 < 0) throw Error(SCG_ERR_INVALID, "null argument");
    std::unique_ptr<scg_plan> P(new scg_plan);
    P->kind = scg_plan::COMBO;
    int len0 = scg::pool_length(pool0, n0);
    int len1 = scg::pool_length(pool1, n1);
    P->ht1 = scg::parse_template(constant, strand);
    if (P->ht1.t.nreg != 2) {                                  // CombinatorialBarcodesSingleEnd.hpp:79-81
        throw Error(SCG_ERR_INVALID, "expected 2 variable regions in the constant template");
    }
    check_region_length(P->ht1.t, 0, len0);                    // :86-93
    check_region_length(P->ht1.t, 1, len1);
    if (mismatches < 0) throw Error(SCG_ERR_INVALID, "negative number of mismatches");
    // pools of 33..64 bases take the wide (2 x 64-bit plane) index and kernels, longer ones the big one; both pools then, one
    // key width per kernel
    const int cls = std::max(key_class(len0), key_class(len1));
    P->htab[0] = scg::build_index(pool0, n0, len0, mismatches, cls);
    P->htab[1] = scg::build_index(pool1, n1, len1, mismatches, cls);
    P->scan1 = scg::build_scan(P->ht1.t, mismatches);
    P->n_pool[0] = n0; P->n_pool[1] = n1;
    int64_t cells = static_cast<int64_t>(n0) * static_cast<int64_t>(n1);
    P->sparse = cells > dense_cells();                           // beyond the dense limit: sort + run-length encode, like the reference
    P->n_counters = P->sparse ? 0 : cells;
    P->max_mm1 = mismatches;
    P->use_first = use_first != 0;
    return P;
}

// Combinations over n_regions variable regions: kaori::CombinatorialBarcodesSingleEnd<max_size, n_regions>, whose
// constructor, find_match, tie rule and sort are written for any number of regions (the reference's R glue instantiates
// two: src/count_combo_barcodes_single.cpp:44-46).  The constructor's checks in its order
// (CombinatorialBarcodesSingleEnd.hpp:79-93); what this engine cannot represent is SCG_ERR_UNSUPPORTED.
std::unique_ptr<scg_plan> compile_combo_regions(const char* constant, int strand, const char* const* const* pools, const int32_t* n_pools,
                                                int32_t n_regions, int mismatches, int use_first) {
    if (!constant || (n_regions > 0 && (!pools || !n_pools))) throw Error(SCG_ERR_INVALID, "null argument");
    if (n_regions < 1 || n_regions > SCG_MAX_REGIONS) {           // (the template argument: nothing to construct outside it)
        throw Error(SCG_ERR_UNSUPPORTED, "this engine counts combinations of 1 to " + std::to_string(SCG_MAX_REGIONS) + " variable regions (got " +
                    std::to_string(n_regions) + ")");
    }
    std::unique_ptr<scg_plan> P(new scg_plan);
    P->kind = scg_plan::COMBO_REGIONS;
    std::vector<int> plen(n_regions);
    for (int r = 0; r < n_regions; ++r) {
        if (n_pools[r] < 0 || (n_pools[r] > 0 && !pools[r])) throw Error(SCG_ERR_INVALID, "null argument");
        plen[r] = scg::pool_length(pools[r], n_pools[r]);         // src/utils.cpp:15-17 (format_pointers per pool)
    }
    P->ht1 = scg::parse_template(constant, strand);
    const ScgTemplate& t = P->ht1.t;
    if (t.nreg != n_regions) {                                    // :79-81
        throw Error(SCG_ERR_INVALID, "expected " + std::to_string(n_regions) + " variable regions in the constant template");
    }
    for (int r = 0; r < n_regions; ++r) check_region_length(t, r, plen[r]);      // :86-93
    if (mismatches < 0) throw Error(SCG_ERR_INVALID, "negative number of mismatches");
    // a combination is one 64-bit key, ~0 being "none" in a key stream: the pools' sizes must multiply to less than 2^63
    uint64_t cells = 1;
    for (int r = 0; r < n_regions; ++r) {
        uint64_t next = 0;
        if (__builtin_mul_overflow(cells, static_cast<uint64_t>(n_pools[r]), &next) || next >= (uint64_t(1) << 63)) {
            throw Error(SCG_ERR_UNSUPPORTED, "the pools of the " + std::to_string(n_regions) + " variable regions span 2^63 combinations or more: beyond the 64-bit keys of this engine");
        }
        cells = next;
    }
    // one key width per kernel: every pool in the widest key class among them
    int cls = 0;
    for (int r = 0; r < n_regions; ++r) cls = std::max(cls, key_class(plen[r]));
    P->n_regions = n_regions;
    P->hpools.resize(static_cast<size_t>(n_regions));
    P->pool_sizes.assign(n_pools, n_pools + n_regions);
    for (int r = 0; r < n_regions; ++r) P->hpools[static_cast<size_t>(r)] = scg::build_index(pools[r], n_pools[r], plen[r], mismatches, cls);
    uint64_t stride = 1;
    for (int r = n_regions - 1; r >= 0; --r) {                    // (an empty pool: nothing is ever found, the strides do not matter)
        P->stride[r] = stride;
        stride *= static_cast<uint64_t>(std::max<int32_t>(n_pools[r], 1));
    }
    P->scan1 = scg::build_scan(t, mismatches);
    P->n_pool[0] = P->n_pool[1] = 0;
    P->sparse = cells > static_cast<uint64_t>(std::max<int64_t>(dense_cells(), 0));      // as compile_combo: $SCG_DENSE_CELLS switches it per call
    P->n_counters = P->sparse ? 0 : static_cast<int64_t>(cells);
    P->max_mm1 = mismatches;
    P->use_first = use_first != 0;
    return P;
}

std::unique_ptr<scg_plan> compile_dual(const char* constant1, int reverse1, int mismatches1, const char* const* pool1,
                                       const char* constant2, int reverse2, int mismatches2, const char* const* pool2,
                                       int32_t n_pool, int randomized, int use_first, int diagnostics) {
    if (!constant1 || !constant2 || (n_pool > 0 && (!pool1 || !pool2)) || n_pool < 0) throw Error(SCG_ERR_INVALID, "null argument");
    std::unique_ptr<scg_plan> P(new scg_plan);
    P->kind = scg_plan::DUAL;
    int len1 = scg::pool_length(pool1, n_pool);                // src/count_dual_barcodes.cpp:93-97
    int len2 = scg::pool_length(pool2, n_pool);
    P->ht1 = scg::parse_template(constant1, reverse1 ? 1 : 0); // DualBarcodesPairedEnd.hpp:99-100
    P->ht2 = scg::parse_template(constant2, reverse2 ? 1 : 0);
    if (P->ht1.t.nreg != 1) throw Error(SCG_ERR_INVALID, "expected one variable region in the first constant template");    // :115-117
    if (P->ht1.t.flen[0] != len1) {                            // :119-122
        throw Error(SCG_ERR_INVALID, "length of variable sequences (" + std::to_string(len1) + ") should be the same as the variable region (" +
                    std::to_string(P->ht1.t.flen[0]) + ")");
    }
    if (P->ht2.t.nreg != 1) throw Error(SCG_ERR_INVALID, "expected one variable region in the second constant template");   // :128-130
    if (P->ht2.t.flen[0] != len2) {
        throw Error(SCG_ERR_INVALID, "length of variable sequences (" + std::to_string(len2) + ") should be the same as the variable region (" +
                    std::to_string(P->ht2.t.flen[0]) + ")");
    }
    if (mismatches1 < 0 || mismatches2 < 0) throw Error(SCG_ERR_INVALID, "negative number of mismatches");
    const UidIndexes uid(P.get(), pool1, n_pool, len1, mismatches1, pool2, n_pool, len2, mismatches2);
    P->scan1 = scg::build_scan(P->ht1.t, mismatches1);
    P->scan2 = scg::build_scan(P->ht2.t, mismatches2);
    P->hpairs = scg::build_pair_table(uid.exp[0], uid.keys[0], uid.exp[1], uid.keys[1]);   // :138-178 (duplicate pairs => error)
    P->n_pool[0] = P->n_pool[1] = n_pool;
    P->n_counters = n_pool;
    if (diagnostics) {
        uid.diagnostics_grid(P.get(), n_pool);
        P->diagnostics = 1;
    }
    P->max_mm1 = mismatches1; P->max_mm2 = mismatches2;
    P->rev1 = reverse1 != 0; P->rev2 = reverse2 != 0;
    P->randomized = randomized != 0;
    P->use_first = use_first != 0;
    return P;
}

// countDualBarcodesSingleEnd(include.invalid=TRUE): DualBarcodesSingleEndWithDiagnostics<N, 2>
// (handlers/DualBarcodesSingleEndWithDiagnostics.hpp:35-60) = the valid-combination handler plus
// CombinatorialBarcodesSingleEnd<N, 2> over the same pools with DuplicateAction::FIRST.
std::unique_ptr<scg_plan> compile_dual_single_end_diag(const char* constant, int strand, const char* const* const* pools, const int32_t* n_pools,
                                                       int32_t n_regions, int mismatches, int use_first) {
    auto P = compile_dual_single_end(constant, strand, pools, n_pools, n_regions, mismatches, use_first);   // its constructor runs first
    const ScgTemplate& t = P->ht1.t;
    if (t.nreg != 2) throw Error(SCG_ERR_INVALID, "expected 2 variable regions in the constant template");   // CombinatorialBarcodesSingleEnd.hpp:84-86
    P->kind = scg_plan::DUAL_SE_DIAG;
    P->htab_combined = std::move(P->htab[0]);
    const UidIndexes uid(P.get(), pools[0], n_pools[0], t.flen[0], mismatches, pools[1], n_pools[1], t.flen[1], mismatches);
    uid.diagnostics_grid(P.get(), P->n_pool[0]);
    P->n_pool[1] = P->n_pool[0];
    return P;
}

// countPairedComboBarcodes: two independent SimpleSingleMatch matchers (CombinatorialBarcodesPairedEnd.hpp:85-118).
std::unique_ptr<scg_plan> compile_paired_combo(const char* constant1, int reverse1, int mismatches1, const char* const* pool1, int32_t n1,
                                               const char* constant2, int reverse2, int mismatches2, const char* const* pool2, int32_t n2,
                                               int randomized, int use_first) {
    if (!constant1 || !constant2 || (n1 > 0 && !pool1) || (n2 > 0 && !pool2) || n1 < 0 || n2 < 0) throw Error(SCG_ERR_INVALID, "null argument");
    std::unique_ptr<scg_plan> P(new scg_plan);
    P->kind = scg_plan::DUAL;
    int len1 = scg::pool_length(pool1, n1);                    // src/utils.cpp:15-17
    int len2 = scg::pool_length(pool2, n2);
    P->ht1 = scg::parse_template(constant1, reverse1 ? 1 : 0);
    P->ht2 = scg::parse_template(constant2, reverse2 ? 1 : 0);
    check_single_match(P->ht1, len1);
    check_single_match(P->ht2, len2);
    if (mismatches1 < 0 || mismatches2 < 0) throw Error(SCG_ERR_INVALID, "negative number of mismatches");
    const int cls = std::max(key_class(len1), key_class(len2));
    P->htab[0] = scg::build_index(pool1, n1, len1, mismatches1, cls);     // values = pool indices; duplicates => error
    P->htab[1] = scg::build_index(pool2, n2, len2, mismatches2, cls);
    P->scan1 = scg::build_scan(P->ht1.t, mismatches1);
    P->scan2 = scg::build_scan(P->ht2.t, mismatches2);
    int64_t cells = static_cast<int64_t>(n1) * static_cast<int64_t>(n2);
    P->sparse = cells > dense_cells();
    P->first1.resize(n1);
    P->first2.resize(n2);
    for (int32_t i = 0; i < n1; ++i) P->first1[i] = i;
    for (int32_t i = 0; i < n2; ++i) P->first2[i] = i;
    P->n_pool[0] = P->n_pool[1] = 0;                           // no list of valid pairs
    P->diagnostics = 2;
    P->n_counters = 2 + (P->sparse ? 0 : cells);               // [barcode1-only][barcode2-only][n1 x n2]
    P->max_mm1 = mismatches1; P->max_mm2 = mismatches2;
    P->rev1 = reverse1 != 0; P->rev2 = reverse2 != 0;
    P->randomized = randomized != 0;
    P->use_first = use_first != 0;
    return P;
}

// ---- kernel arguments: each struct is built in one place, from a value-initialised one ----

// Counters at `base` and nothing else: no replicas, no index or combination stream, no hot slots.
ScgCounters plain_counters(int32_t* base) {
    ScgCounters c = ScgCounters();
    c.base = base;
    return c;
}

ScgCounters plan_counters(const scg_plan* P) {
    ScgCounters c = plain_counters(P->counters);
    if (P->replica_shift > 0) {
        c.base = P->replicas.as<int32_t>();
        c.replica_shift = static_cast<uint32_t>(P->replica_shift);
        c.replica_mask = (1u << P->replica_shift) - 1u;
    }
    c.hot = P->hot.p ? P->hot.as<int32_t>() : nullptr;
    return c;
}

// The template of the plan searched in `index`; the random-barcode paths, which have no library, pass ScgIndex().
ScgSingleParams single_params(const scg_plan* P, const ScgIndex& index) {
    ScgSingleParams sp = ScgSingleParams();
    sp.scan = P->scan1;
    sp.tmpl = P->d_tmpl1.as<ScgTemplate>();
    sp.index = index;
    sp.max_mm = P->max_mm1; sp.use_first = P->use_first;
    sp.fwd = P->ht1.fwd; sp.rev = P->ht1.rev;
    return sp;
}

// The combination search over the plan's two pools; the second pass of include.invalid=TRUE overrides n_pool,
// only_if_negative and keep_first.
ScgComboParams combo_params(const scg_plan* P) {
    ScgComboParams cp = ScgComboParams();
    cp.scan = P->scan1;
    cp.tmpl = P->d_tmpl1.as<ScgTemplate>();
    cp.index[0] = P->tab[0].view; cp.index[1] = P->tab[1].view;
    cp.n_pool[0] = P->n_pool[0]; cp.n_pool[1] = P->n_pool[1];
    cp.max_mm = P->max_mm1; cp.use_first = P->use_first;
    cp.fwd = P->ht1.fwd; cp.rev = P->ht1.rev;
    return cp;
}

// The combination search over the plan's n_regions pools (COMBO_REGIONS).
ScgComboRegionsParams combo_regions_params(const scg_plan* P) {
    ScgComboRegionsParams cp = ScgComboRegionsParams();
    cp.scan = P->scan1;
    cp.tmpl = P->d_tmpl1.as<ScgTemplate>();
    cp.nreg = P->n_regions;
    for (int r = 0; r < P->n_regions; ++r) { cp.index[r] = P->rtab[r].view; cp.stride[r] = P->stride[r]; }
    cp.max_mm = P->max_mm1; cp.use_first = P->use_first;
    cp.fwd = P->ht1.fwd; cp.rev = P->ht1.rev;
    return cp;
}

// The index stream of the batch of n reads about to run on `stream`: the barcode index per read, for the tally
// (ScgCounters::unit_index).  One buffer per stream: batches on different streams may be in flight together.
int32_t* index_stream(scg_plan* P, hipStream_t stream, int64_t n) {
    DevBuf& buf = P->unit_index[stream];
    buf.ensure(static_cast<size_t>(n) * sizeof(int32_t));
    return buf.as<int32_t>();
}

// ---- sparse mode: combination streams ----

// The runs of the batch last counted on `stream` -> the plan's map.
void retire_pairs(scg_plan* P, hipStream_t stream, scg_plan::PairStream& ps) {
    if (!ps.pending) return;
    uint32_t runs = 0;
    HIP_CHECK(hipEventSynchronize(ps.done));
    HIP_CHECK(hipMemcpy(&runs, ps.runs.p, sizeof(runs), hipMemcpyDeviceToHost));
    std::vector<uint64_t> keys(runs);
    std::vector<uint32_t> counts(runs);
    if (runs) {
        HIP_CHECK(hipMemcpy(keys.data(), ps.unique.p, sizeof(uint64_t) * runs, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(counts.data(), ps.counts.p, sizeof(uint32_t) * runs, hipMemcpyDeviceToHost));
    }
    for (uint32_t i = 0; i < runs; ++i) {
        if (keys[i] != ~uint64_t(0)) P->sparse_counts[keys[i]] += counts[i];
    }
    ps.pending = 0;
}

// A stream of n keys for the next batch on `stream`, every slot "none" (kernels that skip a read leave it so).
uint64_t* begin_pairs(scg_plan* P, hipStream_t stream, int64_t n) {
    scg_plan::PairStream& ps = P->pair_stream[stream];
    retire_pairs(P, stream, ps);
    const size_t m = static_cast<size_t>(std::max<int64_t>(n, 1));
    ps.keys.ensure(m * sizeof(uint64_t));
    ps.sorted.ensure(m * sizeof(uint64_t));
    ps.unique.ensure(m * sizeof(uint64_t));
    ps.counts.ensure(m * sizeof(uint32_t));
    if (!ps.runs.p) ps.runs.alloc(sizeof(uint32_t));
    ps.scratch.ensure(scg::sort_rle_scratch_bytes(m));
    HIP_CHECK(hipMemsetAsync(ps.keys.p, 0xFF, m * sizeof(uint64_t), stream));
    return ps.keys.as<uint64_t>();
}

// Behind the counting kernels of the batch: sort + run-length encode, still asynchronous.
void finish_pairs(scg_plan* P, hipStream_t stream, int64_t n) {
    scg_plan::PairStream& ps = P->pair_stream[stream];
    HIP_CHECK(scg::launch_sort_rle(ps.keys.as<uint64_t>(), ps.sorted.as<uint64_t>(), static_cast<size_t>(n), ps.unique.as<uint64_t>(),
                                   ps.counts.as<uint32_t>(), ps.runs.as<uint32_t>(), ps.scratch.p, ps.scratch.bytes, stream));
    if (!ps.done) HIP_CHECK(hipEventCreateWithFlags(&ps.done, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(ps.done, stream));
    ps.pending = n;
}

void retire_all_pairs(scg_plan* P) {
    DeviceGuard g(P->device);
    for (auto& kv : P->pair_stream) retire_pairs(P, kv.first, kv.second);
}

// A reset of the plan: the batches in flight are let finish and their runs dropped.
void drop_pending_pairs(scg_plan* P) {
    for (auto& kv : P->pair_stream) {
        if (kv.second.pending) { HIP_CHECK(hipEventSynchronize(kv.second.done)); kv.second.pending = 0; }
    }
}

// Tally mode pays off when the library is large enough that block-level aggregation finds no repeats
// (small libraries are served by the replicas) and small enough for a few LDS passes, on batches
// large enough to amortise the second kernel.  SCG_TALLY=0/1 overrides (measurement aid).
bool use_tally(const scg_plan* P, int64_t n) {
    if (P->diagnostics) return false;      // the diagnostics kernels count several things per pair
    if (scg::env().tally >= 0) return scg::env().tally != 0;
    return P->n_counters >= 4096 && P->n_counters <= 4 * 80 * 1024 && n >= (int64_t(1) << 20);
}

void fold_replicas(scg_plan* P, hipStream_t stream) {
    if (P->replica_shift > 0) {
        HIP_CHECK(scg::launch_fold(P->replicas.as<int32_t>(), P->replica_shift, P->n_counters, P->counters, stream));
    }
}

// countDualBarcodesSingleEnd(include.invalid=TRUE) in two passes over the batch: the valid-combination search
// writes its per-read result as an index stream (tallied into counters[0 .. n_pool)), then the combinatorial
// search runs on the reads that found nothing (ScgComboParams::only_if_negative) with DuplicateAction::FIRST
// and counts (uid1, uid2) cells behind the two unused diagnostics slots: [n_pool][2][n_uid1 x n_uid2].
void launch_batch_se_diag(scg_plan* P, const ScgReads& R, int64_t n, hipStream_t stream) {
    scg_plan::Timer timer(P, stream);
    ScgCounters c1 = plain_counters(P->counters);
    c1.unit_index = index_stream(P, stream, n);
    HIP_CHECK(scg::launch_single(single_params(P, P->tab_combined.view), P->ht1.t.len, R, n, c1, P->error_flag.as<int32_t>(), stream));
    HIP_CHECK(scg::launch_tally(c1.unit_index, n, P->counters, P->n_pool[0], stream));
    ScgComboParams cp = combo_params(P);
    cp.n_pool[0] = static_cast<int32_t>(P->first1.size()); cp.n_pool[1] = static_cast<int32_t>(P->first2.size());
    cp.only_if_negative = c1.unit_index; cp.keep_first = 1;
    ScgCounters c2 = plain_counters(P->counters + P->n_pool[0] + 2);
    if (P->sparse) c2.unit_pair = begin_pairs(P, stream, n);
    HIP_CHECK(scg::launch_combo(cp, P->ht1.t.len, R, n, c2, P->error_flag.as<int32_t>(), stream));
    timer.stop();
    if (P->sparse) finish_pairs(P, stream, n);
    P->total += n;
}

// ---- countRandomBarcodes plans: the tally in HBM (scg_random.hip) ----

// kaori::RandomBarcodeSingleEnd (handlers/RandomBarcodeSingleEnd.hpp:86-181): the template and every argument check of
// countRandomBarcodes, for the file entry (count_random_file, which tallies on the host) and for the plans below.  A plan
// of the SINGLE kind without a library or counters: the template is located by launch_random, which reads no index.
std::unique_ptr<scg_plan> compile_random_template(const char* constant, int strand, int mismatches, int use_first) {
    if (!constant) throw Error(SCG_ERR_INVALID, "null argument");
    std::unique_ptr<scg_plan> P(new scg_plan);
    P->kind = scg_plan::SINGLE;
    P->ht1 = scg::parse_template(constant, strand);
    const ScgTemplate& t = P->ht1.t;
    if (t.nreg < 1) throw Error(SCG_ERR_INVALID, "expected one variable region in the constant template");
    if (t.nreg > SCG_MAX_REGIONS) throw Error(SCG_ERR_UNSUPPORTED, "this engine handles templates with at most " + std::to_string(SCG_MAX_REGIONS) + " variable regions");
    if (mismatches < 0) throw Error(SCG_ERR_INVALID, "negative number of mismatches");
    P->scan1 = scg::build_scan(t, mismatches);
    P->max_mm1 = mismatches;
    P->use_first = use_first != 0;
    P->n_counters = 0;
    return P;
}

// The same with the tally in HBM.  The key is the FIRST forward region on both strands, like the reference.
std::unique_ptr<scg_plan> compile_random(const char* constant, int strand, int mismatches, int use_first) {
    std::unique_ptr<scg_plan> P = compile_random_template(constant, strand, mismatches, use_first);
    P->kind = scg_plan::RANDOM;
    P->rnd.reset(new RandomTally);
    P->rnd->vstart = P->ht1.t.fstart[0];
    P->rnd->vlen = P->ht1.t.flen[0];
    // Test hook, used here only: hashed tags keep this many hash bits (default and maximum 61), so that tests can make
    // tags collide and exhaust the rounds.  Results never depend on it unless the rounds run out, which read-out reports.
    P->rnd->tag_bits = scg::env().random_tag_bits;
    return P;
}

namespace {

const uint64_t RANDOM_INITIAL_SLOTS = uint64_t(1) << 16;
const uint64_t RANDOM_MAX_SLOTS = uint64_t(1) << 30;     // slot indices travel in 30 bits (scg_random.hip)

void swap_buf(DevBuf& a, DevBuf& b) { std::swap(a.p, b.p); std::swap(a.bytes, b.bytes); }

// (ids: files mode only)
void alloc_table(DevBuf& tags, DevBuf& counts, DevBuf& arena, DevBuf* ids, uint64_t cap, int vlen) {
    tags.alloc(cap * sizeof(unsigned long long));
    counts.alloc(cap * sizeof(unsigned long long));
    arena.alloc(cap * static_cast<uint64_t>(vlen));
    if (ids) ids->alloc(cap * sizeof(uint32_t));
}

// Every call on the plan waits for the previous one, on whichever stream that ran.
void random_order(RandomTally& T, hipStream_t stream) {
    if (T.has_last) HIP_CHECK(hipStreamWaitEvent(stream, T.last, 0));
}
void random_done(RandomTally& T, hipStream_t stream) {
    HIP_CHECK(hipEventRecord(T.last, stream));
    T.has_last = true;
}

// Keeps occupancy <= capacity / 2 for the batch of n reads about to be counted on `stream`.  The bound is the last
// occupancy known on the host plus every read counted since; only when it exceeds half the capacity is the exact
// occupancy fetched (one synchronisation), and the table doubles while that plus n still does.
void random_reserve(scg_plan* P, int64_t n, hipStream_t stream) {
    RandomTally& T = *P->rnd;
    if (T.snap_pending && hipEventQuery(T.snap_event) == hipSuccess) {
        T.known_occ = static_cast<int64_t>(*T.snap.as<unsigned long long>());
        T.known_at = T.snap_at;
        T.snap_pending = false;
    }
    auto bound = [&] { return static_cast<uint64_t>(T.known_occ + (P->total - T.known_at) + n); };
    if (bound() * 2 <= T.cap) return;
    HIP_CHECK(hipMemcpyAsync(T.snap.p, T.state.as<unsigned long long>() + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    T.known_occ = static_cast<int64_t>(*T.snap.as<unsigned long long>());
    T.known_at = P->total;
    T.snap_pending = false;
    uint64_t cap = T.cap;
    while (bound() * 2 > cap) {
        if (cap >= RANDOM_MAX_SLOTS) {
            throw Error(SCG_ERR_UNSUPPORTED, "random barcode tally: " + std::to_string(bound()) + " possible keys exceed the table limit of " +
                        std::to_string(RANDOM_MAX_SLOTS / 2) + " (read out, reset and count the rest in another plan)");
        }
        cap *= 2;
    }
    if (cap == T.cap) return;
    DevBuf tags, counts, arena, ids;
    try {
        alloc_table(tags, counts, arena, T.files ? &ids : nullptr, cap, T.vlen);
    } catch (const Error& e) {
        throw Error(SCG_ERR_DEVICE, "random barcode tally: cannot grow the table from " + std::to_string(T.cap) + " to " + std::to_string(cap) +
                    " slots (" + e.what() + "); no key was dropped, the counts so far stay readable");
    }
    HIP_CHECK(hipMemsetAsync(tags.p, 0, tags.bytes, stream));
    HIP_CHECK(hipMemsetAsync(counts.p, 0, counts.bytes, stream));
    const scg::ScgRandomTable from = T.view();
    scg::ScgRandomTable to = from;
    to.tags = tags.as<unsigned long long>(); to.counts = counts.as<unsigned long long>(); to.arena = arena.as<uint8_t>(); to.mask = cap - 1;
    if (T.files) to.ids = ids.as<uint32_t>();
    HIP_CHECK(scg::launch_random_rehash(from, to, stream));
    HIP_CHECK(hipStreamSynchronize(stream));          // before the old table is released
    swap_buf(T.tags, tags); swap_buf(T.counts, counts); swap_buf(T.arena, arena); swap_buf(T.ids, ids);
    T.cap = cap;
}

void launch_batch_random(scg_plan* P, const ScgReads& R, int64_t n, hipStream_t stream) {
    RandomTally& T = *P->rnd;
    if (n >= INT32_MAX) throw Error(SCG_ERR_INVALID, "random-barcode plans take batches of fewer than 2^31 - 1 reads");
    random_order(T, stream);
    if (n > 0) {
        random_reserve(P, n, stream);
        RandomTally::Scratch& s = T.scratch[stream];
        const size_t bytes = static_cast<size_t>(n) * sizeof(int32_t);
        s.hits.ensure(bytes); s.slots.ensure(bytes); s.list_a.ensure(bytes); s.list_b.ensure(bytes);
        s.lens.ensure(SCG_RANDOM_ROUNDS * sizeof(int32_t));
        scg_plan::Timer timer(P, stream);
        // a staged kernel that meets an oversize read flags it and leaves its hit unwritten: -1 there
        HIP_CHECK(hipMemsetAsync(s.hits.p, 0xFF, bytes, stream));
        HIP_CHECK(hipMemsetAsync(s.lens.p, 0, SCG_RANDOM_ROUNDS * sizeof(int32_t), stream));
        HIP_CHECK(scg::launch_random(single_params(P, ScgIndex()), P->ht1.t.len, R, n, s.hits.as<int32_t>(), P->error_flag.as<int32_t>(), stream));
        const scg::ScgRandomTable view = T.view();
        HIP_CHECK(scg::launch_random_insert(view, R, n, s.hits.as<int32_t>(), s.slots.as<int32_t>(), P->total, stream));
        HIP_CHECK(scg::launch_random_verify_rounds(view, R, n, s.hits.as<int32_t>(), s.slots.as<int32_t>(), s.list_a.as<int32_t>(),
                                                   s.list_b.as<int32_t>(), s.lens.as<int32_t>(), stream));
        timer.stop();
        P->total += n;
        if (!T.snap_pending) {
            HIP_CHECK(hipMemcpyAsync(T.snap.p, T.state.as<unsigned long long>() + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipEventRecord(T.snap_event, stream));
            T.snap_pending = true;
            T.snap_at = P->total;
        }
    }
    random_done(T, stream);
}

} // namespace

void random_to_device(scg_plan* P) {
    RandomTally& T = *P->rnd;
    DeviceGuard g(P->device);
    T.cap = RANDOM_INITIAL_SLOTS;
    alloc_table(T.tags, T.counts, T.arena, T.files ? &T.ids : nullptr, T.cap, T.vlen);
    T.state.alloc(4 * sizeof(unsigned long long));
    T.snap.ensure(sizeof(unsigned long long));
    HIP_CHECK(hipEventCreateWithFlags(&T.snap_event, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&T.last, hipEventDisableTiming));
    HIP_CHECK(hipMemset(T.tags.p, 0, T.tags.bytes));
    HIP_CHECK(hipMemset(T.counts.p, 0, T.counts.bytes));
    HIP_CHECK(hipMemset(T.state.p, 0, T.state.bytes));
    HIP_CHECK(hipMemset(T.state.p, 0xFF, sizeof(unsigned long long)));   // no unknown-base error yet
    HIP_CHECK(hipStreamSynchronize(nullptr));         // the fills are only enqueued (see scg_plan::to_device)
}

void random_reset(scg_plan* P, hipStream_t stream) {
    RandomTally& T = *P->rnd;
    random_order(T, stream);
    HIP_CHECK(hipMemsetAsync(T.tags.p, 0, T.tags.bytes, stream));
    HIP_CHECK(hipMemsetAsync(T.counts.p, 0, T.counts.bytes, stream));
    HIP_CHECK(hipMemsetAsync(T.state.p, 0, T.state.bytes, stream));
    HIP_CHECK(hipMemsetAsync(T.state.p, 0xFF, sizeof(unsigned long long), stream));
    HIP_CHECK(hipMemsetAsync(P->error_flag.p, 0, sizeof(int32_t), stream));
    random_done(T, stream);
    T.known_occ = T.known_at = 0;
    T.snap_pending = false;       // (a copy still in flight lands before any later one: the plan's calls are ordered)
}

namespace {

// What a read-out checks before it hands anything out, in this order: the reference's unknown-base error, reads longer
// than their batch's declared maximum, reads whose key collided in every round.
void check_random_state(scg_plan* P, const unsigned long long* st) {
    if (st[0] != ~0ull) {                              // kaori/utils.hpp:117, first offending read in counting order
        throw Error(SCG_ERR_INVALID, std::string("cannot complement unknown base '") + static_cast<char>(st[0] & 0xFF) + "'");
    }
    read_counters(P, nullptr);                         // reads longer than their batch's declared maximum
    if (st[2]) {
        throw Error(SCG_ERR_UNSUPPORTED, "random barcode tally: the keys of " + std::to_string(st[2]) + " reads collided with other keys in all " +
                    std::to_string(SCG_RANDOM_ROUNDS) + " hash rounds; counts are incomplete");
    }
}

// Occupied slots (`occ` of them at most) -> packed keys sorted on the device and decoded there, hashed keys' bytes sorted
// here; the two sorted lists merged byte-wise (all keys have the same length).  Each key comes with its count, and only
// keys that have one; or, with_ids, every key with its id.  Synchronises `stream`.
RandomKeys random_sorted_keys(RandomTally& T, hipStream_t stream, uint64_t occ, bool with_ids) {
    const int vlen = T.vlen;
    const size_t m = static_cast<size_t>(std::max<uint64_t>(occ, 1));
    DevBuf ptags, pcounts, hslots, hcounts, nout;
    ptags.alloc(m * 8); pcounts.alloc(m * 8); hslots.alloc(m * 4); hcounts.alloc(m * 8); nout.alloc(2 * 8);
    HIP_CHECK(hipMemsetAsync(nout.p, 0, 2 * 8, stream));
    HIP_CHECK(scg::launch_random_compact(T.view(), ptags.as<unsigned long long>(), pcounts.as<unsigned long long>(), hslots.as<int32_t>(),
                                         hcounts.as<unsigned long long>(), nout.as<unsigned long long>(), with_ids, stream));
    unsigned long long nn[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(nn, nout.p, sizeof(nn), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    const size_t np = static_cast<size_t>(nn[0]), nh = static_cast<size_t>(nn[1]);
    const size_t stride = static_cast<size_t>(vlen) + 1;
    std::vector<unsigned long long> pc(np), hc(nh);
    std::vector<char> pbytes(np * stride);
    std::vector<uint8_t> hbytes(nh * static_cast<size_t>(vlen));
    if (np) {
        DevBuf stags, scounts, scratch, dec;
        stags.alloc(np * 8); scounts.alloc(np * 8);
        scratch.alloc(scg::random_sort_scratch_bytes(np));
        dec.alloc(np * stride);
        HIP_CHECK(scg::launch_random_sort(ptags.as<unsigned long long>(), stags.as<unsigned long long>(), pcounts.as<unsigned long long>(),
                                          scounts.as<unsigned long long>(), np, 2 * vlen, scratch.p, scratch.bytes, stream));
        HIP_CHECK(scg::launch_random_decode(stags.as<unsigned long long>(), static_cast<int64_t>(np), vlen, dec.as<char>(), stream));
        HIP_CHECK(hipMemcpyAsync(pc.data(), scounts.p, np * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(pbytes.data(), dec.p, np * stride, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    std::vector<size_t> horder(nh);
    if (nh) {
        DevBuf gathered;
        gathered.alloc(hbytes.size());
        HIP_CHECK(scg::launch_random_gather(T.view(), hslots.as<int32_t>(), static_cast<int64_t>(nh), gathered.as<uint8_t>(), stream));
        HIP_CHECK(hipMemcpyAsync(hbytes.data(), gathered.p, hbytes.size(), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(hc.data(), hcounts.p, nh * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        for (size_t i = 0; i < nh; ++i) horder[i] = i;
        const uint8_t* hb = hbytes.data();
        std::sort(horder.begin(), horder.end(), [&](size_t a, size_t b) {
            return std::memcmp(hb + a * vlen, hb + b * vlen, static_cast<size_t>(vlen)) < 0;
        });
    }
    const size_t K = np + nh;
    RandomKeys out;
    out.bytes.reset(static_cast<char*>(std::malloc(K * stride + 1)));
    if (!out.bytes) throw std::bad_alloc();
    out.vals.resize(K);
    char* so = out.bytes.get();
    size_t a = 0, b = 0;
    for (size_t k = 0; k < K; ++k) {
        const bool take_packed = b == nh ||
            (a < np && std::memcmp(pbytes.data() + a * stride, hbytes.data() + horder[b] * vlen, static_cast<size_t>(vlen)) < 0);
        if (take_packed) {
            std::memcpy(so + k * stride, pbytes.data() + a * stride, stride);
            out.vals[k] = pc[a++];
        } else {
            std::memcpy(so + k * stride, hbytes.data() + horder[b] * vlen, static_cast<size_t>(vlen));
            so[k * stride + vlen] = 0;
            out.vals[k] = hc[horder[b++]];
        }
    }
    return out;
}

} // namespace

// Read-out of a plan: the keys with a count, in the file entry's form.  Synchronises `stream`.
void read_random(scg_plan* P, hipStream_t stream, char** sequences_out, int32_t** freq_out, int64_t* k_out, int32_t* length_out) {
    RandomTally& T = *P->rnd;
    DeviceGuard g(P->device);
    random_order(T, stream);
    unsigned long long st[4] = {0, 0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(st, T.state.p, sizeof(st), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    check_random_state(P, st);
    RandomKeys keys = random_sorted_keys(T, stream, st[1], false);
    random_done(T, stream);
    const size_t K = keys.vals.size();
    std::unique_ptr<int32_t, void (*)(void*)> freq(static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (K + 1))), std::free);
    if (!freq) throw std::bad_alloc();
    for (size_t k = 0; k < K; ++k) {
        const unsigned long long c = keys.vals[k];
        if (c > static_cast<unsigned long long>(INT32_MAX)) {
            throw Error(SCG_ERR_INVALID, "frequency of a random barcode (" + std::to_string(c) + ") exceeds the 32-bit range of the count vectors");
        }
        freq.get()[k] = static_cast<int32_t>(c);
    }
    *sequences_out = keys.bytes.release(); *freq_out = freq.release();
    *k_out = static_cast<int64_t>(K); *length_out = T.vlen;
}

// ---- files mode: one table for all the files a device takes (scg_count_random_barcodes_files) ----
// These run between files, when the pipelines of the last one are gone: on the null stream, behind the plan's last call.

// Counts, the error word and the unresolved reads go (the oversize-read flag and the total: reset_plan, the caller);
// tags, keys, ids, occupancy and capacity stay.  A key first seen in a pass that was abandoned keeps its slot with a
// count of zero, which no harvest lists.
void random_soft_reset(scg_plan* P) {
    RandomTally& T = *P->rnd;
    DeviceGuard g(P->device);
    unsigned long long* st = T.state.as<unsigned long long>();
    random_order(T, nullptr);
    HIP_CHECK(hipMemsetAsync(T.counts.p, 0, T.counts.bytes, nullptr));
    HIP_CHECK(hipMemsetAsync(st, 0xFF, sizeof(unsigned long long), nullptr));
    HIP_CHECK(hipMemsetAsync(st + 2, 0, 2 * sizeof(unsigned long long), nullptr));
    HIP_CHECK(hipMemcpyAsync(T.snap.p, st + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, nullptr));
    HIP_CHECK(hipStreamSynchronize(nullptr));
    random_done(T, nullptr);
    T.known_occ = static_cast<int64_t>(*T.snap.as<unsigned long long>());      // the growth bound starts over from the keys kept
    T.known_at = 0;
    T.snap_pending = false;
    if (T.scratch.size() > 8) T.scratch.clear();       // (the host readers bring two new streams per file)
}

void random_harvest(scg_plan* P, std::vector<int32_t>& pairs) {
    RandomTally& T = *P->rnd;
    DeviceGuard g(P->device);
    random_order(T, nullptr);
    unsigned long long st[4] = {0, 0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(st, T.state.p, sizeof(st), hipMemcpyDeviceToHost, nullptr));
    HIP_CHECK(hipStreamSynchronize(nullptr));
    check_random_state(P, st);
    if (st[1] > static_cast<unsigned long long>(INT32_MAX)) throw Error(SCG_ERR_DEVICE, "internal: random barcode tally: occupancy out of range");
    const uint32_t cap = static_cast<uint32_t>(st[1]);
    T.harvest.ensure(static_cast<size_t>(std::max<uint32_t>(cap, 1)) * 2 * sizeof(int32_t));
    T.harvest_n.ensure(2 * sizeof(unsigned int));
    HIP_CHECK(hipMemsetAsync(T.harvest_n.p, 0, 2 * sizeof(unsigned int), nullptr));
    HIP_CHECK(scg::launch_random_harvest(T.view(), T.harvest.as<int32_t>(), cap, T.harvest_n.as<unsigned int>(), nullptr));
    unsigned int n[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(n, T.harvest_n.p, sizeof(n), hipMemcpyDeviceToHost, nullptr));
    HIP_CHECK(hipStreamSynchronize(nullptr));
    random_done(T, nullptr);
    if (n[1] & 2u) throw Error(SCG_ERR_DEVICE, "internal: random barcode tally: more counted slots than occupied ones");
    if (n[1]) throw Error(SCG_ERR_INVALID, "frequency of a random barcode exceeds the 32-bit range of the count vectors");
    pairs.resize(static_cast<size_t>(n[0]) * 2);
    if (n[0]) HIP_CHECK(hipMemcpy(pairs.data(), T.harvest.p, pairs.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
}

RandomKeys random_keys_with_ids(scg_plan* P) {
    RandomTally& T = *P->rnd;
    DeviceGuard g(P->device);
    random_order(T, nullptr);
    unsigned long long occ = 0;
    HIP_CHECK(hipMemcpyAsync(&occ, T.state.as<unsigned long long>() + 1, sizeof(occ), hipMemcpyDeviceToHost, nullptr));
    HIP_CHECK(hipStreamSynchronize(nullptr));
    RandomKeys keys = random_sorted_keys(T, nullptr, occ, true);
    random_done(T, nullptr);
    return keys;
}

// One batch of a single-end plan.  Combinations beyond the dense limit travel as a key stream (sparse mode); otherwise
// the staged kernels can write an index stream for the tally (use_tally), and what remains counts with atomics on the
// replicas, folded behind the kernel.
void launch_batch(scg_plan* P, const ScgReads& R, int64_t n, hipStream_t stream) {
    if (P->kind == scg_plan::RANDOM) { launch_batch_random(P, R, n, stream); return; }
    if (P->kind == scg_plan::DUAL_SE_DIAG) { launch_batch_se_diag(P, R, n, stream); return; }
    scg_plan::Timer timer(P, stream);
    ScgCounters counts = plan_counters(P);
    const bool tally = !P->sparse && P->kind != scg_plan::COMBO_REGIONS && use_tally(P, n) && scg::staged_takes(R.max_len) && !general_only(P);
    if (P->sparse) counts.unit_pair = begin_pairs(P, stream, n);
    else if (tally) counts.unit_index = index_stream(P, stream, n);
    if (P->kind == scg_plan::SINGLE) {
        HIP_CHECK(scg::launch_single(single_params(P, P->tab[0].view), P->ht1.t.len, R, n, counts, P->error_flag.as<int32_t>(), stream));
    } else if (P->kind == scg_plan::COMBO_REGIONS) {       // (cells or a key stream; its kernels write no index stream)
        HIP_CHECK(scg::launch_combo_regions(combo_regions_params(P), P->ht1.t.len, R, n, counts, P->error_flag.as<int32_t>(), stream));
    } else {
        HIP_CHECK(scg::launch_combo(combo_params(P), P->ht1.t.len, R, n, counts, P->error_flag.as<int32_t>(), stream));
    }
    timer.stop();                                          // kernel statistics cover the counting kernel, as in rocprof
    if (P->sparse) finish_pairs(P, stream, n);
    else if (tally) HIP_CHECK(scg::launch_tally(counts.unit_index, n, P->counters, P->n_counters, stream));
    else fold_replicas(P, stream);
    P->total += n;
}

// One batch of a single-barcode plan, assigned: launch_single's kernels under the state-keeping policy, writing to the
// caller's arrays.  Counters, replicas, index streams and the total are not touched; only the error flag is shared.
void launch_batch_assign(scg_plan* P, const ScgReads& R, int64_t n, const ScgAssignOut& out, hipStream_t stream) {
    HIP_CHECK(scg::launch_assign(single_params(P, P->tab[0].view), P->ht1.t.len, R, n, out, P->error_flag.as<int32_t>(), stream));
}

// Paired-end kernels search each template on ONE strand, fixed per plan: they get the scan description with that strand in
// the forward fields, so that they neither carry both strands' seeds and planes in SGPRs nor select between them at run time.
ScgScan searched_strand_first(const ScgScan& t, bool reverse) {
    if (!reverse) return t;
    ScgScan o = t;
    o.fseeds = t.rseeds; o.rseeds = t.fseeds;
    for (int r = 0; r < SCG_MAX_REGIONS; ++r) {
        o.fstart[r] = t.rstart[r]; o.rstart[r] = t.fstart[r];
        o.flen[r] = t.rlen[r]; o.rlen[r] = t.flen[r];
    }
    for (int w = 0; w < SCG_MAX_TEMPLATE / 32; ++w) {
        o.fplane0[w] = t.rplane0[w]; o.rplane0[w] = t.fplane0[w];
        o.fplane1[w] = t.rplane1[w]; o.rplane1[w] = t.fplane1[w];
        o.fmask[w] = t.rmask[w]; o.rmask[w] = t.fmask[w];
    }
    return o;
}

// One batch of a single-barcode plan over pairs: the index stream and the tally when both mates are staged (use_tally),
// the replicas otherwise.
static void launch_batch_single_paired(scg_plan* P, const ScgReads& R1, const ScgReads& R2, int64_t n, hipStream_t stream) {
    scg_plan::Timer timer(P, stream);
    ScgCounters counts = plan_counters(P);
    const bool staged = scg::staged_takes(std::min(R1.max_len, R2.max_len)) && scg::staged_takes(std::max(R1.max_len, R2.max_len)) && !general_only(P);
    const bool tally = use_tally(P, n) && staged;
    if (tally) counts.unit_index = index_stream(P, stream, n);
    HIP_CHECK(scg::launch_single_paired(single_params(P, P->tab[0].view), P->ht1.t.len, R1, R2, n, counts, P->error_flag.as<int32_t>(), stream));
    timer.stop();
    if (tally) HIP_CHECK(scg::launch_tally(counts.unit_index, n, P->counters, P->n_counters, stream));
    else fold_replicas(P, stream);
    P->total += n;
}

void launch_batch_paired(scg_plan* P, const ScgReads& R1, const ScgReads& R2, int64_t n, hipStream_t stream) {
    if (P->kind == scg_plan::SINGLE_PAIRED) { launch_batch_single_paired(P, R1, R2, n, stream); return; }
    scg_plan::Timer timer(P, stream);
    ScgDualParams dp = ScgDualParams();
    dp.scan1 = searched_strand_first(P->scan1, P->rev1); dp.scan2 = searched_strand_first(P->scan2, P->rev2);
    dp.tmpl1 = P->d_tmpl1.as<ScgTemplate>(); dp.tmpl2 = P->d_tmpl2.as<ScgTemplate>();
    dp.index1 = P->tab[0].view; dp.index2 = P->tab[1].view; dp.pairs = P->pairs.view;
    dp.rev1 = P->rev1; dp.rev2 = P->rev2; dp.max_mm1 = P->max_mm1; dp.max_mm2 = P->max_mm2;
    dp.randomized = P->randomized; dp.use_first = P->use_first;
    dp.diagnostics = P->diagnostics; dp.n_pool = P->diagnostics == 2 ? 0 : P->n_pool[0]; dp.n_uid2 = static_cast<int32_t>(P->first2.size());
    dp.keep_first = P->diagnostics == 1; dp.only_if_negative = nullptr;
    ScgCounters counts = plan_counters(P);
    if (P->sparse) counts.unit_pair = begin_pairs(P, stream, n);      // (the invalid / all combinations of the diagnostics passes)
    const int lo_len = std::min(R1.max_len, R2.max_len), hi_len = std::max(R1.max_len, R2.max_len);
    const bool staged = scg::staged_takes(lo_len) && scg::staged_takes(hi_len) && !general_only(P);
    const int tmpl_len = std::max(P->ht1.t.len, P->ht2.t.len);
    dp.overflow = nullptr;
    if (staged && P->diagnostics != 2 && n < INT32_MAX) {
        DevBuf& buf = P->overflow[stream];
        buf.ensure((static_cast<size_t>(n) + 1) * sizeof(int32_t));
        dp.overflow = buf.as<int32_t>();
    }
    if (P->diagnostics == 1 && staged) {
        // include.invalid=TRUE in two lean passes: valid pairs as an index stream (tallied), then the mate-by-mate
        // search on the pairs that found none
        ScgCounters c1 = counts;
        c1.unit_index = index_stream(P, stream, n);
        c1.unit_pair = nullptr;
        dp.diagnostics = 0;
        HIP_CHECK(scg::launch_dual(dp, tmpl_len, R1, R2, n, c1, P->error_flag.as<int32_t>(), stream));
        HIP_CHECK(scg::launch_tally(c1.unit_index, n, P->counters, P->n_pool[0], stream));
        dp.diagnostics = 2;
        dp.only_if_negative = c1.unit_index;
        HIP_CHECK(scg::launch_dual(dp, tmpl_len, R1, R2, n, counts, P->error_flag.as<int32_t>(), stream));
        timer.stop();
        if (P->sparse) finish_pairs(P, stream, n);
        fold_replicas(P, stream);
        HIP_CHECK(scg::launch_hot_fold(P->hot.as<int32_t>(), P->counters + P->n_pool[0], stream));
        P->total += n;
        return;
    }
    const bool tally = use_tally(P, n) && staged;
    if (tally) counts.unit_index = index_stream(P, stream, n);
    HIP_CHECK(scg::launch_dual(dp, tmpl_len, R1, R2, n, counts, P->error_flag.as<int32_t>(), stream));
    timer.stop();
    if (P->sparse) finish_pairs(P, stream, n);
    if (tally) HIP_CHECK(scg::launch_tally(counts.unit_index, n, P->counters, P->n_counters, stream));
    else fold_replicas(P, stream);
    if (P->hot.p) HIP_CHECK(scg::launch_hot_fold(P->hot.as<int32_t>(), P->counters + (P->diagnostics == 2 ? 0 : P->n_pool[0]), stream));
    P->total += n;
}

} // namespace scgapi
