// scg_results.cpp -- what a file-level call has around its pipelines: the devices it may use, the plans on them (PlanSet),
// the scheduling of many files over them, and the shaping of counters into the reference's outputs: one reader per kind
// of result (result_counts, result_combinations, result_diagnostics), shared by the plan, one-file and many-files entries;
// and the matrices of many files: random barcodes (result_random_matrix) and combinations (combine_lists, on the device).
#include "scg_internal.hpp"
#include "scg_gzip.h"

namespace scgapi {

void reset_plan(scg_plan* P) {
    DeviceGuard g(P->device);
    if (P->n_counters) HIP_CHECK(hipMemset(P->counters, 0, static_cast<size_t>(P->n_counters) * sizeof(int32_t)));
    if (P->replica_shift > 0) HIP_CHECK(hipMemset(P->replicas.p, 0, P->replicas.bytes));
    HIP_CHECK(hipMemset(P->error_flag.p, 0, sizeof(int32_t)));    // (what set it is recounted, or belongs to the previous file)
    HIP_CHECK(hipStreamSynchronize(nullptr));               // (the fills are only enqueued: scg_plan::upload)
    drop_pending_pairs(P);                                  // (sparse mode: batches in flight are let finish and dropped)
    P->sparse_counts.clear();
    P->total = 0;
    if (P->kind == scg_plan::RANDOM && P->rnd->files) random_soft_reset(P);    // (the table's keys and ids stay for the next file)
}

// The reference's totals and counters are 32-bit `int`s (SingleBarcodeSingleEnd.hpp:132-133) and R integers
// are 32-bit; a file with more reads than that would overflow them silently there.  Here the total is kept
// in 64 bits and narrowing at the ABI is checked; no counter can exceed the total.
int32_t narrow_total(int64_t total) {
    if (total > static_cast<int64_t>(INT32_MAX)) {
        throw Error(SCG_ERR_INVALID, "number of reads (" + std::to_string(total) + ") exceeds the 32-bit range of the count vectors");
    }
    return static_cast<int32_t>(total);
}

void read_counters(scg_plan* P, int32_t* counts_out) {
    int32_t flag = 0;
    HIP_CHECK(hipMemcpy(&flag, P->error_flag.p, sizeof(flag), hipMemcpyDeviceToHost));
    if (flag) {
        throw Error(SCG_ERR_INVALID, "a read is longer than the max_len declared for its batch: counts are incomplete");
    }
    if (counts_out && P->n_counters) {
        HIP_CHECK(hipMemcpy(counts_out, P->counters, static_cast<size_t>(P->n_counters) * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
}

// ---- devices and plan sets ---------------------------------------------------------------------------------
// Which devices a file-level call may use: $SCG_DEVICES ("all", or a comma list in which an id may repeat: several
// pipelines on one card) if set; else every visible device, the calling thread's current one ($SCG_DEVICE) first.
thread_local std::vector<int> tl_devices;       // scg_set_devices(): overrides $SCG_DEVICES for the calling thread

std::vector<int> device_list(bool* explicit_list) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        throw Error(SCG_ERR_DEVICE, "no HIP device available: libscg has no CPU fallback");
    }
    if (!tl_devices.empty()) {
        for (int v : tl_devices) {
            if (v < 0 || v >= n) throw Error(SCG_ERR_DEVICE, "HIP device " + std::to_string(v) + " out of range (" + std::to_string(n) + " visible)");
        }
        if (explicit_list) *explicit_list = true;
        return tl_devices;
    }
    std::vector<int> out;
    const char* list = scg::env().devices.c_str();       // (empty when unset)
    if (explicit_list) *explicit_list = *list && std::strcmp(list, "all") != 0;
    if (*list && std::strcmp(list, "all") != 0) {
        const char* p = list;
        while (*p) {
            char* end = nullptr;
            const long v = std::strtol(p, &end, 10);
            if (end == p) throw Error(SCG_ERR_DEVICE, std::string("cannot parse SCG_DEVICES='") + list + "'");
            if (v < 0 || v >= n) throw Error(SCG_ERR_DEVICE, "HIP device " + std::to_string(v) + " out of range (" + std::to_string(n) + " visible)");
            out.push_back(static_cast<int>(v));
            p = end;
            while (*p == ',' || *p == ' ') ++p;
        }
        if (out.empty()) throw Error(SCG_ERR_DEVICE, "SCG_DEVICES lists no device");
        return out;
    }
    const int first = resolve_device(-1);
    const bool only_one = scg::env().device_set && !scg::env().devices_set;
    out.push_back(first);
    if (!only_one) for (int d = 0; d < n; ++d) if (d != first) out.push_back(d);
    return out;
}

// Devices for ONE input of about `text_bytes` of FASTQ text: an explicit $SCG_DEVICES is taken as given; otherwise one
// more device per four windows of text, so that small files do not pay for contexts and pinned buffers they cannot use.
std::vector<int> devices_for_input(uint64_t text_bytes, size_t window) {
    bool given = false;
    std::vector<int> all = device_list(&given);
    if (given) return all;
    const uint64_t per_device = uint64_t(4) * window;
    const size_t want = static_cast<size_t>(std::max<uint64_t>(1, text_bytes / per_device));
    if (all.size() > want) all.resize(want);
    return all;
}

uint64_t text_bytes_hint(const char* path) {
    struct stat st;
    if (!path || ::stat(path, &st) != 0) return 0;
    unsigned char h[2] = {0, 0};
    FILE* f = std::fopen(path, "rb");
    size_t got = 0;
    if (f) { got = std::fread(h, 1, 2, f); std::fclose(f); }
    return static_cast<uint64_t>(st.st_size) * (got == 2 && scg::gz::is_gzip(h) ? 5 : 1);
}

// A second plan with the same compiled (host-side) content, for another device.  Call before to_device().
std::unique_ptr<scg_plan> clone_compiled(const scg_plan& a) {
    std::unique_ptr<scg_plan> b(new scg_plan);
    b->kind = a.kind;
    b->ht1 = a.ht1; b->ht2 = a.ht2;
    b->scan1 = a.scan1; b->scan2 = a.scan2;
    b->htab[0] = a.htab[0]; b->htab[1] = a.htab[1];
    b->hpairs = a.hpairs;
    b->htab_combined = a.htab_combined;
    b->n_pool[0] = a.n_pool[0]; b->n_pool[1] = a.n_pool[1];
    b->max_mm1 = a.max_mm1; b->max_mm2 = a.max_mm2;
    b->rev1 = a.rev1; b->rev2 = a.rev2; b->randomized = a.randomized; b->use_first = a.use_first;
    b->diagnostics = a.diagnostics;
    b->first1 = a.first1; b->first2 = a.first2;
    b->n_regions = a.n_regions; b->hpools = a.hpools; b->pool_sizes = a.pool_sizes;
    std::copy(a.stride, a.stride + SCG_MAX_REGIONS, b->stride);
    b->n_counters = a.n_counters;
    b->sparse = a.sparse;
    if (a.rnd) {                                            // (the tally's settings; its table is made by random_to_device)
        b->rnd.reset(new RandomTally);
        b->rnd->vstart = a.rnd->vstart; b->rnd->vlen = a.rnd->vlen; b->rnd->tag_bits = a.rnd->tag_bits;
        b->rnd->files = a.rnd->files;
    }
    return b;
}

// Files over devices inside one call (the matrixOf* functions: R/countSingleBarcodes.R:112-126, R/countComboBarcodes.R:149-164,
// R/countDualBarcodes.R:205-254 hand the files to BiocParallel workers): every device runs one pipeline at a time and takes
// the next unprocessed file when it is done; per_file(plan, i) counts file i and stores its column.  The error of the
// lowest-numbered failing file is reported, as a serial loop over the files would.
void schedule_files(int32_t n_files, const PlanSet& set, const std::function<void(scg_plan*, int32_t)>& per_file) {
    std::atomic<int32_t> next(0), first_bad(n_files);
    std::mutex mu;
    int32_t bad = n_files;
    int bad_code = 0;
    std::string bad_msg;
    auto worker = [&](scg_plan* P) {
        for (;;) {
            const int32_t i = next.fetch_add(1);
            if (i >= n_files) return;
            if (i > first_bad.load()) return;      // a file before this one has failed: the call reports that error, whatever comes after
            int code = 0;
            std::string msg;
            try {
                DeviceGuard g(P->device);
                per_file(P, i);
                continue;
            } catch (const Error& e) { code = e.code; msg = e.what();
            } catch (const std::bad_alloc&) { code = SCG_ERR_DEVICE; msg = "out of host memory";
            } catch (const std::exception& e) { code = SCG_ERR_INVALID; msg = e.what(); }
            std::lock_guard<std::mutex> g(mu);
            if (i < bad) { bad = i; bad_code = code; bad_msg = msg; first_bad.store(i); }
        }
    };
    std::vector<std::thread> th;
    for (size_t d = 1; d < set.plans.size(); ++d) th.emplace_back(worker, set.plans[d].get());
    worker(set.plans[0].get());
    for (auto& t : th) t.join();
    if (bad < n_files) throw Error(bad_code, bad_msg);
}

// What the many-files entries share: at most one device per file; and per file of a worker's plan: the readers, a full
// reset of the plan, the file's ladder, then `read_file(plan, f)` stores file f's outputs.
std::vector<int> devices_for_files(int32_t n_files) {
    std::vector<int> devices = device_list();
    if (devices.size() > static_cast<size_t>(n_files)) devices.resize(static_cast<size_t>(n_files));
    return devices;
}
void schedule_single_end(int32_t n_files, const PlanSet& set, const char* const* paths, int nthreads, const std::function<void(scg_plan*, int32_t)>& read_file) {
    schedule_files(n_files, set, [&](scg_plan* P, int32_t f) {
        scg::FastqStream fq(paths[f]);
        reset_plan(P);
        count_single_end(std::vector<scg_plan*>(1, P), paths[f], fq, nthreads);
        read_file(P, f);
    });
}
void schedule_paired(int32_t n_files, const PlanSet& set, const char* const* paths1, const char* const* paths2, int nthreads,
                     const std::function<void(scg_plan*, int32_t)>& read_file) {
    schedule_files(n_files, set, [&](scg_plan* P, int32_t f) {
        scg::FastqStream fq1(paths1[f]);
        scg::FastqStream fq2(paths2[f]);
        reset_plan(P);
        count_paired_files(P, paths1[f], paths2[f], fq1, fq2, nthreads);
        read_file(P, f);
    });
}

void combo_compact(const int32_t* cells, int32_t n0, int32_t n1, int32_t** indices_out, int32_t** freq_out, int64_t* k_out) {
    int64_t total = static_cast<int64_t>(n0) * n1, k = 0;
    for (int64_t c = 0; c < total; ++c) k += cells[c] != 0;
    OutPair<int32_t, int32_t> out(static_cast<size_t>(2 * k + 1), static_cast<size_t>(k + 1));
    int64_t j = 0;
    // cell order = (first, second) lexicographic order = the reference's sorted column order
    for (int64_t c = 0; c < total; ++c) {
        if (cells[c]) {
            out.a[2 * j] = static_cast<int32_t>(c / n1);
            out.a[2 * j + 1] = static_cast<int32_t>(c % n1);
            out.b[j] = cells[c];
            ++j;
        }
    }
    out.release(indices_out, freq_out);
    *k_out = k;
}

// Sparse mode: (first << 32 | second) -> count, as the reference's sorted run-length form (src/utils.h:14-45).
void combos_from_sparse(const std::unordered_map<uint64_t, int64_t>& m, int32_t** indices_out, int32_t** freq_out, int64_t* k_out) {
    std::vector<std::pair<uint64_t, int64_t> > rows(m.begin(), m.end());
    std::sort(rows.begin(), rows.end());                    // key order = (first, second) order
    const size_t k = rows.size();
    OutPair<int32_t, int32_t> out(2 * k + 1, k + 1);
    for (size_t j = 0; j < k; ++j) {
        if (rows[j].second > static_cast<int64_t>(INT32_MAX)) throw Error(SCG_ERR_INVALID, "a count exceeds the 32-bit range of the count vectors");
        out.a[2 * j] = static_cast<int32_t>(rows[j].first >> 32);
        out.a[2 * j + 1] = static_cast<int32_t>(rows[j].first & 0xFFFFFFFFu);
        out.b[j] = static_cast<int32_t>(rows[j].second);
    }
    out.release(indices_out, freq_out);
    *k_out = static_cast<int64_t>(k);
}

// [n_pool valid][b1][b2][uid1 x uid2] -> the reference's outputs: invalid combinations by first pool
// index, merged (several uids of one IUPAC barcode share an index), sorted by (first, second).
// (sparse: the plan is in sparse mode and these are its combinations by sequence uid, in place of the dense cells)
void diagnostics_from_counters(const scg_plan* P, const std::vector<int32_t>& all, int32_t* counts_out,
                               int32_t** idx_out, int32_t** freq_out, int64_t* k_out, int32_t* b1, int32_t* b2,
                               const std::unordered_map<uint64_t, int64_t>* sparse) {
    const int32_t n_pool = P->n_pool[0];
    if (counts_out) std::copy(all.begin(), all.begin() + n_pool, counts_out);
    *b1 = all[n_pool];
    *b2 = all[n_pool + 1];
    const int32_t* cells = all.data() + n_pool + 2;
    const size_t nu1 = P->first1.size(), nu2 = P->first2.size();
    std::vector<std::pair<std::pair<int32_t, int32_t>, int32_t> > found;
    if (sparse) {
        for (auto& kv : *sparse) {
            const size_t u1 = static_cast<size_t>(kv.first >> 32), u2 = static_cast<size_t>(kv.first & 0xFFFFFFFFu);
            if (u1 >= nu1 || u2 >= nu2) throw Error(SCG_ERR_DEVICE, "internal: combination out of range");
            if (kv.second > static_cast<int64_t>(INT32_MAX)) throw Error(SCG_ERR_INVALID, "a count exceeds the 32-bit range of the count vectors");
            found.push_back(std::make_pair(std::make_pair(P->first1[u1], P->first2[u2]), static_cast<int32_t>(kv.second)));
        }
    } else {
        for (size_t u1 = 0; u1 < nu1; ++u1) {
            for (size_t u2 = 0; u2 < nu2; ++u2) {
                int32_t c = cells[u1 * nu2 + u2];
                if (c) found.push_back(std::make_pair(std::make_pair(P->first1[u1], P->first2[u2]), c));
            }
        }
    }
    std::sort(found.begin(), found.end());
    std::vector<int32_t> idx, freq;
    for (size_t i = 0; i < found.size(); ++i) {
        if (i && found[i].first == found[i - 1].first) {
            freq.back() += found[i].second;
        } else {
            idx.push_back(found[i].first.first);
            idx.push_back(found[i].first.second);
            freq.push_back(found[i].second);
        }
    }
    vectors_out(idx, 1, freq, 1, idx_out, freq_out);
    *k_out = static_cast<int64_t>(freq.size());
}

PlanSet::PlanSet(std::unique_ptr<scg_plan> compiled, const std::vector<int>& devices) {
    for (size_t i = 1; i < devices.size(); ++i) plans.push_back(clone_compiled(*compiled));
    plans.insert(plans.begin(), std::move(compiled));
    for (size_t i = 0; i < plans.size(); ++i) {
        plans[i]->to_device(devices[i]);
        if (plans[i]->kind == scg_plan::RANDOM) random_to_device(plans[i].get());
    }
}
std::vector<scg_plan*> PlanSet::all() const {
    std::vector<scg_plan*> v;
    for (auto& p : plans) v.push_back(p.get());
    return v;
}

// ---- one counted input -> the outputs of its entry point ------------------------------------------------------
int64_t total_of(const std::vector<scg_plan*>& plans) {
    int64_t t = 0;
    for (scg_plan* p : plans) t += p->total;
    return t;
}

void read_plans(const std::vector<scg_plan*>& plans, int32_t* counts_out) {
    if (plans.size() == 1) {
        DeviceGuard g(plans[0]->device);
        read_counters(plans[0], counts_out);
        return;
    }
    const size_t n = static_cast<size_t>(plans[0]->n_counters);
    std::vector<int64_t> acc(n, 0);
    std::vector<int32_t> part(n + 1);
    for (scg_plan* p : plans) {
        DeviceGuard g(p->device);
        read_counters(p, part.data());
        for (size_t i = 0; i < n; ++i) acc[i] += part[i];
    }
    if (counts_out) {
        for (size_t i = 0; i < n; ++i) {
            if (acc[i] > static_cast<int64_t>(INT32_MAX)) throw Error(SCG_ERR_INVALID, "a count exceeds the 32-bit range of the count vectors");
            counts_out[i] = static_cast<int32_t>(acc[i]);
        }
    }
}

std::unordered_map<uint64_t, int64_t> sparse_merged(const std::vector<scg_plan*>& plans) {
    std::unordered_map<uint64_t, int64_t> all;
    for (scg_plan* p : plans) {
        retire_all_pairs(p);
        if (all.empty()) all = p->sparse_counts;
        else for (auto& kv : p->sparse_counts) all[kv.first] += kv.second;
    }
    return all;
}

void result_counts(const std::vector<scg_plan*>& plans, int32_t* counts_out, int32_t* total_out) {
    read_plans(plans, counts_out);
    *total_out = narrow_total(total_of(plans));
}

void result_combinations(const std::vector<scg_plan*>& plans, int32_t** idx_out, int32_t** freq_out, int64_t* k_out, int32_t* total_out) {
    const scg_plan* P = plans[0];
    if (P->kind == scg_plan::COMBO_REGIONS) { result_combinations_regions(plans, idx_out, freq_out, k_out, total_out); return; }
    std::vector<int32_t> cells(static_cast<size_t>(P->n_counters) + 1);
    read_plans(plans, cells.data());
    const int32_t total = total_out ? narrow_total(total_of(plans)) : 0;      // (before anything is allocated for the caller)
    if (P->sparse) combos_from_sparse(sparse_merged(plans), idx_out, freq_out, k_out);
    else combo_compact(cells.data(), P->n_pool[0], P->n_pool[1], idx_out, freq_out, k_out);
    if (total_out) *total_out = total;
}

void result_diagnostics(const std::vector<scg_plan*>& plans, int32_t* counts_out, int32_t** idx_out, int32_t** freq_out, int64_t* k_out,
                        int32_t* total_out, int32_t* b1_out, int32_t* b2_out) {
    const scg_plan* P = plans[0];
    std::vector<int32_t> all(static_cast<size_t>(P->n_counters) + 1);
    read_plans(plans, all.data());
    const int32_t total = narrow_total(total_of(plans));       // (before anything is allocated for the caller)
    int32_t b1 = 0, b2 = 0;
    const auto sparse = P->sparse ? sparse_merged(plans) : std::unordered_map<uint64_t, int64_t>();
    diagnostics_from_counters(P, all, counts_out, idx_out, freq_out, k_out, b1_out ? b1_out : &b1, b2_out ? b2_out : &b2,
                              P->sparse ? &sparse : nullptr);
    *total_out = total;
}

// The matrix of matrixOfRandomBarcodes (R/countRandomBarcodes.R:87-92).  Every plan's keys come sorted with their ids;
// the lists -- one per device, as a rule -- are merged with memcmp, equal keys of several plans sharing a row, and a key
// that no file counted (first seen in a pass that was abandoned) gets no row.
void result_random_matrix(const PlanSet& set, const std::vector<int>& plan_of, const std::vector<std::vector<int32_t> >& pairs,
                          char** sequences_out, int64_t* k_out, int32_t* length_out, int64_t** col_ptr_out, int32_t** rows_out, int32_t** freq_out) {
    const size_t n_plans = set.plans.size(), n_files = pairs.size();
    const int vlen = set.first()->rnd->vlen;
    const size_t stride = static_cast<size_t>(vlen) + 1;
    std::vector<RandomKeys> keys(n_plans);
    std::vector<std::vector<int64_t> > row_of_id(n_plans);    // id -> place in the plan's sorted list
    std::vector<std::vector<char> > counted(n_plans);         // by place in the plan's sorted list
    for (size_t p = 0; p < n_plans; ++p) {
        keys[p] = random_keys_with_ids(set.plans[p].get());
        const size_t n = keys[p].vals.size();
        row_of_id[p].assign(n, -1);
        counted[p].assign(n, 0);
        for (size_t i = 0; i < n; ++i) {
            if (keys[p].vals[i] >= n || row_of_id[p][keys[p].vals[i]] >= 0) throw Error(SCG_ERR_DEVICE, "internal: random barcode tally: row ids are not a permutation");
            row_of_id[p][keys[p].vals[i]] = static_cast<int64_t>(i);
        }
    }
    size_t nnz = 0;
    for (size_t f = 0; f < n_files; ++f) {
        const size_t p = static_cast<size_t>(plan_of[f]);
        for (size_t j = 0; j < pairs[f].size(); j += 2) {
            const int32_t id = pairs[f][j];
            if (id < 0 || static_cast<size_t>(id) >= row_of_id[p].size()) throw Error(SCG_ERR_DEVICE, "internal: random barcode tally: row id out of range");
            counted[p][static_cast<size_t>(row_of_id[p][id])] = 1;
        }
        nnz += pairs[f].size() / 2;
    }
    // the union: the smallest key under the plans' cursors takes the next row, in every plan that holds it
    std::vector<size_t> at(n_plans, 0);
    std::vector<std::vector<int64_t> > row_of_place(n_plans);  // place in the plan's sorted list -> row of the union (-1: no file counted it)
    for (size_t p = 0; p < n_plans; ++p) row_of_place[p].assign(counted[p].size(), -1);
    std::vector<const char*> union_keys;
    for (;;) {
        const char* least = nullptr;
        for (size_t p = 0; p < n_plans; ++p) {
            while (at[p] < counted[p].size() && !counted[p][at[p]]) ++at[p];
            if (at[p] == counted[p].size()) continue;
            const char* k = keys[p].bytes.get() + at[p] * stride;
            if (!least || std::memcmp(k, least, static_cast<size_t>(vlen)) < 0) least = k;
        }
        if (!least) break;
        for (size_t p = 0; p < n_plans; ++p) {
            if (at[p] < counted[p].size() && std::memcmp(keys[p].bytes.get() + at[p] * stride, least, static_cast<size_t>(vlen)) == 0) {
                row_of_place[p][at[p]++] = static_cast<int64_t>(union_keys.size());
            }
        }
        union_keys.push_back(least);
    }
    const size_t K = union_keys.size();
    if (K > static_cast<size_t>(INT32_MAX)) throw Error(SCG_ERR_INVALID, "number of distinct random barcodes exceeds the 32-bit range of the row indices");
    OutPair<char, int64_t> head(K * stride + 1, n_files + 1);
    OutPair<int32_t, int32_t> body(nnz + 1, nnz + 1);
    for (size_t k = 0; k < K; ++k) {
        std::memcpy(head.a + k * stride, union_keys[k], static_cast<size_t>(vlen));
        head.a[k * stride + vlen] = 0;
    }
    std::vector<std::pair<int32_t, int32_t> > column;
    size_t filled = 0;
    for (size_t f = 0; f < n_files; ++f) {
        const size_t p = static_cast<size_t>(plan_of[f]);
        head.b[f] = static_cast<int64_t>(filled);
        column.clear();
        for (size_t j = 0; j < pairs[f].size(); j += 2) {
            const int64_t place = row_of_id[p][pairs[f][j]];
            column.push_back(std::make_pair(static_cast<int32_t>(row_of_place[p][place]), pairs[f][j + 1]));
        }
        std::sort(column.begin(), column.end());
        for (const auto& e : column) { body.a[filled] = e.first; body.b[filled] = e.second; ++filled; }
    }
    head.b[n_files] = static_cast<int64_t>(filled);
    head.release(sequences_out, col_ptr_out);
    body.release(rows_out, freq_out);
    *k_out = static_cast<int64_t>(K); *length_out = vlen;
}

// ---- combination counts of many files as one matrix (combineComboCounts, R/combineComboCounts.R:31-57) -------------------
namespace {

// A stream of its own for one compaction or one union: the workers of a many-files call share devices.
struct OwnStream {
    hipStream_t s = nullptr;
    OwnStream() { HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    OwnStream(const OwnStream&) = delete;
    OwnStream& operator=(const OwnStream&) = delete;
    ~OwnStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};

// Device buffers of `what`, all or SCG_ERR_DEVICE with the sizes asked for.
void alloc_all(const char* what, const std::string& sizes, const std::vector<std::pair<DevBuf*, size_t> >& wanted) {
    size_t bytes = 0;
    for (const auto& w : wanted) bytes += w.second;
    try {
        for (const auto& w : wanted) w.first->alloc(w.second);
    } catch (const Error& e) {
        throw Error(SCG_ERR_DEVICE, std::string("cannot allocate the device buffers of ") + what + " (" + sizes + ", " + std::to_string(bytes) +
                                        " bytes): " + e.what());
    }
}

} // namespace

void compact_cells_on_device(const int32_t* d_cells, int32_t n0, int32_t n1, ComboList& out) {
    out.keys.clear();
    out.counts.clear();
    if (n0 <= 0 || n1 <= 0) return;
    const uint64_t n_cells = static_cast<uint64_t>(n0) * static_cast<uint64_t>(n1);
    const uint64_t tiles = scg::compact_tiles(n_cells);
    if (tiles > static_cast<uint64_t>(INT32_MAX)) {
        throw Error(SCG_ERR_UNSUPPORTED, "a dense grid of " + std::to_string(n_cells) + " cells is beyond the device compaction (" +
                                             std::to_string(INT32_MAX) + " tiles of " + std::to_string(SCG_COMPACT_TILE_CELLS) + " cells)");
    }
    const std::string grid = std::to_string(n0) + " x " + std::to_string(n1) + " cells";
    OwnStream st;
    DevBuf tile_counts, tile_offsets, scratch, keys, counts;
    const size_t scratch_bytes = scg::compact_scan_scratch_bytes(n_cells);
    alloc_all("the combination compaction", grid, {{&tile_counts, (tiles + 1) * sizeof(unsigned long long)},
                                                   {&tile_offsets, (tiles + 1) * sizeof(unsigned long long)}, {&scratch, scratch_bytes}});
    HIP_CHECK(scg::launch_compact_count(d_cells, n_cells, tile_counts.as<unsigned long long>(), tile_offsets.as<unsigned long long>(), scratch.p,
                                        scratch_bytes, st.s));
    // the one number the second pass's buffers depend on
    unsigned long long k = 0;
    HIP_CHECK(hipMemcpyAsync(&k, tile_offsets.as<unsigned long long>() + tiles, sizeof(k), hipMemcpyDeviceToHost, st.s));
    HIP_CHECK(hipStreamSynchronize(st.s));
    if (k == 0) return;
    if (k > n_cells) throw Error(SCG_ERR_DEVICE, "internal: combination compaction: more pairs than cells");
    alloc_all("the combination compaction", grid + ", " + std::to_string(k) + " pairs", {{&keys, k * sizeof(uint64_t)}, {&counts, k * sizeof(int32_t)}});
    HIP_CHECK(scg::launch_compact_scatter(d_cells, n_cells, static_cast<uint32_t>(n1), tile_offsets.as<unsigned long long>(), keys.as<uint64_t>(),
                                          counts.as<int32_t>(), st.s));
    out.keys.resize(k);
    out.counts.resize(k);
    HIP_CHECK(hipMemcpyAsync(out.keys.data(), keys.p, k * sizeof(uint64_t), hipMemcpyDeviceToHost, st.s));
    HIP_CHECK(hipMemcpyAsync(out.counts.data(), counts.p, k * sizeof(int32_t), hipMemcpyDeviceToHost, st.s));
    HIP_CHECK(hipStreamSynchronize(st.s));
}

void combo_list_of_plan(scg_plan* P, ComboList& out) {
    DeviceGuard g(P->device);
    read_counters(P, nullptr);                              // (the oversize-read flag, as before every read-out)
    if (!P->sparse) {
        compact_cells_on_device(P->counters, P->n_pool[0], P->n_pool[1], out);
        return;
    }
    const std::unordered_map<uint64_t, int64_t> m = sparse_merged(std::vector<scg_plan*>(1, P));
    std::vector<std::pair<uint64_t, int64_t> > rows(m.begin(), m.end());
    std::sort(rows.begin(), rows.end());
    out.keys.resize(rows.size());
    out.counts.resize(rows.size());
    for (size_t j = 0; j < rows.size(); ++j) {
        if (rows[j].second > static_cast<int64_t>(INT32_MAX)) throw Error(SCG_ERR_INVALID, "a count exceeds the 32-bit range of the count vectors");
        out.keys[j] = rows[j].first;
        out.counts[j] = static_cast<int32_t>(rows[j].second);
    }
}

void result_combinations_regions(const std::vector<scg_plan*>& plans, int32_t** idx_out, int32_t** freq_out, int64_t* k_out, int32_t* total_out) {
    const scg_plan* P0 = plans[0];
    const size_t nreg = static_cast<size_t>(P0->n_regions);
    std::vector<std::pair<uint64_t, int64_t> > rows;             // (mixed-radix key, count), ascending
    for (scg_plan* p : plans) {                                   // (the oversize-read flag, as before every read-out)
        DeviceGuard g(p->device);
        read_counters(p, nullptr);
    }
    if (P0->sparse) {
        const std::unordered_map<uint64_t, int64_t> m = sparse_merged(plans);
        rows.assign(m.begin(), m.end());
        std::sort(rows.begin(), rows.end());
    } else if (P0->n_counters > 0) {
        // the flat histogram as (all pools but the last) x (last pool): cell = head * n_last + last
        const int64_t n_last = P0->pool_sizes[nreg - 1], n_head = P0->n_counters / n_last;
        if (n_head > static_cast<int64_t>(INT32_MAX)) {
            throw Error(SCG_ERR_UNSUPPORTED, "a dense grid of " + std::to_string(n_head) + " x " + std::to_string(n_last) + " cells is beyond the device compaction");
        }
        for (scg_plan* p : plans) {
            DeviceGuard g(p->device);
            ComboList list;
            compact_cells_on_device(p->counters, static_cast<int32_t>(n_head), static_cast<int32_t>(n_last), list);
            const size_t before = rows.size();
            for (size_t j = 0; j < list.keys.size(); ++j) {
                rows.push_back(std::make_pair((list.keys[j] >> 32) * static_cast<uint64_t>(n_last) + (list.keys[j] & 0xFFFFFFFFu), static_cast<int64_t>(list.counts[j])));
            }
            if (before) {                                         // several devices: equal keys of two sorted lists share a row
                std::inplace_merge(rows.begin(), rows.begin() + static_cast<long>(before), rows.end());
                size_t w = 0;
                for (size_t j = 0; j < rows.size(); ++j) {
                    if (w && rows[w - 1].first == rows[j].first) rows[w - 1].second += rows[j].second;
                    else rows[w++] = rows[j];
                }
                rows.resize(w);
            }
        }
    }
    const int32_t total = total_out ? narrow_total(total_of(plans)) : 0;      // (before anything is allocated for the caller)
    const size_t k = rows.size();
    OutPair<int32_t, int32_t> out(nreg * k + 1, k + 1);
    for (size_t j = 0; j < k; ++j) {
        if (rows[j].second > static_cast<int64_t>(INT32_MAX)) throw Error(SCG_ERR_INVALID, "a count exceeds the 32-bit range of the count vectors");
        uint64_t key = rows[j].first;
        for (size_t r = nreg; r-- > 0;) {
            const uint64_t size = static_cast<uint64_t>(P0->pool_sizes[r]);
            if (size == 0 || (r == 0 && key >= size)) throw Error(SCG_ERR_DEVICE, "internal: combination out of range");
            out.a[nreg * j + r] = static_cast<int32_t>(key % size);
            key /= size;
        }
        out.b[j] = static_cast<int32_t>(rows[j].second);
    }
    out.release(idx_out, freq_out);
    *k_out = static_cast<int64_t>(k);
    if (total_out) *total_out = total;
}

void combo_list_of_outputs(const int32_t* idx, const int32_t* freq, int64_t k, ComboList& out) {
    out.keys.resize(static_cast<size_t>(k));
    out.counts.assign(freq, freq + k);
    for (int64_t j = 0; j < k; ++j) {
        if (idx[2 * j] < 0 || idx[2 * j + 1] < 0) throw Error(SCG_ERR_INVALID, "negative barcode index in a combination");
        out.keys[static_cast<size_t>(j)] = (static_cast<uint64_t>(static_cast<uint32_t>(idx[2 * j])) << 32) | static_cast<uint32_t>(idx[2 * j + 1]);
    }
}

void empty_combo_matrix(int32_t n_files, int32_t** indices_out, int64_t* k_out, int64_t** col_ptr_out, int32_t** rows_out, int32_t** freq_out) {
    OutPair<int32_t, int64_t> head(1, static_cast<size_t>(n_files) + 1);
    OutPair<int32_t, int32_t> body(1, 1);
    head.a[0] = 0; body.a[0] = 0; body.b[0] = 0;
    for (int32_t f = 0; f <= n_files; ++f) head.b[f] = 0;
    head.release(indices_out, col_ptr_out);
    body.release(rows_out, freq_out);
    *k_out = 0;
}

void combine_lists(const std::vector<ComboList>& lists, bool sorted_unique, int device, int32_t** indices_out, int64_t* k_out,
                   int64_t** col_ptr_out, int32_t** rows_out, int32_t** freq_out) {
    const size_t n_files = lists.size();
    uint64_t n = 0;
    size_t longest = 0;
    for (const ComboList& l : lists) { n += l.keys.size(); longest = std::max(longest, l.keys.size()); }
    if (n > 0xFFFFFFFFull) {
        throw Error(SCG_ERR_UNSUPPORTED, "the files hold " + std::to_string(n) + " combinations in all: more than the 4294967295 one union takes");
    }
    if (n == 0) {
        empty_combo_matrix(static_cast<int32_t>(n_files), indices_out, k_out, col_ptr_out, rows_out, freq_out);
        return;
    }
    std::vector<uint64_t> all_keys(n);
    std::vector<int32_t> all_counts(n);
    std::vector<size_t> start(n_files + 1, 0);
    for (size_t f = 0; f < n_files; ++f) {
        std::copy(lists[f].keys.begin(), lists[f].keys.end(), all_keys.begin() + static_cast<long>(start[f]));
        std::copy(lists[f].counts.begin(), lists[f].counts.end(), all_counts.begin() + static_cast<long>(start[f]));
        start[f + 1] = start[f] + lists[f].keys.size();
    }

    DeviceGuard g(device);
    OwnStream st;
    // keys: the files' lists back to back, every list ascending (as given, or sorted here with its counts in vals)
    DevBuf keys, sorted, unique, run_lengths, runs, rows, flags, scratch, raw_keys, raw_vals, vals;
    const size_t scratch_bytes = std::max(scg::sort_rle_scratch_bytes(n), sorted_unique ? size_t(0) : scg::sort_pairs_scratch_bytes(longest));
    std::vector<std::pair<DevBuf*, size_t> > wanted = {
        {&keys, n * sizeof(uint64_t)}, {&sorted, n * sizeof(uint64_t)}, {&unique, n * sizeof(uint64_t)}, {&run_lengths, n * sizeof(uint32_t)},
        {&runs, sizeof(uint32_t)}, {&rows, n * sizeof(int32_t)}, {&flags, 2 * sizeof(int32_t)}, {&scratch, scratch_bytes}};
    if (!sorted_unique) {
        wanted.push_back({&raw_keys, n * sizeof(uint64_t)});
        wanted.push_back({&raw_vals, n * sizeof(int32_t)});
        wanted.push_back({&vals, n * sizeof(int32_t)});
    }
    alloc_all("the union of the files' combinations", std::to_string(n) + " combinations of " + std::to_string(n_files) + " files", wanted);
    int32_t* const not_found = flags.as<int32_t>();         // flags[0]: a key without a row; flags[1]: a repeat within one list
    int32_t* const repeated = flags.as<int32_t>() + 1;
    HIP_CHECK(hipMemsetAsync(flags.p, 0, 2 * sizeof(int32_t), st.s));
    if (sorted_unique) {
        HIP_CHECK(hipMemcpyAsync(keys.p, all_keys.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st.s));
    } else {
        HIP_CHECK(hipMemcpyAsync(raw_keys.p, all_keys.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st.s));
        HIP_CHECK(hipMemcpyAsync(raw_vals.p, all_counts.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, st.s));
        for (size_t f = 0; f < n_files; ++f) {
            const size_t len = start[f + 1] - start[f];
            if (len == 0) continue;
            HIP_CHECK(scg::launch_sort_pairs(raw_keys.as<uint64_t>() + start[f], keys.as<uint64_t>() + start[f], raw_vals.as<int32_t>() + start[f],
                                             vals.as<int32_t>() + start[f], len, scratch.p, scratch_bytes, st.s));
            HIP_CHECK(scg::launch_flag_equal_neighbours(keys.as<uint64_t>() + start[f], len, repeated, st.s));
        }
    }
    HIP_CHECK(scg::launch_sort_rle(keys.as<uint64_t>(), sorted.as<uint64_t>(), n, unique.as<uint64_t>(), run_lengths.as<uint32_t>(), runs.as<uint32_t>(),
                                   scratch.p, scratch_bytes, st.s));
    HIP_CHECK(scg::launch_union_rows(keys.as<uint64_t>(), n, unique.as<uint64_t>(), runs.as<uint32_t>(), rows.as<int32_t>(), not_found, st.s));
    uint32_t n_unique = 0;
    int32_t flagged[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(&n_unique, runs.p, sizeof(n_unique), hipMemcpyDeviceToHost, st.s));
    HIP_CHECK(hipMemcpyAsync(flagged, flags.p, sizeof(flagged), hipMemcpyDeviceToHost, st.s));
    HIP_CHECK(hipStreamSynchronize(st.s));                  // the one wait of the union; the results are copied behind it
    if (flagged[1]) throw Error(SCG_ERR_INVALID, "barcode combinations should be unique within each DataFrame in '...'");   // R/combineComboCounts.R:50-52
    if (flagged[0]) throw Error(SCG_ERR_DEVICE, "internal: union of combinations: a combination has no row");
    if (n_unique > static_cast<uint32_t>(INT32_MAX)) {
        throw Error(SCG_ERR_INVALID, "number of distinct barcode combinations exceeds the 32-bit range of the row indices");
    }
    const size_t K = n_unique;
    std::vector<uint64_t> union_keys(K);
    HIP_CHECK(hipMemcpy(union_keys.data(), unique.p, K * sizeof(uint64_t), hipMemcpyDeviceToHost));
    OutPair<int32_t, int64_t> head(2 * K + 1, n_files + 1);
    OutPair<int32_t, int32_t> body(n + 1, n + 1);
    for (size_t k = 0; k < K; ++k) {
        head.a[2 * k] = static_cast<int32_t>(union_keys[k] >> 32);
        head.a[2 * k + 1] = static_cast<int32_t>(union_keys[k] & 0xFFFFFFFFu);
    }
    for (size_t f = 0; f <= n_files; ++f) head.b[f] = static_cast<int64_t>(start[f]);
    HIP_CHECK(hipMemcpy(body.a, rows.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (sorted_unique) std::memcpy(body.b, all_counts.data(), n * sizeof(int32_t));
    else HIP_CHECK(hipMemcpy(body.b, vals.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    head.release(indices_out, col_ptr_out);
    body.release(rows_out, freq_out);
    *k_out = static_cast<int64_t>(K);
}

void with_per_file_outputs(int32_t** idx_out, int32_t** freq_out, int64_t* k_out, int32_t n_files, const std::function<void()>& body) {
    for (int32_t f = 0; f < n_files; ++f) { idx_out[f] = nullptr; freq_out[f] = nullptr; k_out[f] = 0; }
    try {
        body();
    } catch (...) {
        for (int32_t f = 0; f < n_files; ++f) {
            std::free(idx_out[f]); std::free(freq_out[f]);
            idx_out[f] = nullptr; freq_out[f] = nullptr; k_out[f] = 0;
        }
        throw;
    }
}

void set_thread_devices(const int* devices, int32_t n) { tl_devices.assign(devices, devices + n); }

} // namespace scgapi
