// scg_api.cpp -- the C ABI (include/scg.h): every entry point, over the plans (scg_plan.cpp), the file entries
// (scg_files.cpp) and the read-out of results (scg_results.cpp).  An entry checks its pointers, keeps the reference's
// order of errors, and calls; no pipeline lives here.
//
// Host-side counterpart of the reference's Rcpp glue (src/count_single_barcodes.cpp,
// src/count_combo_barcodes_single.cpp, src/count_dual_barcodes.cpp, src/match_barcodes.cpp): same argument order,
// same checks in the same order, status + message instead of exceptions.
#include "scg_internal.hpp"

namespace {

// What the plan factories share: every argument check (`compile`: host work only) before any device work, then the upload;
// *plan_out is null whenever the call fails.
int new_plan(scg_plan** plan_out, int device, char* err, size_t errcap, const Compile& compile, void (*after_upload)(scg_plan*) = nullptr) {
    return guarded(err, errcap, [&] {
        if (!plan_out) throw Error(SCG_ERR_INVALID, "null argument");
        *plan_out = nullptr;
        std::unique_ptr<scg_plan> P = compile();
        P->to_device(device);
        if (after_upload) after_upload(P.get());
        *plan_out = P.release();
    });
}

// ---- many files on one compiled plan per device (matrixOf*) ------------------------------------------------------------
// What the nine many-files entries share, after the null-argument condition each states for itself.  An entry is: its
// lists of paths, the order of its first steps, what it compiles, and how a counted file is read out.

// One list of n_files paths (single-end), or two (paired: paths2 is not null).
struct FileLists { const char* const* paths1; const char* const* paths2; int32_t n_files; };

// The order of the first steps, which is the order of the entry's errors (include/scg.h, "Many files in one call").
enum class Order {
    ARGUMENTS_FIRST,        // compile, device list: argument errors before any file is opened or any device is touched
    FILE0_FIRST,            // reader(s) of file 0, device list, compile: a missing first file first, as in a loop over files
    FILE0_THEN_ARGUMENTS,   // reader of file 0, compile, device list (the random entry)
};

typedef std::function<void(scg_plan*, int32_t)> ReadFile;     // (the plan that counted file f, f) -> file f's outputs

// Null paths, no files (nothing is written; null), then the first steps in `order`, one plan per device, and every file
// counted by schedule_single_end / schedule_paired and read by `read_file`.  The plans are handed back for a read-out
// that needs them all (the random entry).
std::unique_ptr<PlanSet> count_files(const FileLists& files, int nthreads, Order order, const Compile& compile, const ReadFile& read_file) {
    const int32_t n = files.n_files;
    for (int32_t f = 0; f < n; ++f) if (!files.paths1[f] || (files.paths2 && !files.paths2[f])) throw Error(SCG_ERR_INVALID, "null argument");
    if (n == 0) return nullptr;
    if (order != Order::ARGUMENTS_FIRST) {
        scg::FastqStream probe1(files.paths1[0]);
        if (files.paths2) scg::FastqStream probe2(files.paths2[0]);
    }
    std::unique_ptr<PlanSet> set;
    if (order == Order::FILE0_FIRST) {
        const std::vector<int> devices = devices_for_files(n);
        set.reset(new PlanSet(compile(), devices));
    } else {
        std::unique_ptr<scg_plan> compiled = compile();
        set.reset(new PlanSet(std::move(compiled), devices_for_files(n)));
    }
    if (files.paths2) schedule_paired(n, *set, files.paths1, files.paths2, nthreads, read_file);
    else schedule_single_end(n, *set, files.paths1, nthreads, read_file);
    return set;
}

// The outputs of a many-files entry with a library, in the order of its prototype: caller-allocated arrays of n_files
// entries (null: the entry has no such output); `counts` is column-major, one column of n_pool[0] counts per file.
struct PerFile {
    int32_t* counts;
    int32_t** idx; int32_t** freq; int64_t* k;
    int32_t* totals; int32_t* b1; int32_t* b2;
};
enum class ReadOut { COUNTS, COMBINATIONS, DIAGNOSTICS };

// File f into entry f of those arrays, by the function the one-file entry reads its outputs with.  Column f starts at
// n_pool[0] * f, the plan's own pool count: the n_pool argument where the entry has one (compile_* store it), and all
// there is for the single-end dual entries.
void read_file_into(const PerFile& out, ReadOut what, scg_plan* P, int32_t f) {
    const std::vector<scg_plan*> plan(1, P);
    int32_t* column = out.counts ? out.counts + static_cast<size_t>(P->n_pool[0]) * static_cast<size_t>(f) : nullptr;
    switch (what) {
    case ReadOut::COUNTS: result_counts(plan, column, &out.totals[f]); break;
    case ReadOut::COMBINATIONS: result_combinations(plan, &out.idx[f], &out.freq[f], &out.k[f], &out.totals[f]); break;
    case ReadOut::DIAGNOSTICS:
        result_diagnostics(plan, column, &out.idx[f], &out.freq[f], &out.k[f], &out.totals[f], out.b1 ? &out.b1[f] : nullptr, out.b2 ? &out.b2[f] : nullptr);
        break;
    }
}

// count_files for the eight entries with a library.  Per-file pointer outputs are all-NULL (k: 0) before anything else
// happens -- the null paths included -- and again after any failure (with_per_file_outputs).
void count_files_into(const FileLists& files, int nthreads, Order order, const Compile& compile, ReadOut what, const PerFile& out) {
    auto run = [&] { count_files(files, nthreads, order, compile, [&](scg_plan* P, int32_t f) { read_file_into(out, what, P, f); }); };
    if (out.idx) with_per_file_outputs(out.idx, out.freq, out.k, files.n_files, run);
    else run();
}

} // namespace

// -------------------------------------------------------------------------------------------------
// C ABI
// -------------------------------------------------------------------------------------------------
#pragma GCC visibility push(default)     // the C ABI is the library's whole export list (csrc/Makefile: -fvisibility=hidden)
extern "C" {

const char* scg_version(void) { return "scg 0.3.0 (gfx950)"; }

int scg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void scg_free(void* p) { std::free(p); }

void scg_release_buffers(void) {
    release_cached_slots();
    scg::ParallelGunzip::release_cached();
    scg::release_device_gunzip_scratch();
}

int scg_parse_fastq(const char* path, char** seqs_out, uint64_t** offsets_out, int64_t* n_reads_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path || !seqs_out || !offsets_out || !n_reads_out) throw Error(SCG_ERR_INVALID, "null argument");
        scg::FastqStream fq(path);
        scg::ReadBatch all, b;
        all.clear();
        bool done = false;
        const int threads = scg::default_host_threads(1);
        if (threads > 1 && scg::ParallelFastq::is_plain_file(path)) {
            scg::ParallelFastq pf(path, threads);
            std::vector<scg::ReadBatch> window;
            while (pf.next_window(window)) {
                for (auto& w : window) {
                    uint64_t base = all.seqs.size();
                    all.seqs.insert(all.seqs.end(), w.seqs.begin(), w.seqs.end());
                    for (int64_t i = 1; i <= w.size(); ++i) all.offsets.push_back(base + w.offsets[i]);
                }
            }
            done = !pf.unusual();
            if (!done) all.clear();
        }
        while (!done && fq.next_batch(b, BATCH_READS, BATCH_BYTES)) {
            uint64_t base = all.seqs.size();
            all.seqs.insert(all.seqs.end(), b.seqs.begin(), b.seqs.end());
            for (int64_t i = 1; i <= b.size(); ++i) all.offsets.push_back(base + b.offsets[i]);
        }
        vectors_out(all.seqs, 1, all.offsets, 0, seqs_out, offsets_out);
        *n_reads_out = all.size();
    });
}

int scg_fastq_text_windows(const char* path, int64_t window_bytes, int nthreads, char** text_out, int64_t* n_bytes_out,
                           int64_t** cuts_out, int64_t* n_windows_out, char* kind_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path || !text_out || !n_bytes_out || !cuts_out || !n_windows_out || window_bytes < 64) throw Error(SCG_ERR_INVALID, "null argument");
        std::vector<char> all, window(static_cast<size_t>(window_bytes));
        std::vector<int64_t> cuts(1, 0);
        for (int attempt = 0; attempt < 2; ++attempt) {
            std::unique_ptr<scg::TextSource> src = scg::TextSource::open(path, scg::default_host_threads(nthreads), attempt == 0);
            if (kind_out) { std::strncpy(kind_out, src->kind(), 15); kind_out[15] = 0; }
            bool again = false;
            all.clear(); cuts.assign(1, 0);
            for (;;) {
                const size_t got = src->next(window.data(), window.size());
                if (src->unusual()) {
                    // (a gzip file the parallel decoder hands back is read again through one inflate stream, as the pipelines do)
                    if (attempt == 0 && is_parallel_gzip(src.get())) { again = true; break; }
                    throw Error(SCG_ERR_UNSUPPORTED, "the text cannot be cut into windows of whole 4-line records");
                }
                if (!got) break;
                all.insert(all.end(), window.begin(), window.begin() + got);
                cuts.push_back(static_cast<int64_t>(all.size()));
            }
            if (!again) break;
        }
        vectors_out(all, 1, cuts, 0, text_out, cuts_out);
        *n_bytes_out = static_cast<int64_t>(all.size());
        *n_windows_out = static_cast<int64_t>(cuts.size()) - 1;
    });
}

int scg_fastq_scan_windows(const char* path, int64_t window_bytes, int nthreads, char** seqs_out, uint64_t** offsets_out,
                           int64_t* n_reads_out, int64_t* n_windows_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path || !seqs_out || !offsets_out || !n_reads_out || !n_windows_out || window_bytes < 64) throw Error(SCG_ERR_INVALID, "null argument");
        std::unique_ptr<scg::TextSource> src = scg::TextSource::open(path, scg::default_host_threads(nthreads));
        if (!src->parses()) throw Error(SCG_ERR_UNSUPPORTED, std::string("no host-side record scan for ") + src->kind() + " input");
        const size_t cap = static_cast<size_t>(window_bytes), cap_offsets = cap / 4 + 64;
        std::vector<char> all, window(cap);
        std::vector<uint32_t> offs(cap_offsets);
        std::vector<uint64_t> offsets(1, 0);
        int64_t n_windows = 0;
        for (;;) {
            scg::ParsedWindow w;
            const size_t got = src->next_parsed(window.data(), cap, offs.data(), cap_offsets, w);
            if (src->unusual()) throw Error(SCG_ERR_UNSUPPORTED, "the text is not a run of ordinary 4-line records");
            if (!got) break;
            ++n_windows;
            for (int i = 0; i < w.n_segs; ++i) {
                const scg::ParsedSegment& g = w.seg[i];
                const uint64_t base = all.size();
                all.insert(all.end(), window.begin() + static_cast<long>(g.seq_at), window.begin() + static_cast<long>(g.seq_at + g.seq_bytes));
                for (uint32_t r = 0; r < g.n_records; ++r) offsets.push_back(base + offs[g.off_at + r + 1]);
            }
        }
        vectors_out(all, 1, offsets, 0, seqs_out, offsets_out);
        *n_reads_out = static_cast<int64_t>(offsets.size()) - 1;
        *n_windows_out = n_windows;
    });
}

int scg_bgzf_member_batches(const char* path, int64_t staging_bytes, int64_t text_bytes, int nthreads, uint32_t** table_out, int64_t* n_members_out,
                            char** payloads_out, int64_t* n_payload_bytes_out, int64_t* n_batches_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path || !table_out || !n_members_out || !payloads_out || !n_payload_bytes_out || !n_batches_out || staging_bytes < 64 || text_bytes < 1) {
            throw Error(SCG_ERR_INVALID, "null argument");
        }
        std::unique_ptr<scg::TextSource> src = scg::TextSource::open(path, scg::default_host_threads(nthreads));
        if (!src->has_members()) throw Error(SCG_ERR_UNSUPPORTED, std::string("no member batches for ") + src->kind() + " input");
        const size_t slack = scg::inflate_input_slack();
        std::vector<char> staging(static_cast<size_t>(staging_bytes) + slack), all;
        std::vector<uint32_t> table;
        std::vector<scg::CompressedMember> members;
        int64_t batches = 0;
        for (;;) {
            size_t text = 0;
            bool last = false;
            const size_t got = src->next_members(staging.data(), staging.size(), slack, static_cast<size_t>(text_bytes), members, text, last);
            if (src->unusual()) throw Error(SCG_ERR_UNSUPPORTED, "a member the device inflater does not take (not BGZF throughout, extra header fields, or larger than a batch)");
            if (!got) break;
            for (const scg::CompressedMember& m : members) {
                const uint32_t row[6] = {static_cast<uint32_t>(batches), static_cast<uint32_t>(all.size() + m.in_off), m.in_len, m.out_off, m.out_len, m.crc};
                table.insert(table.end(), row, row + 6);
            }
            all.insert(all.end(), staging.begin(), staging.begin() + static_cast<long>(got - slack));
            ++batches;
            if (last) break;
        }
        vectors_out(table, 1, all, 1, table_out, payloads_out);
        *n_members_out = static_cast<int64_t>(table.size() / 6);
        *n_payload_bytes_out = static_cast<int64_t>(all.size());
        *n_batches_out = batches;
    });
}

int scg_set_device(int device, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw Error(SCG_ERR_DEVICE, "no HIP device available: libscg has no CPU fallback");
        if (device < 0 || device >= n) {
            throw Error(SCG_ERR_DEVICE, "HIP device " + std::to_string(device) + " out of range (" + std::to_string(n) + " visible)");
        }
        HIP_CHECK(hipSetDevice(device));
    });
}

int scg_set_devices(const int* devices, int n, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (n < 0 || (n > 0 && !devices)) throw Error(SCG_ERR_INVALID, "null argument");
        set_thread_devices(devices, n);
    });
}

int scg_plan_single(scg_plan** plan_out, const char* constant, int strand, const char* const* pool, int32_t n_pool,
                    int mismatches, int use_first, int device, char* err, size_t errcap) {
    return new_plan(plan_out, device, err, errcap, [&] {
        return compile_single(constant, strand, pool, n_pool, mismatches, use_first);
    });
}

int scg_plan_single_paired(scg_plan** plan_out, const char* constant, int strand, const char* const* pool, int32_t n_pool,
                           int mismatches, int use_first, int device, char* err, size_t errcap) {
    return new_plan(plan_out, device, err, errcap, [&] {
        return compile_single_paired(constant, strand, pool, n_pool, mismatches, use_first);
    });
}

int scg_plan_combo(scg_plan** plan_out, const char* constant, int strand, const char* const* pool0, int32_t n_pool0,
                   const char* const* pool1, int32_t n_pool1, int mismatches, int use_first,
                   int device, char* err, size_t errcap) {
    return new_plan(plan_out, device, err, errcap, [&] {
        return compile_combo(constant, strand, pool0, n_pool0, pool1, n_pool1, mismatches, use_first);
    });
}

int scg_plan_combo_regions(scg_plan** plan_out, const char* constant, int strand, const char* const* const* pools, const int32_t* n_pools,
                           int32_t n_regions, int mismatches, int use_first, int device, char* err, size_t errcap) {
    return new_plan(plan_out, device, err, errcap, [&] {
        return compile_combo_regions(constant, strand, pools, n_pools, n_regions, mismatches, use_first);
    });
}

int scg_plan_dual(scg_plan** plan_out, const char* constant1, int reverse1, int mismatches1, const char* const* pool1,
                  const char* constant2, int reverse2, int mismatches2, const char* const* pool2,
                  int32_t n_pool, int randomized, int use_first, int diagnostics, int device, char* err, size_t errcap) {
    return new_plan(plan_out, device, err, errcap, [&] {
        return compile_dual(constant1, reverse1, mismatches1, pool1, constant2, reverse2, mismatches2, pool2, n_pool, randomized, use_first, diagnostics);
    });
}

int scg_plan_dual_single_end(scg_plan** plan_out, const char* constant, int strand, const char* const* const* pools, const int32_t* n_pools,
                             int32_t n_regions, int mismatches, int use_first, int device, char* err, size_t errcap) {
    return new_plan(plan_out, device, err, errcap, [&] {
        return compile_dual_single_end(constant, strand, pools, n_pools, n_regions, mismatches, use_first);
    });
}

int scg_plan_paired_combo(scg_plan** plan_out,
                          const char* constant1, int reverse1, int mismatches1, const char* const* pool1, int32_t n_pool1,
                          const char* constant2, int reverse2, int mismatches2, const char* const* pool2, int32_t n_pool2,
                          int randomized, int use_first, int device, char* err, size_t errcap) {
    return new_plan(plan_out, device, err, errcap, [&] {
        return compile_paired_combo(constant1, reverse1, mismatches1, pool1, n_pool1, constant2, reverse2, mismatches2, pool2, n_pool2,
                                    randomized, use_first);
    });
}

int scg_plan_random(scg_plan** plan_out, const char* constant, int strand, int mismatches, int use_first,
                    int device, char* err, size_t errcap) {
    return new_plan(plan_out, device, err, errcap, [&] {
        return compile_random(constant, strand, mismatches, use_first);
    }, random_to_device);
}

int scg_plan_read_random(scg_plan* plan, char** sequences_out, int32_t** freq_out, int64_t* k_out, int32_t* length_out, int64_t* total_out,
                         void* stream, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!plan || !sequences_out || !freq_out || !k_out || !length_out) throw Error(SCG_ERR_INVALID, "null argument");
        *sequences_out = nullptr; *freq_out = nullptr; *k_out = 0;
        if (plan->kind != scg_plan::RANDOM) throw Error(SCG_ERR_INVALID, "not a random-barcode plan");
        read_random(plan, static_cast<hipStream_t>(stream), sequences_out, freq_out, k_out, length_out);
        if (total_out) *total_out = plan->total;
    });
}

void scg_plan_destroy(scg_plan* plan) {
    if (!plan) return;
    int prev = -1;
    if (hipGetDevice(&prev) == hipSuccess && prev != plan->device) (void)hipSetDevice(plan->device); else prev = -1;
    delete plan;
    if (prev >= 0) (void)hipSetDevice(prev);
}

int64_t scg_plan_num_counters(const scg_plan* plan) { return plan ? plan->n_counters : 0; }

int32_t scg_plan_num_regions(const scg_plan* plan) {
    if (!plan) return 0;
    return plan->kind == scg_plan::COMBO_REGIONS ? plan->n_regions : plan->ht1.t.nreg;
}

int32_t* scg_plan_device_counters(scg_plan* plan) { return plan ? plan->counters : nullptr; }

int scg_plan_bind_counters(scg_plan* plan, int32_t* d_counters, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!plan) throw Error(SCG_ERR_INVALID, "null plan");
        if (plan->kind == scg_plan::RANDOM) throw Error(SCG_ERR_INVALID, "random-barcode plans keep no counters to bind");
        plan->counters = d_counters ? d_counters : plan->own_counters.as<int32_t>();
    });
}

int scg_plan_reset(scg_plan* plan, void* stream, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!plan) throw Error(SCG_ERR_INVALID, "null plan");
        DeviceGuard g(plan->device);
        if (plan->kind == scg_plan::RANDOM) {                 // (ordered after the plan's previous call, like its batches)
            random_reset(plan, static_cast<hipStream_t>(stream));
            plan->total = 0;
            return;
        }
        HIP_CHECK(hipMemsetAsync(plan->counters, 0, static_cast<size_t>(plan->n_counters) * sizeof(int32_t), static_cast<hipStream_t>(stream)));
        HIP_CHECK(hipMemsetAsync(plan->error_flag.p, 0, sizeof(int32_t), static_cast<hipStream_t>(stream)));
        drop_pending_pairs(plan);
        plan->sparse_counts.clear();
        plan->total = 0;
    });
}

int scg_count_batch(scg_plan* plan, const char* d_seqs, const uint32_t* d_offsets, int32_t fixed_len, int32_t max_len,
                    int64_t n_reads, void* stream, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!plan) throw Error(SCG_ERR_INVALID, "null plan");
        if (plan->kind == scg_plan::DUAL) throw Error(SCG_ERR_INVALID, "scg_count_batch called on a dual plan; use scg_count_batch_paired");
        if (plan->kind == scg_plan::SINGLE_PAIRED) throw Error(SCG_ERR_INVALID, "scg_count_batch called on a paired single-barcode plan; use scg_count_batch_paired");
        check_reads_args(d_seqs, d_offsets, fixed_len, n_reads);
        DeviceGuard g(plan->device);
        launch_batch(plan, make_reads(d_seqs, d_offsets, fixed_len, max_len), n_reads, static_cast<hipStream_t>(stream));
    });
}

int scg_count_batch_paired(scg_plan* plan, const char* d_seqs1, const uint32_t* d_offsets1, int32_t fixed_len1,
                           const char* d_seqs2, const uint32_t* d_offsets2, int32_t fixed_len2, int32_t max_len,
                           int64_t n_pairs, void* stream, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!plan) throw Error(SCG_ERR_INVALID, "null plan");
        if (plan->kind != scg_plan::DUAL && plan->kind != scg_plan::SINGLE_PAIRED) throw Error(SCG_ERR_INVALID, "scg_count_batch_paired needs a dual plan");
        check_reads_args(d_seqs1, d_offsets1, fixed_len1, n_pairs);
        check_reads_args(d_seqs2, d_offsets2, fixed_len2, n_pairs);
        DeviceGuard g(plan->device);
        launch_batch_paired(plan, make_reads(d_seqs1, d_offsets1, fixed_len1, max_len), make_reads(d_seqs2, d_offsets2, fixed_len2, max_len),
                            n_pairs, static_cast<hipStream_t>(stream));
    });
}

int scg_assign_batch(scg_plan* plan, const char* d_seqs, const uint32_t* d_offsets, int32_t fixed_len, int32_t max_len, int64_t n_reads,
                     int32_t* d_index_out, int32_t* d_position_out, int8_t* d_mismatches_out, int8_t* d_variable_mismatches_out,
                     int8_t* d_reverse_out, void* stream, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!plan) throw Error(SCG_ERR_INVALID, "null plan");
        if (n_reads > 0 && !d_index_out) throw Error(SCG_ERR_INVALID, "null argument");
        if (plan->kind != scg_plan::SINGLE || !plan->simple_match) {
            throw Error(SCG_ERR_INVALID, "scg_assign_batch needs a single-barcode plan (scg_plan_single)");
        }
        check_reads_args(d_seqs, d_offsets, fixed_len, n_reads);
        if (plan->max_mm1 > INT8_MAX) {
            throw Error(SCG_ERR_UNSUPPORTED, "scg_assign_batch reports mismatches as int8: a budget of " + std::to_string(plan->max_mm1) + " exceeds 127");
        }
        if (n_reads == 0) return;
        DeviceGuard g(plan->device);
        ScgAssignOut out;
        out.index = d_index_out; out.position = d_position_out; out.mismatches = d_mismatches_out;
        out.variable_mismatches = d_variable_mismatches_out; out.reverse = d_reverse_out;
        launch_batch_assign(plan, make_reads(d_seqs, d_offsets, fixed_len, max_len), n_reads, out, static_cast<hipStream_t>(stream));
    });
}

int scg_plan_read(scg_plan* plan, int32_t* counts_out, int64_t* total_out, void* stream, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!plan) throw Error(SCG_ERR_INVALID, "null plan");
        DeviceGuard g(plan->device);
        HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
        read_counters(plan, counts_out);
        if (total_out) *total_out = plan->total;
    });
}

int scg_plan_read_combinations(scg_plan* plan, int32_t** indices_out, int32_t** freq_out, int64_t* k_out, int64_t* total_out,
                               void* stream, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!plan || !indices_out || !freq_out || !k_out) throw Error(SCG_ERR_INVALID, "null argument");
        if (plan->kind != scg_plan::COMBO && plan->kind != scg_plan::COMBO_REGIONS) throw Error(SCG_ERR_INVALID, "not a combination plan");
        DeviceGuard g(plan->device);
        HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
        result_combinations(std::vector<scg_plan*>(1, plan), indices_out, freq_out, k_out, nullptr);
        if (total_out) *total_out = plan->total;
    });
}

int scg_combo_compact(const int32_t* cells, int32_t n_pool0, int32_t n_pool1,
                      int32_t** indices_out, int32_t** freq_out, int64_t* k_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!cells || !indices_out || !freq_out || !k_out) throw Error(SCG_ERR_INVALID, "null argument");
        combo_compact(cells, n_pool0, n_pool1, indices_out, freq_out, k_out);
    });
}

int scg_plan_set_profiling(scg_plan* plan, int enabled) {
    if (!plan) return SCG_ERR_INVALID;
    plan->profiling = enabled != 0;
    plan->events_used = 0;   // (re)starting a measurement window
    return SCG_OK;
}

int scg_plan_kernel_stats(scg_plan* plan, double* total_ms_out, int64_t* launches_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!plan) throw Error(SCG_ERR_INVALID, "null plan");
        DeviceGuard g(plan->device);
        double ms = 0;
        for (size_t i = 0; i < plan->events_used; ++i) {
            HIP_CHECK(hipEventSynchronize(plan->events[i].second));
            float t = 0;
            HIP_CHECK(hipEventElapsedTime(&t, plan->events[i].first, plan->events[i].second));
            ms += t;
        }
        if (total_ms_out) *total_ms_out = ms;
        if (launches_out) *launches_out = static_cast<int64_t>(plan->events_used);
    });
}

// ---- file-level entry points -------------------------------------------------------------------

int scg_count_single_barcodes(const char* path, const char* constant, int strand, const char* const* pool, int32_t n_pool,
                              int mismatches, int use_first, int nthreads, int32_t* counts_out, int32_t* total_out,
                              char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path || !counts_out || !total_out) throw Error(SCG_ERR_INVALID, "null argument");
        Trace tr;
        scg::FastqStream fq(path);                                           // src/count_single_barcodes.cpp:30
        tr.mark("open");
        auto set = compile_and_count_single_end(path, fq, nthreads, [&] {
            return compile_single(constant, strand, pool, n_pool, mismatches, use_first);   // :31-47
        });
        tr.mark("compile + count");
        result_counts(set->all(), counts_out, total_out);
        tr.mark("read counters");
        set.reset();
        tr.mark("release the plan");
    });
}

int scg_count_combo_barcodes_single(const char* path, const char* constant, int strand,
                                    const char* const* pool0, int32_t n_pool0, const char* const* pool1, int32_t n_pool1,
                                    int mismatches, int use_first, int nthreads,
                                    int32_t** indices_out, int32_t** freq_out, int64_t* k_out, int32_t* total_out,
                                    char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path || !indices_out || !freq_out || !k_out || !total_out) throw Error(SCG_ERR_INVALID, "null argument");
        scg::FastqStream fq(path);
        auto set = compile_and_count_single_end(path, fq, nthreads, [&] {
            return compile_combo(constant, strand, pool0, n_pool0, pool1, n_pool1, mismatches, use_first);
        });
        result_combinations(set->all(), indices_out, freq_out, k_out, total_out);
    });
}

int scg_count_combo_barcodes_regions(const char* path, const char* constant, int strand,
                                     const char* const* const* pools, const int32_t* n_pools, int32_t n_regions,
                                     int mismatches, int use_first, int nthreads,
                                     int32_t** indices_out, int32_t** freq_out, int64_t* k_out, int32_t* total_out,
                                     char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path || !indices_out || !freq_out || !k_out || !total_out) throw Error(SCG_ERR_INVALID, "null argument");
        scg::FastqStream fq(path);                                           // the reader first, as in the two-region entry
        auto set = compile_and_count_single_end(path, fq, nthreads, [&] {
            return compile_combo_regions(constant, strand, pools, n_pools, n_regions, mismatches, use_first);
        });
        result_combinations(set->all(), indices_out, freq_out, k_out, total_out);
    });
}

int scg_count_dual_barcodes(const char* path1, const char* constant1, int reverse1, int mismatches1, const char* const* pool1,
                            const char* path2, const char* constant2, int reverse2, int mismatches2, const char* const* pool2,
                            int32_t n_pool, int randomized, int use_first, int diagnostics, int nthreads,
                            int32_t* counts_out, int32_t* total_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path1 || !path2 || !counts_out || !total_out) throw Error(SCG_ERR_INVALID, "null argument");
        scg::FastqStream fq1(path1);                                         // src/count_dual_barcodes.cpp:93-97
        scg::FastqStream fq2(path2);
        if (diagnostics) {
            throw Error(SCG_ERR_INVALID, "diagnostics requested: call scg_count_dual_barcodes_diagnostics, which returns the extra outputs");
        }
        auto set = compile_and_count_paired(path1, path2, fq1, fq2, nthreads, [&] {
            return compile_dual(constant1, reverse1, mismatches1, pool1, constant2, reverse2, mismatches2, pool2, n_pool, randomized, use_first);
        });
        result_counts(set->all(), counts_out, total_out);
    });
}

// kaori::SingleBarcodePairedEnd over two files: both readers first, as scg_count_dual_barcodes.
int scg_count_single_barcodes_paired(const char* path1, const char* path2, const char* constant, int strand, const char* const* pool, int32_t n_pool,
                                     int mismatches, int use_first, int nthreads, int32_t* counts_out, int32_t* total_out,
                                     char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path1 || !path2 || !counts_out || !total_out) throw Error(SCG_ERR_INVALID, "null argument");
        scg::FastqStream fq1(path1);
        scg::FastqStream fq2(path2);
        auto set = compile_and_count_paired(path1, path2, fq1, fq2, nthreads, [&] {
            return compile_single_paired(constant, strand, pool, n_pool, mismatches, use_first);
        });
        result_counts(set->all(), counts_out, total_out);
    });
}

int scg_count_dual_barcodes_diagnostics(const char* path1, const char* constant1, int reverse1, int mismatches1, const char* const* pool1,
                                        const char* path2, const char* constant2, int reverse2, int mismatches2, const char* const* pool2,
                                        int32_t n_pool, int randomized, int use_first, int nthreads,
                                        int32_t* counts_out, int32_t** invalid_indices_out, int32_t** invalid_freq_out, int64_t* k_out,
                                        int32_t* total_out, int32_t* barcode1_only_out, int32_t* barcode2_only_out,
                                        char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path1 || !path2 || !counts_out || !invalid_indices_out || !invalid_freq_out || !k_out || !total_out ||
            !barcode1_only_out || !barcode2_only_out) {
            throw Error(SCG_ERR_INVALID, "null argument");
        }
        scg::FastqStream fq1(path1);
        scg::FastqStream fq2(path2);
        auto set = compile_and_count_paired(path1, path2, fq1, fq2, nthreads, [&] {
            return compile_dual(constant1, reverse1, mismatches1, pool1, constant2, reverse2, mismatches2, pool2, n_pool, randomized, use_first, 1);
        });
        result_diagnostics(set->all(), counts_out, invalid_indices_out, invalid_freq_out, k_out, total_out, barcode1_only_out, barcode2_only_out);
    });
}

int scg_count_dual_barcodes_single_end(const char* path, const char* constant, const char* const* const* pools, const int32_t* n_pools,
                                       int32_t n_regions, int strand, int mismatches, int use_first, int diagnostics, int nthreads,
                                       int32_t* counts_out, int32_t* total_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path || !total_out || (n_regions > 0 && n_pools && n_pools[0] > 0 && !counts_out)) throw Error(SCG_ERR_INVALID, "null argument");
        scg::FastqStream fq(path);                             // src/count_dual_barcodes_single_end.cpp:64: reader first
        auto set = compile_and_count_single_end(path, fq, nthreads, [&] {
            auto P = compile_dual_single_end(constant, strand, pools, n_pools, n_regions, mismatches, use_first);
            if (diagnostics) {
                throw Error(SCG_ERR_INVALID, "diagnostics requested: call scg_count_dual_barcodes_single_end_diagnostics, which returns the extra outputs");
            }
            return P;
        });
        result_counts(set->all(), counts_out, total_out);
    });
}

// countRandomBarcodes: the reader first (src/count_random_barcodes.cpp:42), then the template's checks and the host tally
// of count_random_file (scg_files.cpp).
int scg_count_random_barcodes(const char* path, const char* constant, int strand, int mismatches, int use_first, int nthreads,
                              char** sequences_out, int32_t** freq_out, int64_t* k_out, int32_t* length_out, int32_t* total_out,
                              char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path || !constant || !sequences_out || !freq_out || !k_out || !length_out || !total_out) throw Error(SCG_ERR_INVALID, "null argument");
        scg::FastqStream fq(path);
        count_random_file(path, fq, constant, strand, mismatches, use_first, nthreads, sequences_out, freq_out, k_out, length_out, total_out);
    });
}

int scg_count_dual_barcodes_single_end_diagnostics(const char* path, const char* constant, const char* const* const* pools, const int32_t* n_pools,
                                                   int32_t n_regions, int strand, int mismatches, int use_first, int nthreads,
                                                   int32_t* counts_out, int32_t** invalid_indices_out, int32_t** invalid_freq_out, int64_t* k_out,
                                                   int32_t* total_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path || !invalid_indices_out || !invalid_freq_out || !k_out || !total_out) throw Error(SCG_ERR_INVALID, "null argument");
        scg::FastqStream fq(path);
        auto set = compile_and_count_single_end(path, fq, nthreads, [&] {
            return compile_dual_single_end_diag(constant, strand, pools, n_pools, n_regions, mismatches, use_first);
        });
        result_diagnostics(set->all(), counts_out, invalid_indices_out, invalid_freq_out, k_out, total_out, nullptr, nullptr);
    });
}

int scg_count_combo_barcodes_paired(const char* path1, const char* constant1, int reverse1, int mismatches1,
                                    const char* const* pool1, int32_t n_pool1,
                                    const char* path2, const char* constant2, int reverse2, int mismatches2,
                                    const char* const* pool2, int32_t n_pool2,
                                    int randomized, int use_first, int nthreads,
                                    int32_t** indices_out, int32_t** freq_out, int64_t* k_out,
                                    int32_t* total_out, int32_t* barcode1_only_out, int32_t* barcode2_only_out,
                                    char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!path1 || !path2 || !indices_out || !freq_out || !k_out || !total_out || !barcode1_only_out || !barcode2_only_out) {
            throw Error(SCG_ERR_INVALID, "null argument");
        }
        scg::FastqStream fq1(path1);                           // src/count_combo_barcodes_paired.cpp:75-79: readers first
        scg::FastqStream fq2(path2);
        auto set = compile_and_count_paired(path1, path2, fq1, fq2, nthreads, [&] {
            return compile_paired_combo(constant1, reverse1, mismatches1, pool1, n_pool1, constant2, reverse2, mismatches2, pool2, n_pool2,
                                        randomized, use_first);
        });
        result_diagnostics(set->all(), nullptr, indices_out, freq_out, k_out, total_out, barcode1_only_out, barcode2_only_out);
    });
}

// ---- many files in one call (matrixOf*) ---------------------------------------------------------------------

int scg_count_single_barcodes_files(const char* const* paths, int32_t n_files, const char* constant, int strand,
                                    const char* const* pool, int32_t n_pool, int mismatches, int use_first, int nthreads,
                                    int32_t* counts_out, int32_t* totals_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (n_files < 0 || (n_files > 0 && (!paths || !totals_out || (n_pool > 0 && !counts_out)))) throw Error(SCG_ERR_INVALID, "null argument");
        if (n_files == 1) {      // one file: all devices share it (a null path is the one-file entry's "null argument" too)
            const int rc = scg_count_single_barcodes(paths[0], constant, strand, pool, n_pool, mismatches, use_first, nthreads,
                                                     counts_out, totals_out, err, errcap);
            if (rc != SCG_OK) throw Error(rc, err ? err : "");
            return;
        }
        count_files_into(FileLists{paths, nullptr, n_files}, nthreads, Order::FILE0_FIRST, [&] {
            return compile_single(constant, strand, pool, n_pool, mismatches, use_first);
        }, ReadOut::COUNTS, PerFile{counts_out, nullptr, nullptr, nullptr, totals_out, nullptr, nullptr});
    });
}

int scg_count_combo_barcodes_single_files(const char* const* paths, int32_t n_files, const char* constant, int strand,
                                          const char* const* pool0, int32_t n_pool0, const char* const* pool1, int32_t n_pool1,
                                          int mismatches, int use_first, int nthreads,
                                          int32_t** indices_out, int32_t** freq_out, int64_t* k_out, int32_t* totals_out,
                                          char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (n_files < 0 || (n_files > 0 && (!paths || !indices_out || !freq_out || !k_out || !totals_out))) throw Error(SCG_ERR_INVALID, "null argument");
        count_files_into(FileLists{paths, nullptr, n_files}, nthreads, Order::FILE0_FIRST, [&] {
            return compile_combo(constant, strand, pool0, n_pool0, pool1, n_pool1, mismatches, use_first);
        }, ReadOut::COMBINATIONS, PerFile{nullptr, indices_out, freq_out, k_out, totals_out, nullptr, nullptr});
    });
}

int scg_count_combo_barcodes_regions_files(const char* const* paths, int32_t n_files, const char* constant, int strand,
                                           const char* const* const* pools, const int32_t* n_pools, int32_t n_regions,
                                           int mismatches, int use_first, int nthreads,
                                           int32_t** indices_out, int32_t** freq_out, int64_t* k_out, int32_t* totals_out,
                                           char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (n_files < 0 || (n_files > 0 && (!paths || !indices_out || !freq_out || !k_out || !totals_out))) throw Error(SCG_ERR_INVALID, "null argument");
        count_files_into(FileLists{paths, nullptr, n_files}, nthreads, Order::FILE0_THEN_ARGUMENTS, [&] {
            return compile_combo_regions(constant, strand, pools, n_pools, n_regions, mismatches, use_first);
        }, ReadOut::COMBINATIONS, PerFile{nullptr, indices_out, freq_out, k_out, totals_out, nullptr, nullptr});
    });
}

int scg_count_dual_barcodes_files(const char* const* paths1, const char* constant1, int reverse1, int mismatches1, const char* const* pool1,
                                  const char* const* paths2, const char* constant2, int reverse2, int mismatches2, const char* const* pool2,
                                  int32_t n_pool, int32_t n_files, int randomized, int use_first, int nthreads,
                                  int32_t* counts_out, int32_t* totals_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (n_files < 0 || (n_files > 0 && (!paths1 || !paths2 || !totals_out || (n_pool > 0 && !counts_out)))) throw Error(SCG_ERR_INVALID, "null argument");
        count_files_into(FileLists{paths1, paths2, n_files}, nthreads, Order::FILE0_FIRST, [&] {
            return compile_dual(constant1, reverse1, mismatches1, pool1, constant2, reverse2, mismatches2, pool2, n_pool, randomized, use_first);
        }, ReadOut::COUNTS, PerFile{counts_out, nullptr, nullptr, nullptr, totals_out, nullptr, nullptr});
    });
}

// The five entries below check their arguments -- the template and the pools are compiled, host work only -- before any
// file is opened and any device is touched (Order::ARGUMENTS_FIRST); then every device gets its plan and takes the files
// one at a time.  In all eight many-files entries with a library a plan starts every file from reset_plan (counters,
// sparse combinations, runs in flight, the oversize-read flag), and a file's outputs are read by the function its
// one-file entry reads them with (read_file_into: result_counts, result_combinations, result_diagnostics).

int scg_count_dual_barcodes_diagnostics_files(const char* const* paths1, const char* constant1, int reverse1, int mismatches1, const char* const* pool1,
                                              const char* const* paths2, const char* constant2, int reverse2, int mismatches2, const char* const* pool2,
                                              int32_t n_pool, int32_t n_files, int randomized, int use_first, int nthreads,
                                              int32_t* counts_out, int32_t** invalid_indices_out, int32_t** invalid_freq_out, int64_t* k_out,
                                              int32_t* totals_out, int32_t* barcode1_only_out, int32_t* barcode2_only_out,
                                              char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (n_files < 0 || (n_files > 0 && (!paths1 || !paths2 || !invalid_indices_out || !invalid_freq_out || !k_out || !totals_out ||
                                            !barcode1_only_out || !barcode2_only_out || (n_pool > 0 && !counts_out)))) {
            throw Error(SCG_ERR_INVALID, "null argument");
        }
        count_files_into(FileLists{paths1, paths2, n_files}, nthreads, Order::ARGUMENTS_FIRST, [&] {
            return compile_dual(constant1, reverse1, mismatches1, pool1, constant2, reverse2, mismatches2, pool2, n_pool, randomized, use_first, 1);
        }, ReadOut::DIAGNOSTICS, PerFile{counts_out, invalid_indices_out, invalid_freq_out, k_out, totals_out, barcode1_only_out, barcode2_only_out});
    });
}

int scg_count_single_barcodes_paired_files(const char* const* paths1, const char* const* paths2, int32_t n_files, const char* constant, int strand,
                                           const char* const* pool, int32_t n_pool, int mismatches, int use_first, int nthreads,
                                           int32_t* counts_out, int32_t* totals_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (n_files < 0 || (n_files > 0 && (!paths1 || !paths2 || !totals_out || (n_pool > 0 && !counts_out)))) throw Error(SCG_ERR_INVALID, "null argument");
        count_files_into(FileLists{paths1, paths2, n_files}, nthreads, Order::ARGUMENTS_FIRST, [&] {
            return compile_single_paired(constant, strand, pool, n_pool, mismatches, use_first);
        }, ReadOut::COUNTS, PerFile{counts_out, nullptr, nullptr, nullptr, totals_out, nullptr, nullptr});
    });
}

int scg_count_dual_barcodes_single_end_files(const char* const* paths, int32_t n_files, const char* constant,
                                             const char* const* const* pools, const int32_t* n_pools, int32_t n_regions,
                                             int strand, int mismatches, int use_first, int nthreads,
                                             int32_t* counts_out, int32_t* totals_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (n_files < 0 || (n_files > 0 && (!paths || !totals_out || (n_regions > 0 && n_pools && n_pools[0] > 0 && !counts_out)))) {
            throw Error(SCG_ERR_INVALID, "null argument");
        }
        count_files_into(FileLists{paths, nullptr, n_files}, nthreads, Order::ARGUMENTS_FIRST, [&] {
            return compile_dual_single_end(constant, strand, pools, n_pools, n_regions, mismatches, use_first);
        }, ReadOut::COUNTS, PerFile{counts_out, nullptr, nullptr, nullptr, totals_out, nullptr, nullptr});
    });
}

int scg_count_dual_barcodes_single_end_diagnostics_files(const char* const* paths, int32_t n_files, const char* constant,
                                                         const char* const* const* pools, const int32_t* n_pools, int32_t n_regions,
                                                         int strand, int mismatches, int use_first, int nthreads,
                                                         int32_t* counts_out, int32_t** invalid_indices_out, int32_t** invalid_freq_out, int64_t* k_out,
                                                         int32_t* totals_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (n_files < 0 || (n_files > 0 && (!paths || !invalid_indices_out || !invalid_freq_out || !k_out || !totals_out ||
                                            (n_regions > 0 && n_pools && n_pools[0] > 0 && !counts_out)))) {
            throw Error(SCG_ERR_INVALID, "null argument");
        }
        count_files_into(FileLists{paths, nullptr, n_files}, nthreads, Order::ARGUMENTS_FIRST, [&] {
            return compile_dual_single_end_diag(constant, strand, pools, n_pools, n_regions, mismatches, use_first);
        }, ReadOut::DIAGNOSTICS, PerFile{counts_out, invalid_indices_out, invalid_freq_out, k_out, totals_out, nullptr, nullptr});
    });
}

int scg_count_combo_barcodes_paired_files(const char* const* paths1, const char* constant1, int reverse1, int mismatches1,
                                          const char* const* pool1, int32_t n_pool1,
                                          const char* const* paths2, const char* constant2, int reverse2, int mismatches2,
                                          const char* const* pool2, int32_t n_pool2, int32_t n_files,
                                          int randomized, int use_first, int nthreads,
                                          int32_t** indices_out, int32_t** freq_out, int64_t* k_out,
                                          int32_t* totals_out, int32_t* barcode1_only_out, int32_t* barcode2_only_out,
                                          char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (n_files < 0 || (n_files > 0 && (!paths1 || !paths2 || !indices_out || !freq_out || !k_out || !totals_out ||
                                            !barcode1_only_out || !barcode2_only_out))) {
            throw Error(SCG_ERR_INVALID, "null argument");
        }
        count_files_into(FileLists{paths1, paths2, n_files}, nthreads, Order::ARGUMENTS_FIRST, [&] {
            return compile_paired_combo(constant1, reverse1, mismatches1, pool1, n_pool1, constant2, reverse2, mismatches2, pool2, n_pool2,
                                        randomized, use_first);
        }, ReadOut::DIAGNOSTICS, PerFile{nullptr, indices_out, freq_out, k_out, totals_out, barcode1_only_out, barcode2_only_out});
    });
}

// matrixOfRandomBarcodes.  Every device keeps ONE random-barcode table (files mode) for all the files it
// takes: a file starts from the soft reset of reset_plan, runs the ladder of every other single-end entry, and leaves as
// (row id, count) pairs (random_harvest, which makes the checks of the plan read-out first); the keys leave each device
// once, when all files are done.  Nothing is handed out before the whole matrix stands.
int scg_count_random_barcodes_files(const char* const* paths, int32_t n_files, const char* constant, int strand, int mismatches, int use_first,
                                    int nthreads, char** sequences_out, int64_t* k_out, int32_t* length_out, int64_t** col_ptr_out,
                                    int32_t** rows_out, int32_t** freq_out, int32_t* totals_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (n_files < 0 || !constant || !sequences_out || !k_out || !length_out || !col_ptr_out || !rows_out || !freq_out ||
            (n_files > 0 && (!paths || !totals_out))) {
            throw Error(SCG_ERR_INVALID, "null argument");
        }
        *sequences_out = nullptr; *col_ptr_out = nullptr; *rows_out = nullptr; *freq_out = nullptr; *k_out = 0; *length_out = 0;
        if (n_files == 0) {                                            // an empty matrix, with arrays to release like any other
            OutPair<char, int64_t> head(1, 1);
            OutPair<int32_t, int32_t> body(1, 1);
            head.a[0] = 0; head.b[0] = 0;
            head.release(sequences_out, col_ptr_out);
            body.release(rows_out, freq_out);
            return;
        }
        std::vector<scg_plan*> counted_by(static_cast<size_t>(n_files), nullptr);
        std::vector<std::vector<int32_t> > pairs(static_cast<size_t>(n_files));
        const std::unique_ptr<PlanSet> set = count_files(FileLists{paths, nullptr, n_files}, nthreads, Order::FILE0_THEN_ARGUMENTS, [&] {
            std::unique_ptr<scg_plan> compiled = compile_random(constant, strand, mismatches, use_first);
            compiled->rnd->files = true;
            return compiled;
        }, [&](scg_plan* P, int32_t f) {
            random_harvest(P, pairs[static_cast<size_t>(f)]);
            totals_out[f] = narrow_total(P->total);
            counted_by[static_cast<size_t>(f)] = P;
        });
        std::vector<int> plan_of(static_cast<size_t>(n_files), 0);
        for (size_t f = 0; f < plan_of.size(); ++f) {
            for (size_t p = 0; p < set->plans.size(); ++p) if (set->plans[p].get() == counted_by[f]) plan_of[f] = static_cast<int>(p);
        }
        result_random_matrix(*set, plan_of, pairs, sequences_out, k_out, length_out, col_ptr_out, rows_out, freq_out);
    });
}

// ---- combination counts of many files as one matrix (matrixOfComboBarcodes, matrixOfPairedComboBarcodes) ----------------
// The three entries below hand out what combineComboCounts builds (R/combineComboCounts.R:31-57) in the shape of
// scg_count_random_barcodes_files: the union of the files' combinations as rows, one compressed column per file.  The
// files are counted as in the *_files entries; a file leaves its device as sorted (key, count) pairs -- a dense histogram
// is compacted where it was counted (scg_combine.hip) -- and the union runs on the first device when all files are done.

int scg_combine_combinations(const int32_t* const* indices, const int32_t* const* freq, const int64_t* k, int32_t n_files,
                             int32_t** indices_out, int64_t* k_out, int64_t** col_ptr_out, int32_t** rows_out, int32_t** freq_out,
                             char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!indices_out || !k_out || !col_ptr_out || !rows_out || !freq_out) throw Error(SCG_ERR_INVALID, "null argument");
        *indices_out = nullptr; *col_ptr_out = nullptr; *rows_out = nullptr; *freq_out = nullptr; *k_out = 0;
        if (n_files < 0 || (n_files > 0 && (!indices || !freq || !k))) throw Error(SCG_ERR_INVALID, "null argument");
        std::vector<ComboList> lists(static_cast<size_t>(n_files));
        for (int32_t f = 0; f < n_files; ++f) {
            if (k[f] < 0) throw Error(SCG_ERR_INVALID, "negative number of combinations");
            if (k[f] > 0 && (!indices[f] || !freq[f])) throw Error(SCG_ERR_INVALID, "null argument");
            combo_list_of_outputs(indices[f], freq[f], k[f], lists[static_cast<size_t>(f)]);
        }
        if (n_files == 0) {                                            // an empty matrix, with arrays to release like any other
            empty_combo_matrix(0, indices_out, k_out, col_ptr_out, rows_out, freq_out);
            return;
        }
        combine_lists(lists, false, device_list()[0], indices_out, k_out, col_ptr_out, rows_out, freq_out);
    });
}

int scg_count_combo_barcodes_single_matrix(const char* const* paths, int32_t n_files, const char* constant, int strand,
                                           const char* const* pool0, int32_t n_pool0, const char* const* pool1, int32_t n_pool1,
                                           int mismatches, int use_first, int nthreads,
                                           int32_t** indices_out, int64_t* k_out, int64_t** col_ptr_out, int32_t** rows_out, int32_t** freq_out,
                                           int32_t* totals_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!indices_out || !k_out || !col_ptr_out || !rows_out || !freq_out) throw Error(SCG_ERR_INVALID, "null argument");
        *indices_out = nullptr; *col_ptr_out = nullptr; *rows_out = nullptr; *freq_out = nullptr; *k_out = 0;
        if (n_files < 0 || (n_files > 0 && (!paths || !totals_out))) throw Error(SCG_ERR_INVALID, "null argument");
        std::vector<ComboList> lists(static_cast<size_t>(n_files));
        std::vector<int32_t> totals(static_cast<size_t>(n_files), 0);
        const std::unique_ptr<PlanSet> set = count_files(FileLists{paths, nullptr, n_files}, nthreads, Order::FILE0_THEN_ARGUMENTS, [&] {
            return compile_combo(constant, strand, pool0, n_pool0, pool1, n_pool1, mismatches, use_first);
        }, [&](scg_plan* P, int32_t f) {
            totals[static_cast<size_t>(f)] = narrow_total(P->total);
            combo_list_of_plan(P, lists[static_cast<size_t>(f)]);
        });
        if (n_files == 0) {
            empty_combo_matrix(0, indices_out, k_out, col_ptr_out, rows_out, freq_out);
            return;
        }
        combine_lists(lists, true, set->first()->device, indices_out, k_out, col_ptr_out, rows_out, freq_out);
        std::copy(totals.begin(), totals.end(), totals_out);
    });
}

int scg_count_combo_barcodes_paired_matrix(const char* const* paths1, const char* constant1, int reverse1, int mismatches1,
                                           const char* const* pool1, int32_t n_pool1,
                                           const char* const* paths2, const char* constant2, int reverse2, int mismatches2,
                                           const char* const* pool2, int32_t n_pool2, int32_t n_files,
                                           int randomized, int use_first, int nthreads,
                                           int32_t** indices_out, int64_t* k_out, int64_t** col_ptr_out, int32_t** rows_out, int32_t** freq_out,
                                           int32_t* totals_out, int32_t* barcode1_only_out, int32_t* barcode2_only_out,
                                           char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!indices_out || !k_out || !col_ptr_out || !rows_out || !freq_out) throw Error(SCG_ERR_INVALID, "null argument");
        *indices_out = nullptr; *col_ptr_out = nullptr; *rows_out = nullptr; *freq_out = nullptr; *k_out = 0;
        if (n_files < 0 || (n_files > 0 && (!paths1 || !paths2 || !totals_out || !barcode1_only_out || !barcode2_only_out))) {
            throw Error(SCG_ERR_INVALID, "null argument");
        }
        const size_t n = static_cast<size_t>(n_files);
        std::vector<ComboList> lists(n);
        std::vector<int32_t> totals(n, 0), b1(n, 0), b2(n, 0);
        const std::unique_ptr<PlanSet> set = count_files(FileLists{paths1, paths2, n_files}, nthreads, Order::ARGUMENTS_FIRST, [&] {
            return compile_paired_combo(constant1, reverse1, mismatches1, pool1, n_pool1, constant2, reverse2, mismatches2, pool2, n_pool2,
                                        randomized, use_first);
        }, [&](scg_plan* P, int32_t f) {
            // the file's list by the read-out of the paired entries (sequence uids to pool indices on the host)
            int32_t* idx = nullptr;
            int32_t* fr = nullptr;
            int64_t kf = 0;
            result_diagnostics(std::vector<scg_plan*>(1, P), nullptr, &idx, &fr, &kf, &totals[static_cast<size_t>(f)], &b1[static_cast<size_t>(f)],
                               &b2[static_cast<size_t>(f)]);
            const std::unique_ptr<int32_t, void (*)(void*)> keep_idx(idx, std::free), keep_fr(fr, std::free);
            combo_list_of_outputs(idx, fr, kf, lists[static_cast<size_t>(f)]);
        });
        if (n_files == 0) {
            empty_combo_matrix(0, indices_out, k_out, col_ptr_out, rows_out, freq_out);
            return;
        }
        combine_lists(lists, true, set->first()->device, indices_out, k_out, col_ptr_out, rows_out, freq_out);
        std::copy(totals.begin(), totals.end(), totals_out);
        std::copy(b1.begin(), b1.end(), barcode1_only_out);
        std::copy(b2.begin(), b2.end(), barcode2_only_out);
    });
}

int scg_combo_compact_device(const int32_t* cells, int32_t n_pool0, int32_t n_pool1,
                             int32_t** indices_out, int32_t** freq_out, int64_t* k_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!cells || !indices_out || !freq_out || !k_out) throw Error(SCG_ERR_INVALID, "null argument");
        *indices_out = nullptr; *freq_out = nullptr; *k_out = 0;
        const int device = resolve_device(-1);
        DeviceGuard g(device);
        const uint64_t n_cells = n_pool0 > 0 && n_pool1 > 0 ? static_cast<uint64_t>(n_pool0) * static_cast<uint64_t>(n_pool1) : 0;
        ComboList list;
        if (n_cells) {
            DevBuf d_cells;
            try {
                d_cells.alloc(n_cells * sizeof(int32_t));
            } catch (const Error& e) {
                throw Error(SCG_ERR_DEVICE, "cannot allocate " + std::to_string(n_cells) + " cells on the device: " + e.what());
            }
            HIP_CHECK(hipMemcpy(d_cells.p, cells, n_cells * sizeof(int32_t), hipMemcpyHostToDevice));
            compact_cells_on_device(d_cells.as<int32_t>(), n_pool0, n_pool1, list);
        }
        const size_t K = list.keys.size();
        OutPair<int32_t, int32_t> out(2 * K + 1, K + 1);
        for (size_t j = 0; j < K; ++j) {
            out.a[2 * j] = static_cast<int32_t>(list.keys[j] >> 32);
            out.a[2 * j + 1] = static_cast<int32_t>(list.keys[j] & 0xFFFFFFFFu);
            out.b[j] = list.counts[j];
        }
        out.release(indices_out, freq_out);
        *k_out = static_cast<int64_t>(K);
    });
}

int scg_plan_read_diagnostics(scg_plan* plan, int32_t* counts_out, int32_t** invalid_indices_out, int32_t** invalid_freq_out,
                              int64_t* k_out, int64_t* total_out, int32_t* barcode1_only_out, int32_t* barcode2_only_out,
                              void* stream, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!plan || !invalid_indices_out || !invalid_freq_out || !k_out || !barcode1_only_out || !barcode2_only_out) {
            throw Error(SCG_ERR_INVALID, "null argument");
        }
        if (plan->kind != scg_plan::DUAL || !plan->diagnostics) throw Error(SCG_ERR_INVALID, "not a dual plan with diagnostics");
        DeviceGuard g(plan->device);
        HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
        std::vector<int32_t> all(static_cast<size_t>(plan->n_counters) + 1);
        read_counters(plan, all.data());
        if (plan->sparse) retire_all_pairs(plan);
        diagnostics_from_counters(plan, all, counts_out, invalid_indices_out, invalid_freq_out, k_out, barcode1_only_out, barcode2_only_out,
                                  plan->sparse ? &plan->sparse_counts : nullptr);
        if (total_out) *total_out = plan->total;
    });
}

int scg_match_barcodes(const char* const* sequences, int32_t n_sequences, const char* const* choices, int32_t n_choices,
                       int substitutions, int reverse, int32_t* index_out, int32_t* mismatches_out, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if ((n_sequences > 0 && (!sequences || !index_out || !mismatches_out)) || (n_choices > 0 && !choices)) {
            throw Error(SCG_ERR_INVALID, "null argument");
        }
        int clen = scg::pool_length(choices, n_choices);                     // src/match_barcodes.cpp:12
        scg::HostIndex ht = scg::build_index(choices, n_choices, clen, substitutions < 0 ? 0 : substitutions, scg::key_class(clen));   // :13
        int slen = scg::pool_length(sequences, n_sequences);                 // :20
        if (n_sequences > 0 && slen != clen) {
            throw Error(SCG_ERR_INVALID, "sequences should have the same length as the choices (" + std::to_string(clen) + ")");
        }
        if (substitutions < 0) throw Error(SCG_ERR_INVALID, "negative number of mismatches");
        if (n_sequences == 0) return;
        int device = resolve_device(-1);
        DeviceGuard g(device);
        DevIndex tab;
        tab.upload(ht);
        std::vector<uint8_t> flat(static_cast<size_t>(n_sequences) * clen);
        for (int32_t i = 0; i < n_sequences; ++i) std::memcpy(flat.data() + static_cast<size_t>(i) * clen, sequences[i], clen);
        DevBuf d_seqs, d_idx, d_mm;
        d_seqs.upload(flat);
        d_idx.alloc(sizeof(int32_t) * n_sequences);
        d_mm.alloc(sizeof(int32_t) * n_sequences);
        HIP_CHECK(scg::launch_match(tab.view, d_seqs.as<uint8_t>(), n_sequences, substitutions, reverse, d_idx.as<int32_t>(), d_mm.as<int32_t>(), nullptr));
        HIP_CHECK(hipMemcpy(index_out, d_idx.p, sizeof(int32_t) * n_sequences, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(mismatches_out, d_mm.p, sizeof(int32_t) * n_sequences, hipMemcpyDeviceToHost));
    });
}

int scg_synth_reads(const scg_synth_spec* spec, char* d_seqs_out, int64_t n_reads, void* stream, char* err, size_t errcap) {
    return guarded(err, errcap, [&] {
        if (!spec || (!d_seqs_out && n_reads > 0)) throw Error(SCG_ERR_INVALID, "null argument");
        if (spec->read_len <= 0 || spec->template_len < 0 || spec->n_regions < 0 || spec->n_regions > 2) {
            throw Error(SCG_ERR_INVALID, "bad synthetic read specification");
        }
        HIP_CHECK(scg::launch_synth(*spec, d_seqs_out, n_reads, static_cast<hipStream_t>(stream)));
    });
}

} // extern "C"
#pragma GCC visibility pop
