// scg_files.cpp -- FASTQ files to counts: the host readers (staging of parsed batches) and the host tally of
// countRandomBarcodes over them, the fall-back ladders that decide which reader takes a file, and the file entries
// scg_api.cpp calls.  The windowed pipelines are in scg_windows.hpp.
#include "scg_windows.hpp"

namespace scgapi {

// FASTQ file -> counters for single-end plans.  Plain 4-line FASTQ is parsed by several host
// threads (ParallelFastq); gzip input, and any file the parallel reader finds unusual, goes
// through the sequential reader, which reproduces the reference's parse and errors exactly.
void count_single_end_file(scg_plan* P, const char* path, scg::FastqStream& fq, int nthreads,
                           const std::function<void(Stager::Slot&, const ScgReads&, int64_t)>& launch,
                           const std::function<void(Stager::Slot&)>& retire,
                           const std::function<void()>& restart) {
    Stager st;
    st.retire = retire;
    auto run = [&](Stager::Slot& s, const ScgReads& R, int64_t n) {
        s.n_reads = n;
        if (launch) launch(s, R, n); else launch_batch(P, R, n, s.stream);
    };
    const int threads = scg::default_host_threads(nthreads);
    if (threads > 1 && scg::ParallelFastq::is_plain_file(path)) {
        scg::ParallelFastq pf(path, threads);
        // window k + 1 is parsed by the workers while window k is copied to the device and counted
        std::vector<scg::ReadBatch> window, ahead;
        bool have = pf.next_window(window);
        while (have) {
            bool have_next = false;
            std::thread prefetch([&] { have_next = pf.next_window(ahead); });
            try {
                for (auto& b : window) {
                    if (b.size() == 0) continue;
                    auto& s = st.acquire();
                    ScgReads R = st.stage(s, 0, b);
                    run(s, R, b.size());
                    s.busy = true;
                }
            } catch (...) {
                prefetch.join();
                throw;
            }
            prefetch.join();
            window.swap(ahead);
            have = have_next;
        }
        st.drain();
        if (!pf.unusual()) return;
        // start over with the reference-exact sequential reader; what the windows counted goes, sparse combinations included
        reset_plan(P);
        if (restart) restart();
    }
    scg::ReadBatch b;
    while (fq.next_batch(b, BATCH_READS, BATCH_BYTES)) {
        auto& s = st.acquire();
        ScgReads R = st.stage(s, 0, b);
        run(s, R, b.size());
        s.busy = true;
    }
    st.drain();
}

// countRandomBarcodes on one file (src/count_random_barcodes.cpp:41-62, kaori::RandomBarcodeSingleEnd): the device
// locates the template in every read (same scan kernels, no library), the host cuts the variable region
// out of its copy of the batch and tallies the strings.  Reproduced quirks of the reference:
//  * the forward-strand string is the raw read bytes (case preserved);
//  * on the reverse strand the region is taken at the FORWARD template's offset inside the window
//    (RandomBarcodeSingleEnd.hpp:103-105 reads variable_regions()[0], not the reverse regions) and then
//    reverse-complemented with complement_base<true>: ACGTN in either case -> upper case, anything
//    else is the error "cannot complement unknown base".
// Output order: byte-wise ascending (the reference iterates an unordered_map; its R caller sorts).
void count_random_file(const char* path, scg::FastqStream& fq, const char* constant, int strand, int mismatches, int use_first, int nthreads,
                       char** sequences_out, int32_t** freq_out, int64_t* k_out, int32_t* length_out, int32_t* total_out) {
    std::unique_ptr<scg_plan> P = compile_random_template(constant, strand, mismatches, use_first);
    const ScgTemplate& t = P->ht1.t;
    P->to_device(-1);
    DeviceGuard g(P->device);
    const int vstart = t.fstart[0], vlen = t.flen[0];      // forward coordinates on both strands (see above)
    std::unordered_map<std::string, int32_t> tally;
    std::string key(static_cast<size_t>(vlen), ' ');
    const ScgSingleParams sp = single_params(P.get(), ScgIndex());
    auto launch = [&](Stager::Slot& s, const ScgReads& R, int64_t n) {
        s.d_aux.ensure(static_cast<size_t>(n) * sizeof(int32_t));
        s.h_aux.ensure(static_cast<size_t>(n) * sizeof(int32_t));
        HIP_CHECK(scg::launch_random(sp, t.len, R, n, s.d_aux.as<int32_t>(), P->error_flag.as<int32_t>(), s.stream));
        HIP_CHECK(hipMemcpyAsync(s.h_aux.p, s.d_aux.p, static_cast<size_t>(n) * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
        P->total += n;
    };
    auto retire = [&](Stager::Slot& s) {
        const int32_t* hits = s.h_aux.as<int32_t>();
        const char* seqs = s.h_seqs[0].as<char>();
        const uint32_t* offs = s.h_offs[0].as<uint32_t>();
        for (int64_t i = 0; i < s.n_reads; ++i) {
            const int32_t h = hits[i];
            if (h < 0) continue;
            const char* start = seqs + offs[i] + (h >> 1) + vstart;
            if (!(h & 1)) {
                key.assign(start, static_cast<size_t>(vlen));
            } else {
                for (int j = 0; j < vlen; ++j) {
                    char b = start[vlen - j - 1], o;
                    switch (b) {                            // kaori/utils.hpp:41-120, complement_base<true>
                        case 'A': case 'a': o = 'T'; break;
                        case 'C': case 'c': o = 'G'; break;
                        case 'G': case 'g': o = 'C'; break;
                        case 'T': case 't': o = 'A'; break;
                        case 'N': case 'n': o = 'N'; break;
                        default: throw Error(SCG_ERR_INVALID, std::string("cannot complement unknown base '") + b + "'");
                    }
                    key[static_cast<size_t>(j)] = o;
                }
            }
            ++tally[key];
        }
    };
    auto restart = [&] { tally.clear(); };
    count_single_end_file(P.get(), path, fq, nthreads, launch, retire, restart);
    read_counters(P.get(), nullptr);                       // surfaces the oversize-read flag
    std::vector<std::pair<std::string, int32_t> > rows(tally.begin(), tally.end());
    std::sort(rows.begin(), rows.end());
    const size_t stride = static_cast<size_t>(vlen) + 1;
    OutPair<char, int32_t> out(rows.size() * stride + 1, rows.size() + 1);
    for (size_t i = 0; i < rows.size(); ++i) {
        std::memcpy(out.a + i * stride, rows[i].first.data(), static_cast<size_t>(vlen));
        out.a[i * stride + vlen] = 0;
        out.b[i] = rows[i].second;
    }
    const int32_t total = narrow_total(P->total);
    out.release(sequences_out, freq_out);
    *k_out = static_cast<int64_t>(rows.size()); *length_out = vlen; *total_out = total;
}

// -------------------------------------------------------------------------------------------------
// The fall-back ladders: which reader takes a file, and what runs next when that reader declines it.
// One rule throughout: a decline (UnusualInput) at any point, in the first window or a later one, tears the pipeline
// down -- so its kernels have finished --, resets every plan through reset_plan and moves to the next rung that applies.
// Every rung is oracle-exact, so the order decides speed only.  The one-file entries begin() the first rung before the
// plans exist, while the template and the library are compiled on another thread; the many-files entries call finish()
// alone.
// -------------------------------------------------------------------------------------------------
// A gzip file the parallel decoder (scg_pgzip.h) handed back gets a second try with one inflate stream before the
// host readers take it.
bool is_parallel_gzip(const scg::TextSource* s) { return s && std::strcmp(s->kind(), "gzip-parallel") == 0; }

// What the two ladders share: the rung they stand on, and what a decline does to the plans.
struct Ladder {
    int rung = 0;
    bool traced;
    std::vector<int> devices;     // of the call; cut down to those the rung in use works on
    int threads = 1;              // of the host-side sources
    Ladder() : traced(Trace().on) {}
    void entered(const char* name) const { if (traced) std::fprintf(stderr, "[scg] rung %s\n", name); }
    // An ordinary gzip file of some size is decoded by the device when it is of the plain kind (one member, or several
    // large ones), its text left in HBM.  Null when the file is not of that kind, or the device's decoder hands it back
    // before anything was enqueued: the host threads' decoders take it.
    std::unique_ptr<scg::TextSource> device_gunzip(const char* path) const {
        if (!scg::TextSource::ordinary_gzip(path, threads)) return nullptr;
        std::unique_ptr<scg::TextSource> s = scg::TextSource::open_on_device(path, devices[0], threads);
        if (!s && traced) std::fprintf(stderr, "[scg] rung device-gunzip: declined -> host-threads\n");
        if (!s && scg::env().gunzip_strict) throw Error(SCG_ERR_UNSUPPORTED, "the device gzip decoder handed the file back (SCG_DEVICE_GUNZIP=2 forbids the fall-back)");
        return s;
    }
    // `plans`: null while they do not exist yet
    void declined(const char* name, const char* next, bool strict, const std::vector<scg_plan*>* plans) const {
        if (traced) std::fprintf(stderr, "[scg] rung %s: declined -> %s\n", name, next);
        if (strict) throw Error(SCG_ERR_UNSUPPORTED, "the device inflater handed the file back (SCG_DEVICE_INFLATE=2 forbids the fall-back)");
        if (plans) for (scg_plan* P : *plans) reset_plan(P);
    }
};

// One single-end file.  The rungs, fastest first: an ordinary gzip file decoded by the device (one-file entries only);
// BGZF members inflated on the device; the host threads' sources (mapped pages, zlib per BGZF member, the parallel gzip
// decoder) with the records scanned on the device or by those threads; one inflate stream, for a gzip file the parallel
// decoder handed back; the host readers of count_single_end_file, which end in the sequential reference-exact parser.
struct SingleEndLadder : Ladder {
    enum Rung { DEVICE_GUNZIP, DEVICE_INFLATE, HOST_THREADS, SINGLE_STREAM, HOST_READER };

    SingleEndLadder(const char* file, scg::FastqStream& stream, int n_threads, bool one_file) : path(file), fq(stream), nthreads(n_threads) {
        rung = !scg::env().device_scan ? HOST_READER : one_file ? DEVICE_GUNZIP : DEVICE_INFLATE;
    }

    // The first rung that applies takes its first windows; no plan is needed for that.
    void begin() {
        try {
            while (rung != HOST_READER && !enter()) ++rung;
            if (ring) ring->start();
        } catch (const UnusualInput&) {
            decline(nullptr);
        }
    }

    void finish(const std::vector<scg_plan*>& plans) {
        while (rung != HOST_READER) {
            try {
                if (!ring && !enter()) { ++rung; continue; }
                ring->run(plans);
                ring.reset();
                return;
            } catch (const UnusualInput&) {
                decline(&plans);
            }
        }
        entered(name(HOST_READER));
        DeviceGuard g(plans[0]->device);
        count_single_end_file(plans[0], path, fq, nthreads, nullptr, nullptr, nullptr);
    }

private:
    const char* path;
    scg::FastqStream& fq;
    int nthreads;
    std::unique_ptr<scg::TextSource> src;      // (declared before the ring that reads it)
    std::unique_ptr<WindowRing> ring;
    bool parallel_gzip = false;                // the source of HOST_THREADS is the parallel gzip decoder

    static const char* name(int r) {
        static const char* const names[] = {"device-gunzip", "device-inflate", "host-threads", "single-stream", "host-reader"};
        return names[r];
    }

    // Opens the rung's source and sets up its ring; false when the rung does not apply to this file.
    bool enter() {
        bool inflate = false;
        switch (rung) {
        case DEVICE_GUNZIP:
            src = device_gunzip(path);
            if (!src) return false;
            devices.resize(1);
            break;
        case DEVICE_INFLATE:
            if (!scg::env().device_inflate) return false;
            src = scg::TextSource::open(path, threads);
            if (!src->has_members()) return false;           // (the source serves HOST_THREADS)
            inflate = true;
            break;
        case HOST_THREADS:
            if (!src) src = scg::TextSource::open(path, threads);
            parallel_gzip = is_parallel_gzip(src.get());
            break;
        case SINGLE_STREAM:
            if (!parallel_gzip) return false;
            src = scg::TextSource::open(path, threads, false);
            break;
        }
        entered(name(rung));
        ring.reset(new WindowRing(*src, devices, inflate));
        devices.resize(ring->n_devices());
        return true;
    }

    void decline(const std::vector<scg_plan*>* plans) {
        ring.reset();
        src.reset();
        const int next = rung < HOST_THREADS ? HOST_THREADS : rung == HOST_THREADS && parallel_gzip ? SINGLE_STREAM : HOST_READER;
        declined(name(rung), name(next), rung == DEVICE_INFLATE && scg::env().inflate_strict, plans);
        rung = next;
    }
};

// What the one-file entries share: `compile` (template + pools -> plan: host work only) runs on a second thread while
// `begin` picks the devices and sends the first windows on their way; then the plans go to the devices and the ladder is
// finished.  Errors keep the reference's order: the reader was opened by the caller, the handler's constructor (compile)
// comes before anything met while reading.
template<class L>
std::unique_ptr<PlanSet> compile_and_finish(L& ladder, const Compile& compile, const std::function<void()>& begin, const char* first, const char* counted) {
    Trace tr;
    std::unique_ptr<scg_plan> compiled;
    std::exception_ptr compile_err, early;
    std::thread th([&] {
        try { compiled = compile(); } catch (...) { compile_err = std::current_exception(); }
    });
    try { begin(); } catch (...) { early = std::current_exception(); }
    th.join();
    if (compile_err) std::rethrow_exception(compile_err);
    if (early) std::rethrow_exception(early);
    tr.mark(first);
    std::unique_ptr<PlanSet> set(new PlanSet(std::move(compiled), ladder.devices));
    tr.mark("upload to device(s)");
    ladder.finish(set->all());
    tr.mark(counted);
    return set;
}

size_t whole_text_window() { return window_bytes(TEXT_WINDOW, ~uint64_t(0) >> 8); }

// One single-end file on a set of plans (one per device), for the many-files entries.
void count_single_end(const std::vector<scg_plan*>& plans, const char* path, scg::FastqStream& fq, int nthreads) {
    SingleEndLadder ladder(path, fq, nthreads, false);
    for (scg_plan* P : plans) ladder.devices.push_back(P->device);
    ladder.threads = scg::default_host_threads(nthreads);
    ladder.finish(plans);
}

// One single-end file for a one-file entry point.
std::unique_ptr<PlanSet> compile_and_count_single_end(const char* path, scg::FastqStream& fq, int nthreads, Compile compile) {
    SingleEndLadder ladder(path, fq, nthreads, true);
    return compile_and_finish(ladder, compile, [&] {
        ladder.devices = devices_for_input(text_bytes_hint(path), whole_text_window());
        ladder.threads = scg::default_host_threads(nthreads, static_cast<int>(ladder.devices.size()));
        ladder.begin();
    }, "compile + first window", "count file");
}

// Appends the reads [from, to) of `src` to `dst`.
void append_reads(scg::ReadBatch& dst, const scg::ReadBatch& src, int64_t from, int64_t to) {
    if (to <= from) return;
    const uint64_t b0 = src.offsets[from], b1 = src.offsets[to];
    const uint64_t base = dst.seqs.size();
    dst.seqs.insert(dst.seqs.end(), src.seqs.begin() + b0, src.seqs.begin() + b1);
    for (int64_t i = from + 1; i <= to; ++i) dst.offsets.push_back(base + (src.offsets[i] - b0));
}

// Both FASTQ files of a paired-end run (process_data.hpp:224-340).  Plain files are parsed by the
// multi-threaded reader, each file on its own; the two read streams are re-cut into batches of
// equal read counts (pair i = read i of both files).  gzip input or anything unusual falls back to
// the sequential readers in lock-step.  Unequal read counts => the reference's error.
void count_paired_host(scg_plan* P, const char* path1, const char* path2, scg::FastqStream& fq1, scg::FastqStream& fq2, int nthreads) {
    Stager st;
    auto launch_pair = [&](const scg::ReadBatch& x, const scg::ReadBatch& y) {
        auto& s = st.acquire();
        ScgReads R1 = st.stage(s, 0, x);
        ScgReads R2 = st.stage(s, 1, y);
        launch_batch_paired(P, R1, R2, x.size(), s.stream);
        s.busy = true;
    };
    const int threads = scg::default_host_threads(nthreads);
    if (threads > 1 && scg::ParallelFastq::is_plain_file(path1) && scg::ParallelFastq::is_plain_file(path2)) {
        const int half = threads > 3 ? threads / 2 : 2;
        scg::ParallelFastq pf1(path1, half), pf2(path2, half);
        scg::ReadBatch q1, q2;          // reads parsed but not yet paired
        q1.clear(); q2.clear();
        std::vector<scg::ReadBatch> w1, w2;
        bool more1 = true, more2 = true, odd = false;
        while (more1 || more2) {
            // advance whichever stream is behind (both at first)
            const bool need1 = more1 && q1.size() <= q2.size();
            const bool need2 = more2 && q2.size() <= q1.size();
            std::thread t;
            bool got2 = false;
            if (need2) t = std::thread([&] { got2 = pf2.next_window(w2); });
            bool got1 = need1 ? pf1.next_window(w1) : false;
            if (t.joinable()) t.join();
            if (need1) { if (got1) for (auto& b : w1) append_reads(q1, b, 0, b.size()); else more1 = false; }
            if (need2) { if (got2) for (auto& b : w2) append_reads(q2, b, 0, b.size()); else more2 = false; }
            if (pf1.unusual() || pf2.unusual()) { odd = true; break; }
            const int64_t n = std::min(q1.size(), q2.size());
            if (n > 0) {
                scg::ReadBatch a, b2, r1, r2;
                a.clear(); b2.clear(); r1.clear(); r2.clear();
                append_reads(a, q1, 0, n); append_reads(r1, q1, n, q1.size());
                append_reads(b2, q2, 0, n); append_reads(r2, q2, n, q2.size());
                launch_pair(a, b2);
                q1.seqs.swap(r1.seqs); q1.offsets.swap(r1.offsets);
                q2.seqs.swap(r2.seqs); q2.offsets.swap(r2.offsets);
            }
            if (!need1 && !need2) break;
        }
        st.drain();
        if (!odd) {
            if (q1.size() != q2.size()) {
                throw Error(SCG_ERR_IO, "different number of reads in paired FASTQ files");   // process_data.hpp:284-285
            }
            return;
        }
        reset_plan(P);                  // (as above: the windows' counts go, dense and sparse)
    }
    scg::ReadBatch b1, b2;
    for (;;) {
        bool more1 = fq1.next_batch(b1, BATCH_READS / 4, INT64_MAX);
        bool more2 = fq2.next_batch(b2, BATCH_READS / 4, INT64_MAX);
        if (b1.size() != b2.size()) {
            throw Error(SCG_ERR_IO, "different number of reads in paired FASTQ files");   // process_data.hpp:284-285
        }
        if (!more1 && !more2) break;
        launch_pair(b1, b2);
    }
    st.drain();
}

// Both files of a paired-end run, on one plan per device (several only for PairedRounds).  The rungs: mates the device
// decodes itself (BGZF members inflated, ordinary gzip decoded there), paired on that device; mates decoded by the host
// threads, paired on one device (PairedPipeline) or, plain files in a one-file entry, over all of them (PairedRounds); one
// inflate stream per mate, for gzip mates the parallel decoder handed back; the host readers of count_paired_host.
struct PairedLadder : Ladder {
    enum Rung { DEVICE_MATES, HOST_THREADS, SINGLE_STREAM, HOST_READER };

    PairedLadder(const char* file1, const char* file2, scg::FastqStream& stream1, scg::FastqStream& stream2, int n_threads)
        : path1(file1), path2(file2), fq1(stream1), fq2(stream2), nthreads(n_threads) {
        rung = scg::env().device_scan ? DEVICE_MATES : HOST_READER;
    }

    // The first rung that applies takes the first window of each file; no plan is needed for that.
    void begin() {
        try {
            while (rung != HOST_READER && !enter()) ++rung;
            if (pipe) pipe->start();
        } catch (const UnusualInput&) {
            decline(nullptr);
        }
        if (!rounds) devices.resize(1);
    }

    void finish(const std::vector<scg_plan*>& plans) {
        DeviceGuard g(plans[0]->device);
        while (rung != HOST_READER) {
            try {
                if (!pipe && !rounds && !enter()) { ++rung; continue; }
                if (rounds) rounds->run(plans); else pipe->run(plans[0]);
                rounds.reset();
                pipe.reset();
                return;
            } catch (const UnusualInput&) {
                decline(&plans);
            }
        }
        entered(name(HOST_READER));
        count_paired_host(plans[0], path1, path2, fq1, fq2, nthreads);
    }

private:
    const char *path1, *path2;
    scg::FastqStream &fq1, &fq2;
    int nthreads;
    std::unique_ptr<scg::TextSource> s1, s2;   // (declared before the pipelines that read them)
    std::unique_ptr<PairedPipeline> pipe;
    std::unique_ptr<PairedRounds> rounds;
    bool parallel_gzip = false;                // a source of HOST_THREADS is the parallel gzip decoder

    static const char* name(int r) {
        static const char* const names[] = {"device-mates", "host-threads", "single-stream", "host-reader"};
        return names[r];
    }

    // One mate for the host threads (two parallel gzip decoders share them).
    std::unique_ptr<scg::TextSource> open_mate(const char* path, bool on_device) const {
        std::unique_ptr<scg::TextSource> s;
        if (on_device) s = device_gunzip(path);
        if (!s) s = scg::TextSource::open(path, threads, rung != SINGLE_STREAM, std::max(2, threads / 2));
        return s;
    }

    // Opens the rung's sources and sets up its pipeline; false when the rung does not apply to these files.
    bool enter() {
        if (rung == SINGLE_STREAM && !parallel_gzip) return false;
        if (rung != HOST_THREADS || !s1) {
            // (an ordinary gzip mate is decoded by the device one mate after the other)
            s1 = open_mate(path1, rung == DEVICE_MATES);
            s2 = open_mate(path2, rung == DEVICE_MATES);
        }
        if (rung == DEVICE_MATES) {
            const bool inflates = scg::env().device_inflate && (s1->has_members() || s2->has_members());
            if (!inflates && !s1->device_resident() && !s2->device_resident()) return false;      // (the sources serve HOST_THREADS)
        }
        if (rung == HOST_THREADS) parallel_gzip = is_parallel_gzip(s1.get()) || is_parallel_gzip(s2.get());
        entered(name(rung));
        if (rung == HOST_THREADS && devices.size() > 1 && s1->parses() && s2->parses() && scg::env().host_scan) {
            rounds.reset(new PairedRounds(devices, *s1, *s2));
        } else {
            devices.resize(1);
            pipe.reset(new PairedPipeline(devices[0], *s1, *s2, rung == DEVICE_MATES));
        }
        return true;
    }

    void decline(const std::vector<scg_plan*>* plans) {
        const bool strict = rung == DEVICE_MATES && scg::env().inflate_strict && pipe && pipe->inflates();
        pipe.reset();
        rounds.reset();
        s1.reset();
        s2.reset();
        const int next = rung == DEVICE_MATES ? HOST_THREADS : rung == HOST_THREADS && parallel_gzip ? SINGLE_STREAM : HOST_READER;
        declined(name(rung), name(next), strict, plans);
        rung = next;
    }
};

// One pair of files on one plan, for the many-files entries.
void count_paired_files(scg_plan* P, const char* path1, const char* path2, scg::FastqStream& fq1, scg::FastqStream& fq2, int nthreads) {
    PairedLadder ladder(path1, path2, fq1, fq2, nthreads);
    ladder.devices.assign(1, P->device);
    ladder.threads = scg::default_host_threads(nthreads);
    ladder.finish(std::vector<scg_plan*>(1, P));
}

// One pair of files for a one-file entry point.  Plain mates and more than one device: the pairs go round-robin over all
// of them (PairedRounds); otherwise one device.
std::unique_ptr<PlanSet> compile_and_count_paired(const char* path1, const char* path2, scg::FastqStream& fq1, scg::FastqStream& fq2, int nthreads,
                                                  Compile compile) {
    PairedLadder ladder(path1, path2, fq1, fq2, nthreads);
    return compile_and_finish(ladder, compile, [&] {
        ladder.devices = devices_for_input(text_bytes_hint(path1) + text_bytes_hint(path2), whole_text_window());
        ladder.threads = scg::default_host_threads(nthreads, static_cast<int>(ladder.devices.size()));
        ladder.begin();
    }, "compile + first windows", "count files");
}

void release_cached_slots() { slot_pool().clear(); }

} // namespace scgapi
