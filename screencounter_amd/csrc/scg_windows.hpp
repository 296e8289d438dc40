// scg_windows.hpp -- windows of FASTQ text on their way to the counting kernels: the scan slots and their pool, how a
// window of text or of BGZF members is enqueued and read back, the ring of slots of single-end input (WindowRing) and the
// two paired pipelines (PairedPipeline, PairedRounds).  Included by scg_files.cpp alone.
//
// Host-side counterpart of the reference's chunked drivers (inst/include/kaori/process_data.hpp:105-190, :224-340):
// instead of handing 100 000-read chunks to std::threads, windows of the file go through pinned buffers into HBM on
// several HIP streams and are counted by the kernels of scg_kernels.hip.
#ifndef SCG_WINDOWS_HPP
#define SCG_WINDOWS_HPP
#include "scg_internal.hpp"

namespace scgapi {

// -------------------------------------------------------------------------------------------------
// Device-scan windows: raw FASTQ text -> pinned window -> HBM -> record scan -> counting kernels.
//
// The host moves bytes only (scg_ingest.cpp: file pages or inflated gzip blocks, cut at record boundaries); the
// records are found and validated on the GPU (scg_textscan.hip), so the text crosses PCIe once and no host thread
// parses it.  Anything the scan reports as out of the ordinary raises UnusualInput and the ladder of scg_files.cpp
// moves the file to its next rung.
// -------------------------------------------------------------------------------------------------
struct UnusualInput {};

inline double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

struct ScanSlot {
    scg_plan* plan = nullptr;
    int plan_device = -1;
    hipStream_t stream = nullptr;
    PinnedBuf text, h_result, h_offsets;
    DevBuf d_text, d_counts, d_nl, d_offsets, d_seqs, d_result, d_scan;
    scg::TextScanBuffers B;
    size_t cap = 0;
    bool pending = false;      // scan enqueued; the counting kernels still have to be launched
    bool parsed = false;       // the host did the record scan of the pending window: `host_result` holds its outcome
    scg::TextScanResult host_result{};
    bool busy = false;         // work of an earlier window may still be running on the stream

    // device-side inflate only:
    DevBuf d_in, d_status;     // compressed members + their table; failure flags of the inflate / carry kernels
    PinnedBuf h_status;
    hipEvent_t scanned = nullptr, carried = nullptr;
    size_t pinned_cap = 0;     // bytes of `text` (the pinned staging buffer): the window, or less when only compressed bytes pass through
    uint32_t text_bytes = 0;   // text in d_text for the pending window
    bool inflated = false;     // the pending window was inflated on the device: its records lie behind the gap's dummy
    bool last = false;         // the pending window is the input's last

    void init(int device, size_t window, size_t pinned_bytes) {
        plan_device = device;
        cap = window;
        pinned_cap = pinned_bytes;
        DeviceGuard g(device);
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        text.ensure(pinned_cap);
        h_result.ensure(sizeof(scg::TextScanResult));
        B.cap_blocks = scg::text_scan_blocks(cap) + 1;
        B.cap_lines = cap / 16 + 1024;              // lines shorter than 16 bytes on average: left to the sequential reader
        B.cap_records = B.cap_lines / 4 + 1;
        B.cap_seq_bytes = cap / 2 + 64;
        h_offsets.ensure((B.cap_records + 1) * sizeof(uint32_t));
        d_text.alloc(scg::text_scan_padded(cap) + 16);
        d_counts.alloc(B.cap_blocks * sizeof(uint32_t));
        d_nl.alloc(B.cap_lines * sizeof(uint32_t));
        d_offsets.alloc((B.cap_records + 1) * sizeof(uint32_t));
        d_seqs.alloc(B.cap_seq_bytes + 64);
        d_result.alloc(sizeof(scg::TextScanResult));
        d_scan.alloc(scg::text_scan_scratch(B.cap_blocks, B.cap_records) * sizeof(uint32_t));
        B.scan_scratch = d_scan.as<uint32_t>();
        B.block_counts = d_counts.as<uint32_t>();
        B.nl = d_nl.as<uint32_t>();
        B.offsets = d_offsets.as<uint32_t>();
        B.seqs = d_seqs.as<char>();
        B.result = d_result.as<scg::TextScanResult>();
    }
    // The extras of device-side inflate, on first use.
    void ensure_inflate() {
        if (scanned) return;
        DeviceGuard g(plan_device);
        d_in.alloc(pinned_cap);
        d_status.alloc(sizeof(uint32_t));
        h_status.ensure(sizeof(uint32_t));
        HIP_CHECK(hipEventCreateWithFlags(&scanned, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&carried, hipEventDisableTiming));
    }
    ~ScanSlot() {
        if (!stream) return;
        QuietDeviceGuard g(plan_device);
        (void)hipStreamSynchronize(stream);
        if (scanned) (void)hipEventDestroy(scanned);
        if (carried) (void)hipEventDestroy(carried);
        (void)hipStreamDestroy(stream);
    }
};

// Idle scan slots are kept for the next call (pinning and unpinning 3 x 128 MB of host memory costs ~120 ms, a third
// of the time a 10 GB file takes): at most four per device (the paired pipeline uses four), released by scg_release_buffers() or with the process.
struct SlotPool {
    std::mutex mu;
    std::vector<std::unique_ptr<ScanSlot> > idle;
    // pinned_bytes = 0: as much pinned staging as text (the raw-text and host-scan windows)
    std::unique_ptr<ScanSlot> take(int device, size_t window, size_t pinned_bytes = 0) {
        const bool whole = pinned_bytes == 0;          // these windows fill the pinned buffer up to the slot's capacity
        if (whole) pinned_bytes = window;
        {
            std::lock_guard<std::mutex> g(mu);
            for (size_t i = 0; i < idle.size(); ++i) {
                if (idle[i]->plan_device == device && idle[i]->cap >= window && idle[i]->cap <= 2 * window + (size_t(8) << 20) &&
                    idle[i]->pinned_cap >= (whole ? idle[i]->cap : pinned_bytes)) {
                    std::unique_ptr<ScanSlot> s = std::move(idle[i]);
                    idle.erase(idle.begin() + static_cast<long>(i));
                    s->plan = nullptr;
                    return s;
                }
            }
        }
        std::unique_ptr<ScanSlot> s(new ScanSlot);
        s->init(device, window, pinned_bytes);
        return s;
    }
    void give(std::unique_ptr<ScanSlot> s) {
        s->plan = nullptr;
        std::lock_guard<std::mutex> g(mu);
        // At most 4 idle slots per device and size class (slots that could serve one another's windows), 8 per device:
        // a process that alternates between input forms -- plain files, then BGZF -- keeps both kinds instead of
        // allocating 2.5 GB anew on every call of the second kind (25 ms per call, measured in bench.py's BGZF leg).
        int same = 0, on_device = 0;
        for (auto& x : idle) {
            if (x->plan_device != s->plan_device) continue;
            ++on_device;
            same += 2 * x->cap <= 3 * s->cap && 2 * s->cap <= 3 * x->cap;       // (within a factor of 1.5: 128 MB text windows and 257 MB inflate windows are two classes)
        }
        if (same < 4 && on_device < 8) idle.push_back(std::move(s));
    }
    void clear() {
        std::lock_guard<std::mutex> g(mu);
        idle.clear();
    }
};

inline SlotPool& slot_pool() {
    static SlotPool* pool = new SlotPool;      // deliberately never destroyed: the HIP runtime may be gone by then
    return *pool;
}

// The end of a pipeline's slots: their streams are let finish (a pipeline that is torn down after a decline has no kernel
// running when the plans are reset); slots of a call that went through are kept for the next one.
inline void retire_slot(std::unique_ptr<ScanSlot>& s, bool keep) {
    if (!s) return;
    {
        QuietDeviceGuard g(s->plan_device);
        (void)hipStreamSynchronize(s->stream);
    }
    s->busy = false; s->pending = false;
    if (keep) slot_pool().give(std::move(s));
}

// Text capacity of a window: `base` bytes (SCG_WINDOW_KB overrides it), less for small inputs.
inline size_t window_bytes(size_t base, uint64_t hint) {
    const size_t window_kb = scg::env().window_kb;
    size_t w = window_kb ? window_kb << 10 : base;                // test hook: tiny windows force many hand-overs
    const uint64_t need = hint + (hint >> 4) + 4096;               // the whole input in one window when it is small
    if (need < w) w = static_cast<size_t>(need);
    return std::max(w, window_kb ? size_t(4) << 10 : scg::TextSource::min_capacity());
}
constexpr size_t TEXT_WINDOW = size_t(128) << 20;
constexpr size_t INFLATE_WINDOW = size_t(256) << 20;   // 4 000 BGZF members in flight
constexpr size_t INFLATE_GAP = size_t(1) << 20;        // room in front of a window's text for the previous window's partial record
inline size_t inflate_window_staging(size_t cap_text) { return cap_text / 2 + (size_t(1) << 20); }     // compressed bytes + member table
inline size_t inflate_window_slot(size_t cap_text) { return INFLATE_GAP + cap_text + 64; }

// The sequences and offsets the host threads found in a window (pinned, in segments) go to the slot's HBM buffers,
// back to back: one kernel pulls them over the link.  Returns the number of records.
inline uint32_t enqueue_gather(ScanSlot& s, const scg::ParsedWindow& w) {
    if (w.seq_bytes > s.B.cap_seq_bytes || w.seq_bytes > 0xFFFFFFFFull || w.n_records > s.B.cap_records) throw UnusualInput();
    scg::GatherSegments G;
    G.n = static_cast<uint32_t>(w.n_segs);
    uint32_t rec = 0, at = 0;
    for (int i = 0; i < w.n_segs; ++i) {
        const scg::ParsedSegment& g = w.seg[i];
        G.seq_src[i] = s.text.as<char>() + g.seq_at;
        G.off_src[i] = s.h_offsets.as<uint32_t>() + g.off_at;
        G.seq_at[i] = at;
        G.first[i] = rec;
        G.off_base[i] = 0;
        rec += g.n_records;
        at += g.seq_bytes;
    }
    G.seq_at[G.n] = at;
    G.first[G.n] = rec;
    HIP_CHECK(scg::launch_gather_segments(s.B.seqs, s.B.offsets, G, s.stream));
    return rec;
}

// Takes the next window of `src` into slot `s` and enqueues, on the slot's stream, what turns it into sequences and
// offsets in HBM: text that lies in this device's HBM already (an ordinary gzip file decoded by the device) is scanned
// where it is; records the host threads found (`host_scan`) are gathered over the link; raw text is copied and scanned.
// Returns false at the end of the input.
inline bool enqueue_text_window(scg::TextSource& src, ScanSlot& s, bool host_scan, double* t_fill) {
    const auto f0 = std::chrono::steady_clock::now();
    scg::ParsedWindow w;
    const bool on_device = src.device_resident() && src.device() == s.plan_device;
    host_scan = host_scan && !on_device;
    const size_t bytes = on_device ? src.next_device(s.d_text.as<char>(), s.cap, s.stream)
                       : host_scan ? src.next_parsed(s.text.as<char>(), s.cap, s.h_offsets.as<uint32_t>(), s.B.cap_records + 1, w)
                                   : src.next(s.text.as<char>(), s.cap);
    *t_fill += ms_since(f0);
    if (src.unusual()) throw UnusualInput();
    if (bytes == 0) return false;
    s.inflated = false;
    s.parsed = host_scan;
    if (host_scan) {
        const uint32_t rec = enqueue_gather(s, w);
        s.host_result = scg::TextScanResult{0, rec, w.max_len, 0, w.seq_bytes, 0, 0};
        return true;
    }
    if (!on_device) HIP_CHECK(hipMemcpyAsync(s.d_text.p, s.text.p, bytes, hipMemcpyHostToDevice, s.stream));
    HIP_CHECK(scg::launch_text_scan(s.d_text.as<char>(), bytes, s.B, s.stream));
    HIP_CHECK(hipMemcpyAsync(s.h_result.p, s.d_result.p, sizeof(scg::TextScanResult), hipMemcpyDeviceToHost, s.stream));
    return true;
}

// Takes the next BGZF members of `src` into slot `s` (staging = its pinned buffer) and enqueues, on the slot's stream:
// members + table -> HBM, inflate + CRC check behind the gap, then -- once `prev` (the window before, if any) has its
// record structure -- the carry of prev's partial record into the gap, the record scan, and the copies back of the
// scan result and the status word.  `reader` is the slot whose carry read this slot's previous text (its `carried`
// event is waited for before the text is overwritten).  Returns false at the end of the input.
inline bool enqueue_inflate_window(scg::TextSource& src, ScanSlot& s, const ScanSlot* prev, const ScanSlot& reader, size_t cap_text, size_t cap_in,
                                   std::vector<scg::CompressedMember>& members, double* t_fill) {
    const auto f0 = std::chrono::steady_clock::now();
    // staging: [member table | payloads]; room for one member per 32 bytes of compressed input is never short
    const size_t slack = scg::inflate_input_slack();
    const size_t table_cap = (cap_in / 32 / sizeof(scg::InflateMember)) * sizeof(scg::InflateMember);
    char* const stage = s.text.as<char>();
    size_t text_bytes = 0;
    bool last = false;
    const size_t in_bytes = src.next_members(stage + table_cap, cap_in - table_cap, slack, cap_text, members, text_bytes, last);
    if (src.unusual()) throw UnusualInput();
    if (in_bytes == 0) return false;
    if (members.size() * sizeof(scg::InflateMember) > table_cap) throw UnusualInput();        // (members of < 32 bytes: not a real file)
    static_assert(sizeof(scg::InflateMember) == sizeof(scg::CompressedMember), "same layout");
    scg::InflateMember* table = reinterpret_cast<scg::InflateMember*>(stage);
    for (size_t i = 0; i < members.size(); ++i) {
        table[i].in_off = static_cast<uint32_t>(table_cap) + members[i].in_off;
        table[i].in_len = members[i].in_len;
        table[i].out_off = static_cast<uint32_t>(INFLATE_GAP) + members[i].out_off;
        table[i].out_len = members[i].out_len;
        table[i].crc = members[i].crc;
    }
    *t_fill += ms_since(f0);
    const uint32_t n = static_cast<uint32_t>(members.size());
    HIP_CHECK(hipStreamWaitEvent(s.stream, reader.carried, 0));
    HIP_CHECK(hipMemsetAsync(s.d_status.p, 0, sizeof(uint32_t), s.stream));
    HIP_CHECK(hipMemcpyAsync(s.d_in.p, stage, n * sizeof(scg::InflateMember), hipMemcpyHostToDevice, s.stream));
    HIP_CHECK(hipMemcpyAsync(s.d_in.as<char>() + table_cap, stage + table_cap, in_bytes, hipMemcpyHostToDevice, s.stream));
    HIP_CHECK(scg::launch_inflate_members(s.d_in.as<uint8_t>(), s.d_in.as<scg::InflateMember>(), n, s.d_text.as<char>(), s.d_status.as<uint32_t>(), s.stream));
    s.text_bytes = static_cast<uint32_t>(INFLATE_GAP + text_bytes);
    if (last) {
        // the reference accepts a final record without its newline: one is appended (a second one is harmless, see window_records)
        HIP_CHECK(hipMemsetAsync(s.d_text.as<char>() + s.text_bytes, '\n', 1, s.stream));
        s.text_bytes += 1;
    }
    s.last = last;
    s.inflated = true;
    s.parsed = false;
    if (prev) HIP_CHECK(hipStreamWaitEvent(s.stream, prev->scanned, 0));
    HIP_CHECK(scg::launch_carry_tail(prev ? prev->d_text.as<char>() : nullptr, prev ? prev->B.result : nullptr, prev ? prev->text_bytes : 0u,
                                     s.d_text.as<char>(), static_cast<uint32_t>(INFLATE_GAP), s.d_status.as<uint32_t>(), s.stream));
    HIP_CHECK(hipEventRecord(s.carried, s.stream));
    HIP_CHECK(scg::launch_text_scan(s.d_text.as<char>(), s.text_bytes, s.B, s.stream, true, s.scanned));
    HIP_CHECK(hipMemcpyAsync(s.h_result.p, s.d_result.p, sizeof(scg::TextScanResult), hipMemcpyDeviceToHost, s.stream));
    HIP_CHECK(hipMemcpyAsync(s.h_status.p, s.d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    return true;
}

// The records of a slot's window: `n` of them from offsets[first] on.
struct WindowRecords {
    uint32_t first, n, max_len;
};

// After the slot's stream has been synchronised (windows scanned by the host need no such wait): the window's records.
// Throws UnusualInput for whatever a later rung has to redo: anything but ordinary records and, behind the device's
// inflater, a member zlib has to look at (corrupt, or in a form the device's decoder declines) or a record longer than the gap.
inline WindowRecords window_records(const ScanSlot& s) {
    const scg::TextScanResult r = s.parsed ? s.host_result : *s.h_result.as<scg::TextScanResult>();
    if (r.flags) throw UnusualInput();
    if (!s.inflated) return WindowRecords{0, r.n_records, r.max_len};
    if (*s.h_status.as<uint32_t>() || r.n_records == 0) throw UnusualInput();
    // behind the last whole record of the input: nothing, or the newline appended above
    if (s.last && s.text_bytes - r.cut > 1) throw UnusualInput();
    return WindowRecords{1, r.n_records - 1, r.max_len};            // record 0 is the gap's dummy
}

inline ScgReads window_reads(const ScanSlot& s, uint32_t first, uint32_t max_len) {
    return make_reads(s.B.seqs, s.B.offsets + first, 0, static_cast<int32_t>(std::min<uint32_t>(max_len, 1u << 30)));
}

// Kernels of one device read another device's memory (the previous window's tail, when the windows of a BGZF file go
// round-robin over the devices of a call): peer access, once per ordered pair.  False if the hardware does not offer it.
inline bool enable_peer_access(const std::vector<int>& devices) {
    for (int a : devices) {
        for (int b : devices) {
            if (a == b) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) return false;
            DeviceGuard g(a);
            const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); return false; }
            (void)hipGetLastError();
        }
    }
    return true;
}

// The single-end pipeline: a ring of slots, three per device, the windows going round-robin over the devices.  While
// window k is copied and scanned, the host fills window k + 1 and the counting kernels of window k - 1 run.  Slots belong
// to devices, not to plans, so the first windows can be on their way (start) while the template and the library are still
// being compiled on another thread; run() then binds the slots to the plans and carries on.  Replaces
// kaori::process_single_end_data (process_data.hpp:105-190).
//
// Two kinds of window go through it.  Text (enqueue_text_window): plain files, host-inflated gzip, text a device decoded.
// BGZF members inflated on the device (`inflate`; scg_inflate.hip): per window, on the slot's stream, compressed members +
// their table -> HBM; inflate + CRC check into the text buffer behind a gap; then -- once the previous window has been
// scanned -- the gap receives that window's partial last record (launch_carry_tail), the text is scanned for records and
// the result comes back.  The inflate kernels -- the expensive part -- of all slots overlap; only the carry chains the
// windows, and where the previous window lies on another device the carry kernel reads its tail (<= 1 MB) and its scan
// result over xGMI (peer access; the streams wait on each other's events).
class WindowRing {
public:
    WindowRing(scg::TextSource& source, const std::vector<int>& devs, bool inflate_on_device)
        : src(source), devices(devs), inflate(inflate_on_device), host_scan(!inflate_on_device && source.parses() && scg::env().host_scan), keep(scg::env().buffer_cache) {
        if (inflate && devices.size() > 1 && !enable_peer_access(devices)) devices.resize(1);
        cap_text = window_bytes(inflate ? INFLATE_WINDOW : TEXT_WINDOW, source.size_hint());
        cap_in = inflate ? inflate_window_staging(cap_text) : 0;
        for (int k = 0; k < 3; ++k) {
            for (int d : devices) {
                slots.push_back(slot_pool().take(d, inflate ? inflate_window_slot(cap_text) : cap_text, cap_in));
                if (inflate) slots.back()->ensure_inflate();
            }
        }
        tr.mark("  scan slots (pinned + HBM)");
    }
    ~WindowRing() {
        for (auto& s : slots) retire_slot(s, ok && keep);
    }
    size_t n_devices() const { return devices.size(); }     // (one device when the others cannot be reached over xGMI)

    // Before the plans exist (the library is still being compiled on another thread): every slot takes a window -- parse
    // or copy, the link, inflate and the device's record scan need no plan, only the counting does.
    void start() {
        for (size_t k = 0; k < slots.size() && !ended && filled == k; ++k) fill_next();
    }

    // plans[i] counts what device i of the list was given (fewer plans than devices: the list was cut down at construction)
    void run(const std::vector<scg_plan*>& plans) {
        for (size_t i = 0; i < slots.size(); ++i) slots[i]->plan = plans[(i % devices.size()) % plans.size()];
        // Window k is filled and put on the wire; the counting kernels of window k - lag are launched afterwards, by
        // which time its copy and scan have normally finished: the host thread does not wait on the link.
        // (Windows scanned by the host need no such wait.)
        const size_t lag = host_scan ? 0 : std::min(2 * devices.size(), slots.size() - 1);
        while (finished + lag < filled) finish_next();              // (the windows start() has taken while there was no plan)
        while (!ended) {
            fill_next();
            if (filled > lag && finished < filled - lag) finish_next();
        }
        while (finished < filled) finish_next();
        for (auto& s : slots) {
            DeviceGuard g(s->plan_device);
            HIP_CHECK(hipStreamSynchronize(s->stream));
            s->busy = false;
        }
        ok = true;
        if (tr.on) {
            std::fprintf(stderr, "[scg]   windows of %zu MB (%s, %zu device(s)): host fill %.2f ms, waiting for the device %.2f ms, for free slots %.2f ms\n",
                         cap_text >> 20, inflate ? "device inflate" : host_scan ? "host scan" : "device scan", devices.size(), t_fill, t_finish, t_busy);
        }
        tr.mark("  windows");
    }

private:
    scg::TextSource& src;
    std::vector<int> devices;
    bool inflate, host_scan, keep;
    size_t cap_text = 0, cap_in = 0;
    std::vector<std::unique_ptr<ScanSlot> > slots;
    std::vector<scg::CompressedMember> members;
    size_t filled = 0, finished = 0;     // windows put on the wire / windows whose counting kernels have been launched
    bool ended = false, ok = false;
    Trace tr;
    double t_fill = 0, t_finish = 0, t_busy = 0;

    void fill_next() {
        ScanSlot& s = *slots[filled % slots.size()];
        DeviceGuard g(s.plan_device);
        if (s.pending) finish_next();                              // (only when there are fewer slots than the lag needs)
        const auto b0 = std::chrono::steady_clock::now();
        if (s.busy) { HIP_CHECK(hipStreamSynchronize(s.stream)); s.busy = false; }
        t_busy += ms_since(b0);
        bool more;
        if (inflate) {
            const ScanSlot* prev = filled ? slots[(filled - 1) % slots.size()].get() : nullptr;
            const ScanSlot& next = *slots[(filled + 1) % slots.size()];  // the window after this slot's previous one read its tail from here
            more = enqueue_inflate_window(src, s, prev, next, cap_text, cap_in, members, &t_fill);
        } else {
            more = enqueue_text_window(src, s, host_scan, &t_fill);
        }
        if (!more) { ended = true; return; }
        s.pending = true;
        ++filled;
        if (inflate && s.last) ended = true;
    }

    void finish_next() {
        ScanSlot& s = *slots[finished % slots.size()];
        const auto f1 = std::chrono::steady_clock::now();
        DeviceGuard g(s.plan_device);
        if (!s.parsed) HIP_CHECK(hipStreamSynchronize(s.stream)); // copy + scan + result are in
        t_finish += ms_since(f1);
        s.pending = false;
        ++finished;
        const WindowRecords r = window_records(s);
        if (r.n) launch_batch(s.plan, window_reads(s, r.first, r.max_len), static_cast<int64_t>(r.n), s.stream);
        s.busy = true;
    }
};

// -------------------------------------------------------------------------------------------------
// The paired-end pipeline.  Each file is taken in windows like single-end input -- plain files scanned for records by
// the host threads, compressed ones shipped as text and scanned on the device -- and the two streams of sequences are
// brought into step on the device without moving them again: windows of the two files hold different numbers of
// records, so each mate keeps a cursor into its current window (sequences + offsets in HBM); the kernels count
// min(remaining, remaining) pairs from the two cursors, and the mate whose window is used up takes its next one.
// Replaces kaori::process_paired_end_data (process_data.hpp:224-340).  One device: pair i needs read i of both files.
// -------------------------------------------------------------------------------------------------
struct MateWindows {
    scg::TextSource* src = nullptr;
    std::unique_ptr<ScanSlot> slot[2];      // double buffer: the host fills one while the kernels read the other
    hipEvent_t used[2] = {nullptr, nullptr};// the last kernel reading slot k has been enqueued before this event
    hipEvent_t ready = nullptr;             // the current window has arrived in HBM
    bool host_scan = false, done = false, fresh = false;
    bool inflate = false;                   // BGZF mate, members inflated on the device (enqueue_inflate_window)
    bool any = false;                       // (inflate) a window has been taken before: its partial last record is carried on
    size_t cap_text = 0, cap_in = 0;        // (inflate) window sizes
    int cur = 1;
    uint32_t first = 0;                     // records of the current window start at offsets[first] (1 behind a gap's dummy record)
    uint32_t n = 0, k = 0, max_len = 0;     // records in the current window, of which k have been paired
    uint32_t remaining() const { return n - k; }
    ~MateWindows() {
        for (hipEvent_t e : used) if (e) (void)hipEventDestroy(e);
        if (ready) (void)hipEventDestroy(ready);
    }
};

class PairedPipeline {
public:
    // device_inflate: BGZF mates may have their members inflated on the device (false: by the host threads)
    PairedPipeline(int dev, scg::TextSource& src1, scg::TextSource& src2, bool device_inflate)
        : device(dev), window(std::max(window_bytes(TEXT_WINDOW, src1.size_hint()), window_bytes(TEXT_WINDOW, src2.size_hint()))),
          keep(scg::env().buffer_cache) {
        DeviceGuard g(device);
        mate[0].src = &src1; mate[1].src = &src2;
        HIP_CHECK(hipStreamCreateWithFlags(&compute, hipStreamNonBlocking));
        for (auto& m : mate) {
            m.host_scan = m.src->parses() && scg::env().host_scan;
            m.inflate = device_inflate && m.src->has_members() && scg::env().device_inflate;
            if (m.inflate) {
                m.cap_text = window_bytes(INFLATE_WINDOW, m.src->size_hint());
                m.cap_in = inflate_window_staging(m.cap_text);
            }
            for (int k = 0; k < 2; ++k) {
                m.slot[k] = slot_pool().take(device, m.inflate ? inflate_window_slot(m.cap_text) : window, m.cap_in);
                if (m.inflate) m.slot[k]->ensure_inflate();
                HIP_CHECK(hipEventCreateWithFlags(&m.used[k], hipEventDisableTiming));
            }
            HIP_CHECK(hipEventCreateWithFlags(&m.ready, hipEventDisableTiming));
            any_inflate |= m.inflate;
        }
        tr.mark("  scan slots (pinned + HBM)");
    }
    bool inflates() const { return any_inflate; }
    ~PairedPipeline() {
        QuietDeviceGuard g(device);
        if (compute) { (void)hipStreamSynchronize(compute); (void)hipStreamDestroy(compute); }
        for (auto& m : mate) for (auto& s : m.slot) retire_slot(s, ok && keep);
    }

    // The first window of each file on its way (no plan needed yet).
    void start() {
        DeviceGuard g(device);
        advance();
        advanced = true;
    }

    void run(scg_plan* P) {
        DeviceGuard g(device);
        for (;;) {
            if (advanced) advanced = false; else advance();
            for (auto& m : mate) {
                if (!m.fresh) continue;
                m.fresh = false;
                const ScanSlot& s = *m.slot[m.cur];
                const auto w0 = std::chrono::steady_clock::now();
                if (!s.parsed) HIP_CHECK(hipStreamSynchronize(s.stream));   // device scan: the record count comes back from the card
                t_wait += ms_since(w0);
                const WindowRecords r = window_records(s);
                m.first = r.first;
                m.n = r.n;
                m.max_len = r.max_len;
            }
            // one file is exhausted and fully paired while the other still holds reads (process_data.hpp:284-285)
            for (int i = 0; i < 2; ++i) {
                if (mate[i].done && mate[i].remaining() == 0 && mate[1 - i].remaining() > 0) {
                    throw Error(SCG_ERR_IO, "different number of reads in paired FASTQ files");
                }
            }
            if (mate[0].done && mate[1].done) break;
            const uint32_t np = std::min(mate[0].remaining(), mate[1].remaining());
            if (np == 0) continue;
            const uint32_t max_len = std::max(mate[0].max_len, mate[1].max_len);
            ScgReads R[2];
            for (int i = 0; i < 2; ++i) {
                MateWindows& m = mate[i];
                HIP_CHECK(hipStreamWaitEvent(compute, m.ready, 0));
                R[i] = window_reads(*m.slot[m.cur], m.first + m.k, max_len);
            }
            launch_batch_paired(P, R[0], R[1], static_cast<int64_t>(np), compute);
            for (auto& m : mate) {
                m.k += np;
                HIP_CHECK(hipEventRecord(m.used[m.cur], compute));
            }
        }
        HIP_CHECK(hipStreamSynchronize(compute));
        ok = true;
        if (tr.on) std::fprintf(stderr, "[scg]   paired windows of %zu MB: host fill %.2f ms, waiting for the device %.2f ms\n", window >> 20, t_fill, t_wait);
        tr.mark("  windows");
    }

private:
    int device;
    size_t window;
    bool keep;
    MateWindows mate[2];
    hipStream_t compute = nullptr;
    bool ok = false, advanced = false, any_inflate = false;
    std::vector<scg::CompressedMember> members;
    Trace tr;
    double t_fill = 0, t_wait = 0;

    // A mate whose window is used up takes its next one.
    void advance() {
        for (auto& m : mate) {
            m.fresh = false;
            if (m.done || m.remaining() > 0) continue;
            m.cur ^= 1;
            ScanSlot& s = *m.slot[m.cur];
            const auto w0 = std::chrono::steady_clock::now();
            HIP_CHECK(hipEventSynchronize(m.used[m.cur]));        // its previous content is no longer being read
            t_wait += ms_since(w0);
            m.n = m.k = 0;
            // (inflate: the window before lies in the mate's other slot: its partial last record is carried over on the device)
            const ScanSlot& other = *m.slot[m.cur ^ 1];
            const bool more = m.inflate ? enqueue_inflate_window(*m.src, s, m.any ? &other : nullptr, other, m.cap_text, m.cap_in, members, &t_fill)
                                        : enqueue_text_window(*m.src, s, m.host_scan, &t_fill);
            if (!more) { m.done = true; continue; }
            m.any = true;
            m.fresh = true;
            HIP_CHECK(hipEventRecord(m.ready, s.stream));
        }
    }
};

// -------------------------------------------------------------------------------------------------
// Paired plain files over SEVERAL devices.  Pair i needs read i of both files, so the work is handed out by record
// index: the host threads scan each mate's file in windows as they do for one device (PlainSource::next_parsed: sequences
// and offsets in pinned memory) and keep a cursor into each mate's current window; a round takes the
// min(remaining, remaining) pairs the two cursors have in common, and ONE device -- round-robin -- gathers exactly those
// records of both mates over its own PCIe link and counts them.  Every record crosses a link once, the devices work on
// different rounds at the same time, the per-device counters are summed at the end (PlanSet::read).  Replaces
// kaori::process_paired_end_data (process_data.hpp:224-340) for calls with more than one device; compressed mates keep
// the one-device pipeline above (their text exists only in one device's memory).
// -------------------------------------------------------------------------------------------------
class PairedRounds {
public:
    PairedRounds(const std::vector<int>& devs, scg::TextSource& src1, scg::TextSource& src2)
        : devices(devs), window(std::max(window_bytes(TEXT_WINDOW, src1.size_hint()), window_bytes(TEXT_WINDOW, src2.size_hint()))) {
        mate[0].src = &src1; mate[1].src = &src2;
        cap_lines = window / 16 + 1024;
        cap_records = cap_lines / 4 + 1;
        cap_seq = window / 2 + 64;
        for (auto& m : mate) {
            for (auto& hw : m.win) {
                hw.text.ensure(window);
                hw.offs.ensure((cap_records + 1) * sizeof(uint32_t));
            }
        }
        for (size_t i = 0; i < devices.size() * 2; ++i) {
            rounds.emplace_back(new Round);
            Round& R = *rounds.back();
            R.device = devices[i / 2];
            DeviceGuard g(R.device);
            HIP_CHECK(hipStreamCreateWithFlags(&R.stream, hipStreamNonBlocking));
            HIP_CHECK(hipEventCreateWithFlags(&R.done, hipEventDisableTiming));
            for (int k = 0; k < 2; ++k) {
                R.seqs[k].alloc(cap_seq + 64);
                R.offs[k].alloc((cap_records + 1) * sizeof(uint32_t));
            }
        }
        tr.mark("  round buffers (pinned + HBM)");
    }
    ~PairedRounds() {
        for (auto& rp : rounds) {
            Round& R = *rp;
            QuietDeviceGuard g(R.device);
            if (R.stream) { (void)hipStreamSynchronize(R.stream); (void)hipStreamDestroy(R.stream); }
            if (R.done) (void)hipEventDestroy(R.done);
            R.seqs[0].release(); R.seqs[1].release(); R.offs[0].release(); R.offs[1].release();
        }
    }

    // plans[d] belongs to devices[d]
    void run(const std::vector<scg_plan*>& plans) {
        const size_t D = devices.size();
        for (size_t r = 0;; ++r) {
            for (auto& m : mate) advance(m);
            const uint64_t rem0 = remaining(mate[0]), rem1 = remaining(mate[1]);
            if (rem0 == 0 && rem1 == 0) break;                                  // both files used up
            if (rem0 == 0 || rem1 == 0) throw Error(SCG_ERR_IO, "different number of reads in paired FASTQ files");   // process_data.hpp:284-285
            const uint64_t np = std::min(rem0, rem1);
            Round& R = *rounds[(r % D) * 2 + (r / D) % 2];
            DeviceGuard g(R.device);
            if (R.busy) { HIP_CHECK(hipStreamSynchronize(R.stream)); R.busy = false; }
            ScgReads reads[2];
            uint32_t max_len = 0;
            for (int i = 0; i < 2; ++i) {
                HostWindow& hw = mate[i].win[mate[i].cur];
                enqueue_range(R, i, hw, mate[i].k, np);
                max_len = std::max(max_len, hw.w.max_len);
            }
            for (int i = 0; i < 2; ++i) {
                reads[i] = make_reads(R.seqs[i].as<char>(), R.offs[i].as<uint32_t>(), 0, static_cast<int32_t>(std::min<uint32_t>(max_len, 1u << 30)));
            }
            launch_batch_paired(plans[r % D], reads[0], reads[1], static_cast<int64_t>(np), R.stream);
            HIP_CHECK(hipEventRecord(R.done, R.stream));
            R.busy = true;
            for (auto& m : mate) {
                m.win[m.cur].readers.push_back(std::make_pair(R.device, R.done));
                m.k += np;
            }
            ++n_rounds;
        }
        for (auto& rp : rounds) {
            DeviceGuard g(rp->device);
            HIP_CHECK(hipStreamSynchronize(rp->stream));
            rp->busy = false;
        }
        if (tr.on) std::fprintf(stderr, "[scg]   paired rounds over %zu device(s): %zu rounds of <= %zu MB windows, host scan %.2f ms\n", D, n_rounds, window >> 20, t_fill);
        tr.mark("  rounds");
    }

private:
    struct HostWindow {
        PinnedBuf text, offs;
        scg::ParsedWindow w;
        std::vector<std::pair<int, hipEvent_t> > readers;      // rounds whose gathers read this window
    };
    struct Mate {
        scg::TextSource* src = nullptr;
        HostWindow win[3];
        int cur = -1;
        uint64_t k = 0;              // records of the current window that have been paired
        bool done = false;
    };
    struct Round {
        int device = 0;
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        DevBuf seqs[2], offs[2];
        bool busy = false;
    };
    std::vector<int> devices;
    size_t window, cap_lines = 0, cap_records = 0, cap_seq = 0, n_rounds = 0;
    Mate mate[2];
    std::vector<std::unique_ptr<Round> > rounds;
    Trace tr;
    double t_fill = 0;

    static uint64_t remaining(const Mate& m) { return m.cur < 0 ? 0 : m.win[m.cur].w.n_records - m.k; }

    // A mate whose window is used up takes its next one (into the buffer whose readers have long finished).
    void advance(Mate& m) {
        if (m.done || remaining(m) > 0) return;
        const int next = (m.cur + 1) % 3;
        HostWindow& hw = m.win[next];
        for (auto& rd : hw.readers) {
            DeviceGuard g(rd.first);
            HIP_CHECK(hipEventSynchronize(rd.second));
        }
        hw.readers.clear();
        const auto f0 = std::chrono::steady_clock::now();
        const size_t bytes = m.src->next_parsed(hw.text.as<char>(), window, hw.offs.as<uint32_t>(), cap_records + 1, hw.w);
        t_fill += ms_since(f0);
        if (m.src->unusual()) throw UnusualInput();
        if (bytes == 0) { m.done = true; m.cur = -1; return; }
        if (hw.w.seq_bytes > cap_seq || hw.w.n_records > cap_records) throw UnusualInput();
        m.cur = next;
        m.k = 0;
    }

    // Records [k, k + n) of a parsed window -> the round's device buffers of mate i.
    void enqueue_range(Round& R, int i, const HostWindow& hw, uint64_t k, uint64_t n) {
        scg::GatherSegments G;
        G.n = 0;
        uint32_t rec = 0, at = 0;
        uint64_t base = 0;
        const uint32_t* offs = hw.offs.as<uint32_t>();
        for (int sgm = 0; sgm < hw.w.n_segs && base < k + n; ++sgm) {
            const scg::ParsedSegment& g = hw.w.seg[sgm];
            const uint64_t lo = std::max<uint64_t>(k, base), hi = std::min<uint64_t>(k + n, base + g.n_records);
            if (hi > lo) {
                const uint32_t j0 = static_cast<uint32_t>(lo - base), j1 = static_cast<uint32_t>(hi - base);
                const uint32_t* so = offs + g.off_at;
                G.seq_src[G.n] = hw.text.as<char>() + g.seq_at + so[j0];
                G.off_src[G.n] = so + j0;
                G.off_base[G.n] = so[j0];
                G.seq_at[G.n] = at;
                G.first[G.n] = rec;
                at += so[j1] - so[j0];
                rec += j1 - j0;
                ++G.n;
            }
            base += g.n_records;
        }
        G.seq_at[G.n] = at;
        G.first[G.n] = rec;
        HIP_CHECK(scg::launch_gather_segments(R.seqs[i].as<char>(), R.offs[i].as<uint32_t>(), G, R.stream));
    }
};

} // namespace scgapi

#endif
