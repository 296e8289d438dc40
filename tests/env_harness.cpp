// env_harness.cpp -- csrc/scg_env.h on its own (tests/test_env_cpu.py builds and runs this, natively and under
// AddressSanitizer + UBSan).
//   env_harness read     prints Env::read() of the process environment as one line of name=value pairs
//   env_harness scopes   the snapshot rules of EnvScope and env(), in process; prints "ok: ..." or the rule that broke
//   env_harness first    the same for a program that never opens a scope
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "../screencounter_amd/csrc/scg_env.h"

static int print_env() {
    const scg::Env e = scg::Env::read();
    std::printf("SCG_DEVICE=%d SCG_DEVICE.set=%d SCG_DEVICES=[%s] SCG_DEVICES.set=%d SCG_HOST_THREADS=%d ", e.device, e.device_set, e.devices.c_str(),
                e.devices_set, e.host_threads);
    std::printf("SCG_REPLICA_ADDR_LOG2=%d SCG_DENSE_CELLS=%lld SCG_TALLY=%d SCG_EXTRA_LDS_KB=%zu SCG_DUAL_TWO_TILES=%d SCG_INFLATE_LANES=%d ",
                e.replica_addr_log2, static_cast<long long>(e.dense_cells), e.tally, e.extra_lds_kb, e.dual_two_tiles, e.inflate_lanes);
    std::printf("SCG_TABLE_FACTOR=%d SCG_SEED_MAX=%d SCG_GZIP_WHOLE_GB=%g SCG_LIBDEFLATE=%d SCG_TRACE=%d SCG_FORCE_GENERAL=%d ", e.table_factor, e.seed_max,
                e.gzip_whole_gb, e.libdeflate, e.trace, e.force_general);
    std::printf("SCG_DEVICE_SCAN=%d SCG_HOST_SCAN=%d SCG_BUFFER_CACHE=%d SCG_DEVICE_INFLATE=%d SCG_DEVICE_INFLATE.strict=%d SCG_DEVICE_GUNZIP=%d "
                "SCG_DEVICE_GUNZIP.strict=%d SCG_PGZIP=%d ",
                e.device_scan, e.host_scan, e.buffer_cache, e.device_inflate, e.inflate_strict, e.device_gunzip, e.gunzip_strict, e.pgzip);
    std::printf("SCG_WINDOW_KB=%zu SCG_FASTQ_PIECE_KB=%zu SCG_TEST_RANDOM_TAG_BITS=%d SCG_DGZIP_CHUNK_KB=%zu SCG_DGZIP_CHUNK_KB.set=%d SCG_DGZIP_TAIL_GROUP=%u "
                "SCG_DGZIP_MIN_MEMBER_CHUNKS=%llu SCG_DGZIP_GROUP_KB=%llu SCG_PGZIP_CHUNK_KB=%zu SCG_PGZIP_CAP_KB=%zu\n",
                e.window_kb, e.fastq_piece_kb, e.random_tag_bits, e.dgzip_chunk_kb, e.dgzip_tiny, e.dgzip_tail_group,
                static_cast<unsigned long long>(e.dgzip_min_member_chunks), static_cast<unsigned long long>(e.dgzip_group_kb), e.pgzip_chunk_kb, e.pgzip_cap_kb);
    return 0;
}

#define EXPECT(cond, what) do { if (!(cond)) { std::printf("FAILED: %s\n", what); return 1; } } while (0)

// SCG_SEED_MAX stands for every switch: 9 unless the variable says 4 .. 10.
static int seen() { return scg::env().seed_max; }
static void set(const char* v) { ::setenv("SCG_SEED_MAX", v, 1); }

static int scopes() {
    set("5");
    {
        scg::EnvScope outer;
        EXPECT(seen() == 5, "the outermost scope takes the snapshot");
        set("6");
        EXPECT(seen() == 5, "setenv inside an open scope does not change env()");
        {
            scg::EnvScope nested;
            EXPECT(seen() == 5, "a nested scope does not refresh the snapshot");
        }
        EXPECT(seen() == 5, "leaving a nested scope does not refresh the snapshot");
        int on_worker = 0;
        std::thread([&] { on_worker = seen(); }).join();
        EXPECT(on_worker == 5, "a thread of the call sees the call's snapshot");
    }
    EXPECT(seen() == 5, "leaving the last scope does not refresh the snapshot");
    {
        scg::EnvScope next;
        EXPECT(seen() == 6, "the next outermost scope sees the new value");
    }
    // a scope held open by a second thread: one opened meanwhile on this thread is not the outermost
    set("7");
    scg::EnvScope* other = nullptr;
    std::thread([&] { other = new scg::EnvScope; }).join();
    EXPECT(seen() == 7, "a scope on a second thread, with none open, takes the snapshot");
    set("8");
    {
        scg::EnvScope mine;
        EXPECT(seen() == 7, "a scope does not refresh while one opened on a second thread is alive");
    }
    std::thread([&] { delete other; }).join();
    {
        scg::EnvScope mine;
        EXPECT(seen() == 8, "once the second thread's scope is gone, the next scope refreshes");
    }
    std::printf("ok: scopes\n");
    return 0;
}

static int first_use() {
    set("5");
    EXPECT(seen() == 5, "without a scope the first env() takes the snapshot");
    set("6");
    EXPECT(seen() == 5, "without a scope a later setenv does not change env()");
    int on_worker = 0;
    std::thread([&] { on_worker = seen(); }).join();
    EXPECT(on_worker == 5, "another thread sees the same first-use snapshot");
    std::printf("ok: first\n");
    return 0;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!std::strcmp(mode, "read")) return print_env();
    if (!std::strcmp(mode, "scopes")) return scopes();
    if (!std::strcmp(mode, "first")) return first_use();
    std::fprintf(stderr, "usage: env_harness read|scopes|first\n");
    return 2;
}
