// Stand-alone checks of csrc/stream_slots.h (tests/test_stream_slots_cpu.py compiles this for the host and runs it as a child process; it
// needs no device: without one hipMalloc fails cleanly, which is the failure path of erl_slot_grow).
//   stream_slots_main table    claim / find / exhaustion / release / failed grow
//   stream_slots_main threads  8 threads x 10 000 find-or-claim calls over 12 keys
//   stream_slots_main time     host time of one find on a warm 16-entry table: the hand-written scan the table replaced vs find under its lock
#include "stream_slots.h"

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

void erl_set_error(const char *, ...) {}      // (api.cpp's is not linked in)

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

namespace {

struct Two {                 // the shape of grad_tail.hip's S3Slot: two growable buffers
    void *buf = nullptr;
    size_t bytes = 0;
    void *aux = nullptr;
    size_t aux_bytes = 0;
    int marker = 7;
};

const void *stream_of(int i) { return reinterpret_cast<const void *>((uintptr_t)0x1000 * (i + 1)); }

int table_cases()
{
    // claim and find
    static StreamSlots<Two, 4> t;
    auto lock = t.lock();
    Two *a = t.find_or_claim(0, stream_of(0));
    CHECK(a && a->marker == 7 && !a->buf);
    CHECK(t.find_or_claim(0, stream_of(0)) == a && t.find(0, stream_of(0)) == a);
    Two *b = t.find_or_claim(1, stream_of(0)), *c = t.find_or_claim(0, stream_of(1)), *d = t.find_or_claim(0, stream_of(0), 199);
    CHECK(b && c && d && b != a && c != a && d != a && b != c && b != d && c != d);
    CHECK(!t.find(1, stream_of(1)) && !t.find(0, stream_of(0), 200));
    // exhaustion: Cap keys fill the table, one more gets nothing, the first Cap are still there
    CHECK(!t.find_or_claim(1, stream_of(1)));
    CHECK(t.find(0, stream_of(0)) == a && t.find(1, stream_of(0)) == b && t.find(0, stream_of(1)) == c && t.find(0, stream_of(0), 199) == d);
    // release: the entry is free again and its payload value-initialised
    c->marker = 99;
    c->bytes = 5;
    t.release(c);
    CHECK(!t.find(0, stream_of(1)));
    Two *e = t.find_or_claim(1, stream_of(1));
    CHECK(e == c && e->marker == 7 && e->bytes == 0 && !t.find_or_claim(0, stream_of(1)));     // (and the table is full again)

    // failed grow, first allocation: no device, so hipMalloc fails
    CHECK(erl_slot_grow(&a->buf, &a->bytes, 1024, nullptr, "hipMalloc(weight images)") != 0);
    CHECK(!a->buf && a->bytes == 0);
    // failed regrow: a block that is there (a stand-in address: with no device the wait on the stream fails before anything is freed)
    static char block[64], records[64];
    a->buf = block;
    a->bytes = sizeof(block);
    a->aux = records;
    a->aux_bytes = sizeof(records);
    CHECK(erl_slot_grow(&a->buf, &a->bytes, 64, nullptr, "hipMalloc(weight images)") == 0 && a->buf == block);    // never shrinks, no call
    CHECK(erl_slot_grow(&a->buf, &a->bytes, 4096, nullptr, "hipMalloc(weight images)") != 0);
    CHECK(!a->buf && a->bytes == 0);                                  // no stale size: a smaller request cannot take the null block for enough
    CHECK(a->aux == records && a->aux_bytes == sizeof(records));      // the other buffer stays with its key ...
    CHECK(t.find(0, stream_of(0)) == a);                              // ... and the entry is still found under it
    t.release(e);
    Two *f = t.find_or_claim(2, stream_of(2));                        // another key gets the free entry, not this one and not its records
    CHECK(f && f != a && !f->aux && f->aux_bytes == 0);
    puts("table ok");
    return 0;
}

struct Counter {
    long n = 0;
};

int thread_case()
{
    static StreamSlots<Counter, 16> t;
    std::vector<std::thread> th;
    int bad = 0;
    for (int k = 0; k < 8; ++k)
        th.emplace_back([k, &bad] {
            for (int i = 0; i < 10000; ++i) {
                const int key = (i * 7 + k) % 12;
                auto lock = t.lock();
                Counter *c = t.find_or_claim(key % 3, stream_of(key / 3));
                if (c) c->n++;        // (what a caller hands out under the look-up's lock: nonces, parities, ticket bases)
                else bad++;
            }
        });
    for (auto &x : th) x.join();
    auto lock = t.lock();
    long sum = 0;
    for (int key = 0; key < 12; ++key) {
        Counter *c = t.find(key % 3, stream_of(key / 3));
        CHECK(c);
        sum += c->n;
    }
    CHECK(bad == 0 && sum == 80000);
    for (int k = 0; k < 4; ++k) CHECK(t.find_or_claim(7, stream_of(k)));      // exactly 12 of the 16 entries were used: four more keys fit,
    CHECK(!t.find_or_claim(7, stream_of(4)));                                 // a fifth does not
    puts("threads ok");
    return 0;
}

// the scan as it stood at each of the eight sites before the table (occupied = payload pointer non-null, no lock)
struct OldSlot {
    int device = -1;
    const void *stream = nullptr;
    void *buf = nullptr;
};
OldSlot g_old[16];

int time_case()
{
    static StreamSlots<Two, 16> t;
    static char block[16];
    std::thread([] {}).join();      // a process that has started a thread, as one with the HIP runtime in it has: the C library then locks for real
    for (int i = 0; i < 16; ++i) {
        g_old[i].device = i % 2; g_old[i].stream = stream_of(i / 2); g_old[i].buf = block;
        auto lock = t.lock();
        t.find_or_claim(i % 2, stream_of(i / 2))->buf = block;
    }
    const int reps = 2000000;
    uintptr_t sink = 0;
    double ns[2] = {0, 0};
    for (int pass = 0; pass < 3; ++pass)         // the last pass counts
        for (int which = 0; which < 2; ++which) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int r = 0; r < reps; ++r) {
                const int i = r & 15, dev = i % 2;
                const void *stream = stream_of(i / 2);
                if (which == 0) {
                    OldSlot *slot = nullptr;
                    for (auto &s : g_old)
                        if (s.buf && s.device == dev && s.stream == stream) { slot = &s; break; }
                    sink += (uintptr_t)slot;
                } else {
                    auto lock = t.lock();
                    sink += (uintptr_t)t.find(dev, stream);
                }
                asm volatile("" ::: "memory");
            }
            ns[which] = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / reps;
        }
    printf("find on a warm 16-entry table, keys in turn, ns per call: hand-written scan (no lock) %.1f, StreamSlots lock + find %.1f  [%lx]\n",
           ns[0], ns[1], (unsigned long)(sink & 0xf));
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "table")) return table_cases();
    if (!strcmp(what, "threads")) return thread_case();
    if (!strcmp(what, "time")) return time_case();
    fprintf(stderr, "usage: %s table|threads|time\n", argv[0]);
    return 2;
}
