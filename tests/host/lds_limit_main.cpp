// Stand-alone check of the (kernel, device) bookkeeping behind pn2_allow_lds (csrc/pn2_device_set.h), meant to be built with
// -fsanitize=thread (tests/test_lds_limit_cpu.py).  Several threads hammer ONE set.  Ordinal d < 64 is marked by thread
// d % kThreads only, after it has written payload[d] with a plain store -- the stand-in for the attribute call whose effect a
// thread that sees "done" relies on; every thread reads payload[d] once it sees d done, so a missing acquire / release pair
// is a data race the sanitizer reports.  Exit status 0 and "ok" on success.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../open3d-pointnet2-semantic3d_amd/csrc/pn2_device_set.h"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

namespace {
constexpr int kThreads = 8, kPasses = 200;
constexpr int kUncached[] = {64, 65, 1000, INT_MAX, -1, -64, INT_MIN};  // always "not yet done": the step is repeated

Pn2DeviceSet set;
int payload[64];

// every ordinal seen done stays done, and what its marker wrote before is visible
void observe(bool* seen) {
    for (int d = 0; d < 64; ++d) {
        const bool now = set.done(d);
        CHECK(now || !seen[d]);
        if (now) CHECK(payload[d] == d + 1);
        seen[d] = now;
    }
    for (int d : kUncached) CHECK(!set.done(d));
}

void worker(int t) {
    bool seen[64] = {};
    for (int d = t; d < 64; d += kThreads) {
        for (int p = 0; p < kPasses; ++p) observe(seen);
        CHECK(!set.done(d));  // nobody else marks d
        payload[d] = d + 1;
        set.mark(d);
        CHECK(set.done(d));
        const uint64_t before = set.bits.load();
        set.mark(d);  // idempotent: marks nothing new (other threads may add THEIR bits meanwhile, never remove one)
        CHECK((set.bits.load() & before) == before && set.done(d));
        for (int u : kUncached) set.mark(u);
    }
    for (int p = 0; p < kPasses; ++p) observe(seen);
}
}  // namespace

int main() {
    for (int d = 0; d < 64; ++d) CHECK(!set.done(d));
    for (int d : kUncached) {
        set.mark(d);
        CHECK(!set.done(d) && set.bits.load() == 0);  // marking an uncached ordinal sets no bit
    }
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; ++t) th.emplace_back(worker, t);
    for (auto& x : th) x.join();
    CHECK(set.bits.load() == ~uint64_t(0));
    for (int d = 0; d < 64; ++d) CHECK(set.done(d));
    for (int d : kUncached) CHECK(!set.done(d));
    Pn2DeviceSet one;  // single-threaded: marking 63 marks 63 alone
    one.mark(63);
    one.mark(63);
    CHECK(one.bits.load() == uint64_t(1) << 63 && one.done(63) && !one.done(62) && !one.done(0));
    std::puts("ok");
    return 0;
}
