// pn2_device_set.h -- the devices of this process on which an idempotent per-device step has been done.  Plain C++ (no HIP
// headers): tests/host/lds_limit_main.cpp exercises this very struct under ThreadSanitizer.
#pragma once
#include <atomic>
#include <cstdint>

// A set of device ordinals 0..63, safe from any number of host threads.  An ordinal outside that range is never a member: its
// step is repeated on every call, which is correct for an idempotent step, only uncached.
struct Pn2DeviceSet {
    std::atomic<uint64_t> bits{0};

    static constexpr bool cached(int dev) { return dev >= 0 && dev < 64; }
    // acquire: a thread that sees the bit also sees what the marking thread did before mark()
    bool done(int dev) const { return cached(dev) && ((bits.load(std::memory_order_acquire) >> dev) & 1u) != 0; }
    // call only after the step has succeeded on `dev`
    void mark(int dev) {
        if (cached(dev)) bits.fetch_or(uint64_t(1) << dev, std::memory_order_release);
    }
};
