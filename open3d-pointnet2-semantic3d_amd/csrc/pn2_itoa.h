// pn2_itoa.h -- the arithmetic of the integer formatter (pn2_scene_io.hip): how many characters Python's "%d" prints for an
// int32 and which ones.  Plain integer C++ that a host compiler reads as well, so the same lines that run on the device can be
// checked against snprintf("%d") under the host sanitizers (EXPERIMENTS.md, "scene files").
#pragma once

#if defined(__HIPCC__)
#define PN2_HD __host__ __device__ __forceinline__
#else
#define PN2_HD inline
#endif

// |v| as unsigned: INT32_MIN has no signed negation, 0u - (unsigned)v is exact for every v < 0
PN2_HD unsigned pn2_i32_magnitude(int v) { return v < 0 ? 0u - (unsigned)v : (unsigned)v; }

// decimal digits of m: 1 for 0 .. 9, 10 for 1000000000 .. 4294967295
PN2_HD int pn2_u32_digits(unsigned m) {
    return 1 + (m >= 10u) + (m >= 100u) + (m >= 1000u) + (m >= 10000u) + (m >= 100000u) + (m >= 1000000u) + (m >= 10000000u) +
           (m >= 100000000u) + (m >= 1000000000u);
}

// characters of "%d" % v: a '-' for negatives, no '+', no leading zeros -- 1 to 11
PN2_HD int pn2_i32_chars(int v) { return pn2_u32_digits(pn2_i32_magnitude(v)) + (v < 0); }

// writes those characters through put(position, byte) at positions at .. at + pn2_i32_chars(v) - 1 and returns the position
// after them; the digits are produced from the last one back
template <class Put>
PN2_HD int pn2_i32_emit(int v, int at, Put&& put) {
    unsigned m = pn2_i32_magnitude(v);
    if (v < 0) put(at++, (unsigned char)'-');
    const int nd = pn2_u32_digits(m);
    for (int k = nd - 1; k >= 0; --k) {
        const unsigned q = m / 10u;
        put(at + k, (unsigned char)('0' + (m - q * 10u)));
        m = q;
    }
    return at + nd;
}
