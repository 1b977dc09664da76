// The per-pixel transition of the temporal mask stabiliser (stabilize_ops.hip; definition: include/floodseg_test.h, mask_stabilize;
// DESIGN §3.16).  Plain __host__ __device__ C++ with nothing of HIP in it: the kernels call these functions, and a host program
// (tests/test_stabilize_cpu.py builds tests/stabilize_host_check.cpp) runs them on the CPU.  Integers throughout.
#ifndef FS_STABILIZE_DEFS_H_
#define FS_STABILIZE_DEFS_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define FS_STB_HD __host__ __device__ __forceinline__
#else
#define FS_STB_HD inline
#endif

namespace fs {
namespace stb {

constexpr int MAX_CLASSES = 255, MAX_PERSIST = 255, TRUST_OFF = 256;  // K 1..255, P 1..255, T 0..256 (256: never trusted)
constexpr int MAX_RUN = 255;                                          // the run length saturates here

// ---- the state word: bit 31 valid, bits 0-7 the emitted class e, 8-15 the candidate c, 16-23 the run length r.  0 = no state.
constexpr uint32_t VALID = 1u << 31;
FS_STB_HD uint32_t pack(int e, int c, int r) { return VALID | ((uint32_t)r << 16) | ((uint32_t)c << 8) | (uint32_t)e; }
FS_STB_HD bool valid(uint32_t s) { return (s & VALID) != 0u; }
FS_STB_HD int emitted(uint32_t s) { return (int)(s & 0xffu); }
FS_STB_HD int candidate(uint32_t s) { return (int)((s >> 8) & 0xffu); }
FS_STB_HD int run(uint32_t s) { return (int)((s >> 16) & 0xffu); }

// ---- what a transition is counted as: one byte per counter of counts[f] = (held, switched, seeded, trusted), so that the events of up
// to four pixels add up in one dword without a carry between the bytes (each byte <= 4)
constexpr uint32_t EV_NONE = 0u, EV_HELD = 1u, EV_SWITCHED = 1u << 8, EV_SEEDED = 1u << 16, EV_TRUSTED = 1u << 24;

// is the observation trusted outright?  conf = the pixel's confidence code 0..255, or -1 without a plane; T = 256 is never reached
FS_STB_HD bool trusted(int conf, int T) { return conf >= 0 && conf >= T; }

// One pixel, one frame: prior word s (0 = none), observed class o 0..255, K classes, persistence P, `trust` from trusted().  Returns the
// new state word; *out = the emitted class, *event = the EV_ bits of what happened.
FS_STB_HD uint32_t step(uint32_t s, int o, int K, int P, bool trust, int* out, uint32_t* event) {
    *out = o;
    *event = EV_NONE;
    if (o >= K) return 0u;  // not a class: passed through, and the pixel's history ends
    if (!valid(s)) {
        *event = EV_SEEDED;
        return pack(o, o, 0);
    }
    const int e = emitted(s);
    if (o == e) return pack(e, e, 0);
    if (trust) {
        *event = EV_SWITCHED | EV_TRUSTED;
        return pack(o, o, 0);
    }
    const int r = o == candidate(s) ? (run(s) < MAX_RUN ? run(s) + 1 : MAX_RUN) : 1;
    if (r >= P) {
        *event = EV_SWITCHED;
        return pack(o, o, 0);
    }
    *event = EV_HELD;
    *out = e;
    return pack(e, o, r);
}

}  // namespace stb
}  // namespace fs
#endif  // FS_STABILIZE_DEFS_H_
