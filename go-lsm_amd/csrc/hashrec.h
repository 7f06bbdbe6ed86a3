// hashrec.h — the 16-byte hash record of a key (gfx950).
//
// What the .sst builder (encode.hip) and the read path (lookup.hip) share: a
// key's sum256 digest reduced, for one filter size m, to what rebuilds its
// k <= 16 bloom locations by additions.  location(j) = h[j%2] +
// j*h[2 + ((j + j%2) % 4)/2] (bloom.go:133-136): class c = j%4 is an
// arithmetic progression, so the record holds the residues mod m of the four
// class bases and of the class step of classes 0 and 3, plus the carry bit of
// each 64-bit step and the two carries that rebuild the other class step from
// the class bases.
//
// Record (m <= 2^21: a two-slice filter is at most 2 * 819,200 bits), dword c
// of 4: bits 0-20 the residue of class c's base, bits 21-23 the carries of
// its three steps, bits 24-31 byte c of X = res(4 h2) | a << 21 | b << 22,
// where T = 2 h3 mod 2^64, a = carry of h0 + T (class 2's base) and b = the
// top bit of T: res(T) = res(base2) - res(base0) + a (2^64 mod m), and
// res(4 h3) = 2 res(T) - b (2^64 mod m), all mod m.  (24 bytes per key, the
// round-4 record, were read twice and written once: 1.28x the algorithmic
// traffic of config 3.)
#pragma once

#include "common.h"
#include "murmur.h"

namespace lsm {

constexpr uint32_t kHashRecDwords = 4;
constexpr uint32_t kHashRecBits = 21;  // residue bits: m <= 2^21
constexpr uint32_t kSplitMaxK = 16;  // three carries per class fit the record

// floor((2^64-1)/m), mod_barrett's and mod_small's reciprocal (host side)
inline uint64_t barrett_recip(uint64_t m) { return ~0ull / m; }

// The 16-byte hash record of a key from its sum256 digest (layout above).
__device__ __forceinline__ void store_hash_rec(const uint64_t h[4], uint32_t m, uint32_t rl,
                                               uint32_t rh, uint32_t *rec) {
    const uint64_t T = h[3] << 1;
    const uint64_t loc[4] = {h[0], h[1] + h[3], h[0] + T, h[1] + h[2] + (h[2] << 1)};
    const uint64_t st2 = h[2] << 2, st3 = h[3] << 2;
    uint32_t r[4];
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) {
        uint32_t cy = 0;  // bit n: the step to location 4(n + 1) + c carries
        const uint64_t st = (c == 0 || c == 3) ? st2 : st3;
        uint64_t l = loc[c];
#pragma unroll
        for (uint32_t n = 0; n < 3; n++) {
            uint64_t nl;
            cy |= (uint32_t)__builtin_add_overflow(l, st, &nl) << n;
            l = nl;
        }
        r[c] = mod_small(loc[c], m, rl, rh) | cy << kHashRecBits;
    }
    const uint32_t a = loc[2] < h[0];  // h0 + T wrapped
    const uint32_t x = mod_small(st2, m, rl, rh) | a << 21 | (uint32_t)(T >> 63) << 22;
#pragma unroll
    for (uint32_t c = 0; c < 3; c++) r[c] |= ((x >> (8 * c)) & 0xFFu) << 24;
    *(gptr_t<u32x4>)gbl(rec) = u32x4{r[0], r[1], r[2], r[3]};
}

// A hash record (store_hash_rec) unpacked: the residues of the four class
// bases (location c of class c) and each class's three steps, the carried
// ones already less 2^64 mod m: location 4(n + 1) + c = r[c] + st[c][n] mod m.
struct HashRecSteps {
    uint32_t r[4];
    uint32_t st[4][3];
};

__device__ __forceinline__ HashRecSteps unpack_hash_rec(const u32x4 x, uint32_t m, uint32_t c64) {
    constexpr uint32_t kRes = (1u << kHashRecBits) - 1;
    const uint32_t raw[4] = {x.x, x.y, x.z, x.w};
    HashRecSteps H;
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) H.r[c] = raw[c] & kRes;
    // X = res(4 h2) | a << 21 | b << 22 from the top bytes of dwords 0-2
    const uint32_t X = __builtin_amdgcn_perm(raw[1], raw[0], 0x0c0c0703u) |
                       (raw[2] >> 24) << 16;
    const uint32_t d2 = X & kRes;
    // res(T) = res(base2) - res(base0) + a c64, res(4 h3) = 2 res(T) - b c64 (mod m)
    uint32_t rt = H.r[2] - H.r[0];
    rt = min(rt, rt + m);
    rt = (X >> 21) & 1 ? rt + c64 : rt;
    rt = min(rt, rt - m);
    uint32_t d3 = rt << 1;
    d3 = min(d3, d3 - m);
    d3 = (X >> 22) & 1 ? d3 - c64 : d3;
    d3 = min(d3, d3 + m);
    // the steps less 2^64 mod m, for a step whose 64-bit add wraps
    const uint32_t t2 = d2 - c64, t3 = d3 - c64;
    const uint32_t w2 = min(t2, t2 + m), w3 = min(t3, t3 + m);
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) {
        const bool a2 = c == 0 || c == 3;
#pragma unroll
        for (uint32_t n = 0; n < 3; n++) {
            // all-ones where the step from location 4n + c carries (bit
            // 21 + n of dword c), then one bitfield insert (the compiler's
            // and / compare / cndmask form is three VALU)
            const uint32_t msk = (uint32_t)__builtin_amdgcn_sbfe((int)raw[c], kHashRecBits + n, 1);
            uint32_t v;
            __asm__("v_bfi_b32 %0, %1, %2, %3" : "=v"(v) : "v"(msk), "v"(a2 ? w2 : w3), "v"(a2 ? d2 : d3));
            H.st[c][n] = v;
        }
    }
    return H;
}

}  // namespace lsm
