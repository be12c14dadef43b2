// pack_common.cuh -- what the device front ends share (state_pack.cuh: Proof-of-State; account_pack.cuh: Proof-of-Account): the cursor over a slice of the
// uploaded bytes, the canonical-form test of a base-field element, and the greedy packer of openmina's `Inputs` writing straight into a record.
// Bincode only; one lane per item; everything in named registers.  Compiles for the host too (tests/fuzz/*_twin.cpp).
#pragma once
#include <cstddef>
#include "fp.cuh"
#include "../../include/mina_verify.h"

namespace mb {

// ------------------------------------------------------------------------------------------------ cursor over [pos, end) of the blob (wire_state.h Cursor)
struct PackCur { const uint8_t *p; uint64_t end, pos; bool ok; };
__device__ __forceinline__ bool pc_take(PackCur &c, uint64_t k) { if (!c.ok || c.end - c.pos < k) { c.ok = false; return false; } return true; }
__device__ __forceinline__ uint64_t pc_ld64(const uint8_t *q) { uint64_t v; __builtin_memcpy(&v, q, 8); return v; }
__device__ __forceinline__ uint32_t pc_ld32(const uint8_t *q) { uint32_t v; __builtin_memcpy(&v, q, 4); return v; }
__device__ __forceinline__ void pc_skip(PackCur &c, uint64_t k) { if (pc_take(c, k)) c.pos += k; }
__device__ __forceinline__ uint64_t pc_u64(PackCur &c) { if (!pc_take(c, 8)) return 0; const uint64_t v = pc_ld64(c.p + c.pos); c.pos += 8; return v; }
__device__ __forceinline__ uint32_t pc_u32(PackCur &c) { if (!pc_take(c, 4)) return 0; const uint32_t v = pc_ld32(c.p + c.pos); c.pos += 4; return v; }
__device__ __forceinline__ uint32_t pc_bool(PackCur &c) { if (!pc_take(c, 1)) return 0; const uint32_t v = c.p[c.pos]; c.pos += 1; if (v > 1) c.ok = false; return v & 1; }
// a u64 length.  The host's `length() > n` test is implied: whatever a length counts takes at least a byte each from the same slice.
__device__ __forceinline__ uint64_t pc_len(PackCur &c) { return pc_u64(c); }
// 32 bytes as four little-endian words (zeros and c.ok = false past the end)
__device__ __forceinline__ void pc_b32(PackCur &c, uint64_t &w0, uint64_t &w1, uint64_t &w2, uint64_t &w3) {
    w0 = w1 = w2 = w3 = 0;
    if (!pc_take(c, 32)) return;
    const uint8_t *q = c.p + c.pos;
    w0 = pc_ld64(q); w1 = pc_ld64(q + 8); w2 = pc_ld64(q + 16); w3 = pc_ld64(q + 24); c.pos += 32;
}
// below the Pallas base modulus (wire_state.h fp_canonical)
__device__ __forceinline__ bool pc_canonical(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
    constexpr uint64_t P3 = 0x4000000000000000ULL, P1 = 0x224698fc094cf91bULL, P0 = 0x992d30ed00000001ULL;      // P2 = 0
    return w3 < P3 || (w3 == P3 && w2 == 0 && (w1 < P1 || (w1 == P1 && w0 < P0)));
}

// ------------------------------------------------------------------------------------------------ openmina `Inputs` packing (wire_state.h Inputs), straight into the record
struct Packer { uint64_t c0, c1, c2, c3; uint32_t nbits, npacked; uint4 *rec; uint32_t base; };      // base: record slot of the first packed element
__device__ __forceinline__ void pk_store(uint4 *rec, uint32_t slot, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
    rec[2 * slot] = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
    rec[2 * slot + 1] = make_uint4((uint32_t)w2, (uint32_t)(w2 >> 32), (uint32_t)w3, (uint32_t)(w3 >> 32));
}
__device__ __forceinline__ void pk_flush(Packer &k) {
    const uint32_t slot = k.base + k.npacked;
    if (slot < MINA_PSTATE_SLOTS) pk_store(k.rec, slot, k.c0, k.c1, k.c2, k.c3);      // past the record: counted, and the input is rejected by its field count
    ++k.npacked;
}
__device__ __forceinline__ void pk_shift_in(Packer &k, uint64_t x, uint32_t b) {        // cur = (cur << b) + x, 1 <= b <= 64
    if (b == 64) { k.c3 = k.c2; k.c2 = k.c1; k.c1 = k.c0; k.c0 = x; }
    else { k.c3 = (k.c3 << b) | (k.c2 >> (64 - b)); k.c2 = (k.c2 << b) | (k.c1 >> (64 - b)); k.c1 = (k.c1 << b) | (k.c0 >> (64 - b)); k.c0 = (k.c0 << b) | x; }
}
__device__ __forceinline__ void pk_packed(Packer &k, uint64_t x, uint32_t b) {
    k.nbits += b;
    if (k.nbits < 255) pk_shift_in(k, x, b);
    else { pk_flush(k); k.c0 = x; k.c1 = k.c2 = k.c3 = 0; k.nbits = b; }
}
// `nb` single-bit chunks (Inputs::bytes_lsb_first): the string is s0..s3 with its first bit on top of s0
__device__ __forceinline__ void pk_bits(Packer &k, uint64_t s0, uint64_t s1, uint64_t s2, uint64_t s3, uint32_t nb) {
    while (nb) {
        const uint32_t room = 254 - k.nbits;
        if (room == 0) { pk_flush(k); k.c0 = k.c1 = k.c2 = k.c3 = 0; k.nbits = 0; continue; }
        uint32_t t = nb < 64 ? nb : 64; if (t > room) t = room;
        uint64_t v;
        if (t == 64) { v = s0; s0 = s1; s1 = s2; s2 = s3; s3 = 0; }
        else { v = s0 >> (64 - t); s0 = (s0 << t) | (s1 >> (64 - t)); s1 = (s1 << t) | (s2 >> (64 - t)); s2 = (s2 << t) | (s3 >> (64 - t)); s3 <<= t; }
        pk_shift_in(k, v, t); k.nbits += t; nb -= t;
    }
}

}  // namespace mb
