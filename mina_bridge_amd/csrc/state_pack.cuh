// state_pack.cuh -- the opt-in device front end of a Proof-of-State job (mina_protocol_state_pack_dev, mina_state_frontend_dev; MINA_VERIFY_PACK_ON_DEVICE):
// serialized protocol states in, records + field counts + the `precheck` byte out.
//
// A streaming twin of the host reader (wire_state.h read_protocol_state<Bincode> + protocol_state_body_inputs + api_wire.hip mb_pack_protocol_state), bincode only --
// the form inside `MinaStateProof`, the only one a verifier is handed.  The host path stays the checker: every output is bit-identical to it for every input
// (tests/test_state_pack_gpu.py), malformed ones included.
//
// One lane per state, ONE walk in wire order, nothing in scratch:
//   * the 38 whole field elements of `to_input` have fixed slots in the record: each goes from the wire to its slot as it is read, checked for canonical form on the
//     way (previous_state_hash -> slot 0 and the staged-ledger hash, which only feeds SHA-256, are checked the same);
//   * the packed chunks of `to_input` come in wire order too, but for three places, so the greedy packer (four u64 + a bit count) runs as the scalars arrive:
//     `success` is read before `account_update_index` and packed after it; the two epoch records' total_currency / epoch_length and the flags behind them are held
//     in a dozen named registers until the block-creator keys are through; body.constants are read as five words and packed in `to_input` order;
//   * the three bit strings (SHA-256 digest, body_reference, the 253 bits of the VRF output) are four u64 with the first bit on top (a bit-reversed little-endian
//     load), consumed by shifting: variable shifts, static indices;
//   * SHA-256 of the 96-byte staged-ledger message is two blocks with a 16-word rolling schedule, fully unrolled.
// A proof's 17 states are consecutive and only parsing finds where one ends: pstate_split_kernel walks the variable-length points (four string lengths, two
// failure-status tables, the density vector) of each, one lane per proof; pstate_precheck_kernel then forms FORMAT / LEDGER / CONSENSUS with consensus.cuh.
#pragma once
#include "pack_common.cuh"
#include "consensus.cuh"

namespace mb {

// `failure_status_tbl`: rows of constructor tags, not hashed (empty in every block state)
__device__ __forceinline__ void pc_table(PackCur &c) {
    const uint64_t rows = pc_len(c);
    for (uint64_t i = 0; i < rows && c.ok; ++i) { const uint64_t m = pc_len(c); if (m > (c.end - c.pos) / 4) c.ok = false; else c.pos += 4 * m; }
}
// a string that is 32 bytes in every well-formed state: the position of its bytes (any other length is rejected)
__device__ __forceinline__ uint64_t pc_str32(PackCur &c) { if (pc_len(c) != 32) c.ok = false; const uint64_t at = c.pos; pc_skip(c, 32); return at; }

// fixed byte counts of the bincode form between the variable-length points
constexpr uint32_t PW_SIGNED = 12;                                        // u64 magnitude + u32 sign tag
constexpr uint32_t PW_LOCAL_HEAD = 4 * 32 + 2 * PW_SIGNED + 32 + 1 + 4;   // local state up to its failure_status_tbl
constexpr uint32_t PW_REG_HEAD = 5 * 32 + PW_LOCAL_HEAD;                  // registers up to that table; `will_succeed` (1) follows it
constexpr uint32_t PW_AFTER_REGS = 2 * 32 + PW_SIGNED + 2 * (32 + PW_SIGNED) + 8;      // connecting ledgers, supply increase, fee excess, timestamp
constexpr uint32_t PW_EPOCH = 32 + 8 + 3 * 32 + 4;
constexpr uint32_t PW_TAIL = 8 + 8 + 4 + 8 + 2 * PW_EPOCH + 1 + 3 * 33 + 1 + 5 * 4 + 8;   // total_currency .. genesis_state_timestamp
constexpr uint32_t PSTATE_REC_BYTES = MINA_PSTATE_SLOTS * 32;
constexpr uint32_t PW_WHOLE = 38;                                         // whole field elements of the body: record slots 1 .. 38, the packed ones follow

// the variable-length points only: where a state that starts at c.pos ends
__device__ __forceinline__ void pstate_skip(PackCur &c) {
    pc_skip(c, 3 * 32); (void)pc_str32(c); (void)pc_str32(c); pc_skip(c, 2 * 32);
    for (int r = 0; r < 2; ++r) { pc_skip(c, PW_REG_HEAD); pc_table(c); pc_skip(c, 1); }
    pc_skip(c, PW_AFTER_REGS); (void)pc_str32(c); pc_skip(c, 12);
    const uint64_t m = pc_len(c);
    if (m > 64) c.ok = false; else pc_skip(c, 4 * m);
    (void)pc_str32(c); pc_skip(c, PW_TAIL);
}

// ------------------------------------------------------------------------------------------------ SHA-256, one block, 16-word rolling schedule
__device__ __forceinline__ uint32_t sha_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
__device__ __forceinline__ void sha256_block(uint32_t (&h)[8], uint32_t (&w)[16]) {
    constexpr uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
        0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
        0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        if (i >= 16) {
            const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
            w[i & 15] += (sha_rotr(x, 7) ^ sha_rotr(x, 18) ^ (x >> 3)) + w[(i + 9) & 15] + (sha_rotr(y, 17) ^ sha_rotr(y, 19) ^ (y >> 10));
        }
        const uint32_t t1 = hh + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
        const uint32_t t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
__device__ __forceinline__ uint32_t pk_bswap(uint32_t x) { return __builtin_bswap32(x); }
// digest word pair -> 64 bits of the string bytes_lsb_first reads: byte order kept, every byte's bits reversed
__device__ __forceinline__ uint64_t sha_bits(uint32_t hi, uint32_t lo) { return ((uint64_t)pk_bswap(__brev(hi)) << 32) | pk_bswap(__brev(lo)); }

// ------------------------------------------------------------------------------------------------ BLAKE2b-256 of a 32-byte message (RFC 7693), fully unrolled
__device__ __forceinline__ uint64_t b2p_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
__device__ __forceinline__ void blake2b256_of32(uint64_t m0, uint64_t m1, uint64_t m2, uint64_t m3, uint64_t (&out)[4]) {
    constexpr uint64_t iv[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    constexpr uint8_t sigma[10][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
    uint64_t m[16] = {m0, m1, m2, m3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, v[16];
    const uint64_t h0 = iv[0] ^ 0x01010000ULL ^ 32u;          // digest length 32, fanout 1, depth 1
    v[0] = h0;
#pragma unroll
    for (int i = 1; i < 8; ++i) v[i] = iv[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i + 8] = iv[i];
    v[12] ^= 32u; v[14] = ~v[14];
#pragma unroll
    for (int r = 0; r < 12; ++r) {
#define MB_B2PG(a, b, c, d, x, y)                                                        \
    v[a] = v[a] + v[b] + (x); v[d] = b2p_rotr(v[d] ^ v[a], 32); v[c] = v[c] + v[d];      \
    v[b] = b2p_rotr(v[b] ^ v[c], 24); v[a] = v[a] + v[b] + (y);                          \
    v[d] = b2p_rotr(v[d] ^ v[a], 16); v[c] = v[c] + v[d]; v[b] = b2p_rotr(v[b] ^ v[c], 63);
        MB_B2PG(0, 4, 8, 12, m[sigma[r % 10][0]], m[sigma[r % 10][1]]) MB_B2PG(1, 5, 9, 13, m[sigma[r % 10][2]], m[sigma[r % 10][3]])
        MB_B2PG(2, 6, 10, 14, m[sigma[r % 10][4]], m[sigma[r % 10][5]]) MB_B2PG(3, 7, 11, 15, m[sigma[r % 10][6]], m[sigma[r % 10][7]])
        MB_B2PG(0, 5, 10, 15, m[sigma[r % 10][8]], m[sigma[r % 10][9]]) MB_B2PG(1, 6, 11, 12, m[sigma[r % 10][10]], m[sigma[r % 10][11]])
        MB_B2PG(2, 7, 8, 13, m[sigma[r % 10][12]], m[sigma[r % 10][13]]) MB_B2PG(3, 4, 9, 14, m[sigma[r % 10][14]], m[sigma[r % 10][15]])
#undef MB_B2PG
    }
    out[0] = h0 ^ v[0] ^ v[8]; out[1] = iv[1] ^ v[1] ^ v[9]; out[2] = iv[2] ^ v[2] ^ v[10]; out[3] = iv[3] ^ v[3] ^ v[11];
}

// ------------------------------------------------------------------------------------------------ one state
// mina_protocol_state_info as u32 words (api_wire.hip info_from_state)
enum : uint32_t { PI_PREV = 0, PI_GENESIS = 8, PI_SNARKED = 16, PI_NF = 24, PI_K, PI_SLOTS_PER_EPOCH, PI_SLOTS_PER_SUB_WINDOW, PI_SUB_WINDOWS, PI_GRACE, PI_DELTA,
                  PI_LENGTH, PI_EPOCH, PI_SLOT, PI_MIN_DENSITY, PI_DENSITIES, PI_STAKING_LOCK = PI_DENSITIES + MINA_MAX_SUB_WINDOWS, PI_NEXT_LOCK = PI_STAKING_LOCK + 8,
                  PI_VRF = PI_NEXT_LOCK + 8, PI_STATE_HASH = PI_VRF + 8, PI_WORDS = PI_STATE_HASH + 8 };
static_assert(sizeof(mina_protocol_state_info) == PI_WORDS * 4, "mina_protocol_state_info layout");
static_assert(offsetof(mina_protocol_state_info, consensus) == PI_LENGTH * 4 && offsetof(mina_protocol_state_info, n_body_fields) == PI_NF * 4, "mina_protocol_state_info layout");
static_assert(offsetof(mina_consensus_state, staking_lock_checkpoint) == (PI_STAKING_LOCK - PI_LENGTH) * 4 && offsetof(mina_consensus_state, state_hash) == (PI_STATE_HASH - PI_LENGTH) * 4, "mina_consensus_state layout");

struct PackSink { uint4 *rec; uint32_t *info; };
__device__ __forceinline__ void pi_put(uint32_t *info, uint32_t at, uint32_t v) { if (info) info[at] = v; }
__device__ __forceinline__ void pi_put32(uint32_t *info, uint32_t at, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
    if (!info) return;
    info[at] = (uint32_t)w0; info[at + 1] = (uint32_t)(w0 >> 32); info[at + 2] = (uint32_t)w1; info[at + 3] = (uint32_t)(w1 >> 32);
    info[at + 4] = (uint32_t)w2; info[at + 5] = (uint32_t)(w2 >> 32); info[at + 6] = (uint32_t)w3; info[at + 7] = (uint32_t)(w3 >> 32);
}
// a base-field element: canonical (pc_canonical), and to record slot `slot` (>= 0) / info words `at` (>= 0)
__device__ __forceinline__ void pc_field(PackCur &c, const PackSink &s, int slot, int at, uint64_t &w0, uint64_t &w1, uint64_t &w2, uint64_t &w3) {
    pc_b32(c, w0, w1, w2, w3);
    if (!pc_canonical(w0, w1, w2, w3)) c.ok = false;
    if (slot >= 0) pk_store(s.rec, (uint32_t)slot, w0, w1, w2, w3);
    if (at >= 0) pi_put32(s.info, (uint32_t)at, w0, w1, w2, w3);
}
__device__ __forceinline__ void pc_field(PackCur &c, const PackSink &s, int slot, int at = -1) { uint64_t a, b, d, e; pc_field(c, s, slot, at, a, b, d, e); }
// Signed amount: magnitude, then the bit "is positive"
__device__ __forceinline__ void pc_signed(PackCur &c, Packer &k) {
    const uint64_t mag = pc_u64(c); const uint32_t sgn = pc_u32(c); if (sgn > 1) c.ok = false;
    pk_packed(k, mag, 64); pk_packed(k, sgn == 0 ? 1 : 0, 1);
}
// registers: five ledger / pending-coinbase hashes and the local state; whole fields to slots base .. base + 9
__device__ __forceinline__ void pc_registers(PackCur &c, const PackSink &s, Packer &k, int base, int snarked_at) {
    pc_field(c, s, base, snarked_at);
    for (int i = 1; i < 9; ++i) pc_field(c, s, base + i);                    // second pass ledger, three pending-coinbase stacks; stack frame, call stack, two commitments
    pc_signed(c, k); pc_signed(c, k);                                        // excess, supply increase
    pc_field(c, s, base + 9);                                                // ledger
    const uint32_t success = pc_bool(c);
    pk_packed(k, pc_u32(c), 32);                                             // account_update_index
    pk_packed(k, success, 1);
    pc_table(c);
    pk_packed(k, pc_bool(c), 1);                                             // will_succeed
}
// epoch data: ledger hash, total currency, seed, start / lock checkpoint, epoch length; whole fields to base .. base + 3 in `to_input` order
__device__ __forceinline__ void pc_epoch(PackCur &c, const PackSink &s, int base, int lock_at, uint64_t &total_currency, uint32_t &epoch_length) {
    pc_field(c, s, base + 2); total_currency = pc_u64(c); pc_field(c, s, base); pc_field(c, s, base + 1); pc_field(c, s, base + 3, lock_at); epoch_length = pc_u32(c);
}

// The state in [c.pos, c.end) -> the record at s.rec (16-byte aligned), the info words at s.info (or null).  Returns the body's field count; c.ok = false: rejected
// (record and info then hold rubbish: the caller zeroes the record).  c.pos ends behind the state.
__device__ __forceinline__ uint32_t pstate_pack_one(PackCur &c, const PackSink &s) {
    Packer k{0, 0, 0, 0, 0, 0, s.rec, 1 + PW_WHOLE};
    pc_field(c, s, 0, PI_PREV);                                              // previous_state_hash
    pc_field(c, s, 1, PI_GENESIS);                                           // genesis_state_hash
    {   // Staged_ledger_hash.Non_snark: SHA-256(ledger hash as 32 big-endian bytes || aux_hash || pending_coinbase_aux), bit by bit
        uint64_t l0, l1, l2, l3, a0, a1, a2, a3, b0, b1, b2, b3;
        pc_field(c, s, -1, -1, l0, l1, l2, l3);
        if (pc_len(c) != 32) c.ok = false;
        pc_b32(c, a0, a1, a2, a3);
        if (pc_len(c) != 32) c.ok = false;
        pc_b32(c, b0, b1, b2, b3);
        uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
        uint32_t w[16] = {(uint32_t)(l3 >> 32), (uint32_t)l3, (uint32_t)(l2 >> 32), (uint32_t)l2, (uint32_t)(l1 >> 32), (uint32_t)l1, (uint32_t)(l0 >> 32), (uint32_t)l0,
                          pk_bswap((uint32_t)a0), pk_bswap((uint32_t)(a0 >> 32)), pk_bswap((uint32_t)a1), pk_bswap((uint32_t)(a1 >> 32)),
                          pk_bswap((uint32_t)a2), pk_bswap((uint32_t)(a2 >> 32)), pk_bswap((uint32_t)a3), pk_bswap((uint32_t)(a3 >> 32))};
        sha256_block(h, w);
        uint32_t w2[16] = {pk_bswap((uint32_t)b0), pk_bswap((uint32_t)(b0 >> 32)), pk_bswap((uint32_t)b1), pk_bswap((uint32_t)(b1 >> 32)),
                           pk_bswap((uint32_t)b2), pk_bswap((uint32_t)(b2 >> 32)), pk_bswap((uint32_t)b3), pk_bswap((uint32_t)(b3 >> 32)),
                           0x80000000u, 0, 0, 0, 0, 0, 0, 96 * 8};
        sha256_block(h, w2);
        pk_bits(k, sha_bits(h[0], h[1]), sha_bits(h[2], h[3]), sha_bits(h[4], h[5]), sha_bits(h[6], h[7]), 256);
    }
    pc_field(c, s, 2); pc_field(c, s, 3);                                    // pending_coinbase_hash, genesis_ledger_hash
    pc_registers(c, s, k, 4, -1);                                            // ledger_proof_statement.source
    pc_registers(c, s, k, 14, PI_SNARKED);                                   // .target: its first_pass_ledger is `snarked_ledger_hash`
    pc_field(c, s, 24); pc_field(c, s, 25); pc_signed(c, k);                 // connecting ledgers, supply increase
    pc_field(c, s, 26); pc_signed(c, k); pc_field(c, s, 27); pc_signed(c, k);      // fee excess: token, amount; token, amount            (sok_digest: unit, no bytes)
    pk_packed(k, pc_u64(c), 64);                                             // timestamp
    {   // body_reference: 256 bits
        uint64_t r0, r1, r2, r3;
        if (pc_len(c) != 32) c.ok = false;
        pc_b32(c, r0, r1, r2, r3);
        pk_bits(k, __brevll(r0), __brevll(r1), __brevll(r2), __brevll(r3), 256);
    }
    { uint32_t v = pc_u32(c); pi_put(s.info, PI_LENGTH, v); pk_packed(k, v, 32); }
    { uint32_t v = pc_u32(c); pi_put(s.info, PI_EPOCH, v); pk_packed(k, v, 32); }
    { uint32_t v = pc_u32(c); pi_put(s.info, PI_MIN_DENSITY, v); pk_packed(k, v, 32); }
    {
        uint64_t m = pc_len(c); if (m > 64) { c.ok = false; m = 0; }
        pi_put(s.info, PI_SUB_WINDOWS, (uint32_t)m);
        for (uint32_t i = 0; i < (uint32_t)m && c.ok; ++i) { const uint32_t d = pc_u32(c); pk_packed(k, d, 32); if (i < MINA_MAX_SUB_WINDOWS) pi_put(s.info, PI_DENSITIES + i, d); }
        for (uint32_t i = (uint32_t)m; i < MINA_MAX_SUB_WINDOWS; ++i) pi_put(s.info, PI_DENSITIES + i, 0);
    }
    {   // last_vrf_output, truncated to 253 bits (the info keeps the string itself)
        uint64_t r0, r1, r2, r3;
        if (pc_len(c) != 32) c.ok = false;
        pc_b32(c, r0, r1, r2, r3);
        pi_put32(s.info, PI_VRF, r0, r1, r2, r3);
        pk_bits(k, __brevll(r0), __brevll(r1), __brevll(r2), __brevll(r3), 253);
    }
    pk_packed(k, pc_u64(c), 64);                                             // total_currency
    { if (pc_u32(c) != 0) c.ok = false; uint32_t v = pc_u32(c); pi_put(s.info, PI_SLOT, v); pk_packed(k, v, 32); }      // curr_global_slot.slot_number: Since_hard_fork of u32
    pk_packed(k, pc_u32(c), 32);                                             // .slots_per_epoch
    { if (pc_u32(c) != 0) c.ok = false; pk_packed(k, pc_u32(c), 32); }       // global_slot_since_genesis: Since_genesis of u32
    uint64_t st_tc, nx_tc; uint32_t st_len, nx_len;
    pc_epoch(c, s, 28, PI_STAKING_LOCK, st_tc, st_len); pc_epoch(c, s, 32, PI_NEXT_LOCK, nx_tc, nx_len);
    const uint32_t has_ancestor = pc_bool(c);
    pc_field(c, s, 36); const uint32_t odd0 = pc_bool(c);                    // block_stake_winner, block_creator, coinbase_receiver
    pc_field(c, s, 37); const uint32_t odd1 = pc_bool(c);
    pc_field(c, s, 38); const uint32_t odd2 = pc_bool(c);
    const uint32_t supercharge = pc_bool(c);
    pk_packed(k, has_ancestor, 1); pk_packed(k, supercharge, 1);
    pk_packed(k, st_len, 32); pk_packed(k, st_tc, 64); pk_packed(k, nx_len, 32); pk_packed(k, nx_tc, 64);
    pk_packed(k, odd0, 1); pk_packed(k, odd1, 1); pk_packed(k, odd2, 1);
    const uint32_t kk = pc_u32(c), slots_per_epoch = pc_u32(c), slots_per_sub_window = pc_u32(c), grace = pc_u32(c), delta = pc_u32(c);
    pk_packed(k, kk, 32); pk_packed(k, delta, 32); pk_packed(k, slots_per_epoch, 32); pk_packed(k, slots_per_sub_window, 32); pk_packed(k, grace, 32);
    pk_packed(k, pc_u64(c), 64);                                             // genesis_state_timestamp
    if (k.nbits > 0) pk_flush(k);
    const uint32_t nf = PW_WHOLE + k.npacked;
    if (nf > MINA_PSTATE_SLOTS - 1) c.ok = false;                            // more elements than a record holds (mb_pack_protocol_state)
    pi_put(s.info, PI_NF, nf); pi_put(s.info, PI_K, kk); pi_put(s.info, PI_SLOTS_PER_EPOCH, slots_per_epoch); pi_put(s.info, PI_SLOTS_PER_SUB_WINDOW, slots_per_sub_window);
    pi_put(s.info, PI_GRACE, grace); pi_put(s.info, PI_DELTA, delta);
    if (s.info) for (uint32_t i = 0; i < 8; ++i) s.info[PI_STATE_HASH + i] = 0;
    return nf;
}

// ------------------------------------------------------------------------------------------------ kernels
// One lane per state.  The state is bytes [off[i], off[i] + len[i]) of the blob and must fill them exactly; a slice that reaches past the blob is status 0.
// info_pairs = 0: info[i] for every state (or none: info == null); 1: only the candidate tip and the bridge tip of each proof (states 15 and 16 of 17), as entries
// 2 b and 2 b + 1 -- what pstate_precheck_kernel reads.  A rejected state leaves a zeroed record and field count 0.
__device__ __forceinline__ void pstate_pack_entry(uint32_t i, const uint8_t *__restrict__ blob, uint64_t blob_len, const uint64_t *__restrict__ off, const uint32_t *__restrict__ len,
                                                  uint4 *__restrict__ records, uint32_t *__restrict__ nfields, uint32_t *__restrict__ info, uint32_t info_pairs, uint8_t *__restrict__ status) {
    uint4 *rec = records + (size_t)i * (PSTATE_REC_BYTES / 16);
    uint32_t *inf = nullptr;
    if (info) {
        if (!info_pairs) inf = info + (size_t)i * PI_WORDS;
        else { const uint32_t b = i / MINA_STATES_PER_PROOF, r = i % MINA_STATES_PER_PROOF; if (r >= MINA_STATES_PER_PROOF - 2) inf = info + ((size_t)2 * b + (r - (MINA_STATES_PER_PROOF - 2))) * PI_WORDS; }
    }
    const uint64_t o = off[i], l = len[i];
    bool ok = o <= blob_len && l <= blob_len - o;
    uint32_t nf = 0;
    if (ok) {
        PackCur c{blob, o + l, o, true};
        nf = pstate_pack_one(c, PackSink{rec, inf});
        ok = c.ok && c.pos == c.end;
    }
    if (ok) { for (uint32_t s = 2 * (1 + nf); s < PSTATE_REC_BYTES / 16; ++s) rec[s] = make_uint4(0, 0, 0, 0); }
    else { nf = 0; for (uint32_t s = 0; s < PSTATE_REC_BYTES / 16; ++s) rec[s] = make_uint4(0, 0, 0, 0); }
    nfields[i] = nf; status[i] = ok ? 1 : 0;
}
__global__ void __launch_bounds__(256)
pstate_pack_kernel(uint32_t n, const uint8_t *__restrict__ blob, uint64_t blob_len, const uint64_t *__restrict__ off, const uint32_t *__restrict__ len,
                   uint4 *__restrict__ records, uint32_t *__restrict__ nfields, uint32_t *__restrict__ info, uint32_t info_pairs, uint8_t *__restrict__ status) { mb_wave_prio();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) pstate_pack_entry(i, blob, blob_len, off, len, records, nfields, info, info_pairs, status);
}

// One lane per proof: where its 17 consecutive states begin.  begin[b] .. end[b] of the blob hold them; off / len [b * 17 + i] come out as pstate_pack_kernel reads
// them.  A proof whose states do not end at end[b] (or whose variable-length points run out of it) has split_ok 0 and slices past the blob.
__device__ __forceinline__ void pstate_split_entry(uint32_t b, const uint8_t *__restrict__ blob, uint64_t blob_len, const uint64_t *__restrict__ begin, const uint64_t *__restrict__ end,
                                                   uint64_t *__restrict__ off, uint32_t *__restrict__ len, uint8_t *__restrict__ split_ok) {
    const uint64_t lo = begin[b], hi = end[b];
    PackCur c{blob, hi, lo, lo <= hi && hi <= blob_len};
    for (uint32_t i = 0; i < MINA_STATES_PER_PROOF; ++i) {
        const uint64_t at = c.pos;
        pstate_skip(c);
        const bool ok = c.ok && c.pos - at <= 0xffffffffu;
        off[(size_t)b * MINA_STATES_PER_PROOF + i] = ok ? at : ~0ull;
        len[(size_t)b * MINA_STATES_PER_PROOF + i] = ok ? (uint32_t)(c.pos - at) : 0;
        if (!ok) c.ok = false;
    }
    split_ok[b] = c.ok && c.pos == hi ? 1 : 0;
}
__global__ void __launch_bounds__(256)
pstate_split_kernel(uint32_t batch, const uint8_t *__restrict__ blob, uint64_t blob_len, const uint64_t *__restrict__ begin, const uint64_t *__restrict__ end,
                    uint64_t *__restrict__ off, uint32_t *__restrict__ len, uint8_t *__restrict__ split_ok) { mb_wave_prio();
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) pstate_split_entry(b, blob, blob_len, begin, end, off, len, split_ok);
}

// One lane per proof, after the two above: FORMAT = every state parsed and the last one ended at the proof's end; LEDGER = the public input's 16 ledger hashes are
// the snarked ledger hashes of states 0 .. 15 (record slot 14); CONSENSUS = the candidate tip (state 15) is selected over the bridge tip (state 16), parameters
// from state 15, tie-breaks by Blake2b-256 of the VRF output and by the expected state hashes -- api_verify.hip parse_states_half.  precheck = LEDGER and
// CONSENSUS and the caller's byte.  `info` is the pair array of pstate_pack_kernel; the VRF digests replace the strings in it.  fmt[b] in: split_ok; out: FORMAT.
__device__ __forceinline__ void pstate_precheck_entry(uint32_t b, const uint4 *__restrict__ records, const uint8_t *__restrict__ status, uint32_t *info, const uint8_t *expected_hashes,
                                                      const uint64_t *__restrict__ ledger_hashes, const uint8_t *__restrict__ and_in, uint8_t *fmt, uint8_t *__restrict__ precheck, uint32_t *__restrict__ masks) {
    bool format = fmt[b] != 0;
    for (uint32_t i = 0; i < MINA_STATES_PER_PROOF; ++i) format = format && status[(size_t)b * MINA_STATES_PER_PROOF + i] != 0;
    bool ledger = false, consensus = false;
    if (format) {
        ledger = true;
        for (uint32_t i = 0; i < 16; ++i) {
            const uint4 *r = records + ((size_t)b * MINA_STATES_PER_PROOF + i) * (PSTATE_REC_BYTES / 16) + 2 * 14;
            const uint64_t *want = ledger_hashes + ((size_t)b * 16 + i) * 4;
            const uint4 x = r[0], y = r[1];
            ledger = ledger && want[0] == (((uint64_t)x.y << 32) | x.x) && want[1] == (((uint64_t)x.w << 32) | x.z) && want[2] == (((uint64_t)y.y << 32) | y.x) && want[3] == (((uint64_t)y.w << 32) | y.z);
        }
        uint32_t *ic = info + (size_t)2 * b * PI_WORDS, *it = ic + PI_WORDS;      // candidate tip, bridge tip
        for (int j = 0; j < 2; ++j) {
            uint32_t *q = (j ? it : ic) + PI_VRF;
            uint64_t d[4];
            blake2b256_of32(((uint64_t)q[1] << 32) | q[0], ((uint64_t)q[3] << 32) | q[2], ((uint64_t)q[5] << 32) | q[4], ((uint64_t)q[7] << 32) | q[6], d);
            for (int t = 0; t < 4; ++t) { q[2 * t] = (uint32_t)d[t]; q[2 * t + 1] = (uint32_t)(d[t] >> 32); }
        }
        const mina_consensus_state *cand = (const mina_consensus_state *)(ic + PI_LENGTH), *tip = (const mina_consensus_state *)(it + PI_LENGTH);
        const mina_consensus_params cp{ic[PI_SLOTS_PER_SUB_WINDOW], ic[PI_SUB_WINDOWS]};
        const uint8_t *exp = expected_hashes + (size_t)b * MINA_STATES_PER_PROOF * 32;
        bool sel = false;
        if (it[PI_SUB_WINDOWS] == cp.sub_windows_per_window && cs_params_ok(&cp) &&
            cs_select_secure_chain(&cp, tip, CsTie{tip->last_vrf_output_hash, exp + 16 * 32}, cand, CsTie{cand->last_vrf_output_hash, exp + 15 * 32}, &sel))
            consensus = sel;
    }
    fmt[b] = format ? 1 : 0;
    precheck[b] = (ledger && consensus && (!and_in || and_in[b] != 0)) ? 1 : 0;
    if (masks) masks[b] = (format ? MINA_CHECK_FORMAT : 0u) | (ledger ? MINA_CHECK_LEDGER : 0u) | (consensus ? MINA_CHECK_CONSENSUS : 0u);
}
__global__ void __launch_bounds__(128)
pstate_precheck_kernel(uint32_t batch, const uint4 *__restrict__ records, const uint8_t *__restrict__ status, uint32_t *info, const uint8_t *expected_hashes,
                       const uint64_t *__restrict__ ledger_hashes, const uint8_t *__restrict__ and_in, uint8_t *fmt, uint8_t *__restrict__ precheck, uint32_t *__restrict__ masks) { mb_wave_prio();
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) pstate_precheck_entry(b, records, status, info, expected_hashes, ledger_hashes, and_in, fmt, precheck, masks);
}

// the records and field counts of a proof that failed FORMAT: zero, as the boundary's clear_states_half leaves them.  One lane per 16 bytes.
__global__ void __launch_bounds__(256)
pstate_clear_kernel(uint32_t batch, const uint8_t *__restrict__ fmt, uint4 *__restrict__ records, uint32_t *__restrict__ nfields) { mb_wave_prio();
    constexpr uint32_t PER = MINA_STATES_PER_PROOF * (PSTATE_REC_BYTES / 16);
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t b = t / PER; const uint32_t r = (uint32_t)(t % PER);
    if (b >= batch || fmt[b]) return;
    records[t] = make_uint4(0, 0, 0, 0);
    if (r < MINA_STATES_PER_PROOF) nfields[b * MINA_STATES_PER_PROOF + r] = 0;
}

}  // namespace mb
