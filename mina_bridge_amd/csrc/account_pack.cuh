// account_pack.cuh -- the opt-in device path of a Proof-of-Account job (mina_account_frontend_dev, mina_account_job_dev; MINA_VERIFY_ACCOUNT_ON_DEVICE):
// serialized `MinaAccountProof` / `MinaAccountPubInputs` pairs in, `passed` / `ran` words out.
//
// A streaming twin of the host path (wire_pub.h parse_merkle_path / parse_account_pub_inputs, wire_account.h read_account<Bincode> + abi_encode_account + the four
// `*_fields` flatteners, api_account.hip mb_verify_account_on), bincode only -- the form inside `MinaAccountProof`, the only one a verifier is handed.  The host path
// stays the checker: FORMAT / ACCOUNT_ABI / MERKLE, the account hash and the root are bit-identical to it for every input (tests/test_account_job_gpu.py), malformed
// ones included.
//
// Front end, one lane per proof, ONE walk in wire order, nothing in scratch:
//   * the Merkle path goes to a 64-sibling stride as it is read (depth <= 64, tags 0 / 1, 32-byte canonical elements);
//   * the account's whole field elements have fixed slots in the four `to_input` records (zkApp URI, verification key, zkApp, account) and go from the wire to
//     their slot as they are read; the packed chunks of the account record come in the REVERSE of wire order (permissions first, public-key parity last), so the
//     scalars ahead of the permissions wait in a dozen named registers; the zkApp record's three scalars and the URI's bits are packed as they arrive;
//   * the layout of `abi_encode_account` is a fixed function of the symbol and URI lengths: every value is compared with its 32-byte word of the public input's
//     `encoded_account` as it is read, bounds first, and the total length at the end -- the encoding is never materialised.  An absent delegate is (0, isOdd = true),
//     an absent zkApp the all-zero record with an empty URI, an absent verification key all zeros (the HASH of an absent key takes the dummy key instead);
//   * an account that carries a zkApp takes the next slot of a compacted list (one atomic add): its three zkApp records live at that slot, and the three zkApp hash
//     stages run over the list only.  An account without one is marked, and the account stage takes the context's cached hash of the default zkApp for it.
// Then: acct_hash_kernel (the salted sponge of api_account.hip salted_hash_kernel over a list whose length is in device memory), acct_fold_kernel (the Merkle fold
// with a depth per path) and acct_verdict_kernel (root against ledger hash, `passed` / `ran` by the host's rule).
#pragma once
#include "pack_common.cuh"
#ifndef MB_HIP_STUB
#include "sponge.cuh"
#endif

namespace mb {

constexpr uint32_t ACCT_REC16 = MINA_PSTATE_SLOTS * 32 / 16;               // a record in 16-byte units
constexpr uint32_t ACCT_MAX_DEPTH = 64;                                    // sibling / direction stride of a path
enum : uint32_t { AS_URI = 0, AS_VK, AS_ZKAPP, AS_ACCOUNT, AS_STAGES };    // records, field counts and salt indices: stage s of entry k at [s * n + k]
constexpr uint32_t ACCT_SALT_URI = 4, ACCT_SALT_VK = 5, ACCT_SALT_ZKAPP = 3, ACCT_SALT_ACCOUNT = 2;      // ctx.h MB_SALT_* (asserted in api_account_dev.hip)
// the front end's word per proof: MINA_CHECK_FORMAT, MINA_CHECK_ACCOUNT_ABI (only with FORMAT) and which of the three readers accepted
enum : uint32_t { AB_PATH = 0x100u, AB_PUB = 0x200u, AB_ACCOUNT = 0x400u };
// record slots (wire_account.h account_fields / zkapp_fields / vk_fields)
constexpr uint32_t AR_ZKAPP_HASH = 0, AR_VOTING_FOR = 1, AR_DELEGATE = 2, AR_RECEIPT = 3, AR_TOKEN_ID = 4, AR_PK = 5, AR_PACKED = 6;
constexpr uint32_t ZR_URI_HASH = 0, ZR_ACTION = 1, ZR_VK_HASH = 6, ZR_APP = 7, ZR_PACKED = 15;
constexpr uint32_t VR_POINTS = 56;                                         // 28 commitments, x and y; the six tag bits follow in slot 56
// `abi_encode_account` in 32-byte words: [0] offset 32, [1 .. 30] the head, [31] symbol length, [32] its bytes (if any), then the zkApp tuple at Z
constexpr uint32_t AW_HEAD = 30, AW_SYM = 31, AW_ZK_WORDS = 75, AW_ZK_URI_OFF = 74;

// ------------------------------------------------------------------------------------------------ the public input's `encoded_account`, compared in place
struct AbiCmp { const uint8_t *p; uint64_t len; bool ok; };
__device__ __forceinline__ void abi_b32(AbiCmp &a, uint32_t word, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {      // bytes32: the stored bytes as they are
    if (!a.ok || a.len / 32 <= word) { a.ok = false; return; }
    const uint8_t *q = a.p + 32 * (uint64_t)word;
    if (pc_ld64(q) != w0 || pc_ld64(q + 8) != w1 || pc_ld64(q + 16) != w2 || pc_ld64(q + 24) != w3) a.ok = false;
}
__device__ __forceinline__ void abi_uint(AbiCmp &a, uint32_t word, uint64_t v) { abi_b32(a, word, 0, 0, 0, __builtin_bswap64(v)); }      // uintN / bool / enum: one big-endian word
__device__ __forceinline__ void abi_chunk(AbiCmp &a, uint64_t at, uint64_t v) {          // 8 bytes of a dynamic member's tail
    if (!a.ok || a.len < 8 || a.len - 8 < at) { a.ok = false; return; }
    if (pc_ld64(a.p + at) != v) a.ok = false;
}

// a canonical base-field element -> record slot `slot`; returned for the ABI comparison
__device__ __forceinline__ void ac_field(PackCur &c, uint4 *rec, uint32_t slot, uint64_t &w0, uint64_t &w1, uint64_t &w2, uint64_t &w3) {
    pc_b32(c, w0, w1, w2, w3);
    if (!pc_canonical(w0, w1, w2, w3)) c.ok = false;
    pk_store(rec, slot, w0, w1, w2, w3);
}
__device__ __forceinline__ uint32_t ac_tag(PackCur &c, uint32_t max) { const uint32_t v = pc_u32(c); if (v > max) { c.ok = false; return 0; } return v; }
// up to 8 bytes at `q` as a little-endian word
__device__ __forceinline__ uint64_t ac_bytes(const uint8_t *q, uint32_t k) { if (k == 8) return pc_ld64(q); uint64_t v = 0; for (uint32_t b = 0; b < k; ++b) v |= (uint64_t)q[b] << (8 * b); return v; }

// ------------------------------------------------------------------------------------------------ one proof
// Proof i is bytes [proof_off[i], + proof_len[i]) of the blob, its public input [pub_off[i], + pub_len[i]); a slice that reaches past the blob is rejected.
// records / nfields / salt_idx: AS_STAGES * n entries.  Entry AS_ACCOUNT * n + i is account i's; the three zkApp stages are indexed by the SLOT a zkApp account
// takes in the compacted list (zk_index[slot] = i, *zk_count slots taken; the caller zeroes *zk_count).  Slots of a record past its field count are not written.
// A rejected proof has field count 0 everywhere, depth 0 unless its path alone parsed, a zero ledger hash unless its public input alone parsed.
__device__ __forceinline__ void acct_frontend_entry(uint32_t i, uint32_t n, const uint8_t *__restrict__ blob, uint64_t blob_len, const uint64_t *__restrict__ proof_off,
                                                    const uint64_t *__restrict__ proof_len, const uint64_t *__restrict__ pub_off, const uint64_t *__restrict__ pub_len,
                                                    uint4 *__restrict__ records, uint32_t *__restrict__ nfields, uint32_t *__restrict__ salt_idx, uint4 *__restrict__ siblings,
                                                    uint8_t *__restrict__ dirs, uint32_t *__restrict__ depths, uint4 *__restrict__ ledger, uint32_t *__restrict__ zk_marks,
                                                    uint32_t *__restrict__ zk_index, uint32_t *zk_count, uint32_t *__restrict__ bits) {
    uint64_t w0, w1, w2, w3;
    // ---- MinaAccountPubInputs: ledger hash, u64 length, encoded_account (wire_pub.h parse_account_pub_inputs)
    const uint64_t qo = pub_off[i], ql = pub_len[i];
    bool pub_ok = qo <= blob_len && ql <= blob_len - qo && ql >= 40;
    AbiCmp abi{blob, 0, false};
    w0 = w1 = w2 = w3 = 0;
    if (pub_ok) {
        const uint8_t *q = blob + qo;
        w0 = pc_ld64(q); w1 = pc_ld64(q + 8); w2 = pc_ld64(q + 16); w3 = pc_ld64(q + 24);
        pub_ok = pc_canonical(w0, w1, w2, w3) && pc_ld64(q + 32) == ql - 40;
        abi = AbiCmp{q + 40, ql - 40, pub_ok};
    }
    if (!pub_ok) w0 = w1 = w2 = w3 = 0;
    pk_store(ledger, i, w0, w1, w2, w3);

    // ---- MinaAccountProof: the Merkle path (wire_pub.h parse_merkle_path)
    const uint64_t po = proof_off[i], pl = proof_len[i];
    const bool in_blob = po <= blob_len && pl <= blob_len - po;
    PackCur c{blob, in_blob ? po + pl : 0, in_blob ? po : 0, in_blob};
    uint32_t depth = 0;
    {
        const uint64_t m = pc_u64(c);
        if (m > ACCT_MAX_DEPTH) c.ok = false;
        for (uint32_t h = 0; c.ok && h < (uint32_t)m; ++h) {
            const uint32_t tag = ac_tag(c, 1);
            if (pc_u64(c) != 32) c.ok = false;
            pc_b32(c, w0, w1, w2, w3);
            if (!pc_canonical(w0, w1, w2, w3)) c.ok = false;
            if (c.ok) { pk_store(siblings + (size_t)i * ACCT_MAX_DEPTH * 2, h, w0, w1, w2, w3); dirs[(size_t)i * ACCT_MAX_DEPTH + h] = (uint8_t)tag; }
        }
        if (c.ok) depth = (uint32_t)m;
    }
    const bool path_ok = c.ok;

    // ---- the account (wire_account.h read_account<Bincode>), its record (account_fields) and its ABI words as they come
    uint4 *ra = records + ((size_t)AS_ACCOUNT * n + i) * ACCT_REC16;
    pk_store(ra, AR_ZKAPP_HASH, 0, 0, 0, 0);                                 // patched in on the GPU
    abi_uint(abi, 0, 32);                                                    // the struct is dynamic: one offset word in front
    ac_field(c, ra, AR_PK, w0, w1, w2, w3); abi_b32(abi, 1, w0, w1, w2, w3);
    const uint32_t pk_odd = pc_bool(c); abi_uint(abi, 2, pk_odd);
    ac_field(c, ra, AR_TOKEN_ID, w0, w1, w2, w3); abi_b32(abi, 3, w0, w1, w2, w3);
    abi_uint(abi, 4, AW_HEAD * 32);                                          // offset of tokenSymbol
    uint64_t sym = 0; uint32_t symlen = 0;
    {   // Token_symbol.max_length = 6
        const uint64_t k = pc_len(c);
        if (k > 6) c.ok = false;
        if (pc_take(c, k)) { symlen = (uint32_t)k; sym = ac_bytes(c.p + c.pos, symlen); c.pos += k; }
    }
    const uint32_t Z = AW_SYM + 1 + (symlen ? 1u : 0u);                      // first word of the zkApp tuple
    abi_uint(abi, AW_SYM, symlen); if (symlen) abi_b32(abi, AW_SYM + 1, sym, 0, 0, 0);
    const uint64_t balance = pc_u64(c); abi_uint(abi, 5, balance);
    const uint32_t nonce = pc_u32(c); abi_uint(abi, 6, nonce);
    ac_field(c, ra, AR_RECEIPT, w0, w1, w2, w3); abi_b32(abi, 7, w0, w1, w2, w3);
    uint32_t delegate_odd = 0;
    if (pc_bool(c)) {
        ac_field(c, ra, AR_DELEGATE, w0, w1, w2, w3); abi_b32(abi, 8, w0, w1, w2, w3);
        delegate_odd = pc_bool(c); abi_uint(abi, 9, delegate_odd);
    } else { pk_store(ra, AR_DELEGATE, 0, 0, 0, 0); abi_b32(abi, 8, 0, 0, 0, 0); abi_uint(abi, 9, 1); }      // absent delegate: (zero, isOdd = true) in the ABI, (zero, false) in the hash
    ac_field(c, ra, AR_VOTING_FOR, w0, w1, w2, w3); abi_b32(abi, 10, w0, w1, w2, w3);
    const uint32_t timed = ac_tag(c, 1);
    uint64_t t_min = 0, t_cliff_amount = 0, t_increment = 0; uint32_t t_cliff_time = 0, t_period = 0;
    if (timed) {
        t_min = pc_u64(c); if (pc_u32(c) != 0) c.ok = false; t_cliff_time = pc_u32(c); t_cliff_amount = pc_u64(c);
        if (pc_u32(c) != 0) c.ok = false; t_period = pc_u32(c); t_increment = pc_u64(c);
    }
    abi_uint(abi, 11, t_min); abi_uint(abi, 12, t_cliff_time); abi_uint(abi, 13, t_cliff_amount); abi_uint(abi, 14, t_period); abi_uint(abi, 15, t_increment);
    Packer k{0, 0, 0, 0, 0, 0, ra, AR_PACKED};
    for (uint32_t p = 0; p < 13; ++p) {                                      // permissions: (constant, signature_necessary, signature_sufficient) per tag
        const uint32_t tag = ac_tag(c, 4);
        abi_uint(abi, 16 + p + (p > 6 ? 1u : 0u), tag);
        pk_bits(k, (uint64_t)((0x63015u >> (4 * tag)) & 7u) << 61, 0, 0, 0, 3);
        if (p == 6) { const uint32_t v = pc_u32(c); abi_uint(abi, 23, v); pk_packed(k, v, 32); }      // set_verification_key's txn version
    }
    pk_packed(k, timed, 1); pk_packed(k, t_min, 64); pk_packed(k, t_cliff_time, 32); pk_packed(k, t_cliff_amount, 64);
    pk_packed(k, timed ? t_period : 1u, 32); pk_packed(k, t_increment, 64);      // untimed: vesting period 1
    pk_packed(k, delegate_odd, 1); pk_packed(k, nonce, 32); pk_packed(k, balance, 64); pk_packed(k, sym, 48); pk_packed(k, pk_odd, 1);
    if (k.nbits > 0) pk_flush(k);
    const uint32_t nf_account = AR_PACKED + k.npacked;
    abi_uint(abi, AW_HEAD, AW_HEAD * 32 + 32 + (symlen ? 32u : 0u));         // offset of the zkApp tuple: behind the symbol's tail

    // ---- the zkApp, if any: three more records at the account's slot of the compacted list
    const uint32_t has_zkapp = pc_bool(c);
    uint32_t slot = 0, nf_uri = 0, uri_words = 0;
    if (has_zkapp) {
        slot = atomicAdd(zk_count, 1u);
        zk_index[slot] = i;
        uint4 *ru = records + ((size_t)AS_URI * n + slot) * ACCT_REC16, *rv = records + ((size_t)AS_VK * n + slot) * ACCT_REC16, *rz = records + ((size_t)AS_ZKAPP * n + slot) * ACCT_REC16;
        pk_store(rz, ZR_URI_HASH, 0, 0, 0, 0); pk_store(rz, ZR_VK_HASH, 0, 0, 0, 0);      // patched in on the GPU
        for (uint32_t j = 0; j < 8; ++j) { ac_field(c, rz, ZR_APP + j, w0, w1, w2, w3); abi_b32(abi, Z + j, w0, w1, w2, w3); }
        uint32_t mpv = 2, awds = 2;                                          // no key: the hash takes the dummy key (2, 2, every commitment (1, 2)), the ABI all zeros
        if (pc_bool(c)) {
            mpv = ac_tag(c, 2); awds = ac_tag(c, 2);
            abi_uint(abi, Z + 8, mpv); abi_uint(abi, Z + 9, awds);
            for (uint32_t j = 0; j < VR_POINTS; ++j) { ac_field(c, rv, j, w0, w1, w2, w3); abi_b32(abi, Z + 10 + j, w0, w1, w2, w3); }
        } else {
            abi_uint(abi, Z + 8, 0); abi_uint(abi, Z + 9, 0);
            for (uint32_t j = 0; j < VR_POINTS; ++j) { pk_store(rv, j, 1 + (j & 1u), 0, 0, 0); abi_b32(abi, Z + 10 + j, 0, 0, 0, 0); }
        }
        pk_store(rv, VR_POINTS, ((mpv == 0) << 5) | ((mpv == 1) << 4) | ((mpv == 2) << 3) | ((awds == 0) << 2) | ((awds == 1) << 1) | (awds == 2), 0, 0, 0);
        const uint32_t version = pc_u32(c); abi_uint(abi, Z + 66, version);
        for (uint32_t j = 0; j < 5; ++j) { ac_field(c, rz, ZR_ACTION + j, w0, w1, w2, w3); abi_b32(abi, Z + 67 + j, w0, w1, w2, w3); }
        if (pc_u32(c) != 0) c.ok = false;                                    // last_action_slot: Since_genesis of u32
        const uint32_t action_slot = pc_u32(c); abi_uint(abi, Z + 72, action_slot);
        const uint32_t proved = pc_bool(c); abi_uint(abi, Z + 73, proved);
        Packer kz{0, 0, 0, 0, 0, 0, rz, ZR_PACKED};
        pk_packed(kz, proved, 1); pk_packed(kz, action_slot, 32); pk_packed(kz, version, 32); pk_flush(kz);
        abi_uint(abi, Z + AW_ZK_URI_OFF, AW_ZK_WORDS * 32);                  // offset of zkappUri inside the tuple
        // the URI (at most 255 bytes), eight bytes at a time: its bits into the record, its bytes and their zero padding against the ABI tail
        Packer ku{0, 0, 0, 0, 0, 0, ru, 0};
        const uint64_t ul = pc_len(c);
        if (ul > 255) c.ok = false;
        if (pc_take(c, ul)) {
            abi_uint(abi, Z + AW_ZK_WORDS, ul);
            uri_words = ((uint32_t)ul + 31) / 32;
            for (uint32_t ch = 0; ch < 4 * uri_words; ++ch) {
                const uint32_t have = 8 * ch < (uint32_t)ul ? ((uint32_t)ul - 8 * ch < 8 ? (uint32_t)ul - 8 * ch : 8u) : 0u;
                const uint64_t v = ac_bytes(c.p + c.pos + 8 * ch, have);
                abi_chunk(abi, 32 * (uint64_t)(Z + AW_ZK_WORDS + 1) + 8 * ch, v);
                if (have) pk_bits(ku, __brevll(v), 0, 0, 0, 8 * have);
            }
            c.pos += ul;
        }
        pk_packed(ku, 1, 1); pk_flush(ku);
        nf_uri = ku.npacked;
    } else {
        for (uint32_t j = 0; j <= AW_ZK_WORDS; ++j) abi_uint(abi, Z + j, j == AW_ZK_URI_OFF ? AW_ZK_WORDS * 32 : 0);      // the all-zero zkApp, an empty URI
    }
    const bool account_ok = c.ok && c.pos == c.end;                          // nothing behind the account
    const bool abi_ok = abi.ok && abi.len == 32 * (uint64_t)(Z + AW_ZK_WORDS + 1 + uri_words);
    const bool format = path_ok && pub_ok && account_ok;

    nfields[AS_ACCOUNT * n + i] = format ? nf_account : 0; salt_idx[AS_ACCOUNT * n + i] = ACCT_SALT_ACCOUNT;
    if (has_zkapp) {
        nfields[AS_URI * n + slot] = format ? nf_uri : 0; salt_idx[AS_URI * n + slot] = ACCT_SALT_URI;
        nfields[AS_VK * n + slot] = format ? VR_POINTS + 1 : 0; salt_idx[AS_VK * n + slot] = ACCT_SALT_VK;
        nfields[AS_ZKAPP * n + slot] = format ? ZR_PACKED + 1 : 0; salt_idx[AS_ZKAPP * n + slot] = ACCT_SALT_ZKAPP;
    }
    zk_marks[i] = format && has_zkapp ? 1u : 0u;
    depths[i] = depth;
    bits[i] = (format ? MINA_CHECK_FORMAT : 0u) | (format && abi_ok ? MINA_CHECK_ACCOUNT_ABI : 0u) | (path_ok ? AB_PATH : 0u) | (pub_ok ? AB_PUB : 0u) | (account_ok ? AB_ACCOUNT : 0u);
}
__global__ void __launch_bounds__(256)
acct_frontend_kernel(uint32_t n, const uint8_t *__restrict__ blob, uint64_t blob_len, const uint64_t *__restrict__ proof_off, const uint64_t *__restrict__ proof_len,
                     const uint64_t *__restrict__ pub_off, const uint64_t *__restrict__ pub_len, uint4 *__restrict__ records, uint32_t *__restrict__ nfields,
                     uint32_t *__restrict__ salt_idx, uint4 *__restrict__ siblings, uint8_t *__restrict__ dirs, uint32_t *__restrict__ depths, uint4 *__restrict__ ledger,
                     uint32_t *__restrict__ zk_marks, uint32_t *__restrict__ zk_index, uint32_t *zk_count, uint32_t *__restrict__ bits) { mb_wave_prio();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) acct_frontend_entry(i, n, blob, blob_len, proof_off, proof_len, pub_off, pub_len, records, nfields, salt_idx, siblings, dirs, depths, ledger, zk_marks, zk_index, zk_count, bits);
}

// One lane per proof, after the fold: `passed` / `ran` by the rule of mb_verify_account_on.  Unparsable: ran = FORMAT, passed = 0.  Parsable: ran |= ACCOUNT_ABI | MERKLE,
// passed = FORMAT, ACCOUNT_ABI if the encodings agreed, MERKLE if the root is the ledger hash (a depth-0 path: the account hash itself).
__device__ __forceinline__ void acct_verdict_entry(uint32_t i, const uint32_t *__restrict__ bits, const uint4 *__restrict__ roots, const uint4 *__restrict__ ledger,
                                                   uint32_t *__restrict__ passed, uint32_t *__restrict__ ran) {
    const uint32_t b = bits[i];
    uint32_t p = 0, r = MINA_CHECK_FORMAT;
    if (b & MINA_CHECK_FORMAT) {
        p = MINA_CHECK_FORMAT | (b & MINA_CHECK_ACCOUNT_ABI); r |= MINA_CHECK_ACCOUNT_ABI | MINA_CHECK_MERKLE;
        const uint4 a0 = roots[2 * (size_t)i], a1 = roots[2 * (size_t)i + 1], l0 = ledger[2 * (size_t)i], l1 = ledger[2 * (size_t)i + 1];
        if (a0.x == l0.x && a0.y == l0.y && a0.z == l0.z && a0.w == l0.w && a1.x == l1.x && a1.y == l1.y && a1.z == l1.z && a1.w == l1.w) p |= MINA_CHECK_MERKLE;
    }
    passed[i] = p; ran[i] = r;
}
__global__ void __launch_bounds__(256)
acct_verdict_kernel(uint32_t n, const uint32_t *__restrict__ bits, const uint4 *__restrict__ roots, const uint4 *__restrict__ ledger, uint32_t *__restrict__ passed,
                    uint32_t *__restrict__ ran) { mb_wave_prio();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) acct_verdict_entry(i, bits, roots, ledger, passed, ran);
}

#ifndef MB_HIP_STUB
// ------------------------------------------------------------------------------------------------ the Poseidon stages
// salted_hash_kernel (api_account.hip) over a list whose length may be known on the device only: `roles` x n sponges, sponge (role, j) live for j < min(n, *count_dev)
// (count_dev null: n).  Its record, field count and salt index are entry role * n + j; patch_a / patch_b (optional, entry j of an earlier stage) replace slots slot_a /
// slot_b.  With `marks`: an entry whose mark is 0 takes patch_a_default (8 words, the same for all) for slot_a instead.  The hash goes to entry role * n + j of `out`,
// or to entry out_index[j].  A wave without a live sponge leaves at once; dead groups of a live wave shadow entry 0.
template <int F, int LANES>
__global__ void __launch_bounds__(256)
acct_hash_kernel(uint32_t n, uint32_t roles, const uint32_t *__restrict__ count_dev, FieldK fk, const PoseidonParams *__restrict__ pp, const fe_t *__restrict__ salts,
                 const uint32_t *__restrict__ salt_idx, const uint32_t *__restrict__ records, const uint32_t *__restrict__ nfields, const uint32_t *__restrict__ patch_a,
                 uint32_t slot_a, const uint32_t *__restrict__ patch_b, uint32_t slot_b, const uint32_t *__restrict__ marks, const uint32_t *__restrict__ patch_a_default,
                 const uint32_t *__restrict__ out_index, uint32_t *__restrict__ out) { mb_wave_prio();
    bool writer;
    const uint32_t sp = coop_sponge_index<LANES>(writer), e = coop_elem<LANES>();
    uint32_t cnt = n;
    if (count_dev) { const uint32_t m = *count_dev; if (m < cnt) cnt = m; }
    const uint32_t role = sp / n, j = sp - role * n;
    const bool live = role < roles && j < cnt;
    if (__ballot(live) == 0) return;
    const uint32_t idx = live ? role * n + j : 0, jj = live ? j : 0;
    const uint32_t *rec = records + (size_t)idx * MINA_PSTATE_SLOTS * 8;
    uint32_t nf = nfields[idx]; if (nf > MINA_PSTATE_SLOTS) nf = MINA_PSTATE_SLOTS;
    uint32_t si = salt_idx[idx]; if (si > ACCT_SALT_VK) si = ACCT_SALT_VK;
    const uint32_t *pa = patch_a ? ((marks && !marks[jj]) ? patch_a_default : patch_a + (size_t)jj * 8) : nullptr;
    fe_t s = salts[si * 3 + e];
    uint32_t count = 0;
    for (uint32_t el = 0; el < nf; ++el) {
        if (count == 2) { poseidon_permute_coop<F, LANES>(s, pp); count = 0; }
        if (e == count) {
            const uint32_t *src = (pa && el == slot_a) ? pa : ((patch_b && el == slot_b) ? patch_b + (size_t)jj * 8 : rec + (size_t)el * 8);
            s = fe_add<F>(s, fe_to_mont<F>(load_fe<F>(src), fk.r2));
        }
        ++count;
    }
    poseidon_permute_coop<F, LANES>(s, pp);
    s = coop_get<LANES>(s, 0);
    if (live && writer) { const fe_t w = fe_from_mont<F>(s); const size_t o = out_index ? out_index[j] : idx; for (int i = 0; i < 8; ++i) out[o * 8 + i] = w.v[i]; }
}

// merkle_fold_coop_kernel (sponge.cuh) with a depth per path and a sibling / direction stride of ACCT_MAX_DEPTH.  A wave runs to the deepest of its paths; a lane
// group whose path is shorter keeps its node meanwhile (the cooperative permutation needs every lane of the wave).  depth 0: the root is the leaf.
template <int F, int LANES>
__global__ void __launch_bounds__(256)
acct_fold_kernel(uint32_t n, FieldK fk, const PoseidonParams *__restrict__ pp, const fe_t *__restrict__ salts /* ACCT_MAX_DEPTH x 3, Montgomery */,
                 const uint32_t *__restrict__ leaves, const uint32_t *__restrict__ siblings, const uint8_t *__restrict__ dirs, const uint32_t *__restrict__ depths,
                 uint32_t *__restrict__ roots) { mb_wave_prio();
    bool writer; const uint32_t path = coop_sponge_index<LANES>(writer), e = coop_elem<LANES>();
    const bool live = path < n;
    const uint32_t pidx = live ? path : 0;
    uint32_t d = live ? depths[pidx] : 0; if (d > ACCT_MAX_DEPTH) d = ACCT_MAX_DEPTH;
    fe_t node = fe_to_mont<F>(load_fe<F>(leaves + (size_t)pidx * 8), fk.r2);
    for (uint32_t h = 0; __ballot(h < d) != 0; ++h) {
        const bool on = h < d;
        const uint32_t hh = on ? h : 0;
        const fe_t sib = fe_to_mont<F>(load_fe<F>(siblings + ((size_t)pidx * ACCT_MAX_DEPTH + hh) * 8), fk.r2);
        const bool node_is_left = dirs[(size_t)pidx * ACCT_MAX_DEPTH + hh] == 0;
        fe_t st = salts[(size_t)hh * 3 + e];
        if (e == 0) st = fe_add<F>(st, node_is_left ? node : sib);
        if (e == 1) st = fe_add<F>(st, node_is_left ? sib : node);
        poseidon_permute_coop<F, LANES>(st, pp);
        const fe_t up = coop_get<LANES>(st, 0);
        if (on) node = up;
    }
    if (live && writer) { const fe_t o = fe_from_mont<F>(node); for (int i = 0; i < 8; ++i) roots[(size_t)path * 8 + i] = o.v[i]; }
}
#endif

}  // namespace mb
