// api_account_dev.hip -- the opt-in device path of a Proof-of-Account job (account_pack.cuh): serialized (MinaAccountProof, MinaAccountPubInputs) pairs in HBM ->
// `passed` / `ran` words, with nothing read on the host.
//
// mina_account_frontend_dev is the reader alone; mina_account_job_dev queues the whole job on one lane without waiting for the GPU:
//     front end -> [URI + verification-key hashes -> zkApp hash] over the accounts that carry a zkApp -> account hash -> Merkle fold (a depth per path) -> verdicts.
// mb_verify_account_dev_on is what the boundary runs under MINA_VERIFY_ACCOUNT_ON_DEVICE: it uploads a call's bytes as they are and runs the job.  The host path
// (api_account.hip mb_verify_account_on) is the checker: every output is bit-identical to it for every input.
//
// The sub-hashes of an account WITHOUT a zkApp -- H_"MinaZkappUri"(empty URI), H_"MinaSideLoadedVk"(dummy key), H_"MinaZkappAccount"(default record) -- depend on the
// installed Poseidon tables only: ensure_defaults hashes them once per context (about 40 of the ~95 permutations of a plain account's chain) and
// mina_poseidon_set_params drops them.
#include <mutex>

#include "ctx.h"
#include "account_pack.cuh"
#include "wire_account.h"

int mb_merkle_prepare_salts(mina_ctx *c, int field, uint32_t depth);
int mb_ensure_state_salts(mina_ctx *c);

static_assert(mb::ACCT_SALT_URI == MB_SALT_ZKAPP_URI && mb::ACCT_SALT_VK == MB_SALT_SIDE_LOADED_VK && mb::ACCT_SALT_ZKAPP == MB_SALT_ZKAPP_ACCOUNT && mb::ACCT_SALT_ACCOUNT == MB_SALT_ACCOUNT &&
              mb::ACCT_SALT_VK == MB_N_PREFIX_SALTS - 1, "account_pack.cuh names the salts of ctx.h");
static_assert(mb::ZR_URI_HASH == mw::ZK_SLOT_URI && mb::ZR_VK_HASH == mw::ZK_SLOT_VK, "the zkApp record's patched slots (wire_account.h)");

static constexpr size_t ACCOUNT_MAX_PROOFS = (size_t)1 << 22;
static constexpr size_t REC_BYTES = (size_t)MINA_PSTATE_SLOTS * 32;

// n sponges per role on the current lane; see acct_hash_kernel
static int acct_hash_dev(mina_ctx *c, size_t n, uint32_t roles, const uint32_t *count_dev, const uint32_t *salt_idx, const uint32_t *recs, const uint32_t *nf, const uint32_t *pa, uint32_t sa,
                         const uint32_t *pb, uint32_t sb, const uint32_t *marks, const uint32_t *pa_default, const uint32_t *out_index, uint32_t *out) {
    const PoseidonParams *pp = c->pparams[FIELD_FP].as<PoseidonParams>();
    const fe_t *salts = c->state_salts.as<fe_t>();
    ProfScope ps_(c, PS_STATE_HASH);
    return with_lanes<16, 8, 3>(hash_lanes(c, n, n * roles), [&](auto lanes) {
        constexpr int LN = decltype(lanes)::value;
        mb::acct_hash_kernel<FIELD_FP, LN><<<cdiv(coop_threads<LN>(n * roles), 256), 256, 0, c->L->stream>>>((uint32_t)n, roles, count_dev, c->fk[FIELD_FP], pp, salts, salt_idx, recs, nf, pa, sa,
                                                                                                           pb, sb, marks, pa_default, out_index, out);
        HIPC(hipGetLastError());
        return MINA_OK;
    });
}

// c->acct_defaults: [0, 24) words = the three default hashes (URI, key, zkApp), then their records, field counts and salt indices.  Waits for the lane once.
static constexpr size_t DEF_RECS = 96, DEF_NF = DEF_RECS + 3 * REC_BYTES, DEF_SALT = DEF_NF + 12, DEF_BYTES = DEF_SALT + 12;
static int ensure_defaults(mina_ctx *c) {
    if (c->have_acct_defaults) return MINA_OK;
    int rc;
    if ((rc = c->acct_defaults.ensure(DEF_BYTES))) return rc;
    std::vector<uint8_t> host(DEF_BYTES, 0);
    uint32_t *nf = (uint32_t *)(host.data() + DEF_NF), *salt = (uint32_t *)(host.data() + DEF_SALT);
    const mw::ZkappAccount z;
    std::vector<mw::B32> f;
    auto put = [&](size_t k, uint32_t salt_id) { for (size_t j = 0; j < f.size() && j < MINA_PSTATE_SLOTS; ++j) memcpy(host.data() + DEF_RECS + k * REC_BYTES + j * 32, f[j].b, 32);
                                                 nf[k] = (uint32_t)(f.size() < MINA_PSTATE_SLOTS ? f.size() : MINA_PSTATE_SLOTS); salt[k] = salt_id; };
    mw::zkapp_uri_fields(z.zkapp_uri, f); put(0, MB_SALT_ZKAPP_URI);
    mw::vk_fields(mw::dummy_vk(), f); put(1, MB_SALT_SIDE_LOADED_VK);
    mw::zkapp_fields(z, f); put(2, MB_SALT_ZKAPP_ACCOUNT);
    uint8_t *d = c->acct_defaults.as<uint8_t>();
    uint32_t *h = c->acct_defaults.as<uint32_t>();
    HIPC(hipMemcpyAsync(d, host.data(), DEF_BYTES, hipMemcpyHostToDevice, c->L->stream));
    const uint32_t *recs = (const uint32_t *)(d + DEF_RECS), *dnf = (const uint32_t *)(d + DEF_NF), *dsalt = (const uint32_t *)(d + DEF_SALT);
    if ((rc = acct_hash_dev(c, 1, 2, nullptr, dsalt, recs, dnf, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, h))) return rc;                                  // URI, key
    if ((rc = acct_hash_dev(c, 1, 1, nullptr, dsalt + 2, recs + 2 * REC_BYTES / 4, dnf + 2, h, mw::ZK_SLOT_URI, h + 8, mw::ZK_SLOT_VK, nullptr, nullptr, nullptr, h + 16))) return rc;   // zkApp
    HIPC(hipStreamSynchronize(c->L->stream));                    // `host` leaves; other lanes read the hashes
    c->have_acct_defaults = true;
    return MINA_OK;
}

// everything a job needs before its first launch, on the current lane: the prefix salts, the Merkle salts up to the deepest height a path may have, the default sub-hashes
static int account_prepare(mina_ctx *c) {
    int rc; Lane *L = c->L;
    if ((rc = mb_ensure_state_salts(c))) return rc;
    c->L = L;
    if ((rc = mb_merkle_prepare_salts(c, FIELD_FP, mb::ACCT_MAX_DEPTH))) return rc;
    c->L = L;
    return ensure_defaults(c);
}

// the workspace of a job of n proofs inside Lane::ac_ws (every part 256-byte aligned)
struct AccountWs {
    size_t records, nfields, salt_idx, siblings, dirs, depths, ledger, marks, zk_index, zk_count, bits, h_uri /* + key: 2 n */, h_zkapp, h_account, roots, total;
    explicit AccountWs(size_t n) {
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 255) & ~(size_t)255; return o; };
        records = take(mb::AS_STAGES * n * REC_BYTES); nfields = take(mb::AS_STAGES * n * 4); salt_idx = take(mb::AS_STAGES * n * 4);
        siblings = take(n * mb::ACCT_MAX_DEPTH * 32); dirs = take(n * mb::ACCT_MAX_DEPTH); depths = take(n * 4); ledger = take(n * 32); marks = take(n * 4);
        zk_index = take(n * 4); zk_count = take(4); bits = take(n * 4); h_uri = take(2 * n * 32); h_zkapp = take(n * 32); h_account = take(n * 32); roots = take(n * 32);
        total = at;
    }
};

static int frontend_launch(mina_ctx *c, size_t n, const void *d_blob, size_t blob_len, const void *d_proof_off, const void *d_proof_len, const void *d_pub_off, const void *d_pub_len,
                           void *d_records, void *d_nfields, void *d_salt_idx, void *d_siblings, void *d_dirs, void *d_depths, void *d_ledger, void *d_marks, void *d_zk_index,
                           void *d_zk_count, void *d_bits) {
    HIPC(hipMemsetAsync(d_zk_count, 0, 4, c->L->stream));
    mb::acct_frontend_kernel<<<cdiv(n, 256), 256, 0, c->L->stream>>>((uint32_t)n, (const uint8_t *)d_blob, (uint64_t)blob_len, (const uint64_t *)d_proof_off, (const uint64_t *)d_proof_len,
                                                                   (const uint64_t *)d_pub_off, (const uint64_t *)d_pub_len, (uint4 *)d_records, (uint32_t *)d_nfields, (uint32_t *)d_salt_idx,
                                                                   (uint4 *)d_siblings, (uint8_t *)d_dirs, (uint32_t *)d_depths, (uint4 *)d_ledger, (uint32_t *)d_marks, (uint32_t *)d_zk_index,
                                                                   (uint32_t *)d_zk_count, (uint32_t *)d_bits);
    HIPC(hipGetLastError());
    return MINA_OK;
}

// mina_account_job_dev without the argument checks, queued on the CURRENT lane; account_prepare has run
static int account_job_on_lane(mina_ctx *c, size_t n, const void *d_blob, size_t blob_len, const void *d_proof_off, const void *d_proof_len, const void *d_pub_off, const void *d_pub_len,
                               void *d_passed, void *d_ran, void *d_account_hashes, void *d_roots) {
    Lane &L = *c->L;
    const AccountWs w(n);
    int rc;
    if ((rc = L.ac_ws.ensure(w.total))) return rc;
    uint8_t *d = L.ac_ws.as<uint8_t>();
    auto W = [&](size_t off) { return (uint32_t *)(d + off); };
    auto stage = [&](size_t off, uint32_t s, size_t per) { return (const uint32_t *)(d + off + (size_t)s * n * per); };
    if ((rc = frontend_launch(c, n, d_blob, blob_len, d_proof_off, d_proof_len, d_pub_off, d_pub_len, d + w.records, d + w.nfields, d + w.salt_idx, d + w.siblings, d + w.dirs, d + w.depths,
                              d + w.ledger, d + w.marks, d + w.zk_index, d + w.zk_count, d + w.bits))) return rc;
    const uint32_t *defaults = c->acct_defaults.as<uint32_t>(), *zk_count = W(w.zk_count);
    // URI and key hashes of the accounts that carry a zkApp (one launch, two roles), then their zkApp hashes, each to its account's place
    if ((rc = acct_hash_dev(c, n, 2, zk_count, stage(w.salt_idx, mb::AS_URI, 4), stage(w.records, mb::AS_URI, REC_BYTES), stage(w.nfields, mb::AS_URI, 4), nullptr, 0, nullptr, 0, nullptr, nullptr,
                            nullptr, W(w.h_uri)))) return rc;
    if ((rc = acct_hash_dev(c, n, 1, zk_count, stage(w.salt_idx, mb::AS_ZKAPP, 4), stage(w.records, mb::AS_ZKAPP, REC_BYTES), stage(w.nfields, mb::AS_ZKAPP, 4), W(w.h_uri), mw::ZK_SLOT_URI,
                            W(w.h_uri) + n * 8, mw::ZK_SLOT_VK, nullptr, nullptr, W(w.zk_index), W(w.h_zkapp)))) return rc;
    // every account; one without a zkApp takes the cached hash of the default record
    if ((rc = acct_hash_dev(c, n, 1, nullptr, stage(w.salt_idx, mb::AS_ACCOUNT, 4), stage(w.records, mb::AS_ACCOUNT, REC_BYTES), stage(w.nfields, mb::AS_ACCOUNT, 4), W(w.h_zkapp), mb::AR_ZKAPP_HASH,
                            nullptr, 0, W(w.marks), defaults + 16, nullptr, W(w.h_account)))) return rc;
    if ((rc = with_lanes<16, 8, 3>(merkle_lanes(c, n), [&](auto lanes) {
            constexpr int LN = decltype(lanes)::value;
            mb::acct_fold_kernel<FIELD_FP, LN><<<cdiv(coop_threads<LN>(n), 256), 256, 0, L.stream>>>((uint32_t)n, c->fk[FIELD_FP], c->pparams[FIELD_FP].as<PoseidonParams>(),
                c->merkle_salts[FIELD_FP].as<fe_t>(), W(w.h_account), W(w.siblings), d + w.dirs, W(w.depths), W(w.roots));
            HIPC(hipGetLastError());
            return MINA_OK;
        }))) return rc;
    mb::acct_verdict_kernel<<<cdiv(n, 256), 256, 0, L.stream>>>((uint32_t)n, W(w.bits), (const uint4 *)(d + w.roots), (const uint4 *)(d + w.ledger), (uint32_t *)d_passed, (uint32_t *)d_ran);
    HIPC(hipGetLastError());
    if (d_account_hashes) HIPC(hipMemcpyAsync(d_account_hashes, d + w.h_account, n * 32, hipMemcpyDeviceToDevice, L.stream));
    if (d_roots) HIPC(hipMemcpyAsync(d_roots, d + w.roots, n * 32, hipMemcpyDeviceToDevice, L.stream));
    return MINA_OK;
}

static bool misaligned8(const void *a, const void *b, const void *c2, const void *d) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c2 | (uintptr_t)d) & 7u) != 0; }

extern "C" int mina_account_frontend_dev(mina_ctx *c, size_t n, const void *d_blob, size_t blob_len, const void *d_proof_off, const void *d_proof_len, const void *d_pub_off,
                                         const void *d_pub_len, void *d_records, void *d_nfields, void *d_salt_idx, void *d_siblings, void *d_dirs, void *d_depths, void *d_ledger_hashes,
                                         void *d_zk_marks, void *d_zk_index, void *d_zk_count, void *d_bits) {
    if (!c || !d_zk_count || (n && (!d_blob || !d_proof_off || !d_proof_len || !d_pub_off || !d_pub_len || !d_records || !d_nfields || !d_salt_idx || !d_siblings || !d_dirs || !d_depths ||
                                    !d_ledger_hashes || !d_zk_marks || !d_zk_index || !d_bits))) return fail(MINA_ERR_ARG, "null argument");
    if (misaligned8(d_proof_off, d_proof_len, d_pub_off, d_pub_len) || (((uintptr_t)d_records | (uintptr_t)d_siblings | (uintptr_t)d_ledger_hashes) & 15u) ||
        (((uintptr_t)d_nfields | (uintptr_t)d_salt_idx | (uintptr_t)d_depths | (uintptr_t)d_zk_marks | (uintptr_t)d_zk_index | (uintptr_t)d_zk_count | (uintptr_t)d_bits) & 3u))
        return fail(MINA_ERR_ARG, "misaligned argument: offsets / lengths 8, records / siblings / ledger hashes 16, the u32 arrays 4 bytes");
    if (n > ACCOUNT_MAX_PROOFS) return fail(MINA_ERR_ARG, "n too large");
    if (!c->have_pparams[FIELD_FP]) return fail(MINA_ERR_STATE, "Poseidon constants not installed for Fp");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    if (n == 0) { HIPC(hipMemsetAsync(d_zk_count, 0, 4, c->L->stream)); return MINA_OK; }
    return frontend_launch(c, n, d_blob, blob_len, d_proof_off, d_proof_len, d_pub_off, d_pub_len, d_records, d_nfields, d_salt_idx, d_siblings, d_dirs, d_depths, d_ledger_hashes, d_zk_marks,
                           d_zk_index, d_zk_count, d_bits);
}

extern "C" int mina_account_job_dev(mina_ctx *c, size_t n, const void *d_blob, size_t blob_len, const void *d_proof_off, const void *d_proof_len, const void *d_pub_off, const void *d_pub_len,
                                    void *d_passed, void *d_ran, void *d_account_hashes, void *d_roots) {
    if (!c || (n && (!d_blob || !d_proof_off || !d_proof_len || !d_pub_off || !d_pub_len || !d_passed || !d_ran))) return fail(MINA_ERR_ARG, "null argument");
    if (misaligned8(d_proof_off, d_proof_len, d_pub_off, d_pub_len) || (((uintptr_t)d_passed | (uintptr_t)d_ran | (uintptr_t)d_account_hashes | (uintptr_t)d_roots) & 3u))
        return fail(MINA_ERR_ARG, "misaligned argument: offsets / lengths 8, the outputs 4 bytes");
    if (n > ACCOUNT_MAX_PROOFS) return fail(MINA_ERR_ARG, "n too large");
    if (!c->have_pparams[FIELD_FP]) return fail(MINA_ERR_STATE, "Poseidon constants not installed for Fp");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    if (n == 0) return MINA_OK;
    int rc;
    if ((rc = account_prepare(c))) return rc;
    return account_job_on_lane(c, n, d_blob, blob_len, d_proof_off, d_proof_len, d_pub_off, d_pub_len, d_passed, d_ran, d_account_hashes, d_roots);
}

// The device twin of mb_verify_account_on (api_account.hip), same arguments and the same use of `lane` / `enq_mu`: the lock is held while the job is QUEUED, not while
// the host copies the call's bytes into the page-locked upload block or waits for the GPU.  The block: n u64 proof offsets, proof lengths, public-input offsets and
// lengths, then the bytes as they are; a null proof or public input gets an offset past the block, which the reader rejects as the host path does.
int mb_verify_account_dev_on(mina_ctx *c, size_t n, const uint8_t *const *proofs, const size_t *proof_lens, const uint8_t *const *pubs, const size_t *pub_lens, uint32_t *passed, uint32_t *ran,
                             Lane *lane, std::mutex *enq_mu) {
    if (!c || (n && (!proofs || !proof_lens || !pubs || !pub_lens || !passed || !ran))) return fail(MINA_ERR_ARG, "null argument");
    if (!c->have_pparams[FIELD_FP]) return fail(MINA_ERR_STATE, "Poseidon constants not installed for Fp");
    if (n > ACCOUNT_MAX_PROOFS) return fail(MINA_ERR_ARG, "n too large");
    if (n == 0) return MINA_OK;
    HIPC(hipSetDevice(c->device));
    int rc;
    struct Enq {                                                 // as in api_account.hip account_hashes: the lane cursor is set inside the lock and put back before it is released
        mina_ctx *c; Lane *lane; std::mutex *mu; bool held = false;
        void lock() { if (mu) mu->lock(); held = true; if (lane) c->L = lane; else c->use_lane0(); }
        void unlock() { if (held) { c->use_lane0(); if (mu) mu->unlock(); held = false; } }
        ~Enq() { unlock(); }
    } enq{c, lane, enq_mu};
    enq.lock();
    if (lane && !lane->stream) HIPC(hipStreamCreateWithFlags(&lane->stream, hipStreamNonBlocking));
    if ((rc = account_prepare(c))) return rc;
    Lane &L = *c->L;
    enq.unlock();
    const size_t table = 4 * n * 8;
    std::vector<size_t> at(2 * n);
    size_t bytes = table;
    for (size_t i = 0; i < n; ++i) { at[2 * i] = bytes; if (proofs[i]) bytes += proof_lens[i]; at[2 * i + 1] = bytes; if (pubs[i]) bytes += pub_lens[i]; }
    const size_t o_out = (bytes + 255) & ~(size_t)255, total = o_out + 2 * n * 4;
    if ((rc = L.host_stage.ensure(total))) return rc;
    uint8_t *blob = (uint8_t *)L.host_stage.p;
    uint64_t *tab = (uint64_t *)blob;
    mb_parallel_for(n, [&](size_t i) {
        tab[i] = proofs[i] ? at[2 * i] : ~0ull; tab[n + i] = proofs[i] ? proof_lens[i] : 0;
        tab[2 * n + i] = pubs[i] ? at[2 * i + 1] : ~0ull; tab[3 * n + i] = pubs[i] ? pub_lens[i] : 0;
        if (proofs[i]) memcpy(blob + at[2 * i], proofs[i], proof_lens[i]);
        if (pubs[i]) memcpy(blob + at[2 * i + 1], pubs[i], pub_lens[i]);
    });
    if ((rc = L.ac_in.ensure(total))) return rc;
    uint8_t *d = L.ac_in.as<uint8_t>();
    enq.lock();
    HIPC(hipMemcpyAsync(d, blob, bytes, hipMemcpyHostToDevice, L.stream));
    if ((rc = account_job_on_lane(c, n, d, bytes, d, d + n * 8, d + 2 * n * 8, d + 3 * n * 8, d + o_out, d + o_out + n * 4, nullptr, nullptr))) return rc;
    HIPC(hipMemcpyAsync(blob + o_out, d + o_out, 2 * n * 4, hipMemcpyDeviceToHost, L.stream));
    enq.unlock();
    HIPC(hipStreamSynchronize(L.stream));
    memcpy(passed, blob + o_out, n * 4); memcpy(ran, blob + o_out + n * 4, n * 4);
    return MINA_OK;
}
