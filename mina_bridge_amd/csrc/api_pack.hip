// api_pack.hip -- the opt-in device front end of a Proof-of-State job (state_pack.cuh): serialized protocol states in HBM -> records, field counts, `precheck`.
//
// mina_protocol_state_pack_dev is mina_protocol_state_pack for n states at once; mina_state_frontend_dev does for a batch of proofs what the boundary's host pool
// does per proof (api_verify.hip parse_states_half): split the 17 consecutive states, pack them, compare the ledger hashes, run chain selection.  Both queue on the
// next pipeline lane (or the pinned one) and never wait for the GPU.  The host path is their checker: outputs are bit-identical to it for every input.
#include "ctx.h"
#include "state_pack.cuh"

static constexpr size_t PACK_MAX_STATES = (size_t)1 << 22;

// n states on the current lane; info_pairs as pstate_pack_kernel
static int pstate_pack_on_lane(mina_ctx *c, size_t n, const void *d_blob, size_t blob_len, const void *d_off, const void *d_len, void *d_records, void *d_nfields,
                               void *d_info, uint32_t info_pairs, void *d_status) {
    mb::pstate_pack_kernel<<<cdiv(n, 256), 256, 0, c->L->stream>>>((uint32_t)n, (const uint8_t *)d_blob, (uint64_t)blob_len, (const uint64_t *)d_off, (const uint32_t *)d_len,
                                                                 (uint4 *)d_records, (uint32_t *)d_nfields, (uint32_t *)d_info, info_pairs, (uint8_t *)d_status);
    HIPC(hipGetLastError());
    return MINA_OK;
}

extern "C" int mina_protocol_state_pack_dev(mina_ctx *c, size_t n, const void *d_blob, size_t blob_len, const void *d_off, const void *d_len, void *d_records,
                                            void *d_nfields, void *d_info, void *d_status) {
    if (!c || (n && (!d_blob || !d_off || !d_len || !d_records || !d_nfields || !d_status))) return fail(MINA_ERR_ARG, "null argument");
    if (((uintptr_t)d_off & 7u) || ((uintptr_t)d_len & 3u) || ((uintptr_t)d_records & 15u) || ((uintptr_t)d_nfields & 3u) || ((uintptr_t)d_info & 3u))
        return fail(MINA_ERR_ARG, "misaligned argument: offsets 8, lengths / field counts / info 4, records 16 bytes");
    if (n > PACK_MAX_STATES) return fail(MINA_ERR_ARG, "n too large");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    if (n == 0) return MINA_OK;
    return pstate_pack_on_lane(c, n, d_blob, blob_len, d_off, d_len, d_records, d_nfields, d_info, 0, d_status);
}

int mb_state_frontend_on_lane(mina_ctx *c, size_t batch, const void *d_blob, size_t blob_len, const void *d_begin, const void *d_end, const void *d_expected_hashes,
                              const void *d_ledger_hashes, const void *d_and, void *d_records, void *d_nfields, void *d_precheck, void *d_masks) {
    Lane &L = *c->L;
    const size_t n = batch * MINA_STATES_PER_PROOF;
    int rc;
    if ((rc = L.pk_off.ensure(n * 8)) || (rc = L.pk_len.ensure(n * 4)) || (rc = L.pk_status.ensure(n)) || (rc = L.pk_info.ensure(2 * batch * sizeof(mina_protocol_state_info))) ||
        (rc = L.pk_fmt.ensure(batch))) return rc;
    mb::pstate_split_kernel<<<cdiv(batch, 256), 256, 0, L.stream>>>((uint32_t)batch, (const uint8_t *)d_blob, (uint64_t)blob_len, (const uint64_t *)d_begin, (const uint64_t *)d_end,
                                                                    L.pk_off.as<uint64_t>(), L.pk_len.as<uint32_t>(), L.pk_fmt.as<uint8_t>());
    if ((rc = pstate_pack_on_lane(c, n, d_blob, blob_len, L.pk_off.p, L.pk_len.p, d_records, d_nfields, L.pk_info.p, 1, L.pk_status.p))) return rc;
    mb::pstate_precheck_kernel<<<cdiv(batch, 128), 128, 0, L.stream>>>((uint32_t)batch, (const uint4 *)d_records, L.pk_status.as<uint8_t>(), L.pk_info.as<uint32_t>(),
                                                                       (const uint8_t *)d_expected_hashes, (const uint64_t *)d_ledger_hashes, (const uint8_t *)d_and,
                                                                       L.pk_fmt.as<uint8_t>(), (uint8_t *)d_precheck, (uint32_t *)d_masks);
    mb::pstate_clear_kernel<<<cdiv(n * (mb::PSTATE_REC_BYTES / 16), 256), 256, 0, L.stream>>>((uint32_t)batch, L.pk_fmt.as<uint8_t>(), (uint4 *)d_records, (uint32_t *)d_nfields);
    HIPC(hipGetLastError());
    return MINA_OK;
}

extern "C" int mina_state_frontend_dev(mina_ctx *c, size_t batch, const void *d_blob, size_t blob_len, const void *d_begin, const void *d_end, const void *d_expected_hashes,
                                       const void *d_ledger_hashes, const void *d_and, void *d_records, void *d_nfields, void *d_precheck, void *d_masks) {
    if (!c || (batch && (!d_blob || !d_begin || !d_end || !d_expected_hashes || !d_ledger_hashes || !d_records || !d_nfields || !d_precheck))) return fail(MINA_ERR_ARG, "null argument");
    if (((uintptr_t)d_begin & 7u) || ((uintptr_t)d_end & 7u) || ((uintptr_t)d_ledger_hashes & 7u) || ((uintptr_t)d_records & 15u) || ((uintptr_t)d_nfields & 3u) || ((uintptr_t)d_masks & 3u))
        return fail(MINA_ERR_ARG, "misaligned argument: begin / end / ledger hashes 8, field counts / masks 4, records 16 bytes");
    if (batch > PACK_MAX_STATES / MINA_STATES_PER_PROOF) return fail(MINA_ERR_ARG, "batch too large");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    if (batch == 0) return MINA_OK;
    return mb_state_frontend_on_lane(c, batch, d_blob, blob_len, d_begin, d_end, d_expected_hashes, d_ledger_hashes, d_and, d_records, d_nfields, d_precheck, d_masks);
}
