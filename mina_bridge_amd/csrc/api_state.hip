// api_state.hip -- the Proof-of-State job behind `verify_mina_state` (8f-1; BASELINE config C3).
//
// What the reference's verifier does per state proof (README.md:281-310; Aligned `verify_mina_state_ffi`, un-vendored):
//   1. hash the 16 candidate-chain protocol states and the bridge tip state (`MinaHash`: Poseidon over `to_input`, twice),
//      compare with the public inputs, check that the states form a chain                       -> pstate_hash_kernel + chain check
//   2. Pickles wrap verification of the tip proof:
//        public-input commitment (Lagrange MSM, Pallas)                                         -> mb_msm_table + pubcomm finish
//        Fiat-Shamir + combined IPA opening (k = 15)                                            -> mb_ipa_batch_check_dev
//        step accumulator check (Vesta, 2^16 bases)                                             -> mb_accumulator_check_dev
// All of it is queued on ONE lane with no host synchronisation between the stages; one verdict word per proof.
#include <chrono>
#include <optional>
#include "ctx.h"
#include "msm.cuh"
#include "sponge.cuh"
#include "lagrange.cuh"
#include "wire_state.h"
#include "state_dedup.cuh"
#include "state_masks.h"

namespace mb {

template <int F> __device__ __forceinline__ fe_t ld_fe(const uint32_t *p) { fe_t r; for (int i = 0; i < 8; ++i) r.v[i] = p[i]; return r; }

// `MinaHash(ProtocolState)`: body = H_{"MinaProtoStateBody"}(fields[1 .. 1+nf)); hash = H_{"MinaProtoState"}(fields[0], body).
// One lane group (8 lanes, or a wave-packed triple for chip-filling batches) per state; record = MINA_PSTATE_SLOTS field elements, canonical words.
// The sponge of one state, shared by pstate_hash_kernel (hash `sp` is that of record `sp`) and pstate_hash_uniq_kernel (of record uniq[sp]): `rec` / `nf` = the group's
// record and its clamped field count; the `live && writer` lanes write hash `sp`.
template <int F, int LANES>
__device__ __forceinline__ void pstate_sponge(const bool live, const bool writer, const uint32_t e, const uint32_t sp, const uint32_t *__restrict__ rec, const uint32_t nf,
                                              const FieldK &fk, const PoseidonParams *__restrict__ pp, const fe_t *__restrict__ salts, uint32_t *__restrict__ out_hash,
                                              uint32_t *__restrict__ out_body) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (LANES == 3) {
        // The chip-filling form keeps the state in the 29-bit form (x 2^261, lazily reduced) from the first absorb to the last squeeze: a field enters by ONE signed-digit
        // product with 2^522 mod p -- both fields of a block at once, each on the lane that owns its state element; a lane with nothing to absorb multiplies zero, which
        // gives a multiple of p -- instead of a Montgomery conversion per field (two divergent ones per permutation) and a product into and out of the 29-bit form around
        // every permutation: ~ 600 of the ~ 51 500 instructions of a permutation.  Bounds: tools/fe29_bounds.py prove_sponge_rounds (row + absorbed field < 4.1 p).
        const TriPos tp = tri_pos();
        const PoseidonParams29 *__restrict__ q = pparams29_of(pp);
        auto field29 = [&](const uint32_t *w, bool take) {           // (words)(2^522) / 2^261; nothing to take: a multiple of p
            fe_t v = fe_zero();
            if (take) v = ld_fe<F>(w);
            return fe29_mul_sg<F>(fe29_from_words(v), q->absorb);
        };
        fe29_t x = fe29_mul_asm<F>(fe29_from_words(salts[e]), q->enter);
        const uint32_t nblk = (nf + 1) / 2;
#pragma unroll 1
        for (uint32_t k = 0; k < nblk; ++k) {
            if (k) poseidon_rounds_tri<F>(x, q, tp);
            const uint32_t el = 2 * k + e;
            x = fe29_add(x, field29(rec + (size_t)(1 + el) * 8, e < 2 && el < nf));
        }
        poseidon_rounds_tri<F>(x, q, tp);
        const fe29_t body29 = tri_bcast29(x, tp.base);               // state element 0, still x 2^261, below 2.07 p
        fe29_t y = fe29_mul_asm<F>(fe29_from_words(salts[3 + e]), q->enter);
        fe29_t add = field29(rec, e == 0);
        if (e == 1) add = body29;
        y = fe29_add(y, add);
        poseidon_rounds_tri<F>(y, q, tp);
        if (live) {                                                  // out of the 29-bit form once per state (element 0 lives on the writer lane)
            if (writer) {
                const fe_t w = fe_from_mont<F>(fe_cond_sub_p<F>(fe29_to_words(fe29_mul_asm<F>(y, q->leave)))); for (int i = 0; i < 8; ++i) out_hash[(size_t)sp * 8 + i] = w.v[i];
                if (out_body) { const fe_t bw = fe_from_mont<F>(fe_cond_sub_p<F>(fe29_to_words(fe29_mul_asm<F>(x, q->leave)))); for (int i = 0; i < 8; ++i) out_body[(size_t)sp * 8 + i] = bw.v[i]; }
            }
        }
        return;
    }
#endif
    fe_t s = salts[e];
    uint32_t count = 0;
    for (uint32_t el = 0; el < nf; ++el) {
        if (count == 2) { poseidon_permute_coop<F, LANES>(s, pp); count = 0; }
        if (e == count) s = fe_add<F>(s, fe_to_mont<F>(ld_fe<F>(rec + (size_t)(1 + el) * 8), fk.r2));
        ++count;
    }
    poseidon_permute_coop<F, LANES>(s, pp);
    const fe_t body = coop_get<LANES>(s, 0);
    s = salts[3 + e];
    if (e == 0) s = fe_add<F>(s, fe_to_mont<F>(ld_fe<F>(rec), fk.r2));
    if (e == 1) s = fe_add<F>(s, body);
    poseidon_permute_coop<F, LANES>(s, pp);
    s = coop_get<LANES>(s, 0);
    if (live && writer) {
        const fe_t w = fe_from_mont<F>(s); for (int i = 0; i < 8; ++i) out_hash[(size_t)sp * 8 + i] = w.v[i];
        if (out_body) { const fe_t bw = fe_from_mont<F>(body); for (int i = 0; i < 8; ++i) out_body[(size_t)sp * 8 + i] = bw.v[i]; }
    }
}

template <int F, int LANES>
// LANES == 3: five waves per SIMD (96 VGPRs) as before the signed-digit forms, whose digits pin the low halves of register pairs (100 VGPRs unasked): the three values
// the allocator parks in scratch are touched outside the round loops only (pinned from the code object: tests/test_code_object.py::test_dominant_kernel_round_loops)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LANES == 3 ? 5 : 1, LANES == 3 ? 5 : 8)))
pstate_hash_kernel(uint32_t n, FieldK fk, const PoseidonParams *__restrict__ pp, const fe_t *__restrict__ salts /* [0..3) body, [3..6) state */,
                   const uint32_t *__restrict__ records, const uint32_t *__restrict__ nfields, uint32_t *__restrict__ out_hash /* n*8 */,
                   uint32_t *__restrict__ out_body /* n*8 or null */) {
    bool writer;
    const uint32_t sp = coop_sponge_index<LANES>(writer), e = coop_elem<LANES>();
    const bool live = sp < n;
    const uint32_t idx = live ? sp : 0;                            // dead groups shadow state 0 (whole waves run the cross-lane moves)
    const uint32_t *rec = records + (size_t)idx * MINA_PSTATE_SLOTS * 8;
    uint32_t nf = nfields[idx]; if (nf > MINA_PSTATE_SLOTS - 1) nf = MINA_PSTATE_SLOTS - 1;
    pstate_sponge<F, LANES>(live, writer, e, sp, rec, nf, fk, pp, salts, out_hash, out_body);
}

// The deduplicated state leg (state_dedup.cuh; pstate_hash_dedup_dev): states [lo, lo + cnt) of the DISTINCT records, hash `sp` = that of record uniq[sp].  The number
// of distinct records `*m` is known on the device only: the grid covers the upper bound, a workgroup whose first state is past `*m` returns at once.
template <int F, int LANES>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LANES == 3 ? 5 : 1, LANES == 3 ? 5 : 8)))
pstate_hash_uniq_kernel(uint32_t lo, uint32_t cnt, const uint32_t *__restrict__ m, const uint32_t *__restrict__ uniq, FieldK fk, const PoseidonParams *__restrict__ pp,
                        const fe_t *__restrict__ salts, const uint32_t *__restrict__ records, const uint32_t *__restrict__ nfields, uint32_t *__restrict__ out_hash /* by position in uniq */,
                        uint32_t *__restrict__ out_body /* likewise, or null */) {
    const uint32_t end = min(lo + cnt, *m);
    if (lo + blockIdx.x * (LANES == 3 ? (blockDim.x >> 6) * 21u : blockDim.x / LANES) >= end) return;
    bool writer;
    const uint32_t sp = lo + coop_sponge_index<LANES>(writer), e = coop_elem<LANES>();
    const bool live = sp < end;
    const uint32_t idx = uniq[live ? sp : lo];                     // dead groups shadow the piece's first state (whole waves run the cross-lane moves)
    const uint32_t *rec = records + (size_t)idx * MINA_PSTATE_SLOTS * 8;
    uint32_t nf = nfields[idx]; if (nf > MINA_PSTATE_SLOTS - 1) nf = MINA_PSTATE_SLOTS - 1;
    asm volatile("" : "+v"(rec));                                  // from here on the compiler knows the address only, not the index it came from
    const uint32_t at = (uint32_t)((size_t)(rec - records) / (MINA_PSTATE_SLOTS * 8));
    pstate_sponge<F, LANES>(live, writer, e, at, rec, nf, fk, pp, salts, out_hash, out_body);
}

// The same hashes, ONE lane per state (64 per wave) -- the largest batches (pstate_hash_dev).  The whole sponge state lives on its lane in the 29-bit form from the first
// absorb to the last squeeze, as in the 3-lane form; the rounds use the diagonal-normalised rows (sponge.cuh poseidon_rounds_one): no cross-lane move, the row
// constants in SGPRs: 2103 multiply-accumulates per sponge-round in the build's code object (2106 written: the first product of a column starts its accumulator) against
// 2322.  Five waves per SIMD (91 VGPRs; amdgpu_waves_per_eu caps them at 96): the three S-box chains of a lane hide each other's latency.
static constexpr uint32_t PSTATE_HASH1_WAVES = 5;
// the sponge of one lane's state, shared by pstate_hash1_kernel and pstate_hash1_uniq_kernel: hash `sp` from record `rec` with `nf` (clamped) body fields
template <int F>
__device__ __forceinline__ void pstate_sponge1(const uint32_t sp, const uint32_t *__restrict__ rec, const uint32_t nf, const PoseidonParams *__restrict__ pp,
                                               const fe_t *__restrict__ salts, uint32_t *__restrict__ out_hash, uint32_t *__restrict__ out_body) {
#if defined(__HIP_DEVICE_COMPILE__)
    const PoseidonParams29 *__restrict__ q = pparams29_of(pp);
    const PoseidonRows1 *__restrict__ q1 = prows1_of(pp);
    auto field29 = [&](const uint32_t *w) { return fe29_mul_sg<F>(fe29_from_words(ld_fe<F>(w)), q->absorb); };   // (words)(2^522) / 2^261 = x 2^261
    fe29_t x[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) x[e] = fe29_mul_asm<F>(fe29_from_words(salts[e]), q->enter);
    const uint32_t nblk = (nf + 1) / 2;
#pragma unroll 1
    for (uint32_t k = 0; k < nblk; ++k) {
        if (k) poseidon_rounds_one<F>(x, q1);
        x[0] = fe29_add(x[0], field29(rec + (size_t)(1 + 2 * k) * 8));
        if (2 * k + 1 < nf) x[1] = fe29_add(x[1], field29(rec + (size_t)(2 + 2 * k) * 8));
    }
    poseidon_rounds_one<F>(x, q1);
    fe29_t y[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) y[e] = fe29_mul_asm<F>(fe29_from_words(salts[3 + e]), q->enter);
    y[0] = fe29_add(y[0], field29(rec));
    y[1] = fe29_add(y[1], x[0]);                                     // the body hash, still x 2^261
    poseidon_rounds_one<F>(y, q1);
    const fe_t w = fe_from_mont<F>(fe_cond_sub_p<F>(fe29_to_words(fe29_mul_asm<F>(y[0], q->leave)))); for (int i = 0; i < 8; ++i) out_hash[(size_t)sp * 8 + i] = w.v[i];
    if (out_body) { const fe_t bw = fe_from_mont<F>(fe_cond_sub_p<F>(fe29_to_words(fe29_mul_asm<F>(x[0], q->leave)))); for (int i = 0; i < 8; ++i) out_body[(size_t)sp * 8 + i] = bw.v[i]; }
#else
    (void)sp; (void)rec; (void)nf; (void)pp; (void)salts; (void)out_hash; (void)out_body;
#endif
}
template <int F>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PSTATE_HASH1_WAVES, PSTATE_HASH1_WAVES)))
pstate_hash1_kernel(uint32_t n, const PoseidonParams *__restrict__ pp, const fe_t *__restrict__ salts /* [0..3) body, [3..6) state */,
                    const uint32_t *__restrict__ records, const uint32_t *__restrict__ nfields, uint32_t *__restrict__ out_hash /* n*8 */,
                    uint32_t *__restrict__ out_body /* n*8 or null */) {
    const uint32_t sp = blockIdx.x * blockDim.x + threadIdx.x;
    if (sp >= n) return;                                             // nothing crosses lanes: a dead lane just leaves
    const uint32_t *rec = records + (size_t)sp * MINA_PSTATE_SLOTS * 8;
    uint32_t nf = nfields[sp]; if (nf > MINA_PSTATE_SLOTS - 1) nf = MINA_PSTATE_SLOTS - 1;
    pstate_sponge1<F>(sp, rec, nf, pp, salts, out_hash, out_body);
}
// ... of the distinct records only (see pstate_hash_uniq_kernel): a lane past `*m` leaves, so a workgroup whose first state is past it returns at once
template <int F>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PSTATE_HASH1_WAVES, PSTATE_HASH1_WAVES)))
pstate_hash1_uniq_kernel(uint32_t lo, uint32_t cnt, const uint32_t *__restrict__ m, const uint32_t *__restrict__ uniq, const PoseidonParams *__restrict__ pp,
                         const fe_t *__restrict__ salts, const uint32_t *__restrict__ records, const uint32_t *__restrict__ nfields, uint32_t *__restrict__ out_hash,
                         uint32_t *__restrict__ out_body) {
    const uint32_t sp = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (sp >= min(lo + cnt, *m)) return;
    const uint32_t idx = uniq[sp];
    const uint32_t *rec = records + (size_t)idx * MINA_PSTATE_SLOTS * 8;
    uint32_t nf = nfields[idx]; if (nf > MINA_PSTATE_SLOTS - 1) nf = MINA_PSTATE_SLOTS - 1;
    pstate_sponge1<F>(idx, rec, nf, pp, salts, out_hash, out_body);                          // the hash goes to the record's own place
}

// salts of the hash prefixes: state after absorbing the prefix element into the zero state and permuting (3 elements each)
template <int F>
__global__ void prefix_salt_kernel(uint32_t n, FieldK fk, const PoseidonParams *__restrict__ pp, const uint32_t *__restrict__ prefixes, fe_t *__restrict__ salts) {
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= n) return;
    fe_t s[3] = {fe_to_mont<F>(ld_fe<F>(prefixes + (size_t)h * 8), fk.r2), fe_zero(), fe_zero()};
    poseidon_permute<F>(s, pp);
    for (int j = 0; j < 3; ++j) salts[(size_t)h * 3 + j] = s[j];
}

// README.md:283-288 per proof: hashes of the 16 chain states and of the bridge tip state equal the public inputs, and
// state i+1 names state i as its predecessor.  One lane per proof (pure comparisons).
__global__ void pstate_chain_check_kernel(uint32_t batch, const uint32_t *__restrict__ hashes /* b*17*8 */, const uint32_t *__restrict__ expected /* b*17*8 */,
                                          const uint32_t *__restrict__ records, const uint8_t *__restrict__ precheck /* b or null */, uint32_t *__restrict__ ok) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    bool good = precheck ? precheck[b] != 0 : true;
    const uint32_t *h = hashes + (size_t)b * MINA_STATES_PER_PROOF * 8, *x = expected + (size_t)b * MINA_STATES_PER_PROOF * 8;
    for (uint32_t i = 0; i < MINA_STATES_PER_PROOF * 8; ++i) good = good && (h[i] == x[i]);
    for (uint32_t s = 1; s < MINA_STATES_PER_PROOF - 1; ++s) {          // candidate chain: states 0..15 (oldest .. tip); 16 = bridge tip (not linked)
        const uint32_t *prev = records + ((size_t)b * MINA_STATES_PER_PROOF + s) * MINA_PSTATE_SLOTS * 8;   // slot 0 = previous_state_hash
        for (int i = 0; i < 8; ++i) good = good && (prev[i] == h[(s - 1) * 8 + i]);
    }
    ok[b] = good ? 1u : 0u;
}

// public-input commitment h - A as canonical affine words (16 per proof, zeros = infinity): feeds ipa_prepare_kernel's override slot
// (Inv: the inversion by the power, FeInvPow, or by divsteps, FeInvGcd -- pubcomm_finish16_gcd_kernel under mina_ctx_set_chain_inverse; fe_modinv.cuh)
template <int FB, class Inv>
__device__ __forceinline__ void pubcomm_finish16_body(uint32_t batch, const FieldK &kb, const affine_t *__restrict__ h, const xyzz_t *__restrict__ a, uint32_t *__restrict__ out_words) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= batch) return;
    xyzz_t t = a[m];
    t.y = fe_neg<FB>(t.y);
    const affine_t H = *h;
    xyzz_add_affine<FB>(t, H.x, H.y, kb.one);
    uint32_t *o = out_words + (size_t)m * 16;
    if (xyzz_is_inf(t)) { for (int i = 0; i < 16; ++i) o[i] = 0; return; }
    const fe_t zi = Inv::template inv<FB>(fe_mul<FB>(t.zz, t.zzz), kb);
    const fe_t x = fe_from_mont<FB>(fe_mul<FB>(t.x, fe_mul<FB>(zi, t.zzz))), y = fe_from_mont<FB>(fe_mul<FB>(t.y, fe_mul<FB>(zi, t.zz)));
    for (int i = 0; i < 8; ++i) { o[i] = x.v[i]; o[8 + i] = y.v[i]; }
}
template <int FB>
__global__ void __launch_bounds__(64)
pubcomm_finish16_kernel(uint32_t batch, FieldK kb, const affine_t *__restrict__ h, const xyzz_t *__restrict__ a, uint32_t *__restrict__ out_words) { mb_wave_prio();
    pubcomm_finish16_body<FB, FeInvPow>(batch, kb, h, a, out_words);
}
template <int FB>
__global__ void __launch_bounds__(64)
pubcomm_finish16_gcd_kernel(uint32_t batch, FieldK kb, const affine_t *__restrict__ h, const xyzz_t *__restrict__ a, uint32_t *__restrict__ out_words) { mb_wave_prio();
    pubcomm_finish16_body<FB, FeInvGcd>(batch, kb, h, a, out_words);
}

__global__ void fill_u32_kernel(uint32_t n, uint32_t v, uint32_t *__restrict__ out) { const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) out[i] = v; }

// verdict[b] = chain_ok[b] AND folded IPA verdict AND folded accumulator verdict; flags = {ipa, ipa malformed, acc, 0}
__global__ void state_job_verdict_kernel(uint32_t batch, const uint32_t *__restrict__ chain_ok, const uint32_t *__restrict__ ipa_v /* [2] or null */,
                                         const uint32_t *__restrict__ acc_v /* [1] or null */, const uint32_t *__restrict__ kimchi_bad /* [1] or null */,
                                         const uint32_t *__restrict__ stmt_ok /* [batch] or null: Pickles statement well-formed */,
                                         uint32_t *__restrict__ verdicts, uint32_t *__restrict__ flags, uint32_t *__restrict__ stmt_out /* [batch] or null: copy of stmt_ok */) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t kb = kimchi_bad ? kimchi_bad[0] : 0u;
    const uint32_t iv = (ipa_v ? ipa_v[0] : 1u) && !kb, av = acc_v ? acc_v[0] : 1u;
    if (b == 0 && flags) { flags[0] = iv; flags[1] = (ipa_v ? ipa_v[1] : 0u) | kb; flags[2] = av; flags[3] = 0u; }
    if (b < batch) { const uint32_t so = stmt_ok ? stmt_ok[b] : 1u; verdicts[b] = (chain_ok[b] && iv && av && so) ? 1u : 0u; if (stmt_out) stmt_out[b] = so; }
}

// ---- the masks form of the job (state_job_checks below; the rule: state_masks.h).  Both kernels: one lane per proof, pure comparisons and bit operations.
// pstate_chain_check_kernel's comparisons with their own word per proof: chain[b] = the 17 hashes equal the expected ones and states 1..15 name their predecessor.
// `precheck` is not read: the host checks have their own bits in the masks.
__global__ void __launch_bounds__(64)
pstate_chain_detail_kernel(uint32_t batch, const uint32_t *__restrict__ hashes /* b*17*8 */, const uint32_t *__restrict__ expected /* b*17*8 */,
                           const uint32_t *__restrict__ records, uint32_t *__restrict__ chain) { mb_wave_prio();
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    bool good = true;
    const uint32_t *h = hashes + (size_t)b * MINA_STATES_PER_PROOF * 8, *x = expected + (size_t)b * MINA_STATES_PER_PROOF * 8;
    for (uint32_t i = 0; i < MINA_STATES_PER_PROOF * 8; ++i) good = good && (h[i] == x[i]);
    for (uint32_t s = 1; s < MINA_STATES_PER_PROOF - 1; ++s) {          // candidate chain: states 0..15 (oldest .. tip); 16 = bridge tip (not linked)
        const uint32_t *prev = records + ((size_t)b * MINA_STATES_PER_PROOF + s) * MINA_PSTATE_SLOTS * 8;   // slot 0 = previous_state_hash
        for (int i = 0; i < 8; ++i) good = good && (prev[i] == h[(s - 1) * 8 + i]);
    }
    chain[b] = good ? 1u : 0u;
}

// passed[b] / ran[b] = state_masks_of(what the job left in HBM about proof b).  sections: bit 0 with_states, bit 1 with_accumulator, bit 2 with_ipa.  front / deny /
// chain may be null (absent / 0 / no state leg); ipa_each / acc_each null = nobody is a culprit (both folded checks passed).
__global__ void __launch_bounds__(64)
state_job_masks_kernel(uint32_t batch, uint32_t sections, const uint32_t *__restrict__ front, const uint32_t *__restrict__ deny, const uint32_t *__restrict__ chain,
                       const uint32_t *__restrict__ stmt, const uint32_t *__restrict__ ipa_each, const uint32_t *__restrict__ acc_each, uint32_t *__restrict__ passed,
                       uint32_t *__restrict__ ran) { mb_wave_prio();
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const StateMasks m = state_masks_of(front != nullptr, front ? front[b] : 0u, deny ? deny[b] : 0u, (sections & 1u) != 0, (sections & 2u) != 0, (sections & 4u) != 0,
                                        chain ? chain[b] != 0 : true, stmt[b] != 0, ipa_each ? ipa_each[b] != 0 : true, acc_each ? acc_each[b] != 0 : true);
    passed[b] = m.passed; ran[b] = m.ran;
}

}  // namespace mb

// ------------------------------------------------------------------------------------------------ salts
static int ensure_state_salts(mina_ctx *c) {
    if (c->have_state_salts) return MINA_OK;
    if (!c->have_pparams[FIELD_FP]) return fail(MINA_ERR_STATE, "Poseidon constants not installed for Fp");
    const char *names[MB_N_PREFIX_SALTS] = {"MinaProtoStateBody", "MinaProtoState", "MinaAccount", "MinaZkappAccount", "MinaZkappUri", "MinaSideLoadedVk"};
    uint8_t pre[MB_N_PREFIX_SALTS * 32];
    for (int i = 0; i < MB_N_PREFIX_SALTS; ++i) { const mw::B32 f = mw::prefix_field(names[i]); memcpy(pre + 32 * i, f.b, 32); }
    int rc;
    if ((rc = c->state_salts.ensure(MB_N_PREFIX_SALTS * 3 * sizeof(fe_t)))) return rc;
    DevBuf tmp;
    if ((rc = tmp.ensure(sizeof pre))) return rc;
    HIPC(hipMemcpyAsync(tmp.p, pre, sizeof pre, hipMemcpyHostToDevice, c->L->stream));
    mb::prefix_salt_kernel<FIELD_FP><<<1, 64, 0, c->L->stream>>>(MB_N_PREFIX_SALTS, c->fk[FIELD_FP], c->pparams[FIELD_FP].as<PoseidonParams>(), tmp.as<uint32_t>(), c->state_salts.as<fe_t>());
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(c->L->stream));
    c->have_state_salts = true;
    return MINA_OK;
}

int mb_ensure_state_salts(mina_ctx *c) { return ensure_state_salts(c); }

// The launches of `n` state hashes of a leg of `leg` states on the current lane, in the lane form of the leg (ctx.h pstate_hash_lanes) and in the pieces and behind the
// LDS reservation of `hl`.  Without `u`: records [0, n) -> hashes [0, n).  With it: the distinct records uniq[0 .. *m) of the `n`, each hash to its record's own place;
// `*m` is known on the device only, so the grids cover `n` and the pieces past the distinct count are empty launches.
struct UniqList { const uint32_t *m, *uniq; };
static int pstate_hash_launch(mina_ctx *c, size_t n, size_t leg, HashLaunch hl, const uint32_t *d_records, const uint32_t *d_nfields, uint32_t *d_hashes, uint32_t *d_bodies,
                              const UniqList *u) {
    const PoseidonParams *pp = c->pparams[FIELD_FP].as<PoseidonParams>();
    const fe_t *salts = c->state_salts.as<fe_t>();
    hipStream_t stream = c->L->stream;
    // below ~8 k states the chip is latency-bound: 8 lanes per state (shortest chain); above, wave-packed triples (63 of 64 lanes busy); with several
    // jobs in flight and HASH1_MIN_STATES between them, one lane per state (ctx.h pstate_hash_lanes)
    return with_lanes<1, 16, 8, 3>(pstate_hash_lanes(c, n, leg), [&](auto lanes) {
        constexpr int LN = decltype(lanes)::value;
        constexpr bool wide = LN == 1 || LN == 3;             // the chip-filling forms
        std::optional<ProfScope> ps1_;
        if (LN == 1) ps1_.emplace(c, PS_STATE_HASH1);
        // A whole chip-filling launch would hold every wave slot its VGPRs allow (5 per SIMD in the 3-lane form) for most of its 20 ms, and the kernels of
        // the other legs / chunks of a call (a few hundred waves each, one behind the other) would wait for slots.  In pieces of `hl.piece_waves` waves
        // (~2 per SIMD: the multiplier is still saturated) the rest of the register file stays free for them.
        const size_t per = wide && hl.piece_waves ? hash_piece_states(c, leg, hl.piece_waves) : n;
        const uint32_t lds = wide ? hl.lds_bytes : 0;
        for (size_t lo = 0; lo < n; lo += per) {
            const size_t cnt = std::min(per, n - lo);
            const uint32_t grid = cdiv(coop_threads<LN>(cnt), 256);      // (one lane per state: a thread each)
            if (u) {
                if constexpr (LN == 1) mb::pstate_hash1_uniq_kernel<FIELD_FP><<<grid, 256, lds, stream>>>((uint32_t)lo, (uint32_t)cnt, u->m, u->uniq, pp, salts, d_records, d_nfields, d_hashes, d_bodies);
                else mb::pstate_hash_uniq_kernel<FIELD_FP, LN><<<grid, 256, lds, stream>>>((uint32_t)lo, (uint32_t)cnt, u->m, u->uniq, c->fk[FIELD_FP], pp, salts, d_records, d_nfields, d_hashes, d_bodies);
                continue;
            }
            const uint32_t *rec = d_records + lo * MINA_PSTATE_SLOTS * 8, *nf = d_nfields + lo;
            uint32_t *hash = d_hashes + lo * 8, *body = d_bodies ? d_bodies + lo * 8 : nullptr;
            if constexpr (LN == 1) mb::pstate_hash1_kernel<FIELD_FP><<<grid, 256, lds, stream>>>((uint32_t)cnt, pp, salts, rec, nf, hash, body);
            else mb::pstate_hash_kernel<FIELD_FP, LN><<<grid, 256, lds, stream>>>((uint32_t)cnt, c->fk[FIELD_FP], pp, salts, rec, nf, hash, body);
        }
        HIPC(hipGetLastError());
        return MINA_OK;
    });
}

// `n` states of a leg of `leg` states (a piece of it, or all of it): the form follows the leg (ctx.h hash_one_lane), so that callers that cut a leg into
// pieces (hash_piece_states) and this function agree on it
int pstate_hash_dev(mina_ctx *c, size_t n, size_t leg, HashLaunch hl, const uint32_t *d_records, const uint32_t *d_nfields, uint32_t *d_hashes, uint32_t *d_bodies) {
    ProfScope ps_(c, PS_STATE_HASH);
    return pstate_hash_launch(c, n, leg, hl, d_records, d_nfields, d_hashes, d_bodies, nullptr);
}

// ------------------------------------------------------------------------------------------------ the deduplicated state leg (state_dedup.cuh)
// rep[] and {n_distinct, n_collisions} of `n` records, queued on the current lane with its table; with `d_uniq` the ascending list of the representatives as well.
// `totals`: the context's running {distinct, collisions}, or null.
static int pstate_dedup_group_dev(mina_ctx *c, size_t n, const uint32_t *d_records, const uint32_t *d_nfields, uint32_t fingerprint_bits, uint32_t *d_rep, uint32_t *d_counts,
                                  uint32_t *d_uniq, unsigned long long *totals) {
    Lane &L = *c->L;
    if ((uintptr_t)d_records & 15u) return fail(MINA_ERR_ARG, "deduplication reads the records 16 bytes at a time: the pointer must be 16-byte aligned");
    size_t slots = 64; while (slots < 2 * n) slots <<= 1;              // at most half full
    const uint32_t ntiles = cdiv(n, mb::DEDUP_SCAN_TILE);
    int rc;
    if ((rc = L.dd_table.ensure(slots * sizeof(mb::DedupSlot))) || (rc = L.dd_counts.ensure((4 + (size_t)ntiles) * 4))) return rc;
    uint32_t *tiles = L.dd_counts.as<uint32_t>() + 4;
    HIPC(hipMemsetAsync(L.dd_table.p, 0xff, slots * sizeof(mb::DedupSlot), L.stream));     // word = empty, min = 2^32 - 1
    HIPC(hipMemsetAsync(d_counts, 0, 8, L.stream));
    mb::pstate_dedup_group_kernel<<<cdiv(n * mb::DEDUP_SUB, 256), 256, 0, L.stream>>>((uint32_t)n, (uint32_t)(slots - 1), fingerprint_bits, d_records, d_nfields,
                                                                                      L.dd_table.as<mb::DedupSlot>(), d_rep, d_counts);
    mb::pstate_dedup_rep_kernel<<<ntiles, mb::DEDUP_SCAN_BLOCK, 0, L.stream>>>((uint32_t)n, L.dd_table.as<mb::DedupSlot>(), d_rep, tiles);
    mb::pstate_dedup_scan_kernel<<<1, mb::DEDUP_SCAN_BLOCK, 0, L.stream>>>(ntiles, tiles, d_counts, totals);
    if (d_uniq) mb::pstate_dedup_compact_kernel<<<ntiles, mb::DEDUP_SCAN_BLOCK, 0, L.stream>>>((uint32_t)n, d_rep, tiles, d_uniq);
    HIPC(hipGetLastError());
    return MINA_OK;
}

// pstate_hash_dev with every distinct record hashed once: group, hash the representatives through uniq[] in the lane form pstate_hash_dev would take for `n` of `leg`
// (the distinct count is known on the device only: the grids cover `n`, workgroups past the count return at once) straight into the representatives' places of
// `d_hashes`, copy every other record's hash from its representative's.  Everything on the current lane's stream, in its dd_* buffers; no host synchronisation.
// `d_hashes` (and `d_bodies`) must be 16-byte aligned.
int pstate_hash_dedup_dev(mina_ctx *c, size_t n, size_t leg, HashLaunch hl, const uint32_t *d_records, const uint32_t *d_nfields, uint32_t *d_hashes, uint32_t *d_bodies, bool count) {
    Lane &L = *c->L;
    ProfScope ps_(c, PS_STATE_HASH);
    int rc;
    if ((rc = L.dd_rep.ensure(n * 4)) || (rc = L.dd_uniq.ensure(n * 4)) ||
        (rc = L.dd_counts.ensure((4 + (size_t)cdiv(n, mb::DEDUP_SCAN_TILE)) * 4))) return rc;      // (its full size here: pstate_dedup_group_dev must not move the counters it is handed)
    if ((rc = pstate_dedup_group_dev(c, n, d_records, d_nfields, 0, L.dd_rep.as<uint32_t>(), L.dd_counts.as<uint32_t>(), L.dd_uniq.as<uint32_t>(),
                                     count ? c->dedup_totals.as<unsigned long long>() : nullptr))) return rc;
    if (count) c->dedup_states += n;
    const UniqList u{L.dd_counts.as<uint32_t>(), L.dd_uniq.as<uint32_t>()};
    if ((rc = pstate_hash_launch(c, n, leg, hl, d_records, d_nfields, d_hashes, d_bodies, &u))) return rc;
    mb::pstate_dedup_scatter_kernel<<<cdiv(2 * n, 256), 256, 0, L.stream>>>((uint32_t)n, L.dd_rep.as<uint32_t>(), d_hashes, d_bodies);
    HIPC(hipGetLastError());
    return MINA_OK;
}

extern "C" int mina_ctx_set_state_dedup(mina_ctx *c, int on) {
    if (!c) return fail(MINA_ERR_ARG, "null ctx");
    HIPC(hipSetDevice(c->device));
    return mb_ctx_state_dedup(c, on != 0);
}
extern "C" int mina_ctx_state_dedup_stats(mina_ctx *c, uint64_t *states, uint64_t *distinct, uint64_t *collisions) {
    if (!c) return fail(MINA_ERR_ARG, "null ctx");
    int rc = mina_ctx_synchronize(c);
    if (rc) return rc;
    unsigned long long t[2] = {0, 0};
    if (c->dedup_totals.p) HIPC(hipMemcpy(t, c->dedup_totals.p, 16, hipMemcpyDeviceToHost));
    if (states) *states = c->dedup_states;
    if (distinct) *distinct = t[0];
    if (collisions) *collisions = t[1];
    return MINA_OK;
}

extern "C" int mina_protocol_state_dedup_dev(mina_ctx *c, size_t n, const void *d_records, const void *d_nfields, void *d_rep, void *d_counts, uint32_t fingerprint_bits) {
    if (!c || !d_counts || (n && (!d_records || !d_nfields || !d_rep))) return fail(MINA_ERR_ARG, "null argument");
    if (fingerprint_bits > 32) return fail(MINA_ERR_ARG, "fingerprint_bits must be 0 (the full fingerprint) or 1..32");
    if (n > ((size_t)1 << mb::DEDUP_OWNER_BITS)) return fail(MINA_ERR_ARG, "n too large");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    if (n == 0) { HIPC(hipMemsetAsync(d_counts, 0, 8, c->L->stream)); return MINA_OK; }
    return pstate_dedup_group_dev(c, n, (const uint32_t *)d_records, (const uint32_t *)d_nfields, fingerprint_bits, (uint32_t *)d_rep, (uint32_t *)d_counts, nullptr, nullptr);
}

// host-buffer hashes: upload, hash (with `dedup` each distinct record once; its count -> *n_distinct), download
static int pstate_hash_batch(mina_ctx *c, size_t n, const uint8_t *records, const uint32_t *n_body_fields, uint8_t *hashes_out, uint8_t *body_hashes_out, bool dedup, size_t *n_distinct) {
    if (!c || (n && (!records || !n_body_fields || !hashes_out))) return fail(MINA_ERR_ARG, "null argument");
    if (n_distinct) *n_distinct = 0;
    if (n == 0) return MINA_OK;
    if (n > (1u << 22)) return fail(MINA_ERR_ARG, "n too large");
    for (size_t i = 0; i < n; ++i) if (n_body_fields[i] > MINA_PSTATE_SLOTS - 1) return fail(MINA_ERR_ARG, "n_body_fields exceeds the record");
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = ensure_state_salts(c))) return rc;
    Lane &L = *c->L;
    if ((rc = h2d(c, L.tmp_a, records, n * MINA_PSTATE_SLOTS * 32))) return rc;
    if ((rc = h2d(c, L.tmp_b, n_body_fields, n * 4))) return rc;
    if ((rc = L.tmp_c.ensure(n * 32))) return rc;
    if ((rc = L.tmp_d.ensure(n * 32))) return rc;
    uint32_t *bodies = body_hashes_out ? L.tmp_d.as<uint32_t>() : nullptr;
    if ((rc = dedup ? pstate_hash_dedup_dev(c, n, n, HashLaunch{}, L.tmp_a.as<uint32_t>(), L.tmp_b.as<uint32_t>(), L.tmp_c.as<uint32_t>(), bodies, false)
                    : pstate_hash_dev(c, n, n, HashLaunch{}, L.tmp_a.as<uint32_t>(), L.tmp_b.as<uint32_t>(), L.tmp_c.as<uint32_t>(), bodies))) return rc;
    if (body_hashes_out) HIPC(hipMemcpyAsync(body_hashes_out, L.tmp_d.p, n * 32, hipMemcpyDeviceToHost, L.stream));
    uint32_t m = 0;
    if (dedup) HIPC(hipMemcpyAsync(&m, L.dd_counts.p, 4, hipMemcpyDeviceToHost, L.stream));
    if ((rc = d2h_sync(c, hashes_out, L.tmp_c, n * 32))) return rc;
    if (n_distinct) *n_distinct = m;
    return MINA_OK;
}
extern "C" int mina_protocol_state_hash_batch_dedup(mina_ctx *c, size_t n, const uint8_t *records, const uint32_t *n_body_fields, uint8_t *hashes_out,
                                                    uint8_t *body_hashes_out, size_t *n_distinct) {
    return pstate_hash_batch(c, n, records, n_body_fields, hashes_out, body_hashes_out, true, n_distinct);
}
extern "C" int mina_protocol_state_hash_batch(mina_ctx *c, size_t n, const uint8_t *records, const uint32_t *n_body_fields, uint8_t *hashes_out,
                                              uint8_t *body_hashes_out) {
    return pstate_hash_batch(c, n, records, n_body_fields, hashes_out, body_hashes_out, false, nullptr);
}

// convenience: serialized states in, state hashes out (parse on the host, hash on the GPU); malformed state -> MINA_ERR_FORMAT
extern "C" int mina_protocol_state_hash_bytes(mina_ctx *c, int encoding, size_t n, const uint8_t *const *states, const size_t *lens, uint8_t *hashes_out) {
    if (!c || (n && (!states || !lens || !hashes_out))) return fail(MINA_ERR_ARG, "null argument");
    std::vector<uint8_t> rec(n * MINA_PSTATE_SLOTS * 32); std::vector<uint32_t> nf(n);
    for (size_t i = 0; i < n; ++i) {
        if (!states[i]) return fail(MINA_ERR_ARG, "null state");
        int rc = mina_protocol_state_pack(states[i], lens[i], encoding, &rec[i * MINA_PSTATE_SLOTS * 32], &nf[i], nullptr, nullptr);
        if (rc) return rc;
    }
    return mina_protocol_state_hash_batch(c, n, rec.data(), nf.data(), hashes_out, nullptr);
}

// ------------------------------------------------------------------------------------------------ the composite job
int mb_pickles_check(mina_ctx *c, const mina_pickles_statements *s);                                                    // api_pickles.hip
size_t mb_pickles_sections(const mina_pickles_statements *s, const void ***slots, size_t *strides, mina_pickles_statements *copy);
int mb_check_jobs(mina_ctx *c, const mina_state_jobs *j) {
    if (!c || !j) return fail(MINA_ERR_ARG, "null argument");
    if (j->batch == 0 || j->batch > 65536) return fail(MINA_ERR_ARG, "batch must be in 1..65536");
    if (j->with_states && (!j->state_records || !j->state_nfields || !j->expected_hashes)) return fail(MINA_ERR_ARG, "null protocol-state section");
    if (j->with_ipa) {
        if (!j->lr || !j->delta || !j->sg || !j->z1 || !j->z2 || !j->rand_base || !j->sg_rand_base) return fail(MINA_ERR_ARG, "null IPA section");
        if (j->kimchi) {
            const mina_kimchi_proofs &kp = *j->kimchi;
            if (!c->have_kimchi) return fail(MINA_ERR_STATE, "no verifier index installed");
            if (kp.batch != j->batch || j->k != c->kimchi_log2 || j->log2_domain != c->kimchi_log2 || j->n_evalpoints != 2 || j->n_comms != kp.n_prev + 45 || kp.npub != j->npub || kp.n_prev > 8)
                return fail(MINA_ERR_ARG, "kimchi section does not match the installed index / the job's shape");
            if ((kp.n_prev && ((!kp.prev_chals && !kp.prev_prechallenges && !(kp.statements && kp.n_prev == 2 && j->k == 15)) || !kp.prev_comms)) || !kp.w_comm || !kp.z_comm || !kp.t_comm || !kp.evals || !kp.ft_eval1 || (kp.npub && !kp.public_inputs && !kp.statements)) return fail(MINA_ERR_ARG, "null kimchi section");
            if (kp.statements) { if (kp.npub != 40) return fail(MINA_ERR_ARG, "statements derive exactly 40 public inputs"); int prc = mb_pickles_check(c, kp.statements); if (prc) return prc; }
        } else if (!j->sponge_state || !j->sponge_pos || !j->cip || !j->evalscale || !j->polyscale || (j->n_evalpoints && !j->evalpoints) || (j->n_comms && !j->comms))
            return fail(MINA_ERR_ARG, "null IPA section");
        if (j->k < 1 || j->k > 20 || ((size_t)1 << j->k) > c->srs[CURVE_PALLAS].depth) return fail(c->srs[CURVE_PALLAS].depth ? MINA_ERR_ARG : MINA_ERR_STATE, "Pallas SRS missing or 2^k exceeds its depth");
        if (j->n_comms > 4096 || j->n_evalpoints > 64) return fail(MINA_ERR_ARG, "too many commitments / evaluation points");
        if (!c->have_pparams[FIELD_FP]) return fail(MINA_ERR_STATE, "Poseidon constants not installed for Fp");
    }
    if (j->npub) {
        if (!j->public_inputs && !(j->kimchi && j->kimchi->statements)) return fail(MINA_ERR_ARG, "null public inputs");
        if (!j->with_ipa || (!j->kimchi && j->pub_comm_slot >= j->n_comms)) return fail(MINA_ERR_ARG, "public-input commitment needs an IPA section and a valid commitment slot");
        if (j->log2_domain > 20 || ((uint64_t)1 << j->log2_domain) > c->srs[CURVE_PALLAS].depth || j->npub > 4096 || j->npub > ((uint64_t)1 << j->log2_domain)) return fail(MINA_ERR_ARG, "bad domain / npub");
    }
    if (j->with_accumulator) {
        if (!j->acc_prechallenges || !j->acc_sg || (j->batch > 1 && !j->acc_rho)) return fail(MINA_ERR_ARG, "null accumulator section");
        if (j->acc_k < 1 || j->acc_k > 20 || ((size_t)1 << j->acc_k) > c->srs[CURVE_VESTA].depth) return fail(c->srs[CURVE_VESTA].depth ? MINA_ERR_ARG : MINA_ERR_STATE, "Vesta SRS missing or 2^k exceeds its depth");
    }
    return MINA_OK;
}

int mb_ensure_lagrange_table(mina_ctx *c, int curve, uint32_t log2_domain, uint32_t npub);   // api_srs.hip
int mb_lagrange_sums_dev(mina_ctx *c, int curve, uint32_t npub, size_t batch, const uint32_t *d_scalars, void *d_out_xyzz);

// public-input commitments h - sum_i pub_i L_i of `batch` proofs as canonical affine words (16 per proof) on the current lane
int mb_pubcomm_dev(mina_ctx *c, size_t batch, uint32_t log2_domain, uint32_t npub, const uint32_t *d_pub, uint32_t *d_out16) {
    Lane &L = *c->L;
    SrsState &s = c->srs[CURVE_PALLAS];
    int rc;
    if ((rc = L.st_pub_xyzz.ensure(batch * sizeof(xyzz_t)))) return rc;
    if (npub == 0) {                                                // empty public input: A = infinity, commitment = h
        HIPC(hipMemsetAsync(L.st_pub_xyzz.p, 0, batch * sizeof(xyzz_t), L.stream));
    } else {
        if (s.lagrange_table_log2 != (int)log2_domain || s.lagrange_table_n < npub) return fail(MINA_ERR_STATE, "call mina_state_jobs_prepare(log2_domain, npub) first");
        if ((rc = mb_lagrange_sums_dev(c, CURVE_PALLAS, npub, batch, d_pub, L.st_pub_xyzz.p))) return rc;
    }
    if (c->gcd_launch()) mb::pubcomm_finish16_gcd_kernel<FIELD_FP><<<cdiv(batch, 64), 64, 0, L.stream>>>((uint32_t)batch, c->fk[FIELD_FP], s.h.as<affine_t>(), L.st_pub_xyzz.as<xyzz_t>(), d_out16);
    else mb::pubcomm_finish16_kernel<FIELD_FP><<<cdiv(batch, 64), 64, 0, L.stream>>>((uint32_t)batch, c->fk[FIELD_FP], s.h.as<affine_t>(), L.st_pub_xyzz.as<xyzz_t>(), d_out16);
    HIPC(hipGetLastError());
    return MINA_OK;
}

// everything that needs a host synchronisation (salts, Lagrange basis + its window table): done once, before the first job
extern "C" int mina_state_jobs_prepare(mina_ctx *c, uint32_t log2_domain, uint32_t npub) {
    if (!c) return fail(MINA_ERR_ARG, "null argument");
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = ensure_state_salts(c))) return rc;
    if (npub && (rc = mb_ensure_lagrange_table(c, CURVE_PALLAS, log2_domain, npub))) return rc;
    return MINA_OK;
}

// ---- what state_job.hip (the job's host orchestration) launches directly: one function per kernel, the same launch on the stream it is told
void mb_launch_pstate_chain_check(hipStream_t stream, uint32_t batch, const uint32_t *hashes, const uint32_t *expected, const uint32_t *records, const uint8_t *precheck, uint32_t *ok) {
    mb::pstate_chain_check_kernel<<<cdiv(batch, 64), 64, 0, stream>>>(batch, hashes, expected, records, precheck, ok);
}
void mb_launch_fill_u32(hipStream_t stream, uint32_t n, uint32_t v, uint32_t *out) { mb::fill_u32_kernel<<<cdiv(n, 256), 256, 0, stream>>>(n, v, out); }
void mb_launch_state_job_verdict(hipStream_t stream, uint32_t batch, const uint32_t *chain_ok, const uint32_t *ipa_v, const uint32_t *acc_v, const uint32_t *kimchi_bad,
                                 const uint32_t *stmt_ok, uint32_t *verdicts, uint32_t *flags, uint32_t *stmt_out) {
    mb::state_job_verdict_kernel<<<cdiv(batch, 64), 64, 0, stream>>>(batch, chain_ok, ipa_v, acc_v, kimchi_bad, stmt_ok, verdicts, flags, stmt_out);
}
void mb_launch_challenge_to_field_fq(hipStream_t stream, uint32_t n, FieldK fk, const uint32_t *chal, uint32_t *out_words) { challenge_to_field_kernel<FIELD_FQ><<<cdiv(n, 64), 64, 0, stream>>>(n, fk, chal, out_words); }

namespace {
struct Section { const void **slot; size_t bytes; };
// The culprit searches of a job on lane L whose folded checks failed (every pointer of `d` a device pointer): what state_job_each and state_job_checks share.
// malformed: word [1] of the failed job's flags (a malformed opening input: the rows it left cannot be re-checked).
struct CulpritSearch {
    mina_ctx *const c; Lane &L; const mina_state_jobs &d; const bool rows_ok;
    const uint8_t *d_net = nullptr;                    // a mixed job's bytes (StateJobPlan::d_net): a slice that re-queues the wrap-proof leg takes its own
    const size_t B = d.batch, k = d.k, m = d.n_comms, np = d.n_evalpoints;
    mina_kimchi_proofs kslice{}; mina_pickles_statements sslice{};
    // The opening leg of well-formed proofs does not repeat its transcripts: the prepared rows of the failed batch are still on their
    // lane and any slice of them is the folded check of that slice (mb_ipa_recheck_rows): a round costs a fold + two MSMs per part.
    CulpritSearch(mina_ctx *c_, Lane &L_, const mina_state_jobs &d_, bool malformed)
        : c(c_), L(L_), d(d_), rows_ok(!malformed && c_->ipa_rows && c_->ipa_rows_batch == d_.batch && !mb_tune().search_full) {}
    // proofs [lo, lo + cnt) of `src` as a job of their own, without the protocol-state leg
    mina_state_jobs slice(const mina_state_jobs &src, size_t lo, size_t cnt) {
        mina_state_jobs s = src; s.batch = cnt; s.with_states = 0; s.precheck = nullptr;
        auto adv = [&](const void *&p, size_t stride) { if (p) p = (const uint8_t *)p + lo * stride; };
        if (s.kimchi) {
            kslice = *s.kimchi; kslice.batch = cnt; s.kimchi = &kslice;
            adv(kslice.public_inputs, (size_t)kslice.npub * 32); adv(kslice.prev_chals, (size_t)kslice.n_prev * k * 32); adv(kslice.prev_prechallenges, (size_t)kslice.n_prev * k * 16); adv(kslice.prev_comms, (size_t)kslice.n_prev * 64);
            adv(kslice.w_comm, 15 * 64); adv(kslice.z_comm, 64); adv(kslice.t_comm, 7 * 64); adv(kslice.evals, 43 * 64); adv(kslice.ft_eval1, 32);
            if (kslice.statements) {
                const void **slots[12]; size_t strides[12];
                mb_pickles_sections(kslice.statements, slots, strides, &sslice);
                kslice.statements = &sslice;
                for (int i = 0; i < 12; ++i) adv(*slots[i], strides[i]);
            }
        }
        adv(s.public_inputs, (size_t)s.npub * 32);
        adv(s.sponge_state, 96); adv(s.sponge_pos, 8); adv(s.cip, 32); adv(s.lr, 2 * k * 64); adv(s.delta, 64); adv(s.sg, 64); adv(s.z1, 32); adv(s.z2, 32);
        adv(s.evalpoints, np * 32); adv(s.evalscale, 32); adv(s.polyscale, 32); adv(s.comms, m * 64);
        adv(s.acc_prechallenges, (size_t)s.acc_k * 16); adv(s.acc_sg, 64); adv(s.acc_rho, 32);
        return s;
    }
    // the culprits of one folded leg: a failing range is cut into FAN parts whose jobs run CONCURRENTLY on lanes 0..FAN-1 of the context
    // (inputs stay where lane 0 uploaded them; every lane has its own verdict words); parts that fail are cut again: depth log_FAN(B) rounds
    // of ~one job latency each, where a bisection ran log2(B) jobs one after the other per culprit.  FAN = 4 (mina_verify_tuning.search_fan): with 32 -- the
    // fan-out until the end of round 3 -- a search over 8192 proofs took 370 ms instead of 165, and the 28 streams it created left the process
    // with more streams than the runtime has hardware queues: every later call of the boundary was 30 % slower, for the life of the process
    // (tools/after_search.py; destroying the streams afterwards does not undo it).
    int search(bool ipa_leg, std::vector<uint8_t> &each) {
        const size_t FAN = std::min<size_t>(MB_PIPE_LANES, std::max<size_t>(2, (size_t)mb_tune().search_fan));
        static const bool timing = getenv("MINA_VERIFY_TIMING") != nullptr;
        // streams this search had to create are destroyed when it is done
        struct Restore {
            mina_ctx *c; std::vector<size_t> made;
            ~Restore() { for (size_t i : made) if (c->lanes[i].stream) { (void)hipStreamSynchronize(c->lanes[i].stream); (void)hipStreamDestroy(c->lanes[i].stream); c->lanes[i].stream = nullptr; } c->use_lane0(); }
        } restore{c, {}};
        for (size_t i = 0; i < FAN; ++i)
            if (!c->lanes[i].stream) { HIPC(hipStreamCreateWithFlags(&c->lanes[i].stream, hipStreamNonBlocking)); restore.made.push_back(i); ++c->search_streams_made; }
        std::vector<std::pair<size_t, size_t>> failing{{0, B}};
        while (!failing.empty()) {
            std::vector<std::pair<size_t, size_t>> parts;
            for (auto [lo, cnt] : failing) {
                if (cnt == 1) { each[lo] = 0; continue; }
                const size_t np_ = std::min(FAN, cnt);
                for (size_t q = 0; q < np_; ++q) { const size_t a = lo + cnt * q / np_, e = lo + cnt * (q + 1) / np_; parts.push_back({a, e - a}); }
            }
            failing.clear();
            const auto t_round = std::chrono::steady_clock::now();
            for (size_t base = 0; base < parts.size(); base += FAN) {
                const size_t w = std::min(FAN, parts.size() - base);
                uint32_t *flags_at[MB_PIPE_LANES];
                for (size_t q = 0; q < w; ++q) {                      // issue: nothing here waits for the GPU
                    const auto [lo, cnt] = parts[base + q];
                    c->L = &c->lanes[q];
                    int r = c->L->st_verdicts.ensure(2 * cnt * 4 + 16);
                    if (r) return r;
                    uint32_t *v = c->L->st_verdicts.as<uint32_t>();
                    flags_at[q] = v + cnt;
                    if (ipa_leg && rows_ok) { if ((r = mb_ipa_recheck_rows(c, lo, cnt, flags_at[q]))) return r; continue; }
                    mina_state_jobs sj = slice(d, lo, cnt);
                    if (ipa_leg) sj.with_accumulator = 0; else { sj.with_ipa = 0; sj.npub = 0; sj.kimchi = nullptr; }
                    StateJobPlan sp; sp.count_mixed = false;
                    if (d_net && ipa_leg) sp.d_net = d_net + lo;
                    if ((r = mb_state_jobs_on_lane(c, &sj, v, flags_at[q], sp))) return r;
                }
                for (size_t q = 0; q < w; ++q) {
                    uint32_t f[4];
                    HIPC(hipStreamSynchronize(c->lanes[q].stream));
                    HIPC(hipMemcpy(f, flags_at[q], 16, hipMemcpyDeviceToHost));
                    if (!(ipa_leg ? f[0] != 0 : f[2] != 0)) failing.push_back(parts[base + q]);
                }
            }
            if (timing) fprintf(stderr, "mina_state_job_batch: culprit search (%s), %zu parts -> %zu failing, %.2f ms\n", ipa_leg ? "opening" : "accumulator", parts.size(), failing.size(),
                                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_round).count());
        }
        return MINA_OK;
    }
    // The grouped search (mina_ctx_set_search_groups; off by default): a failing range is cut into min(G, cnt) parts by the same formula, and ALL parts of a round --
    // of every failing range -- are checked in one pass on lane L: one segmented fold, the fixed-base MSM with one problem per part, one segmented variable-base
    // MSM, one comparison launch, one wait and one read-back of the parts' flags.  Depth ceil(log_G B) rounds; no lane but L is used and no stream is created.  A
    // round goes out in several passes only beyond mb_search_parts_cap parts (or where the segmented MSM's limits ask for fewer), queued back to back.  The opening
    // leg needs the rows of the failed batch (rows_ok), else it keeps the fan search; the counters depend on (B, G, culprits) alone.
    int grouped(bool ipa_leg, std::vector<uint8_t> &each) {
        c->L = &L;
        const size_t G = c->search_groups;
        const int curve = ipa_leg ? CURVE_PALLAS : CURVE_VESTA;
        const size_t cap = mb_search_parts_cap(c, curve, ipa_leg ? d.k : d.acc_k);
        const uint32_t per = ipa_leg ? c->ipa_rows_per : 1;
        int r;
        if (!ipa_leg && (r = mb_accumulator_parts_prepare(c, CURVE_VESTA, d.acc_k, B, (const uint32_t *)d.acc_prechallenges, (const uint32_t *)d.acc_sg))) return r;
        ++c->gs_searches;
        std::vector<std::pair<size_t, size_t>> failing{{0, B}};
        while (!failing.empty()) {
            std::vector<uint32_t> lo, cnt;
            for (auto [l, n] : failing) {
                if (n == 1) { each[l] = 0; continue; }
                const size_t g = std::min(G, n);
                for (size_t q = 0; q < g; ++q) { const size_t a = l + n * q / g, e = l + n * (q + 1) / g; lo.push_back((uint32_t)a); cnt.push_back((uint32_t)(e - a)); }
            }
            failing.clear();
            const size_t nparts = lo.size();
            if (nparts == 0) break;
            ++c->gs_rounds; c->gs_parts += nparts;
            if ((r = L.gs_flags.ensure(nparts * 4)) || (r = L.host_stage.ensure(nparts * MB_PARTS_STAGE))) return r;
            uint32_t *fl = L.gs_flags.as<uint32_t>();
            for (size_t base = 0; base < nparts;) {
                size_t w = std::min(cap, nparts - base);
                auto longest = [&](size_t w_) { uint32_t x = 0; for (size_t q = 0; q < w_; ++q) x = std::max(x, cnt[base + q]); return x; };
                while (w > 1 && !mb_msm_segments_fit(longest(w) * per, w)) w = (w + 1) / 2;
                r = ipa_leg ? mb_ipa_recheck_rows_parts(c, w, &lo[base], &cnt[base], fl + base, base * MB_PARTS_STAGE)
                            : mb_accumulator_check_parts(c, CURVE_VESTA, d.acc_k, B, (const uint32_t *)d.acc_rho, w, &lo[base], &cnt[base], fl + base, base * MB_PARTS_STAGE);
                if (r) return r;
                base += w;
            }
            std::vector<uint32_t> f(nparts);
            if ((r = d2h_sync(c, f.data(), L.gs_flags, nparts * 4))) return r;
            for (size_t p = 0; p < nparts; ++p) if (!f[p]) failing.push_back({lo[p], cnt[p]});
        }
        return MINA_OK;
    }
    // the failed legs, each by the search the context's settings and the leg's inputs allow: each[b] = 0 for its culprits
    int run(bool ipa_ok, bool acc_ok, std::vector<uint8_t> &ipa_each, std::vector<uint8_t> &acc_each) {
        int rc;
        const bool in_groups = c->search_groups >= 2 && !mb_tune().search_full;
        if (!ipa_ok) { rc = (in_groups && rows_ok) ? grouped(true, ipa_each) : search(true, ipa_each); c->L = &L; if (rc) return rc; }
        if (!acc_ok) { rc = (in_groups && B > 1 && d.acc_rho) ? grouped(false, acc_each) : search(false, acc_each); c->L = &L; if (rc) return rc; }
        return MINA_OK;
    }
};
}  // namespace

// The body mina_state_job_batch (after its upload) and mina_state_job_each_dev share: the job on lane L from inputs in HBM (every pointer of `d` a device pointer),
// one verdict byte per proof on the host.  When a folded check fails: a run without the folded legs for the per-proof chain verdicts, then the search for the
// culprits of each failed leg -- in groups on lane L alone (mina_ctx_set_search_groups) or over the fan's lanes.  Waits for lane L.  flags: the four words of the
// whole job's folded checks ([0] opening verdict, [1] malformed opening input, [2] accumulator verdict), or null.
// d_net (StateJobPlan): a mixed job.
static int state_job_each(mina_ctx *c, Lane &L, const mina_state_jobs &d, uint8_t *verdicts, uint32_t *flags, const uint8_t *d_net = nullptr, bool count_mixed = true) {
    c->L = &L;
    const size_t B = d.batch;
    int rc;
    if ((rc = L.st_verdicts.ensure(2 * B * 4 + 16))) return rc;
    uint32_t *dv = L.st_verdicts.as<uint32_t>(), *df = dv + B, *ds = df + 4;
    // small, latency-bound batches: the three independent legs go to three lanes (lane 0 plus two helpers), joined by events
    StateJobPlan plan; plan.d_stmt_out = ds; plan.d_net = d_net; plan.count_mixed = count_mixed;
    if (B <= 1024 && c->nlanes == 1 && &L == &c->lanes[0]) { plan.wrap = &c->lanes[1]; plan.acc = &c->lanes[2]; }
    if ((rc = mb_state_jobs_on_lane(c, &d, dv, df, plan))) return rc;
    std::vector<uint32_t> hv(2 * B + 4);
    if ((rc = d2h_sync(c, hv.data(), L.st_verdicts, (2 * B + 4) * 4))) return rc;
    if (flags) memcpy(flags, &hv[B], 16);
    std::vector<uint8_t> stmt_each(B); for (size_t b = 0; b < B; ++b) stmt_each[b] = hv[B + 4 + b] ? 1 : 0;
    const bool ipa_ok = hv[B] != 0, acc_ok = hv[B + 2] != 0;
    if (ipa_ok && acc_ok) { for (size_t b = 0; b < B; ++b) verdicts[b] = hv[b] ? 1 : 0; return MINA_OK; }
    // a folded check failed somewhere: find the culprits.  chain_ok per proof comes from a run without the folded legs.
    std::vector<uint8_t> ipa_each(B, 1), acc_each(B, 1), chain_each(B, 1);
    {
        mina_state_jobs only = d; only.with_ipa = 0; only.with_accumulator = 0; only.npub = 0; only.kimchi = nullptr;
        if (only.with_states) {
            if ((rc = mb_state_jobs_on_lane(c, &only, dv, df))) return rc;
            if ((rc = d2h_sync(c, hv.data(), L.st_verdicts, B * 4))) return rc;
            for (size_t b = 0; b < B; ++b) chain_each[b] = hv[b] ? 1 : 0;
        }
    }
    CulpritSearch cs(c, L, d, hv[B + 1] != 0);
    cs.d_net = d_net;
    if ((rc = cs.run(ipa_ok, acc_ok, ipa_each, acc_each))) return rc;
    for (size_t b = 0; b < B; ++b) verdicts[b] = (chain_each[b] && ipa_each[b] && acc_each[b] && stmt_each[b]) ? 1 : 0;
    return MINA_OK;
}

// The masks form of that body: `passed` / `ran` words of every proof (state_masks.h) from ONE pass of the job on lane L.  The job runs once with every requested
// leg; the chain-detail kernel then reads the hashes the state leg left on L (st_hashes) and keeps the chain word apart from the folded verdicts, so that a
// folded failure needs the culprit searches only -- no state is hashed a second time.  d.precheck is not read (the host checks have their own bits: d_front).
// Both folded checks good: the only host read is the four flag words.  Otherwise the culprit vectors of the failed legs are uploaded for the masks kernel.
// d_front / d_deny: batch u32 in HBM, or null.  d_passed / d_ran: batch u32 in HBM.  Waits for lane L.  Adds (1, B) to the checks counters.
static int state_job_checks(mina_ctx *c, Lane &L, const mina_state_jobs &jobs, const uint32_t *d_front, const uint32_t *d_deny, uint32_t *d_passed, uint32_t *d_ran, uint32_t *flags) {
    c->L = &L;
    mina_state_jobs d = jobs; d.precheck = nullptr;
    const size_t B = d.batch;
    int rc;
    if ((rc = L.st_verdicts.ensure(2 * B * 4 + 16)) || (rc = L.st_masks.ensure(8 * B * 4))) return rc;
    uint32_t *dv = L.st_verdicts.as<uint32_t>(), *df = dv + B;
    uint32_t *chain = L.st_masks.as<uint32_t>(), *stmt = chain + B, *d_ipa_each = stmt + B, *d_acc_each = d_ipa_each + B;      // (the searches reuse st_verdicts: the statement words live here)
    StateJobPlan plan; plan.d_stmt_out = stmt;
    if (B <= 1024 && c->nlanes == 1 && &L == &c->lanes[0]) { plan.wrap = &c->lanes[1]; plan.acc = &c->lanes[2]; }
    if ((rc = mb_state_jobs_on_lane(c, &d, dv, df, plan))) return rc;
    ++c->checks_jobs; c->checks_proofs += B;
    // the state leg ran on L's own stream (the plan above names no lane for it): its hashes are in L.st_hashes, ahead of this launch in stream order
    if (d.with_states) mb::pstate_chain_detail_kernel<<<cdiv(B, 64), 64, 0, L.stream>>>((uint32_t)B, L.st_hashes.as<uint32_t>(), (const uint32_t *)d.expected_hashes, (const uint32_t *)d.state_records, chain);
    uint32_t hf[4];
    HIPC(hipMemcpyAsync(hf, df, 16, hipMemcpyDeviceToHost, L.stream));
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(L.stream));
    if (flags) memcpy(flags, hf, 16);
    const bool ipa_ok = hf[0] != 0, acc_ok = hf[2] != 0;
    std::vector<uint32_t> each;
    if (!(ipa_ok && acc_ok)) {
        std::vector<uint8_t> ipa_each(B, 1), acc_each(B, 1);
        CulpritSearch cs(c, L, d, hf[1] != 0);
        if ((rc = cs.run(ipa_ok, acc_ok, ipa_each, acc_each))) return rc;
        each.resize(2 * B);
        for (size_t b = 0; b < B; ++b) { each[b] = ipa_each[b]; each[B + b] = acc_each[b]; }
        HIPC(hipMemcpyAsync(d_ipa_each, each.data(), 2 * B * 4, hipMemcpyHostToDevice, L.stream));
    }
    const uint32_t sections = (d.with_states ? 1u : 0u) | (d.with_accumulator ? 2u : 0u) | (d.with_ipa ? 4u : 0u);
    mb::state_job_masks_kernel<<<cdiv(B, 64), 64, 0, L.stream>>>((uint32_t)B, sections, d_front, d_deny, d.with_states ? chain : nullptr, stmt, each.empty() ? nullptr : d_ipa_each,
                                                                 each.empty() ? nullptr : d_acc_each, d_passed, d_ran);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(L.stream));
    return MINA_OK;
}

// The upload of mina_state_job_batch and mina_state_job_checks: every section of `jobs` (host pointers) in one copy through lane L's pinned staging into L.st_in;
// d (with kd, sd behind its pointers) = the same job over the device copies.  more: further host sections that travel behind the job's (their slots rewritten likewise).
static int upload_jobs(mina_ctx *c, Lane &L, const mina_state_jobs *jobs, mina_state_jobs &d, mina_kimchi_proofs &kd, mina_pickles_statements &sd, const std::vector<Section> &more = {}) {
    int rc;
    d = *jobs;
    const size_t B = jobs->batch, k = jobs->k, m = jobs->n_comms, np = jobs->n_evalpoints, S = MINA_STATES_PER_PROOF;
    std::vector<Section> secs;
    auto add = [&](const void *&slot, size_t bytes) { if (slot && bytes) secs.push_back({&slot, bytes}); };
    if (d.with_states) { add(d.state_records, B * S * MINA_PSTATE_SLOTS * 32); add(d.state_nfields, B * S * 4); add(d.expected_hashes, B * S * 32); add(d.precheck, B); }
    if (d.npub) add(d.public_inputs, B * d.npub * 32);
    kd = mina_kimchi_proofs{}; sd = mina_pickles_statements{};
    if (d.with_ipa && d.kimchi) {
        kd = *d.kimchi; d.kimchi = &kd;
        kd.public_inputs = nullptr;                                   // the job's own public_inputs section is the one uploaded
        add(kd.prev_chals, B * kd.n_prev * k * 32); add(kd.prev_prechallenges, B * kd.n_prev * k * 16); add(kd.prev_comms, B * kd.n_prev * 64); add(kd.w_comm, B * 15 * 64); add(kd.z_comm, B * 64);
        add(kd.t_comm, B * 7 * 64); add(kd.evals, B * 43 * 64); add(kd.ft_eval1, B * 32);
        if (kd.statements) {
            const void **slots[12]; size_t strides[12];
            mb_pickles_sections(kd.statements, slots, strides, &sd);
            kd.statements = &sd;
            for (int i = 0; i < 12; ++i) add(*slots[i], B * strides[i]);
        }
        d.sponge_state = d.sponge_pos = d.cip = d.evalpoints = d.evalscale = d.polyscale = d.comms = nullptr;
    }
    if (d.with_ipa) {
        add(d.sponge_state, B * 96); add(d.sponge_pos, B * 8); add(d.cip, B * 32); add(d.lr, B * 2 * k * 64); add(d.delta, B * 64); add(d.sg, B * 64);
        add(d.z1, B * 32); add(d.z2, B * 32); add(d.evalpoints, B * np * 32); add(d.evalscale, B * 32); add(d.polyscale, B * 32); add(d.comms, B * m * 64);
        add(d.rand_base, 32); add(d.sg_rand_base, 32);
    }
    if (d.with_accumulator) { add(d.acc_prechallenges, B * d.acc_k * 16); add(d.acc_sg, B * 64); add(d.acc_rho, B * 32); }
    for (const Section &s : more) if (*s.slot && s.bytes) secs.push_back(s);
    size_t total = 0;
    std::vector<size_t> offs;
    for (auto &s : secs) { offs.push_back(total); total += (s.bytes + 255) & ~(size_t)255; }
    if ((rc = L.host_stage.ensure(total + B * 4))) return rc;
    uint8_t *blob = (uint8_t *)L.host_stage.p;
    for (size_t i = 0; i < secs.size(); ++i) memcpy(blob + offs[i], *secs[i].slot, secs[i].bytes);
    if ((rc = L.st_in.ensure(total))) return rc;
    HIPC(hipMemcpyAsync(L.st_in.p, blob, total, hipMemcpyHostToDevice, L.stream));
    for (size_t i = 0; i < secs.size(); ++i) *secs[i].slot = L.st_in.as<uint8_t>() + offs[i];
    if (d.kimchi) kd.public_inputs = d.public_inputs;
    return MINA_OK;
}

// host-buffer form: one upload of every section, the pipeline, one download; when a folded check fails the proofs are
// re-checked in parts (32-way cuts, the parts of a round concurrently) so that every proof gets its own verdict (README.md:281-310: every failure is `false`)
extern "C" int mina_state_job_batch(mina_ctx *c, const mina_state_jobs *jobs, uint8_t *verdicts) {
    int rc = mb_check_jobs(c, jobs);
    if (rc) return rc;
    if (!verdicts) return fail(MINA_ERR_ARG, "null argument");
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    if ((rc = mina_state_jobs_prepare(c, jobs->log2_domain, jobs->npub))) return rc;
    c->use_lane0();
    Lane &L = *c->L;
    mina_state_jobs d; mina_kimchi_proofs kd; mina_pickles_statements sd;
    if ((rc = upload_jobs(c, L, jobs, d, kd, sd))) return rc;
    return state_job_each(c, L, d, verdicts, nullptr);
}

// The masks of a job whose inputs are host buffers: mina_state_job_batch's upload (front / deny behind the job's sections), state_job_checks, one download.
extern "C" int mina_state_job_checks(mina_ctx *c, const mina_state_jobs *jobs, const uint32_t *front, const uint32_t *deny, uint32_t *passed, uint32_t *ran) {
    int rc = mb_check_jobs(c, jobs);
    if (rc) return rc;
    if (!passed || !ran) return fail(MINA_ERR_ARG, "null argument");
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    if ((rc = mina_state_jobs_prepare(c, jobs->log2_domain, jobs->npub))) return rc;
    c->use_lane0();
    Lane &L = *c->L;
    const size_t B = jobs->batch;
    const void *fr = front, *dn = deny;
    mina_state_jobs d; mina_kimchi_proofs kd; mina_pickles_statements sd;
    if ((rc = upload_jobs(c, L, jobs, d, kd, sd, {{&fr, B * 4}, {&dn, B * 4}}))) return rc;
    if ((rc = L.st_masks.ensure(8 * B * 4))) return rc;
    uint32_t *out = L.st_masks.as<uint32_t>() + 6 * B;
    if ((rc = state_job_checks(c, L, d, (const uint32_t *)fr, (const uint32_t *)dn, out, out + B, nullptr))) return rc;
    std::vector<uint32_t> hv(2 * B);
    HIPC(hipMemcpy(hv.data(), out, 2 * B * 4, hipMemcpyDeviceToHost));
    memcpy(passed, hv.data(), B * 4); memcpy(ran, &hv[B], B * 4);
    return MINA_OK;
}

// the masks body on lane 0 with the words on the host: what the boundary's mina_verify_state_checks_batch runs over a chunk's device staging (mina_ctx::state_job_checks)
int mb_state_job_checks_host(mina_ctx *c, const mina_state_jobs *jobs, const uint32_t *d_front, const uint32_t *front, const uint32_t *deny, uint32_t *passed, uint32_t *ran) {
    int rc = mb_check_jobs(c, jobs);
    if (rc) return rc;
    if (!passed || !ran || (d_front && front)) return fail(MINA_ERR_ARG, "null argument / two front vectors");
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    if ((rc = mina_state_jobs_prepare(c, jobs->log2_domain, jobs->npub))) return rc;
    c->use_lane0();
    Lane &L = *c->L;
    const size_t B = jobs->batch;
    if ((rc = L.st_masks.ensure(8 * B * 4))) return rc;
    uint32_t *w = L.st_masks.as<uint32_t>(), *d_fr = w + 4 * B, *d_dn = w + 5 * B, *out = w + 6 * B;
    if (front) HIPC(hipMemcpyAsync(d_fr, front, B * 4, hipMemcpyHostToDevice, L.stream));
    if (deny) HIPC(hipMemcpyAsync(d_dn, deny, B * 4, hipMemcpyHostToDevice, L.stream));
    if ((rc = state_job_checks(c, L, *jobs, front ? d_fr : d_front, deny ? d_dn : nullptr, out, out + B, nullptr))) return rc;
    std::vector<uint32_t> hv(2 * B);
    HIPC(hipMemcpy(hv.data(), out, 2 * B * 4, hipMemcpyDeviceToHost));
    memcpy(passed, hv.data(), B * 4); memcpy(ran, &hv[B], B * 4);
    return MINA_OK;
}

extern "C" int mina_state_job_checks_dev(mina_ctx *c, const mina_state_jobs *jobs, const void *d_front, const void *d_deny, void *d_passed, void *d_ran, void *d_flags) {
    int rc = mb_check_jobs(c, jobs);
    if (rc) return rc;
    if (!d_passed || !d_ran) return fail(MINA_ERR_ARG, "null argument");
    if (((uintptr_t)d_front | (uintptr_t)d_deny | (uintptr_t)d_passed | (uintptr_t)d_ran | (uintptr_t)d_flags) & 3u) return fail(MINA_ERR_ARG, "masks and flags are 32-bit words: 4-byte alignment");
    if (!c->have_state_salts && jobs->with_states) return fail(MINA_ERR_STATE, "call mina_state_jobs_prepare first");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    Lane &L = *c->L;
    uint32_t hf[4];
    rc = state_job_checks(c, L, *jobs, (const uint32_t *)d_front, (const uint32_t *)d_deny, (uint32_t *)d_passed, (uint32_t *)d_ran, hf);
    c->L = &L;
    if (rc) return rc;
    if (d_flags) { HIPC(hipMemcpyAsync(d_flags, hf, 16, hipMemcpyHostToDevice, L.stream)); HIPC(hipStreamSynchronize(L.stream)); }
    return MINA_OK;
}

extern "C" int mina_ctx_checks_stats(mina_ctx *c, uint64_t *jobs, uint64_t *proofs) {
    if (!c || !jobs || !proofs) return fail(MINA_ERR_ARG, "null argument");
    *jobs = c->checks_jobs; *proofs = c->checks_proofs;
    return MINA_OK;
}

// the shared body on lane 0 with the verdict bytes on the host: what the boundary's fallback runs over a failed chunk's device staging (mina_ctx::state_job_each)
int mb_state_job_each_host(mina_ctx *c, const mina_state_jobs *jobs, uint8_t *verdicts) {
    int rc = mb_check_jobs(c, jobs);
    if (rc) return rc;
    if (!verdicts) return fail(MINA_ERR_ARG, "null argument");
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    if ((rc = mina_state_jobs_prepare(c, jobs->log2_domain, jobs->npub))) return rc;
    c->use_lane0();
    return state_job_each(c, *c->L, *jobs, verdicts, nullptr);
}

// the same for a mixed job (ctx.h StateJobPlan::d_net): what the boundary's fallback runs over a failed mixed chunk (mina_ctx::state_job_each_net).  The chunk's own
// job counted it and its proofs (mina_ctx_mixed_job_stats): this pass counts nothing.
int mb_state_job_each_net_host(mina_ctx *c, const mina_state_jobs *jobs, const uint8_t *d_net, uint8_t *verdicts) {
    int rc = mb_check_jobs(c, jobs);
    if (rc) return rc;
    if (!verdicts || !d_net) return fail(MINA_ERR_ARG, "null argument");
    if ((rc = mb_mixed_sets_check(c))) return rc;
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    if ((rc = mina_state_jobs_prepare(c, jobs->log2_domain, jobs->npub))) return rc;
    c->use_lane0();
    return state_job_each(c, *c->L, *jobs, verdicts, nullptr, d_net, false);
}

static int state_job_each_dev(mina_ctx *c, const mina_state_jobs *jobs, const void *d_net, bool mixed, void *d_verdicts, void *d_flags) {
    int rc = mb_check_jobs(c, jobs);
    if (rc) return rc;
    if (!d_verdicts || (mixed && !d_net)) return fail(MINA_ERR_ARG, "null argument");
    if (mixed && (rc = mb_mixed_sets_check(c))) return rc;
    if (((uintptr_t)d_verdicts | (uintptr_t)d_flags) & 3u) return fail(MINA_ERR_ARG, "verdicts and flags are 32-bit words: 4-byte alignment");
    if (!c->have_state_salts && jobs->with_states) return fail(MINA_ERR_STATE, "call mina_state_jobs_prepare first");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    Lane &L = *c->L;
    const size_t B = jobs->batch;
    std::vector<uint8_t> each(B);
    std::vector<uint32_t> words(B + 4);
    if ((rc = state_job_each(c, L, *jobs, each.data(), &words[B], mixed ? (const uint8_t *)d_net : nullptr))) { c->L = &L; return rc; }
    c->L = &L;
    for (size_t b = 0; b < B; ++b) words[b] = each[b];
    HIPC(hipMemcpyAsync(d_verdicts, words.data(), B * 4, hipMemcpyHostToDevice, L.stream));
    if (d_flags) HIPC(hipMemcpyAsync(d_flags, &words[B], 16, hipMemcpyHostToDevice, L.stream));
    HIPC(hipStreamSynchronize(L.stream));
    return MINA_OK;
}
extern "C" int mina_state_job_each_dev(mina_ctx *c, const mina_state_jobs *jobs, void *d_verdicts, void *d_flags) { return state_job_each_dev(c, jobs, nullptr, false, d_verdicts, d_flags); }
extern "C" int mina_state_job_each_net_dev(mina_ctx *c, const mina_state_jobs *jobs, const void *d_net, void *d_verdicts, void *d_flags) {
    return state_job_each_dev(c, jobs, d_net, true, d_verdicts, d_flags);
}

extern "C" int mina_ctx_set_search_groups(mina_ctx *c, uint32_t groups) {
    if (!c) return fail(MINA_ERR_ARG, "null argument");
    if (groups == 1 || groups > 128) return fail(MINA_ERR_ARG, "search groups: 0 (off) or 2 .. 128");
    c->search_groups = groups;
    return MINA_OK;
}

// test-facing: the streams the context's lanes hold now (main and side streams of every lane, helpers included) and the streams its culprit searches have created
// so far (the fan search creates the ones its lanes lack and destroys them when it is done; the grouped search creates none)
extern "C" int mina_ctx_lane_streams(mina_ctx *c, uint32_t *live, uint64_t *made_by_searches) {
    if (!c || !live || !made_by_searches) return fail(MINA_ERR_ARG, "null argument");
    uint32_t n = 0;
    for (int i = 0; i < MB_MAX_LANES; ++i) n += ((c->lanes[i].stream && i < MB_DEV_HELPER0) ? 1u : 0u) + (c->lanes[i].aux ? 1u : 0u);      // (the forked jobs' helper lanes alias the streams below)
    for (hipStream_t s : c->fork_own) n += s ? 1u : 0u;
    for (hipStream_t s : c->role) n += s ? 1u : 0u;
    *live = n; *made_by_searches = c->search_streams_made;
    return MINA_OK;
}

extern "C" int mina_ctx_search_stats(mina_ctx *c, uint64_t *searches, uint64_t *rounds, uint64_t *parts) {
    if (!c || !searches || !rounds || !parts) return fail(MINA_ERR_ARG, "null argument");
    *searches = c->gs_searches; *rounds = c->gs_rounds; *parts = c->gs_parts;
    return MINA_OK;
}
