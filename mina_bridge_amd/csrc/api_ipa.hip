// api_ipa.hip -- the combined IPA checks on top of K1..K4.
//
// Replaces poly-commitment `SRS::verify` (batched opening check) and openmina `accumulator_check`
// (pins core/Cargo.toml:16,23; README.md:469-475, 534-544).  Per proof b (rho = rand_base^b,
// sigma = sg_rand_base^b) upstream pushes onto ONE multi-scalar multiplication
//     g[j] += sigma * s_b[j]          h -= rho z2          sg: -rho z1 - sigma        U: -rho z1 b0 + rho c cip
//     L_j: rho c / chal_j             R_j: rho c chal_j    comm_i: rho c xi^i         delta: rho
// and asserts the result is the identity.  Here the g-part is K2 (fold) + K1 (fixed-base tables) and the
// per-proof points go through the variable-base K1 path; the two partial results are compared on the GPU.
// The Fiat-Shamir transcript of each proof runs as one lane of `ipa_prepare_kernel` (throughput layout:
// one proof per lane; a wave-cooperative sponge is the planned latency optimisation).
#include "ctx.h"
#include "msm.cuh"
#include "sponge.cuh"

namespace mb {

// ---------------------------------------------------------------- generic Fq-sponge transcript ("tape")
// mina-poseidon `DefaultFqSponge` over the base field of CURVE (pins core/Cargo.toml:14; README.md:413-475 lists the order
// kimchi absorbs/squeezes in).  Every proof of a batch runs the same tape of opcodes over its own input stream:
enum : uint8_t {
    TAPE_ABSORB_FQ = 0,        // one base-field element                                   (32 B in)
    TAPE_ABSORB_G = 1,         // one affine point: x then y; infinity absorbs (0, 0)      (64 B in)
    TAPE_ABSORB_FR = 2,        // one scalar-field element: whole if r < q, else (x >> 1, x & 1)   (32 B in)
    TAPE_CHALLENGE = 3,        // squeeze, low 128 bits                                    (32 B out, upper 16 zero)
    TAPE_CHALLENGE_FQ = 4,     // squeeze, full base-field element                         (32 B out)
    TAPE_CHALLENGE_ENDO = 5,   // squeeze 128 bits -> ScalarChallenge::to_field (scalar field)      (32 B out)
    TAPE_DIGEST = 6,           // squeeze; as a scalar-field element if it fits, else 0    (32 B out)
    TAPE_CHALLENGE_ENDO_OWN = 7, // squeeze 128 bits -> to_field in the sponge's OWN field (kimchi `DefaultFrSponge::challenge`:
                               // run the tape on the curve whose BASE field is the proof's scalar field)      (32 B out)
};
template <int CURVE, int LANES>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LANES == 3 ? 4 : 1, 8)))   // 3-lane form: the four waves per SIMD it had before the signed-digit forms (+ 6 VGPRs)
sponge_tape_kernel(uint32_t batch, uint32_t tape_len, uint32_t in_stride_words, uint32_t out_stride_words, FieldK kb, FieldK ks,
                   const PoseidonParams *__restrict__ pp, const uint8_t *__restrict__ tape, const uint32_t *__restrict__ init_state /* b*24 or null */,
                   const uint32_t *__restrict__ init_pos /* b*2 or null */, const uint32_t *__restrict__ inputs, uint32_t *__restrict__ outputs,
                   uint32_t *__restrict__ final_state /* b*24 or null */, uint32_t *__restrict__ final_pos /* b*2 or null */) {
    constexpr int FB = (CURVE == CURVE_PALLAS) ? FIELD_FP : FIELD_FQ;
    constexpr int FS = (CURVE == CURVE_PALLAS) ? FIELD_FQ : FIELD_FP;
    bool writer_; const uint32_t b = coop_sponge_index<LANES>(writer_), qq = coop_elem<LANES>();
    if (b >= batch) return;                                   // whole lane groups leave together
    DevSponge<FB, LANES, false> sp; sp.pp = pp; sp.squeezed = 0; sp.count = 0; sp.s = fe_zero();   // the plain rounds: with the second round form beside them the 3-lane tape spills past its scratch budget (test-facing: not on a job's path)
    if (init_state) { sp.s = fe_to_mont<FB>(load_fe<FB>(init_state + (size_t)b * 24 + qq * 8), kb.r2); sp.squeezed = (int)init_pos[2 * b]; sp.count = (int)init_pos[2 * b + 1]; }
    const uint32_t *in = inputs + (size_t)b * in_stride_words;
    uint32_t *out = outputs + (size_t)b * out_stride_words;
    for (uint32_t t = 0; t < tape_len; ++t) {
        const uint8_t op = tape[t];
        if (op == TAPE_ABSORB_FQ) { sp.absorb(fe_to_mont<FB>(load_fe<FB>(in), kb.r2)); in += 8; }
        else if (op == TAPE_ABSORB_G) { sp.absorb(fe_to_mont<FB>(load_fe<FB>(in), kb.r2)); sp.absorb(fe_to_mont<FB>(load_fe<FB>(in + 8), kb.r2)); in += 16; }
        else if (op == TAPE_ABSORB_FR) {
            fe_t x = load_fe<FS>(in); in += 8;
            if (CURVE == CURVE_PALLAS) {                       // scalar modulus (q) > base modulus (p): split off the low bit
                fe_t lowbit = fe_zero(); lowbit.v[0] = x.v[0] & 1u;
                fe_t hi = x; for (int i = 0; i < 7; ++i) hi.v[i] = (hi.v[i] >> 1) | (hi.v[i + 1] << 31); hi.v[7] >>= 1;
                sp.absorb(fe_to_mont<FB>(hi, kb.r2)); sp.absorb(fe_to_mont<FB>(lowbit, kb.r2));
            } else sp.absorb(fe_to_mont<FB>(x, kb.r2));
        } else {
            fe_t sq = fe_from_mont<FB>(sp.squeeze()), o = fe_zero();
            if (op == TAPE_CHALLENGE) { o.v[0] = sq.v[0]; o.v[1] = sq.v[1]; o.v[2] = sq.v[2]; o.v[3] = sq.v[3]; }
            else if (op == TAPE_CHALLENGE_FQ) o = sq;
            else if (op == TAPE_CHALLENGE_ENDO) {
                uint64_t lo = (uint64_t)sq.v[0] | ((uint64_t)sq.v[1] << 32), hi = (uint64_t)sq.v[2] | ((uint64_t)sq.v[3] << 32);
                o = fe_from_mont<FS>(challenge_to_field<FS>(lo, hi, ks));
            } else if (op == TAPE_CHALLENGE_ENDO_OWN) {
                uint64_t lo = (uint64_t)sq.v[0] | ((uint64_t)sq.v[1] << 32), hi = (uint64_t)sq.v[2] | ((uint64_t)sq.v[3] << 32);
                o = fe_from_mont<FB>(challenge_to_field<FB>(lo, hi, kb));
            } else {                                          // TAPE_DIGEST: fits the scalar field?  (compare with its modulus)
                bool fits = false;
                for (int i = 7; i >= 0; --i) { uint32_t m = modulus_limb<FS>(i); if (sq.v[i] != m) { fits = sq.v[i] < m; break; } }
                if (fits) o = sq;
            }
            store_fe<LANES>(out, o); out += 8;
        }
    }
    if (final_state && coop_state_owner<LANES>()) { fe_t w = fe_from_mont<FB>(sp.s); for (int i = 0; i < 8; ++i) final_state[(size_t)b * 24 + qq * 8 + i] = w.v[i]; }
    if (final_pos && writer_) { final_pos[2 * b] = (uint32_t)sp.squeezed; final_pos[2 * b + 1] = (uint32_t)sp.count; }
}


// One lane group (8 lanes, or a wave-packed triple above 1024 proofs per call) per proof: the Fq-sponge runs lane-cooperatively (6.3 / 4.65 dependent product latencies per
// Poseidon round instead of 21), all other (scalar-field) work is computed redundantly by the lanes, lane 0 writes.
// CURVE fixes (FB, FS).
// PHASE 0: the whole transcript.  PHASE 1 / 2: split at the first squeeze -- `U = to_group(t)` (an inversion and 1-3 square
// roots, ~0.75 ms of dependent products) is not fed back into the sponge, so it runs as its own kernel on a second stream
// while PHASE 2 continues the transcript; the sponge is handed over through `xfer` (40 words per proof: state in
// Montgomery form, position, t).
static constexpr uint32_t IPA_XFER_WORDS = 40;
template <int CURVE, int LANES, int PHASE>
__global__ void __launch_bounds__(64)
ipa_prepare_kernel(IpaShape sh, FieldK kb, FieldK ks, const PoseidonParams *__restrict__ pp,
                   const uint32_t *__restrict__ sponge_state /* b*24 */, const uint32_t *__restrict__ sponge_pos /* b*2 */,
                   const uint32_t *__restrict__ cip /* b*8 */,
                   const uint32_t *__restrict__ lr /* b*2k*16 */, const uint32_t *__restrict__ delta /* b*16 */,
                   const uint32_t *__restrict__ sg /* b*16 */, const uint32_t *__restrict__ z1, const uint32_t *__restrict__ z2,
                   const uint32_t *__restrict__ evalpoints /* b*npts*8 */, const uint32_t *__restrict__ evalscale,
                   const uint32_t *__restrict__ polyscale, const uint32_t *__restrict__ comms /* b*ncomms*16 */,
                   const uint32_t *__restrict__ comm_override /* b*16 or null */, IpaExpand ex,
                   const uint32_t *__restrict__ rand_base, const uint32_t *__restrict__ sg_rand_base,
                   const affine_t *__restrict__ srs_h,
                   affine_t *__restrict__ out_points /* b*per */, uint32_t *__restrict__ out_scalars /* b*per*8 canonical */,
                   uint32_t *__restrict__ out_chals /* b*k*8 canonical */, uint32_t *__restrict__ out_sigma /* b*8 canonical */,
                   uint32_t *__restrict__ bad_input /* zeroed by the host; set to 1 on a malformed point */,
                   uint32_t *__restrict__ xfer /* PHASE 1 writes, PHASE 2 reads: b * IPA_XFER_WORDS */,
                   uint32_t *__restrict__ shared_sc /* b * nshared * 8 canonical, or null */, uint32_t *__restrict__ shared_off /* nshared list offsets */) { mb_wave_prio();
    constexpr int FB = (CURVE == CURVE_PALLAS) ? FIELD_FP : FIELD_FQ;
    constexpr int FS = (CURVE == CURVE_PALLAS) ? FIELD_FQ : FIELD_FP;
    bool writer_; const uint32_t b = coop_sponge_index<LANES>(writer_);
    if (b >= sh.batch) return;                                // whole lane groups leave together
    const uint32_t k = sh.k;
    bool pts_ok = true;                                       // every input well-formed (canonical field elements, points on the curve)
    uint32_t *xf = xfer ? xfer + (size_t)b * IPA_XFER_WORDS : nullptr;

    // ---- Fq-sponge transcript (base field)
    // PHASE 1 -- one or two permutations -- keeps the plain rounds: it runs beside the state hashes at 96 VGPRs (5 waves per SIMD), and the normalised rounds' last round takes 101
    DevSponge<FB, LANES, PHASE != 1> sp; sp.pp = pp; sp.squeezed = 0; sp.count = 0;
    if (PHASE == 2) {                                         // resume after the first squeeze
        sp.s = load_fe<FB>(xf + coop_elem<LANES>() * 8);
        sp.squeezed = (int)xf[24]; sp.count = (int)xf[25];
    } else {
        const fe_t w = load_fe<FB>(sponge_state + (size_t)b * 24 + coop_elem<LANES>() * 8);
        bool okw = true;                                      // all three state elements, checked redundantly by every lane
        for (int e = 0; e < 3; ++e) okw = okw && fe_words_canonical<FB>(load_fe<FB>(sponge_state + (size_t)b * 24 + e * 8));
        pts_ok = pts_ok && okw;
        sp.s = fe_to_mont<FB>(w, kb.r2);
    }
    if (PHASE != 2) { sp.squeezed = (int)sponge_pos[2 * b]; sp.count = (int)sponge_pos[2 * b + 1]; }
    auto load_scalar_checked = [&](const uint32_t *p) {           // scalar-field element: canonical or the batch is rejected
        const fe_t w = load_fe<FS>(p);
        pts_ok = pts_ok && fe_words_canonical<FS>(w);
        return fe_to_mont<FS>(w, ks.r2);
    };
    const fe_t cip_m = PHASE == 2 ? fe_to_mont<FS>(load_fe<FS>(cip + (size_t)b * 8), ks.r2) : load_scalar_checked(cip + (size_t)b * 8);
    affine_t U; U.x = fe_zero(); U.y = fe_zero();
    if (PHASE != 2) {   // absorb_fr(shift_scalar(cip))
        const fe_t two255 = ks.two255;
        if (CURVE == CURVE_PALLAS) {
            // scalar modulus > base modulus: x = cip - 2^255 ; absorb (x >> 1), then (x & 1)
            fe_t x = fe_from_mont<FS>(fe_sub<FS>(cip_m, two255));
            fe_t lowbit = fe_zero(); lowbit.v[0] = x.v[0] & 1u;
            fe_t hi = x; for (int i = 0; i < 7; ++i) hi.v[i] = (hi.v[i] >> 1) | (hi.v[i + 1] << 31); hi.v[7] >>= 1;
            sp.absorb(fe_to_mont<FB>(hi, kb.r2));
            sp.absorb(fe_to_mont<FB>(lowbit, kb.r2));
        } else {
            // scalar modulus < base modulus: x = (cip - (2^255 + 1)) / 2, absorbed as one base-field element
            fe_t x = fe_from_mont<FS>(fe_mul<FS>(fe_sub<FS>(cip_m, fe_add<FS>(two255, ks.one)), ks.inv2));
            sp.absorb(fe_to_mont<FB>(x, kb.r2));
        }
        const fe_t t = sp.squeeze();                          // challenge_fq
        if (PHASE == 1) {                                     // hand over: state (owner lanes), position, t; flag; done
            if (coop_state_owner<LANES>()) for (int i = 0; i < 8; ++i) xf[coop_elem<LANES>() * 8 + i] = sp.s.v[i];
            if (writer_) { xf[24] = (uint32_t)sp.squeezed; xf[25] = (uint32_t)sp.count; for (int i = 0; i < 8; ++i) xf[26 + i] = t.v[i]; }
            if (!pts_ok && writer_) *bad_input = 1u;
            return;
        }
        U = bw_to_group<FB>(t, kb);
    }

    affine_t *pts = out_points + (size_t)b * sh.per;
    uint32_t *scs = out_scalars + (size_t)b * sh.per * 8;
    // entries whose point is shared by the whole batch: zero scalar in the list, the real one in the side matrix, the point once at the tail
    uint32_t shq = 0;
    auto put = [&](uint32_t o, const affine_t &P, const fe_t &sc_canon, bool shared) {
        store_pt<LANES>(&pts[o], P);
        if (shared && sh.nshared) {
            store_fe<LANES>(scs + (size_t)o * 8, fe_zero());
            store_fe<LANES>(shared_sc + ((size_t)b * sh.nshared + shq) * 8, sc_canon);
            if (b == 0) { store_pt<LANES>(out_points + (size_t)sh.batch * sh.per + shq, P); if (coop_writer<LANES>()) shared_off[shq] = o; }
            ++shq;
        } else store_fe<LANES>(scs + (size_t)o * 8, sc_canon);
    };

    // rho = rand_base^(b + pow_first), sigma = sg_rand_base^(b + pow_first)   (pow_first = 0: upstream's rho_b = rand_base^b)
    fe_t rho = ks.one, sigma = ks.one;
    {
        fe_t rb = fe_to_mont<FS>(load_fe<FS>(rand_base), ks.r2), sb = fe_to_mont<FS>(load_fe<FS>(sg_rand_base), ks.r2);
        for (uint32_t e = b + sh.pow_first; e; e >>= 1) {
            if (e & 1u) { rho = fe_mul<FS>(rho, rb); sigma = fe_mul<FS>(sigma, sb); }
            rb = fe_sqr<FS>(rb); sb = fe_sqr<FS>(sb);
        }
    }

    fe_t chal_m[20];                                          // k <= 20
    // challenges: absorb L_j, R_j ; squeeze 128 bits ; endo-expand.  Points go straight to the output list.
    // layout of the per-proof list: [h, sg, U, delta, L_0, R_0, ..., L_{k-1}, R_{k-1}, comm_0 .. comm_{m-1}]
    for (uint32_t j = 0; j < k; ++j) {
        const uint32_t *lp = lr + ((size_t)b * 2 * k + 2 * j) * 16;
        affine_t L = load_point_checked<FB>(lp, kb, pts_ok), R = load_point_checked<FB>(lp + 16, kb, pts_ok);
        sp.absorb(L.x); sp.absorb(L.y);                     // infinity is (0,0): absorbs two zeros, as upstream
        sp.absorb(R.x); sp.absorb(R.y);
        fe_t sq = fe_from_mont<FB>(sp.squeeze());
        uint64_t lo = (uint64_t)sq.v[0] | ((uint64_t)sq.v[1] << 32), hi = (uint64_t)sq.v[2] | ((uint64_t)sq.v[3] << 32);
        fe_t chal = challenge_to_field<FS>(lo, hi, ks);
        chal_m[j] = chal;                                     // Montgomery copy for the scalar work below
        store_fe<LANES>(out_chals + ((size_t)b * k + j) * 8, fe_from_mont<FS>(chal));
        store_pt<LANES>(&pts[4 + 2 * j], L); store_pt<LANES>(&pts[5 + 2 * j], R);
    }
    const affine_t D = load_point_checked<FB>(delta + (size_t)b * 16, kb, pts_ok);
    sp.absorb(D.x); sp.absorb(D.y);
    fe_t c;
    {
        fe_t sq = fe_from_mont<FB>(sp.squeeze());
        uint64_t lo = (uint64_t)sq.v[0] | ((uint64_t)sq.v[1] << 32), hi = (uint64_t)sq.v[2] | ((uint64_t)sq.v[3] << 32);
        c = challenge_to_field<FS>(lo, hi, ks);
    }

    // b0 = sum_p r^p * b_poly(chal, pt_p)
    const fe_t r = load_scalar_checked(evalscale + (size_t)b * 8);
    fe_t b0 = fe_zero(), scale = ks.one;
    for (uint32_t p = 0; p < sh.npts; ++p) {
        fe_t pw = load_scalar_checked(evalpoints + ((size_t)b * sh.npts + p) * 8), acc = ks.one;
        for (int i = (int)k - 1; i >= 0; --i) {
            acc = fe_mul<FS>(acc, fe_add<FS>(ks.one, fe_mul<FS>(chal_m[i], pw)));
            pw = fe_sqr<FS>(pw);
        }
        b0 = fe_add<FS>(b0, fe_mul<FS>(scale, acc));
        scale = fe_mul<FS>(scale, r);
    }

    const fe_t z1m = load_scalar_checked(z1 + (size_t)b * 8);
    const fe_t z2m = load_scalar_checked(z2 + (size_t)b * 8);
    const fe_t neg_rho = fe_neg<FS>(rho);
    const fe_t rho_c = fe_mul<FS>(rho, c);

    put(0, *srs_h, fe_from_mont<FS>(fe_mul<FS>(neg_rho, z2m)), sh.shared_h != 0);
    store_pt<LANES>(&pts[1], load_point_checked<FB>(sg + (size_t)b * 16, kb, pts_ok));
    store_fe<LANES>(scs + 1 * 8, fe_from_mont<FS>(fe_sub<FS>(fe_mul<FS>(neg_rho, z1m), sigma)));
    if (PHASE == 0) store_pt<LANES>(&pts[2], U);                // PHASE 2: written by ipa_to_group_kernel
    store_fe<LANES>(scs + 2 * 8, fe_from_mont<FS>(fe_add<FS>(fe_mul<FS>(fe_mul<FS>(neg_rho, z1m), b0), fe_mul<FS>(rho_c, cip_m))));
    store_pt<LANES>(&pts[3], D);                    store_fe<LANES>(scs + 3 * 8, fe_from_mont<FS>(rho));
    {   // chal^-1 for all rounds with ONE inversion (Montgomery's trick, as upstream's ark_ff::batch_inversion)
        fe_t pre[20]; fe_t run = ks.one;
        for (uint32_t j = 0; j < k; ++j) { pre[j] = run; run = fe_mul<FS>(run, chal_m[j]); }
        fe_t inv_run = fe_inv<FS>(run, ks);
        for (int j = (int)k - 1; j >= 0; --j) {
            const fe_t ch_inv = fe_mul<FS>(inv_run, pre[j]);
            inv_run = fe_mul<FS>(inv_run, chal_m[j]);
            store_fe<LANES>(scs + (size_t)(4 + 2 * j) * 8, fe_from_mont<FS>(fe_mul<FS>(rho_c, ch_inv)));
            store_fe<LANES>(scs + (size_t)(5 + 2 * j) * 8, fe_from_mont<FS>(fe_mul<FS>(rho_c, chal_m[j])));
        }
    }
    const fe_t xi = load_scalar_checked(polyscale + (size_t)b * 8);
    fe_t xi_i = ks.one;
    uint32_t o = 4 + 2 * k;
    for (uint32_t i = 0; i < sh.ncomms; ++i) {
        const fe_t wgt = fe_mul<FS>(rho_c, xi_i);
        if (i == sh.expand_slot) {                            // a linear combination in place of the point: the MSM evaluates it
            for (uint32_t j = 0; j < IPA_EXPAND; ++j, ++o) {
                put(o, j == 0 ? *ex.p0 : load_point_checked<FB>(ex.pts + ((size_t)b * (IPA_EXPAND - 1) + (j - 1)) * 16, kb, pts_ok),
                    fe_from_mont<FS>(fe_mul<FS>(wgt, ex.sc[(size_t)b * ex.stride + j])), j == 0 && sh.shared_expand0 != 0);
            }
        } else {
            const uint32_t *cp = (i == sh.override_slot && comm_override) ? comm_override + (size_t)b * 16 : comms + ((size_t)b * sh.ncomms + i) * 16;
            put(o, load_point_checked<FB>(cp, kb, pts_ok), fe_from_mont<FS>(wgt), i < 64 && (((i < 32 ? sh.shared_lo >> i : sh.shared_hi >> (i - 32)) & 1u) != 0));
            ++o;
        }
        xi_i = fe_mul<FS>(xi_i, xi);
    }
    store_fe<LANES>(out_sigma + (size_t)b * 8, fe_from_mont<FS>(sigma));
    if (!pts_ok && coop_writer<LANES>()) *bad_input = 1u;         // any malformed point in any proof: the batch verdict is 0
}

// Scalars of the batch-shared points (IpaShape::shared_*): their sum over the batch -> the `nsh` tail entries of the list (canonical words; a sum
// mod r does not care about the representation).  One block per shared entry.
template <int FS>
__global__ void __launch_bounds__(256)
ipa_shared_tail_kernel(uint32_t batch, uint32_t nsh, uint32_t per, const uint32_t *__restrict__ shared_sc, uint32_t *__restrict__ scalars) { mb_wave_prio();
    __shared__ fe_t red[256];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    fe_t acc = fe_zero();
    for (uint32_t b = tid; b < batch; b += 256) acc = fe_add<FS>(acc, load_fe<FS>(shared_sc + ((size_t)b * nsh + q) * 8));
    red[tid] = acc;
    __syncthreads();
    for (uint32_t s = 128; s; s >>= 1) { if (tid < s) red[tid] = fe_add<FS>(red[tid], red[tid + s]); __syncthreads(); }
    if (tid == 0) for (int i = 0; i < 8; ++i) scalars[((size_t)batch * per + q) * 8 + i] = red[0].v[i];
}
// the culprit search re-checks slices of the rows: give the proofs [lo, lo + cnt) their own scalars of the shared points back
__global__ void ipa_shared_restore_kernel(uint32_t lo, uint32_t cnt, uint32_t nsh, uint32_t per, const uint32_t *__restrict__ shared_off,
                                          const uint32_t *__restrict__ shared_sc, uint32_t *__restrict__ scalars) { mb_wave_prio();
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (size_t)cnt * nsh * 8) return;
    const uint32_t w = (uint32_t)(gid & 7u), q = (uint32_t)((gid >> 3) % nsh); const size_t b = lo + (gid >> 3) / nsh;
    scalars[(b * per + shared_off[q]) * 8 + w] = shared_sc[(b * nsh + q) * 8 + w];
}

// U_b = to_group(t_b) for the split transcript: one lane per proof, t in Montgomery form from the hand-over buffer
template <int FB>
__global__ void __launch_bounds__(64)
ipa_to_group_kernel(uint32_t batch, uint32_t per, FieldK kb, const uint32_t *__restrict__ xfer, affine_t *__restrict__ out_points) { mb_wave_prio();
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const fe_t t = load_fe<FB>(xfer + (size_t)b * IPA_XFER_WORDS + 26);
    out_points[(size_t)b * per + 2] = bw_to_group<FB>(t, kb);
}

// verdict[0] = 1 iff  A + sign * B == identity  (sign = +1: A == -B ; sign = -1: A == B)
template <int F>
__global__ void xyzz_compare_kernel(const xyzz_t *__restrict__ a, const xyzz_t *__restrict__ b, int negate_b, uint32_t *__restrict__ verdict,
                                    const uint32_t *__restrict__ bad_input = nullptr) { mb_wave_prio();
    if (threadIdx.x || blockIdx.x) return;
    if (bad_input && *bad_input) { *verdict = 0u; return; }
    xyzz_t A = *a, B = *b;
    if (negate_b) B.y = fe_neg<F>(B.y);
    bool ai = xyzz_is_inf(A), bi = xyzz_is_inf(B), eq;
    if (ai || bi) eq = ai && bi;
    else eq = fe_eq(fe_mul<F>(A.x, B.zz), fe_mul<F>(B.x, A.zz)) && fe_eq(fe_mul<F>(A.y, B.zzz), fe_mul<F>(B.y, A.zzz));
    *verdict = eq ? 1u : 0u;
}

// sg points of a folded batch: canonical words -> Montgomery, with the deserialiser's checks (canonical, on the curve);
// any malformed point raises the batch's flag (the folded verdict is then 0 and the caller falls back to per-proof checks)
template <int F>
__global__ void points_to_mont_checked_kernel(uint32_t n, const uint32_t *__restrict__ in_words, FieldK kb, affine_t *__restrict__ out,
                                              uint32_t *__restrict__ bad_input) { mb_wave_prio();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool ok = true;
    out[i] = load_point_checked<F>(in_words + (size_t)i * 16, kb, ok);
    if (!ok) *bad_input = 1u;
}

// A (xyzz) == affine point q (canonical words; zeros = infinity) ?
template <int F>
__global__ void xyzz_eq_affine_kernel(const xyzz_t *__restrict__ a, const uint32_t *__restrict__ q_words, fe_t r2, uint32_t *__restrict__ verdict) {
    if (threadIdx.x) return;                                  // one block per comparison: a[b] vs q_words[16 b ..] -> verdict[b]
    a += blockIdx.x; q_words += (size_t)blockIdx.x * 16; verdict += blockIdx.x;
    xyzz_t A = *a;
    const fe_t qxw = load_fe<F>(q_words), qyw = load_fe<F>(q_words + 8);
    if (!fe_words_canonical<F>(qxw) || !fe_words_canonical<F>(qyw)) { *verdict = 0u; return; }   // alias encodings are rejected, as upstream's deserialiser does
    fe_t qx = fe_to_mont<F>(qxw, r2), qy = fe_to_mont<F>(qyw, r2);
    bool qi = fe_is_zero(qx) && fe_is_zero(qy), ai = xyzz_is_inf(A), eq;
    if (ai || qi) eq = ai && qi;
    else eq = fe_eq(fe_mul<F>(qx, A.zz), A.x) && fe_eq(fe_mul<F>(qy, A.zzz), A.y);
    *verdict = eq ? 1u : 0u;
}

// the grouped culprit search: the accumulator commitments of a whole batch with ONE malformed word per proof (a part of the search fails iff it holds one)
template <int F>
__global__ void points_to_mont_checked_each_kernel(uint32_t n, const uint32_t *__restrict__ in_words, FieldK kb, affine_t *__restrict__ out, uint32_t *__restrict__ bad) { mb_wave_prio();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool ok = true;
    out[i] = load_point_checked<F>(in_words + (size_t)i * 16, kb, ok);
    bad[i] = ok ? 0u : 1u;
}
// one block per part p: flags[p] = 1 iff  A[p] + sign * B[p] == identity  and no proof of [begin[p], end[p]) has its malformed word set (bad may be null)
template <int F>
__global__ void __launch_bounds__(64)
xyzz_compare_parts_kernel(const xyzz_t *__restrict__ a, const xyzz_t *__restrict__ b, int negate_b, const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end,
                          const uint32_t *__restrict__ bad, uint32_t nbad, uint32_t *__restrict__ flags) { mb_wave_prio();
    const uint32_t p = blockIdx.x;
    int any = 0;
    if (bad) { const uint32_t e = end[p] < nbad ? end[p] : nbad; for (uint32_t i = begin[p] + threadIdx.x; i < e; i += 64) any |= bad[i] != 0; }
    any = __syncthreads_or(any);
    if (threadIdx.x) return;
    if (any) { flags[p] = 0u; return; }
    xyzz_t A = a[p], B = b[p];
    if (negate_b) B.y = fe_neg<F>(B.y);
    bool ai = xyzz_is_inf(A), bi = xyzz_is_inf(B), eq;
    if (ai || bi) eq = ai && bi;
    else eq = fe_eq(fe_mul<F>(A.x, B.zz), fe_mul<F>(B.x, A.zz)) && fe_eq(fe_mul<F>(A.y, B.zzz), fe_mul<F>(B.y, A.zzz));
    flags[p] = eq ? 1u : 0u;
}

}  // namespace mb

// ------------------------------------------------------------------------------------------------
// a10: accumulator check
// exchange variant: the shard's folded check is decided by the caller; here only "this shard held no malformed point"
__global__ void fold_export_flag_kernel(const uint32_t *__restrict__ malformed, uint32_t *__restrict__ verdict) { if (threadIdx.x == 0) verdict[0] = malformed[0] ? 0u : 1u; }

// out[i] = in[i] * lambda (canonical words in and out; lambda by value: no upload, no synchronisation)
struct Words8 { uint32_t v[8]; };
template <int F>
__global__ void scale_words_kernel(uint32_t n, FieldK fk, const uint32_t *__restrict__ in, Words8 lambda, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe_t a, l;
    for (int j = 0; j < 8; ++j) { a.v[j] = in[(size_t)i * 8 + j]; l.v[j] = lambda.v[j]; }
    const fe_t r = fe_from_mont<F>(fe_mul<F>(fe_to_mont<F>(a, fk.r2), fe_to_mont<F>(l, fk.r2)));
    for (int j = 0; j < 8; ++j) out[(size_t)i * 8 + j] = r.v[j];
}

int mb_accumulator_check_dev(mina_ctx *c, int curve, uint32_t k, size_t batch, const uint32_t *d_prechal,
                                 const uint32_t *d_sg_words, const uint32_t *d_rho, uint32_t *d_verdict, const FoldExport *fx) {
    SrsState &s = c->srs[curve];
    if (s.depth == 0) return fail(MINA_ERR_STATE, "SRS not loaded for this curve");
    if (k < 1 || k > 20 || ((size_t)1 << k) > s.depth) return fail(MINA_ERR_ARG, "2^k exceeds the SRS depth");
    const int FS = scalar_field_of(curve), FB = base_field_of(curve);
    const uint32_t n = 1u << k;
    int rc;
    if (fx && batch > 1) {
        // The exchange variant ADDS the shards' partial sums, so no proof of any shard may carry a coefficient an adversary can predict: the opening leg draws its
        // own powers (pow_first), and until round 5 this leg trusted the caller's acc_rho (a caller following upstream's rho_0 = 1, or fixed test randomisers,
        // re-opened the +t / -t cancellation between shards).  Now every acc_rho[b] is multiplied by ONE scalar this call draws from the OS CSPRNG:
        // both sides of the shard's check scale by it, so a good shard stays good, and the cross-shard sum is a combination with G unknown coefficients.
        Words8 lam; uint8_t raw[32];
        if (!mb_secure_random(raw, 32)) return fail(MINA_ERR_STATE, "no entropy for the shard's accumulator randomiser");
        raw[31] &= 0x3f; raw[0] |= 1;                                  // < 2^254 < p, and not zero
        memcpy(lam.v, raw, 32);
        if ((rc = c->L->acc_rho_scaled.ensure(batch * 32))) return rc;
        DISPATCH_FIELD(FS, { scale_words_kernel<F_><<<cdiv(batch, 64), 64, 0, c->L->stream>>>((uint32_t)batch, c->fk[F_], d_rho, lam, c->L->acc_rho_scaled.as<uint32_t>()); });
        HIPC(hipGetLastError());
        d_rho = c->L->acc_rho_scaled.as<uint32_t>();
    }
    if ((rc = c->L->ipa_chals.ensure(batch * k * 32))) return rc;
    if ((rc = c->L->ipa_folded.ensure((size_t)n * 32))) return rc;
    if ((rc = c->L->ipa_xyzz_a.ensure(sizeof(xyzz_t)))) return rc;
    if ((rc = c->L->ipa_xyzz_b.ensure(sizeof(xyzz_t)))) return rc;
    if (batch == 1) {                                            // prechallenges -> coefficients in one launch
        if ((rc = mb_bpoly_single_from_prechallenges(c, FS, k, d_prechal, c->L->ipa_folded.as<uint32_t>(), 1))) return rc;
    } else {
        DISPATCH_FIELD(FS, { challenge_to_field_kernel<F_><<<cdiv(batch * k, 64), 64, 0, c->L->stream>>>((uint32_t)(batch * k), c->fk[F_], d_prechal, c->L->ipa_chals.as<uint32_t>()); });
        if ((rc = mb_bpoly_fold(c, FS, k, batch, c->L->ipa_chals.as<uint32_t>(), d_rho, c->L->ipa_folded.as<uint32_t>()))) return rc;
    }
    if (fx && batch > 1) {       // the exchange variant over several GPUs: the caller folds the shards' vectors and runs the MSM over its slice of the bases
        HIPC(hipMemcpyAsync(fx->acc_scalars, c->L->ipa_folded.p, (size_t)n * 32, hipMemcpyDeviceToDevice, c->L->stream));
        if ((rc = c->L->ipa_points.ensure(batch * sizeof(affine_t)))) return rc;
        if ((rc = c->L->ipa_sigma.ensure(4))) return rc;
        HIPC(hipMemsetAsync(c->L->ipa_sigma.p, 0, 4, c->L->stream));
        DISPATCH_FIELD(FB, { points_to_mont_checked_kernel<F_><<<cdiv(batch, 256), 256, 0, c->L->stream>>>((uint32_t)batch, d_sg_words, c->fk[F_], c->L->ipa_points.as<affine_t>(), c->L->ipa_sigma.as<uint32_t>()); });
        if ((rc = mb_msm_variable(c, curve, (uint32_t)batch, d_rho, c->L->ipa_points.p, fx->acc_point, nullptr))) return rc;
        fold_export_flag_kernel<<<1, 64, 0, c->L->stream>>>(c->L->ipa_sigma.as<uint32_t>(), d_verdict);      // verdict word = "no malformed commitment in this shard"
        HIPC(hipGetLastError());
        return MINA_OK;
    }
    if ((rc = mb_msm_fixed(c, curve, n, c->L->ipa_folded.as<uint32_t>(), nullptr, c->L->ipa_xyzz_a.p))) return rc;
    if (batch == 1) {
        DISPATCH_FIELD(FB, { xyzz_eq_affine_kernel<F_><<<1, 64, 0, c->L->stream>>>(c->L->ipa_xyzz_a.as<xyzz_t>(), d_sg_words, c->fk[F_].r2, d_verdict); });
    } else {
        if ((rc = c->L->ipa_points.ensure(batch * sizeof(affine_t)))) return rc;
        if ((rc = c->L->ipa_sigma.ensure(4))) return rc;            // malformed-input flag of this folded batch
        HIPC(hipMemsetAsync(c->L->ipa_sigma.p, 0, 4, c->L->stream));
        DISPATCH_FIELD(FB, { points_to_mont_checked_kernel<F_><<<cdiv(batch, 256), 256, 0, c->L->stream>>>((uint32_t)batch, d_sg_words, c->fk[F_], c->L->ipa_points.as<affine_t>(), c->L->ipa_sigma.as<uint32_t>()); });
        if ((rc = mb_msm_variable(c, curve, (uint32_t)batch, d_rho, c->L->ipa_points.p, nullptr, c->L->ipa_xyzz_b.p))) return rc;
        DISPATCH_FIELD(FB, { xyzz_compare_kernel<F_><<<1, 64, 0, c->L->stream>>>(c->L->ipa_xyzz_a.as<xyzz_t>(), c->L->ipa_xyzz_b.as<xyzz_t>(), 0, d_verdict, c->L->ipa_sigma.as<uint32_t>()); });
    }
    HIPC(hipGetLastError());
    return MINA_OK;
}

// `count` INDEPENDENT checks (no random folding: one verdict word each) through ONE kernel pipeline: the count MSMs are
// problems of the multi-problem pipeline, so the ~14 dependent dispatches of a check are paid once per group.
static int accumulator_check_multi_dev(mina_ctx *c, int curve, uint32_t k, size_t count, const uint32_t *d_prechal,
                                       const uint32_t *d_sg_words, uint32_t *d_verdicts) {
    SrsState &s = c->srs[curve];
    if (s.depth == 0) return fail(MINA_ERR_STATE, "SRS not loaded for this curve");
    if (k < 1 || k > 20 || ((size_t)1 << k) > s.depth) return fail(MINA_ERR_ARG, "2^k exceeds the SRS depth");
    const int FS = scalar_field_of(curve), FB = base_field_of(curve);
    const uint32_t n = 1u << k;
    int rc;
    if ((rc = c->L->ipa_folded.ensure(count * n * 32))) return rc;
    if ((rc = c->L->ipa_xyzz_a.ensure(count * sizeof(xyzz_t)))) return rc;
    if ((rc = mb_bpoly_single_from_prechallenges(c, FS, k, d_prechal, c->L->ipa_folded.as<uint32_t>(), (uint32_t)count))) return rc;
    if ((rc = mb_msm_table(c, curve, s.table.p, s.depth, s.c, s.W, 0, n, (uint32_t)count, c->L->ipa_folded.as<uint32_t>(), nullptr, c->L->ipa_xyzz_a.p))) return rc;
    DISPATCH_FIELD(FB, { xyzz_eq_affine_kernel<F_><<<(uint32_t)count, 64, 0, c->L->stream>>>(c->L->ipa_xyzz_a.as<xyzz_t>(), d_sg_words, c->fk[F_].r2, d_verdicts); });
    HIPC(hipGetLastError());
    return MINA_OK;
}

extern "C" int mina_accumulator_check_multi_dev(mina_ctx *c, int curve, uint32_t k, size_t count, const void *d_prechallenges,
                                                const void *d_sg, void *d_verdicts) {
    if (!c || !d_prechallenges || !d_sg || !d_verdicts) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (count == 0 || count > 64) return fail(MINA_ERR_ARG, "count must be in 1..64");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    return accumulator_check_multi_dev(c, curve, k, count, (const uint32_t *)d_prechallenges, (const uint32_t *)d_sg, (uint32_t *)d_verdicts);
}

extern "C" int mina_accumulator_check_dev(mina_ctx *c, int curve, uint32_t k, size_t batch, const void *d_prechallenges,
                                          const void *d_sg, const void *d_rho, void *d_verdict) {
    if (!c || !d_prechallenges || !d_sg || !d_verdict || (batch > 1 && !d_rho)) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (batch == 0 || batch > (1u << 20)) return fail(MINA_ERR_ARG, "bad batch");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    return mb_accumulator_check_dev(c, curve, k, batch, (const uint32_t *)d_prechallenges, (const uint32_t *)d_sg, (const uint32_t *)d_rho, (uint32_t *)d_verdict);
}

// per-proof verdicts for the `count` proofs already staged in ipa_in_a (prechallenges) / ipa_in_b (sg) of the current lane
static int accumulator_check_each(mina_ctx *c, int curve, uint32_t k, size_t count, uint8_t *verdicts) {
    constexpr size_t GROUP = 16;
    int rc;
    if ((rc = c->L->ipa_verdict.ensure(GROUP * 4))) return rc;
    for (size_t b = 0; b < count; b += GROUP) {
        const size_t g = count - b < GROUP ? count - b : GROUP;
        if ((rc = accumulator_check_multi_dev(c, curve, k, g, c->L->ipa_in_a.as<uint32_t>() + b * k * 4, c->L->ipa_in_b.as<uint32_t>() + b * 16,
                                              c->L->ipa_verdict.as<uint32_t>()))) return rc;
        uint32_t v[GROUP];
        if ((rc = d2h_sync(c, v, c->L->ipa_verdict, g * 4))) return rc;
        for (size_t i = 0; i < g; ++i) verdicts[b + i] = v[i] ? 1 : 0;
    }
    return MINA_OK;
}

extern "C" int mina_accumulator_check_batch(mina_ctx *c, int curve, uint32_t k, size_t batch, const uint8_t *prechallenges,
                                            const uint8_t *sg, const uint8_t *rho, uint8_t *verdicts) {
    if (!c || !prechallenges || !sg || !verdicts || (batch > 1 && !rho)) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (batch == 0 || batch > (1u << 20)) return fail(MINA_ERR_ARG, "bad batch");
    if (c->srs[curve].depth == 0) return fail(MINA_ERR_STATE, "SRS not loaded for this curve");
    if (k < 1 || k > 20 || ((size_t)1 << k) > c->srs[curve].depth) return fail(MINA_ERR_ARG, "k must be in 1..20 with 2^k <= SRS depth");
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = h2d(c, c->L->ipa_in_a, prechallenges, batch * k * 16))) return rc;
    if ((rc = h2d(c, c->L->ipa_in_b, sg, batch * 64))) return rc;
    if (batch > 1 && (rc = h2d(c, c->L->ipa_in_c, rho, batch * 32))) return rc;
    if ((rc = c->L->ipa_verdict.ensure(64))) return rc;
    if ((rc = mb_accumulator_check_dev(c, curve, k, batch, c->L->ipa_in_a.as<uint32_t>(), c->L->ipa_in_b.as<uint32_t>(),
                                    batch > 1 ? c->L->ipa_in_c.as<uint32_t>() : nullptr, c->L->ipa_verdict.as<uint32_t>()))) return rc;
    uint32_t v = 0;
    if ((rc = d2h_sync(c, &v, c->L->ipa_verdict, 4))) return rc;
    if (v || batch == 1) { memset(verdicts, v ? 1 : 0, batch); return MINA_OK; }
    // the folded check failed: every proof on its own (rare path), groups of independent checks per pipeline
    return accumulator_check_each(c, curve, k, batch, verdicts);
}

// host-buffer form of the un-folded group check: per-proof verdicts, no randomness involved
extern "C" int mina_accumulator_check_multi(mina_ctx *c, int curve, uint32_t k, size_t count, const uint8_t *prechallenges,
                                            const uint8_t *sg, uint8_t *verdicts) {
    if (!c || !prechallenges || !sg || !verdicts) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (count == 0 || count > (1u << 20)) return fail(MINA_ERR_ARG, "bad count");
    if (c->srs[curve].depth == 0) return fail(MINA_ERR_STATE, "SRS not loaded for this curve");
    if (k < 1 || k > 20 || ((size_t)1 << k) > c->srs[curve].depth) return fail(MINA_ERR_ARG, "k must be in 1..20 with 2^k <= SRS depth");
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = h2d(c, c->L->ipa_in_a, prechallenges, count * k * 16))) return rc;
    if ((rc = h2d(c, c->L->ipa_in_b, sg, count * 64))) return rc;
    return accumulator_check_each(c, curve, k, count, verdicts);
}

// ------------------------------------------------------------------------------------------------
// The transcript stage of the check: workspaces, the malformed word cleared, phase 1, the group map (beside phase 2 on the lane's second stream where the context
// has one), phase 2, the sums of the batch-shared scalars.  Leaves the rows on the current lane -- ipa_points / ipa_scalars (batch * per + nshared entries), ipa_chals,
// ipa_sigma, ipa_shared, ipa_shared_off -- and the malformed-input word at d_verdict[1]; the side stream has joined the lane's stream when it returns.
// lanes_ran / side_ran (may be null): the lane form the transcripts ran in and whether the group map went to the side stream (mina_selftest_ipa_rows reports them).
static int ipa_transcript_stage(mina_ctx *c, int curve, const mb::IpaShape &sh, const mb::IpaDevIn &in, uint32_t *d_verdict, int *lanes_ran, bool *side_ran) {
    SrsState &s = c->srs[curve];
    const int FB = base_field_of(curve), FS = scalar_field_of(curve);
    const size_t batch = sh.batch; const uint32_t k = sh.k;
    int rc;
    if (sh.nshared && (sh.ncomms > 64 || sh.nshared > 64)) return fail(MINA_ERR_ARG, "shared entries need <= 64 commitments");
    const size_t npoints = batch * sh.per + sh.nshared;           // per-proof lists, then the batch-shared points once
    if ((rc = c->L->ipa_points.ensure(npoints * sizeof(affine_t)))) return rc;
    if ((rc = c->L->ipa_scalars.ensure(npoints * 32))) return rc;
    if ((rc = c->L->ipa_chals.ensure(batch * k * 32))) return rc;
    if ((rc = c->L->ipa_sigma.ensure(batch * 32))) return rc;
    if ((rc = c->L->ipa_folded.ensure(((size_t)1 << k) * 32))) return rc;
    if ((rc = c->L->ipa_xyzz_a.ensure(sizeof(xyzz_t)))) return rc;
    if ((rc = c->L->ipa_xyzz_b.ensure(sizeof(xyzz_t)))) return rc;
    if (sh.nshared) { if ((rc = c->L->ipa_shared.ensure(batch * sh.nshared * 32))) return rc; if ((rc = c->L->ipa_shared_off.ensure(sh.nshared * 4))) return rc; }
    HIPC(hipMemsetAsync(d_verdict, 0, 8, c->L->stream));
    const PoseidonParams *pp = c->pparams[FB].as<PoseidonParams>();
    { ProfScope ps_(c, PS_IPA_TRANSCRIPT);
    {
        // the transcript splits at its first squeeze: to_group (one lane per proof) runs on a second stream beside the rest
        const mina_verify_tuning tune = mb_tune();
        Lane &L = *c->L;
        if ((rc = L.ipa_xfer.ensure(batch * mb::IPA_XFER_WORDS * 4))) return rc;
        // second stream only for a context that runs ONE call at a time: with pipeline lanes in flight the other lanes fill the chip, and a
        // side stream per lane would make 2 x lanes streams share the 16 hardware queues (lanes then serialise behind each other's kernels)
        const bool side = c->nlanes == 1 && tune.ipa_side_stream != 0 && !c->is_view;      // (a view context creates no streams: ctx.h)
        hipStream_t tg = L.stream;
        if (side) {
            if (!L.aux) { HIPC(hipStreamCreateWithFlags(&L.aux, hipStreamNonBlocking)); HIPC(hipEventCreateWithFlags(&L.ev_fork, hipEventDisableTiming)); HIPC(hipEventCreateWithFlags(&L.ev_join, hipEventDisableTiming)); }
            tg = L.aux;
        }
        const int ln = transcript_lanes(c, batch, (size_t)tune.ipa_coop8_max);
        auto prepare = [&](auto phase) {                        // phase 1: the transcript up to its first squeeze, phase 2: the rest
            return with_lanes<16, 8, 3>(ln, [&](auto lanes) {
                constexpr int LN = decltype(lanes)::value, PH = decltype(phase)::value;
                DISPATCH_CURVE(curve, {
                    mb::ipa_prepare_kernel<C_, LN, PH><<<cdiv(coop_threads<LN>(batch), 64), 64, 0, L.stream>>>(
                        sh, c->fk[FB], c->fk[FS], pp, in.state, in.pos, in.cip, in.lr, in.delta, in.sg, in.z1, in.z2, in.pts, in.r,
                        in.xi, in.comms, in.comm_override, in.expand, in.rb, in.sb, s.h.as<affine_t>(), L.ipa_points.as<affine_t>(), L.ipa_scalars.as<uint32_t>(),
                        L.ipa_chals.as<uint32_t>(), L.ipa_sigma.as<uint32_t>(), d_verdict + 1, L.ipa_xfer.as<uint32_t>(), L.ipa_shared.as<uint32_t>(), L.ipa_shared_off.as<uint32_t>());
                });
                return MINA_OK;
            });
        };
        if ((rc = prepare(std::integral_constant<int, 1>{}))) return rc;
        if (side) { HIPC(hipEventRecord(L.ev_fork, L.stream)); HIPC(hipStreamWaitEvent(L.aux, L.ev_fork, 0)); }
        DISPATCH_FIELD(FB, { mb::ipa_to_group_kernel<F_><<<cdiv(batch, 64), 64, 0, tg>>>((uint32_t)batch, sh.per, c->fk[F_], L.ipa_xfer.as<uint32_t>(), L.ipa_points.as<affine_t>()); });
        if (side) HIPC(hipEventRecord(L.ev_join, L.aux));
        if ((rc = prepare(std::integral_constant<int, 2>{}))) return rc;
        if (side) HIPC(hipStreamWaitEvent(L.stream, L.ev_join, 0));
        if (lanes_ran) *lanes_ran = ln;
        if (side_ran) *side_ran = side;
    }
    }
    HIPC(hipGetLastError());
    if (sh.nshared) { DISPATCH_FIELD(FS, { mb::ipa_shared_tail_kernel<F_><<<sh.nshared, 256, 0, c->L->stream>>>(sh.batch, sh.nshared, sh.per, c->L->ipa_shared.as<uint32_t>(), c->L->ipa_scalars.as<uint32_t>()); }); }
    return MINA_OK;
}

// a8: combined opening check, inputs resident in HBM (structure-of-arrays, see IpaDevIn).  Queued on the current lane, no host
// synchronisation: d_verdict[0] = 1 iff the folded check holds, d_verdict[1] = malformed-input flag.
int mb_ipa_batch_check_dev(mina_ctx *c, int curve, mb::IpaShape sh, const mb::IpaDevIn &in, uint32_t *d_verdict, const FoldExport *fx) {
    const int FB = base_field_of(curve), FS = scalar_field_of(curve);
    const size_t batch = sh.batch; const uint32_t k = sh.k;
    int rc;
    if (fx) sh.pow_first = 1;          // partial sums that the caller adds to other shards': no coefficient-1 proof (ctx.h IpaShape::pow_first)
    if ((rc = ipa_transcript_stage(c, curve, sh, in, d_verdict, nullptr, nullptr))) return rc;
    const size_t npoints = batch * sh.per + sh.nshared;
    if ((rc = mb_bpoly_fold(c, FS, k, batch, c->L->ipa_chals.as<uint32_t>(), c->L->ipa_sigma.as<uint32_t>(), c->L->ipa_folded.as<uint32_t>()))) return rc;
    if (fx) {                        // the exchange variant over several GPUs: scalars and the variable-base partial go to the caller
        HIPC(hipMemcpyAsync(fx->ipa_scalars, c->L->ipa_folded.p, ((size_t)1 << k) * 32, hipMemcpyDeviceToDevice, c->L->stream));
        if ((rc = mb_msm_variable(c, curve, (uint32_t)npoints, c->L->ipa_scalars.as<uint32_t>(), c->L->ipa_points.p, fx->ipa_point, nullptr))) return rc;
        fold_export_flag_kernel<<<1, 64, 0, c->L->stream>>>(d_verdict + 1, d_verdict);     // [1] = malformed flag of the transcripts -> [0] = 1 unless malformed
        HIPC(hipGetLastError());
        return MINA_OK;
    }
    if ((rc = mb_msm_fixed(c, curve, 1u << k, c->L->ipa_folded.as<uint32_t>(), nullptr, c->L->ipa_xyzz_a.p))) return rc;
    if ((rc = mb_msm_variable(c, curve, (uint32_t)npoints, c->L->ipa_scalars.as<uint32_t>(), c->L->ipa_points.p, nullptr, c->L->ipa_xyzz_b.p))) return rc;
    DISPATCH_FIELD(FB, { xyzz_compare_kernel<F_><<<1, 64, 0, c->L->stream>>>(c->L->ipa_xyzz_a.as<xyzz_t>(), c->L->ipa_xyzz_b.as<xyzz_t>(), 1, d_verdict, d_verdict + 1); });
    HIPC(hipGetLastError());
    c->ipa_rows = c->L; c->ipa_rows_batch = sh.batch; c->ipa_rows_k = k; c->ipa_rows_per = sh.per; c->ipa_rows_nshared = sh.nshared; c->ipa_rows_curve = curve;
    return MINA_OK;
}

// The rows ipa_prepare_kernel left on a lane (per proof: `per` (point, scalar) pairs, the k challenges and the fold weight) already carry the
// batch's randomisers rho^b, sigma^b, so the rows of any subset of proofs ARE a folded check of that subset: fold + the two MSMs + the
// comparison, no transcript work.  mina_state_job_batch's search for the culprits of a failed batch runs this on slices, one lane each.
// The caller has synchronised the lane that holds the rows.
int mb_ipa_recheck_rows(mina_ctx *c, size_t lo, size_t cnt, uint32_t *d_verdict) {
    Lane *src = c->ipa_rows;
    if (!src || cnt == 0 || lo + cnt > c->ipa_rows_batch) return fail(MINA_ERR_STATE, "no prepared rows for that range");
    const int curve = c->ipa_rows_curve, FB = base_field_of(curve), FS = scalar_field_of(curve);
    const uint32_t k = c->ipa_rows_k, per = c->ipa_rows_per;
    Lane &L = *c->L;
    int rc;
    if ((rc = L.ipa_folded.ensure(((size_t)1 << k) * 32))) return rc;
    if ((rc = L.ipa_xyzz_a.ensure(sizeof(xyzz_t)))) return rc;
    if ((rc = L.ipa_xyzz_b.ensure(sizeof(xyzz_t)))) return rc;
    HIPC(hipMemsetAsync(d_verdict, 0, 8, L.stream));
    if (const uint32_t nsh = c->ipa_rows_nshared)              // the slice's proofs get their own scalars of the batch-shared points back (idempotent)
        mb::ipa_shared_restore_kernel<<<cdiv(cnt * nsh * 8, 256), 256, 0, L.stream>>>((uint32_t)lo, (uint32_t)cnt, nsh, per, src->ipa_shared_off.as<uint32_t>(), src->ipa_shared.as<uint32_t>(), src->ipa_scalars.as<uint32_t>());
    if ((rc = mb_bpoly_fold(c, FS, k, cnt, src->ipa_chals.as<uint32_t>() + lo * k * 8, src->ipa_sigma.as<uint32_t>() + lo * 8, L.ipa_folded.as<uint32_t>()))) return rc;
    if ((rc = mb_msm_fixed(c, curve, 1u << k, L.ipa_folded.as<uint32_t>(), nullptr, L.ipa_xyzz_a.p))) return rc;
    if ((rc = mb_msm_variable(c, curve, (uint32_t)(cnt * per), src->ipa_scalars.as<uint32_t>() + lo * per * 8, src->ipa_points.as<affine_t>() + lo * per, nullptr, L.ipa_xyzz_b.p))) return rc;
    DISPATCH_FIELD(FB, { xyzz_compare_kernel<F_><<<1, 64, 0, L.stream>>>(L.ipa_xyzz_a.as<xyzz_t>(), L.ipa_xyzz_b.as<xyzz_t>(), 1, d_verdict, d_verdict + 1); });
    HIPC(hipGetLastError());
    return MINA_OK;
}

// ------------------------------------------------------------------------------------------------
// The grouped culprit search (api_state.hip): every part of a round in one pass on the current lane.
size_t mb_search_parts_cap(mina_ctx *c, int curve, uint32_t k) {
    const SrsState &s = c->srs[curve];
    const uint64_t by_entries = ((uint64_t)1 << 28) / (((uint64_t)1 << k) * (s.W ? s.W : 1));
    return (size_t)std::max<uint64_t>(1, std::min<uint64_t>(128, by_entries));
}

// the tables of a pass into the lane's gs_tab: [begin | end] in proofs, [begin | end] scaled by `per` (entries of the rows), then the ids of the parts whose fold
// runs on the matrix cores (mb_bpoly_seg_plan: the host knows every length), np words each.  They go through the lane's pinned staging buffer at `stage_off`: the
// passes of a round are queued back to back, each with its own MB_PARTS_STAGE * np bytes of it, and the search waits for the lane at the end of the round -- the
// buffer is free again when the next round fills it.
static int parts_tables(mina_ctx *c, uint32_t k, size_t np, const uint32_t *lo, const uint32_t *cnt, uint32_t base, uint32_t per, size_t stage_off, BpolySegPlan &plan) {
    Lane &L = *c->L;
    int rc;
    if ((rc = L.host_stage.ensure(stage_off + np * MB_PARTS_STAGE)) || (rc = L.gs_tab.ensure(np * MB_PARTS_STAGE))) return rc;      // (the caller sized the staging buffer for the whole round: no reallocation between its passes)
    uint32_t *t = (uint32_t *)((uint8_t *)L.host_stage.p + stage_off);
    for (size_t p = 0; p < np; ++p) {
        t[p] = lo[p] - base; t[np + p] = lo[p] - base + cnt[p];
        t[2 * np + p] = (lo[p] - base) * per; t[3 * np + p] = (lo[p] - base + cnt[p]) * per;
        t[4 * np + p] = 0;
    }
    plan = mb_bpoly_seg_plan(c, k, np, cnt, t + 4 * np);
    plan.d_ids = L.gs_tab.as<uint32_t>() + 4 * np;
    HIPC(hipMemcpyAsync(L.gs_tab.p, t, np * MB_PARTS_STAGE, hipMemcpyHostToDevice, L.stream));
    return MINA_OK;
}

int mb_ipa_recheck_rows_parts(mina_ctx *c, size_t np, const uint32_t *lo, const uint32_t *cnt, uint32_t *d_flags, size_t stage_off) {
    Lane *src = c->ipa_rows;
    if (!src || np == 0) return fail(MINA_ERR_STATE, "no prepared rows");
    const int curve = c->ipa_rows_curve, FB = base_field_of(curve), FS = scalar_field_of(curve);
    const uint32_t k = c->ipa_rows_k, per = c->ipa_rows_per, n = 1u << k;
    SrsState &s = c->srs[curve];
    uint32_t first = 0xffffffffu, last = 0, longest = 0;
    for (size_t p = 0; p < np; ++p) {
        if (cnt[p] == 0 || (uint64_t)lo[p] + cnt[p] > c->ipa_rows_batch) return fail(MINA_ERR_STATE, "no prepared rows for that range");
        first = std::min(first, lo[p]); last = std::max(last, lo[p] + cnt[p]); longest = std::max(longest, cnt[p]);
    }
    const uint32_t span = last - first;                         // the pass works on proofs [first, last) of the rows; the tables are relative to `first`
    Lane &L = *c->L;
    int rc;
    if ((rc = L.gs_folded.ensure(np * (size_t)n * 32)) || (rc = L.gs_xa.ensure(np * sizeof(xyzz_t))) || (rc = L.gs_xb.ensure(np * sizeof(xyzz_t)))) return rc;
    BpolySegPlan plan;
    if ((rc = parts_tables(c, k, np, lo, cnt, first, per, stage_off, plan))) return rc;
    const uint32_t *tab = L.gs_tab.as<uint32_t>();
    if (const uint32_t nsh = c->ipa_rows_nshared)              // these proofs get their own scalars of the batch-shared points back (idempotent)
        mb::ipa_shared_restore_kernel<<<cdiv((size_t)span * nsh * 8, 256), 256, 0, L.stream>>>(first, span, nsh, per, src->ipa_shared_off.as<uint32_t>(), src->ipa_shared.as<uint32_t>(), src->ipa_scalars.as<uint32_t>());
    if ((rc = mb_bpoly_fold_segments(c, FS, k, span, np, plan, tab, tab + np, src->ipa_chals.as<uint32_t>() + (size_t)first * k * 8, src->ipa_sigma.as<uint32_t>() + (size_t)first * 8, L.gs_folded.as<uint32_t>()))) return rc;
    if ((rc = mb_msm_table(c, curve, s.table.p, s.depth, s.c, s.W, 0, n, (uint32_t)np, L.gs_folded.as<uint32_t>(), nullptr, L.gs_xa.p))) return rc;
    if ((rc = mb_msm_segments(c, curve, span * per, np, longest * per, tab + 2 * np, tab + 3 * np, src->ipa_scalars.as<uint32_t>() + (size_t)first * per * 8,
                              src->ipa_points.as<affine_t>() + (size_t)first * per, nullptr, L.gs_xb.p))) return rc;
    DISPATCH_FIELD(FB, { mb::xyzz_compare_parts_kernel<F_><<<(uint32_t)np, 64, 0, L.stream>>>(L.gs_xa.as<xyzz_t>(), L.gs_xb.as<xyzz_t>(), 1, tab, tab + np, nullptr, 0, d_flags); });
    HIPC(hipGetLastError());
    return MINA_OK;
}

int mb_accumulator_parts_prepare(mina_ctx *c, int curve, uint32_t k, size_t batch, const uint32_t *d_prechal, const uint32_t *d_sg_words) {
    const int FS = scalar_field_of(curve), FB = base_field_of(curve);
    Lane &L = *c->L;
    int rc;
    if ((rc = L.gs_chals.ensure(batch * k * 32)) || (rc = L.gs_points.ensure(batch * sizeof(affine_t))) || (rc = L.gs_bad.ensure(batch * 4))) return rc;
    DISPATCH_FIELD(FS, { challenge_to_field_kernel<F_><<<cdiv(batch * k, 64), 64, 0, L.stream>>>((uint32_t)(batch * k), c->fk[F_], d_prechal, L.gs_chals.as<uint32_t>()); });
    DISPATCH_FIELD(FB, { mb::points_to_mont_checked_each_kernel<F_><<<cdiv(batch, 256), 256, 0, L.stream>>>((uint32_t)batch, d_sg_words, c->fk[F_], L.gs_points.as<affine_t>(), L.gs_bad.as<uint32_t>()); });
    HIPC(hipGetLastError());
    return MINA_OK;
}

int mb_accumulator_check_parts(mina_ctx *c, int curve, uint32_t k, size_t batch, const uint32_t *d_rho, size_t np, const uint32_t *lo, const uint32_t *cnt, uint32_t *d_flags, size_t stage_off) {
    SrsState &s = c->srs[curve];
    if (s.depth == 0 || k < 1 || k > 20 || ((size_t)1 << k) > s.depth || np == 0 || !d_rho) return fail(MINA_ERR_ARG, "bad grouped accumulator check");
    const int FS = scalar_field_of(curve), FB = base_field_of(curve);
    const uint32_t n = 1u << k;
    uint32_t longest = 0;
    for (size_t p = 0; p < np; ++p) {
        if (cnt[p] == 0 || (uint64_t)lo[p] + cnt[p] > batch) return fail(MINA_ERR_ARG, "part outside the batch");
        longest = std::max(longest, cnt[p]);
    }
    Lane &L = *c->L;
    int rc;
    if ((rc = L.gs_folded.ensure(np * (size_t)n * 32)) || (rc = L.gs_xa.ensure(np * sizeof(xyzz_t))) || (rc = L.gs_xb.ensure(np * sizeof(xyzz_t)))) return rc;
    BpolySegPlan plan;
    if ((rc = parts_tables(c, k, np, lo, cnt, 0, 1, stage_off, plan))) return rc;
    const uint32_t *tab = L.gs_tab.as<uint32_t>();
    if ((rc = mb_bpoly_fold_segments(c, FS, k, batch, np, plan, tab, tab + np, L.gs_chals.as<uint32_t>(), d_rho, L.gs_folded.as<uint32_t>()))) return rc;
    if ((rc = mb_msm_table(c, curve, s.table.p, s.depth, s.c, s.W, 0, n, (uint32_t)np, L.gs_folded.as<uint32_t>(), nullptr, L.gs_xa.p))) return rc;
    if ((rc = mb_msm_segments(c, curve, (uint32_t)batch, np, longest, tab, tab + np, d_rho, L.gs_points.p, nullptr, L.gs_xb.p))) return rc;
    DISPATCH_FIELD(FB, { mb::xyzz_compare_parts_kernel<F_><<<(uint32_t)np, 64, 0, L.stream>>>(L.gs_xa.as<xyzz_t>(), L.gs_xb.as<xyzz_t>(), 0, tab, tab + np, L.gs_bad.as<uint32_t>(), (uint32_t)batch, d_flags); });
    HIPC(hipGetLastError());
    return MINA_OK;
}

// ------------------------------------------------------------------------------------------------
// a8: combined opening check
// The openings of one call: validated, packed on the host into one staging blob, uploaded to the lane's ipa_in_a.  Fills the plain shape (none of the job's
// options) and the device pointers.  need_srs_points: the caller goes on to the fold and the fixed-base MSM over g[0..2^k).
static int ipa_stage_openings(mina_ctx *c, int curve, size_t batch, const mina_ipa_opening *op, const uint8_t *rand_base, const uint8_t *sg_rand_base,
                              bool need_srs_points, mb::IpaShape &sh, mb::IpaDevIn &in) {
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (batch == 0 || batch > (1u << 16)) return fail(MINA_ERR_ARG, "bad batch");
    SrsState &s = c->srs[curve];
    if (s.depth == 0) return fail(MINA_ERR_STATE, "SRS not loaded for this curve");
    const int FB = base_field_of(curve);
    if (!c->have_pparams[FB]) return fail(MINA_ERR_STATE, "Poseidon constants not installed for the base field");
    const uint32_t k = op[0].k, npts = op[0].n_evalpoints;
    uint32_t m = 0;                                             // commitments per opening in the device layout = the maximum;
    for (size_t b = 0; b < batch; ++b) if (op[b].n_comms > m) m = op[b].n_comms;   // shorter lists are padded with infinity
    if (m > 4096) return fail(MINA_ERR_ARG, "too many commitments in one opening");
    if (k < 1 || k > 20 || (need_srs_points && ((size_t)1 << k) > s.depth)) return fail(MINA_ERR_ARG, "2^k exceeds the SRS depth");
    for (size_t b = 0; b < batch; ++b) {
        const mina_ipa_opening &o = op[b];
        if (o.k != k || o.n_evalpoints != npts) return fail(MINA_ERR_ARG, "openings of one batch must share k and n_evalpoints");
        if (!o.lr || !o.delta || !o.sg || !o.z1 || !o.z2 || !o.combined_inner_product || !o.polyscale || !o.evalscale || !o.sponge_state ||
            (npts && !o.evalpoints) || (o.n_comms && !o.comms)) return fail(MINA_ERR_ARG, "null field in opening");
    }
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    sh.batch = (uint32_t)batch; sh.k = k; sh.npts = npts; sh.ncomms = m; sh.per = 2 * k + m + 4;

    // pack (host) -> one staging blob -> HBM
    const size_t o_state = 0, o_cip = o_state + batch * 96, o_lr = o_cip + batch * 32, o_delta = o_lr + batch * 2 * k * 64,
                 o_sg = o_delta + batch * 64, o_z1 = o_sg + batch * 64, o_z2 = o_z1 + batch * 32, o_pts = o_z2 + batch * 32,
                 o_r = o_pts + batch * npts * 32, o_xi = o_r + batch * 32, o_comms = o_xi + batch * 32, o_rb = o_comms + batch * m * 64,
                 o_sb = o_rb + 32, o_pos = o_sb + 32, total = o_pos + batch * 8;
    int rc;
    if ((rc = c->L->host_stage.ensure(total))) return rc;       // packed straight into page-locked memory
    uint8_t *blob = (uint8_t *)c->L->host_stage.p;
    memset(blob + o_comms, 0, batch * m * 64);                   // shorter commitment lists are padded with infinity = (0, 0)
    for (size_t b = 0; b < batch; ++b) {
        const mina_ipa_opening &o = op[b];
        memcpy(&blob[o_state + b * 96], o.sponge_state, 96);
        memcpy(&blob[o_cip + b * 32], o.combined_inner_product, 32);
        { uint32_t pos[2] = {o.sponge_mode, o.sponge_count}; memcpy(&blob[o_pos + b * 8], pos, 8); }
        if (o.sponge_mode > 1 || o.sponge_count > 2) return fail(MINA_ERR_ARG, "bad sponge position");
        memcpy(&blob[o_lr + b * 2 * k * 64], o.lr, (size_t)2 * k * 64);
        memcpy(&blob[o_delta + b * 64], o.delta, 64);
        memcpy(&blob[o_sg + b * 64], o.sg, 64);
        memcpy(&blob[o_z1 + b * 32], o.z1, 32);
        memcpy(&blob[o_z2 + b * 32], o.z2, 32);
        if (npts) memcpy(&blob[o_pts + b * npts * 32], o.evalpoints, (size_t)npts * 32);
        memcpy(&blob[o_r + b * 32], o.evalscale, 32);
        memcpy(&blob[o_xi + b * 32], o.polyscale, 32);
        if (o.n_comms) memcpy(&blob[o_comms + b * m * 64], o.comms, (size_t)o.n_comms * 64);   // rest stays (0, 0) = infinity: contributes nothing
    }
    memcpy(&blob[o_rb], rand_base, 32);
    memcpy(&blob[o_sb], sg_rand_base, 32);
    if ((rc = h2d(c, c->L->ipa_in_a, blob, total))) return rc;
    const uint8_t *d = c->L->ipa_in_a.as<uint8_t>();
    auto W = [&](size_t off) { return reinterpret_cast<const uint32_t *>(d + off); };
    in = mb::IpaDevIn{W(o_state), W(o_pos), W(o_cip), W(o_lr), W(o_delta), W(o_sg), W(o_z1), W(o_z2), W(o_pts), W(o_r), W(o_xi), W(o_comms), nullptr, W(o_rb), W(o_sb)};
    return MINA_OK;
}

extern "C" int mina_ipa_batch_check(mina_ctx *c, int curve, size_t batch, const mina_ipa_opening *op, const uint8_t *rand_base,
                                    const uint8_t *sg_rand_base, uint8_t *verdict) {
    if (!c || !op || !rand_base || !sg_rand_base || !verdict) return fail(MINA_ERR_ARG, "null argument");
    mb::IpaShape sh; mb::IpaDevIn in;
    int rc;
    if ((rc = ipa_stage_openings(c, curve, batch, op, rand_base, sg_rand_base, true, sh, in))) return rc;
    if ((rc = c->L->ipa_verdict.ensure(8))) return rc;          // [0] verdict, [1] malformed-input flag
    if ((rc = mb_ipa_batch_check_dev(c, curve, sh, in, c->L->ipa_verdict.as<uint32_t>()))) return rc;
    uint32_t v = 0;
    if ((rc = d2h_sync(c, &v, c->L->ipa_verdict, 4))) return rc;
    *verdict = v ? 1 : 0;
    return MINA_OK;
}

// ------------------------------------------------------------------------------------------------
// mina_selftest_ipa_rows: the transcript stage alone, on the caller's openings and the job's shape options; the rows come back as canonical bytes.  Test-facing
// (tests/test_gpu_ipa_rows.py holds them against tests/ipa_rows_model.py); nothing on a job's path.
template <int F>
__global__ void words_to_mont_kernel(uint32_t n, const uint32_t *__restrict__ in_words, fe_t r2, fe_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = fe_to_mont<F>(mb::load_fe<F>(in_words + (size_t)i * 8), r2);
}

extern "C" int mina_selftest_ipa_rows(mina_ctx *c, int curve, size_t batch, const mina_ipa_opening *op, const uint8_t *rand_base, const uint8_t *sg_rand_base,
                                      const mina_ipa_rows_options *opt, uint8_t *out_points, uint8_t *out_scalars, uint8_t *out_chals, uint8_t *out_sigma,
                                      uint8_t *out_side, uint32_t *out_offsets, uint32_t *out_flags) {
    if (!c || !op || !rand_base || !sg_rand_base || !out_points || !out_scalars || !out_chals || !out_sigma || !out_flags) return fail(MINA_ERR_ARG, "null argument");
    if (opt && opt->struct_size != sizeof(mina_ipa_rows_options)) return fail(MINA_ERR_ARG, "mina_ipa_rows_options.struct_size does not match this library");
    mb::IpaShape sh; mb::IpaDevIn in;
    int rc;
    if ((rc = ipa_stage_openings(c, curve, batch, op, rand_base, sg_rand_base, false, sh, in))) return rc;
    const int FB = base_field_of(curve), FS = scalar_field_of(curve);
    Lane &L = *c->L;
    const uint32_t m = sh.ncomms, NO = MINA_IPA_ROWS_NO_SLOT;
    uint32_t restore_lo = 0, restore_cnt = 0;
    if (opt) {
        if (opt->pow_first > 1) return fail(MINA_ERR_ARG, "pow_first is 0 or 1");
        const bool ovr = opt->override_slot != NO, exp = opt->expand_slot != NO;
        if (ovr && (opt->override_slot >= m || !opt->comm_override)) return fail(MINA_ERR_ARG, "override_slot beyond the commitments, or no comm_override");
        if (exp && opt->expand_slot >= m) return fail(MINA_ERR_ARG, "expand_slot beyond the commitments");
        if (exp && (!opt->expand_point0 || !opt->expand_points || !opt->expand_scalars)) return fail(MINA_ERR_ARG, "null argument");
        if (ovr && exp && opt->override_slot == opt->expand_slot) return fail(MINA_ERR_ARG, "one slot is both overridden and expanded");
        if (m < 64 && (opt->shared_mask >> m)) return fail(MINA_ERR_ARG, "shared_mask names a commitment beyond n_comms");
        if (exp && ((opt->shared_mask >> opt->expand_slot) & 1u)) return fail(MINA_ERR_ARG, "the expanded slot is shared through shared_expand0, not shared_mask");
        if ((uint64_t)opt->restore_lo + opt->restore_cnt > batch) return fail(MINA_ERR_ARG, "restore range beyond the batch");
        sh.pow_first = opt->pow_first; sh.override_slot = opt->override_slot; sh.expand_slot = opt->expand_slot;
        if (exp) sh.per += mb::IPA_EXPAND - 1;
        sh.shared_lo = (uint32_t)opt->shared_mask; sh.shared_hi = (uint32_t)(opt->shared_mask >> 32);
        sh.shared_h = opt->shared_h ? 1u : 0u; sh.shared_expand0 = (exp && opt->shared_expand0) ? 1u : 0u;
        sh.nshared = (uint32_t)__builtin_popcountll(opt->shared_mask) + sh.shared_h + sh.shared_expand0;
        if (sh.nshared && m > 64) return fail(MINA_ERR_ARG, "shared entries need <= 64 commitments");
        restore_lo = opt->restore_lo; restore_cnt = opt->restore_cnt;
        // the job's extra inputs: [override batch*64 | point 0 64 | points batch*7*64 | scalars batch*8*32] -> ipa_in_b; point 0 and the scalars -> Montgomery in ipa_in_c
        const size_t o_ovr = 0, o_p0 = o_ovr + (ovr ? batch * 64 : 0), o_pts = o_p0 + (exp ? 64 : 0), o_sc = o_pts + (exp ? batch * 7 * 64 : 0), total = o_sc + (exp ? batch * 8 * 32 : 0);
        if (total) {
            std::vector<uint8_t> blob(total);
            if (ovr) memcpy(&blob[o_ovr], opt->comm_override, batch * 64);
            if (exp) { memcpy(&blob[o_p0], opt->expand_point0, 64); memcpy(&blob[o_pts], opt->expand_points, batch * 7 * 64); memcpy(&blob[o_sc], opt->expand_scalars, batch * 8 * 32); }
            if ((rc = h2d(c, L.ipa_in_b, blob.data(), total))) return rc;
            HIPC(hipStreamSynchronize(L.stream));                  // (the blob is pageable host memory of this scope)
            const uint8_t *d = L.ipa_in_b.as<uint8_t>();
            if (ovr) in.comm_override = reinterpret_cast<const uint32_t *>(d + o_ovr);
            if (exp) {
                const size_t nsc = batch * mb::IPA_EXPAND;
                if ((rc = L.ipa_in_c.ensure(sizeof(mb::affine_t) + nsc * sizeof(mb::fe_t)))) return rc;
                mb::affine_t *p0 = L.ipa_in_c.as<mb::affine_t>(); mb::fe_t *sc = reinterpret_cast<mb::fe_t *>(p0 + 1);
                DISPATCH_FIELD(FB, { points_to_mont_kernel<F_><<<1, 64, 0, L.stream>>>(1, reinterpret_cast<const uint32_t *>(d + o_p0), c->fk[F_].r2, p0); });
                DISPATCH_FIELD(FS, { words_to_mont_kernel<F_><<<cdiv(nsc, 256), 256, 0, L.stream>>>((uint32_t)nsc, reinterpret_cast<const uint32_t *>(d + o_sc), c->fk[F_].r2, sc); });
                HIPC(hipGetLastError());
                in.expand.p0 = p0; in.expand.pts = reinterpret_cast<const uint32_t *>(d + o_pts); in.expand.sc = sc; in.expand.stride = mb::IPA_EXPAND;
            }
        }
    }
    if (sh.nshared && (!out_side || !out_offsets)) return fail(MINA_ERR_ARG, "null argument");
    if ((rc = L.ipa_verdict.ensure(8))) return rc;              // [1] malformed-input flag
    int lanes_ran = 0; bool side_ran = false;
    c->ipa_rows = nullptr;                                      // the lane's rows are no longer those of the last folded check (mb_ipa_recheck_rows)
    if ((rc = ipa_transcript_stage(c, curve, sh, in, L.ipa_verdict.as<uint32_t>(), &lanes_ran, &side_ran))) return rc;
    if (sh.nshared && restore_cnt)
        mb::ipa_shared_restore_kernel<<<cdiv((size_t)restore_cnt * sh.nshared * 8, 256), 256, 0, L.stream>>>(restore_lo, restore_cnt, sh.nshared, sh.per, L.ipa_shared_off.as<uint32_t>(), L.ipa_shared.as<uint32_t>(), L.ipa_scalars.as<uint32_t>());
    // everything below is queued on the lane's stream, which the stage left waiting for the side stream: the copies see the group map's points
    const size_t rows = batch * sh.per + sh.nshared;
    if ((rc = L.tmp_a.ensure(rows * 64))) return rc;
    DISPATCH_FIELD(FB, { points_from_mont_kernel<F_><<<cdiv(rows, 256), 256, 0, L.stream>>>((uint32_t)rows, L.ipa_points.as<mb::affine_t>(), L.tmp_a.as<uint32_t>()); });
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(out_points, L.tmp_a.p, rows * 64, hipMemcpyDeviceToHost, L.stream));
    HIPC(hipMemcpyAsync(out_scalars, L.ipa_scalars.p, rows * 32, hipMemcpyDeviceToHost, L.stream));
    HIPC(hipMemcpyAsync(out_chals, L.ipa_chals.p, batch * sh.k * 32, hipMemcpyDeviceToHost, L.stream));
    HIPC(hipMemcpyAsync(out_sigma, L.ipa_sigma.p, batch * 32, hipMemcpyDeviceToHost, L.stream));
    if (sh.nshared) {
        HIPC(hipMemcpyAsync(out_side, L.ipa_shared.p, batch * sh.nshared * 32, hipMemcpyDeviceToHost, L.stream));
        HIPC(hipMemcpyAsync(out_offsets, L.ipa_shared_off.p, sh.nshared * 4, hipMemcpyDeviceToHost, L.stream));
    }
    uint32_t v[2] = {0, 0};
    if ((rc = d2h_sync(c, v, L.ipa_verdict, 8))) return rc;
    out_flags[0] = v[1] ? 1u : 0u; out_flags[1] = (uint32_t)lanes_ran; out_flags[2] = side_ran ? 1u : 0u;
    return MINA_OK;
}

// ------------------------------------------------------------------------------------------------
// a12: batched Fq-sponge transcripts
extern "C" int mina_fq_sponge_run(mina_ctx *c, int curve, size_t batch, const uint8_t *tape, size_t tape_len, const uint8_t *init_state,
                                  const uint32_t *init_pos, const uint8_t *inputs, uint8_t *outputs, uint8_t *final_state, uint32_t *final_pos) {
    if (!c || !tape || (batch && tape_len && !outputs && !final_state)) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if ((init_state == nullptr) != (init_pos == nullptr)) return fail(MINA_ERR_ARG, "init_state and init_pos go together");
    if (batch == 0) return MINA_OK;
    if (batch > (1u << 22) || tape_len > (1u << 16)) return fail(MINA_ERR_ARG, "batch or tape too large");
    const int FB = base_field_of(curve);
    if (!c->have_pparams[FB]) return fail(MINA_ERR_STATE, "Poseidon constants not installed for the base field");
    size_t in_words = 0, out_words = 0;
    for (size_t t = 0; t < tape_len; ++t) {
        switch (tape[t]) {
            case TAPE_ABSORB_FQ: case TAPE_ABSORB_FR: in_words += 8; break;
            case TAPE_ABSORB_G: in_words += 16; break;
            case TAPE_CHALLENGE: case TAPE_CHALLENGE_FQ: case TAPE_CHALLENGE_ENDO: case TAPE_DIGEST: case TAPE_CHALLENGE_ENDO_OWN: out_words += 8; break;
            default: return fail(MINA_ERR_ARG, "unknown tape opcode");
        }
    }
    if ((in_words && !inputs) || (out_words && !outputs)) return fail(MINA_ERR_ARG, "null argument");
    if (init_pos) for (size_t b = 0; b < batch; ++b) if (init_pos[2 * b] > 1 || init_pos[2 * b + 1] > 2) return fail(MINA_ERR_ARG, "bad sponge position");
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    Lane &L = *c->L;
    if ((rc = h2d(c, L.ipa_in_a, tape, tape_len))) return rc;
    if ((rc = h2d(c, L.ipa_in_b, inputs, batch * in_words * 4))) return rc;
    if (init_state) { if ((rc = h2d(c, L.ipa_in_c, init_state, batch * 96))) return rc; if ((rc = h2d(c, L.ipa_sigma, init_pos, batch * 8))) return rc; }
    if ((rc = L.ipa_scalars.ensure(batch * (out_words ? out_words : 8) * 4))) return rc;
    if ((rc = L.ipa_points.ensure(batch * 96))) return rc;
    if ((rc = L.ipa_chals.ensure(batch * 8))) return rc;
    const PoseidonParams *pp = c->pparams[FB].as<PoseidonParams>();
    const int FS = scalar_field_of(curve);
    if ((rc = with_lanes<8, 3>(sponge_batch_lanes(batch), [&](auto lanes) {
            constexpr int LN = decltype(lanes)::value;
            DISPATCH_CURVE(curve, {
                mb::sponge_tape_kernel<C_, LN><<<cdiv(coop_threads<LN>(batch), 64), 64, 0, L.stream>>>((uint32_t)batch, (uint32_t)tape_len, (uint32_t)in_words, (uint32_t)out_words,
                    c->fk[FB], c->fk[FS], pp, L.ipa_in_a.as<uint8_t>(), init_state ? L.ipa_in_c.as<uint32_t>() : nullptr, init_state ? L.ipa_sigma.as<uint32_t>() : nullptr,
                    L.ipa_in_b.as<uint32_t>(), L.ipa_scalars.as<uint32_t>(), L.ipa_points.as<uint32_t>(), L.ipa_chals.as<uint32_t>());
            });
            return MINA_OK;
        }))) return rc;
    HIPC(hipGetLastError());
    if (final_state) HIPC(hipMemcpyAsync(final_state, L.ipa_points.p, batch * 96, hipMemcpyDeviceToHost, L.stream));
    if (final_pos) HIPC(hipMemcpyAsync(final_pos, L.ipa_chals.p, batch * 8, hipMemcpyDeviceToHost, L.stream));
    return d2h_sync(c, outputs, L.ipa_scalars, batch * out_words * 4);
}
