/*
 * mina_verify.h -- C-ABI of libminaverify.so, the MI355X-native (gfx950) Kimchi/Pickles IPA batch
 * verifier that sits behind the byte contract of lambdaclass/mina_bridge.
 *
 * What each entry point replaces (reference = /root/reference; "pin" = un-vendored crate pinned in
 * core/Cargo.toml:14-25, whose source is not in the tree -- see SURVEY.md section 0 and 8b):
 *
 *   (whole library)
 *       the verifier the bytes built at core/src/aligned.rs:31-58 are handed to
 *       (`ProvingSystemId::Mina` / `MinaAccount`; README.md:275-279,358-362: Aligned's
 *       `verify_mina_state_ffi` / `verify_account_inclusion_ffi`); this header exports the hot path
 *       of that verifier -- the combined IPA check and its kernels.
 *   mina_srs_*
 *       poly-commitment `SRS::create` and the loader for srs/vesta.srs, srs/pallas.srs
 *       (MessagePack `SRS{g,h}`; format in SURVEY.md section 0).
 *   mina_msm*
 *       ark-ec 0.3 `VariableBaseMSM::multi_scalar_mul` (pin core/Cargo.toml:20,49; README.md:538-540).
 *   mina_b_poly*, mina_ipa_*
 *       poly-commitment `b_poly`, `b_poly_coefficients`, `SRS::verify` (pin core/Cargo.toml:16;
 *       README.md:469-475,534-544).
 *   mina_poseidon_*, mina_challenge_to_field
 *       mina-poseidon `ArithmeticSponge` (PlonkSpongeConstantsKimchi), kimchi `ScalarChallenge::to_field`
 *       (pin core/Cargo.toml:14; README.md:443).
 *   mina_to_group
 *       groupmap `BWParameters::to_group` (core/Cargo.lock:2825-2827).
 *
 * Conventions
 *   - plain C types only; caller owns every host buffer; the library owns device memory, SRS tables
 *     and streams inside a `mina_ctx`.  No exceptions cross the ABI: every function returns 0 (MINA_OK)
 *     or a negative error code; verdicts are separate outputs.
 *   - field element: 32-byte little-endian canonical integer (< modulus), the ark `CanonicalSerialize`
 *     form used at core/src/sol/serialization.rs:63-86.  Values >= modulus are a caller error (upstream's
 *     deserialiser rejects them before this boundary); the arithmetic entry points (MSM, b_poly, Poseidon, Merkle) do
 *     not re-check and the result is then unspecified.  The proof-level entry points (mina_ipa_batch_check, the wire
 *     parsers) do validate and reject.
 *   - affine point: x || y, 64 bytes; the point at infinity is 64 zero bytes.
 *   - `field`: 0 = Fp (Pallas base, Vesta scalar), 1 = Fq (Vesta base, Pallas scalar).
 *   - `curve`: 0 = Pallas (base Fp, scalar Fq), 1 = Vesta (base Fq, scalar Fp).
 *   - entry points ending in `_dev` take device pointers (HBM-resident inputs) and run on the
 *     context's stream without synchronising unless stated.
 *   - a context is bound to one GPU; calls on one context are serialised by the caller
 *     (one context per thread / per rank).
 */
#ifndef MINA_VERIFY_H
#define MINA_VERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MINA_OK 0
#define MINA_ERR_ARG (-1)
#define MINA_ERR_HIP (-2)
#define MINA_ERR_STATE (-3)   /* e.g. SRS not loaded */
#define MINA_ERR_FORMAT (-4)  /* malformed bytes */

#define MINA_FIELD_FP 0
#define MINA_FIELD_FQ 1
#define MINA_CURVE_PALLAS 0
#define MINA_CURVE_VESTA 1

typedef struct mina_ctx mina_ctx;

/* ---- context -------------------------------------------------------------------------------- */
int mina_ctx_create(int device_id, mina_ctx **out);
void mina_ctx_destroy(mina_ctx *ctx);
/* last error text of the calling thread (never NULL) */
const char *mina_last_error(void);
/* block until everything queued on the context's stream has finished */
int mina_ctx_synchronize(mina_ctx *ctx);
/* the hipStream_t the `_dev` entry points are queued on: lane 0's, or the pinned lane's (for event timing and for stream-ordered work of the caller) */
void *mina_ctx_stream(mina_ctx *ctx);
/* Pin every `_dev` entry point to pipeline lane `lane` (0 <= lane < lanes; negative: back to round-robin).  While pinned, all work the library queues is
 * ordered on mina_ctx_stream(): a caller that queues its own copies / kernels / collectives on that stream needs no host synchronisation between calls
 * (the multi-GPU exchange step, SURVEY.md 8e.2: mina_bridge_amd/sharded.py).  mina_ctx_set_pipeline unpins. */
int mina_ctx_pin_lane(mina_ctx *ctx, int lane);

/* Pipelining: the `_dev` entry points are issued round-robin over `lanes` internal streams (1..32, default 1),
 * each with its own workspace, so independent calls overlap on the GPU.  mina_ctx_synchronize waits for all. */
int mina_ctx_set_pipeline(mina_ctx *ctx, int lanes);
/* Device memory for the `_dev` entry points, for callers without a HIP binding of their own (the copies are synchronous;
 * download first waits for everything queued on the context). */
int mina_dev_malloc(mina_ctx *ctx, size_t bytes, void **out);
int mina_dev_free(mina_ctx *ctx, void *p);
int mina_dev_upload(mina_ctx *ctx, void *dst, const void *src, size_t bytes);
int mina_dev_download(mina_ctx *ctx, void *dst, const void *src, size_t bytes);

/* HIP-event stage timing on the context stream.  `stage_mask` has one bit per pipeline stage (0 = off,
 * -1 = all; bit 3 = the MSM bucket-accumulate kernel).  mina_prof_read synchronises and writes a JSON object
 * {"stage": [launches, total_ms], ...} covering everything recorded since the previous read. */
int mina_prof_enable(mina_ctx *ctx, int stage_mask);
int mina_prof_read(mina_ctx *ctx, char *buf, size_t cap);

/* ---- SRS (a6) -------------------------------------------------------------------------------- */
/* Regenerate SRS{g[0..depth), h} exactly as poly-commitment `SRS::create(depth)` does
 * (BLAKE2b-512 -> field -> BW group map, K4 on the GPU) and build the MSM window tables in HBM. */
int mina_srs_create(mina_ctx *ctx, int curve, uint32_t depth);
/* Build (on != 0) or drop the pre-split form of the curve's window table: 128-byte records holding x, y and p - y as nine 29-bit limbs each, read by the accumulate
 * kernels when mina_verify_tuning.msm_fp29 = 2 (no limb conversion, no negation; twice the gather traffic, 128 MiB per curve at depth 2^16).  Without it
 * msm_fp29 = 2 behaves as 1.  Waits for the context's queued work. */
int mina_srs_split_table(mina_ctx *ctx, int curve, int on);
/* Load from the MessagePack bytes of srs/vesta.srs / srs/pallas.srs (33-byte compressed points). */
int mina_srs_load(mina_ctx *ctx, int curve, const uint8_t *msgpack, size_t len);
/* depth of the loaded SRS (0 if none) */
uint32_t mina_srs_depth(mina_ctx *ctx, int curve);
/* copy g[first..first+count) (affine, canonical bytes) / h to host */
int mina_srs_get_g(mina_ctx *ctx, int curve, uint32_t first, uint32_t count, uint8_t *out_affine);
int mina_srs_get_h(mina_ctx *ctx, int curve, uint8_t *out_affine);
/* Lagrange-basis commitments of g[0..2^k) over the radix-2 domain of size 2^k (poly-commitment `SRS::add_lagrange_basis`,
 * used by kimchi for the public-input commitment): out[i] = (1/n) sum_j w^(-ij) g[j], affine canonical bytes, n*64. */
int mina_srs_lagrange_basis(mina_ctx *ctx, int curve, uint32_t log2_domain, uint8_t *out_affine);
/* kimchi verifier's public-input commitment: h - sum_i public[i] * lagrange[i]  (i < npub; `mask_custom` with blinder 1).
 * The Lagrange basis of the domain is computed once and cached in the context. */
int mina_public_input_commitment(mina_ctx *ctx, int curve, uint32_t log2_domain, size_t npub, const uint8_t *public_inputs /* npub*32 */,
                                 uint8_t *out_affine);
/* `batch` public-input commitments at once (batch_verify computes one per proof): out[m] = h - sum_i public[m][i] * lagrange[i].
 * The first npub basis points get a fixed-base window table once; every proof is one problem of the multi-problem MSM. */
int mina_public_input_commitment_batch(mina_ctx *ctx, int curve, uint32_t log2_domain, size_t npub, size_t batch,
                                       const uint8_t *public_inputs /* batch*npub*32 */, uint8_t *out_affine /* batch*64 */);
/* serialise back to the reference's file format; *len receives the size (2 293 801 for depth 2^16) */
int mina_srs_serialize(mina_ctx *ctx, int curve, uint8_t *out, size_t cap, size_t *len);

/* ---- K1: multi-scalar multiplication (a7) ---------------------------------------------------- */
/* out = sum_i scalars[i] * bases[i]; any points (variable-base Pippenger). */
int mina_msm(mina_ctx *ctx, int curve, size_t n, const uint8_t *bases_affine, const uint8_t *scalars,
             uint8_t *out_affine);
/* out = sum_i scalars[i] * g[i], g = loaded SRS of `curve`, n <= depth (fixed-base window tables). */
int mina_msm_srs(mina_ctx *ctx, int curve, size_t n, const uint8_t *scalars, uint8_t *out_affine);
/* out = sum_i scalars[i] * g[first + i]: the slice of the SRS owned by one rank when an MSM is sharded by bases. */
int mina_msm_srs_range(mina_ctx *ctx, int curve, uint32_t first, size_t n, const uint8_t *scalars, uint8_t *out_affine);
/* nprob MSMs over the same SRS bases in ONE kernel pipeline: out[m] = sum_i scalars[m][i] * g[i], i < n.
 * (poly-commitment `SRS::commit_non_hiding` of nprob polynomials -- kimchi commits ~45 per proof; also nprob un-folded
 * accumulator MSMs.)  Each problem owns one set of 2^15 buckets; everything else is shared. */
int mina_msm_srs_multi(mina_ctx *ctx, int curve, size_t n, size_t nprob, const uint8_t *scalars /* nprob*n*32 */,
                       uint8_t *out_affine /* nprob*64 */);
/* Same with scalars already in HBM (n x 32 bytes, canonical).  Queued on the context stream; the
 * 68-byte result record {x[32], y[32], u32 is_infinity} is written to `d_out` (device memory). */
int mina_msm_srs_dev(mina_ctx *ctx, int curve, size_t n, const void *d_scalars, void *d_out);

/* ---- K2: IPA challenge polynomial (a9) ------------------------------------------------------- */
/* b_poly(chals, x) for `npoints` evaluation points */
int mina_b_poly(mina_ctx *ctx, int field, uint32_t k, const uint8_t *chals, size_t npoints,
                const uint8_t *xs, uint8_t *out);
/* s[0..2^k) = b_poly_coefficients(chals) */
int mina_b_poly_coefficients(mina_ctx *ctx, int field, uint32_t k, const uint8_t *chals, uint8_t *out);
/* folded[j] = sum_b weights[b] * b_poly_coefficients(chals[b])[j], j < 2^k  (batch fold of a8) */
int mina_b_poly_fold(mina_ctx *ctx, int field, uint32_t k, size_t batch, const uint8_t *chals /* batch*k */,
                     const uint8_t *weights /* batch */, uint8_t *out /* 2^k */);
int mina_b_poly_fold_dev(mina_ctx *ctx, int field, uint32_t k, size_t batch, const void *d_chals,
                         const void *d_weights, void *d_out);

/* ---- K3: Poseidon (a12) / challenges (a13) --------------------------------------------------- */
/* Install the sponge constants of `field`: mds[9] row-major then rc[55*3], 32-byte LE each.
 * The constants are parameters of the engine (the real fp_kimchi/fq_kimchi tables are not in the
 * reference tree). */
int mina_poseidon_set_params(mina_ctx *ctx, int field, const uint8_t *params /* (9+165)*32 */);
/* The same from the text forms upstream publishes the tables in: the JSON object of o1js' constants.ts ({"mds": [[...]], "roundConstants":
 * [[...]], ...}) or the Rust table of mina-poseidon's fp_kimchi.rs / fq_kimchi.rs (`mds: vec![...]`, `round_constants: vec![...]`); decimal
 * or 0x-hex literals, quoted or not.  Exactly 9 + 55 x 3 canonical field elements, else MINA_ERR_FORMAT.  The process-wide contexts of
 * mina_verify_* load $MINA_POSEIDON_PARAMS_FP / $MINA_POSEIDON_PARAMS_FQ (file paths) at start-up instead of the compiled-in surrogate. */
int mina_poseidon_params_parse(int field, const char *text, size_t len, uint8_t *params_out /* (9+165)*32 */);   /* host-side, no context */
int mina_poseidon_load_params(mina_ctx *ctx, int field, const char *text, size_t len);
int mina_poseidon_load_params_file(mina_ctx *ctx, int field, const char *path);
/* in-place permutation of n states (3 field elements each) */
int mina_poseidon_permute(mina_ctx *ctx, int field, size_t n, uint8_t *states /* n*96 */);
int mina_poseidon_permute_dev(mina_ctx *ctx, int field, size_t n, void *d_states);
/* n independent sponges: absorb `len` elements each (inputs: n*len*32 bytes), squeeze one. */
int mina_poseidon_hash(mina_ctx *ctx, int field, size_t n, size_t len, const uint8_t *inputs, uint8_t *out);
/* ScalarChallenge::to_field: n 128-bit challenges (16 bytes LE each) -> field, endo = endo_r of the
 * curve whose scalar field is `field`. */
int mina_challenge_to_field(mina_ctx *ctx, int field, size_t n, const uint8_t *chal128, uint8_t *out);

/* ---- a16: Merkle-path fold of Proof-of-Account (core/src/proof/account_proof.rs:9-14,30-35; README.md:358-362) ------
 * roots[i] = fold of leaves[i] along its path: node <- H_h(node, sib) for dirs = 0 (`MerkleNode::Left(sib)`: the node is
 * the left input) or H_h(sib, node) for dirs = 1 (`MerkleNode::Right(sib)`), h = 0..depth-1, with the per-height salt
 * "MinaMklTree%03d" (mina `hash_with_kimchi`).  depth <= 64.  Cooperative Poseidon in one of three lane forms: 16 lanes
 * per path while n x the context's pipeline lanes <= mina_verify_tuning.coop16_max (64), 8 lanes per path up to 8192
 * paths, wave-packed triples (21 paths per wave) above. */
int mina_merkle_roots(mina_ctx *ctx, int field, size_t n, uint32_t depth, const uint8_t *leaves /* n*32 */,
                      const uint8_t *siblings /* n*depth*32 */, const uint8_t *dirs /* n*depth */, uint8_t *roots_out /* n*32 */);
/* verdicts[i] = (root of path i == expected_roots[i]) -- the ledger-hash comparison of verify_account_inclusion */
int mina_merkle_verify_batch(mina_ctx *ctx, int field, size_t n, uint32_t depth, const uint8_t *leaves, const uint8_t *siblings,
                             const uint8_t *dirs, const uint8_t *expected_roots, uint8_t *verdicts);

/* ---- a12: batched Fq-sponge transcripts (mina-poseidon `DefaultFqSponge` over the base field of `curve`) -------------
 * Every proof of the batch runs the same `tape` of opcodes over its own input stream (inputs: per proof, the operands in
 * tape order, 32 B per field element, 64 B per point; outputs: per proof, 32 B per squeeze opcode).  4 lanes per proof.
 * init_state/init_pos (may both be NULL = fresh sponge): 3 field elements + {mode, count} per proof, as in mina_ipa_opening;
 * final_state/final_pos (may be NULL) receive the sponge after the tape. */
#define MINA_TAPE_ABSORB_FQ 0      /* base-field element */
#define MINA_TAPE_ABSORB_G 1       /* affine point (x, y); infinity absorbs (0, 0) */
#define MINA_TAPE_ABSORB_FR 2      /* scalar-field element: whole if r < q, else (x >> 1) then (x & 1) */
#define MINA_TAPE_CHALLENGE 3      /* squeeze -> low 128 bits */
#define MINA_TAPE_CHALLENGE_FQ 4   /* squeeze -> full base-field element */
#define MINA_TAPE_CHALLENGE_ENDO 5 /* squeeze 128 bits -> ScalarChallenge::to_field */
#define MINA_TAPE_DIGEST 6         /* squeeze -> scalar-field element if it fits, else 0 */
#define MINA_TAPE_CHALLENGE_ENDO_OWN 7 /* squeeze 128 bits -> to_field in the sponge's own field: kimchi's Fr-sponge
                                        (`DefaultFrSponge`) = this tape on the curve whose base field is the proof's scalar field */
int mina_fq_sponge_run(mina_ctx *ctx, int curve, size_t batch, const uint8_t *tape, size_t tape_len, const uint8_t *init_state,
                       const uint32_t *init_pos, const uint8_t *inputs, uint8_t *outputs, uint8_t *final_state, uint32_t *final_pos);

/* ---- K4: group map (a14) --------------------------------------------------------------------- */
int mina_to_group(mina_ctx *ctx, int curve, size_t n, const uint8_t *t, uint8_t *out_affine);

/* ---- field self-test hooks (used by the parity tests only) ----------------------------------- */
int mina_field_mul(mina_ctx *ctx, int field, size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out);
int mina_field_inv(mina_ctx *ctx, int field, size_t n, const uint8_t *a, uint8_t *out);
/* mina_field_inv by the divstep iteration (below: mina_ctx_set_fast_inverse) instead of the power p - 2, whatever the context's mode: the same arguments, the same
 * errors, the same bytes (0 -> 0). */
int mina_field_inv_gcd(mina_ctx *ctx, int field, size_t n, const uint8_t *a, uint8_t *out);
int mina_field_sqrt(mina_ctx *ctx, int field, size_t n, const uint8_t *a, uint8_t *out, uint8_t *out_is_square);
/* group law: the same chain of XYZZ additions/doublings on (P_i, Q_i) with the single-lane and with the 4-lane cooperative
 * routines; both results as affine points, same[i] = 1 iff the XYZZ coordinates agreed word for word at every step */
int mina_selftest_group_law(mina_ctx *ctx, int curve, size_t n, const uint8_t *p_affine, const uint8_t *q_affine,
                            uint8_t *out_serial, uint8_t *out_quad, uint8_t *same);
/* the 9 x 29-bit layer (fp29.cuh, ec29.cuh), one routine per call.  TEST-FACING: the caller owns the operand bounds (tools/fe29_bounds.py states them per call
 * site) and nothing is range-checked on the device -- an operand beyond them wraps an accumulator or a limb silently, which is what the tests look for.
 * Rows of fixed size whatever the op, uint32 words: in = MINA_FE29_IN_OPERANDS operands of 9 limbs + 1 flag word (73 words), out = MINA_FE29_OUT_RESULTS results of
 * 9 limbs + 1 flag word (37 words).  Unused slots are ignored on input and zero on output; a result of eight 32-bit words sits in limbs 0..7 of its slot.
 *   products: the pairs (a0, b0), (a1, b1), (a2, b2) in slots 0..5 (a square reads slot 0), c -- added before the reduction -- in slot 6, h / t -- added to the
 *             high half -- in slot 7; result in slot 0.  MINA_FE29_ROW1_SG: a0, a1 and c are wave-uniform by contract; its rows run one per workgroup.
 *   limb-wise forms: operands in slots 0, 1 (, 2), result in slot 0; _WORDS: slot 0 holds eight words, out slot 0 = fe29_from_words, slot 1 = fe29_to_words of it;
 *             _IS_MULTIPLE_OF_P: out flag = the bool; _LEAVE: eight canonical Montgomery-2^256 words
 *   laws:     accumulator (x, y, zz, zzz) in slots 0..3; _ADD_AFFINE: qx, qy in slots 4, 5 (qy normalised or the raw K p - y); _ADD_AFFINE_TWIN: qx, py in slots 4, 5,
 *             in flag = MINA_FE29_FLAG_NEG | MINA_FE29_FLAG_INF; _XYZZ_ADD: the second accumulator in slots 4..7; _XYZZ_LEAVE: in flag MINA_FE29_FLAG_INF, four
 *             results of eight words.  Out: the accumulator's raw limbs, out flag = MINA_FE29_FLAG_OK (the returned bool) | MINA_FE29_FLAG_INF (`inf` afterwards). */
#define MINA_FE29_IN_OPERANDS 8
#define MINA_FE29_OUT_RESULTS 4
#define MINA_FE29_FLAG_NEG 1
#define MINA_FE29_FLAG_OK 1
#define MINA_FE29_FLAG_INF 2
#define MINA_FE29_MUL_ASM 0
#define MINA_FE29_SQR_ASM 1
#define MINA_FE29_DOT2_ASM 2
#define MINA_FE29_DOT3_ASM 3
#define MINA_FE29_SQR_HI_ASM 4
#define MINA_FE29_MUL_HI_ASM 5
#define MINA_FE29_MUL_LZ 6
#define MINA_FE29_SQR_LZ 7
#define MINA_FE29_MUL_HI_LZ 8
#define MINA_FE29_MULRC_LZ 9
#define MINA_FE29_DOT2RC_LZ 10
#define MINA_FE29_DOT3RC_LZ 11
#define MINA_FE29_MUL_SG 12
#define MINA_FE29_SQR_SG 13
#define MINA_FE29_MUL_HI_SG 14
#define MINA_FE29_SQR_HI_SG 15
#define MINA_FE29_MULRC_SG 16
#define MINA_FE29_DOT2RC_SG 17
#define MINA_FE29_DOT3RC_SG 18
#define MINA_FE29_ROW1_SG 19
#define MINA_FE29_SUB_KP_ONE 32                 /* fe29_sub_kp<F, 1>: the first point of a bucket, negated */
#define MINA_FE29_KP_MINUS_NEG_Y 33             /* fe29_kp_minus<F, EC29::NEG_Y_MULT> ... */
#define MINA_FE29_KP_MINUS_SUB_X1 34
#define MINA_FE29_KP_MINUS_SUB_Y1 35
#define MINA_FE29_KP_MINUS_G_U1 36
#define MINA_FE29_KP_MINUS_G_S1 37
#define MINA_FE29_KP_MINUS_A_2B_X3_SUB 38       /* fe29_kp_minus_a_minus_2b<F, EC29::X3_SUB_MULT> / G_X3_SUB_MULT */
#define MINA_FE29_KP_MINUS_A_2B_G_X3_SUB 39
#define MINA_FE29_ADD_KP_MINUS_SUB_X3 40        /* fe29_add_kp_minus<F, EC29::SUB_X3_MULT> / G_SUB_X3_MULT */
#define MINA_FE29_ADD_KP_MINUS_G_SUB_X3 41
#define MINA_FE29_ADD 42
#define MINA_FE29_ADD3 43
#define MINA_FE29_WORDS 44
#define MINA_FE29_IS_MULTIPLE_OF_P 45
#define MINA_FE29_LEAVE 46
#define MINA_FE29_ADD_AFFINE 64
#define MINA_FE29_ADD_AFFINE_TWIN 65
#define MINA_FE29_XYZZ_ADD 66
#define MINA_FE29_XYZZ_LEAVE 67
int mina_selftest_fe29(mina_ctx *ctx, int field, int op, size_t n, const uint32_t *rows_in /* n*73 */, uint32_t *rows_out /* n*37 */);
/* the 8 x 32 layer (fp.cuh, ec.cuh, fe_inv / fe_sqrt of groupmap.cuh), one routine per call.  TEST-FACING: raw words in, raw words out -- no Montgomery conversion and no
 * range check on the device; the caller owns each routine's contract (chains: operands below p, or below 2p for _COND_SUB_P; products: sum a_i b_i < p 2^256, canonical
 * or not; laws: coordinates below p).  Rows of fixed size whatever the op, uint32 words: in = MINA_FE32_IN_OPERANDS operands of 8 words + 1 flag word (65 words, the flag
 * is reserved and ignored), out = MINA_FE32_OUT_RESULTS results of 8 words + 1 flag word (33 words).  Unused slots are ignored on input and zero on output.
 *   field:  a, b in slots 0, 1; _DOT2 / _DOT3: the pairs (a0, b0), (a1, b1), (a2, b2) in slots 0..5; result in slot 0.  _TO_MONT multiplies slot 0 by R^2 mod p, _FROM_MONT
 *           by the plain 1; _INV and _SQRT take and give Montgomery words (_SQRT: out flag MINA_FE32_FLAG_TRUE iff a square, the root -- ark's -- in slot 0, else zero);
 *           _WORDS_CANONICAL: out flag MINA_FE32_FLAG_TRUE iff the plain integer in slot 0 is below p.
 *   laws:   Montgomery words.  _DBL_AFFINE: x, y in slots 0, 1; _XYZZ_DBL: (x, y, zz, zzz) in slots 0..3; _ADD_AFFINE: the accumulator in slots 0..3, qx, qy in slots 4, 5;
 *           _XYZZ_ADD: the second operand in slots 4..7.  Out: the four raw XYZZ words.  The _QUAD forms run four lanes per row on identical operands; the result is
 *           lane 0's, and the out flag has MINA_FE32_FLAG_LANES_AGREE iff all four lanes ended with identical words. */
#define MINA_FE32_IN_OPERANDS 8
#define MINA_FE32_OUT_RESULTS 4
#define MINA_FE32_FLAG_TRUE 1
#define MINA_FE32_FLAG_LANES_AGREE 2
#define MINA_FE32_COND_SUB_P 0
#define MINA_FE32_ADD 1
#define MINA_FE32_SUB 2
#define MINA_FE32_NEG 3
#define MINA_FE32_DBL 4
#define MINA_FE32_MUL 5
#define MINA_FE32_SQR 6
#define MINA_FE32_DOT2 7
#define MINA_FE32_DOT3 8
#define MINA_FE32_TO_MONT 9
#define MINA_FE32_FROM_MONT 10
#define MINA_FE32_INV 11
#define MINA_FE32_SQRT 12
#define MINA_FE32_WORDS_CANONICAL 13
#define MINA_FE32_DBL_AFFINE 32
#define MINA_FE32_XYZZ_DBL 33
#define MINA_FE32_ADD_AFFINE 34
#define MINA_FE32_XYZZ_ADD 35
#define MINA_FE32_XYZZ_DBL_QUAD 36
#define MINA_FE32_XYZZ_ADD_QUAD 37
int mina_selftest_fe32(mina_ctx *ctx, int field, int op, size_t n, const uint32_t *rows_in /* n*65 */, uint32_t *rows_out /* n*33 */);

/* ---- a8 / a10: combined IPA check ------------------------------------------------------------ */
/* Accumulator check (a10) for `batch` proofs on the SRS of `curve`:
 *   verdicts[b] = ( MSM(g[0..2^k), b_poly_coefficients(chals_b)) == sg_b ).
 * `prechallenges`: batch*k 128-bit values (16 bytes LE), expanded with ScalarChallenge::to_field.
 * Implemented as ONE folded MSM with the caller-supplied batching randomisers `rho` (batch field
 * elements; upstream draws them from an RNG) and a search for the culprits on failure. */
int mina_accumulator_check_batch(mina_ctx *ctx, int curve, uint32_t k, size_t batch,
                                 const uint8_t *prechallenges /* batch*k*16 */, const uint8_t *sg /* batch*64 */,
                                 const uint8_t *rho /* batch*32 */, uint8_t *verdicts /* batch */);

/* Same with everything in HBM: prechallenges (batch*k*16 B), sg (batch*64 B, canonical), rho (batch*32 B,
 * may be NULL when batch == 1).  Queued on the context stream, no host synchronisation: the u32 word at
 * `d_verdict` becomes 1 iff the (folded) check holds. */
int mina_accumulator_check_dev(mina_ctx *ctx, int curve, uint32_t k, size_t batch, const void *d_prechallenges,
                               const void *d_sg, const void *d_rho, void *d_verdict);

/* `count` (<= 64) INDEPENDENT accumulator checks -- no random folding, one u32 verdict each at d_verdicts[i] -- issued as ONE
 * kernel pipeline (the MSMs are problems of the multi-problem pipeline): the fixed per-check dispatch latency is paid once
 * per group.  prechallenges count*k*16 B, sg count*64 B, all in HBM; queued, no host synchronisation. */
int mina_accumulator_check_multi_dev(mina_ctx *ctx, int curve, uint32_t k, size_t count, const void *d_prechallenges,
                                     const void *d_sg, void *d_verdicts);
/* Host-buffer form, any count (groups of 16 per pipeline): verdicts[i] = 1 iff proof i's check holds.  Deterministic --
 * the alternative to the folded check when the caller has no randomness to hand over. */
int mina_accumulator_check_multi(mina_ctx *ctx, int curve, uint32_t k, size_t count, const uint8_t *prechallenges /* count*k*16 */,
                                 const uint8_t *sg /* count*64 */, uint8_t *verdicts /* count */);

/* Combined IPA opening check `SRS::verify` (a8).  One entry = one upstream `BatchEvaluationProof`
 * (sponge, evaluation_points, polyscale, evalscale, evaluations[].commitment, opening,
 * combined_inner_product), single-chunk commitments without degree bounds. */
typedef struct {
    uint32_t k;                 /* IPA rounds; the opening is over g[0..2^k) */
    const uint8_t *lr;          /* k pairs (L_j, R_j): 2*k*64 bytes */
    const uint8_t *delta;       /* 64 */
    const uint8_t *sg;          /* 64 */
    const uint8_t *z1, *z2;     /* 32 each (scalar field) */
    uint32_t n_evalpoints;      /* evaluation points */
    const uint8_t *evalpoints;  /* n_evalpoints * 32 (scalar field) */
    uint32_t n_comms;           /* commitments being opened */
    const uint8_t *comms;       /* n_comms * 64 */
    const uint8_t *combined_inner_product; /* 32 (scalar field) */
    const uint8_t *polyscale;   /* xi, 32 */
    const uint8_t *evalscale;   /* r, 32 */
    const uint8_t *sponge_state;/* 3 * 32: Fq-sponge state (base field) handed over by the caller ... */
    uint32_t sponge_mode;       /* ... 0 = Absorbed(count), 1 = Squeezed(count) (mina-poseidon SpongeState) */
    uint32_t sponge_count;
} mina_ipa_opening;

/* poly-commitment `combined_inner_product` (single-chunk polynomials, no degree bounds): sum_i xi^i sum_j r^j evals[i][j].
 * Host-side (needs no context): the value goes into mina_ipa_opening.combined_inner_product. */
int mina_combined_inner_product(int field, size_t n_polys, size_t n_points, const uint8_t *evals /* n_polys*n_points*32 */,
                                const uint8_t *polyscale, const uint8_t *evalscale, uint8_t *out /* 32 */);

/* The openings of one call share k and n_evalpoints; n_comms may differ (proofs of different circuits), at most 4096 per opening.
 * `lr` is a bare pointer: the caller guarantees it holds 2*k points -- k is bounded (1..20, 2^k <= SRS depth) but the length of
 * the caller's buffer cannot be checked here (the container readers, mina_verify_state, do check the proof's own L/R count).
 * The proof data is validated the way upstream's deserialiser validates it before `SRS::verify` runs: every field element
 * canonical, every point on the curve (or the all-zero encoding of infinity); a malformed opening anywhere in the batch
 * gives verdict 0, never an error code (README.md:281-310: every failure is `false`). */
int mina_ipa_batch_check(mina_ctx *ctx, int curve, size_t batch, const mina_ipa_opening *openings,
                         const uint8_t *rand_base /* 32 */, const uint8_t *sg_rand_base /* 32 */,
                         uint8_t *verdict /* 1 byte: 1 = all openings valid */);

/* Test-facing, like mina_selftest_group_law / _fe29 / _fe32: the transcript stage of the opening check ALONE -- what mina_ipa_batch_check and the Proof-of-State
 * job run before the fold and the two MSMs -- and the rows it leaves, handed back as canonical little-endian bytes.  Nothing on a job's path calls it.
 * Per proof the rows are `per` (point, scalar) pairs in the order [h, sg, U, delta, L_0, R_0, .., L_{k-1}, R_{k-1}, comm_0 ..], per = 2k + n_comms + 4
 * (+ 7 with an expanded slot: that commitment becomes its 8 terms), n_comms = the largest of the batch (shorter lists are padded with infinity); behind the
 * batch * per rows come the `nshared` batch-shared points with the sums of their scalars.  Needs the SRS `h` and the Poseidon tables of the base field, NOT
 * 2^k SRS points (k = 1..20 on any SRS).  Openings are validated as by mina_ipa_batch_check; their CONTENTS need not be a valid proof.
 * The optional shape (NULL = none of it, as mina_ipa_batch_check runs) is what only the Proof-of-State job sets in production: */
#define MINA_IPA_ROWS_NO_SLOT 4294967295
typedef struct {
    uint32_t struct_size;           /* sizeof(mina_ipa_rows_options) */
    uint32_t pow_first;             /* 0 or 1: rho_b = rand_base^(b + pow_first), sigma_b likewise */
    uint32_t override_slot;         /* commitment index taken from comm_override, or MINA_IPA_ROWS_NO_SLOT */
    uint32_t expand_slot;           /* commitment index given as 8 (point, scalar) terms, or MINA_IPA_ROWS_NO_SLOT */
    const uint8_t *comm_override;   /* batch * 64 */
    const uint8_t *expand_point0;   /* 64: term 0's point, the same for every proof (trusted index data in production: not validated) */
    const uint8_t *expand_points;   /* batch * 7 * 64: the points of terms 1..7 */
    const uint8_t *expand_scalars;  /* batch * 8 * 32: canonical scalars */
    uint64_t shared_mask;           /* bit i: commitment i has the same point in every proof (bits at or beyond n_comms are an error) */
    uint32_t shared_h;              /* h is shared */
    uint32_t shared_expand0;        /* term 0 of the expanded slot is shared */
    uint32_t restore_lo, restore_cnt; /* restore_cnt > 0: proofs [restore_lo, restore_lo + restore_cnt) get their own scalars of the shared points back */
} mina_ipa_rows_options;
/* nshared = popcount(shared_mask) + (shared_h != 0) + (shared_expand0 != 0 with an expanded slot); with nshared > 0, n_comms <= 64.  Outputs, with
 * rows = batch * per + nshared: out_points rows * 64, out_scalars rows * 32 (after the shared sums and the restore), out_chals batch * k * 32, out_sigma
 * batch * 32, out_side batch * nshared * 32 (the per-proof scalars of the shared points) and out_offsets nshared words (their places in a proof's list) --
 * both may be NULL when nshared = 0 --, out_flags 3 words: [0] 1 iff some input was malformed (non-canonical element, point off the curve), [1] the lane form
 * the transcripts ran in (16, 8 or 3 lanes per proof), [2] 1 iff the group map ran on the side stream. */
int mina_selftest_ipa_rows(mina_ctx *ctx, int curve, size_t batch, const mina_ipa_opening *openings, const uint8_t *rand_base /* 32 */,
                           const uint8_t *sg_rand_base /* 32 */, const mina_ipa_rows_options *options /* may be NULL */, uint8_t *out_points,
                           uint8_t *out_scalars, uint8_t *out_chals, uint8_t *out_sigma, uint8_t *out_side, uint32_t *out_offsets, uint32_t *out_flags /* 3 */);

/* ---- wire formats of the reference (a2, a3, a4) and the inclusion part of Proof-of-Account (a16) -----------------
 * Host-side, no GPU needed for the parsers.  Layouts: api_wire.hip header / SURVEY.md 8a.  Malformed input -> MINA_ERR_FORMAT. */
typedef struct {
    uint8_t is_state_proof_from_devnet;
    uint8_t bridge_tip_state_hash[32];
    uint8_t candidate_chain_state_hashes[16][32];
    uint8_t candidate_chain_ledger_hashes[16][32];
} mina_state_pub_inputs;                       /* core/src/proof/state_proof.rs:10-25, 1057 bytes on the wire */
int mina_parse_state_pub_inputs(const uint8_t *bytes, size_t len, mina_state_pub_inputs *out);
/* MinaAccountPubInputs (account_proof.rs:18-25): ledger hash + where the ABI-encoded account sits in `bytes` */
int mina_parse_account_pub_inputs(const uint8_t *bytes, size_t len, uint8_t *ledger_hash /* 32 */, size_t *encoded_offset,
                                  size_t *encoded_len);
/* merkle_path prefix of a bincode MinaAccountProof (account_proof.rs:9-14,30-35): dirs[i] = 0 Left / 1 Right */
int mina_parse_merkle_path(const uint8_t *proof, size_t len, uint32_t max_depth, uint8_t *siblings /* max_depth*32 */,
                           uint8_t *dirs /* max_depth */, uint32_t *depth, size_t *account_offset);
/* Batched inclusion check of `verify_account_inclusion` (README.md:358-362): for each i parse proof i's Merkle path and
 * pub input i's ledger hash, fold leaf_hashes[i] along the path on the GPU and compare.  The leaf (account) hash is
 * supplied by the caller: hashing the binprot account is a "next" row.  Malformed entries -> verdict 0. */
int mina_verify_account_inclusion(mina_ctx *ctx, size_t n, const uint8_t *const *proofs, const size_t *proof_lens,
                                  const uint8_t *const *pub_inputs, const size_t *pub_lens, const uint8_t *leaf_hashes /* n*32 */,
                                  uint8_t *verdicts /* n */);

/* ---- Samasika chain selection (spec: reference README.md:619-735 + img/consensus0{3,7,8}.png) -------
 * Host-side.  The verifier runs it between the candidate tip and the bridge's tip (README.md:290-294). */
#define MINA_MAX_SUB_WINDOWS 16
typedef struct {
    uint32_t slots_per_sub_window;      /* v: window shift, in slots (mainnet 7) */
    uint32_t sub_windows_per_window;    /* window length in sub-windows (mainnet 11) */
} mina_consensus_params;
typedef struct {                        /* fields of ProtocolState.body.consensus_state used by chain selection */
    uint32_t blockchain_length;
    uint32_t epoch_count;
    uint32_t curr_global_slot;
    uint32_t min_window_density;
    uint32_t sub_window_densities[MINA_MAX_SUB_WINDOWS];
    uint8_t staking_lock_checkpoint[32];   /* previous-epoch data */
    uint8_t next_lock_checkpoint[32];      /* current-epoch data */
    uint8_t last_vrf_output_hash[32];      /* digest compared lexicographically (hashLastVRF) */
    uint8_t state_hash[32];                /* hashState, compared lexicographically */
} mina_consensus_state;
int mina_consensus_project_window(const mina_consensus_params *p, const mina_consensus_state *s, uint32_t next_global_slot,
                                  uint32_t *out_window /* sub_windows_per_window entries */);
int mina_consensus_relative_min_window_density(const mina_consensus_params *p, const mina_consensus_state *a,
                                               const mina_consensus_state *b, uint32_t *out);
int mina_consensus_is_short_range(const mina_consensus_state *a, const mina_consensus_state *b);   /* 1 / 0 */
/* selectSecureChain for one candidate: *candidate_selected = 1 if the candidate replaces the current tip */
int mina_consensus_select_secure_chain(const mina_consensus_params *p, const mina_consensus_state *tip,
                                       const mina_consensus_state *candidate, int *candidate_selected);

/* ---- protocol states: `MinaHash(ProtocolState)` (core/src/mina.rs:143-168, core/src/utils/constants.rs:22-24) -------
 * A serialized `MinaStateProtocolStateValueStableV2` (bin_prot as the reference reads it at core/src/mina.rs:164, or the bincode-of-serde
 * form inside `MinaStateProof`, core/src/proof/state_proof.rs:28-41) is flattened on the host into a fixed-size RECORD of
 * MINA_PSTATE_SLOTS field elements: slot 0 = previous_state_hash, slots 1..1+n = the body's `to_input` fields
 * (`Protocol_state.Body.to_input` packed as openmina's `Inputs::to_fields`).  The GPU then computes
 *     state_hash = H_"MinaProtoState"(previous_state_hash, H_"MinaProtoStateBody"(body fields)).
 * Host-side parsers need no context. */
#define MINA_PSTATE_SLOTS 64
#define MINA_STATES_PER_PROOF 17   /* 16 candidate-chain states (oldest .. tip) + the bridge tip state (state_proof.rs:28-41) */
#define MINA_ENC_BINPROT 0
#define MINA_ENC_BINCODE 1
typedef struct {
    uint8_t previous_state_hash[32];
    uint8_t genesis_state_hash[32];
    uint8_t snarked_ledger_hash[32];       /* body.blockchain_state.ledger_proof_statement.target.first_pass_ledger */
    uint32_t n_body_fields;
    uint32_t k, slots_per_epoch, slots_per_sub_window, sub_windows_per_window, grace_period_slots, delta;   /* body.constants (+ window length) */
    mina_consensus_state consensus;        /* state_hash is left zero: fill it with the computed hash before chain selection */
} mina_protocol_state_info;
/* *consumed (may be NULL: then the state must fill `len` exactly) receives the number of bytes read */
int mina_protocol_state_pack(const uint8_t *bytes, size_t len, int encoding, uint8_t *record /* MINA_PSTATE_SLOTS*32 */,
                             uint32_t *n_body_fields, mina_protocol_state_info *info /* may be NULL */, size_t *consumed);
/* n records -> n state hashes (and, if body_hashes_out != NULL, the n body hashes) on the GPU */
int mina_protocol_state_hash_batch(mina_ctx *ctx, size_t n, const uint8_t *records /* n*MINA_PSTATE_SLOTS*32 */,
                                   const uint32_t *n_body_fields /* n */, uint8_t *hashes_out /* n*32 */, uint8_t *body_hashes_out /* n*32 or NULL */);
/* ---- deduplicated protocol states (opt-in; changes NO result) -------------------------------------------------------
 * The proofs an operator submits within minutes share most of their 16 chain states and usually the bridge tip state.  Records i and j are THE SAME iff their
 * n_body_fields agree (clamped to MINA_PSTATE_SLOTS - 1, as the hash kernels clamp them) and their first 1 + n_body_fields slots are byte-identical; slots past
 * that are ignored, as the hashes ignore them.  rep[i] is the SMALLEST index whose record is the same as record i.  With the mode on, Poseidon runs once per
 * distinct record and every record takes its representative's hash: every hash, verdict and flag is bit-identical to the mode off, for every input.  It is not a
 * probabilistic shortcut: a 128-bit fingerprint only chooses where a record looks in a table, and a record joins a class only after its used slots compared
 * equal to the class owner's in full, so two different records never share a result whatever the fingerprint does.  Per call / per job, never across calls.
 *
 * Building block: device pointers, queued on the next pipeline lane, no host synchronisation.  d_records: n*MINA_PSTATE_SLOTS*32 bytes, 16-byte aligned;
 * d_nfields: n u32; d_rep: n u32; d_counts: 2 u32 {n_distinct, n_collisions} -- n_collisions counts the fingerprint matches whose records differed.
 * fingerprint_bits: 0 = the full fingerprint; 1..32 = cut it to that many bits (exists so that the collision path can be tested: rep and n_distinct are the
 * same for every value); above 32: MINA_ERR_ARG.  n <= 2^22. */
int mina_protocol_state_dedup_dev(mina_ctx *ctx, size_t n, const void *d_records, const void *d_nfields, void *d_rep, void *d_counts, uint32_t fingerprint_bits);
/* mina_protocol_state_hash_batch with the distinct records hashed once; *n_distinct (may be NULL) receives their number */
int mina_protocol_state_hash_batch_dedup(mina_ctx *ctx, size_t n, const uint8_t *records /* n*MINA_PSTATE_SLOTS*32 */, const uint32_t *n_body_fields /* n */,
                                         uint8_t *hashes_out /* n*32 */, uint8_t *body_hashes_out /* n*32 or NULL */, size_t *n_distinct);
/* Per context, default 0 (off: every code path, launch and result as without this call).  On: the protocol-state leg of mina_state_job_batch / _batch_dev /
 * _fold_dev finds the identical records of the job, hashes each distinct one once and copies the hash to the records that share it.  Workspace per lane that
 * runs such a leg: 8 B per state and a table of 16 B x the next power of two >= 2 x states.  The lane form of the hashes follows the number of
 * records, not of distinct ones (that number never leaves the device).  Switching the mode on waits for the context and restarts the statistics. */
int mina_ctx_set_state_dedup(mina_ctx *ctx, int on);
/* Waits for the context; states that went through a deduplicated leg, the distinct ones among them, and fingerprint collisions, summed since the context was
 * created or the mode was last switched on.  Any of the three pointers may be NULL. */
int mina_ctx_state_dedup_stats(mina_ctx *ctx, uint64_t *states, uint64_t *distinct, uint64_t *collisions);
/* ---- protocol states packed on the device (opt-in; changes NO result) -----------------------------------------------
 * mina_protocol_state_pack for states whose bytes already sit in HBM, and the rest of what the boundary's host pool does per proof before a job starts: find where
 * each of a proof's 17 consecutive states ends, compare the 16 ledger hashes, run chain selection between the candidate tip (state 15) and the bridge tip
 * (state 16).  Records, field counts, info structs, status bytes, `precheck` bytes and masks are bit-identical to the host path (mina_protocol_state_pack,
 * mina_consensus_select_secure_chain, the checks behind mina_verify_state_checks) for every input, malformed ones included: same length checks, four 32-byte
 * strings, at most 64 sub-windows, variant tags and booleans in range, 40 canonical field elements, at most MINA_PSTATE_SLOTS - 1 elements, the slice consumed
 * exactly.  No encoding argument: the device reads the bincode form (MINA_ENC_BINCODE) only -- the form inside `MinaStateProof`, the only one a verifier is handed;
 * bin_prot stays with the host reader.
 * Device pointers, queued on the next pipeline lane (the pinned one under mina_ctx_pin_lane), no host synchronisation.  d_records: MINA_PSTATE_SLOTS*32 bytes per
 * state, 16-byte aligned; d_nfields: u32 per state.  A null or misaligned argument: MINA_ERR_ARG.
 * State i is bytes [d_off[i], d_off[i] + d_len[i]) of the blob and must fill them exactly.  d_status[i] = 1: accepted; 0: rejected -- the record is then zero and
 * the field count 0 (d_info[i] undefined); a slice that reaches past blob_len is rejected, not a fault. */
int mina_protocol_state_pack_dev(mina_ctx *ctx, size_t n, const void *d_blob, size_t blob_len, const void *d_off /* n u64 */, const void *d_len /* n u32 */,
                                 void *d_records, void *d_nfields, void *d_info /* n mina_protocol_state_info, or NULL */, void *d_status /* n u8 */);
/* Proof b's 17 states are bytes [d_begin[b], d_end[b]) of the blob, one behind the other.  d_precheck[b] = LEDGER and CONSENSUS and (d_and ? d_and[b] != 0 : 1),
 * as mina_state_jobs.precheck takes it; d_masks[b] = the MINA_CHECK_FORMAT / _LEDGER / _CONSENSUS bits that passed.  A proof that fails FORMAT (a state rejected,
 * or the last one not ending at d_end[b], or a range past blob_len) gets zero records, zero field counts, precheck 0 and mask 0.  d_ledger_hashes: 8-byte aligned. */
int mina_state_frontend_dev(mina_ctx *ctx, size_t batch, const void *d_blob, size_t blob_len,
                            const void *d_begin, const void *d_end /* batch u64 each: the 17 states of proof b */,
                            const void *d_expected_hashes /* batch*17*32, as mina_state_jobs.expected_hashes */,
                            const void *d_ledger_hashes /* batch*16*32 */, const void *d_and /* batch u8 or NULL: host-side bits to AND in */,
                            void *d_records, void *d_nfields, void *d_precheck /* batch u8 */, void *d_masks /* batch u32 MINA_CHECK_{FORMAT,LEDGER,CONSENSUS}, or NULL */);
/* serialized states in, state hashes out */
int mina_protocol_state_hash_bytes(mina_ctx *ctx, int encoding, size_t n, const uint8_t *const *states, const size_t *lens,
                                   uint8_t *hashes_out /* n*32 */);

/* ---- the Proof-of-State job (BASELINE config C3; README.md:281-310) ------------------------------------------------
 * `batch` state proofs through ONE device pipeline: per proof the 17 protocol-state hashes + public-input comparison + chain
 * linkage, the wrap proof's public-input commitment (Pallas Lagrange MSM; its result replaces commitment `pub_comm_slot` of
 * the opening), the wrap proof's combined IPA opening (folded over the batch) and the step accumulator check (Vesta 2^acc_k
 * bases, folded with acc_rho).  Sections are structure-of-arrays over the batch; layouts as in mina_ipa_opening /
 * mina_accumulator_check_batch.  A section is skipped when its `with_*` flag (or npub) is 0. */
struct mina_kimchi_proofs;
typedef struct {
    size_t batch;
    /* (1) protocol states */
    int with_states;
    const void *state_records;    /* batch*17 records (mina_protocol_state_pack) */
    const void *state_nfields;    /* batch*17 u32 */
    const void *expected_hashes;  /* batch*17*32: candidate_chain_state_hashes[16] then bridge_tip_state_hash (state_proof.rs:10-25) */
    const void *precheck;         /* batch bytes from host-side checks (ledger hashes, consensus), NULL = all pass */
    /* (2) wrap proof public input (scalar field of Pallas) */
    uint32_t log2_domain, npub, pub_comm_slot;
    const void *public_inputs;    /* batch*npub*32 */
    /* (3) wrap proof opening (Pallas) */
    int with_ipa;
    uint32_t k, n_evalpoints, n_comms;
    const void *sponge_state /* b*96 */, *sponge_pos /* b*2 u32 {mode, count} */, *cip /* b*32 */, *lr /* b*2k*64 */, *delta /* b*64 */,
               *sg /* b*64 */, *z1, *z2 /* b*32 */, *evalpoints /* b*n_evalpoints*32 */, *evalscale, *polyscale /* b*32 */, *comms /* b*n_comms*64 */;
    const void *rand_base, *sg_rand_base;   /* 32 each */
    /* (3') instead of the derived rows above (sponge_state, sponge_pos, cip, evalpoints, evalscale, polyscale, comms): the raw wrap
     * proofs; kimchi `oracles` + `to_batch` then run on the GPU against the installed verifier index (k = its domain, n_evalpoints = 2,
     * n_comms = n_prev + 45; lr, delta, sg, z1, z2 still come from the fields above).  The struct lives on the host; its inner
     * pointers are host or device addresses like every other section. */
    const struct mina_kimchi_proofs *kimchi;
    /* (4) step accumulator (Vesta) */
    int with_accumulator;
    uint32_t acc_k;
    const void *acc_prechallenges /* b*acc_k*16 */, *acc_sg /* b*64 */, *acc_rho /* b*32 */;
} mina_state_jobs;
/* one-off set-up that needs host synchronisation (prefix salts; Lagrange basis of the domain + window table of its first npub points) */
int mina_state_jobs_prepare(mina_ctx *ctx, uint32_t log2_domain, uint32_t npub);
/* Every pointer of `jobs` is a DEVICE pointer.  Queued on the next pipeline lane, no host synchronisation.
 * d_verdicts: batch u32, 1 = proof accepted.  d_flags (may be NULL): 4 u32 {folded IPA ok, IPA input malformed, folded accumulator ok, 0};
 * when a folded check fails every verdict of the batch is 0 (the host-buffer form below then finds the culprits). */
int mina_state_job_batch_dev(mina_ctx *ctx, const mina_state_jobs *jobs, void *d_verdicts, void *d_flags);
/* SURVEY.md 8e.2 for the whole job -- several GPUs, ONE exchange step (the multi-GPU variant north_star names): this shard's proofs through every stage of the
 * job except the two fixed-base MSMs and their comparisons; the shard's folded scalar vectors and variable-base partial sums are handed to the caller instead
 * (device buffers: d_ipa_scalars 2^k * 32 B and d_ipa_point 17 words for the wrap openings on Pallas -- fixed-base part + point must be infinity;
 * d_acc_scalars 2^acc_k * 32 B and d_acc_point 17 words for the step accumulators on Vesta -- fixed-base part must equal the point).  The caller
 * exchanges the vectors (all-to-all), commits over its slice of the SRS (mina_msm_srs_range_dev) and reduces the partial points (mina_points_sum_dev):
 * mina_bridge_amd/sharded.py ShardedStateJob.  d_verdicts[b] = the per-proof checks only.  batch >= 2, with_ipa and with_accumulator set.
 * Soundness of the sum over shards: here the opening fold runs with rho_b = rand_base^(b + 1), sigma_b = sg_rand_base^(b + 1) -- NOT upstream's ^b, whose first
 * proof carries coefficient 1: partial sums of G shards are added, and G coefficient-1 proofs could cancel each other's discrepancies.  Every shard draws its own
 * rand_base / sg_rand_base from a CSPRNG after its proofs are fixed.  The accumulator fold no longer depends on the caller for that (round 6): the library multiplies
 * every acc_rho[b] by ONE scalar it draws from the OS CSPRNG per call (both sides of the shard's check scale by it), so upstream's rho_0 = 1 or fixed test
 * randomisers cannot re-open the cancellation between shards; random acc_rho (b = 0 included) remain the recommendation. */
int mina_state_job_fold_dev(mina_ctx *ctx, const mina_state_jobs *jobs, void *d_verdicts, void *d_flags, void *d_ipa_scalars, void *d_ipa_point,
                            void *d_acc_scalars, void *d_acc_point);
/* Host-buffer form: one upload, the pipeline, one download; on a folded failure the failing range is cut into four parts ($MINA_SEARCH_FAN) that are
 * re-checked concurrently (and failing parts cut again) so that every proof gets its own verdict byte; the opening check of well-formed
 * proofs is re-checked from the rows of the failed batch, without repeating the transcripts. */
int mina_state_job_batch(mina_ctx *ctx, const mina_state_jobs *jobs, uint8_t *verdicts /* batch */);
/* Per-proof verdicts for a job whose inputs are already in HBM: mina_state_job_batch without its staging copy (the two share one body).  `jobs` as for
 * mina_state_job_batch_dev (device pointers).  Runs the job on the next pipeline lane (the pinned one under mina_ctx_pin_lane); if a folded check fails, runs the
 * job's per-proof part again without the folded legs and searches the failed legs for their culprits (in groups or over the fan, as the context is set).  Writes
 * d_verdicts[b] = 1 / 0 (u32 per proof) and, if d_flags is not NULL, the four words mina_state_job_batch_dev writes for the WHOLE job.  SYNCHRONISES ITS LANE: when
 * it returns the verdicts are in d_verdicts.  Call mina_state_jobs_prepare first. */
int mina_state_job_each_dev(mina_ctx *ctx, const mina_state_jobs *jobs, void *d_verdicts /* batch u32 */, void *d_flags /* 4 u32 or NULL */);
/* The masks form of the job: which checks ran and which passed (bit masks of MINA_CHECK_*, below) for EVERY proof of a batch, from ONE pass of the job -- what
 * mina_verify_account_ctx / mina_account_job_dev answer for the account side.  `jobs` as for mina_state_job_batch_dev (device pointers); jobs->precheck is NOT read:
 * the host checks have their own bits in d_front.  Per proof b the inputs are front = d_front[b] (the MINA_CHECK_FORMAT | _LEDGER | _CONSENSUS bits that passed, as
 * mina_state_frontend_dev writes d_masks; d_front may be NULL: absent), deny = d_deny[b] (MINA_CHECK_* bits the caller has already decided fail; NULL: 0), the job's
 * section flags, chain (all 17 hashes equal the expected ones and states 1..15 name their predecessor), stmt (the Pickles statement is well-formed) and ipa_each /
 * acc_each (the proof is not a culprit of the opening leg / of the accumulator leg).  The rule (csrc/state_masks.h, one host/device function):
 *   ran = FORMAT.
 *   If `front` is present and lacks FORMAT, or `deny` has FORMAT: passed = 0, nothing else is in `ran`, and the proof is done.
 *   Otherwise passed = FORMAT.
 *   With `front` present: ran |= LEDGER | CONSENSUS and passed |= front & (LEDGER | CONSENSUS).  Without it, neither bit runs.
 *   with_states: ran |= CHAIN; passed iff `chain`.
 *   with_accumulator: ran |= ACCUMULATOR; passed iff `acc_each`.
 *   with_ipa: ran |= KIMCHI; passed iff `stmt && ipa_each`.
 *   Finally passed &= ~deny.  `ran` is not touched by `deny`.
 * The job runs once with every requested leg, on the next pipeline lane (the pinned one under mina_ctx_pin_lane); a kernel then keeps the chain word of every proof
 * apart from the folded verdicts.  Both folded checks good: the only host read is the four flag words.  A folded check failed: that leg is searched for its culprits
 * as mina_state_job_each_dev searches it (in groups or over the fan, counted by mina_ctx_search_stats) -- and no state is hashed a second time.  Writes d_passed[b] /
 * d_ran[b] and, if d_flags is not NULL, the four words mina_state_job_each_dev writes.  MINA_ERR_ARG for a null d_passed / d_ran or a pointer that is not 4-byte
 * aligned, before any launch.  SYNCHRONISES ITS LANE.  Call mina_state_jobs_prepare first.
 * mina_state_job_checks: the host-buffer form (every pointer a host pointer; uploads as mina_state_job_batch does, lane 0).
 * mina_ctx_checks_stats: the full job passes the checks calls of the context have queued (one per call, whatever fails) and the proofs in them. */
int mina_state_job_checks_dev(mina_ctx *ctx, const mina_state_jobs *jobs, const void *d_front /* batch u32 or NULL */, const void *d_deny /* batch u32 or NULL */,
                              void *d_passed /* batch u32 */, void *d_ran /* batch u32 */, void *d_flags /* 4 u32 or NULL */);
int mina_state_job_checks(mina_ctx *ctx, const mina_state_jobs *jobs, const uint32_t *front, const uint32_t *deny, uint32_t *passed, uint32_t *ran);
int mina_ctx_checks_stats(mina_ctx *ctx, uint64_t *jobs, uint64_t *proofs);
/* The grouped culprit search (off by default).  groups = 0: the fan search above.  groups = G in 2 .. 128: each failed leg starts with failing = {[0, batch)};
 * every round cuts every failing range [lo, lo + cnt) of more than one proof into g = min(G, cnt) parts [lo + cnt*q/g, lo + cnt*(q+1)/g), checks ALL parts of the
 * round in one pass on the job's own lane (mina_b_poly_fold_segments_dev's fold, the fixed-base MSM with one problem per part, mina_msm_segments_dev's MSM, one
 * comparison launch, one wait, one read-back of a flag per part) and keeps the parts that fail; a failing range of one proof is a culprit.  ceil(log_G batch) rounds
 * instead of ceil(log_4 batch), no lane but the job's, no stream created.  A round is split into passes only beyond min(128, 2^28 / (2^k * 16)) parts.  The opening
 * leg runs from the rows the failed batch left on its lane; where those cannot be used (malformed opening input, mina_verify_tuning.search_full, rows of another
 * batch) that leg keeps the fan search.  A part of the accumulator leg that holds a malformed commitment fails.  Verdicts are those of the fan search for every
 * input.  Measured: not on an MI355X yet -- tools/bench_search.py is the tool; the expected gain is derived from round depth and launch counts only.
 * mina_ctx_search_stats: legs searched in groups, rounds (levels) and parts (segments checked) since the context was created; functions of (batch, G, culprits). */
int mina_ctx_set_search_groups(mina_ctx *ctx, uint32_t groups);
int mina_ctx_search_stats(mina_ctx *ctx, uint64_t *searches, uint64_t *rounds, uint64_t *parts);
/* Which kernels fold the segments of mina_b_poly_fold_segments_dev and of the grouped search's rounds.  The rule, applied on the host per segment: the int8 matrix
 * cores (the single fold's GEMM with the K loop cut to the segment, neighbours masked out) where mina_verify_tuning.bpoly_mfma != 0, k >= 2 and
 * min_len <= length < 2^17 -- an int32 accumulator holds length * 2^14 only below 2^17 proofs; the VALU segmented kernels for every other non-empty segment; an empty
 * segment is all zero.  Results are the same bytes either way (exact integers modulo p).  min_len: 0 = never, else 1 .. 2^17 - 1; the default is 256, the single
 * fold's rule and the only measured crossover (not measured for segments on an MI355X yet: tools/bench_search.py --fold-mfma-min).  Workspace: 512 B x 2^k of column
 * sums per matrix-core segment, capped at a budget of 256 MiB per lane -- the segments go out in passes of max(1, 256 MiB / (512 B x 2^k)), queued back to back.
 * mina_ctx_seg_fold_stats: running totals of the context that RAN the folds -- segments folded on the matrix cores, segments folded by the VALU kernels (empty
 * segments count in neither) and matrix-core passes.  A boundary search (MINA_VERIFY_GROUPED_SEARCH) runs on a view context of its own with the default min_len;
 * its counters are not carried over to the device's context. */
int mina_ctx_set_seg_fold_mfma_min(mina_ctx *ctx, uint32_t min_len);
int mina_ctx_seg_fold_stats(mina_ctx *ctx, uint64_t *mfma_segments, uint64_t *valu_segments, uint64_t *mfma_passes);
/* The tail of an MSM -- bucket sums, bucket reduction, finish -- as ONE launch instead of five or six (opt-in).  With the mode on, every MSM that accumulates in
 * tasks (a single MSM, a segmented one, the lanes of a pipelined context; NOT the multi-problem calls that give every bucket a lane, which keep the staged tail) runs
 * one kernel behind its accumulate: a workgroup per row of 128 buckets sums the row's buckets in LDS and publishes the row's plain and weighted sums; the workgroup
 * that arrives last at a bucket set's counter totals the set, and the one that completes a problem's last set writes the result.  No workgroup waits for another.
 * Results are the same points: the 68-byte records and 64-byte points are the same bytes as with the mode off, XYZZ outputs the same point in another
 * representation.  on: 0 or 1; the default is 0.  Takes effect for the calls queued after it; a view context takes its parent's setting when it is created or
 * refreshed.  The boundary (mina_verify_*) does not use the mode.  Measured on one MI355X (tools/bench_msm_tail.py, profiles/msm_fused_tail.json): 9 kernels per lone 2^16 MSM
 * instead of 14, but a lone call is SLOWER (568 -> 646 us; a lone accumulator check 399 -> 479 us) and 16 pipelined lanes are level: for callers who pay per launch.
 * mina_ctx_msm_tail_stats: MSMs this context has queued with the fused tail and with the staged one since it was created. */
int mina_ctx_set_msm_fused_tail(mina_ctx *ctx, int on);      /* default 0; takes effect for the calls queued after it */
int mina_ctx_msm_tail_stats(mina_ctx *ctx, uint64_t *fused_runs, uint64_t *staged_runs);
/* The one field inversion at the end of every MSM -- 1 / (zz * zzz), which turns the XYZZ result into the affine record, on a single lane -- by batched divsteps
 * (Bernstein-Yang "safegcd"; mina_bridge_amd/csrc/fe_modinv.cuh) instead of the power p - 2 (opt-in).  on: 0 or 1; the default is 0.  With the mode on, the finish
 * of every MSM queued afterwards -- its own kernel, or the last step of the fused tail where mina_ctx_set_msm_fused_tail is on -- runs at most 25 batches of 30
 * branch-free divsteps on nine signed 30-bit limbs in place of 254 dependent squarings: a FIXED bound (750 divsteps, above the 741 proven to suffice for 256-bit
 * inputs), never a loop that waits for data.  The inverse of a field element is unique: records, points and verdicts are the same bytes as with the mode off.
 * The mode does not touch anything else: mina_field_inv, the square roots, SRS and Lagrange generation, the transcript kernels (kimchi, IPA, Pickles), the
 * normalisations of the state and shard paths, the launch shapes and the workspace all stay as they are, and the boundary (mina_verify_*) does not use the mode.
 * Takes effect for the calls queued after it; a view context takes its parent's setting when it is created or refreshed.
 * Measured on one MI355X (tools/bench_inverse.py, profiles/fast_inverse.json): the finish stage of a lone 2^16 MSM 198 -> 51 us, the lone MSM 569 -> 422 us wall; a
 * lone accumulator check, whose MSM hands out XYZZ and has no finish, is level.
 * mina_ctx_inverse_stats: MSM finishes this context has queued with the divstep inversion and with the power since it was created (an MSM that asks for the XYZZ
 * result of a single bucket set alone has no finish and counts in neither). */
int mina_ctx_set_fast_inverse(mina_ctx *ctx, int on);        /* default 0; takes effect for the MSMs queued after it */
int mina_ctx_inverse_stats(mina_ctx *ctx, uint64_t *gcd_finishes, uint64_t *fermat_finishes);
/* The chain inverse: the single-lane field inversions in the scalar stages of the wrap-proof chain and in the Lagrange set-up by the same divstep iteration
 * (fe_modinv.cuh) instead of the power p - 2 (opt-in, a mode of its own).  on: 0 or 1; the default is 0.  With the mode on, every launch queued afterwards of
 *   pickles_scalar_kernel, kimchi_scalar_kernel      ft_eval0 of the step and the wrap side: 1 / ((zeta - w_zk)(zeta - 1)) and one per UNNORMALIZED_LAGRANGE token
 *   kimchi_pub_kernel<8>, <10>                       the public polynomial's one Montgomery-trick inversion per lane pass
 *   kimchi_ftcomm_kernel                             the ft commitment row of mina_kimchi_to_batch
 *   pubcomm_finish16_kernel, pubcomm_finish_kernel   the public-input commitment h - A as an affine record (the job path; mina_public_input_commitment_batch)
 *   lagrange_finish_kernel, lagrange_digit_table_kernel      mina_srs_lagrange_basis and the 128 digit multiples per window of mina_state_jobs_prepare
 *   points_sum_kernel                                mina_points_sum_dev
 * is the launch of its twin `..._gcd_kernel`: the same body, arguments and launch shape with fe_inv_gcd in place of fe_inv (kimchi_pub_gcd_kernel keeps its
 * denominators in LDS, 40 KiB per workgroup at chunks of 10, where kimchi_pub_kernel<10> keeps them in scratch).  The inverse of a field element is unique: every
 * output is the same bytes as with the mode off, and with the mode off every launch, kernel and byte is what it was before the mode existed.
 * The two modes are independent: mina_ctx_set_fast_inverse is the MSM finish alone and does not imply this mode; this mode does not touch the MSM finish.
 * Left on the power whatever the modes say: ipa_prepare_kernel (its latency form keeps its challenge arrays in scratch, which the code-object contract allows
 * under that kernel's name only), the group map and the square roots, mina_field_inv, the group-law self-test hook, and every inversion the HOST computes (polish.h,
 * the host half of the Pickles statement, the single mina_public_input_commitment, the constant set-up of the fields, sponges and indexes).
 * The boundary (mina_verify_*) does not use the mode.
 * Takes effect for the calls queued after it; a view context takes its parent's setting when it is created or refreshed.
 * mina_ctx_chain_inverse_stats: launches of the kernels listed above this context has queued in the divstep form and in the power form since it was created. */
int mina_ctx_set_chain_inverse(mina_ctx *ctx, int on);       /* default 0; takes effect for the calls queued after it */
int mina_ctx_chain_inverse_stats(mina_ctx *ctx, uint64_t *gcd_launches, uint64_t *fermat_launches);
/* Two INDEX SETS per context.  Everything that belongs to an installed (wrap index, step index) pair -- device buffers, digest, commitments, the derived Tick sponge
 * state -- is one index set; a context holds two, numbered 0 and 1, and one of them is SELECTED (set 0 when the context is created).  Every installer, loader and
 * getter (mina_verifier_index_install, _load_json, _digest, mina_step_index_install, _load_json, mina_polish_tokens_from_json where it installs) and every job acts on
 * the selected set; field constants, both SRS with their Lagrange tables, the Poseidon tables and the salts are shared by both.  The boundary keeps one set per Mina
 * network (mina_verify_install_verifier_index_net).
 * Selecting is host bookkeeping only: no HIP call, no allocation, no synchronisation; launches already queued keep the buffers they captured.  Installing into a set
 * frees that set's old buffers -- the hazard of a re-install, with the same remedy.  mina_poseidon_set_params invalidates the table-derived state of BOTH sets.
 * Like the installers, not to be called while another thread queues work on the context.  set: 0 | 1, MINA_ERR_ARG otherwise. */
int mina_ctx_select_index_set(mina_ctx *ctx, uint32_t set);
uint32_t mina_ctx_index_set(const mina_ctx *ctx);
/* MIXED jobs: proofs of BOTH index sets of the context in one call (opt-in: nothing else launches these forms).  net[b] = 0 | 1 names the index set proof b is
 * checked against (the numbering of mina_ctx_select_index_set), whichever set is selected; the selection is unchanged when a call returns.  Every kernel that reads
 * index data has a `_net` twin that takes both sets' pointers and the byte array and resolves proof b's index once, then runs the body it shares with its kernel
 * (kimchi_fq / _rows / _pub / _scalar / _ftcomm, pickles_digest / _scalar `_net_kernel`); the kernels that read no index are the ones every job launches.  The
 * proofs of a mixed job therefore share one wrap-proof chain, one fold, one fixed-base MSM and one accumulator check.
 * A byte other than 0 or 1 marks THAT proof malformed (the malformed word of mina_kimchi_to_batch_net, ok[b] = 0, a 0 verdict) and is never an out-of-range read.
 * In a job the kimchi stage's malformed word is ONE word for the whole job, as for any malformed input: mina_state_job_batch_net_dev then answers 0 for every proof
 * with flags[1] = 1, and mina_state_job_each_net_dev (and the boundary's search) finds that proof alone.
 * Preconditions, checked on the host before anything is queued: net not NULL (MINA_ERR_ARG); both sets fully installed -- wrap index and step index -- and the same
 * log2_domain in both wrap indexes (MINA_ERR_STATE).  The step side of a set is prepared on its first job, mixed or not; that step synchronises, as it always has.
 * The `_net` stages of a mixed job invert by the power whatever mina_ctx_set_chain_inverse says (there are no `_gcd` twins of the `_net` kernels) and count as
 * power-form launches in mina_ctx_chain_inverse_stats; the kernels that read no index (the public-input commitment's finish) follow the mode.  In the opening check the index commitments are no longer the same point for every proof: only h stays a
 * batch-shared point, and the ft commitment is computed per proof (kimchi_ftcomm_net_kernel) instead of entering the MSM as its eight terms.
 *   mina_kimchi_to_batch_net, mina_pickles_public_inputs_batch_net    the host-buffer forms of mina_kimchi_to_batch / mina_pickles_public_inputs_batch (net: host bytes)
 *   mina_state_job_batch_net_dev, mina_state_job_each_net_dev         mina_state_job_batch_dev / mina_state_job_each_dev with d_net: batch bytes in HBM.  The culprit
 *                                                                     search of _each_ re-queues the stages with the same bytes.
 *   mina_ctx_mixed_job_stats    mixed jobs this context has queued through the two job calls since it was created (one per call, whatever fails; the passes a
 *                               culprit search re-queues are not counted) and the proofs in them by the set their byte names (a byte other than 0 / 1 counts in
 *                               neither).  The proofs are counted on the GPU, where the bytes are: the call waits for everything the context has queued.
 * The masks form (mina_state_job_checks*) has no mixed form.  (The two host-buffer forms are declared beside the calls they mirror, below.) */
int mina_state_job_batch_net_dev(mina_ctx *ctx, const mina_state_jobs *jobs, const void *d_net /* batch u8 */, void *d_verdicts, void *d_flags);
int mina_state_job_each_net_dev(mina_ctx *ctx, const mina_state_jobs *jobs, const void *d_net /* batch u8 */, void *d_verdicts /* batch u32 */, void *d_flags /* 4 u32 or NULL */);
int mina_ctx_mixed_job_stats(mina_ctx *ctx, uint64_t *jobs, uint64_t *proofs_set0, uint64_t *proofs_set1);
/* Test-facing: *live = the streams the context's lanes hold now, *made_by_searches = the streams its culprit searches have created since the context was created
 * (the fan search creates the streams its lanes lack and destroys them when it is done; the grouped search creates none and queues on the job's lane only). */
int mina_ctx_lane_streams(mina_ctx *ctx, uint32_t *live, uint64_t *made_by_searches);
/* The streams the pipelined device-resident jobs of the context (mina_state_job_batch_dev, mina_state_job_fold_dev over mina_ctx_set_pipeline lanes) may keep busy.
 * Streams run side by side only on separate hardware queues, and the process has GPU_MAX_HW_QUEUES of them, one of which serves the caller's null stream: the
 * default budget is that value (1 .. 32) less one, read when the first such job is queued.  With `lanes` jobs in flight: 4 * lanes <= budget, a lone job and a
 * pinned context fork each job's three legs onto streams of its lane (plan A); otherwise the jobs of all lanes flow FIFO through shared role streams -- one for
 * the state hashes, and s = clamp((budget - 1) / 2, 1, lanes) pairs for the two stages of the wrap-proof chain, the accumulator check and the verdict (plan B).
 * A budget with room for one stream more than those 1 + 2 s (4, 6, ...; any budget above 1 + 2 * lanes) gives plan B a second state-hash stream: the jobs of the
 * odd lanes hash on it in equal pieces, and the opening check of every other job follows its kimchi stage on the first chain stream.  Where no budget is
 * forced and four lanes or more are in flight, plan B may take the null stream's queue for that second stream (4 queues: two hash streams and one pair).
 * Verdicts are the same under every plan; mina_ctx_synchronize waits for either.  n in 1 .. 31 forces a budget (tests, tools), n <= 0 goes back to the
 * environment's.  Waits for what the context has queued. */
int mina_ctx_set_stream_budget(mina_ctx *ctx, int n);
/* The plan the context's last pipelined device-resident job was queued under: *roles = 1 under plan B, *carriers = its state-hash streams (1 or 2), *sets = its
 * chain pairs, *streams = the streams it keeps busy; all 0 under plan A and before the first such job. */
int mina_ctx_stream_plan_stats(mina_ctx *ctx, uint32_t *roles, uint32_t *carriers, uint32_t *sets, uint32_t *streams);

/* ---- multi-GPU building blocks --------------------------------------------------------------------
 * One process per GPU; RCCL moves bytes (all-to-all of scalar slices, all-gather of partial points), these entry points are the
 * reduction operators RCCL lacks.  Device pointers; queued on the next pipeline lane, no host synchronisation.
 * Point record: 68 bytes {x[32], y[32], u32 is_infinity} as written by mina_msm_srs_dev. */
int mina_challenge_to_field_dev(mina_ctx *ctx, int field, size_t n, const void *d_chal128 /* n*16 */, void *d_out /* n*32 */);
/* out[j] = sum_r in[r][j] mod p for `rows` vectors of m canonical field elements: the fold of the peers' scalar slices */
int mina_field_sum_rows_dev(mina_ctx *ctx, int field, size_t rows, size_t m, const void *d_in /* rows*m*32 */, void *d_out /* m*32 */);
/* sum_i scalars[i] * g[first + i] over this rank's slice of the SRS */
int mina_msm_srs_range_dev(mina_ctx *ctx, int curve, uint32_t first, size_t n, const void *d_scalars, void *d_out /* record */);
/* variable-base MSM over canonical affine points in HBM */
int mina_msm_dev(mina_ctx *ctx, int curve, size_t n, const void *d_bases /* n*64 */, const void *d_scalars /* n*32 */, void *d_out /* record */);
/* sum of n point records (the all-gathered partial results).  Record contract of this call and of mina_point_records_equal_dev: a record whose flag word is
 * != 0 (any non-zero value, not only 1) is the point at infinity and its 64 coordinate bytes are ignored, whatever they hold; a record whose flag word is 0 holds
 * canonical affine coordinates.  The sum skips infinity records; the comparison calls two infinity records equal and a finite record unequal to an infinity
 * record, and writes the verdict word 1 or 0 over whatever it held.  Records written here are canonical: infinity is 64 zero bytes and the word 1. */
int mina_points_sum_dev(mina_ctx *ctx, int curve, size_t n, const void *d_records /* n*68 */, void *d_out /* record */);
int mina_point_records_equal_dev(mina_ctx *ctx, const void *d_a, const void *d_b, void *d_verdict /* u32 */);
/* ---- segmented building blocks: many independent sums over ranges of ONE input array, in one launch set -------------
 * Segment s covers entries [seg_begin[s], seg_end[s]) of the arrays (u32 tables in device memory, nseg words each).  Segments may be empty, of different
 * lengths, overlapping or out of order; entries no segment names are ignored.  Both calls queue on the next pipeline lane (the pinned one under
 * mina_ctx_pin_lane).  They read the two tables back first -- 8 * nseg bytes, one wait for what the lane already holds -- because the longest segment sizes
 * the launches and a segment that breaks begin <= end <= limit is refused with MINA_ERR_ARG before any kernel is queued; they do not wait for their own
 * kernels.  Null or misaligned pointers and shapes beyond the limits are refused before the device is touched.  Measured: nothing yet (no MI355X timing of
 * either call is recorded); what the tests pin is that the bytes equal those of the single-range calls.
 *
 * mina_msm_segments_dev: d_out[s] = sum over i in segment s of scalars[i] * bases[i], a 68-byte point record each (an empty segment: is_infinity = 1), equal byte
 * for byte to mina_msm_dev over that range alone.  The segments are the problems of one multi-problem bucket pipeline: every segment owns W bucket sets of NB
 * buckets, chosen by the LONGEST segment L (W x NB = 32 x 128 for L < 2048, 20 x 4096 for L < 2^17, 18 x 16384 above), and the pipeline's limits are
 * NB * W * nseg <= 2^26 and max(L, 1) * W * nseg <= 2^28; n_total <= 2^24.  Scalars are canonical (< 2^255).  d_bases and d_scalars: 16-byte aligned.
 *
 * mina_b_poly_fold_segments_dev: d_out[s][j] = sum over b in segment s of weights[b] * b_poly_coefficients(chals[b])[j], canonical, equal byte for byte to
 * mina_b_poly_fold_dev over that range alone (both are exact sums modulo p, whichever kernels that call takes; an empty segment gives zeros).  d_weights may be
 * null (every weight 1).  nseg <= 65535, nseg * 2^k <= 2^28; d_out 16-byte aligned.  Long segments are folded on the matrix cores, the others by the VALU
 * kernels: mina_ctx_set_seg_fold_mfma_min. */
int mina_msm_segments_dev(mina_ctx *ctx, int curve, size_t n_total, size_t nseg, const void *d_seg_begin, const void *d_seg_end /* nseg u32 each */,
                          const void *d_bases /* n_total*64 canonical affine */, const void *d_scalars /* n_total*32 */, void *d_out /* nseg records */);
int mina_b_poly_fold_segments_dev(mina_ctx *ctx, int field, uint32_t k, size_t batch, size_t nseg, const void *d_seg_begin,
                                  const void *d_seg_end /* nseg u32 each, in proofs */, const void *d_chals /* batch*k*32 */,
                                  const void *d_weights /* batch*32 */, void *d_out /* nseg * 2^k * 32 */);

struct mina_pickles_statements;
/* ---- kimchi verifier for the Pickles wrap proof (a11): `oracles` + `to_batch` on the GPU ---------------------------------
 * The verifier index is DATA: the reference tree does not hold the blockchain-snark index, so the engine takes domain, shifts,
 * commitments and the linearization's constant term (a PolishToken program in the byte-code below) as a parameter. */
#define MINA_TOK_ALPHA 0
#define MINA_TOK_BETA 1
#define MINA_TOK_GAMMA 2
#define MINA_TOK_JOINT_COMBINER 3
#define MINA_TOK_ENDO_COEFFICIENT 4
#define MINA_TOK_MDS 5                    /* + u8 row, u8 col */
#define MINA_TOK_LITERAL 6                /* + 32-byte scalar */
#define MINA_TOK_CELL 7                   /* + u8 column (0 z, 1..6 selectors, 7..21 w, 22..36 coefficients, 37..42 sigma), u8 row (0 = zeta, 1 = zeta*omega) */
#define MINA_TOK_DUP 8
#define MINA_TOK_POW 9                    /* + u64 exponent */
#define MINA_TOK_ADD 10
#define MINA_TOK_MUL 11
#define MINA_TOK_SUB 12
#define MINA_TOK_VANISHES_ON_ZK_ROWS 13   /* VanishesOnZeroKnowledgeAndPreviousRows */
#define MINA_TOK_UNNORMALIZED_LAGRANGE 14 /* + i32 row offset (negative: counted back from the first zero-knowledge row; INT32_MIN: that row itself) */
#define MINA_TOK_STORE 15
#define MINA_TOK_LOAD 16                  /* + u16 cache slot */
#define MINA_TOK_SKIP_IF 17               /* + u8 feature code, u16 n: if the proof has the feature, push 0 and skip the next n tokens (kimchi SkipIf) */
#define MINA_TOK_SKIP_IF_NOT 18           /* + u8 feature code, u16 n: the same when the proof does NOT have it.  Feature codes: 0..5 the optional gates
                                             (range_check0, range_check1, foreign_field_add, foreign_field_mul, xor, rot), 6 LookupTables, 7 RuntimeLookupTables,
                                             8..11 LookupPattern Xor / Lookup / RangeCheck / ForeignFieldMul, 12 + w TableWidth(w <= 3), 16 + n LookupsPerRow(n <= 4);
                                             derived per proof from the statement's eight feature flags (csrc/polish.h).  A skipped region must net one value. */
typedef struct {
    uint32_t log2_domain;              /* evaluation domain = SRS chunk size = 2^log2_domain (wrap: 15) */
    uint32_t zk_rows;                  /* 3 */
    uint32_t perm_alpha_offset;        /* first power of alpha of the permutation argument (21) */
    const uint8_t *shifts;             /* 7 * 32, scalar field (Fq) */
    const uint8_t *sigma_comm;         /* 7 * 64 */
    const uint8_t *coefficients_comm;  /* 15 * 64 */
    const uint8_t *selector_comm;      /* 6 * 64: generic, poseidon, complete_add, mul, emul, endomul_scalar */
    const uint8_t *constant_term;      /* PolishToken byte-code of linearization.constant_term */
    size_t constant_term_len;
} mina_verifier_index;
int mina_verifier_index_install(mina_ctx *ctx, const mina_verifier_index *index);
int mina_verifier_index_digest(mina_ctx *ctx, uint8_t *out32);   /* `VerifierIndex::digest` (base-field element) */
/* File-drop forms [UPSTREAM-RECALL for every key / enum spelling; pinned by round trips against independent writers, tests/test_loaders.py]:
 * `serde_json` of kimchi's `Vec<PolishToken>` (externally tagged: "Alpha", {"Mds": {"row": r, "col": c}}, {"Literal": "<hex>"},
 * {"Cell": {"col": {"Witness": i} | "Z" | {"Index": "<gate>"} | {"Coefficient": i} | {"Permutation": i}, "row": "Curr" | "Next"}}, "Dup",
 * {"Pow": n}, "Add", "Mul", "Sub", "VanishesOnZeroKnowledgeAndPreviousRows", {"UnnormalizedLagrangeBasis": {"zk_rows": b, "offset": i}},
 * "Store", {"Load": i}, {"SkipIf" | "SkipIfNot": [<feature>, n]}; also {"Challenge": ..} / {"Constant": ..}) -> the byte-code above.
 * SkipIf / SkipIfNot: with `enabled_features` = MINA_FEATURES_RUNTIME they become MINA_TOK_SKIP_IF / _NOT and every proof's own flags decide
 * (the step index); otherwise they are resolved here against `enabled_features` (bit = feature code, see MINA_TOK_SKIP_IF_NOT; a fixed circuit
 * such as the wrap index: 0).  `optional_present`: bit i = the proofs carry optional evaluation i (wire order) -- naming another one is an
 * error -- or MINA_FEATURES_RUNTIME for "any" (the proof's presence mask decides).  `out` may be NULL to query the length.  Host-side. */
#define MINA_FEATURES_RUNTIME 0xffffffffu
int mina_polish_tokens_from_json(int field, const char *json, size_t len, uint32_t enabled_features, uint32_t optional_present, uint8_t *out,
                                 size_t cap, size_t *out_len);
/* `serde_json` of kimchi `VerifierIndex<Pallas>` (domain, zk_rows, shift, sigma_comm, coefficients_comm, generic_comm, psm_comm,
 * complete_add_comm, mul_comm, emul_comm, endomul_scalar_comm; o1-utils SerdeAs hex; 33-byte compressed points) + the constant term of its
 * linearization (`serde_json::to_string(&index.linearization.constant_term)` -- the index itself skips it) -> mina_verifier_index_install.
 * An index that enables optional gates or lookups is refused. */
int mina_verifier_index_load_json(mina_ctx *ctx, const char *index_json, size_t index_len, const char *constant_term_json, size_t ct_len,
                                  uint32_t perm_alpha_offset /* 21 for kimchi's gate set */);
typedef struct mina_kimchi_proofs {
    size_t batch;
    uint32_t n_prev, npub;             /* recursion challenges per proof (wrap: 2), public inputs per proof */
    const void *public_inputs;         /* b * npub * 32 */
    const void *prev_chals;            /* b * n_prev * k * 32 (expanded challenges, scalar field) */
    const void *prev_comms;            /* b * n_prev * 64 */
    const void *w_comm /* b*15*64 */, *z_comm /* b*64 */, *t_comm /* b*7*64 */;
    const void *evals;                 /* b * 43 * 2 * 32: column order of MINA_TOK_CELL, [zeta, zeta*omega] */
    const void *ft_eval1;              /* b * 32 */
    /* NULL, or the Pickles statements the public inputs are DERIVED from on the GPU (needs mina_step_index_install; npub must be 40
     * and public_inputs is ignored): compute_deferred_values + the message digests + the packing run ahead of `oracles`, and a
     * malformed statement fails its proof.  Host struct; inner pointers host or device like the sections above. */
    const struct mina_pickles_statements *statements;
    /* NULL, or instead of prev_chals (which may then be NULL) the 128-bit prechallenges, b * n_prev * k * 16: expanded on the GPU
     * (`ScalarChallenge::to_field` with the scalar field's endo coefficient) inside mina_state_job_batch[_dev].
     * BOTH may be NULL when `statements` is given (n_prev = 2, k = 15): the recursion challenges are then the statement's
     * messages_for_next_wrap_proof.old_bulletproof_challenges (`wrap_old_challenges`) -- the one source a verifier has -- and kimchi's
     * digest of them comes out of the statement's own sponge (15 permutations per proof that are not repeated). */
    const void *prev_prechallenges;
} mina_kimchi_proofs;
typedef struct {                       /* one `BatchEvaluationProof` row per proof, host buffers */
    uint8_t *sponge_state /* b*96 */; uint32_t *sponge_pos /* b*2 */; uint8_t *cip /* b*32 */, *evalpoints /* b*64: zeta, zeta*omega */,
            *polyscale /* b*32: v */, *evalscale /* b*32: u */, *comms /* b*(n_prev+45)*64 */, *ft_eval0 /* b*32 or NULL */;
    uint8_t *malformed;                /* 1 byte or NULL: some input was not canonical / not on the curve */
} mina_kimchi_batch_out;
int mina_kimchi_to_batch(mina_ctx *ctx, const mina_kimchi_proofs *proofs, mina_kimchi_batch_out *out);

/* ---- Pickles glue of `verify_block` (a15): statement -> deferred values -> the wrap circuit's 40 public inputs ---------------
 * openmina `compute_deferred_values` + the two message digests + `PreparedStatement::to_public_input`.  Needs, besides the wrap
 * index, the STEP circuit's data (also absent from the reference tree): zero-knowledge rows, the 7 permutation shifts of every
 * step domain in use, and the step linearization's constant term in the same PolishToken byte-code (columns: as MINA_TOK_CELL,
 * optional evaluations following at 43, 44, ... in wire order).  With a step index installed the kimchi step of mina_verify_state
 * runs on these public inputs (every statement field is then bound to the proof); without one it runs with none. */
typedef struct {
    uint32_t zk_rows;                 /* 3 */
    uint32_t n_domains;               /* step domains in use (<= 8) */
    const uint32_t *domain_log2;      /* n_domains */
    const uint8_t *shifts;            /* n_domains * 7 * 32 (Fp) */
    const uint8_t *constant_term;     /* PolishToken byte-code over Fp.  A CELL column c >= 43 names optional evaluation SLOT c - 43 (wire order);
                                         the proof's presence mask (`misc`) says where it sits among the evaluations the proof carries; naming a
                                         slot the proof lacks, outside a skipped region, fails that proof.  MINA_TOK_JOINT_COMBINER is the statement's
                                         joint combiner (endo-expanded; 0 without one); SkipIf / SkipIfNot look at the statement's feature flags. */
    size_t constant_term_len;
} mina_step_index;
int mina_step_index_install(mina_ctx *ctx, const mina_step_index *index);
/* the step side from files: one `VerifierIndex<Vesta>` JSON per step domain in use (domain, zk_rows and shift are read) + the step
 * linearization's constant term -> mina_step_index_install */
int mina_step_index_load_json(mina_ctx *ctx, size_t n_indexes, const char *const *index_jsons, const size_t *index_lens, const char *constant_term_json,
                              size_t ct_len, uint32_t enabled_features, uint32_t optional_present);
/* The statements of `batch` wrap proofs, structure-of-arrays (what `compute_deferred_values` and the two message digests read).
 * 128-bit challenges are 16 little-endian bytes; field elements 32.  Every proof of one call has the same n_old / n_evals. */
typedef struct mina_pickles_statements {
    uint32_t n_old;                     /* step-side previous accumulators per proof (0..4; Mina blockchain proof: 2) */
    uint32_t n_evals;                   /* evaluation pairs of the step proof: 43 + the optional ones present (<= 62) */
    const void *plonk;                  /* b * 64: alpha, beta, gamma, zeta */
    const void *bulletproof_challenges; /* b * 16 * 16: deferred_values.bulletproof_challenges (step, Tick rounds) */
    const void *step_old_challenges;    /* b * n_old * 16 * 16: messages_for_next_step_proof.old_bulletproof_challenges */
    const void *step_comms;             /* b * n_old * 64: messages_for_next_step_proof.challenge_polynomial_commitments */
    const void *wrap_old_challenges;    /* b * 2 * 15 * 16: messages_for_next_wrap_proof.old_bulletproof_challenges */
    const void *wrap_sg;                /* b * 64: messages_for_next_wrap_proof.challenge_polynomial_commitment */
    const void *sponge_digest;          /* b * 32: sponge_digest_before_evaluations (4 x u64, not reduced) */
    const void *prev_evals;             /* b * n_evals * 64 (Fp): kimchi column order (MINA_TOK_CELL), then the optional ones; (zeta, zeta*omega)
                                           pairs, chunked evaluations already combined with zeta^(2^16) */
    const void *prev_public_input;      /* b * 64 (Fp): the step proof's public-input evaluations */
    const void *prev_ft_eval1;          /* b * 32 (Fp) */
    const void *app_state;              /* b * 32 (Fp): the application state = hash of the tip protocol state */
    const void *misc;                   /* b * 32: [0] domain_log2, [1] proofs_verified (0..2), [2..10) feature flags, [10] has joint
                                           combiner, [11..14) little-endian presence mask of the 19 optional evaluations (wire order: 6 optional
                                           gate selectors, lookup aggregation, lookup table, 5 lookup sorted, runtime table, runtime selector,
                                           4 lookup-pattern selectors); its popcount must be n_evals - 43, [16..32) joint combiner */
} mina_pickles_statements;
/* statements -> the wrap circuit's 40 public inputs, entirely on the GPU (three sponge kernels, one scalar kernel).  Host buffers.
 * ok[b] = 0: statement b is malformed (non-canonical element, unknown step domain); its public inputs are then unspecified. */
int mina_pickles_public_inputs_batch(mina_ctx *ctx, const mina_pickles_statements *st, size_t batch, uint8_t *public_inputs_out /* b*40*32 */,
                                     uint8_t *ok /* b */);
/* The MIXED forms of mina_kimchi_to_batch and mina_pickles_public_inputs_batch ("MIXED jobs", above): proof b against index set net[b] of the context. */
int mina_kimchi_to_batch_net(mina_ctx *ctx, const mina_kimchi_proofs *proofs, const uint8_t *net /* batch */, mina_kimchi_batch_out *out);
int mina_pickles_public_inputs_batch_net(mina_ctx *ctx, const mina_pickles_statements *st, size_t batch, const uint8_t *net /* batch */, uint8_t *public_inputs_out /* b*40*32 */,
                                         uint8_t *ok /* b */);
/* one serialized wrap proof + the application state (the tip's protocol-state hash) -> public_input_out[40*32] (Fq) and, if
 * derived_out != NULL, 7*32 bytes: combined_inner_product, b, zeta^(2^16), zeta^n, perm, xi, r (Fp).  Sponges run on the GPU. */
int mina_pickles_public_input(mina_ctx *ctx, const uint8_t *wrap_proof, size_t len, int encoding, const uint8_t *app_state /* 32 */,
                              uint8_t *public_input_out, uint8_t *derived_out);

/* ---- containers (a1, a5, 8f-2) -------------------------------------------------------------------------------------
 * Serialized Pickles wrap proof (`MinaBaseProofStableV2`; bin_prot as core/src/mina.rs:235-248 reads it, or the serde/bincode form
 * at the head of `MinaStateProof`) -> one flat byte string in the fixed order the kernels consume:
 *   alpha beta gamma zeta (16 each) | has_joint_combiner (1) joint_combiner (16) | feature_flags (8) | 16 step prechallenges (16 each)
 *   | proofs_verified (1) domain_log2 (1) | sponge_digest (32) | step accumulator sg (64) | 2 x 15 wrap prechallenges
 *   | u32 n, n points | u32 n, n x 16 prechallenges | prev public-input evals | u32 count, prev evals (each: u32 n, n x 32, u32 n, n x 32)
 *   | optional-presence bytes | prev ft_eval1 | 15 w_comm, z_comm, 7 t_comm | evals w(15) coefficients(15) z s(6) selectors(6), (zeta, zeta*omega) each
 *   | ft_eval1 | u32 n, n x (L, R) | z1 z2 delta sg.
 * `out` may be NULL to query the length.  Host-side, no context. */
int mina_wrap_proof_flatten(const uint8_t *bytes, size_t len, int encoding, uint8_t *out, size_t cap, size_t *out_len, size_t *consumed /* may be NULL: exact */);
/* bincode `MinaStateProof` (core/src/proof/state_proof.rs:28-41): length of the leading proof, then where each of the 17 states sits */
int mina_state_proof_split(const uint8_t *bytes, size_t len, size_t *proof_len, size_t *state_offsets /* 17 */, size_t *state_lens /* 17 */);

/* ---- the reference-shaped boundary (README.md:275-279, 281-310, 358-362) --------------------------------
 * Same (ptr, len, ptr, len) -> bool shape as Aligned's `verify_mina_state_ffi` / `verify_account_inclusion_ffi`, fed with exactly
 * the bytes core/src/aligned.rs:31-58 produces.  Every failure is `false`; nothing unwinds; callable from any thread (one
 * process-wide context on GPU $MINA_VERIFY_DEVICE (default 0), created on first use).  Concurrent calls of the single-proof entry
 * points are merged: calls that arrive while a job runs on the GPU leave together as the next job (one proof is a 23 ms dependent
 * chain that leaves the chip idle; 256 threads calling at once see 9 k proofs/s instead of 40, each call lasting about one job).  Every caller still gets the
 * verdict of its own proof.  Batch calls of up to mina_verify_tuning.merge_batch_max (default 512) proofs share jobs with concurrent callers the same
 * way; bigger ones are pipelined on their own (chunks of 8192: parsing, uploads and the GPU job of consecutive chunks overlap; at most four jobs
 * per device in flight over all callers).  mina_verify_tuning (below): .merge = 0 sends each call through on its own; .linger_us (default 500, + 2 us per
 * caller of the previous job) bounds how long the leader of a job waits for the callers of the previous job to come back. */
#define MINA_CHECK_FORMAT 1u        /* pub inputs (1057 B) and bincode MinaStateProof parse */
#define MINA_CHECK_LEDGER 2u        /* ledger hashes of the public input == the states' snarked ledger hashes   (README.md:287) */
#define MINA_CHECK_CHAIN 4u         /* 17 state hashes == public input, states linked                          (README.md:285-288) */
#define MINA_CHECK_CONSENSUS 8u     /* candidate tip selected over the bridge tip                              (README.md:290-294) */
#define MINA_CHECK_ACCUMULATOR 16u  /* step accumulator: MSM(vesta.g, b_poly_coefficients) == challenge_polynomial_commitment */
#define MINA_CHECK_KIMCHI 32u       /* kimchi verification of the wrap proof (needs an installed verifier index) */
#define MINA_CHECK_ACCOUNT_ABI 64u  /* Proof of Account: encoded_account == ABI encoding re-derived from `account`    (README.md:349-352) */
#define MINA_CHECK_MERKLE 128u      /* Proof of Account: account hash folded along the path == ledger hash            (README.md:345-347) */
#define MINA_VERIFY_ALLOW_MISSING_KIMCHI 1u   /* verdict ignores MINA_CHECK_KIMCHI when the kimchi step cannot run: NOT a full verification */
#define MINA_VERIFY_ALLOW_UNBOUND_STATEMENT 2u /* a wrap index WITHOUT a step index: run the kimchi step with an EMPTY public input (the proof is then
                                                  not bound to the Pickles statement / the candidate tip).  Test hook; never in a deployment. */
#define MINA_VERIFY_ALLOW_SURROGATE 4u        /* verify although the installed Poseidon tables are the library's surrogate (mina_poseidon_params_name()
                                                  contains "UNPINNED"): hashes then agree with this repo's oracle, not with the Mina network.  Without the
                                                  flag every mina_verify_* verdict is `false` on such a context. */
#define MINA_VERIFY_DEDUP_STATES 8u          /* the boundary's process-wide contexts run with mina_ctx_set_state_dedup on: a chunk's state hashes are not queued
                                                  while the chunk is still being parsed; its whole state leg runs deduplicated, per chunk.  Verdicts are unchanged. */
#define MINA_VERIFY_PACK_ON_DEVICE 16u       /* the boundary's host pool does not read the protocol states: a chunk's state bytes are uploaded as they are and
                                                  mina_state_frontend_dev writes the records, field counts and `precheck` on the GPU; the state leg follows per chunk.
                                                  Off by default; verdicts and masks are unchanged.  Works together with MINA_VERIFY_DEDUP_STATES. */
#define MINA_VERIFY_ACCOUNT_ON_DEVICE 32u    /* mina_verify_account, _account_batch and _account_checks do not read a call's proofs on the host: the bytes are uploaded
                                                  as they are and mina_account_job_dev's job parses, cross-checks, hashes, folds and compares on the GPU.  Off by
                                                  default; verdicts and masks are unchanged.  A context without the device path or without Fp tables keeps the host path. */
#define MINA_VERIFY_GROUPED_SEARCH 64u       /* when a folded check of a chunk fails, its culprits are searched in groups of 64 (mina_ctx_set_search_groups) from the
                                                  chunk's staging in HBM, through mina_state_job_each_dev's body: no second upload of the chunk and, under
                                                  MINA_VERIFY_PACK_ON_DEVICE, no download of the records and `precheck` the GPU made.  Off by default; verdicts and masks
                                                  are unchanged.  Works together with the other flags.  The searches are counted on the device's context
                                                  (mina_ctx_search_stats of mina_verify_device_ctx).  Not measured on an MI355X yet (tools/bench_search.py). */
#define MINA_VERIFY_MIXED_NETWORK_JOB 128u   /* network mode with both networks ready, equal wrap domains and step programs of the same kind (csrc/net_route.h
                                                  mixed_pass_allowed): ONE pass serves the proofs of both networks that share the voted evaluation shape -- one job per
                                                  chunk, the index set chosen per proof on the GPU ("MIXED jobs", above; counted by mina_ctx_mixed_job_stats on the
                                                  device's context) -- instead of one pass per network, one after the other.  A pass whose proofs all claim one network
                                                  runs as without the flag; so does everything where the conditions do not hold.  Verdicts are unchanged: a failed folded
                                                  check goes through the culprit search on the chunk (from its device staging), a proof whose flag does not parse or whose
                                                  shape differs is treated as without the flag.  mina_verify_state_checks_batch keeps grouping by network.  Off by default. */
#include <stdbool.h>
bool mina_verify_state(const uint8_t *proof, size_t proof_len, const uint8_t *pub_input, size_t pub_len);
int mina_verify_state_batch(size_t n, const uint8_t *const *proofs, const size_t *proof_lens, const uint8_t *const *pub_inputs,
                            const size_t *pub_lens, uint8_t *verdicts_out /* n bytes 0/1 */);
/* which steps ran and which passed (bit masks of MINA_CHECK_*) */
int mina_verify_state_checks(const uint8_t *proof, size_t proof_len, const uint8_t *pub_input, size_t pub_len, uint32_t *passed_mask, uint32_t *ran_mask);
/* The same masks for n pairs at once: (passed_masks[i], ran_masks[i]) is what mina_verify_state_checks answers for pair i under the same configuration, for every
 * input, malformed ones included.  The pairs are grouped by evaluation shape; each group is parsed by the host pool (the protocol states on the GPU under
 * MINA_VERIFY_PACK_ON_DEVICE) and runs, in chunks of at most mina_verify_tuning.chunk proofs, as ONE job with all three legs through mina_state_job_checks_dev's
 * body, where the single-proof form runs three jobs per proof.  On device 0, under its lock: a checks call is not merged with other callers and not sharded over
 * several GPUs.  n = 0 is MINA_OK; a call in which no pair parses is answered without a job.  Counted by mina_ctx_checks_stats of mina_verify_device_ctx(0). */
int mina_verify_state_checks_batch(size_t n, const uint8_t *const *proofs, const size_t *proof_lens, const uint8_t *const *pub_inputs, const size_t *pub_lens,
                                   uint32_t *passed_masks /* n */, uint32_t *ran_masks /* n */);
/* the `--save-proof` files of the reference CLI (core/src/aligned.rs:60-69): mina_state.proof / mina_state.pub */
bool mina_verify_state_files(const char *proof_path, const char *pub_path);
bool mina_verify_account(const uint8_t *proof, size_t proof_len, const uint8_t *pub_input, size_t pub_len);
int mina_verify_account_batch(size_t n, const uint8_t *const *proofs, const size_t *proof_lens, const uint8_t *const *pub_inputs,
                              const size_t *pub_lens, uint8_t *verdicts_out);
bool mina_verify_account_files(const char *proof_path, const char *pub_path);   /* mina_account.proof / mina_account.pub */
/* The symbol names Aligned's operator binds (README.md:277-279, 358-362; proving-system tags `Mina` / `MinaAccount`, core/src/aligned.rs:40,53):
 * the library can be linked in place of the Rust verifier crate without a shim.  The caller passes its fixed-size buffers (48 KiB proof, 6 KiB public
 * input at the pinned revision: MINA_FFI_MAX_PROOF_SIZE / MINA_FFI_MAX_PUB_INPUT_SIZE) and the used lengths; a Proof-of-State length beyond the buffer
 * is `false` (the account entry reads `len` bytes whatever the buffer: its operator's buffer sizes are not in the tree).
 * Later Aligned versions pass the lengths as u32: the `_u32` forms.  Same semantics as mina_verify_state / mina_verify_account. */
#define MINA_FFI_MAX_PROOF_SIZE (48u * 1024u)
#define MINA_FFI_MAX_PUB_INPUT_SIZE (6u * 1024u)
bool verify_mina_state_ffi(const uint8_t *proof_buffer, size_t proof_len, const uint8_t *pub_input_buffer, size_t pub_input_len);
bool verify_account_inclusion_ffi(const uint8_t *proof_buffer, size_t proof_len, const uint8_t *pub_input_buffer, size_t pub_input_len);
bool verify_mina_state_ffi_u32(const uint8_t *proof_buffer, uint32_t proof_len, const uint8_t *pub_input_buffer, uint32_t pub_input_len);
bool verify_account_inclusion_ffi_u32(const uint8_t *proof_buffer, uint32_t proof_len, const uint8_t *pub_input_buffer, uint32_t pub_input_len);
/* ---- completion queue: submit proofs, collect verdicts later -----------------------------------------------------------
 * The entry points above block one OS thread per proof in flight.  An async caller (a tokio task, a goroutine) submits to a queue instead and takes the verdicts
 * later, from `poll`, `wait`, or when the queue's descriptor turns readable: thousands of proofs in flight from a few threads.  The queue adds no verification path
 * of its own: its workers hand their submissions to the same merged jobs the synchronous entry points feed, so a verdict is the synchronous one by construction.
 *
 * submit    copies both byte strings into storage the queue owns -- the caller may free or overwrite its buffers as soon as it returns --, never blocks on the
 *           GPU and never runs a job on the calling thread.  A null queue, an unknown `kind`, an unknown bit in `flags`, a null pointer with a non-zero length or a
 *           length above 1 MiB (the cap of the `_files` forms) is MINA_ERR_ARG and consumes no slot.  Zero lengths are legal: an empty proof is a `false` verdict,
 *           as it is for mina_verify_state.  `tag` is the caller's; it comes back in the completion.
 * slots     a submission holds one of the queue's `capacity` (1 .. 65 536) slots from `submit` until its completion has been HANDED OUT by `poll` or `wait`.  With
 *           every slot held `submit` returns MINA_ERR_FULL and changes nothing.  That is the only back-pressure: it bounds the queue's memory to `capacity` x the
 *           submitted bytes, and completions can never overflow.  A slot keeps its byte buffer: a queue in steady state stops allocating.
 * completions  one per accepted submission, exactly once, in no particular order.  `verdict` is 0 or 1; `rc` is the code the synchronous batch entry point would
 *           have returned for the job the submission rode in (MINA_OK, or e.g. MINA_ERR_HIP without a device), and the verdict is 0 whenever rc != MINA_OK.  For
 *           every input, malformed ones included, and under every mina_verify_configure flag set, `verdict` equals mina_verify_state / mina_verify_account called
 *           with the same bytes at the same moment.
 * dispatch  `workers` (1 .. 4) threads belong to the queue, created by `create` and joined by `destroy`.  A free worker takes every dispatchable submission of ONE
 *           kind, at most 8192, and passes them as one group to the merger of concurrent callers, the way mina_verify_state_batch / _account_batch pass a small
 *           batch: queue submissions merge with synchronous callers' proofs and obey mina_verify_tuning.merge, .max_jobs and .linger_us exactly as a thread calling
 *           the batch entry point with those proofs would.  While a job runs, new submissions pile up and leave together as the next job: the merger's group commit
 *           with no thread per proof.  A submission with MINA_SUBMIT_MORE is not dispatchable until a later submission of the same queue (of either kind) arrives
 *           without the flag, or `flush` or `destroy` is called: a caller that knows its burst puts it into one job.  (A burst that meets MINA_ERR_FULL must
 *           `flush`: what it holds back may be all the queue holds, and nothing else would start it.)  workers = 1 is the recommendation: the
 *           measured table (tools/bench_queue.py) shows no consistent gain from two workers or from two overlapping jobs.
 * poll / wait  `poll` never blocks; `wait` blocks until at least one completion is available or `timeout_us` has passed (negative: for ever).  Both write at most
 *           `cap` completions, set *n_out (which may be 0) and return MINA_OK unless an argument is bad (null queue or n_out, null `out` with cap > 0).
 * fd        an eventfd (non-blocking, close-on-exec) that is readable whenever completions are pending -- what a tokio `AsyncFd` or Go's netpoller registers.  The
 *           queue owns the descriptor (never close it); it is written once per finished job.  The consumer reads it (8 bytes) to clear it and then polls until
 *           *n_out == 0.  `poll` / `wait` clear it themselves when they hand out the last pending completion.
 * stats     submissions accepted, completions published (taken or not), groups the workers handed to the merger (jobs they led or joined), the largest group.
 *           Any output may be NULL.
 * threads   every call except `destroy` is safe from any number of threads at once.  `destroy` must not race with other calls on the same queue: it makes
 *           everything pending dispatchable, waits for the jobs that are running, discards completions not yet taken and frees everything.  destroy(NULL) is a no-op.
 * shutdown  a worker stands towards mina_verify_shutdown and mina_verify_install_* / _set_poseidon_params exactly where a synchronous caller thread stands: same locks,
 *           same order (g_mu, search_mu, mu), taken inside the job only.  The installers may run beside a busy queue.  mina_verify_shutdown does NOT wait for a
 *           running merged job -- it is for a process with no verification in flight --, so call it on an IDLE queue only (stats: submitted == completed); the queue
 *           stays usable afterwards, the process-wide contexts come back with the next job as they do for mina_verify_state.  Creating a queue touches no device. */
typedef struct mina_verify_queue mina_verify_queue;
typedef struct {
    uint64_t tag;       /* the submission's */
    int32_t rc;         /* MINA_OK or the job's error code */
    uint8_t verdict;    /* 0 / 1 */
    uint8_t kind;       /* MINA_QUEUE_STATE / MINA_QUEUE_ACCOUNT */
    uint8_t pad[2];
} mina_verify_completion;                        /* 16 bytes */
#define MINA_QUEUE_STATE 0u
#define MINA_QUEUE_ACCOUNT 1u
#define MINA_SUBMIT_MORE 1u      /* more submissions follow at once: do not start a job for this one yet */
#define MINA_ERR_FULL (-5)       /* the queue holds `capacity` submissions whose completions have not been taken */
int mina_verify_queue_create(uint32_t capacity, uint32_t workers, mina_verify_queue **out);
void mina_verify_queue_destroy(mina_verify_queue *q);
int mina_verify_queue_submit(mina_verify_queue *q, uint32_t kind, const uint8_t *proof, size_t proof_len, const uint8_t *pub_input, size_t pub_len, uint64_t tag,
                             uint32_t flags);
int mina_verify_queue_flush(mina_verify_queue *q);
int mina_verify_queue_poll(mina_verify_queue *q, mina_verify_completion *out, size_t cap, size_t *n_out);
int mina_verify_queue_wait(mina_verify_queue *q, mina_verify_completion *out, size_t cap, size_t *n_out, int64_t timeout_us);
int mina_verify_queue_fd(mina_verify_queue *q);
int mina_verify_queue_stats(mina_verify_queue *q, uint64_t *submitted, uint64_t *completed, uint64_t *jobs, uint64_t *max_job);
int mina_verify_account_checks(const uint8_t *proof, size_t proof_len, const uint8_t *pub_input, size_t pub_len, uint32_t *passed_mask, uint32_t *ran_mask);
/* the same on a caller-owned context (n pairs, masks per pair) */
int mina_verify_account_ctx(mina_ctx *ctx, size_t n, const uint8_t *const *proofs, const size_t *proof_lens, const uint8_t *const *pub_inputs,
                            const size_t *pub_lens, uint32_t *passed_masks, uint32_t *ran_masks);
/* serialized `MinaBaseAccountBinableArgStableV2` (bin_prot as core/src/mina.rs:307-313 reads it, or the bincode form inside
 * MinaAccountProof) -> account hashes on the GPU / the ABI bytes of sol/account.rs:25-314 (host only; out may be NULL to query the length) */
int mina_account_hash_batch(mina_ctx *ctx, int encoding, size_t n, const uint8_t *const *accounts, const size_t *lens, uint8_t *hashes_out /* n*32 */);
int mina_account_abi_encode(const uint8_t *account, size_t len, int encoding, uint8_t *out, size_t cap, size_t *out_len);
/* ---- Proof-of-Account from serialized bytes on the device (opt-in; changes NO result) --------------------------------
 * What mina_verify_account_ctx does per pair -- mina_parse_merkle_path (depth <= 64), mina_parse_account_pub_inputs, the account reader (tags in range, symbol <= 6 and
 * URI <= 255 bytes, every field element canonical, nothing behind the account), the byte comparison with mina_account_abi_encode, the four `to_input` records, the
 * account hash, the Merkle fold and the comparison with the ledger hash -- for pairs whose bytes already sit in HBM, bit-identical to the host path for every
 * input, malformed ones included.  No encoding argument: the device reads the bincode form (MINA_ENC_BINCODE) only -- the form inside `MinaAccountProof`, the only
 * one a verifier is handed; bin_prot stays with the host reader.
 * Pair i: proof = bytes [d_proof_off[i], + d_proof_len[i]) of the blob, public input = [d_pub_off[i], + d_pub_len[i]); u64 each, 8-byte aligned.  A slice that
 * reaches past blob_len is rejected, not a fault.  Device pointers; both calls queue on the next pipeline lane (the pinned one under mina_ctx_pin_lane) and do not
 * wait for the GPU (the first job of a context, or the first after mina_poseidon_set_params, prepares its salts and the default sub-hashes and waits for those).
 * A null, misaligned or inconsistent argument: MINA_ERR_ARG, before any device is touched; no Fp Poseidon tables: MINA_ERR_STATE.
 *
 * mina_account_frontend_dev: the reader alone.  d_records / d_nfields / d_salt_idx hold 4 * n entries (a record = MINA_PSTATE_SLOTS*32 bytes, 16-byte aligned; slots
 * past the field count are not written): stage s (0 zkApp URI, 1 verification key, 2 zkApp, 3 account) of entry k at [s * n + k].  The account stage is indexed by
 * the pair; the three zkApp stages by the SLOT a pair whose account carries a zkApp takes in a compacted list: d_zk_index[slot] = pair, *d_zk_count = slots taken
 * (in no particular order), d_zk_marks[i] = 1 for such a pair.  An account without a zkApp has no slot: its three sub-hashes are constants of the Poseidon tables.
 * d_siblings / d_dirs: 64 entries per pair (32 bytes / 1 byte each), d_depths[i] of them written.  d_bits[i]: MINA_CHECK_FORMAT, MINA_CHECK_ACCOUNT_ABI (only with
 * FORMAT), and 0x100 / 0x200 / 0x400 = the path / the public input / the account parsed.  A pair that fails FORMAT has field count 0 in every stage. */
int mina_account_frontend_dev(mina_ctx *ctx, size_t n, const void *d_blob, size_t blob_len, const void *d_proof_off, const void *d_proof_len, const void *d_pub_off,
                              const void *d_pub_len, void *d_records, void *d_nfields, void *d_salt_idx /* 4*n u32: index of the hash prefix */,
                              void *d_siblings /* n*64*32, 16-byte aligned */, void *d_dirs /* n*64 */, void *d_depths /* n u32 */, void *d_ledger_hashes /* n*32, 16-byte aligned */,
                              void *d_zk_marks /* n u32 */, void *d_zk_index /* n u32 */, void *d_zk_count /* 1 u32 */, void *d_bits /* n u32 */);
/* The whole job: d_passed[i] / d_ran[i] = the masks mina_verify_account_ctx returns for pair i.  d_account_hashes / d_roots (n*32 bytes each, canonical words; may be
 * NULL): the account hash and the folded root of every pair that passed FORMAT (undefined for the others).  Stream-ordered on its lane like
 * mina_state_job_batch_dev; the caller synchronises (mina_ctx_sync). */
int mina_account_job_dev(mina_ctx *ctx, size_t n, const void *d_blob, size_t blob_len, const void *d_proof_off, const void *d_proof_len, const void *d_pub_off,
                         const void *d_pub_len, void *d_passed /* n u32 */, void *d_ran /* n u32 */, void *d_account_hashes, void *d_roots);
int mina_verify_configure(uint32_t flags);       /* MINA_VERIFY_* */
/* Tuning: every knob of the library in ONE struct instead of environment switches (the defaults are the measured optima on one MI355X, DESIGN.md
 * section 5; tests force other shapes to prove the verdicts do not depend on them).  Process-wide; set it before the first verification or between
 * calls -- not while calls are in flight.  mina_verify_configure_ex(NULL) restores the defaults.  The environment is read only for deployment facts:
 * MINA_VERIFY_DEVICES / MINA_VERIFY_DEVICE (which GPUs), MINA_HOST_THREADS (parser pool), MINA_POSEIDON_PARAMS_FP / _FQ (table files),
 * MINA_VERIFY_TIMING (stderr timeline). */
typedef struct mina_verify_tuning {
    uint32_t struct_size;          /* sizeof(mina_verify_tuning), filled by mina_verify_tuning_default */
    /* bytes -> bools pipeline of mina_verify_state_batch (api_verify.hip run_device) */
    uint32_t chunk;                /* 8192  proofs per chunk of a call beyond `single_max` */
    uint32_t single_max;           /* 8192  calls up to this many proofs are ONE chunk */
    uint32_t slots;                /* 4     chunks in flight per device over all callers (<= 16) */
    uint32_t window;               /* 4     chunks of one call on the GPU at a time */
    uint32_t ahead;                /* 0     chunks parsed ahead of the window */
    uint32_t early_min;            /* 2048  chunks from this many entries are streamed: records uploaded and hashed run by run */
    uint32_t early_sub;            /* 1024  entries per run (0 = no streaming) */
    uint32_t head_min;             /* 6144  streamed chunks from this many entries parse their first run whole, ahead of everything else */
    uint32_t split_max;            /* 4     up to this many chunks in flight the three legs of a job fork onto three streams */
    uint32_t chain_cus;            /* 128   CUs of the wrap-proof chain's stream mask (the state hashes get the rest; 0 = no CU masks) */
    uint32_t cu_period;            /* 256   period of the mask pattern over the CU index */
    uint32_t acc_mask;             /* 0     accumulator leg under: 0 the chain's mask, 1 the hashes', 2 none */
    uint32_t hash_piece_waves;     /* 1024  state hashes are launched in pieces of this many waves */
    uint32_t up_stream;            /* 1     uploads on a stream of their own */
    uint32_t min_shard;            /* 64    fewer proofs per device than this: the call stays on one device */
    uint32_t pace_us;              /* 0     gap between the first `window` chunk issues of a long call */
    /* merging of concurrent single-proof / small-batch callers */
    uint32_t merge;                /* 1     0 = every call runs on its own */
    uint32_t merge_batch_max;      /* 512   batch calls up to this size join merged jobs */
    uint32_t linger_us;            /* 500   how long a job's leader waits for the previous job's callers to come back */
    uint32_t max_jobs;             /* 1     merged jobs overlapping on the device */
    /* lane forms of the Poseidon kernels: sponges (or proofs) in flight up to which the 16- / 8-lane latency forms are used */
    uint32_t coop16_max;           /* 64 */
    uint32_t coop8_max;            /* 8192 */
    uint32_t coop8_per_call;       /* 0     1 = the limits look at one call, not at calls x lanes in flight */
    uint32_t transcript_coop8_max; /* 0     0 = built-in rule (ctx.h use_coop8_transcripts) */
    uint32_t ipa_coop8_max;        /* 1024 */
    uint32_t kimchi_coop8_max;     /* 1024 */
    /* shortcuts, each with a slower equivalent path kept for cross-checking */
    uint32_t bpoly_mfma;           /* 1     b_poly fold of batches >= 256 on the matrix cores (0: VALU fold) */
    uint32_t pubcomm_direct;       /* 1     public-input commitments by digit-table lookups (0: bucket MSM) */
    uint32_t ipa_shared_points;    /* 1     batch-shared points of the opening check enter the MSM once */
    uint32_t kimchi_shared_digest; /* 1     kimchi's challenge digest taken from the statement's sponge */
    uint32_t ipa_side_stream;      /* 1     U = to_group(t) beside the transcript on a second stream */
    uint32_t search_fan;           /* 4     fan-out of the culprit search (2 .. 32) */
    uint32_t search_full;          /* 0     1 = every part of a culprit search repeats its transcripts */
    uint32_t msm_fp29;             /* 1     SRS-table MSMs accumulate their buckets on 29-bit limbs: 1 = points gathered from the 64-byte twin table (8 x 32 words in the 2^261 domain),
                                            2 = from the pre-split 128-byte records (x, y, p - y as 29-bit limbs: no conversion, no negation, twice the gather traffic; needs mina_srs_split_table),
                                            3 = as 1, and in the multi-MSM form the buckets STAY on 29-bit limbs through the 2-D bucket reduction; 0: the 8 x 32-bit law */
    uint32_t search_ctx;           /* 1     the culprit search of a failed chunk runs on a SECOND context of its device (its own lanes, workspaces and lock): valid traffic keeps
                                            flowing beside it.  0 = round 4: on the device's one context, with the device drained and its lock held for the length of the search */
    /* device-resident jobs (mina_state_job_batch_dev): the three independent legs of ONE job -- protocol-state hashes / wrap-proof chain / accumulator -- on streams
     * of their own, joined before the verdict kernel, so that a few jobs in flight fill the chip (round 6; until then one stream per job and ~20 jobs in flight) */
    uint32_t dev_fork;             /* 1     bit 0: fork the legs (pipelines of up to 8 lanes; a pinned lane and mina_state_job_fold_dev fork as well: fork and join are events on the lane's stream); bit 1: the chain's and the hashes' streams get disjoint CU masks (`dev_chain_cus`);
                                            bit 2: the wrap-proof chain's stream is created with the highest stream priority, the hashes' with the lowest */
    uint32_t dev_chain_cus;        /* 96    CUs of the chain's mask when bit 1 of dev_fork is set */
    uint32_t dev_piece_waves;      /* 0     a forked job's state hashes are launched in pieces of this many waves; 0 = 6144 / pipeline lanes (whole for a lone lane), 0xffffffff = never */
    uint32_t dev_hash_lds_kb;      /* 0     KiB of LDS a forked job's state-hash workgroup reserves (33 = four waves per SIMD instead of five, 41 = three: room for the waves of the other legs);
                                            0 = 41 for a lone lane, none with several lanes; 0xffffffff = never */
    uint32_t dev_acc_lane;         /* 0     the accumulator leg of a forked job: 0 = on a stream of its own, 1 = on the hashes' stream behind them, 2 = on the hashes' stream ahead of them */
} mina_verify_tuning;
void mina_verify_tuning_default(mina_verify_tuning *out);
int mina_verify_tuning_get(mina_verify_tuning *out);
int mina_verify_configure_ex(const mina_verify_tuning *tuning);
/* How many RETIRED tuning environment variables (MINA_VERIFY_CHUNK, MINA_VERIFY_NO_MERGE, MINA_COOP8_MAX ... -- the switches of rounds 1 - 3, now fields of
 * mina_verify_tuning) the process environment still sets.  They are not read; the library says so once on stderr when it is loaded, naming the field that
 * replaces each.  A strict deployment checks this for 0 at start-up. */
int mina_verify_retired_env(void);
int mina_verify_shutdown(void);                  /* destroy the process-wide contexts */
mina_ctx *mina_verify_global_ctx(void);          /* the first device's context, e.g. to install a verifier index; NULL without a GPU.  Installing through this handle with the
                                                    kernel-level installers (mina_verifier_index_install, mina_srs_*, mina_poseidon_set_params ...) takes none of the boundary's locks: do it
                                                    BEFORE the first mina_verify_* call only.  While verification calls may be in flight use the mina_verify_install_* / mina_verify_set_*
                                                    functions below: they serialise against running jobs and culprit searches (lock order g_mu, search_mu, mu) on every device. */
/* Multi-GPU behind the boundary: the process holds one context per GPU named by $MINA_VERIFY_DEVICES ("all" | comma list of
 * ordinals; an ordinal may repeat = several logical contexts on one GPU; default: $MINA_VERIFY_DEVICE or 0).  mina_verify_state_batch cuts
 * its proofs into contiguous shards, one per device, each with its own folding randomisers and its own culprit search; merged single-proof
 * jobs are dealt round-robin.  The installers below put the same data on EVERY device. */
/* which network the installed indexes belong to: 0 = mainnet, 1 = devnet, -1 (default) = not declared.  Once declared, a proof whose public
 * input claims the other network (`is_state_proof_from_devnet`, core/src/proof/state_proof.rs:10-25) fails the kimchi step.
 * This is the form for a process that holds ONE index pair.  A process that serves both networks installs a pair per network instead
 * (mina_verify_install_verifier_index_net / mina_verify_install_step_index_net, below); in that mode this call returns MINA_ERR_STATE and changes nothing. */
int mina_verify_set_network(int devnet);
int mina_verify_device_count(void);
mina_ctx *mina_verify_device_ctx(int i);
int mina_verify_install_verifier_index(const mina_verifier_index *index);
int mina_verify_install_step_index(const mina_step_index *index);
/* An index pair PER NETWORK (the reference verifier picks the devnet or the mainnet blockchain-snark index per proof, by `is_state_proof_from_devnet`).
 * The `_net` installers write index set `devnet` (0 = mainnet, 1 = devnet; mina_ctx_select_index_set) on EVERY device, under the locks of the installers above.
 * The first successful one puts the process into NETWORK MODE; mina_verify_drop_network_indexes (which empties both sets) and mina_verify_shutdown end it.
 * In network mode, for every Proof-of-State entry point (mina_verify_state, _files, _batch, _checks, _checks_batch, verify_mina_state_ffi, the completion queue):
 *   - a proof's network is the parsed flag of its public input, and its kimchi step runs against the set of that network;
 *   - if that set lacks what a full configuration needs (a wrap index, plus a step index unless MINA_VERIFY_ALLOW_UNBOUND_STATEMENT), the proof is rejected as a
 *     wrong-network proof is under mina_verify_set_network: KIMCHI is in `ran` and not in `passed`, CHAIN and ACCUMULATOR keep their own bits, no other verdict changes;
 *   - the proofs of one call are verified network by network, one pass after the other (the majority network first), as proofs of different evaluation shapes are;
 *   - mina_verify_set_network, mina_verify_install_verifier_index and mina_verify_install_step_index return MINA_ERR_STATE and change nothing.
 * A `_net` call while a network is declared (mina_verify_set_network(0 | 1)) returns MINA_ERR_STATE: a process declares one network or installs per network,
 * never both.  devnet outside {0, 1} or a null index: MINA_ERR_ARG, before any device is touched.  Outside network mode nothing changes.
 * mina_verify_networks: which networks are ready (1) -- hold a full configuration -- on the first device; (0, 0) outside network mode; either pointer may be NULL.
 * Proof-of-Account carries no network flag and is not affected. */
int mina_verify_install_verifier_index_net(int devnet, const mina_verifier_index *index);
int mina_verify_install_step_index_net(int devnet, const mina_step_index *index);
int mina_verify_drop_network_indexes(void);
int mina_verify_networks(int *mainnet_ready, int *devnet_ready);
int mina_verify_set_poseidon_params(int field, const uint8_t *params /* (9+165)*32 */);
/* the Poseidon constant set compiled into the library (name contains "UNPINNED" while it is a surrogate for fp_kimchi/fq_kimchi) */
const char *mina_poseidon_params_name(void);
int mina_poseidon_install_default_params(mina_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* MINA_VERIFY_H */
