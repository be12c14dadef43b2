// api_selftest.hip -- the test-facing entry points of the two field layers (mina_selftest_fe32 for fp.cuh / ec.cuh: second half of this file).  The 9 x 29-bit layer
// (fp29.cuh, ec29.cuh): mina_selftest_fe29 runs ONE routine -- a generated product, a limb-wise
// form, a whole group law -- on rows of caller-chosen limbs and hands back the raw limbs it produced.  The parity tests reach these routines only through composite
// kernels, on the values those kernels happen to meet; tests/test_gpu_fe29.py feeds them the corner inputs of tools/fe29_bounds.py instead.  Nothing here is on a
// job's path, and nothing is range-checked on the device: the CALLER owns the operand bounds (a product fed operands beyond what fe29_bounds.py proves wraps its
// accumulator silently -- that is what the hook is for finding out about).
//
// One kernel instantiation per <field, op>: each holds one routine in straight-line code, every operand slot a compile-time index -- no scratch.  One thread per row,
// except fe29_row1_sg, whose a0, a1 and c are wave-uniform by contract (they ride the constant bus as SGPR operands): its rows run one per workgroup, every lane on
// the same row, lane 0 stores.
#include "ctx.h"
#include "ec29.cuh"
#include "groupmap.cuh"

static constexpr uint32_t FE29_IN_WORDS = MINA_FE29_IN_OPERANDS * 9 + 1, FE29_OUT_WORDS = MINA_FE29_OUT_RESULTS * 9 + 1;

#define FE29_OPS(X)                                                                                                                                                  \
    X(MINA_FE29_MUL_ASM) X(MINA_FE29_SQR_ASM) X(MINA_FE29_DOT2_ASM) X(MINA_FE29_DOT3_ASM) X(MINA_FE29_SQR_HI_ASM) X(MINA_FE29_MUL_HI_ASM)                            \
    X(MINA_FE29_MUL_LZ) X(MINA_FE29_SQR_LZ) X(MINA_FE29_MUL_HI_LZ) X(MINA_FE29_MULRC_LZ) X(MINA_FE29_DOT2RC_LZ) X(MINA_FE29_DOT3RC_LZ)                               \
    X(MINA_FE29_MUL_SG) X(MINA_FE29_SQR_SG) X(MINA_FE29_MUL_HI_SG) X(MINA_FE29_SQR_HI_SG) X(MINA_FE29_MULRC_SG) X(MINA_FE29_DOT2RC_SG) X(MINA_FE29_DOT3RC_SG)        \
    X(MINA_FE29_ROW1_SG)                                                                                                                                             \
    X(MINA_FE29_SUB_KP_ONE) X(MINA_FE29_KP_MINUS_NEG_Y) X(MINA_FE29_KP_MINUS_SUB_X1) X(MINA_FE29_KP_MINUS_SUB_Y1) X(MINA_FE29_KP_MINUS_G_U1) X(MINA_FE29_KP_MINUS_G_S1) \
    X(MINA_FE29_KP_MINUS_A_2B_X3_SUB) X(MINA_FE29_KP_MINUS_A_2B_G_X3_SUB) X(MINA_FE29_ADD_KP_MINUS_SUB_X3) X(MINA_FE29_ADD_KP_MINUS_G_SUB_X3)                        \
    X(MINA_FE29_ADD) X(MINA_FE29_ADD3) X(MINA_FE29_WORDS) X(MINA_FE29_IS_MULTIPLE_OF_P) X(MINA_FE29_LEAVE)                                                           \
    X(MINA_FE29_ADD_AFFINE) X(MINA_FE29_ADD_AFFINE_TWIN) X(MINA_FE29_XYZZ_ADD) X(MINA_FE29_XYZZ_LEAVE)

template <int F, int OP>
__global__ void __launch_bounds__(64)
fe29_selftest_kernel(uint32_t n, fe_t one, fe_t m32, const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t row = OP == MINA_FE29_ROW1_SG ? blockIdx.x : blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const uint32_t *w = in + (size_t)row * FE29_IN_WORDS;
    fe29_t s[MINA_FE29_IN_OPERANDS], o[MINA_FE29_OUT_RESULTS];
#pragma unroll
    for (int k = 0; k < MINA_FE29_IN_OPERANDS; ++k)
#pragma unroll
        for (int i = 0; i < L29; ++i) s[k].v[i] = w[k * L29 + i];
    const uint32_t flag = w[FE29_IN_WORDS - 1];
#pragma unroll
    for (int k = 0; k < MINA_FE29_OUT_RESULTS; ++k) o[k] = fe29_zero();
    uint32_t oflag = 0;
    auto words_out = [&](int k, const fe_t &x) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[k].v[i] = x.v[i];
    };
    // products: the pairs in slots 0 .. 5, c (added before the reduction) in slot 6, h / t (added to the high half) in slot 7
    if constexpr (OP == MINA_FE29_MUL_ASM) o[0] = fe29_mul_asm<F>(s[0], s[1]);
    else if constexpr (OP == MINA_FE29_SQR_ASM) o[0] = fe29_sqr_asm<F>(s[0]);
    else if constexpr (OP == MINA_FE29_DOT2_ASM) o[0] = fe29_dot2_asm<F>(s[0], s[1], s[2], s[3]);
    else if constexpr (OP == MINA_FE29_DOT3_ASM) o[0] = fe29_dot3_asm<F>(s[0], s[1], s[2], s[3], s[4], s[5]);
    else if constexpr (OP == MINA_FE29_SQR_HI_ASM) o[0] = fe29_sqr_hi_asm<F>(s[0], s[7]);
    else if constexpr (OP == MINA_FE29_MUL_HI_ASM) o[0] = fe29_mul_hi_asm<F>(s[0], s[1], s[7]);
    else if constexpr (OP == MINA_FE29_MUL_LZ) o[0] = fe29_mul_lz<F>(s[0], s[1]);
    else if constexpr (OP == MINA_FE29_SQR_LZ) o[0] = fe29_sqr_lz<F>(s[0]);
    else if constexpr (OP == MINA_FE29_MUL_HI_LZ) o[0] = fe29_mul_hi_lz<F>(s[0], s[1], s[7]);
    else if constexpr (OP == MINA_FE29_MULRC_LZ) o[0] = fe29_mulrc_lz<F>(s[0], s[1], s[6]);
    else if constexpr (OP == MINA_FE29_DOT2RC_LZ) o[0] = fe29_dot2rc_lz<F>(s[0], s[1], s[2], s[3], s[6]);
    else if constexpr (OP == MINA_FE29_DOT3RC_LZ) o[0] = fe29_dot3rc_lz<F>(s[0], s[1], s[2], s[3], s[4], s[5], s[6]);
    else if constexpr (OP == MINA_FE29_MUL_SG) o[0] = fe29_mul_sg<F>(s[0], s[1]);
    else if constexpr (OP == MINA_FE29_SQR_SG) o[0] = fe29_sqr_sg<F>(s[0]);
    else if constexpr (OP == MINA_FE29_MUL_HI_SG) o[0] = fe29_mul_hi_sg<F>(s[0], s[1], s[7]);
    else if constexpr (OP == MINA_FE29_SQR_HI_SG) o[0] = fe29_sqr_hi_sg<F>(s[0], s[7]);
    else if constexpr (OP == MINA_FE29_MULRC_SG) o[0] = fe29_mulrc_sg<F>(s[0], s[1], s[6]);
    else if constexpr (OP == MINA_FE29_DOT2RC_SG) o[0] = fe29_dot2rc_sg<F>(s[0], s[1], s[2], s[3], s[6]);
    else if constexpr (OP == MINA_FE29_DOT3RC_SG) o[0] = fe29_dot3rc_sg<F>(s[0], s[1], s[2], s[3], s[4], s[5], s[6]);
    else if constexpr (OP == MINA_FE29_ROW1_SG) o[0] = fe29_row1_sg<F>(s[7], s[0], s[1], s[2], s[3], s[6]);
    // the limb-wise forms, in the instantiations the group laws use
    else if constexpr (OP == MINA_FE29_SUB_KP_ONE) o[0] = fe29_sub_kp<F, 1>(s[0], s[1]);
    else if constexpr (OP == MINA_FE29_KP_MINUS_NEG_Y) o[0] = fe29_kp_minus<F, EC29::NEG_Y_MULT>(s[0]);
    else if constexpr (OP == MINA_FE29_KP_MINUS_SUB_X1) o[0] = fe29_kp_minus<F, EC29::SUB_X1_MULT>(s[0]);
    else if constexpr (OP == MINA_FE29_KP_MINUS_SUB_Y1) o[0] = fe29_kp_minus<F, EC29::SUB_Y1_MULT>(s[0]);
    else if constexpr (OP == MINA_FE29_KP_MINUS_G_U1) o[0] = fe29_kp_minus<F, EC29::G_U1_MULT>(s[0]);
    else if constexpr (OP == MINA_FE29_KP_MINUS_G_S1) o[0] = fe29_kp_minus<F, EC29::G_S1_MULT>(s[0]);
    else if constexpr (OP == MINA_FE29_KP_MINUS_A_2B_X3_SUB) o[0] = fe29_kp_minus_a_minus_2b<F, EC29::X3_SUB_MULT>(s[0], s[1]);
    else if constexpr (OP == MINA_FE29_KP_MINUS_A_2B_G_X3_SUB) o[0] = fe29_kp_minus_a_minus_2b<F, EC29::G_X3_SUB_MULT>(s[0], s[1]);
    else if constexpr (OP == MINA_FE29_ADD_KP_MINUS_SUB_X3) o[0] = fe29_add_kp_minus<F, EC29::SUB_X3_MULT>(s[0], s[1]);
    else if constexpr (OP == MINA_FE29_ADD_KP_MINUS_G_SUB_X3) o[0] = fe29_add_kp_minus<F, EC29::G_SUB_X3_MULT>(s[0], s[1]);
    else if constexpr (OP == MINA_FE29_ADD) o[0] = fe29_add(s[0], s[1]);
    else if constexpr (OP == MINA_FE29_ADD3) o[0] = fe29_add3(s[0], s[1], s[2]);
    else if constexpr (OP == MINA_FE29_WORDS) {                  // slot 0: eight 32-bit words -> the nine limbs, and the words made of them again
        fe_t x;
#pragma unroll
        for (int i = 0; i < 8; ++i) x.v[i] = s[0].v[i];
        o[0] = fe29_from_words(x); words_out(1, fe29_to_words(o[0]));
    }
    else if constexpr (OP == MINA_FE29_IS_MULTIPLE_OF_P) oflag = fe29_is_multiple_of_p<F>(s[0]) ? 1u : 0u;
    else if constexpr (OP == MINA_FE29_LEAVE) words_out(0, fe29_leave<F>(s[0], fe29_from_words(one)));
    // the laws whole: accumulator in slots 0 .. 3 (x, y, zz, zzz)
    else {
        xyzz29_t acc; acc.x = s[0]; acc.y = s[1]; acc.zz = s[2]; acc.zzz = s[3];
        bool inf = (flag & MINA_FE29_FLAG_INF) != 0, ok = true;
        if constexpr (OP == MINA_FE29_ADD_AFFINE) { inf = false; ok = xyzz29_add_affine<F>(acc, inf, s[4], s[5], [&]() { return s[5]; }, []() {}, m32); }
        else if constexpr (OP == MINA_FE29_ADD_AFFINE_TWIN) ok = xyzz29_add_affine<F>(acc, inf, s[4], s[5], (flag & MINA_FE29_FLAG_NEG) != 0, m32);
        else if constexpr (OP == MINA_FE29_XYZZ_ADD) { xyzz29_t b; b.x = s[4]; b.y = s[5]; b.zz = s[6]; b.zzz = s[7]; inf = false; ok = xyzz29_add<F>(acc, b); }
        else static_assert(OP == MINA_FE29_XYZZ_LEAVE, "unknown op");
        if constexpr (OP == MINA_FE29_XYZZ_LEAVE) {
            const xyzz_t v = xyzz29_leave<F>(acc, inf, one);
            words_out(0, v.x); words_out(1, v.y); words_out(2, v.zz); words_out(3, v.zzz);
        } else { o[0] = acc.x; o[1] = acc.y; o[2] = acc.zz; o[3] = acc.zzz; }
        oflag = (ok ? MINA_FE29_FLAG_OK : 0u) | (inf ? MINA_FE29_FLAG_INF : 0u);
    }
    if (OP == MINA_FE29_ROW1_SG && threadIdx.x != 0) return;
    uint32_t *dst = out + (size_t)row * FE29_OUT_WORDS;
#pragma unroll
    for (int k = 0; k < MINA_FE29_OUT_RESULTS; ++k)
#pragma unroll
        for (int i = 0; i < L29; ++i) dst[k * L29 + i] = o[k].v[i];
    dst[FE29_OUT_WORDS - 1] = oflag;
#endif
}

static bool fe29_known_op(int op) {
    switch (op) {
#define X(o) case o:
        FE29_OPS(X)
#undef X
        return true;
    default: return false;
    }
}

template <int F> static void fe29_selftest_launch(int op, uint32_t blocks, hipStream_t st, uint32_t n, const FieldK &fk, const uint32_t *in, uint32_t *out) {
    switch (op) {
#define X(o) case o: fe29_selftest_kernel<F, o><<<blocks, 64, 0, st>>>(n, fk.one, fk.m32, in, out); break;
        FE29_OPS(X)
#undef X
    }
}

extern "C" int mina_selftest_fe29(mina_ctx *c, int field, int op, size_t n, const uint32_t *in, uint32_t *out) {
    if (!c || (n && (!in || !out))) return fail(MINA_ERR_ARG, "null argument");
    if (bad_field(field)) return fail(MINA_ERR_ARG, "bad field");
    if (!fe29_known_op(op)) return fail(MINA_ERR_ARG, "bad op");
    if (n > (1u << 22)) return fail(MINA_ERR_ARG, "more than 2^22 rows");
    if (n == 0) return MINA_OK;
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = h2d(c, c->L->tmp_a, in, n * FE29_IN_WORDS * 4))) return rc;
    if ((rc = c->L->tmp_c.ensure(n * FE29_OUT_WORDS * 4))) return rc;
    const uint32_t blocks = op == MINA_FE29_ROW1_SG ? (uint32_t)n : cdiv(n, 64);
    DISPATCH_FIELD(field, { fe29_selftest_launch<F_>(op, blocks, c->L->stream, (uint32_t)n, c->fk[F_], c->L->tmp_a.as<uint32_t>(), c->L->tmp_c.as<uint32_t>()); });
    return d2h_sync(c, out, c->L->tmp_c, n * FE29_OUT_WORDS * 4);
}

// ------------------------------------------------------------------------------------------------
// mina_selftest_fe32: the same hook for the 8 x 32 layer -- the inline-assembly carry chains and generated products of fp.cuh, fe_inv / fe_sqrt of groupmap.cuh, the
// group laws of ec.cuh -- which carries everything the 29-bit forms do not: the redo queues of the MSM, every transcript and scalar, b_poly, the codec, every `leave`.
// Raw words in, raw words out: no Montgomery conversion, no range check -- the caller owns each routine's contract (tests/fe32_model.py states them).  One kernel per
// <field, op>, one thread per row; the lane-cooperative laws run four lanes per row on identical operands, lane 0 stores, and one flag bit says whether the four
// lanes ended with identical words.
static constexpr uint32_t FE32_IN_WORDS = MINA_FE32_IN_OPERANDS * 8 + 1, FE32_OUT_WORDS = MINA_FE32_OUT_RESULTS * 8 + 1;

#define FE32_OPS(X)                                                                                                                                                  \
    X(MINA_FE32_COND_SUB_P) X(MINA_FE32_ADD) X(MINA_FE32_SUB) X(MINA_FE32_NEG) X(MINA_FE32_DBL) X(MINA_FE32_MUL) X(MINA_FE32_SQR) X(MINA_FE32_DOT2) X(MINA_FE32_DOT3)    \
    X(MINA_FE32_TO_MONT) X(MINA_FE32_FROM_MONT) X(MINA_FE32_INV) X(MINA_FE32_SQRT) X(MINA_FE32_WORDS_CANONICAL)                                                      \
    X(MINA_FE32_DBL_AFFINE) X(MINA_FE32_XYZZ_DBL) X(MINA_FE32_ADD_AFFINE) X(MINA_FE32_XYZZ_ADD) X(MINA_FE32_XYZZ_DBL_QUAD) X(MINA_FE32_XYZZ_ADD_QUAD)

static constexpr bool fe32_is_quad(int op) { return op == MINA_FE32_XYZZ_DBL_QUAD || op == MINA_FE32_XYZZ_ADD_QUAD; }

template <int F, int OP>
__global__ void __launch_bounds__(64)
fe32_selftest_kernel(uint32_t n, FieldK fk, const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr bool QUAD = fe32_is_quad(OP);
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, row = QUAD ? gid >> 2 : gid;
    if (row >= n) return;                                      // a quad shares its row: it leaves whole or not at all
    const uint32_t *w = in + (size_t)row * FE32_IN_WORDS;
    fe_t s[MINA_FE32_IN_OPERANDS], o[MINA_FE32_OUT_RESULTS];
#pragma unroll
    for (int k = 0; k < MINA_FE32_IN_OPERANDS; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) s[k].v[i] = w[k * 8 + i];
#pragma unroll
    for (int k = 0; k < MINA_FE32_OUT_RESULTS; ++k) o[k] = fe_zero();
    uint32_t oflag = 0;
    if constexpr (OP == MINA_FE32_COND_SUB_P) o[0] = fe_cond_sub_p<F>(s[0]);
    else if constexpr (OP == MINA_FE32_ADD) o[0] = fe_add<F>(s[0], s[1]);
    else if constexpr (OP == MINA_FE32_SUB) o[0] = fe_sub<F>(s[0], s[1]);
    else if constexpr (OP == MINA_FE32_NEG) o[0] = fe_neg<F>(s[0]);
    else if constexpr (OP == MINA_FE32_DBL) o[0] = fe_dbl<F>(s[0]);
    else if constexpr (OP == MINA_FE32_MUL) o[0] = fe_mul<F>(s[0], s[1]);
    else if constexpr (OP == MINA_FE32_SQR) o[0] = fe_sqr<F>(s[0]);
    else if constexpr (OP == MINA_FE32_DOT2) o[0] = fe_dot2<F>(s[0], s[1], s[2], s[3]);
    else if constexpr (OP == MINA_FE32_DOT3) o[0] = fe_dot3<F>(s[0], s[1], s[2], s[3], s[4], s[5]);
    else if constexpr (OP == MINA_FE32_TO_MONT) o[0] = fe_to_mont<F>(s[0], fk.r2);
    else if constexpr (OP == MINA_FE32_FROM_MONT) o[0] = fe_from_mont<F>(s[0]);
    else if constexpr (OP == MINA_FE32_INV) o[0] = fe_inv<F>(s[0], fk);
    else if constexpr (OP == MINA_FE32_SQRT) { fe_t r = fe_zero(); if (fe_sqrt<F>(r, s[0], fk)) { o[0] = r; oflag = MINA_FE32_FLAG_TRUE; } }
    else if constexpr (OP == MINA_FE32_WORDS_CANONICAL) oflag = fe_words_canonical<F>(s[0]) ? MINA_FE32_FLAG_TRUE : 0u;
    else {
        xyzz_t acc; acc.x = s[0]; acc.y = s[1]; acc.zz = s[2]; acc.zzz = s[3];
        xyzz_t q; q.x = s[4]; q.y = s[5]; q.zz = s[6]; q.zzz = s[7];
        if constexpr (OP == MINA_FE32_DBL_AFFINE) acc = xyzz_dbl_affine<F>(s[0], s[1]);
        else if constexpr (OP == MINA_FE32_XYZZ_DBL) acc = xyzz_dbl<F>(acc);
        else if constexpr (OP == MINA_FE32_ADD_AFFINE) xyzz_add_affine<F>(acc, s[4], s[5], fk.one);
        else if constexpr (OP == MINA_FE32_XYZZ_ADD) xyzz_add<F>(acc, q);
        else if constexpr (OP == MINA_FE32_XYZZ_DBL_QUAD) acc = xyzz_dbl_quad<F>(acc);
        else { static_assert(OP == MINA_FE32_XYZZ_ADD_QUAD, "unknown op"); xyzz_add_quad<F>(acc, q); }
        o[0] = acc.x; o[1] = acc.y; o[2] = acc.zz; o[3] = acc.zzz;
        if constexpr (QUAD) {                                  // every lane against lane 0's words, then the four verdicts gathered on every lane
            uint32_t d = 0;
#pragma unroll
            for (int k = 0; k < MINA_FE32_OUT_RESULTS; ++k) { const fe_t l0 = quad_bcast<0>(o[k]);
#pragma unroll
                for (int i = 0; i < 8; ++i) d |= o[k].v[i] ^ l0.v[i]; }
            const int differs = d != 0;
            const int any = __builtin_amdgcn_mov_dpp(differs, 0x00, 0xf, 0xf, true) | __builtin_amdgcn_mov_dpp(differs, 0x55, 0xf, 0xf, true) |
                            __builtin_amdgcn_mov_dpp(differs, 0xaa, 0xf, 0xf, true) | __builtin_amdgcn_mov_dpp(differs, 0xff, 0xf, 0xf, true);
            oflag = any ? 0u : MINA_FE32_FLAG_LANES_AGREE;
            if ((gid & 3u) != 0) return;
        }
    }
    uint32_t *dst = out + (size_t)row * FE32_OUT_WORDS;
#pragma unroll
    for (int k = 0; k < MINA_FE32_OUT_RESULTS; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[k * 8 + i] = o[k].v[i];
    dst[FE32_OUT_WORDS - 1] = oflag;
#endif
}

static bool fe32_known_op(int op) {
    switch (op) {
#define X(o) case o:
        FE32_OPS(X)
#undef X
        return true;
    default: return false;
    }
}

template <int F> static void fe32_selftest_launch(int op, hipStream_t st, uint32_t n, const FieldK &fk, const uint32_t *in, uint32_t *out) {
    switch (op) {
#define X(o) case o: fe32_selftest_kernel<F, o><<<cdiv(fe32_is_quad(o) ? (size_t)n * 4 : n, 64), 64, 0, st>>>(n, fk, in, out); break;
        FE32_OPS(X)
#undef X
    }
}

extern "C" int mina_selftest_fe32(mina_ctx *c, int field, int op, size_t n, const uint32_t *in, uint32_t *out) {
    if (!c || (n && (!in || !out))) return fail(MINA_ERR_ARG, "null argument");
    if (bad_field(field)) return fail(MINA_ERR_ARG, "bad field");
    if (!fe32_known_op(op)) return fail(MINA_ERR_ARG, "bad op");
    if (n > (1u << 22)) return fail(MINA_ERR_ARG, "more than 2^22 rows");
    if (n == 0) return MINA_OK;
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = h2d(c, c->L->tmp_a, in, n * FE32_IN_WORDS * 4))) return rc;
    if ((rc = c->L->tmp_c.ensure(n * FE32_OUT_WORDS * 4))) return rc;
    DISPATCH_FIELD(field, { fe32_selftest_launch<F_>(op, c->L->stream, (uint32_t)n, c->fk[F_], c->L->tmp_a.as<uint32_t>(), c->L->tmp_c.as<uint32_t>()); });
    return d2h_sync(c, out, c->L->tmp_c, n * FE32_OUT_WORDS * 4);
}
