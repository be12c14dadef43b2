// The PORTABLE forms of the 8 x 32 layer (mina_bridge_amd/csrc/fp.cuh `*_portable`, ec.cuh, fe_inv / fe_sqrt of groupmap.cuh) on the rows of mina_selftest_fe32: the same
// headers the gfx950 kernels are compiled from, built for the host with the stand-in runtime header of this directory (hip_stub) -- where fe_add, fe_sub, fe_mul resolve
// to the CIOS / loop forms and fe_dot2 / fe_dot3 to sums of products.  tests/test_fe32_rows.py builds it with the C++ compiler (once more with
// -fsanitize=address,undefined), feeds it every row of tests/fe32_model.py and demands the model's words back: the device path (inline assembly, tests/test_gpu_fe32.py)
// and this path are then both pinned to the same big-integer contract.  The lane-cooperative laws exist on the device only: their ops run the single-lane law here and
// report "lanes agree".
//
//   fe32_twin IN OUT
//   IN:  sections, until the end of the file: u32 field, u32 op, u32 n; 5 x 8 words of FieldK (one, r2, pm2, tm1d2, root); n rows of 65 words
//   OUT: per section n rows of 33 words
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../include/mina_verify.h"
#include "../../mina_bridge_amd/csrc/groupmap.cuh"

using namespace mb;

static const uint32_t IN_WORDS = MINA_FE32_IN_OPERANDS * 8 + 1, OUT_WORDS = MINA_FE32_OUT_RESULTS * 8 + 1;

template <int F> static bool run_row(int op, const FieldK &fk, const uint32_t *w, uint32_t *dst) {
    fe_t s[MINA_FE32_IN_OPERANDS], o[MINA_FE32_OUT_RESULTS];
    for (int k = 0; k < MINA_FE32_IN_OPERANDS; ++k) for (int i = 0; i < 8; ++i) s[k].v[i] = w[k * 8 + i];
    for (int k = 0; k < MINA_FE32_OUT_RESULTS; ++k) o[k] = fe_zero();
    uint32_t oflag = 0;
    xyzz_t acc; acc.x = s[0]; acc.y = s[1]; acc.zz = s[2]; acc.zzz = s[3];
    xyzz_t q; q.x = s[4]; q.y = s[5]; q.zz = s[6]; q.zzz = s[7];
    bool law = false;
    switch (op) {
    case MINA_FE32_COND_SUB_P: o[0] = fe_cond_sub_p<F>(s[0]); break;
    case MINA_FE32_ADD: o[0] = fe_add<F>(s[0], s[1]); break;
    case MINA_FE32_SUB: o[0] = fe_sub<F>(s[0], s[1]); break;
    case MINA_FE32_NEG: o[0] = fe_neg<F>(s[0]); break;
    case MINA_FE32_DBL: o[0] = fe_dbl<F>(s[0]); break;
    case MINA_FE32_MUL: o[0] = fe_mul<F>(s[0], s[1]); break;
    case MINA_FE32_SQR: o[0] = fe_sqr<F>(s[0]); break;
    case MINA_FE32_DOT2: o[0] = fe_dot2<F>(s[0], s[1], s[2], s[3]); break;
    case MINA_FE32_DOT3: o[0] = fe_dot3<F>(s[0], s[1], s[2], s[3], s[4], s[5]); break;
    case MINA_FE32_TO_MONT: o[0] = fe_to_mont<F>(s[0], fk.r2); break;
    case MINA_FE32_FROM_MONT: o[0] = fe_from_mont<F>(s[0]); break;
    case MINA_FE32_INV: o[0] = fe_inv<F>(s[0], fk); break;
    case MINA_FE32_SQRT: { fe_t r = fe_zero(); if (fe_sqrt<F>(r, s[0], fk)) { o[0] = r; oflag = MINA_FE32_FLAG_TRUE; } break; }
    case MINA_FE32_WORDS_CANONICAL: oflag = fe_words_canonical<F>(s[0]) ? MINA_FE32_FLAG_TRUE : 0u; break;
    case MINA_FE32_DBL_AFFINE: acc = xyzz_dbl_affine<F>(s[0], s[1]); law = true; break;
    case MINA_FE32_XYZZ_DBL_QUAD: oflag = MINA_FE32_FLAG_LANES_AGREE;   // fall through
    case MINA_FE32_XYZZ_DBL: acc = xyzz_dbl<F>(acc); law = true; break;
    case MINA_FE32_ADD_AFFINE: xyzz_add_affine<F>(acc, s[4], s[5], fk.one); law = true; break;
    case MINA_FE32_XYZZ_ADD_QUAD: oflag = MINA_FE32_FLAG_LANES_AGREE;   // fall through
    case MINA_FE32_XYZZ_ADD: xyzz_add<F>(acc, q); law = true; break;
    default: return false;
    }
    if (law) { o[0] = acc.x; o[1] = acc.y; o[2] = acc.zz; o[3] = acc.zzz; }
    for (int k = 0; k < MINA_FE32_OUT_RESULTS; ++k) for (int i = 0; i < 8; ++i) dst[k * 8 + i] = o[k].v[i];
    dst[OUT_WORDS - 1] = oflag;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: fe32_twin IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t head[3];
    while (fread(head, 4, 3, in) == 3) {
        const uint32_t field = head[0], op = head[1], n = head[2];
        if (field > 1 || n > (1u << 22)) return 3;
        uint32_t consts[40];
        if (fread(consts, 4, 40, in) != 40) return 3;
        FieldK fk = {};
        fe_t *dst[5] = {&fk.one, &fk.r2, &fk.pm2, &fk.tm1d2, &fk.root};
        for (int c = 0; c < 5; ++c) for (int i = 0; i < 8; ++i) dst[c]->v[i] = consts[c * 8 + i];
        std::vector<uint32_t> rows((size_t)n * IN_WORDS), res((size_t)n * OUT_WORDS, 0u);
        if (n && fread(rows.data(), 4, rows.size(), in) != rows.size()) return 3;
        for (uint32_t i = 0; i < n; ++i) {
            const bool ok = field == 0 ? run_row<FIELD_FP>((int)op, fk, &rows[(size_t)i * IN_WORDS], &res[(size_t)i * OUT_WORDS])
                                       : run_row<FIELD_FQ>((int)op, fk, &rows[(size_t)i * IN_WORDS], &res[(size_t)i * OUT_WORDS]);
            if (!ok) return 4;
        }
        if (n && fwrite(res.data(), 4, res.size(), out) != res.size()) return 5;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 5;
}
