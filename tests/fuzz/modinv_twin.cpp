// The divstep inversion (mina_bridge_amd/csrc/fe_modinv.cuh) beside the Fermat one (groupmap.cuh fe_inv) on the host: the same header the gfx950 kernels are
// compiled from, built with the C++ compiler through the stand-in runtime header of this directory (hip_stub).  tests/test_modinv_host.py builds it twice -- the
// second time with -fsanitize=address,undefined -fno-sanitize-recover=all -- feeds it the rows of tests/modinv_model.py and demands that the two columns agree,
// that they are Python's pow, and that the limbs at the end of every batch are the model's.
//
//   modinv_twin IN OUT
//   IN:  u32 n, u32 ntrace (<= n); then per field (Fp, Fq): 3 x 8 words of FieldK (one, r2, pm2) and n rows of 8 words (Montgomery words below p)
//   OUT: per field: n rows of 16 words (fe_inv_gcd, fe_inv); then for each of the first ntrace rows 1 + 25 * 37 words: the number of batches that ran, and per
//        batch delta and the nine limbs of f, g, d, e (signed, as 32-bit words; zero for the batches that did not run)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../mina_bridge_amd/csrc/fe_modinv.cuh"

using namespace mb;

static const int TRACE_WORDS = 1 + MI_BATCHES * 37;

struct Recorder {
    int32_t *out;                                  // TRACE_WORDS
    void operator()(int b, int32_t delta, const mi30_t &f, const mi30_t &g, const mi30_t &d, const mi30_t &e) const {
        int32_t *row = out + 1 + b * 37;
        out[0] = b + 1;
        row[0] = delta;
        for (int i = 0; i < 9; ++i) { row[1 + i] = f.v[i]; row[10 + i] = g.v[i]; row[19 + i] = d.v[i]; row[28 + i] = e.v[i]; }
    }
};

template <int F> static bool run_field(FILE *in, uint32_t n, uint32_t ntrace, FILE *out) {
    uint32_t consts[24];
    std::vector<uint32_t> rows((size_t)n * 8);
    if (fread(consts, 4, 24, in) != 24 || (n && fread(rows.data(), 4, rows.size(), in) != rows.size())) return false;
    FieldK fk = {};
    fe_t *dst[3] = {&fk.one, &fk.r2, &fk.pm2};
    for (int c = 0; c < 3; ++c) for (int i = 0; i < 8; ++i) dst[c]->v[i] = consts[c * 8 + i];
    std::vector<uint32_t> res((size_t)n * 16);
    std::vector<int32_t> trace((size_t)ntrace * TRACE_WORDS, 0);
    for (uint32_t r = 0; r < n; ++r) {
        fe_t a;
        for (int i = 0; i < 8; ++i) a.v[i] = rows[(size_t)r * 8 + i];
        const fe_t x = fe_inv_gcd<F>(a, fk), y = fe_inv<F>(a, fk);
        for (int i = 0; i < 8; ++i) { res[(size_t)r * 16 + i] = x.v[i]; res[(size_t)r * 16 + 8 + i] = y.v[i]; }
        if (r < ntrace) (void)mi_inverse_words<F>(a, Recorder{&trace[(size_t)r * TRACE_WORDS]});
    }
    if (n && fwrite(res.data(), 4, res.size(), out) != res.size()) return false;
    if (ntrace && fwrite(trace.data(), 4, trace.size(), out) != trace.size()) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: modinv_twin IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t head[2];
    if (fread(head, 4, 2, in) != 2 || head[0] > (1u << 20) || head[1] > head[0]) return 3;
    if (!run_field<FIELD_FP>(in, head[0], head[1], out)) return 4;
    if (!run_field<FIELD_FQ>(in, head[0], head[1], out)) return 4;
    fclose(in);
    return fclose(out) == 0 ? 0 : 5;
}
