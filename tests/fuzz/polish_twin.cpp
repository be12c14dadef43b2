// The validator and the host interpreter of PolishToken programs (mina_bridge_amd/csrc/polish.h: decode_tokens, polish_eval_host) on programs handed in by
// tests/test_polish_programs.py: the header the product compiles, built for the host with the stand-in runtime header of this directory (hip_stub), once plainly and
// once with -fsanitize=address,undefined -fno-sanitize-recover=all.  The sanitized build is the check that a program the validator accepts keeps the interpreter's
// stack[KC_STACK] and cache[KC_CACHE] in bounds under every feature mask; the values are compared with tests/polish_model.py by the test.
//
//   polish_twin IN OUT
//   IN:  sections, until the end of the file:
//          u32 field, ncols, log2_domain, zk_rows, slots, n_evals, code_len, n_masks
//          5 x 8 words of FieldK (one, r2, pm2, tm1d2, root)
//          the environment, plain canonical 8-word values: alpha, beta, gamma, endo, zkpm, zeta, zeta^n, omega, joint combiner, 9 x mds, n_evals x 2 evaluations
//          code_len bytes of byte-code, padded with zeros to a multiple of 4
//          n_masks x (u32 feature mask, u32 presence mask)
//        a section whose field has bit 8 set holds its 8 header words and its byte-code only: FieldK, the environment and the masks are the previous section's
//   OUT: per section u32 accepted; if accepted, per mask u32 verdict and the 8 words of the value (plain; zeros where the verdict is 0)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mina_bridge_amd/csrc/polish.h"

using namespace mb;

template <int F> static bool run(const FieldK &fk, const uint32_t *head, const std::vector<uint32_t> &envw, const std::vector<uint8_t> &code, const std::vector<uint32_t> &masks, std::vector<uint32_t> &out) {
    const uint32_t ncols = head[1], n_evals = head[5], n_masks = head[7];
    std::vector<KimchiToken> toks; std::vector<std::array<uint8_t, 32>> lits8;
    const bool accepted = decode_tokens(code.data(), code.size(), F, ncols, toks, lits8);
    out.push_back(accepted ? 1u : 0u);
    if (!accepted) return true;
    auto fe_at = [&](size_t i) { fe_t w; for (int j = 0; j < 8; ++j) w.v[j] = envw[i * 8 + j]; return fe_to_mont<F>(w, fk.r2); };
    std::vector<fe_t> lits;
    for (const auto &l : lits8) { fe_t w; memcpy(w.v, l.data(), 32); lits.push_back(fe_to_mont<F>(w, fk.r2)); }
    fe_t mds[9]; for (int i = 0; i < 9; ++i) mds[i] = fe_at(9 + i);
    std::vector<std::array<fe_t, 2>> evals(n_evals);
    for (uint32_t c = 0; c < n_evals; ++c) evals[c] = {fe_at(18 + 2 * c), fe_at(18 + 2 * c + 1)};
    PolishEnv<F> env{fe_at(0), fe_at(1), fe_at(2), fe_at(3), fe_at(4), fe_at(5), fe_at(6), fe_at(7), mds, head[2], head[3], &evals};
    env.joint_combiner = fe_at(8); env.slots = head[4] != 0;
    for (uint32_t m = 0; m < n_masks; ++m) {
        env.features = masks[2 * m]; env.present = masks[2 * m + 1];
        fe_t v = fe_zero();
        const bool ok = polish_eval_host<F>(toks, lits, env, fk, v);
        out.push_back(ok ? 1u : 0u);
        const fe_t plain = ok ? fe_from_mont<F>(v) : fe_zero();
        for (int j = 0; j < 8; ++j) out.push_back(plain.v[j]);
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: polish_twin IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *outf = fopen(argv[2], "wb");
    if (!in || !outf) return 2;
    uint32_t head[8];
    std::vector<uint32_t> out, envw, masks;
    FieldK fk = {};
    uint32_t prev[8] = {~0u};
    while (fread(head, 4, 8, in) == 8) {
        const bool reuse = (head[0] & 0x100u) != 0;
        head[0] &= ~0x100u;
        const uint32_t field = head[0], n_evals = head[5], code_len = head[6], n_masks = head[7];
        if (reuse && (head[0] != prev[0] || head[5] != prev[5] || head[7] != prev[7])) return 3;
        memcpy(prev, head, sizeof prev);
        if (field > 1 || n_evals > 64 || code_len > (1u << 24) || n_masks > (1u << 16) || head[2] < 1 || head[2] > 24 || head[3] < 1 || head[3] > 8) return 3;
        std::vector<uint8_t> code((code_len + 3) / 4 * 4);
        if (!reuse) {
            uint32_t consts[40];
            if (fread(consts, 4, 40, in) != 40) return 3;
            fe_t *dst[5] = {&fk.one, &fk.r2, &fk.pm2, &fk.tm1d2, &fk.root};
            for (int c = 0; c < 5; ++c) for (int i = 0; i < 8; ++i) dst[c]->v[i] = consts[c * 8 + i];
            envw.assign((size_t)(18 + 2 * n_evals) * 8, 0u);
            if (fread(envw.data(), 4, envw.size(), in) != envw.size()) return 3;
        }
        if (!code.empty() && fread(code.data(), 1, code.size(), in) != code.size()) return 3;
        if (!reuse) {
            masks.assign((size_t)n_masks * 2, 0u);
            if (!masks.empty() && fread(masks.data(), 4, masks.size(), in) != masks.size()) return 3;
        }
        code.resize(code_len);                                     // the pad is not the validator's to see
        code.shrink_to_fit();                                      // nor to read: AddressSanitizer guards the end of the allocation
        const bool ok = field == 0 ? run<FIELD_FP>(fk, head, envw, code, masks, out) : run<FIELD_FQ>(fk, head, envw, code, masks, out);
        if (!ok) return 4;
    }
    fclose(in);
    if (!out.empty() && fwrite(out.data(), 4, out.size(), outf) != out.size()) return 5;
    return fclose(outf) == 0 ? 0 : 5;
}
